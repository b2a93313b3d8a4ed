"""The host map builder (csrc/sit_map_build.h) under ASan + UBSan, bit for bit against the images
the library built before the builder left sit_load_map.

tests/csrc/map_build_main.cpp includes only sit_map_build.h.  It is compiled here with the host
compiler (-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all) and run as a child
process; nothing is preloaded and nothing is loaded into Python.

Maps (tests/golden/map_<name>.txt: n_poly, offsets, (east, north) vertices as hex floats), the
smallest that reach every path of the builder:
  scenario         the four islands of the scenario (helpers.POLYS)
  triangle         n_poly = 1, three vertices
  repeated_vertex  a square whose second vertex is repeated: a zero-length edge (il2 = 0, the
                   l2 > 0 guards)
  gon256           a regular 256-gon of 3 km radius: edge ids up to 255 in the u8 packing, cells near
                   its centre with far more than five candidates (further groups: more > 0, grest)

Expectations (tests/golden/map_images.json): per map and real size the SHA-256 of the image and
every MapMeta field, doubles as C "%a" strings -- equality, no tolerance.  They were recorded
from the commit before this builder existed, not from the code under test: in a scratch copy of
that commit, sit_load_map got a throwaway dump (when SIT_DUMP_MAP is set: `host` to that file and
the handle's map fields, the doubles printed with %a, as JSON beside it); the copy's
sit_kernels.hip was compiled alone at -O3 with -DSIT_HOST_MEMORY_TEST and no sanitizer, and driven
through SIT_LIBRARY and ctypes (sit_create, sit_load_map, sit_map_info for "lds_bytes") on a
machine without a GPU.  That commit accepted all four maps (use_index = use_cells = 1 for each).
The sanitizer build at -O1 and the -O3 library agree because the baseline x86-64 target has no
fused multiply-add: nothing contracts."""
import functools
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, POLYS, ROOT

MAPS = ("scenario", "triangle", "repeated_vertex", "gon256")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _host_compiler():
    for cand in (os.environ.get("SIT_HOST_CXX"), "/opt/rocm/llvm/bin/clang++", "g++"):
        if cand and (os.path.exists(cand) if os.path.sep in cand else shutil.which(cand)):
            return cand
    return None


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (ROCm's clang++ or g++) to build tests/csrc/map_build_main.cpp")
    exe = str(tmp_path_factory.mktemp("map_build") / "map_build_main")
    subprocess.run([cxx, *FLAGS, "-I", os.path.join(ROOT, "sac_maritime_ast_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "map_build_main.cpp"), "-o", exe], check=True)
    return exe


@functools.lru_cache(maxsize=None)
def _built(exe, name):
    """{real size: (meta dict, image bytes)} of one run of the program on a map."""
    prefix = os.path.join(os.path.dirname(exe), name)
    r = subprocess.run([exe, os.path.join(GOLDEN, f"map_{name}.txt"), prefix], capture_output=True, text=True)
    assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stderr[-4000:]}"
    out = {}
    for line in r.stdout.splitlines():
        meta = json.loads(line)
        with open(f"{prefix}.{meta['real_size']}.bin", "rb") as f:
            out[meta["real_size"]] = (meta, f.read())
    return out


@functools.lru_cache(maxsize=None)
def golden_images():
    with open(os.path.join(GOLDEN, "map_images.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("real_size", [4, 8])
@pytest.mark.parametrize("name", MAPS)
def test_image_and_meta_match_the_recorded_build(program, name, real_size):
    meta, image = _built(program, name)[real_size]
    want = dict(golden_images()[name][str(real_size)])
    assert len(image) == meta["size"] == want["size"]
    assert hashlib.sha256(image).hexdigest() == want.pop("sha256")
    want.pop("lds_bytes")   # sit_map_info's, not a MapMeta field (tests/test_abi_host.py)
    assert meta == want


def _map_file(name):
    with open(os.path.join(GOLDEN, f"map_{name}.txt")) as f:
        tok = f.read().split()
    n = int(tok[0])
    return [int(t) for t in tok[1:n + 2]], np.array([float.fromhex(t) for t in tok[n + 2:]]).reshape(-1, 2)


def test_map_files_hold_the_maps_the_docstring_names():
    offs, verts = _map_file("scenario")
    assert offs == [0, *np.cumsum([len(p) for p in POLYS])] and np.array_equal(verts, np.concatenate(POLYS))
    offs, verts = _map_file("repeated_vertex")
    assert offs == [0, 5] and np.array_equal(verts[1], verts[2])
    offs, verts = _map_file("gon256")
    assert offs == [0, 256]


def test_maps_reach_the_paths_the_scenario_never_takes(program):
    """Further groups per grid cell (y bits 8-15 of a cell record, sit_map_format.h): at most one in
    the scenario's image, many in the 256-gon's, whose largest ids reach 255; the repeated vertex's
    zero-length edge carries il2 = 0."""
    grid, band_base, head = 32, 4 * 32 * 32, 4 * 32 * 32 + 64 + 1   # kGrid, kBandBase, kIdxHead

    def index(name):
        meta, image = _built(program, name)[8]
        idx = np.frombuffer(image, dtype=np.uint16, count=meta["n_idx"], offset=meta["idx_off"])
        return idx, idx[2:4 * grid * grid:4] >> 8   # the u16 index, further groups per cell
    idx, more = index("scenario")
    assert more.max() <= 1
    idx, more = index("gon256")
    assert more.max() >= 10 and idx[head:idx[band_base + 64]].max() == 255   # band entries: edge ids
    meta, image = _built(program, "repeated_vertex")[8]
    edges = np.frombuffer(image, dtype=np.float64, count=6 * meta["n_vert"]).reshape(-1, 6)   # Edge<double>: 48 bytes
    assert np.array_equal(edges[1, :2], edges[1, 2:4]) and edges[1, 4] == 0.0 and np.all(np.delete(edges[:, 4], 1) > 0)
