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
fused multiply-add: nothing contracts.

The maps of tests/map_cases.py (NEW_MAPS; its docstring: which limit of the index format each one reaches) run
through the same program.  No older build recorded them, so there is no image hash: the flags and counts
must equal the table the GPU tests rely on (map_cases.expected), and the image must be sound in itself --
every candidate, band and live entry an edge id below n_vert, every group pointer and band range inside the
n_idx entries of the index, every mixed-cell record's span inside the n_live entries, frank the prefix
popcount of the class words."""
import functools
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import map_cases as mc
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


@pytest.mark.parametrize("real_size", [4, 8])
@pytest.mark.parametrize("name", mc.NEW_MAPS)
def test_new_maps_reach_their_paths_with_sound_images(program, name, real_size):
    meta, image = _built(program, name)[real_size]
    want = mc.expected(name, real_size)
    assert {k: meta[k] for k in want} == want
    assert len(image) == meta["size"] and meta["map_bytes"] <= meta["ring_off"] <= meta["bbox_off"] <= meta["size"]
    nv, n_idx, n_mixed, n_live = meta["n_vert"], meta["n_idx"], meta["n_mixed"], meta["n_live"]
    esz = 48 if real_size == 8 else 32          # Edge<T>: five reals and the polygon id, 16-byte aligned
    real = np.float32 if real_size == 4 else np.float64
    edges = np.frombuffer(image, dtype=np.uint8, count=nv * esz).reshape(nv, esz)
    poly = edges[:, 5 * real_size:5 * real_size + 4].copy().view(np.uint32).ravel()
    offs, verts = _map_file(name)
    assert np.array_equal(poly, np.repeat(np.arange(meta["n_poly"]), np.diff(offs)))
    assert np.array_equal(edges[:, :2 * real_size].copy().view(real).reshape(nv, 2), verts.astype(real))
    idx = np.frombuffer(image, dtype=np.uint16, count=n_idx, offset=meta["idx_off"]).astype(np.int64)
    if meta["use_index"]:
        rec = idx[:mc.K_BAND_BASE].reshape(-1, 4)
        first_ids = np.stack([rec[:, 0] & 0xff, rec[:, 0] >> 8, rec[:, 1] & 0xff, rec[:, 1] >> 8, rec[:, 2] & 0xff], 1)
        assert first_ids.max() < nv
        more, ptr = rec[:, 2] >> 8, rec[:, 3]
        starts = idx[mc.K_BAND_BASE:mc.K_IDX_HEAD]
        assert starts[0] == mc.K_IDX_HEAD and (np.diff(starts) >= 0).all() and starts[-1] <= n_idx
        gbase = (starts[-1] + 3) & ~3
        assert idx[mc.K_IDX_HEAD:starts[-1]].max() < nv                        # band entries: edge ids
        assert (4 * ptr >= gbase).all() and (4 * (ptr + more) <= n_idx).all()     # further groups: inside idx
        assert 4 * (ptr + more).max() == n_idx and (n_idx - gbase) == 4 * more.sum()
        grp = idx[gbase:].reshape(-1, 4)
        if len(grp):                                                              # 5 u8 ids in 8 bytes
            assert max((grp[:, :2] >> 8).max(), (grp[:, :3] & 0xff).max()) < nv
            assert not grp[:, 3].any() and not (grp[:, 2] >> 8).any()
    else:
        assert n_idx == 4 and not idx.any()                                       # the placeholder pf_cell reads
    fine = np.frombuffer(image, dtype=np.uint32, count=mc.K_FINE * mc.K_FINE // 16, offset=meta["fine_off"])
    cls = (fine[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3    # [word, cell in word]
    assert cls.max() == 2 and int((cls == 2).sum()) == n_mixed
    if meta["use_cells"]:
        assert n_mixed <= 65535 and n_live <= 65535
        frank = np.frombuffer(image, dtype=np.uint16, count=len(fine), offset=meta["frank_off"])
        per_word = (cls == 2).sum(axis=1)
        assert np.array_equal(frank, np.concatenate([[0], np.cumsum(per_word)[:-1]]))
        crec = np.frombuffer(image, dtype=np.uint32, count=2 * n_mixed, offset=meta["crec_off"]).reshape(-1, 2)
        first, cnt = (crec[:, 1] & 0xffff).astype(np.int64), (crec[:, 1] >> 16).astype(np.int64)
        assert (first + cnt <= n_live).all() and first[0] == 0 and np.array_equal(first[1:], np.cumsum(cnt)[:-1] & 0xffff)
        assert not (crec[:, 0] >> np.uint32(meta["n_poly"] - 1) >> np.uint32(1)).any()   # parity bits of real rings only
        clive = np.frombuffer(image, dtype=np.uint8, count=n_live, offset=meta["clive_off"])
        assert int(clive.max()) < nv
        assert meta["clive_off"] + n_live <= meta["map_bytes"]
    else:
        assert meta["frank_off"] <= meta["crec_off"] == meta["clive_off"] <= meta["map_bytes"] < meta["frank_off"] + 256 + 8


def test_new_maps_set_what_they_are_for(program):
    """Parity bit 31 in squares32's records; tens of further groups in comb_dense; negative grid origins in
    shifted; a clockwise ring in nested."""
    meta, image = _built(program, "squares32")[8]
    crec = np.frombuffer(image, dtype=np.uint32, count=2 * meta["n_mixed"], offset=meta["crec_off"]).reshape(-1, 2)
    assert (crec[:, 0] >> np.uint32(31)).any()
    meta, image = _built(program, "comb_dense")[8]
    idx = np.frombuffer(image, dtype=np.uint16, count=meta["n_idx"], offset=meta["idx_off"])
    assert (idx[2:mc.K_BAND_BASE:4] >> 8).max() >= 20
    meta, _ = _built(program, "shifted")[8]
    assert max(float.fromhex(meta[k]) for k in ("gx0", "gy0", "fx0", "fy0", "by0", "max_e", "max_n")) < 0

    def area(r):
        return 0.5 * float(np.sum(r[:, 0] * np.roll(r[:, 1], -1) - np.roll(r[:, 0], -1) * r[:, 1]))
    assert [area(r) > 0 for r in mc.load("nested")] == [True, True, True, False]
