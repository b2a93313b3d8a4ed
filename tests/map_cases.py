"""The island maps the map tests share (tests/test_gpu_map_paths.py, test_gpu_debug.py, test_map_build_host.py):
the fixtures tests/golden/map_<name>.txt (written by tests/golden/make_map_fixtures.py; triangle,
repeated_vertex and gon256 are the older ones of test_map_build_host.py), what the host builder makes of each,
probe points that reach every path of the device predicates, and the oracle's answers in chunks.  A plain
module over numpy and the oracle: nothing here needs a GPU.

What each map is for (sit_map_format.h, sit_device.h):
  comb_v      256 edges that all span every band: the packed index exceeds 48 KB, use_index = 0, full scans with
              the ring bounding boxes (point_in_polys, distance_to_polys); the one-wave step kernel
  comb_h      use_index = 1 but > 65535 live-edge entries: use_cells = 0, band scans (pip_indexed,
              pip_pair_indexed)
  comb_corner use_index = 0 with use_cells = 1: a tall narrow comb in a corner of a 30 km extent, whose far grid
              cells list most of its 248 edges (the further groups exceed 48 KB) while few class cells are mixed:
              full-scan distance, mixed-cell records for containment
  star128     comb_h's path with 4.7 km diagonals through one centre: long candidate lists, long bands
  comb_h64    use_cells = 1 with a 260 KB image: larger than a CU's LDS, fused launches fall back to the one-wave
              kernel reading the map from global memory
  squares32   32 rings (parity bit 31), horizontal and vertical edges only, an image between the one-wave
              kernel's 80 KB LDS budget and the two-wave kernel's
  comb_dense  ~27 live edges per mixed cell, up to tens of further candidate groups per grid cell
  nested      a ring inside a ring, two overlapping rings, a clockwise ring
  shifted     the scenario's islands at negative coordinates (every grid-origin subtraction)
  triangle / repeated_vertex / gon256   three edges; a zero-length edge (il2 = 0); ids up to 255"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

from helpers import GOLDEN
from oracle import sit_oracle as so

HALF = 40.0           # l/2 of the reference ship (test_policy.py ShipConfiguration length 80 m)
K_GRID, K_BANDS, K_FINE = 32, 64, 256     # kGrid, kBands, kFine (sit_map_format.h)
K_BAND_BASE, K_IDX_HEAD = 4 * K_GRID * K_GRID, 4 * K_GRID * K_GRID + K_BANDS + 1
CHUNK = 20_000        # oracle points per call: its broadcast temporaries are points x edges

NEW_MAPS = ("comb_v", "comb_h", "comb_h64", "comb_dense", "comb_corner", "star128", "squares32", "nested", "shifted")
OLD_MAPS = ("triangle", "repeated_vertex", "gon256")
MAPS = NEW_MAPS + OLD_MAPS
STEP_MAPS = ("comb_v", "comb_h", "comb_h64", "squares32")      # the maps that change the step kernels' dispatch

# what build_map_image makes of the new maps: (n_poly, n_vert, use_index, use_cells, n_idx, n_mixed, n_live,
# map_bytes float32, map_bytes float64), from the host builder alone (the older three: map_images.json)
_BUILT = {
    "comb_v":     (1, 256, 0, 0, 4, 39312, 108931, 24832, 28928),
    "comb_h":     (1, 256, 1, 0, 10480, 39312, 100927, 45568, 49664),
    "comb_h64":   (1, 128, 1, 1, 7304, 21906, 41776, 260608, 262656),
    "comb_dense": (3, 256, 1, 1, 17996, 304, 8360, 79872, 83968),
    "comb_corner": (3, 256, 0, 1, 4, 266, 22250, 57600, 61696),
    "star128":    (1, 256, 1, 0, 14892, 23240, 93512, 54528, 58624),
    "squares32":  (32, 128, 1, 1, 4832, 3981, 10065, 80384, 82432),
    "nested":     (4, 16, 1, 1, 4340, 1830, 2149, 50688, 50944),
    "shifted":    (4, 39, 1, 1, 4420, 1960, 2416, 52992, 53760),
}


@functools.lru_cache(maxsize=None)
def expected(name: str, real_size: int) -> dict:
    """MapMeta fields the builder must produce for a map (real_size 4 or 8)."""
    keys = ("n_poly", "n_vert", "use_index", "use_cells", "n_idx", "n_mixed", "n_live", "map_bytes")
    if name in _BUILT:
        b = _BUILT[name]
        return dict(zip(keys, (*b[:7], b[7 if real_size == 4 else 8])))
    with open(os.path.join(GOLDEN, "map_images.json")) as f:
        rec = json.load(f)[name][str(real_size)]
    return {k: rec[k] for k in keys}


@functools.lru_cache(maxsize=None)
def load(name: str) -> tuple:
    """The rings of tests/golden/map_<name>.txt as float64[m, 2] (east, north) arrays."""
    with open(os.path.join(GOLDEN, f"map_{name}.txt")) as f:
        tok = f.read().split()
    n = int(tok[0])
    offs = [int(t) for t in tok[1:n + 2]]
    verts = np.array([float.fromhex(t) for t in tok[n + 2:]]).reshape(-1, 2)
    assert len(verts) == offs[-1]
    return tuple(verts[a:b] for a, b in zip(offs[:-1], offs[1:]))


def extent(polys):
    v = np.concatenate(polys)
    return v[:, 0].min(), v[:, 0].max(), v[:, 1].min(), v[:, 1].max()     # min_e, max_e, min_n, max_n


def longest_edge(polys) -> float:
    return max(float(np.hypot(*(np.roll(r, -1, axis=0) - r).T).max()) for r in polys)


def lattices(polys) -> dict:
    """The cell lines of the three lattices with build_map_image's formulas: name -> (east lines, north lines);
    the bands have north lines only."""
    min_e, max_e, min_n, max_n = extent(polys)
    ext_x, ext_y = max_e - min_e, max_n - min_n
    mg = 0.1 * max(ext_x, ext_y) + 500.0
    sx, sy = (ext_x + 2 * mg) / K_GRID, (ext_y + 2 * mg) / K_GRID
    fsx, fsy = (ext_x + 200.0) / K_FINE, (ext_y + 200.0) / K_FINE
    bh = (ext_y + 2.0) / K_BANDS
    return {"grid": (min_e - mg + np.arange(K_GRID + 1) * sx, min_n - mg + np.arange(K_GRID + 1) * sy),
            "class": (min_e - 100.0 + np.arange(K_FINE + 1) * fsx, min_n - 100.0 + np.arange(K_FINE + 1) * fsy),
            "band": (np.zeros(0), min_n - 1.0 + np.arange(K_BANDS + 1) * bh)}


def _around(x):
    """x, its float64 neighbours and the float32 values around it (a float32 handle sees only those)."""
    f = x.astype(np.float32)
    lo32 = np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f)
    hi32 = np.nextafter(lo32, np.float32(np.inf))
    return np.concatenate([x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf), lo32.astype(np.float64),
                           hi32.astype(np.float64), np.nextafter(lo32, np.float32(-np.inf)).astype(np.float64),
                           np.nextafter(hi32, np.float32(np.inf)).astype(np.float64)])


@functools.lru_cache(maxsize=None)
def probe_points(name: str, seed: int = 7) -> np.ndarray:
    """About 40 000 (north, east) points of a map, float64 (module docstring of test_gpu_map_paths.py)."""
    polys = load(name)
    rng = np.random.default_rng(seed)
    min_e, max_e, min_n, max_n = extent(polys)
    lo_e, hi_e, lo_n, hi_n = min_e - 3000.0, max_e + 3000.0, min_n - 3000.0, max_n + 3000.0
    # uniform: inside the class grid, between its 100 m and the candidate grid's margin, beyond both
    pts = [np.stack([rng.uniform(lo_n, hi_n, 12_000), rng.uniform(lo_e, hi_e, 12_000)], 1)]
    n_edge = sum(len(r) for r in polys)
    m = int(np.clip(16_000 // n_edge, 60, 1000))          # band points per edge
    for ring in polys:
        for (ax, ay), (bx, by) in zip(ring, np.roll(ring, -1, axis=0)):
            ex, ey = bx - ax, by - ay
            L = np.hypot(ex, ey)
            pts.append(np.array([[ay, ax], [(ay + by) / 2, (ax + bx) / 2]]))          # vertex, midpoint
            # rays through the vertex latitude (horizontal-ray degeneracies), left and right
            xs = np.concatenate([rng.uniform(lo_e, hi_e, 4), [ax - 1.0, ax + 1.0, ax - 1e-7, ax + 1e-7]])
            pts.append(np.stack([np.full(xs.shape, ay), xs], 1))
            # hull corners landing exactly on the vertex
            pts.append(np.array([[ay + s1 * HALF, ax + s2 * HALF] for s1 in (-1, 1) for s2 in (-1, 1)]))
            if L == 0:
                continue
            t = rng.uniform(0, 1, m)
            nx, ny = -ey / L, ex / L
            off = np.exp(rng.uniform(np.log(1e-9), np.log(80.0), m)) * rng.choice([-1.0, 1.0], m)
            pts.append(np.stack([ay + t * ey + off * ny, ax + t * ex + off * nx], 1))
        # points in (and around) every ring
        e0, n0, e1, n1 = ring[:, 0].min(), ring[:, 1].min(), ring[:, 0].max(), ring[:, 1].max()
        pts.append(np.stack([rng.uniform(n0 - 1, n1 + 1, 60), rng.uniform(e0 - 1, e1 + 1, 60)], 1))
    # on and one ulp (float64 and float32) either side of every cell line of the three lattices, the outermost
    # included; the other coordinate anywhere, and for the class grid also on a line of its own
    for key, k in (("grid", 4), ("class", 3), ("band", 4)):
        e_lines, n_lines = lattices(polys)[key]
        if len(e_lines):
            x = _around(np.repeat(e_lines, k))
            pts.append(np.stack([rng.uniform(min_n - 200, max_n + 200, len(x)), x], 1))
        y = _around(np.repeat(n_lines, k))
        pts.append(np.stack([y, rng.uniform(min_e - 200, max_e + 200, len(y))], 1))
    e_lines, n_lines = lattices(polys)["class"]
    i, j = rng.integers(0, K_FINE + 1, 100), rng.integers(0, K_FINE + 1, 100)
    pts.append(np.stack([_around(n_lines[j]), _around(e_lines[i])], 1))
    return np.concatenate(pts)


def _chunks(fn, polys, n, e):
    return np.concatenate([fn(polys, n[k:k + CHUNK], e[k:k + CHUNK]) for k in range(0, len(n), CHUNK)])


def oracle_distance(polys, n, e):
    return _chunks(so.distance_to_polygons, polys, np.asarray(n, np.float64).ravel(), np.asarray(e, np.float64).ravel())


def oracle_inside(polys, n, e):
    return _chunks(so.point_in_polygons, polys, np.asarray(n, np.float64).ravel(), np.asarray(e, np.float64).ravel())


def oracle_predicates(polys, pts):
    """(distance, contains, four-corner hull test) of (north, east) points."""
    polys = list(polys)
    n, e = pts[:, 0], pts[:, 1]
    hull = np.zeros(len(n), bool)
    for s1 in (-1, 1):
        for s2 in (-1, 1):
            hull |= oracle_inside(polys, n + s1 * HALF, e + s2 * HALF)
    return oracle_distance(polys, n, e), oracle_inside(polys, n, e), hull


def corner_margin(polys, n, e):
    """Smallest boundary distance over a point and its four hull corners."""
    polys = list(polys)
    m = oracle_distance(polys, n, e)
    for s1 in (-1, 1):
        for s2 in (-1, 1):
            m = np.minimum(m, oracle_distance(polys, n + s1 * HALF, e + s2 * HALF))
    return m
