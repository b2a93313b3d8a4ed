#!/usr/bin/env python3
"""Write the island maps that reach every path of the spatial index (tests/map_cases.py lists what
each one is for) as tests/golden/map_<name>.txt: n_poly, the n_poly + 1 vertex offsets, then
(east, north) per vertex as C hex floats -- the format of tests/csrc/map_build_main.cpp.

Every coordinate is a whole metre below 2^17 in magnitude, so a float32 handle and a float64 handle
hold the same polygons.

    python tests/golden/make_map_fixtures.py
"""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def zig(n, W, H, w, vertical):
    """A zigzag strip of 2 n vertices: n teeth along x (vertical: the teeth stand upright) or along y,
    and the same chain back, shifted by w across the teeth's direction.  A translated function graph
    cannot cross itself, so the ring is simple."""
    i = np.arange(n)
    if vertical:
        fwd = np.stack([i * W / (n - 1), (i % 2) * H], 1)
        back = fwd[::-1] + [0.0, w]
    else:
        fwd = np.stack([(i % 2) * W, i * H / (n - 1)], 1)
        back = fwd[::-1] + [w, 0.0]
    return np.rint(np.concatenate([fwd, back]))


def square(e0, n0, side, clockwise=False):
    ring = np.array([[e0, n0], [e0 + side, n0], [e0 + side, n0 + side], [e0, n0 + side]], dtype=np.float64)
    return ring[::-1].copy() if clockwise else ring


def star(spikes, r_in, r_out, ce, cn):
    k = np.arange(2 * spikes)
    r = np.where(k % 2 == 0, r_out, r_in)
    a = 2 * math.pi * k / (2 * spikes)
    return np.rint(np.stack([ce + r * np.cos(a), cn + r * np.sin(a)], 1))


def squares32():
    """27 squares of 950 m, three of 500 m (rings 29 to 31) and two of 2 m that pin the extent to
    (0, 0)-(10000, 10000).  The scenario's ships start at (east, north) = (500, 1200) and (5300, 2200),
    jittered by +-100 m, and make about 300 m in 300 steps: the test ship to the south-east, the obstacle
    ship to the north-west.  The lattice (1010 m pitch in east, 1760 m in north, odd columns 500 m further
    north) leaves both start boxes, grown by the 40 m half hull, in open water with squares 1 m further on:
    a large one east and ring 29 south of the test ship, ring 30 west and ring 31 north of the obstacle ship.
    Those are small, and the lattice has a gap behind them, because the obstacle ship's first intermediate
    waypoint lies 914 m ahead within +-30 degrees (north 2890 to 3214, east 4740 to 5860) and must fall into
    open water for an episode to start at all."""
    rings = [square(0, 0, 2), square(9998, 9998, 2)]
    for j in range(4):
        for i in range(8):
            if (i, j) in ((4, 1), (5, 1), (7, 3), (6, 3), (7, 2)):
                continue
            rings.append(square(641 + 1010 * i, 600 + 1760 * j + (500 if i % 2 else 0), 950))
    rings += [square(140, 559, 500), square(4659, 1900, 500), square(4950, 2341, 500)]
    assert len(rings) == 32
    return rings


def scenario_shifted():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from sac_maritime_ast_amd.scenario import polygons
    return [p + [-20000.0, -15000.0] for p in polygons()]


MAPS = {
    "comb_v": lambda: [zig(128, 10000, 10000, 30, True)],
    "comb_h": lambda: [zig(128, 10000, 10000, 30, False)],
    "comb_h64": lambda: [zig(64, 10000, 10000, 30, False)],
    "comb_dense": lambda: [zig(124, 600, 600, 8, True) + [4000.0, 4000.0], square(0, 0, 50), square(9950, 9950, 50)],
    # a tall narrow comb in a corner of a 30 km extent: every far grid cell lists most of its edges
    "comb_corner": lambda: [zig(124, 250, 10000, 8, True) + [1000.0, 1000.0], square(0, 0, 50),
                            square(29950, 29950, 50)],
    "star128": lambda: [star(128, 300, 5000, 5000, 5000)],
    "squares32": squares32,
    # a square inside a square, two overlapping squares, the second of them clockwise
    "nested": lambda: [square(1000, 1000, 4000), square(2500, 2500, 1000), square(6000, 5000, 2000),
                       square(7000, 6000, 2500, clockwise=True)],
    "shifted": scenario_shifted,
}


def write(name, rings):
    verts = np.concatenate(rings)
    assert np.array_equal(verts, np.rint(verts)) and np.abs(verts).max() < 2 ** 17
    assert len(rings) <= 32 and len(verts) <= 256
    offs = np.concatenate([[0], np.cumsum([len(r) for r in rings])])
    with open(os.path.join(HERE, f"map_{name}.txt"), "w") as f:
        f.write(f"{len(rings)}\n{' '.join(str(int(o)) for o in offs)}\n")
        for e, n in verts:
            f.write(f"{float(e).hex()} {float(n).hex()}\n")


if __name__ == "__main__":
    for name, make in MAPS.items():
        write(name, make())
