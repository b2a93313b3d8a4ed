// sit_map_format.h — the island map's edge record and the constants of its spatial index, shared
// by the device predicates (sit_device.h, Map<T>) and the host builder (sit_map_build.h).  No HIP
// include: the builder and its test program compile with a plain host compiler.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace sit {

constexpr int kMaxPolyVerts = 256;
constexpr int kMaxPolys = 32;

// island map (obstacle.py:92-124): edge i of the closed rings runs from (ax, ay) to (bx, by);
// coordinates are (x = east, y = north) as in obstacle.py:128.  One Edge record per edge (one
// LDS base pointer, immediate field offsets) so the predicates need no per-array registers.
//
// Spatial index (built on the host by build_map_image, sit_map_build.h; exact by construction),
// one u16 array:
//   idx[0 .. 4*G*G)          grid cell records, 8 bytes each: the list's first group inline
//                            (x = ids 0-3, y bits 0-7 = id 4), y bits 8-15 = number of further
//                            groups, y bits 16-31 = the first of them (in 8-byte groups from the
//                            start of idx).  The cell's first 5 candidates are then one LDS read
//                            away from the cell index, their edges two.
//   idx[kBandBase ..]        NB+1 band starts (absolute positions in idx)
//   then the band entries (edge ids), then the further grid groups (8-byte aligned).
//  * grid: G x G cells over the map extent plus a margin; cell c lists every edge that can be
//    the nearest edge of some point within 1 m of the cell (conservative prefilter, then a
//    Lipschitz-sampled refinement with a 1 m float slack; grid_candidates), so the minimum over the
//    list equals the minimum over all edges.  A list is padded to a multiple of 5 with its first
//    id and packed as 5 u8 ids per 8-byte group, so one LDS read yields 5 ids whose edge loads
//    are independent (duplicates do not change a minimum).
//  * bands: NB horizontal bands; band b lists every edge whose y-range meets the band (+-1 m).
//    GEOS's ray-crossing test only looks at edges whose y-range contains the point's y.
//  * classes (separate u32 array): kFine x kFine cells over the map extent + 100 m, 2 bits per
//    cell: 0 = no boundary within 1 m of the cell and its points are outside every polygon,
//    1 = likewise inside one, 2 = mixed.  A point outside the class grid is > 100 m off the
//    map and therefore outside every polygon.  With ~40 m cells every point farther than
//    ~31 m from the shore resolves by one lookup.
constexpr int kGrid = 32;
constexpr int kBands = 64;
constexpr int kBandBase = 4 * kGrid * kGrid;
constexpr int kIdxHead = kBandBase + kBands + 1;
constexpr int kFine = 256;
constexpr int kFineWords = kFine * kFine / 16;

template <typename T>
struct alignas(16) Edge {
  T ax, ay, bx, by;
  T il2;            // 1 / |edge|^2 (0 for a degenerate edge)
  uint32_t poly;    // polygon id
};

// What the handle keeps about a built map image (build_map_image): where its sections start and
// the geometry the kernels' constants are derived from.
// image: [Edge<T>[n_vert]][u16 index][u32 classes][frank][crec][clive] (staged into LDS: map_bytes)
//        [ring offsets][bboxes] (fallback scan, global)
struct MapMeta {
  size_t idx_off = 0, fine_off = 0, frank_off = 0, crec_off = 0, clive_off = 0, ring_off = 0, bbox_off = 0;
  size_t map_bytes = 0;      // bytes staged into LDS: edges, packed index, classes, mixed-cell records
  int n_poly = 0, n_vert = 0;
  int use_index = 0, use_cells = 0;           // 0: the index / the mixed-cell records exceed their u16 limits
  int64_t n_idx = 0, n_mixed = 0, n_live = 0;   // entries of idx / crec / clive
  double gx0 = 0, gy0 = 0, ginvx = 0, ginvy = 0;   // grid origin and 1 / cell size
  double by0 = 0, binv = 0;                        // band origin and 1 / band height
  double fx0 = 0, fy0 = 0, finvx = 0, finvy = 0;   // class grid origin and 1 / cell size
  double min_n = 0, max_n = 0, min_e = 0, max_e = 0;   // PolygonObstacle.map_boundaries
};

}  // namespace sit
