// sit_map_build.h — host-only builder of the island map's device image (sit_load_map): edge
// records, the packed spatial index, the class grid and the mixed-cell records in the format of
// sit_map_format.h.  Pure double-precision geometry over standard headers, no HIP: the same code
// runs in the library and in the stand-alone program of tests/test_map_build_host.py.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sit_map_format.h"

namespace sit {

struct MapImage {
  MapMeta meta;
  std::vector<unsigned char> bytes;
};

namespace map_build {

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// the closed rings as edges i: (vx, vy) -> (bxv, byv), with 1 / |edge|^2 and the polygons' bboxes
struct Edges {
  int n_poly = 0, nv = 0;
  std::vector<double> vx, vy, bxv, byv, il2, bbox;
  std::vector<int32_t> offs;
  std::vector<int> poly_of;
  double min_e = INFINITY, max_e = -INFINITY, min_n = INFINITY, max_n = -INFINITY;

  double seg_dist(double px, double py, int i) const {
    const double ex = bxv[i] - vx[i], ey = byv[i] - vy[i], l2 = ex * ex + ey * ey;
    double t = l2 > 0 ? ((px - vx[i]) * ex + (py - vy[i]) * ey) / l2 : 0.0;
    t = std::min(1.0, std::max(0.0, t));
    return std::hypot(px - (vx[i] + t * ex), py - (vy[i] + t * ey));
  }
};

// u16 entries of consecutive lists: list c is entries[start[c] .. start[c + 1])
struct Lists {
  std::vector<uint16_t> entries;
  std::vector<uint32_t> start;
};

inline Edges edges_and_bboxes(int n_poly, const int32_t* vert_offsets, const double* verts_en) {
  Edges E;
  const int nv = vert_offsets[n_poly];
  E.n_poly = n_poly;
  E.nv = nv;
  E.vx.resize(nv); E.vy.resize(nv); E.il2.resize(nv); E.bbox.resize(4 * n_poly);
  E.offs.assign(vert_offsets, vert_offsets + n_poly + 1);
  std::vector<int32_t> nxt(nv);
  const std::vector<int32_t>& offs = E.offs;
  // PolygonObstacle.map_boundaries (obstacle.py:111-124): vertices are (east, north)
  for (int p = 0; p < n_poly; ++p) {
    double bx0 = INFINITY, bx1 = -INFINITY, by0 = INFINITY, by1 = -INFINITY;
    for (int i = offs[p]; i < offs[p + 1]; ++i) {
      E.vx[i] = verts_en[2 * i];
      E.vy[i] = verts_en[2 * i + 1];
      nxt[i] = (i + 1 < offs[p + 1]) ? i + 1 : offs[p];
      bx0 = std::min(bx0, E.vx[i]); bx1 = std::max(bx1, E.vx[i]);
      by0 = std::min(by0, E.vy[i]); by1 = std::max(by1, E.vy[i]);
    }
    E.bbox[4 * p + 0] = bx0; E.bbox[4 * p + 1] = bx1; E.bbox[4 * p + 2] = by0; E.bbox[4 * p + 3] = by1;
    E.min_e = std::min(E.min_e, bx0); E.max_e = std::max(E.max_e, bx1);
    E.min_n = std::min(E.min_n, by0); E.max_n = std::max(E.max_n, by1);
  }
  E.bxv.resize(nv); E.byv.resize(nv);
  for (int i = 0; i < nv; ++i) {
    E.bxv[i] = E.vx[nxt[i]];
    E.byv[i] = E.vy[nxt[i]];
    const double ex = E.bxv[i] - E.vx[i], ey = E.byv[i] - E.vy[i];
    const double l2 = ex * ex + ey * ey;
    E.il2[i] = l2 > 0 ? 1.0 / l2 : 0.0;
  }
  E.poly_of.resize(nv);
  for (int p = 0; p < n_poly; ++p)
    for (int i = offs[p]; i < offs[p + 1]; ++i) E.poly_of[i] = p;
  return E;
}

// ---- spatial index (see sit_map_format.h): conservative nearest-edge candidates per grid cell,
//      edges per horizontal band.  Exact by construction; 1 m slack covers float rounding.
inline Lists grid_candidates(const Edges& E, double gx0, double gy0, double sx, double sy) {
  const int nv = E.nv;
  const double hd = 0.5 * std::sqrt(sx * sx + sy * sy) + 1.0;
  Lists G;
  G.start.resize(kGrid * kGrid + 1);
  std::vector<uint16_t>& gentries = G.entries;
  std::vector<double> dcell(nv);
  std::vector<int> cand;
  constexpr int kSamples = 64;   // per cell side for the candidate refinement
  for (int j = 0; j < kGrid; ++j)
    for (int i = 0; i < kGrid; ++i) {
      const double cx = gx0 + (i + 0.5) * sx, cy = gy0 + (j + 0.5) * sy;
      double D = INFINITY;
      for (int e = 0; e < nv; ++e) { dcell[e] = E.seg_dist(cx, cy, e); D = std::min(D, dcell[e] + hd); }
      G.start[j * kGrid + i] = (uint32_t)gentries.size();
      // conservative prefilter, then the Lipschitz refinement: for every point p of the cell
      // grown by 1 m, some sample s lies within r; the nearest edge e* of p has
      // d_e*(s) <= d*(p) + r and min_f d_f(s) >= d*(p) - r, so e* is kept by
      // d_e(s) <= min_f d_f(s) + 2r + 1 m at some sample.  A dropped edge is >= 1 m farther than
      // the nearest at every point of the grown cell, so float rounding cannot make it the
      // minimum: the minimum over the list equals the full scan's.
      cand.clear();
      for (int e = 0; e < nv; ++e)
        if (dcell[e] - hd <= D + 1.0) cand.push_back(e);
      if (cand.size() > 1) {
        const double x0 = gx0 + i * sx - 1.0, y0 = gy0 + j * sy - 1.0;
        const double dx = (sx + 2.0) / kSamples, dy = (sy + 2.0) / kSamples;
        const double r2 = std::sqrt(dx * dx + dy * dy) + 1.0;   // 2r + 1 m
        std::vector<char> keep(cand.size(), 0);
        std::vector<double> dd(cand.size());
        for (int v = 0; v < kSamples; ++v)
          for (int u = 0; u < kSamples; ++u) {
            const double px = x0 + (u + 0.5) * dx, py = y0 + (v + 0.5) * dy;
            double m = INFINITY;
            for (size_t q = 0; q < cand.size(); ++q) { dd[q] = E.seg_dist(px, py, cand[q]); m = std::min(m, dd[q]); }
            for (size_t q = 0; q < cand.size(); ++q) keep[q] |= dd[q] <= m + r2;
          }
        size_t w = 0;
        for (size_t q = 0; q < cand.size(); ++q)
          if (keep[q]) cand[w++] = cand[q];
        cand.resize(w);
      }
      // groups of 5 u8 ids in 8 bytes (padded with the list's first id): every list of the
      // reference map fits one group (lists of 5 near some vertices would need two groups of 4)
      while (cand.size() % 5) cand.push_back(cand[0]);
      for (size_t q = 0; q < cand.size(); q += 5) {
        gentries.push_back((uint16_t)(cand[q] | (cand[q + 1] << 8)));
        gentries.push_back((uint16_t)(cand[q + 2] | (cand[q + 3] << 8)));
        gentries.push_back((uint16_t)cand[q + 4]);
        gentries.push_back(0);
      }
    }
  G.start[kGrid * kGrid] = (uint32_t)gentries.size();
  return G;
}

inline Lists band_lists(const Edges& E, double by0, double bh) {
  Lists B;
  B.start.resize(kBands + 1);
  for (int b = 0; b < kBands; ++b) {
    B.start[b] = (uint32_t)B.entries.size();
    const double lo = by0 + b * bh - 1.0, hi = by0 + (b + 1) * bh + 1.0;
    for (int e = 0; e < E.nv; ++e)
      if (std::min(E.vy[e], E.byv[e]) <= hi && std::max(E.vy[e], E.byv[e]) >= lo) B.entries.push_back((uint16_t)e);
  }
  B.start[kBands] = (uint32_t)B.entries.size();
  return B;
}

// point-in-polygon by crossing number for class-grid cell centres (>= 1 m off every edge)
inline bool inside_center(const Edges& E, double px, double py) {
  bool in = false;
  for (int p = 0; p < E.n_poly; ++p) {
    int cross = 0;
    for (int i = E.offs[p]; i < E.offs[p + 1]; ++i) {
      const double x1 = E.vx[i], y1 = E.vy[i], x2 = E.bxv[i], y2 = E.byv[i];
      if ((y1 > py) != (y2 > py)) {
        const double xi = x1 + (py - y1) * (x2 - x1) / (y2 - y1);
        if (xi > px) ++cross;
      }
    }
    in |= (cross & 1) != 0;
  }
  return in;
}

// fine 2-bit classes over the map extent + 100 m
inline std::vector<uint32_t> class_grid(const Edges& E, double fx0, double fy0, double fsx, double fsy) {
  const double fhd = 0.5 * std::sqrt(fsx * fsx + fsy * fsy) + 1.0;
  std::vector<uint32_t> fine(kFineWords, 0);
  for (int j = 0; j < kFine; ++j)
    for (int i = 0; i < kFine; ++i) {
      const double cx = fx0 + (i + 0.5) * fsx, cy = fy0 + (j + 0.5) * fsy;
      double dmin = INFINITY;
      for (int e = 0; e < E.nv && dmin > fhd + 1.0; ++e) dmin = std::min(dmin, E.seg_dist(cx, cy, e));
      const uint32_t k = dmin > fhd + 1.0 ? (inside_center(E, cx, cy) ? 1u : 0u) : 2u;
      const int cell = j * kFine + i;
      fine[cell >> 4] |= k << ((cell & 15) * 2);
    }
  return fine;
}

// point-in-polygon records of the mixed cells (see Map in sit_device.h).  An edge's GEOS
// crossing contribution is the same for every point of cell [x0,x1]x[y0,y1] when (1 m
// margin, far above float rounding of coordinates <= 1e5 m): it lies wholly left of the cell
// (early return), its y-range misses the cell's rows, or it spans the rows strictly and,
// within them, lies wholly right or wholly left of the cell (then it straddles every row and
// its orientation against every point is that against the centre).  All other edges are live.
struct MixedCells {
  std::vector<uint16_t> frank;
  std::vector<uint32_t> crec;
  std::vector<uint8_t> clive;
};
inline MixedCells mixed_cell_records(const Edges& E, const std::vector<uint32_t>& fine, double fx0, double fy0,
                                     double fsx, double fsy) {
  MixedCells M;
  M.frank.assign(kFineWords, 0);
  int rank = 0;
  for (int w = 0; w < kFineWords; ++w) {
    M.frank[w] = (uint16_t)std::min(rank, 65535);
    rank += __builtin_popcount((fine[w] >> 1) & 0x55555555u);
  }
  for (int cell = 0; cell < kFine * kFine; ++cell) {
    if (((fine[cell >> 4] >> ((cell & 15) * 2)) & 3) != 2) continue;
    const int i = cell % kFine, j = cell / kFine;
    const double x0 = fx0 + i * fsx, x1 = fx0 + (i + 1) * fsx, y0 = fy0 + j * fsy, y1 = fy0 + (j + 1) * fsy;
    const double cx = 0.5 * (x0 + x1), cy = 0.5 * (y0 + y1), mgn = 1.0;
    uint32_t par = 0;
    const size_t first = M.clive.size();
    for (int e = 0; e < E.nv; ++e) {
      const double p1x = E.vx[e], p1y = E.vy[e], p2x = E.bxv[e], p2y = E.byv[e];
      const double xmax = std::max(p1x, p2x), ymin = std::min(p1y, p2y), ymax = std::max(p1y, p2y);
      if (xmax < x0 - mgn) continue;                          // left of every point: no count
      if (ymax < y0 - mgn || ymin > y1 + mgn) continue;       // never straddles a cell row
      if (ymin < y0 - mgn && ymax > y1 + mgn) {
        const double ta = (y0 - mgn - p1y) / (p2y - p1y), tb = (y1 + mgn - p1y) / (p2y - p1y);
        const double xa = p1x + ta * (p2x - p1x), xb = p1x + tb * (p2x - p1x);
        const bool right = std::min(xa, xb) > x1 + mgn && xmax > x1 + mgn;
        const bool left = std::max(xa, xb) < x0 - mgn && xmax > x1 + mgn;
        if (right || left) {
          const double det = (p1x - cx) * (p2y - cy) - (p1y - cy) * (p2x - cx);
          const int o = (det > 0) - (det < 0);
          const int oo = (p2y < p1y) ? -o : o;
          if (oo > 0) par ^= 1u << E.poly_of[e];
          continue;
        }
      }
      M.clive.push_back((uint8_t)e);
    }
    const size_t cnt = M.clive.size() - first;
    M.crec.push_back(par);
    M.crec.push_back((uint32_t)first | ((uint32_t)cnt << 16));
  }
  return M;
}

// packed u16 index: [grid records (u32 pair per cell)][band starts (NB+1)][band entries][grid groups].
// Each cell's first group goes into its record; the further groups (lists of > 5) follow the band
// entries.  *use_index = 0 (and a 4-entry placeholder) when the index exceeds u16 positions or 48 KB.
inline std::vector<uint16_t> pack_index(const Lists& G, const Lists& B, int* use_index) {
  std::vector<uint16_t> grest;
  std::vector<uint32_t> rstart(kGrid * kGrid);
  for (int c = 0; c < kGrid * kGrid; ++c) {
    rstart[c] = (uint32_t)grest.size();
    grest.insert(grest.end(), G.entries.begin() + G.start[c] + 4, G.entries.begin() + G.start[c + 1]);
  }
  const size_t head = (size_t)kIdxHead;
  const size_t gbase = (head + B.entries.size() + 3) & ~size_t(3);   // 8-byte aligned groups
  const size_t n_idx = gbase + grest.size();
  *use_index = (n_idx < 65535 && n_idx * 2 <= 48 * 1024) ? 1 : 0;
  std::vector<uint16_t> idx(*use_index ? n_idx : 4, 0);
  if (*use_index) {
    for (int c = 0; c < kGrid * kGrid; ++c) {
      const uint16_t* f = G.entries.data() + G.start[c];
      const uint32_t more = (G.start[c + 1] - G.start[c]) / 4 - 1;    // < 52: ids are u8, 5 per group
      const uint32_t y = (f[2] & 0xffu) | (more << 8) | ((uint32_t)((gbase + rstart[c]) / 4) << 16);
      idx[4 * c] = f[0];                       // ids 0, 1
      idx[4 * c + 1] = f[1];                   // ids 2, 3
      idx[4 * c + 2] = (uint16_t)(y & 0xffffu);
      idx[4 * c + 3] = (uint16_t)(y >> 16);
    }
    for (int b = 0; b <= kBands; ++b) idx[kBandBase + b] = (uint16_t)(head + B.start[b]);
    std::copy(B.entries.begin(), B.entries.end(), idx.begin() + head);
    std::copy(grest.begin(), grest.end(), idx.begin() + gbase);
  }
  return idx;
}

}  // namespace map_build

// The device image of a validated map (sit_load_map's checks: 1..kMaxPolys rings of >= 3 vertices,
// at most kMaxPolyVerts in all; vertices are (east, north)) for reals of real_size 4 or 8 bytes.
inline MapImage build_map_image(int n_poly, const int32_t* vert_offsets, const double* verts_en, size_t real_size) {
  using namespace map_build;
  const size_t rs = real_size;
  MapImage img;
  MapMeta& m = img.meta;
  const Edges E = edges_and_bboxes(n_poly, vert_offsets, verts_en);
  const int nv = E.nv;
  m.n_poly = n_poly; m.n_vert = nv;
  m.min_e = E.min_e; m.max_e = E.max_e; m.min_n = E.min_n; m.max_n = E.max_n;
  const double ext_x = m.max_e - m.min_e, ext_y = m.max_n - m.min_n;
  const double mg = 0.1 * std::max(ext_x, ext_y) + 500.0;
  const double gx0 = m.min_e - mg, gy0 = m.min_n - mg;
  const double sx = (ext_x + 2 * mg) / kGrid, sy = (ext_y + 2 * mg) / kGrid;
  const Lists G = grid_candidates(E, gx0, gy0, sx, sy);
  const double by0 = m.min_n - 1.0, bh = (ext_y + 2.0) / kBands;
  const Lists B = band_lists(E, by0, bh);
  const double fx0 = m.min_e - 100.0, fy0 = m.min_n - 100.0;
  const double fsx = (ext_x + 200.0) / kFine, fsy = (ext_y + 200.0) / kFine;
  const std::vector<uint32_t> fine = class_grid(E, fx0, fy0, fsx, fsy);
  const MixedCells M = mixed_cell_records(E, fine, fx0, fy0, fsx, fsy);
  const bool cells_ok = M.crec.size() / 2 <= 65535 && M.clive.size() <= 65535;
  const std::vector<uint16_t> idx = pack_index(G, B, &m.use_index);
  m.n_idx = (int64_t)idx.size();
  m.gx0 = gx0; m.gy0 = gy0; m.ginvx = 1.0 / sx; m.ginvy = 1.0 / sy;
  m.by0 = by0; m.binv = 1.0 / bh;
  m.fx0 = fx0; m.fy0 = fy0; m.finvx = 1.0 / fsx; m.finvy = 1.0 / fsy;
  // layout (MapMeta, sit_map_format.h)
  const size_t esz = rs == 8 ? sizeof(Edge<double>) : sizeof(Edge<float>);
  size_t o = align256(nv * esz);
  m.idx_off = o; o = align256(o + idx.size() * 2);
  m.fine_off = o; o = align256(o + fine.size() * 4);
  m.use_cells = cells_ok ? 1 : 0;
  m.n_mixed = (int64_t)M.crec.size() / 2;
  m.n_live = (int64_t)M.clive.size();
  m.frank_off = o; o += (cells_ok ? M.frank.size() * 2 : 0); o = (o + 7) & ~size_t(7);
  m.crec_off = o; o += (cells_ok ? M.crec.size() * 4 : 0);
  m.clive_off = o; o = align256(o + (cells_ok ? M.clive.size() : 0));
  m.map_bytes = o;
  m.ring_off = o; o = align256(o + (n_poly + 1) * 4);
  m.bbox_off = o; o = align256(o + 4 * n_poly * rs);
  img.bytes.assign(o, 0);
  unsigned char* host = img.bytes.data();
  for (int e = 0; e < nv; ++e) {
    if (rs == 8) {
      Edge<double> g{E.vx[e], E.vy[e], E.bxv[e], E.byv[e], E.il2[e], (uint32_t)E.poly_of[e]};
      std::memcpy(host + e * esz, &g, sizeof(g));
    } else {
      Edge<float> g{(float)E.vx[e], (float)E.vy[e], (float)E.bxv[e], (float)E.byv[e], (float)E.il2[e],
                    (uint32_t)E.poly_of[e]};
      std::memcpy(host + e * esz, &g, sizeof(g));
    }
  }
  std::memcpy(host + m.idx_off, idx.data(), idx.size() * 2);
  std::memcpy(host + m.fine_off, fine.data(), fine.size() * 4);
  if (cells_ok) {
    std::memcpy(host + m.frank_off, M.frank.data(), M.frank.size() * 2);
    std::memcpy(host + m.crec_off, M.crec.data(), M.crec.size() * 4);
    if (!M.clive.empty()) std::memcpy(host + m.clive_off, M.clive.data(), M.clive.size());
  }
  std::memcpy(host + m.ring_off, E.offs.data(), (n_poly + 1) * 4);
  for (size_t i = 0; i < E.bbox.size(); ++i) {
    if (rs == 8) reinterpret_cast<double*>(host + m.bbox_off)[i] = E.bbox[i];
    else reinterpret_cast<float*>(host + m.bbox_off)[i] = (float)E.bbox[i];
  }
  return img;
}

}  // namespace sit
