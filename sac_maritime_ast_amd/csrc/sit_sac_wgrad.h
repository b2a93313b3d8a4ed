// sit_sac_wgrad.h — the weight gradients of a SAC update as MFMA tiles, fused with Adam (include/sit.h:
// sit_sac_critic_step_tiled, sit_sac_policy_step_tiled).
//
// k_sac_wgrad_adam is the counterpart of k_sac_adam (sit_sac_grad.h) and reads the same workspace
// records.  A weight gradient is a matrix product over the batch, dW2T[k][n] = sum_b h1[b][k] d2[b][n] and
// likewise for W1 and W3, so one wave forms one 32 x 32 tile of one parameter segment of one network with
// v_mfma_f32_32x32x2_f32 whose k index is the batch row: two rows per instruction, ascending, from a zero
// accumulator, never split over the batch.  The instruction is a k-ordered float32 fmaf chain with one
// rounding per product, which is the sum k_sac_adam forms per element, so the two kernels give the same
// bits.  A bias is the same chain with the other operand fixed at 1.0f (fmaf(d, 1, g) is g + d rounded
// once) and takes a tile of its own.
//
// Tiles of SacNet<IN, NOUT>: each segment of sac_segment (sit_sac.h, the map k_sac_adam reads too) cut into
// 32 x 32 tiles, rows x columns, the column index the contiguous index of the packed block; T = 256 / 32 = 8,
// 97 tiles per network, in the block's order:
//   W1    T tiles      A = d1[b][32 jt + i]   B = x[b][j], j < IN
//   b1    T tiles      A = 1 (row 0 is kept)  B = d1[b][32 jt + j]
//   W2^T  T x T tiles  A = h1[b][32 kt + i]   B = d2[b][32 nt + j]
//   b2    T tiles      A = 1                  B = d2[b][32 nt + j]
//   W3    T tiles      A = g[b][i], i < NOUT  B = h2[b][32 nt + j]
//   b3    1 tile       A = g[b][i], i < NOUT  B = 1 (column 0 is kept)
// Lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]: each half-wave reads 32
// contiguous floats of one record.  Operand columns past a segment's width supply 0.0f (their lanes load
// the operand's column 0, a float of the same record, and discard it); their results are never written.
// When B is odd the lanes of row B supply 0.0f for both operands and do not load.
//
// The K loop runs in groups of kWgGroup instructions (32 rows) through two register buffers: the next
// group's 32 operand loads are issued before the current group's MFMAs, so a group's loads have 16 x 64
// cycles of matrix work to arrive in, and 32 to 64 vector-memory loads are in flight per wave (the
// counter holds 63: the last issue of a group waits for the oldest return if none has come back).  The
// last, partial group takes bounds-checked loads and only the instructions that have a row.  Epilogue: C/D element (reg, lane) is row (reg & 3) +
// 8 (reg >> 2) + 4 (lane >> 5), column lane & 31; each lane applies sac_adam_apply to its 16 elements of
// p, m, v, a half-wave per 128 contiguous bytes.  The gradient is never stored and padding floats are not
// touched.
//
// The losses: one wave per network pass behind the tiles.  64 rows' terms are fetched at a time, one per
// lane, and added in ascending row order in float64 as k_sac_adam's thread 0 adds them; lane 0 then calls the
// same sac_finish_losses (sit_sac_grad.h).
//
// Included from sit_kernels.hip only (the strictly compiled translation unit).
#ifndef SIT_SAC_WGRAD_H
#define SIT_SAC_WGRAD_H

#include "sit_sac_grad.h"

namespace {

typedef float SacAcc __attribute__((ext_vector_type(16)));

constexpr int kWgGroup = 16;                       // MFMAs per prefetch group
constexpr int kWgGroupRows = 2 * kWgGroup;
constexpr int kWgT = kActorHidden / 32;            // tiles along a hidden dimension
constexpr int kWgTiles = kWgT * kWgT + 4 * kWgT + 1;   // W2^T, then W1, b1, b2, W3 a strip each, and b3
static_assert(kWsXDim <= 32 && 2 * kWgGroup <= 63, "x fits a tile; a group's loads fit the counter");

struct SacWgradTile {
  int a_at, a_n;                // operand A: its field of a record and its width (0: the constant 1.0f)
  int b_at, b_n;                // operand B
  int out, stride, rows, cols;  // the tile's corner in the block, its row stride, the part that is kept
};

// Tile t of a network: the segments of sac_segment in order, each cut into 32 x 32 tiles, row-major.
template <int IN, int NOUT>
constexpr int sac_wgrad_tiles(int segments) {      // the tiles of segments [0, segments)
  int n = 0;
  for (int s = 0; s < segments; ++s) n += ((sac_segment<IN, NOUT>(s).rows + 31) / 32) * ((sac_segment<IN, NOUT>(s).cols + 31) / 32);
  return n;
}

template <int IN, int NOUT>
__device__ __forceinline__ SacWgradTile sac_wgrad_tile(int t) {
  static_assert(sac_wgrad_tiles<IN, NOUT>(kSacSegments) == kWgTiles, "the grid's tile blocks per network");
  constexpr auto width = [](int n, int at) { return n - at < 32 ? n - at : 32; };   // of a tile that starts at `at`
  SacWgradTile d{};
#pragma unroll
  for (int s = 0; s < kSacSegments; ++s) {
    const SacSegment g = sac_segment<IN, NOUT>(s);
    const int first = sac_wgrad_tiles<IN, NOUT>(s), across = (g.cols + 31) / 32;
    if (t >= first && t < sac_wgrad_tiles<IN, NOUT>(s + 1)) {
      const int r0 = 32 * ((t - first) / across), c0 = 32 * ((t - first) % across);
      d = {g.row_at + r0, g.row_n ? width(g.row_n, r0) : 0, g.col_at + c0, g.col_n ? width(g.col_n, c0) : 0,
           g.out + r0 * g.cols + c0, g.cols, width(g.rows, r0), width(g.cols, c0)};
    }
  }
  return d;
}

// A lane's side of the K loop: pa / pb are its A and B addresses in the record of row `half` (lanes past an
// operand's width: of a float that is there), ca / cb what such a lane supplies instead of what it loaded.
struct SacWgradLane {
  const float *pa, *pb;
  bool la, lb;
  float ca, cb;
  int half, batch;
};

// A whole group's operands, row0 its first row (wave-uniform), as they are in memory: the lanes past an
// operand's width substitute their constant when the MFMA consumes the value (sac_wgrad_mfma), so nothing
// waits for a load here.
__device__ __forceinline__ void sac_wgrad_load(const SacWgradLane& w, int row0, float (&av)[kWgGroup],
                                               float (&bv)[kWgGroup]) {
#pragma unroll
  for (int u = 0; u < kWgGroup; ++u) {
    const size_t at = (size_t)(row0 + 2 * u) * kWsRow;
    av[u] = w.pa[at];
    bv[u] = w.pb[at];
  }
  // the loads stay ahead of the MFMAs that follow in program order: left alone, the scheduler sinks a
  // group's loads to just before their use, into the registers of the group being consumed
  __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ void sac_wgrad_mfma(const SacWgradLane& w, const float (&av)[kWgGroup],
                                               const float (&bv)[kWgGroup], SacAcc& acc) {
#pragma unroll
  for (int u = 0; u < kWgGroup; ++u)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.la ? av[u] : w.ca, w.lb ? bv[u] : w.cb, acc, 0, 0, 0);
  __builtin_amdgcn_sched_barrier(0);
}

// The last, partial group (rows [row0, batch), fewer than kWgGroupRows): bounds-checked and complete as
// loaded.  A row past the batch is not loaded: its lanes supply 0 for both operands.
__device__ __forceinline__ void sac_wgrad_load_tail(const SacWgradLane& w, int row0, float (&av)[kWgGroup],
                                                    float (&bv)[kWgGroup]) {
#pragma unroll
  for (int u = 0; u < kWgGroup; ++u) {
    const int row = row0 + 2 * u;
    float x = 0.0f, y = 0.0f;
    if (row + w.half < w.batch) {
      const size_t at = (size_t)row * kWsRow;
      x = w.la ? w.pa[at] : w.ca;
      y = w.lb ? w.pb[at] : w.cb;
    }
    av[u] = x;
    bv[u] = y;
  }
}

__device__ __forceinline__ void sac_wgrad_mfma_tail(int rows, const float (&av)[kWgGroup], const float (&bv)[kWgGroup],
                                                    SacAcc& acc) {
#pragma unroll
  for (int u = 0; u < kWgGroup; ++u)
    if (2 * u < rows) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
}

// the per-row loss terms of one network pass, 64 rows per fetch; every lane ends with the same sums
template <bool TEMPERATURE>
__device__ __forceinline__ void sac_wgrad_loss_sums(const float* g, int batch, float target_entropy, double& sum,
                                                    double& ent) {
  const int lane = threadIdx.x;
  auto fetch = [&](int b0, float& t2, float& t3) {
    t2 = 0.0f;
    t3 = 0.0f;
    if (b0 + lane < batch) {
      const float* p = g + (size_t)(b0 + lane) * kWsRow;
      t2 = p[2];
      if (TEMPERATURE) t3 = p[3];
    }
  };
  auto term = [&](float t2, float t3, int i) {
    sum += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(t2), i));
    if (TEMPERATURE)
      ent += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(t3), i)) + (double)target_entropy;
  };
  float t2, t3;
  fetch(0, t2, t3);
  for (int b0 = 0; b0 < batch; b0 += 64) {
    float n2 = 0.0f, n3 = 0.0f;
    if (b0 + 64 < batch) fetch(b0 + 64, n2, n3);
    const int n = batch - b0;
    if (n >= 64) {
#pragma unroll
      for (int i = 0; i < 64; ++i) term(t2, t3, i);
    } else {
      for (int i = 0; i < n; ++i) term(t2, t3, i);
    }
    t2 = n2;
    t3 = n3;
  }
}

// NETS networks of SacNet<IN, NOUT>, STRIDE floats apart: blocks of one wave, kWgTiles tile blocks per
// network, then the loss blocks (one per network; TEMPERATURE: one, which also takes the temperature step).
// CLOCKED: as in k_sac_adam (sit_sac_grad.h).
template <int IN, int NOUT, int NETS, int STRIDE, bool TEMPERATURE, bool CLOCKED = false>
__global__ __launch_bounds__(64) void k_sac_wgrad_adam(const SacAdamArgs<CLOCKED> a) {
#pragma clang fp reassociate(off) contract(off)
  static_assert(!TEMPERATURE || NETS == 1, "the temperature step belongs to the actor's launch");
  const int B = a.batch;
  const int blk = blockIdx.x;
  if (blk >= NETS * kWgTiles) {                    // a loss block
    const int c = blk - NETS * kWgTiles;
    double sum = 0.0, ent = 0.0;
    sac_wgrad_loss_sums<TEMPERATURE>(a.ws + (size_t)c * (size_t)B * kWsRow + kWsG, B, a.target_entropy, sum, ent);
    if constexpr (CLOCKED) {
      if (threadIdx.x == 0) {
        sac_finish_losses<TEMPERATURE>(sac_adam_from_tick<TEMPERATURE>(a), c, sum, ent);
        if (TEMPERATURE) sac_clock_advance(a.k.clock, a.k.hy, a.k.slot ^ 1);
      }
    } else {
      if (threadIdx.x == 0) sac_finish_losses<TEMPERATURE>(a, c, sum, ent);
    }
    return;
  }
  const int c = blk / kWgTiles;
  const SacWgradTile d = sac_wgrad_tile<IN, NOUT>(blk % kWgTiles);
  const int col = threadIdx.x & 31, half = threadIdx.x >> 5;
  SacWgradLane w;
  w.la = col < d.a_n;
  w.lb = col < d.b_n;
  w.ca = d.a_n ? 0.0f : 1.0f;
  w.cb = d.b_n ? 0.0f : 1.0f;
  w.half = half;
  w.batch = B;
  const float* rec = a.ws + ((size_t)c * (size_t)B + (size_t)half) * kWsRow;
  w.pa = rec + d.a_at + (w.la ? col : 0);
  w.pb = rec + d.b_at + (w.lb ? col : 0);

  SacAcc acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  // Whole groups through two register buffers in turn, each loaded one group of MFMAs ahead of its use;
  // the partial group's loads go out ahead of the last whole group's MFMAs.
  const int full = B / kWgGroupRows * kWgGroupRows, tail = B - full;
  float a0[kWgGroup], b0[kWgGroup], a1[kWgGroup], b1[kWgGroup], at[kWgGroup], bt[kWgGroup];
  if (full > 0) {
    int row0 = 0;
    sac_wgrad_load(w, 0, a0, b0);
    for (; row0 + 2 * kWgGroupRows < full; row0 += 2 * kWgGroupRows) {
      sac_wgrad_load(w, row0 + kWgGroupRows, a1, b1);
      sac_wgrad_mfma(w, a0, b0, acc);
      sac_wgrad_load(w, row0 + 2 * kWgGroupRows, a0, b0);
      sac_wgrad_mfma(w, a1, b1, acc);
    }
    if (row0 + kWgGroupRows < full) {
      sac_wgrad_load(w, row0 + kWgGroupRows, a1, b1);
      sac_wgrad_mfma(w, a0, b0, acc);
      if (tail > 0) sac_wgrad_load_tail(w, full, at, bt);
      sac_wgrad_mfma(w, a1, b1, acc);
    } else {
      if (tail > 0) sac_wgrad_load_tail(w, full, at, bt);
      sac_wgrad_mfma(w, a0, b0, acc);
    }
  } else {
    sac_wgrad_load_tail(w, 0, at, bt);
  }
  if (tail > 0) sac_wgrad_mfma_tail(tail, at, bt, acc);

  if (col >= d.cols) return;
  const size_t corner = (size_t)c * STRIDE + (size_t)d.out + (size_t)col;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
    if (row < d.rows) {
      const size_t e = corner + (size_t)row * (size_t)d.stride;
      if constexpr (CLOCKED) sac_adam_apply_clocked<TEMPERATURE>(a, sac_clock_tick(a.k.clock, a.k.slot), acc[r], e);
      else sac_adam_apply(a.o, acc[r], a.p + e, a.m + e, a.v + e);
    }
  }
}

// the Adam kernel of a call and its grid: the tiled one here, or k_sac_adam (sit_sac_grad.h)
template <int IN, int NOUT, int NETS, int STRIDE, bool TEMPERATURE>
inline SacAdamLaunch sac_adam_launch(bool tiled) {
  if (!tiled) return {k_sac_adam<IN, NOUT, NETS, STRIDE, TEMPERATURE>, (NETS * STRIDE + 255) / 256 + 1, 256};
  return {k_sac_wgrad_adam<IN, NOUT, NETS, STRIDE, TEMPERATURE>, NETS * kWgTiles + NETS, 64};
}

template <int IN, int NOUT, int NETS, int STRIDE, bool TEMPERATURE>
inline SacAdamClockLaunch sac_adam_clocked_launch(bool tiled) {
  if (!tiled) return {k_sac_adam<IN, NOUT, NETS, STRIDE, TEMPERATURE, true>, (NETS * STRIDE + 255) / 256 + 1, 256};
  return {k_sac_wgrad_adam<IN, NOUT, NETS, STRIDE, TEMPERATURE, true>, NETS * kWgTiles + NETS, 64};
}

}  // namespace

#endif  // SIT_SAC_WGRAD_H
