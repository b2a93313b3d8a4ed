// sit_sac_rows.h — the SAC row kernels with their two 256 x 256 products on the matrix cores (include/sit.h:
// sit_sac_target_wide, sit_sac_critic_step_wide, sit_sac_policy_step_wide).
//
// k_sac_target_wide, k_sac_critic_fb_wide and k_sac_policy_fb_wide are the counterparts of k_sac_target
// (sit_sac.h), k_sac_critic_fb and k_sac_policy_fb (sit_sac_grad.h): same argument structs, same workspace
// records, same outputs, the same bits.  One block of 256 threads (4 waves) takes kRwRows = 32 minibatch
// rows instead of 8, so W2^T is streamed once per 32 rows, and the two sums that are 95 % of a row's
// arithmetic run as v_mfma_f32_32x32x2_f32 chains:
//
//   forward layer 2   z2[r][n] = sum_k h1[r][k] W2T[k][n]: i = row, j = output unit, k = input unit.  Wave w owns
//       units [64 w, 64 w + 64) as two tiles, tile t unit 64 w + 2 j + t, so that one 8-byte load per lane
//       (W2T[k][64 w + 2 j ..]) feeds both tiles and a half-wave reads 256 contiguous bytes.  Per tile four
//       accumulators, one per K quarter [64 q, 64 q + 64), each from zero with k ascending; the epilogue is
//       relu(((q0 + q1) + (q2 + q3)) + b2) on the VALU: sac_mlp's sums and its join.
//   backward layer 2  d1[r][k] = (sum_n W2T[k][n] d2[r][n]) [h1[r][k] > 0]: i = row, j = input unit k, the MFMA's
//       k index is n.  Wave w owns units [64 w, 64 w + 64) as two tiles, tile t unit 64 w + 32 t + j; one
//       accumulator per tile, n = 0..255 ascending from zero, never split: sac_mlp_backward's chain.  The
//       weight operand W2T[k][n + (lane >> 5)] would touch 32 cache lines per 4-byte load, so each lane loads
//       whole float4s of its own row k and consumes one over two MFMAs (the low half-wave supplies elements
//       x, z, the high one y, w).
//
// The float32-input MFMA is a k-ordered fmaf chain with one rounding per product (sit_sac_wgrad.h holds it
// to that on the device), and a product does not depend on the order of its factors, so both sums are the
// narrow kernels' bit for bit.  Everything else keeps their per-row arithmetic, operation for operation:
// layer 1 (thread j = hidden unit j, fmaf over i ascending, + b1), layer 3 and g_a (16 lanes x 16 units, the
// xor tree 8, 4, 2, 1, + b3; with 32 rows in several passes of 256 threads), d2 (fmaf over o, then the
// mask), sac_gaussian_head, the loss terms, the q1 <= q2 tie rule and the TD target in the handle's real.
//
// LDS (dynamic, 66.6 KiB: two blocks per CU): two 32 x 256 float fields with a row stride of 257 floats.
// f1 holds h1 and then d1, f2 holds h2 and then d2: d2[r][n] needs only h2[r][n] and is written by the thread
// that has just stored h2[r][n] to the record, and d1[r][k] needs only h1[r][k], which the lane that holds the
// accumulator reads before it writes.  With the odd stride the MFMA's A operand (lane l reads
// f[l & 31][k + (l >> 5)]), the column-wise writes of layer 1 and the epilogues' writes are free of bank
// conflicts.  Rows past B in the last block run on zeros with zero output gradients and are neither read
// from nor written to global memory.
//
// The K loops run in groups of 16 (forward) and 32 (backward) MFMAs through two register buffers, the next group's operands issued ahead
// of the current group's MFMAs (as k_sac_wgrad_adam does); a forward pass asks for its first group's weights
// before layer 1.
//
// Included from sit_kernels.hip only (the strictly compiled translation unit).
#ifndef SIT_SAC_ROWS_H
#define SIT_SAC_ROWS_H

#include <cstddef>

#include "sit_sac_wgrad.h"

namespace {

constexpr int kRwRows = 32;                        // minibatch rows per block
constexpr int kRwStride = kActorHidden + 1;        // row stride of an LDS field: odd, see above
static_assert(kActorHidden == 256, "4 waves x 2 tiles x 32 units; 4 K quarters of 64");

struct SacRowsLds {
  float in[kRwRows][kWsXDim];                      // the rows' inputs: a record's x field
  float f1[kRwRows][kRwStride];                    // h1, then d1
  float f2[kRwRows][kRwStride];                    // h2, then d2
  __attribute__((aligned(16))) float head[kRwRows][4];   // layer-3 outputs [row][output] (sac_rows_head: why 4)
  float gout[kRwRows][2];                          // the output gradients
  float ga[kRwRows];                               // the policy step's gradient at the action input
};
static_assert(sizeof(SacRowsLds) <= 80 * 1024, "two blocks per CU");

// sac_gaussian_head (sit_sac.h) reads a row's two outputs as S.head[2 j], S.head[2 j + 1] of a SacLds.  Here
// it is given j = 0 and the SacLds whose head member starts at this row's outputs: rows are 16 bytes apart
// (SacLds's alignment), the member's 16 floats lie inside SacRowsLds (gout follows head), and so does the
// rest of that SacLds, which is never touched, because head lies deeper in SacRowsLds than in SacLds.
static_assert(offsetof(SacRowsLds, head) >= offsetof(SacLds, head) && offsetof(SacLds, head) % 16 == 0 &&
                  sizeof(SacRowsLds) - offsetof(SacRowsLds, head[kRwRows - 1]) >= sizeof(SacLds) - offsetof(SacLds, head),
              "a SacLds around every row of head lies inside SacRowsLds");

template <typename T>
__device__ __forceinline__ SacHead sac_rows_head(const SacRowsLds& S, int r, int row, bool live, const T* noise,
                                                 uint64_t seed, uint64_t update, uint32_t tag) {
  const SacLds& view =
      *reinterpret_cast<const SacLds*>(reinterpret_cast<const char*>(&S.head[r][0]) - offsetof(SacLds, head));
  return sac_gaussian_head<T>(view, 0, row, live, noise, seed, update, tag);
}

// The block's rows [row0, row0 + nrow) of `state` into S.in, zeros past nrow (nrow may be anything <= kRwRows);
// column kActorObs is the row's `extra` (nullptr: zero), the padding column zero.  The caller's barrier follows.
template <typename T>
__device__ __forceinline__ void sac_rows_stage(SacRowsLds& S, const T* state, const T* extra, int row0, int nrow) {
  for (int e = threadIdx.x; e < kRwRows * kWsXDim; e += 256) {
    const int r = e / kWsXDim, i = e % kWsXDim;
    float v = 0.0f;
    if (r < nrow) {
      if (i < kActorObs) v = (float)state[(size_t)(row0 + r) * kActorObs + i];
      else if (i == kActorObs && extra) v = (float)extra[row0 + r];
    }
    S.in[r][i] = v;
  }
}

constexpr int kRwSteps = 2;                        // forward: k pairs per K quarter and prefetch group
constexpr int kRwCols = 8;                         // backward: float4 columns per prefetch group

struct SacRowsFwdOps {
  float a[kRwSteps][4];                            // [k pair][K quarter]: h1[lane & 31][64 q + 2 s + (lane >> 5)]
  float2 b[kRwSteps][4];                           // W2T[the same k][64 w + 2 (lane & 31) + {0, 1}]
};

// A group's weight operands (global) and its activation operands (LDS) are loaded apart: the first group's
// weights are asked for before layer 1, whose barrier the activations have to wait for.
__device__ __forceinline__ void sac_rows_fwd_load_b(const float* b_at, int s0, SacRowsFwdOps& o) {
#pragma unroll
  for (int u = 0; u < kRwSteps; ++u)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      o.b[u][q] = *reinterpret_cast<const float2*>(b_at + (size_t)(64 * q + 2 * (s0 + u)) * kActorHidden);
}

__device__ __forceinline__ void sac_rows_fwd_load_a(const float* a_at, int s0, SacRowsFwdOps& o) {
#pragma unroll
  for (int u = 0; u < kRwSteps; ++u)
#pragma unroll
    for (int q = 0; q < 4; ++q) o.a[u][q] = a_at[64 * q + 2 * (s0 + u)];
  // (as in sac_wgrad_load: the loads stay ahead of the MFMAs that follow in program order)
  __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ void sac_rows_fwd_load(const float* a_at, const float* b_at, int s0, SacRowsFwdOps& o) {
  sac_rows_fwd_load_b(b_at, s0, o);
  sac_rows_fwd_load_a(a_at, s0, o);
}

__device__ __forceinline__ void sac_rows_fwd_mfma(const SacRowsFwdOps& o, SacAcc (&acc)[4][2]) {
#pragma unroll
  for (int u = 0; u < kRwSteps; ++u)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      acc[q][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.a[u][q], o.b[u][q].x, acc[q][0], 0, 0, 0);
      acc[q][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.a[u][q], o.b[u][q].y, acc[q][1], 0, 0, 0);
    }
  __builtin_amdgcn_sched_barrier(0);
}

struct SacRowsBwdOps {
  float a[kRwCols][2];                             // d2[lane & 31][4 m + 2 p + (lane >> 5)]
  float4 b[kRwCols][2];                            // [column m][tile]: W2T[k of the lane][4 m .. 4 m + 3]
};

__device__ __forceinline__ void sac_rows_bwd_load(const float* a_at, const float* b_at, int m0, SacRowsBwdOps& o) {
#pragma unroll
  for (int u = 0; u < kRwCols; ++u) {
    const int n = 4 * (m0 + u);
#pragma unroll
    for (int t = 0; t < 2; ++t) o.b[u][t] = *reinterpret_cast<const float4*>(b_at + (size_t)t * 32 * kActorHidden + n);
    o.a[u][0] = a_at[n];
    o.a[u][1] = a_at[n + 2];
  }
  __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ void sac_rows_bwd_mfma(const SacRowsBwdOps& o, bool high, SacAcc (&acc)[2]) {
#pragma unroll
  for (int u = 0; u < kRwCols; ++u) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.a[u][0], high ? o.b[u][t].y : o.b[u][t].x, acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 2; ++t)
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.a[u][1], high ? o.b[u][t].w : o.b[u][t].z, acc[t], 0, 0, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
}

// The forward pass of one MLP over the block's 32 rows: reads S.in[r][0..IN), leaves h1 in S.f1, h2 in S.f2 and
// the outputs in S.head[r][o].  Called by all 256 threads with S.in complete (a barrier behind its last
// write); ends with a barrier.
template <int IN, int NOUT>
__device__ __forceinline__ void sac_rows_mlp(const float* __restrict__ w, SacRowsLds& S) {
#pragma clang fp reassociate(off) contract(off)
  using N = SacNet<IN, NOUT>;
  constexpr int H = kActorHidden, R = kRwRows;
  const int j = threadIdx.x, lane = j & 63, col = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(j >> 6);
  const float* a_at = &S.f1[col][half];
  const float* b_at = w + N::W2T + (size_t)half * H + 64 * wave + 2 * col;
  SacRowsFwdOps o0, o1;
  sac_rows_fwd_load_b(b_at, 0, o0);
  __builtin_amdgcn_sched_barrier(0);
  // layer 1: h1 = relu(W1 x + b1), thread j = hidden unit j
  {
    float wr[IN];
#pragma unroll
    for (int i = 0; i < IN; ++i) wr[i] = w[N::W1 + j * IN + i];
    const float b1 = w[N::B1 + j];
#pragma unroll 4
    for (int r = 0; r < R; ++r) {
      float acc = 0.0f;
#pragma unroll
      for (int i = 0; i < IN; ++i) acc = __builtin_fmaf(wr[i], S.in[r][i], acc);
      S.f1[r][j] = __builtin_fmaxf(acc + b1, 0.0f);
    }
  }
  __syncthreads();
  // layer 2 on the matrix cores (the lane maps: the head of this file).  Two register buffers in turn, each
  // loaded one group of MFMAs ahead of its use; the last pair of groups is peeled so that every wait in the
  // loop counts the loads that are in flight behind the ones it needs.
  {
    SacAcc acc[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[q][t][e] = 0.0f;
    sac_rows_fwd_load_a(a_at, 0, o0);
    int s0 = 0;
#pragma unroll 1
    for (; s0 + 2 * kRwSteps < 32; s0 += 2 * kRwSteps) {
      sac_rows_fwd_load(a_at, b_at, s0 + kRwSteps, o1);
      sac_rows_fwd_mfma(o0, acc);
      sac_rows_fwd_load(a_at, b_at, s0 + 2 * kRwSteps, o0);
      sac_rows_fwd_mfma(o1, acc);
    }
    sac_rows_fwd_load(a_at, b_at, s0 + kRwSteps, o1);
    sac_rows_fwd_mfma(o0, acc);
    sac_rows_fwd_mfma(o1, acc);
    // C/D element (e, lane) is row (e & 3) + 8 (e >> 2) + 4 (lane >> 5), column lane & 31
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int n = 64 * wave + 2 * col + t;
      const float b2 = w[N::B2 + n];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = (e & 3) + 8 * (e >> 2) + 4 * half;
        S.f2[r][n] = __builtin_fmaxf(((acc[0][t][e] + acc[1][t][e]) + (acc[2][t][e] + acc[3][t][e])) + b2, 0.0f);
      }
    }
  }
  __syncthreads();
  // layer 3: (row, output) pairs x 16 lanes, each lane 16 units, then a 16-lane reduction; 16 pairs a pass
  {
    const int c = j & 15;
#pragma unroll
    for (int p0 = 0; p0 < R * NOUT; p0 += 16) {
      const int pr = p0 + (j >> 4);
      const int r = pr / NOUT, o = pr % NOUT;
      const float* v = w + N::W3 + o * H + c * 16;
      float sum = 0.0f;
#pragma unroll
      for (int i = 0; i < 16; ++i) sum = __builtin_fmaf(S.f2[r][c * 16 + i], v[i], sum);
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 16);
      if (c == 0) S.head[r][o] = sum + w[N::B3 + o];
    }
  }
  __syncthreads();
}

// d2 of one MLP from the output gradients S.gout[r][o], in place over h2 in S.f2, thread j = unit n.  store: the
// thread first stores h1 and h2 of rows < nrow to the records `rec` (the backward pass overwrites both).
// Called by all 256 threads with S.gout complete (a barrier behind its last write); the caller's barrier follows.
template <int IN, int NOUT>
__device__ __forceinline__ void sac_rows_d2(const float* __restrict__ w, SacRowsLds& S, float* rec, int nrow, bool store) {
#pragma clang fp reassociate(off) contract(off)
  using N = SacNet<IN, NOUT>;
  constexpr int H = kActorHidden, R = kRwRows;
  const int j = threadIdx.x;
  if (store)
    for (int r = 0; r < nrow; ++r) {
      float* p = rec + (size_t)r * kWsRow;
      p[kWsH1 + j] = S.f1[r][j];
      p[kWsH2 + j] = S.f2[r][j];
    }
  float w3[NOUT];
#pragma unroll
  for (int o = 0; o < NOUT; ++o) w3[o] = w[N::W3 + o * H + j];
#pragma unroll 4
  for (int r = 0; r < R; ++r) {
    float d = 0.0f;
#pragma unroll
    for (int o = 0; o < NOUT; ++o) d = __builtin_fmaf(w3[o], S.gout[r][o], d);
    S.f2[r][j] = S.f2[r][j] > 0.0f ? d : 0.0f;
  }
}

// d1 of one MLP on the matrix cores, in place over h1 in S.f1, from d2 in S.f2.  Called by all 256 threads with
// S.f2 complete and S.f1 no longer needed as h1 by any other thread (a barrier behind both); ends with a
// barrier.
template <int IN, int NOUT>
__device__ __forceinline__ void sac_rows_d1(const float* __restrict__ w, SacRowsLds& S) {
#pragma clang fp reassociate(off) contract(off)
  using N = SacNet<IN, NOUT>;
  constexpr int H = kActorHidden;
  const int j = threadIdx.x, lane = j & 63, col = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(j >> 6);
  const float* a_at = &S.f2[col][half];
  const float* b_at = w + N::W2T + (size_t)(64 * wave + col) * H;
  SacAcc acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.0f;
  SacRowsBwdOps o0, o1;
  sac_rows_bwd_load(a_at, b_at, 0, o0);
  int m0 = 0;
#pragma unroll 1
  for (; m0 + 2 * kRwCols < H / 4; m0 += 2 * kRwCols) {
    sac_rows_bwd_load(a_at, b_at, m0 + kRwCols, o1);
    sac_rows_bwd_mfma(o0, half != 0, acc);
    sac_rows_bwd_load(a_at, b_at, m0 + 2 * kRwCols, o0);
    sac_rows_bwd_mfma(o1, half != 0, acc);
  }
  sac_rows_bwd_load(a_at, b_at, m0 + kRwCols, o1);
  sac_rows_bwd_mfma(o0, half != 0, acc);
  sac_rows_bwd_mfma(o1, half != 0, acc);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int k = 64 * wave + 32 * t + col;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int r = (e & 3) + 8 * (e >> 2) + 4 * half;
      S.f1[r][k] = S.f1[r][k] > 0.0f ? acc[t][e] : 0.0f;
    }
  }
  __syncthreads();
}

// d1 and d2 of rows < nrow from S.f1, S.f2 to the records, thread j = unit j
__device__ __forceinline__ void sac_rows_store_deltas(float* rec, int nrow, const SacRowsLds& S) {
  const int j = threadIdx.x;
  for (int r = 0; r < nrow; ++r) {
    float* p = rec + (size_t)r * kWsRow;
    p[kWsD1 + j] = S.f1[r][j];
    p[kWsD2 + j] = S.f2[r][j];
  }
}

// the x field of the block's records: columns [0, n) of S.in's rows, zeros behind them
__device__ __forceinline__ void sac_rows_store_x(float* rec, int nrow, const SacRowsLds& S, int n) {
  for (int e = threadIdx.x; e < kRwRows * kWsXDim; e += 256) {
    const int r = e / kWsXDim, i = e % kWsXDim;
    if (r < nrow) rec[(size_t)r * kWsRow + kWsX + i] = i < n ? S.in[r][i] : 0.0f;
  }
}

#define SAC_ROWS_LDS(S)                                                  \
  extern __shared__ __align__(16) unsigned char sac_rows_smem[];         \
  SacRowsLds& S = *reinterpret_cast<SacRowsLds*>(sac_rows_smem)

template <typename T, bool CLOCKED = false>
__global__ __launch_bounds__(256, 2) void k_sac_target_wide(const SacRowArgs<SacTarget<T>, CLOCKED> a) {
#pragma clang fp reassociate(off) contract(off)
  constexpr int R = kRwRows;
  SAC_ROWS_LDS(S);
  const int j = threadIdx.x;
  const int row0 = blockIdx.x * R;
  const int nrow = min(R, a.batch - row0);    // >= 1: the grid is ceil(batch / R) blocks
  sac_rows_stage<T>(S, a.next_state, nullptr, row0, nrow);
  __syncthreads();
  sac_rows_mlp<kActorObs, 2>(a.actor, S);
  float logp = 0.0f, act = 0.0f;
  if (j < R) {
    uint64_t update;
    if constexpr (CLOCKED) update = a.tick->update; else update = a.update;
    const SacHead hd = sac_rows_head(S, j, row0 + j, j < nrow, a.noise, a.seed, update, kSacTag);
    act = hd.act;
    logp = hd.logp;
    S.in[j][kActorObs] = act;
  }
  __syncthreads();
  sac_rows_mlp<kSacIn, 1>(a.critic, S);
  const float q1 = j < R ? S.head[j][0] : 0.0f;
  sac_rows_mlp<kSacIn, 1>(a.critic + SIT_CRITIC_WEIGHTS, S);
  if (j < nrow) {
    const float q2 = S.head[j][0];
    const int row = row0 + j;
    const T soft = (T)__builtin_fminf(q1, q2) - (T)(*a.alpha) * (T)logp;
    a.y[row] = a.reward_scale * a.reward[row] + a.mask[row] * a.gamma * soft;
    if (a.next_action) a.next_action[row] = (T)act;
    if (a.next_logp) a.next_logp[row] = (T)logp;
    if (a.q1) a.q1[row] = (T)q1;
    if (a.q2) a.q2[row] = (T)q2;
  }
}

template <typename T>
__global__ __launch_bounds__(256, 2) void k_sac_critic_fb_wide(const SacCriticFb<T> a) {
#pragma clang fp reassociate(off) contract(off)
  constexpr int R = kRwRows;
  SAC_ROWS_LDS(S);
  const int j = threadIdx.x;
  const int row0 = blockIdx.x * R;
  const int nrow = min(R, a.batch - row0);    // >= 1: the grid is ceil(batch / R) blocks
  sac_rows_stage<T>(S, a.state, a.action, row0, nrow);
  const float yv = j < nrow ? (float)a.y[row0 + j] : 0.0f;
  __syncthreads();
#pragma unroll 1
  for (int c = 0; c < 2; ++c) {
    const float* w = a.critic + (size_t)c * SIT_CRITIC_WEIGHTS;
    float* rec = sac_ws_rows(a.ws, a.batch, c, row0);
    sac_rows_mlp<kSacIn, 1>(w, S);
    if (j < R) {
      float g = 0.0f, sq = 0.0f;
      const float diff = S.head[j][0] - yv;
      if (j < nrow) {
        g = (2.0f * diff) / (float)a.batch;
        sq = diff * diff;
        float* p = rec + (size_t)j * kWsRow + kWsG;
        p[0] = g; p[1] = 0.0f; p[2] = sq; p[3] = 0.0f;
      }
      S.gout[j][0] = g;
    }
    sac_rows_store_x(rec, nrow, S, kWsXDim);
    __syncthreads();
    sac_rows_d2<kSacIn, 1>(w, S, rec, nrow, true);
    __syncthreads();
    sac_rows_d1<kSacIn, 1>(w, S);
    sac_rows_store_deltas(rec, nrow, S);
    __syncthreads();                          // the records are read before the next pass overwrites the LDS
  }
}

template <typename T, bool CLOCKED = false>
__global__ __launch_bounds__(256, 2) void k_sac_policy_fb_wide(const SacRowArgs<SacPolicyFb<T>, CLOCKED> a) {
#pragma clang fp reassociate(off) contract(off)
  constexpr int R = kRwRows;
  SAC_ROWS_LDS(S);
  const int j = threadIdx.x;
  const int row0 = blockIdx.x * R;
  const int nrow = min(R, a.batch - row0);
  float* rec = sac_ws_rows(a.ws, a.batch, 0, row0);
  sac_rows_stage<T>(S, a.state, nullptr, row0, nrow);
  __syncthreads();
  sac_rows_mlp<kActorObs, 2>(a.actor, S);
  // the actor's activations go to the records now: the critics run through the same LDS
  // (column 10 of S.in receives the action below: the actor's record holds zeros there)
  for (int r = 0; r < nrow; ++r) {
    float* p = rec + (size_t)r * kWsRow;
    p[kWsH1 + j] = S.f1[r][j];
    p[kWsH2 + j] = S.f2[r][j];
  }
  sac_rows_store_x(rec, nrow, S, kActorObs);
  // the squashed Gaussian head, thread j < R = row j (rows past nrow: on zeros)
  SacHead hd{};
  if (j < R) {
    uint64_t update;
    if constexpr (CLOCKED) update = a.tick->update; else update = a.update;
    hd = sac_rows_head(S, j, row0 + j, j < nrow, a.noise, a.seed, update, kSacPolicyTag);
    S.in[j][kActorObs] = hd.act;
  }
  __syncthreads();
  // both critics at (state, a), each taken back to the action input from an output gradient of -1/B
  float q[2] = {0.0f, 0.0f}, ga[2] = {0.0f, 0.0f};
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const float* w = a.critic + (size_t)c * SIT_CRITIC_WEIGHTS;
    sac_rows_mlp<kSacIn, 1>(w, S);
    if (j < R) {
      q[c] = S.head[j][0];
      S.gout[j][0] = j < nrow ? -1.0f / (float)a.batch : 0.0f;
    }
    __syncthreads();
    sac_rows_d2<kSacIn, 1>(w, S, nullptr, 0, false);
    __syncthreads();
    sac_rows_d1<kSacIn, 1>(w, S);
    // g_a[r] = sum_j W1[j][10] d1[r][j]: 16 lanes per row, each 16 units, then a 16-lane reduction
    {
      const int cl = j & 15;
#pragma unroll
      for (int r0 = 0; r0 < R; r0 += 16) {
        const int r = r0 + (j >> 4);
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int u = cl * 16 + i;
          sum = __builtin_fmaf(w[SacNet<kSacIn, 1>::W1 + u * kSacIn + kActorObs], S.f1[r][u], sum);
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 16);
        if (cl == 0) S.ga[r] = sum;
      }
    }
    __syncthreads();
    if (j < R) ga[c] = S.ga[j];
  }
  if (j < R) {
    const float alpha = *a.alpha;
    const bool first = q[0] <= q[1];
    const float gsel = first ? ga[0] : ga[1], qmin = first ? q[0] : q[1];
    const float ab = alpha / (float)a.batch;
    const float dx = ab * (((2.0f * hd.act) * hd.s) / (hd.s + 1e-6f)) + gsel * hd.s;
    float dmu = dx, dls = (dx * hd.sig) * hd.eps - ab;
    if (hd.ls_raw < -20.0f || hd.ls_raw > 2.0f) dls = 0.0f;
    if (j >= nrow) { dmu = 0.0f; dls = 0.0f; }
    S.gout[j][0] = dmu;
    S.gout[j][1] = dls;
    if (j < nrow) {
      float* p = rec + (size_t)j * kWsRow + kWsG;
      p[0] = dmu; p[1] = dls; p[2] = alpha * hd.logp - qmin; p[3] = hd.logp;
    }
  }
  // the actor's activations back from the records (each thread reads what it wrote)
#pragma unroll 4
  for (int r = 0; r < R; ++r) {
    const float* p = rec + (size_t)r * kWsRow;
    S.f1[r][j] = r < nrow ? p[kWsH1 + j] : 0.0f;
    S.f2[r][j] = r < nrow ? p[kWsH2 + j] : 0.0f;
  }
  __syncthreads();
  sac_rows_d2<kActorObs, 2>(a.actor, S, nullptr, 0, false);
  __syncthreads();
  sac_rows_d1<kActorObs, 2>(a.actor, S);
  sac_rows_store_deltas(rec, nrow, S);
}

#undef SAC_ROWS_LDS

// ---- launches -------------------------------------------------------------------------------

// A wide row kernel over `batch` rows.  Its dynamic LDS is above the 64 KiB a launch may ask for unannounced,
// so the attribute is set once per handle and kernel (`slot`), not per launch (launches may be captured).
template <typename A>
int sac_rows_launch(sit_handle* h, int slot, void (*kern)(const A), int batch, const A& a, hipStream_t stream) {
  if (!h->lds_attr_rows[slot]) {
    HIP_TRY(h, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(SacRowsLds)));
    h->lds_attr_rows[slot] = true;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)((batch + kRwRows - 1) / kRwRows)), dim3(256), sizeof(SacRowsLds), stream, a);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
}

template <typename T>
int sac_launch_target_wide(sit_handle* h, const sit_sac_target_args* s, hipStream_t stream) {
  SacTarget<T> a{};
  a.batch = s->batch;
  a.seed = s->seed;
  a.update = s->update;
  a.gamma = (T)s->gamma;
  a.reward_scale = (T)s->reward_scale;
  a.actor = s->actor_weights;
  a.critic = s->critic_weights;
  a.alpha = s->alpha;
  a.next_state = (const T*)s->next_state;
  a.reward = (const T*)s->reward;
  a.mask = (const T*)s->mask;
  a.noise = (const T*)s->noise;
  a.y = (T*)s->y;
  a.next_action = (T*)s->next_action;
  a.next_logp = (T*)s->next_logp;
  a.q1 = (T*)s->q1;
  a.q2 = (T*)s->q2;
  return sac_rows_launch(h, 0, k_sac_target_wide<T>, s->batch, a, stream);
}

// the wide row kernel, then k_sac_wgrad_adam as the _tiled call launches it
template <typename T>
int sac_launch_critic_step_wide(sit_handle* h, const sit_sac_critic_step_args* s, hipStream_t stream) {
  SacCriticFb<T> f{};
  f.batch = s->batch;
  f.critic = s->critic_weights;
  f.state = (const T*)s->state;
  f.action = (const T*)s->action;
  f.y = (const T*)s->y;
  f.ws = s->workspace;
  if (int rc = sac_rows_launch(h, 1, k_sac_critic_fb_wide<T>, s->batch, f, stream)) return rc;
  SacAdam a{};
  a.batch = s->batch;
  a.p = s->critic_weights; a.m = s->critic_m; a.v = s->critic_v;
  a.ws = s->workspace;
  a.results = s->results;
  a.o = sac_adam_scalars(s->adam);
  return sac_launch_adam(h, sac_adam_launch<kSacIn, 1, 2, SIT_CRITIC_WEIGHTS, false>(true), a, stream);
}

template <typename T>
int sac_launch_policy_step_wide(sit_handle* h, const sit_sac_policy_step_args* s, hipStream_t stream) {
  SacPolicyFb<T> f{};
  f.batch = s->batch;
  f.seed = s->seed;
  f.update = s->update;
  f.actor = s->actor_weights;
  f.critic = s->critic_weights;
  f.alpha = s->alpha;
  f.state = (const T*)s->state;
  f.noise = (const T*)s->noise;
  f.ws = s->workspace;
  if (int rc = sac_rows_launch(h, 2, k_sac_policy_fb_wide<T>, s->batch, f, stream)) return rc;
  SacAdam a{};
  a.batch = s->batch;
  a.p = s->actor_weights; a.m = s->actor_m; a.v = s->actor_v;
  a.ws = s->workspace;
  a.results = s->results;
  a.o = sac_adam_scalars(s->adam);
  a.tune = s->tune != 0;
  a.target_entropy = (float)s->target_entropy;
  a.alpha = s->alpha;
  if (a.tune) {
    a.log_alpha = s->log_alpha; a.log_alpha_m = s->log_alpha_m; a.log_alpha_v = s->log_alpha_v;
    a.oa = sac_adam_scalars(s->alpha_adam);
  }
  return sac_launch_adam(h, sac_adam_launch<kActorObs, 2, 1, SIT_ACTOR_WEIGHTS, true>(true), a, stream);
}

// ---- many updates per call from the device clock (include/sit.h: sit_sac_updates; sit_sac_clock.h) ----------
//
// One k_sac_clock_begin forms tick slot 0 from the clock's state words; update u of the call then reads slot
// u & 1 in five launches: target rows, critic rows, critics' Adam (+ Polyak), policy rows, actor's Adam (+ the
// temperature step, the clock's advance and the next tick in slot (u + 1) & 1).  The slot is a by-value
// argument and the launches of a stream run in order, so a tick is complete before anything reads it and is
// not written while anything may.  The wide row kernels' clocked instantiations are kernels of their own and
// take slots 3, 4 of the handle's lds_attr_rows (sac_rows_launch).

__global__ void k_sac_clock_begin(int64_t* clock, const SacClockHyper hy) {
  if (blockIdx.x == 0 && threadIdx.x == 0) sac_clock_form_tick(clock, hy, 0);
}

// the scalars of steps t0 .. t0 + n - 1 as the device forms them (the specification's test hook)
__global__ __launch_bounds__(256) void k_sac_adam_scalars(const sit_sac_adam o, int64_t t0, int n, float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const SacAdamScalars s = sac_clock_scalars(o, t0 + i);
  float* p = out + (size_t)i * 6;
  p[0] = s.one_minus_beta1; p[1] = s.beta2; p[2] = s.one_minus_beta2;
  p[3] = s.step_size; p[4] = s.sqrt_bias2; p[5] = s.eps;
}

inline int sac_launch_adam_scalars(sit_handle* h, const sit_sac_adam* o, int64_t t0, int32_t n, float* out,
                                   hipStream_t stream) {
  hipLaunchKernelGGL(k_sac_adam_scalars, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, *o, t0, (int)n, out);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
}

template <typename T>
int sac_launch_updates(sit_handle* h, const sit_sac_updates_args* s, hipStream_t stream) {
  const bool tiled = s->mode != SIT_SAC_UPDATES_PLAIN, wide = s->mode == SIT_SAC_UPDATES_WIDE;
  const int B = s->batch;
  const unsigned narrow_blocks = (unsigned)((B + kSacRows - 1) / kSacRows);
  SacClockHyper hy{};
  hy.adam[kClockCritic] = s->critic_adam;
  hy.adam[kClockPolicy] = s->actor_adam;
  hy.adam[kClockAlpha] = s->tune ? s->alpha_adam : s->actor_adam;   // (untuned: formed, never used)
  hy.target_update_interval = s->target_update_interval;
  hy.results_capacity = s->results_capacity;
  hy.tune = s->tune != 0;
  hipLaunchKernelGGL(k_sac_clock_begin, dim3(1), dim3(64), 0, stream, s->clock, hy);
  HIP_TRY(h, hipGetLastError());

  const SacAdamClockLaunch critic_adam = sac_adam_clocked_launch<kSacIn, 1, 2, SIT_CRITIC_WEIGHTS, false>(tiled);
  const SacAdamClockLaunch actor_adam = sac_adam_clocked_launch<kActorObs, 2, 1, SIT_ACTOR_WEIGHTS, true>(tiled);
  for (int u = 0; u < s->n_updates; ++u) {
    const size_t row0 = (size_t)u * (size_t)B;
    const SacTick* tick = sac_clock_tick(s->clock, u & 1);
    const T* state = (const T*)s->state + row0 * kActorObs;

    SacClocked<SacTarget<T>> t{};
    t.tick = tick;
    t.batch = B;
    t.seed = s->seed;
    t.gamma = (T)s->gamma;
    t.reward_scale = (T)s->reward_scale;
    t.actor = s->actor_weights;
    t.critic = s->target_weights;
    t.alpha = s->alpha;
    t.next_state = (const T*)s->next_state + row0 * kActorObs;
    t.reward = (const T*)s->reward + row0;
    t.mask = (const T*)s->mask + row0;
    t.y = (T*)s->y;
    if (wide) {
      if (int rc = sac_rows_launch(h, 3, k_sac_target_wide<T, true>, B, t, stream)) return rc;
    } else {
      hipLaunchKernelGGL((k_sac_target<T, true>), dim3(narrow_blocks), dim3(256), 0, stream, t);
      HIP_TRY(h, hipGetLastError());
    }

    SacCriticFb<T> cf{};
    cf.batch = B;
    cf.critic = s->critic_weights;
    cf.state = state;
    cf.action = (const T*)s->action + row0;
    cf.y = (const T*)s->y;
    cf.ws = s->workspace;
    if (wide) {
      if (int rc = sac_rows_launch(h, 1, k_sac_critic_fb_wide<T>, B, cf, stream)) return rc;
    } else {
      hipLaunchKernelGGL(k_sac_critic_fb<T>, dim3(narrow_blocks), dim3(256), 0, stream, cf);
      HIP_TRY(h, hipGetLastError());
    }
    SacAdamClock k{};
    k.clock = s->clock;
    k.slot = u & 1;
    k.target = s->target_weights;
    k.tau = (float)s->tau;
    k.hy = hy;
    SacAdam ca{};
    ca.batch = B;
    ca.p = s->critic_weights; ca.m = s->critic_m; ca.v = s->critic_v;
    ca.ws = s->workspace;
    ca.results = s->results;
    if (int rc = sac_launch_adam_clocked(h, critic_adam, ca, k, stream)) return rc;

    SacClocked<SacPolicyFb<T>> pf{};
    pf.tick = tick;
    pf.batch = B;
    pf.seed = s->seed;
    pf.actor = s->actor_weights;
    pf.critic = s->critic_weights;
    pf.alpha = s->alpha;
    pf.state = state;
    pf.ws = s->workspace;
    if (wide) {
      if (int rc = sac_rows_launch(h, 4, k_sac_policy_fb_wide<T, true>, B, pf, stream)) return rc;
    } else {
      hipLaunchKernelGGL((k_sac_policy_fb<T, true>), dim3(narrow_blocks), dim3(256), 0, stream, pf);
      HIP_TRY(h, hipGetLastError());
    }
    SacAdam pa{};
    pa.batch = B;
    pa.p = s->actor_weights; pa.m = s->actor_m; pa.v = s->actor_v;
    pa.ws = s->workspace;
    pa.results = s->results;
    pa.tune = s->tune != 0;
    pa.target_entropy = (float)s->target_entropy;
    pa.alpha = s->alpha;
    if (pa.tune) { pa.log_alpha = s->log_alpha; pa.log_alpha_m = s->log_alpha_m; pa.log_alpha_v = s->log_alpha_v; }
    if (int rc = sac_launch_adam_clocked(h, actor_adam, pa, k, stream)) return rc;
  }
  return SIT_OK;
}

}  // namespace

#endif  // SIT_SAC_ROWS_H
