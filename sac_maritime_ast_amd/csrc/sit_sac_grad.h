// sit_sac_grad.h — the gradient half of a SAC update (include/sit.h: sit_sac_critic_step,
// sit_sac_policy_step): forward and backward passes of the three MLPs and their Adam steps.
//
// Two kernels per call.  k_sac_critic_fb / k_sac_policy_fb have the shape of k_sac_target (sit_sac.h): one
// block of 256 threads per kSacRows minibatch rows, the networks one after another through the same LDS
// by sac_mlp, then sac_mlp_backward in the same block (rows are independent); staging the rows and the
// squashed Gaussian head are sit_sac.h's (sac_stage_rows, sac_gaussian_head).  Each block leaves its rows'
// records in the caller's float32 workspace, kWsRow floats per row and network pass (the layout: sit_sac.h,
// next to SacNet).
// k_sac_adam then runs one thread per element of a packed parameter block: the element's gradient is
// the sum over b = 0 .. B-1, ascending, of the two record fields sac_segment (sit_sac.h) names for its
// segment, (delta of its output unit) x (activation of its input unit), and Adam is applied to p, m, v in
// place; the gradient is never stored and the padding floats of a block are not touched.  Thread 0 of one
// extra block adds up the per-row loss terms in ascending row order (in float64); sac_finish_losses then
// writes the losses and in the actor's launch takes the temperature step (lp, la, alpha).
//
// Backward layer 2 is a dot over a contiguous row of W2^T (thread k = input unit k).  Every sum has a
// fixed order, there are no atomics, and no row's arithmetic depends on another row, so the result does
// not depend on how blocks are scheduled.  Rows past B in the last block run on zeros with zero output
// gradients and are neither read from nor written to global memory.
//
// k_sac_policy_fb and k_sac_adam have a CLOCKED instantiation for sit_sac_updates (sit_sac_clock.h): the update
// number, the Adam scalars and the results row then come from the device clock's tick; the critics' Adam launch
// also applies the Polyak update and the actor's finishing thread advances the clock.  The instantiations
// without it are the kernels as they were before there was a clock.
//
// Included from sit_kernels.hip only (the strictly compiled translation unit).
#ifndef SIT_SAC_GRAD_H
#define SIT_SAC_GRAD_H

#include "sit_sac.h"

namespace {

constexpr uint32_t kSacPolicyTag = 0x5049u;   // counter word 1 of the policy loss's noise draw

struct SacGradLds {
  SacLds S;
  float gout[2 * kSacRows];   // the output gradients, [row][output]
  float ga[kSacRows];         // the policy step's gradient at the action input
};
static_assert(sizeof(SacGradLds) <= 64 * 1024, "static LDS limit");

// Backward of one MLP over the block's rows from the output gradients gout[r * NOUT + o], with the
// forward activations in S.h1, S.h2: leaves d2 in S.part[0] and d1 in S.part[1].  Called by all 256
// threads with gout complete (a barrier behind its last write); ends with a barrier.
template <int IN, int NOUT>
__device__ __forceinline__ void sac_mlp_backward(const float* __restrict__ w, SacLds& S, const float* gout) {
#pragma clang fp reassociate(off) contract(off)
  using N = SacNet<IN, NOUT>;
  constexpr int H = kActorHidden, R = kSacRows;
  const int j = threadIdx.x;
  // d2[r][n] = (sum_o W3[o][n] g[r][o]) [h2[r][n] > 0], thread j = unit n
  {
    float w3[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) w3[o] = w[N::W3 + o * H + j];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float d = 0.0f;
#pragma unroll
      for (int o = 0; o < NOUT; ++o) d = __builtin_fmaf(w3[o], gout[r * NOUT + o], d);
      S.part[0][r][j] = S.h2[r][j] > 0.0f ? d : 0.0f;
    }
  }
  __syncthreads();
  // d1[r][k] = (sum_n W2T[k][n] d2[r][n]) [h1[r][k] > 0], thread j = unit k: row k of W2^T is contiguous,
  // the deltas are wave-uniform LDS broadcasts
  {
    const float4* wrow = reinterpret_cast<const float4*>(w + N::W2T + (size_t)j * H);
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0f;
#pragma unroll 4
    for (int n4 = 0; n4 < H / 4; ++n4) {
      const float4 wv = wrow[n4];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float4 dv = *reinterpret_cast<const float4*>(&S.part[0][r][4 * n4]);
        acc[r] = __builtin_fmaf(wv.x, dv.x, acc[r]);
        acc[r] = __builtin_fmaf(wv.y, dv.y, acc[r]);
        acc[r] = __builtin_fmaf(wv.z, dv.z, acc[r]);
        acc[r] = __builtin_fmaf(wv.w, dv.w, acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) S.part[1][r][j] = S.h1[r][j] > 0.0f ? acc[r] : 0.0f;
  }
  __syncthreads();
}

// the block's records of one network pass: rows [row0, row0 + nrow) of pass `pass`
__device__ __forceinline__ float* sac_ws_rows(float* ws, int batch, int pass, int row0) {
  return ws + ((size_t)pass * (size_t)batch + (size_t)row0) * kWsRow;
}

// two 256-wide fields of the block's records from their LDS arrays, thread j = unit j
__device__ __forceinline__ void sac_store_fields(float* rec, int nrow, int at0, const float (&v0)[kSacRows][kActorHidden],
                                                 int at1, const float (&v1)[kSacRows][kActorHidden]) {
  const int j = threadIdx.x;
  for (int r = 0; r < nrow; ++r) {
    float* p = rec + (size_t)r * kWsRow;
    p[at0 + j] = v0[r][j];
    p[at1 + j] = v1[r][j];
  }
}

// the x field of the block's records: columns [0, n) of S.in's rows, zeros behind them
__device__ __forceinline__ void sac_store_x(float* rec, int nrow, const SacLds& S, int n) {
  const int j = threadIdx.x;
  if (j < kSacRows * kWsXDim) {
    const int r = j / kWsXDim, i = j % kWsXDim;
    if (r < nrow) rec[(size_t)r * kWsRow + kWsX + i] = i < n ? S.in[r][i] : 0.0f;
  }
}

template <typename T>
struct SacCriticFb {
  int batch;
  const float* critic;
  const T *state, *action, *y;
  float* ws;
};

template <typename T>
__global__ __launch_bounds__(256) void k_sac_critic_fb(const SacCriticFb<T> a) {
#pragma clang fp reassociate(off) contract(off)
  constexpr int R = kSacRows;
  __shared__ SacGradLds G;
  SacLds& S = G.S;
  const int j = threadIdx.x;
  const int row0 = blockIdx.x * R;
  const int nrow = min(R, a.batch - row0);    // >= 1: the grid is ceil(batch / R) blocks
  sac_stage_rows<T>(S, a.state, a.action, row0, nrow);
  const float yv = j < nrow ? (float)a.y[row0 + j] : 0.0f;
  __syncthreads();
#pragma unroll 1
  for (int c = 0; c < 2; ++c) {
    const float* w = a.critic + (size_t)c * SIT_CRITIC_WEIGHTS;
    sac_mlp<kSacIn, 1>(w, S);
    float g = 0.0f, sq = 0.0f;
    if (j < R) {
      const float diff = S.head[j] - yv;
      if (j < nrow) { g = (2.0f * diff) / (float)a.batch; sq = diff * diff; }
      G.gout[j] = g;
    }
    __syncthreads();
    sac_mlp_backward<kSacIn, 1>(w, S, G.gout);
    float* rec = sac_ws_rows(a.ws, a.batch, c, row0);
    sac_store_fields(rec, nrow, kWsH1, S.h1, kWsH2, S.h2);
    sac_store_fields(rec, nrow, kWsD1, S.part[1], kWsD2, S.part[0]);
    sac_store_x(rec, nrow, S, kWsXDim);
    if (j < nrow) {
      float* p = rec + (size_t)j * kWsRow + kWsG;
      p[0] = g; p[1] = 0.0f; p[2] = sq; p[3] = 0.0f;
    }
    __syncthreads();                          // the records are read before the next pass overwrites the LDS
  }
}

template <typename T>
struct SacPolicyFb {
  int batch;
  uint64_t seed, update;
  const float *actor, *critic, *alpha;
  const T *state, *noise;
  float* ws;
};

// (CLOCKED: sit_sac.h, SacClocked)
template <typename T, bool CLOCKED = false>
__global__ __launch_bounds__(256) void k_sac_policy_fb(const SacRowArgs<SacPolicyFb<T>, CLOCKED> a) {
#pragma clang fp reassociate(off) contract(off)
  constexpr int R = kSacRows;
  __shared__ SacGradLds G;
  SacLds& S = G.S;
  const int j = threadIdx.x;
  const int row0 = blockIdx.x * R;
  const int nrow = min(R, a.batch - row0);
  float* rec = sac_ws_rows(a.ws, a.batch, 0, row0);
  sac_stage_rows<T>(S, a.state, nullptr, row0, nrow);
  __syncthreads();
  sac_mlp<kActorObs, 2>(a.actor, S);
  // the actor's activations go to the records now: the critics run through the same LDS
  // (column 10 of S.in receives the action below: the actor's record holds zeros there)
  sac_store_fields(rec, nrow, kWsH1, S.h1, kWsH2, S.h2);
  sac_store_x(rec, nrow, S, kActorObs);
  // the squashed Gaussian head, thread j < R = row j (rows past nrow: on zeros)
  SacHead hd{};
  if (j < R) {
    uint64_t update;
    if constexpr (CLOCKED) update = a.tick->update; else update = a.update;
    hd = sac_gaussian_head(S, j, row0 + j, j < nrow, a.noise, a.seed, update, kSacPolicyTag);
    S.in[j][kActorObs] = hd.act;
  }
  __syncthreads();
  // both critics at (state, a), each taken back to the action input from an output gradient of -1/B
  float q[2] = {0.0f, 0.0f}, ga[2] = {0.0f, 0.0f};
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const float* w = a.critic + (size_t)c * SIT_CRITIC_WEIGHTS;
    sac_mlp<kSacIn, 1>(w, S);
    if (j < R) {
      q[c] = S.head[j];
      G.gout[j] = j < nrow ? -1.0f / (float)a.batch : 0.0f;
    }
    __syncthreads();
    sac_mlp_backward<kSacIn, 1>(w, S, G.gout);
    // g_a[r] = sum_j W1[j][10] d1[r][j]: 16 lanes per row, each 16 units, then a 16-lane reduction
    {
      const int pr_raw = j >> 4, cl = j & 15;
      const int r = pr_raw < R ? pr_raw : R - 1;
      float sum = 0.0f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int u = cl * 16 + i;
        sum = __builtin_fmaf(w[SacNet<kSacIn, 1>::W1 + u * kSacIn + kActorObs], S.part[1][r][u], sum);
      }
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 16);
      if (cl == 0 && pr_raw < R) G.ga[r] = sum;
    }
    __syncthreads();
    if (j < R) ga[c] = G.ga[j];
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
    G.gout[2 * j] = dmu;
    G.gout[2 * j + 1] = dls;
    if (j < nrow) {
      float* p = rec + (size_t)j * kWsRow + kWsG;
      p[0] = dmu; p[1] = dls; p[2] = alpha * hd.logp - qmin; p[3] = hd.logp;
    }
  }
  // the actor's activations back from the records (each thread reads what it wrote)
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float* p = rec + (size_t)r * kWsRow;
    S.h1[r][j] = r < nrow ? p[kWsH1 + j] : 0.0f;
    S.h2[r][j] = r < nrow ? p[kWsH2 + j] : 0.0f;
  }
  __syncthreads();
  sac_mlp_backward<kActorObs, 2>(a.actor, S, G.gout);
  sac_store_fields(rec, nrow, kWsD1, S.part[1], kWsD2, S.part[0]);
}

// (SacAdamScalars: sit_sac_clock.h)

__device__ __forceinline__ void sac_adam_apply(const SacAdamScalars& o, float g, float* p, float* m, float* v) {
#pragma clang fp reassociate(off) contract(off)
  const float m1 = *m + o.one_minus_beta1 * (g - *m);
  const float v1 = o.beta2 * *v + o.one_minus_beta2 * (g * g);
  *m = m1;
  *v = v1;
  *p = *p - o.step_size * (m1 / (sqrtf(v1) / o.sqrt_bias2 + o.eps));
}

struct SacAdam {
  int batch;
  float *p, *m, *v;            // nets x STRIDE floats each
  const float* ws;
  float* results;
  SacAdamScalars o;
  // the actor's launch only
  int tune;
  float target_entropy;
  float *alpha, *log_alpha, *log_alpha_m, *log_alpha_v;
  SacAdamScalars oa;
};

// What follows the loss sums of network pass c: `sum` of the rows' loss terms gives results[c], or in the
// actor's launch (TEMPERATURE) results[2], and there `ent` = sum of (logp + target_entropy) gives the
// temperature loss, log_alpha's Adam step and alpha = exp(log_alpha): results[3], results[4].  One thread.
template <bool TEMPERATURE>
__device__ __forceinline__ void sac_finish_losses(const SacAdam& a, int c, double sum, double ent) {
#pragma clang fp reassociate(off) contract(off)
  const double B = (double)a.batch;
  if (!TEMPERATURE) {
    a.results[c] = (float)(sum / B);
    return;
  }
  a.results[2] = (float)(sum / B);
  float la = 0.0f;
  if (a.tune) {
    const double mean = ent / B;
    la = (float)-((double)*a.log_alpha * mean);
    sac_adam_apply(a.oa, (float)-mean, a.log_alpha, a.log_alpha_m, a.log_alpha_v);
    *a.alpha = expf(*a.log_alpha);
  }
  a.results[3] = la;
  a.results[4] = *a.alpha;
}

// What an Adam kernel's CLOCKED instantiation (sit_sac_updates) takes besides SacAdam, whose o, oa and results
// it replaces from the tick of slot `slot`: the critics' launch the target block of the Polyak update, the
// actor's launch the hyper-parameters from which its finishing thread forms the next update's tick in the
// other slot.  The other instantiation is the kernel as it was before there was a clock.
struct SacAdamClock {
  int64_t* clock;
  int slot;
  float* target;
  float tau;
  SacClockHyper hy;
};
struct SacAdamClocked : SacAdam {
  SacAdamClock k;
};
template <bool CLOCKED>
using SacAdamArgs = std::conditional_t<CLOCKED, SacAdamClocked, SacAdam>;

// SacAdam as the finishing thread of a clocked launch sees it: the step's scalars and the results row from the tick
template <bool TEMPERATURE>
__device__ __forceinline__ SacAdam sac_adam_from_tick(const SacAdamClocked& a) {
  const SacTick* t = sac_clock_tick(a.k.clock, a.k.slot);
  SacAdam b = a;
  b.o = t->o[TEMPERATURE ? kClockPolicy : kClockCritic];
  if (TEMPERATURE) b.oa = t->o[kClockAlpha];
  b.results = a.results + 5 * t->results_row;
  return b;
}

// The Adam step of one element in a clocked launch, with the tick's scalars; the critics' launch then applies
// the Polyak update to the element when the tick says so: k_sac_polyak's arithmetic on the values k_sac_polyak
// would read, since nothing writes the online critics between the two.
template <bool TEMPERATURE>
__device__ __forceinline__ void sac_adam_apply_clocked(const SacAdamClocked& a, const SacTick* t, float g, size_t e) {
#pragma clang fp reassociate(off) contract(off)
  sac_adam_apply(t->o[TEMPERATURE ? kClockPolicy : kClockCritic], g, a.p + e, a.m + e, a.v + e);
  if (!TEMPERATURE && t->polyak) {
    float* target = a.k.target + e;
    *target = __builtin_fmaf(a.k.tau, a.p[e] - *target, *target);
  }
}

// NETS networks of SacNet<IN, NOUT>, STRIDE floats apart (the records of network c are pass c).
// TEMPERATURE: the actor's launch (results[2..4] and the temperature step) instead of the critics'
// (results[0..1]).  CLOCKED: scalars and results row from the clock's tick; the critics' launch also applies
// the Polyak update, and the actor's finishing thread advances the clock.
template <int IN, int NOUT, int NETS, int STRIDE, bool TEMPERATURE, bool CLOCKED = false>
__global__ __launch_bounds__(256) void k_sac_adam(const SacAdamArgs<CLOCKED> a) {
#pragma clang fp reassociate(off) contract(off)
  static_assert(!TEMPERATURE || NETS == 1, "the temperature step belongs to the actor's launch");
  constexpr unsigned kBlocks = (NETS * STRIDE + 255) / 256;
  const int B = a.batch;
  if (blockIdx.x == kBlocks) {                 // the extra block: the losses
    if (threadIdx.x != 0) return;
    // (one thread, so the sums over the rows are kept in float64: a float32 running sum of B terms loses
    // about sqrt(B) ulp, more than the pairwise sums of a library reduction)
    for (int c = 0; c < NETS; ++c) {
      const float* g = a.ws + (size_t)c * (size_t)B * kWsRow + kWsG;
      double sum = 0.0, ent = 0.0;
      for (int b = 0; b < B; ++b) {
        sum += (double)g[(size_t)b * kWsRow + 2];
        if (TEMPERATURE) ent += (double)g[(size_t)b * kWsRow + 3] + (double)a.target_entropy;
      }
      if constexpr (CLOCKED) sac_finish_losses<TEMPERATURE>(sac_adam_from_tick<TEMPERATURE>(a), c, sum, ent);
      else sac_finish_losses<TEMPERATURE>(a, c, sum, ent);
    }
    if constexpr (CLOCKED && TEMPERATURE) sac_clock_advance(a.k.clock, a.k.hy, a.k.slot ^ 1);
    return;
  }
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int c = e / STRIDE, off = e % STRIDE;
  if (c >= NETS || off >= SacNet<IN, NOUT>::kSize) return;    // past the block, or its padding
  // the element's gradient: the sum over the rows of its segment's two operands (sac_segment)
  int row_at = -1, col_at = -1;
#pragma unroll
  for (int s = 0; s < kSacSegments; ++s) {
    const SacSegment g = sac_segment<IN, NOUT>(s);
    if (off >= g.out && off < g.out + g.rows * g.cols) {
      if (g.row_n) row_at = g.row_at + (off - g.out) / g.cols;
      if (g.col_n) col_at = g.col_at + (off - g.out) % g.cols;
    }
  }
  const float* rec = a.ws + (size_t)c * (size_t)B * kWsRow;
  float g = 0.0f;
  if (row_at >= 0 && col_at >= 0) {
    // (the column operand first: in W2^T, most of a block, it is the load a wave coalesces)
    for (int b = 0; b < B; ++b) g = __builtin_fmaf(rec[(size_t)b * kWsRow + col_at], rec[(size_t)b * kWsRow + row_at], g);
  } else {                                     // a bias: the other operand is the constant 1
    const int at = row_at >= 0 ? row_at : col_at;
    for (int b = 0; b < B; ++b) g += rec[(size_t)b * kWsRow + at];
  }
  if constexpr (CLOCKED) sac_adam_apply_clocked<TEMPERATURE>(a, sac_clock_tick(a.k.clock, a.k.slot), g, (size_t)e);
  else sac_adam_apply(a.o, g, a.p + e, a.m + e, a.v + e);
}

inline SacAdamScalars sac_adam_scalars(const sit_sac_adam& o) {
  SacAdamScalars s;
  s.one_minus_beta1 = (float)(1.0 - o.beta1);
  s.beta2 = (float)o.beta2;
  s.one_minus_beta2 = (float)(1.0 - o.beta2);
  s.step_size = (float)(o.lr / o.bias1);
  s.sqrt_bias2 = (float)std::sqrt(o.bias2);
  s.eps = (float)o.eps;
  return s;
}

// The Adam kernel that follows a call's row kernel, with its grid: k_sac_adam here, or k_sac_wgrad_adam of
// sit_sac_wgrad.h in the _tiled calls (sac_adam_launch there picks one).
struct SacAdamLaunch {
  void (*kernel)(const SacAdam);
  unsigned blocks, threads;
};

inline int sac_launch_adam(sit_handle* h, const SacAdamLaunch& k, const SacAdam& a, hipStream_t stream) {
  hipLaunchKernelGGL(k.kernel, dim3(k.blocks), dim3(k.threads), 0, stream, a);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
}

// the same for the clocked forms (sit_sac_updates)
struct SacAdamClockLaunch {
  void (*kernel)(const SacAdamClocked);
  unsigned blocks, threads;
};

inline int sac_launch_adam_clocked(sit_handle* h, const SacAdamClockLaunch& k, const SacAdam& a, const SacAdamClock& c,
                                   hipStream_t stream) {
  SacAdamClocked ac{};
  static_cast<SacAdam&>(ac) = a;
  ac.k = c;
  hipLaunchKernelGGL(k.kernel, dim3(k.blocks), dim3(k.threads), 0, stream, ac);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
}

template <typename T>
int sac_launch_critic_step(sit_handle* h, const sit_sac_critic_step_args* s, const SacAdamLaunch& adam, hipStream_t stream) {
  SacCriticFb<T> f{};
  f.batch = s->batch;
  f.critic = s->critic_weights;
  f.state = (const T*)s->state;
  f.action = (const T*)s->action;
  f.y = (const T*)s->y;
  f.ws = s->workspace;
  hipLaunchKernelGGL(k_sac_critic_fb<T>, dim3((unsigned)((s->batch + kSacRows - 1) / kSacRows)), dim3(256), 0, stream, f);
  HIP_TRY(h, hipGetLastError());
  SacAdam a{};
  a.batch = s->batch;
  a.p = s->critic_weights; a.m = s->critic_m; a.v = s->critic_v;
  a.ws = s->workspace;
  a.results = s->results;
  a.o = sac_adam_scalars(s->adam);
  return sac_launch_adam(h, adam, a, stream);
}

template <typename T>
int sac_launch_policy_step(sit_handle* h, const sit_sac_policy_step_args* s, const SacAdamLaunch& adam, hipStream_t stream) {
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
  hipLaunchKernelGGL(k_sac_policy_fb<T>, dim3((unsigned)((s->batch + kSacRows - 1) / kSacRows)), dim3(256), 0, stream, f);
  HIP_TRY(h, hipGetLastError());
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
  return sac_launch_adam(h, adam, a, stream);
}

}  // namespace

#endif  // SIT_SAC_GRAD_H
