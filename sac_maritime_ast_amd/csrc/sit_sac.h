// sit_sac.h — the no-gradient half of a SAC update (include/sit.h: sit_sac_target, sit_sac_polyak).
//
// agent.update_parameters (test_beds/main_ast.py:350-362) has a gradient half (two critic losses, the
// policy loss, the temperature loss: autograd's) and a half that is inference only: the actor at
// next_state with its log-probability, both target critics at (next_state, a'), the TD target, and the
// Polyak update of the targets.  As library GEMMs and elementwise kernels the second half is ~25
// launches per update; here it is two.
//
// k_sac_target: one block of 256 threads per kSacRows minibatch rows; the three MLPs (actor 10 -> 256
// -> 256 -> 2, critics 11 -> 256 -> 256 -> 1) run one after another through the same LDS.  Layer 1:
// thread j = hidden unit j.  Layer 2 is split over K as in k_policy_actor: wave q sums inputs
// [64 q, 64 q + 64) for all 256 units, lane l owning units 4l..4l+3 (one coalesced float4 of W2^T per
// k, the activations wave-uniform LDS broadcasts); the four quarter sums meet in LDS as
// ((q0 + q1) + (q2 + q3)) + b2.  Layer 3: 16 lanes per (row, output) and a 16-lane shuffle reduction.
// Every sum has a fixed order and no row's arithmetic depends on another row or on the batch size, so
// the kernel is deterministic and rows [0, B) are the same bits for every B.  Rows past B in the last
// block are computed on zeros and neither read nor written.
//
// The gradient half (sit_sac_grad.h, sit_sac_wgrad.h) builds on this file: its row kernels share sac_mlp,
// sac_stage_rows and sac_gaussian_head, and the workspace record and the map from parameter segments to
// record fields (sac_segment) are stated here, next to SacNet.
//
// Included from sit_kernels.hip only (the strictly compiled translation unit).
#ifndef SIT_SAC_H
#define SIT_SAC_H

#include <type_traits>

#include "sit_host.h"
#include "sit_sac_args.h"
#include "sit_sac_clock.h"

namespace {

constexpr int kSacRows = 8;
constexpr int kSacIn = SIT_OBS_DIM + 1;   // a critic's input: (next_state, a')
constexpr uint32_t kSacTag = 0x5441u;     // counter word 1 of the target's noise draw
static_assert(SIT_CRITIC_WEIGHTS % 4 == 0, "the second critic's block is 16-byte aligned");

// packed block of a (IN -> 256 -> 256 -> NOUT) ReLU MLP: W1 [H][IN], b1 [H], W2^T [H in][H out], b2 [H],
// W3 [NOUT][H], b3 [NOUT] (the actor's layout of sit_serve.h with IN = 10, NOUT = 2)
template <int IN, int NOUT>
struct SacNet {
  static constexpr int H = kActorHidden;
  static constexpr int W1 = 0, B1 = W1 + H * IN, W2T = B1 + H, B2 = W2T + H * H, W3 = B2 + H, B3 = W3 + NOUT * H;
  static constexpr int kSize = B3 + NOUT;
};
static_assert(SacNet<kActorObs, 2>::kSize == SIT_ACTOR_WEIGHTS && SacNet<kActorObs, 2>::W2T == kActorW2T,
              "the actor block is sit_serve.h's");
static_assert(SacNet<kSacIn, 1>::kSize <= SIT_CRITIC_WEIGHTS && SIT_CRITIC_WEIGHTS - SacNet<kSacIn, 1>::kSize < 4,
              "critic block: the packed network padded to 4 floats");
static_assert(SacNet<kSacIn, 1>::W2T % 4 == 0, "float4 reads of the critic's W2^T");

// A row's record in the float32 workspace of the gradient calls (sit_sac_grad.h writes it): x [12] (the
// input row, zero padded), h1, h2 (the activations), d1, d2 (the deltas of the two hidden layers), then 4
// floats: the output gradients g[0], g[1] and two per-row loss terms.
constexpr int kWsX = 0, kWsXDim = 12;
constexpr int kWsH1 = kWsX + kWsXDim, kWsH2 = kWsH1 + kActorHidden, kWsD1 = kWsH2 + kActorHidden;
constexpr int kWsD2 = kWsD1 + kActorHidden, kWsG = kWsD2 + kActorHidden, kWsRow = kWsG + 4;
static_assert(kWsRow == SIT_SAC_WORKSPACE_ROW, "the workspace row of include/sit.h");
static_assert(kWsXDim == kSacIn + 1, "a record's input is SacLds::in's row");

// Segment s = 0..5 of SacNet<IN, NOUT> (W1, b1, W2^T, b2, W3, b3) as its gradient reads the records: `out`
// its offset in the block, rows x cols its row-major shape; element (r, c) is the sum over the batch of
// (float row_at + r of a record) x (float col_at + c), an operand of width 0 being the constant 1.  The one
// statement of which record fields make which parameter: k_sac_adam and k_sac_wgrad_adam both read it.
struct SacSegment {
  int out, rows, cols;
  int row_at, row_n;
  int col_at, col_n;
};
constexpr int kSacSegments = 6;

template <int IN, int NOUT>
constexpr SacSegment sac_segment(int s) {
  using N = SacNet<IN, NOUT>;
  constexpr int H = kActorHidden;
  static_assert(IN <= kWsXDim && NOUT <= 2, "the record's x and g fields");
  switch (s) {
    case 0: return {N::W1, H, IN, kWsD1, H, kWsX, IN};
    case 1: return {N::B1, 1, H, 0, 0, kWsD1, H};
    case 2: return {N::W2T, H, H, kWsH1, H, kWsD2, H};
    case 3: return {N::B2, 1, H, 0, 0, kWsD2, H};
    case 4: return {N::W3, NOUT, H, kWsG, NOUT, kWsH2, H};
    default: return {N::B3, NOUT, 1, kWsG, NOUT, 0, 0};
  }
}

struct SacLds {
  float in[kSacRows][kSacIn + 1];                       // the rows' inputs: next_state, then a'
  __attribute__((aligned(16))) float h1[kSacRows][kActorHidden];      // layer-1 activations
  __attribute__((aligned(16))) float part[4][kSacRows][kActorHidden]; // layer-2 sums of the 4 K quarters
  __attribute__((aligned(16))) float h2[kSacRows][kActorHidden];      // layer-2 activations
  float head[2 * kSacRows];                             // layer-3 outputs, [row][output]
};

// One MLP over the block's rows: reads S.in[r][0..IN), leaves its outputs in S.head[r * NOUT + o].
// Called by all 256 threads; S.in is complete (a barrier behind its last write), and S.head may be
// read by anyone once the call returns (it ends with a barrier).
template <int IN, int NOUT>
__device__ __forceinline__ void sac_mlp(const float* __restrict__ w, SacLds& S) {
#pragma clang fp reassociate(off) contract(off)
  using N = SacNet<IN, NOUT>;
  constexpr int H = kActorHidden, R = kSacRows;
  static_assert(R * NOUT * 16 <= H, "layer 3: 16 lanes per (row, output)");
  const int j = threadIdx.x, q = j >> 6, l = j & 63;
  // layer 1: h1 = relu(W1 x + b1), thread j = hidden unit j
  {
    float wr[IN];
#pragma unroll
    for (int i = 0; i < IN; ++i) wr[i] = w[N::W1 + j * IN + i];
    const float b1 = w[N::B1 + j];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float acc = 0.0f;
#pragma unroll
      for (int i = 0; i < IN; ++i) acc = __builtin_fmaf(wr[i], S.in[r][i], acc);
      S.h1[r][j] = __builtin_fmaxf(acc + b1, 0.0f);
    }
  }
  __syncthreads();
  // layer 2, split-K
  {
    const float4* w2 = reinterpret_cast<const float4*>(w + N::W2T) + l;
    const int kq = q * 64;
    float acc[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[r][n] = 0.0f;
#pragma unroll 2
    for (int g = 0; g < 16; ++g) {
      const int k = kq + 4 * g;
      float4 wk[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) wk[i] = w2[(size_t)(k + i) * (H / 4)];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float4 hv = *reinterpret_cast<const float4*>(&S.h1[r][k]);
        const float hk[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[r][0] = __builtin_fmaf(hk[i], wk[i].x, acc[r][0]);
          acc[r][1] = __builtin_fmaf(hk[i], wk[i].y, acc[r][1]);
          acc[r][2] = __builtin_fmaf(hk[i], wk[i].z, acc[r][2]);
          acc[r][3] = __builtin_fmaf(hk[i], wk[i].w, acc[r][3]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
      *reinterpret_cast<float4*>(&S.part[q][r][4 * l]) = float4{acc[r][0], acc[r][1], acc[r][2], acc[r][3]};
  }
  __syncthreads();
  {
    const float b2 = w[N::B2 + j];
#pragma unroll
    for (int r = 0; r < R; ++r)
      S.h2[r][j] = __builtin_fmaxf(((S.part[0][r][j] + S.part[1][r][j]) + (S.part[2][r][j] + S.part[3][r][j])) + b2, 0.0f);
  }
  __syncthreads();
  // layer 3: (row, output) pairs x 16 lanes, each lane 16 units, then a 16-lane reduction (pairs past
  // R * NOUT recompute the last one and write nothing)
  {
    const int pr_raw = j >> 4, c = j & 15;
    const int pr = pr_raw < R * NOUT ? pr_raw : R * NOUT - 1;
    const int r = pr / NOUT, o = pr % NOUT;
    const float* v = w + N::W3 + o * H + c * 16;
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) sum = __builtin_fmaf(S.h2[r][c * 16 + i], v[i], sum);
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 16);
    if (c == 0 && pr_raw < R * NOUT) S.head[pr] = sum + w[N::B3 + o];
  }
  __syncthreads();
}

// The block's rows [row0, row0 + nrow) of `state` into S.in, zeros past nrow; column kActorObs is the row's
// `extra` (the critic step's action; nullptr: zero), the padding column zero.  The caller's barrier follows.
template <typename T>
__device__ __forceinline__ void sac_stage_rows(SacLds& S, const T* state, const T* extra, int row0, int nrow) {
  const int j = threadIdx.x;
  const int r = j / kActorObs, i = j % kActorObs;
  if (j < kSacRows * kActorObs) S.in[r][i] = r < nrow ? (float)state[(size_t)(row0 + r) * kActorObs + i] : 0.0f;
  if (j < kSacRows) {
    S.in[j][kActorObs] = extra && j < nrow ? (float)extra[row0 + j] : 0.0f;
    S.in[j][kActorObs + 1] = 0.0f;
  }
}

// standard normal of (seed, row, update): Philox4x32-10(key = seed, ctr = (row, tag, update lo, update hi)),
// then sampler_normal's Box-Muller step (sit_device.h)
__device__ __forceinline__ double sac_normal(uint64_t seed, uint32_t row, uint64_t update, uint32_t tag) {
  uint32_t c[4] = {row, tag, (uint32_t)update, (uint32_t)(update >> 32)};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const double u1 = ((double)(c[0] >> 5) * 67108864.0 + (double)(c[1] >> 6) + 1.0) * (1.0 / 9007199254740992.0);
  const double u2 = ((double)(c[2] >> 5) * 67108864.0 + (double)(c[3] >> 6)) * (1.0 / 9007199254740992.0);
  return sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2);
}

// log(1 - tanh(x)^2 + 1e-6) without the cancellation of 1 - a * a: with em = expm1(2|x|) (formed as
// actor_tanh forms it), 1 - tanh(x)^2 = 4 (em + 1) / (em + 2)^2, every factor a positive number known to
// a few ulp.  |x| is capped at 40 (em < 6e34 stays finite; the term is below 1e-68 there, against 1e-6).
// sac_one_minus_sq is 1 - tanh(x)^2 itself; sac_gaussian_head takes the logarithm.
__device__ __forceinline__ float sac_one_minus_sq(float x) {
#pragma clang fp reassociate(off) contract(off)
  const float ax = __builtin_fminf(__builtin_fabsf(x), 40.0f);
  const float t = ax + ax;
  float em;
  if (t < 0.35f) {
    float p = 2.48015873e-5f;                           // 1/8!
    p = __builtin_fmaf(p, t, 1.98412698e-4f);
    p = __builtin_fmaf(p, t, 1.38888889e-3f);
    p = __builtin_fmaf(p, t, 8.33333333e-3f);
    p = __builtin_fmaf(p, t, 4.16666667e-2f);
    p = __builtin_fmaf(p, t, 1.66666667e-1f);
    p = __builtin_fmaf(p, t, 0.5f);
    p = __builtin_fmaf(p, t, 1.0f);
    em = p * t;
  } else {
    em = actor_exp(t) - 1.0f;
  }
  const float rc = 1.0f / (em + 2.0f);
  return (4.0f * ((em + 1.0f) * rc)) * rc;              // (em + 1) / (em + 2) <= 1: no overflow
}

// The squashed Gaussian head of row `row` = row0 + j from the actor's outputs S.head[2 j], S.head[2 j + 1]:
// x = mu + exp(clip(ls_raw)) eps, the action tanh(x), s = 1 - tanh(x)^2 and the log-probability.  eps is the
// caller's noise[row], or without one the draw of (seed, row, update, tag); a row that is not `live` (past
// the batch) takes eps = 0.
struct SacHead {
  float mu, ls_raw, ls, eps, sig, x, act, s, logp;
};

template <typename T>
__device__ __forceinline__ SacHead sac_gaussian_head(const SacLds& S, int j, int row, bool live, const T* noise,
                                                     uint64_t seed, uint64_t update, uint32_t tag) {
#pragma clang fp reassociate(off) contract(off)
  SacHead h;
  h.mu = S.head[2 * j];
  h.ls_raw = S.head[2 * j + 1];
  h.ls = __builtin_fminf(__builtin_fmaxf(h.ls_raw, -20.0f), 2.0f);
  h.eps = 0.0f;
  if (live) h.eps = noise ? (float)noise[row] : (float)sac_normal(seed, (uint32_t)row, update, tag);
  h.sig = actor_exp(h.ls);
  h.x = __builtin_fmaf(h.sig, h.eps, h.mu);
  h.act = actor_tanh(h.x);
  h.s = sac_one_minus_sq(h.x);
  h.logp = ((-0.5f * (h.eps * h.eps) - h.ls) - 0.918938533f) - logf(h.s + 1e-6f);   // 0.5 log(2 pi)
  return h;
}

template <typename T>
struct SacTarget {
  int batch;
  uint64_t seed, update;
  T gamma, reward_scale;
  const float *actor, *critic, *alpha;
  const T *next_state, *reward, *mask, *noise;
  T *y, *next_action, *next_logp, *q1, *q2;
};

// The arguments of a clocked row kernel (sit_sac_updates): those of the kernel, whose `update` is not read, and
// the clock's tick that holds the update number instead.  A row kernel's CLOCKED instantiation takes them; its
// other instantiation is the kernel as it was before there was a clock, instruction for instruction.
template <typename A>
struct SacClocked : A {
  const SacTick* tick;
};
template <typename A, bool CLOCKED>
using SacRowArgs = std::conditional_t<CLOCKED, SacClocked<A>, A>;

template <typename T, bool CLOCKED = false>
__global__ __launch_bounds__(256) void k_sac_target(const SacRowArgs<SacTarget<T>, CLOCKED> a) {
#pragma clang fp reassociate(off) contract(off)
  constexpr int R = kSacRows;
  __shared__ SacLds S;
  const int j = threadIdx.x;
  const int row0 = blockIdx.x * R;
  const int nrow = min(R, a.batch - row0);    // >= 1: the grid is ceil(batch / R) blocks
  sac_stage_rows<T>(S, a.next_state, nullptr, row0, nrow);
  __syncthreads();
  sac_mlp<kActorObs, 2>(a.actor, S);
  // the squashed Gaussian head and its log-probability, thread j < R = row j (rows past nrow: on zeros)
  float logp = 0.0f, act = 0.0f;
  if (j < R) {
    uint64_t update;
    if constexpr (CLOCKED) update = a.tick->update; else update = a.update;
    const SacHead hd = sac_gaussian_head(S, j, row0 + j, j < nrow, a.noise, a.seed, update, kSacTag);
    act = hd.act;
    logp = hd.logp;
    S.in[j][kActorObs] = act;
  }
  __syncthreads();
  sac_mlp<kSacIn, 1>(a.critic, S);
  const float q1 = j < R ? S.head[j] : 0.0f;
  sac_mlp<kSacIn, 1>(a.critic + SIT_CRITIC_WEIGHTS, S);
  if (j < nrow) {
    const float q2 = S.head[j];
    const int row = row0 + j;
    const T soft = (T)__builtin_fminf(q1, q2) - (T)(*a.alpha) * (T)logp;
    a.y[row] = a.reward_scale * a.reward[row] + a.mask[row] * a.gamma * soft;
    if (a.next_action) a.next_action[row] = (T)act;
    if (a.next_logp) a.next_logp[row] = (T)logp;
    if (a.q1) a.q1[row] = (T)q1;
    if (a.q2) a.q2[row] = (T)q2;
  }
}

// t = fma(tau, p - t, t) over a packed float32 block: float4 body, scalar tail
__global__ __launch_bounds__(256) void k_sac_polyak(float* __restrict__ target, const float* __restrict__ online,
                                                    long long n, float tau) {
#pragma clang fp reassociate(off) contract(off)
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n4 = n >> 2;
  if (t < n4) {
    float4 tv = reinterpret_cast<float4*>(target)[t];
    const float4 pv = reinterpret_cast<const float4*>(online)[t];
    tv.x = __builtin_fmaf(tau, pv.x - tv.x, tv.x);
    tv.y = __builtin_fmaf(tau, pv.y - tv.y, tv.y);
    tv.z = __builtin_fmaf(tau, pv.z - tv.z, tv.z);
    tv.w = __builtin_fmaf(tau, pv.w - tv.w, tv.w);
    reinterpret_cast<float4*>(target)[t] = tv;
  } else {
    const long long i = 4 * n4 + (t - n4);
    if (i < n) target[i] = __builtin_fmaf(tau, online[i] - target[i], target[i]);
  }
}

template <typename T>
int sac_launch_target(sit_handle* h, const sit_sac_target_args* s, hipStream_t stream) {
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
  hipLaunchKernelGGL(k_sac_target<T>, dim3((unsigned)((s->batch + kSacRows - 1) / kSacRows)), dim3(256), 0, stream, a);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
}

int sac_launch_polyak(sit_handle* h, float* target, const float* online, int64_t n, float tau, hipStream_t stream) {
  const long long lanes = (n >> 2) + (n & 3);
  hipLaunchKernelGGL(k_sac_polyak, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, target, online,
                     (long long)n, tau);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
}

}  // namespace

#endif  // SIT_SAC_H
