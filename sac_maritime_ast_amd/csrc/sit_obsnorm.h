// sit_obsnorm.h — observation normalisation on the device (include/sit.h: sit_obsnorm_*).
//
// Running mean and M2 of the ten observation columns of the records entering a replay ring, the affine
// (shift, scale) derived from them, its application to sampled rows and its folding into an actor block's
// first layer.  The statistics follow the pattern of sit_score.h, sized by max_new (the host never knows m):
//   k_obsnorm_chunks<R, false>  one 256-lane block per chunk of 256 new records: the chunk's ten column sums
//                               through the halving tree; a block whose first record is >= m exits after
//                               reading the cursor
//   k_obsnorm_groups<false>     one block: the chunk sums in groups of 256 through the same tree, the groups
//                               added in ascending order, mean_b = S / m
//   k_obsnorm_chunks<R, true>   the chunk sums of (x - mean_b)^2
//   k_obsnorm_groups<true>      one block: Q the same way, the merge into the block, the affine, the book-keeping
// and k_obsnorm_apply (in place over rows), k_obsnorm_fold (the serving block) and obsnorm_apply (what the
// normalised gather of sit_replay.h calls per element).
//
// Included from sit_kernels.hip only (the strictly compiled translation unit): every sum is a fixed tree of
// IEEE float64 adds, and every function that rounds turns contraction off for itself.
#ifndef SIT_OBSNORM_H
#define SIT_OBSNORM_H

#include "sit_host.h"
#include "sit_obsnorm_args.h"

namespace {

constexpr int kOnBlock = 256;       // lanes per block = records per chunk = chunk sums per group
constexpr int kOnCols = SIT_OBS_DIM;
constexpr int kOnStride = 16;       // doubles per chunk in the scratch, and per array of the blocks
constexpr int kOnMean = 8, kOnM2 = 24;                      // words of the block
constexpr int kOnShift = 0, kOnScale = 16, kOnMinStd = 32;  // words of the affine
static_assert(kOnMean + kOnCols <= kOnM2 && kOnM2 + kOnCols <= SIT_OBSNORM_DIM, "obsnorm block layout");
static_assert(kOnMinStd + kOnCols <= SIT_OBSNORM_AFFINE && SIT_TRANSITION_DIM % 2 == 0 && kOnCols % 2 == 0,
              "obsnorm affine layout; rows are read as pairs of reals");

template <typename R>
struct OnPair { using type = float2; };
template <>
struct OnPair<double> { using type = double2; };

struct OnMinStd { float v[kOnCols]; };

template <typename R>
struct OnArgs {
  const R* ring;
  const long long* cursor;
  double* block;
  float* affine;
  double *meanb, *sum, *q;     // the handle's scratch: mean_b[16], then [chunks][16] twice
  int capacity, max_new;
};

// x^ = (x - shift) * scale: two roundings in R
template <typename R>
__device__ __forceinline__ R obsnorm_apply(R x, R shift, R scale) {
#pragma clang fp reassociate(off) contract(off)
  const R d = x - shift;
  return d * scale;
}

// the new records: logical indices [*start, *start + m)
template <typename R>
__device__ inline long long on_range(const OnArgs<R>& a, long long* start, long long* seen) {
  const long long pushed = a.cursor[0];
  *seen = (long long)a.block[2];
  long long s = pushed - a.capacity;
  if (*seen > s) s = *seen;
  if (s < 0) s = 0;   // (a block that was never reset: no row below 0 is read)
  long long m = pushed - s;
  if (m > a.max_new) m = a.max_new;
  *start = s;
  return m < 0 ? 0 : m;
}

// The halving tree of sit_score.h's sc_tree, x[i] += x[i + s] for s = 128, 64, ..., 1, over ten columns at
// once; lane 0 returns the sums.  Every lane of the block calls it.
__device__ inline void on_tree(double (&x)[kOnCols]) {
#pragma clang fp reassociate(off) contract(off)
  __shared__ double sh[kOnCols][kOnBlock];
  const int t = threadIdx.x;
  __syncthreads();   // the previous call's readers are done with sh
#pragma unroll
  for (int c = 0; c < kOnCols; ++c) sh[c][t] = x[c];
  __syncthreads();
  if (t < 128) {
#pragma unroll
    for (int c = 0; c < kOnCols; ++c) {
      x[c] = x[c] + sh[c][t + 128];
      sh[c][t] = x[c];
    }
  }
  __syncthreads();
  if (t < 64) {
#pragma unroll
    for (int c = 0; c < kOnCols; ++c) x[c] = x[c] + sh[c][t + 64];
  }
  for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
    for (int c = 0; c < kOnCols; ++c) {
      const double y = __shfl_down(x[c], s);
      if (t < s) x[c] = x[c] + y;
    }
  }
}

__global__ __launch_bounds__(64) void k_obsnorm_reset(double* block, float* affine, OnMinStd ms) {
  const int t = threadIdx.x;
  block[t] = 0.0;
  if (t >= SIT_OBSNORM_AFFINE) return;
  float v = 0.0f;
  if (t >= kOnScale && t < kOnScale + kOnCols) v = 1.0f;
#pragma unroll
  for (int c = 0; c < kOnCols; ++c)
    if (t == kOnMinStd + c) v = ms.v[c];
  affine[t] = v;
}

template <typename R, bool kDev>
__global__ __launch_bounds__(kOnBlock) void k_obsnorm_chunks(OnArgs<R> a) {
#pragma clang fp reassociate(off) contract(off)
  long long start, seen;
  const long long m = on_range(a, &start, &seen);
  const long long j0 = (long long)blockIdx.x * kOnBlock;
  if (j0 >= m) return;
  const long long j = j0 + threadIdx.x;
  double x[kOnCols];
#pragma unroll
  for (int c = 0; c < kOnCols; ++c) x[c] = 0.0;
  if (j < m) {
    const long long row = (start + j) % a.capacity;
    using V = typename OnPair<R>::type;
    const V* p = reinterpret_cast<const V*>(a.ring + (size_t)row * SIT_TRANSITION_DIM);
#pragma unroll
    for (int q = 0; q < kOnCols / 2; ++q) {
      const V v = p[q];
      x[2 * q] = (double)v.x;
      x[2 * q + 1] = (double)v.y;
    }
    if (kDev) {
#pragma unroll
      for (int c = 0; c < kOnCols; ++c) {
        const double d = x[c] - a.meanb[c];
        x[c] = d * d;
      }
    }
  }
  on_tree(x);
  if (threadIdx.x == 0) {
    double* out = (kDev ? a.q : a.sum) + (size_t)blockIdx.x * kOnStride;
#pragma unroll
    for (int c = 0; c < kOnCols; ++c) out[c] = x[c];
  }
}

template <typename R, bool kFinish>
__global__ __launch_bounds__(kOnBlock) void k_obsnorm_groups(OnArgs<R> a) {
#pragma clang fp reassociate(off) contract(off)
  const int t = threadIdx.x;
  long long start, seen;
  const long long m = on_range(a, &start, &seen);
  if (m == 0) {
    if (kFinish && t == 0) a.block[1] += 1.0;
    return;
  }
  const long long chunks = (m + kOnBlock - 1) / kOnBlock;
  const double* part = kFinish ? a.q : a.sum;
  double total[kOnCols], x[kOnCols];
#pragma unroll
  for (int c = 0; c < kOnCols; ++c) total[c] = 0.0;
  for (long long g0 = 0; g0 < chunks; g0 += kOnBlock) {
    const long long k = g0 + t;
#pragma unroll
    for (int c = 0; c < kOnCols; ++c) x[c] = k < chunks ? part[(size_t)k * kOnStride + c] : 0.0;
    on_tree(x);
#pragma unroll
    for (int c = 0; c < kOnCols; ++c) total[c] = total[c] + x[c];   // (lane 0's is the one used)
  }
  if (t != 0) return;
  const double md = (double)m;
  if (!kFinish) {
#pragma unroll
    for (int c = 0; c < kOnCols; ++c) a.meanb[c] = ieee_div(total[c], md);
    return;
  }
  const double n = a.block[0], n2 = n + md;
  const double r = ieee_div(md, n2), w = ieee_div(n * md, n2);
#pragma unroll
  for (int c = 0; c < kOnCols; ++c) {
    const double mean = a.block[kOnMean + c];
    const double d = a.meanb[c] - mean;
    const double mean2 = mean + d * r;
    const double m2 = (a.block[kOnM2 + c] + total[c]) + (d * d) * w;
    a.block[kOnMean + c] = mean2;
    a.block[kOnM2 + c] = m2;
    const double s = ieee_sqrt(ieee_div(m2, n2)), least = (double)a.affine[kOnMinStd + c];
    const double sd = s > least ? s : least;
    a.affine[kOnScale + c] = (float)ieee_div(1.0, sd);
    a.affine[kOnShift + c] = (float)mean2;
  }
  a.block[3] += (double)(start - seen);
  a.block[2] = (double)(start + m);
  a.block[0] = n2;
  a.block[1] += 1.0;
}

// lane p: the p-th pair of reals of rows [n][10]; a pair never straddles a row (10 is even)
template <typename R>
__global__ __launch_bounds__(kOnBlock) void k_obsnorm_apply(const float* __restrict__ affine, R* rows_a, R* rows_b,
                                                            long long pairs) {
  const long long p = (long long)blockIdx.x * kOnBlock + threadIdx.x;
  if (p >= pairs) return;
  const int c = 2 * (int)(p % (kOnCols / 2));
  const R sh0 = (R)affine[kOnShift + c], sh1 = (R)affine[kOnShift + c + 1];
  const R sc0 = (R)affine[kOnScale + c], sc1 = (R)affine[kOnScale + c + 1];
  using V = typename OnPair<R>::type;
  V* pa = reinterpret_cast<V*>(rows_a) + p;
  V v = *pa;
  v.x = obsnorm_apply<R>(v.x, sh0, sc0);
  v.y = obsnorm_apply<R>(v.y, sh1, sc1);
  *pa = v;
  if (rows_b) {
    V* pb = reinterpret_cast<V*>(rows_b) + p;
    v = *pb;
    v.x = obsnorm_apply<R>(v.x, sh0, sc0);
    v.y = obsnorm_apply<R>(v.y, sh1, sc1);
    *pb = v;
  }
}

constexpr int kOnFoldHead = kActorW2T;   // W1 and b1: block 0, thread j = hidden unit j
constexpr int kOnFoldBlocks = 1 + ((SIT_ACTOR_WEIGHTS - kOnFoldHead + 3) / 4 + kOnBlock - 1) / kOnBlock;
static_assert(kActorHidden == kOnBlock && kActorW1 == 0 && kActorB1 == kActorHidden * kActorObs &&
              kOnFoldHead == kActorB1 + kActorHidden && kOnFoldHead % 4 == 0, "obsnorm fold: the actor block's head");

// block 0: the first layer; blocks 1..: the copy of the other segments, one float4 per lane, the last lane
// its 1..3 tail floats.  Every float of dst is written once.
__global__ __launch_bounds__(kOnBlock) void k_obsnorm_fold(const float* __restrict__ affine, const float* __restrict__ src,
                                                           float* __restrict__ dst) {
#pragma clang fp reassociate(off) contract(off)
  if (blockIdx.x == 0) {
    const int j = threadIdx.x;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < kActorObs; ++i) {
      const float w = src[kActorW1 + j * kActorObs + i] * affine[kOnScale + i];
      dst[kActorW1 + j * kActorObs + i] = w;
      acc = acc + (double)w * (double)affine[kOnShift + i];
    }
    dst[kActorB1 + j] = (float)((double)src[kActorB1 + j] - acc);
    return;
  }
  const int o = kOnFoldHead + 4 * ((int)(blockIdx.x - 1) * kOnBlock + (int)threadIdx.x);
  if (o + 4 <= SIT_ACTOR_WEIGHTS) {
    *reinterpret_cast<float4*>(dst + o) = *reinterpret_cast<const float4*>(src + o);
  } else {
    for (int i = o; i < SIT_ACTOR_WEIGHTS; ++i) dst[i] = src[i];
  }
}

// scratch for updates of up to `max_new` records; never shrinks (allocates when it grows: not capturable)
int obsnorm_reserve(sit_handle* h, size_t max_new) {
  if (h->obsnorm && max_new <= h->obsnorm_records) return SIT_OK;
  const size_t chunks = (max_new + kOnBlock - 1) / kOnBlock;
  const size_t bytes = (kOnStride + 2 * chunks * kOnStride) * sizeof(double);
  unsigned char* p = nullptr;
  if (setup_alloc(&p, bytes) != hipSuccess) return fail(h, SIT_E_NOMEM, "obsnorm: hipMalloc of %zu bytes failed", bytes);
  if (h->obsnorm) (void)setup_free(h->obsnorm);
  h->obsnorm = p;
  h->obsnorm_records = max_new;
  return SIT_OK;
}

int obsnorm_launch_reset(sit_handle* h, double* block, float* affine, const float* min_std, hipStream_t s) {
#ifdef SIT_HOST_MEMORY_TEST
  (void)block; (void)affine; (void)min_std; (void)s;
  return fail(h, SIT_E_STATE, "obsnorm: no device in the host-memory test build");
#else
  OnMinStd ms{};
  for (int c = 0; c < kOnCols; ++c) ms.v[c] = min_std ? min_std[c] : 0.0f;
  hipLaunchKernelGGL(k_obsnorm_reset, dim3(1), dim3(SIT_OBSNORM_DIM), 0, s, block, affine, ms);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
#endif
}

template <typename R>
int obsnorm_launch_update(sit_handle* h, const sit_obsnorm_args* ua, hipStream_t s) {
#ifdef SIT_HOST_MEMORY_TEST
  (void)ua; (void)s;
  return fail(h, SIT_E_STATE, "obsnorm: no device in the host-memory test build");
#else
  const size_t have = (h->obsnorm_records + kOnBlock - 1) / kOnBlock;   // chunks the scratch holds
  OnArgs<R> a{};
  a.ring = (const R*)ua->ring;
  a.cursor = reinterpret_cast<const long long*>(ua->cursor);
  a.block = ua->block;
  a.affine = ua->affine;
  a.meanb = reinterpret_cast<double*>(h->obsnorm);
  a.sum = a.meanb + kOnStride;
  a.q = a.sum + have * kOnStride;
  a.capacity = ua->capacity;
  a.max_new = ua->max_new;
  const unsigned chunks = (unsigned)(((size_t)ua->max_new + kOnBlock - 1) / kOnBlock);   // <= have: checked by the caller
  hipLaunchKernelGGL((k_obsnorm_chunks<R, false>), dim3(chunks), dim3(kOnBlock), 0, s, a);
  hipLaunchKernelGGL((k_obsnorm_groups<R, false>), dim3(1), dim3(kOnBlock), 0, s, a);
  hipLaunchKernelGGL((k_obsnorm_chunks<R, true>), dim3(chunks), dim3(kOnBlock), 0, s, a);
  hipLaunchKernelGGL((k_obsnorm_groups<R, true>), dim3(1), dim3(kOnBlock), 0, s, a);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
#endif
}

template <typename R>
int obsnorm_launch_apply(sit_handle* h, const float* affine, void* rows_a, void* rows_b, int64_t n_rows, hipStream_t s) {
#ifdef SIT_HOST_MEMORY_TEST
  (void)affine; (void)rows_a; (void)rows_b; (void)n_rows; (void)s;
  return fail(h, SIT_E_STATE, "obsnorm: no device in the host-memory test build");
#else
  const long long pairs = (long long)n_rows * (kOnCols / 2);
  hipLaunchKernelGGL(k_obsnorm_apply<R>, dim3((unsigned)((pairs + kOnBlock - 1) / kOnBlock)), dim3(kOnBlock), 0, s, affine,
                     (R*)rows_a, (R*)rows_b, pairs);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
#endif
}

int obsnorm_launch_fold(sit_handle* h, const float* affine, const float* src, float* dst, hipStream_t s) {
#ifdef SIT_HOST_MEMORY_TEST
  (void)affine; (void)src; (void)dst; (void)s;
  return fail(h, SIT_E_STATE, "obsnorm: no device in the host-memory test build");
#else
  hipLaunchKernelGGL(k_obsnorm_fold, dim3(kOnFoldBlocks), dim3(kOnBlock), 0, s, affine, src, dst);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
#endif
}

}  // namespace

#endif  // SIT_OBSNORM_H
