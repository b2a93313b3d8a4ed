// sit_score.h — device-side scores over the episode records (include/sit.h: sit_score_*).
//
// What the reference's driver loop keeps over episodes (test_beds/main_ast.py:432-444 best_reward and the
// checkpoint behind it, 453-523 avg_reward and status_record of a scoring round), reduced from the records
// of sit_episodes.h into the caller's 64-double score block.
//
// Two launches per update on the caller's stream, sized by record_capacity (the host never knows m):
//   k_score_chunks  one 256-lane block per chunk of 256 record slots: the chunk's return sum through the
//                   halving tree, (return, slot) argmax, min, max and the integer partials; a block whose
//                   first slot is >= m exits after reading the count
//   k_score_finish  one block: the chunk sums in groups of 256 through the same tree, the carry over the
//                   groups, the other partials, the comparison with the block's best, the record copy and
//                   the consume step
// and k_score_keep, the copy of up to four float32 blocks that happens iff the last update set score[7].
//
// Included from sit_kernels.hip only (the strictly compiled translation unit): the sum is a fixed tree of
// IEEE float64 adds, which fast-math could reassociate.
#ifndef SIT_SCORE_H
#define SIT_SCORE_H

#include "sit_episodes.h"
#include "sit_score_args.h"

namespace {

constexpr int kScBlock = 256;   // lanes per block = record slots per chunk = chunk sums per group

// the order-free partials of a set of records (a lane's, a chunk's, a round's)
struct ScAcc {
  double mn, mx, best;                 // over the included non-NaN returns (+inf, -inf, unused without one)
  long long slot;                      // slot of `best`, -1 without one
  long long n, steps;                  // included records, their steps
  long long cls[SIT_SCORE_CLASSES];
};

// one chunk's partials in the handle's scratch
struct ScPart {
  double sum;                          // the chunk's tree sum
  ScAcc acc;
  long long pad;
};
static_assert(sizeof(ScPart) == 128, "ScPart: 128 bytes per chunk");

struct ScArgs {
  const double* records;
  long long* record_count;
  double* score;
  ScPart* part;
  long long limit;
  int capacity;
  uint32_t flags;
  uint32_t any[SIT_SCORE_CLASSES], none[SIT_SCORE_CLASSES];
};

struct ScKeep {
  const float* src[SIT_SCORE_KEEP_BLOCKS];
  float* dst[SIT_SCORE_KEEP_BLOCKS];
  long long floats[SIT_SCORE_KEEP_BLOCKS];
  double* score;
  const long long* stamp;
  int n_blocks;
};

__device__ inline ScAcc sc_empty() {
  ScAcc a;
  a.mn = __longlong_as_double(0x7ff0000000000000LL);
  a.mx = __longlong_as_double((long long)0xfff0000000000000ULL);
  a.best = 0.0;
  a.slot = -1;
  a.n = a.steps = 0;
  for (int c = 0; c < SIT_SCORE_CLASSES; ++c) a.cls[c] = 0;
  return a;
}

// a <- a joined with b; every field is independent of the order of the joins
__device__ inline void sc_join(ScAcc& a, const ScAcc& b) {
  a.mn = b.mn < a.mn ? b.mn : a.mn;
  a.mx = b.mx > a.mx ? b.mx : a.mx;
  if (b.slot >= 0 && (a.slot < 0 || b.best > a.best || (b.best == a.best && b.slot < a.slot))) {
    a.best = b.best;
    a.slot = b.slot;
  }
  a.n += b.n;
  a.steps += b.steps;
  for (int c = 0; c < SIT_SCORE_CLASSES; ++c) a.cls[c] += b.cls[c];
}

// the value of word t of a reset block
__device__ inline double sc_reset_value(int t) {
  if (t == 3) return __longlong_as_double(0x7ff0000000000000LL);
  if (t == 4) return __longlong_as_double((long long)0xfff0000000000000ULL);
  if (t == 16 || t >= 32) return ep_nan();
  return 0.0;
}

// The halving tree x[i] += x[i + s], s = 128, 64, ..., 1, over the block's 256 lanes (LDS across the waves,
// shuffles inside wave 0); lane 0 returns x[0].  Every lane of the block calls it.
__device__ inline double sc_tree(double x) {
  __shared__ double sh[kScBlock];
  const int t = threadIdx.x;
  __syncthreads();   // the previous call's readers are done with sh
  sh[t] = x;
  __syncthreads();
  if (t < 128) {
    x = x + sh[t + 128];
    sh[t] = x;
  }
  __syncthreads();
  if (t < 64) x = x + sh[t + 64];
  for (int s = 32; s >= 1; s >>= 1) {
    const double y = __shfl_down(x, s);
    if (t < s) x = x + y;
  }
  return x;
}

// the join of the block's 256 partials, in thread 0.  Every lane of the block calls it.
__device__ inline void sc_block_join(ScAcc& a) {
  __shared__ ScAcc wacc[kScBlock / kWave];
  for (int s = kWave / 2; s >= 1; s >>= 1) {
    ScAcc b;
    b.mn = __shfl_xor(a.mn, s);
    b.mx = __shfl_xor(a.mx, s);
    b.best = __shfl_xor(a.best, s);
    b.slot = __shfl_xor(a.slot, s);
    b.n = __shfl_xor(a.n, s);
    b.steps = __shfl_xor(a.steps, s);
    for (int c = 0; c < SIT_SCORE_CLASSES; ++c) b.cls[c] = __shfl_xor(a.cls[c], s);
    sc_join(a, b);
  }
  __syncthreads();   // the previous call's reader is done with wacc
  if ((threadIdx.x & (kWave - 1)) == 0) wacc[threadIdx.x / kWave] = a;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kScBlock / kWave; ++w) sc_join(a, wacc[w]);
}

// count = max(*record_count, 0) and m = min(count, capacity)
__device__ inline long long sc_valid(const ScArgs& a, long long* count) {
  const long long c = *a.record_count;
  *count = c < 0 ? 0 : c;
  return *count < a.capacity ? *count : (long long)a.capacity;
}

__global__ __launch_bounds__(64) void k_score_reset(double* score) { score[threadIdx.x] = sc_reset_value(threadIdx.x); }

__global__ __launch_bounds__(kScBlock) void k_score_chunks(ScArgs a) {
  long long count;
  const long long m = sc_valid(a, &count);
  const long long j0 = (long long)blockIdx.x * kScBlock;
  if (j0 >= m) return;
  const long long j = j0 + threadIdx.x;
  ScAcc acc = sc_empty();
  double x = 0.0;
  if (j < m) {
    const double* rec = a.records + (size_t)j * SIT_EPISODE_DIM;
    const double episode = rec[1], steps = rec[2], ret = rec[3], status = rec[4];
    if (a.limit == 0 || episode < (double)a.limit) {
      const uint32_t bits = (uint32_t)(long long)status;
      x = ret;
      acc.n = 1;
      acc.steps = (long long)steps;
      for (int c = 0; c < SIT_SCORE_CLASSES; ++c) {
        const bool used = (a.any[c] | a.none[c]) != 0;
        acc.cls[c] = used && (a.any[c] == 0 || (bits & a.any[c])) && !(bits & a.none[c]) ? 1 : 0;
      }
      if (ret == ret) {
        acc.mn = acc.mx = acc.best = ret;
        acc.slot = j;
      }
    }
  }
  const double sum = sc_tree(x);
  sc_block_join(acc);
  if (threadIdx.x == 0) {
    ScPart p;
    p.sum = sum;
    p.acc = acc;
    p.pad = 0;
    a.part[blockIdx.x] = p;
  }
}

__global__ __launch_bounds__(kScBlock) void k_score_finish(ScArgs a) {
  __shared__ double sc[SIT_SCORE_DIM];
  __shared__ long long take;
  const int t = threadIdx.x;
  long long count;
  const long long m = sc_valid(a, &count);
  const long long chunks = (m + kScBlock - 1) / kScBlock;
  if (t < SIT_SCORE_DIM) sc[t] = (a.flags & SIT_SCORE_FRESH) ? sc_reset_value(t) : a.score[t];
  ScAcc acc = sc_empty();
  double round = 0.0;
  for (long long g0 = 0; g0 < chunks; g0 += kScBlock) {
    const long long c = g0 + t;
    double x = 0.0;
    if (c < chunks) {
      x = a.part[c].sum;
      sc_join(acc, a.part[c].acc);
    }
    const double group = sc_tree(x);
    if (t == 0) round = round + group;
  }
  sc_block_join(acc);
  if (t == 0) {
    sc[0] += (double)acc.n;
    sc[1] = sc[1] + round;
    sc[2] += (double)acc.steps;
    sc[3] = (acc.mn < sc[3] ? acc.mn : sc[3]) + 0.0;
    sc[4] = (acc.mx > sc[4] ? acc.mx : sc[4]) + 0.0;
    sc[6] += 1.0;
    for (int c = 0; c < SIT_SCORE_CLASSES; ++c) sc[8 + c] += (double)acc.cls[c];
    const double have = sc[SIT_SCORE_DIM / 2 + 3];
    const bool replace = acc.slot >= 0 && (have != have || acc.best > have);
    sc[7] = replace ? 1.0 : 0.0;
    take = replace ? acc.slot : -1;
    if (a.flags & SIT_SCORE_CONSUME) {
      sc[5] += (double)(count - m);
      *a.record_count = 0;
    }
  }
  __syncthreads();
  if (t < SIT_SCORE_DIM) {
    double v = sc[t];
    if (t >= SIT_SCORE_DIM / 2 && take >= 0) v = a.records[(size_t)take * SIT_EPISODE_DIM + (t - SIT_SCORE_DIM / 2)];
    a.score[t] = v;
  }
}

// blockIdx.y: the float32 block; a lane copies one float4, the last lane of a block its 1..3 tail floats
__global__ __launch_bounds__(kScBlock) void k_score_keep(ScKeep k) {
  if (k.score[7] == 0.0) return;
  const int b = blockIdx.y;
  if (b == 0 && blockIdx.x == 0 && threadIdx.x == 0 && k.stamp) k.score[16] = (double)*k.stamp;
  if (b >= k.n_blocks) return;
  const float* src = nullptr;
  float* dst = nullptr;
  long long n = 0;
#pragma unroll
  for (int i = 0; i < SIT_SCORE_KEEP_BLOCKS; ++i)
    if (i == b) {
      src = k.src[i];
      dst = k.dst[i];
      n = k.floats[i];
    }
  const long long o = 4 * ((long long)blockIdx.x * kScBlock + threadIdx.x);
  if (o + 4 <= n) {
    reinterpret_cast<float4*>(dst)[o / 4] = reinterpret_cast<const float4*>(src)[o / 4];
  } else {
    for (long long i = o; i < n; ++i) dst[i] = src[i];
  }
}

// scratch for buffers of up to `records` records; never shrinks (allocates when it grows: not capturable)
int score_reserve(sit_handle* h, size_t records) {
  const size_t chunks = (records + kScBlock - 1) / kScBlock;
  if (h->score && chunks <= h->score_chunks) return SIT_OK;
  const size_t bytes = chunks * sizeof(ScPart);
  unsigned char* p = nullptr;
  if (setup_alloc(&p, bytes) != hipSuccess) return fail(h, SIT_E_NOMEM, "score: hipMalloc of %zu bytes failed", bytes);
  if (h->score) (void)setup_free(h->score);
  h->score = p;
  h->score_chunks = chunks;
  return SIT_OK;
}

int score_launch_reset(sit_handle* h, double* score, hipStream_t s) {
#ifdef SIT_HOST_MEMORY_TEST
  (void)score; (void)s;
  return fail(h, SIT_E_STATE, "score: no device in the host-memory test build");
#else
  hipLaunchKernelGGL(k_score_reset, dim3(1), dim3(SIT_SCORE_DIM), 0, s, score);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
#endif
}

int score_launch_update(sit_handle* h, const sit_score_args* sa, hipStream_t s) {
#ifdef SIT_HOST_MEMORY_TEST
  (void)sa; (void)s;
  return fail(h, SIT_E_STATE, "score: no device in the host-memory test build");
#else
  int rc = score_reserve(h, (size_t)sa->record_capacity);   // a no-op after a sufficient sit_score_reserve
  if (rc) return rc;
  ScArgs a{};
  a.records = sa->records;
  a.record_count = reinterpret_cast<long long*>(sa->record_count);
  a.score = sa->score;
  a.part = reinterpret_cast<ScPart*>(h->score);
  a.limit = sa->episode_limit;
  a.capacity = sa->record_capacity;
  a.flags = sa->flags;
  for (int c = 0; c < SIT_SCORE_CLASSES; ++c) {
    a.any[c] = sa->class_any[c];
    a.none[c] = sa->class_none[c];
  }
  const unsigned chunks = (unsigned)(((size_t)sa->record_capacity + kScBlock - 1) / kScBlock);
  hipLaunchKernelGGL(k_score_chunks, dim3(chunks), dim3(kScBlock), 0, s, a);
  hipLaunchKernelGGL(k_score_finish, dim3(1), dim3(kScBlock), 0, s, a);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
#endif
}

int score_launch_keep(sit_handle* h, const sit_score_keep_args* ka, hipStream_t s) {
#ifdef SIT_HOST_MEMORY_TEST
  (void)ka; (void)s;
  return fail(h, SIT_E_STATE, "score: no device in the host-memory test build");
#else
  ScKeep k{};
  long long most = 1;
  for (int i = 0; i < ka->n_blocks; ++i) {
    k.src[i] = ka->src[i];
    k.dst[i] = ka->dst[i];
    k.floats[i] = ka->floats[i];
    if (ka->floats[i] > most) most = ka->floats[i];
  }
  k.score = ka->score;
  k.stamp = reinterpret_cast<const long long*>(ka->stamp);
  k.n_blocks = ka->n_blocks;
  const long long lanes = (most + 3) / 4;
  hipLaunchKernelGGL(k_score_keep, dim3((unsigned)((lanes + kScBlock - 1) / kScBlock), (unsigned)(ka->n_blocks > 0 ? ka->n_blocks : 1)),
                     dim3(kScBlock), 0, s, k);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
#endif
}

}  // namespace

#endif  // SIT_SCORE_H
