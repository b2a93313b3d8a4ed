// sit_replay.h — device-side replay memory (include/sit.h: sit_replay_*).
//
// The reference's memory.push / memory.sample (test_beds/main_ast.py:350-396) on the transition
// records the step kernels append: a ring whose contents depend on the records only, never on the
// order in which waves reached the counter, and minibatches that depend on (seed, draw number) only.
//
// Push, on the caller's stream; no block of these kernels waits on another one:
//   k_replay_keys     item i < src_capacity: key = env id of record i as uint32 (rows past the count:
//                     0xFFFFFFFF), value = i
//   hipcub::DeviceRadixSort::SortPairs   stable, so equal ids keep their source order: value j of the
//                     result is the source row of canonical record j
//   k_replay_scatter  canonical record j -> slot (pushed + j) mod capacity, 16 bytes per lane; only
//                     the last `capacity` records are copied, so no slot is written twice
//   k_replay_pushed   one thread: pushed += n, dropped += count - n
// Sample:
//   k_replay_gather   one lane per (u, b): the keyed permutation, then the record split into the outputs
//                     (kNorm: state and next_state through the affine of sit_obsnorm.h as they are copied;
//                     sit_replay_sample_normalised only)
//   k_replay_drawn    one thread: draws += n_batches
//
// Included from sit_kernels.hip only (the strictly compiled translation unit).  Records and sampled
// values are moved as bits: NaN payloads and -0.0 survive.
#ifndef SIT_REPLAY_H
#define SIT_REPLAY_H

#include <hipcub/hipcub.hpp>

#include "sit_host.h"
#include "sit_obsnorm.h"

namespace {

constexpr int kRpBlock = 256;
constexpr uint32_t kRpInvalidKey = 0xFFFFFFFFu;   // rows past the count
constexpr uint32_t kRpNoIdKey = 0xFFFFFFFEu;      // valid rows whose column 23 is no id
constexpr uint32_t kRpTag = 0x5250u;
constexpr int kRpRounds = 4;

// Sort scratch of `items` records behind h->replay: keys in/out, values in/out, then hipcub's temporary storage.
struct RpScratch {
  uint32_t *key_in, *key_out, *val_in, *val_out;
  void* temp;
};

size_t rp_array_bytes(size_t items) { return align256(4 * items); }

RpScratch rp_scratch(const sit_handle* h) {
  const size_t a = rp_array_bytes(h->replay_items);
  unsigned char* p = h->replay;
  return RpScratch{reinterpret_cast<uint32_t*>(p), reinterpret_cast<uint32_t*>(p + a), reinterpret_cast<uint32_t*>(p + 2 * a),
                   reinterpret_cast<uint32_t*>(p + 3 * a), p + 4 * a};
}

// valid records of a source buffer: the kernels count every record and write those below the capacity
__device__ inline long long rp_count(const int32_t* src_count) {
  const int c = *src_count;
  return c > 0 ? c : 0;
}

template <typename R>
__global__ __launch_bounds__(kRpBlock) void k_replay_keys(const R* __restrict__ src, const int32_t* __restrict__ src_count,
                                                          int src_capacity, uint32_t* __restrict__ key,
                                                          uint32_t* __restrict__ val) {
  const int i = blockIdx.x * kRpBlock + threadIdx.x;
  if (i >= src_capacity) return;
  uint32_t k = kRpInvalidKey;
  if (i < rp_count(src_count)) {
    const double id = (double)src[(size_t)i * SIT_TRANSITION_DIM + SIT_TRANSITION_DIM - 1];
    k = id >= 0.0 && id < 4294967294.0 ? (uint32_t)id : kRpNoIdKey;
  }
  key[i] = k;
  val[i] = (uint32_t)i;
}

// one 16-byte chunk of one canonical record per lane (chunks: 16-byte chunks per record, 6 or 12)
__global__ __launch_bounds__(kRpBlock) void k_replay_scatter(const uint4* __restrict__ src, const int32_t* __restrict__ src_count,
                                                             int src_capacity, const uint32_t* __restrict__ order,
                                                             uint4* __restrict__ ring, const long long* __restrict__ cursor,
                                                             int capacity, int chunks) {
  const long long t = (long long)blockIdx.x * kRpBlock + threadIdx.x;
  const long long j = t / chunks;
  const int q = (int)(t - j * chunks);
  const long long c = rp_count(src_count);
  const long long n = c < src_capacity ? c : src_capacity;
  if (j >= n || j < n - capacity) return;
  const uint32_t row = order[j];
  if (row >= (uint32_t)src_capacity) return;   // cannot happen: the values are a permutation of the rows
  const long long slot = (cursor[0] + j) % capacity;
  ring[slot * chunks + q] = src[(size_t)row * chunks + q];
}

__global__ void k_replay_pushed(const int32_t* __restrict__ src_count, int src_capacity, long long* cursor) {
  const long long c = rp_count(src_count);
  const long long n = c < src_capacity ? c : src_capacity;
  cursor[0] += n;
  cursor[1] += c - n;
}

// P_{seed,draw}(x) for x < size (include/sit.h "replay memory"): 4 Feistel rounds on 2h bits, cycle-walked
__device__ inline uint32_t rp_permute(uint32_t x, uint32_t size, int h, uint64_t seed, uint64_t draw) {
  const uint32_t low = (1u << h) - 1u;
  do {
    uint32_t left = x >> h, right = x & low;
#pragma unroll
    for (int r = 0; r < kRpRounds; ++r) {
      uint32_t c[4] = {right, (kRpTag << 8) | (uint32_t)r, (uint32_t)draw, (uint32_t)(draw >> 32)};
      philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
      const uint32_t f = left ^ (c[0] & low);
      left = right;
      right = f;
    }
    x = (left << h) | right;
  } while (x >= size);
  return x;
}

template <typename R>
struct RpSample {
  const R* ring;
  const long long* cursor;
  int capacity, batch, n_batches;
  uint64_t seed;
  R *state, *action, *reward, *next_state, *mask;
  int32_t *env, *index;
  const float* affine;   // kNorm only
};

template <typename R, bool kNorm>
__global__ __launch_bounds__(kRpBlock) void k_replay_gather(RpSample<R> a) {
  const long long t = (long long)blockIdx.x * kRpBlock + threadIdx.x;
  if (t >= (long long)a.batch * a.n_batches) return;
  const int u = (int)(t / a.batch), b = (int)(t - (long long)u * a.batch);
  const long long pushed = a.cursor[0];
  const uint32_t size = (uint32_t)(pushed < a.capacity ? pushed : a.capacity);
  constexpr int kPer = 16 / (int)sizeof(R);          // reals per 16-byte chunk
  constexpr int kChunks = SIT_TRANSITION_DIM / kPer;
  union { uint4 v[kChunks]; R r[SIT_TRANSITION_DIM]; } rec;
  int32_t idx = -1, env = 0;
  if (size == 0) {
#pragma unroll
    for (int q = 0; q < kChunks; ++q) rec.v[q] = make_uint4(0, 0, 0, 0);
  } else {
    int bits = 32 - __clz(size - 1);                 // bit_length(size - 1); __clz(0) is 32
    if (bits < 2) bits = 2;
    idx = (int32_t)rp_permute((uint32_t)b % size, size, (bits + 1) / 2, a.seed, (uint64_t)a.cursor[2] + (uint64_t)u);
    const uint4* row = reinterpret_cast<const uint4*>(a.ring + (size_t)idx * SIT_TRANSITION_DIM);
#pragma unroll
    for (int q = 0; q < kChunks; ++q) rec.v[q] = row[q];
    const double id = (double)rec.r[SIT_TRANSITION_DIM - 1];
    env = id >= 0.0 && id < 2147483648.0 ? (int32_t)id : -1;
  }
  if (kNorm) {
#pragma unroll
    for (int j = 0; j < SIT_OBS_DIM; ++j) {
      const R shift = (R)a.affine[kOnShift + j], scale = (R)a.affine[kOnScale + j];
      a.state[t * SIT_OBS_DIM + j] = obsnorm_apply<R>(rec.r[j], shift, scale);
      a.next_state[t * SIT_OBS_DIM + j] = obsnorm_apply<R>(rec.r[SIT_OBS_DIM + 2 + j], shift, scale);
    }
  } else {
#pragma unroll
    for (int j = 0; j < SIT_OBS_DIM; ++j) {
      a.state[t * SIT_OBS_DIM + j] = rec.r[j];
      a.next_state[t * SIT_OBS_DIM + j] = rec.r[SIT_OBS_DIM + 2 + j];
    }
  }
  a.action[t] = rec.r[SIT_OBS_DIM];
  a.reward[t] = rec.r[SIT_OBS_DIM + 1];
  a.mask[t] = rec.r[SIT_TRANSITION_DIM - 2];
  a.env[t] = env;
  a.index[t] = idx;
}

__global__ void k_replay_drawn(long long* cursor, int n_batches) { cursor[2] += n_batches; }

// bytes of hipcub's temporary storage for `items` pairs: a host-side query that launches nothing; the
// last answer is kept, so a loop of equal pushes asks once
int replay_temp_bytes(sit_handle* h, size_t items, hipStream_t s, size_t* bytes) {
  if (items != h->replay_asked) {
    size_t need = 0;
    const uint32_t* none = nullptr;
    uint32_t* nout = nullptr;
    HIP_TRY(h, hipcub::DeviceRadixSort::SortPairs(nullptr, need, none, nout, none, nout, (int)items, 0, 32, s));
    h->replay_asked = items;
    h->replay_answer = need;
  }
  *bytes = h->replay_answer;
  return SIT_OK;
}

// scratch for source buffers of up to `items` records and at least `min_temp` bytes of sort storage; never
// shrinks (allocates when it grows: not capturable)
int replay_reserve(sit_handle* h, size_t items, hipStream_t s, size_t min_temp = 0) {
#ifdef SIT_HOST_MEMORY_TEST
  (void)items; (void)s; (void)min_temp;
  return fail(h, SIT_E_STATE, "replay: no device in the host-memory test build");
#else
  if (h->replay && items <= h->replay_items && min_temp <= h->replay_temp) return SIT_OK;
  if (items < h->replay_items) items = h->replay_items;
  size_t temp = 0;
  int rc = replay_temp_bytes(h, items, s, &temp);
  if (rc) return rc;
  temp = align256(temp > min_temp ? temp : min_temp);
  if (temp < h->replay_temp) temp = h->replay_temp;
  const size_t bytes = 4 * rp_array_bytes(items) + temp;
  unsigned char* p = nullptr;
  if (setup_alloc(&p, bytes) != hipSuccess) return fail(h, SIT_E_NOMEM, "replay: hipMalloc of %zu bytes failed", bytes);
  if (h->replay) (void)setup_free(h->replay);
  h->replay = p;
  h->replay_items = items;
  h->replay_temp = temp;
  return SIT_OK;
#endif
}

template <typename R>
int replay_launch_push(sit_handle* h, const sit_replay_push_args* a, hipStream_t s) {
#ifdef SIT_HOST_MEMORY_TEST
  (void)a; (void)s;
  return fail(h, SIT_E_STATE, "replay: no device in the host-memory test build");
#else
  const size_t items = (size_t)a->src_capacity;
  size_t temp = 0;
  int rc = replay_temp_bytes(h, items, s, &temp);
  if (rc) return rc;
  rc = replay_reserve(h, items, s, temp);   // a no-op after a sufficient sit_replay_reserve
  if (rc) return rc;
  const RpScratch sc = rp_scratch(h);
  const int chunks = SIT_TRANSITION_DIM * (int)sizeof(R) / 16;
  const R* src = (const R*)a->src;
  long long* cursor = reinterpret_cast<long long*>(a->cursor);
  hipLaunchKernelGGL(k_replay_keys<R>, dim3((unsigned)((items + kRpBlock - 1) / kRpBlock)), dim3(kRpBlock), 0, s, src,
                     a->src_count, a->src_capacity, sc.key_in, sc.val_in);
  HIP_TRY(h, hipGetLastError());
  size_t have = h->replay_temp;
  HIP_TRY(h, hipcub::DeviceRadixSort::SortPairs(sc.temp, have, (const uint32_t*)sc.key_in, sc.key_out,
                                                (const uint32_t*)sc.val_in, sc.val_out, a->src_capacity, 0, 32, s));
  const size_t lanes = items * (size_t)chunks;
  hipLaunchKernelGGL(k_replay_scatter, dim3((unsigned)((lanes + kRpBlock - 1) / kRpBlock)), dim3(kRpBlock), 0, s,
                     reinterpret_cast<const uint4*>(a->src), a->src_count, a->src_capacity, (const uint32_t*)sc.val_out,
                     reinterpret_cast<uint4*>(a->ring), (const long long*)cursor, a->capacity, chunks);
  hipLaunchKernelGGL(k_replay_pushed, dim3(1), dim3(1), 0, s, a->src_count, a->src_capacity, cursor);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
#endif
}

// affine: NULL for the plain gather, else the normalised one (sit_replay_sample_normalised)
template <typename R>
int replay_launch_sample(sit_handle* h, const sit_replay_sample_args* a, hipStream_t s, const float* affine = nullptr) {
#ifdef SIT_HOST_MEMORY_TEST
  (void)a; (void)s; (void)affine;
  return fail(h, SIT_E_STATE, "replay: no device in the host-memory test build");
#else
  RpSample<R> g{};
  g.ring = (const R*)a->ring;
  g.cursor = reinterpret_cast<const long long*>(a->cursor);
  g.capacity = a->capacity;
  g.batch = a->batch;
  g.n_batches = a->n_batches;
  g.seed = a->seed;
  g.state = (R*)a->state;
  g.action = (R*)a->action;
  g.reward = (R*)a->reward;
  g.next_state = (R*)a->next_state;
  g.mask = (R*)a->mask;
  g.env = a->env;
  g.index = a->index;
  g.affine = affine;
  const long long lanes = (long long)a->batch * a->n_batches;
  const dim3 grid((unsigned)((lanes + kRpBlock - 1) / kRpBlock));
  if (affine)
    hipLaunchKernelGGL((k_replay_gather<R, true>), grid, dim3(kRpBlock), 0, s, g);
  else
    hipLaunchKernelGGL((k_replay_gather<R, false>), grid, dim3(kRpBlock), 0, s, g);
  hipLaunchKernelGGL(k_replay_drawn, dim3(1), dim3(1), 0, s, reinterpret_cast<long long*>(a->cursor), a->n_batches);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
#endif
}

}  // namespace

#endif  // SIT_REPLAY_H
