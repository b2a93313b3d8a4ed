// sit_episodes.h — device-side episode reducer (include/sit.h: sit_episodes_*).
//
// A post-pass over the rows a rollout (or step) has just written: per env it keeps the running
// values of the reference's driver loop (test_beds/main_ast.py:310-440: episode_reward,
// episode_steps, status, action_record[i_episode]) across launches and appends one fixed-size
// record per finished episode, plus a histogram of the terminal status bits.
//
// Three launches per update on the caller's stream; no block waits on another one:
//   k_episodes_count  each lane owns one env and counts its finished episodes; block totals
//   k_episodes_scan   one block: exclusive scan of the block totals; latches *record_count as the
//                     base and rows_seen as this update's first row; advances both
//   k_episodes_walk   each lane walks its env's rows; its first record slot is
//                     base + block offset + in-block exclusive prefix of the per-env counts
// so the slot of every record is a function of the inputs only.
//
// Included from sit_kernels.hip only (the strictly compiled translation unit): the return is one
// IEEE float64 add per row in row order, which fast-math could reassociate.
#ifndef SIT_EPISODES_H
#define SIT_EPISODES_H

#include "sit_host.h"

namespace {

constexpr int kEpBlock = 256;   // threads per block: one env per lane
constexpr int kEpBatch = 8;     // rows fetched ahead of the walk's dependent add chain

// Accumulator blob (sit_episodes_get / _set): a 256-byte header (int64 rows_seen), then per env, each
// array 256-byte aligned: ret f64[n], episode i64[n], steps i32[n], events i32[n], angle f64[14][n].
struct EpLayout {
  size_t ret, episode, steps, events, angle, blob_bytes;
  // scratch behind the blob (not checkpointed): per-env counts, per-block totals and offsets, and the
  // two values the scan latches for the walk (base slot, first row index)
  size_t cnt, btot, boff, latch, bytes;
  int blocks;
};

EpLayout ep_layout(const sit_handle* h) {
  const size_t n = (size_t)h->n_env;
  EpLayout L{};
  L.blocks = (int)((n + kEpBlock - 1) / kEpBlock);
  size_t o = 256;
  L.ret = o; o = align256(o + 8 * n);
  L.episode = o; o = align256(o + 8 * n);
  L.steps = o; o = align256(o + 4 * n);
  L.events = o; o = align256(o + 4 * n);
  L.angle = o; o = align256(o + 8 * n * SIT_EPISODE_ACTIONS);
  L.blob_bytes = o;
  L.cnt = o; o = align256(o + 4 * n);
  L.btot = o; o = align256(o + 4 * (size_t)L.blocks);
  L.boff = o; o = align256(o + 8 * (size_t)L.blocks);
  L.latch = o; o = align256(o + 16);
  L.bytes = o;
  return L;
}

struct EpAcc {
  long long* rows_seen;   // [1]
  double* ret;            // [n]
  long long* episode;     // [n]
  int* steps;             // [n]
  int* events;            // [n]
  double* angle;          // [SIT_EPISODE_ACTIONS][n]
  int* cnt;               // [n]       finished episodes of env e in this update
  int* btot;              // [blocks]  their sum per block
  long long* boff;        // [blocks]  exclusive scan of btot
  long long* latch;       // [2]       base slot, first row index of this update
  int n_env;
  int blocks;
};

EpAcc ep_acc(const sit_handle* h) {
  const EpLayout L = ep_layout(h);
  unsigned char* p = h->episodes;
  EpAcc a{};
  a.rows_seen = reinterpret_cast<long long*>(p);
  a.ret = reinterpret_cast<double*>(p + L.ret);
  a.episode = reinterpret_cast<long long*>(p + L.episode);
  a.steps = reinterpret_cast<int*>(p + L.steps);
  a.events = reinterpret_cast<int*>(p + L.events);
  a.angle = reinterpret_cast<double*>(p + L.angle);
  a.cnt = reinterpret_cast<int*>(p + L.cnt);
  a.btot = reinterpret_cast<int*>(p + L.btot);
  a.boff = reinterpret_cast<long long*>(p + L.boff);
  a.latch = reinterpret_cast<long long*>(p + L.latch);
  a.n_env = h->n_env;
  a.blocks = L.blocks;
  return a;
}

template <typename R>
struct EpRows {
  int n_steps;
  int record_capacity;
  long long env_id_offset;
  const R* reward;               // [n_steps][n_env]
  const uint8_t* done;           // [n_steps][n_env]
  const uint32_t* status;        // [n_steps][n_env]
  const R* action_out;           // [n_steps][n_env][4] or null
  const R* next_state;           // [n_steps][n_env][SIT_OBS_DIM] or null
  double* records;               // [record_capacity][SIT_EPISODE_DIM] or null
  long long* record_count;       // [1]
  unsigned long long* status_hist;   // [32] or null
};

__device__ inline double ep_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// Inclusive sum over the block's kEpBlock lanes (wave prefix, then LDS across the waves); *total
// receives the block's sum.  Every lane of the block calls it.
__device__ inline long long ep_block_scan(long long x, long long* total) {
  __shared__ long long wsum[kEpBlock / kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int off = 1; off < kWave; off <<= 1) {
    const long long y = __shfl_up(x, off);
    if (lane >= off) x += y;
  }
  __syncthreads();   // the previous call's readers are done with wsum
  if (lane == kWave - 1) wsum[wave] = x;
  __syncthreads();
  long long before = 0, all = 0;
  for (int w = 0; w < kEpBlock / kWave; ++w) {
    if (w < wave) before += wsum[w];
    all += wsum[w];
  }
  *total = all;
  return x + before;
}

__global__ __launch_bounds__(kEpBlock) void k_episodes_reset(EpAcc a) {
  const int e = blockIdx.x * kEpBlock + threadIdx.x;
  if (e == 0) *a.rows_seen = 0;
  if (e >= a.n_env) return;
  a.ret[e] = 0.0;
  a.episode[e] = 0;
  a.steps[e] = 0;
  a.events[e] = 0;
  for (int j = 0; j < SIT_EPISODE_ACTIONS; ++j) a.angle[(size_t)j * a.n_env + e] = ep_nan();
}

// 1. count: finished episodes per env (done rows that are not SIT_ST_NO_STEP rows) and per block
__global__ __launch_bounds__(kEpBlock) void k_episodes_count(EpAcc a, int n_steps, const uint8_t* __restrict__ done,
                                                             const uint32_t* __restrict__ status) {
  const int e = blockIdx.x * kEpBlock + threadIdx.x;
  const size_t n = (size_t)a.n_env;
  int c = 0;
  if (e < a.n_env) {
    int k = 0;
    for (; k + kEpBatch <= n_steps; k += kEpBatch) {
      uint8_t d[kEpBatch];
#pragma unroll
      for (int i = 0; i < kEpBatch; ++i) d[i] = done[(size_t)(k + i) * n + e];
#pragma unroll
      for (int i = 0; i < kEpBatch; ++i)
        if (d[i] && !(status[(size_t)(k + i) * n + e] & SIT_ST_NO_STEP)) ++c;
    }
    for (; k < n_steps; ++k)
      if (done[(size_t)k * n + e] && !(status[(size_t)k * n + e] & SIT_ST_NO_STEP)) ++c;
    a.cnt[e] = c;
  }
  long long total;
  (void)ep_block_scan(c, &total);
  if (threadIdx.x == 0) a.btot[blockIdx.x] = (int)total;
}

// 2. scan: one block; exclusive scan of the block totals (any block count), the latches, the counters
__global__ __launch_bounds__(kEpBlock) void k_episodes_scan(EpAcc a, int n_steps, long long* record_count) {
  long long carry = 0;
  for (int b0 = 0; b0 < a.blocks; b0 += kEpBlock) {
    const int b = b0 + threadIdx.x;
    const long long x = b < a.blocks ? a.btot[b] : 0;
    long long total;
    const long long incl = ep_block_scan(x, &total);
    if (b < a.blocks) a.boff[b] = carry + incl - x;
    carry += total;
  }
  if (threadIdx.x == 0) {
    const long long base = *record_count, row0 = *a.rows_seen;
    a.latch[0] = base;
    a.latch[1] = row0;
    *record_count = base + carry;
    *a.rows_seen = row0 + n_steps;
  }
}

// one batch of rows of one env, held in registers (every index is a compile-time constant)
template <typename R>
struct EpBatch {
  R r[kEpBatch];
  R f[kEpBatch];
  uint32_t s[kEpBatch];
  uint8_t d[kEpBatch];
};

// rows k0 .. k0 + kEpBatch - 1 of env e; rows past n_steps read as skipped rows
template <typename R>
__device__ inline void ep_fetch(EpBatch<R>& b, const EpRows<R>& io, int k0, size_t n, int e) {
#pragma unroll
  for (int i = 0; i < kEpBatch; ++i) {
    const int k = k0 + i;
    const bool in = k < io.n_steps;
    const size_t row = (size_t)(in ? k : 0) * n + e;
    b.s[i] = in ? io.status[row] : (uint32_t)SIT_ST_NO_STEP;
    b.d[i] = io.done[row];
    b.r[i] = io.reward[row];
    b.f[i] = io.action_out ? io.action_out[row * 4 + 3] : R(0);
  }
}

// 3. walk: the semantics of include/sit.h ("Episode records"), one env per lane
template <typename R>
__global__ __launch_bounds__(kEpBlock) void k_episodes_walk(EpAcc a, EpRows<R> io) {
  const int e = blockIdx.x * kEpBlock + threadIdx.x;
  const bool live = e < a.n_env;
  const size_t n = (size_t)a.n_env;
  long long total;
  const int mine = live ? a.cnt[e] : 0;
  long long slot = a.latch[0] + a.boff[blockIdx.x] + ep_block_scan(mine, &total) - mine;
  if (!live) return;
  const long long row0 = a.latch[1];
  double ret = a.ret[e];
  long long episode = a.episode[e];
  int steps = a.steps[e], events = a.events[e];
  EpBatch<R> cur, nxt;
  ep_fetch(cur, io, 0, n, e);
  nxt = cur;
  for (int k0 = 0; k0 < io.n_steps; k0 += kEpBatch) {
    if (k0 + kEpBatch < io.n_steps) ep_fetch(nxt, io, k0 + kEpBatch, n, e);
#pragma unroll
    for (int i = 0; i < kEpBatch; ++i) {
      if (cur.s[i] & SIT_ST_NO_STEP) continue;
      const int k = k0 + i;
      const size_t row = (size_t)k * n + e;
      ret = ret + (double)cur.r[i];
      ++steps;
      if (cur.f[i] != R(0)) {
        if (events < SIT_EPISODE_ACTIONS) a.angle[(size_t)events * n + e] = (double)io.action_out[row * 4 + 2];
        ++events;
      }
      if (cur.d[i]) {
        if (slot < io.record_capacity) {
          double* rec = io.records + (size_t)slot * SIT_EPISODE_DIM;
          rec[0] = (double)(io.env_id_offset + e);
          rec[1] = (double)episode;
          rec[2] = (double)steps;
          rec[3] = ret;
          rec[4] = (double)cur.s[i];
          rec[5] = (double)events;
          rec[6] = (double)(row0 + k);
          rec[7] = (double)cur.r[i];
          for (int j = 0; j < SIT_OBS_DIM; ++j)
            rec[8 + j] = io.next_state ? (double)io.next_state[row * SIT_OBS_DIM + j] : ep_nan();
          for (int j = 0; j < SIT_EPISODE_ACTIONS; ++j)
            rec[8 + SIT_OBS_DIM + j] = j < events ? a.angle[(size_t)j * n + e] : ep_nan();
        }
        if (io.status_hist)
          for (uint32_t bits = cur.s[i]; bits; bits &= bits - 1) atomicAdd(io.status_hist + (__ffs(bits) - 1), 1ULL);
        for (int j = 0; j < SIT_EPISODE_ACTIONS && j < events; ++j) a.angle[(size_t)j * n + e] = ep_nan();
        ++slot;
        ++episode;
        ret = 0.0;
        steps = 0;
        events = 0;
      }
    }
    cur = nxt;
  }
  a.ret[e] = ret;
  a.episode[e] = episode;
  a.steps[e] = steps;
  a.events[e] = events;
}

int episodes_alloc(sit_handle* h) {
  if (h->episodes) return SIT_OK;
  const EpLayout L = ep_layout(h);
  unsigned char* p = nullptr;
  if (setup_alloc(&p, L.bytes) != hipSuccess) return fail(h, SIT_E_NOMEM, "episodes: hipMalloc of %zu bytes failed", L.bytes);
  if (setup_zero(p, L.bytes) != hipSuccess) {
    (void)setup_free(p);
    return fail(h, SIT_E_HIP, "episodes: hipMemset failed");
  }
  h->episodes = p;
  return SIT_OK;
}

int episodes_launch_reset(sit_handle* h, hipStream_t s) {
#ifdef SIT_HOST_MEMORY_TEST
  (void)s;
  return fail(h, SIT_E_STATE, "episodes: no device in the host-memory test build");
#else
  const EpAcc a = ep_acc(h);
  hipLaunchKernelGGL(k_episodes_reset, dim3(a.blocks), dim3(kEpBlock), 0, s, a);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
#endif
}

template <typename R>
int episodes_launch_update(sit_handle* h, const sit_episodes_args* ea, hipStream_t s) {
#ifdef SIT_HOST_MEMORY_TEST
  (void)ea; (void)s;
  return fail(h, SIT_E_STATE, "episodes: no device in the host-memory test build");
#else
  const EpAcc a = ep_acc(h);
  EpRows<R> io{};
  io.n_steps = ea->n_steps;
  io.record_capacity = ea->records ? ea->record_capacity : 0;
  io.env_id_offset = ea->env_id_offset;
  io.reward = (const R*)ea->reward;
  io.done = ea->done;
  io.status = ea->status;
  io.action_out = (const R*)ea->action_out;
  io.next_state = (const R*)ea->next_state;
  io.records = ea->records;
  io.record_count = reinterpret_cast<long long*>(ea->record_count);
  io.status_hist = reinterpret_cast<unsigned long long*>(ea->status_hist);
  hipLaunchKernelGGL(k_episodes_count, dim3(a.blocks), dim3(kEpBlock), 0, s, a, ea->n_steps, ea->done, ea->status);
  hipLaunchKernelGGL(k_episodes_scan, dim3(1), dim3(kEpBlock), 0, s, a, ea->n_steps, io.record_count);
  hipLaunchKernelGGL(k_episodes_walk<R>, dim3(a.blocks), dim3(kEpBlock), 0, s, a, io);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
#endif
}

}  // namespace

#endif  // SIT_EPISODES_H
