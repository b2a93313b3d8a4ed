// sit_sac_clock.h — the device-side update clock of sit_sac_updates (include/sit.h): its layout, and the one
// function that makes an Adam step's scalars from the hyper-parameters and the step count.
//
// The clock is SIT_SAC_CLOCK_WORDS int64 of device memory.  Words 0..7 are its state (SacClockState order:
// update, critic_steps, policy_steps, alpha_steps, results_written, three zeros); behind them lie two
// "tick" slots (SacTick).  A tick is everything the kernels of one update would otherwise take by value: the
// three optimisers' SacAdamScalars for the step the update takes, the update number of the noise counters,
// the Polyak flag and the row of the results ring.  Update u of a call reads slot u & 1; the one thread that
// finishes the update's losses (sac_finish_losses<true>, sit_sac_grad.h) advances the state words and forms
// the next update's tick in the other slot, so no kernel reads a word that another block of the same launch
// writes.  A call's first tick is formed from the state words by k_sac_clock_begin.
//
// sac_clock_scalars is specified exactly (sit.h), so that the host, NumPy and the device give the same bits:
// powers by repeated squaring in IEEE double without contraction, a correctly rounded double divide and
// square root, one rounding to float32 each.  Host code and device code both compile this file: the device
// copy belongs to sit_kernels.hip, the strictly compiled translation unit; tests/csrc/sac_updates_args_main.cpp
// compiles the host copy alone.
#ifndef SIT_SAC_CLOCK_H
#define SIT_SAC_CLOCK_H

#include <cmath>
#include <cstdint>

#include "sit.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SIT_CLOCK_FN __host__ __device__ inline
#else
#define SIT_CLOCK_FN inline
#endif

namespace {

struct SacAdamScalars {
  float one_minus_beta1, beta2, one_minus_beta2, step_size, sqrt_bias2, eps;
};

// beta^t by repeated squaring: the products in the order sit.h states, each an IEEE double product
SIT_CLOCK_FN double sac_clock_pow_sq(double beta, int64_t t) {
#pragma clang fp reassociate(off) contract(off)
  double r = 1.0, b = beta;
  uint64_t n = (uint64_t)t;
  while (n) {
    if (n & 1) r = r * b;
    b = b * b;
    n >>= 1;
  }
  return r;
}

// the scalars of Adam step t >= 1 (bias1 and bias2 of `o` are not read)
SIT_CLOCK_FN SacAdamScalars sac_clock_scalars(const sit_sac_adam& o, int64_t t) {
#pragma clang fp reassociate(off) contract(off)
  const double bias1 = 1.0 - sac_clock_pow_sq(o.beta1, t);
  const double bias2 = 1.0 - sac_clock_pow_sq(o.beta2, t);
  SacAdamScalars s;
  s.one_minus_beta1 = (float)(1.0 - o.beta1);
  s.beta2 = (float)o.beta2;
  s.one_minus_beta2 = (float)(1.0 - o.beta2);
  s.step_size = (float)(o.lr / bias1);
  s.sqrt_bias2 = (float)sqrt(bias2);
  s.eps = (float)o.eps;
  return s;
}

// ---- the layout ---------------------------------------------------------------------------------
constexpr int kClockStateWords = 8;
enum SacClockWord { kClockUpdate = 0, kClockCriticSteps, kClockPolicySteps, kClockAlphaSteps, kClockResultsWritten };
enum SacClockOptimiser { kClockCritic = 0, kClockPolicy, kClockAlpha };

struct SacTick {
  SacAdamScalars o[3];         // critic, policy, alpha: the step this update takes
  uint64_t update;             // counter words 2, 3 of both noise draws
  int64_t results_row;         // results_written % results_capacity
  int32_t polyak;              // update % target_update_interval == 0
  int32_t reserved;
};
static_assert(sizeof(SacTick) % 8 == 0 && kClockStateWords * 8 + 2 * sizeof(SacTick) <= SIT_SAC_CLOCK_WORDS * 8,
              "the state words and two tick slots fit the clock");

// What forms a tick besides the state words: a call's hyper-parameters, by value in the launches that form one.
struct SacClockHyper {
  sit_sac_adam adam[3];        // critic, policy, alpha
  int64_t target_update_interval, results_capacity;
  int32_t tune;
};

SIT_CLOCK_FN SacTick* sac_clock_tick(int64_t* clock, int slot) {
  return reinterpret_cast<SacTick*>(clock + kClockStateWords) + slot;
}
SIT_CLOCK_FN const SacTick* sac_clock_tick(const int64_t* clock, int slot) {
  return reinterpret_cast<const SacTick*>(clock + kClockStateWords) + slot;
}

// the tick of the update the state words name, into `slot`
SIT_CLOCK_FN void sac_clock_form_tick(int64_t* clock, const SacClockHyper& hy, int slot) {
  SacTick* t = sac_clock_tick(clock, slot);
  t->o[kClockCritic] = sac_clock_scalars(hy.adam[kClockCritic], clock[kClockCriticSteps] + 1);
  t->o[kClockPolicy] = sac_clock_scalars(hy.adam[kClockPolicy], clock[kClockPolicySteps] + 1);
  t->o[kClockAlpha] = sac_clock_scalars(hy.adam[kClockAlpha], clock[kClockAlphaSteps] + 1);
  const int64_t u = clock[kClockUpdate];
  t->update = (uint64_t)u;
  const int64_t row = clock[kClockResultsWritten] % hy.results_capacity;
  t->results_row = row < 0 ? row + hy.results_capacity : row;    // (a count a caller made negative stays in the ring)
  t->polyak = u % hy.target_update_interval == 0;
  t->reserved = 0;
}

// one update done: the state words move on, and the next update's tick goes to `next_slot`
SIT_CLOCK_FN void sac_clock_advance(int64_t* clock, const SacClockHyper& hy, int next_slot) {
  clock[kClockUpdate] += 1;
  clock[kClockCriticSteps] += 1;
  clock[kClockPolicySteps] += 1;
  if (hy.tune) clock[kClockAlphaSteps] += 1;
  clock[kClockResultsWritten] += 1;
  sac_clock_form_tick(clock, hy, next_slot);
}

}  // namespace

#endif  // SIT_SAC_CLOCK_H
