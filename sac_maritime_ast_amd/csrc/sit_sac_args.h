// sit_sac_args.h — argument checks of sit_sac_target / sit_sac_polyak and of sit_sac_critic_step /
// sit_sac_policy_step and of sit_sac_updates / sit_sac_adam_scalars (include/sit.h), host code that depends
// on nothing but the public header: the library calls them before any launch, and tests/csrc/sac_args_main.cpp,
// tests/csrc/sac_update_args_main.cpp and tests/csrc/sac_updates_args_main.cpp call them alone under
// ASan + UBSan.
//
// Each returns NULL for acceptable arguments, or a static string naming the first thing wrong.
#ifndef SIT_SAC_ARGS_H
#define SIT_SAC_ARGS_H

#include <cstdint>

#include "sit.h"

namespace {

constexpr uintptr_t kSacWeightAlign = 16;   // the kernels read W2^T and the Polyak blocks as float4

inline const char* sac_target_args_error(const sit_sac_target_args* a) {
  if (!a) return "sac: null args";
  if (a->batch <= 0) return "sac: batch must be positive";
  if (!a->actor_weights) return "sac: actor_weights is required";
  if (!a->critic_weights) return "sac: critic_weights is required";
  if (!a->alpha) return "sac: alpha is required";
  if (!a->next_state) return "sac: next_state is required";
  if (!a->reward) return "sac: reward is required";
  if (!a->mask) return "sac: mask is required";
  if (!a->y) return "sac: y is required";
  if ((uintptr_t)a->actor_weights % kSacWeightAlign) return "sac: actor_weights must be 16-byte aligned";
  if ((uintptr_t)a->critic_weights % kSacWeightAlign) return "sac: critic_weights must be 16-byte aligned";
  if ((uintptr_t)a->alpha % sizeof(float)) return "sac: alpha must be 4-byte aligned";
  return nullptr;
}

inline const char* sac_polyak_args_error(const float* target, const float* online, int64_t n) {
  if (!target) return "sac: target is required";
  if (!online) return "sac: online is required";
  if (n <= 0) return "sac: n must be positive";
  if (n > ((int64_t)1 << 34)) return "sac: n must not exceed 2^34";
  if ((uintptr_t)target % kSacWeightAlign) return "sac: target must be 16-byte aligned";
  if ((uintptr_t)online % kSacWeightAlign) return "sac: online must be 16-byte aligned";
  return nullptr;
}

// the float32 workspace of the gradient half: two network passes of SIT_SAC_WORKSPACE_ROW floats per row
inline int64_t sac_workspace_floats(int32_t batch) {
  return batch > 0 ? 2 * (int64_t)batch * SIT_SAC_WORKSPACE_ROW : 0;
}

inline const char* sac_adam_error(const sit_sac_adam* o) {
  if (!(o->lr >= 0.0)) return "sac: lr must be >= 0";
  if (!(o->beta1 >= 0.0 && o->beta1 < 1.0) || !(o->beta2 >= 0.0 && o->beta2 < 1.0)) return "sac: betas must lie in [0, 1)";
  if (!(o->eps >= 0.0)) return "sac: eps must be >= 0";
  if (!(o->bias1 > 0.0 && o->bias1 <= 1.0) || !(o->bias2 > 0.0 && o->bias2 <= 1.0))
    return "sac: the bias corrections must lie in (0, 1]";
  return nullptr;
}

inline const char* sac_critic_step_args_error(const sit_sac_critic_step_args* a) {
  if (!a) return "sac: null args";
  if (a->batch <= 0) return "sac: batch must be positive";
  if (!a->critic_weights) return "sac: critic_weights is required";
  if (!a->critic_m) return "sac: critic_m is required";
  if (!a->critic_v) return "sac: critic_v is required";
  if (!a->state) return "sac: state is required";
  if (!a->action) return "sac: action is required";
  if (!a->y) return "sac: y is required";
  if (!a->workspace) return "sac: workspace is required";
  if (!a->results) return "sac: results is required";
  if ((uintptr_t)a->critic_weights % kSacWeightAlign) return "sac: critic_weights must be 16-byte aligned";
  if ((uintptr_t)a->critic_m % kSacWeightAlign) return "sac: critic_m must be 16-byte aligned";
  if ((uintptr_t)a->critic_v % kSacWeightAlign) return "sac: critic_v must be 16-byte aligned";
  if ((uintptr_t)a->workspace % sizeof(float)) return "sac: workspace must be 4-byte aligned";
  if ((uintptr_t)a->results % sizeof(float)) return "sac: results must be 4-byte aligned";
  if (a->workspace_floats < sac_workspace_floats(a->batch)) return "sac: workspace is too small";
  return sac_adam_error(&a->adam);
}

inline const char* sac_policy_step_args_error(const sit_sac_policy_step_args* a) {
  if (!a) return "sac: null args";
  if (a->batch <= 0) return "sac: batch must be positive";
  if (!a->actor_weights) return "sac: actor_weights is required";
  if (!a->actor_m) return "sac: actor_m is required";
  if (!a->actor_v) return "sac: actor_v is required";
  if (!a->critic_weights) return "sac: critic_weights is required";
  if (!a->alpha) return "sac: alpha is required";
  if (a->tune && !a->log_alpha) return "sac: log_alpha is required";
  if (a->tune && !a->log_alpha_m) return "sac: log_alpha_m is required";
  if (a->tune && !a->log_alpha_v) return "sac: log_alpha_v is required";
  if (!a->state) return "sac: state is required";
  if (!a->workspace) return "sac: workspace is required";
  if (!a->results) return "sac: results is required";
  if ((uintptr_t)a->actor_weights % kSacWeightAlign) return "sac: actor_weights must be 16-byte aligned";
  if ((uintptr_t)a->actor_m % kSacWeightAlign) return "sac: actor_m must be 16-byte aligned";
  if ((uintptr_t)a->actor_v % kSacWeightAlign) return "sac: actor_v must be 16-byte aligned";
  if ((uintptr_t)a->critic_weights % kSacWeightAlign) return "sac: critic_weights must be 16-byte aligned";
  if ((uintptr_t)a->alpha % sizeof(float)) return "sac: alpha must be 4-byte aligned";
  if (a->tune && ((uintptr_t)a->log_alpha % sizeof(float) || (uintptr_t)a->log_alpha_m % sizeof(float) ||
                  (uintptr_t)a->log_alpha_v % sizeof(float)))
    return "sac: log_alpha and its moments must be 4-byte aligned";
  if ((uintptr_t)a->workspace % sizeof(float)) return "sac: workspace must be 4-byte aligned";
  if ((uintptr_t)a->results % sizeof(float)) return "sac: results must be 4-byte aligned";
  if (a->workspace_floats < sac_workspace_floats(a->batch)) return "sac: workspace is too small";
  if (const char* why = sac_adam_error(&a->adam)) return why;
  return a->tune ? sac_adam_error(&a->alpha_adam) : nullptr;
}

// an optimiser of sit_sac_updates: its bias corrections come from the clock, what the caller left there is not read
inline const char* sac_clocked_adam_error(const sit_sac_adam* o) {
  sit_sac_adam c = *o;
  c.bias1 = c.bias2 = 1.0;
  return sac_adam_error(&c);
}

inline const char* sac_updates_args_error(const sit_sac_updates_args* a) {
  if (!a) return "sac: null args";
  if (a->mode != SIT_SAC_UPDATES_PLAIN && a->mode != SIT_SAC_UPDATES_TILED && a->mode != SIT_SAC_UPDATES_WIDE)
    return "sac: mode must be one of SIT_SAC_UPDATES_*";
  if (a->batch <= 0) return "sac: batch must be positive";
  if (a->n_updates <= 0) return "sac: n_updates must be positive";
  if (a->target_update_interval <= 0) return "sac: target_update_interval must be positive";
  if (a->results_capacity <= 0) return "sac: results_capacity must be positive";
  if (!a->critic_weights) return "sac: critic_weights is required";
  if (!a->critic_m) return "sac: critic_m is required";
  if (!a->critic_v) return "sac: critic_v is required";
  if (!a->actor_weights) return "sac: actor_weights is required";
  if (!a->actor_m) return "sac: actor_m is required";
  if (!a->actor_v) return "sac: actor_v is required";
  if (!a->target_weights) return "sac: target_weights is required";
  if (!a->alpha) return "sac: alpha is required";
  if (a->tune && !a->log_alpha) return "sac: log_alpha is required";
  if (a->tune && !a->log_alpha_m) return "sac: log_alpha_m is required";
  if (a->tune && !a->log_alpha_v) return "sac: log_alpha_v is required";
  if (!a->state) return "sac: state is required";
  if (!a->action) return "sac: action is required";
  if (!a->reward) return "sac: reward is required";
  if (!a->next_state) return "sac: next_state is required";
  if (!a->mask) return "sac: mask is required";
  if (!a->y) return "sac: y is required";
  if (!a->workspace) return "sac: workspace is required";
  if (!a->clock) return "sac: clock is required";
  if (!a->results) return "sac: results is required";
  if ((uintptr_t)a->critic_weights % kSacWeightAlign) return "sac: critic_weights must be 16-byte aligned";
  if ((uintptr_t)a->critic_m % kSacWeightAlign) return "sac: critic_m must be 16-byte aligned";
  if ((uintptr_t)a->critic_v % kSacWeightAlign) return "sac: critic_v must be 16-byte aligned";
  if ((uintptr_t)a->actor_weights % kSacWeightAlign) return "sac: actor_weights must be 16-byte aligned";
  if ((uintptr_t)a->actor_m % kSacWeightAlign) return "sac: actor_m must be 16-byte aligned";
  if ((uintptr_t)a->actor_v % kSacWeightAlign) return "sac: actor_v must be 16-byte aligned";
  if ((uintptr_t)a->target_weights % kSacWeightAlign) return "sac: target_weights must be 16-byte aligned";
  if ((uintptr_t)a->alpha % sizeof(float)) return "sac: alpha must be 4-byte aligned";
  if (a->tune && ((uintptr_t)a->log_alpha % sizeof(float) || (uintptr_t)a->log_alpha_m % sizeof(float) ||
                  (uintptr_t)a->log_alpha_v % sizeof(float)))
    return "sac: log_alpha and its moments must be 4-byte aligned";
  if ((uintptr_t)a->workspace % sizeof(float)) return "sac: workspace must be 4-byte aligned";
  if ((uintptr_t)a->clock % sizeof(int64_t)) return "sac: clock must be 8-byte aligned";
  if ((uintptr_t)a->results % sizeof(float)) return "sac: results must be 4-byte aligned";
  if (a->workspace_floats < sac_workspace_floats(a->batch)) return "sac: workspace is too small";
  if (const char* why = sac_clocked_adam_error(&a->critic_adam)) return why;
  if (const char* why = sac_clocked_adam_error(&a->actor_adam)) return why;
  return a->tune ? sac_clocked_adam_error(&a->alpha_adam) : nullptr;
}

inline const char* sac_adam_scalars_args_error(const sit_sac_adam* o, int64_t t0, int32_t n, const float* out) {
  if (!o) return "sac: null args";
  if (t0 < 1) return "sac: t0 must be at least 1";
  if (n <= 0) return "sac: n must be positive";
  if (!out) return "sac: out is required";
  if ((uintptr_t)out % sizeof(float)) return "sac: out must be 4-byte aligned";
  return sac_clocked_adam_error(o);
}

}  // namespace

#endif  // SIT_SAC_ARGS_H
