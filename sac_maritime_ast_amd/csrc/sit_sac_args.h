// sit_sac_args.h — argument checks of sit_sac_target / sit_sac_polyak (include/sit.h), host code that
// depends on nothing but the public header: the library calls them before any launch, and
// tests/csrc/sac_args_main.cpp calls them alone under ASan + UBSan.
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

}  // namespace

#endif  // SIT_SAC_ARGS_H
