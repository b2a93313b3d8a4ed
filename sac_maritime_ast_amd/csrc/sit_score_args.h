// sit_score_args.h — argument checks of sit_score_reset / sit_score_reserve / sit_score_update /
// sit_score_keep (include/sit.h), host code that depends on nothing but the public header: the library
// calls them before any launch, and tests/csrc/score_args_main.cpp calls them alone under ASan + UBSan.
//
// Each returns NULL for acceptable arguments, or a static string naming the first thing wrong.
#ifndef SIT_SCORE_ARGS_H
#define SIT_SCORE_ARGS_H

#include "sit.h"

namespace {

constexpr uintptr_t kScoreBlockAlign = 16;            // k_score_keep copies float4
constexpr int64_t kScoreMaxFloats = (int64_t)1 << 34;

inline const char* score_block_error(const double* score) {
  if (!score) return "score: score is required";
  if ((uintptr_t)score % sizeof(double)) return "score: score must be 8-byte aligned";
  return nullptr;
}

inline const char* score_reserve_args_error(int32_t max_records) {
  if (max_records <= 0) return "score: max_records must be positive";
  return nullptr;
}

inline const char* score_update_args_error(const sit_score_args* a) {
  if (!a) return "score: null args";
  if (a->record_capacity <= 0) return "score: record_capacity must be positive";
  if (a->flags & ~(uint32_t)(SIT_SCORE_CONSUME | SIT_SCORE_FRESH)) return "score: flags has unknown bits";
  if (a->episode_limit < 0) return "score: episode_limit must be >= 0";
  if (!a->records) return "score: records is required";
  if (!a->record_count) return "score: record_count is required";
  if ((uintptr_t)a->records % sizeof(double)) return "score: records must be 8-byte aligned";
  if ((uintptr_t)a->record_count % sizeof(int64_t)) return "score: record_count must be 8-byte aligned";
  return score_block_error(a->score);
}

inline const char* score_keep_args_error(const sit_score_keep_args* a) {
  if (!a) return "score: null args";
  if (a->n_blocks < 0 || a->n_blocks > SIT_SCORE_KEEP_BLOCKS) return "score: n_blocks must lie in 0..4";
  for (int i = 0; i < a->n_blocks; ++i) {
    if (!a->src[i]) return "score: src is required";
    if (!a->dst[i]) return "score: dst is required";
    if (a->floats[i] <= 0) return "score: floats must be positive";
    if (a->floats[i] > kScoreMaxFloats) return "score: floats must not exceed 2^34";
    if ((uintptr_t)a->src[i] % kScoreBlockAlign) return "score: src must be 16-byte aligned";
    if ((uintptr_t)a->dst[i] % kScoreBlockAlign) return "score: dst must be 16-byte aligned";
  }
  if (a->stamp && (uintptr_t)a->stamp % sizeof(int64_t)) return "score: stamp must be 8-byte aligned";
  return score_block_error(a->score);
}

}  // namespace

#endif  // SIT_SCORE_ARGS_H
