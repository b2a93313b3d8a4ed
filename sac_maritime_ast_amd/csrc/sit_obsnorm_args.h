// sit_obsnorm_args.h — argument checks of sit_obsnorm_reset / sit_obsnorm_reserve / sit_obsnorm_update /
// sit_obsnorm_apply / sit_obsnorm_fold and of sit_replay_sample_normalised's affine (include/sit.h), host code
// that depends on nothing but the public header: the library calls them before any launch, and
// tests/csrc/obsnorm_args_main.cpp calls them alone under ASan + UBSan.
//
// Each returns NULL for acceptable arguments, or a static string naming the first thing wrong.
#ifndef SIT_OBSNORM_ARGS_H
#define SIT_OBSNORM_ARGS_H

#include <math.h>

#include "sit.h"

namespace {

constexpr uintptr_t kObsnormAffineAlign = 16;          // read as float4 rows by the fold and the gather
constexpr int64_t kObsnormMaxRows = (int64_t)1 << 30;   // 5 pairs per row, 256 per block: the grid stays below 2^31

inline const char* obsnorm_block_error(const double* block) {
  if (!block) return "obsnorm: block is required";
  if ((uintptr_t)block % sizeof(double)) return "obsnorm: block must be 8-byte aligned";
  return nullptr;
}

inline const char* obsnorm_affine_error(const float* affine) {
  if (!affine) return "obsnorm: affine is required";
  if ((uintptr_t)affine % kObsnormAffineAlign) return "obsnorm: affine must be 16-byte aligned";
  return nullptr;
}

// min_std: NULL, or ten host floats, each finite and >= 0
inline const char* obsnorm_reset_args_error(const double* block, const float* affine, const float* min_std) {
  if (const char* why = obsnorm_block_error(block)) return why;
  if (const char* why = obsnorm_affine_error(affine)) return why;
  if (min_std)
    for (int i = 0; i < SIT_OBS_DIM; ++i)
      if (!(min_std[i] >= 0.0f) || isinf(min_std[i])) return "obsnorm: min_std must be finite and >= 0";
  return nullptr;
}

inline const char* obsnorm_reserve_args_error(int32_t max_new) {
  if (max_new <= 0) return "obsnorm: max_new must be positive";
  return nullptr;
}

// reserved: the records the handle's scratch holds (sit_obsnorm_reserve)
inline const char* obsnorm_update_args_error(const sit_obsnorm_args* a, size_t real_bytes, int64_t reserved) {
  if (!a) return "obsnorm: null args";
  if (a->capacity <= 0) return "obsnorm: capacity must be positive";
  if (a->max_new <= 0) return "obsnorm: max_new must be positive";
  if ((int64_t)a->max_new > reserved) return "obsnorm: max_new exceeds the reserve (sit_obsnorm_reserve)";
  if (!a->ring) return "obsnorm: ring is required";
  if (!a->cursor) return "obsnorm: cursor is required";
  if ((uintptr_t)a->ring % (4 * real_bytes)) return "obsnorm: ring must be aligned to 4 reals";
  if ((uintptr_t)a->cursor % sizeof(int64_t)) return "obsnorm: cursor must be 8-byte aligned";
  if (const char* why = obsnorm_block_error(a->block)) return why;
  return obsnorm_affine_error(a->affine);
}

inline const char* obsnorm_apply_args_error(const float* affine, const void* rows_a, const void* rows_b, int64_t n_rows,
                                            size_t real_bytes) {
  if (const char* why = obsnorm_affine_error(affine)) return why;
  if (!rows_a) return "obsnorm: rows_a is required";
  if (n_rows <= 0) return "obsnorm: n_rows must be positive";
  if (n_rows > kObsnormMaxRows) return "obsnorm: n_rows must not exceed 2^30";
  if ((uintptr_t)rows_a % (2 * real_bytes)) return "obsnorm: rows_a must be aligned to 2 reals";
  if (rows_b && (uintptr_t)rows_b % (2 * real_bytes)) return "obsnorm: rows_b must be aligned to 2 reals";
  return nullptr;
}

inline const char* obsnorm_fold_args_error(const float* affine, const float* src, const float* dst) {
  if (const char* why = obsnorm_affine_error(affine)) return why;
  if (!src) return "obsnorm: src is required";
  if (!dst) return "obsnorm: dst is required";
  if ((uintptr_t)src % 16) return "obsnorm: src must be 16-byte aligned";
  if ((uintptr_t)dst % 16) return "obsnorm: dst must be 16-byte aligned";
  const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst, bytes = (uintptr_t)SIT_ACTOR_WEIGHTS * sizeof(float);
  if (s < d + bytes && d < s + bytes) return "obsnorm: src and dst must not overlap";
  return nullptr;
}

}  // namespace

#endif  // SIT_OBSNORM_ARGS_H
