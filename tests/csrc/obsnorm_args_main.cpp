// Stand-alone driver of the argument checks of sit_obsnorm_reset / sit_obsnorm_reserve / sit_obsnorm_update /
// sit_obsnorm_apply / sit_obsnorm_fold and of sit_replay_sample_normalised's affine (csrc/sit_obsnorm_args.h),
// built by tests/test_obsnorm_host.py with -fsanitize=address,undefined.  It includes nothing but that header
// (and through it include/sit.h): no HIP, no device.  Prints one line per case, "name: message" or "name: ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sit_obsnorm_args.h"

static void show(const char* name, const char* why) { std::printf("%s: %s\n", name, why ? why : "ok"); }

int main() {
  // pointers are only compared and taken modulo their alignment, never dereferenced (min_std apart, which is
  // host data): one aligned heap block serves all
  const size_t block_bytes = (size_t)SIT_ACTOR_WEIGHTS * sizeof(float);
  void* raw = nullptr;
  if (posix_memalign(&raw, 64, 4096 + 3 * block_bytes)) return 2;
  char* bytes = static_cast<char*>(raw);
  double* dbase = static_cast<double*>(raw);
  float* fbase = static_cast<float*>(raw);

  double* block = dbase + 8;
  float* affine = fbase + 256;
  float min_std[SIT_OBS_DIM];
  for (int i = 0; i < SIT_OBS_DIM; ++i) min_std[i] = 0.5f * (float)(i + 1);
  show("reset_good", obsnorm_reset_args_error(block, affine, min_std));
  show("reset_no_min_std", obsnorm_reset_args_error(block, affine, nullptr));
  {
    float zero[SIT_OBS_DIM] = {};
    show("reset_zero_min_std", obsnorm_reset_args_error(block, affine, zero));
    float bad[SIT_OBS_DIM];
    std::memcpy(bad, min_std, sizeof(bad));
    bad[9] = -1e-3f;
    show("reset_bad_min_std", obsnorm_reset_args_error(block, affine, bad));
    bad[9] = 1.0f; bad[0] = NAN;
    show("reset_bad_min_std", obsnorm_reset_args_error(block, affine, bad));
    bad[0] = 1.0f; bad[4] = INFINITY;
    show("reset_bad_min_std", obsnorm_reset_args_error(block, affine, bad));
  }
  show("reset_null_block", obsnorm_reset_args_error(nullptr, affine, min_std));
  show("reset_null_affine", obsnorm_reset_args_error(block, nullptr, min_std));
  for (int off = 1; off < 8; ++off)
    show("reset_misaligned_block", obsnorm_reset_args_error(reinterpret_cast<double*>(bytes + 64 + off), affine, min_std));
  for (int off = 1; off < 4; ++off) {
    show("reset_misaligned_affine", obsnorm_reset_args_error(block, affine + off, min_std));
    show("affine_misaligned", obsnorm_affine_error(affine + off));
  }
  show("affine_good", obsnorm_affine_error(affine));
  show("affine_null", obsnorm_affine_error(nullptr));

  show("reserve_good", obsnorm_reserve_args_error(1));
  show("reserve_good", obsnorm_reserve_args_error(INT32_MAX));

  sit_obsnorm_args g;
  std::memset(&g, 0, sizeof(g));
  g.capacity = 4096;
  g.max_new = 1024;
  g.ring = bytes + 2048;
  g.cursor = reinterpret_cast<const int64_t*>(dbase + 1);
  g.block = block;
  g.affine = affine;
  const int64_t reserved = 1024;
  show("update_good_f32", obsnorm_update_args_error(&g, 4, reserved));
  show("update_good_f64", obsnorm_update_args_error(&g, 8, reserved));
  show("update_null_args", obsnorm_update_args_error(nullptr, 4, reserved));
  {
    sit_obsnorm_args a = g;
    a.max_new = 1024;
    show("update_at_the_reserve", obsnorm_update_args_error(&a, 4, 1024));
    a.max_new = 1025;
    show("update_beyond_the_reserve", obsnorm_update_args_error(&a, 4, 1024));
    a.max_new = 1;
    show("update_beyond_the_reserve", obsnorm_update_args_error(&a, 8, 0));   // nothing was reserved
    a = g; a.capacity = INT32_MAX; a.max_new = INT32_MAX;
    show("update_largest", obsnorm_update_args_error(&a, 8, INT32_MAX));
  }
  const int counts[] = {0, -1, INT32_MIN};
  for (int n : counts) {
    sit_obsnorm_args a = g;
    a.max_new = n;
    show("max_new_not_positive", obsnorm_update_args_error(&a, 4, reserved));
    show("max_new_not_positive", obsnorm_reserve_args_error(n));
    a = g; a.capacity = n;
    show("capacity_not_positive", obsnorm_update_args_error(&a, 4, reserved));
  }
#define NULLED(field)                                                   \
  do {                                                                  \
    sit_obsnorm_args a = g;                                             \
    a.field = nullptr;                                                  \
    show("update_null_" #field, obsnorm_update_args_error(&a, 4, reserved)); \
  } while (0)
  NULLED(ring); NULLED(cursor); NULLED(block); NULLED(affine);
  {
    sit_obsnorm_args a = g;
    a.ring = bytes + 2048 + 8;                  // 8-byte aligned: not 4 float32, not 4 float64
    show("update_misaligned_ring", obsnorm_update_args_error(&a, 4, reserved));
    a.ring = bytes + 2048 + 16;                 // 4 float32, but not 4 float64
    show("update_misaligned_ring", obsnorm_update_args_error(&a, 8, reserved));
    a = g; a.cursor = reinterpret_cast<const int64_t*>(bytes + 12);
    show("update_misaligned_cursor", obsnorm_update_args_error(&a, 4, reserved));
    a = g; a.block = reinterpret_cast<double*>(bytes + 68);
    show("update_misaligned_block", obsnorm_update_args_error(&a, 4, reserved));
    a = g; a.affine = affine + 2;
    show("update_misaligned_affine", obsnorm_update_args_error(&a, 4, reserved));
  }

  void* rows_a = bytes + 2048;
  void* rows_b = bytes + 3072;
  show("apply_good_f32", obsnorm_apply_args_error(affine, rows_a, rows_b, 64, 4));
  show("apply_good_f64", obsnorm_apply_args_error(affine, rows_a, rows_b, 64, 8));
  show("apply_one_array", obsnorm_apply_args_error(affine, rows_a, nullptr, 1, 4));
  show("apply_largest", obsnorm_apply_args_error(affine, rows_a, rows_b, (int64_t)1 << 30, 8));
  show("apply_rows_too_many", obsnorm_apply_args_error(affine, rows_a, rows_b, ((int64_t)1 << 30) + 1, 8));
  show("apply_null_affine", obsnorm_apply_args_error(nullptr, rows_a, rows_b, 64, 4));
  show("apply_null_rows_a", obsnorm_apply_args_error(affine, nullptr, rows_b, 64, 4));
  const int64_t row_counts[] = {0, -1, INT64_MIN};
  for (int64_t n : row_counts) show("apply_rows_not_positive", obsnorm_apply_args_error(affine, rows_a, rows_b, n, 4));
  show("apply_misaligned_rows_a", obsnorm_apply_args_error(affine, bytes + 2048 + 4, rows_b, 64, 4));
  show("apply_misaligned_rows_a", obsnorm_apply_args_error(affine, bytes + 2048 + 8, rows_b, 64, 8));
  show("apply_misaligned_rows_b", obsnorm_apply_args_error(affine, rows_a, bytes + 3072 + 4, 64, 4));
  show("apply_misaligned_rows_b", obsnorm_apply_args_error(affine, rows_a, bytes + 3072 + 8, 64, 8));

  // two blocks of SIT_ACTOR_WEIGHTS floats, each rounded up to 16 bytes
  const size_t step = (block_bytes + 15) / 16 * 16;
  float* src = reinterpret_cast<float*>(bytes + 4096);
  float* dst = reinterpret_cast<float*>(bytes + 4096 + step);
  show("fold_good", obsnorm_fold_args_error(affine, src, dst));
  show("fold_adjacent", obsnorm_fold_args_error(affine, dst, src));
  show("fold_null_affine", obsnorm_fold_args_error(nullptr, src, dst));
  show("fold_null_src", obsnorm_fold_args_error(affine, nullptr, dst));
  show("fold_null_dst", obsnorm_fold_args_error(affine, src, nullptr));
  for (int off = 1; off < 4; ++off) {
    show("fold_misaligned_src", obsnorm_fold_args_error(affine, src + off, dst));
    show("fold_misaligned_dst", obsnorm_fold_args_error(affine, src, dst + off));
  }
  show("fold_overlap", obsnorm_fold_args_error(affine, src, src));
  show("fold_overlap", obsnorm_fold_args_error(affine, src, src + 4));
  show("fold_overlap", obsnorm_fold_args_error(affine, src + 4, src));
  show("fold_overlap", obsnorm_fold_args_error(affine, src, dst - 4));
  std::free(raw);
  return 0;
}
