// Stand-alone driver of the argument checks of sit_score_reset / sit_score_reserve / sit_score_update /
// sit_score_keep (csrc/sit_score_args.h), built by tests/test_score_host.py with -fsanitize=address,undefined.
// It includes nothing but that header (and through it include/sit.h): no HIP, no device.  Prints one line per
// case, "name: message" or "name: ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sit_score_args.h"

static void show(const char* name, const char* why) { std::printf("%s: %s\n", name, why ? why : "ok"); }

int main() {
  // pointers are only compared and taken modulo their alignment, never dereferenced: one aligned heap block serves all
  void* raw = nullptr;
  if (posix_memalign(&raw, 64, 1024)) return 2;
  char* bytes = static_cast<char*>(raw);
  float* base = static_cast<float*>(raw);
  double* dbase = static_cast<double*>(raw);

  sit_score_args g;
  std::memset(&g, 0, sizeof(g));
  g.record_capacity = 4096;
  g.flags = 0;
  g.episode_limit = 0;
  g.records = dbase + 8;
  g.record_count = reinterpret_cast<int64_t*>(dbase + 1);
  g.score = dbase + 2;
  g.class_any[0] = 1u << 5;
  g.class_none[6] = 1u << 12;
  show("good", score_update_args_error(&g));
  show("null_args", score_update_args_error(nullptr));
  {
    sit_score_args a = g;
    a.flags = SIT_SCORE_CONSUME;
    show("flag_consume", score_update_args_error(&a));
    a.flags = SIT_SCORE_FRESH;
    show("flag_fresh", score_update_args_error(&a));
    a.flags = SIT_SCORE_CONSUME | SIT_SCORE_FRESH;
    show("flag_both", score_update_args_error(&a));
    a.flags = 4u;
    show("flags_unknown", score_update_args_error(&a));
    a.flags = 0x80000001u;
    show("flags_unknown", score_update_args_error(&a));
    a = g; a.record_capacity = 1;
    show("smallest", score_update_args_error(&a));
    a = g; a.record_capacity = INT32_MAX; a.episode_limit = INT64_MAX;
    show("largest", score_update_args_error(&a));
    a = g; a.episode_limit = 2;
    show("limit_2", score_update_args_error(&a));
    a = g; a.episode_limit = -1;
    show("limit_negative", score_update_args_error(&a));
    a = g; a.episode_limit = INT64_MIN;
    show("limit_negative", score_update_args_error(&a));
    a = g; std::memset(a.class_any, 0xff, sizeof(a.class_any)); std::memset(a.class_none, 0xff, sizeof(a.class_none));
    show("all_class_bits", score_update_args_error(&a));
  }
  const int counts[] = {0, -1, INT32_MIN};
  for (int n : counts) {
    sit_score_args a = g;
    a.record_capacity = n;
    show("capacity_not_positive", score_update_args_error(&a));
    show("max_records_not_positive", score_reserve_args_error(n));
  }
  show("reserve_good", score_reserve_args_error(1));
  show("reserve_good", score_reserve_args_error(INT32_MAX));
#define NULLED(field)                                  \
  do {                                                 \
    sit_score_args a = g;                              \
    a.field = nullptr;                                 \
    show("null_" #field, score_update_args_error(&a)); \
  } while (0)
  NULLED(records); NULLED(record_count); NULLED(score);
  for (int off = 1; off < 8; ++off) {
    sit_score_args a = g;
    a.records = reinterpret_cast<const double*>(bytes + 64 + off);
    show("misaligned_records", score_update_args_error(&a));
    a = g; a.record_count = reinterpret_cast<int64_t*>(bytes + 8 + off);
    show("misaligned_record_count", score_update_args_error(&a));
    a = g; a.score = reinterpret_cast<double*>(bytes + 16 + off);
    show("misaligned_score", score_update_args_error(&a));
    show("reset_misaligned_score", score_block_error(reinterpret_cast<double*>(bytes + 16 + off)));
  }
  show("reset_good", score_block_error(dbase));
  show("reset_null_score", score_block_error(nullptr));

  sit_score_keep_args k;
  std::memset(&k, 0, sizeof(k));
  k.n_blocks = 4;
  for (int i = 0; i < 4; ++i) {
    k.src[i] = base + 16 + 8 * i;
    k.dst[i] = base + 20 + 8 * i;
    k.floats[i] = i + 1;
  }
  k.score = dbase;
  k.stamp = reinterpret_cast<const int64_t*>(dbase + 1);
  show("keep_good", score_keep_args_error(&k));
  show("keep_null_args", score_keep_args_error(nullptr));
  {
    sit_score_keep_args a = k;
    a.stamp = nullptr;
    show("keep_no_stamp", score_keep_args_error(&a));
    a = k; a.n_blocks = 0;
    show("keep_no_blocks", score_keep_args_error(&a));
    a = k; a.n_blocks = 1; a.src[1] = nullptr; a.dst[2] = nullptr; a.floats[3] = 0;   // unused slots are not read
    show("keep_one_block", score_keep_args_error(&a));
    a = k; a.floats[0] = (int64_t)1 << 34;
    show("keep_largest", score_keep_args_error(&a));
    a = k; a.floats[0] = ((int64_t)1 << 34) + 1;
    show("keep_floats_too_many", score_keep_args_error(&a));
    a = k; a.n_blocks = 5;
    show("keep_n_blocks_outside", score_keep_args_error(&a));
    a = k; a.n_blocks = -1;
    show("keep_n_blocks_outside", score_keep_args_error(&a));
    a = k; a.n_blocks = INT32_MIN;
    show("keep_n_blocks_outside", score_keep_args_error(&a));
    a = k; a.score = nullptr;
    show("keep_null_score", score_keep_args_error(&a));
    a = k; a.score = reinterpret_cast<double*>(bytes + 4);
    show("keep_misaligned_score", score_keep_args_error(&a));
    a = k; a.stamp = reinterpret_cast<const int64_t*>(bytes + 12);
    show("keep_misaligned_stamp", score_keep_args_error(&a));
  }
  for (int i = 0; i < 4; ++i) {
    sit_score_keep_args a = k;
    a.src[i] = nullptr;
    show("keep_null_src", score_keep_args_error(&a));
    a = k; a.dst[i] = nullptr;
    show("keep_null_dst", score_keep_args_error(&a));
    a = k; a.floats[i] = 0;
    show("keep_floats_not_positive", score_keep_args_error(&a));
    a = k; a.floats[i] = -3;
    show("keep_floats_not_positive", score_keep_args_error(&a));
    for (int off = 1; off < 4; ++off) {
      a = k; a.src[i] = k.src[i] + off;
      show("keep_misaligned_src", score_keep_args_error(&a));
      a = k; a.dst[i] = k.dst[i] + off;
      show("keep_misaligned_dst", score_keep_args_error(&a));
    }
  }
  std::free(raw);
  return 0;
}
