// Stand-alone driver of the SAC calls' argument checks (csrc/sit_sac_args.h), built by
// tests/test_sac_args_host.py with -fsanitize=address,undefined.  It includes nothing but that header
// (and through it include/sit.h): no HIP, no device.  Prints one line per case, "name: message" or
// "name: ok"; the test compares them.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sit_sac_args.h"

static void show(const char* name, const char* why) { std::printf("%s: %s\n", name, why ? why : "ok"); }

int main() {
  // pointers are only compared and taken modulo 16, never dereferenced: one aligned heap block serves all
  void* raw = nullptr;
  if (posix_memalign(&raw, 64, 256)) return 2;
  float* base = static_cast<float*>(raw);
  sit_sac_target_args good;
  std::memset(&good, 0, sizeof(good));
  good.batch = 64;
  good.gamma = 0.99;
  good.reward_scale = 1.0;
  good.actor_weights = base;
  good.critic_weights = base + 4;
  good.alpha = base + 9;
  good.next_state = base + 1;    // the reals need no 16-byte alignment
  good.reward = base + 2;
  good.mask = base + 3;
  good.y = base + 5;
  show("good", sac_target_args_error(&good));
  show("null_args", sac_target_args_error(nullptr));
  {
    sit_sac_target_args a = good;
    a.noise = base + 6; a.next_action = base + 7; a.next_logp = base + 8; a.q1 = base + 10; a.q2 = base + 11;
    show("with_optionals", sac_target_args_error(&a));
  }
  const int batches[] = {0, -1, INT32_MIN, 1, INT32_MAX};
  for (int b : batches) {
    sit_sac_target_args a = good;
    a.batch = b;
    char name[32];
    std::snprintf(name, sizeof(name), "batch_%d", b);
    show(name, sac_target_args_error(&a));
  }
#define NULLED(field)                          \
  do {                                         \
    sit_sac_target_args a = good;              \
    a.field = nullptr;                         \
    show("null_" #field, sac_target_args_error(&a)); \
  } while (0)
  NULLED(actor_weights);
  NULLED(critic_weights);
  NULLED(alpha);
  NULLED(next_state);
  NULLED(reward);
  NULLED(mask);
  NULLED(y);
  for (int off = 1; off < 4; ++off) {
    sit_sac_target_args a = good;
    a.actor_weights = base + off;
    show("misaligned_actor", sac_target_args_error(&a));
    a = good;
    a.critic_weights = base + 4 + off;
    show("misaligned_critic", sac_target_args_error(&a));
  }
  {
    sit_sac_target_args a = good;
    a.alpha = reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + 2);
    show("misaligned_alpha", sac_target_args_error(&a));
  }
  show("polyak_good", sac_polyak_args_error(base, base + 8, 1));
  show("polyak_big", sac_polyak_args_error(base, base + 8, (int64_t)1 << 34));
  show("polyak_null_target", sac_polyak_args_error(nullptr, base, 4));
  show("polyak_null_online", sac_polyak_args_error(base, nullptr, 4));
  show("polyak_n_0", sac_polyak_args_error(base, base + 8, 0));
  show("polyak_n_negative", sac_polyak_args_error(base, base + 8, INT64_MIN));
  show("polyak_n_too_big", sac_polyak_args_error(base, base + 8, ((int64_t)1 << 34) + 1));
  show("polyak_n_max", sac_polyak_args_error(base, base + 8, INT64_MAX));
  show("polyak_misaligned_target", sac_polyak_args_error(base + 1, base + 8, 4));
  show("polyak_misaligned_online", sac_polyak_args_error(base, base + 9, 4));
  std::free(raw);
  return 0;
}
