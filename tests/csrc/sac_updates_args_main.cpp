// Stand-alone driver of the argument checks of sit_sac_updates / sit_sac_adam_scalars (csrc/sit_sac_args.h) and
// of the host copy of the clock's Adam scalars (csrc/sit_sac_clock.h), built by tests/test_sac_clock_host.py
// with -fsanitize=address,undefined.  It includes nothing but those headers (and through them include/sit.h):
// no HIP, no device.  Prints one line per case, "name: message" or "name: ok", and the scalars of a step as
// "scalars_<lr>_<beta1>_<beta2>_<t>: six float32 bit patterns in hex"; the test compares them.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sit_sac_args.h"
#include "sit_sac_clock.h"

static void show(const char* name, const char* why) { std::printf("%s: %s\n", name, why ? why : "ok"); }

static sit_sac_adam adam(double lr, double beta1, double beta2) {
  sit_sac_adam o;
  o.lr = lr; o.beta1 = beta1; o.beta2 = beta2; o.eps = 1e-8;
  o.bias1 = -7.0; o.bias2 = 0.0;          // not read by the clocked calls
  return o;
}

static void scalars(const char* tag, const sit_sac_adam& o, int64_t t) {
  const SacAdamScalars s = sac_clock_scalars(o, t);
  const float f[6] = {s.one_minus_beta1, s.beta2, s.one_minus_beta2, s.step_size, s.sqrt_bias2, s.eps};
  std::printf("scalars_%s_%" PRId64 ":", tag, t);
  for (float v : f) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof(u));
    std::printf(" %08x", u);
  }
  std::printf("\n");
}

int main() {
  // pointers are only compared and taken modulo 16, never dereferenced: one aligned heap block serves all
  void* raw = nullptr;
  if (posix_memalign(&raw, 64, 1024)) return 2;
  float* base = static_cast<float*>(raw);

  sit_sac_updates_args g;
  std::memset(&g, 0, sizeof(g));
  g.mode = SIT_SAC_UPDATES_PLAIN;
  g.batch = 64; g.n_updates = 8; g.tune = 1;
  g.target_update_interval = 1;
  g.workspace_floats = sac_workspace_floats(64);
  g.results_capacity = 1024;
  g.gamma = 0.99; g.reward_scale = 1.0; g.target_entropy = -1.0; g.tau = 0.005;
  g.critic_adam = g.actor_adam = g.alpha_adam = adam(3e-4, 0.9, 0.999);
  g.critic_weights = base; g.critic_m = base + 4; g.critic_v = base + 8;
  g.actor_weights = base + 12; g.actor_m = base + 16; g.actor_v = base + 20; g.target_weights = base + 24;
  g.alpha = base + 1; g.log_alpha = base + 2; g.log_alpha_m = base + 3; g.log_alpha_v = base + 5;
  g.state = base + 6; g.action = base + 7; g.reward = base + 9; g.next_state = base + 10; g.mask = base + 11;
  g.y = base + 13; g.workspace = base + 14;
  g.clock = reinterpret_cast<int64_t*>(base + 32);
  g.results = base + 15;
  show("good", sac_updates_args_error(&g));
  show("null_args", sac_updates_args_error(nullptr));
  {
    sit_sac_updates_args a = g;
    a.mode = SIT_SAC_UPDATES_TILED;
    show("mode_tiled", sac_updates_args_error(&a));
    a.mode = SIT_SAC_UPDATES_WIDE;
    show("mode_wide", sac_updates_args_error(&a));
    a.mode = 3;
    show("mode_bad", sac_updates_args_error(&a));
    a.mode = -1;
    show("mode_bad", sac_updates_args_error(&a));
    a = g; a.batch = 1; a.n_updates = 1; a.results_capacity = 1; a.workspace_floats = sac_workspace_floats(1);
    show("smallest", sac_updates_args_error(&a));
    a = g; a.batch = INT32_MAX; a.n_updates = INT32_MAX; a.workspace_floats = sac_workspace_floats(INT32_MAX);
    show("largest", sac_updates_args_error(&a));
    a = g; a.tune = 0; a.log_alpha = nullptr; a.log_alpha_m = nullptr; a.log_alpha_v = nullptr;
    std::memset(&a.alpha_adam, 0, sizeof(a.alpha_adam));
    show("untuned", sac_updates_args_error(&a));
    a = g; a.workspace_floats += 1;
    show("long_workspace", sac_updates_args_error(&a));
    a = g; a.target_update_interval = 1000;
    show("interval_1000", sac_updates_args_error(&a));
  }
  const int counts[] = {0, -1, INT32_MIN};
  for (int n : counts) {
    sit_sac_updates_args a = g;
    a.batch = n;
    show("batch_not_positive", sac_updates_args_error(&a));
    a = g; a.n_updates = n;
    show("n_updates_not_positive", sac_updates_args_error(&a));
    a = g; a.results_capacity = n;
    show("results_capacity_not_positive", sac_updates_args_error(&a));
    a = g; a.target_update_interval = n;
    show("interval_not_positive", sac_updates_args_error(&a));
  }
#define NULLED(field)                                   \
  do {                                                  \
    sit_sac_updates_args a = g;                         \
    a.field = nullptr;                                  \
    show("null_" #field, sac_updates_args_error(&a));   \
  } while (0)
  NULLED(critic_weights); NULLED(critic_m); NULLED(critic_v);
  NULLED(actor_weights); NULLED(actor_m); NULLED(actor_v);
  NULLED(target_weights); NULLED(alpha);
  NULLED(log_alpha); NULLED(log_alpha_m); NULLED(log_alpha_v);
  NULLED(state); NULLED(action); NULLED(reward); NULLED(next_state); NULLED(mask);
  NULLED(y); NULLED(workspace); NULLED(clock); NULLED(results);
#define MISALIGNED(field, off)                                \
  do {                                                        \
    sit_sac_updates_args a = g;                               \
    a.field = g.field + (off);                                \
    show("misaligned_" #field, sac_updates_args_error(&a));   \
  } while (0)
  for (int off = 1; off < 4; ++off) {
    MISALIGNED(critic_weights, off); MISALIGNED(critic_m, off); MISALIGNED(critic_v, off);
    MISALIGNED(actor_weights, off); MISALIGNED(actor_m, off); MISALIGNED(actor_v, off);
    MISALIGNED(target_weights, off);
  }
  {
    sit_sac_updates_args a = g;
    a.alpha = reinterpret_cast<float*>(reinterpret_cast<char*>(base) + 2);
    show("misaligned_alpha", sac_updates_args_error(&a));
    a = g; a.log_alpha_v = reinterpret_cast<float*>(reinterpret_cast<char*>(base) + 6);
    show("misaligned_log_alpha", sac_updates_args_error(&a));
    a = g; a.clock = reinterpret_cast<int64_t*>(base + 33);
    show("misaligned_clock", sac_updates_args_error(&a));
    a = g; a.results = reinterpret_cast<float*>(reinterpret_cast<char*>(base) + 62);
    show("misaligned_results", sac_updates_args_error(&a));
    a = g; a.workspace = reinterpret_cast<float*>(reinterpret_cast<char*>(base) + 58);
    show("misaligned_workspace", sac_updates_args_error(&a));
    a = g; a.workspace_floats -= 1;
    show("short_workspace", sac_updates_args_error(&a));
    a.workspace_floats = 0;
    show("short_workspace", sac_updates_args_error(&a));
    a = g; a.critic_adam.beta1 = 1.0;
    show("critic_beta_1", sac_updates_args_error(&a));
    a = g; a.actor_adam.lr = -1.0;
    show("actor_lr_negative", sac_updates_args_error(&a));
    a = g; a.alpha_adam.eps = -1.0;
    show("alpha_eps_negative", sac_updates_args_error(&a));
  }

  const sit_sac_adam d = adam(3e-4, 0.9, 0.999);
  show("scalars_good", sac_adam_scalars_args_error(&d, 1, 4096, base));
  show("scalars_null_adam", sac_adam_scalars_args_error(nullptr, 1, 1, base));
  show("scalars_t0_0", sac_adam_scalars_args_error(&d, 0, 1, base));
  show("scalars_n_0", sac_adam_scalars_args_error(&d, 1, 0, base));
  show("scalars_null_out", sac_adam_scalars_args_error(&d, 1, 1, nullptr));

  const int64_t steps[] = {1, 2, 3, 355, 1000, 37400, 1000000, (int64_t)1 << 40};
  const sit_sac_adam other = adam(1e-3, 0.5, 0.99);
  for (int64_t t : steps) {
    scalars("default", d, t);
    scalars("other", other, t);
  }
  std::free(raw);
  return 0;
}
