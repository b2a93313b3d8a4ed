// Stand-alone driver of the argument checks of sit_sac_critic_step / sit_sac_policy_step
// (csrc/sit_sac_args.h), built by tests/test_sac_update_args_host.py with -fsanitize=address,undefined.
// It includes nothing but that header (and through it include/sit.h): no HIP, no device.  Prints one
// line per case, "name: message" or "name: ok"; the test compares them.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sit_sac_args.h"

static void show(const char* name, const char* why) { std::printf("%s: %s\n", name, why ? why : "ok"); }

static sit_sac_adam adam(int t) {
  sit_sac_adam o;
  o.lr = 3e-4; o.beta1 = 0.9; o.beta2 = 0.999; o.eps = 1e-8;
  o.bias1 = 1.0; o.bias2 = 1.0;
  for (int i = 0; i < t; ++i) { o.bias1 *= o.beta1; o.bias2 *= o.beta2; }
  o.bias1 = 1.0 - o.bias1; o.bias2 = 1.0 - o.bias2;
  return o;
}

int main() {
  // pointers are only compared and taken modulo 16, never dereferenced: one aligned heap block serves all
  void* raw = nullptr;
  if (posix_memalign(&raw, 64, 512)) return 2;
  float* base = static_cast<float*>(raw);
  std::printf("workspace_floats: %lld %lld %lld %lld %lld\n", (long long)sac_workspace_floats(-1),
              (long long)sac_workspace_floats(0), (long long)sac_workspace_floats(1), (long long)sac_workspace_floats(64),
              (long long)sac_workspace_floats(INT32_MAX));

  sit_sac_critic_step_args cg;
  std::memset(&cg, 0, sizeof(cg));
  cg.batch = 64;
  cg.workspace_floats = sac_workspace_floats(64);
  cg.adam = adam(1);
  cg.critic_weights = base; cg.critic_m = base + 4; cg.critic_v = base + 8;
  cg.state = base + 1; cg.action = base + 2; cg.y = base + 3;     // the reals need no 16-byte alignment
  cg.workspace = base + 5; cg.results = base + 6;
  show("critic_good", sac_critic_step_args_error(&cg));
  show("critic_null_args", sac_critic_step_args_error(nullptr));
  const int batches[] = {0, -1, INT32_MIN, 1, INT32_MAX};
  for (int b : batches) {
    sit_sac_critic_step_args a = cg;
    a.batch = b;
    a.workspace_floats = sac_workspace_floats(b);
    char name[40];
    std::snprintf(name, sizeof(name), "critic_batch_%d", b);
    show(name, sac_critic_step_args_error(&a));
  }
#define CRITIC_NULLED(field)                                       \
  do {                                                             \
    sit_sac_critic_step_args a = cg;                               \
    a.field = nullptr;                                             \
    show("critic_null_" #field, sac_critic_step_args_error(&a));   \
  } while (0)
  CRITIC_NULLED(critic_weights);
  CRITIC_NULLED(critic_m);
  CRITIC_NULLED(critic_v);
  CRITIC_NULLED(state);
  CRITIC_NULLED(action);
  CRITIC_NULLED(y);
  CRITIC_NULLED(workspace);
  CRITIC_NULLED(results);
  for (int off = 1; off < 4; ++off) {
    sit_sac_critic_step_args a = cg;
    a.critic_weights = base + off;
    show("critic_misaligned_weights", sac_critic_step_args_error(&a));
    a = cg; a.critic_m = base + 4 + off;
    show("critic_misaligned_m", sac_critic_step_args_error(&a));
    a = cg; a.critic_v = base + 8 + off;
    show("critic_misaligned_v", sac_critic_step_args_error(&a));
  }
  {
    sit_sac_critic_step_args a = cg;
    a.workspace_floats -= 1;
    show("critic_short_workspace", sac_critic_step_args_error(&a));
    a.workspace_floats = 0;
    show("critic_short_workspace", sac_critic_step_args_error(&a));
    a.workspace_floats = -1;
    show("critic_short_workspace", sac_critic_step_args_error(&a));
    a = cg; a.workspace_floats += 1;
    show("critic_long_workspace", sac_critic_step_args_error(&a));
    a = cg; a.adam = adam(1000);
    show("critic_step_1000", sac_critic_step_args_error(&a));
    a = cg; a.adam.bias1 = 0.0;
    show("critic_bias_0", sac_critic_step_args_error(&a));
    a = cg; a.adam.bias2 = 1.5;
    show("critic_bias_big", sac_critic_step_args_error(&a));
    a = cg; a.adam.beta1 = 1.0;
    show("critic_beta_1", sac_critic_step_args_error(&a));
    a = cg; a.adam.lr = -1.0;
    show("critic_lr_negative", sac_critic_step_args_error(&a));
  }

  sit_sac_policy_step_args pg;
  std::memset(&pg, 0, sizeof(pg));
  pg.batch = 64;
  pg.tune = 1;
  pg.workspace_floats = sac_workspace_floats(64);
  pg.target_entropy = -1.0;
  pg.adam = adam(1);
  pg.alpha_adam = adam(1);
  pg.actor_weights = base; pg.actor_m = base + 4; pg.actor_v = base + 8; pg.critic_weights = base + 12;
  pg.alpha = base + 1; pg.log_alpha = base + 2; pg.log_alpha_m = base + 3; pg.log_alpha_v = base + 5;
  pg.state = base + 6;
  pg.workspace = base + 7; pg.results = base + 9;
  show("policy_good", sac_policy_step_args_error(&pg));
  show("policy_null_args", sac_policy_step_args_error(nullptr));
  {
    sit_sac_policy_step_args a = pg;
    a.noise = base + 10;
    show("policy_with_noise", sac_policy_step_args_error(&a));
    a = pg; a.tune = 0; a.log_alpha = nullptr; a.log_alpha_m = nullptr; a.log_alpha_v = nullptr;
    std::memset(&a.alpha_adam, 0, sizeof(a.alpha_adam));
    show("policy_untuned", sac_policy_step_args_error(&a));
  }
  for (int b : batches) {
    sit_sac_policy_step_args a = pg;
    a.batch = b;
    a.workspace_floats = sac_workspace_floats(b);
    char name[40];
    std::snprintf(name, sizeof(name), "policy_batch_%d", b);
    show(name, sac_policy_step_args_error(&a));
  }
#define POLICY_NULLED(field)                                       \
  do {                                                             \
    sit_sac_policy_step_args a = pg;                               \
    a.field = nullptr;                                             \
    show("policy_null_" #field, sac_policy_step_args_error(&a));   \
  } while (0)
  POLICY_NULLED(actor_weights);
  POLICY_NULLED(actor_m);
  POLICY_NULLED(actor_v);
  POLICY_NULLED(critic_weights);
  POLICY_NULLED(alpha);
  POLICY_NULLED(log_alpha);
  POLICY_NULLED(log_alpha_m);
  POLICY_NULLED(log_alpha_v);
  POLICY_NULLED(state);
  POLICY_NULLED(workspace);
  POLICY_NULLED(results);
  for (int off = 1; off < 4; ++off) {
    sit_sac_policy_step_args a = pg;
    a.actor_weights = base + off;
    show("policy_misaligned_weights", sac_policy_step_args_error(&a));
    a = pg; a.actor_m = base + 4 + off;
    show("policy_misaligned_m", sac_policy_step_args_error(&a));
    a = pg; a.actor_v = base + 8 + off;
    show("policy_misaligned_v", sac_policy_step_args_error(&a));
    a = pg; a.critic_weights = base + 12 + off;
    show("policy_misaligned_critic", sac_policy_step_args_error(&a));
  }
  {
    sit_sac_policy_step_args a = pg;
    a.alpha = reinterpret_cast<float*>(reinterpret_cast<char*>(base) + 2);
    show("policy_misaligned_alpha", sac_policy_step_args_error(&a));
    a = pg; a.log_alpha_m = reinterpret_cast<float*>(reinterpret_cast<char*>(base) + 6);
    show("policy_misaligned_log_alpha", sac_policy_step_args_error(&a));
    a = pg; a.workspace_floats -= 1;
    show("policy_short_workspace", sac_policy_step_args_error(&a));
    a = pg; a.alpha_adam.bias1 = 0.0;
    show("policy_alpha_bias_0", sac_policy_step_args_error(&a));
    a = pg; a.adam.eps = -1.0;
    show("policy_eps_negative", sac_policy_step_args_error(&a));
  }
  std::free(raw);
  return 0;
}
