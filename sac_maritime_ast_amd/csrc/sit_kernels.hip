// sit_kernels.hip — C ABI of the ship-in-transit env step (include/sit.h) on MI355X (gfx950).
// Kernels: sit_impl.h.  Handle, layouts, constants and launchers: sit_host.h.  The map image:
// sit_map_build.h.  float32 step kernels: sit_steps_f32.hip.

#include "sit_host.h"
#include "sit_map_build.h"
#include "sit_actor.h"
#include "sit_episodes.h"
#include "sit_score.h"
#include "sit_obsnorm.h"
#include "sit_replay.h"
#include "sit_sac.h"
#include "sit_sac_grad.h"
#include "sit_sac_wgrad.h"
#include "sit_sac_rows.h"

#ifdef SIT_F32_TU
int sit_launch_steps_f32(sit_handle* h, const void* io, void* stream);   // sit_steps_f32.hip
int sit_launch_probe_f32(sit_handle* h, int n, const void* pts_ne, void* dist, uint8_t* inside, uint8_t* hull,
                         void* stream);
int sit_launch_selftest_f32tu(int op, int n, const double* a, const double* b, double* out, void* stream);
int sit_role_fallbacks_f32tu(unsigned long long* out, int reset);
#ifdef SIT_DEBUG
int sit_debug_flags_f32tu(uint32_t* out);
#endif
#endif

namespace {

// The step and probe launches by real type (the probe's by a tag; its arrays are untyped).  float64
// runs in this translation unit; float32 goes to the fast-math unit in the two-unit build and is
// compiled here, strict, in single-unit (diagnostic) builds.  The generic code under with_real
// calls steps / probe and stays oblivious to the split.
int steps(sit_handle* h, const StepIO<double>& io, void* stream) {
  return launch_steps<double>(h, io, (hipStream_t)stream);
}
int probe(sit_handle* h, double, int n, const void* pts, void* dist, uint8_t* inside, uint8_t* hull, void* stream) {
  return launch_probe<double>(h, n, pts, dist, inside, hull, (hipStream_t)stream);
}
#ifdef SIT_F32_TU
int steps(sit_handle* h, const StepIO<float>& io, void* stream) { return sit_launch_steps_f32(h, &io, stream); }
int probe(sit_handle* h, float, int n, const void* pts, void* dist, uint8_t* inside, uint8_t* hull, void* stream) {
  return sit_launch_probe_f32(h, n, pts, dist, inside, hull, stream);
}
int launch_selftest_f32tu(int op, int n, const double* a, const double* b, double* out, void* stream) {
  return sit_launch_selftest_f32tu(op, n, a, b, out, stream);
}
#else
int steps(sit_handle* h, const StepIO<float>& io, void* stream) {
  return launch_steps<float>(h, io, (hipStream_t)stream);
}
int probe(sit_handle* h, float, int n, const void* pts, void* dist, uint8_t* inside, uint8_t* hull, void* stream) {
  return launch_probe<float>(h, n, pts, dist, inside, hull, (hipStream_t)stream);
}
int launch_selftest_f32tu(int op, int n, const double* a, const double* b, double* out, void* stream) {
  return launch_selftest(op, n, a, b, out, (hipStream_t)stream);
}
#endif

// n doubles as the handle's reals (real_size 8: copied, 4: rounded to float)
std::vector<unsigned char> to_real(const double* src, size_t n, size_t real_size) {
  std::vector<unsigned char> out(n * real_size);
  for (size_t i = 0; i < n; ++i) {
    if (real_size == 8) reinterpret_cast<double*>(out.data())[i] = src[i];
    else reinterpret_cast<float*>(out.data())[i] = (float)src[i];
  }
  return out;
}

// sit_step / sit_step_host: one step on explicit actions
template <typename T>
StepIO<T> single_step_io(const void* action_ne, const uint8_t* sac_update, const uint8_t* init, void* next_state,
                         void* reward, uint8_t* done, uint32_t* status) {
  StepIO<T> io{};
  io.n_steps = 1; io.action_ne = (const T*)action_ne; io.sac_update = sac_update; io.init = init;
  io.next_state = (T*)next_state; io.reward = (T*)reward; io.done = done; io.status = status;
  return io;
}

}  // namespace

// =======================================================================================
// C ABI
// =======================================================================================
extern "C" {

#if defined(SIT_DIAG_PATHS) || defined(SIT_DIAG_PHASES) || defined(SIT_DIAG_SYNC) || defined(SIT_DIAG_SERVE)
#ifdef SIT_DIAG_PHASES
int sit_diag_read_waves(unsigned long long* out, int n) {   // [n][4], diagnostic builds only
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (n > kDiagWaves) n = kDiagWaves;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sit_wave), sizeof(unsigned long long) * 4 * n) != hipSuccess) return -1;
  return 0;
}
#endif
int sit_diag_read(unsigned long long* out, int reset) { return diag_read_impl(out, reset); }   // diagnostic builds only
#endif

int sit_probe_map(sit_handle* h, int32_t n, const void* pts_ne, void* dist, uint8_t* inside, uint8_t* hull,
                  void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (!h->have_map) return fail(h, SIT_E_STATE, "sit_load_map has not been called");
  if (n < 0 || (n > 0 && !pts_ne)) return fail(h, SIT_E_INVALID, "need n >= 0 points");
  if (n == 0) return SIT_OK;
  return with_real(h, [&](auto t) { return probe(h, t, n, pts_ne, dist, inside, hull, stream); });
}

int sit_selftest_f64(int32_t op, int32_t n, const double* a, const double* b, double* out, int32_t fast_tu,
                     void* stream) {
  if (op < 0 || op > 12 || n < 0 || (n > 0 && (!a || !b || !out))) return SIT_E_INVALID;
  if (n == 0) return SIT_OK;
  return fast_tu ? launch_selftest_f32tu(op, n, a, b, out, stream)
                 : launch_selftest(op, n, a, b, out, (hipStream_t)stream);
}

int sit_policy_apply(sit_handle* h, int32_t capacity, const void* head, int32_t head_stride, const void* noise,
                     const int32_t* request_env, const int32_t* request_count, int32_t deterministic,
                     void* policy_action, int32_t* policy_ready, int64_t* served, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (capacity <= 0 || !head || head_stride < 2 || !request_env || !request_count || !policy_action ||
      !policy_ready || (!deterministic && !noise))
    return fail(h, SIT_E_INVALID, "policy_apply: bad arguments");
  const int blocks = (capacity + 255) / 256;
  with_real(h, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_policy_apply<T>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, capacity,
                       (const T*)head, head_stride, (const T*)noise, request_env, request_count,
                       deterministic, (T*)policy_action, policy_ready, (unsigned long long*)served, h->n_env);
  });
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
}

int sit_policy_actor(sit_handle* h, int32_t capacity, const float* weights, const void* obs, const void* noise,
                     const int32_t* request_env, const int32_t* request_count, int32_t deterministic,
                     void* policy_action, int32_t* policy_ready, int64_t* served, int32_t* clear_count,
                     void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (capacity <= 0 || !weights || !obs || !request_env || !request_count || !policy_action || !policy_ready ||
      (!deterministic && !noise))
    return fail(h, SIT_E_INVALID, "policy_actor: bad arguments");
  int rc = with_real(h, [&](auto t) {
    return launch_policy_actor<decltype(t)>(h, capacity, weights, obs, noise, request_env, request_count,
                                            deterministic, policy_action, policy_ready, served, clear_count,
                                            (hipStream_t)stream);
  });
  if (rc) return rc;
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
}

int sit_map_info(const sit_handle* h, int64_t* info, int32_t n) {
  if (!h || !info || n < 0) return SIT_E_INVALID;
  if (!h->have_map) return SIT_E_STATE;
  const MapMeta& m = h->meta;
  const int64_t v[6] = {(int64_t)m.map_bytes, m.n_mixed, m.n_live, m.use_index, m.use_cells,
                        (int64_t)map_lds_bytes(h)};
  for (int i = 0; i < n && i < 6; ++i) info[i] = v[i];
  return SIT_OK;
}

int32_t sit_abi_version(void) { return SIT_ABI_VERSION; }

#ifdef SIT_DEBUG
int32_t sit_debug_build(void) { return 1; }
#else
int32_t sit_debug_build(void) { return 0; }
#endif

int sit_debug_flags(uint32_t* flags) {
  if (!flags) return SIT_E_INVALID;
  *flags = 0;
#ifdef SIT_DEBUG
  int rc = debug_flags_impl(flags);
#ifdef SIT_F32_TU
  if (rc == SIT_OK) rc = sit_debug_flags_f32tu(flags);
#endif
  return rc;
#else
  return SIT_OK;
#endif
}
int sit_role_fallbacks(uint64_t* count, int32_t reset) {
  if (!count) return SIT_E_INVALID;
  unsigned long long v = 0;
  int rc = role_fallbacks_impl(&v, reset);
#ifdef SIT_F32_TU
  if (rc == SIT_OK) rc = sit_role_fallbacks_f32tu(&v, reset);
#endif
  *count = v;
  return rc;
}
size_t sit_rollout_args_size(void) { return sizeof(sit_rollout_args); }
size_t sit_params_size(void) { return sizeof(sit_params); }

void sit_params_default(sit_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  // test_beds/test_policy.py:102-124
  p->dead_weight_tonnage = 3850000;
  p->coefficient_of_deadweight_to_displacement = 0.7;
  p->bunkers = 200000;
  p->ballast = 200000;
  p->length_of_ship = 80;
  p->width_of_ship = 16;
  p->added_mass_coefficient_in_surge = 0.4;
  p->added_mass_coefficient_in_sway = 0.4;
  p->added_mass_coefficient_in_yaw = 0.4;
  p->mass_over_linear_friction_coefficient_in_surge = 130;
  p->mass_over_linear_friction_coefficient_in_sway = 18;
  p->mass_over_linear_friction_coefficient_in_yaw = 90;
  p->nonlinear_friction_coefficient_in_surge = 2400;
  p->nonlinear_friction_coefficient_in_sway = 4000;
  p->nonlinear_friction_coefficient_in_yaw = 400;
  p->current_velocity_component_from_north = -2;
  p->current_velocity_component_from_east = -2;
  p->wind_speed = 2;
  p->wind_direction = -M_PI / 4;
  // ship_model.py:123-130
  p->rho_air = 1.2; p->front_height = 8.0; p->side_height = 8.0;
  p->cx = 0.5; p->cy = 0.7; p->cn = 0.08;
  p->integration_step = 0.5;
  // test_policy.py:132-168 (PTI mode)
  p->hotel_load = 200000;
  p->main_engine_capacity = 0;
  p->electrical_capacity = 2 * 510e3;
  p->shaft_generator_state = SIT_SG_MOTOR;
  p->rated_speed_main_engine_rpm = 1000;
  p->linear_friction_main_engine = 68;
  p->linear_friction_hybrid_shaft_generator = 57;
  p->gear_ratio_between_main_engine_and_propeller = 0.6;
  p->gear_ratio_between_hybrid_shaft_generator_and_propeller = 0.6;
  p->propeller_inertia = 6000;
  p->propeller_speed_to_torque_coefficient = 7.5;
  p->propeller_diameter = 3.1;
  p->propeller_speed_to_thrust_force_coefficient = 1.7;
  p->rudder_angle_to_sway_force_coefficient = 50e3;
  p->rudder_angle_to_yaw_force_coefficient = 500e3;
  p->max_rudder_angle_degrees = 30;
  // test_policy.py:199-217
  p->kp_ship_speed = 7; p->ki_ship_speed = 0.13; p->kp_shaft_speed = 0.05; p->ki_shaft_speed = 0.005;
  p->heading_kp = 1; p->heading_kd = 90; p->heading_ki = 0.01;
  p->radius_of_acceptance = 300; p->lookahead_distance = 1000;
  p->los_integral_gain = 0.002; p->integrator_windup_limit = 4000;
  // test_policy.py:39-42; MSRL_env_ex.py:119, 557, 592, 754; MSRL_Env.py:246-250
  p->theta = 2; p->sampling_frequency = 7; p->collision_bias = 1;
  p->e_tolerance = 1000; p->arrival_radius = 200; p->shaft_rpm_max = 2000; p->minimum_ship_distance = 50;
  p->bias_throttle_scale = 0.5; p->bias_throttle_max = 1.1; p->bias_rudder_degrees = 3;
  // SpecificFuelConsumptionWartila6L26 / Baudouin6M26Dot3 (ship_engine.py:89-115), test_policy.py:162-163
  p->fuel_me_a = 128.9; p->fuel_me_b = -168.9; p->fuel_me_c = 246.8;
  p->fuel_dg_a = 108.7; p->fuel_dg_b = -289.9; p->fuel_dg_c = 324.9;
  // SIT_MACH_SIMPLIFIED only: the reference configures no SimplifiedMachineryModel (no value to
  // quote); 30 s is this library's default
  p->machinery_model = SIT_MACH_SHAFT;
  p->thrust_force_dynamic_time_constant = 30;
}

const char* sit_last_error(const sit_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }
int32_t sit_precision(const sit_handle* h) { return h ? h->precision : 0; }
int32_t sit_n_env(const sit_handle* h) { return h ? h->n_env : 0; }
const char* sit_step_kernel(const sit_handle* h) { return h ? h->last_kernel : ""; }
int32_t sit_state_nfields(void) { return kNumFields; }

int sit_create(const sit_params* p, int32_t n_env, int32_t wpt_capacity, int32_t precision, sit_handle** out) {
  if (!p || !out) return fail(nullptr, SIT_E_INVALID, "null argument");
  *out = nullptr;
  if (n_env <= 0) return fail(nullptr, SIT_E_INVALID, "n_env must be positive (got %d)", n_env);
  if (wpt_capacity < 2 || wpt_capacity > 1024)
    return fail(nullptr, SIT_E_INVALID, "wpt_capacity must be in [2, 1024] (got %d)", wpt_capacity);
  if (precision != SIT_F32 && precision != SIT_F64)
    return fail(nullptr, SIT_E_INVALID, "precision must be SIT_F32 or SIT_F64 (got %d)", precision);
  if (p->integration_step <= 0 || p->sampling_frequency <= 0 || p->lookahead_distance <= 0)
    return fail(nullptr, SIT_E_INVALID, "integration_step, sampling_frequency and lookahead_distance must be positive");
  if (p->shaft_generator_state < SIT_SG_MOTOR || p->shaft_generator_state > SIT_SG_OFF)
    return fail(nullptr, SIT_E_INVALID, "shaft_generator_state out of range");
  if (p->machinery_model != SIT_MACH_SHAFT && p->machinery_model != SIT_MACH_SIMPLIFIED)
    return fail(nullptr, SIT_E_INVALID, "machinery_model out of range");
  if (p->machinery_model == SIT_MACH_SIMPLIFIED && !(p->thrust_force_dynamic_time_constant > 0))
    return fail(nullptr, SIT_E_INVALID, "thrust_force_dynamic_time_constant must be > 0");
  sit_handle* h = new sit_handle();
  h->precision = precision;
  h->n_env = n_env;
  h->cap = wpt_capacity;
  h->p = *p;
  // diagnostic kernel selection (read once; the launch path reads no environment)
  if (const char* sel = getenv("SIT_STEP_KERNEL")) h->kernel_classic = strcmp(sel, "classic") == 0;
  if (const char* lm = getenv("SIT_LDS_MAP")) h->lds_map_sel = (lm[0] == '0') ? 0 : (lm[0] == '1') ? 1 : -1;
  // test hook (tests/test_gpu_placement.py): the fused step kernel's waves report SIMD digit w of this
  // base-4 assignment (XOR the block index's low bits) instead of HW_ID, so shared-SIMD placements run
  if (const char* fs = getenv("SIT_TEST_FAKE_SIMDS")) h->fake_simds = 0x100 | (atoi(fs) & 0xFF);
  hipError_t e = setup_device(&h->device);
  if (e != hipSuccess) { fail(nullptr, SIT_E_HIP, "hipGetDevice: %s", hipGetErrorString(e)); delete h; return SIT_E_HIP; }
  layout_state(h);
  layout_scen(h);
  if (setup_alloc(&h->blob, h->blob_bytes) != hipSuccess || setup_alloc(&h->scen, h->scen_bytes) != hipSuccess) {
    fail(nullptr, SIT_E_NOMEM, "hipMalloc of %zu + %zu bytes failed", h->blob_bytes, h->scen_bytes);
    sit_destroy(h);
    return SIT_E_NOMEM;
  }
  if (setup_zero(h->blob, h->blob_bytes) != hipSuccess || setup_zero(h->scen, h->scen_bytes) != hipSuccess) {
    fail(nullptr, SIT_E_HIP, "hipMemset failed");
    sit_destroy(h);
    return SIT_E_HIP;
  }
  *out = h;
  return SIT_OK;
}

void sit_destroy(sit_handle* h) {
  if (!h) return;
  if (h->blob) (void)setup_free(h->blob);
  if (h->scen) (void)setup_free(h->scen);
  if (h->map) (void)setup_free(h->map);
  if (h->episodes) (void)setup_free(h->episodes);
  if (h->replay) (void)setup_free(h->replay);
  if (h->score) (void)setup_free(h->score);
  if (h->obsnorm) (void)setup_free(h->obsnorm);
#ifndef SIT_HOST_MEMORY_TEST
  if (h->stage) (void)hipHostFree(h->stage);
#endif
  delete h;
}

int sit_load_map(sit_handle* h, int32_t n_poly, const int32_t* vert_offsets, const double* verts_en) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (n_poly <= 0 || n_poly > kMaxPolys || !vert_offsets || !verts_en)
    return fail(h, SIT_E_INVALID, "need 1..%d polygons with offsets and vertices", kMaxPolys);
  if (vert_offsets[0] != 0) return fail(h, SIT_E_INVALID, "vert_offsets[0] must be 0");
  for (int p = 0; p < n_poly; ++p)
    if (vert_offsets[p + 1] - vert_offsets[p] < 3) return fail(h, SIT_E_INVALID, "polygon %d has < 3 vertices", p);
  const int nv = vert_offsets[n_poly];
  if (nv > kMaxPolyVerts) return fail(h, SIT_E_INVALID, "at most %d vertices (got %d)", kMaxPolyVerts, nv);
  const MapImage img = build_map_image(n_poly, vert_offsets, verts_en, real_size(h));
  if (h->map) { (void)setup_free(h->map); h->map = nullptr; }
  HIP_TRY(h, setup_alloc(&h->map, img.bytes.size()));
  HIP_TRY(h, setup_upload(h->map, img.bytes.data(), img.bytes.size()));
  h->meta = img.meta;
  h->have_map = true;
  // the cached IW tests describe the previous map
  HIP_TRY(h, setup_zero(h->blob + h->off[F_IWK_FLAGS], (size_t)h->n_env * 4));
  return SIT_OK;
}

int sit_load_routes(sit_handle* h, const double* wpt_ne, const int32_t* n_wpt) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (!wpt_ne || !n_wpt) return fail(h, SIT_E_INVALID, "null route arrays");
  const int n = h->n_env, cap = h->cap;
  const size_t rs = real_size(h);
  std::vector<double> tab((size_t)2 * 2 * cap * n, 0.0), end((size_t)2 * 2 * n), ab_len(n), ab_alpha(n);
  std::vector<int32_t> nw0((size_t)2 * n);
  for (int e = 0; e < n; ++e) {
    for (int t = 0; t < 2; ++t) {
      const int nw = n_wpt[2 * e + t];
      if (nw < 2 || nw > cap) return fail(h, SIT_E_INVALID, "env %d ship %d: n_wpt %d not in [2, %d]", e, t, nw, cap);
      const double* r = wpt_ne + ((size_t)(e * 2 + t) * cap) * 2;
      for (int i = 0; i < nw - 1; ++i) {
        tab[((size_t)(0 * 2 + t) * cap + i) * n + e] = r[2 * i];
        tab[((size_t)(1 * 2 + t) * cap + i) * n + e] = r[2 * i + 1];
      }
      end[(size_t)(0 * 2 + t) * n + e] = r[2 * (nw - 1)];
      end[(size_t)(1 * 2 + t) * n + e] = r[2 * (nw - 1) + 1];
      nw0[(size_t)t * n + e] = nw;
      if (t == 1) {   // reward_function_params (MSRL_Env.py:119-128)
        const double dn = r[2 * (nw - 1)] - r[0], de = r[2 * (nw - 1) + 1] - r[1];
        ab_len[e] = std::sqrt(dn * dn + de * de) / h->p.sampling_frequency;
        ab_alpha[e] = std::atan2(de, dn);
      }
    }
  }
  const size_t tcnt = (size_t)2 * cap * n;
  auto tn = to_real(tab.data(), tcnt, rs), te = to_real(tab.data() + tcnt, tcnt, rs);
  auto en = to_real(end.data(), (size_t)2 * n, rs), ee = to_real(end.data() + (size_t)2 * n, (size_t)2 * n, rs);
  HIP_TRY(h, setup_upload(h->blob + h->off[F_WN], tn.data(), tn.size()));
  HIP_TRY(h, setup_upload(h->blob + h->off[F_WE], te.data(), te.size()));
  HIP_TRY(h, setup_upload(h->scen + h->scen_end_n, en.data(), en.size()));
  HIP_TRY(h, setup_upload(h->scen + h->scen_end_e, ee.data(), ee.size()));
  HIP_TRY(h, setup_upload(h->scen + h->scen_nw0, nw0.data(), nw0.size() * 4));
  HIP_TRY(h, setup_upload(h->scen + h->scen_ab_len, ab_len.data(), (size_t)n * 8));
  HIP_TRY(h, setup_upload(h->scen + h->scen_ab_alpha, ab_alpha.data(), (size_t)n * 8));
  h->have_routes = true;
  return SIT_OK;
}

int sit_load_initial(sit_handle* h, const double* init) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (!init) return fail(h, SIT_E_INVALID, "null init array");
  const int n = h->n_env;
  const size_t rs = real_size(h);
  std::vector<double> sc((size_t)2 * SIT_INIT_NF * n), ist((size_t)n * SIT_OBS_DIM, 0.0);
  for (int e = 0; e < n; ++e)
    for (int t = 0; t < 2; ++t)
      for (int f = 0; f < SIT_INIT_NF; ++f)
        sc[((size_t)t * SIT_INIT_NF + f) * n + e] = init[((size_t)e * 2 + t) * SIT_INIT_NF + f];
  // construction-time observation, rounded to float32 as the reference's array (MSRL_Env.py:88-91)
  for (int e = 0; e < n; ++e) {
    const double* a = init + (size_t)e * 2 * SIT_INIT_NF;
    const double* b = a + SIT_INIT_NF;
    double* o = &ist[(size_t)e * SIT_OBS_DIM];
    o[0] = (float)a[SIT_INIT_NORTH]; o[1] = (float)a[SIT_INIT_EAST]; o[2] = (float)a[SIT_INIT_YAW];
    o[6] = (float)b[SIT_INIT_NORTH]; o[7] = (float)b[SIT_INIT_EAST]; o[8] = (float)b[SIT_INIT_YAW];
  }
  auto a = to_real(sc.data(), sc.size(), rs), b = to_real(ist.data(), ist.size(), rs);
  HIP_TRY(h, setup_upload(h->scen + h->scen_init, a.data(), a.size()));
  if (rs == 4) {   // float32: the low parts of the initial values (double-float starts, comp_add)
    std::vector<float> lo(sc.size());
    for (size_t i = 0; i < sc.size(); ++i) lo[i] = (float)(sc[i] - (double)(float)sc[i]);
    HIP_TRY(h, setup_upload(h->scen + h->scen_init_lo, lo.data(), lo.size() * 4));
  }
  HIP_TRY(h, setup_upload(h->scen + h->scen_initial, b.data(), b.size()));
  h->have_init = true;
  return SIT_OK;
}

int sit_restart(sit_handle* h, void* stream) {
  int rc = ready(h);
  if (rc) return rc;
  const int blocks = (h->n_env + 255) / 256;
  with_real(h, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_restart<T>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, make_args<T>(h));
  });
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
}

int sit_reset(sit_handle* h, const uint8_t* env_mask, void* initial_state, void* stream) {
  int rc = ready(h);
  if (rc) return rc;
  const int blocks = (h->n_env + 255) / 256;
  with_real(h, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_reset<T>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, make_args<T>(h), env_mask,
                       (T*)initial_state);
  });
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
}

int sit_init_step(sit_handle* h, const uint8_t* env_mask, void* stream) {
  int rc = ready(h);
  if (rc) return rc;
  const int blocks = (2 * h->n_env + 255) / 256;
  with_real(h, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_init_step<T>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, make_args<T>(h), env_mask);
  });
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
}

// next_state and action_out rows are written with paired stores (store2)
static bool pair_aligned(const sit_handle* h, const void* p) {
  return reinterpret_cast<uintptr_t>(p) % (2 * real_size(h)) == 0;
}

int sit_step(sit_handle* h, const void* action_ne, const uint8_t* sac_update, const uint8_t* init,
             void* next_state, void* reward, uint8_t* done, uint32_t* status, int32_t* done_count,
             void* stream) {
  int rc = ready(h);
  if (rc) return rc;
  if (!action_ne || !sac_update || !init) return fail(h, SIT_E_INVALID, "action_ne, sac_update and init are required");
  if (!next_state && !reward) return fail(h, SIT_E_INVALID, "need next_state or reward output");
  if (!pair_aligned(h, next_state)) return fail(h, SIT_E_INVALID, "next_state must be aligned to 2 reals");
  return with_real(h, [&](auto t) {
    auto io = single_step_io<decltype(t)>(action_ne, sac_update, init, next_state, reward, done, status);
    io.done_count = done_count;
    return steps(h, io, stream);
  });
}

// sit_step_host's staging: pinned, coherent host memory mapped for the device (the step kernel reads
// the inputs and writes the outputs there directly; no copy call per step)
struct StageLayout {
  size_t act, sac, init, ns, rw, dn, st, log, blob, bytes;
};
static StageLayout stage_layout(const sit_handle* h) {
  const size_t n = (size_t)h->n_env, rs = real_size(h);
  StageLayout L{};
  size_t o = 0;
  L.act = o; o = align256(o + 2 * n * rs);
  L.sac = o; o = align256(o + n);
  L.init = o; o = align256(o + n);
  L.ns = o; o = align256(o + (size_t)SIT_OBS_DIM * n * rs);
  L.rw = o; o = align256(o + n * rs);
  L.dn = o; o = align256(o + n);
  L.st = o; o = align256(o + 4 * n);
  L.log = o; o = align256(o + (size_t)SIT_LOG_ROWS * n * rs);
  L.blob = o; o = align256(o + h->blob_bytes);
  L.bytes = o;
  return L;
}

int sit_step_host(sit_handle* h, const void* action_ne, const uint8_t* sac_update, const uint8_t* init,
                  void* next_state, void* reward, uint8_t* done, uint32_t* status, void* log, void* state,
                  void* stream) {
  int rc = ready(h);
  if (rc) return rc;
  if (!action_ne || !sac_update || !init) return fail(h, SIT_E_INVALID, "action_ne, sac_update and init are required");
#ifdef SIT_HOST_MEMORY_TEST
  (void)next_state; (void)reward; (void)done; (void)status; (void)log; (void)state; (void)stream;
  return fail(h, SIT_E_STATE, "sit_step_host: no device in the host-memory test build");
#else
  const StageLayout L = stage_layout(h);
  if (!h->stage_dev) {   // allocated into locals; published only once both calls succeeded
    unsigned char* hp = nullptr;
    HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&hp), L.bytes, hipHostMallocMapped | hipHostMallocCoherent));
    void* dp = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&dp, hp, 0);
    if (e != hipSuccess || !dp) {
      (void)hipHostFree(hp);
      return fail(h, SIT_E_HIP, "hipHostGetDevicePointer: %s", hipGetErrorString(e));
    }
    h->stage = hp;
    h->stage_dev = static_cast<unsigned char*>(dp);
  }
  const size_t n = (size_t)h->n_env, rs = real_size(h);
  std::memcpy(h->stage + L.act, action_ne, 2 * n * rs);
  std::memcpy(h->stage + L.sac, sac_update, n);
  std::memcpy(h->stage + L.init, init, n);
  unsigned char* d = h->stage_dev;
  hipStream_t s = (hipStream_t)stream;
  rc = with_real(h, [&](auto t) {
    using T = decltype(t);
    auto io = single_step_io<T>(d + L.act, d + L.sac, d + L.init, d + L.ns, d + L.rw, d + L.dn, (uint32_t*)(d + L.st));
    io.log = log ? (T*)(d + L.log) : nullptr;
    return steps(h, io, stream);
  });
  if (rc) return rc;
  if (state) HIP_TRY(h, hipMemcpyAsync(h->stage + L.blob, h->blob, h->blob_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  if (next_state) std::memcpy(next_state, h->stage + L.ns, (size_t)SIT_OBS_DIM * n * rs);
  if (reward) std::memcpy(reward, h->stage + L.rw, n * rs);
  if (done) std::memcpy(done, h->stage + L.dn, n);
  if (status) std::memcpy(status, h->stage + L.st, 4 * n);
  if (log) std::memcpy(log, h->stage + L.log, (size_t)SIT_LOG_ROWS * n * rs);
  if (state) std::memcpy(state, h->stage + L.blob, h->blob_bytes);
  return SIT_OK;
#endif
}

int sit_rollout(sit_handle* h, const sit_rollout_args* ra, void* stream) {
  int rc = ready(h);
  if (rc) return rc;
  if (!ra) return fail(h, SIT_E_INVALID, "null rollout args");
  if (ra->n_steps <= 0) return fail(h, SIT_E_INVALID, "n_steps must be positive");
  if (!ra->next_state && !ra->reward) return fail(h, SIT_E_INVALID, "need next_state or reward output");
  if (ra->action_ne && (!ra->sac_update || !ra->init))
    return fail(h, SIT_E_INVALID, "explicit actions need sac_update and init");
  if (ra->env_id_offset < 0) return fail(h, SIT_E_INVALID, "env_id_offset must be >= 0");
  if (!pair_aligned(h, ra->next_state) || !pair_aligned(h, ra->action_out))
    return fail(h, SIT_E_INVALID, "next_state and action_out must be aligned to 2 reals");
  if (ra->transitions && (!ra->transition_count || ra->transition_capacity <= 0))
    return fail(h, SIT_E_INVALID, "transitions need transition_count and a positive capacity");
  if (reinterpret_cast<uintptr_t>(ra->transitions) % (4 * real_size(h)) != 0)
    return fail(h, SIT_E_INVALID, "transitions must be aligned to 4 reals");
  if (ra->policy_action && ra->action_ne)
    return fail(h, SIT_E_INVALID, "policy mode and explicit actions are exclusive");
  const bool serve = ra->policy_action && ra->actor_weights;
  if (ra->actor_weights && !ra->policy_action) return fail(h, SIT_E_INVALID, "actor_weights need policy mode");
  if (serve && !ra->policy_ready) return fail(h, SIT_E_INVALID, "policy mode needs policy_ready");
  if (ra->policy_action && !serve &&
      (!ra->policy_ready || !ra->request_env || !ra->request_noise || !ra->request_obs || !ra->request_count ||
       !ra->request_age || ra->request_capacity <= 0))
    return fail(h, SIT_E_INVALID, "policy mode needs policy_ready, request_env, request_noise, "
                                  "request_obs, request_count, request_age and a positive request_capacity "
                                  "(or actor_weights: in-kernel serving)");
  auto fill = [&](auto* io) {
    using R = std::remove_pointer_t<decltype(io->next_state)>;
    io->n_steps = ra->n_steps; io->auto_reset = ra->auto_reset; io->seed = ra->seed;
    io->env_id_offset = ra->env_id_offset;
    io->action_ne = (const R*)ra->action_ne; io->sac_update = ra->sac_update; io->init = ra->init;
    io->next_state = (R*)ra->next_state; io->reward = (R*)ra->reward; io->done = ra->done;
    io->status = ra->status; io->action_out = (R*)ra->action_out; io->done_count = ra->done_count;
    io->transitions = (R*)ra->transitions; io->transition_count = ra->transition_count;
    io->transition_capacity = ra->transition_capacity; io->mask_horizon = ra->mask_horizon;
    // (policy_action: the kernel reads it and, serving, writes it)
    io->policy_action = const_cast<R*>(static_cast<const R*>(ra->policy_action)); io->policy_ready = ra->policy_ready;
    io->request_age = serve ? nullptr : ra->request_age;
    io->group_counts = (ra->policy_action && !serve) ? admit_counts(h) : nullptr;
    io->env_steps = reinterpret_cast<unsigned long long*>(ra->env_steps);
    io->log = (R*)ra->log;
    io->actor_w = serve ? ra->actor_weights : nullptr;
    io->actor_det = ra->actor_deterministic;
    io->actor_served = reinterpret_cast<unsigned long long*>(ra->actor_served);
  };
  // policy mode: the step kernel, then the deterministic admission of the waiting envs into the
  // request queue (k_policy_admit, sit_actor.h) on the same stream — or, serving in the kernel, nothing;
  // a serving launch that takes the one-wave kernel (logged) is served through the library's own queue
  auto run = [&](auto* io) -> int {
    using R = std::remove_pointer_t<decltype(io->next_state)>;    sit_rollout_args q = *ra;
    if (serve && sync_launch_lds<R>(h, *io, nullptr, nullptr) == 0) {
      const ServeQueue sq = serve_queue(h);
      io->actor_w = nullptr;
      io->request_age = sq.age;
      io->group_counts = admit_counts(h);
      q.request_capacity = h->n_env; q.request_env = sq.env; q.request_obs = sq.obs; q.request_noise = sq.noise;
      q.request_count = sq.count; q.request_age = sq.age;
    } else if (serve) {
      return steps(h, *io, stream);
    }
    int r = steps(h, *io, stream);
    if (r == SIT_OK && ra->policy_action) r = launch_policy_admit<R>(h, &q, (hipStream_t)stream);
    if (r == SIT_OK && serve)
      r = launch_policy_actor<R>(h, h->n_env, ra->actor_weights, q.request_obs, q.request_noise, q.request_env,
                                 q.request_count, ra->actor_deterministic, const_cast<void*>(ra->policy_action),
                                 ra->policy_ready, ra->actor_served, nullptr, (hipStream_t)stream);
    return r;
  };
  rc = with_real(h, [&](auto t) {
    StepIO<decltype(t)> io{};
    fill(&io);
    return run(&io);
  });
  if (rc) return rc;
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
}

int sit_state_field(const sit_handle* h, int32_t id, const char** name, size_t* offset, int32_t* dtype,
                    int64_t* count) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (id < 0 || id >= kNumFields) return SIT_E_INVALID;
  if (name) *name = kFields[id].name;
  if (offset) *offset = h->off[id];
  if (dtype) *dtype = kFields[id].dtype;
  if (count) *count = h->count[id];
  return SIT_OK;
}

int sit_state_bytes(const sit_handle* h, size_t* bytes) {
  if (!h || !bytes) return fail(nullptr, SIT_E_INVALID, "null argument");
  *bytes = h->blob_bytes;
  return SIT_OK;
}

int sit_get_state(sit_handle* h, void* dst, void* stream) {
  if (!h || !dst) return fail(h, SIT_E_INVALID, "null argument");
  HIP_TRY(h, hipMemcpyAsync(dst, h->blob, h->blob_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SIT_OK;
}

int sit_set_state(sit_handle* h, const void* src, void* stream) {
  if (!h || !src) return fail(h, SIT_E_INVALID, "null argument");
  HIP_TRY(h, hipMemcpyAsync(h->blob, src, h->blob_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  // the cached IW terrain tests (iw_key_*) are answers for the map of the handle that saved the blob:
  // a restored state re-tests its IW against this handle's map
  HIP_TRY(h, hipMemsetAsync(h->blob + h->off[F_IWK_FLAGS], 0, (size_t)h->n_env * 4, (hipStream_t)stream));
  return SIT_OK;
}

// ---- episode records (sit_episodes.h) ------------------------------------------------------
size_t sit_episodes_args_size(void) { return sizeof(sit_episodes_args); }

int sit_episodes_reset(sit_handle* h, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  int rc = episodes_alloc(h);
  if (rc) return rc;
  return episodes_launch_reset(h, (hipStream_t)stream);
}

int sit_episodes_update(sit_handle* h, const sit_episodes_args* a, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (!a) return fail(h, SIT_E_INVALID, "episodes: null args");
  if (a->n_steps <= 0) return fail(h, SIT_E_INVALID, "episodes: n_steps must be positive (got %d)", a->n_steps);
  if (a->record_capacity < 0)
    return fail(h, SIT_E_INVALID, "episodes: record_capacity must be >= 0 (got %d)", a->record_capacity);
  if (!a->reward) return fail(h, SIT_E_INVALID, "episodes: reward is required");
  if (!a->done) return fail(h, SIT_E_INVALID, "episodes: done is required");
  if (!a->status) return fail(h, SIT_E_INVALID, "episodes: status is required");
  if (!a->record_count) return fail(h, SIT_E_INVALID, "episodes: record_count is required");
  if (!a->records && a->record_capacity > 0)
    return fail(h, SIT_E_INVALID, "episodes: records is NULL with record_capacity %d", a->record_capacity);
  if (a->env_id_offset < 0) return fail(h, SIT_E_INVALID, "episodes: env_id_offset must be >= 0");
  if (!h->episodes) {   // first use without sit_episodes_reset: allocate and zero (not capturable)
    int rc = sit_episodes_reset(h, stream);
    if (rc) return rc;
  }
  return with_real(h, [&](auto t) { return episodes_launch_update<decltype(t)>(h, a, (hipStream_t)stream); });
}

int sit_episodes_bytes(const sit_handle* h, size_t* bytes) {
  if (!h || !bytes) return fail(nullptr, SIT_E_INVALID, "null argument");
  *bytes = ep_layout(h).blob_bytes;
  return SIT_OK;
}

int sit_episodes_get(sit_handle* h, void* dst, void* stream) {
  if (!h || !dst) return fail(h, SIT_E_INVALID, "null argument");
  if (!h->episodes) {
    int rc = sit_episodes_reset(h, stream);
    if (rc) return rc;
  }
  HIP_TRY(h, hipMemcpyAsync(dst, h->episodes, ep_layout(h).blob_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SIT_OK;
}

int sit_episodes_set(sit_handle* h, const void* src, void* stream) {
  if (!h || !src) return fail(h, SIT_E_INVALID, "null argument");
  int rc = episodes_alloc(h);
  if (rc) return rc;
  HIP_TRY(h, hipMemcpyAsync(h->episodes, src, ep_layout(h).blob_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SIT_OK;
}

// ---- scores (sit_score.h) --------------------------------------------------------------------
size_t sit_score_args_size(void) { return sizeof(sit_score_args); }
size_t sit_score_keep_args_size(void) { return sizeof(sit_score_keep_args); }

int sit_score_reset(sit_handle* h, double* score, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = score_block_error(score)) return fail(h, SIT_E_INVALID, "%s", why);
  return score_launch_reset(h, score, (hipStream_t)stream);
}

int sit_score_reserve(sit_handle* h, int32_t max_records) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = score_reserve_args_error(max_records)) return fail(h, SIT_E_INVALID, "%s (got %d)", why, max_records);
  return score_reserve(h, (size_t)max_records);
}

int sit_score_update(sit_handle* h, const sit_score_args* a, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = score_update_args_error(a)) return fail(h, SIT_E_INVALID, "%s", why);
  return score_launch_update(h, a, (hipStream_t)stream);
}

int sit_score_keep(sit_handle* h, const sit_score_keep_args* a, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = score_keep_args_error(a)) return fail(h, SIT_E_INVALID, "%s", why);
  return score_launch_keep(h, a, (hipStream_t)stream);
}

// ---- replay memory (sit_replay.h) ----------------------------------------------------------
size_t sit_replay_push_args_size(void) { return sizeof(sit_replay_push_args); }
size_t sit_replay_sample_args_size(void) { return sizeof(sit_replay_sample_args); }

int sit_replay_reserve(sit_handle* h, int32_t max_src_capacity, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (max_src_capacity <= 0)
    return fail(h, SIT_E_INVALID, "replay: max_src_capacity must be positive (got %d)", max_src_capacity);
  return replay_reserve(h, (size_t)max_src_capacity, (hipStream_t)stream);
}

int sit_replay_push(sit_handle* h, const sit_replay_push_args* a, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (!a) return fail(h, SIT_E_INVALID, "replay: null args");
  if (a->capacity <= 0) return fail(h, SIT_E_INVALID, "replay: capacity must be positive (got %d)", a->capacity);
  if (a->src_capacity <= 0)
    return fail(h, SIT_E_INVALID, "replay: src_capacity must be positive (got %d)", a->src_capacity);
  if (!a->ring) return fail(h, SIT_E_INVALID, "replay: ring is required");
  if (!a->cursor) return fail(h, SIT_E_INVALID, "replay: cursor is required");
  if (!a->src) return fail(h, SIT_E_INVALID, "replay: src is required");
  if (!a->src_count) return fail(h, SIT_E_INVALID, "replay: src_count is required");
  const size_t quad = 4 * real_size(h);   // records are copied in 16-byte pieces
  if ((uintptr_t)a->ring % quad) return fail(h, SIT_E_INVALID, "replay: ring must be aligned to 4 reals (%zu bytes)", quad);
  if ((uintptr_t)a->src % quad) return fail(h, SIT_E_INVALID, "replay: src must be aligned to 4 reals (%zu bytes)", quad);
  return with_real(h, [&](auto t) { return replay_launch_push<decltype(t)>(h, a, (hipStream_t)stream); });
}

// affine: NULL for sit_replay_sample, the affine of sit_replay_sample_normalised
static int replay_sample(sit_handle* h, const sit_replay_sample_args* a, const float* affine, void* stream) {
  if (!a) return fail(h, SIT_E_INVALID, "replay: null args");
  if (a->capacity <= 0) return fail(h, SIT_E_INVALID, "replay: capacity must be positive (got %d)", a->capacity);
  if (a->batch <= 0) return fail(h, SIT_E_INVALID, "replay: batch must be positive (got %d)", a->batch);
  if (a->n_batches <= 0) return fail(h, SIT_E_INVALID, "replay: n_batches must be positive (got %d)", a->n_batches);
  if ((int64_t)a->batch * a->n_batches > (int64_t)1 << 30)
    return fail(h, SIT_E_INVALID, "replay: batch * n_batches must not exceed 2^30 (got %d * %d)", a->batch, a->n_batches);
  if (!a->ring) return fail(h, SIT_E_INVALID, "replay: ring is required");
  if (!a->cursor) return fail(h, SIT_E_INVALID, "replay: cursor is required");
  if (!a->state || !a->action || !a->reward || !a->next_state || !a->mask || !a->env || !a->index)
    return fail(h, SIT_E_INVALID, "replay: every output (state, action, reward, next_state, mask, env, index) is required");
  const size_t quad = 4 * real_size(h);
  if ((uintptr_t)a->ring % quad) return fail(h, SIT_E_INVALID, "replay: ring must be aligned to 4 reals (%zu bytes)", quad);
  return with_real(h, [&](auto t) { return replay_launch_sample<decltype(t)>(h, a, (hipStream_t)stream, affine); });
}

int sit_replay_sample(sit_handle* h, const sit_replay_sample_args* a, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  return replay_sample(h, a, nullptr, stream);
}

int sit_replay_sample_normalised(sit_handle* h, const sit_replay_sample_args* a, const float* affine, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = obsnorm_affine_error(affine)) return fail(h, SIT_E_INVALID, "%s", why);
  return replay_sample(h, a, affine, stream);
}

// ---- SAC learner (sit_sac.h) ---------------------------------------------------------------
size_t sit_sac_target_args_size(void) { return sizeof(sit_sac_target_args); }

int sit_sac_target(sit_handle* h, const sit_sac_target_args* a, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = sac_target_args_error(a)) return fail(h, SIT_E_INVALID, "%s", why);
  return with_real(h, [&](auto t) { return sac_launch_target<decltype(t)>(h, a, (hipStream_t)stream); });
}

int sit_sac_polyak(sit_handle* h, float* target, const float* online, int64_t n, float tau, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = sac_polyak_args_error(target, online, n)) return fail(h, SIT_E_INVALID, "%s", why);
  return sac_launch_polyak(h, target, online, n, tau, (hipStream_t)stream);
}

// ---- SAC learner, the gradient half (sit_sac_grad.h) -----------------------------------------
int64_t sit_sac_workspace_floats(int32_t batch) { return sac_workspace_floats(batch); }
size_t sit_sac_critic_step_args_size(void) { return sizeof(sit_sac_critic_step_args); }
size_t sit_sac_policy_step_args_size(void) { return sizeof(sit_sac_policy_step_args); }

// tiled: the weight gradients as MFMA tiles (sit_sac_wgrad.h) instead of one sum per element
static int sac_critic_step(sit_handle* h, const sit_sac_critic_step_args* a, bool tiled, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = sac_critic_step_args_error(a)) return fail(h, SIT_E_INVALID, "%s", why);
  const SacAdamLaunch adam = sac_adam_launch<kSacIn, 1, 2, SIT_CRITIC_WEIGHTS, false>(tiled);
  return with_real(h, [&](auto t) { return sac_launch_critic_step<decltype(t)>(h, a, adam, (hipStream_t)stream); });
}

static int sac_policy_step(sit_handle* h, const sit_sac_policy_step_args* a, bool tiled, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = sac_policy_step_args_error(a)) return fail(h, SIT_E_INVALID, "%s", why);
  const SacAdamLaunch adam = sac_adam_launch<kActorObs, 2, 1, SIT_ACTOR_WEIGHTS, true>(tiled);
  return with_real(h, [&](auto t) { return sac_launch_policy_step<decltype(t)>(h, a, adam, (hipStream_t)stream); });
}

int sit_sac_critic_step(sit_handle* h, const sit_sac_critic_step_args* a, void* stream) {
  return sac_critic_step(h, a, false, stream);
}
int sit_sac_policy_step(sit_handle* h, const sit_sac_policy_step_args* a, void* stream) {
  return sac_policy_step(h, a, false, stream);
}
int sit_sac_critic_step_tiled(sit_handle* h, const sit_sac_critic_step_args* a, void* stream) {
  return sac_critic_step(h, a, true, stream);
}
int sit_sac_policy_step_tiled(sit_handle* h, const sit_sac_policy_step_args* a, void* stream) {
  return sac_policy_step(h, a, true, stream);
}

// ---- SAC learner, the row kernels on the matrix cores (sit_sac_rows.h) -------------------------
int sit_sac_target_wide(sit_handle* h, const sit_sac_target_args* a, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = sac_target_args_error(a)) return fail(h, SIT_E_INVALID, "%s", why);
  return with_real(h, [&](auto t) { return sac_launch_target_wide<decltype(t)>(h, a, (hipStream_t)stream); });
}
int sit_sac_critic_step_wide(sit_handle* h, const sit_sac_critic_step_args* a, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = sac_critic_step_args_error(a)) return fail(h, SIT_E_INVALID, "%s", why);
  return with_real(h, [&](auto t) { return sac_launch_critic_step_wide<decltype(t)>(h, a, (hipStream_t)stream); });
}
int sit_sac_policy_step_wide(sit_handle* h, const sit_sac_policy_step_args* a, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = sac_policy_step_args_error(a)) return fail(h, SIT_E_INVALID, "%s", why);
  return with_real(h, [&](auto t) { return sac_launch_policy_step_wide<decltype(t)>(h, a, (hipStream_t)stream); });
}

// ---- SAC learner, many updates per call from the device clock (sit_sac_clock.h, sit_sac_rows.h) ----
size_t sit_sac_updates_args_size(void) { return sizeof(sit_sac_updates_args); }

int sit_sac_updates(sit_handle* h, const sit_sac_updates_args* a, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = sac_updates_args_error(a)) return fail(h, SIT_E_INVALID, "%s", why);
  return with_real(h, [&](auto t) { return sac_launch_updates<decltype(t)>(h, a, (hipStream_t)stream); });
}

int sit_sac_adam_scalars(sit_handle* h, const sit_sac_adam* o, int64_t t0, int32_t n, float* out, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = sac_adam_scalars_args_error(o, t0, n, out)) return fail(h, SIT_E_INVALID, "%s", why);
  return sac_launch_adam_scalars(h, o, t0, n, out, (hipStream_t)stream);
}

// ---- observation normalisation (sit_obsnorm.h) -------------------------------------------------
size_t sit_obsnorm_args_size(void) { return sizeof(sit_obsnorm_args); }

int sit_obsnorm_reset(sit_handle* h, double* block, float* affine, const float* min_std, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = obsnorm_reset_args_error(block, affine, min_std)) return fail(h, SIT_E_INVALID, "%s", why);
  return obsnorm_launch_reset(h, block, affine, min_std, (hipStream_t)stream);
}

int sit_obsnorm_reserve(sit_handle* h, int32_t max_new) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = obsnorm_reserve_args_error(max_new)) return fail(h, SIT_E_INVALID, "%s (got %d)", why, max_new);
  return obsnorm_reserve(h, (size_t)max_new);
}

int sit_obsnorm_update(sit_handle* h, const sit_obsnorm_args* a, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = obsnorm_update_args_error(a, real_size(h), (int64_t)h->obsnorm_records))
    return fail(h, SIT_E_INVALID, "%s", why);
  return with_real(h, [&](auto t) { return obsnorm_launch_update<decltype(t)>(h, a, (hipStream_t)stream); });
}

int sit_obsnorm_apply(sit_handle* h, const float* affine, void* rows_a, void* rows_b, int64_t n_rows, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = obsnorm_apply_args_error(affine, rows_a, rows_b, n_rows, real_size(h)))
    return fail(h, SIT_E_INVALID, "%s", why);
  return with_real(h, [&](auto t) {
    return obsnorm_launch_apply<decltype(t)>(h, affine, rows_a, rows_b, n_rows, (hipStream_t)stream);
  });
}

int sit_obsnorm_fold(sit_handle* h, const float* affine, const float* src, float* dst, void* stream) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (const char* why = obsnorm_fold_args_error(affine, src, dst)) return fail(h, SIT_E_INVALID, "%s", why);
  return obsnorm_launch_fold(h, affine, src, dst, (hipStream_t)stream);
}

}  // extern "C"
