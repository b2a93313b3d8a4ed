// sit_host.h — host side of the ship-in-transit env step over the kernels of sit_impl.h: the
// handle, error reporting, the setup-memory shims, the blob layouts, the derived constants and
// kernel arguments, and the step / probe launchers.  Included by both translation units
// (sit_kernels.hip: the C ABI; sit_steps_f32.hip: the float32 step launches).
#pragma once

#include "sit_impl.h"

struct sit_handle {
  int precision = SIT_F32;
  int n_env = 0;
  int cap = 0;
  int device = 0;
  sit_params p{};
  std::string err;
  // state blob
  unsigned char* blob = nullptr;
  size_t blob_bytes = 0;
  size_t off[kNumFields] = {};
  int64_t count[kNumFields] = {};
  // scenario
  unsigned char* scen = nullptr;
  size_t scen_init = 0, scen_init_lo = 0, scen_end_n = 0, scen_end_e = 0, scen_nw0 = 0, scen_ab_len = 0,
         scen_ab_alpha = 0, scen_initial = 0, scen_admit = 0, scen_serve = 0, scen_bytes = 0;
  // map: the uploaded image (build_map_image, sit_map_build.h) and what it says about itself
  unsigned char* map = nullptr;
  MapMeta meta;
  int lds_attr[24] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
                      -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};   // dynamic-LDS size per step-kernel variant
  int lds_attr_sync[12] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};   // k_env_steps_sync [mode][mach][lds]
  bool lds_attr_rows[5] = {false, false, false, false, false};   // the wide SAC row kernels (sit_sac_rows.h): attribute set
  // step-kernel selection, read once at sit_create (diagnostics / A-B runs only):
  //   SIT_STEP_KERNEL=classic  k_env_steps for every mode (default: k_env_steps_sync where it applies)
  //   SIT_LDS_MAP=0|1          map read through the caches / staged in LDS for every launch
  //                            (default: staged when the launch has >= kLdsMinSteps steps)
  int kernel_classic = 0;
  int lds_map_sel = -1;
  int fake_simds = 0;                // SIT_TEST_FAKE_SIMDS (test hook): 0x100 | base-4 SIMD assignment
  char last_kernel[96] = {};         // the step kernel of the last sit_step / sit_rollout launch
  bool have_map = false, have_routes = false, have_init = false;
  unsigned char* stage = nullptr;       // sit_step_host: pinned coherent host staging
  unsigned char* stage_dev = nullptr;   // its device address
  unsigned char* episodes = nullptr;    // sit_episodes_*: accumulator blob + scratch (sit_episodes.h)
  unsigned char* replay = nullptr;      // sit_replay_push: sort keys, values and temporary storage (sit_replay.h)
  size_t replay_items = 0;              //   records the scratch holds
  size_t replay_temp = 0;               //   bytes of the sort's temporary storage
  size_t replay_asked = 0;              //   the last size query: items and the bytes hipcub asked for
  size_t replay_answer = 0;
  unsigned char* score = nullptr;       // sit_score_update: one ScPart per chunk of 256 record slots (sit_score.h)
  size_t score_chunks = 0;              //   chunks the scratch holds
  unsigned char* obsnorm = nullptr;     // sit_obsnorm_update: mean_b and two sums per chunk of 256 records (sit_obsnorm.h)
  size_t obsnorm_records = 0;           //   records the scratch was reserved for
};

namespace {

thread_local std::string g_create_err;

int fail(sit_handle* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h) h->err = buf; else g_create_err = buf;
  return code;
}

#define HIP_TRY(h, call)                                                                    \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) return fail((h), SIT_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)

// Device memory of the setup calls (sit_create / sit_load_* / sit_destroy).  Sanitizer builds
// (-DSIT_HOST_MEMORY_TEST, tools/sanitize.sh: host ASan/UBSan) back it with host memory, so that
// the host logic -- argument checks, blob layout, the map index, route and scenario staging --
// runs and is checked on a machine without a GPU; kernels are not launched in that build.
#ifdef SIT_HOST_MEMORY_TEST
hipError_t setup_device(int* d) { *d = 0; return hipSuccess; }
hipError_t setup_alloc(unsigned char** p, size_t n) {
  *p = static_cast<unsigned char*>(std::malloc(n ? n : 1));
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t setup_free(void* p) { std::free(p); return hipSuccess; }
hipError_t setup_zero(void* p, size_t n) { std::memset(p, 0, n); return hipSuccess; }
hipError_t setup_upload(void* dst, const void* src, size_t n) { std::memcpy(dst, src, n); return hipSuccess; }
#else
hipError_t setup_device(int* d) { return hipGetDevice(d); }
hipError_t setup_alloc(unsigned char** p, size_t n) { return hipMalloc(p, n); }
hipError_t setup_free(void* p) { return hipFree(p); }
hipError_t setup_zero(void* p, size_t n) { return hipMemset(p, 0, n); }
hipError_t setup_upload(void* dst, const void* src, size_t n) { return hipMemcpy(dst, src, n, hipMemcpyHostToDevice); }
#endif

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }
size_t real_size(const sit_handle* h) { return h->precision == SIT_F64 ? 8 : 4; }

// f(T{}) with T the handle's real type: the one place a handle's precision picks a template argument
template <typename F>
auto with_real(const sit_handle* h, F&& f) {
  if (h->precision == SIT_F64) return f(double{});
  return f(float{});
}

// state blob (sit_create): the fields of kFields in order, each 256-B aligned
void layout_state(sit_handle* h) {
  const size_t rs = real_size(h);
  const int64_t n_env = h->n_env;
  size_t off = 0;
  for (int f = 0; f < kNumFields; ++f) {
    int64_t cnt = kFields[f].extent == kShip ? 2 * n_env
                 : kFields[f].extent == kEnv ? n_env
                 : kFields[f].extent == kObs ? SIT_OBS_DIM * n_env
                 : kFields[f].extent == kLogRow ? SIT_LOG_KEYS * n_env : 2LL * h->cap * n_env;
    const size_t el = kFields[f].dtype == SIT_DT_REAL ? rs : 4;
    h->off[f] = off;
    h->count[f] = cnt;
    off = align256(off + (size_t)cnt * el);
  }
  h->blob_bytes = off;
}

// in-kernel serving's fallback queue inside the scenario blob (serve_queue): env, age and count as
// [3][n_env] i32, then 256-B aligned the observations and the noise
struct ServeLayout {
  size_t obs, noise, bytes;
};
ServeLayout serve_layout(const sit_handle* h) {
  const size_t n = (size_t)h->n_env, rs = real_size(h);
  ServeLayout L{};
  L.obs = align256(3 * n * 4);
  L.noise = L.obs + n * SIT_OBS_DIM * rs;
  L.bytes = n * (3 * 4 + (SIT_OBS_DIM + 1) * rs) + 256;   // reserved: >= noise + n reals
  return L;
}

// scenario blob (sit_create)
void layout_scen(sit_handle* h) {
  const size_t rs = real_size(h), n_env = (size_t)h->n_env;
  size_t so = 0;
  h->scen_init = so; so = align256(so + (size_t)2 * SIT_INIT_NF * n_env * rs);
  h->scen_init_lo = so; so = align256(so + (size_t)2 * SIT_INIT_NF * n_env * rs);
  h->scen_end_n = so; so = align256(so + (size_t)2 * n_env * rs);
  h->scen_end_e = so; so = align256(so + (size_t)2 * n_env * rs);
  h->scen_nw0 = so; so = align256(so + (size_t)2 * n_env * 4);
  h->scen_ab_len = so; so = align256(so + (size_t)n_env * 8);
  h->scen_ab_alpha = so; so = align256(so + (size_t)n_env * 8);
  h->scen_initial = so; so = align256(so + (size_t)n_env * SIT_OBS_DIM * rs);
  // policy-mode admission scratch (sit_actor.h): per 64-env group the age-bucket counts and the plan
  const size_t n_groups = (n_env + kAdmitGroup - 1) / kAdmitGroup;
  h->scen_admit = so; so = align256(so + (n_groups * (kAgeBuckets + 2) + 16) * 4);
  // in-kernel serving's fallback queue (logged policy launches): capacity n_env, zero ages
  h->scen_serve = so; so = align256(so + serve_layout(h).bytes);
  h->scen_bytes = so;
}

// Derived constants, computed like the reference constructors (ship_model.py:71-130,
// ship_engine.py:32-44, 316-325; controllers; MSRL_env_ex.py).
template <typename T>
Consts<T> make_consts(const sit_handle* h) {
  const sit_params& p = h->p;
  const MapMeta& m = h->meta;
  Consts<T> c{};
  const double dwt = p.dead_weight_tonnage;
  const double payload = 0.9 * (dwt - p.bunkers);
  const double lsw = dwt / p.coefficient_of_deadweight_to_displacement - dwt;
  const double mass = lsw + payload + p.bunkers + p.ballast;
  const double l = p.length_of_ship, w = p.width_of_ship;
  const double i_z = mass * (l * l + w * w) / 12;
  const double x_du = mass * p.added_mass_coefficient_in_surge;
  const double y_dv = mass * p.added_mass_coefficient_in_sway;
  const double n_dr = i_z * p.added_mass_coefficient_in_yaw;
  const double area_f = w * p.front_height, area_l = l * p.side_height;
  c.dt = (T)p.integration_step;
  c.mass = (T)mass; c.x_du = (T)x_du; c.y_dv = (T)y_dv;
  c.inv_m11 = (T)(1.0 / (mass + x_du));
  c.inv_m22 = (T)(1.0 / (mass + y_dv));
  c.inv_m33 = (T)(1.0 / (i_z + n_dr));
  c.d_u = (T)(mass / p.mass_over_linear_friction_coefficient_in_surge);
  c.d_v = (T)(mass / p.mass_over_linear_friction_coefficient_in_sway);
  c.d_r = (T)(i_z / p.mass_over_linear_friction_coefficient_in_yaw);
  c.ku = (T)p.nonlinear_friction_coefficient_in_surge;
  c.kv = (T)p.nonlinear_friction_coefficient_in_sway;
  c.kr = (T)p.nonlinear_friction_coefficient_in_yaw;
  c.vc_n = (T)p.current_velocity_component_from_north;
  c.vc_e = (T)p.current_velocity_component_from_east;
  c.wind_speed = (T)p.wind_speed;
  c.wind_sin = (T)std::sin(p.wind_direction);
  c.wind_cos = (T)std::cos(p.wind_direction);
  c.wk_u = (T)(-0.5 * p.rho_air * p.cx * area_f);
  c.wk_v = (T)(-0.5 * p.rho_air * p.cy * area_l);
  c.wk_n = (T)(-p.rho_air * p.cn * area_l * l);
  c.c_rv = (T)p.rudder_angle_to_sway_force_coefficient;
  c.c_rr = (T)p.rudder_angle_to_yaw_force_coefficient;
  c.rudder_max = (T)(p.max_rudder_angle_degrees * M_PI / 180);
  const double me = p.main_engine_capacity, el = p.electrical_capacity, hotel = p.hotel_load;
  double avail = 0, avail_me = 0, avail_el = 0;
  if (hotel != 0.0) {   // BaseMachineryModel only sets the powers for a truthy hotel load
    if (p.shaft_generator_state == SIT_SG_MOTOR) { avail = me + el - hotel; avail_me = me; avail_el = el - hotel; }
    else if (p.shaft_generator_state == SIT_SG_GEN) { avail = me - hotel; avail_me = me - hotel; avail_el = 0; }
    else { avail = me; avail_me = me; avail_el = 0; }
  }
  c.avail_prop = (T)avail; c.avail_me = (T)avail_me; c.avail_el = (T)avail_el;
  c.tqcap_me = (T)(avail_me / 5 * M_PI / 30);
  c.tqcap_el = (T)(avail_el / 5 * M_PI / 30);
  c.d_me = (T)p.linear_friction_main_engine;
  c.d_hsg = (T)p.linear_friction_hybrid_shaft_generator;
  c.r_me = (T)p.gear_ratio_between_main_engine_and_propeller;
  c.r_hsg = (T)p.gear_ratio_between_hybrid_shaft_generator_and_propeller;
  c.kp_prop = (T)p.propeller_speed_to_torque_coefficient;
  c.jp = (T)p.propeller_inertia;
  c.thrust_k = (T)(std::pow(p.propeller_diameter, 4.0) * p.propeller_speed_to_thrust_force_coefficient);
  c.me_cap = (T)me; c.hotel = (T)hotel; c.load_el_gen = (T)std::min(hotel, el);
  c.sg_mode = p.shaft_generator_state;
  c.mach_simpl = p.machinery_model == SIT_MACH_SIMPLIFIED;
  // SimplifiedMachineryModel (ship_engine.py:420-428): power = load_perc * (available propulsion
  // power of the main engine + of the electrical side), k_thrust = 2160 / 790
  c.k_thrust = (T)(2160.0 / 790.0);
  c.inv_tau = (T)(1.0 / p.thrust_force_dynamic_time_constant);
  c.p_simpl = (T)(avail_me + avail_el);
  c.collision_bias = p.collision_bias;
  c.kp1 = (T)p.kp_ship_speed; c.ki1 = (T)p.ki_ship_speed;
  c.kp2 = (T)p.kp_shaft_speed; c.ki2 = (T)p.ki_shaft_speed;
  c.kp_h = (T)p.heading_kp; c.kd_h = (T)p.heading_kd; c.ki_h = (T)p.heading_ki;
  c.los_r = (T)p.lookahead_distance;
  c.los_r2 = (T)(p.lookahead_distance * p.lookahead_distance);
  c.los_clamp = (T)(0.99 * p.lookahead_distance);
  c.los_ki = (T)p.los_integral_gain;
  c.windup = (T)p.integrator_windup_limit;
  c.ra2 = p.radius_of_acceptance * p.radius_of_acceptance;
  c.bias_scale = (T)p.bias_throttle_scale;
  c.bias_max = (T)p.bias_throttle_max;
  c.bias_rudder = (T)(p.bias_rudder_degrees * (M_PI / 180.0));
  c.e_tol = (T)p.e_tolerance;
  c.arrival_radius = (T)p.arrival_radius;
  c.rpm_max = (T)p.shaft_rpm_max;
  c.min_dist2 = (T)(p.minimum_ship_distance * p.minimum_ship_distance);
  c.coll_d2 = p.minimum_ship_distance * p.minimum_ship_distance;
  {  // sqrt(x) <= r  <=>  x <= d2_le (IEEE sqrt is correctly rounded and monotone)
    const double r = p.arrival_radius;
    double v = r * r;
    // (towards +-DBL_MAX, not infinity: the float32 TU's device pass parses this with finite math)
    while (std::sqrt(std::nextafter(v, DBL_MAX)) <= r) v = std::nextafter(v, DBL_MAX);
    while (v > 0 && std::sqrt(v) > r) v = std::nextafter(v, -DBL_MAX);
    c.arrive_d2_le = v;
  }
  c.theta = (T)p.theta;
  c.blackout_kw = (T)(me / 1000);
  c.rpm_k = c.mach_simpl ? T(0) : (T)(30.0 / M_PI);   // SimplifiedMachineryModel: no shaft
  c.inv_dt = (T)(1.0 / p.integration_step);
  c.inv_e_tol = (T)(1.0 / p.e_tolerance);
  c.inv_maxn = (T)(1.0 / m.max_n);
  c.inv_jp = (T)(1.0 / p.propeller_inertia);
  c.inv_r_me = (T)(1.0 / p.gear_ratio_between_main_engine_and_propeller);
  c.inv_r_hsg = (T)(1.0 / p.gear_ratio_between_hybrid_shaft_generator_and_propeller);
  c.half_len = (T)(l / 2);
  c.min_n = (T)m.min_n; c.max_n = (T)m.max_n; c.min_e = (T)m.min_e; c.max_e = (T)m.max_e;
  c.pi6 = (T)(M_PI / 6.0);
  c.gx0 = (T)m.gx0; c.gy0 = (T)m.gy0; c.ginvx = (T)m.ginvx; c.ginvy = (T)m.ginvy;
  c.by0 = (T)m.by0; c.binv = (T)m.binv;
  c.hull_safe = (T)(l / 2 * std::sqrt(2.0) + 1.0);
  c.fx0 = (T)m.fx0; c.fy0 = (T)m.fy0; c.finvx = (T)m.finvx; c.finvy = (T)m.finvy;
  c.el_cap = (T)el;
  c.fuel_me_a = (T)p.fuel_me_a; c.fuel_me_b = (T)p.fuel_me_b; c.fuel_me_c = (T)p.fuel_me_c;
  c.fuel_dg_a = (T)p.fuel_dg_a; c.fuel_dg_b = (T)p.fuel_dg_b; c.fuel_dg_c = (T)p.fuel_dg_c;
  c.rad2deg = (T)(180.0 / M_PI);
  // float64 thresholds and gains (knife-edge decisions; MSRL_env_ex.py:119, 554-603, 754, 829)
  c.x.los_r = p.lookahead_distance;
  c.x.windup = p.integrator_windup_limit;
  c.x.e_tol = p.e_tolerance;
  c.x.arrival = p.arrival_radius;
  c.x.rpm_max = p.shaft_rpm_max;
  c.x.min_dist = p.minimum_ship_distance;
  c.x.blackout = me / 1000;
  c.x.dt = p.integration_step;
  c.x.kp1 = p.kp_ship_speed; c.x.ki1 = p.ki_ship_speed;
  c.x.kp2 = p.kp_shaft_speed; c.x.ki2 = p.ki_shaft_speed;
  c.x.avail_prop = avail; c.x.me_cap = me; c.x.hotel = hotel; c.x.load_el_gen = std::min(hotel, el);
  c.x.bias_scale = p.bias_throttle_scale; c.x.bias_max = p.bias_throttle_max;
  c.x.half_len = l / 2;
  c.x.theta = p.theta;
  return c;
}

// bytes of the map blob the fused step kernels stage into LDS (SIT_LDS_CELLS)
size_t map_stage_bytes(const sit_handle* h) { return SIT_LDS_CELLS ? h->meta.map_bytes : h->meta.frank_off; }

template <typename T>
KArgs<T> make_args(const sit_handle* h) {
  KArgs<T> a{};
  a.c = make_consts<T>(h);
  a.n_env = h->n_env;
  a.cap = h->cap;
  auto fp = [&](int f) { return reinterpret_cast<T*>(h->blob + h->off[f]); };
  auto ip = [&](int f) { return reinterpret_cast<int32_t*>(h->blob + h->off[f]); };
  for (int i = 0; i < kShipReal; ++i) a.st.ship[i] = fp(F_NORTH + i);
  a.st.k = ip(F_K); a.st.nw = ip(F_NW); a.st.ticks = ip(F_TICKS); a.st.stop = ip(F_STOP);
  for (int i = 0; i < kEnvReal; ++i) a.st.env[i] = fp(F_SAMP + i);
  a.st.ep_step = ip(F_EP);
  a.st.event = reinterpret_cast<uint32_t*>(h->blob + h->off[F_EVENT]);
  a.st.episodes = reinterpret_cast<uint32_t*>(h->blob + h->off[F_EPISODES]);
  a.st.wn = fp(F_WN); a.st.we = fp(F_WE);
  a.st.last_obs = fp(F_LAST_OBS);
  for (int i = 0; i < 3; ++i) a.st.fuel[i] = fp(F_FUEL_ME + i);
  a.st.last_log = fp(F_LAST_LOG);
  a.st.iwk[0] = fp(F_IWK_N); a.st.iwk[1] = fp(F_IWK_E);
  a.st.iwk_flags = reinterpret_cast<uint32_t*>(h->blob + h->off[F_IWK_FLAGS]);
  for (int i = 0; i < kShipLo; ++i) a.st.ship_lo[i] = fp(F_SHIP_LO + i);
  for (int i = 0; i < kEnvLo; ++i) a.st.env_lo[i] = fp(F_ENV_LO + i);
  a.sc.init = reinterpret_cast<const T*>(h->scen + h->scen_init);
  a.sc.end_n = reinterpret_cast<const T*>(h->scen + h->scen_end_n);
  a.sc.end_e = reinterpret_cast<const T*>(h->scen + h->scen_end_e);
  a.sc.nw0 = reinterpret_cast<const int32_t*>(h->scen + h->scen_nw0);
  a.sc.ab_len = reinterpret_cast<const double*>(h->scen + h->scen_ab_len);
  a.sc.ab_alpha = reinterpret_cast<const double*>(h->scen + h->scen_ab_alpha);
  a.sc.initial_state = reinterpret_cast<const T*>(h->scen + h->scen_initial);
  a.sc.init_lo = reinterpret_cast<const T*>(h->scen + h->scen_init_lo);
  const MapMeta& m = h->meta;
  a.map.n_poly = m.n_poly;
  a.map.n_edge = m.n_vert;
  a.map.use_index = m.use_index;
  a.map.edge = reinterpret_cast<const Edge<T>*>(h->map);
  a.map.idx = reinterpret_cast<const uint16_t*>(h->map + m.idx_off);
  a.map.fine = reinterpret_cast<const uint32_t*>(h->map + m.fine_off);
  a.map.frank = reinterpret_cast<const uint16_t*>(h->map + m.frank_off);
  a.map.crec = reinterpret_cast<const uint2*>(h->map + m.crec_off);
  a.map.clive = reinterpret_cast<const uint8_t*>(h->map + m.clive_off);
  a.map.use_cells = m.use_cells;
  a.map.n_idx = (int32_t)m.n_idx;
  a.map.n_mixed = (int32_t)m.n_mixed;
  a.map.n_live = (int32_t)m.n_live;
  a.map.off = reinterpret_cast<const int32_t*>(h->map + m.ring_off);
  a.map.bbox = reinterpret_cast<const T*>(h->map + m.bbox_off);
  a.map_bytes = (int32_t)map_stage_bytes(h);
  return a;
}

// policy-mode admission scratch: [n_groups][kAgeBuckets] counts, [n_groups][2] plan, header
int32_t* admit_counts(const sit_handle* h) { return reinterpret_cast<int32_t*>(h->scen + h->scen_admit); }
// in-kernel serving's fallback queue (logged launches run the one-wave kernel): capacity n_env
struct ServeQueue {
  int32_t* env;
  int32_t* age;
  int32_t* count;
  void* obs;
  void* noise;
};
ServeQueue serve_queue(const sit_handle* h) {
  unsigned char* b = h->scen + h->scen_serve;
  const size_t n = (size_t)h->n_env;
  const ServeLayout L = serve_layout(h);
  ServeQueue q;
  q.env = reinterpret_cast<int32_t*>(b);
  q.age = q.env + n;
  q.count = q.age + n;
  q.obs = b + L.obs;
  q.noise = b + L.noise;
  return q;
}

int ready(sit_handle* h) {
  if (!h) return fail(nullptr, SIT_E_INVALID, "null handle");
  if (!h->have_map) return fail(h, SIT_E_STATE, "sit_load_map has not been called");
  if (!h->have_routes) return fail(h, SIT_E_STATE, "sit_load_routes has not been called");
  if (!h->have_init) return fail(h, SIT_E_STATE, "sit_load_initial has not been called");
  return SIT_OK;
}

// LDS budget of one step-kernel block: two blocks (4 waves, one per SIMD) must fit the CU's
// 160 KB; above 80 KB only one block fits and the grid runs in two rounds (~1.75x slower)
constexpr size_t kLdsBudget = 80 * 1024;
constexpr size_t kLdsCu = 160 * 1024;       // the CU's LDS (k_env_steps_sync: two 256-thread blocks per CU)
// launches of fewer steps read the map through the caches instead of staging it into LDS: staging
// 57 KB per block is a prologue that a single step (sit_step, the scalar drop-in) cannot amortise
#ifndef SIT_LDS_MIN_STEPS
#define SIT_LDS_MIN_STEPS 8
#endif
constexpr int kLdsMinSteps = SIT_LDS_MIN_STEPS;
size_t map_lds_bytes(const sit_handle* h) { return (map_stage_bytes(h) + 255) & ~size_t(255); }

// the step kernel of a launch as a readable instantiation name (sit_step_kernel)
template <typename T>
void set_kernel_name(sit_handle* h, bool sync, int mode, bool lds, bool log, int mach) {
  static const char* const modes[3] = {"kExplicit", "kSynth", "kPolicy"};
  const char* t = kIsF32<T> ? "float" : "double";
  if (sync) snprintf(h->last_kernel, sizeof(h->last_kernel), "k_env_steps_sync<%s,%s,%s,MACH=%d>", t, modes[mode],
                     lds ? "map=LDS" : "map=global", mach);
  else snprintf(h->last_kernel, sizeof(h->last_kernel), "k_env_steps<%s,%s,%s,%s,MACH=%d>", t, modes[mode],
                lds ? "map=LDS" : "map=global", log ? "log" : "nolog", mach);
}

// the launch's k_env_steps_sync map placement and dynamic LDS (0: the launch takes k_env_steps);
// *attr: the kernel's dynamic-LDS attribute (policy mode: the in-kernel serving size, whether or not
// the launch serves, so one attribute covers both)
template <typename T>
size_t sync_launch_lds(const sit_handle* h, const StepIO<T>& io, bool* lds_map, size_t* attr) {
  const bool sync_lds = h->lds_map_sel == 1 || (h->lds_map_sel < 0 && io.n_steps >= kLdsMinSteps);
  const size_t map = sync_lds ? map_stage_bytes(h) : 0;
  const bool policy = io.policy_action && !io.action_ne;
  const size_t lds = io.actor_w ? serve_lds_bytes<T>(map)
                     : policy   ? sync_lds_bytes<T, kPolicy>(map)
                     : io.action_ne ? sync_lds_bytes<T, kExplicit>(map) : sync_lds_bytes<T, kSynth>(map);
  const size_t at_serve = (policy ? serve_lds_bytes<T>(map) : lds) + SIT_DYN_OFF;
  const size_t at = at_serve + sizeof(Consts<T>) + 256 <= kLdsCu ? at_serve : lds + SIT_DYN_OFF;
  if (lds_map) *lds_map = sync_lds;
  if (attr) *attr = at;
  // (the fit check on the LDS the launch uses: a queue-path policy launch is not refused for serving LDS)
  if (h->kernel_classic || io.log || !h->meta.use_index || lds + SIT_DYN_OFF + sizeof(Consts<T>) + 256 > kLdsCu) return 0;
  return lds + SIT_DYN_OFF;
}

template <typename T>
int launch_steps(sit_handle* h, const StepIO<T>& io, hipStream_t stream) {
  KArgs<T> a = make_args<T>(h);
  a.io = io;
  const int mode = io.action_ne ? kExplicit : (io.policy_action ? kPolicy : kSynth);
  const int mach = a.c.mach_simpl ? 1 : 0;
  if (io.actor_w && mode != kPolicy) return fail(h, SIT_E_INVALID, "in-kernel serving needs policy mode");
  // k_env_steps_sync (sit_sync.h), two waves per ship with the map predicates on their own wave, for
  // every launch without the trajectory log: synthetic sampler (C3/C4), policy (C5) and explicit
  // actions (sit_step, the drop-in MultiShipRLEnv.step).  k_env_steps (one wave per ship) runs the
  // logged launches, and every launch under SIT_STEP_KERNEL=classic.  The sync kernel stages the map
  // into LDS for fused launches; single-step launches read it through the caches.
  bool sync_lds = false;
  size_t lds_attr = 0;
  const size_t lds_sync = sync_launch_lds<T>(h, io, &sync_lds, &lds_attr);
  if (lds_sync > 0) {
    const void* kern = nullptr;
    auto pick = [&](auto mode_tag, auto mach_tag, auto lds_tag) {
      constexpr int M = decltype(mode_tag)::value, K = decltype(mach_tag)::value;
      constexpr bool L = decltype(lds_tag)::value;
      kern = reinterpret_cast<const void*>(&k_env_steps_sync<T, M, K, L>);
    };
    auto pick_lds = [&](auto mode_tag, auto mach_tag) {
      if (sync_lds) pick(mode_tag, mach_tag, std::true_type{});
      else pick(mode_tag, mach_tag, std::false_type{});
    };
    auto pick_mach = [&](auto mode_tag) {
      if (mach) pick_lds(mode_tag, std::integral_constant<int, 1>{});
      else pick_lds(mode_tag, std::integral_constant<int, 0>{});
    };
    if (mode == kPolicy) pick_mach(std::integral_constant<int, kPolicy>{});
    else if (mode == kSynth) pick_mach(std::integral_constant<int, kSynth>{});
    else pick_mach(std::integral_constant<int, kExplicit>{});
    const int slot = ((mode * 2 + mach) * 2) + (sync_lds ? 1 : 0);
    if (h->lds_attr_sync[slot] != (int)lds_attr) {
      HIP_TRY(h, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_attr));
      h->lds_attr_sync[slot] = (int)lds_attr;
    }
    const int blocks = (h->n_env + kSyncLanes - 1) / kSyncLanes;
    a.lds_bytes = (int32_t)(lds_sync - SIT_DYN_OFF);
    a.fake_simds = h->fake_simds;
    void* args[] = {&a};
    HIP_TRY(h, hipLaunchKernel(kern, dim3(blocks), dim3(256), args, lds_sync, stream));
    set_kernel_name<T>(h, true, mode, sync_lds, false, mach);
    return SIT_OK;
  }
  if (io.actor_w) return fail(h, SIT_E_INVALID, "in-kernel serving runs on k_env_steps_sync only");
  const int blocks = (h->n_env + kEnvsPerBlock * kGroups - 1) / (kEnvsPerBlock * kGroups);
  // the map (edges, index, classes) is staged in LDS when it fits the budget next to the static
  // exchange buffers and the launch has enough steps to amortise the staging; otherwise the
  // predicates read it through the caches
  const size_t stat = sizeof(Xchg<T>) * 2 * kGroups + sizeof(Consts<T>) + 256;
  const bool fits = map_lds_bytes(h) + stat <= kLdsBudget;
  const bool lds_map = fits && (h->lds_map_sel == 1 || (h->lds_map_sel < 0 && io.n_steps >= kLdsMinSteps));
  const size_t lds = lds_map ? map_lds_bytes(h) : 0;
  auto go = [&](auto kern) -> int {
    // the dynamic-LDS attribute is set once per kernel and size (not per launch: launches may be
    // captured into HIP graphs)
    const int slot = ((mode * 2 + (lds_map ? 1 : 0)) * 2 + (io.log ? 1 : 0)) * 2 + mach;
    if (lds_map && h->lds_attr[slot] != (int)lds) {
      HIP_TRY(h, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      h->lds_attr[slot] = (int)lds;
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(128 * kGroups), lds, stream, a);
    return SIT_OK;
  };
  auto pick_mach = [&](auto mode_tag, auto mach_tag) -> int {
    constexpr int M = decltype(mode_tag)::value, K = decltype(mach_tag)::value;
    if (io.log) return lds_map ? go(k_env_steps<T, M, true, true, K>) : go(k_env_steps<T, M, false, true, K>);
    return lds_map ? go(k_env_steps<T, M, true, false, K>) : go(k_env_steps<T, M, false, false, K>);
  };
  auto pick = [&](auto mode_tag) -> int {
    if (mach) return pick_mach(mode_tag, std::integral_constant<int, 1>{});
    return pick_mach(mode_tag, std::integral_constant<int, 0>{});
  };
  int rc;
  if (mode == kSynth) rc = pick(std::integral_constant<int, kSynth>{});
  else if (mode == kPolicy) rc = pick(std::integral_constant<int, kPolicy>{});
  else rc = pick(std::integral_constant<int, kExplicit>{});
  if (rc) return rc;
  HIP_TRY(h, hipGetLastError());
  set_kernel_name<T>(h, false, mode, lds_map, io.log != nullptr, mach);
  return SIT_OK;
}

template <typename T>
int launch_probe(sit_handle* h, int n, const void* pts_ne, void* dist, uint8_t* inside, uint8_t* hull,
                 hipStream_t stream) {
  const KArgs<T> a = make_args<T>(h);
  const int blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_probe_map<T>, dim3(blocks), dim3(256), 0, stream, a, n, (const T*)pts_ne, (T*)dist,
                     inside, hull);
  HIP_TRY(h, hipGetLastError());
  return SIT_OK;
}

int launch_selftest(int op, int n, const double* a, const double* b, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(k_selftest_f64, dim3((n + 255) / 256), dim3(256), 0, stream, op, n, a, b, out);
  return hipGetLastError() == hipSuccess ? SIT_OK : SIT_E_HIP;
}

}  // namespace

