/*
 * sit.h — C ABI of the MI355X-native ship-in-transit (SIT) environment step.
 *
 * This is the drop-in boundary for the one hot path of AndreasKing-Goks/sac-maritime-ast:
 * the two-ship `MultiShipRLEnv` (RLEnv/MSRL_Env.py:37-450, completed by
 * RLEnv/MSRL_env_ex.py:450-980) stepping the ship-in-transit simulator
 * (the simulators/ship_in_transit package).  One handle holds N independent two-ship
 * environments ("envs"): ship type 0 is the ship under test, type 1 the obstacle
 * ship whose route the AST sampler perturbs with intermediate waypoints (IWs).
 *
 * Conventions
 *  - Plain C types only; no HIP/torch types cross the boundary.  `stream` is a
 *    hipStream_t passed as void* (NULL = default stream).
 *  - "real" below means float32 when the handle was created with SIT_F32 and
 *    float64 with SIT_F64.  Every per-step array argument is a DEVICE pointer
 *    owned by the caller; setup calls (sit_load_*) take HOST pointers.
 *  - Every entry point returns SIT_OK (0) or a negative SIT_E_* code; the message
 *    is available from sit_last_error().  No exception crosses the ABI.
 *  - Calls are stream-ordered and asynchronous.  A handle must not be used from two
 *    host threads at once; independent handles (one per GPU/stream) are independent.
 *
 * Reference interface each entry point replaces (file:line in the reference):
 *   sit_create / sit_load_*   MultiShipRLEnv.__init__ + ShipAssets    MSRL_Env.py:25-116,
 *                             ShipModelAST/ShipMachineryModel/controllers constructors
 *                             (ship_model.py:563-574, ship_engine.py:298-353,
 *                              controllers.py:114-136, 253-296), PolygonObstacle obstacle.py:98-124
 *   sit_reset                 MultiShipRLEnv.reset                    MSRL_Env.py:147-188
 *   sit_init_step             MultiShipRLEnv.init_step                MSRL_Env.py:190-217
 *   sit_step                  MultiShipRLEnv.step                     MSRL_Env.py:404-442
 *                             (+ reward_function                      MSRL_env_ex.py:906-980)
 *   sit_rollout               K x step with the driver loop of test_beds/main_ast.py:310-412
 *                             (the consumer ast_core/samplers/intermediate_waypoint_sampler.py
 *                              is empty in the reference; the synthetic sampler is SURVEY §8(d))
 *   sit_get_state/set_state   (no reference counterpart: SoA export/import for teacher-forced
 *                              parity and checkpointing)
 */
#ifndef SIT_H
#define SIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIT_ABI_VERSION 1

/* ---- return codes ---------------------------------------------------------------- */
#define SIT_OK 0
#define SIT_E_INVALID (-1)   /* bad argument (null pointer, out-of-range size, ...) */
#define SIT_E_HIP (-2)       /* a HIP runtime call failed */
#define SIT_E_NOMEM (-3)     /* device allocation failed */
#define SIT_E_STATE (-4)     /* call out of order (e.g. stepping before routes are loaded) */

/* ---- precision of a handle -------------------------------------------------------- */
#define SIT_F32 32
#define SIT_F64 64

/* ---- hybrid shaft generator state (ship_engine.py:32-76) --------------------------- */
#define SIT_SG_MOTOR 0 /* 'MOTOR' (PTI)  */
#define SIT_SG_GEN 1   /* 'GEN'   (PTO)  */
#define SIT_SG_OFF 2   /* anything else  */

/* ---- machinery model (sit_params.machinery_model) ---------------------------------- */
#define SIT_MACH_SHAFT 0      /* ShipMachineryModel: shaft speed ODE, thrust = k D^4 w|w| (ship_engine.py:298-395) */
#define SIT_MACH_SIMPLIFIED 1 /* SimplifiedMachineryModel: first-order thrust-force lag (ship_engine.py:398-433)
                               * with ThrottleFromSpeedSetPointSimplifiedPropulsion (controllers.py:154-172);
                               * the shaft_speed state holds the thrust force [N], see sit_params */

/* ---- status bitmask: one bit per reference status string, in the order the
 *      reference concatenates them (MSRL_env_ex.py:755-803, 830-874, 897-899) ------- */
#define SIT_ST_TEST_ENDPOINT (1u << 0)   /* "|Test ship reaches endpoint|"             */
#define SIT_ST_TEST_HORIZON (1u << 1)    /* "|Test ship hits map horizon|"             */
#define SIT_ST_TEST_TERRAIN (1u << 2)    /* "|Test ship collides with the terrain|"    */
#define SIT_ST_TEST_MECHANICAL (1u << 3) /* "|Test ship mechanical failure|"           */
#define SIT_ST_TEST_NAVIGATION (1u << 4) /* "|Test ship navigation failure|"           */
#define SIT_ST_TEST_BLACKOUT (1u << 5)   /* "|Test ship blackout failure|"             */
#define SIT_ST_OBS_ENDPOINT (1u << 6)    /* "|Obstacle ship reaches endpoint|"         */
#define SIT_ST_OBS_HORIZON (1u << 7)     /* "|Obstacle ship hits map horizon|"         */
#define SIT_ST_OBS_TERRAIN (1u << 8)     /* "|Obstacle ship collides with the terrain|"*/
#define SIT_ST_OBS_IW_TERMINAL (1u << 9) /* "|Obstacle ship IW sampled in terminal state|" */
#define SIT_ST_OBS_NAVIGATION (1u << 10) /* "|Obstacle ship navigation failure|"       */
#define SIT_ST_COLLISION (1u << 11)      /* "|Ship collision|"                         */
#define SIT_ST_TEST_DONE (1u << 12)      /* test ship terminal  (else "|Test ship not in terminal state|")     */
#define SIT_ST_OBS_DONE (1u << 13)       /* obstacle ship terminal (else "|Obstacle ship not in terminal state|") */
#define SIT_ST_NO_STEP (1u << 30)        /* policy mode: the env waited for its action; no step taken in this row */
#define SIT_ST_ROUTE_OVERFLOW (1u << 31) /* IW insertion dropped: route table full (no reference counterpart) */

/* ---- next_state layout (MSRL_Env.py:426-437) --------------------------------------- */
#define SIT_OBS_DIM 10 /* test n,e,psi,rpm,|e_ct|,P_me[kW], obs n,e,psi,|e_ct| */
/* ---- replay transition record (memory.push, test_beds/main_ast.py:385-396) ----------
 *   [0:10] state (the observation before the step; reset()'s array at an episode start)
 *   [10] action: the SAC action of the event in [-1, 1] (the route angle a = action * pi/6; the
 *        synthetic sampler's U[-1, 1] draw or the policy's squashed action; NaN in explicit mode),
 *   [11] reward, [12:22] next_state,
 *   [22] mask (1 if the episode step reaches mask_horizon, else not done), [23] env id */
#define SIT_TRANSITION_DIM 24
/* Trajectory log rows per env and step (sit_rollout_args.log): ShipModelAST.store_simulation_data's
 * 27 keys (ship_model.py:645-684, in that order: time [s], north/east position [m], yaw angle
 * [deg], rudder angle [deg], forward/sideways speed [m/s], yaw rate [deg/sec], propeller shaft
 * speed [rpm], commanded load fraction me/hsg [-], power me [kw], available power me [kw], power
 * electrical [kw], available power electrical [kw], power [kw], propulsion power [kw], fuel
 * rate me/hsg/total [kg/s], fuel consumption me/hsg/total [kg], motor torque [Nm], thrust force
 * [kN], cross track error [m], heading error [deg] (radians, as the reference stores it)) for
 * the ship under test (rows 0-26) and the obstacle ship (rows 27-53), then the 8 per-step terms
 * whose per-episode sums are MultiShipRLEnv.reward_results (MSRL_env_ex.py:926-964): test
 * reward_e_ct, reward_near_col, total_non_terminal; obstacle reward_base, reward_e_ct,
 * reward_near_col, total_non_terminal; shared total_non_terminal (rows 54-61). */
#define SIT_LOG_KEYS 27
#define SIT_LOG_ROWS 62

/* ---- per-ship initial values for sit_load_initial ---------------------------------- */
enum {
  SIT_INIT_NORTH = 0,      /* SimulationConfiguration.initial_north_position_m           */
  SIT_INIT_EAST,           /* initial_east_position_m                                    */
  SIT_INIT_YAW,            /* initial_yaw_angle_rad                                      */
  SIT_INIT_SURGE,          /* initial_forward_speed_m_per_s                              */
  SIT_INIT_SWAY,           /* initial_sideways_speed_m_per_s                             */
  SIT_INIT_YAW_RATE,       /* initial_yaw_rate_rad_per_s                                 */
  SIT_INIT_SHAFT_SPEED,    /* initial_propeller_shaft_speed_rad_per_s (ship_model.py:567) */
  SIT_INIT_DESIRED_SPEED,  /* ShipAssets.desired_forward_speed (MSRL_Env.py:30)           */
  SIT_INIT_SHIP_SPEED_I,   /* ship-speed PI initial integral (controllers.py:122-124: 0)  */
  SIT_INIT_SHAFT_SPEED_I,  /* initial_shaft_speed_integral_error (controllers.py:119, 129) */
  SIT_INIT_NF
};

/* ---- configuration: the reference's NamedTuple fields, verbatim ------------------- */
typedef struct sit_params {
  /* ShipConfiguration (ship_model.py:20-35) */
  double dead_weight_tonnage;
  double coefficient_of_deadweight_to_displacement;
  double bunkers;
  double ballast;
  double length_of_ship;
  double width_of_ship;
  double added_mass_coefficient_in_surge;
  double added_mass_coefficient_in_sway;
  double added_mass_coefficient_in_yaw;
  double mass_over_linear_friction_coefficient_in_surge;
  double mass_over_linear_friction_coefficient_in_sway;
  double mass_over_linear_friction_coefficient_in_yaw;
  double nonlinear_friction_coefficient_in_surge;
  double nonlinear_friction_coefficient_in_sway;
  double nonlinear_friction_coefficient_in_yaw;
  /* EnvironmentConfiguration (ship_model.py:38-42) */
  double current_velocity_component_from_north;
  double current_velocity_component_from_east;
  double wind_speed;
  double wind_direction;
  /* wind model constants hard-coded in BaseShipModel (ship_model.py:123-130) */
  double rho_air;
  double front_height;
  double side_height;
  double cx;
  double cy;
  double cn;
  /* SimulationConfiguration.integration_step (ship_model.py:52) */
  double integration_step;
  /* MachinerySystemConfiguration (ship_engine.py:121-138) and the selected MachineryMode */
  double hotel_load;
  double main_engine_capacity;   /* MachineryModeParams of the operating mode */
  double electrical_capacity;
  int32_t shaft_generator_state; /* SIT_SG_* */
  int32_t machinery_model;       /* SIT_MACH_* (0 = the reference's ShipModelAST machinery)  */
  double rated_speed_main_engine_rpm;
  double linear_friction_main_engine;
  double linear_friction_hybrid_shaft_generator;
  double gear_ratio_between_main_engine_and_propeller;
  double gear_ratio_between_hybrid_shaft_generator_and_propeller;
  double propeller_inertia;
  double propeller_speed_to_torque_coefficient;
  double propeller_diameter;
  double propeller_speed_to_thrust_force_coefficient;
  double rudder_angle_to_sway_force_coefficient;
  double rudder_angle_to_yaw_force_coefficient;
  double max_rudder_angle_degrees;
  /* ThrottleControllerGains (controllers.py:16-20) */
  double kp_ship_speed;
  double ki_ship_speed;
  double kp_shaft_speed;
  double ki_shaft_speed;
  /* HeadingControllerGains (controllers.py:23-26) */
  double heading_kp;
  double heading_kd;
  double heading_ki;
  /* LosParameters (LOS_guidance.py:15-19) */
  double radius_of_acceptance;
  double lookahead_distance;
  double los_integral_gain;
  double integrator_windup_limit;
  /* env args (test_policy.py:39-42) and reward constants of MSRL_env_ex.py */
  double theta;                  /* navigation-failure coefficient (:569)      */
  int32_t sampling_frequency;    /* AB segment divisor (:125)                  */
  int32_t collision_bias;        /* 1 = reference behaviour: always on (MSRL_Env.py:98-99, 242) */
  double e_tolerance;            /* 1000 (:119)                                */
  double arrival_radius;         /* 200  (:754, :829)                          */
  double shaft_rpm_max;          /* 2000 (:557)                                */
  double minimum_ship_distance;  /* 50   (:592)                                */
  double bias_throttle_scale;    /* 0.5  (MSRL_Env.py:246)                     */
  double bias_throttle_max;      /* 1.1  (MSRL_Env.py:247)                     */
  double bias_rudder_degrees;    /* 3    (MSRL_Env.py:250)                     */
  /* specific fuel consumption a x^2 + b x + c [g/kWh] of the main engine and the diesel
   * generators (MachinerySystemConfiguration, ship_engine.py:137-138, 89-115; test_policy.py:
   * 162-163): logging only (trajectory log, fuel keys) */
  double fuel_me_a, fuel_me_b, fuel_me_c;
  double fuel_dg_a, fuel_dg_b, fuel_dg_c;
  /* SIT_MACH_SIMPLIFIED only (SimplifiedPropulsionMachinerySystemConfiguration, ship_engine.py:
   * 148-157): thrust_force_dynamic_time_constant [s].  In that mode the ship-speed PI gains
   * kp_ship_speed / ki_ship_speed are ThrottleFromSpeedSetPointSimplifiedPropulsion's kp / ki
   * (throttle saturated to [0, 1.1]), the shaft-speed PI is unused, the shaft_speed state and
   * SIT_INIT_SHAFT_SPEED hold the thrust force [N] (initial_thrust_force), and the observed shaft
   * speed is 0 (the model has no shaft, so no mechanical failure). */
  double thrust_force_dynamic_time_constant;
} sit_params;

/* Fill `p` with the configuration of test_beds/test_policy.py:94-226 (PTI mode). */
void sit_params_default(sit_params* p);
/* sizeof(sit_params) as compiled into the library (binding layout check). */
size_t sit_params_size(void);

/* ---- handle lifecycle ------------------------------------------------------------- */
typedef struct sit_handle sit_handle;

/* Create N envs on the current HIP device.  `wpt_capacity` bounds the waypoints of one
 * ship's route including start and end (IW insertions beyond it set
 * SIT_ST_ROUTE_OVERFLOW and are dropped).  `precision` is SIT_F32 or SIT_F64. */
int sit_create(const sit_params* p, int32_t n_env, int32_t wpt_capacity, int32_t precision,
               sit_handle** out);
void sit_destroy(sit_handle* h);
/* Last error message of `h`, or of the failed sit_create on this thread when h == NULL. */
const char* sit_last_error(const sit_handle* h);
int32_t sit_abi_version(void);
int32_t sit_precision(const sit_handle* h);
int32_t sit_n_env(const sit_handle* h);
/* Instantiation name of the step kernel the last sit_step / sit_rollout launch of `h` ran, e.g.
 * "k_env_steps_sync<float,kSynth,MACH=0>" (diagnostics and bench labels; "" before the first). */
const char* sit_step_kernel(const sit_handle* h);

/* ---- setup (host pointers) --------------------------------------------------------- */
/* Island map: PolygonObstacle(list_of_vertices_list) (obstacle.py:98-124).  Vertices are
 * (east, north) pairs exactly as in the reference; polygon p owns vertices
 * [vert_offsets[p], vert_offsets[p+1]).  The ring is closed implicitly. */
int sit_load_map(sit_handle* h, int32_t n_poly, const int32_t* vert_offsets,
                 const double* verts_en);
/* Routes: wpt_ne[env][ship][i][2] = (north, east) for i < n_wpt[env][ship], laid out with
 * stride wpt_capacity in i (NavigationSystem.load_waypoints, LOS_guidance.py:65-86). */
int sit_load_routes(sit_handle* h, const double* wpt_ne, const int32_t* n_wpt);
/* Construction-time values: init[env][ship][SIT_INIT_NF]. */
int sit_load_initial(sit_handle* h, const double* init);
/* Spatial-index statistics of the loaded map (diagnostics; no reference counterpart):
 * info[0] bytes of the map blob staged into LDS per step-kernel block, [1] mixed class cells
 * with a point-in-polygon record, [2] live edge entries of those records, [3] nearest-edge
 * grid and bands in use, [4] cell records in use, [5] LDS bytes per block for the map.
 * Writes min(n, 6) values. */
int sit_map_info(const sit_handle* h, int64_t* info, int32_t n);
/* The step kernel's map predicates at arbitrary points (test/diagnostic entry; the reference
 * counterparts are PolygonObstacle.obstacles_distance / Polygon.contains / is_pos_inside_obstacles,
 * obstacle.py:126-141, MSRL_env_ex.py:490-515), through the same spatial index:
 *   pts_ne real[n][2] (north, east); dist real[n] boundary distance; inside u8[n] point strictly
 *   inside a polygon; hull u8[n] any hull corner (+-l/2) inside.  Device pointers; any output may
 *   be NULL. */
int sit_probe_map(sit_handle* h, int32_t n, const void* pts_ne, void* dist, uint8_t* inside,
                  uint8_t* hull, void* stream);
/* Self-test of the IEEE float64 helpers the knife-edge decisions use (diagnostic; no reference
 * counterpart): out[i] = op(a[i], b[i]) with op 0 a / b, 1 sqrt(a), 2 a*a + b*b, 3 (a + b) - a,
 * 4 a*b + b*a (each correctly rounded per operation, as numpy's float64), 5 sin(a), 6 cos(a),
 * 7 atan2(a, b) (the device math library the float64 path uses), 8 the fused step kernel's wave
 * roles (sync_role_of) for the SIMD assignment a (base 4, digit v = SIMD of wave v) and CU ticket b,
 * packed as role of wave v in base-4 digit v, 9 / 10 sin / cos of (float)a as the float32 step takes
 * them (xsincos), 11 atan((float)a), 12 atan2((float)a, (float)b) in float32, each widened to
 * float64.  fast_tu != 0 runs the copy compiled with the float32
 * step kernels' fast-math flags.  Device pointers. */
int sit_selftest_f64(int32_t op, int32_t n, const double* a, const double* b, double* out, int32_t fast_tu,
                     void* stream);
/* Debug builds (libsit_debug.so, compiled with -DSIT_DEBUG; no reference counterpart): every table
 * index the step kernels compute is bounds-checked; a failed check sets bit i of the returned word
 * (0 route-table row, 1 next-waypoint index, 2 route length, 3 spatial-index entry or range, 4 edge
 * id, 5 class-grid word, 6 mixed-cell record or live-edge range, 7 in-kernel serving: a block's
 * published request count outside [0, 64] or its LDS past the launch's dynamic LDS, 8 in-kernel
 * serving: a served env id outside [0, n_env)), and every table read or write it guards is
 * clamped into its table (indices to a valid entry, ranges to their in-table part; the next-waypoint
 * and route-length checks guard the route-table rows of bit 0), so the launch completes without an
 * out-of-bounds access.  sit_debug_flags synchronises the device, returns the bits set since the last
 * call and clears them; release builds return 0.  sit_debug_build: 1 in a debug build. */
int sit_debug_flags(uint32_t* flags);
int32_t sit_debug_build(void);
/* Placement record of the fused two-wave step kernel (no reference counterpart): the number of
 * blocks, since the last reset, whose four waves did not sit on four different SIMDs.  Roles are a
 * permutation of D0, D1, P0, P1 for every placement (results never depend on it); the count shows
 * how often the issue-priority pairing the kernel is tuned for was not available.  Synchronises the
 * device; reset != 0 clears the count. */
int sit_role_fallbacks(uint64_t* count, int32_t reset);
/* Put every env into its construction-time state (as if freshly built).  Unlike
 * sit_reset this also re-initialises the shaft speed and all controller integrators. */
int sit_restart(sit_handle* h, void* stream);

/* ---- stepping (device pointers, stream-ordered) ------------------------------------ */
/* MultiShipRLEnv.reset for envs with env_mask[e] != 0 (NULL = all).  Keeps shaft speed and
 * all PI/PID integrator states, as the reference does.  If initial_state is not NULL it
 * receives the construction-time observation of every env, real[n_env][SIT_OBS_DIM]. */
int sit_reset(sit_handle* h, const uint8_t* env_mask, void* initial_state, void* stream);
/* MultiShipRLEnv.init_step for masked envs (NULL = all). */
int sit_init_step(sit_handle* h, const uint8_t* env_mask, void* stream);
/* MultiShipRLEnv.step for all envs.
 *   action_ne  real[n_env][2]  converted_action = intermediate waypoint (north, east)
 *   sac_update u8[n_env]       SAC_update: insert the IW into the obstacle ship's route
 *   init       u8[n_env]       init: first step of an episode (no distance accounting)
 *   next_state real[n_env][SIT_OBS_DIM], reward real[n_env], done u8[n_env], status u32[n_env]
 *   done_count int32[1] or NULL: += number of envs with done (wave ballot reduction)
 * next_state (and action_out below) must be aligned to 2 reals (SIT_E_INVALID otherwise). */
int sit_step(sit_handle* h, const void* action_ne, const uint8_t* sac_update,
             const uint8_t* init, void* next_state, void* reward, uint8_t* done,
             uint32_t* status, int32_t* done_count, void* stream);
/* MultiShipRLEnv.step with HOST arrays (the scalar drop-in, compat.MultiShipRLEnv.step; the reference
 * API is synchronous): the same step as sit_step, with the arrays above in host memory and
 *   log   real[SIT_LOG_ROWS][n_env] or NULL: the step's trajectory-log row (sit_rollout_args.log)
 *   state sit_state_bytes() bytes or NULL: the state blob after the step (sit_get_state)
 * The inputs go into the handle's pinned, coherent host staging, which the step kernel reads and
 * writes directly (no copy call); one launch, one copy of the state blob when asked, one
 * synchronisation of `stream`, then the outputs are copied to the caller's arrays.  Any output may be
 * NULL.  Returns after the step has completed. */
int sit_step_host(sit_handle* h, const void* action_ne, const uint8_t* sac_update, const uint8_t* init,
                  void* next_state, void* reward, uint8_t* done, uint32_t* status, void* log, void* state,
                  void* stream);

/* K fused steps.  With action_ne == NULL the synthetic AST sampler drives the obstacle
 * ship: a sampling event happens on the first step of an episode and
 * whenever the obstacle ship's sampling distance reaches AB_len; it draws
 * a ~ U[-pi/6, pi/6] from Philox4x32-10(key = seed, counter = (env_id, event, 0x5A4D, 0))
 * and inserts IW = (n + AB_len cos(AB_alpha + a), e + AB_len sin(AB_alpha + a)).
 * Otherwise action_ne/sac_update/init are [n_steps][n_env] explicit inputs.
 * With auto_reset != 0, an env whose step returned done is reset, init-stepped and
 * restarted at episode step 1 before its next step (test_beds/main_ast.py:310-330).
 * Output arrays are [n_steps][n_env]...; any may be NULL except that at least one of
 * next_state/reward must be given.  action_out (real[n_steps][n_env][4]) receives
 * (IW north, IW east, scoping angle a, SAC_update) of every step. */
typedef struct sit_rollout_args {
  int32_t n_steps;
  int32_t auto_reset;
  uint64_t seed;
  int64_t env_id_offset;     /* global id of env 0 (for sharding across GPUs) */
  const void* action_ne;     /* real[n_steps][n_env][2] or NULL (synthetic sampler) */
  const uint8_t* sac_update; /* u8[n_steps][n_env] (explicit mode only) */
  const uint8_t* init;       /* u8[n_steps][n_env] (explicit mode only) */
  void* next_state;          /* real[n_steps][n_env][SIT_OBS_DIM] or NULL */
  void* reward;              /* real[n_steps][n_env] or NULL */
  uint8_t* done;             /* u8[n_steps][n_env] or NULL */
  uint32_t* status;          /* u32[n_steps][n_env] or NULL */
  void* action_out;          /* real[n_steps][n_env][4] or NULL */
  int32_t* done_count;       /* int32[n_steps] or NULL: += envs done at each step */
  /* sampling-event transitions (synthetic sampler mode): one record per step whose
   * SAC_update is set, appended at transition_count (atomic); records beyond
   * transition_capacity are counted but not written */
  void* transitions;          /* real[transition_capacity][SIT_TRANSITION_DIM] or NULL, 4-real aligned */
  int32_t* transition_count;  /* int32[1] */
  int32_t transition_capacity;
  int32_t mask_horizon;       /* args.num_steps_episode (main_ast.py:71, 387); 0 = none */
  /* Policy mode (action_ne == NULL, policy_action != NULL): the actions of sampling events come
   * from a policy evaluated between launches (the SAC actor, agent.select_action mode 1,
   * main_ast.py:344-349).  At a sampling event an env consumes policy_action[e] if
   * policy_ready[e] == SIT_POLICY_READY (route angle a = policy_action[e] * pi/6, IW as in the
   * synthetic sampler); otherwise it takes no further step in this launch (its rows get status
   * SIT_ST_NO_STEP and done 0).  At the end of the launch policy_ready[e] is SIT_POLICY_WAITING
   * for every env stopped at a sampling event, SIT_POLICY_READY for an env holding an unused
   * action, else 0.
   * Admission (after the step kernel, same call, same stream; deterministic): the waiting envs
   * enter the request queue oldest request first, ties by env id, at most request_capacity of
   * them; request_age[e] counts the admission rounds env e has waited (kept by the library,
   * zero-initialised by the caller).  An env that starts waiting in launch L is admitted at the
   * latest in round L + ceil(n_env / request_capacity) - 1 (exact while ceil(n_env / request_capacity) < 16).  The
   * queue rows are in env-id order: request_env[q] = e, request_obs[q] = the observation the env
   * waits at (state field last_obs), request_noise[q] = N(0,1) from Philox4x32-10(key = seed,
   * counter = (env_id, event, 0x504F, 0)) (Box-Muller), *request_count = rows.  Which envs step
   * how many rows is therefore a function of (scenario, seed, request_capacity, n_steps, actions),
   * never of scheduling.  The caller runs the policy on the queue and writes policy_action /
   * policy_ready = SIT_POLICY_READY for the queued envs before the next launch (sit_policy_actor
   * does both).  Per-env trajectories equal those of a synchronous per-step loop. */
  const void* policy_action;  /* real[n_env] in [-1, 1] */
  int32_t* policy_ready;      /* int32[n_env]: 0, SIT_POLICY_READY or SIT_POLICY_WAITING */
  int32_t* request_env;       /* int32[request_capacity] */
  void* request_noise;        /* real[request_capacity] */
  void* request_obs;          /* real[request_capacity][SIT_OBS_DIM]: the waiting env's state */
  int32_t* request_count;     /* int32[1] */
  int32_t request_capacity;
  int64_t* env_steps;         /* int64[1] or NULL: += env-steps executed (policy mode) */
  /* Trajectory log (optional): real[n_steps][SIT_LOG_ROWS][n_env].  The obstacle ship's stop
   * path repeats its last logged row with the time updated (store_last_simulation_data), and
   * the fuel consumption accumulates over logged steps only (logging-only quantities). */
  void* log;
  int32_t* request_age;       /* int32[n_env] (policy mode): admission rounds waited, see above */
  /* In-kernel serving (policy mode, optional).  With actor_weights != NULL the launch evaluates the
   * actor itself — sit_policy_actor's network, weight layout and head, in float32, on the observation
   * each env waits at and its event's normal draw (as request_obs / request_noise above) — for every
   * env that ends the launch waiting, at the end of the same launch: policy_action[e] = its squashed
   * action, policy_ready[e] = SIT_POLICY_READY (never SIT_POLICY_WAITING), *actor_served += the envs
   * served.  No queue and no capacity: request_env/noise/obs/count/age may be NULL and
   * request_capacity is ignored.  An env stopped at a sampling event steps again from the start of the
   * next launch, and every env's rows equal those of the queued path with request_capacity = n_env
   * and sit_policy_actor, bit for bit.  (Logged launches, which run the one-wave kernel, are served
   * through the library's own queue of capacity n_env and sit_policy_actor, with the same result.) */
  const float* actor_weights;  /* float32[SIT_ACTOR_WEIGHTS] (sit_policy_actor's layout) or NULL */
  int32_t actor_deterministic; /* nonzero: x = mu (no sampling noise) */
  int64_t* actor_served;       /* int64[1] or NULL: += envs served */
} sit_rollout_args;
#define SIT_POLICY_READY 1    /* policy_ready: an action waits in policy_action[e] */
#define SIT_POLICY_WAITING 2  /* policy_ready: the env stopped at a sampling event for its action */
int sit_rollout(sit_handle* h, const sit_rollout_args* a, void* stream);
size_t sit_rollout_args_size(void);
/* Policy mode helper: the squashed Gaussian head of the actor (ast_core/distributions/normal.py:
 * 88-101, ast_core/policies/gaussian_policy.py:71-72) applied to the actor network's output and
 * scattered into the env action slots, for request rows q < *request_count:
 *   x = mu + exp(clip(log_sigma, -20, 2)) * noise[q]   (x = mu when deterministic != 0)
 *   policy_action[request_env[q]] = tanh(x); policy_ready[request_env[q]] = 1
 * head real[capacity][head_stride] holds (mu, log_sigma) in its first two columns.
 *   served   int64[1] or NULL: += min(*request_count, capacity) (the policy evaluations used, as
 *            sit_policy_actor counts them) */
int sit_policy_apply(sit_handle* h, int32_t capacity, const void* head, int32_t head_stride,
                     const void* noise, const int32_t* request_env, const int32_t* request_count,
                     int32_t deterministic, void* policy_action, int32_t* policy_ready, int64_t* served,
                     void* stream);
/* Policy mode helper, the whole actor in one kernel: the SAC-AST Gaussian policy's MLP
 * (ast_core/nn_models/mlp.py:95-148: obs[SIT_OBS_DIM] -> 256 -> ReLU -> 256 -> ReLU -> (mu, log_sigma),
 * main_ast.py:67's hidden sizes) in float32 on request rows q < min(*request_count, capacity), then the
 * head and scatter of sit_policy_apply (GaussianPolicy.get_actions, gaussian_policy.py:114-126, as
 * agent.select_action mode 1 calls it, main_ast.py:344-349).
 *   weights  float32[SIT_ACTOR_WEIGHTS]: W1 [256][SIT_OBS_DIM] (torch Linear layout), b1 [256],
 *            W2 transposed [256 in][256 out], b2 [256], W3 [2][256], b3 [2]
 *   obs      real[capacity][SIT_OBS_DIM] (the request_obs rows of sit_rollout_args)
 *   served   int64[1] or NULL: += min(*request_count, capacity)
 *   clear_count int32[1] or NULL: set to 0 (one store, no grid-wide synchronisation).  sit_rollout's
 *            admission writes *request_count itself, so the build's sampler passes NULL. */
#define SIT_ACTOR_HIDDEN 256
#define SIT_ACTOR_WEIGHTS (SIT_ACTOR_HIDDEN * SIT_OBS_DIM + SIT_ACTOR_HIDDEN + SIT_ACTOR_HIDDEN * SIT_ACTOR_HIDDEN + \
                           SIT_ACTOR_HIDDEN + 2 * SIT_ACTOR_HIDDEN + 2)
int sit_policy_actor(sit_handle* h, int32_t capacity, const float* weights, const void* obs, const void* noise,
                     const int32_t* request_env, const int32_t* request_count, int32_t deterministic,
                     void* policy_action, int32_t* policy_ready, int64_t* served, int32_t* clear_count,
                     void* stream);

/* ---- state export / import (device blob) ------------------------------------------ */
/* The dynamic state of all envs (ship states, controller integrators, route tables,
 * stop flags, counters) lives in one device blob; fields are described by
 * sit_state_field(id) for id in [0, sit_state_nfields()). */
#define SIT_DT_REAL 0
#define SIT_DT_I32 1
#define SIT_DT_U32 2
int32_t sit_state_nfields(void);
int sit_state_field(const sit_handle* h, int32_t id, const char** name, size_t* offset,
                    int32_t* dtype, int64_t* count);
int sit_state_bytes(const sit_handle* h, size_t* bytes);
int sit_get_state(sit_handle* h, void* dst, void* stream);
int sit_set_state(sit_handle* h, const void* src, void* stream);

/* ---- episode records (device-side episode reducer) ---------------------------------
 * What the reference's driver loop keeps per episode (test_beds/main_ast.py:310-440: episode_reward,
 * episode_steps, status, action_record[i_episode]), reduced on the device from the [n_steps][n_env]
 * rows a sit_rollout or sit_step has just written: a post-pass on the same stream (three kernels),
 * for rows of any producer and mode.  The handle owns one accumulator: per env the running values
 * below, kept across updates, and rows_seen (int64), the rows consumed by earlier updates.
 *
 * An update reads rows k = 0..n_steps-1 of every env e in row order:
 *  - a row whose status has SIT_ST_NO_STEP is skipped entirely (reward not read into the sum, even if
 *    NaN; done ignored);
 *  - ret (float64) = ret + (double)reward[k][e]: one IEEE add per row, for both precisions (the
 *    reference's episode_reward += reward); steps counts the rows stepped in the episode; events
 *    counts the rows whose action_out[k][e][3] != 0; angle[j] = action_out[k][e][2] of event j for
 *    j < SIT_EPISODE_ACTIONS (later events are counted, not stored); episode counts the episodes
 *    this accumulator has finished for env e;
 *  - a row with done != 0 ends the episode: one record is emitted and ret, steps, events and the
 *    angles start again from zero / NaN.
 * Record: double[SIT_EPISODE_DIM], integers as exactly representable doubles:
 *   [0] global env id (env_id_offset + e)   [1] episode number of that env (0-based)   [2] steps
 *   [3] return (ret after the done row)     [4] terminal status bits (the done row's status, uint32)
 *   [5] events                              [6] row index of the done row (rows_seen + k)
 *   [7] terminal reward                     [8:18] the done row's next_state (NaN without next_state)
 *   [18:32] angle[0..13], NaN-padded (all NaN without action_out)
 * The records of one update are appended at *record_count in ascending (env id, episode) order; the
 * slot of a record is a function of the inputs only, never of scheduling.  Records past
 * record_capacity are counted in *record_count but not written.  status_hist[b] += 1 for every
 * finished episode (written or not) whose terminal status has bit b.
 *
 * sit_episodes_reset allocates the accumulator and every scratch buffer on first use and zeroes all
 * running values and rows_seen; the first sit_episodes_update does the same if reset was never
 * called.  Afterwards an update allocates nothing and never synchronises, so it can be captured in a
 * HIP graph: call reset once before capturing.  The accumulator is freed by sit_destroy and is not
 * part of the sit_get_state blob; sit_episodes_get / _set copy it (sit_episodes_bytes bytes, device
 * pointers) for checkpointing. */
#define SIT_EPISODE_ACTIONS 14
#define SIT_EPISODE_DIM 32
typedef struct sit_episodes_args {
  int32_t n_steps;
  int32_t record_capacity;
  int64_t env_id_offset;
  const void* reward;       /* real[n_steps][n_env]        required */
  const uint8_t* done;      /* u8[n_steps][n_env]          required */
  const uint32_t* status;   /* u32[n_steps][n_env]         required */
  const void* action_out;   /* real[n_steps][n_env][4]     or NULL  */
  const void* next_state;   /* real[n_steps][n_env][10]    or NULL  */
  double* records;          /* double[record_capacity][32] or NULL  */
  int64_t* record_count;    /* int64[1]: += finished episodes (written or not); required */
  int64_t* status_hist;     /* int64[32] or NULL */
} sit_episodes_args;
size_t sit_episodes_args_size(void);
int sit_episodes_reset(sit_handle* h, void* stream);
int sit_episodes_update(sit_handle* h, const sit_episodes_args* a, void* stream);
int sit_episodes_bytes(const sit_handle* h, size_t* bytes);
int sit_episodes_get(sit_handle* h, void* dst, void* stream);
int sit_episodes_set(sit_handle* h, const void* src, void* stream);

/* ---- scores (reduction of the episode records, best episode, conditional weight copy) --
 * What the reference's driver loop keeps over episodes (test_beds/main_ast.py:432-444: best_reward and
 * the checkpoint of the policy that reached it; 453-523: avg_reward and the status_record of a scoring
 * round), reduced on the device from the records above, so that a launch needs no host read.
 *
 * The score block is double score[SIT_SCORE_DIM], caller-owned, 8-byte aligned (a checkpoint is that
 * tensor); integers are stored as exactly representable doubles:
 *   [0] episodes scored     [1] sum of returns      [2] sum of steps       [3] minimum return
 *   [4] maximum return      [5] dropped records     [6] updates applied
 *   [7] 1 if the last update replaced the best episode, else 0
 *   [8:16] class counts (SIT_SCORE_CLASSES)         [16] stamp of the best episode (sit_score_keep)
 *   [17:32] zero            [32:64] the best episode's record (the 32 columns above)
 * sit_score_reset sets everything to zero, then [3] = +inf, [4] = -inf, [16] = NaN, [32:64] = NaN.
 *
 * sit_score_update reduces the records a sit_episodes_update left in (records, record_count).  With
 * count = max(*record_count, 0) and m = min(count, record_capacity), both read on the device:
 *  - SIT_SCORE_FRESH resets the block first;
 *  - record j < m is included iff episode_limit == 0 or rec[1] < episode_limit (a scoring round takes
 *    the first episode_limit episodes of every env);
 *  - [0] += included records, [2] += their steps, [6] += 1;
 *  - class c += included records with (class_any[c] == 0 || status & class_any[c]) and
 *    !(status & class_none[c]); a class whose masks are both 0 is unused and stays 0;
 *  - the round's return sum is formed in a fixed order, so its bits never depend on scheduling: x[j] = ret
 *    of an included record, +0.0 otherwise; chunks of 256 slots, zero-padded; in each chunk the halving
 *    tree x[i] += x[i + s] for s = 128, 64, ..., 1; the chunk sums go in groups of 256 (zero-padded)
 *    through the same tree; the group sums are added to a running value that starts at +0.0, in
 *    ascending order; finally [1] = [1] + round sum;
 *  - [3] = min([3], the included non-NaN returns) + 0.0 and [4] = max(...) + 0.0 (a zero result is +0.0);
 *  - the round's best is the included record with the greatest non-NaN return, the lowest slot among
 *    equal returns; it replaces the block's best iff the block has none ([35] is NaN) or its return is
 *    strictly greater: then its 32 columns go to [32:64] and [7] = 1; otherwise [7] = 0;
 *  - SIT_SCORE_CONSUME: [5] += count - m, then *record_count = 0, so the log holds only what arrived
 *    since the last score.  Without the flag nothing of the log is written, and scoring the same buffer
 *    twice counts its records twice.
 * Two launches on the caller's stream (one block per chunk of record_capacity, since the host never
 * knows m: a block past m reads the count and exits; then one block).  The per-chunk scratch belongs
 * to the handle and is freed by sit_destroy; sit_score_reserve allocates it for buffers of up to
 * max_records records, and an update that needs more grows it, which allocates and cannot be captured
 * (the contract of sit_replay_reserve).  After a sufficient reserve an update allocates nothing, never
 * synchronises and can be captured in a HIP graph.  Arguments are validated before any launch
 * (SIT_E_INVALID).
 *
 * sit_score_keep: when score[7] != 0 it copies every src[i] to dst[i] (floats[i] float32 each) and
 * sets score[16] = (double)*stamp if stamp is given; otherwise it writes nothing.  One launch; the
 * decision is read from the block on the device, so "update, keep" keeps the weights that produced the
 * best episode without a host step.  Blocks must not overlap. */
#define SIT_SCORE_DIM 64
#define SIT_SCORE_CLASSES 8
#define SIT_SCORE_KEEP_BLOCKS 4
#define SIT_SCORE_CONSUME 1u  /* count the dropped records and empty the log */
#define SIT_SCORE_FRESH 2u    /* reset the block before the update */
typedef struct sit_score_args {
  int32_t record_capacity;  /* rows of records, > 0 */
  uint32_t flags;           /* SIT_SCORE_* */
  int64_t episode_limit;    /* >= 0; 0: no limit */
  const double* records;    /* double[record_capacity][32] */
  int64_t* record_count;    /* int64[1], 8-byte aligned; written with SIT_SCORE_CONSUME only */
  double* score;            /* double[SIT_SCORE_DIM], 8-byte aligned */
  uint32_t class_any[SIT_SCORE_CLASSES];
  uint32_t class_none[SIT_SCORE_CLASSES];
} sit_score_args;
typedef struct sit_score_keep_args {
  int32_t n_blocks;                          /* 0 .. SIT_SCORE_KEEP_BLOCKS */
  const float* src[SIT_SCORE_KEEP_BLOCKS];   /* 16-byte aligned */
  float* dst[SIT_SCORE_KEEP_BLOCKS];         /* 16-byte aligned */
  int64_t floats[SIT_SCORE_KEEP_BLOCKS];     /* > 0, at most 2^34 */
  double* score;                             /* double[SIT_SCORE_DIM], 8-byte aligned */
  const int64_t* stamp;                      /* int64[1], 8-byte aligned, or NULL */
} sit_score_keep_args;
size_t sit_score_args_size(void);
size_t sit_score_keep_args_size(void);
int sit_score_reset(sit_handle* h, double* score, void* stream);
int sit_score_reserve(sit_handle* h, int32_t max_records);
int sit_score_update(sit_handle* h, const sit_score_args* a, void* stream);
int sit_score_keep(sit_handle* h, const sit_score_keep_args* a, void* stream);

/* ---- replay memory (device-side ring and minibatches) -------------------------------
 * What the reference's driver loop does with its ReplayMemory (test_beds/main_ast.py:350-396:
 * memory.push per sampling event, len(memory), memory.sample for agent.update_parameters), on the
 * transition records above.  The caller owns both tensors, so a checkpoint is those two:
 *   ring    real[capacity][SIT_TRANSITION_DIM], 4-real aligned
 *   cursor  int64[4] = {pushed, dropped, draws, 0}: records pushed so far (the ring holds
 *           size = min(pushed, capacity) of them), records their source buffers had no room for,
 *           minibatches drawn so far
 *
 * sit_replay_push appends the records of one source buffer (a sit_rollout's transitions and
 * transition_count: records are counted, not clamped).  With count = max(*src_count, 0), read on the
 * device, and n = min(count, src_capacity):
 *  - the n valid records are taken in canonical order: ascending env id (column 23, as uint32; a value
 *    that is no integer id in [0, 2^32 - 2) sorts behind every id), and within one env the order in
 *    which they stand in src.  One env is always stepped by the same lane of the same wave, whose slot
 *    allocations increase over time, so this is "env-major, each env in step order", whatever order the
 *    waves reached the counter in;
 *  - record j of that order goes to slot (pushed + j) mod capacity; if n > capacity only the last
 *    capacity records are written, so no slot is written twice in one push;
 *  - pushed += n, dropped += count - n.
 * Pushing the buffers of ranks 0, 1, ... one after another (shard r owns ids [r n_env, (r+1) n_env))
 * therefore leaves the ring one rank owning all envs would have.
 *
 * sit_replay_sample draws n_batches minibatches of batch records.  Minibatch u has draw number
 * d = draws + u; its element b is ring row P(b mod size), P = P_{seed,d} a bijection of [0, size), so for
 * batch <= size the rows of one minibatch are distinct (a sample without replacement):
 *  - a 4-round balanced Feistel network on 2h bits, h = ceil(max(bit_length(size - 1), 2) / 2): with
 *    x = L 2^h + R, a round maps (L, R) to (R, L ^ F), F the low h bits of word 0 of
 *    Philox4x32-10(key = (seed lo, seed hi), ctr = (R, 0x525000 | round, d lo, d hi)), round = 0..3;
 *  - applied again while the value is not below size (cycle walking).
 * Outputs, [n_batches][batch] rows: state real[..][10], action real[..][1], reward real, next_state
 * real[..][10], mask real (columns 0:10, 10, 11, 12:22, 22, copied as bits), env int32 (column 23; -1 if it
 * is no id below 2^31), index int32 (the ring row).  From an empty ring every output is zero and index
 * is -1.  Then draws += n_batches.
 *
 * Push runs a key kernel, a stable radix sort of (env id, source row) over src_capacity items, a
 * scatter with 16-byte accesses and a one-thread cursor update; sample a gather kernel and a cursor
 * update; all on the caller's stream, with no host synchronisation.  The sort's scratch belongs to the
 * handle and is freed by sit_destroy.  sit_replay_reserve allocates it for source buffers of up to
 * max_src_capacity records; a push that needs more grows it, which allocates and cannot be captured
 * (the contract of sit_episodes_reset).  After a sufficient reserve, push and sample allocate nothing
 * and can be captured in a HIP graph. */
typedef struct sit_replay_push_args {
  int32_t capacity;         /* ring records, > 0 */
  int32_t src_capacity;     /* records src has room for, > 0 */
  void* ring;               /* real[capacity][24] */
  int64_t* cursor;          /* int64[4] */
  const void* src;          /* real[src_capacity][24], 4-real aligned */
  const int32_t* src_count; /* int32[1]: records counted by the producer */
} sit_replay_push_args;
typedef struct sit_replay_sample_args {
  int32_t capacity;         /* ring records, > 0 */
  int32_t batch;            /* > 0 */
  int32_t n_batches;        /* > 0; batch * n_batches <= 2^30 */
  uint64_t seed;
  const void* ring;         /* real[capacity][24] */
  int64_t* cursor;          /* int64[4] */
  void* state;              /* real[n_batches][batch][10] */
  void* action;             /* real[n_batches][batch][1]  */
  void* reward;             /* real[n_batches][batch]     */
  void* next_state;         /* real[n_batches][batch][10] */
  void* mask;               /* real[n_batches][batch]     */
  int32_t* env;             /* int32[n_batches][batch]    */
  int32_t* index;           /* int32[n_batches][batch]    */
} sit_replay_sample_args;
size_t sit_replay_push_args_size(void);
size_t sit_replay_sample_args_size(void);
int sit_replay_reserve(sit_handle* h, int32_t max_src_capacity, void* stream);
int sit_replay_push(sit_handle* h, const sit_replay_push_args* a, void* stream);
int sit_replay_sample(sit_handle* h, const sit_replay_sample_args* a, void* stream);
/* sit_replay_sample with the state and next_state columns normalised by `affine` (float[SIT_OBSNORM_AFFINE],
 * "observation normalisation" below) as they are copied: the bits of sit_replay_sample followed by
 * sit_obsnorm_apply on state and next_state.  Every other output is sit_replay_sample's. */
int sit_replay_sample_normalised(sit_handle* h, const sit_replay_sample_args* a, const float* affine, void* stream);

/* ---- SAC learner: the no-gradient half of an update ----------------------------------
 * agent.update_parameters (test_beds/main_ast.py:350-362; twin Q networks of hidden size 256,
 * main_ast.py:41-90) needs, per minibatch and without gradients, the actor at next_state with its
 * log-probability, both target critics at (next_state, a'), the TD target, and afterwards the Polyak
 * update of the targets.  Two calls, one kernel each, on the caller's stream; they validate their
 * arguments (SIT_E_INVALID for a null required pointer, batch <= 0 or n <= 0, or a weight block that is
 * not 16-byte aligned: nothing is launched), allocate nothing and never synchronise.
 *
 * Critic block: SIT_CRITIC_WEIGHTS float32 per critic, 11 -> 256 -> ReLU -> 256 -> ReLU -> 1 on
 * concat(next_state, a'):  W1 [256][11] (torch Linear layout), b1 [256], W2 transposed [256 in][256 out],
 * b2 [256], W3 [256], b3 [1], then zero padding to a multiple of 4 floats.  critic_weights holds two such
 * blocks, Q1's then Q2's.  The actor block is sit_policy_actor's (SIT_ACTOR_WEIGHTS).
 *
 * sit_sac_target, for each row b < batch, networks and logp in float32:
 *   (mu, ls) = actor(next_state[b]);  ls = clip(ls, -20, 2)
 *   x = fma(exp(ls), eps, mu);  a' = tanh(x)
 *   logp = -0.5 eps^2 - ls - 0.5 log(2 pi) - log(1 - tanh(x)^2 + 1e-6)
 *   q_i = Q_i(concat(next_state[b], a')), i = 1, 2
 *   y[b] = reward_scale * reward[b] + mask[b] * gamma * (min(q1, q2) - alpha * logp)   in the handle's real
 * 1 - tanh(x)^2 is formed from x as 4 (em + 1) / (em + 2)^2, em = expm1(2 |x|), never as 1 - a' a'.
 * eps is noise[b] when noise is given; otherwise a standard normal drawn per row from Philox4x32-10(key =
 * (seed lo, seed hi), ctr = (b, 0x5441, update lo, update hi)) by the Box-Muller step of the policy's
 * event noise: u1 = (2^26 (c0 >> 5) + (c1 >> 6) + 1) / 2^53, u2 = (2^26 (c2 >> 5) + (c3 >> 6)) / 2^53,
 * eps = sqrt(-2 log u1) cos(2 pi u2), in float64, then rounded to float32.  alpha is read on the device.
 * Deterministic; rows [0, batch) do not depend on batch.
 *
 * sit_sac_polyak: target[i] = fma(tau, online[i] - target[i], target[i]) in float32 for i < n, over any
 * packed block (both critics at once: n = 2 SIT_CRITIC_WEIGHTS). */
#define SIT_CRITIC_INPUT (SIT_OBS_DIM + 1)
#define SIT_CRITIC_WEIGHTS \
  ((SIT_ACTOR_HIDDEN * SIT_CRITIC_INPUT + SIT_ACTOR_HIDDEN + SIT_ACTOR_HIDDEN * SIT_ACTOR_HIDDEN + SIT_ACTOR_HIDDEN + \
    SIT_ACTOR_HIDDEN + 1 + 3) / 4 * 4)
typedef struct sit_sac_target_args {
  int32_t batch;               /* rows B, > 0 */
  uint64_t seed;               /* key of the noise draw (noise == NULL) */
  uint64_t update;             /* counter words 2, 3 of the noise draw */
  double gamma;
  double reward_scale;
  const float* actor_weights;  /* float[SIT_ACTOR_WEIGHTS], 16-byte aligned */
  const float* critic_weights; /* float[2][SIT_CRITIC_WEIGHTS] (the target critics), 16-byte aligned */
  const float* alpha;          /* float[1], device */
  const void* next_state;      /* real[B][10] */
  const void* reward;          /* real[B] */
  const void* mask;            /* real[B] */
  void* y;                     /* real[B] */
  const void* noise;           /* real[B] or NULL (drawn on the device) */
  void* next_action;           /* real[B] or NULL: a' */
  void* next_logp;             /* real[B] or NULL */
  void* q1;                    /* real[B] or NULL */
  void* q2;                    /* real[B] or NULL */
} sit_sac_target_args;
size_t sit_sac_target_args_size(void);
int sit_sac_target(sit_handle* h, const sit_sac_target_args* a, void* stream);
int sit_sac_polyak(sit_handle* h, float* target, const float* online, int64_t n, float tau, void* stream);

/* ---- SAC learner: the gradient half of an update -------------------------------------
 * The two critic losses, the policy loss and the temperature loss of agent.update_parameters with their
 * backward passes and Adam steps, for the architectures above (actor 10 -> 256 -> 256 -> 2, twin critic
 * 11 -> 256 -> 256 -> 1).  Two calls of two kernels each on the caller's stream (forward + backward per
 * row, then the weight gradients fused with Adam); a whole update is sit_sac_target, sit_sac_critic_step,
 * sit_sac_policy_step, sit_sac_polyak.  Networks, gradients and Adam moments are float32; the minibatch
 * arrays are in the handle's real type.  Both calls validate their arguments (SIT_E_INVALID for a null
 * required pointer, batch <= 0, a parameter or moment block that is not 16-byte aligned, or a workspace
 * smaller than sit_sac_workspace_floats(batch): nothing is launched), allocate nothing and never
 * synchronise.  Every sum has a fixed order and there are no atomics: the same state gives the same bits.
 * The means over the rows that form the results (and the temperature's gradient) are summed in float64,
 * ascending, and rounded to float32 once.
 *
 * One network's backward pass, from its output gradients g[b][o], with x the input row, h1, h2 the hidden
 * activations and z2[n] = sum_k W2T[k][n] h1[k] + b2[n]:
 *   dW3[o] = sum_b g[b][o] h2[b];  db3[o] = sum_b g[b][o]
 *   d2 = (sum_o W3[o] g[o]) * [h2 > 0];  dW2T[k][n] = sum_b h1[b][k] d2[b][n];  db2 = sum_b d2
 *   d1[k] = (sum_n W2T[k][n] d2[n]) * [h1[k] > 0];  dW1[j][i] = sum_b d1[b][j] x[b][i];  db1 = sum_b d1
 * each sum over b ascending.  Adam (torch defaults; `bias1` = 1 - beta1^t, `bias2` = 1 - beta2^t of the
 * step count t the caller keeps, formed in double on the host), per element with gradient g:
 *   m <- m + (1 - beta1) (g - m);  v <- beta2 v + (1 - beta2) g^2
 *   p <- p - (lr / bias1) m / (sqrt(v) / sqrt(bias2) + eps)
 * applied in place to the packed block and its moment blocks of the same layout; padding floats are not
 * touched.  The gradient is never stored.
 *
 * sit_sac_critic_step, B = batch, x = concat(state, action), y from sit_sac_target, for i = 1, 2:
 *   q_i = Q_i(x);  l_i = mean_b (q_i - y)^2;  g_i[b] = 2 (q_i[b] - y[b]) / B
 * then one Adam step on both critics.  results[0], results[1] = l_1, l_2.
 *
 * sit_sac_policy_step, with the critics as they are (just updated) and alpha as it is before this call:
 *   (mu, ls_raw) = actor(state);  ls = clip(ls_raw, -20, 2)
 *   eps = noise[b], or the draw of sit_sac_target with counter word 1 = 0x5049
 *   x = fma(exp(ls), eps, mu);  a = tanh(x);  s = 1 - tanh(x)^2 = 4 (em + 1) / (em + 2)^2, em = expm1(2 |x|)
 *   logp = -0.5 eps^2 - ls - 0.5 log(2 pi) - log(s + 1e-6)
 *   q_i = Q_i(concat(state, a));  lp = mean_b (alpha logp - min(q1, q2))
 * backward: the critic with the smaller q (q1 on a tie) is seeded with -1/B and taken through to input
 * column 10 only, g_a = sum_j W1[j][10] d1[j] (no critic parameter gradient is formed);
 *   dx = (alpha / B) 2 a s / (s + 1e-6) + g_a s;  dmu = dx
 *   dls = dx exp(ls) eps - alpha / B, and 0 where ls_raw lies outside [-20, 2] (the bounds pass it)
 * then the actor's backward pass with the two output gradients (dmu, dls) and one Adam step on the actor.
 * Temperature, when tune != 0 (log_alpha as it is before this call):
 *   la = -mean_b (log_alpha (logp + target_entropy));  d la / d log_alpha = -mean_b (logp + target_entropy)
 *   one scalar Adam step on log_alpha (alpha_adam), then alpha[0] = exp(log_alpha)
 * tune == 0: la = 0, alpha and log_alpha are untouched.  results[2..4] = lp, la, alpha[0] after the call.
 *
 * Workspace: float32, sit_sac_workspace_floats(batch) = 2 * batch * SIT_SAC_WORKSPACE_ROW elements, where
 * the row kernels leave each row's input, h1, h2, d1, d2, output gradients and loss terms for the Adam
 * kernels.  The two calls may share one workspace.
 *
 * sit_sac_critic_step_tiled and sit_sac_policy_step_tiled take the same arguments, apply the same checks,
 * need the same workspace and produce the same results as the plain calls, bit for bit: after the same row
 * kernel they form each 32 x 32 tile of a weight gradient with the float32-input MFMA
 * (v_mfma_f32_32x32x2_f32) instead of one serial sum per element.  The bits agree because the batch is the
 * MFMA's k index: the instruction is a k-ordered float32 fmaf chain with one rounding per product, taken
 * over the rows ascending from zero and never split, which is the sum above.  They are the calls for large
 * batches, where the serial sum's time grows with B per element.
 *
 * sit_sac_target_wide, sit_sac_critic_step_wide and sit_sac_policy_step_wide take the arguments of
 * sit_sac_target and of the two step calls, apply the same checks with the same error strings, need the same
 * workspace, allocate nothing, never synchronise, and produce the same results as sit_sac_target and the
 * _tiled step calls, bit for bit (the workspace records included).  Their row kernels take 32 minibatch
 * rows per block of 256 threads instead of 8, so W2^T is streamed once per 32 rows, and run the two sums
 * that are 95 % of a row's arithmetic as v_mfma_f32_32x32x2_f32 chains: forward layer 2,
 * sum_k h1[b][k] W2T[k][n], as four chains per element, one per K quarter [64 q, 64 q + 64) from zero with k
 * ascending, joined as ((q0 + q1) + (q2 + q3)) + b2; and backward layer 2, sum_n W2T[k][n] d2[b][n], as one
 * chain per element over n = 0..255 from zero.  Those are the orders in which the other calls form these sums
 * with fmaf, and the float32-input MFMA is a k-ordered fmaf chain with one rounding per product, so the bits
 * agree; layers 1 and 3, d2, the Gaussian head and the loss terms are the same VALU arithmetic.  Each step
 * call launches its wide row kernel and then the _tiled call's weight-gradient kernel.  They are the calls
 * for large batches: with fewer than a few hundred rows there are too few blocks of 32 to fill the device. */
#define SIT_SAC_WORKSPACE_ROW 1040
typedef struct sit_sac_adam {
  double lr, beta1, beta2, eps;
  double bias1;                /* 1 - beta1^t */
  double bias2;                /* 1 - beta2^t */
} sit_sac_adam;
typedef struct sit_sac_critic_step_args {
  int32_t batch;               /* rows B, > 0 */
  int64_t workspace_floats;    /* elements of workspace, >= sit_sac_workspace_floats(batch) */
  sit_sac_adam adam;
  float* critic_weights;       /* float[2][SIT_CRITIC_WEIGHTS] (the online critics), 16-byte aligned */
  float* critic_m;             /* first moments, the same layout, 16-byte aligned */
  float* critic_v;             /* second moments */
  const void* state;           /* real[B][10] */
  const void* action;          /* real[B] */
  const void* y;               /* real[B] */
  float* workspace;
  float* results;              /* float[5]: [0], [1] are written */
} sit_sac_critic_step_args;
typedef struct sit_sac_policy_step_args {
  int32_t batch;               /* rows B, > 0 */
  int32_t tune;                /* != 0: the temperature step */
  int64_t workspace_floats;
  uint64_t seed;               /* key of the noise draw (noise == NULL) */
  uint64_t update;             /* counter words 2, 3 of the noise draw */
  double target_entropy;
  sit_sac_adam adam;           /* the actor's */
  sit_sac_adam alpha_adam;     /* log_alpha's (tune != 0) */
  float* actor_weights;        /* float[SIT_ACTOR_WEIGHTS], 16-byte aligned */
  float* actor_m;
  float* actor_v;
  const float* critic_weights; /* float[2][SIT_CRITIC_WEIGHTS], read only, 16-byte aligned */
  float* alpha;                /* float[1], device; written when tune != 0 */
  float* log_alpha;            /* float[1] and its two moments: required when tune != 0 */
  float* log_alpha_m;
  float* log_alpha_v;
  const void* state;           /* real[B][10] */
  const void* noise;           /* real[B] or NULL (drawn on the device) */
  float* workspace;
  float* results;              /* float[5]: [2], [3], [4] are written */
} sit_sac_policy_step_args;
int64_t sit_sac_workspace_floats(int32_t batch);   /* 0 for batch <= 0 */
size_t sit_sac_critic_step_args_size(void);
size_t sit_sac_policy_step_args_size(void);
int sit_sac_critic_step(sit_handle* h, const sit_sac_critic_step_args* a, void* stream);
int sit_sac_policy_step(sit_handle* h, const sit_sac_policy_step_args* a, void* stream);
int sit_sac_critic_step_tiled(sit_handle* h, const sit_sac_critic_step_args* a, void* stream);
int sit_sac_policy_step_tiled(sit_handle* h, const sit_sac_policy_step_args* a, void* stream);
int sit_sac_target_wide(sit_handle* h, const sit_sac_target_args* a, void* stream);
int sit_sac_critic_step_wide(sit_handle* h, const sit_sac_critic_step_args* a, void* stream);
int sit_sac_policy_step_wide(sit_handle* h, const sit_sac_policy_step_args* a, void* stream);

/* ---- SAC learner: many updates per call from a device clock ----------------------------
 * The calls above take the update number and the Adam bias corrections by value, so the host forms them
 * for every update.  sit_sac_updates enqueues n_updates whole updates whose per-update scalars come from a
 * clock in device memory that the kernels themselves advance: the host reads nothing back, and a HIP graph
 * of the call replays as the next n_updates updates, not as the captured ones.
 *
 * The clock: SIT_SAC_CLOCK_WORDS int64, caller-owned, 8-byte aligned, zero for a fresh learner.  Words 0..7
 * are its state, and all a checkpoint needs:
 *   {update, critic_steps, policy_steps, alpha_steps, results_written, 0, 0, 0}
 * update is the number of the next update (the `update` of sit_sac_target / sit_sac_policy_step and the
 * operand of the Polyak decision update % target_update_interval == 0), the three step words are the Adam
 * steps already taken, results_written the result rows written so far.  The caller may write the state
 * words between calls (on the stream).  The rest is opaque: two "tick" slots that hold, for one update, the
 * three optimisers' step scalars, the update number, the Polyak flag and the results row, formed on the
 * device.
 *
 * The Adam scalars of step t, a pure function of (lr, beta1, beta2, eps, t) in IEEE double without
 * contraction, so that the host, NumPy and the device agree bit for bit:
 *   pow_sq(beta, t):  r = 1; b = beta; n = t;  while n: { if (n & 1) r = r * b;  b = b * b;  n >>= 1 }
 *   bias1 = 1 - pow_sq(beta1, t);  bias2 = 1 - pow_sq(beta2, t)
 *   step_size = (float)(lr / bias1);  sqrt_bias2 = (float)sqrt(bias2)     (correctly rounded divide and sqrt)
 *   one_minus_beta1 = (float)(1 - beta1), beta2 = (float)beta2, one_minus_beta2 = (float)(1 - beta2), eps = (float)eps
 * At beta1 = 0.9, beta2 = 0.999 the two rounded floats equal those of bias = 1 - beta^t formed with pow (the
 * calls above as the Python learner drives them) for every t up to 300 000 at least; for other betas
 * pow_sq is the specification.  The `bias1`, `bias2` members of the three sit_sac_adam are ignored.
 *
 * sit_sac_updates: one small launch forms the first tick from the state words, then for u = 0 .. n_updates-1
 * five launches: the target rows (sit_sac_target on slice u of next_state, reward, mask, with the target
 * critics and y), the critic rows, the critics' Adam step, the policy rows, the actor's Adam step with the
 * temperature step; arithmetic, noise draws and results are those of sit_sac_target, sit_sac_critic_step,
 * sit_sac_policy_step and sit_sac_polyak called with update = clock.update and the step counts of the clock
 * (mode: the plain, _tiled or _wide forms; the same bits).  Differences: the critics' Adam launch also
 * applies target[e] = fma(tau, p - target[e], target[e]) to each element e it has just stepped when
 * update % target_update_interval == 0 (padding floats are skipped: the Polyak update leaves equal values
 * equal); the five results go to row results_written % results_capacity of `results`; and the thread that
 * finishes the losses advances the clock: update, critic_steps, policy_steps, results_written each + 1,
 * alpha_steps + 1 when tune != 0.  The minibatch arrays hold n_updates minibatches one after another
 * ([n_updates][batch][...], sit_replay_sample's layout); update u reads slice u.
 * The call validates its arguments (SIT_E_INVALID: nothing is launched), allocates nothing and never
 * synchronises.
 *
 * sit_sac_adam_scalars: the device's six scalars (the order above: one_minus_beta1, beta2, one_minus_beta2,
 * step_size, sqrt_bias2, eps) of steps t0 .. t0 + n - 1 into out[n][6]; t0 >= 1, n > 0. */
#define SIT_SAC_CLOCK_WORDS 64
#define SIT_SAC_UPDATES_PLAIN 0  /* sit_sac_target, sit_sac_critic_step, sit_sac_policy_step */
#define SIT_SAC_UPDATES_TILED 1  /* sit_sac_target and the _tiled step calls */
#define SIT_SAC_UPDATES_WIDE 2   /* the _wide calls */
typedef struct sit_sac_updates_args {
  int32_t mode;                /* SIT_SAC_UPDATES_* */
  int32_t batch;               /* rows B per update, > 0 */
  int32_t n_updates;           /* > 0 */
  int32_t tune;                /* != 0: the temperature step */
  uint64_t seed;               /* key of both noise draws */
  double gamma, reward_scale, target_entropy, tau;
  int64_t target_update_interval; /* > 0 */
  int64_t workspace_floats;    /* elements of workspace, >= sit_sac_workspace_floats(batch) */
  int64_t results_capacity;    /* rows of results, > 0 */
  sit_sac_adam critic_adam;    /* bias1, bias2 are ignored in all three */
  sit_sac_adam actor_adam;
  sit_sac_adam alpha_adam;     /* log_alpha's (tune != 0) */
  float* critic_weights;       /* float[2][SIT_CRITIC_WEIGHTS] (the online critics), 16-byte aligned */
  float* critic_m;
  float* critic_v;
  float* actor_weights;        /* float[SIT_ACTOR_WEIGHTS], 16-byte aligned */
  float* actor_m;
  float* actor_v;
  float* target_weights;       /* float[2][SIT_CRITIC_WEIGHTS] (the target critics), 16-byte aligned */
  float* alpha;                /* float[1], device; written when tune != 0 */
  float* log_alpha;            /* float[1] and its two moments: required when tune != 0 */
  float* log_alpha_m;
  float* log_alpha_v;
  const void* state;           /* real[n_updates][B][10] */
  const void* action;          /* real[n_updates][B] */
  const void* reward;          /* real[n_updates][B] */
  const void* next_state;      /* real[n_updates][B][10] */
  const void* mask;            /* real[n_updates][B] */
  void* y;                     /* real[B], scratch */
  float* workspace;
  int64_t* clock;              /* int64[SIT_SAC_CLOCK_WORDS], 8-byte aligned */
  float* results;              /* float[results_capacity][5] */
} sit_sac_updates_args;
size_t sit_sac_updates_args_size(void);
int sit_sac_updates(sit_handle* h, const sit_sac_updates_args* a, void* stream);
int sit_sac_adam_scalars(sit_handle* h, const sit_sac_adam* o, int64_t t0, int32_t n, float* out, void* stream);

/* ---- observation normalisation (running statistics, the affine, the folded actor block) ----
 * Per-column x^_i = (x_i - shift_i) * scale_i over the ten observation columns, applied where minibatches
 * are drawn (sit_replay_sample_normalised, sit_obsnorm_apply) and where the actor is served (sit_obsnorm_fold
 * writes a serving block whose first layer absorbs the affine); no step kernel and no learner kernel knows
 * of it.  x^ is never clipped: a clip cannot be folded into W1.  Outliers are bounded by min_std instead.
 * Two caller-owned device tensors, so a checkpoint is those two:
 *   block   double[SIT_OBSNORM_DIM], 8-byte aligned: 0 n (records accounted), 1 updates applied, 2 seen (the
 *           replay cursor's `pushed` up to which records are accounted), 3 records overwritten in the ring
 *           before they were seen, 8:18 mean, 24:34 M2 (sum of squared deviations), the rest zero
 *   affine  float[SIT_OBSNORM_AFFINE], 16-byte aligned: 0:10 shift, 16:26 scale, 32:42 min_std, the rest zero
 * sit_obsnorm_reset: block zero, shift 0, scale 1, min_std from the host array of ten floats (NULL: zeros).
 *
 * sit_obsnorm_update accounts the records of a replay ring that are new since the last update; everything
 * is decided on the device.  With pushed = cursor[0]:
 *   start = max(seen, pushed - capacity);  m = min(pushed - start, max_new)   (m < 0 counts as 0)
 *   the new records are logical indices g in [start, start + m), ring row g mod capacity, ascending g
 *   per column c < 10 of those rows, as float64:  S = tree sum of x;  mean_b = S / m;
 *     Q = tree sum of (x - mean_b)^2      (the tree of the scores' return sum above: chunks of 256 through
 *     the zero-padded halving tree, chunk sums in groups of 256 through the same tree, groups ascending)
 *   n' = n + m;  d = mean_b - mean;  mean' = mean + d (m / n');  M2' = (M2 + Q) + (d d) ((n m) / n')
 *   s = sqrt(M2' / n');  std = s > min_std ? s : min_std;  scale = (float)(1 / std);  shift = (float)mean'
 *   word 3 += start - seen;  seen = start + m;  n = n';  word 1 += 1
 * in IEEE double in this order without contraction.  A remainder beyond max_new is picked up by the next
 * update; m = 0 writes nothing but word 1.  Four launches (chunk sums, batch mean, chunk deviations, finish)
 * sized by max_new; their scratch belongs to the handle and is allocated by sit_obsnorm_reserve only: an
 * update with max_new beyond the reserve fails.  No block waits on another.
 *
 * sit_obsnorm_apply: x^ = (x - (real)shift) * (real)scale in the handle's real type, two roundings, in place
 * over rows_a and, when given, rows_b (real[n_rows][10], 2-real aligned).  NaN passes.
 * sit_obsnorm_fold: dst = src (float[SIT_ACTOR_WEIGHTS], 16-byte aligned, not overlapping) except
 *   W1'[j][i] = W1[j][i] * scale[i] in float32;  b1'[j] = (float)((double)b1[j] - sum_i (double)W1'[j][i] *
 *   (double)shift[i]), i ascending from +0.0
 * so that actor(dst, x) = actor(src, x^).  The identity affine gives src's bits. */
#define SIT_OBSNORM_DIM 64
#define SIT_OBSNORM_AFFINE 48
typedef struct sit_obsnorm_args {
  int32_t capacity;         /* ring records, > 0 */
  int32_t max_new;          /* most records accounted by this update, > 0 and within the reserve */
  const void* ring;         /* real[capacity][24], 4-real aligned */
  const int64_t* cursor;    /* the replay cursor, int64[4] */
  double* block;            /* double[SIT_OBSNORM_DIM] */
  float* affine;            /* float[SIT_OBSNORM_AFFINE] */
} sit_obsnorm_args;
size_t sit_obsnorm_args_size(void);
int sit_obsnorm_reset(sit_handle* h, double* block, float* affine, const float* min_std, void* stream);
int sit_obsnorm_reserve(sit_handle* h, int32_t max_new);
int sit_obsnorm_update(sit_handle* h, const sit_obsnorm_args* a, void* stream);
int sit_obsnorm_apply(sit_handle* h, const float* affine, void* rows_a, void* rows_b, int64_t n_rows, void* stream);
int sit_obsnorm_fold(sit_handle* h, const float* affine, const float* src, float* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIT_H */
