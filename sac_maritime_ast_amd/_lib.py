"""ctypes binding of libsit.so (the HIP C ABI declared in include/sit.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc --offload-arch=gfx950).
There is no fallback: importing the product path without the library raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_int32, c_int64, c_size_t, c_uint64, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SIT_LIBRARY", os.path.join(HERE, "libsit.so"))

SIT_OK, SIT_E_INVALID, SIT_E_HIP, SIT_E_NOMEM, SIT_E_STATE = 0, -1, -2, -3, -4
SIT_F32, SIT_F64 = 32, 64
SIT_SG_MOTOR, SIT_SG_GEN, SIT_SG_OFF = 0, 1, 2
SIT_MACH_SHAFT, SIT_MACH_SIMPLIFIED = 0, 1
SIT_DT_REAL, SIT_DT_I32, SIT_DT_U32 = 0, 1, 2
SIT_OBS_DIM = 10
SIT_TRANSITION_DIM = 24
SIT_ACTOR_HIDDEN = 256
SIT_ACTOR_WEIGHTS = SIT_ACTOR_HIDDEN * SIT_OBS_DIM + SIT_ACTOR_HIDDEN + SIT_ACTOR_HIDDEN ** 2 + SIT_ACTOR_HIDDEN + 2 * SIT_ACTOR_HIDDEN + 2
# one critic's packed block (11 -> 256 -> 256 -> 1), padded to a multiple of 4 floats
SIT_CRITIC_INPUT = SIT_OBS_DIM + 1
SIT_CRITIC_WEIGHTS = (SIT_ACTOR_HIDDEN * SIT_CRITIC_INPUT + SIT_ACTOR_HIDDEN + SIT_ACTOR_HIDDEN ** 2 + SIT_ACTOR_HIDDEN
                      + SIT_ACTOR_HIDDEN + 1 + 3) // 4 * 4
SIT_SAC_WORKSPACE_ROW = 1040   # floats per row and network pass of the gradient half's workspace
SIT_SAC_CLOCK_WORDS = 64       # int64 words of the device-side update clock (sit_sac_updates); 0..7 are its state
SIT_SAC_UPDATES_PLAIN, SIT_SAC_UPDATES_TILED, SIT_SAC_UPDATES_WIDE = 0, 1, 2
SIT_LOG_KEYS, SIT_LOG_ROWS = 27, 62
SIT_EPISODE_ACTIONS, SIT_EPISODE_DIM = 14, 32
SIT_SCORE_DIM, SIT_SCORE_CLASSES, SIT_SCORE_KEEP_BLOCKS = 64, 8, 4
SIT_SCORE_CONSUME, SIT_SCORE_FRESH = 1, 2
SIT_OBSNORM_DIM, SIT_OBSNORM_AFFINE = 64, 48
INIT_FIELDS = ("north", "east", "yaw", "surge", "sway", "yaw_rate", "shaft_speed", "desired_speed",
               "ship_speed_i", "shaft_speed_i")

ST_TEST_ENDPOINT, ST_TEST_HORIZON, ST_TEST_TERRAIN = 1 << 0, 1 << 1, 1 << 2
ST_TEST_MECHANICAL, ST_TEST_NAVIGATION, ST_TEST_BLACKOUT = 1 << 3, 1 << 4, 1 << 5
ST_OBS_ENDPOINT, ST_OBS_HORIZON, ST_OBS_TERRAIN = 1 << 6, 1 << 7, 1 << 8
ST_OBS_IW_TERMINAL, ST_OBS_NAVIGATION, ST_COLLISION = 1 << 9, 1 << 10, 1 << 11
ST_TEST_DONE, ST_OBS_DONE, ST_ROUTE_OVERFLOW = 1 << 12, 1 << 13, 1 << 31
ST_NO_STEP = 1 << 30
SIT_POLICY_READY, SIT_POLICY_WAITING = 1, 2

_D = c_double
PARAM_FIELDS = [
    ("dead_weight_tonnage", _D), ("coefficient_of_deadweight_to_displacement", _D), ("bunkers", _D),
    ("ballast", _D), ("length_of_ship", _D), ("width_of_ship", _D),
    ("added_mass_coefficient_in_surge", _D), ("added_mass_coefficient_in_sway", _D),
    ("added_mass_coefficient_in_yaw", _D), ("mass_over_linear_friction_coefficient_in_surge", _D),
    ("mass_over_linear_friction_coefficient_in_sway", _D), ("mass_over_linear_friction_coefficient_in_yaw", _D),
    ("nonlinear_friction_coefficient_in_surge", _D), ("nonlinear_friction_coefficient_in_sway", _D),
    ("nonlinear_friction_coefficient_in_yaw", _D),
    ("current_velocity_component_from_north", _D), ("current_velocity_component_from_east", _D),
    ("wind_speed", _D), ("wind_direction", _D),
    ("rho_air", _D), ("front_height", _D), ("side_height", _D), ("cx", _D), ("cy", _D), ("cn", _D),
    ("integration_step", _D),
    ("hotel_load", _D), ("main_engine_capacity", _D), ("electrical_capacity", _D),
    ("shaft_generator_state", c_int32), ("machinery_model", c_int32),
    ("rated_speed_main_engine_rpm", _D), ("linear_friction_main_engine", _D),
    ("linear_friction_hybrid_shaft_generator", _D), ("gear_ratio_between_main_engine_and_propeller", _D),
    ("gear_ratio_between_hybrid_shaft_generator_and_propeller", _D), ("propeller_inertia", _D),
    ("propeller_speed_to_torque_coefficient", _D), ("propeller_diameter", _D),
    ("propeller_speed_to_thrust_force_coefficient", _D), ("rudder_angle_to_sway_force_coefficient", _D),
    ("rudder_angle_to_yaw_force_coefficient", _D), ("max_rudder_angle_degrees", _D),
    ("kp_ship_speed", _D), ("ki_ship_speed", _D), ("kp_shaft_speed", _D), ("ki_shaft_speed", _D),
    ("heading_kp", _D), ("heading_kd", _D), ("heading_ki", _D),
    ("radius_of_acceptance", _D), ("lookahead_distance", _D), ("los_integral_gain", _D),
    ("integrator_windup_limit", _D),
    ("theta", _D), ("sampling_frequency", c_int32), ("collision_bias", c_int32),
    ("e_tolerance", _D), ("arrival_radius", _D), ("shaft_rpm_max", _D), ("minimum_ship_distance", _D),
    ("bias_throttle_scale", _D), ("bias_throttle_max", _D), ("bias_rudder_degrees", _D),
    ("fuel_me_a", _D), ("fuel_me_b", _D), ("fuel_me_c", _D), ("fuel_dg_a", _D), ("fuel_dg_b", _D),
    ("fuel_dg_c", _D), ("thrust_force_dynamic_time_constant", _D),
]


class SitParams(ctypes.Structure):
    _fields_ = PARAM_FIELDS

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in PARAM_FIELDS if not k.startswith("_")}


class RolloutArgs(ctypes.Structure):
    _fields_ = [
        ("n_steps", c_int32), ("auto_reset", c_int32), ("seed", c_uint64), ("env_id_offset", c_int64),
        ("action_ne", c_void_p), ("sac_update", c_void_p), ("init", c_void_p),
        ("next_state", c_void_p), ("reward", c_void_p), ("done", c_void_p), ("status", c_void_p),
        ("action_out", c_void_p), ("done_count", c_void_p),
        ("transitions", c_void_p), ("transition_count", c_void_p), ("transition_capacity", c_int32),
        ("mask_horizon", c_int32),
        ("policy_action", c_void_p), ("policy_ready", c_void_p), ("request_env", c_void_p),
        ("request_noise", c_void_p), ("request_obs", c_void_p), ("request_count", c_void_p),
        ("request_capacity", c_int32),
        ("env_steps", c_void_p), ("log", c_void_p), ("request_age", c_void_p),
        ("actor_weights", c_void_p), ("actor_deterministic", c_int32), ("actor_served", c_void_p),
    ]


class EpisodesArgs(ctypes.Structure):
    _fields_ = [
        ("n_steps", c_int32), ("record_capacity", c_int32), ("env_id_offset", c_int64),
        ("reward", c_void_p), ("done", c_void_p), ("status", c_void_p), ("action_out", c_void_p),
        ("next_state", c_void_p), ("records", c_void_p), ("record_count", c_void_p), ("status_hist", c_void_p),
    ]


class ScoreArgs(ctypes.Structure):
    _fields_ = [
        ("record_capacity", c_int32), ("flags", ctypes.c_uint32), ("episode_limit", c_int64),
        ("records", c_void_p), ("record_count", c_void_p), ("score", c_void_p),
        ("class_any", ctypes.c_uint32 * SIT_SCORE_CLASSES), ("class_none", ctypes.c_uint32 * SIT_SCORE_CLASSES),
    ]


class ScoreKeepArgs(ctypes.Structure):
    _fields_ = [
        ("n_blocks", c_int32), ("src", c_void_p * SIT_SCORE_KEEP_BLOCKS), ("dst", c_void_p * SIT_SCORE_KEEP_BLOCKS),
        ("floats", c_int64 * SIT_SCORE_KEEP_BLOCKS), ("score", c_void_p), ("stamp", c_void_p),
    ]


class ReplayPushArgs(ctypes.Structure):
    _fields_ = [
        ("capacity", c_int32), ("src_capacity", c_int32), ("ring", c_void_p), ("cursor", c_void_p),
        ("src", c_void_p), ("src_count", c_void_p),
    ]


class ReplaySampleArgs(ctypes.Structure):
    _fields_ = [
        ("capacity", c_int32), ("batch", c_int32), ("n_batches", c_int32), ("seed", c_uint64),
        ("ring", c_void_p), ("cursor", c_void_p), ("state", c_void_p), ("action", c_void_p), ("reward", c_void_p),
        ("next_state", c_void_p), ("mask", c_void_p), ("env", c_void_p), ("index", c_void_p),
    ]


class SacTargetArgs(ctypes.Structure):
    _fields_ = [
        ("batch", c_int32), ("seed", c_uint64), ("update", c_uint64), ("gamma", c_double), ("reward_scale", c_double),
        ("actor_weights", c_void_p), ("critic_weights", c_void_p), ("alpha", c_void_p),
        ("next_state", c_void_p), ("reward", c_void_p), ("mask", c_void_p), ("y", c_void_p), ("noise", c_void_p),
        ("next_action", c_void_p), ("next_logp", c_void_p), ("q1", c_void_p), ("q2", c_void_p),
    ]


class SacAdam(ctypes.Structure):
    _fields_ = [("lr", c_double), ("beta1", c_double), ("beta2", c_double), ("eps", c_double), ("bias1", c_double),
                ("bias2", c_double)]


class SacCriticStepArgs(ctypes.Structure):
    _fields_ = [
        ("batch", c_int32), ("workspace_floats", c_int64), ("adam", SacAdam),
        ("critic_weights", c_void_p), ("critic_m", c_void_p), ("critic_v", c_void_p),
        ("state", c_void_p), ("action", c_void_p), ("y", c_void_p), ("workspace", c_void_p), ("results", c_void_p),
    ]


class SacPolicyStepArgs(ctypes.Structure):
    _fields_ = [
        ("batch", c_int32), ("tune", c_int32), ("workspace_floats", c_int64), ("seed", c_uint64), ("update", c_uint64),
        ("target_entropy", c_double), ("adam", SacAdam), ("alpha_adam", SacAdam),
        ("actor_weights", c_void_p), ("actor_m", c_void_p), ("actor_v", c_void_p), ("critic_weights", c_void_p),
        ("alpha", c_void_p), ("log_alpha", c_void_p), ("log_alpha_m", c_void_p), ("log_alpha_v", c_void_p),
        ("state", c_void_p), ("noise", c_void_p), ("workspace", c_void_p), ("results", c_void_p),
    ]


class SacUpdatesArgs(ctypes.Structure):
    _fields_ = [
        ("mode", c_int32), ("batch", c_int32), ("n_updates", c_int32), ("tune", c_int32), ("seed", c_uint64),
        ("gamma", c_double), ("reward_scale", c_double), ("target_entropy", c_double), ("tau", c_double),
        ("target_update_interval", c_int64), ("workspace_floats", c_int64), ("results_capacity", c_int64),
        ("critic_adam", SacAdam), ("actor_adam", SacAdam), ("alpha_adam", SacAdam),
        ("critic_weights", c_void_p), ("critic_m", c_void_p), ("critic_v", c_void_p),
        ("actor_weights", c_void_p), ("actor_m", c_void_p), ("actor_v", c_void_p), ("target_weights", c_void_p),
        ("alpha", c_void_p), ("log_alpha", c_void_p), ("log_alpha_m", c_void_p), ("log_alpha_v", c_void_p),
        ("state", c_void_p), ("action", c_void_p), ("reward", c_void_p), ("next_state", c_void_p), ("mask", c_void_p),
        ("y", c_void_p), ("workspace", c_void_p), ("clock", c_void_p), ("results", c_void_p),
    ]


class ObsnormArgs(ctypes.Structure):
    _fields_ = [
        ("capacity", c_int32), ("max_new", c_int32), ("ring", c_void_p), ("cursor", c_void_p), ("block", c_void_p),
        ("affine", c_void_p),
    ]


class SitError(RuntimeError):
    pass


# every entry point of include/sit.h: name -> (restype, argtypes)
SIGNATURES = {
    "sit_abi_version": (c_int32, []),
    "sit_params_size": (c_size_t, []),
    "sit_rollout_args_size": (c_size_t, []),
    "sit_params_default": (None, [POINTER(SitParams)]),
    "sit_create": (c_int32, [POINTER(SitParams), c_int32, c_int32, c_int32, POINTER(c_void_p)]),
    "sit_destroy": (None, [c_void_p]),
    "sit_last_error": (c_char_p, [c_void_p]),
    "sit_precision": (c_int32, [c_void_p]),
    "sit_n_env": (c_int32, [c_void_p]),
    "sit_step_kernel": (c_char_p, [c_void_p]),
    "sit_debug_flags": (c_int32, [c_void_p]),
    "sit_debug_build": (c_int32, []),
    "sit_role_fallbacks": (c_int32, [c_void_p, c_int32]),
    "sit_load_map": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p]),
    "sit_load_routes": (c_int32, [c_void_p, c_void_p, c_void_p]),
    "sit_load_initial": (c_int32, [c_void_p, c_void_p]),
    "sit_map_info": (c_int32, [c_void_p, c_void_p, c_int32]),
    "sit_policy_apply": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                                   c_void_p, c_void_p, c_void_p, c_void_p]),
    "sit_policy_actor": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sit_probe_map": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sit_selftest_f64": (c_int32, [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p]),
    "sit_restart": (c_int32, [c_void_p, c_void_p]),
    "sit_reset": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "sit_init_step": (c_int32, [c_void_p, c_void_p, c_void_p]),
    "sit_step": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_void_p, c_void_p]),
    "sit_step_host": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p]),
    "sit_rollout": (c_int32, [c_void_p, POINTER(RolloutArgs), c_void_p]),
    "sit_state_nfields": (c_int32, []),
    "sit_state_field": (c_int32, [c_void_p, c_int32, POINTER(c_char_p), POINTER(c_size_t),
                                  POINTER(c_int32), POINTER(c_int64)]),
    "sit_state_bytes": (c_int32, [c_void_p, POINTER(c_size_t)]),
    "sit_get_state": (c_int32, [c_void_p, c_void_p, c_void_p]),
    "sit_set_state": (c_int32, [c_void_p, c_void_p, c_void_p]),
    "sit_episodes_args_size": (c_size_t, []),
    "sit_episodes_reset": (c_int32, [c_void_p, c_void_p]),
    "sit_episodes_update": (c_int32, [c_void_p, POINTER(EpisodesArgs), c_void_p]),
    "sit_episodes_bytes": (c_int32, [c_void_p, POINTER(c_size_t)]),
    "sit_episodes_get": (c_int32, [c_void_p, c_void_p, c_void_p]),
    "sit_episodes_set": (c_int32, [c_void_p, c_void_p, c_void_p]),
    "sit_score_args_size": (c_size_t, []),
    "sit_score_keep_args_size": (c_size_t, []),
    "sit_score_reset": (c_int32, [c_void_p, c_void_p, c_void_p]),
    "sit_score_reserve": (c_int32, [c_void_p, c_int32]),
    "sit_score_update": (c_int32, [c_void_p, POINTER(ScoreArgs), c_void_p]),
    "sit_score_keep": (c_int32, [c_void_p, POINTER(ScoreKeepArgs), c_void_p]),
    "sit_replay_push_args_size": (c_size_t, []),
    "sit_replay_sample_args_size": (c_size_t, []),
    "sit_replay_reserve": (c_int32, [c_void_p, c_int32, c_void_p]),
    "sit_replay_push": (c_int32, [c_void_p, POINTER(ReplayPushArgs), c_void_p]),
    "sit_replay_sample": (c_int32, [c_void_p, POINTER(ReplaySampleArgs), c_void_p]),
    "sit_replay_sample_normalised": (c_int32, [c_void_p, POINTER(ReplaySampleArgs), c_void_p, c_void_p]),
    "sit_sac_target_args_size": (c_size_t, []),
    "sit_sac_target": (c_int32, [c_void_p, POINTER(SacTargetArgs), c_void_p]),
    "sit_sac_polyak": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, ctypes.c_float, c_void_p]),
    "sit_sac_workspace_floats": (c_int64, [c_int32]),
    "sit_sac_critic_step_args_size": (c_size_t, []),
    "sit_sac_policy_step_args_size": (c_size_t, []),
    "sit_sac_critic_step": (c_int32, [c_void_p, POINTER(SacCriticStepArgs), c_void_p]),
    "sit_sac_policy_step": (c_int32, [c_void_p, POINTER(SacPolicyStepArgs), c_void_p]),
    "sit_sac_critic_step_tiled": (c_int32, [c_void_p, POINTER(SacCriticStepArgs), c_void_p]),
    "sit_sac_policy_step_tiled": (c_int32, [c_void_p, POINTER(SacPolicyStepArgs), c_void_p]),
    "sit_sac_target_wide": (c_int32, [c_void_p, POINTER(SacTargetArgs), c_void_p]),
    "sit_sac_critic_step_wide": (c_int32, [c_void_p, POINTER(SacCriticStepArgs), c_void_p]),
    "sit_sac_policy_step_wide": (c_int32, [c_void_p, POINTER(SacPolicyStepArgs), c_void_p]),
    "sit_sac_updates_args_size": (c_size_t, []),
    "sit_sac_updates": (c_int32, [c_void_p, POINTER(SacUpdatesArgs), c_void_p]),
    "sit_sac_adam_scalars": (c_int32, [c_void_p, POINTER(SacAdam), c_int64, c_int32, c_void_p, c_void_p]),
    "sit_obsnorm_args_size": (c_size_t, []),
    "sit_obsnorm_reset": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sit_obsnorm_reserve": (c_int32, [c_void_p, c_int32]),
    "sit_obsnorm_update": (c_int32, [c_void_p, POINTER(ObsnormArgs), c_void_p]),
    "sit_obsnorm_apply": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "sit_obsnorm_fold": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

_lib = None


def load():
    """Load libsit.so (once).  Raises ImportError if the HIP library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"HIP library {LIB_PATH} is missing; build it with "
                          "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:        # diagnostic builds of older revisions (A/B timing) lack newer entries
            continue
        fn.restype = res
        fn.argtypes = args
    if lib.sit_abi_version() != 1:
        raise ImportError("libsit.so ABI version mismatch")
    if lib.sit_params_size() != ctypes.sizeof(SitParams):
        raise ImportError(f"sit_params layout mismatch: C {lib.sit_params_size()} vs "
                          f"ctypes {ctypes.sizeof(SitParams)} bytes")
    if lib.sit_rollout_args_size() != ctypes.sizeof(RolloutArgs):
        raise ImportError(f"sit_rollout_args layout mismatch: C {lib.sit_rollout_args_size()} vs "
                          f"ctypes {ctypes.sizeof(RolloutArgs)} bytes")
    if hasattr(lib, "sit_episodes_args_size") and lib.sit_episodes_args_size() != ctypes.sizeof(EpisodesArgs):
        raise ImportError(f"sit_episodes_args layout mismatch: C {lib.sit_episodes_args_size()} vs "
                          f"ctypes {ctypes.sizeof(EpisodesArgs)} bytes")
    for fn, struct in (("sit_replay_push_args_size", ReplayPushArgs), ("sit_replay_sample_args_size", ReplaySampleArgs),
                       ("sit_score_args_size", ScoreArgs), ("sit_score_keep_args_size", ScoreKeepArgs),
                       ("sit_sac_target_args_size", SacTargetArgs),
                       ("sit_sac_critic_step_args_size", SacCriticStepArgs),
                       ("sit_sac_policy_step_args_size", SacPolicyStepArgs),
                       ("sit_sac_updates_args_size", SacUpdatesArgs), ("sit_obsnorm_args_size", ObsnormArgs)):
        if hasattr(lib, fn) and getattr(lib, fn)() != ctypes.sizeof(struct):
            raise ImportError(f"{fn[:-5]} layout mismatch: C {getattr(lib, fn)()} vs ctypes {ctypes.sizeof(struct)} bytes")
    _lib = lib
    return lib


def check(rc, handle=None):
    if rc != SIT_OK:
        msg = load().sit_last_error(handle)
        raise SitError(f"sit error {rc}: {msg.decode() if msg else ''}")
    return rc


def default_params() -> SitParams:
    p = SitParams()
    load().sit_params_default(ctypes.byref(p))
    return p
