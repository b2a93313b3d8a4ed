"""MI355X-native ship-in-transit env step for SAC-AST rollouts (drop-in for the reference's
``MultiShipRLEnv`` hot path).  The compute is the HIP library libsit.so; see include/sit.h."""
from . import _lib
from .config import params, params_from_reference
from .scenario import Scenario, make_scenario
from .status import status_string
from .episodes import EpisodeLog, episodes_reference
from .replay import ReplayMemory, replay_reference
from .score import REFERENCE_CLASSES, Scoreboard, Scorer, score_reference
from .obsnorm import REFERENCE_OBS_HIGH, REFERENCE_OBS_LOW, ObsNormalizer, ObsNormReference

__all__ = ["params", "params_from_reference", "Scenario", "make_scenario", "status_string",
           "VecMultiShipRLEnv", "MultiShipRLEnv", "load_library", "EpisodeLog", "episodes_reference",
           "ReplayMemory", "replay_reference", "REFERENCE_CLASSES", "Scoreboard", "Scorer", "score_reference",
           "ObsNormalizer", "ObsNormReference", "REFERENCE_OBS_LOW", "REFERENCE_OBS_HIGH", "QNetwork", "SacLearner", "SacUpdateReference",
           "pack_critic_weights", "unpack_critic_weights", "sac_noise", "policy_noise", "sac_target_reference",
           "sac_update_reference", "bind_parameters", "block_views", "moments_to_adam_state", "adam_state_to_moments"]
# the learner's names (sac.py imports torch: resolved on first use, like the env classes)
_SAC = ("QNetwork", "SacLearner", "SacUpdateReference", "pack_critic_weights", "unpack_critic_weights", "sac_noise",
        "policy_noise", "sac_target_reference", "sac_update_reference", "bind_parameters", "block_views",
        "moments_to_adam_state", "adam_state_to_moments")


def load_library():
    return _lib.load()


def __getattr__(name):
    if name == "VecMultiShipRLEnv":
        from .env import VecMultiShipRLEnv
        return VecMultiShipRLEnv
    if name == "MultiShipRLEnv":
        from .compat import MultiShipRLEnv
        return MultiShipRLEnv
    if name in _SAC:
        from . import sac
        return getattr(sac, name)
    raise AttributeError(name)
