"""MI355X-native vectorised engine for the Harvest / Cleanup social-dilemma gridworlds.

    from sequential_social_dilemma_games_amd import HarvestEnv, CleanupEnv     # dict API (RLlib MultiAgentEnv)
    from sequential_social_dilemma_games_amd import VecEngine                  # batched tensor API
    from sequential_social_dilemma_games_amd import WatershedSeqEnv, WatershedSeqCommEnv, WatershedVecEngine
    from sequential_social_dilemma_games_amd import EpisodeStats                # per-episode returns and social metrics
    from sequential_social_dilemma_games_amd import WatershedEpisodeStats       # the same for Watershed, with the launchers' metrics
    from sequential_social_dilemma_games_amd import ConvFCPolicy                # the conv-FC policy net, run in the loop
    from sequential_social_dilemma_games_amd import ConvLSTMPolicy              # the same trunk under the baseline's LSTM
    from sequential_social_dilemma_games_amd import ConvMOAPolicy               # the causal-influence (MOA) policy
    from sequential_social_dilemma_games_amd import WatershedLSTMPolicy         # the Watershed baselines' LSTM-FC policy
    from sequential_social_dilemma_games_amd import compute_advantages          # GAE / discounted returns of a rollout batch
    from sequential_social_dilemma_games_amd import standardize_advantages, explained_variance, update_kl_coeff   # PPO's batch moments
    from sequential_social_dilemma_games_amd import ppo_loss                    # the PPO loss and its gradients, on the device
    from sequential_social_dilemma_games_amd import ppo_loss_recurrent          # the same for the recurrent policy, with BPTT
    from sequential_social_dilemma_games_amd import ppo_loss_moa                # PPO + MOA loss for the MOA policy, with BPTT
    from sequential_social_dilemma_games_amd import ppo_loss_watershed          # the PPO loss for the Watershed policy, with BPTT
    from sequential_social_dilemma_games_amd import a3c_loss, a3c_loss_recurrent, a3c_loss_moa   # the A3C loss, likewise
    from sequential_social_dilemma_games_amd import clip_grad_by_set_norm       # A3C's gradient clip, per weight set
    from sequential_social_dilemma_games_amd import vtrace, evaluate_fragment   # IMPALA's V-trace targets of a fragment
    from sequential_social_dilemma_games_amd import impala_loss, impala_loss_recurrent, impala_loss_moa   # the IMPALA loss
    from sequential_social_dilemma_games_amd import a3c_loss_watershed, impala_loss_watershed   # both for the Watershed policy
    from sequential_social_dilemma_games_amd import evaluate_sequences, ws_a3c_terms   # its sequences under the current weights

Everything that steps an env goes through libssd_hip.so (include/ssd.h); importing this package does
not load it, constructing an env does -- and fails loudly if it is missing.
"""
from .constants import CLEANUP_MAP, HARVEST_MAP  # noqa: F401


def __getattr__(name):
    if name == "VecEngine":
        from .engine import VecEngine
        return VecEngine
    if name in ("HarvestEnv", "HarvestAgent"):
        from . import harvest
        return getattr(harvest, name)
    if name in ("CleanupEnv", "CleanupAgent"):
        from . import cleanup
        return getattr(cleanup, name)
    if name in ("WatershedSeqEnv", "WatershedSeqCommEnv", "WatershedVecEngine"):
        from . import watershed
        return getattr(watershed, name)
    if name == "EpisodeStats":
        from .episode_stats import EpisodeStats
        return EpisodeStats
    if name == "WatershedEpisodeStats":
        from .watershed_stats import WatershedEpisodeStats
        return WatershedEpisodeStats
    if name in ("ConvFCPolicy", "ConvLSTMPolicy", "ConvMOAPolicy", "WatershedLSTMPolicy", "ppo_loss", "ppo_loss_recurrent",
                "ppo_loss_moa", "ppo_loss_watershed", "ws_ppo_terms", "a3c_loss", "a3c_loss_recurrent", "a3c_loss_moa", "clip_grad_by_set_norm", "A3C_STATS",
                "MOA_A3C_STATS", "evaluate_fragment", "impala_loss", "impala_loss_recurrent", "impala_loss_moa",
                "ws_a3c_terms", "a3c_loss_watershed", "evaluate_sequences", "impala_loss_watershed"):
        from . import policy
        return getattr(policy, name)
    if name in ("compute_advantages", "vtrace", "standardize_advantages", "explained_variance", "update_kl_coeff"):
        from . import postprocessing
        return getattr(postprocessing, name)
    if name == "MapEnv":
        from .map_env import MapEnv
        return MapEnv
    raise AttributeError(name)
