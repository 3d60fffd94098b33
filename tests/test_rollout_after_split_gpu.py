"""A rollout call that is not split after a split one on the same handle.  A split call leaves the state in either buffer of the
handle's pair; a call without observations has an argument set of ONE orientation, whose blocks name the buffer that is current
(csrc/ssd_rollout_plan.hpp, start_orientation and kind_table): it has to go out with that orientation's kinds wherever the state
sits.  Both parities of the first call's launch count, against oracle/pyoracle.py bit for bit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("first", [9, 8])
def test_a_call_without_observations_after_a_split_call(first):
    """Harvest's shipped map, 5 agents, 9 envs, reset_every = 5 from step 0.  9 steps are launches of 4 + 1 + 4 steps (the state ends
    in the second buffer), 8 steps of 4 + 1 + 3 = 4 + 1 + 2 + 1 (in the first); then 6 steps that write rewards and dones only."""
    import torch
    from oracle import pyoracle
    from sequential_social_dilemma_games_amd import config, constants as K
    from sequential_social_dilemma_games_amd.engine import VecEngine
    from test_split_common_path_gpu import _split_expected
    E, N = 9, 5
    eng = VecEngine(K.GAME_HARVEST, K.HARVEST_MAP, num_envs=E, num_agents=N, seed=7)
    ora = pyoracle.Oracle(K.GAME_HARVEST, K.HARVEST_MAP, E, N, config.make_lut(), seed=7)
    obs = torch.zeros((2, E, N, 15, 15, 3), dtype=torch.uint8, device="cuda")
    rew = torch.zeros((2, E, N), dtype=torch.int32, device="cuda")
    done = torch.zeros((2, E, N), dtype=torch.uint8, device="cuda")

    def oracle_steps(k0, n):
        for k in range(k0, k0 + n):
            if k % 5 == 0:
                ora.reset()
            _, o_obs, o_rew, o_done = ora.step_random()
        return o_obs, o_rew, o_done

    eng.rollout_random(first, obs, rew, done, reset_every=5, step0=0)
    path = eng.rollout_path()
    if _split_expected() and path["aql"]:
        assert path["coherent"] and path["split"] and path["run"] == 4, path
    o_obs, o_rew, _ = oracle_steps(0, first)
    last = (first - 1) % 2
    assert np.array_equal(obs[last].cpu().numpy(), o_obs) and np.array_equal(rew[last].cpu().numpy(), o_rew)

    eng.rollout_random(6, None, rew, done, reset_every=5, step0=first)
    assert eng.rollout_path()["aql"] == path["aql"] and not eng.rollout_path()["split"], eng.rollout_path()
    _, o_rew, o_done = oracle_steps(first, 6)
    last = (first + 5) % 2
    assert np.array_equal(rew[last].cpu().numpy(), o_rew)
    assert np.array_equal(done[last].cpu().numpy().astype(bool), np.asarray(o_done).astype(bool))
    a, b = eng.get_state(), ora.get_state()
    for key in ("world", "pos", "orient", "t"):
        assert np.array_equal(a[key], b[key]), key
    assert eng.status() == 0
