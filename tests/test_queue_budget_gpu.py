"""The queue rule (csrc/ssd_queue_budget.hpp) where it meets the GPU: a process that exports GPU_MAX_HW_QUEUES=4 -- the HIP
runtime's own default, and what the GPU runners put in front of every command -- keeps the default pool of two dispatch queues,
so that bench.py's headline (4096 Harvest envs) runs the way it was built to: 2 chains of 2048 envs through the library's own
queues, coherent kernel variant, split rendering -- with the oracle's results.  A process of its own per case: the library reads
the variables once."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import golden_util as G
from oracle import pyoracle
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd.engine import VecEngine
E, N, RING, STEPS, EVERY = %(envs)d, 5, %(ring)d, %(steps)d, %(every)d
eng = VecEngine(K.GAME_HARVEST, None, num_envs=E, num_agents=N, seed=5)
ora = pyoracle.Oracle(K.GAME_HARVEST, K.HARVEST_MAP, E, N, G.default_lut(), seed=5)
out = eng.alloc_outputs()
obs = torch.zeros((RING,) + tuple(out[0].shape), dtype=torch.uint8, device="cuda")
rew = torch.zeros((RING,) + tuple(out[1].shape), dtype=torch.int32, device="cuda")
eng.rollout_random(STEPS, obs, rew, None, reset_every=EVERY, step0=0); torch.cuda.synchronize()
g_obs, g_rew = obs.cpu().numpy(), rew.cpu().numpy()
for k in range(STEPS):
    if EVERY > 0 and k %% EVERY == 0:
        ora.reset()
    last = k >= STEPS - RING
    _, o_obs, o_rew, _ = ora.step_random(want_obs=last)
    if last:
        assert np.array_equal(g_rew[k %% RING], o_rew), "rewards of step %%d differ" %% k
        assert np.array_equal(g_obs[k %% RING], o_obs), "observations of step %%d differ" %% k
p = eng.rollout_path(); assert eng.status() == 0
print("PATH", p["aql"], p["coherent"], p["split"], p["chains"], p["pool"], p["queue_dropped"])
"""


def _child(env_set, envs, ring, steps, every):
    env = dict(os.environ)
    for k in ("GPU_MAX_HW_QUEUES", "SSD_AQL_QUEUES", "SSD_ROLLOUT_CHAINS", "SSD_AQL", "SSD_AQL_COHERENT", "SSD_AQL_SPLIT",
              "SSD_LIB_PATH"):
        env.pop(k, None)
    env.update(env_set)
    code = CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "envs": envs, "ring": ring, "steps": steps, "every": every}
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-2000:]
    return out


def test_hip_default_queue_count_keeps_the_two_chain_split_path():
    """GPU_MAX_HW_QUEUES=4 exported, SSD_AQL_QUEUES unset: a pool of 2 (not 1), and the headline's 4096 envs as 2 chains of 2048
    with the coherent variant and split rendering, 12 steps across a reset, the last ring slots against the oracle."""
    out = _child({"GPU_MAX_HW_QUEUES": "4"}, envs=4096, ring=4, steps=12, every=5)
    assert "PATH True True True 2 2 False" in out, out[-2000:]


@pytest.mark.parametrize("ring", [1, 3])
def test_one_queue_pool_splits_a_single_chain_up_to_3072_envs(ring):
    """SSD_AQL_QUEUES=1: one chain.  3072 envs in that chain take split rendering (the single-chain cap, csrc/ssd_rollout_plan.hpp, choose_form), 12
    steps across resets at steps 0, 5 and 10 -- the call ends in the renderer-only launch -- and the last ring slots equal the
    oracle's."""
    out = _child({"GPU_MAX_HW_QUEUES": "4", "SSD_AQL_QUEUES": "1"}, envs=3072, ring=ring, steps=12, every=5)
    assert "PATH True True True 1 1 False" in out, out[-2000:]


def test_one_queue_pool_does_not_split_4096_envs():
    """... and 4096 envs in one chain stay unsplit (measured slower split), with the oracle's results."""
    out = _child({"GPU_MAX_HW_QUEUES": "4", "SSD_AQL_QUEUES": "1"}, envs=4096, ring=2, steps=12, every=5)
    assert "PATH True True False 1 1 False" in out, out[-2000:]
