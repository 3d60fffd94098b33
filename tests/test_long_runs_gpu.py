"""Long runs: in calls of LONG = 256 steps or more (kLongCallSteps: it began at 64, the measurements of EXPERIMENTS.md round 28
moved it) the split coherent chains of Harvest 16 x 38 with 5 agents advance their envs by up to EIGHT steps per launch (ssd_rollout_plan.hpp: choose_form's long cap, Schedule under it, the long kinds and their blocks, sent by
ssd_rollout.hip; the long instantiation of the step kernel, ssd_kernels.hip kModeStepLong: its pass loop counting to eight from a
LongParams block, its renderer role running the four-step body once per half of a run).  Every case runs rollout calls against
oracle/pyoracle.py, bit for bit -- every step's observations, rewards and dones as far as the ring still holds them, and the state
after the call -- and asserts the longest run ssd_rollout_path() reports: 8, except where the case says why not.

The cases are those of tests/test_step_pairs_gpu.py, whose `_case` / `_child` run them the way tests/test_step_runs_gpu.py runs
them, at the shapes where a run of eight can go wrong and a run of four cannot: step counts that leave remainders of 0, 1, 2 + 1
and 4 + 2 + 1 behind the runs of eight; rings of 1, 3, 8 and 9 slots under LONG + 3 steps and one slot per step; a reset on each
of a would-be run's eight positions; two calls back to back and a per-call step; two chains; overlay snapshots on each of a run's eight
positions; the test-hook library's SSD_AQL_RUN=4 (the long call planned as a call that is not) and =8; and a call one step short of
long.  9 or 10 envs at 4 per workgroup."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))

from sequential_social_dilemma_games_amd import constants as K  # noqa: E402
from sequential_social_dilemma_games_amd.engine import VecEngine  # noqa: E402
from test_split_common_path_gpu import HOOKS_LIB, _split_expected  # noqa: E402
import test_step_runs_gpu as R  # noqa: E402

pytestmark = pytest.mark.gpu

LONG = 256       # ssd_rollout_plan.hpp, kLongCallSteps: a multiple of eight (the remainders below are those of 64, 65, 67 and 71 steps)


@pytest.fixture(autouse=True)
def _needs_split():
    if not _split_expected():
        pytest.skip("the environment turns the split coherent chains off")


@pytest.mark.parametrize("steps", [LONG, LONG + 1, LONG + 3, LONG + 7])
def test_remainders_behind_runs_of_eight(monkeypatch, steps):
    """9 envs at 4 per workgroup, one chain, from the edge state, one ring slot per step: 32 runs of eight, then nothing, a
    single step, a pair and a single step, a run of four, a pair and a single step -- each of whose launches renders the run
    before it, the first of them a run of eight."""
    R._child(monkeypatch, R._pairs(8, map="harvest", E=9, steps=steps, ring=steps, edge=True), SSD_ENVS_PER_BLOCK="4")


@pytest.mark.parametrize("ring", [1, 3, 8, 9])
def test_ring_sizes(ring):
    """LONG + 3 steps into a ring of 1 (a run's eight steps land in one slot, the last over the others, through both halves of a
    renderer wave's work), of 3 (a run covers the ring more than twice), of 8 (a run is one round of the ring) and of 9 (runs straddle the
    wrap at every position in turn): every slot holds the last step that maps to it."""
    R._run_case(R._pairs(8, map="harvest", E=9, steps=LONG + 3, ring=ring, edge=True))


@pytest.mark.parametrize("step0", [1, 2, 3, 4, 5, 6, 7, 8])
def test_resets_on_each_position_of_a_run(step0):
    """reset_every = 13, LONG + 6 steps, horizon 3.  The steps before the first reset are 13 - step0 = 12 .. 5: 8 + 4, 8 + 2 + 1,
    8 + 2, 8 + 1, 8, 4 + 2 + 1, 4 + 2, 4 + 1 -- that reset falls on each of the eight positions of a would-be run of eight, and the
    renderer-only launch ahead of it delivers a run of four, a single step, a pair or a run of eight.  Every later period is
    8 + 4 + 1."""
    R._run_case(R._pairs(8, map="harvest", E=9, steps=LONG + 6, ring=LONG + 6, reset_every=13, step0=step0, horizon=3))


def test_repeat_calls_then_a_per_call_step():
    """Two calls of LONG + 3 steps back to back on one handle (32 runs of eight, a pair and a single step each: the second call
    starts from the other buffer of the state pair), then a per-call step() and get_state."""
    R._run_case(R._pairs(8, map="harvest", E=9, steps=LONG + 3, ring=LONG + 3, calls=2, per_call_step=True))


def test_two_chains():
    """Two chains of 5 envs (where the device's pool has two queues), LONG + 1 steps: the second chain's env offsets into the
    seven mid sets."""
    import torch
    probe = VecEngine(K.GAME_HARVEST, K.HARVEST_MAP, num_envs=10, num_agents=5, seed=1)
    probe.reset()
    probe.set_rollout_chains(2)
    probe.rollout_random(4, torch.zeros((1, 10, 5, 15, 15, 3), dtype=torch.uint8, device="cuda"), None, None)
    pool = probe.rollout_path()["pool"]
    probe.close()
    if pool < 2:
        pytest.skip("the device's pool has one dispatch queue")
    R._run_case(R._pairs(8, map="harvest", E=10, steps=LONG + 1, ring=LONG + 1, chains=2))


def test_scripted_actions_force_snapshots_on_each_position_of_a_run():
    """rollout_actions with an action ring of 5 and LONG steps into a ring of LONG + 4 slots (a multiple of 5; 32 runs of eight;
    every pass past a run's second fetches its actions at the top of the pass before).  All five agents fire (an overlay snapshot instead of a beam list) in slots 0 and 4 of
    the even envs and in slots 2 and 3 of the odd ones: 5 and 8 have no common factor, so over 40 steps each of those slots meets
    each of a run's eight positions."""
    R._run_case(R._pairs(8, map="harvest", E=9, steps=LONG, ring=LONG + 4, action_ring=5))


@pytest.mark.parametrize("run,knob", [(4, dict(SSD_AQL_RUN="4")), (8, dict(SSD_AQL_RUN="8")), (8, {})])
def test_hook_run_of_four_plans_a_long_call_as_before(monkeypatch, run, knob):
    """SSD_AQL_RUN=4 (test-hook library) gives a call of LONG + 3 steps the launches of a call that is not long -- runs of four --,
    =8 and the hook library with nothing set runs of eight: same results."""
    R._child(monkeypatch, R._pairs(run, map="harvest", E=9, steps=LONG + 3, ring=LONG + 3, edge=True), SSD_ENVS_PER_BLOCK="4",
             SSD_LIB_PATH=HOOKS_LIB, **knob)


def test_a_call_one_step_short_is_not_long():
    """One step short of a long call: runs of four, as ever."""
    R._run_case(R._pairs(4, map="harvest", E=9, steps=LONG - 1, ring=LONG - 1, edge=True))
