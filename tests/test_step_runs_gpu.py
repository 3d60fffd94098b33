"""Step runs: the split coherent chains advance their envs by up to FOUR steps per launch (ssd_rollout_plan.hpp, Schedule, sent by ssd_rollout.hip, rollout_aql; the step-pair
kernels' pass loop with a pass count and their renderer role's rounds of two, ssd_kernels.hip kModeStepPair).  Every case runs
rollout calls against oracle/pyoracle.py, bit for bit -- every step's observations, rewards and dones as far as the ring still holds
them, and the state after the call -- and asserts what ssd_rollout_path() reports: aql, coherent, split, pairs and the longest run
one launch took ("run").

The cases are those of tests/test_step_pairs_gpu.py and tests/test_step_pair_args_gpu.py, whose `_case` / `_child` run them, at the
shapes where a run of four can go wrong and a pair cannot: step counts that leave remainders of 1, 2 and 2 + 1 behind the runs of
four, rings of 1, 3 and 5 slots under 12 steps, a reset on each of a would-be run's four positions, two calls of 4 + 4 + 2 + 1,
two chains, overlay snapshots on each of a run's four positions, the test-hook library's SSD_AQL_RUN = 3 (launches of three steps,
which no product call makes: the kernel's general pass and render counts) and = 2 (today's pairs), and -- Cleanup 25 x 18 with 5
agents, whose kernel lays out ONE window of spawn thresholds for a run's four passes -- a waste count that leaves the window's
usual lanes on each of the four.

Which kernels take runs of four: Harvest 16 x 38 and 25 x 38 with 5 agents, Harvest 16 x 38 with 10, Cleanup 25 x 18 with 5.
Cleanup 25 x 18 with 10 agents keeps pairs by rule (built for runs of four it spills two vector registers to scratch memory): its
case asserts the same results and run == 2.

9 or 10 envs at 4 per workgroup (two full workgroups and one with a single env).  Cases that need what a process reads once when it
loads the library (SSD_ENVS_PER_BLOCK, the test-hook library's SSD_AQL_RUN / SSD_AQL_PAIRS) run this file as a script in a child
process; the imported `_child` helpers start the script named by their module's `__file__`, which is pointed here for the call."""
import json
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
import test_step_pairs_gpu as P  # noqa: E402
import test_step_pair_args_gpu as A  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.abspath(__file__)


class _RunEngine(VecEngine):
    """The engine the imported cases build: every look at rollout_path() also asserts the longest run the call's launches took."""
    want_run = None

    def rollout_path(self):
        path = super().rollout_path()
        assert path["run"] == _RunEngine.want_run, (path, _RunEngine.want_run)
        return path


def _run_case(spec):
    """spec = {"suite": "pairs" | "args", "run": the longest run expected, "clean_steps": [...] (args: the all-CLEAN steps), "cfg":
    the imported _case's configuration}."""
    mod = P if spec["suite"] == "pairs" else A
    _RunEngine.want_run = spec["run"]
    old = mod.VecEngine, A.CLEAN_STEPS
    mod.VecEngine = _RunEngine
    if spec.get("clean_steps"):
        A.CLEAN_STEPS = tuple(spec["clean_steps"])
    try:
        mod._case(spec["cfg"])
    finally:
        mod.VecEngine, A.CLEAN_STEPS = old
        _RunEngine.want_run = None


def _pairs(run, **cfg):
    cfg.setdefault("pairs", run > 1)
    return dict(suite="pairs", run=run, cfg=cfg)


def _child(monkeypatch, spec, **env_vars):
    """The imported module's _child, starting THIS file with the whole spec."""
    mod = P if spec["suite"] == "pairs" else A
    monkeypatch.setattr(mod, "__file__", HERE)
    for k in ("SSD_AQL_RUN",):
        monkeypatch.delenv(k, raising=False)
    if spec["suite"] == "pairs":
        P._child(spec, **env_vars)
    else:
        assert not env_vars
        A._child(spec)


@pytest.fixture(autouse=True)
def _needs_split():
    if not _split_expected():
        pytest.skip("the environment turns the split coherent chains off")


@pytest.mark.parametrize("steps", [16, 17, 18, 19])
@pytest.mark.parametrize("name", ["harvest", "cleanup"])
def test_remainders_behind_runs_of_four(monkeypatch, name, steps):
    """Shipped maps, N = 5, 9 envs at 4 per workgroup, one chain, from the edge state, ring = steps: four runs of four, then nothing,
    a single step, a pair, a pair and a single step -- each of whose launches renders the run before it."""
    _child(monkeypatch, _pairs(4, map=name, E=9, steps=steps, ring=steps, edge=True), SSD_ENVS_PER_BLOCK="4")


@pytest.mark.parametrize("ring", [1, 3, 5])
def test_ring_sizes(ring):
    """12 steps into a ring of 1 (a run's four steps land in one slot, the last over the others), of 3 and of 5 (runs straddle the
    ring's wrap, a run covers the ring more than once): every slot holds the last step that maps to it."""
    _run_case(_pairs(4, map="harvest", E=9, steps=12, ring=ring, edge=True))


@pytest.mark.parametrize("step0", [1, 2, 3, 4])
def test_resets_on_each_position_of_a_run(step0):
    """reset_every = 6, 20 steps, horizon 3.  The steps before the first reset are 4 + 1, 4, 2 + 1 and 2 -- so that reset falls on
    each of the four positions of a would-be run of four, and the renderer-only launch ahead of it delivers a single step, a run of
    four, a single step and a pair; every later period is 4 + 2 (a pair ahead of the reset)."""
    _run_case(_pairs(4, map="harvest", E=9, steps=20, ring=20, reset_every=6, step0=step0, horizon=3))


def test_repeat_calls_then_a_per_call_step():
    """Two calls of 11 steps back to back on one handle (4 + 4 + 2 + 1 each, so the second call starts from the other buffer of the
    state pair), then a per-call step() and get_state."""
    _run_case(_pairs(4, map="harvest", E=9, steps=11, ring=11, calls=2, per_call_step=True))


def test_two_chains():
    """Two chains of 5 envs (where the device's pool has two queues), 13 steps: the second chain's env offsets into the three mid
    sets."""
    import torch
    probe = VecEngine(K.GAME_HARVEST, K.HARVEST_MAP, num_envs=10, num_agents=5, seed=1)
    probe.reset()
    probe.set_rollout_chains(2)
    probe.rollout_random(4, torch.zeros((1, 10, 5, 15, 15, 3), dtype=torch.uint8, device="cuda"), None, None)
    pool = probe.rollout_path()["pool"]
    probe.close()
    if pool < 2:
        pytest.skip("the device's pool has one dispatch queue")
    _run_case(_pairs(4, map="harvest", E=10, steps=13, ring=13, chains=2))


def test_scripted_actions_force_snapshots_on_each_position_of_a_run():
    """rollout_actions, Harvest, 5 agents, an action ring of 5 with 12 steps (three runs of four; every pass past a run's second
    fetches its actions at the top of the pass before).  All five agents fire (an overlay snapshot instead of a beam list) in slots
    0 and 4 of the even envs -- steps 0, 4, 5, 9, 10: positions 0, 0, 1, 1, 2 of their runs -- and in slots 2 and 3 of the odd ones
    -- steps 2, 3, 7, 8: positions 2, 3, 3, 0."""
    _run_case(_pairs(4, map="harvest", E=9, steps=12, ring=12, action_ring=5))


def test_cleanup_ten_agents_scripted_actions_keep_pairs():
    """The same with Cleanup's shipped map and 10 agents: six shooters per env in every step (two beam lists), all ten in slot 1 of
    the even envs (a snapshot).  Its kernel keeps pairs by rule: same results, run == 2."""
    _run_case(_pairs(2, map="cleanup", E=6, N=10, steps=12, ring=12, action_ring=5))


def test_hook_run_of_three_exercises_the_general_counts(monkeypatch):
    """SSD_AQL_RUN=3 (test-hook library), 17 steps: five launches of three steps and one of two -- pass and render counts no
    product call uses (a renderer wave's first round then holds one step, its second two)."""
    _child(monkeypatch, _pairs(3, map="harvest", E=9, steps=17, ring=17, edge=True), SSD_ENVS_PER_BLOCK="4", SSD_LIB_PATH=HOOKS_LIB, SSD_AQL_RUN="3")


@pytest.mark.parametrize("run,knob", [(2, dict(SSD_AQL_RUN="2")), (1, dict(SSD_AQL_PAIRS="0")), (4, {})])
def test_hook_caps_and_knob_off(monkeypatch, run, knob):
    """SSD_AQL_RUN=2 (test-hook library) reproduces the launches in pairs, SSD_AQL_PAIRS=0 single steps, the hook library with
    neither set runs of four: same results."""
    _child(monkeypatch, _pairs(run, map="harvest", E=9, steps=17, ring=17, edge=True), SSD_ENVS_PER_BLOCK="4", SSD_LIB_PATH=HOOKS_LIB, **knob)


def test_cleanup_counts_leave_the_threshold_window_on_each_position_of_a_run(monkeypatch):
    """Cleanup 25 x 18 with 5 agents, whose kernel prefetches one window of the spawn thresholds by waste count for the run's four
    passes.  Every env starts with its waste count AT the spawn threshold, the agents crowded on the river; 12 scripted steps, all
    agents CLEAN in steps 0, 5, 10 and 7 -- positions 0, 1, 2 and 3 of their runs.  The oracle's states say that in some env each of
    those steps reads its thresholds two or more counts below where the step began (asserted before the comparison)."""
    _child(monkeypatch, dict(suite="args", run=4, clean_steps=[0, 5, 10, 7],
                             cfg=dict(map="cleanup", E=9, N=5, ring=12, threshold_start=True, calls=[dict(steps=12, outputs="all")])))


if __name__ == "__main__":
    _run_case(json.loads(sys.argv[1]))
