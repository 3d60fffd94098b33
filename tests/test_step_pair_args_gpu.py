"""Step pairs, the argument side: a step-pair launch's env waves take where each of their two passes leaves its state and outputs
from one record per pass behind the kernel's declared arguments (ssd_internal.hpp, PassRec; filled by ssd_rollout_plan.hpp, fill_block, for ssd_rollout.hip, aql_set).
What such a record can get wrong and tests/test_step_pairs_gpu.py does not run: a pair whose second step's ring and action slots
belong to ANOTHER argument block index than its first (rings of 3 and 2: six blocks, a pair that starts on the last), a second
chain's offsets into the action ring, the two pair kernels no other test reaches (Harvest 25 x 38 with 5 agents, Harvest 16 x 38
with 10), records whose reward and done pointers are null, and -- Cleanup 25 x 18, whose pair kernels prefetch one window of
spawn thresholds for both passes -- waste counts that leave the window's usual lanes on a pair's first step and on its second.

Every case runs against oracle/pyoracle.py, bit for bit -- every step's observations, rewards and dones as far as the ring still
holds them, and the state after the call -- and asserts what ssd_rollout_path() reports.  9 or 10 envs at 4 per workgroup
(SSD_ENVS_PER_BLOCK, read once per process: the cases run this file as a script in a child process), at most 13 steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))

import golden_util as G  # noqa: E402
from oracle import pyoracle  # noqa: E402
from sequential_social_dilemma_games_amd import constants as K  # noqa: E402
from sequential_social_dilemma_games_amd.engine import VecEngine  # noqa: E402
from test_split_common_path_gpu import _split_expected  # noqa: E402
from test_step_pairs_gpu import _scripted  # noqa: E402
import spawn_tables as ST  # noqa: E402

pytestmark = pytest.mark.gpu

ONE_QUEUE = "the device's pool has one dispatch queue"
CLEAN = 8
CLEAN_STEPS = (2, 5)                                     # of a 12-step call in pairs: a pair's first step, a pair's second


def _map(name):
    return {"harvest": (K.GAME_HARVEST, K.HARVEST_MAP), "harvest25x38": (K.GAME_HARVEST, K.harvest_map_25x38()),
            "cleanup": (K.GAME_CLEANUP, K.CLEANUP_MAP)}[name]


def _threshold_start(ora, amap, E, N):
    """Cleanup: every env holds as many 'H' cells as the smallest count at which no apple grows (the spawn threshold, cleanup.py:
    161-163), the agents crowd on and beside the river."""
    import types
    potential = ora.potential_waste_area
    at = min(n for n in range(potential + 1) if ora.cleanup_thresholds(n)[0] == 0)
    assert 0 < at <= len(ST.cells(amap, "HR")), at
    case, rng, st = types.SimpleNamespace(amap=amap, E=E, N=N), np.random.RandomState(5), ora.get_state()
    pos, orient = ST._crowd(case, st, rng, ST.cells(amap, "HR"))
    return dict(world=ST._waste_world(case, st, rng, lambda e, p: at), pos=pos, orient=orient), at


def _clean_script(E, N, slots):
    """Moves and turns, and in the slots of CLEAN_STEPS every agent cleans."""
    a = np.random.RandomState(23).randint(0, 7, size=(slots, E, N)).astype(np.int32)
    for k in CLEAN_STEPS:
        a[k] = CLEAN
    return a


def _edge_state(amap, E, N):
    """Positions and orientations with agents at the map's edges: the free cells nearest to the four corners, the centre, the middles
    of the four sides and the upper left quarter -- the first N of them, handed to the agents in another order in every env;
    orientations (agent + env) % 4."""
    H, W = len(amap), len(amap[0])
    free = np.array([(r, c) for r in range(H) for c in range(W) if amap[r][c] != "@"])
    anchors = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1),
               (H // 4, W // 4)]
    spots = []
    for anchor in anchors[:N]:
        d = np.abs(free - np.array(anchor)).sum(1).astype(np.float64)
        for s in spots:                                              # (distinct cells)
            d[(free == s).all(1)] = 1e9
        spots.append(free[int(np.argmin(d))])
    spots = np.array(spots)
    assert spots[:, 0].min() <= 7 and spots[:, 0].max() >= H - 8 and spots[:, 1].min() <= 7 and spots[:, 1].max() >= W - 8
    pos = np.zeros((E, N, 2), np.int16)
    orient = np.zeros((E, N), np.uint8)
    for e in range(E):
        for i in range(N):
            pos[e, i] = spots[(i + e) % N]
            orient[e, i] = (i + e) % 4
    return pos, orient


def _case(cfg):
    """One handle, one oracle; the calls of cfg["calls"], each {steps, outputs: "all" | "obs"}, back to back.  After every call each
    ring slot is compared with the last step that mapped to it (a buffer the call did not get keeps its fill value)."""
    import torch
    name, E, N, ring = cfg["map"], cfg["E"], cfg.get("N", 5), cfg["ring"]
    game, amap = _map(name)
    chains = cfg.get("chains", 1)
    if chains > 1:
        probe = VecEngine(game, amap, num_envs=E, num_agents=N, seed=1)
        probe.reset()
        probe.set_rollout_chains(chains)
        probe.rollout_random(4, torch.zeros((1, E, N, 15, 15, 3), dtype=torch.uint8, device="cuda"), None, None)
        pool = probe.rollout_path()["pool"]
        probe.close()
        if pool < chains:
            print(ONE_QUEUE)
            return
    eng = VecEngine(game, amap, num_envs=E, num_agents=N, seed=cfg.get("seed", 11))
    ora = pyoracle.Oracle(game, amap, E, N, G.default_lut(), seed=cfg.get("seed", 11))
    eng.reset()
    ora.reset()
    if cfg.get("edge"):
        pos, orient = _edge_state(amap, E, N)
        eng.set_state(pos=pos, orient=orient)
        ora.set_state(pos=pos, orient=orient)
    at = None
    if cfg.get("threshold_start"):
        start, at = _threshold_start(ora, amap, E, N)
        eng.set_state(**start)
        ora.set_state(**start)
        assert (ora.get_state()["world"] == ord("H")).sum((1, 2)).tolist() == [at] * E
    obs = torch.zeros((ring, E, N, 15, 15, 3), dtype=torch.uint8, device="cuda")
    rew = torch.full((ring, E, N), -77, dtype=torch.int32, device="cuda")
    done = torch.full((ring, E, N), 7, dtype=torch.uint8, device="cuda")
    eng.set_rollout_chains(chains)
    a_host = _scripted(name, E, N, cfg["action_ring"]) if cfg.get("action_ring") else None
    if cfg.get("threshold_start"):
        a_host = _clean_script(E, N, 12)
    off_lane = {}                                        # CLEAN step -> envs whose count left the window's usual lanes
    a_dev = torch.from_numpy(a_host).cuda() if a_host is not None else None
    s0 = cfg.get("step0", 0)
    for call, spec in enumerate(cfg["calls"]):
        steps, full = spec["steps"], spec["outputs"] == "all"
        rew.fill_(-77)
        done.fill_(7)
        if a_dev is not None:
            eng.rollout_actions(a_dev, steps, obs, rew if full else None, done if full else None, reset_every=0, step0=s0)
        else:
            eng.rollout_random(steps, obs, rew if full else None, done if full else None, reset_every=0, step0=s0)
        path = eng.rollout_path()
        assert path["aql"] and path["coherent"] and path["split"] and not path["fused"], path
        assert path["pairs"] is True, path
        assert path["chains"] == chains, path
        g_obs, g_rew, g_done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        want = {}
        for k in range(s0, s0 + steps):
            before = (ora.get_state()["world"] == ord("H")).sum((1, 2))
            if a_host is not None:
                o_obs, o_rew, o_done = ora.step(a_host[k % a_host.shape[0]])
            else:
                _, o_obs, o_rew, o_done = ora.step_random()
            if at is not None and k in CLEAN_STEPS:      # (the count the spawn pass used: two or more cells below the step's start)
                off_lane[k] = int((before.astype(np.int64) - ora.waste_count().astype(np.int64) >= 2).sum())
            want[k % ring] = (k, o_obs.copy(), o_rew.copy(), o_done.copy())
        if at is not None:
            assert all(off_lane.get(k, 0) > 0 for k in CLEAN_STEPS), off_lane
        for slot, (k, o_obs, o_rew, o_done) in sorted(want.items()):
            assert np.array_equal(g_obs[slot], o_obs), "call %d: observations of step %d (slot %d) differ" % (call, k, slot)
            if full:
                np.testing.assert_array_equal(g_rew[slot], o_rew, err_msg="call %d: rewards of step %d" % (call, k))
                np.testing.assert_array_equal(g_done[slot], o_done, err_msg="call %d: dones of step %d" % (call, k))
        if not full:                                                 # (nothing was to be written: null pointers in both records)
            assert (g_rew == -77).all() and (g_done == 7).all(), "call %d wrote rewards or dones it was not given" % call
        a, b = eng.get_state(), ora.get_state()
        for key in ("world", "pos", "orient", "episode", "t"):
            np.testing.assert_array_equal(a[key], b[key], err_msg="call %d: %s" % (call, key))
        s0 += steps
    status = eng.status()
    eng.close()
    assert status == 0, status
    print("step-pair argument case ok")


def _child(cfg):
    env = dict(os.environ)
    for k in ("SSD_LIB_PATH", "SSD_AQL_PAIRS"):
        env.pop(k, None)
    env["SSD_ENVS_PER_BLOCK"] = "4"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(cfg)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=300)
    out = r.stdout.decode(errors="replace")
    if r.returncode == 0 and ONE_QUEUE in out:
        pytest.skip(ONE_QUEUE)
    assert r.returncode == 0 and "step-pair argument case ok" in out, out[-3000:]


@pytest.fixture(autouse=True)
def _needs_split():
    if not _split_expected():
        pytest.skip("the environment turns the split coherent chains off")


@pytest.mark.parametrize("steps", [9, 13])
def test_pair_starts_on_the_last_of_six_argument_blocks(steps):
    """rollout_actions, an output ring of 3 and an action ring of 2: six argument blocks.  From step0 = 5 the call's first pair is
    steps 5 and 6 -- block 5, whose second pass takes output slot 0 and action slot 0, those of block 0 -- and every later pair
    starts on an odd block.  9 steps: the ring ends with steps 11, 12 and 13, and slot 0 holds step 12 -- the second pass of block
    5 again, across the ring's wrap: its observations, rewards and dones are compared.  13 steps: the odd remainder comes last."""
    _child(dict(map="harvest", E=9, ring=3, action_ring=2, step0=5, edge=True, calls=[dict(steps=steps, outputs="all")]))


def test_two_chains_with_supplied_actions():
    """rollout_actions, 10 envs in two chains of 5, an action ring of 3, 9 steps: the second chain's records point five envs into
    every slot -- the second pass's action slot among them."""
    _child(dict(map="harvest", E=10, ring=9, action_ring=3, chains=2, calls=[dict(steps=9, outputs="all")]))


@pytest.mark.parametrize("name,N", [("harvest25x38", 5), ("harvest", 10)])
def test_pair_kernels_no_other_test_reaches(name, N):
    """Harvest 25 x 38 with 5 agents (two 1 KiB pieces of grid per pass) and Harvest 16 x 38 with 10 agents: 9 random-action steps
    (four pairs and a single step) from a state with agents at the map's edges."""
    _child(dict(map=name, E=9, N=N, ring=9, edge=True, calls=[dict(steps=9, outputs="all")]))


def test_call_without_rewards_and_dones_then_one_with_them():
    """8 steps into a ring of 8 with observations alone -- null reward and done pointers in both passes' records: nothing is written
    there, observations and final state are the oracle's -- then 8 more steps with all three buffers."""
    _child(dict(map="harvest", E=9, ring=8, edge=True, calls=[dict(steps=8, outputs="obs"), dict(steps=8, outputs="all")]))


@pytest.mark.parametrize("N", [5, 10])
def test_cleanup_counts_leave_the_threshold_window_on_either_step(N):
    """Cleanup 25 x 18, whose pair kernels prefetch a window of the spawn thresholds by waste count (kPre) in the prologue -- one
    window for both passes.  Every env starts with its waste count AT the spawn threshold, the agents crowded on the river; 12
    scripted steps, all agents CLEAN in steps 2 and 5 -- a pair's first step and a pair's second.  The oracle's states say that in
    some env each of those steps reads its thresholds two or more counts below where the step began, i.e. out of the window's
    usual lanes (asserted before the comparison)."""
    _child(dict(map="cleanup", E=9, N=N, ring=12, threshold_start=True, calls=[dict(steps=12, outputs="all")]))


if __name__ == "__main__":
    _case(json.loads(sys.argv[1]))
