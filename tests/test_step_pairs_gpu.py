"""Step pairs: the split coherent chains advance their envs by two steps per launch (ssd_rollout_plan.hpp, Schedule, sent by ssd_rollout.hip, rollout_aql; the step-pair
kernel, ssd_kernels.hip kModeStepPair).  Every case runs rollout calls against oracle/pyoracle.py -- every step's observations,
rewards and dones as far as the ring still holds them, and the state after the call -- and asserts what ssd_rollout_path()
reports.  Shapes are the smallest at which the form can go wrong: 9 envs at 4 per workgroup (two full workgroups and one with a
single env), odd step counts, rings of 1 and 3 slots, resets on either step of a would-be pair, a second call on the same handle.

Harvest's maps and Cleanup's shipped map have step-pair kernels; Cleanup 48 x 36 keeps single steps by rule (its pair kernel
does not fit eight waves per SIMD without scratch memory): its case asserts the same results and that `pairs` is off.

Cases that need what a process reads once when it loads the library (SSD_ENVS_PER_BLOCK, the test-hook library's SSD_AQL_PAIRS)
run this file as a script in a child process."""
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
from test_split_common_path_gpu import HOOKS_LIB, _edge_state, _split_expected  # noqa: E402

pytestmark = pytest.mark.gpu

FIRE, CLEAN = 7, 8


def _map(name):
    return {"harvest": (K.GAME_HARVEST, K.HARVEST_MAP), "cleanup": (K.GAME_CLEANUP, K.CLEANUP_MAP),
            "cleanup48x36": (K.GAME_CLEANUP, K.cleanup_map_48x36())}[name]


def _assert_path(eng, pairs, chains=None):
    path = eng.rollout_path()
    assert path["aql"] and path["coherent"] and path["split"] and not path["fused"], path
    assert path["pairs"] is pairs, path
    if chains is not None:
        assert path["chains"] == chains, path


def _scripted(name, E, N, slots):
    """Actions [slots][E][N] that force what random actions almost never produce.  Harvest, 5 agents: slots 0 and 2 have all five
    agents FIRE in the even / odd envs (more shooters than one beam pass has groups: the step leaves an overlay snapshot).  Cleanup
    (either map), 10 agents: six shooters per env in every slot (two beam passes, the second beam list), FIRE and CLEAN mixed -- and in
    slot 1 all ten CLEAN or FIRE (three passes: a snapshot)."""
    rng = np.random.RandomState(17)
    a = rng.randint(0, 7, size=(slots, E, N)).astype(np.int32)
    for s in range(slots):
        for e in range(E):
            if N == 5:
                if s != 1 and (e + s // 2) % 2 == 0:
                    a[s, e, :] = FIRE
            else:
                a[s, e, rng.permutation(N)[:6]] = rng.randint(FIRE, CLEAN + 1, size=6)
                if s == 1 and e % 2 == 0:
                    a[s, e, :] = rng.randint(FIRE, CLEAN + 1, size=N)
    return a


def _case(cfg):
    """One handle, one oracle, `calls` rollout calls of `steps` steps each; then (per_call_step) a per-call step().  After every
    call each ring slot is compared with the last step that mapped to it."""
    import torch
    name, E, N = cfg["map"], cfg["E"], cfg.get("N", 5)
    steps, ring, calls = cfg["steps"], cfg["ring"], cfg.get("calls", 1)
    reset_every, step0, horizon = cfg.get("reset_every", 0), cfg.get("step0", 0), cfg.get("horizon", 0)
    game, amap = _map(name)
    eng = VecEngine(game, amap, num_envs=E, num_agents=N, seed=cfg.get("seed", 11))
    ora = pyoracle.Oracle(game, amap, E, N, G.default_lut(), seed=cfg.get("seed", 11))
    eng.reset()
    ora.reset()
    if cfg.get("edge"):
        pos, orient = _edge_state(amap, E, N)
        eng.set_state(pos=pos, orient=orient)
        ora.set_state(pos=pos, orient=orient)
    if horizon:
        eng.set_horizon(horizon)
    obs = torch.zeros((ring, E, N, 15, 15, 3), dtype=torch.uint8, device="cuda")
    rew = torch.zeros((ring, E, N), dtype=torch.int32, device="cuda")
    done = torch.full((ring, E, N), 7, dtype=torch.uint8, device="cuda")
    eng.set_rollout_chains(cfg.get("chains", 1))
    a_host = _scripted(name, E, N, cfg["action_ring"]) if cfg.get("action_ring") else None
    a_dev = torch.from_numpy(a_host).cuda() if a_host is not None else None
    for call in range(calls):
        s0 = step0 + call * steps
        if a_dev is not None:
            eng.rollout_actions(a_dev, steps, obs, rew, done, reset_every=reset_every, step0=s0)
        else:
            eng.rollout_random(steps, obs, rew, done, reset_every=reset_every, step0=s0)
        _assert_path(eng, cfg["pairs"], cfg.get("chains", 1))
        g_obs, g_rew, g_done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        want = {}
        for k in range(s0, s0 + steps):
            if reset_every and k % reset_every == 0:
                ora.reset()
            if a_host is not None:
                o_obs, o_rew, _ = ora.step(a_host[k % a_host.shape[0]])
            else:
                _, o_obs, o_rew, _ = ora.step_random()
            t = ora.get_state()["t"]
            o_done = np.repeat(((t >= horizon) if horizon else np.zeros_like(t, bool)).astype(np.uint8)[:, None], N, 1)
            want[k % ring] = (k, o_obs.copy(), o_rew.copy(), o_done)
        for slot, (k, o_obs, o_rew, o_done) in sorted(want.items()):
            assert np.array_equal(g_obs[slot], o_obs), "call %d: observations of step %d (slot %d) differ" % (call, k, slot)
            np.testing.assert_array_equal(g_rew[slot], o_rew, err_msg="call %d: rewards of step %d" % (call, k))
            np.testing.assert_array_equal(g_done[slot], o_done, err_msg="call %d: dones of step %d" % (call, k))
        if horizon:
            assert any(w[3].any() for w in want.values()) and not all(w[3].all() for w in want.values()), "the horizon must fire on some steps only"
        a, b = eng.get_state(), ora.get_state()
        for key in ("world", "pos", "orient", "episode", "t"):
            np.testing.assert_array_equal(a[key], b[key], err_msg="call %d: %s" % (call, key))
    if cfg.get("per_call_step"):
        o, r, _ = eng.step_random()
        _, o_obs, o_rew, _ = ora.step_random()
        assert np.array_equal(o.cpu().numpy(), o_obs), "step() after the calls: observations differ"
        np.testing.assert_array_equal(r.cpu().numpy(), o_rew)
        a, b = eng.get_state(), ora.get_state()
        for key in ("world", "pos", "orient", "episode", "t"):
            np.testing.assert_array_equal(a[key], b[key], err_msg="after step(): %s" % key)
    status = eng.status()
    eng.close()
    assert status == 0, status
    print("step-pair case ok")


def _child(cfg, **env_vars):
    env = dict(os.environ)
    for k in ("SSD_LIB_PATH", "SSD_ENVS_PER_BLOCK", "SSD_AQL_PAIRS"):
        env.pop(k, None)
    env.update(env_vars)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(cfg)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "step-pair case ok" in out, out[-3000:]


@pytest.fixture(autouse=True)
def _needs_split():
    if not _split_expected():
        pytest.skip("the environment turns the split coherent chains off")


@pytest.mark.parametrize("steps", [12, 13])
@pytest.mark.parametrize("name", ["harvest", "cleanup"])
def test_plain_rollout_over_two_workgroups_and_an_odd_env(name, steps):
    """Shipped maps, N = 5, 9 envs at 4 per workgroup, one chain, from the edge state; 12 steps (six pairs) and 13 (the odd
    remainder: a single step whose launch renders the pair before it); ring = steps: every step's outputs and the final state."""
    _child(dict(map=name, E=9, steps=steps, ring=steps, edge=True, pairs=True), SSD_ENVS_PER_BLOCK="4")


@pytest.mark.parametrize("ring", [1, 3])
def test_ring_sizes(ring):
    """8 steps into a ring of 1 (a pair's two steps land in one slot, the second over the first) and of 3 (pairs straddle the
    ring's wrap): every slot holds the last step that maps to it."""
    _case(dict(map="harvest", E=9, steps=8, ring=ring, edge=True, pairs=True))


def test_resets_inside_the_call():
    """reset_every = 5 from step0 = 3, 14 steps, horizon 3: steps 3 4 | reset 5 6 7 8 9 | reset 10 .. 14 | reset 15 16.  Resets fall
    where a pair's first and second step would be, a single step precedes each later reset, and a renderer-only launch delivers
    the launch ahead of every reset -- a pair's two steps (before step 5) or a single step's (before 10 and 15)."""
    _case(dict(map="harvest", E=9, steps=14, ring=17, reset_every=5, step0=3, horizon=3, pairs=True))


def test_repeat_calls_then_a_per_call_step():
    """Two calls of 7 steps back to back on one handle -- three pairs and a single step each, so the second call starts from the
    other buffer of the state pair and the other mid set -- then a per-call step() and get_state."""
    _case(dict(map="harvest", E=9, steps=7, ring=7, calls=2, per_call_step=True, pairs=True))


def test_two_chains():
    """10 envs in two chains of 5 (where the device's pool has two queues): the second chain's env offsets into the mid sets."""
    import torch
    probe = VecEngine(K.GAME_HARVEST, K.HARVEST_MAP, num_envs=10, num_agents=5, seed=1)
    probe.reset()
    probe.set_rollout_chains(2)
    probe.rollout_random(4, torch.zeros((1, 10, 5, 15, 15, 3), dtype=torch.uint8, device="cuda"), None, None)
    pool = probe.rollout_path()["pool"]
    probe.close()
    if pool < 2:
        pytest.skip("the device's pool has one dispatch queue")
    _case(dict(map="harvest", E=10, steps=9, ring=9, chains=2, pairs=True))


def test_scripted_actions_force_snapshots_on_either_step():
    """rollout_actions, Harvest, 5 agents, an action ring of 3 with 8 steps: all five agents fire (an overlay snapshot instead of
    a beam list) in slot 0 of the even envs and slot 2 of the odd ones -- steps 0, 3 and 6 / 2 and 5: a pair's first step and its
    second, in some env of every launch."""
    _case(dict(map="harvest", E=9, steps=8, ring=8, action_ring=3, pairs=True))


def test_cleanup_ten_agents_scripted_actions_two_beam_lists_and_snapshots():
    """rollout_actions, Cleanup's shipped map with 10 agents, an action ring of 3 with 8 steps: six shooters per env in every step,
    FIRE and CLEAN mixed (two beam passes: the second beam list, on a pair's first step and on its second), and in slot 1 -- steps
    1, 4 and 7: a pair's second step, its first, its second -- all ten shooting in the even envs (three passes, CLEAN among them:
    an overlay snapshot)."""
    _case(dict(map="cleanup", E=6, N=10, steps=8, ring=8, action_ring=3, pairs=True))


def test_cleanup_48x36_scripted_actions_keep_single_steps():
    """Cleanup 48 x 36, 10 agents, scripted actions (six shooters per env: the second beam list; all ten: a snapshot; CLEAN among
    them), an action ring of 3 with 8 steps: Cleanup has no step-pair kernel, the call runs single steps -- same results."""
    _case(dict(map="cleanup48x36", E=6, N=10, steps=8, ring=8, action_ring=3, pairs=False))


def test_knob_off_keeps_single_steps():
    """SSD_AQL_PAIRS=0 (test-hook library): the same 13-step rollout in single steps, same results, `pairs` off."""
    _child(dict(map="harvest", E=9, steps=13, ring=13, edge=True, pairs=False), SSD_ENVS_PER_BLOCK="4", SSD_LIB_PATH=HOOKS_LIB, SSD_AQL_PAIRS="0")
    _child(dict(map="harvest", E=9, steps=13, ring=13, edge=True, pairs=True), SSD_ENVS_PER_BLOCK="4", SSD_LIB_PATH=HOOKS_LIB)


if __name__ == "__main__":
    _case(json.loads(sys.argv[1]))
