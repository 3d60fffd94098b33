"""The common path of the split coherent step kernel, both wave roles, at the smallest shapes where it can go wrong, against
oracle/pyoracle.py.  The renderer waves' window bases (the LDS base added per lane = agent) and their store-policy test
(ssd_kernels.hip, render_views_std) are what round 15 changed; the env x stride addressing of the per-env arrays and the launch-uniform cases beside the straight line
are code as it was, covered here because no test met it at these shapes.

Two of the cases need what a process reads once, when it loads the library: SSD_ENVS_PER_BLOCK (4 envs per workgroup at 9 envs:
two full workgroups and one with a single env) and the test-hook library's SSD_OBS_WT / SSD_OBS_NT.  They run this file as a
script in a child process; the others run in the test process."""
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

pytestmark = pytest.mark.gpu

HOOKS_LIB = os.path.join(ROOT, "sequential_social_dilemma_games_amd", "libssd_hip_testhooks.so")


def _split_expected():
    """The split coherent chains are the library's default; the documented knobs can turn each layer off."""
    return all(os.environ.get(k, "1") != "0" for k in ("SSD_AQL", "SSD_AQL_COHERENT", "SSD_AQL_SPLIT"))


def _assert_split(eng):
    path = eng.rollout_path()
    assert path["aql"] and path["coherent"] and path["split"] and not path["fused"], path


def _edge_state(amap, E, N):
    """Positions and orientations for N = 5 agents per env: the free cells nearest to the map's four corners and to its centre
    (so some agent is within 7 cells of every edge: every apron and the row padding are read), handed to the agents in another
    order in every env; orientations (agent + env) % 4 -- all four in every env."""
    H, W = len(amap), len(amap[0])
    free = np.array([(r, c) for r in range(H) for c in range(W) if amap[r][c] != "@"])
    spots = []
    for anchor in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
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


def _nine_env_rollout(game):
    """9 envs, one chain, 12 random-action steps from the edge state: every step's observations, rewards and dones in its own ring
    slot, and the state after the call, against the oracle."""
    import torch
    amap = K.HARVEST_MAP if game == K.GAME_HARVEST else K.CLEANUP_MAP
    E, N, steps = 9, 5, 12
    eng = VecEngine(game, amap, num_envs=E, num_agents=N, seed=11)
    ora = pyoracle.Oracle(game, amap, E, N, G.default_lut(), seed=11)
    eng.reset()
    ora.reset()
    pos, orient = _edge_state(amap, E, N)
    eng.set_state(pos=pos, orient=orient)
    ora.set_state(pos=pos, orient=orient)
    obs = torch.zeros((steps, E, N, 15, 15, 3), dtype=torch.uint8, device="cuda")
    rew = torch.zeros((steps, E, N), dtype=torch.int32, device="cuda")
    done = torch.ones((steps, E, N), dtype=torch.uint8, device="cuda")
    eng.set_rollout_chains(1)
    eng.rollout_random(steps, obs, rew, done, reset_every=0, step0=0)
    g_obs, g_rew, g_done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
    if _split_expected():
        _assert_split(eng)
    for k in range(steps):
        _, o_obs, o_rew, o_done = ora.step_random()
        assert np.array_equal(g_obs[k], o_obs), "observations of step %d differ" % k
        np.testing.assert_array_equal(g_rew[k], o_rew, err_msg="rewards of step %d" % k)
        np.testing.assert_array_equal(g_done[k], np.asarray(o_done).reshape(E, N).astype(np.uint8), err_msg="dones of step %d" % k)
    a, b = eng.get_state(), ora.get_state()
    for key in ("world", "pos", "orient", "episode", "t"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert eng.status() == 0
    eng.close()
    print("nine-env rollout ok")


def _child(game, **env_vars):
    env = dict(os.environ)
    for k in ("SSD_LIB_PATH", "SSD_OBS_WT", "SSD_OBS_NT", "SSD_ENVS_PER_BLOCK"):
        env.pop(k, None)
    env.update(env_vars)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(game)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "nine-env rollout ok" in out, out[-3000:]


@pytest.mark.parametrize("game", [K.GAME_HARVEST, K.GAME_CLEANUP])
def test_rotation_select_over_two_workgroups_and_an_odd_env(game):
    """The renderer waves pick the window-offset table per agent by the rotation's parity, from window bases computed with lane =
    agent (the test's name is the issue's: the select it was written for was measured and dropped).  Harvest and Cleanup,
    N = 5, 9 envs with 4 per workgroup, 12 steps from a state in which the five agents cover all four orientations and stand
    near every edge of the map; every step's observations."""
    if not _split_expected():
        pytest.skip("the environment turns the split coherent chains off")
    _child(game, SSD_ENVS_PER_BLOCK="4")


@pytest.mark.parametrize("hook", [dict(SSD_OBS_WT="0"), dict(SSD_OBS_WT="1"), dict(SSD_OBS_NT="1")])
def test_store_policies_of_the_renderer_stores(hook):
    """The renderer waves' store policies behind their one branch per pass of five agents, forced through the test-hook library; the
    same 9-env rollout against the oracle.  A coherent launch always stores write-through (select() sets obs_wt = 1 after the hook
    is read), so SSD_OBS_WT = 0 and 1 both run policy 1, the fall-through, and SSD_OBS_NT = 1 runs policy 3 (non-temporal
    write-back).  A renderer wave has no other policy: its test is two-way (3, else 1); policies 0 and 2 belong to the
    other kernels (non-coherent launches above 16 384 envs, float32 observations), whose code this round left as it was."""
    if not _split_expected():
        pytest.skip("the environment turns the split coherent chains off")
    _child(K.GAME_HARVEST, SSD_ENVS_PER_BLOCK="4", SSD_LIB_PATH=HOOKS_LIB, **hook)


@pytest.mark.parametrize("cfg", ["harvest_n5", "cleanup48x36_n10"])
def test_env_offsets_in_the_second_chain_with_an_env_base(cfg):
    """Existing code, new coverage: the coherent kernels' env x stride addressing where the env index is not the workgroup's: the second chain of a 2-chain
    call (e_begin != 0) of a handle with env_index_base != 0.  Ring of 3 slots; the call's last step lands in slot 2 and is compared
    (every env, the last env of the second range by name), with the rewards, the dones and the state after the call.
    Cleanup 48 x 36 with N = 10 and six shooters per env and step: every step takes two beam passes, so the second beam list
    -- behind all envs' first -- is written and read."""
    import torch
    if cfg == "harvest_n5":
        game, amap, E, N = K.GAME_HARVEST, K.HARVEST_MAP, 10, 5
    else:
        game, amap, E, N = K.GAME_CLEANUP, K.cleanup_map_48x36(), 8, 10
    steps, ring, base = 6, 3, 1000
    eng = VecEngine(game, amap, num_envs=E, num_agents=N, seed=3, env_index_base=base)
    ora = pyoracle.Oracle(game, amap, E, N, G.default_lut(), seed=3, env_base=base)
    eng.reset()
    ora.reset()
    obs = torch.zeros((ring, E, N, 15, 15, 3), dtype=torch.uint8, device="cuda")
    rew = torch.zeros((ring, E, N), dtype=torch.int32, device="cuda")
    done = torch.ones((ring, E, N), dtype=torch.uint8, device="cuda")
    eng.set_rollout_chains(2)
    rng = np.random.RandomState(5)
    a_host = None
    if N == 10:
        a_host = rng.randint(0, 7, size=(steps, E, N)).astype(np.int32)
        for k in range(steps):
            for e in range(E):
                a_host[k, e, rng.permutation(N)[:6]] = rng.randint(7, 9, size=6)      # FIRE or CLEAN
        eng.rollout_actions(torch.from_numpy(a_host).cuda(), steps, obs, rew, done, reset_every=0, step0=0)
    else:
        eng.rollout_random(steps, obs, rew, done, reset_every=0, step0=0)
    path = eng.rollout_path()
    if _split_expected():
        _assert_split(eng)
        assert path["chains"] == 2, path
    for k in range(steps):
        if a_host is not None:
            o_obs, o_rew, o_done = ora.step(a_host[k])
        else:
            _, o_obs, o_rew, o_done = ora.step_random()
    slot = (steps - 1) % ring
    assert slot == 2
    g_obs, g_rew, g_done = obs[slot].cpu().numpy(), rew[slot].cpu().numpy(), done[slot].cpu().numpy()
    assert np.array_equal(g_obs[E - 1], o_obs[E - 1]), "observations of the last env of the second range differ"
    assert np.array_equal(g_obs, o_obs), "observations differ"
    np.testing.assert_array_equal(g_rew, o_rew)
    np.testing.assert_array_equal(g_done, np.asarray(o_done).reshape(E, N).astype(np.uint8))
    a, b = eng.get_state(), ora.get_state()
    for key in ("world", "pos", "orient", "episode", "t"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert eng.status() == 0
    eng.close()


def test_launch_uniform_cases_off_the_straight_line():
    """What the coherent chains rarely meet, beside the step kernels' straight line: caller-supplied actions
    (ssd_rollout_actions), a request for the drawn actions (actions_out), and a 3-step call, which is not split -- the env waves
    render.  One short call each, from one state, against the oracle."""
    import torch
    game, amap, E, N = K.GAME_HARVEST, K.HARVEST_MAP, 9, 5
    eng = VecEngine(game, amap, num_envs=E, num_agents=N, seed=21)
    ora = pyoracle.Oracle(game, amap, E, N, G.default_lut(), seed=21)
    eng.reset()
    ora.reset()
    obs = torch.zeros((1, E, N, 15, 15, 3), dtype=torch.uint8, device="cuda")
    rew = torch.zeros((1, E, N), dtype=torch.int32, device="cuda")
    done = torch.ones((1, E, N), dtype=torch.uint8, device="cuda")
    eng.set_rollout_chains(1)
    # caller-supplied actions, absent agents among them: 4 steps (split)
    a_host = np.random.RandomState(9).randint(-1, 8, size=(4, E, N)).astype(np.int32)
    eng.rollout_actions(torch.from_numpy(a_host).cuda(), 4, obs, rew, done, reset_every=0, step0=0)
    if _split_expected():
        _assert_split(eng)
    for k in range(4):
        o_obs, o_rew, _ = ora.step(a_host[k])
    assert np.array_equal(obs[0].cpu().numpy(), o_obs), "rollout_actions: observations differ"
    np.testing.assert_array_equal(rew[0].cpu().numpy(), o_rew)
    # the drawn actions requested: one per-step launch
    acts = torch.full((E, N), -7, dtype=torch.int32, device="cuda")
    o, r, _ = eng.step_random(actions_out=acts)
    o_act, o_obs, o_rew, _ = ora.step_random()
    np.testing.assert_array_equal(acts.cpu().numpy(), o_act)
    assert np.array_equal(o.cpu().numpy(), o_obs), "step_random: observations differ"
    np.testing.assert_array_equal(r.cpu().numpy(), o_rew)
    # a 3-step call: not split, the env waves render
    eng.rollout_random(3, obs, rew, done, reset_every=0, step0=5)
    assert eng.rollout_path()["split"] is False, eng.rollout_path()
    for k in range(3):
        _, o_obs, o_rew, _ = ora.step_random()
    assert np.array_equal(obs[0].cpu().numpy(), o_obs), "3-step call: observations differ"
    np.testing.assert_array_equal(rew[0].cpu().numpy(), o_rew)
    assert not done.any()
    a, b = eng.get_state(), ora.get_state()
    for key in ("world", "pos", "orient", "episode", "t"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert eng.status() == 0
    eng.close()


if __name__ == "__main__":
    _nine_env_rollout(int(sys.argv[1]))
