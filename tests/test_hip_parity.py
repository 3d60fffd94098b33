"""GPU parity tests proper: the HIP path, called through the C ABI (libssd_hip.so), against
(a) the golden transitions recorded from the reference and (b) the C oracle on the same seeded
inputs.  Integer / byte work: the bar is bit-exact."""
import numpy as np
import pytest

import golden_util as G
from oracle import pyoracle
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd.engine import VecEngine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", G.group_names())
def test_hip_replays_reference_transitions(name):
    g = G.load(name)
    eng = VecEngine(g.game, g.map, num_envs=1, num_agents=g.N, view_len=g.view_len, seed=g.seed,
                    env_index_base=g.env, keep_beams=True, harvest_thresholds=g.harvest_thresholds,
                    cleanup_thresholds=g.cleanup_thresholds)     # (None but for the spawn-table fixtures, which carry theirs)
    s = g.steps
    zero_beam = np.zeros((1, eng.H, eng.W), np.int8)
    for k in range(g.n_steps):
        eng.set_state(world=s["pre_world"][k][None], beam=zero_beam, pos=s["pre_pos"][k][None],
                      orient=s["pre_orient"][k][None], episode=np.array([s["episode"][k]], np.uint32),
                      t=np.array([s["t"][k] - 1], np.uint32))
        obs, rew, done = eng.step_host(s["act"][k][None], order=s["order"][k][None])
        st = eng.get_state()
        where = "%s step %d" % (name, k)
        np.testing.assert_array_equal(st["pos"][0], s["pos"][k], err_msg=where)
        np.testing.assert_array_equal(st["orient"][0], s["orient"][k], err_msg=where)
        np.testing.assert_array_equal(st["world"][0], s["world"][k], err_msg=where)
        np.testing.assert_array_equal(st["beam"][0], s["beam"][k], err_msg=where)
        np.testing.assert_array_equal(rew[0], s["rew"][k], err_msg=where)
        np.testing.assert_array_equal(obs[0], s["obs"][k], err_msg=where)
        assert st["t"][0] == s["t"][k] and not done.any()
    r = g.resets
    for k in range(g.n_resets):
        ep = int(r["episode"][k])
        eng.set_state(episode=np.array([(ep - 1) & 0xFFFFFFFF], np.uint32))
        obs = eng.reset_host()
        st = eng.get_state()
        where = "%s reset %d" % (name, k)
        assert st["episode"][0] == ep and st["t"][0] == 0
        np.testing.assert_array_equal(st["pos"][0], r["pos"][k], err_msg=where)
        np.testing.assert_array_equal(st["orient"][0], r["orient"][k], err_msg=where)
        np.testing.assert_array_equal(st["world"][0], r["world"][k], err_msg=where)
        np.testing.assert_array_equal(obs[0], r["obs"][k], err_msg=where)
    assert eng.status() == 0


CASES = [
    # game, map, E, N, view_len, steps
    (K.GAME_HARVEST, K.HARVEST_MAP, 257, 5, 7, 60),          # E % 4 != 0 exercises the ragged last workgroup
    (K.GAME_CLEANUP, K.CLEANUP_MAP, 128, 5, 7, 60),
    (K.GAME_CLEANUP, K.CLEANUP_MAP, 66, 10, 7, 40),
    (K.GAME_HARVEST, K.harvest_map_25x38(), 64, 5, 7, 40),
    (K.GAME_CLEANUP, K.cleanup_map_48x36(), 33, 10, 7, 40),
    (K.GAME_HARVEST, ['@@@@@@@', '@PAPAP@', '@APAPA@', '@PAPAP@', '@@@@@@@'], 512, 6, 2, 80),
    (K.GAME_CLEANUP, ['@@@@@@@', '@PHBPP@', '@RPBPH@', '@PHBPP@', '@@@@@@@'], 512, 5, 3, 80),
    (K.GAME_HARVEST, ['@@@@@@@', '@PPPPP@', '@PPPPP@', '@PPPPP@', '@@@@@@@'], 300, 13, 1, 60),
    (K.GAME_HARVEST, K.HARVEST_MAP, 3, 0, 7, 5),             # no agents
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_hip_rollout_matches_oracle(case):
    """Free-running random-action rollouts (device-drawn actions) on E envs: every state array
    and output must equal the oracle's at every step, including a masked mid-rollout reset."""
    game, amap, E, N, v, steps = CASES[case]
    seed, base = 1234 + case, 1000 * case
    eng = VecEngine(game, amap, num_envs=E, num_agents=N, view_len=v, seed=seed, env_index_base=base, keep_beams=True)
    ora = pyoracle.Oracle(game, amap, E, N, G.default_lut(), view_len=v, seed=seed, env_base=base)
    np.testing.assert_array_equal(eng.reset_host(), ora.reset())

    def same_state(where):
        a, b = eng.get_state(), ora.get_state()
        for k in ("world", "beam", "pos", "orient", "episode", "t"):
            np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (where, k))

    same_state("after reset")
    for s in range(steps):
        act, obs, rew, done = eng.step_random_host()
        o_act, o_obs, o_rew, o_done = ora.step_random()
        np.testing.assert_array_equal(act, o_act, err_msg="actions step %d" % s)
        np.testing.assert_array_equal(rew, o_rew, err_msg="rew step %d" % s)
        np.testing.assert_array_equal(obs, o_obs, err_msg="obs step %d" % s)
        np.testing.assert_array_equal(done, o_done)
        same_state("step %d" % s)
        if s == steps // 2:
            mask = (np.arange(E) % 3 == 1).astype(np.uint8)
            h_obs, o_obs = eng.reset_host(mask), ora.reset(mask)
            sel = mask.astype(bool)
            np.testing.assert_array_equal(h_obs[sel], o_obs[sel])
            assert not h_obs[~sel].any()                     # rows of envs that were not reset stay untouched
            same_state("after masked reset")
    np.testing.assert_array_equal(eng.observe_host(rotate=True), ora.observe(True))
    np.testing.assert_array_equal(eng.observe_host(rotate=False), ora.observe(False))
    assert eng.status() == 0


def test_hip_explicit_actions_orders_and_subsets():
    """Arbitrary action-dict orders and subsets (tests/test_envs.py:437-438,594-597 style) on a
    crowded map, given as actions + order arrays."""
    amap = ['@@@@@@@', '@PPPPP@', '@PPPPP@', '@PPPPP@', '@@@@@@@']
    E, N = 256, 7
    rng = np.random.RandomState(7)
    eng = VecEngine(K.GAME_HARVEST, amap, num_envs=E, num_agents=N, view_len=2, seed=99, keep_beams=True)
    ora = pyoracle.Oracle(K.GAME_HARVEST, amap, E, N, G.default_lut(), view_len=2, seed=99)
    eng.reset_host(); ora.reset()
    for s in range(60):
        act = rng.randint(0, 8, size=(E, N)).astype(np.int32)
        order = np.full((E, N), 0xFF, np.uint8)
        for e in range(E):
            k = rng.randint(0, N + 1)
            perm = rng.permutation(N)[:k]
            order[e, :k] = perm
            absent = np.setdiff1d(np.arange(N), perm)
            act[e, absent] = -1
        obs, rew, done = eng.step_host(act, order)
        o_obs, o_rew, _ = ora.step(act, order)
        np.testing.assert_array_equal(rew, o_rew, err_msg="step %d" % s)
        np.testing.assert_array_equal(obs, o_obs, err_msg="step %d" % s)
        a, b = eng.get_state(), ora.get_state()
        for k in ("world", "beam", "pos", "orient"):
            np.testing.assert_array_equal(a[k], b[k], err_msg="step %d %s" % (s, k))
    assert eng.status() == 0


def test_device_tensor_api_matches_host_api():
    import torch
    E, N = 64, 5
    a = VecEngine(K.GAME_HARVEST, None, num_envs=E, num_agents=N, seed=5)
    b = VecEngine(K.GAME_HARVEST, None, num_envs=E, num_agents=N, seed=5)
    obs_a = a.reset()
    obs_b = b.reset_host()
    assert np.array_equal(obs_a.cpu().numpy(), obs_b)
    rng = np.random.RandomState(0)
    for s in range(20):
        act = rng.randint(0, 8, size=(E, N)).astype(np.int32)
        o, r, d = a.step(torch.from_numpy(act).cuda())
        ho, hr, hd = b.step_host(act)
        assert np.array_equal(o.cpu().numpy(), ho) and np.array_equal(r.cpu().numpy(), hr)
        assert np.array_equal(d.cpu().numpy(), hd)
    assert a.status() == 0 and b.status() == 0


def test_bad_action_sets_status_and_is_ignored():
    eng = VecEngine(K.GAME_HARVEST, None, num_envs=2, num_agents=2, seed=1)
    eng.reset_host()
    before = eng.get_state()
    eng.step_host(np.array([[8, 4], [4, 99]], np.int32))     # CLEAN does not exist in Harvest (KeyError in the reference)
    assert eng.status() & 1
    after = eng.get_state()
    np.testing.assert_array_equal(before["pos"], after["pos"])


def test_render_full_matches_lut_of_overlay():
    eng = VecEngine(K.GAME_CLEANUP, None, num_envs=3, num_agents=5, seed=3, keep_beams=True)
    ora = pyoracle.Oracle(K.GAME_CLEANUP, K.CLEANUP_MAP, 3, 5, G.default_lut(), seed=3)
    eng.reset_host(); ora.reset()
    for _ in range(10):
        eng.step_random_host(); ora.step_random()
    st = ora.get_state()
    lut = G.default_lut()
    for e in range(3):
        grid = st["world"][e].copy()
        for i in range(5):
            grid[st["pos"][e, i, 0], st["pos"][e, i, 1]] = ord("12345"[i])
        grid = np.where(st["beam"][e] != 0, st["beam"][e], grid)
        np.testing.assert_array_equal(eng.render_full(e), lut[grid.astype(np.int64)])


@pytest.mark.parametrize("game", ["harvest", "cleanup"])
def test_render_frames_batch_matches_oracle_overlay(game):
    """ssd_render_frames: every env's full frame in one launch (device tensor and host array), sub-ranges, and the
    single-frame entry point -- all equal to the colour table applied to the oracle's overlay (map_env.py:280-339)."""
    import torch
    gid, amap = (K.GAME_HARVEST, K.HARVEST_MAP) if game == "harvest" else (K.GAME_CLEANUP, K.CLEANUP_MAP)
    E, N = 37, 5
    eng = VecEngine(gid, None, num_envs=E, num_agents=N, seed=11, keep_beams=True)
    ora = pyoracle.Oracle(gid, amap, E, N, G.default_lut(), seed=11)
    eng.reset_host(); ora.reset()
    for _ in range(25):
        eng.step_random_host(); ora.step_random()
    st = ora.get_state()
    lut = G.default_lut()
    want = np.zeros((E, eng.H, eng.W, 3), np.uint8)
    for e in range(E):
        grid = st["world"][e].copy()
        for i in range(N):
            grid[st["pos"][e, i, 0], st["pos"][e, i, 1]] = ord("12345"[i])
        grid = np.where(st["beam"][e] != 0, st["beam"][e], grid)
        want[e] = lut[grid.astype(np.int64)]
    dev = eng.render_frames()
    assert dev.is_cuda and tuple(dev.shape) == want.shape
    np.testing.assert_array_equal(dev.cpu().numpy(), want)
    np.testing.assert_array_equal(eng.render_frames(host=True), want)
    np.testing.assert_array_equal(eng.render_frames(5, 9, host=True), want[5:14])
    out = torch.zeros((3, eng.H, eng.W, 3), dtype=torch.uint8, device=dev.device)
    assert eng.render_frames(E - 3, 3, out=out) is out
    np.testing.assert_array_equal(out.cpu().numpy(), want[E - 3:])
    np.testing.assert_array_equal(eng.render_full(E - 1), want[E - 1])
    assert eng.render_frames(4, 0, host=True).shape == (0, eng.H, eng.W, 3)
    with pytest.raises(ValueError):
        eng.render_frames(30, 8)


def test_vector_env_horizon_auto_reset_matches_oracle():
    """SSDVectorEnv: done at t == horizon, masked auto-reset, obs of finished envs = first obs of the next episode."""
    import torch
    from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv
    E, N, Hz = 48, 5, 7
    venv = SSDVectorEnv(K.GAME_CLEANUP, E, N, horizon=Hz, seed=11)
    ora = pyoracle.Oracle(K.GAME_CLEANUP, K.CLEANUP_MAP, E, N, G.default_lut(), seed=11)
    np.testing.assert_array_equal(venv.reset().cpu().numpy(), ora.reset())
    rng = np.random.RandomState(3)
    # put half of the envs out of phase so that they finish at different steps
    half = (np.arange(E) % 2).astype(np.uint8)
    for _ in range(3):
        act = rng.randint(0, 9, size=(E, N)).astype(np.int32)
        venv.step(torch.from_numpy(act).cuda()); ora.step(act)
    venv.engine.reset(mask=torch.from_numpy(half).cuda(), obs=venv._out[0]); ora.reset(half)
    for s in range(20):
        act = rng.randint(0, 9, size=(E, N)).astype(np.int32)
        obs, rew, done = venv.step(torch.from_numpy(act).cuda())
        o_obs, o_rew, _ = ora.step(act)
        t = ora.get_state()["t"]
        o_done = (t >= Hz)
        if o_done.any():
            r_obs = ora.reset(o_done.astype(np.uint8))
            o_obs[o_done] = r_obs[o_done]
        np.testing.assert_array_equal(done.cpu().numpy(), np.repeat(o_done[:, None], N, 1).astype(np.uint8), err_msg="step %d" % s)
        np.testing.assert_array_equal(rew.cpu().numpy(), o_rew)
        np.testing.assert_array_equal(obs.cpu().numpy(), o_obs, err_msg="step %d" % s)
    a, b = venv.engine.get_state(), ora.get_state()
    for k in ("world", "pos", "orient", "episode", "t"):
        np.testing.assert_array_equal(a[k], b[k])
    f = SSDVectorEnv.to_float(obs)
    assert f.shape == (E * N, 15, 15, 3) and f.dtype == torch.float32
    np.testing.assert_allclose(f.cpu().numpy().reshape(E, N, 15, 15, 3), (o_obs.astype(np.float64) - 128.0) / 255.0, rtol=0, atol=1e-7)


def test_vector_env_base_env_style_dicts():
    from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv
    venv = SSDVectorEnv(K.GAME_HARVEST, 3, 2, horizon=2, seed=4)
    o, r, d, i, _ = venv.poll()
    assert set(o) == {0, 1, 2} and set(o[0]) == {'agent-0', 'agent-1'} and o[0]['agent-0'].shape == (15, 15, 3)
    venv.send_actions({e: {'agent-0': 4, 'agent-1': 5} for e in range(3)})
    o, r, d, i, _ = venv.poll()
    assert d[0]["__all__"] is False
    venv.send_actions({e: {'agent-0': 4} for e in range(3)})
    o, r, d, i, _ = venv.poll()
    assert all(d[e]["__all__"] for e in range(3))                  # horizon 2 reached, envs were reset
    assert (venv.engine.get_state()["t"] == 0).all()
    first = venv.try_reset(1)
    assert first['agent-1'].shape == (15, 15, 3)


def test_large_cleanup_map_with_active_spawning_exercises_long_cell_lists():
    """Synthetic 48x36 Cleanup (412 apple points, 476 waste cells: more than the 192 list entries a wave keeps
    in registers).  Random rollouts there never clean below the 0.4 density threshold, so most waste is removed
    by hand first: apple and waste respawn then run on the long lists, against the oracle at every step."""
    amap = K.cleanup_map_48x36()
    E, N = 24, 10
    eng = VecEngine(K.GAME_CLEANUP, amap, num_envs=E, num_agents=N, seed=21, keep_beams=True)
    ora = pyoracle.Oracle(K.GAME_CLEANUP, amap, E, N, G.default_lut(), seed=21)
    eng.reset_host(); ora.reset()
    world = ora.get_state()["world"].copy()
    rng = np.random.RandomState(5)
    for e in range(E):
        hs = np.argwhere(world[e] == ord('H'))
        keep = rng.rand(len(hs)) < (0.02 + 0.03 * e)            # densities from ~0.01 to ~0.35 across envs
        for (r, c), k in zip(hs, keep):
            if not k:
                world[e, r, c] = ord('R')
    eng.set_state(world=world); ora.set_state(world=world)
    spawned_a = spawned_h = 0
    for s in range(60):
        act, obs, rew, _ = eng.step_random_host()
        o_act, o_obs, o_rew, _ = ora.step_random()
        a, b = eng.get_state(), ora.get_state()
        np.testing.assert_array_equal(a["world"], b["world"], err_msg="world step %d" % s)
        np.testing.assert_array_equal(obs, o_obs, err_msg="obs step %d" % s)
        np.testing.assert_array_equal(rew, o_rew)
        spawned_a += int(((a["world"] == ord('A')) & (world != ord('A'))).sum())
        spawned_h += int(((a["world"] == ord('H')) & (world != ord('H'))).sum())
        world = a["world"].copy()
    assert spawned_a > 200 and spawned_h > 100, (spawned_a, spawned_h)
    # apples appeared in the second half of the apple list and waste in the second half of the waste list
    cells_a = np.argwhere(np.array([[ch == 'B' for ch in row] for row in amap]))
    late = cells_a[300:]
    assert (world[:, late[:, 0], late[:, 1]] == ord('A')).any()
    assert eng.status() == 0


def test_stepping_before_reset_and_border_positions_are_safe():
    eng = VecEngine(K.GAME_HARVEST, None, num_envs=8, num_agents=5, seed=1)
    obs, rew, done = eng.step_random_host()[1:]                 # never reset: agents sit on (1,1), world is blank
    st = eng.get_state()
    assert (st["pos"] >= 0).all() and (st["pos"][..., 0] < 16).all() and (st["pos"][..., 1] < 38).all()
    bad = st["pos"].copy(); bad[0, 0] = [0, 5]
    with pytest.raises(Exception):
        eng.set_state(pos=bad)


def _random_map(rng, H, W, game, n_spawn):
    """Wall-closed random map with interior walls, apple / waste / river / stream cells and spawn points."""
    g = np.full((H, W), ' ', dtype='<U1')
    g[0, :] = g[-1, :] = '@'; g[:, 0] = g[:, -1] = '@'
    inner = [(r, c) for r in range(1, H - 1) for c in range(1, W - 1)]
    rng.shuffle(inner)
    k = 0
    for r, c in inner[k:k + n_spawn]:
        g[r, c] = 'P'
    k += n_spawn
    n = len(inner)
    for ch, frac in (('@', 0.06), ('A' if game == K.GAME_HARVEST else 'B', 0.25)) + \
            ((('H', 0.10), ('R', 0.12), ('S', 0.03)) if game == K.GAME_CLEANUP else ()):
        m = int(frac * n)
        for r, c in inner[k:k + m]:
            g[r, c] = ch
        k += m
    return ["".join(row) for row in g]


UNUSUAL = [
    # game, H, W, E, N, view_len, beam_len, steps
    (K.GAME_HARVEST, 12, 14, 37, 64, 3, 5, 25),      # 64 agents: every lane of the wave is an agent
    (K.GAME_CLEANUP, 12, 14, 37, 33, 2, 7, 25),
    (K.GAME_HARVEST, 64, 64, 5, 20, 7, 5, 20),       # largest supported map (4096 cells)
    (K.GAME_CLEANUP, 64, 64, 5, 20, 7, 3, 20),
    (K.GAME_HARVEST, 9, 40, 130, 4, 15, 21, 25),     # widest view (31 x 31) and longest beam
    (K.GAME_CLEANUP, 40, 9, 130, 4, 0, 1, 25),       # 1 x 1 view, beam of one cell
    (K.GAME_CLEANUP, 20, 20, 64, 7, 7, 5, 60),
    (K.GAME_CLEANUP, 24, 8, 49, 12, 8, 1, 40),       # beam of one cell, 12 agents: more shooters than the 8 slots a cell's mask holds
    (K.GAME_CLEANUP, 14, 14, 40, 16, 3, 2, 40),      # 10 shooters' worth of lanes, 16 agents: several groups of 8
]


@pytest.mark.parametrize("case", range(len(UNUSUAL)))
def test_unusual_configurations_match_the_oracle(case):
    game, H, W, E, N, v, L, steps = UNUSUAL[case]
    rng = np.random.RandomState(100 + case)
    amap = _random_map(rng, H, W, game, n_spawn=N + 3)
    eng = VecEngine(game, amap, num_envs=E, num_agents=N, view_len=v, beam_len=L, seed=case, keep_beams=True)
    ora = pyoracle.Oracle(game, amap, E, N, G.default_lut(), view_len=v, beam_len=L, seed=case)
    np.testing.assert_array_equal(eng.reset_host(), ora.reset())
    if game == K.GAME_CLEANUP:                       # thin the waste out so that spawning is active in most envs
        world = ora.get_state()["world"].copy()
        hs = np.argwhere(world == ord('H'))
        drop = rng.rand(len(hs)) < 0.8
        world[hs[drop, 0], hs[drop, 1], hs[drop, 2]] = ord('R')
        eng.set_state(world=world); ora.set_state(world=world)
    for s in range(steps):
        if s % 3 == 2:                               # explicit random orders / subsets every third step
            act = rng.randint(0, 8 if game == K.GAME_HARVEST else 9, size=(E, N)).astype(np.int32)
            order = np.full((E, N), 0xFF, np.uint8)
            for e in range(E):
                k = rng.randint(0, N + 1)
                perm = rng.permutation(N)[:k]
                order[e, :k] = perm
                act[e, np.setdiff1d(np.arange(N), perm)] = -1
            obs, rew, _ = eng.step_host(act, order)
            o_obs, o_rew, _ = ora.step(act, order)
        else:
            _, obs, rew, _ = eng.step_random_host()
            _, o_obs, o_rew, _ = ora.step_random()
        np.testing.assert_array_equal(rew, o_rew, err_msg="rewards step %d" % s)
        np.testing.assert_array_equal(obs, o_obs, err_msg="obs step %d" % s)
        a, b = eng.get_state(), ora.get_state()
        for key in ("world", "beam", "pos", "orient"):
            np.testing.assert_array_equal(a[key], b[key], err_msg="%s step %d" % (key, s))
    assert eng.status() == 0


def test_limits_are_rejected_with_messages():
    from sequential_social_dilemma_games_amd import _capi
    wall = ['@' * 66] + ['@' + ' ' * 64 + '@'] * 64 + ['@' * 66]
    for kw, needle in ((dict(ascii_map=wall), "4096 cells"), (dict(num_agents=65), "num_agents"),
                       (dict(view_len=16), "view_len"), (dict(beam_len=22), "beam_len")):
        args = dict(game=K.GAME_HARVEST, ascii_map=None, num_envs=1, num_agents=1)
        args.update(kw)
        with pytest.raises(_capi.SsdError) as ei:
            VecEngine(**args)
        assert needle in str(ei.value), str(ei.value)


def _f32_of(u8):
    """map_env.py:199 in float64, cast to the declared float32 observation space (harvest.py:39-40)."""
    return ((u8.astype(np.float64) - 128.0) / 255.0).astype(np.float32)


def test_float32_observation_mode_is_the_cast_of_the_reference_float64():
    """SSD_OBS_F32: the kernel writes float32((u8 - 128.0) / 255.0) -- the reference's float64 observation
    (map_env.py:199) cast to its declared float32 space -- for step, reset, masked reset and observe.  The expectation is
    the ORACLE's uint8 observation pushed through that formula (not another HIP engine's output); bit-exact, ragged E."""
    import torch
    for game, E, N in ((K.GAME_HARVEST, 259, 5), (K.GAME_CLEANUP, 64, 10)):
        amap = K.HARVEST_MAP if game == K.GAME_HARVEST else K.CLEANUP_MAP
        a = VecEngine(game, None, num_envs=E, num_agents=N, seed=8, keep_beams=True)
        ora = pyoracle.Oracle(game, amap, E, N, G.default_lut(), seed=8)
        fa = a.alloc_outputs(float32=True)
        a.reset(obs=fa[0])
        assert np.array_equal(fa[0].cpu().numpy(), _f32_of(ora.reset()))
        for s in range(12):
            a.step_random(out=fa)
            _, o_obs, o_rew, _ = ora.step_random()
            assert np.array_equal(fa[0].cpu().numpy(), _f32_of(o_obs)), "step %d" % s
            np.testing.assert_array_equal(fa[1].cpu().numpy(), o_rew)
        got = a.observe(rotate=False, obs=torch.empty_like(fa[0]))
        assert np.array_equal(got.cpu().numpy(), _f32_of(ora.observe(rotate=False)))
        got = a.observe(rotate=True, obs=torch.empty_like(fa[0]))
        assert np.array_equal(got.cpu().numpy(), _f32_of(ora.observe(rotate=True)))
        mask_np = (np.arange(E) % 2).astype(np.uint8)
        mask = torch.from_numpy(mask_np).cuda()
        before = fa[0].clone()
        a.reset(mask=mask, obs=fa[0])
        o_reset = ora.reset(mask_np)
        assert np.array_equal(fa[0].cpu().numpy()[mask_np != 0], _f32_of(o_reset[mask_np != 0]))
        assert torch.equal(fa[0][~mask.bool()], before[~mask.bool()])          # rows of envs that were not reset stay
        st, so = a.get_state(), ora.get_state()
        for k in ("world", "pos", "orient", "episode", "t"):
            np.testing.assert_array_equal(st[k], so[k], err_msg=k)
        assert a.status() == 0


@pytest.mark.parametrize("view_len", [0, 1, 2, 4, 9, 15])
def test_float32_observations_of_other_view_sizes(view_len):
    """The float32 stores are laid out by float index (four consecutive floats of an agent's block per lane and store, so a
    store instruction covers contiguous memory): views whose V*V*3 is below one store (3, 27, 75 floats), around one or a
    few (243, 1083) and the largest (31 x 31: 2883 floats, 12 stores per agent) against the oracle's observations."""
    rng = np.random.default_rng(100 + view_len)
    amap = _random_map(rng, 11, 13, K.GAME_CLEANUP, 8)
    E, N = 37, 6
    a = VecEngine(K.GAME_CLEANUP, amap, num_envs=E, num_agents=N, seed=3, view_len=view_len)
    ora = pyoracle.Oracle(K.GAME_CLEANUP, amap, E, N, G.default_lut(), view_len=view_len, seed=3)
    fa = a.alloc_outputs(float32=True)
    a.reset(obs=fa[0])
    assert np.array_equal(fa[0].cpu().numpy(), _f32_of(ora.reset()))
    for _ in range(8):
        a.step_random(out=fa)
        _, o_obs, _, _ = ora.step_random()
        assert np.array_equal(fa[0].cpu().numpy(), _f32_of(o_obs))
    assert a.status() == 0


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("game", [K.GAME_HARVEST, K.GAME_CLEANUP])
def test_rollout_random_is_the_same_launches_as_step_by_step(game, fused):
    """ssd_rollout_random (one library call for a whole random-action rollout, rollout.py:58-70) against the oracle
    stepped one call at a time (fused: the whole call is ONE kernel launch, envs resident in LDS): every ring slot holds the observations / rewards of its step, a reset happens every
    `reset_every` steps, and a second call continues where the first stopped (step0)."""
    import torch
    E, N, ring, every = 96, 5, 4, 7
    eng = VecEngine(game, None, num_envs=E, num_agents=N, seed=11)
    ora = pyoracle.Oracle(game, K.HARVEST_MAP if game == K.GAME_HARVEST else K.CLEANUP_MAP, E, N, G.default_lut(), seed=11)
    obs = torch.zeros((ring, E, N, 15, 15, 3), dtype=torch.uint8, device="cuda")
    rew = torch.zeros((ring, E, N), dtype=torch.int32, device="cuda")
    done = torch.zeros((ring, E, N), dtype=torch.uint8, device="cuda")
    want = {}
    for k in range(23):
        if k % every == 0:
            ora.reset()
        _, o_obs, o_rew, _ = ora.step_random()
        want[k] = (o_obs, o_rew)
    eng.rollout_random(10, obs, rew, done, reset_every=every, step0=0, fused=fused)
    eng.set_rollout_chains(3)                                   # three env ranges on streams of their own: same results
    eng.rollout_random(13, obs, rew, done, reset_every=every, step0=10, fused=fused)
    got_obs, got_rew = obs.cpu().numpy(), rew.cpu().numpy()
    for k in range(23 - ring, 23):                              # the last `ring` steps are still in the ring
        np.testing.assert_array_equal(got_obs[k % ring], want[k][0], err_msg="obs of step %d" % k)
        np.testing.assert_array_equal(got_rew[k % ring], want[k][1], err_msg="rew of step %d" % k)
    a, b = eng.get_state(), ora.get_state()
    for key in ("world", "pos", "orient", "episode", "t"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert not done.any().item() and eng.status() == 0
    with pytest.raises(ValueError):
        eng.rollout_random(1, obs[:, :1], rew, done)


def _fused_vs_oracle(eng, ora, E, N, V, steps, every, ring):
    import torch
    obs = torch.zeros((ring, E, N, V, V, 3), dtype=torch.uint8, device="cuda")
    rew = torch.zeros((ring, E, N), dtype=torch.int32, device="cuda")
    done = torch.ones((ring, E, N), dtype=torch.uint8, device="cuda")
    want = {}
    for k in range(steps):
        if k % every == 0:
            ora.reset()
        _, o_obs, o_rew, _ = ora.step_random()
        want[k] = (o_obs, o_rew)
    first = steps // 3
    eng.rollout_random(first, obs, rew, done, reset_every=every, step0=0, fused=True)
    eng.rollout_random(steps - first, obs, rew, done, reset_every=every, step0=first, fused=True)
    got_obs, got_rew = obs.cpu().numpy(), rew.cpu().numpy()
    for k in range(max(steps - ring, 0), steps):
        np.testing.assert_array_equal(got_rew[k % ring], want[k][1], err_msg="rew of step %d" % k)
        np.testing.assert_array_equal(got_obs[k % ring], want[k][0], err_msg="obs of step %d" % k)
    a, b = eng.get_state(), ora.get_state()
    for key in ("world", "pos", "orient", "episode", "t"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert not done.any().item() and eng.status() == 0


@pytest.mark.parametrize("case", range(len(UNUSUAL)))
def test_fused_rollout_on_unusual_configurations(case):
    """The rollout kernel's general instantiations (any map, view, beam length, agent count; maps above 1024 cells)."""
    game, H, W, E, N, v, L, steps = UNUSUAL[case]
    rng = np.random.RandomState(100 + case)
    amap = _random_map(rng, H, W, game, n_spawn=N + 3)
    eng = VecEngine(game, amap, num_envs=E, num_agents=N, view_len=v, beam_len=L, seed=case, keep_beams=bool(case % 2))
    ora = pyoracle.Oracle(game, amap, E, N, G.default_lut(), view_len=v, beam_len=L, seed=case)
    _fused_vs_oracle(eng, ora, E, N, 2 * v + 1, steps, every=9, ring=2)


@pytest.mark.parametrize("cfg", [(K.GAME_HARVEST, "default", 10, 37), (K.GAME_CLEANUP, "default", 10, 64), (K.GAME_HARVEST, "default", 7, 50),
                                 (K.GAME_HARVEST, "25x38", 5, 33), (K.GAME_CLEANUP, "48x36", 10, 21), (K.GAME_CLEANUP, "default", 1, 40)])
def test_fused_rollout_specialisations(cfg):
    """Every specialisation of the rollout kernel: N = 5 / 10 / other, shipped and other maps, ragged env counts; a reset
    falls on the first step, in the middle and on the last step of a call."""
    game, which, N, E = cfg
    amap = {"default": K.HARVEST_MAP if game == K.GAME_HARVEST else K.CLEANUP_MAP, "25x38": K.harvest_map_25x38(),
            "48x36": K.cleanup_map_48x36()}[which]
    eng = VecEngine(game, amap, num_envs=E, num_agents=N, seed=5)
    ora = pyoracle.Oracle(game, amap, E, N, G.default_lut(), seed=5)
    _fused_vs_oracle(eng, ora, E, N, 15, steps=31, every=10, ring=3)


@pytest.mark.parametrize("game", [K.GAME_HARVEST, K.GAME_CLEANUP])
@pytest.mark.parametrize("mode", ["chain1", "chain2", "fused"])
def test_rollout_actions_matches_the_oracle(game, mode):
    """ssd_rollout_actions: the rollout call with CALLER-SUPPLIED actions (what the reference's callers do per step,
    visuallizer_rllib.py:121-153 -> map_env.py:152-212), through every dispatch form -- the library's own queues with one and two
    chains (split rendering from 4 steps on), the fused kernel.  Action ring and output ring of different lengths (argument blocks
    per residue of lcm(3, 4) = 12), absent agents (-1), resets in the middle of a call, calls of 1 / 2 / many steps; the same
    buffers again (cached argument set) and other buffers (a new set).  Oracle stepped call by call with the same actions."""
    import torch
    E, N, ring, aring, every = 300, 5, 3, 4, 11
    na = 8 if game == K.GAME_HARVEST else 9
    eng = VecEngine(game, None, num_envs=E, num_agents=N, seed=5)
    ora = pyoracle.Oracle(game, K.HARVEST_MAP if game == K.GAME_HARVEST else K.CLEANUP_MAP, E, N, G.default_lut(), seed=5)
    obs = torch.zeros((ring, E, N, 15, 15, 3), dtype=torch.uint8, device="cuda")
    rew = torch.zeros((ring, E, N), dtype=torch.int32, device="cuda")
    done = torch.zeros((ring, E, N), dtype=torch.uint8, device="cuda")
    acts = [torch.zeros((aring, E, N), dtype=torch.int32, device="cuda") for _ in range(2)]
    eng.set_rollout_chains(2 if mode == "chain2" else 1)
    rng = np.random.RandomState(17 + game)
    total = 0
    for call, n in enumerate((4, 1, 2, 4, 3, 4)):               # (at most `aring` steps per call: a slot is read once per call)
        a_host = rng.randint(-1, na, size=(aring, E, N)).astype(np.int32)
        buf = acts[call % 2] if call >= 3 else acts[0]
        buf.copy_(torch.from_numpy(a_host))
        eng.rollout_actions(buf, n, obs, rew, done, reset_every=every, step0=total, fused=(mode == "fused"))
        want = {}
        for k in range(total, total + n):
            if k % every == 0:
                ora.reset()
            o_obs, o_rew, _ = ora.step(a_host[k % aring])
            want[k] = (o_obs, o_rew)
        total += n
        got_obs, got_rew = obs.cpu().numpy(), rew.cpu().numpy()
        for k in range(max(total - ring, total - n), total):
            np.testing.assert_array_equal(got_obs[k % ring], want[k][0], err_msg="obs of step %d" % k)
            np.testing.assert_array_equal(got_rew[k % ring], want[k][1], err_msg="rew of step %d" % k)
        a, b = eng.get_state(), ora.get_state()
        for key in ("world", "pos", "orient", "episode", "t"):
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        path = eng.rollout_path()
        assert path["fused"] == (mode == "fused") and path["chains"] == (2 if mode == "chain2" else 1), path
    assert eng.status() == 0
    # a bad action id is reported, not obeyed (KeyError in agent.action_map)
    acts[0].fill_(na)
    eng.rollout_actions(acts[0], 2, obs, rew, done, step0=total, fused=(mode == "fused"))
    from sequential_social_dilemma_games_amd import _capi
    assert eng.status() == _capi.SSD_ST_BAD_ACTION
    o_obs, o_rew, _ = ora.step(np.full((E, N), -1, np.int32))
    o_obs, o_rew, _ = ora.step(np.full((E, N), -1, np.int32))
    np.testing.assert_array_equal(obs[(total + 1) % ring].cpu().numpy(), o_obs)
    # afterwards the ordinary paths continue from the same state
    a1 = rng.randint(0, na, size=(E, N)).astype(np.int32)
    o2, r2, _ = eng.step(torch.from_numpy(a1).cuda())
    o_obs, o_rew, _ = ora.step(a1)
    np.testing.assert_array_equal(o2.cpu().numpy(), o_obs)
    np.testing.assert_array_equal(r2.cpu().numpy(), o_rew)
    o2, r2, _ = eng.step_random()
    _, o_obs, o_rew, _ = ora.step_random()
    np.testing.assert_array_equal(o2.cpu().numpy(), o_obs)
    np.testing.assert_array_equal(r2.cpu().numpy(), o_rew)


@pytest.mark.parametrize("mode", ["calls", "chains", "fused"])
@pytest.mark.parametrize("which", ["48x36", "25x18", "25x18_general"])
def test_cleanup_steps_with_many_shooters(which, mode):
    """Cleanup with 10 agents of which 4 ... 10 FIRE or CLEAN in the same step (cleanup.py:94-111 through map_env.py:545-649, in
    action order): more shooters than the 64 / 15 = 4 slots of one parallel beam pass.  Two passes keep the first pass's cells and
    marks in a second set of registers (overlay patch; in split rollouts a second beam list for the renderer workgroups); nine or
    ten shooters take three passes and the merged overlay.  Crowded starts (in two thirds of the envs the agents are moved onto
    ten neighbouring cells, so that beams overlap, hit agents and share waste cells), 40 steps, every step's observations, rewards and state
    against the oracle -- per-call stepping (plain kernels: the overlay patch), rollout chains (coherent + split kernels: both
    lists) and the fused kernel; the enlarged map's own kernel, the shipped map's 10-agent kernel, and the general kernel
    (view_len 6: no map-specific variant)."""
    import torch
    amap = K.cleanup_map_48x36() if which == "48x36" else K.CLEANUP_MAP
    E, N, steps = 192, 10, 40
    kw = dict(view_len=6) if which == "25x18_general" else {}
    V = 13 if which == "25x18_general" else 15
    eng = VecEngine(K.GAME_CLEANUP, amap, num_envs=E, num_agents=N, seed=77, **kw)
    ora = pyoracle.Oracle(K.GAME_CLEANUP, amap, E, N, G.default_lut(), seed=77, **kw)
    eng.reset()
    ora.reset()
    rng = np.random.RandomState(4242)
    # crowd the agents: in every env the ten cells nearest to a random cell that are neither wall nor river-side void, in random
    # order, facing anywhere (two thirds of the envs; the rest keep their spawn points)
    st = ora.get_state()
    free = [(r, c) for r in range(len(amap)) for c in range(len(amap[0])) if amap[r][c] != "@"]
    fr = np.array(free)
    pos, orient = st["pos"].copy(), st["orient"].copy()
    for e in range(E):
        if e % 3 == 2:
            continue
        anchor = fr[rng.randint(len(fr))]
        near = np.argsort(np.abs(fr - anchor).sum(1) + 0.01 * rng.rand(len(fr)))[:N]
        pos[e] = fr[near[rng.permutation(N)]]
        orient[e] = rng.randint(0, 4, size=N)
    eng.set_state(pos=pos, orient=orient)
    ora.set_state(pos=pos, orient=orient)
    a_host = np.zeros((steps, E, N), dtype=np.int32)
    for k in range(steps):
        for e in range(E):
            n_sh = 4 + (e + k) % 7                                  # 4 .. 10 shooters
            a = rng.randint(0, 7, size=N)                           # movers / turners
            sh = rng.permutation(N)[:n_sh]
            a[sh] = rng.randint(7, 9, size=n_sh)                    # FIRE or CLEAN
            a_host[k, e] = a
    a_dev = torch.from_numpy(a_host).cuda()
    if mode == "calls":
        for k in range(steps):
            o, r, _ = eng.step(a_dev[k])
            o_obs, o_rew, _ = ora.step(a_host[k])
            np.testing.assert_array_equal(r.cpu().numpy(), o_rew, err_msg="rewards of step %d" % k)
            assert np.array_equal(o.cpu().numpy(), o_obs), "observations of step %d differ" % k
    else:
        obs = torch.zeros((steps, E, N, V, V, 3), dtype=torch.uint8, device="cuda")
        rew = torch.zeros((steps, E, N), dtype=torch.int32, device="cuda")
        done = torch.zeros((steps, E, N), dtype=torch.uint8, device="cuda")
        eng.set_rollout_chains(2 if mode == "chains" else 1)
        eng.rollout_actions(a_dev, steps, obs, rew, done, reset_every=0, step0=0, fused=(mode == "fused"))
        g_obs, g_rew = obs.cpu().numpy(), rew.cpu().numpy()
        for k in range(steps):
            o_obs, o_rew, _ = ora.step(a_host[k])
            np.testing.assert_array_equal(g_rew[k], o_rew, err_msg="rewards of step %d" % k)
            assert np.array_equal(g_obs[k], o_obs), "observations of step %d differ" % k
        if which != "25x18_general":
            path = eng.rollout_path()
            assert path["fused"] == (mode == "fused"), path
            assert mode == "fused" or (path["aql"] and path["split"]) or not path["aql"], path
    a, b = eng.get_state(), ora.get_state()
    for key in ("world", "pos", "orient", "episode", "t"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert eng.status() == 0
    eng.close()


@pytest.mark.parametrize("mode", ["calls", "chains", "fused"])
@pytest.mark.parametrize("which", ["cleanup48x36", "cleanup25x18", "harvest"])
@pytest.mark.parametrize("N", [10, 5])
def test_crowded_moves(N, which, mode):
    """Ten / five agents that mostly MOVE, from crowded starts: targets that are taken, chains of agents following each other, swaps,
    cycles, cells wanted by several movers (the shuffle decides) and -- in every fourth env -- two agents STARTING on one cell
    (map_env.py:357-543 in full).  The five- and ten-agent per-step kernels keep the pairwise loop's masks and "who stands on my target"
    for the contested path and know from a bit in the env's header whether two agents may share a cell (set here by
    ssd_set_state, afterwards by every step's consume phase); 60 steps, every step's observations and rewards and the final state
    against the oracle, through per-call stepping, the rollout chains and the fused kernel."""
    import torch
    game = K.GAME_HARVEST if which == "harvest" else K.GAME_CLEANUP
    amap = {"cleanup48x36": K.cleanup_map_48x36(), "cleanup25x18": K.CLEANUP_MAP, "harvest": K.HARVEST_MAP}[which]
    E, steps = 160, 60
    eng = VecEngine(game, amap, num_envs=E, num_agents=N, seed=91)
    ora = pyoracle.Oracle(game, amap, E, N, G.default_lut(), seed=91)
    eng.reset()
    ora.reset()
    rng = np.random.RandomState(777)
    st = ora.get_state()
    fr = np.array([(r, c) for r in range(len(amap)) for c in range(len(amap[0])) if amap[r][c] != "@"])
    pos, orient = st["pos"].copy(), st["orient"].copy()
    for e in range(E):
        if e % 5 == 4:
            continue                                               # (these keep their spawn points)
        anchor = fr[rng.randint(len(fr))]
        near = np.argsort(np.abs(fr - anchor).sum(1) + 0.01 * rng.rand(len(fr)))[:N]
        pos[e] = fr[near[rng.permutation(N)]]
        if e % 4 == 1:
            pos[e, rng.randint(1, N)] = pos[e, 0]                   # two agents on one cell
        orient[e] = rng.randint(0, 4, size=N)
    eng.set_state(pos=pos, orient=orient)
    ora.set_state(pos=pos, orient=orient)
    a_host = rng.randint(0, 5, size=(steps, E, N)).astype(np.int32)    # the four moves and STAY ...
    other = rng.rand(steps, E, N) < 0.15
    a_host[other] = rng.randint(5, 9 if game == K.GAME_CLEANUP else 8, size=int(other.sum()))   # ... and now and then a turn or a beam
    a_dev = torch.from_numpy(a_host).cuda()
    if mode == "calls":
        for k in range(steps):
            o, r, _ = eng.step(a_dev[k])
            o_obs, o_rew, _ = ora.step(a_host[k])
            np.testing.assert_array_equal(r.cpu().numpy(), o_rew, err_msg="rewards of step %d" % k)
            assert np.array_equal(o.cpu().numpy(), o_obs), "observations of step %d differ" % k
    else:
        obs = torch.zeros((steps, E, N, 15, 15, 3), dtype=torch.uint8, device="cuda")
        rew = torch.zeros((steps, E, N), dtype=torch.int32, device="cuda")
        done = torch.zeros((steps, E, N), dtype=torch.uint8, device="cuda")
        eng.set_rollout_chains(2 if mode == "chains" else 1)
        eng.rollout_actions(a_dev, steps, obs, rew, done, reset_every=0, step0=0, fused=(mode == "fused"))
        g_obs, g_rew = obs.cpu().numpy(), rew.cpu().numpy()
        for k in range(steps):
            o_obs, o_rew, _ = ora.step(a_host[k])
            np.testing.assert_array_equal(g_rew[k], o_rew, err_msg="rewards of step %d" % k)
            assert np.array_equal(g_obs[k], o_obs), "observations of step %d differ" % k
    a, b = eng.get_state(), ora.get_state()
    for key in ("world", "pos", "orient", "episode", "t"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert eng.status() == 0
    eng.close()


def test_agents_on_one_cell_survive_a_later_world_update():
    """ssd_set_state(pos) tells the kernels that agents share a cell (a bit beside the header's waste counts); a later
    ssd_set_state(world) -- which rewrites those counts for Cleanup -- must keep it: the steps that follow resolve the moves of the
    overlapping agents as map_env.py:494-543 does, not as agents that stand apart."""
    import torch
    E, N, steps = 96, 5, 40
    eng = VecEngine(K.GAME_CLEANUP, K.CLEANUP_MAP, num_envs=E, num_agents=N, seed=5)
    ora = pyoracle.Oracle(K.GAME_CLEANUP, K.CLEANUP_MAP, E, N, G.default_lut(), seed=5)
    eng.reset(); ora.reset()
    st = ora.get_state()
    pos = st["pos"].copy()
    pos[:, 1] = pos[:, 0]                                           # agents 0 and 1 on one cell, everywhere
    pos[::2, 3] = pos[::2, 2]                                       # ... and 2 and 3 in every other env
    eng.set_state(pos=pos); ora.set_state(pos=pos)
    world = ora.get_state()["world"].copy()
    world[:, 2, 2] = np.where(world[:, 2, 2] == ord("H"), ord("R"), ord("H"))   # (a waste cell toggled: the call recounts the waste)
    eng.set_state(world=world); ora.set_state(world=world)
    rng = np.random.RandomState(11)
    for k in range(steps):
        a = rng.randint(0, 5, size=(E, N)).astype(np.int32)
        o, r, _ = eng.step(torch.from_numpy(a).cuda())
        o_obs, o_rew, _ = ora.step(a)
        np.testing.assert_array_equal(r.cpu().numpy(), o_rew, err_msg="rewards of step %d" % k)
        assert np.array_equal(o.cpu().numpy(), o_obs), "observations of step %d differ" % k
    a, b = eng.get_state(), ora.get_state()
    for key in ("world", "pos", "orient"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    eng.close()


def test_a_masked_reset_leaves_the_other_envs_shared_cells_alone():
    """Agents that share a cell in EVERY env, then a reset of every other env (ssd_reset with a mask): the reset envs start from spawn
    points of their own (their header says "apart" again), the others still hold their overlapping agents and keep resolving
    their moves as map_env.py:494-543 does -- the bit a step's move phase trusts is per env."""
    import torch
    E, N, steps = 64, 5, 30
    eng = VecEngine(K.GAME_HARVEST, K.HARVEST_MAP, num_envs=E, num_agents=N, seed=21)
    ora = pyoracle.Oracle(K.GAME_HARVEST, K.HARVEST_MAP, E, N, G.default_lut(), seed=21)
    eng.reset(); ora.reset()
    pos = ora.get_state()["pos"].copy()
    pos[:, 4] = pos[:, 3]
    pos[:, 1] = pos[:, 0]
    eng.set_state(pos=pos); ora.set_state(pos=pos)
    mask = (np.arange(E) % 2).astype(np.uint8)
    o = eng.reset(mask=torch.from_numpy(mask).cuda())
    o_obs = ora.reset(mask=mask)
    assert np.array_equal(o.cpu().numpy()[mask == 1], o_obs[mask == 1]), "observations of the reset envs differ"
    rng = np.random.RandomState(3)
    for k in range(steps):
        a = rng.randint(0, 5, size=(E, N)).astype(np.int32)
        o, r, _ = eng.step(torch.from_numpy(a).cuda())
        o_obs, o_rew, _ = ora.step(a)
        np.testing.assert_array_equal(r.cpu().numpy(), o_rew, err_msg="rewards of step %d" % k)
        assert np.array_equal(o.cpu().numpy(), o_obs), "observations of step %d differ" % k
    a, b = eng.get_state(), ora.get_state()
    for key in ("world", "pos", "orient", "episode", "t"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    eng.close()


def test_per_call_steps_can_be_captured_into_a_hip_graph():
    """ssd_step with device pointers is ONE kernel launch on the caller's stream and nothing else -- no synchronisation, no
    allocation, no other stream -- so a training loop may capture it (with its policy) into a HIP graph: torch.cuda.CUDAGraph
    over 6 steps whose action tensors are rewritten between replays; every replayed step against the oracle.  (The multi-step
    rollout calls are not capturable: they dispatch through queues of the library's own.)"""
    import torch
    E, N, KS = 96, 5, 6
    eng = VecEngine(K.GAME_CLEANUP, None, num_envs=E, num_agents=N, seed=11)
    ora = pyoracle.Oracle(K.GAME_CLEANUP, K.CLEANUP_MAP, E, N, G.default_lut(), seed=11)
    eng.reset()
    ora.reset()
    acts = torch.zeros((KS, E, N), dtype=torch.int32, device="cuda")
    views = [acts[k] for k in range(KS)]
    outs = [eng.alloc_outputs() for _ in range(KS)]
    rng = np.random.RandomState(5)
    side = torch.cuda.Stream()                                          # (torch's capture recipe: warm up on a side stream)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = rng.randint(-1, 9, size=(KS, E, N)).astype(np.int32)
        acts.copy_(torch.from_numpy(a))
        for k in range(KS):
            eng.step(views[k], out=outs[k])
            ora.step(a[k])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(KS):
            eng.step(views[k], out=outs[k])
    torch.cuda.synchronize()                                            # (capturing executes nothing: the state is the warm-up's)
    for rep in range(3):
        a = rng.randint(-1, 9, size=(KS, E, N)).astype(np.int32)
        acts.copy_(torch.from_numpy(a))
        g.replay()
        torch.cuda.synchronize()
        for k in range(KS):
            o_obs, o_rew, _ = ora.step(a[k])
            np.testing.assert_array_equal(outs[k][1].cpu().numpy(), o_rew, err_msg="replay %d, rewards of step %d" % (rep, k))
            assert np.array_equal(outs[k][0].cpu().numpy(), o_obs), "replay %d, observations of step %d differ" % (rep, k)
    st_a, st_b = eng.get_state(), ora.get_state()
    for key in ("world", "pos", "orient", "t"):
        np.testing.assert_array_equal(st_a[key], st_b[key], err_msg=key)
    assert eng.status() == 0
    del g
    eng.close()


def test_two_handles_share_the_dispatch_queues():
    """The library's dispatch queues belong to the device, not to a handle: two handles whose rollout calls are enqueued back
    to back follow each other in them.  Both bit-exact."""
    import torch
    E, N, ring, steps = 1024, 5, 2, 60
    engs = [VecEngine(g, None, num_envs=E, num_agents=N, seed=31 + g) for g in (K.GAME_HARVEST, K.GAME_CLEANUP)]
    oras = [pyoracle.Oracle(g, K.HARVEST_MAP if g == K.GAME_HARVEST else K.CLEANUP_MAP, E, N, G.default_lut(), seed=31 + g)
            for g in (K.GAME_HARVEST, K.GAME_CLEANUP)]
    bufs = [(torch.zeros((ring, E, N, 15, 15, 3), dtype=torch.uint8, device="cuda"),
             torch.zeros((ring, E, N), dtype=torch.int32, device="cuda")) for _ in engs]
    for eng in engs:
        eng.set_rollout_chains(2)
    for rep in range(2):
        for eng, (obs, rew) in zip(engs, bufs):                  # enqueued back to back: the second call finds the first in flight
            eng.rollout_random(steps, obs, rew, None, reset_every=25, step0=rep * steps)
        for eng, ora, (obs, rew) in zip(engs, oras, bufs):
            for k in range(rep * steps, (rep + 1) * steps):
                if k % 25 == 0:
                    ora.reset()
                _, o_obs, o_rew, _ = ora.step_random(want_obs=(k == (rep + 1) * steps - 1))
            last = ((rep + 1) * steps - 1) % ring
            np.testing.assert_array_equal(rew[last].cpu().numpy(), o_rew)
            assert np.array_equal(obs[last].cpu().numpy(), o_obs)
            a, b = eng.get_state(), ora.get_state()
            for key in ("world", "pos", "orient", "episode", "t"):
                np.testing.assert_array_equal(a[key], b[key], err_msg=key)
            assert eng.status() == 0


@pytest.mark.parametrize("fused", [False, True])
def test_rollout_random_edge_cases(fused):
    """n_steps = 0 is a no-op; reset_every = 1 resets before every step; more chains than envs; a ring longer than the
    rollout; and bad arguments are rejected."""
    import torch
    from sequential_social_dilemma_games_amd import _capi
    E, N = 5, 3
    eng = VecEngine(K.GAME_CLEANUP, None, num_envs=E, num_agents=N, seed=21)
    ora = pyoracle.Oracle(K.GAME_CLEANUP, K.CLEANUP_MAP, E, N, G.default_lut(), seed=21)
    obs = torch.zeros((6, E, N, 15, 15, 3), dtype=torch.uint8, device="cuda")
    rew = torch.zeros((6, E, N), dtype=torch.int32, device="cuda")
    eng.set_rollout_chains(8)                                   # clipped to the 5 envs
    eng.rollout_random(0, obs, rew, None, reset_every=1, fused=fused)
    assert (eng.get_state()["episode"] == 0xFFFFFFFF).all()     # nothing happened: never reset
    eng.rollout_random(4, obs, rew, None, reset_every=1, step0=3, fused=fused)
    for k in range(3, 7):
        ora.reset()
        _, o_obs, o_rew, _ = ora.step_random()
        np.testing.assert_array_equal(obs[k % 6].cpu().numpy(), o_obs, err_msg="obs of step %d" % k)
        np.testing.assert_array_equal(rew[k % 6].cpu().numpy(), o_rew, err_msg="rew of step %d" % k)
    a, b = eng.get_state(), ora.get_state()
    for key in ("world", "pos", "orient", "episode", "t"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    with pytest.raises(_capi.SsdError):
        eng.rollout_random(-1, obs, rew, None, fused=fused)
    with pytest.raises(_capi.SsdError):
        eng.set_rollout_chains(9)
    assert eng.status() == 0


def test_vector_env_in_sync_resets_only_on_the_horizon_step():
    """While all envs were reset together the adapter knows on which step they finish: no reset launch until then, a full
    reset exactly then; results as with a masked reset after every step.  A rollout call keeps the count."""
    import torch
    from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv
    E, N, Hz = 33, 5, 5
    venv = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=Hz, seed=8)
    ora = pyoracle.Oracle(K.GAME_HARVEST, K.HARVEST_MAP, E, N, G.default_lut(), seed=8)
    np.testing.assert_array_equal(venv.reset().cpu().numpy(), ora.reset())
    calls = []
    real_reset = venv.engine.reset
    venv.engine.reset = lambda *a, **kw: (calls.append(kw.get("mask") is not None), real_reset(*a, **kw))[1]
    rng = np.random.RandomState(5)
    for s in range(13):
        act = rng.randint(0, 8, size=(E, N)).astype(np.int32)
        obs, rew, done = venv.step(torch.from_numpy(act).cuda())
        o_obs, o_rew, _ = ora.step(act)
        finished = (s + 1) % Hz == 0
        if finished:
            o_obs = ora.reset()
        assert bool(done.all().item()) == finished and bool(done.any().item()) == finished
        np.testing.assert_array_equal(rew.cpu().numpy(), o_rew)
        np.testing.assert_array_equal(obs.cpu().numpy(), o_obs, err_msg="step %d" % s)
    assert calls == [False, False]                             # two full resets (steps 5 and 10), never a masked one
    assert venv.engine.steps_since_full_reset == 3
    ring = tuple(t.unsqueeze(0) for t in venv._out)
    venv.engine.rollout_random(4, *ring, reset_every=3, step0=1)     # resets before its steps 2 (and no other): 2 steps since
    assert venv.engine.steps_since_full_reset == 2
    venv.engine.reset = real_reset
    venv.try_reset(0)
    assert venv.engine.steps_since_full_reset is None


@pytest.mark.parametrize("cfg", [(K.GAME_HARVEST, 5, 41), (K.GAME_CLEANUP, 10, 24), (K.GAME_HARVEST, 7, 19),
                                 (K.GAME_HARVEST, 5, 23, "25x38"), (K.GAME_CLEANUP, 10, 17, "48x36")])
def test_auto_reset_in_the_step_launch(cfg):
    """SSD_AUTO_RESET: the step launch resets the envs that reach the horizon; same rewards / dones as a plain step, the
    observation rows of finished envs are the reset's, the state afterwards is the reset state (oracle: step, then reset
    with the done flags as the mask).  Envs are put out of phase first; random and explicit actions."""
    import torch
    game, N, E = cfg[:3]
    Hz = 6
    amap = K.HARVEST_MAP if game == K.GAME_HARVEST else K.CLEANUP_MAP
    if len(cfg) > 3:                                            # the enlarged maps have kernels of their own (FAST = 2)
        amap = K.harvest_map_25x38() if cfg[3] == "25x38" else K.cleanup_map_48x36()
    eng = VecEngine(game, amap, num_envs=E, num_agents=N, seed=31)
    ora = pyoracle.Oracle(game, amap, E, N, G.default_lut(), seed=31)
    eng.set_horizon(Hz)
    out = eng.alloc_outputs()
    eng.reset(obs=out[0]); ora.reset()
    rng = np.random.RandomState(1)
    for _ in range(2):
        eng.step_random(out=out); ora.step_random()
    third = (np.arange(E) % 3 == 0).astype(np.uint8)
    eng.reset(mask=torch.from_numpy(third).cuda(), obs=out[0]); ora.reset(third)
    na = 8 if game == K.GAME_HARVEST else 9
    for s in range(17):
        if s % 2:
            act = rng.randint(0, na, size=(E, N)).astype(np.int32)
            obs, rew, done = eng.step(torch.from_numpy(act).cuda(), out=out, auto_reset=True)
            o_obs, o_rew, _ = ora.step(act)
        else:
            obs, rew, done = eng.step_random(out=out, auto_reset=True)
            _, o_obs, o_rew, _ = ora.step_random()
        o_done = ora.get_state()["t"] >= Hz
        if o_done.any():
            r_obs = ora.reset(o_done.astype(np.uint8))
            o_obs[o_done] = r_obs[o_done]
        np.testing.assert_array_equal(done.cpu().numpy(), np.repeat(o_done[:, None], N, 1).astype(np.uint8), err_msg="step %d" % s)
        np.testing.assert_array_equal(rew.cpu().numpy(), o_rew, err_msg="step %d" % s)
        np.testing.assert_array_equal(obs.cpu().numpy(), o_obs, err_msg="step %d" % s)
    a, b = eng.get_state(), ora.get_state()
    for k in ("world", "pos", "orient", "episode", "t"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert eng.status() == 0


def test_handles_on_one_device_share_the_dispatch_queues():
    """The library's dispatch queues belong to the device, not to a handle (a process gets slow with more than a few queues):
    three live engines -- different games, sizes and chain counts -- take turns with rollout calls and per-step calls on the same
    stream; each stays bit-exact against its oracle, and destroying one in the middle does not disturb the others."""
    import torch
    specs = [(K.GAME_HARVEST, K.HARVEST_MAP, 300, 5, 2), (K.GAME_CLEANUP, K.CLEANUP_MAP, 2100, 5, 3), (K.GAME_HARVEST, K.HARVEST_MAP, 64, 5, 1)]
    engs, oras, bufs = [], [], []
    for i, (game, amap, E, N, chains) in enumerate(specs):
        eng = VecEngine(game, amap, num_envs=E, num_agents=N, seed=40 + i)
        eng.set_rollout_chains(chains)
        engs.append(eng)
        oras.append(pyoracle.Oracle(game, amap, E, N, G.default_lut(), seed=40 + i))
        bufs.append((torch.zeros((2, E, N, 15, 15, 3), dtype=torch.uint8, device="cuda"), torch.zeros((2, E, N), dtype=torch.int32, device="cuda")))
    step0 = [0, 0, 0]
    for rnd in range(4):
        for i, eng in enumerate(engs):
            if eng is None:
                continue
            n = 3 + 2 * rnd + i
            eng.rollout_random(n, bufs[i][0], bufs[i][1], None, reset_every=7, step0=step0[i])
            for k in range(step0[i], step0[i] + n):
                if k % 7 == 0:
                    oras[i].reset()
                _, o_obs, o_rew, _ = oras[i].step_random()
            step0[i] += n
            last = (step0[i] - 1) % 2
            np.testing.assert_array_equal(bufs[i][1][last].cpu().numpy(), o_rew, err_msg="engine %d round %d" % (i, rnd))
            assert np.array_equal(bufs[i][0][last].cpu().numpy(), o_obs), "engine %d round %d: observations" % (i, rnd)
        if rnd == 1:
            engs[0].close()
            engs[0] = None
    for i, eng in enumerate(engs):
        if eng is not None:
            a, b = eng.get_state(), oras[i].get_state()
            for key in ("world", "pos", "orient", "episode", "t"):
                np.testing.assert_array_equal(a[key], b[key], err_msg="engine %d %s" % (i, key))
            assert eng.status() == 0
