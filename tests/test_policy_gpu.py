"""Policy rollouts on the MI355X (csrc/ssd_policy.hip, ssd_rollout_policy): the forward kernel against the float64 restatement
of models/conv_to_fc_net.py (policy_ref.py), the action selection against its host mirror, the rollout against a replay through
VecEngine.step, call splitting and ring lengths, weight sets, episodes, argument checks and the adapter."""
import ctypes as C

import numpy as np
import pytest
import torch

from episode_stats_ref import same
from policy_ref import forward as ref_forward, random_weights
from sequential_social_dilemma_games_amd import _capi, prng
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd.engine import VecEngine
from sequential_social_dilemma_games_amd.episode_stats import EpisodeStats
from sequential_social_dilemma_games_amd.policy import ConvFCPolicy, cdf_margin, sample_host
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
KEYS = ("obs", "actions", "logp", "value", "logits", "rew", "done")


def _engine(game, E, N, seed=3, horizon=0, amap=None):
    eng = VecEngine(game, amap, num_envs=E, num_agents=N, seed=seed)
    if horizon:
        eng.set_horizon(horizon)
    return eng, eng.reset()


def _policy(A, P, pseed=0, scale=1.0):
    w = random_weights(np.random.default_rng(pseed), P, A, scale)
    return ConvFCPolicy(A, P).load_arrays(w).to(DEV), w


def _rings(eng, R):
    E, N, A = eng.E, eng.N, eng.num_actions
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)   # noqa: E731
    return {"obs": z((R, E, N, 15, 15, 3), torch.uint8), "actions": z((R, E, N), torch.int32), "logp": z((R, E, N), torch.float32),
            "value": z((R, E, N), torch.float32), "logits": z((R, E, N, A), torch.float32), "rew": z((R, E, N), torch.int32),
            "done": z((R, E, N), torch.uint8), "last_value": z((E, N), torch.float32)}


def _roll(eng, pol, obs_in, n, r, step0=0, greedy=False, stats=None):
    eng.rollout_policy(pol, obs_in, n, r["obs"], actions=r["actions"], logp=r["logp"], value=r["value"], logits=r["logits"],
                       rew=r["rew"], done=r["done"], last_value=r["last_value"], step0=step0, greedy=greedy, stats=stats)


def _host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _coords(st0, done):
    """(episode, t) of the state each step's action is taken in, from the start state and the done ring [K,E,N]."""
    ep, t = st0["episode"].astype(np.int64).copy(), st0["t"].astype(np.int64).copy()
    out = []
    for k in range(done.shape[0]):
        out.append((ep.copy(), t.copy()))
        d = done[k, :, 0] != 0
        t = np.where(d, 0, t + 1)
        ep = np.where(d, ep + 1, ep)
    return out


def _check_sampled(eng, st0, h, max_frac=1e-4):
    """Every recorded action against the host mirror of the S_POLICY draw; only actions whose u is within 1e-5 of a boundary of
    the cumulative softmax may differ (expf / logf against NumPy's).  Returns the number of such steps."""
    envs = eng.env_index_base + np.arange(eng.E)
    bad = 0
    for k, (ep, t) in enumerate(_coords(st0, h["done"])):
        u = prng.policy_uniforms(eng.seed, envs, ep, t, eng.N)
        act, logp = sample_host(h["logits"][k], u)
        diff = act != h["actions"][k]
        if diff.any():
            assert np.all(cdf_margin(h["logits"][k], u)[diff] < 1e-5), "an action differs away from a CDF boundary"
            bad += int(diff.sum())
        same_a = ~diff
        assert np.abs(logp[same_a] - h["logp"][k][same_a]).max() <= 1e-5
    assert bad <= max(2, max_frac * h["actions"].size), bad
    return bad


def _check_replay(game, E, N, seed, horizon, st0, h, amap=None):
    """Replay the recorded actions through VecEngine.step(auto_reset=True) from the start state: obs / rew / done bit for bit."""
    eng, _ = _engine(game, E, N, seed=seed, horizon=horizon, amap=amap)
    eng.set_state(world=st0["world"], pos=st0["pos"], orient=st0["orient"], episode=st0["episode"], t=st0["t"])
    for k in range(h["actions"].shape[0]):
        obs, rew, done = eng.step(torch.from_numpy(h["actions"][k]).to(DEV), auto_reset=True)
        torch.cuda.synchronize()
        assert np.array_equal(obs.cpu().numpy(), h["obs"][k]), "obs of step %d" % k
        assert np.array_equal(rew.cpu().numpy(), h["rew"][k]), "rew of step %d" % k
        assert np.array_equal(done.cpu().numpy(), h["done"][k]), "done of step %d" % k
    return eng


# ---------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("P", [1, 5])
def test_forward_against_restatement(P):
    eng, obs0 = _engine(K.GAME_HARVEST, 4096, 5)
    pol, w = _policy(8, P, pseed=10 + P)
    noise = torch.randint(0, 256, (64, 5, 15, 15, 3), dtype=torch.uint8, device=DEV)
    for obs in (obs0, noise):
        lg, v = eng.policy_forward(pol, obs)
        lg2, v2 = eng.policy_forward(pol, obs)
        with torch.no_grad():
            tl, tv = pol(obs)
        torch.cuda.synchronize()
        assert torch.equal(lg, lg2) and torch.equal(v, v2), "two calls on the same input differ"
        rl, rv = ref_forward(w, obs.cpu().numpy())
        for got, tor, ref in ((lg, tl, rl), (v, tv, rv)):
            ek = np.abs(got.cpu().numpy().astype(np.float64) - ref).max()
            et = np.abs(tor.cpu().numpy().astype(np.float64) - ref).max()
            assert ek <= 4 * et + 1e-6, (ek, et)
        assert np.ptp(rl) > 1e-2


# ---------------------------------------------------------------------------------------------------- 2-4, 8. configurations
CONFIGS = [(K.GAME_HARVEST, None, 4096, 5, 5), (K.GAME_CLEANUP, None, 512, 5, 1), (K.GAME_HARVEST, None, 256, 2, 2),
           (K.GAME_CLEANUP, "48x36", 8, 10, 10)]


@pytest.mark.parametrize("game,amap,E,N,P", CONFIGS)
def test_rollout_configurations(game, amap, E, N, P):
    amap = K.cleanup_map_48x36() if amap == "48x36" else None
    seed, horizon, n = 5, 6, 9
    A = 8 if game == K.GAME_HARVEST else 9
    pol, _ = _policy(A, P, pseed=E + N)
    for greedy in (True, False):
        eng, obs0 = _engine(game, E, N, seed=seed, horizon=horizon, amap=amap)
        # a few random steps first, so that the start state is not a fresh reset
        for _ in range(2):
            eng.step_random(auto_reset=True)
        obs_in = eng.observe()
        st0 = eng.get_state()
        r = _rings(eng, n)
        _roll(eng, pol, obs_in, n, r, greedy=greedy)
        h = _host(r)
        # logits recorded = policy_forward of the observation the step acted on, bit for bit; value likewise
        prev = torch.cat([obs_in[None], r["obs"][:-1]])
        lg, v = eng.policy_forward(pol, prev)
        lv = eng.policy_forward(pol, r["obs"][-1])[1]
        torch.cuda.synchronize()
        assert np.array_equal(lg.cpu().numpy(), h["logits"]) and np.array_equal(v.cpu().numpy(), h["value"])
        assert np.array_equal(lv.cpu().numpy(), h["last_value"])
        if greedy:
            assert np.array_equal(h["actions"], torch.from_numpy(h["logits"]).argmax(-1).numpy().astype(np.int32))
            lsm = torch.log_softmax(torch.from_numpy(h["logits"]).double(), -1).numpy()
            assert np.abs(np.take_along_axis(lsm, h["actions"][..., None].astype(np.int64), -1)[..., 0] - h["logp"]).max() <= 1e-5
        else:
            _check_sampled(eng, st0, h)
            assert len(np.unique(h["actions"])) > 1                # a real distribution, not a constant
        assert h["done"][horizon - 3].all() and not h["done"][: horizon - 3].any()     # (2 random steps before: t = 2)
        rep = _check_replay(game, E, N, seed, horizon, st0, h, amap=amap)
        a, b = eng.get_state(), rep.get_state()
        for key in ("world", "pos", "orient", "episode", "t"):
            assert np.array_equal(a[key], b[key]), key
        assert eng.status() == 0


# ---------------------------------------------------------------------------------------------------- 5. call splitting, ring
def test_call_splitting_and_ring_length():
    E, N, P = 256, 5, 5
    pol, _ = _policy(8, P, pseed=4)
    outs = []
    for mode in ("one", "split", "ring1"):
        eng, obs0 = _engine(K.GAME_HARVEST, E, N, seed=9, horizon=5)
        if mode == "one":
            r = _rings(eng, 16)
            _roll(eng, pol, obs0, 16, r)
        elif mode == "split":
            r = _rings(eng, 16)
            _roll(eng, pol, obs0, 8, r)
            _roll(eng, pol, r["obs"][7].clone(), 8, r, step0=8)
        else:
            r = _rings(eng, 1)
            _roll(eng, pol, obs0, 16, r)
        outs.append(_host(r))
        assert eng.steps_since_full_reset == 16 % 5
    one, split, ring1 = outs
    for k in KEYS:
        assert np.array_equal(one[k], split[k]), k
        assert np.array_equal(one[k][15], ring1[k][0]), k
    assert np.array_equal(one["last_value"], ring1["last_value"])


# ---------------------------------------------------------------------------------------------------- 6. weight sets
@pytest.mark.parametrize("greedy", [True, False])
def test_weight_sets(greedy):
    E, N, A = 128, 5, 9
    for P in (N, 1):
        eng, obs0 = _engine(K.GAME_CLEANUP, E, N, seed=2)
        pol = ConvFCPolicy(A, P)
        with torch.no_grad():
            pol.logits_w.zero_()
            pol.logits_b.zero_()
            for p in range(P):
                pol.logits_b[p, p % A if P == N else 3] = 200.0
        pol = pol.to(DEV)
        r = _rings(eng, 4)
        _roll(eng, pol, obs0, 4, r, greedy=greedy)
        h = _host(r)
        want = np.array([i % A if P == N else 3 for i in range(N)], np.int32)
        assert np.array_equal(h["actions"], np.broadcast_to(want, h["actions"].shape))


# ---------------------------------------------------------------------------------------------------- 7. episodes
def test_episodes_and_stats():
    E, N, seed = 64, 5, 12
    pol, _ = _policy(8, 1, pseed=6)
    eng, obs0 = _engine(K.GAME_HARVEST, E, N, seed=seed, horizon=10)
    st0 = eng.get_state()
    stats = EpisodeStats(E, N)
    r = _rings(eng, 25)
    _roll(eng, pol, obs0, 25, r, stats=stats)
    h = _host(r)
    ended = [k for k in range(25) if h["done"][k].any()]
    assert ended == [9, 19] and h["done"][9].all() and h["done"][19].all()
    st = eng.get_state()
    assert np.all(st["episode"] == st0["episode"] + 2) and np.all(st["t"] == 5) and eng.steps_since_full_reset == 5
    # the obs rows after an episode ends are the reset's: the replay through step(auto_reset=True) gives the same rows
    _check_replay(K.GAME_HARVEST, E, N, seed, 10, st0, h)
    other = EpisodeStats(E, N)
    other.fold(r["rew"], r["done"], n_steps=25)
    a, b = stats.drain(), other.drain()
    assert same(a, b)
    assert int(a["counts"][:, 0].sum()) == 2 * E


def test_reset_rows_equal_a_fresh_reset():
    E, N, seed = 32, 5, 21
    pol, _ = _policy(8, 5, pseed=8)
    eng, obs0 = _engine(K.GAME_HARVEST, E, N, seed=seed, horizon=3)
    r = _rings(eng, 4)
    _roll(eng, pol, obs0, 4, r)
    h = _host(r)
    twin, _ = _engine(K.GAME_HARVEST, E, N, seed=seed)
    twin.set_state(episode=np.zeros(E, np.uint32))            # the next reset starts episode 1, as the auto reset at step 2 did
    o = twin.reset().cpu().numpy()
    assert np.array_equal(h["obs"][2], o)


# ---------------------------------------------------------------------------------------------------- 9. rejection
def test_rejection_leaves_state_alone():
    E, N = 8, 5
    eng, obs0 = _engine(K.GAME_HARVEST, E, N, horizon=4)
    pol, _ = _policy(8, 1)
    st0 = eng.get_state()
    r = _rings(eng, 3)
    good = dict(actions=r["actions"], logp=r["logp"], value=r["value"], logits=r["logits"], rew=r["rew"], done=r["done"],
                last_value=r["last_value"])

    def call(policy=pol, obs_in=obs0, n=3, obs=r["obs"], **kw):
        args = dict(good)
        args.update(kw)
        eng.rollout_policy(policy, obs_in, n, obs, **args)

    bad_calls = [
        lambda: call(policy=_policy(9, 1)[0]),                              # A != Discrete(8)
        lambda: call(policy=_policy(8, 3)[0]),                              # P not in {1, N}
        lambda: call(policy=ConvFCPolicy(8, 1)),                            # parameters on the CPU
        lambda: call(policy="not a policy"),
        lambda: call(n=0),
        lambda: call(step0=-1),
        lambda: call(obs=r["obs"].float()),
        lambda: call(obs=r["obs"].cpu()),
        lambda: call(obs=r["obs"][:, :4]),
        lambda: call(obs=torch.zeros((0, E, N, 15, 15, 3), dtype=torch.uint8, device=DEV)),
        lambda: call(obs=r["obs"].transpose(0, 1).contiguous().transpose(0, 1)),  # not contiguous
        lambda: call(obs_in=obs0[:4]),
        lambda: call(obs_in=obs0.float()),
        lambda: call(actions=r["actions"].long()),
        lambda: call(logp=r["logp"][:2]),
        lambda: call(value=r["value"].double()),
        lambda: call(logits=r["logits"][..., :7]),
        lambda: call(rew=r["rew"].to(torch.uint8)),
        lambda: call(done=r["done"].to(torch.int32)),
        lambda: call(last_value=r["last_value"][None]),
        lambda: call(stats=EpisodeStats(E, N), done=None),                  # stats need done
        lambda: call(n=4, stats=EpisodeStats(E, N)),                        # ring shorter than n_steps
        lambda: eng.policy_forward(pol, obs0.float()),
        lambda: eng.policy_forward(_policy(8, 2)[0], obs0),
    ]
    for k, f in enumerate(bad_calls):
        with pytest.raises(ValueError):
            f()
    # a multi-slot ring of misaligned slots, and a view the network does not take
    e3, o3 = _engine(K.GAME_HARVEST, 3, 5)
    with pytest.raises(ValueError):
        e3.rollout_policy(pol, o3, 2, torch.zeros((2, 3, 5, 15, 15, 3), dtype=torch.uint8, device=DEV))
    e5 = VecEngine(K.GAME_HARVEST, num_envs=4, num_agents=5, view_len=5)
    o5 = e5.reset()
    with pytest.raises(ValueError):
        e5.rollout_policy(pol, o5, 1, torch.zeros((1, 4, 5, 11, 11, 3), dtype=torch.uint8, device=DEV))
    # the C side rejects the same things before launching
    L, w = _capi.lib(), pol.packed()
    dp = lambda t: C.c_void_p(t.data_ptr())                                # noqa: E731
    assert L.ssd_rollout_policy(eng._h, dp(w), 3, dp(obs0), 3, 0, dp(r["obs"]), dp(r["actions"]), None, None, None, None, None, 3,
                                None, 0, None) == _capi.SSD_E_INVALID
    assert L.ssd_rollout_policy(eng._h, dp(w), 1, dp(obs0), 0, 0, dp(r["obs"]), dp(r["actions"]), None, None, None, None, None, 3,
                                None, 0, None) == _capi.SSD_E_INVALID
    assert L.ssd_rollout_policy(eng._h, dp(w), 1, dp(obs0), 3, 0, dp(r["obs"]), None, None, None, None, None, None, 3,
                                None, 0, None) == _capi.SSD_E_INVALID
    assert L.ssd_policy_forward(dp(w), 1, 16, dp(obs0), E, N, None, None, 0, 0, None) == _capi.SSD_E_INVALID
    torch.cuda.synchronize()
    st = eng.get_state()
    for key in ("world", "pos", "orient", "episode", "t"):
        assert np.array_equal(st0[key], st[key]), key
    assert eng.status() == 0


# ---------------------------------------------------------------------------------------------------- 10. adapter
def test_adapter_sample():
    E, N, seed, horizon = 64, 5, 17, 7
    pol, _ = _policy(8, 5, pseed=3)
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=horizon, seed=seed, track_episodes=True)
    env.reset()
    out = env.sample(pol, 10)
    h = {k: v.cpu().numpy() for k, v in out.items()}
    eng, obs0 = _engine(K.GAME_HARVEST, E, N, seed=seed, horizon=horizon)
    r = _rings(eng, 10)
    _roll(eng, pol, obs0, 10, r)
    ref = _host(r)
    for k in ("obs", "actions", "logp", "value", "rew", "done", "last_value"):
        assert np.array_equal(h[k], ref[k]), k
    # the adapter continues from there: the next steps equal the engine's
    rng = np.random.default_rng(0)
    for _ in range(5):
        a = torch.from_numpy(rng.integers(0, 8, (E, N), dtype=np.int32)).to(DEV)
        o1, r1, d1 = env.step(a)
        o2, r2, d2 = eng.step(a, auto_reset=True)
        torch.cuda.synchronize()
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    a, b = env.engine.get_state(), eng.get_state()
    for key in ("world", "pos", "orient", "episode", "t"):
        assert np.array_equal(a[key], b[key]), key
    assert env.summary()["episodes"] == E * (15 // horizon)
    for kw in ({"float32_obs": True}, {"return_agent_actions": True}):
        bad = SSDVectorEnv(K.GAME_HARVEST, 8, N, horizon=horizon, seed=seed, **kw)
        with pytest.raises(ValueError):
            bad.sample(pol, 2)
