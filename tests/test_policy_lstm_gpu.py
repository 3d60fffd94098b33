"""Recurrent policy rollouts on the MI355X (csrc/ssd_policy_lstm.hip, ssd_policy_lstm_forward, ssd_rollout_policy_lstm): the
forward against the float64 restatement (policy_lstm_ref.py), the start rule, the rollout step by step against the restatement
and a replay through VecEngine.step, determinism across call splits and ring lengths, the learner's BPTT path, argument checks
and the adapter."""
import ctypes as C

import numpy as np
import pytest
import torch

from policy_lstm_ref import forward as ref_forward, random_weights
from test_policy_gpu import _check_replay, _check_sampled
from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd.engine import VecEngine
from sequential_social_dilemma_games_amd.policy import ConvFCPolicy, ConvLSTMPolicy
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
KEYS = ("obs", "actions", "logp", "value", "logits", "rew", "done")


def _engine(game, E, N, seed=3, horizon=0):
    eng = VecEngine(game, None, num_envs=E, num_agents=N, seed=seed)
    if horizon:
        eng.set_horizon(horizon)
    return eng, eng.reset()


def _policy(A, P, Cs, pseed=0):
    w = random_weights(np.random.default_rng(pseed), P, A, Cs)
    return ConvLSTMPolicy(A, P, Cs).load_arrays(w).to(DEV), w


def _rings(eng, R, n, Cs):
    E, N, A = eng.E, eng.N, eng.num_actions
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)   # noqa: E731
    return {"obs": z((R, E, N, 15, 15, 3), torch.uint8), "actions": z((R, E, N), torch.int32), "logp": z((R, E, N), torch.float32),
            "value": z((R, E, N), torch.float32), "logits": z((R, E, N, A), torch.float32), "rew": z((R, E, N), torch.int32),
            "done": z((R, E, N), torch.uint8), "last_value": z((E, N), torch.float32), "state_ring": z((n, E, N, 2, Cs), torch.float32)}


def _roll(eng, pol, obs_in, n, r, state, step0=0, greedy=False, every=1, last=True):
    eng.rollout_policy(pol, obs_in, n, r["obs"], actions=r["actions"], logp=r["logp"], value=r["value"], logits=r["logits"],
                       rew=r["rew"], done=r["done"], last_value=r["last_value"] if last else None, step0=step0, greedy=greedy,
                       state=state, state_ring=r["state_ring"], state_every=every)


def _host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _within_bound(got, tor, ref):
    ek = np.abs(np.asarray(got, np.float64) - ref).max()
    et = np.abs(np.asarray(tor, np.float64) - ref).max()
    assert ek <= 4 * et + 1e-6, (ek, et)


# ---------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("Cs", [128, 256])
@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("game", [K.GAME_HARVEST, K.GAME_CLEANUP])
def test_forward_against_restatement(game, P, Cs):
    A = 8 if game == K.GAME_HARVEST else 9
    eng, obs0 = _engine(game, 96, 5)
    pol, w = _policy(A, P, Cs, pseed=P + Cs + A)
    g = torch.Generator(device=DEV).manual_seed(P + Cs)
    noise = torch.randint(0, 256, (40, 5, 15, 15, 3), dtype=torch.uint8, device=DEV, generator=g)
    for obs in (obs0, noise):
        B = obs.shape[0]
        state = torch.randn((B, 5, 2, Cs), device=DEV, generator=g)
        starts = torch.rand((B, 5), device=DEV, generator=g) < 0.3
        lg, v, ns = eng.policy_forward(pol, obs, state=state, starts=starts)
        lg2, v2, ns2 = eng.policy_forward(pol, obs, state=state, starts=starts)
        with torch.no_grad():
            tl, tv, ts = pol(obs, state, starts)
        torch.cuda.synchronize()
        assert torch.equal(lg, lg2) and torch.equal(v, v2) and torch.equal(ns, ns2), "two calls on the same input differ"
        rl, rv, rs = ref_forward(w, obs.cpu().numpy(), state.cpu().numpy(), starts.cpu().numpy())
        for got, tor, ref in ((lg, tl, rl), (v, tv, rv), (ns[..., 0, :], ts[..., 0, :], rs[..., 0, :]), (ns[..., 1, :], ts[..., 1, :], rs[..., 1, :])):
            _within_bound(got.cpu().numpy(), tor.cpu().numpy(), ref)
        assert np.ptp(rl) > 1e-2 and np.ptp(rs[..., 1, :]) > 1e-2


# ---------------------------------------------------------------------------------------------------- 2. start rule
@pytest.mark.parametrize("Cs", [64, 128, 256])
def test_start_rule_never_reads_the_state(Cs):
    eng, obs0 = _engine(K.GAME_HARVEST, 70, 5)
    pol, _ = _policy(8, 5, Cs, pseed=2)
    g = torch.Generator(device=DEV).manual_seed(Cs)
    state = torch.randn((70, 5, 2, Cs), device=DEV, generator=g)
    starts = torch.rand((70, 5), device=DEV, generator=g) < 0.4
    poisoned = state.clone()
    poisoned[starts] = float("nan")
    zeroed = state.clone()
    zeroed[starts] = 0.0
    a = eng.policy_forward(pol, obs0, state=poisoned, starts=starts)
    b = eng.policy_forward(pol, obs0, state=zeroed)
    c = eng.policy_forward(pol, obs0, state=zeroed, starts=starts.to(torch.uint8))
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.isfinite(x).all()
        assert torch.equal(x, y) and torch.equal(x, z)


# ---------------------------------------------------------------------------------------------------- 3-4. rollout
@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("game,P,Cs", [(K.GAME_HARVEST, 5, 128), (K.GAME_CLEANUP, 1, 256)])
def test_rollout_step_by_step(game, P, Cs, greedy):
    E, N, n, horizon, seed = 128, 5, 24, 10, 7
    A = 8 if game == K.GAME_HARVEST else 9
    pol, w = _policy(A, P, Cs, pseed=11 + Cs)
    eng, _ = _engine(game, E, N, seed=seed, horizon=horizon)
    for _ in range(3):                                        # not a fresh reset: the first auto reset comes at step 6
        eng.step_random(auto_reset=True)
    obs_in = eng.observe()
    st0 = eng.get_state()
    state = torch.randn((E, N, 2, Cs), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    s_start = state.clone()
    r = _rings(eng, n, n, Cs)
    _roll(eng, pol, obs_in, n, r, state, greedy=greedy)
    h = _host(r)
    final = state.cpu().numpy()
    assert np.array_equal(h["state_ring"][0], s_start.cpu().numpy()), "step 0 used the state given (t > 0 everywhere)"
    ended = [k for k in range(n) if h["done"][k].any()]
    assert ended == [6, 16] and h["done"][6].all()
    prev = np.concatenate([obs_in.cpu().numpy()[None], h["obs"][:-1]])
    for k in range(n):
        st_in = h["state_ring"][k]
        rl, rv, rs = ref_forward(w, prev[k], st_in)
        with torch.no_grad():
            tl, tv, ts = pol(torch.from_numpy(prev[k]).to(DEV), torch.from_numpy(st_in).to(DEV))
        _within_bound(h["logits"][k], tl.cpu().numpy(), rl)
        _within_bound(h["value"][k], tv.cpu().numpy(), rv)
        nxt = h["state_ring"][k + 1] if k + 1 < n else final
        d = h["done"][k][:, 0] != 0
        if d.any():
            assert np.all(nxt[d] == 0.0), "the state after a done is exactly zero"
        if (~d).any():
            _within_bound(nxt[~d], ts.cpu().numpy()[~d], rs[~d])
    if greedy:
        assert np.array_equal(h["actions"], h["logits"].argmax(-1).astype(np.int32))
    else:
        _check_sampled(eng, st0, h)
        assert len(np.unique(h["actions"])) > 1
    # 4. the env side: replaying the recorded actions through step() gives the same obs / rew / done
    rep = _check_replay(game, E, N, seed, horizon, st0, h)
    a, b = eng.get_state(), rep.get_state()
    for key in ("world", "pos", "orient", "episode", "t"):
        assert np.array_equal(a[key], b[key]), key
    assert eng.status() == 0


# ---------------------------------------------------------------------------------------------------- 5. determinism
def test_call_splitting_ring_lengths_and_last_value():
    E, N, Cs, n, seed, horizon = 64, 5, 128, 24, 9, 10
    pol, _ = _policy(8, 5, Cs, pseed=4)
    outs = []
    for mode in ("one", "split", "ring1", "every3", "no_last"):
        eng, obs0 = _engine(K.GAME_HARVEST, E, N, seed=seed, horizon=horizon)
        state = torch.full((E, N, 2, Cs), 0.25, device=DEV)
        if mode in ("one", "no_last"):
            r = _rings(eng, n, n, Cs)
            _roll(eng, pol, obs0, n, r, state, last=mode == "one")
        elif mode == "split":
            r = _rings(eng, n, n, Cs)
            ring = r["state_ring"]
            r["state_ring"] = ring[:7]
            _roll(eng, pol, obs0, 7, r, state)
            r["state_ring"] = ring[7:]
            _roll(eng, pol, r["obs"][6].clone(), n - 7, r, state, step0=7)
            r["state_ring"] = ring
        elif mode == "ring1":
            r = _rings(eng, 1, n, Cs)
            _roll(eng, pol, obs0, n, r, state)
        else:
            r = _rings(eng, n, 8, Cs)
            _roll(eng, pol, obs0, n, r, state, every=3)
        o = _host(r)
        o["final"] = state.cpu().numpy()
        if mode == "one":
            # last_value = the forward on the final observation under the final state (start rule: the envs at t = 0)
            starts = torch.from_numpy(eng.get_state()["t"] == 0).to(DEV)[:, None].expand(E, N).contiguous()
            lv = eng.policy_forward(pol, r["obs"][n - 1], state=state, starts=starts)[1]
            torch.cuda.synchronize()
            assert np.array_equal(lv.cpu().numpy(), o["last_value"])
        outs.append(o)
    one, split, ring1, every3, no_last = outs
    for k in KEYS + ("state_ring", "final", "last_value"):
        assert np.array_equal(one[k], split[k]), k
    for k in KEYS:
        assert np.array_equal(one[k][n - 1], ring1[k][0]), k
        assert np.array_equal(one[k], every3[k]), k
        assert np.array_equal(one[k], no_last[k]), k
    for k in ("final", "last_value"):
        assert np.array_equal(one[k], ring1[k]) and np.array_equal(one[k], every3[k]), k
    assert np.array_equal(one["state_ring"][::3], every3["state_ring"])
    assert np.array_equal(one["final"], no_last["final"]), "the last_value pass advanced the state"
    assert not np.array_equal(one["state_ring"][1], one["state_ring"][2])


# ---------------------------------------------------------------------------------------------------- 6. learner path
def test_forward_sequence_reproduces_the_rollout_and_backpropagates():
    E, N, Cs, n, seed, horizon = 32, 5, 128, 12, 5, 5
    pol, w = _policy(8, 5, Cs, pseed=6)
    eng, obs0 = _engine(K.GAME_HARVEST, E, N, seed=seed, horizon=horizon)
    state = torch.zeros((E, N, 2, Cs), device=DEV)
    r = _rings(eng, n, n, Cs)
    _roll(eng, pol, obs0, n, r, state)
    h = _host(r)
    prev = torch.cat([obs0[None], r["obs"][:-1]])
    resets = torch.zeros((n, E, N), dtype=torch.bool, device=DEV)
    resets[1:] = r["done"][:-1] != 0
    lg, v, _ = pol.forward_sequence(prev, r["state_ring"][0], resets)
    st = h["state_ring"][0]
    refs = []
    prev_h = prev.cpu().numpy()
    res_h = resets.cpu().numpy()
    for k in range(n):
        rl, rv, st = ref_forward(w, prev_h[k], st, res_h[k])
        refs.append(rl)
    refs = np.stack(refs)
    assert res_h.any()
    _within_bound(h["logits"], lg.detach().cpu().numpy(), refs)
    assert np.abs(lg.detach().cpu().numpy() - h["logits"]).max() <= 1e-4
    (lg.square().mean() + v.mean()).backward()
    assert pol.lstm_w.grad is not None and torch.isfinite(pol.lstm_w.grad).all() and pol.lstm_w.grad.abs().sum() > 0


# ---------------------------------------------------------------------------------------------------- 7. rejection
def test_rejection_leaves_engine_and_state_alone():
    E, N, Cs = 8, 5, 128
    eng, obs0 = _engine(K.GAME_HARVEST, E, N, horizon=4)
    pol, _ = _policy(8, 1, Cs)
    st0 = eng.get_state()
    state = torch.randn((E, N, 2, Cs), device=DEV)
    s_copy = state.clone()
    r = _rings(eng, 3, 3, Cs)

    def call(policy=pol, n=3, st=state, ring=r["state_ring"], every=1):
        eng.rollout_policy(policy, obs0, n, r["obs"], actions=r["actions"], state=st, state_ring=ring, state_every=every)

    bad_calls = [
        lambda: call(st=None),                                              # the recurrent policy needs a state
        lambda: call(st=torch.zeros((E, N, 2, 256), device=DEV)),           # another C
        lambda: call(st=torch.zeros((E, N, 2, Cs), device=DEV, dtype=torch.float64)),
        lambda: call(st=torch.zeros((E, N, Cs, 2), device=DEV)),
        lambda: call(st=torch.zeros((E, N, 2, Cs))),                        # on the CPU
        lambda: call(st=torch.zeros((E, N, 2, 2 * Cs), device=DEV)[..., ::2]),   # not contiguous
        lambda: call(ring=r["state_ring"][:2]),                             # ceil(3 / 1) = 3 slots needed
        lambda: call(ring=r["state_ring"][:1], every=2),
        lambda: call(ring=r["state_ring"], every=0),
        lambda: call(ring=r["state_ring"].double()),
        lambda: call(ring=r["state_ring"][:, :4]),
        lambda: call(ring=torch.zeros((3, E, N, 2, 64), device=DEV)),
        lambda: call(ring=state[None]),                                     # overlaps the state
        lambda: call(policy=ConvFCPolicy(8, 1).to(DEV)),                    # a feed-forward policy has no state
        lambda: eng.rollout_policy(ConvFCPolicy(8, 1).to(DEV), obs0, 3, r["obs"], state_ring=r["state_ring"]),
        lambda: call(policy=ConvLSTMPolicy(8, 1, Cs)),                      # parameters on the CPU
        lambda: call(policy=_policy(9, 1, Cs)[0]),
        lambda: eng.policy_forward(pol, obs0),                              # no state
        lambda: eng.policy_forward(pol, obs0, state=state[:4]),
        lambda: eng.policy_forward(pol, obs0, state=state, starts=torch.zeros((E, N), dtype=torch.int32, device=DEV)),
        lambda: eng.policy_forward(pol, obs0, state=state, starts=torch.zeros(E, dtype=torch.bool, device=DEV)),
        lambda: eng.policy_forward(ConvFCPolicy(8, 1).to(DEV), obs0, state=state),
    ]
    for f in bad_calls:
        with pytest.raises(ValueError):
            f()
    # the C side rejects the same things before launching
    L, w = _capi.lib(), pol.packed()
    dp = lambda t: C.c_void_p(t.data_ptr())                                # noqa: E731
    feat = torch.zeros((E, N, 32), device=DEV)

    def c_call(cs=Cs, ring_len=3, every=1, st=state, f=feat):
        return L.ssd_rollout_policy_lstm(eng._h, dp(w), 1, cs, dp(obs0), 3, 0, None if st is None else dp(st), dp(r["state_ring"]),
                                         ring_len, every, None if f is None else dp(f), dp(r["obs"]), dp(r["actions"]),
                                         None, None, None, None, None, 3, None, 0, None)
    for kw in ({"cs": 100}, {"cs": 512}, {"ring_len": 2}, {"every": 0}, {"st": None}, {"f": None}):
        assert c_call(**kw) == _capi.SSD_E_INVALID, kw
    out = torch.zeros((E, N, 2, Cs), device=DEV)
    assert L.ssd_policy_lstm_forward(dp(w), 1, 8, 96, dp(obs0), dp(state), None, E, N, dp(feat), dp(out), None, None, 0, 0,
                                     None) == _capi.SSD_E_INVALID
    assert L.ssd_policy_lstm_forward(dp(w), 1, 8, Cs, dp(obs0), dp(state), None, E, N, dp(feat), C.c_void_p(state.data_ptr() + 4),
                                     None, None, 0, 0, None) == _capi.SSD_E_INVALID
    torch.cuda.synchronize()
    st = eng.get_state()
    for key in ("world", "pos", "orient", "episode", "t"):
        assert np.array_equal(st0[key], st[key]), key
    assert torch.equal(state, s_copy)
    assert eng.status() == 0


# ---------------------------------------------------------------------------------------------------- 8. adapter
def test_adapter_sample_carries_the_state():
    E, N, seed, horizon, n, Cs = 64, 5, 17, 7, 10, 128
    pol, _ = _policy(8, 5, Cs, pseed=3)
    outs = []
    for split in (False, True):
        env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=horizon, seed=seed)
        env.reset()
        if split:
            a = env.sample(pol, n // 2, state_every=1)
            b = env.sample(pol, n // 2, state_every=1)
            out = {k: torch.cat([a[k], b[k]]) for k in ("obs", "actions", "logp", "value", "rew", "done", "state")}
            out["last_value"] = b["last_value"]
            assert torch.equal(b["state_in"], b["state"][0]) and b["state_in"].abs().sum() > 0
        else:
            out = env.sample(pol, n, state_every=1)
            assert not out["state_in"].any(), "the first state after reset() is zero"
        outs.append({k: v.cpu().numpy() for k, v in out.items() if k != "state_in"})
    one, two = outs
    for k in one:
        assert np.array_equal(one[k], two[k]), k
    # the same as one engine call from a zero state
    eng, obs0 = _engine(K.GAME_HARVEST, E, N, seed=seed, horizon=horizon)
    r = _rings(eng, n, n, Cs)
    _roll(eng, pol, obs0, n, r, torch.zeros((E, N, 2, Cs), device=DEV))
    ref = _host(r)
    for k in ("obs", "actions", "logp", "value", "rew", "done", "last_value"):
        assert np.array_equal(one[k], ref[k]), k
    assert np.array_equal(one["state"], ref["state_ring"])
    # without state_every: state_in alone; another cell size raises until reset()
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=horizon, seed=seed)
    env.reset()
    out = env.sample(pol, 3)
    assert "state" not in out and out["state_in"].shape == (E, N, 2, Cs)
    out = env.sample(pol, 3)
    assert out["state_in"].abs().sum() > 0
    other, _ = _policy(8, 5, 64)
    with pytest.raises(ValueError):
        env.sample(other, 2)
    env.reset()
    out = env.sample(other, 2)
    assert out["state_in"].shape == (E, N, 2, 64) and not out["state_in"].any()
    with pytest.raises(ValueError):
        env.sample(ConvFCPolicy(8, 5).to(DEV), 2, state_every=1)
