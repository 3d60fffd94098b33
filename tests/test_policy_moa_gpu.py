"""MOA policy rollouts on the MI355X (csrc/ssd_policy_moa.hip, ssd_policy_moa_forward, ssd_rollout_policy_moa): the forward and
the influence against the float64 restatement (policy_moa_ref.py), moa_logits as a counterfactual, the start rule, the
rollout step by step against the forward, determinism across call splits and ring lengths, argument checks and the adapter."""
import numpy as np
import pytest
import torch

from policy_moa_ref import forward as ref_forward, influence as ref_influence, random_weights
from test_policy_gpu import _check_replay
from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd.engine import VecEngine
from sequential_social_dilemma_games_amd.policy import ConvMOAPolicy, influence
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
KEYS = ("obs", "actions", "logp", "value", "logits", "rew", "done", "influence", "prev_actions")


def _engine(game, E, N, seed=3, horizon=0):
    eng = VecEngine(game, None, num_envs=E, num_agents=N, seed=seed)
    if horizon:
        eng.set_horizon(horizon)
    return eng, eng.reset()


def _policy(A, N, P, Cs, pseed=0):
    w = random_weights(np.random.default_rng(pseed), P, A, N, Cs)
    return ConvMOAPolicy(A, N, P, Cs).load_arrays(w).to(DEV), w


def _within_bound(got, tor, ref):
    ek = np.abs(np.asarray(got, np.float64) - ref).max()
    et = np.abs(np.asarray(tor, np.float64) - ref).max()
    assert ek <= 4 * et + 1e-6, (ek, et)


def _rings(eng, R, n, Cs):
    E, N, A = eng.E, eng.N, eng.num_actions
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)   # noqa: E731
    return {"obs": z((R, E, N, 15, 15, 3), torch.uint8), "actions": z((R, E, N), torch.int32), "logp": z((R, E, N), torch.float32),
            "value": z((R, E, N), torch.float32), "logits": z((R, E, N, A), torch.float32), "rew": z((R, E, N), torch.int32),
            "done": z((R, E, N), torch.uint8), "influence": z((R, E, N), torch.float32), "prev_actions": z((R, E, N), torch.int32),
            "last_value": z((E, N), torch.float32), "state_ring": z((n, E, N, 4, Cs), torch.float32)}


def _roll(eng, pol, obs_in, n, r, state, prev, step0=0, greedy=False, clip=10.0):
    eng.rollout_policy(pol, obs_in, n, r["obs"], actions=r["actions"], logp=r["logp"], value=r["value"], logits=r["logits"],
                       rew=r["rew"], done=r["done"], last_value=r["last_value"], step0=step0, greedy=greedy, state=state,
                       state_ring=r["state_ring"], prev_actions=prev, prev_actions_ring=r["prev_actions"],
                       influence=r["influence"], influence_clip=clip)


def _host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


# ---------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("game,N,P,Cs", [(K.GAME_HARVEST, 5, 5, 128), (K.GAME_HARVEST, 5, 1, 64), (K.GAME_CLEANUP, 5, 1, 256),
                                         (K.GAME_CLEANUP, 2, 2, 128), (K.GAME_HARVEST, 10, 10, 64), (K.GAME_CLEANUP, 10, 1, 128)])
def test_forward_against_restatement(game, N, P, Cs):
    A = 8 if game == K.GAME_HARVEST else 9
    eng, obs0 = _engine(game, 40, N)
    pol, w = _policy(A, N, P, Cs, pseed=N + P + Cs)
    g = torch.Generator(device=DEV).manual_seed(P + Cs)
    noise = torch.randint(0, 256, (24, N, 15, 15, 3), dtype=torch.uint8, device=DEV, generator=g)
    for obs in (obs0, noise):
        B = obs.shape[0]
        state = torch.randn((B, N, 4, Cs), device=DEV, generator=g) * 0.5
        starts = torch.rand((B, N), device=DEV, generator=g) < 0.3
        prev = torch.randint(0, A, (B, N), dtype=torch.int32, device=DEV, generator=g)
        acts = torch.randint(0, A, (B, N), dtype=torch.int32, device=DEV, generator=g)
        out = eng.policy_forward(pol, obs, state=state, starts=starts, prev_actions=prev, actions=acts)
        out2 = eng.policy_forward(pol, obs, state=state, starts=starts, prev_actions=prev, actions=acts)
        with torch.no_grad():
            tor = pol(obs, prev, state, starts)
        torch.cuda.synchronize()
        for x, y in zip(out, out2):
            assert torch.equal(x, y), "two calls on the same input differ"
        lg, v, moa, cf, ns, infl = out
        ref = ref_forward(w, obs.cpu().numpy(), prev.cpu().numpy(), state.cpu().numpy(), starts.cpu().numpy())
        for got, t, rf in zip((lg, v, moa, cf, ns), tor, ref):
            _within_bound(got.cpu().numpy(), t.cpu().numpy(), rf)
        assert np.ptp(ref[3]) > 1e-2 and np.ptp(ref[4][..., 2, :]) > 1e-2
        # moa_logits IS the counterfactual of the own previous action (zero at a start)
        own = torch.where(starts, torch.zeros_like(prev), prev).long()
        pick = torch.gather(cf, 2, own[:, :, None, None, None].expand(B, N, 1, N - 1, A))[:, :, 0]
        assert torch.equal(moa, pick)
        # the device influence against influence() on the device's own outputs (float32, log space in both): the two sum
        # the same terms in other orders, so they agree to a few ulp of the largest term
        ti = influence(lg, cf, acts, 10.0)
        assert torch.isfinite(infl).all()
        assert (infl - ti).abs().max().item() <= 1e-5 + 1e-4 * ti.abs().max().item()
        ri = ref_influence(ref[0].reshape(-1, A), ref[3].reshape(-1, A, N - 1, A), acts.cpu().numpy().reshape(-1))
        assert np.abs(infl.cpu().numpy().reshape(-1) - ri).max() <= 1e-4 + 1e-3 * np.abs(ri).max()


# ---------------------------------------------------------------------------------------------------- 2. start rule
@pytest.mark.parametrize("Cs", [64, 256])
def test_start_rule_never_reads_state_or_previous_actions(Cs):
    N, A = 5, 8
    eng, obs0 = _engine(K.GAME_HARVEST, 50, N)
    pol, _ = _policy(A, N, N, Cs, pseed=2)
    g = torch.Generator(device=DEV).manual_seed(Cs)
    state = torch.randn((50, N, 4, Cs), device=DEV, generator=g)
    starts = (torch.rand((50, 1), device=DEV, generator=g) < 0.4).expand(50, N).contiguous()   # per env, as the rollout's
    prev = torch.randint(0, A, (50, N), dtype=torch.int32, device=DEV, generator=g)
    acts = torch.randint(0, A, (50, N), dtype=torch.int32, device=DEV, generator=g)
    poisoned, zeroed = state.clone(), state.clone()
    poisoned[starts] = float("nan")
    zeroed[starts] = 0.0
    garbage, zprev = prev.clone(), prev.clone()
    garbage[starts] = 123456
    zprev[starts] = 0
    # a start row's previous-action vector is zero: every agent's slot of that row, not only its own
    a = eng.policy_forward(pol, obs0, state=poisoned, starts=starts, prev_actions=garbage, actions=acts)
    c = eng.policy_forward(pol, obs0, state=zeroed, starts=starts.to(torch.uint8), prev_actions=prev, actions=acts)
    torch.cuda.synchronize()
    for x, z in zip(a, c):
        assert torch.isfinite(x).all()
        assert torch.equal(x, z)
    rows = starts.all(dim=1)                                    # envs where every agent starts: the whole vector is zero
    if rows.any():
        b = eng.policy_forward(pol, obs0[rows], state=zeroed[rows], prev_actions=zprev[rows] * 0, actions=acts[rows])
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert torch.equal(x[rows], y)


# ---------------------------------------------------------------------------------------------------- 3. rollout
@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("game,P,Cs", [(K.GAME_HARVEST, 5, 128), (K.GAME_CLEANUP, 1, 64)])
def test_rollout_step_by_step(game, P, Cs, greedy):
    E, N, n, horizon, seed = 64, 5, 16, 10, 7
    A = 8 if game == K.GAME_HARVEST else 9
    pol, w = _policy(A, N, P, Cs, pseed=11 + Cs)
    eng, _ = _engine(game, E, N, seed=seed, horizon=horizon)
    for _ in range(3):
        eng.step_random(auto_reset=True)
    obs_in = eng.observe()
    st0 = eng.get_state()
    g = torch.Generator(device=DEV).manual_seed(1)
    state = torch.randn((E, N, 4, Cs), device=DEV, generator=g) * 0.5
    prev = torch.randint(0, A, (E, N), dtype=torch.int32, device=DEV, generator=g)
    prev0 = prev.clone()
    r = _rings(eng, n, n, Cs)
    _roll(eng, pol, obs_in, n, r, state, prev, greedy=greedy)
    h = _host(r)
    final, final_prev = state.cpu().numpy(), prev.cpu().numpy()
    assert np.array_equal(h["prev_actions"][0], prev0.cpu().numpy()), "step 0 read the carried joint action (t > 0)"
    assert np.array_equal(final_prev, h["actions"][n - 1]), "the carried joint action is the last step's"
    ended = [k for k in range(n) if h["done"][k].any()]
    assert ended == [6] and h["done"][6].all()
    assert np.all(h["prev_actions"][7] == 0) and np.all(h["state_ring"][7] == 0), "an episode start reads zeros"
    obs_prev = np.concatenate([obs_in.cpu().numpy()[None], h["obs"][:-1]])
    for k in range(n):
        # the forward on what step k read (after the start rule) reproduces the step bitwise
        o = [torch.from_numpy(x).to(DEV) for x in (obs_prev[k], h["state_ring"][k], h["prev_actions"][k], h["actions"][k])]
        lg, v, moa, cf, ns, infl = eng.policy_forward(pol, o[0], state=o[1], prev_actions=o[2], actions=o[3])
        torch.cuda.synchronize()
        assert np.array_equal(lg.cpu().numpy(), h["logits"][k]) and np.array_equal(v.cpu().numpy(), h["value"][k])
        assert np.array_equal(infl.cpu().numpy(), h["influence"][k])
        nxt = h["state_ring"][k + 1] if k + 1 < n else final
        d = h["done"][k][:, 0] != 0
        assert np.array_equal(ns.cpu().numpy()[~d], nxt[~d])
        if k + 1 < n:
            assert np.array_equal(h["prev_actions"][k + 1][~d], h["actions"][k][~d])
        lsm = torch.log_softmax(lg.double(), -1).cpu().numpy()
        assert np.abs(np.take_along_axis(lsm, h["actions"][k][..., None].astype(np.int64), -1)[..., 0] - h["logp"][k]).max() < 1e-5
        if k in (0, n - 1):                                     # the float64 check, on the kernel's own recorded actions
            ref = ref_forward(w, obs_prev[k], h["prev_actions"][k], h["state_ring"][k])
            _within_bound(h["logits"][k], lg.cpu().numpy(), ref[0])
            ri = ref_influence(ref[0].reshape(-1, A), ref[3].reshape(-1, A, N - 1, A), h["actions"][k].reshape(-1))
            assert np.abs(h["influence"][k].reshape(-1) - ri).max() <= 1e-4 + 1e-3 * np.abs(ri).max()
    if greedy:
        assert np.array_equal(h["actions"], h["logits"].argmax(-1).astype(np.int32))
    else:
        assert len(np.unique(h["actions"])) > 1
    assert np.all(np.isfinite(h["influence"])) and h["influence"].min() >= -1e-6 and h["influence"].max() > 0
    rep = _check_replay(game, E, N, seed, horizon, st0, {k: h[k] for k in ("obs", "actions", "rew", "done")})
    a, b = eng.get_state(), rep.get_state()
    for key in ("world", "pos", "orient", "episode", "t"):
        assert np.array_equal(a[key], b[key]), key


# ---------------------------------------------------------------------------------------------------- 4. determinism
def test_call_splitting_and_ring_lengths():
    E, N, Cs, n, seed, horizon = 32, 5, 64, 16, 9, 6
    pol, _ = _policy(8, N, 5, Cs, pseed=4)
    outs = []
    for mode in ("one", "split", "ring1", "ring3"):
        eng, obs0 = _engine(K.GAME_HARVEST, E, N, seed=seed, horizon=horizon)
        state = torch.zeros((E, N, 4, Cs), device=DEV)
        prev = torch.zeros((E, N), dtype=torch.int32, device=DEV)
        if mode == "one":
            r = _rings(eng, n, n, Cs)
            _roll(eng, pol, obs0, n, r, state, prev)
        elif mode == "split":
            r = _rings(eng, n, n, Cs)
            ring = r["state_ring"]
            r["state_ring"] = ring[:8]
            _roll(eng, pol, obs0, 8, r, state, prev)
            r["state_ring"] = ring[8:]
            _roll(eng, pol, r["obs"][7].clone(), n - 8, r, state, prev, step0=8)
            r["state_ring"] = ring
        else:
            R = 1 if mode == "ring1" else 3
            r = _rings(eng, R, n, Cs)
            _roll(eng, pol, obs0, n, r, state, prev)
        o = _host(r)
        o["final"], o["final_prev"] = state.cpu().numpy(), prev.cpu().numpy()
        outs.append(o)
    one, split, ring1, ring3 = outs
    assert one["done"].any()
    for k in KEYS + ("state_ring", "final", "final_prev", "last_value"):
        assert np.array_equal(one[k], split[k]), k
    for k in KEYS:
        assert np.array_equal(one[k][n - 1], ring1[k][0]), k
        assert np.array_equal(one[k][n - 3:], ring3[k][[(n - 3) % 3, (n - 2) % 3, (n - 1) % 3]]), k
    for k in ("state_ring", "final", "final_prev", "last_value"):
        assert np.array_equal(one[k], ring1[k]) and np.array_equal(one[k], ring3[k]), k


# ---------------------------------------------------------------------------------------------------- 5. arguments
def test_bad_arguments_are_rejected_before_anything_is_enqueued():
    E, N, Cs = 16, 5, 64
    eng, obs0 = _engine(K.GAME_HARVEST, E, N)
    pol, _ = _policy(8, N, 5, Cs)
    r = _rings(eng, 2, 4, Cs)
    state = torch.randn((E, N, 4, Cs), device=DEV)
    prev = torch.ones((E, N), dtype=torch.int32, device=DEV)
    s0, p0, g0 = state.clone(), prev.clone(), eng.get_state()
    bad = [dict(policy=_policy(8, N, 1, 128)[0], state=state),                       # C of the state differs
           dict(state=torch.zeros((E, N, 2, Cs), device=DEV)),                      # an LSTM-sized state
           dict(prev=torch.ones((E, N - 1), dtype=torch.int32, device=DEV)),
           dict(influence=torch.zeros((3, E, N), device=DEV)),
           dict(prev_ring=torch.zeros((2, E, N + 1), dtype=torch.int32, device=DEV)),
           dict(state_ring=torch.zeros((1, E, N, 4, Cs), device=DEV)),              # 4 steps need 4 slots
           dict(clip=float("nan"))]
    for b in bad:
        with pytest.raises(ValueError):
            eng.rollout_policy(b.get("policy", pol), obs0, 4, r["obs"], actions=r["actions"], state=b.get("state", state),
                               state_ring=b.get("state_ring", r["state_ring"]), prev_actions=b.get("prev", prev),
                               prev_actions_ring=b.get("prev_ring", r["prev_actions"]), influence=b.get("influence", r["influence"]),
                               influence_clip=b.get("clip", 10.0))
    with pytest.raises(ValueError):                                                  # wrong P
        ConvMOAPolicy(8, N, 3, Cs)
    with pytest.raises(ValueError):                                                  # N = 1
        ConvMOAPolicy(8, 1, 1, Cs)
    with pytest.raises(ValueError):                                                  # the policy's N is not the engine's
        eng.rollout_policy(_policy(8, 4, 1, Cs)[0], obs0, 4, r["obs"], state=state, prev_actions=prev)
    torch.cuda.synchronize()
    assert torch.equal(state, s0) and torch.equal(prev, p0)
    g1 = eng.get_state()
    for key in ("world", "pos", "t", "episode"):
        assert np.array_equal(g0[key], g1[key])
    # the C library's own checks (N = 1, view_len != 7, wrong P, wrong C)
    L = _capi.lib()
    one, _ = _engine(K.GAME_HARVEST, E, 1)
    wide = VecEngine(K.GAME_HARVEST, None, num_envs=E, num_agents=N, seed=1, view_len=5)
    wide.reset()
    w = pol.packed()
    scratch = torch.empty(_capi.SSD_MOA_SCRATCH_FLOATS(E * N), device=DEV)
    for h, P, C in ((one._h, 1, Cs), (wide._h, 1, Cs), (eng._h, 3, Cs), (eng._h, 5, 96)):
        rc = L.ssd_rollout_policy_moa(h, w.data_ptr(), P, C, obs0.data_ptr(), 4, 0, state.data_ptr(), None, 0, 1,
                                      prev.data_ptr(), None, None, 10.0, scratch.data_ptr(), r["obs"].data_ptr(),
                                      r["actions"].data_ptr(), None, None, None, None, None, 2, None, 0, None)
        assert rc == _capi.SSD_E_INVALID
    torch.cuda.synchronize()
    assert torch.equal(state, s0) and torch.equal(prev, p0)


# ---------------------------------------------------------------------------------------------------- 6. the adapter
def test_vector_env_sample_carries_state_and_previous_actions():
    E, N, Cs, horizon = 32, 5, 64, 7
    pol, _ = _policy(8, N, 1, Cs, pseed=5)
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=horizon, seed=21)
    env.reset()
    a = env.sample(pol, 5, influence_weight=0.5)
    b = env.sample(pol, 6, state_every=2)
    eng, obs0 = _engine(K.GAME_HARVEST, E, N, seed=21, horizon=horizon)
    state = torch.zeros((E, N, 4, Cs), device=DEV)
    prev = torch.zeros((E, N), dtype=torch.int32, device=DEV)
    r = _rings(eng, 11, 11, Cs)
    _roll(eng, pol, obs0, 11, r, state, prev)
    h = _host(r)
    ha = {k: v.cpu().numpy() for k, v in a.items()}
    hb = {k: v.cpu().numpy() for k, v in b.items()}
    for k in ("obs", "actions", "logp", "value", "rew", "done", "influence", "prev_actions"):
        assert np.array_equal(np.concatenate([ha[k], hb[k]]), h[k]), k
    assert np.array_equal(ha["rewards"], (h["rew"][:5] + np.float32(0.5) * h["influence"][:5]).astype(np.float32))
    assert np.array_equal(hb["rewards"], (h["rew"][5:] + h["influence"][5:]).astype(np.float32))
    assert np.array_equal(hb["state_in"], h["state_ring"][5]) and np.array_equal(hb["state"], h["state_ring"][5::2])
    assert np.all(ha["state_in"] == 0) and np.all(ha["prev_actions"][0] == 0)
    env.reset()
    c = env.sample(pol, 2)
    assert np.all(c["state_in"].cpu().numpy() == 0) and np.all(c["prev_actions"][0].cpu().numpy() == 0)


# ---------------------------------------------------------------------------------------------------- 7. full size
def test_full_size_influence_is_a_clipped_kl():
    E, N, Cs, clip = 4096, 5, 128, 0.05
    pol = ConvMOAPolicy(8, N, N, Cs, seed=3).to(DEV)
    eng, obs0 = _engine(K.GAME_HARVEST, E, N, seed=5, horizon=1000)
    state = torch.zeros((E, N, 4, Cs), device=DEV)
    prev = torch.zeros((E, N), dtype=torch.int32, device=DEV)
    r = _rings(eng, 4, 1, Cs)
    r["state_ring"] = None
    eng.rollout_policy(pol, obs0, 4, r["obs"], actions=r["actions"], state=state, prev_actions=prev,
                       influence=r["influence"], influence_clip=clip)
    infl = r["influence"].cpu().numpy()
    assert np.all(np.isfinite(infl)) and infl.min() >= -1e-6 and infl.max() <= clip
    assert np.all(np.isfinite(state.cpu().numpy()))
