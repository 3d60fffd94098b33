"""Watershed policy rollouts on the MI355X (csrc/ssd_ws_policy.hip, ssd_ws_policy_forward, ssd_ws_rollout_policy): the forward
against the float64 restatement (policy_ws_ref.py) with the acting agents mixed within a tile, the start rule, the rollout step
by step in lock step and after a masked reset, the sampled actions against the host mirrors of the draws, the env side against a
second engine and the NumPy mirror, determinism across call splits and ring lengths, the BPTT path, argument checks, sample()."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import policy_ws_ref as ref
from watershed_mirror import WatershedMirror
from sequential_social_dilemma_games_amd import _capi, prng
from sequential_social_dilemma_games_amd.policy import WatershedLSTMPolicy, cdf_margin, sample_gaussian_host, sample_host
from sequential_social_dilemma_games_amd.watershed import WatershedVecEngine

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEQ, SEQ_COMM = _capi.SSD_WS_SEQ, _capi.SSD_WS_SEQ_COMM
VARIANTS = [SEQ, SEQ_COMM]
SEED, BASE = 11, 1000
RING_KEYS = ("obs", "agent", "rew", "done", "actor", "actions", "logp", "value", "dist", "state_ring")


def _policy(variant, Cs, pseed=0, share=False):
    w = ref.random_weights(np.random.default_rng(pseed), variant, Cs, share=share)
    return WatershedLSTMPolicy(variant, cell_size=Cs, share_comm_layer=share).load_arrays(w).to(DEV), w


def _within_bound(got, tor, want):
    ek = np.abs(np.asarray(got, np.float64) - want).max()
    et = np.abs(np.asarray(tor, np.float64) - want).max()
    print("kernel max error %.3e, torch float32 max error %.3e" % (ek, et))
    assert ek <= 4 * et + 1e-6, (ek, et)


def _is_comm(variant, agent):
    return (variant == SEQ_COMM) & (np.asarray(agent) < 4)


def _clip(variant, actor, actions):
    """What the env steps with: an action agent's action clipped to [0, 1], a comm agent's message as it is."""
    a = np.asarray(actions, np.float32)
    return np.where(_is_comm(variant, actor), a, np.fmin(np.fmax(a, np.float32(0)), np.float32(1))).astype(np.float32)


def _fresh(variant, E):
    """An engine that is NOT at a fresh reset: six fixed steps in.  Deterministic, so every call gives the same state."""
    eng = WatershedVecEngine(variant, E, seed=SEED, env_index_base=BASE)
    obs, agent = eng.reset()
    for j in range(6):
        a = torch.where(agent < (4 if variant == SEQ_COMM else 0), torch.full((E,), float(j % 5), device=DEV),
                        torch.full((E,), 0.3, device=DEV))
        obs, agent, _, _ = eng.step(a, auto_reset=True)
    return eng, obs, agent


def _rings(E, R, Cs, S):
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)   # noqa: E731
    return {"obs": z((R, E, 12), torch.float32), "agent": z((R, E), torch.int8), "rew": z((R, E), torch.float64),
            "done": z((R, E), torch.uint8), "actor": z((R, E), torch.int8), "actions": z((R, E), torch.float32),
            "logp": z((R, E), torch.float32), "value": z((R, E), torch.float32), "dist": z((R, E, 5), torch.float32),
            "state_ring": z((R, E, 2, Cs), torch.float32), "last_value": z((E,), torch.float32)}


def _roll(eng, pol, obs_in, agent_in, n, r, state, step0=0, greedy=False, last=True):
    eng.rollout_policy(pol, obs_in, agent_in, n, r["obs"], r["agent"], rew=r["rew"], done=r["done"], actor=r["actor"],
                       actions=r["actions"], logp=r["logp"], value=r["value"], dist=r["dist"], state=state,
                       state_ring=r["state_ring"], last_value=r["last_value"] if last else None, step0=step0, greedy=greedy)


def _host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _init_state(E, S, Cs, seed=1):
    return torch.randn((E, S, 2, Cs), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


# ---------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("Cs", [64, 128, 256])
@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_against_restatement(variant, Cs):
    eng = WatershedVecEngine(variant, 4, seed=1)
    pol, w = _policy(variant, Cs, pseed=Cs + variant)
    S, B = pol.num_sets, 16 * 5 + 7                              # not a multiple of the 16-env tile
    rng = np.random.default_rng(Cs)
    for agent in (rng.integers(0, S, B), np.full(B, S - 1), np.resize(np.repeat(np.arange(S), 16), B)):   # mixed in a tile, uniform, per tile
        obs = torch.from_numpy(ref.random_obs(rng, variant, False, agent)).to(DEV)
        ag = torch.from_numpy(agent.astype(np.int8)).to(DEV)
        state = torch.from_numpy(rng.standard_normal((B, 2, Cs)).astype(np.float32)).to(DEV)
        starts = torch.from_numpy(rng.random(B) < 0.3).to(DEV)
        d, v, ns = eng.policy_forward(pol, obs, ag, state, starts)
        d2, v2, ns2 = eng.policy_forward(pol, obs, ag, state, starts)
        with torch.no_grad():
            td, tv, ts = pol(obs, ag.long(), state, starts)
        torch.cuda.synchronize()
        assert torch.equal(d, d2) and torch.equal(v, v2) and torch.equal(ns, ns2), "two calls on the same input differ"
        rd, rv, rs = ref.forward(w, obs.cpu().numpy(), agent, state.cpu().numpy(), starts.cpu().numpy())
        for got, tor, want in ((d, td, rd), (v, tv, rv), (ns[:, 0], ts[:, 0], rs[:, 0]), (ns[:, 1], ts[:, 1], rs[:, 1])):
            _within_bound(got.cpu().numpy(), tor.cpu().numpy(), want)
        assert np.ptp(rd) > 1e-2 and np.ptp(rs[:, 0]) > 1e-2
    # in place
    st, s8 = state.clone(), starts.to(torch.uint8)
    vp = C.c_void_p
    _capi.policy_check(_capi.lib().ssd_ws_policy_forward(vp(pol.packed().data_ptr()), S, Cs, variant, vp(obs.data_ptr()), vp(ag.data_ptr()),
                                                         vp(st.data_ptr()), vp(s8.data_ptr()), B, vp(st.data_ptr()), None, None, 0, 0,
                                                         vp(torch.cuda.current_stream(DEV).cuda_stream)))
    torch.cuda.synchronize()
    assert torch.equal(st, ns)


# ---------------------------------------------------------------------------------------------------- 2. start rule
@pytest.mark.parametrize("variant", VARIANTS)
def test_start_rule_never_reads_the_state(variant):
    Cs, B = 128, 70
    eng = WatershedVecEngine(variant, 4, seed=1)
    pol, _ = _policy(variant, Cs, pseed=2)
    rng = np.random.default_rng(3)
    agent = rng.integers(0, pol.num_sets, B)
    obs = torch.from_numpy(ref.random_obs(rng, variant, False, agent)).to(DEV)
    ag = torch.from_numpy(agent.astype(np.int8)).to(DEV)
    state = torch.from_numpy(rng.standard_normal((B, 2, Cs)).astype(np.float32)).to(DEV)
    starts = torch.from_numpy(rng.random(B) < 0.4).to(DEV)
    poisoned, zeroed = state.clone(), state.clone()
    poisoned[starts] = float("nan")
    zeroed[starts] = 0.0
    a = eng.policy_forward(pol, obs, ag, poisoned, starts)
    b = eng.policy_forward(pol, obs, ag, zeroed)
    c = eng.policy_forward(pol, obs, ag, zeroed, starts.to(torch.uint8))
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.isfinite(x).all()
        assert torch.equal(x, y) and torch.equal(x, z)


# ---------------------------------------------------------------------------------------------------- 3-5. the rollout
def _steps(variant):
    return 65 if variant == SEQ else 197                         # one and a half episodes (43 / 131 steps)


@functools.lru_cache(maxsize=None)
def _run(variant, greedy, masked):
    """The rollout one step per call, with what each step saw and left: the engine's counters before it, the policy state before
    and after, and torch's float32 forward on the same inputs.  masked: a third of the envs is reset part-way, so that from then
    on a 16-env tile holds several acting agents."""
    E, Cs, n = 256, 128, _steps(variant)
    pol, w = _policy(variant, Cs, pseed=21 + variant)
    S = pol.num_sets
    eng, cur_obs, cur_agent = _fresh(variant, E)
    st0 = eng.get_state()
    state = _init_state(E, S, Cs)
    r = _rings(E, n, Cs, S)
    ar = torch.arange(E, device=DEV)
    mask = (ar % 3) == 1
    k_reset = n // 3 if masked else -1
    rec = {k: [] for k in ("in_obs", "in_agent", "before_row", "after_row", "td", "tv", "ts", "episode", "round", "phase")}
    for k in range(n):
        if k == k_reset:
            o2, a2 = eng.reset(mask)
            cur_obs = torch.where(mask[:, None], o2, cur_obs).contiguous()
            cur_agent = torch.where(mask, a2, cur_agent).contiguous()
        s = eng.get_state()
        before = state.clone()
        _roll(eng, pol, cur_obs, cur_agent, 1, r, state, step0=k, greedy=greedy, last=k == n - 1)
        actor = r["actor"][k].long()
        changed = (before != state).flatten(2).any(-1)
        changed[ar, actor] = False
        assert not bool(changed.any()), "step %d changed the state of an agent that did not act" % k
        with torch.no_grad():
            td, tv, ts = pol(cur_obs, actor, r["state_ring"][k])
        for key, val in (("in_obs", cur_obs), ("in_agent", cur_agent), ("before_row", before[ar, actor]), ("after_row", state[ar, actor]),
                         ("td", td), ("tv", tv), ("ts", ts)):
            rec[key].append(val.cpu().numpy())
        for key in ("episode", "round", "phase"):
            rec[key].append(s[key].astype(np.int64))
        cur_obs, cur_agent = r["obs"][k], r["agent"][k]
    h = _host(r)
    out = {k: np.stack(v) for k, v in rec.items()}
    out.update(h=h, st0=st0, final=eng.get_state(), status=eng.status(), w=w, pol=pol, n=n, E=E, k_reset=k_reset,
               mask=mask.cpu().numpy(), policy_state=state.cpu().numpy(), variant=variant)
    eng.close()
    return out


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("variant", VARIANTS)
def test_rollout_step_by_step(variant, greedy, masked):
    x = _run(variant, greedy, masked)
    h, n, E = x["h"], x["n"], x["E"]
    assert x["status"] == 0
    assert np.array_equal(h["actor"], x["in_agent"]), "the actor is the agent of the observation acted on"
    prev_agent = np.concatenate([x["in_agent"][:1], h["agent"][:-1]])
    if not masked:
        assert np.array_equal(h["actor"], prev_agent) and (h["actor"] == h["actor"][:, :1]).all(), "lock step"
    else:
        k = x["k_reset"]
        keep = np.ones((n, E), bool)
        keep[k, x["mask"]] = False                               # (the masked reset replaced these rows' observation)
        assert np.array_equal(h["actor"][keep], prev_agent[keep])
        mixed = [len(set(h["actor"][j, :16].tolist())) for j in range(n)]
        assert max(mixed[k:]) >= 2 and max(mixed[:k]) == 1, "tiles hold several actors after the masked reset"
    assert (h["done"] & 2).any(), "an episode ends inside the rollout"
    # the start rule: zero state at an agent's first action of an episode, else the carried row, bit for bit
    start = ref.start_rule(variant, x["round"], x["phase"])
    assert start.any() and not start.all()
    used = h["state_ring"]
    assert not used[start].any(), "the state of a first action is exactly zero"
    assert np.array_equal(used[~start], x["before_row"][~start])
    first = {}
    for k in range(n):                                           # the rule against the recorded history itself
        for e in (0, 1, E - 1):
            key = (e, int(x["episode"][k, e]), int(h["actor"][k, e]))
            assert bool(start[k, e]) == (key not in first) or x["episode"][k, e] == x["st0"]["episode"][e]
            first[key] = k
    # dist / value / next state against the restatement, from the recorded observation and the state used
    flat = lambda a: a.reshape((n * E,) + a.shape[2:])           # noqa: E731
    rd, rv, rs = ref.forward(x["w"], flat(x["in_obs"]), flat(h["actor"]), flat(used))
    _within_bound(flat(h["dist"]), flat(x["td"]), rd)
    _within_bound(flat(h["value"]), flat(x["tv"]), rv)
    _within_bound(flat(x["after_row"]), flat(x["ts"]), rs)
    assert np.isfinite(h["dist"]).all() and np.isfinite(x["policy_state"]).all()
    # greedy actions, bit for bit
    comm = _is_comm(variant, h["actor"])
    if greedy:
        assert np.array_equal(h["actions"][~comm], h["dist"][..., 0][~comm]), "greedy Gaussian action = the mean"
        assert np.array_equal(h["actions"][comm], h["dist"][comm].argmax(-1).astype(np.float32)), "greedy message = first argmax"


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_sampled_actions_against_the_host_mirrors(variant, masked):
    x = _run(variant, False, masked)
    h = x["h"]
    P = 4 if variant == SEQ else 12
    t = x["round"] * P + x["phase"] - 1
    envs = BASE + np.broadcast_to(np.arange(x["E"]), t.shape)
    d1, d2 = prng.ws_policy_draws(SEED, envs, x["episode"], t, h["actor"])
    u, u1, u2 = prng.ws_uniforms(d1, d2)
    comm = _is_comm(variant, h["actor"])
    if comm.any():
        lg, got = h["dist"][comm], h["actions"][comm]
        act, logp = sample_host(lg, u[comm])
        diff = act.astype(np.float32) != got
        if diff.any():
            assert np.all(cdf_margin(lg, u[comm])[diff] < 1e-5), "a message differs away from a CDF boundary"
        assert diff.sum() <= max(2, 1e-4 * got.size), diff.sum()
        assert np.abs(logp[~diff] - h["logp"][comm][~diff]).max() <= 1e-5
        assert len(set(got.tolist())) == 5 and set(got.tolist()) <= {0.0, 1.0, 2.0, 3.0, 4.0}
    else:
        assert variant == SEQ
    g = ~comm
    mean, log_std = h["dist"][..., 0][g], h["dist"][..., 1][g]
    a32, lp32, _ = sample_gaussian_host(mean, log_std, u1[g], u2[g])
    a64, lp64, _ = sample_gaussian_host(mean, log_std, u1[g], u2[g], dtype=np.float64)
    for name, got, m32, m64 in (("action", h["actions"][g], a32, a64), ("logp", h["logp"][g], lp32, lp64)):
        ek, eh = np.abs(got.astype(np.float64) - m64).max(), np.abs(m32.astype(np.float64) - m64).max()
        print("%s: device max error %.3e, float32 host mirror max error %.3e" % (name, ek, eh))
        assert ek <= 4 * eh + 1e-6, (name, ek, eh)
    assert np.std(h["actions"][g] - mean) > 1e-2, "the actions are sampled"


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_env_side_against_a_second_engine_and_the_mirror(variant, masked):
    x = _run(variant, False, masked)
    h, n, E, st0 = x["h"], x["n"], x["E"], x["st0"]
    clipped = _clip(variant, h["actor"], h["actions"])
    assert (clipped != h["actions"]).any(), "some sampled action lies outside [0, 1]"
    eng, _, _ = _fresh(variant, E)
    s2 = eng.get_state()
    for key in st0:
        assert np.array_equal(s2[key], st0[key]), key
    r = _rings(E, n, 64, 4)
    acts = torch.from_numpy(clipped).to(DEV)
    segs = [(0, n)] if not masked else [(0, x["k_reset"]), (x["k_reset"], n)]
    for lo, hi in segs:
        if lo:
            eng.reset(torch.from_numpy(x["mask"]).to(DEV))
        eng.rollout_actions(acts, hi - lo, obs=r["obs"], agent=r["agent"], rew=r["rew"], done=r["done"], step0=lo, auto_reset=True)
    g = _host(r)
    for key in ("obs", "agent", "rew", "done"):
        assert np.array_equal(g[key], h[key]), key
    fin = eng.get_state()
    for key in fin:
        assert np.array_equal(fin[key], x["final"][key]), key
    assert eng.status() == 0 and x["status"] == 0
    eng.close()
    m = WatershedMirror(variant, E, seed=SEED, env_index_base=BASE)
    m.season, m.p, m.rnd = st0["season"].astype(np.int64), st0["phase"].astype(np.int64), st0["round"].astype(np.int64)
    m.episode, m.hist, m.fr, m.pen = st0["episode"].astype(np.int64), st0["hist"].copy(), st0["f_rew"].copy(), st0["pen"].copy()
    m.wrapped, m.viol, m.csum = st0["wrapped"].astype(bool), st0["viol"].copy(), st0["current_sums"].copy()
    m.run, m.prev = st0["running_rew"].copy(), st0["prev_actions"].copy()
    for k in range(n):
        if masked and k == x["k_reset"]:
            m.reset(x["mask"])
        obs, agent, rew, done = m.step(clipped[k], auto_reset=True)
        assert np.array_equal(obs, h["obs"][k]) and np.array_equal(agent, h["agent"][k]), k
        assert np.array_equal(rew, h["rew"][k]) and np.array_equal(done, h["done"][k]), k
    assert m.status == 0


# ---------------------------------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("greedy", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_split_and_ring_length_do_not_matter(variant, greedy):
    E, Cs, n = 96, 128, 50
    pol, _ = _policy(variant, Cs, pseed=5)
    S = pol.num_sets

    def run(chunks, R):
        eng, obs, agent = _fresh(variant, E)
        state = _init_state(E, S, Cs, seed=2)
        r = _rings(E, R, Cs, S)
        k = 0
        for c in chunks:
            _roll(eng, pol, obs, agent, c, r, state, step0=k, greedy=greedy)
            k += c
            obs, agent = r["obs"][(k - 1) % R], r["agent"][(k - 1) % R]
        out = _host(r)
        out["state"] = state.cpu().numpy()
        out["env"] = eng.get_state()
        # last_value is the forward on the final observation under the observer's row, after the start rule
        before = state.clone()
        s = out["env"]
        starts = torch.from_numpy(ref.start_rule(variant, s["round"], s["phase"])).to(DEV)
        rows = state[torch.arange(E, device=DEV), agent.long()].contiguous()
        _, v, _ = eng.policy_forward(pol, obs.contiguous(), agent.contiguous(), rows, starts)
        torch.cuda.synchronize()
        assert np.array_equal(v.cpu().numpy(), out["last_value"]) and torch.equal(before, state)
        eng.close()
        return out

    whole = run([n], n)
    assert np.isfinite(whole["last_value"]).all() and np.ptp(whole["last_value"]) > 0
    for chunks, R in (([1, n - 1], n), ([7] * 7 + [1], n), ([n], 1), ([n], 3), ([7] * 7 + [1], 3), ([1, n - 1], 1)):
        got = run(chunks, R)
        for key in RING_KEYS:
            for j in range(max(0, n - R), n):
                assert np.array_equal(got[key][j % R], whole[key][j]), (key, j, chunks, R)
        assert np.array_equal(got["state"], whole["state"]) and np.array_equal(got["last_value"], whole["last_value"])
        for key in whole["env"]:
            assert np.array_equal(got["env"][key], whole["env"][key]), key


# ---------------------------------------------------------------------------------------------------- 7. BPTT path
@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_sequence_reproduces_one_agents_rows(variant):
    x = _run(variant, False, False)
    h, pol, w = x["h"], x["pol"], x["w"]
    a = pol.num_sets - 1
    ks = [k for k in range(x["n"]) if h["actor"][k, 0] == a]
    assert len(ks) >= 10 and (h["actor"][ks] == a).all()
    obs_seq = x["in_obs"][ks]
    resets = ref.start_rule(variant, x["round"][ks], x["phase"][ks])
    assert resets.any() and not resets.all()
    state_in = h["state_ring"][ks[0]]
    with torch.no_grad():
        td, tv, _ = pol.forward_sequence(a, torch.from_numpy(obs_seq).to(DEV), torch.from_numpy(state_in).to(DEV),
                                         torch.from_numpy(resets).to(DEV))
    st = state_in.astype(np.float64)
    rd, rv = [], []
    agent = np.full(x["E"], a)
    for t in range(len(ks)):
        d, v, st = ref.forward(w, obs_seq[t], agent, st, resets[t])
        rd.append(d)
        rv.append(v)
    _within_bound(h["dist"][ks], td.cpu().numpy(), np.stack(rd))
    _within_bound(h["value"][ks], tv.cpu().numpy(), np.stack(rv))


# ---------------------------------------------------------------------------------------------------- 8. rejections
def test_bad_arguments_are_rejected_and_change_nothing():
    variant, E, Cs, n = SEQ_COMM, 64, 128, 20
    pol, _ = _policy(variant, Cs, pseed=8)
    S = pol.num_sets

    def setup():
        eng, obs, agent = _fresh(variant, E)
        return eng, obs, agent, _init_state(E, S, Cs, seed=4), _rings(E, n, Cs, S)

    eng, obs, agent, state, r = setup()
    _roll(eng, pol, obs, agent, n, r, state)
    want = _host(r)
    want_state = state.cpu().numpy()
    eng.close()

    eng, obs, agent, state, r = setup()
    L, vp = _capi.lib(), C.c_void_p
    stream = vp(torch.cuda.current_stream(DEV).cuda_stream)
    p = lambda t: None if t is None else vp(t.data_ptr())     # noqa: E731
    scratch = torch.zeros(E, device=DEV)

    def raw(weights=pol.packed(), num_sets=S, cells=Cs, obs_in=obs, agent_in=agent, steps=n, step0=0, st=state, ring=n, flags=0, **kw):
        g = dict(r)
        g.update(kw)
        return L.ssd_ws_rollout_policy(eng._h, p(weights), num_sets, cells, p(obs_in), p(agent_in), steps, step0, p(st), p(g["state_ring"]),
                                       p(scratch), p(g["obs"]), p(g["agent"]), p(g["rew"]), p(g["done"]), p(g["actor"]), p(g["actions"]),
                                       p(g["logp"]), p(g["value"]), p(g["dist"]), ring, p(g["last_value"]), flags, stream)

    bad = [dict(num_sets=4), dict(num_sets=1), dict(cells=100), dict(obs=None), dict(agent=None), dict(actions=None), dict(steps=0),
           dict(step0=-1), dict(ring=0), dict(flags=1), dict(weights=None), dict(st=None), dict(obs_in=None), dict(agent_in=None)]
    for kw in bad:
        assert raw(**kw) == _capi.SSD_E_INVALID, kw
        assert L.ssd_ws_last_error(eng._h)
    mis = torch.zeros(n * E * 12 + 1, device=DEV)[1:].view(n, E, 12)         # rows not 16-byte aligned
    assert raw(obs=mis) == _capi.SSD_E_INVALID
    assert L.ssd_ws_policy_forward(p(pol.packed()), 4, Cs, variant, p(obs), p(agent), p(state), None, E, None, None, None, 0, 0,
                                   stream) == _capi.SSD_E_INVALID
    assert L.ssd_ws_policy_forward(p(pol.packed()), S, 100, variant, p(obs), p(agent), p(state), None, E, None, None, None, 0, 0,
                                   stream) == _capi.SSD_E_INVALID
    assert b"cell_size" in L.ssd_policy_last_error()
    # the Python layer: shapes, dtypes, the policy's variant
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=DEV)   # noqa: E731
    for kw in (dict(actions=z((n, E + 1))), dict(dist=z((n, E, 4))), dict(logp=z((n + 1, E))), dict(state_ring=z((n, E, 2, 64))),
               dict(actor=z((n, E), torch.int32)), dict(actions=None), dict(value=z((n, E), torch.float64))):
        g = dict(r)
        g.update(kw)
        with pytest.raises(ValueError):
            eng.rollout_policy(pol, obs, agent, n, g["obs"], g["agent"], actions=g["actions"], logp=g["logp"], value=g["value"],
                               dist=g["dist"], actor=g["actor"], state=state, state_ring=g["state_ring"])
    for a_in, o_in, st in ((agent.to(torch.int32), obs, state), (agent, obs[:, :8], state), (agent, obs, state[:, :4]), (agent, obs, None)):
        with pytest.raises(ValueError):
            eng.rollout_policy(pol, o_in, a_in, n, r["obs"], r["agent"], actions=r["actions"], state=st)
    with pytest.raises(ValueError):
        eng.rollout_policy(_policy(SEQ, Cs)[0], obs, agent, n, r["obs"], r["agent"], actions=r["actions"], state=state)
    with pytest.raises(ValueError):
        eng.rollout_policy(pol, obs, agent, n, r["obs"][0], r["agent"], actions=r["actions"], state=state)
    # ... and none of it touched the engine or the state: the rollout gives the bits it would have given
    _roll(eng, pol, obs, agent, n, r, state)
    got = _host(r)
    for key in want:
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(state.cpu().numpy(), want_state)
    eng.close()


# ---------------------------------------------------------------------------------------------------- 9. sample()
@pytest.mark.parametrize("variant", VARIANTS)
def test_sample_twice_equals_once(variant):
    E, K = 80, 37
    pol, _ = _policy(variant, 128, pseed=6)
    a = WatershedVecEngine(variant, E, seed=SEED)
    b = WatershedVecEngine(variant, E, seed=SEED)
    a.reset()
    b.reset()
    one = a.sample(pol, 2 * K)
    x, y = b.sample(pol, K), b.sample(pol, K)
    torch.cuda.synchronize()
    assert set(one) == {"obs", "agent", "actor", "actions", "logp", "value", "dist", "rew", "done", "state_in", "last_value"}
    for key in one:
        if key == "last_value":
            assert torch.equal(one[key], y[key])
        else:
            assert tuple(one[key].shape[:2]) == (2 * K, E)
            assert torch.equal(one[key], torch.cat([x[key], y[key]])), key
    assert not one["state_in"][0].any() and one["state_in"][2 * K - 1].any()
    sa, sb = a.get_state(), b.get_state()
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    # an optimiser step shows in the next rollout
    with torch.no_grad():
        pol.out_b.add_(0.5)
    z = a.sample(pol, 3)
    w = b.sample(pol, 3, greedy=True)
    torch.cuda.synchronize()
    assert torch.isfinite(z["dist"]).all() and not torch.equal(z["actions"], w["actions"])
    assert a.status() == 0 and b.status() == 0


def test_a_never_reset_env_is_left_alone():
    E, Cs, n = 40, 64, 5
    pol, _ = _policy(SEQ, Cs, pseed=1)
    eng = WatershedVecEngine(SEQ, E, seed=1)
    mask = torch.arange(E, device=DEV) % 2 == 0
    obs, agent = eng.reset(mask)
    state = _init_state(E, 4, Cs)
    s0 = state.clone()
    r = _rings(E, n, Cs, 4)
    for t in r.values():
        t.fill_(1)
    _roll(eng, pol, obs, agent, n, r, state)
    h = _host(r)
    dead = ~mask.cpu().numpy()
    for key in RING_KEYS + ("last_value",):
        v = h[key][:, dead] if key != "last_value" else h[key][dead]
        assert not v.any(), key
        assert (h[key][:, ~dead] if key != "last_value" else h[key][~dead]).any(), key
    assert torch.equal(state[~mask], s0[~mask]) and not torch.equal(state[mask], s0[mask])
    assert eng.status() == _capi.SSD_ST_NOT_RESET
    assert (eng.get_state()["phase"][dead] == 0).all()
