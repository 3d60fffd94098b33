"""The Watershed policy without a GPU: the torch module against the float64 restatement of include/ssd.h's contract
(policy_ws_ref.py), the Keras gate order by hand-built gates, the packed layout against the header's macros, the shared comm
layer, the normal deviate of the counter PRNG, the start rule against a walk of the env mirror, and the BPTT path."""
import os
import re

import numpy as np
import pytest
import torch

import policy_ws_ref as ref
from watershed_mirror import WatershedMirror
from sequential_social_dilemma_games_amd import _capi, prng
from sequential_social_dilemma_games_amd.policy import (WatershedLSTMPolicy, sample_gaussian_host, ws_is_comm, ws_policy_start,
                                                        ws_policy_t)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ, SEQ_COMM = _capi.SSD_WS_SEQ, _capi.SSD_WS_SEQ_COMM


def _module(variant, C, local_obs=False, share=False, seed=0):
    w = ref.random_weights(np.random.default_rng(seed), variant, C, share=share)
    return WatershedLSTMPolicy(variant, local_obs=local_obs, cell_size=C, share_comm_layer=share).load_arrays(w), w


# ---------------------------------------------------------------------------------------------------- 1. module == restatement
@pytest.mark.parametrize("C", [64, 128, 256])
@pytest.mark.parametrize("local_obs", [False, True])
@pytest.mark.parametrize("variant,share", [(SEQ, False), (SEQ_COMM, False), (SEQ_COMM, True)])
def test_module_against_restatement(variant, share, local_obs, C):
    rng = np.random.default_rng(C + variant)
    pol, w = _module(variant, C, local_obs, share, seed=C)
    pol = pol.double()
    S, B = pol.num_sets, 53
    agent = rng.integers(0, S, B)                               # ids mixed within the batch
    assert len(set(agent.tolist())) == S
    obs = ref.random_obs(rng, variant, local_obs, agent)
    state = rng.standard_normal((B, 2, C))
    starts = rng.random(B) < 0.3
    with torch.no_grad():
        d, v, s = pol(torch.from_numpy(obs), torch.from_numpy(agent), torch.from_numpy(state), torch.from_numpy(starts))
    rd, rv, rs = ref.forward(w, obs, agent, state, starts)
    for got, want in ((d, rd), (v, rv), (s, rs)):
        assert np.abs(got.numpy() - want).max() <= 1e-12
    assert np.ptp(rd) > 1e-2 and np.ptp(rv) > 1e-2 and np.ptp(rs[:, 0]) > 1e-2


# ---------------------------------------------------------------------------------------------------- 2. gate order
def test_hand_built_gates_pin_the_keras_cell():
    """One non-zero gate block at a time.  With z = 0 every sigmoid is 0.5 and tanh(g) = 0, so c' = 0.5 c (no forget bias: a
    TF LSTMCell's +1 would give sigmoid(1) c); a large bias in one block moves exactly what that gate controls."""
    C = 64
    pol = WatershedLSTMPolicy(SEQ, cell_size=C).double()
    with torch.no_grad():
        for p in pol.parameters():
            p.zero_()
        pol.out_w[:, :, 0] = 1.0 / C                             # dist[0] = mean of h'
        pol.value_w[:, :, 0] = 1.0 / C
    obs = torch.zeros((1, 12), dtype=torch.float64)
    agent = torch.zeros(1, dtype=torch.int64)
    h = torch.full((C,), 0.25, dtype=torch.float64)
    c = torch.full((C,), 0.8, dtype=torch.float64)

    def run(block=None, bias=0.0, state=None):
        with torch.no_grad():
            pol.lstm_bias.zero_()
            if block is not None:
                pol.lstm_bias[0, block * C:(block + 1) * C] = bias
            return pol(obs, agent, torch.stack([h, c])[None] if state is None else state)

    big = 30.0
    _, _, s = run()
    assert np.allclose(s[0, 1].numpy(), 0.5 * 0.8, atol=1e-15), "c' = sigmoid(0) c: no forget bias"
    assert np.allclose(s[0, 0].numpy(), 0.5 * np.tanh(0.4), atol=1e-15), "h' = sigmoid(0) tanh(c')"
    _, _, s = run(1, big)                                        # block 1 = f: the old cell passes whole
    assert np.allclose(s[0, 1].numpy(), 0.8, atol=1e-12)
    _, _, s = run(1, -big)                                       # ... or not at all
    assert np.allclose(s[0, 1].numpy(), 0.0, atol=1e-12)
    _, _, s = run(2, big)                                        # block 2 = the candidate: tanh -> 1, gated by i = 0.5
    assert np.allclose(s[0, 1].numpy(), 0.4 + 0.5, atol=1e-12)
    _, _, s = run(0, big)                                        # block 0 = i: opens on a zero candidate, nothing changes
    assert np.allclose(s[0, 1].numpy(), 0.4, atol=1e-12)
    d, v, s = run(3, big)                                        # block 3 = o: h' = tanh(c')
    assert np.allclose(s[0, 0].numpy(), np.tanh(0.4), atol=1e-12) and np.allclose(s[0, 1].numpy(), 0.4, atol=1e-12)
    assert abs(float(d[0, 0]) - np.tanh(0.4)) < 1e-12 and abs(float(v[0]) - np.tanh(0.4)) < 1e-12, "the heads read h'"
    # the (h, c) order of the state: the recurrent kernel reads index 0
    with torch.no_grad():
        pol.lstm_recurrent[0, :, 2 * C:3 * C] = torch.eye(C, dtype=torch.float64) * big
    swapped = torch.stack([torch.full((C,), 1.0, dtype=torch.float64), torch.full((C,), 0.3, dtype=torch.float64)])[None]
    _, _, s = run(state=swapped)                                 # h = 1 drives the candidate to 1; c = 0.3 (the other order: 1.0)
    assert np.allclose(s[0, 1].numpy(), 0.5 * 0.3 + 0.5, atol=1e-12)


# ---------------------------------------------------------------------------------------------------- 3. layout
def _header_macros():
    text = open(os.path.join(REPO, "include", "ssd.h")).read()
    env = {}
    m = re.search(r"enum \{ (SSD_WSP_X = [^}]+)\}", text)
    for item in m.group(1).split(","):
        k, v = item.split("=")
        env[k.strip()] = int(v)
    for name, args, body in re.findall(r"#define (SSD_WSP_[A-Z_0-9]+)\(([A-Za-z, ]+)\) (.+)", text):
        env[name] = eval("lambda %s: %s" % (args, body.replace("/", "//")), env)
    return env


@pytest.mark.parametrize("C", [64, 128, 256])
def test_packed_matches_the_header(C):
    H = _header_macros()
    for name in ("SSD_WSP_X", "SSD_WSP_OUT", "SSD_WSP_D0_W", "SSD_WSP_D0_B", "SSD_WSP_D1_W", "SSD_WSP_D1_B", "SSD_WSP_LSTM_W"):
        assert H[name] == getattr(_capi, name), name
    for name in ("SSD_WSP_LSTM_B", "SSD_WSP_OUT_W", "SSD_WSP_OUT_B", "SSD_WSP_VALUE_W", "SSD_WSP_VALUE_B", "SSD_WSP_SET_FLOATS"):
        assert H[name](C) == getattr(_capi, name)(C), name
    pol, w = _module(SEQ_COMM, C, seed=5)
    F = H["SSD_WSP_SET_FLOATS"](C)
    packed = pol.packed().numpy().reshape(8, F)
    lw = H["SSD_WSP_LSTM_W"]
    where = {"dense0_w": 0, "dense0_b": H["SSD_WSP_D0_B"], "dense1_w": H["SSD_WSP_D1_W"], "dense1_b": H["SSD_WSP_D1_B"],
             "lstm_kernel": lw, "lstm_recurrent": lw + 16 * 4 * C, "lstm_bias": H["SSD_WSP_LSTM_B"](C), "out_w": H["SSD_WSP_OUT_W"](C),
             "out_b": H["SSD_WSP_OUT_B"](C), "value_w": H["SSD_WSP_VALUE_W"](C), "value_b": H["SSD_WSP_VALUE_B"](C)}
    covered = np.zeros(F, bool)
    for name, off in where.items():
        n = w[name][0].size
        assert off % 64 == 0 or name == "lstm_recurrent"
        assert not covered[off:off + n].any(), name
        covered[off:off + n] = True
        for i in range(8):
            assert np.array_equal(packed[i, off:off + n], w[name][i].reshape(-1)), (name, i)
    assert not packed[:, ~covered].any(), "padding is zero"
    assert F % 64 == 0 and where["value_b"] + 1 <= F


def test_shared_comm_layer_is_one_parameter_in_both_sets():
    C = 64
    pol, w = _module(SEQ_COMM, C, share=True, seed=2)
    assert pol.dense1_w.shape[0] == 4 and pol.dense1_b.shape[0] == 4
    F, o, n = pol.set_floats, _capi.SSD_WSP_D1_W, 256
    p0 = pol.packed().numpy().reshape(8, F).copy()
    for k in range(4):
        assert np.array_equal(p0[k, o:o + n], p0[k + 4, o:o + n]) and np.array_equal(p0[k, o:o + n], w["dense1_w"][k].reshape(-1))
    # a gradient step driven by agent 6 alone moves dense1 of sets 2 AND 6, and of no other set
    rng = np.random.default_rng(0)
    agent = np.full(9, 6)
    obs = torch.from_numpy(ref.random_obs(rng, SEQ_COMM, False, agent))
    opt = torch.optim.SGD(pol.parameters(), lr=0.1)
    d, v, _ = pol(obs, torch.from_numpy(agent), pol.initial_state(9))
    (d.square().sum() + v.square().sum()).backward()
    opt.step()
    p1 = pol.packed().numpy().reshape(8, F)
    changed = [k for k in range(8) if not np.array_equal(p0[k, o:o + n], p1[k, o:o + n])]
    assert changed == [2, 6]
    assert np.array_equal(p1[2, o:o + n], p1[6, o:o + n])


def test_dense0_rows_beyond_the_observation_are_irrelevant():
    rng = np.random.default_rng(1)
    pol, w = _module(SEQ_COMM, 64, local_obs=True, seed=3)
    assert pol.obs_lens == (8, 8, 8, 8, 9, 9, 9, 9)
    agent = rng.integers(0, 8, 40)
    obs = torch.from_numpy(ref.random_obs(rng, SEQ_COMM, True, agent))
    st = torch.from_numpy(rng.standard_normal((40, 2, 64)).astype(np.float32))
    with torch.no_grad():
        a = pol(obs, torch.from_numpy(agent), st)
        for i, n in enumerate(pol.obs_lens):
            pol.dense0_w[i, n:] = 1e6
        b = pol(obs, torch.from_numpy(agent), st)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    fresh = WatershedLSTMPolicy(SEQ_COMM, local_obs=True, cell_size=64)
    for i, n in enumerate(fresh.obs_lens):
        assert not fresh.dense0_w[i, n:].any() and fresh.dense0_w[i, :n].abs().min() > 0


# ---------------------------------------------------------------------------------------------------- 4. the deviate
@pytest.mark.parametrize("seed", [0, 3, 12345678901])
def test_normal_deviate_statistics(seed):
    """2^16 envs x agents 4-7 x t 8-11 = 2^20 deviates: mean and variance within five standard errors of an N(0,1) sample, and
    no deviate beyond sqrt(-2 ln 2^-24) (u1 >= 2^-24)."""
    envs = np.arange(1 << 16)
    out, differ = [], True
    for i in range(4, 8):
        for t in range(8, 12):
            d1, d2 = prng.ws_policy_draws(seed, envs, 0, t, i)
            differ &= bool((d1 != d2).mean() > 0.999)
            _, u1, u2 = prng.ws_uniforms(d1, d2)
            assert u1.min() > 0.0 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
            a, _, _ = sample_gaussian_host(np.zeros(envs.shape, np.float32), np.zeros(envs.shape, np.float32), u1, u2)
            out.append(a)
    n = np.concatenate(out).astype(np.float64)
    M = n.size
    assert M == 1 << 20 and differ
    assert abs(n.mean()) <= 5 / np.sqrt(M), n.mean()
    assert abs(n.var() - 1.0) <= 5 * np.sqrt(2.0 / M), n.var()
    assert np.abs(n).max() <= np.sqrt(2 * 24 * np.log(2.0)) + 1e-6


def test_draws_match_the_scalar_chain_and_gaussian_rules():
    d1, d2 = prng.ws_policy_draws(12345678901, np.array([7, 8]), np.array([2, 0]), np.array([9, 0]), np.array([5, 1]))
    assert int(d1[0]) == prng.draw_full(12345678901, 7, 2, 9, prng.S_POLICY, 5)
    assert int(d2[0]) == prng.draw_full(12345678901, 7, 2, 9, prng.S_POLICY, 21)
    assert int(d1[1]) == prng.draw_full(12345678901, 8, 0, 0, prng.S_POLICY, 1) and d1[0] != d2[0]
    u, u1, u2 = prng.ws_uniforms(d1, d2)
    assert u[0] == np.float32((int(d1[0]) >> 8) * 2.0 ** -24) and u1[0] == np.float32(((int(d1[0]) >> 8) + 1) * 2.0 ** -24)
    # policy_uniforms (the categorical draw of the other policies) is the same u for index = agent
    assert u[0] == prng.policy_uniforms(12345678901, np.array([7]), 2, 9, 6)[0, 5]
    mean = np.array([0.3, -2.0, 5.0, np.nan], np.float32)
    ls = np.array([-1.0, 0.5, 0.0, 0.0], np.float32)
    a, lp, cl = sample_gaussian_host(mean, ls, None, None, greedy=True)
    assert np.array_equal(a[:3], mean[:3]) and np.isnan(a[3])
    assert np.array_equal(lp[:3], (np.float32(-0.0) - ls[:3]) - np.float32(0.9189385))
    assert np.array_equal(cl, np.array([0.3, 0.0, 1.0, 0.0], np.float32)), "clipped to [0, 1], NaN -> 0"
    a, lp, cl = sample_gaussian_host(mean[:3], ls[:3], np.array([0.2, 1.0, 2.0 ** -24], np.float32), np.array([0.1, 0.6, 0.0], np.float32))
    assert a[1] == mean[1] and abs(a[2] - (5.0 + np.sqrt(2 * 24 * np.log(2.0)))) < 1e-5        # u1 = 1 gives n = 0
    assert ((cl >= 0) & (cl <= 1)).all()
    a64, lp64, _ = sample_gaussian_host(mean[:3], ls[:3], np.array([0.2, 1.0, 2.0 ** -24], np.float32), np.array([0.1, 0.6, 0.0], np.float32),
                                        dtype=np.float64)
    assert a64.dtype == np.float64 and np.abs(a64 - a).max() < 1e-5 and np.abs(lp64 - lp).max() < 1e-4


# ---------------------------------------------------------------------------------------------------- 5. the start rule
@pytest.mark.parametrize("variant", [SEQ, SEQ_COMM])
def test_start_rule_fires_once_per_agent_and_episode(variant):
    """Walk the env mirror through two episodes (auto reset): by (round, phase) alone the rule marks exactly each agent's first
    action of each episode, and t counts the actions of the episode from 0."""
    m = WatershedMirror(variant, 3, seed=5)
    _, agent = m.reset()
    S = ref.num_sets(variant)
    steps = 2 * (43 if variant == SEQ else 131)
    seen = [set() for _ in range(3)]                             # agents that have acted this episode, per env
    count = np.zeros(3, np.int64)
    fired = np.zeros((3, S), np.int64)
    for k in range(steps):
        start = ws_policy_start(variant, m.rnd, m.p)
        assert np.array_equal(start, ref.start_rule(variant, m.rnd, m.p))
        assert np.array_equal(ws_policy_t(variant, m.rnd, m.p), count)
        for e in range(3):
            a = int(agent[e])
            assert bool(start[e]) == (a not in seen[e]), (k, e, a)
            seen[e].add(a)
            fired[e, a] += int(start[e])
        act = np.where(ws_is_comm(variant, agent), 2.0, 0.4).astype(np.float32)
        _, agent, _, done = m.step(act, auto_reset=True)
        count += 1
        for e in range(3):
            if done[e] & 2:
                assert len(seen[e]) == S
                seen[e] = set()
                count[e] = 0
    assert (fired == 2).all()


# ---------------------------------------------------------------------------------------------------- 6. BPTT
def test_forward_sequence_equals_steps_and_backpropagates():
    rng = np.random.default_rng(4)
    C, T, B, i = 64, 6, 5, 5
    pol, _ = _module(SEQ_COMM, C, seed=9)
    pol = pol.double()
    obs = torch.from_numpy(ref.random_obs(rng, SEQ_COMM, False, np.full((T, B), i))).double()
    state = torch.from_numpy(rng.standard_normal((B, 2, C)))
    resets = torch.from_numpy(rng.random((T, B)) < 0.3)
    d, v, final = pol.forward_sequence(i, obs, state, resets)
    st = state
    agent = torch.full((B,), i, dtype=torch.int64)
    for t in range(T):
        dd, vv, st = pol(obs[t], agent, st, resets[t])
        assert torch.allclose(dd, d[t], atol=1e-13, rtol=0) and torch.allclose(vv, v[t], atol=1e-13, rtol=0)
    assert torch.allclose(st, final, atol=1e-13, rtol=0)
    (d.square().sum() + v.sum()).backward()
    for name in ("dense0_w", "dense1_w", "lstm_kernel", "lstm_recurrent", "lstm_bias", "out_w", "value_w"):
        g = getattr(pol, name).grad
        assert g is not None and g[i].abs().sum() > 0, name
        others = [k for k in range(8) if k != i]
        assert not g[others].any(), name
    with pytest.raises(ValueError):
        pol.forward_sequence(8, obs, state)


def test_symbols_and_exports():
    import sequential_social_dilemma_games_amd as pkg
    assert pkg.WatershedLSTMPolicy is WatershedLSTMPolicy
    assert {"ssd_ws_policy_forward", "ssd_ws_rollout_policy"} <= set(_capi.SYMBOLS)
    with pytest.raises(ValueError):
        WatershedLSTMPolicy(SEQ, cell_size=100)
