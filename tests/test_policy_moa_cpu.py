"""The MOA policy without a GPU: ConvMOAPolicy against the float64 restatement (policy_moa_ref.py), hand-built gates that pin the
Keras cell (gate order i, f, c, o; no forget bias at run time; state (h, c)) apart from ConvLSTMPolicy's, the start rule, the
string order of the other agents, influence() and moa_loss() against NumPy transcriptions, and the weight layout."""
import re

import numpy as np
import pytest
import torch

import policy_moa_ref as ref
from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd.policy import ConvMOAPolicy, agent_order, influence, other_agents


def _policy(A, N, P, C, seed=0):
    w = ref.random_weights(np.random.default_rng(seed), P, A, N, C)
    return ConvMOAPolicy(A, N, P, C).load_arrays(w).double(), w


def _inputs(rng, B, N, A, C, p_start=0.3):
    return (rng.integers(0, 256, (B, N, 15, 15, 3), dtype=np.uint8), rng.integers(0, A, (B, N)).astype(np.int32),
            rng.standard_normal((B, N, 4, C)) * 0.5, rng.random((B, N)) < p_start)


@pytest.mark.parametrize("N,P,C", [(5, 5, 64), (2, 1, 64), (10, 1, 64)])
def test_module_against_restatement(N, P, C):
    rng = np.random.default_rng(N + P)
    pol, w = _policy(8, N, P, C, seed=N)
    obs, prev, st, starts = _inputs(rng, 3, N, 8, C)
    r = ref.forward(w, obs, prev, st, starts)
    with torch.no_grad():
        t = pol(torch.from_numpy(obs), torch.from_numpy(prev), torch.from_numpy(st), torch.from_numpy(starts))
    for a, b in zip(r, t):
        assert np.abs(a - b.numpy()).max() < 1e-5
    moa = t[2].numpy()
    own = np.where(starts, 0, prev)
    assert np.array_equal(moa, np.take_along_axis(t[3].numpy(), own[:, :, None, None, None], 2)[:, :, 0])


def test_sequence_with_resets_matches_step_by_step_restatement():
    N, A, C, T = 3, 8, 64, 4
    rng = np.random.default_rng(1)
    pol, w = _policy(A, N, N, C, seed=3)
    obs = rng.integers(0, 256, (T, 2, N, 15, 15, 3), dtype=np.uint8)
    prev = rng.integers(0, A, (T, 2, N)).astype(np.int32)
    resets = np.zeros((T, 2, N), bool)
    resets[2, 1] = True
    st = rng.standard_normal((2, N, 4, C)) * 0.5
    lg, v, moa, final = pol.forward_sequence(torch.from_numpy(obs), torch.from_numpy(prev), torch.from_numpy(st),
                                             torch.from_numpy(resets))
    s = st
    for t in range(T):
        rl, rv, rm, _, s = ref.forward(w, obs[t], prev[t], s, resets[t])
        assert np.abs(lg[t].detach().numpy() - rl).max() < 1e-5 and np.abs(moa[t].detach().numpy() - rm).max() < 1e-5
    assert np.abs(final.detach().numpy() - s).max() < 1e-5
    lg.sum().backward()                                          # differentiable
    assert pol.lstm_kernel.grad is not None


def _one_gate_cell(block, x, h, c):
    """The actions LSTM with 1 cell, the kernel and bias zero except one gate block where both are 1: returns (h', c')."""
    C = 64
    pol = ConvMOAPolicy(2, 2, 1, C)
    with torch.no_grad():
        for p in pol.parameters():
            p.zero_()
    k = torch.zeros((32, 4 * C), dtype=torch.float64)
    k[:, block * C] = 1.0
    rec = torch.zeros((C, 4 * C), dtype=torch.float64)
    b = torch.zeros(4 * C, dtype=torch.float64)
    b[block * C] = 1.0
    from sequential_social_dilemma_games_amd.policy import keras_lstm
    hh = torch.zeros(C, dtype=torch.float64)
    cc = torch.zeros(C, dtype=torch.float64)
    hh[0], cc[0] = h, c
    xx = torch.full((32,), x / 32.0, dtype=torch.float64)
    h2, c2 = keras_lstm(xx, hh, cc, k, rec, b)
    return h2[0].item(), c2[0].item()


def test_hand_built_gates_pin_the_keras_cell():
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))                     # noqa: E731
    x, h, c = 0.7, 0.3, 0.5
    z = x + 1.0
    # block 0 = i: c' = sig(0) c + sig(z) tanh(0) = c / 2
    # block 1 = f: c' = sig(z) c + sig(0) tanh(0)  (no +1: RLlib's cell would give sig(z + 1) c)
    # block 2 = c~: c' = sig(0) c + sig(0) tanh(z)
    # block 3 = o: c' = c / 2, h' = sig(z) tanh(c / 2)
    want = {0: 0.5 * c, 1: sig(z) * c, 2: 0.5 * c + 0.5 * np.tanh(z), 3: 0.5 * c}
    for block, cw in want.items():
        h2, c2 = _one_gate_cell(block, x, h, c)
        assert abs(c2 - cw) < 1e-12, block
        ho = sig(z) if block == 3 else 0.5
        assert abs(h2 - ho * np.tanh(c2)) < 1e-12, block
    # under ConvLSTMPolicy's conventions (i, j, f, o with f + 1) every case above comes out differently
    lstm_c = {0: sig(0 + 1) * c + sig(z) * np.tanh(0), 1: sig(1) * c + 0.5 * np.tanh(z), 2: sig(z + 1) * c, 3: sig(1) * c}
    for block in want:
        assert abs(lstm_c[block] - want[block]) > 1e-3, block


def test_state_is_h_then_c():
    pol, w = _policy(8, 2, 1, 64, seed=9)
    rng = np.random.default_rng(2)
    obs, prev, st, _ = _inputs(rng, 2, 2, 8, 64)
    with torch.no_grad():
        out = pol(torch.from_numpy(obs), torch.from_numpy(prev), torch.from_numpy(st))[4].numpy()
    # h = sig(o) tanh(c) in rows 0 and 2, so |h| < |tanh(c)| <= 1 and sign(h) = sign(c)
    for hr, cr in ((0, 1), (2, 3)):
        assert np.all(np.abs(out[..., hr, :]) <= np.abs(np.tanh(out[..., cr, :])) + 1e-12)
        assert np.all(np.sign(out[..., hr, :]) == np.sign(out[..., cr, :]))


def test_start_rule_ignores_poisoned_state_and_garbage_actions():
    N, A, C = 4, 8, 64
    pol, _ = _policy(A, N, 1, C, seed=4)
    rng = np.random.default_rng(3)
    obs, prev, st, _ = _inputs(rng, 4, N, A, C)
    starts = np.zeros((4, N), bool)
    starts[1:3] = True
    p_st, p_prev = st.copy(), prev.copy()
    p_st[starts] = np.nan
    p_prev[starts] = 999
    z_st = st.copy()
    z_st[starts] = 0.0
    z_prev = prev.copy()
    z_prev[starts] = 0
    with torch.no_grad():
        a = pol(torch.from_numpy(obs), torch.from_numpy(p_prev), torch.from_numpy(p_st), torch.from_numpy(starts))
        b = pol(torch.from_numpy(obs), torch.from_numpy(z_prev), torch.from_numpy(z_st))
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y)


def test_string_order_of_the_other_agents():
    assert agent_order(12) == [0, 1, 10, 11, 2, 3, 4, 5, 6, 7, 8, 9]
    o = other_agents(12)
    assert list(o[2]) == [0, 1, 10, 11, 3, 4, 5, 6, 7, 8, 9] and list(o[10]) == [0, 1, 11, 2, 3, 4, 5, 6, 7, 8, 9]
    for i in range(12):
        assert list(o[i]) == ref.others(12)[i] == [n for n in sorted(range(12), key=lambda n: "agent-%d" % n) if n != i]


def test_influence_matches_kl_div_of_the_discrete_marginal():
    rng = np.random.default_rng(5)
    R, N, A = 40, 4, 8
    logits = rng.standard_normal((R, A)) * 2
    cf = rng.standard_normal((R, A, N - 1, A)) * 2
    acts = rng.integers(0, A, R)
    got = influence(torch.from_numpy(logits), torch.from_numpy(cf), torch.from_numpy(acts), 10.0).numpy()
    want = ref.influence(logits, cf, acts, 10.0)
    assert np.abs(got - want).max() < 1e-5 and want.min() > 0
    # an own-action column of zeros: every counterfactual is the same, so p = q and the influence is 0
    same = np.broadcast_to(cf[:, :1], cf.shape).copy()
    z = influence(torch.from_numpy(logits).float(), torch.from_numpy(same).float(), torch.from_numpy(acts), 10.0).numpy()
    assert np.abs(z).max() <= 1e-6
    # scaled weights clip at exactly clip
    big = influence(torch.from_numpy(logits), torch.from_numpy(cf * 50), torch.from_numpy(acts), 0.25).numpy()
    assert np.all(big <= np.float32(0.25)) and np.any(big == np.float32(0.25))
    # a non-finite row gives 0, the others are untouched
    bad = cf.copy()
    bad[3, 0, 0, 0] = np.nan
    g2 = influence(torch.from_numpy(logits), torch.from_numpy(bad), torch.from_numpy(acts), 10.0).numpy()
    assert g2[3] == 0.0 and np.array_equal(np.delete(g2, 3), np.delete(got, 3))


def test_moa_loss_matches_restatement():
    rng = np.random.default_rng(6)
    N, A = 5, 8
    pol = ConvMOAPolicy(A, N, 1, 64)
    moa = rng.standard_normal((7, N, N - 1, A))
    acts = rng.integers(0, A, (7, N))
    got = pol.moa_loss(torch.from_numpy(moa), torch.from_numpy(acts), 0.5).item()
    assert abs(got - ref.moa_loss(moa, acts, 0.5)) < 1e-10


def test_header_constants_and_packed_layout():
    import os
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "ssd.h")).read()
    enum = re.search(r"enum \{ (SSD_MOA_FC = .*?) \};", hdr).group(1)
    for name, val in re.findall(r"(SSD_MOA_\w+) = (\d+)", enum):
        assert getattr(_capi, name) == int(val), name
    for sym in ("ssd_policy_moa_forward", "ssd_rollout_policy_moa"):
        assert sym in _capi.SYMBOLS and sym in hdr
    assert "#define SSD_MOA_SCRATCH_FLOATS(rows) (82 * (size_t)(rows))" in hdr
    assert _capi.ABI_VERSION == 6
    A, N, C, P = 9, 5, 128, 5
    pol, w = _policy(A, N, P, C, seed=8)
    pk = pol.float().packed().numpy().reshape(P, -1)
    S = _capi.SSD_MOA_SET_FLOATS(C, A, N)
    assert pk.shape == (P, S) and S % 64 == 0
    offs = {name: off for name, _, off in pol.layout()}
    for name, shape, off in pol.layout():
        if name.startswith(("lstm", "moa", "value", "logits", "pred", "a_fc1_w", "m_fc1_w")) and "recurrent" not in name:
            assert off % 64 == 0, name
        n = int(np.prod(shape))
        assert np.array_equal(pk[:, off:off + n], np.asarray(w[name], np.float32).reshape(P, n)), name
    mw = _capi.SSD_MOA_MW(C, A)
    assert offs["moa_kernel"] == mw and offs["moa_recurrent"] == mw + 48 * 4 * C
    assert np.all(pk[:, mw + (32 + N) * 4 * C:mw + 48 * 4 * C] == 0), "the MOA input's padding rows are zero"
    assert _capi.SSD_MOA_FC1_W(1) - _capi.SSD_MOA_FC1_W(0) == _capi.SSD_MOA_FC_STRIDE
    assert _capi.SSD_MOA_FC2_B(0) + 32 <= _capi.SSD_MOA_FC1_W(1)
    assert _capi.SSD_MOA_LSTM_W(C) >= _capi.SSD_MOA_FC2_B(1) + 32


def test_initialisers():
    pol = ConvMOAPolicy(8, 5, 5, 64, seed=1)
    C = 64
    for name in ("lstm_bias", "moa_bias"):
        b = getattr(pol, name).detach()
        assert torch.all(b[:, C:2 * C] == 1) and torch.all(b[:, :C] == 0) and torch.all(b[:, 2 * C:] == 0)
    r = pol.lstm_recurrent.detach().double()[0]
    assert torch.allclose(r @ r.T, torch.eye(C, dtype=torch.float64), atol=1e-5)      # orthogonal rows
    cols = pol.a_fc1_w.detach().double().square().sum(1).sqrt()
    assert torch.allclose(cols, torch.ones_like(cols), atol=1e-5)                     # normc(1.0)
    v = pol.value_w.detach().double().square().sum(1).sqrt()
    assert torch.allclose(v, torch.full_like(v, 0.01), atol=1e-7)                     # normc(0.01)
