"""The recurrent policy module (policy.ConvLSTMPolicy) against the float64 restatement (policy_lstm_ref.py): one step and
sequences with resets, the cell's gate order and forget bias by hand-built weights, the start rule, the BPTT path, and the packed
weight layout against include/ssd.h.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

from policy_lstm_ref import forward as ref_forward, random_weights
from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd.policy import ConvFCPolicy, ConvLSTMPolicy

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssd.h")


def _policy(P, A, C, seed):
    w = random_weights(np.random.default_rng(seed), P, A, C)
    return ConvLSTMPolicy(A, P, C).double().load_arrays(w), w


def _inputs(rng, lead, N, C):
    obs = rng.integers(0, 256, size=lead + (N, 15, 15, 3), dtype=np.uint8)
    state = rng.standard_normal(lead + (N, 2, C))
    starts = rng.random(lead + (N,)) < 0.3
    return obs, state, starts


@pytest.mark.parametrize("C", [64, 128, 256])
@pytest.mark.parametrize("P,N,A", [(1, 5, 8), (5, 5, 9)])
def test_one_step_equals_restatement(P, N, A, C):
    pol, w = _policy(P, A, C, 3 + P + C)
    obs, state, starts = _inputs(np.random.default_rng(C + P), (4,), N, C)
    for st in (None, starts):
        lg, v, ns = pol(torch.from_numpy(obs), torch.from_numpy(state), None if st is None else torch.from_numpy(st))
        rl, rv, rs = ref_forward(w, obs, state, st)
        assert lg.shape == (4, N, A) and v.shape == (4, N) and ns.shape == (4, N, 2, C)
        assert np.abs(lg.detach().numpy() - rl).max() <= 1e-12
        assert np.abs(v.detach().numpy() - rv).max() <= 1e-12
        assert np.abs(ns.detach().numpy() - rs).max() <= 1e-12
    assert np.ptp(rl) > 1e-2 and np.ptp(rs[..., 1, :]) > 1e-2


@pytest.mark.parametrize("C", [64, 128, 256])
@pytest.mark.parametrize("P", [1, 3])
def test_sequence_with_resets_equals_restatement(P, C):
    N, A, T = 3, 8, 5
    pol, w = _policy(P, A, C, 40 + P)
    rng = np.random.default_rng(C)
    obs = rng.integers(0, 256, size=(T, 2, N, 15, 15, 3), dtype=np.uint8)
    state = rng.standard_normal((2, N, 2, C))
    resets = rng.random((T, 2, N)) < 0.25
    lg, v, final = pol.forward_sequence(torch.from_numpy(obs), torch.from_numpy(state), torch.from_numpy(resets))
    st = state
    for t in range(T):
        rl, rv, st = ref_forward(w, obs[t], st, resets[t])
        assert np.abs(lg[t].detach().numpy() - rl).max() <= 1e-12
        assert np.abs(v[t].detach().numpy() - rv).max() <= 1e-12
    assert np.abs(final.detach().numpy() - st).max() <= 1e-12


@pytest.mark.parametrize("gate", ["i", "j", "f", "o"])
def test_hand_built_gates(gate):
    """Only one gate block of lstm_w / lstm_b is non-zero: the others see z = 0, so the closed forms below pin the (i, j, f, o)
    order and the +1 forget bias."""
    C, A = 64, 8
    rng = np.random.default_rng(5)
    w = random_weights(rng, 1, A, C)
    g = "ijfo".index(gate)
    keep = np.zeros(4 * C, bool)
    keep[g * C:(g + 1) * C] = True
    w["lstm_w"][..., ~keep] = 0.0
    w["lstm_b"][..., ~keep] = 0.0
    pol = ConvLSTMPolicy(A, 1, C).double().load_arrays(w)
    obs, state, _ = _inputs(rng, (), 4, C)
    _, _, ns = pol(torch.from_numpy(obs), torch.from_numpy(state))
    c2, h2 = ns.detach().numpy()[:, 0], ns.detach().numpy()[:, 1]
    x = torch.from_numpy(obs)
    from sequential_social_dilemma_games_amd.policy import _trunk
    feat = _trunk(pol, x)[0][:, 0].detach().numpy()
    z = np.concatenate([feat, state[:, 1]], -1) @ w["lstm_w"][0][:, g * C:(g + 1) * C] + w["lstm_b"][0][g * C:(g + 1) * C]
    assert np.ptp(z) > 0.1
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))                               # noqa: E731
    c = state[:, 0]
    want_c = {"i": sig(1.0) * c + sig(z) * 0.0,                            # tanh(j = 0) = 0: the input adds nothing
              "j": sig(1.0) * c + 0.5 * np.tanh(z),
              "f": sig(z + 1.0) * c,
              "o": sig(1.0) * c}[gate]
    want_h = (sig(z) if gate == "o" else 0.5) * np.tanh(want_c)
    assert np.abs(c2 - want_c).max() <= 1e-12
    assert np.abs(h2 - want_h).max() <= 1e-12


def test_start_rule_selects_zero_and_ignores_nan():
    pol, w = _policy(5, 8, 128, 9)
    obs, state, starts = _inputs(np.random.default_rng(1), (3,), 5, 128)
    starts[0, 0] = True
    poisoned = state.copy()
    poisoned[starts] = np.nan
    zeroed = state.copy()
    zeroed[starts] = 0.0
    a = pol(torch.from_numpy(obs), torch.from_numpy(poisoned), torch.from_numpy(starts))
    b = pol(torch.from_numpy(obs), torch.from_numpy(zeroed), None)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_forward_sequence_equals_stepwise_forward_and_backpropagates():
    pol = ConvLSTMPolicy(9, 2, 64, seed=4)
    rng = np.random.default_rng(2)
    T = 6
    obs = torch.from_numpy(rng.integers(0, 256, size=(T, 3, 2, 15, 15, 3), dtype=np.uint8))
    state = torch.from_numpy(rng.standard_normal((3, 2, 2, 64)).astype(np.float32))
    resets = torch.from_numpy(rng.random((T, 3, 2)) < 0.3)
    lg, v, final = pol.forward_sequence(obs, state, resets)
    st = state
    for t in range(T):
        st = torch.where(resets[t][..., None, None], torch.zeros_like(st), st)
        l1, v1, st = pol(obs[t], st)
        assert torch.equal(l1, lg[t]) and torch.equal(v1, v[t])
    assert torch.equal(final, st)
    (lg.square().sum() + v.sum()).backward()
    for name in ("lstm_w", "lstm_b", "fc1_w", "conv_w", "logits_w", "value_b"):
        assert getattr(pol, name).grad is not None and torch.isfinite(getattr(pol, name).grad).all(), name
    assert pol.lstm_w.grad.abs().sum() > 0


def test_initialisers_and_shapes():
    for C in (64, 128, 256):
        pol = ConvLSTMPolicy(8, 3, C, seed=1)
        assert pol.lstm_w.shape == (3, 32 + C, 4 * C) and pol.lstm_b.shape == (3, 4 * C)
        assert pol.logits_w.shape == (3, C, 8) and pol.value_w.shape == (3, C, 1)
        limit = np.sqrt(6.0 / (32 + C + 4 * C))
        assert pol.lstm_w.abs().max() <= limit and pol.lstm_w.abs().max() > 0.9 * limit
        for name, std in (("fc1_w", 1.0), ("fc2_w", 1.0), ("value_w", 1.0), ("logits_w", 0.01)):
            norms = getattr(pol, name).detach().double().square().sum(dim=-2).sqrt().numpy()
            assert np.allclose(norms, std, rtol=1e-6), name
        for name in ("conv_b", "fc1_b", "fc2_b", "lstm_b", "logits_b", "value_b"):
            assert torch.all(getattr(pol, name) == 0), name
        assert pol.initial_state((4, 3)).shape == (4, 3, 2, C) and not pol.initial_state(2).any()
    for bad in ({"cell_size": 32}, {"num_sets": 0}, {"num_actions": 16}):
        kw = dict(num_actions=8, num_sets=1, cell_size=128)
        kw.update(bad)
        with pytest.raises(ValueError):
            ConvLSTMPolicy(**kw)
    pol = ConvLSTMPolicy(8, 1, 64)
    obs = torch.zeros((2, 15, 15, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        pol(obs, torch.zeros((2, 2, 128)))
    with pytest.raises(ValueError):
        pol(obs, torch.zeros((2, 2, 64)), torch.zeros(3, dtype=torch.bool))


def test_trunk_is_shared_with_the_feed_forward_policy():
    """Both modules run the same trunk code: with the trunk's weights copied over, fc2's output agrees bit for bit."""
    from sequential_social_dilemma_games_amd.policy import _trunk
    ff = ConvFCPolicy(8, 2, seed=3)
    rec = ConvLSTMPolicy(8, 2, 64, seed=4)
    with torch.no_grad():
        for name in ("conv_w", "conv_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b"):
            getattr(rec, name).copy_(getattr(ff, name))
    obs = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(3, 2, 15, 15, 3), dtype=np.uint8))
    assert torch.equal(_trunk(ff, obs)[0], _trunk(rec, obs)[0])


def _header():
    text = open(HEADER).read()
    vals = {k: int(v) for k, v in re.findall(r"\b(SSD_LSTM_[A-Z0-9_]+)\s*=\s*([0-9]+)", text)}
    macros = re.findall(r"#define (SSD_LSTM_\w+)\(([A-Za-z, ]+)\) (.+)", text)
    ns = dict(vals)
    for name, params, body in macros:
        args = [p.strip() for p in params.split(",")]
        expr = body.replace("/", "//")
        ns[name] = (lambda args, expr: lambda *v: eval(expr, ns, dict(zip(args, v))))(args, expr)
    return vals, ns, [m[0] for m in macros]


def test_python_layout_constants_equal_the_header():
    vals, ns, names = _header()
    assert set(vals) == {"SSD_LSTM_W", "SSD_LSTM_X", "SSD_LSTM_MAX_CELLS"}
    for k, v in vals.items():
        assert getattr(_capi, k) == v, k
    assert _capi.SSD_LSTM_W == (_capi.SSD_POL_FC2_B + 32 + 63) // 64 * 64
    assert set(names) == {"SSD_LSTM_ALIGN", "SSD_LSTM_B", "SSD_LSTM_VALUE_W", "SSD_LSTM_VALUE_B", "SSD_LSTM_LOGITS_W",
                          "SSD_LSTM_LOGITS_B", "SSD_LSTM_SET_FLOATS"}
    for C in (64, 128, 256):
        for name in ("SSD_LSTM_B", "SSD_LSTM_VALUE_W", "SSD_LSTM_VALUE_B", "SSD_LSTM_LOGITS_W"):
            assert ns[name](C) == getattr(_capi, name)(C) and ns[name](C) % 64 == 0, (name, C)
        for A in range(1, 16):
            for name in ("SSD_LSTM_LOGITS_B", "SSD_LSTM_SET_FLOATS"):
                assert ns[name](C, A) == getattr(_capi, name)(C, A) and ns[name](C, A) % 64 == 0, (name, C, A)
    for sym in ("ssd_policy_lstm_forward", "ssd_rollout_policy_lstm"):
        assert sym in _capi.SYMBOLS and sym in _capi.LSTM_SYMBOLS
    assert _capi.LSTM_CELL_SIZES == (64, 128, 256)


@pytest.mark.parametrize("P,C,A", [(1, 128, 8), (5, 64, 9), (5, 256, 8), (2, 128, 15)])
def test_packed_unpacks_by_the_header_offsets(P, C, A):
    pol = ConvLSTMPolicy(A, P, C, seed=2)
    with torch.no_grad():
        for p in pol.parameters():
            p.normal_()
    buf = pol.packed()
    assert buf.dtype == torch.float32 and buf.is_contiguous() and buf.numel() == P * _capi.SSD_LSTM_SET_FLOATS(C, A)
    v = buf.view(P, -1).numpy()
    K = _capi
    spans = {"conv_w": (K.SSD_POL_CONV_W, (3, 3, 3, 6)), "conv_b": (K.SSD_POL_CONV_B, (6,)), "fc1_w": (K.SSD_POL_FC1_W, (1014, 32)),
             "fc1_b": (K.SSD_POL_FC1_B, (32,)), "fc2_w": (K.SSD_POL_FC2_W, (32, 32)), "fc2_b": (K.SSD_POL_FC2_B, (32,)),
             "lstm_w": (K.SSD_LSTM_W, (32 + C, 4 * C)), "lstm_b": (K.SSD_LSTM_B(C), (4 * C,)),
             "value_w": (K.SSD_LSTM_VALUE_W(C), (C, 1)), "value_b": (K.SSD_LSTM_VALUE_B(C), (1,)),
             "logits_w": (K.SSD_LSTM_LOGITS_W(C), (C, A)), "logits_b": (K.SSD_LSTM_LOGITS_B(C, A), (A,))}
    covered = np.zeros(v.shape[1], bool)
    for name, (off, shape) in spans.items():
        n = int(np.prod(shape))
        assert off % 64 == 0 or name in ("conv_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b"), name
        assert np.array_equal(v[:, off:off + n].reshape((P,) + shape), getattr(pol, name).detach().numpy()), name
        assert not covered[off:off + n].any()
        covered[off:off + n] = True
    assert np.all(v[:, ~covered] == 0)
    with torch.no_grad():
        pol.lstm_b[0, 3] = 123.0
    assert pol.packed().view(P, -1)[0, K.SSD_LSTM_B(C) + 3].item() == 123.0
