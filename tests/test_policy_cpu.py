"""The conv-FC policy module (policy.py) against the float64 restatement of models/conv_to_fc_net.py (policy_ref.py), the packed
weight layout against include/ssd.h, and the host mirror of the rollout's action selection.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

from policy_ref import forward as ref_forward, random_weights
from sequential_social_dilemma_games_amd import _capi, prng
from sequential_social_dilemma_games_amd.policy import ConvFCPolicy, cdf_margin, sample_host

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssd.h")


def _policy(P, A, seed):
    w = random_weights(np.random.default_rng(seed), P, A)
    return ConvFCPolicy(A, P).double().load_arrays(w), w


@pytest.mark.parametrize("P,N,A", [(1, 5, 8), (5, 5, 8), (1, 2, 9), (10, 10, 9)])
def test_module_equals_restatement(P, N, A):
    pol, w = _policy(P, A, 1 + P + N)
    obs = np.random.default_rng(7).integers(0, 256, size=(6, N, 15, 15, 3), dtype=np.uint8)
    lg, v = pol(torch.from_numpy(obs))
    rl, rv = ref_forward(w, obs)
    assert lg.shape == (6, N, A) and v.shape == (6, N)
    assert np.abs(lg.detach().numpy() - rl).max() <= 1e-12
    assert np.abs(v.detach().numpy() - rv).max() <= 1e-12
    # some ReLUs on and some off: the comparison means something
    assert np.ptp(rl) > 1e-3


def test_shared_set_takes_any_leading_shape():
    pol, w = _policy(1, 8, 3)
    obs = np.random.default_rng(8).integers(0, 256, size=(4, 15, 15, 3), dtype=np.uint8)
    lg, v = pol(torch.from_numpy(obs))
    rl, rv = ref_forward(w, obs[:, None])
    assert np.abs(lg.detach().numpy() - rl[:, 0]).max() <= 1e-12 and np.abs(v.detach().numpy() - rv[:, 0]).max() <= 1e-12


@pytest.mark.parametrize("row,col,ch", [(0, 0, 0), (0, 0, 5), (0, 1, 0), (1, 0, 0), (6, 9, 3), (12, 12, 5)])
def test_flatten_order_is_row_col_channel(row, col, ch):
    # fc1 reads the single conv output (row, col, ch); fc2 and the logits pass it through: logit 0 is that conv output
    rng = np.random.default_rng(11)
    w = random_weights(rng, 1, 8)
    w["conv_b"][:] = 0.5                                           # positive: the ReLU passes most outputs
    w["fc1_w"][:] = 0.0
    w["fc1_w"][0, (row * 13 + col) * 6 + ch, 0] = 1.0
    w["fc1_b"][:] = 0.0
    w["fc2_w"][:] = 0.0
    w["fc2_w"][0, 0, 0] = 1.0
    w["fc2_b"][:] = 0.0
    w["logits_w"][:] = 0.0
    w["logits_w"][0, 0, 0] = 1.0
    w["logits_b"][:] = 0.0
    pol = ConvFCPolicy(8, 1).double().load_arrays(w)
    obs = rng.integers(0, 256, size=(3, 15, 15, 3), dtype=np.uint8)
    lg, _ = pol(torch.from_numpy(obs))
    x = (obs.astype(np.float64) - 128.0) / 255.0
    want = np.maximum(np.einsum("mhwc,hwc->m", x[:, row:row + 3, col:col + 3, :], w["conv_w"][0, :, :, :, ch]) + 0.5, 0.0)
    assert np.abs(lg.detach().numpy()[:, 0] - want).max() <= 1e-12
    assert np.all(lg.detach().numpy()[:, 1:] == 0.0)


def test_normc_column_norms():
    pol = ConvFCPolicy(9, 3, seed=5)
    for name, std in (("fc1_w", 1.0), ("fc2_w", 1.0), ("value_w", 1.0), ("logits_w", 0.01)):
        norms = getattr(pol, name).detach().double().square().sum(dim=-2).sqrt().numpy()
        assert np.allclose(norms, std, rtol=1e-6), name
    for name in ("conv_b", "fc1_b", "fc2_b", "logits_b", "value_b"):
        assert torch.all(getattr(pol, name) == 0), name
    assert not torch.equal(pol.fc1_w[0], pol.fc1_w[1])                 # independent sets


def _header_enum():
    text = open(HEADER).read()
    vals = {k: int(v) for k, v in re.findall(r"\b(SSD_POL_[A-Z0-9_]+|SSD_S_POLICY|SSD_POLICY_GREEDY)\s*=\s*([0-9]+)", text)}
    shift = re.search(r"SSD_POLICY_GREEDY\s*=\s*1u\s*<<\s*([0-9]+)", text)
    vals["SSD_POLICY_GREEDY"] = 1 << int(shift.group(1))
    macros = dict(re.findall(r"#define (SSD_POL_\w+)\(A\) (.+)", text))
    return vals, macros


def test_python_layout_constants_equal_the_header():
    vals, macros = _header_enum()
    for k, v in vals.items():
        assert getattr(_capi, k) == v, k
    assert prng.S_POLICY == vals["SSD_S_POLICY"] == 9
    assert _capi.ABI_VERSION == int(re.search(r"#define SSD_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == 6
    for A in range(1, 16):
        env = dict(vals, A=A)
        for name in ("SSD_POL_LOGITS_B", "SSD_POL_SET_FLOATS"):
            expr = macros[name].replace("/", "//")
            assert eval(expr, {}, env) == getattr(_capi, name)(A), (name, A)
        assert _capi.SSD_POL_SET_FLOATS(A) % 64 == 0
    for sym in ("ssd_policy_forward", "ssd_policy_last_error", "ssd_rollout_policy"):
        assert sym in _capi.SYMBOLS


@pytest.mark.parametrize("P,A", [(1, 8), (5, 9)])
def test_packed_unpacks_by_the_header_offsets(P, A):
    pol = ConvFCPolicy(A, P, seed=2)
    with torch.no_grad():
        for p in pol.parameters():
            p.normal_()
    buf = pol.packed()
    assert buf.dtype == torch.float32 and buf.is_contiguous() and buf.numel() == P * _capi.SSD_POL_SET_FLOATS(A)
    v = buf.view(P, -1).numpy()
    C = _capi
    spans = {"conv_w": (C.SSD_POL_CONV_W, (3, 3, 3, 6)), "conv_b": (C.SSD_POL_CONV_B, (6,)), "fc1_w": (C.SSD_POL_FC1_W, (1014, 32)),
             "fc1_b": (C.SSD_POL_FC1_B, (32,)), "fc2_w": (C.SSD_POL_FC2_W, (32, 32)), "fc2_b": (C.SSD_POL_FC2_B, (32,)),
             "value_w": (C.SSD_POL_VALUE_W, (32, 1)), "value_b": (C.SSD_POL_VALUE_B, (1,)),
             "logits_w": (C.SSD_POL_LOGITS_W, (32, A)), "logits_b": (C.SSD_POL_LOGITS_B(A), (A,))}
    covered = np.zeros(v.shape[1], bool)
    for name, (off, shape) in spans.items():
        n = int(np.prod(shape))
        assert np.array_equal(v[:, off:off + n].reshape((P,) + shape), getattr(pol, name).detach().numpy()), name
        assert not covered[off:off + n].any()
        covered[off:off + n] = True
    assert np.all(v[:, ~covered] == 0)                                  # padding
    # an update between calls shows in the next packed()
    with torch.no_grad():
        pol.fc2_b[0, 3] = 123.0
    assert pol.packed().view(P, -1)[0, C.SSD_POL_FC2_B + 3].item() == 123.0


def test_policy_stream_mirror():
    seed, envs, eps, t, N = 0x123456789, np.array([0, 1, 7, 4095, 70000]), np.array([0, 3, 0, 12, 1]), 17, 5
    u = prng.policy_uniforms(seed, envs, eps, t, N)
    for r, (e, ep) in enumerate(zip(envs, eps)):
        for i in range(N):
            d = prng.draw_full(seed, int(e), int(ep), t, prng.S_POLICY, i)
            assert u[r, i] == np.float32((d >> 8) / 16777216.0)
            assert 0.0 <= u[r, i] < 1.0
    # t and episode are per env too; the stream differs from the random-action stream
    u2 = prng.policy_uniforms(seed, envs, eps, np.full(5, t), N)
    assert np.array_equal(u, u2)
    assert prng.draw_full(seed, 0, 0, 0, prng.S_POLICY, 0) != prng.draw_full(seed, 0, 0, 0, prng.S_ACTION, 0)


def test_inverse_cdf_sampler_and_greedy_ties():
    lg = np.log(np.array([0.1, 0.2, 0.3, 0.4], np.float32))[None].repeat(6, 0)
    u = np.array([0.05, 0.15, 0.31, 0.59, 0.61, 0.999], np.float32)
    act, logp = sample_host(lg, u)
    assert act.tolist() == [0, 1, 2, 2, 3, 3]
    assert np.allclose(logp, np.log([0.1, 0.2, 0.3, 0.3, 0.4, 0.4]), atol=1e-6)
    # no cumulative sum exceeds u: the last action
    act, _ = sample_host(lg[:1], np.array([1.0], np.float32))
    assert act.tolist() == [3]
    # greedy: the first of equal maxima
    act, logp = sample_host(np.array([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0]], np.float32), None, greedy=True)
    assert act.tolist() == [1, 0]
    want = 3.0 - np.log(np.exp([1.0, 3.0, 3.0, 2.0]).sum())
    assert abs(logp[0] - want) < 1e-6 and abs(logp[1] - np.log(0.25)) < 1e-6
    # the boundary distance the GPU test uses to excuse host / device disagreements
    assert np.allclose(cdf_margin(lg[:2], np.array([0.1, 0.31], np.float32)), [0.0, 0.01], atol=1e-6)
