"""ssd_policy_ppo_grad on the MI355X where a tolerance cannot look: every row counted exactly once (integer sums, bit equality),
the weight sets' isolation bit for bit, the contract's derivatives at the kinks on the kernel itself (rows that are clipped and
dead, the first-epoch tie), and the edges of the contract against float64 -- A = 1, 2 and 15, clip_param = vf_clip_param = 0,
saturated logits, and the kept scratch reused by a smaller call."""
import copy

import numpy as np
import pytest
import torch

from ppo_ref import (COUNTING_HYPER, HYPER, MARGIN, as_numpy_u32, autograd_loss, branch_report, clipped_fragment, clipped_rows,
                     counting_inputs, make_inputs, make_policy, saturate, set_fragment, set_policy, shifted_obs, zero_policy)
from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd.policy import PPO_STATS
from test_ppo_loss_gpu import DEV, _check_against_reference, _run, _to_dev, compare_with_float64

pytestmark = pytest.mark.gpu


def _device_run(pol, t, first, h):
    """A fresh device copy of (pol, t, first) through the kernel -> (loss, stats, grads), synchronised."""
    out = _run(copy.deepcopy(pol).to(DEV), _to_dev(t), None if first is None else first.to(DEV), h)
    torch.cuda.synchronize()
    return out


def _same_bits(a, b):
    return np.array_equal(as_numpy_u32(a), as_numpy_u32(b))


# ---- every row exactly once ----

# (A, P, K, E, N): 1, 15, 16, 17 and 33 rows per set for P = N and P = 1, then the shapes whose loop runs a second time: 16 425
# rows = 1027 tiles over 1024 workgroups, 257 rows per set = 17 tiles over 16, 4104 rows per set = 257 tiles over 204; and a third
# time: 1500 rows per set = 94 tiles over 32 workgroups
COUNT_SHAPES = [(8, 5, 1, 1, 5), (9, 5, 3, 5, 5), (8, 5, 4, 4, 5), (9, 5, 17, 1, 5), (8, 5, 3, 11, 5),
                (9, 1, 1, 1, 1), (8, 1, 1, 3, 5), (9, 1, 4, 2, 2), (8, 1, 17, 1, 1), (9, 1, 3, 11, 1),
                (9, 1, 3, 1825, 3), (8, 64, 257, 1, 64), (8, 5, 8, 513, 5), (8, 32, 3, 500, 32)]
_one_row_entropy = {}


def _entropy_of_one_row(A):
    if A not in _one_row_entropy:
        t, first = counting_inputs(A, 1, 1, 1, seed=0)
        _one_row_entropy[A] = _device_run(zero_policy(A, 1), t, first, COUNTING_HYPER)[1]["entropy"].cpu()
    return _one_row_entropy[A]


@pytest.mark.parametrize("use_first", [True, False])
@pytest.mark.parametrize("A,P,K_,E,N", COUNT_SHAPES)
def test_every_row_is_counted_exactly_once(A, P, K_, E, N, use_first):
    """All parameters zero, adv = 0, vf_pred = 0, vf_loss_coeff = 0.5 and value_targets[flat row] = 1 + flat row mod 4093: value
    = 0 exactly, each row's d loss / d value is -vt and its vf is vt^2 < 2^24, so every partial sum -- float32 in the
    workgroups, float64 in the reduction -- is an exact integer and the outputs are known to the bit.  A dropped, duplicated or
    misassigned row or tile changes an integer sum; no tolerance is involved."""
    t, first = counting_inputs(A, K_, E, N, seed=7 * K_ + E, obs_first=use_first)
    loss, stats, g = _device_run(zero_policy(A, P), t, first, COUNTING_HYPER)
    vt = t["value_targets"].double().numpy().reshape(-1, P)          # a set's rows: flat rows p, p + P, ... (all of them for P = 1)
    R = vt.shape[0]
    assert R == K_ * E * N // P
    S1, S2 = vt.sum(0), (vt * vt).sum(0)                              # exact: integers below 2^53
    assert float(S2.max()) < 2.0 ** 53
    want_b = (-S1 / np.float64(R)).astype(np.float32)                 # the reduce kernel: a float64 division, then one cast
    assert np.array_equal(as_numpy_u32(g["value_b"]).reshape(-1), want_b.view(np.uint32)), (g["value_b"].reshape(-1), want_b)
    assert np.array_equal(as_numpy_u32(stats["vf_loss"]), (S2 / np.float64(R)).view(np.uint64)), (stats["vf_loss"], S2 / R)
    assert np.array_equal(as_numpy_u32(stats["total_loss"]), (S2 / np.float64(2 * R)).view(np.uint64)), (stats["total_loss"], S2 / (2 * R))
    assert float(stats["policy_loss"].abs().max()) == 0.0 and float(stats["kl"].abs().max()) == 0.0
    for name in g:
        if name != "value_b":                                         # ReLU'(0) = 0 and adv = 0
            assert float(g[name].abs().max()) == 0.0, name
    ent = stats["entropy"].cpu()
    assert _same_bits(ent, _entropy_of_one_row(A).expand(P).contiguous()), ent
    assert abs(float(ent[0]) - np.log(A)) < 1e-6
    if P == 1:
        assert _same_bits(loss, torch.tensor(S2 / np.float64(2 * R)).sum().float())


# ---- the weight sets do not see each other ----

@pytest.mark.parametrize("use_first", [True, False])
def test_sets_are_isolated_bit_for_bit(use_first):
    """P = N = 5 with 21 rows per set (two tiles, the second ragged): set p's gradient and statistics are those of a P = 1,
    N = 1 call on set p's rows alone, to the bit -- both calls cut 21 rows into the same tiles over the same two workgroups,
    which is asserted.  Then one set's rows become the all-clipped, dead fragment: that set's gradient is exactly zero and
    every other set's outputs keep their bits."""
    A, N, K_, E = 9, 5, 3, 7
    pol = make_policy(A, N, seed=23)
    t, first = make_inputs(pol, K_, E, N, seed=123, obs_first=use_first)
    assert _capi.SSD_PPO_GROUPS(K_ * E, N) == _capi.SSD_PPO_GROUPS(K_ * E, 1) == 2
    _, stats, g = _device_run(pol, t, first, HYPER)
    for p in range(N):
        _, s1, g1 = _device_run(set_policy(pol, p), set_fragment(t, first, p), None, HYPER)
        for k in PPO_STATS:
            assert _same_bits(stats[k][p:p + 1], s1[k]), (p, k)
        for name in g:
            assert _same_bits(g[name][p:p + 1], g1[name]), (p, name)
            assert float(g1[name].abs().max()) > 0.0, (p, name)
    h = dict(HYPER, entropy_coeff=0.0, kl_coeff=0.0)
    q = 2
    dead = clipped_rows(pol, t, first)
    t2 = {k: v.clone() for k, v in t.items()}
    for k, v in dead.items():
        t2[k][:, :, q] = v[:, :, q]
    _, sa, ga = _device_run(pol, t, first, h)
    _, sb, gb = _device_run(pol, t2, first, h)
    others = [p for p in range(N) if p != q]
    for name in ga:
        assert float(gb[name][q].abs().max()) == 0.0, name
        assert float(ga[name][q].abs().max()) > 0.0, name
        assert _same_bits(ga[name][others], gb[name][others]), name
    for k in PPO_STATS:
        assert _same_bits(sa[k][others], sb[k][others]), k


# ---- the kink rules on the kernel ----

@pytest.mark.parametrize("P,K_,E,N", [(1, 2, 4, 5), (4, 2, 5, 4)])
def test_clipped_and_dead_rows_pull_nothing(P, K_, E, N):
    """40 rows, every one with the clipped branch of the surrogate as the minimum and a clipped value (test_ppo_loss_cpu.py's
    test_every_clip_branch_is_exercised, on the kernel): with vf2 the larger the whole gradient is exactly zero; with vf1 the
    larger the value side is live and meets the float64 reference while logits_w and logits_b stay exactly zero."""
    h = dict(HYPER, entropy_coeff=0.0, kl_coeff=0.0)
    pol = make_policy(8, P, seed=25 + P)
    t, first = clipped_fragment(pol, K_, E, N, seed=125 + P)
    rep = branch_report(pol, t, h, first)
    assert rep["clipped_pos"] == 1.0 and rep["vf_dead"] == 1.0 and rep["margin"] > 0.1, rep
    _, stats, g = _device_run(pol, t, first, h)
    for name in g:
        assert float(g[name].abs().max()) == 0.0, name
    assert bool(torch.isfinite(stats["total_loss"]).all())
    t, first = clipped_fragment(pol, K_, E, N, seed=125 + P, live=True)
    rep = branch_report(pol, t, h, first)
    assert rep["clipped_pos"] == 1.0 and rep["vf_clipped_live"] == 1.0 and rep["margin"] > 0.1, rep
    value_side = ("conv_w", "conv_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "value_w", "value_b")
    _, _, g, g64 = compare_with_float64(pol, t, first, h, only=value_side)
    for name in ("logits_w", "logits_b"):
        assert float(g[name].abs().max()) == 0.0 and float(g64[name].abs().max()) == 0.0, name
    for name in value_side:
        assert float(g[name].abs().max()) > 0.0, name


@pytest.mark.parametrize("P", [1, 4])
def test_first_epoch_tie_on_the_kernel(P):
    """An on-policy fragment built on the device (logp_old and vf_pred from the policy's own float32 forward there): every row
    sits inside both clip ranges, where the kernel takes the unclipped derivative and min and max see identical operands.  So
    the call with (clip_param, vf_clip_param) = (0.3, 1) equals the call with (1e6, 1e6) to the bit, the gradient is not zero,
    and it meets the float64 reference of the unclipped loss."""
    K_, E, N = 4, 6, 4
    h = dict(HYPER, kl_coeff=0.0)
    huge = dict(h, clip_param=1e6, vf_clip_param=1e6)
    pol = make_policy(8, P, seed=27 + P)
    t, first = make_inputs(pol, K_, E, N, seed=127 + P, behaviour=False, on_policy=True)
    dpol = copy.deepcopy(pol).to(DEV)
    with torch.no_grad():
        logits, value = dpol(shifted_obs(t["obs"], first, K_).to(DEV))
        logp = torch.log_softmax(logits, -1).gather(-1, t["actions"].to(DEV).long().unsqueeze(-1)).squeeze(-1)
        t["logp_old"], t["vf_pred"] = logp.cpu().contiguous(), value.cpu().contiguous()
        logits64, value64 = copy.deepcopy(pol).double()(shifted_obs(t["obs"], first, K_))
        logp64 = torch.log_softmax(logits64, -1).gather(-1, t["actions"].long().unsqueeze(-1)).squeeze(-1)
    assert float((torch.exp(logp64 - t["logp_old"].double()) - 1).abs().max()) < 1e-4
    assert float((value64 - t["vf_pred"].double()).abs().max()) < 1e-4
    la, sa, ga = _device_run(pol, t, first, h)
    lb, sb, gb = _device_run(pol, t, first, huge)
    assert _same_bits(la, lb)
    for k in PPO_STATS:
        assert _same_bits(sa[k], sb[k]), k
    for name in ga:
        assert _same_bits(ga[name], gb[name]), name
        assert float(ga[name].abs().max()) > 0.0, name
    _, _, g64 = autograd_loss(pol, t, huge, first)
    _, _, g32 = autograd_loss(pol, t, huge, first, dtype=torch.float32, device=DEV)
    _check_against_reference(ga, g32, g64, "tie grad")


# ---- the edges of the contract against float64 ----

@pytest.mark.parametrize("P,N", [(1, 3), (5, 5)])
@pytest.mark.parametrize("A", [1, 2, 15])
def test_fewest_and_most_actions(A, P, N):
    """A = 15 puts the value into the last of the sixteen head columns, A = 1 makes the softmax trivial (and the gradient of
    the logits layer exactly zero: p = 1, log p = 0), A = 2 is the smallest softmax that is not."""
    seed = 30 + A + P
    pol = make_policy(A, P, seed=seed)
    t, first = make_inputs(pol, 3, 6, N, seed=100 + seed)
    rep = branch_report(pol, t, HYPER, first)
    print("A", A, "P", P, rep)
    assert rep["margin"] > MARGIN, rep
    _, _, g, _ = compare_with_float64(pol, t, first, HYPER)
    if A == 1:
        assert float(g["logits_w"].abs().max()) == 0.0 and float(g["logits_b"].abs().max()) == 0.0
    else:
        assert float(g["logits_w"].abs().max()) > 0.0 and float(g["logits_b"].abs().max()) > 0.0


@pytest.mark.parametrize("P,seed", [(5, 40), (1, 41)])
def test_zero_clip_ranges(P, seed):
    """clip_param = 0 and vf_clip_param = 0, both legal: every row is clipped on both sides."""
    h = dict(HYPER, clip_param=0.0, vf_clip_param=0.0)
    pol = make_policy(8, P, seed=seed)
    t, first = make_inputs(pol, 4, 9, 5, seed=100 + seed)
    rep = branch_report(pol, t, h, first)
    print("P", P, rep)
    assert rep["margin"] > MARGIN and rep["open_pos"] == rep["open_neg"] == 0.0, rep
    assert rep["vf_dead"] > 0.1 and rep["vf_live"] > 0.1 and rep["vf_clipped_live"] == rep["vf_live"], rep
    compare_with_float64(pol, t, first, h)


@pytest.mark.parametrize("P,N", [(1, 3), (5, 5)])
def test_saturated_logits(P, N):
    """logits_w scaled until the float64 reference's smallest chosen-action log-probability is below -80: float32 probabilities
    underflow (to subnormals or zero).  Every output stays finite and meets the bound; logp_old comes from that saturated forward, so the
    ratios stay in make_inputs' regions."""
    pol = make_policy(8, P, seed=50 + P)
    t, first, low = saturate(pol, lambda q: make_inputs(q, 3, 6, N, seed=150 + P))
    rep = branch_report(pol, t, HYPER, first)
    print("P", P, "smallest chosen log-probability", low, rep)
    assert low < -80.0 and rep["margin"] > MARGIN, (low, rep)
    with torch.no_grad():                                  # float32 probabilities below the normal range: they underflow
        assert float(torch.softmax(pol(shifted_obs(t["obs"], first, 3))[0], -1).min()) < torch.finfo(torch.float32).tiny
    compare_with_float64(pol, t, first, HYPER)


@pytest.mark.parametrize("P,big,small", [(1, (8, 16, 5), (17, 1, 1)), (5, (8, 20, 5), (17, 1, 5))])
def test_kept_scratch_serves_a_smaller_call(P, big, small):
    """ppo_loss keeps a grow-only scratch on the policy.  A 17-row call after a call that needed a larger one reads partials
    at the smaller call's own pitch: its outputs equal, to the bit, those of the same call on a fresh copy of the policy."""
    pol = make_policy(9, P, seed=60 + P)
    tb, fb = make_inputs(pol, *big, seed=160 + P)
    ts, fs = make_inputs(pol, *small, seed=161 + P)
    dpol = copy.deepcopy(pol).to(DEV)
    fresh = copy.deepcopy(dpol)
    _run(dpol, _to_dev(tb), fb.to(DEV), HYPER)
    kept = dpol._ppo_scratch
    assert kept.numel() == pol.ppo_scratch_shape(big[0] * big[1] * big[2] // P)[0] > pol.ppo_scratch_shape(17)[0]
    la, sa, ga = _run(dpol, _to_dev(ts), fs.to(DEV), HYPER)
    assert dpol._ppo_scratch is kept and not hasattr(fresh, "_ppo_scratch")
    lb, sb, gb = _run(fresh, _to_dev(ts), fs.to(DEV), HYPER)
    torch.cuda.synchronize()
    assert fresh._ppo_scratch.numel() == pol.ppo_scratch_shape(17)[0]
    assert _same_bits(la, lb)
    for k in PPO_STATS:
        assert _same_bits(sa[k], sb[k]), k
    for name in ga:
        assert _same_bits(ga[name], gb[name]) and float(ga[name].abs().max()) > 0.0, name
