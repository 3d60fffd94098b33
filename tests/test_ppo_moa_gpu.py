"""ppo_loss_moa on the MI355X (csrc/ssd_policy_moa_grad.hip, ssd_policy_moa_ppo_grad): the kernels' gradients and statistics
against the float64 restatement (ppo_moa_ref.py) with torch's own float32 autograd on the same device as the yardstick, the
persistent tile loop (in the row accounting, and an accuracy case with the float64 restatement on the device), the split-K kernels' second chunks (windows of
more than 32 chunks of one set's rows: the second pass over the accumulators, a ragged last chunk that is a second chunk, splits
that get no chunk of the second window, rows >= 2048), exact row accounting, exact zeros where no gradient may flow, bit-equal repeats, set isolation,
moa_weight = 0, the kink rules on rows clipped on both signs of the advantage (dead and live), rows exactly on policy (the
clip range does not show, policy_loss = -1 and kl = 0 exactly), and one optimiser step end to end from sample()."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from ppo_moa_ref import (ACTIONS_BRANCH, CONV_MARGIN, HYPER, MARGIN, MOA_BRANCH, MOA_WEIGHT, as_numpy_u32, autograd_loss, branch_report, clipped_rows,
                         counting_inputs, forward, make_inputs, make_policy, max_err, shifted_obs, split_case, zero_policy)
from ppo_ref import COUNTING_HYPER, LOOSE, on_policy_checks
from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd import evaluate_fragment, ppo_loss_moa
from sequential_social_dilemma_games_amd.policy import MOA_PPO_STATS
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# The factor of `ek <= FACTOR * et + 1e-6 * max(1, max |ref|)` per parameter tensor (DESIGN.md section 18 records the measured
# ek / et): the project's margin, 4, for every tensor.
FACTOR = {}
BRANCHES = ("clipped_pos", "clipped_neg", "open_pos", "open_neg", "vf_dead", "vf_live", "vf_clipped_live")


def case(K_=7, T=3, E=17, N=5, P=5, A=8, C_=64, beh=True, first=True, done="none", stream=False, seed=1):
    return (K_, T, E, N, P, A, C_, beh, first, done, stream, seed)


# each line varies one thing from (K, T) = (7, 3), 17 envs, N = P = 5, A = 8, C = 64
CASES = [case(1, 1, seed=1), case(5, 5, seed=2), case(7, 3, seed=3), case(4, 8, seed=4), case(6, 1, seed=5),             # (K, T)
         case(E=1, seed=6), case(E=15, seed=7), case(E=16, seed=8), case(E=33, seed=3112),                               # sequences per set
         case(P=1, seed=10),
         case(N=2, P=2, seed=11),                                  # one other agent: a partial prediction tile
         case(N=11, P=11, seed=12),                                # string order != index order
         case(N=16, P=16, A=15, seed=13),                          # 225 prediction columns: all 15 tiles, the last ragged
         case(3, 3, E=16, C_=256, seed=15),
         case(A=1, seed=14), case(C_=128, seed=16),
         case(first=False, seed=17), case(beh=False, seed=18),
         case(done="mid", seed=19), case(done="window_end", seed=20), case(done="last", seed=21), case(done="per_env", seed=22),
         case(stream=True, done="per_env", seed=23)]


def _to_dev(t):
    return {k: v.to(DEV) for k, v in t.items()}


def _grads(pol):
    return {name: getattr(pol, name).grad.detach().clone() for name, _, _ in pol.layout()}


def _run(pol, t, first, h, T, moa_weight=MOA_WEIGHT):
    """ppo_loss_moa + backward on the device -> (loss, stats, {param: grad})."""
    pol.zero_grad()
    loss, stats = ppo_loss_moa(pol, t, seq_len=T, moa_weight=moa_weight, obs_first=first, **h)
    loss.backward()
    return loss.detach(), stats, _grads(pol)


def _check_against_reference(got, tor, ref, what):
    """ek <= factor * et + 1e-6 * max(1, max |ref|) for every tensor of the dicts; prints each figure before it asserts."""
    bad = []
    for name in ref:
        ek, et = max_err(got[name], ref[name]), max_err(tor[name], ref[name])
        scale = max(1.0, float(ref[name].abs().max()))
        print("%s %-14s ek %.3e et %.3e ek/et %.2f max|ref| %.3e" % (what, name, ek, et, ek / et if et else float("inf"), scale))
        if not ek <= FACTOR.get(name, 4.0) * et + 1e-6 * scale:
            bad.append((name, ek, et))
    assert not bad, (what, bad)


def _equal_bits(a, b):
    la, sa, ga = a
    lb, sb, gb = b
    assert np.array_equal(as_numpy_u32(la), as_numpy_u32(lb))
    for k in MOA_PPO_STATS:
        assert np.array_equal(as_numpy_u32(sa[k]), as_numpy_u32(sb[k])), k
    for name in ga:
        assert np.array_equal(as_numpy_u32(ga[name]), as_numpy_u32(gb[name])), name


def compare_with_float64(pol, t, first, h, T, own_stream=False, ref_device="cpu"):
    """The kernels on (pol, t, first, h) against the float64 restatement (torch's float64 ops on ref_device) with torch's
    float32 autograd on the device as the yardstick -- gradients, statistics and loss under the bound --, all outputs finite,
    and a second call bit-equal to the first."""
    P = pol.num_sets
    loss64, stats64, g64 = autograd_loss(pol, t, h, first, T, device=ref_device)
    loss32, stats32, g32 = autograd_loss(pol, t, h, first, T, dtype=torch.float32, device=DEV)
    dpol, dt, dfirst = copy.deepcopy(pol).to(DEV), _to_dev(t), None if first is None else first.to(DEV)
    if own_stream:
        s = torch.cuda.Stream(DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            out = _run(dpol, dt, dfirst, h, T)
        s.synchronize()
    else:
        out = _run(dpol, dt, dfirst, h, T)
    torch.cuda.synchronize()
    loss, stats, g = out
    assert all(tuple(stats[k].shape) == (P,) and stats[k].dtype == torch.float64 for k in MOA_PPO_STATS)
    assert all(bool(torch.isfinite(x).all()) for x in list(g.values()) + list(stats.values()) + [loss])
    _check_against_reference(g, g32, g64, "grad")
    _check_against_reference(stats, stats32, stats64, "stat")
    _check_against_reference({"loss": loss}, {"loss": loss32}, {"loss": loss64}, "loss")
    out2 = _run(dpol, dt, dfirst, h, T)
    torch.cuda.synchronize()
    _equal_bits(out, out2)
    return out


@pytest.mark.parametrize("K_,T,E,N,P,A,C_,beh,use_first,done,own_stream,seed", CASES)
def test_gradients_and_stats_against_float64(K_, T, E, N, P, A, C_, beh, use_first, done, own_stream, seed):
    h = dict(HYPER, kl_coeff=HYPER["kl_coeff"] if beh else 0.0)
    pol = make_policy(A, N, P, C_, seed=seed)
    t, first = make_inputs(pol, K_, E, N, T, seed=100 + seed, obs_first=use_first, behaviour=beh, done_mode=done)
    rep = branch_report(pol, t, h, first, T)
    print("case", (K_, T, E, N, P, A, C_, beh, use_first, done, own_stream), rep)
    assert rep["margin"] > MARGIN and rep["conv_margin"] >= CONV_MARGIN, rep
    if K_ * E * N >= 1000:                                       # E = 33, N = 11 and N = 16: the seeds were chosen on the CPU
        for k in BRANCHES:
            assert rep[k] > 0.2, rep
    _, _, g = compare_with_float64(pol, t, first, h, T, own_stream)
    if A == 1:                                                   # one action: softmax = onehot = 1, nothing to learn
        for name in ("logits_w", "logits_b", "pred_w", "pred_b"):
            assert float(g[name].abs().max()) == 0.0, name


# The persistent loop (more tiles than workgroups) needs 16 G + 1 sequences per set, G the exported groups macro: at P = N = 16
# that is 1025 envs.
def _multi_tile_envs(P):
    G = _capi.SSD_MPPO_GROUPS(10 ** 6, P)
    E = 16 * G + 1
    assert _capi.SSD_MPPO_GROUPS(E, P) == G and -(-E // 16) == G + 1
    return E


def test_persistent_loop_takes_a_second_tile():
    """The accuracy case of the persistent loop: P = N = 16, 1025 envs, K = T = 2, 32 800 rows, input seed 300 chosen on the
    CPU (margin 2.5e-4, every branch above 0.2 of the rows).  With the float64 restatement on the CPU it took 14.3 s; here
    make_inputs, branch_report and the reference run torch's float64 ops on the device (the random numbers are drawn on the CPU
    as ever).  Same bound, same factor.  What the row accounting cannot see: the carried dh / dc, the heads' register sums
    across tiles, dpred through scratch, the trunk's third mode adding the second stack's conv sums on a second tile.
    4.8 s on the MI355X, 4.3 s in a second run (the phases, timed once: make_inputs 1.2 s, branch_report 0.6 s, the float64 autograd 0.7 s, the float32
    yardstick's first call at this shape 2.0 s)."""
    P = N = 16
    E = _multi_tile_envs(P)
    pol = make_policy(8, N, P, 64, seed=30 + P)
    t, first = make_inputs(pol, 2, E, N, 2, seed=300, done_mode="per_env", device=DEV)
    rep = branch_report(pol, t, HYPER, first, 2, device=DEV)
    print("multi-tile", (P, N, E), rep)
    assert rep["margin"] > MARGIN and rep["conv_margin"] >= CONV_MARGIN, rep
    for k in BRANCHES:
        assert rep[k] > 0.2, rep
    compare_with_float64(pol, t, first, HYPER, 2, ref_device=DEV)


def test_inputs_do_not_depend_on_where_the_float64_forward_runs():
    """make_inputs draws every random number on the CPU and rounds what it takes from the float64 forward to float32: the
    fragment (the rows drawn again for the conv's kink included) is the same to the bit with that forward on the device, and
    branch_report's figures agree."""
    pol = make_policy(8, 5, 5, 64, seed=22)
    t, first = make_inputs(pol, 7, 17, 5, 3, seed=122, done_mode="per_env")
    td, firstd = make_inputs(pol, 7, 17, 5, 3, seed=122, done_mode="per_env", device=DEV)
    assert t.keys() == td.keys() and torch.equal(first, firstd)
    for k in t:
        assert td[k].device.type == "cpu" and td[k].dtype == t[k].dtype and torch.equal(t[k], td[k]), k
    rep, repd = branch_report(pol, t, HYPER, first, 3), branch_report(pol, t, HYPER, first, 3, device=DEV)
    assert all(abs(rep[k] - repd[k]) <= 1e-12 for k in rep), (rep, repd)


@pytest.mark.parametrize("shape", ["A", "B"])
def test_split_k_takes_a_second_chunk(shape):
    """`chunk += S` of ssd_bptt_dw_kernel (both branches) and ssd_moa_dpred_kernel: the first window holds more than
    SSD_MPPO_MAX_SPLITS chunks of a set's rows (A: P = 1, N = 5, 2145 rows, 34 chunks, the last of 33 rows; B: P = N = 2, 2080
    rows a set, 33 chunks, the last of 32 rows, and one other agent: the partial prediction tile), the second window fewer chunks
    than splits (3 and 2), so most splits must keep what the first left.  Ordinary inputs: at MOA_WEIGHT one row lost or doubled
    is 10 bounds or more in every tensor these kernels write (test_ppo_moa_cpu.py measures it)."""
    splits, chunk = _capi.SSD_MPPO_MAX_SPLITS, _capi.SSD_MPPO_CHUNK
    pol, t, first, (K_, T, E, N, P), _ = split_case(shape, 64, splits, chunk)
    rows1, rows2 = T * (E * N // P), (K_ - T) * (E * N // P)
    assert _capi.SSD_MPPO_SPLITS(rows1) == splits == 32 and -(-rows1 // chunk) > splits and rows1 % chunk
    assert 0 < -(-rows2 // chunk) < splits
    rep = branch_report(pol, t, HYPER, first, T)
    print("split", shape, rep)
    assert rep["margin"] > MARGIN and rep["conv_margin"] >= CONV_MARGIN, rep
    for k in BRANCHES:
        assert rep[k] > 0.2, rep
    compare_with_float64(pol, t, first, HYPER, T)


@pytest.mark.parametrize("P,N,E", [(5, 5, 1), (5, 5, 16), (5, 5, 17), (5, 5, 33), (1, 5, 1), (1, 5, 16), (1, 5, 17), (1, 5, 33),
                                   (16, 16, _multi_tile_envs(16))])
def test_every_row_is_counted_exactly_once(P, N, E):
    """All parameters zero, adv = 0, vf_pred = 0, vf_loss_coeff = 0.5 and value_targets[flat row] = 1 + flat row mod 4093: z = 0,
    (h', c') = 0 from a zero ring and value = 0, so d loss / d value_b = -sum(vt) / R and vf_loss = sum(vt^2) / R, both exact.
    The predictions are zero too: every cross-entropy is logf(8) (the same float32 for every row, so its float64 sum is exact),
    moa_loss is that number for every set, and pred_b's gradient of column (j, k) is moa_weight / (N - 1) (softmax - [k is the
    target]) summed over the rows: with moa_weight = N - 1, pred_b.grad = 1/8 - the share of the set's rows whose j-th other
    agent took k, up to expf's rounding of 1/8.  Every other gradient is exactly zero.  E counts envs: E or E N sequences per
    set."""
    A, C_, K_, T = 8, 64, 7, 3
    pol = zero_policy(A, N, P, C_).to(DEV)
    t, first = counting_inputs(A, C_, K_, E, N, T, seed=40 + E)
    _, stats, g = _run(pol, _to_dev(t), first.to(DEV), COUNTING_HYPER, T, moa_weight=float(N - 1))
    torch.cuda.synchronize()
    vt = t["value_targets"].double()
    R = K_ * E * N // P
    per_set = (lambda x: x.reshape(-1, P).sum(0)) if P > 1 else (lambda x: x.sum().reshape(1))
    want_b = (-per_set(vt) / R).float()
    assert np.array_equal(as_numpy_u32(g["value_b"].reshape(-1)), as_numpy_u32(want_b))
    want_vf = per_set(vt * vt) / R
    assert np.array_equal(as_numpy_u32(stats["vf_loss"]), as_numpy_u32(want_vf))
    ce = float(stats["moa_loss"][0])
    assert abs(ce - np.log(8.0)) < 1e-6 and bool((stats["moa_loss"] == ce).all())
    others = torch.from_numpy(np.asarray(pol._others.cpu()))
    tgt = torch.nn.functional.one_hot(t["actions"].long()[..., others], A).double()          # [K, E, N, N-1, A]
    count = tgt.reshape(-1, N, (N - 1) * A).sum(0) if P > 1 else tgt.reshape(-1, (N - 1) * A).sum(0, keepdim=True)
    want_pb = (R / 8.0 - count) / R
    assert float((g["pred_b"].cpu().double() - want_pb).abs().max()) < 1e-6      # one row more or less moves it by 1 / R > 8e-4
    for name in g:
        if name not in ("value_b", "pred_b"):
            assert float(g[name].abs().max()) == 0.0, name


def _packed_call(pol, t, first, K_, E, N, T, moa_weight, scratch=None):
    """The C call itself on a NaN-filled gradient buffer -> (packed [P, set_floats], stats [P, 6])."""
    P, A = pol.num_sets, pol.num_actions
    packed = torch.full((P, pol.set_floats), float("nan"), dtype=torch.float32, device=DEV)
    stats = torch.zeros((P, 6), dtype=torch.float64, device=DEV)
    if scratch is None:
        scratch = torch.empty(pol.ppo_scratch_shape(K_, E, N, T), dtype=torch.float32, device=DEV)
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())   # noqa: E731
    hv = [HYPER[k] for k in ("clip_param", "vf_clip_param", "vf_loss_coeff", "entropy_coeff", "kl_coeff")] + [moa_weight]
    _capi.policy_check(_capi.lib().ssd_policy_moa_ppo_grad(
        ptr(pol.packed()), P, A, pol.cell_size, T, ptr(first), ptr(t["obs"]), ptr(t["state"]), ptr(t["prev_actions"]), ptr(t.get("done")),
        ptr(t["actions"]), ptr(t["logp_old"]), ptr(t["advantages"]), ptr(t["value_targets"]), ptr(t["vf_pred"]),
        ptr(t["behaviour_logits"]), K_, E, N, *hv, ptr(scratch), ptr(packed), ptr(stats), 0, 0,
        C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
    torch.cuda.synchronize()
    return packed, stats


def test_packed_gradient_padding_scaling_and_minibatch():
    """The library's packed gradient has zero padding floats, zero rows 32 + N .. 47 of the MOA matrix, and holds what backward
    scatters; backward multiplies by the incoming gradient; a minibatch is addressed by slices."""
    A, N, K_, E, T = 9, 5, 5, 7, 2
    pol = make_policy(A, N, N, 64, seed=90)
    t, first = make_inputs(pol, K_, E, N, T, seed=91, done_mode="mid")
    pol, t, first = pol.to(DEV), _to_dev(t), first.to(DEV)
    _, _, g = _run(pol, t, first, HYPER, T)
    packed, _ = _packed_call(pol, t, first, K_, E, N, T, MOA_WEIGHT)
    S = pol.set_floats
    used = torch.zeros(S, dtype=torch.bool, device=DEV)
    for name, shape, off in pol.layout():
        n = int(np.prod(shape))
        used[off:off + n] = True
        assert torch.equal(packed[:, off:off + n].reshape(g[name].shape), g[name]), name
    assert int((~used).sum()) > 0 and float(packed[:, ~used].abs().max()) == 0.0
    mw, n4 = _capi.SSD_MOA_MW(64, A), 4 * 64
    assert not bool(used[mw + (32 + N) * n4:mw + 48 * n4].any())                  # the MOA input's zero rows are padding
    assert float(g["moa_kernel"][:, 32:].abs().amax(2).min()) > 0.0            # ... and the action rows are not
    pol.zero_grad()
    loss, _ = ppo_loss_moa(pol, t, seq_len=T, moa_weight=MOA_WEIGHT, obs_first=first, **HYPER)
    (loss * 3.0).backward()
    for name in g:
        assert torch.equal(getattr(pol, name).grad, g[name] * 3.0), name
    # a minibatch addressed by slices: steps 2 .. 4 with the ring from slot 1 and obs_first = obs[1]
    mb = {k: v[2:] for k, v in t.items() if k != "state"}
    a = _run(pol, dict(mb, state=t["state"][1:]), t["obs"][1], HYPER, T)
    b = _run(pol, dict({k: v.clone() for k, v in mb.items()}, state=t["state"][1:].clone(), obs=t["obs"][1:4].clone()), None, HYPER, T)
    _equal_bits(a, b)


def test_repeats_and_a_grown_scratch_give_the_same_bits():
    pol = make_policy(8, 5, 5, 64, seed=60)
    t, first = make_inputs(pol, 7, 17, 5, 3, seed=61, done_mode="per_env")
    big, big_first = make_inputs(pol, 9, 40, 5, 4, seed=62)
    pol, t, first = pol.to(DEV), _to_dev(t), first.to(DEV)
    fresh = copy.deepcopy(pol)
    a = _run(pol, t, first, HYPER, 3)
    _run(pol, _to_dev(big), big_first.to(DEV), HYPER, 4)
    grown = pol._ppo_scratch.numel()
    pol._ppo_scratch.fill_(float("nan"))                       # whatever an earlier call left there is never read
    b = _run(pol, t, first, HYPER, 3)
    assert pol._ppo_scratch.numel() == grown > fresh.ppo_scratch_shape(7, 17, 5, 3)[0]
    c = _run(fresh, t, first, HYPER, 3)
    torch.cuda.synchronize()
    _equal_bits(a, b)
    _equal_bits(a, c)


def test_set_isolation():
    """At P = N = 5 set p's gradient and statistics depend on set p's weights, on agent p's rows and on the joint actions
    alone: with every other set's weights and every other agent's observations, states and per-row floats replaced, they keep
    their bits."""
    E, N, K_, T = 17, 5, 7, 3
    pol = make_policy(8, N, N, 64, seed=70)
    t, first = make_inputs(pol, K_, E, N, T, seed=71, done_mode="per_env")
    other = make_policy(8, N, N, 64, seed=72)
    t2, first2 = make_inputs(other, K_, E, N, T, seed=73, done_mode="per_env")
    _, stats, g = _run(copy.deepcopy(pol).to(DEV), _to_dev(t), first.to(DEV), HYPER, T)
    for p in (0, 3):
        mixed = copy.deepcopy(other)
        with torch.no_grad():
            for name, _, _ in pol.layout():
                getattr(mixed, name)[p] = getattr(pol, name)[p]
        tm = {}
        for k in t:
            if k in ("actions", "prev_actions"):
                tm[k] = t[k]
            elif k == "state":
                tm[k] = t2[k].clone()
                tm[k][:, :, p] = t[k][:, :, p]
            else:
                tm[k] = t2[k].clone()
                tm[k][:, :, p] = t[k][:, :, p]
        fm = first2.clone()
        fm[:, p] = first[:, p]
        _, s1, g1 = _run(mixed.to(DEV), _to_dev(tm), fm.to(DEV), HYPER, T)
        torch.cuda.synchronize()
        for name in g1:
            assert np.array_equal(as_numpy_u32(g[name][p:p + 1]), as_numpy_u32(g1[name][p:p + 1])), (p, name)
        for k in MOA_PPO_STATS:
            assert np.array_equal(as_numpy_u32(stats[k][p:p + 1]), as_numpy_u32(s1[k][p:p + 1])), (p, k)


def test_a_reset_row_reads_neither_state_nor_previous_actions():
    """The zero of a step after a done row is selected, never loaded: with other previous actions at those rows (a rollout's
    ring holds zero there) the call returns the same bits."""
    K_, T = 7, 3
    pol = make_policy(8, 5, 5, 64, seed=77)
    t, first = make_inputs(pol, K_, 17, 5, T, seed=78, done_mode="per_env")
    reset = torch.zeros_like(t["done"])
    reset[1:] = t["done"][:-1]
    reset[::T] = 0                                              # a window's first step reads the ring as stored
    assert int(reset.sum()) > 0 and int(t["prev_actions"][reset.bool()].abs().sum()) == 0
    dirty = torch.where(reset.bool(), 1 + t["actions"] % 7, t["prev_actions"]).contiguous()
    pol, first = pol.to(DEV), first.to(DEV)
    a = _run(pol, _to_dev(t), first, HYPER, T)
    b = _run(pol, _to_dev(dict(t, prev_actions=dirty)), first, HYPER, T)
    torch.cuda.synchronize()
    _equal_bits(a, b)


def test_moa_weight_zero():
    """moa_weight = 0: exact zeros on the MOA branch, the bits of the weighted call's actions branch (no term of the
    cross-entropy reaches it), a total_loss without the MOA term and the same moa_loss."""
    T = 3
    pol = make_policy(8, 5, 5, 64, seed=75)
    t, first = make_inputs(pol, 7, 17, 5, T, seed=76, done_mode="per_env")
    pol, t, first = pol.to(DEV), _to_dev(t), first.to(DEV)
    _, s1, g1 = _run(pol, t, first, HYPER, T)
    _, s0, g0 = _run(pol, t, first, HYPER, T, moa_weight=0.0)
    torch.cuda.synchronize()
    for name in MOA_BRANCH:
        assert float(g0[name].abs().max()) == 0.0 and float(g1[name].abs().max()) > 0.0, name
    for name in ACTIONS_BRANCH:
        assert np.array_equal(as_numpy_u32(g0[name]), as_numpy_u32(g1[name])), name
    assert not torch.equal(g0["conv_w"], g1["conv_w"])
    for k in MOA_PPO_STATS[1:]:
        assert np.array_equal(as_numpy_u32(s0[k]), as_numpy_u32(s1[k])), k
    assert float((s1["total_loss"] - s0["total_loss"] - MOA_WEIGHT * s1["moa_loss"]).abs().max()) < 1e-12


KINK_HYPER = dict(HYPER, entropy_coeff=0.0, kl_coeff=0.0)


def _clipped_fragment(live):
    """The file's smallest standard fragment (K = 7, T = 3, 17 envs, N = P = 5, A = 8, C = 64, done per env) with every row
    clipped on both signs of the advantage (ppo_moa_ref.clipped_rows with a seed) -> (policy, t, obs_first, branch report),
    the conditions on the float64 reference asserted."""
    T = 3
    pol = make_policy(8, 5, 5, 64, seed=80)
    t, first = make_inputs(pol, 7, 17, 5, T, seed=81, behaviour=False, done_mode="per_env")
    t = dict(t, **clipped_rows(pol, t, first, T, live=live, seed=82))
    rep = branch_report(pol, t, KINK_HYPER, first, T)
    print("clipped, live" if live else "clipped, dead", rep)
    assert rep["open_pos"] == 0.0 and rep["open_neg"] == 0.0 and abs(rep["clipped_pos"] + rep["clipped_neg"] - 1.0) <= 1e-12, rep
    assert rep["clipped_pos"] > 0.3 and rep["clipped_neg"] > 0.3 and rep["margin"] > 0.1 and rep["conv_margin"] >= CONV_MARGIN, rep
    assert (rep["vf_clipped_live"] == 1.0 and rep["vf_dead"] == 0.0) if live else (rep["vf_dead"] == 1.0), rep
    return pol, t, first, rep


def test_clipped_and_dead_rows_give_exactly_zero():
    """The kink rules on ssd_policy_moa_ppo_grad: every row clipped with the clipped operand the minimum (adv = +1 at ratio 1.5,
    adv = -1 at ratio 0.5) and dead; with moa_weight = entropy_coeff = kl_coeff = 0 every gradient tensor is exactly zero, and a
    set's policy_loss is -(1.3 * its share of adv > 0) + 0.7 * its share of adv < 0 (the tolerance of the recurrent test)."""
    pol, t, first, _ = _clipped_fragment(live=False)
    loss, stats, g = _run(pol.to(DEV), _to_dev(t), first.to(DEV), KINK_HYPER, 3, moa_weight=0.0)
    torch.cuda.synchronize()
    pos = (t["advantages"] > 0).double().reshape(-1, 5).mean(0)
    want = -(1.3 * pos) + 0.7 * (1.0 - pos)
    print("policy_loss", stats["policy_loss"].tolist(), "want", want.tolist(), "vf_loss", stats["vf_loss"].tolist())
    for name in g:
        assert float(g[name].abs().max()) == 0.0, name
    assert float((stats["policy_loss"].cpu() - want).abs().max()) < 1e-4 and float((stats["vf_loss"] - 0.64).abs().max()) < 1e-3
    assert all(bool(torch.isfinite(stats[k]).all()) for k in MOA_PPO_STATS) and bool(torch.isfinite(loss))


def test_clipped_and_live_rows_pull_through_the_value_alone():
    """The same rows with the value branch clipped and live: d vf / d value = 2 (value - vt), nothing through the ratio.  The
    logits layer is exactly zero in the kernel and in the float64 reference, the MOA branch is exactly zero (moa_weight = 0), and
    the value head, the actions LSTM, stack 0 and the conv are non-zero and within the project's bound of float64."""
    T = 3
    pol, t, first, _ = _clipped_fragment(live=True)
    loss64, stats64, g64 = autograd_loss(pol, t, KINK_HYPER, first, T, moa_weight=0.0)
    loss32, stats32, g32 = autograd_loss(pol, t, KINK_HYPER, first, T, moa_weight=0.0, dtype=torch.float32, device=DEV)
    loss, stats, g = _run(copy.deepcopy(pol).to(DEV), _to_dev(t), first.to(DEV), KINK_HYPER, T, moa_weight=0.0)
    torch.cuda.synchronize()
    for name in ("logits_w", "logits_b") + MOA_BRANCH:
        assert float(g[name].abs().max()) == 0.0 and float(g64[name].abs().max()) == 0.0, name
    rest = [name for name in g if name not in ("logits_w", "logits_b") + MOA_BRANCH]
    assert set(rest) == set(ACTIONS_BRANCH + ("conv_w", "conv_b")) - {"logits_w", "logits_b"}
    for name in rest:
        assert float(g[name].abs().max()) > 0.0 and float(g64[name].abs().max()) > 0.0, name
    assert all(bool(torch.isfinite(x).all()) for x in list(g.values()) + list(stats.values()) + [loss])
    _check_against_reference(g, g32, g64, "live grad")
    _check_against_reference(stats, stats32, stats64, "live stat")
    _check_against_reference({"loss": loss}, {"loss": loss32}, {"loss": loss64}, "live loss")


def test_on_policy_rows_exactly():
    """test_sample_loss_step_sample's fragment before any step: the weights that sampled, logp_old = the rollout's logp, vf_pred
    = its value, and the behaviour logits from the library's sequence forward of the same rows (sample() records no logits;
    that call gives the rollout's to the bit).  The header builds the loss call's forward from the device pieces of the
    rollout, so the kernel's ratio is 1 and its value - vf_pred is 0 exactly: ppo_ref.on_policy_checks -- the clip ranges
    (0, 0) and (1e6, 1e6) give the same bits, policy_loss = -1 and kl = 0 exactly under advantages = 1, the KL term moves no
    gradient -- and the (0, 0) gradient against the float64 reference of the unclipped loss."""
    E, N, steps, T = 64, 5, 12, 4
    h = dict(vf_loss_coeff=1e-2, entropy_coeff=1e-3, kl_coeff=0.2)
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=7, seed=5)
    pol = make_policy(env.engine.num_actions, N, N, 64, seed=31, recur=2.0).to(DEV)
    first = env.reset().clone()
    batch = env.sample(pol, steps, state_every=T, gamma=0.99, lambda_=0.95, influence_weight=1.0)
    logits, value, _ = evaluate_fragment(pol, batch, obs_first=first, seq_len=T, one_call=True)
    assert torch.equal(value, batch["value"])                  # the sequence forward gives back the rollout's values ...
    lp = torch.log_softmax(logits, -1).gather(-1, batch["actions"].long().unsqueeze(-1)).squeeze(-1)
    assert float((torch.exp(lp - batch["logp"]) - 1).abs().max()) < 1e-4      # ... and its logits the rollout's logp

    def call(clip_param, vf_clip_param, kl=True, ones=False):
        b = dict(batch, advantages=torch.ones_like(batch["value"])) if ones else dict(batch)
        if kl:
            b["logits"] = logits.contiguous()
        out = _run(pol, b, first, dict(h, clip_param=clip_param, vf_clip_param=vf_clip_param, kl_coeff=h["kl_coeff"] if kl else 0.0), T)
        torch.cuda.synchronize()
        return out
    loss, stats, g = on_policy_checks(call, MOA_PPO_STATS, "moa")
    t = {"obs": batch["obs"], "actions": batch["actions"], "logp_old": batch["logp"], "advantages": batch["advantages"],
         "value_targets": batch["value_targets"], "vf_pred": batch["value"], "behaviour_logits": logits.contiguous(),
         "state": batch["state"], "done": batch["done"], "prev_actions": batch["prev_actions"]}
    cpu_t = {k: v.cpu() for k, v in t.items()}
    hl = dict(h, **LOOSE)
    loss64, stats64, g64 = autograd_loss(copy.deepcopy(pol).cpu(), cpu_t, hl, first.cpu(), T)
    loss32, stats32, g32 = autograd_loss(pol, cpu_t, hl, first.cpu(), T, dtype=torch.float32, device=DEV)
    _check_against_reference(g, g32, g64, "on-policy grad")
    _check_against_reference(stats, stats32, stats64, "on-policy stat")
    _check_against_reference({"loss": loss}, {"loss": loss32}, {"loss": loss64}, "on-policy loss")


def test_sample_loss_step_sample():
    """sample(..., state_every=4, gamma=, influence_weight=1) -> ppo_loss_moa on the batch -> backward -> one Adam step, against
    the same step from the torch loss; then the next sample() runs on the updated weights.  The horizon ends an episode inside
    the fragment."""
    E, N, steps, T, lr = 64, 5, 12, 4, 1e-2
    h = dict(clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1e-2, entropy_coeff=1e-3, kl_coeff=0.2)
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=7, seed=5)
    pol = make_policy(env.engine.num_actions, N, N, 64, seed=31, recur=2.0).to(DEV)
    twin = copy.deepcopy(pol)
    first = env.reset().clone()
    batch = env.sample(pol, steps, state_every=T, gamma=0.99, lambda_=0.95, influence_weight=1.0)
    ends = torch.nonzero(batch["done"][:steps - 1].flatten(1).any(1)).flatten().tolist()
    assert any((k + 1) % T for k in ends), ends                # an episode ends inside a window: the step after it starts from zero
    with torch.no_grad():                                      # the behaviour logits by a replay: sample() records logp only
        logits, _, _ = forward(pol, shifted_obs(batch["obs"], first, steps), batch["prev_actions"], batch["state"], batch["done"], T)
        logp = torch.log_softmax(logits, -1).gather(-1, batch["actions"].long().unsqueeze(-1)).squeeze(-1)
    # before the step the policy is the one that sampled: the ring, the done rule and the shift agree with what the rollout did
    assert float((torch.exp(logp - batch["logp"]) - 1).abs().max()) < 1e-4
    t = {"obs": batch["obs"], "actions": batch["actions"], "logp_old": batch["logp"], "advantages": batch["advantages"],
         "value_targets": batch["value_targets"], "vf_pred": batch["value"], "behaviour_logits": logits.contiguous(),
         "state": batch["state"], "done": batch["done"], "prev_actions": batch["prev_actions"]}
    opt = torch.optim.Adam(pol.parameters(), lr=lr, eps=1.0)   # eps = 1: |d step / d grad| <= lr
    opt_twin = torch.optim.Adam(twin.parameters(), lr=lr, eps=1.0)
    loss, stats = ppo_loss_moa(pol, dict(batch, logits=t["behaviour_logits"]), seq_len=T, moa_weight=MOA_WEIGHT, obs_first=first, **h)
    assert float(stats["kl"].abs().max()) < 1e-6, stats["kl"]  # the kernel's own logits are the rollout's
    opt.zero_grad()
    loss.backward()
    cpu_t = {k: v.cpu() for k, v in t.items()}
    _, _, g64 = autograd_loss(twin.cpu(), cpu_t, h, first.cpu(), T)
    twin = twin.to(DEV)
    _, _, g32 = autograd_loss(twin, cpu_t, h, first.cpu(), T, dtype=torch.float32, device=DEV)
    _check_against_reference(_grads(pol), g32, g64, "e2e grad")
    for name, _, _ in twin.layout():
        getattr(twin, name).grad = g32[name].clone()
    opt.step()
    opt_twin.step()
    for name, _, _ in pol.layout():
        et = max_err(g32[name], g64[name])
        scale = max(1.0, float(g64[name].abs().max()))
        bound = lr * (5 * et + 1e-6 * scale) + 2 ** -22 * float(getattr(twin, name).detach().abs().max())     # ek + et, and the update's rounding
        diff = max_err(getattr(pol, name), getattr(twin, name))
        print("step %-14s diff %.3e bound %.3e" % (name, diff, bound))
        assert diff <= bound, (name, diff, bound)
    nxt = env.sample(pol, steps, state_every=T, gamma=0.99, lambda_=0.95, influence_weight=1.0)
    torch.cuda.synchronize()
    assert torch.isfinite(nxt["advantages"]).all() and not torch.equal(batch["value"], nxt["value"])
