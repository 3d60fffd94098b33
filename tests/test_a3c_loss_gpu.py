"""a3c_loss, a3c_loss_recurrent and a3c_loss_moa on the MI355X (ssd_policy_ac_grad, ssd_policy_lstm_ac_grad,
ssd_policy_moa_ac_grad): the kernels' gradients, statistics and loss against the float64 restatement (a3c_ref.py) with torch's
own float32 autograd on the same device as the yardstick -- ek <= 4 et + 1e-6 max(1, max |ref|) per tensor --, the persistent
loops' second tiles, the split-K kernels' second chunk, exact sums (the loss is a sum over rows: nothing is divided), the
bound's power against four wrong losses, the MOA term's scale, bit-equal repeats on a scratch shared with the PPO calls, the
packed gradient, minibatch slices, and one clipped SGD step end to end from sample() per policy."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import ppo_lstm_ref
import ppo_moa_ref
import ppo_ref
from a3c_ref import (ACTIONS_BRANCH, CONV_MARGIN, COUNTING_HYPER, HYPER, MOA_BRANCH, MOA_WEIGHT, as_numpy_u32, autograd_loss, bound,
                     conv_margin, counting_inputs, make_inputs, make_policy, max_err, variants_of, zero_policy)
from sequential_social_dilemma_games_amd import (_capi, a3c_loss, a3c_loss_moa, a3c_loss_recurrent, clip_grad_by_set_norm, ppo_loss,
                                                 ppo_loss_moa, ppo_loss_recurrent)
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd.policy import A3C_STATS, MOA_A3C_STATS
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
KINDS = ("fc", "lstm", "moa")


@pytest.fixture(scope="module", autouse=True)
def rollout_before_the_first_stream():
    """The library sizes its pool of dispatch queues by a timed probe at the process's first rollout call and keeps the verdict
    (ssd_aql.hip, probe_pool_queue: a process that already runs four busy streams gets no queue of the library's, for good).  The
    caller's-stream cases below make torch create HIP streams; were they the first GPU work of the process -- this file is the
    first of the suite by name --, the rollouts of every later test would step on the caller's stream and the tests that assert
    the dispatch path would fail.  So one short rollout comes first, as in an application, which samples before it learns: of
    4096 envs, which the library steps as two chains, so that the pool's second queue is probed now as well."""
    from sequential_social_dilemma_games_amd.engine import VecEngine
    E = 4096
    eng = VecEngine(K.GAME_HARVEST, K.HARVEST_MAP, num_envs=E, num_agents=5, seed=1)
    eng.reset()
    obs = torch.zeros((2, E, 5, 15, 15, 3), dtype=torch.uint8, device=DEV)
    rew = torch.zeros((2, E, 5), dtype=torch.int32, device=DEV)
    eng.rollout_random(4, obs, rew, None, reset_every=0, step0=0)
    torch.cuda.synchronize()
    assert eng.status() == 0
    yield


def _stats_names(kind):
    return MOA_A3C_STATS if kind == "moa" else A3C_STATS


def _to_dev(t):
    return {k: v.to(DEV) for k, v in t.items()}


def _grads(pol):
    return {name: getattr(pol, name).grad.detach().clone() for name, _, _ in pol.layout()}


def _run(kind, pol, t, first, h, T, moa_weight=MOA_WEIGHT):
    """The kind's loss + backward on the device -> (loss, stats, {param: grad})."""
    pol.zero_grad()
    if kind == "fc":
        loss, stats = a3c_loss(pol, t, obs_first=first, **h)
    elif kind == "lstm":
        loss, stats = a3c_loss_recurrent(pol, t, seq_len=T, obs_first=first, **h)
    else:
        loss, stats = a3c_loss_moa(pol, t, seq_len=T, moa_weight=moa_weight, obs_first=first, **h)
    loss.backward()
    return loss.detach(), stats, _grads(pol)


def _check_against_reference(got, tor, ref, what, only=None):
    """ek <= 4 et + 1e-6 * max(1, max |ref|) for every tensor of the dicts; prints each figure before it asserts."""
    bad = []
    for name in ref:
        if only is not None and name not in only:
            continue
        ek, et = max_err(got[name], ref[name]), max_err(tor[name], ref[name])
        scale = max(1.0, float(ref[name].abs().max()))
        print("%s %-14s ek %.3e et %.3e ek/et %.2f max|ref| %.3e" % (what, name, ek, et, ek / et if et else float("inf"), scale))
        if not ek <= 4.0 * et + 1e-6 * scale:
            bad.append((name, ek, et))
    assert not bad, (what, bad)


def _equal_bits(kind, a, b):
    la, sa, ga = a
    lb, sb, gb = b
    assert np.array_equal(as_numpy_u32(la), as_numpy_u32(lb))
    for k in _stats_names(kind):
        assert np.array_equal(as_numpy_u32(sa[k]), as_numpy_u32(sb[k])), k
    for name in ga:
        assert np.array_equal(as_numpy_u32(ga[name]), as_numpy_u32(gb[name])), name


def compare_with_float64(kind, pol, t, first, T, h=HYPER, own_stream=False, ref_device="cpu", moa_weight=MOA_WEIGHT, before=None, only=None):
    """The kernels on (pol, t, first, h) against the float64 restatement with torch's float32 autograd on the device as the
    yardstick -- gradients, statistics and loss under the bound --, all outputs finite, and a second call bit-equal to the
    first.  before(g64, g32): a check on the references that must hold before the kernel is looked at."""
    P = pol.num_sets
    loss64, stats64, g64 = autograd_loss(kind, pol, t, h, first, T, moa_weight, device=ref_device)
    loss32, stats32, g32 = autograd_loss(kind, pol, t, h, first, T, moa_weight, dtype=torch.float32, device=DEV)
    if before is not None:
        before(g64, g32)
    dpol, dt, dfirst = copy.deepcopy(pol).to(DEV), _to_dev(t), None if first is None else first.to(DEV)
    if own_stream:
        s = torch.cuda.Stream(DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            out = _run(kind, dpol, dt, dfirst, h, T, moa_weight)
        s.synchronize()
    else:
        out = _run(kind, dpol, dt, dfirst, h, T, moa_weight)
    torch.cuda.synchronize()
    loss, stats, g = out
    names = _stats_names(kind)
    assert tuple(stats) == names and all(tuple(stats[k].shape) == (P,) and stats[k].dtype == torch.float64 for k in names)
    assert all(bool(torch.isfinite(x).all()) for x in list(g.values()) + list(stats.values()) + [loss])
    _check_against_reference(g, g32, g64, "grad", only)
    _check_against_reference(stats, stats32, stats64, "stat")
    _check_against_reference({"loss": loss}, {"loss": loss32}, {"loss": loss64}, "loss")
    out2 = _run(kind, dpol, dt, dfirst, h, T, moa_weight)
    torch.cuda.synchronize()
    _equal_bits(kind, out, out2)
    return out


def _input_conditions(kind, pol, t, first, device="cpu"):
    """What the PPO tests assert of these inputs and the A3C loss still depends on: the MOA fragments keep every conv
    pre-activation away from its ReLU's kink (the A3C loss itself has no kinks)."""
    if kind == "moa":
        m = float(conv_margin(pol, ppo_ref.shifted_obs(t["obs"], first, t["actions"].shape[0]), device).min())
        assert m >= CONV_MARGIN, m


# ---- the conv-FC policy: rows per set 1, 15, 16 and 17 of test_ppo_loss_gpu.py's CASES (the same seeds, so the same
# observations, actions, advantages and value targets) for P = N and P = 1, and its second-tile case P = N = 64, K = 257, E = 1:
# G = 16 with 17 tiles, so workgroup 0's second tile holds one live row.  (A, P, K, E, N, obs_first, own stream, seed)
FC_CASES = [(8, 5, 1, 1, 5, True, False, 1), (8, 5, 3, 5, 5, True, False, 2), (9, 5, 4, 4, 5, False, False, 3), (8, 5, 17, 1, 5, True, True, 4),
            (9, 1, 1, 1, 1, True, False, 7), (8, 1, 1, 3, 5, False, False, 8), (9, 1, 4, 2, 2, True, False, 9), (8, 1, 17, 1, 1, True, False, 10),
            (8, 64, 257, 1, 64, True, False, 18)]


@pytest.mark.parametrize("A,P,K_,E,N,use_first,own_stream,seed", FC_CASES)
def test_conv_fc_against_float64(A, P, K_, E, N, use_first, own_stream, seed):
    R = K_ * E * N // P
    if P == 64:
        assert _capi.SSD_PPO_GROUPS(R, P) == 16 and -(-R // 16) == 17 and R % 16 == 1
    pol = make_policy("fc", A, N, P, seed=seed)
    t, first = make_inputs("fc", pol, K_, E, N, None, seed=100 + seed, obs_first=use_first)
    print("case", (A, P, K_, E, N, use_first, own_stream, seed))
    compare_with_float64("fc", pol, t, first, None, own_stream=own_stream)


# ---- the recurrent and the MOA policy: (K, T) over one window, whole windows, a ragged last window, T > K and T = 1, with
# the done modes; then P = 1, C = 128, no obs_first, a caller's stream.  E = 17, N = 5, A = 8.
def case(K_=7, T=3, P=5, C_=64, first=True, done="none", stream=False, seed=1):
    return (K_, T, P, C_, first, done, stream, seed)


SEQ_CASES = [case(1, 1, seed=1), case(5, 5, done="mid", seed=2), case(7, 3, done="window_end", seed=3), case(4, 8, done="per_env", seed=4),
             case(6, 1, done="mid", seed=5), case(P=1, done="per_env", seed=10), case(C_=128, done="mid", seed=14),
             case(first=False, done="window_end", seed=16), case(stream=True, done="per_env", seed=23)]


@pytest.mark.parametrize("kind", ["lstm", "moa"])
@pytest.mark.parametrize("K_,T,P,C_,use_first,done,own_stream,seed", SEQ_CASES)
def test_sequences_against_float64(kind, K_, T, P, C_, use_first, done, own_stream, seed):
    E, N, A = 17, 5, 8
    pol = make_policy(kind, A, N, P, C_, seed=seed)
    t, first = make_inputs(kind, pol, K_, E, N, T, seed=100 + seed, obs_first=use_first, done_mode=done)
    _input_conditions(kind, pol, t, first)
    print("case", kind, (K_, T, P, C_, use_first, done, own_stream, seed))
    compare_with_float64(kind, pol, t, first, T, own_stream=own_stream)


@pytest.mark.parametrize("kind", ["lstm", "moa"])
def test_persistent_loop_takes_a_second_tile(kind):
    """16 G + 1 sequences per set, G the exported groups macro, so that workgroup 0 of every set takes a second tile with one
    live sequence: the recurrent policy at P = N = 64 (257 envs), the MOA policy at P = N = 16 (1025 envs); K = T = 2.  The
    shapes and input seeds of the PPO tests of the same name; the float64 restatement runs torch's float64 ops on the device."""
    P, seed = (64, 197) if kind == "lstm" else (16, 300)
    N = P
    groups = _capi.SSD_RPPO_GROUPS if kind == "lstm" else _capi.SSD_MPPO_GROUPS
    G = groups(10 ** 6, P)
    E = 16 * G + 1
    assert groups(E, P) == G and -(-E // 16) == G + 1
    pol = make_policy(kind, 8, N, P, 64, seed=30 + P)
    t, first = make_inputs(kind, pol, 2, E, N, 2, seed=seed, done_mode="per_env", device=DEV)
    _input_conditions(kind, pol, t, first, DEV)
    compare_with_float64(kind, pol, t, first, 2, ref_device=DEV)


@pytest.mark.parametrize("kind", ["lstm", "moa"])
def test_split_k_takes_a_second_chunk(kind):
    """SPLIT_SHAPES["A"] (K = 14, T = 13, E = 33, N = 5, P = 1) at C = 64: the first window holds 2145 rows of the set, 34
    chunks of 64 over 32 splits, the last chunk ragged; the second window 3 chunks, so most splits keep what the first left."""
    splits, chunk = _capi.SSD_RPPO_MAX_SPLITS, _capi.SSD_RPPO_CHUNK
    if kind == "lstm":
        pol, t, first, _, (K_, T, E, N, P), _ = ppo_lstm_ref.split_case("A", "ordinary", 64, splits, chunk)
    else:
        pol, t, first, (K_, T, E, N, P), _ = ppo_moa_ref.split_case("A", 64, splits, chunk)
    rows1, rows2 = T * (E * N // P), (K_ - T) * (E * N // P)
    assert (K_, T, E, N, P) == (14, 13, 33, 5, 1)
    assert _capi.SSD_RPPO_SPLITS(rows1) == splits == 32 and -(-rows1 // chunk) > splits and rows1 % chunk and 0 < -(-rows2 // chunk) < splits
    _input_conditions(kind, pol, t, first)
    compare_with_float64(kind, pol, t, first, T)


# ---- exact sums ----
# more tiles than workgroups: (kind, P, N, K, T, E)
EXACT_CASES = [("fc", 64, 64, 257, None, 1), ("fc", 32, 32, 3, None, 200), ("lstm", 64, 64, 2, 2, 257), ("moa", 16, 16, 2, 2, 1025)]


@pytest.mark.parametrize("kind,P,N,K_,T,E", EXACT_CASES)
def test_sums_are_exact_and_nothing_is_divided(kind, P, N, K_, T, E):
    """All parameters zero, adv = 0, vf_loss_coeff = 1, entropy_coeff = 0 (moa_weight = 0) and value_targets[flat row] = 1 + flat
    row mod 4093: value = 0, so vf_loss = 0.5 sum(vt^2) and d loss / d value_b = -sum(vt) per set, exact integers or halves, and
    every other gradient is exactly zero.  A kernel that divides by the rows, or skips or double-counts a tile, misses them."""
    A, C_ = 8, 64
    t, first = counting_inputs(kind, A, C_, K_, E, N, T, seed=40 + E)
    vt = t["value_targets"].double()
    per_set = (lambda x: x.reshape(-1, P).sum(0)) if P > 1 else (lambda x: x.sum().reshape(1))
    sum_vt, sum_sq = per_set(vt), per_set(vt * vt)
    # exactness is a property of the inputs: every partial sum is an integer (or a half) a float32 / float64 holds
    assert float(sum_vt.max()) < 2 ** 24 and float(sum_sq.max()) < 2 ** 53 and float((vt * vt).max()) < 2 ** 24
    assert bool((t["advantages"] == 0).all())
    R = K_ * E * N // P
    tiles = -(-(R if kind == "fc" else R // K_) // 16)
    G = _capi.SSD_PPO_GROUPS(R, P) if kind == "fc" else _capi.SSD_RPPO_GROUPS(R // K_, P)
    assert tiles > G, (tiles, G)
    pol = zero_policy(kind, A, N, P, C_).to(DEV)
    _, stats, g = _run(kind, pol, _to_dev(t), first.to(DEV), COUNTING_HYPER, T, moa_weight=0.0)
    torch.cuda.synchronize()
    assert np.array_equal(as_numpy_u32(g["value_b"].reshape(-1)), as_numpy_u32((-sum_vt).float()))
    assert np.array_equal(as_numpy_u32(stats["vf_loss"]), as_numpy_u32(0.5 * sum_sq))
    assert np.array_equal(as_numpy_u32(stats["total_loss"]), as_numpy_u32(0.5 * sum_sq))
    assert float(stats["policy_loss"].abs().max()) == 0.0
    assert float((stats["policy_entropy"] / R - np.log(8.0)).abs().max()) < 1e-6
    for name in g:
        if name != "value_b":
            assert float(g[name].abs().max()) == 0.0, name


# ---- would the bound notice a wrong loss? ----
@pytest.mark.parametrize("kind", KINDS)
def test_bound_separates_the_loss_from_wrong_ones(kind):
    """For each wrong variant of the restatement (the A3C terms as means, the MOA term as a sum, the value term without its
    half, the advantage's sign flipped), its float64 gradient is off from the true one by 100 bounds or more in some tensor --
    asserted before the kernel is compared; then the kernel passes the bound."""
    K_, T, E, N, P, A = 7, 3, 17, 5, 5, 8
    pol = make_policy(kind, A, N, P, 64, seed=41)
    t, first = make_inputs(kind, pol, K_, E, N, T, seed=141, done_mode="per_env")
    _input_conditions(kind, pol, t, first)

    def before(g64, g32):
        bounds = {name: bound(g64[name], max_err(g32[name], g64[name])) for name in g64}
        for variant in variants_of(kind):
            _, _, gv = autograd_loss(kind, pol, t, HYPER, first, T, variant=variant)
            ratios = {name: max_err(gv[name], g64[name]) / bounds[name] for name in g64}
            worst = max(ratios, key=ratios.get)
            print("variant %-10s off by %.1f bounds in %s" % (variant, ratios[worst], worst))
            assert ratios[worst] >= 100.0, (variant, ratios)
    compare_with_float64(kind, pol, t, first, T, before=before)


# ---- the MOA term ----
def _moa_case():
    K_, T, E, N = 7, 3, 17, 5
    pol = make_policy("moa", 8, N, N, 64, seed=75)
    t, first = make_inputs("moa", pol, K_, E, N, T, seed=76, done_mode="per_env")
    _input_conditions("moa", pol, t, first)
    return pol, t, first, T


def test_moa_term_alone():
    """adv = 0 and vf_loss_coeff = entropy_coeff = 0 with moa_weight = 10: the loss is the MOA term alone, so the gradients of the
    actions branch less the conv are exactly zero, and the MOA branch and the conv -- which carry moa_weight / ((N - 1) rows),
    the scale folded into dpred -- match the restatement under the bound."""
    pol, t, first, T = _moa_case()
    t = dict(t, advantages=torch.zeros_like(t["advantages"]))
    h = dict(vf_loss_coeff=0.0, entropy_coeff=0.0)
    _, _, g = compare_with_float64("moa", pol, t, first, T, h=h, moa_weight=10.0, only=MOA_BRANCH + ("conv_w", "conv_b"))
    for name in ACTIONS_BRANCH:
        assert float(g[name].abs().max()) == 0.0, name
    for name in MOA_BRANCH + ("conv_w", "conv_b"):
        assert float(g[name].abs().max()) > 0.0, name


def test_moa_weight_zero():
    """moa_weight = 0: exact zeros on the MOA branch, the bits of the weighted call's actions branch, a total_loss without the
    MOA term and the same moa_loss."""
    pol, t, first, T = _moa_case()
    pol, t, first = pol.to(DEV), _to_dev(t), first.to(DEV)
    _, s1, g1 = _run("moa", pol, t, first, HYPER, T)
    _, s0, g0 = _run("moa", pol, t, first, HYPER, T, moa_weight=0.0)
    torch.cuda.synchronize()
    for name in MOA_BRANCH:
        assert float(g0[name].abs().max()) == 0.0 and float(g1[name].abs().max()) > 0.0, name
    for name in ACTIONS_BRANCH:
        assert np.array_equal(as_numpy_u32(g0[name]), as_numpy_u32(g1[name])), name
    for k in MOA_A3C_STATS[1:]:
        assert np.array_equal(as_numpy_u32(s0[k]), as_numpy_u32(s1[k])), k
    assert float((s1["total_loss"] - s0["total_loss"] - MOA_WEIGHT * s1["moa_loss"]).abs().max()) < 1e-9


# ---- repeats, the scratch, the packed gradient, minibatches ----
def _ppo_call(kind, pol, t, first, T):
    h = ppo_ref.HYPER
    if kind == "fc":
        return ppo_loss(pol, t, obs_first=first, **h)
    if kind == "lstm":
        return ppo_loss_recurrent(pol, t, seq_len=T, obs_first=first, **h)
    return ppo_loss_moa(pol, t, seq_len=T, moa_weight=MOA_WEIGHT, obs_first=first, **h)


@pytest.mark.parametrize("kind", KINDS)
def test_repeats_and_a_scratch_grown_by_a_ppo_call_give_the_same_bits(kind):
    """One buffer on the policy serves its PPO and A3C calls: after a larger PPO call has grown it (and with NaN written over
    it) the A3C call returns the bits of its first run, and those of a fresh policy."""
    mod = {"fc": ppo_ref, "lstm": ppo_lstm_ref, "moa": ppo_moa_ref}[kind]
    pol = make_policy(kind, 8, 5, 5, 64, seed=60)
    t, first = make_inputs(kind, pol, 7, 17, 5, 3, seed=61, done_mode="per_env")
    big, big_first = mod.make_inputs(pol, 9, 40, 5, seed=62) if kind == "fc" else mod.make_inputs(pol, 9, 40, 5, 4, seed=62)
    pol, t, first = pol.to(DEV), _to_dev(t), first.to(DEV)
    fresh = copy.deepcopy(pol)
    a = _run(kind, pol, t, first, HYPER, 3)
    small = pol._ppo_scratch.numel()
    _ppo_call(kind, pol, _to_dev(big), big_first.to(DEV), 4)[0].backward()
    grown = pol._ppo_scratch.numel()
    assert grown > small
    pol._ppo_scratch.fill_(float("nan"))                       # whatever an earlier call left there is never read
    b = _run(kind, pol, t, first, HYPER, 3)
    assert pol._ppo_scratch.numel() == grown
    c = _run(kind, fresh, t, first, HYPER, 3)
    torch.cuda.synchronize()
    _equal_bits(kind, a, b)
    _equal_bits(kind, a, c)


def _packed_call(kind, pol, t, first, K_, E, N, T):
    """The C call itself on a NaN-filled gradient buffer -> packed [P, set_floats]."""
    P, A = pol.num_sets, pol.num_actions
    packed = torch.full((P, pol.set_floats), float("nan"), dtype=torch.float32, device=DEV)
    stats = torch.zeros((P, len(_stats_names(kind))), dtype=torch.float64, device=DEV)
    shape = pol.ppo_scratch_shape(K_ * E * N // P) if kind == "fc" else pol.ppo_scratch_shape(K_, E, N, T)
    scratch = torch.empty(shape, dtype=torch.float32, device=DEV)
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())   # noqa: E731
    rows = (ptr(t["actions"]), ptr(t["advantages"]), ptr(t["value_targets"]), K_, E, N)
    tail = (ptr(scratch), ptr(packed), ptr(stats), 0, 0, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    hv = (HYPER["vf_loss_coeff"], HYPER["entropy_coeff"])
    L = _capi.lib()
    if kind == "fc":
        rc = L.ssd_policy_ac_grad(ptr(pol.packed()), P, A, ptr(first), ptr(t["obs"]), *rows, *hv, *tail)
    elif kind == "lstm":
        rc = L.ssd_policy_lstm_ac_grad(ptr(pol.packed()), P, A, pol.cell_size, T, ptr(first), ptr(t["obs"]), ptr(t["state"]),
                                       ptr(t.get("done")), *rows, *hv, *tail)
    else:
        rc = L.ssd_policy_moa_ac_grad(ptr(pol.packed()), P, A, pol.cell_size, T, ptr(first), ptr(t["obs"]), ptr(t["state"]),
                                      ptr(t["prev_actions"]), ptr(t.get("done")), *rows, *hv, MOA_WEIGHT, *tail)
    _capi.policy_check(rc)
    torch.cuda.synchronize()
    return packed


@pytest.mark.parametrize("kind", KINDS)
def test_packed_gradient_padding_scaling_and_minibatch(kind):
    """The library's packed gradient has zero padding floats and holds what backward scatters; backward multiplies by the
    incoming gradient; a minibatch addressed by the documented slices equals the same rows gathered explicitly."""
    A, N, K_, E, T = 9, 5, 5, 7, 2
    pol = make_policy(kind, A, N, N, 64, seed=90)
    t, first = make_inputs(kind, pol, K_, E, N, T, seed=91, done_mode="mid")
    pol, t, first = pol.to(DEV), _to_dev(t), first.to(DEV)
    _, _, g = _run(kind, pol, t, first, HYPER, T)
    packed = _packed_call(kind, pol, t, first, K_, E, N, T)
    used = torch.zeros(pol.set_floats, dtype=torch.bool, device=DEV)
    for name, shape, off in pol.layout():
        n = int(np.prod(shape))
        used[off:off + n] = True
        assert torch.equal(packed[:, off:off + n].reshape(g[name].shape), g[name]), name
    assert int((~used).sum()) > 0 and float(packed[:, ~used].abs().max()) == 0.0
    pol.zero_grad()
    if kind == "fc":
        loss, _ = a3c_loss(pol, t, obs_first=first, **HYPER)
    elif kind == "lstm":
        loss, _ = a3c_loss_recurrent(pol, t, seq_len=T, obs_first=first, **HYPER)
    else:
        loss, _ = a3c_loss_moa(pol, t, seq_len=T, moa_weight=MOA_WEIGHT, obs_first=first, **HYPER)
    (loss * 3.0).backward()
    for name in g:
        assert torch.equal(getattr(pol, name).grad, g[name] * 3.0), name
    # steps 2 .. 4 (k0 = 2 = T): the slices [2:] of the per-row tensors, the ring from slot 1 and obs_first = obs[1]
    mb = {k: v[2:] for k, v in t.items() if k != "state"}
    explicit = dict({k: v.clone() for k, v in mb.items()}, obs=t["obs"][1:4].clone())
    if kind != "fc":
        mb["state"], explicit["state"] = t["state"][1:], t["state"][1:].clone()
    a = _run(kind, pol, mb, t["obs"][1], HYPER, T)
    b = _run(kind, pol, explicit, None, HYPER, T)
    torch.cuda.synchronize()
    _equal_bits(kind, a, b)


# ---- end to end ----
@pytest.mark.parametrize("kind", KINDS)
def test_sample_loss_clip_step_sample(kind):
    """sample(..., gamma=0.99, use_gae=False) -> the A3C loss on the batch -> backward -> clip_grad_by_set_norm -> one SGD step,
    against the same step from torch's float32 autograd of the restatement under the bound test_sample_loss_step_sample uses
    (lr (ek + et) and the update's rounding); then the next sample() runs on the updated weights.  max_norm lies above every
    set's norm (asserted on the float64 gradient), so the clip's factor is exactly 1 and the bound on the gradients carries
    over to the step; test_a3c_loss_cpu.py checks the clip itself on both sides of max_norm."""
    E, N, steps, T, lr = 64, 5, 12, 4, 1e-4
    h = dict(vf_loss_coeff=0.5, entropy_coeff=0.01)
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=7, seed=5)
    A = env.engine.num_actions
    pol = (make_policy(kind, A, N, N, 64, seed=31) if kind == "fc" else make_policy(kind, A, N, N, 64, seed=31, recur=2.0)).to(DEV)
    twin = copy.deepcopy(pol)
    first = env.reset().clone()
    kw = {} if kind == "fc" else {"state_every": T}
    batch = env.sample(pol, steps, gamma=0.99, use_gae=False, **kw)
    loss, stats = (a3c_loss(pol, batch, obs_first=first, **h) if kind == "fc" else
                   a3c_loss_recurrent(pol, batch, seq_len=T, obs_first=first, **h) if kind == "lstm" else
                   a3c_loss_moa(pol, batch, seq_len=T, moa_weight=MOA_WEIGHT, obs_first=first, **h))
    pol.zero_grad()
    loss.backward()
    cpu_t = {k: v.cpu() for k, v in batch.items() if isinstance(v, torch.Tensor)}
    _, _, g64 = autograd_loss(kind, twin.cpu(), cpu_t, h, first.cpu(), T)
    twin = twin.to(DEV)
    _, _, g32 = autograd_loss(kind, twin, cpu_t, h, first.cpu(), T, dtype=torch.float32, device=DEV)
    _check_against_reference(_grads(pol), g32, g64, "e2e grad")
    norm64 = torch.sqrt(sum(g.double().reshape(N, -1).square().sum(1) for g in g64.values()))
    max_norm = 2.0 * float(norm64.max())
    for name, _, _ in twin.layout():
        getattr(twin, name).grad = g32[name].clone()
    norms = clip_grad_by_set_norm(pol, max_norm)
    clip_grad_by_set_norm(twin, max_norm)
    assert tuple(norms.shape) == (N,) and bool(torch.isfinite(norms).all())
    assert float((norms.double().cpu() / norm64 - 1).abs().max()) < 1e-3
    opt, opt_twin = torch.optim.SGD(pol.parameters(), lr=lr), torch.optim.SGD(twin.parameters(), lr=lr)
    opt.step()
    opt_twin.step()
    for name, _, _ in pol.layout():
        et = max_err(g32[name], g64[name])
        scale = max(1.0, float(g64[name].abs().max()))
        limit = lr * (5 * et + 1e-6 * scale) + 2 ** -22 * float(getattr(twin, name).detach().abs().max())     # ek + et, and the update's rounding
        diff = max_err(getattr(pol, name), getattr(twin, name))
        print("step %-14s diff %.3e bound %.3e" % (name, diff, limit))
        assert bool(torch.isfinite(getattr(pol, name)).all()) and diff <= limit, (name, diff, limit)
    nxt = env.sample(pol, steps, gamma=0.99, use_gae=False, **kw)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(nxt[k]).all()) for k in ("advantages", "value_targets", "value"))
    assert not torch.equal(batch["value"], nxt["value"])
