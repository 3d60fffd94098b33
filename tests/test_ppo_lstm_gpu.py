"""ppo_loss_recurrent on the MI355X (csrc/ssd_policy_lstm_grad.hip, ssd_policy_lstm_ppo_grad): the kernels' gradients and
statistics against the float64 restatement (ppo_lstm_ref.py) with torch's own float32 autograd on the same device as the
yardstick, the persistent tile loop, the split-K kernel's
second chunks (windows of more than 32 chunks of one set's rows: the second pass over the accumulators, a ragged last chunk that
is a second chunk, splits that get no chunk of the second window, rows >= 2048; spotlight inputs make a single row count), exact
row accounting, exact zeros where no gradient may flow, bit-equal repeats, set
isolation, the kink rules, rows exactly on policy (the clip range does not show, policy_loss = -1 and kl = 0 exactly), and one
optimiser step end to end from sample()."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from ppo_lstm_ref import (HYPER, MARGIN, as_numpy_u32, autograd_loss, branch_report, clipped_rows, counting_inputs, forward, make_inputs,
                          make_policy, max_err, set_fragment, set_policy, shifted_obs, split_case, zero_policy)
from ppo_ref import COUNTING_HYPER, LOOSE, on_policy_checks
from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd import evaluate_fragment, ppo_loss_recurrent
from sequential_social_dilemma_games_amd.policy import PPO_STATS
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# The factor of `ek <= FACTOR * et + 1e-6 * max(1, max |ref|)` per parameter tensor (DESIGN.md section 17 records the measured
# ek / et): the project's margin, 4, for every tensor.
FACTOR = {}


def case(K_=7, T=3, E=17, N=5, P=5, A=8, C_=64, beh=True, first=True, done="none", stream=False, seed=1):
    return (K_, T, E, N, P, A, C_, beh, first, done, stream, seed)


# each line varies one thing from (K, T) = (7, 3), 17 sequences per set, C = 64, N = P = 5, A = 8
CASES = [case(1, 1, seed=1), case(5, 5, seed=2), case(7, 3, seed=3), case(4, 8, seed=4), case(6, 1, seed=5),             # (K, T)
         case(E=1, seed=6), case(E=15, seed=7), case(E=16, seed=8), case(E=33, seed=9),                                  # sequences per set
         case(E=7, P=1, seed=10), case(N=1, P=1, seed=11),                                                               # P = 1
         case(A=1, seed=12), case(A=15, seed=13),
         case(C_=128, seed=14), case(3, 3, E=16, C_=256, seed=15),
         case(first=False, seed=16), case(beh=False, seed=17),
         case(done="mid", seed=18), case(done="window_end", seed=19), case(done="last", seed=20), case(done="per_env", seed=21),
         case(5, 5, done="mid", seed=22), case(stream=True, done="per_env", seed=23)]


def _to_dev(t):
    return {k: v.to(DEV) for k, v in t.items()}


def _grads(pol):
    return {name: getattr(pol, name).grad.detach().clone() for name, _, _ in pol.layout()}


def _run(pol, t, first, h, T):
    """ppo_loss_recurrent + backward on the device -> (loss, stats, {param: grad})."""
    pol.zero_grad()
    loss, stats = ppo_loss_recurrent(pol, t, seq_len=T, obs_first=first, **h)
    loss.backward()
    return loss.detach(), stats, _grads(pol)


def _check_against_reference(got, tor, ref, what):
    """ek <= factor * et + 1e-6 * max(1, max |ref|) for every tensor of the dicts; prints each figure before it asserts."""
    bad = []
    for name in ref:
        ek, et = max_err(got[name], ref[name]), max_err(tor[name], ref[name])
        scale = max(1.0, float(ref[name].abs().max()))
        print("%s %-10s ek %.3e et %.3e ek/et %.2f max|ref| %.3e" % (what, name, ek, et, ek / et if et else float("inf"), scale))
        if not ek <= FACTOR.get(name, 4.0) * et + 1e-6 * scale:
            bad.append((name, ek, et))
    assert not bad, (what, bad)


def _equal_bits(a, b):
    la, sa, ga = a
    lb, sb, gb = b
    assert np.array_equal(as_numpy_u32(la), as_numpy_u32(lb))
    for k in PPO_STATS:
        assert np.array_equal(as_numpy_u32(sa[k]), as_numpy_u32(sb[k])), k
    for name in ga:
        assert np.array_equal(as_numpy_u32(ga[name]), as_numpy_u32(gb[name])), name


def compare_with_float64(pol, t, first, h, T, own_stream=False):
    """The kernels on (pol, t, first, h) against the float64 restatement with torch's float32 autograd on the device as the
    yardstick -- gradients, statistics and loss under the bound --, all outputs finite, and a second call bit-equal to the
    first."""
    P = pol.num_sets
    loss64, stats64, g64 = autograd_loss(pol, t, h, first, T)
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
    assert all(tuple(stats[k].shape) == (P,) and stats[k].dtype == torch.float64 for k in PPO_STATS)
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
    pol = make_policy(A, P, C_, seed=seed)
    t, first = make_inputs(pol, K_, E, N, T, seed=100 + seed, obs_first=use_first, behaviour=beh, done_mode=done)
    rep = branch_report(pol, t, h, first, T)
    print("case", (K_, T, E, N, P, A, C_, beh, use_first, done, own_stream), rep)
    assert rep["margin"] > MARGIN, rep
    if K_ * E * N >= 1000:
        # the case of 1155 rows (E = 33, seed 9), found on the CPU: clipped_pos 0.251, clipped_neg 0.263, open_pos 0.230,
        # open_neg 0.255, vf_dead 0.300, vf_clipped_live 0.204 of the rows
        for k in ("clipped_pos", "clipped_neg", "open_pos", "open_neg", "vf_dead", "vf_live", "vf_clipped_live"):
            assert rep[k] > 0.2, rep
    compare_with_float64(pol, t, first, h, T, own_stream)


def _multi_tile_shape(P):
    """Sequences per set = 16 G + 1: workgroup 0 of every set takes a second tile, with one live sequence."""
    G = _capi.SSD_RPPO_GROUPS(10 ** 6, P)
    seqs = 16 * G + 1
    assert _capi.SSD_RPPO_GROUPS(seqs, P) == G and -(-seqs // 16) == G + 1
    return seqs


def test_persistent_loop_takes_a_second_tile():
    """More tiles than workgroups at P = N = 64: 16 G + 1 sequences per set (G the exported groups macro: 16, so 257 envs),
    K = T = 2.  The input seed is chosen on the CPU for its margin (3.1e-4; of the seeds 194 .. 197 only 197 clears 1e-4: with
    33 000 rows some row's vf1 - vf2 is usually closer); every surrogate case and vf branch holds 20 % of the rows or more.
    The P = 1 twin sized the same way (1024 groups, 16 385 sequences; input seed 200: margin 3.8e-4 on the CPU) passes under
    the same bound but is left out for its time, measured once on the MI355X with the float64 restatement on the device: 9.1 s,
    of which the restatement is 1.6 s and make_inputs and branch_report 1.1 s; 9.4 s are the yardstick's, torch's float32
    autograd on the device, on its first call with a batch of 32 770 images in one conv group (0.01 s on a second call in the
    same process; the cost is the conv's first use at that shape, not arithmetic, and the yardstick is not to be swapped)."""
    P = N = 64
    seqs = _multi_tile_shape(P)
    E = seqs * P // N
    pol = make_policy(8, P, 64, seed=30 + P)
    t, first = make_inputs(pol, 2, E, N, 2, seed=197, done_mode="per_env")
    rep = branch_report(pol, t, HYPER, first, 2)
    print("multi-tile", (P, N, E), rep)
    assert rep["margin"] > MARGIN, rep
    for k in ("clipped_pos", "clipped_neg", "open_pos", "open_neg", "vf_dead", "vf_live", "vf_clipped_live"):
        assert rep[k] > 0.2, rep
    compare_with_float64(pol, t, first, HYPER, 2)


def test_inputs_do_not_depend_on_where_the_float64_forward_runs():
    """make_inputs draws every random number on the CPU and rounds what it takes from the float64 forward to float32: the
    fragment is the same to the bit with that forward on the device, and branch_report's figures agree."""
    pol = make_policy(8, 5, 64, seed=21)
    t, first = make_inputs(pol, 7, 17, 5, 3, seed=121, done_mode="per_env")
    td, firstd = make_inputs(pol, 7, 17, 5, 3, seed=121, done_mode="per_env", device=DEV)
    assert t.keys() == td.keys() and torch.equal(first, firstd)
    for k in t:
        assert td[k].device.type == "cpu" and td[k].dtype == t[k].dtype and torch.equal(t[k], td[k]), k
    rep, repd = branch_report(pol, t, HYPER, first, 3), branch_report(pol, t, HYPER, first, 3, device=DEV)
    assert all(abs(rep[k] - repd[k]) <= 1e-12 for k in rep), (rep, repd)


# (shape of ppo_lstm_ref.SPLIT_SHAPES, inputs, C).  Ordinary inputs catch a whole chunk lost or doubled, spotlight inputs a
# single row (test_ppo_lstm_cpu.py measures by how much); C = 128, the workload's cell size, changes the accumulator tiles per
# lane and the column blocks.
SPLIT_CASES = [("A", "ordinary", 64), ("A", "spotlight", 64), ("A", "spotlight", 128), ("B", "ordinary", 64), ("B", "spotlight", 64)]


@pytest.mark.parametrize("shape,inputs,C_", SPLIT_CASES)
def test_split_k_takes_a_second_chunk(shape, inputs, C_):
    """ssd_bptt_dw_kernel's `chunk += S`: the first window holds more than SSD_RPPO_MAX_SPLITS chunks of a set's rows (A: P = 1,
    2145 rows, 34 chunks, the last of 33 rows; B: P = N = 2, 2080 rows a set, 33 chunks, the last of 32 rows), the second window
    fewer chunks than splits (3 and 2), so most splits must keep what the first left."""
    splits, chunk = _capi.SSD_RPPO_MAX_SPLITS, _capi.SSD_RPPO_CHUNK
    pol, t, first, h, (K_, T, E, N, P), _ = split_case(shape, inputs, C_, splits, chunk)
    rows1, rows2 = T * (E * N // P), (K_ - T) * (E * N // P)
    assert _capi.SSD_RPPO_SPLITS(rows1) == splits == 32 and -(-rows1 // chunk) > splits and rows1 % chunk
    assert 0 < -(-rows2 // chunk) < splits
    rep = branch_report(pol, t, h, first, T)
    print("split", (shape, inputs, C_), rep)
    assert rep["margin"] > MARGIN, rep
    if inputs == "ordinary":
        for k in ("clipped_pos", "clipped_neg", "open_pos", "open_neg", "vf_dead", "vf_live", "vf_clipped_live"):
            assert rep[k] > 0.2, rep
    compare_with_float64(pol, t, first, h, T)


@pytest.mark.parametrize("P,N,E", [(5, 5, 1), (5, 5, 16), (5, 5, 17), (5, 5, 33), (1, 5, 1), (1, 5, 16), (1, 5, 17), (1, 5, 33),
                                   (64, 64, 257)])
def test_every_row_is_counted_exactly_once(P, N, E):
    """All parameters zero, adv = 0, vf_pred = 0, vf_loss_coeff = 0.5 and value_targets[flat row] = 1 + flat row mod 4093: z = 0,
    c' = h' = 0 from a zero ring and value = 0, so d loss / d value_b = -sum(vt) / R, vf_loss = sum(vt^2) / R, both exact, and
    every other gradient is exactly zero.  E counts envs: E or E N sequences per set."""
    A, C_ = 8, 64
    K_, T = (2, 2) if P == 64 else (7, 3)
    pol = zero_policy(A, P, C_).to(DEV)
    t, first = counting_inputs(A, C_, K_, E, N, T, seed=40 + E)
    _, stats, g = _run(pol, _to_dev(t), first.to(DEV), COUNTING_HYPER, T)
    torch.cuda.synchronize()
    vt = t["value_targets"].double()
    R = K_ * E * N // P
    per_set = (lambda x: x.reshape(-1, P).sum(0)) if P > 1 else (lambda x: x.sum().reshape(1))
    want_b = (-per_set(vt) / R).float()
    assert np.array_equal(as_numpy_u32(g["value_b"].reshape(-1)), as_numpy_u32(want_b))
    want_vf = per_set(vt * vt) / R
    assert np.array_equal(as_numpy_u32(stats["vf_loss"]), as_numpy_u32(want_vf))
    assert np.array_equal(as_numpy_u32(stats["total_loss"]), as_numpy_u32((0.5 * per_set(vt * vt)) / R))
    for name in g:
        if name != "value_b":
            assert float(g[name].abs().max()) == 0.0, name


@pytest.mark.parametrize("T,all_done", [(1, False), (3, True)])
def test_no_gradient_without_a_past(T, all_done):
    """With a zero ring and T = 1, or done set on every row, no step has an h to read: the h rows of lstm_w.grad (32 .. 32 + C
    - 1) are exactly zero, the x rows of every set are not.  (Single x rows are zero in the float64 reference too: a feature whose
    ReLU is dead on every row; and with no past c_prev = 0 zeroes the forget gate's columns.  So the x rows are asked for as a
    block per set.)"""
    pol = make_policy(8, 5, 64, seed=50)
    t, first = make_inputs(pol, 6, 17, 5, T, seed=51, zero_ring=True, done_mode="all" if all_done else "none")
    _, _, g = _run(pol.to(DEV), _to_dev(t), first.to(DEV), HYPER, T)
    torch.cuda.synchronize()
    assert float(g["lstm_w"][:, 32:].abs().max()) == 0.0
    assert float(g["lstm_w"][:, :32].abs().amax((1, 2)).min()) > 0.0
    assert float(g["fc1_w"].abs().max()) > 0.0


def test_repeats_and_a_grown_scratch_give_the_same_bits():
    pol = make_policy(8, 5, 64, seed=60)
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
    """At P = N = 5, set p's gradient is that of a P = 1, N = 1 call on that set's sequences, to the bit: the group counts of
    both calls agree, so every sum has the same order."""
    E, N, K_, T = 17, 5, 7, 3
    pol = make_policy(8, N, 64, seed=70)
    t, first = make_inputs(pol, K_, E, N, T, seed=71, done_mode="per_env")
    assert _capi.SSD_RPPO_GROUPS(E, N) == _capi.SSD_RPPO_GROUPS(E, 1)
    assert _capi.SSD_PPO_GROUPS(T * E, N) == _capi.SSD_PPO_GROUPS(T * E, 1)
    _, stats, g = _run(copy.deepcopy(pol).to(DEV), _to_dev(t), first.to(DEV), HYPER, T)
    for p in (0, 3):
        one = set_policy(pol, p).to(DEV)
        _, s1, g1 = _run(one, _to_dev(set_fragment(t, first, p)), None, HYPER, T)
        torch.cuda.synchronize()
        for name in g1:
            assert np.array_equal(as_numpy_u32(g[name][p:p + 1]), as_numpy_u32(g1[name])), (p, name)
        for k in PPO_STATS:
            assert np.array_equal(as_numpy_u32(stats[k][p:p + 1]), as_numpy_u32(s1[k])), (p, k)


def test_clipped_and_dead_rows_give_exactly_zero():
    """The kink rules: a fragment whose rows are all clipped (ratio 1.5, adv 1) and dead (vf2 > vf1 beyond the clip) gives an
    exactly zero gradient in every tensor, with entropy_coeff = kl_coeff = 0."""
    T = 3
    pol = make_policy(8, 5, 64, seed=80)
    t, first = make_inputs(pol, 7, 17, 5, T, seed=81, behaviour=False, done_mode="per_env")
    t = dict(t, **clipped_rows(pol, t, first, T))
    h = dict(HYPER, entropy_coeff=0.0, kl_coeff=0.0)
    loss, stats, g = _run(pol.to(DEV), _to_dev(t), first.to(DEV), h, T)
    torch.cuda.synchronize()
    assert abs(float(stats["policy_loss"].mean()) + 1.3) < 1e-4 and abs(float(stats["vf_loss"].mean()) - 0.64) < 1e-3
    for name in g:
        assert float(g[name].abs().max()) == 0.0, name


def test_packed_gradient_padding_and_scaling():
    """The library's packed gradient has zero padding floats and holds what backward scatters; backward multiplies by the
    incoming gradient."""
    A, N, K_, E, T = 9, 5, 5, 7, 2
    pol = make_policy(A, N, 64, seed=90)
    t, first = make_inputs(pol, K_, E, N, T, seed=91, done_mode="mid")
    pol, t, first = pol.to(DEV), _to_dev(t), first.to(DEV)
    _, _, g = _run(pol, t, first, HYPER, T)
    S = pol.set_floats
    packed = torch.full((N, S), float("nan"), dtype=torch.float32, device=DEV)
    stats = torch.zeros((N, 5), dtype=torch.float64, device=DEV)
    scratch = torch.empty(pol.ppo_scratch_shape(K_, E, N, T), dtype=torch.float32, device=DEV)
    ptr = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
    hv = [HYPER[k] for k in ("clip_param", "vf_clip_param", "vf_loss_coeff", "entropy_coeff", "kl_coeff")]
    _capi.policy_check(_capi.lib().ssd_policy_lstm_ppo_grad(
        ptr(pol.packed()), N, A, 64, T, ptr(first), ptr(t["obs"]), ptr(t["state"]), ptr(t["done"]), ptr(t["actions"]),
        ptr(t["logp_old"]), ptr(t["advantages"]), ptr(t["value_targets"]), ptr(t["vf_pred"]), ptr(t["behaviour_logits"]), K_, E, N, *hv,
        ptr(scratch), ptr(packed), ptr(stats), 0, 0, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
    torch.cuda.synchronize()
    used = torch.zeros(S, dtype=torch.bool, device=DEV)
    for name, shape, off in pol.layout():
        n = int(np.prod(shape))
        used[off:off + n] = True
        assert torch.equal(packed[:, off:off + n].reshape(g[name].shape), g[name]), name
    assert int((~used).sum()) > 0 and float(packed[:, ~used].abs().max()) == 0.0
    pol.zero_grad()
    loss, _ = ppo_loss_recurrent(pol, t, seq_len=T, obs_first=first, **HYPER)
    (loss * 3.0).backward()
    for name in g:
        assert torch.equal(getattr(pol, name).grad, g[name] * 3.0), name
    # a minibatch addressed by slices: steps 2 .. 4 with the ring from slot 1 and obs_first = obs[1]
    mb = {k: v[2:] for k, v in t.items() if k != "state"}
    a = _run(pol, dict(mb, state=t["state"][1:]), t["obs"][1], HYPER, T)
    b = _run(pol, dict(mb, state=t["state"][1:].clone(), obs=t["obs"][1:4].clone()), None, HYPER, T)
    _equal_bits(a, b)


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
    pol = make_policy(env.engine.num_actions, N, 64, seed=31, recur=2.0).to(DEV)
    first = env.reset().clone()
    batch = env.sample(pol, steps, state_every=T, gamma=0.99, lambda_=0.95)
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
    loss, stats, g = on_policy_checks(call, PPO_STATS, "recurrent")
    t = {"obs": batch["obs"], "actions": batch["actions"], "logp_old": batch["logp"], "advantages": batch["advantages"],
         "value_targets": batch["value_targets"], "vf_pred": batch["value"], "behaviour_logits": logits.contiguous(),
         "state": batch["state"], "done": batch["done"]}
    cpu_t = {k: v.cpu() for k, v in t.items()}
    hl = dict(h, **LOOSE)
    loss64, stats64, g64 = autograd_loss(copy.deepcopy(pol).cpu(), cpu_t, hl, first.cpu(), T)
    loss32, stats32, g32 = autograd_loss(pol, cpu_t, hl, first.cpu(), T, dtype=torch.float32, device=DEV)
    _check_against_reference(g, g32, g64, "on-policy grad")
    _check_against_reference(stats, stats32, stats64, "on-policy stat")
    _check_against_reference({"loss": loss}, {"loss": loss32}, {"loss": loss64}, "on-policy loss")


def test_sample_loss_step_sample():
    """sample(..., state_every=4, gamma=) -> ppo_loss_recurrent on the batch -> backward -> one Adam step, against the same step
    from the torch loss; then the next sample() runs on the updated weights.  The horizon ends an episode inside the
    fragment."""
    E, N, steps, T, lr = 64, 5, 12, 4, 1e-2
    h = dict(clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1e-2, entropy_coeff=1e-3, kl_coeff=0.2)
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=7, seed=5)
    pol = make_policy(env.engine.num_actions, N, 64, seed=31, recur=2.0).to(DEV)
    twin = copy.deepcopy(pol)
    first = env.reset().clone()
    batch = env.sample(pol, steps, state_every=T, gamma=0.99, lambda_=0.95)
    ends = torch.nonzero(batch["done"][:steps - 1].flatten(1).any(1)).flatten().tolist()
    assert any((k + 1) % T for k in ends), ends                # an episode ends inside a window: the step after it starts from zero
    with torch.no_grad():                                      # the behaviour logits by a replay: sample() records logp only
        logits, _ = forward(pol, shifted_obs(batch["obs"], first, steps), batch["state"], batch["done"], T)
        logp = torch.log_softmax(logits, -1).gather(-1, batch["actions"].long().unsqueeze(-1)).squeeze(-1)
    # before the step the policy is the one that sampled: the ring, the done rule and the shift agree with what the rollout did
    assert float((torch.exp(logp - batch["logp"]) - 1).abs().max()) < 1e-4
    t = {"obs": batch["obs"], "actions": batch["actions"], "logp_old": batch["logp"], "advantages": batch["advantages"],
         "value_targets": batch["value_targets"], "vf_pred": batch["value"], "behaviour_logits": logits.contiguous(),
         "state": batch["state"], "done": batch["done"]}
    opt = torch.optim.Adam(pol.parameters(), lr=lr, eps=1.0)   # eps = 1: |d step / d grad| <= lr
    opt_twin = torch.optim.Adam(twin.parameters(), lr=lr, eps=1.0)
    loss, stats = ppo_loss_recurrent(pol, dict(batch, logits=t["behaviour_logits"]), seq_len=T, obs_first=first, **h)
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
        print("step %-10s diff %.3e bound %.3e" % (name, diff, bound))
        assert diff <= bound, (name, diff, bound)
    nxt = env.sample(pol, steps, state_every=T, gamma=0.99, lambda_=0.95)
    torch.cuda.synchronize()
    assert torch.isfinite(nxt["advantages"]).all() and not torch.equal(batch["value"], nxt["value"])
