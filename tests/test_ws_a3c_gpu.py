"""a3c_loss_watershed on the MI355X (csrc/ssd_ws_policy_grad.hip, ssd_ws_policy_ac_grad): the kernels' gradients, statistics and
loss against the float64 restatement (ws_a3c_ref.py) with torch's own float32 autograd on the same device as the yardstick, for
both heads; whether the bound would notice a wrong loss; exact sums with more tiles than workgroups; the split-K kernel's
second chunk; exact zeros where no gradient may flow; bit-equal repeats; the refusals; and one optimiser step end to end from
sample()."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from sequential_social_dilemma_games_amd import (WatershedVecEngine, _capi, a3c_loss_watershed, clip_grad_by_set_norm,
                                                 compute_advantages)
from sequential_social_dilemma_games_amd.policy import A3C_STATS, ws_is_comm
from ws_a3c_ref import (HYPER, SEQ, SEQ_COMM, STARTS_MODES, VARIANTS, as_numpy_u32, autograd_loss, bound, gather_own_steps, make_inputs,
                        make_policy, max_err, zero_policy)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FACTOR = 4.0            # of `ek <= FACTOR * et + 1e-6 * max(1, max |ref|)`: the project's margin, for every tensor


def _to_dev(t):
    return {k: v.to(DEV) for k, v in t.items()}


def _grads(pol):
    out = {}
    for name, _, _ in pol.layout():
        g = getattr(pol, name).grad
        out[name] = torch.zeros_like(getattr(pol, name)) if g is None else g.detach().clone()
    return out


def _run(pol, agent, t, h, T):
    """a3c_loss_watershed + backward on the device -> (loss, stats, {param: grad})."""
    pol.zero_grad()
    loss, stats = a3c_loss_watershed(pol, agent, t, seq_len=T, **h)
    loss.backward()
    return loss.detach(), stats, _grads(pol)


def _check_against_reference(got, tor, ref, what):
    """ek <= FACTOR * et + 1e-6 * max(1, max |ref|) for every tensor of the dicts; prints each figure before it asserts."""
    bad = []
    for name in ref:
        ek, et = max_err(got[name], ref[name]), max_err(tor[name], ref[name])
        scale = max(1.0, float(ref[name].abs().max()))
        print("%s %-14s ek %.3e et %.3e ek/et %.2f max|ref| %.3e" % (what, name, ek, et, ek / et if et else float("inf"), scale))
        if not ek <= FACTOR * et + 1e-6 * scale:
            bad.append((name, ek, et))
    assert not bad, (what, bad)


def _equal_bits(a, b):
    la, sa, ga = a
    lb, sb, gb = b
    assert np.array_equal(as_numpy_u32(la), as_numpy_u32(lb))
    for k in A3C_STATS:
        assert np.array_equal(as_numpy_u32(sa[k]), as_numpy_u32(sb[k])), k
    for name in ga:
        assert np.array_equal(as_numpy_u32(ga[name]), as_numpy_u32(gb[name])), name


def _exact_zeros(pol, agent, g):
    """What must be exactly zero whatever the inputs: every other set's rows (a shared dense1: every entry but id % 4), an action
    agent's unused outputs, and the rows of dense0_w beyond the agent's observation length."""
    for name in g:
        rest = torch.ones(g[name].shape[0], dtype=torch.bool)
        rest[agent % g[name].shape[0]] = False
        assert float(g[name][rest].abs().max()) == 0.0, name
    if not ws_is_comm(pol.variant, agent):
        assert float(g["out_w"][agent][:, 2:].abs().max()) == 0.0 and float(g["out_b"][agent][2:].abs().max()) == 0.0
    n = pol.obs_lens[agent]
    if n < 12:
        assert float(g["dense0_w"][agent][n:].abs().max()) == 0.0
    assert float(g["dense0_w"][agent][:n].abs().max()) > 0.0 and float(g["lstm_kernel"][agent].abs().max()) > 0.0


def compare_with_float64(pol, agent, t, h, T, before=None):
    """The kernels on (pol, agent, t, h) against the float64 restatement with torch's float32 autograd on the device as the
    yardstick -- gradients, statistics and loss under the bound --, all outputs finite, the exact zeros, and a second call
    bit-equal to the first.  before(g64, g32): asserted on the references after the kernel has run, before it is compared."""
    loss64, stats64, g64 = autograd_loss(pol, agent, t, h, T)
    loss32, stats32, g32 = autograd_loss(pol, agent, t, h, T, dtype=torch.float32, device=DEV)
    dpol, dt = copy.deepcopy(pol).to(DEV), _to_dev(t)
    out = _run(dpol, agent, dt, h, T)
    torch.cuda.synchronize()
    if before is not None:
        before(g64, g32)
    loss, stats, g = out
    assert all(stats[k].dim() == 0 and stats[k].dtype == torch.float64 for k in A3C_STATS)
    assert all(bool(torch.isfinite(x).all()) for x in list(g.values()) + list(stats.values()) + [loss])
    _check_against_reference(g, g32, g64, "grad")
    _check_against_reference(stats, stats32, stats64, "stat")
    _check_against_reference({"loss": loss}, {"loss": loss32}, {"loss": loss64}, "loss")
    _exact_zeros(pol, agent, g)
    out2 = _run(dpol, agent, dt, h, T)
    torch.cuda.synchronize()
    _equal_bits(out, out2)
    return out


def case(M=7, T=3, Q=17, C_=64, variant=SEQ_COMM, agent=5, share=False, starts="none", seed=1):
    return (M, T, Q, C_, variant, agent, share, starts, seed)


# M = 7, T = 3, Q = 17, C = 64: a short last window, a tile and a one-row tail, for a comm id and an action id of SeqComm and an
# id of Seq under each starts mode; then M = 1, M < T, the two larger cells once each, and a shared dense1
CASES = ([case(variant=v, agent=a, starts=s, seed=10 * i + j) for i, (v, a) in enumerate(((SEQ_COMM, 1), (SEQ_COMM, 5), (SEQ, 1)))
          for j, s in enumerate(STARTS_MODES)]
         + [case(M=1, T=3, seed=40), case(M=1, T=1, agent=1, seed=41), case(M=2, T=5, starts="per_seq", seed=42),
            case(M=4, T=4, C_=128, starts="per_seq", seed=43), case(M=4, T=4, C_=256, agent=1, starts="per_seq", seed=44),
            case(share=True, starts="mid", seed=45), case(share=True, agent=1, seed=46)])


@pytest.mark.parametrize("M,T,Q,C_,variant,agent,share,starts,seed", CASES)
def test_gradients_and_stats_against_float64(M, T, Q, C_, variant, agent, share, starts, seed):
    pol = make_policy(variant, C_, seed=seed, share_comm_layer=share)
    t = make_inputs(pol, agent, M, Q, T, seed=100 + seed, behaviour=False, starts_mode=starts)
    print("case", (M, T, Q, C_, variant, agent, share, starts))
    compare_with_float64(pol, agent, t, HYPER, T)


@pytest.mark.parametrize("agent", [1, 5])
def test_bound_separates_the_loss_from_wrong_ones(agent):
    """For each wrong variant of the restatement (the terms as means, the value term without its half, the advantage's sign
    flipped), its float64 gradient is off from the true one by 100 bounds or more in some tensor -- asserted after the kernel
    call and before the kernel is compared; then the kernel passes the bound."""
    M, T, Q = 7, 3, 17
    pol = make_policy(SEQ_COMM, 64, seed=50 + agent)
    t = make_inputs(pol, agent, M, Q, T, seed=150 + agent, behaviour=False, starts_mode="per_seq")

    def before(g64, g32):
        bounds = {name: bound(g64[name], max_err(g32[name], g64[name])) for name in g64}
        for variant in VARIANTS:
            _, _, gv = autograd_loss(pol, agent, t, HYPER, T, variant=variant)
            ratios = {name: max_err(gv[name], g64[name]) / bounds[name] for name in g64}
            worst = max(ratios, key=ratios.get)
            print("variant %-10s off by %.1f bounds in %s" % (variant, ratios[worst], worst))
            assert ratios[worst] >= 100.0, (variant, ratios)
    compare_with_float64(pol, agent, t, HYPER, T, before=before)


@pytest.mark.parametrize("agent", [1, 5])
def test_exact_sums_with_more_tiles_than_workgroups(agent):
    """Q = 16 * 1024 + 17, M = T = 2, C = 64: 1026 tiles for 1024 workgroups, the last tile with one live row.  Every parameter
    zero, adv = 0, vf_loss_coeff = 1, entropy_coeff = 0 and integer value targets: value = 0 on every row, so
    vf_loss = 0.5 sum vt^2 and d loss / d value_b = -sum vt, every partial sum an integer or a half below 2^24 (float32) and
    2^53 (float64): matched with ==.  A kernel that divides by the rows, or skips or double-counts a tile, fails it."""
    G = _capi.SSD_WSPPO_GROUPS(10 ** 6)
    M, T, Q = 2, 2, 16 * G + 17
    assert G == 1024 and _capi.SSD_WSPPO_GROUPS(Q) == G and -(-Q // 16) == G + 2
    pol = zero_policy(SEQ_COMM, 64)
    g = torch.Generator().manual_seed(60 + agent)
    vt = torch.randint(-5, 6, (M, Q), generator=g).float()
    assert float(vt.abs().sum()) < 2 ** 24 and float((vt.double() ** 2).sum()) < 2 ** 53
    acts = torch.randint(0, 5, (M, Q), generator=g).float() if ws_is_comm(SEQ_COMM, agent) else torch.randn((M, Q), generator=g)
    t = {"obs": torch.rand((M, Q, 12), generator=g), "state": torch.randn((1, Q, 2, 64), generator=g), "actions": acts,
         "advantages": torch.zeros((M, Q)), "value_targets": vt, "starts": (torch.rand((M, Q), generator=g) < 0.3).to(torch.uint8)}
    loss, stats, grads = _run(pol.to(DEV), agent, _to_dev(t), dict(vf_loss_coeff=1.0, entropy_coeff=0.0), T)
    torch.cuda.synchronize()
    want_vf, want_db = 0.5 * float((vt.double() ** 2).sum()), -float(vt.double().sum())
    assert float(stats["vf_loss"]) == want_vf and float(stats["total_loss"]) == want_vf
    assert float(stats["policy_loss"]) == 0.0
    assert float(grads["value_b"][agent, 0]) == want_db
    assert float(loss) == float(np.float32(want_vf))


@pytest.mark.parametrize("agent", [5, 1])
def test_split_k_takes_a_second_chunk(agent):
    """ssd_ws_dw_kernel's `chunk += S` under the A3C call: T = 2, Q = 1100: a window of 2200 rows, 35 chunks of 64 (a ragged
    last one of 24 rows) for 32 splits, so splits 0 to 2 take a second chunk."""
    M, T, Q = 2, 2, 1100
    rows, chunk, splits = T * Q, _capi.SSD_WSPPO_CHUNK, _capi.SSD_WSPPO_MAX_SPLITS
    assert rows > chunk * splits and _capi.SSD_WSPPO_SPLITS(rows) == splits == 32 and rows % chunk
    pol = make_policy(SEQ_COMM, 64, seed=70 + agent)
    t = make_inputs(pol, agent, M, Q, T, seed=170 + agent, behaviour=False, starts_mode="per_seq")
    compare_with_float64(pol, agent, t, HYPER, T)


def test_repeats_and_a_grown_scratch_give_the_same_bits():
    pol = make_policy(SEQ_COMM, 64, seed=80)
    t = make_inputs(pol, 5, 7, 17, 3, seed=81, behaviour=False, starts_mode="per_seq")
    big = make_inputs(pol, 1, 9, 40, 4, seed=82, behaviour=False)
    pol, t = pol.to(DEV), _to_dev(t)
    fresh = copy.deepcopy(pol)
    a = _run(pol, 5, t, HYPER, 3)
    _run(pol, 1, _to_dev(big), HYPER, 4)
    grown = pol._ppo_scratch.numel()
    pol._ppo_scratch.fill_(float("nan"))                       # whatever an earlier call left there is never read
    b = _run(pol, 5, t, HYPER, 3)
    assert pol._ppo_scratch.numel() == grown > _capi.SSD_WSPPO_SCRATCH_FLOATS(7, 17, 64, 3)
    c = _run(fresh, 5, t, HYPER, 3)
    torch.cuda.synchronize()
    _equal_bits(a, b)
    _equal_bits(a, c)


def _raw_call(pol, agent, t, h, T, **over):
    """ssd_ws_policy_ac_grad itself -> (rc, packed grads, stats); `over` replaces arguments by name."""
    M, Q = t["actions"].shape
    packed = torch.full((pol.set_floats,), float("nan"), dtype=torch.float32, device=DEV)
    stats = torch.zeros((4,), dtype=torch.float64, device=DEV)
    scratch = torch.empty(_capi.SSD_WSPPO_SCRATCH_FLOATS(M, Q, pol.cell_size, T) + 2, dtype=torch.float32, device=DEV)
    ptr = lambda x: None if x is None else C.c_void_p(x if isinstance(x, int) else x.data_ptr())   # noqa: E731
    a = dict(weights=pol.packed(), num_sets=pol.num_sets, cell_size=pol.cell_size, variant=pol.variant, agent_id=agent, seq_len=T,
             obs=t["obs"], state=t["state"], starts=t.get("starts"), actions=t["actions"], advantages=t["advantages"],
             value_targets=t["value_targets"], n_steps=M, num_seqs=Q, scratch=scratch, grads=packed, stats=stats)
    hv = dict(h)
    for k, v in over.items():
        (hv if k in hv else a)[k] = v
    rc = _capi.lib().ssd_ws_policy_ac_grad(
        ptr(a["weights"]), a["num_sets"], a["cell_size"], a["variant"], a["agent_id"], a["seq_len"], ptr(a["obs"]), ptr(a["state"]),
        ptr(a["starts"]), ptr(a["actions"]), ptr(a["advantages"]), ptr(a["value_targets"]), a["n_steps"], a["num_seqs"],
        hv["vf_loss_coeff"], hv["entropy_coeff"], ptr(a["scratch"]), ptr(a["grads"]), ptr(a["stats"]), 0, over.get("flags", 0),
        C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return rc, packed, stats


def test_packed_gradient_padding_and_scaling():
    """The library's packed gradient has zero padding floats and holds what backward scatters; the statistics are the raw
    call's sums; backward multiplies by the incoming gradient."""
    M, Q, T = 5, 7, 2
    pol = make_policy(SEQ_COMM, 64, seed=85)
    t = make_inputs(pol, 5, M, Q, T, seed=86, behaviour=False, starts_mode="mid")
    pol, t = pol.to(DEV), _to_dev(t)
    _, stats, g = _run(pol, 5, t, HYPER, T)
    rc, packed, raw_stats = _raw_call(pol, 5, t, HYPER, T)
    assert rc == _capi.SSD_OK
    used = torch.zeros(pol.set_floats, dtype=torch.bool, device=DEV)
    for name, shape, off in pol.layout():
        n = int(np.prod(shape))
        used[off:off + n] = True
        assert torch.equal(packed[off:off + n].reshape(g[name][5].shape), g[name][5]), name
    assert int((~used).sum()) > 0 and float(packed[~used].abs().max()) == 0.0
    for k, name in enumerate(A3C_STATS):
        assert float(raw_stats[k]) == float(stats[name])
    pol.zero_grad()
    loss, _ = a3c_loss_watershed(pol, 5, t, seq_len=T, **HYPER)
    (loss * 3.0).backward()
    for name in g:
        assert torch.equal(getattr(pol, name).grad, g[name] * 3.0), name


def test_refusals():
    """Every SSD_E_INVALID case of the contract: refused before any launch (the outputs keep what they held) with a reason."""
    M, Q, T = 4, 5, 2
    pol = make_policy(SEQ_COMM, 64, seed=90)
    t = make_inputs(pol, 5, M, Q, T, seed=91, behaviour=False)
    pol, t = pol.to(DEV), _to_dev(t)
    odd = torch.empty(_capi.SSD_WSPPO_SCRATCH_FLOATS(M, Q, 64, T) + 2, dtype=torch.float32, device=DEV)
    bad = [dict(agent_id=8), dict(agent_id=-1), dict(cell_size=96), dict(seq_len=0), dict(n_steps=0), dict(num_seqs=0),
           dict(weights=None), dict(obs=None), dict(state=None), dict(actions=None), dict(advantages=None), dict(value_targets=None),
           dict(scratch=None), dict(grads=None), dict(stats=None), dict(scratch=odd.data_ptr() + 4), dict(variant=7), dict(num_sets=4),
           dict(flags=1), dict(vf_loss_coeff=float("nan")), dict(entropy_coeff=float("inf"))]
    for over in bad:
        rc, packed, stats = _raw_call(pol, 5, t, HYPER, T, **over)
        msg = _capi.lib().ssd_policy_last_error()
        assert rc == _capi.SSD_E_INVALID and msg, over
        if "grads" not in over:
            assert bool(torch.isnan(packed).all()), over          # nothing was launched
        if "stats" not in over:
            assert float(stats.abs().max()) == 0.0, over
    rc, _, _ = _raw_call(pol, 5, t, HYPER, T, actions=None)
    assert b"obs, state, actions, advantages and value_targets are required" in _capi.lib().ssd_policy_last_error()
    rc, packed, _ = _raw_call(pol, 5, t, HYPER, T)
    assert rc == _capi.SSD_OK and bool(torch.isfinite(packed).all())


@pytest.mark.parametrize("agent", [5, 1])
def test_sample_loss_step(agent):
    """sample() over two rounds and most of a third at E = 64 -> the agent's own rows gathered -> compute_advantages(use_gae=False)
    -> a3c_loss_watershed -> backward -> clip_grad_by_set_norm -> one SGD step, against the same step from the float32 torch
    loss, within test_ws_ppo_gpu.py::test_sample_loss_step's bound of the float64 twin's."""
    E, T, K_ = 64, 2, 34
    eng = WatershedVecEngine(SEQ_COMM, E, seed=5)
    pol = make_policy(SEQ_COMM, 64, seed=31).to(DEV)
    first, _ = eng.reset()
    first = first.clone()
    batch = eng.sample(pol, K_)
    seq, ks = gather_own_steps(batch, first, agent, T)
    M = len(ks)
    assert M > T, ks
    idx = torch.tensor(ks, device=DEV)
    rew = batch["rew"][idx].to(torch.float32).contiguous()      # the reward of the own step itself: this test's choice
    done = torch.cat([seq["starts"][1:], torch.zeros_like(seq["starts"][:1])]).contiguous()
    adv, vt = compute_advantages(torch.zeros((M, E), dtype=torch.int32, device=DEV), seq["value"], done=done, gamma=0.99, use_gae=False,
                                 bonus=rew, bonus_weight=1.0)
    seq.update(advantages=adv, value_targets=vt)
    twin = copy.deepcopy(pol)
    cpu_t = {k: v.cpu() for k, v in seq.items()}
    _, _, g64 = autograd_loss(copy.deepcopy(twin).cpu(), agent, cpu_t, HYPER, T)
    _, _, g32 = autograd_loss(twin, agent, cpu_t, HYPER, T, dtype=torch.float32, device=DEV)
    # The A3C loss is a sum over rows of this game's rewards (hundreds): the gradient is large.  The float64 twin's norm sets the
    # scale: a step of 1e-2 along the unit gradient, and a max_norm of twice the norm, so that the clip leaves the gradient
    # as it is and the bound on the gradients carries over to the step (test_ws_a3c_cpu.py's clip is test_a3c_loss_cpu.py's).
    norm64 = float(torch.sqrt(sum((g64[name][agent % g64[name].shape[0]] ** 2).sum() for name in g64)))
    lr, max_norm = 1e-2 / norm64, 2.0 * norm64
    opt = torch.optim.SGD(pol.parameters(), lr=lr)
    opt_twin = torch.optim.SGD(twin.parameters(), lr=lr)
    loss, stats = a3c_loss_watershed(pol, agent, seq, seq_len=T, **HYPER)
    opt.zero_grad()
    loss.backward()
    got = _grads(pol)
    norms = clip_grad_by_set_norm(pol, max_norm)
    print("e2e %d: M %d, float64 norm %.4e, norms %s" % (agent, M, norm64, norms.tolist()))
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v)) for v in stats.values()) and bool(torch.isfinite(norms).all())
    assert abs(float(norms[agent]) - norm64) <= 1e-3 * norm64 and float(norms.sum()) == float(norms[agent])
    for name in got:                                             # below max_norm: the clip changed nothing
        assert torch.equal(getattr(pol, name).grad, got[name]), name
    _check_against_reference(got, g32, g64, "e2e grad %d" % agent)
    for name, _, _ in twin.layout():
        getattr(twin, name).grad = g32[name].clone()
    opt.step()
    opt_twin.step()
    for name, _, _ in pol.layout():
        et = max_err(g32[name], g64[name])
        scale = max(1.0, float(g64[name].abs().max()))
        limit = lr * (5 * et + 1e-6 * scale) + 2 ** -22 * float(getattr(twin, name).detach().abs().max())   # ek + et, and the update's rounding
        diff = max_err(getattr(pol, name), getattr(twin, name))
        print("step %d %-14s diff %.3e bound %.3e" % (agent, name, diff, limit))
        assert bool(torch.isfinite(getattr(pol, name)).all()) and diff <= limit, (name, diff, limit)
