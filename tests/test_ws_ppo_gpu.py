"""ppo_loss_watershed on the MI355X (csrc/ssd_ws_policy_grad.hip, ssd_ws_policy_ppo_grad): the kernels' gradients, statistics and
loss against the float64 restatement (ws_ppo_ref.py) with torch's own float32 autograd on the same device as the yardstick, for
both heads; bit-equal repeats; exact zeros where no gradient may flow; the sequence kernel's tile loop and the split-K kernel's
second chunks; the state rule; the refusals; and one optimiser step end to end from sample()."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from sequential_social_dilemma_games_amd import WatershedVecEngine, _capi, ppo_loss_watershed
from sequential_social_dilemma_games_amd.policy import PPO_STATS, ws_is_comm
from ws_ppo_ref import (BRANCHES, HYPER, HYPER_KEYS, MARGIN, SEQ, SEQ_COMM, as_numpy_u32, autograd_loss, branch_report, current_logp,
                        forward, gather_own_steps, make_inputs, make_policy, max_err)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# The factor of `ek <= FACTOR * et + 1e-6 * max(1, max |ref|)` per tensor: the project's margin, 4, for every tensor (DESIGN.md
# section 21 records the measured ek / et).
FACTOR = {}


def case(M=7, T=3, Q=17, C_=64, variant=SEQ_COMM, agent=5, local=False, share=False, beh=True, starts="none", stream=False, seed=1):
    return (M, T, Q, C_, variant, agent, local, share, beh, starts, stream, seed)


# each line varies one thing from M = 7, T = 3, Q = 17, C = 64, SeqComm, agent 5.  The seeds are chosen on the CPU for the margin.
CASES = [case(1, 1, seed=1), case(5, 5, seed=2), case(7, 3, seed=3), case(4, 8, seed=4), case(6, 1, seed=5),           # (M, T)
         case(Q=1, seed=6), case(Q=15, seed=7), case(Q=16, seed=8), case(Q=33, seed=9),                                # Q
         case(C_=128, seed=10), case(3, 3, Q=16, C_=256, seed=11),
         case(agent=0, seed=12), case(agent=3, seed=13), case(agent=7, seed=14), case(variant=SEQ, agent=0, seed=15),  # the heads
         case(local=True, seed=16), case(local=True, agent=2, seed=17), case(share=True, seed=18), case(share=True, agent=1, seed=19),
         case(beh=False, seed=20), case(beh=False, agent=1, seed=21),
         case(starts="mid", seed=22), case(starts="window_start", seed=23), case(starts="per_seq", seed=24),
         case(starts="per_seq", agent=2, seed=25), case(stream=True, starts="per_seq", seed=26),
         # 1001 rows: every branch of the report above 0.2 (seed 27, on the CPU: clipped_pos 0.265, clipped_neg 0.227,
         # open_pos 0.247, open_neg 0.262, vf_dead 0.326, vf_live 0.674, vf_clipped_live 0.217; margin 5.0e-4)
         case(M=13, T=4, Q=77, starts="per_seq", seed=27)]


def _to_dev(t):
    return {k: v.to(DEV) for k, v in t.items()}


def _grads(pol):
    out = {}
    for name, _, _ in pol.layout():
        g = getattr(pol, name).grad
        out[name] = torch.zeros_like(getattr(pol, name)) if g is None else g.detach().clone()
    return out


def _run(pol, agent, t, h, T):
    """ppo_loss_watershed + backward on the device -> (loss, stats, {param: grad})."""
    pol.zero_grad()
    loss, stats = ppo_loss_watershed(pol, agent, t, seq_len=T, **h)
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
    for k in PPO_STATS:
        assert np.array_equal(as_numpy_u32(sa[k]), as_numpy_u32(sb[k])), k
    for name in ga:
        assert np.array_equal(as_numpy_u32(ga[name]), as_numpy_u32(gb[name])), name


def _exact_zeros(pol, agent, g):
    """What must be exactly zero whatever the inputs: every other set's rows (a shared dense1: every entry but id % 4), an action
    agent's unused outputs, and the rows of dense0_w beyond the agent's observation length."""
    for name in g:
        e = agent % g[name].shape[0]
        rest = torch.ones(g[name].shape[0], dtype=torch.bool)
        rest[e] = False
        assert float(g[name][rest].abs().max()) == 0.0, name
    if not ws_is_comm(pol.variant, agent):
        assert float(g["out_w"][agent][:, 2:].abs().max()) == 0.0 and float(g["out_b"][agent][2:].abs().max()) == 0.0
    n = pol.obs_lens[agent]
    if n < 12:
        assert float(g["dense0_w"][agent][n:].abs().max()) == 0.0
    assert float(g["dense0_w"][agent][:n].abs().max()) > 0.0 and float(g["lstm_kernel"][agent].abs().max()) > 0.0


def compare_with_float64(pol, agent, t, h, T, own_stream=False):
    """The kernels on (pol, agent, t, h) against the float64 restatement with torch's float32 autograd on the device as the
    yardstick -- gradients, statistics and loss under the bound --, all outputs finite, the exact zeros, and a second call
    bit-equal to the first."""
    loss64, stats64, g64 = autograd_loss(pol, agent, t, h, T)
    loss32, stats32, g32 = autograd_loss(pol, agent, t, h, T, dtype=torch.float32, device=DEV)
    dpol, dt = copy.deepcopy(pol).to(DEV), _to_dev(t)
    if own_stream:
        s = torch.cuda.Stream(DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            out = _run(dpol, agent, dt, h, T)
        s.synchronize()
    else:
        out = _run(dpol, agent, dt, h, T)
    torch.cuda.synchronize()
    loss, stats, g = out
    assert all(stats[k].dim() == 0 and stats[k].dtype == torch.float64 for k in PPO_STATS)
    assert all(bool(torch.isfinite(x).all()) for x in list(g.values()) + list(stats.values()) + [loss])
    _check_against_reference(g, g32, g64, "grad")
    _check_against_reference(stats, stats32, stats64, "stat")
    _check_against_reference({"loss": loss}, {"loss": loss32}, {"loss": loss64}, "loss")
    _exact_zeros(pol, agent, g)
    out2 = _run(dpol, agent, dt, h, T)
    torch.cuda.synchronize()
    _equal_bits(out, out2)
    return out


@pytest.mark.parametrize("M,T,Q,C_,variant,agent,local,share,beh,starts,own_stream,seed", CASES)
def test_gradients_and_stats_against_float64(M, T, Q, C_, variant, agent, local, share, beh, starts, own_stream, seed):
    h = dict(HYPER, kl_coeff=HYPER["kl_coeff"] if beh else 0.0)
    pol = make_policy(variant, C_, seed=seed, local_obs=local, share_comm_layer=share)
    t = make_inputs(pol, agent, M, Q, T, seed=100 + seed, behaviour=beh, starts_mode=starts)
    rep = branch_report(pol, agent, t, h, T)
    print("case", (M, T, Q, C_, variant, agent, local, share, beh, starts, own_stream), rep)
    assert rep["margin"] > MARGIN and rep["max_abs_log_std"] <= 1.0, rep
    if M * Q >= 1000:
        for k in BRANCHES:
            assert rep[k] > 0.2, rep
    compare_with_float64(pol, agent, t, h, T, own_stream)


def test_persistent_loop_takes_a_second_tile():
    """More tiles than workgroups: Q = 16 G + 1 with G the call's groups cap (1024: 16 385 sequences), M = T = 2, C = 64, so
    workgroup 0 takes a second tile with one live sequence.  The seed is chosen on the CPU for the margin."""
    G = _capi.SSD_WSPPO_GROUPS(10 ** 6)
    Q = 16 * G + 1
    assert _capi.SSD_WSPPO_GROUPS(Q) == G and -(-Q // 16) == G + 1
    pol = make_policy(SEQ_COMM, 64, seed=30)
    t = make_inputs(pol, 5, 2, Q, 2, seed=MULTI_TILE_SEED, starts_mode="per_seq")
    rep = branch_report(pol, 5, t, HYPER, 2)
    print("multi-tile", Q, rep)
    assert rep["margin"] > MARGIN, rep
    for k in BRANCHES:
        assert rep[k] > 0.2, rep
    compare_with_float64(pol, 5, t, HYPER, 2)


# input seeds found on the CPU: 131 (margin 1.9e-4; 130 has a row 7.9e-6 from a kink), and 142 for both split cases (margins 1.9e-3
# and 2.6e-4; 141 leaves agent 5 a row 3.4e-5 from one); every branch holds 0.2 of the rows or more
MULTI_TILE_SEED = 131
SPLIT_SEEDS = {5: 142, 1: 142}


@pytest.mark.parametrize("agent", [5, 1])
def test_split_k_takes_a_second_chunk(agent):
    """ssd_ws_dw_kernel's `chunk += S`: Q = 129, M = 17, T = 16: the first window holds 2064 rows, 33 chunks of 64 with a ragged
    last one of 16 rows, for 32 splits; the second window (129 rows, 3 chunks) leaves most splits what the first left."""
    M, T, Q = 17, 16, 129
    splits, chunk = _capi.SSD_WSPPO_MAX_SPLITS, _capi.SSD_WSPPO_CHUNK
    rows1, rows2 = T * Q, (M - T) * Q
    assert _capi.SSD_WSPPO_SPLITS(rows1) == splits == 32 and -(-rows1 // chunk) > splits and rows1 % chunk
    assert 0 < -(-rows2 // chunk) < splits
    pol = make_policy(SEQ_COMM, 64, seed=40 + agent)
    t = make_inputs(pol, agent, M, Q, T, seed=SPLIT_SEEDS[agent], starts_mode="per_seq")
    rep = branch_report(pol, agent, t, HYPER, T)
    print("split", agent, rep)
    assert rep["margin"] > MARGIN, rep
    for k in BRANCHES:
        assert rep[k] > 0.2, rep
    compare_with_float64(pol, agent, t, HYPER, T)


def test_state_rows_other_than_the_window_starts_change_nothing():
    """state may hold more rows than ceil(M / T) (a longer ring), and within the rule only state[m / T] at m % T == 0 is read:
    a ring with garbage appended, and starts set at the windows' first steps, give the same bits; no gradient reaches state."""
    M, T, Q = 7, 3, 17
    pol = make_policy(SEQ_COMM, 64, seed=50)
    t = make_inputs(pol, 5, M, Q, T, seed=51, starts_mode="mid")
    dpol, dt = pol.to(DEV), _to_dev(t)
    a = _run(dpol, 5, dt, HYPER, T)
    longer = torch.cat([dt["state"], torch.full_like(dt["state"][:2], float("nan"))])
    b = _run(dpol, 5, dict(dt, state=longer), HYPER, T)
    s = dt["starts"].clone()
    s[::T] = 1
    c = _run(dpol, 5, dict(dt, starts=s), HYPER, T)
    st = dt["state"].clone().requires_grad_(True)
    dpol.zero_grad()
    loss, _ = ppo_loss_watershed(dpol, 5, dict(dt, state=st), seq_len=T, **HYPER)
    loss.backward()
    torch.cuda.synchronize()
    _equal_bits(a, b)
    _equal_bits(a, c)
    assert st.grad is None
    # and a step that starts reads no state at all: with starts on every row past the window starts, the values of state at a
    # window start still count, nothing else could
    ones = torch.ones_like(dt["starts"])
    d = _run(dpol, 5, dict(dt, starts=ones), HYPER, T)
    e = _run(dpol, 5, dict(dt, starts=ones, state=dt["state"] + 1.0), HYPER, T)
    torch.cuda.synchronize()
    assert not np.array_equal(as_numpy_u32(d[2]["lstm_recurrent"]), as_numpy_u32(e[2]["lstm_recurrent"]))


def test_nothing_crosses_a_start():
    """Changing obs of the rows before a starts row changes no gradient contribution after it: with starts on every sequence at
    step 2 of a 4-step window, the call equals (to float32 rounding of the sums' order) the sum of the two fragments cut
    there -- asked for exactly as: the gradient of the whole minus that of the head fragment does not move, to the bit, when
    the head's observations change, with the loss hyper-parameters such that the tail rows alone carry weight."""
    M, T, Q = 4, 4, 17
    pol = make_policy(SEQ_COMM, 64, seed=60)
    t = make_inputs(pol, 5, M, Q, T, seed=61, behaviour=False)
    s = torch.zeros((M, Q), dtype=torch.uint8)
    s[2] = 1
    t["starts"] = s
    # rows 0 and 1 weigh nothing: adv = 0 there, and with vf_loss_coeff = entropy_coeff = kl_coeff = 0 the row loss is -surr alone
    t["advantages"][:2] = 0.0
    h = dict(HYPER, vf_loss_coeff=0.0, entropy_coeff=0.0, kl_coeff=0.0)
    dpol, dt = pol.to(DEV), _to_dev(t)
    a = _run(dpol, 5, dt, h, T)
    moved = dict(dt, obs=dt["obs"].clone())
    moved["obs"][:2] += 0.25
    b = _run(dpol, 5, moved, h, T)
    # the fragment cut at the start: steps 2 and 3 alone from a zero state, the same rows over the same divisor
    tail = {k: v[2:].contiguous() for k, v in dt.items() if k != "state"}
    tail["state"] = torch.zeros_like(dt["state"])
    c = _run(dpol, 5, tail, h, 2)
    torch.cuda.synchronize()
    for name in a[2]:
        assert np.array_equal(as_numpy_u32(a[2][name]), as_numpy_u32(b[2][name])), name
        want = c[2][name] * 0.5                                   # the tail alone averages over half the rows
        # (the two calls cut the rows into other chunks and tiles: some 40 float32 roundings of terms below 1 apart; a
        # contribution that crossed the start would be of the gradient's own size)
        assert max_err(a[2][name], want) <= 1e-5 * max(1.0, float(want.abs().max())), name
    assert float(a[2]["lstm_recurrent"][5].abs().max()) > 0.0


def test_repeats_and_a_grown_scratch_give_the_same_bits():
    pol = make_policy(SEQ_COMM, 64, seed=70)
    t = make_inputs(pol, 5, 7, 17, 3, seed=71, starts_mode="per_seq")
    big = make_inputs(pol, 1, 9, 40, 4, seed=72)
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
    """ssd_ws_policy_ppo_grad itself -> (rc, packed grads, stats); `over` replaces arguments by name."""
    M, Q = t["actions"].shape
    S = pol.set_floats
    packed = torch.full((S,), float("nan"), dtype=torch.float32, device=DEV)
    stats = torch.zeros((5,), dtype=torch.float64, device=DEV)
    scratch = torch.empty(_capi.SSD_WSPPO_SCRATCH_FLOATS(M, Q, pol.cell_size, T) + 2, dtype=torch.float32, device=DEV)
    ptr = lambda x: None if x is None else C.c_void_p(x if isinstance(x, int) else x.data_ptr())   # noqa: E731
    a = dict(weights=pol.packed(), num_sets=pol.num_sets, cell_size=pol.cell_size, variant=pol.variant, agent_id=agent, seq_len=T,
             obs=t["obs"], state=t["state"], starts=t.get("starts"), actions=t["actions"], logp_old=t["logp_old"],
             advantages=t["advantages"], value_targets=t["value_targets"], vf_preds=t["vf_pred"],
             behaviour_dist=t.get("behaviour_dist") if h["kl_coeff"] != 0 else None, n_steps=M, num_seqs=Q, scratch=scratch,
             grads=packed, stats=stats)
    hv = {k: h[k] for k in HYPER_KEYS}
    for k, v in over.items():
        (hv if k in hv else a)[k] = v
    rc = _capi.lib().ssd_ws_policy_ppo_grad(
        ptr(a["weights"]), a["num_sets"], a["cell_size"], a["variant"], a["agent_id"], a["seq_len"], ptr(a["obs"]), ptr(a["state"]),
        ptr(a["starts"]), ptr(a["actions"]), ptr(a["logp_old"]), ptr(a["advantages"]), ptr(a["value_targets"]), ptr(a["vf_preds"]),
        ptr(a["behaviour_dist"]), a["n_steps"], a["num_seqs"], *(hv[k] for k in HYPER_KEYS), ptr(a["scratch"]), ptr(a["grads"]),
        ptr(a["stats"]), 0, over.get("flags", 0), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return rc, packed, stats


def test_packed_gradient_padding_and_scaling():
    """The library's packed gradient has zero padding floats and holds what backward scatters; backward multiplies by the
    incoming gradient."""
    M, Q, T = 5, 7, 2
    pol = make_policy(SEQ_COMM, 64, seed=80)
    t = make_inputs(pol, 5, M, Q, T, seed=81, starts_mode="mid")
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
    for k, name in enumerate(PPO_STATS):
        assert float(raw_stats[k]) == float(stats[name])
    pol.zero_grad()
    loss, _ = ppo_loss_watershed(pol, 5, t, seq_len=T, **HYPER)
    (loss * 3.0).backward()
    for name in g:
        assert torch.equal(getattr(pol, name).grad, g[name] * 3.0), name


def test_refusals():
    """Every SSD_E_INVALID case of the contract: refused before any launch (the outputs keep what they held) with a reason."""
    M, Q, T = 4, 5, 2
    pol = make_policy(SEQ_COMM, 64, seed=90)
    t = make_inputs(pol, 5, M, Q, T, seed=91)
    pol, t = pol.to(DEV), _to_dev(t)
    seq_pol = make_policy(SEQ, 64, seed=90).to(DEV)
    odd = torch.empty(_capi.SSD_WSPPO_SCRATCH_FLOATS(M, Q, 64, T) + 2, dtype=torch.float32, device=DEV)
    bad = [dict(agent_id=8), dict(agent_id=-1), dict(cell_size=96), dict(seq_len=0), dict(n_steps=0), dict(num_seqs=0),
           dict(weights=None), dict(obs=None), dict(state=None), dict(actions=None), dict(logp_old=None), dict(advantages=None),
           dict(value_targets=None), dict(vf_preds=None), dict(scratch=None), dict(grads=None), dict(stats=None),
           dict(behaviour_dist=None), dict(scratch=odd.data_ptr() + 4), dict(variant=7), dict(num_sets=4), dict(flags=1),
           dict(clip_param=-0.1), dict(vf_loss_coeff=float("nan"))]
    for over in bad:
        rc, packed, stats = _raw_call(pol, 5, t, HYPER, T, **over)
        msg = _capi.lib().ssd_policy_last_error()
        assert rc == _capi.SSD_E_INVALID and msg, over
        if "grads" not in over:
            assert bool(torch.isnan(packed).all()), over          # nothing was launched
        if "stats" not in over:
            assert float(stats.abs().max()) == 0.0, over
    rc, _, _ = _raw_call(seq_pol, 4, make_inputs_dev(seq_pol, 0, M, Q, T), HYPER, T)      # id 4 is outside Seq's 0 .. 3
    assert rc == _capi.SSD_E_INVALID and _capi.lib().ssd_policy_last_error()
    rc, packed, _ = _raw_call(pol, 5, t, HYPER, T)
    assert rc == _capi.SSD_OK and bool(torch.isfinite(packed).all())
    # behaviour_dist may be NULL with kl_coeff == 0
    rc, packed, _ = _raw_call(pol, 5, t, dict(HYPER, kl_coeff=0.0), T)
    assert rc == _capi.SSD_OK and bool(torch.isfinite(packed).all())


def make_inputs_dev(pol, agent, M, Q, T):
    return _to_dev(make_inputs(copy.deepcopy(pol).cpu(), agent, M, Q, T, seed=92))


@pytest.mark.parametrize("variant,agents", [(SEQ_COMM, (5, 1)), (SEQ, (1,))])
def test_sample_loss_step(variant, agents):
    """sample() over two rounds and most of a third at E = 64 -> the agent's own rows gathered as the example gathers them ->
    ppo_loss_watershed -> backward -> one SGD step, against the same step from the torch loss.  With the weights that sampled,
    the call's own logp and dist are the rollout's: ratio - 1 under 1e-4, kl under 1e-6."""
    E, T, lr = 64, 2, 1e-2
    K_ = 34 if variant == SEQ_COMM else 11                      # the third own step of the last agent of a round included
    h = dict(clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1e-2, entropy_coeff=1e-3, kl_coeff=0.2)
    eng = WatershedVecEngine(variant, E, seed=5)
    pol = make_policy(variant, 64, seed=31).to(DEV)
    first, _ = eng.reset()
    first = first.clone()
    batch = eng.sample(pol, K_)
    for agent in agents:
        seq, ks = gather_own_steps(batch, first, agent, T)
        M = len(ks)
        assert M >= (4 if ws_is_comm(variant, agent) else 2) and M > T, ks
        comm = bool(ws_is_comm(variant, agent))
        with torch.no_grad():                                    # a replay in torch: the gather, the ring and the start rule agree
            dist, value = forward(pol, agent, seq["obs"], seq["state"], seq["starts"], T)
            logp = current_logp(dist, seq["actions"], comm)
        assert float((torch.exp(logp - seq["logp"]) - 1).abs().max()) < 1e-4
        g = torch.Generator().manual_seed(7 + agent)
        seq["advantages"] = torch.randn((M, E), generator=g).to(DEV)
        seq["value_targets"] = (seq["value"] + torch.randn((M, E), generator=g).to(DEV)).contiguous()
        # the call's own ratio and kl: adv = 1 and no clip in reach make policy_loss = -mean(ratio)
        _, stats = ppo_loss_watershed(pol, agent, dict(seq, advantages=torch.ones_like(seq["value"])), seq_len=T,
                                      **dict(h, clip_param=1e6))
        assert abs(float(stats["policy_loss"]) + 1.0) < 1e-4 and abs(float(stats["kl"])) < 1e-6, stats
        twin = copy.deepcopy(pol)
        opt = torch.optim.SGD(pol.parameters(), lr=lr)
        opt_twin = torch.optim.SGD(twin.parameters(), lr=lr)
        loss, stats = ppo_loss_watershed(pol, agent, seq, seq_len=T, **h)
        opt.zero_grad()
        loss.backward()
        got = _grads(pol)
        t = {"obs": seq["obs"], "state": seq["state"], "starts": seq["starts"], "actions": seq["actions"], "logp_old": seq["logp"],
             "advantages": seq["advantages"], "value_targets": seq["value_targets"], "vf_pred": seq["value"],
             "behaviour_dist": seq["dist"]}
        cpu_t = {k: v.cpu() for k, v in t.items()}
        _, _, g64 = autograd_loss(copy.deepcopy(twin).cpu(), agent, cpu_t, h, T)
        _, _, g32 = autograd_loss(twin, agent, cpu_t, h, T, dtype=torch.float32, device=DEV)
        _check_against_reference(got, g32, g64, "e2e grad %d" % agent)
        for name, _, _ in twin.layout():
            getattr(twin, name).grad = g32[name].clone()
        opt.step()
        opt_twin.step()
        for name, _, _ in pol.layout():
            et = max_err(g32[name], g64[name])
            scale = max(1.0, float(g64[name].abs().max()))
            bound = lr * (5 * et + 1e-6 * scale) + 2 ** -22 * float(getattr(twin, name).detach().abs().max())   # ek + et, and the update's rounding
            diff = max_err(getattr(pol, name), getattr(twin, name))
            print("step %d %-14s diff %.3e bound %.3e" % (agent, name, diff, bound))
            assert diff <= bound, (name, diff, bound)
