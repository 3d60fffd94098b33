"""The four policy forwards on the MI355X at the shapes the C ABI promises and no rollout reaches (include/ssd.h: 1 <= A <= 15,
1 <= N <= 64, or 2 <= N <= 16 for the MOA policy, P = 1 or N, any batch), called through policy_abi.py: ragged tiles, 64 agents
and 64 weight sets, A = 1 and 15, the MOA cell's string order of the agents (N >= 11) and all of its prediction tiles, the
Watershed rows of no agent, and nothing written past row B (policy_abi.py's sentinel tails, checked by every call below).

Two kinds of assertion: the project's bound ek <= 4 et + 1e-6 against the float64 restatements (et: the float32 torch module's
error against the same restatement), and exact bits where the expected value follows from integers alone (the selector and the
integer constructions of policy_shape_cases.py, checked on the host by test_policy_shapes_cpu.py).  Each bound prints how much
of it the kernel uses ("RATIO ..." lines; profiles/r11_policy_shapes keeps a run's)."""
import numpy as np
import pytest
import torch

import policy_abi as abi
import policy_lstm_ref
import policy_moa_ref
import policy_ref
import policy_shape_cases as cases
import policy_ws_ref
from gae_ref import same_bits
from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd.policy import (ConvFCPolicy, ConvLSTMPolicy, ConvMOAPolicy, WatershedLSTMPolicy, _trunk,
                                                        influence)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _bound(name, case, got, tor, ref):
    ek, et, ratio = cases.error_ratio(_np(got), _np(tor), ref)
    print("RATIO %s %s ek %.3e et %.3e ek/(4et+1e-6) %.3f" % (name, "x".join(str(c) for c in case), ek, et, ratio))
    assert ek <= 4 * et + 1e-6, (name, case, ek, et)


def _same(a, b):
    return same_bits(_np(a), _np(b))


# ------------------------------------------------------------------------------------------------------ 1. conv-FC, bound
@pytest.mark.parametrize("case", cases.CONV_CASES, ids=lambda c: "B%d-N%d-P%d-A%d" % c)
def test_conv_fc_against_restatement(case):
    B, N, P, A = case
    w, obs_h = cases.conv_inputs(case)
    pol = ConvFCPolicy(A, P).load_arrays(w).to(DEV)
    obs = _dev(obs_h)
    lg, v = abi.conv_fc(pol, obs)
    with torch.no_grad():
        tl, tv = pol(obs)
    rl, rv = policy_ref.forward(w, obs_h)
    _bound("convfc.logits", case, lg, tl, rl)
    _bound("convfc.value", case, v, tv, rv)
    assert np.ptp(rl) > 1e-2
    # either output alone: the other one is the same to the bit
    only_v = abi.conv_fc(pol, obs, logits=False)
    only_l = abi.conv_fc(pol, obs, value=False)
    assert only_v[0] is None and _same(only_v[1], v)
    assert only_l[1] is None and _same(only_l[0], lg)


@pytest.mark.parametrize("B,N,A,a,b", [(17, 2, 8, 0, 1), (17, 64, 15, 5, 62)])
def test_conv_fc_swapping_two_weight_sets_swaps_those_agents(B, N, A, a, b):
    w, obs_h = cases.conv_inputs((B, N, N, A))
    obs_h[:, b] = obs_h[:, a]                                    # the two agents see the same, so only their sets tell them apart
    obs = _dev(obs_h)
    lg, v = abi.conv_fc(ConvFCPolicy(A, N).load_arrays(w).to(DEV), obs)
    perm = np.arange(N)
    perm[[a, b]] = perm[[b, a]]
    lg2, v2 = abi.conv_fc(ConvFCPolicy(A, N).load_arrays({k: x[perm] for k, x in w.items()}).to(DEV), obs)
    assert not torch.equal(lg[:, a], lg[:, b]) and not torch.equal(v[:, a], v[:, b]), "the two sets differ"
    assert _same(lg2, lg[:, perm]) and _same(v2, v[:, perm])    # agents a and b swapped, every other agent as before


# ------------------------------------------------------------------------------------------------------ 2. conv-FC, exact
@pytest.mark.parametrize("sign", [1, -1])
def test_selector_pins_every_flat_index(sign):
    """fc1's index map to the bit: the flatten order (row, col, channel), the two K halves that meet at k = 507 | 508 (k-steps
    126 | 127) and are added through LDS, and the peeled last k-step (k = 1012, 1013 and two rows of padding), at B = 17."""
    sets = cases.selector_sets()
    covered = cases.selector_coverage(sets)
    assert covered == list(range(cases.FLAT))
    assert {0, 506, 507, 508, 1011, 1012, 1013} <= set(covered)
    B, half = 17, len(sets) // 2
    rng = np.random.default_rng(17 + sign)
    nonzero = 0
    for part in (sets[:half], sets[half:]):                     # 33 sets of 16 outputs a call
        N = len(part)
        obs_h = cases.random_obs(rng, B, N)
        pol = ConvFCPolicy(cases.SELECTOR_A, N).load_arrays(cases.selector_weights(part, sign)).to(DEV)
        lg, v = abi.conv_fc(pol, _dev(obs_h))
        el, ev = cases.selector_expected(part, sign, obs_h)
        assert same_bits(_np(lg), el) and same_bits(_np(v), ev)
        nonzero += int((el != 0).sum())
    assert nonzero > B * len(sets) * 4                          # (about half of the bytes are on the ReLU's open side)


def test_padding_rows_of_fc1_are_inert():
    """The peel's rows 1014 and 1015 are no rows of fc1_w, and with P = 1 nothing behind the one set is the network's: the same
    bits with a second set's worth of NaN behind it as with the policy's own buffer.  With the set that reads k = 1012, 1013
    (exact), and with random weights (fc1_b and fc2_w, which follow fc1_w in a set, non-zero)."""
    sets = [s for s in cases.selector_sets() if 1013 in s["ks"] or 1012 in s["ks"]]
    assert len(sets) == 2
    rng = np.random.default_rng(5)
    for w, A in [(cases.selector_weights(sets[:1], 1), cases.SELECTOR_A), (cases.selector_weights(sets[1:], -1), cases.SELECTOR_A),
                 (policy_ref.random_weights(rng, 1, 8), 8)]:
        pol = ConvFCPolicy(A, 1).load_arrays(w).to(DEV)
        obs = _dev(cases.random_obs(rng, 17, 2))
        lg, v = abi.conv_fc(pol, obs)
        behind = torch.full((2 * pol.set_floats,), float("nan"), device=DEV)
        behind[: pol.set_floats] = pol.packed()
        lg2, v2 = abi.conv_fc(pol, obs, weights=behind, num_sets=1)
        assert torch.isfinite(lg).all() and torch.isfinite(v).all()
        assert _same(lg, lg2) and _same(v, v2)


@pytest.mark.parametrize("B,N,P,A", [(17, 3, 3, 15), (33, 2, 1, 8)])
def test_integer_network_is_exact(B, N, P, A):
    """Every partial sum an integer below 2^24 (test_policy_shapes_cpu.py proves it of the construction): the float32 result is
    the int64 one in any order of summation, and a dropped or doubled k of fc1 moves it (no fc1 weight is zero)."""
    wi = cases.integer_weights(P, A)
    el, ev, ef = cases.integer_expected(wi, B, N)
    assert (ef == 0).any() and (ef > 0).any(), "both branches of the ReLUs"
    obs = _dev(cases.random_obs(np.random.default_rng(B), B, N))
    lg, v = abi.conv_fc(ConvFCPolicy(A, P).load_arrays(wi).to(DEV), obs)
    assert same_bits(_np(lg), el.astype(np.float32)) and same_bits(_np(v), ev.astype(np.float32))
    # the same trunk in features mode (the recurrent policy's): fc2's output, exact
    rec = ConvLSTMPolicy(A, P, 64)
    rec.load_arrays({**{k: _np(getattr(rec, k)) for k, _, _ in rec.layout()}, **{k: wi[k] for k in list(wi)[:6]}})
    state = torch.zeros((B, N, 2, 64), device=DEV)
    feat = abi.lstm(rec.to(DEV), obs, state)[3]
    assert same_bits(_np(feat), ef.astype(np.float32))


# ------------------------------------------------------------------------------------------------------ 3. LSTM
@pytest.mark.parametrize("case", cases.LSTM_CASES, ids=lambda c: "B%d-N%d-P%d-A%d-C%d" % c)
def test_lstm_against_restatement(case):
    B, N, P, A, Cs = case
    w, obs_h, state_h, starts_h = cases.lstm_inputs(case)
    pol = ConvLSTMPolicy(A, P, Cs).load_arrays(w).to(DEV)
    obs, state, starts = _dev(obs_h), _dev(state_h), _dev(starts_h)
    if B >= 16:
        assert starts_h[:16, 0].all() and (N == 1 or not starts_h[:16, 1].any())
    lg, v, ns, feat = abi.lstm(pol, obs, state, starts)
    with torch.no_grad():
        tl, tv, ts = pol(obs, state, starts)
        tf = _trunk(pol, obs)[0].reshape(B, N, 32)
    rl, rv, rs = policy_lstm_ref.forward(w, obs_h, state_h, starts_h)
    x = policy_ref.normalise(obs_h)
    rf = np.stack([policy_lstm_ref.features_set(w, 0 if P == 1 else i, x[:, i]) for i in range(N)], axis=1)
    _bound("lstm.features", case, feat, tf, rf)
    _bound("lstm.logits", case, lg, tl, rl)
    _bound("lstm.value", case, v, tv, rv)
    _bound("lstm.c", case, ns[..., 0, :], ts[..., 0, :], rs[..., 0, :])
    _bound("lstm.h", case, ns[..., 1, :], ts[..., 1, :], rs[..., 1, :])
    assert np.ptp(rl) > 1e-2 and np.ptp(rs[..., 1, :]) > 1e-2 and np.ptp(rf) > 1e-2
    # in place: the same bits, and the one buffer's tail as untouched
    lg2, v2, ns2, feat2 = abi.lstm(pol, obs, state, starts, in_place=True)
    assert _same(lg, lg2) and _same(v, v2) and _same(ns, ns2) and _same(feat, feat2)


# ------------------------------------------------------------------------------------------------------ 4. MOA
@pytest.mark.parametrize("case", cases.MOA_CASES, ids=lambda c: "N%d-A%d-C%d-B%d-P%d" % c)
def test_moa_against_restatement(case):
    N, A, Cs, B, P = case
    w, obs_h, prev_h, state_h, starts_h, acts_h = cases.moa_inputs(case)
    pol = ConvMOAPolicy(A, N, P, Cs).load_arrays(w).to(DEV)
    obs, prev, state, starts, acts = (_dev(x) for x in (obs_h, prev_h, state_h, starts_h, acts_h))
    out = abi.moa(pol, obs, prev, state, starts, actions=acts)
    with torch.no_grad():
        tor = pol(obs, prev, state, starts)
    ref = policy_moa_ref.forward(w, obs_h, prev_h, state_h, starts_h)
    for name, t, rf in zip(("logits", "value", "moa_logits", "cf_logits", "state"), tor, ref):
        _bound("moa." + name, case, out[name], t, rf)
    assert np.ptp(ref[3]) > 1e-2 and np.ptp(ref[4][..., 2, :]) > 1e-2
    lg, cf, moa_lg, infl = out["logits"], out["cf_logits"], out["moa_logits"], out["influence"]
    # moa_logits IS the counterfactual of the own previous action (zero at a start)
    own = torch.where(starts, torch.zeros_like(prev), prev).long()
    pick = torch.gather(cf, 2, own[:, :, None, None, None].expand(B, N, 1, N - 1, A))[:, :, 0]
    assert _same(moa_lg, pick)
    # the influence: against influence() on the device's own outputs, and against the restatement's
    ti = influence(lg, cf, acts, 10.0)
    assert torch.isfinite(infl).all()
    d_t = (infl - ti).abs().max().item()
    ri = policy_moa_ref.influence(ref[0].reshape(-1, A), ref[3].reshape(-1, A, N - 1, A), acts_h.reshape(-1))
    d_r = float(np.abs(_np(infl).reshape(-1) - ri).max())
    b_t, b_r = 1e-5 + 1e-4 * ti.abs().max().item(), 1e-4 + 1e-3 * float(np.abs(ri).max())
    print("RATIO moa.influence_vs_torch %s diff %.3e bound %.3e ratio %.3f" % ("x".join(map(str, case)), d_t, b_t, d_t / b_t))
    print("RATIO moa.influence_vs_ref %s diff %.3e bound %.3e ratio %.3f" % ("x".join(map(str, case)), d_r, b_r, d_r / b_r))
    assert d_t <= b_t and d_r <= b_r
    if A == 1:
        assert (infl == 0.0).all(), "with one action every KL term is exactly zero"
    else:
        assert float(np.abs(ri).max()) > 1e-4
    # in place, and without the influence: the same bits
    inp = abi.moa(pol, obs, prev, state, starts, actions=acts, in_place=True)
    bare = abi.moa(pol, obs, prev, state, starts)
    assert bare["influence"] is None
    for k in ("logits", "value", "moa_logits", "cf_logits", "state"):
        assert _same(out[k], inp[k]), k
        assert _same(out[k], bare[k]), k
    assert _same(infl, inp["influence"])


# ------------------------------------------------------------------------------------------------------ 5. Watershed
def _ws_policy(variant, Cs=64):
    w = policy_ws_ref.random_weights(np.random.default_rng(40 + variant), variant, Cs)
    return WatershedLSTMPolicy(variant, cell_size=Cs).load_arrays(w).to(DEV), w


@pytest.mark.parametrize("variant", [_capi.SSD_WS_SEQ, _capi.SSD_WS_SEQ_COMM])
def test_watershed_rows_of_no_agent(variant):
    """include/ssd.h: a row whose agent is outside 0 .. num_sets - 1 gets zero outputs and an unwritten state_out row.  Such
    rows mixed into two tiles, and one whole tile of them (no agent present in it)."""
    pol, w = _ws_policy(variant)
    S, Cs, B = pol.num_sets, 64, 16 * 2 + 3
    rng = np.random.default_rng(variant)
    agent = rng.integers(0, S, B).astype(np.int64)
    agent[[1, 6, 15]] = [-1, S, 127]                            # tile 0: mixed
    agent[16:32] = np.resize([-1, S, 127, -128], 16)            # tile 1: nobody
    agent[33] = S                                               # tile 2 (3 real rows): mixed
    valid = (agent >= 0) & (agent < S)
    assert valid[:16].any() and not valid[16:32].any() and valid[32:].any() and not valid[32:].all()
    obs_h = policy_ws_ref.random_obs(rng, variant, False, np.where(valid, agent, 0))
    state_h = rng.standard_normal((B, 2, Cs)).astype(np.float32)
    starts_h = rng.random(B) < 0.3
    obs, ag, state, starts = _dev(obs_h), _dev(agent.astype(np.int8)), _dev(state_h), _dev(starts_h)
    dist, value, ns = abi.watershed(pol, obs, ag, state, starts)
    vt = _dev(valid)
    assert (dist[~vt] == 0).all() and (value[~vt] == 0).all()
    assert abi.unwritten(ns[~vt]).all(), "state_out of a row of no agent was written"
    assert not abi.unwritten(ns[vt]).any()
    # the valid rows: the same bits as a call with them alone, and within the bound of the restatement
    d1, v1, s1 = abi.watershed(pol, obs[vt], ag[vt], state[vt], starts[vt])
    assert _same(dist[vt], d1) and _same(value[vt], v1) and _same(ns[vt], s1)
    with torch.no_grad():
        td, tv, ts = pol(obs[vt], ag[vt].long(), state[vt], starts[vt])
    rd, rv, rs = policy_ws_ref.forward(w, obs_h[valid], agent[valid], state_h[valid], starts_h[valid])
    case = (variant, B)
    _bound("ws.dist", case, d1, td, rd)
    _bound("ws.value", case, v1, tv, rv)
    _bound("ws.h", case, s1[:, 0], ts[:, 0], rs[:, 0])
    _bound("ws.c", case, s1[:, 1], ts[:, 1], rs[:, 1])
    assert np.ptp(rd) > 1e-2
    # in place: a row of no agent keeps its state
    d2, v2, s2 = abi.watershed(pol, obs, ag, state, starts, in_place=True)
    assert _same(d2, dist) and _same(v2, value) and _same(s2[vt], ns[vt]) and _same(s2[~vt], state[~vt])


@pytest.mark.parametrize("variant", [_capi.SSD_WS_SEQ, _capi.SSD_WS_SEQ_COMM])
def test_watershed_single_row(variant):
    pol, w = _ws_policy(variant)
    S, Cs = pol.num_sets, 64
    rng = np.random.default_rng(9 + variant)
    for agent in (np.array([S - 1]), np.array([0])):
        obs_h = policy_ws_ref.random_obs(rng, variant, False, agent)
        state_h = rng.standard_normal((1, 2, Cs)).astype(np.float32)
        obs, ag, state = _dev(obs_h), _dev(agent.astype(np.int8)), _dev(state_h)
        dist, value, ns = abi.watershed(pol, obs, ag, state)
        with torch.no_grad():
            td, tv, ts = pol(obs, ag.long(), state)
        rd, rv, rs = policy_ws_ref.forward(w, obs_h, agent, state_h)
        case = (variant, 1, int(agent[0]))
        _bound("ws.dist", case, dist, td, rd)
        _bound("ws.value", case, value, tv, rv)
        _bound("ws.state", case, ns, ts, rs)
    none = abi.watershed(pol, obs, _dev(np.array([-1], np.int8)), state)
    assert (none[0] == 0).all() and (none[1] == 0).all() and abi.unwritten(none[2]).all()
