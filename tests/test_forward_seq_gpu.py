"""The sequence forwards on the MI355X (include/ssd.h, SEQUENCE FORWARD): ssd_policy_lstm_forward_seq and
ssd_policy_moa_forward_seq against the chain of per-step forwards they replace.  The contract is equality of bits, so every
comparison here is one of uint32 words: evaluate_fragment(one_call=True) against one_call=False over impala_ref.EDGE_CASES
(E = 17, N = 5: a second tile of one env; K % T == 0 with both kinds of lanes on the bootstrap's start rule; T > K; T = 1) with and
without obs_first, at all three cell sizes, state_out against the chain's carry, a scratch at its minimum (several chunks)
against one that holds the fragment, what the MOA call may not read, guard rows behind every output, inputs left as they were,
a caller's stream, and the IMPALA calls.  make_batch's behaviour policy differs from the target policy, so a ring entry is
never the state the target policy carries there: a wrong state rule shows."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import policy_abi
from a3c_ref import as_numpy_u32
from impala_ref import EDGE_CASES, EDGE_E, EDGE_N, HYPER, INFLUENCE_WEIGHT, MOA_WEIGHT, edge, edge_batch, edge_id, make_batch
from sequential_social_dilemma_games_amd import _capi, evaluate_fragment, impala_loss_moa, impala_loss_recurrent

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
KINDS = ("lstm", "moa")
NAMES = ("logits", "value", "bootstrap")
WHOLE, RAGGED, T_ONE, ONE_WINDOW, THREES = EDGE_CASES[0], EDGE_CASES[10], EDGE_CASES[7], EDGE_CASES[11], EDGE_CASES[4]
assert WHOLE[:2] == (4, 2) and RAGGED[:2] == (5, 2) and T_ONE[:2] == (3, 1) and ONE_WINDOW[:2] == (4, 8) and THREES[:2] == (6, 3)


def _to(t, dev):
    return {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in t.items()}


def _on_device(pol, t, first):
    return copy.deepcopy(pol).to(DEV), _to(t, DEV), None if first is None else first.to(DEV)


def _eval(pol, t, first, T, one_call):
    out = evaluate_fragment(pol, t, first, T, one_call=one_call)
    torch.cuda.synchronize()
    return dict(zip(NAMES, out))


def _same_bits(a, b, what=""):
    assert set(a) == set(b), what
    for name in a:
        assert a[name].shape == b[name].shape, (what, name)
        assert np.array_equal(as_numpy_u32(a[name]), as_numpy_u32(b[name])), (what, name)


def _clones(t):
    return {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in t.items()}


def _unchanged(now, before, what):
    for k, v in before.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(now[k].contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), (what, k)


def _without_first(t, first):
    return dict(t, obs=torch.cat([first.unsqueeze(0), t["obs"]]).contiguous())


# ---- 1. bit equality over the edge matrix ----

@pytest.mark.parametrize("case", EDGE_CASES, ids=edge_id)
@pytest.mark.parametrize("kind", KINDS)
def test_one_call_equals_the_chain_to_the_bit(kind, case):
    T = case[1]
    pol, t, first = _on_device(*edge_batch(kind, case))
    chain = _eval(pol, t, first, T, False)
    assert all(bool(torch.isfinite(x).all()) for x in chain.values())
    _same_bits(chain, _eval(pol, t, first, T, True), "with obs_first")
    _same_bits(chain, _eval(pol, _without_first(t, first), None, T, True), "without obs_first")


# ---- 2. the other cell sizes: 8 and 16 waves per workgroup ----

@pytest.mark.parametrize("cells", (128, 256))
@pytest.mark.parametrize("kind", KINDS)
def test_all_cell_sizes(kind, cells):
    K_, T, E, N = 3, 2, 3, 2
    pol, t, first = _on_device(*make_batch(kind, 8, N, N, K_, E, T, seed=60 + cells, C=cells, done_mode="per_env", last_done="alternate"))
    assert bool(t["done"].any()) and not bool(t["done"].all())
    chain = _eval(pol, t, first, T, False)
    _same_bits(chain, _eval(pol, t, first, T, True), "with obs_first")
    _same_bits(chain, _eval(pol, _without_first(t, first), None, T, True), "without obs_first")


# ---- the entry points through ctypes, every output with poisoned guard rows behind it ----

def _seq_call(kind, pol, t, first, T, feature_rows=None, outputs=("logits", "value", "bootstrap", "state_out")):
    """ssd_policy_{lstm,moa}_forward_seq on the current stream -> {output: tensor}, feature_rows (default: the whole fragment's)
    in a scratch of exactly that size; the guard rows behind each output and behind the scratch must still hold their fill."""
    K_, E, N = (int(n) for n in t["actions"].shape)
    A, Cs = pol.num_actions, pol.cell_size
    rows = (K_ + 1) * E * N if feature_rows is None else feature_rows
    bufs = {"logits": policy_abi.Tailed("logits", K_, (E, N, A), DEV), "value": policy_abi.Tailed("value", K_, (E, N), DEV),
            "bootstrap": policy_abi.Tailed("bootstrap_value", E, (N,), DEV), "state_out": policy_abi.Tailed("state_out", E, (N, 2, Cs), DEV)}
    bufs = {k: v for k, v in bufs.items() if k in outputs}
    feat = policy_abi.Tailed("features", rows, (32,), DEV)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())            # noqa: E731
    out = lambda k: p(bufs[k].full) if k in bufs else None                   # noqa: E731
    L = _capi.lib()
    fn = L.ssd_policy_moa_forward_seq if kind == "moa" else L.ssd_policy_lstm_forward_seq
    rc = fn(p(pol.packed()), pol.num_sets, A, Cs, T, p(first), p(t["obs"]), p(t["state"]), p(t.get("done")), K_, E, N, p(feat.full), rows,
            out("logits"), out("value"), out("bootstrap"), out("state_out"), 0, 0,
            C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    _capi.policy_check(rc)
    torch.cuda.synchronize()
    for b in list(bufs.values()) + [feat]:
        b.check_tail()
    got = {k: b.view for k, b in bufs.items()}
    for k, v in got.items():
        assert not bool(policy_abi.unwritten(v).any()), k                    # and every row of the body was written
    return got


def _chain(kind, pol, t, first, T):
    """The per-step forwards chained under the state rule, through the C ABI -> (logits, value, the carry after step K - 1)."""
    K_ = int(t["actions"].shape[0])
    done, carry, lgs, vs = t.get("done"), None, [], []
    for k in range(K_):
        o = first if k == 0 else t["obs"][k - 1]
        s_in, starts = (t["state"][k // T], None) if k % T == 0 else (carry, None if done is None else done[k - 1])
        if kind == "lstm":
            lg, v, carry, _ = policy_abi.lstm(pol, o, s_in, starts)
        else:
            out = policy_abi.moa(pol, o, t["prev_actions"][k], s_in, starts)
            lg, v, carry = out["logits"], out["value"], out["state"]
        lgs.append(lg.clone())
        vs.append(v.clone())
        carry = carry.clone()
    return torch.stack(lgs), torch.stack(vs), carry


# ---- 3. state_out ----

@pytest.mark.parametrize("case", [WHOLE, RAGGED, ONE_WINDOW], ids=edge_id)
@pytest.mark.parametrize("kind", KINDS)
def test_state_out_is_the_chains_carry_after_the_last_step(kind, case):
    """... with the bootstrap step run after it (K % T == 0 and ragged), and alone, every other output NULL."""
    T = case[1]
    pol, t, first = _on_device(*edge_batch(kind, case))
    logits, value, carry = _chain(kind, pol, t, first, T)
    want = {"logits": logits, "value": value, "state_out": carry if kind == "lstm" else carry[:, :, :2].contiguous()}
    got = _seq_call(kind, pol, t, first, T)
    _same_bits(want, {k: got[k] for k in want}, "all outputs")
    _same_bits({"state_out": want["state_out"]}, _seq_call(kind, pol, t, first, T, outputs=("state_out",)), "state_out alone")
    _same_bits({"bootstrap": got["bootstrap"]}, _seq_call(kind, pol, t, first, T, outputs=("bootstrap",)), "bootstrap alone")


# ---- 4. chunks ----

@pytest.mark.parametrize("case", [T_ONE, RAGGED, THREES, WHOLE, ONE_WINDOW], ids=edge_id)
@pytest.mark.parametrize("kind", KINDS)
def test_a_scratch_at_its_minimum_gives_the_same_bits(kind, case):
    """feature_rows = (min(T, K) + 1) E N: one window per chunk, the last window with the bootstrap row (and, where K % T == 0
    and the scratch holds two windows but not the bootstrap row, the last window held back for it); then a scratch of one
    more step, and of two windows.  T = 1: four chunks for K = 3."""
    K_, T = case[:2]
    pol, t, first = _on_device(*edge_batch(kind, case))
    step = EDGE_E * EDGE_N
    whole = _seq_call(kind, pol, t, first, T)
    least = (min(T, K_) + 1) * step
    for rows in sorted({least, least + step - 1, least + step, 2 * T * step}):
        if rows >= least:
            _same_bits(whole, _seq_call(kind, pol, t, first, T, feature_rows=rows), rows)
    _same_bits(whole, _seq_call(kind, pol, _without_first(t, first), None, T, feature_rows=least), "without obs_first")


# ---- 5. the MOA call reads the actions branch's inputs alone ----

@pytest.mark.parametrize("case", [WHOLE, RAGGED], ids=edge_id)
def test_the_moa_call_reads_neither_prev_actions_nor_the_moa_cells_state(case):
    T = case[1]
    pol, t, first = _on_device(*edge_batch("moa", case))
    want = _eval(pol, t, first, T, True)
    bare = {k: v for k, v in t.items() if k != "prev_actions"}
    bare["state"] = t["state"].clone()
    bare["state"][:, :, :, 2:] = float("nan")
    _same_bits(want, _eval(pol, bare, first, T, True))
    with pytest.raises(ValueError, match="prev_actions"):                     # the chain's MOA forward does read it
        evaluate_fragment(pol, bare, first, T)


# ---- 6. nothing beyond the fragment is read, every input is left as it was (the guard rows: _seq_call) ----

@pytest.mark.parametrize("case", [WHOLE, RAGGED], ids=edge_id)
@pytest.mark.parametrize("kind", KINDS)
def test_nothing_beyond_the_fragment_is_read(kind, case):
    """The obs rows after the last one read differ (all 255 against all 0) and two more ring entries are NaN: the same bits.
    At K % T == 0 ring entry K // T is there to be taken, and the bootstrap row must use the carried state."""
    T = case[1]
    pol, t, first = _on_device(*edge_batch(kind, case))
    exact = _eval(pol, t, first, T, True)
    nan = torch.full((2,) + tuple(t["state"].shape[1:]), float("nan"), dtype=torch.float32, device=DEV)
    for fill in (0, 255):
        more = torch.full((2,) + tuple(t["obs"].shape[1:]), fill, dtype=torch.uint8, device=DEV)
        longer = dict(t, obs=torch.cat([t["obs"], more]).contiguous(), state=torch.cat([t["state"], nan]).contiguous())
        _same_bits(exact, _eval(pol, longer, first, T, True), "with obs_first")
        longer["obs"] = torch.cat([first.unsqueeze(0), t["obs"], more]).contiguous()
        _same_bits(exact, _eval(pol, longer, None, T, True), "without obs_first")


@pytest.mark.parametrize("case", [T_ONE, WHOLE], ids=edge_id)
@pytest.mark.parametrize("kind", KINDS)
def test_inputs_are_left_as_they_were(kind, case):
    pol, t, first = _on_device(*edge_batch(kind, case))
    before, first_before = _clones(t), first.clone()
    params = {name: p.detach().clone() for name, p in pol.named_parameters()}
    _eval(pol, t, first, case[1], True)
    _seq_call(kind, pol, t, first, case[1], feature_rows=(min(case[1], case[0]) + 1) * EDGE_E * EDGE_N)
    _unchanged(t, before, "batch")
    assert torch.equal(first, first_before)
    _unchanged({name: p.detach() for name, p in pol.named_parameters()}, params, "parameters")


@pytest.mark.parametrize("kind", KINDS)
def test_the_kept_scratch_serves_smaller_and_larger_calls(kind):
    case = edge(4, 2, "per_env", seed=31)
    pol = None
    for E in (33, 1, 17):
        p, t, first = edge_batch(kind, case, E=E)
        if pol is None:
            pol = copy.deepcopy(p).to(DEV)
            assert not hasattr(pol, "_eval_seq_scratch")
        t, first = _to(t, DEV), first.to(DEV)
        kept = getattr(pol, "_eval_seq_scratch", None)
        got = _eval(pol, t, first, case[1], True)
        if E == 1:
            assert pol._eval_seq_scratch is kept                  # reused, not allocated anew
        assert not hasattr(pol, "_eval_scratch")                  # the chain's scratch is not this path's
        _same_bits(got, _eval(copy.deepcopy(p).to(DEV), t, first, case[1], False), E)


# ---- 7. a caller's stream ----

@pytest.mark.parametrize("kind", KINDS)
def test_a_stream_of_the_callers(kind):
    p, t, first = edge_batch(kind, RAGGED)
    want = _eval(*_on_device(p, t, first), RAGGED[1], False)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        pol = copy.deepcopy(p).to(DEV)
        dt, dfirst = _to(t, DEV), first.to(DEV)
        out = evaluate_fragment(pol, dt, dfirst, RAGGED[1], one_call=True)
    s.synchronize()
    _same_bits(want, dict(zip(NAMES, out)))


# ---- 8. the IMPALA calls ----

def _impala(kind, pol, t, first, T, one_call):
    pol.zero_grad()
    if kind == "lstm":
        loss, stats = impala_loss_recurrent(pol, t, seq_len=T, obs_first=first, one_call=one_call, **HYPER)
    else:
        loss, stats = impala_loss_moa(pol, t, seq_len=T, moa_weight=MOA_WEIGHT, influence_weight=INFLUENCE_WEIGHT, obs_first=first,
                                      one_call=one_call, **HYPER)
    loss.backward()
    torch.cuda.synchronize()
    d = {"loss": loss.detach()}
    d.update({"stat " + k: v for k, v in stats.items()})
    for name, _, _ in pol.layout():
        g = getattr(pol, name).grad
        d["grad " + name] = torch.zeros_like(getattr(pol, name)).detach() if g is None else g.detach().clone()
    return d


@pytest.mark.parametrize("kind,case", [("lstm", RAGGED), ("moa", WHOLE)], ids=lambda x: x if isinstance(x, str) else edge_id(x))
def test_the_impala_calls_give_the_same_loss_and_gradients(kind, case):
    pol, t, first = _on_device(*edge_batch(kind, case))
    _same_bits(_impala(kind, pol, t, first, case[1], False), _impala(kind, pol, t, first, case[1], True))
