"""evaluate_fragment on the MI355X at its edges: policy._evaluate_device's addressing -- which observation
row a step reads, when a step reads the state ring and when the carried state, the bootstrap as row K of one allocation,
logits[1:] as an output pointer, one carry buffer that is a launch's input and output, the scratch kept on the policy --
over impala_ref.EDGE_CASES (E = 17, N = 5: two 16-row tiles per weight set, the second with one row) against the float64
restatement with the float32 CPU path as the yardstick (ek <= 4 et + 1e-6 max(1, max |ref|) per output); everything else is
equality of bits: obs_first=None against the obs_first form, tensors longer than the fragment, inputs left as they were, the
kept scratch, a caller's stream, state_in, views with a storage offset, and the refusals.  The loss cannot see the bootstrap
row's start rule (test_impala_loss_cpu.py), so the three outputs are compared themselves."""
import copy

import numpy as np
import pytest
import torch

from a3c_ref import as_numpy_u32, max_err
from impala_ref import (EDGE_CASES, EDGE_E, EDGE_N, HYPER, INFLUENCE_WEIGHT, MOA_WEIGHT, edge, edge_batch, edge_id, evaluate)
from sequential_social_dilemma_games_amd import evaluate_fragment, impala_loss, impala_loss_moa, impala_loss_recurrent

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
KINDS = ("fc", "lstm", "moa")
SEQ = ("lstm", "moa")
NAMES = ("logits", "value", "bootstrap")
WHOLE, RAGGED, T_ONE, ONE_WINDOW = EDGE_CASES[0], EDGE_CASES[10], EDGE_CASES[7], EDGE_CASES[11]
assert WHOLE[:2] == (4, 2) and RAGGED[:2] == (5, 2) and T_ONE[:2] == (3, 1) and ONE_WINDOW[:2] == (4, 8)


def _to(t, dev):
    return {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in t.items()}


def _on_device(pol, t, first):
    return copy.deepcopy(pol).to(DEV), _to(t, DEV), None if first is None else first.to(DEV)


def _eval(pol, t, first, T):
    out = evaluate_fragment(pol, t, first, T)
    torch.cuda.synchronize()
    return dict(zip(NAMES, out))


def _same_bits(a, b, what=""):
    for name in a:
        assert a[name].shape == b[name].shape, (what, name)
        assert np.array_equal(as_numpy_u32(a[name]), as_numpy_u32(b[name])), (what, name)


def _clones(t):
    return {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in t.items()}


def _unchanged(now, before, what):
    for k, v in before.items():
        if isinstance(v, torch.Tensor):
            assert now[k].dtype == v.dtype and now[k].shape == v.shape, (what, k)
            assert torch.equal(now[k].contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), (what, k)


# ---- a. the matrix against float64 ----

@pytest.mark.parametrize("case", EDGE_CASES, ids=edge_id)
@pytest.mark.parametrize("kind", KINDS)
def test_the_matrix_against_float64(kind, case):
    K_, T = case[:2]
    pol, t, first = edge_batch(kind, case)
    done = t.get("done")
    if case[2] == "per_env":
        share = float(done[K_ - 1].double().mean())
        assert 0.25 <= share <= 0.75, share                       # trajectories that end on the last row, and that do not
    with torch.no_grad():
        ref = evaluate(kind, copy.deepcopy(pol).double(), t, first, T)
    ref = dict(zip(NAMES, (ref[0], ref[1], ref[3])))
    yard = dict(zip(NAMES, evaluate_fragment(pol, t, first, T)))  # the float32 CPU path
    got = _eval(*_on_device(pol, t, first), T)
    assert tuple(got["logits"].shape) == (K_, EDGE_E, EDGE_N, case[4]) and tuple(got["value"].shape) == (K_, EDGE_E, EDGE_N)
    assert tuple(got["bootstrap"].shape) == (EDGE_E, EDGE_N)
    assert all(x.dtype == torch.float32 and x.device.type == "cuda" and bool(torch.isfinite(x).all()) for x in got.values())
    bad, bounds = [], {}
    for name in NAMES:
        ek, et = max_err(got[name], ref[name]), max_err(yard[name], ref[name])
        scale = max(1.0, float(ref[name].abs().max()))
        bounds[name] = 4.0 * et + 1e-6 * scale
        print("%s %s %-9s ek %.3e et %.3e max|ref| %.3e  %.2f of the bound" % (kind, edge_id(case), name, ek, et, scale, ek / bounds[name]))
        if not ek <= bounds[name]:
            bad.append((name, ek, et))
    ended = torch.zeros((EDGE_E, EDGE_N), dtype=torch.bool) if done is None else done[K_ - 1].bool()
    for what, lanes in (("bootstrap where done[K - 1]", ended), ("bootstrap where not done[K - 1]", ~ended)):
        if bool(lanes.any()):
            ek = max_err(got["bootstrap"].cpu()[lanes], ref["bootstrap"][lanes])
            print("%s %s %-31s ek %.3e on %d lanes" % (kind, edge_id(case), what, ek, int(lanes.sum())))
            if not ek <= bounds["bootstrap"]:
                bad.append((what, ek, bounds["bootstrap"]))
    assert not bad, (kind, edge_id(case), bad)


# ---- b. obs_first=None ----

@pytest.mark.parametrize("case", [WHOLE, RAGGED], ids=edge_id)
@pytest.mark.parametrize("kind", KINDS)
def test_without_obs_first_to_the_bit(kind, case):
    """obs = cat([first, obs]): for the conv-FC policy one launch of (K + 1) E rows against launches of E and K E rows; for
    the recurrent policies obs[k] and obs[K] against obs_first, obs[k - 1] and obs[K - 1]."""
    pol, t, first = _on_device(*edge_batch(kind, case))
    t2 = dict(t, obs=torch.cat([first.unsqueeze(0), t["obs"]]).contiguous())
    _same_bits(_eval(pol, t, first, case[1]), _eval(pol, t2, None, case[1]))


# ---- c. nothing beyond the fragment is read ----

@pytest.mark.parametrize("case", [WHOLE, RAGGED], ids=edge_id)
@pytest.mark.parametrize("kind", KINDS)
def test_nothing_beyond_the_fragment_is_read(kind, case):
    """Two more ring entries, NaN, and three more rows of obs, random bytes: the outputs are those of the exact-length
    tensors.  At K % T == 0 ring entry K // T is there to be read, and the bootstrap row must take the carried state."""
    pol, t, first = _on_device(*edge_batch(kind, case))
    exact = _eval(pol, t, first, case[1])
    g = torch.Generator().manual_seed(77)
    more = torch.randint(0, 256, (3,) + tuple(t["obs"].shape[1:]), dtype=torch.uint8, generator=g).to(DEV)
    longer = dict(t, obs=torch.cat([t["obs"], more]).contiguous())
    if kind != "fc":
        nan = torch.full((2,) + tuple(t["state"].shape[1:]), float("nan"), dtype=torch.float32, device=DEV)
        longer["state"] = torch.cat([t["state"], nan]).contiguous()
    _same_bits(exact, _eval(pol, longer, first, case[1]), "with obs_first")
    # and without obs_first: the bootstrap's row is obs[K], the rows after it are the random ones
    longer["obs"] = torch.cat([first.unsqueeze(0), t["obs"], more]).contiguous()
    _same_bits(exact, _eval(pol, longer, None, case[1]), "without obs_first")


# ---- d. inputs are data ----

@pytest.mark.parametrize("case", [T_ONE, WHOLE], ids=edge_id)
@pytest.mark.parametrize("kind", SEQ)
def test_inputs_are_left_as_they_were(kind, case):
    """Every tensor of the batch, obs_first and every parameter after a call, against clones taken before: the carried state,
    a launch's input and output, never lands in the ring (at T = 1 every loss row reads the ring)."""
    pol, t, first = _on_device(*edge_batch(kind, case))
    before, first_before = _clones(t), first.clone()
    params = {name: p.detach().clone() for name, p in pol.named_parameters()}
    _eval(pol, t, first, case[1])
    _unchanged(t, before, "batch")
    assert torch.equal(first, first_before)
    _unchanged({name: p.detach() for name, p in pol.named_parameters()}, params, "parameters")


# ---- e. the kept scratch and repeats ----

@pytest.mark.parametrize("kind", SEQ)
def test_the_kept_scratch_serves_smaller_and_larger_calls(kind):
    """E = 33, then E = 1 (the kept scratch is larger than needed), then E = 17, on one policy: each result is that of a fresh
    copy of the policy that has no scratch yet, and a second identical call gives equal bits."""
    case = edge(4, 2, "per_env", seed=31)
    pol = None
    for E in (33, 1, 17):
        p, t, first = edge_batch(kind, case, E=E)
        if pol is None:
            pol = copy.deepcopy(p).to(DEV)
            assert not hasattr(pol, "_eval_scratch")
        fresh = copy.deepcopy(p).to(DEV)
        t, first = _to(t, DEV), first.to(DEV)
        kept = getattr(pol, "_eval_scratch", None)
        got = _eval(pol, t, first, case[1])
        if E == 1:
            assert pol._eval_scratch is kept                      # reused, not allocated anew
        _same_bits(got, _eval(fresh, t, first, case[1]), E)
        _same_bits(got, _eval(pol, t, first, case[1]), E)


# ---- f. a caller's stream ----

@pytest.mark.parametrize("kind", KINDS)
def test_a_stream_of_the_callers(kind):
    p, t, first = edge_batch(kind, RAGGED)
    want = _eval(*_on_device(p, t, first), RAGGED[1])
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        pol = copy.deepcopy(p).to(DEV)
        dt, dfirst = _to(t, DEV), first.to(DEV)
        out = evaluate_fragment(pol, dt, dfirst, RAGGED[1])
    s.synchronize()
    _same_bits(want, dict(zip(NAMES, out)))


# ---- g. state_in in place of state ----

@pytest.mark.parametrize("kind", SEQ)
def test_state_in_serves_one_window(kind):
    K_, T = ONE_WINDOW[:2]
    pol, t, first = _on_device(*edge_batch(kind, ONE_WINDOW))
    assert T >= K_ and t["state"].shape[0] == 1
    t2 = {k: v for k, v in t.items() if k != "state"}
    t2["state_in"] = t["state"][0].clone()
    _same_bits(_eval(pol, dict(t, state=t2["state_in"].unsqueeze(0)), first, T), _eval(pol, t2, first, T))


# ---- h. views ----

def _minibatch(kind, clone):
    """Steps 2 .. 5 of a fragment of K = 7, T = 2 by the documented slice rule (k0 a multiple of T, obs_first = obs[k0 - 1],
    state[k0 // T:]): K % T == 0 inside longer tensors, every tensor a view with a storage offset -- or, with clone, the same
    data in fresh tensors of exactly the fragment's length."""
    k0, k1, T = 2, 6, 2
    pol, t, _ = edge_batch(kind, edge(7, T, "per_env", seed=41))
    pol, t = copy.deepcopy(pol).to(DEV), _to(t, DEV)
    mb = {k: v[k0:k1] for k, v in t.items() if k not in ("state", "last_value")}
    first = t["obs"][k0 - 1]
    if kind != "fc":
        mb["state"] = t["state"][k0 // T:]
    if clone:
        mb, first = _clones(mb), first.clone()
        if kind != "fc":
            mb["state"] = mb["state"][:(k1 - k0) // T].clone()
    else:
        assert all(v.storage_offset() > 0 and v.is_contiguous() for v in mb.values()) and first.storage_offset() > 0
    return pol, mb, first, T


def _impala(kind, pol, t, first, T):
    pol.zero_grad()
    if kind == "fc":
        loss, stats = impala_loss(pol, t, obs_first=first, **HYPER)
    elif kind == "lstm":
        loss, stats = impala_loss_recurrent(pol, t, seq_len=T, obs_first=first, **HYPER)
    else:
        loss, stats = impala_loss_moa(pol, t, seq_len=T, moa_weight=MOA_WEIGHT, influence_weight=INFLUENCE_WEIGHT, obs_first=first, **HYPER)
    loss.backward()
    torch.cuda.synchronize()
    d = {"loss": loss.detach()}
    d.update({"stat " + k: v for k, v in stats.items()})
    for name, _, _ in pol.layout():
        g = getattr(pol, name).grad
        d["grad " + name] = torch.zeros_like(getattr(pol, name)).detach() if g is None else g.detach().clone()
    return d


@pytest.mark.parametrize("kind", KINDS)
def test_a_minibatch_of_views(kind):
    pol, mb, first, T = _minibatch(kind, clone=False)
    pol2, mb2, first2, _ = _minibatch(kind, clone=True)
    _same_bits(_eval(pol, mb, first, T), _eval(pol2, mb2, first2, T), "evaluate_fragment")
    _same_bits(_impala(kind, pol, mb, first, T), _impala(kind, pol2, mb2, first2, T), "impala_loss")


# ---- i. refusals with device tensors ----

@pytest.mark.parametrize("kind", KINDS)
def test_refusals_leave_the_scratch_alone(kind):
    K_, T = WHOLE[:2]
    p, t, first = edge_batch(kind, WHOLE)
    pol, t, first = _on_device(p, t, first)
    sentinel = None
    if kind != "fc":
        _eval(pol, t, first, T)                                   # the scratch of this shape
        pol._eval_scratch.fill_(-7.5)
        sentinel = pol._eval_scratch
        p._eval_scratch = sentinel                                # the CPU policy's too
    swapped = t["obs"].transpose(3, 4)
    assert tuple(swapped.shape) == tuple(t["obs"].shape) and not swapped.is_contiguous()
    refused = [(pol, t, None),                                    # obs with K rows and no obs_first: obs[K] is missing
               (p, t, first),                                     # a CPU policy
               (pol, dict(t, obs=swapped), first)]
    if kind != "fc":
        refused += [(pol, dict(t, state=t["state"].double()), first),
                    (pol, dict(t, state=t["state"][:-(-K_ // T) - 1]), first)]
    for who, batch, f in refused:
        with pytest.raises(ValueError):
            evaluate_fragment(who, batch, f, T)
    torch.cuda.synchronize()
    if kind != "fc":
        assert pol._eval_scratch is sentinel and p._eval_scratch is sentinel
        assert bool((sentinel == -7.5).all())
