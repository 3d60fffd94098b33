"""impala_loss, impala_loss_recurrent and impala_loss_moa without a GPU: the CPU paths -- evaluate_fragment
in plain torch, the importance weights, postprocessing.vtrace's NumPy path and a3c_terms on the detached targets -- against
the float64 autograd restatement of impala_ref.py, on fragments built as a3c_ref.make_inputs builds them with a behaviour
policy that differs from the target; the power of the suites' bound against four wrong losses; the argument checks.
Then the edge matrix the device suites share (impala_ref.EDGE_CASES, E = 17, N = 5): the same two agreements at every case,
the obs_first=None form, and the power of the bound on evaluate_fragment's own outputs against five wrong evaluation rules,
one of which no loss can see."""
import copy
import functools

import pytest
import torch

import impala_ref
from a3c_ref import bound, max_err
from impala_ref import (EDGE_CASES, EDGE_E, EDGE_N, HYPER, INFLUENCE_WEIGHT, MOA_WEIGHT, VARIANTS, autograd_loss, edge_batch, edge_id,
                        eval_variant_applies, eval_variants_of, make_batch)
from sequential_social_dilemma_games_amd import evaluate_fragment, impala_loss, impala_loss_moa, impala_loss_recurrent
from sequential_social_dilemma_games_amd.policy import A3C_STATS, MOA_A3C_STATS

KINDS = ("fc", "lstm", "moa")
A, C, E, N, K, T = 8, 64, 3, 2, 5, 2                            # two full windows and a ragged one
# a float64 policy on the CPU path and the restatement round at the same places (vtrace's float32 interface), so what is left
# is float64 rounding in sums of some tens of rows with terms up to max |ref|
EQUAL = 1e-11


def run(kind, pol, t, first, h=HYPER, T_=T):
    """The kind's loss + backward through the package -> (loss, stats, {param: grad})."""
    pol.zero_grad()
    if kind == "fc":
        loss, stats = impala_loss(pol, t, obs_first=first, **h)
    elif kind == "lstm":
        loss, stats = impala_loss_recurrent(pol, t, seq_len=T_, obs_first=first, **h)
    else:
        loss, stats = impala_loss_moa(pol, t, seq_len=T_, moa_weight=MOA_WEIGHT, influence_weight=INFLUENCE_WEIGHT, obs_first=first, **h)
    loss.backward()
    grads = {}
    for name, _, _ in pol.layout():
        g = getattr(pol, name).grad
        grads[name] = torch.zeros_like(getattr(pol, name)).detach() if g is None else g.detach().clone()
    return loss.detach(), stats, grads


def flat(out):
    """One dict of everything a call returns: the loss, the statistics and the gradients."""
    loss, stats, grads = out[:3]
    d = {"loss": loss}
    d.update({"stat " + k: v for k, v in stats.items()})
    d.update({"grad " + k: v for k, v in grads.items()})
    return d


@pytest.mark.parametrize("P", [1, N])
@pytest.mark.parametrize("kind", KINDS)
def test_cpu_path_equals_the_float64_restatement(kind, P):
    pol, t, first = make_batch(kind, A, N, P, K, E, T, seed=3 + P)
    assert t["done"][K - 1].any() and t["done"][:K - 1].any()    # done on the last row, and inside a window
    ref = autograd_loss(kind, pol, t, HYPER, first, T)
    rhos = ref[3]
    print("rho quantiles", torch.quantile(rhos.flatten(), torch.tensor([0.0, 0.1, 0.5, 0.9, 1.0], dtype=torch.float64)).tolist())
    assert (rhos < 1).double().mean() >= 0.1 and (rhos > 1).double().mean() >= 0.1
    got = run(kind, copy.deepcopy(pol).double(), t, first)
    assert tuple(got[1]) == (MOA_A3C_STATS if kind == "moa" else A3C_STATS)
    got, ref = flat(got), flat(ref)
    for name in ref:
        e, scale = max_err(got[name], ref[name]), max(1.0, float(ref[name].abs().max()))
        print("%-22s err %.3e max|ref| %.3e" % (name, e, scale))
        assert e <= EQUAL * scale, name
    # and the float32 policy, the one the device runs: its error is the yardstick of the GPU suite
    got32 = flat(run(kind, pol, t, first))
    for name in ref:
        assert got32[name].dtype in (torch.float32, torch.float64) and bool(torch.isfinite(got32[name]).all())
        assert max_err(got32[name], ref[name]) <= 1e-3 * max(1.0, float(ref[name].abs().max())), name


@pytest.mark.parametrize("kind", KINDS)
def test_the_bound_notices_four_wrong_losses(kind):
    """Each variant's distance from the restatement, over the bound 4 et + 1e-6 max(1, max |ref|) with et the float32 CPU
    path's error: the largest factor over the tensors must be clear of 1 (10 and more)."""
    pol, t, first = make_batch(kind, A, N, N, K, E, T, seed=11)
    ref = flat(autograd_loss(kind, pol, t, HYPER, first, T))
    got32 = flat(run(kind, pol, t, first))
    bounds = {name: bound(ref[name], max_err(got32[name], ref[name])) for name in ref}
    for name in ref:
        assert max_err(got32[name], ref[name]) <= bounds[name]
    for variant in VARIANTS:
        wrong = flat(autograd_loss(kind, pol, t, HYPER, first, T, variant=variant))
        factors = {name: max_err(wrong[name], ref[name]) / bounds[name] for name in ref}
        worst = max(factors, key=factors.get)
        print("%s %-16s largest factor %.3g (%s); loss factor %.3g" % (kind, variant, factors[worst], worst, factors["loss"]))
        assert factors[worst] >= 10.0, (variant, factors)


@pytest.mark.parametrize("kind", KINDS)
def test_evaluate_fragment_follows_the_state_rule(kind):
    pol, t, first = make_batch(kind, A, N, N, K, E, T, seed=21)
    p64 = copy.deepcopy(pol).double()
    logits, value, boot = evaluate_fragment(p64, t, first, T)
    assert not (logits.requires_grad or value.requires_grad or boot.requires_grad)
    assert tuple(logits.shape) == (K, E, N, A) and tuple(value.shape) == (K, E, N) and tuple(boot.shape) == (E, N)
    with torch.no_grad():
        r_logits, r_value, _, r_boot = impala_ref.evaluate(kind, p64, t, first, T)
    for a, b in ((logits, r_logits), (value, r_value), (boot, r_boot)):
        assert max_err(a, b) <= 1e-12 * max(1.0, float(b.abs().max()))
    # without obs_first row k reads obs[k] and the bootstrap obs[K]: one row more
    t2 = dict(t, obs=torch.cat([first.unsqueeze(0), t["obs"]]))
    logits2, value2, boot2 = evaluate_fragment(p64, t2, None, T)
    assert torch.equal(logits2, logits) and torch.equal(value2, value) and torch.equal(boot2, boot)
    with pytest.raises(ValueError):
        evaluate_fragment(p64, t, None, T)                       # obs[K] is missing


def test_argument_checks():
    pol, t, first = make_batch("lstm", A, N, N, K, E, T, seed=31)
    fc, tf, ff = make_batch("fc", A, N, N, K, E, T, seed=32)
    moa, tm, fm = make_batch("moa", A, N, N, K, E, T, seed=33)
    for key in ("logp", "rew"):
        with pytest.raises(ValueError, match=key):
            impala_loss_recurrent(pol, {k: v for k, v in t.items() if k != key}, seq_len=T, obs_first=first)
        with pytest.raises(ValueError, match=key):
            impala_loss(fc, {k: v for k, v in tf.items() if k != key}, obs_first=ff)
    with pytest.raises(ValueError, match="influence"):
        impala_loss_moa(moa, {k: v for k, v in tm.items() if k != "influence"}, seq_len=T, moa_weight=1.0, obs_first=fm)
    with pytest.raises(ValueError):
        impala_loss(pol, t, obs_first=first)                     # the wrong policy class
    with pytest.raises(ValueError):
        impala_loss_recurrent(fc, tf, seq_len=T, obs_first=ff)
    with pytest.raises(ValueError):
        impala_loss_moa(pol, t, seq_len=T, moa_weight=1.0, obs_first=first)
    with pytest.raises(ValueError):
        impala_loss_recurrent(pol, t, seq_len=0, obs_first=first)
    with pytest.raises(ValueError):
        impala_loss_recurrent(pol, dict(t, logp=t["logp"].double()), seq_len=T, obs_first=first)
    with pytest.raises(ValueError):
        impala_loss_recurrent(pol, dict(t, obs=t["obs"][:K - 1]), seq_len=T, obs_first=first)    # the bootstrap's row
    with pytest.raises(ValueError):
        impala_loss_recurrent(pol, t, seq_len=T, obs_first=first, clip_rho_threshold=0.0)
    with pytest.raises(ValueError):
        impala_loss_recurrent(pol, tuple(t.values()), seq_len=T, obs_first=first)


# ---- the edge matrix: E = 17, N = 5, (K, T) with whole windows only, K < T, T = 1, ragged, T > K; four done modes ----

@functools.lru_cache(maxsize=None)
def edge_inputs(kind, case):
    """(policy, batch, obs_first) of a case, built once and read only.  The ring has one entry more than the windows need:
    nothing but the "boot_from_ring" rule may read it."""
    return edge_batch(kind, case, ring_extra=1)


def last_row_condition(t, case):
    """The "per_env" cases end every other env on the last row: at least a quarter of the trajectories on each side."""
    K, done = case[0], t.get("done")
    assert (done is None) == (case[2] == "none")
    if case[2] == "per_env":
        share = float(done[K - 1].double().mean())
        assert 0.25 <= share <= 0.75, share


@pytest.mark.parametrize("case", EDGE_CASES, ids=edge_id)
@pytest.mark.parametrize("kind", KINDS)
def test_edge_matrix_equals_the_float64_restatement(kind, case):
    K_, T_ = case[:2]
    pol, t, first = edge_inputs(kind, case)
    last_row_condition(t, case)
    ref = autograd_loss(kind, pol, t, HYPER, first, T_)
    rhos = ref[3]
    low, high = float((rhos < 1).double().mean()), float((rhos > 1).double().mean())
    print("rho: %.2f below 1, %.2f above, of %d" % (low, high, rhos.numel()))
    assert low >= 0.1 and high >= 0.1
    p64 = copy.deepcopy(pol).double()
    got, ref = flat(run(kind, p64, t, first, T_=T_)), flat(ref)
    for name in ref:
        e, scale = max_err(got[name], ref[name]), max(1.0, float(ref[name].abs().max()))
        print("%-22s err %.3e max|ref| %.3e" % (name, e, scale))
        assert e <= EQUAL * scale, name
    logits, value, boot = evaluate_fragment(p64, t, first, T_)
    assert tuple(logits.shape) == (K_, EDGE_E, EDGE_N, case[4]) and tuple(value.shape) == (K_, EDGE_E, EDGE_N)
    assert tuple(boot.shape) == (EDGE_E, EDGE_N)
    with torch.no_grad():
        r_logits, r_value, _, r_boot = impala_ref.evaluate(kind, p64, t, first, T_)
    for a, b in ((logits, r_logits), (value, r_value), (boot, r_boot)):
        assert max_err(a, b) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("case", [EDGE_CASES[0], EDGE_CASES[10]], ids=edge_id)      # K % T == 0, and ragged
@pytest.mark.parametrize("kind", KINDS)
def test_without_obs_first_it_is_the_same_call(kind, case):
    """obs = cat([first, obs]) and obs_first=None: row k reads obs[k], the bootstrap obs[K] -- the same numbers go through the
    same operations, so the loss, the statistics, every gradient and evaluate_fragment's outputs are equal, not close."""
    K_, T_ = case[:2]
    assert (K_ % T_ == 0) == (case is EDGE_CASES[0])
    pol, t, first = edge_inputs(kind, case)
    t2 = dict(t, obs=torch.cat([first.unsqueeze(0), t["obs"]]))
    a, b = flat(run(kind, copy.deepcopy(pol), t, first, T_=T_)), flat(run(kind, copy.deepcopy(pol), t2, None, T_=T_))
    for name in a:
        assert torch.equal(a[name], b[name]), name
    for x, y in zip(evaluate_fragment(pol, t, first, T_), evaluate_fragment(pol, t2, None, T_)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("kind", KINDS)
def test_the_bound_notices_wrong_evaluation_rules(kind):
    """Each wrong rule of impala_ref.EVAL_VARIANTS, at each case where it applies: its distance from the right rule in
    evaluate_fragment's three outputs over the bound 4 et + 1e-6 max(1, max |ref|), et the float32 CPU evaluate_fragment's
    error; the largest of the three factors must be 10 or more.  And why the outputs are compared at all: the rule "the
    bootstrap row ignores done[K - 1]" leaves the loss and every gradient where they are, exactly -- where done[K - 1] is set
    V-trace's discount is 0 and the bootstrap is multiplied away."""
    names = ("logits", "value", "bootstrap")
    applied = {v: 0 for v in eval_variants_of(kind)}
    for case in EDGE_CASES:
        K_, T_ = case[:2]
        pol, t, first = edge_inputs(kind, case)
        p64 = copy.deepcopy(pol).double()
        with torch.no_grad():
            ref = impala_ref.evaluate(kind, p64, t, first, T_)
        ref = dict(zip(names, (ref[0], ref[1], ref[3])))
        got32 = dict(zip(names, evaluate_fragment(pol, t, first, T_)))
        bounds = {n: bound(ref[n], max_err(got32[n], ref[n])) for n in names}
        for n in names:
            assert max_err(got32[n], ref[n]) <= bounds[n]
        right = None
        for variant in eval_variants_of(kind):
            if not eval_variant_applies(kind, variant, t, first, T_):
                continue
            applied[variant] += 1
            with torch.no_grad():
                wrong = impala_ref.evaluate(kind, p64, t, first, T_, variant)
            wrong = dict(zip(names, (wrong[0], wrong[1], wrong[3])))
            factors = {n: max_err(wrong[n], ref[n]) / bounds[n] for n in names}
            print("%s %-22s %-18s factors %s" % (kind, edge_id(case), variant, {n: "%.3g" % f for n, f in factors.items()}))
            assert max(factors.values()) >= 10.0, (edge_id(case), variant, factors)
            if variant == "boot_ignores_done":
                right = right or flat(autograd_loss(kind, pol, t, HYPER, first, T_))
                blind = flat(autograd_loss(kind, pol, t, HYPER, first, T_, eval_variant=variant))
                for n in right:
                    assert max_err(blind[n], right[n]) == 0.0, (edge_id(case), n)
    assert all(applied.values()), applied
