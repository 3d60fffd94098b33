"""impala_loss, impala_loss_recurrent and impala_loss_moa without a GPU: the CPU paths -- evaluate_fragment
in plain torch, the importance weights, postprocessing.vtrace's NumPy path and a3c_terms on the detached targets -- against
the float64 autograd restatement of impala_ref.py, on fragments built as a3c_ref.make_inputs builds them with a behaviour
policy that differs from the target; the power of the suites' bound against four wrong losses; the argument checks."""
import copy

import pytest
import torch

import impala_ref
from a3c_ref import bound, max_err
from impala_ref import HYPER, INFLUENCE_WEIGHT, MOA_WEIGHT, VARIANTS, autograd_loss, make_batch
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
