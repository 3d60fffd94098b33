"""test_ws_loss_kinks_gpu.py's conditions on its inputs without a GPU -- the clipped-rows cases and the Gaussian head away from
log_std = 0, on the float64 reference alone -- and whether the project's bound would notice a wrong formula of the Gaussian
head at those inputs: float64 restatements of the header's explicit derivatives with one slip each, against torch's autograd
in float64, with torch's float32 autograd on the CPU as the yardstick."""
import pytest
import torch

import ws_a3c_ref
from sequential_social_dilemma_games_amd import ppo_loss_watershed
from ws_ppo_ref import (HYPER, KINK_AGENTS, KINK_HYPER, KINK_SHAPE, WIDE_SEEDS, WIDE_SHAPE, WRONG_FORMULAS, assert_kink_conditions,
                        assert_wide_conditions, autograd_loss, bound, branch_report, gauss_formula_grads, kink_case, make_policy,
                        max_err, wide_case)


@pytest.mark.parametrize("variant,agent", KINK_AGENTS)
@pytest.mark.parametrize("live", [False, True])
def test_clipped_rows_on_the_reference(variant, agent, live):
    """clipped_rows' promises on the float64 reference: every row clipped on both signs of the advantage, dead or clipped and
    live, 0.1 and more from every boundary; the dead case's gradient is exactly zero and its policy_loss the stated number; the
    live case leaves the heads' layer exactly zero and reaches every other tensor; the CPU path of the call agrees."""
    T = KINK_SHAPE["T"]
    pol, t = kink_case(variant, agent, live)
    rep = branch_report(pol, agent, t, KINK_HYPER, T)
    assert_kink_conditions(rep, live)
    _, stats, g = autograd_loss(pol, agent, t, KINK_HYPER, T)
    assert abs(float(stats["policy_loss"]) - (-(1.3 * rep["clipped_pos"]) + 0.7 * rep["clipped_neg"])) < 1e-6
    for name in g:
        zero = not live or name in ("out_w", "out_b")
        assert (float(g[name].abs().max()) == 0.0) == zero, name
    pol.zero_grad()
    loss, _ = ppo_loss_watershed(pol, agent, t, seq_len=T, **KINK_HYPER)
    loss.backward()
    for name in g:
        got = getattr(pol, name).grad
        assert got is None and not float(g[name].abs().max()) or max_err(got, g[name]) <= 1e-5 * max(1.0, float(g[name].abs().max())), name


def test_default_makers_are_unchanged_by_the_new_keywords():
    """log_std_reach = 0.9 is the default's scaling, to the bit: the existing cases keep their policies."""
    a, b = make_policy(1, 64, seed=3), make_policy(1, 64, seed=3, log_std_reach=0.9)
    for name, _, _ in a.layout():
        assert torch.equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize("variant,agent", sorted(WIDE_SEEDS))
def test_wide_log_std_inputs_and_wrong_formulas(variant, agent):
    """The wide case's conditions, its references finite, and the bound at these inputs: the header's formulas restated agree
    with autograd (a thousandth of a bound), and each wrong formula -- d logp / d log_std = z^2, d kl / d log_std = -q, d kl /
    d mean over expf(log_std) -- is 100 bounds or more off in some tensor, for the PPO loss and (the first) for the A3C loss.
    Measured: PPO 6.9e3, 1.1e4, 8.0e4 (SeqComm 5) and 7.0e3, 2.8e4, 1.8e4 (Seq 0) bounds; A3C 1.2e4 and 7.3e4."""
    T = WIDE_SHAPE["T"]
    pol, t, rep = wide_case(variant, agent)
    assert_wide_conditions(rep)
    for a3c in (False, True):
        h, ref = (ws_a3c_ref.HYPER, ws_a3c_ref.autograd_loss) if a3c else (HYPER, autograd_loss)
        loss64, stats64, g64 = ref(pol, agent, t, h, T)
        _, _, g32 = ref(pol, agent, t, h, T, dtype=torch.float32)
        assert all(bool(torch.isfinite(x).all()) for x in list(g64.values()) + list(stats64.values()) + [loss64])
        bounds = {name: bound(g64[name], max_err(g32[name], g64[name])) for name in g64}
        right = gauss_formula_grads(pol, agent, t, h, T, a3c=a3c)
        assert max(max_err(right[name], g64[name]) / bounds[name] for name in g64) <= 1e-3
        for wrong in WRONG_FORMULAS[:1] if a3c else WRONG_FORMULAS:
            gw = gauss_formula_grads(pol, agent, t, h, T, wrong=wrong, a3c=a3c)
            ratios = {name: max_err(gw[name], g64[name]) / bounds[name] for name in g64}
            worst = max(ratios, key=ratios.get)
            print("%s %-14s off by %.3g bounds in %s" % ("a3c" if a3c else "ppo", wrong, ratios[worst], worst))
            assert ratios[worst] >= 100.0, (wrong, ratios)
