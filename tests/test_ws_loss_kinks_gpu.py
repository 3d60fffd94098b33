"""The Watershed loss kernels on the MI355X where the contract is most particular and the other files' inputs keep away
(csrc/ssd_ws_policy_grad.hip: ws_gauss_row, ws_gauss_ac_row, ppo_row under ssd_ws_policy_ppo_grad / ssd_ws_policy_ac_grad):
 - the derivatives at the kinks: fragments whose every row is clipped, on both signs of the advantage, with the value branch
   dead (every gradient exactly zero) or clipped and live (the heads' layer exactly zero, the rest against float64);
 - rows that are exactly on policy, from sample(): the forward of the loss kernel is the rollout's bit for bit, so clip ranges
   of (0, 0) and (1e6, 1e6) give the same bits, policy_loss is -1 and kl is 0 exactly, and the KL term moves no gradient;
 - the Gaussian head away from log_std = 0 and |z| <= 2.5, for the PPO and the A3C call.
Every test asserts the conditions on its inputs on the float64 reference before it touches the device (the same conditions
test_ws_loss_kinks_cpu.py asserts without one) and prints ek, et and the branch report it relies on."""
import copy
import functools

import pytest
import torch

import test_ws_a3c_gpu as a3c_gpu
import test_ws_ppo_gpu as ppo_gpu
import ws_a3c_ref
from sequential_social_dilemma_games_amd import WatershedVecEngine
from sequential_social_dilemma_games_amd.policy import PPO_STATS, ws_is_comm
from ws_ppo_ref import (HYPER, KINK_AGENTS, KINK_HYPER, KINK_SHAPE, SEQ, SEQ_COMM, WIDE_SEEDS, WIDE_SHAPE, as_numpy_u32,
                        assert_kink_conditions, assert_wide_conditions, autograd_loss, branch_report, gather_own_steps, kink_case,
                        make_policy, wide_case)

pytestmark = pytest.mark.gpu

DEV = ppo_gpu.DEV
_run, _to_dev, _equal_bits, _check_against_reference = ppo_gpu._run, ppo_gpu._to_dev, ppo_gpu._equal_bits, ppo_gpu._check_against_reference


# ---- 1. clipped rows ----

@pytest.mark.parametrize("variant,agent", KINK_AGENTS)
def test_clipped_and_dead_rows_give_exactly_zero(variant, agent):
    """Every row clipped with the clipped operand the minimum -- adv = +1 at ratio 1.5 and adv = -1 at ratio 0.5 -- and dead
    (vf2 > vf1 beyond the value clip): with entropy_coeff = kl_coeff = 0 nothing flows, every gradient is exactly zero, and
    policy_loss is -(1.3 * the share of adv > 0) + 0.7 * the share of adv < 0."""
    T = KINK_SHAPE["T"]
    pol, t = kink_case(variant, agent, live=False)
    rep = branch_report(pol, agent, t, KINK_HYPER, T)
    print("dead", (variant, agent), rep)
    assert_kink_conditions(rep, live=False)
    loss, stats, g = _run(copy.deepcopy(pol).to(DEV), agent, _to_dev(t), KINK_HYPER, T)
    torch.cuda.synchronize()
    want = -(1.3 * rep["clipped_pos"]) + 0.7 * rep["clipped_neg"]
    print("policy_loss %.9f want %.9f" % (float(stats["policy_loss"]), want), {k: float(stats[k]) for k in PPO_STATS})
    for name in g:
        assert float(g[name].abs().max()) == 0.0, name
    assert abs(float(stats["policy_loss"]) - want) < 1e-4
    assert all(bool(torch.isfinite(stats[k])) for k in PPO_STATS) and bool(torch.isfinite(loss))


@pytest.mark.parametrize("variant,agent", KINK_AGENTS)
def test_clipped_and_live_rows_pull_through_the_value_alone(variant, agent):
    """The same rows with the value branch clipped and live (vf1 > vf2): d vf / d value = 2 (value - vt) on every row, nothing
    through the ratio.  out_w and out_b are exactly zero in the kernel and in the float64 reference; every other tensor is
    non-zero and within the project's bound of float64."""
    T = KINK_SHAPE["T"]
    pol, t = kink_case(variant, agent, live=True)
    rep = branch_report(pol, agent, t, KINK_HYPER, T)
    print("live", (variant, agent), rep)
    assert_kink_conditions(rep, live=True)
    loss64, stats64, g64 = autograd_loss(pol, agent, t, KINK_HYPER, T)
    loss32, stats32, g32 = autograd_loss(pol, agent, t, KINK_HYPER, T, dtype=torch.float32, device=DEV)
    loss, stats, g = _run(copy.deepcopy(pol).to(DEV), agent, _to_dev(t), KINK_HYPER, T)
    torch.cuda.synchronize()
    for name in ("out_w", "out_b"):
        assert float(g[name].abs().max()) == 0.0 and float(g64[name].abs().max()) == 0.0, name
    for name in g:
        if name not in ("out_w", "out_b"):
            assert float(g[name].abs().max()) > 0.0 and float(g64[name].abs().max()) > 0.0, name
    assert all(bool(torch.isfinite(x).all()) for x in list(g.values()) + list(stats.values()) + [loss])
    _check_against_reference(g, g32, g64, "live grad")
    _check_against_reference(stats, stats32, stats64, "live stat")
    _check_against_reference({"loss": loss}, {"loss": loss32}, {"loss": loss64}, "live loss")
    ppo_gpu._exact_zeros(pol, agent, g)


# ---- 3. rows exactly on policy ----

ON_POLICY_T = 2
ON_POLICY_HYPER = dict(vf_loss_coeff=1e-2, entropy_coeff=1e-3, kl_coeff=0.2)      # test_sample_loss_step's
ON_POLICY_AGENTS = [(SEQ_COMM, 5), (SEQ_COMM, 1), (SEQ, 1)]
TIGHT, LOOSE = dict(clip_param=0.0, vf_clip_param=0.0), dict(clip_param=1e6, vf_clip_param=1e6)


@functools.lru_cache(maxsize=None)
def _sampled(variant):
    """test_sample_loss_step's batch: sample() over two rounds and most of a third at E = 64, kept for all tests of the variant
    -> (policy on the device, batch, the first observations)."""
    eng = WatershedVecEngine(variant, 64, seed=5)
    pol = make_policy(variant, 64, seed=31).to(DEV)
    first, _ = eng.reset()
    first = first.clone()
    batch = eng.sample(pol, 34 if variant == SEQ_COMM else 11)
    torch.cuda.synchronize()
    return pol, batch, first


@functools.lru_cache(maxsize=None)
def _on_policy(variant, agent):
    """The agent's own rows of _sampled(variant) as the example gathers them, with logp_old = the batch's logp, vf_pred = its
    value, the behaviour dist its dist, and random advantages and value targets as in test_sample_loss_step."""
    pol, batch, first = _sampled(variant)
    seq, ks = gather_own_steps(batch, first, agent, ON_POLICY_T)
    M = len(ks)
    assert M > ON_POLICY_T, ks
    g = torch.Generator().manual_seed(7 + agent)
    seq["advantages"] = torch.randn((M, 64), generator=g).to(DEV)
    seq["value_targets"] = (seq["value"] + torch.randn((M, 64), generator=g).to(DEV)).contiguous()
    return pol, seq


def _call(pol, agent, seq, **h):
    out = _run(pol, agent, seq, dict(ON_POLICY_HYPER, **h), ON_POLICY_T)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("variant,agent", ON_POLICY_AGENTS)
def test_on_policy_rows_do_not_see_the_clip_range(variant, agent):
    """With the weights that sampled, logp_old = the rollout's logp and vf_pred = its value, the kernel's ratio is 1 and its
    value - vf_pred is 0 exactly, because its forward is the rollout's bit for bit.  So clip ranges of (0, 0), where lo = hi = 1
    and the value clip is 0, and of (1e6, 1e6) give the same uint32 words in the loss, every statistic and every gradient; a
    forward one ulp off in one row would clip that row under (0, 0)."""
    pol, seq = _on_policy(variant, agent)
    tight, loose = _call(pol, agent, seq, **TIGHT), _call(pol, agent, seq, **LOOSE)
    print("on-policy", (variant, agent), {k: float(tight[1][k]) for k in PPO_STATS}, {k: float(loose[1][k]) for k in PPO_STATS})
    for name in loose[2]:
        words = (as_numpy_u32(tight[2][name]) != as_numpy_u32(loose[2][name])).sum()
        print("%-14s max |g| %.3e differing words %d" % (name, float(loose[2][name].abs().max()), words))
    _equal_bits(tight, loose)
    for name in loose[2]:
        if float(loose[2][name].abs().max()) > 0.0:
            assert float(tight[2][name].abs().max()) > 0.0, name
    assert float(loose[2]["out_w"].abs().max()) > 0.0 and float(loose[2]["value_w"].abs().max()) > 0.0


@pytest.mark.parametrize("variant,agent", ON_POLICY_AGENTS)
def test_on_policy_statistics_are_exact(variant, agent):
    """advantages = 1 under the clip range (0, 0): every row's -surr is -1 and its kl is 0 -- the Gaussian's q is 1 exactly, the
    Categorical's blp - lp is 0 term by term --, so the float64 means are -1.0 and 0.0 to the bit."""
    pol, seq = _on_policy(variant, agent)
    _, stats, _ = _call(pol, agent, dict(seq, advantages=torch.ones_like(seq["value"])), **TIGHT)
    print("on-policy stats", (variant, agent), {k: repr(float(stats[k])) for k in PPO_STATS})
    assert float(stats["policy_loss"]) == -1.0
    assert float(stats["kl"]) == 0.0


@pytest.mark.parametrize("variant,agent", ON_POLICY_AGENTS)
def test_on_policy_kl_term_moves_no_gradient(variant, agent):
    """d kl / d dist is zero on every row when the behaviour dist is the current one: the gradients with kl_coeff = 0.2 and the
    batch's dist equal those with kl_coeff = 0 and no dist (torch.equal: x + 0.2 * 0 may turn a -0.0 into +0.0)."""
    pol, seq = _on_policy(variant, agent)
    with_kl = _call(pol, agent, seq, **TIGHT)
    bare = {k: v for k, v in seq.items() if k != "dist"}
    without = _call(pol, agent, bare, kl_coeff=0.0, **TIGHT)
    for name in with_kl[2]:
        d = float((with_kl[2][name] - without[2][name]).abs().max())
        print("kl term %-14s max |g| %.3e max difference %.3e" % (name, float(without[2][name].abs().max()), d))
    for name in with_kl[2]:
        assert torch.equal(with_kl[2][name], without[2][name]), name


@pytest.mark.parametrize("variant,agent", ON_POLICY_AGENTS)
def test_on_policy_gradient_against_float64(variant, agent):
    """The (0, 0) gradient, where both branches of both clips tie on every row, is the gradient of the unclipped loss (the
    header's rule for the first epoch): against the float64 reference of the loss under (1e6, 1e6), by the project's bound."""
    pol, seq = _on_policy(variant, agent)
    h = dict(ON_POLICY_HYPER, **LOOSE)
    t = {"obs": seq["obs"], "state": seq["state"], "starts": seq["starts"], "actions": seq["actions"], "logp_old": seq["logp"],
         "advantages": seq["advantages"], "value_targets": seq["value_targets"], "vf_pred": seq["value"], "behaviour_dist": seq["dist"]}
    cpu_t = {k: v.cpu() for k, v in t.items()}
    loss64, stats64, g64 = autograd_loss(copy.deepcopy(pol).cpu(), agent, cpu_t, h, ON_POLICY_T)
    loss32, stats32, g32 = autograd_loss(pol, agent, cpu_t, h, ON_POLICY_T, dtype=torch.float32, device=DEV)
    loss, stats, g = _call(pol, agent, seq, **TIGHT)
    _check_against_reference(g, g32, g64, "on-policy grad %d" % agent)
    _check_against_reference(stats, stats32, stats64, "on-policy stat %d" % agent)
    _check_against_reference({"loss": loss}, {"loss": loss32}, {"loss": loss64}, "on-policy loss %d" % agent)


# ---- 4. the Gaussian head away from log_std = 0 ----

@pytest.mark.parametrize("variant,agent", sorted(WIDE_SEEDS))
def test_wide_log_std_ppo_against_float64(variant, agent):
    """log_std from below -3.5 to above +1.5 and |z| beyond 4: expf(2 log_std), 1 / expf(2 log_std), z * z - 1 and z / sd of
    ws_gauss_row where they lose accuracy first; gradients, statistics and loss under the project's bound, the exact zeros, and
    a repeat with the same bits (compare_with_float64 of test_ws_ppo_gpu.py)."""
    pol, t, rep = wide_case(variant, agent)
    print("wide ppo", (variant, agent), rep)
    assert_wide_conditions(rep)
    _, stats64, g64 = autograd_loss(pol, agent, t, HYPER, WIDE_SHAPE["T"])
    assert all(bool(torch.isfinite(x).all()) for x in list(g64.values()) + list(stats64.values()))
    ppo_gpu.compare_with_float64(pol, agent, t, HYPER, WIDE_SHAPE["T"])


@pytest.mark.parametrize("variant,agent", sorted(WIDE_SEEDS))
def test_wide_log_std_a3c_against_float64(variant, agent):
    """The same sequences through a3c_loss_watershed (ws_gauss_ac_row): the bound, the exact zeros, a repeat with the same bits."""
    pol, t, rep = wide_case(variant, agent)
    print("wide a3c", (variant, agent), rep)
    assert_wide_conditions(rep)
    assert not ws_is_comm(variant, agent)
    _, stats64, g64 = ws_a3c_ref.autograd_loss(pol, agent, t, ws_a3c_ref.HYPER, WIDE_SHAPE["T"])
    assert all(bool(torch.isfinite(x).all()) for x in list(g64.values()) + list(stats64.values()))
    a3c_gpu.compare_with_float64(pol, agent, t, ws_a3c_ref.HYPER, WIDE_SHAPE["T"])
