"""impala_loss, impala_loss_recurrent and impala_loss_moa on the MI355X: the device path -- the forward entry
points under the state rule, three torch ops, ssd_vtrace, the A3C gradient kernels -- against the float64 restatement of
impala_ref.py with the float32 CPU path as the yardstick (ek <= 4 et + 1e-6 max(1, max |ref|) per tensor), bit-equal repeats,
evaluate_fragment against what a fresh sample() recorded (to the bit), the on-policy agreement with the A3C calls, and one
clipped SGD step end to end per policy after a second pass over the fragment.  A = 8, C = 64, E = 3, N = 2, K = 5, T = 2: two
full windows and a ragged one; and four cases of the edge matrix at E = 17, N = 5 (test_evaluate_fragment_gpu.py has the rest)."""
import copy

import numpy as np
import pytest
import torch

from a3c_ref import as_numpy_u32, make_policy, max_err
from impala_ref import EDGE_CASES, HYPER, INFLUENCE_WEIGHT, MOA_WEIGHT, autograd_loss, edge_batch, edge_id, make_batch
from sequential_social_dilemma_games_amd import (a3c_loss, a3c_loss_moa, a3c_loss_recurrent, clip_grad_by_set_norm, evaluate_fragment,
                                                 impala_loss, impala_loss_moa, impala_loss_recurrent)
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
KINDS = ("fc", "lstm", "moa")
A, C, E, N, STEPS, T = 8, 64, 3, 2, 5, 2


def _impala(kind, pol, t, first, h=HYPER, influence_weight=INFLUENCE_WEIGHT, T_=T):
    if kind == "fc":
        return impala_loss(pol, t, obs_first=first, **h)
    if kind == "lstm":
        return impala_loss_recurrent(pol, t, seq_len=T_, obs_first=first, **h)
    return impala_loss_moa(pol, t, seq_len=T_, moa_weight=MOA_WEIGHT, influence_weight=influence_weight, obs_first=first, **h)


def _a3c(kind, pol, t, first, h):
    if kind == "fc":
        return a3c_loss(pol, t, obs_first=first, **h)
    if kind == "lstm":
        return a3c_loss_recurrent(pol, t, seq_len=T, obs_first=first, **h)
    return a3c_loss_moa(pol, t, seq_len=T, moa_weight=MOA_WEIGHT, obs_first=first, **h)


def _flat(pol, loss, stats):
    """loss.backward() and one dict of everything the call gave: the loss, the statistics and the gradients."""
    pol.zero_grad()
    loss.backward()
    d = {"loss": loss.detach()}
    d.update({"stat " + k: v for k, v in stats.items()})
    for name, _, _ in pol.layout():
        g = getattr(pol, name).grad
        d["grad " + name] = torch.zeros_like(getattr(pol, name)).detach() if g is None else g.detach().clone()
    return d


def _under_the_bound(got, yard, ref, what):
    """ek <= 4 et + 1e-6 max(1, max |ref|) for every tensor; prints each figure before it asserts."""
    bad = []
    for name in ref:
        ek, et = max_err(got[name], ref[name]), max_err(yard[name], ref[name])
        scale = max(1.0, float(ref[name].abs().max()))
        print("%s %-22s ek %.3e et %.3e max|ref| %.3e" % (what, name, ek, et, scale))
        if not ek <= 4.0 * et + 1e-6 * scale:
            bad.append((name, ek, et))
    assert not bad, (what, bad)


def _to(t, dev):
    return {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in t.items()}


@pytest.mark.parametrize("P", [1, N])
@pytest.mark.parametrize("kind", KINDS)
def test_against_float64_and_repeats(kind, P):
    pol, t, first = make_batch(kind, A, N, P, STEPS, E, T, seed=3 + P)
    loss64, stats64, g64, rhos = autograd_loss(kind, pol, t, HYPER, first, T)
    ref = {"loss": loss64}
    ref.update({"stat " + k: v for k, v in stats64.items()})
    ref.update({"grad " + k: v for k, v in g64.items()})
    assert (rhos < 1).double().mean() >= 0.1 and (rhos > 1).double().mean() >= 0.1
    cpu = copy.deepcopy(pol)
    yard = _flat(cpu, *_impala(kind, cpu, t, first))              # the float32 CPU path
    dpol, dt, dfirst = copy.deepcopy(pol).to(DEV), _to(t, DEV), first.to(DEV)
    got = _flat(dpol, *_impala(kind, dpol, dt, dfirst))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(x).all()) for x in got.values())
    _under_the_bound(got, yard, ref, kind)
    again = _flat(dpol, *_impala(kind, dpol, dt, dfirst))
    torch.cuda.synchronize()
    for name in got:
        assert np.array_equal(as_numpy_u32(got[name]), as_numpy_u32(again[name])), name


# four cases of the edge matrix (impala_ref.EDGE_CASES; E = 17, N = 5, a second tile with one row): whole windows only with
# every other env ending on the last row, T = 1, one window with T > K, and whole windows with neither done nor obs_first
EDGE_LOSS_CASES = [(EDGE_CASES[0], True), (EDGE_CASES[7], True), (EDGE_CASES[11], True), (EDGE_CASES[2], False)]
assert [c[:3] for c, _ in EDGE_LOSS_CASES] == [(4, 2, "per_env"), (3, 1, "per_env"), (4, 8, "window_end"), (6, 3, "none")]


@pytest.mark.parametrize("case,use_first", EDGE_LOSS_CASES, ids=lambda x: edge_id(x) if isinstance(x, tuple) else ("first" if x else "nofirst"))
@pytest.mark.parametrize("kind", KINDS)
def test_edge_cases_against_float64_and_repeat(kind, case, use_first):
    """test_against_float64_and_repeats at four shapes of the edge matrix, the last one in the obs_first=None form."""
    T_ = case[1]
    pol, t, first = edge_batch(kind, case)
    loss64, stats64, g64, rhos = autograd_loss(kind, pol, t, HYPER, first, T_)
    ref = {"loss": loss64}
    ref.update({"stat " + k: v for k, v in stats64.items()})
    ref.update({"grad " + k: v for k, v in g64.items()})
    assert (rhos < 1).double().mean() >= 0.1 and (rhos > 1).double().mean() >= 0.1
    if not use_first:
        assert "done" not in t
        t, first = dict(t, obs=torch.cat([first.unsqueeze(0), t["obs"]]).contiguous()), None
    cpu = copy.deepcopy(pol)
    yard = _flat(cpu, *_impala(kind, cpu, t, first, T_=T_))        # the float32 CPU path
    dpol, dt, dfirst = copy.deepcopy(pol).to(DEV), _to(t, DEV), None if first is None else first.to(DEV)
    got = _flat(dpol, *_impala(kind, dpol, dt, dfirst, T_=T_))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(x).all()) for x in got.values())
    _under_the_bound(got, yard, ref, "%s %s" % (kind, edge_id(case)))
    again = _flat(dpol, *_impala(kind, dpol, dt, dfirst, T_=T_))
    torch.cuda.synchronize()
    for name in got:
        assert np.array_equal(as_numpy_u32(got[name]), as_numpy_u32(again[name])), name


def _sampled(kind, seed, horizon=3, **kw):
    """A policy and a fresh fragment of 4 envs x 5 agents (E N a multiple of 4) whose episodes end inside it."""
    E_, N_ = 4, 5
    env = SSDVectorEnv(K.GAME_HARVEST, E_, N_, horizon=horizon, seed=seed)
    pol = (make_policy(kind, env.engine.num_actions, N_, N_, C, seed=40 + seed) if kind == "fc" else
           make_policy(kind, env.engine.num_actions, N_, N_, C, seed=40 + seed, recur=2.0)).to(DEV)
    first = env.reset().clone()
    if kind != "fc":
        kw["state_every"] = T
    batch = env.sample(pol, STEPS, **kw)
    return env, pol, first, batch


@pytest.mark.parametrize("kind", KINDS)
def test_evaluate_fragment_gives_back_what_sample_recorded(kind):
    """Unchanged weights, state_every = T: the forward entry points run the rollout's kernels and the windows replay the
    rollout's own state rule, so value and last_value come back to the bit."""
    _, pol, first, batch = _sampled(kind, seed=7)
    assert bool(batch["done"][:STEPS - 1].any())
    logits, value, boot = evaluate_fragment(pol, batch, first, T)
    torch.cuda.synchronize()
    assert np.array_equal(as_numpy_u32(value), as_numpy_u32(batch["value"]))
    assert np.array_equal(as_numpy_u32(boot), as_numpy_u32(batch["last_value"]))
    assert tuple(logits.shape) == tuple(value.shape) + (pol.num_actions,) and bool(torch.isfinite(logits).all())


@pytest.mark.parametrize("kind", KINDS)
def test_on_policy_it_is_the_a3c_loss(kind):
    """Sampled with gamma and use_gae=False and unchanged weights, rho is 1 up to the rounding of two log-softmaxes and
    V-trace's targets are the discounted returns: impala_loss* and a3c_loss* agree in loss, statistics and every gradient
    under the yardstick, with et the distance of the same two calls on the CPU path in float32 on a copy of the batch."""
    w = 0.25
    kw = dict(influence_weight=w) if kind == "moa" else {}
    _, pol, first, batch = _sampled(kind, seed=9, gamma=0.99, use_gae=False, **kw)
    h = dict(vf_loss_coeff=0.5, entropy_coeff=0.01)
    hi = dict(HYPER, **h)
    ref = _flat(pol, *_a3c(kind, pol, batch, first, h))
    got = _flat(pol, *_impala(kind, pol, batch, first, hi, influence_weight=w))
    torch.cuda.synchronize()
    cpu, cb, cf = copy.deepcopy(pol).cpu(), _to(batch, "cpu"), first.cpu()
    ref_cpu = _flat(cpu, *_a3c(kind, cpu, cb, cf, h))
    got_cpu = _flat(cpu, *_impala(kind, cpu, cb, cf, hi, influence_weight=w))
    bad = []
    for name in ref:
        ek, et = max_err(got[name], ref[name]), max_err(got_cpu[name], ref_cpu[name])
        scale = max(1.0, float(ref[name].abs().max()))
        print("%s on-policy %-22s ek %.3e et %.3e max|ref| %.3e" % (kind, name, ek, et, scale))
        if not ek <= 4.0 * et + 1e-6 * scale:
            bad.append((name, ek, et))
    assert not bad, bad


@pytest.mark.parametrize("kind", KINDS)
def test_sample_two_passes_clip_step(kind):
    """sample() once, then two passes of loss -> backward -> clip_grad_by_set_norm -> SGD step over the same fragment: from
    the second pass on the weights have moved, rho != 1, and everything stays finite."""
    _, pol, first, batch = _sampled(kind, seed=11)
    opt = torch.optim.SGD(pol.parameters(), lr=1e-3)
    for _ in range(2):
        got = _flat(pol, *_impala(kind, pol, batch, first))
        norms = clip_grad_by_set_norm(pol, 40.0)
        opt.step()
    logits, value, boot = evaluate_fragment(pol, batch, first, T)
    logp = torch.log_softmax(logits, -1).gather(-1, batch["actions"].long().unsqueeze(-1)).squeeze(-1)
    rhos = torch.exp(logp - batch["logp"])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(x).all()) for x in list(got.values()) + [norms, value, boot, rhos])
    assert all(bool(torch.isfinite(p).all()) for p in pol.parameters())
    assert bool(((rhos - 1).abs() > 1e-4).any())
    assert not np.array_equal(as_numpy_u32(value), as_numpy_u32(batch["value"]))
