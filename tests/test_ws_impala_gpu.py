"""impala_loss_watershed on the MI355X: the loss, its statistics and gradients against the float64 restatement
(ws_a3c_ref.impala_autograd_loss: the sequences evaluated step by step, V-trace restated in the contract's order, the targets
detached) with the float32 CPU path of the same call as the yardstick; the same bits as a3c_loss_watershed fed
with the device vtrace's outputs; and two passes over one batch with an SGD step between them."""
import copy

import numpy as np
import pytest
import torch

from sequential_social_dilemma_games_amd import a3c_loss_watershed, evaluate_sequences, impala_loss_watershed, vtrace
from sequential_social_dilemma_games_amd.policy import A3C_STATS
from ws_a3c_ref import IMPALA_HYPER, SEQ, SEQ_COMM, as_numpy_u32, impala_autograd_loss, make_impala_inputs, make_policy, max_err

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


def _cpu_path(pol, agent, t, T, h):
    """The yardstick, as tests/test_impala_loss_gpu.py has it: the float32 CPU path of the same call (plain torch for the
    evaluation and the A3C terms, the NumPy V-trace of the contract) -> (loss, stats, grads)."""
    pol = copy.deepcopy(pol).cpu()
    pol.zero_grad()
    loss, stats = impala_loss_watershed(pol, agent, t, seq_len=T, **h)
    loss.backward()
    return loss.detach(), stats, _grads(pol)


def _check(got, tor, ref, what):
    bad = []
    for name in ref:
        ek, et = max_err(got[name], ref[name]), max_err(tor[name], ref[name])
        scale = max(1.0, float(ref[name].abs().max()))
        print("%s %-14s ek %.3e et %.3e ek/et %.2f max|ref| %.3e" % (what, name, ek, et, ek / et if et else float("inf"), scale))
        if not ek <= FACTOR * et + 1e-6 * scale:
            bad.append((name, ek, et))
    assert not bad, (what, bad)


@pytest.mark.parametrize("variant,agent,Cs", [(SEQ_COMM, 1, 64), (SEQ_COMM, 5, 64), (SEQ, 1, 128)])
def test_against_the_float64_restatement_and_the_a3c_call(variant, agent, Cs):
    M, T, Q = 7, 3, 17
    pol = make_policy(variant, Cs, seed=20 + agent)
    t = make_impala_inputs(pol, agent, M, Q, T, seed=120 + agent)
    loss64, stats64, g64, rhos64 = impala_autograd_loss(pol, agent, t, IMPALA_HYPER, T)
    assert float(rhos64.min()) < 0.9 and float(rhos64.max()) > 1.1      # the weights spread on both sides of the clip
    loss32, stats32, g32 = _cpu_path(pol, agent, t, T, IMPALA_HYPER)
    dpol, dt = pol.to(DEV), _to_dev(t)
    dpol.zero_grad()
    loss, stats = impala_loss_watershed(dpol, agent, dt, seq_len=T, **IMPALA_HYPER)
    loss.backward()
    g = _grads(dpol)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(x).all()) for x in list(g.values()) + list(stats.values()) + [loss])
    _check(g, g32, g64, "grad")
    _check(stats, stats32, stats64, "stat")
    _check({"loss": loss.detach()}, {"loss": loss32}, {"loss": loss64}, "loss")
    # the same bits as the A3C call fed with the device vtrace's outputs
    with torch.no_grad():
        _, value, logp, boot = evaluate_sequences(dpol, agent, dict(dt, start_next=dt["done"][-1].contiguous()), T)
        rhos = torch.exp(logp - dt["logp"])
        vs, pg = vtrace(torch.zeros((M, Q), dtype=torch.int32, device=DEV), value, rhos, boot, dt["done"], gamma=0.99, bonus=dt["rew"],
                        bonus_weight=1.0)
    assert max_err(rhos, rhos64) <= 1e-5 * float(rhos64.max())
    dpol.zero_grad()
    want, wstats = a3c_loss_watershed(dpol, agent, dict(dt, advantages=pg, value_targets=vs), seq_len=T, vf_loss_coeff=0.5,
                                      entropy_coeff=0.01)
    want.backward()
    gw = _grads(dpol)
    torch.cuda.synchronize()
    assert np.array_equal(as_numpy_u32(loss.detach()), as_numpy_u32(want.detach()))
    for k in A3C_STATS:
        assert np.array_equal(as_numpy_u32(stats[k]), as_numpy_u32(wstats[k])), k
    for name in g:
        assert np.array_equal(as_numpy_u32(g[name]), as_numpy_u32(gw[name])), name


@pytest.mark.parametrize("agent", [1, 5])
def test_two_passes_with_a_step_between(agent):
    """The first pass under the weights that recorded logp (rhos == 1 exactly), an SGD step, the second pass: everything finite,
    and the importance weights have moved off 1."""
    M, T, Q = 6, 3, 17
    pol = make_policy(SEQ_COMM, 64, seed=30 + agent).to(DEV)
    t = _to_dev(make_impala_inputs(pol.cpu(), agent, M, Q, T, seed=130 + agent))
    pol = pol.to(DEV)
    full = dict(t, start_next=t["done"][-1].contiguous())
    t["logp"] = evaluate_sequences(pol, agent, full, T)[2].clone()       # what a rollout under these weights records
    opt = torch.optim.SGD(pol.parameters(), lr=1e-3)
    seen = []
    for _ in range(2):
        rhos = torch.exp(evaluate_sequences(pol, agent, full, T)[2] - t["logp"])
        seen.append(rhos)
        loss, stats = impala_loss_watershed(pol, agent, t, seq_len=T, **IMPALA_HYPER)
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v)) for v in stats.values())
        assert all(bool(torch.isfinite(p).all()) and bool(torch.isfinite(p.grad).all()) for p in pol.parameters())
    torch.cuda.synchronize()
    assert torch.equal(seen[0], torch.ones_like(seen[0]))
    assert float((seen[1] - 1).abs().max()) > 0.0 and bool(torch.isfinite(seen[1]).all())
