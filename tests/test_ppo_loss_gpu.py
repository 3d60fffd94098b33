"""ppo_loss on the MI355X (csrc/ssd_policy_grad.hip, ssd_policy_ppo_grad): the kernel's gradients and statistics against the
float64 restatement (ppo_ref.py) with torch's own float32 autograd on the same device as the yardstick, bit-equal repeats, a
caller's stream, rows exactly on policy (the clip range does not show, policy_loss = -1 and kl = 0 exactly), and one optimiser
step end to end from sample()."""
import copy

import numpy as np
import pytest
import torch

from ppo_ref import HYPER, LOOSE, MARGIN, as_numpy_u32, autograd_loss, branch_report, make_inputs, make_policy, max_err, on_policy_checks
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd import evaluate_fragment, ppo_loss
from sequential_social_dilemma_games_amd.policy import PPO_STATS
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# The factor of `ek <= FACTOR * et + 1e-6 * max(1, max |ref|)` per parameter tensor (DESIGN.md section 16 records the measured
# ek / et): the project's margin for the forward, 4, for every tensor.
FACTOR = {}

# (A, P, K, E, N, behaviour_logits, obs_first, own stream, seed): rows per set 1, 15, 16, 17 and a few thousand (one tile per
# workgroup), for P = N and P = 1
CASES = [(8, 5, 1, 1, 5, True, True, False, 1), (8, 5, 3, 5, 5, False, True, False, 2), (9, 5, 4, 4, 5, True, False, False, 3),
         (8, 5, 17, 1, 5, True, True, True, 4), (8, 5, 64, 48, 5, True, True, False, 5), (9, 5, 40, 50, 5, False, False, False, 6),
         (9, 1, 1, 1, 1, True, True, False, 7), (8, 1, 1, 3, 5, True, False, False, 8), (9, 1, 4, 2, 2, False, True, False, 9),
         (8, 1, 17, 1, 1, True, True, False, 10), (8, 1, 16, 40, 5, True, True, True, 11), (9, 1, 20, 60, 3, False, False, False, 14),
         # more tiles than workgroups, so that the persistent loop runs more than once, with a ragged last tile: 4104 rows per set =
         # 257 tiles over 204 workgroups (53 take two tiles, 151 one); 16 828 rows = 1052 tiles over 1024; 1500 rows per set = 94
         # tiles over 32 workgroups (two or three tiles each)
         (8, 5, 8, 513, 5, True, True, False, 15), (9, 1, 7, 601, 4, False, True, False, 16), (8, 32, 3, 500, 32, True, False, True, 17),
         # just past the point where the loop starts a second iteration, 1025 tiles or so in all: N = P = 64, the largest allowed
         # and so the smallest G (16), with 257 rows per set = 17 tiles, workgroup 0's second tile holding one live row (K = 257:
         # a row per step; E = 257: every row in step 0); 16 425 rows = 1027 tiles over 1024, the last tile with 9 rows
         (8, 64, 257, 1, 64, True, True, False, 18), (9, 64, 1, 257, 64, False, False, False, 19), (9, 1, 3, 1825, 3, True, True, False, 20)]


def _to_dev(t):
    return {k: v.to(DEV) for k, v in t.items()}


def _run(pol, t, first, h):
    """ppo_loss + backward on the device -> (loss, stats, {param: grad})."""
    pol.zero_grad()
    loss, stats = ppo_loss(pol, t, obs_first=first, **h)
    loss.backward()
    return loss.detach(), stats, {name: getattr(pol, name).grad.detach().clone() for name, _, _ in pol.layout()}


def _check_against_reference(got, tor, ref, what):
    """ek <= factor * et + 1e-6 * max(1, max |ref|) for every tensor of the dicts; prints each figure before it asserts."""
    bad = []
    for name in ref:
        ek, et = max_err(got[name], ref[name]), max_err(tor[name], ref[name])
        scale = max(1.0, float(ref[name].abs().max()))
        print("%s %-10s ek %.3e et %.3e ek/et %.2f max|ref| %.3e" % (what, name, ek, et, ek / et if et else float("inf"), scale))
        if not ek <= FACTOR.get(name, 4.0) * et + 1e-6 * scale:
            bad.append((name, ek, et))
    assert not bad, (what, bad)


def compare_with_float64(pol, t, first, h, own_stream=False, only=None):
    """The kernel on (pol, t, first, h) against the float64 restatement with torch's float32 autograd on the device as the
    yardstick -- gradients (the tensors named in `only`, or all), statistics and loss under the bound --, all outputs finite,
    and a second call `uint32`-equal to the first.  Returns (loss, stats, grads, float64 grads) of the kernel's first call."""
    P = pol.num_sets
    loss64, stats64, g64 = autograd_loss(pol, t, h, first)
    loss32, stats32, g32 = autograd_loss(pol, t, h, first, dtype=torch.float32, device=DEV)      # torch's own float32, same device
    dpol, dt, dfirst = copy.deepcopy(pol).to(DEV), _to_dev(t), None if first is None else first.to(DEV)
    if own_stream:
        s = torch.cuda.Stream(DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            loss, stats, g = _run(dpol, dt, dfirst, h)
        s.synchronize()
    else:
        loss, stats, g = _run(dpol, dt, dfirst, h)
    torch.cuda.synchronize()
    assert all(tuple(stats[k].shape) == (P,) and stats[k].dtype == torch.float64 for k in PPO_STATS)
    assert all(bool(torch.isfinite(x).all()) for x in list(g.values()) + list(stats.values()) + [loss])
    keep = (lambda d: d) if only is None else (lambda d: {k: d[k] for k in only})   # noqa: E731
    _check_against_reference(keep(g), keep(g32), keep(g64), "grad")
    _check_against_reference(stats, stats32, stats64, "stat")
    _check_against_reference({"loss": loss}, {"loss": loss32}, {"loss": loss64}, "loss")
    # the same inputs give the same bits, on the default stream too
    loss2, stats2, g2 = _run(dpol, dt, dfirst, h)
    torch.cuda.synchronize()
    assert np.array_equal(as_numpy_u32(loss), as_numpy_u32(loss2))
    for k in PPO_STATS:
        assert np.array_equal(as_numpy_u32(stats[k]), as_numpy_u32(stats2[k])), k
    for name in g:
        assert np.array_equal(as_numpy_u32(g[name]), as_numpy_u32(g2[name])), name
    return loss, stats, g, g64


@pytest.mark.parametrize("A,P,K_,E,N,beh,use_first,own_stream,seed", CASES)
def test_gradients_and_stats_against_float64(A, P, K_, E, N, beh, use_first, own_stream, seed):
    h = dict(HYPER, kl_coeff=HYPER["kl_coeff"] if beh else 0.0)
    pol = make_policy(A, P, seed=seed)
    t, first = make_inputs(pol, K_, E, N, seed=100 + seed, obs_first=use_first, behaviour=beh)
    rep = branch_report(pol, t, h, first)
    print("case", (A, P, K_, E, N, beh, use_first, own_stream), rep)
    assert rep["margin"] > MARGIN, rep                     # conditions on the inputs: no float32 branch can flip ...
    if K_ * E * N >= 1000:                                 # ... and every branch holds a real share of the rows
        for k in ("clipped_pos", "clipped_neg", "open_pos", "open_neg", "vf_dead", "vf_live", "vf_clipped_live"):
            assert rep[k] > 0.1, rep
    compare_with_float64(pol, t, first, h, own_stream)


def test_packed_gradient_padding_and_scaling():
    """The library's packed gradient has zero padding floats and holds what backward scatters; backward multiplies by the
    incoming gradient; a minibatch addressed by slices equals the explicit copy."""
    import ctypes as C
    from sequential_social_dilemma_games_amd import _capi
    A, N = 9, 5
    pol = make_policy(A, N, seed=21)
    t, first = make_inputs(pol, 5, 7, N, seed=22)
    pol, t, first = pol.to(DEV), _to_dev(t), first.to(DEV)
    _, _, g = _run(pol, t, first, HYPER)
    S = pol.set_floats
    packed = torch.full((N, S), float("nan"), dtype=torch.float32, device=DEV)
    stats = torch.zeros((N, 5), dtype=torch.float64, device=DEV)
    scratch = torch.empty(pol.ppo_scratch_shape(5 * 7), dtype=torch.float32, device=DEV)
    ptr = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
    hv = [HYPER[k] for k in ("clip_param", "vf_clip_param", "vf_loss_coeff", "entropy_coeff", "kl_coeff")]
    _capi.policy_check(_capi.lib().ssd_policy_ppo_grad(
        ptr(pol.packed()), N, A, ptr(first), ptr(t["obs"]), ptr(t["actions"]), ptr(t["logp_old"]), ptr(t["advantages"]),
        ptr(t["value_targets"]), ptr(t["vf_pred"]), ptr(t["behaviour_logits"]), 5, 7, N, *hv, ptr(scratch), ptr(packed), ptr(stats), 0, 0,
        C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
    torch.cuda.synchronize()
    used = torch.zeros(S, dtype=torch.bool, device=DEV)
    for name, shape, off in pol.layout():
        n = int(np.prod(shape))
        used[off:off + n] = True
        assert torch.equal(packed[:, off:off + n].reshape(g[name].shape), g[name]), name
    assert int((~used).sum()) > 0 and float(packed[:, ~used].abs().max()) == 0.0
    pol.zero_grad()
    loss, _ = ppo_loss(pol, t, obs_first=first, **HYPER)
    (loss * 3.0).backward()
    for name in g:
        assert torch.equal(getattr(pol, name).grad, g[name] * 3.0), name
    # minibatch slices by address: steps 1..3 with obs_first = obs[0] equal the explicit copy without obs_first
    mb = {k: v[1:4] for k, v in t.items()}
    a, sa, ga = _run(pol, mb, t["obs"][0], HYPER)
    b, sb, gb = _run(pol, dict(mb, obs=t["obs"][0:3].clone()), None, HYPER)
    assert torch.equal(a, b)
    for name in ga:
        assert torch.equal(ga[name], gb[name]), name


def test_on_policy_rows_exactly():
    """test_sample_loss_step_sample's fragment before any step: the weights that sampled, logp_old = the rollout's logp, vf_pred
    = its value, and the behaviour logits from the library's forward of the same rows (sample() records no logits; that call
    gives the rollout's to the bit).  The loss call's forward is exact float32 as that forward, so the kernel's ratio is 1 and
    its value - vf_pred is 0 exactly: ppo_ref.on_policy_checks -- the clip ranges (0, 0) and (1e6, 1e6) give the same bits,
    policy_loss = -1 and kl = 0 exactly under advantages = 1, the KL term moves no gradient -- and the (0, 0) gradient against
    the float64 reference of the unclipped loss."""
    E, N, steps = 64, 5, 8
    h = dict(vf_loss_coeff=1e-2, entropy_coeff=1e-3, kl_coeff=0.2)
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=1000, seed=5)
    pol = make_policy(env.engine.num_actions, N, seed=31).to(DEV)
    first = env.reset().clone()
    batch = env.sample(pol, steps, gamma=0.99, lambda_=0.95)
    logits, value, _ = evaluate_fragment(pol, batch, obs_first=first)
    assert torch.equal(value, batch["value"])                  # the library's forward gives back the rollout's values ...
    lp = torch.log_softmax(logits, -1).gather(-1, batch["actions"].long().unsqueeze(-1)).squeeze(-1)
    assert float((torch.exp(lp - batch["logp"]) - 1).abs().max()) < 1e-4      # ... and its logits the rollout's logp

    def call(clip_param, vf_clip_param, kl=True, ones=False):
        b = dict(batch, advantages=torch.ones_like(batch["value"])) if ones else dict(batch)
        if kl:
            b["logits"] = logits.contiguous()
        out = _run(pol, b, first, dict(h, clip_param=clip_param, vf_clip_param=vf_clip_param, kl_coeff=h["kl_coeff"] if kl else 0.0))
        torch.cuda.synchronize()
        return out
    loss, stats, g = on_policy_checks(call, PPO_STATS, "conv-FC")
    t = {"obs": batch["obs"], "actions": batch["actions"], "logp_old": batch["logp"], "advantages": batch["advantages"],
         "value_targets": batch["value_targets"], "vf_pred": batch["value"], "behaviour_logits": logits.contiguous()}
    cpu_t = {k: v.cpu() for k, v in t.items()}
    hl = dict(h, **LOOSE)
    loss64, stats64, g64 = autograd_loss(copy.deepcopy(pol).cpu(), cpu_t, hl, first.cpu())
    loss32, stats32, g32 = autograd_loss(pol, cpu_t, hl, first.cpu(), dtype=torch.float32, device=DEV)
    _check_against_reference(g, g32, g64, "on-policy grad")
    _check_against_reference(stats, stats32, stats64, "on-policy stat")
    _check_against_reference({"loss": loss}, {"loss": loss32}, {"loss": loss64}, "on-policy loss")


def test_sample_loss_step_sample():
    """sample(..., gamma=) -> ppo_loss on the batch -> backward -> one Adam step, against the same step from the torch loss;
    then the next sample() runs on the updated weights."""
    E, N, steps, lr = 64, 5, 8, 1e-2
    h = dict(clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1e-2, entropy_coeff=1e-3, kl_coeff=0.2)
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=1000, seed=5)
    pol = make_policy(env.engine.num_actions, N, seed=31).to(DEV)
    twin = copy.deepcopy(pol)
    first = env.reset().clone()
    batch = env.sample(pol, steps, gamma=0.99, lambda_=0.95)
    obs = torch.cat([first.unsqueeze(0), batch["obs"][:-1]])
    with torch.no_grad():
        logits, _ = pol(obs)                               # the behaviour logits: sample() records logp, not the logits
        logp = torch.log_softmax(logits, -1).gather(-1, batch["actions"].long().unsqueeze(-1)).squeeze(-1)
    t = {"obs": batch["obs"], "actions": batch["actions"], "logp_old": batch["logp"], "advantages": batch["advantages"],
         "value_targets": batch["value_targets"], "vf_pred": batch["value"], "behaviour_logits": logits.contiguous()}
    # before the step the policy is the one that sampled: ratio = 1 and kl = 0 up to rounding
    assert float((torch.exp(logp - batch["logp"]) - 1).abs().max()) < 1e-4
    # eps = 1: |d step / d grad| <= lr, so the two steps differ by at most lr times the gradients' difference (Adam's default eps
    # turns the first step into lr * sign(grad), which no gradient bound carries over to)
    opt = torch.optim.Adam(pol.parameters(), lr=lr, eps=1.0)
    opt_twin = torch.optim.Adam(twin.parameters(), lr=lr, eps=1.0)
    loss, stats = ppo_loss(pol, dict(batch, logits=t["behaviour_logits"]), obs_first=first, **h)
    assert float(stats["kl"].abs().max()) < 1e-6, stats["kl"]
    opt.zero_grad()
    loss.backward()
    cpu_t = {k: v.cpu() for k, v in t.items()}
    loss64, stats64, g64 = autograd_loss(twin.cpu(), cpu_t, h, first.cpu())
    twin = twin.to(DEV)
    _, _, g32 = autograd_loss(twin, cpu_t, h, first.cpu(), dtype=torch.float32, device=DEV)
    gk = {name: getattr(pol, name).grad for name, _, _ in pol.layout()}
    _check_against_reference(gk, g32, g64, "e2e grad")
    for name, _, _ in twin.layout():
        getattr(twin, name).grad = g32[name].clone()
    opt.step()
    opt_twin.step()
    for name, _, _ in pol.layout():
        et = max_err(g32[name], g64[name])
        scale = max(1.0, float(g64[name].abs().max()))
        bound = lr * (5 * et + 1e-6 * scale) + 2 ** -22 * float(getattr(twin, name).detach().abs().max())     # ek + et, and the update's rounding
        diff = max_err(getattr(pol, name), getattr(twin, name))
        print("step %-10s diff %.3e bound %.3e" % (name, diff, bound))
        assert diff <= bound, (name, diff, bound)
    before = batch["value"].clone()
    nxt = env.sample(pol, steps, gamma=0.99, lambda_=0.95)
    torch.cuda.synchronize()
    with torch.no_grad():
        _, v = pol(torch.cat([batch["obs"][-1:], nxt["obs"][:-1]]))
    assert float((v - nxt["value"]).abs().max()) < 1e-3        # the rollout used the updated weights
    assert torch.isfinite(nxt["advantages"]).all() and not torch.equal(before, nxt["value"])
