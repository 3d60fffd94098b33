"""The float64 reference of a3c_loss_watershed, evaluate_sequences and impala_loss_watershed (include/ssd.h, WATERSHED A3C LOSS
AND GRADIENTS and WATERSHED SEQUENCE FORWARD), built on ws_ppo_ref's forward, policies, inputs and starts:
the state rule window by window, the A3C row terms of the head restated here (not the library's ws_a3c_terms) as SUMS over the
rows, differentiated by autograd; runnable in float32 on the device as the tests' yardstick.  For IMPALA: the sequences
evaluated step by step with the bootstrap row, the importance weights, V-trace in torch in the contract's order
(impala_ref.vtrace_torch) with the roundings of its float32 interface, and the A3C terms on the detached targets.  Also three
deliberately wrong losses (VARIANTS) for the tests that ask whether the bound would notice."""
import copy

import numpy as np
import torch

from impala_ref import vtrace_torch
from sequential_social_dilemma_games_amd.policy import A3C_STATS, WS_OBS, ws_is_comm
from ws_ppo_ref import (SEQ, SEQ_COMM, STARTS_MODES, bound, current_logp, forward, gather_own_steps, make_inputs,  # noqa: F401
                        make_policy, make_starts)
from ppo_ref import as_numpy_u32, max_err   # noqa: F401  (re-exported for the tests)

HYPER = dict(vf_loss_coeff=0.5, entropy_coeff=0.01)                        # a3c_causal.py's
IMPALA_HYPER = dict(gamma=0.99, vf_loss_coeff=0.5, entropy_coeff=0.01, clip_rho_threshold=1.0, clip_pg_rho_threshold=1.0)
# "mean": the terms as means over the rows; "vf_no_half": the value term without its half; "adv_sign": the advantage's sign flipped
VARIANTS = ("mean", "vf_no_half", "adv_sign")


def row_terms(dist, value, actions, adv, vt, comm, h, variant=None):
    """(row_loss, pi, vf, ent) per row in dist's dtype: the Categorical over the five outputs, or the Gaussian of (mean, log_std)."""
    dt = dist.dtype
    actions, adv, vt = actions.to(dt), adv.to(dt), vt.to(dt)
    if comm:
        lp_all = torch.log_softmax(dist, -1)
        logp = lp_all.gather(-1, actions.long().clamp(0, 4).unsqueeze(-1)).squeeze(-1)
        ent = -(lp_all.exp() * lp_all).sum(-1)
    else:
        z = (actions - dist[..., 0]) / dist[..., 1].exp()
        logp = -0.5 * z * z - dist[..., 1] - float(np.float32(0.9189385))
        ent = dist[..., 1] + float(np.float32(1.4189385))
    pi = -logp * (-adv if variant == "adv_sign" else adv)
    vf = (1.0 if variant == "vf_no_half" else 0.5) * (value - vt) ** 2
    return pi + h["vf_loss_coeff"] * vf - h["entropy_coeff"] * ent, pi, vf, ent


def _grads(pol):
    out = {}
    for name, _, _ in pol.layout():
        g = getattr(pol, name).grad
        out[name] = torch.zeros_like(getattr(pol, name)).detach() if g is None else g.detach().clone()
    return out


def autograd_loss(policy, agent_id, t, h, T, dtype=torch.float64, device="cpu", variant=None):
    """The restatement under torch autograd on a copy of `policy` in `dtype` on `device` -> (loss, {stat: scalar}, {param: grad})."""
    pol = copy.deepcopy(policy).to(device=device, dtype=dtype)
    pol.zero_grad()
    starts = None if t.get("starts") is None else t["starts"].to(device)
    dist, value = forward(pol, agent_id, t["obs"].to(device), t["state"].to(device), starts, T)
    terms = row_terms(dist, value, t["actions"].to(device), t["advantages"].to(device), t["value_targets"].to(device),
                      bool(ws_is_comm(pol.variant, agent_id)), h, variant)
    rows = t["actions"].numel()
    sums = [x.sum() / (rows if variant == "mean" else 1) for x in terms]
    sums[0].backward()
    return sums[0].detach(), {k: m.detach() for k, m in zip(A3C_STATS, sums)}, _grads(pol)


def zero_policy(variant, C):
    """Every parameter zero: dist = 0 and value = 0 on every row."""
    pol = make_policy(variant, C, seed=0)
    with torch.no_grad():
        for p in pol.parameters():
            p.zero_()
    return pol


# ---- the sequences under the current weights, step by step ----

def evaluate(pol, agent_id, t, T):
    """(dist [M,Q,5], value [M,Q], bootstrap [Q] or None, the state [Q,2,C] after step M - 1) with gradient: M + 1 single steps
    of the module's forward, by the state rule; the bootstrap row from the carried state, zero where start_next."""
    M, Q = t["actions"].shape
    dt = pol.dense0_w.dtype
    agent = torch.full((Q,), agent_id, dtype=torch.int64, device=t["obs"].device)
    starts, dists, values, st = t.get("starts"), [], [], None
    for m in range(M):
        if m % T == 0:
            st, s = t["state"][m // T].detach().to(dt), None
        else:
            s = None if starts is None else starts[m].to(torch.bool)
        d, v, st = pol(t["obs"][m].to(dt), agent, st, s)
        dists.append(d)
        values.append(v)
    boot = None
    if t.get("obs_next") is not None:
        s = None if t.get("start_next") is None else t["start_next"].to(torch.bool)
        boot = pol(t["obs_next"].to(dt), agent, st, s)[1]
    return torch.stack(dists), torch.stack(values), boot, st


def make_impala_inputs(policy, agent_id, M, Q, T, seed, starts_mode="per_seq", last_done=True):
    """make_inputs' sequences and besides float rewards, done (a quarter of the rows; on the last row of sequence 0 with
    last_done), obs_next, and logp from a BEHAVIOUR policy -- the policy of another seed in float64 by the same rule -- so that
    the importance weights spread on both sides of 1."""
    t = make_inputs(policy, agent_id, M, Q, T, seed=seed, behaviour=False, starts_mode=starts_mode)
    g = torch.Generator().manual_seed(7000 + seed)
    t["rew"] = (torch.randn((M, Q), generator=g) * 0.5).contiguous()
    t["done"] = (torch.rand((M, Q), generator=g) < 0.25).to(torch.uint8)
    if last_done:
        t["done"][M - 1, 0] = 1
    nxt = torch.rand((Q, WS_OBS), generator=g)
    nxt[..., policy.obs_lens[agent_id]:] = 0.0
    t["obs_next"] = nxt
    beh = make_policy(policy.variant, policy.cell_size, seed=seed + 50, local_obs=policy.local_obs,
                      share_comm_layer=policy.share_comm_layer).double()
    with torch.no_grad():
        dist, _, _, _ = evaluate(beh, agent_id, t, T)
        t["logp"] = current_logp(dist, t["actions"].double(), bool(ws_is_comm(policy.variant, agent_id))).float().contiguous()
    return t


def impala_autograd_loss(policy, agent_id, t, h, T):
    """impala_loss_watershed restated in float64 -> (loss, {stat: scalar}, {param: grad}, rhos): targets detached and rounded
    to float32 where the contract's interface rounds them; start_next defaults to done[M - 1]."""
    f64 = torch.float64
    pol = copy.deepcopy(policy).to(dtype=f64)
    pol.zero_grad()
    comm = bool(ws_is_comm(pol.variant, agent_id))
    tt = dict(t)
    if tt.get("start_next") is None:
        tt["start_next"] = t["done"][-1]
    dist, value, boot, _ = evaluate(pol, agent_id, tt, T)
    rnd = lambda x: x.detach().float().to(f64)                   # noqa: E731  (the contract's float32 interface)
    logp = current_logp(dist, t["actions"].double().clamp(0, 4) if comm else t["actions"].double(), comm)
    rhos = rnd(torch.exp(rnd(logp) - t["logp"].to(f64)))
    gamma = torch.full(value.shape, h["gamma"], dtype=f64)
    disc = torch.where(t["done"] != 0, torch.zeros((), dtype=f64), gamma)
    vs, pg = vtrace_torch(t["rew"].to(f64), rnd(value), rhos, rnd(boot), disc, h["clip_rho_threshold"], h["clip_pg_rho_threshold"])
    terms = row_terms(dist, value, t["actions"], rnd(pg), rnd(vs), comm, h)
    sums = [x.sum() for x in terms]
    sums[0].backward()
    return sums[0].detach(), {k: m.detach() for k, m in zip(A3C_STATS, sums)}, _grads(pol), rhos
