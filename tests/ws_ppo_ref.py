"""The float64 reference of ppo_loss_watershed (include/ssd.h, WATERSHED PPO LOSS AND GRADIENTS): WatershedLSTMPolicy.double()
run window by window through forward_sequence, each window from the recorded state (detached: data) with the resets the starts
give, then ws_ppo_terms under torch autograd; runnable in float32 on the device as the tests' yardstick.  Also the inputs the
tests use -- built from that float64 forward so that no row lies near a clip boundary -- and a branch report.

What the makers guarantee: make_policy scales column 1 of out_w (log_std of an action agent) to an L1 norm of 0.9 and draws
out_b[:, 1] within +-0.1, and |h'| < 1, so |log_std| <= 1.0 for every row whatever the inputs; make_inputs draws the Gaussian
actions within 2.5 standard deviations of the mean and the behaviour's log_std within 0.3 of the current one."""
import copy

import numpy as np
import torch

from ppo_ref import HYPER, MARGIN, as_numpy_u32, max_err   # noqa: F401  (re-exported for the tests)
from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd.policy import PPO_STATS, WS_OBS, WatershedLSTMPolicy, ws_is_comm, ws_ppo_terms

SEQ, SEQ_COMM = _capi.SSD_WS_SEQ, _capi.SSD_WS_SEQ_COMM
STARTS_MODES = ("none", "mid", "window_start", "per_seq")
HYPER_KEYS = ("clip_param", "vf_clip_param", "vf_loss_coeff", "entropy_coeff", "kl_coeff")


def forward(pol, agent_id, obs, state, starts, T):
    """The state rule, window by window: obs [M,Q,12], state [S,Q,2,C], starts u8 [M,Q] or None -> (dist [M,Q,5], value [M,Q]).
    A window's first step takes state[w] as stored (its starts row is not looked at); later steps reset where starts is set."""
    M = obs.shape[0]
    dt = pol.dense0_w.dtype
    dists, values = [], []
    for w, m0 in enumerate(range(0, M, T)):
        m1 = min(m0 + T, M)
        resets = None
        if starts is not None:
            resets = starts[m0:m1].to(torch.bool).clone()
            resets[0] = False
        d, v, _ = pol.forward_sequence(agent_id, obs[m0:m1].to(dt), state[w].detach().to(dt), resets)
        dists.append(d)
        values.append(v)
    return torch.cat(dists), torch.cat(values)


def _terms(dist, value, t, comm, h, dtype, device):
    cast = lambda x: None if x is None else x.to(device=device, dtype=dtype)   # noqa: E731
    tt = {"actions": cast(t["actions"]), "logp_old": cast(t["logp_old"]), "advantages": cast(t["advantages"]),
          "value_targets": cast(t["value_targets"]), "vf_pred": cast(t["vf_pred"]),
          "behaviour_dist": cast(t.get("behaviour_dist")) if h["kl_coeff"] != 0 else None}
    return ws_ppo_terms(dist, value, tt, comm, *(h[k] for k in HYPER_KEYS))


def autograd_loss(policy, agent_id, t, h, T, dtype=torch.float64, device="cpu"):
    """The restatement under torch autograd on a copy of `policy` in `dtype` on `device` -> (loss, {stat: scalar}, {param: grad}),
    the gradients of every entry of every parameter (zero where autograd gave none)."""
    pol = copy.deepcopy(policy).to(device=device, dtype=dtype)
    pol.zero_grad()
    starts = None if t.get("starts") is None else t["starts"].to(device)
    dist, value = forward(pol, agent_id, t["obs"].to(device), t["state"].to(device), starts, T)
    terms = _terms(dist, value, t, bool(ws_is_comm(pol.variant, agent_id)), h, dtype, device)
    means = [x.mean() for x in terms]
    means[0].backward()
    grads = {}
    for name, _, _ in pol.layout():
        g = getattr(pol, name).grad
        grads[name] = torch.zeros_like(getattr(pol, name)) if g is None else g.detach().clone()
    return means[0].detach(), {k: m.detach() for k, m in zip(PPO_STATS, means)}, grads


def make_policy(variant, C, seed, local_obs=False, share_comm_layer=False, recur=2.0):
    """A WatershedLSTMPolicy whose outputs spread: the LSTM's matrices `recur` times their initial scale, so that h and c of one
    step move the next step's gates, biases that are not zero, the Categorical's and the mean's columns of out_w tripled, and
    the log_std column bounded as the module docstring says."""
    pol = WatershedLSTMPolicy(variant, local_obs=local_obs, cell_size=C, share_comm_layer=share_comm_layer, seed=seed)
    g = torch.Generator().manual_seed(3000 + seed)
    with torch.no_grad():
        pol.lstm_kernel.mul_(recur)
        pol.lstm_recurrent.mul_(recur)
        for name in ("dense0_b", "dense1_b", "lstm_bias", "out_b", "value_b"):
            getattr(pol, name).copy_(0.1 * torch.randn(getattr(pol, name).shape, generator=g))
        pol.out_w.mul_(3.0)
        pol.out_w[:, :, 1] *= 0.9 / pol.out_w[:, :, 1].abs().sum(1, keepdim=True)
        pol.out_b[:, 1].clamp_(-0.1, 0.1)
    return pol


def make_starts(mode, M, Q, T, g):
    """starts u8 [M,Q] or None: "mid": every sequence starts anew in the middle of each window (step T // 2 of it, where the
    window has one); "window_start": set on the windows' first steps only, where the call must not look; "per_seq": each
    sequence at a random step of its own (a window's first step included)."""
    if mode == "none":
        return None
    s = torch.zeros((M, Q), dtype=torch.uint8)
    if mode == "mid":
        for m in range(M):
            if m % T == max(T // 2, 1) and m % T != 0:
                s[m] = 1
    elif mode == "window_start":
        s[::T] = 1
    elif mode == "per_seq":
        s[torch.randint(0, M, (Q,), generator=g), torch.arange(Q)] = 1
    else:
        raise ValueError(mode)
    return s


def _forward64(policy, agent_id, t, T, device="cpu"):
    with torch.no_grad():
        pol = copy.deepcopy(policy).to(device=device, dtype=torch.float64)
        starts = None if t.get("starts") is None else t["starts"].to(device)
        out = forward(pol, agent_id, t["obs"].to(device), t["state"].to(device), starts, T)
    return tuple(x.cpu() for x in out)


def current_logp(dist, actions, comm):
    """float64 logp of `actions` under dist, by the head."""
    if comm:
        return torch.log_softmax(dist, -1).gather(-1, actions.long().unsqueeze(-1)).squeeze(-1)
    z = (actions.to(dist.dtype) - dist[..., 0]) / dist[..., 1].exp()
    return -0.5 * z * z - dist[..., 1] - float(np.float32(0.9189385))


def make_inputs(policy, agent_id, M, Q, T, seed, behaviour=True, starts_mode="none"):
    """Sequences for agent `agent_id` of `policy`: random observations in [0, 1) (zero beyond the agent's observation length, as
    the engine pads them) and window states, starts by `starts_mode`, actions by the head (a message index, or a sample within
    2.5 standard deviations of the float64 mean), and logp_old / vf_pred set from the float64 forward so that the ratio and
    value - vf_pred land in chosen regions on either side of the clip boundaries (the recipe of ppo_ref.make_inputs)."""
    g = torch.Generator().manual_seed(seed)
    C = policy.cell_size
    comm = bool(ws_is_comm(policy.variant, agent_id))
    rows = (M, Q)
    S = -(-M // T)
    obs = torch.rand(rows + (WS_OBS,), generator=g)
    obs[..., policy.obs_lens[agent_id]:] = 0.0
    t = {"obs": obs, "state": 0.5 * torch.randn((S, Q, 2, C), generator=g)}
    starts = make_starts(starts_mode, M, Q, T, g)
    if starts is not None:
        t["starts"] = starts
    dist, value = _forward64(policy, agent_id, t, T)
    if comm:
        t["actions"] = torch.randint(0, 5, rows, generator=g).float()
    else:
        n = (5.0 * torch.rand(rows, generator=g, dtype=torch.float64) - 2.5)
        t["actions"] = (dist[..., 0] + dist[..., 1].exp() * n).float()
    logp = current_logp(dist, t["actions"].double(), comm)
    u = torch.rand(rows, generator=g, dtype=torch.float64)
    region = torch.randint(0, 4, rows, generator=g)
    # ratio in [0.45, 0.65], [0.75, 0.95], [1.05, 1.25] or [1.35, 1.6]: 0.05 and more from 1 - c = 0.7 and 1 + c = 1.3
    lo = torch.tensor([0.45, 0.75, 1.05, 1.35], dtype=torch.float64)[region]
    ratio = lo + u * torch.tensor([0.2, 0.2, 0.2, 0.25], dtype=torch.float64)[region]
    sign = torch.where(torch.rand(rows, generator=g) < 0.5, -1.0, 1.0).double()
    mag = torch.where(torch.rand(rows, generator=g) < 0.5, 0.1 + 0.7 * u, 1.2 + 0.8 * u)     # |value - vf_pred| against vc = 1
    t["logp_old"] = (logp - ratio.log()).float()
    t["vf_pred"] = (value - sign * mag).float()
    t["advantages"] = torch.randn(rows, generator=g) + torch.where(torch.rand(rows, generator=g) < 0.5, -0.3, 0.3)
    t["value_targets"] = (value + 1.5 * torch.randn(rows, generator=g, dtype=torch.float64)).float()
    if behaviour:
        noise = torch.randn(rows + (5,), generator=g, dtype=torch.float64)
        scale = torch.tensor([0.5] * 5 if comm else [0.3, 0.1, 0.5, 0.5, 0.5], dtype=torch.float64)
        t["behaviour_dist"] = (dist + (noise * scale).clamp(-3 * scale, 3 * scale)).float()
    return {k: v.contiguous() for k, v in t.items()}


def branch_report(policy, agent_id, t, h, T):
    """On the float64 reference: the share of rows in each surrogate case (clipped or not x sign of adv) and vf branch, and the
    smallest distance of any row from a boundary where a branch could flip."""
    c, vc = h["clip_param"], h["vf_clip_param"]
    comm = bool(ws_is_comm(policy.variant, agent_id))
    dist, value = _forward64(policy, agent_id, t, T)
    with torch.no_grad():
        adv, vt, vfp = t["advantages"].double(), t["value_targets"].double(), t["vf_pred"].double()
        ratio = torch.exp(current_logp(dist, t["actions"].double(), comm) - t["logp_old"].double())
        clipped = (ratio < 1 - c) | (ratio > 1 + c)
        dv = value - vfp
        vclip = dv.abs() > vc
        vf1 = (value - vt) ** 2
        vf2 = (vfp + dv.clamp(-vc, vc) - vt) ** 2
        dead = vclip & (vf1 < vf2)
        d = torch.minimum((ratio - (1 - c)).abs(), (ratio - (1 + c)).abs()).min()
        d = torch.minimum(d, (dv.abs() - vc).abs().min())
        if vclip.any():
            d = torch.minimum(d, (vf1 - vf2).abs()[vclip].min())
        log_std = float(dist[..., 1].abs().max())
    share = lambda m: float(m.double().mean())   # noqa: E731
    return {"clipped_pos": share(clipped & (adv > 0)), "clipped_neg": share(clipped & (adv < 0)),
            "open_pos": share(~clipped & (adv > 0)), "open_neg": share(~clipped & (adv < 0)),
            "vf_dead": share(dead), "vf_live": share(~dead), "vf_clipped_live": share(vclip & ~dead),
            "margin": float(d), "max_abs_log_std": log_std}


BRANCHES = ("clipped_pos", "clipped_neg", "open_pos", "open_neg", "vf_dead", "vf_live", "vf_clipped_live")


def bound(ref, et, factor=4.0):
    """The project's bound for one tensor: factor * et + 1e-6 * max(1, max |ref|)."""
    return factor * et + 1e-6 * max(1.0, float(ref.abs().max()))


def gather_own_steps(batch, obs_before, agent_id, T):
    """Agent `agent_id`'s own steps of a lock-step sample() batch, as examples/ppo_train_watershed.py gathers them: the steps k
    with actor[k] == agent_id (the same in every env, or ValueError), the observation each acted on (obs[k - 1], or
    obs_before for k = 0), the state ring of the windows' first steps, and starts from the done rows (their SSD_WS_DONE_ALL
    bit: the episode ended and the env was reset) between consecutive own steps.  Returns (seq dict of [M, E, ...] tensors, the list of steps)."""
    actor = batch["actor"]
    if not bool((actor == actor[:, :1]).all()):
        raise ValueError("the envs are not in lock step: actor[k] differs between envs")
    ks = torch.nonzero(actor[:, 0] == agent_id).flatten().tolist()
    if not ks:
        raise ValueError("agent %d does not act in the batch" % agent_id)
    idx = torch.tensor(ks, device=actor.device)
    prev = torch.cat([obs_before.unsqueeze(0), batch["obs"][:-1]])
    done = batch["done"]
    starts = torch.zeros((len(ks), actor.shape[1]), dtype=torch.uint8, device=actor.device)
    for m in range(1, len(ks)):
        starts[m] = ((done[ks[m - 1]:ks[m]] & _capi.SSD_WS_DONE_ALL) != 0).any(0).to(torch.uint8)
    seq = {"obs": prev[idx].contiguous(), "actions": batch["actions"][idx].contiguous(), "logp": batch["logp"][idx].contiguous(),
           "value": batch["value"][idx].contiguous(), "dist": batch["dist"][idx].contiguous(), "starts": starts,
           "state": batch["state_in"][idx[::T]].contiguous()}
    return seq, ks
