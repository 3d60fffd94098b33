"""The float64 reference of ppo_loss_watershed (include/ssd.h, WATERSHED PPO LOSS AND GRADIENTS): WatershedLSTMPolicy.double()
run window by window through forward_sequence, each window from the recorded state (detached: data) with the resets the starts
give, then ws_ppo_terms under torch autograd; runnable in float32 on the device as the tests' yardstick.  Also the inputs the
tests use -- built from that float64 forward so that no row lies near a clip boundary -- and a branch report.

What the makers guarantee: make_policy scales column 1 of out_w (log_std of an action agent) to an L1 norm of 0.9 and draws
out_b[:, 1] within +-0.1, and |h'| < 1, so |log_std| <= 1.0 for every row whatever the inputs; make_inputs draws the Gaussian
actions within 2.5 standard deviations of the mean and the behaviour's log_std within 0.3 of the current one.  Both reaches
are keywords (log_std_reach, z_reach) for the tests of the Gaussian head away from log_std = 0; clipped_rows builds the rows
of the kink tests."""
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


def make_policy(variant, C, seed, local_obs=False, share_comm_layer=False, recur=2.0, log_std_reach=None):
    """A WatershedLSTMPolicy whose outputs spread: the LSTM's matrices `recur` times their initial scale, so that h and c of one
    step move the next step's gates, biases that are not zero, the Categorical's and the mean's columns of out_w tripled, and
    the log_std column bounded as the module docstring says.  With log_std_reach the log_std column of out_w is scaled to that
    L1 norm in the place of 0.9 (|log_std| <= log_std_reach + 0.1; how far the rows really go depends on h', which the tests
    that use it read off the float64 forward) and nothing else changes."""
    pol = WatershedLSTMPolicy(variant, local_obs=local_obs, cell_size=C, share_comm_layer=share_comm_layer, seed=seed)
    g = torch.Generator().manual_seed(3000 + seed)
    with torch.no_grad():
        pol.lstm_kernel.mul_(recur)
        pol.lstm_recurrent.mul_(recur)
        for name in ("dense0_b", "dense1_b", "lstm_bias", "out_b", "value_b"):
            getattr(pol, name).copy_(0.1 * torch.randn(getattr(pol, name).shape, generator=g))
        pol.out_w.mul_(3.0)
        pol.out_w[:, :, 1] *= (0.9 if log_std_reach is None else float(log_std_reach)) / pol.out_w[:, :, 1].abs().sum(1, keepdim=True)
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


def make_inputs(policy, agent_id, M, Q, T, seed, behaviour=True, starts_mode="none", z_reach=2.5):
    """Sequences for agent `agent_id` of `policy`: random observations in [0, 1) (zero beyond the agent's observation length, as
    the engine pads them) and window states, starts by `starts_mode`, actions by the head (a message index, or a sample within
    z_reach = 2.5 standard deviations of the float64 mean, uniform), and logp_old / vf_pred set from the float64 forward so that
    the ratio and value - vf_pred land in chosen regions on either side of the clip boundaries (the recipe of
    ppo_ref.make_inputs)."""
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
        n = (2.0 * z_reach * torch.rand(rows, generator=g, dtype=torch.float64) - z_reach)
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


def clipped_rows(policy, agent_id, t, T, live=False, vf_clip_param=1.0, seed=0):
    """logp_old, advantages, vf_pred and value_targets that put EVERY row of t on the clipped side of the surrogate, on both
    signs of the advantage, built from the float64 forward (ppo_ref.clipped_rows for this policy; for clip_param = 0.3 and
    entropy_coeff = kl_coeff = 0).  A seeded mask gives half the rows adv = +1 and ratio 1.5 (s1 = 1.5 > s2 = 1.3) and the
    other half adv = -1 and ratio 0.5 (s1 = -0.5 > s2 = -0.7): the clipped operand is the minimum, nothing flows through the
    ratio, and -surr is -1.3 or +0.7.  With vc = vf_clip_param and a random sign s per row, vf_pred = value - 3 vc s, so
    value - vf_pred clips to vc s and d2 = d1 - 2 vc s; value_targets = value - 0.2 vc s (d1 = 0.2 vc s, d2 = -1.8 vc s:
    vf2 - vf1 = 3.2 vc^2, dead, nothing through the value) or, live, value - 3 vc s (d1 = 3 vc s, d2 = vc s: vf1 - vf2 =
    8 vc^2, and d vf / d value = 2 d1)."""
    comm = bool(ws_is_comm(policy.variant, agent_id))
    dist, value = _forward64(policy, agent_id, t, T)
    g = torch.Generator().manual_seed(7000 + seed)
    rows = t["actions"].shape
    pos = torch.rand(rows, generator=g) < 0.5
    s = torch.where(torch.rand(rows, generator=g) < 0.5, -1.0, 1.0).double()
    vc = float(vf_clip_param)
    with torch.no_grad():
        logp = current_logp(dist, t["actions"].double(), comm)
        shift = torch.where(pos, float(np.log(1.5)), float(np.log(0.5))).double()
    return {"advantages": torch.where(pos, 1.0, -1.0).float().contiguous(), "logp_old": (logp - shift).float().contiguous(),
            "vf_pred": (value - 3.0 * vc * s).float().contiguous(),
            "value_targets": (value - (3.0 if live else 0.2) * vc * s).float().contiguous()}


# ---- the cases the kink tests and the wide-log_std tests share between their CPU guards and their GPU runs ----
KINK_SHAPE = dict(M=7, T=3, Q=17, C=64)
KINK_HYPER = dict(HYPER, entropy_coeff=0.0, kl_coeff=0.0)           # clip_param 0.3, vf_clip_param 1
KINK_AGENTS = ((SEQ_COMM, 5), (SEQ_COMM, 1), (SEQ, 0))              # an action agent, a comm agent, Seq's Gaussian
# kink_case's seeds are 600 / 700 + 10 variant + id; on the CPU (119 rows each): the shares of adv > 0 and adv < 0 are 0.471 and
# 0.529 (SeqComm 5), 0.437 and 0.563 (SeqComm 1), 0.454 and 0.546 (Seq 0), the margin 0.2 (the ratios' 0.2 from 0.7 and 1.3;
# |value - vf_pred| - vc = 2, |vf1 - vf2| = 3.2 dead and 8 live), |log_std| 0.17 at most
WIDE_SHAPE = dict(M=7, T=3, Q=33, C=64)
WIDE_LOG_STD_REACH, WIDE_Z_REACH = 64.0, 4.5
# (variant, agent) -> (make_policy's seed, make_inputs' seed), chosen on the CPU (test_ws_loss_kinks_cpu.py asserts the figures):
#   SeqComm 5: log_std -4.38 .. 4.52, max |z| 4.47, margin 4.7e-2, the smallest branch share 0.22 (vf_clipped_live)
#   Seq 0:     log_std -3.83 .. 3.44, max |z| 4.46, margin 5.0e-2, the smallest branch share 0.17 (vf_clipped_live)
# (of seeds 1 .. 8 at this reach, 1, 3, 6, 8 meet the conditions for SeqComm 5 and 2 .. 6 for Seq 0)
WIDE_SEEDS = {(SEQ_COMM, 5): (8, 408), (SEQ, 0): (2, 402)}


def kink_case(variant, agent_id, live):
    """(policy, sequences) of the clipped-rows case of (variant, agent_id): KINK_SHAPE, starts per sequence, no behaviour_dist,
    every row clipped on both signs of the advantage and its value branch dead (or, live, clipped and live)."""
    d = KINK_SHAPE
    pol = make_policy(variant, d["C"], seed=600 + 10 * variant + agent_id)
    t = make_inputs(pol, agent_id, d["M"], d["Q"], d["T"], seed=700 + 10 * variant + agent_id, behaviour=False, starts_mode="per_seq")
    t.update(clipped_rows(pol, agent_id, t, d["T"], live=live, vf_clip_param=KINK_HYPER["vf_clip_param"], seed=agent_id))
    return pol, t


def wide_case(variant, agent_id):
    """(policy, sequences, report) of the Gaussian head away from log_std = 0: WIDE_SHAPE, starts per sequence, behaviour_dist,
    the log_std column of out_w at WIDE_LOG_STD_REACH and the actions within WIDE_Z_REACH standard deviations.  report:
    branch_report under HYPER and, on the float64 forward, min_log_std, max_log_std and max_abs_z."""
    d = WIDE_SHAPE
    ps, ts = WIDE_SEEDS[(variant, agent_id)]
    pol = make_policy(variant, d["C"], seed=ps, log_std_reach=WIDE_LOG_STD_REACH)
    t = make_inputs(pol, agent_id, d["M"], d["Q"], d["T"], seed=ts, starts_mode="per_seq", z_reach=WIDE_Z_REACH)
    rep = branch_report(pol, agent_id, t, HYPER, d["T"])
    dist, _ = _forward64(pol, agent_id, t, d["T"])
    z = (t["actions"].double() - dist[..., 0]) / dist[..., 1].exp()
    rep.update(min_log_std=float(dist[..., 1].min()), max_log_std=float(dist[..., 1].max()), max_abs_z=float(z.abs().max()))
    return pol, t, rep


def assert_wide_conditions(rep):
    """The conditions of the wide case on the float64 reference alone."""
    assert rep["min_log_std"] < -3.5 and rep["max_log_std"] > 1.5 and rep["max_abs_z"] > 4.0, rep
    assert rep["margin"] > MARGIN, rep
    for k in BRANCHES:
        assert rep[k] >= 0.1, rep


def assert_kink_conditions(rep, live):
    """The guards of the clipped-rows cases on the float64 reference alone (clipped_pos + clipped_neg == 1 is asked for as: no
    open row, and the two shares one apart from 1 by float64 rounding at most)."""
    assert rep["open_pos"] == 0.0 and rep["open_neg"] == 0.0 and abs(rep["clipped_pos"] + rep["clipped_neg"] - 1.0) <= 1e-12, rep
    assert rep["clipped_pos"] > 0.3 and rep["clipped_neg"] > 0.3 and rep["margin"] > 0.1, rep
    assert (rep["vf_clipped_live"] == 1.0 and rep["vf_dead"] == 0.0) if live else (rep["vf_dead"] == 1.0), rep


WRONG_FORMULAS = ("dlogp_dls_z2", "dkl_dls_neg_q", "dkl_dmean_sd")


def gauss_formula_grads(policy, agent_id, t, h, T, wrong=None, a3c=False):
    """The header's explicit derivatives of an ACTION agent's row loss with respect to (mean, log_std, value) in float64 --
    WATERSHED PPO LOSS AND GRADIENTS, or with a3c WATERSHED A3C LOSS AND GRADIENTS (h: vf_loss_coeff and entropy_coeff) --
    pushed through the network by autograd -> {param: grad}.  wrong: one formula replaced by a plausible slip:
      "dlogp_dls_z2":  d logp / d log_std = z^2                              (for z^2 - 1)
      "dkl_dls_neg_q": d kl / d log_std = -q                                 (for 1 - q; PPO)
      "dkl_dmean_sd":  d kl / d mean = -(mean_old - mean) / exp(log_std)     (for exp(2 log_std); PPO)"""
    pol = copy.deepcopy(policy).double()
    pol.zero_grad()
    assert not ws_is_comm(pol.variant, agent_id) and wrong in (None,) + WRONG_FORMULAS
    dist, value = forward(pol, agent_id, t["obs"], t["state"], t.get("starts"), T)
    with torch.no_grad():
        mean, ls = dist[..., 0], dist[..., 1]
        sd = ls.exp()
        z = (t["actions"].double() - mean) / sd
        adv, vt = t["advantages"].double(), t["value_targets"].double()
        dlogp_dls = z * z if wrong == "dlogp_dls_z2" else z * z - 1.0
        if a3c:
            gl = -adv
            dkl_mean = dkl_ls = torch.zeros_like(z)
            klc, dvalue, rows = 0.0, h["vf_loss_coeff"] * (value - vt), 1
        else:
            c, vc, klc = h["clip_param"], h["vf_clip_param"], h["kl_coeff"]
            logp = -0.5 * z * z - ls - float(np.float32(0.9189385))
            ratio = torch.exp(logp - t["logp_old"].double())
            inside = (ratio >= 1 - c) & (ratio <= 1 + c)
            dsurr = torch.where(inside | (adv * ratio < adv * ratio.clamp(1 - c, 1 + c)), adv, torch.zeros_like(adv))
            gl = -dsurr * ratio
            dkl_mean = dkl_ls = torch.zeros_like(z)
            if klc != 0:
                b = t["behaviour_dist"].double()
                dm = b[..., 0] - mean
                q = (torch.exp(2 * b[..., 1]) + dm * dm) / torch.exp(2 * ls)
                dkl_mean = -dm / (sd if wrong == "dkl_dmean_sd" else torch.exp(2 * ls))
                dkl_ls = -q if wrong == "dkl_dls_neg_q" else 1.0 - q
            vfp = t["vf_pred"].double()
            vf1 = (value - vt) ** 2
            vf2 = (vfp + (value - vfp).clamp(-vc, vc) - vt) ** 2
            alive = ((value - vfp).abs() <= vc) | (vf1 >= vf2)
            dvalue = h["vf_loss_coeff"] * torch.where(alive, 2 * (value - vt), torch.zeros_like(value))
            rows = value.numel()
        ddist = torch.zeros_like(dist)
        ddist[..., 0] = gl * (z / sd) + klc * dkl_mean
        ddist[..., 1] = gl * dlogp_dls - h["entropy_coeff"] + klc * dkl_ls
    torch.autograd.backward([dist, value], [ddist / rows, dvalue / rows])
    grads = {}
    for name, _, _ in pol.layout():
        g = getattr(pol, name).grad
        grads[name] = torch.zeros_like(getattr(pol, name)) if g is None else g.detach().clone()
    return grads


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
