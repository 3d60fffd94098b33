"""The float64 reference of ppo_loss_recurrent (include/ssd.h, RECURRENT PPO LOSS AND GRADIENTS): ConvLSTMPolicy.double() run
window by window through forward_sequence, each window from the ring's state (detached: data) with the resets the done flags
give, then ppo_ref's restatement of RLlib's PPOLoss under autograd.  Also the inputs the tests use -- built from that float64
forward so that no row lies near a clip boundary, with weights scaled so that the recurrence carries gradient -- and three
deliberately wrong "kernels" (BPTT cut at every step, done ignored, the last ragged window dropped) for the tests that ask
whether the bound would notice."""
import copy

import torch

from ppo_ref import HYPER, MARGIN, as_numpy_u32, max_err, row_terms, set_means   # noqa: F401  (re-exported for the tests)
from sequential_social_dilemma_games_amd.policy import PPO_STATS, ConvLSTMPolicy

DONE_MODES = ("none", "mid", "window_end", "last", "per_env", "all")


def shifted_obs(obs, obs_first, K):
    """The observation each row acted on, by an explicit torch.cat."""
    return obs[:K] if obs_first is None else torch.cat([obs_first.unsqueeze(0), obs[:K - 1]])


def forward(pol, obs, state, done, T, variant=None, twin=None):
    """The state rule, step by step: obs u8 [K,E,N,15,15,3] (already shifted), state [S,E,N,2,C], done u8 [K,E,N] or None ->
    (logits [K,E,N,A], value [K,E,N]).  variant: None (the contract), "cut" (the state detached at every step: no BPTT),
    "ignore_done" (no resets), "drop_last" (the rows of a last window shorter than T give zero outputs without gradient).
    twin: None, or (a copy of pol holding the same values, mask bool [K,E,N]): the masked rows take their logits, value and new
    state from the copy.  Every value is unchanged and d x / d h still flow through every row, so after backward the copy's
    .grad is exactly the masked rows' share of each weight gradient and pol's .grad is the rest."""
    K = obs.shape[0]
    dt = pol.conv_w.dtype
    logits, value = [], []
    st = None
    for k in range(K):
        if k % T == 0:
            st = state[k // T].detach().to(dt)
            starts = None
        else:
            starts = None if done is None or variant == "ignore_done" else done[k - 1].to(torch.bool)
            if variant == "cut":
                st = st.detach()
        lg, v, nxt = pol(obs[k], st, starts)
        if twin is not None and bool(twin[1][k].any()):
            m = twin[1][k]
            lg2, v2, nxt2 = twin[0](obs[k], st, starts)
            lg, v, nxt = torch.where(m[..., None], lg2, lg), torch.where(m, v2, v), torch.where(m[..., None, None], nxt2, nxt)
        st = nxt
        if variant == "drop_last" and K % T and k >= K - K % T:
            lg, v = lg.detach() * 0, v.detach() * 0
        logits.append(lg)
        value.append(v)
    return torch.stack(logits), torch.stack(value)


def _inputs(t, dtype, device):
    cast = lambda x: None if x is None else x.to(device=device, dtype=dtype)   # noqa: E731
    return (t["actions"].to(device), cast(t["logp_old"]), cast(t["advantages"]), cast(t["value_targets"]), cast(t["vf_pred"]),
            cast(t.get("behaviour_logits")))


def autograd_loss(policy, t, h, obs_first, T, dtype=torch.float64, device="cpu", variant=None, twin_rows=None):
    """The restatement under torch autograd on a copy of `policy` in `dtype` on `device` -> (loss, {stat: [P]}, {param: grad}).
    With a variant the loss is still divided by the whole fragment's rows, as a kernel with that fault would.  With twin_rows
    (bool [K,E,N], see rows_mask) the gradients are {param: (the other rows' share, those rows' share)}: the two add up to the
    gradient, the first alone is what a kernel that lost those rows from its weight sums would return, the first plus twice the
    second what one that counted them twice would."""
    pol = copy.deepcopy(policy).to(device=device, dtype=dtype)
    pol.zero_grad()
    twin = None if twin_rows is None else (copy.deepcopy(pol), twin_rows.to(device))
    K = t["actions"].shape[0]
    beh = t.get("behaviour_logits") if h["kl_coeff"] != 0 else None
    obs = shifted_obs(t["obs"], obs_first, K).to(device)
    done = None if t.get("done") is None else t["done"].to(device)
    logits, value = forward(pol, obs, t["state"].to(device), done, T, variant, twin)
    acts, lpo, adv, vt, vfp, b = _inputs(dict(t, behaviour_logits=beh), dtype, device)
    terms = row_terms(logits, value, acts, lpo, adv, vt, vfp, b, h)[:5]
    if variant == "drop_last" and K % T:
        keep = torch.zeros_like(terms[0])
        keep[:K - K % T] = 1
        terms = [x * keep for x in terms]
    means = [set_means(x, pol.num_sets) for x in terms]
    loss = means[0].sum()
    loss.backward()
    grads = {}
    for name, _, _ in pol.layout():
        g = getattr(pol, name).grad
        grads[name] = torch.zeros_like(getattr(pol, name)) if g is None else g.detach().clone()
        if twin is not None:
            g2 = getattr(twin[0], name).grad
            grads[name] = (grads[name], torch.zeros_like(grads[name]) if g2 is None else g2.detach().clone())
    return loss.detach(), {k: m.detach() for k, m in zip(PPO_STATS, means)}, grads


def make_policy(A, P, C, seed, recur=4.0):
    """A ConvLSTMPolicy whose logits spread (the initial logits layer is 0.01-normed: a flat distribution), whose biases are
    not zero and whose lstm_w is `recur` times Glorot's, so that h and c of one step move the next step's gates: the gradient
    through time is a real share of lstm_w's and the trunk's (test_ppo_lstm_cpu.py asserts how large)."""
    pol = ConvLSTMPolicy(A, num_sets=P, cell_size=C, seed=seed)
    g = torch.Generator().manual_seed(2000 + seed)
    with torch.no_grad():
        pol.logits_w.mul_(300.0)
        pol.lstm_w.mul_(recur)
        for name in ("conv_b", "fc1_b", "fc2_b", "lstm_b", "logits_b", "value_b"):
            getattr(pol, name).copy_(0.1 * torch.randn(getattr(pol, name).shape, generator=g))
    return pol


def make_done(mode, K, E, N, T, g):
    """done u8 [K,E,N] or None: "mid": every sequence ends once in the middle of the first window (step 1 of it, or step 0 for
    T = 2); "window_end": at k = T - 1, so the next window's start is an episode start; "last": at K - 1 (never looked at);
    "per_env": each env ends at a random step of its own; "all": every row ends its episode."""
    if mode == "none":
        return None
    done = torch.zeros((K, E, N), dtype=torch.uint8)
    if mode == "mid":
        done[min(max(min(T, K) // 2 - 1, 0), K - 1)] = 1
    elif mode == "window_end":
        done[min(T, K) - 1] = 1
    elif mode == "last":
        done[K - 1] = 1
    elif mode == "all":
        done[:] = 1
    elif mode == "per_env":
        when = torch.randint(0, K, (E,), generator=g)
        done[when, torch.arange(E)] = 1
    else:
        raise ValueError(mode)
    return done


def _forward64(policy, obs, state, done, T, device):
    """The float64 forward without gradient on `device`, its outputs back on the CPU."""
    with torch.no_grad():
        pol = copy.deepcopy(policy).to(device=device, dtype=torch.float64)
        out = forward(pol, obs.to(device), state.to(device), None if done is None else done.to(device), T)
    return tuple(x.cpu() for x in out)


def make_inputs(policy, K, E, N, T, seed, obs_first=True, behaviour=True, done_mode="none", zero_ring=False, device="cpu"):
    """A fragment for `policy`: random observations, actions and ring states (zero at a window start that follows a done row, as
    a rollout records it; all zero with zero_ring), done flags by `done_mode`, and logp_old / vf_pred set from the float64
    forward so that the ratio and value - vf_pred land in chosen regions on either side of the clip boundaries (the recipe of
    ppo_ref.make_inputs).  Every random number is drawn on the CPU; `device` is where the float64 forward runs.  Returns (t,
    obs_first or None)."""
    g = torch.Generator().manual_seed(seed)
    A, C = policy.num_actions, policy.cell_size
    rows = (K, E, N)
    S = -(-K // T)
    t = {"obs": torch.randint(0, 256, rows + (15, 15, 3), dtype=torch.uint8, generator=g),
         "actions": torch.randint(0, A, rows, dtype=torch.int32, generator=g),
         "state": 0.5 * torch.randn((S, E, N, 2, C), generator=g)}
    if zero_ring:
        t["state"].zero_()
    done = make_done(done_mode, K, E, N, T, g)
    if done is not None:
        t["done"] = done
        for s in range(1, S):
            t["state"][s][done[s * T - 1].bool()] = 0.0
    first = torch.randint(0, 256, (E, N, 15, 15, 3), dtype=torch.uint8, generator=g) if obs_first else None
    logits, value = _forward64(policy, shifted_obs(t["obs"], first, K), t["state"], done, T, device)
    logp = torch.log_softmax(logits, -1).gather(-1, t["actions"].long().unsqueeze(-1)).squeeze(-1)
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
        t["behaviour_logits"] = (logits + 0.5 * torch.randn(rows + (A,), generator=g, dtype=torch.float64)).float()
    return {k: v.contiguous() for k, v in t.items()}, first


def branch_report(policy, t, h, obs_first, T, device="cpu"):
    """On the float64 reference (its forward on `device`): the share of rows in each surrogate case (clipped or not x sign of
    adv) and vf branch, and the smallest distance of any row from a boundary where a branch could flip."""
    c, vc = h["clip_param"], h["vf_clip_param"]
    K = t["actions"].shape[0]
    logits, value = _forward64(policy, shifted_obs(t["obs"], obs_first, K), t["state"], t.get("done"), T, device)
    with torch.no_grad():
        acts, lpo, adv, vt, vfp, b = _inputs(t, torch.float64, "cpu")
        ratio = row_terms(logits, value, acts, lpo, adv, vt, vfp, None, dict(h, kl_coeff=0.0))[5]
        clipped = (ratio < 1 - c) | (ratio > 1 + c)
        dv = value - vfp
        vclip = dv.abs() > vc
        vf1 = (value - vt) ** 2
        vf2 = (vfp + dv.clamp(-vc, vc) - vt) ** 2
        dead = vclip & (vf1 < vf2)
        dist = torch.minimum((ratio - (1 - c)).abs(), (ratio - (1 + c)).abs()).min()
        dist = torch.minimum(dist, (dv.abs() - vc).abs().min())
        if vclip.any():
            dist = torch.minimum(dist, (vf1 - vf2).abs()[vclip].min())
    share = lambda m: float(m.double().mean())   # noqa: E731
    return {"clipped_pos": share(clipped & (adv > 0)), "clipped_neg": share(clipped & (adv < 0)),
            "open_pos": share(~clipped & (adv > 0)), "open_neg": share(~clipped & (adv < 0)),
            "vf_dead": share(dead), "vf_live": share(~dead), "vf_clipped_live": share(vclip & ~dead),
            "margin": float(dist)}


def bound(ref, et, factor=4.0):
    """The project's bound for one tensor: factor * et + 1e-6 * max(1, max |ref|)."""
    return factor * et + 1e-6 * max(1.0, float(ref.abs().max()))


def zero_policy(A, P, C):
    """A ConvLSTMPolicy with every parameter zero: z = 0, so c' = h' = 0 from a zero state, and value = 0, logits = 0 exactly."""
    pol = ConvLSTMPolicy(A, num_sets=P, cell_size=C, seed=0)
    with torch.no_grad():
        for name, _, _ in pol.layout():
            getattr(pol, name).zero_()
    return pol


def counting_inputs(A, C, K, E, N, T, seed):
    """ppo_ref.counting_inputs for the recurrent call: a zero ring, no done."""
    from ppo_ref import counting_inputs as base
    t, first = base(A, K, E, N, seed)
    t["state"] = torch.zeros((-(-K // T), E, N, 2, C))
    return t, first


def clipped_rows(policy, t, first, T):
    """ppo_ref.clipped_rows on the recurrent forward: every row clipped and dead."""
    logits, value = _forward64(policy, shifted_obs(t["obs"], first, t["actions"].shape[0]), t["state"], t.get("done"), T, "cpu")
    with torch.no_grad():
        logp = torch.log_softmax(logits, -1).gather(-1, t["actions"].long().unsqueeze(-1)).squeeze(-1)
    import numpy as np
    return {"advantages": torch.ones(t["actions"].shape), "logp_old": (logp - float(np.log(1.5))).float().contiguous(),
            "vf_pred": (value + 2.0).float().contiguous(), "value_targets": (value + 0.2).float().contiguous()}


def set_policy(policy, p):
    """Weight set p of `policy` as a ConvLSTMPolicy of its own with one set."""
    one = ConvLSTMPolicy(policy.num_actions, num_sets=1, cell_size=policy.cell_size, seed=0)
    with torch.no_grad():
        for name, _, _ in policy.layout():
            getattr(one, name).copy_(getattr(policy, name)[p:p + 1])
    return one


def set_fragment(t, first, p):
    """Agent p's sequences of a [K, E, N] fragment as a [K, E, 1] fragment, the shifted observations passed explicitly (no
    obs_first)."""
    K = t["actions"].shape[0]
    out = {k: v[:, :, p:p + 1].contiguous() for k, v in t.items() if k != "obs"}
    out["obs"] = shifted_obs(t["obs"], first, K)[:, :, p:p + 1].contiguous()
    return out


# ---- the split-K kernels' second chunks ----
# Two windows; window 1 holds more than splits * chunk rows of one weight set, its last chunk ragged, so splits 0 .. take a
# second chunk; window 2 holds fewer chunks than there are splits, so most splits must keep what window 1 left.
# A: P = 1, 165 sequences, 2145 + 165 set rows (34 and 3 chunks of 64).  B: P = N = 2, 65 sequences per set, 2080 + 65 (33 and 2).
SPLIT_SHAPES = {"A": dict(K_=14, T=13, E=33, N=5, P=1), "B": dict(K_=33, T=32, E=65, N=2, P=2)}
# (shape, inputs, C) -> the seed of make_policy (the inputs' is 100 more), chosen on the CPU for the margin
SPLIT_SEEDS = {("A", "ordinary", 64): 202, ("A", "spotlight", 64): 202, ("A", "spotlight", 128): 202,
               ("B", "ordinary", 64): 211, ("B", "spotlight", 64): 211}


def split_rows(K, T, E, N, P, splits, chunk):
    """For a fragment of two windows, in window set rows (the split kernels' order: step-major, r = step * sequences + sequence;
    row r of set p is row r of the window's [steps][E][N] arrays for P = 1, row r * N + p for P = N) ->
    (probes {name: (window, range)}, lit [(window, range)], unlit (window, range)): the rows whose loss or double count a test
    must see, the rows a spotlight lights, and one row of window 1's last step between the lit ones."""
    seqs = E * N // P
    assert T < K <= 2 * T
    R1, R2 = T * seqs, (K - T) * seqs
    second = splits * chunk                                      # the first row of split 0's second chunk
    assert second < R1 < 2 * second and R1 % chunk and -(-R2 // chunk) < splits, (R1, R2, splits, chunk)
    probes = {"second_chunks": (0, range(second, R1)), "last_of_first_pass": (0, range(second - 1, second)),
              "first_of_second_pass": (0, range(second, second + 1)), "last_of_ragged_chunk": (0, range(R1 - 1, R1)),
              "window2_first": (1, range(0, 1)), "window2_last": (1, range(R2 - 1, R2))}
    lit = [(0, range(second - 8, second + 8)), (0, range(R1 - 16, R1)), (1, range(0, 8)), (1, range(R2 - 8, R2))]
    u = (second + 8 + R1 - 16) // 2
    assert second + 8 <= u < R1 - 16 and u >= (T - 1) * seqs      # unlit, and of the last step: nothing later feeds it gradient
    return probes, lit, (0, range(u, u + 1))


def rows_mask(K, T, E, N, P, rows):
    """rows: [(window, set, range of window set rows)] -> bool [K, E, N]."""
    m = torch.zeros(K * E * N, dtype=torch.bool)
    stride = 1 if P == 1 else N
    for window, p, rng in rows:
        steps = min(T, K - window * T)
        assert 0 <= p < P and 0 <= rng.start and rng.stop <= steps * (E * N // P), (window, p, rng)
        m[window * T * E * N + torch.arange(rng.start, rng.stop) * stride + p] = True
    return m.reshape(K, E, N)


def spotlight_inputs(policy, K, E, N, T, seed, lit, done_mode="none"):
    """A fragment in which single rows show: every row clipped and dead as clipped_rows makes them and, with entropy_coeff =
    kl_coeff = 0 and no behaviour logits, of exactly zero gradient -- but the rows `lit` ([(window, set, range)]), which are
    open (ratio e^+-0.1) and live (|value - vf_pred| = 0.5 < vc) with advantages of +-1000, so that one lit row is some 1e4
    bounds of lstm_w's gradient where an ordinary row is one.  Returns (t, obs_first, the hyper-parameters to use)."""
    t, first = make_inputs(policy, K, E, N, T, seed, behaviour=False, done_mode=done_mode)
    g = torch.Generator().manual_seed(seed + 7919)
    rows = (K, E, N)
    m = rows_mask(K, T, E, N, policy.num_sets, lit)
    logits, value = _forward64(policy, shifted_obs(t["obs"], first, K), t["state"], t.get("done"), T, "cpu")
    logp = torch.log_softmax(logits, -1).gather(-1, t["actions"].long().unsqueeze(-1)).squeeze(-1)
    sign = lambda: torch.where(torch.rand(rows, generator=g) < 0.5, -1.0, 1.0).double()   # noqa: E731
    dark = clipped_rows(policy, t, first, T)
    t = dict(t, logp_old=torch.where(m, (logp - 0.1 * sign()).float(), dark["logp_old"]),
             vf_pred=torch.where(m, (value + 0.5 * sign()).float(), dark["vf_pred"]),
             value_targets=torch.where(m, (value + 1.5 * torch.randn(rows, generator=g, dtype=torch.float64)).float(), dark["value_targets"]),
             advantages=torch.where(m, (1000.0 * sign()).float(), dark["advantages"]))
    return {k: v.contiguous() for k, v in t.items()}, first, dict(HYPER, entropy_coeff=0.0, kl_coeff=0.0)


def split_case(shape, inputs, C, splits, chunk):
    """The split case (shape of SPLIT_SHAPES, "ordinary" or "spotlight" inputs, cell size C) that the CPU sensitivity tests and
    the GPU accuracy tests share -> (policy, t, obs_first, hyper-parameters, (K, T, E, N, P), split_rows' result).  At P = N
    every set's rows are lit."""
    d = SPLIT_SHAPES[shape]
    K, T, E, N, P = d["K_"], d["T"], d["E"], d["N"], d["P"]
    rows = split_rows(K, T, E, N, P, splits, chunk)
    seed = SPLIT_SEEDS[shape, inputs, C]
    pol = make_policy(8, P, C, seed=seed)
    if inputs == "spotlight":
        t, first, h = spotlight_inputs(pol, K, E, N, T, 100 + seed, [(w, p, r) for w, r in rows[1] for p in range(P)], done_mode="per_env")
    else:
        t, first = make_inputs(pol, K, E, N, T, seed=100 + seed, done_mode="per_env")
        h = HYPER
    return pol, t, first, h, (K, T, E, N, P), rows
