"""The float64 reference of ppo_loss_moa (include/ssd.h, MOA PPO LOSS AND GRADIENTS): the ConvMOAPolicy's network restated
step by step from its parameters (conv, the two tanh stacks, the two Keras LSTMs, the heads and the prediction), stepped by
the state rule -- a window starts from the ring's state (detached: data), a step after a done row from a zero state and a zero
previous-action vector --, then ppo_ref's restatement of RLlib's PPOLoss plus moa_weight times the cross-entropy of the
predictions against the other agents' actions of the same step, under autograd.  Also the inputs the tests use -- built from
that float64 forward so that no row lies near a clip boundary, with weights scaled so that both recurrences and the MOA
stack's path into the conv carry gradient -- and deliberately wrong "kernels" (the `variant`s of forward and autograd_loss)
for the tests that ask whether the bound would notice."""
import copy

import torch

from ppo_lstm_ref import DONE_MODES, SPLIT_SHAPES, bound, make_done, rows_mask, shifted_obs, split_rows   # noqa: F401  (re-exported)
from ppo_ref import HYPER, MARGIN, as_numpy_u32, max_err, row_terms, set_means   # noqa: F401  (re-exported for the tests)
from sequential_social_dilemma_games_amd.policy import MOA_PPO_STATS, ConvMOAPolicy, _conv_flat, _dense, keras_lstm, other_agents

CONV_MARGIN = 1e-6         # no conv pre-activation of the reference may lie this close to its ReLU's kink (see conv_margin)
MOA_WEIGHT = 10.0          # train_moa.py's default is 10.0
VARIANTS = ("index_inputs", "index_targets", "no_stack1_conv", "cut_moa", "ignore_done_moa", "prev_not_zeroed", "ce_over_n",
            "no_moa_weight", "drop_last")
SPLIT_SEEDS = {"A": 241, "B": 233}   # shape of SPLIT_SHAPES -> the seed of make_policy (the inputs' is 100 more), chosen on the CPU
MOA_BRANCH = ("m_fc1_w", "m_fc1_b", "m_fc2_w", "m_fc2_b", "moa_kernel", "moa_recurrent", "moa_bias", "pred_w", "pred_b")
ACTIONS_BRANCH = ("a_fc1_w", "a_fc1_b", "a_fc2_w", "a_fc2_b", "lstm_kernel", "lstm_recurrent", "lstm_bias", "logits_w", "logits_b",
                  "value_w", "value_b")


def index_others(N):
    """The other agents of each agent in INDEX order: what a kernel that forgot the string order would use."""
    return torch.tensor([[n for n in range(N) if n != i] for i in range(N)], dtype=torch.int64).reshape(N, -1)


def step(pol, obs, prev, st, starts, variant=None):
    """One step of the network on obs u8 [E,N,15,15,3], prev int [E,N], st [E,N,4,C], starts bool [E,N] or None ->
    (logits [E,N,A], value [E,N], pred [E,N,N-1,A], new state)."""
    N, A, C = pol.num_agents, pol.num_actions, pol.cell_size
    w = pol._per_agent
    dev = obs.device
    flat = _conv_flat(pol, obs, N, w("conv_w"), w("conv_b"))                      # [E, N, 1014]
    ya = torch.tanh(_dense(torch.tanh(_dense(flat, w("a_fc1_w"), w("a_fc1_b"))), w("a_fc2_w"), w("a_fc2_b")))
    fm = flat.detach() if variant == "no_stack1_conv" else flat
    ym = torch.tanh(_dense(torch.tanh(_dense(fm, w("m_fc1_w"), w("m_fc1_b"))), w("m_fc2_w"), w("m_fc2_b")))
    zero = torch.zeros((), dtype=st.dtype, device=dev)
    s_act, s_moa = st[:, :, :2], st[:, :, 2:]
    others = (index_others(N) if variant == "index_inputs" else torch.from_numpy(other_agents(N))).to(dev)
    acts = torch.cat([prev[..., None], prev[:, others]], dim=-1).to(ya.dtype)     # [E, N, N]: own first
    if starts is not None:
        m = starts.to(torch.bool)
        s_act = torch.where(m[..., None, None], zero, s_act)
        if variant != "ignore_done_moa":
            s_moa = torch.where(m[..., None, None], zero, s_moa)
        if variant not in ("ignore_done_moa", "prev_not_zeroed"):
            acts = torch.where(m[..., None], zero, acts)
    if variant == "cut_moa":
        s_moa = s_moa.detach()
    h1, c1 = keras_lstm(ya[:, :, None], s_act[:, :, 0, None], s_act[:, :, 1, None], w("lstm_kernel"), w("lstm_recurrent"),
                        w("lstm_bias")[:, None])
    h1, c1 = h1[:, :, 0], c1[:, :, 0]
    logits = _dense(h1, w("logits_w"), w("logits_b"))
    value = _dense(h1, w("value_w"), w("value_b"))[..., 0]
    h2, c2 = keras_lstm(torch.cat([ym, acts], dim=-1)[:, :, None], s_moa[:, :, 0, None], s_moa[:, :, 1, None], w("moa_kernel"),
                        w("moa_recurrent"), w("moa_bias")[:, None])
    h2, c2 = h2[:, :, 0], c2[:, :, 0]
    pred = _dense(h2, w("pred_w"), w("pred_b")).reshape(h2.shape[0], N, N - 1, A)
    return logits, value, pred, torch.stack([h1, c1, h2, c2], dim=2)


def forward(pol, obs, prev, state, done, T, variant=None, twin=None):
    """The state rule, step by step: obs u8 [K,E,N,15,15,3] (already shifted), prev int [K,E,N], state [S,E,N,4,C], done u8
    [K,E,N] or None -> (logits [K,E,N,A], value [K,E,N], pred [K,E,N,N-1,A]).  variant: None (the contract) or one of VARIANTS
    ("drop_last": the rows of a last window shorter than T give zero outputs without gradient).  twin: None, or (a copy of pol
    holding the same values, mask bool [K,E,N]): the masked rows take their logits, value, pred and new state from the copy, so
    that after backward the copy's .grad is exactly those rows' share of each weight gradient (ppo_lstm_ref.forward)."""
    K = obs.shape[0]
    dt = pol.conv_w.dtype
    outs = ([], [], [])
    st = None
    for k in range(K):
        if k % T == 0:
            st = state[k // T].detach().to(dt)
            starts = None
        else:
            starts = None if done is None else done[k - 1].to(torch.bool)
        lg, v, pr, nxt = step(pol, obs[k], prev[k], st, starts, variant)
        if twin is not None and bool(twin[1][k].any()):
            m = twin[1][k]
            lg2, v2, pr2, nxt2 = step(twin[0], obs[k], prev[k], st, starts, variant)
            lg, v = torch.where(m[..., None], lg2, lg), torch.where(m, v2, v)
            pr, nxt = torch.where(m[..., None, None], pr2, pr), torch.where(m[..., None, None], nxt2, nxt)
        st = nxt
        if variant == "drop_last" and K % T and k >= K - K % T:
            lg, v, pr = lg.detach() * 0, v.detach() * 0, pr.detach() * 0
        for o, x in zip(outs, (lg, v, pr)):
            o.append(x)
    return tuple(torch.stack(o) for o in outs)


def moa_ce(pred, actions, N, A, variant=None):
    """Per row, the mean over the other agents of the cross-entropy of pred [K,E,N,N-1,A] against their actions of the same
    step: [K,E,N]."""
    others = (index_others(N) if variant == "index_targets" else torch.from_numpy(other_agents(N))).to(actions.device)
    tgt = actions.long().clamp(0, A - 1)[..., others]                             # [K, E, N, N-1]
    ce = torch.logsumexp(pred, -1) - pred.gather(-1, tgt.unsqueeze(-1)).squeeze(-1)
    return ce.sum(-1) / (N if variant == "ce_over_n" else N - 1)


def _inputs(t, dtype, device):
    cast = lambda x: None if x is None else x.to(device=device, dtype=dtype)   # noqa: E731
    return (t["actions"].to(device), cast(t["logp_old"]), cast(t["advantages"]), cast(t["value_targets"]), cast(t["vf_pred"]),
            cast(t.get("behaviour_logits")))


def autograd_loss(policy, t, h, obs_first, T, moa_weight=MOA_WEIGHT, dtype=torch.float64, device="cpu", variant=None, branch=None,
                  twin_rows=None):
    """The restatement under torch autograd on a copy of `policy` in `dtype` on `device` -> (loss, {stat: [P]}, {param: grad}).
    With a variant the loss is still divided by the whole fragment's rows, as a kernel with that fault would.  branch: None, or
    "ppo" / "moa" for that term of the loss alone.  With twin_rows (bool [K,E,N], see rows_mask) the gradients are {param: (the
    other rows' share, those rows' share)}, as in ppo_lstm_ref.autograd_loss."""
    pol = copy.deepcopy(policy).to(device=device, dtype=dtype)
    pol.zero_grad()
    twin = None if twin_rows is None else (copy.deepcopy(pol), twin_rows.to(device))
    N, A = pol.num_agents, pol.num_actions
    K = t["actions"].shape[0]
    beh = t.get("behaviour_logits") if h["kl_coeff"] != 0 else None
    obs = shifted_obs(t["obs"], obs_first, K).to(device)
    done = None if t.get("done") is None else t["done"].to(device)
    logits, value, pred = forward(pol, obs, t["prev_actions"].to(device), t["state"].to(device), done, T, variant, twin)
    acts, lpo, adv, vt, vfp, b = _inputs(dict(t, behaviour_logits=beh), dtype, device)
    terms = list(row_terms(logits, value, acts, lpo, adv, vt, vfp, b, h)[:5])
    ce = moa_ce(pred, acts, N, A, variant)
    if variant == "drop_last" and K % T:
        keep = torch.zeros_like(terms[0])
        keep[:K - K % T] = 1
        terms = [x * keep for x in terms]
        ce = ce * keep
    weight = 1.0 if variant == "no_moa_weight" else moa_weight
    if branch == "ppo":
        total = terms[0]
    elif branch == "moa":
        total = weight * ce
    else:
        total = terms[0] + weight * ce
    means = [set_means(x, pol.num_sets) for x in [total] + terms[1:] + [ce]]
    loss = means[0].sum()
    loss.backward()
    grads = {}
    for name, _, _ in pol.layout():
        g = getattr(pol, name).grad
        grads[name] = torch.zeros_like(getattr(pol, name)) if g is None else g.detach().clone()
        if twin is not None:
            g2 = getattr(twin[0], name).grad
            grads[name] = (grads[name], torch.zeros_like(grads[name]) if g2 is None else g2.detach().clone())
    return loss.detach(), {k: m.detach() for k, m in zip(MOA_PPO_STATS, means)}, grads


def conv_margin(policy, obs, device="cpu"):
    """The distance of every row's conv pre-activations from zero, in float64: obs u8 [..., N, 15, 15, 3] -> [..., N] (the
    smallest |pre-activation| over the row's 169 positions and 6 filters).  The conv's ReLU has a kink there: a float32 sum of
    27 products rounds by some 1e-7 in an order-dependent way, so a pre-activation nearer to zero than that is positive in one
    float32 implementation and not in another, and d loss / d conv of that position (some 1e-3 of conv_w's gradient at these
    sizes) is in or out.  As with the clip boundaries of the loss (MARGIN), the tests' inputs keep away from it."""
    N = policy.num_agents
    pol = copy.deepcopy(policy).to(device=device, dtype=torch.float64)
    w, b = pol._per_agent("conv_w"), pol._per_agent("conv_b")
    with torch.no_grad():
        x = ((obs.to(device).double() - 128.0) / 255.0).reshape(-1, N, 15, 15, 3)
        x = x.permute(0, 1, 4, 2, 3).reshape(x.shape[0], N * 3, 15, 15)
        wc = w.permute(0, 4, 3, 1, 2).reshape(N * 6, 3, 3, 3)
        pre = torch.nn.functional.conv2d(x, wc, b.reshape(N * 6), groups=N)
        return pre.reshape(-1, N, 6 * 169).abs().amin(-1).reshape(obs.shape[:-3]).cpu()


def clear_of_kinks(policy, obs, g, device="cpu"):
    """obs with every row whose conv_margin is below CONV_MARGIN drawn again from g (some 0.6 % of the rows a pass), until
    none is left."""
    for _ in range(20):
        near = conv_margin(policy, obs, device) < CONV_MARGIN
        n = int(near.sum())
        if not n:
            return obs
        obs[near] = torch.randint(0, 256, (n, 15, 15, 3), dtype=torch.uint8, generator=g)
    raise AssertionError("observations stayed near the conv's kink")


def make_policy(A, N, P, C, seed, recur=3.0, pred=6.0):
    """A ConvMOAPolicy whose logits spread, whose biases are all non-zero, whose LSTM matrices are `recur` times their
    initialisation (h and c of one step move the next step's gates: the gradient through time is a real share) and whose
    pred_w is `pred` times Glorot's (the cross-entropy's gradient into the MOA LSTM, stack 1 and the conv is a real share of
    the conv's).  The stacks' first layers are halved, which keeps their tanh away from saturation."""
    pol = ConvMOAPolicy(A, num_agents=N, num_sets=P, cell_size=C, seed=seed)
    g = torch.Generator().manual_seed(3000 + seed)
    with torch.no_grad():
        pol.logits_w.mul_(12.0)
        pol.value_w.mul_(30.0)
        pol.pred_w.mul_(pred)
        for name in ("lstm_kernel", "lstm_recurrent", "moa_kernel", "moa_recurrent"):
            getattr(pol, name).mul_(recur)
        pol.moa_kernel[:, 32:].mul_(0.25)          # the action inputs are 0 .. A - 1, not O(1)
        for name in ("a_fc1_w", "m_fc1_w"):
            getattr(pol, name).mul_(0.5)
        for name, _, _ in pol.layout():
            if name.endswith("_b") or name.endswith("_bias"):
                p = getattr(pol, name)
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return pol


def _forward64(policy, obs, prev, state, done, T, device):
    """The float64 forward without gradient on `device`, its outputs back on the CPU."""
    with torch.no_grad():
        pol = copy.deepcopy(policy).to(device=device, dtype=torch.float64)
        out = forward(pol, obs.to(device), prev.to(device), state.to(device), None if done is None else done.to(device), T)
    return tuple(x.cpu() for x in out)


def make_inputs(policy, K, E, N, T, seed, obs_first=True, behaviour=True, done_mode="none", zero_ring=False, device="cpu"):
    """A fragment for `policy`: random observations (clear_of_kinks), actions (the cross-entropy's targets too), previous actions (zero where a
    done row precedes, as the rollout's ring holds them) and ring states (zero at a window start that follows a done row; all
    zero with zero_ring), done flags by `done_mode`, and logp_old / vf_pred set from the float64 forward so that the ratio and
    value - vf_pred land in chosen regions on either side of the clip boundaries (the recipe of ppo_ref.make_inputs).  Every
    random number is drawn on the CPU; `device` is where the float64 forward and conv_margin run.  Returns (t, obs_first or
    None)."""
    g = torch.Generator().manual_seed(seed)
    A, C = policy.num_actions, policy.cell_size
    rows = (K, E, N)
    S = -(-K // T)
    t = {"obs": torch.randint(0, 256, rows + (15, 15, 3), dtype=torch.uint8, generator=g),
         "actions": torch.randint(0, A, rows, dtype=torch.int32, generator=g),
         "prev_actions": torch.randint(0, A, rows, dtype=torch.int32, generator=g),
         "state": 0.5 * torch.randn((S, E, N, 4, C), generator=g)}
    if zero_ring:
        t["state"].zero_()
    done = make_done(done_mode, K, E, N, T, g)
    if done is not None:
        t["done"] = done
        for s in range(1, S):
            t["state"][s][done[s * T - 1].bool()] = 0.0
        ended = done[:K - 1].bool().any(-1)                      # an env whose episode ended: the whole joint action is zero
        t["prev_actions"][1:][ended] = 0
    first = torch.randint(0, 256, (E, N, 15, 15, 3), dtype=torch.uint8, generator=g) if obs_first else None
    t["obs"] = clear_of_kinks(policy, t["obs"], g, device)
    if obs_first:
        first = clear_of_kinks(policy, first, g, device)
    logits, value, _ = _forward64(policy, shifted_obs(t["obs"], first, K), t["prev_actions"], t["state"], done, T, device)
    with torch.no_grad():
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
    """On the float64 reference (its forward on `device`): the share of rows in each surrogate case (clipped or not x sign of adv) and vf branch, the
    smallest distance of any row from a boundary where a branch could flip, and the smallest conv_margin of a row."""
    c, vc = h["clip_param"], h["vf_clip_param"]
    K = t["actions"].shape[0]
    logits, value, _ = _forward64(policy, shifted_obs(t["obs"], obs_first, K), t["prev_actions"], t["state"], t.get("done"), T, device)
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
            "margin": float(dist), "conv_margin": float(conv_margin(policy, shifted_obs(t["obs"], obs_first, K), device).min())}


def stack_saturation(policy, obs):
    """The share of the two stacks' tanh outputs (both layers) beyond 0.99 in magnitude on obs u8 [..., N, 15, 15, 3]."""
    pol = copy.deepcopy(policy).double()
    w = pol._per_agent
    with torch.no_grad():
        flat = _conv_flat(pol, obs, pol.num_agents, w("conv_w"), w("conv_b"))
        outs = []
        for s in ("a", "m"):
            y1 = torch.tanh(_dense(flat, w(s + "_fc1_w"), w(s + "_fc1_b")))
            outs += [y1, torch.tanh(_dense(y1, w(s + "_fc2_w"), w(s + "_fc2_b")))]
    return max(float((y.abs() > 0.99).double().mean()) for y in outs)


def zero_policy(A, N, P, C):
    """A ConvMOAPolicy with every parameter zero: both cells' z = 0, so (h', c') = 0 from a zero state, value = 0, logits = 0
    and pred = 0 exactly."""
    pol = ConvMOAPolicy(A, num_agents=N, num_sets=P, cell_size=C, seed=0)
    with torch.no_grad():
        for name, _, _ in pol.layout():
            getattr(pol, name).zero_()
    return pol


def counting_inputs(A, C, K, E, N, T, seed):
    """ppo_ref.counting_inputs for the MOA call: a zero ring, zero previous actions, no done."""
    from ppo_ref import counting_inputs as base
    t, first = base(A, K, E, N, seed)
    t["state"] = torch.zeros((-(-K // T), E, N, 4, C))
    t["prev_actions"] = torch.zeros((K, E, N), dtype=torch.int32)
    return t, first


def clipped_rows(policy, t, first, T, live=False, seed=None):
    """ppo_ref.clipped_rows on the MOA policy's forward: every row clipped (adv = +1 at ratio 1.5) and dead (vf_pred = value + 2,
    value_targets = value + 0.2).  With a seed, both signs of the advantage: a seeded mask keeps that for half the rows and
    gives the other half adv = -1 at ratio 0.5 (s1 = -0.5 > s2 = -0.7: the clipped operand is the minimum again), and the side
    vf_pred lies on is random too (value - 2 s, value_targets = value - 0.2 s).  live: value_targets = value + 3, or with a
    seed value - 3 s: clipped and live, vf1 = 9 > vf2 = 4, d vf / d value = 2 (value - vt)."""
    import numpy as np
    with torch.no_grad():
        logits, value, _ = forward(copy.deepcopy(policy).double(), shifted_obs(t["obs"], first, t["actions"].shape[0]),
                                   t["prev_actions"], t["state"], t.get("done"), T)
        logp = torch.log_softmax(logits, -1).gather(-1, t["actions"].long().unsqueeze(-1)).squeeze(-1)
    rows = t["actions"].shape
    if seed is None:
        return {"advantages": torch.ones(rows), "logp_old": (logp - float(np.log(1.5))).float().contiguous(),
                "vf_pred": (value + 2.0).float().contiguous(), "value_targets": (value + (3.0 if live else 0.2)).float().contiguous()}
    g = torch.Generator().manual_seed(7000 + seed)
    pos = torch.rand(rows, generator=g) < 0.5
    s = torch.where(torch.rand(rows, generator=g) < 0.5, -1.0, 1.0).double()
    shift = torch.where(pos, float(np.log(1.5)), float(np.log(0.5))).double()
    return {"advantages": torch.where(pos, 1.0, -1.0).float().contiguous(), "logp_old": (logp - shift).float().contiguous(),
            "vf_pred": (value - 2.0 * s).float().contiguous(), "value_targets": (value - (3.0 if live else 0.2) * s).float().contiguous()}


def split_case(shape, C, splits, chunk):
    """The split case (shape of SPLIT_SHAPES, ordinary inputs, A = 8) that the CPU sensitivity tests and the GPU accuracy tests
    share -> (policy, t, obs_first, (K, T, E, N, P), split_rows' probes)."""
    d = SPLIT_SHAPES[shape]
    K, T, E, N, P = d["K_"], d["T"], d["E"], d["N"], d["P"]
    probes, _, _ = split_rows(K, T, E, N, P, splits, chunk)
    pol = make_policy(8, N, P, C, seed=SPLIT_SEEDS[shape])
    t, first = make_inputs(pol, K, E, N, T, seed=100 + SPLIT_SEEDS[shape], done_mode="per_env")
    return pol, t, first, (K, T, E, N, P), probes
