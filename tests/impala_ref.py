"""The float64 reference of impala_loss, impala_loss_recurrent and impala_loss_moa: the fragment
evaluated under the policy's current weights step by step by the state rule (K rows and the bootstrap row), the importance
weights, V-trace in torch in the contract's operation order, and the A3C row terms of a3c_ref on the detached targets,
differentiated by autograd.  The roundings to float32 at vtrace's interface (value, rhos and bootstrap in, vs and pg out) are
the contract's and are restated; everything else is float64.  Also four deliberately wrong losses (VARIANTS) for the tests that
ask whether the bound would notice."""
import copy

import numpy as np
import torch

import a3c_ref
import ppo_moa_ref
import ppo_ref
from gae_ref import rewards
from ppo_lstm_ref import make_done
from sequential_social_dilemma_games_amd.policy import A3C_STATS, MOA_A3C_STATS

HYPER = dict(gamma=0.99, vf_loss_coeff=0.5, entropy_coeff=0.01, clip_rho_threshold=1.0, clip_pg_rho_threshold=1.0)
MOA_WEIGHT, INFLUENCE_WEIGHT = 10.0, 0.25
# "grad_vs": the gradient flows through vs into the value head; "no_clip": rho left unclipped in delta and pg;
# "stale_bootstrap": the bootstrap is batch["last_value"], the behaviour policy's; "ignore_done": the discount is gamma everywhere
VARIANTS = ("grad_vs", "no_clip", "stale_bootstrap", "ignore_done")
# wrong rules of the EVALUATION (evaluate's variant).  "no_shift": rows read obs[k] although obs_first is given; "boot_prev_row":
# the bootstrap reads the observation row K - 1 acted on; "boot_from_ring": when K % T == 0 the bootstrap row takes state[K // T]
# as stored, with no start rule; "boot_ignores_done": the bootstrap row gets starts = None; "carry_ignores_done": the loss rows
# that read the carried state get starts = None.  The last three do not apply to the conv-FC policy (eval_variants_of).
EVAL_VARIANTS = ("no_shift", "boot_prev_row", "boot_from_ring", "boot_ignores_done", "carry_ignores_done")


def eval_variants_of(kind):
    return EVAL_VARIANTS[:2] if kind == "fc" else EVAL_VARIANTS


def eval_variant_applies(kind, variant, t, first, T):
    """True where the wrong rule `variant` reads something else than the right one on this fragment: done is present and set
    where the rule looks; "boot_from_ring" needs K % T == 0 (and a ring entry state[K // T] to take, make_batch's ring_extra)."""
    K, done = t["actions"].shape[0], t.get("done")
    if variant == "boot_prev_row":
        return True
    if variant == "no_shift":
        return first is not None
    if kind == "fc":
        return False
    if variant == "boot_from_ring":
        return K % T == 0
    if done is None:
        return False
    if variant == "boot_ignores_done":
        return bool(done[K - 1].any())
    return any(bool(done[k - 1].any()) for k in range(1, K) if k % T)           # "carry_ignores_done"


def evaluate(kind, pol, t, first, T, variant=None):
    """(logits [K,E,N,A], value [K,E,N], pred or None, bootstrap [E,N]) with gradient: K + 1 steps, one after the other.
    variant: None (the contract) or one of EVAL_VARIANTS."""
    K = t["actions"].shape[0]
    rows = t["obs"][:K] if variant == "no_shift" else ppo_ref.shifted_obs(t["obs"], first, K)
    last = rows[K - 1:K] if variant == "boot_prev_row" else (t["obs"][K - 1:K] if first is not None else t["obs"][K:K + 1])
    obs = torch.cat([rows, last])
    if kind == "fc":
        logits, value = pol(obs)
        return logits[:K], value[:K], None, value[K]
    done, dt = t.get("done"), pol.conv_w.dtype
    outs, st = ([], [], []), None
    for k in range(K + 1):
        if k % T == 0 and (k < K or variant == "boot_from_ring"):
            st, starts = t["state"][k // T].detach().to(dt), None
        else:
            starts = None if done is None else done[k - 1].to(torch.bool)
            if variant == ("boot_ignores_done" if k == K else "carry_ignores_done"):
                starts = None
        if kind == "lstm":
            lg, v, nxt = pol(obs[k], st, starts)
            pr = None
        else:
            prev = t["actions"][K - 1] if k == K else t["prev_actions"][k]
            lg, v, pr, nxt = ppo_moa_ref.step(pol, obs[k], prev, st, starts, None)
        if k == K:
            return torch.stack(outs[0]), torch.stack(outs[1]), (None if kind == "lstm" else torch.stack(outs[2])), v
        st = nxt
        for o, x in zip(outs, (lg, v, pr)):
            o.append(x)


def vtrace_torch(r, value, rhos, boot, disc, clip_rho, clip_pg):
    """float64 tensors [K, ...] (boot [...]) -> (vs, pg) float64, in the contract's operation order, differentiable."""
    K = r.shape[0]
    acc, v_after, vs_after = torch.zeros_like(boot), boot, boot
    vs_rows, pg_rows = [None] * K, [None] * K
    for k in range(K - 1, -1, -1):
        rho, v = rhos[k], value[k]
        delta = rho.clamp(max=clip_rho) * ((r[k] + disc[k] * v_after) - v)
        acc = delta + (disc[k] * rho.clamp(max=1.0)) * acc
        vs = v + acc
        pg_rows[k] = rho.clamp(max=clip_pg) * ((r[k] + disc[k] * vs_after) - v)
        vs_rows[k] = vs
        v_after, vs_after = v, vs
    return torch.stack(vs_rows), torch.stack(pg_rows)


def targets(kind, t, logits, value, boot, h, variant=None):
    """(vs, pg, rhos) float64: data unless the variant says otherwise."""
    f64 = torch.float64
    acts = t["actions"].long().clamp(0, logits.shape[-1] - 1)
    logp = torch.log_softmax(logits, -1).gather(-1, acts.unsqueeze(-1)).squeeze(-1)
    rhos = torch.exp(logp - t["logp"].to(f64)).detach().float().to(f64)
    r = t["rew"].to(f64)
    if kind == "moa":
        r = r + INFLUENCE_WEIGHT * t["influence"].to(f64)
    done = t.get("done")
    gamma = torch.full(r.shape, h["gamma"], dtype=f64)
    disc = gamma if done is None or variant == "ignore_done" else torch.where(done != 0, torch.zeros((), dtype=f64), gamma)
    c_rho, c_pg = (float("inf"),) * 2 if variant == "no_clip" else (h["clip_rho_threshold"], h["clip_pg_rho_threshold"])
    if variant == "stale_bootstrap":
        boot = t["last_value"].to(f64)
    if variant == "grad_vs":                                     # (no rounding: the graph must stay whole)
        vs, pg = vtrace_torch(r, value, rhos, boot, disc, c_rho, c_pg)
        return vs, pg.detach(), rhos
    rnd = lambda x: x.detach().float().to(f64)                   # noqa: E731  (the contract's float32 interface)
    vs, pg = vtrace_torch(r, rnd(value), rhos, rnd(boot), disc, c_rho, c_pg)
    return rnd(vs), rnd(pg), rhos


def autograd_loss(kind, policy, t, h, first, T=None, moa_weight=MOA_WEIGHT, variant=None, eval_variant=None):
    """The restatement under torch autograd on a float64 copy of `policy` -> (loss, {stat: [P]}, {param: grad}, rhos).
    variant: one of VARIANTS (a wrong loss); eval_variant: one of EVAL_VARIANTS (a wrong evaluation under a right loss)."""
    pol = copy.deepcopy(policy).to(dtype=torch.float64)
    pol.zero_grad()
    P = pol.num_sets
    logits, value, pred, boot = evaluate(kind, pol, t, first, T, eval_variant)
    vs, pg, rhos = targets(kind, t, logits, value, boot, h, variant)
    terms = a3c_ref.row_terms(logits, value, t["actions"], pg, vs, h)
    rows = t["actions"].numel() // P
    sums = [a3c_ref.set_sums(x, P) for x in terms]
    names = A3C_STATS
    if kind == "moa":
        ce = a3c_ref.set_sums(ppo_moa_ref.moa_ce(pred, t["actions"], pol.num_agents, pol.num_actions), P) / rows
        sums[0] = sums[0] + moa_weight * ce
        sums.append(ce)
        names = MOA_A3C_STATS
    loss = sums[0].sum()
    loss.backward()
    grads = {}
    for name, _, _ in pol.layout():
        g = getattr(pol, name).grad
        grads[name] = torch.zeros_like(getattr(pol, name)).detach() if g is None else g.detach().clone()
    return loss.detach(), {k: m.detach() for k, m in zip(names, sums)}, grads, rhos


def make_batch(kind, A, N, P, K, E, T, seed, C=64, done_mode="per_env", last_done=True, ring_extra=0):
    """(the target policy, batch, obs_first): a3c_ref.make_inputs' fragment for the policy of `seed`, and besides rew (as the
    games pay it), done for the conv-FC policy too (at rate 0.25 for "per_env", ppo_lstm_ref.make_done's otherwise), influence
    for the MOA policy, and logp and last_value from a BEHAVIOUR policy -- the policy of another seed, in float64 by the same
    state rule -- so that the importance weights spread on both sides of 1.  last_done: True ends env 0 on the last row as well;
    "alternate" makes the last row of done 1 for every other env (0, 2, ...) and 0 for the rest, so that the bootstrap row's
    start rule has lanes of both kinds (no ring entry and no prev_actions depend on the last row).  ring_extra: that many more
    entries on the state ring than ceil(K / T), random as a stale entry would be; nothing may read them."""
    pol = a3c_ref.make_policy(kind, A, N, P, C=C, seed=seed)
    t, first = a3c_ref.make_inputs(kind, pol, K, E, N, T, seed=500 + seed, obs_first=True, done_mode=done_mode)
    g = torch.Generator().manual_seed(900 + seed)
    rng = np.random.default_rng(900 + seed)
    if t.get("done") is None and done_mode == "per_env":
        t["done"] = (torch.rand((K, E, N), generator=g) < 0.25).to(torch.uint8)
    elif t.get("done") is None and done_mode != "none":
        t["done"] = make_done(done_mode, K, E, N, min(T or K, K), g)
    if t.get("done") is not None and last_done == "alternate":
        t["done"][K - 1] = 0
        t["done"][K - 1, ::2] = 1
    elif t.get("done") is not None and last_done:
        t["done"][K - 1, 0] = 1
    t["rew"] = torch.from_numpy(rewards(rng, (K, E, N)))
    if kind == "moa":
        t["influence"] = torch.randn((K, E, N), generator=g).abs() * 0.5
    beh = a3c_ref.make_policy(kind, A, N, P, C=C, seed=seed + 50).to(dtype=torch.float64)
    with torch.no_grad():
        logits, _, _, boot = evaluate(kind, beh, t, first, T)
        t["logp"] = torch.log_softmax(logits, -1).gather(-1, t["actions"].long().unsqueeze(-1)).squeeze(-1).float()
        t["last_value"] = boot.float()
    if ring_extra and kind != "fc":
        stale = 0.5 * torch.randn((ring_extra,) + tuple(t["state"].shape[1:]), generator=torch.Generator().manual_seed(1300 + seed))
        t["state"] = torch.cat([t["state"], stale]).contiguous()
    return pol, t, first


# ---- the edge matrix of evaluate_fragment and the IMPALA calls (test_impala_loss_cpu.py, test_evaluate_fragment_gpu.py,
# ---- test_impala_loss_gpu.py): E = 17, N = 5 is two 16-row tiles per weight set at P = N, the second with one row ----
EDGE_E, EDGE_N = 17, 5


def edge(K, T, done, P=5, A=8, C=64, seed=1):
    return (K, T, done, P, A, C, seed)


# (K, T): whole windows only (4, 2) and (6, 3); K = 1 < T; T = 1; the ragged (5, 2); one window with T > K.  done: "none"
# (absent), "per_env" with the alternating last row, "window_end", "all".  P, A and C rotate.
EDGE_CASES = [edge(4, 2, "per_env", seed=1), edge(4, 2, "none", P=1, A=9, seed=2), edge(6, 3, "none", seed=3),
              edge(6, 3, "all", P=1, seed=4), edge(6, 3, "window_end", A=9, seed=5), edge(1, 2, "per_env", seed=6),
              edge(1, 2, "none", P=1, A=9, seed=7), edge(3, 1, "per_env", A=9, seed=8), edge(3, 1, "all", P=1, seed=9),
              edge(5, 2, "window_end", seed=10), edge(5, 2, "per_env", P=1, A=9, seed=11), edge(4, 8, "window_end", seed=12),
              edge(4, 8, "all", P=1, A=9, seed=13), edge(4, 2, "all", C=128, seed=14)]


def edge_id(case):
    return "K%d-T%d-%s-P%d-A%d-C%d" % case[:6]


def edge_batch(kind, case, E=EDGE_E, ring_extra=0):
    """make_batch for a case of EDGE_CASES; "per_env" gets the alternating last row."""
    K, T, done, P, A, C, seed = case
    return make_batch(kind, A, EDGE_N, P, K, E, T, seed=seed, C=C, done_mode=done, last_done="alternate" if done == "per_env" else True,
                      ring_extra=ring_extra)
