"""a3c_loss_watershed, evaluate_sequences and impala_loss_watershed without a GPU: the CPU path of the A3C call against the
float64 restatement (ws_a3c_ref.py) for a comm id and an action id, sums versus means, where the gradient of one id may land,
the evaluation against ws_forward_windows with the bootstrap's start rule, the IMPALA call as the A3C call fed with vtrace's
outputs, rhos == 1 under unchanged weights, and every new refusal held to its words."""
import copy
import os

import pytest
import torch

from sequential_social_dilemma_games_amd import (_capi, a3c_loss_watershed, evaluate_sequences, impala_loss_watershed, vtrace,
                                                 ws_a3c_terms)
from sequential_social_dilemma_games_amd.policy import (A3C_STATS, ConvFCPolicy, a3c_terms, ws_forward_windows, ws_is_comm, ws_logp,
                                                        ws_ppo_terms)
from ws_a3c_ref import (HYPER, IMPALA_HYPER, SEQ, SEQ_COMM, autograd_loss, evaluate, impala_autograd_loss, make_impala_inputs,
                        make_inputs, make_policy, row_terms)


@pytest.mark.parametrize("agent,mode", [(1, "per_seq"), (5, "mid"), (6, "window_start"), (2, "none")])
def test_cpu_path_is_the_restatement(agent, mode):
    """Loss, the four statistics and every gradient, for comm ids (1, 2) and action ids (5, 6), M = 7, T = 3, Q = 5."""
    pol = make_policy(SEQ_COMM, 64, seed=31)
    t = make_inputs(pol, agent, 7, 5, 3, seed=32 + agent, starts_mode=mode)
    p64 = copy.deepcopy(pol).double()
    p64.zero_grad()
    loss, stats = a3c_loss_watershed(p64, agent, t, seq_len=3, **HYPER)
    assert loss.dtype == torch.float64 and tuple(stats) == A3C_STATS
    loss.backward()
    ref_loss, ref_stats, ref_g = autograd_loss(pol, agent, t, HYPER, 3)
    assert abs(float(loss.detach()) - float(ref_loss)) <= 1e-12 * max(1.0, abs(float(ref_loss)))
    for k in A3C_STATS:
        assert abs(float(stats[k]) - float(ref_stats[k])) <= 1e-12 * max(1.0, abs(float(ref_stats[k]))), k
    for name in ref_g:
        got = getattr(p64, name).grad
        got = torch.zeros_like(ref_g[name]) if got is None else got
        assert float((got - ref_g[name]).abs().max()) <= 1e-12 * max(1.0, float(ref_g[name].abs().max())), name
        others = torch.ones(got.shape[0], dtype=torch.bool)
        others[agent % got.shape[0]] = False
        assert float(got[others].abs().max()) == 0.0, name        # every other id's rows: exactly zero
    assert float(p64.lstm_recurrent.grad[agent].abs().max()) > 0.0
    if not ws_is_comm(SEQ_COMM, agent):
        assert float(p64.out_w.grad[agent][:, 2:].abs().max()) == 0.0 and float(p64.out_b.grad[agent][2:].abs().max()) == 0.0


@pytest.mark.parametrize("comm", [False, True])
def test_terms_against_the_restatement_and_the_ppo_terms(comm):
    g = torch.Generator().manual_seed(3)
    dist = torch.randn((64, 5), generator=g, dtype=torch.float64)
    dist[:, 1].clamp_(-1, 1)
    value, adv, vt = (torch.randn(64, generator=g, dtype=torch.float64) for _ in range(3))
    acts = torch.randint(-1, 7, (64,), generator=g).double() if comm else dist[:, 0] + torch.randn(64, generator=g, dtype=torch.float64)
    t = {"actions": acts, "advantages": adv, "value_targets": vt}
    got = ws_a3c_terms(dist, value, t, comm, 0.5, 0.01)
    want = row_terms(dist, value, acts, adv, vt, comm, HYPER)
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) <= 1e-13
    if comm:                                                      # a comm head is a3c_terms with A = 5, the index clamped
        for a, b in zip(got, a3c_terms(dist, value, t, 0.5, 0.01)):
            assert torch.equal(a, b)
    # logp and the entropy are the PPO terms' own: with logp_old = 0, adv = 1 and no clip in reach -surr = -exp(logp)
    z = torch.zeros(64, dtype=torch.float64)
    ppo = ws_ppo_terms(dist, value, dict(t, logp_old=z, advantages=torch.ones_like(z), vf_pred=z, actions=acts.clamp(0, 4) if comm else acts),
                       comm, 1e9, 1.0, 0.0, 0.0, 0.0)
    assert float((torch.log(-ppo[1]) - ws_logp(dist, acts, comm)).abs().max()) <= 1e-12
    assert float((ppo[4] - got[3]).abs().max()) <= 1e-13


@pytest.mark.parametrize("agent", [1, 5])
def test_the_loss_is_a_sum_over_rows(agent):
    """Doubling Q with duplicated sequences doubles the loss, every statistic and every gradient."""
    pol = make_policy(SEQ_COMM, 64, seed=41).double()
    t = make_inputs(pol, agent, 5, 4, 2, seed=42 + agent, starts_mode="per_seq")
    twice = {k: torch.cat([v, v], dim=1).contiguous() for k, v in t.items()}
    pol.zero_grad()
    a, sa = a3c_loss_watershed(pol, agent, t, seq_len=2, **HYPER)
    a.backward()
    ga = pol.lstm_kernel.grad[agent].clone()
    pol.zero_grad()
    b, sb = a3c_loss_watershed(pol, agent, twice, seq_len=2, **HYPER)
    b.backward()
    a, b = a.detach(), b.detach()
    assert abs(float(b) - 2.0 * float(a)) <= 1e-12 * abs(float(a))
    for k in A3C_STATS:
        assert abs(float(sb[k]) - 2.0 * float(sa[k])) <= 1e-12 * max(1.0, abs(float(sa[k]))), k
    assert float((pol.lstm_kernel.grad[agent] - 2.0 * ga).abs().max()) <= 1e-12 * float(ga.abs().max())


def test_logp_value_and_dist_of_the_dict_are_ignored():
    pol = make_policy(SEQ_COMM, 64, seed=45).double()
    t = make_inputs(pol, 5, 4, 3, 2, seed=46)
    a, _ = a3c_loss_watershed(pol, 5, t, seq_len=2, **HYPER)
    bare = {k: t[k] for k in ("obs", "actions", "advantages", "value_targets", "state")}
    b, _ = a3c_loss_watershed(pol, 5, dict(bare, logp=None, value="nonsense", dist=None), seq_len=2, **HYPER)
    assert float(a.detach()) == float(b.detach())


@pytest.mark.parametrize("agent,with_start_next", [(1, True), (5, True), (5, False)])
def test_evaluate_sequences_is_ws_forward_windows_and_the_bootstrap_rule(agent, with_start_next):
    M, Q, T = 7, 5, 3
    pol = make_policy(SEQ_COMM, 64, seed=51).double()
    t = make_impala_inputs(pol, agent, M, Q, T, seed=52 + agent)
    if with_start_next:
        t["start_next"] = torch.tensor([1, 0, 0, 1, 0], dtype=torch.uint8)
    dist, value, logp, boot = evaluate_sequences(pol, agent, t, T)
    assert not dist.requires_grad and not boot.requires_grad
    with torch.no_grad():
        d, v, last = ws_forward_windows(pol, agent, t["obs"], t["state"], t["starts"], T, return_state=True)
        rd, rv, rboot, rlast = evaluate(pol, agent, t, T)
    assert torch.equal(dist, d) and torch.equal(value, v)
    assert float((dist - rd).abs().max()) <= 1e-13 and float((value - rv).abs().max()) <= 1e-13
    assert float((last - rlast).abs().max()) <= 1e-13 and float((boot - rboot).abs().max()) <= 1e-13
    comm = bool(ws_is_comm(SEQ_COMM, agent))
    assert torch.equal(logp, ws_logp(dist, t["actions"], comm))
    # the bootstrap row: the carried state, zero where start_next, never a state entry (M = 7, T = 3: no window starts there;
    # with M = 6 one would, and the rule must not change)
    agent_t = torch.full((Q,), agent, dtype=torch.int64)
    with torch.no_grad():
        carried = pol(t["obs_next"], agent_t, last, None)[1]
        fresh = pol(t["obs_next"], agent_t, torch.zeros_like(last), None)[1]
    if with_start_next:
        s = t["start_next"].bool()
        assert torch.equal(boot[s], fresh[s]) and torch.equal(boot[~s], carried[~s]) and not torch.equal(carried[s], fresh[s])
    else:
        assert torch.equal(boot, carried)
    six = {k: (v[:6].contiguous() if v.dim() >= 2 and v.shape[0] == M else v) for k, v in t.items()}
    six["state"] = torch.cat([t["state"][:2], torch.full_like(t["state"][:1], float("nan"))])     # state[6 // 3] is never read
    _, _, _, boot6 = evaluate_sequences(pol, agent, six, T)
    assert bool(torch.isfinite(boot6).all())
    # without obs_next there is no bootstrap
    assert evaluate_sequences(pol, agent, {k: v for k, v in t.items() if k not in ("obs_next", "start_next")}, T)[3] is None


@pytest.mark.parametrize("agent", [2, 6])
def test_impala_is_a3c_fed_with_vtrace(agent):
    M, Q, T = 7, 5, 3
    pol = make_policy(SEQ_COMM, 64, seed=61)
    t = make_impala_inputs(pol, agent, M, Q, T, seed=62 + agent)
    loss, stats = impala_loss_watershed(pol, agent, t, seq_len=T, **IMPALA_HYPER)
    dist, value, logp, boot = evaluate_sequences(pol, agent, dict(t, start_next=t["done"][-1]), T)
    rhos = torch.exp(logp - t["logp"])
    assert float((rhos - 1).abs().max()) > 0.05                   # the behaviour policy is another one
    vs, pg = vtrace(torch.zeros((M, Q), dtype=torch.int32), value, rhos, boot, t["done"], gamma=0.99, bonus=t["rew"], bonus_weight=1.0)
    want, wstats = a3c_loss_watershed(pol, agent, dict(t, advantages=pg, value_targets=vs), seq_len=T, vf_loss_coeff=0.5,
                                      entropy_coeff=0.01)
    assert float(loss.detach()) == float(want.detach()) and tuple(stats) == A3C_STATS
    for k in A3C_STATS:
        assert float(stats[k]) == float(wstats[k]), k
    # and against the float64 restatement of the whole call (float32 CPU path: a loose check that the pieces are wired right)
    ref_loss, ref_stats, _, ref_rhos = impala_autograd_loss(pol, agent, t, IMPALA_HYPER, T)
    assert float((rhos.double() - ref_rhos).abs().max()) <= 1e-4
    assert abs(float(loss.detach()) - float(ref_loss)) <= 1e-3 * max(1.0, abs(float(ref_loss)))
    # the targets are data: no gradient reaches the inputs, and the loss backpropagates into the id's rows only
    pol.zero_grad()
    loss.backward()
    assert float(pol.value_w.grad[agent].abs().max()) > 0.0 and float(pol.value_w.grad[agent - 1].abs().max()) == 0.0


@pytest.mark.parametrize("agent", [1, 5])
def test_unchanged_weights_give_rhos_of_exactly_one(agent):
    """logp recorded by evaluate_sequences itself (what a rollout under the same weights records) -> rhos == 1 exactly, and the
    V-trace targets are then the discounted returns' recursion with rho = 1."""
    M, Q, T = 6, 4, 3
    pol = make_policy(SEQ_COMM, 64, seed=71)
    t = make_impala_inputs(pol, agent, M, Q, T, seed=72 + agent)
    _, _, logp, _ = evaluate_sequences(pol, agent, t, T)
    t["logp"] = logp.clone()
    _, _, again, _ = evaluate_sequences(pol, agent, t, T)
    rhos = torch.exp(again - t["logp"])
    assert torch.equal(rhos, torch.ones_like(rhos))
    loss, _ = impala_loss_watershed(pol, agent, t, seq_len=T, **IMPALA_HYPER)
    assert bool(torch.isfinite(loss))


def test_refusals_are_held_to_their_words():
    pol = make_policy(SEQ_COMM, 64, seed=91)
    t = make_impala_inputs(pol, 5, 4, 3, 2, seed=92)
    t.update(advantages=torch.randn(4, 3), value_targets=torch.randn(4, 3))
    a3c = lambda p, i, s, T=2, **kw: a3c_loss_watershed(p, i, s, seq_len=T, **dict(HYPER, **kw))      # noqa: E731
    imp = lambda p, i, s, T=2, **kw: impala_loss_watershed(p, i, s, seq_len=T, **dict(IMPALA_HYPER, **kw))      # noqa: E731
    ev = lambda p, i, s, T=2: evaluate_sequences(p, i, s, T)      # noqa: E731
    fc = ConvFCPolicy(num_actions=8, num_sets=1)
    cases = [
        (a3c, (fc, 5, t), {}, "a3c_loss_watershed is for a WatershedLSTMPolicy"),
        (ev, (fc, 5, t), {}, "evaluate_sequences is for a WatershedLSTMPolicy"),
        (imp, (fc, 5, t), {}, "impala_loss_watershed is for a WatershedLSTMPolicy"),
        (a3c, (pol, 8, t), {}, "agent_id must be 0..7"),
        (ev, (pol, True, t), {}, "agent_id must be 0..7"),
        (imp, (pol, -1, t), {}, "agent_id must be 0..7"),
        (a3c, (pol, 5, t, 0), {}, "seq_len must be an integer >= 1"),
        (ev, (pol, 5, t, 1.5), {}, "seq_len must be an integer >= 1"),
        (a3c, (pol, 5, t), dict(vf_loss_coeff=float("nan")), "the hyper-parameters must be finite"),
        (a3c, (pol, 5, t), dict(entropy_coeff=float("inf")), "the hyper-parameters must be finite"),
        (a3c, (pol, 5, [t]), {}, "seq must be a dict of [M, Q, ...] tensors"),
        (ev, (pol, 5, [t]), {}, "seq must be a dict of [M, Q, ...] tensors"),
        (imp, (pol, 5, [t]), {}, "seq must be a dict of [M, Q, ...] tensors"),
        (a3c, (pol, 5, dict(t, actions=t["actions"][0])), {}, "actions must be a float32 tensor [M, Q]"),
        (ev, (pol, 5, dict(t, actions=None)), {}, "actions must be a float32 tensor [M, Q]"),
        (a3c, (pol, 5, dict(t, advantages=None)), {}, "advantages must be a contiguous torch.float32 tensor of shape (4, 3) on cpu"),
        (a3c, (pol, 5, dict(t, value_targets=t["value_targets"].double())), {},
         "value_targets must be a contiguous torch.float32 tensor of shape (4, 3) on cpu"),
        (a3c, (pol, 5, dict(t, obs=t["obs"][..., :11].contiguous())), {}, "obs must be a contiguous torch.float32 tensor of shape (4, 3, 12) on cpu"),
        (a3c, (pol, 5, dict(t, state=t["state"][:1])), {}, "state must be [S, 3, 2, 64] with S >= ceil(M / seq_len) = 2"),
        (ev, (pol, 5, dict(t, state=t["state"][:1])), {}, "state must be [S, 3, 2, 64] with S >= ceil(M / seq_len) = 2"),
        (ev, (pol, 5, dict(t, obs_next=t["obs_next"][:2])), {}, "obs_next must be a contiguous torch.float32 tensor of shape (3, 12) on cpu"),
        (ev, (pol, 5, dict(t, start_next=torch.zeros(4, dtype=torch.uint8))), {},
         "start_next must be a contiguous torch.uint8 tensor of shape (3,) on cpu"),
        (ev, (pol, 5, dict(t, obs_next=None, start_next=torch.zeros(3, dtype=torch.uint8))), {}, "start_next needs obs_next"),
        (ev, (pol, 5, dict(t, starts=torch.zeros((4, 2), dtype=torch.uint8))), {},
         "starts must be a contiguous torch.uint8 tensor of shape (4, 3) on cpu"),
        (imp, (pol, 5, {k: v for k, v in t.items() if k != "logp"}), {}, "logp is required"),
        (imp, (pol, 5, {k: v for k, v in t.items() if k != "rew"}), {}, "rew is required"),
        (imp, (pol, 5, {k: v for k, v in t.items() if k != "done"}), {}, "done is required"),
        (imp, (pol, 5, {k: v for k, v in t.items() if k != "obs_next"}), {}, "obs_next is required"),
        (imp, (pol, 5, dict(t, rew=t["rew"].to(torch.int32))), {}, "rew must be a contiguous torch.float32 tensor of shape (4, 3) on cpu"),
        (imp, (pol, 5, dict(t, logp=t["logp"][:3])), {}, "logp must be a contiguous torch.float32 tensor of shape (4, 3) on cpu"),
        (imp, (pol, 5, dict(t, done=t["done"][:, :2].contiguous())), {}, "done must be a contiguous torch.uint8 tensor of shape (4, 3) on cpu"),
        (imp, (pol, 5, t), dict(clip_rho_threshold=0.0), "clip_rho_threshold and clip_pg_rho_threshold must be > 0 (inf: no clip)"),
    ]
    for fn, args, kw, words in cases:
        with pytest.raises(ValueError) as err:
            fn(*args, **kw)
        assert str(err.value) == words, (words, str(err.value))
    # a device policy refuses sequences on another device by the PPO call's words (no GPU needed: the meta device)
    with pytest.raises(ValueError) as err:
        a3c(copy.deepcopy(pol).to("meta"), 5, t)
    assert str(err.value) == "the policy is on meta, the sequences on cpu"


def test_header_python_and_library_agree():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "ssd.h")).read()
    for token in ("WATERSHED A3C LOSS AND GRADIENTS", "int ssd_ws_policy_ac_grad(", "WATERSHED SEQUENCE FORWARD",
                  "int ssd_ws_policy_forward_seq(", "#define SSD_ABI_VERSION 6"):
        assert token in hdr, token
    assert _capi.WS_A3C_SYMBOLS == ("ssd_ws_policy_ac_grad", "ssd_ws_policy_forward_seq")
    L = _capi.lib()
    for name in _capi.WS_A3C_SYMBOLS:
        assert name in _capi.SYMBOLS and hasattr(L, name) and not any(c.isdigit() for c in name)
    # the prototypes' lengths are the header's argument counts
    for name in _capi.WS_A3C_SYMBOLS:
        decl = hdr[hdr.index("int %s(" % name):]
        decl = decl[:decl.index(");")]
        assert len(getattr(L, name).argtypes) == decl.count(",") + 1, name
    assert isinstance(make_policy(SEQ, 64, seed=1).num_sets, int)
