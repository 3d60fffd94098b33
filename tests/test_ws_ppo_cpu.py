"""ppo_loss_watershed without a GPU: the Gaussian and Categorical row terms of ws_ppo_terms against the rollout's own logp and a
NumPy restatement, the CPU path's gradients against central finite differences in float64, and where the gradient of one agent
id may land (its own entries only; a shared dense1's entry id % 4; nothing in the padded rows of dense0_w)."""
import copy
import os

import numpy as np
import pytest
import torch

from sequential_social_dilemma_games_amd import _capi, ppo_loss_watershed
from sequential_social_dilemma_games_amd.policy import (PPO_STATS, WatershedLSTMPolicy, sample_gaussian_host, unpack_gradient,
                                                        ws_is_comm, ws_ppo_terms)
from ws_ppo_ref import HYPER, HYPER_KEYS, SEQ, SEQ_COMM, autograd_loss, branch_report, make_inputs, make_policy

HV = tuple(HYPER[k] for k in HYPER_KEYS)
_trapezoid = getattr(np, "trapezoid", None) or np.trapz


def _rows(n, seed):
    g = np.random.default_rng(seed)
    mean, log_std = g.normal(size=n), g.uniform(-1.0, 1.0, size=n)
    u1, u2 = g.uniform(1e-3, 1.0, size=n), g.uniform(size=n)
    return mean, log_std, u1, u2


def test_gaussian_logp_is_the_rollouts():
    mean, log_std, u1, u2 = _rows(257, 1)
    a, logp, _ = sample_gaussian_host(mean, log_std, u1, u2, dtype=np.float64)
    dist = torch.zeros((257, 5), dtype=torch.float64)
    dist[:, 0], dist[:, 1] = torch.from_numpy(mean), torch.from_numpy(log_std)
    z = torch.zeros(257, dtype=torch.float64)
    t = {"actions": torch.from_numpy(a), "logp_old": z, "advantages": torch.ones(257, dtype=torch.float64), "value_targets": z,
         "vf_pred": z}
    # with logp_old = 0, adv = 1 and no clip in reach, -surr = -exp(logp)
    terms = ws_ppo_terms(dist, z, t, False, 1e9, 1.0, 0.0, 0.0, 0.0)
    assert float((torch.log(-terms[1]) - torch.from_numpy(logp)).abs().max()) <= 1e-12


@pytest.mark.parametrize("comm", [False, True])
def test_on_behaviour_kl_is_zero_and_ratio_one(comm):
    g = torch.Generator().manual_seed(2)
    dist = torch.randn((64, 5), generator=g, dtype=torch.float64)
    dist[:, 1].clamp_(-1, 1)
    if comm:
        acts = torch.randint(0, 5, (64,), generator=g).double()
        logp = torch.log_softmax(dist, -1).gather(-1, acts.long()[:, None])[:, 0]
    else:
        acts = dist[:, 0] + dist[:, 1].exp() * torch.randn(64, generator=g, dtype=torch.float64)
        logp = -0.5 * ((acts - dist[:, 0]) / dist[:, 1].exp()) ** 2 - dist[:, 1] - float(np.float32(0.9189385))
    adv = torch.randn(64, generator=g, dtype=torch.float64)
    z = torch.zeros(64, dtype=torch.float64)
    t = {"actions": acts, "logp_old": logp, "advantages": adv, "value_targets": z, "vf_pred": z, "behaviour_dist": dist.clone()}
    row, pol, vf, kl, ent = ws_ppo_terms(dist, z, t, comm, 0.3, 1.0, 0.0, 0.0, 1.0)
    assert float(kl.abs().max()) <= 1e-15
    assert float((pol + adv).abs().max()) <= 1e-14               # -surr = -adv * 1


def test_gaussian_entropy_and_kl_against_numpy():
    mean, log_std, _, _ = _rows(100, 3)
    mean_o, log_std_o, _, _ = _rows(100, 4)
    ent = log_std + float(np.float32(1.4189385))
    kl = log_std - log_std_o + (np.exp(2 * log_std_o) + (mean_o - mean) ** 2) / (2 * np.exp(2 * log_std)) - 0.5
    # the closed forms themselves, against the definitions: entropy 0.5 log(2 pi e) + log_std, KL by quadrature
    assert np.abs(ent - (0.5 * np.log(2 * np.pi * np.e) + log_std)).max() < 1e-7
    x = np.linspace(-40, 40, 400001)
    for i in (0, 17, 63):
        lp_o = -0.5 * ((x - mean_o[i]) / np.exp(log_std_o[i])) ** 2 - log_std_o[i] - 0.5 * np.log(2 * np.pi)
        lp = -0.5 * ((x - mean[i]) / np.exp(log_std[i])) ** 2 - log_std[i] - 0.5 * np.log(2 * np.pi)
        assert abs(_trapezoid(np.exp(lp_o) * (lp_o - lp), x) - kl[i]) < 1e-6 * max(1.0, abs(kl[i]))
    dist, beh = torch.zeros((100, 5), dtype=torch.float64), torch.zeros((100, 5), dtype=torch.float64)
    dist[:, 0], dist[:, 1] = torch.from_numpy(mean), torch.from_numpy(log_std)
    beh[:, 0], beh[:, 1] = torch.from_numpy(mean_o), torch.from_numpy(log_std_o)
    z = torch.zeros(100, dtype=torch.float64)
    t = {"actions": torch.from_numpy(mean), "logp_old": z, "advantages": z, "value_targets": z, "vf_pred": z, "behaviour_dist": beh}
    terms = ws_ppo_terms(dist, z, t, False, 0.3, 1.0, 0.0, 0.0, 1.0)
    assert np.abs(terms[3].numpy() - kl).max() <= 1e-12 and np.abs(terms[4].numpy() - ent).max() <= 1e-12


def _loss64(pol, agent, t, T):
    loss, _ = ppo_loss_watershed(pol, agent, t, seq_len=T, **HYPER)
    return loss.detach()


@pytest.mark.parametrize("agent", [1, 5])
def test_cpu_path_against_finite_differences(agent):
    """M = 3, T = 2, Q = 2, C = 64 on SeqComm, a comm id and an action id: central differences in float64 through the public
    call, at entries of every parameter.  (The inputs keep every row 0.05 from a kink, so a step of 1e-6 crosses none.)"""
    M, T, Q = 3, 2, 2
    pol = make_policy(SEQ_COMM, 64, seed=10 + agent)
    t32 = make_inputs(pol, agent, M, Q, T, seed=20 + agent, starts_mode="none")
    assert branch_report(pol, agent, t32, HYPER, T)["margin"] > 1e-3
    pol = pol.double()
    pol.zero_grad()
    loss, stats = ppo_loss_watershed(pol, agent, t32, seq_len=T, **HYPER)
    assert loss.dtype == torch.float64 and set(stats) == set(PPO_STATS)
    loss.backward()
    g = torch.Generator().manual_seed(agent)
    eps = 1e-6
    for name, shape, _ in pol.layout():
        p = getattr(pol, name)
        own = p.grad[agent]
        flat = p.data[agent].reshape(-1)
        picks = torch.randperm(flat.numel(), generator=g)[:6].tolist() + [int(own.abs().reshape(-1).argmax())]
        for i in picks:
            keep = float(flat[i])
            flat[i] = keep + eps
            up = float(_loss64(pol, agent, t32, T))
            flat[i] = keep - eps
            dn = float(_loss64(pol, agent, t32, T))
            flat[i] = keep
            fd = (up - dn) / (2 * eps)
            got = float(own.reshape(-1)[i])
            assert abs(fd - got) <= 1e-7 * max(1.0, abs(got)) + 1e-8, (name, i, fd, got)
        others = torch.ones(p.shape[0], dtype=torch.bool)
        others[agent] = False
        assert float(p.grad[others].abs().max()) == 0.0, name    # every other set's rows: exactly zero
    assert float(pol.lstm_recurrent.grad[agent].abs().max()) > 0.0


def test_cpu_path_is_the_restatement():
    pol = make_policy(SEQ_COMM, 64, seed=31)
    for agent, mode in ((5, "mid"), (2, "per_seq"), (6, "window_start")):
        t = make_inputs(pol, agent, 7, 5, 3, seed=32 + agent, starts_mode=mode)
        p64 = copy.deepcopy(pol).double()
        p64.zero_grad()
        loss, stats = ppo_loss_watershed(p64, agent, t, seq_len=3, **HYPER)
        loss.backward()
        ref_loss, ref_stats, ref_g = autograd_loss(pol, agent, t, HYPER, 3)
        assert abs(float(loss) - float(ref_loss)) <= 1e-14
        for k in PPO_STATS:
            assert abs(float(stats[k]) - float(ref_stats[k])) <= 1e-14, k
        for name in ref_g:
            got = getattr(p64, name).grad
            got = torch.zeros_like(ref_g[name]) if got is None else got
            assert float((got - ref_g[name]).abs().max()) <= 1e-14, name


def test_starts_at_a_window_start_are_ignored_and_state_gets_no_gradient():
    pol = make_policy(SEQ_COMM, 64, seed=41).double()
    t = make_inputs(pol, 5, 6, 3, 3, seed=42, starts_mode="none")
    a, _ = ppo_loss_watershed(pol, 5, t, seq_len=3, **HYPER)
    s = torch.zeros((6, 3), dtype=torch.uint8)
    s[::3] = 1
    b, _ = ppo_loss_watershed(pol, 5, dict(t, starts=s), seq_len=3, **HYPER)
    assert float(a) == float(b)
    st = t["state"].clone().requires_grad_(True)
    c, _ = ppo_loss_watershed(pol, 5, dict(t, state=st), seq_len=3, **HYPER)
    c.backward()
    assert st.grad is None


def test_shared_comm_layer_gradient_lands_in_entry_id_mod_4():
    pol = make_policy(SEQ_COMM, 64, seed=51, share_comm_layer=True).double()
    assert pol.dense1_w.shape[0] == 4
    for agent in (1, 5):
        t = make_inputs(pol, agent, 4, 3, 2, seed=52 + agent)
        pol.zero_grad()
        loss, _ = ppo_loss_watershed(pol, agent, t, seq_len=2, **HYPER)
        loss.backward()
        for name in ("dense1_w", "dense1_b"):
            g = getattr(pol, name).grad
            assert float(g[1].abs().max()) > 0.0 and float(g[[0, 2, 3]].abs().max()) == 0.0, (agent, name)
        assert float(pol.dense0_w.grad[agent].abs().max()) > 0.0
    # and what unpack_gradient does with a packed set of one id: entry id % entries, the rest exactly zero
    pol32 = make_policy(SEQ_COMM, 64, seed=51, share_comm_layer=True)
    packed = torch.arange(pol32.set_floats, dtype=torch.float32) + 1.0
    for agent in (1, 5):
        out = dict(zip((n for n, _, _ in pol32.layout()), unpack_gradient(pol32, packed, only_set=agent)))
        for name, shape, off in pol32.layout():
            n = int(np.prod(shape))
            e = agent % getattr(pol32, name).shape[0]
            assert torch.equal(out[name][e].reshape(-1), packed[off:off + n]), name
            rest = torch.ones(out[name].shape[0], dtype=torch.bool)
            rest[e] = False
            assert float(out[name][rest].abs().max()) == 0.0, name
        assert out["dense1_w"].shape[0] == 4 and out["dense0_w"].shape[0] == 8


@pytest.mark.parametrize("variant,agent", [(SEQ_COMM, 5), (SEQ_COMM, 2), (SEQ, 0)])
def test_padded_dense0_rows_get_exactly_zero(variant, agent):
    pol = make_policy(variant, 64, seed=61, local_obs=True).double()
    n = pol.obs_lens[agent]
    assert n < 12
    t = make_inputs(pol, agent, 4, 3, 2, seed=62)
    assert float(t["obs"][..., n:].abs().max()) == 0.0
    loss, _ = ppo_loss_watershed(pol, agent, t, seq_len=2, **HYPER)
    loss.backward()
    g = pol.dense0_w.grad[agent]
    assert float(g[n:].abs().max()) == 0.0 and float(g[:n].abs().max()) > 0.0


def test_action_agent_unused_outputs_get_exactly_zero():
    pol = make_policy(SEQ, 64, seed=71).double()
    t = make_inputs(pol, 0, 5, 3, 2, seed=72)
    loss, _ = ppo_loss_watershed(pol, 0, t, seq_len=2, **HYPER)
    loss.backward()
    assert float(pol.out_w.grad[0][:, 2:].abs().max()) == 0.0 and float(pol.out_b.grad[0][2:].abs().max()) == 0.0
    assert float(pol.out_w.grad[0][:, :2].abs().max()) > 0.0


def test_makers_bound_log_std():
    for variant, agent in ((SEQ, 3), (SEQ_COMM, 7)):
        pol = make_policy(variant, 128, seed=81)
        t = make_inputs(pol, agent, 9, 40, 4, seed=82, starts_mode="per_seq")
        rep = branch_report(pol, agent, t, HYPER, 4)
        assert rep["max_abs_log_std"] <= 1.0 and not ws_is_comm(variant, agent)


def test_argument_errors():
    pol = make_policy(SEQ_COMM, 64, seed=91)
    t = make_inputs(pol, 5, 4, 3, 2, seed=92)
    with pytest.raises(ValueError):
        ppo_loss_watershed(pol, 8, t, seq_len=2, **HYPER)
    with pytest.raises(ValueError):
        ppo_loss_watershed(pol, 5, t, seq_len=0, **HYPER)
    with pytest.raises(ValueError):
        ppo_loss_watershed(pol, 5, {k: v for k, v in t.items() if k != "behaviour_dist"}, seq_len=2, **HYPER)
    with pytest.raises(ValueError):
        ppo_loss_watershed(pol, 5, dict(t, state=t["state"][:1]), seq_len=2, **HYPER)
    with pytest.raises(ValueError):
        ppo_loss_watershed(pol, 5, dict(t, obs=t["obs"][..., :11].contiguous()), seq_len=2, **HYPER)


def test_header_python_and_library_agree():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "ssd.h")).read()
    assert "WATERSHED PPO LOSS AND GRADIENTS" in hdr and "int ssd_ws_policy_ppo_grad(" in hdr
    assert "#define SSD_ABI_VERSION 6" in hdr
    assert "ssd_ws_policy_ppo_grad" in _capi.SYMBOLS and _capi.WS_PPO_SYMBOLS == ("ssd_ws_policy_ppo_grad",)
    assert hasattr(_capi.lib(), "ssd_ws_policy_ppo_grad")
    for token in ("SSD_WSPPO_TILE = 16", "SSD_WSPPO_CHUNK = 64", "SSD_WSPPO_MAX_GROUPS = 1024", "SSD_WSPPO_MAX_SPLITS = 32",
                  "SSD_WSPPO_MAX_TRUNK_GROUPS = 256", "#define SSD_WSPPO_ROW_FLOATS(C) (48 + 6 * (C))"):
        assert token in hdr, token
    # the scratch macro, term by term, for a shape with a short last window
    M, Q, C, T = 7, 33, 128, 3
    rows = 3 * 33
    want = (16 + C) * 4 * C + rows * (48 + 6 * C) + 7 * 576 + 3 * (8 * C + 8 + 16) + 2 * ((16 + C) * 4 * C + 4 * C)
    assert _capi.SSD_WSPPO_SCRATCH_FLOATS(M, Q, C, T) == want
    assert _capi.SSD_WSPPO_SCRATCH_FLOATS(700, Q, C, T) == want   # grows with one window's rows, not with M
    assert isinstance(WatershedLSTMPolicy(SEQ, cell_size=64), WatershedLSTMPolicy)
