"""a3c_loss, a3c_loss_recurrent and a3c_loss_moa without a device: the plain-torch path against the float64 restatement
(a3c_ref.py), a one-row case worked by hand, the three C calls' refusals with their ssd_policy_last_error texts,
clip_grad_by_set_norm against a per-set loop, and the package's exports."""
import copy
import ctypes as C
import math

import pytest
import torch

import a3c_ref
from a3c_ref import HYPER, MOA_WEIGHT, autograd_loss, make_inputs, make_policy, max_err
from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd.policy import (A3C_STATS, MOA_A3C_STATS, ConvFCPolicy, ConvLSTMPolicy, a3c_loss, a3c_loss_moa,
                                                        a3c_loss_recurrent, clip_grad_by_set_norm)


def _call(kind, pol, t, first, T, h=HYPER, moa_weight=MOA_WEIGHT):
    if kind == "fc":
        return a3c_loss(pol, t, obs_first=first, **h)
    if kind == "lstm":
        return a3c_loss_recurrent(pol, t, seq_len=T, obs_first=first, **h)
    return a3c_loss_moa(pol, t, seq_len=T, moa_weight=moa_weight, obs_first=first, **h)


@pytest.mark.parametrize("kind,P,done", [("fc", 5, "none"), ("fc", 1, "none"), ("lstm", 5, "per_env"), ("lstm", 1, "mid"),
                                         ("moa", 5, "per_env"), ("moa", 1, "window_end")])
def test_torch_path_matches_the_restatement(kind, P, done):
    """The CPU path in float64 (the policy's dtype) is the restatement to rounding: loss, statistics and every gradient."""
    K_, E, N, T = 7, 3, 5, 3
    pol = make_policy(kind, 8, N, P, seed=3)
    t, first = make_inputs(kind, pol, K_, E, N, T, seed=103, done_mode=done)
    loss64, stats64, g64 = autograd_loss(kind, pol, t, HYPER, first, T)
    dpol = copy.deepcopy(pol).double()
    loss, stats = _call(kind, dpol, t, first, T)
    loss.backward()
    names = MOA_A3C_STATS if kind == "moa" else A3C_STATS
    assert tuple(stats) == names
    assert abs(float(loss) - float(loss64)) <= 1e-10 * max(1.0, abs(float(loss64)))
    for k in names:
        assert tuple(stats[k].shape) == (P,) and max_err(stats[k], stats64[k]) <= 1e-10 * max(1.0, float(stats64[k].abs().max())), k
    for name, _, _ in dpol.layout():
        g = getattr(dpol, name).grad
        g = torch.zeros_like(g64[name]) if g is None else g
        assert max_err(g, g64[name]) <= 1e-10 * max(1.0, float(g64[name].abs().max())), name
    # the loss is a sum over rows: twice the rows of the same fragment give twice the A3C terms
    assert float(stats["vf_loss"].sum()) > 0 and float(loss64) == pytest.approx(float(stats64["total_loss"].sum()))
    # the dict sample() returns carries logp, value and logits too: they are ignored
    noisy = dict(t, logp=torch.full_like(t["advantages"], float("nan")), value=None, logits="ignored")
    for k in ("logp_old", "vf_pred", "behaviour_logits"):
        noisy.pop(k, None)
    loss2, _ = _call(kind, dpol, noisy, first, T)
    assert float(loss2) == float(loss)


def test_one_row_by_hand():
    """A = 2, every weight zero but the value's bias b: logits = 0, value = b, so pi = adv ln 2, vf = 0.5 (b - vt)^2 and
    ent = ln 2; d loss / d value_b = vf_loss_coeff (b - vt) and d loss / d logits_b = -adv ([k = a] - 1/2) (the entropy's
    gradient vanishes at the uniform distribution)."""
    b, adv, vt, cv, ce = 0.75, -1.5, 2.0, 0.25, 0.125
    pol = ConvFCPolicy(2, num_sets=1, seed=0).double()
    with torch.no_grad():
        for name, _, _ in pol.layout():
            getattr(pol, name).zero_()
        pol.value_b.fill_(b)
    t = (torch.randint(0, 256, (1, 1, 1, 15, 15, 3), dtype=torch.uint8), torch.ones((1, 1, 1), dtype=torch.int32),
         torch.full((1, 1, 1), adv), torch.full((1, 1, 1), vt))
    loss, stats = a3c_loss(pol, t, vf_loss_coeff=cv, entropy_coeff=ce)
    loss.backward()
    ln2 = math.log(2.0)
    want = {"policy_loss": adv * ln2, "vf_loss": 0.5 * (b - vt) ** 2, "policy_entropy": ln2}
    want["total_loss"] = want["policy_loss"] + cv * want["vf_loss"] - ce * ln2
    for k in A3C_STATS:
        assert float(stats[k][0]) == pytest.approx(want[k], rel=1e-12), k
    assert float(loss) == pytest.approx(want["total_loss"], rel=1e-12)
    assert float(pol.value_b.grad.reshape(-1)[0]) == pytest.approx(cv * (b - vt), rel=1e-12)
    assert pol.logits_b.grad.reshape(-1).tolist() == pytest.approx([adv * 0.5, -adv * 0.5], rel=1e-12)


def test_python_argument_checks():
    pol = make_policy("fc", 8, 5, 5, seed=0)
    t, first = make_inputs("fc", pol, 2, 2, 5, None, seed=0)
    with pytest.raises(ValueError, match="value_targets"):
        a3c_loss(pol, {k: v for k, v in t.items() if k != "value_targets"}, obs_first=first, **HYPER)
    with pytest.raises(ValueError, match="weight sets"):
        a3c_loss(make_policy("fc", 8, 3, 3, seed=0), t, obs_first=first, **HYPER)
    with pytest.raises(ValueError, match="finite"):
        a3c_loss(pol, t, obs_first=first, vf_loss_coeff=float("inf"), entropy_coeff=0.0)
    with pytest.raises(ValueError, match="ConvFCPolicy"):
        a3c_loss(ConvLSTMPolicy(8, 5, 64), t, obs_first=first, **HYPER)
    with pytest.raises(ValueError, match="ConvLSTMPolicy"):
        a3c_loss_recurrent(pol, t, seq_len=2, obs_first=first, **HYPER)
    with pytest.raises(ValueError, match="ConvMOAPolicy"):
        a3c_loss_moa(pol, t, seq_len=2, moa_weight=1.0, obs_first=first, **HYPER)
    lpol = make_policy("lstm", 8, 5, 5, seed=0)
    lt, lfirst = make_inputs("lstm", lpol, 4, 2, 5, 2, seed=0)
    with pytest.raises(ValueError, match="seq_len"):
        a3c_loss_recurrent(lpol, lt, seq_len=0, obs_first=lfirst, **HYPER)
    with pytest.raises(ValueError, match="state"):
        a3c_loss_recurrent(lpol, {k: v for k, v in lt.items() if k != "state"}, seq_len=2, obs_first=lfirst, **HYPER)
    mpol = make_policy("moa", 8, 5, 5, seed=0)
    mt, mfirst = make_inputs("moa", mpol, 4, 2, 5, 2, seed=0)
    with pytest.raises(ValueError, match="moa_weight"):
        a3c_loss_moa(mpol, mt, seq_len=2, moa_weight=-1.0, obs_first=mfirst, **HYPER)
    with pytest.raises(ValueError, match="prev_actions"):
        a3c_loss_moa(mpol, {k: v for k, v in mt.items() if k != "prev_actions"}, seq_len=2, moa_weight=1.0, obs_first=mfirst, **HYPER)


def test_abi_argument_checks_need_no_device():
    """The three calls are exported and refuse bad arguments before anything is launched, with the reason in
    ssd_policy_last_error (lower-case argument names): the matching PPO call's refusals, less the arguments that are gone."""
    L = _capi.lib()
    for name in _capi.A3C_SYMBOLS:
        assert name in _capi.SYMBOLS and hasattr(L, name)
    A, N = 8, 5
    w = (C.c_float * 16)()
    buf = (C.c_double * 16)()
    p = lambda x: C.cast(x, C.c_void_p)   # noqa: E731
    q = lambda x: None if x is None else p(x)   # noqa: E731

    def call(kind, weights=w, P=N, A=A, C_=64, T=2, obs_first=None, obs=buf, state=buf, prev=buf, done=None, actions=buf, adv=buf,
             vt=buf, K=2, E=3, N=N, hyper=(0.5, 0.01), moa_weight=10.0, scratch=buf, grads=buf, stats=buf, flags=0):
        rows = (q(actions), q(adv), q(vt), K, E, N)
        tail = (q(scratch), q(grads), q(stats), 0, flags, None)
        if kind == "fc":
            rc = L.ssd_policy_ac_grad(q(weights), P, A, q(obs_first), q(obs), *rows, *hyper, *tail)
        elif kind == "lstm":
            rc = L.ssd_policy_lstm_ac_grad(q(weights), P, A, C_, T, q(obs_first), q(obs), q(state), q(done), *rows, *hyper, *tail)
        else:
            rc = L.ssd_policy_moa_ac_grad(q(weights), P, A, C_, T, q(obs_first), q(obs), q(state), q(prev), q(done), *rows, *hyper,
                                          moa_weight, *tail)
        return rc, L.ssd_policy_last_error().decode()

    odd = C.cast(C.addressof(buf) + 4, C.c_void_p)
    odd1 = C.cast(C.addressof(buf) + 1, C.c_void_p)
    common = ((dict(weights=None), "weights"), (dict(P=2), "num_sets"), (dict(A=16), "num_actions"), (dict(K=0), "n_steps"),
              (dict(E=0), "num_envs"), (dict(K=2 ** 20, E=2 ** 11), "2^31"), (dict(obs=None), "obs"),
              (dict(obs=None, obs_first=buf), "obs"), (dict(actions=None), "actions"), (dict(adv=None), "advantages"),
              (dict(vt=None), "value_targets"), (dict(scratch=None), "scratch"), (dict(grads=None), "grads"), (dict(stats=None), "stats"),
              (dict(scratch=odd), "aligned"), (dict(stats=odd), "aligned"), (dict(grads=odd1), "aligned"),
              (dict(hyper=(float("nan"), 0.01)), "finite"), (dict(hyper=(0.5, float("inf"))), "finite"), (dict(flags=1), "flags"))
    recurrent = ((dict(C_=100), "cell_size"), (dict(T=0), "seq_len"), (dict(state=None), "state"), (dict(state=odd1), "state"))
    table = {"fc": common + ((dict(N=0, P=1), "num_agents"),),
             "lstm": common + recurrent + ((dict(N=0, P=1), "num_agents"),),
             "moa": common + recurrent + ((dict(N=1, P=1), "2..16 agents"), (dict(N=17, P=17), "2..16 agents"), (dict(prev=None), "prev_actions"),
                                          (dict(prev=odd1), "prev_actions"), (dict(moa_weight=-1.0), "moa_weight"),
                                          (dict(moa_weight=float("nan")), "moa_weight"))}
    for kind, rows in table.items():
        for kw, why in rows:
            rc, msg = call(kind, **kw)
            assert rc == _capi.SSD_E_INVALID, (kind, kw, rc, msg)
            assert why in msg and msg.replace("MOA", "moa") == msg.lower(), (kind, kw, msg)
            for gone in ("logp_old", "vf_preds", "clip_param"):
                assert gone not in msg, (kind, kw, msg)
        # good arguments get as far as the device, which a box without one does not have
        if not torch.cuda.is_available():
            rc, msg = call(kind)
            assert rc in (_capi.SSD_E_INVALID, _capi.SSD_E_DEVICE) and "device" in msg.lower(), (kind, rc, msg)


def test_clip_grad_by_set_norm_matches_a_per_set_loop():
    """tf.clip_by_global_norm per weight set: a set below max_norm keeps its gradient to the bit, a set above it is scaled to
    max_norm, and the returned norms are those before clipping."""
    P = 5
    pol = make_policy("lstm", 8, 5, P, seed=1)
    g = torch.Generator().manual_seed(7)
    size = torch.tensor([0.001, 10.0, 0.01, 3.0, 0.002])                       # sets 1 and 3 end above max_norm, the others below
    for name, _, _ in pol.layout():
        prm = getattr(pol, name)
        prm.grad = torch.randn(prm.shape, generator=g) * size.reshape((P,) + (1,) * (prm.dim() - 1))
    before = {name: getattr(pol, name).grad.clone() for name, _, _ in pol.layout()}
    max_norm = 40.0
    norms = clip_grad_by_set_norm(pol, max_norm)
    assert tuple(norms.shape) == (P,)
    for s in range(P):
        want = math.sqrt(sum(float(x[s].double().square().sum()) for x in before.values()))
        assert float(norms[s]) == pytest.approx(want, rel=1e-5)
        above = want > max_norm
        assert above == (s in (1, 3)), (s, want)
        for name, x in before.items():
            got = getattr(pol, name).grad[s]
            if above:
                assert torch.allclose(got, x[s] * (max_norm / want), rtol=1e-5, atol=0), (s, name)
            else:
                assert torch.equal(got, x[s]), (s, name)
        after = math.sqrt(sum(float(getattr(pol, name).grad[s].double().square().sum()) for name in before))
        assert after == pytest.approx(min(want, max_norm), rel=1e-5)
    # torch's own clip is over all sets at once: it would have scaled the small sets too
    assert float(torch.sqrt((norms.double() ** 2).sum())) > max_norm
    with pytest.raises(ValueError, match="max_norm"):
        clip_grad_by_set_norm(pol, 0.0)


def test_clip_grad_by_set_norm_counts_a_shared_parameter_in_each_set():
    from sequential_social_dilemma_games_amd.policy import WatershedLSTMPolicy
    pol = WatershedLSTMPolicy(_capi.SSD_WS_SEQ_COMM, cell_size=64, share_comm_layer=True)
    for name, _, _ in pol.layout():
        prm = getattr(pol, name)
        prm.grad = torch.ones_like(prm)
    norms = clip_grad_by_set_norm(pol, 1e9)
    per_set = sum(int(torch.tensor(shape).prod()) for _, shape, _ in pol.layout())       # every entry 1: the norm is sqrt(count)
    assert torch.allclose(norms, torch.full((8,), math.sqrt(per_set)))


def test_package_exports():
    import sequential_social_dilemma_games_amd as pkg
    for name in ("a3c_loss", "a3c_loss_recurrent", "a3c_loss_moa", "clip_grad_by_set_norm"):
        assert callable(getattr(pkg, name)), name
    assert pkg.A3C_STATS == ("total_loss", "policy_loss", "vf_loss", "policy_entropy")
    assert pkg.MOA_A3C_STATS == pkg.A3C_STATS + ("moa_loss",)
    assert set(a3c_ref.VARIANTS) == {"mean", "moa_sum", "vf_no_half", "adv_sign"}
