"""ppo_loss without a device: the CPU path against the float64 restatement (ppo_ref.py), the restatement's autograd against the
contract's explicit derivatives, a case worked by hand, every clip branch, the first-epoch tie, the observation shift and
minibatch slices against an explicit torch.cat, both weight-set modes, the C ABI's argument checks, and that the GPU tests'
acceptance bound tells the right gradient from one that lost a row or a tile."""
import ctypes as C
import math

import pytest
import torch

from ppo_ref import (HYPER, MARGIN, autograd_loss, branch_report, kink_loss, make_inputs, make_policy, max_err, row_terms,
                     skipped_rows_error)
from sequential_social_dilemma_games_amd import _capi, ppo_loss
from sequential_social_dilemma_games_amd.policy import PPO_STATS, ConvLSTMPolicy


def _params(policy):
    return [name for name, _, _ in policy.layout()]


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("kl", [0.2, 0.0])
def test_cpu_path_against_restatement(P, kl):
    """The float32 CPU path agrees with the float64 restatement to float32 rounding, and the restatement's autograd with the
    explicit kink formula to float64 rounding (no row is on a boundary)."""
    h = dict(HYPER, kl_coeff=kl)
    pol = make_policy(8, P, seed=3)
    t, first = make_inputs(pol, 6, 8, 5, seed=11)
    rep = branch_report(pol, t, h, first)
    assert rep["margin"] > MARGIN, rep
    loss64, stats64, g64 = autograd_loss(pol, t, h, first)
    lossk, statsk, gk = kink_loss(pol, t, h, first)
    assert abs(float(loss64 - lossk)) < 1e-12
    for name in _params(pol):
        assert max_err(g64[name], gk[name]) <= 1e-12 * max(1.0, float(g64[name].abs().max())), name
    pol.zero_grad()
    loss, stats = ppo_loss(pol, t, obs_first=first, **h)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    loss.backward()
    loss = loss.detach()
    assert abs(float(loss) - float(loss64)) < 1e-4 * max(1.0, abs(float(loss64)))
    assert set(stats) == set(PPO_STATS)
    for k in PPO_STATS:
        assert tuple(stats[k].shape) == (P,)
        assert max_err(stats[k], stats64[k]) < 1e-4 * max(1.0, float(stats64[k].abs().max())), k
    assert abs(float(stats["total_loss"].sum()) - float(loss)) < 1e-5 * max(1.0, abs(float(loss)))
    for name in _params(pol):
        ref = g64[name]
        assert max_err(getattr(pol, name).grad, ref) < 2e-4 * max(1.0, float(ref.abs().max())), name
    if kl == 0.0:
        assert float(stats["kl"].abs().max()) == 0.0


def test_two_rows_by_hand():
    """Two rows with known logits and value: the per-row terms against numbers worked by hand."""
    h = dict(clip_param=0.2, vf_clip_param=0.5, vf_loss_coeff=2.0, entropy_coeff=0.1, kl_coeff=0.5)
    ln2, ln4 = math.log(2.0), math.log(4.0)
    logits = torch.tensor([[0.0, 0.0], [ln4, 0.0]], dtype=torch.float64)          # p = (1/2, 1/2) and (4/5, 1/5)
    value = torch.tensor([1.0, 3.0], dtype=torch.float64)
    actions = torch.tensor([1, 0], dtype=torch.int32)
    logp_old = torch.tensor([-ln2 - math.log(1.5), math.log(0.8)], dtype=torch.float64)   # ratio 1.5 (clipped) and 1
    adv = torch.tensor([2.0, -1.0], dtype=torch.float64)
    vt = torch.tensor([0.0, 1.0], dtype=torch.float64)
    vf_pred = torch.tensor([1.25, 1.0], dtype=torch.float64)                    # |dv| = 0.25 (open) and 2 (clipped to 0.5)
    beh = torch.tensor([[ln4, 0.0], [ln4, 0.0]], dtype=torch.float64)
    row, pl, vf, kl, ent, ratio = row_terms(logits, value, actions, logp_old, adv, vt, vf_pred, beh, h)
    assert torch.allclose(ratio, torch.tensor([1.5, 1.0], dtype=torch.float64), atol=1e-12)
    # row 0: surr = min(2 * 1.5, 2 * 1.2) = 2.4; row 1: surr = -1
    assert torch.allclose(pl, torch.tensor([-2.4, 1.0], dtype=torch.float64), atol=1e-12)
    # row 0: vf1 = vf2 = 1; row 1: vf1 = 4, vf2 = (1 + 0.5 - 1)^2 = 0.25
    assert torch.allclose(vf, torch.tensor([1.0, 4.0], dtype=torch.float64), atol=1e-12)
    ent1 = -(0.8 * math.log(0.8) + 0.2 * math.log(0.2))
    assert torch.allclose(ent, torch.tensor([ln2, ent1], dtype=torch.float64), atol=1e-12)
    kl0 = 0.8 * math.log(0.8 / 0.5) + 0.2 * math.log(0.2 / 0.5)
    assert torch.allclose(kl, torch.tensor([kl0, 0.0], dtype=torch.float64), atol=1e-12)
    want = torch.tensor([-2.4 + 0.5 * kl0 + 2.0 * 1.0 - 0.1 * ln2, 1.0 + 2.0 * 4.0 - 0.1 * ent1], dtype=torch.float64)
    assert torch.allclose(row, want, atol=1e-12)


def test_every_clip_branch_is_exercised():
    """The inputs the tests use put a real share of the rows into each surrogate case and vf branch, and the gradient is what
    the branch says: zero through the ratio where the clipped branch is the minimum, zero through the value where vf2 wins."""
    pol = make_policy(8, 1, seed=5)
    t, first = make_inputs(pol, 8, 16, 4, seed=2)
    rep = branch_report(pol, t, HYPER, first)
    for k in ("clipped_pos", "clipped_neg", "open_pos", "open_neg", "vf_dead", "vf_live", "vf_clipped_live"):
        assert rep[k] > 0.05, rep
    assert rep["margin"] > MARGIN, rep
    # rows whose ratio lies above 1 + c with adv > 0 (or below 1 - c with adv < 0) and whose vf is dead pull nothing
    h = dict(HYPER, entropy_coeff=0.0, kl_coeff=0.0)
    t2 = dict(t)
    K, E, N = t["actions"].shape
    with torch.no_grad():
        import copy
        logits, value = copy.deepcopy(pol).double()(torch.cat([first.unsqueeze(0), t["obs"][:-1]]))
        logp = torch.log_softmax(logits, -1).gather(-1, t["actions"].long().unsqueeze(-1)).squeeze(-1)
    t2["advantages"] = torch.ones((K, E, N))
    t2["logp_old"] = (logp - math.log(1.5)).float()              # ratio 1.5, adv 1: the clipped branch is the minimum
    t2["vf_pred"] = (value + 2.0).float()                         # value - vf_pred = -2: clipped to -1
    t2["value_targets"] = (value + 3.0).float()                   # vf1 = 9, vf2 = (vf_pred - 1 - vt)^2 = 4: vf1 wins, live
    _, _, g = autograd_loss(pol, t2, h, first)
    assert float(g["logits_w"].abs().max()) == 0.0 and float(g["value_w"].abs().max()) > 0.0
    t2["value_targets"] = (value + 0.2).float()                   # vf1 = 0.04, vf2 = (2 - 1 - 0.2)^2 = 0.64: vf2 wins, dead
    _, _, g = autograd_loss(pol, t2, h, first)
    for name in _params(pol):
        assert float(g[name].abs().max()) == 0.0, name
    pol.zero_grad()
    loss, _ = ppo_loss(pol, t2, obs_first=first, **h)
    loss.backward()
    for name in _params(pol):
        assert float(getattr(pol, name).grad.abs().max()) == 0.0, name


@pytest.mark.parametrize("P", [1, 4])
def test_first_epoch_tie_gives_the_unclipped_gradient(P):
    """logp_old and vf_pred from the same weights: ratio = 1, value = vf_pred, both branches of min and max tie.  The gradient
    is the unclipped one -- that of -adv * ratio + vf_coeff * (value - vt)^2 --, not zero and not half of it."""
    h = dict(HYPER, kl_coeff=0.0)
    pol = make_policy(8, P, seed=7)
    t, first = make_inputs(pol, 4, 6, 4, seed=9, behaviour=False, on_policy=True)
    with torch.no_grad():
        logits, value = pol(torch.cat([first.unsqueeze(0), t["obs"][:-1]]))     # the float32 policy's own outputs: exact ties
        t["logp_old"] = torch.log_softmax(logits, -1).gather(-1, t["actions"].long().unsqueeze(-1)).squeeze(-1).contiguous()
        t["vf_pred"] = value.contiguous()
    pol.zero_grad()
    loss, stats = ppo_loss(pol, t, obs_first=first, **h)
    loss.backward()
    got = {name: getattr(pol, name).grad.clone() for name in _params(pol)}
    huge = dict(h, clip_param=1e6, vf_clip_param=1e6)             # no clipping anywhere: the unclipped loss
    _, _, want = autograd_loss(pol, t, huge, first)
    _, _, kink = kink_loss(pol, t, h, first)
    for name in _params(pol):
        scale = max(1.0, float(want[name].abs().max()))
        assert float(want[name].abs().max()) > 0.0
        assert max_err(got[name], want[name]) < 2e-4 * scale, name
        assert max_err(kink[name], want[name]) < 1e-6 * scale, name


def test_obs_shift_and_minibatch_slices():
    """obs_first shifts by address, not by value: the same loss as the explicit torch.cat without obs_first, and a step-range
    minibatch is the leading-axis slices with obs_first = obs[k0 - 1]."""
    h = HYPER
    pol = make_policy(9, 3, seed=1)
    t, first = make_inputs(pol, 7, 4, 3, seed=4)
    K = 7
    cat = torch.cat([first.unsqueeze(0), t["obs"][:-1]]).contiguous()
    a, sa = ppo_loss(pol, t, obs_first=first, **h)
    b, sb = ppo_loss(pol, dict(t, obs=cat), **h)
    assert float(a) == float(b)
    for k in PPO_STATS:
        assert torch.equal(sa[k], sb[k])
    k0, k1 = 2, 6
    mb = {k: v[k0:k1] for k, v in t.items()}
    c, _ = ppo_loss(pol, mb, obs_first=t["obs"][k0 - 1], **h)
    d, _ = ppo_loss(pol, dict(mb, obs=cat[k0:k1]), **h)
    assert float(c) == float(d)
    e, _ = ppo_loss(pol, {k: v[0:3] for k, v in t.items()}, obs_first=first, **h)
    f, _ = ppo_loss(pol, {k: (cat if k == "obs" else v)[0:3] for k, v in t.items()}, **h)
    assert float(e) == float(f)
    # the dict sample() returns: logp, value and logits under their rollout names; a tuple in contract order
    named = {"obs": t["obs"], "actions": t["actions"], "logp": t["logp_old"], "value": t["vf_pred"], "logits": t["behaviour_logits"],
             "advantages": t["advantages"], "value_targets": t["value_targets"], "rew": None, "done": None}
    g, _ = ppo_loss(pol, named, obs_first=first, **h)
    tup = (t["obs"], t["actions"], t["logp_old"], t["advantages"], t["value_targets"], t["vf_pred"], t["behaviour_logits"])
    i, _ = ppo_loss(pol, tup, obs_first=first, **h)
    assert float(g) == float(a) == float(i)
    assert K == t["actions"].shape[0]


def test_python_argument_checks():
    pol = make_policy(8, 5, seed=0)
    t, first = make_inputs(pol, 2, 2, 5, seed=0)
    with pytest.raises(ValueError, match="behaviour_logits"):
        ppo_loss(pol, {k: v for k, v in t.items() if k != "behaviour_logits"}, obs_first=first, **HYPER)
    with pytest.raises(ValueError, match="weight sets"):
        ppo_loss(make_policy(8, 3, seed=0), t, obs_first=first, **HYPER)
    with pytest.raises(ValueError, match="actions"):
        ppo_loss(pol, dict(t, actions=t["actions"].long()), obs_first=first, **HYPER)
    with pytest.raises(ValueError, match="obs"):
        ppo_loss(pol, dict(t, obs=t["obs"][:1]), **HYPER)
    with pytest.raises(ValueError, match="finite"):
        ppo_loss(pol, t, obs_first=first, **dict(HYPER, clip_param=float("nan")))
    with pytest.raises(ValueError, match="ConvFCPolicy"):
        ppo_loss(ConvLSTMPolicy(8, 5, 64), t, obs_first=first, **HYPER)
    # without kl_coeff the behaviour logits are not needed and not read
    ppo_loss(pol, {k: v for k, v in t.items() if k != "behaviour_logits"}, obs_first=first, **dict(HYPER, kl_coeff=0.0))


def test_abi_argument_checks_need_no_device():
    """ssd_policy_ppo_grad is exported and refuses bad arguments before anything is launched, with the reason in
    ssd_policy_last_error (lower-case argument names)."""
    L = _capi.lib()
    assert "ssd_policy_ppo_grad" in _capi.SYMBOLS and hasattr(L, "ssd_policy_ppo_grad")
    A, N = 8, 5
    w = (C.c_float * 16)()
    buf = (C.c_double * 16)()
    p = lambda x: C.cast(x, C.c_void_p)   # noqa: E731

    def call(weights=w, P=N, A=A, obs_first=None, obs=buf, actions=buf, logp_old=buf, adv=buf, vt=buf, vfp=buf, beh=None, K=2, E=3,
             N=N, hyper=(0.3, 1.0, 0.5, 0.01, 0.0), scratch=buf, grads=buf, stats=buf, flags=0):
        q = lambda x: None if x is None else p(x)   # noqa: E731
        rc = L.ssd_policy_ppo_grad(q(weights), P, A, q(obs_first), q(obs), q(actions), q(logp_old), q(adv), q(vt), q(vfp), q(beh),
                                   K, E, N, *hyper, q(scratch), q(grads), q(stats), 0, flags, None)
        return rc, L.ssd_policy_last_error().decode()

    for kw, why in ((dict(weights=None), "weights"), (dict(P=2), "num_sets"), (dict(A=16), "num_actions"), (dict(N=0, P=1), "num_agents"),
                    (dict(K=0), "n_steps"), (dict(E=0), "num_envs"), (dict(K=2 ** 20, E=2 ** 11), "2^31"), (dict(K=2 ** 31 - 16, E=1, N=1, P=1), "2^31"), (dict(obs=None), "obs"),
                    (dict(obs=None, obs_first=buf), "obs"), (dict(actions=None), "actions"), (dict(vfp=None), "vf_preds"),
                    (dict(scratch=None), "scratch"), (dict(stats=None), "stats"),
                    (dict(hyper=(float("nan"), 1.0, 0.5, 0.01, 0.0)), "finite"), (dict(hyper=(-0.1, 1.0, 0.5, 0.01, 0.0)), "clip_param"),
                    (dict(hyper=(0.3, 1.0, 0.5, 0.01, 0.2)), "behaviour_logits"), (dict(beh=buf), "behaviour_logits"),
                    (dict(flags=1), "flags")):
        rc, msg = call(**kw)
        assert rc == _capi.SSD_E_INVALID, (kw, rc, msg)
        assert why in msg and msg == msg.lower(), (kw, msg)
    odd = C.cast(C.addressof(buf) + 4, C.c_void_p)
    rc = L.ssd_policy_ppo_grad(p(w), N, A, None, p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), None, 2, 3, N, 0.3, 1.0, 0.5, 0.01, 0.0,
                               odd, p(buf), p(buf), 0, 0, None)
    assert rc == _capi.SSD_E_INVALID and "aligned" in L.ssd_policy_last_error().decode()
    # good arguments get as far as the device, which a box without one does not have
    if not torch.cuda.is_available():
        rc, msg = call()
        assert rc in (_capi.SSD_E_INVALID, _capi.SSD_E_DEVICE) and "device" in msg.lower(), (rc, msg)
    assert _capi.SSD_PPO_GROUPS(1, 5) == 1 and _capi.SSD_PPO_GROUPS(4096 * 128, 5) == 204 and _capi.SSD_PPO_GROUPS(17, 1) == 2
    assert _capi.SSD_PPO_SCRATCH_FLOATS(17, 1, 8) == 2 * (_capi.SSD_POL_SET_FLOATS(8) + 16)


def test_scratch_query_and_gradient_unpacking():
    """The policy reports the call's scratch, and a packed gradient unpacks by layout(): a parameter with fewer entries than
    sets gets the sum of its sets' gradients (no ConvFCPolicy parameter is shared; a Watershed policy's dense1 can be)."""
    import numpy as np
    from sequential_social_dilemma_games_amd.policy import WatershedLSTMPolicy, unpack_gradient
    pol = make_policy(9, 5, seed=0)
    assert pol.ppo_scratch_shape(4096 * 128) == (5 * 204 * (pol.set_floats + 16),)
    assert pol.ppo_scratch_shape(17) == (_capi.SSD_PPO_SCRATCH_FLOATS(17, 5, 9),) == (5 * 2 * (pol.set_floats + 16),)
    assert make_policy(8, 1, seed=0).ppo_scratch_shape(10 ** 6) == (1024 * (_capi.SSD_POL_SET_FLOATS(8) + 16),)
    g = torch.Generator().manual_seed(3)
    for policy in (pol, WatershedLSTMPolicy(_capi.SSD_WS_SEQ_COMM, cell_size=64, share_comm_layer=True)):
        P, S = policy.num_sets, policy.set_floats
        packed = torch.randn((P, S), generator=g)
        out = dict(zip((name for name, _, _ in policy.layout()), unpack_gradient(policy, packed, 2.0)))
        for name, shape, off in policy.layout():
            n = int(np.prod(shape))
            want = packed[:, off:off + n].reshape((P,) + tuple(shape)) * 2.0
            param = getattr(policy, name)
            if param.shape[0] != P:                              # dense1 of agents k and k + 4 is one layer
                assert (name.startswith("dense1"), param.shape[0], P) == (True, 4, 8)
                want = want[:4] + want[4:]
            assert out[name].shape == param.shape and torch.equal(out[name], want), name
        # ... which is what autograd gives a parameter that packed() repeats into several sets
        w = policy.packed().clone()
        for name, _, _ in policy.layout():
            getattr(policy, name).grad = None
        leaves = [getattr(policy, name) for name, _, _ in policy.layout()]
        P_, S_ = policy.num_sets, policy.set_floats
        rebuilt = torch.zeros((P_, S_))
        for name, shape, off in policy.layout():
            n = int(np.prod(shape))
            t = getattr(policy, name).reshape(-1, n)
            rebuilt[:, off:off + n] = t.repeat(P_ // t.shape[0], 1)
        assert torch.equal(rebuilt.detach().reshape(-1), w)
        (rebuilt * packed).sum().backward()
        for leaf, got in zip(leaves, unpack_gradient(policy, packed)):
            assert torch.allclose(leaf.grad, got, rtol=0, atol=1e-6)


# (A, P, K, E, N, behaviour_logits, seed): multi-iteration cases of tests/test_ppo_loss_gpu.py's CASES (same seeds, so the same
# inputs), P = 1 and P = N
NEAR_MISS_CASES = [(9, 1, 7, 601, 4, False, 16), (9, 1, 3, 1825, 3, True, 20), (8, 5, 8, 513, 5, True, 15), (8, 64, 257, 1, 64, True, 18)]


@pytest.mark.parametrize("A,P,K_,E,N,beh,seed", NEAR_MISS_CASES)
def test_bound_separates_the_gradient_from_a_near_miss(A, P, K_, E, N, beh, seed):
    """The GPU tests accept ek <= 4 et + 1e-6 max(1, max |ref|), and with gradients of 1e-2 the 1e-6 floor is most of it.
    Would that bound notice a kernel whose persistent loop lost rows in its second iteration?  The loss is a mean over a
    set's rows, so such a kernel's gradient is off by exactly grad(the lost rows alone) * lost / rows: one float64 autograd.
    With et from torch's float32 autograd on the CPU (a stand-in for the device's), max |difference| / bound must be
      >= 10 for some tensor when the one row 16 G is lost (the first row of the second iteration),
      >= 5 for every tensor when the ragged last tile is lost,
      >= 10 for every tensor when every tile >= G is lost (the whole second iteration).
    For P = N the rows are lost in every set, as an error in the tiling would lose them (the sets share one tiling), and ek
    is the largest difference over the whole [P, ...] tensor, as the GPU tests form it.  These are conditions on the inputs (a
    seed that misses one is replaced, the ratios stay)."""
    h = dict(HYPER, kl_coeff=HYPER["kl_coeff"] if beh else 0.0)
    pol = make_policy(A, P, seed=seed)
    t, first = make_inputs(pol, K_, E, N, seed=100 + seed, behaviour=beh)
    R = K_ * E * N // P
    G = _capi.SSD_PPO_GROUPS(R, P)
    tiles = (R + 15) // 16
    assert G < tiles <= 2 * G and R > 16 * G                      # the loop runs a second time and no third
    _, _, g64 = autograd_loss(pol, t, h, first)
    _, _, g32 = autograd_loss(pol, t, h, first, dtype=torch.float32)
    bound = {name: 4.0 * max_err(g32[name], g64[name]) + 1e-6 * max(1.0, float(g64[name].abs().max())) for name in g64}
    lost = {"row 16 G": torch.tensor([16 * G]), "ragged last tile": torch.arange(16 * (tiles - 1), R),
            "second iteration": torch.arange(16 * G, R)}
    ratios = {}
    for what, idx in lost.items():
        diff = skipped_rows_error(pol, t, h, first, idx)
        ratios[what] = {name: float(d.abs().max()) / bound[name] for name, d in diff.items()}
        print(what, len(idx), "rows of", R, {name: round(r, 1) for name, r in ratios[what].items()})
    assert max(ratios["row 16 G"].values()) >= 10.0, ratios["row 16 G"]
    assert min(ratios["ragged last tile"].values()) >= 5.0, ratios["ragged last tile"]
    assert min(ratios["second iteration"].values()) >= 10.0, ratios["second iteration"]
