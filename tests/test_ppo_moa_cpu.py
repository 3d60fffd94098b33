"""ppo_loss_moa without a device: the CPU path against the float64 restatement (ppo_moa_ref.py), where gradient flows and
where it must not (moa_weight = 0, clipped and dead rows, the padding rows of the MOA matrix), the conv's gradient as the sum of
the two branches', minibatch slices, the sixth statistic, the argument checks of the Python entry point and of the ABI, the
scratch query against the header's macro, and whether the GPU tests' bound would notice a kernel with one of the faults this
loss invites, or whose split-K kernels lost or doubled rows of a second chunk."""
import copy
import ctypes as C
import os
import subprocess

import pytest
import torch

from ppo_moa_ref import (ACTIONS_BRANCH, CONV_MARGIN, HYPER, MARGIN, MOA_BRANCH, MOA_WEIGHT, SPLIT_SHAPES, VARIANTS, autograd_loss, bound,
                         branch_report, clipped_rows, forward, make_inputs, make_policy, max_err, moa_ce, rows_mask, set_means, shifted_obs,
                         split_case, stack_saturation)
from ppo_ref import row_terms
from sequential_social_dilemma_games_amd import _capi, ppo_loss_moa
from sequential_social_dilemma_games_amd.policy import MOA_PPO_STATS, PPO_STATS, ConvLSTMPolicy, ConvMOAPolicy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu64(pol, t, first, T, h=HYPER, moa_weight=MOA_WEIGHT):
    """ppo_loss_moa's CPU path on a float64 copy -> (loss, stats, grads)."""
    p = copy.deepcopy(pol).double()
    loss, stats = ppo_loss_moa(p, t, seq_len=T, moa_weight=moa_weight, obs_first=first, **h)
    loss.backward()
    return loss.detach(), stats, {name: getattr(p, name).grad.clone() for name, _, _ in p.layout()}


# (N, P, K, T, E, done mode, kl): P = N and P = 1; N = 2, 5, 11; a ragged last window, T > K, T = 1; done per env, inside a
# window and at a window's end
@pytest.mark.parametrize("N,P,K_,T,mode,kl", [(5, 5, 7, 3, "per_env", True), (5, 1, 4, 8, "mid", False), (2, 2, 6, 1, "none", True),
                                             (11, 11, 5, 5, "window_end", True), (11, 1, 7, 3, "window_end", True),
                                             (2, 1, 5, 2, "mid", True)])
def test_cpu_path_against_restatement(N, P, K_, T, mode, kl):
    h = dict(HYPER, kl_coeff=HYPER["kl_coeff"] if kl else 0.0)
    pol = make_policy(8, N, P, 64, seed=1)
    t, first = make_inputs(pol, K_, 3, N, T, seed=2, behaviour=kl, done_mode=mode)
    loss, stats, g = _cpu64(pol, t, first, T, h)
    loss64, stats64, g64 = autograd_loss(pol, t, h, first, T)
    assert abs(float(loss - loss64)) < 1e-12 * max(1.0, abs(float(loss64)))
    assert tuple(stats) == MOA_PPO_STATS == PPO_STATS + ("moa_loss",)
    for k in MOA_PPO_STATS:
        assert tuple(stats[k].shape) == (P,) and max_err(stats[k], stats64[k]) < 1e-12 * max(1.0, float(stats64[k].abs().max())), k
    for name in g64:
        assert max_err(g[name], g64[name]) < 1e-12 * max(1.0, float(g64[name].abs().max())), name
    # the float32 CPU path agrees with it as float32 does
    l32, _ = ppo_loss_moa(pol, t, seq_len=T, moa_weight=MOA_WEIGHT, obs_first=first, **h)
    assert abs(float(l32.detach()) - float(loss64)) < 1e-4 * max(1.0, abs(float(loss64)))


def test_sixth_statistic_is_moa_loss_per_set():
    """moa_loss of set p is policy.moa_loss(the set's predictions, the actions, weight=1): for P = N the rows of agent p, for
    P = 1 all of them; total_loss carries moa_weight times it."""
    N, K_, T = 5, 5, 2
    for P in (N, 1):
        pol = make_policy(8, N, P, 64, seed=3)
        t, first = make_inputs(pol, K_, 3, N, T, seed=4, done_mode="mid")
        _, stats, _ = _cpu64(pol, t, first, T)
        p = copy.deepcopy(pol).double()
        with torch.no_grad():
            logits, value, pred = forward(p, shifted_obs(t["obs"], first, K_), t["prev_actions"], t["state"], t["done"], T)
            terms = row_terms(logits, value, t["actions"], t["logp_old"].double(), t["advantages"].double(), t["value_targets"].double(),
                              t["vf_pred"].double(), t["behaviour_logits"].double(), HYPER)
            if P == 1:
                want = p.moa_loss(pred, t["actions"], weight=1.0).reshape(1)
            else:                                                # agent i's rows alone: every other agent's predictions masked out
                want = torch.stack([set_means(moa_ce(pred, t["actions"], N, 8), N)[i] for i in range(N)])
                whole = p.moa_loss(pred, t["actions"], weight=1.0)
                assert abs(float(want.mean() - whole)) < 1e-12   # the sets have equal rows: their mean is the policy's own
        assert max_err(stats["moa_loss"], want) < 1e-12
        assert max_err(stats["total_loss"], set_means(terms[0], P) + MOA_WEIGHT * want) < 1e-12


def test_moa_weight_zero_is_the_ppo_gradient():
    """moa_weight = 0: the actions branch and the conv receive exactly the PPO term's gradient, the MOA branch exact zeros."""
    pol = make_policy(8, 5, 5, 64, seed=5)
    t, first = make_inputs(pol, 6, 3, 5, 3, seed=6, done_mode="per_env")
    _, stats, g = _cpu64(pol, t, first, 3, moa_weight=0.0)
    _, _, gp = autograd_loss(pol, t, HYPER, first, 3, branch="ppo")
    for name in MOA_BRANCH:
        assert float(g[name].abs().max()) == 0.0, name
    for name in ACTIONS_BRANCH + ("conv_w", "conv_b"):
        assert max_err(g[name], gp[name]) < 1e-12 and float(gp[name].abs().max()) > 0.0, name
    assert float(stats["moa_loss"].min()) > 0.0


def test_clipped_and_dead_rows_leave_the_moa_branch_alone():
    """Every row clipped and dead, entropy_coeff = kl_coeff = 0, moa_weight > 0: exact zeros on the actions branch, the MOA
    branch's gradient is the cross-entropy's and not zero."""
    T = 3
    pol = make_policy(8, 5, 5, 64, seed=7)
    t, first = make_inputs(pol, 7, 3, 5, T, seed=8, behaviour=False, done_mode="per_env")
    t = dict(t, **clipped_rows(pol, t, first, T))
    h = dict(HYPER, entropy_coeff=0.0, kl_coeff=0.0)
    _, _, g = _cpu64(pol, t, first, T, h)
    _, _, gm = autograd_loss(pol, t, h, first, T, branch="moa")
    for name in ACTIONS_BRANCH:
        assert float(g[name].abs().max()) == 0.0, name
    for name in MOA_BRANCH + ("conv_w", "conv_b"):
        assert float(g[name].abs().max()) > 0.0 and max_err(g[name], gm[name]) < 1e-12, name


@pytest.mark.parametrize("live", [False, True])
def test_clipped_rows_on_both_signs_on_the_reference(live):
    """clipped_rows with a seed, on the float64 reference and the fragment of the GPU tests: every row clipped on both signs of
    the advantage, dead or clipped and live, 0.1 and more from every boundary; with moa_weight = entropy_coeff = kl_coeff = 0
    the dead case's gradient is exactly zero, the live case's is exactly zero in the logits layer and the MOA branch and
    reaches every other tensor."""
    T = 3
    h = dict(HYPER, entropy_coeff=0.0, kl_coeff=0.0)
    pol = make_policy(8, 5, 5, 64, seed=80)
    t, first = make_inputs(pol, 7, 17, 5, T, seed=81, behaviour=False, done_mode="per_env")
    t = dict(t, **clipped_rows(pol, t, first, T, live=live, seed=82))
    rep = branch_report(pol, t, h, first, T)
    assert rep["open_pos"] == 0.0 and rep["open_neg"] == 0.0 and rep["clipped_pos"] > 0.3 and rep["clipped_neg"] > 0.3, rep
    assert rep["margin"] > 0.1 and rep["conv_margin"] >= CONV_MARGIN and rep["vf_clipped_live" if live else "vf_dead"] == 1.0, rep
    _, stats, g = autograd_loss(pol, t, h, first, T, moa_weight=0.0)
    pos = (t["advantages"] > 0).double().reshape(-1, 5).mean(0)
    assert max_err(stats["policy_loss"], -(1.3 * pos) + 0.7 * (1.0 - pos)) < 1e-6
    for name in g:
        zero = not live or name in MOA_BRANCH + ("logits_w", "logits_b")
        assert (float(g[name].abs().max()) == 0.0) == zero, name


def test_conv_gradient_is_the_sum_of_the_branches():
    pol = make_policy(8, 5, 5, 64, seed=9)
    t, first = make_inputs(pol, 7, 3, 5, 3, seed=10, done_mode="mid")
    _, _, g = _cpu64(pol, t, first, 3)
    _, _, gp = autograd_loss(pol, t, HYPER, first, 3, branch="ppo")
    _, _, gm = autograd_loss(pol, t, HYPER, first, 3, branch="moa")
    for name in ("conv_w", "conv_b"):
        assert max_err(g[name], gp[name] + gm[name]) < 1e-12, name
        # both paths are a real share of the conv's gradient
        assert min(float(gp[name].abs().max()), float(gm[name].abs().max())) > 0.05 * float(g[name].abs().max()), name
    for name in MOA_BRANCH:
        assert float(gp[name].abs().max()) == 0.0 and max_err(g[name], gm[name]) < 1e-12, name
    for name in ACTIONS_BRANCH:
        assert float(gm[name].abs().max()) == 0.0 and max_err(g[name], gp[name]) < 1e-12, name


def test_padding_rows_of_the_moa_matrix():
    """The packed MOA matrix has 48 input rows, the parameter 32 + N: rows 32 + N .. 47 belong to no parameter (layout()), so
    nothing of them reaches a gradient; the N action rows do receive one."""
    N, C_ = 5, 64
    pol = make_policy(8, N, N, C_, seed=11)
    t, first = make_inputs(pol, 4, 3, N, 2, seed=12)
    _, _, g = _cpu64(pol, t, first, 2)
    assert tuple(g["moa_kernel"].shape) == (N, 32 + N, 4 * C_)
    assert float(g["moa_kernel"][:, 32:].abs().amax(2).min()) > 0.0
    used = torch.zeros(pol.set_floats, dtype=torch.bool)
    for name, shape, off in pol.layout():
        used[off:off + int(torch.tensor(shape).prod())] = True
    mw = _capi.SSD_MOA_MW(C_, 8)
    assert not bool(used[mw + (32 + N) * 4 * C_:mw + 48 * 4 * C_].any()) and bool(used[mw:mw + (32 + N) * 4 * C_].all())
    assert bool(used[mw + 48 * 4 * C_:mw + (48 + C_) * 4 * C_].all())               # the recurrent rows follow the padding
    assert float(pol.packed().reshape(N, -1)[:, mw + (32 + N) * 4 * C_:mw + 48 * 4 * C_].abs().max()) == 0.0


def test_minibatch_slices_against_the_whole_fragment():
    """Steps k0 .. k1 - 1 (k0 a multiple of T) addressed by slices (prev_actions among them) give the whole fragment's rows."""
    K_, T, N = 8, 3, 5
    pol = make_policy(8, N, N, 64, seed=13)
    t, first = make_inputs(pol, K_, 2, N, T, seed=14, done_mode="per_env")
    p = copy.deepcopy(pol).double()
    lg, v, pr = forward(p, shifted_obs(t["obs"], first, K_), t["prev_actions"], t["state"], t["done"], T)
    for k0, k1 in ((3, 8), (6, 8), (3, 6), (0, 3)):
        mb = {k: x[k0:k1].contiguous() for k, x in t.items() if k != "state"}
        mb["state"] = t["state"][k0 // T:].contiguous()
        loss, stats, g = _cpu64(pol, mb, first if k0 == 0 else t["obs"][k0 - 1], T)
        terms = row_terms(lg[k0:k1], v[k0:k1], mb["actions"], mb["logp_old"].double(), mb["advantages"].double(),
                          mb["value_targets"].double(), mb["vf_pred"].double(), mb["behaviour_logits"].double(), HYPER)
        ref = set_means(terms[0] + MOA_WEIGHT * moa_ce(pr[k0:k1], mb["actions"], N, 8), N).sum()
        assert abs(float(loss - ref)) < 1e-11, (k0, k1)
        grads = torch.autograd.grad(ref, [getattr(p, name) for name, _, _ in p.layout()], retain_graph=True)
        for (name, _, _), gr in zip(p.layout(), grads):
            assert max_err(g[name], gr) < 1e-12 * max(1.0, float(gr.abs().max())), (k0, k1, name)


def test_python_argument_checks():
    pol = make_policy(8, 5, 5, 64, seed=0)
    t, first = make_inputs(pol, 4, 2, 5, 2, seed=0, done_mode="mid")
    call = lambda b, T=2, pol=pol, mw=MOA_WEIGHT, **kw: ppo_loss_moa(pol, b, seq_len=T, moa_weight=mw, obs_first=first,   # noqa: E731
                                                                     **dict(HYPER, **kw))
    call(t)
    with pytest.raises(ValueError, match="ConvMOAPolicy"):
        call(t, pol=ConvLSTMPolicy(8, 5, 64))
    with pytest.raises(ValueError, match="agents"):
        call(t, pol=ConvMOAPolicy(8, 4, 1, 64))
    with pytest.raises(ValueError, match="seq_len"):
        call(t, T=0)
    with pytest.raises(ValueError, match="moa_weight"):
        call(t, mw=-1.0)
    with pytest.raises(ValueError, match="finite"):
        call(t, mw=float("nan"))
    with pytest.raises(ValueError, match="state"):
        call({k: v for k, v in t.items() if k != "state"})
    with pytest.raises(ValueError, match="state"):
        call(dict(t, state=t["state"][:1]))                       # S = ceil(4 / 2) = 2
    with pytest.raises(ValueError, match="state"):
        call(dict(t, state=t["state"][:, :, :, :2].contiguous()))  # a two-row state is the recurrent policy's
    with pytest.raises(ValueError, match="state"):
        call(dict(t, state=t["state"].double()))
    with pytest.raises(ValueError, match="cells"):
        call(dict(t, state=torch.zeros((2, 2, 5, 4, 128))))
    with pytest.raises(ValueError, match="prev_actions"):
        call({k: v for k, v in t.items() if k != "prev_actions"})
    with pytest.raises(ValueError, match="prev_actions"):
        call(dict(t, prev_actions=t["prev_actions"].long()))
    with pytest.raises(ValueError, match="prev_actions"):
        call(dict(t, prev_actions=t["prev_actions"][:3]))
    with pytest.raises(ValueError, match="done"):
        call(dict(t, done=t["done"].bool()))
    with pytest.raises(ValueError, match="behaviour_logits"):
        call({k: v for k, v in t.items() if k != "behaviour_logits"})
    with pytest.raises(ValueError, match="actions"):
        call(dict(t, actions=t["actions"].long()))
    with pytest.raises(ValueError, match="finite"):
        call(t, clip_param=float("inf"))
    with pytest.raises(ValueError, match="dict"):
        call((t["obs"], t["actions"]))
    one = {k: v for k, v in t.items() if k != "state"}
    a, _ = call(dict(one, state_in=t["state"][0].contiguous()), T=4)
    b, _ = call(dict(one, state=t["state"][:1].contiguous()), T=9)
    assert torch.equal(a, b)
    renamed = {{"logp_old": "logp", "vf_pred": "value", "behaviour_logits": "logits"}.get(k, k): v for k, v in t.items()}
    assert torch.equal(call(renamed)[0], call(t)[0])


def test_abi_argument_checks_need_no_device():
    """ssd_policy_moa_ppo_grad is exported and refuses bad arguments before anything is launched, with the reason in
    ssd_policy_last_error (lower case)."""
    L = _capi.lib()
    assert "ssd_policy_moa_ppo_grad" in _capi.SYMBOLS and _capi.MOA_PPO_SYMBOLS == ("ssd_policy_moa_ppo_grad",)
    w = (C.c_float * 16)()
    buf = (C.c_double * 16)()
    p = lambda x: C.cast(x, C.c_void_p)   # noqa: E731

    def call(weights=w, P=5, A=8, cell=64, T=3, obs_first=None, obs=buf, state=buf, prev=buf, done=None, actions=buf, logp_old=buf, adv=buf,
             vt=buf, vfp=buf, beh=None, K=2, E=3, N=5, hyper=(0.3, 1.0, 0.5, 0.01, 0.0, 10.0), scratch=buf, grads=buf, stats=buf, flags=0):
        q = lambda x: None if x is None else (x if isinstance(x, C.c_void_p) else p(x))   # noqa: E731
        rc = L.ssd_policy_moa_ppo_grad(q(weights), P, A, cell, T, q(obs_first), q(obs), q(state), q(prev), q(done), q(actions), q(logp_old),
                                       q(adv), q(vt), q(vfp), q(beh), K, E, N, *hyper, q(scratch), q(grads), q(stats), 0, flags, None)
        return rc, L.ssd_policy_last_error().decode()

    odd = lambda k: C.cast(C.addressof(buf) + k, C.c_void_p)   # noqa: E731
    for kw, why in ((dict(weights=None), "weights"), (dict(P=2), "num_sets"), (dict(A=16), "num_actions"), (dict(N=1, P=1), "agents"),
                    (dict(N=17, P=17), "agents"), (dict(cell=100), "cell_size"), (dict(T=0), "seq_len"),
                    (dict(state=None), "state"), (dict(state=odd(2)), "aligned"), (dict(prev=None), "prev_actions"),
                    (dict(prev=odd(2)), "aligned"), (dict(scratch=odd(4)), "aligned"),
                    (dict(stats=odd(4)), "aligned"), (dict(grads=odd(2)), "aligned"), (dict(weights=odd(2)), "aligned"),
                    (dict(K=0), "n_steps"), (dict(E=0), "num_envs"), (dict(K=2 ** 20, E=2 ** 11), "2^31"), (dict(obs=None), "obs"),
                    (dict(obs=None, obs_first=buf), "obs"), (dict(actions=None), "actions"), (dict(vfp=None), "vf_preds"),
                    (dict(scratch=None), "scratch"), (dict(stats=None), "stats"),
                    (dict(hyper=(float("nan"), 1.0, 0.5, 0.01, 0.0, 10.0)), "finite"), (dict(hyper=(-0.1, 1.0, 0.5, 0.01, 0.0, 10.0)), "clip_param"),
                    (dict(hyper=(0.3, 1.0, 0.5, 0.01, 0.0, -1.0)), "moa_weight"), (dict(hyper=(0.3, 1.0, 0.5, 0.01, 0.0, float("inf"))), "moa_weight"),
                    (dict(hyper=(0.3, 1.0, 0.5, 0.01, 0.2, 10.0)), "behaviour_logits"), (dict(beh=buf), "behaviour_logits"),
                    (dict(flags=1), "flags")):
        rc, msg = call(**kw)
        assert rc == _capi.SSD_E_INVALID, (kw, rc, msg)
        assert why in msg and msg.replace("MOA", "moa") == msg.lower(), (kw, msg)
    if not torch.cuda.is_available():                          # good arguments get as far as the device
        rc, msg = call()
        assert rc in (_capi.SSD_E_INVALID, _capi.SSD_E_DEVICE) and "device" in msg.lower(), (rc, msg)


# (K, E, N, P, A, C, T)
SHAPES = [(1, 1, 5, 5, 8, 64, 1), (7, 33, 5, 5, 8, 64, 3), (4, 17, 5, 1, 15, 128, 8), (128, 4096, 5, 5, 8, 128, 16), (16, 4096, 5, 5, 8, 128, 16),
          (2, 1025, 16, 16, 8, 64, 2), (3, 16, 5, 5, 9, 256, 3), (6, 1000, 3, 1, 1, 64, 1), (7, 17, 16, 16, 15, 64, 3), (7, 17, 2, 2, 8, 64, 3),
          (14, 33, 5, 1, 8, 64, 13), (33, 65, 2, 2, 8, 64, 32), (14, 33, 5, 1, 8, 128, 13)]   # the last three: the split-K shapes A and B


def test_scratch_query_matches_the_header(tmp_path):
    """ConvMOAPolicy.ppo_scratch_shape and _capi's functions are the header's macros (evaluated by the C compiler); the scratch
    does not grow with K beyond one window."""
    src = tmp_path / "q.c"
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <stdint.h>", '#include "ssd.h"', "int main(void) {"]
    for K_, E, N, P, A, Cc, T in SHAPES:
        lines.append('printf("%%zu %%d %%d %%d\\n", (size_t)SSD_MPPO_SCRATCH_FLOATS(%d, %d, %d, %d, %d, %d, %d), '
                     "(int)SSD_MPPO_GROUPS(SSD_RPPO_SEQS(%d, %d, %d), %d), (int)SSD_MPPO_SPLITS((int64_t)%d * %d), (int)SSD_MPPO_PRED_PITCH(%d, %d));"
                     % (K_, E, N, P, A, Cc, T, E, N, P, P, min(T, K_), E * N // P, A, N))
    lines += ['printf("%d %d %d\\n", (int)SSD_MPPO_TILE, (int)SSD_MPPO_CHUNK, (int)SSD_MPPO_MAX_SPLITS);', "return 0; }"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "q"
    subprocess.run(["cc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
    for (K_, E, N, P, A, Cc, T), line in zip(SHAPES, out):
        floats, groups, splits, pitch = (int(x) for x in line.split())
        assert ConvMOAPolicy(A, N, P, Cc).ppo_scratch_shape(K_, E, N, T) == (floats,), (K_, E, N, P, A, Cc, T)
        assert _capi.SSD_MPPO_GROUPS(E * N // P, P) == groups and _capi.SSD_MPPO_SPLITS(min(T, K_) * (E * N // P)) == splits
        assert _capi.SSD_MPPO_PRED_PITCH(A, N) == pitch
    assert [int(x) for x in out[len(SHAPES)].split()] == [_capi.SSD_MPPO_TILE, _capi.SSD_MPPO_CHUNK, _capi.SSD_MPPO_MAX_SPLITS]
    pol = ConvMOAPolicy(8, 5, 5, 128)
    assert pol.ppo_scratch_shape(16, 4096, 5, 16) == pol.ppo_scratch_shape(128, 4096, 5, 16) == pol.ppo_scratch_shape(10 ** 4, 4096, 5, 16)
    assert _capi.SSD_MPPO_GROUPS(1025, 16) == 64 and _capi.SSD_MPPO_GROUPS(17, 5) == 2 and _capi.SSD_MPPO_GROUPS(10 ** 6, 1) == 1024


# ---- would the bound notice? ----
# The GPU accuracy cases' own inputs (test_ppo_moa_gpu.py's CASES: (K, T, E, N, A, done mode, seed)) in float64, et from the
# CPU's float32 autograd.  Each wrong "kernel" must exceed the bound of at least one tensor by a factor of 10 or more.
DEFECTS = {  # variant -> (case, the tensors of which at least one must show it)
    "index_inputs": ((7, 3, 17, 11, 8, "none", 12), ("moa_kernel",)),
    "index_targets": ((7, 3, 17, 11, 8, "none", 12), ("pred_w", "pred_b")),
    "no_stack1_conv": ((7, 3, 17, 5, 8, "per_env", 22), ("conv_w", "conv_b")),
    "cut_moa": ((7, 3, 17, 5, 8, "per_env", 22), ("moa_recurrent", "moa_kernel", "m_fc1_w")),
    "ignore_done_moa": ((7, 3, 17, 5, 8, "per_env", 22), ("moa_recurrent", "moa_kernel", "pred_w")),
    "prev_not_zeroed": ((7, 3, 17, 5, 8, "per_env", 22), ("moa_kernel",)),
    "ce_over_n": ((7, 3, 17, 5, 8, "per_env", 22), ("pred_b", "pred_w")),
    "no_moa_weight": ((7, 3, 17, 5, 8, "per_env", 22), ("pred_b", "pred_w")),
    "drop_last": ((7, 3, 17, 5, 8, "per_env", 22), ("pred_w", "logits_w", "conv_w")),
}
assert set(DEFECTS) == set(VARIANTS)
_CACHE = {}


def _case(K_, T, E, N, A, mode, seed):
    """The case's policy, inputs and float64 / float32 gradients, computed once and shared (never modified)."""
    key = (K_, T, E, N, A, mode, seed)
    if key not in _CACHE:
        pol = make_policy(A, N, N, 64, seed=seed)
        t, first = make_inputs(pol, K_, E, N, T, seed=100 + seed, done_mode=mode)
        rep = branch_report(pol, t, HYPER, first, T)
        assert rep["margin"] > MARGIN and rep["conv_margin"] >= CONV_MARGIN, rep
        _, _, g64 = autograd_loss(pol, t, HYPER, first, T)
        _, _, g32 = autograd_loss(pol, t, HYPER, first, T, dtype=torch.float32)
        _CACHE[key] = (pol, t, first, g64, {name: bound(g64[name], max_err(g32[name], g64[name])) for name in g64})
    return _CACHE[key]


@pytest.mark.parametrize("variant", VARIANTS)
def test_bound_separates_the_gradient_from_a_defect(variant):
    """A condition on the inputs, not a measurement of the kernel: in float64, the gradient of a "kernel" with the fault
    differs from the true one by at least 10 times the bound in one of the named tensors.  DESIGN.md section 18 records the
    factors."""
    case, names = DEFECTS[variant]
    pol, t, first, g64, bounds = _case(*case)
    if variant == "prev_not_zeroed":
        # the inputs hold zero where a done row precedes, as a rollout's ring does, and the fault would not show; the contract
        # selects that zero whatever the ring holds, so the same case with something else there has the same gradient
        reset = torch.zeros_like(t["done"])
        reset[1:] = t["done"][:-1]
        reset[::case[1]] = 0                                     # a window's first step reads the ring as stored
        dirty = torch.where(reset.bool(), 1 + t["actions"] % 7, t["prev_actions"]).contiguous()
        assert not torch.equal(dirty, t["prev_actions"])
        t = dict(t, prev_actions=dirty)
        _, _, again = autograd_loss(pol, t, HYPER, first, case[1])
        assert all(torch.equal(again[name], g64[name]) for name in g64)
    _, _, gv = autograd_loss(pol, t, HYPER, first, case[1], variant=variant)
    ratios = {name: max_err(gv[name], g64[name]) / bounds[name] for name in g64}
    for name in names:
        print("%-16s %-14s off / bound %.1f" % (variant, name, ratios[name]))
    assert max(ratios[name] for name in names) >= 10.0, (variant, {n: ratios[n] for n in names})


@pytest.mark.parametrize("case", [(7, 3, 17, 5, 8, "per_env", 22), (7, 3, 17, 11, 8, "none", 12)])
def test_no_tensor_compares_against_nothing(case):
    """Any single parameter tensor returned as zero exceeds its bound by 10 or more: no gradient of the cases is so small
    that its comparison is empty.  The stacks' tanh stay out of saturation."""
    pol, t, first, g64, bounds = _case(*case)
    for name in g64:
        ratio = float(g64[name].abs().max()) / bounds[name]
        print("zeroed %-14s |grad| / bound %.1f" % (name, ratio))
        assert ratio >= 10.0, (name, ratio)
    assert stack_saturation(pol, t["obs"]) < 0.01


# ---- would the bound notice a row lost or doubled in the split-K kernels' second pass? ----
# what ssd_bptt_dw_kernel (once per branch) and ssd_moa_dpred_kernel write
SPLIT_TENSORS = ("lstm_kernel", "lstm_recurrent", "lstm_bias", "moa_kernel", "moa_recurrent", "moa_bias", "pred_w", "pred_b")
SPLIT_PROBES = ("second_chunks", "last_of_first_pass", "first_of_second_pass", "last_of_ragged_chunk", "window2_first", "window2_last")
BRANCHES = ("clipped_pos", "clipped_neg", "open_pos", "open_neg", "vf_dead", "vf_live", "vf_clipped_live")
_SPLIT_CACHE = {}


def _split_case(shape):
    """The GPU split case's own policy and (ordinary) inputs with the float64 gradient and each tensor's bound (et from the
    CPU's float32), computed once and shared (never modified)."""
    if shape not in _SPLIT_CACHE:
        splits = _capi.SSD_MPPO_MAX_SPLITS
        pol, t, first, (K_, T, E, N, P), probes = split_case(shape, 64, splits, _capi.SSD_MPPO_CHUNK)
        assert _capi.SSD_MPPO_SPLITS(T * (E * N // P)) == splits == 32
        rep = branch_report(pol, t, HYPER, first, T)
        print("split", shape, rep)
        assert rep["margin"] > MARGIN and rep["conv_margin"] >= CONV_MARGIN, rep
        assert all(rep[k] > 0.2 for k in BRANCHES), rep
        _, _, g64 = autograd_loss(pol, t, HYPER, first, T)
        _, _, g32 = autograd_loss(pol, t, HYPER, first, T, dtype=torch.float32)
        bounds = {name: bound(g64[name], max_err(g32[name], g64[name])) for name in g64}
        _SPLIT_CACHE[shape] = (pol, t, first, (K_, T, E, N, P), g64, bounds, probes)
    return _SPLIT_CACHE[shape]


@pytest.mark.parametrize("probe", SPLIT_PROBES)
@pytest.mark.parametrize("shape", sorted(SPLIT_SHAPES))
def test_bound_separates_a_row_of_a_second_chunk(shape, probe):
    """A condition on the inputs of the GPU split cases, not a measurement of the kernel: in float64, losing or doubling the
    probed window set rows -- all rows of the second chunks, the last row of split 31's only chunk, the first row of split 0's
    second, the last valid row of the ragged chunk, the first and the last row of the second window -- moves every tensor the
    split-K kernels write by at least 10 times the bound.  The shares come from a twin of the policy (ppo_moa_ref.forward).  At
    P = N the last set is probed, which a kernel that dropped `+ p` from the row would get wrong; the whole chunks also in
    set 0."""
    pol, t, first, (K_, T, E, N, P), g64, bounds, probes = _split_case(shape)
    window, rng = probes[probe]
    for p in sorted({P - 1, 0} if probe == "second_chunks" else {P - 1}):
        _, _, g = autograd_loss(pol, t, HYPER, first, T, twin_rows=rows_mask(K_, T, E, N, P, [(window, p, rng)]))
        for name in SPLIT_TENSORS:
            rest, share = g[name]
            assert max_err(rest + share, g64[name]) <= 1e-12 * max(1.0, float(g64[name].abs().max())), name
            ratios = (max_err(rest, g64[name]) / bounds[name], max_err(rest + 2 * share, g64[name]) / bounds[name])
            print("%s %-22s set %d %-14s dropped / bound %.1f  twice / bound %.1f" % (shape, probe, p, name, *ratios))
            assert min(ratios) >= 10.0, (shape, probe, p, name, ratios)
