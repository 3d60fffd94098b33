"""ppo_loss_recurrent without a device: the CPU path against the float64 restatement (ppo_lstm_ref.py), the state rule's
properties (T = 1, the truncation, the resets, minibatch slices), the argument checks of the Python entry point and of the ABI,
the scratch query against the header's macro, and whether the GPU tests' bound would notice a kernel that cut BPTT, ignored
done or dropped a ragged last window, or whose split-K kernel lost or doubled rows of a second chunk."""
import copy
import ctypes as C
import os
import subprocess

import pytest
import torch

from ppo_lstm_ref import (HYPER, MARGIN, SPLIT_SHAPES, autograd_loss, bound, branch_report, forward, make_inputs, make_policy,
                          max_err, rows_mask, set_means, shifted_obs, split_case)
from ppo_ref import row_terms
from sequential_social_dilemma_games_amd import _capi, ppo_loss_recurrent
from sequential_social_dilemma_games_amd.policy import PPO_STATS, ConvFCPolicy, recurrent_forward

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu64(pol, t, first, T, h=HYPER):
    """ppo_loss_recurrent's CPU path on a float64 copy -> (loss, stats, grads)."""
    p = copy.deepcopy(pol).double()
    loss, stats = ppo_loss_recurrent(p, t, seq_len=T, obs_first=first, **h)
    loss.backward()
    return loss.detach(), stats, {name: getattr(p, name).grad.clone() for name, _, _ in p.layout()}


@pytest.mark.parametrize("P,K_,T,mode,kl", [(5, 7, 3, "per_env", True), (1, 4, 8, "mid", False), (5, 6, 1, "none", True),
                                           (1, 5, 5, "window_end", True)])
def test_cpu_path_against_restatement(P, K_, T, mode, kl):
    h = dict(HYPER, kl_coeff=HYPER["kl_coeff"] if kl else 0.0)
    pol = make_policy(8, P, 64, seed=1)
    t, first = make_inputs(pol, K_, 3, 5, T, seed=2, behaviour=kl, done_mode=mode)
    loss, stats, g = _cpu64(pol, t, first, T, h)
    loss64, stats64, g64 = autograd_loss(pol, t, h, first, T)
    assert abs(float(loss - loss64)) < 1e-12
    for k in PPO_STATS:
        assert tuple(stats[k].shape) == (P,) and max_err(stats[k], stats64[k]) < 1e-12, k
    for name in g64:
        assert max_err(g[name], g64[name]) < 1e-12, name
    # the float32 CPU path agrees with it as float32 does
    l32, _ = ppo_loss_recurrent(pol, t, seq_len=T, obs_first=first, **h)
    assert abs(float(l32.detach()) - float(loss64)) < 1e-4 * max(1.0, abs(float(loss64)))


def test_seq_len_one_is_a_per_step_forward():
    """T = 1: every step's state comes from the ring, so the loss is that of K independent forward() calls."""
    pol = make_policy(8, 5, 64, seed=3).double()
    t, first = make_inputs(pol, 4, 2, 5, 1, seed=4)
    loss, _, g = _cpu64(pol, t, first, 1)
    twin = copy.deepcopy(pol)
    obs = shifted_obs(t["obs"], first, 4)
    outs = [twin(obs[k], t["state"][k].double(), None) for k in range(4)]
    logits, value = torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
    terms = row_terms(logits, value, t["actions"], t["logp_old"].double(), t["advantages"].double(), t["value_targets"].double(),
                      t["vf_pred"].double(), t["behaviour_logits"].double(), HYPER)
    ref = set_means(terms[0], 5).sum()
    ref.backward()
    assert abs(float(loss - ref)) < 1e-12
    for name in g:
        assert max_err(g[name], getattr(twin, name).grad) < 1e-12, name
    assert float(g["lstm_w"][:, 32:].abs().max()) > 0          # the ring's h is data the gates read


def test_truncation_splits_the_gradient_at_the_window():
    """T = 3, K = 6: no gradient crosses k = 3, so the gradient is the rows-weighted mean of the two windows' own."""
    pol = make_policy(8, 5, 64, seed=5)
    t, first = make_inputs(pol, 6, 2, 5, 3, seed=6)
    _, _, g = _cpu64(pol, t, first, 3)
    a = {k: v[:3].contiguous() for k, v in t.items() if k != "state"}
    b = {k: v[3:].contiguous() for k, v in t.items() if k != "state"}
    _, _, ga = _cpu64(pol, dict(a, state=t["state"][:1]), first, 3)
    _, _, gb = _cpu64(pol, dict(b, state=t["state"][1:].contiguous()), t["obs"][2], 3)
    for name in g:
        assert max_err(g[name], 0.5 * (ga[name] + gb[name])) < 1e-12, name


def test_a_done_row_cuts_values_and_gradient():
    """done[k - 1] makes step k independent of everything before it: rows >= k are unchanged to the bit when earlier
    observations change, and a NaN where the rule does not read (a ring slot past S, done[K - 1]) does not surface."""
    K_, T, E, N = 6, 6, 2, 5
    pol = make_policy(8, N, 64, seed=7)
    t, first = make_inputs(pol, K_, E, N, T, seed=8)
    done = torch.zeros((K_, E, N), dtype=torch.uint8)
    done[2] = 1                                                # step 3 starts from zero
    t = dict(t, done=done)
    obs = shifted_obs(t["obs"], first, K_)
    with torch.no_grad():
        lg, v = recurrent_forward(pol, obs, t["state"], done, T)
        other = obs.clone()
        other[:3] = 255 - other[:3]
        lg2, v2 = recurrent_forward(pol, other, t["state"], done, T)
        lg3, v3 = recurrent_forward(pol, other, t["state"], None, T)
    assert torch.equal(lg[3:], lg2[3:]) and torch.equal(v[3:], v2[3:]) and not torch.equal(lg[:3], lg2[:3])
    assert not torch.equal(lg[3:], lg3[3:])                    # without the flag the past reaches step 3
    loss, stats = ppo_loss_recurrent(pol, t, seq_len=T, obs_first=first, **HYPER)
    ring = torch.cat([t["state"], torch.full_like(t["state"][:1], float("nan"))])
    done2 = done.clone()
    done2[K_ - 1] = 1
    loss2, stats2 = ppo_loss_recurrent(pol, dict(t, state=ring, done=done2), seq_len=T, obs_first=first, **HYPER)
    assert torch.equal(loss, loss2) and bool(torch.isfinite(loss2))
    # the gradient does not cross the done row either: the rows before it do not feel the rows after it
    p = copy.deepcopy(pol).double()
    lg, v = recurrent_forward(p, obs, t["state"], done, T)
    (g,) = torch.autograd.grad(lg[3:].sum() + v[3:].sum(), p.conv_w, retain_graph=True)
    p2 = copy.deepcopy(pol).double()
    lgb, vb = recurrent_forward(p2, obs[3:], torch.zeros_like(t["state"]), None, T)
    (gb,) = torch.autograd.grad(lgb.sum() + vb.sum(), p2.conv_w)
    assert max_err(g, gb) < 1e-12


def test_minibatch_slices_against_the_whole_fragment():
    """Steps k0 .. k1 - 1 (k0 a multiple of T) addressed by slices give the whole fragment's rows k0 .. k1 - 1."""
    K_, T = 8, 3
    pol = make_policy(8, 5, 64, seed=9)
    t, first = make_inputs(pol, K_, 2, 5, T, seed=10, done_mode="per_env")
    p = copy.deepcopy(pol).double()
    lg, v = forward(p, shifted_obs(t["obs"], first, K_), t["state"], t["done"], T)
    for k0, k1 in ((3, 8), (6, 8), (3, 6), (0, 3)):
        mb = {k: x[k0:k1].contiguous() for k, x in t.items() if k != "state"}
        mb["state"] = t["state"][k0 // T:].contiguous()
        loss, stats, g = _cpu64(pol, mb, first if k0 == 0 else t["obs"][k0 - 1], T)
        terms = row_terms(lg[k0:k1], v[k0:k1], mb["actions"], mb["logp_old"].double(), mb["advantages"].double(),
                          mb["value_targets"].double(), mb["vf_pred"].double(), mb["behaviour_logits"].double(), HYPER)
        ref = set_means(terms[0], 5).sum()
        assert abs(float(loss - ref)) < 1e-12, (k0, k1)
        grads = torch.autograd.grad(ref, [getattr(p, name) for name, _, _ in p.layout()], retain_graph=True)
        for (name, _, _), gr in zip(p.layout(), grads):
            assert max_err(g[name], gr) < 1e-12, (k0, k1, name)


def test_python_argument_checks():
    pol = make_policy(8, 5, 64, seed=0)
    t, first = make_inputs(pol, 4, 2, 5, 2, seed=0, done_mode="mid")
    call = lambda b, T=2, pol=pol, **kw: ppo_loss_recurrent(pol, b, seq_len=T, obs_first=first, **dict(HYPER, **kw))   # noqa: E731
    call(t)
    with pytest.raises(ValueError, match="ConvLSTMPolicy"):
        call(t, pol=ConvFCPolicy(8, 5))
    with pytest.raises(ValueError, match="seq_len"):
        call(t, T=0)
    with pytest.raises(ValueError, match="state"):
        call({k: v for k, v in t.items() if k != "state"})
    with pytest.raises(ValueError, match="state"):
        call(dict(t, state=t["state"][:1]))                       # S = ceil(4 / 2) = 2
    with pytest.raises(ValueError, match="state"):
        call(dict(t, state=t["state"].double()))
    with pytest.raises(ValueError, match="state"):
        call(dict(t, state=t["state"].transpose(1, 2)))
    with pytest.raises(ValueError, match="cells"):
        call(dict(t, state=torch.zeros((2, 2, 5, 2, 128))))
    with pytest.raises(ValueError, match="done"):
        call(dict(t, done=t["done"].bool()))
    with pytest.raises(ValueError, match="done"):
        call(dict(t, done=t["done"][:3]))
    with pytest.raises(ValueError, match="behaviour_logits"):
        call({k: v for k, v in t.items() if k != "behaviour_logits"})
    with pytest.raises(ValueError, match="actions"):
        call(dict(t, actions=t["actions"].long()))
    with pytest.raises(ValueError, match="finite"):
        call(t, clip_param=float("inf"))
    with pytest.raises(ValueError, match="dict"):
        call((t["obs"], t["actions"]))
    # state_in serves when one window covers the fragment; the contract names and sample()'s names are both accepted
    one = {k: v for k, v in t.items() if k != "state"}
    a, _ = call(dict(one, state_in=t["state"][0].contiguous()), T=4)
    b, _ = call(dict(one, state=t["state"][:1].contiguous()), T=9)
    assert torch.equal(a, b)
    renamed = {{"logp_old": "logp", "vf_pred": "value", "behaviour_logits": "logits"}.get(k, k): v for k, v in t.items()}
    assert torch.equal(call(renamed)[0], call(t)[0])


def test_abi_argument_checks_need_no_device():
    """ssd_policy_lstm_ppo_grad is exported and refuses bad arguments before anything is launched, with the reason in
    ssd_policy_last_error (lower case)."""
    L = _capi.lib()
    assert "ssd_policy_lstm_ppo_grad" in _capi.SYMBOLS and _capi.LSTM_PPO_SYMBOLS == ("ssd_policy_lstm_ppo_grad",)
    w = (C.c_float * 16)()
    buf = (C.c_double * 16)()
    p = lambda x: C.cast(x, C.c_void_p)   # noqa: E731

    def call(weights=w, P=5, A=8, cell=64, T=3, obs_first=None, obs=buf, state=buf, done=None, actions=buf, logp_old=buf, adv=buf, vt=buf,
             vfp=buf, beh=None, K=2, E=3, N=5, hyper=(0.3, 1.0, 0.5, 0.01, 0.0), scratch=buf, grads=buf, stats=buf, flags=0):
        q = lambda x: None if x is None else (x if isinstance(x, C.c_void_p) else p(x))   # noqa: E731
        rc = L.ssd_policy_lstm_ppo_grad(q(weights), P, A, cell, T, q(obs_first), q(obs), q(state), q(done), q(actions), q(logp_old),
                                        q(adv), q(vt), q(vfp), q(beh), K, E, N, *hyper, q(scratch), q(grads), q(stats), 0, flags, None)
        return rc, L.ssd_policy_last_error().decode()

    odd = lambda k: C.cast(C.addressof(buf) + k, C.c_void_p)   # noqa: E731
    for kw, why in ((dict(weights=None), "weights"), (dict(P=2), "num_sets"), (dict(A=16), "num_actions"), (dict(N=0, P=1), "num_agents"),
                    (dict(cell=100), "cell_size"), (dict(cell=0), "cell_size"), (dict(T=0), "seq_len"), (dict(T=-3), "seq_len"),
                    (dict(state=None), "state"), (dict(state=odd(2)), "aligned"), (dict(scratch=odd(4)), "aligned"),
                    (dict(stats=odd(4)), "aligned"), (dict(grads=odd(2)), "aligned"), (dict(weights=odd(2)), "aligned"),
                    (dict(K=0), "n_steps"), (dict(E=0), "num_envs"), (dict(K=2 ** 20, E=2 ** 11), "2^31"), (dict(obs=None), "obs"),
                    (dict(obs=None, obs_first=buf), "obs"), (dict(actions=None), "actions"), (dict(vfp=None), "vf_preds"),
                    (dict(scratch=None), "scratch"), (dict(stats=None), "stats"),
                    (dict(hyper=(float("nan"), 1.0, 0.5, 0.01, 0.0)), "finite"), (dict(hyper=(-0.1, 1.0, 0.5, 0.01, 0.0)), "clip_param"),
                    (dict(hyper=(0.3, 1.0, 0.5, 0.01, 0.2)), "behaviour_logits"), (dict(beh=buf), "behaviour_logits"),
                    (dict(flags=1), "flags")):
        rc, msg = call(**kw)
        assert rc == _capi.SSD_E_INVALID, (kw, rc, msg)
        assert why in msg and msg == msg.lower(), (kw, msg)
    if not torch.cuda.is_available():                          # good arguments get as far as the device
        rc, msg = call()
        assert rc in (_capi.SSD_E_INVALID, _capi.SSD_E_DEVICE) and "device" in msg.lower(), (rc, msg)


SHAPES = [(1, 1, 5, 5, 8, 64, 1), (7, 33, 5, 5, 8, 64, 3), (4, 17, 5, 1, 15, 128, 8), (128, 4096, 5, 5, 8, 128, 16), (16, 4096, 5, 5, 8, 128, 16),
          (2, 257, 64, 64, 8, 64, 2), (3, 16, 5, 5, 9, 256, 3), (6, 1000, 3, 1, 1, 64, 1),
          (14, 33, 5, 1, 8, 64, 13), (33, 65, 2, 2, 8, 64, 32), (14, 33, 5, 1, 8, 128, 13)]   # the last three: the split-K shapes A and B


def test_scratch_query_matches_the_header(tmp_path):
    """ConvLSTMPolicy.ppo_scratch_shape and _capi's functions are the header's macros (evaluated by the C compiler); the
    scratch does not grow with K beyond one window."""
    src = tmp_path / "q.c"
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <stdint.h>", '#include "ssd.h"', "int main(void) {"]
    for K_, E, N, P, A, Cc, T in SHAPES:
        lines.append('printf("%%zu %%d %%d\\n", (size_t)SSD_RPPO_SCRATCH_FLOATS(%d, %d, %d, %d, %d, %d, %d), '
                     "(int)SSD_RPPO_GROUPS(SSD_RPPO_SEQS(%d, %d, %d), %d), (int)SSD_RPPO_SPLITS((int64_t)%d * %d));"
                     % (K_, E, N, P, A, Cc, T, E, N, P, P, min(T, K_), E * N // P))
    lines += ["return 0; }"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "q"
    subprocess.run(["cc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
    from sequential_social_dilemma_games_amd.policy import ConvLSTMPolicy
    for (K_, E, N, P, A, Cc, T), line in zip(SHAPES, out):
        floats, groups, splits = (int(x) for x in line.split())
        assert ConvLSTMPolicy(A, P, Cc).ppo_scratch_shape(K_, E, N, T) == (floats,), (K_, E, N, P, A, Cc, T)
        assert _capi.SSD_RPPO_GROUPS(E * N // P, P) == groups and _capi.SSD_RPPO_SPLITS(min(T, K_) * (E * N // P)) == splits
    pol = ConvLSTMPolicy(8, 5, 128)
    assert pol.ppo_scratch_shape(16, 4096, 5, 16) == pol.ppo_scratch_shape(128, 4096, 5, 16) == pol.ppo_scratch_shape(10 ** 4, 4096, 5, 16)
    assert _capi.SSD_RPPO_GROUPS(257, 64) == 16 and _capi.SSD_RPPO_GROUPS(17, 5) == 2 and _capi.SSD_RPPO_GROUPS(10 ** 6, 1) == 1024


# (K, T, E, done mode, seed): the GPU accuracy cases' inputs that a wrong treatment of time could pass through, with the seeds of
# test_ppo_lstm_gpu.py's CASES (`done="per_env"` at (7, 3): 21; `done="mid"` at (5, 5): 22)
NEAR_MISS = [(7, 3, 17, "per_env", 21), (5, 5, 17, "mid", 22)]


@pytest.mark.parametrize("K_,T,E,mode,seed", NEAR_MISS)
def test_bound_separates_the_gradient_from_a_near_miss(K_, T, E, mode, seed):
    """Would the bound notice?  In float64, the gradient of a "kernel" that cut BPTT at every step, of one that ignored done and
    of one that dropped the ragged last window each differ from the true gradient by at least 10 times the bound (et from the
    CPU's float32) in lstm_w and in a trunk tensor.  A condition on the inputs, not a measurement of the kernel."""
    N = 5
    pol = make_policy(8, N, 64, seed=seed)
    t, first = make_inputs(pol, K_, E, N, T, seed=100 + seed, done_mode=mode)
    rep = branch_report(pol, t, HYPER, first, T)
    assert rep["margin"] > MARGIN, rep
    _, _, g64 = autograd_loss(pol, t, HYPER, first, T)
    _, _, g32 = autograd_loss(pol, t, HYPER, first, T, dtype=torch.float32)
    variants = ["cut", "ignore_done"] + (["drop_last"] if K_ % T else [])
    for variant in variants:
        _, _, gv = autograd_loss(pol, t, HYPER, first, T, variant=variant)
        for name in ("lstm_w", "fc1_w"):
            b = bound(g64[name], max_err(g32[name], g64[name]))
            off = max_err(gv[name], g64[name])
            print("%-12s %-7s off %.3e bound %.3e ratio %.1f" % (variant, name, off, b, off / b))
            assert off >= 10 * b, (variant, name, off, b)


# ---- would the bound notice a row lost or doubled in the split-K kernel's second pass? ----
SPLIT_TENSORS = ("lstm_w", "lstm_b")                             # what ssd_bptt_dw_kernel writes
SPLIT_PROBES = ("second_chunks", "last_of_first_pass", "first_of_second_pass", "last_of_ragged_chunk", "window2_first", "window2_last")
BRANCHES = ("clipped_pos", "clipped_neg", "open_pos", "open_neg", "vf_dead", "vf_live", "vf_clipped_live")
_SPLIT_CACHE = {}


def _split_case(shape, kind):
    """The GPU split case's own policy and inputs (test_ppo_lstm_gpu.py's SPLIT_CASES) with the float64 gradient and each
    tensor's bound (et from the CPU's float32), computed once and shared (never modified)."""
    if (shape, kind) not in _SPLIT_CACHE:
        splits = _capi.SSD_RPPO_MAX_SPLITS
        pol, t, first, h, (K_, T, E, N, P), (probes, _, unlit) = split_case(shape, kind, 64, splits, _capi.SSD_RPPO_CHUNK)
        assert _capi.SSD_RPPO_SPLITS(T * (E * N // P)) == splits == 32
        rep = branch_report(pol, t, h, first, T)
        print("split", shape, kind, rep)
        assert rep["margin"] > MARGIN, rep
        if kind == "ordinary":
            assert all(rep[k] > 0.2 for k in BRANCHES), rep
        _, _, g64 = autograd_loss(pol, t, h, first, T)
        _, _, g32 = autograd_loss(pol, t, h, first, T, dtype=torch.float32)
        bounds = {name: bound(g64[name], max_err(g32[name], g64[name])) for name in g64}
        _SPLIT_CACHE[shape, kind] = (pol, t, first, h, (K_, T, E, N, P), g64, bounds, probes, unlit)
    return _SPLIT_CACHE[shape, kind]


def _split_defect(case, rows, tensors, what):
    """The rows' share of the gradient by the twin: asserts that the two shares add up to the gradient, and returns for each
    tensor how far a kernel that dropped the rows from its sums, and one that counted them twice, would be off, over the
    bound."""
    pol, t, first, h, (K_, T, E, N, P), g64, bounds, _, _ = case
    _, _, g = autograd_loss(pol, t, h, first, T, twin_rows=rows_mask(K_, T, E, N, P, rows))
    out = {}
    for name in tensors:
        rest, share = g[name]
        assert max_err(rest + share, g64[name]) <= 1e-12 * max(1.0, float(g64[name].abs().max())), name
        out[name] = (max_err(rest, g64[name]) / bounds[name], max_err(rest + 2 * share, g64[name]) / bounds[name])
        print("%-28s %-8s dropped / bound %.1f  twice / bound %.1f" % (what, name, *out[name]))
    return out


@pytest.mark.parametrize("probe", SPLIT_PROBES)
@pytest.mark.parametrize("shape", sorted(SPLIT_SHAPES))
def test_bound_separates_a_row_of_a_second_chunk(shape, probe):
    """A condition on the spotlight inputs of the GPU split cases, not a measurement of the kernel: in float64, losing or
    doubling the probed window set rows -- all rows of the second chunks, the last row of split 31's only chunk, the first row
    of split 0's second, the last valid row of the ragged chunk, the first and the last row of the second window -- moves
    lstm_w and lstm_b by at least 10 times the bound.  At P = N the last set is probed, which a kernel that dropped `+ p` from
    the row would get wrong; the whole chunks also in set 0."""
    case = _split_case(shape, "spotlight")
    P, probes = case[4][4], case[7]
    window, rng = probes[probe]
    for p in sorted({P - 1, 0} if probe == "second_chunks" else {P - 1}):
        for name, ratios in _split_defect(case, [(window, p, rng)], SPLIT_TENSORS, "%s %s set %d" % (shape, probe, p)).items():
            assert min(ratios) >= 10.0, (shape, probe, p, name, ratios)


@pytest.mark.parametrize("shape", sorted(SPLIT_SHAPES))
def test_an_unlit_row_moves_nothing(shape):
    """The spotlight's dark rows are dark: an unlit row of window 1's last step has an exactly zero share of every tensor."""
    case = _split_case(shape, "spotlight")
    pol, t, first, h, (K_, T, E, N, P), g64, _, _, (window, rng) = case
    _, _, g = autograd_loss(pol, t, h, first, T, twin_rows=rows_mask(K_, T, E, N, P, [(window, P - 1, rng)]))
    for name in g:
        assert float(g[name][1].abs().max()) == 0.0 and torch.equal(g[name][0], g64[name]), name


@pytest.mark.parametrize("shape", sorted(SPLIT_SHAPES))
def test_bound_separates_whole_second_chunks_with_ordinary_rows(shape):
    """With ordinary make_inputs rows one row in 2310 is about the bound's floor; all rows of the second chunks are not."""
    case = _split_case(shape, "ordinary")
    P, (window, rng) = case[4][4], case[7]["second_chunks"]
    for name, ratios in _split_defect(case, [(window, P - 1, rng)], SPLIT_TENSORS, "%s ordinary second_chunks" % shape).items():
        assert min(ratios) >= 10.0, (shape, name, ratios)
