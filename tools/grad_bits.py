"""Do two builds of the library -- or two versions of the Python layer on one library -- give the same bits in the eleven loss
calls and the Watershed sequence forward?  For the four BPTT calls (ppo_loss_recurrent, a3c_loss_recurrent, ppo_loss_moa, a3c_loss_moa), fixed inputs from the tests' makers (tests/ppo_lstm_ref.py, tests/ppo_moa_ref.py)
at the smallest shapes that reach every shared device piece of csrc/ssd_bptt_device.hpp: (K, T) = (5, 3) (a ragged last window
and the accumulate path), E = 17 (two 16-sequence tiles, the second with one live row), N = P = 5, A = 8, done per env, obs_first
and behaviour logits given, at C = 64, 128 and 256; at C = 64 also P = 1 (stride 1), E = 33 (a second 64-row chunk) and, for the
MOA policy, N = P = 11 (string order differs from index order, and the prediction tile is partial).  ppo_loss and a3c_loss:
tests/ppo_ref.py's and tests/a3c_ref.py's makers at (K, E, N) = (3, 17, 5) with P = 1 and P = 5, obs_first and behaviour logits
given.  ppo_loss_watershed, a3c_loss_watershed and evaluate_sequences (dist, value, logp, bootstrap value): tests/ws_ppo_ref.py's
makers at M = 5, T = 3, Q = 17 (one full tile and one live row) at C = 64, 128 and 256, and Q = 33 at C = 64 (a window of 99
rows: a second, ragged 64-row chunk), for SEQ_COMM, a comm id and an action id, starts per sequence and dist given.  The three
IMPALA calls: tests/impala_ref.py's make_batch at the shapes of tests/test_impala_loss_cpu.py
(K = 5, E = 3, N = P = 2, T = 2).  Loss, statistics and every parameter's gradient of every call go to an .npz; run once per
library (or per tree) in a fresh process, then compare the uint32 views.  --cpu: the same cases on CPU tensors, the plain-torch
paths, which need no GPU.

    SSD_LIB_PATH=/path/to/libssd_hip.so python tools/grad_bits.py [--cpu] out.npz
    python tools/grad_bits.py --compare a.npz b.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K_, T = 5, 3
# (C, E, N, P)
LSTM_CASES = [(64, 17, 5, 5), (128, 17, 5, 5), (256, 17, 5, 5), (64, 17, 5, 1), (64, 33, 5, 5)]
MOA_CASES = LSTM_CASES + [(64, 17, 11, 11)]
A = 8
A3C = dict(vf_loss_coeff=0.5, entropy_coeff=0.01)
FC_SHAPE = (3, 17, 5)                                               # (K, E, N) of ppo_loss and a3c_loss, with P = 1 and P = N
WS_M, WS_T = 5, 3                                                   # the Watershed calls: a ragged last window, the accumulate path
WS_CASES = [(64, 17), (128, 17), (256, 17), (64, 33)]               # (C, Q): a second tile with one live row; 99 rows, a second chunk
WS_AGENTS = (1, 5)                                                  # a comm id and an action id of SEQ_COMM
IMPALA_SHAPE = dict(A=8, N=2, P=2, K=5, E=3, T=2)


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    if sorted(a.files) != sorted(b.files):
        print("different arrays: %s" % sorted(set(a.files) ^ set(b.files)))
        return 1
    bad = 0
    for name in sorted(a.files):
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        same = x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32))
        bad += not same
        if not same:
            print("DIFFERENT %s" % name)
    print("%d arrays, %d different" % (len(a.files), bad))
    return 1 if bad else 0


def record(out, tag, pol, loss, stats):
    pol.zero_grad()
    loss.backward()
    out[tag + "/loss"] = loss.detach().cpu().numpy().reshape(1)
    for name, s in stats.items():
        out[tag + "/stat/" + name] = s.detach().cpu().numpy()
    for name, _, _ in pol.layout():
        out[tag + "/grad/" + name] = getattr(pol, name).grad.detach().cpu().numpy()


def main(path, cpu=False):
    import torch

    import a3c_ref
    import impala_ref
    import ppo_lstm_ref
    import ppo_moa_ref
    import ppo_ref
    import ws_ppo_ref
    import sequential_social_dilemma_games_amd as ssd
    from sequential_social_dilemma_games_amd import _capi, a3c_loss_moa, a3c_loss_recurrent, ppo_loss_moa, ppo_loss_recurrent

    dev = torch.device("cpu") if cpu else torch.device("cuda", 0)
    print("package: %s\nlibrary: %s\ndevice: %s" % (os.path.dirname(ssd.__file__), _capi.LIB_PATH, dev))
    out = {}
    K, E, N = FC_SHAPE
    for P in (1, N):
        pol = ppo_ref.make_policy(A, P, seed=7 + P)
        t, first = ppo_ref.make_inputs(pol, K, E, N, seed=107 + P)
        pol, t, first = pol.to(dev), {k: v.to(dev) for k, v in t.items()}, first.to(dev)
        record(out, "fc/P%d/ppo" % P, pol, *ssd.ppo_loss(pol, t, obs_first=first, **ppo_ref.HYPER))
        pol = a3c_ref.make_policy("fc", A, N, P, seed=7 + P)
        t, first = a3c_ref.make_inputs("fc", pol, K, E, N, None, seed=107 + P)
        pol, t, first = pol.to(dev), {k: v.to(dev) for k, v in t.items()}, first.to(dev)
        record(out, "fc/P%d/a3c" % P, pol, *ssd.a3c_loss(pol, t, obs_first=first, **A3C))
        print("fc/P%d" % P)
    M, Tw = WS_M, WS_T
    for C, Q in WS_CASES:
        for agent in WS_AGENTS:
            pol = ws_ppo_ref.make_policy(_capi.SSD_WS_SEQ_COMM, C, seed=20 + agent + C + Q)
            t = ws_ppo_ref.make_inputs(pol, agent, M, Q, Tw, seed=120 + agent + C + Q, starts_mode="per_seq")
            g = torch.Generator().manual_seed(220 + agent + C + Q)
            t["obs_next"] = t["obs"][torch.randint(0, M, (1,), generator=g).item()].flip(0).contiguous()
            t["start_next"] = (torch.rand((Q,), generator=g) < 0.3).to(torch.uint8)
            pol, t = pol.to(dev), {k: v.to(dev) for k, v in t.items()}
            tag = "ws/C%d_Q%d_agent%d" % (C, Q, agent)
            record(out, tag + "/ppo", pol, *ssd.ppo_loss_watershed(pol, agent, t, seq_len=Tw, **ppo_ref.HYPER))
            record(out, tag + "/a3c", pol, *ssd.a3c_loss_watershed(pol, agent, t, seq_len=Tw, **A3C))
            names = ("dist", "value", "logp", "bootstrap_value")
            for name, x in zip(names, ssd.evaluate_sequences(pol, agent, t, Tw)):
                out[tag + "/eval/" + name] = x.detach().cpu().numpy()
            print(tag)
    s = IMPALA_SHAPE
    for kind in ("fc", "lstm", "moa"):
        pol, t, first = impala_ref.make_batch(kind, s["A"], s["N"], s["P"], s["K"], s["E"], s["T"], seed=40)
        pol, t, first = pol.to(dev), {k: v.to(dev) for k, v in t.items()}, first.to(dev)
        if kind == "fc":
            res = ssd.impala_loss(pol, t, obs_first=first, **impala_ref.HYPER)
        elif kind == "lstm":
            res = ssd.impala_loss_recurrent(pol, t, seq_len=s["T"], obs_first=first, **impala_ref.HYPER)
        else:
            res = ssd.impala_loss_moa(pol, t, seq_len=s["T"], moa_weight=impala_ref.MOA_WEIGHT,
                                      influence_weight=impala_ref.INFLUENCE_WEIGHT, obs_first=first, **impala_ref.HYPER)
        record(out, "impala/" + kind, pol, *res)
        print("impala/" + kind)
    for C, E, N, P in LSTM_CASES:
        pol = ppo_lstm_ref.make_policy(A, P, C, seed=C + E + P)
        t, first = ppo_lstm_ref.make_inputs(pol, K_, E, N, T, seed=100 + C + E + P, done_mode="per_env")
        pol, t, first = pol.to(dev), {k: v.to(dev) for k, v in t.items()}, first.to(dev)
        tag = "lstm/C%d_E%d_N%d_P%d" % (C, E, N, P)
        record(out, tag + "/ppo", pol, *ppo_loss_recurrent(pol, t, seq_len=T, obs_first=first, **ppo_lstm_ref.HYPER))
        record(out, tag + "/a3c", pol, *a3c_loss_recurrent(pol, t, seq_len=T, obs_first=first, **A3C))
        print(tag)
    for C, E, N, P in MOA_CASES:
        pol = ppo_moa_ref.make_policy(A, N, P, C, seed=C + E + P)
        t, first = ppo_moa_ref.make_inputs(pol, K_, E, N, T, seed=100 + C + E + P, done_mode="per_env")
        pol, t, first = pol.to(dev), {k: v.to(dev) for k, v in t.items()}, first.to(dev)
        tag = "moa/C%d_E%d_N%d_P%d" % (C, E, N, P)
        w = ppo_moa_ref.MOA_WEIGHT
        record(out, tag + "/ppo", pol, *ppo_loss_moa(pol, t, seq_len=T, moa_weight=w, obs_first=first, **ppo_moa_ref.HYPER))
        record(out, tag + "/a3c", pol, *a3c_loss_moa(pol, t, seq_len=T, moa_weight=w, obs_first=first, **A3C))
        print(tag)
    if not cpu:
        torch.cuda.synchronize()
    np.savez(path, **out)
    print("%d arrays -> %s" % (len(out), path))
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    args = [a for a in sys.argv[1:] if a != "--cpu"]
    if len(args) != 1:
        sys.exit(__doc__)
    sys.exit(main(args[0], cpu="--cpu" in sys.argv[1:]))
