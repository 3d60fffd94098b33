"""Do two builds of the library give the same bits in the four BPTT loss-and-gradient calls (ppo_loss_recurrent,
a3c_loss_recurrent, ppo_loss_moa, a3c_loss_moa)?  Fixed inputs from the tests' makers (tests/ppo_lstm_ref.py, tests/ppo_moa_ref.py)
at the smallest shapes that reach every shared device piece of csrc/ssd_bptt_device.hpp: (K, T) = (5, 3) (a ragged last window
and the accumulate path), E = 17 (two 16-sequence tiles, the second with one live row), N = P = 5, A = 8, done per env, obs_first
and behaviour logits given, at C = 64, 128 and 256; at C = 64 also P = 1 (stride 1), E = 33 (a second 64-row chunk) and, for the
MOA policy, N = P = 11 (string order differs from index order, and the prediction tile is partial).  Loss, statistics and every
parameter's gradient of every call go to an .npz; run once per library in a fresh process, then compare the uint32 views.

    SSD_LIB_PATH=/path/to/libssd_hip.so python tools/grad_bits.py out.npz
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


def main(path):
    import torch

    import ppo_lstm_ref
    import ppo_moa_ref
    from sequential_social_dilemma_games_amd import _capi, a3c_loss_moa, a3c_loss_recurrent, ppo_loss_moa, ppo_loss_recurrent

    dev = torch.device("cuda", 0)
    print("library: %s" % _capi.LIB_PATH)
    out = {}
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
    torch.cuda.synchronize()
    np.savez(path, **out)
    print("%d arrays -> %s" % (len(out), path))
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
