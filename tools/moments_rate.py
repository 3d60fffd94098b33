"""What the batch moments cost: ssd_standardize and ssd_explained_variance (three launches each) against
the torch expressions a user writes without them, alternated in one process, with the bytes each must move as a fraction of the
practical HBM rate, and SSDVectorEnv.sample of 128 steps with and without standardize.  Before a shape is timed the device's
out, moments and explained variance are compared with the package's CPU path bit for bit, on the whole shape, and the tool stops
with a message if they differ.  Device events around work that ends in
a synchronise; per leg the median over the rounds and the rounds' range; one JSON line per figure, the library's sha first.

    python tools/moments_rate.py [--rounds 7] [--reps 100] [--skip-sample]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sequential_social_dilemma_games_amd import ConvFCPolicy, _capi, explained_variance, standardize_advantages  # noqa: E402
from sequential_social_dilemma_games_amd import constants as K  # noqa: E402
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv  # noqa: E402

HBM_BPS = 6.29e12                                                # the measured float4-copy rate of the MI355X
DEV = torch.device("cuda", 0)


def timed(fn, reps):
    """Mean µs per call of fn over reps calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def alternated(legs, rounds, reps):
    """{name: fn} -> {name: {"median_us", "min_us", "max_us"}}: every round times each leg once, in turn."""
    for fn in legs.values():                                     # warm-up: code objects, torch's allocator
        fn()
        fn()
    torch.cuda.synchronize()
    us = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            us[name].append(timed(fn, reps))
    return {name: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
            for name, v in us.items()}


def torch_standardize(a, P):
    """The expression a user of the batches writes today (float32 reductions, temporaries of the batch's size)."""
    f = a.reshape(-1, P)
    return ((f - f.mean(0)) / f.std(0, unbiased=False).clamp_min(1e-4)).reshape(a.shape)


def torch_explained_variance(y, pred, P):
    y, d = y.reshape(-1, P), (y - pred).reshape(-1, P)
    return (1 - d.var(0, unbiased=False) / y.var(0, unbiased=False)).clamp_min(-1)


def same_bits(a, b):
    """Two tensors of one dtype hold the same bits (a NaN equals itself, +0.0 does not equal -0.0)."""
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    as_int = torch.int32 if a.dtype == torch.float32 else torch.int64
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(as_int), b.view(as_int))


def verify(x, pred, P):
    """What is timed below is what the contract says: the device's out, moments and explained variance against the package's
    CPU path (the NumPy restatement of the summation order, which the suite pins), bit for bit, on the whole shape."""
    out, moments = standardize_advantages(x, num_sets=P, return_moments=True)
    ev = explained_variance(x, pred, num_sets=P)
    host_out, host_moments = standardize_advantages(x.cpu(), num_sets=P, return_moments=True)
    host_ev = explained_variance(x.cpu(), pred.cpu(), num_sets=P)
    for name, got, want in (("out", out, host_out), ("moments", moments, host_moments), ("explained variance", ev, host_ev)):
        if not same_bits(got, want):
            sys.exit("moments_rate: at shape %s with %d set(s) the device's %s differs from the package's CPU path: nothing timed"
                     % (list(x.shape), P, name))


def kernel_rate(shape, P, rounds, reps):
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    x = torch.randn(shape, device=DEV, generator=g) * 3.0 + 0.5
    pred = x * 0.7 + 0.3 * torch.randn(shape, device=DEV, generator=g)
    verify(x, pred, P)
    out = torch.empty_like(x)
    res = alternated({"ssd_standardize": lambda: standardize_advantages(x, num_sets=P, out=out),
                      "torch_standardize": lambda: torch_standardize(x, P),
                      "ssd_explained_variance": lambda: explained_variance(x, pred, num_sets=P),
                      "torch_explained_variance": lambda: torch_explained_variance(x, pred, P)}, rounds, reps)
    floats = x.numel()
    moved = {"ssd_standardize": 3 * 4 * floats,                  # two reads and one write of the tensor
             "ssd_explained_variance": 4 * 4 * floats}           # two reads of both tensors
    diff = float((out - torch_standardize(x, P)).abs().max())
    line = {"shape": list(shape), "num_sets": P, "floats": floats, "equals_cpu_path_bit_for_bit": True,   # (verify() above)
            "max_abs_diff_to_torch": diff}
    for name, r in res.items():
        line[name] = r
        if name in moved:
            r["bytes"] = moved[name]
            r["frac_of_6.29TBps"] = round(moved[name] / (r["median_us"] * 1e-6) / HBM_BPS, 4)
    line["standardize_torch_over_kernel"] = round(res["torch_standardize"]["median_us"] / res["ssd_standardize"]["median_us"], 2)
    line["explained_variance_torch_over_kernel"] = round(res["torch_explained_variance"]["median_us"]
                                                         / res["ssd_explained_variance"]["median_us"], 2)
    return line


def sample_rate(E, N, steps, rounds, reps):
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=1000, seed=1)
    env.reset()
    pol = ConvFCPolicy(env.engine.num_actions, N, seed=2).to(DEV)
    res = alternated({"standardize=False": lambda: env.sample(pol, steps, gamma=0.99, lambda_=0.95),
                      "standardize=True": lambda: env.sample(pol, steps, gamma=0.99, lambda_=0.95, standardize=True)}, rounds, reps)
    return dict({"what": "SSDVectorEnv.sample ConvFCPolicy, gamma=0.99", "E": E, "N": N, "K": steps}, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--sample-reps", type=int, default=3)
    ap.add_argument("--skip-sample", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures the GPU"
    sha = hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(json.dumps({"library": os.path.basename(_capi.LIB_PATH), "sha256": sha, "device": torch.cuda.get_device_name(0),
                      "rounds": args.rounds, "reps": args.reps}), flush=True)
    for shape, P in (((128, 4096, 5), 5), ((128, 4096, 5), 1), ((16, 65536, 5), 5), ((16, 65536, 5), 1), ((16, 4096), 1)):
        print(json.dumps(kernel_rate(shape, P, args.rounds, args.reps)), flush=True)
    if not args.skip_sample:
        print(json.dumps(sample_rate(4096, 5, 128, args.rounds, args.sample_reps)), flush=True)


if __name__ == "__main__":
    main()
