"""What the advantages cost: the kernel alone with its bytes as a fraction of 6.3 TB/s, the backward
loop over K in torch (float64, on the same device) that a user would write without it, and SSDVectorEnv.sample of 128 steps
with and without gamma.  Device events around work that ends in a synchronise; one JSON line per figure.

    python tools/gae_rate.py [--reps 200] [--skip-sample]

The load-block length of the kernel is a compile-time constant: for another one, `make -C sequential_social_dilemma_games_amd/csrc
exp EXP=-DSSD_GAE_LOAD_BLOCK=n`, then run this with SSD_LIB_PATH=.../libssd_hip_exp.so.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sequential_social_dilemma_games_amd import ConvFCPolicy, compute_advantages  # noqa: E402
from sequential_social_dilemma_games_amd import constants as K  # noqa: E402
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv  # noqa: E402

HBM_BPS = 6.3e12
DEV = torch.device("cuda", 0)


def timed(fn, reps):
    """Mean µs per call of fn over reps calls (after two warm-up calls)."""
    fn()
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def rings(E, N, steps):
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    rew = torch.randint(-2, 2, (steps, E, N), device=DEV, generator=g, dtype=torch.int32)
    rew[rew == -2] = -50
    value = torch.randn((steps, E, N), device=DEV, generator=g)
    done = (torch.rand((steps, E, N), device=DEV, generator=g) < 0.001).to(torch.uint8)
    last = torch.randn((E, N), device=DEV, generator=g)
    return rew, value, done, last


def torch_loop(rew, value, done, last, gamma, lam):
    """The same advantages as a backward loop of torch operations in float64: what a user of the batches writes today."""
    steps = rew.shape[0]
    adv, vt = torch.empty_like(value), torch.empty_like(value)
    v_after, run = last.double(), torch.zeros_like(last, dtype=torch.float64)
    gl = gamma * lam
    for k in range(steps - 1, -1, -1):
        keep = 1.0 - done[k].double()
        vk = value[k].double()
        delta = (rew[k].double() + gamma * (v_after * keep)) - vk
        run = delta + gl * (run * keep)
        adv[k] = run.float()
        vt[k] = (run + vk).float()
        v_after = vk
    return adv, vt


def kernel_rate(E, N, steps, reps, loop_reps):
    rew, value, done, last = rings(E, N, steps)
    out = (torch.empty_like(value), torch.empty_like(value))
    us = timed(lambda: compute_advantages(rew, value, last, done, gamma=0.99, lambda_=0.95, out=out), reps)
    moved = steps * E * N * (4 + 4 + 1 + 4 + 4)                  # rew, value, done in; advantages, value_targets out
    line = {"what": "compute_advantages (GAE)", "L": E * N, "K": steps, "us": round(us, 2), "bytes": moved,
            "frac_of_6.3TBps": round(moved / (us * 1e-6) / HBM_BPS, 4)}
    if loop_reps:
        a, t = torch_loop(rew, value, done, last, 0.99, 0.95)
        line["torch_loop_equal_bits"] = bool(torch.equal(a.view(torch.int32), out[0].view(torch.int32))
                                             and torch.equal(t.view(torch.int32), out[1].view(torch.int32)))
        line["torch_loop_us"] = round(timed(lambda: torch_loop(rew, value, done, last, 0.99, 0.95), loop_reps), 1)
        line["torch_loop_over_kernel"] = round(line["torch_loop_us"] / us, 1)
    return line


def sample_rate(E, N, steps, reps, gamma):
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=1000, seed=1)
    env.reset()
    pol = ConvFCPolicy(env.engine.num_actions, N, seed=2).to(DEV)
    us = timed(lambda: env.sample(pol, steps, gamma=gamma, lambda_=0.95), reps)
    return {"what": "SSDVectorEnv.sample ConvFCPolicy", "E": E, "N": N, "K": steps, "gamma": gamma, "us": round(us, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--sample-reps", type=int, default=5)
    ap.add_argument("--skip-sample", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures the GPU"
    lines = [lambda: kernel_rate(4096, 5, 128, args.reps, args.loop_reps),
             lambda: kernel_rate(4096, 5, 1000, args.reps, args.loop_reps),
             lambda: kernel_rate(32768, 5, 1000, args.reps, args.loop_reps)]
    if not args.skip_sample:
        for gamma in (None, 0.99, None, 0.99):                   # alternated: the spread shows in the repeat
            lines.append(lambda gamma=gamma: sample_rate(4096, 5, 128, args.sample_reps, gamma))
    for ln in lines:
        print(json.dumps(ln()), flush=True)


if __name__ == "__main__":
    main()
