"""What the MOA policy's PPO + MOA loss and its gradients cost: ppo_loss_moa + backward
(ssd_policy_moa_ppo_grad) against the torch path a user had before -- forward_sequence per window, ppo_terms, moa_loss,
backward -- on the same box and the same sampled fragment, for Harvest 4096 x 5 with C = 128 and windows of 16 steps: K = 16
(one window) and K = 128.  Device events around each leg, one warm-up of each, the legs alternated, at least 3 pairs; per leg the peak of
torch's allocator above what was allocated before it, and the scratch the kernel path keeps.  The first line says which
library ran (tools/_label.py); then one JSON line per shape.

    python tools/ppo_moa_grad_rate.py [--loss a3c] [--envs 4096] [--steps 128] [--seq-len 16] [--cells 128] [--pairs 3] [--torch-full]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sequential_social_dilemma_games_amd import ConvMOAPolicy, a3c_loss_moa, ppo_loss_moa  # noqa: E402
from sequential_social_dilemma_games_amd import constants as K  # noqa: E402
from sequential_social_dilemma_games_amd.policy import _set_means, _set_sums, a3c_terms, moa_forward, ppo_terms  # noqa: E402
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv  # noqa: E402
from tools._label import label_line  # noqa: E402

FP32_PEAK = 157.3e12            # MI355X_MICROARCH.md: FP32 vector = FP32 matrix peak
DEV = torch.device("cuda", 0)
HYPER = dict(clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1e-4, entropy_coeff=1e-3, kl_coeff=0.0)
MOA_WEIGHT = 10.0               # train_moa.py's default
A3C_HYPER = dict(vf_loss_coeff=0.5, entropy_coeff=0.01)          # a3c_causal.py's defaults
LOSS = "ppo"                    # --loss


def flop_per_row(C, A, N):
    """What the loss needs, not what the call spends: the trunk's 307 kFLOP (conv and one stack, forward
    and backward) and the second stack's 3 * 2 * (1014 * 32 + 32 * 32); the two cells: forward 2 (32 + C) 4C and 2 (48 + C) 4C
    for the gates, 2 C (A + 1) for the heads and 2 C (N - 1) A for the prediction; backward twice that.  (The call runs the conv
    and its backward once per stack and the forward of both stacks three times.)"""
    return (307e3 + 3 * 2 * (1014 * 32 + 32 * 32)
            + 3 * (2 * (32 + C) * 4 * C + 2 * (48 + C) * 4 * C + 2 * C * (A + 1) + 2 * C * (N - 1) * A))


def torch_leg(policy, batch, first, seq_len):
    obs = torch.cat([first.unsqueeze(0), batch["obs"][:-1]])
    logits, value, moa = moa_forward(policy, obs, batch["prev_actions"], batch["state"], batch["done"], seq_len)
    t = {"actions": batch["actions"], "logp_old": batch["logp"], "advantages": batch["advantages"],
         "value_targets": batch["value_targets"], "vf_pred": batch["value"]}
    loss = _set_means(ppo_terms(logits, value, t, *HYPER.values())[0], policy.num_sets).sum()
    A, P = policy.num_actions, policy.num_sets
    others = batch["actions"].long()[..., policy._others.to(DEV)]
    for p in range(P):                                           # policy.moa_loss of each set's rows (P = N: agent p's)
        loss = loss + MOA_WEIGHT * torch.nn.functional.cross_entropy(moa[:, :, p].reshape(-1, A), others[:, :, p].reshape(-1))
    policy.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach()


def kernel_leg(policy, batch, first, seq_len):
    loss, _ = ppo_loss_moa(policy, batch, seq_len=seq_len, moa_weight=MOA_WEIGHT, obs_first=first, **HYPER)
    policy.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach()


def a3c_torch_leg(policy, batch, first, seq_len):
    """a3c_loss_moa's CPU path (moa_forward, a3c_terms, the mean cross-entropy per set) on the device, and its backward."""
    obs = torch.cat([first.unsqueeze(0), batch["obs"][:-1]])
    logits, value, moa = moa_forward(policy, obs, batch["prev_actions"], batch["state"], batch["done"], seq_len)
    loss = _set_sums(a3c_terms(logits, value, batch, *A3C_HYPER.values())[0], policy.num_sets).sum()
    A, P = policy.num_actions, policy.num_sets
    others = batch["actions"].long()[..., policy._others.to(DEV)]
    for p in range(P):
        loss = loss + MOA_WEIGHT * torch.nn.functional.cross_entropy(moa[:, :, p].reshape(-1, A), others[:, :, p].reshape(-1))
    policy.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach()


def a3c_kernel_leg(policy, batch, first, seq_len):
    loss, _ = a3c_loss_moa(policy, batch, seq_len=seq_len, moa_weight=MOA_WEIGHT, obs_first=first, **A3C_HYPER)
    policy.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach()


def measure(leg, *args):
    """(ms, peak bytes above the start) of one call of leg."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    loss = leg(*args)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated(DEV) - base, float(loss)


def shape_line(what, policy, batch, first, seq_len, pairs, with_torch):
    rows = batch["actions"].numel()
    Kk, E, N = batch["actions"].shape
    legs = [("kernel", kernel_leg)] + ([("torch", torch_leg)] if with_torch else [])
    cycles = [legs]
    if LOSS == "a3c":
        # the A3C call and the PPO call of the same library alternated on their own, then the A3C torch path: whichever kernel
        # leg follows the torch leg in a cycle runs 2 to 4 % slower at the one-window shapes
        cycles = [[("kernel", a3c_kernel_leg), ("ppo_kernel", kernel_leg)]] + ([[("torch", a3c_torch_leg)]] if with_torch else [])
        legs = [leg for cycle in cycles for leg in cycle]
    ms = {name: [] for name, _ in legs}
    peak, loss = {}, {}
    policy._ppo_scratch = None                                   # the kernel leg's first call allocates it: counted in its peak
    for name, leg in legs:                                       # warm-up: allocator, packed(), code objects
        _, p, _ = measure(leg, policy, batch, first, seq_len)
        peak[name] = p
    for cycle in cycles:
        for _ in range(pairs):                                   # alternated: a drift of the box shows in both legs
            for name, leg in cycle:
                t, p, ls = measure(leg, policy, batch, first, seq_len)
                ms[name].append(t)
                peak[name] = max(peak[name], p)
                loss[name] = ls
    line = {"what": what, "rows": rows, "pairs": pairs, "seq_len": seq_len, "cells": policy.cell_size,
            "scratch_MiB": round(policy.ppo_scratch_shape(Kk, E, N, seq_len)[0] * 4 / 2 ** 20, 1),
            "flop_per_row": flop_per_row(policy.cell_size, policy.num_actions, N)}
    for name, _ in legs:
        line[name + "_ms"] = [round(x, 3) for x in ms[name]]
        line[name + "_ms_median"] = round(statistics.median(ms[name]), 3)
        line[name + "_peak_MiB"] = round(peak[name] / 2 ** 20, 1)
        line[name + "_loss"] = loss[name]
    k = line["kernel_ms_median"]
    line["kernel_frac_fp32_peak"] = round(rows * line["flop_per_row"] / (k * 1e-3) / FP32_PEAK, 4)
    if with_torch:
        line["torch_over_kernel"] = round(line["torch_ms_median"] / k, 2)
    if LOSS == "a3c":
        line["loss"] = "a3c"
        line["a3c_over_ppo_kernel"] = round(k / line["ppo_kernel_ms_median"], 4)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--seq-len", type=int, default=16)
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--torch-full", action="store_true", help="also run the torch leg on the full fragment (it keeps every activation)")
    ap.add_argument("--loss", choices=("ppo", "a3c"), default="ppo",
                    help="a3c: the A3C call (kernel) alternated with the PPO call (ppo_kernel) and the A3C torch path (torch)")
    args = ap.parse_args()
    global LOSS
    LOSS = args.loss
    assert torch.cuda.is_available(), "this tool measures the GPU"
    assert args.pairs >= 3, "at least 3 pairs"
    print(label_line("ppo_moa_grad_rate %s" % " ".join(sys.argv[1:])), flush=True)
    N, T = 5, args.seq_len
    env = SSDVectorEnv(K.GAME_HARVEST, args.envs, N, horizon=1000, seed=1)
    policy = ConvMOAPolicy(env.engine.num_actions, num_agents=N, num_sets=N, cell_size=args.cells, seed=2).to(DEV)
    first = env.reset().clone()
    batch = env.sample(policy, args.steps, state_every=T, gamma=0.99, lambda_=0.95, influence_weight=1.0)
    one = {k: v[:T] for k, v in batch.items() if k not in ("last_value", "state", "state_in")}
    one["state"] = batch["state"][:1]
    print(json.dumps(shape_line("one window %d x %d x %d" % (T, args.envs, N), policy, one, first, T, args.pairs, True)), flush=True)
    print(json.dumps(shape_line("fragment %d x %d x %d" % (args.steps, args.envs, N), policy, batch, first, T, args.pairs,
                                args.torch_full)), flush=True)


if __name__ == "__main__":
    main()
