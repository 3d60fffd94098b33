"""What the PPO loss and its gradients cost: ppo_loss + backward (ssd_policy_ppo_grad, two launches) against
the loss of examples/ppo_update.py + backward in torch on the same box and the same sampled fragment -- the path a user had
before --, for Harvest 4096 x 5 x 128 as one batch and for a 16-step minibatch of it.  Device events around each leg, one
warm-up of each, the legs alternated, at least 3 pairs; per leg the peak of torch's allocator above what was allocated before
it.  One JSON line per shape.

    python tools/ppo_grad_rate.py [--loss a3c] [--envs 4096] [--steps 128] [--minibatch 16] [--pairs 3] [--skip-torch-full]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sequential_social_dilemma_games_amd import ConvFCPolicy, a3c_loss, ppo_loss  # noqa: E402
from sequential_social_dilemma_games_amd import constants as K  # noqa: E402
from sequential_social_dilemma_games_amd.policy import _set_sums, a3c_terms  # noqa: E402
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv  # noqa: E402

FP32_PEAK = 157.3e12            # MI355X_MICROARCH.md: FP32 vector = FP32 matrix peak
FLOP_PER_ROW = 307e3            # forward 2 x 51 k MAC (conv 27.4 k, fc1 32.4 k, the rest 1.3 k), backward 2 x as much less dx of the conv
DEV = torch.device("cuda", 0)
HYPER = dict(clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1e-4, entropy_coeff=1e-3, kl_coeff=0.0)
A3C_HYPER = dict(vf_loss_coeff=0.5, entropy_coeff=0.01)          # a3c_causal.py's defaults
LOSS = "ppo"                    # --loss


def torch_leg(policy, batch, first):
    """examples/ppo_update.py's loss (with the clipped value loss of HYPER) and its backward."""
    obs = torch.cat([first.unsqueeze(0), batch["obs"][:-1]])
    logits, value = policy(obs)
    logp_all = torch.log_softmax(logits, dim=-1)
    logp = logp_all.gather(-1, batch["actions"].long().unsqueeze(-1)).squeeze(-1)
    adv, vt, vfp = batch["advantages"], batch["value_targets"], batch["value"]
    ratio = torch.exp(logp - batch["logp"])
    c, vc = HYPER["clip_param"], HYPER["vf_clip_param"]
    surrogate = torch.minimum(ratio * adv, ratio.clamp(1 - c, 1 + c) * adv)
    entropy = -(logp_all.exp() * logp_all).sum(-1)
    vf = torch.maximum((value - vt).square(), (vfp + (value - vfp).clamp(-vc, vc) - vt).square())
    row = -surrogate + HYPER["vf_loss_coeff"] * vf - HYPER["entropy_coeff"] * entropy
    loss = row.reshape(-1, policy.num_sets).mean(0).sum()
    policy.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach()


def kernel_leg(policy, batch, first):
    loss, _ = ppo_loss(policy, batch, obs_first=first, **HYPER)
    policy.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach()


def a3c_torch_leg(policy, batch, first):
    """a3c_loss's CPU path (a3c_terms over the policy's forward) on the device, and its backward."""
    obs = torch.cat([first.unsqueeze(0), batch["obs"][:-1]])
    logits, value = policy(obs)
    loss = _set_sums(a3c_terms(logits, value, batch, *A3C_HYPER.values())[0], policy.num_sets).sum()
    policy.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach()


def a3c_kernel_leg(policy, batch, first):
    loss, _ = a3c_loss(policy, batch, obs_first=first, **A3C_HYPER)
    policy.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach()


def measure(leg, policy, batch, first):
    """(ms, peak bytes above the start) of one call of leg."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    loss = leg(policy, batch, first)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated(DEV) - base, float(loss)


def shape_line(what, policy, batch, first, pairs, with_torch):
    rows = batch["actions"].numel()
    legs = [("kernel", kernel_leg)] + ([("torch", torch_leg)] if with_torch else [])
    cycles = [legs]
    if LOSS == "a3c":
        # the A3C call and the PPO call of the same library alternated on their own, then the A3C torch path: whichever kernel
        # leg follows the torch leg in a cycle runs 2 to 4 % slower at the one-window shapes
        cycles = [[("kernel", a3c_kernel_leg), ("ppo_kernel", kernel_leg)]] + ([[("torch", a3c_torch_leg)]] if with_torch else [])
        legs = [leg for cycle in cycles for leg in cycle]
    ms = {name: [] for name, _ in legs}
    peak, loss = {}, {}
    for name, leg in legs:                                       # warm-up: allocator, packed(), code objects
        measure(leg, policy, batch, first)
    for cycle in cycles:
        for _ in range(pairs):                                   # alternated: a drift of the box shows in both legs
            for name, leg in cycle:
                t, p, ls = measure(leg, policy, batch, first)
                ms[name].append(t)
                peak[name] = max(peak.get(name, 0), p)
                loss[name] = ls
    line = {"what": what, "rows": rows, "pairs": pairs}
    for name, _ in legs:
        line[name + "_ms"] = [round(x, 3) for x in ms[name]]
        line[name + "_ms_median"] = round(statistics.median(ms[name]), 3)
        line[name + "_peak_MiB"] = round(peak[name] / 2 ** 20, 1)
        line[name + "_loss"] = loss[name]
    k = line["kernel_ms_median"]
    line["kernel_frac_fp32_peak"] = round(rows * FLOP_PER_ROW / (k * 1e-3) / FP32_PEAK, 4)
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
    ap.add_argument("--minibatch", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--skip-torch-full", action="store_true", help="the torch leg of the full batch keeps some 40 GB of activations")
    ap.add_argument("--loss", choices=("ppo", "a3c"), default="ppo",
                    help="a3c: the A3C call (kernel) alternated with the PPO call (ppo_kernel) and the A3C torch path (torch)")
    args = ap.parse_args()
    global LOSS
    LOSS = args.loss
    assert torch.cuda.is_available(), "this tool measures the GPU"
    assert args.pairs >= 3, "at least 3 pairs"
    N = 5
    env = SSDVectorEnv(K.GAME_HARVEST, args.envs, N, horizon=1000, seed=1)
    policy = ConvFCPolicy(env.engine.num_actions, num_sets=N, seed=2).to(DEV)
    first = env.reset().clone()
    batch = env.sample(policy, args.steps, gamma=0.99, lambda_=0.95)
    k0 = args.steps // 2
    mb = {k: v[k0:k0 + args.minibatch] for k, v in batch.items() if k != "last_value"}
    print(json.dumps(shape_line("minibatch %d x %d x %d" % (args.minibatch, args.envs, N), policy, mb, batch["obs"][k0 - 1],
                                args.pairs, True)), flush=True)
    print(json.dumps(shape_line("batch %d x %d x %d" % (args.steps, args.envs, N), policy, batch, first, args.pairs,
                                not args.skip_torch_full)), flush=True)


if __name__ == "__main__":
    main()
