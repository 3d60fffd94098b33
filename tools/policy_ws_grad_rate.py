"""What the Watershed PPO loss and its gradients cost: ppo_loss_watershed + backward
(ssd_ws_policy_ppo_grad) against the torch path a user had before -- forward_sequence per window, ws_ppo_terms, backward -- in
the same process on the same sequences, for SeqComm with C = 128 and windows of 16 steps: Q = 4096 and 65 536 sequences, an
action id and a comm id, one window (M = 16) and a fragment of 8 windows (M = 128).  The sequences are synthetic (random
observations, states and actions: the cost does not depend on the values).  Device events around each leg, one warm-up of each,
the legs alternated, at least 3 pairs; per leg the peak of torch's allocator above what was allocated before it, and the scratch
the kernel path keeps.  The first line says which library ran (tools/_label.py); then one JSON line per shape.

    python tools/policy_ws_grad_rate.py [--seqs 4096 65536] [--steps 128] [--seq-len 16] [--cells 128] [--agents 5 1] [--pairs 3] [--torch-full]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sequential_social_dilemma_games_amd import WatershedLSTMPolicy, _capi, ppo_loss_watershed  # noqa: E402
from sequential_social_dilemma_games_amd.policy import ws_forward_windows, ws_is_comm, ws_ppo_terms  # noqa: E402
from tools._label import label_line  # noqa: E402

FP32_PEAK = 157.3e12            # MI355X_MICROARCH.md: FP32 vector = FP32 matrix peak
DEV = torch.device("cuda", 0)
HYPER = dict(clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1e-4, entropy_coeff=1e-3, kl_coeff=0.0)   # the launchers' PPO settings
TORCH_ROW_LIMIT = 1 << 20       # rows above which the torch leg is skipped without --torch-full (it keeps every activation)


def mac_floor_flop_per_row(C):
    """The floor the issue names: the gates forward, d [x, h] and d lstm_w, (16 + C) 4C multiply-adds each."""
    return 2.0 * 3 * (16 + C) * 4 * C


def make_seq(policy, agent, M, Q, T, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *shape: torch.rand(shape, generator=g, device=DEV)   # noqa: E731
    n = lambda *shape: torch.randn(shape, generator=g, device=DEV)   # noqa: E731
    seq = {"obs": r(M, Q, 12), "state": 0.5 * n(-(-M // T), Q, 2, policy.cell_size), "logp": -1.0 - r(M, Q), "value": n(M, Q),
           "advantages": n(M, Q), "value_targets": n(M, Q), "starts": (r(M, Q) < 0.01).to(torch.uint8)}
    seq["actions"] = torch.randint(0, 5, (M, Q), generator=g, device=DEV).float() if ws_is_comm(policy.variant, agent) else r(M, Q)
    return seq


def torch_leg(policy, agent, seq, T):
    dist, value = ws_forward_windows(policy, agent, seq["obs"], seq["state"], seq["starts"], T)
    t = {"actions": seq["actions"], "logp_old": seq["logp"], "advantages": seq["advantages"], "value_targets": seq["value_targets"],
         "vf_pred": seq["value"]}
    loss = ws_ppo_terms(dist, value, t, bool(ws_is_comm(policy.variant, agent)), *HYPER.values())[0].mean()
    policy.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach()


def kernel_leg(policy, agent, seq, T):
    loss, _ = ppo_loss_watershed(policy, agent, seq, seq_len=T, **HYPER)
    policy.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach()


def measure(leg, *args):
    """(ms, peak bytes above the start, loss) of one call of leg."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    loss = leg(*args)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated(DEV) - base, float(loss)


def shape_line(what, policy, agent, seq, T, pairs, with_torch):
    M, Q = seq["actions"].shape
    rows = M * Q
    legs = [("kernel", kernel_leg)] + ([("torch", torch_leg)] if with_torch else [])
    ms = {name: [] for name, _ in legs}
    peak, loss = {}, {}
    policy._ppo_scratch = None                                   # the kernel leg's first call allocates it: counted in its peak
    for name, leg in legs:                                       # warm-up: allocator, packed(), code objects
        _, p, _ = measure(leg, policy, agent, seq, T)
        peak[name] = p
    for _ in range(pairs):                                       # alternated: a drift of the box shows in both legs
        for name, leg in legs:
            t, p, ls = measure(leg, policy, agent, seq, T)
            ms[name].append(t)
            peak[name] = max(peak[name], p)
            loss[name] = ls
    line = {"what": what, "agent": agent, "comm": bool(ws_is_comm(policy.variant, agent)), "rows": rows, "pairs": pairs, "seq_len": T,
            "cells": policy.cell_size, "scratch_MiB": round(_capi.SSD_WSPPO_SCRATCH_FLOATS(M, Q, policy.cell_size, T) * 4 / 2 ** 20, 1),
            "mac_floor_flop_per_row": mac_floor_flop_per_row(policy.cell_size)}
    for name, _ in legs:
        line[name + "_ms"] = [round(x, 3) for x in ms[name]]
        line[name + "_ms_median"] = round(statistics.median(ms[name]), 3)
        line[name + "_peak_MiB"] = round(peak[name] / 2 ** 20, 1)
        line[name + "_loss"] = loss[name]
    k = line["kernel_ms_median"]
    line["kernel_us_per_row"] = round(k * 1e3 / rows, 5)
    line["kernel_frac_fp32_peak"] = round(rows * line["mac_floor_flop_per_row"] / (k * 1e-3) / FP32_PEAK, 4)
    if with_torch:
        line["torch_over_kernel"] = round(line["torch_ms_median"] / k, 2)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--seq-len", type=int, default=16)
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--agents", type=int, nargs="+", default=[5, 1], help="agent ids of SeqComm: 0-3 comm agents, 4-7 action agents")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--torch-full", action="store_true", help="run the torch leg on shapes of more than 2^20 rows too")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures the GPU"
    assert args.pairs >= 3, "at least 3 pairs"
    print(label_line("policy_ws_grad_rate %s" % " ".join(sys.argv[1:])), flush=True)
    T = args.seq_len
    policy = WatershedLSTMPolicy(_capi.SSD_WS_SEQ_COMM, cell_size=args.cells, seed=2).to(DEV)
    for Q in args.seqs:
        for agent in args.agents:
            for M, what in ((T, "one window"), (args.steps, "fragment")):
                seq = make_seq(policy, agent, M, Q, T, seed=Q + agent)
                with_torch = args.torch_full or M * Q <= TORCH_ROW_LIMIT
                print(json.dumps(shape_line("%s %d x %d" % (what, M, Q), policy, agent, seq, T, args.pairs, with_torch)), flush=True)
                del seq
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
