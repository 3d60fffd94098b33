"""What the Watershed PPO loss and its gradients cost: ppo_loss_watershed + backward
(ssd_ws_policy_ppo_grad) against the torch path a user had before -- forward_sequence per window, ws_ppo_terms, backward -- in
the same process on the same sequences, for SeqComm with C = 128 and windows of 16 steps: Q = 4096 and 65 536 sequences, an
action id and a comm id, one window (M = 16) and a fragment of 8 windows (M = 128).  The sequences are synthetic (random
observations, states and actions: the cost does not depend on the values).  Device events around each leg, one warm-up of each,
the legs alternated, at least 3 pairs; per leg the peak of torch's allocator above what was allocated before it, and the scratch
the kernel path keeps.  The first line says which library ran (tools/_label.py); then one JSON line per shape.

    python tools/policy_ws_grad_rate.py [--seqs 4096 65536] [--steps 128] [--seq-len 16] [--cells 128] [--agents 5 1] [--pairs 3] [--torch-full]

--loss a3c, per shape three lines: (1) a3c_loss_watershed + backward (ssd_ws_policy_ac_grad) against the
PPO call of the same library, the two kernel legs alternated on their own in both orders (A3C first, then PPO first); (2) the
evaluation: ssd_ws_policy_forward_seq, one launch, against the M + 1 chained launches of ssd_ws_policy_forward it replaces, on
preallocated buffers; (3) impala_loss_watershed + backward against the torch path (forward_sequence per window for the
evaluation and again for the loss, torch terms, backward), with each leg's peak memory.

    python tools/policy_ws_grad_rate.py --loss a3c --seqs 4096 --agents 5 --pairs 3
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sequential_social_dilemma_games_amd import (WatershedLSTMPolicy, _capi, a3c_loss_watershed, impala_loss_watershed,  # noqa: E402
                                                 ppo_loss_watershed, vtrace)
from sequential_social_dilemma_games_amd.policy import (ws_a3c_terms, ws_forward_windows, ws_is_comm, ws_logp,  # noqa: E402
                                                        ws_ppo_terms)
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
    # what the IMPALA call and the evaluation read besides
    seq.update(rew=n(M, Q), done=(r(M, Q) < 0.01).to(torch.uint8), obs_next=r(Q, 12))
    seq["start_next"] = seq["done"][-1].contiguous()
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


A3C_HYPER = dict(vf_loss_coeff=0.5, entropy_coeff=0.01)          # a3c_causal.py's
IMPALA_HYPER = dict(gamma=0.99, clip_rho_threshold=1.0, clip_pg_rho_threshold=1.0, **A3C_HYPER)


def a3c_leg(policy, agent, seq, T):
    loss, _ = a3c_loss_watershed(policy, agent, seq, seq_len=T, **A3C_HYPER)
    policy.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach()


def impala_leg(policy, agent, seq, T):
    loss, _ = impala_loss_watershed(policy, agent, seq, seq_len=T, **IMPALA_HYPER)
    policy.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach()


def impala_torch_leg(policy, agent, seq, T):
    """What a user had: the evaluation through forward_sequence per window under no_grad, V-trace, then the loss's own forward
    under autograd with the torch terms, and backward."""
    comm = bool(ws_is_comm(policy.variant, agent))
    M, Q = seq["actions"].shape
    with torch.no_grad():
        dist, value, last = ws_forward_windows(policy, agent, seq["obs"], seq["state"], seq["starts"], T, return_state=True)
        ag = torch.full((Q,), agent, dtype=torch.int64, device=DEV)
        boot = policy(seq["obs_next"], ag, last, seq["done"][-1].to(torch.bool))[1]
        rhos = torch.exp(ws_logp(dist, seq["actions"], comm) - seq["logp"])
        vs, pg = vtrace(torch.zeros((M, Q), dtype=torch.int32, device=DEV), value.contiguous(), rhos, boot.contiguous(), seq["done"],
                        gamma=0.99, bonus=seq["rew"], bonus_weight=1.0)
    dist, value = ws_forward_windows(policy, agent, seq["obs"], seq["state"], seq["starts"], T)
    loss = ws_a3c_terms(dist, value, dict(seq, advantages=pg, value_targets=vs), comm, *A3C_HYPER.values())[0].sum()
    policy.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach()


class EvalBuffers:
    """Preallocated outputs of both evaluation legs, so that a leg is its launches and nothing else."""

    def __init__(self, policy, M, Q):
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=DEV)   # noqa: E731
        self.dist, self.value, self.logp, self.boot = f(M + 1, Q, 5), f(M + 1, Q), f(M, Q), f(Q)
        self.carry = f(Q, 2, policy.cell_size)
        self.agent = None


def _handles():
    ptr = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())   # noqa: E731
    return ptr, ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def eval_one_launch_leg(policy, agent, seq, T, buf):
    M, Q = seq["actions"].shape
    ptr, stream = _handles()
    _capi.policy_check(_capi.lib().ssd_ws_policy_forward_seq(
        ptr(policy.packed()), policy.num_sets, policy.cell_size, policy.variant, agent, T, ptr(seq["obs"]), ptr(seq["state"]),
        ptr(seq["starts"]), ptr(seq["actions"]), ptr(seq["obs_next"]), ptr(seq["start_next"]), M, Q, ptr(buf.dist), ptr(buf.value),
        ptr(buf.logp), ptr(buf.boot), None, 0, 0, stream))
    return buf.boot[0]


def eval_chained_leg(policy, agent, seq, T, buf):
    """M + 1 launches of ssd_ws_policy_forward by the state rule (no logp: the caller would add a torch expression)."""
    M, Q = seq["actions"].shape
    ptr, stream = _handles()
    if buf.agent is None:
        buf.agent = torch.full((Q,), agent, dtype=torch.int8, device=DEV)
    L, w = _capi.lib(), policy.packed()
    for m in range(M + 1):
        boot = m == M
        if not boot and m % T == 0:
            s_in, starts = seq["state"][m // T], None
        else:
            s_in, starts = buf.carry, (seq["start_next"] if boot else seq["starts"][m])
        obs = seq["obs_next"] if boot else seq["obs"][m]
        _capi.policy_check(L.ssd_ws_policy_forward(ptr(w), policy.num_sets, policy.cell_size, policy.variant, ptr(obs), ptr(buf.agent),
                                                   ptr(s_in), ptr(starts), Q, None if boot else ptr(buf.carry),
                                                   None if boot else ptr(buf.dist[m]), ptr(buf.value[m]), 0, 0, stream))
    return buf.value[M, 0]


def alternate(legs, pairs, *args):
    """One warm-up of each leg, then `pairs` rounds of the legs in the given order -> {name: (ms list, peak bytes, loss)}."""
    out = {name: ([], 0, None) for name, _ in legs}
    for name, leg in legs:
        _, p, _ = measure(leg, *args)
        out[name] = ([], p, None)
    for _ in range(pairs):
        for name, leg in legs:
            t, p, ls = measure(leg, *args)
            ms, peak, _ = out[name]
            out[name] = (ms + [t], max(peak, p), ls)
    return out


def _put(line, name, res):
    ms, peak, loss = res
    line[name + "_ms"] = [round(x, 3) for x in ms]
    line[name + "_ms_median"] = round(statistics.median(ms), 3)
    line[name + "_peak_MiB"] = round(peak / 2 ** 20, 1)
    line[name + "_value"] = loss


def a3c_lines(what, policy, agent, seq, T, pairs, with_torch):
    """The three lines of --loss a3c for one shape."""
    M, Q = seq["actions"].shape
    head = {"what": what, "agent": agent, "comm": bool(ws_is_comm(policy.variant, agent)), "rows": M * Q, "pairs": pairs, "seq_len": T,
            "cells": policy.cell_size}
    line = dict(head, line="a3c against ppo")
    for order, legs in (("a3c_first", [("a3c", a3c_leg), ("ppo", kernel_leg)]), ("ppo_first", [("ppo", kernel_leg), ("a3c", a3c_leg)])):
        res = alternate(legs, pairs, policy, agent, seq, T)
        for name in ("a3c", "ppo"):
            _put(line, "%s_%s" % (order, name), res[name])
        line[order + "_a3c_over_ppo"] = round(line[order + "_a3c_ms_median"] / line[order + "_ppo_ms_median"], 4)
    yield line
    buf = EvalBuffers(policy, M, Q)
    line = dict(head, line="evaluation: one launch against %d chained" % (M + 1))
    res = alternate([("one_launch", eval_one_launch_leg), ("chained", eval_chained_leg)], pairs, policy, agent, seq, T, buf)
    _put(line, "one_launch", res["one_launch"])
    _put(line, "chained", res["chained"])
    line["chained_over_one_launch"] = round(line["chained_ms_median"] / line["one_launch_ms_median"], 2)
    yield line
    del buf
    line = dict(head, line="impala against torch")
    legs = [("impala", impala_leg)] + ([("torch", impala_torch_leg)] if with_torch else [])
    policy._ppo_scratch = None                                   # the kernel leg's first call allocates it: counted in its peak
    res = alternate(legs, pairs, policy, agent, seq, T)
    for name, _ in legs:
        _put(line, name, res[name])
    if with_torch:
        line["torch_over_impala"] = round(line["torch_ms_median"] / line["impala_ms_median"], 2)
    yield line


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
    ap.add_argument("--loss", choices=("ppo", "a3c"), default="ppo", help="a3c: the A3C call against the PPO call, the evaluation legs and the IMPALA call")
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
                if args.loss == "a3c":
                    for line in a3c_lines("%s %d x %d" % (what, M, Q), policy, agent, seq, T, args.pairs, with_torch):
                        print(json.dumps(line), flush=True)
                else:
                    print(json.dumps(shape_line("%s %d x %d" % (what, M, Q), policy, agent, seq, T, args.pairs, with_torch)), flush=True)
                del seq
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
