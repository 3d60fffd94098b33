"""What V-trace and the IMPALA calls cost.

The kernel: ssd_vtrace (with done) and ssd_advantages (GAE with done) in one process, legs alternating, device events around
`--reps` calls after warm-up, `--runs` runs each, at L = 20 480 x K = 128, L = 20 480 x K = 1000 and L = 163 840 x K = 1000,
with each leg's bytes (21 a row against 17) as a fraction of 6.3 TB/s and the ratio of the medians.

The calls (--calls): impala_loss* + backward against a3c_loss* + backward of the same policy on one sampled Harvest fragment
(4096 envs x 5 agents, K = 128, C = 128, T = 16), legs alternating, `--pairs` calls each, and the parts of the difference on their
own: evaluate_fragment, the three torch ops (log-softmax, gather, exp of the difference) and the scan.  --torch: one call of
the CPU-path code (the modules' forwards, a3c_terms under autograd) on the device, last.

    python tools/vtrace_rate.py [--reps 200] [--runs 2] [--calls] [--kinds fc,lstm,moa] [--pairs 3] [--torch]

The load-block length of the kernel is a compile-time constant: for another one, `make -C sequential_social_dilemma_games_amd/csrc
exp EXP=-DSSD_VTRACE_LOAD_BLOCK=n`, then run this with SSD_LIB_PATH=.../libssd_hip_exp.so.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sequential_social_dilemma_games_amd import (ConvFCPolicy, ConvLSTMPolicy, ConvMOAPolicy, a3c_loss, a3c_loss_moa,  # noqa: E402
                                                 a3c_loss_recurrent, compute_advantages, evaluate_fragment, impala_loss,
                                                 impala_loss_moa, impala_loss_recurrent, vtrace)
from sequential_social_dilemma_games_amd import constants as K  # noqa: E402
from sequential_social_dilemma_games_amd import policy as P  # noqa: E402
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv  # noqa: E402

HBM_BPS = 6.3e12
DEV = torch.device("cuda", 0)
HYPER = dict(vf_loss_coeff=0.5, entropy_coeff=0.01)


def timed(fn, reps, warm=2):
    """Mean µs per call of fn over reps calls (after warm-up calls), by device events."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernel_rates(L, steps, reps, runs):
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    rew = torch.randint(-2, 2, (steps, L), device=DEV, generator=g, dtype=torch.int32)
    value = torch.randn((steps, L), device=DEV, generator=g)
    rhos = torch.exp(torch.randn((steps, L), device=DEV, generator=g))
    done = (torch.rand((steps, L), device=DEV, generator=g) < 0.001).to(torch.uint8)
    last = torch.randn((L,), device=DEV, generator=g)
    out = (torch.empty_like(value), torch.empty_like(value))
    legs = {"vtrace": lambda: vtrace(rew, value, rhos, last, done, gamma=0.99, out=out),
            "gae": lambda: compute_advantages(rew, value, last, done, gamma=0.99, lambda_=0.95, out=out)}
    us = {name: [] for name in legs}
    for _ in range(runs):
        for name, fn in legs.items():
            us[name].append(round(timed(fn, reps), 2))
    rows = steps * L
    line = {"what": "ssd_vtrace against ssd_advantages (GAE), both with done", "L": L, "K": steps, "reps": reps}
    for name, per_row in (("vtrace", 21), ("gae", 17)):
        med = statistics.median(us[name])
        line[name + "_us"] = us[name]
        line[name + "_frac_of_6.3TBps"] = round(rows * per_row / (med * 1e-6) / HBM_BPS, 4)
    line["vtrace_over_gae"] = round(statistics.median(us["vtrace"]) / statistics.median(us["gae"]), 4)
    line["byte_ratio"] = round(21 / 17, 4)
    return line


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def call_rates(kind, envs, steps, T, cells, pairs, with_torch):
    N = 5
    env = SSDVectorEnv(K.GAME_HARVEST, envs, N, horizon=1000, seed=1)
    A = env.engine.num_actions
    pol = (ConvFCPolicy(A, N, seed=2) if kind == "fc" else ConvLSTMPolicy(A, N, cells, seed=2) if kind == "lstm" else
           ConvMOAPolicy(A, N, N, cells, seed=2)).to(DEV)
    first = env.reset().clone()
    kw = {} if kind == "fc" else {"state_every": T}
    batch = env.sample(pol, steps, gamma=0.99, use_gae=False, **kw)
    seq = {} if kind == "fc" else {"seq_len": T}
    moa = {"moa_weight": 10.0} if kind == "moa" else {}
    a3c = {"fc": a3c_loss, "lstm": a3c_loss_recurrent, "moa": a3c_loss_moa}[kind]
    imp = {"fc": impala_loss, "lstm": impala_loss_recurrent, "moa": impala_loss_moa}[kind]

    def leg(fn, **more):
        pol.zero_grad()
        loss, _ = fn(pol, batch, obs_first=first, **seq, **moa, **HYPER, **more)
        loss.backward()

    legs = {"impala": lambda: leg(imp, gamma=0.99), "a3c": lambda: leg(a3c)}
    for fn in legs.values():                                     # warm-up: scratch allocations, first launches
        fn()
    ms = {name: [] for name in legs}
    for _ in range(pairs):
        for name, fn in legs.items():
            ms[name].append(round(wall_ms(fn), 3))
    logits, value, boot = evaluate_fragment(pol, batch, first, T)
    acts = batch["actions"].long().unsqueeze(-1)

    def ops():
        return torch.exp(torch.log_softmax(logits, -1).gather(-1, acts).squeeze(-1) - batch["logp"])

    rhos = ops()
    parts = {"evaluate_ms": [round(wall_ms(lambda: evaluate_fragment(pol, batch, first, T)), 3) for _ in range(pairs)],
             "torch_ops_ms": [round(wall_ms(ops), 3) for _ in range(pairs)],
             "scan_ms": [round(wall_ms(lambda: vtrace(batch["rew"], value, rhos, boot, batch["done"], gamma=0.99)), 3)
                         for _ in range(pairs)]}
    line = {"what": "impala_loss + backward against a3c_loss + backward", "kind": kind, "E": envs, "N": N, "K": steps, "T": T,
            "C": cells if kind != "fc" else None, "impala_ms": ms["impala"], "a3c_ms": ms["a3c"]}
    line["difference_ms"] = round(statistics.median(ms["impala"]) - statistics.median(ms["a3c"]), 3)
    line.update(parts)
    line["evaluate_share_of_call"] = round(statistics.median(parts["evaluate_ms"]) / statistics.median(ms["impala"]), 4)
    if with_torch:
        def torch_leg():
            pol.zero_grad()
            t, dims, T_ = P._fragment_tensors(pol, batch, first, None if kind == "fc" else T)
            with torch.no_grad():
                lg, v, b = P._evaluate_host(pol, t, dims, T_)
                r = torch.exp(torch.log_softmax(lg, -1).gather(-1, acts).squeeze(-1) - batch["logp"])
                vs, pg = vtrace(batch["rew"], v.contiguous(), r, b.contiguous(), batch["done"], gamma=0.99)
            t.update(advantages=pg, value_targets=vs)
            lg, v, _ = P._evaluate_host(pol, t, dims, T_)
            P._set_sums(P.a3c_terms(lg, v, t, *HYPER.values())[0], pol.num_sets).sum().backward()
        line["torch_path_on_device_ms"] = round(wall_ms(torch_leg), 1)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--calls", action="store_true", help="the impala_loss* calls against the a3c_loss* calls, and their parts")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--kinds", default="fc,lstm,moa")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--seq-len", type=int, default=16)
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--torch", action="store_true", help="one call of the CPU-path code on the device, last (the MOA term is left out)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures the GPU"
    if args.calls:                                               # first: a rollout comes before the process's first streams
        for kind in args.kinds.split(","):
            print(json.dumps(call_rates(kind, args.envs, args.steps, args.seq_len, args.cells, args.pairs, args.torch)), flush=True)
    if not args.skip_kernel:
        for L, steps in ((20480, 128), (20480, 1000), (163840, 1000)):
            print(json.dumps(kernel_rates(L, steps, args.reps, args.runs)), flush=True)


if __name__ == "__main__":
    main()
