"""What a MOA policy rollout costs: ssd_policy_moa_forward (trunk in MOA mode, actions cell, MOA cell
with the counterfactuals and the influence) per call, and the MOA cell's share of the FP32 peak by the FLOP count of its matrix
work; VecEngine.rollout_policy with a ConvMOAPolicy per step (greedy and sampled); and the torch-eager loop a user would write
(VecEngine.step + ConvMOAPolicy.forward + torch.multinomial + influence()) per step.  Harvest 16x38 and Cleanup 25x18, 4096
envs x 5 agents, one weight set per agent, C = 128.  Each kernel alone: run this under rocprofv3 --kernel-trace --stats
(--quick keeps that run short).  Device events around work that ends in a synchronise.  One JSON line.

    python tools/policy_moa_rate.py [--steps 32] [--reps 5] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools._label import label_line  # noqa: E402
from sequential_social_dilemma_games_amd import _capi  # noqa: E402
from sequential_social_dilemma_games_amd import constants as K  # noqa: E402
from sequential_social_dilemma_games_amd.engine import VecEngine  # noqa: E402
from sequential_social_dilemma_games_amd.policy import ConvMOAPolicy, influence  # noqa: E402

FP32_PEAK = 157.3e12            # MI355X_MICROARCH.md: FP32 vector = FP32 matrix peak
DEV = torch.device("cuda", 0)


def flop_per_row(Cs, A, N):
    """2 x the multiply-adds per agent-env: both FC stacks, the actions gates, the MOA gates, A predictions."""
    return 2 * (2 * (1014 * 32 + 32 * 32) + (32 + Cs) * 4 * Cs + (48 + Cs) * 4 * Cs + A * Cs * (N - 1) * A)


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


def measure(name, game, E, N, Cs, steps, reps):
    eng = VecEngine(game, None, num_envs=E, num_agents=N, seed=1)
    eng.set_horizon(1000)
    obs0 = eng.reset()
    A = eng.num_actions
    pol = ConvMOAPolicy(A, N, N, Cs, seed=2).to(DEV)
    w = pol.packed()
    L, stream = _capi.lib(), eng._stream()
    dp = lambda t: C.c_void_p(t.data_ptr())                                # noqa: E731
    e = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=DEV)  # noqa: E731
    state, prev = e(E, N, 4, Cs), torch.zeros((E, N), dtype=torch.int32, device=DEV)
    scratch, logits, value, moa, infl = e(_capi.SSD_MOA_SCRATCH_FLOATS(E * N)), e(E, N, A), e(E, N), e(E, N, N - 1, A), e(E, N)
    args = (dp(w), N, A, Cs, dp(obs0), dp(prev), dp(state), None, E, N, dp(scratch), dp(state), dp(logits), dp(value), dp(moa),
            None, dp(prev), dp(infl), C.c_float(10.0), 0, 0)
    fwd_us = timed(lambda: _capi.policy_check(L.ssd_policy_moa_forward(*args, stream)), reps * 10)
    flop = flop_per_row(Cs, A, N) * E * N
    out = {"config": name, "E": E, "N": N, "A": A, "P": N, "C": Cs, "forward_us": round(fwd_us, 2),
           "gflop_per_step": round(flop / 1e9, 3), "forward_frac_fp32_peak": round(flop / (fwd_us * 1e-6) / FP32_PEAK, 3)}
    z = lambda shape, dt: torch.empty(shape, dtype=dt, device=DEV)         # noqa: E731
    r = {"obs": z((steps, E, N, 15, 15, 3), torch.uint8), "actions": z((steps, E, N), torch.int32),
         "logp": z((steps, E, N), torch.float32), "value": z((steps, E, N), torch.float32), "rew": z((steps, E, N), torch.int32),
         "done": z((steps, E, N), torch.uint8), "influence": z((steps, E, N), torch.float32)}
    last_value = e(E, N)
    cur = obs0.clone()
    for greedy in (True, False):
        def call(greedy=greedy):
            eng.rollout_policy(pol, cur, steps, r["obs"], actions=r["actions"], logp=r["logp"], value=r["value"], rew=r["rew"],
                               done=r["done"], last_value=last_value, greedy=greedy, state=state, prev_actions=prev,
                               influence=r["influence"])
            cur.copy_(r["obs"][steps - 1])
        out["rollout_%s_us_per_step" % ("greedy" if greedy else "sampled")] = round(timed(call, reps) / steps, 2)
    # the torch-eager loop: step, forward with the state and the previous joint action carried, multinomial, influence
    acts = torch.zeros((E, N), dtype=torch.int32, device=DEV)
    outs = eng.alloc_outputs()
    carry = [e(E, N, 4, Cs), torch.zeros((E, N), dtype=torch.int32, device=DEV), obs0.clone(), torch.zeros((E, N), dtype=torch.bool, device=DEV)]

    def eager():
        with torch.no_grad():
            lg, v, m, cf, carry[0] = pol(carry[2], carry[1], carry[0], carry[3])
            a = torch.multinomial(torch.softmax(lg.reshape(-1, A), -1), 1).view(E, N)
            influence(lg, cf, a, 10.0)
        acts.copy_(a)
        obs, rew, done = eng.step(acts, out=outs, auto_reset=True)
        carry[1], carry[2], carry[3] = acts.clone(), obs, done.bool()
    out["torch_eager_us_per_step"] = round(timed(eager, max(steps // 4, 2)), 2)
    out["rollout_sampled_vs_eager"] = round(out["torch_eager_us_per_step"] / out["rollout_sampled_us_per_step"], 2)
    assert eng.status() == 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="one configuration, few repetitions (for a profiler run)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures the GPU"
    configs = [("harvest_16x38", K.GAME_HARVEST, 4096, 5, 128), ("cleanup_25x18", K.GAME_CLEANUP, 4096, 5, 128)]
    if args.quick:
        configs, args.reps, args.steps = configs[:1], 2, 8
    rows = [measure(n, g, E, N, Cs, steps=args.steps, reps=args.reps) for n, g, E, N, Cs in configs]
    print(json.dumps({"label": label_line("policy_moa_rate.py"), "results": rows}), flush=True)


if __name__ == "__main__":
    main()
