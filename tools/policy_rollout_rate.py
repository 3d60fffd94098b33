"""What a closed-loop policy rollout costs: the forward kernel alone (µs and its share of the FP32 peak by
the FLOP count of the network), VecEngine.rollout_policy per step (greedy and sampled), the torch-eager loop a user would write
(VecEngine.step + ConvFCPolicy + softmax + torch.multinomial) per step, and the env step alone.  Device events around work that
ends in a synchronise.  One JSON line.

    python tools/policy_rollout_rate.py [--steps 64] [--reps 5] [--quick]
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
from sequential_social_dilemma_games_amd.policy import ConvFCPolicy  # noqa: E402

FP32_PEAK = 157.3e12            # MI355X_MICROARCH.md: FP32 vector = FP32 matrix peak
DEV = torch.device("cuda", 0)


def flop_per_agent_step(A):
    """2 x the multiply-adds of the network: conv 13*13*6*27, fc1 1014*32, fc2 32*32, logits 32*A, value 32."""
    return 2 * (13 * 13 * 6 * 27 + 1014 * 32 + 32 * 32 + 32 * A + 32)


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


def measure(name, game, amap, E, N, steps, reps):
    eng = VecEngine(game, amap, num_envs=E, num_agents=N, seed=1)
    eng.set_horizon(1000)
    obs0 = eng.reset()
    A = eng.num_actions
    pol = ConvFCPolicy(A, N, seed=2).to(DEV)
    # forward kernel alone: the C call on packed weights (no repacking)
    w = pol.packed()
    logits = torch.empty((E, N, A), dtype=torch.float32, device=DEV)
    value = torch.empty((E, N), dtype=torch.float32, device=DEV)
    L, stream = _capi.lib(), eng._stream()
    args = (C.c_void_p(w.data_ptr()), N, A, C.c_void_p(obs0.data_ptr()), E, N, C.c_void_p(logits.data_ptr()), C.c_void_p(value.data_ptr()), 0, 0)
    fwd_us = timed(lambda: _capi.policy_check(L.ssd_policy_forward(*args, stream)), reps * 20)
    flop = flop_per_agent_step(A) * E * N
    out = {"config": name, "E": E, "N": N, "A": A, "P": N, "forward_us": round(fwd_us, 2),
           "forward_gflop": round(flop / 1e9, 3), "forward_frac_fp32_peak": round(flop / (fwd_us * 1e-6) / FP32_PEAK, 3)}
    # rollout_policy: K steps per call into rings of K slots
    ring = {"obs": torch.empty((steps, E, N, 15, 15, 3), dtype=torch.uint8, device=DEV),
            "actions": torch.empty((steps, E, N), dtype=torch.int32, device=DEV),
            "logp": torch.empty((steps, E, N), dtype=torch.float32, device=DEV),
            "value": torch.empty((steps, E, N), dtype=torch.float32, device=DEV),
            "rew": torch.empty((steps, E, N), dtype=torch.int32, device=DEV),
            "done": torch.empty((steps, E, N), dtype=torch.uint8, device=DEV)}
    last_value = torch.empty((E, N), dtype=torch.float32, device=DEV)
    cur = obs0.clone()
    for greedy in (True, False):
        def call(greedy=greedy):
            eng.rollout_policy(pol, cur, steps, ring["obs"], actions=ring["actions"], logp=ring["logp"], value=ring["value"],
                               rew=ring["rew"], done=ring["done"], last_value=last_value, greedy=greedy)
            cur.copy_(ring["obs"][steps - 1])
        out["rollout_%s_us_per_step" % ("greedy" if greedy else "sampled")] = round(timed(call, reps) / steps, 2)
    # the torch-eager loop: step, forward, softmax, multinomial
    acts = torch.zeros((E, N), dtype=torch.int32, device=DEV)
    outs = eng.alloc_outputs()

    def eager():
        obs, rew, done = eng.step(acts, out=outs, auto_reset=True)
        with torch.no_grad():
            lg, v = pol(obs)
            a = torch.multinomial(torch.softmax(lg.reshape(-1, A), -1), 1)
        acts.copy_(a.view(E, N))
    out["torch_eager_us_per_step"] = round(timed(eager, steps), 2)
    out["env_step_us"] = round(timed(lambda: eng.step(acts, out=outs, auto_reset=True), steps * 4), 2)
    out["rollout_sampled_vs_eager"] = round(out["torch_eager_us_per_step"] / out["rollout_sampled_us_per_step"], 2)
    assert eng.status() == 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="one configuration, few repetitions (for a profiler run)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures the GPU"
    configs = [("harvest_16x38", K.GAME_HARVEST, None, 4096, 5), ("cleanup_25x18", K.GAME_CLEANUP, None, 4096, 5),
               ("harvest_16x38_2agents", K.GAME_HARVEST, None, 4096, 2)]
    if args.quick:
        configs, args.reps, args.steps = configs[:1], 2, 16
    rows = [measure(*c, steps=args.steps, reps=args.reps) for c in configs]
    print(json.dumps({"label": label_line("policy_rollout_rate.py"), "results": rows}), flush=True)


if __name__ == "__main__":
    main()
