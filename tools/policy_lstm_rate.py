"""What a recurrent policy rollout costs: the trunk kernel (features mode) and the LSTM kernel alone (µs,
and the LSTM kernel's share of the FP32 peak by the FLOP count of its matrix work), VecEngine.rollout_policy with a
ConvLSTMPolicy per step (greedy and sampled), the torch-eager loop a user would write (VecEngine.step + ConvLSTMPolicy.forward +
softmax + torch.multinomial) per step, and the ConvFCPolicy rollout per step for comparison.  Harvest 16x38 and Cleanup 25x18,
4096 envs x 5 agents, one weight set per agent, C = 128 and 256.  Device events around work that ends in a synchronise.  One
JSON line.

    python tools/policy_lstm_rate.py [--steps 64] [--reps 5] [--quick]
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
from sequential_social_dilemma_games_amd.policy import ConvFCPolicy, ConvLSTMPolicy  # noqa: E402

FP32_PEAK = 157.3e12            # MI355X_MICROARCH.md: FP32 vector = FP32 matrix peak
DEV = torch.device("cuda", 0)


def lstm_flop_per_row(Cs):
    """2 x the multiply-adds of the cell's matrix product: [x, h] (32 + C) x 4C."""
    return 2 * (32 + Cs) * 4 * Cs


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
    z = lambda shape, dt: torch.empty(shape, dtype=dt, device=DEV)   # noqa: E731
    return {"obs": z((steps, E, N, 15, 15, 3), torch.uint8), "actions": z((steps, E, N), torch.int32),
            "logp": z((steps, E, N), torch.float32), "value": z((steps, E, N), torch.float32),
            "rew": z((steps, E, N), torch.int32), "done": z((steps, E, N), torch.uint8)}


def measure(name, game, E, N, Cs, steps, reps, with_ff):
    eng = VecEngine(game, None, num_envs=E, num_agents=N, seed=1)
    eng.set_horizon(1000)
    obs0 = eng.reset()
    A = eng.num_actions
    pol = ConvLSTMPolicy(A, N, Cs, seed=2).to(DEV)
    w = pol.packed()
    L, stream = _capi.lib(), eng._stream()
    dp = lambda t: C.c_void_p(t.data_ptr())                                # noqa: E731
    state = torch.zeros((E, N, 2, Cs), dtype=torch.float32, device=DEV)
    feat = torch.empty((E, N, 32), dtype=torch.float32, device=DEV)
    logits = torch.empty((E, N, A), dtype=torch.float32, device=DEV)
    value = torch.empty((E, N), dtype=torch.float32, device=DEV)
    # the forward: trunk (features mode) + cell, ssd_policy_lstm_forward; the trunk alone is what ssd_policy_forward runs less its
    # heads (1 % of it), so the cell's time is the difference.  rocprofv3 --kernel-trace --stats splits the two kernels exactly.
    args = (dp(w), N, A, Cs, dp(obs0), dp(state), None, E, N, dp(feat), dp(state), dp(logits), dp(value), 0, 0)
    fwd_us = timed(lambda: _capi.policy_check(L.ssd_policy_lstm_forward(*args, stream)), reps * 20)
    ff = ConvFCPolicy(A, N, seed=2).to(DEV)
    wf = ff.packed()
    fargs = (dp(wf), N, A, dp(obs0), E, N, dp(logits), dp(value), 0, 0)
    trunk_us = timed(lambda: _capi.policy_check(L.ssd_policy_forward(*fargs, stream)), reps * 20)
    out = {"config": name, "E": E, "N": N, "A": A, "P": N, "C": Cs, "forward_us": round(fwd_us, 2), "trunk_us": round(trunk_us, 2),
           "lstm_us": round(fwd_us - trunk_us, 2)}
    flop = lstm_flop_per_row(Cs) * E * N
    out["lstm_gflop"] = round(flop / 1e9, 3)
    out["lstm_frac_fp32_peak"] = round(flop / (max(fwd_us - trunk_us, 1e-3) * 1e-6) / FP32_PEAK, 3)
    r = rings(E, N, steps)
    last_value = torch.empty((E, N), dtype=torch.float32, device=DEV)
    cur = obs0.clone()
    for greedy in (True, False):
        def call(greedy=greedy):
            eng.rollout_policy(pol, cur, steps, r["obs"], actions=r["actions"], logp=r["logp"], value=r["value"], rew=r["rew"],
                               done=r["done"], last_value=last_value, greedy=greedy, state=state)
            cur.copy_(r["obs"][steps - 1])
        out["rollout_%s_us_per_step" % ("greedy" if greedy else "sampled")] = round(timed(call, reps) / steps, 2)
    # the torch-eager loop: step, forward with the state carried, softmax, multinomial
    acts = torch.zeros((E, N), dtype=torch.int32, device=DEV)
    outs = eng.alloc_outputs()
    st = [torch.zeros((E, N, 2, Cs), dtype=torch.float32, device=DEV)]

    def eager():
        obs, rew, done = eng.step(acts, out=outs, auto_reset=True)
        with torch.no_grad():
            lg, v, st[0] = pol(obs, st[0], done.bool())
            a = torch.multinomial(torch.softmax(lg.reshape(-1, A), -1), 1)
        acts.copy_(a.view(E, N))
    out["torch_eager_us_per_step"] = round(timed(eager, steps), 2)
    out["rollout_sampled_vs_eager"] = round(out["torch_eager_us_per_step"] / out["rollout_sampled_us_per_step"], 2)
    if with_ff:
        def ffcall():
            eng.rollout_policy(ff, cur, steps, r["obs"], actions=r["actions"], logp=r["logp"], value=r["value"], rew=r["rew"],
                               done=r["done"], last_value=last_value)
            cur.copy_(r["obs"][steps - 1])
        out["ff_rollout_sampled_us_per_step"] = round(timed(ffcall, reps) / steps, 2)
    assert eng.status() == 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="one configuration, few repetitions (for a profiler run)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures the GPU"
    configs = [("harvest_16x38", K.GAME_HARVEST, 4096, 5, 128, True), ("harvest_16x38", K.GAME_HARVEST, 4096, 5, 256, False),
               ("cleanup_25x18", K.GAME_CLEANUP, 4096, 5, 128, True), ("cleanup_25x18", K.GAME_CLEANUP, 4096, 5, 256, False)]
    if args.quick:
        configs, args.reps, args.steps = configs[:2], 2, 16
    rows = [measure(n, g, E, N, Cs, steps=args.steps, reps=args.reps, with_ff=ff) for n, g, E, N, Cs, ff in configs]
    print(json.dumps({"label": label_line("policy_lstm_rate.py"), "results": rows}), flush=True)


if __name__ == "__main__":
    main()
