#!/usr/bin/env python3
"""Watershed throughput on one device: one JSON line.

    python tools/watershed_rate.py [--reference DIR] [--no-gpu]

* us per phase-step through ssd_ws_step (one launch per phase) and through ssd_ws_rollout_actions (K = 131 phases per launch,
  the state in registers), for WatershedSeqEnv and WatershedSeqCommEnv at E = 4096, 65536 and 1048576 envs (CUDA-event timed,
  median of the timed repetitions, after warm-up);
* the bytes a rollout phase-step moves per env (action in; observation, agent, reward, done out; the state's load and store
  amortised over the K phases) and the fraction of 8 TB/s that makes at the measured rate;
* with --reference DIR (a checkout of the reference): its WatershedSeqEnv dict steps per second on one CPU core.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K_ROLLOUT = 131
HBM = 8.0e12
STREAM_BYTES = 4 + 48 + 1 + 8 + 1                    # action f32, obs f32 x 12, agent i8, reward f64, done u8
STATE_BYTES = {0: 4 + 4 + 4 + 16 + 24 + 4 + 64 + 16, 1: 4 + 4 + 4 + 32 + 24 + 4 + 64 + 16}   # u8 x 4, i32, u32, hist, f_rew, pen, f64 x 8, prev


def gpu_rates(variant, E, reps):
    import torch
    from sequential_social_dilemma_games_amd import WatershedVecEngine
    eng = WatershedVecEngine(variant, E, seed=1)
    eng.reset()
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    acts = torch.randint(0, 2, (K_ROLLOUT, E), device="cuda", generator=g).float()   # 0 / 1: valid messages and withdrawals alike
    out1 = eng._outputs()
    outK = eng._outputs((K_ROLLOUT,))

    def timed(fn, n):
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3 / n)
        return statistics.median(ts)

    k = [0]

    def one_step():
        eng.step(acts[k[0] % K_ROLLOUT], auto_reset=True, out=out1)
        k[0] += 1

    def rollout():
        eng.rollout_actions(acts, K_ROLLOUT, *outK, auto_reset=True)

    for _ in range(3):
        rollout()
        one_step()
    torch.cuda.synchronize()
    step_us = timed(one_step, 64)
    roll_us = timed(rollout, 4) / K_ROLLOUT
    status = eng.status()
    eng.close()
    per_env = STREAM_BYTES + 2.0 * STATE_BYTES[variant] / K_ROLLOUT
    return {"step_us": round(step_us, 3), "rollout_us_per_step": round(roll_us, 3),
            "rollout_bytes_per_env_step": round(per_env, 2),
            "rollout_hbm_fraction": round(per_env * E / (roll_us * 1e-6) / HBM, 3), "status": status}


def reference_rate(ref_dir, seconds=3.0):
    """WatershedSeqEnv of the reference, dict API, one core (the stand-ins of tests/golden/gen_golden_watershed.py)."""
    import numpy as np
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import gen_golden_watershed as gen
    gen.REFERENCE = ref_dir
    W = gen.import_reference()
    env = W.WatershedSeqEnv()
    rng = np.random.default_rng(0)
    acts = rng.random(4096).astype(np.float32)
    n, t0 = 0, time.perf_counter()
    obs = env.reset()
    while time.perf_counter() - t0 < seconds:
        aid = next(iter(obs))
        obs, rew, done, info = env.step({aid: acts[n % 4096:n % 4096 + 1]})
        n += 1
        if done["__all__"]:
            obs = env.reset()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="reference checkout: also time its dict steps on one core")
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    out = {"metric": "watershed_rate", "k_rollout": K_ROLLOUT}
    if not args.no_gpu:
        for variant, name in ((0, "seq"), (1, "seqcomm")):
            for E in (4096, 65536, 1 << 20):
                out["%s_E%d" % (name, E)] = gpu_rates(variant, E, args.reps)
    if args.reference:
        out["reference_dict_steps_per_s_one_core"] = round(reference_rate(args.reference), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
