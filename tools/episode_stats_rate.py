"""What the episode statistics cost: the fold alone, the adapter's tracking per step, and a fused
1000-step rollout (rewards only: the outputs of one call share one ring) with and without stats=.  Device events around work that ends in a synchronise; one JSON line per figure.

    python tools/episode_stats_rate.py [--reps 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sequential_social_dilemma_games_amd import constants as K  # noqa: E402
from sequential_social_dilemma_games_amd.engine import VecEngine  # noqa: E402
from sequential_social_dilemma_games_amd.episode_stats import EpisodeStats  # noqa: E402
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


def fold_rate(E, N, K_steps, reps):
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    rew = (torch.randint(-2, 2, (K_steps, E, N), device=DEV, generator=g, dtype=torch.int32) * 1)
    rew[rew == -2] = -50
    st = EpisodeStats(E, N)
    us = timed(lambda: st.fold(rew, None, step0=0, n_steps=K_steps, reset_every=K_steps), reps)
    read = K_steps * E * N * 4
    return {"what": "fold", "E": E, "N": N, "K": K_steps, "us": round(us, 2), "rew_bytes": read,
            "frac_of_6.3TBps": round(read / (us * 1e-6) / HBM_BPS, 3)}


def adapter_rate(E, N, steps, track):
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=1000, seed=1, track_episodes=track)
    env.reset()
    us = timed(env.step_random, steps)
    if track:
        env.summary()
    return {"what": "SSDVectorEnv.step_random", "E": E, "N": N, "track_episodes": track, "us_per_step": round(us, 2)}


def rollout_rate(E, N, reps, with_stats):
    eng = VecEngine(K.GAME_HARVEST, None, num_envs=E, num_agents=N, seed=2)
    eng.reset()
    rew = torch.empty((1000, E, N), dtype=torch.int32, device=DEV)   # (outputs share one ring: obs is left out)
    st = EpisodeStats(E, N) if with_stats else None
    us = timed(lambda: eng.rollout_random(1000, None, rew, None, reset_every=1000, step0=0, fused=True, stats=st), reps)
    return {"what": "rollout_random fused 1000 steps", "E": E, "N": N, "stats": with_stats, "us": round(us, 1),
            "path": eng.rollout_path()["fused"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--adapter-steps", type=int, default=2000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures the GPU"
    lines = [lambda: fold_rate(4096, 5, 1000, args.reps), lambda: fold_rate(32768, 5, 1000, args.reps)]
    for track in (False, True, False, True):                     # alternated: the spread shows in the repeat
        lines.append(lambda track=track: adapter_rate(4096, 5, args.adapter_steps, track))
    for with_stats in (False, True, False, True):
        lines.append(lambda with_stats=with_stats: rollout_rate(4096, 5, max(args.reps // 4, 3), with_stats))
    for ln in lines:
        print(json.dumps(ln()), flush=True)


if __name__ == "__main__":
    main()
