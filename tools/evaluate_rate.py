"""What evaluate_fragment costs for the two recurrent gridworld policies: the K + 1 chained per-step
forwards (one_call=False) against the sequence forward's one call (one_call=True), on Harvest's shape 4096 envs x 5 agents,
C = 128, T = 16, at K = 16 and K = 128, on seeded random fragments.  Device events around `reps` calls that end in a
synchronise; the arms alternate within one process -- chained, one call, chained again -- for `rounds` rounds, and a line gives
each arm's median over the rounds.  The two chained arms run the same code: the distance between their medians is the spread
of this visit, and the one call counts as faster only where its median beats the chained one's by more than that.  One JSON
line per (policy, K); the outputs of the two paths are compared bit for bit first.

    python tools/evaluate_rate.py [--rounds 7] [--reps 3] [--envs 4096] [--steps 16 128]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sequential_social_dilemma_games_amd import ConvLSTMPolicy, ConvMOAPolicy, evaluate_fragment  # noqa: E402

DEV = torch.device("cuda", 0)
A, N, C, T = 8, 5, 128, 16


def fragment(kind, pol, steps, E):
    """A seeded random fragment of `steps` steps with every key evaluate_fragment reads -> (batch, obs_first)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(steps)
    S = -(-steps // T)
    t = {"obs": torch.randint(0, 256, (steps, E, N, 15, 15, 3), device=DEV, generator=g, dtype=torch.uint8),
         "actions": torch.randint(0, A, (steps, E, N), device=DEV, generator=g, dtype=torch.int32),
         "state": 0.5 * torch.randn((S, E, N, pol.STATE_ROWS, C), device=DEV, generator=g),
         "done": (torch.rand((steps, E, N), device=DEV, generator=g) < 0.001).to(torch.uint8)}
    if kind == "moa":
        t["prev_actions"] = torch.randint(0, A, (steps, E, N), device=DEV, generator=g, dtype=torch.int32)
    first = torch.randint(0, 256, (E, N, 15, 15, 3), device=DEV, generator=g, dtype=torch.uint8)
    return t, first


def timed(fn, reps):
    """Mean ms per call of fn over reps calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def rate(kind, steps, E, rounds, reps):
    pol = ConvLSTMPolicy(A, num_sets=N, cell_size=C, seed=3) if kind == "lstm" else ConvMOAPolicy(A, N, num_sets=N, cell_size=C, seed=3)
    pol = pol.to(DEV)
    t, first = fragment(kind, pol, steps, E)
    chained = lambda: evaluate_fragment(pol, t, first, T, one_call=False)   # noqa: E731
    one = lambda: evaluate_fragment(pol, t, first, T, one_call=True)        # noqa: E731
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(chained(), one()))   # (and the warm-up)
    chained(), one()
    torch.cuda.synchronize()
    ms = {"chained": [], "one_call": [], "chained_again": []}
    for _ in range(rounds):
        for name, fn in (("chained", chained), ("one_call", one), ("chained_again", chained)):
            ms[name].append(timed(fn, reps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    base = min(med["chained"], med["chained_again"])
    spread = abs(med["chained"] - med["chained_again"]) / base
    gain = 1.0 - med["one_call"] / base
    return {"what": "evaluate_fragment", "policy": kind, "E": E, "N": N, "C": C, "T": T, "K": steps, "equal_bits": bool(same),
            "chained_ms": round(med["chained"], 3), "chained_again_ms": round(med["chained_again"], 3),
            "one_call_ms": round(med["one_call"], 3), "min_ms": {k: round(min(v), 3) for k, v in ms.items()},
            "baseline_spread": round(spread, 4), "one_call_saves": round(gain, 4), "faster_beyond_spread": bool(gain > spread),
            "scratch_rows": pol._eval_seq_scratch.numel() // 32, "fragment_rows": (steps + 1) * E * N}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, nargs="+", default=[16, 128])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures the GPU"
    for kind in ("lstm", "moa"):
        for steps in args.steps:
            print(json.dumps(rate(kind, steps, args.envs, args.rounds, args.reps)), flush=True)


if __name__ == "__main__":
    main()
