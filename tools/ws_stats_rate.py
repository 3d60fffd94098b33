#!/usr/bin/env python3
"""What Watershed episode statistics cost the stepping kernel: one JSON line.

    python tools/ws_stats_rate.py [--rounds N] [--reps N] [--envs 4096,1048576] [--unattached-only] [--package-root DIR]

`rollout_actions` of 131 phases (one SeqComm episode; auto-reset, every output ring written) per variant and env count, on two
engines of one process: one with no statistics handle (the kernel instances that exist without this feature) and one with a
WatershedEpisodeStats attached.  The two are timed in alternated rounds (unattached, attached, unattached, ...), each round
`reps` calls between two device events after a warm-up of both; reported: the median over the rounds of each arm in us per
call, the attached arm as a ratio to the unattached one, and one drain() (kernel + copies to the host, host clock).

--package-root DIR imports the package from another checkout (one that may lack the statistics: the attached arm is then left
out; --unattached-only leaves it out of this tree's run too).  That is how the unattached path is compared with an earlier
commit: the same tool, the same process layout.
"""
import argparse
import json
import os
import statistics
import sys
import time

K = 131


def measure(pkg, variant, E, rounds, reps, attach=True):
    import torch
    if E <= 65536:
        reps *= 64                                                             # a timed window of milliseconds, not microseconds
    eng_u = pkg.WatershedVecEngine(variant, E, seed=1)
    arms = [("unattached", eng_u)]
    stats = None
    if attach and hasattr(eng_u, "attach_stats"):
        eng_a = pkg.WatershedVecEngine(variant, E, seed=1)
        stats = pkg.WatershedEpisodeStats(variant, E)
        eng_a.attach_stats(stats)
        arms.append(("attached", eng_a))
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    acts = torch.randint(0, 2, (K, E), device="cuda", generator=g).float()     # 0 / 1: valid messages and withdrawals alike
    out = eng_u._outputs((K,))                                                  # one set of rings: both arms write the same values
    for _, eng in arms:
        eng.reset()
        for _ in range(2):
            eng.rollout_actions(acts, K, *out, auto_reset=True)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in arms}
    for _ in range(rounds):
        for name, eng in arms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                eng.rollout_actions(acts, K, *out, auto_reset=True)
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / reps)
    res = {name + "_us": round(statistics.median(ts), 2) for name, ts in times.items()}
    res["calls_per_round"] = reps
    res["unattached_rounds_us"] = [round(t, 2) for t in times["unattached"]]
    if stats is not None:
        res["attached_over_unattached"] = round(res["attached_us"] / res["unattached_us"], 4)
        t0 = time.perf_counter()
        d = stats.drain()
        res["drain_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        res["episodes"] = int(d["counts"][:, 0].sum())
    for _, eng in arms:
        res["status"] = res.get("status", 0) | eng.status()
        eng.close()
    if stats is not None:
        stats.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--envs", default="4096,1048576")
    ap.add_argument("--unattached-only", action="store_true", help="leave the attached arm out (the process an earlier commit gets)")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import sequential_social_dilemma_games_amd as pkg
    out = {"metric": "ws_stats_rate", "phases_per_call": K, "rounds": args.rounds, "reps": args.reps,
           "package": os.path.relpath(os.path.dirname(pkg.__file__))}
    for variant, name in ((0, "seq"), (1, "seqcomm")):
        for E in [int(v) for v in args.envs.split(",")]:
            out["%s_E%d" % (name, E)] = measure(pkg, variant, E, args.rounds, args.reps, attach=not args.unattached_only)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
