"""What a Watershed policy rollout costs: the policy kernel alone in a lock-step batch (one acting agent per
16-env tile) and in a deliberately mixed one (µs, and its share of the FP32 peak by the FLOP count of the cell's matrix product),
WatershedVecEngine.rollout_policy per phase (greedy and sampled), ssd_ws_step alone, and the loop a user writes without it
(eng.step, WatershedLSTMPolicy.forward with its gather by acting agent, torch sampling) per phase.  SeqComm and Seq, C = 128,
4096 and 65 536 envs, K = 131 phases per call.  Device events around work that ends in a synchronise; every figure after two
warm-up calls.  One JSON line.

    python tools/policy_ws_rate.py [--steps 131] [--reps 20] [--quick]
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
from sequential_social_dilemma_games_amd.policy import WatershedLSTMPolicy  # noqa: E402
from sequential_social_dilemma_games_amd.watershed import WatershedVecEngine  # noqa: E402

FP32_PEAK = 157.3e12            # MI355X_MICROARCH.md: FP32 vector = FP32 matrix peak
DEV = torch.device("cuda", 0)


def cell_flop_per_row(Cs):
    """2 x the multiply-adds of the cell's matrix product: [d1, h] (16 + C) x 4C."""
    return 2 * (16 + Cs) * 4 * Cs


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


def measure(name, variant, E, Cs, steps, reps):
    eng = WatershedVecEngine(variant, E, seed=1)
    obs0, agent0 = eng.reset()
    pol = WatershedLSTMPolicy(variant, cell_size=Cs, seed=2).to(DEV)
    S = pol.num_sets
    out = {"config": name, "E": E, "sets": S, "C": Cs, "phases_per_call": steps}
    # the kernel alone: every tile one acting agent (what lock step gives), then ids mixed within every tile
    rows = torch.zeros((E, 2, Cs), dtype=torch.float32, device=DEV)
    uniform = torch.full((E,), S - 1, dtype=torch.int8, device=DEV)
    mixed = (torch.arange(E, device=DEV) % S).to(torch.int8)
    L, w, dp = _capi.lib(), pol.packed(), lambda t: C.c_void_p(t.data_ptr())                       # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    dist, value = torch.empty((E, 5), dtype=torch.float32, device=DEV), torch.empty((E,), dtype=torch.float32, device=DEV)

    def forward(agent):                                          # the library call itself: one launch, the state in place
        _capi.policy_check(L.ssd_ws_policy_forward(dp(w), S, Cs, variant, dp(obs0), dp(agent), dp(rows), None, E, dp(rows), dp(dist),
                                                   dp(value), 0, 0, stream))
    out["forward_us"] = round(timed(lambda: forward(uniform), reps * 50), 2)
    out["forward_mixed_tiles_us"] = round(timed(lambda: forward(mixed), reps * 50), 2)
    flop = cell_flop_per_row(Cs) * E
    out["cell_gflop"] = round(flop / 1e9, 4)
    out["floor_us"] = round(flop / FP32_PEAK * 1e6, 3)
    out["forward_frac_fp32_peak"] = round(flop / (out["forward_us"] * 1e-6) / FP32_PEAK, 4)
    # the closed loop
    z = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=DEV)   # noqa: E731
    r = {"obs": z((steps, E, 12)), "agent": z((steps, E), torch.int8), "rew": z((steps, E), torch.float64), "done": z((steps, E), torch.uint8),
         "actor": z((steps, E), torch.int8), "actions": z((steps, E)), "logp": z((steps, E)), "value": z((steps, E)), "dist": z((steps, E, 5))}
    last_value = z((E,))
    state = pol.initial_state((E, S))
    cur = [obs0, agent0]
    for greedy in (True, False):
        def call(greedy=greedy):
            eng.rollout_policy(pol, cur[0], cur[1], steps, r["obs"], r["agent"], rew=r["rew"], done=r["done"], actor=r["actor"],
                               actions=r["actions"], logp=r["logp"], value=r["value"], dist=r["dist"], state=state, last_value=last_value,
                               greedy=greedy)
            cur[0], cur[1] = r["obs"][steps - 1].clone(), r["agent"][steps - 1].clone()
        out["rollout_%s_us_per_phase" % ("greedy" if greedy else "sampled")] = round(timed(call, reps) / steps, 2)
    # the env step alone, and the loop written with it
    acts = torch.full((E,), 1.0, dtype=torch.float32, device=DEV)    # a valid message and a valid withdrawal
    outs = eng._outputs()
    out["ws_step_us"] = round(timed(lambda: eng.step(acts, auto_reset=True, out=outs), steps), 2)
    ar = torch.arange(E, device=DEV)
    comm_ids = 4 if variant == _capi.SSD_WS_SEQ_COMM else 0
    carry = [eng.step(acts, auto_reset=True, out=outs)[:2]]

    def eager():
        obs, agent = carry[0]
        ag = agent.long()
        with torch.no_grad():
            dist, v, new = pol(obs, ag, state[ar, ag])
            state[ar, ag] = new
            msg = torch.multinomial(torch.softmax(dist, -1), 1)[:, 0].to(torch.float32)
            a = torch.normal(dist[:, 0], torch.exp(dist[:, 1]))
            acts.copy_(torch.where(ag < comm_ids, msg, a.clamp(0.0, 1.0)))
        carry[0] = eng.step(acts, auto_reset=True, out=outs)[:2]
    out["torch_eager_us_per_phase"] = round(timed(eager, steps), 2)
    out["rollout_sampled_vs_eager"] = round(out["torch_eager_us_per_phase"] / out["rollout_sampled_us_per_phase"], 2)
    assert eng.status() == 0
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=131)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="the small configurations, few repetitions (for a profiler run)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures the GPU"
    configs = [("seq_comm", _capi.SSD_WS_SEQ_COMM, 4096, 128), ("seq", _capi.SSD_WS_SEQ, 4096, 128),
               ("seq_comm", _capi.SSD_WS_SEQ_COMM, 65536, 128), ("seq", _capi.SSD_WS_SEQ, 65536, 128)]
    if args.quick:
        configs, args.reps, args.steps = configs[:2], 2, 24
    rows = [measure(n, v, E, Cs, steps=args.steps, reps=args.reps) for n, v, E, Cs in configs]
    print(json.dumps({"label": label_line("policy_ws_rate.py"), "results": rows}), flush=True)


if __name__ == "__main__":
    main()
