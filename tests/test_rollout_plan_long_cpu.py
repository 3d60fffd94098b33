"""The host-side decisions of LONG rollout calls (csrc/ssd_rollout_plan.hpp: choose_form's long cap, Schedule under it, the long kinds
and fill_long_block's LongParams blocks; carried out by ssd_rollout.hip) without a GPU, as tests/test_rollout_plan_cpu.py checks
the calls that are not long.  Over calls of 56 .. 90 steps -- first steps 0 .. 9, reset periods {0, 7, 8, 9, 13, 64}, rings of 1, 3,
8, 9 and one slot per step, action rings of 0 and 5, both orientations of the state pair, planned long and not -- every plan's
packets are run symbolically against the kernels' contract: every step computed once and in order and rendered once, in step
order, from buffers that hold exactly that step, into its ring slot; runs of eight wherever eight steps remain before the call's
end and the next reset, else four, two, one, never across a reset; no launch writing what it or its renderers read; a block in the
argument set for every kind a packet names; the final orientation the planner's.  With the long cap 0 every group equals the one
the constructor without a long cap gives.  Plus one schedule written out by hand (75 steps = 8 x 9 + 2 + 1) and the form of a
call one step below the long-call threshold and at it (and at 63 and 64 steps, where the threshold began)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sequential_social_dilemma_games_amd", "csrc")

# n_steps 56 .. 90 x step0 0 .. 9 x 6 reset periods x 5 rings x 2 action rings x 2 orientations x long or not
GRID_CASES = 35 * 10 * 6 * 5 * 2 * 2 * 2


def test_long_rollout_plans_over_the_grid(tmp_path):
    exe = str(tmp_path / "rollout_plan_long_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(HERE, "native", "rollout_plan_long_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and len(lines) == 4, r.stdout
    assert GRID_CASES == 84000 and lines[-2] == "grid: %d cases ok" % GRID_CASES, r.stdout
    assert "runtime error" not in r.stderr
