"""The host-side decisions of a rollout through the library's own dispatch queues (csrc/ssd_rollout_plan.hpp; carried out by
ssd_rollout.hip, rollout_aql and aql_set) without a GPU: over a grid of calls -- step counts 0 .. 21, first steps, reset periods,
output and action rings, run caps, split or not, both orientations of the state pair, coherent or not -- every plan's packets are
run symbolically against the kernels' contract: every step computed once and in order, no run across a reset, every step's
observations rendered once, from buffers that hold exactly that step, into its ring slot; rewards, dones and actions in their
slots; no launch writing what it reads; a block in the argument set for every kind a packet names; the fences and the doorbells
by their rules.  Plus the kind tables' sizes, two schedules written out by hand, and the form of a call at its thresholds."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sequential_social_dilemma_games_amd", "csrc")

# n_steps 0 .. 21 x step0 0 .. 6 x 9 reset periods x 4 action rings x 4 caps x split x orientation x coherent, over the rings
# {1, 2, 3, 5, 8, n_steps}: six each, five for n_steps = 0
GRID_CASES = (22 * 6 - 1) * 7 * 9 * 4 * 4 * 2 * 2 * 2


def test_rollout_plan_over_the_grid(tmp_path):
    exe = str(tmp_path / "rollout_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(HERE, "native", "rollout_plan_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and len(lines) == 5, r.stdout
    assert GRID_CASES == 1056384 and lines[-2] == "grid: %d cases ok" % GRID_CASES, r.stdout
    assert "runtime error" not in r.stderr


def test_the_rollout_unit_plans_through_that_header():
    """rollout_aql and aql_set decide nothing themselves: kinds, blocks and packets come from the plan header, and the header
    stays free of HIP."""
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "ssd_rollout.hip")).read())
    for call in ("plan::choose_form(", "plan::block_slots(", "plan::kind_table(", "plan::fill_block(", "plan::Schedule sched(",
                 "plan::start_orientation("):
        assert src.count(call) == 1, call
    assert "dense[" in src and "run_kind" not in src and "kKindsPerO" not in src
    hdr = open(os.path.join(CSRC, "ssd_rollout_plan.hpp")).read()
    assert "#include <hip" not in hdr and not re.search(r"\bhip[A-Z]\w*\(", re.sub(r"//[^\n]*", "", hdr))
