"""The launch arithmetic of a fold of the episode statistics (csrc/ssd_stats_plan.hpp; carried out by ssd_stats_fold and indexed
by its two kernels) without a GPU: over n_steps and chunk lengths up to 2^31 - 1 and env counts up to 2^26 every accepted plan
has 1 <= L <= n_steps and chunks that tile the steps, a scratch that covers them, grids within a launch's limits, and a pass-1
guard that turns away every spare wave; every refusal gives its reason.  Under the address and undefined-behaviour sanitizers, so
a product that wraps stops the driver."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sequential_social_dilemma_games_amd", "csrc")

# n_steps {1, 2, 7, 8, 9, 63, 64, 65, 600, 2^30, 2^31 - 1} x chunk {0, 1, 2, 63, 64, 65, n - 1, n, n + 1, 2^30, 2^31 - 1}
# x (E, N) {(1, 1), (37, 5), (3, 64), (4096, 5), (2^26, 1), (2^26, 64)}
GRID_CASES = 11 * 11 * 6


def test_stats_plan_over_the_grid(tmp_path):
    exe = str(tmp_path / "stats_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(HERE, "native", "stats_plan_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and len(lines) == 4, r.stdout
    m = re.match(r"grid: (\d+) cases ok, (\d+) accepted, (\d+) refused$", lines[0])
    assert m and GRID_CASES == 726 and int(m.group(1)) == GRID_CASES, r.stdout
    # (2^26 envs of 64 agents are 2^26 waves a pass: refused at every one of the 121 (n_steps, chunk); more are refused for
    # their chunk counts)
    assert int(m.group(2)) + int(m.group(3)) == GRID_CASES and int(m.group(3)) >= 121 and int(m.group(2)) >= 400, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_stats_unit_plans_through_that_header():
    """ssd_stats_fold sizes nothing itself and the kernels form no chunk product of their own; the header stays free of HIP."""
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "ssd_stats.hip")).read())
    assert src.count("plan::plan_fold(") == 1 and src.count("plan::wave_has_chunk(") == 1
    assert src.count("plan::chunk_begin(") == 2 and src.count("plan::chunk_end(") == 2
    assert "c * L" not in src and "k0 + L" not in src and "+ L - 1" not in src and "kAutoChunk" not in src
    for launch in ("<<<p.grid1, kBlock, 0, s>>>", "<<<p.grid2, kBlock, 0, s>>>"):
        assert src.count(launch) == 1, launch
    hdr = open(os.path.join(CSRC, "ssd_stats_plan.hpp")).read()
    assert "#include <hip" not in hdr and not re.search(r"\bhip[A-Z]\w*\(", re.sub(r"//[^\n]*", "", hdr))
