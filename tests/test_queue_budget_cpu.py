"""The rule that sizes the library's pool of dispatch queues (csrc/ssd_queue_budget.hpp; used by ssd_aql.hip, pool_limit) over
every case: GPU_MAX_HW_QUEUES unset, 1 .. 3, HIP's own default 4, 8, 32, 0, negative and garbage, each with and without
SSD_AQL_QUEUES, and the pool's upper bound.  A GPU box shows one of these environments at a time: this is what covers the rest."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sequential_social_dilemma_games_amd", "csrc")


def test_queue_budget_rule_over_every_case(tmp_path):
    exe = str(tmp_path / "queue_budget_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(HERE, "native", "queue_budget_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and len(lines) == 5, r.stdout
    assert "runtime error" not in r.stderr


def test_the_dispatch_layer_uses_that_rule():
    """pool_limit() decides through queue_pool_limit() and nothing else: no second copy of the rule in ssd_aql.hip."""
    src = open(os.path.join(CSRC, "ssd_aql.hip")).read()
    assert '#include "ssd_queue_budget.hpp"' in src
    assert 'queue_pool_limit(getenv("GPU_MAX_HW_QUEUES"), getenv("SSD_AQL_QUEUES"), top)' in src
    code = re.sub(r"//[^\n]*", "", src)                     # (the comments may name the rule; the code may not restate it)
    assert code.count('getenv("GPU_MAX_HW_QUEUES")') == 1 and code.count('getenv("SSD_AQL_QUEUES")') == 1
    assert not re.search(r"4\s*-\s*hq", code)
