"""CPU-side checks of the boundary: the C-ABI library loads, exports every symbol include/ssd.h
declares, agrees with the ctypes struct layout, and refuses to run without a GPU."""
import ctypes as C
import os
import re

import pytest

from sequential_social_dilemma_games_amd import _capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(REPO, "include", "ssd.h")).read()
    declared = set(re.findall(r"\b(ssd_[a-z_]+)\s*\(", header))
    assert declared == set(_capi.SYMBOLS), declared ^ set(_capi.SYMBOLS)
    L = _capi.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert L.ssd_abi_version() == _capi.ABI_VERSION


def test_libraries_export_nothing_but_the_declared_symbols():
    """The defined, unmangled ssd_* names of the product's and the test-hook library's dynamic symbol tables are the header's:
    what a library keeps for itself -- the embedded code object's two labels (ssd_codeobj.S) -- is hidden."""
    import subprocess
    header = open(os.path.join(REPO, "include", "ssd.h")).read()
    declared = set(re.findall(r"\b(ssd_[a-z_]+)\s*\(", header))
    for name in ("libssd_hip.so", "libssd_hip_testhooks.so"):
        lib = os.path.join(REPO, "sequential_social_dilemma_games_amd", name)
        assert os.path.exists(lib), "make all"
        out = subprocess.run(["readelf", "--dyn-syms", "-W", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        exported = set()
        for line in out.splitlines():                            # Num: Value Size Type Bind Vis Ndx Name
            f = line.split()
            if len(f) >= 8 and f[0].rstrip(":").isdigit() and f[6] != "UND" and f[7].startswith("ssd_"):
                exported.add(f[7].split("@")[0])
        assert exported == declared, (name, exported ^ declared)


def test_create_rejects_bad_configs_and_needs_a_gpu():
    import torch
    L = _capi.lib()
    c = _capi.SsdConfig()
    h = C.c_void_p()
    c.struct_size = 4
    assert L.ssd_create(C.byref(c), C.byref(h)) == _capi.SSD_E_INVALID
    c.struct_size = C.sizeof(_capi.SsdConfig)
    c.game, c.height, c.width, c.num_envs, c.num_agents, c.view_len, c.beam_len = 0, 3, 4, 1, 1, 7, 5
    c.base_map = b"@@@@" b"@ P " b"@@@@"                       # open border
    assert L.ssd_create(C.byref(c), C.byref(h)) == _capi.SSD_E_INVALID
    assert b"border" in L.ssd_last_error(None)
    c.base_map = b"@@@@" b"@ P@" b"@@@@"
    rc = L.ssd_create(C.byref(c), C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0
        L.ssd_destroy(h)
    else:
        assert rc == _capi.SSD_E_DEVICE                          # no CPU path, by design
        assert b"no CPU path" in L.ssd_last_error(None)


def test_engine_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from sequential_social_dilemma_games_amd.engine import VecEngine
    with pytest.raises(_capi.SsdError):
        VecEngine(0, None, num_envs=1, num_agents=1)


def test_python_constants_match_the_header():
    """The flag / status / error values _capi.py uses are the ones include/ssd.h declares."""
    import os
    import re
    from sequential_social_dilemma_games_amd import _capi
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssd.h")).read()

    def value(name):
        m = re.search(r"\b%s\s*=\s*([^,/\n}]+)" % name, text)
        assert m, name
        expr = m.group(1).strip().replace("u", "")
        return int(eval(expr))                                   # "1 << 3", "-2", ...

    for name in ("SSD_HOST_PTRS", "SSD_NO_ROTATE", "SSD_OBS_F32", "SSD_ROLLOUT_FUSED", "SSD_AUTO_RESET", "SSD_ROLLOUT_AUTO"):
        assert getattr(_capi, name) == value(name), name
    for name in ("SSD_ST_BAD_ACTION", "SSD_ST_NO_SPAWN", "SSD_ST_MOVE_LOOKUP", "SSD_ST_WAIT_TIMEOUT"):
        assert getattr(_capi, name) == value(name), name
    for name in ("SSD_PATH_AQL", "SSD_PATH_COHERENT", "SSD_PATH_SPLIT", "SSD_PATH_FUSED", "SSD_PATH_SYNC", "SSD_PATH_QUEUE_DROPPED", "SSD_PATH_FORKED"):
        assert getattr(_capi, name) == value(name), name
    assert value("SSD_OK") == 0 and value("SSD_E_DEVICE") == -2
    assert int(re.search(r"#define SSD_ABI_VERSION (\d+)", text).group(1)) == _capi.lib().ssd_abi_version()


def test_product_library_reads_only_the_documented_knobs():
    """the shipped library honours the safe, documented environment variables only (the table in include/ssd.h);
    knobs that can change results -- fence scopes, forced forks, alternating geometries -- exist in the test-hook build alone."""
    import subprocess
    pkg = os.path.join(REPO, "sequential_social_dilemma_games_amd")
    documented = {"SSD_AQL", "SSD_AQL_COHERENT", "SSD_AQL_SPLIT", "SSD_AQL_SYNC", "SSD_AQL_QUEUES", "SSD_ROLLOUT_CHAINS",
                  "SSD_ENVS_PER_BLOCK", "SSD_AQL_VERBOSE"}
    header = open(os.path.join(REPO, "include", "ssd.h")).read()
    for k in documented:
        assert re.search(r"\b%s\b" % k, header), "%s is not in the header's table" % k
    out = subprocess.run(["strings", os.path.join(pkg, "libssd_hip.so")], stdout=subprocess.PIPE, check=True).stdout.decode()
    found = set(re.findall(r"SSD_[A-Z][A-Z_0-9]*", out))
    assert found == documented, found ^ documented
    hooks = os.path.join(pkg, "libssd_hip_testhooks.so")
    assert os.path.exists(hooks), "make testhooks"
    out = subprocess.run(["strings", hooks], stdout=subprocess.PIPE, check=True).stdout.decode()
    more = set(re.findall(r"SSD_[A-Z][A-Z_0-9]*", out))
    assert {"SSD_AQL_ACQ", "SSD_AQL_REL", "SSD_AQL_ALTERNATE", "SSD_AQL_ALWAYS_FORK"} <= more and documented <= more


@pytest.mark.parametrize("var,want", [(None, 0), ("ROCP_TOOL_LIBRARIES", 1), ("HSA_TOOLS_LIB", 1), ("ROCPROF_COUNTER_COLLECTION", 1),
                                      ("LD_PRELOAD_NAME", 1)])
def test_profiler_detection(var, want):
    """with a profiling tool attached the rollout calls must not make kernels wait for other queues' kernels
    (such tools may run kernels one at a time).  ssd_profiler_attached() is the rule the library applies: the ROCm tools'
    environment variables, or their libraries already loaded.  Needs no device."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if not k.startswith(("ROCP", "ROCPROF", "HSA_TOOLS")) and k != "LD_PRELOAD"}
    # (the variable is set AFTER the library -- and with it the HIP runtime -- has loaded: the runtime itself acts on these
    # variables when it loads, and a made-up tool path makes it abort; the rule under test only reads the text)
    name = "LD_PRELOAD" if var == "LD_PRELOAD_NAME" else var
    value = {"LD_PRELOAD_NAME": "librocprofiler-sdk-tool.so", "ROCPROF_COUNTER_COLLECTION": "1"}.get(var, "/nonexistent/libtool.so")
    code = ("import os, sys; sys.path.insert(0, %r); from sequential_social_dilemma_games_amd import _capi; L = _capi.lib(); "
            "assert L.ssd_profiler_attached() == 0; " % REPO)
    if var:
        code += "os.environ[%r] = %r; " % (name, value)
    code += "print(L.ssd_profiler_attached())"
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert int(r.stdout.decode().strip().splitlines()[-1]) == want


def test_no_vector_memory_instruction_is_inline_asm():
    """the coherent kernels' agent-scope / non-temporal loads and stores are the compiler-tracked buffer builtins,
    not inline asm the compiler cannot see as outstanding (round 3 lost a grid piece to such a load under a divergent branch, and
    a kernel to asm loads with much code between issue and wait).  tools/check_no_asm_vmem.py on the committed source and its ISA."""
    import shutil
    import subprocess
    import sys
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    csrc = os.path.join(REPO, "sequential_social_dilemma_games_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "ARCH=gfx950", "asm"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_no_asm_vmem.py"), os.path.join(csrc, "ssd_kernels.hip"),
                        os.path.join(csrc, "ssd_kernels.s")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
