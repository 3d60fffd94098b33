"""V-trace targets on the device (csrc/ssd_vtrace.hip): the kernel against the package's NumPy path -- which
the CPU suite pins to the restatement of RLlib's form -- and against that restatement itself, bit for bit: the CPU suite's
matrix, the step counts and lane counts at which the kernel takes another path, all four instances, out= on a stream of the
caller's, and one full-size case."""
import numpy as np
import pytest
import torch

import gae_ref
import vtrace_ref
from gae_ref import same_bits
from sequential_social_dilemma_games_amd.postprocessing import vtrace
from vtrace_ref import build, make_rings

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CASES = vtrace_ref.matrix(vtrace_ref.CPU_STEPS, vtrace_ref.CPU_LANES)
# K: no full block of 16 steps, one, two (the odd buffer), three, and a remainder after each; L: spare lanes, a second and a third wave
BLOCK_CASES = vtrace_ref.matrix(vtrace_ref.GPU_STEPS, vtrace_ref.GPU_LANES)


def _call(c, dev, **kw):
    t = {k: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in c.items()}
    vs, pg = vtrace(t["rew"], t["value"], t["rhos"], t["bootstrap_value"], t["done"], bonus=t["bonus"], **kw)
    return vs.cpu().numpy(), pg.cpu().numpy()


def _check(c, call, restatement=True):
    vs, pg = _call(c, DEV, **call)
    host_vs, host_pg = _call(c, "cpu", **call)
    assert same_bits(vs, host_vs), np.argwhere(gae_ref.bits(vs) != gae_ref.bits(host_vs))[:5]
    assert same_bits(pg, host_pg), np.argwhere(gae_ref.bits(pg) != gae_ref.bits(host_pg))[:5]
    if restatement:
        ref_vs, ref_pg = vtrace_ref.vtrace_ref(c["rew"], c["value"], c["rhos"], c["bootstrap_value"], c["done"], bonus=c["bonus"], **call)
        assert same_bits(vs, ref_vs) and same_bits(pg, ref_pg)


@pytest.mark.parametrize("name,rings,call", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_the_host_path(name, rings, call):
    _check(build(rings, call), call)


@pytest.mark.parametrize("name,rings,call", BLOCK_CASES, ids=[c[0] for c in BLOCK_CASES])
def test_blocks_buffers_and_waves(name, rings, call):
    _check(build(rings, call), call)


def test_the_block_matrix_reaches_every_instance_at_every_step_count():
    seen = set()
    for _, rings, call in BLOCK_CASES:
        c = build(rings, call)
        seen.add((call.get("n_steps", rings["R"]), c["bonus"] is not None, c["done"] is not None))
    for K in vtrace_ref.GPU_STEPS:
        assert {(b, d) for k, b, d in seen if k == K} == {(False, False), (False, True), (True, False), (True, True)}, K


@pytest.mark.parametrize("bonus,done_mode", [(False, "none"), (False, "some"), (True, "none"), (True, "some")])
def test_full_size(bonus, done_mode):
    """4096 envs x 5 agents, 128 steps: 320 waves, eight blocks of 16 steps each, in each of the four instances."""
    c = make_rings(seed=21, R=128, trailing=(4096, 5), done_mode=done_mode, with_bonus=bonus)
    _check(c, dict(gamma=0.99, clip_rho_threshold=1.0, clip_pg_rho_threshold=1.0, bonus_weight=0.25), restatement=False)


def test_out_and_a_stream_of_the_callers():
    c = make_rings(seed=14, R=130, trailing=(9, 5), done_mode="some")
    call = dict(gamma=0.99, clip_rho_threshold=0.7, clip_pg_rho_threshold=1.3, step0=100, n_steps=90)
    out = (torch.full((130, 9, 5), 9.0, device=DEV), torch.full((130, 9, 5), 8.0, device=DEV))
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        t = {k: None if v is None else torch.from_numpy(v).to(DEV) for k, v in c.items()}
        vs, pg = vtrace(t["rew"], t["value"], t["rhos"], t["bootstrap_value"], t["done"], out=out, **call)
    s.synchronize()
    assert vs is out[0] and pg is out[1]
    ref_vs, ref_pg = vtrace_ref.vtrace_ref(c["rew"], c["value"], c["rhos"], c["bootstrap_value"], c["done"], **call)
    rows = [(100 + k) % 130 for k in range(90)]
    rest = [r for r in range(130) if r not in rows]
    vs, pg = vs.cpu().numpy(), pg.cpu().numpy()
    assert same_bits(vs[rows], ref_vs[rows]) and same_bits(pg[rows], ref_pg[rows])
    assert np.all(vs[rest] == 9.0) and np.all(pg[rest] == 8.0)   # rows outside the call are left alone


def test_device_argument_checks():
    c = make_rings(seed=15, R=4, trailing=(3,), done_mode="some")
    t = {k: None if v is None else torch.from_numpy(v).to(DEV) for k, v in c.items()}
    with pytest.raises(ValueError):
        vtrace(t["rew"], t["value"].cpu(), t["rhos"], t["bootstrap_value"], t["done"])
    with pytest.raises(ValueError):
        vtrace(t["rew"], t["value"], t["rhos"], t["bootstrap_value"], t["done"], out=(torch.empty(4, 3), torch.empty(4, 3)))
