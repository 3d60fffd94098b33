"""V-trace targets (include/ssd.h, V-TRACE TARGETS) without a GPU: postprocessing.vtrace's NumPy path
against the tests' time-major restatement of RLlib's form (vtrace_ref), bit for bit; the properties of the contract; the C
ABI's refusals, which come before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import vtrace_ref
from gae_ref import same_bits
from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd.postprocessing import compute_advantages, vtrace
from vtrace_ref import FINITE, INF, build, make_rings, spacing32

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = vtrace_ref.matrix(vtrace_ref.CPU_STEPS, vtrace_ref.CPU_LANES)
NAMES = ("rew", "value", "rhos", "bootstrap_value", "done", "bonus")


def _tensors(c):
    return {k: None if v is None else torch.from_numpy(np.ascontiguousarray(v)) for k, v in c.items()}


def _run(c, **kw):
    t = _tensors(c)
    vs, pg = vtrace(t["rew"], t["value"], t["rhos"], t["bootstrap_value"], t["done"], bonus=t["bonus"], **kw)
    return vs.numpy(), pg.numpy()


def _ref(c, **kw):
    return vtrace_ref.vtrace_ref(c["rew"], c["value"], c["rhos"], c["bootstrap_value"], c["done"], bonus=c["bonus"], **kw)


@pytest.mark.parametrize("name,rings,call", CASES, ids=[c[0] for c in CASES])
def test_host_path_equals_the_restatement(name, rings, call):
    c = build(rings, call)
    vs, pg = _run(c, **call)
    ref_vs, ref_pg = _ref(c, **call)
    assert same_bits(vs, ref_vs), name
    assert same_bits(pg, ref_pg), name


def test_the_matrix_covers_what_it_should():
    """Every K, L, done mode, gamma and threshold pair, every (bonus, done) instance of the kernel, rings that wrap -- and
    importance weights on both sides of every finite threshold: at least a tenth of the rows below and a tenth above, in
    every case of 1000 rows or more and over the rows of all cases together (a case of one row has one side)."""
    seen = {"K": set(), "L": set(), "dm": set(), "g": set(), "th": set(), "inst": set(), "boot": set(), "wrap": 0}
    pooled = []
    for name, rings, call in CASES:
        c = build(rings, call)
        R, K = rings["R"], call.get("n_steps", rings["R"])
        seen["K"].add(K), seen["L"].add(int(np.prod(rings["trailing"]))), seen["dm"].add(rings["done_mode"])
        seen["g"].add(call["gamma"]), seen["th"].add((call["clip_rho_threshold"], call["clip_pg_rho_threshold"]))
        seen["inst"].add((c["bonus"] is not None, c["done"] is not None)), seen["boot"].add(c["bootstrap_value"] is not None)
        seen["wrap"] += (call.get("step0", 0) % R) + K > R
        rows = [(call.get("step0", 0) + k) % R for k in range(K)]
        rho = c["rhos"].reshape(R, -1)[rows].astype(np.float64).ravel()
        pooled.append(rho)
        if rho.size >= 1000:
            for th in FINITE:
                assert (rho < th).mean() >= 0.1 and (rho > th).mean() >= 0.1, (name, th)
        if rings["done_mode"] == "last":
            assert c["done"].reshape(R, -1)[rows[-1]].all()
    assert seen["K"] >= set(vtrace_ref.CPU_STEPS) and seen["L"] >= set(vtrace_ref.CPU_LANES)
    assert seen["dm"] == set(vtrace_ref.DONES) and seen["g"] == set(vtrace_ref.GAMMAS) and seen["th"] == set(vtrace_ref.THRESHOLDS)
    assert len(seen["inst"]) == 4 and seen["boot"] == {True, False} and seen["wrap"] >= 4
    rho = np.concatenate(pooled)
    for th in FINITE:
        assert (rho < th).mean() >= 0.1 and (rho > th).mean() >= 0.1, th


def test_three_steps_by_hand():
    """One lane, gamma 0.9, thresholds (1, 1), bootstrap 3: every number written out."""
    rew = torch.tensor([[1], [0], [2]], dtype=torch.int32)
    value = torch.tensor([[0.5], [0.25], [1.0]])
    rhos = torch.tensor([[2.0], [0.5], [1.0]])
    vs, pg = vtrace(rew, value, rhos, torch.tensor([3.0]), gamma=0.9)
    g = 0.9
    d2 = 1.0 * ((2.0 + g * 3.0) - 1.0)                           # rho 1
    acc2 = d2 + (g * 1.0) * 0.0
    vs2, pg2 = 1.0 + acc2, 1.0 * ((2.0 + g * 3.0) - 1.0)
    d1 = 0.5 * ((0.0 + g * 1.0) - 0.25)                          # rho 0.5: below both thresholds, and c = 0.5
    acc1 = d1 + (g * 0.5) * acc2
    vs1, pg1 = 0.25 + acc1, 0.5 * ((0.0 + g * vs2) - 0.25)
    d0 = 1.0 * ((1.0 + g * 0.25) - 0.5)                          # rho 2: clipped to 1 three times
    acc0 = d0 + (g * 1.0) * acc1
    vs0, pg0 = 0.5 + acc0, 1.0 * ((1.0 + g * vs1) - 0.5)
    assert same_bits(vs.numpy(), np.array([[vs0], [vs1], [vs2]], np.float32))
    assert same_bits(pg.numpy(), np.array([[pg0], [pg1], [pg2]], np.float32))
    assert abs(vs0 - 3.016) < 1e-12 and abs(pg1 - 1.99) < 1e-12 and abs(vs2 - 4.7) < 1e-12
    # with a done on the middle row nothing of row 2 or the bootstrap reaches rows 0 and 1
    done = torch.tensor([[0], [1], [0]], dtype=torch.uint8)
    vs, pg = vtrace(rew, value, rhos, torch.tensor([3.0]), done, gamma=0.9)
    e1 = 0.5 * ((0.0 + 0.0 * 1.0) - 0.25)
    assert same_bits(vs.numpy()[1], np.array([0.25 + (e1 + 0.0 * acc2)], np.float32))
    assert same_bits(pg.numpy()[1], np.array([e1], np.float32))
    # without clipping rho 2 counts twice in delta and pg, and still once (c bar = 1) in the trace
    vs, pg = vtrace(rew, value, rhos, torch.tensor([3.0]), gamma=0.9, clip_rho_threshold=INF, clip_pg_rho_threshold=INF)
    u0 = 2.0 * ((1.0 + g * 0.25) - 0.5)
    assert same_bits(vs.numpy()[0], np.array([0.5 + (u0 + (g * 1.0) * acc1)], np.float32))
    assert same_bits(pg.numpy()[0], np.array([2.0 * ((1.0 + g * vs1) - 0.5)], np.float32))


def test_rows_up_to_a_done_row_do_not_see_what_follows():
    c = make_rings(seed=5, R=40, trailing=(9,), done_mode="some", with_bonus=True)
    c["done"][17] = 1
    kw = dict(gamma=0.99, clip_rho_threshold=0.7, clip_pg_rho_threshold=1.3, bonus_weight=0.5)
    vs, pg = _run(c, **kw)
    other = make_rings(seed=6, R=40, trailing=(9,), done_mode="some", with_bonus=True)
    d = {k: (None if c[k] is None else c[k].copy()) for k in NAMES}
    for k in ("rew", "value", "rhos", "bonus", "done"):
        d[k][18:] = other[k][18:]
    d["bootstrap_value"] = other["bootstrap_value"]
    vs2, pg2 = _run(d, **kw)
    assert same_bits(vs[:18], vs2[:18]) and same_bits(pg[:18], pg2[:18])
    assert not same_bits(vs[18:], vs2[18:])


def test_rows_outside_the_call_are_left_alone():
    c = make_rings(seed=7, R=10, trailing=(5,), done_mode="some")
    t = _tensors(c)
    out = (torch.full((10, 5), 7.0), torch.full((10, 5), -7.0))
    vs, pg = vtrace(t["rew"], t["value"], t["rhos"], t["bootstrap_value"], t["done"], step0=8, n_steps=4, out=out)
    assert vs is out[0] and pg is out[1]
    outside = [2, 3, 4, 5, 6, 7]
    assert (vs[outside] == 7.0).all() and (pg[outside] == -7.0).all()
    ref_vs, ref_pg = _ref(c, step0=8, n_steps=4)
    inside = [8, 9, 0, 1]
    assert same_bits(vs.numpy()[inside], ref_vs[inside]) and same_bits(pg.numpy()[inside], ref_pg[inside])
    vs, pg = vtrace(t["rew"], t["value"], t["rhos"], step0=8, n_steps=4)
    assert (vs[outside] == 0).all() and (pg[outside] == 0).all()


@pytest.mark.parametrize("T", [2, 16, 17])
def test_the_reference_trainers_dropped_last_row(T):
    """RLlib's VTraceLoss on one T-row sequence: the time-major tensors lose their last row and the bootstrap is the value of
    that row.  That is vtrace() on the sequence's first T - 1 rows with bootstrap_value = value[T - 1]."""
    c = make_rings(seed=40 + T, R=T, trailing=(66,), done_mode="some")
    f64 = np.float64
    disc = (1.0 - (c["done"] != 0).astype(f64)) * f64(0.99)
    ref_vs, ref_pg = vtrace_ref.from_importance_weights(c["rhos"].astype(f64)[:-1], disc[:-1], c["rew"].astype(f64)[:-1],
                                                        c["value"].astype(f64)[:-1], c["value"].astype(f64)[-1], 1.0, 1.0)
    t = _tensors(c)
    vs, pg = vtrace(t["rew"], t["value"], t["rhos"], t["value"][T - 1].contiguous(), t["done"], gamma=0.99, n_steps=T - 1)
    assert same_bits(vs.numpy()[:-1], ref_vs.astype(np.float32)) and same_bits(pg.numpy()[:-1], ref_pg.astype(np.float32))
    assert (vs[-1] == 0).all() and (pg[-1] == 0).all()


@pytest.mark.parametrize("thresholds", [(1.0, 1.0), (1.3, 2.0), (INF, INF)])
def test_on_policy_it_is_the_discounted_return(thresholds):
    """rhos = 1 and thresholds >= 1: vs is the value_targets and pg the advantages of compute_advantages(use_gae=False).  Two
    float64 computations in different orders, each rounded once: |a - b| <= spacing32(max(|a|, |b|)) + 1e-12 (1 + max |vt|)."""
    c = make_rings(seed=11, R=37, trailing=(130,), done_mode="some")
    c["done"] = (np.random.default_rng(12).random(c["done"].shape) < 0.1).astype(np.uint8)
    c["rhos"] = np.ones_like(c["rhos"])
    t = _tensors(c)
    vs, pg = vtrace(t["rew"], t["value"], t["rhos"], t["bootstrap_value"], t["done"], gamma=0.99,
                    clip_rho_threshold=thresholds[0], clip_pg_rho_threshold=thresholds[1])
    adv, vt = compute_advantages(t["rew"], t["value"], t["bootstrap_value"], t["done"], gamma=0.99, use_gae=False)
    scale = 1e-12 * (1.0 + float(vt.abs().max()))
    for a, b in ((vs, vt), (pg, adv)):
        a, b = a.numpy().astype(np.float64), b.numpy().astype(np.float64)
        diff, tol = np.abs(a - b), spacing32(np.maximum(np.abs(a), np.abs(b))) + scale
        print("on-policy: max difference %.3g, max |x| %.3g" % (diff.max(), np.abs(b).max()))
        assert (diff <= tol).all()


def test_python_argument_checks():
    c = _tensors(make_rings(seed=8, R=6, trailing=(2, 3), done_mode="some", with_bonus=True))
    rew, value, rhos, boot, done, bonus = (c[k] for k in NAMES)
    ok = lambda **kw: vtrace(**dict(dict(rew=rew, value=value, rhos=rhos, bootstrap_value=boot, done=done, bonus=bonus), **kw))  # noqa: E731
    ok()
    ok(clip_rho_threshold=INF, clip_pg_rho_threshold=INF)
    bad = [dict(rew=rew.to(torch.int64)), dict(rew=rew.numpy()), dict(value=value.to(torch.float64)), dict(value=None),
           dict(value=value[:5]), dict(value=value.transpose(1, 2)), dict(rhos=None), dict(rhos=rhos.to(torch.float64)),
           dict(rhos=rhos[:, :1]), dict(done=done.to(torch.int32)), dict(bootstrap_value=boot[0]),
           dict(bootstrap_value=boot.to(torch.float64)), dict(bonus=bonus.to(torch.float64)), dict(bonus=bonus[:, :1]),
           dict(gamma=float("nan")), dict(gamma=INF), dict(clip_rho_threshold=0.0), dict(clip_rho_threshold=-1.0),
           dict(clip_rho_threshold=float("nan")), dict(clip_pg_rho_threshold=0.0), dict(clip_pg_rho_threshold=float("nan")),
           dict(bonus_weight=float("nan")), dict(n_steps=0), dict(n_steps=7), dict(step0=-1), dict(out=(torch.empty(6, 2, 3),)),
           dict(out=(torch.empty(6, 2, 3), torch.empty(6, 2, 2))),
           dict(out=(torch.empty(6, 2, 3), torch.empty(6, 2, 3, dtype=torch.float64)))]
    for kw in bad:
        with pytest.raises(ValueError):
            ok(**kw)
    same = torch.empty(6, 2, 3)
    with pytest.raises(ValueError):
        ok(out=(same, same))
    with pytest.raises(ValueError):
        vtrace(torch.zeros((0, 3), dtype=torch.int32), torch.zeros((0, 3)), torch.zeros((0, 3)))
    vs, pg = vtrace(rew[:, 0, 0].contiguous(), value[:, 0, 0].contiguous(), rhos[:, 0, 0].contiguous())   # [R]: one trajectory
    assert vs.shape == (6,)


def _call(L, **kw):
    one = C.c_void_p(64)                                         # never dereferenced: the checks come before any device call
    a = dict(rew=one, bonus=None, bonus_weight=1.0, value=one, rhos=one, done=None, bootstrap_value=None, lanes=4, ring=8, step0=0,
             n_steps=8, gamma=0.99, clip_rho=1.0, clip_pg=1.0, flags=0, vs=one, pg=one, device_id=0, stream=None)
    a.update(kw)
    return L.ssd_vtrace(a["rew"], a["bonus"], a["bonus_weight"], a["value"], a["rhos"], a["done"], a["bootstrap_value"], a["lanes"],
                        a["ring"], a["step0"], a["n_steps"], a["gamma"], a["clip_rho"], a["clip_pg"], a["flags"], a["vs"], a["pg"],
                        a["device_id"], a["stream"])


@pytest.mark.parametrize("kw,word", [
    (dict(lanes=0), b"lanes"), (dict(ring=0), b"ring"), (dict(n_steps=0), b"n_steps"), (dict(n_steps=9), b"n_steps > ring"),
    (dict(step0=-1), b"step0"), (dict(flags=1), b"flag"), (dict(rew=None), b"rew"), (dict(value=None), b"value"),
    (dict(rhos=None), b"rhos"), (dict(vs=None), b"vs"), (dict(pg=None), b"pg_advantages"), (dict(gamma=float("nan")), b"gamma"),
    (dict(gamma=float("inf")), b"gamma"), (dict(clip_rho=0.0), b"clip_rho_threshold"), (dict(clip_rho=float("nan")), b"clip_rho_threshold"),
    (dict(clip_pg=-1.0), b"clip_pg_rho_threshold"), (dict(clip_pg=float("nan")), b"clip_pg_rho_threshold"),
    (dict(bonus=C.c_void_p(64), bonus_weight=float("inf")), b"bonus_weight")])
def test_abi_rejects_bad_arguments_before_any_device_call(kw, word):
    L = _capi.lib()
    assert _call(L, **kw) == _capi.SSD_E_INVALID
    assert word in L.ssd_vtrace_last_error()


def test_abi_without_a_device_fails_cleanly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = _capi.lib()
    assert _call(L) == _capi.SSD_E_DEVICE
    assert _call(L, clip_rho=INF, clip_pg=INF) == _capi.SSD_E_DEVICE      # +inf passes the checks: no clip
    assert b"no HIP device" in L.ssd_vtrace_last_error()
    with pytest.raises(_capi.SsdError):
        _capi.vtrace_check(_capi.SSD_E_DEVICE)


def test_symbols_header_and_export():
    import sequential_social_dilemma_games_amd as pkg
    assert {"ssd_vtrace", "ssd_vtrace_last_error"} <= set(_capi.SYMBOLS)
    header = open(os.path.join(REPO, "include", "ssd.h")).read()
    assert re.search(r"int ssd_vtrace\(const int32_t \*rew, const float \*bonus, double bonus_weight, const float \*value, "
                     r"const float \*rhos,", header)
    assert "const char *ssd_vtrace_last_error(void);" in header
    assert pkg.vtrace is vtrace
    assert _capi.lib().ssd_abi_version() == 6
