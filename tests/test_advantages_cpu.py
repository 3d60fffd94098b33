"""Advantages and value targets without a GPU: the package's NumPy path against the tests' restatement
(gae_ref.py: scipy's lfilter per episode segment) bit for bit, a case computed by hand, the isolation of episodes by done rows,
and the argument checks of the C ABI and of the Python function."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import gae_ref
from gae_ref import advantages_ref, make_rings, same_bits
from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd.postprocessing import compute_advantages

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = gae_ref.matrix()
BLOCK_CASES = gae_ref.block_matrix()


def _tensors(c):
    return {k: None if v is None else torch.from_numpy(v.copy()) for k, v in c.items()}


def _run(c, **kw):
    t = _tensors(c)
    adv, vt = compute_advantages(t["rew"], t["value"], t["last_value"], t["done"], bonus=t["bonus"], **kw)
    return adv.numpy(), vt.numpy()


@pytest.mark.parametrize("name,rings,call", CASES, ids=[c[0] for c in CASES])
def test_host_path_equals_the_restatement(name, rings, call):
    c = make_rings(**rings)
    adv, vt = _run(c, **call)
    want_a, want_t = advantages_ref(c["rew"], c["value"], c["last_value"], c["done"], bonus=c["bonus"], **call)
    assert adv.dtype == np.float32 and vt.dtype == np.float32 and adv.shape == c["rew"].shape
    assert same_bits(adv, want_a), np.argwhere(gae_ref.bits(adv) != gae_ref.bits(want_a))[:5]
    assert same_bits(vt, want_t), np.argwhere(gae_ref.bits(vt) != gae_ref.bits(want_t))[:5]


def test_the_matrix_covers_what_it_should():
    ks = {c[1]["R"] for c in CASES}
    assert set(gae_ref.STEPS) <= ks
    assert all(int(np.prod(c[1]["trailing"])) % 64 for c in CASES)
    for K in gae_ref.STEPS:
        for dm in gae_ref.DONES:
            for mode in gae_ref.MODES.values():
                assert any(c[1]["R"] == K and c[1]["done_mode"] == dm and all(c[2][k] == v for k, v in mode.items()) for c in CASES)
    pairs = {(c[2]["gamma"], c[2]["lambda_"], c[2]["use_gae"], c[2]["use_critic"], c[1]["with_bonus"]) for c in CASES}
    for g in gae_ref.GAMMAS:
        for lam in gae_ref.LAMBDAS:
            for mode in gae_ref.MODES.values():
                for bonus in (False, True):
                    assert (g, lam, mode["use_gae"], mode["use_critic"], bonus) in pairs
    assert any(not c[1].get("with_last", True) for c in CASES)
    assert any(c[2].get("n_steps", c[1]["R"]) < c[1]["R"] and c[2]["step0"] % c[1]["R"] + c[2]["n_steps"] > c[1]["R"] for c in CASES)


@pytest.mark.parametrize("name,rings,call", BLOCK_CASES, ids=[c[0] for c in BLOCK_CASES])
def test_host_path_equals_the_restatement_on_the_block_matrix(name, rings, call):
    c = gae_ref.build(rings, call)
    adv, vt = _run(c, **call)
    want_a, want_t = advantages_ref(c["rew"], c["value"], c["last_value"], c["done"], bonus=c["bonus"], **call)
    assert same_bits(adv, want_a), np.argwhere(gae_ref.bits(adv) != gae_ref.bits(want_a))[:5]
    assert same_bits(vt, want_t), np.argwhere(gae_ref.bits(vt) != gae_ref.bits(want_t))[:5]


def test_the_block_matrix_reaches_every_instance_at_every_step_count():
    """The kernel has twelve instances (mode x bonus given / absent x done given / absent), and its two-buffer loop another
    path for no, one, two and three full blocks of 16 steps with and without rows left over: every instance meets every step
    count; every lane count -- spare lanes, whole last waves, a second and a third wave -- meets every mode and every step count;
    the three done patterns meet every mode; and each "some" case has what it is there for."""
    assert gae_ref.LOAD_BLOCK == int(re.search(r"#define SSD_GAE_LOAD_BLOCK (\d+)", open(os.path.join(
        REPO, "sequential_social_dilemma_games_amd", "csrc", "ssd_gae.hip")).read()).group(1))
    seen, some, wraps = set(), 0, set()
    for _, rings, call in BLOCK_CASES:
        c = gae_ref.build(rings, call)
        R, (L,) = rings["R"], rings["trailing"]
        K = call.get("n_steps", R)
        mode = (call["use_gae"], call["use_critic"])
        if "step0" in call:
            assert call["step0"] % R + K > R and c["bonus"] is None and c["done"] is None     # the rows wrap
            wraps.add((mode, R, K, call["step0"]))
            continue
        seen.add((K, L, mode, c["bonus"] is not None, c["done"] is not None, rings["done_mode"], call["gamma"], call["lambda_"],
                  c["last_value"] is not None))
        if rings["done_mode"] == "all":
            assert c["done"].all()
        if rings["done_mode"] == "last":
            assert c["done"][K - 1].all() and not c["done"][:K - 1].any()
        if rings["done_mode"] == "some":
            assert gae_ref.some_conditions(c["done"], K) == (True, True, True), (rings, gae_ref.some_conditions(c["done"], K))
            some += 1
    modes = {(m["use_gae"], m["use_critic"]) for m in gae_ref.MODES.values()}
    instances = {(m, b, d) for m in modes for b in (False, True) for d in (False, True)}
    for K in gae_ref.BLOCK_STEPS:
        assert {(s[2], s[3], s[4]) for s in seen if s[0] == K} == instances, K
        assert {s[1] for s in seen if s[0] == K} == set(gae_ref.BLOCK_LANES), K
    for m in modes:
        mine = [s for s in seen if s[2] == m]
        assert {s[1] for s in mine} == set(gae_ref.BLOCK_LANES)
        assert {s[5] for s in mine} == {"none", "all", "last", "some"}
        assert {s[6] for s in mine} == set(gae_ref.GAMMAS) and {s[7] for s in mine} == set(gae_ref.LAMBDAS)
        assert {s[8] for s in mine} == {False, True}                   # last_value given and absent
        assert {w[1:] for w in wraps if w[0] == m} == {(40, 33, 30), (17, 16, 9), (48, 48, 47)}
    assert some == len(gae_ref.SOME_SEEDS) == 18
    assert {s[1] for s in seen if s[5] == "some"} >= {1, 64, 65, 128}  # one lane, whole last waves and a wave with spare lanes


def test_three_steps_by_hand():
    """rew 1, 2, 3; value 0.5, 0.25, 0.125; step 1 ends its episode; last_value 4; gamma 0.5, lambda 0.5 (all exact in binary).
    GAE: row 2 is the last row: delta = 3 + 0.5 * 4 - 0.125 = 4.875, A = 4.875.  Row 1 ended an episode: v_next = 0, carry 0:
    A = 2 - 0.25 = 1.75.  Row 0: delta = 1 + 0.5 * 0.25 - 0.5 = 0.625, A = 0.625 + 0.25 * 1.75 = 1.0625.
    Returns: G2 = 3 + 0.5 * 4 = 5, G1 = 2, G0 = 1 + 0.5 * 2 = 2."""
    rew = torch.tensor([[1], [2], [3]], dtype=torch.int32)
    value = torch.tensor([[0.5], [0.25], [0.125]], dtype=torch.float32)
    done = torch.tensor([[0], [1], [0]], dtype=torch.uint8)
    last = torch.tensor([4.0], dtype=torch.float32)
    adv, vt = compute_advantages(rew, value, last, done, gamma=0.5, lambda_=0.5)
    assert adv[:, 0].tolist() == [1.0625, 1.75, 4.875]
    assert vt[:, 0].tolist() == [1.5625, 2.0, 5.0]
    adv, vt = compute_advantages(rew, value, last, done, gamma=0.5, use_gae=False)
    assert adv[:, 0].tolist() == [1.5, 1.75, 4.875] and vt[:, 0].tolist() == [2.0, 2.0, 5.0]
    adv, vt = compute_advantages(rew, None, last, done, gamma=0.5, use_gae=False, use_critic=False)
    assert adv[:, 0].tolist() == [2.0, 2.0, 5.0] and vt[:, 0].tolist() == [0.0, 0.0, 0.0]
    # without the done row the three steps are one fragment: G1 = 2 + 0.5 * 5 = 4.5, G0 = 1 + 0.5 * 4.5 = 3.25
    adv, vt = compute_advantages(rew, value, last, None, gamma=0.5, use_gae=False)
    assert vt[:, 0].tolist() == [3.25, 4.5, 5.0]
    # a bonus of 2 with weight 0.25 adds 0.5 to every reward; no last_value bootstraps with 0
    bonus = torch.full((3, 1), 2.0)
    adv, vt = compute_advantages(rew, value, None, done, gamma=0.5, use_gae=False, bonus=bonus, bonus_weight=0.25)
    assert vt[:, 0].tolist() == [2.75, 2.5, 3.5]


@pytest.mark.parametrize("mode", sorted(gae_ref.MODES))
def test_a_done_row_isolates_episodes(mode):
    kw = dict(gamma=0.99, lambda_=0.95, bonus_weight=0.25, **gae_ref.MODES[mode])
    c = make_rings(seed=5, R=40, trailing=(9,), done_mode="none", with_bonus=True)
    c["done"] = np.zeros((40, 9), np.uint8)
    cut = np.arange(9) * 4 + 2                                   # lane l ends an episode at row cut[l]
    c["done"][cut, np.arange(9)] = 1
    adv, vt = _run(c, **kw)
    rng = np.random.default_rng(6)
    for key in ("rew", "value", "bonus", "last_value", "done"):
        d = {k: None if v is None else v.copy() for k, v in c.items()}
        for l in range(9):
            after = slice(cut[l] + 1, None)
            if key == "last_value":
                d[key][l] += 1.0
            elif key == "done":
                d[key][after, l] = rng.random(40 - cut[l] - 1) < 0.3
            elif key == "rew":
                d[key][after, l] += 7
            else:
                d[key][after, l] += np.float32(0.5)
        adv2, vt2 = _run(d, **kw)
        for l in range(9):
            assert same_bits(adv[:cut[l] + 1, l], adv2[:cut[l] + 1, l]), (key, l)
            assert same_bits(vt[:cut[l] + 1, l], vt2[:cut[l] + 1, l]), (key, l)
        if key != "done" and not (key == "value" and mode == "returns"):
            assert not same_bits(adv, adv2), key                 # (the change did reach the rows after the cut)


def test_rows_outside_the_call_are_left_alone():
    c = make_rings(seed=7, R=10, trailing=(3,), done_mode="some")
    t = _tensors(c)
    out = (torch.full((10, 3), 9.0), torch.full((10, 3), 8.0))
    adv, vt = compute_advantages(t["rew"], t["value"], t["last_value"], t["done"], step0=8, n_steps=4, out=out)
    assert adv is out[0] and vt is out[1]
    assert torch.all(adv[2:8] == 9.0) and torch.all(vt[2:8] == 8.0)
    want_a, want_t = advantages_ref(c["rew"], c["value"], c["last_value"], c["done"], step0=8, n_steps=4)
    rows = [8, 9, 0, 1]
    assert same_bits(adv.numpy()[rows], want_a[rows]) and same_bits(vt.numpy()[rows], want_t[rows])
    adv, vt = compute_advantages(t["rew"], t["value"], t["last_value"], t["done"], step0=8, n_steps=4)
    assert same_bits(adv.numpy(), want_a) and same_bits(vt.numpy(), want_t)


def test_python_argument_checks():
    c = _tensors(make_rings(seed=8, R=6, trailing=(2, 3), done_mode="some", with_bonus=True))
    rew, value, last, done, bonus = c["rew"], c["value"], c["last_value"], c["done"], c["bonus"]
    ok = lambda **kw: compute_advantages(**dict(dict(rew=rew, value=value, last_value=last, done=done, bonus=bonus), **kw))  # noqa: E731
    ok()
    bad = [dict(rew=rew.to(torch.int64)), dict(rew=rew.numpy()), dict(value=value.to(torch.float64)), dict(value=None),
           dict(value=value[:5]), dict(value=value.transpose(1, 2)), dict(done=done.to(torch.int32)), dict(last_value=last[0]),
           dict(last_value=last.to(torch.float64)), dict(bonus=bonus.to(torch.float64)), dict(bonus=bonus[:, :1]),
           dict(gamma=float("nan")), dict(lambda_=float("inf")), dict(bonus_weight=float("nan")), dict(n_steps=0), dict(n_steps=7),
           dict(step0=-1), dict(use_gae=True, use_critic=False), dict(out=(torch.empty(6, 2, 3),)),
           dict(out=(torch.empty(6, 2, 3), torch.empty(6, 2, 2))),
           dict(out=(torch.empty(6, 2, 3), torch.empty(6, 2, 3, dtype=torch.float64)))]
    for kw in bad:
        with pytest.raises(ValueError):
            ok(**kw)
    same = torch.empty(6, 2, 3)
    with pytest.raises(ValueError):
        ok(out=(same, same))
    with pytest.raises(ValueError):
        compute_advantages(torch.zeros((0, 3), dtype=torch.int32), torch.zeros((0, 3)))
    adv, vt = compute_advantages(rew[:, 0, 0].contiguous(), value[:, 0, 0].contiguous())     # [R]: one trajectory
    assert adv.shape == (6,)


def _call(L, **kw):
    one = C.c_void_p(64)                                         # never dereferenced: the checks come before any device call
    a = dict(rew=one, bonus=None, bonus_weight=1.0, value=one, done=None, last_value=None, lanes=4, ring=8, step0=0, n_steps=8,
             gamma=0.99, lambda_=0.95, flags=_capi.SSD_ADV_GAE | _capi.SSD_ADV_CRITIC, advantages=one, value_targets=one,
             device_id=0, stream=None)
    a.update(kw)
    return L.ssd_advantages(a["rew"], a["bonus"], a["bonus_weight"], a["value"], a["done"], a["last_value"], a["lanes"], a["ring"],
                            a["step0"], a["n_steps"], a["gamma"], a["lambda_"], a["flags"], a["advantages"], a["value_targets"],
                            a["device_id"], a["stream"])


@pytest.mark.parametrize("kw,word", [
    (dict(lanes=0), b"lanes"), (dict(ring=0), b"ring"), (dict(n_steps=0), b"n_steps"), (dict(n_steps=9), b"n_steps > ring"),
    (dict(step0=-1), b"step0"), (dict(rew=None), b"rew"), (dict(value=None), b"value"),
    (dict(value=None, flags=_capi.SSD_ADV_CRITIC), b"value"), (dict(advantages=None), b"advantages"),
    (dict(value_targets=None), b"value_targets"), (dict(gamma=float("nan")), b"gamma"), (dict(gamma=float("inf")), b"gamma"),
    (dict(lambda_=float("-inf")), b"lambda"), (dict(lambda_=float("nan")), b"lambda"), (dict(flags=4), b"flag"),
    (dict(flags=_capi.SSD_ADV_GAE), b"critic"), (dict(bonus=C.c_void_p(64), bonus_weight=float("nan")), b"bonus_weight")])
def test_abi_rejects_bad_arguments_before_any_device_call(kw, word):
    L = _capi.lib()
    assert _call(L, **kw) == _capi.SSD_E_INVALID
    assert word in L.ssd_advantages_last_error()


def test_abi_without_a_device_fails_cleanly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = _capi.lib()
    assert _call(L) == _capi.SSD_E_DEVICE
    assert b"no HIP device" in L.ssd_advantages_last_error()
    with pytest.raises(_capi.SsdError):
        _capi.advantages_check(_capi.SSD_E_DEVICE)


def test_symbols_header_and_export():
    import sequential_social_dilemma_games_amd as pkg
    assert {"ssd_advantages", "ssd_advantages_last_error"} <= set(_capi.SYMBOLS)
    header = open(os.path.join(REPO, "include", "ssd.h")).read()
    assert re.search(r"int ssd_advantages\(const int32_t \*rew, const float \*bonus, double bonus_weight,", header)
    assert "const char *ssd_advantages_last_error(void);" in header
    for name in ("SSD_ADV_GAE", "SSD_ADV_CRITIC"):
        m = re.search(r"\b%s\s*=\s*1u << (\d)" % name, header)
        assert m and getattr(_capi, name) == 1 << int(m.group(1)), name
    assert pkg.compute_advantages is compute_advantages
    assert _capi.lib().ssd_abi_version() == 6
