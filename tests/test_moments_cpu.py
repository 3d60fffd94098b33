"""Batch moments without a device (include/ssd.h, BATCH MOMENTS): the tests' restatement of the header's
summation order against an independent float64 check within the bound moments_ref derives, the package's host path against
the restatement bit for bit (at 255 to 513 chunks per set too, with inputs that tell five wrong orders of the across-chunk
sum from the right one), every refusal by its words, update_kl_coeff at its thresholds, and the ABI block."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import moments_ref as M
from moments_ref import W, same_bits, same_bits_or_nan
from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd.postprocessing import explained_variance, standardize_advantages, update_kl_coeff

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, x) with x [R, L]; the per-set counts are those of the GPU suite
INPUTS = [("unit", 1, M.noise(1, (W + 1, 1))),
          ("five_sets", 5, M.noise(2, (3 * W + 7, 5), scale=3.0, offset=-0.5)),
          ("offset_1e4", 5, M.noise(3, (3 * W + 7, 5), scale=1e-2, offset=1e4)),
          ("lanes65", 5, M.noise(4, (7, 65), scale=0.1, offset=2.0)),
          ("two", 1, M.noise(5, (2, 1)))]


def _huge():
    x = M.noise(6, (W + 1, 5))
    x[17] = 1e30                                                 # one value per set huge beside small ones
    return x


INPUTS.append(("huge", 5, _huge()))


@pytest.mark.parametrize("name,P,x", INPUTS, ids=[c[0] for c in INPUTS])
def test_restatement_meets_the_derived_bound_against_the_independent_check(name, P, x):
    out, moments = M.standardize_ref(x, num_sets=P)
    want, mean, std = M.independent(x, num_sets=P)
    got = M.sets_of(out, P, 0, x.shape[0]).astype(np.float64)
    for p in range(P):
        v = M.sets_of(x, P, 0, x.shape[0])[:, p].astype(np.float64)
        e_m, e_s, _ = M.bound(v)
        assert abs(moments[p, 0] - mean[p]) <= 2.0 * e_m, (p, moments[p, 0], mean[p], e_m)
        assert abs(moments[p, 1] - std[p]) <= 2.0 * e_s, (p, moments[p, 1], std[p], e_s)
        err, lim = np.abs(got[:, p] - want[:, p]), M.out_bound(v)
        assert np.all(err <= lim), (p, float(err.max()), float(lim[np.argmax(err - lim)]))


def test_the_one_pass_variance_misses_that_bound():
    """What pins the second pass: at x = 1e4 + 1e-2 noise, E[x^2] - mean^2 in float64 loses its variance's low digits to
    x^2 ~ 1e8 and is outside the bound the two-pass form meets."""
    x = M.noise(3, (3 * W + 7, 1), scale=1e-2, offset=1e4)
    v = x[:, 0].astype(np.float64)
    want = M.independent(x)[0][:, 0]
    mean = np.sum(v) / v.size
    one_pass = (v - mean) / max(1e-4, np.sqrt(np.sum(v * v) / v.size - mean * mean))
    lim = M.out_bound(v)
    assert not np.all(np.abs(one_pass - want) <= lim)
    two_pass = M.standardize_ref(x)[0][:, 0].astype(np.float64)
    assert np.all(np.abs(two_pass - want) <= lim)


def test_constant_and_single_inputs_are_exactly_zero():
    for x in (np.full((W + 1, 5), 3.7, np.float32), np.full((1, 5), -2.5, np.float32), np.full((1, 1), 1e4, np.float32)):
        out, moments = M.standardize_ref(x, num_sets=x.shape[1])
        assert same_bits(out, np.zeros_like(x))
        assert np.all(moments[:, 0] == x[0, 0]) and np.all(moments[:, 1] == 0.0)


@pytest.mark.parametrize("name,P,x", INPUTS, ids=[c[0] for c in INPUTS])
def test_host_path_equals_the_restatement(name, P, x):
    out, moments = standardize_advantages(torch.from_numpy(x), num_sets=P, return_moments=True)
    want, want_m = M.standardize_ref(x, num_sets=P)
    assert same_bits(out.numpy(), want) and same_bits(moments.numpy(), want_m)
    pred = (x * np.float32(0.75) + M.noise(9, x.shape, scale=0.1)).astype(np.float32)
    ev = explained_variance(torch.from_numpy(x), torch.from_numpy(pred), num_sets=P)
    assert same_bits_or_nan(ev.numpy(), M.explained_variance_ref(x, pred, num_sets=P))


@pytest.mark.parametrize("P,n,seed", M.STAGE_CASES, ids=M.STAGE_IDS)
def test_host_path_equals_the_restatement_at_the_stage_boundaries(P, n, seed):
    """255, 256, 257 and 513 chunks per set: the twin of the device test of that name."""
    x, pred, want, want_m, want_ev = M.stage_input(P, n, seed)
    assert -(-n // W) in (M.BLOCK - 1, M.BLOCK, M.BLOCK + 1, 2 * M.BLOCK + 1) and x.shape == (n, P)
    x, pred = torch.tensor(x), torch.tensor(pred)                # (copies: the shared inputs are read-only)
    out, moments = standardize_advantages(x, num_sets=P, return_moments=True)
    assert same_bits(moments.numpy(), want_m), (moments.numpy(), want_m)
    assert same_bits(out.numpy(), want)
    ev = explained_variance(x, pred, num_sets=P)
    assert same_bits(ev.numpy(), want_ev) and np.isfinite(want_ev).all()


@pytest.mark.parametrize("P,n,seed", M.STAGE_CASES, ids=M.STAGE_IDS)
def test_the_stage_inputs_tell_a_wrong_order_from_the_right_one(P, n, seed):
    """`moments` is what pins the across-chunk order on the device, so for every set of every input each wrong order that can
    differ at its chunk count changes the bits of the mean, and -- from the right mean, with S2 alone added in that order -- of
    the std: all five at 513 chunks; below, the reversed one and the two ways of letting each wave add its 64 partials (the
    four sub-totals one after the other onto the sum, or among themselves first).  Sub-totals of 256 are the contract's own
    order up to 257 chunks, which is asserted too."""
    x, _, _, want_m, _ = M.stage_input(P, n, seed)
    chunks = -(-n // W)
    orders = list(M.WRONG_ORDERS) if chunks > 2 * M.BLOCK else ["reversed", "subtotals_of_64", "waves_then_pairs"]
    for p in range(P):
        got = M.wrong_moments(x[:, p].astype(np.float64), orders + ["subtotals_of_256"])
        assert same_bits(np.array(got[None]), want_m[p])
        for o in orders:
            assert M.bits(got[o][0]) != M.bits(want_m[p, 0]), (p, o, "mean")
            assert M.bits(got[o][1]) != M.bits(want_m[p, 1]), (p, o, "std")
        if chunks <= M.BLOCK + 1:
            assert same_bits(np.array(got["subtotals_of_256"]), want_m[p])


def test_host_path_ring_rows_in_place_and_shapes():
    x = M.noise(10, (7, 13, 5))
    t = torch.from_numpy(x.copy())
    want, _ = M.standardize_ref(x.reshape(7, 65), num_sets=5, step0=5, n_steps=4)
    res = standardize_advantages(t, num_sets=5, step0=5, n_steps=4, out=t)                      # in place, with wrap
    assert res is t and same_bits(t.numpy().reshape(7, 65), want)
    assert same_bits(t.numpy()[2:5], x[2:5])                     # slots 2, 3, 4 are outside the call
    fresh = standardize_advantages(torch.from_numpy(x), num_sets=5, step0=5, n_steps=4)
    assert same_bits(fresh.numpy()[[5, 6, 0, 1]], t.numpy()[[5, 6, 0, 1]]) and not fresh.numpy()[2:5].any()
    one = standardize_advantages(torch.from_numpy(x[:, 0, 0].copy()))                         # [R]: one trajectory
    assert one.shape == (7,) and same_bits(one.numpy(), M.standardize_ref(x[:, 0, 0].copy())[0])
    lo = standardize_advantages(torch.from_numpy(x), min_std=100.0)                           # the min_std branch
    v = x.reshape(-1).astype(np.float64)
    assert same_bits(lo.numpy().reshape(-1), ((v - M.mean_var(v)[0]) / 100.0).astype(np.float32))


def test_explained_variance_by_hand_and_at_its_edges():
    y = M.noise(11, (W + 1, 5), scale=4.0)
    t = torch.from_numpy
    assert same_bits(explained_variance(t(y), t(y), num_sets=5).numpy(), np.ones(5, np.float32))          # pred == y: exactly 1
    assert same_bits(explained_variance(t(y), t(-y), num_sets=5).numpy(), np.full(5, -1.0, np.float32))   # 1 - 4 clamps to -1
    const = np.full_like(y, 2.0)
    assert same_bits(explained_variance(t(const), t(y), num_sets=5).numpy(), np.full(5, -1.0, np.float32))  # var(y) = 0 < var(d)
    assert np.isnan(explained_variance(t(const), t(const + 1), num_sets=5).numpy()).all()                 # 0 / 0
    y3, p3 = np.array([[1.0], [2.0], [3.0]], np.float32), np.array([[1.0], [2.0], [4.0]], np.float32)
    # var(y) = 2/3; y - pred = (0, 0, -1): mean -1/3, var = (1/9 + 1/9 + 4/9) / 3 = 2/9;  1 - (2/9) / (2/3) = 2/3
    assert abs(float(explained_variance(t(y3), t(p3))[0]) - 2.0 / 3.0) < 1e-6
    assert same_bits(explained_variance(t(y3), t(p3)).numpy(), M.explained_variance_ref(y3, p3))


def test_python_argument_checks_by_their_words():
    x = torch.from_numpy(M.noise(12, (6, 2, 5)))
    for kw, word in [(dict(adv=x.numpy()), "float32 tensor"), (dict(adv=x.double()), "float32"), (dict(adv=x.transpose(1, 2)), "contiguous"),
                     (dict(adv=torch.zeros((0, 5))), "holds no step"), (dict(num_sets=3), "divide"), (dict(num_sets=0), "num_sets"),
                     (dict(min_std=0.0), "min_std"), (dict(min_std=float("nan")), "min_std"), (dict(min_std=float("inf")), "min_std"),
                     (dict(n_steps=0), "n_steps"), (dict(n_steps=7), "n_steps"), (dict(step0=-1), "step0"),
                     (dict(out=torch.empty(6, 2, 4)), "out"), (dict(out=torch.empty(6, 2, 5, dtype=torch.float64)), "out")]:
        with pytest.raises(ValueError, match=word):
            standardize_advantages(**dict(dict(adv=x), **kw))
    for kw, word in [(dict(pred=x[:5]), "pred"), (dict(pred=x.double()), "pred"), (dict(targets=x.double()), "targets"),
                     (dict(num_sets=4), "divide"), (dict(n_steps=9), "n_steps"), (dict(step0=-2), "step0")]:
        with pytest.raises(ValueError, match=word):
            explained_variance(**dict(dict(targets=x, pred=x), **kw))


def _std(L, **kw):
    one = C.c_void_p(64)                                         # never dereferenced: the checks come before any device call
    a = dict(x=one, lanes=10, ring=8, step0=0, n_steps=8, num_sets=5, min_std=1e-4, scratch=one, moments=None, out=one,
             device_id=0, stream=None)
    a.update(kw)
    return L.ssd_standardize(a["x"], a["lanes"], a["ring"], a["step0"], a["n_steps"], a["num_sets"], a["min_std"], a["scratch"],
                             a["moments"], a["out"], a["device_id"], a["stream"])


def _ev(L, **kw):
    one = C.c_void_p(64)
    a = dict(y=one, pred=one, lanes=10, ring=8, step0=0, n_steps=8, num_sets=5, scratch=one, out=one, device_id=0, stream=None)
    a.update(kw)
    return L.ssd_explained_variance(a["y"], a["pred"], a["lanes"], a["ring"], a["step0"], a["n_steps"], a["num_sets"], a["scratch"],
                                    a["out"], a["device_id"], a["stream"])


BAD_SHARED = [(dict(lanes=0), b"lanes must be >= 1"), (dict(ring=0), b"ring must be >= 1"), (dict(n_steps=0), b"n_steps must be >= 1"),
              (dict(n_steps=9), b"n_steps > ring"), (dict(step0=-1), b"step0 must be >= 0"), (dict(num_sets=0), b"num_sets must be >= 1"),
              (dict(num_sets=3), b"num_sets must divide lanes"), (dict(num_sets=20), b"num_sets must divide lanes"),
              (dict(scratch=None), b"scratch is required"), (dict(scratch=C.c_void_p(68)), b"scratch must be aligned to 8 bytes")]


@pytest.mark.parametrize("kw,word", BAD_SHARED + [
    (dict(x=None), b"x and out are required"), (dict(out=None), b"x and out are required"),
    (dict(x=C.c_void_p(66)), b"aligned to 4 bytes"), (dict(out=C.c_void_p(65)), b"aligned to 4 bytes"),
    (dict(moments=C.c_void_p(68)), b"moments must be aligned to 8 bytes"),
    (dict(min_std=0.0), b"min_std must be finite and > 0"), (dict(min_std=-1.0), b"min_std must be finite and > 0"),
    (dict(min_std=float("nan")), b"min_std must be finite and > 0"), (dict(min_std=float("inf")), b"min_std must be finite and > 0")])
def test_standardize_abi_refuses_before_any_device_call(kw, word):
    L = _capi.lib()
    assert _std(L, **kw) == _capi.SSD_E_INVALID
    assert word in L.ssd_moments_last_error()


@pytest.mark.parametrize("kw,word", BAD_SHARED + [
    (dict(y=None), b"y, pred and out are required"), (dict(pred=None), b"y, pred and out are required"),
    (dict(out=None), b"y, pred and out are required"), (dict(pred=C.c_void_p(66)), b"aligned to 4 bytes")])
def test_explained_variance_abi_refuses_before_any_device_call(kw, word):
    L = _capi.lib()
    assert _ev(L, **kw) == _capi.SSD_E_INVALID
    assert word in L.ssd_moments_last_error()


def test_abi_without_a_device_fails_cleanly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = _capi.lib()
    assert _std(L) == _capi.SSD_E_DEVICE and b"no HIP device" in L.ssd_moments_last_error()
    assert _ev(L) == _capi.SSD_E_DEVICE and b"no HIP device" in L.ssd_moments_last_error()
    with pytest.raises(_capi.SsdError, match="batch-moments"):
        _capi.moments_check(_capi.SSD_E_DEVICE)


def test_update_kl_coeff_at_both_thresholds_and_on_them():
    t = 0.01
    assert update_kl_coeff(0.2, 0.0201, t) == 0.2 * 1.5          # above 2 * target
    assert update_kl_coeff(0.2, 0.02, t) == 0.2                  # exactly on it: unchanged
    assert update_kl_coeff(0.2, 0.0049, t) == 0.2 * 0.5          # below 0.5 * target
    assert update_kl_coeff(0.2, 0.005, t) == 0.2                 # exactly on it: unchanged
    assert update_kl_coeff(0.2, 0.01, t) == 0.2
    assert isinstance(update_kl_coeff(0.2, 0.01, t), float)
    got = update_kl_coeff(np.array([0.2, 0.2, 0.2, 1.0, 1.0]), np.array([0.03, 0.02, 0.001, 0.005, np.nextafter(0.005, 0)]), t)
    assert got.dtype == np.float64 and np.array_equal(got, np.array([0.2 * 1.5, 0.2, 0.1, 1.0, 0.5]))
    assert np.array_equal(update_kl_coeff(0.3, np.array([1.0, 0.0]), np.array([0.01, 0.01])), np.array([0.3 * 1.5, 0.15]))


def test_symbols_header_constants_and_export():
    import sequential_social_dilemma_games_amd as pkg
    assert set(_capi.MOMENTS_SYMBOLS) == {"ssd_standardize", "ssd_explained_variance", "ssd_moments_last_error"} <= set(_capi.SYMBOLS)
    header = open(os.path.join(REPO, "include", "ssd.h")).read()
    assert header.index("V-TRACE TARGETS --") < header.index("BATCH MOMENTS --") < header.index("WATERSHED PPO LOSS AND GRADIENTS --")
    assert re.search(r"int ssd_standardize\(const float \*x, int32_t lanes, int32_t ring, int32_t step0, int32_t n_steps, "
                     r"int32_t num_sets, double min_std,\s+double \*scratch, double \*moments, float \*out, int32_t device_id, "
                     r"void \*stream\);", header)
    assert re.search(r"int ssd_explained_variance\(const float \*y, const float \*pred, int32_t lanes, int32_t ring, int32_t step0, "
                     r"int32_t n_steps,\s+int32_t num_sets, double \*scratch, float \*out, int32_t device_id, void \*stream\);", header)
    assert "const char *ssd_moments_last_error(void);" in header
    for name in ("SSD_MOM_BLOCK", "SSD_MOM_ITEMS"):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == getattr(_capi, name), name
    assert re.search(r"#define SSD_MOM_CHUNK \(SSD_MOM_BLOCK \* SSD_MOM_ITEMS\)", header) and _capi.SSD_MOM_CHUNK == W == 4096
    assert re.search(r"#define SSD_MOM_SCRATCH_DOUBLES\(n_steps, lanes, num_sets\) \(4 \* \(int64_t\)\(num_sets\) \* "
                     r"SSD_MOM_CHUNKS\(n_steps, lanes, num_sets\)\)", header)
    for K, L, P in [(1, 1, 1), (1, 5, 5), (W, 5, 5), (W + 1, 5, 5), (4, 65, 5), (4096, 20480, 1), (4096, 20480, 5)]:
        chunks = -(-(K * (L // P)) // W)
        assert _capi.SSD_MOM_CHUNKS(K, L, P) == chunks and _capi.SSD_MOM_SCRATCH_DOUBLES(K, L, P) == 4 * P * chunks
    assert pkg.standardize_advantages is standardize_advantages and pkg.explained_variance is explained_variance
    assert pkg.update_kl_coeff is update_kl_coeff


def test_sample_standardizes_only_on_request():
    """(the refusal without a gamma needs an adapter, so a device: test_moments_gpu.py)"""
    import inspect
    from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv
    assert inspect.signature(SSDVectorEnv.sample).parameters["standardize"].default is False
