"""The refusals the four batch post-processing calls share (csrc/ssd_batch.hpp; ssd_advantages, ssd_vtrace, ssd_standardize,
ssd_explained_variance) and the Python checks ahead of them (postprocessing.py), by their whole text.  Every expected string is
a literal recorded from the library and the package as they were before the calls shared their host code: the ring rules word
for word in all four calls, which of two faults a call reports, the refusal without a device, and the Python messages.  No
device is needed: every refusal here comes before any device call."""
import ctypes as C

import pytest
import torch

from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd.postprocessing import compute_advantages, explained_variance, standardize_advantages, vtrace

ONE = C.c_void_p(64)                                             # never dereferenced: the checks come before any device call


def _adv(L, **kw):
    a = dict(rew=ONE, bonus=None, bonus_weight=1.0, value=ONE, done=None, last_value=None, lanes=10, ring=8, step0=0, n_steps=8,
             gamma=0.99, lambda_=0.95, flags=_capi.SSD_ADV_GAE | _capi.SSD_ADV_CRITIC, advantages=ONE, value_targets=ONE,
             device_id=0, stream=None)
    a.update(kw)
    return L.ssd_advantages(a["rew"], a["bonus"], a["bonus_weight"], a["value"], a["done"], a["last_value"], a["lanes"], a["ring"],
                            a["step0"], a["n_steps"], a["gamma"], a["lambda_"], a["flags"], a["advantages"], a["value_targets"],
                            a["device_id"], a["stream"])


def _vt(L, **kw):
    a = dict(rew=ONE, bonus=None, bonus_weight=1.0, value=ONE, rhos=ONE, done=None, bootstrap_value=None, lanes=10, ring=8, step0=0,
             n_steps=8, gamma=0.99, clip_rho=1.0, clip_pg=1.0, flags=0, vs=ONE, pg=ONE, device_id=0, stream=None)
    a.update(kw)
    return L.ssd_vtrace(a["rew"], a["bonus"], a["bonus_weight"], a["value"], a["rhos"], a["done"], a["bootstrap_value"], a["lanes"],
                        a["ring"], a["step0"], a["n_steps"], a["gamma"], a["clip_rho"], a["clip_pg"], a["flags"], a["vs"], a["pg"],
                        a["device_id"], a["stream"])


def _std(L, **kw):
    a = dict(x=ONE, lanes=10, ring=8, step0=0, n_steps=8, num_sets=5, min_std=1e-4, scratch=ONE, moments=None, out=ONE,
             device_id=0, stream=None)
    a.update(kw)
    return L.ssd_standardize(a["x"], a["lanes"], a["ring"], a["step0"], a["n_steps"], a["num_sets"], a["min_std"], a["scratch"],
                             a["moments"], a["out"], a["device_id"], a["stream"])


def _ev(L, **kw):
    a = dict(y=ONE, pred=ONE, lanes=10, ring=8, step0=0, n_steps=8, num_sets=5, scratch=ONE, out=ONE, device_id=0, stream=None)
    a.update(kw)
    return L.ssd_explained_variance(a["y"], a["pred"], a["lanes"], a["ring"], a["step0"], a["n_steps"], a["num_sets"], a["scratch"],
                                    a["out"], a["device_id"], a["stream"])


# call -> (the call with placeholder pointers, its family's last-error export)
CALLS = {"ssd_advantages": (_adv, "ssd_advantages_last_error"), "ssd_vtrace": (_vt, "ssd_vtrace_last_error"),
         "ssd_standardize": (_std, "ssd_moments_last_error"), "ssd_explained_variance": (_ev, "ssd_moments_last_error")}

RING = [(dict(lanes=0), b"lanes must be >= 1"), (dict(lanes=-3), b"lanes must be >= 1"),
        (dict(ring=0), b"ring must be >= 1"),
        (dict(n_steps=0), b"n_steps must be >= 1"),
        (dict(n_steps=9), b"n_steps > ring: a call reads each step's slot once"),
        (dict(step0=-1), b"step0 must be >= 0"),
        # two of the five at once: the first in the order lanes, ring, n_steps, n_steps > ring, step0
        (dict(lanes=0, ring=0), b"lanes must be >= 1"), (dict(ring=0, n_steps=0), b"ring must be >= 1"),
        (dict(n_steps=0, step0=-1), b"n_steps must be >= 1"), (dict(n_steps=9, step0=-1), b"n_steps > ring: a call reads each step's slot once")]


def _refused(call, kw):
    L = _capi.lib()
    fn, last_error = CALLS[call]
    rc = fn(L, **kw)
    return rc, getattr(L, last_error)()


@pytest.mark.parametrize("call", list(CALLS))
@pytest.mark.parametrize("kw,text", RING, ids=["-".join("%s=%d" % i for i in kw.items()) for kw, _ in RING])
def test_the_ring_refusals_are_the_same_words_in_all_four_calls(call, kw, text):
    assert _refused(call, kw) == (_capi.SSD_E_INVALID, text)


TWO_FAULTS = [
    # the ring comes before the pointers in ssd_advantages and ssd_vtrace ...
    ("ssd_advantages", dict(lanes=0, rew=None), b"lanes must be >= 1"),
    ("ssd_vtrace", dict(lanes=0, rew=None), b"lanes must be >= 1"),
    # ... and after the pointers, the alignment and min_std in the two moments calls
    ("ssd_standardize", dict(lanes=0, x=None), b"x and out are required"),
    ("ssd_standardize", dict(ring=0, min_std=0.0), b"min_std must be finite and > 0"),
    ("ssd_standardize", dict(n_steps=9, moments=C.c_void_p(68)), b"moments must be aligned to 8 bytes"),
    ("ssd_explained_variance", dict(lanes=0, y=None), b"y, pred and out are required"),
    ("ssd_explained_variance", dict(step0=-1, pred=C.c_void_p(66)), b"y, pred and out must be aligned to 4 bytes"),
    # the ring before the sets and the scratch
    ("ssd_explained_variance", dict(n_steps=0, scratch=C.c_void_p(68)), b"n_steps must be >= 1"),
    ("ssd_standardize", dict(step0=-1, num_sets=0), b"step0 must be >= 0"),
    ("ssd_explained_variance", dict(num_sets=3, scratch=None), b"num_sets must divide lanes: lane l belongs to set l % num_sets"),
    # flags before pointers, pointers before numbers
    ("ssd_advantages", dict(flags=8, rew=None), b"unsupported flag"),
    ("ssd_advantages", dict(step0=-1, flags=8), b"step0 must be >= 0"),
    ("ssd_advantages", dict(flags=_capi.SSD_ADV_GAE, advantages=None), b"generalised advantage estimation needs the critic: set both flags"),
    ("ssd_advantages", dict(value=None, gamma=float("nan")), b"value is required when the critic is used"),
    ("ssd_vtrace", dict(flags=1, value=None), b"unsupported flag"),
    ("ssd_vtrace", dict(rhos=None, clip_rho=0.0), b"rhos is required: the importance weights of the taken actions"),
    # numbers before the device
    ("ssd_advantages", dict(lambda_=float("inf"), device_id=-1), b"gamma and lambda must be finite"),
    ("ssd_vtrace", dict(clip_pg=-1.0, device_id=-1), b"clip_rho_threshold and clip_pg_rho_threshold must be > 0 (+inf: no clip)"),
]


@pytest.mark.parametrize("call,kw,text", TWO_FAULTS, ids=["%s-%s" % (c, "-".join(kw)) for c, kw, _ in TWO_FAULTS])
def test_which_of_two_faults_a_call_reports(call, kw, text):
    assert _refused(call, kw) == (_capi.SSD_E_INVALID, text)


@pytest.mark.parametrize("call", list(CALLS))
def test_without_a_device_good_arguments_are_refused_in_these_words(call):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _refused(call, {}) == (_capi.SSD_E_DEVICE, b"no HIP device available: this call has no CPU path")


# ---- the Python checks: R = 6, L = 2 * 5 ----

def _python_calls(device="cpu"):
    """name -> (function, its good keyword arguments, the name of the tensor that gives the call its shape)"""
    f32 = lambda: torch.zeros((6, 2, 5), dtype=torch.float32, device=device)   # noqa: E731
    rew = torch.zeros((6, 2, 5), dtype=torch.int32, device=device)
    return {"compute_advantages": (compute_advantages, dict(rew=rew, value=f32()), "rew"),
            "vtrace": (vtrace, dict(rew=rew, value=f32(), rhos=f32()), "rew"),
            "standardize_advantages": (standardize_advantages, dict(adv=f32(), num_sets=5), "adv"),
            "explained_variance": (explained_variance, dict(targets=f32(), pred=f32(), num_sets=5), "targets")}


FOUR = ["compute_advantages", "vtrace", "standardize_advantages", "explained_variance"]


def _message(name, device="cpu", **kw):
    fn, good, _ = _python_calls(device)[name]
    with pytest.raises(ValueError) as e:
        fn(**dict(good, **kw))
    return str(e.value)


@pytest.mark.parametrize("name", FOUR)
def test_python_ring_messages(name):
    assert _message(name, n_steps=0) == "n_steps (0) must be 1..6, the ring length: a call reads each slot once"
    assert _message(name, n_steps=7) == "n_steps (7) must be 1..6, the ring length: a call reads each slot once"
    assert _message(name, step0=-1) == "step0 must be 0..2^31 - 1"


@pytest.mark.parametrize("name,dtype", [("compute_advantages", "torch.int32"), ("vtrace", "torch.int32"),
                                        ("standardize_advantages", "torch.float32"), ("explained_variance", "torch.float32")])
def test_python_message_for_a_leading_tensor_that_is_not_contiguous(name, dtype):
    _, good, lead = _python_calls()[name]
    t = good[lead].transpose(1, 2)                               # [6, 5, 2], strides of [6, 2, 5]
    assert _message(name, **{lead: t}) == "%s must be a contiguous %s tensor of shape (6, 5, 2) on cpu" % (lead, dtype)


def test_python_message_for_one_tensor_as_both_outputs():
    t = torch.empty((6, 2, 5), dtype=torch.float32)
    for name in ("compute_advantages", "vtrace"):
        assert _message(name, out=(t, t)) == "out[0] and out[1] must be two tensors"
        assert _message(name, out=[t, t]) == "out[0] and out[1] must be two tensors"
    assert _message("compute_advantages", out=(t,)) == "out must be a pair (advantages, value_targets)"
    assert _message("vtrace", out=t) == "out must be a pair (vs, pg_advantages)"


@pytest.mark.parametrize("name", ["standardize_advantages", "explained_variance"])
def test_python_message_for_sets_that_do_not_divide_a_row(name):
    assert _message(name, num_sets=3) == ("num_sets (3) must be 1..65535 and divide the 10 trajectories of a row: trajectory l "
                                          "belongs to set l % num_sets")


@pytest.mark.parametrize("name", FOUR)
def test_python_message_for_tensors_on_neither_the_cpu_nor_a_gpu(name):
    assert _message(name, device="meta") == "the tensors must be on the CPU or on a GPU, not on meta"
