"""The host side of test_policy_shapes_gpu.py: that its exact constructions are right before they meet a kernel (the int64 bound
of the integer network; both constructions through the torch modules on the CPU, to the bit), and that its bounded cases would
catch a kernel that is wrong the way kernels go wrong at those shapes (the sensitivity tests: the float64 restatement is
perturbed, and the perturbation must exceed the acceptance bound of the very case the GPU file runs)."""
import numpy as np
import pytest
import torch

import policy_moa_ref
import policy_ref
import policy_shape_cases as cases
from gae_ref import same_bits
from sequential_social_dilemma_games_amd.policy import ConvFCPolicy, ConvMOAPolicy

INTEGER_SHAPES = [(3, 15), (1, 8)]          # (P, A) of test_policy_shapes_gpu.py::test_integer_network_is_exact


# ------------------------------------------------------------------------------------------------ the exact constructions
@pytest.mark.parametrize("P,A", INTEGER_SHAPES)
def test_integer_construction_stays_below_2_24(P, A):
    """What makes the integer test exact rests on the construction, not on the kernel: in int64, every prefix of every sum in k
    order, every prefix within fc1's two K halves (k < 508 and k >= 508, the halves the kernel adds through LDS), the halves'
    totals, and -- covering every other order and grouping, such as the kernel's two interleaved accumulators -- the sum of the
    terms' magnitudes plus the bias's are all below 2^24, so float32 holds each exactly.  And a dropped or doubled k of fc1 is
    visible: no term of fc1 is zero."""
    wi = cases.integer_weights(P, A)
    assert (wi["conv_w"] == 0).all() and (wi["conv_b"] > 0).all() and (wi["fc1_w"] != 0).all()
    lim = 2 ** 24
    for p in range(P):
        for depth, (h, w, b, z) in enumerate(cases.integer_layers(wi, p)):
            terms = h[:, None].astype(np.int64) * w.astype(np.int64)          # [K, J]
            assert np.abs(np.cumsum(terms, axis=0)).max() < lim
            assert (np.abs(terms).sum(axis=0) + np.abs(b)).max() < lim
            assert np.array_equal(terms.sum(axis=0) + b, z) and np.abs(z).max() < lim
            if depth == 0:
                assert (terms != 0).all()
                for half in (terms[:508], terms[508:]):
                    assert np.abs(np.cumsum(half, axis=0)).max() < lim
                assert np.array_equal(terms[:508].sum(axis=0) + terms[508:].sum(axis=0) + b, z)
            if depth < 2:
                assert (z > 0).any() and (z < 0).any(), "both branches of the ReLU"


@pytest.mark.parametrize("P,A", INTEGER_SHAPES)
def test_integer_construction_on_the_torch_module(P, A):
    B, N = 3, max(P, 2)
    wi = cases.integer_weights(P, A)
    el, ev, _ = cases.integer_expected(wi, B, N)
    obs = torch.from_numpy(cases.random_obs(np.random.default_rng(0), B, N))
    with torch.no_grad():
        lg, v = ConvFCPolicy(A, P).load_arrays(wi)(obs)
    assert same_bits(lg.numpy(), el.astype(np.float32)) and same_bits(v.numpy(), ev.astype(np.float32))
    # and the float64 restatement says the same integers
    rl, rv = policy_ref.forward({k: x.astype(np.float64) for k, x in wi.items()}, obs.numpy())
    assert np.array_equal(rl, el) and np.array_equal(rv, ev)


@pytest.mark.parametrize("sign", [1, -1])
def test_selector_construction_on_the_torch_module(sign):
    sets = cases.selector_sets()
    assert cases.selector_coverage(sets) == list(range(cases.FLAT))
    assert all(len(set(s["units"])) == cases.SELECTOR_OUTPUTS and all(k % 6 == s["f"] for k in s["ks"]) for s in sets)
    assert {(s["dy"], s["dx"], s["c"]) for s in sets} == {(a, b, c) for a in range(3) for b in range(3) for c in range(3)}
    rng = np.random.default_rng(sign + 1)
    part = sets[::5] + sets[-1:]                                # a sample of the sets (the GPU test runs all of them)
    obs_h = cases.random_obs(rng, 5, len(part))
    with torch.no_grad():
        lg, v = ConvFCPolicy(cases.SELECTOR_A, len(part)).load_arrays(cases.selector_weights(part, sign))(torch.from_numpy(obs_h))
    el, ev = cases.selector_expected(part, sign, obs_h)
    assert same_bits(lg.numpy(), el) and same_bits(v.numpy(), ev)
    assert (el > 0).any() and (el == 0).any()
    # the restatement agrees to float32's rounding of the one term
    rl, rv = policy_ref.forward(cases.selector_weights(part, sign), obs_h)
    assert np.abs(rl - el).max() < 1e-7 and np.abs(rv - ev).max() < 1e-7


# ----------------------------------------------------------------------------------------------------------- sensitivity
# A kernel that computes a perturbed function f' in float32 returns f' plus its own rounding, which the bound presumes to be
# within the bound itself.  So a perturbation with max |f' - f| >= 2 (4 et + 1e-6) on some asserted output cannot pass the case:
# its ek is at least twice the bound less its own rounding.  Each test asserts that factor of 2 and prints the factor it finds
# (et here is the torch module's float32 error on this CPU; on the device it is of the same size).
FACTOR = 2.0


def _factor(name, ref, pert, tor):
    """The largest, over the outputs a case asserts, of max |pert - ref| / (4 et + 1e-6)."""
    f = 0.0
    for r, p, t in zip(ref, pert, tor):
        et = float(np.abs(np.asarray(t, np.float64) - r).max())
        f = max(f, float(np.abs(np.asarray(p) - r).max()) / (4 * et + 1e-6))
    print("SENSITIVITY %s factor %.1f" % (name, f))
    return f


CONV_CASE = (17, 2, 2, 8)


def _conv_case():
    assert CONV_CASE in cases.CONV_CASES
    B, N, P, A = CONV_CASE
    w, obs = cases.conv_inputs(CONV_CASE)
    with torch.no_grad():
        tor = [x.numpy() for x in ConvFCPolicy(A, P).load_arrays(w)(torch.from_numpy(obs))]
    return w, obs, policy_ref.forward(w, obs), tor


def test_sensitivity_conv_fc():
    """fc1 without its last two rows (the peeled k-step dropped), fc1's halves meeting at the wrong k (one k-step of 4 rows
    counted by both halves, or by neither), set 0 used for every agent, and the ragged tile's one row taken from its neighbour:
    each exceeds the bound of test_conv_fc_against_restatement[B17-N2-P2-A8].  The fc1 perturbations depend on the weights and on
    which conv units are past their ReLU: on these inputs they clear the bound by a factor above 10^4, the smallest of this file
    (profiles/r11_policy_shapes/cpu_sensitivity.txt).  Whatever the weights, it is the tolerance-free selector test
    (test_selector_pins_every_flat_index) that pins k = 1012, 1013 and the boundary 507 | 508, and the integer test
    (test_integer_network_is_exact) that shows a dropped or doubled k."""
    w, obs, ref, tor = _conv_case()

    def edit(f):
        w2 = {k: x.copy() for k, x in w.items()}
        f(w2["fc1_w"])
        return policy_ref.forward(w2, obs)

    def zero(rows):
        def f(m):
            m[:, rows] = 0.0
        return f

    def double(rows):
        def f(m):
            m[:, rows] *= 2.0
        return f

    factors = [_factor("convfc fc1 rows 1012..1013 dropped", ref, edit(zero(slice(1012, 1014))), tor),
               _factor("convfc k-step 508..511 in neither half", ref, edit(zero(slice(508, 512))), tor),
               _factor("convfc k-step 504..507 in both halves", ref, edit(double(slice(504, 508))), tor),
               _factor("convfc set 0 for every agent", ref, policy_ref.forward({k: x[:1] for k, x in w.items()}, obs), tor)]
    shifted = [x.copy() for x in ref]
    for x in shifted:
        x[16] = x[15]
    factors.append(_factor("convfc ragged row from its neighbour", ref, shifted, tor))
    assert min(factors) >= FACTOR, factors


def _moa_case(case, monkeypatch, others=None):
    N, A, C, B, P = case
    assert case in cases.MOA_CASES
    w, obs, prev, state, starts, acts = cases.moa_inputs(case)
    ref = policy_moa_ref.forward(w, obs, prev, state, starts)
    with torch.no_grad():
        tor = ConvMOAPolicy(A, N, P, C).load_arrays(w)(torch.from_numpy(obs), torch.from_numpy(prev), torch.from_numpy(state),
                                                       torch.from_numpy(starts))
    pert = None
    if others is not None:
        monkeypatch.setattr(policy_moa_ref, "others", others)
        pert = policy_moa_ref.forward(w, obs, prev, state, starts)
    return ref, [t.numpy() for t in tor], pert


@pytest.mark.parametrize("case", [(11, 8, 64, 33, 11), (16, 15, 64, 17, 16)], ids=lambda c: "N%d" % c[0])
def test_sensitivity_moa_agent_order(case, monkeypatch):
    """The others in index order instead of the order of their ids as strings ('agent-10' < 'agent-2'): what id_key as the
    identity would compute.  It differs from N = 11 on, and exceeds the bound of test_moa_against_restatement at N = 11, 16."""
    N = case[0]
    index_order = lambda n: [[j for j in range(n) if j != i] for i in range(n)]          # noqa: E731
    assert index_order(N) != policy_moa_ref.others(N) and index_order(10) == policy_moa_ref.others(10)
    ref, tor, pert = _moa_case(case, monkeypatch, index_order)
    assert np.array_equal(pert[0], ref[0]) and np.array_equal(pert[1], ref[1])          # (the actions cell does not read them)
    assert _factor("moa index order N=%d" % N, ref, pert, tor) >= FACTOR


def test_sensitivity_moa_prediction_tile(monkeypatch):
    """One 16-column tile of the 225 prediction columns zeroed (a tile loop that stops short; an unwritten tile shows as the
    fill of policy_abi.py instead): every one of the 15 tiles, the ragged last one included, exceeds the bound at N = 16, A = 15."""
    case = (16, 15, 64, 17, 16)
    N, A = case[:2]
    ref, tor, _ = _moa_case(case, monkeypatch)
    factors = []
    for t in range(15):
        pert = [x.copy() for x in ref]
        flat = pert[3].reshape(pert[3].shape[:-2] + ((N - 1) * A,))
        flat[..., 16 * t:16 * t + 16] = 0.0
        pert[3] = flat.reshape(ref[3].shape)
        factors.append(_factor("moa prediction tile %d zeroed" % t, ref, pert, tor))
    assert min(factors) >= FACTOR, factors
