"""Batch moments on the device (csrc/ssd_moments.hip; include/ssd.h, BATCH MOMENTS): ssd_standardize and
ssd_explained_variance against the tests' restatement of the header's summation order (moments_ref.py) bit for bit -- out,
moments and the explained variance -- at the per-set counts around W, the elements a workgroup takes per pass, and at 255 to
513 chunks per set, where the kernels add the partials in stages of 256; the ring rows, in place, the second pass, the edges
of the explained variance; and SSDVectorEnv.sample(..., standardize=True) and one PPO loss on standardised advantages end to
end."""
import copy

import numpy as np
import pytest
import torch

import moments_ref as M
from moments_ref import W, same_bits, same_bits_or_nan
from ppo_ref import HYPER, make_inputs, make_policy
from sequential_social_dilemma_games_amd import ConvFCPolicy, ppo_loss
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd.policy import PPO_STATS, ppo_terms
from sequential_social_dilemma_games_amd.postprocessing import explained_variance, standardize_advantages
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv
from test_ppo_loss_gpu import _check_against_reference          # the bound of the existing ppo_loss tests, as it is

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
COUNTS = [1, 2, W - 1, W, W + 1, 3 * W + 7]                      # per-set elements n; lanes = num_sets, so n_steps = n


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)              # (a copy: the shared inputs are read-only)


_inputs = {}


def _input(n, P):
    """x [n, P] and its restatement, computed once and left alone."""
    if (n, P) not in _inputs:
        x = M.noise(100 * P + n % 97, (n, P), scale=2.0, offset=0.25)
        pred = (x * np.float32(0.5) + M.noise(7, (n, P), scale=0.3)).astype(np.float32)
        _inputs[n, P] = (x, pred) + M.standardize_ref(x, num_sets=P) + (M.explained_variance_ref(x, pred, num_sets=P),)
        for a in _inputs[n, P]:
            a.setflags(write=False)
    return _inputs[n, P]


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("n", COUNTS)
def test_device_equals_the_restatement(n, P):
    x, pred, want, want_m, want_ev = _input(n, P)
    out, moments = standardize_advantages(_dev(x), num_sets=P, return_moments=True)
    ev = explained_variance(_dev(x), _dev(pred), num_sets=P)
    out, moments, ev = out.cpu().numpy(), moments.cpu().numpy(), ev.cpu().numpy()
    assert same_bits(moments, want_m), (moments, want_m)
    assert same_bits(out, want), np.argwhere(M.bits(out) != M.bits(want))[:5]
    assert same_bits_or_nan(ev, want_ev), (ev, want_ev)       # (n = 1: both variances are 0, and 0 / 0 is a NaN)


@pytest.mark.parametrize("n,P", [(1, 1), (1, 5), (W + 1, 5)])
def test_one_element_and_constant_sets_are_exactly_zero(n, P):
    """std = 0 takes the min_std branch: a float32 constant adds up exactly in float64, so the mean is the constant itself."""
    x = np.full((n, P), 3.7, np.float32)
    if n == 1:
        x = x * np.arange(1, P + 1, dtype=np.float32)             # one element per set, each its own value
    out, moments = standardize_advantages(_dev(x), num_sets=P, return_moments=True)
    assert same_bits(out.cpu().numpy(), np.zeros_like(x))
    m = moments.cpu().numpy()
    assert same_bits(m, M.standardize_ref(x, num_sets=P)[1]) and np.array_equal(m[:, 0], x[0].astype(np.float64)) and not m[:, 1].any()


@pytest.mark.parametrize("P", [1, 5, 13, 65])
def test_lanes_65_and_a_ring_with_wrap(P):
    """lanes = 65 = 5 x 13, no multiple of a wave; ring = 7, step0 = 5, n_steps = 4: slots 5, 6, 0, 1.  Slots outside the call
    keep their fill pattern out of place, and their values in place; in place equals out of place."""
    x = M.noise(21, (7, 13, 5), scale=1.5, offset=-1.0)
    want, want_m = M.standardize_ref(x.reshape(7, 65), num_sets=P, step0=5, n_steps=4)
    want = want.reshape(x.shape)
    fill = torch.full((7, 13, 5), 9.0, device=DEV)
    out, moments = standardize_advantages(_dev(x), num_sets=P, step0=5, n_steps=4, out=fill, return_moments=True)
    assert out is fill and same_bits(moments.cpu().numpy(), want_m)
    got = out.cpu().numpy()
    assert same_bits(got[[5, 6, 0, 1]], want[[5, 6, 0, 1]]) and np.all(got[2:5] == 9.0)
    t = _dev(x)
    assert standardize_advantages(t, num_sets=P, step0=5, n_steps=4, out=t) is t
    assert same_bits(t.cpu().numpy(), want)                      # (want holds x in the rows outside the call)
    fresh = standardize_advantages(_dev(x), num_sets=P, step0=5 + 7 * 3, n_steps=4).cpu().numpy()     # step0 past the ring: mod
    assert same_bits(fresh[[5, 6, 0, 1]], want[[5, 6, 0, 1]]) and not fresh[2:5].any()
    pred = M.noise(22, x.shape)
    ev = explained_variance(_dev(x), _dev(pred), num_sets=P, step0=5, n_steps=4).cpu().numpy()
    assert same_bits_or_nan(ev, M.explained_variance_ref(x.reshape(7, 65), pred.reshape(7, 65), num_sets=P, step0=5, n_steps=4))
    whole = standardize_advantages(_dev(x), num_sets=P).cpu().numpy()                                 # all 7 rows, no wrap
    assert same_bits(whole, M.standardize_ref(x.reshape(7, 65), num_sets=P)[0].reshape(x.shape))


def test_in_place_equals_out_of_place_over_several_workgroups():
    x = _input(3 * W + 7, 5)[0]
    t = _dev(x)
    apart = standardize_advantages(t, num_sets=5)
    assert apart.data_ptr() != t.data_ptr() and torch.equal(t, _dev(x))        # the input is left alone
    standardize_advantages(t, num_sets=5, out=t)
    assert same_bits(t.cpu().numpy(), apart.cpu().numpy())


# ------------------------------------------------------------------------- past 256 chunks: the stages of combine()
# The kernels add the chunk partials of a set 256 at a time from LDS: a full stage and a short one are two branches, and LDS is
# reused from stage to stage and from quantity to quantity.  The counts above reach four chunks.  `moments` is float64 and
# pins the order; `out`, a float32, hides a wrong one (moments_ref.STAGE_CASES has how the inputs were chosen).
BIG = M.STAGE_CASES[3]                                            # one set of 513 chunks: two full stages and a short one
THREE = M.STAGE_CASES[4]                                          # three sets of 257 chunks: a full stage and one partial


@pytest.mark.parametrize("P,n,seed", M.STAGE_CASES, ids=M.STAGE_IDS)
def test_device_equals_the_restatement_at_the_stage_boundaries(P, n, seed):
    x, pred, want, want_m, want_ev = M.stage_input(P, n, seed)
    a, b = _dev(x), _dev(pred)
    out, moments = standardize_advantages(a, num_sets=P, return_moments=True)
    ev = explained_variance(a, b, num_sets=P)
    out2, moments2 = standardize_advantages(a, num_sets=P, return_moments=True)
    ev2 = explained_variance(a, b, num_sets=P)
    out, moments, ev = out.cpu().numpy(), moments.cpu().numpy(), ev.cpu().numpy()
    assert same_bits(moments, want_m), (moments, want_m)
    assert same_bits(out, want), np.argwhere(M.bits(out) != M.bits(want))[:5]
    assert same_bits(ev, want_ev), (ev, want_ev)
    for u, v in ((out, out2), (moments, moments2), (ev, ev2)):    # a second call gives the same bits
        assert same_bits(u, v.cpu().numpy())


def test_the_wrap_inside_a_late_chunk():
    """[260, 4099], step0 = 130, n_steps = 257: 258 chunks, and split = 130 x 4099 = 130 W + 130 x 3 falls in chunk 130 at
    offset 390 = 1 x 256 + 134 -- item 1 of thread 134, whose sixteen elements so come from both ends of the ring."""
    R, L, step0, K = 260, 4099, 130, 257
    assert -(-(K * L) // W) == 258 and divmod((R - step0) * L, W) == (130, 256 + 134)
    x, pred = M.noise(31, (R, L), scale=2.0, offset=0.25), M.noise(32, (R, L))
    want, want_m = M.standardize_ref(x, step0=step0, n_steps=K)
    inside = M.call_rows(R, step0, K)
    outside = sorted(set(range(R)) - set(inside))
    assert outside == [127, 128, 129]
    fill = torch.full((R, L), 9.0, device=DEV)
    out, moments = standardize_advantages(_dev(x), step0=step0, n_steps=K, out=fill, return_moments=True)
    got = out.cpu().numpy()
    assert out is fill and same_bits(moments.cpu().numpy(), want_m)
    assert same_bits(got[inside], want[inside]) and np.all(got[outside] == 9.0)
    t = _dev(x)
    assert standardize_advantages(t, step0=step0, n_steps=K, out=t) is t
    assert same_bits(t.cpu().numpy(), want)                      # (want holds x in the rows outside the call)
    past, past_m = standardize_advantages(_dev(x), step0=step0 + R * 3, n_steps=K, return_moments=True)   # step0 past the ring: mod
    past = past.cpu().numpy()
    assert same_bits(past[inside], want[inside]) and not past[outside].any() and same_bits(past_m.cpu().numpy(), want_m)
    ev = explained_variance(_dev(x), _dev(pred), step0=step0, n_steps=K).cpu().numpy()
    assert same_bits(ev, M.explained_variance_ref(x, pred, step0=step0, n_steps=K))


def test_the_scratch_on_entry_does_not_matter():
    """The 513-chunk call once; NaN in every scratch tensor the package holds; a one-chunk call, which has another scratch size;
    then the big call and the big explained variance give their bits again."""
    from sequential_social_dilemma_games_amd import postprocessing
    P, n, seed = BIG
    x, pred, want, want_m, want_ev = M.stage_input(P, n, seed)
    a, b = _dev(x), _dev(pred)
    standardize_advantages(a, num_sets=P)
    explained_variance(a, b, num_sets=P)
    torch.cuda.synchronize()
    assert len(postprocessing._moments_scratch) >= 1
    for buf in postprocessing._moments_scratch.values():
        buf.fill_(float("nan"))
    small = _input(W, 1)
    got = standardize_advantages(_dev(small[0]), num_sets=1)
    assert same_bits(got.cpu().numpy(), small[2])
    assert len({buf.numel() for buf in postprocessing._moments_scratch.values()}) >= 2
    out, moments = standardize_advantages(a, num_sets=P, return_moments=True)
    ev = explained_variance(a, b, num_sets=P)
    assert same_bits(moments.cpu().numpy(), want_m) and same_bits(out.cpu().numpy(), want) and same_bits(ev.cpu().numpy(), want_ev)


def test_in_place_equals_out_of_place_at_513_chunks():
    P, n, seed = BIG
    x, _, want, _, _ = M.stage_input(P, n, seed)
    t = _dev(x)
    apart = standardize_advantages(t, num_sets=P)
    assert apart.data_ptr() != t.data_ptr() and torch.equal(t, _dev(x))        # the input is left alone
    standardize_advantages(t, num_sets=P, out=t)
    assert same_bits(t.cpu().numpy(), apart.cpu().numpy()) and same_bits(t.cpu().numpy(), want)


def test_one_constant_set_among_three_at_257_chunks():
    """A float32 constant adds up exactly through every stage, so a stray or a missing partial of that set shows as a mean
    that is not the constant, a std or an `out` that is not 0; the other two sets are the restatement's as they were."""
    P, n, seed = THREE
    x0, _, want0, want_m0, _ = M.stage_input(P, n, seed)
    x = x0.copy()
    x[:, 1] = np.float32(3.7)
    out, moments = standardize_advantages(_dev(x), num_sets=P, return_moments=True)
    out, moments = out.cpu().numpy(), moments.cpu().numpy()
    assert same_bits(out[:, 1], np.zeros(n, np.float32))
    assert same_bits(moments[1], np.array([np.float64(np.float32(3.7)), 0.0]))
    assert same_bits(out[:, [0, 2]], want0[:, [0, 2]]) and same_bits(moments[[0, 2]], want_m0[[0, 2]])


def test_the_second_pass_at_a_large_offset():
    """x = 1e4 + 1e-2 noise.  The device meets the derived bound against the independent float64 check, and equals the
    restatement.  The one-pass form does not meet it, which is what pins the second pass -- in NumPy, float64 throughout:
        v = x.astype(np.float64); mean = v.sum() / v.size
        one_pass = (v - mean) / max(1e-4, np.sqrt((v * v).sum() / v.size - mean * mean))
    x^2 is about 1e8, so E[x^2] and mean^2 carry an absolute error of about 1e8 * 2^-53 = 1e-8 each, against a variance of 1e-4:
    a relative error of 1e-4 in the variance, 5e-5 in the standard deviation and so about 1e-4 in an `out` of 2 or 3, where the
    bound is 3e-6 (n * 2^-53 * 1e4 / 1e-2 for the mean's error, the dominant term, twice).  test_moments_cpu.py asserts both."""
    P = 5
    x = M.noise(3, (3 * W + 7, P), scale=1e-2, offset=1e4)
    out = standardize_advantages(_dev(x), num_sets=P).cpu().numpy()
    want = M.independent(x, num_sets=P)[0]
    for p in range(P):
        v = x[:, p].astype(np.float64)
        err, lim = np.abs(out[:, p].astype(np.float64) - want[:, p]), M.out_bound(v)
        print("set %d max err %.3e bound there %.3e" % (p, err.max(), lim[np.argmax(err)]))
        assert np.all(err <= lim)
    assert same_bits(out, M.standardize_ref(x, num_sets=P)[0])


def test_one_huge_value_per_set():
    x = M.noise(6, (W + 1, 5))
    x[17] = 1e30
    out, moments = standardize_advantages(_dev(x), num_sets=5, return_moments=True)
    want, want_m = M.standardize_ref(x, num_sets=5)
    assert same_bits(out.cpu().numpy(), want) and same_bits(moments.cpu().numpy(), want_m)
    assert np.isfinite(want).all() and want[17].min() > 60.0     # sqrt(n) or so: the one value that stands out


def test_explained_variance_edges():
    y = M.noise(11, (W + 1, 5), scale=4.0)
    ev = lambda a, b: explained_variance(_dev(a), _dev(b), num_sets=5).cpu().numpy()   # noqa: E731
    assert same_bits(ev(y, y), np.ones(5, np.float32))                               # pred == y: exactly 1
    assert same_bits(ev(y, -y), np.full(5, -1.0, np.float32))                        # 1 - 4 = -3: exactly -1 by the clamp
    const = np.full_like(y, 2.0)
    assert same_bits(ev(const, y), np.full(5, -1.0, np.float32))                     # var(y) = 0 < var(y - pred): -inf, so -1
    assert np.isnan(ev(const, const + 1)).all()                                      # var(y) = 0 = var(y - pred): 0 / 0
    mixed = y.copy()
    mixed[:, 2] = 2.0                                                                # one constant set among the others
    got, want = ev(mixed, y * np.float32(0.5)), M.explained_variance_ref(mixed, y * np.float32(0.5), num_sets=5)
    assert same_bits(got, want) and got[2] == -1.0 and np.all(got[[0, 1, 3, 4]] > 0.5)


def test_two_calls_give_identical_bits():
    x, pred = _input(3 * W + 7, 5)[:2]
    a, b = _dev(x), _dev(pred)
    o1, m1 = standardize_advantages(a, num_sets=5, return_moments=True)
    e1 = explained_variance(a, b, num_sets=5)
    o2, m2 = standardize_advantages(a, num_sets=5, return_moments=True)
    e2 = explained_variance(a, b, num_sets=5)
    for u, v in ((o1, o2), (m1, m2), (e1, e2)):
        assert same_bits(u.cpu().numpy(), v.cpu().numpy())


def test_device_argument_checks():
    x = _dev(M.noise(1, (4, 5)))
    with pytest.raises(ValueError, match="out"):
        standardize_advantages(x, num_sets=5, out=torch.empty(4, 5))
    with pytest.raises(ValueError, match="pred"):
        explained_variance(x, x.cpu(), num_sets=5)


# ---------------------------------------------------------------------------------------------------- the adapter
def test_sample_with_standardize():
    """sample(policy, 8, gamma=0.99, lambda_=0.95, standardize=True) equals standardize_advantages of the standardize=False
    call's advantages, both engines seeded alike, and leaves value_targets as they were; per set the result's float64 mean is
    0 and its std 1 within the derived bound.  E = 8, N = 5: a fragment of more than one step needs num_envs * num_agents to
    be a multiple of 4, so 8 envs are the nearest size to 6 that sample() accepts; 40 lanes are no multiple of a wave either."""
    E, N, steps = 8, 5, 8
    pol = ConvFCPolicy(8, N, seed=3).to(DEV)
    with torch.no_grad():
        pol.value_w.mul_(50.0)                                   # values that differ from row to row: a std far above min_std

    def batch(**kw):
        env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=1000, seed=41)
        env.reset()
        return env, env.sample(pol, steps, gamma=0.99, lambda_=0.95, **kw)

    _, plain = batch()
    env, std = batch(standardize=True)
    assert set(std) == set(plain)
    for k in plain:
        if k != "advantages":
            assert torch.equal(plain[k], std[k]), k
    assert same_bits(std["value_targets"].cpu().numpy(), plain["value_targets"].cpu().numpy())
    want = standardize_advantages(plain["advantages"], num_sets=pol.num_sets)
    assert same_bits(std["advantages"].cpu().numpy(), want.cpu().numpy())
    raw = plain["advantages"].cpu().numpy()
    assert same_bits(want.cpu().numpy(), M.standardize_ref(raw.reshape(steps, E * N), num_sets=N)[0].reshape(raw.shape))
    got = std["advantages"].cpu().numpy().reshape(-1, N).astype(np.float64)
    for p in range(N):
        v = raw.reshape(-1, N)[:, p].astype(np.float64)
        assert np.std(v) > 1e-2, "a condition on the input: the set's std is far from min_std"
        e_o = M.bound(v)[2]
        e = e_o + M.f32_rounding(got[:, p], e_o)                 # every element's distance from the exact standardisation,
        n = v.size                                               # whose mean is 0 and whose std is 1
        mean_lim = e.mean() + M.g(n) * np.abs(got[:, p]).mean()  # ... and np.mean's own sum
        std_lim = np.sqrt((e * e).mean()) + M.g(n + 4) + 2.0 * M.U          # std is 1-Lipschitz in the rms; np.std's own error
        print("set %d mean %.3e (bound %.3e) std - 1 %.3e (bound %.3e)" % (p, got[:, p].mean(), mean_lim, got[:, p].std() - 1.0, std_lim))
        assert abs(got[:, p].mean()) <= mean_lim and abs(got[:, p].std() - 1.0) <= std_lim
    with pytest.raises(ValueError, match="give a gamma"):
        env.sample(pol, steps, standardize=True)


def _terms_loss(pol, t, h, first, dtype, device):
    """policy.ppo_terms under torch autograd on a copy of pol in dtype on device -> (loss, stats, grads)."""
    pol = copy.deepcopy(pol).to(device=device, dtype=dtype)
    pol.zero_grad()
    t = {k: v.to(device) for k, v in t.items()}
    logits, value = pol(torch.cat([first.to(device).unsqueeze(0), t["obs"][:-1]]))
    hyper = tuple(h[k] for k in ("clip_param", "vf_clip_param", "vf_loss_coeff", "entropy_coeff", "kl_coeff"))
    means = [x.reshape(-1, pol.num_sets).mean(0) for x in ppo_terms(logits, value, t, *hyper)]
    loss = means[0].sum()
    loss.backward()
    return (loss.detach(), {k: m.detach() for k, m in zip(PPO_STATS, means)},
            {name: getattr(pol, name).grad.detach().clone() for name, _, _ in pol.layout()})


def test_ppo_loss_on_standardised_advantages():
    """One end-to-end step: advantages on another scale (37 x + 12) standardised on the device, then ppo_loss on them against
    policy.ppo_terms in float64 torch on the same tensors, at the bound of the existing ppo_loss tests (torch's own float32 on
    the device as the yardstick)."""
    P, steps, E, N = 5, 6, 7, 5
    pol = make_policy(8, P, seed=51)
    t, first = make_inputs(pol, steps, E, N, seed=151)
    raw = (t["advantages"] * 37.0 + 12.0).contiguous()
    adv = standardize_advantages(raw.to(DEV), num_sets=P)
    assert same_bits(adv.cpu().numpy(), M.standardize_ref(raw.numpy().reshape(steps, -1), num_sets=P)[0].reshape(raw.shape))
    t["advantages"] = adv.cpu()
    loss64, stats64, g64 = _terms_loss(pol, t, HYPER, first, torch.float64, "cpu")
    loss32, stats32, g32 = _terms_loss(pol, t, HYPER, first, torch.float32, DEV)
    dpol = copy.deepcopy(pol).to(DEV)
    loss, stats = ppo_loss(dpol, {k: v.to(DEV) for k, v in t.items()}, obs_first=first.to(DEV), **HYPER)
    loss.backward()
    g = {name: getattr(dpol, name).grad.detach().clone() for name, _, _ in dpol.layout()}
    _check_against_reference(g, g32, g64, "standardised grad")
    _check_against_reference(stats, stats32, stats64, "standardised stat")
    _check_against_reference({"loss": loss.detach()}, {"loss": loss32}, {"loss": loss64}, "standardised loss")
