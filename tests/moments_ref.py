"""The tests' own statement of the batch moments (include/ssd.h, BATCH MOMENTS), in three parts.

1. The restatement: the header's summation order followed line by line in NumPy -- a thread's items one after the other, the
   workgroup's tree by halving, the chunk partials in their order -- with the header's own constants, read from the header.
   The device and the package's host path must agree with it bit for bit.
2. An independent float64 check, np.mean / np.std on float64 copies (pairwise sums, another order), and the error bound that
   separates the two, derived here from the arithmetic and from nothing the code under test returns.

The bound.  u = 2^-53.  A float64 sum of n terms, in any order, errs by at most g(n) * sum|x_i| with g(n) = n u / (1 - n u)
(Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4).  With A = mean|x_i|, per set:
  mean:  the sum, then one division:                          |d mean| <= e_m = (g(n) + u) * A * (1 + u)
  var:   the deviations are taken from the computed mean.  sum (x_i - mu - dm)^2 = sum (x_i - mu)^2 + n dm^2 exactly (the true
         deviations add up to 0), so the shift adds dm^2 to the variance; each term then carries three roundings (subtract,
         multiply, and one more for slack), the sum g(n), the division u:   |d var| <= e_v = e_m^2 + g(n + 4) * (var + e_m^2)
  std:   |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt|a - b|), then the root's own rounding:
                                                              |d std| <= e_s = min(e_v / std, sqrt(e_v)) * (1 + u) + u * std
  out:   o = (x - mu) / den with den = max(min_std, std), which moves by at most e_s (max is 1-Lipschitz); the numerator moves
         by e_m and carries two roundings (subtract, divide):
         |d o| <= e_o = (e_m + 2 u (|x - mu| + e_m)) / (den - e_s) + |x - mu| * e_s / (den * (den - e_s))
         and the one rounding to float32 adds 2^-24 * (|o| + e_o) + 2^-150 (half an ulp, or half the smallest subnormal).
3. The inputs at the stage boundaries of the across-chunk sum (255 to 513 chunks per set) and that sum in four orders the
   contract does not allow, which the inputs are chosen to tell from the right one.
Both the restatement and the independent check are float64 evaluations of the same two passes in some order, so each is
within e of the exact value and they are within 2 e of each other; the float32 rounding is counted once.
"""
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "ssd.h")).read()
BLOCK = int(re.search(r"#define SSD_MOM_BLOCK (\d+)", HEADER).group(1))
ITEMS = int(re.search(r"#define SSD_MOM_ITEMS (\d+)", HEADER).group(1))
W = BLOCK * ITEMS                                                # the elements of one set a workgroup takes per pass
U = 2.0 ** -53


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_bits_or_nan(a, b):
    """same_bits, but a NaN equals a NaN: the contract says where one appears, not its sign or payload."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


# ---- 1. the restatement ----

def ordered_sum(f):
    """SUM(f) of the header for the float64 values f [n] of one set; also the chunk partials."""
    f = np.asarray(f, np.float64)
    n = f.shape[0]
    chunks = (n + W - 1) // W
    partial = np.zeros(chunks, np.float64)
    t = np.arange(BLOCK)
    for c in range(chunks):
        a = np.zeros(BLOCK, np.float64)                          # a[t] = 0.0
        for u in range(ITEMS):                                   # a thread's items, one after the other
            j = c * W + u * BLOCK + t
            m = j < n
            a[m] = a[m] + f[j[m]]
        off = BLOCK // 2
        while off >= 1:                                          # the workgroup's tree
            a[:off] = a[:off] + a[off:2 * off]
            off //= 2
        partial[c] = a[0]
    s = np.float64(0.0)
    for c in range(chunks):                                      # across chunks, in their order
        s = s + partial[c]
    return s, partial


def mean_var(f):
    """(mean, var, S1, S2) of one set's float64 values by the header's two passes."""
    f = np.asarray(f, np.float64)
    nd = np.float64(f.shape[0])
    s1 = ordered_sum(f)[0]
    mean = s1 / nd
    d = f - mean
    s2 = ordered_sum(d * d)[0]
    return mean, s2 / nd, s1, s2


def call_rows(R, step0, n_steps):
    return [(step0 + k) % R for k in range(n_steps)]


def sets_of(x, num_sets, step0, n_steps):
    """The call's elements as [n, P]: column p is set p, in the set's element order."""
    R = x.shape[0]
    return x.reshape(R, -1)[call_rows(R, step0, n_steps)].reshape(-1, num_sets)


def standardize_ref(x, num_sets=1, min_std=1e-4, step0=0, n_steps=None):
    """-> (out float32 of x's shape: x with the call's rows standardised, moments float64 [P, 2])."""
    x = np.asarray(x, np.float32)
    R = x.shape[0]
    n_steps = R if n_steps is None else n_steps
    xs = sets_of(x, num_sets, step0, n_steps)
    res = np.empty_like(xs)
    moments = np.empty((num_sets, 2), np.float64)
    for p in range(num_sets):
        v = xs[:, p].astype(np.float64)
        mean, var, _, _ = mean_var(v)
        std = np.sqrt(var)
        denom = std if std > min_std else np.float64(min_std)
        res[:, p] = ((v - mean) / denom).astype(np.float32)
        moments[p] = mean, std
    out = x.copy().reshape(R, -1)
    out[call_rows(R, step0, n_steps)] = res.reshape(n_steps, -1)
    return out.reshape(x.shape), moments


def explained_variance_ref(y, pred, num_sets=1, step0=0, n_steps=None):
    y, pred = np.asarray(y, np.float32), np.asarray(pred, np.float32)
    n_steps = y.shape[0] if n_steps is None else n_steps
    ys, ps = sets_of(y, num_sets, step0, n_steps), sets_of(pred, num_sets, step0, n_steps)
    out = np.empty(num_sets, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for p in range(num_sets):
            v = ys[:, p].astype(np.float64)
            var_y = mean_var(v)[1]
            var_d = mean_var(v - ps[:, p].astype(np.float64))[1]
            r = np.float64(1.0) - var_d / var_y
            out[p] = np.float32(-1.0) if r < -1.0 else np.float32(r)
    return out


# ---- 2. the independent check and the bound ----

def independent(x, num_sets=1, min_std=1e-4, step0=0, n_steps=None):
    """-> (out float64 [n, P], mean [P], std [P]) by np.mean / np.std on float64 copies: nothing of the restatement's."""
    x = np.asarray(x, np.float32)
    n_steps = x.shape[0] if n_steps is None else n_steps
    v = sets_of(x, num_sets, step0, n_steps).astype(np.float64)
    mean, std = np.mean(v, axis=0), np.std(v, axis=0)
    return (v - mean) / np.maximum(min_std, std), mean, std


def g(n):
    return n * U / (1.0 - n * U)


def bound(v, min_std=1e-4):
    """For one set's float64 values v [n]: (e_m, e_s, e_o [n]) of the module docstring, each against the exact value; e_o
    without the float32 rounding.  Uses np.mean / np.std for mu and std (their own errors are second order here)."""
    v = np.asarray(v, np.float64)
    n = v.shape[0]
    A = np.mean(np.abs(v))
    mu, std = np.mean(v), np.std(v)
    var = std * std
    e_m = (g(n) + U) * A * (1.0 + U)
    e_v = e_m * e_m + g(n + 4) * (var + e_m * e_m)
    root = min(e_v / std, np.sqrt(e_v)) if std > 0.0 else np.sqrt(e_v)
    e_s = root * (1.0 + U) + U * std
    den = max(min_std, std)
    assert den - e_s > 0.0, "the bound needs a denominator that stays away from 0"
    dev = np.abs(v - mu)
    e_o = (e_m + 2.0 * U * (dev + e_m)) / (den - e_s) + dev * e_s / (den * (den - e_s))
    return e_m, e_s, e_o


def f32_rounding(o, e_o):
    """What the one rounding to float32 adds to a result within e_o of o."""
    return 2.0 ** -24 * (np.abs(o) + e_o) + 2.0 ** -150


def out_bound(v, min_std=1e-4):
    """|restatement's float32 out - the independent float64 out| <= this, per element of one set."""
    o = (v - np.mean(v)) / max(min_std, np.std(v))
    e_o = bound(v, min_std)[2]
    return 2.0 * e_o + f32_rounding(o, 2.0 * e_o)


# ---- inputs ----

def noise(seed, shape, scale=1.0, offset=0.0):
    r = np.random.RandomState(seed)
    return (offset + scale * r.standard_normal(shape)).astype(np.float32)


# ---- 3. the stage boundaries of the across-chunk sum, and orders it must not take ----
# The device stages BLOCK chunk partials at a time (csrc/ssd_moments.hip, combine()): a short stage and a full one are two
# branches, and LDS is handed from stage to stage.  (num_sets, per-set count, seed of noise()): the fewest chunks at which
# each path exists -- the longest short stage, exactly one full stage (its last chunk holds one element), a full stage and a
# stage of one partial, two full stages and a short one; then 257 chunks per set for three sets (blockIdx.y > 0, an odd
# stride between the sets' partials, every third float read).  Random data alone need not tell a wrong order from the right
# one, and `out`, a float32, does not at all (a 256-wide regrouping of 513 chunks changed none of 2.1 M elements), so the seeds
# are chosen on the CPU, the first of 1, 2, ... under which every order of WRONG_ORDERS that can differ at that count changes
# the bits of both the mean and the std of every set: all five at 513 chunks (seeds 2, 4 and 6 of 1 .. 8 do), the reversed one
# and the two 64-wide ones at 255 to 257 chunks, where sub-totals of 256 are the contract's own order (the pairwise sum is left
# to the 513-chunk case).  test_moments_cpu.py asserts it for every case.
STAGE_CASES = [(1, (BLOCK - 1) * W, 5), (1, (BLOCK - 1) * W + 1, 2), (1, BLOCK * W + 1, 2), (1, 2 * BLOCK * W + 7, 2),
               (3, BLOCK * W + 1, 7)]
STAGE_IDS = ["P%d-%dchunks" % (P, -(-n // W)) for P, n, _ in STAGE_CASES]
_stage = {}


def stage_input(P, n, seed):
    """x [n, P], pred, and their restatement (out, moments, explained variance): computed once, shared, read-only."""
    if (P, n, seed) not in _stage:
        x = noise(seed, (n, P), scale=2.0, offset=0.25)
        pred = (x * np.float32(0.5) + noise(seed + 1000, (n, P), scale=0.3)).astype(np.float32)     # (never x's own draw)
        _stage[P, n, seed] = (x, pred) + standardize_ref(x, num_sets=P) + (explained_variance_ref(x, pred, num_sets=P),)
        for a in _stage[P, n, seed]:
            a.setflags(write=False)
    return _stage[P, n, seed]


def _in_order(partial):
    s = np.float64(0.0)
    for v in partial:
        s = s + v
    return s


def _subtotals(width):
    """Sub-totals of `width` partials, each from +0.0 in chunk order, then the sub-totals in their order from +0.0."""
    return lambda partial: _in_order([_in_order(partial[i:i + width]) for i in range(0, len(partial), width)])


# name -> the chunk partials of one set added up in an order that is not the contract's
def _waves_then_pairs(partial):
    """Per stage of BLOCK partials: four sub-totals of 64, added among themselves as (w0 + w1) + (w2 + w3), then onto the sum."""
    s = np.float64(0.0)
    for i in range(0, len(partial), BLOCK):
        w = [_in_order(partial[j:j + 64]) for j in range(i, i + BLOCK, 64)]
        s = s + ((w[0] + w[1]) + (w[2] + w[3]))
    return s


WRONG_ORDERS = {"reversed": lambda partial: _in_order(partial[::-1]),
                "subtotals_of_64": _subtotals(64),               # every wave adding its own share of a stage
                "waves_then_pairs": _waves_then_pairs,           # ... with the four shares added among themselves first
                "subtotals_of_256": _subtotals(BLOCK),           # every stage from +0.0
                "pairwise": lambda partial: np.asarray(partial, np.float64).sum()}


def wrong_moments(v, orders):
    """For one set's float64 values v: {order: (mean, std)} with the mean from S1's chunk partials added in that wrong order,
    and the std from the RIGHT mean with only S2's chunk partials added in it; and the contract's (mean, std) under None."""
    v = np.asarray(v, np.float64)
    nd = np.float64(v.shape[0])
    s1, p1 = ordered_sum(v)
    mean = s1 / nd
    d = v - mean
    s2, p2 = ordered_sum(d * d)
    res = {None: (mean, np.sqrt(s2 / nd))}
    for o in orders:
        res[o] = WRONG_ORDERS[o](p1) / nd, np.sqrt(WRONG_ORDERS[o](p2) / nd)
    return res
