"""The tests' restatement of the advantages contract, written the way RLlib computes it: each
trajectory is split into its episode segments at the done rows, and per segment `discount` -- scipy.signal.lfilter over the
reversed sequence -- is applied to float64 inputs; the results are cast to float32 at the end.  Independent of the package's
own NumPy path (a vectorised backward loop), which it checks."""
import numpy as np
import scipy.signal

F64 = np.float64


def discount(x, g):
    """RLlib's discount(): y[t] = x[t] + g * y[t + 1]."""
    return scipy.signal.lfilter([1], [1, float(-g)], x[::-1], axis=0)[::-1]


def _segment(r, v, last_r, gamma, lambda_, use_gae, use_critic):
    """compute_advantages of one episode segment (float64 arrays; last_r: the value after its last step, 0.0 if it ended)."""
    if use_gae:
        vpred_t = np.concatenate([v, np.array([last_r], F64)])
        delta = r + F64(gamma) * vpred_t[1:] - vpred_t[:-1]
        adv = discount(delta, F64(gamma) * F64(lambda_))
        return adv.astype(np.float32), (adv + v).astype(np.float32)
    ret = discount(np.concatenate([r, np.array([last_r], F64)]), gamma)[:-1]
    if use_critic:
        return (ret - v).astype(np.float32), ret.astype(np.float32)
    return ret.astype(np.float32), np.zeros(len(r), np.float32)


def advantages_ref(rew, value, last_value=None, done=None, gamma=0.99, lambda_=1.0, use_gae=True, use_critic=True, bonus=None,
                   bonus_weight=1.0, step0=0, n_steps=None):
    """NumPy arrays in, (advantages, value_targets) float32 arrays of rew's shape out; rows outside the call are zero."""
    shape = rew.shape
    R = shape[0]
    K = R if n_steps is None else n_steps
    rows = [(step0 + k) % R for k in range(K)]
    flat = lambda a: None if a is None else np.asarray(a).reshape(R, -1)[rows]   # noqa: E731
    rew2, val2, done2, bon2 = flat(rew), flat(value), flat(done), flat(bonus)
    L = rew2.shape[1]
    last = np.zeros(L, np.float32) if last_value is None else np.asarray(last_value).reshape(L)
    adv, vt = np.zeros((K, L), np.float32), np.zeros((K, L), np.float32)
    for l in range(L):
        r = rew2[:, l].astype(F64)
        if bon2 is not None:
            r = r + F64(bonus_weight) * bon2[:, l].astype(F64)
        v = np.zeros(K, F64) if val2 is None else val2[:, l].astype(F64)
        ends = [] if done2 is None else list(np.flatnonzero(done2[:, l]))
        start = 0
        for e in ends + [K - 1]:
            if e < start:
                continue                                         # (the last row was a done row: nothing is left)
            ended = done2 is not None and done2[e, l] != 0
            last_r = 0.0 if ended else float(F64(last[l]))
            a, t = _segment(r[start:e + 1], v[start:e + 1], last_r, gamma, lambda_, use_gae, use_critic)
            adv[start:e + 1, l], vt[start:e + 1, l] = a, t
            start = e + 1
    out_a, out_t = np.zeros((R, L), np.float32), np.zeros((R, L), np.float32)
    out_a[rows], out_t[rows] = adv, vt
    return out_a.reshape(shape), out_t.reshape(shape)


def rewards(rng, shape):
    # (tests/test_episode_stats_gpu.py _rew) apples, FIRE costs, single and multiple hits, and a zero-sum tail
    return rng.choice([1, 0, 0, -1, -50, -49, -51, -100, -101, -150], size=shape,
                      p=[.25, .3, .1, .1, .08, .05, .04, .04, .02, .02]).astype(np.int32)


def make_rings(seed, R, trailing, done_mode, with_bonus=False, with_last=True, done_rate=0.02):
    """Random rings: rew as the games pay it, value and bonus normal float32, done nowhere / everywhere / at done_rate / on no
    row yet ("last": build() sets the call's last row)."""
    rng = np.random.default_rng(seed)
    shape = (R,) + tuple(trailing)
    c = {"rew": rewards(rng, shape), "value": (rng.standard_normal(shape) * 3).astype(np.float32),
         "last_value": np.asarray(rng.standard_normal(tuple(trailing)) * 3, dtype=np.float32) if with_last else None,
         "done": {"none": None, "all": np.ones(shape, np.uint8), "last": np.zeros(shape, np.uint8),
                  "some": (rng.random(shape) < done_rate).astype(np.uint8)}[done_mode],
         "bonus": np.abs(rng.standard_normal(shape)).astype(np.float32) * np.float32(0.05) if with_bonus else None}
    return c


MODES = {"gae": dict(use_gae=True, use_critic=True), "returns_critic": dict(use_gae=False, use_critic=True),
         "returns": dict(use_gae=False, use_critic=False)}
GAMMAS, LAMBDAS = (0.0, 0.5, 0.99, 1.0), (0.0, 0.95, 1.0)
STEPS = (1, 2, 63, 64, 65, 400)
DONES = ("none", "all", "some")


def matrix():
    """The synthetic cases both suites run: (id, rings kwargs, call kwargs).  Every K x done x mode, with gamma, lambda,
    bonus and the absent last_value rotating through them so that each value meets each K and mode; then every (gamma,
    lambda) pair in every mode at K = 65; then rings longer than the call whose rows wrap."""
    out, n = [], 0
    for K in STEPS:
        for dm in DONES:
            for mode in MODES:
                g, lam = GAMMAS[n % 4], LAMBDAS[(n // 4) % 3]
                bonus, last = n % 2 == 1, n % 5 != 0
                out.append(("K%d-%s-%s-g%s-l%s%s%s" % (K, dm, mode, g, lam, "-bonus" if bonus else "", "" if last else "-nolast"),
                            dict(seed=100 + n, R=K, trailing=(70,), done_mode=dm, with_bonus=bonus, with_last=last),
                            dict(gamma=g, lambda_=lam, bonus_weight=0.25, **MODES[mode])))
                n += 1
    for g in GAMMAS:
        for lam in LAMBDAS:
            for mode in MODES:
                for bonus in (False, True):
                    out.append(("K65-some-%s-g%s-l%s%s" % (mode, g, lam, "-bonus" if bonus else ""),
                                dict(seed=100 + n, R=65, trailing=(7, 5), done_mode="some", with_bonus=bonus),
                                dict(gamma=g, lambda_=lam, bonus_weight=-1.5, **MODES[mode])))
                    n += 1
    for mode in MODES:
        for R, K, step0 in ((100, 64, 70), (65, 65, 13), (7, 2, 6), (400, 399, 123456)):
            out.append(("wrap-R%d-K%d-s%d-%s" % (R, K, step0, mode),
                        dict(seed=100 + n, R=R, trailing=(67,), done_mode="some", with_bonus=True),
                        dict(gamma=0.99, lambda_=0.95, bonus_weight=0.25, step0=step0, n_steps=K, **MODES[mode])))
            n += 1
    return out


# The kernel requests LOAD_BLOCK steps at a time through two register buffers that swap roles (csrc/ssd_gae.hip, kLoad).
LOAD_BLOCK = 16
# no full block, then one, two (the odd buffer's exit) and three full blocks: each alone, one short and one over
BLOCK_STEPS = (15, 16, 17, 31, 32, 33, 47, 48, 49)
# spare lanes, a whole last wave (64, 128), a second and a third wave
BLOCK_LANES = (1, 63, 64, 65, 128, 130)
BLOCK_DONES = ("all", "last", "some")
# The seeds of the "some" cases in the order block_matrix() makes them, found on the CPU: for the i-th of them the first of
# 700 + 10 i, 701 + 10 i, ... whose rings have what some_conditions() asks for; test_advantages_cpu.py asserts that each does.
# The rate is 0.3 for one lane (it needs two done rows of its own in as few as 17 steps) and 0.06 otherwise (a lane of 49
# steps stays without a done row with probability 0.05).
SOME_SEEDS = (700, 710, 720, 730, 740, 751, 760, 770, 780, 790, 801, 810, 820, 830, 840, 850, 860, 870)


def some_rate(L):
    return 0.3 if L == 1 else 0.06


def some_conditions(done, K):
    """What a "some" case of K steps (rows 0 .. K - 1 of done [K, L]) must hold: a done row inside a full block (the kernel
    walks down from row K - 1, so the full blocks are rows K % LOAD_BLOCK ... K - 1; the call's last row cuts by itself and does
    not count), one among the K % LOAD_BLOCK rows left at the fragment's start where there are any, and a lane without any when
    there is more than one lane.  -> the three as booleans, True where a condition does not apply."""
    done = np.asarray(done).reshape(K, -1) != 0
    left = K % LOAD_BLOCK
    return (K < LOAD_BLOCK or bool(done[left:K - 1].any()), left == 0 or bool(done[:left].any()),
            done.shape[1] == 1 or bool((~done.any(axis=0)).any()))


def build(rings, call):
    """The rings of a block_matrix() case; done mode "last" sets the whole last row of the call and no other."""
    c = make_rings(**rings)
    if rings["done_mode"] == "last":
        R = rings["R"]
        c["done"][(call.get("step0", 0) + call.get("n_steps", R) - 1) % R] = 1
    return c


def block_matrix(some_seeds=None):
    """(id, rings kwargs, call kwargs) for build(): at every K of BLOCK_STEPS each of the twelve kernel instances (mode x bonus
    given / absent x done given / absent) once, with the lane counts, gamma, lambda and the absent last_value rotating so that
    every lane count meets every mode; where done is given, "all", the call's last row only and "some" rotate; then three
    rings that wrap per mode in the instance without bonus and done.  some_seeds: SOME_SEEDS, or a function of (case index
    among the "some" cases, rings kwargs without a seed) for the search that found them."""
    seeds = SOME_SEEDS if some_seeds is None else some_seeds
    out, n, some = [], 0, 0
    for ki, K in enumerate(BLOCK_STEPS):
        for mi, mode in enumerate(MODES):
            for bi, bonus in enumerate((False, True)):
                for di, given in enumerate((False, True)):
                    L = BLOCK_LANES[(ki + 2 * bi + di + mi) % 6]
                    g, lam = GAMMAS[(n + n // 4) % 4], LAMBDAS[(2 * ki + 2 * mi + bi) % 3]
                    dm = BLOCK_DONES[(ki + 2 * mi + bi) % 3] if given else "none"
                    last = n % 5 != 0
                    rings = dict(R=K, trailing=(L,), done_mode=dm, with_bonus=bonus, with_last=last)
                    if dm == "some":
                        rings["done_rate"] = some_rate(L)
                        rings["seed"] = seeds(some, rings) if callable(seeds) else seeds[some]
                        some += 1
                    else:
                        rings["seed"] = 500 + n
                    out.append(("K%d-L%d-%s-%s-g%s-l%s%s%s" % (K, L, mode, dm, g, lam, "-bonus" if bonus else "", "" if last else "-nolast"),
                                rings, dict(gamma=g, lambda_=lam, bonus_weight=0.25, **MODES[mode])))
                    n += 1
    for mode in MODES:
        for (R, K, step0), L in zip(((40, 33, 30), (17, 16, 9), (48, 48, 47)), (65, 64, 130)):
            out.append(("wrap-R%d-K%d-s%d-L%d-%s" % (R, K, step0, L, mode),
                        dict(seed=500 + n, R=R, trailing=(L,), done_mode="none", with_bonus=False),
                        dict(gamma=0.99, lambda_=0.95, step0=step0, n_steps=K, **MODES[mode])))
            n += 1
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))
