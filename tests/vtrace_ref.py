"""The tests' restatement of the V-trace contract (include/ssd.h, V-TRACE TARGETS), written the way RLlib
0.7.6's vtrace.from_importance_weights computes it: time-major arrays [K, L], everything promoted to float64 first, the deltas
and the shifted values formed for all steps at once, a reverse scan of delta + discount * c * acc, vs = acc + values, vs_{t+1}
by concatenation with the bootstrap; the results are cast to float32 at the end.  discounts = (1 - done) * gamma.  Written from
the formulas (ray is not needed); independent of the package's own NumPy path (a per-step backward walk), which it checks."""
import numpy as np

from gae_ref import rewards

F64 = np.float64
INF = float("inf")


def from_importance_weights(rhos, discounts, rew, values, bootstrap, clip_rho, clip_pg):
    """float64 arrays [K, L] (bootstrap [L]) -> (vs, pg_advantages) float64 [K, L], in RLlib's operation order."""
    clipped_rhos = np.minimum(F64(clip_rho), rhos) if clip_rho is not None else rhos
    cs = np.minimum(F64(1.0), rhos)
    values_t_plus_1 = np.concatenate([values[1:], bootstrap[None]], axis=0)
    deltas = clipped_rhos * (rew + discounts * values_t_plus_1 - values)
    acc = np.zeros_like(bootstrap)
    vs_minus_v = np.empty_like(values)
    for t in range(values.shape[0] - 1, -1, -1):                 # tf.scan over the reversed sequences
        acc = deltas[t] + discounts[t] * cs[t] * acc
        vs_minus_v[t] = acc
    vs = vs_minus_v + values
    vs_t_plus_1 = np.concatenate([vs[1:], bootstrap[None]], axis=0)
    clipped_pg_rhos = np.minimum(F64(clip_pg), rhos) if clip_pg is not None else rhos
    pg = clipped_pg_rhos * (rew + discounts * vs_t_plus_1 - values)
    return vs, pg


def vtrace_ref(rew, value, rhos, bootstrap_value=None, done=None, gamma=0.99, clip_rho_threshold=1.0, clip_pg_rho_threshold=1.0,
               bonus=None, bonus_weight=1.0, step0=0, n_steps=None):
    """NumPy arrays in, (vs, pg_advantages) float32 arrays of rew's shape out; rows outside the call are zero."""
    shape = rew.shape
    R = shape[0]
    K = R if n_steps is None else n_steps
    rows = [(step0 + k) % R for k in range(K)]
    flat = lambda a: None if a is None else np.asarray(a).reshape(R, -1)[rows]   # noqa: E731
    rew2, val2, rho2, done2, bon2 = flat(rew), flat(value), flat(rhos), flat(done), flat(bonus)
    L = rew2.shape[1]
    boot = np.zeros(L, F64) if bootstrap_value is None else np.asarray(bootstrap_value).reshape(L).astype(F64)
    r = rew2.astype(F64)
    if bon2 is not None:
        r = r + F64(bonus_weight) * bon2.astype(F64)
    not_done = np.ones((K, L), F64) if done2 is None else F64(1.0) - (done2 != 0).astype(F64)
    unclipped = lambda c: None if c == INF else c                # noqa: E731  (RLlib: a threshold of None does not clip)
    vs, pg = from_importance_weights(rho2.astype(F64), not_done * F64(gamma), r, val2.astype(F64), boot,
                                     unclipped(clip_rho_threshold), unclipped(clip_pg_rho_threshold))
    out_v, out_p = np.zeros((R, L), np.float32), np.zeros((R, L), np.float32)
    out_v[rows], out_p[rows] = vs.astype(np.float32), pg.astype(np.float32)
    return out_v.reshape(shape), out_p.reshape(shape)


DONES = ("none", "all", "some", "last")
GAMMAS = (0.0, 0.99, 1.0)
THRESHOLDS = ((1.0, 1.0), (0.7, 1.3), (INF, INF))
FINITE = (0.7, 1.0, 1.3)                                         # every finite threshold of the matrix
CPU_STEPS, CPU_LANES = (1, 2, 15, 16, 17, 33, 400), (1, 63, 65, 130)
# no full block of 16 steps, one, the odd buffer, a remainder after each; spare lanes, a second and a third wave
GPU_STEPS, GPU_LANES = (1, 15, 16, 17, 32, 33, 48, 49), (1, 63, 64, 65, 130)


def make_rings(seed, R, trailing, done_mode, with_bonus=False, with_boot=True, sigma=1.0):
    """Random rings: rew as the games pay it, value and bootstrap normal float32, rhos = exp(sigma * normal) in float32 (a
    spread wide enough for both sides of every threshold), done nowhere / everywhere / at rate 0.05 / on the call's last row
    (set by the caller of `last`: see matrix())."""
    rng = np.random.default_rng(seed)
    shape = (R,) + tuple(trailing)
    done = {"none": None, "all": np.ones(shape, np.uint8), "some": (rng.random(shape) < 0.05).astype(np.uint8),
            "last": (rng.random(shape) < 0.05).astype(np.uint8)}[done_mode]
    return {"rew": rewards(rng, shape), "value": (rng.standard_normal(shape) * 3).astype(np.float32),
            "rhos": np.exp((rng.standard_normal(shape) * sigma).astype(np.float32)),
            "bootstrap_value": np.asarray(rng.standard_normal(tuple(trailing)) * 3, dtype=np.float32) if with_boot else None,
            "done": done,
            "bonus": np.abs(rng.standard_normal(shape)).astype(np.float32) * np.float32(0.05) if with_bonus else None}


def build(rings, call):
    """The rings of a matrix case; done mode "last" sets the whole last row of the call."""
    c = make_rings(**rings)
    if rings["done_mode"] == "last":
        R = rings["R"]
        c["done"][(call.get("step0", 0) + call.get("n_steps", R) - 1) % R] = 1
    return c


def matrix(steps, lanes):
    """(id, rings kwargs, call kwargs): every K x L x done mode, with gamma, the thresholds, the bonus and the absent bootstrap
    rotating through them by the three indices, so that every done mode meets the bonus present and absent (all four kernel
    instances) at every K; then every (gamma, thresholds, bonus) combination at K = 33 with the done modes rotating; then
    rings longer than the call whose rows wrap."""
    out, n = [], 0
    for ki, K in enumerate(steps):
        for li, L in enumerate(lanes):
            for di, dm in enumerate(DONES):
                g, th = GAMMAS[(ki + li + di) % 3], THRESHOLDS[(ki + 2 * li + di) % 3]
                bonus, boot = (ki + li + di) % 2 == 1, (3 * ki + li + di) % 5 != 0
                out.append(("K%d-L%d-%s-g%s-c%s-%s%s%s" % (K, L, dm, g, th[0], th[1], "-bonus" if bonus else "", "" if boot else "-noboot"),
                            dict(seed=300 + n, R=K, trailing=(L,), done_mode=dm, with_bonus=bonus, with_boot=boot),
                            dict(gamma=g, clip_rho_threshold=th[0], clip_pg_rho_threshold=th[1], bonus_weight=0.25)))
                n += 1
    for g in GAMMAS:
        for th in THRESHOLDS:
            for bonus in (False, True):
                dm = DONES[n % 4]
                out.append(("K33-%s-g%s-c%s-%s%s" % (dm, g, th[0], th[1], "-bonus" if bonus else ""),
                            dict(seed=300 + n, R=33, trailing=(7, 5), done_mode=dm, with_bonus=bonus),
                            dict(gamma=g, clip_rho_threshold=th[0], clip_pg_rho_threshold=th[1], bonus_weight=-1.5)))
                n += 1
    for R, K, step0 in ((100, 64, 70), (65, 65, 13), (7, 2, 6), (400, 399, 123456), (50, 33, 40)):
        for bonus, dm in ((True, "some"), (False, "last")):
            out.append(("wrap-R%d-K%d-s%d-%s%s" % (R, K, step0, dm, "-bonus" if bonus else ""),
                        dict(seed=300 + n, R=R, trailing=(67,), done_mode=dm, with_bonus=bonus),
                        dict(gamma=0.99, clip_rho_threshold=0.7, clip_pg_rho_threshold=1.3, bonus_weight=0.25, step0=step0, n_steps=K)))
            n += 1
    return out


def spacing32(x):
    """The float32 spacing at |x| (float64 in, float64 out)."""
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(F64)
