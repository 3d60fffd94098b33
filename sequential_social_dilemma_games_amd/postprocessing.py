"""Advantages and value targets of rollout batches (csrc/ssd_gae.hip, include/ssd.h ssd_advantages): the step every trainer
takes between sampling and its loss -- RLlib's compute_advantages, i.e. generalised advantage estimation (PPO) or discounted
returns with or without a critic (A3C) -- with the episode cuts at `done` rows and the fragment bootstrap `last_value`.
DESIGN.md section 15 states the contract: float64 operations in a fixed order, one rounding to float32 at the end.

    batch = env.sample(policy, 128, gamma=0.99, lambda_=0.95)          # gains "advantages" and "value_targets"
    adv, vt = compute_advantages(batch["rew"], batch["value"], batch["last_value"], batch["done"], gamma=0.99, lambda_=0.95)

CUDA tensors go to the kernel (one launch on torch's current stream, no synchronisation); CPU tensors run a NumPy loop of
the same contract, bit for bit.

vtrace() is the same step for the IMPALA trainer (csrc/ssd_vtrace.hip, include/ssd.h ssd_vtrace): the
V-trace value targets and policy-gradient advantages from the target policy's values and the importance weights, by the same
conventions.

    logits, value, boot = evaluate_fragment(policy, batch, first, seq_len)            # under the learner's current weights
    vs, pg = vtrace(batch["rew"], value, rhos, boot, batch["done"], gamma=0.99)       # rhos = exp(logp_target - batch["logp"])

standardize_advantages() and explained_variance() are the per-weight-set moments RLlib's PPO trainer takes of a train batch
(csrc/ssd_moments.hip, include/ssd.h BATCH MOMENTS): the advantages standardised before the SGD epochs,
and vf_explained_var, as two-pass float64 moments in a fixed summation order.  update_kl_coeff() is the trainer's rule for
its KL coefficient, on the host.

    adv = standardize_advantages(batch["advantages"], num_sets=policy.num_sets)       # or sample(..., standardize=True)
    ev = explained_variance(batch["value_targets"], batch["value"], num_sets=policy.num_sets)
    kl_coeff = update_kl_coeff(kl_coeff, float(stats["kl"].mean()), kl_target=0.01)
"""
import ctypes as C
import math

import numpy as np

from . import _capi


def _check(torch, t, dtype, shape, device, name):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device \
            or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, tuple(shape), device))


# ---- what the four calls on the [R, ...] rings share: each rule once ----

def _leading(torch, t, dtype, name):
    """The tensor that gives a call its shape -> shape, device, R (ring rows), L (trajectories of a row)."""
    what = {torch.int32: "an int32", torch.float32: "a float32"}[dtype]
    if not isinstance(t, torch.Tensor) or t.dim() < 1:
        raise ValueError("%s must be %s tensor of shape [R, ...]" % (name, what))
    shape, dev = tuple(t.shape), t.device
    R = shape[0]
    L = int(np.prod(shape[1:], dtype=np.int64))
    if R < 1 or L < 1:
        raise ValueError("%s holds no step" % name)
    if L >= 2 ** 31 or R >= 2 ** 31:
        raise ValueError("%s is too large: fewer than 2^31 rows and trajectories" % name)
    _check(torch, t, dtype, shape, dev, name)
    return shape, dev, R, L


def _ring_rows(R, step0, n_steps):
    """-> step0, n_steps as ints: row k of the call is ring slot (step0 + k) % R, k < n_steps (default R)."""
    step0 = int(step0)
    n_steps = R if n_steps is None else int(n_steps)
    if n_steps < 1 or n_steps > R:
        raise ValueError("n_steps (%d) must be 1..%d, the ring length: a call reads each slot once" % (n_steps, R))
    if step0 < 0 or step0 >= 2 ** 31:
        raise ValueError("step0 must be 0..2^31 - 1")
    return step0, n_steps


def _slots(R, step0, n_steps):
    return [(step0 + k) % R for k in range(n_steps)]


def _episode_inputs(torch, shape, dev, bootstrap, bootstrap_name, done, bonus, bonus_weight):
    """The optional inputs compute_advantages and vtrace take alike -> bonus_weight as a float."""
    if bootstrap is not None:
        _check(torch, bootstrap, torch.float32, shape[1:], dev, bootstrap_name)
    if done is not None:
        _check(torch, done, torch.uint8, shape, dev, "done")
    if bonus is not None:
        _check(torch, bonus, torch.float32, shape, dev, "bonus")
    bonus_weight = float(bonus_weight)
    if bonus is not None and not math.isfinite(bonus_weight):
        raise ValueError("bonus_weight must be finite")
    return bonus_weight


def _out_pair(torch, out, shape, dev, whole_ring, names):
    """The two float32 results: allocated (zero where the call writes only some of the rows), or the caller's pair."""
    if out is None:
        make = torch.empty if whole_ring else torch.zeros
        return make(shape, dtype=torch.float32, device=dev), make(shape, dtype=torch.float32, device=dev)
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        raise ValueError("out must be a pair (%s, %s)" % names)
    first, second = out
    _check(torch, first, torch.float32, shape, dev, "out[0]")
    _check(torch, second, torch.float32, shape, dev, "out[1]")
    if first.data_ptr() == second.data_ptr():
        raise ValueError("out[0] and out[1] must be two tensors")
    return first, second


def _kernel_target(torch, dev):
    """-> None where the NumPy path runs (CPU tensors), else (device index, torch's current stream) for the kernels."""
    if dev.type == "cpu":
        return None
    if dev.type != "cuda":
        raise ValueError("the tensors must be on the CPU or on a GPU, not on %s" % (dev,))
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    return index, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _host(rew, value, last_value, done, bonus, bonus_weight, gamma, lambda_, use_gae, use_critic, step0, n_steps, adv, vt):
    """The contract on the host: the lanes at once, the steps one after the other, every operation a float64 array operation."""
    R = rew.shape[0]
    f64 = np.float64
    flat = lambda t: None if t is None else t.numpy().reshape(R, -1)   # noqa: E731
    rew, value, done, bonus, adv, vt = flat(rew), flat(value), flat(done), flat(bonus), flat(adv), flat(vt)
    L = rew.shape[1]
    gl = gamma * lambda_
    v_after = np.zeros(L, f64) if last_value is None else last_value.numpy().reshape(L).astype(f64)
    run = np.zeros(L, f64)
    for k in range(n_steps - 1, -1, -1):
        s = (step0 + k) % R
        r = rew[s].astype(f64)
        if bonus is not None:
            r = r + bonus_weight * bonus[s].astype(f64)
        dn = np.zeros(L, bool) if done is None else done[s] != 0
        cut = dn if k < n_steps - 1 else np.ones(L, bool)
        v_next = np.where(dn, 0.0, v_after)
        if use_gae:
            vk = value[s].astype(f64)
            delta = (r + gamma * v_next) - vk
            A = delta + gl * np.where(cut, 0.0, run)
            adv[s] = A.astype(np.float32)
            vt[s] = (A + vk).astype(np.float32)
            run, v_after = A, vk
        else:
            G = r + gamma * np.where(cut, v_next, run)
            if use_critic:
                adv[s] = (G - value[s].astype(f64)).astype(np.float32)
                vt[s] = G.astype(np.float32)
            else:
                adv[s] = G.astype(np.float32)
                vt[s] = 0.0
            run = G


def compute_advantages(rew, value, last_value=None, done=None, gamma=0.99, lambda_=1.0, use_gae=True, use_critic=True,
                       bonus=None, bonus_weight=1.0, step0=0, n_steps=None, out=None):
    """-> (advantages, value_targets), float32 tensors of rew's shape.

    rew int32 [R, ...] (any trailing shape: [R,E,N] from sample(), [R,E], [R,L]; each trailing index is a trajectory), value
    float32 and done uint8 of the same shape, last_value float32 of the trailing shape; all contiguous and on one device.
    Row k of the call is ring slot (step0 + k) % R, k < n_steps (default R); rows outside the call are not written (zero
    in tensors this function allocates).  done[k] != 0: the episode ended with step k and row k + 1 belongs to the next one
    (None: no episode ends).  last_value: the value of the observation after the last row, the bootstrap of a fragment that
    does not end with its episode (None: 0).  bonus float32 of rew's shape: the reward is rew + bonus_weight * bonus in
    float64 (the MOA trainers' rewards + influence * weight).
    use_gae: generalised advantage estimation with lambda_; else discounted returns, minus value when use_critic (value may
    be None otherwise, and value_targets is 0).  out: (advantages, value_targets) tensors to write into.
    """
    import torch
    shape, dev, R, L = _leading(torch, rew, torch.int32, "rew")
    use_gae, use_critic = bool(use_gae), bool(use_critic)
    if use_gae and not use_critic:
        raise ValueError("use_gae needs use_critic: generalised advantage estimation uses the value function")
    if value is not None or use_critic:
        _check(torch, value, torch.float32, shape, dev, "value")
    bonus_weight = _episode_inputs(torch, shape, dev, last_value, "last_value", done, bonus, bonus_weight)
    gamma, lambda_ = float(gamma), float(lambda_)
    if not (math.isfinite(gamma) and math.isfinite(lambda_)):
        raise ValueError("gamma and lambda_ must be finite")
    step0, n_steps = _ring_rows(R, step0, n_steps)
    adv, vt = _out_pair(torch, out, shape, dev, n_steps == R, ("advantages", "value_targets"))
    target = _kernel_target(torch, dev)
    if target is None:
        _host(rew, value, last_value, done, bonus, bonus_weight, gamma, lambda_, use_gae, use_critic, step0, n_steps, adv, vt)
        return adv, vt
    index, stream = target
    flags = (_capi.SSD_ADV_GAE if use_gae else 0) | (_capi.SSD_ADV_CRITIC if use_critic else 0)
    _capi.advantages_check(_capi.lib().ssd_advantages(_ptr(rew), _ptr(bonus), bonus_weight, _ptr(value) if use_critic else None,
                                                      _ptr(done), _ptr(last_value), L, R, step0, n_steps, gamma, lambda_, flags,
                                                      _ptr(adv), _ptr(vt), index, stream))
    return adv, vt


# ---- V-trace targets (csrc/ssd_vtrace.hip, include/ssd.h ssd_vtrace) ----

def _host_vtrace(rew, value, rhos, bootstrap, done, bonus, bonus_weight, gamma, clip_rho, clip_pg, step0, n_steps, vs_out, pg_out):
    """The contract on the host: the lanes at once, the steps one after the other, every operation a float64 array operation."""
    R = rew.shape[0]
    f64 = np.float64
    flat = lambda t: None if t is None else t.numpy().reshape(R, -1)   # noqa: E731
    rew, value, rhos, done, bonus, vs_out, pg_out = (flat(x) for x in (rew, value, rhos, done, bonus, vs_out, pg_out))
    L = rew.shape[1]
    boot = np.zeros(L, f64) if bootstrap is None else bootstrap.numpy().reshape(L).astype(f64)
    v_after, vs_after = boot, boot
    acc = np.zeros(L, f64)
    for k in range(n_steps - 1, -1, -1):
        s = (step0 + k) % R
        r = rew[s].astype(f64)
        if bonus is not None:
            r = r + bonus_weight * bonus[s].astype(f64)
        disc = np.full(L, gamma, f64) if done is None else np.where(done[s] != 0, 0.0, gamma)
        v = value[s].astype(f64)
        rho = rhos[s].astype(f64)
        delta = np.minimum(clip_rho, rho) * ((r + disc * v_after) - v)
        dc = disc * np.minimum(1.0, rho)
        acc = delta + dc * acc
        vs = v + acc
        pg = np.minimum(clip_pg, rho) * ((r + disc * vs_after) - v)
        vs_out[s] = vs.astype(np.float32)
        pg_out[s] = pg.astype(np.float32)
        v_after, vs_after = v, vs


def vtrace(rew, value, rhos, bootstrap_value=None, done=None, gamma=0.99, clip_rho_threshold=1.0, clip_pg_rho_threshold=1.0,
           bonus=None, bonus_weight=1.0, step0=0, n_steps=None, out=None):
    """-> (vs, pg_advantages), float32 tensors of rew's shape: the V-trace value targets and policy-gradient advantages of
    IMPALA (RLlib 0.7.6's vtrace.from_importance_weights with discounts = (1 - done) * gamma and c bar = 1; include/ssd.h, V-TRACE
    TARGETS states every operation: float64 in a fixed order, one rounding to float32 at the end).

    rew int32 [R, ...], done uint8 and bonus float32 as compute_advantages takes them (the same shapes, ring rows step0,
    n_steps, and `out` pair).  value float32 of rew's shape and bootstrap_value float32 of the trailing shape are the TARGET
    policy's -- the learner's current weights on the fragment's observations (policy.evaluate_fragment), not what the rollout
    recorded; None for bootstrap_value: 0.  rhos float32 of rew's shape: the importance weights pi / mu of the taken actions,
    exp(logp_target - logp_behaviour), finite and >= 0.  The thresholds are > 0; float("inf") means no clip.
    Every row of the call is a target row.  RLlib's trainer drops the last row of each T-row sequence and bootstraps from its
    value: that is this function on the sequence's first T - 1 rows with bootstrap_value = the current value of row T - 1.
    CUDA tensors go to the kernel (one launch on torch's current stream, no synchronisation); CPU tensors run a NumPy loop
    of the same contract, bit for bit.
    """
    import torch
    shape, dev, R, L = _leading(torch, rew, torch.int32, "rew")
    _check(torch, value, torch.float32, shape, dev, "value")
    _check(torch, rhos, torch.float32, shape, dev, "rhos")
    bonus_weight = _episode_inputs(torch, shape, dev, bootstrap_value, "bootstrap_value", done, bonus, bonus_weight)
    gamma = float(gamma)
    clip_rho, clip_pg = float(clip_rho_threshold), float(clip_pg_rho_threshold)
    if not math.isfinite(gamma):
        raise ValueError("gamma must be finite")
    if not (clip_rho > 0.0 and clip_pg > 0.0):
        raise ValueError("clip_rho_threshold and clip_pg_rho_threshold must be > 0 (inf: no clip)")
    step0, n_steps = _ring_rows(R, step0, n_steps)
    vs, pg = _out_pair(torch, out, shape, dev, n_steps == R, ("vs", "pg_advantages"))
    target = _kernel_target(torch, dev)
    if target is None:
        _host_vtrace(rew, value, rhos, bootstrap_value, done, bonus, bonus_weight, gamma, clip_rho, clip_pg, step0, n_steps, vs, pg)
        return vs, pg
    index, stream = target
    _capi.vtrace_check(_capi.lib().ssd_vtrace(_ptr(rew), _ptr(bonus), bonus_weight, _ptr(value), _ptr(rhos), _ptr(done),
                                              _ptr(bootstrap_value), L, R, step0, n_steps, gamma, clip_rho, clip_pg, 0,
                                              _ptr(vs), _ptr(pg), index, stream))
    return vs, pg


# ---- batch moments (csrc/ssd_moments.hip, include/ssd.h BATCH MOMENTS) ----

def _ordered_sum(f):
    """SUM(f) of include/ssd.h, BATCH MOMENTS, for the float64 values f [n] of one set: the threads' sequential sums (all
    chunks and threads at once, the items one after the other), the workgroup's tree by halving, the chunks in their order.
    The places past n hold +0.0, which changes no sum: an accumulator that starts at +0.0 is never -0.0."""
    B, I, W = _capi.SSD_MOM_BLOCK, _capi.SSD_MOM_ITEMS, _capi.SSD_MOM_CHUNK
    n = f.shape[0]
    chunks = (n + W - 1) // W
    padded = np.zeros(chunks * W, np.float64)
    padded[:n] = f
    padded = padded.reshape(chunks, I, B)
    a = np.zeros((chunks, B), np.float64)
    for u in range(I):
        a = a + padded[:, u, :]
    off = B // 2
    while off >= 1:
        a = a[:, :off] + a[:, off:2 * off]
        off //= 2
    s = np.float64(0.0)
    for c in range(chunks):
        s = s + a[c, 0]
    return s


def _mean_var(f):
    """(mean, var) of the float64 values f [n] by the two passes of the contract."""
    nd = np.float64(f.shape[0])
    mean = _ordered_sum(f) / nd
    d = f - mean
    return mean, _ordered_sum(d * d) / nd


def _moments_args(torch, x, num_sets, step0, n_steps, name):
    shape, dev, R, L = _leading(torch, x, torch.float32, name)
    num_sets = int(num_sets)
    if num_sets < 1 or L % num_sets or num_sets > 65535:
        raise ValueError("num_sets (%d) must be 1..65535 and divide the %d trajectories of a row: trajectory l belongs to set "
                         "l %% num_sets" % (num_sets, L))
    return (shape, dev, R, L, num_sets) + _ring_rows(R, step0, n_steps)


_moments_scratch = {}


def _scratch(torch, dev, index, doubles):
    """The calls' float64 scratch: one torch allocation per device and size, kept.  Calls that share it are ordered by the
    stream they run on; use one stream per device for these calls."""
    key = (index, doubles)
    buf = _moments_scratch.get(key)
    if buf is None:
        buf = _moments_scratch[key] = torch.empty(doubles, dtype=torch.float64, device=dev)
    return buf


def standardize_advantages(adv, num_sets=1, min_std=1e-4, step0=0, n_steps=None, out=None, return_moments=False):
    """-> adv standardised per weight set, a float32 tensor of adv's shape: (adv - mean) / max(min_std, std) with the set's
    mean and population std, what RLlib 0.7.6's PPO optimizers do to each policy's train batch before the SGD epochs
    (standardize_fields=["advantages"], min_std 1e-4; stated from memory of its source).  include/ssd.h, BATCH MOMENTS states
    every operation: two-pass float64 moments in a fixed summation order, one rounding to float32, so that two runs of one
    seed give the same bits on any device.

    adv float32 [R, ...] contiguous (any trailing shape, as compute_advantages takes: [K,E,N] from sample(), [M,E], [R,L]).
    The weight set of trailing index l is l % num_sets, as the loss calls have it: num_sets is 1 or policy.num_sets, and
    divides the trailing size.  Row k of the call is ring slot (step0 + k) % R, k < n_steps (default R); rows outside the call
    are not written (zero in a tensor this function allocates).  out: the tensor to write into; it may be adv itself.
    return_moments: -> (out, moments) with moments float64 [num_sets, 2] = (mean, std) per set, on adv's device.
    CUDA tensors go to the kernels (three launches on torch's current stream, no synchronisation, no temporary of the
    batch's size); CPU tensors run a NumPy restatement of the same contract, bit for bit.
    """
    import torch
    shape, dev, R, L, num_sets, step0, n_steps = _moments_args(torch, adv, num_sets, step0, n_steps, "adv")
    min_std = float(min_std)
    if not (math.isfinite(min_std) and min_std > 0.0):
        raise ValueError("min_std must be finite and > 0")
    if out is None:
        out = (torch.empty if n_steps == R else torch.zeros)(shape, dtype=torch.float32, device=dev)
    else:
        _check(torch, out, torch.float32, shape, dev, "out")
    moments = torch.empty((num_sets, 2), dtype=torch.float64, device=dev) if return_moments else None
    target = _kernel_target(torch, dev)
    if target is None:
        rows = _slots(R, step0, n_steps)
        x = adv.numpy().reshape(R, L)[rows].reshape(-1, num_sets)
        res = np.empty_like(x)
        for p in range(num_sets):
            xs = x[:, p].astype(np.float64)
            mean, var = _mean_var(xs)
            sd = np.sqrt(var)
            denom = sd if sd > min_std else np.float64(min_std)
            res[:, p] = ((xs - mean) / denom).astype(np.float32)
            if moments is not None:
                moments[p, 0], moments[p, 1] = float(mean), float(sd)
        out.numpy().reshape(R, L)[rows] = res.reshape(n_steps, L)
        return (out, moments) if return_moments else out
    index, stream = target
    scratch = _scratch(torch, dev, index, _capi.SSD_MOM_SCRATCH_DOUBLES(n_steps, L, num_sets))
    _capi.moments_check(_capi.lib().ssd_standardize(
        _ptr(adv), L, R, step0, n_steps, num_sets, min_std, _ptr(scratch), _ptr(moments), _ptr(out), index, stream))
    return (out, moments) if return_moments else out


def explained_variance(targets, pred, num_sets=1, step0=0, n_steps=None):
    """-> float32 [num_sets] on the tensors' device: max(-1, 1 - var(targets - pred) / var(targets)) per weight set, RLlib's
    vf_explained_var (rllib/utils/explained_variance.py, stated from memory) of value_targets and the value predictions.

    targets and pred float32 [R, ...] of one shape, contiguous, on one device; num_sets, step0 and n_steps as
    standardize_advantages takes them.  The difference is formed in float64 and both population variances are the two-pass
    float64 moments of include/ssd.h, BATCH MOMENTS, in its fixed order.  var(targets) == 0 follows IEEE arithmetic: -1 when the
    residual's variance is > 0, NaN when both are 0.  CUDA tensors go to the kernels (three launches on torch's current
    stream, no synchronisation); CPU tensors run the NumPy restatement, bit for bit.
    """
    import torch
    shape, dev, R, L, num_sets, step0, n_steps = _moments_args(torch, targets, num_sets, step0, n_steps, "targets")
    _check(torch, pred, torch.float32, shape, dev, "pred")
    out = torch.empty(num_sets, dtype=torch.float32, device=dev)
    target = _kernel_target(torch, dev)
    if target is None:
        rows = _slots(R, step0, n_steps)
        y = targets.numpy().reshape(R, L)[rows].reshape(-1, num_sets)
        q = pred.numpy().reshape(R, L)[rows].reshape(-1, num_sets)
        with np.errstate(divide="ignore", invalid="ignore"):
            for p in range(num_sets):
                ys = y[:, p].astype(np.float64)
                var_y = _mean_var(ys)[1]
                var_d = _mean_var(ys - q[:, p].astype(np.float64))[1]
                r = np.float64(1.0) - var_d / var_y
                out[p] = float(np.float32(-1.0 if r < -1.0 else r))
        return out
    index, stream = target
    scratch = _scratch(torch, dev, index, _capi.SSD_MOM_SCRATCH_DOUBLES(n_steps, L, num_sets))
    _capi.moments_check(_capi.lib().ssd_explained_variance(
        _ptr(targets), _ptr(pred), L, R, step0, n_steps, num_sets, _ptr(scratch), _ptr(out), index, stream))
    return out


def update_kl_coeff(kl_coeff, sampled_kl, kl_target):
    """-> the next KL coefficient(s): RLlib 0.7.6's KLCoeffMixin.update_kl (stated from memory), elementwise over scalars or
    arrays that broadcast: kl_coeff * 1.5 where sampled_kl > 2 * kl_target, kl_coeff * 0.5 where sampled_kl < 0.5 * kl_target,
    kl_coeff otherwise (a sampled_kl exactly on a threshold changes nothing).  Pure NumPy on the host: sampled_kl is the "kl"
    statistic the PPO loss calls return (one value per weight set).  The loss calls take ONE scalar kl_coeff for all weight
    sets; a coefficient per weight set inside the loss kernels is out of scope here, so a caller with several sets either
    adapts one coefficient from the mean kl, or runs one loss call per coefficient.  Scalars in, a Python float out; arrays
    in, a float64 array out."""
    k = np.asarray(kl_coeff, np.float64)
    s = np.asarray(sampled_kl, np.float64)
    t = np.asarray(kl_target, np.float64)
    nxt = np.where(s > 2.0 * t, k * 1.5, np.where(s < 0.5 * t, k * 0.5, k))
    return float(nxt) if nxt.ndim == 0 else nxt
