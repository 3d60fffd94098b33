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
"""
import ctypes as C
import math

import numpy as np

from . import _capi


def _check(torch, t, dtype, shape, device, name):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device \
            or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, tuple(shape), device))


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
    if not isinstance(rew, torch.Tensor) or rew.dim() < 1:
        raise ValueError("rew must be an int32 tensor of shape [R, ...]")
    shape, dev = tuple(rew.shape), rew.device
    R = shape[0]
    L = int(np.prod(shape[1:], dtype=np.int64))
    if R < 1 or L < 1:
        raise ValueError("rew holds no step")
    if L >= 2 ** 31 or R >= 2 ** 31:
        raise ValueError("rew is too large: fewer than 2^31 rows and trajectories")
    _check(torch, rew, torch.int32, shape, dev, "rew")
    use_gae, use_critic = bool(use_gae), bool(use_critic)
    if use_gae and not use_critic:
        raise ValueError("use_gae needs use_critic: generalised advantage estimation uses the value function")
    if value is not None or use_critic:
        _check(torch, value, torch.float32, shape, dev, "value")
    if last_value is not None:
        _check(torch, last_value, torch.float32, shape[1:], dev, "last_value")
    if done is not None:
        _check(torch, done, torch.uint8, shape, dev, "done")
    if bonus is not None:
        _check(torch, bonus, torch.float32, shape, dev, "bonus")
    gamma, lambda_, bonus_weight = float(gamma), float(lambda_), float(bonus_weight)
    if not (math.isfinite(gamma) and math.isfinite(lambda_)):
        raise ValueError("gamma and lambda_ must be finite")
    if bonus is not None and not math.isfinite(bonus_weight):
        raise ValueError("bonus_weight must be finite")
    step0 = int(step0)
    n_steps = R if n_steps is None else int(n_steps)
    if n_steps < 1 or n_steps > R:
        raise ValueError("n_steps (%d) must be 1..%d, the ring length: a call reads each slot once" % (n_steps, R))
    if step0 < 0 or step0 >= 2 ** 31:
        raise ValueError("step0 must be 0..2^31 - 1")
    if out is None:
        make = torch.empty if n_steps == R else torch.zeros
        adv, vt = make(shape, dtype=torch.float32, device=dev), make(shape, dtype=torch.float32, device=dev)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise ValueError("out must be a pair (advantages, value_targets)")
        adv, vt = out
        _check(torch, adv, torch.float32, shape, dev, "out[0]")
        _check(torch, vt, torch.float32, shape, dev, "out[1]")
        if adv.data_ptr() == vt.data_ptr():
            raise ValueError("out[0] and out[1] must be two tensors")
    if dev.type == "cpu":
        _host(rew, value, last_value, done, bonus, bonus_weight, gamma, lambda_, use_gae, use_critic, step0, n_steps, adv, vt)
        return adv, vt
    if dev.type != "cuda":
        raise ValueError("the tensors must be on the CPU or on a GPU, not on %s" % (dev,))
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    flags = (_capi.SSD_ADV_GAE if use_gae else 0) | (_capi.SSD_ADV_CRITIC if use_critic else 0)
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _capi.advantages_check(_capi.lib().ssd_advantages(ptr(rew), ptr(bonus), bonus_weight, ptr(value) if use_critic else None,
                                                      ptr(done), ptr(last_value), L, R, step0, n_steps, gamma, lambda_, flags,
                                                      ptr(adv), ptr(vt), index, stream))
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
    if not isinstance(rew, torch.Tensor) or rew.dim() < 1:
        raise ValueError("rew must be an int32 tensor of shape [R, ...]")
    shape, dev = tuple(rew.shape), rew.device
    R = shape[0]
    L = int(np.prod(shape[1:], dtype=np.int64))
    if R < 1 or L < 1:
        raise ValueError("rew holds no step")
    if L >= 2 ** 31 or R >= 2 ** 31:
        raise ValueError("rew is too large: fewer than 2^31 rows and trajectories")
    _check(torch, rew, torch.int32, shape, dev, "rew")
    _check(torch, value, torch.float32, shape, dev, "value")
    _check(torch, rhos, torch.float32, shape, dev, "rhos")
    if bootstrap_value is not None:
        _check(torch, bootstrap_value, torch.float32, shape[1:], dev, "bootstrap_value")
    if done is not None:
        _check(torch, done, torch.uint8, shape, dev, "done")
    if bonus is not None:
        _check(torch, bonus, torch.float32, shape, dev, "bonus")
    gamma, bonus_weight = float(gamma), float(bonus_weight)
    clip_rho, clip_pg = float(clip_rho_threshold), float(clip_pg_rho_threshold)
    if not math.isfinite(gamma):
        raise ValueError("gamma must be finite")
    if not (clip_rho > 0.0 and clip_pg > 0.0):
        raise ValueError("clip_rho_threshold and clip_pg_rho_threshold must be > 0 (inf: no clip)")
    if bonus is not None and not math.isfinite(bonus_weight):
        raise ValueError("bonus_weight must be finite")
    step0 = int(step0)
    n_steps = R if n_steps is None else int(n_steps)
    if n_steps < 1 or n_steps > R:
        raise ValueError("n_steps (%d) must be 1..%d, the ring length: a call reads each slot once" % (n_steps, R))
    if step0 < 0 or step0 >= 2 ** 31:
        raise ValueError("step0 must be 0..2^31 - 1")
    if out is None:
        make = torch.empty if n_steps == R else torch.zeros
        vs, pg = make(shape, dtype=torch.float32, device=dev), make(shape, dtype=torch.float32, device=dev)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise ValueError("out must be a pair (vs, pg_advantages)")
        vs, pg = out
        _check(torch, vs, torch.float32, shape, dev, "out[0]")
        _check(torch, pg, torch.float32, shape, dev, "out[1]")
        if vs.data_ptr() == pg.data_ptr():
            raise ValueError("out[0] and out[1] must be two tensors")
    if dev.type == "cpu":
        _host_vtrace(rew, value, rhos, bootstrap_value, done, bonus, bonus_weight, gamma, clip_rho, clip_pg, step0, n_steps, vs, pg)
        return vs, pg
    if dev.type != "cuda":
        raise ValueError("the tensors must be on the CPU or on a GPU, not on %s" % (dev,))
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _capi.vtrace_check(_capi.lib().ssd_vtrace(ptr(rew), ptr(bonus), bonus_weight, ptr(value), ptr(rhos), ptr(done),
                                              ptr(bootstrap_value), L, R, step0, n_steps, gamma, clip_rho, clip_pg, 0,
                                              ptr(vs), ptr(pg), index, stream))
    return vs, pg
