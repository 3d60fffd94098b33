"""Per-episode statistics of batched rollouts, folded on the device (csrc/ssd_stats.hip, include/ssd.h ssd_stats_*).

What RLlib logs for every run (episode_reward_mean, policy_reward_mean, episode_len_mean) and the social-outcome metrics of
Perolat et al. 2017 (efficiency, equality, sustainability, peace), computed from the rew [ring,E,N] (and done) rings the
stepping calls already write: nothing goes through the host per step.  DESIGN.md section 10 has the definitions.

    stats = EpisodeStats(E, N)
    eng.rollout_random(1000, obs, rew, reset_every=1000, fused=True, stats=stats)    # or stats.fold(rew, done, ...)
    stats.summary()        # {"episode_reward_mean": ..., "policy_reward_mean": {"agent-0": ...}, "efficiency": ..., ...}
"""
import ctypes as C

import numpy as np

from . import _capi

METRICS = ("efficiency", "equality", "sustainability", "peace")


def summarize(drained, num_agents):
    """RLlib-style means of one drain (the per-env arrays of EpisodeStats.drain()), reduced over envs in env order:
    integer sums are exact, each metric's float64 sum is added env after env from 0.0.  A mean over nothing is NaN."""
    counts, agent_sums = drained["counts"], drained["agent_sums"]
    episodes, truncated = int(counts[:, 0].sum()), int(counts[:, 1].sum())

    def mean(total, n):
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.float64(total) / np.float64(n))

    out = {"episodes": episodes, "truncated": truncated,
           "episode_len_mean": mean(int(counts[:, 2].sum()), episodes),
           "episode_reward_mean": mean(int(counts[:, 3].sum()), episodes),
           "policy_reward_mean": {"agent-%d" % i: mean(int(agent_sums[:, 0, i].sum()), episodes) for i in range(num_agents)}}
    for q, name in enumerate(METRICS):
        total = 0.0
        for v in drained["metric_sums"][:, q].tolist():
            total += v
        out[name] = mean(total, int(drained["metric_counts"][:, q].sum()))
    return out


class EpisodeStats(object):
    """Episode accumulators for E envs of N agents on one device.  fold() / discard() / drain() are enqueued on torch's current
    stream of that device; drain(), last_episode() and summary() then copy to the host (synchronous)."""

    def __init__(self, num_envs, num_agents, device=0):
        import torch
        self.E, self.N, self.device = int(num_envs), int(num_agents), int(device)
        self._torch, self._dev = torch, torch.device("cuda", self.device)
        self._h = C.c_void_p()
        L = _capi.lib()
        _capi.stats_check(L.ssd_stats_create(self.E, self.N, self.device, C.byref(self._h)))
        self._L = L
        self._out = None

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.ssd_stats_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self._dev).cuda_stream)

    def _check(self, t, dtype, shape, name):
        if not isinstance(t, self._torch.Tensor) or t.device != self._dev or t.dtype != dtype or tuple(t.shape) != tuple(shape) \
                or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, tuple(shape), self._dev))

    def set_chunk(self, steps):
        """Steps per time chunk of the fold kernel (0 = automatic).  Changes speed only, never a result."""
        _capi.stats_check(self._L.ssd_stats_set_chunk(self._h, int(steps)), self._h)

    def fold(self, rew, done=None, step0=0, n_steps=None, reset_every=0):
        """Add n_steps steps (default: the whole ring): step k reads slot (step0 + k) % R of rew int32 [R,E,N] and of done
        uint8 [R,E,N] (optional).  An episode ends where done[slot, e, 0] != 0, or where (step0 + k + 1) % reset_every == 0;
        when step0 % reset_every == 0 every open episode is first discarded (the rollout calls' full reset)."""
        torch = self._torch
        ring = int(rew.shape[0]) if isinstance(rew, torch.Tensor) and rew.dim() == 3 else -1
        self._check(rew, torch.int32, (ring, self.E, self.N), "rew")
        if done is not None:
            self._check(done, torch.uint8, (ring, self.E, self.N), "done")
        n_steps = ring if n_steps is None else int(n_steps)
        step0, reset_every = int(step0), int(reset_every)
        if n_steps < 0 or n_steps > ring:
            raise ValueError("n_steps (%d) must be 0..%d, the ring length: a fold reads each slot once" % (n_steps, ring))
        if step0 < 0 or reset_every < 0:
            raise ValueError("step0 and reset_every must be >= 0")
        _capi.stats_check(self._L.ssd_stats_fold(self._h, C.c_void_p(rew.data_ptr()),
                                                 None if done is None else C.c_void_p(done.data_ptr()), ring, step0, n_steps,
                                                 reset_every, 0, self._stream()), self._h)

    def discard(self, mask=None):
        """Discard the open episode of the envs with mask != 0 (uint8 [E] device tensor; None = all): they count as truncated."""
        if mask is not None:
            self._check(mask, self._torch.uint8, (self.E,), "mask")
        _capi.stats_check(self._L.ssd_stats_discard(self._h, None if mask is None else C.c_void_p(mask.data_ptr()),
                                                    self._stream()), self._h)

    def _copy_out(self, keep):
        torch, E, N = self._torch, self.E, self.N
        if self._out is None:
            i64, f64 = torch.int64, torch.float64
            self._out = {"counts": torch.empty((E, 4), dtype=i64, device=self._dev),
                         "agent_sums": torch.empty((E, 3, N), dtype=i64, device=self._dev),
                         "metric_sums": torch.empty((E, 4), dtype=f64, device=self._dev),
                         "metric_counts": torch.empty((E, 4), dtype=i64, device=self._dev),
                         "last_len": torch.empty((E,), dtype=i64, device=self._dev),
                         "last_ret": torch.empty((E, N), dtype=i64, device=self._dev),
                         "last_metrics": torch.empty((E, 4), dtype=f64, device=self._dev)}
        o = self._out
        p = [C.c_void_p(o[k].data_ptr()) for k in ("counts", "agent_sums", "metric_sums", "metric_counts", "last_len", "last_ret",
                                                   "last_metrics")]
        _capi.stats_check(self._L.ssd_stats_drain(self._h, *p, _capi.SSD_STATS_KEEP if keep else 0, self._stream()), self._h)
        return {k: v.cpu().numpy() for k, v in o.items()}

    def drain(self, keep=False):
        """The accumulators since the last drain, as host arrays, and clears them (unless keep):
        counts int64 [E,4] (episodes, truncated, sum of lengths, sum of collective returns), agent_sums int64 [E,3,N] (sums
        of returns, hits, tagged steps), metric_sums float64 [E,4] / metric_counts int64 [E,4] (efficiency, equality,
        sustainability, peace: finite values only), last_len int64 [E] (0: no episode ended), last_ret int64 [E,N],
        last_metrics float64 [E,4]: the last episode that ended."""
        return self._copy_out(keep)

    def last_episode(self):
        """The last episode each env ended since the last drain, without draining: {"len" [E] (0: none), "ret" [E,N],
        "efficiency" [E], "equality" [E], "sustainability" [E], "peace" [E]}."""
        d = self._copy_out(keep=True)
        out = {"len": d["last_len"], "ret": d["last_ret"]}
        for q, name in enumerate(METRICS):
            out[name] = d["last_metrics"][:, q].copy()
        return out

    def summary(self):
        """drain() reduced over envs: episode_len_mean, episode_reward_mean (the collective return, RLlib's multi-agent
        episode reward), policy_reward_mean {"agent-i": ...}, the four metric means, episodes, truncated."""
        return summarize(self.drain(), self.N)
