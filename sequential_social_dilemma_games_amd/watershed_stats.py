"""Per-episode statistics of the Watershed games, folded inside the stepping kernel (csrc/ssd_ws_stats.hip and the stats
instances of csrc/ssd_watershed.hip; include/ssd.h ssd_ws_stats_*).

What RLlib logs for every run (episode_reward_mean, policy_reward_mean, episode_len_mean) and the three custom metrics the
reference's Watershed launchers install through social_dilemmas/envs/watershedLogging.py: violations, Equality and Utility.
Two of them are built from values that exist only in the env's info dict (viol, running_rew, true_end), which no rollout
call records; an attached handle sees them in the kernel, and nothing goes through the host per step.  DESIGN.md section 24
has the definitions and the one assumption about RLlib they rest on.

    stats = WatershedEpisodeStats(SEQ, E)
    eng.attach_stats(stats)                       # before the reset that starts the first episode to be counted
    eng.reset()
    batch = eng.sample(policy, 430)               # or step() / rollout_actions() / rollout_policy()
    stats.summary()        # {"episode_reward_mean": ..., "custom_metrics": {"violations_mean": ..., "Equality_mean": ..., ...}}
"""
import ctypes as C

import numpy as np

from . import _capi

METRICS = ("violations", "Equality", "Utility")
NUM_AGENTS = {_capi.SSD_WS_SEQ: 4, _capi.SSD_WS_SEQ_COMM: 8}
# the arrays of a drain, in the order of ssd_ws_stats_drain's arguments: name, dtype, trailing shape
DRAINED = (("counts", np.int64, (3,)), ("reward_sum", np.float64, ()), ("agent_sums", np.float64, (8,)),
           ("metric_sums", np.float64, (3,)), ("metric_counts", np.int64, (3,)), ("metric_min", np.float64, (3,)),
           ("metric_max", np.float64, (3,)), ("last_len", np.int64, ()), ("last_reward", np.float64, ()),
           ("last_agent", np.float64, (8,)), ("last_total_rews", np.float64, (4,)), ("last_metrics", np.float64, (3,)))


def summarize(drained, variant):
    """RLlib-style result of one drain (the per-env arrays of WatershedEpisodeStats.drain()), reduced over envs in env order:
    integer sums are exact, every float64 sum is added env after env from 0.0.  A mean (min, max) over nothing is NaN."""
    counts = drained["counts"]
    episodes, truncated = int(counts[:, 0].sum()), int(counts[:, 1].sum())

    def mean(total, n):
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.float64(total) / np.float64(n))

    def fsum(column):
        total = 0.0
        for v in column.tolist():
            total += v
        return total

    out = {"episodes": episodes, "truncated": truncated,
           "episode_len_mean": mean(int(counts[:, 2].sum()), episodes),
           "episode_reward_mean": mean(fsum(drained["reward_sum"]), episodes),
           "policy_reward_mean": {"agent-%d" % i: mean(fsum(drained["agent_sums"][:, i]), episodes)
                                  for i in range(NUM_AGENTS[int(variant)])}}
    custom = {}
    for q, name in enumerate(METRICS):
        n = drained["metric_counts"][:, q]
        have = n > 0
        custom[name + "_mean"] = mean(fsum(drained["metric_sums"][:, q]), int(n.sum()))
        custom[name + "_min"] = float(drained["metric_min"][have, q].min()) if have.any() else float("nan")
        custom[name + "_max"] = float(drained["metric_max"][have, q].max()) if have.any() else float("nan")
    out["custom_metrics"] = custom
    return out


class WatershedEpisodeStats(object):
    """Episode accumulators for E Watershed envs of one variant on one device.  WatershedVecEngine.attach_stats(stats) makes the
    engine's stepping calls fold into it; discard() and drain() are enqueued on torch's current stream of that device; drain(),
    last_episode() and summary() then copy to the host (synchronous)."""

    def __init__(self, variant, num_envs, device=0):
        import torch
        self.variant, self.E, self.device = int(variant), int(num_envs), int(device)
        self._torch, self._dev = torch, torch.device("cuda", self.device)
        self._h = C.c_void_p()
        L = _capi.lib()
        _capi.ws_stats_check(L.ssd_ws_stats_create(self.variant, self.E, self.device, C.byref(self._h)))
        self._L = L
        self._out = None

    def close(self):
        """Frees the handle.  An engine that still holds it must detach it first (attach_stats(None)) or be closed."""
        if getattr(self, "_h", None) is not None and self._h:
            _capi.ws_stats_check(self._L.ssd_ws_stats_destroy(self._h), self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self._dev).cuda_stream)

    def discard(self, mask=None):
        """Discard the open episode of the envs with mask != 0 (bool / uint8 [E]; None = all): one that had a step counts as
        truncated, and the env is not counted again before its next reset."""
        torch = self._torch
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self._dev).to(torch.uint8).contiguous()
            if tuple(m.shape) != (self.E,):
                raise ValueError("mask must be bool / uint8 [%d]" % self.E)
        _capi.ws_stats_check(self._L.ssd_ws_stats_discard(self._h, None if m is None else C.c_void_p(m.data_ptr()), self._stream()),
                             self._h)

    def _copy_out(self, keep):
        torch = self._torch
        if self._out is None:
            self._out = {name: torch.empty((self.E,) + shape, dtype=torch.int64 if dt is np.int64 else torch.float64, device=self._dev)
                         for name, dt, shape in DRAINED}
        p = [C.c_void_p(self._out[name].data_ptr()) for name, _, _ in DRAINED]
        _capi.ws_stats_check(self._L.ssd_ws_stats_drain(self._h, *p, _capi.SSD_STATS_KEEP if keep else 0, self._stream()), self._h)
        return {k: v.cpu().numpy() for k, v in self._out.items()}

    def drain(self, keep=False):
        """The accumulators since the last drain, as host arrays, and clears them (unless keep).  Metrics in the order
        violations, Equality, Utility:
        counts int64 [E,3] (episodes, truncated, sum of lengths), reward_sum float64 [E], agent_sums float64 [E,8],
        metric_sums float64 [E,3] / metric_counts int64 [E,3] (finite values only), metric_min / metric_max float64 [E,3]
        (+inf / -inf where metric_counts is 0), and the last episode that finished: last_len int64 [E] (0: none), last_reward
        float64 [E], last_agent float64 [E,8], last_total_rews float64 [E,4], last_metrics float64 [E,3]."""
        return self._copy_out(keep)

    def last_episode(self):
        """The last episode each env finished since the last drain, without draining: {"len" [E] (0: none), "reward" [E],
        "agent_reward" [E,8], "total_rews" [E,4], "violations" [E], "Equality" [E], "Utility" [E]}."""
        d = self._copy_out(keep=True)
        out = {"len": d["last_len"], "reward": d["last_reward"], "agent_reward": d["last_agent"], "total_rews": d["last_total_rews"]}
        for q, name in enumerate(METRICS):
            out[name] = d["last_metrics"][:, q].copy()
        return out

    def summary(self):
        """drain() reduced over envs (summarize): episodes, truncated, episode_len_mean, episode_reward_mean,
        policy_reward_mean {"agent-i": ...} and custom_metrics {violations,Equality,Utility}_{mean,min,max}, RLlib's naming."""
        return summarize(self.drain(), self.variant)
