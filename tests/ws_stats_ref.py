"""Sequential NumPy restatement of the Watershed episode statistics (include/ssd.h, WATERSHED EPISODE STATISTICS; DESIGN.md
section 24).  Test infrastructure: what the stepping kernel's stats instances fold, written env by env and step by step from
the per-step records a caller can see -- the rew and done outputs, the agent output, and ssd_ws_info's viol and running_rew
taken after the step and BEFORE any reset of the env -- with every float64 operation a Python float operation in the stated
order.  It produces the arrays of WatershedEpisodeStats.drain() and, per env, the list of its finished episodes.
"""
import math

import numpy as np

DONE_ALL = 2
LAST_AGENT = {0: 3, 1: 7}
FIRST_VIOL_STEP = 4                       # agent-0's first info arrives with the episode's 4th step, in both variants


def episode_metrics(vsum, vcnt, total_rews):
    """(violations, Equality, Utility): np.mean of the appended viol vectors, and on_episode_end line for line."""
    with np.errstate(divide="ignore", invalid="ignore"):
        violations = float(np.float64(vsum) / np.float64(vcnt))
        usum = 0.0
        for v in total_rews:
            usum = usum + float(v)
        den = 2.0 * usum
        num = 0.0
        for i in total_rews:
            for j in total_rews:
                num = num + math.fabs(float(i) - float(j))
        equality = float(np.float64(1.0) - np.float64(num) / np.float64(den))
    return violations, equality, den


class WsStatsRef(object):
    def __init__(self, variant, num_envs):
        self.variant, self.E = int(variant), int(num_envs)
        E = self.E
        self.open = np.zeros(E, bool)
        self.len = np.zeros(E, np.int64)
        self.rew = [0.0] * E
        self.agent = [[0.0] * 8 for _ in range(E)]
        self.vsum = np.zeros(E, np.int64)
        self.vcnt = np.zeros(E, np.int64)
        self.episodes = [[] for _ in range(E)]                    # every finished episode of env e, in order
        self._clear()

    def _clear(self):
        E = self.E
        self.acc = {"counts": np.zeros((E, 3), np.int64), "reward_sum": np.zeros(E), "agent_sums": np.zeros((E, 8)),
                    "metric_sums": np.zeros((E, 3)), "metric_counts": np.zeros((E, 3), np.int64),
                    "metric_min": np.full((E, 3), np.inf), "metric_max": np.full((E, 3), -np.inf),
                    "last_len": np.zeros(E, np.int64), "last_reward": np.zeros(E), "last_agent": np.zeros((E, 8)),
                    "last_total_rews": np.zeros((E, 4)), "last_metrics": np.zeros((E, 3))}

    def _zero(self, e):
        self.len[e] = 0
        self.rew[e] = 0.0
        self.agent[e] = [0.0] * 8
        self.vsum[e] = self.vcnt[e] = 0

    def discard(self, mask=None, reopen=False):
        """ssd_ws_stats_discard; with reopen, what ssd_ws_reset does to the handle of an attached engine."""
        for e in range(self.E):
            if mask is not None and not mask[e]:
                continue
            if self.open[e] and self.len[e] > 0:
                self.acc["counts"][e, 1] += 1
            self.open[e] = reopen
            self._zero(e)

    def reset(self, mask=None):
        self.discard(mask, reopen=True)

    def step(self, rew, done, agent, viol, running_rew, auto_reset=False, live=None):
        """One step of every env: rew f64 [E] and done u8 [E] as the rings get them, agent i8 [E] as the agent ring gets it
        (at a DONE_ALL step the receiver is the variant's last agent whatever an auto-reset wrote there), viol u8 [E,6] and
        running_rew f64 [E,4] of the state the step left.  auto_reset: the env is reset (a new episode opens) where the step
        set DONE_ALL.  live: bool [E], False for a never-reset env (ignored)."""
        a = self.acc
        for e in range(self.E):
            if live is not None and not live[e]:
                continue
            ended = bool(int(done[e]) & DONE_ALL)
            if self.open[e]:
                r = float(rew[e])
                receiver = LAST_AGENT[self.variant] if ended else int(agent[e])
                self.len[e] += 1
                self.rew[e] = self.rew[e] + r
                self.agent[e][receiver] = self.agent[e][receiver] + r
                if self.len[e] >= FIRST_VIOL_STEP:
                    self.vsum[e] += int(np.asarray(viol[e]).sum())
                    self.vcnt[e] += 6
            if ended:
                if self.open[e]:
                    tot = [float(v) for v in running_rew[e]]
                    met = episode_metrics(int(self.vsum[e]), int(self.vcnt[e]), tot)
                    self.episodes[e].append({"len": int(self.len[e]), "reward": self.rew[e], "agent_reward": list(self.agent[e]),
                                             "total_rews": tot, "violations": met[0], "Equality": met[1], "Utility": met[2]})
                    a["counts"][e, 0] += 1
                    a["counts"][e, 2] += self.len[e]
                    a["reward_sum"][e] = float(a["reward_sum"][e]) + self.rew[e]
                    a["last_len"][e], a["last_reward"][e] = self.len[e], self.rew[e]
                    for j in range(8):
                        a["agent_sums"][e, j] = float(a["agent_sums"][e, j]) + self.agent[e][j]
                        a["last_agent"][e, j] = self.agent[e][j]
                    a["last_total_rews"][e] = tot
                    for m in range(3):
                        v = met[m]
                        a["last_metrics"][e, m] = v
                        if math.isfinite(v):
                            a["metric_sums"][e, m] = float(a["metric_sums"][e, m]) + v
                            a["metric_counts"][e, m] += 1
                            a["metric_min"][e, m] = min(float(a["metric_min"][e, m]), v)
                            a["metric_max"][e, m] = max(float(a["metric_max"][e, m]), v)
                self._zero(e)
                self.open[e] = bool(auto_reset)

    def drain(self, keep=False):
        out = {k: v.copy() for k, v in self.acc.items()}
        if not keep:
            self._clear()
        return out


def assert_drains_equal(got, want, what=""):
    """Bit for bit: float64 arrays compared through their int64 views (NaN equals NaN, -0.0 differs from 0.0)."""
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k in sorted(want):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        gi, wi = (g.view(np.int64), w.view(np.int64)) if g.dtype == np.float64 else (g, w)
        bad = np.argwhere(gi != wi)
        assert bad.size == 0, "%s %s: %d entries differ, first at %s: %r != %r" % (what, k, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


def assert_summaries_equal(got, want):
    def flat(d, pre=""):
        for k, v in d.items():
            if isinstance(v, dict):
                for kv in flat(v, pre + k + "."):
                    yield kv
            else:
                yield pre + k, v
    g, w = dict(flat(got)), dict(flat(want))
    assert sorted(g) == sorted(w)
    for k in w:
        if isinstance(w[k], float):
            assert np.float64(g[k]).view(np.int64) == np.float64(w[k]).view(np.int64), (k, g[k], w[k])
        else:
            assert g[k] == w[k], (k, g[k], w[k])
