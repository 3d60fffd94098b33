"""Sequential NumPy restatement of the episode statistics (include/ssd.h, ssd_stats_*).

One env at a time, one step at a time, Python integers for every count and sum, float64 scalars for the metrics in the
stated order.  The GPU fold must match it bit for bit, NaNs included."""
import numpy as np


def hits_of(r):
    return (1 - int(r)) // 50                                    # floor division


def metrics(R, pos, tsum, tagged, T):
    """(U, Eq, S, P) of one episode of T steps from the per-agent lists."""
    N = len(R)
    C = sum(R)
    G = sum(abs(a - b) for a in R for b in R)
    with np.errstate(divide="ignore", invalid="ignore"):
        U = np.float64(C) / np.float64(T)
        Eq = np.float64(1.0) - np.float64(G) / np.float64(2 * N * C)
        s, n = np.float64(0.0), 0
        for i in range(N):
            if pos[i] > 0:
                s = s + np.float64(tsum[i]) / np.float64(pos[i])
                n += 1
        S = s / np.float64(n)
        P = np.float64(N * T - sum(tagged)) / np.float64(T)
    return [U, Eq, S, P]


class RefStats(object):
    def __init__(self, E, N):
        self.E, self.N = E, N
        self.t = [0] * E
        self.open = [self._zero() for _ in range(E)]
        self._clear()

    def _zero(self):
        return {k: [0] * self.N for k in ("R", "pos", "tsum", "tagged", "hits")}

    def _clear(self):
        E, N = self.E, self.N
        self.episodes, self.truncated, self.sum_len, self.sum_coll = [0] * E, [0] * E, [0] * E, [0] * E
        self.sum_ret, self.sum_hits, self.sum_tagged = [[0] * N for _ in range(E)], [[0] * N for _ in range(E)], [[0] * N for _ in range(E)]
        self.msum = [[np.float64(0.0)] * 4 for _ in range(E)]
        self.mcnt = [[0] * 4 for _ in range(E)]
        self.last_len, self.last_ret = [0] * E, [[0] * N for _ in range(E)]
        self.last_m = [[np.float64(0.0)] * 4 for _ in range(E)]

    def _close(self, e):
        o, T = self.open[e], self.t[e]
        m = metrics(o["R"], o["pos"], o["tsum"], o["tagged"], T)
        self.episodes[e] += 1
        self.sum_len[e] += T
        self.sum_coll[e] += sum(o["R"])
        for q in range(4):
            if np.isfinite(m[q]):
                self.msum[e][q] = self.msum[e][q] + m[q]
                self.mcnt[e][q] += 1
        self.last_m[e] = list(m)
        self.last_len[e] = T
        self.last_ret[e] = list(o["R"])
        for i in range(self.N):
            self.sum_ret[e][i] += o["R"][i]
            self.sum_hits[e][i] += o["hits"][i]
            self.sum_tagged[e][i] += o["tagged"][i]
        self.open[e], self.t[e] = self._zero(), 0

    def discard(self, mask=None):
        for e in range(self.E):
            if (mask is None or mask[e]) and self.t[e] > 0:
                self.truncated[e] += 1
                self.open[e], self.t[e] = self._zero(), 0

    def fold(self, rew, done=None, step0=0, n_steps=None, reset_every=0):
        rew = np.asarray(rew)
        ring = rew.shape[0]
        n_steps = ring if n_steps is None else n_steps
        assert n_steps <= ring
        if n_steps > 0 and reset_every > 0 and step0 % reset_every == 0:
            self.discard()
        for k in range(n_steps):
            slot = (step0 + k) % ring
            for e in range(self.E):
                self.t[e] += 1
                o = self.open[e]
                for i in range(self.N):
                    r = int(rew[slot, e, i])
                    h = hits_of(r)
                    o["R"][i] += r
                    o["hits"][i] += h
                    if r > 0:
                        o["pos"][i] += 1
                        o["tsum"][i] += self.t[e]
                    if h > 0:
                        o["tagged"][i] += 1
                end = (done is not None and done[slot, e, 0] != 0) or (reset_every > 0 and (step0 + k + 1) % reset_every == 0)
                if end:
                    self._close(e)

    def drain(self, keep=False):
        E, N = self.E, self.N
        out = {"counts": np.array([[self.episodes[e], self.truncated[e], self.sum_len[e], self.sum_coll[e]] for e in range(E)],
                                  np.int64).reshape(E, 4),
               "agent_sums": np.array([[self.sum_ret[e], self.sum_hits[e], self.sum_tagged[e]] for e in range(E)], np.int64).reshape(E, 3, N),
               "metric_sums": np.array(self.msum, np.float64).reshape(E, 4),
               "metric_counts": np.array(self.mcnt, np.int64).reshape(E, 4),
               "last_len": np.array(self.last_len, np.int64),
               "last_ret": np.array(self.last_ret, np.int64).reshape(E, N),
               "last_metrics": np.array(self.last_m, np.float64).reshape(E, 4)}
        if not keep:
            self._clear()
        return out


def summary(drained, N):
    """The RLlib-style means of one drain, restated: env-order sums, float64(total) / float64(count)."""
    c, a = drained["counts"], drained["agent_sums"]
    E = c.shape[0]
    eps = sum(int(c[e, 0]) for e in range(E))

    def div(x, n):
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.float64(x) / np.float64(n))

    out = {"episodes": eps, "truncated": sum(int(c[e, 1]) for e in range(E)),
           "episode_len_mean": div(sum(int(c[e, 2]) for e in range(E)), eps),
           "episode_reward_mean": div(sum(int(c[e, 3]) for e in range(E)), eps),
           "policy_reward_mean": {"agent-%d" % i: div(sum(int(a[e, 0, i]) for e in range(E)), eps) for i in range(N)}}
    for q, name in enumerate(("efficiency", "equality", "sustainability", "peace")):
        s = np.float64(0.0)
        for e in range(E):
            s = s + drained["metric_sums"][e, q]
        out[name] = div(s, sum(int(drained["metric_counts"][e, q]) for e in range(E)))
    return out


def same(a, b):
    """Equality of two drains / summaries bit for bit, except that any NaN equals any NaN (where the NaNs fall must agree;
    their sign and payload are the hardware's: x86 and the GPU make different default NaNs)."""
    if isinstance(a, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (int, float)) and isinstance(b, (int, float)):
        if type(a) is not type(b):
            return False
        a, b = np.asarray(a), np.asarray(b)
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        return bool(np.array_equal(na, nb)) and a[~na].tobytes() == b[~nb].tobytes()
    return a.tobytes() == b.tobytes()
