#!/usr/bin/env python3
"""Generate the Watershed episode-statistics golden vectors in tests/golden/watershed/stats_*.npz from the REFERENCE itself.

Runs only in the build container (needs the reference checkout gen_golden_watershed.py names); the fixtures it writes are
committed, the reference is never copied.  Usage:  python tests/golden/gen_golden_watershed_stats.py

Method: the reference's envs (social_dilemmas/envs/watershedOrderedComm.py, imported by gen_golden_watershed.import_reference
with its PRNG proxy) are stepped with random actions, and the reference's OWN callbacks (social_dilemmas/envs/
watershedLogging.py: on_episode_start, on_episode_step / on_episode_step_comm, on_episode_end) are called on a stand-in for
RLlib's episode object.  RLlib itself is not available, so what its sampler does around the callbacks is an ASSUMPTION, and
this stand-in encodes exactly it and nothing more:
    * on_episode_step runs once after every env.step, the last one included;
    * last_info_for(a) is the latest info the env returned for agent a in this episode (None before the first);
    * user_data and custom_metrics are plain dicts.
Besides the callbacks' three custom metrics, RLlib's own per-episode numbers are recorded as DESIGN.md section 24 defines them:
the episode length, the float64 sum of every reward the env returned (in step order, from 0.0), and the same per receiving agent.

One file per (class, local_rew) with local_obs = 0, plus one local_obs = 1 case: NSEEDS envs (env index = row) x EPISODES
episodes each.  Actions: withdrawal fractions uniform in [0, 1) as float32 (1,) arrays, comm messages Python ints 0..4.

Recorded: actions f32 [NSEEDS, EPISODES * L] (the acting agent's, step after step), and per episode [NSEEDS, EPISODES, ...]:
len, reward, agent_reward [8], total_rews [4], violations, Equality, Utility.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden_watershed as G  # noqa: E402

OUT = G.OUT
NSEEDS = 3
EPISODES = 3
CASES = ((0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1))         # comm, local_rew, local_obs


class Episode(object):
    """The stand-in for RLlib's MultiAgentEpisode: what the callbacks touch, under the assumption stated above."""

    def __init__(self):
        self.user_data, self.custom_metrics = {}, {}
        self._last_info = {}
        self.length = 0
        self.total_reward = 0.0
        self.agent_rewards = [0.0] * 8

    def last_info_for(self, agent_id):
        return self._last_info.get(agent_id)

    def add(self, rew, info):
        """What one env.step returned."""
        self.length += 1
        for aid, r in rew.items():
            self.total_reward += float(r)                        # float64, whatever type the env used
            self.agent_rewards[int(aid.split("-")[1])] += float(r)
        self._last_info.update(info)


def name_of(comm, local_rew, local_obs):
    return "stats_%s_r%d_o%d.npz" % ("seqcomm" if comm else "seq", local_rew, local_obs)


def record(W, cb, comm, local_rew, local_obs):
    cls = W.WatershedSeqCommEnv if comm else W.WatershedSeqEnv
    on_step = cb.on_episode_step_comm if comm else cb.on_episode_step
    L = 131 if comm else 43
    z = lambda *s, d=np.float64: np.zeros((NSEEDS, EPISODES) + s, d)  # noqa: E731
    out = dict(actions=np.zeros((NSEEDS, EPISODES * L), np.float32), len=z(d=np.int64), reward=z(), agent_reward=z(8),
               total_rews=z(4), violations=z(), Equality=z(), Utility=z())
    for s in range(NSEEDS):
        rng = np.random.default_rng(500000 + 1000 * comm + 10 * local_rew + local_obs + 7919 * s)
        G.CTX.env, G.CTX.episode = s, -1
        env = cls(return_agent_actions=False, local_rew=bool(local_rew), local_obs=bool(local_obs))
        t = 0
        for ep in range(EPISODES):
            G.CTX.episode += 1
            obs = env.reset()
            episode = Episode()
            cb.on_episode_start({"episode": episode})
            done = {"__all__": False}
            while not done["__all__"]:
                aid = next(iter(obs))
                if comm and int(aid.split("-")[1]) < 4:
                    act = int(rng.integers(0, 5))
                    out["actions"][s, t] = act
                else:
                    act = rng.random(1).astype(np.float32)
                    out["actions"][s, t] = act[0]
                obs, rew, done, info = env.step({aid: act})
                t += 1
                episode.add(rew, info)
                on_step({"episode": episode})
            cb.on_episode_end({"episode": episode})
            assert episode.length == L and t == (ep + 1) * L, "episode of %d steps" % episode.length
            m = episode.custom_metrics
            out["len"][s, ep] = episode.length
            out["reward"][s, ep] = episode.total_reward
            out["agent_reward"][s, ep] = episode.agent_rewards
            out["total_rews"][s, ep] = [float(v) for v in episode.user_data["total_rews"]]
            out["violations"][s, ep], out["Equality"][s, ep], out["Utility"][s, ep] = m["violations"], m["Equality"], m["Utility"]
            assert all(type(v) is np.float64 for v in episode.user_data["total_rews"]), "total_rews are float64 at the end"
            assert all(np.isfinite(float(m[k])) for k in m), "the finite-only rule drops nothing for these inputs"
    out["meta"] = np.array([comm, local_rew, local_obs, G.SEED, NSEEDS, EPISODES, L], dtype=np.int64)
    return out


def save_npz(path, arrays):
    """np.savez_compressed with the archive's timestamps pinned, so that the file regenerates byte for byte."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[name]), allow_pickle=False)


def main():
    W = G.import_reference()
    from social_dilemmas.envs import watershedLogging as cb
    os.makedirs(OUT, exist_ok=True)
    for comm, lr, lo in CASES:
        rec = record(W, cb, comm, lr, lo)
        save_npz(os.path.join(OUT, name_of(comm, lr, lo)), rec)
        print(name_of(comm, lr, lo), "Equality", rec["Equality"].min(), rec["Equality"].max(), "violations", rec["violations"].mean())


if __name__ == "__main__":
    main()
