"""Batched adapter for rollouts: E envs stepped by one kernel launch, per-env
episode horizon with automatic reset, observations left on the GPU.

This is what removes the Python-dict bottleneck of running E `MapEnv` objects: RLlib's `horizon: 1000`
lives in the launcher, not in the env (run_scripts/train_baseline.py:131, train_moa.py:122), so here the
kernel reports `done = (t >= horizon)` and the adapter resets exactly those envs with a masked reset --
the returned observation row of a finished env is the first observation of its next episode (the usual
vector-env auto-reset convention).

Two surfaces:
  * tensors: `reset()` / `step(actions)` -> torch tensors on the engine's device;
  * RLlib `BaseEnv`-style `poll()` / `send_actions()` / `try_reset()` with {env_id: {agent_id: ...}} dicts,
    for code written against that interface (a host round trip per call: use it for compatibility,
    not for speed).

track_episodes=True keeps per-episode statistics on the device (episode_stats.py): the steps write rew / done into the
slots of a ring, which is folded when it fills, before a reset, and whenever the statistics are read.
"""
import numpy as np

from . import constants as K
from .engine import VecEngine

_NORMALISE = (np.arange(256, dtype=np.float64) - 128.0) / 255.0


class SSDVectorEnv(object):
    def __init__(self, game, num_envs, num_agents, horizon=1000, ascii_map=None, seed=0, device=0,
                 env_index_base=0, view_len=K.VIEW_LEN, float32_obs=False, return_agent_actions=False, track_episodes=False,
                 track_ring=64):
        self.engine = VecEngine(game, ascii_map, num_envs=num_envs, num_agents=num_agents, seed=seed, device=device,
                                env_index_base=env_index_base, view_len=view_len)
        self.num_envs, self.num_agents, self.horizon = num_envs, num_agents, int(horizon)
        self.float32_obs = bool(float32_obs)     # the kernel writes float32((u8 - 128) / 255) NHWC directly
        self.engine.set_horizon(self.horizon)
        self.agent_ids = ['agent-%d' % i for i in range(num_agents)]
        # return_agent_actions=True (the MOA trainers' envs, run_scripts/train_moa.py:70): observations become a dict
        # {"curr_obs", "other_agent_actions" int64 [E,N,N-1], "visible_agents" int64 [E,N,N-1]} of device tensors -- the
        # reference's per-agent observation dict (map_env.py:201-205, :242-246) batched (engine.agent_action_obs)
        self.return_agent_actions = bool(return_agent_actions)
        self._out = None
        self._extras = None
        self._act_buf = None
        self._pending = None
        # what sample() carries across calls, per kind of policy (its C_ROLLOUT): {"state": [E,N,rows,C]} and, for the MOA policy,
        # "prev_actions" [E,N], the previous joint action
        self._carried = {}
        # track_episodes: step k writes rew / done into slot k % track_ring of a ring that the episode statistics fold
        self.stats = None
        if track_episodes:
            from .episode_stats import EpisodeStats
            if int(track_ring) < 1:
                raise ValueError("track_ring must be >= 1")
            self.stats = EpisodeStats(num_envs, num_agents, device=device)
            self._ring_len = int(track_ring)
            self._ring = self._slot_outs = None
            self._slot = self._fold_from = self._unfolded = 0

    # ------------------------------------------------------------------ tensor API
    def _wrap(self, obs, actions, done):
        if not self.return_agent_actions:
            return obs
        self._extras = self.engine.agent_action_obs(actions, done, out=self._extras)
        return {"curr_obs": obs, "other_agent_actions": self._extras[0], "visible_agents": self._extras[1]}

    def _alloc(self):
        self._out = self.engine.alloc_outputs(float32=self.float32_obs)
        if self.stats is not None:
            import torch
            dev = self._out[1].device
            shape = (self._ring_len, self.num_envs, self.num_agents)
            self._ring = (torch.zeros(shape, dtype=torch.int32, device=dev), torch.zeros(shape, dtype=torch.uint8, device=dev))
            self._slot_outs = [(self._out[0], self._ring[0][s], self._ring[1][s]) for s in range(self._ring_len)]
            self.engine.register_outputs(self._slot_outs)
            self._slot = self._fold_from = self._unfolded = 0
            self._out = self._slot_outs[0]

    def _fold(self):
        """Fold the ring's steps not yet folded (in slot order, episodes ending at done)."""
        if self.stats is not None and self._unfolded:
            self.stats.fold(self._ring[0], self._ring[1], step0=self._fold_from, n_steps=self._unfolded)
            self._fold_from, self._unfolded = self._slot, 0

    def _advance(self):
        """After a step that wrote slot self._slot: the next step writes the next slot; a full ring is folded first."""
        if self.stats is None or self._ring is None:
            return
        self._unfolded += 1
        self._slot = (self._slot + 1) % self._ring_len
        if self._unfolded == self._ring_len:
            self._fold()
        self._out = self._slot_outs[self._slot]

    def episode_stats(self):
        """The EpisodeStats of this batch (track_episodes=True), every step so far folded into it."""
        if self.stats is None:
            raise RuntimeError("construct with track_episodes=True")
        self._fold()
        return self.stats

    def summary(self):
        """episode_stats().summary(): RLlib-style means of the episodes that ended since the last read, and clears them."""
        return self.episode_stats().summary()

    def reset(self):
        if self.stats is not None and self._ring is not None:
            self._fold()
            self.stats.discard()                 # the episodes still open are cut short
        self._alloc()
        self._carried = {}
        self.engine.reset(obs=self._out[0])
        return self._wrap(self._out[0], None, None)

    # Auto-reset, three ways.  (1) While every env was last reset by the same call (the engine keeps count) they all reach the
    # horizon on the same step and the host knows which one: nothing to launch until then, a full reset then.  (2) Otherwise
    # the step launch itself resets the envs that finish (SSD_AUTO_RESET).  (3) float32 observations, which that kernel does
    # not write: a masked reset launch after every step (a masked reset only touches envs whose flag is set, so no host
    # synchronisation is needed to decide whether anything finished).
    def _in_kernel(self):
        return (self.horizon > 0 and self.num_agents > 0 and self.engine.steps_since_full_reset is None
                and not self.float32_obs)

    def _auto_reset(self, obs, done, in_kernel):
        if self.horizon <= 0 or not self.num_agents or in_kernel:
            return
        since = self.engine.steps_since_full_reset
        if since is not None:
            if since >= self.horizon:
                self.engine.reset(obs=obs)           # everybody just finished: a full reset, no mask needed
            return
        self.engine.reset(mask=done[:, 0].contiguous(), obs=obs)

    def step(self, actions, order=None):
        """actions: int32 [E,N] on the device (-1: the agent sent no action); order: optional uint8 [E,N] on the device, per env
        the agent indices in action-dict order, 0xFF-terminated (None: index order).  Returns (obs u8, rew i32, done u8) device
        tensors; envs whose episode just ended have been reset and their obs rows replaced by the new episode's first observation."""
        in_kernel = self._in_kernel()
        obs, rew, done = self.engine.step(actions, order=order, out=self._out, auto_reset=in_kernel)
        self._auto_reset(obs, done, in_kernel)
        self._advance()
        # (rows of envs whose episode just ended carry a reset's observation: their other_agent_actions are the reset's zeros)
        return self._wrap(obs, actions, done if self.horizon > 0 else None), rew, done

    def step_random(self):
        in_kernel = self._in_kernel()
        if self.return_agent_actions and self._act_buf is None:
            import torch
            self._act_buf = torch.empty((self.num_envs, self.num_agents), dtype=torch.int32, device=self._out[1].device)
        obs, rew, done = self.engine.step_random(out=self._out, actions_out=self._act_buf, auto_reset=in_kernel)
        self._auto_reset(obs, done, in_kernel)
        self._advance()
        return self._wrap(obs, self._act_buf, done if self.horizon > 0 else None), rew, done

    def sample(self, policy, n_steps, greedy=False, state_every=None, influence_weight=1.0, gamma=None, lambda_=1.0, use_gae=True,
               use_critic=True, standardize=False):
        """n_steps closed-loop steps of a ConvFCPolicy or a ConvLSTMPolicy on the device in one call (VecEngine.rollout_policy): returns a dict of
        device tensors obs u8 [K,E,N,15,15,3], actions i32, logp f32, value f32, rew i32, done u8 (all [K,E,N], step k in row
        k) and last_value f32 [E,N] (the value of the final observation).  Episodes end at the horizon as in step(): a finished
        env's obs row is its next episode's first.  Afterwards the adapter is where n_steps calls of step() with the sampled
        actions would have left it; track_episodes keeps counting.  With n_steps > 1, num_envs * num_agents must be a multiple
        of 4.  Not for float32_obs or return_agent_actions adapters.
        A ConvLSTMPolicy's state [E,N,2,C] is kept by the adapter across calls (zero after reset(), and at every episode start)
        and the dict gains "state_in" f32 [E,N,2,C], the state step 0 used; with state_every, "state" f32 [S,E,N,2,C] too, the
        state of steps 0, state_every, 2 state_every, ... (S = ceil(n_steps / state_every)).  A policy of another cell size than
        the state held raises until reset().
        A ConvMOAPolicy's state [E,N,4,C] and previous joint action [E,N] are kept the same way (both zero after reset() and
        at every episode start), and the dict gains "state_in", "state" (with state_every), "influence" f32 [K,E,N],
        "prev_actions" i32 [K,E,N] (what each step's MOA read) and "rewards" f32 [K,E,N] = rew + influence_weight *
        influence.
        With a gamma the dict gains "advantages" and "value_targets" f32 [K,E,N]: postprocessing.compute_advantages of rew,
        value, done and last_value (for a ConvMOAPolicy of rew + influence_weight * influence, formed in float64), enqueued
        behind the rollout on the same stream.  With standardize=True (it needs a gamma) "advantages" is standardised per weight
        set of the policy, postprocessing.standardize_advantages with num_sets = policy.num_sets, in place behind the
        advantages' launch: what RLlib's PPO optimizers do to a train batch before the SGD epochs.  "value_targets" is
        untouched."""
        import torch
        if self.float32_obs:
            raise ValueError("sample() records uint8 observations: construct with float32_obs=False")
        if self.return_agent_actions:
            raise ValueError("sample() does not build the agent-action observation extras: construct with return_agent_actions=False")
        n_steps = int(n_steps)
        if n_steps < 1:
            raise ValueError("n_steps must be >= 1")
        eng = self.engine
        eng._policy_weights(policy)                  # (every check before anything is enqueued)
        if standardize and gamma is None:
            raise ValueError("standardize=True standardises the advantages: give a gamma")
        if gamma is not None:
            import math
            gamma, lambda_ = float(gamma), float(lambda_)
            if not (math.isfinite(gamma) and math.isfinite(lambda_)):
                raise ValueError("gamma and lambda_ must be finite")
            if use_gae and not use_critic:
                raise ValueError("use_gae needs use_critic: generalised advantage estimation uses the value function")
        rows, moa = policy.STATE_ROWS, policy.TAKES_PREV_ACTIONS
        if not rows and state_every is not None:
            raise ValueError("state_every belongs to a ConvLSTMPolicy")
        if rows:
            held = self._carried.get(policy.C_ROLLOUT)       # what this kind of policy left here: its state (and previous actions)
            if held is not None and held["state"].shape[-1] != policy.cell_size:
                raise ValueError("the adapter holds the state of a %d-cell policy, this one has %d cells: reset() first"
                                 % (held["state"].shape[-1], policy.cell_size))
            every = n_steps if state_every is None else int(state_every)
            if every < 1:
                raise ValueError("state_every must be >= 1")
        E, N, V = self.num_envs, self.num_agents, eng.V
        if n_steps > 1 and (E * N) % 4:
            raise ValueError("an observation ring of more than one slot needs num_envs * num_agents to be a multiple of 4")
        if self._out is None:
            self.reset()                             # (an adapter that never sampled: nothing is carried, held is None)
        dev = self._out[1].device
        out = {"obs": torch.empty((n_steps, E, N, V, V, 3), dtype=torch.uint8, device=dev),
               "actions": torch.empty((n_steps, E, N), dtype=torch.int32, device=dev),
               "logp": torch.empty((n_steps, E, N), dtype=torch.float32, device=dev),
               "value": torch.empty((n_steps, E, N), dtype=torch.float32, device=dev),
               "rew": torch.empty((n_steps, E, N), dtype=torch.int32, device=dev),
               "done": torch.empty((n_steps, E, N), dtype=torch.uint8, device=dev),
               "last_value": torch.empty((E, N), dtype=torch.float32, device=dev)}
        kw = {}
        if rows:
            if held is None:
                held = self._carried[policy.C_ROLLOUT] = {"state": torch.zeros((E, N, rows, policy.cell_size), dtype=torch.float32, device=dev)}
                if moa:
                    held["prev_actions"] = torch.zeros((E, N), dtype=torch.int32, device=dev)
            ring = torch.empty((-(-n_steps // every), E, N, rows, policy.cell_size), dtype=torch.float32, device=dev)
            if moa:
                out["influence"] = torch.empty((n_steps, E, N), dtype=torch.float32, device=dev)
                out["prev_actions"] = torch.empty((n_steps, E, N), dtype=torch.int32, device=dev)
                kw = dict(prev_actions_ring=out["prev_actions"], influence=out["influence"])
            kw.update(held, state_ring=ring, state_every=every)
            out["state_in"] = ring[0]
            if state_every is not None:
                out["state"] = ring
        self._fold()                                 # the adapter's own ring first: episodes are folded in step order
        eng.rollout_policy(policy, self._out[0], n_steps, out["obs"], actions=out["actions"], logp=out["logp"], value=out["value"],
                           rew=out["rew"], done=out["done"], last_value=out["last_value"], greedy=greedy, stats=self.stats, **kw)
        self._out[0].copy_(out["obs"][n_steps - 1])  # the current observation, as step() would have left it
        if moa:
            out["rewards"] = out["rew"].to(torch.float32) + float(influence_weight) * out["influence"]
        if gamma is not None:
            from .postprocessing import compute_advantages
            bonus = dict(bonus=out["influence"], bonus_weight=float(influence_weight)) if moa else {}
            out["advantages"], out["value_targets"] = compute_advantages(
                out["rew"], out["value"], out["last_value"], out["done"], gamma=gamma, lambda_=lambda_, use_gae=use_gae,
                use_critic=use_critic, **bonus)
            if standardize:
                from .postprocessing import standardize_advantages
                standardize_advantages(out["advantages"], num_sets=policy.num_sets, out=out["advantages"])
        return out

    @staticmethod
    def to_float(obs):
        """uint8 [E,N,V,V,3] -> float32 NHWC batch [(E*N),V,V,3] with the reference's scaling
        ((x - 128) / 255, map_env.py:199), on the device: the input the first conv layer of
        models/conv_to_fcnet_v2.py:33-56 expects.  With float32_obs=True the step
        kernel writes this directly and no conversion pass is needed."""
        import torch
        E, N, V = obs.shape[0], obs.shape[1], obs.shape[2]
        return ((obs.to(torch.float32) - 128.0) / 255.0).reshape(E * N, V, V, 3)

    # ------------------------------------------------------------------ BaseEnv-style API
    def poll(self):
        """-> (obs, rewards, dones, infos, off_policy_actions) as {env_id: {agent_id: value}} dicts."""
        if self.float32_obs:
            raise RuntimeError("the dict surface renormalises uint8 observations: construct with float32_obs=False")
        if self._pending is None:
            obs = self.reset()
            rew = np.zeros((self.num_envs, self.num_agents), np.int32)
            done = np.zeros((self.num_envs, self.num_agents), np.uint8)
        else:
            obs, rew, done = self._pending
            rew, done = rew.cpu().numpy(), done.cpu().numpy()
        oaa = vis = None
        if self.return_agent_actions:
            oaa, vis = obs["other_agent_actions"].cpu().numpy(), obs["visible_agents"].cpu().numpy()
            obs = obs["curr_obs"]
        obs = obs.cpu().numpy()
        o, r, d, i = {}, {}, {}, {}
        for e in range(self.num_envs):
            if self.return_agent_actions:
                # (an agent that sent no action is absent from the reference's array: drop its -1)
                o[e] = {a: {"curr_obs": _NORMALISE[obs[e, k]], "other_agent_actions": oaa[e, k][oaa[e, k] >= 0],
                            "visible_agents": vis[e, k]} for k, a in enumerate(self.agent_ids)}
            else:
                o[e] = {a: _NORMALISE[obs[e, k]] for k, a in enumerate(self.agent_ids)}
            r[e] = {a: int(rew[e, k]) for k, a in enumerate(self.agent_ids)}
            d[e] = {a: bool(done[e, k]) for k, a in enumerate(self.agent_ids)}
            d[e]["__all__"] = bool(done[e].any()) if self.num_agents else False
            i[e] = {}
        return o, r, d, i, {}

    def send_actions(self, action_dict):
        """{env_id: {agent_id: action}}.  The reference's step depends on the iteration order of the inner dicts (who is
        shuffled where in update_moves, whose beam lands first: map_env.py:171,379,546), so the order of every env's dict goes to
        the kernel with the actions, as MapEnv.step passes its own (map_env.py of this package); envs whose dicts are in
        index order -- what RLlib's sampler sends -- need none, and a batch of only such envs takes the map-specific kernels."""
        import torch
        N = self.num_agents
        act = np.full((self.num_envs, N), K.NO_ACTION, np.int32)
        order = np.full((self.num_envs, N), 0xFF, np.uint8)
        index_of = {a: k for k, a in enumerate(self.agent_ids)}
        explicit = False
        for e, per_agent in action_dict.items():
            last = -1
            for k, (a, v) in enumerate(per_agent.items()):
                i = index_of[a]                                  # KeyError for an unknown agent, as in the reference
                act[e, i] = int(v)
                order[e, k] = i
                explicit = explicit or i < last
                last = i
        dev = torch.device("cuda", self.engine.device)
        if explicit:
            # (envs that sent nothing keep an empty order: nobody acts there, which is what their all -1 action rows say too)
            self._pending = self.step(torch.from_numpy(act).to(dev), torch.from_numpy(order).to(dev))
        else:
            self._pending = self.step(torch.from_numpy(act).to(dev))

    def try_reset(self, env_id):
        import torch
        mask = torch.zeros(self.num_envs, dtype=torch.uint8, device=torch.device("cuda", self.engine.device))
        mask[env_id] = 1
        if self._out is None:
            self._alloc()
        elif self.stats is not None:
            self._fold()
            self.stats.discard(mask)             # the env's open episode is cut short
        self.engine.reset(mask=mask, obs=self._out[0])
        if self.return_agent_actions:
            n1 = max(self.num_agents - 1, 0)
            return {a: {"curr_obs": _NORMALISE[self._out[0][env_id, k].cpu().numpy()], "other_agent_actions": np.zeros(n1, np.int64),
                        "visible_agents": np.ones(n1, np.int64)} for k, a in enumerate(self.agent_ids)}
        return {a: _NORMALISE[self._out[0][env_id, k].cpu().numpy()] for k, a in enumerate(self.agent_ids)}
