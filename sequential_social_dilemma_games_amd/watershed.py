"""The Watershed games on the MI355X engine (reference: social_dilemmas/envs/watershedOrderedComm.py:284-637).

    WatershedVecEngine      E envs as batched device tensors (include/ssd.h, ssd_ws_*; csrc/ssd_watershed.hip)
    WatershedSeqEnv         dict drop-in for the reference class of the same name (:284-423)
    WatershedSeqCommEnv     dict drop-in for :425-637

Each step has exactly one acting agent.  WatershedSeqEnv: agents 0-3 take turns, an episode is 43
steps.  WatershedSeqCommEnv: comm agents 0-3 act twice (Discrete(5) messages), then action agents
4-7 act (Box(0, 1, (1,)) withdrawal fractions), an episode is 131 steps.  Rewards, violations and
the episode sums change when a round closes; the arithmetic is the reference's float32 (float64 for
the episode sums and the end-of-episode rewards), squares included (libm powf, not x*x).

The season (np.random.choice(range(108)) at :69) comes from the engine's counter PRNG
(prng.S_SEASON), keyed on (seed, env index, episode).  The reference's other global draws only
gate debug prints and have no counterpart.
"""
import ctypes as C

import numpy as np

from . import _capi
from .map_env import Box, Dict, Discrete, MultiAgentEnv

SEQ, SEQ_COMM = _capi.SSD_WS_SEQ, _capi.SSD_WS_SEQ_COMM
OBS_WIDTH = _capi.SSD_WS_OBS_WIDTH
EPISODE_STEPS = {SEQ: 43, SEQ_COMM: 131}


def obs_len(variant, local_obs, agent):
    """Length of the reference's curr_obs for `agent` (the rest of an engine row is zero padding)."""
    base = 4 if local_obs else 7
    if variant == SEQ:
        return base + 1
    return base + 4 if agent < 4 else base + 5


def obs_dtype_is_float(variant, agent):
    """The reference builds curr_obs with np.array(list): float64 when the list holds the agent's float32 flow (agents 1 and 3 of
    the action agents: Q1 * (1 - a) and the confluence), int64 otherwise (Q1 and Q2 are Python ints, comm actions integers)."""
    k = agent if variant == SEQ else agent - 4
    return k in (1, 3)


def _stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class WatershedVecEngine(object):
    """E Watershed envs resident on one device.  Device-tensor API (torch, asynchronous on torch's current stream):

        obs, agent = eng.reset(mask=None)                  obs f32 [E,12], agent i8 [E]
        obs, agent, rew, done = eng.step(actions)           actions f32 [E]; rew f64 [E]; done u8 [E] (SSD_WS_* bits)
        eng.rollout_actions(actions [R,E], n_steps, obs [ring,E,12], agent, rew, done)   n_steps phases in one launch
        eng.info()                                          viol, true_end, running_rew, temp, other_agent_actions
        eng.sample(policy, n_steps)                         a closed-loop rollout with a WatershedLSTMPolicy (policy.py) on the device
        eng.attach_stats(stats)                             episode statistics folded by the stepping kernel (watershed_stats.py)
    """

    def __init__(self, variant=SEQ, num_envs=1, seed=0, local_obs=False, local_rew=False, env_index_base=0, device=0):
        import torch
        self.variant, self.E, self.seed = int(variant), int(num_envs), int(seed)
        self.local_obs, self.local_rew, self.env_index_base, self.device = bool(local_obs), bool(local_rew), int(env_index_base), int(device)
        self.P = 4 if self.variant == SEQ else 12
        self.episode_steps = EPISODE_STEPS.get(self.variant)
        c = _capi.WsConfig()
        c.struct_size = C.sizeof(_capi.WsConfig)
        c.variant, c.num_envs, c.local_obs, c.local_rew = self.variant, self.E, int(self.local_obs), int(self.local_rew)
        c.device_id, c.seed, c.env_index_base = self.device, self.seed, self.env_index_base
        self._L = _capi.lib()
        self._h = C.c_void_p()
        _capi.ws_check(self._L.ssd_ws_create(C.byref(c), C.byref(self._h)))
        self._dev = torch.device("cuda", self.device)
        self._last_obs = self._last_agent = None                 # the current observation and its agent, for sample()
        self._pol_scratch = self._pol_key = self._pol_state = None   # rollout_policy's action scratch; sample()'s policy state
        self._stats = None                                       # the attached WatershedEpisodeStats (attach_stats)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.ssd_ws_destroy(self._h)                      # lets go of an attached statistics handle
            self._h = None
            self._stats = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def attach_stats(self, stats):
        """Fold every later step() / rollout_actions() / rollout_policy() / sample() into `stats` (a WatershedEpisodeStats of this
        engine's variant, env count and device; None detaches), inside the stepping kernel.  An episode is counted from a reset()
        (or an auto-reset) made while the handle is attached: attach before the reset that starts the first one.  Whatever the
        handle had open is discarded here (on torch's current stream), since the envs may have moved on meanwhile; reset(mask)
        discards the open episodes of the envs it resets.  Observations, rewards, dones and the state do not change."""
        from .watershed_stats import WatershedEpisodeStats
        if stats is not None and not isinstance(stats, WatershedEpisodeStats):
            raise ValueError("stats must be a WatershedEpisodeStats or None")
        self._check(self._L.ssd_ws_stats_attach(self._h, None if stats is None else stats._h))
        self._stats = stats                                      # keeps the handle alive while the engine holds it
        if stats is not None:
            stats.discard()

    def _outputs(self, lead=()):
        import torch
        E, d = self.E, self._dev
        return (torch.empty(lead + (E, OBS_WIDTH), dtype=torch.float32, device=d), torch.empty(lead + (E,), dtype=torch.int8, device=d),
                torch.empty(lead + (E,), dtype=torch.float64, device=d), torch.empty(lead + (E,), dtype=torch.uint8, device=d))

    def _actions(self, actions):
        import torch
        return torch.as_tensor(actions, dtype=torch.float32, device=self._dev).contiguous()

    def _check(self, rc):
        _capi.ws_check(rc, self._h)

    def _check_tensor(self, t, shape, dtype, name):
        """Every buffer handed to a kernel: on this handle's device, of the kernel's dtype and exact shape, contiguous, and aligned
        (the observation rows are written as 16-byte stores)."""
        if (t.device != self._dev or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous()
                or t.data_ptr() % (16 if name == "obs" else t.element_size())):
            raise ValueError("%s must be a contiguous, aligned %s tensor of shape %s on %s (got %s %s %s)"
                             % (name, dtype, tuple(shape), self._dev, t.dtype, tuple(t.shape), t.device))

    def _check_outputs(self, lead, obs, agent, rew, done):
        import torch
        E = self.E
        for t, shape, dtype, name in ((obs, lead + (E, OBS_WIDTH), torch.float32, "obs"), (agent, lead + (E,), torch.int8, "agent"),
                                      (rew, lead + (E,), torch.float64, "rew"), (done, lead + (E,), torch.uint8, "done")):
            if t is not None:
                self._check_tensor(t, shape, dtype, name)

    def reset(self, mask=None):
        """reset() on the envs selected by `mask` (bool / u8 [E]; None = all).  Rows of the other envs are zero."""
        import torch
        obs, agent, _, _ = self._outputs()
        obs.zero_()
        agent.zero_()
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self._dev).to(torch.uint8).contiguous()
            self._check_tensor(m, (self.E,), torch.uint8, "mask")
        self._check(self._L.ssd_ws_reset(self._h, _p(m), _p(obs), _p(agent), _stream(self._dev)))
        if mask is None:
            self._last_obs, self._last_agent = obs, agent        # where sample() starts
        elif self._last_obs is not None:                         # the reset rows replace those of the kept observation
            self._last_obs = torch.where(m.bool()[:, None], obs, self._last_obs)
            self._last_agent = torch.where(m.bool(), agent, self._last_agent)
        return obs, agent

    def step(self, actions, auto_reset=False, out=None):
        """One phase of every env: actions f32 [E] (the acting agent's).  -> obs, agent, rew, done."""
        import torch
        a = self._actions(actions)
        self._check_tensor(a, (self.E,), torch.float32, "actions")
        obs, agent, rew, done = out if out is not None else self._outputs()
        self._check_outputs((), obs, agent, rew, done)
        flags = _capi.SSD_AUTO_RESET if auto_reset else 0
        self._check(self._L.ssd_ws_step(self._h, _p(a), _p(obs), _p(agent), _p(rew), _p(done), flags, _stream(self._dev)))
        self._last_obs, self._last_agent = obs, agent
        return obs, agent, rew, done

    def rollout_actions(self, actions, n_steps, obs=None, agent=None, rew=None, done=None, step0=0, auto_reset=False):
        """n_steps phases in ONE launch: step k reads actions[(step0 + k) % R] (f32 [R,E]) and writes ring slot (step0 + k) % ring
        of each output given ([ring,E,12] / [ring,E]; None = not written)."""
        import torch
        a = self._actions(actions)
        if a.dim() != 2 or a.shape[0] < 1:
            raise ValueError("actions must be f32 [R, E] with R >= 1")
        self._check_tensor(a, (a.shape[0], self.E), torch.float32, "actions")
        rings = [t.shape[0] if t.dim() else 0 for t in (obs, agent, rew, done) if t is not None]
        ring = rings[0] if rings else 1
        if ring < 1:
            raise ValueError("outputs need a leading ring dimension >= 1")
        self._check_outputs((ring,), obs, agent, rew, done)
        if int(n_steps) < 0 or int(step0) < 0:
            raise ValueError("n_steps and step0 must be >= 0")
        flags = _capi.SSD_AUTO_RESET if auto_reset else 0
        self._check(self._L.ssd_ws_rollout_actions(self._h, _p(a), a.shape[0], int(n_steps), int(step0), _p(obs), _p(agent), _p(rew),
                                                   _p(done), ring, flags, _stream(self._dev)))
        if int(n_steps) > 0:
            last = (int(step0) + int(n_steps) - 1) % ring
            self._last_obs, self._last_agent = (obs[last], agent[last]) if obs is not None and agent is not None else (None, None)

    # ---------------------------------------------------------------- policy rollouts (include/ssd.h, WATERSHED POLICY ROLLOUTS)
    # (the network's state rows and the library's entry points are the policy's class attributes, policy.PolicyBase)
    def _check_policy(self, policy):
        from .policy import WatershedLSTMPolicy
        if not isinstance(policy, WatershedLSTMPolicy):
            raise ValueError("policy must be a WatershedLSTMPolicy")
        if policy.variant != self.variant:
            raise ValueError("the policy is of variant %d, the engine of variant %d" % (policy.variant, self.variant))
        w = policy.packed()
        if w.device != self._dev:
            raise ValueError("the policy's parameters must be on %s" % (self._dev,))
        return w

    def policy_forward(self, policy, obs, agent, state, starts=None):
        """The policy's forward pass on the device: obs f32 [B,12], agent i8 [B] (the acting agent of each row), state f32
        [B,2,C] (each row's own), starts u8 / bool [B] or None -> (dist f32 [B,5], value f32 [B], new state f32 [B,2,C])."""
        import torch
        w = self._check_policy(policy)
        B, Cc = int(agent.shape[0]) if agent.dim() == 1 else -1, policy.cell_size
        if B < 1:
            raise ValueError("agent must be i8 [B] with B >= 1")
        self._check_tensor(obs, (B, OBS_WIDTH), torch.float32, "policy obs")
        self._check_tensor(agent, (B,), torch.int8, "agent")
        self._check_tensor(state, (B, policy.STATE_ROWS, Cc), torch.float32, "state")
        s = None
        if starts is not None:
            s = torch.as_tensor(starts, device=self._dev).to(torch.uint8).contiguous()
            self._check_tensor(s, (B,), torch.uint8, "starts")
        dist = torch.empty((B, 5), dtype=torch.float32, device=self._dev)
        value = torch.empty((B,), dtype=torch.float32, device=self._dev)
        out = torch.empty_like(state)
        _capi.policy_check(getattr(self._L, policy.C_FORWARD)(_p(w), policy.num_sets, Cc, self.variant, _p(obs), _p(agent), _p(state), _p(s),
                                                              B, _p(out), _p(dist), _p(value), self.device, 0, _stream(self._dev)))
        return dist, value, out

    def rollout_policy(self, policy, obs_in, agent_in, n_steps, obs, agent, rew=None, done=None, actor=None, actions=None, logp=None,
                       value=None, dist=None, state=None, state_ring=None, last_value=None, step0=0, greedy=False):
        """n_steps phases of the closed loop in one call (no host round trip): step k runs the policy on the current observation
        (obs_in f32 [E,12] / agent_in i8 [E] for k = 0, then the previous ring slot), advances row [e, agent] of state f32
        [E,num_sets,2,C] in place, writes actor i8, actions f32 (unclipped), logp f32, value f32 ([ring,E]), dist f32 [ring,E,5]
        and state_ring f32 [ring,E,2,C] (the state it used) into ring slot (step0 + k) % ring, then steps the env (auto-reset)
        with the clipped action into obs / agent / rew / done of the same slot.  obs, agent, actions and state are required;
        last_value f32 [E] receives the value of the final observation."""
        import torch
        w = self._check_policy(policy)
        E, Cc = self.E, policy.cell_size
        if obs is None or agent is None or actions is None or state is None:
            raise ValueError("obs, agent, actions and state are required")
        ring = int(obs.shape[0]) if obs.dim() == 3 else 0
        if ring < 1:
            raise ValueError("obs must be f32 [ring, E, 12] with ring >= 1")
        if int(n_steps) < 1 or int(step0) < 0:
            raise ValueError("n_steps must be >= 1 and step0 >= 0")
        self._check_tensor(obs_in, (E, OBS_WIDTH), torch.float32, "obs")
        self._check_tensor(agent_in, (E,), torch.int8, "agent_in")
        self._check_outputs((ring,), obs, agent, rew, done)
        SR = policy.STATE_ROWS
        self._check_tensor(state, (E, policy.num_sets, SR, Cc), torch.float32, "state")
        for t, shape, dtype, name in ((actor, (ring, E), torch.int8, "actor"), (actions, (ring, E), torch.float32, "actions"),
                                      (logp, (ring, E), torch.float32, "logp"), (value, (ring, E), torch.float32, "value"),
                                      (dist, (ring, E, 5), torch.float32, "dist"), (state_ring, (ring, E, SR, Cc), torch.float32, "state_ring"),
                                      (last_value, (E,), torch.float32, "last_value")):
            if t is not None:
                self._check_tensor(t, shape, dtype, name)
        if self._pol_scratch is None:
            self._pol_scratch = torch.zeros((E,), dtype=torch.float32, device=self._dev)
        flags = _capi.SSD_POLICY_GREEDY if greedy else 0
        self._check(getattr(self._L, policy.C_ROLLOUT)(self._h, _p(w), policy.num_sets, Cc, _p(obs_in), _p(agent_in), int(n_steps), int(step0),
                                                       _p(state), _p(state_ring), _p(self._pol_scratch), _p(obs), _p(agent), _p(rew), _p(done),
                                                       _p(actor), _p(actions), _p(logp), _p(value), _p(dist), ring, _p(last_value), flags,
                                                       _stream(self._dev)))
        last = (int(step0) + int(n_steps) - 1) % ring
        self._last_obs, self._last_agent = obs[last], agent[last]

    def sample(self, policy, n_steps, greedy=False):
        """A closed-loop rollout of n_steps phases from where the last sample() (or reset()) left the envs.  Keeps the last
        observation, its agent and the policy state between calls (it zeroes nothing itself: the start rule does), so two calls
        give what one call of twice the length gives.  Returns a dict of device tensors [K,E,...]: obs, agent (after each step),
        actor, actions, logp, value, dist, rew, done, and state_in [K,E,2,C] (the state each step used), last_value [E]."""
        import torch
        K, E, d = int(n_steps), self.E, self._dev
        key = (id(policy), policy.cell_size)
        if self._pol_key != key:
            self._pol_key = key
            self._pol_state = policy.initial_state((E, policy.num_sets), device=d).to(torch.float32)
        if self._last_obs is None:
            raise RuntimeError("sample() needs the current observation: call reset() (or step()) first")
        obs, agent, rew, done = self._outputs((K,))
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=d)   # noqa: E731
        out = dict(obs=obs, agent=agent, rew=rew, done=done, actor=torch.empty((K, E), dtype=torch.int8, device=d), actions=f(K, E),
                   logp=f(K, E), value=f(K, E), dist=f(K, E, 5), state_in=f(K, E, policy.STATE_ROWS, policy.cell_size), last_value=f(E))
        self.rollout_policy(policy, self._last_obs, self._last_agent, K, obs, agent, rew=rew, done=done, actor=out["actor"],
                            actions=out["actions"], logp=out["logp"], value=out["value"], dist=out["dist"], state=self._pol_state,
                            state_ring=out["state_in"], last_value=out["last_value"], greedy=greedy)
        return out

    def info(self):
        """The info fields of the current state, as device tensors."""
        import torch
        E, d = self.E, self._dev
        out = dict(viol=torch.empty((E, 6), dtype=torch.uint8, device=d), true_end=torch.empty((E,), dtype=torch.uint8, device=d),
                   running_rew=torch.empty((E, 4), dtype=torch.float64, device=d), temp=torch.empty((E,), dtype=torch.float64, device=d),
                   other_agent_actions=torch.empty((E, 3), dtype=torch.int64, device=d))
        self._check(self._L.ssd_ws_info(self._h, _p(out["viol"]), _p(out["true_end"]), _p(out["running_rew"]), _p(out["temp"]),
                                        _p(out["other_agent_actions"]), _stream(self._dev)))
        return out

    _STATE = (("season", np.uint8, ()), ("phase", np.uint8, ()), ("wrapped", np.uint8, ()), ("viol", np.uint8, (6,)),
              ("round", np.int32, ()), ("episode", np.uint32, ()), ("hist", np.float32, (8,)), ("f_rew", np.float32, (6,)),
              ("pen", np.float32, ()), ("current_sums", np.float64, (4,)), ("running_rew", np.float64, (4,)),
              ("prev_actions", np.float32, (4,)))

    def get_state(self):
        """Host copy of the state (synchronous): dict of numpy arrays, rows = envs (include/ssd.h, ssd_ws_state)."""
        arrs = {k: np.zeros((self.E,) + shp, dt) for k, dt, shp in self._STATE}
        st = _capi.WsState(**{k: arrs[k].ctypes.data for k in arrs})
        self._check(self._L.ssd_ws_get_state(self._h, C.byref(st)))
        return arrs

    def set_state(self, state):
        arrs = {k: np.ascontiguousarray(np.asarray(state[k], dt).reshape((self.E,) + shp)) for k, dt, shp in self._STATE}
        st = _capi.WsState(**{k: arrs[k].ctypes.data for k in arrs})
        self._check(self._L.ssd_ws_set_state(self._h, C.byref(st)))

    def status(self, clear=True):
        s = C.c_uint32()
        self._check(self._L.ssd_ws_device_status(self._h, C.byref(s), int(clear)))
        return s.value


class WatershedSeqEnv(MultiAgentEnv):
    """Drop-in for the reference's WatershedSeqEnv: the same obs / rew / done / info dicts, keys, values, Python and NumPy types
    and dtypes, including the in-place rewrite of the caller's action dict (:338-340).  The action dict holds the acting agent's
    action only (what RLlib sends: the agent that was given an observation), a float32 array of shape (1,).

    seed / env_index: coordinates of the season draw (the episode counter is the third)."""
    VARIANT = SEQ

    def __init__(self, return_agent_actions=False, local_rew=False, local_obs=False, seed=0, env_index=0, device=0):
        self.return_agent_actions, self.local_rew, self.local_obs = return_agent_actions, local_rew, local_obs
        self.comm_agents = 4
        self.num_agents = 4 if self.VARIANT == SEQ else 8
        self.max_steps = 10
        self.mybigreq = [24 * 10, 40 * 10, 24 * 10, 10 * 10]
        self._eng = WatershedVecEngine(self.VARIANT, 1, seed=seed, local_obs=local_obs, local_rew=local_rew, env_index_base=env_index,
                                       device=device)
        self._spaces()
        self._acting = None

    def _spaces(self):
        n_reqs = 1 if self.local_obs else 4
        curr = Box(low=-250, high=250, shape=(3 + n_reqs + 1,))
        if self.return_agent_actions:
            self.observation_space = Dict({"curr_obs": curr, "other_agent_actions": Box(low=0, high=10, shape=(3,), dtype=np.int32),
                                           "visible_agents": Box(low=0, high=4, shape=(3,), dtype=np.int32)})
        else:
            self.observation_space = curr
        self.action_space = Box(low=0, high=1, shape=(1,))

    def get_observation_space(self, t=0):
        return self.observation_space if t == 0 else self.observation_space_comm

    def get_action_space(self, t=0):
        return self.action_space if t == 0 else self.action_space_comm

    @staticmethod
    def i2id(i):
        return 'agent-' + str(i)

    def _is_comm(self, agent):
        return self.VARIANT == SEQ_COMM and agent < self.comm_agents

    def _obs_value(self, row, agent, other):
        n = obs_len(self.VARIANT, self.local_obs, agent)
        vals = row[:n]
        arr = vals.astype(np.float64) if obs_dtype_is_float(self.VARIANT, agent) else vals.astype(np.int64)
        if self.return_agent_actions and not self._is_comm(agent):
            return {"curr_obs": arr, "other_agent_actions": other, "visible_agents": np.array([1, 1, 1])}
        return arr

    def reset(self):
        obs, agent = self._eng.reset()
        other = None
        if self.return_agent_actions:
            other = self._eng.info()["other_agent_actions"][0].cpu().numpy()
        row, a = obs[0].cpu().numpy(), int(agent[0].item())
        self.action_hist = {}
        self.rew_sum_keeper = [0, 0, 0, 0]
        self._acting = a
        return {self.i2id(a): self._obs_value(row, a, other)}

    def _take_action(self, action_dict):
        aid = self.i2id(self._acting)
        if aid not in action_dict or len(action_dict) != 1:
            raise ValueError("the action dict must hold exactly the acting agent's action (%s), got %s" % (aid, sorted(action_dict)))
        if not self._is_comm(self._acting):
            action_dict[aid] = action_dict[aid][0]                 # the reference rewrites the caller's dict (:338-340, :524-526)
        v = action_dict[aid]
        self.action_hist[aid] = v
        return np.float32(v)

    def step(self, action_dict):
        if self._acting is None:
            raise RuntimeError("call reset() first")
        a = self._take_action(action_dict)
        import torch
        obs, agent, rew, done = self._eng.step(torch.tensor([a], dtype=torch.float32))
        inf = self._eng.info()
        row, ag = obs[0].cpu().numpy(), int(agent[0].item())
        r, flags = float(rew[0].item()), int(done[0].item())
        viol = inf["viol"][0].cpu().numpy()
        temp = float(inf["temp"][0].item())
        other = inf["other_agent_actions"][0].cpu().numpy()
        if flags & _capi.SSD_WS_REW_INT:
            rv = 0
        elif flags & _capi.SSD_WS_REW_F64:
            rv = np.float64(r)
        else:
            rv = np.float32(r)
        end = bool(flags & _capi.SSD_WS_END)
        true_end = bool(flags & _capi.SSD_WS_DONE_ALL)
        if not self._is_comm(ag):
            self.rew_sum_keeper[ag % 4] += rv                      # NumPy promotes as the reference's list does
        aid = self.i2id(ag)
        self._acting = ag
        obs_d = {aid: self._obs_value(row, ag, other)}
        rew_d = {aid: rv}
        done_d = {aid: bool(flags & _capi.SSD_WS_DONE_AGENT), "__all__": true_end}
        info_d = {aid: {"viol": [int(v) for v in viol], "temp": np.float64(temp) if end else 0, "acts": self.action_hist,
                        "end": end, "true_end": true_end, "running_rew": self.rew_sum_keeper}}
        return obs_d, rew_d, done_d, info_d

    def close(self):
        self._eng.close()


class WatershedSeqCommEnv(WatershedSeqEnv):
    """Drop-in for the reference's WatershedSeqCommEnv: comm agents 0-3 send Discrete(5) messages (an integer 0..4, kept in the
    action dict as given) in two rounds, then action agents 4-7 act as in WatershedSeqEnv and see the four latest messages."""
    VARIANT = SEQ_COMM

    def _spaces(self):
        n_reqs = 1 if self.local_obs else 4
        curr = Box(low=-250, high=250, shape=(3 + n_reqs + 4 + 1,))
        if self.return_agent_actions:
            self.observation_space = Dict({"curr_obs": curr, "other_agent_actions": Box(low=0, high=10, shape=(3,), dtype=np.int32),
                                           "visible_agents": Box(low=0, high=8, shape=(3,), dtype=np.int32)})
        else:
            self.observation_space = curr
        self.observation_space_comm = Box(low=-250, high=250, shape=(3 + n_reqs + 4,))
        self.action_space = Box(low=0, high=1, shape=(1,))
        self.action_space_comm = Discrete(5)
