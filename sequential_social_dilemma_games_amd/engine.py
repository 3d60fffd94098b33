"""Batched engine: E independent Harvest / Cleanup envs resident in the HBM of one MI355X.

This is the throughput API behind the dict-API env classes (map_env.py): actions i32 [E,N] in,
uint8 observations [E,N,V,V,3], i32 rewards and u8 dones out, one fused HIP kernel launch per
step (csrc/ssd_kernels.hip) reached through the C ABI of include/ssd.h.

Two calling styles:
  * device tensors (`reset`, `step`, `step_random`, `observe`): torch is used only to own the
    output buffers and to name the HIP stream; calls are asynchronous on torch's current stream;
  * host arrays (`*_host`): numpy in / numpy out, the library stages through its own device
    buffers and returns when the results have landed.
"""
import ctypes as C

import numpy as np

from . import _capi
from . import config as cfgmod
from . import constants as K


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class VecEngine(object):
    def __init__(self, game, ascii_map=None, num_envs=1, num_agents=1, view_len=K.VIEW_LEN, beam_len=K.BEAM_LEN,
                 seed=0, env_index_base=0, device=0, keep_beams=False, color_map=None, harvest_thresholds=None,
                 cleanup_thresholds=None, library_tables=False):
        """harvest_thresholds: uint64 [4], the spawn thresholds by min(#neighbour apples, 3) (a u32 draw succeeds when it is below
        the threshold; 2^32 and above = always); cleanup_thresholds: (apple, waste), uint64 [potential_waste_area + 1] each, by
        the number of 'H' cells.  None: the reference's constants, derived here.  library_tables=True passes NULL for the three
        tables and the colour table -- the library derives them itself -- and excludes the other two and
        color_map."""
        self.game = int(game)
        if ascii_map is None:
            ascii_map = K.HARVEST_MAP if self.game == K.GAME_HARVEST else K.CLEANUP_MAP
        self.ascii_map = [str(r) for r in ascii_map]
        flat, self.H, self.W = cfgmod.ascii_to_bytes(self.ascii_map)
        self.E, self.N = int(num_envs), int(num_agents)
        self.view_len, self.V, self.beam_len = int(view_len), 2 * int(view_len) + 1, int(beam_len)
        self.seed, self.env_index_base, self.device = int(seed), int(env_index_base), int(device)
        self.keep_beams = bool(keep_beams)
        self.num_actions = 8 if self.game == K.GAME_HARVEST else 9     # harvest.py:44, cleanup.py:70
        self._lut = np.ascontiguousarray(cfgmod.make_lut(color_map))
        self.potential_waste_area = cfgmod.potential_waste_area(self.ascii_map) if self.game == K.GAME_CLEANUP else 0
        self.library_tables = bool(library_tables)
        if self.library_tables and (harvest_thresholds is not None or cleanup_thresholds is not None or color_map is not None):
            raise ValueError("library_tables=True excludes harvest_thresholds, cleanup_thresholds and color_map")
        self._thr_h = self._table(harvest_thresholds, 4, "harvest_thresholds") if harvest_thresholds is not None \
            else cfgmod.harvest_thresholds()
        if cleanup_thresholds is not None:
            if not isinstance(cleanup_thresholds, (tuple, list)) or len(cleanup_thresholds) != 2:
                raise ValueError("cleanup_thresholds must be a pair (apple thresholds, waste thresholds)")
            self._thr_ca, self._thr_cw = (self._table(a, self.potential_waste_area + 1, "cleanup_thresholds[%d]" % i)
                                          for i, a in enumerate(cleanup_thresholds))
        else:
            self._thr_ca, self._thr_cw = cfgmod.cleanup_thresholds(self.potential_waste_area)
        self._flat = flat
        c = _capi.SsdConfig()
        c.struct_size = C.sizeof(_capi.SsdConfig)
        c.game, c.height, c.width, c.base_map = self.game, self.H, self.W, flat
        c.num_envs, c.num_agents, c.view_len, c.beam_len = self.E, self.N, self.view_len, self.beam_len
        c.seed, c.env_index_base, c.device_id, c.keep_beams = self.seed, self.env_index_base, self.device, int(self.keep_beams)
        if not self.library_tables:                  # (else NULL: the library's own derivation, ssd_create)
            c.color_lut = self._lut.ctypes.data
            c.harvest_thresholds = self._thr_h.ctypes.data
            c.cleanup_apple_thresholds = self._thr_ca.ctypes.data
            c.cleanup_waste_thresholds = self._thr_cw.ctypes.data
        self._h = C.c_void_p()
        L = _capi.lib()
        _capi.check(L.ssd_create(C.byref(c), C.byref(self._h)))
        self._L = L
        self._out_cache = (None, None)               # (outputs tuple, its pointers) of the last step_random call
        self._ring_out_cache = {}                    # id(outputs tuple) -> (tuple, pointers): register_outputs()
        # Steps since the last reset of ALL envs, or None once envs may be at different points of their episodes (a masked
        # reset, set_state(t=...)): lets SSDVectorEnv know, without asking the device, on which step everybody reaches the
        # horizon.
        self.steps_since_full_reset = None
        self._torch_dev = None
        self._scratch_bufs = {}                      # _scratch(): key -> (the buffer, its view of the shape last asked for)
        if L.ssd_potential_waste_area(self._h) != self.potential_waste_area:
            raise _capi.SsdError("potential_waste_area mismatch between host and library")

    @staticmethod
    def _table(a, n, name):
        """A caller's threshold table: a uint64 array of n entries (checked here, before the library sees a pointer)."""
        if not isinstance(a, np.ndarray) or a.dtype != np.uint64 or a.shape != (n,):
            raise ValueError("%s must be a uint64 array of %d entries" % (name, n))
        return np.ascontiguousarray(a).copy()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.ssd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ device-tensor API
    def _torch(self):
        if self._torch_dev is None:
            import torch
            self._torch_dev = (torch, torch.device("cuda", self.device))
        return self._torch_dev

    def _stream(self):
        """torch's current stream on the engine's device (what the kernels are enqueued on)."""
        torch, dev = self._torch()
        raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)     # the cheap way; the public API builds a Stream object
        if raw is not None:
            return C.c_void_p(raw(dev.index if dev.index is not None else torch.cuda.current_device()))
        return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def alloc_outputs(self, float32=False):
        """(obs u8 -- or float32 -- [E,N,V,V,3], rew i32 [E,N], done u8 [E,N]) on the engine's device."""
        torch, dev = self._torch()
        return (torch.empty((self.E, self.N, self.V, self.V, 3), dtype=torch.float32 if float32 else torch.uint8, device=dev),
                torch.empty((self.E, self.N), dtype=torch.int32, device=dev),
                torch.empty((self.E, self.N), dtype=torch.uint8, device=dev))

    @staticmethod
    def _dp(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _check_tensor(self, t, shape, dtype, name):
        torch, dev = self._torch()
        if t.device != dev or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, tuple(shape), dev))

    def _obs_flags(self, obs):
        """Observation buffers may be uint8 (default) or float32: float32((u8 - 128.0) / 255.0), written by the
        kernel itself (SSD_OBS_F32) -- what the first layer of a policy network consumes."""
        torch, dev = self._torch()
        if obs is None:
            return 0
        if obs.dtype not in (torch.uint8, torch.float32):
            raise ValueError("obs must be uint8 or float32")
        self._check_tensor(obs, (self.E, self.N, self.V, self.V, 3), obs.dtype, "obs")
        return _capi.SSD_OBS_F32 if obs.dtype == torch.float32 else 0

    def reset(self, mask=None, obs=None):
        """MapEnv.reset (map_env.py:214-249) for every env (or those with mask != 0).  Returns obs."""
        torch, dev = self._torch()
        if obs is None:
            obs = (torch.zeros if mask is not None else torch.empty)(
                (self.E, self.N, self.V, self.V, 3), dtype=torch.uint8, device=dev)
        if mask is not None:
            self._check_tensor(mask, (self.E,), torch.uint8, "mask")
        _capi.check(self._L.ssd_reset(self._h, self._dp(mask), self._dp(obs), self._obs_flags(obs), self._stream()), self._h)
        self.steps_since_full_reset = 0 if mask is None else None
        return obs

    def step(self, actions, order=None, out=None, auto_reset=False):
        """MapEnv.step (map_env.py:152-212) on every env.  actions: i32 [E,N] (-1 = absent);
        order: optional u8 [E,N] action-dict order.  Returns (obs, rew, done) device tensors.
        auto_reset: envs that reach the horizon (set_horizon) are reset by the same launch, their obs rows are the
        reset's (SSD_AUTO_RESET; uint8 observations only)."""
        torch, dev = self._torch()
        self._check_tensor(actions, (self.E, self.N), torch.int32, "actions")
        if order is not None:
            self._check_tensor(order, (self.E, self.N), torch.uint8, "order")
        # (back-to-back calls are bound by the host -- tools/step_rate.py -- so the output buffers of the last call again skip
        # their checks and pointer conversions, as in step_random())
        if out is not None and out is self._out_cache[0]:
            obs, rew, done = out
            po, pr, pd, fl = self._out_cache[1]
        else:
            obs, rew, done = out if out is not None else self.alloc_outputs()
            po, pr, pd, fl = self._out_pointers(out, obs, rew, done)
        rc = self._L.ssd_step(self._h, C.c_void_p(actions.data_ptr()), self._dp(order), po, pr, pd,
                              fl | (_capi.SSD_AUTO_RESET if auto_reset else 0), self._stream())
        if rc:
            _capi.check(rc, self._h)
        self._count_after_step(auto_reset)
        return obs, rew, done

    def _out_pointers(self, out, obs, rew, done):
        hit = self._ring_out_cache.get(id(out)) if out is not None else None
        if hit is not None and hit[0] is out:
            ptrs = hit[1]
        else:
            ptrs = (self._dp(obs), self._dp(rew), self._dp(done), self._obs_flags(obs))
        self._out_cache = (out, ptrs)
        return ptrs

    def register_outputs(self, outs):
        """Output tuples (obs, rew, done) that step() / step_random() will be handed in turn -- the slots of an output ring
        (SSDVectorEnv(track_episodes=True)): their pointers are worked out once, here.  Replaces the previous registration."""
        self._ring_out_cache = {}
        for out in outs:
            obs, rew, done = out
            self._ring_out_cache[id(out)] = (out, (self._dp(obs), self._dp(rew), self._dp(done), self._obs_flags(obs)))

    def _count_after_step(self, auto_reset):
        self._count_steps(1)
        if auto_reset and self.steps_since_full_reset is not None and getattr(self, "horizon", 0) > 0 \
                and self.steps_since_full_reset >= self.horizon:
            self.steps_since_full_reset = 0          # everybody reached the horizon together and was reset by that launch

    def step_random(self, out=None, actions_out=None, num_actions=None, auto_reset=False):
        """One step with uniform random actions drawn on the device (rollout.py:62-70)."""
        if out is not None and out is self._out_cache[0]:                  # same buffers as last time: pointers are known
            obs, rew, done = out
            po, pr, pd, fl = self._out_cache[1]
        else:
            obs, rew, done = out if out is not None else self.alloc_outputs()
            po, pr, pd, fl = self._out_pointers(out, obs, rew, done)
        na = self.num_actions if num_actions is None else int(num_actions)
        rc = self._L.ssd_step_random(self._h, na, self._dp(actions_out), po, pr, pd,
                                     fl | (_capi.SSD_AUTO_RESET if auto_reset else 0), self._stream())
        if rc:
            _capi.check(rc, self._h)
        self._count_after_step(auto_reset)
        return obs, rew, done

    def _count_steps(self, n):
        if self.steps_since_full_reset is not None:
            self.steps_since_full_reset += n

    def set_rollout_chains(self, chains):
        """How many independent env ranges rollout_random() enqueues on streams of its own (0 = automatic)."""
        _capi.check(self._L.ssd_set_rollout_chains(self._h, int(chains)), self._h)

    def _rollout_args(self, obs, rew, done):
        # (the buffers of the last call again: their checks and pointers are known -- a short call is mostly fixed costs)
        cache = getattr(self, "_roll_cache", None)
        if cache is not None and cache[0] is obs and cache[1] is rew and cache[2] is done:
            return cache[3]
        torch, dev = self._torch()
        first = obs if obs is not None else rew if rew is not None else done
        if first is None:
            raise ValueError("a rollout needs at least one of obs / rew / done (their leading dimension is the output ring)")
        ring = int(first.shape[0])
        if obs is not None:
            if obs.dtype not in (torch.uint8, torch.float32):
                raise ValueError("obs must be uint8 or float32")
            self._check_tensor(obs, (ring, self.E, self.N, self.V, self.V, 3), obs.dtype, "obs")
        if rew is not None:
            self._check_tensor(rew, (ring, self.E, self.N), torch.int32, "rew")
        if done is not None:
            self._check_tensor(done, (ring, self.E, self.N), torch.uint8, "done")
        args = (self._dp(obs), self._dp(rew), self._dp(done), ring, (_capi.SSD_OBS_F32 if obs is not None and obs.dtype == torch.float32 else 0))
        self._roll_cache = (obs, rew, done, args)
        return args

    def _count_rollout(self, n_steps, reset_every, step0):
        n_steps, reset_every, step0 = int(n_steps), int(reset_every), int(step0)
        last = None                                  # index of the last step of this call that a full reset preceded
        if reset_every > 0 and n_steps > 0:
            k = (n_steps - 1) - ((step0 + n_steps - 1) % reset_every)
            last = k if k >= 0 else None
        if last is not None:
            self.steps_since_full_reset = n_steps - last
        else:
            self._count_steps(n_steps)

    def _check_stats(self, stats, rew, n_steps):
        """A rollout with `stats` (an EpisodeStats of this batch) needs its rew ring, long enough to hold every step of the call."""
        if stats is None:
            return
        if rew is None:
            raise ValueError("stats need the call's rewards: pass rew")
        if stats.E != self.E or stats.N != self.N or stats.device != self.device:
            raise ValueError("stats were made for %d envs x %d agents on device %d, the engine has %d x %d on device %d"
                             % (stats.E, stats.N, stats.device, self.E, self.N, self.device))
        if int(rew.shape[0]) < int(n_steps):
            raise ValueError("stats need every step's rewards: the rew ring (%d) is shorter than n_steps (%d)"
                             % (int(rew.shape[0]), int(n_steps)))

    def rollout_random(self, n_steps, obs, rew=None, done=None, reset_every=0, step0=0, num_actions=None, fused=False, stats=None):
        """rollout.py:58-70 as ONE library call: `n_steps` random-action steps (plus a full reset whenever
        (step0 + k) % reset_every == 0) enqueued back to back.  obs / rew / done are device tensors with a leading ring
        dimension R: step k writes slot (step0 + k) % R  (obs u8 or f32 [R,E,N,V,V,3], rew i32 [R,E,N], done u8 [R,E,N]).
        Same steps, bit for bit, as n_steps calls of step_random(), without the host as the bottleneck -- not the same launches:
        the library's split chains render a step's observations in the next launch, and on Harvest's shipped and enlarged maps and
        Cleanup's shipped one a launch advances its envs by a run of steps -- four wherever four remain before the call's end and the
        next reset, else two where two remain (Cleanup with 10 agents: two at the most; Harvest's shipped map with 5 agents in calls of
        256 steps or more: eight wherever eight remain); rollout_path()["pairs"] and ["run"] say so.
        fused=True: ONE kernel launch for the whole call (SSD_ROLLOUT_FUSED) -- every env stays in LDS / registers across
        its steps; same results, uint8 observations only.  fused="auto": the library picks (SSD_ROLLOUT_AUTO: the fused kernel
        for uint8 observations and two steps or more, the chains otherwise; rollout_path() says which form ran).
        stats: an EpisodeStats of this batch, folded after the call from its rew ring (episodes end at the full resets of
        reset_every only; rew is required and its ring must hold n_steps steps)."""
        self._check_stats(stats, rew, n_steps)
        po, pr, pd, ring, f32 = self._rollout_args(obs, rew, done)
        na = self.num_actions if num_actions is None else int(num_actions)
        rc = self._L.ssd_rollout_random(self._h, na, int(n_steps), int(reset_every), int(step0), po, pr, pd, ring,
                                        f32 | self._fused_flag(fused), self._stream())
        if rc:
            _capi.check(rc, self._h)
        self._count_rollout(n_steps, reset_every, step0)
        if stats is not None:
            stats.fold(rew, None, step0=step0, n_steps=n_steps, reset_every=reset_every)

    def rollout_actions(self, actions, n_steps, obs, rew=None, done=None, reset_every=0, step0=0, fused=False, order=None,
                        stats=None):
        """The same call with caller-supplied actions (ssd_rollout_actions): what the reference's callers do, env.step(policy
        actions) per step (visuallizer_rllib.py:121-153), for a recorded sequence / an action chunk of n_steps steps.
        actions: int32 [A,E,N] device tensor (-1 = the agent does not act); step k reads slot (step0 + k) % A.  order: optional
        uint8 [A,E,N], per step the agent indices in action-dict order, 0xFF-terminated (None: index order).  Outputs as
        rollout_random() (fused=True / "auto" as there).  Reuse the same action / output tensors from call to call: the launches'
        arguments are cached by them.  stats: as in rollout_random()."""
        torch, dev = self._torch()
        self._check_stats(stats, rew, n_steps)
        cache = getattr(self, "_act_cache", None)
        if cache is not None and cache[0] is actions and cache[1] is order:
            pa, pord, aring = cache[2]
        else:
            aring = int(actions.shape[0])
            self._check_tensor(actions, (aring, self.E, self.N), torch.int32, "actions")
            if order is not None:
                self._check_tensor(order, (aring, self.E, self.N), torch.uint8, "order")
            pa, pord = self._dp(actions), self._dp(order)
            self._act_cache = (actions, order, (pa, pord, aring))
        po, pr, pd, ring, f32 = self._rollout_args(obs, rew, done)
        rc = self._L.ssd_rollout_actions(self._h, pa, pord, aring, int(n_steps), int(reset_every), int(step0), po, pr, pd, ring,
                                         f32 | self._fused_flag(fused), self._stream())
        if rc:
            _capi.check(rc, self._h)
        self._count_rollout(n_steps, reset_every, step0)
        if stats is not None:
            stats.fold(rew, None, step0=step0, n_steps=n_steps, reset_every=reset_every)

    @staticmethod
    def _fused_flag(fused):
        if isinstance(fused, str):
            if fused != "auto":
                raise ValueError("fused must be True, False or 'auto'")
            return _capi.SSD_ROLLOUT_AUTO
        return _capi.SSD_ROLLOUT_FUSED if fused else 0

    # ------------------------------------------------------------------ policy in the loop (include/ssd.h, POLICY ROLLOUTS)
    # What differs between the policies is read from the policy's class attributes (policy.PolicyBase): STATE_ROWS (0: no
    # state), TAKES_PREV_ACTIONS (the MOA's previous joint action, influence and clip), C_FORWARD / C_ROLLOUT (the library's
    # entry points) and scratch_shape().
    def _policy_weights(self, policy):
        """Checks a ConvFCPolicy, ConvLSTMPolicy or ConvMOAPolicy against this engine (everything before anything is enqueued);
        returns its weight-set count."""
        from .policy import ConvFCPolicy, ConvLSTMPolicy, ConvMOAPolicy
        torch, dev = self._torch()
        if not isinstance(policy, (ConvFCPolicy, ConvLSTMPolicy, ConvMOAPolicy)):
            raise ValueError("policy must be a ConvFCPolicy, a ConvLSTMPolicy or a ConvMOAPolicy")
        if policy.TAKES_PREV_ACTIONS and policy.num_agents != self.N:
            raise ValueError("the MOA policy is built for %d agents, the engine has %d" % (policy.num_agents, self.N))
        if self.V != _capi.SSD_POL_VIEW:
            raise ValueError("the policy network takes 15 x 15 views (view_len 7); this engine has V = %d" % self.V)
        if policy.num_actions != self.num_actions:
            raise ValueError("the policy has %d actions, the game Discrete(%d)" % (policy.num_actions, self.num_actions))
        if policy.num_sets not in (1, self.N):
            raise ValueError("the policy has %d weight sets: 1 (shared) or %d (one per agent) expected" % (policy.num_sets, self.N))
        if policy.conv_w.device != dev:
            raise ValueError("the policy's parameters are on %s, the engine on %s" % (policy.conv_w.device, dev))
        if self.N < 1:
            raise ValueError("a policy needs at least one agent")
        return policy.num_sets

    def _scratch(self, key, shape, dtype):
        """The engine's buffer `key` as a tensor of `shape`: kept between calls, allocated anew only to grow.  "policy" is the
        scratch of a recurrent policy's calls (policy.scratch_shape), "actions" the action ring a rollout was not given."""
        flat, t = self._scratch_bufs.get(key, (None, None))
        if t is None or tuple(t.shape) != shape:
            torch, dev = self._torch()
            n = int(np.prod(shape))
            if flat is None or flat.numel() < n:
                flat = torch.empty(n, dtype=dtype, device=dev)
            t = flat[:n].view(shape)
            self._scratch_bufs[key] = (flat, t)
        return t

    def _check_actions_like(self, t, shape, name):
        torch, dev = self._torch()
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be an int32 tensor of shape %s" % (name, tuple(shape)))
        self._check_tensor(t, tuple(shape), torch.int32, name)

    def _check_state(self, state, shape, who, shown):
        """The state a call of a policy with one needs: a float32 tensor of `shape` on the engine's device."""
        torch, dev = self._torch()
        if not isinstance(state, torch.Tensor):
            raise ValueError("%s needs state: a float32 tensor %s" % (who, shown))
        self._check_tensor(state, shape, torch.float32, "state")

    def _check_starts(self, starts, lead):
        """starts bool / uint8 of shape lead, or None -> the uint8 tensor the library reads, or None."""
        torch, dev = self._torch()
        if starts is None:
            return None
        if not isinstance(starts, torch.Tensor) or starts.dtype not in (torch.bool, torch.uint8):
            raise ValueError("starts must be a bool or uint8 tensor of shape %s" % (lead,))
        self._check_tensor(starts, lead, starts.dtype, "starts")
        return starts.view(torch.uint8)

    @staticmethod
    def _check_clip(influence_clip):
        clip = float(influence_clip)
        if not (0.0 <= clip < float("inf")):
            raise ValueError("influence_clip must be finite and >= 0")
        return clip

    def policy_forward(self, policy, obs, state=None, starts=None, prev_actions=None, actions=None, influence_clip=10.0):
        """The policy's forward pass on the device (ssd_policy_forward): obs uint8 [..., N, 15, 15, 3] -> (logits float32
        [..., N, A], value float32 [..., N]), enqueued on the current stream.  The same kernel as rollout_policy()'s.
        A ConvLSTMPolicy (ssd_policy_lstm_forward) takes state float32 [..., N, 2, C] (required) and starts bool / uint8
        [..., N] (rows whose state is taken as zero; None: none) and returns (logits, value, new state [..., N, 2, C]).
        A ConvMOAPolicy (ssd_policy_moa_forward) takes state float32 [..., N, 4, C] and prev_actions int32 [..., N] (both
        required), starts as above and, for the influence, actions int32 [..., N] (this step's) and influence_clip; it returns
        (logits, value, moa_logits [..., N, N-1, A], cf_logits [..., N, A, N-1, A], new state, influence [..., N] or None)."""
        torch, dev = self._torch()
        P = self._policy_weights(policy)
        V, N, A = self.V, self.N, self.num_actions
        if not isinstance(obs, torch.Tensor) or obs.dtype != torch.uint8 or obs.device != dev or not obs.is_contiguous() \
                or obs.dim() < 4 or tuple(obs.shape[-4:]) != (N, V, V, 3):
            raise ValueError("obs must be a contiguous uint8 tensor of shape [..., %d, %d, %d, 3] on %s" % (N, V, V, dev))
        B = obs.numel() // (N * V * V * 3)
        if B < 1:
            raise ValueError("obs holds no observation")
        lead = tuple(obs.shape[:-3])
        rows, moa = policy.STATE_ROWS, policy.TAKES_PREV_ACTIONS
        if not moa and (prev_actions is not None or actions is not None):
            raise ValueError("prev_actions and actions belong to a ConvMOAPolicy")
        if not rows:
            if state is not None or starts is not None:
                raise ValueError("state and starts belong to a ConvLSTMPolicy; a ConvFCPolicy has no state")
        else:
            C = policy.cell_size
            self._check_state(state, lead + (rows, C), "a " + type(policy).__name__, lead + (rows, C))
        if moa:
            self._check_actions_like(prev_actions, lead, "prev_actions")
            if actions is not None:
                self._check_actions_like(actions, lead, "actions")
        starts = self._check_starts(starts, lead)
        clip = self._check_clip(influence_clip) if moa else None
        e = lambda shape: torch.empty(lead + shape, dtype=torch.float32, device=dev)   # noqa: E731
        dp = self._dp
        logits, value = e((A,)), e(())
        # the entry points take (weights, P, A[, C], obs[, prev_actions][, state, starts], B, N[, scratch, new state], logits,
        # value[, moa_logits, cf_logits, actions, influence, clip], device, flags, stream)
        out, net, inp, res, extra = (logits, value), [], [], [], []
        if rows:
            new_state = torch.empty_like(state)
            scratch = self._scratch("policy", policy.scratch_shape(B * N), torch.float32)
            net, inp, res = [C], [dp(state), dp(starts)], [dp(scratch), dp(new_state)]
            out += (new_state,)
        if moa:
            pred, cf, infl = e((N - 1, A)), e((A, N - 1, A)), e(()) if actions is not None else None
            inp.insert(0, dp(prev_actions))
            extra = [dp(pred), dp(cf), dp(actions), dp(infl), clip]
            out = (logits, value, pred, cf, new_state, infl)
        w = policy.packed()
        _capi.policy_check(getattr(self._L, policy.C_FORWARD)(dp(w), P, A, *net, dp(obs), *inp, B, N, *res, dp(logits), dp(value),
                                                               *extra, self.device, 0, self._stream()))
        return out

    def rollout_policy(self, policy, obs_in, n_steps, obs, actions=None, logp=None, value=None, logits=None, rew=None, done=None,
                       last_value=None, step0=0, greedy=False, stats=None, state=None, state_ring=None, state_every=1,
                       prev_actions=None, prev_actions_ring=None, influence=None, influence_clip=10.0):
        """A closed-loop rollout (ssd_rollout_policy): n_steps rounds of (policy forward on the current observation, action, step
        with automatic reset at the horizon) enqueued by one call, no host synchronisation.  The rings have a leading dimension
        R and step k writes slot (step0 + k) % R:
          obs u8 [R,E,N,15,15,3] (required: the next step's policy reads it), actions i32 [R,E,N] (None: a ring of the engine's
          own), logp / value f32 [R,E,N], logits f32 [R,E,N,A], rew i32 [R,E,N], done u8 [R,E,N];
        obs_in u8 [E,N,15,15,3] is the observation of the current state (the last reset's or step's); last_value f32 [E,N]
        receives the value of the final observation.  greedy: argmax actions, else drawn from the S_POLICY stream
        (include/ssd.h).  stats: an EpisodeStats of this batch folded from rew and done (both required, R >= n_steps).
        A ConvLSTMPolicy (ssd_rollout_policy_lstm) also takes state float32 [E,N,2,C] (required), the carried state, updated in
        place and zero at every episode start; state_ring float32 [S,E,N,2,C] receives the state call-relative step k used in
        slot k // state_every for every k that is a multiple of state_every (S >= ceil(n_steps / state_every)).
        A ConvMOAPolicy (ssd_rollout_policy_moa) takes state [E,N,4,C] and state_ring [S,E,N,4,C] as above, prev_actions int32
        [E,N] (required: the carried previous joint action, read by step 0 and left holding the last step's), and the rings
        prev_actions_ring int32 [R,E,N] (what each step's MOA read) and influence float32 [R,E,N] (each step's influence reward,
        clipped to influence_clip)."""
        torch, dev = self._torch()
        P = self._policy_weights(policy)
        SR, moa = policy.STATE_ROWS, policy.TAKES_PREV_ACTIONS
        n_steps, step0 = int(n_steps), int(step0)
        if n_steps < 1:
            raise ValueError("n_steps must be >= 1")
        if step0 < 0:
            raise ValueError("step0 must be >= 0")
        E, N, V, A = self.E, self.N, self.V, self.num_actions
        if not isinstance(obs, torch.Tensor) or obs.dim() != 6:
            raise ValueError("obs must be a uint8 ring [R,%d,%d,%d,%d,3]" % (E, N, V, V))
        R = int(obs.shape[0])
        if R < 1:
            raise ValueError("the ring length must be >= 1")
        self._check_tensor(obs, (R, E, N, V, V, 3), torch.uint8, "obs")
        if not isinstance(obs_in, torch.Tensor):
            raise ValueError("obs_in must be a uint8 tensor [%d,%d,%d,%d,3]" % (E, N, V, V))
        self._check_tensor(obs_in, (E, N, V, V, 3), torch.uint8, "obs_in")
        if R > 1 and (E * N) % 4:
            raise ValueError("an observation ring of more than one slot needs num_envs * num_agents to be a multiple of 4")
        for t, dt, shape, name in ((actions, torch.int32, (R, E, N), "actions"), (logp, torch.float32, (R, E, N), "logp"),
                                   (value, torch.float32, (R, E, N), "value"), (logits, torch.float32, (R, E, N, A), "logits"),
                                   (rew, torch.int32, (R, E, N), "rew"), (done, torch.uint8, (R, E, N), "done"),
                                   (last_value, torch.float32, (E, N), "last_value")):
            if t is not None:
                if not isinstance(t, torch.Tensor):
                    raise ValueError("%s must be a tensor" % name)
                self._check_tensor(t, shape, dt, name)
        if stats is not None:
            self._check_stats(stats, rew, n_steps)
            if done is None:
                raise ValueError("stats need the call's done flags: pass done")
        if not SR:
            if state is not None or state_ring is not None:
                raise ValueError("state and state_ring belong to a ConvLSTMPolicy; a ConvFCPolicy has no state")
        else:
            C = policy.cell_size
            self._check_state(state, (E, N, SR, C), "a recurrent policy", "[%d,%d,%d,%d]" % (E, N, SR, C))
            state_every = int(state_every)
            S = 0
            if state_ring is not None:
                if state_every < 1:
                    raise ValueError("state_every must be >= 1")
                if not isinstance(state_ring, torch.Tensor) or state_ring.dim() != 5:
                    raise ValueError("state_ring must be a float32 ring [S,%d,%d,%d,%d]" % (E, N, SR, C))
                S = int(state_ring.shape[0])
                self._check_tensor(state_ring, (S, E, N, SR, C), torch.float32, "state_ring")
                if S < -(-n_steps // state_every):
                    raise ValueError("state_ring needs ceil(n_steps / state_every) = %d slots, has %d" % (-(-n_steps // state_every), S))
                if state_ring.data_ptr() < state.data_ptr() + state.numel() * 4 and state.data_ptr() < state_ring.data_ptr() + state_ring.numel() * 4:
                    raise ValueError("state_ring must not overlap state")
        if moa:
            self._check_actions_like(prev_actions, (E, N), "prev_actions")
            if prev_actions_ring is not None:
                self._check_actions_like(prev_actions_ring, (R, E, N), "prev_actions_ring")
            if influence is not None:
                if not isinstance(influence, torch.Tensor):
                    raise ValueError("influence must be a float32 ring [R,%d,%d]" % (E, N))
                self._check_tensor(influence, (R, E, N), torch.float32, "influence")
            clip = self._check_clip(influence_clip)
        elif prev_actions is not None or prev_actions_ring is not None or influence is not None:
            raise ValueError("prev_actions, prev_actions_ring and influence belong to a ConvMOAPolicy")
        if actions is None:
            actions = self._scratch("actions", (R, E, N), torch.int32)
        w = policy.packed()
        dp = self._dp
        # (handle, weights, P[, C], obs_in, n_steps, step0[, the state's arguments][, the MOA's][, scratch]), then what every
        # policy's rollout ends in
        head = [self._h, dp(w), P, dp(obs_in), n_steps, step0]
        if SR:
            head.insert(3, C)
            head += [dp(state), dp(state_ring), S, state_every]
            if moa:
                head += [dp(prev_actions), dp(prev_actions_ring), dp(influence), clip]
            head.append(dp(self._scratch("policy", policy.scratch_shape(E * N), torch.float32)))
        rc = getattr(self._L, policy.C_ROLLOUT)(*head, dp(obs), dp(actions), dp(logp), dp(value), dp(logits), dp(rew), dp(done), R,
                                                dp(last_value), _capi.SSD_POLICY_GREEDY if greedy else 0, self._stream())
        if rc:
            _capi.check(rc, self._h)
        self._count_auto_steps(n_steps)
        if stats is not None:
            stats.fold(rew, done, step0=step0, n_steps=n_steps)
        return actions

    def _count_auto_steps(self, n):
        """n steps with SSD_AUTO_RESET: while every env started its episode together, they all reach the horizon together."""
        s, h = self.steps_since_full_reset, getattr(self, "horizon", 0)
        if s is None:
            return
        if h <= 0:
            self.steps_since_full_reset = s + n
            return
        first = max(h - s, 1)                        # steps until the first reset
        self.steps_since_full_reset = s + n if n < first else (n - first) % h

    def rollout_path(self):
        """How the last rollout call was dispatched (ssd_rollout_path): {"aql", "coherent", "split", "pairs", "fused", "sync", "forked",
        "queue_dropped": bool, "chains": n, "pool": dispatch queues the device's pool settled on, "agent_match": how the HSA agent
        of the handle's HIP device was found ("pci" / "uuid" / "ordinal" / "none"), "run": the longest run of steps one launch of
        the call took (1, 2, 4 or 8; 0: the call did not go through the library's own queues)} -- lets a benchmark or a test
        tell a silent fallback from the path it meant to measure."""
        m = self._L.ssd_rollout_path(self._h)
        return {"aql": bool(m & _capi.SSD_PATH_AQL), "coherent": bool(m & _capi.SSD_PATH_COHERENT), "split": bool(m & _capi.SSD_PATH_SPLIT),
                "pairs": bool(m & _capi.SSD_PATH_PAIRS),
                "fused": bool(m & _capi.SSD_PATH_FUSED), "sync": bool(m & _capi.SSD_PATH_SYNC), "forked": bool(m & _capi.SSD_PATH_FORKED),
                "queue_dropped": bool(m & _capi.SSD_PATH_QUEUE_DROPPED), "chains": (m >> 8) & 15, "pool": (m >> 12) & 7,
                "agent_match": ("none", "pci", "uuid", "ordinal")[(m >> 16) & 3], "run": (m >> _capi.SSD_PATH_RUN_SHIFT) & 15}

    def observe(self, rotate=True, obs=None):
        torch, dev = self._torch()
        if obs is None:
            obs = torch.empty((self.E, self.N, self.V, self.V, 3), dtype=torch.uint8, device=dev)
        _capi.check(self._L.ssd_observe(self._h, self._dp(obs), (0 if rotate else _capi.SSD_NO_ROTATE) | self._obs_flags(obs),
                                        self._stream()), self._h)
        return obs

    # ------------------------------------------------------------------ host-array API
    def _host_out(self):
        return (np.zeros((self.E, self.N, self.V, self.V, 3), np.uint8), np.zeros((self.E, self.N), np.int32),
                np.zeros((self.E, self.N), np.uint8))

    def reset_host(self, mask=None):
        obs = np.zeros((self.E, self.N, self.V, self.V, 3), np.uint8)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.E)
        _capi.check(self._L.ssd_reset(self._h, _ptr(m), _ptr(obs), _capi.SSD_HOST_PTRS, None), self._h)
        self.steps_since_full_reset = 0 if mask is None else None
        return obs

    def step_host(self, actions, order=None):
        actions = np.ascontiguousarray(actions, dtype=np.int32).reshape(self.E, self.N)
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.uint8).reshape(self.E, self.N)
        obs, rew, done = self._host_out()
        _capi.check(self._L.ssd_step(self._h, _ptr(actions), _ptr(order), _ptr(obs), _ptr(rew), _ptr(done),
                                     _capi.SSD_HOST_PTRS, None), self._h)
        self._count_steps(1)
        return obs, rew, done

    def step_random_host(self):
        act = np.zeros((self.E, self.N), np.int32)
        obs, rew, done = self._host_out()
        _capi.check(self._L.ssd_step_random(self._h, self.num_actions, _ptr(act), _ptr(obs), _ptr(rew), _ptr(done),
                                            _capi.SSD_HOST_PTRS, None), self._h)
        self._count_steps(1)
        return act, obs, rew, done

    def observe_host(self, rotate=True):
        obs = np.zeros((self.E, self.N, self.V, self.V, 3), np.uint8)
        flags = _capi.SSD_HOST_PTRS | (0 if rotate else _capi.SSD_NO_ROTATE)
        _capi.check(self._L.ssd_observe(self._h, _ptr(obs), flags, None), self._h)
        return obs

    # ------------------------------------------------------------------ state access
    def get_state(self):
        E, N, H, W = self.E, self.N, self.H, self.W
        s = dict(world=np.zeros((E, H, W), np.int8), beam=np.zeros((E, H, W), np.int8) if self.keep_beams else None,
                 pos=np.zeros((E, N, 2), np.int16), orient=np.zeros((E, N), np.uint8),
                 episode=np.zeros(E, np.uint32), t=np.zeros(E, np.uint32))
        _capi.check(self._L.ssd_get_state(self._h, _ptr(s["world"]), _ptr(s["beam"]), _ptr(s["pos"]), _ptr(s["orient"]),
                                          _ptr(s["episode"]), _ptr(s["t"])), self._h)
        return s

    def set_state(self, world=None, beam=None, pos=None, orient=None, episode=None, t=None):
        E, N, H, W = self.E, self.N, self.H, self.W

        def prep(a, dt, shape, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            if a.shape != shape:
                raise ValueError("%s must have shape %s, got %s" % (name, shape, a.shape))
            return a
        world, beam = prep(world, np.int8, (E, H, W), "world"), prep(beam, np.int8, (E, H, W), "beam")
        pos, orient = prep(pos, np.int16, (E, N, 2), "pos"), prep(orient, np.uint8, (E, N), "orient")
        episode, t = prep(episode, np.uint32, (E,), "episode"), prep(t, np.uint32, (E,), "t")
        _capi.check(self._L.ssd_set_state(self._h, _ptr(world), _ptr(beam), _ptr(pos), _ptr(orient), _ptr(episode),
                                          _ptr(t)), self._h)
        if t is not None:
            self.steps_since_full_reset = None

    def set_horizon(self, horizon):
        """done = (t >= horizon) from now on (RLlib's `horizon`, train_baseline.py:131); 0 = never (reference envs)."""
        _capi.check(self._L.ssd_set_horizon(self._h, int(horizon)), self._h)
        self.horizon = int(horizon)

    def waste_count(self):
        """u32 [E]: the number of 'H' cells the last step / reset computed the Cleanup spawn probabilities from."""
        out = np.zeros(self.E, np.uint32)
        _capi.check(self._L.ssd_get_waste_count(self._h, _ptr(out)), self._h)
        return out

    def render_full(self, e=0):
        """map_to_colors() of the whole grid of env e (map_env.py:316-339): u8 [H,W,3]."""
        rgb = np.zeros((self.H, self.W, 3), np.uint8)
        _capi.check(self._L.ssd_render_full(self._h, int(e), _ptr(rgb)), self._h)
        return rgb

    def render_frames(self, e_begin=0, count=None, out=None, host=False):
        """map_to_colors() of the whole grids of envs [e_begin, e_begin+count) in one launch: u8 [count,H,W,3] -- a device
        tensor (enqueued on the current stream), or with host=True a NumPy array (synchronous).  These are the frames
        rollout.py:77 / visuallizer_rllib.py:161 collect one env at a time."""
        count = self.E - e_begin if count is None else int(count)
        if e_begin < 0 or count < 0 or e_begin + count > self.E:
            raise ValueError("env range [%d, %d) outside the batch of %d" % (e_begin, e_begin + count, self.E))
        shape = (count, self.H, self.W, 3)
        if host:
            rgb = np.zeros(shape, np.uint8) if out is None else out
            if rgb.dtype != np.uint8 or rgb.shape != shape or not rgb.flags.c_contiguous:
                raise ValueError("out must be a C-contiguous uint8 array of shape %s" % (shape,))
            if count:
                _capi.check(self._L.ssd_render_frames(self._h, int(e_begin), count, _ptr(rgb), _capi.SSD_HOST_PTRS, None), self._h)
            return rgb
        torch, dev = self._torch()
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        elif out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError("out must be a contiguous uint8 tensor of shape %s" % (shape,))
        if count:
            _capi.check(self._L.ssd_render_frames(self._h, int(e_begin), count, self._dp(out), 0, self._stream()), self._h)
        return out

    def agent_action_obs(self, actions=None, done=None, out=None):
        """The `other_agent_actions` / `visible_agents` members of the reference's observation dict under
        return_agent_actions=True (map_env.py:201-205, :242-246, :749-770) for the whole batch: int64 [E,N,N-1] device tensors.
        actions: this step's int32 [E,N] actions (None: the reset form, zeros); done: optional u8 [E,N] (rows of envs that the
        step reset, or is about to, are zeros).  Row (e,i) lists the OTHER agents' actions in string-sorted id order, -1 for an
        agent that did not act.  visible_agents is all ones (the reference's quirk, :767)."""
        torch, dev = self._torch()
        shape = (self.E, self.N, max(self.N - 1, 0))
        if actions is not None:
            self._check_tensor(actions, (self.E, self.N), torch.int32, "actions")
        if done is not None:
            self._check_tensor(done, (self.E, self.N), torch.uint8, "done")
        oaa, vis = out if out is not None else (torch.empty(shape, dtype=torch.int64, device=dev), torch.empty(shape, dtype=torch.int64, device=dev))
        for t, name in ((oaa, "other_agent_actions"), (vis, "visible_agents")):
            self._check_tensor(t, shape, torch.int64, name)
        _capi.check(self._L.ssd_agent_action_obs(self._h, self._dp(actions), self._dp(done), self._dp(oaa), self._dp(vis), 0,
                                                 self._stream()), self._h)
        return oaa, vis

    def agent_action_obs_host(self, actions=None, done=None):
        shape = (self.E, self.N, max(self.N - 1, 0))
        oaa, vis = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
        a = None if actions is None else np.ascontiguousarray(actions, dtype=np.int32).reshape(self.E, self.N)
        d = None if done is None else np.ascontiguousarray(done, dtype=np.uint8).reshape(self.E, self.N)
        _capi.check(self._L.ssd_agent_action_obs(self._h, _ptr(a), _ptr(d), _ptr(oaa), _ptr(vis), _capi.SSD_HOST_PTRS, None), self._h)
        return oaa, vis

    def status(self, clear=True):
        st = C.c_uint32(0)
        _capi.check(self._L.ssd_device_status(self._h, C.byref(st), int(clear)), self._h)
        return st.value

    def synchronize(self):
        _capi.check(self._L.ssd_synchronize(self._h), self._h)

    # ------------------------------------------------------------------ bookkeeping for bench / roofline
    def algorithmic_bytes_per_env_step(self):
        return cfgmod.algorithmic_bytes_per_env_step(self.H, self.W, self.N, self.V)
