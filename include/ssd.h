/* include/ssd.h -- C ABI of libssd_hip.so, the MI355X-native engine for the
 * MapEnv.step() hot path of the Harvest / Cleanup gridworlds.
 *
 * The reference is pure Python: it has no FFI.  The boundary this ABI replaces is the
 * RLlib MultiAgentEnv duck type that `MapEnv` implements (reference
 * social_dilemmas/envs/map_env.py:60,152,214) -- every entry point below cites the
 * reference method it stands in for.  The host-side mirror of that interface
 * (sequential_social_dilemma_games_amd/map_env.py) binds these symbols through ctypes;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions: every call returns 0 on success or a negative SSD_E_* code and never
 * throws; the caller owns every buffer passed in (the engine only allocates its own
 * state); one handle = one device + one caller-chosen stream per call; calls on one
 * handle are not re-entrant, distinct handles are independent (a host-pointer call first waits for the stream of the handle's
 * last device-pointer call when that is another stream, so mixing the two styles keeps program order); there is no global state
 * (the reference's module-global RNGs become per-handle seed + counters).  There is no
 * CPU backend: without a usable HIP device ssd_create fails with SSD_E_DEVICE.
 *
 * Batched layouts (E = num_envs of the handle, N = num_agents, V = 2*view_len+1):
 *   actions i32 [E,N]   -1 = agent absent from the action dict this step
 *   order   u8  [E,N]   agent indices in action-dict order, 0xFF-terminated; NULL = index order
 *   obs     u8  [E,N,V,V,3]   RGB; the reference's float64 obs is (u8 - 128.0) / 255.0
 *           f32 [E,N,V,V,3]   with SSD_OBS_F32: float32(that float64 value), i.e. the reference observation cast to
 *                             its declared Box(dtype=float32) space (harvest.py:39-40), NHWC per agent
 *   rew     i32 [E,N]
 *   done    u8  [E,N]   0 (agent.py:174-175,209-210) unless a horizon is set (ssd_set_horizon)
 */
#ifndef SSD_H
#define SSD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSD_ABI_VERSION 6   /* 6: policy rollouts (ssd_policy_forward, ssd_rollout_policy).  5: episode statistics (ssd_stats_*).  4: the Watershed games (ssd_ws_*).  3: SSD_ROLLOUT_AUTO; SSD_STEP_CHAINS removed.  2: ssd_rollout_actions, ssd_profiler_attached; SSD_ROLLOUT_PIPELINED removed */

enum {
    SSD_OK = 0,
    SSD_E_INVALID = -1,   /* bad argument / configuration (open map, too many agents, ...) */
    SSD_E_DEVICE = -2,    /* no usable HIP device, or a HIP call failed (see ssd_last_error) */
    SSD_E_NOMEM = -3,
    SSD_E_STATE = -4      /* device status word is non-zero (see ssd_device_status) */
};

enum { SSD_GAME_HARVEST = 0, SSD_GAME_CLEANUP = 1 };

/* flags of the stepping calls */
enum {
    SSD_HOST_PTRS = 1u << 0, /* actions/order/obs/rew/done are host memory: the engine stages them
                                and the call returns after the results have landed.  Without it
                                they are device pointers on the handle's device and the call only
                                enqueues work on `stream`. */
    SSD_NO_ROTATE = 1u << 1, /* ssd_observe only: reset-form observation (map_env.py:239-240) */
    SSD_ROLLOUT_FUSED = 1u << 3, /* ssd_rollout_random only: ONE kernel launch for the whole call -- every env stays in LDS and
                                registers across its n_steps steps and only the per-step outputs (and, at the end, the state)
                                go to HBM.  Same results; no per-step launch, state reload or write-back.  uint8 obs only. */
    SSD_AUTO_RESET = 1u << 4,   /* ssd_step / ssd_step_random: an env whose step reaches the horizon (ssd_set_horizon; its done flags
                                are 1) starts its next episode in the same launch: MapEnv.reset (map_env.py:214-249) is applied to it
                                and its observation rows are the reset's (unrotated, :239-240), as if ssd_reset had been called with
                                the done flags as the mask.  uint8 obs only. */
    /* (1u << 5 was SSD_ROLLOUT_PIPELINED, rounds 1-2: launches of consecutive steps overlapped through per-env pass counters.
       It bought nothing once the library dispatched through its own queues -- 4.44 against 4.50 us per step at 2048 envs -- and
       was the one mode in which kernels waited on other kernels' flags: removed.  The bit is ignored.) */
    /* (1u << 6 was SSD_STEP_CHAINS, ABI 2: ssd_step dispatched like a one-step ssd_rollout_actions call.  Measured at the named
       batch -- 4096 envs -- it cost 21.7 us per call against 7.3 for the plain launch: a single launch has no chain of dependent
       launches to hide, and the fork / join cost more than two concurrent half-launches save.  Removed; the bit is ignored.) */
    SSD_ROLLOUT_AUTO = 1u << 7, /* ssd_rollout_random / ssd_rollout_actions: let the library pick the form of the call.  uint8
                                observations, index action order and n_steps >= 2 take the fused kernel (SSD_ROLLOUT_FUSED: 3.5 us per
                                4096-env step against 5.4 through the chains); anything else is dispatched as without the flag.
                                Same results either way; ssd_rollout_path() says which form ran. */
    SSD_POLICY_GREEDY = 1u << 8, /* ssd_rollout_policy only: the action is the argmax of the logits (lowest index on ties)
                                instead of a draw from the S_POLICY stream */
    SSD_OBS_F32 = 1u << 2    /* obs points at float32 [E,N,V,V,3] instead of uint8: the normalisation of map_env.py:199
                                fused into the kernel (4x the observation bytes; a separate, slower mode) */
};

/* bits of the device status word */
enum {
    SSD_ST_BAD_ACTION = 1u << 0,  /* action id outside the game's Discrete(n): KeyError in agent.action_map */
    SSD_ST_NO_SPAWN = 1u << 1,    /* not enough spawn points (assert at map_env.py:661) */
    SSD_ST_MOVE_LOOKUP = 1u << 2, /* agent_by_pos lookup miss (would be a KeyError at map_env.py:506) */
    SSD_ST_WAIT_TIMEOUT = 1u << 3 /* a rollout call's stream-side wait for the library's queues gave up (seconds: the queues' kernels
                                     never ran -- e.g. a tool that runs kernels one at a time, attached in a way the library did not
                                     notice); the call's outputs are not in place.  See SSD_AQL_SYNC below.  The condition is STICKY:
                                     the handle's next rollout call, or ssd_synchronize, drains the library's queues on the host
                                     (bounded), returns SSD_E_DEVICE once, and the handle steps through hipLaunchKernel from then
                                     on.  Until one of them has returned, the timed-out call's buffers must not be freed or reused:
                                     its launches may still be writing them */
};

typedef struct ssd_env ssd_env;

typedef struct ssd_config {
    uint32_t struct_size;        /* sizeof(ssd_config), for ABI evolution */
    int32_t game;                /* SSD_GAME_*: HarvestEnv (harvest.py:18) or CleanupEnv (cleanup.py:30) */
    int32_t height, width;       /* ascii_map shape (map_env.py:132-150) */
    const char *base_map;        /* height*width ASCII bytes, row-major, wall-closed */
    int32_t num_envs;            /* E: independent env copies held by this handle */
    int32_t num_agents;          /* N (ctor arg num_agents, map_env.py:62); 0..64 */
    int32_t view_len;            /* HARVEST_VIEW_SIZE / CLEANUP_VIEW_SIZE = 7 (harvest.py:15, cleanup.py:22) */
    int32_t beam_len;            /* ACTIONS['FIRE'] = ACTIONS['CLEAN'] = 5 (harvest.py:11, cleanup.py:11-12) */
    uint64_t seed;               /* replaces np.random.seed / random.seed */
    uint32_t env_index_base;     /* global index of env 0 of this handle (multi-GPU shards) */
    int32_t device_id;           /* HIP device ordinal */
    int32_t keep_beams;          /* 1: persist the beam overlay (map_env.py:86 beam_pos) between steps so that
                                    ssd_get_state / ssd_observe / ssd_render_full see it; 0: beams live only
                                    inside the step that draws them (they are already in that step's obs) */
    const uint8_t *color_lut;    /* 128*3 glyph -> RGB (map_env.py:24-41, cleanup.py:15-18); NULL = defaults */
    /* rand < p thresholds as ceil(p * 2^32); NULL = derived from the reference constants */
    const uint64_t *harvest_thresholds;        /* [4]  SPAWN_PROB[min(n,3)] (harvest.py:13,100) */
    const uint64_t *cleanup_apple_thresholds;  /* [potential_waste_area+1], index = current #'H' (cleanup.py:156-171) */
    const uint64_t *cleanup_waste_thresholds;  /* same indexing */
} ssd_config;

/* MapEnv.__init__ (map_env.py:62-102) + HarvestEnv/CleanupEnv.__init__ (harvest.py:20-28, cleanup.py:32-66)
 * for E env copies.  Unlike the reference constructor it does not spawn agents: call ssd_reset first. */
int ssd_create(const ssd_config *cfg, ssd_env **out);
int ssd_destroy(ssd_env *env);

/* MapEnv.reset (map_env.py:214-249) on the envs selected by env_mask (u8 [E], NULL = all; same memory
 * kind as obs).  obs may be NULL. */
int ssd_reset(ssd_env *env, const uint8_t *env_mask, void *obs, uint32_t flags, void *stream);

/* MapEnv.step (map_env.py:152-212) on every env.  obs / rew / done may be NULL. */
int ssd_step(ssd_env *env, const int32_t *actions, const uint8_t *order, void *obs, int32_t *rew,
             uint8_t *done, uint32_t flags, void *stream);

/* The random-action rollout step of rollout.py:62-70: actions are drawn on the device, uniformly over
 * Discrete(num_actions), from the ACTION stream; actions_out (i32 [E,N]) may be NULL. */
int ssd_step_random(ssd_env *env, int32_t num_actions, int32_t *actions_out, void *obs, int32_t *rew,
                    uint8_t *done, uint32_t flags, void *stream);

/* A whole random-action rollout (rollout.py:58-70: reset, then `horizon` steps of uniformly drawn actions) enqueued
 * by ONE call: n_steps launches of the step kernel, preceded by a full reset whenever (step0 + k) % reset_every == 0
 * (reset_every = 0: never).  Step k writes slot (step0 + k) % ring of obs [ring,E,N,V,V,3], rew [ring,E,N] and
 * done [ring,E,N] (ring = 1: every step overwrites the same buffers); any of the three may be NULL.  Device pointers
 * only; the call enqueues on `stream` and returns.  Exactly the launches that n_steps calls of ssd_step_random (and
 * ssd_reset) would make -- the point is the host: one library call instead of one per step keeps a launch-bound
 * rollout fed.  Envs are independent, so the library may split the batch into up to 8 env ranges ("chains") that it
 * enqueues on queues of its own, forked from and joined back into `stream`: the launches of one chain then overlap
 * the dispatch / drain gaps of the others.  Results do not depend on the number of chains.
 * How the launches are issued is the library's business and does not change what the caller sees on `stream`: up to 3
 * chains are written as AQL packets into HSA queues the library owns (one pool per device), with the observation rendering
 * of a step carried out by extra workgroups of the next step's launch where that pays; otherwise, and
 * with SSD_AQL=0 in the environment, through hipLaunchKernel on HIP streams.  Every step's outputs are in their ring slots
 * when the work enqueued by the call has completed on `stream`.
 * (An observation ring of more than 232 MB -- beyond what the device's 256-MB memory-side cache can hold next to the state -- is
 * written with non-temporal write-back stores, flushed by the call's closing release and by an agent-scope release on one launch
 * per round of the ring: a ring that thrashes that cache costs 8.1 us per 4096-env step, past it 5.8 (write-through: 7.0);
 * a single slot rewritten every step lives in it: 5.4.) */
int ssd_rollout_random(ssd_env *env, int32_t num_actions, int32_t n_steps, int32_t reset_every, int32_t step0,
                       void *obs, int32_t *rew, uint8_t *done, int32_t ring, uint32_t flags, void *stream);

/* The same call with CALLER-SUPPLIED actions -- what the reference's real callers do: env.step(policy actions)
 * (visuallizer_rllib.py:121-153; RLlib's sampler behind train_baseline.py:71-81), map_env.py:152-212 per step -- for open-loop
 * replay of recorded action sequences, action chunking, or a policy that emits several steps at once.
 *   actions i32 [action_ring,E,N] (device): step k of the call reads slot (step0 + k) % action_ring; -1 = the agent does not act.
 *           action_ring = n_steps with step0 = 0 is the plain [K,E,N] form; action_ring = 1 feeds every step the same actions.
 *   order   u8  [action_ring,E,N] (device) or NULL: per step, the agent indices in action-dict order, 0xFF-terminated, as ssd_step
 *           takes them; NULL = index order (what the map-specific kernels and the coherent chains need: an explicit order takes
 *           the general kernels).
 * Everything else -- resets, output ring, chains, flags (SSD_ROLLOUT_FUSED: one launch, the actions fetched a step ahead;
 * SSD_OBS_F32) -- as ssd_rollout_random, and dispatched the same way: the step launches' kernel arguments are static per
 * (output slot, action slot) pair, so a call enqueues 64-byte packets only (argument sets are cached by the buffers passed: reuse
 * the same action / output buffers from call to call; more than 2048 / chains distinct (slot, slot) pairs go through HIP streams).
 * The actions must be in place on `stream` before the call (the call orders itself after the stream's earlier work) and must not
 * change until the call's work has completed on `stream`.  An action outside the game's Discrete(n) sets SSD_ST_BAD_ACTION. */
int ssd_rollout_actions(ssd_env *env, const int32_t *actions, const uint8_t *order, int32_t action_ring, int32_t n_steps,
                        int32_t reset_every, int32_t step0, void *obs, int32_t *rew, uint8_t *done, int32_t ring, uint32_t flags,
                        void *stream);

/* How the last rollout call (ssd_rollout_random / ssd_rollout_actions) of the handle was
 * dispatched (a bit mask; 0 before the first call):
 *   SSD_PATH_AQL       the launches were written as AQL packets into the library's own queues (else: hipLaunchKernel)
 *   SSD_PATH_COHERENT  ... with the kernel variant that needs no cache write-back between a chain's launches
 *   SSD_PATH_SPLIT     ... and every step's observations rendered by extra workgroups of the next launch
 *   SSD_PATH_PAIRS     ... and the chains' launches took more than one step each: runs of four wherever four steps remained before
 *                      the call's end and the next reset, else of two where two remained; in calls of 256 steps or more, where the
 *                      form's kernel has a long instantiation (Harvest 16 x 38 with 5 agents), runs of eight wherever eight remained
 *                      (bits 20..23 say how long the longest was)
 *   SSD_PATH_FUSED     the call ran as the fused rollout kernel
 *   SSD_PATH_SYNC      ... with host-side waits instead of waiting kernels (a profiling tool is attached, or SSD_AQL_SYNC=1)
 *   SSD_PATH_FORKED    ... behind a fork from `stream`, which had work pending when the call came
 *   SSD_PATH_QUEUE_DROPPED  a dispatch queue of the device's pool failed its probe and was destroyed again (the rule below)
 *   bits 8..11         number of chains        bits 12..14  dispatch queues the device's pool has settled on
 *   bits 16..17        how the library found the HSA agent of the handle's HIP device: 1 PCI address, 2 UUID, 3 ordinal (cross-
 *                      checked by architecture and compute-unit count); 0: not at all -- no dispatch path of its own on this device
 *   bits 20..23        the longest run of steps one launch of the call took: 1, 2, 4 or 8 (SSD_PATH_RUN_SHIFT; 0: the call did not go
 *                      through the library's own queues)
 * So that a caller (a test, a benchmark) can tell a silent fallback from the path it meant to measure. */
enum { SSD_PATH_AQL = 1, SSD_PATH_COHERENT = 2, SSD_PATH_SPLIT = 4, SSD_PATH_FUSED = 8, SSD_PATH_SYNC = 16, SSD_PATH_QUEUE_DROPPED = 32,
       SSD_PATH_FORKED = 64, SSD_PATH_PAIRS = 128, SSD_PATH_RUN_SHIFT = 20 };
int ssd_rollout_path(const ssd_env *env);

/* Number of chains the rollout calls use: 1..8, or 0 = automatic (1 below 2048 envs, 3 from 6144 to 24576, else 2 -- and never
 * more than the device's pool has dispatch queues).
 *
 * THE QUEUE RULE.  A process has about four hardware queues before the device time-slices them, and past that EVERY kernel launch
 * of the process -- the host application's too -- takes ~30 us.  The HIP runtime takes up to GPU_MAX_HW_QUEUES of them (default 4,
 * one per stream in use), RCCL one more stream.  So: the library's pool holds SSD_AQL_QUEUES queues (1..3) if that is set; else
 * 4 - GPU_MAX_HW_QUEUES if the process holds the HIP runtime to 1, 2 or 3 queues; else 2 -- GPU_MAX_HW_QUEUES unset, 4 (the
 * runtime's own default, which it fills lazily, as streams need queues) or more, 0 or unparsable.  And whatever the rule says,
 * every queue is PROBED when it is created (first rollout call that needs it; the device is synchronised once).  The cliff is about
 * queues that are ACTIVE at the same time, so the probe is a rollout in miniature: 16 dependent one-wave dispatches on every queue
 * of the pool at once, joined through the null stream the way a rollout call is joined, timed against the pool's first queue
 * alone (MI355X: ~50 us with a hardware queue slot each, ~140 us when time-sliced); and a burst of HIP launches against its figure
 * from before the pool existed.  A queue whose arrival makes the concurrent burst more than 1.6 x (+ 10 us) slower, or the HIP burst
 * more than 2.5 x (+ 20 us) -- in two measurements, the second after the device has drained -- is destroyed again and the pool stays at the size that was fine for the life of the process
 * (SSD_PATH_QUEUE_DROPPED, bits 12..14 of ssd_rollout_path); an automatic chain count follows the smaller pool.  If already the
 * FIRST queue's burst takes more than 100 us, the process is past the cliff without the library (a host application with four
 * busy streams): the library then holds no queue at all and an automatic chain count is 1 -- the launches go to the caller's own
 * stream.  Streams the host application starts using LATER are not seen by the probe: an application that knows it will hold
 * many should set SSD_AQL_QUEUES=1 or SSD_AQL=0.
 *
 * ENVIRONMENT (read once per process; these are all the variables the product library reads):
 *   SSD_AQL=0            no dispatch queues of the library's own: every launch through hipLaunchKernel
 *   SSD_AQL_QUEUES=n     size of the pool (1..3), see above
 *   SSD_AQL_COHERENT=0   plain kernels behind agent-scope fences instead of the coherent variant
 *   SSD_AQL_SPLIT=0      every step renders its own observations
 *   SSD_AQL_SYNC=1 / 0   host-side waits instead of waiting kernels: forced / forbidden (default: on when a profiling tool
 *                        is attached -- ssd_profiler_attached() -- because such tools may run kernels one at a time)
 *   SSD_AQL_VERBOSE=1    the dispatch layer says on stderr what it set up (agent match, probe figures, fallbacks)
 *   SSD_ROLLOUT_CHAINS=n chains of the rollout calls when ssd_set_rollout_chains is 0
 *   SSD_ENVS_PER_BLOCK=n envs (waves) per workgroup, 1..16
 * Nothing here changes results.  The knobs that CAN (fence scopes, alternating geometries, forced forks) -- and SSD_AQL_PAIRS=0,
 * which keeps the split chains at one step per launch, and SSD_AQL_RUN=1..4, which caps the steps one launch takes (4: long
 * calls in runs of four, as calls below 256 steps; 8: no cap; same results; for A/B runs and tests) -- exist only in the
 * test-hook build, libssd_hip_testhooks.so (make testhooks), which the product never loads. */
int ssd_set_rollout_chains(ssd_env *env, int32_t chains);

/* 1 when a profiling / tracing tool is attached to the process (the ROCm tools' environment variables, or their libraries
 * loaded): the rollout calls then use host-side waits (SSD_PATH_SYNC).  Needs no device. */
int ssd_profiler_attached(void);

/* Observation of the current state without stepping (the per-agent part of map_env.py:189-199). */
int ssd_observe(ssd_env *env, void *obs, uint32_t flags, void *stream);

/* State access (host pointers, synchronous; any pointer may be NULL).  Mirrors what the reference's tests
 * poke directly: world_map (map_env.py:85), beam_pos (:86), Agent.pos / .orientation (agent.py:37-38).
 *   world, beam: i8 [E,H,W] ASCII (beam: 0 = none; needs keep_beams)   pos: i16 [E,N,2] (row, col)
 *   orient: u8 [E,N] 0 LEFT 1 RIGHT 2 UP 3 DOWN (key order of ORIENTATIONS, map_env.py:19-22)
 *   episode, t: u32 [E] PRNG coordinates (resets so far - 1, steps since reset) */
int ssd_get_state(ssd_env *env, int8_t *world, int8_t *beam, int16_t *pos, uint8_t *orient,
                  uint32_t *episode, uint32_t *t);
int ssd_set_state(ssd_env *env, const int8_t *world, const int8_t *beam, const int16_t *pos,
                  const uint8_t *orient, const uint32_t *episode, const uint32_t *t);

/* Cleanup only: waste_count u32 [E] = number of 'H' cells from which the last step / reset computed
 * current_apple_spawn_prob and current_waste_spawn_prob (compute_probabilities, cleanup.py:115,156-171;
 * it runs after the beams and before the spawn).  Host pointer, synchronous. */
int ssd_get_waste_count(ssd_env *env, uint32_t *waste_count);

/* MapEnv.map_to_colors() on the full grid of env e (map_env.py:316-339): rgb u8 [H,W,3], host pointer, synchronous. */
int ssd_render_full(ssd_env *env, int32_t e, uint8_t *rgb);

/* The same for envs [e_begin, e_begin + count) in one go: rgb u8 [count,H,W,3] -- the frames rollout.py:77 and
 * visuallizer_rllib.py:161 take one env at a time with map_to_colors().  Device pointer (enqueued on `stream`, returns
 * at once) or, with SSD_HOST_PTRS, host pointer (returns when the frames have arrived).  No other flag applies. */
int ssd_render_frames(ssd_env *env, int32_t e_begin, int32_t count, uint8_t *rgb, uint32_t flags, void *stream);

/* The extra members of the observation dict of an env built with return_agent_actions=True (map_env.py:201-205 step,
 * :242-246 reset, find_visible_agents :749-770; consumers run_scripts/train_moa.py:70, models/moa_model.py:216-249), for the
 * whole batch, as device tensors (or host arrays with SSD_HOST_PTRS):
 *   other_actions i64 [E,N,N-1]  row (e,i): this step's actions of the agents other than i, in the order of their ids sorted AS
 *           STRINGS, i.e. `sorted(actions.keys())` ('agent-10' < 'agent-2').  An agent absent from the action dict (action -1)
 *           contributes -1 in its place -- the reference's array is shorter then, the dict API mirror drops these entries.
 *           actions == NULL is the reset form: all zeros.  Rows whose done_mask byte (u8 [E,N], may be NULL: ssd_step's done output)
 *           is non-zero are zeros too -- the env was reset by the step launch (SSD_AUTO_RESET) or is about to be, and its
 *           observation row is a reset's.
 *   visible       i64 [E,N,N-1]  all ones: the reference tests the agent's OWN position against its window (:767).
 * Either output may be NULL.  Needs no engine state: a pure function of `actions`. */
int ssd_agent_action_obs(ssd_env *env, const int32_t *actions, const uint8_t *done_mask, int64_t *other_actions,
                         int64_t *visible, uint32_t flags, void *stream);

/* Episode length.  The reference's agents never report done; episodes end through RLlib's `horizon`
 * (run_scripts/train_baseline.py:131, train_moa.py:122).  horizon > 0: a step whose t reaches it writes
 * done = 1 for that env's agents (the caller then resets those envs, e.g. ssd_reset with done as the mask);
 * 0 (default): done stays 0. */
int ssd_set_horizon(ssd_env *env, int32_t horizon);

/* Queries. */
int ssd_potential_waste_area(const ssd_env *env);             /* cleanup.py:36-38 */
int ssd_device_status(ssd_env *env, uint32_t *status, int clear); /* synchronises the handle's device work */
int ssd_synchronize(ssd_env *env);
const char *ssd_last_error(const ssd_env *env);               /* NULL env: error of the last failed ssd_create */
int ssd_abi_version(void);

/* ======================================================================================================================
 * WATERSHED -- WatershedSeqEnv (watershedOrderedComm.py:284-423) and WatershedSeqCommEnv (:425-637) for E envs per handle,
 * one lane per env (csrc/ssd_watershed.hip).  Each step has exactly one acting agent: Seq agents 0,1,2,3 take turns; SeqComm
 * comm agents 0-3 act twice, then action agents 4-7.  An episode is 43 (Seq) / 131 (SeqComm) steps after its reset.  The
 * season -- np.random.choice(range(108)) at :69 -- is randint(draw(seed, env, episode, t = 0, SSD_S_SEASON, 0), 108), drawn
 * once per (env, episode); the reference's other global draws only gate debug prints and have no counterpart.
 *
 * Per-step outputs (device pointers, enqueued on `stream`; any may be NULL):
 *   obs    f32 [E,12]  the observing agent's curr_obs, zero-padded: [Q1,Q2,S, al1..al4 | al[agentID2real[k]], flow, comm x4]
 *                      (Seq 8 / 5 values; SeqComm comm agents 11 / 8 with no flow, action agents 12 / 9).  Every value is
 *                      exact in float32.
 *   agent  i8  [E]     whose observation the row holds (the one key of the reference's obs dict)
 *   rew    f64 [E]     the reference's reward, exactly (its float32 or float64 value widened; see SSD_WS_REW_*)
 *   done   u8  [E]     SSD_WS_* bits below
 * Actions f32 [E]: the acting agent's action.  Action agents: Box(0,1,(1,)) values, unclipped, as the reference takes them.
 * Comm agents: an integer 0..4 (Discrete(5)); anything else sets SSD_ST_BAD_ACTION and is used as given.
 * ====================================================================================================================== */
enum { SSD_WS_SEQ = 0, SSD_WS_SEQ_COMM = 1 };
enum { SSD_S_SEASON = 8 };          /* PRNG stream of the season draw (sequential_social_dilemma_games_amd/prng.py) */
enum { SSD_WS_OBS_WIDTH = 12 };
enum {
    SSD_WS_DONE_AGENT = 1u << 0,    /* done[agent] */
    SSD_WS_DONE_ALL = 1u << 1,      /* done["__all__"] (== info true_end) */
    SSD_WS_END = 1u << 2,           /* info "end" (end_episode) */
    SSD_WS_REW_INT = 1u << 3,       /* the reference's reward is the Python int 0 (no round closed yet; a comm agent's second round) */
    SSD_WS_REW_F64 = 1u << 4        /* ... is a float64 (end of episode: sum(temp) added); neither bit: a float32 */
};
enum { SSD_ST_NOT_RESET = 1u << 4 }; /* a step met an env that was never reset; it was left alone and its outputs are zero */

typedef struct ssd_ws_env ssd_ws_env;

typedef struct ssd_ws_config {
    uint32_t struct_size;           /* sizeof(ssd_ws_config) */
    int32_t variant;                /* SSD_WS_SEQ / SSD_WS_SEQ_COMM */
    int32_t num_envs;               /* E >= 1 */
    int32_t local_obs, local_rew;   /* the reference's constructor flags (return_agent_actions only shapes the dict API) */
    int32_t device_id;
    uint64_t seed;
    uint32_t env_index_base;        /* global index of env 0 of this handle */
    uint32_t reserved;
} ssd_ws_config;

/* Host-side copy of the state, SoA rows [E] / [E,n] (get: any pointer may be NULL; set: all must be given) */
typedef struct ssd_ws_state {
    uint8_t *season;                /* [E] 0..107: Q1/Q2/S = season % 3, al = all_al[season / 3] */
    uint8_t *phase;                 /* [E] current_phase after the last call, 1..4 / 1..12; 0 = never reset */
    uint8_t *wrapped;               /* [E] 1 once a round has closed this episode (f_rew / pen are no longer the int zeros) */
    uint8_t *viol;                  /* [E,6] n_viol of the last round */
    int32_t *round;                 /* [E] internal_step */
    uint32_t *episode;              /* [E] resets so far - 1 (PRNG coordinate) */
    float *hist;                    /* [E,8] action history: slot = agent id (Seq: 0..3; SeqComm: 0..7) */
    float *f_rew;                   /* [E,6] */
    float *pen;                     /* [E] */
    double *current_sums;           /* [E,4] */
    double *running_rew;            /* [E,4] rew_sum_keeper */
    float *prev_actions;            /* [E,4] the round's four action-agent actions (other_agent_actions truncates them) */
} ssd_ws_state;

int ssd_ws_create(const ssd_ws_config *cfg, ssd_ws_env **out);
int ssd_ws_destroy(ssd_ws_env *env);
/* reset() (:297-334 / :475-520) on the envs selected by env_mask (u8 [E] device, NULL = all); obs / agent rows of the other
 * envs are left alone. */
int ssd_ws_reset(ssd_ws_env *env, const uint8_t *env_mask, float *obs, int8_t *agent, void *stream);
/* step() (:336-422 / :522-637): one phase of every env.  flags: SSD_AUTO_RESET -- an env whose step sets SSD_WS_DONE_ALL
 * is reset in the same launch and its obs / agent rows are the reset's (rew and done stay the final step's). */
int ssd_ws_step(ssd_ws_env *env, const float *actions, float *obs, int8_t *agent, double *rew, uint8_t *done, uint32_t flags,
                void *stream);
/* n_steps phases in ONE launch, the state held in registers: step k reads actions slot (step0 + k) % action_ring of
 * f32 [action_ring,E] and writes slot (step0 + k) % ring of obs [ring,E,12], agent [ring,E], rew [ring,E], done [ring,E].
 * The same results as n_steps calls of ssd_ws_step with the same flags. */
int ssd_ws_rollout_actions(ssd_ws_env *env, const float *actions, int32_t action_ring, int32_t n_steps, int32_t step0, float *obs,
                           int8_t *agent, double *rew, uint8_t *done, int32_t ring, uint32_t flags, void *stream);
/* The info fields of the current state (device pointers, any may be NULL): viol u8 [E,6], true_end u8 [E], running_rew f64 [E,4],
 * temp f64 [E] (sum(temp); 0 before the end phase) and other_agent_actions i64 [E,3] of the agent whose observation the last
 * call returned (prev_actions of :355 / :548 truncated toward zero; defined for |action| < 2^63). */
int ssd_ws_info(ssd_ws_env *env, uint8_t *viol, uint8_t *true_end, double *running_rew, double *temp, int64_t *other_agent_actions,
                void *stream);
/* Host pointers, synchronous. */
int ssd_ws_get_state(ssd_ws_env *env, const ssd_ws_state *st);
int ssd_ws_set_state(ssd_ws_env *env, const ssd_ws_state *st);
int ssd_ws_device_status(ssd_ws_env *env, uint32_t *status, int clear);   /* synchronises the handle's device */
const char *ssd_ws_last_error(const ssd_ws_env *env);                   /* NULL env: error of the last failed ssd_ws_create */


/* ======================================================================================================================
 * EPISODE STATISTICS -- per-episode returns and the social-outcome metrics of Perolat et al. 2017 (efficiency, equality,
 * sustainability, peace), folded on the device from the step outputs (csrc/ssd_stats.hip).  An
 * ssd_stats object is independent of any ssd_env: it reads the rew (and done) rings the stepping calls wrote.
 *
 * A step's reward is r = a - f - 50h (agent.py:166-183, :205-222): a apple eaten, f FIRE cost, h beams that hit the agent.
 * Since |a - f| <= 1 < 25, h = floor((1 - r) / 50) and r > 0 iff (a,f,h) = (1,0,0); nothing but rew is needed.
 * Per episode of T >= 1 steps (t = 1..T) and agent i: R_i = sum r, pos_i = #{r > 0}, tsum_i = sum of t over those steps,
 * tagged_i = #{h > 0}, hits_i = sum h; C = sum_i R_i.  In float64, no contraction:
 *   efficiency      U  = (double)C / T
 *   equality        Eq = 1 - (double)G / (double)(2 N C),  G = sum_i sum_j |R_i - R_j| (int64); C = 0 gives -inf / NaN, and
 *                   the value means something only when every R_i >= 0
 *   sustainability  S  = mean over agents with pos_i > 0 of (double)tsum_i / pos_i, summed in agent order; NaN if none
 *   peace           P  = (double)(N T - sum_i tagged_i) / T
 * Every env starts at t = 0.  The step at fold index k ends env e's episode when done != NULL and done[slot,e,0] != 0
 * (the adapter's contract: done envs are reset before their next step), or when reset_every > 0 and
 * (step0 + k + 1) % reset_every == 0 (the rollout calls' full resets).  When reset_every > 0 and step0 % reset_every == 0
 * the rollout resets every env before its first step: an open episode (t > 0) is discarded and counted as truncated.
 *
 * Accumulated per env until the next drain: episodes, truncated, sum of lengths, sum of C, per agent the sums of R_i,
 * hits_i and tagged_i; per metric the float64 sum of its finite values in chronological order and their count; and the
 * record of the last episode that ended (length, R_i, the four metrics).  The results do not depend on how the steps are
 * split into folds nor on the fold's chunk length.
 * ====================================================================================================================== */
enum { SSD_STATS_KEEP = 1u << 0 };  /* ssd_stats_drain: copy out without clearing */

typedef struct ssd_stats ssd_stats;

/* num_envs 1..2^26, num_agents 1..64 (else SSD_E_INVALID); SSD_E_DEVICE without a usable HIP device. */
int ssd_stats_create(int32_t num_envs, int32_t num_agents, int32_t device_id, ssd_stats **out);
int ssd_stats_destroy(ssd_stats *st);
/* Fold n_steps steps: step k < n_steps reads slot (step0 + k) % ring of rew i32 [ring,E,N] and done u8 [ring,E,N] (device
 * pointers; done may be NULL).  n_steps <= ring, else SSD_E_INVALID.  flags: 0.  Two launches on `stream`; the object keeps
 * a scratch buffer of about n_steps * E * N bytes, grown (with a device synchronisation) when a fold needs more. */
int ssd_stats_fold(ssd_stats *st, const int32_t *rew, const uint8_t *done, int32_t ring, int32_t step0, int32_t n_steps,
                   int32_t reset_every, uint32_t flags, void *stream);
/* Steps per time chunk of the fold (0 = automatic, 64; any value up to INT32_MAX).  Changes speed only, never a result: a
 * fold clamps it to 1 .. n_steps, so a chunk above n_steps acts as n_steps (one chunk).  A fold whose chunks are too many
 * for one launch (about 2^26 waves of 64 / num_agents envs each) returns SSD_E_INVALID and says so. */
int ssd_stats_set_chunk(ssd_stats *st, int32_t steps);
/* Discard the open episode of every env with env_mask[e] != 0 (u8 [E] device, NULL = all) that has t > 0; it counts as
 * truncated. */
int ssd_stats_discard(ssd_stats *st, const uint8_t *env_mask, void *stream);
/* Copy the accumulators out (device pointers, any may be NULL) and clear them (unless SSD_STATS_KEEP):
 *   counts        i64 [E,4]    episodes, truncated, sum of lengths, sum of collective returns C
 *   agent_sums    i64 [E,3,N]  sums of R_i, hits_i, tagged_i
 *   metric_sums   f64 [E,4]    U, Eq, S, P: sums of the finite values, chronological
 *   metric_counts i64 [E,4]    how many values each sum holds
 *   last_len      i64 [E]      length of the last episode that ended (0: none since the last drain)
 *   last_ret      i64 [E,N]    its R_i
 *   last_metrics  f64 [E,4]    its U, Eq, S, P (non-finite values included) */
int ssd_stats_drain(ssd_stats *st, int64_t *counts, int64_t *agent_sums, double *metric_sums, int64_t *metric_counts,
                    int64_t *last_len, int64_t *last_ret, double *last_metrics, uint32_t flags, void *stream);
const char *ssd_stats_last_error(const ssd_stats *st);  /* NULL st: error of the last failed ssd_stats_create */

/* ======================================================================================================================
 * WATERSHED EPISODE STATISTICS -- RLlib's episode_reward_mean, policy_reward_mean and episode_len_mean and the three custom
 * metrics of the reference's Watershed launchers (social_dilemmas/envs/watershedLogging.py: violations, Equality, Utility),
 * folded INSIDE the Watershed stepping kernel while a handle is attached to the engine (csrc/ssd_ws_stats.hip, the stats
 * instances of csrc/ssd_watershed.hip).  Added after ABI 6 without a version bump: the calls are
 * additive.  Nothing is recorded per step; one drain per training iteration reads the numbers back.
 *
 * An episode of env e runs from a reset (ssd_ws_reset, or the in-kernel reset of SSD_AUTO_RESET) to the step whose done
 * carries SSD_WS_DONE_ALL: 43 steps (Seq) / 131 (SeqComm).  Per finished episode, every float64 operation one IEEE operation
 * in the stated order, no contraction:
 *   len             the number of steps
 *   reward          the float64 sum, from 0.0, in step order, of the values the rew output gets for that env
 *   agent_reward[8] the same sum over the steps whose reward was delivered to agent i (Seq: 0..3).  The receiver is the agent
 *                   whose observation the step returns; at a DONE_ALL step the variant's last agent (3 / 7), not the agent an
 *                   auto-reset then writes into `agent`
 *   total_rews[4]   running_rew as ssd_ws_info would report it at the DONE_ALL step (before an auto-reset)
 *   Utility         2 * sum(total_rews), the sum sequential from 0
 *   Equality        1 - num / Utility, num = sum over i (outer), j (inner) of |total_rews[i] - total_rews[j]|, added from 0
 *   violations      (double)S / (double)C: S the sum over the episode's steps 4, 5, ... of popcount(viol after the step),
 *                   C six times the number of those steps.  This is np.mean of the list on_episode_step builds UNDER THE
 *                   ASSUMPTION (RLlib is not part of this project) that RLlib calls on_episode_step once after every
 *                   env.step, the last included, and that last_info_for(a) is the latest info the env returned for a in this
 *                   episode: agent-0's first info comes with step 4 in both variants, and from then on its latest viol is the
 *                   env's current one.  In SeqComm the first eight counted steps hold the initial zeros, as in the reference.
 * A finished episode stays closed until the env is reset: further steps of that env are not counted.  A never-reset env is
 * ignored.  An episode is counted only from a reset made while the handle is attached.  ssd_ws_reset on an attached engine
 * first discards the open episodes of the envs it resets (truncated, if they had a step).  Observations, rewards, dones and
 * the engine state are bit-identical with and without a handle, and the results do not depend on how the steps are split
 * into calls.
 * ====================================================================================================================== */
typedef struct ssd_ws_stats ssd_ws_stats;

/* variant SSD_WS_SEQ / SSD_WS_SEQ_COMM, num_envs 1..2^26 (else SSD_E_INVALID); SSD_E_DEVICE without a usable HIP device.
 * 413 bytes of device memory per env. */
int ssd_ws_stats_create(int32_t variant, int32_t num_envs, int32_t device_id, ssd_ws_stats **out);
/* SSD_E_INVALID while an engine still holds the handle. */
int ssd_ws_stats_destroy(ssd_ws_stats *st);
/* Attach `st` to the engine (NULL detaches): from now on ssd_ws_step, ssd_ws_rollout_actions and ssd_ws_rollout_policy fold
 * into it and ssd_ws_reset opens its episodes.  SSD_E_INVALID (ssd_ws_last_error(env) says why) when the handle's variant,
 * env count or device differ from the engine's.  Host state only: nothing is launched.  A handle serves one engine at a time;
 * its open episodes are not touched (discard them when the envs were stepped in between). */
int ssd_ws_stats_attach(ssd_ws_env *env, ssd_ws_stats *st);
/* Discard the open episode of every env with env_mask[e] != 0 (u8 [E] device, NULL = all): it counts as truncated if it had a
 * step, and the env is not counted again before its next reset. */
int ssd_ws_stats_discard(ssd_ws_stats *st, const uint8_t *env_mask, void *stream);
/* Copy the per-env accumulators since the last drain out (device pointers, any may be NULL) and clear them (unless
 * SSD_STATS_KEEP).  Metrics in the order violations, Equality, Utility.
 *   counts          i64 [E,3]  episodes, truncated, sum of lengths
 *   reward_sum      f64 [E]    sum of `reward`, in episode order from 0.0 (as every float64 sum here)
 *   agent_sums      f64 [E,8]  sums of agent_reward
 *   metric_sums     f64 [E,3]  sums of the finite values
 *   metric_counts   i64 [E,3]  how many values each sum holds
 *   metric_min/max  f64 [E,3]  over the same values (+inf / -inf where there is none)
 *   last_len        i64 [E]    the last episode that finished (0: none since the last drain) ...
 *   last_reward     f64 [E]
 *   last_agent      f64 [E,8]
 *   last_total_rews f64 [E,4]
 *   last_metrics    f64 [E,3]  ... non-finite values included */
int ssd_ws_stats_drain(ssd_ws_stats *st, int64_t *counts, double *reward_sum, double *agent_sums, double *metric_sums,
                       int64_t *metric_counts, double *metric_min, double *metric_max, int64_t *last_len, double *last_reward,
                       double *last_agent, double *last_total_rews, double *last_metrics, uint32_t flags, void *stream);
const char *ssd_ws_stats_last_error(const ssd_ws_stats *st);  /* NULL st: error of the last failed ssd_ws_stats_create */

/* ======================================================================================================================
 * POLICY ROLLOUTS -- the conv-FC policy network of models/conv_to_fc_net.py:1-51 (Jaques et al. 2019) run on the device and
 * interleaved with the step kernel, so that a closed-loop rollout (observe, act, step: visuallizer_rllib.py:121-153) is
 * enqueued by one call (csrc/ssd_policy.hip).  Exact float32 throughout.
 *
 * The network, per weight set and observation x = float32((u8 - 128) / 255) of shape [15,15,3] (view_len 7 only):
 *   conv   6 filters 3x3, stride 1, no padding, ReLU           -> [13,13,6]
 *   flatten in (row, col, channel) order (TF's flatten of NHWC) -> 1014
 *   fc1    1014 -> 32, ReLU      fc2  32 -> 32, ReLU            (the trunk)
 *   logits 32 -> A               value 32 -> 1                  (both on fc2's output)
 * A weight buffer holds P sets back to back, each SSD_POL_SET_FLOATS(A) floats (a multiple of 64), in this layout (float
 * offsets within a set; every matrix is [in][out], the layout of a TF checkpoint's kernels):
 *   conv_w   [3][3][3][6]  (kh, kw, c_in, c_out)      conv_b   [6]
 *   fc1_w    [1014][32]                               fc1_b    [32]
 *   fc2_w    [32][32]                                 fc2_b    [32]
 *   value_w  [32]                                     value_b  [1]    (then 3 floats of padding)
 *   logits_w [32][A]                                  logits_b [A]    (then padding up to the set stride)
 * Agent i of an env uses set i when P = N and set 0 when P = 1 (train_baseline.py:87-96: one policy per agent).
 *
 * Sampling (ssd_rollout_policy without SSD_POLICY_GREEDY): for the state an action is taken in, with (episode, t) as
 * ssd_get_state reports them, draw = H(seed, env_index_base + e, episode, t, SSD_S_POLICY, i) and u = (draw >> 8) * 2^-24.
 * With m = max_a logits[a], e_a = expf(logits[a] - m), s = the float32 sum of e_a in index order and c_a the running float32
 * sum of e_a / s in index order, the action is the first a with u < c_a, else A - 1.  SSD_POLICY_GREEDY: the first a with
 * the largest logit.  logp = logits[a] - (m + logf(s)), float32.
 * ====================================================================================================================== */
enum { SSD_S_POLICY = 9 };          /* PRNG stream of the policy's action draw (sequential_social_dilemma_games_amd/prng.py) */
enum {
    SSD_POL_VIEW = 15, SSD_POL_CONV_OUT = 13, SSD_POL_FILTERS = 6, SSD_POL_HIDDEN = 32, SSD_POL_FLAT = 1014, SSD_POL_MAX_ACTIONS = 15,
    SSD_POL_CONV_W = 0,             /* 162 */
    SSD_POL_CONV_B = 162,           /* 6 */
    SSD_POL_FC1_W = 168,            /* 1014 * 32 */
    SSD_POL_FC1_B = 32616,          /* 32 */
    SSD_POL_FC2_W = 32648,          /* 32 * 32 */
    SSD_POL_FC2_B = 33672,          /* 32 */
    SSD_POL_VALUE_W = 33704,        /* 32 */
    SSD_POL_VALUE_B = 33736,        /* 1 */
    SSD_POL_LOGITS_W = 33740        /* 32 * A, then logits_b [A] at SSD_POL_LOGITS_W + 32 * A */
};
#define SSD_POL_LOGITS_B(A) (SSD_POL_LOGITS_W + 32 * (A))
#define SSD_POL_SET_FLOATS(A) ((SSD_POL_LOGITS_W + 33 * (A) + 63) / 64 * 64)

/* The forward pass alone: obs u8 [B,N,15,15,3] -> logits f32 [B,N,A] and value f32 [B,N] (either may be NULL), device pointers
 * on device_id, enqueued on `stream`.  weights: P sets as above (P = 1 or N), 4-byte aligned; 1 <= A <= 15; 1 <= N <= 64.
 * flags: 0.  Bad arguments: SSD_E_INVALID before anything is launched (ssd_policy_last_error says why). */
int ssd_policy_forward(const float *weights, int32_t num_sets, int32_t num_actions, const uint8_t *obs, int32_t batch,
                       int32_t num_agents, float *logits, float *value, int32_t device_id, uint32_t flags, void *stream);
const char *ssd_policy_last_error(void);   /* the calling thread's last ssd_policy_forward error */

/* A closed-loop rollout of n_steps steps in one call (device pointers, enqueued on `stream`, no host synchronisation).  A is the
 * game's Discrete(n) (8 Harvest, 9 Cleanup); the handle's view_len must be 7.  Step k:
 *   1. the policy runs on the current observation: obs_in u8 [E,N,15,15,3] for k = 0, else slot (step0 + k - 1) % ring of obs;
 *   2. it writes actions i32, logp f32, value f32 (and logits f32 [.., A]) into slot s = (step0 + k) % ring of
 *      actions [ring,E,N], logp [ring,E,N], value [ring,E,N], logits [ring,E,N,A];
 *   3. the step runs with those actions in index order and SSD_AUTO_RESET (horizon of ssd_set_horizon), writing obs u8
 *      [ring,E,N,15,15,3], rew i32 [ring,E,N] and done u8 [ring,E,N] into slot s.
 * After the last step last_value f32 [E,N] holds the value of the final observation (the bootstrap of GAE).  obs and actions
 * are required; logp, value, logits, rew, done and last_value may be NULL.  ring >= 1, n_steps >= 1, step0 >= 0.
 * flags: SSD_POLICY_GREEDY or 0.  The same results as n_steps rounds of (ssd_policy_forward, the sampling above,
 * ssd_step(..., SSD_AUTO_RESET)): a pure function of (state, weights, seed), whatever the ring length or the split into calls.
 * Two hipLaunchKernel launches per step on `stream` (plus one for last_value). */
int ssd_rollout_policy(ssd_env *env, const float *weights, int32_t num_sets, const uint8_t *obs_in, int32_t n_steps, int32_t step0,
                       uint8_t *obs, int32_t *actions, float *logp, float *value, float *logits, int32_t *rew, uint8_t *done,
                       int32_t ring, float *last_value, uint32_t flags, void *stream);

/* ======================================================================================================================
 * RECURRENT POLICY ROLLOUTS -- the policy the reference's Harvest / Cleanup baseline trains (run_scripts/train_baseline.py:146-147,
 * "use_lstm": True): the trunk above (conv, fc1, fc2) wrapped by RLlib 0.7.6's LSTM, the model of Jaques et al. 2019
 * (csrc/ssd_policy_lstm.hip).  Exact float32 throughout.
 *
 * Per weight set, with x = fc2's output (32 floats, after its ReLU) and a state (c, h) of C cells, C = 64, 128 or 256:
 *   z = [x, h] @ lstm_w + lstm_b               lstm_w [32 + C][4C] (the x rows first, then the h rows), lstm_b [4C]
 *   i, j, f, o = the column blocks z[0:C], z[C:2C], z[2C:3C], z[3C:4C]     (TF's LSTMCell / BasicLSTMCell order)
 *   c' = sigmoid(f + 1) * c + sigmoid(i) * tanh(j)                      (forget bias 1.0; no peepholes, no projection)
 *   h' = sigmoid(o) * tanh(c')
 *   logits = h' @ logits_w + logits_b          value = h' @ value_w + value_b      (both heads on the LSTM output)
 * The trunk's own logits and value heads are not used (RLlib's wrapper reads the inner model's last layer).  A state is f32
 * [.., 2, C]: c at index 0, h at index 1 (RLlib's state_init order).
 * Start rule: the state a step uses is zero where the env is at the start of an episode -- the env's t is 0 in a rollout (after
 * a reset, a masked reset or an automatic reset), starts[row] != 0 in the forward.  Such a row of the state is never read.
 * A weight set holds the trunk at SSD_POL_CONV_W ... SSD_POL_FC2_B, then the blocks below, each on a 64-float boundary (every
 * matrix [in][out]); a buffer holds P sets, set p at p * SSD_LSTM_SET_FLOATS(C, A):
 *   lstm_w [32 + C][4C]   lstm_b [4C]   value_w [C]   value_b [1]   logits_w [C][A]   logits_b [A]
 * ====================================================================================================================== */
enum { SSD_LSTM_W = 33728, SSD_LSTM_X = 32, SSD_LSTM_MAX_CELLS = 256 };
#define SSD_LSTM_ALIGN(n) (((n) + 63) / 64 * 64)
#define SSD_LSTM_B(C) SSD_LSTM_ALIGN(SSD_LSTM_W + (32 + (C)) * 4 * (C))
#define SSD_LSTM_VALUE_W(C) SSD_LSTM_ALIGN(SSD_LSTM_B(C) + 4 * (C))
#define SSD_LSTM_VALUE_B(C) SSD_LSTM_ALIGN(SSD_LSTM_VALUE_W(C) + (C))
#define SSD_LSTM_LOGITS_W(C) SSD_LSTM_ALIGN(SSD_LSTM_VALUE_B(C) + 1)
#define SSD_LSTM_LOGITS_B(C, A) SSD_LSTM_ALIGN(SSD_LSTM_LOGITS_W(C) + (C) * (A))
#define SSD_LSTM_SET_FLOATS(C, A) SSD_LSTM_ALIGN(SSD_LSTM_LOGITS_B(C, A) + (A))

/* The recurrent forward pass alone (device pointers on device_id, enqueued on `stream`): obs u8 [B,N,15,15,3] and state_in f32
 * [B,N,2,C] -> features f32 [B,N,32] (fc2's output; caller-supplied scratch, required), state_out f32 [B,N,2,C], logits f32
 * [B,N,A], value f32 [B,N].  state_out, logits and value may be NULL; state_out may equal state_in (updated in place) but must
 * not overlap it otherwise.  starts: u8 [B,N] or NULL (no row starts).  weights: P sets as above (P = 1 or N), 4-byte
 * aligned.  flags: 0.  Bad arguments: SSD_E_INVALID before anything is launched (ssd_policy_last_error says why). */
int ssd_policy_lstm_forward(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size, const uint8_t *obs,
                            const float *state_in, const uint8_t *starts, int32_t batch, int32_t num_agents, float *features,
                            float *state_out, float *logits, float *value, int32_t device_id, uint32_t flags, void *stream);

/* ssd_rollout_policy with the recurrent network: the same rings, sampling contract, flags and step order, and besides
 *   state f32 [E,N,2,C]: the carried state, read and updated in place by every step (zero at every episode start, above);
 *   state_ring f32 [S,E,N,2,C] or NULL: for call-relative k = 0, state_every, 2 state_every, ... slot k / state_every receives
 *     the state step k used (after the start rule).  state_every >= 1 and S >= ceil(n_steps / state_every);
 *   features f32 [E,N,32]: caller-supplied scratch (the call allocates nothing and does not synchronise).
 * last_value is the value of the final observation under the final state; that pass leaves the carried state as it is.
 * Three hipLaunchKernel launches per step on `stream` (plus two for last_value). */
int ssd_rollout_policy_lstm(ssd_env *env, const float *weights, int32_t num_sets, int32_t cell_size, const uint8_t *obs_in,
                            int32_t n_steps, int32_t step0, float *state, float *state_ring, int32_t state_ring_len,
                            int32_t state_every, float *features, uint8_t *obs, int32_t *actions, float *logp, float *value,
                            float *logits, int32_t *rew, uint8_t *done, int32_t ring, float *last_value, uint32_t flags,
                            void *stream);

/* ======================================================================================================================
 * MOA POLICY ROLLOUTS -- the causal-influence policy of run_scripts/train_moa.py:64-155 (MOA_LSTM, models/moa_model.py:121-311)
 * with the social-influence reward of Jaques et al. 2019 (algorithms/common_funcs.py:134-195), on the device
 * (csrc/ssd_policy_moa.hip).  Exact float32 throughout.  N agents, 2 <= N <= SSD_MOA_MAX_AGENTS.
 *
 * Per weight set, with x the normalised observation of the trunk above (view_len 7):
 *   conv at SSD_POL_CONV_W / SSD_POL_CONV_B, ReLU, flatten (row, col, channel) to 1014 -- the trunk's conv, run once;
 *   two FC stacks on it, s = 0 (actions) and s = 1 (MOA): y_s = tanh(tanh(x @ fc1_w + fc1_b) @ fc2_w + fc2_b), 32 floats
 *     (RLlib's default fcnet_activation "tanh": train_moa.py:138-144 does not set it);
 *   Keras LSTMs of C cells, C = 64, 128 or 256: z = in @ kernel + h @ recurrent_kernel + bias, gate blocks (i, f, c, o):
 *     c' = sigmoid(f) * c + sigmoid(i) * tanh(c~),  h' = sigmoid(o) * tanh(c')   (no +1 on f at run time; not RLlib's cell)
 *   actions LSTM on y_0: logits = h1' @ logits_w + logits_b, value = h1' @ value_w + value_b;
 *   MOA LSTM on in = [y_1, the N previous actions as floats, own first] -> pred = h2' @ pred_w + pred_b, read as [N-1][A].
 * A state is f32 [.., 4, C] = (h1, c1, h2, c2) (moa_model.py:114-118).  The previous actions of row (e, i) are agent i's, then
 * the other agents' in the order of their ids sorted AS STRINGS ('agent-10' < 'agent-2', as ssd_agent_action_obs); the j of
 * pred [j][a] is the j-th of those others.  Start rule: where the env's t is 0 (rollouts) or starts[row] != 0 (the forward),
 * the state and the previous-action vector of the row are zero; they are selected, never read.
 * Counterfactuals: with z the MOA gates of the true input and a_prev the own previous action (0 at a start),
 * cf[a] = pred of the cell update from z + (a - a_prev) * kernel[32] (kernel row 32 is the own-action input; a = 0 .. A-1),
 * in float32 as written: (z + bias) + (float)(a - a_prev) * row.  moa_logits IS cf[a_prev] (bitwise); the state advances with
 * the true input only.
 * Influence of row (e, i), with a_t the action chosen from this step's logits (common_funcs.py:140-157) and pi their softmax:
 *   for each other agent j: log p = log_softmax(cf[a_t][j]), log q = logsumexp over a of (log pi(a) + log_softmax(cf[a][j]));
 *   KL_j = sum over k with p_k != 0 of p_k (log p_k - log q_k);  influence = clip(sum_j KL_j, -clip, clip).
 * A non-finite sum gives 0 for that row (the reference zeroes the whole trajectory, common_funcs.py:62-66).  The visibility
 * factor is 1 (visible agents are all ones, above) and is not read.  The shaped reward is rew + w * influence.
 *
 * Weight set (floats, every block on a 64-float boundary, matrices [in][out]); a buffer holds P = 1 or N sets, set p at
 * p * SSD_MOA_SET_FLOATS(C, A, N).  Stack s's fc1_w [1014][32], fc1_b, fc2_w [32][32], fc2_b sit at SSD_MOA_FC(s) + the trunk's
 * relative offsets (SSD_POL_FC1_W ... SSD_POL_FC2_B minus SSD_POL_FC1_W).  Each (kernel, recurrent_kernel) pair is one matrix
 * with the input rows first: lstm [32 + C][4C]; moa [48 + C][4C] whose rows 32 + N .. 47 are zero.
 * ====================================================================================================================== */
enum { SSD_MOA_FC = 33728, SSD_MOA_FC_STRIDE = 33536, SSD_MOA_X = 32, SSD_MOA_XM = 48, SSD_MOA_MAX_AGENTS = 16 };
#define SSD_MOA_ALIGN(n) (((n) + 63) / 64 * 64)
#define SSD_MOA_FC1_W(s) (SSD_MOA_FC + (s) * SSD_MOA_FC_STRIDE)
#define SSD_MOA_FC1_B(s) (SSD_MOA_FC1_W(s) + (SSD_POL_FC1_B - SSD_POL_FC1_W))
#define SSD_MOA_FC2_W(s) (SSD_MOA_FC1_W(s) + (SSD_POL_FC2_W - SSD_POL_FC1_W))
#define SSD_MOA_FC2_B(s) (SSD_MOA_FC1_W(s) + (SSD_POL_FC2_B - SSD_POL_FC1_W))
#define SSD_MOA_LSTM_W(C) (SSD_MOA_FC + 2 * SSD_MOA_FC_STRIDE)
#define SSD_MOA_LSTM_B(C) SSD_MOA_ALIGN(SSD_MOA_LSTM_W(C) + (32 + (C)) * 4 * (C))
#define SSD_MOA_VALUE_W(C) SSD_MOA_ALIGN(SSD_MOA_LSTM_B(C) + 4 * (C))
#define SSD_MOA_VALUE_B(C) SSD_MOA_ALIGN(SSD_MOA_VALUE_W(C) + (C))
#define SSD_MOA_LOGITS_W(C) SSD_MOA_ALIGN(SSD_MOA_VALUE_B(C) + 1)
#define SSD_MOA_LOGITS_B(C, A) SSD_MOA_ALIGN(SSD_MOA_LOGITS_W(C) + (C) * (A))
#define SSD_MOA_MW(C, A) SSD_MOA_ALIGN(SSD_MOA_LOGITS_B(C, A) + (A))
#define SSD_MOA_MB(C, A) SSD_MOA_ALIGN(SSD_MOA_MW(C, A) + (SSD_MOA_XM + (C)) * 4 * (C))
#define SSD_MOA_PRED_W(C, A) SSD_MOA_ALIGN(SSD_MOA_MB(C, A) + 4 * (C))
#define SSD_MOA_PRED_B(C, A, N) SSD_MOA_ALIGN(SSD_MOA_PRED_W(C, A) + (C) * ((N) - 1) * (A))
#define SSD_MOA_SET_FLOATS(C, A, N) SSD_MOA_ALIGN(SSD_MOA_PRED_B(C, A, N) + ((N) - 1) * (A))
/* Caller scratch of both calls, in floats, for rows = B * N (or E * N): features [rows][2][32], then logits [rows][16] (this
 * step's, for the MOA cell), then two i32 [rows] buffers of joint actions (the rollout's ping-pong). */
#define SSD_MOA_SCRATCH_FLOATS(rows) (82 * (size_t)(rows))

/* The MOA forward pass alone (device pointers on device_id, enqueued on `stream`): obs u8 [B,N,15,15,3], prev_actions i32 [B,N]
 * (the previous joint action of each row's env, by agent index), state_in f32 [B,N,4,C] and starts u8 [B,N] or NULL ->
 * state_out f32 [B,N,4,C], logits f32 [B,N,A], value f32 [B,N], moa_logits f32 [B,N,N-1,A], cf_logits f32 [B,N,A,N-1,A].
 * Every output may be NULL; state_out may equal state_in (in place) but must not overlap it otherwise.  With actions i32
 * [B,N] (this step's, as chosen from these logits) it also writes influence f32 [B,N] with the given clip (finite, >= 0).
 * scratch: SSD_MOA_SCRATCH_FLOATS(B * N) floats, required.  weights: P sets (P = 1 or N), 4-byte aligned.  flags: 0.
 * Bad arguments: SSD_E_INVALID before anything is launched (ssd_policy_last_error says why). */
int ssd_policy_moa_forward(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size, const uint8_t *obs,
                           const int32_t *prev_actions, const float *state_in, const uint8_t *starts, int32_t batch,
                           int32_t num_agents, float *scratch, float *state_out, float *logits, float *value, float *moa_logits,
                           float *cf_logits, const int32_t *actions, float *influence, float influence_clip, int32_t device_id,
                           uint32_t flags, void *stream);

/* ssd_rollout_policy_lstm with the MOA network: the same rings, sampling contract, flags and step order, state [E,N,4,C] and
 * state ring (of the 4-row state), and besides
 *   prev_actions i32 [E,N]: the carried previous joint action, read by step 0 and left holding the last step's actions;
 *   prev_actions_ring i32 [R,E,N] or NULL: slot (step0 + k) % R receives what step k's MOA read (zero where t was 0);
 *   influence f32 [R,E,N] or NULL: slot (step0 + k) % R receives step k's influence (clip: influence_clip, finite, >= 0);
 *   scratch: SSD_MOA_SCRATCH_FLOATS(E * N) floats (the call allocates nothing and does not synchronise).
 * Four hipLaunchKernel launches per step on `stream` (trunk, actions cell, MOA cell with the influence, env step), one
 * device-to-device copy of the joint action at the end, and two launches for last_value, which leaves the state alone. */
int ssd_rollout_policy_moa(ssd_env *env, const float *weights, int32_t num_sets, int32_t cell_size, const uint8_t *obs_in,
                           int32_t n_steps, int32_t step0, float *state, float *state_ring, int32_t state_ring_len,
                           int32_t state_every, int32_t *prev_actions, int32_t *prev_actions_ring, float *influence,
                           float influence_clip, float *scratch, uint8_t *obs, int32_t *actions, float *logp, float *value,
                           float *logits, int32_t *rew, uint8_t *done, int32_t ring, float *last_value, uint32_t flags,
                           void *stream);

/* ======================================================================================================================
 * WATERSHED POLICY ROLLOUTS -- LSTMFCNet (models/watershed_nets.py:94-177), the policy of every agent of the Watershed
 * baselines (run_scripts/train_watershed_baseline.py:119,162, train_watershed_comm_baseline.py:97-127) and of the comm
 * agents of train_watershed_comm_moa.py:115,124, on the device between the phases of the Watershed engine above
 * (csrc/ssd_ws_policy.hip).  Exact float32 throughout, every sum in a fixed order: a sum over k is
 * s = 0, s = fmaf(in[k], w[k][j], s) for k ascending, then s + bias.
 *
 * One weight set per agent id: num_sets = 4 for SSD_WS_SEQ, 8 for SSD_WS_SEQ_COMM.  The row that acts uses the set of its
 * agent.  Per set, with x0 the engine's observation row f32 [12] (zero-padded: rows of dense0_w beyond the agent's
 * observation length meet zeros) and a state (h, c) of C cells, C = 64, 128 or 256:
 *   d0 = relu(x0 @ dense0_w + dense0_b)   [12][16]        d1 = relu(d0 @ dense1_w + dense1_b)   [16][16]
 *   z  = [d1, h] @ lstm_w + lstm_b        lstm_w [16 + C][4C]: Keras' kernel rows, then its recurrent_kernel rows
 *   i, f, g, o = the column blocks z[0:C], z[C:2C], z[2C:3C], z[3C:4C]          (Keras' order; no forget bias at run time)
 *   c' = sigmoid(f) * c + sigmoid(i) * tanh(g)            h' = sigmoid(o) * tanh(c')
 *   dist = h' @ out_w + out_b   [C][5]                    value = h' @ value_w + value_b   [C]
 * sigmoid(x) = 1 / (1 + expf(-x)).  A state is f32 [.., 2, C]: h at index 0, c at index 1 (Keras' order).
 * Weight set (floats, every block on a 64-float boundary, matrices [in][out]); set p at p * SSD_WSP_SET_FLOATS(C):
 *   dense0_w [12][16]  dense0_b [16]  dense1_w [16][16]  dense1_b [16]  lstm_w [16 + C][4C]  lstm_b [4C]  out_w [C][5]
 *   out_b [5]  value_w [C]  value_b [1]
 *
 * The action distribution follows from (variant, agent id):
 *   comm agents (SSD_WS_SEQ_COMM ids 0-3): Categorical over dist[0:5] by the POLICY ROLLOUTS rule above (the first a with
 *     u < the running float32 softmax sum; greedy: the first maximal logit; logp = l_a - (m + logf(s))); the action is
 *     recorded as a float;
 *   action agents (SSD_WS_SEQ ids 0-3, SSD_WS_SEQ_COMM ids 4-7): RLlib's DiagGaussian, mean = dist[0], log_std = dist[1]
 *     (dist[2:5] are computed and written, and unused): std = expf(log_std), a = mean + std * n,
 *     z = (a - mean) / std, logp = ((-0.5f * (z * z)) - log_std) - 0.9189385f.  Greedy: n = 0, i.e. a = mean (bitwise).
 *     The rings record the unclipped a; the env steps with fminf(fmaxf(a, 0), 1) (RLlib's clip_actions; a NaN gives 0).
 * Draws: with (episode, t) of the state the action is taken in, t = round * P + phase - 1 (P = 4 / 12; round and phase as
 * ssd_ws_get_state reports them; 0 for the first action after a reset) and i the acting agent's id,
 *   d1 = H(seed, env_index_base + e, episode, t, SSD_S_POLICY, i),  d2 = H(.., i + 16),
 *   categorical: u = (d1 >> 8) * 2^-24;
 *   Gaussian: u1 = ((d1 >> 8) + 1) * 2^-24 in (0, 1], u2 = (d2 >> 8) * 2^-24, n = sqrtf(-2 * logf(u1)) * cosf(6.2831855f * u2).
 * Start rule: the state an agent uses at its first action of an episode is zero, and such a row is never read.  In a
 * rollout that is round == 0, and for SSD_WS_SEQ_COMM besides phase <= 4 or phase >= 9 (phases 5-8 are the comm agents'
 * second message); in the forward call it is starts[row] != 0.
 * ====================================================================================================================== */
enum { SSD_WSP_X = 16, SSD_WSP_OUT = 5, SSD_WSP_D0_W = 0, SSD_WSP_D0_B = 192, SSD_WSP_D1_W = 256, SSD_WSP_D1_B = 512, SSD_WSP_LSTM_W = 576 };
#define SSD_WSP_ALIGN(n) (((n) + 63) / 64 * 64)
#define SSD_WSP_LSTM_B(C) SSD_WSP_ALIGN(SSD_WSP_LSTM_W + (16 + (C)) * 4 * (C))
#define SSD_WSP_OUT_W(C) SSD_WSP_ALIGN(SSD_WSP_LSTM_B(C) + 4 * (C))
#define SSD_WSP_OUT_B(C) SSD_WSP_ALIGN(SSD_WSP_OUT_W(C) + 5 * (C))
#define SSD_WSP_VALUE_W(C) SSD_WSP_ALIGN(SSD_WSP_OUT_B(C) + 5)
#define SSD_WSP_VALUE_B(C) SSD_WSP_ALIGN(SSD_WSP_VALUE_W(C) + (C))
#define SSD_WSP_SET_FLOATS(C) SSD_WSP_ALIGN(SSD_WSP_VALUE_B(C) + 1)

/* The forward pass alone (device pointers on device_id, enqueued on `stream`): obs f32 [B,12], agent i8 [B] (row b uses weight
 * set agent[b]; ids mix freely) and state_in f32 [B,2,C] -> state_out f32 [B,2,C], dist f32 [B,5], value f32 [B].  state_out,
 * dist and value may be NULL; state_out may equal state_in (in place) but must not overlap it otherwise.  starts: u8 [B] or
 * NULL (no row starts).  A row whose agent is outside 0 .. num_sets - 1 gets zero outputs and its state_out row is not written.
 * weights: num_sets sets as above, 4-byte aligned; variant fixes num_sets.  flags: 0.  Bad arguments: SSD_E_INVALID before
 * anything is launched (ssd_policy_last_error says why). */
int ssd_ws_policy_forward(const float *weights, int32_t num_sets, int32_t cell_size, int32_t variant, const float *obs,
                          const int8_t *agent, const float *state_in, const uint8_t *starts, int32_t batch, float *state_out,
                          float *dist, float *value, int32_t device_id, uint32_t flags, void *stream);

/* A closed-loop rollout of n_steps phases in one call (device pointers, enqueued on `stream`; the call allocates nothing and
 * never synchronises).  Step k:
 *   1. the policy reads the current observation and its agent: obs_in f32 [E,12] / agent_in i8 [E] (what the engine last
 *      returned) for k = 0, else slot (step0 + k - 1) % ring of obs / agent.  It uses and updates row [e, agent] of
 *      state f32 [E,NA,2,C] (NA = num_sets) and leaves the other agents' rows as they are;
 *   2. it writes actor i8 (= that agent), actions f32, logp f32, value f32 (all [ring,E]), dist f32 [ring,E,5] and
 *      state_ring f32 [ring,E,2,C] (the state it used, after the start rule) into slot s = (step0 + k) % ring, and the
 *      clipped action into scratch f32 [E] (caller-supplied);
 *   3. one phase of the env with scratch as its actions and SSD_AUTO_RESET writes obs f32 [ring,E,12], agent i8 [ring,E],
 *      rew f64 [ring,E] and done u8 [ring,E] into slot s, exactly as the step call of the Watershed section does.
 * After the last step last_value f32 [E] holds the value of the final observation under its observer's state; that pass
 * leaves `state` alone.  obs, agent and actions are required (obs rows 16-byte aligned); state_ring, rew, done, actor, logp,
 * value, dist and last_value may be NULL.  A never-reset env (phase 0) is left alone as by SSD_ST_NOT_RESET: zero outputs,
 * state untouched.  ring >= 1, n_steps >= 1, step0 >= 0.  flags: SSD_POLICY_GREEDY or 0.  A pure function of (env state,
 * policy state, weights, seed), whatever the ring length or the split into calls.  Bad arguments: SSD_E_INVALID before
 * anything is launched, engine and state untouched (ssd_ws_last_error says why).  Two launches per step on `stream`, one more
 * for last_value. */
int ssd_ws_rollout_policy(ssd_ws_env *env, const float *weights, int32_t num_sets, int32_t cell_size, const float *obs_in,
                          const int8_t *agent_in, int32_t n_steps, int32_t step0, float *state, float *state_ring, float *scratch,
                          float *obs, int8_t *agent, double *rew, uint8_t *done, int8_t *actor, float *actions, float *logp,
                          float *value, float *dist, int32_t ring, float *last_value, uint32_t flags, void *stream);

/* ======================================================================================================================
 * ADVANTAGES AND VALUE TARGETS -- what every trainer does between sampling and its loss (RLlib's compute_advantages:
 * generalised advantage estimation for PPO, discounted returns for A3C), computed on the device from the [ring, ...] rings
 * of the policy rollouts above (csrc/ssd_gae.hip).  Added after ABI 6 without a version bump: the
 * call is additive.
 *
 * Lanes are trajectories: L = lanes (E * N for the rollouts' rings), lane l is column l of the [ring, L] rings.  Row k of a
 * call is slot (step0 + k) % ring.  Every operation is one IEEE float64 operation in the order written here (no fused
 * multiply-add); the two results are rounded to float32 once, when they are stored.  gl = gamma * lambda, formed once.
 * Walking k = n_steps - 1 ... 0, per lane:
 *   r      = (double)rew[k], or (double)rew[k] + bonus_weight * (double)bonus[k] with a bonus (multiply, then add)
 *   v_next = 0.0 if done[k] != 0; else (double)last_value for k = n_steps - 1 and (double)value[k + 1] otherwise
 *   carry  = 0.0 if done[k] != 0 or k = n_steps - 1; else the running A of row k + 1
 * SSD_ADV_GAE | SSD_ADV_CRITIC:   delta = (r + gamma * v_next) - (double)value[k];  A = delta + gl * carry;
 *                                 advantages[k] = (float)A;  value_targets[k] = (float)(A + (double)value[k])
 * SSD_ADV_CRITIC:                 G = r + gamma * G_next, where G_next is v_next where the carry is cut (a done row or the
 *                                 last row) and the running G of row k + 1 otherwise;
 *                                 advantages[k] = (float)(G - (double)value[k]);  value_targets[k] = (float)G
 * 0:                              the same G;  advantages[k] = (float)G;  value_targets[k] = 0;  value may be NULL
 * done[k] != 0 says that the episode ended with step k and row k + 1 belongs to the next one (what the rollouts record at
 * the horizon); a fragment that ends without one is bootstrapped with last_value.  NULL done: no episode ends.  NULL
 * last_value: 0.  NULL bonus: none (bonus_weight is not read).  Inputs are assumed finite.
 *
 * rew i32, bonus f32, value f32, done u8, advantages f32 and value_targets f32 are [ring, L]; last_value f32 is [L]; device
 * pointers on device_id.  One launch on `stream`, no allocation, no synchronisation.  SSD_E_INVALID before any device call
 * (ssd_advantages_last_error says why) for lanes < 1, ring < 1, n_steps < 1 or > ring, step0 < 0, an unknown flag, the first
 * flag without the second, a missing rew, output or (with the critic) value pointer, a gamma, lambda or (with a bonus)
 * bonus_weight that is not finite; SSD_E_DEVICE without a usable HIP device.
 * ====================================================================================================================== */
enum {
    SSD_ADV_GAE = 1u << 0,      /* generalised advantage estimation (needs SSD_ADV_CRITIC); else discounted returns */
    SSD_ADV_CRITIC = 1u << 1    /* value is the critic's prediction: a baseline for the returns, the target of value_targets */
};
int ssd_advantages(const int32_t *rew, const float *bonus, double bonus_weight, const float *value, const uint8_t *done,
                   const float *last_value, int32_t lanes, int32_t ring, int32_t step0, int32_t n_steps, double gamma,
                   double lambda, uint32_t flags, float *advantages, float *value_targets, int32_t device_id, void *stream);
const char *ssd_advantages_last_error(void);   /* the calling thread's last ssd_advantages error */

/* ======================================================================================================================
 * PPO LOSS AND GRADIENTS -- the learner's half of the loop for the conv-FC policy: RLlib 0.7.6's PPOLoss with use_gae=True
 * (what algorithms/ppo_causal.py:53-72 builds) on a sampled fragment, its statistics and the gradient of every parameter, in
 * one call (csrc/ssd_policy_grad.hip).  Added after ABI 6 without a version bump: the call is additive.
 *
 * Network: that of ssd_policy_forward above, the same packed weight layout, P = 1 or P = N sets, A <= 15, view 15.
 *
 * Rows.  A fragment is K x E x N rows (n_steps, num_envs, num_agents); every per-row array below is [K,E,N] (behaviour_logits
 * [K,E,N,A]).  Row (k, e, i) uses weight set i when P = N and set 0 when P = 1.  A set's rows are all the rows that use it:
 * K E of them for P = N, K E N for P = 1, in (k, e, i) order.
 *
 * Observation shift.  With obs_first u8 [E,N,15,15,3], row k reads obs_first for k = 0 and obs[k - 1] otherwise: what the
 * rollouts record (slot k of their obs ring is the observation AFTER step k, and step k acted on the one before it).  The
 * shift is address arithmetic; nothing is copied, and obs[K - 1] is not read (obs may be NULL when K = 1).  Without obs_first
 * (NULL), row k reads obs[k].  obs is u8 [K,E,N,15,15,3]; a leading-axis slice of a ring is such an array, so the minibatch of
 * steps k0 .. k1 - 1 of a fragment is obs_first = ring[k0 - 1] (the fragment's own obs_first for k0 = 0), obs = ring + k0.
 *
 * Loss.  Per row, with (logits, value) the network's outputs, a = actions[row] (0 <= a < A; the caller's duty):
 *   logp  = log_softmax(logits)[a]                    ratio = exp(logp - logp_old)
 *   surr  = min(adv * ratio, adv * clip(ratio, 1 - c, 1 + c))                               c = clip_param
 *   kl    = KL(softmax(behaviour_logits) || softmax(logits))   (0 without behaviour_logits)
 *   ent   = the entropy of softmax(logits)
 *   vf1   = (value - vt)^2      vf2 = (vf_pred + clip(value - vf_pred, -vc, vc) - vt)^2     vc = vf_clip_param
 *   vf    = max(vf1, vf2)
 *   row_loss = -surr + kl_coeff * kl + vf_loss_coeff * vf - entropy_coeff * ent
 * loss_p is the mean of row_loss over set p's rows, and the call's scalar is the sum of loss_p over the sets: the sets share
 * no parameter, so each set's gradient is its own policy's (train_baseline.py:87-96).  behaviour_logits must be NULL if and
 * only if kl_coeff == 0.
 *
 * Derivatives at the kinks:
 *   d surr / d ratio = adv when 1 - c <= ratio <= 1 + c, or when adv * ratio < adv * clip(ratio) strictly; else 0
 *   d vf / d value   = 2 (value - vt) when |value - vf_pred| <= vc or vf1 >= vf2; else 0
 *   ReLU's derivative at 0 is 0.
 * So the first epoch, where ratio = 1 and value = vf_pred up to rounding and both branches tie, gives the unclipped gradient.
 * This equals torch autograd everywhere except on exact clip boundaries (at a tie torch's half-and-half split of minimum /
 * maximum sums to the same number).
 *
 * Arithmetic and order.  Exact float32, as the forward (the hyper-parameters are rounded to float32 once); the per-row loss
 * terms are float32 and enter float64 sums.  Every sum over rows has a fixed order that is a function of (K, E, N, P) alone:
 * a set's rows are cut into tiles of SSD_PPO_TILE rows, workgroup g of the G = SSD_PPO_GROUPS(set rows, P) of a set sums
 * tiles g, g + G, ... in that order in float32 (float64 for the statistics) -- the dense layers' biases, fc2's kernel and the
 * heads' kernels as a sum per tile added to the sum carried so far, fc1's and the conv's kernel and the conv's bias as one
 * accumulator continued through the tiles --, and the G partial sums are added in order in float64, scaled by 1 / rows and
 * rounded to float32 once.  No atomics: the same inputs give the same bits on every call and
 * on every device.
 *
 * Outputs.  grads f32 [P, SSD_POL_SET_FLOATS(A)]: d loss / d weights in the packed layout, padding floats zero.  stats f64
 * [P, 5]: the set means of row_loss, -surr (policy loss), vf, kl and ent (RLlib's kl_and_loss_stats less the explained
 * variance).  scratch: SSD_PPO_SCRATCH_FLOATS(set rows, P, A) floats the call overwrites, 8-byte aligned as stats is.
 *
 * Device pointers on device_id; two launches on `stream`, no allocation, no host synchronisation.  SSD_E_INVALID before
 * anything is launched (ssd_policy_last_error says why) for the network rules of ssd_policy_forward, n_steps or num_envs
 * < 1, more than 2^31 - 17 rows, a missing pointer, a misaligned scratch, grads or stats, a hyper-parameter that is not finite, a
 * negative clip_param or vf_clip_param, behaviour_logits without kl_coeff or the reverse, flags other than 0.
 * ====================================================================================================================== */
enum { SSD_PPO_TILE = 16, SSD_PPO_STAT_FLOATS = 16, SSD_PPO_MAX_GROUPS = 1024 };
/* workgroups (partial sums) per set: one per tile up to SSD_PPO_MAX_GROUPS / P */
#define SSD_PPO_TILES(set_rows) ((set_rows) / SSD_PPO_TILE + ((set_rows) % SSD_PPO_TILE != 0))
#define SSD_PPO_GROUPS(set_rows, P) \
    (SSD_PPO_TILES(set_rows) < SSD_PPO_MAX_GROUPS / (P) ? SSD_PPO_TILES(set_rows) : SSD_PPO_MAX_GROUPS / (P))
#define SSD_PPO_SCRATCH_FLOATS(set_rows, P, A) \
    ((size_t)(P) * (size_t)SSD_PPO_GROUPS(set_rows, P) * (size_t)(SSD_POL_SET_FLOATS(A) + SSD_PPO_STAT_FLOATS))
int ssd_policy_ppo_grad(const float *weights, int32_t num_sets, int32_t num_actions, const uint8_t *obs_first, const uint8_t *obs,
                        const int32_t *actions, const float *logp_old, const float *advantages, const float *value_targets,
                        const float *vf_preds, const float *behaviour_logits, int32_t n_steps, int32_t num_envs,
                        int32_t num_agents, double clip_param, double vf_clip_param, double vf_loss_coeff, double entropy_coeff,
                        double kl_coeff, float *scratch, float *grads, double *stats, int32_t device_id, uint32_t flags,
                        void *stream);

/* ======================================================================================================================
 * RECURRENT PPO LOSS AND GRADIENTS -- the learner's half of the loop for the recurrent policy the baseline trains: the loss of
 * PPO LOSS AND GRADIENTS above with truncated backpropagation through time (BPTT), its statistics and the gradient of every
 * parameter, in one call (csrc/ssd_policy_lstm_grad.hip).  Added after ABI 6 without a version bump: the
 * call is additive.
 *
 * Network: that of ssd_policy_lstm_forward above, the same packed weight layout (SSD_LSTM_*), P = 1 or P = N sets, A <= 15,
 * C = cell_size = 64, 128 or 256.
 *
 * Rows, observation shift, loss, statistics and derivatives at the kinks: exactly those of PPO LOSS AND GRADIENTS above (the
 * same device code forms a row's terms); loss = the sum over the sets of the set's mean row loss.  A sequence is one (e, i):
 * the K rows (k, e, i), k = 0 .. K - 1.
 *
 * State rule.  With T = seq_len (RLlib's max_seq_len) and state f32 [S, E, N, 2, C], S = ceil(K / T), the ring
 * ssd_rollout_policy_lstm records with state_every = T ((c, h) order), the state step k of sequence (e, i) uses is
 *   state[k / T] as stored, when k % T == 0: data, no gradient flows into it -- the truncation;
 *   zero, when k % T != 0 and done[k - 1, e, i] != 0 (selected, never loaded, as the forward's start rule): neither values nor
 *     gradient cross an episode end;
 *   the (c', h') this call computed for step k - 1 with the current weights, otherwise.
 * done is u8 [K, E, N] or NULL (no episode ends inside the fragment); done[K - 1] is not read.  The ring holds zero at a window
 * start that is an episode start, so a minibatch of steps k0 .. k1 - 1 with k0 % T == 0 is the slices [k0:k1] of the per-row
 * arrays and of done, obs_first = obs ring[k0 - 1] and state = ring + k0 / T.  Every row is a valid row: no padding, no mask;
 * a window cut short by K is a shorter window.
 *
 * Arithmetic and order.  The forward is exact float32 from the device pieces of the rollout (trunk, gates, cell, heads), the
 * per-row loss terms are float32 and enter float64 sums.  Every sum has a fixed order that is a function of (K, E, N, P, A, C,
 * T) alone; the call walks the windows w = 0, 1, ... in order and every partial sum below is continued from window to window:
 *   heads' kernels and biases, statistics: the sequences of a set ((e) for P = N, (e, i) for P = 1, in that order) are cut into
 *     tiles of SSD_RPPO_TILE; workgroup g of the Gs = SSD_RPPO_GROUPS(sequences of a set, P) takes tiles g, g + Gs, ...;
 *     per tile it walks the window's steps backwards (forwards for the statistics) and adds each step's sum over the tile
 *     to the sum carried so far (float32; float64 for the statistics);
 *   lstm_w, lstm_b: a set's rows of the window, in (k, e, i) order, are cut into chunks of SSD_RPPO_CHUNK rows; split s of
 *     the SSD_RPPO_SPLITS(a whole window's set rows) takes chunks s, s + S, ... as one accumulator in row order (lstm_b: four
 *     accumulators of every fourth row, added in order at the end of a window);
 *   the trunk: as PPO LOSS AND GRADIENTS orders it, over the window's rows, with G = SSD_PPO_GROUPS(a whole window's set rows, P).
 * A whole window has min(T, K) steps.  The partial sums of an entry are then added in order in float64, scaled by 1 / (the
 * set's rows, K E or K E N) and rounded to float32 once.  No atomics: the same inputs give the same bits.
 *
 * Outputs.  grads f32 [P, SSD_LSTM_SET_FLOATS(C, A)] in the packed layout, padding floats zero.  stats f64 [P, 5] as above.
 * scratch: SSD_RPPO_SCRATCH_FLOATS(K, E, N, P, A, C, T) floats the call overwrites, 8-byte aligned; it grows with the rows
 * of one window and the numbers of partial sums, not with K beyond min(T, K).
 *
 * Device pointers on device_id; everything is enqueued on `stream`, no allocation, no host synchronisation.  SSD_E_INVALID
 * before anything is launched (ssd_policy_last_error says why) for everything ssd_policy_ppo_grad refuses, a cell_size other
 * than 64, 128 or 256, seq_len < 1, a missing or misaligned state.
 * ====================================================================================================================== */
enum { SSD_RPPO_TILE = 16, SSD_RPPO_CHUNK = 64, SSD_RPPO_MAX_SPLITS = 32 };
#define SSD_RPPO_MIN(a, b) ((a) < (b) ? (a) : (b))
/* sequences of one weight set; workgroups (partial sums) per set of the sequence kernel; splits per set of lstm_w's */
#define SSD_RPPO_SEQS(E, N, P) ((E) * (N) / (P))
#define SSD_RPPO_GROUPS(seqs, P) \
    SSD_RPPO_MIN(((seqs) + SSD_RPPO_TILE - 1) / SSD_RPPO_TILE, SSD_PPO_MAX_GROUPS / (P))
#define SSD_RPPO_SPLITS(window_set_rows) \
    ((int)SSD_RPPO_MIN(((window_set_rows) + SSD_RPPO_CHUNK - 1) / SSD_RPPO_CHUNK, SSD_RPPO_MAX_SPLITS))
/* per row of a whole window: features 32, d (logits, value) / dx 32, (c', h') 2C, gates / dz 4C */
#define SSD_RPPO_ROW_FLOATS(C) (64 + 6 * (C))
#define SSD_RPPO_WINDOW_SET_ROWS(K, E, N, P, T) ((int64_t)SSD_RPPO_MIN(T, K) * SSD_RPPO_SEQS(E, N, P))
#define SSD_RPPO_SCRATCH_FLOATS(K, E, N, P, A, C, T)                                                                          \
    ((size_t)(P) * (32 + (C)) * 4 * (C) + (size_t)SSD_RPPO_MIN(T, K) * (E) * (N) * SSD_RPPO_ROW_FLOATS(C) +               \
     (size_t)(P) * SSD_PPO_GROUPS((int32_t)SSD_RPPO_WINDOW_SET_ROWS(K, E, N, P, T), P) * (SSD_LSTM_W + SSD_PPO_STAT_FLOATS) + \
     (size_t)(P) * SSD_RPPO_GROUPS(SSD_RPPO_SEQS(E, N, P), P) * (16 * (C) + 16 + SSD_PPO_STAT_FLOATS) +                  \
     (size_t)(P) * SSD_RPPO_SPLITS(SSD_RPPO_WINDOW_SET_ROWS(K, E, N, P, T)) * ((32 + (C)) * 4 * (C) + 4 * (C)))
int ssd_policy_lstm_ppo_grad(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size, int32_t seq_len,
                             const uint8_t *obs_first, const uint8_t *obs, const float *state, const uint8_t *done,
                             const int32_t *actions, const float *logp_old, const float *advantages, const float *value_targets,
                             const float *vf_preds, const float *behaviour_logits, int32_t n_steps, int32_t num_envs,
                             int32_t num_agents, double clip_param, double vf_clip_param, double vf_loss_coeff,
                             double entropy_coeff, double kl_coeff, float *scratch, float *grads, double *stats,
                             int32_t device_id, uint32_t flags, void *stream);

/* ======================================================================================================================
 * MOA PPO LOSS AND GRADIENTS -- the learner's half of the loop for the causal-influence policy (run_scripts/train_moa.py,
 * algorithms/ppo_causal.py:36-75): PPOLoss + moa_weight * MOALoss on a sampled fragment with truncated BPTT through both
 * Keras LSTMs, its statistics and the gradient of every parameter, in one call (csrc/ssd_policy_moa_grad.hip; DESIGN.md
 * section 18).  Added after ABI 6 without a version bump: the call is additive.
 *
 * Network: that of ssd_policy_moa_forward above, the same packed weight layout (SSD_MOA_*), P = 1 or P = N sets,
 * 2 <= N <= SSD_MOA_MAX_AGENTS, A <= 15, C = cell_size = 64, 128 or 256.  Exact float32 on v_mfma_f32_16x16x4_f32.
 *
 * Rows, observation shift, the PPO terms and their derivatives at the kinks: exactly those of PPO LOSS AND GRADIENTS (the
 * same device code forms them, on the actions LSTM's logits and value).  The row loss of row (k, e, i) is
 *   the PPO row loss  +  moa_weight * (1 / (N - 1)) * sum over j of CE(pred[j], actions[k, e, others(i)[j]]),
 * pred [N-1][A] the MOA LSTM's prediction of the step, others(i) the agents other than i in the order of their ids sorted as
 * strings, CE(l, a) = logsumexp(l) - l[a]; the targets are this step's actions of the other agents (the pairing of
 * ConvMOAPolicy.moa_loss; the visibility factor is 1), clamped to 0 .. A - 1 as actions are.  The loss of a weight set is the
 * mean of the row loss over the set's rows (K E for P = N, K E N for P = 1); the returned loss is the sum over the sets.
 * stats f64 [P][6]: the five of PPO LOSS AND GRADIENTS (total_loss includes the weighted MOA term), then moa_loss, the mean
 * cross-entropy (over rows and other agents) without the weight.
 *
 * State rule: that of RECURRENT PPO LOSS AND GRADIENTS for all four rows of state f32 [S, E, N, 4, C] = (h1, c1, h2, c2), the
 * ring ssd_rollout_policy_moa records with state_every = T = seq_len.  prev_actions i32 [K, E, N] is the ring that call records:
 * row (k, e, .) is the joint action step k's MOA read, by agent index.  It is data everywhere: read as stored at a window's
 * first step (the ring holds zero at an episode start); at a step k % T != 0 after done[k - 1, e, i] != 0 the whole
 * previous-action vector of row (k, e, i) is zero, selected and never loaded, as its state is.  A minibatch of steps
 * k0 .. k1 - 1 with k0 % T == 0 is the slices [k0:k1] of the per-row arrays, done and prev_actions, obs_first = obs ring
 * [k0 - 1] and state = ring + k0 / T.
 *
 * Gradient flows from the PPO terms through the heads, the actions LSTM (BPTT) and stack 0 into the conv, and from the
 * cross-entropy through pred_w / pred_b, the MOA LSTM (BPTT), stack 1 and the action rows 32 .. 32 + N - 1 of the MOA kernel
 * into the conv; conv_w and conv_b receive the sum.  The counterfactuals and the influence are not part of the loss (the
 * influence is data inside the advantages).  grads f32 [P, SSD_MOA_SET_FLOATS(C, A, N)] in the packed layout; rows 32 + N .. 47
 * of the MOA matrix and all padding floats are zero.
 *
 * Arithmetic and order: as RECURRENT PPO LOSS AND GRADIENTS.  Per window the call runs the features of both stacks, then for
 * the actions branch and after it for the MOA branch the sequence kernel (tiles of SSD_MPPO_TILE sequences, workgroup g of
 * SSD_MPPO_GROUPS takes tiles g, g + G, ...; the cross-entropies of a workgroup are float32 terms in float64 sums, one per
 * (tile row, other agent), added in that order at the end) and the split sums of the LSTM matrix and bias (chunks of
 * SSD_MPPO_CHUNK rows, split s of SSD_MPPO_SPLITS takes chunks s, s + S, ...); pred_w = h2'^T dpred and pred_b by the same
 * partition; then the trunk's backward once per stack, stack 1 adding its conv sums to stack 0's.  The partial sums of an
 * entry are added in order in float64, scaled by 1 / (the set's rows) and rounded once.  No atomics: the same inputs give the
 * same bits.
 *
 * scratch: SSD_MPPO_SCRATCH_FLOATS(K, E, N, P, A, C, T) floats the call overwrites, 8-byte aligned; it grows with the rows of
 * one window and the numbers of partial sums, not with K beyond min(T, K).  moa_weight: finite, >= 0.
 *
 * Device pointers on device_id; everything is enqueued on `stream`, no allocation, no host synchronisation.  SSD_E_INVALID
 * before anything is launched (ssd_policy_last_error says why) for everything ssd_policy_lstm_ppo_grad refuses, fewer than 2
 * or more than SSD_MOA_MAX_AGENTS agents, a missing or misaligned prev_actions, a moa_weight that is not finite or negative.
 * ====================================================================================================================== */
enum { SSD_MPPO_TILE = 16, SSD_MPPO_CHUNK = 64, SSD_MPPO_MAX_SPLITS = 32 };
#define SSD_MPPO_GROUPS(seqs, P) SSD_RPPO_GROUPS(seqs, P)
#define SSD_MPPO_SPLITS(window_set_rows) SSD_RPPO_SPLITS(window_set_rows)
/* floats between the rows of dpred and of pred_w's partial sums: (N - 1) A rounded up to whole 16-column tiles */
#define SSD_MPPO_PRED_PITCH(A, N) ((((N) - 1) * (A) + 15) / 16 * 16)
/* per row of a whole window: both stacks' features 64, their d (logits, value) / dx 64, (h', c') 2C and gates / dz 4C (one
 * branch at a time), dpred */
#define SSD_MPPO_ROW_FLOATS(C, A, N) (128 + 6 * (C) + SSD_MPPO_PRED_PITCH(A, N))
/* the blocks, in order: both LSTM matrices transposed; the window's rows; the trunk's partial sets (the MOA layout below
 * SSD_MOA_LSTM_W); the sequence kernel's (heads, then 8 float64 statistics); the two LSTM matrices' and pred_w's splits */
#define SSD_MPPO_SCRATCH_FLOATS(K, E, N, P, A, C, T)                                                                              \
    ((size_t)(P) * (80 + 2 * (C)) * 4 * (C) + (size_t)SSD_RPPO_MIN(T, K) * (E) * (N) * SSD_MPPO_ROW_FLOATS(C, A, N) +            \
     (size_t)(P) * SSD_PPO_GROUPS((int32_t)SSD_RPPO_WINDOW_SET_ROWS(K, E, N, P, T), P) * (SSD_MOA_LSTM_W(C) + SSD_PPO_STAT_FLOATS) + \
     (size_t)(P) * SSD_MPPO_GROUPS(SSD_RPPO_SEQS(E, N, P), P) * (16 * (C) + 16 + SSD_PPO_STAT_FLOATS) +                         \
     (size_t)(P) * SSD_MPPO_SPLITS(SSD_RPPO_WINDOW_SET_ROWS(K, E, N, P, T)) *                                                    \
         ((80 + 2 * (C)) * 4 * (C) + 8 * (C) + ((C) + 1) * SSD_MPPO_PRED_PITCH(A, N)))
int ssd_policy_moa_ppo_grad(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size, int32_t seq_len,
                            const uint8_t *obs_first, const uint8_t *obs, const float *state, const int32_t *prev_actions,
                            const uint8_t *done, const int32_t *actions, const float *logp_old, const float *advantages,
                            const float *value_targets, const float *vf_preds, const float *behaviour_logits, int32_t n_steps,
                            int32_t num_envs, int32_t num_agents, double clip_param, double vf_clip_param, double vf_loss_coeff,
                            double entropy_coeff, double kl_coeff, double moa_weight, float *scratch, float *grads,
                            double *stats, int32_t device_id, uint32_t flags, void *stream);

/* ======================================================================================================================
 * A3C LOSS AND GRADIENTS -- the learner's half of the loop under the baseline's default algorithm (run_scripts/
 * train_baseline.py:23; algorithms/a3c_causal.py:28-46 and :60-76) for the three policies: ssd_policy_ac_grad (conv-FC),
 * ssd_policy_lstm_ac_grad (recurrent) and ssd_policy_moa_ac_grad (MOA), `ac` for the actor-critic loss.  Each is the PPO call
 * of the same policy above with another row loss and another last step: the same kernels compiled with the A3C row terms,
 * the same host code (csrc/ssd_policy_grad.hip, ssd_policy_lstm_grad.hip, ssd_policy_moa_grad.hip).
 * Added after ABI 6 without a version bump: the calls are additive.  advantages and value_targets are what ssd_advantages
 * returns with use_gae = 0 (discounted returns), or any other.
 *
 * Networks, rows, the observation shift, the state rule, prev_actions, windows of seq_len and the minibatch slices: exactly
 * those of PPO LOSS AND GRADIENTS, RECURRENT PPO LOSS AND GRADIENTS and MOA PPO LOSS AND GRADIENTS, for the matching call.
 * logp_old, vf_preds and behaviour_logits are not inputs, and there are no clip or KL hyper-parameters.
 *
 * Loss.  Per row, with (logits, value) the network's outputs, a = actions[row] clamped to 0 .. A - 1:
 *   logp = log_softmax(logits)[a]        pi  = -logp * adv
 *   vf   = 0.5 * (value - vt)^2          ent = the entropy of softmax(logits)
 *   row_loss = (pi + vf_loss_coeff * vf) - entropy_coeff * ent
 *   d row_loss / d logits[k] = -adv * ([k = a] - p_k) + entropy_coeff * p_k * (logp_k + ent)
 *   d row_loss / d value     = vf_loss_coeff * (value - vt)
 * loss_p is the SUM of row_loss over set p's rows (the reference reduces with reduce_sum), and the call's scalar is the sum
 * of loss_p over the sets.  The loss has no clip kinks; ReLU's derivative at 0 is 0.
 *
 * The MOA policy (a3c_causal.py:70-71): total += moa_weight * MOALoss, and MOALoss is a MEAN (common_funcs.py:96) while the
 * A3C terms are sums.  So the MOA term of row (k, e, i) is the cross-entropy term of MOA PPO LOSS AND GRADIENTS (the same
 * pairing, the same string-sorted others, the same clamped targets, visibility 1) times 1 / (the set's rows):
 *   row_loss + moa_weight * (1 / (N - 1)) * (1 / rows) * sum over j of CE(pred[j], actions[k, e, others(i)[j]]).
 * The three factors are one float32 scale on d loss / d pred, formed in double as moa_weight / ((N - 1) * rows) and rounded
 * once: the conv's gradient adds both branches into one slot before the reduction, so the factor cannot wait for it.
 *
 * Arithmetic and order.  Exact float32, the row terms in float64 sums, and every sum in exactly the matching PPO call's
 * order: the same tiles, groups, chunks and splits.  The one difference is the last step: the float64 total of an entry is
 * rounded to float32 as it is, without the division by the set's rows.  No atomics: the same inputs give the same bits.
 *
 * Outputs.  grads in the policy's packed layout, padding floats zero.  stats f64 [P][4] for ssd_policy_ac_grad and
 * ssd_policy_lstm_ac_grad: the set SUMS of row_loss, pi, vf and ent (the reference's total_loss, policy_loss, vf_loss and
 * policy_entropy; the explained variance stays out).  stats f64 [P][5] for ssd_policy_moa_ac_grad: those four, total_loss
 * including moa_weight * moa_loss, then moa_loss, the mean cross-entropy over rows and other agents without the weight (the
 * one statistic that is divided by the set's rows).
 *
 * scratch: SSD_PPO_SCRATCH_FLOATS, SSD_RPPO_SCRATCH_FLOATS and SSD_MPPO_SCRATCH_FLOATS of the same shape, for the matching
 * call; one buffer serves a policy's PPO and A3C calls.
 *
 * SSD_E_INVALID before anything is launched (ssd_policy_last_error says why) for everything the matching PPO call refuses,
 * less the arguments that are gone: the required per-row pointers are actions, advantages and value_targets, the
 * hyper-parameters that must be finite are vf_loss_coeff and entropy_coeff (and moa_weight, finite and >= 0), flags other
 * than 0.
 * ====================================================================================================================== */
int ssd_policy_ac_grad(const float *weights, int32_t num_sets, int32_t num_actions, const uint8_t *obs_first, const uint8_t *obs,
                       const int32_t *actions, const float *advantages, const float *value_targets, int32_t n_steps,
                       int32_t num_envs, int32_t num_agents, double vf_loss_coeff, double entropy_coeff, float *scratch,
                       float *grads, double *stats, int32_t device_id, uint32_t flags, void *stream);
int ssd_policy_lstm_ac_grad(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size, int32_t seq_len,
                            const uint8_t *obs_first, const uint8_t *obs, const float *state, const uint8_t *done,
                            const int32_t *actions, const float *advantages, const float *value_targets, int32_t n_steps,
                            int32_t num_envs, int32_t num_agents, double vf_loss_coeff, double entropy_coeff, float *scratch,
                            float *grads, double *stats, int32_t device_id, uint32_t flags, void *stream);
int ssd_policy_moa_ac_grad(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size, int32_t seq_len,
                           const uint8_t *obs_first, const uint8_t *obs, const float *state, const int32_t *prev_actions,
                           const uint8_t *done, const int32_t *actions, const float *advantages, const float *value_targets,
                           int32_t n_steps, int32_t num_envs, int32_t num_agents, double vf_loss_coeff, double entropy_coeff,
                           double moa_weight, float *scratch, float *grads, double *stats, int32_t device_id, uint32_t flags,
                           void *stream);

/* ======================================================================================================================
 * V-TRACE TARGETS -- what the IMPALA trainer (algorithms/impala_causal.py; RLlib 0.7.6's VTraceLoss) does between evaluating
 * a fragment under the learner's current weights and its loss: vtrace.from_importance_weights (Espeholt et al. 2018) with
 * discounts = (1 - done) * gamma, computed on the device from the [ring, ...] rings of the policy rollouts above
 * (csrc/ssd_vtrace.hip).  Added after ABI 6 without a version bump: the call is additive.
 *
 * Lanes are trajectories: L = lanes (E * N for the rollouts' rings), lane l is column l of the [ring, L] rings.  Row k of a
 * call is slot (step0 + k) % ring.  Every operation is one IEEE float64 operation in the order written here (no fused
 * multiply-add); the two results are rounded to float32 once, when they are stored.  The truncation level of the trace
 * coefficients (c bar) is fixed at 1, as in RLlib.  With K = n_steps and bootstrap = (double)bootstrap_value, walking
 * k = K - 1 ... 0, per lane:
 *   r       = (double)rew[k], or (double)rew[k] + bonus_weight * (double)bonus[k] with a bonus (multiply, then add)
 *   disc    = 0.0 if done[k] != 0, else gamma
 *   v       = (double)value[k]            rho = (double)rhos[k]
 *   v_next  = bootstrap for k = K - 1, else (double)value[k + 1]
 *   vs_next = bootstrap for k = K - 1, else the unrounded vs of row k + 1
 *   delta   = min(clip_rho_threshold, rho) * ((r + disc * v_next) - v)
 *   dc      = disc * min(1.0, rho)
 *   acc     = delta + dc * (0.0 for k = K - 1, else the acc of row k + 1)
 *   vs[k]            = (float)(v + acc)
 *   pg_advantages[k] = (float)(min(clip_pg_rho_threshold, rho) * ((r + disc * vs_next) - v))
 * value and bootstrap_value are the TARGET policy's (the learner's current weights), not what the rollout recorded; rhos is
 * pi / mu of the taken actions, exp(logp_target - logp_behaviour), formed by the caller (the kernel computes no exp), assumed
 * finite and >= 0.  done[k] != 0 says that the episode ended with step k and row k + 1 belongs to the next one.  NULL done:
 * no episode ends.  NULL bootstrap_value: 0.  NULL bonus: none (bonus_weight is not read).  A threshold of +inf means no
 * clip.  Inputs are assumed finite.
 *
 * One difference from the reference's trainer, on the caller's side: RLlib cuts the batch into sequences of T rows, drops each
 * sequence's last row from the loss and bootstraps from that row's value.  Here every row of the call is a target row, as in
 * every other call of this library; the reference's targets of one T-row sequence are this call on its first T - 1 rows with
 * bootstrap_value = the current value of row T - 1.  There is no row mask.
 *
 * rew i32, bonus f32, value f32, rhos f32, done u8, vs f32 and pg_advantages f32 are [ring, L]; bootstrap_value f32 is [L];
 * device pointers on device_id.  One launch on `stream`, no allocation, no synchronisation.  SSD_E_INVALID before any device
 * call (ssd_vtrace_last_error says why) for lanes < 1, ring < 1, n_steps < 1 or > ring, step0 < 0, flags other than 0, a
 * missing rew, value, rhos or output pointer, a gamma that is not finite, a threshold that is NaN or <= 0, a bonus with a
 * bonus_weight that is not finite; SSD_E_DEVICE without a usable HIP device.
 * ====================================================================================================================== */
int ssd_vtrace(const int32_t *rew, const float *bonus, double bonus_weight, const float *value, const float *rhos,
               const uint8_t *done, const float *bootstrap_value, int32_t lanes, int32_t ring, int32_t step0, int32_t n_steps,
               double gamma, double clip_rho_threshold, double clip_pg_rho_threshold, uint32_t flags, float *vs,
               float *pg_advantages, int32_t device_id, void *stream);
const char *ssd_vtrace_last_error(void);   /* the calling thread's last ssd_vtrace error */

/* ======================================================================================================================
 * BATCH MOMENTS -- the step RLlib 0.7.6's PPO trainer takes between compute_advantages and its SGD epochs, and one of the
 * statistics it reports (csrc/ssd_moments.hip).  Its optimizers are built with
 * standardize_fields=["advantages"]: each policy's train batch has its advantages replaced by
 * (value - value.mean()) / max(1e-4, value.std()) -- ssd_standardize; vf_explained_var is
 * max(-1, 1 - var(targets - prediction) / var(targets)) -- ssd_explained_variance.  RLlib is not installed beside this
 * library: both rules are stated from memory of its source.  Added after ABI 6 without a version bump: the calls are additive.
 *
 * Lanes and rows are those of ssd_advantages: x is f32 [ring, lanes], row k of a call is slot (step0 + k) % ring for
 * k < n_steps, rows outside the call are neither read nor written.  The weight set of lane l is l % num_sets (num_sets is 1,
 * or any value that divides lanes: the lanes of [E, N] rings with one set per agent).  Per set p the call holds
 * n = n_steps * (lanes / num_sets) elements; element j of the set, j = k * (lanes / num_sets) + l / num_sets, is the call's
 * flat element (k * lanes + l) = j * num_sets + p.
 *
 * THE SUMMATION ORDER IS THE CONTRACT.  It is a function of (n_steps, lanes, num_sets) and the three constants below alone --
 * not of the grid, the device or the number of compute units.  Every operation is one IEEE float64 operation, round to
 * nearest even, in the order written here; there is no fused multiply-add and no atomic.  SUM(f), for a quantity f(j) of a set:
 *   chunk c = 0 .. SSD_MOM_CHUNKS - 1 holds the elements j in [c * SSD_MOM_CHUNK, (c + 1) * SSD_MOM_CHUNK), j < n
 *   thread t = 0 .. SSD_MOM_BLOCK - 1 of chunk c:   a[t] = 0.0;  for u = 0 .. SSD_MOM_ITEMS - 1, in this order, with
 *       j = c * SSD_MOM_CHUNK + u * SSD_MOM_BLOCK + t:   if j < n:  a[t] = a[t] + f(j)
 *   the workgroup's tree:   for off = SSD_MOM_BLOCK / 2, SSD_MOM_BLOCK / 4, ..., 1:   a[t] = a[t] + a[t + off] for every t < off
 *       (all t of one off at once, from the values before that off);   partial[c] = a[0]
 *   across chunks:   s = 0.0;  for c = 0 .. SSD_MOM_CHUNKS - 1:  s = s + partial[c];   SUM(f) = s
 * With nd = (double)n, per set, for a quantity x(j) converted to float64:
 *   mean = SUM(x) / nd
 *   var  = SUM(d * d) / nd  with  d = x(j) - mean   (subtract, multiply, then the add of SUM: a true second pass over the
 *          data, never E[x^2] - mean^2)
 *   std  = sqrt(var)        (the correctly rounded square root)
 *
 * ssd_standardize:  denom = std if std > min_std, else min_std;  out = (float)((x(j) - mean) / denom), one subtraction and one
 * correctly rounded division in float64, one rounding to float32.  A set of one element, or of equal elements, has std = 0
 * and out exactly 0.  out may be x itself (in place); it must not overlap x otherwise.  moments, when not NULL, is
 * f64 [num_sets][2] = (mean, std) per set.  RLlib's min_std is 1e-4.
 *
 * ssd_explained_variance:  with y(j) and diff(j) = (double)y - (double)pred (formed in float64), both variances by the rule
 * above;  r = 1.0 - var(diff) / var(y);  out[p] = (float)(-1.0 if r < -1.0, else r);  out is f32 [num_sets].  var(y) = 0
 * follows IEEE arithmetic: var(diff) > 0 gives -inf and so -1; both 0 give 0 / 0, and out[p] is a NaN (of no particular sign
 * or payload); a set of one element is such a set.
 *
 * scratch is SSD_MOM_SCRATCH_DOUBLES(n_steps, lanes, num_sets) float64 of device memory, aligned to 8 bytes, the call's own
 * until it has finished (the chunk partials; contents on entry do not matter).  Inputs are assumed finite.  Device pointers on
 * device_id.  Three launches on `stream` (the sums; the squared deviations; the result), each of which adds up the earlier
 * ones' partials again in the order above; no allocation, no synchronisation, no launch that waits for another workgroup.
 * SSD_E_INVALID before any device call (ssd_moments_last_error says why) for lanes < 1, ring < 1, n_steps < 1 or > ring,
 * step0 < 0, num_sets < 1 or not a divisor of lanes or > 65535, a missing x, y, pred, out or scratch pointer, a pointer
 * not aligned to its element, a min_std that is not finite or <= 0; SSD_E_DEVICE without a usable HIP device.
 * ====================================================================================================================== */
#define SSD_MOM_BLOCK 256                                     /* threads of a workgroup */
#define SSD_MOM_ITEMS 16                                      /* elements a thread adds, one after the other */
#define SSD_MOM_CHUNK (SSD_MOM_BLOCK * SSD_MOM_ITEMS)         /* elements of one set a workgroup takes per pass */
#define SSD_MOM_CHUNKS(n_steps, lanes, num_sets) \
    (((int64_t)(n_steps) * ((lanes) / (num_sets)) + SSD_MOM_CHUNK - 1) / SSD_MOM_CHUNK)
#define SSD_MOM_SCRATCH_DOUBLES(n_steps, lanes, num_sets) (4 * (int64_t)(num_sets) * SSD_MOM_CHUNKS(n_steps, lanes, num_sets))
int ssd_standardize(const float *x, int32_t lanes, int32_t ring, int32_t step0, int32_t n_steps, int32_t num_sets, double min_std,
                    double *scratch, double *moments, float *out, int32_t device_id, void *stream);
int ssd_explained_variance(const float *y, const float *pred, int32_t lanes, int32_t ring, int32_t step0, int32_t n_steps,
                           int32_t num_sets, double *scratch, float *out, int32_t device_id, void *stream);
const char *ssd_moments_last_error(void);   /* the calling thread's last ssd_standardize / ssd_explained_variance error */

/* ======================================================================================================================
 * WATERSHED PPO LOSS AND GRADIENTS -- the learner's half of the loop for the Watershed baselines' policy (LSTMFCNet, WATERSHED
 * POLICY ROLLOUTS above), whose launchers default to PPO (run_scripts/train_watershed_baseline.py,
 * train_watershed_comm_baseline.py): RLlib 0.7.6's PPO loss on sequences the caller has gathered, with truncated
 * backpropagation through time, its statistics and the gradient of every parameter of one agent id's weight set, in one call
 * (csrc/ssd_ws_policy_grad.hip).  Added after ABI 6 without a version bump: the call is additive.
 *
 * One call is one agent id, and so one weight set: in the reference each agent's policy is its own graph and its own loss, so
 * a learner makes one call per id.  Network: that of ssd_ws_policy_forward, the same packed layout (SSD_WSP_*); weights are all
 * num_sets sets, of which set agent_id is read.  C = cell_size = 64, 128 or 256.  (variant, agent_id) decide the head as in
 * WATERSHED POLICY ROLLOUTS: SSD_WS_SEQ_COMM ids 0-3 are comm agents, every other id is an action agent.
 *
 * Rows.  M = n_steps is the number of the agent's OWN steps, in order; Q = num_seqs the number of sequences, a sequence being
 * one env's trajectory of this agent.  Every per-row array is [M, Q]: actions f32 (the message index as a float for a comm
 * agent, clamped to 0 .. 4; the UNCLIPPED Gaussian sample for an action agent: what the rollouts record), logp_old,
 * advantages, value_targets, vf_preds f32.  obs is f32 [M, Q, 12]: the observation each step acted on, already gathered (no
 * shift by address here); dense0 reads all 12 columns, the rows of dense0_w beyond the agent's observation length meet the
 * zero padding.  behaviour_dist is f32 [M, Q, 5] (the dist the actions were drawn from), or NULL when kl_coeff == 0 (with
 * kl_coeff == 0 it is not read).  Which reward is credited to which step, advantages and value targets are the caller's
 * (ssd_advantages accepts any [R, L] arrays).
 *
 * State rule: that of RECURRENT PPO LOSS AND GRADIENTS with T = seq_len and starts u8 [M, Q] in the place of done[k - 1].
 * state is f32 [ceil(M / T), Q, 2, C] in (h, c) order, as the rollouts' state ring holds it.  Step m of sequence q uses
 *   state[m / T] as stored, when m % T == 0: data, no gradient flows into it (starts[m] is NOT looked at there);
 *   zero, when m % T != 0 and starts[m, q] != 0 (selected, never loaded);
 *   the (h', c') this call computed for step m - 1 with the current weights, otherwise.
 * starts may be NULL.  A fragment that is no multiple of T ends in a shorter window; no padding, no mask.
 *
 * Row loss: PPO LOSS AND GRADIENTS' terms (ratio, surr, vf, the derivatives at the kinks, row_loss and the statistics) with
 * the head's distribution in the place of the Categorical over A actions.
 *   comm agent:   Categorical over dist[0:5]: exactly the row terms of PPO LOSS AND GRADIENTS with A = 5 (the same device code).
 *   action agent: a one-dimensional DiagGaussian, mean = dist[0], log_std = dist[1]; dist[2:5] are unused and their gradient
 *     is exactly zero.  With a = actions[row], std = expf(log_std), z = (a - mean) / std:
 *       logp = ((-0.5f * (z * z)) - log_std) - 0.9189385f            (the rollout's expression)
 *       ent  = log_std + 1.4189385f
 *       kl   = ((log_std - log_std_old) + 0.5f * q) - 0.5f,  q = (expf(2 log_std_old) + (mean_old - mean)^2) / expf(2 log_std)
 *              (RLlib's prev_dist.kl(curr_dist); 0 without behaviour_dist)
 *       d logp / d mean = z / std     d logp / d log_std = z^2 - 1     d ent / d log_std = 1
 *       d kl / d mean = -(mean_old - mean) / expf(2 log_std)           d kl / d log_std = 1 - q
 *     These three formulas are stated from memory of RLlib 0.7.6's DiagGaussian (ray is not available to check against), as
 *     the Categorical's are above.
 * loss is the mean of row_loss over the M Q rows.  ReLU's derivative at 0 is 0.
 *
 * Arithmetic and order.  The forward is exact float32 from the device pieces of the rollout (the dense chains, gates, cell,
 * heads); the per-row loss terms are float32 and enter float64 sums.  Every sum has a fixed order that is a function of
 * (M, Q, C, T) alone; the windows are walked in order and every partial sum is continued from window to window:
 *   heads' kernels and biases, statistics: the sequences are cut into tiles of SSD_WSPPO_TILE; workgroup g of the
 *     SSD_WSPPO_GROUPS(Q) takes tiles g, g + G, ...; per tile it walks the window's steps backwards (forwards for the
 *     statistics) and adds each step's sum over the tile to the sum carried so far (float32; float64 for the statistics);
 *   lstm_w, lstm_b: the window's rows in (m, q) order are cut into chunks of SSD_WSPPO_CHUNK rows; split s of the
 *     SSD_WSPPO_SPLITS(a whole window's rows) takes chunks s, s + S, ... as one accumulator in row order (lstm_b: four
 *     accumulators of every fourth row, added in order at the end of a window);
 *   dense0, dense1: the window's rows are cut into tiles of SSD_WSPPO_TILE rows; workgroup g of the
 *     SSD_WSPPO_TRUNK_GROUPS(a whole window's rows) takes tiles g, g + TG, ..., a sum per tile added to the sum carried so far.
 * A whole window has min(T, M) steps.  The partial sums of an entry are then added in order in float64, scaled by 1 / (M Q)
 * and rounded to float32 once.  No atomics: the same inputs give the same bits.
 *
 * Outputs.  grads f32 [SSD_WSP_SET_FLOATS(C)]: set agent_id's gradient in the packed layout, padding floats zero (the other
 * sets' gradients are zero and not written anywhere).  stats f64 [5]: the means of row_loss, -surr, vf, kl and ent.  scratch:
 * SSD_WSPPO_SCRATCH_FLOATS(M, Q, C, T) floats the call overwrites, 8-byte aligned as stats is; it grows with the rows of one
 * window and the numbers of partial sums, not with M beyond min(T, M).
 *
 * Device pointers on device_id; everything is enqueued on `stream` (1 + 3 per window + 1 launches), no allocation, no host
 * synchronisation.  SSD_E_INVALID before anything is launched (ssd_policy_last_error says why) for an unknown variant, a
 * num_sets that is not the variant's, an agent_id outside 0 .. num_sets - 1, a cell_size other than 64, 128 or 256, seq_len,
 * n_steps or num_seqs < 1, more than 2^31 - 17 rows, a NULL weights, obs, state, actions, logp_old, advantages, value_targets,
 * vf_preds, scratch, grads or stats, a NULL behaviour_dist with kl_coeff != 0, a hyper-parameter that is not finite, a
 * negative clip_param or vf_clip_param, a misaligned scratch, stats or float buffer, flags other than 0.
 * ====================================================================================================================== */
enum { SSD_WSPPO_TILE = 16, SSD_WSPPO_CHUNK = 64, SSD_WSPPO_MAX_GROUPS = 1024, SSD_WSPPO_MAX_SPLITS = 32, SSD_WSPPO_MAX_TRUNK_GROUPS = 256 };
#define SSD_WSPPO_MIN(a, b) ((a) < (b) ? (a) : (b))
/* workgroups (partial sums) of the sequence kernel; splits of lstm_w's; workgroups of the dense layers' */
#define SSD_WSPPO_GROUPS(Q) SSD_WSPPO_MIN(((Q) + SSD_WSPPO_TILE - 1) / SSD_WSPPO_TILE, SSD_WSPPO_MAX_GROUPS)
#define SSD_WSPPO_SPLITS(window_rows) \
    ((int)SSD_WSPPO_MIN(((window_rows) + SSD_WSPPO_CHUNK - 1) / SSD_WSPPO_CHUNK, SSD_WSPPO_MAX_SPLITS))
#define SSD_WSPPO_TRUNK_GROUPS(window_rows) \
    ((int)SSD_WSPPO_MIN(((window_rows) + SSD_WSPPO_TILE - 1) / SSD_WSPPO_TILE, SSD_WSPPO_MAX_TRUNK_GROUPS))
/* per row of a whole window: dense0's output 16, dense1's 16, d (dist, value) / dx 16, (h', c') 2C, gates / dz 4C */
#define SSD_WSPPO_ROW_FLOATS(C) (48 + 6 * (C))
#define SSD_WSPPO_WINDOW_ROWS(M, Q, T) ((int64_t)SSD_WSPPO_MIN(T, M) * (Q))
#define SSD_WSPPO_SCRATCH_FLOATS(M, Q, C, T)                                                                  \
    ((size_t)(16 + (C)) * 4 * (C) + (size_t)SSD_WSPPO_WINDOW_ROWS(M, Q, T) * SSD_WSPPO_ROW_FLOATS(C) +      \
     (size_t)SSD_WSPPO_TRUNK_GROUPS(SSD_WSPPO_WINDOW_ROWS(M, Q, T)) * SSD_WSP_LSTM_W +                       \
     (size_t)SSD_WSPPO_GROUPS(Q) * (8 * (C) + 8 + SSD_PPO_STAT_FLOATS) +                                     \
     (size_t)SSD_WSPPO_SPLITS(SSD_WSPPO_WINDOW_ROWS(M, Q, T)) * ((16 + (C)) * 4 * (C) + 4 * (C)))
int ssd_ws_policy_ppo_grad(const float *weights, int32_t num_sets, int32_t cell_size, int32_t variant, int32_t agent_id,
                           int32_t seq_len, const float *obs, const float *state, const uint8_t *starts, const float *actions,
                           const float *logp_old, const float *advantages, const float *value_targets, const float *vf_preds,
                           const float *behaviour_dist, int32_t n_steps, int32_t num_seqs, double clip_param,
                           double vf_clip_param, double vf_loss_coeff, double entropy_coeff, double kl_coeff, float *scratch,
                           float *grads, double *stats, int32_t device_id, uint32_t flags, void *stream);

/* ======================================================================================================================
 * WATERSHED A3C LOSS AND GRADIENTS -- ssd_ws_policy_ac_grad, the A3C twin of ssd_ws_policy_ppo_grad: the reference's A3C loss
 * (algorithms/a3c_causal.py:28-46), which every Watershed launcher offers next to PPO (run_scripts/
 * train_watershed_baseline.py:173-187), on one agent id's sequences with truncated backpropagation through time.  It is the
 * call above with another row loss and another last step, exactly as A3C LOSS AND GRADIENTS is to the other policies' PPO
 * calls: the same kernels compiled with the A3C row terms, the same host code (csrc/ssd_ws_policy_grad.hip; DESIGN.md
 * section 22).  Added after ABI 6 without a version bump: the call is additive.  With advantages = V-trace's pg_advantages
 * and value_targets = vs it is the IMPALA loss (V-TRACE TARGETS; ssd_ws_policy_forward_seq below gives the target policy's
 * values and log-probabilities).
 *
 * Network, rows [M, Q], the gathered obs, the state rule with starts, windows of seq_len, tiles, groups, chunks and splits,
 * the order of every sum, the scratch (SSD_WSPPO_SCRATCH_FLOATS: one buffer serves both calls) and its alignment, and the
 * 1 + 3 per window + 1 launches: exactly those of WATERSHED PPO LOSS AND GRADIENTS.  logp_old, vf_preds and behaviour_dist
 * are not inputs, and there are no clip or KL hyper-parameters.
 *
 * Row loss, in float32 in this order.
 *   comm agent:   exactly the row terms of A3C LOSS AND GRADIENTS with A = 5 (the same device code), a = actions[row] clamped
 *     to 0 .. 4.
 *   action agent: with a = actions[row] (the unclipped sample), (mean, log_std) = dist[0:2]:
 *       sd = expf(log_std)            z = (a - mean) / sd
 *       logp = ((-0.5f * (z * z)) - log_std) - 0.9189385f        ent = log_std + 1.4189385f
 *       pi = -(logp * adv)            d1 = value - vt            vf = 0.5f * (d1 * d1)
 *       row_loss = (pi + vf_loss_coeff * vf) - entropy_coeff * ent
 *       d row_loss / d mean = -adv * (z / sd)        d row_loss / d log_std = (-adv * (z * z - 1.f)) - entropy_coeff
 *       d row_loss / d dist[2:5] = 0 exactly         d row_loss / d value = vf_loss_coeff * d1
 * The loss is the SUM of row_loss over the M Q rows (the reference reduces with reduce_sum).  No clip kinks; ReLU's
 * derivative at 0 is 0.
 *
 * Arithmetic and order: the PPO call's.  The one difference is the last step: the float64 total of an entry is rounded to
 * float32 as it is, without the division by the rows.  No atomics: the same inputs give the same bits.
 *
 * Outputs.  grads f32 [SSD_WSP_SET_FLOATS(C)], padding floats zero.  stats f64 [4]: the SUMS of row_loss, pi, vf and ent (the
 * reference's total_loss, policy_loss, vf_loss and policy_entropy).
 *
 * SSD_E_INVALID before anything is launched (ssd_policy_last_error says why) for everything ssd_ws_policy_ppo_grad refuses,
 * less the arguments that are gone: the required per-row pointers are obs, state, actions, advantages and value_targets, the
 * hyper-parameters that must be finite are vf_loss_coeff and entropy_coeff.
 * ====================================================================================================================== */
int ssd_ws_policy_ac_grad(const float *weights, int32_t num_sets, int32_t cell_size, int32_t variant, int32_t agent_id,
                          int32_t seq_len, const float *obs, const float *state, const uint8_t *starts, const float *actions,
                          const float *advantages, const float *value_targets, int32_t n_steps, int32_t num_seqs,
                          double vf_loss_coeff, double entropy_coeff, float *scratch, float *grads, double *stats,
                          int32_t device_id, uint32_t flags, void *stream);

/* ======================================================================================================================
 * WATERSHED SEQUENCE FORWARD -- ssd_ws_policy_forward_seq: one agent id's sequences under the CURRENT weights, without
 * gradient, in ONE launch: what V-trace needs of the target policy (dist, value, the log-probability of the taken action and
 * the bootstrap value) when the weights have moved since the rollout ran (csrc/ssd_ws_policy_seq.hip).
 * It replaces M + 1 chained launches of ssd_ws_policy_forward, each of which reads and writes the state through memory.
 * Added after ABI 6 without a version bump: the call is additive.
 *
 * Network, weight layout, (variant, agent_id) and the heads: WATERSHED POLICY ROLLOUTS.  Rows: M = n_steps own steps of
 * Q = num_seqs sequences, as WATERSHED PPO LOSS AND GRADIENTS.  Inputs: obs f32 [M, Q, 12], state f32 [ceil(M / T), Q, 2, C]
 * (T = seq_len), starts u8 [M, Q] or NULL, actions f32 [M, Q] or NULL, obs_next f32 [Q, 12] or NULL (the observation after
 * the last own step), start_next u8 [Q] or NULL.  Outputs, each may be NULL: dist f32 [M, Q, 5], value f32 [M, Q], logp f32
 * [M, Q] (needs actions), bootstrap_value f32 [Q] (needs obs_next), state_out f32 [Q, 2, C].  A NULL output is not written.
 *
 * State rule: that of the loss calls.  Step m of sequence q uses state[m / T] as stored when m % T == 0 (starts[m] is NOT
 * looked at there), zero when m % T != 0 and starts[m, q] != 0, otherwise the (h', c') this call computed for step m - 1.
 * The bootstrap row runs one more step on obs_next with the state step M - 1 computed, zero where start_next[q] != 0, and
 * never a state entry (not even when M % T == 0).  state_out is the state after step M - 1; the bootstrap step changes nothing.
 *
 * logp: the rollouts' expression of the taken action under the current dist.  A comm agent: l_a - (m + logf(s)) with
 * a = (int)actions[row] clamped to 0 .. 4, m the maximal logit and s the float32 sum of expf(l_k - m) over k ascending.  An
 * action agent: ((-0.5f * (z * z)) - log_std) - 0.9189385f with z = (a - mean) / expf(log_std) on the unclipped sample.
 *
 * Arithmetic: the header's exact float32, every fmaf chain in ascending k.  dist, value and the state equal, bit for bit,
 * what ssd_ws_policy_forward gives when it is chained step by step under the same rule; with unchanged weights on a fresh
 * rollout's rows of one id, dist, value and logp give back what the rollout recorded.
 *
 * One workgroup of 4 C threads per tile of SSD_WSPPO_TILE sequences, persistent over tiles g, g + G, ... with
 * G = SSD_WSPPO_GROUPS(Q); h stays in LDS and c in registers across all steps.  One launch on `stream`, no scratch, no
 * allocation, no synchronisation.  SSD_E_INVALID before anything is launched (ssd_policy_last_error says why) for an unknown
 * variant, a num_sets that is not the variant's, an agent_id outside 0 .. num_sets - 1, a cell_size other than 64, 128 or 256,
 * seq_len, n_steps or num_seqs < 1, more than 2^31 - 17 rows with the bootstrap's, a NULL weights, obs or state, logp without
 * actions, bootstrap_value without obs_next, a misaligned float buffer, flags other than 0.
 * ====================================================================================================================== */
int ssd_ws_policy_forward_seq(const float *weights, int32_t num_sets, int32_t cell_size, int32_t variant, int32_t agent_id,
                              int32_t seq_len, const float *obs, const float *state, const uint8_t *starts,
                              const float *actions, const float *obs_next, const uint8_t *start_next, int32_t n_steps,
                              int32_t num_seqs, float *dist, float *value, float *logp, float *bootstrap_value,
                              float *state_out, int32_t device_id, uint32_t flags, void *stream);

/* ======================================================================================================================
 * SEQUENCE FORWARD -- ssd_policy_lstm_forward_seq, ssd_policy_moa_forward_seq: a sampled fragment of the recurrent or of the
 * MOA policy under the CURRENT weights, without gradient, in one call: what V-trace needs of the target policy (logits, value
 * and the bootstrap value) when the weights have moved since the rollout ran (csrc/ssd_policy_seq.hip; DESIGN.md section
 * 23).  It replaces K + 1 chained calls of ssd_policy_lstm_forward / ssd_policy_moa_forward, each a trunk launch and a cell
 * launch (two for the MOA policy) that read and write the carried state through memory.  Added after ABI 6 without a version
 * bump: the calls are additive.
 *
 * Network, weight layout and cell rule: RECURRENT POLICY ROLLOUTS and MOA POLICY ROLLOUTS.  Of the MOA policy only the
 * actions branch runs -- the conv, FC stack 0, the actions LSTM and its heads --, which is all that logits and value depend
 * on: prev_actions is no argument, and rows 2 and 3 (h2, c2) of a state entry, the MOA cell and the counterfactual
 * predictions are not touched.
 *
 * Rows: K = n_steps steps of E = num_envs envs and N = num_agents agents, in windows of T = seq_len steps, as RECURRENT PPO
 * LOSS AND GRADIENTS.  Inputs: obs_first u8 [E, N, 15, 15, 3] or NULL, obs u8 [R, E, N, 15, 15, 3], state f32
 * [ceil(K / T), E, N, 2, C] (the MOA call: [ceil(K / T), E, N, 4, C]), done u8 [K, E, N] or NULL.  Row k reads obs_first for
 * k = 0 and obs[k - 1] otherwise, and the bootstrap row reads obs[K - 1] (R >= K); with obs_first NULL row k reads obs[k] and
 * the bootstrap row obs[K] (R >= K + 1).  All of this is by address, as the loss calls read their rows.  Outputs, each may be
 * NULL: logits f32 [K, E, N, A], value f32 [K, E, N], bootstrap_value f32 [E, N], state_out f32 [E, N, 2, C] (the cell's two
 * rows in the state's order: (c, h) for the recurrent policy, (h1, c1) for the MOA policy).  A NULL output is not written.
 *
 * State rule: that of the loss calls.  Step k uses state[k / T] as stored when k % T == 0 (done is NOT looked at there),
 * otherwise the state this call computed for step k - 1, zero where done[k - 1, e, n] != 0.  The bootstrap row runs one more
 * step on the carried state with the start rule of done[K - 1], and never takes a state entry (not even when K % T == 0).
 * state_out is the state after step K - 1; the bootstrap step changes nothing.
 *
 * Arithmetic: the per-step forwards', every sum in their order on the same device pieces.  logits, value, bootstrap_value and
 * state_out equal, bit for bit, what ssd_policy_lstm_forward / ssd_policy_moa_forward give when they are chained step by step
 * under the same rule.
 *
 * Scratch and launches.  features is caller scratch of feature_rows rows of 32 floats, at least one window's and the
 * bootstrap's: (min(T, K) + 1) E N rows.  The call works in chunks of as many whole windows as the scratch holds, the
 * bootstrap row with the last window.  A chunk is two launches: the trunk over the chunk's rows (ssd_policy_kernel up to fc2;
 * FC stack 0 alone for the MOA policy) -- two launches where obs_first splits the rows, in the first chunk --, then one cell
 * launch over (tile of 16 envs, agent, window): a workgroup of 4 C threads walks its window's steps with h in LDS and c in
 * registers, and the last window's workgroup the bootstrap row after them.  The outputs do not depend on feature_rows.
 * Everything runs on `stream`: no allocation, no synchronisation.
 *
 * SSD_E_INVALID before anything is launched (ssd_policy_last_error says why) for everything the per-step forwards refuse (a
 * NULL weights, obs, state or features; misaligned weights; a cell_size other than 64, 128 or 256; num_agents outside 1 .. 64,
 * for the MOA call 2 .. 16; num_sets other than 1 or num_agents; num_actions outside 1 .. 15; flags other than 0; a device
 * that does not exist), for a misaligned float buffer, seq_len, n_steps or num_envs < 1, more than 2^31 - 17 rows with the
 * bootstrap's, and a feature_rows below the minimum.
 * ====================================================================================================================== */
int ssd_policy_lstm_forward_seq(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size, int32_t seq_len,
                                const uint8_t *obs_first, const uint8_t *obs, const float *state, const uint8_t *done,
                                int32_t n_steps, int32_t num_envs, int32_t num_agents, float *features, int64_t feature_rows,
                                float *logits, float *value, float *bootstrap_value, float *state_out, int32_t device_id,
                                uint32_t flags, void *stream);
int ssd_policy_moa_forward_seq(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size, int32_t seq_len,
                               const uint8_t *obs_first, const uint8_t *obs, const float *state, const uint8_t *done,
                               int32_t n_steps, int32_t num_envs, int32_t num_agents, float *features, int64_t feature_rows,
                               float *logits, float *value, float *bootstrap_value, float *state_out, int32_t device_id,
                               uint32_t flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif
