"""Shared counter-based PRNG of the engine (host mirror).

The reference draws from two global Mersenne Twisters by *sequence position*
(`map_env.py:422`, `harvest.py:101`, `cleanup.py:139,145,150`,
`map_env.py:656,666`), which no parallel kernel can reproduce.  The engine
instead keys every draw on *what it is for*:

    draw = H(seed, env, episode, t, stream, index)

`H` is a chain of one 32-bit bijective mixer ("triple32", Wellons) absorbing
one word at a time: ``h <- mix32(h ^ word)``.  The (seed, env, episode) prefix
is folded once per reset into a per-env key; (t, stream) once per phase; only
the last `mix32` is paid per draw.  The HIP kernels (csrc/ssd_device.hpp), the
C oracle (oracle/ssd_oracle.c) and this file are three independent statements
of the same function; tests/test_prng.py pins them against each other.

Streams (the `index` word is given in brackets):
    SPAWN_POINT [agent << 16 | cell]  reset, t = 0   (replaces map_env.py:656)
    SPAWN_ROT   [agent]               reset, t = 0   (replaces map_env.py:666)
    MOVE        [i]   Fisher-Yates position i = n-1..1 (replaces map_env.py:422)
    APPLE       [cell]                (replaces harvest.py:101, cleanup.py:139)
    WASTE_COIN  [cell]                (replaces cleanup.py:150)
    WASTE_ORDER [cell]                (replaces cleanup.py:145)
    ACTION      [agent]               random-action rollouts (rollout.py:65)
    SEASON      [0]                   Watershed reset, t = 0: the season, randint(draw, 108)
                                      (replaces watershedOrderedComm.py:69; once per (env, episode))
    POLICY      [agent]               policy rollouts: the sampled action of the conv-FC policy (policy.py), drawn with
                                      the (episode, t) of the state the action is taken in
    POLICY      [agent], [agent + 16] Watershed policy rollouts (ws_policy_draws): d1 picks a comm agent's message or, with
                                      d2, makes an action agent's normal deviate (Box-Muller); t = round * P + phase - 1
`cell` is `row * W + col`; `t` is 0 for reset and k for the k-th step after it.
"""

import numpy as np

M32 = 0xFFFFFFFF
H0 = 0x243F6A88

S_SPAWN_POINT = 1
S_SPAWN_ROT = 2
S_MOVE = 3
S_APPLE = 4
S_WASTE_COIN = 5
S_WASTE_ORDER = 6
S_ACTION = 7
S_SEASON = 8
S_POLICY = 9


def mix32(x):
    """triple32: 32-bit bijection with low avalanche bias (scalar ints)."""
    x &= M32
    x ^= x >> 17
    x = (x * 0xED5AD4BB) & M32
    x ^= x >> 11
    x = (x * 0xAC4C1B51) & M32
    x ^= x >> 15
    x = (x * 0x31848BAB) & M32
    x ^= x >> 14
    return x


def env_key(seed, env, episode):
    """Per-env, per-episode key: absorbs seed_lo, seed_hi, env, episode."""
    h = H0
    for w in (seed & M32, (seed >> 32) & M32, env & M32, episode & M32):
        h = mix32(h ^ w)
    return h


def phase_key(key, t, stream):
    return mix32(mix32(key ^ (t & M32)) ^ stream)


def draw(pkey, index):
    """One uniform u32."""
    return mix32(pkey ^ (index & M32))


def draw_full(seed, env, episode, t, stream, index):
    return draw(phase_key(env_key(seed, env, episode), t, stream), index)


def randint(u32, n):
    """Uniform integer in [0, n) from one u32 (multiply-shift, no rejection)."""
    return (u32 * n) >> 32


def threshold(p):
    """Smallest T with (k / 2**32 < p)  <=>  (k < T) for every u32 k.

    `p * 2**32` is exact in float64 (power-of-two scaling), so the ceiling is
    exact too.  p <= 0 -> 0 (never), p >= 1 -> 2**32 (always; callers clamp).
    """
    import math
    if p <= 0.0:
        return 0
    return min(int(math.ceil(p * 4294967296.0)), 1 << 32)


# ---- vectorised forms (numpy uint32 arrays), used by host-side action generation ----

def mix32_np(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(17)
    x = (x * np.uint64(0xED5AD4BB)) & M32
    x ^= x >> np.uint64(11)
    x = (x * np.uint64(0xAC4C1B51)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x31848BAB)) & M32
    x ^= x >> np.uint64(14)
    return x


def random_actions(seed, env_ids, episodes, t, num_agents, num_actions):
    """Actions the ACTION stream yields for step `t` (same as the device kernel).

    env_ids, episodes: int arrays [E].  Returns int32 [E, num_agents].
    """
    env_ids = np.asarray(env_ids, dtype=np.uint64)
    episodes = np.asarray(episodes, dtype=np.uint64)
    h = np.full(env_ids.shape, H0, dtype=np.uint64)
    h = mix32_np(h ^ np.uint64(seed & M32))
    h = mix32_np(h ^ np.uint64((seed >> 32) & M32))
    h = mix32_np(h ^ (env_ids & M32))
    h = mix32_np(h ^ (episodes & M32))
    pk = mix32_np(mix32_np(h ^ np.uint64(t & M32)) ^ np.uint64(S_ACTION))
    idx = np.arange(num_agents, dtype=np.uint64)[None, :]
    u = mix32_np(pk[:, None] ^ idx)
    return ((u * np.uint64(num_actions)) >> np.uint64(32)).astype(np.int32)


def policy_uniforms(seed, env_ids, episodes, t, num_agents):
    """u = (draw >> 8) * 2^-24 of the POLICY stream, float32 [E, num_agents]: the uniform a policy rollout compares with the
    cumulative softmax (include/ssd.h).  env_ids are global env indices; episodes, t: the state's, per env (scalars or [E])."""
    env_ids = np.asarray(env_ids, dtype=np.uint64)
    episodes = np.broadcast_to(np.asarray(episodes, dtype=np.uint64), env_ids.shape)
    t = np.broadcast_to(np.asarray(t, dtype=np.uint64), env_ids.shape)
    h = np.full(env_ids.shape, H0, dtype=np.uint64)
    h = mix32_np(h ^ np.uint64(seed & M32))
    h = mix32_np(h ^ np.uint64((seed >> 32) & M32))
    h = mix32_np(h ^ (env_ids & M32))
    h = mix32_np(h ^ (episodes & M32))
    pk = mix32_np(mix32_np(h ^ (t & M32)) ^ np.uint64(S_POLICY))
    idx = np.arange(num_agents, dtype=np.uint64)[None, :]
    d = mix32_np(pk[:, None] ^ idx)
    return ((d >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def ws_policy_draws(seed, env_ids, episodes, t, agent):
    """(d1, d2) = H(.., POLICY, agent), H(.., POLICY, agent + 16) of a Watershed policy rollout, uint32 arrays shaped like
    env_ids (global env indices); episodes, t (= round * P + phase - 1 of the state acted in) and agent (the acting agent's
    id): scalars or arrays of that shape."""
    env_ids = np.asarray(env_ids, dtype=np.uint64)
    episodes = np.broadcast_to(np.asarray(episodes, dtype=np.uint64), env_ids.shape)
    t = np.broadcast_to(np.asarray(t, dtype=np.uint64), env_ids.shape)
    agent = np.broadcast_to(np.asarray(agent, dtype=np.uint64), env_ids.shape)
    h = np.full(env_ids.shape, H0, dtype=np.uint64)
    h = mix32_np(h ^ np.uint64(seed & M32))
    h = mix32_np(h ^ np.uint64((seed >> 32) & M32))
    h = mix32_np(h ^ (env_ids & M32))
    h = mix32_np(h ^ (episodes & M32))
    pk = mix32_np(mix32_np(h ^ (t & M32)) ^ np.uint64(S_POLICY))
    d1 = mix32_np(pk ^ agent)
    d2 = mix32_np(pk ^ (agent + np.uint64(16)))
    return d1.astype(np.uint32), d2.astype(np.uint32)


def ws_uniforms(d1, d2):
    """(u, u1, u2) float32 of the draws above: u = (d1 >> 8) * 2^-24 in [0, 1) for the categorical pick; u1 = ((d1 >> 8) + 1) *
    2^-24 in (0, 1] and u2 = (d2 >> 8) * 2^-24 for the normal deviate (include/ssd.h)."""
    k1 = np.asarray(d1, np.uint32) >> np.uint32(8)
    k2 = np.asarray(d2, np.uint32) >> np.uint32(8)
    s = np.float32(2.0 ** -24)
    return ((k1.astype(np.float32) * s).astype(np.float32), ((k1 + np.uint32(1)).astype(np.float32) * s).astype(np.float32),
            (k2.astype(np.float32) * s).astype(np.float32))
