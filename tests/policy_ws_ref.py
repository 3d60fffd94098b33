"""Float64 NumPy restatement of the Watershed policy's contract (include/ssd.h, WATERSHED POLICY ROLLOUTS).

Test infrastructure: written from the header, independent of the torch module and of the kernel.  A weight dict holds one
array per block with a leading weight-set axis (one set per agent id), in Keras' layouts: dense0_w [S,12,16], dense0_b [S,16],
dense1_w [S,16,16] ([4,16,16] when the comm layer is shared: entry id % 4), dense1_b, lstm_kernel [S,16,4C], lstm_recurrent
[S,C,4C], lstm_bias [S,4C], out_w [S,C,5], out_b [S,5], value_w [S,C,1], value_b [S,1].
"""
import numpy as np

OBS_W, X, OUT = 12, 16, 5


def num_sets(variant):
    return 4 if int(variant) == 0 else 8


def obs_len(variant, local_obs, agent):
    base = 4 if local_obs else 7
    if int(variant) == 0:
        return base + 1
    return base + 4 if agent < 4 else base + 5


def random_weights(rng, variant, C, share=False, scale=1.0):
    """Weights of a size that keeps every layer's output O(1) on engine observations (flows up to a few hundred)."""
    S = num_sets(variant)
    D1 = 4 if share else S
    n = lambda *shape: rng.standard_normal(shape)                # noqa: E731
    w = {"dense0_w": n(S, OBS_W, X) * 0.01, "dense0_b": n(S, X) * 0.1,
         "dense1_w": n(D1, X, X) * 0.3, "dense1_b": n(D1, X) * 0.1,
         "lstm_kernel": n(S, X, 4 * C) * 0.3, "lstm_recurrent": n(S, C, 4 * C) * (1.0 / np.sqrt(C)), "lstm_bias": n(S, 4 * C) * 0.2,
         "out_w": n(S, C, OUT) * (scale * 2.0 / np.sqrt(C)), "out_b": n(S, OUT) * 0.2,
         "value_w": n(S, C, 1) * (2.0 / np.sqrt(C)), "value_b": n(S, 1) * 0.2}
    return {k: v.astype(np.float32) for k, v in w.items()}


def random_obs(rng, variant, local_obs, agent):
    """Observation rows shaped like the engine's for the given acting agents: values up to a few hundred, zero padding beyond
    the agent's observation length."""
    agent = np.asarray(agent)
    obs = rng.uniform(-1.0, 160.0, agent.shape + (OBS_W,)).astype(np.float32)
    n = np.array([obs_len(variant, local_obs, i) for i in range(num_sets(variant))])[agent]
    obs[np.arange(OBS_W) >= n[..., None]] = 0.0
    return obs


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def forward(w, obs, agent, state, starts=None):
    """obs [B,12], agent [B], state [B,2,C] (h, c), starts [B] or None -> (dist [B,5], value [B], new state [B,2,C]), float64.
    Row b uses weight set agent[b]; a start row's state is zero whatever it holds."""
    w = {k: np.asarray(v, np.float64) for k, v in w.items()}
    obs, state, agent = np.asarray(obs, np.float64), np.asarray(state, np.float64), np.asarray(agent).astype(np.int64)
    B, C = obs.shape[0], state.shape[-1]
    dist, value, new = np.zeros((B, OUT)), np.zeros(B), state.copy()
    for b in range(B):
        i = int(agent[b])
        h, c = state[b, 0], state[b, 1]
        if starts is not None and starts[b]:
            h, c = np.zeros(C), np.zeros(C)
        i1 = i % w["dense1_w"].shape[0]
        d0 = np.maximum(obs[b] @ w["dense0_w"][i] + w["dense0_b"][i], 0.0)
        d1 = np.maximum(d0 @ w["dense1_w"][i1] + w["dense1_b"][i1], 0.0)
        z = d1 @ w["lstm_kernel"][i] + h @ w["lstm_recurrent"][i] + w["lstm_bias"][i]
        zi, zf, zg, zo = z[:C], z[C:2 * C], z[2 * C:3 * C], z[3 * C:]
        c2 = sigmoid(zf) * c + sigmoid(zi) * np.tanh(zg)
        h2 = sigmoid(zo) * np.tanh(c2)
        dist[b] = h2 @ w["out_w"][i] + w["out_b"][i]
        value[b] = (h2 @ w["value_w"][i])[0] + w["value_b"][i][0]
        new[b, 0], new[b, 1] = h2, c2
    return dist, value, new


def start_rule(variant, rnd, phase):
    """The header's start rule, restated: round 0, and for SeqComm not the comm agents' second message (phases 5-8)."""
    rnd, phase = np.asarray(rnd), np.asarray(phase)
    if int(variant) == 0:
        return rnd == 0
    return (rnd == 0) & ~((phase >= 5) & (phase <= 8))
