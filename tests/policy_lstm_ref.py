"""A float64 NumPy restatement of the baseline's recurrent policy: the conv-FC trunk of models/conv_to_fc_net.py (policy_ref.py)
under RLlib 0.7.6's LSTM wrapper, as include/ssd.h states it.  Independent of torch and of the package's policy module.

The cell is TF's LSTMCell / BasicLSTMCell: z = [x, h] @ lstm_w + lstm_b, split into (i, j, f, o) in that order,
c' = sigmoid(f + 1) c + sigmoid(i) tanh(j), h' = sigmoid(o) tanh(c'); the logits and the value read h'.

Weights: the trunk's arrays of policy_ref.py (conv_w ... fc2_b) and lstm_w [P, 32 + C, 4C], lstm_b [P, 4C], logits_w [P, C, A],
logits_b [P, A], value_w [P, C, 1], value_b [P, 1].  A state is [..., 2, C]: c, then h.
"""
import numpy as np

from policy_ref import conv_relu, normalise


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def features_set(weights, p, x):
    """fc2's output of weight set p on normalised observations x [M,15,15,3] -> [M,32]."""
    h = conv_relu(x, weights["conv_w"][p], weights["conv_b"][p]).reshape(x.shape[0], -1)
    h = np.maximum(h @ weights["fc1_w"][p] + weights["fc1_b"][p], 0.0)
    return np.maximum(h @ weights["fc2_w"][p] + weights["fc2_b"][p], 0.0)


def cell(weights, p, x, c, h):
    """One LSTM step of set p: x [M,32], c, h [M,C] -> (c', h')."""
    C = c.shape[-1]
    z = np.concatenate([x, h], axis=-1) @ weights["lstm_w"][p] + weights["lstm_b"][p]
    i, j, f, o = z[:, :C], z[:, C:2 * C], z[:, 2 * C:3 * C], z[:, 3 * C:]
    c2 = sigmoid(f + 1.0) * c + sigmoid(i) * np.tanh(j)
    return c2, sigmoid(o) * np.tanh(c2)


def forward(weights, obs_u8, state, starts=None):
    """obs u8 [..., N, 15, 15, 3], state [..., N, 2, C], starts bool [..., N] or None -> (logits [..., N, A], value [..., N],
    new state [..., N, 2, C]).  Agent i uses set i when there are N sets, set 0 when there is one; a starting row's state is
    taken as zero whatever it holds."""
    obs_u8 = np.asarray(obs_u8)
    P = weights["conv_w"].shape[0]
    N = obs_u8.shape[-4]
    lead = obs_u8.shape[:-3]
    C = weights["lstm_w"].shape[-1] // 4
    A = weights["logits_w"].shape[-1]
    x = normalise(obs_u8).reshape(-1, N, 15, 15, 3)
    st = np.asarray(state, np.float64).reshape(-1, N, 2, C).copy()
    if starts is not None:
        st[np.asarray(starts, bool).reshape(-1, N)] = 0.0
    M = x.shape[0]
    logits, value, out = np.zeros((M, N, A)), np.zeros((M, N)), np.zeros((M, N, 2, C))
    for i in range(N):
        p = 0 if P == 1 else i
        c2, h2 = cell(weights, p, features_set(weights, p, x[:, i]), st[:, i, 0], st[:, i, 1])
        logits[:, i] = h2 @ weights["logits_w"][p] + weights["logits_b"][p]
        value[:, i] = (h2 @ weights["value_w"][p] + weights["value_b"][p])[:, 0]
        out[:, i, 0], out[:, i, 1] = c2, h2
    return logits.reshape(lead + (A,)), value.reshape(lead), out.reshape(lead + (2, C))


def random_weights(rng, P, A, C, scale=1.0):
    """Random weights of every parameter (biases too): the trunk's as policy_ref.random_weights, the cell's sized so that the
    gates are neither saturated nor constant."""
    from policy_ref import random_weights as trunk_weights
    w = trunk_weights(rng, P, A, scale)
    for k in ("logits_w", "logits_b", "value_w", "value_b"):
        del w[k]
    w["lstm_w"] = rng.standard_normal((P, 32 + C, 4 * C)) * scale / np.sqrt(32 + C)
    w["lstm_b"] = rng.standard_normal((P, 4 * C)) * 0.5
    w["logits_w"] = rng.standard_normal((P, C, A)) * scale / np.sqrt(C)
    w["logits_b"] = rng.standard_normal((P, A)) * 0.5
    w["value_w"] = rng.standard_normal((P, C, 1)) * scale / np.sqrt(C)
    w["value_b"] = rng.standard_normal((P, 1)) * 0.5
    return w
