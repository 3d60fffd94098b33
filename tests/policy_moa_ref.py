"""A float64 NumPy restatement of the causal-influence policy of run_scripts/train_moa.py (MOA_LSTM, models/moa_model.py:121-311)
and its social-influence reward (algorithms/common_funcs.py:134-195), as include/ssd.h states them.  Written from those files and
the Keras (TF 2.0) LSTM semantics, independent of torch and of the package's policy module.

Per weight set: the conv of policy_ref.py (ReLU), flatten (row, col, channel); two FC stacks 1014 -> 32 -> 32 with tanh
(moa_model.py:44-56, 185-196; RLlib's default fcnet_activation); a Keras LSTM of C cells on the actions stack (logits and value
on its output) and one on [MOA stack, the N previous actions] (moa_model.py:57-62) followed by pred C -> (N-1) A.
Keras LSTM: z = x @ kernel + h @ recurrent + bias, gate blocks (i, f, c, o), c' = sig(f) c + sig(i) tanh(c~), h' = sig(o)
tanh(c'); the state of a row is (h1, c1, h2, c2).  The previous actions of row i are agent i's, then the others' in the order
of their ids sorted as strings (map_env.py:202).  Counterfactual a: the MOA step with the own slot replaced by a
(moa_model.py:239-244).
"""
import numpy as np

from policy_ref import conv_relu, normalise


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def others(N):
    """Row i: the agents other than i, ids sorted as strings ('agent-10' < 'agent-2')."""
    order = sorted(range(N), key=lambda n: "agent-%d" % n)
    return [[n for n in order if n != i] for i in range(N)]


def keras_lstm(x, h, c, kernel, recurrent, bias):
    C = h.shape[-1]
    z = x @ kernel + h @ recurrent + bias
    i, f, cc, o = z[..., :C], z[..., C:2 * C], z[..., 2 * C:3 * C], z[..., 3 * C:]
    c2 = sigmoid(f) * c + sigmoid(i) * np.tanh(cc)
    return sigmoid(o) * np.tanh(c2), c2


def stacks(w, p, x):
    """Both FC stacks' outputs of set p on normalised observations x [M,15,15,3] -> ([M,32], [M,32])."""
    h = conv_relu(x, w["conv_w"][p], w["conv_b"][p]).reshape(x.shape[0], -1)
    out = []
    for s in ("a", "m"):
        y = np.tanh(h @ w[s + "_fc1_w"][p] + w[s + "_fc1_b"][p])
        out.append(np.tanh(y @ w[s + "_fc2_w"][p] + w[s + "_fc2_b"][p]))
    return out


def forward(w, obs_u8, prev_actions, state, starts=None):
    """obs u8 [..., N, 15, 15, 3], prev_actions [..., N], state [..., N, 4, C], starts bool [..., N] or None ->
    (logits [..., N, A], value [..., N], moa_logits [..., N, N-1, A], cf_logits [..., N, A, N-1, A], state [..., N, 4, C])."""
    obs_u8 = np.asarray(obs_u8)
    P = w["conv_w"].shape[0]
    N = obs_u8.shape[-4]
    lead = obs_u8.shape[:-3]
    C = w["lstm_recurrent"].shape[-2]
    A = w["logits_w"].shape[-1]
    x = normalise(obs_u8).reshape(-1, N, 15, 15, 3)
    M = x.shape[0]
    st = np.asarray(state, np.float64).reshape(M, N, 4, C).copy()
    prev = np.asarray(prev_actions).reshape(M, N).astype(np.float64)
    s = np.zeros((M, N), bool) if starts is None else np.asarray(starts, bool).reshape(M, N)
    st[s] = 0.0
    oth = others(N)
    logits, value = np.zeros((M, N, A)), np.zeros((M, N))
    cf, out = np.zeros((M, N, A, N - 1, A)), np.zeros((M, N, 4, C))
    moa = np.zeros((M, N, N - 1, A))
    for i in range(N):
        p = 0 if P == 1 else i
        ya, ym = stacks(w, p, x[:, i])
        h1, c1 = keras_lstm(ya, st[:, i, 0], st[:, i, 1], w["lstm_kernel"][p], w["lstm_recurrent"][p], w["lstm_bias"][p])
        logits[:, i] = h1 @ w["logits_w"][p] + w["logits_b"][p]
        value[:, i] = (h1 @ w["value_w"][p] + w["value_b"][p])[:, 0]
        acts = np.concatenate([prev[:, i:i + 1], prev[:, oth[i]]], axis=1)
        acts[s[:, i]] = 0.0                                      # a starting row's whole vector is zero
        mk, mr, mb = w["moa_kernel"][p], w["moa_recurrent"][p], w["moa_bias"][p]
        h2, c2 = keras_lstm(np.concatenate([ym, acts], axis=1), st[:, i, 2], st[:, i, 3], mk, mr, mb)
        moa[:, i] = (h2 @ w["pred_w"][p] + w["pred_b"][p]).reshape(M, N - 1, A)
        for a in range(A):
            ca = acts.copy()
            ca[:, 0] = a
            hc, _ = keras_lstm(np.concatenate([ym, ca], axis=1), st[:, i, 2], st[:, i, 3], mk, mr, mb)
            cf[:, i, a] = (hc @ w["pred_w"][p] + w["pred_b"][p]).reshape(M, N - 1, A)
        out[:, i] = np.stack([h1, c1, h2, c2], axis=1)
    return (logits.reshape(lead + (A,)), value.reshape(lead), moa.reshape(lead + (N - 1, A)),
            cf.reshape(lead + (A, N - 1, A)), out.reshape(lead + (4, C)))


def softmax(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def kl_div(p, q):
    """common_funcs.py:49-67 for one row: sum over the last axis of p log(p / q) where p != 0; non-finite -> 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = np.sum(np.where(p != 0, p * np.log(p / q), 0), axis=-1)
    return kl if np.all(np.isfinite(kl)) else np.zeros(kl.shape)


def influence(logits, cf_logits, actions, clip=10.0):
    """The discrete influence reward of rows [R]: logits [R, A], cf_logits [R, A, N-1, A], actions [R].  For each row:
    p = softmax(cf[a_t]) [N-1, A], q = sum_a pi(a) softmax(cf[a]) -- the marginal of common_funcs.py's
    marginalize_predictions_over_own_actions for discrete actions -- and clip(sum_j kl_div(p_j, q_j))."""
    logits = np.asarray(logits, np.float64)
    cf = np.asarray(cf_logits, np.float64)
    out = np.zeros(logits.shape[0])
    for r in range(logits.shape[0]):
        pi = softmax(logits[r])
        probs = softmax(cf[r])                                   # [A, N-1, A]
        p = probs[int(actions[r])]
        q = np.einsum("a,ajk->jk", pi, probs)
        out[r] = np.clip(np.sum(kl_div(p, q)), -clip, clip)
    return out


def moa_loss(moa_logits, actions, weight=1.0):
    """Mean over rows and other agents of the cross-entropy of moa_logits [..., N, N-1, A] against the others' actions [..., N]
    of the same step, times weight."""
    moa = np.asarray(moa_logits, np.float64)
    N, A = moa.shape[-3], moa.shape[-1]
    acts = np.asarray(actions).reshape(-1, N)
    lg = moa.reshape(-1, N, N - 1, A)
    oth = others(N)
    total, count = 0.0, 0
    for m in range(lg.shape[0]):
        for i in range(N):
            for j, n in enumerate(oth[i]):
                row = lg[m, i, j]
                lse = row.max() + np.log(np.exp(row - row.max()).sum())
                total += lse - row[acts[m, n]]
                count += 1
    return total / count * weight


def random_weights(rng, P, A, N, C, scale=1.0):
    """Random weights of every parameter (biases too), sized so that the tanh layers and the gates are neither saturated nor
    constant."""
    w = {"conv_w": rng.standard_normal((P, 3, 3, 3, 6)) * scale / np.sqrt(27), "conv_b": rng.standard_normal((P, 6)) * 0.2}
    for s in ("a", "m"):
        w[s + "_fc1_w"] = rng.standard_normal((P, 1014, 32)) * scale / np.sqrt(1014)
        w[s + "_fc1_b"] = rng.standard_normal((P, 32)) * 0.2
        w[s + "_fc2_w"] = rng.standard_normal((P, 32, 32)) * scale / np.sqrt(32)
        w[s + "_fc2_b"] = rng.standard_normal((P, 32)) * 0.2
    w["lstm_kernel"] = rng.standard_normal((P, 32, 4 * C)) * scale / np.sqrt(32 + C)
    w["lstm_recurrent"] = rng.standard_normal((P, C, 4 * C)) * scale / np.sqrt(32 + C)
    w["lstm_bias"] = rng.standard_normal((P, 4 * C)) * 0.5
    w["logits_w"] = rng.standard_normal((P, C, A)) * scale / np.sqrt(C)
    w["logits_b"] = rng.standard_normal((P, A)) * 0.5
    w["value_w"] = rng.standard_normal((P, C, 1)) * scale / np.sqrt(C)
    w["value_b"] = rng.standard_normal((P, 1)) * 0.5
    w["moa_kernel"] = rng.standard_normal((P, 32 + N, 4 * C)) * scale / np.sqrt(32 + C)
    w["moa_kernel"][:, 32:] /= 4.0                               # the action inputs run to A - 1
    w["moa_recurrent"] = rng.standard_normal((P, C, 4 * C)) * scale / np.sqrt(32 + C)
    w["moa_bias"] = rng.standard_normal((P, 4 * C)) * 0.5
    w["pred_w"] = rng.standard_normal((P, C, (N - 1) * A)) * scale * 2.0 / np.sqrt(C)
    w["pred_b"] = rng.standard_normal((P, (N - 1) * A)) * 0.5
    return w
