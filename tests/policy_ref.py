"""A float64 NumPy restatement of the reference's policy network, models/conv_to_fc_net.py:1-51 (ConvToFCNet), written
from that file, plus the value head RLlib's v1 Model puts on its last hidden layer.  Independent of torch and of the package's
policy module: the CPU and GPU tests hold both the module and the kernel against it.

Weights: dict of float64 arrays with a leading weight-set axis P, in TF's layouts --
conv_w [P,3,3,3,6] (kh, kw, c_in, c_out), conv_b [P,6], fc1_w [P,1014,32], fc1_b [P,32], fc2_w [P,32,32], fc2_b [P,32],
logits_w [P,32,A], logits_b [P,A], value_w [P,32,1], value_b [P,1].
"""
import numpy as np


def normalise(obs_u8):
    """The observation the network sees: (u8 - 128) / 255 in float64 (map_env.py:199)."""
    return (np.asarray(obs_u8).astype(np.float64) - 128.0) / 255.0


def conv_relu(x, w, b):
    """conv_to_fc_net.py:27-33: tf conv, 6 filters, kernel [3, 3], stride 1, VALID padding, ReLU.  x [M,15,15,3] -> [M,13,13,6]."""
    M, H, W, _ = x.shape
    out = np.zeros((M, H - 2, W - 2, w.shape[-1]), np.float64)
    for dy in range(3):
        for dx in range(3):
            out += np.einsum("mhwc,cf->mhwf", x[:, dy:dy + H - 2, dx:dx + W - 2, :], w[dy, dx])
    return np.maximum(out + b, 0.0)


def forward_set(weights, p, x):
    """One weight set p on normalised observations x [M,15,15,3] -> (logits [M,A], value [M])."""
    h = conv_relu(x, weights["conv_w"][p], weights["conv_b"][p])
    h = h.reshape(h.shape[0], -1)                                         # flatten (:34): row, col, channel
    h = np.maximum(h @ weights["fc1_w"][p] + weights["fc1_b"][p], 0.0)    # fc1 (:36-44), ReLU
    h = np.maximum(h @ weights["fc2_w"][p] + weights["fc2_b"][p], 0.0)    # fc2
    logits = h @ weights["logits_w"][p] + weights["logits_b"][p]          # fc_out (:45-50), no activation
    value = (h @ weights["value_w"][p] + weights["value_b"][p])[:, 0]     # value_function() on last_layer
    return logits, value


def forward(weights, obs_u8):
    """obs u8 [..., N, 15, 15, 3]; agent i uses set i when there are N sets, set 0 when there is one."""
    obs_u8 = np.asarray(obs_u8)
    P = weights["conv_w"].shape[0]
    N = obs_u8.shape[-4]
    lead = obs_u8.shape[:-3]
    x = normalise(obs_u8).reshape(-1, N, 15, 15, 3)
    A = weights["logits_w"].shape[-1]
    logits = np.zeros((x.shape[0], N, A))
    value = np.zeros((x.shape[0], N))
    for i in range(N):
        logits[:, i], value[:, i] = forward_set(weights, 0 if P == 1 else i, x[:, i])
    return logits.reshape(lead + (A,)), value.reshape(lead)


def random_weights(rng, P, A, scale=1.0):
    """Random weights of every parameter (biases too), sized so that every ReLU is sometimes on and sometimes off."""
    shapes = {"conv_w": (3, 3, 3, 6), "conv_b": (6,), "fc1_w": (1014, 32), "fc1_b": (32,), "fc2_w": (32, 32), "fc2_b": (32,),
              "logits_w": (32, A), "logits_b": (A,), "value_w": (32, 1), "value_b": (1,)}
    fan = {"conv_w": 27, "fc1_w": 1014, "fc2_w": 32, "logits_w": 32, "value_w": 32}
    out = {}
    for k, s in shapes.items():
        std = scale / np.sqrt(fan.get(k, 4))
        out[k] = rng.standard_normal((P,) + s) * std
    return out
