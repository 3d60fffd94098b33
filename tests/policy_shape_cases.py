"""The shapes, inputs and exact constructions that test_policy_shapes_gpu.py runs on the device and test_policy_shapes_cpu.py
checks on the host: NumPy only, seeded by the case, so both files see the same numbers.

The tile of every policy kernel is 16 batch rows of one agent index (csrc/ssd_policy_device.hpp, kTile), so B = 1 has no full
tile, 15 is one row short, 16 exact, 17 one row over and 33 two tiles and a row.
"""
import numpy as np

import policy_lstm_ref
import policy_moa_ref
import policy_ref

TILE = 16
FLAT = 1014

# (B, N, P, A): every B of {1, 15, 16, 17, 33}, N of {1, 2, 64}, P = 1 and P = N (64 sets once), A of {1, 2, 15} and the game's 8
CONV_CASES = [(1, 2, 2, 15), (15, 1, 1, 2), (16, 2, 1, 8), (17, 2, 2, 8), (17, 64, 64, 8), (33, 2, 2, 1), (33, 64, 1, 15)]
# (B, N, P, A, C): 64 sets at C = 64 only; one set at C = 256
LSTM_CASES = [(1, 2, 2, 15, 64), (17, 12, 12, 1, 128), (33, 1, 1, 15, 256), (17, 64, 64, 15, 64), (33, 2, 1, 1, 256),
              (17, 12, 1, 15, 64)]
# (N, A, C, B, P): 225 prediction columns over 4 and over 16 waves; string order != index order (N >= 11); one partial tile
MOA_CASES = [(16, 15, 64, 17, 16), (16, 15, 256, 1, 1), (11, 8, 64, 33, 11), (12, 9, 128, 17, 1), (3, 2, 64, 33, 3),
             (2, 1, 64, 17, 2)]


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def random_obs(rng, B, N):
    return rng.integers(0, 256, (B, N, 15, 15, 3), dtype=np.uint8)


def random_starts(rng, B, N):
    """bool [B, N], about a third set; and where the shape has them: the tile (rows 0..15, agent 0) starts in every row, the
    tile (rows 0..15, agent 1) and the tile (rows 16..31, agent 0) in none."""
    s = rng.random((B, N)) < 0.3
    s[:TILE, 0] = True
    if N > 1:
        s[:TILE, 1] = False
    if B >= 2 * TILE:
        s[TILE:2 * TILE, 0] = False
    return s


def conv_inputs(case):
    B, N, P, A = case
    rng = _rng(1, *case)
    return policy_ref.random_weights(rng, P, A), random_obs(rng, B, N)


def lstm_inputs(case):
    B, N, P, A, C = case
    rng = _rng(2, *case)
    w = policy_lstm_ref.random_weights(rng, P, A, C)
    return w, random_obs(rng, B, N), rng.standard_normal((B, N, 2, C)).astype(np.float32), random_starts(rng, B, N)


def moa_inputs(case):
    N, A, C, B, P = case
    rng = _rng(3, *case)
    w = policy_moa_ref.random_weights(rng, P, A, N, C)
    state = (rng.standard_normal((B, N, 4, C)) * 0.5).astype(np.float32)
    prev = rng.integers(0, A, (B, N)).astype(np.int32)
    acts = rng.integers(0, A, (B, N)).astype(np.int32)
    return w, random_obs(rng, B, N), prev, state, random_starts(rng, B, N), acts


def error_ratio(got, tor, ref):
    """(ek, et, ek / (4 et + 1e-6)): the kernel's and the float32 torch module's largest error against the float64 restatement,
    and how much of the project's bound ek <= 4 et + 1e-6 the kernel uses."""
    ek = float(np.abs(np.asarray(got, np.float64) - ref).max())
    et = float(np.abs(np.asarray(tor, np.float64) - ref).max())
    return ek, et, ek / (4 * et + 1e-6)


# ------------------------------------------------------------------------------------------------ the selector construction
# Every sum of the network has ONE non-zero term: conv_w is a single +-1 at (dy, dx, c, f), fc1_w has a single 1 per used hidden
# unit at flat index k = (y 13 + x) 6 + f, fc2_w is the identity, and the heads route one hidden unit to each output.  Output j
# of a row is then float32(max(+-(u8 - 128) / 255, 0)) of the observation byte [y + dy, x + dx, c], whatever the order of any sum.

SELECTOR_A = 15
SELECTOR_OUTPUTS = SELECTOR_A + 1          # 15 logits and the value


def selector_sets():
    """66 weight-set plans {f, dy, dx, c, ks[16], units[16]}: filter f's 169 flat indices k = pos 6 + f in 11 sets of 16 (the
    last set of a filter wraps round to its first positions).  Set s takes its conv tap from s, and its hidden units j 2 + s
    (mod 32), so both 16-column halves of fc1 carry outputs of every set."""
    sets = []
    for f in range(6):
        for chunk in range(11):
            s = len(sets)
            pos = [(chunk * 16 + j) % 169 for j in range(SELECTOR_OUTPUTS)]
            dy, rest = divmod(s % 27, 9)
            dx, c = divmod(rest, 3)
            sets.append({"f": f, "dy": dy, "dx": dx, "c": c, "ks": [p * 6 + f for p in pos],
                         "units": [(2 * j + s) % 32 for j in range(SELECTOR_OUTPUTS)]})
    return sets


def selector_coverage(sets):
    return sorted({k for s in sets for k in s["ks"]})


def selector_weights(sets, sign):
    """policy_ref-style float64 weights of P = len(sets) sets and A = 15 for the plans `sets`; the conv tap is `sign` (+-1)."""
    P, A = len(sets), SELECTOR_A
    w = {"conv_w": np.zeros((P, 3, 3, 3, 6)), "conv_b": np.zeros((P, 6)), "fc1_w": np.zeros((P, FLAT, 32)), "fc1_b": np.zeros((P, 32)),
         "fc2_w": np.tile(np.eye(32), (P, 1, 1)), "fc2_b": np.zeros((P, 32)), "logits_w": np.zeros((P, 32, A)),
         "logits_b": np.zeros((P, A)), "value_w": np.zeros((P, 32, 1)), "value_b": np.zeros((P, 1))}
    for p, s in enumerate(sets):
        w["conv_w"][p, s["dy"], s["dx"], s["c"], s["f"]] = float(sign)
        for j, (k, n) in enumerate(zip(s["ks"], s["units"])):
            w["fc1_w"][p, k, n] = 1.0
            if j < A:
                w["logits_w"][p, n, j] = 1.0
            else:
                w["value_w"][p, n, 0] = 1.0
    return w


def selector_expected(sets, sign, obs):
    """(logits f32 [B, N, 15], value f32 [B, N]) of obs u8 [B, N = len(sets), 15, 15, 3], from the bytes alone."""
    B, N = obs.shape[:2]
    assert N == len(sets)
    out = np.zeros((B, N, SELECTOR_OUTPUTS), np.float32)
    for i, s in enumerate(sets):
        for j, k in enumerate(s["ks"]):
            pos, f = divmod(k, 6)
            assert f == s["f"]
            y, x = divmod(pos, 13)
            byte = obs[:, i, y + s["dy"], x + s["dx"], s["c"]].astype(np.float64)
            v = ((byte - 128.0) / 255.0).astype(np.float32)          # the network's input: float32 of the float64 quotient
            out[:, i, j] = np.maximum(np.float32(sign) * v, np.float32(0)) + np.float32(0)      # (+ 0: no negative zero)
    return out[..., :SELECTOR_A].copy(), out[..., SELECTOR_A].copy()


# ------------------------------------------------------------------------------------------------- the integer construction
# conv_w = 0 and conv_b small positive integers: the conv's output is conv_b[f] at every position, whatever the observation.
# fc1, fc2 and the heads have small integer weights and biases of both signs, none of fc1's zero, so every partial sum is an
# integer far below 2^24: float32 holds each exactly in any order of summation, and the result is the int64 one.

def integer_weights(P, A, seed=0):
    """int64 arrays in policy_ref's layout [P, ...]."""
    rng = _rng(4, P, A, seed)
    nz = np.array([-3, -2, -1, 1, 2, 3])
    return {"conv_w": np.zeros((P, 3, 3, 3, 6), np.int64), "conv_b": rng.integers(1, 4, (P, 6)),
            "fc1_w": nz[rng.integers(0, 6, (P, FLAT, 32))], "fc1_b": rng.integers(-40, 41, (P, 32)),
            "fc2_w": rng.integers(-2, 3, (P, 32, 32)), "fc2_b": rng.integers(-50, 51, (P, 32)),
            "logits_w": rng.integers(-2, 3, (P, 32, A)), "logits_b": rng.integers(-5, 6, (P, A)),
            "value_w": rng.integers(-2, 3, (P, 32, 1)), "value_b": rng.integers(-5, 6, (P, 1))}


def integer_layers(wi, p):
    """Set p's layers in int64: [(input [K], weights [K, J], bias [J], pre-activation [J]), ...] for fc1, fc2, logits, value."""
    h = wi["conv_b"][p][np.arange(FLAT) % 6]                          # the conv's output in the flatten order (row, col, channel)
    out = []
    for name, relu in (("fc1", True), ("fc2", True)):
        z = h @ wi[name + "_w"][p] + wi[name + "_b"][p]
        out.append((h, wi[name + "_w"][p], wi[name + "_b"][p], z))
        h = np.maximum(z, 0)
    for name in ("logits", "value"):
        out.append((h, wi[name + "_w"][p], wi[name + "_b"][p], h @ wi[name + "_w"][p] + wi[name + "_b"][p]))
    return out


def integer_expected(wi, B, N):
    """(logits i64 [B, N, A], value i64 [B, N], fc2's output i64 [B, N, 32]): every batch row of an agent is the same."""
    P = wi["conv_b"].shape[0]
    A = wi["logits_w"].shape[-1]
    logits, value, feat = np.zeros((B, N, A), np.int64), np.zeros((B, N), np.int64), np.zeros((B, N, 32), np.int64)
    for i in range(N):
        layers = integer_layers(wi, 0 if P == 1 else i)
        logits[:, i], value[:, i], feat[:, i] = layers[2][3], layers[3][3][0], layers[2][0]
    return logits, value, feat
