"""The sequence forwards (include/ssd.h, SEQUENCE FORWARD) without a GPU: what ssd_policy_lstm_forward_seq
and ssd_policy_moa_forward_seq refuse and in which words -- every check comes before the device is looked at, so a call whose
arguments are good is told apart by the one refusal that is left, "no such HIP device" for device_id -1 --, the two symbols in
header, bindings and library, the size of the scratch evaluate_fragment keeps for the call, and one_call=True on CPU tensors,
which has no effect."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from a3c_ref import as_numpy_u32
from impala_ref import HYPER, INFLUENCE_WEIGHT, MOA_WEIGHT, edge, edge_batch
from sequential_social_dilemma_games_amd import _capi, evaluate_fragment, impala_loss, impala_loss_moa, impala_loss_recurrent
from sequential_social_dilemma_games_amd import policy as policy_module

KINDS = ("lstm", "moa")
ROWS = {"lstm": 2, "moa": 4}
A_, CS, T_, K_, E_, N_ = 8, 64, 2, 3, 2, 2
NO_DEVICE = "no such HIP device"
REQUIRED = "weights, obs, state and features are required"
ALIGNED = "float buffers must be 4-byte aligned"
TOO_SMALL = "feature_rows must hold one window and the bootstrap row: (min(seq_len, n_steps) + 1) * num_envs * num_agents"
TOO_MANY = "at most 2^31 - 17 rows, the bootstrap's included"

# host memory nothing will read: the checks look at null and alignment only, and device_id -1 refuses what passes them
BUF = np.zeros(4096, dtype=np.uint8)
BASE = BUF.ctypes.data + (-BUF.ctypes.data) % 8


def good(kind):
    """The arguments of a call that passes every check but the device's, by name."""
    p = lambda n: BASE + 64 * n                                   # noqa: E731
    return dict(weights=p(0), num_sets=N_, num_actions=A_, cell_size=CS, seq_len=T_, obs_first=p(1), obs=p(2), state=p(3), done=p(4),
                n_steps=K_, num_envs=E_, num_agents=N_, features=p(5), feature_rows=(min(T_, K_) + 1) * E_ * N_, logits=p(6),
                value=p(7), bootstrap_value=p(8), state_out=p(9), device_id=-1, flags=0, stream=None)


def call(kind, **changes):
    L = _capi.lib()
    fn = L.ssd_policy_moa_forward_seq if kind == "moa" else L.ssd_policy_lstm_forward_seq
    rc = fn(*dict(good(kind), **changes).values())
    return rc, L.ssd_policy_last_error().decode()


def refusals(kind):
    odd = BASE + 2
    agents = [(0, "num_agents must be 1..64"), (65, "num_agents must be 1..64")] if kind == "lstm" else \
        [(1, "the MOA policy needs 2..16 agents"), (17, "the MOA policy needs 2..16 agents")]
    out = [(dict(weights=None), REQUIRED), (dict(obs=None), REQUIRED), (dict(state=None), REQUIRED), (dict(features=None), REQUIRED),
           (dict(weights=odd), "weights must be 4-byte aligned"),
           (dict(cell_size=100), "cell_size must be 64, 128 or 256"), (dict(cell_size=0), "cell_size must be 64, 128 or 256"),
           (dict(num_sets=3), "num_sets must be 1 or num_agents"), (dict(num_sets=0), "num_sets must be 1 or num_agents"),
           (dict(num_actions=0), "num_actions must be 1..15"), (dict(num_actions=16), "num_actions must be 1..15"),
           (dict(seq_len=0), "seq_len must be >= 1"), (dict(seq_len=-3), "seq_len must be >= 1"),
           (dict(n_steps=0), "n_steps and num_envs must be >= 1"), (dict(num_envs=0), "n_steps and num_envs must be >= 1"),
           (dict(num_envs=-1), "n_steps and num_envs must be >= 1"),
           (dict(n_steps=2 ** 20, num_envs=2 ** 10, feature_rows=2 ** 40), TOO_MANY),
           (dict(n_steps=2 ** 31 - 17, num_envs=1, num_agents=2 if kind == "moa" else 1, num_sets=1, feature_rows=2 ** 40), TOO_MANY),
           (dict(feature_rows=(min(T_, K_) + 1) * E_ * N_ - 1), TOO_SMALL), (dict(feature_rows=0), TOO_SMALL),
           (dict(feature_rows=-8), TOO_SMALL),
           (dict(seq_len=8, feature_rows=(K_ + 1) * E_ * N_ - 1), TOO_SMALL),          # T > K: the whole fragment and the bootstrap
           (dict(flags=1), "flags must be 0"), (dict(flags=0x80000000), "flags must be 0")]
    out += [(dict(num_agents=n, num_sets=1), words) for n, words in agents]
    out += [(dict([(name, odd)]), ALIGNED) for name in ("state", "features", "logits", "value", "bootstrap_value", "state_out")]
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_good_arguments_pass_every_check_but_the_devices(kind):
    """... also with every optional pointer null, at the largest row count, and with the scratch at its minimum."""
    assert call(kind) == (_capi.SSD_E_INVALID, NO_DEVICE)
    none = dict(obs_first=None, done=None, logits=None, value=None, bootstrap_value=None, state_out=None)
    assert call(kind, **none) == (_capi.SSD_E_INVALID, NO_DEVICE)
    n = 2 if kind == "moa" else 1                                 # (n_steps + 1) * num_envs * num_agents = 2^31 - 17, or one row below
    most = dict(n_steps=(2 ** 31 - 17) // n - 1, num_envs=1, num_agents=n, num_sets=1, seq_len=1, feature_rows=2 * n)
    assert call(kind, **most) == (_capi.SSD_E_INVALID, NO_DEVICE)
    assert call(kind, seq_len=8, feature_rows=(K_ + 1) * E_ * N_) == (_capi.SSD_E_INVALID, NO_DEVICE)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_and_their_words(kind):
    for changes, words in refusals(kind):
        assert call(kind, **changes) == (_capi.SSD_E_INVALID, words), changes


def test_two_bad_arguments_speak_in_the_order_of_the_checks():
    for kind in KINDS:
        assert call(kind, weights=None, flags=1)[1] == REQUIRED
        assert call(kind, cell_size=1, seq_len=0)[1] == "cell_size must be 64, 128 or 256"
        assert call(kind, seq_len=0, n_steps=0)[1] == "seq_len must be >= 1"
        assert call(kind, feature_rows=0, flags=1)[1] == TOO_SMALL
        assert call(kind, flags=1, device_id=-1)[1] == "flags must be 0"


def test_header_python_and_library_agree():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "ssd.h")).read()
    for token in (" * SEQUENCE FORWARD -- ", "int ssd_policy_lstm_forward_seq(", "int ssd_policy_moa_forward_seq(", "#define SSD_ABI_VERSION 6"):
        assert token in hdr, token
    assert _capi.FORWARD_SEQ_SYMBOLS == ("ssd_policy_lstm_forward_seq", "ssd_policy_moa_forward_seq")
    L = _capi.lib()
    for name in _capi.FORWARD_SEQ_SYMBOLS:
        assert name in _capi.SYMBOLS and hasattr(L, name)
        decl = hdr[hdr.index("int %s(" % name):]
        decl = decl[:decl.index(");")]
        assert len(getattr(L, name).argtypes) == decl.count(",") + 1 == len(good("lstm")), name
        assert "int64_t feature_rows" in decl and getattr(L, name).argtypes[13] is C.c_int64


@pytest.mark.parametrize("kind", KINDS)
def test_the_scratch_is_the_fragment_or_whole_windows_within_the_loss_calls(kind):
    """_seq_scratch_rows: the whole fragment and the bootstrap row where that is no more than the loss call's scratch for the
    batch, else 1 + a multiple of T steps that fits in it, and at least one window and the bootstrap row."""
    pol, _, _ = edge_batch(kind, edge(1, 2, "none"), E=1)
    for K, E, T in ((1, 1, 2), (4, 17, 2), (128, 64, 16), (128, 4096, 16), (1000, 4096, 16), (1000, 4096, 1000), (5000, 64, 7)):
        N = 5
        rows = policy_module._seq_scratch_rows(pol, (K, E, N), T)
        limit = pol.ppo_scratch_shape(K, E, N, T)[0] // 32
        whole, least = (K + 1) * E * N, (min(T, K) + 1) * E * N
        assert rows % (E * N) == 0 and least <= rows <= whole, (K, E, T)
        if whole <= limit:
            assert rows == whole, (K, E, T)
        else:
            steps = rows // (E * N)
            assert (steps - 1) % T == 0 and (rows <= limit or rows == least), (K, E, T)
            assert rows + T * E * N > limit, (K, E, T)               # and no window more would fit


def _bits_equal(a, b):
    return all(x.shape == y.shape and np.array_equal(as_numpy_u32(x), as_numpy_u32(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ("fc",) + KINDS)
def test_one_call_on_cpu_tensors_gives_the_host_paths_results(kind):
    case = edge(5, 2, "per_env", seed=21)
    pol, t, first = edge_batch(kind, case, E=3)
    T = case[1]
    want = evaluate_fragment(pol, t, first, T)
    assert _bits_equal(want, evaluate_fragment(pol, t, first, T, one_call=True))
    assert _bits_equal(want, evaluate_fragment(pol, t, first, seq_len=T, one_call=True))
    if kind == "moa":                                             # on the CPU the MOA step still reads prev_actions
        with pytest.raises(ValueError, match="prev_actions must be a contiguous torch.int32 tensor"):
            evaluate_fragment(pol, {k: v for k, v in t.items() if k != "prev_actions"}, first, T, one_call=True)

    def loss(**kw):
        pol.zero_grad()
        if kind == "fc":
            out, stats = impala_loss(pol, t, obs_first=first, **HYPER)
        elif kind == "lstm":
            out, stats = impala_loss_recurrent(pol, t, seq_len=T, obs_first=first, **HYPER, **kw)
        else:
            out, stats = impala_loss_moa(pol, t, seq_len=T, moa_weight=MOA_WEIGHT, influence_weight=INFLUENCE_WEIGHT, obs_first=first,
                                         **HYPER, **kw)
        out.backward()
        return [out.detach()] + [v for v in stats.values()] + [p.grad.clone() for p in pol.parameters() if p.grad is not None]

    if kind != "fc":
        assert _bits_equal(loss(), loss(one_call=True))
    else:
        with pytest.raises(TypeError):
            impala_loss(pol, t, obs_first=first, one_call=True, **HYPER)           # the conv-FC call has no such keyword
