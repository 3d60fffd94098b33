"""ctypes binding of libssd_hip.so (the C ABI declared in include/ssd.h).

There is no fallback: if the shared library is missing or cannot be loaded this module
raises, and every product entry point (engine, envs, bench) fails with it.
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
# SSD_LIB_PATH lets tools/phase_profile.py load the diagnostic (stamped) build of the SAME sources, and the tests that need
# test hooks the test-hook build (libssd_hip_testhooks.so: the product sources with -DSSD_TESTHOOKS).
LIB_PATH = os.environ.get("SSD_LIB_PATH") or os.path.join(_PKG, "libssd_hip.so")

SSD_OK, SSD_E_INVALID, SSD_E_DEVICE, SSD_E_NOMEM, SSD_E_STATE = 0, -1, -2, -3, -4
SSD_HOST_PTRS, SSD_NO_ROTATE, SSD_OBS_F32, SSD_ROLLOUT_FUSED, SSD_AUTO_RESET, SSD_ROLLOUT_AUTO = 1, 2, 4, 8, 16, 128
SSD_POLICY_GREEDY = 256
SSD_PATH_AQL, SSD_PATH_COHERENT, SSD_PATH_SPLIT, SSD_PATH_FUSED, SSD_PATH_SYNC, SSD_PATH_QUEUE_DROPPED, SSD_PATH_FORKED = 1, 2, 4, 8, 16, 32, 64
SSD_PATH_PAIRS = 128
SSD_PATH_RUN_SHIFT = 20            # bits 20..23: the longest run of steps one launch of the call took
SSD_ST_BAD_ACTION, SSD_ST_NO_SPAWN, SSD_ST_MOVE_LOOKUP, SSD_ST_WAIT_TIMEOUT = 1, 2, 4, 8
ABI_VERSION = 6
SSD_WS_SEQ, SSD_WS_SEQ_COMM = 0, 1
SSD_WS_DONE_AGENT, SSD_WS_DONE_ALL, SSD_WS_END, SSD_WS_REW_INT, SSD_WS_REW_F64 = 1, 2, 4, 8, 16
SSD_ST_NOT_RESET = 16
SSD_WS_OBS_WIDTH = 12
SSD_STATS_KEEP = 1
SSD_ADV_GAE, SSD_ADV_CRITIC = 1, 2
# the policy network's weight layout (include/ssd.h, SSD_POL_*): float offsets within one weight set
SSD_S_POLICY = 9
SSD_POL_VIEW, SSD_POL_CONV_OUT, SSD_POL_FILTERS, SSD_POL_HIDDEN, SSD_POL_FLAT, SSD_POL_MAX_ACTIONS = 15, 13, 6, 32, 1014, 15
SSD_POL_CONV_W, SSD_POL_CONV_B, SSD_POL_FC1_W, SSD_POL_FC1_B = 0, 162, 168, 32616
SSD_POL_FC2_W, SSD_POL_FC2_B, SSD_POL_VALUE_W, SSD_POL_VALUE_B, SSD_POL_LOGITS_W = 32648, 33672, 33704, 33736, 33740


def SSD_POL_LOGITS_B(num_actions):
    return SSD_POL_LOGITS_W + 32 * int(num_actions)


def SSD_POL_SET_FLOATS(num_actions):
    return (SSD_POL_LOGITS_W + 33 * int(num_actions) + 63) // 64 * 64


# the PPO loss-and-gradient call's partial sums (include/ssd.h, SSD_PPO_*)
SSD_PPO_TILE, SSD_PPO_STAT_FLOATS, SSD_PPO_MAX_GROUPS = 16, 16, 1024


def SSD_PPO_GROUPS(set_rows, num_sets):
    return min((int(set_rows) + SSD_PPO_TILE - 1) // SSD_PPO_TILE, SSD_PPO_MAX_GROUPS // int(num_sets))


def SSD_PPO_SCRATCH_FLOATS(set_rows, num_sets, num_actions):
    return int(num_sets) * SSD_PPO_GROUPS(set_rows, num_sets) * (SSD_POL_SET_FLOATS(num_actions) + SSD_PPO_STAT_FLOATS)


# the recurrent PPO loss-and-gradient call's partial sums and scratch (include/ssd.h, SSD_RPPO_*)
SSD_RPPO_TILE, SSD_RPPO_CHUNK, SSD_RPPO_MAX_SPLITS = 16, 64, 32


def SSD_RPPO_SEQS(E, N, P):
    return int(E) * int(N) // int(P)


def SSD_RPPO_GROUPS(seqs, num_sets):
    return min((int(seqs) + SSD_RPPO_TILE - 1) // SSD_RPPO_TILE, SSD_PPO_MAX_GROUPS // int(num_sets))


def SSD_RPPO_SPLITS(window_set_rows):
    return min((int(window_set_rows) + SSD_RPPO_CHUNK - 1) // SSD_RPPO_CHUNK, SSD_RPPO_MAX_SPLITS)


def SSD_RPPO_ROW_FLOATS(C):
    return 64 + 6 * int(C)


def SSD_RPPO_SCRATCH_FLOATS(K, E, N, P, A, C, T):
    K, E, N, P, C, T = int(K), int(E), int(N), int(P), int(C), int(T)
    seqs = SSD_RPPO_SEQS(E, N, P)
    rows = min(T, K) * seqs
    return (P * (32 + C) * 4 * C + min(T, K) * E * N * SSD_RPPO_ROW_FLOATS(C)
            + P * SSD_PPO_GROUPS(rows, P) * (SSD_LSTM_W + SSD_PPO_STAT_FLOATS)
            + P * SSD_RPPO_GROUPS(seqs, P) * (16 * C + 16 + SSD_PPO_STAT_FLOATS)
            + P * SSD_RPPO_SPLITS(rows) * ((32 + C) * 4 * C + 4 * C))


# the MOA PPO loss-and-gradient call's partial sums and scratch (include/ssd.h, SSD_MPPO_*)
SSD_MPPO_TILE, SSD_MPPO_CHUNK, SSD_MPPO_MAX_SPLITS = 16, 64, 32
SSD_MPPO_GROUPS, SSD_MPPO_SPLITS = SSD_RPPO_GROUPS, SSD_RPPO_SPLITS


def SSD_MPPO_PRED_PITCH(A, N):
    return ((int(N) - 1) * int(A) + 15) // 16 * 16


def SSD_MPPO_ROW_FLOATS(C, A, N):
    return 128 + 6 * int(C) + SSD_MPPO_PRED_PITCH(A, N)


def SSD_MPPO_SCRATCH_FLOATS(K, E, N, P, A, C, T):
    K, E, N, P, A, C, T = int(K), int(E), int(N), int(P), int(A), int(C), int(T)
    seqs = SSD_RPPO_SEQS(E, N, P)
    rows = min(T, K) * seqs
    return (P * (80 + 2 * C) * 4 * C + min(T, K) * E * N * SSD_MPPO_ROW_FLOATS(C, A, N)
            + P * SSD_PPO_GROUPS(rows, P) * (SSD_MOA_LSTM_W(C) + SSD_PPO_STAT_FLOATS)
            + P * SSD_MPPO_GROUPS(seqs, P) * (16 * C + 16 + SSD_PPO_STAT_FLOATS)
            + P * SSD_MPPO_SPLITS(rows) * ((80 + 2 * C) * 4 * C + 8 * C + (C + 1) * SSD_MPPO_PRED_PITCH(A, N)))


# the recurrent policy's weight layout (include/ssd.h, SSD_LSTM_*): the trunk at the SSD_POL_* offsets, then these blocks
SSD_LSTM_W, SSD_LSTM_X, SSD_LSTM_MAX_CELLS = 33728, 32, 256
LSTM_CELL_SIZES = (64, 128, 256)


def SSD_LSTM_ALIGN(n):
    return (int(n) + 63) // 64 * 64


def SSD_LSTM_B(C):
    return SSD_LSTM_ALIGN(SSD_LSTM_W + (32 + int(C)) * 4 * int(C))


def SSD_LSTM_VALUE_W(C):
    return SSD_LSTM_ALIGN(SSD_LSTM_B(C) + 4 * int(C))


def SSD_LSTM_VALUE_B(C):
    return SSD_LSTM_ALIGN(SSD_LSTM_VALUE_W(C) + int(C))


def SSD_LSTM_LOGITS_W(C):
    return SSD_LSTM_ALIGN(SSD_LSTM_VALUE_B(C) + 1)


def SSD_LSTM_LOGITS_B(C, A):
    return SSD_LSTM_ALIGN(SSD_LSTM_LOGITS_W(C) + int(C) * int(A))


def SSD_LSTM_SET_FLOATS(C, A):
    return SSD_LSTM_ALIGN(SSD_LSTM_LOGITS_B(C, A) + int(A))


# the MOA policy's weight layout (include/ssd.h, SSD_MOA_*): the trunk's conv, two FC stacks, the actions LSTM with its heads,
# the MOA LSTM with pred
SSD_MOA_FC, SSD_MOA_FC_STRIDE, SSD_MOA_X, SSD_MOA_XM, SSD_MOA_MAX_AGENTS = 33728, 33536, 32, 48, 16
SSD_MOA_ALIGN = SSD_LSTM_ALIGN


def SSD_MOA_FC1_W(s):
    return SSD_MOA_FC + int(s) * SSD_MOA_FC_STRIDE


def SSD_MOA_FC1_B(s):
    return SSD_MOA_FC1_W(s) + (SSD_POL_FC1_B - SSD_POL_FC1_W)


def SSD_MOA_FC2_W(s):
    return SSD_MOA_FC1_W(s) + (SSD_POL_FC2_W - SSD_POL_FC1_W)


def SSD_MOA_FC2_B(s):
    return SSD_MOA_FC1_W(s) + (SSD_POL_FC2_B - SSD_POL_FC1_W)


def SSD_MOA_LSTM_W(C):
    return SSD_MOA_FC + 2 * SSD_MOA_FC_STRIDE


def SSD_MOA_LSTM_B(C):
    return SSD_MOA_ALIGN(SSD_MOA_LSTM_W(C) + (32 + int(C)) * 4 * int(C))


def SSD_MOA_VALUE_W(C):
    return SSD_MOA_ALIGN(SSD_MOA_LSTM_B(C) + 4 * int(C))


def SSD_MOA_VALUE_B(C):
    return SSD_MOA_ALIGN(SSD_MOA_VALUE_W(C) + int(C))


def SSD_MOA_LOGITS_W(C):
    return SSD_MOA_ALIGN(SSD_MOA_VALUE_B(C) + 1)


def SSD_MOA_LOGITS_B(C, A):
    return SSD_MOA_ALIGN(SSD_MOA_LOGITS_W(C) + int(C) * int(A))


def SSD_MOA_MW(C, A):
    return SSD_MOA_ALIGN(SSD_MOA_LOGITS_B(C, A) + int(A))


def SSD_MOA_MB(C, A):
    return SSD_MOA_ALIGN(SSD_MOA_MW(C, A) + (SSD_MOA_XM + int(C)) * 4 * int(C))


def SSD_MOA_PRED_W(C, A):
    return SSD_MOA_ALIGN(SSD_MOA_MB(C, A) + 4 * int(C))


def SSD_MOA_PRED_B(C, A, N):
    return SSD_MOA_ALIGN(SSD_MOA_PRED_W(C, A) + int(C) * (int(N) - 1) * int(A))


def SSD_MOA_SET_FLOATS(C, A, N):
    return SSD_MOA_ALIGN(SSD_MOA_PRED_B(C, A, N) + (int(N) - 1) * int(A))


def SSD_MOA_SCRATCH_FLOATS(rows):
    return 82 * int(rows)


# the Watershed policy's weight layout (include/ssd.h, SSD_WSP_*): dense0, dense1, the Keras LSTM, the dist and value heads
SSD_WSP_X, SSD_WSP_OUT, SSD_WSP_D0_W, SSD_WSP_D0_B, SSD_WSP_D1_W, SSD_WSP_D1_B, SSD_WSP_LSTM_W = 16, 5, 0, 192, 256, 512, 576
SSD_WSP_ALIGN = SSD_LSTM_ALIGN


def SSD_WSP_LSTM_B(C):
    return SSD_WSP_ALIGN(SSD_WSP_LSTM_W + (16 + int(C)) * 4 * int(C))


def SSD_WSP_OUT_W(C):
    return SSD_WSP_ALIGN(SSD_WSP_LSTM_B(C) + 4 * int(C))


def SSD_WSP_OUT_B(C):
    return SSD_WSP_ALIGN(SSD_WSP_OUT_W(C) + 5 * int(C))


def SSD_WSP_VALUE_W(C):
    return SSD_WSP_ALIGN(SSD_WSP_OUT_B(C) + 5)


def SSD_WSP_VALUE_B(C):
    return SSD_WSP_ALIGN(SSD_WSP_VALUE_W(C) + int(C))


def SSD_WSP_SET_FLOATS(C):
    return SSD_WSP_ALIGN(SSD_WSP_VALUE_B(C) + 1)


# the Watershed PPO loss-and-gradient call's partial sums and scratch (include/ssd.h, SSD_WSPPO_*)
SSD_WSPPO_TILE, SSD_WSPPO_CHUNK, SSD_WSPPO_MAX_GROUPS, SSD_WSPPO_MAX_SPLITS, SSD_WSPPO_MAX_TRUNK_GROUPS = 16, 64, 1024, 32, 256


def SSD_WSPPO_GROUPS(Q):
    return min((int(Q) + SSD_WSPPO_TILE - 1) // SSD_WSPPO_TILE, SSD_WSPPO_MAX_GROUPS)


def SSD_WSPPO_SPLITS(window_rows):
    return min((int(window_rows) + SSD_WSPPO_CHUNK - 1) // SSD_WSPPO_CHUNK, SSD_WSPPO_MAX_SPLITS)


def SSD_WSPPO_TRUNK_GROUPS(window_rows):
    return min((int(window_rows) + SSD_WSPPO_TILE - 1) // SSD_WSPPO_TILE, SSD_WSPPO_MAX_TRUNK_GROUPS)


def SSD_WSPPO_ROW_FLOATS(C):
    return 48 + 6 * int(C)


def SSD_WSPPO_SCRATCH_FLOATS(M, Q, C, T):
    M, Q, C, T = int(M), int(Q), int(C), int(T)
    rows = min(T, M) * Q
    return ((16 + C) * 4 * C + rows * SSD_WSPPO_ROW_FLOATS(C) + SSD_WSPPO_TRUNK_GROUPS(rows) * SSD_WSP_LSTM_W
            + SSD_WSPPO_GROUPS(Q) * (8 * C + 8 + SSD_PPO_STAT_FLOATS) + SSD_WSPPO_SPLITS(rows) * ((16 + C) * 4 * C + 4 * C))


# the batch moments' summation order and scratch (include/ssd.h, SSD_MOM_*)
SSD_MOM_BLOCK, SSD_MOM_ITEMS = 256, 16
SSD_MOM_CHUNK = SSD_MOM_BLOCK * SSD_MOM_ITEMS


def SSD_MOM_CHUNKS(n_steps, lanes, num_sets):
    return (int(n_steps) * (int(lanes) // int(num_sets)) + SSD_MOM_CHUNK - 1) // SSD_MOM_CHUNK


def SSD_MOM_SCRATCH_DOUBLES(n_steps, lanes, num_sets):
    return 4 * int(num_sets) * SSD_MOM_CHUNKS(n_steps, lanes, num_sets)


# every symbol include/ssd.h declares
SYMBOLS = ("ssd_create", "ssd_destroy", "ssd_reset", "ssd_step", "ssd_step_random", "ssd_rollout_random", "ssd_rollout_actions", "ssd_rollout_path", "ssd_set_rollout_chains",
           "ssd_profiler_attached", "ssd_observe",
           "ssd_get_state", "ssd_set_state", "ssd_get_waste_count", "ssd_render_full", "ssd_render_frames", "ssd_agent_action_obs", "ssd_set_horizon", "ssd_potential_waste_area",
           "ssd_device_status", "ssd_synchronize", "ssd_last_error", "ssd_abi_version",
           "ssd_ws_create", "ssd_ws_destroy", "ssd_ws_reset", "ssd_ws_step", "ssd_ws_rollout_actions", "ssd_ws_info", "ssd_ws_get_state",
           "ssd_ws_set_state", "ssd_ws_device_status", "ssd_ws_last_error",
           "ssd_stats_create", "ssd_stats_destroy", "ssd_stats_fold", "ssd_stats_set_chunk", "ssd_stats_discard", "ssd_stats_drain",
           "ssd_stats_last_error", "ssd_policy_forward", "ssd_policy_last_error", "ssd_rollout_policy",
           "ssd_policy_lstm_forward", "ssd_rollout_policy_lstm", "ssd_policy_moa_forward", "ssd_rollout_policy_moa",
           "ssd_ws_policy_forward", "ssd_ws_rollout_policy", "ssd_advantages", "ssd_advantages_last_error",
           "ssd_policy_ppo_grad", "ssd_policy_lstm_ppo_grad", "ssd_policy_moa_ppo_grad",
           "ssd_policy_ac_grad", "ssd_policy_lstm_ac_grad", "ssd_policy_moa_ac_grad", "ssd_vtrace", "ssd_vtrace_last_error",
           "ssd_ws_policy_ppo_grad", "ssd_ws_policy_ac_grad", "ssd_ws_policy_forward_seq",
           "ssd_policy_lstm_forward_seq", "ssd_policy_moa_forward_seq",
           "ssd_ws_stats_create", "ssd_ws_stats_destroy", "ssd_ws_stats_attach", "ssd_ws_stats_discard", "ssd_ws_stats_drain",
           "ssd_ws_stats_last_error", "ssd_standardize", "ssd_explained_variance", "ssd_moments_last_error")
# added after ABI 6 without a version bump (the calls are additive): a library built before them lacks them
LSTM_SYMBOLS = ("ssd_policy_lstm_forward", "ssd_rollout_policy_lstm")
MOA_SYMBOLS = ("ssd_policy_moa_forward", "ssd_rollout_policy_moa")
WS_POLICY_SYMBOLS = ("ssd_ws_policy_forward", "ssd_ws_rollout_policy")
ADVANTAGES_SYMBOLS = ("ssd_advantages", "ssd_advantages_last_error")
PPO_SYMBOLS = ("ssd_policy_ppo_grad",)
LSTM_PPO_SYMBOLS = ("ssd_policy_lstm_ppo_grad",)
MOA_PPO_SYMBOLS = ("ssd_policy_moa_ppo_grad",)
A3C_SYMBOLS = ("ssd_policy_ac_grad", "ssd_policy_lstm_ac_grad", "ssd_policy_moa_ac_grad")
VTRACE_SYMBOLS = ("ssd_vtrace", "ssd_vtrace_last_error")
WS_PPO_SYMBOLS = ("ssd_ws_policy_ppo_grad",)
WS_A3C_SYMBOLS = ("ssd_ws_policy_ac_grad", "ssd_ws_policy_forward_seq")
FORWARD_SEQ_SYMBOLS = ("ssd_policy_lstm_forward_seq", "ssd_policy_moa_forward_seq")
WS_STATS_SYMBOLS = ("ssd_ws_stats_create", "ssd_ws_stats_destroy", "ssd_ws_stats_attach", "ssd_ws_stats_discard", "ssd_ws_stats_drain",
                    "ssd_ws_stats_last_error")
MOMENTS_SYMBOLS = ("ssd_standardize", "ssd_explained_variance", "ssd_moments_last_error")


class SsdConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("game", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("base_map", C.c_char_p), ("num_envs", C.c_int32), ("num_agents", C.c_int32),
                ("view_len", C.c_int32), ("beam_len", C.c_int32), ("seed", C.c_uint64),
                ("env_index_base", C.c_uint32), ("device_id", C.c_int32), ("keep_beams", C.c_int32),
                ("color_lut", C.c_void_p), ("harvest_thresholds", C.c_void_p),
                ("cleanup_apple_thresholds", C.c_void_p), ("cleanup_waste_thresholds", C.c_void_p)]


class WsConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("variant", C.c_int32), ("num_envs", C.c_int32), ("local_obs", C.c_int32),
                ("local_rew", C.c_int32), ("device_id", C.c_int32), ("seed", C.c_uint64), ("env_index_base", C.c_uint32),
                ("reserved", C.c_uint32)]


class WsState(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("season", "phase", "wrapped", "viol", "round", "episode", "hist", "f_rew", "pen",
                                                 "current_sums", "running_rew", "prev_actions")]


class SsdError(RuntimeError):
    pass


_lib = None


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7).  Two HIP
    runtimes in one process cannot both initialise the GPU, so bind libssd_hip.so to the copy torch
    will use: load it first, and the dynamic linker resolves our NEEDED entry to it by SONAME.
    Without torch installed the system runtime (/opt/rocm) is used."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return None
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        return C.CDLL(cand, mode=C.RTLD_GLOBAL)
    return None


_hip_runtime = None


def lib():
    """The loaded library; raises SsdError when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SsdError("HIP extension missing: %s (build it with `python -c 'import __graft_entry__ as g; "
                           "g.build()'` or `make -C sequential_social_dilemma_games_amd/csrc`); there is no CPU "
                           "fallback" % LIB_PATH)
        global _hip_runtime
        try:
            _hip_runtime = _preload_torch_hip_runtime()
            L = C.CDLL(LIB_PATH)
        except OSError as exc:
            raise SsdError("cannot load %s: %s (no CPU fallback)" % (LIB_PATH, exc))
        vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
        L.ssd_create.argtypes = [C.POINTER(SsdConfig), C.POINTER(vp)]
        L.ssd_destroy.argtypes = [vp]
        L.ssd_reset.argtypes = [vp, vp, vp, u32, vp]
        L.ssd_step.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp]
        L.ssd_step_random.argtypes = [vp, i32, vp, vp, vp, vp, u32, vp]
        L.ssd_rollout_random.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, i32, u32, vp]
        L.ssd_rollout_actions.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, u32, vp]
        L.ssd_profiler_attached.argtypes = []
        L.ssd_rollout_path.argtypes = [vp]
        L.ssd_set_rollout_chains.argtypes = [vp, i32]
        L.ssd_observe.argtypes = [vp, vp, u32, vp]
        L.ssd_get_state.argtypes = [vp] + [vp] * 6
        L.ssd_set_state.argtypes = [vp] + [vp] * 6
        L.ssd_get_waste_count.argtypes = [vp, vp]
        L.ssd_render_full.argtypes = [vp, i32, vp]
        L.ssd_render_frames.argtypes = [vp, i32, i32, vp, u32, vp]
        L.ssd_agent_action_obs.argtypes = [vp, vp, vp, vp, vp, u32, vp]
        L.ssd_set_horizon.argtypes = [vp, i32]
        L.ssd_potential_waste_area.argtypes = [vp]
        L.ssd_device_status.argtypes = [vp, C.POINTER(u32), C.c_int]
        L.ssd_synchronize.argtypes = [vp]
        L.ssd_last_error.argtypes = [vp]
        L.ssd_last_error.restype = C.c_char_p
        L.ssd_abi_version.argtypes = []
        L.ssd_ws_create.argtypes = [C.POINTER(WsConfig), C.POINTER(vp)]
        L.ssd_ws_destroy.argtypes = [vp]
        L.ssd_ws_reset.argtypes = [vp, vp, vp, vp, vp]
        L.ssd_ws_step.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp]
        L.ssd_ws_rollout_actions.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, i32, u32, vp]
        L.ssd_ws_info.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.ssd_ws_get_state.argtypes = [vp, C.POINTER(WsState)]
        L.ssd_ws_set_state.argtypes = [vp, C.POINTER(WsState)]
        L.ssd_ws_device_status.argtypes = [vp, C.POINTER(u32), C.c_int]
        L.ssd_ws_last_error.argtypes = [vp]
        L.ssd_ws_last_error.restype = C.c_char_p
        L.ssd_stats_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
        L.ssd_stats_destroy.argtypes = [vp]
        L.ssd_stats_fold.argtypes = [vp, vp, vp, i32, i32, i32, i32, u32, vp]
        L.ssd_stats_set_chunk.argtypes = [vp, i32]
        L.ssd_stats_discard.argtypes = [vp, vp, vp]
        L.ssd_stats_drain.argtypes = [vp] + [vp] * 7 + [u32, vp]
        L.ssd_stats_last_error.argtypes = [vp]
        L.ssd_stats_last_error.restype = C.c_char_p
        L.ssd_policy_forward.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, i32, u32, vp]
        L.ssd_policy_last_error.argtypes = []
        L.ssd_policy_last_error.restype = C.c_char_p
        L.ssd_rollout_policy.argtypes = [vp, vp, i32, vp, i32, i32] + [vp] * 7 + [i32, vp, u32, vp]
        missing = [name for name in LSTM_SYMBOLS + MOA_SYMBOLS + WS_POLICY_SYMBOLS + ADVANTAGES_SYMBOLS + PPO_SYMBOLS + LSTM_PPO_SYMBOLS + MOA_PPO_SYMBOLS + A3C_SYMBOLS + VTRACE_SYMBOLS + WS_PPO_SYMBOLS + WS_A3C_SYMBOLS + FORWARD_SEQ_SYMBOLS + WS_STATS_SYMBOLS + MOMENTS_SYMBOLS if not hasattr(L, name)]
        if missing:
            raise SsdError("%s lacks %s (built before the recurrent, MOA or Watershed policy calls, the advantages call, the PPO or A3C gradient calls, the V-trace call, the Watershed PPO gradient call, the sequence forwards, the Watershed episode statistics or the batch moments): rebuild it with `python -c 'import "
                           "__graft_entry__ as g; g.build()'`" % (LIB_PATH, ", ".join(missing)))
        L.ssd_policy_lstm_forward.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, u32, vp]
        L.ssd_rollout_policy_lstm.argtypes = [vp, vp, i32, i32, vp, i32, i32, vp, vp, i32, i32] + [vp] * 8 + [i32, vp, u32, vp]
        L.ssd_policy_moa_forward.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, i32, i32] + [vp] * 8 + [C.c_float, i32, u32, vp]
        L.ssd_rollout_policy_moa.argtypes = ([vp, vp, i32, i32, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp, C.c_float] + [vp] * 8
                                             + [i32, vp, u32, vp])
        L.ssd_ws_policy_forward.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, u32, vp]
        L.ssd_ws_rollout_policy.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32] + [vp] * 12 + [i32, vp, u32, vp]
        L.ssd_advantages.argtypes = [vp, vp, C.c_double, vp, vp, vp, i32, i32, i32, i32, C.c_double, C.c_double, u32, vp, vp, i32, vp]
        L.ssd_advantages_last_error.argtypes = []
        L.ssd_advantages_last_error.restype = C.c_char_p
        L.ssd_policy_ppo_grad.argtypes = [vp, i32, i32] + [vp] * 8 + [i32, i32, i32] + [C.c_double] * 5 + [vp, vp, vp, i32, u32, vp]
        L.ssd_policy_lstm_ppo_grad.argtypes = ([vp, i32, i32, i32, i32] + [vp] * 10 + [i32, i32, i32] + [C.c_double] * 5
                                               + [vp, vp, vp, i32, u32, vp])
        L.ssd_policy_moa_ppo_grad.argtypes = ([vp, i32, i32, i32, i32] + [vp] * 11 + [i32, i32, i32] + [C.c_double] * 6
                                              + [vp, vp, vp, i32, u32, vp])
        L.ssd_policy_ac_grad.argtypes = [vp, i32, i32] + [vp] * 5 + [i32, i32, i32] + [C.c_double] * 2 + [vp, vp, vp, i32, u32, vp]
        L.ssd_policy_lstm_ac_grad.argtypes = ([vp, i32, i32, i32, i32] + [vp] * 7 + [i32, i32, i32] + [C.c_double] * 2
                                              + [vp, vp, vp, i32, u32, vp])
        L.ssd_policy_moa_ac_grad.argtypes = ([vp, i32, i32, i32, i32] + [vp] * 8 + [i32, i32, i32] + [C.c_double] * 3
                                             + [vp, vp, vp, i32, u32, vp])
        L.ssd_vtrace.argtypes = [vp, vp, C.c_double, vp, vp, vp, vp, i32, i32, i32, i32, C.c_double, C.c_double, C.c_double, u32, vp, vp, i32, vp]
        L.ssd_vtrace_last_error.argtypes = []
        L.ssd_vtrace_last_error.restype = C.c_char_p
        L.ssd_ws_policy_ppo_grad.argtypes = ([vp, i32, i32, i32, i32, i32] + [vp] * 9 + [i32, i32] + [C.c_double] * 5
                                             + [vp, vp, vp, i32, u32, vp])
        L.ssd_ws_policy_ac_grad.argtypes = ([vp, i32, i32, i32, i32, i32] + [vp] * 6 + [i32, i32] + [C.c_double] * 2
                                            + [vp, vp, vp, i32, u32, vp])
        L.ssd_ws_policy_forward_seq.argtypes = [vp, i32, i32, i32, i32, i32] + [vp] * 6 + [i32, i32] + [vp] * 5 + [i32, u32, vp]
        for name in FORWARD_SEQ_SYMBOLS:
            getattr(L, name).argtypes = [vp, i32, i32, i32, i32] + [vp] * 4 + [i32, i32, i32, vp, C.c_int64] + [vp] * 4 + [i32, u32, vp]
        L.ssd_ws_stats_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
        L.ssd_ws_stats_destroy.argtypes = [vp]
        L.ssd_ws_stats_attach.argtypes = [vp, vp]
        L.ssd_ws_stats_discard.argtypes = [vp, vp, vp]
        L.ssd_ws_stats_drain.argtypes = [vp] + [vp] * 12 + [u32, vp]
        L.ssd_ws_stats_last_error.argtypes = [vp]
        L.ssd_ws_stats_last_error.restype = C.c_char_p
        L.ssd_standardize.argtypes = [vp, i32, i32, i32, i32, i32, C.c_double, vp, vp, vp, i32, vp]
        L.ssd_explained_variance.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, vp]
        L.ssd_moments_last_error.argtypes = []
        L.ssd_moments_last_error.restype = C.c_char_p
        for name in SYMBOLS:
            getattr(L, name)
        if L.ssd_abi_version() != ABI_VERSION:
            raise SsdError("libssd_hip.so ABI %d != expected %d: rebuild" % (L.ssd_abi_version(), ABI_VERSION))
        _lib = L
    return _lib


def _fail(symbol, what, rc, *handle):
    msg = getattr(lib(), symbol)(*handle)
    raise SsdError("libssd_hip %s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


def _checker(symbol, what):
    """-> check(rc) of a family without a handle: raises SsdError with the calling thread's last error text unless rc is SSD_OK."""
    def check(rc):
        if rc != SSD_OK:
            _fail(symbol, what, rc)
    return check


def _handle_checker(symbol, what):
    """-> check(rc, handle=None) of a family whose last-error call takes the handle."""
    def check(rc, handle=None):
        if rc != SSD_OK:
            _fail(symbol, what, rc, handle)
    return check


check = _handle_checker("ssd_last_error", "call")
ws_check = _handle_checker("ssd_ws_last_error", "Watershed call")
stats_check = _handle_checker("ssd_stats_last_error", "episode-statistics call")
ws_stats_check = _handle_checker("ssd_ws_stats_last_error", "Watershed episode-statistics call")
policy_check = _checker("ssd_policy_last_error", "policy call")
advantages_check = _checker("ssd_advantages_last_error", "advantages call")
vtrace_check = _checker("ssd_vtrace_last_error", "V-trace call")
moments_check = _checker("ssd_moments_last_error", "batch-moments call")
