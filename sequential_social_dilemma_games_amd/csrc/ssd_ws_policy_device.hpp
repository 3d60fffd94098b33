// csrc/ssd_ws_policy_device.hpp -- what the three files of the Watershed baselines' policy (LSTMFCNet) state alike, each defined
// once: the tile constants and the weight layout they rest on, the two dense chains, the DiagGaussian head's expressions, the
// comm-agent rule and the argument checks of the entry points.  Used by ssd_ws_policy.hip (the per-phase forward and the
// rollout), ssd_ws_policy_seq.hip (the sequence forward) and ssd_ws_policy_grad.hip (the PPO and A3C losses with BPTT).
// ssd_ws_policy.hpp next to it is something else: the view of a Watershed handle.
//
// Every sum is one chain in a fixed order (ssd_policy_device.hpp's rule) and include/ssd.h demands the same bits of dist, value
// and logp from all three files: a change here reaches them together.
#pragma once
#include "ssd_policy.hpp"
#include "ssd_policy_device.hpp"

namespace ssd {
namespace wsp {

constexpr int kX = SSD_WSP_X;           // dense1's width: the x columns of the [x, h] tile
constexpr int kObs = SSD_WS_OBS_WIDTH;
constexpr int kOut = SSD_WSP_OUT;
constexpr int kTile = SSD_WSPPO_TILE;   // envs or sequences of a workgroup's tile, rows of a trunk-kernel tile
constexpr int kTrunk = SSD_WSP_LSTM_W;  // floats of dense0 and dense1 in the packed layout: what lies below lstm_w
constexpr int kHd = 8;                  // pitch of a row's head outputs: dist 0..4, the value at 5, two zeros

static_assert(kTile == 16 && kX == 16 && kOut + 1 <= kHd, "the tiles of the Watershed kernels");
static_assert(SSD_WSP_D0_B == SSD_WSP_D0_W + kObs * kX && SSD_WSP_D1_W >= SSD_WSP_D0_B + kX && SSD_WSP_D1_B == SSD_WSP_D1_W + kX * kX &&
              kTrunk >= SSD_WSP_D1_B + kX, "weight layout of include/ssd.h");

using Cell = KerasCell;                 // gates i, f, c~, o, no forget bias; a state is (h, c)

// dense0 and dense1 of tile row m, column j, after their ReLUs.  wd: the packed trunk weights (the weight set's base in global
// memory, or a copy of its first kTrunk floats in LDS); obs [kTile][kObs] and d0 [kTile][kX] are in LDS.  The sequence forward
// and the loss kernel call them.  ssd_ws_policy_kernel has the same two chains written out in its step 2 and must follow any
// change here: called, they gave that kernel another register allocation and a forward measured 4 to 6 % slower.
__device__ __forceinline__ float ws_dense0(const float *obs, const float *wd, int m, int j) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kObs; ++k) s = fmaf(obs[m * kObs + k], wd[SSD_WSP_D0_W + k * kX + j], s);
    return fmaxf(s + wd[SSD_WSP_D0_B + j], 0.f);
}
__device__ __forceinline__ float ws_dense1(const float *d0, const float *wd, int m, int j) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kX; ++k) s = fmaf(d0[m * kX + k], wd[SSD_WSP_D1_W + k * kX + j], s);
    return fmaxf(s + wd[SSD_WSP_D1_B + j], 0.f);
}

// RLlib's one-dimensional DiagGaussian(mean = dist[0], log_std = dist[1]) of an action agent: sd, then z, logp and the entropy
// of an action.  (The rollout draws its action from sd before it asks for z.)
struct WsGauss {
    float mean, log_std, sd;
    __device__ __forceinline__ WsGauss(float mean_, float log_std_) : mean(mean_), log_std(log_std_), sd(expf(log_std_)) {}
    __device__ __forceinline__ float z(float act) const { return (act - mean) / sd; }
    __device__ __forceinline__ float logp(float z) const { return ((-0.5f * (z * z)) - log_std) - 0.9189385f; }
    __device__ __forceinline__ float entropy() const { return log_std + 1.4189385f; }
};

// A comm agent's head is Categorical over dist[0:5]; every other agent's is the Gaussian above.
__host__ __device__ __forceinline__ bool ws_is_comm(int variant, int agent_id) { return variant == SSD_WS_SEQ_COMM && agent_id < 4; }

// ---- the entry points' argument rules (host); null = fine, else the error text ----
// The sets follow the variant: one per agent id.
inline const char *ws_check_sets(int32_t num_sets, int32_t variant) {
    if (variant != SSD_WS_SEQ && variant != SSD_WS_SEQ_COMM) return "unknown variant";
    if (num_sets != (variant == SSD_WS_SEQ ? 4 : 8)) return "num_sets must be 4 (Seq) or 8 (SeqComm): one set per agent id";
    return nullptr;
}
// The net of the per-phase forward and the rollout: one acting agent per env and 5 outputs, check_policy_net's rules for the
// weights and the cell.
inline const char *ws_check_net(const float *weights, int32_t num_sets, int32_t cell_size, int32_t variant) {
    if (!weights) return "weights are required";
    if (const char *why = check_policy_net(kNetLstm, weights, 1, 1, kOut, cell_size)) return why;
    return ws_check_sets(num_sets, variant);
}
// What the sequence forward and the two loss calls check alike, in the order their callers have always seen it reported (the
// agent id before the cell; the weights' alignment comes with the other float buffers', at the caller).  boot_rows: 1 where the
// call also walks a bootstrap row per sequence.
inline const char *ws_check_seq_call(const float *weights, int32_t num_sets, int32_t cell_size, int32_t variant, int32_t agent_id,
                                     int32_t seq_len, int32_t n_steps, int32_t num_seqs, int boot_rows) {
    if (!weights) return "weights are required";
    if (const char *why = ws_check_sets(num_sets, variant)) return why;
    if (agent_id < 0 || agent_id >= num_sets) return "agent_id is no id of the variant";
    if (cell_size != 64 && cell_size != 128 && cell_size != 256) return "cell_size must be 64, 128 or 256";
    if (seq_len < 1) return "seq_len must be >= 1";
    if (n_steps < 1 || num_seqs < 1) return "n_steps and num_seqs must be >= 1";
    if (((int64_t)n_steps + boot_rows) * num_seqs > (int64_t)INT32_MAX - 16)
        return boot_rows ? "at most 2^31 - 17 rows, the bootstrap's included" : "at most 2^31 - 17 rows";
    return nullptr;
}

}  // namespace wsp
}  // namespace ssd
