// csrc/ssd_policy_device.hpp -- the device pieces the policy kernels are built from, each defined once: the LSTM gate GEMM, the
// two cell rules and the cell update, the start rule and the loader of the h rows, the heads, the PPO loss terms of a row, the
// action draw, and the conv-FC trunk (conv, fc1, fc2) on a tile.  Used by ssd_policy.hip (conv-FC), ssd_policy_grad.hip,
// ssd_policy_lstm.hip, ssd_policy_moa.hip, ssd_ws_policy.hip and ssd_bptt_device.hpp (the pieces of the BPTT gradient kernels,
// through which ssd_policy_lstm_grad.hip and ssd_policy_moa_grad.hip reach these) and ssd_ws_policy_grad.hip; the argument blocks stay in
// ssd_policy.hpp, which host code reads too.  Every sum below is one chain in a fixed order, so a change here changes the
// bits of every kernel that uses the piece, and the tests that compare kernels and paths bit for bit see it.
//
// v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain per accumulator): lane l holds A[l & 15][k = l >> 4] and
// B[k = l >> 4][l & 15]; D: col l & 15, row 4 (l >> 4) + r.
#pragma once
#include <stddef.h>

#include "ssd_policy.hpp"

namespace ssd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// ---------------------------------------------------------------------------------------------------------------- the cell
// The gates of the 16 MT rows of s_in (pitch Pitch: the input columns, then the C columns of h; K of them in all) for a
// workgroup of 4 C threads: acc[g][s] = z[16 s .., g C + 16 wave + l15] without the bias, A[m][k] = s_in row m,
// B[k][n] = w[k][g C + 16 wave + n].  Wave w takes cells 16w .. 16w + 15 of all four gates, so lane (l15, l4) ends up with the
// four gates of cell 16 wave + l15 for rows 16 s + 4 l4 + r, and each weight load feeds MT MFMAs.
template <int C, int K, int Pitch, int MT>
__device__ __forceinline__ void lstm_gates(const float *s_in, const float *__restrict__ w, int tid, f32x4 (&acc)[4][MT]) {
    static_assert(K % 4 == 0 && Pitch % 64 == 4, "tile");    // pitch = 4 (mod 64): lane (l15, l4) of an A load hits bank 4 l15 + l4
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const float *a_row = s_in + l15 * Pitch + l4;
    const float *wg = w + (size_t)l4 * 4 * C + 16 * wave + l15;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int s = 0; s < MT; ++s) acc[g][s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int kk = 0; kk < K / 4; ++kk) {
        const float *wk = wg + (size_t)kk * 16 * C;
        float bv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) bv[g] = wk[g * C];
        float av[MT];
#pragma unroll
        for (int s = 0; s < MT; ++s) av[s] = a_row[s * 16 * Pitch + 4 * kk];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int s = 0; s < MT; ++s) acc[g][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[g], acc[g][s], 0, 0, 0);
    }
}

// The two cell rules: the order of the four gate columns z0..z3 (bias added), and where c and h sit in a state's two rows.
// kI, kJ, kF, kO: the columns of the input gate, the candidate, the forget gate and the output gate.  gates: the four
// activations in column order as update forms them, which the BPTT kernels keep for the backward (ssd_bptt_device.hpp).
struct RllibCell {                  // RLlib 0.7.6: gates i, j, f, o with forget bias 1; a state is (c, h)
    static constexpr int kRowC = 0, kRowH = 1;
    static constexpr int kI = 0, kJ = 1, kF = 2, kO = 3;
    static __device__ __forceinline__ void update(float zi, float zj, float zf, float zo, float c, float *c2, float *h2) {
        *c2 = sigmoidf_(zf + 1.f) * c + sigmoidf_(zi) * tanhf(zj);
        *h2 = sigmoidf_(zo) * tanhf(*c2);
    }
    static __device__ __forceinline__ void gates(float zi, float zj, float zf, float zo, float (&g)[4]) {
        g[0] = sigmoidf_(zi); g[1] = tanhf(zj); g[2] = sigmoidf_(zf + 1.f); g[3] = sigmoidf_(zo);
    }
};
struct KerasCell {                  // Keras: gates i, f, c~, o, no forget bias; a state is (h, c)
    static constexpr int kRowH = 0, kRowC = 1;
    static constexpr int kI = 0, kF = 1, kJ = 2, kO = 3;
    static __device__ __forceinline__ void update(float zi, float zf, float zc, float zo, float c, float *c2, float *h2) {
        *c2 = sigmoidf_(zf) * c + sigmoidf_(zi) * tanhf(zc);
        *h2 = sigmoidf_(zo) * tanhf(*c2);
    }
    static __device__ __forceinline__ void gates(float zi, float zf, float zc, float zo, float (&g)[4]) {
        g[0] = sigmoidf_(zi); g[1] = sigmoidf_(zf); g[2] = tanhf(zc); g[3] = sigmoidf_(zo);
    }
};

// Position of agent n in the order of the ids sorted as strings ('agent-10' < 'agent-2'), for n < 100: first digit, then
// the shorter id first, then the second digit.
__device__ __forceinline__ int id_key(int n) { return n < 10 ? 100 * n : 100 * (n / 10) + 1 + n % 10; }

// The MOA input slots of every agent, by a workgroup of at least 256 threads: s_slot[i * 16 + q] = the agent whose action sits
// in slot q of agent i's previous-action vector: i itself for q = 0, then the others in string order (the j of pred [j][a] is
// slot j + 1).  Entries with i or q >= N are not written.
__device__ __forceinline__ void moa_slots(int N, int tid, int *s_slot) {
    const int i = tid >> 4, q = tid & 15;
    if (tid >= 256 || i >= N || q >= N) return;
    int agent = i;
    if (q > 0) {
        for (int n = 0; n < N; ++n) {
            if (n == i) continue;
            int rank = 0;
            for (int k = 0; k < N; ++k) rank += k != i && id_key(k) < id_key(n);
            if (rank == q - 1) agent = n;
        }
    }
    s_slot[tid] = agent;
}

// start flag of row `row` of env b: starts[row] in the forward, t == 0 in rollouts; envs past B count as starting (nothing read)
__device__ __forceinline__ int row_start(const uint8_t *starts, const uint4 *hdr, int b, size_t row, int B) {
    if (b >= B) return 1;
    return starts ? starts[row] != 0 : (hdr ? hdr[b].y == 0u : 0);
}

// Where tile row m keeps its state (two rows of C floats, Cell's order): the float offset, and whether the row is the caller's
// to touch at all (a row past the batch, or of another agent id, is not).
struct StateRow {
    bool mine;
    size_t at;
};

// h of the kM tile rows to s_h (pitch floats apart; zero where s_start[m], whose state is never read), and the state each row
// used to state_used where that is given.  in(m), used(m): row m's StateRow in state_in and state_used; in(m).mine is not
// looked at (a row that is not the caller's starts).
template <class Cell, int C, int kM, class In, class Used>
__device__ __forceinline__ void load_h(float *s_h, int pitch, const int *s_start, const float *state_in, float *state_used, int tid,
                                       In in, Used used) {
    for (int q = tid; q < kM * C; q += 4 * C) {
        const int m = q / C, u = q - m * C;
        const size_t r = in(m).at;
        const StateRow ru = used(m);
        const float h = s_start[m] ? 0.f : state_in[r + Cell::kRowH * C + u];
        s_h[m * pitch + u] = h;
        if (state_used && ru.mine) {
            state_used[ru.at + Cell::kRowH * C + u] = h;
            state_used[ru.at + Cell::kRowC * C + u] = s_start[m] ? 0.f : state_in[r + Cell::kRowC * C + u];
        }
    }
}

// The cell update of the rows lstm_gates left in acc: lane (l15, l4) holds the four gates of cell u = 16 wave + l15 for rows
// m = 16 s + 4 l4 + r.  bias: [4][C].  h' goes to s_h (as load_h), c' and h' to state_out where that is given (state_in itself:
// in place).  row(m): row m's StateRow; nothing of a row that is not `mine` is touched.
template <class Cell, int C, int MT, class Row>
__device__ __forceinline__ void cell_update(const f32x4 (&acc)[4][MT], const float *__restrict__ bias, const int *s_start,
                                            const float *state_in, float *state_out, float *s_h, int pitch, int tid, Row row) {
    const int lane = tid & 63, u = 16 * (tid >> 6) + (lane & 15), l4 = lane >> 4;
    const float b0 = bias[u], b1 = bias[C + u], b2 = bias[2 * C + u], b3 = bias[3 * C + u];
#pragma unroll
    for (int s = 0; s < MT; ++s) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 16 * s + 4 * l4 + r;
            const StateRow st = row(m);
            if (!st.mine) continue;
            const float c = s_start[m] ? 0.f : state_in[st.at + Cell::kRowC * C + u];
            float c2, h2;
            Cell::update(acc[0][s][r] + b0, acc[1][s][r] + b1, acc[2][s][r] + b2, acc[3][s][r] + b3, c, &c2, &h2);
            s_h[m * pitch + u] = h2;
            if (state_out) {
                state_out[st.at + Cell::kRowC * C + u] = c2;
                state_out[st.at + Cell::kRowH * C + u] = h2;
            }
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- the heads
// Output j of one row from its K hidden values hr: column j of w_out [K][n_out] plus b_out[j] for j < n_out, the value
// (w_value [K], b_value) for j == n_out.  One fmaf chain in k order.
template <int K>
__device__ __forceinline__ float head(const float *hr, const float *__restrict__ w_out, const float *__restrict__ w_value,
                                      const float *__restrict__ b_out, const float *__restrict__ b_value, int n_out, int j) {
    const float *hw = j < n_out ? w_out + j : w_value;
    const int stride = j < n_out ? n_out : 1;
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < K; ++k) s = fmaf(hr[k], hw[k * stride], s);
    return s + (j < n_out ? b_out[j] : *b_value);
}

// The heads of the kM tile rows (envs b0 .., agent i) of a [B][N] batch: logits 0..A-1 and the value at A to s_out [kM][16], and
// to a.logits, a.value (and logits_scratch [B][N][16]) where given.  Args: PolicyArgs, LstmArgs or MoaArgs.
template <int K, int kM, int kThreads, class Args>
__device__ __forceinline__ void heads(const Args &a, const float *s_h, int pitch, const float *__restrict__ w_out,
                                      const float *__restrict__ w_value, const float *__restrict__ b_out,
                                      const float *__restrict__ b_value, float *s_out, float *logits_scratch, int tid, int b0, int i) {
    const int A = a.A;
    for (int q = tid; q < kM * 16; q += kThreads) {
        const int m = q >> 4, j = q & 15, b = b0 + m;
        if (j > A) continue;                                 // j < A: logit j; j == A: the value
        const float s = head<K>(s_h + m * pitch, w_out, w_value, b_out, b_value, A, j);
        s_out[m * 16 + j] = s;
        if (b < a.B) {
            const size_t row = (size_t)b * a.N + i;
            if (j < A) {
                if (a.logits) a.logits[row * A + j] = s;
                if (logits_scratch) logits_scratch[row * 16 + j] = s;
            } else if (a.value) {
                a.value[row] = s;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ the PPO loss
// The loss terms of one row (include/ssd.h, PPO LOSS AND GRADIENTS), one thread per row: l = the row's logits 0..A-1 and its
// value at A, act its action (already within 0 .. A-1), bl its behaviour logits or null.  The five terms are float32 and are
// added to st (total, policy, vf, kl, entropy); d[0..A] receives d row_loss / d (logits, value) with the contract's derivatives
// at the kinks.  Used by the PPO gradient kernels of the three policies (ssd_policy_grad.hip; bptt_policy_forward of
// ssd_bptt_device.hpp for the recurrent and the MOA policy).
struct PpoHyper {
    float clip, vf_clip, vf_coeff, ent_coeff, kl_coeff;
};

__device__ __forceinline__ void ppo_row(const float *l, float *d, int A, int act, float adv, float vt, float vfp, float lpo,
                                        const float *bl, const PpoHyper &a, double (&st)[5]) {
    const float value = l[A];
    float mx = l[0];
    for (int k = 1; k < A; ++k) mx = fmaxf(mx, l[k]);
    float s = 0.f;
    for (int k = 0; k < A; ++k) s += expf(l[k] - mx);
    const float lse = mx + logf(s);
    float ent = 0.f;
    for (int k = 0; k < A; ++k) {
        const float lp = l[k] - lse;
        ent -= expf(lp) * lp;
    }
    float kl = 0.f;
    float bl_lse = 0.f;
    if (bl) {
        float bm = bl[0];
        for (int k = 1; k < A; ++k) bm = fmaxf(bm, bl[k]);
        float bs = 0.f;
        for (int k = 0; k < A; ++k) bs += expf(bl[k] - bm);
        bl_lse = bm + logf(bs);
        for (int k = 0; k < A; ++k) {
            const float blp = bl[k] - bl_lse;
            kl += expf(blp) * (blp - (l[k] - lse));
        }
    }
    const float logp = l[act] - lse;
    const float ratio = expf(logp - lpo);
    const float lo = 1.f - a.clip, hi = 1.f + a.clip;
    const float s1 = adv * ratio, s2 = adv * fminf(fmaxf(ratio, lo), hi);
    const float surr = fminf(s1, s2);
    const float dsurr = ((ratio >= lo && ratio <= hi) || s1 < s2) ? adv : 0.f;     // d surr / d ratio
    const float d1 = value - vt, dv = value - vfp;
    const float d2 = (vfp + fminf(fmaxf(dv, -a.vf_clip), a.vf_clip)) - vt;
    const float vf1 = d1 * d1, vf2 = d2 * d2;
    const float vf = fmaxf(vf1, vf2);
    const float dvf = (fabsf(dv) <= a.vf_clip || vf1 >= vf2) ? 2.f * d1 : 0.f;     // d vf / d value
    const float row_loss = ((-surr + a.kl_coeff * kl) + a.vf_coeff * vf) - a.ent_coeff * ent;
    st[0] += (double)row_loss; st[1] += (double)(-surr); st[2] += (double)vf; st[3] += (double)kl; st[4] += (double)ent;
    const float gl = -dsurr * ratio;           // d row_loss / d logp
    for (int k = 0; k < A; ++k) {
        const float lp = l[k] - lse, pk = expf(lp);
        float dk = gl * ((k == act ? 1.f : 0.f) - pk) + a.ent_coeff * (pk * (lp + ent));
        if (bl) dk += a.kl_coeff * (pk - expf(bl[k] - bl_lse));
        d[k] = dk;
    }
    d[A] = a.vf_coeff * dvf;
}

// ------------------------------------------------------------------------------------------------------------ the A3C loss
// Which loss a gradient kernel forms per row: a compile-time parameter of the kernels that call ppo_row, so that the PPO
// instantiations keep their instruction text.
constexpr int kLossPpo = 0, kLossAc = 1;

// The A3C terms of one row (include/ssd.h, A3C LOSS AND GRADIENTS), as ppo_row: l, d, act, st as there; only vf_coeff and
// ent_coeff of the hyper-parameters are read.  st receives total, policy, vf, entropy in 0..3 (st[4] is left alone).  No kinks.
__device__ __forceinline__ void a3c_row(const float *l, float *d, int A, int act, float adv, float vt, const PpoHyper &a,
                                        double (&st)[5]) {
    const float value = l[A];
    float mx = l[0];
    for (int k = 1; k < A; ++k) mx = fmaxf(mx, l[k]);
    float s = 0.f;
    for (int k = 0; k < A; ++k) s += expf(l[k] - mx);
    const float lse = mx + logf(s);
    float ent = 0.f;
    for (int k = 0; k < A; ++k) {
        const float lp = l[k] - lse;
        ent -= expf(lp) * lp;
    }
    const float logp = l[act] - lse;
    const float pi = -(logp * adv);
    const float d1 = value - vt;
    const float vf = 0.5f * (d1 * d1);
    const float row_loss = (pi + a.vf_coeff * vf) - a.ent_coeff * ent;
    st[0] += (double)row_loss; st[1] += (double)pi; st[2] += (double)vf; st[3] += (double)ent;
    for (int k = 0; k < A; ++k) {
        const float lp = l[k] - lse, pk = expf(lp);
        d[k] = -adv * ((k == act ? 1.f : 0.f) - pk) + a.ent_coeff * (pk * (lp + ent));
    }
    d[A] = a.vf_coeff * d1;
}

// -------------------------------------------------------------------------------------------------------------- the action
// shared PRNG (prng.py): the triple32 chain of ssd_kernels.hip
__device__ __forceinline__ uint32_t pol_mix32(uint32_t x) {
    x ^= x >> 17; x *= 0xED5AD4BBu;
    x ^= x >> 11; x *= 0xAC4C1B51u;
    x ^= x >> 15; x *= 0x31848BABu;
    x ^= x >> 14;
    return x;
}

// The key of the S_POLICY draws of env `env` at (episode, t) (include/ssd.h): draw d of it is pol_mix32(key ^ d).
__device__ __forceinline__ uint32_t policy_key(uint32_t seed_lo, uint32_t seed_hi, uint32_t env, uint32_t episode, uint32_t t) {
    uint32_t key = 0x243F6A88u;
    key = pol_mix32(key ^ seed_lo);
    key = pol_mix32(key ^ seed_hi);
    key = pol_mix32(key ^ env);
    key = pol_mix32(key ^ episode);
    return pol_mix32(pol_mix32(key ^ t) ^ (uint32_t)SSD_S_POLICY);
}

// The action of agent i of env b from its logits l[0..A-1]: argmax (greedy), or the first a with u < cumulative softmax, u from
// the S_POLICY draw of the env's (episode, t) in h = hdr[b] (include/ssd.h); *logp its log-probability.
__device__ __forceinline__ int policy_pick(const float *l, int A, int greedy, uint4 h, uint32_t seed_lo, uint32_t seed_hi,
                                           uint32_t env, uint32_t i, float *logp) {
    float mx = l[0];
    int arg = 0;
    for (int k = 1; k < A; ++k)
        if (l[k] > mx) { mx = l[k]; arg = k; }
    float s = 0.f;
    for (int k = 0; k < A; ++k) s += expf(l[k] - mx);
    int act = arg;
    if (!greedy) {
        const float u = (float)(pol_mix32(policy_key(seed_lo, seed_hi, env, h.z, h.y) ^ i) >> 8) * 0x1p-24f;
        act = A - 1;
        float c = 0.f;
        for (int k = 0; k < A; ++k) {
            c += expf(l[k] - mx) / s;
            if (u < c) { act = k; break; }
        }
    }
    *logp = l[act] - (mx + logf(s));
    return act;
}

// Rollouts, one thread per tile row: the action of agent i of env b0 + tid from the logits heads() left in s_out, to a.actions
// (and actions_copy) and its log-probability to a.logp where given.  Args as heads().
template <int kM, class Args>
__device__ __forceinline__ void pick_actions(const Args &a, const float *s_out, int32_t *actions_copy, int tid, int b0, int i) {
    if (tid < kM && b0 + tid < a.B) {
        const int b = b0 + tid;
        float lp;
        const int act = policy_pick(s_out + tid * 16, a.A, a.greedy, a.greedy ? uint4{} : a.hdr[b], a.seed_lo, a.seed_hi,
                                    a.env_base + (uint32_t)b, (uint32_t)i, &lp);
        const size_t row = (size_t)b * a.N + i;
        a.actions[row] = act;
        if (actions_copy) actions_copy[row] = act;
        if (a.logp) a.logp[row] = lp;
    }
}

// --------------------------------------------------------------------------------------------------------------- the trunk
// The conv-FC trunk on a tile of kTile rows by a workgroup of kThreads threads: the conv into LDS and the FC stack on it.  Used
// by the forward kernel (ssd_policy.hip) and by the PPO loss-and-gradient kernel (ssd_policy_grad.hip).
namespace trunk {

constexpr int kTile = 16;          // envs per workgroup: M of the fc1 tile
constexpr int kThreads = 256;      // 4 waves
constexpr int kObs = 675;          // 15 * 15 * 3 bytes
constexpr int kPos = 169;          // 13 * 13 conv outputs per filter
constexpr int kFlat = 1014;        // 13 * 13 * 6
constexpr int kPitch = 1017;       // LDS pitch (floats) of a row of conv outputs: 1014 + zero padding, odd against bank conflicts
constexpr int kKSteps = 254;       // fc1: K = 1014 padded to 1016 = 254 MFMA k-steps of 4
constexpr int kHalf = kKSteps / 2; // k-steps per wave (odd: 63 pairs and one more)
constexpr int kHP = 33;            // LDS pitch of the hidden layers

static_assert(kThreads == 256, "one thread per entry of the normalisation table");
static_assert(SSD_POL_FC1_B == SSD_POL_FC1_W + kFlat * 32 && SSD_POL_FC2_W == SSD_POL_FC1_B + 32 && SSD_POL_FC2_B == SSD_POL_FC2_W + 1024 &&
              SSD_POL_VALUE_W == SSD_POL_FC2_B + 32 && SSD_POL_VALUE_B == SSD_POL_VALUE_W + 32 && SSD_POL_LOGITS_W >= SSD_POL_VALUE_B + 1,
              "weight layout of include/ssd.h");


// Step 2 of ssd_policy.hip: conv 3x3, 6 filters, ReLU of the kTile observations in s_obs (u8 [kTile][kObs]; s_norm: the 256-entry
// normalisation table) to s_conv [kTile][kPitch] in the flatten order (row, col, channel).  w: the weight set's base.
__device__ __forceinline__ void conv_tile(const float *__restrict__ w, const uint8_t *s_obs, const float *s_norm, float *s_conv,
                                          int tid) {
    for (int q = tid; q < kTile * kPos; q += kThreads) {
        const int r = q / kPos, pos = q - r * kPos, y = pos / 13, x = pos - y * 13;
        const uint8_t *src = s_obs + r * kObs + (y * 15 + x) * 3;
        float acc[6];
#pragma unroll
        for (int f = 0; f < 6; ++f) acc[f] = 0.f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
            for (int j = 0; j < 9; ++j) {                   // (dx, c) = (j / 3, j % 3): 9 contiguous bytes of view row y + dy
                const float v = s_norm[src[dy * 45 + j]];
#pragma unroll
                for (int f = 0; f < 6; ++f) acc[f] = fmaf(v, w[SSD_POL_CONV_W + (dy * 9 + j) * 6 + f], acc[f]);
            }
        }
        float *dst = s_conv + r * kPitch + pos * 6;
#pragma unroll
        for (int f = 0; f < 6; ++f) dst[f] = fmaxf(acc[f] + w[SSD_POL_CONV_B + f], 0.f);
    }
}

// Steps 3 and 4 up to fc2 on the conv output in s_conv: fc1 on the matrix cores, its two K halves added through LDS, fc2 on the
// VALU; ReLU after both layers, or tanh (the MOA policy's stacks).  ws: a weight set's base, moved so that SSD_POL_FC1_W ..
// SSD_POL_FC2_B address the stack's layers.  fc2's output of tile row m < rows goes to out[m * stride + 0..31].
template <bool kTanh>
__device__ __forceinline__ void fc_stack(const float *__restrict__ ws, const float *s_conv, float *s_part, float *s_h1, int tid,
                                         float *out, size_t stride, int rows) {
    const auto act = [](float x) { return kTanh ? tanhf(x) : fmaxf(x, 0.f); };
    // fc1: A[m][k] = conv row m, B[k][n] = fc1_w[k][n] (the lane layout: ssd_policy_device.hpp)
    const int wave = tid >> 6, lane = tid & 63, nt = wave & 1, kh = wave >> 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    const float *a_row = s_conv + l15 * kPitch + l4;
    const float *w1 = ws + SSD_POL_FC1_W + l4 * 32 + nt * 16 + l15;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    // (wave half 0: k-steps 0..126; half 1: 127..253, whose last step is peeled -- its rows 1014, 1015 are padding)
    const int kb = kh * kHalf;
#pragma unroll 4
    for (int p = 0; p < (kHalf - 1) / 2; ++p) {
        const int kk = kb + 2 * p;
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_row[4 * kk], w1[(size_t)kk * 128], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_row[4 * kk + 4], w1[(size_t)kk * 128 + 128], acc1, 0, 0, 0);
    }
    {
        const int kl = kb + kHalf - 1;
        const float bv = 4 * kl + l4 < kFlat ? w1[(size_t)kl * 128] : 0.f;
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_row[4 * kl], bv, acc0, 0, 0, 0);
    }
    const f32x4 acc = acc0 + acc1;
    if (kh) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s_part[(nt * 16 + l4 * 4 + r) * 16 + l15] = acc[r];
    }
    __syncthreads();
    if (!kh) {
        const int n = nt * 16 + l15;
        const float bias = ws[SSD_POL_FC1_B + n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = l4 * 4 + r;
            s_h1[m * kHP + n] = act(acc[r] + s_part[(nt * 16 + m) * 16 + l15] + bias);
        }
    }
    __syncthreads();
    // fc2: thread (m, n) takes columns n and n + 16 of row m
    const int m = tid >> 4, n = tid & 15;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int nn = n + 16 * h;
        float s = 0.f;
#pragma unroll 8
        for (int k = 0; k < 32; ++k) s = fmaf(s_h1[m * kHP + k], ws[SSD_POL_FC2_W + k * 32 + nn], s);
        if (m < rows) out[m * stride + nn] = act(s + ws[SSD_POL_FC2_B + nn]);
    }
}

}  // namespace trunk

}  // namespace ssd
