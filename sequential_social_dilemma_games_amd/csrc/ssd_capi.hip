// csrc/ssd_capi.hip -- host side of the C ABI declared in include/ssd.h.
// Owns the engine state in HBM (hipMalloc), derives the static per-map tables, stages host
// buffers when asked to, and launches the fused kernel of ssd_kernels.hip.  No CPU compute
// path exists here: every stepping call ends in a kernel launch or an error code.  Handle lifecycle, the per-call steps, state,
// render, agent-action observations, debug calls and the policy rollouts; ssd_rollout_random / ssd_rollout_actions and their
// dispatch paths are ssd_rollout.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ssd.h"
#include "ssd_internal.hpp"
#include "ssd_env.hpp"
#include "ssd_policy.hpp"

using ssd::Params;

static thread_local std::string g_create_error;

namespace {

// rand < p  <=>  k < ceil(p * 2^32) for rand = k / 2^32
uint64_t threshold(double p) {
    if (p <= 0.0) return 0;
    const double x = std::ceil(p * 4294967296.0);
    return x >= 4294967296.0 ? 4294967296ull : (uint64_t)x;
}

// cleanup.py:156-171 compute_probabilities for a map holding n_h cells of 'H' (constants :24-27)
void cleanup_probs(int potential, int n_h, double *p_apple, double *p_waste) {
    const double depletion = 0.4, restoration = 0.0, waste_p = 0.5, apple_p = 0.05;
    double density = 0;
    if (potential > 0) density = 1 - (double)(potential - n_h) / (double)potential;
    if (density >= depletion) { *p_apple = 0; *p_waste = 0; return; }
    *p_waste = waste_p;
    *p_apple = density <= restoration ? apple_p : (1 - (density - restoration) / (depletion - restoration)) * apple_p;
}

constexpr uint8_t kVoid = '0';      // the glyph utility_funcs.py:94-114 pads views with; fills the row padding of the grids

// dense [E][H][W] (the ABI's layout) <-> the engine's padded-row grids [E][S], row stride WP
void pack_grid(const ssd_env *env, const int8_t *dense, std::vector<uint8_t> &grid, uint8_t pad) {
    grid.assign((size_t)env->E * env->S, pad);
    for (int e = 0; e < env->E; ++e)
        for (int r = 0; r < env->H; ++r)
            std::memcpy(grid.data() + (size_t)e * env->S + (size_t)r * env->WP, dense + ((size_t)e * env->H + r) * env->W, env->W);
}
void unpack_grid(const ssd_env *env, const std::vector<uint8_t> &grid, int8_t *dense) {
    for (int e = 0; e < env->E; ++e)
        for (int r = 0; r < env->H; ++r)
            std::memcpy(dense + ((size_t)e * env->H + r) * env->W, grid.data() + (size_t)e * env->S + (size_t)r * env->WP, env->W);
}

template <typename T>
int dev_alloc(ssd_env *env, T **out, size_t count, bool zero = true) {
    void *ptr = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    hipError_t e = hipMalloc(&ptr, bytes);
    if (e != hipSuccess) { env->err = std::string("hipMalloc: ") + hipGetErrorString(e); return SSD_E_NOMEM; }
    if (zero) {
        e = hipMemset(ptr, 0, bytes);
        if (e != hipSuccess) { env->err = std::string("hipMemset: ") + hipGetErrorString(e); return SSD_E_DEVICE; }
    }
    env->allocs.push_back(ptr);
    *out = static_cast<T *>(ptr);
    return SSD_OK;
}

template <typename T>
int upload(ssd_env *env, T **out, const std::vector<T> &host) {
    int rc = dev_alloc(env, out, host.size(), host.empty());
    if (rc) return rc;
    if (!host.empty()) SSD_HIP(env, hipMemcpy(*out, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return SSD_OK;
}

int fail_create(const std::string &msg, int code) {
    g_create_error = msg;
    return code;
}

int ensure_staging(ssd_env *env) {
    if (env->st_obs) return SSD_OK;
    const size_t en = (size_t)env->E * env->N;
    int rc;
    const size_t a16 = 15;
    const size_t o_act = 0, o_aout = (o_act + en * 4 + a16) & ~a16, o_rew = (o_aout + en * 4 + a16) & ~a16,
                 o_ord = (o_rew + en * 4 + a16) & ~a16, o_done = (o_ord + en + a16) & ~a16, o_mask = (o_done + en + a16) & ~a16,
                 o_obs = (o_mask + (size_t)env->E + a16) & ~a16, o_f32 = (o_obs + obs_bytes(env) + a16) & ~a16,
                 total = o_f32 + obs_bytes(env, true);
    if (total <= (1u << 20)) {
        void *h = nullptr, *d = nullptr;
        if (hipHostMalloc(&h, total, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&d, h, 0) == hipSuccess) {
            std::memset(h, 0, total);
            env->host_allocs.push_back(h);
            env->st_mapped = true; env->st_host = static_cast<uint8_t *>(h);
            uint8_t *b = static_cast<uint8_t *>(d);
            env->st_actions = reinterpret_cast<int32_t *>(b + o_act); env->st_actions_out = reinterpret_cast<int32_t *>(b + o_aout);
            env->st_rew = reinterpret_cast<int32_t *>(b + o_rew); env->st_order = b + o_ord; env->st_done = b + o_done;
            env->st_mask = b + o_mask; env->st_obs = b + o_obs; env->st_obs_f32 = reinterpret_cast<float *>(b + o_f32);
            return SSD_OK;
        }
        if (h) (void)hipHostFree(h);
        (void)hipGetLastError();                 // fall back to device staging
    }
    if ((rc = dev_alloc(env, &env->st_actions, en))) return rc;
    if ((rc = dev_alloc(env, &env->st_actions_out, en))) return rc;
    if ((rc = dev_alloc(env, &env->st_rew, en))) return rc;
    if ((rc = dev_alloc(env, &env->st_order, en))) return rc;
    if ((rc = dev_alloc(env, &env->st_done, en))) return rc;
    if ((rc = dev_alloc(env, &env->st_mask, (size_t)env->E))) return rc;
    if ((rc = dev_alloc(env, &env->st_obs, obs_bytes(env)))) return rc;
    return SSD_OK;
}

// Runs one launch of the fused kernel with the per-call pointers filled in; handles host staging.
int run(ssd_env *env, int mode, const int32_t *actions, const uint8_t *order, const uint8_t *mask,
        int num_actions_random, int32_t *actions_out, void *obs_v, int32_t *rew, uint8_t *done, int rotate,
        uint32_t flags, void *stream) {
    {   // the stepping calls are launch-bound on the host: only switch devices when the thread is on another one
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || cur != env->device) SSD_HIP(env, hipSetDevice(env->device));
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t en = (size_t)env->E * env->N;
    const bool host = (flags & SSD_HOST_PTRS) != 0, f32 = (flags & SSD_OBS_F32) != 0;
    uint8_t *obs = static_cast<uint8_t *>(obs_v);
    Params p = env->p;
    p.obs_f32 = f32 ? 1 : 0;
    p.mode = mode; p.rotate = rotate; p.num_actions_random = num_actions_random;
    if (!host) {
        if (obs && (reinterpret_cast<uintptr_t>(obs) & 3u)) { env->err = "obs must be 4-byte aligned"; return SSD_E_INVALID; }
        env->last_stream = s; env->last_stream_set = true;
        p.actions = actions; p.order = order; p.mask = mask; p.actions_out = actions_out;
        p.obs = obs; p.rew = rew; p.done = done;
        ssd::launch(p, env->game, stream);
        SSD_HIP(env, hipGetLastError());
        return SSD_OK;
    }
    if (env->last_stream_set && env->last_stream != s) {
        SSD_HIP(env, hipStreamSynchronize(env->last_stream));
        env->last_stream_set = false;
    }
    int rc = ensure_staging(env);
    if (rc) return rc;
    if (env->st_mapped) {
        // the staging block is host memory the GPU addresses directly: plain memcpy in, one launch, one wait, memcpy out
        auto hostp = [&](const void *dev) { return env->st_host + (static_cast<const uint8_t *>(dev) - reinterpret_cast<const uint8_t *>(env->st_actions)); };
        if (actions) { std::memcpy(hostp(env->st_actions), actions, en * sizeof(int32_t)); p.actions = env->st_actions; }
        if (order) { std::memcpy(hostp(env->st_order), order, en); p.order = env->st_order; }
        if (mask) { std::memcpy(hostp(env->st_mask), mask, (size_t)env->E); p.mask = env->st_mask; }
        if (actions_out) p.actions_out = env->st_actions_out;
        if (obs) {
            p.obs = f32 ? reinterpret_cast<uint8_t *>(env->st_obs_f32) : env->st_obs;
            if (mask) std::memcpy(hostp(p.obs), obs, obs_bytes(env, f32));      // rows of envs that are not reset come back unchanged
        }
        if (rew) p.rew = env->st_rew;
        if (done) p.done = env->st_done;
        ssd::launch(p, env->game, stream);
        SSD_HIP(env, hipGetLastError());
        SSD_HIP(env, hipStreamSynchronize(s));
        if (actions_out) std::memcpy(actions_out, hostp(env->st_actions_out), en * sizeof(int32_t));
        if (obs) std::memcpy(obs, hostp(p.obs), obs_bytes(env, f32));
        if (rew) std::memcpy(rew, hostp(env->st_rew), en * sizeof(int32_t));
        if (done) std::memcpy(done, hostp(env->st_done), en);
        return SSD_OK;
    }
    if (actions) { SSD_HIP(env, hipMemcpyAsync(env->st_actions, actions, en * sizeof(int32_t), hipMemcpyHostToDevice, s)); p.actions = env->st_actions; }
    if (order) { SSD_HIP(env, hipMemcpyAsync(env->st_order, order, en, hipMemcpyHostToDevice, s)); p.order = env->st_order; }
    if (mask) { SSD_HIP(env, hipMemcpyAsync(env->st_mask, mask, (size_t)env->E, hipMemcpyHostToDevice, s)); p.mask = env->st_mask; }
    if (actions_out) p.actions_out = env->st_actions_out;
    if (obs) {
        if (f32 && !env->st_obs_f32) { if ((rc = dev_alloc(env, &env->st_obs_f32, obs_bytes(env) /* floats */))) return rc; }
        p.obs = f32 ? reinterpret_cast<uint8_t *>(env->st_obs_f32) : env->st_obs;
        if (mask)   // rows of envs that are not reset must come back unchanged
            SSD_HIP(env, hipMemcpyAsync(p.obs, obs, obs_bytes(env, f32), hipMemcpyHostToDevice, s));
    }
    if (rew) p.rew = env->st_rew;
    if (done) p.done = env->st_done;
    ssd::launch(p, env->game, stream);
    SSD_HIP(env, hipGetLastError());
    if (actions_out) SSD_HIP(env, hipMemcpyAsync(actions_out, env->st_actions_out, en * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (obs) SSD_HIP(env, hipMemcpyAsync(obs, p.obs, obs_bytes(env, f32), hipMemcpyDeviceToHost, s));
    if (rew) SSD_HIP(env, hipMemcpyAsync(rew, env->st_rew, en * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (done) SSD_HIP(env, hipMemcpyAsync(done, env->st_done, en, hipMemcpyDeviceToHost, s));
    SSD_HIP(env, hipStreamSynchronize(s));
    return SSD_OK;
}

}  // namespace

extern "C" {

int ssd_abi_version(void) { return SSD_ABI_VERSION; }

const char *ssd_last_error(const ssd_env *env) { return env ? env->err.c_str() : g_create_error.c_str(); }

int ssd_create(const ssd_config *cfg, ssd_env **out) {
    if (!cfg || !out) return fail_create("null argument", SSD_E_INVALID);
    *out = nullptr;
    if (cfg->struct_size != sizeof(ssd_config)) return fail_create("ssd_config.struct_size mismatch", SSD_E_INVALID);
    const int H = cfg->height, W = cfg->width, N = cfg->num_agents, E = cfg->num_envs;
    const int V = 2 * cfg->view_len + 1;
    if (cfg->game != SSD_GAME_HARVEST && cfg->game != SSD_GAME_CLEANUP) return fail_create("unknown game", SSD_E_INVALID);
    if (!cfg->base_map || H < 3 || W < 3 || H > 4095 || W > 4095 || (long)H * W > ssd::kMaxCells)
        return fail_create("map must be 3..4095 on a side with at most 4096 cells", SSD_E_INVALID);
    if (E < 1 || N < 0 || N > ssd::kMaxAgents) return fail_create("need num_envs >= 1 and 0 <= num_agents <= 64", SSD_E_INVALID);
    if (cfg->view_len < 0 || cfg->view_len > 15) return fail_create("view_len must be 0..15", SSD_E_INVALID);
    if (cfg->beam_len < 0 || cfg->beam_len > ssd::kMaxBeamLen) return fail_create("beam_len must be 0..21", SSD_E_INVALID);
    const int hw = H * W;
    // Appendix C.11 of SURVEY.md: the reference indexes out of range on maps without a closed wall
    // border (agent.py:111); the engine rejects them.
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            const char ch = cfg->base_map[r * W + c];
            if ((r == 0 || c == 0 || r == H - 1 || c == W - 1) && ch != '@') return fail_create("map border must be all '@'", SSD_E_INVALID);
            if (ch <= 0) return fail_create("map cells must be 7-bit ASCII", SSD_E_INVALID);
        }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail_create("no HIP device available: this engine has no CPU path", SSD_E_DEVICE);
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail_create("device_id out of range", SSD_E_INVALID);
    if (hipSetDevice(cfg->device_id) != hipSuccess) return fail_create("hipSetDevice failed", SSD_E_DEVICE);

    ssd_env *env = new ssd_env();
    env->game = cfg->game; env->H = H; env->W = W; env->E = E; env->N = N;
    env->view_len = cfg->view_len; env->V = V; env->beam_len = cfg->beam_len;
    env->device = cfg->device_id; env->keep_beams = cfg->keep_beams ? 1 : 0;
    env->seed = cfg->seed; env->env_base = cfg->env_index_base;
    // grid layout (ssd_kernels.hip): row stride WP = W + view_len, padding = void glyph; LDS aprons of view_len rows
    const int WP = W + cfg->view_len, S = (H * WP + 15) & ~15;
    env->WP = WP; env->S = S;

    // static per-map tables (map_env.py:93-101, harvest.py:22-26, cleanup.py:44-62)
    std::vector<uint8_t> reset_world(S, kVoid);
    std::vector<uint32_t> spawn_cells, apple_cells, waste_cells;   // grid index | dense index << 16
    const char apple_ch = cfg->game == SSD_GAME_HARVEST ? 'A' : 'B';
    for (int dc = 0; dc < hw; ++dc) {
        const char b = cfg->base_map[dc];
        const int c = (dc / W) * WP + dc % W;                   // grid index of the cell
        const uint32_t entry = (uint32_t)c | ((uint32_t)dc << 16);
        if (b == apple_ch) apple_cells.push_back(entry);
        if (cfg->game == SSD_GAME_CLEANUP && (b == 'H' || b == 'R')) { waste_cells.push_back(entry); env->potential_waste++; }
        if (b == 'P') spawn_cells.push_back(entry);
        char w = ' ';                         // reset_map (:560-564) + custom_reset (harvest.py:57-60, cleanup.py:84-92)
        if (b == '@') w = '@';
        else if (cfg->game == SSD_GAME_HARVEST && b == 'A') w = 'A';
        else if (cfg->game == SSD_GAME_CLEANUP && (b == 'H' || b == 'R' || b == 'S')) w = b;
        reset_world[c] = (uint8_t)w;
    }
    std::vector<uint32_t> lut(128, 0);
    if (cfg->color_lut) {
        for (int i = 0; i < 128; ++i)
            lut[i] = cfg->color_lut[3 * i] | (cfg->color_lut[3 * i + 1] << 8) | (cfg->color_lut[3 * i + 2] << 16);
    } else {                                  // map_env.py:24-41 DEFAULT_COLOURS + cleanup.py:15-18 CLEANUP_COLORS
        auto set = [&](char ch, int r, int g, int b) { lut[(int)ch] = r | (g << 8) | (b << 16); };
        set('@', 180, 180, 180); set('A', 0, 255, 0); set('F', 255, 255, 0); set('P', 159, 67, 255);
        set('1', 159, 67, 255); set('2', 2, 81, 154); set('3', 204, 0, 204); set('4', 216, 30, 54);
        set('5', 254, 151, 0); set('6', 100, 255, 255); set('7', 99, 99, 255); set('8', 250, 204, 255);
        set('9', 238, 223, 16); set('C', 100, 255, 255); set('S', 113, 75, 24); set('H', 99, 156, 194);
        set('R', 113, 75, 24);
    }
    const int n_thr = env->potential_waste + 1;
    std::vector<uint64_t> thr_ca(n_thr), thr_cw(n_thr);
    for (int n = 0; n < n_thr; ++n) {
        if (cfg->cleanup_apple_thresholds && cfg->cleanup_waste_thresholds) {
            thr_ca[n] = cfg->cleanup_apple_thresholds[n]; thr_cw[n] = cfg->cleanup_waste_thresholds[n];
        } else {
            double pa, pw;
            cleanup_probs(env->potential_waste, n, &pa, &pw);
            thr_ca[n] = threshold(pa); thr_cw[n] = threshold(pw);
        }
    }

    Params &p = env->p;
    p.E = E; p.E_total = E; p.ring = 1; p.N = N; p.H = H; p.W = W; p.WP = WP; p.S = S;
    p.A0 = (cfg->view_len * (WP + 1) + 15) & ~15;
    p.A1 = (cfg->view_len * WP + 15) & ~15;
    p.view_len = cfg->view_len; p.V = V; p.beam_len = cfg->beam_len;
    p.keep_beams = env->keep_beams;
    p.v_magic16 = (65536u + (uint32_t)V - 1u) / (uint32_t)V;
    p.seed_lo = (uint32_t)cfg->seed; p.seed_hi = (uint32_t)(cfg->seed >> 32); p.env_base = cfg->env_index_base;
    p.n_spawn = (int)spawn_cells.size(); p.n_thr = n_thr;
    p.n_apple = (int)apple_cells.size(); p.n_waste = (int)waste_cells.size();
    p.n_waste_reset = 0;
    for (uint8_t ch : reset_world) p.n_waste_reset += ch == 'H';
    const double sp[4] = {0, 0.005, 0.02, 0.05};   // harvest.py:13 SPAWN_PROB
    for (int i = 0; i < 4; ++i) {
        const uint64_t T = cfg->harvest_thresholds ? cfg->harvest_thresholds[i] : threshold(sp[i]);
        p.thr_h32[i] = T >= 4294967296ull ? 0xFFFFFFFFu : (uint32_t)T;
        if (T >= 4294967296ull) p.thr_h_always |= 1u << i;
    }

    auto bail = [&](int rc) {
        g_create_error = env->err;
        for (void *ptr : env->allocs) (void)hipFree(ptr);
        delete env;
        return rc;
    };
    int rc;
    if (ssd::lds_bytes(p, 1, true) > 64 * 1024) { env->err = "map too large for the 64 KiB LDS budget"; return bail(SSD_E_INVALID); }
    if ((rc = dev_alloc(env, &p.world, (size_t)E * S))) return bail(rc);
    if (env->keep_beams) { if ((rc = dev_alloc(env, &p.beam, (size_t)E * S))) return bail(rc); }
    if ((rc = dev_alloc(env, &p.agents, (size_t)E * N))) return bail(rc);
    if (N > 0) {   // before the first reset every agent sits on interior cell (1,1), facing UP: stepping an env that
                   // was never reset is then well defined and cannot index outside the grid
        std::vector<uint32_t> ag((size_t)E * N, (uint32_t)(WP + 1) | (2u << 16));
        if (hipMemcpy(p.agents, ag.data(), ag.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { env->err = "hipMemcpy(agents)"; return bail(SSD_E_DEVICE); }
    }
    if ((rc = dev_alloc(env, &p.status, 1))) return bail(rc);
    {   // header: episode = 0xFFFFFFFF ("never reset"; the first reset wraps it to 0)
        std::vector<uint4> hdr(E);
        for (int e = 0; e < E; ++e) hdr[e] = make_uint4(0, 0, 0xFFFFFFFFu, 0);
        if ((rc = upload(env, &p.hdr, hdr))) return bail(rc);
        std::vector<uint8_t> w0((size_t)E * S, kVoid);   // world starts blank (map_env.py:85)
        for (int e = 0; e < E; ++e)
            for (int r = 0; r < H; ++r) std::memset(w0.data() + (size_t)e * S + (size_t)r * WP, ' ', W);
        if (hipMemcpy(p.world, w0.data(), w0.size(), hipMemcpyHostToDevice) != hipSuccess) { env->err = "hipMemcpy(world)"; return bail(SSD_E_DEVICE); }
    }
    uint8_t *d8; uint32_t *d32; uint64_t *d64;
    if ((rc = upload(env, &d8, reset_world))) return bail(rc);
    p.reset_world = d8;
    if ((rc = upload(env, &d32, spawn_cells))) return bail(rc);
    p.spawn_cells = d32;
    if ((rc = upload(env, &d32, apple_cells))) return bail(rc);
    p.apple_cells = d32;
    if ((rc = upload(env, &d32, waste_cells))) return bail(rc);
    p.waste_cells = d32;
    if ((rc = upload(env, &d32, lut))) return bail(rc);
    p.lut = d32;
    {   // float32 of the reference's float64 normalisation (map_env.py:199), one entry per byte value
        // ... applied to the colour table: glyph -> (r, g, b, 0) as float32, one 16-byte entry per glyph
        std::vector<float> f32lut(128 * 4, 0.0f);
        for (int g = 0; g < 128; ++g)
            for (int c = 0; c < 3; ++c) f32lut[4 * g + c] = (float)(((double)((lut[g] >> (8 * c)) & 0xFFu) - 128.0) / 255.0);
        float *df;
        if ((rc = upload(env, &df, f32lut))) return bail(rc);
        p.f32lut = df;
    }
    if (cfg->view_len == 7) {   // the per-lane window offsets of the 15 x 15 view (ssd_kernels.hip, render_views_std): constants of the row stride
        std::vector<uint32_t> vt(64 * 8);
        for (int l = 0; l < 64; ++l) {
            const int pp0 = 4 * l > 221 ? 221 : 4 * l;
            for (int q = 0; q < 4; ++q) {
                const int pp = pp0 + q, i = pp / 15, j = pp % 15;
                vt[l * 8 + q] = (uint32_t)(i * WP + j);
                vt[l * 8 + 4 + q] = (uint32_t)(j * WP + (14 - i));
            }
        }
        if ((rc = upload(env, &d32, vt))) return bail(rc);
        p.view_tab = d32;
    }
    if ((rc = upload(env, &d64, thr_ca))) return bail(rc);
    p.thr_ca = d64;
    if ((rc = upload(env, &d64, thr_cw))) return bail(rc);
    p.thr_cw = d64;
    *out = env;
    return SSD_OK;
}

int ssd_destroy(ssd_env *env) {
    if (!env) return SSD_E_INVALID;
    stop_workers(env);
    (void)hipSetDevice(env->device);
    (void)hipDeviceSynchronize();
    aql_teardown(env);
    for (void *ptr : env->allocs) (void)hipFree(ptr);
    for (void *ptr : env->host_allocs) (void)hipHostFree(ptr);
    for (hipStream_t cs : env->chain_streams) (void)hipStreamDestroy(cs);
    for (hipEvent_t ce : env->chain_events) (void)hipEventDestroy(ce);
    if (env->fork_event) (void)hipEventDestroy(env->fork_event);
    delete env;
    return SSD_OK;
}

int ssd_reset(ssd_env *env, const uint8_t *env_mask, void *obs, uint32_t flags, void *stream) {
    if (!env) return SSD_E_INVALID;
    return run(env, ssd::kModeReset, nullptr, nullptr, env_mask, 0, nullptr, obs, nullptr, nullptr, /*rotate=*/0, flags, stream);
}

int ssd_step(ssd_env *env, const int32_t *actions, const uint8_t *order, void *obs, int32_t *rew, uint8_t *done,
             uint32_t flags, void *stream) {
    if (!env) return SSD_E_INVALID;
    if (!actions && env->N > 0) { env->err = "actions is null"; return SSD_E_INVALID; }   // an env without agents has no actions
    if ((flags & SSD_AUTO_RESET) && (flags & SSD_OBS_F32)) { env->err = "an auto-reset step writes uint8 observations"; return SSD_E_INVALID; }
    return run(env, (flags & SSD_AUTO_RESET) ? ssd::kModeStepAuto : ssd::kModeStep, actions, order, nullptr, 0, nullptr, obs, rew, done, 1,
               flags, stream);
}

int ssd_step_random(ssd_env *env, int32_t num_actions, int32_t *actions_out, void *obs, int32_t *rew, uint8_t *done,
                    uint32_t flags, void *stream) {
    if (!env) return SSD_E_INVALID;
    if (num_actions < 1 || num_actions > game_actions(env)) { env->err = "num_actions outside the game's Discrete(n)"; return SSD_E_INVALID; }
    if ((flags & SSD_AUTO_RESET) && (flags & SSD_OBS_F32)) { env->err = "an auto-reset step writes uint8 observations"; return SSD_E_INVALID; }
    return run(env, (flags & SSD_AUTO_RESET) ? ssd::kModeStepAuto : ssd::kModeStep, nullptr, nullptr, nullptr, num_actions, actions_out, obs,
               rew, done, 1, flags, stream);
}

int ssd_observe(ssd_env *env, void *obs, uint32_t flags, void *stream) {
    if (!env || !obs) return SSD_E_INVALID;
    return run(env, ssd::kModeObserve, nullptr, nullptr, nullptr, 0, nullptr, obs, nullptr, nullptr,
               (flags & SSD_NO_ROTATE) ? 0 : 1, flags, stream);
}

int ssd_get_state(ssd_env *env, int8_t *world, int8_t *beam, int16_t *pos, uint8_t *orient, uint32_t *episode, uint32_t *t) {
    if (!env) return SSD_E_INVALID;
    SSD_HIP(env, hipSetDevice(env->device));
    SSD_HIP(env, hipDeviceSynchronize());
    const int E = env->E, N = env->N, S = env->S, WP = env->WP;
    if (world || beam) {
        std::vector<uint8_t> buf((size_t)E * S);
        if (world) {
            SSD_HIP(env, hipMemcpy(buf.data(), env->p.world, buf.size(), hipMemcpyDeviceToHost));
            unpack_grid(env, buf, world);
        }
        if (beam) {
            if (!env->keep_beams) { env->err = "beam overlay is only kept with keep_beams"; return SSD_E_INVALID; }
            SSD_HIP(env, hipMemcpy(buf.data(), env->p.beam, buf.size(), hipMemcpyDeviceToHost));
            unpack_grid(env, buf, beam);
        }
    }
    if (pos || orient) {
        std::vector<uint32_t> ag((size_t)E * N);
        if (!ag.empty()) SSD_HIP(env, hipMemcpy(ag.data(), env->p.agents, ag.size() * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < ag.size(); ++i) {
            const uint32_t cell = ag[i] & 0xFFFFu;
            if (pos) { pos[2 * i] = (int16_t)(cell / WP); pos[2 * i + 1] = (int16_t)(cell % WP); }
            if (orient) orient[i] = (uint8_t)((ag[i] >> 16) & 3u);
        }
    }
    if (episode || t) {
        std::vector<uint4> hdr(E);
        SSD_HIP(env, hipMemcpy(hdr.data(), env->p.hdr, hdr.size() * sizeof(uint4), hipMemcpyDeviceToHost));
        for (int e = 0; e < E; ++e) { if (episode) episode[e] = hdr[e].z; if (t) t[e] = hdr[e].y; }
    }
    return SSD_OK;
}

int ssd_get_waste_count(ssd_env *env, uint32_t *waste_count) {
    if (!env || !waste_count) return SSD_E_INVALID;
    SSD_HIP(env, hipSetDevice(env->device));
    SSD_HIP(env, hipDeviceSynchronize());
    std::vector<uint4> hdr(env->E);
    SSD_HIP(env, hipMemcpy(hdr.data(), env->p.hdr, hdr.size() * sizeof(uint4), hipMemcpyDeviceToHost));
    for (int e = 0; e < env->E; ++e) waste_count[e] = hdr[e].w & 0xFFFFu;   // (upper half: the grid's current count, kernel-internal)
    return SSD_OK;
}

static uint32_t host_mix32(uint32_t x) {
    x ^= x >> 17; x *= 0xED5AD4BBu; x ^= x >> 11; x *= 0xAC4C1B51u; x ^= x >> 15; x *= 0x31848BABu; x ^= x >> 14;
    return x;
}

int ssd_set_state(ssd_env *env, const int8_t *world, const int8_t *beam, const int16_t *pos, const uint8_t *orient,
                  const uint32_t *episode, const uint32_t *t) {
    if (!env) return SSD_E_INVALID;
    SSD_HIP(env, hipSetDevice(env->device));
    SSD_HIP(env, hipDeviceSynchronize());
    const int E = env->E, N = env->N, hw = env->H * env->W, W = env->W, H = env->H, WP = env->WP;
    if (world || beam) {
        std::vector<uint8_t> buf;
        // glyphs index the 128-entry colour table on the device: cells must be 7-bit ASCII
        for (size_t i = 0; world && i < (size_t)E * hw; ++i)
            if (world[i] <= 0) { env->err = "world cells must be 7-bit ASCII (1..127)"; return SSD_E_INVALID; }
        for (size_t i = 0; beam && i < (size_t)E * hw; ++i)
            if (beam[i] < 0) { env->err = "beam cells must be 0 or 7-bit ASCII"; return SSD_E_INVALID; }
        if (world) {
            // the wall border is what keeps agents and beams inside the grid (the kernel has no bounds tests)
            for (int e = 0; e < E; ++e)
                for (int r = 0; r < H; ++r)
                    for (int c = 0; c < W; c += (r == 0 || r == H - 1 || c == W - 1) ? 1 : W - 1)
                        if (world[((size_t)e * H + r) * W + c] != '@') { env->err = "the map border must stay '@'"; return SSD_E_INVALID; }
            pack_grid(env, world, buf, kVoid);
            SSD_HIP(env, hipMemcpy(env->p.world, buf.data(), buf.size(), hipMemcpyHostToDevice));
        }
        if (beam) {
            if (!env->keep_beams) { env->err = "beam overlay is only kept with keep_beams"; return SSD_E_INVALID; }
            pack_grid(env, beam, buf, 0);
            SSD_HIP(env, hipMemcpy(env->p.beam, buf.data(), buf.size(), hipMemcpyHostToDevice));
        }
    }
    std::vector<uint8_t> share;
    if ((pos || orient) && N > 0) {
        std::vector<uint32_t> ag((size_t)E * N);
        SSD_HIP(env, hipMemcpy(ag.data(), env->p.agents, ag.size() * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < ag.size(); ++i) {
            uint32_t cell = ag[i] & 0xFFFFu, o = (ag[i] >> 16) & 3u;
            if (pos) {
                const int r = pos[2 * i], c = pos[2 * i + 1];
                // agents live strictly inside the wall border; a position on the border could step out of the grid
                if (r < 1 || r >= H - 1 || c < 1 || c >= W - 1) { env->err = "agent position must be inside the map's wall border"; return SSD_E_INVALID; }
                cell = (uint32_t)(r * WP + c);
            }
            if (orient) { if (orient[i] > 3) { env->err = "orientation code must be 0..3"; return SSD_E_INVALID; } o = orient[i]; }
            ag[i] = cell | (o << 16);
        }
        SSD_HIP(env, hipMemcpy(env->p.agents, ag.data(), ag.size() * 4, hipMemcpyHostToDevice));
        if (pos) {                                  // hdr.w bit 31: two agents of the env share a cell (the kernel's move phase asks)
            share.assign(E, 0);
            for (int e = 0; e < E; ++e)
                for (int i = 0; i < N; ++i)
                    for (int j = i + 1; j < N; ++j)
                        if (((ag[(size_t)e * N + i] ^ ag[(size_t)e * N + j]) & 0xFFFFu) == 0) share[e] = 1;
        }
    }
    const bool recount = world && env->game == SSD_GAME_CLEANUP;      // the kernel keeps the grid's 'H' count in hdr.w
    if (episode || t || recount || !share.empty()) {
        std::vector<uint4> hdr(E);
        SSD_HIP(env, hipMemcpy(hdr.data(), env->p.hdr, hdr.size() * sizeof(uint4), hipMemcpyDeviceToHost));
        for (int e = 0; e < E; ++e) {
            if (recount) {
                uint32_t n = 0;
                for (int i = 0; i < hw; ++i) n += world[(size_t)e * hw + i] == 'H';
                hdr[e].w = (hdr[e].w & 0x8000FFFFu) | (n << 16);
            }
            if (!share.empty()) hdr[e].w = (hdr[e].w & 0x7FFFFFFFu) | ((uint32_t)share[e] << 31);
            if (t) hdr[e].y = t[e];
            if (episode) {
                hdr[e].z = episode[e];
                uint32_t h = 0x243F6A88u;         // env_key(seed, env, episode), prng.py
                h = host_mix32(h ^ (uint32_t)env->seed);
                h = host_mix32(h ^ (uint32_t)(env->seed >> 32));
                h = host_mix32(h ^ (env->env_base + (uint32_t)e));
                h = host_mix32(h ^ episode[e]);
                hdr[e].x = h;
            }
        }
        SSD_HIP(env, hipMemcpy(env->p.hdr, hdr.data(), hdr.size() * sizeof(uint4), hipMemcpyHostToDevice));
    }
    return SSD_OK;
}

int ssd_render_frames(ssd_env *env, int32_t e_begin, int32_t count, uint8_t *rgb, uint32_t flags, void *stream) {
    if (!env || !rgb || e_begin < 0 || count < 0 || (int64_t)e_begin + count > env->E) return SSD_E_INVALID;
    if (flags & ~(uint32_t)SSD_HOST_PTRS) { env->err = "ssd_render_frames: only the host-pointer flag is meaningful here"; return SSD_E_INVALID; }
    if (count == 0) return SSD_OK;
    SSD_HIP(env, hipSetDevice(env->device));
    const size_t frame = (size_t)env->H * env->W * 3;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *dst = rgb;
    if (flags & SSD_HOST_PTRS) {                       // frames are rendered into a device buffer of the handle and copied back
        if (env->st_rgb_frames < (size_t)count) {
            void *ptr = nullptr;
            hipError_t e = hipMalloc(&ptr, (size_t)count * frame);
            if (e != hipSuccess) { env->err = std::string("hipMalloc: ") + hipGetErrorString(e); return SSD_E_NOMEM; }
            if (env->st_rgb) {
                SSD_HIP(env, hipDeviceSynchronize());
                for (auto &a : env->allocs) if (a == env->st_rgb) a = ptr;
                SSD_HIP(env, hipFree(env->st_rgb));
            } else {
                env->allocs.push_back(ptr);
            }
            env->st_rgb = static_cast<uint8_t *>(ptr);
            env->st_rgb_frames = (size_t)count;
        }
        dst = env->st_rgb;
    }
    for (int32_t k = 0; k < count; k += 32768) {       // gridDim.y carries the env: at most 65535 per launch
        const int32_t n = count - k < 32768 ? count - k : 32768;
        ssd::launch_render_full(env->p, e_begin + k, n, dst + (size_t)k * frame, s);
    }
    SSD_HIP(env, hipGetLastError());
    if (flags & SSD_HOST_PTRS) {
        SSD_HIP(env, hipMemcpyAsync(rgb, dst, (size_t)count * frame, hipMemcpyDeviceToHost, s));
        SSD_HIP(env, hipStreamSynchronize(s));
    }
    return SSD_OK;
}

int ssd_render_full(ssd_env *env, int32_t e, uint8_t *rgb) {
    if (!env || !rgb || e < 0 || e >= env->E) return SSD_E_INVALID;
    SSD_HIP(env, hipSetDevice(env->device));
    SSD_HIP(env, hipDeviceSynchronize());              // (this entry point takes no stream: order it after everything enqueued)
    return ssd_render_frames(env, e, 1, rgb, SSD_HOST_PTRS, nullptr);
}

int ssd_agent_action_obs(ssd_env *env, const int32_t *actions, const uint8_t *done_mask, int64_t *other_actions, int64_t *visible,
                         uint32_t flags, void *stream) {
    if (!env) return SSD_E_INVALID;
    if (flags & ~(uint32_t)SSD_HOST_PTRS) { env->err = "ssd_agent_action_obs: only the host-pointer flag is meaningful here"; return SSD_E_INVALID; }
    const int E = env->E, N = env->N;
    if (N < 2 || (!other_actions && !visible)) return SSD_OK;           // (N - 1 == 0 columns)
    SSD_HIP(env, hipSetDevice(env->device));
    ssd::AgentOrder ord;
    {   // ids 'agent-<i>' sorted as strings (harvest.py:50, map_env.py:202)
        std::vector<std::pair<std::string, int>> ids;
        for (int i = 0; i < N; ++i) ids.emplace_back("agent-" + std::to_string(i), i);
        std::sort(ids.begin(), ids.end());
        std::memset(&ord, 0, sizeof(ord));
        for (int r = 0; r < N; ++r) { ord.sorted[r] = (uint8_t)ids[r].second; ord.rank[ids[r].second] = (uint8_t)r; }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t en = (size_t)E * N, out_n = en * (size_t)(N - 1);
    if (!(flags & SSD_HOST_PTRS)) {
        ssd::launch_agent_action_obs(actions, done_mask, reinterpret_cast<long long *>(other_actions), reinterpret_cast<long long *>(visible), ord, E, N, stream);
        SSD_HIP(env, hipGetLastError());
        return SSD_OK;
    }
    // host arrays: staged through scratch device buffers of this call (a convenience surface, not a fast path)
    int32_t *d_act = nullptr; uint8_t *d_mask = nullptr; long long *d_out = nullptr, *d_vis = nullptr;
    auto cleanup = [&]() { if (d_act) (void)hipFree(d_act); if (d_mask) (void)hipFree(d_mask); if (d_out) (void)hipFree(d_out); if (d_vis) (void)hipFree(d_vis); };
    auto fail = [&](const char *what) { env->err = what; cleanup(); return SSD_E_DEVICE; };
    if (actions) { if (hipMalloc(&d_act, en * 4) != hipSuccess || hipMemcpyAsync(d_act, actions, en * 4, hipMemcpyHostToDevice, s) != hipSuccess) return fail("staging actions"); }
    if (done_mask) { if (hipMalloc(&d_mask, en) != hipSuccess || hipMemcpyAsync(d_mask, done_mask, en, hipMemcpyHostToDevice, s) != hipSuccess) return fail("staging done_mask"); }
    if (other_actions && hipMalloc(&d_out, out_n * 8) != hipSuccess) return fail("staging other_actions");
    if (visible && hipMalloc(&d_vis, out_n * 8) != hipSuccess) return fail("staging visible");
    ssd::launch_agent_action_obs(d_act, d_mask, d_out, d_vis, ord, E, N, stream);
    if (hipGetLastError() != hipSuccess) return fail("kernel launch");
    if (other_actions && hipMemcpyAsync(other_actions, d_out, out_n * 8, hipMemcpyDeviceToHost, s) != hipSuccess) return fail("copy back");
    if (visible && hipMemcpyAsync(visible, d_vis, out_n * 8, hipMemcpyDeviceToHost, s) != hipSuccess) return fail("copy back");
    if (hipStreamSynchronize(s) != hipSuccess) return fail("synchronize");
    cleanup();
    return SSD_OK;
}

int ssd_set_horizon(ssd_env *env, int32_t horizon) {
    if (!env || horizon < 0) return SSD_E_INVALID;
    env->p.horizon = horizon;
    return SSD_OK;
}

}  // extern "C"

// A closed-loop rollout: per step the policy's launches (ssd_policy*.hip: forward + action into the ring slot), then the step
// launch of ssd_step(..., SSD_AUTO_RESET) reading those actions.  All through hipLaunchKernel on `stream`: the library's AQL
// chains (ssd_rollout_actions) are not used here.  The three policies share the argument rules and the
// loop below; each adds its own rules, its argument blocks and its launches.
namespace {

constexpr size_t kPolObs = (size_t)SSD_POL_VIEW * SSD_POL_VIEW * 3;    // observation bytes per agent

// the rules of the step counts and the optional state ring (null: none); null = fine
const char *check_rollout_steps(int32_t n_steps, int32_t step0, int32_t ring, const float *state_ring, int32_t state_ring_len,
                                int32_t state_every) {
    if (n_steps < 1) return "n_steps must be >= 1";
    if (ring < 1) return "ring must be >= 1";
    if (step0 < 0) return "step0 must be >= 0";
    if (state_ring) {
        if (state_every < 1) return "state_every must be >= 1";
        if ((int64_t)state_ring_len * state_every < n_steps) return "the state ring needs ceil(n_steps / state_every) slots";
    }
    return nullptr;
}

// the rules of the flags and the observation ring; null = fine
const char *check_rollout_obs(const ssd_env *env, uint32_t flags, const uint8_t *obs, int32_t ring) {
    if (flags & ~(uint32_t)SSD_POLICY_GREEDY) return "flags: only the greedy-policy bit is defined";
    if (reinterpret_cast<uintptr_t>(obs) & 3u) return "obs must be 4-byte aligned";
    if (ring > 1 && (((size_t)env->E * env->N * kPolObs) & 3u))
        return "an observation ring of more than one slot needs E * N to be a multiple of 4 (4-byte aligned slots)";
    return nullptr;
}

// The loop: step k acts on obs_in (k = 0) or the previous slot's observations and writes ring slot (step0 + k) % ring.
// policy(k, obs_k, slot) launches the policy, leaving the actions in actions[slot]; last(obs) what follows the loop (the
// last_value pass on the final observations).  Both return SSD_OK or an error code with env->err set (SSD_HIP).
template <class Policy, class Last>
int rollout_policy_steps(ssd_env *env, const uint8_t *obs_in, int32_t n_steps, int32_t step0, int32_t ring, uint8_t *obs,
                         int32_t *actions, int32_t *rew, uint8_t *done, void *stream, Policy policy, Last last) {
    if (const hipError_t e = ssd::select_device(env->device)) {
        env->err = std::string("hipSetDevice(env->device): ") + hipGetErrorString(e);
        return SSD_E_DEVICE;
    }
    const size_t en = (size_t)env->E * env->N, ob = en * kPolObs;
    size_t slot = 0;
    for (int32_t k = 0; k < n_steps; ++k) {
        const size_t prev = slot;
        slot = (size_t)(((int64_t)step0 + k) % ring);
        int rc = policy(k, k == 0 ? obs_in : obs + prev * ob, slot);
        if (rc) return rc;
        rc = run(env, ssd::kModeStepAuto, actions + slot * en, nullptr, nullptr, 0, nullptr, obs + slot * ob,
                           rew ? rew + slot * en : nullptr, done ? done + slot * en : nullptr, 1, 0, stream);
        if (rc) return rc;
    }
    return last(obs + slot * ob);
}

// slot `slot` of an optional ring of n elements per slot
template <class T>
T *ring_slot(T *p, size_t slot, size_t n) { return p ? p + slot * n : nullptr; }

}  // namespace

extern "C" {

int ssd_rollout_policy(ssd_env *env, const float *weights, int32_t num_sets, const uint8_t *obs_in, int32_t n_steps, int32_t step0,
                       uint8_t *obs, int32_t *actions, float *logp, float *value, float *logits, int32_t *rew, uint8_t *done,
                       int32_t ring, float *last_value, uint32_t flags, void *stream) {
    if (!env) return SSD_E_INVALID;
    auto bad = [&](const char *msg) { env->err = msg; return SSD_E_INVALID; };
    const int A = game_actions(env);
    if (env->view_len != 7 || env->V != SSD_POL_VIEW) return bad("policy rollouts need view_len 7 (15 x 15 observations)");
    if (env->N < 1) return bad("policy rollouts need at least one agent");
    if (!weights || !obs_in || !obs || !actions) return bad("weights, obs_in, obs and actions are required");
    if (const char *why = ssd::check_policy_net(ssd::kNetConvFc, weights, num_sets, env->N, A)) return bad(why);
    if (const char *why = check_rollout_steps(n_steps, step0, ring, nullptr, 0, 0)) return bad(why);
    if (const char *why = check_rollout_obs(env, flags, obs, ring)) return bad(why);
    const size_t en = (size_t)env->E * env->N;
    ssd::PolicyArgs pa{};
    pa.w = weights; pa.P = num_sets; pa.A = A; pa.B = env->E; pa.N = env->N; pa.set_floats = SSD_POL_SET_FLOATS(A);
    pa.hdr = env->p.hdr; pa.seed_lo = env->p.seed_lo; pa.seed_hi = env->p.seed_hi; pa.env_base = env->p.env_base;
    pa.greedy = (flags & SSD_POLICY_GREEDY) ? 1 : 0;
    return rollout_policy_steps(
        env, obs_in, n_steps, step0, ring, obs, actions, rew, done, stream,
        [&](int32_t, const uint8_t *o, size_t slot) -> int {
            pa.obs = o;
            pa.actions = actions + slot * en;
            pa.logp = ring_slot(logp, slot, en);
            pa.value = ring_slot(value, slot, en);
            pa.logits = ring_slot(logits, slot, en * A);
            SSD_HIP(env, ssd::launch_policy(pa, stream));
            return SSD_OK;
        },
        [&](const uint8_t *o) -> int {
            if (!last_value) return SSD_OK;
            pa.obs = o;
            pa.actions = nullptr; pa.logp = nullptr; pa.logits = nullptr; pa.value = last_value;
            SSD_HIP(env, ssd::launch_policy(pa, stream));
            return SSD_OK;
        });
}

int ssd_rollout_policy_lstm(ssd_env *env, const float *weights, int32_t num_sets, int32_t cell_size, const uint8_t *obs_in,
                            int32_t n_steps, int32_t step0, float *state, float *state_ring, int32_t state_ring_len,
                            int32_t state_every, float *features, uint8_t *obs, int32_t *actions, float *logp, float *value,
                            float *logits, int32_t *rew, uint8_t *done, int32_t ring, float *last_value, uint32_t flags,
                            void *stream) {
    if (!env) return SSD_E_INVALID;
    auto bad = [&](const char *msg) { env->err = msg; return SSD_E_INVALID; };
    const int A = game_actions(env);
    if (env->view_len != 7 || env->V != SSD_POL_VIEW) return bad("policy rollouts need view_len 7 (15 x 15 observations)");
    if (env->N < 1) return bad("policy rollouts need at least one agent");
    if (!weights || !obs_in || !obs || !actions || !state || !features)
        return bad("weights, obs_in, obs, actions, state and features are required");
    if (const char *why = ssd::check_policy_net(ssd::kNetLstm, weights, num_sets, env->N, A, cell_size)) return bad(why);
    if (const char *why = check_rollout_steps(n_steps, step0, ring, state_ring, state_ring_len, state_every)) return bad(why);
    if (const char *why = check_rollout_obs(env, flags, obs, ring)) return bad(why);
    const size_t en = (size_t)env->E * env->N, sn = en * 2 * cell_size;
    ssd::PolicyArgs tr{};                       // the trunk, features mode
    tr.w = weights; tr.P = num_sets; tr.A = A; tr.B = env->E; tr.N = env->N; tr.set_floats = SSD_LSTM_SET_FLOATS(cell_size, A);
    tr.feat = features;
    ssd::LstmArgs la{};
    la.w = weights; la.P = num_sets; la.A = A; la.B = env->E; la.N = env->N; la.C = cell_size; la.set_floats = tr.set_floats;
    la.feat = features; la.state_in = state; la.state_out = state;
    la.hdr = env->p.hdr; la.seed_lo = env->p.seed_lo; la.seed_hi = env->p.seed_hi; la.env_base = env->p.env_base;
    la.greedy = (flags & SSD_POLICY_GREEDY) ? 1 : 0;
    const auto both = [&](const uint8_t *o) -> int {
        tr.obs = o;
        SSD_HIP(env, ssd::launch_policy_features(tr, stream));
        SSD_HIP(env, ssd::launch_policy_lstm(la, stream));
        return SSD_OK;
    };
    return rollout_policy_steps(
        env, obs_in, n_steps, step0, ring, obs, actions, rew, done, stream,
        [&](int32_t k, const uint8_t *o, size_t slot) -> int {
            la.state_used = state_ring && k % state_every == 0 ? state_ring + (size_t)(k / state_every) * sn : nullptr;
            la.actions = actions + slot * en;
            la.logp = ring_slot(logp, slot, en);
            la.value = ring_slot(value, slot, en);
            la.logits = ring_slot(logits, slot, en * A);
            return both(o);
        },
        [&](const uint8_t *o) -> int {          // the final observation under the final state; the state stays as it is
            if (!last_value) return SSD_OK;
            la.state_out = nullptr; la.state_used = nullptr;
            la.actions = nullptr; la.logp = nullptr; la.logits = nullptr; la.value = last_value;
            return both(o);
        });
}

int ssd_rollout_policy_moa(ssd_env *env, const float *weights, int32_t num_sets, int32_t cell_size, const uint8_t *obs_in,
                           int32_t n_steps, int32_t step0, float *state, float *state_ring, int32_t state_ring_len,
                           int32_t state_every, int32_t *prev_actions, int32_t *prev_actions_ring, float *influence,
                           float influence_clip, float *scratch, uint8_t *obs, int32_t *actions, float *logp, float *value,
                           float *logits, int32_t *rew, uint8_t *done, int32_t ring, float *last_value, uint32_t flags,
                           void *stream) {
    if (!env) return SSD_E_INVALID;
    auto bad = [&](const char *msg) { env->err = msg; return SSD_E_INVALID; };
    const int A = game_actions(env);
    if (env->view_len != 7 || env->V != SSD_POL_VIEW) return bad("policy rollouts need view_len 7 (15 x 15 observations)");
    if (env->N < 2 || env->N > SSD_MOA_MAX_AGENTS) return bad("the MOA policy needs 2..16 agents");
    if (!weights || !obs_in || !obs || !actions || !state || !prev_actions || !scratch)
        return bad("weights, obs_in, obs, actions, state, prev_actions and scratch are required");
    if (const char *why = ssd::check_policy_net(ssd::kNetMoa, weights, num_sets, env->N, A, cell_size, scratch)) return bad(why);
    if (const char *why = check_rollout_steps(n_steps, step0, ring, state_ring, state_ring_len, state_every)) return bad(why);
    if (influence && !(influence_clip >= 0.f && influence_clip <= 3.0e38f)) return bad("influence_clip must be finite and >= 0");
    if (const char *why = check_rollout_obs(env, flags, obs, ring)) return bad(why);
    const size_t en = (size_t)env->E * env->N, sn = en * 4 * cell_size;
    // scratch (include/ssd.h): features [en][2][32], logits [en][16], the joint-action ping-pong i32 [2][en]
    int32_t *pp[2] = {reinterpret_cast<int32_t *>(scratch + 80 * en), reinterpret_cast<int32_t *>(scratch + 81 * en)};
    ssd::PolicyArgs tr{};                       // the trunk, MOA mode
    tr.w = weights; tr.P = num_sets; tr.A = A; tr.B = env->E; tr.N = env->N;
    tr.set_floats = SSD_MOA_SET_FLOATS(cell_size, A, env->N); tr.feat = scratch;
    ssd::MoaArgs ma{};
    ma.w = weights; ma.P = num_sets; ma.A = A; ma.B = env->E; ma.N = env->N; ma.C = cell_size; ma.set_floats = tr.set_floats;
    ma.feat = scratch; ma.state_in = state; ma.state_out = state; ma.logits_scratch = scratch + 64 * en;
    ma.hdr = env->p.hdr; ma.seed_lo = env->p.seed_lo; ma.seed_hi = env->p.seed_hi; ma.env_base = env->p.env_base;
    ma.greedy = (flags & SSD_POLICY_GREEDY) ? 1 : 0;
    ma.pi_logits = ma.logits_scratch; ma.pi_stride = 16; ma.clip = influence_clip;
    const auto trunk_actions = [&](const uint8_t *o) -> int {
        tr.obs = o;
        SSD_HIP(env, ssd::launch_policy_moa_features(tr, stream));
        SSD_HIP(env, ssd::launch_policy_moa_actions(ma, stream));
        return SSD_OK;
    };
    return rollout_policy_steps(
        env, obs_in, n_steps, step0, ring, obs, actions, rew, done, stream,
        [&](int32_t k, const uint8_t *o, size_t slot) -> int {
            ma.state_used = state_ring && k % state_every == 0 ? state_ring + (size_t)(k / state_every) * sn : nullptr;
            ma.actions = actions + slot * en;
            ma.actions_copy = pp[(k + 1) & 1];  // the next step's previous joint action: never the buffer this step reads
            ma.logp = ring_slot(logp, slot, en);
            ma.value = ring_slot(value, slot, en);
            ma.logits = ring_slot(logits, slot, en * A);
            if (const int rc = trunk_actions(o)) return rc;
            ma.prev = k == 0 ? prev_actions : pp[k & 1];
            ma.prev_used = ring_slot(prev_actions_ring, slot, en);
            ma.taken = influence ? ma.actions : nullptr;
            ma.influence = ring_slot(influence, slot, en);
            SSD_HIP(env, ssd::launch_policy_moa_cell(ma, stream));
            return SSD_OK;
        },
        [&](const uint8_t *o) -> int {
            SSD_HIP(env, hipMemcpyAsync(prev_actions, pp[n_steps & 1], en * sizeof(int32_t), hipMemcpyDeviceToDevice,
                                        static_cast<hipStream_t>(stream)));
            if (!last_value) return SSD_OK;
            // the final observation under the final state; the state stays as it is
            ma.state_out = nullptr; ma.state_used = nullptr; ma.actions = nullptr; ma.actions_copy = nullptr; ma.logp = nullptr;
            ma.logits = nullptr; ma.logits_scratch = nullptr; ma.value = last_value;
            return trunk_actions(o);
        });
}

int ssd_potential_waste_area(const ssd_env *env) { return env ? env->potential_waste : SSD_E_INVALID; }

int ssd_device_status(ssd_env *env, uint32_t *status, int clear) {
    if (!env || !status) return SSD_E_INVALID;
    SSD_HIP(env, hipSetDevice(env->device));
    SSD_HIP(env, hipDeviceSynchronize());
    SSD_HIP(env, hipMemcpy(status, env->p.status, 4, hipMemcpyDeviceToHost));
    if (clear) SSD_HIP(env, hipMemset(env->p.status, 0, 4));
    return SSD_OK;
}

#ifdef SSD_STAMPS
int ssd_debug_set_skip(ssd_env *env, uint32_t mask) {
    if (!env) return SSD_E_INVALID;
    env->p.dbg_skip = mask;
    return SSD_OK;
}
// Diagnostic library only: a one-wave kernel writes the stamps' 100 MHz clock into a host-visible word `iters` times.
int ssd_debug_clock(ssd_env *env, void *host_word, int iters, void *stream) {
    if (!env || !host_word) return SSD_E_INVALID;
    ssd::launch_clock_kernel(static_cast<unsigned long long *>(host_word), iters, stream);
    return hipGetLastError() == hipSuccess ? SSD_OK : SSD_E_DEVICE;
}
// Diagnostic library only (make stamps): device buffer [E][16] u64 that the kernel fills with cycle stamps.
int ssd_debug_set_stamps(ssd_env *env, void *dev_ptr) {
    if (!env) return SSD_E_INVALID;
    env->p.stamps = static_cast<unsigned long long *>(dev_ptr);
    return SSD_OK;
}
#endif

int ssd_synchronize(ssd_env *env) {
    if (!env) return SSD_E_INVALID;
    SSD_HIP(env, hipSetDevice(env->device));
    SSD_HIP(env, hipDeviceSynchronize());
    return after_timeout(env);      // (SSD_E_DEVICE once if a rollout call's join wait gave up meanwhile: the queues are drained first)
}

}  // extern "C"
