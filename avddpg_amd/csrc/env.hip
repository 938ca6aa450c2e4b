// Platoon environment kernels for gfx950: step (K1-K3), reset (K4), OU noise (K5), policy epilogue.
//
// HBM-bound byte work (48 B per vehicle-step + 5 B per platoon): one thread per vehicle, one
// 16-byte load of x per lane, whole platoons per 256-thread block so the predecessor chain and
// the per-platoon any-terminal / mean-reward reductions stay inside LDS.  All arithmetic is
// written without FMA contraction in the reference's operation order so the float32 result is
// bit-identical to the float32 oracle (oracle/platoon.py:batched_step).
#include <float.h>

#include <type_traits>

#include "eval_common.h"

namespace avd {

constexpr int ENV_THREADS = 256;

// Seed keys. G = false: one experiment, the scalar `seed` (the original entry points). G = true: a batch of E experiments whose
// platoons are interleaved -- experiment e's platoon p is global platoon g = p*E + e -- and every draw of platoon g is made with
// (seeds[g % E], the same call counter, the index the solo run of that experiment uses: platoon g / E). The choice is made at
// compile time: the G = false kernels carry no extra branch, load or division.
template <bool G>
__device__ __forceinline__ int seed_key(uint64_t seed, const uint64_t* __restrict__ seeds, int E, int g, uint64_t& key) {
    if constexpr (G) {
        key = seeds[g % E];
        return g / E;
    } else {
        key = seed;
        return g;
    }
}

struct EnvLds {
    float A[AVD_MAX_L][16];
    float B[AVD_MAX_L][4];
    float C[AVD_MAX_L][4];
    float chain[ENV_THREADS];  // Model B: this step's action; Model A: post-step acceleration
    float negr[ENV_THREADS];
    int term[ENV_THREADS];
};

__global__ __launch_bounds__(ENV_THREADS) void env_step_kernel(const avd_env_consts* __restrict__ cst, int P, int L,
                                                               const float4* __restrict__ x_in,
                                                               float4* __restrict__ x_out, float* __restrict__ prev_a,
                                                               float* __restrict__ cum_accel,
                                                               const float* __restrict__ u,
                                                               const float* __restrict__ leader_exog,
                                                               float* __restrict__ reward, uint8_t* __restrict__ term,
                                                               uint8_t* __restrict__ done,
                                                               float* __restrict__ reward_mean,
                                                               int32_t* __restrict__ any_done) {
#pragma clang fp contract(off)
    __shared__ EnvLds lds;
    const int tid = threadIdx.x;
    const int pb = ENV_THREADS / L;  // whole platoons per block
    const int p0 = blockIdx.x * pb;
    // stage the per-vehicle-index matrices once per block
    for (int i = tid; i < L * 16; i += ENV_THREADS) lds.A[i >> 4][i & 15] = cst->A[i >> 4][i & 15];
    for (int i = tid; i < L * 4; i += ENV_THREADS) {
        lds.B[i >> 2][i & 3] = cst->B[i >> 2][i & 3];
        lds.C[i >> 2][i & 3] = cst->C[i >> 2][i & 3];
    }
    const int lp = tid / L;
    const int i = tid - lp * L;
    const int p = p0 + lp;
    const bool active = (lp < pb) && (p < P);
    const long v = (long)p * L + i;
    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
    float pa = 0.f, uu = 0.f;
    if (active) {
        xv = x_in[v];
        pa = prev_a[v];
        uu = u[v];
    }
    __syncthreads();
    const float* Ai = lds.A[i];
    const float* Bi = lds.B[i];
    const float* Ci = lds.C[i];
    // A.dot(x) row by row, left to right (environment.py:513)
    float ax[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ax[r] = ((Ai[r * 4 + 0] * xv.x + Ai[r * 4 + 1] * xv.y) + Ai[r * 4 + 2] * xv.z) + Ai[r * 4 + 3] * xv.w;
    const int model_a = cst->model_a;
    // what the follower behind needs: Model B the action, Model A the post-step accel (C[2] == 0 by construction)
    lds.chain[tid] = model_a ? (ax[2] + Bi[2] * uu) : uu;
    __syncthreads();
    float exog = 0.f;
    if (active) exog = (i == 0) ? leader_exog[p] : lds.chain[tid - 1];
    // reward from the PRE-update state (environment.py:473-476, 505-510)
    const float norm_ep = fabsf(xv.x) / cst->max_ep;
    const float norm_ev = fabsf(xv.y) / cst->max_ev;
    const float norm_u = fabsf(uu) / cst->abs_action_high;
    const float n_jerk = fabsf(xv.z - pa) / cst->two_max_a;
    const bool is_term = ((fabsf(xv.x) > cst->max_ep) || (fabsf(xv.y) > cst->max_ev)) && (cst->can_terminate != 0);
    float rew = (((cst->ca * norm_ep + cst->cb * norm_ev) + cst->cc * norm_u) + cst->cd * n_jerk) * cst->re_scalar;
    if (is_term) rew = cst->terminal_reward * cst->re_scalar;
    const float negr = -rew;
    if (active) {
        float4 xn;
        xn.x = (ax[0] + Bi[0] * uu) + Ci[0] * exog;
        xn.y = (ax[1] + Bi[1] * uu) + Ci[1] * exog;
        xn.z = (ax[2] + Bi[2] * uu) + Ci[2] * exog;
        xn.w = (ax[3] + Bi[3] * uu) + Ci[3] * exog;
        x_out[v] = xn;      // state advances even when terminal (:512-513)
        prev_a[v] = xv.z;   // prev_x <- x
        if (cum_accel) cum_accel[v] = cum_accel[v] + xv.z;  // :500
        reward[v] = negr;
        if (term) term[v] = is_term ? 1 : 0;
    }
    lds.negr[tid] = negr;
    lds.term[tid] = (active && is_term) ? 1 : 0;
    __syncthreads();
    int block_any = 0;
    if (active && i == 0) {
        int any = 0;
        float s = 0.f;
        for (int k = 0; k < L; ++k) {
            any |= lds.term[tid + k];
            s = s + lds.negr[tid + k];
        }
        done[p] = (uint8_t)any;
        if (reward_mean) reward_mean[p] = (1.0f / (float)L) * s;  // environment.py:281
        block_any = any;
    }
    // any-terminal flag (trainer.py:268): one plain store per workgroup at most. Every writer stores the same value,
    // so no atomic is needed (an atomicOr per terminal platoon serialises on one address: 13x slower at P = 2^20).
    if (any_done && __syncthreads_or(block_any) && tid == 0) *any_done = 1;
}

// Fresh state of vehicle (p, i) (Vehicle.reset, environment.py:520-559; Platoon.reset :284-301) -- the draws only; the caller
// chains a_lead = predecessor's fresh x[2] (:291-294). rv: the Philox index of the vehicle (v; in an experiment batch its index in
// the solo run).
__device__ __forceinline__ void reset_draws(const avd_env_consts* cst, int mode, const float* draws, const float* front_accel,
                                            uint64_t seed, uint64_t counter, int p, int i, long v, uint32_t rv, float& d0,
                                            float& d1, float& d2, float& fa) {
#pragma clang fp contract(off)
    if (mode == 1) {  // evaluator constants (environment.py:534-539)
        d0 = cst->reset_ep_eval, d1 = cst->reset_ev_eval, d2 = cst->reset_a_eval;
    } else if (mode == 2) {  // rand_states=False (:552-555)
        d0 = cst->reset_ep_max, d1 = cst->reset_max_ev, d2 = cst->reset_max_a;
    } else if (draws) {  // host-RNG parity mode
        d0 = draws[v * 3 + 0], d1 = draws[v * 3 + 1], d2 = draws[v * 3 + 2];
    } else {  // device Philox (:547-549; util.py:67-70)
        const u32x4 ra = philox_at(seed, counter, rv, STREAM_RESET_A);
        const u32x4 rb = philox_at(seed, counter, rv, STREAM_RESET_B);
        if (cst->uniform_reset) {
            d0 = uniform_pm1(ra.x) * cst->reset_ep_max;
            d1 = uniform_pm1(ra.y) * cst->reset_max_ev;
            d2 = uniform_pm1(rb.x) * cst->reset_max_a;
        } else {
            float n1;
            const float n0 = box_muller(ra.x, ra.y, &n1);
            d0 = n0 * cst->reset_ep_max;
            d1 = n1 * cst->reset_max_ev;
            d2 = box_muller(rb.x, rb.y, nullptr) * cst->reset_max_a;
        }
    }
    if (i == 0) {
        if (front_accel) {
            fa = front_accel[p];
        } else {
            const u32x4 rb = philox_at(seed, counter, rv, STREAM_RESET_B);
            fa = (cst->uniform_reset ? uniform_pm1(rb.z) : box_muller(rb.z, rb.w, nullptr)) * cst->leader_reset_a;
        }
    }
}

template <bool G>
__global__ __launch_bounds__(ENV_THREADS) void env_reset_kernel(const avd_env_consts* __restrict__ cst, int P, int L,
                                                                float4* __restrict__ x, float* __restrict__ prev_a,
                                                                float* __restrict__ cum_accel,
                                                                const float* __restrict__ draws,
                                                                const float* __restrict__ front_accel, int mode,
                                                                uint64_t seed, uint64_t counter,
                                                                const int32_t* __restrict__ cond,
                                                                const uint64_t* __restrict__ seeds, int E) {
#pragma clang fp contract(off)
    __shared__ float x2s[ENV_THREADS];
    if (cond && *cond == 0) return;  // uniform across the grid
    const int tid = threadIdx.x;
    const int pb = ENV_THREADS / L;
    const int lp = tid / L;
    const int i = tid - lp * L;
    const int p = blockIdx.x * pb + lp;
    const bool active = (lp < pb) && (p < P);
    const long v = (long)p * L + i;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f, fa = 0.f;
    if (active) {
        uint64_t key;
        const int pl = seed_key<G>(seed, seeds, E, p, key);
        reset_draws(cst, mode, draws, front_accel, key, counter, p, i, v, G ? (uint32_t)((long)pl * L + i) : (uint32_t)v, d0, d1, d2, fa);
    }
    x2s[tid] = d2;
    __syncthreads();
    if (active) {
        const float a_lead = (i == 0) ? fa : x2s[tid - 1];  // chain: predecessor's fresh x[2] (:291-294)
        x[v] = make_float4(d0, d1, d2, a_lead);
        prev_a[v] = d2;  // prev_x = x (:557)
        if (cum_accel) cum_accel[v] = 0.f;
    }
}

// Per-platoon episode end (vectorised-environment form of workers/trainer.py:232-273; device-RNG throughput mode). The reference
// ends the episode of ALL platoons when any one is terminal (:268-269) -- with thousands of platoons that cuts every episode to
// the first terminal among them. Here each platoon runs its own episode: after a step, a platoon whose step was terminal
// (done[p]) or whose episode has reached `limit` steps (config.py:89) closes its episode -- its M float32 episodic reward
// counters (:249, 321) go into the platoon's statistics (sum over finished episodes of the platoon-mean episodic reward, of the
// episode lengths, and the episode count: what trainer.py:510-517 appends per episode, kept as sums so that nothing leaves the
// device per step), the counters restart from 0 and the platoon gets fresh reset states (Platoon.reset, same draws as
// env_reset_kernel at (seed, counter, vehicle)). *any_reset is set to 1 when any platoon was reset (the caller's "states changed
// under the actor outputs" flag). One thread per vehicle, whole platoons per block.
template <bool G>
__global__ __launch_bounds__(ENV_THREADS) void episode_end_kernel(const avd_env_consts* __restrict__ cst, int P, int L, int M,
                                                                  float4* __restrict__ x, float* __restrict__ prev_a,
                                                                  float* __restrict__ cum_accel,
                                                                  const uint8_t* __restrict__ done, int32_t* __restrict__ ep_len,
                                                                  float* __restrict__ ep_reward, int limit,
                                                                  float* __restrict__ ret_sum, float* __restrict__ len_sum,
                                                                  int32_t* __restrict__ ep_cnt, int32_t* __restrict__ any_reset,
                                                                  int mode, uint64_t seed, uint64_t counter,
                                                                  const uint64_t* __restrict__ seeds, int E) {
#pragma clang fp contract(off)
    __shared__ float x2s[ENV_THREADS];
    __shared__ float rs[ENV_THREADS];
    const int tid = threadIdx.x;
    const int pb = ENV_THREADS / L;
    const int lp = tid / L;
    const int i = tid - lp * L;
    const int p = blockIdx.x * pb + lp;
    const bool active = (lp < pb) && (p < P);
    const long v = (long)p * L + i;
    int len = 0;
    bool end = false;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f, fa = 0.f, er = 0.f;
    if (active) {
        len = ep_len[p] + 1;
        end = (done[p] != 0) || (len >= limit);
        if (end) {
            uint64_t key;
            const int pl = seed_key<G>(seed, seeds, E, p, key);
            reset_draws(cst, mode, nullptr, nullptr, key, counter, p, i, v, G ? (uint32_t)((long)pl * L + i) : (uint32_t)v, d0, d1, d2,
                        fa);
            if (i < M) er = ep_reward[(long)p * M + i];
        }
    }
    x2s[tid] = d2;
    rs[tid] = er;
    const int block_any = __syncthreads_or(end ? 1 : 0);  // also orders the ep_len reads above before the write below
    if (active && end) {
        const float a_lead = (i == 0) ? fa : x2s[tid - 1];
        x[v] = make_float4(d0, d1, d2, a_lead);
        prev_a[v] = d2;
        if (cum_accel) cum_accel[v] = 0.f;
        if (i < M) ep_reward[(long)p * M + i] = 0.f;
    }
    if (active && i == 0) {
        if (end) {
            float s = 0.f;
            for (int k = 0; k < M; ++k) s = s + rs[tid + k];  // vehicle order
            ret_sum[p] = ret_sum[p] + s / (float)M;
            len_sum[p] = len_sum[p] + (float)len;
            ep_cnt[p] = ep_cnt[p] + 1;
            ep_len[p] = 0;
        } else {
            ep_len[p] = len;
        }
    }
    if (any_reset && block_any && tid == 0) *any_reset = 1;  // every writer stores the same value
}

// ---- one launch per training step: OU noise -> policy clip -> leader exog -> platoon step -> replay add (+ reward sums) -----
// workers/trainer.py:282-322 for every platoon at once (device-RNG mode, decentralized agents): what ou_step_kernel,
// policy_kernel, normal_kernel / uniform_kernel, env_step_kernel, replay_add_kernel and the episodic-reward update do as
// seven launches, with the same Philox draws (stream, call counter, index) and the same unfused float arithmetic -- the
// results are bit-identical to the separate kernels (tests/test_gpu_trainer.py). Whole platoons sit inside ONE wavefront
// (64 / L platoons per wave, the remaining lanes idle), so the predecessor chain is a lane shift and the per-platoon
// any-terminal / reward reductions are wavefront operations (ballot, shuffles in vehicle order), not LDS loops.
struct StepArgs {
    const avd_env_consts* cst;
    int P, L, S;
    const float4* x_in;
    float4* x_out;
    float *prev_a, *cum_accel, *reward;
    uint8_t *term, *done;
    int32_t *any_done, *any_done_other;  // this step's flag (zero on entry); the other step parity's flag, zeroed here
    const float* actor_out;              // [P*L] tanh(.) * high
    float *ou_state, *action, *leader_exog;
    float theta, mean, dt, scale, lo, hi, exog_scale;
    int exog_uniform;
    uint64_t seed, ou_counter, exog_counter;
    float* ring;  // [P*L][cap][2S+2] or NULL (no replay add)
    int cap, slot;
    float* ep_reward;  // [P*L] += reward, or NULL
    const uint64_t* seeds;  // experiment batch (step_fused_kernel<true>): E seeds, platoon g draws with seeds[g % E]
    int n_groups;
};

// ---- training under disturbances (avd_step_fused_dist_f32, avd_observe_f32) ---------------------------------------------------
// The disturbed step's trailing argument, in the style of HpRef: without it the kernel is the nominal one, same parameter list,
// same code. Platoon p trains under level (its solo-run index) % n_levels.
struct DistRef {
    int n_levels;
    const avd_train_level* levels;  // [n_levels]
    const float* plant;             // [n_levels][L][24]: A (16), B (4), C (4) per vehicle
    const float4* obs_in;           // what the actors saw of x_in (the replay row's s)
    float4* obs_out;                // the observation of x_out
    float* link_hist;               // [P*L][16] V2V ring, or NULL with link_recv: no level uses the link
    float* link_recv;               // [P*L] last received value
    uint64_t obs_counter;           // Philox call counter of obs_out
};
template <class... H>
constexpr bool has_dist = (std::is_same<H, DistRef>::value || ...);

// ---- training under leader manoeuvres (avd_step_fused_lead_f32 and its twins) ------------------------------------------------------
// Another trailing argument of the same kind, alone or after a DistRef. Platoon p trains under manoeuvre (its solo-run index /
// n_levels) % n: levels and manoeuvres cross. A deterministic manoeuvre's leader input is its row of the host-made table at the step of
// the platoon's own episode (ep_len[p], or the host's ep_step when ep_len is null; clamped into the row) plus noise * the step's unit
// draw; a gaussian one is the nominal input, the unit draw times its noise.
struct LeadRef {
    int n, T;
    const float* table;          // [n][T], rows of gaussian manoeuvres unread
    const float* noise;          // [n]
    const uint8_t* is_gaussian;  // [n]
    const int32_t* ep_len;       // [P] or NULL
    int ep_step, n_levels;
};
template <class... H>
constexpr bool has_lead = (std::is_same<H, LeadRef>::value || ...);
// the pack's member of type T
template <class T, class First, class... Rest>
__device__ __forceinline__ const T& pack_member(const First& f, const Rest&... r) {
    if constexpr (std::is_same<T, First>::value) return f;
    else return pack_member<T>(r...);
}
template <class... H>
__device__ __forceinline__ const DistRef& dist_of(const H&... h) { return pack_member<DistRef>(h...); }
template <class... H>
__device__ __forceinline__ const LeadRef& lead_of(const H&... h) { return pack_member<LeadRef>(h...); }

// ---- training a residual on a linear law (avd_step_fused_res_f32) --------------------------------------------------------------
// A third trailing argument, the last of the pack, after a DistRef and / or a LeadRef or alone. Seen from the agent the law is part of the
// environment: the plant, the reward's norm_u and the value chained to the follower take u = residual_law(gains row of the vehicle, what
// the agent observes of the pre-step state, scale, the agent's action); action[], the replay row and the learners keep the agent's action.
struct BaseRef {
    const float* gains;  // [L][4]: (kp, kv, ka, kf) per vehicle
    float scale;         // the residual's authority, in (0, 1]
    float* applied;      // [P*L] u, or NULL
};
template <class... H>
constexpr bool has_base = (std::is_same<H, BaseRef>::value || ...);
template <class... H>
__device__ __forceinline__ const BaseRef& base_of(const H&... h) { return pack_member<BaseRef>(h...); }
constexpr int LINK_RING = 16;  // slots of a vehicle's V2V history (delays 0 .. 15), indexed by counter & 15
constexpr int LEVEL_WORDS = sizeof(avd_train_level) / 4;
static_assert(sizeof(avd_train_level) == 32 && (LINK_RING & (LINK_RING - 1)) == 0, "level rows of 8 words; the ring index is a mask");

__device__ __forceinline__ bool level_uses_link(const avd_train_level& lv) { return lv.delay != 0 || lv.drop_q != 0u; }
inline bool level_uses_link_host(const avd_train_level& lv) { return lv.delay != 0 || lv.drop_q != 0u; }

// HP (avd_step_fused_hp_f32, with G): platoon g's ou_theta / ou_scale from the sweep table, row g % n_groups (its experiment)
// DIST (avd_step_fused_dist_f32, one DistRef in the pack): the platoon's level picks its plant, obs_out observes x_out, the replay row
// holds observations. The plant rows of ALL levels and the level table are staged in dynamic LDS once per block ([n_levels][L][24]
// floats, then [n_levels][8] words: at most 25 088 B) in place of the constants block's L rows.
// LEAD (avd_step_fused_lead_f32, one LeadRef in the pack, with or without a DistRef): the leader's input comes from the platoon's
// manoeuvre. Only the leader's lane reads the table, one float from global memory (16 x T floats would cost more to stage per block).
// BASE (avd_step_fused_res_f32, one BaseRef last in the pack): the plant takes u, the law's output plus scale * the agent's action uu.
// Each lane reads its vehicle's gain row as one 16-byte load (L rows, the same for every platoon: cache hits after the first wave).
template <bool G, bool HP = false, class... H>
__global__ __launch_bounds__(ENV_THREADS) void step_fused_kernel(const StepArgs a, H... hp) {
#pragma clang fp contract(off)
    constexpr bool DIST = has_dist<H...>, LEAD = has_lead<H...>, BASE = has_base<H...>;
    __shared__ float sA[AVD_MAX_L][16], sB[AVD_MAX_L][4], sC[AVD_MAX_L][4];  // (DIST: unused, the rows live in dynamic LDS)
    const avd_env_consts* cst = a.cst;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, L = a.L;
    const float* sPlant = nullptr;      // DIST: [n_levels][L][24]
    const uint32_t* sLevels = nullptr;  // DIST: [n_levels][LEVEL_WORDS]
    if constexpr (DIST) {
        extern __shared__ __attribute__((aligned(16))) float dist_lds[];
        const DistRef& d = dist_of(hp...);
        const int np = d.n_levels * L * 24, nl = d.n_levels * LEVEL_WORDS;
        for (int k = tid; k < np; k += ENV_THREADS) dist_lds[k] = d.plant[k];
        for (int k = tid; k < nl; k += ENV_THREADS) dist_lds[np + k] = __uint_as_float(((const uint32_t*)d.levels)[k]);
        sPlant = dist_lds, sLevels = (const uint32_t*)(dist_lds + np);
    } else {
        for (int i = tid; i < L * 16; i += ENV_THREADS) sA[i >> 4][i & 15] = cst->A[i >> 4][i & 15];
        for (int i = tid; i < L * 4; i += ENV_THREADS) sB[i >> 2][i & 3] = cst->B[i >> 2][i & 3], sC[i >> 2][i & 3] = cst->C[i >> 2][i & 3];
    }
    if (blockIdx.x == 0 && tid == 0 && a.any_done_other) *a.any_done_other = 0;
    const int pw = 64 / L;                      // whole platoons per wave
    const int lp = lane / L, i = lane - lp * L;  // platoon of the wave, vehicle
    const int p = (blockIdx.x * (ENV_THREADS / 64) + wv) * pw + lp;
    const bool active = (lp < pw) && (p < a.P);
    const long v = (long)p * L + i;
    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
    float pa = 0.f, uu = 0.f, exog_own = 0.f;
    float ub = 0.f;                                   // BASE: what the plant receives (otherwise uu itself)
    float4 seen = make_float4(0.f, 0.f, 0.f, 0.f);  // BASE with DIST: what the agent observed of x_in (the replay row's s)
    uint64_t okey = 0;  // DIST: the observation's Philox key, vehicle index and level (idle lanes: level 0, nothing stored)
    uint32_t orv = 0;
    int lvl = 0;
    if (active) {
        xv = a.x_in[v];
        pa = a.prev_a[v];
        // OUActionNoise.__call__ (src/noise.py:15-19) and policy (agent/ddpgagent.py:22-27)
        uint64_t key;
        const int pl = seed_key<G>(a.seed, a.seeds, a.n_groups, p, key);  // (the solo run's platoon index)
        if constexpr (DIST) okey = key, orv = G ? (uint32_t)((long)pl * L + i) : (uint32_t)v, lvl = pl % dist_of(hp...).n_levels;
        const u32x4 rn = philox_at(key, a.ou_counter, G ? (uint32_t)((long)pl * L + i) : (uint32_t)v, STREAM_OU);
        const float nrm = box_muller(rn.x, rn.y, nullptr);
        const float st = a.ou_state[v];
        float theta = a.theta, scale = a.scale;
        if constexpr (HP) {
            const avd_hparams& h = hp_of(p, hp...);  // (block 1: row p % n_groups)
            theta = h.ou_theta, scale = h.ou_scale;
        }
        const float noise = (st + (theta * (a.mean - st)) * a.dt) + scale * nrm;
        a.ou_state[v] = noise;
        uu = fminf(fmaxf(a.actor_out[v] + noise, a.lo), a.hi);
        a.action[v] = uu;
        if constexpr (BASE) {
            const BaseRef& b = base_of(hp...);
            float4 ob = xv;
            if constexpr (DIST) ob = seen = dist_of(hp...).obs_in[v];
            ub = residual_law(((const float4*)b.gains)[i], ob, cst->model_a != 0, b.scale, uu, a.lo, a.hi);
            if (b.applied) b.applied[v] = ub;
        }
        if (i == 0) {  // leader exog, redrawn every step (workers/trainer.py:291-295; util.get_random_val)
            const u32x4 re = philox_at(key, a.exog_counter, (uint32_t)pl, STREAM_NORMAL);
            if constexpr (LEAD) {
                const LeadRef& ld = lead_of(hp...);
                const int m = (pl / ld.n_levels) % ld.n;
                const float d = a.exog_uniform ? uniform_pm1(re.x) : box_muller(re.x, re.y, nullptr), nz = ld.noise[m];
                if (ld.is_gaussian[m]) {
                    exog_own = d * nz;
                } else {  // the table's bits, or one rounded product and one add on top of them
                    const int k = min(max(ld.ep_len ? ld.ep_len[p] : ld.ep_step, 0), ld.T - 1);
                    exog_own = ld.table[m * ld.T + k];
                    if (nz != 0.f) exog_own = exog_own + nz * d;
                }
            } else {
                exog_own = (a.exog_uniform ? uniform_pm1(re.x) : box_muller(re.x, re.y, nullptr)) * a.exog_scale;
            }
            a.leader_exog[p] = exog_own;
        }
    }
    __syncthreads();
    const float* Ai = DIST ? sPlant + (lvl * L + i) * 24 : sA[i];
    const float* Bi = DIST ? Ai + 16 : sB[i];
    const float* Ci = DIST ? Ai + 20 : sC[i];
    float ax[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ax[r] = ((Ai[r * 4 + 0] * xv.x + Ai[r * 4 + 1] * xv.y) + Ai[r * 4 + 2] * xv.z) + Ai[r * 4 + 3] * xv.w;
    // what the follower behind needs: Model B the action, Model A the post-step accel -- one lane up
    const float u = BASE ? ub : uu;  // the plant's input
    const float chain = cst->model_a ? (ax[2] + Bi[2] * u) : u;
    const float from_pred = __shfl_up(chain, 1);
    const float exog = (i == 0) ? exog_own : from_pred;
    const float norm_ep = fabsf(xv.x) / cst->max_ep;
    const float norm_ev = fabsf(xv.y) / cst->max_ev;
    const float norm_u = fabsf(u) / cst->abs_action_high;
    const float n_jerk = fabsf(xv.z - pa) / cst->two_max_a;
    const bool is_term = active && ((fabsf(xv.x) > cst->max_ep) || (fabsf(xv.y) > cst->max_ev)) && (cst->can_terminate != 0);
    float rew = (((cst->ca * norm_ep + cst->cb * norm_ev) + cst->cc * norm_u) + cst->cd * n_jerk) * cst->re_scalar;
    if (is_term) rew = cst->terminal_reward * cst->re_scalar;
    const float negr = -rew;
    const unsigned long long tmask = __ballot(is_term);
    if (active) {
        float4 xn;
        xn.x = (ax[0] + Bi[0] * u) + Ci[0] * exog;
        xn.y = (ax[1] + Bi[1] * u) + Ci[1] * exog;
        xn.z = (ax[2] + Bi[2] * u) + Ci[2] * exog;
        xn.w = (ax[3] + Bi[3] * u) + Ci[3] * exog;
        a.x_out[v] = xn;
        a.prev_a[v] = xv.z;
        if (a.cum_accel) a.cum_accel[v] = a.cum_accel[v] + xv.z;
        a.reward[v] = negr;
        if (a.term) a.term[v] = is_term ? 1 : 0;
        if (a.ep_reward) a.ep_reward[v] = a.ep_reward[v] + negr;  // float32 counters (workers/trainer.py:249, 321)
        if (i == 0) a.done[p] = (uint8_t)(((tmask >> (lp * L)) & ((1ull << L) - 1ull)) != 0ull);
        float4 row_s = xv, row_n = xn;  // the replay row's states: the true ones, or (DIST) what the agent saw of them
        if constexpr (DIST) {
            const DistRef& d = dist_of(hp...);
            avd_train_level lv;
            lv.sigma[0] = __uint_as_float(sLevels[lvl * LEVEL_WORDS]), lv.sigma[1] = __uint_as_float(sLevels[lvl * LEVEL_WORDS + 1]);
            lv.sigma[2] = __uint_as_float(sLevels[lvl * LEVEL_WORDS + 2]);
            lv.delay = (int32_t)sLevels[lvl * LEVEL_WORDS + 3], lv.drop_q = sLevels[lvl * LEVEL_WORDS + 4];
            float4 ob = xn;
            if (d.link_hist && level_uses_link(lv)) {  // this vehicle's ring and held value: its own thread's alone
                float* hist = d.link_hist + v * LINK_RING;
                const int c = (int)(uint32_t)d.obs_counter;
                hist[c & (LINK_RING - 1)] = xn.w;
                // (the host refuses delays outside the ring; the mask keeps any value inside it)
                const float delayed = hist[(c - lv.delay) & (LINK_RING - 1)];
                // loss: an integer compare on one Philox word (drop_q = 0 never drops: no draw needed)
                const bool dropped = lv.drop_q != 0u && (philox_at(okey, d.obs_counter, orv, STREAM_TRAIN_LINK).x >> 8) < lv.drop_q;
                if (dropped) ob.w = d.link_recv[v];
                else d.link_recv[v] = ob.w = delayed;
            }
            observe_noise(ob, xn, lv.sigma[0], lv.sigma[1], lv.sigma[2], okey, d.obs_counter, orv, STREAM_TRAIN_OBS);  // the evaluator's model
            d.obs_out[v] = ob;
            row_n = ob;
            if constexpr (BASE) row_s = seen;
            else if (a.ring) row_s = d.obs_in[v];
        }
        if (a.ring) {  // ReplayBuffer.add (src/replaybuffer.py:36-47): row [s a r s'] at slot counter % capacity
            const int S = a.S, row = 2 * S + 2;
            float* dst = a.ring + ((long)v * a.cap + a.slot) * row;
            const float xo[4] = {row_s.x, row_s.y, row_s.z, row_s.w}, xw[4] = {row_n.x, row_n.y, row_n.z, row_n.w};
            if (S == 4) {  // 40-byte rows, 8-byte aligned
                ((float2*)dst)[0] = make_float2(xo[0], xo[1]);
                ((float2*)dst)[1] = make_float2(xo[2], xo[3]);
                ((float2*)dst)[2] = make_float2(uu, negr);
                ((float2*)dst)[3] = make_float2(xw[0], xw[1]);
                ((float2*)dst)[4] = make_float2(xw[2], xw[3]);
            } else {
                for (int k = 0; k < S; ++k) dst[k] = xo[k], dst[S + 2 + k] = xw[k];
                dst[S] = uu, dst[S + 1] = negr;
            }
        }
    }
    // any-terminal flag (trainer.py:268): one plain store per workgroup at most, every writer stores the same value
    if (a.any_done && __syncthreads_or(tmask != 0ull) && tid == 0) *a.any_done = 1;
}

// (Re)observe fresh states (after a reset): obs = the observation of x with the sensor noise of (key, counter, vehicle) and a FRESH
// link -- ring filled with x.w, held value x.w, observed x.w (the start value, as the evaluator's ring before its first step). One
// thread per vehicle. only_where_zero [P] / run_if_nonzero (one flag): nullable gates, see include/avddpg_hip.h.
template <bool G>
__global__ __launch_bounds__(ENV_THREADS) void observe_kernel(int P, int L, const float4* __restrict__ x, float4* __restrict__ obs,
                                                              int n_levels, const avd_train_level* __restrict__ levels,
                                                              float* __restrict__ link_hist, float* __restrict__ link_recv,
                                                              uint64_t seed, uint64_t counter,
                                                              const int32_t* __restrict__ only_where_zero,
                                                              const int32_t* __restrict__ run_if_nonzero,
                                                              const uint64_t* __restrict__ seeds, int E) {
    if (run_if_nonzero && *run_if_nonzero == 0) return;  // uniform across the grid
    const long v = (long)blockIdx.x * ENV_THREADS + threadIdx.x;
    if (v >= (long)P * L) return;
    const int p = (int)(v / L), i = (int)(v - (long)p * L);
    if (only_where_zero && only_where_zero[p] != 0) return;
    uint64_t key;
    const int pl = seed_key<G>(seed, seeds, E, p, key);
    const avd_train_level lv = levels[pl % n_levels];
    const float4 xv = x[v];
    float4 ob = xv;
    observe_noise(ob, xv, lv.sigma[0], lv.sigma[1], lv.sigma[2], key, counter, G ? (uint32_t)((long)pl * L + i) : (uint32_t)v, STREAM_TRAIN_OBS);
    obs[v] = ob;
    if (link_hist) {
        const float4 w4 = make_float4(xv.w, xv.w, xv.w, xv.w);
        float4* hist = (float4*)(link_hist + v * LINK_RING);
#pragma unroll
        for (int k = 0; k < LINK_RING / 4; ++k) hist[k] = w4;
        link_recv[v] = xv.w;
    }
}

__global__ void ou_step_kernel(int n, float* __restrict__ st, const float* __restrict__ normals, float theta,
                               float mean, float dt, float scale, uint64_t seed, uint64_t counter) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float nrm;
    if (normals) {
        nrm = normals[i];
    } else {
        const u32x4 r = philox_at(seed, counter, (uint32_t)i, STREAM_OU);
        nrm = box_muller(r.x, r.y, nullptr);
    }
    const float x = st[i];
    st[i] = (x + (theta * (mean - x)) * dt) + scale * nrm;  // noise.py:15-19
}

__global__ void policy_kernel(int n, const float* __restrict__ actor_out, const float* __restrict__ noise, float lo,
                              float hi, float* __restrict__ action) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a = actor_out[i];
    if (noise) a = a + noise[i];
    action[i] = fminf(fmaxf(a, lo), hi);  // np.clip (ddpgagent.py:27)
}

__global__ void normal_kernel(int n, float* __restrict__ out, float std_dev, uint64_t seed, uint64_t counter) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32x4 r = philox_at(seed, counter, (uint32_t)i, STREAM_NORMAL);
    out[i] = box_muller(r.x, r.y, nullptr) * std_dev;
}

__global__ void uniform_kernel(int n, float* __restrict__ out, float half_width, uint64_t seed, uint64_t counter) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32x4 r = philox_at(seed, counter, (uint32_t)i, STREAM_NORMAL);  // same stream slot as normal_kernel: one or the other
    out[i] = uniform_pm1(r.x) * half_width;
}

}  // namespace avd

using namespace avd;

// Kernel templates are instantiated, and so laid out in the code object, in the order of their first use. The shared launch paths
// below (one per twin pair, one for the fused step's seventeen packs) would change that order; this list keeps the one the file has
// always had, so that the device code of two trees can be compared as text (tools/isa_diff.py). The step's packs: the scalar seed's
// eight, the seed table's eight, the sweep's last.
#define AVD_STEP_PACKS(G)                                                                                                               \
    (const void*)step_fused_kernel<G, false, DistRef, LeadRef, BaseRef>, (const void*)step_fused_kernel<G, false, LeadRef, BaseRef>,  \
    (const void*)step_fused_kernel<G, false, DistRef, BaseRef>, (const void*)step_fused_kernel<G, false, BaseRef>,                    \
    (const void*)step_fused_kernel<G, false, DistRef, LeadRef>, (const void*)step_fused_kernel<G, false, LeadRef>,                    \
    (const void*)step_fused_kernel<G, false, DistRef>, (const void*)step_fused_kernel<G>
[[maybe_unused]] static const void* const env_kernel_order[] = {
    (const void*)env_reset_kernel<false>, (const void*)episode_end_kernel<false>,
    AVD_STEP_PACKS(false), AVD_STEP_PACKS(true), (const void*)step_fused_kernel<true, true, HpRef>,
    (const void*)env_reset_kernel<true>, (const void*)episode_end_kernel<true>,
    (const void*)observe_kernel<false>, (const void*)observe_kernel<true>};
#undef AVD_STEP_PACKS

// ---- experiment batches: the draw kernels keyed by a device seed table (G = true) ----------------------------------------
// P is the batch's platoon count (n_groups experiments x P / n_groups platoons each, interleaved: g = p*n_groups + e).
#define AVD_REQUIRE_GROUPS(who, P)                                                                                            \
    AVD_REQUIRE(d_seeds && n_groups >= 1 && (P) > 0 && (P) % n_groups == 0, "%s: d_seeds=%p n_groups=%d P=%d (P must be a " \
                "multiple of n_groups)", who, (const void*)d_seeds, n_groups, (int)(P))

extern "C" int avd_env_step_f32(const avd_env_consts* d_consts, int P, int L, const float* x_in, float* x_out,
                                float* prev_a, float* cum_accel, const float* u, const float* leader_exog,
                                float* reward, uint8_t* term, uint8_t* done, float* reward_mean, int32_t* any_done,
                                void* stream) {
    AVD_REQUIRE(P > 0 && L > 0 && L <= AVD_MAX_L, "avd_env_step_f32: P=%d L=%d (L must be 1..%d)", P, L, AVD_MAX_L);
    AVD_REQUIRE(d_consts && x_in && x_out && prev_a && u && leader_exog && reward && done,
                "avd_env_step_f32: null pointer");
    const int pb = ENV_THREADS / L;
    const int grid = (P + pb - 1) / pb;
    hipLaunchKernelGGL(env_step_kernel, dim3(grid), dim3(ENV_THREADS), 0, (hipStream_t)stream, d_consts, P, L,
                       (const float4*)x_in, (float4*)x_out, prev_a, cum_accel, u, leader_exog, reward, term, done,
                       reward_mean, any_done);
    return check_launch("avd_env_step_f32");
}

// The reset entry points. G: the seed table's twin (its group check after the others; seed unread); otherwise d_seeds is null
template <bool G>
static int env_reset_impl(const char* who, const avd_env_consts* d_consts, int P, int L, float* x, float* prev_a, float* cum_accel,
                          const float* draws, const float* front_accel, int mode, uint64_t seed, const uint64_t* d_seeds, int n_groups,
                          uint64_t counter, const int32_t* cond, void* stream) {
    AVD_REQUIRE(P > 0 && L > 0 && L <= AVD_MAX_L, "%s: P=%d L=%d", who, P, L);
    AVD_REQUIRE(d_consts && x && prev_a, "%s: null pointer", who);
    AVD_REQUIRE(mode >= 0 && mode <= 2, "%s: mode %d", who, mode);
    if constexpr (G) AVD_REQUIRE_GROUPS(who, P);
    const int pb = ENV_THREADS / L;
    hipLaunchKernelGGL(env_reset_kernel<G>, dim3((P + pb - 1) / pb), dim3(ENV_THREADS), 0, (hipStream_t)stream, d_consts, P, L,
                       (float4*)x, prev_a, cum_accel, draws, front_accel, mode, seed, counter, cond, d_seeds, n_groups);
    return check_launch(who);
}

extern "C" int avd_env_reset_f32(const avd_env_consts* d_consts, int P, int L, float* x, float* prev_a,
                                 float* cum_accel, const float* draws, const float* front_accel, int mode,
                                 uint64_t seed, uint64_t counter, const int32_t* cond, void* stream) {
    return env_reset_impl<false>("avd_env_reset_f32", d_consts, P, L, x, prev_a, cum_accel, draws, front_accel, mode, seed, nullptr, 1,
                                 counter, cond, stream);
}

extern "C" int avd_env_reset_seeds_f32(const avd_env_consts* d_consts, int P, int L, float* x, float* prev_a, float* cum_accel,
                                       int mode, const uint64_t* d_seeds, int n_groups, uint64_t counter, const int32_t* cond,
                                       void* stream) {
    return env_reset_impl<true>("avd_env_reset_seeds_f32", d_consts, P, L, x, prev_a, cum_accel, nullptr, nullptr, mode, 0, d_seeds,
                                n_groups, counter, cond, stream);
}

// The episode-end entry points, in the same way
template <bool G>
static int episode_end_impl(const char* who, const avd_env_consts* d_consts, int P, int L, int M, float* x, float* prev_a,
                            float* cum_accel, const uint8_t* done, int32_t* ep_len, float* ep_reward, int limit, float* ret_sum,
                            float* len_sum, int32_t* ep_cnt, int32_t* any_reset, int mode, uint64_t seed, const uint64_t* d_seeds,
                            int n_groups, uint64_t counter, void* stream) {
    AVD_REQUIRE(P > 0 && L > 0 && L <= AVD_MAX_L && M >= 1 && M <= L, "%s: P=%d L=%d M=%d", who, P, L, M);
    AVD_REQUIRE(d_consts && x && prev_a && done && ep_len && ep_reward && ret_sum && len_sum && ep_cnt, "%s: null pointer", who);
    AVD_REQUIRE(limit >= 1 && mode >= 0 && mode <= 2, "%s: limit=%d mode=%d", who, limit, mode);
    if constexpr (G) AVD_REQUIRE_GROUPS(who, P);
    const int pb = ENV_THREADS / L;
    hipLaunchKernelGGL(episode_end_kernel<G>, dim3((P + pb - 1) / pb), dim3(ENV_THREADS), 0, (hipStream_t)stream, d_consts, P, L, M,
                       (float4*)x, prev_a, cum_accel, done, ep_len, ep_reward, limit, ret_sum, len_sum, ep_cnt, any_reset, mode, seed,
                       counter, d_seeds, n_groups);
    return check_launch(who);
}

extern "C" int avd_episode_end_f32(const avd_env_consts* d_consts, int P, int L, int M, float* x, float* prev_a, float* cum_accel,
                                   const uint8_t* done, int32_t* ep_len, float* ep_reward, int limit, float* ret_sum,
                                   float* len_sum, int32_t* ep_cnt, int32_t* any_reset, int mode, uint64_t seed,
                                   uint64_t counter, void* stream) {
    return episode_end_impl<false>("avd_episode_end_f32", d_consts, P, L, M, x, prev_a, cum_accel, done, ep_len, ep_reward, limit, ret_sum,
                                   len_sum, ep_cnt, any_reset, mode, seed, nullptr, 1, counter, stream);
}

extern "C" int avd_episode_end_seeds_f32(const avd_env_consts* d_consts, int P, int L, int M, float* x, float* prev_a,
                                         float* cum_accel, const uint8_t* done, int32_t* ep_len, float* ep_reward, int limit,
                                         float* ret_sum, float* len_sum, int32_t* ep_cnt, int32_t* any_reset, int mode,
                                         const uint64_t* d_seeds, int n_groups, uint64_t counter, void* stream) {
    return episode_end_impl<true>("avd_episode_end_seeds_f32", d_consts, P, L, M, x, prev_a, cum_accel, done, ep_len, ep_reward, limit,
                                  ret_sum, len_sum, ep_cnt, any_reset, mode, 0, d_seeds, n_groups, counter, stream);
}

extern "C" int avd_ou_step_f32(int n, float* ou_state, const float* normals, float theta, float mean, float dt,
                               float std_dev, uint64_t seed, uint64_t counter, void* stream) {
    AVD_REQUIRE(n > 0 && ou_state, "avd_ou_step_f32: n=%d", n);
    const float scale = std_dev * (float)sqrt((double)dt);  // float32(std_dev) * float32(sqrt(dt)), as the f32 oracle
    hipLaunchKernelGGL(ou_step_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, ou_state, normals,
                       theta, mean, dt, scale, seed, counter);
    return check_launch("avd_ou_step_f32");
}

extern "C" int avd_policy_f32(int n, const float* actor_out, const float* noise, float lo, float hi, float* action,
                              void* stream) {
    AVD_REQUIRE(n > 0 && actor_out && action, "avd_policy_f32: n=%d", n);
    hipLaunchKernelGGL(policy_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, actor_out, noise,
                       lo, hi, action);
    return check_launch("avd_policy_f32");
}

extern "C" int avd_normal_f32(int n, float* out, float std_dev, uint64_t seed, uint64_t counter, void* stream) {
    AVD_REQUIRE(n > 0 && out, "avd_normal_f32: n=%d", n);
    hipLaunchKernelGGL(normal_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, out, std_dev, seed,
                       counter);
    return check_launch("avd_normal_f32");
}

extern "C" int avd_uniform_f32(int n, float* out, float half_width, uint64_t seed, uint64_t counter, void* stream) {
    AVD_REQUIRE(n > 0 && out, "avd_uniform_f32: n=%d", n);
    hipLaunchKernelGGL(uniform_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, out, half_width, seed,
                       counter);
    return check_launch("avd_uniform_f32");
}

// ---- the fused step's host side ------------------------------------------------------------------------
// What an entry point of the fused step asks for. Every avd_step_fused_* wrapper makes one (AVD_STEP_CALL), gives it its seed key and
// its variant's parts after checking them, and hands it to step_fused_run: the one place with the step's own checks and the launch.
struct StepCall {
    StepArgs a;  // the common block as the kernel takes it. The seed key: a.seed, or a.seeds + a.n_groups. a.slot: step_fused_run's
    int64_t replay_counter;
    const avd_hparams* hp;  // the sweep's table (with a seed table), or null
    const DistRef* dist;    // the parts of the kernel's pack, each null where the entry point has none
    const LeadRef* lead;
    const BaseRef* base;
    hipStream_t stream;
    const char* who;  // the entry point, for messages
};

// StepCall c of the wrapper it stands in, from the parameter names that all ten signatures share; the key is the scalar seed 0 until
// the wrapper sets its own. theta_, std_dev_: ou_theta and ou_std_dev, or the sweep's zeros (per platoon there: its kernel reads neither).
#define AVD_STEP_CALL(c, who_, theta_, std_dev_)                                                                                       \
    StepCall c = {};                                                                                                                     \
    c.who = who_, c.stream = (hipStream_t)stream, c.replay_counter = replay_counter, c.a.cst = d_consts, c.a.P = P, c.a.L = L, c.a.S = S; \
    c.a.x_in = (const float4*)x_in, c.a.x_out = (float4*)x_out, c.a.prev_a = prev_a, c.a.cum_accel = cum_accel, c.a.reward = reward;     \
    c.a.term = term, c.a.done = done, c.a.any_done = any_done, c.a.any_done_other = any_done_other, c.a.actor_out = actor_out;           \
    c.a.ou_state = ou_state, c.a.action = action, c.a.leader_exog = leader_exog, c.a.theta = theta_, c.a.mean = ou_mean, c.a.dt = ou_dt; \
    c.a.scale = std_dev_ * (float)sqrt((double)ou_dt); /* as avd_ou_step_f32 */                                                          \
    c.a.lo = action_low, c.a.hi = action_high, c.a.exog_scale = exog_scale, c.a.exog_uniform = exog_uniform, c.a.n_groups = 1;           \
    c.a.ou_counter = ou_counter, c.a.exog_counter = exog_counter, c.a.ring = ring, c.a.cap = cap, c.a.ep_reward = ep_reward

// The step's own checks, then one launch of step_fused_kernel<G, HP, the parts present...>: G from the seed table, the pack in the
// kernel's order (DistRef, LeadRef, BaseRef), or the sweep's lone HpRef
static int step_fused_run(const StepCall& c) {
    StepArgs a = c.a;
    const char* who = c.who;
    AVD_REQUIRE(a.P > 0 && a.L > 0 && a.L <= AVD_MAX_L && (a.S == 3 || a.S == 4), "%s: P=%d L=%d S=%d", who, a.P, a.L, a.S);
    AVD_REQUIRE(a.cst && a.x_in && a.x_out && a.prev_a && a.reward && a.done && a.actor_out && a.ou_state && a.action && a.leader_exog,
                "%s: null pointer", who);
    AVD_REQUIRE(!a.ring || (a.cap > 0 && c.replay_counter >= 0), "%s: cap=%d counter=%ld", who, a.cap, (long)c.replay_counter);
    a.slot = a.ring ? (int)(c.replay_counter % a.cap) : 0;
    const int per_block = (ENV_THREADS / 64) * (64 / a.L);
    const dim3 grid((a.P + per_block - 1) / per_block);
    const size_t lds = c.dist ? sizeof(float) * (size_t)c.dist->n_levels * (a.L * 24 + LEVEL_WORDS) : 0;  // the levels' plant rows and table
    const std::false_type no{};
    const auto go = [&](auto g, auto hp, const auto&... r) {
        hipLaunchKernelGGL((step_fused_kernel<decltype(g)::value, decltype(hp)::value, std::decay_t<decltype(r)>...>), grid, dim3(ENV_THREADS),
                           lds, c.stream, a, r...);
    };
    const auto with_base = [&](auto g, const auto&... r) { c.base ? go(g, no, r..., *c.base) : go(g, no, r...); };
    const auto with_lead = [&](auto g, const auto&... r) { c.lead ? with_base(g, r..., *c.lead) : with_base(g, r...); };
    const auto with_dist = [&](auto g) { c.dist ? with_lead(g, *c.dist) : with_lead(g); };
    if (c.hp) go(std::true_type{}, std::true_type{}, HpRef{c.hp, a.n_groups, 1});  // (avd_step_fused_hp_f32 has required the seed table)
    else if (a.seeds) with_dist(std::true_type{});
    else with_dist(no);
    return check_launch(who);
}

// The disturbed step's own arguments, checked (the level table's HOST copy row by row) and packed
static int dist_args(const char* who, int n_levels, const avd_train_level* h_levels, const avd_train_level* d_levels, const float* d_plant,
                     const float* obs_in, float* obs_out, float* link_hist, float* link_recv, uint64_t obs_counter, DistRef& d) {
    AVD_REQUIRE(n_levels >= 1 && n_levels <= AVD_TRAIN_MAX_LEVELS, "%s: n_levels=%d (must be 1..%d)", who, n_levels, AVD_TRAIN_MAX_LEVELS);
    AVD_REQUIRE(h_levels && d_levels && d_plant && obs_in && obs_out, "%s: null level table, plant table or observation buffer", who);
    AVD_REQUIRE((link_hist == nullptr) == (link_recv == nullptr), "%s: link_hist and link_recv must both be given or both be null", who);
    for (int k = 0; k < n_levels; ++k) {
        const avd_train_level& lv = h_levels[k];
        for (int c = 0; c < 3; ++c)
            AVD_REQUIRE(lv.sigma[c] >= 0.f && lv.sigma[c] <= FLT_MAX, "%s: level %d sigma[%d]=%g (must be finite and >= 0)", who, k, c,
                        (double)lv.sigma[c]);
        AVD_REQUIRE(lv.delay >= 0 && lv.delay <= LINK_RING - 1, "%s: level %d delay=%d (must be 0..%d)", who, k, lv.delay, LINK_RING - 1);
        AVD_REQUIRE(lv.drop_q <= (1u << 24), "%s: level %d drop_q=%u (must be <= 2^24 = %u)", who, k, lv.drop_q, 1u << 24);
        AVD_REQUIRE(link_hist || !level_uses_link_host(lv), "%s: level %d uses the V2V link (delay=%d drop_q=%u) but link_hist is null", who, k,
                    lv.delay, lv.drop_q);
    }
    d.n_levels = n_levels, d.levels = d_levels, d.plant = d_plant, d.obs_in = (const float4*)obs_in, d.obs_out = (float4*)obs_out;
    d.link_hist = link_hist, d.link_recv = link_recv, d.obs_counter = obs_counter;
    return AVD_OK;
}

// The manoeuvre step's own arguments, checked and packed (the tables are device memory: their values are the caller's to check)
static int lead_args(const char* who, int n_manoeuvres, int T, const float* d_table, const float* d_noise, const uint8_t* d_gaussian,
                     const int32_t* ep_len, int ep_step, int n_levels, LeadRef& l) {
    AVD_REQUIRE(n_manoeuvres >= 1 && n_manoeuvres <= AVD_TRAIN_MAX_MANOEUVRES, "%s: n_manoeuvres=%d (must be 1..%d)", who, n_manoeuvres,
                AVD_TRAIN_MAX_MANOEUVRES);
    AVD_REQUIRE(T >= 4, "%s: T=%d (a manoeuvre needs at least 4 steps)", who, T);
    AVD_REQUIRE(d_table && d_noise && d_gaussian, "%s: null manoeuvre table, noise table or gaussian flags", who);
    AVD_REQUIRE(ep_len || (ep_step >= 0 && ep_step < T), "%s: ep_step=%d with a null ep_len (must be in [0, T=%d))", who, ep_step, T);
    AVD_REQUIRE(n_levels >= 1, "%s: n_levels=%d (must be >= 1)", who, n_levels);
    l.n = n_manoeuvres, l.T = T, l.table = d_table, l.noise = d_noise, l.is_gaussian = d_gaussian, l.ep_len = ep_len;
    l.ep_step = ep_step, l.n_levels = n_levels;
    return AVD_OK;
}

extern "C" int avd_step_fused_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out,
                                  float* prev_a, float* cum_accel, float* reward, uint8_t* term, uint8_t* done,
                                  int32_t* any_done, int32_t* any_done_other, const float* actor_out, float* ou_state,
                                  float* action, float* leader_exog, float ou_theta, float ou_mean, float ou_dt, float ou_std_dev,
                                  float action_low, float action_high, float exog_scale, int exog_uniform, uint64_t seed,
                                  uint64_t ou_counter, uint64_t exog_counter, float* ring, int cap, int64_t replay_counter,
                                  float* ep_reward, void* stream) {
    AVD_STEP_CALL(c, "avd_step_fused_f32", ou_theta, ou_std_dev);
    c.a.seed = seed;
    return step_fused_run(c);
}

extern "C" int avd_step_fused_seeds_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out,
                                        float* prev_a, float* cum_accel, float* reward, uint8_t* term, uint8_t* done,
                                        int32_t* any_done, int32_t* any_done_other, const float* actor_out, float* ou_state,
                                        float* action, float* leader_exog, float ou_theta, float ou_mean, float ou_dt,
                                        float ou_std_dev, float action_low, float action_high, float exog_scale, int exog_uniform,
                                        const uint64_t* d_seeds, int n_groups, uint64_t ou_counter, uint64_t exog_counter,
                                        float* ring, int cap, int64_t replay_counter, float* ep_reward, void* stream) {
    const char* who = "avd_step_fused_seeds_f32";
    AVD_REQUIRE_GROUPS(who, P);
    AVD_STEP_CALL(c, who, ou_theta, ou_std_dev);
    c.a.seeds = d_seeds, c.a.n_groups = n_groups;
    return step_fused_run(c);
}

extern "C" int avd_step_fused_hp_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out,
                                     float* prev_a, float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done,
                                     int32_t* any_done_other, const float* actor_out, float* ou_state, float* action, float* leader_exog,
                                     float ou_mean, float ou_dt, float action_low, float action_high, float exog_scale, int exog_uniform,
                                     const uint64_t* d_seeds, const avd_hparams* d_hp, int n_groups, uint64_t ou_counter,
                                     uint64_t exog_counter, float* ring, int cap, int64_t replay_counter, float* ep_reward, void* stream) {
    const char* who = "avd_step_fused_hp_f32";
    AVD_REQUIRE_GROUPS(who, P);
    AVD_REQUIRE_HP(who, d_hp, n_groups, 1, P);
    // (the scalar theta / scale the kernel would read are replaced per platoon; zeros here keep them out of the arithmetic)
    AVD_STEP_CALL(c, who, 0.f, 0.f);
    c.a.seeds = d_seeds, c.a.n_groups = n_groups, c.hp = d_hp;
    return step_fused_run(c);
}

// ---- training under disturbances --------------------------------------------------------------------------------------------
extern "C" int avd_step_fused_dist_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out,
                                       float* prev_a, float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done,
                                       int32_t* any_done_other, const float* actor_out, float* ou_state, float* action,
                                       float* leader_exog, float ou_theta, float ou_mean, float ou_dt, float ou_std_dev, float action_low,
                                       float action_high, float exog_scale, int exog_uniform, uint64_t seed, uint64_t ou_counter,
                                       uint64_t exog_counter, float* ring, int cap, int64_t replay_counter, float* ep_reward,
                                       int n_levels, const avd_train_level* h_levels, const avd_train_level* d_levels,
                                       const float* d_plant, const float* obs_in, float* obs_out, float* link_hist, float* link_recv,
                                       uint64_t obs_counter, void* stream) {
    const char* who = "avd_step_fused_dist_f32";
    DistRef d;
    if (const int rc = dist_args(who, n_levels, h_levels, d_levels, d_plant, obs_in, obs_out, link_hist, link_recv, obs_counter, d)) return rc;
    AVD_STEP_CALL(c, who, ou_theta, ou_std_dev);
    c.a.seed = seed, c.dist = &d;
    return step_fused_run(c);
}

extern "C" int avd_step_fused_dist_seeds_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out,
                                             float* prev_a, float* cum_accel, float* reward, uint8_t* term, uint8_t* done,
                                             int32_t* any_done, int32_t* any_done_other, const float* actor_out, float* ou_state,
                                             float* action, float* leader_exog, float ou_theta, float ou_mean, float ou_dt,
                                             float ou_std_dev, float action_low, float action_high, float exog_scale, int exog_uniform,
                                             const uint64_t* d_seeds, int n_groups, uint64_t ou_counter, uint64_t exog_counter,
                                             float* ring, int cap, int64_t replay_counter, float* ep_reward, int n_levels,
                                             const avd_train_level* h_levels, const avd_train_level* d_levels, const float* d_plant,
                                             const float* obs_in, float* obs_out, float* link_hist, float* link_recv,
                                             uint64_t obs_counter, void* stream) {
    const char* who = "avd_step_fused_dist_seeds_f32";
    AVD_REQUIRE_GROUPS(who, P);
    DistRef d;
    if (const int rc = dist_args(who, n_levels, h_levels, d_levels, d_plant, obs_in, obs_out, link_hist, link_recv, obs_counter, d)) return rc;
    AVD_STEP_CALL(c, who, ou_theta, ou_std_dev);
    c.a.seeds = d_seeds, c.a.n_groups = n_groups, c.dist = &d;
    return step_fused_run(c);
}

// ---- training under leader manoeuvres --------------------------------------------------------------------------------------
extern "C" int avd_step_fused_lead_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out,
    float* prev_a, float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done, int32_t* any_done_other,
    const float* actor_out, float* ou_state, float* action, float* leader_exog, float ou_theta, float ou_mean, float ou_dt,
    float ou_std_dev, float action_low, float action_high, float exog_scale, int exog_uniform, uint64_t seed, uint64_t ou_counter,
    uint64_t exog_counter, float* ring, int cap, int64_t replay_counter, float* ep_reward, int n_manoeuvres, int T, const float* d_table,
    const float* d_noise, const uint8_t* d_gaussian, const int32_t* ep_len, int ep_step, int n_levels, void* stream) {
    const char* who = "avd_step_fused_lead_f32";
    LeadRef l;
    if (const int rc = lead_args(who, n_manoeuvres, T, d_table, d_noise, d_gaussian, ep_len, ep_step, n_levels, l)) return rc;
    AVD_STEP_CALL(c, who, ou_theta, ou_std_dev);
    c.a.seed = seed, c.lead = &l;
    return step_fused_run(c);
}

extern "C" int avd_step_fused_lead_seeds_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out,
    float* prev_a, float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done, int32_t* any_done_other,
    const float* actor_out, float* ou_state, float* action, float* leader_exog, float ou_theta, float ou_mean, float ou_dt,
    float ou_std_dev, float action_low, float action_high, float exog_scale, int exog_uniform, const uint64_t* d_seeds, int n_groups, uint64_t ou_counter,
    uint64_t exog_counter, float* ring, int cap, int64_t replay_counter, float* ep_reward, int n_manoeuvres, int T, const float* d_table,
    const float* d_noise, const uint8_t* d_gaussian, const int32_t* ep_len, int ep_step, int n_levels, void* stream) {
    const char* who = "avd_step_fused_lead_seeds_f32";
    AVD_REQUIRE_GROUPS(who, P);
    LeadRef l;
    if (const int rc = lead_args(who, n_manoeuvres, T, d_table, d_noise, d_gaussian, ep_len, ep_step, n_levels, l)) return rc;
    AVD_STEP_CALL(c, who, ou_theta, ou_std_dev);
    c.a.seeds = d_seeds, c.a.n_groups = n_groups, c.lead = &l;
    return step_fused_run(c);
}

extern "C" int avd_step_fused_dist_lead_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out,
    float* prev_a, float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done, int32_t* any_done_other,
    const float* actor_out, float* ou_state, float* action, float* leader_exog, float ou_theta, float ou_mean, float ou_dt,
    float ou_std_dev, float action_low, float action_high, float exog_scale, int exog_uniform, uint64_t seed, uint64_t ou_counter,
    uint64_t exog_counter, float* ring, int cap, int64_t replay_counter, float* ep_reward, int n_levels, const avd_train_level* h_levels,
    const avd_train_level* d_levels, const float* d_plant, const float* obs_in, float* obs_out, float* link_hist, float* link_recv,
    uint64_t obs_counter, int n_manoeuvres, int T, const float* d_table,
    const float* d_noise, const uint8_t* d_gaussian, const int32_t* ep_len, int ep_step, void* stream) {
    const char* who = "avd_step_fused_dist_lead_f32";
    DistRef d;
    if (const int rc = dist_args(who, n_levels, h_levels, d_levels, d_plant, obs_in, obs_out, link_hist, link_recv, obs_counter, d)) return rc;
    LeadRef l;
    if (const int rc = lead_args(who, n_manoeuvres, T, d_table, d_noise, d_gaussian, ep_len, ep_step, n_levels, l)) return rc;
    AVD_STEP_CALL(c, who, ou_theta, ou_std_dev);
    c.a.seed = seed, c.dist = &d, c.lead = &l;
    return step_fused_run(c);
}

extern "C" int avd_step_fused_dist_lead_seeds_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out,
    float* prev_a, float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done, int32_t* any_done_other,
    const float* actor_out, float* ou_state, float* action, float* leader_exog, float ou_theta, float ou_mean, float ou_dt,
    float ou_std_dev, float action_low, float action_high, float exog_scale, int exog_uniform, const uint64_t* d_seeds, int n_groups, uint64_t ou_counter,
    uint64_t exog_counter, float* ring, int cap, int64_t replay_counter, float* ep_reward, int n_levels, const avd_train_level* h_levels,
    const avd_train_level* d_levels, const float* d_plant, const float* obs_in, float* obs_out, float* link_hist, float* link_recv,
    uint64_t obs_counter, int n_manoeuvres, int T, const float* d_table,
    const float* d_noise, const uint8_t* d_gaussian, const int32_t* ep_len, int ep_step, void* stream) {
    const char* who = "avd_step_fused_dist_lead_seeds_f32";
    AVD_REQUIRE_GROUPS(who, P);
    DistRef d;
    if (const int rc = dist_args(who, n_levels, h_levels, d_levels, d_plant, obs_in, obs_out, link_hist, link_recv, obs_counter, d)) return rc;
    LeadRef l;
    if (const int rc = lead_args(who, n_manoeuvres, T, d_table, d_noise, d_gaussian, ep_len, ep_step, n_levels, l)) return rc;
    AVD_STEP_CALL(c, who, ou_theta, ou_std_dev);
    c.a.seeds = d_seeds, c.a.n_groups = n_groups, c.dist = &d, c.lead = &l;
    return step_fused_run(c);
}

// ---- training a residual on a linear law: ONE entry point for the nominal, seed-batch, disturbed and manoeuvre forms ------------------
extern "C" int avd_step_fused_res_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out,
    float* prev_a, float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done, int32_t* any_done_other,
    const float* actor_out, float* ou_state, float* action, float* leader_exog, float ou_theta, float ou_mean, float ou_dt,
    float ou_std_dev, float action_low, float action_high, float exog_scale, int exog_uniform, uint64_t seed, uint64_t ou_counter,
    uint64_t exog_counter, float* ring, int cap, int64_t replay_counter, float* ep_reward, const uint64_t* d_seeds, int n_groups,
    int n_levels, const avd_train_level* h_levels, const avd_train_level* d_levels, const float* d_plant, const float* obs_in,
    float* obs_out, float* link_hist, float* link_recv, uint64_t obs_counter, int n_manoeuvres, int T, const float* d_table,
    const float* d_noise, const uint8_t* d_gaussian, const int32_t* ep_len, int ep_step, const float* d_gains, float scale,
    float* applied, void* stream) {
    const char* who = "avd_step_fused_res_f32";
    if (const int rc = residual_check(who, d_gains, scale, L, L)) return rc;  // (the fused step is decentralized by construction)
    AVD_REQUIRE(n_levels >= 0 && n_manoeuvres >= 0, "%s: n_levels=%d n_manoeuvres=%d (0: none)", who, n_levels, n_manoeuvres);
    AVD_REQUIRE(!obs_in || ((uintptr_t)obs_in & 15) == 0, "%s: obs_in=%p (must be 16-byte aligned)", who, (const void*)obs_in);
    DistRef d;
    LeadRef l;
    if (n_levels > 0)
        if (const int rc = dist_args(who, n_levels, h_levels, d_levels, d_plant, obs_in, obs_out, link_hist, link_recv, obs_counter, d)) return rc;
    if (n_manoeuvres > 0)
        if (const int rc = lead_args(who, n_manoeuvres, T, d_table, d_noise, d_gaussian, ep_len, ep_step, n_levels > 0 ? n_levels : 1, l)) return rc;
    const BaseRef b = {d_gains, scale, applied};
    if (d_seeds) AVD_REQUIRE_GROUPS(who, P);
    AVD_STEP_CALL(c, who, ou_theta, ou_std_dev);
    if (d_seeds) c.a.seeds = d_seeds, c.a.n_groups = n_groups;  // (seed unread)
    else c.a.seed = seed;
    c.dist = n_levels > 0 ? &d : nullptr, c.lead = n_manoeuvres > 0 ? &l : nullptr, c.base = &b;
    return step_fused_run(c);
}

// The observation entry points: the checks once, the seed table's twin with its group check after them
template <bool G>
static int observe_impl(const char* who, int P, int L, const float* x, float* obs, int n_levels, const avd_train_level* d_levels,
                        float* link_hist, float* link_recv, uint64_t seed, const uint64_t* d_seeds, int n_groups, uint64_t obs_counter,
                        const int32_t* only_where_zero, const int32_t* run_if_nonzero, void* stream) {
    AVD_REQUIRE(P > 0 && L > 0 && L <= AVD_MAX_L, "%s: P=%d L=%d (L must be 1..%d)", who, P, L, AVD_MAX_L);
    AVD_REQUIRE(n_levels >= 1 && n_levels <= AVD_TRAIN_MAX_LEVELS, "%s: n_levels=%d (must be 1..%d)", who, n_levels, AVD_TRAIN_MAX_LEVELS);
    AVD_REQUIRE(x && obs && d_levels, "%s: null pointer", who);
    AVD_REQUIRE((link_hist == nullptr) == (link_recv == nullptr), "%s: link_hist and link_recv must both be given or both be null", who);
    if constexpr (G) AVD_REQUIRE_GROUPS(who, P);
    const long n = (long)P * L;
    hipLaunchKernelGGL(observe_kernel<G>, dim3((unsigned)((n + ENV_THREADS - 1) / ENV_THREADS)), dim3(ENV_THREADS), 0, (hipStream_t)stream, P,
                       L, (const float4*)x, (float4*)obs, n_levels, d_levels, link_hist, link_recv, seed, obs_counter, only_where_zero,
                       run_if_nonzero, d_seeds, n_groups);
    return check_launch(who);
}

extern "C" int avd_observe_f32(int P, int L, const float* x, float* obs, int n_levels, const avd_train_level* d_levels, float* link_hist,
                               float* link_recv, uint64_t seed, uint64_t obs_counter, const int32_t* only_where_zero,
                               const int32_t* run_if_nonzero, void* stream) {
    return observe_impl<false>("avd_observe_f32", P, L, x, obs, n_levels, d_levels, link_hist, link_recv, seed, nullptr, 1, obs_counter,
                               only_where_zero, run_if_nonzero, stream);
}

extern "C" int avd_observe_seeds_f32(int P, int L, const float* x, float* obs, int n_levels, const avd_train_level* d_levels,
                                     float* link_hist, float* link_recv, const uint64_t* d_seeds, int n_groups, uint64_t obs_counter,
                                     const int32_t* only_where_zero, const int32_t* run_if_nonzero, void* stream) {
    return observe_impl<true>("avd_observe_seeds_f32", P, L, x, obs, n_levels, d_levels, link_hist, link_recv, 0, d_seeds, n_groups,
                              obs_counter, only_where_zero, run_if_nonzero, stream);
}
