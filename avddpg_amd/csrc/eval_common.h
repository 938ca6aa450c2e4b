// What the rollout kernels share, so that each steps, observes and scores a vehicle with the same text: the platoon step (eval.hip: one
// rollout per workgroup; evalx.hip: a block of cases per workgroup; lin.hip: one lane per vehicle), the linear and the residual law
// (those three and env.hip's fused step), the sensor noise (evalx.hip, lin.hip, env.hip), and the scenario evaluators' V2V link, metrics
// and per-case disturbance tables (evalx.hip, lin.hip).
#pragma once
#include "learn_common.h"

namespace avd {

// One vehicle's platoon step (env_step_kernel, env.hip: same expressions, same order, no contraction). The caller
// exchanges `chain` through LDS between the two halves: vehicle i's exogenous input is its predecessor's chain value.
struct VehStep {
    float ax[4];
    float chain;  // Model B: this step's action; Model A: post-step acceleration (C[2] == 0 by construction)
};

__device__ __forceinline__ VehStep veh_step_pre(const avd_env_consts* cst, const float* Ai, const float* Bi, float4 xv, float uu) {
#pragma clang fp contract(off)
    VehStep s;
#pragma unroll
    for (int r = 0; r < 4; ++r) s.ax[r] = ((Ai[r * 4 + 0] * xv.x + Ai[r * 4 + 1] * xv.y) + Ai[r * 4 + 2] * xv.z) + Ai[r * 4 + 3] * xv.w;
    s.chain = cst->model_a ? (s.ax[2] + Bi[2] * uu) : uu;
    return s;
}

// The terminal test of the PRE-update state (environment.py:505-506)
__device__ __forceinline__ bool veh_terminal(const avd_env_consts* cst, float4 xv) {
    return ((fabsf(xv.x) > cst->max_ep) || (fabsf(xv.y) > cst->max_ev)) && (cst->can_terminate != 0);
}

// -reward from the PRE-update state (environment.py:473-476, 505-510) and the post-step state (:512-513)
__device__ __forceinline__ float veh_step_post(const avd_env_consts* cst, const VehStep& s, const float* Bi, const float* Ci,
                                               float4 xv, float pa, float uu, float exog, float4& xn) {
#pragma clang fp contract(off)
    const float norm_ep = fabsf(xv.x) / cst->max_ep;
    const float norm_ev = fabsf(xv.y) / cst->max_ev;
    const float norm_u = fabsf(uu) / cst->abs_action_high;
    const float n_jerk = fabsf(xv.z - pa) / cst->two_max_a;
    const bool is_term = veh_terminal(cst, xv);
    float rew = (((cst->ca * norm_ep + cst->cb * norm_ev) + cst->cc * norm_u) + cst->cd * n_jerk) * cst->re_scalar;
    if (is_term) rew = cst->terminal_reward * cst->re_scalar;
    xn.x = (s.ax[0] + Bi[0] * uu) + Ci[0] * exog;
    xn.y = (s.ax[1] + Bi[1] * uu) + Ci[1] * exog;
    xn.z = (s.ax[2] + Bi[2] * uu) + Ci[2] * exog;
    xn.w = (s.ax[3] + Bi[3] * uu) + Ci[3] * exog;  // the state advances even on a terminal step; the evaluator does not stop
    return -rew;
}

// The linear CACC law on what a vehicle observes, before the clip: gn = (kp, kv, ka, kf); the feed-forward term is skipped under Model A
__device__ __forceinline__ float linear_law(float4 gn, float4 ob, bool model_a) {
#pragma clang fp contract(off)
    float z = (gn.x * ob.x + gn.y * ob.y) + gn.z * ob.z;
    if (!model_a) z = z + gn.w * ob.w;
    return z;
}

// The residual policy's plant input (avd_step_fused_res_f32, avd_eval_rollout_res_f32, avd_eval_cases_res_f32): the linear law on what
// the agent observes, plus scale * the agent's action r, clipped. Zero gains and scale 1 give clip(r).
__device__ __forceinline__ float residual_law(float4 gn, float4 ob, bool model_a, float scale, float r, float lo, float hi) {
#pragma clang fp contract(off)
    return fminf(fmaxf(linear_law(gn, ob, model_a) + scale * r, lo), hi);  // np.clip
}

// Sensor noise on the first three components of x: one Philox block of (key, counter, rv) on `stream` per vehicle, unfused multiply and
// add; a zero sigma skips its add and keeps the bits of x: exact by construction.
__device__ __forceinline__ void observe_noise(float4& ob, const float4& x, float sg_ep, float sg_ev, float sg_a, uint64_t key,
                                              uint64_t counter, uint32_t rv, uint32_t stream) {
#pragma clang fp contract(off)
    if (sg_ep != 0.f || sg_ev != 0.f || sg_a != 0.f) {
        const u32x4 r = philox_at(key, counter, rv, stream);
        float n_ev;
        const float n_ep = box_muller(r.x, r.y, &n_ev);
        const float n_a = box_muller(r.z, r.w, nullptr);
        if (sg_ep != 0.f) ob.x = x.x + sg_ep * n_ep;
        if (sg_ev != 0.f) ob.y = x.y + sg_ev * n_ev;
        if (sg_a != 0.f) ob.z = x.z + sg_a * n_a;
    }
}

// ---- the scenario evaluators (evalx.hip, lin.hip) ----------------------------------------------------------------------------------
// The disturbed variants' per-case tables (device memory, [K] each; evaluator.py forms them)
struct DistArgs {
    const float* sigma;          // [K][3] sensor-noise standard deviations of ep, ev, a (finite, >= 0)
    const int32_t* delay;        // [K] V2V delay in steps, 0 .. AVD_EVAL_MAX_DELAY
    const uint32_t* drop_q;      // [K] V2V loss: a sample is dropped iff (word >> 8) < drop_q, drop_q = round(p * 2^24)
    const uint64_t* noise_seed;  // [K] Philox key of the case's draws
    const float* abc;            // [K][L][24] the true plant's A (16), B (4), C (4) per vehicle, or null: the constants block's
};

constexpr int EVAL_RING = AVD_EVAL_MAX_DELAY + 1;  // slots of a vehicle's V2V history
static_assert((EVAL_RING & (EVAL_RING - 1)) == 0, "the ring index is taken with a mask");

// One step of a vehicle's V2V link: w, the communicated 4th state of step t, enters the ring (slot j at ring[j * STRIDE]; the vehicle's
// own thread's alone), the value of dly steps ago arrives unless it is lost, and what the vehicle holds -- `held`, an LDS word or a
// register -- is updated and returned. dly is 0 .. EVAL_RING - 1; a slot of a step < 0 has not been overwritten yet and holds x0's.
template <int STRIDE>
__device__ __forceinline__ float v2v_link(float* ring, float& held, float w, int t, int dly, uint32_t dq, uint64_t key, uint32_t v) {
    ring[(t & (EVAL_RING - 1)) * STRIDE] = w;
    const float delayed = ring[((t - dly) & (EVAL_RING - 1)) * STRIDE];
    // loss: an integer compare on one Philox word (drop_q = 0 never drops: no draw needed)
    const bool dropped = dq != 0 && (philox_at(key, (uint64_t)t, v, STREAM_EVAL_LINK).x >> 8) < dq;
    if (!dropped) held = delayed;
    return held;
}

// A vehicle's control metrics (scenarios.metrics_from_traces: sequential float32 sums in step order, no contraction)
struct VehMetrics {
    // (declared last metric first: in this order eval_linear_kernel<> compiles to the instructions it had with seven local floats; in
    // metric order its loop is scheduled differently and measures 1 to 4 % slower)
    float first = -1.0f, nterm = 0.f, sj2 = 0.f, su2 = 0.f, mx_a = 0.f, mx_ev = 0.f, mx_ep = 0.f;

    // step t took xv (previous acceleration pa) to xn under the plant input uu
    __device__ __forceinline__ void step(const avd_env_consts* cst, float4 xv, float4 xn, float pa, float uu, float inv_dt, int t) {
#pragma clang fp contract(off)
        if (veh_terminal(cst, xv)) {
            nterm = nterm + 1.0f;
            if (first < 0.f) first = (float)t;
        }
        const float jerk = (xv.z - pa) * inv_dt;
        su2 = su2 + uu * uu;
        sj2 = sj2 + jerk * jerk;
        mx_ep = fmaxf(mx_ep, fabsf(xn.x)), mx_ev = fmaxf(mx_ev, fabsf(xn.y)), mx_a = fmaxf(mx_a, fabsf(xn.z));
    }
    // o: the vehicle's AVD_EVAL_NMETRIC floats; xv: its final state
    __device__ __forceinline__ void store(float* o, float4 xv) const {
        o[0] = mx_ep, o[1] = mx_ev, o[2] = mx_a, o[3] = su2, o[4] = sj2, o[5] = nterm, o[6] = first, o[7] = fabsf(xv.x);
    }
};

// The evaluator kernels' trailing argument of a frequency sweep (avd_eval_cases_freq_f32, avd_eval_linear_freq_f32): per case and step
// the pair (c, s) every signal is multiplied with, and where the vehicles' sums go. The window is the table's: a (0, 0) pair adds 0.
struct FreqArgs {
    const float* basis;  // [K][T][2], 8-byte aligned
    float* spectrum;     // [G][K][L][AVD_EVAL_NSPEC]
};

// A vehicle's single-bin Fourier sums (scenarios.spectrum_from_traces: sequential float32 adds in step order, the product rounded
// first): (re, im) of the post-step ep, ev, a, w and of the step's plant input u, in that order
struct VehSpectrum {
    float s[AVD_EVAL_NSPEC] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    __device__ __forceinline__ void step(float4 xn, float uu, float2 cs) {
#pragma clang fp contract(off)
        const float x[5] = {xn.x, xn.y, xn.z, xn.w, uu};
#pragma unroll
        for (int i = 0; i < 5; ++i) s[2 * i] = s[2 * i] + x[i] * cs.x, s[2 * i + 1] = s[2 * i + 1] + x[i] * cs.y;
    }
    // o: the vehicle's AVD_EVAL_NSPEC floats, `stride` apart: the raw sums (the host scales them)
    __device__ __forceinline__ void store(float* o, int stride = 1) const {
#pragma unroll
        for (int i = 0; i < AVD_EVAL_NSPEC; ++i) o[i * stride] = s[i];
    }
    __device__ __forceinline__ void load(const float* o, int stride) {
#pragma unroll
        for (int i = 0; i < AVD_EVAL_NSPEC; ++i) s[i] = o[i * stride];
    }
    // The sums kept in LDS between steps, slot i of a thread at o[i * stride] (the thread's own words: no barrier), where ten more
    // live registers across the step would cost a wave per SIMD
    static __device__ __forceinline__ void step_lds(float* o, int stride, float4 xn, float uu, float2 cs) {
        VehSpectrum sp;
        sp.load(o, stride);
        sp.step(xn, uu, cs);
        sp.store(o, stride);
    }
};

// The frequency entry points' own arguments, checked: both tables non-null, the basis pairs 8-byte aligned (read as float2)
inline int freq_check(const char* who, const FreqArgs& f) {
    AVD_REQUIRE(f.basis && ((uintptr_t)f.basis & 7) == 0, "%s: basis=%p (must be a non-null, 8-byte aligned [K][T][2] table)", who,
                (const void*)f.basis);
    AVD_REQUIRE(f.spectrum, "%s: null spectrum", who);
    return AVD_OK;
}

// The evaluator kernels' trailing argument of a residual policy: the law's gain rows and the residual's authority
struct ResArgs {
    const float* gains;  // [L][4]: (kp, kv, ka, kf) per vehicle
    float scale;         // in (0, 1]
};
template <class T, class... H>
constexpr bool pack_has = (std::is_same<H, T>::value || ...);
template <class T, class First, class... Rest>
__device__ __forceinline__ const T& pack_get(const First& f, const Rest&... r) {
    if constexpr (std::is_same<T, First>::value) return f;
    else return pack_get<T>(r...);
}

// The residual entry points' own arguments, checked: 16-byte aligned gain rows, scale in (0, 1], decentralized agents
inline int residual_check(const char* who, const float* gains, float scale, int M, int L) {
    AVD_REQUIRE(gains && ((uintptr_t)gains & 15) == 0, "%s: gains=%p (must be a non-null, 16-byte aligned [L][4] table)", who, (const void*)gains);
    AVD_REQUIRE(scale > 0.f && scale <= 1.f, "%s: scale=%g (must be in (0, 1])", who, (double)scale);
    if (M != L) {
        set_error("%s: M=%d L=%d (a residual on a per-vehicle law needs decentralized agents, M == L)", who, M, L);
        return AVD_E_UNSUPPORTED;
    }
    return AVD_OK;
}

}  // namespace avd
