// The platoon step of the evaluator kernels (eval.hip: one rollout per workgroup; evalx.hip: a block of cases per workgroup), shared
// so that both step a vehicle with the same text.
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

// -reward from the PRE-update state (environment.py:473-476, 505-510) and the post-step state (:512-513)
__device__ __forceinline__ float veh_step_post(const avd_env_consts* cst, const VehStep& s, const float* Bi, const float* Ci,
                                               float4 xv, float pa, float uu, float exog, float4& xn) {
#pragma clang fp contract(off)
    const float norm_ep = fabsf(xv.x) / cst->max_ep;
    const float norm_ev = fabsf(xv.y) / cst->max_ev;
    const float norm_u = fabsf(uu) / cst->abs_action_high;
    const float n_jerk = fabsf(xv.z - pa) / cst->two_max_a;
    const bool is_term = ((fabsf(xv.x) > cst->max_ep) || (fabsf(xv.y) > cst->max_ev)) && (cst->can_terminate != 0);
    float rew = (((cst->ca * norm_ep + cst->cb * norm_ev) + cst->cc * norm_u) + cst->cd * n_jerk) * cst->re_scalar;
    if (is_term) rew = cst->terminal_reward * cst->re_scalar;
    xn.x = (s.ax[0] + Bi[0] * uu) + Ci[0] * exog;
    xn.y = (s.ax[1] + Bi[1] * uu) + Ci[1] * exog;
    xn.z = (s.ax[2] + Bi[2] * uu) + Ci[2] * exog;
    xn.w = (s.ax[3] + Bi[3] * uu) + Ci[3] * exog;  // the state advances even on a terminal step; the evaluator does not stop
    return -rew;
}

// The residual policy's plant input (avd_step_fused_res_f32, avd_eval_rollout_res_f32, avd_eval_cases_res_f32): the linear law of
// eval_linear_kernel (lin.hip: the same two lines, the feed-forward term skipped under Model A) on what the agent observes, plus
// scale * the agent's action r, clipped. Zero gains and scale 1 give clip(r).
__device__ __forceinline__ float residual_law(float4 gn, float4 ob, bool model_a, float scale, float r, float lo, float hi) {
#pragma clang fp contract(off)
    float z = (gn.x * ob.x + gn.y * ob.y) + gn.z * ob.z;
    if (!model_a) z = z + gn.w * ob.w;
    return fminf(fmaxf(z + scale * r, lo), hi);  // np.clip
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
