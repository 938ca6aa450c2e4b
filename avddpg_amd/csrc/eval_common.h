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

}  // namespace avd
