// The update rule, once: TF 2.4.1's ApplyAdam element step followed by the Polyak target update on the fresh weight, and the
// bias-corrected step sizes of iteration t. Every update kernel (optim.hip), every fused-update epilogue (AdamSink, learn_common.h)
// and the learn kernels that set those epilogues up (mlp.hip, lean.hip) go through these functions: the result is promised
// bit for bit against the float32 oracle (oracle/mlp.py:adam_update), so the rounding contract lives in one place.
#pragma once
#include <hip/hip_runtime.h>

namespace avd {

constexpr float ADAM_B1 = 0.9f, ADAM_B2 = 0.999f, ADAM_EPS = 1e-7f;

// lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t); beta^t as float32(pow) like the oracle / TF (math_ops.pow on float32 scalars).
// In two steps for lean.hip, whose sweep form reads its step sizes from the table after the powers and moves each quotient to a
// scalar register as it is formed; everything else takes both at once (adam_alphas).
struct AdamBias {
    float root, b1p;  // sqrt(1 - b2^t), b1^t
    __device__ __forceinline__ float alpha(float lr) const { return (lr * root) / (1.0f - b1p); }
};
__device__ __forceinline__ AdamBias adam_bias(int t) {
    const float b1p = (float)pow((double)ADAM_B1, (double)t), b2p = (float)pow((double)ADAM_B2, (double)t);
    return {sqrtf(1.0f - b2p), b1p};
}
// the step sizes of the actor and of the critic block at iteration t
struct AdamAlphas {
    float a, c;
};
__device__ __forceinline__ AdamAlphas adam_alphas(float actor_lr, float critic_lr, int t) {
    const AdamBias b = adam_bias(t);
    return {b.alpha(actor_lr), b.alpha(critic_lr)};
}

// One element: (pre-update weight, target, moments, gradient) -> (updated weight, target, moments). No FMA contraction, exact
// division and square root (approximate rcp / sqrt measured no faster: the callers are bound by memory throughput). The pragma
// has to sit HERE: one in a caller's body does not reach the statements of an inlined callee.
struct AdamElem {
    float w, wt, m, v;
};
// The Adam half alone: (pre-update weight, moments, gradient) -> (updated weight, moments); wt is not touched. What a skipped call of
// the delayed update (optim.hip: adam_polyak_delayed_kernel<false>) applies to the critic block, whose target follows only on policy
// calls -- and the first three statements of every other update: adam_polyak_step below goes through it.
__device__ __forceinline__ AdamElem adam_step(float w_in, float wt, float m, float v, float g, float alpha) {
#pragma clang fp contract(off)
    AdamElem o;
    o.m = m + (g - m) * (1.0f - ADAM_B1);
    o.v = v + (g * g - v) * (1.0f - ADAM_B2);
    o.w = w_in - (o.m * alpha) / (sqrtf(o.v) + ADAM_EPS);
    o.wt = wt;
    return o;
}
__device__ __forceinline__ AdamElem adam_polyak_step(float w_in, float wt, float m, float v, float g, float alpha, float tau,
                                                     float omt) {
#pragma clang fp contract(off)
    AdamElem o = adam_step(w_in, wt, m, v, g, alpha);
    o.wt = o.w * tau + wt * omt;  // update_target on the freshly updated weight
    return o;
}

}  // namespace avd
