// Warm start (DESIGN.md "Actor clone"): the batch of one fit step -- states drawn uniformly in a box, and the linear law's clipped
// action on each as the target -- in one launch, for avd_actor_clone_f32 (mlp.hip). The law is eval_common.h's linear_law: the text
// and the rounding order of lin.hip's controller.
#include "eval_common.h"

namespace avd {

constexpr int CLONE_THREADS = 256;

// One thread per (set j, row b). The draw is keyed by (experiment's key, fit step, vehicle index m, row b): it knows neither the
// platoon count nor the experiment's place in a seed batch, so experiment e of a batch draws what its solo run draws.
__global__ __launch_bounds__(CLONE_THREADS) void clone_sample_kernel(int n_sets, int S, int M, const float* __restrict__ gains,
                                                                     const float* __restrict__ box, float lo, float hi, int model_a,
                                                                     uint64_t seed, uint64_t counter,
                                                                     const uint64_t* __restrict__ seeds, int E, float* __restrict__ s,
                                                                     float* __restrict__ u) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * CLONE_THREADS + threadIdx.x;
    if (idx >= (long)n_sets * TILE) return;
    const int j = (int)(idx / TILE), b = (int)(idx - (long)j * TILE);
    const int m = j % M, e = (j / M) % E;
    const uint64_t key = seeds ? seeds[e] : seed;
    const u32x4 w = philox_at(key, counter, (uint32_t)(m * TILE + b), STREAM_CLONE);
    float4 ob;
    ob.x = uniform_pm1(w.x) * box[0];
    ob.y = uniform_pm1(w.y) * box[1];
    ob.z = uniform_pm1(w.z) * box[2];
    ob.w = (S > 3) ? uniform_pm1(w.w) * box[3] : 0.f;
    float* row = s + idx * S;
    row[0] = ob.x, row[1] = ob.y, row[2] = ob.z;
    if (S > 3) row[3] = ob.w;
    const float4 gn = *(const float4*)(gains + (long)m * 4);
    u[idx] = fminf(fmaxf(linear_law(gn, ob, model_a != 0), lo), hi);  // np.clip
}

}  // namespace avd

using namespace avd;

extern "C" int avd_clone_sample_f32(int n_sets, int S, int M, const float* d_gains, const float* d_box, float lo, float hi, int model_a,
                                    uint64_t seed, uint64_t counter, const uint64_t* d_seeds, int E, float* s, float* u_target,
                                    void* stream) {
    const char* who = "avd_clone_sample_f32";
    AVD_REQUIRE(S == 3 || S == 4, "%s: S=%d (3 or 4)", who, S);
    AVD_REQUIRE(M >= 1 && E >= 1 && n_sets > 0 && n_sets % (M * (long)E) == 0 && n_sets <= (1 << 24),
                "%s: n_sets=%d M=%d E=%d (n_sets must be a multiple of E x M, at most 2^24)", who, n_sets, M, E);
    AVD_REQUIRE(d_seeds || E == 1, "%s: E=%d without a seed table", who, E);
    AVD_REQUIRE(d_gains && d_box && s && u_target, "%s: null pointer", who);
    AVD_REQUIRE(lo <= hi, "%s: lo=%g > hi=%g", who, (double)lo, (double)hi);
    const long n = (long)n_sets * TILE;
    hipLaunchKernelGGL(clone_sample_kernel, dim3((unsigned)((n + CLONE_THREADS - 1) / CLONE_THREADS)), dim3(CLONE_THREADS), 0,
                       (hipStream_t)stream, n_sets, S, M, d_gains, d_box, lo, hi, model_a, seed, counter, d_seeds, E, s, u_target);
    return check_launch(who);
}
