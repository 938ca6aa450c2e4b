// Target policy smoothing (TD3's): the split set learner's target actions a2 = mu'(s2) [n_agents][64] become
//   a2' = clip(a2 + clip(sigma n, -c, c), lo, hi),   n ~ N(0, 1)
// in place, in one elementwise launch between the target actor's head (OUT_TANH, which writes a2) and the target critic's (OUT_TD, its
// only reader). Plain 16-byte loads and stores, no LDS, no atomics. A thread owns rows 4q .. 4q + 3 of one agent's tile: one Philox block
// = two Box-Muller pairs = its four normals. The draw is keyed by (experiment's key, learner call, SOLO agent index, q): it knows
// neither the experiment's place in a seed batch nor the other experiments, so experiment e of a batch draws what its solo run draws.
#include <math.h>

#include "common.h"
#include "smooth.h"

namespace avd {

constexpr int SMOOTH_THREADS = 256;  // 16 agents per workgroup
constexpr int SMOOTH_PER_AGENT = 16;  // threads per 64-row tile

// np.clip for an ordered pair of bounds; a NaN stays a NaN (fminf / fmaxf would hand back a bound: the chain's non-finite flag is
// raised by the heads before this kernel runs and does not depend on it, and the stand-alone call must not hide one either)
__device__ __forceinline__ float clip_keep_nan(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ __launch_bounds__(SMOOTH_THREADS) void target_smooth_kernel(const SmoothArgs p) {
#pragma clang fp contract(off)
    const long t = (long)blockIdx.x * SMOOTH_THREADS + threadIdx.x;
    if (t >= (long)p.n_agents * SMOOTH_PER_AGENT) return;  // the tail workgroup: fewer than 16 agents
    const int v = (int)(t / SMOOTH_PER_AGENT), q = (int)(t % SMOOTH_PER_AGENT);
    const int m = v % p.M, e = (v / p.M) % p.E, vs = (v / (p.E * p.M)) * p.M + m;  // agent = (platoon, experiment, vehicle)
    const uint64_t key = p.seeds ? p.seeds[e] : p.seed;
    const u32x4 w = philox_at(key, p.counter, (uint32_t)vs * SMOOTH_PER_AGENT + (uint32_t)q, STREAM_SMOOTH);
    float n[4];
    n[0] = box_muller(w.x, w.y, &n[1]);
    n[2] = box_muller(w.z, w.w, &n[3]);
    float4* at = (float4*)p.a2 + t;  // rows 4q .. 4q + 3 of agent v: 16 bytes, consecutive threads consecutive
    float4 x = *at;
    float* xs = &x.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float eps = fminf(fmaxf(p.sigma * n[k], -p.clip), p.clip);  // (clip = +inf: no noise clip)
        xs[k] = clip_keep_nan(xs[k] + eps, p.lo, p.hi);
    }
    *at = x;
}

int check_smooth(const char* who, const SmoothArgs& q) {
    AVD_REQUIRE(q.M >= 1 && q.E >= 1, "%s: M=%d E=%d (both must be >= 1)", who, q.M, q.E);
    AVD_REQUIRE(q.seeds || q.E == 1, "%s: E=%d without a seed table", who, q.E);
    AVD_REQUIRE(isfinite(q.sigma) && q.sigma >= 0.f, "%s: sigma=%g (must be finite and >= 0)", who, (double)q.sigma);
    AVD_REQUIRE(q.clip > 0.f, "%s: noise_clip=%g (must be > 0; +inf: no clip)", who, (double)q.clip);  // (a NaN fails the comparison)
    AVD_REQUIRE(q.lo <= q.hi, "%s: lo=%g > hi=%g", who, (double)q.lo, (double)q.hi);
    return AVD_OK;
}

void launch_target_smooth(const SmoothArgs& q, hipStream_t st) {
    const long threads = (long)q.n_agents * SMOOTH_PER_AGENT;
    hipLaunchKernelGGL(target_smooth_kernel, dim3((unsigned)((threads + SMOOTH_THREADS - 1) / SMOOTH_THREADS)), dim3(SMOOTH_THREADS), 0, st, q);
}

}  // namespace avd

using namespace avd;

extern "C" int avd_target_smooth_f32(int n_agents, int M, int E, float* a2, float sigma, float noise_clip, float lo, float hi, uint64_t seed,
                                     uint64_t counter, const uint64_t* d_seeds, void* stream) {
    const char* who = "avd_target_smooth_f32";
    AVD_REQUIRE(a2, "%s: null a2", who);
    AVD_REQUIRE(((uintptr_t)a2 & 15) == 0, "%s: a2 must be 16-byte aligned", who);
    AVD_REQUIRE(n_agents >= 1 && n_agents <= (1 << 24), "%s: n_agents=%d (1 .. 2^24)", who, n_agents);
    SmoothArgs q{};
    q.n_agents = n_agents, q.a2 = a2, q.M = M, q.E = E, q.sigma = sigma, q.clip = noise_clip, q.lo = lo, q.hi = hi;
    q.seed = seed, q.counter = counter, q.seeds = d_seeds;
    int rc = check_smooth(who, q);
    if (rc) return rc;
    AVD_REQUIRE(n_agents % ((long)E * M) == 0, "%s: n_agents=%d M=%d E=%d (n_agents must be a multiple of E x M)", who, n_agents, M, E);
    launch_target_smooth(q, (hipStream_t)stream);
    return check_launch(who);
}
