// Linear baseline of the scenario evaluator for gfx950: G gain sets x K cases of the evaluator rollout (evalx.hip's cases, start
// states, leader rows and per-case disturbance tables) in ONE launch, the controller a static gain row per vehicle instead of an MLP:
//   u = clip(((g0 * ob.x + g1 * ob.y) + g2 * ob.z) + g3 * ob.w, lo, hi)        (Model A: the first three terms; g3 is not read)
// with ob the observed state. The law, the observation model (V2V link, sensor noise), the platoon step, the reward and the metrics are
// eval_common.h's: eval_cases_kernel's (evalx.hip) text.
//
// A rollout is T dependent steps of a few dozen flops and shares nothing with any other, so the kernel is built for occupancy and
// latency, not bandwidth:
//   * one lane per (gain set, case, vehicle); the L lanes of a rollout are contiguous inside ONE wave, floor(64 / L) rollouts per wave,
//     the remaining lanes (and the lanes past the last rollout) return at once: they read nothing and write nothing;
//   * one wave per workgroup: nothing is shared between waves, and there is no barrier anywhere;
//   * the predecessor's chain value comes from lane - 1 with __shfl_up (a rollout never straddles a wave), not through LDS;
//   * a vehicle's plant (A, B, C: 24 floats), gains, disturbance scalars, state and metric accumulators live in registers;
//   * the V2V ring (disturbed only: 16 floats per lane) lives in LDS as [slot][lane]: the 64 lanes of a slot are 64 consecutive
//     dwords, so whatever slot each lane addresses (the delay differs per case) lane l hits bank l % 32 and the two 32-lane halves
//     of a ds_read_b32 / ds_write_b32 are conflict-free. A lane touches only its own column: no barrier. A dynamically indexed
//     register array would have become scratch. The nominal instantiation allocates no LDS;
//   * the leader row is read by the vehicle-0 lanes only, one step ahead of its use: the load's latency is off the dependent chain.
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (profiles/eval_linear_resource_usage.txt):
//   eval_linear_kernel<>         (nominal):    64 VGPRs, 0 AGPRs, no scratch,    0 B LDS, 8 waves per SIMD
//   eval_linear_kernel<DistArgs> (disturbed): 118 VGPRs, 0 AGPRs, no scratch, 4096 B LDS, 4 waves per SIMD (the registers are Box-Muller's
//                                             logf / sinf / cosf and Philox's; at 4096 gain sets x 12 cases x 5 vehicles the launch is
//                                             4096 waves, 4 per SIMD of 256 CUs, so the count does not limit that shape)
//   with a FreqArgs (a frequency sweep's ten sums per lane; profiles/eval_freq_resource_usage.txt): 80 VGPRs, 6 waves per SIMD nominal;
//                                             134 VGPRs, 3 waves per SIMD disturbed; no scratch
#include <limits.h>

#include "eval_common.h"

namespace avd {

constexpr int LIN_THREADS = 64;  // one wave

struct LinArgs {
    const avd_env_consts* cst;
    int G, K, L, T;
    const float* gains;    // [G][L][4]
    const float* x0;       // [K][L][4]
    const float* prev_a0;  // [K][L]
    const float* leader;   // [K][T]
    float lo, hi, inv_dt;
    float* counters;       // [G][K][L]
    float* metrics;        // [G][K][L][AVD_EVAL_NMETRIC] or null
};

// D is empty (nominal: the constants block's plant, a perfect observation, no LDS) or one DistArgs; a FreqArgs last adds the single-bin
// Fourier sums of a frequency sweep: every live lane reads its case's basis pair one step ahead of its use, as vehicle 0 reads the
// leader row (the L lanes of a rollout read the same address), and keeps its ten sums in registers (in LDS columns they cost the same
// 16 registers -- 80 and 134 either way, no scratch: profiles/eval_freq_resource_usage.txt)
template <class... D>
__global__ __launch_bounds__(LIN_THREADS) void eval_linear_kernel(const LinArgs a, const D... dist) {
#pragma clang fp contract(off)
    constexpr bool DIST = pack_has<DistArgs, D...>, FREQ = pack_has<FreqArgs, D...>;
    const int nv = a.L, lane = threadIdx.x;
    const int per_wave = LIN_THREADS / nv;
    const int rw = lane / nv, v = lane - rw * nv;
    const long roll = (long)blockIdx.x * per_wave + rw;  // (gain set, case) index of this lane's rollout
    if (rw >= per_wave || roll >= (long)a.G * a.K) return;
    const int g = (int)(roll / a.K), k = (int)(roll - (long)g * a.K);
    const avd_env_consts* cst = a.cst;
    const long kv = (long)k * nv + v;
    // this vehicle's plant A (16, row-major), B (4), C (4): registers for the whole rollout
    float abc[24];
    bool table = false;
    if constexpr (DIST) {
        const DistArgs& da = pack_get<DistArgs>(dist...);
        if (da.abc) {
            table = true;
#pragma unroll
            for (int e = 0; e < 24; ++e) abc[e] = da.abc[kv * 24 + e];
        }
    }
    if (!table) {
#pragma unroll
        for (int e = 0; e < 16; ++e) abc[e] = cst->A[v][e];
#pragma unroll
        for (int e = 0; e < 4; ++e) abc[16 + e] = cst->B[v][e], abc[20 + e] = cst->C[v][e];
    }
    const float* gp = a.gains + ((long)g * nv + v) * 4;
    const float4 gn = make_float4(gp[0], gp[1], gp[2], gp[3]);
    float4 xv = make_float4(a.x0[kv * 4], a.x0[kv * 4 + 1], a.x0[kv * 4 + 2], a.x0[kv * 4 + 3]);
    float pa = a.prev_a0[kv], cnt = 0.f;
    VehMetrics met;
    const bool model_a = cst->model_a != 0;
    const float* leader = a.leader + (long)k * a.T;
    float lead_next = (v == 0) ? leader[0] : 0.f;
    // ---- the case's disturbance (disturbed only) ----
    float sg_ep = 0.f, sg_ev = 0.f, sg_a = 0.f, recv = 0.f;
    int dly = 0;
    uint32_t dq = 0;
    uint64_t nseed = 0;
    float* ring = nullptr;
    if constexpr (DIST) {
        __shared__ float s_ring[EVAL_RING * LIN_THREADS];  // [slot][lane]
        const DistArgs& da = pack_get<DistArgs>(dist...);
        sg_ep = da.sigma[k * 3L], sg_ev = da.sigma[k * 3L + 1], sg_a = da.sigma[k * 3L + 2];
        dly = da.delay[k] & (EVAL_RING - 1);  // (the host refuses delays outside the ring; the mask keeps any value inside it)
        dq = da.drop_q[k];
        nseed = da.noise_seed[k];
        ring = s_ring + lane;
#pragma unroll
        for (int j = 0; j < EVAL_RING; ++j) ring[j * LIN_THREADS] = xv.w;  // steps before the first: x0's
        recv = xv.w;                                                        // and the last received value
    }
    const float2* basis = nullptr;
    float2 cs_next = make_float2(0.f, 0.f);
    VehSpectrum spc;
    if constexpr (FREQ) {
        basis = (const float2*)pack_get<FreqArgs>(dist...).basis + (long)k * a.T;
        cs_next = basis[0];
    }
    for (int t = 0; t < a.T; ++t) {
        const float lead = lead_next;
        if (v == 0 && t + 1 < a.T) lead_next = leader[t + 1];  // next step's, in flight during this one
        const float2 cs = cs_next;
        if constexpr (FREQ)
            if (t + 1 < a.T) cs_next = basis[t + 1];
        // ---- what the controller sees of the true pre-step state xv ----
        float4 ob = xv;
        if constexpr (DIST) {
            ob.w = v2v_link<LIN_THREADS>(ring, recv, xv.w, t, dly, dq, nseed, (uint32_t)v);
            observe_noise(ob, xv, sg_ep, sg_ev, sg_a, nseed, (uint64_t)t, (uint32_t)v, STREAM_EVAL_OBS);
        }
        // ---- the linear law, platoon step ----
        const float uu = fminf(fmaxf(linear_law(gn, ob, model_a), a.lo), a.hi);  // np.clip
        const VehStep vs = veh_step_pre(cst, abc, abc + 16, xv, uu);
        const float up = __shfl_up(vs.chain, 1);  // lane - 1: the predecessor of every vehicle but the first
        const float exog = (v == 0) ? lead : up;
        float4 xn;
        const float nr = veh_step_post(cst, vs, abc + 16, abc + 20, xv, pa, uu, exog, xn);
        cnt = cnt + nr;  // counters += env.reward[0], per vehicle (decentralized)
        met.step(cst, xv, xn, pa, uu, a.inv_dt, t);
        if constexpr (FREQ) spc.step(xn, uu, cs);
        pa = xv.z;  // prev_x <- x
        xv = xn;
    }
    a.counters[roll * nv + v] = cnt;
    if (a.metrics) met.store(a.metrics + (roll * nv + v) * AVD_EVAL_NMETRIC, xv);
    if constexpr (FREQ) {
        spc.store(pack_get<FreqArgs>(dist...).spectrum + (roll * nv + v) * AVD_EVAL_NSPEC);
    }
}

// One thread per gain set: the sequential float32 sum of its K * L counters in (k, v) order, divided by (float)(K * L)
__global__ __launch_bounds__(256) void linear_fitness_kernel(int G, long n, const float* __restrict__ counters, float* __restrict__ fitness) {
#pragma clang fp contract(off)
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const float* c = counters + (long)g * n;
    float s = 0.f;
    for (long i = 0; i < n; ++i) s = s + c[i];
    fitness[g] = s / (float)n;
}

template <class... D>
int launch_linear(const char* who, const LinArgs& a, long blocks, hipStream_t stream, const D&... dist) {
    hipLaunchKernelGGL((eval_linear_kernel<D...>), dim3((unsigned)blocks), dim3(LIN_THREADS), 0, stream, a, dist...);
    return check_launch(who);
}

}  // namespace avd

using namespace avd;

// Both linear entry points: the checks, the argument block and the launch. freq: a frequency sweep's basis and spectrum, or null.
static int linear_launch(const char* who, const FreqArgs* freq, const avd_env_consts* d_consts, int G, int K, int L, int T, const float* gains,
                         const float* x0, const float* prev_a0, const float* leader, float lo, float hi, float sample_rate,
                         const float* sigma, const int32_t* delay, const uint32_t* drop_q, const uint64_t* noise_seed, const float* abc,
                         float* counters, float* metrics, void* stream) {
    AVD_REQUIRE(d_consts && gains && x0 && prev_a0 && leader && counters, "%s: null pointer", who);
    AVD_REQUIRE(L >= 1 && L <= AVD_MAX_L, "%s: L=%d (L must be 1..%d)", who, L, AVD_MAX_L);
    AVD_REQUIRE(G >= 1 && K >= 1 && T >= 1, "%s: G=%d K=%d T=%d (all must be >= 1)", who, G, K, T);
    AVD_REQUIRE(sample_rate > 0.f, "%s: sample_rate=%g", who, (double)sample_rate);
    const bool dist = sigma || delay || drop_q || noise_seed || abc;
    AVD_REQUIRE(!dist || (sigma && delay && drop_q && noise_seed),
                "%s: null disturbance table (all five null: the nominal plant and a perfect observation; otherwise only abc may be null)", who);
    const long long rollouts = (long long)G * K, per_wave = LIN_THREADS / L;
    const long long blocks = (rollouts + per_wave - 1) / per_wave;
    if (blocks > INT_MAX) {
        set_error("%s: G=%d x K=%d = %lld rollouts, %lld per workgroup at L=%d, need %lld workgroups (the grid holds %d)", who, G, K, rollouts,
                  per_wave, L, blocks, INT_MAX);
        return AVD_E_UNSUPPORTED;
    }
    if (freq)
        if (const int rc = freq_check(who, *freq)) return rc;
    LinArgs a;
    a.cst = d_consts, a.G = G, a.K = K, a.L = L, a.T = T, a.gains = gains, a.x0 = x0, a.prev_a0 = prev_a0, a.leader = leader;
    a.lo = lo, a.hi = hi;
    a.inv_dt = 1.0f / sample_rate;  // host float32 division, as avd_eval_cases_f32 forms it
    a.counters = counters, a.metrics = metrics;
    const DistArgs d = {sigma, delay, drop_q, noise_seed, abc};
    if (freq) return dist ? launch_linear(who, a, (long)blocks, (hipStream_t)stream, d, *freq) : launch_linear(who, a, (long)blocks, (hipStream_t)stream, *freq);
    if (!dist) return launch_linear(who, a, (long)blocks, (hipStream_t)stream);
    return launch_linear(who, a, (long)blocks, (hipStream_t)stream, d);
}

extern "C" int avd_eval_linear_f32(const avd_env_consts* d_consts, int G, int K, int L, int T, const float* gains, const float* x0,
                                   const float* prev_a0, const float* leader, float lo, float hi, float sample_rate, const float* sigma,
                                   const int32_t* delay, const uint32_t* drop_q, const uint64_t* noise_seed, const float* abc,
                                   float* counters, float* metrics, void* stream) {
    return linear_launch("avd_eval_linear_f32", nullptr, d_consts, G, K, L, T, gains, x0, prev_a0, leader, lo, hi, sample_rate, sigma, delay,
                         drop_q, noise_seed, abc, counters, metrics, stream);
}

// The linear scenario evaluator of a frequency sweep: avd_eval_linear_f32's arguments plus the per-case basis table and the spectrum output
extern "C" int avd_eval_linear_freq_f32(const avd_env_consts* d_consts, int G, int K, int L, int T, const float* gains, const float* x0,
                                        const float* prev_a0, const float* leader, float lo, float hi, float sample_rate,
                                        const float* sigma, const int32_t* delay, const uint32_t* drop_q, const uint64_t* noise_seed,
                                        const float* abc, float* counters, float* metrics, const float* basis, float* spectrum,
                                        void* stream) {
    const FreqArgs f = {basis, spectrum};
    return linear_launch("avd_eval_linear_freq_f32", &f, d_consts, G, K, L, T, gains, x0, prev_a0, leader, lo, hi, sample_rate, sigma, delay,
                         drop_q, noise_seed, abc, counters, metrics, stream);
}

extern "C" int avd_linear_fitness_f32(int G, int K, int L, const float* counters, float* fitness, void* stream) {
    const char* who = "avd_linear_fitness_f32";
    AVD_REQUIRE(counters && fitness, "%s: null pointer", who);
    AVD_REQUIRE(L >= 1 && L <= AVD_MAX_L, "%s: L=%d (L must be 1..%d)", who, L, AVD_MAX_L);
    AVD_REQUIRE(G >= 1 && K >= 1, "%s: G=%d K=%d (both must be >= 1)", who, G, K);
    hipLaunchKernelGGL(linear_fitness_kernel, dim3((G + 255) / 256), dim3(256), 0, (hipStream_t)stream, G, (long)K * L, counters, fitness);
    return check_launch(who);
}
