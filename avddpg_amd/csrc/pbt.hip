// Population-based training: one experiment's learner state copied onto another's inside a batch of interleaved experiments
// (avd_copy_experiment_sets_f32, include/avddpg_hip.h). A plain HBM stream: 16-byte loads and stores, no LDS, no atomics.
#include <vector>

#include "common.h"

using namespace avd;

namespace {

constexpr int PBT_MAX_PAIRS = 256;  // (src, dst) pairs per launch, passed by value
constexpr int PBT_THREADS = 256;
constexpr int PBT_UNR = 4;                               // float4 groups per thread and array in one unit
constexpr int PBT_CHUNK4 = PBT_THREADS * PBT_UNR;        // float4 groups of a row per unit
constexpr long PBT_MAX_BLOCKS = 8192;                    // grid cap: the blocks stride over the units

struct PbtPairs {
    int32_t src[PBT_MAX_PAIRS], dst[PBT_MAX_PAIRS];  // experiment indices
};

// Set k (0 <= k < sets per experiment) of experiment e: the k-th set j with (j / set_block) % n_groups == e.
__device__ __forceinline__ long set_of(int e, long k, int n_groups, int set_block) {
    return ((k / set_block) * n_groups + e) * set_block + k % set_block;
}

// One unit = one chunk of PBT_CHUNK4 float4 groups of one destination set's rows: theta, theta_t, m, v (t4 groups each) and stats,
// stats_t (s4 groups each); the chunk-0 unit also copies the step counter. Units are uniform per block (blockIdx only).
__global__ __launch_bounds__(PBT_THREADS) void copy_experiment_sets_kernel(
    const PbtPairs pairs, long n_units, int n_chunks, long sets_per_exp, int n_groups, int set_block, long t4, long s4,
    float4* __restrict__ theta, float4* __restrict__ stats, float4* __restrict__ theta_t, float4* __restrict__ stats_t,
    float4* __restrict__ m, float4* __restrict__ v, int32_t* __restrict__ step) {
    for (long u = blockIdx.x; u < n_units; u += gridDim.x) {
        const long row = u / n_chunks;
        const int c = (int)(u - row * n_chunks);
        const int p = (int)(row / sets_per_exp);
        const long k = row - (long)p * sets_per_exp;
        const long sj = set_of(pairs.src[p], k, n_groups, set_block);
        const long dj = set_of(pairs.dst[p], k, n_groups, set_block);
        const long i0 = (long)c * PBT_CHUNK4 + threadIdx.x;
#pragma unroll
        for (int q = 0; q < PBT_UNR; ++q) {  // 4 x 16 B in flight per thread and step: 128 KiB per CU at 8 waves per SIMD
            const long i = i0 + q * PBT_THREADS;
            if (i < t4) {
                const float4 x0 = theta[sj * t4 + i], x1 = theta_t[sj * t4 + i], x2 = m[sj * t4 + i], x3 = v[sj * t4 + i];
                theta[dj * t4 + i] = x0;
                theta_t[dj * t4 + i] = x1;
                m[dj * t4 + i] = x2;
                v[dj * t4 + i] = x3;
            }
        }
        for (long i = i0; i < s4 && i < (long)(c + 1) * PBT_CHUNK4; i += PBT_THREADS) {
            const float4 x = stats[sj * s4 + i], y = stats_t[sj * s4 + i];
            stats[dj * s4 + i] = x;
            stats_t[dj * s4 + i] = y;
        }
        if (c == 0 && threadIdx.x == 0) step[dj] = step[sj];
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int avd_copy_experiment_sets_f32(const avd_mlp_layout* lay, int n_sets, int n_groups, int set_block, const int32_t* pairs,
                                            int n_pairs, float* theta, float* stats, float* theta_t, float* stats_t, float* m, float* v,
                                            int32_t* step, void* stream) {
    const char* who = "avd_copy_experiment_sets_f32";
    // every check before the first launch: a refused call leaves every slab unchanged
    AVD_REQUIRE(lay && lay->theta_size > 0 && lay->stats_size > 0, "%s: null or empty layout", who);
    AVD_REQUIRE(n_sets > 0 && n_groups >= 1 && set_block >= 1 && n_sets % ((long)n_groups * set_block) == 0,
                "%s: n_sets=%d is not a positive multiple of n_groups=%d x set_block=%d", who, n_sets, n_groups, set_block);
    AVD_REQUIRE(n_pairs >= 0 && (n_pairs == 0 || pairs), "%s: n_pairs=%d, pairs=%p", who, n_pairs, (const void*)pairs);
    AVD_REQUIRE(theta && stats && theta_t && stats_t && m && v && step, "%s: null slab pointer", who);
    AVD_REQUIRE(lay->theta_size % 4 == 0 && lay->stats_size % 4 == 0, "%s: theta_size=%d / stats_size=%d are not 4-float aligned", who,
                lay->theta_size, lay->stats_size);
    AVD_REQUIRE(aligned16(theta) && aligned16(stats) && aligned16(theta_t) && aligned16(stats_t) && aligned16(m) && aligned16(v),
                "%s: a slab pointer is not 16-byte aligned", who);
    std::vector<char> is_dst(n_groups, 0);
    for (int i = 0; i < n_pairs; ++i) {
        const int s = pairs[2 * i], d = pairs[2 * i + 1];
        AVD_REQUIRE(s >= 0 && s < n_groups && d >= 0 && d < n_groups, "%s: pair %d = (%d, %d) is outside the %d experiments", who, i, s,
                    d, n_groups);
        AVD_REQUIRE(s != d, "%s: pair %d copies experiment %d onto itself", who, i, s);
        AVD_REQUIRE(!is_dst[d], "%s: experiment %d is the destination of two pairs", who, d);
        is_dst[d] = 1;
    }
    for (int i = 0; i < n_pairs; ++i) {
        const int s = pairs[2 * i];
        AVD_REQUIRE(!is_dst[s], "%s: experiment %d is both a source and a destination (the result would depend on the order)", who, s);
    }
    if (n_pairs == 0) return AVD_OK;
    const long sets_per_exp = n_sets / n_groups;
    const long t4 = lay->theta_size / 4, s4 = lay->stats_size / 4;
    const long rows4 = t4 > s4 ? t4 : s4;
    const int n_chunks = (int)((rows4 + PBT_CHUNK4 - 1) / PBT_CHUNK4);
    for (int lo = 0; lo < n_pairs; lo += PBT_MAX_PAIRS) {
        const int n = n_pairs - lo < PBT_MAX_PAIRS ? n_pairs - lo : PBT_MAX_PAIRS;
        PbtPairs pp;
        for (int i = 0; i < PBT_MAX_PAIRS; ++i) {
            pp.src[i] = i < n ? pairs[2 * (lo + i)] : 0;
            pp.dst[i] = i < n ? pairs[2 * (lo + i) + 1] : 0;
        }
        const long n_units = (long)n * sets_per_exp * n_chunks;
        const long blocks = n_units < PBT_MAX_BLOCKS ? n_units : PBT_MAX_BLOCKS;
        hipLaunchKernelGGL(copy_experiment_sets_kernel, dim3((unsigned)blocks), dim3(PBT_THREADS), 0, (hipStream_t)stream, pp, n_units,
                           n_chunks, sets_per_exp, n_groups, set_block, t4, s4, (float4*)theta, (float4*)stats, (float4*)theta_t,
                           (float4*)stats_t, (float4*)m, (float4*)v, step);
        const int rc = check_launch(who);
        if (rc != AVD_OK) return rc;
    }
    return AVD_OK;
}
