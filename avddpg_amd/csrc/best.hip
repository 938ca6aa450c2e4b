// Keep the best actors seen in training (avd_keep_best_f32, include/avddpg_hip.h): the evaluator rollout's counters reduced to one
// score per unit, compared with the unit's best so far, and the actors of the units that improved copied into a snapshot slab.
// Two launches on one stream: a per-unit decision (one thread per unit: nobody else reads or writes that unit's score), then the copy,
// which only reads the decision. The copy is a plain HBM stream as csrc/pbt.hip: 16-byte loads and stores, no LDS, no atomics.
#include "common.h"

using namespace avd;

namespace {

constexpr int KEEP_THREADS = 256;
constexpr int KEEP_UNR = 4;                              // float4 groups per thread in one work item
constexpr int KEEP_CHUNK4 = KEEP_THREADS * KEEP_UNR;     // float4 groups of a row per work item
constexpr long KEEP_MAX_BLOCKS = 8192;                   // grid cap: the blocks stride over the work items
// (mirrored in avddpg_amd/_hip.py: KEEP_THREADS, KEEP_UNR, KEEP_CHUNK4, KEEP_MAX_BLOCKS)

// Unit u: score = (sum of its NS * M counters in memory order, one IEEE add each, from the first element) / (float)(NS * M);
// it improves iff score > best_score[u] (strict: a tie keeps the older snapshot; a NaN never improves).
__global__ __launch_bounds__(KEEP_THREADS) void keep_best_decide_kernel(int n_units, int M, int NS, int n_sets,
                                                                        const int32_t* __restrict__ set_base,
                                                                        const float* __restrict__ counters, int64_t step_now,
                                                                        float* __restrict__ best_score, int64_t* __restrict__ best_step,
                                                                        int32_t* __restrict__ improved) {
#pragma clang fp contract(off)
    const int u = blockIdx.x * KEEP_THREADS + threadIdx.x;
    if (u >= n_units) return;
    const int n = NS * M;
    const float* c = counters + (long)u * n;
    float s = c[0];
    for (int i = 1; i < n; ++i) s = s + c[i];
    const float score = s / (float)n;
    const int base = set_base[u];
    // (the host has checked its copy of the table; a device table that disagrees must still not send the copy out of bounds)
    const bool better = score > best_score[u] && base >= 0 && base <= n_sets - M;
    if (better) {
        best_score[u] = score;
        best_step[u] = step_now;
    }
    improved[u] = better ? 1 : 0;
}

// One work item = one chunk of KEEP_CHUNK4 float4 groups of one snapshot row (unit u, model m): the actor span of theta (a4 groups) and
// the actor's statistics (s4 groups). Work items are uniform per block (blockIdx only); a unit that did not improve touches nothing.
__global__ __launch_bounds__(KEEP_THREADS) void keep_best_copy_kernel(long n_items, int n_chunks, int M, long t4, long st4, long a4, long s4,
                                                                      const int32_t* __restrict__ set_base,
                                                                      const int32_t* __restrict__ improved,
                                                                      const float4* __restrict__ theta, const float4* __restrict__ stats,
                                                                      float4* __restrict__ best_theta, float4* __restrict__ best_stats) {
    for (long w = blockIdx.x; w < n_items; w += gridDim.x) {
        const long row = w / n_chunks;
        const int c = (int)(w - row * n_chunks);
        const long u = row / M;
        if (!improved[u]) continue;
        const long set = (long)set_base[u] + (row - u * M);
        const long i0 = (long)c * KEEP_CHUNK4 + threadIdx.x;
        const float4* src = theta + set * t4;
        float4* dst = best_theta + row * a4;
        float4 x[KEEP_UNR];
#pragma unroll
        for (int q = 0; q < KEEP_UNR; ++q) {  // 4 x 16 B in flight per thread
            const long i = i0 + q * KEEP_THREADS;
            if (i < a4) x[q] = src[i];
        }
#pragma unroll
        for (int q = 0; q < KEEP_UNR; ++q) {
            const long i = i0 + q * KEEP_THREADS;
            if (i < a4) dst[i] = x[q];
        }
        for (long i = i0; i < s4 && i < (long)(c + 1) * KEEP_CHUNK4; i += KEEP_THREADS) best_stats[row * s4 + i] = stats[set * st4 + i];
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int avd_keep_best_f32(const avd_mlp_layout* lay, int n_units, int M, int NS, int n_sets, const int32_t* d_set_base,
                                 const int32_t* h_set_base, const float* counters, const float* theta, const float* stats,
                                 int64_t step_now, float* best_theta, float* best_stats, float* best_score, int64_t* best_step,
                                 int32_t* improved, void* stream) {
    const char* who = "avd_keep_best_f32";
    // every check before the first launch: a refused call leaves every array unchanged
    AVD_REQUIRE(lay && lay->theta_size > 0 && lay->stats_size > 0 && lay->actor_size > 0 && lay->cmms > 0, "%s: null or empty layout", who);
    AVD_REQUIRE(n_units >= 1 && M >= 1 && NS >= 1, "%s: n_units=%d M=%d NS=%d (each must be >= 1)", who, n_units, M, NS);
    AVD_REQUIRE(n_sets >= M, "%s: n_sets=%d holds no unit of M=%d sets", who, n_sets, M);
    AVD_REQUIRE((long)n_units * M <= 0x7fffffffL && (long)NS * M <= 0x7fffffffL, "%s: n_units=%d x M=%d or NS=%d x M overflows an int",
                who, n_units, M, NS);
    AVD_REQUIRE(d_set_base && h_set_base && counters && theta && stats && best_theta && best_stats && best_score && best_step && improved,
                "%s: null pointer", who);
    AVD_REQUIRE(lay->theta_size % 4 == 0 && lay->stats_size % 4 == 0 && lay->actor_size % 4 == 0 && lay->cmms % 4 == 0 &&
                    lay->actor_size <= lay->theta_size && lay->cmms <= lay->stats_size,
                "%s: theta_size=%d / stats_size=%d / actor_size=%d / cmms=%d are not 4-float aligned spans", who, lay->theta_size,
                lay->stats_size, lay->actor_size, lay->cmms);
    AVD_REQUIRE(aligned16(theta) && aligned16(stats) && aligned16(best_theta) && aligned16(best_stats),
                "%s: a slab pointer is not 16-byte aligned", who);
    for (int u = 0; u < n_units; ++u)
        AVD_REQUIRE(h_set_base[u] >= 0 && h_set_base[u] <= n_sets - M, "%s: set_base[%d]=%d is outside [0, n_sets - M = %d]", who, u,
                    h_set_base[u], n_sets - M);
    const long t4 = lay->theta_size / 4, st4 = lay->stats_size / 4, a4 = lay->actor_size / 4, s4 = lay->cmms / 4;
    const long rows4 = a4 > s4 ? a4 : s4;
    const int n_chunks = (int)((rows4 + KEEP_CHUNK4 - 1) / KEEP_CHUNK4);
    hipLaunchKernelGGL(keep_best_decide_kernel, dim3((unsigned)((n_units + KEEP_THREADS - 1) / KEEP_THREADS)), dim3(KEEP_THREADS), 0,
                       (hipStream_t)stream, n_units, M, NS, n_sets, d_set_base, counters, step_now, best_score, best_step, improved);
    int rc = check_launch(who);
    if (rc != AVD_OK) return rc;
    const long n_items = (long)n_units * M * n_chunks;
    const long blocks = n_items < KEEP_MAX_BLOCKS ? n_items : KEEP_MAX_BLOCKS;
    hipLaunchKernelGGL(keep_best_copy_kernel, dim3((unsigned)blocks), dim3(KEEP_THREADS), 0, (hipStream_t)stream, n_items, n_chunks, M, t4,
                       st4, a4, s4, d_set_base, improved, (const float4*)theta, (const float4*)stats, (float4*)best_theta,
                       (float4*)best_stats);
    return check_launch(who);
}
