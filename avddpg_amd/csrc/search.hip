// Cross-entropy search over linear gain tables for gfx950 (evaluator.search_linear): the two launches that stand around the linear
// evaluator's rollout (lin.hip) in one generation -- sample G candidate tables from a per-dimension normal, and refit that normal to
// the best of them -- so that a whole search is enqueued without a read-back. R searched rows: R = L (one gain row per vehicle) or
// R = 1 (tied: every vehicle takes row 0). All arithmetic is float32 without contraction, in the order include/avddpg_hip.h states;
// tests/search_oracle.py restates it in NumPy.
//   * search_sample_kernel: one thread per (candidate, vehicle), one Philox block and two Box-Muller pairs for its four gains, one
//     float4 store. Candidate 0 is the mean itself. Nothing is shared: no LDS, no barrier.
//   * search_rank_kernel: a candidate's rank is the number of candidates that precede it (fitness descending, lower index first among
//     equals, NaNs last by index). 16 lanes share a candidate, each counting over every 16th other candidate from LDS tiles of the
//     fitness array, and add their counts with shuffles (one thread per candidate, the first form, waited for an LDS read per comparison:
//     a 4096-candidate refit measured 0.172 ms with it and 0.051 ms with this one). Ranks are a permutation of 0..G-1, so elite_idx[rank] = i is a
//     plain store no other thread aims at. G <= 65536: at most 4096 blocks x 256 tiles.
//   * search_refit_kernel: ONE wave, lane d = r * 4 + c owns searched dimension (r, c) (R * 4 <= 64). The sums are sequential in rank
//     order, so a lane that fetched its own terms would pay two dependent global loads (index, value) per term (measured: 0.16 ms more
//     per refit at 512 elites). Instead lane t stages elite base + t (its fitness and its R rows, float4 loads) into LDS as [dimension][elite], pitch
//     65 floats -- writes of one dimension by 64 lanes and reads of one elite by the dimension lanes both fall on banks (d + k) % 32,
//     conflict-free per 32-lane half -- and the dimension lanes add 64 terms from LDS; two passes (mean, then squared deviations).
//     The number of valid elites falls out of pass 1 (NaNs rank last, so the valid ones are a prefix: a ballot per chunk). Each lane
//     writes the values it owns, lane 0 also the scalars; every input of the best-ever update is loaded before any lane stores. No atomics.
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage:
//   search_sample_kernel:  39 VGPRs, 0 AGPRs, no scratch,    0 B LDS, 8 waves per SIMD
//   search_rank_kernel:    13 VGPRs, 0 AGPRs, no scratch, 1024 B LDS, 8 waves per SIMD
//   search_refit_kernel:   47 VGPRs, 0 AGPRs, no scratch, 16896 B LDS, 3 waves per SIMD (the LDS; the launch is one wave)
#include <limits.h>
#include <math.h>

#include "common.h"

namespace avd {

constexpr int SEARCH_THREADS = 256;
constexpr int SEARCH_MAX_G = 65536;  // of a refit: the rank kernel compares every pair

__global__ __launch_bounds__(SEARCH_THREADS) void search_sample_kernel(int G, int L, int R, const float* __restrict__ mean,
                                                                       const float* __restrict__ std, const float* __restrict__ lo,
                                                                       const float* __restrict__ hi, uint64_t seed, uint64_t generation,
                                                                       float* __restrict__ gains) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * SEARCH_THREADS + threadIdx.x;  // (candidate, vehicle)
    if (idx >= (long)G * L) return;
    const int g = (int)(idx / L), v = (int)(idx - (long)g * L);
    const int r = (R == 1) ? 0 : v;
    const u32x4 w = philox_at(seed, generation, (uint32_t)g * (uint32_t)R + (uint32_t)r, STREAM_SEARCH);
    float n[4];
    n[0] = box_muller(w.x, w.y, &n[1]);
    n[2] = box_muller(w.z, w.w, &n[3]);
    const float4 m = *reinterpret_cast<const float4*>(mean + r * 4), s = *reinterpret_cast<const float4*>(std + r * 4);
    const float4 l = *reinterpret_cast<const float4*>(lo + r * 4), h = *reinterpret_cast<const float4*>(hi + r * 4);
    const float mm[4] = {m.x, m.y, m.z, m.w}, ss[4] = {s.x, s.y, s.z, s.w}, ll[4] = {l.x, l.y, l.z, l.w}, hh[4] = {h.x, h.y, h.z, h.w};
    float x[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float t = mm[c];
        if (g != 0 && ss[c] != 0.f) t = mm[c] + ss[c] * n[c];  // candidate 0 and a frozen dimension skip the add: exact
        x[c] = fminf(fmaxf(t, ll[c]), hh[c]);
    }
    *reinterpret_cast<float4*>(gains + idx * 4) = make_float4(x[0], x[1], x[2], x[3]);
}

constexpr int RANK_SEGS = 16;                           // lanes that share one candidate's comparisons
constexpr int RANK_CANDS = SEARCH_THREADS / RANK_SEGS;  // candidates per block

// Candidate j precedes candidate i iff j is not NaN and (i is NaN or f_j > f_i or (f_j == f_i and j < i)); among NaNs the lower index.
// Thread (c, seg) of a block compares candidate i = block * 16 + c with the candidates j = seg (mod 16); the 16 partial counts of a
// candidate sit in 16 adjacent lanes and are added with shuffles. A tile is 256 fitness values in LDS: a wave's read t touches the 16
// consecutive dwords t * 16 + seg (the same for its 4 candidates: a broadcast), conflict-free, and the 16 reads of a tile do not depend
// on each other. The next tile's value is loaded into a register while this one is compared. Places past G hold NaN with an index
// >= G > i, which precedes nothing.
__global__ __launch_bounds__(SEARCH_THREADS) void search_rank_kernel(int G, int n_elite, const float* __restrict__ fitness,
                                                                     int32_t* __restrict__ elite_idx) {
    __shared__ float s_f[SEARCH_THREADS];
    const int tid = threadIdx.x, c = tid / RANK_SEGS, seg = tid % RANK_SEGS;
    const int i = blockIdx.x * RANK_CANDS + c;
    const float fi = (i < G) ? fitness[i] : 0.f;
    const bool nan_i = fi != fi;
    int rank = 0;
    float nxt = (tid < G) ? fitness[tid] : __builtin_nanf("");
    for (int base = 0; base < G; base += SEARCH_THREADS) {
        __syncthreads();  // the previous tile has been read by every thread
        s_f[tid] = nxt;
        __syncthreads();
        const int j1 = base + SEARCH_THREADS + tid;
        nxt = (j1 < G) ? fitness[j1] : __builtin_nanf("");
#pragma unroll
        for (int t = 0; t < SEARCH_THREADS / RANK_SEGS; ++t) {
            const float fj = s_f[t * RANK_SEGS + seg];
            const int j = base + t * RANK_SEGS + seg;
            const bool nan_j = fj != fj;
            const bool pre = nan_i ? (!nan_j || j < i) : (fj > fi || (fj == fi && j < i));
            rank += pre ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = RANK_SEGS / 2; o >= 1; o >>= 1) rank += __shfl_xor(rank, o);
    if (seg == 0 && i < G && rank < n_elite) elite_idx[rank] = i;
}

struct RefitArgs {
    int G, L, R, n_elite;
    float alpha;
    const float* gains;    // [G][L][4]
    const float* fitness;  // [G]
    const float* min_std;  // [R][4]
    float* mean;           // [R][4]
    float* std;            // [R][4]
    float* best_gains;     // [R][4]
    float* best_fitness;   // [1]
    int32_t* best_gen;     // [1]
    int generation;
    const int32_t* elite_idx;  // [n_elite], the rank kernel's
    float* history_row;        // [4]
};

constexpr int REFIT_CHUNK = 64;               // elites staged per step, one per lane
constexpr int REFIT_PITCH = REFIT_CHUNK + 1;  // of s_x[dimension][elite]: lane d reads bank (d + k) % 32, lane k writes bank (d + k) % 32

// This lane's elite (rank k) into the stage: its fitness and the R rows of its table, as float4 loads
__device__ __forceinline__ void refit_stage(const RefitArgs& a, int k, int lane, float* s_x, float* s_f) {
    const int e = a.elite_idx[k];
    s_f[lane] = a.fitness[e];
    const float4* g = reinterpret_cast<const float4*>(a.gains + (long)e * a.L * 4);
    for (int r = 0; r < a.R; ++r) {
        const float4 v = g[r];
        float* o = s_x + (r * 4) * REFIT_PITCH + lane;
        o[0] = v.x, o[REFIT_PITCH] = v.y, o[2 * REFIT_PITCH] = v.z, o[3 * REFIT_PITCH] = v.w;
    }
}

__global__ __launch_bounds__(64) void search_refit_kernel(const RefitArgs a) {
#pragma clang fp contract(off)
    // The sums run in rank order, one lane per dimension, but a lane that fetched its own operands would wait out two dependent loads
    // (index, then value) per term. So the 64 lanes fetch 64 elites at a time into LDS, all loads in flight at once, and the sums read LDS.
    __shared__ float s_x[64 * REFIT_PITCH];
    __shared__ float s_f[REFIT_CHUNK];
    const int d = threadIdx.x, nd = a.R * 4;
    const float best_f_in = a.best_fitness[0];  // (every input of the best-ever update is read before any lane stores)
    const int best_g_in = a.best_gen[0];
    const float* mine = s_x + d * REFIT_PITCH;
    // ---- pass 1: E = min(n_elite, n_valid) (NaNs rank last: the valid entries of the ranked list are a prefix), the sums of x and f
    int E = 0;
    float s = 0.f, fs = 0.f;
    for (int base = 0; base < a.n_elite; base += REFIT_CHUNK) {
        bool valid = false;
        if (base + d < a.n_elite) {
            refit_stage(a, base + d, d, s_x, s_f);
            valid = s_f[d] == s_f[d];
        }
        const int nv = __popcll(__ballot(valid));
        __syncthreads();
        if (d < nd)
            for (int t = 0; t < nv; ++t) s = s + mine[t];
        if (d == 0)
            for (int t = 0; t < nv; ++t) fs = fs + s_f[t];
        E += nv;
        __syncthreads();  // the stage is reused
        if (nv < REFIT_CHUNK) break;
    }
    if (E == 0) {  // nothing valid: the distribution and the best-ever record stay
        if (d == 0) {
            a.history_row[0] = __builtin_nanf(""), a.history_row[1] = __builtin_nanf("");
            a.history_row[2] = best_f_in, a.history_row[3] = 0.f;
        }
        return;
    }
    // ---- pass 2: the squared deviations from m
    const float m = s / (float)E;
    float q = 0.f;
    for (int base = 0; base < E; base += REFIT_CHUNK) {
        if (base + d < E) refit_stage(a, base + d, d, s_x, s_f);
        __syncthreads();
        const int n = min(REFIT_CHUNK, E - base);
        if (d < nd)
            for (int t = 0; t < n; ++t) {
                const float dev = mine[t] - m;
                q = q + dev * dev;
            }
        __syncthreads();
    }
    const int top = a.elite_idx[0];
    const float f_top = a.fitness[top];
    const bool better = best_g_in < 0 || f_top > best_f_in;  // strict: the first generation that reaches a value keeps it
    if (d < nd) {
        const float sd = sqrtf(q / (float)E);
        const float mu = a.mean[d], sg = a.std[d];
        const float top_x = a.gains[(long)top * a.L * 4 + d];  // row r = d / 4 of the R searched rows, column d % 4
        if (sg != 0.f) {  // a frozen dimension never moves
            a.mean[d] = mu + a.alpha * (m - mu);
            a.std[d] = fmaxf(sg + a.alpha * (sd - sg), a.min_std[d]);
        }
        if (better) a.best_gains[d] = top_x;
    }
    if (d == 0) {
        if (better) a.best_fitness[0] = f_top, a.best_gen[0] = a.generation;
        a.history_row[0] = f_top, a.history_row[1] = fs / (float)E;
        a.history_row[2] = better ? f_top : best_f_in, a.history_row[3] = (float)E;
    }
}

}  // namespace avd

using namespace avd;

extern "C" int avd_search_sample_f32(int G, int L, int R, const float* mean, const float* std, const float* lo, const float* hi,
                                     uint64_t seed, uint64_t generation, float* gains, void* stream) {
    const char* who = "avd_search_sample_f32";
    AVD_REQUIRE(mean && std && lo && hi && gains, "%s: null pointer", who);
    AVD_REQUIRE(G >= 1, "%s: G=%d (G must be >= 1)", who, G);
    AVD_REQUIRE(L >= 1 && L <= AVD_MAX_L, "%s: L=%d (L must be 1..%d)", who, L, AVD_MAX_L);
    AVD_REQUIRE(R == 1 || R == L, "%s: R=%d (R must be 1, tied rows, or L=%d, one row per vehicle)", who, R, L);
    const long long threads = (long long)G * L, blocks = (threads + SEARCH_THREADS - 1) / SEARCH_THREADS;
    if (blocks > INT_MAX) {
        set_error("%s: G=%d x L=%d = %lld threads need %lld workgroups (the grid holds %d)", who, G, L, threads, blocks, INT_MAX);
        return AVD_E_UNSUPPORTED;
    }
    hipLaunchKernelGGL(search_sample_kernel, dim3((unsigned)blocks), dim3(SEARCH_THREADS), 0, (hipStream_t)stream, G, L, R, mean, std, lo,
                       hi, seed, generation, gains);
    return check_launch(who);
}

extern "C" int avd_search_refit_f32(int G, int L, int R, int n_elite, float alpha, const float* gains, const float* fitness,
                                    const float* min_std, float* mean, float* std, float* best_gains, float* best_fitness,
                                    int32_t* best_gen, int generation, int32_t* elite_idx, float* history_row, void* stream) {
    const char* who = "avd_search_refit_f32";
    AVD_REQUIRE(gains && fitness && min_std && mean && std && best_gains && best_fitness && best_gen && elite_idx && history_row,
                "%s: null pointer", who);
    AVD_REQUIRE(G >= 1 && G <= SEARCH_MAX_G, "%s: G=%d (G must be 1..%d)", who, G, SEARCH_MAX_G);
    AVD_REQUIRE(L >= 1 && L <= AVD_MAX_L, "%s: L=%d (L must be 1..%d)", who, L, AVD_MAX_L);
    AVD_REQUIRE(R == 1 || R == L, "%s: R=%d (R must be 1, tied rows, or L=%d, one row per vehicle)", who, R, L);
    AVD_REQUIRE(n_elite >= 1 && n_elite <= G, "%s: n_elite=%d (n_elite must be 1..G=%d)", who, n_elite, G);
    AVD_REQUIRE(alpha > 0.f && alpha <= 1.f, "%s: alpha=%g (alpha must be in (0, 1])", who, (double)alpha);
    AVD_REQUIRE(generation >= 0, "%s: generation=%d (generation must be >= 0: -1 in best_gen means none yet)", who, generation);
    hipLaunchKernelGGL(search_rank_kernel, dim3((G + RANK_CANDS - 1) / RANK_CANDS), dim3(SEARCH_THREADS), 0, (hipStream_t)stream, G,
                       n_elite, fitness, elite_idx);
    const int rc = check_launch(who);
    if (rc != AVD_OK) return rc;
    RefitArgs a;
    a.G = G, a.L = L, a.R = R, a.n_elite = n_elite, a.alpha = alpha, a.gains = gains, a.fitness = fitness, a.min_std = min_std;
    a.mean = mean, a.std = std, a.best_gains = best_gains, a.best_fitness = best_fitness, a.best_gen = best_gen;
    a.generation = generation, a.elite_idx = elite_idx, a.history_row = history_row;
    hipLaunchKernelGGL(search_refit_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    return check_launch(who);
}
