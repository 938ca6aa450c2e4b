// Scenario evaluator for gfx950: G groups (one platoon's weight sets each) x K cases (a start state and a leader-input row each) of the
// evaluator rollout (eval.hip) in ONE launch, with per-vehicle control metrics reduced on the device.
//
// One 256-thread workgroup per (group, block of RB cases): grid G x ceil(K / RB), no communication between workgroups, no spin-wait.
// Every case of a group reads the SAME weights, so per step and model each thread loads each weight element it owns once and applies
// it to all RB rows of its block: acc[r] = fmaf(x[r][k], w, acc[r]). Per row the k split, the fmaf order and the reduction tree are
// those of gemv_relu / bn_apply / block_dot (learn_common.h), so row r's actor outputs -- and with the shared platoon step
// (eval_common.h) its counters -- are bit-identical to eval_rollout_kernel's, while the weight bytes streamed drop RB-fold.
//
// Activations live in LDS transposed, [k][RB]: a thread's RB operands of one k are RB consecutive floats (ds_read_b128 for RB % 4 == 0),
// read as a broadcast by every lane of a wave that works on the same k range.
//
// Rows >= K of the tail block are computed on a zero state in LDS only: they read no start state or leader input and write nothing.
//
// The DISTURBED variant (avd_eval_cases_dist_f32) is the same kernel text with one trailing DistArgs argument: per case a sensor-noise
// level, a V2V delay and loss rate on the communicated 4th state, and the true plant's matrices. The actors then read an OBSERVED
// state; the platoon step, the reward and the metrics keep the true one (the vehicle threads' registers). Without that argument the
// kernel is the nominal one: same parameter list, same code.
#include <float.h>

#include "eval_common.h"

namespace avd {

constexpr int CASES_LDS_SHARED = 24 * AVD_MAX_L;                  // sA, sB, sC (floats), one copy per workgroup
constexpr int CASES_LDS_ROW = 11 * AVD_MAX_L + NTHREADS;          // per row: xin, xs, raw, chain, negr, part (floats); + H1 + H2
// A vehicle's block in LDS, disturbed only: its case's A, B, C (24), its V2V ring, the last received value, its case's scalars (sigma
// (3), delay, drop_q, seed (2)), one float of padding: an odd stride puts neighbouring vehicles on different banks. One block per
// vehicle, the scalars repeated, so that a vehicle thread addresses all of it from one base register.
constexpr int DIST_HIST = 24, DIST_RECV = DIST_HIST + EVAL_RING, DIST_PAR = DIST_RECV + 1, DIST_VEH = DIST_PAR + 7 + 1;
static_assert(DIST_VEH % 2 == 1, "odd stride");
constexpr int DIST_LDS_ROW = DIST_VEH * AVD_MAX_L;                // per row

struct CasesArgs {
    avd_mlp_layout lay;
    const avd_env_consts* cst;
    int G, K, L, M, T, x_stride, n_sets;
    const float* theta;
    const float* stats;
    const int32_t* set_base;  // [G]
    const float* x0;          // [K][L][4]
    const float* prev_a0;     // [K][L]
    const float* leader;      // [K][T]
    float high, lo, hi, inv_dt;
    float* counters;          // [G][K][M]
    float* metrics;           // [G][K][L][AVD_EVAL_NMETRIC] or null
};

// the RB row operands of one k: xT[k][0..RB)
template <int RB>
__device__ __forceinline__ void load_rows(const float* p, float (&x)[RB]) {
    if constexpr (RB % 4 == 0) {
#pragma unroll
        for (int r = 0; r < RB; r += 4) {
            const float4 v = *(const float4*)(p + r);
            x[r] = v.x, x[r + 1] = v.y, x[r + 2] = v.z, x[r + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int r = 0; r < RB; ++r) x[r] = p[r];
    }
}

// gemv_relu (learn_common.h) for RB rows: yT[n][r] = relu(sum_k xT[k][r] * W[k][n] + b[n]); part is [RB][NTHREADS]. UNROLL_K is how
// many k are in flight (registers against latency hiding): it does not touch the order of a row's sum.
// 16 rows: two k in flight keep the kernel at 146 VGPRs (3 waves per SIMD)
template <int RB, int UNROLL_K = (RB >= 16 ? 2 : 4)>
__device__ __forceinline__ void gemv_relu_rows(const float* xT, int K, const float* __restrict__ W, const float* __restrict__ b, int N,
                                               float* part, float* yT) {
    const int cols = N < NTHREADS ? N : NTHREADS;
    const int ksplit = NTHREADS / cols;
    for (int n0 = 0; n0 < N; n0 += cols) {
        const int n = n0 + (threadIdx.x % cols);
        const int kh = threadIdx.x / cols;
        float acc[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = 0.f;
        if (kh < ksplit && n < N) {
            const int kb = (K * kh) / ksplit, ke = (K * (kh + 1)) / ksplit;
#pragma unroll UNROLL_K
            for (int k = kb; k < ke; ++k) {
                const float w = W[(long)k * N + n];
                float x[RB];
                load_rows<RB>(xT + k * RB, x);
#pragma unroll
                for (int r = 0; r < RB; ++r) acc[r] = fmaf(x[r], w, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) part[r * NTHREADS + threadIdx.x] = acc[r];
        __syncthreads();
        if (threadIdx.x < cols && n < N) {
            const float bn = b[n];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                float sum = bn;
                for (int h = 0; h < ksplit; ++h) sum += part[r * NTHREADS + h * cols + threadIdx.x];
                yT[n * RB + r] = fmaxf(sum, 0.f);
            }
        }
        __syncthreads();
    }
}

// bn_apply (learn_common.h) for RB rows: the coefficients are formed once per k
template <int RB>
__device__ __forceinline__ void bn_apply_rows(float* yT, int n, const float* __restrict__ g, const float* __restrict__ be,
                                              const float* __restrict__ mm, const float* __restrict__ mv) {
    for (int k = threadIdx.x; k < n; k += NTHREADS) {
        const float iv = (1.0f / sqrtf(mv[k] + BN_EPS)) * g[k];
#pragma unroll
        for (int r = 0; r < RB; ++r) yT[k * RB + r] = fmaf(yT[k * RB + r], iv, be[k] - mm[k] * iv);
    }
}

// block_dot (learn_common.h) for RB rows: out[r] = sum_k xT[k][r] * w[k * wstride] in part[r * NTHREADS + 0..3] (the four waves'
// partial sums, to be added in wave order); one barrier, the caller adds and synchronizes
template <int RB>
__device__ __forceinline__ void block_dot_rows(const float* xT, const float* __restrict__ w, int wstride, int n, float* part) {
    float acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = 0.f;
    for (int k = threadIdx.x; k < n; k += NTHREADS) {
        const float wk = w[(long)k * wstride];
        float x[RB];
        load_rows<RB>(xT + k * RB, x);
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = fmaf(x[r], wk, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[r] += __shfl_xor(acc[r], o);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int r = 0; r < RB; ++r) part[r * NTHREADS + (threadIdx.x >> 6)] = acc[r];
    }
    __syncthreads();
}

// Where a frequency sweep's ten sums per vehicle live between steps: in registers where the instantiation keeps its waves per SIMD with
// them (the nominal 16-row kernel, whose 53.7 KB of LDS at the reference widths leave no room for 10 KB more beside three workgroups per
// CU), else in LDS as [AVD_EVAL_NSPEC][RB * AVD_MAX_L], a vehicle thread's own column (no barrier, no bank conflict)
constexpr bool spec_in_lds(int rb, bool dist) { return dist || rb < 16; }
constexpr int SPEC_LDS_ROW = AVD_EVAL_NSPEC * AVD_MAX_L;  // per row

// D is empty (the nominal kernel: parameter list and code as before the disturbed variant existed), one DistArgs, one ResArgs (a
// residual policy: the plant input is residual_law on the row's xs entry -- under DistArgs the observation) or a DistArgs then a ResArgs;
// a FreqArgs last adds the single-bin Fourier sums of a frequency sweep (the vehicle threads' alone)
template <int RB, class... D>
__global__ __launch_bounds__(NTHREADS) void eval_cases_kernel(const CasesArgs a, const D... dist) {
#pragma clang fp contract(off)
    constexpr bool DIST = pack_has<DistArgs, D...>, RES = pack_has<ResArgs, D...>, FREQ = pack_has<FreqArgs, D...>;
    constexpr bool SPEC_LDS = FREQ && spec_in_lds(RB, DIST);
    constexpr int UK = RB >= 16 || (DIST && RB >= 8) ? 2 : 4;  // disturbed, 8 rows: 170 VGPRs with four k in flight, 2 waves per SIMD
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const avd_mlp_layout& L = a.lay;
    const int tid = threadIdx.x, nv = a.L, g = blockIdx.x, k0 = blockIdx.y * RB;
    const int nrows = (a.K - k0) < RB ? (a.K - k0) : RB;  // rows of this block that are cases (>= 1 by the grid)
    float* sA = smem;                               // [L][16]
    float* sB = sA + 16 * AVD_MAX_L;                // [L][4]
    float* sC = sB + 4 * AVD_MAX_L;                 // [L][4]
    float* xs = sC + 4 * AVD_MAX_L;                 // [RB][4 * AVD_MAX_L] the actors' input: the platoon states (disturbed: as observed)
    float* xinT = xs + RB * 4 * AVD_MAX_L;          // [S][RB] one model's observation, transposed
    float* raw = xinT + RB * 4 * AVD_MAX_L;         // [RB][AVD_MAX_L] actor outputs, vehicle order (m * A + a)
    float* chain = raw + RB * AVD_MAX_L;            // [RB][AVD_MAX_L]
    float* negr = chain + RB * AVD_MAX_L;           // [RB][AVD_MAX_L]
    float* part = negr + RB * AVD_MAX_L;            // [RB][NTHREADS]
    float* h1T = part + RB * NTHREADS;              // [H1][RB]
    float* h2T = h1T + RB * L.H1;                   // [H2][RB]
    float* vdat = h2T + RB * L.H2;                  // disturbed: [RB][AVD_MAX_L][DIST_VEH], see DIST_VEH. The scalars stay out of the
                                                    // registers the forward needs: each step's observation phase reads them back
    float* spec = vdat + (DIST ? RB * DIST_LDS_ROW : 0) + tid;  // frequency sweep, SPEC_LDS: this vehicle thread's column of the sums
    const int row = tid / nv, v = tid - row * nv;   // vehicle threads: RB * L <= NTHREADS (host check)
    const bool veh = tid < RB * nv;
    const bool live = veh && row < nrows;           // a vehicle of a real case: the only threads that touch x0 / leader / the outputs
    const long cas = (long)g * a.K + k0 + row;      // (group, case) index of this thread's row
    const int base = a.set_base[g];
    if (base < 0 || base + a.M > a.n_sets) {  // uniform per workgroup: nothing read
        if (live) {
            if (v < a.M) a.counters[cas * a.M + v] = __builtin_nanf("");
            if (a.metrics)
                for (int i = 0; i < AVD_EVAL_NMETRIC; ++i) a.metrics[(cas * nv + v) * AVD_EVAL_NMETRIC + i] = __builtin_nanf("");
            if constexpr (FREQ)
                for (int i = 0; i < AVD_EVAL_NSPEC; ++i)
                    pack_get<FreqArgs>(dist...).spectrum[(cas * nv + v) * AVD_EVAL_NSPEC + i] = __builtin_nanf("");
        }
        return;
    }
    const avd_env_consts* cst = a.cst;
    if constexpr (DIST) {
        const DistArgs& da = pack_get<DistArgs>(dist...);
        for (int i = tid; i < RB * nv * 24; i += NTHREADS) {
            const int r = i / (nv * 24), j = i - r * (nv * 24), vi = j / 24, e = j - vi * 24;
            vdat[(r * AVD_MAX_L + vi) * DIST_VEH + e] = (da.abc && r < nrows) ? da.abc[(long)(k0 + r) * nv * 24 + j]
                                          : e < 16              ? cst->A[vi][e]
                                          : e < 20              ? cst->B[vi][e - 16]
                                                                : cst->C[vi][e - 20];
        }
        if (veh) {  // the case's disturbance; rows beyond the tail keep the null one
            const long k = k0 + row;
            float* p = vdat + (row * AVD_MAX_L + v) * DIST_VEH + DIST_PAR;
            const uint64_t seed = live ? da.noise_seed[k] : 0;
            p[0] = live ? da.sigma[k * 3] : 0.f, p[1] = live ? da.sigma[k * 3 + 1] : 0.f, p[2] = live ? da.sigma[k * 3 + 2] : 0.f;
            // (the host refuses delays outside the ring; the mask keeps any value inside it)
            p[3] = __int_as_float(live ? (da.delay[k] & (EVAL_RING - 1)) : 0);
            p[4] = __uint_as_float(live ? da.drop_q[k] : 0u);
            p[5] = __uint_as_float((uint32_t)seed), p[6] = __uint_as_float((uint32_t)(seed >> 32));
        }
    } else {
        for (int i = tid; i < nv * 16; i += NTHREADS) sA[i] = cst->A[i >> 4][i & 15];
        for (int i = tid; i < nv * 4; i += NTHREADS) sB[i] = cst->B[i >> 2][i & 3], sC[i] = cst->C[i >> 2][i & 3];
    }
    for (int i = tid; i < RB * 4 * AVD_MAX_L; i += NTHREADS) xs[i] = 0.f;
    __syncthreads();
    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
    float pa = 0.f, cnt = 0.f;
    VehMetrics met;
    VehSpectrum spc;
    if constexpr (SPEC_LDS)
        if (veh) spc.store(spec, RB * AVD_MAX_L);  // zeros
    const float* leader = a.leader + (long)(k0 + (live ? row : 0)) * a.T;
    if (live) {
        const float* x0 = a.x0 + ((long)(k0 + row) * nv + v) * 4;
        xv = make_float4(x0[0], x0[1], x0[2], x0[3]);
        pa = a.prev_a0[(long)(k0 + row) * nv + v];
    }
    if constexpr (DIST) {
        if (veh) {
            float* hist = vdat + (row * AVD_MAX_L + v) * DIST_VEH + DIST_HIST;
            for (int j = 0; j <= EVAL_RING; ++j) hist[j] = xv.w;  // steps before the first, and the last received value: x0's
        }
    } else {
        if (veh) ((float4*)(xs + row * 4 * AVD_MAX_L))[v] = xv;
    }
    __syncthreads();
    const int S = L.S, A = L.A, M = a.M;
    for (int t = 0; t < a.T; ++t) {
        if constexpr (DIST) {
            // ---- what the actors see of the true pre-step state xv ----
            if (veh) {
                float* vd = vdat + (row * AVD_MAX_L + v) * DIST_VEH;
                const float* p = vd + DIST_PAR;
                const float sg_ep = p[0], sg_ev = p[1], sg_a = p[2];
                const int dly = __float_as_int(p[3]);
                const uint32_t dq = __float_as_uint(p[4]);
                const uint64_t nseed = (uint64_t)__float_as_uint(p[5]) | ((uint64_t)__float_as_uint(p[6]) << 32);
                float* hist = vd + DIST_HIST;  // this vehicle's ring (its own thread's alone), then its last received value
                float4 ob = xv;
                ob.w = v2v_link<1>(hist, hist[EVAL_RING], xv.w, t, dly, dq, nseed, (uint32_t)v);
                observe_noise(ob, xv, sg_ep, sg_ev, sg_a, nseed, (uint64_t)t, (uint32_t)v, STREAM_EVAL_OBS);
                ((float4*)(xs + row * 4 * AVD_MAX_L))[v] = ob;
            }
            __syncthreads();
        }
        // ---- actor forward of each model, RB rows at once ----
        for (int m = 0; m < M; ++m) {
            const float* th = a.theta + (long)(base + m) * L.theta_size;
            const float* st = a.stats + (long)(base + m) * L.stats_size;
            for (int i = tid; i < RB * S; i += NTHREADS) {
                const int r = i / S, s = i - r * S;
                xinT[s * RB + r] = xs[r * 4 * AVD_MAX_L + m * a.x_stride + s];
            }
            __syncthreads();
            gemv_relu_rows<RB, UK>(xinT, S, th + L.aW1, th + L.ab1, L.H1, part, h1T);
            bn_apply_rows<RB>(h1T, L.H1, th + L.ag1, th + L.abe1, st + L.amm1, st + L.amv1);
            __syncthreads();
            gemv_relu_rows<RB, UK>(h1T, L.H1, th + L.aW2, th + L.ab2, L.H2, part, h2T);
            bn_apply_rows<RB>(h2T, L.H2, th + L.ag2, th + L.abe2, st + L.amm2, st + L.amv2);
            __syncthreads();
            for (int k = 0; k < A; ++k) {
                block_dot_rows<RB>(h2T, th + L.aW3 + k, A, L.H2, part);
                if (tid < RB) {
                    const float* p = part + tid * NTHREADS;
                    const float z = (p[0] + p[1] + p[2] + p[3]) + th[L.ab3 + k];
                    raw[tid * AVD_MAX_L + m * A + k] = tanhf(z) * a.high;
                }
                __syncthreads();
            }
        }
        // ---- noise-free policy, platoon step ----
        float uu = 0.f;
        VehStep vs = {};
        float2 cs = make_float2(0.f, 0.f);
        if constexpr (FREQ)  // this step's basis pair: in flight over the barrier below
            if (live) cs = ((const float2*)pack_get<FreqArgs>(dist...).basis)[(long)(k0 + row) * a.T + t];
        if (veh) {
            uu = fminf(fmaxf(raw[row * AVD_MAX_L + v], a.lo), a.hi);  // np.clip (ddpgagent.py:27)
            if constexpr (RES) {  // traces, reward and metrics below take the plant's input
                const ResArgs& b = pack_get<ResArgs>(dist...);
                uu = residual_law(((const float4*)b.gains)[v], ((const float4*)(xs + row * 4 * AVD_MAX_L))[v], cst->model_a != 0, b.scale, uu,
                                  a.lo, a.hi);
            }
            const float* Av = DIST ? vdat + (row * AVD_MAX_L + v) * DIST_VEH : sA + v * 16;  // this vehicle's A, B (disturbed: its case's)
            vs = veh_step_pre(cst, Av, DIST ? Av + 16 : sB + v * 4, xv, uu);
            chain[row * AVD_MAX_L + v] = vs.chain;
        }
        __syncthreads();
        if (veh) {
            const float exog = (v == 0) ? (live ? leader[t] : 0.f) : chain[row * AVD_MAX_L + v - 1];
            float4 xn;
            const float* Bv = DIST ? vdat + (row * AVD_MAX_L + v) * DIST_VEH + 16 : sB + v * 4;
            const float nr = veh_step_post(cst, vs, Bv, DIST ? Bv + 4 : sC + v * 4, xv, pa, uu, exog, xn);
            if (M == nv) cnt = cnt + nr;  // counters += env.reward[0]
            else negr[row * AVD_MAX_L + v] = nr;
            met.step(cst, xv, xn, pa, uu, a.inv_dt, t);
            if constexpr (SPEC_LDS) VehSpectrum::step_lds(spec, RB * AVD_MAX_L, xn, uu, cs);
            else if constexpr (FREQ) spc.step(xn, uu, cs);
            pa = xv.z;  // prev_x <- x
            xv = xn;
            if constexpr (!DIST) ((float4*)(xs + row * 4 * AVD_MAX_L))[v] = xn;
        }
        __syncthreads();
        if (M != nv && veh && v == 0) {  // centralized: counters += reward_mean = (1/L) * sum in vehicle order (env.hip)
            float s = 0.f;
            for (int k = 0; k < nv; ++k) s = s + negr[row * AVD_MAX_L + k];
            cnt = cnt + (1.0f / (float)nv) * s;
        }
    }
    if (live) {
        if (v < M) a.counters[cas * M + v] = cnt;
        if (a.metrics) met.store(a.metrics + (cas * nv + v) * AVD_EVAL_NMETRIC, xv);
        if constexpr (FREQ) {
            if constexpr (SPEC_LDS) spc.load(spec, RB * AVD_MAX_L);
            spc.store(pack_get<FreqArgs>(dist...).spectrum + (cas * nv + v) * AVD_EVAL_NSPEC);
        }
    }
}

// the block sizes instantiated, largest first
constexpr int CASES_RB[] = {16, 8, 4, 1};
// The disturbed kernel's: its 24 + 16 more floats per vehicle slot put 16 rows at 94.7 KB of LDS at the reference widths -- one
// workgroup per CU where the nominal kernel keeps three. 8 rows take 48.1 KB and keep the three.
constexpr int DIST_RB[] = {8, 4, 1};

template <int N>
int pick_block(const int (&sizes)[N], int K, int L) {
    int rb = sizes[0];
    for (int c : sizes)  // the smallest block that holds all K cases (no idle rows beyond the tail), else the largest
        if (c >= K && c * L <= NTHREADS) rb = c;
    return rb;
}

// The one dispatch from a block size to its kernel instantiation: CASES_RB's sizes, with a DistArgs in the pack DIST_RB's
template <class... D>
int launch_cases(const char* who, int rb, const CasesArgs& a, size_t lds, hipStream_t stream, const D&... dist) {
    const auto go = [&](auto size) {
        constexpr int RB = decltype(size)::value;
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute((const void*)eval_cases_kernel<RB, D...>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((eval_cases_kernel<RB, D...>), dim3(a.G, (a.K + RB - 1) / RB), dim3(NTHREADS), lds, stream, a, dist...);
        return check_launch(who);
    };
    if constexpr (!pack_has<DistArgs, D...>)
        if (rb == 16) return go(std::integral_constant<int, 16>{});
    switch (rb) {
        case 8: return go(std::integral_constant<int, 8>{});
        case 4: return go(std::integral_constant<int, 4>{});
        default: return go(std::integral_constant<int, 1>{});
    }
}

// Every cases entry point: the checks, the block size, the argument block and the launch. dist: the disturbed variant's tables, or
// null (the nominal kernel); res: a residual policy's law, or null; freq: a frequency sweep's basis and spectrum, or null.
int cases_launch(const char* who, const DistArgs* dist, const ResArgs* res, const FreqArgs* freq, const avd_mlp_layout* lay, const avd_env_consts* d_consts, int G,
                 int K, int L, int M, int T, const float* theta, const float* stats, int n_sets, const int32_t* set_base, const float* x0,
                 const float* prev_a0, const float* leader, float high, float lo, float hi, float sample_rate, float* counters,
                 float* metrics, void* stream) {
    AVD_REQUIRE(lay && d_consts, "%s: null layout or constants", who);
    AVD_REQUIRE(L >= 1 && L <= AVD_MAX_L, "%s: L=%d (L must be 1..%d)", who, L, AVD_MAX_L);
    AVD_REQUIRE(M == L || M == 1, "%s: M=%d (M must be L=%d, decentralized, or 1, centralized)", who, M, L);
    AVD_REQUIRE(G >= 1 && K >= 1 && T >= 1, "%s: G=%d K=%d T=%d (all must be >= 1)", who, G, K, T);
    AVD_REQUIRE(n_sets >= M, "%s: n_sets=%d (need n_sets >= M=%d)", who, n_sets, M);
    AVD_REQUIRE(theta && stats && set_base && x0 && prev_a0 && leader && counters, "%s: null pointer", who);
    AVD_REQUIRE(sample_rate > 0.f, "%s: sample_rate=%g", who, (double)sample_rate);
    // the model shape the platoon implies: M * A = L actions, observations of 4L / M floats (the first S read)
    const int x_stride = 4 * L / M;
    AVD_REQUIRE(lay->A * M == L && lay->S <= x_stride && lay->S >= 1,
                "%s: layout S=%d A=%d does not fit L=%d M=%d (need A * M == L, S <= %d)", who, lay->S, lay->A, L, M, x_stride);
    AVD_REQUIRE(lay->H1 > 0 && lay->H2 > 0, "%s: layout H1=%d H2=%d", who, lay->H1, lay->H2);
    const int rb = dist ? pick_block(DIST_RB, K, L) : pick_block(CASES_RB, K, L);
    const size_t row = (size_t)CASES_LDS_ROW + (dist ? DIST_LDS_ROW : 0) + (freq && spec_in_lds(rb, dist != nullptr) ? SPEC_LDS_ROW : 0) +
                       lay->H1 + lay->H2;
    const size_t lds = sizeof(float) * ((size_t)CASES_LDS_SHARED + (size_t)rb * row);
    if (lds > 160 * 1024) {
        set_error("%s: hidden sizes need %zu B of LDS for blocks of %d cases (> 160 KiB)", who, lds, rb);
        return AVD_E_UNSUPPORTED;
    }
    if ((long)((K + rb - 1) / rb) > 65535) {
        set_error("%s: K=%d cases in blocks of %d exceed the grid's second dimension", who, K, rb);
        return AVD_E_UNSUPPORTED;
    }
    if (dist) AVD_REQUIRE(dist->sigma && dist->delay && dist->drop_q && dist->noise_seed, "%s: null disturbance table (only abc may be null)", who);
    if (res)
        if (const int rc = residual_check(who, res->gains, res->scale, M, L)) return rc;
    if (freq)
        if (const int rc = freq_check(who, *freq)) return rc;
    CasesArgs a;
    a.lay = *lay, a.cst = d_consts, a.G = G, a.K = K, a.L = L, a.M = M, a.T = T, a.x_stride = x_stride, a.n_sets = n_sets;
    a.theta = theta, a.stats = stats, a.set_base = set_base, a.x0 = x0, a.prev_a0 = prev_a0, a.leader = leader;
    a.high = high, a.lo = lo, a.hi = hi;
    a.inv_dt = 1.0f / sample_rate;  // host float32 division, as avd_eval_rollout_f32 forms it
    a.counters = counters, a.metrics = metrics;
    const hipStream_t s = (hipStream_t)stream;
    if (freq) {  // the same packs with the FreqArgs last
        if (dist && res) return launch_cases(who, rb, a, lds, s, *dist, *res, *freq);
        if (dist) return launch_cases(who, rb, a, lds, s, *dist, *freq);
        if (res) return launch_cases(who, rb, a, lds, s, *res, *freq);
        return launch_cases(who, rb, a, lds, s, *freq);
    }
    if (dist && res) return launch_cases(who, rb, a, lds, s, *dist, *res);
    if (dist) return launch_cases(who, rb, a, lds, s, *dist);
    if (res) return launch_cases(who, rb, a, lds, s, *res);
    return launch_cases(who, rb, a, lds, s);
}

}  // namespace avd

using namespace avd;

extern "C" int avd_eval_cases_block(int K, int L) {
    AVD_REQUIRE(K >= 1, "avd_eval_cases_block: K=%d (K must be >= 1)", K);
    AVD_REQUIRE(L >= 1 && L <= AVD_MAX_L, "avd_eval_cases_block: L=%d (L must be 1..%d)", L, AVD_MAX_L);
    return pick_block(CASES_RB, K, L);
}

extern "C" int avd_eval_cases_f32(const avd_mlp_layout* lay, const avd_env_consts* d_consts, int G, int K, int L, int M, int T,
                                  const float* theta, const float* stats, int n_sets, const int32_t* set_base, const float* x0,
                                  const float* prev_a0, const float* leader, float high, float lo, float hi, float sample_rate,
                                  float* counters, float* metrics, void* stream) {
    return cases_launch("avd_eval_cases_f32", nullptr, nullptr, nullptr, lay, d_consts, G, K, L, M, T, theta, stats, n_sets, set_base, x0, prev_a0,
                        leader, high, lo, hi, sample_rate, counters, metrics, stream);
}

extern "C" int avd_eval_cases_dist_block(int K, int L) {
    AVD_REQUIRE(K >= 1, "avd_eval_cases_dist_block: K=%d (K must be >= 1)", K);
    AVD_REQUIRE(L >= 1 && L <= AVD_MAX_L, "avd_eval_cases_dist_block: L=%d (L must be 1..%d)", L, AVD_MAX_L);
    return pick_block(DIST_RB, K, L);
}

extern "C" int avd_eval_cases_dist_check(int K, const float* sigma, const int32_t* delay, const uint32_t* drop_q) {
    const char* who = "avd_eval_cases_dist_check";
    AVD_REQUIRE(K >= 1, "%s: K=%d (K must be >= 1)", who, K);
    AVD_REQUIRE(sigma && delay && drop_q, "%s: null pointer", who);
    for (int k = 0; k < K; ++k) {
        for (int c = 0; c < 3; ++c)
            AVD_REQUIRE(sigma[k * 3 + c] >= 0.f && sigma[k * 3 + c] <= FLT_MAX, "%s: sigma[%d][%d]=%g (must be finite and >= 0)", who, k, c,
                        (double)sigma[k * 3 + c]);
        AVD_REQUIRE(delay[k] >= 0 && delay[k] <= AVD_EVAL_MAX_DELAY, "%s: delay[%d]=%d (must be 0..%d)", who, k, delay[k],
                    AVD_EVAL_MAX_DELAY);
        AVD_REQUIRE(drop_q[k] <= (1u << 24), "%s: drop_q[%d]=%u (must be <= 2^24 = %u)", who, k, drop_q[k], 1u << 24);
    }
    return AVD_OK;
}

extern "C" int avd_eval_cases_dist_f32(const avd_mlp_layout* lay, const avd_env_consts* d_consts, int G, int K, int L, int M, int T,
                                       const float* theta, const float* stats, int n_sets, const int32_t* set_base, const float* x0,
                                       const float* prev_a0, const float* leader, float high, float lo, float hi, float sample_rate,
                                       const float* sigma, const int32_t* delay, const uint32_t* drop_q, const uint64_t* noise_seed,
                                       const float* abc, float* counters, float* metrics, void* stream) {
    const DistArgs d = {sigma, delay, drop_q, noise_seed, abc};
    return cases_launch("avd_eval_cases_dist_f32", &d, nullptr, nullptr, lay, d_consts, G, K, L, M, T, theta, stats, n_sets, set_base, x0, prev_a0,
                        leader, high, lo, hi, sample_rate, counters, metrics, stream);
}

// The scenario evaluator for a residual policy, nominal (all five disturbance tables null) or disturbed (only abc may be null, with
// avd_eval_cases_dist_f32's block sizes): the actors' clipped action r enters the plant as residual_law(gains row, what the vehicle
// observes, scale, r). Decentralized agents only.
extern "C" int avd_eval_cases_res_f32(const avd_mlp_layout* lay, const avd_env_consts* d_consts, int G, int K, int L, int M, int T,
                                      const float* theta, const float* stats, int n_sets, const int32_t* set_base, const float* x0,
                                      const float* prev_a0, const float* leader, float high, float lo, float hi, float sample_rate,
                                      const float* sigma, const int32_t* delay, const uint32_t* drop_q, const uint64_t* noise_seed,
                                      const float* abc, const float* d_gains, float scale, float* counters, float* metrics, void* stream) {
    const char* who = "avd_eval_cases_res_f32";
    const bool dist = sigma || delay || drop_q || noise_seed || abc;  // which variant: a mix of null and non-null tables is refused first
    AVD_REQUIRE(!dist || (sigma && delay && drop_q && noise_seed),
                "%s: null disturbance table (all five null: the nominal plant and a perfect observation; otherwise only abc may be null)", who);
    const DistArgs d = {sigma, delay, drop_q, noise_seed, abc};
    const ResArgs r = {d_gains, scale};
    return cases_launch(who, dist ? &d : nullptr, &r, nullptr, lay, d_consts, G, K, L, M, T, theta, stats, n_sets, set_base, x0, prev_a0, leader, high,
                        lo, hi, sample_rate, counters, metrics, stream);
}

// The scenario evaluator of a frequency sweep: avd_eval_cases_res_f32's arguments (all five disturbance tables null: the nominal plant;
// d_gains null: no residual law, scale unread) plus the per-case basis table and the spectrum output.
extern "C" int avd_eval_cases_freq_f32(const avd_mlp_layout* lay, const avd_env_consts* d_consts, int G, int K, int L, int M, int T,
                                       const float* theta, const float* stats, int n_sets, const int32_t* set_base, const float* x0,
                                       const float* prev_a0, const float* leader, float high, float lo, float hi, float sample_rate,
                                       const float* sigma, const int32_t* delay, const uint32_t* drop_q, const uint64_t* noise_seed,
                                       const float* abc, const float* d_gains, float scale, float* counters, float* metrics,
                                       const float* basis, float* spectrum, void* stream) {
    const char* who = "avd_eval_cases_freq_f32";
    const bool dist = sigma || delay || drop_q || noise_seed || abc;
    AVD_REQUIRE(!dist || (sigma && delay && drop_q && noise_seed),
                "%s: null disturbance table (all five null: the nominal plant and a perfect observation; otherwise only abc may be null)", who);
    const DistArgs d = {sigma, delay, drop_q, noise_seed, abc};
    const ResArgs r = {d_gains, scale};
    const FreqArgs f = {basis, spectrum};
    return cases_launch(who, dist ? &d : nullptr, d_gains ? &r : nullptr, &f, lay, d_consts, G, K, L, M, T, theta, stats, n_sets, set_base, x0,
                        prev_a0, leader, high, lo, hi, sample_rate, counters, metrics, stream);
}
