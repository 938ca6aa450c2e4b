// Evaluator rollout for gfx950: a whole noise-free, deterministic-start episode (workers/evaluator.py:47-95, 145) for R
// rollouts in ONE launch.
//
// One 256-thread workgroup per rollout loops over the T steps on its own: per step the actor forward of each of the M
// models, the noise-free policy clip, the platoon step and the float32 episodic reward counters. There is no
// communication between workgroups (no grid barrier, no spin-wait): every workgroup ends after T steps.
//
// Every operation is the one avddpg_amd/evaluator.py:run issues as separate launches, in the same order and with the same
// float32 rounding, so rollout r is bit-identical to evaluator.run on its weight sets, start state and leader inputs:
//   * actor forward  : mlp_rows_kernel's mode-0 sequence (gemv_relu / bn_apply / block_dot of learn_common.h, same K split
//                      and reduction tree), then tanhf(z) * high;
//   * policy         : policy_kernel without noise, fminf(fmaxf(a, lo), hi);
//   * platoon step   : env_step_kernel's arithmetic (no FMA contraction, the reference's operation order);
//   * counters       : one IEEE add per step of the vehicle's reward (decentralized) or of the platoon-mean reward
//                      (centralized), as `counters += env.reward[0]` / `env.reward_mean`;
//   * jerk trace     : (x_before[2] - prev_a_before) * (1 / sample_rate) -- torch's float32 tensor / Python-scalar division
//                      is a multiplication by the float32 reciprocal (VecPlatoon.get_jerk_from).
#include "eval_common.h"

namespace avd {

constexpr int EVAL_LDS_FIXED = 35 * AVD_MAX_L;  // xin, xs, raw, chain, negr, sA, sB, sC (floats)

struct EvalArgs {
    avd_mlp_layout lay;
    const avd_env_consts* cst;
    int R, L, M, T, x_stride, obs_width, n_sets, n_start;
    const float* theta;
    const float* stats;
    const int32_t* set_base;   // [R]
    const float* x0;           // [n_start][L][4]
    const float* prev_a0;      // [n_start][L]
    const float* leader;       // [n_start][T]
    const int32_t* start_idx;  // [R]
    float high, lo, hi, inv_dt;
    float* counters;           // [R][M]
    int n_trace;
    const int32_t* trace_idx;  // [n_trace] rollout indices
    float *tr_states, *tr_actions, *tr_jerks;  // [n_trace][T][L][obs_width], [n_trace][T][L], [n_trace][T][L]
};

// B is empty (the actors alone: parameter list and code as before the residual variant existed) or one ResArgs: the plant, the reward
// and the traces take residual_law(the vehicle's gain row, its state, scale, the actor's clipped action)
template <class... B>
__global__ __launch_bounds__(NTHREADS) void eval_rollout_kernel(const EvalArgs a, const B... res) {
#pragma clang fp contract(off)
    constexpr bool RES = pack_has<ResArgs, B...>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const avd_mlp_layout& L = a.lay;
    const int tid = threadIdx.x, nv = a.L, r = blockIdx.x;
    // the fixed-size platoon buffers first (560 floats: every offset below a multiple of 16 bytes), then the actor's
    // reduction scratch and hidden activations
    float* xin = smem;                     // MAX_S (<= 4 * AVD_MAX_L)
    float* xs = xin + 4 * AVD_MAX_L;       // [L][4] platoon state (the actors' input)
    float* raw = xs + 4 * AVD_MAX_L;       // [L] actor outputs, vehicle order (m * A + a)
    float* chain = raw + AVD_MAX_L;        // [L]
    float* negr = chain + AVD_MAX_L;       // [L]
    float* sA = negr + AVD_MAX_L;          // [L][16]
    float* sB = sA + 16 * AVD_MAX_L;       // [L][4]
    float* sC = sB + 4 * AVD_MAX_L;        // [L][4]
    float* part = sC + 4 * AVD_MAX_L;      // NTHREADS
    float* h1 = part + NTHREADS;           // H1
    float* h2 = h1 + L.H1;                 // H2
    const int base = a.set_base[r], start = a.start_idx[r];
    if (base < 0 || base + a.M > a.n_sets || start < 0 || start >= a.n_start) {  // uniform per workgroup: nothing read
        if (tid < a.M) a.counters[(long)r * a.M + tid] = __builtin_nanf("");
        return;
    }
    int slot = -1;  // this rollout's trace slot (first match), or none
    for (int j = 0; j < a.n_trace; ++j)
        if (a.trace_idx[j] == r) {
            slot = j;
            break;
        }
    const avd_env_consts* cst = a.cst;
    for (int i = tid; i < nv * 16; i += NTHREADS) sA[i] = cst->A[i >> 4][i & 15];
    for (int i = tid; i < nv * 4; i += NTHREADS) sB[i] = cst->B[i >> 2][i & 3], sC[i] = cst->C[i >> 2][i & 3];
    const bool veh = tid < nv;
    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
    float pa = 0.f, cnt = 0.f;
    const float* leader = a.leader + (long)start * a.T;
    if (veh) {
        const float* x0 = a.x0 + ((long)start * nv + tid) * 4;
        xv = make_float4(x0[0], x0[1], x0[2], x0[3]);
        pa = a.prev_a0[(long)start * nv + tid];
        ((float4*)xs)[tid] = xv;
    }
    __syncthreads();
    const int S = L.S, A = L.A, M = a.M, ow = a.obs_width;
    for (int t = 0; t < a.T; ++t) {
        // ---- actor forward of each model (mlp_rows_kernel, mode 0) ----
        for (int m = 0; m < M; ++m) {
            const float* th = a.theta + (long)(base + m) * L.theta_size;
            const float* st = a.stats + (long)(base + m) * L.stats_size;
            if (tid < S) xin[tid] = xs[m * a.x_stride + tid];
            __syncthreads();
            gemv_relu(xin, S, th + L.aW1, th + L.ab1, L.H1, part, h1);
            bn_apply(h1, L.H1, th + L.ag1, th + L.abe1, st + L.amm1, st + L.amv1);
            __syncthreads();
            gemv_relu(h1, L.H1, th + L.aW2, th + L.ab2, L.H2, part, h2);
            bn_apply(h2, L.H2, th + L.ag2, th + L.abe2, st + L.amm2, st + L.amv2);
            __syncthreads();
            for (int k = 0; k < A; ++k) {
                const float z = block_dot(h2, th + L.aW3 + k, A, L.H2, part) + th[L.ab3 + k];
                if (tid == 0) raw[m * A + k] = tanhf(z) * a.high;
            }
        }
        __syncthreads();
        // ---- noise-free policy, platoon step ----
        float uu = 0.f;
        VehStep vs = {};
        if (veh) {
            uu = fminf(fmaxf(raw[tid], a.lo), a.hi);  // np.clip (ddpgagent.py:27)
            if constexpr (RES) {
                const ResArgs& b = pack_get<ResArgs>(res...);
                uu = residual_law(((const float4*)b.gains)[tid], ((const float4*)xs)[tid], cst->model_a != 0, b.scale, uu, a.lo, a.hi);
            }
            vs = veh_step_pre(cst, sA + tid * 16, sB + tid * 4, xv, uu);
            chain[tid] = vs.chain;
        }
        __syncthreads();
        if (veh) {
            const float exog = (tid == 0) ? leader[t] : chain[tid - 1];
            float4 xn;
            const float nr = veh_step_post(cst, vs, sB + tid * 4, sC + tid * 4, xv, pa, uu, exog, xn);
            if (M == nv) cnt = cnt + nr;  // counters += env.reward[0]
            else negr[tid] = nr;
            if (slot >= 0) {
                const long o = ((long)slot * a.T + t) * nv + tid;
                float* so = a.tr_states + o * ow;
                so[0] = xn.x, so[1] = xn.y, so[2] = xn.z;
                if (ow == 4) so[3] = xn.w;
                a.tr_actions[o] = uu;
                a.tr_jerks[o] = (xv.z - pa) * a.inv_dt;
            }
            pa = xv.z;  // prev_x <- x
            xv = xn;
            ((float4*)xs)[tid] = xn;
        }
        __syncthreads();
        if (M != nv && tid == 0) {  // centralized: counters += reward_mean = (1/L) * sum in vehicle order (env.hip)
            float s = 0.f;
            for (int k = 0; k < nv; ++k) s = s + negr[k];
            cnt = cnt + (1.0f / (float)nv) * s;
        }
    }
    if (tid < M) a.counters[(long)r * M + tid] = cnt;
}

}  // namespace avd

using namespace avd;

static int rollout_launch(const char* who, const ResArgs* res, const avd_mlp_layout* lay, const avd_env_consts* d_consts, int R, int L, int M, int T,
                                    const float* theta, const float* stats, int n_sets, const int32_t* set_base, const float* x0,
                                    const float* prev_a0, const float* leader, int n_start, const int32_t* start_idx, float high,
                                    float lo, float hi, float sample_rate, float* counters, int n_trace, const int32_t* trace_idx,
                                    float* tr_states, float* tr_actions, float* tr_jerks, void* stream) {
    AVD_REQUIRE(lay && d_consts, "%s: null layout or constants", who);
    AVD_REQUIRE(L >= 1 && L <= AVD_MAX_L, "%s: L=%d (L must be 1..%d)", who, L, AVD_MAX_L);
    AVD_REQUIRE(M == L || M == 1, "%s: M=%d (M must be L=%d, decentralized, or 1, centralized)", who, M, L);
    AVD_REQUIRE(R >= 1 && T >= 1, "%s: R=%d T=%d (both must be >= 1)", who, R, T);
    AVD_REQUIRE(n_sets >= M && n_start >= 1, "%s: n_sets=%d n_start=%d (need n_sets >= M=%d, n_start >= 1)", who,
                n_sets, n_start, M);
    AVD_REQUIRE(theta && stats && set_base && x0 && prev_a0 && leader && start_idx && counters,
                "%s: null pointer", who);
    AVD_REQUIRE(n_trace >= 0 && (n_trace == 0 || (trace_idx && tr_states && tr_actions && tr_jerks)),
                "%s: n_trace=%d needs trace_idx and the three trace buffers", who, n_trace);
    AVD_REQUIRE(sample_rate > 0.f, "%s: sample_rate=%g", who, (double)sample_rate);
    // the model shape the platoon implies: M * A = L actions, observations of 4L / M floats (the first S read)
    const int x_stride = 4 * L / M;
    AVD_REQUIRE(lay->A * M == L && lay->S <= x_stride && lay->S >= 1,
                "%s: layout S=%d A=%d does not fit L=%d M=%d (need A * M == L, S <= %d)", who, lay->S, lay->A, L, M,
                x_stride);
    AVD_REQUIRE(lay->H1 > 0 && lay->H2 > 0, "%s: layout H1=%d H2=%d", who, lay->H1, lay->H2);
    const size_t lds = sizeof(float) * ((size_t)EVAL_LDS_FIXED + NTHREADS + lay->H1 + lay->H2);
    if (lds > 160 * 1024) {
        set_error("%s: hidden sizes need %zu B of LDS (> 160 KiB)", who, lds);
        return AVD_E_UNSUPPORTED;
    }
    EvalArgs a;
    a.lay = *lay, a.cst = d_consts, a.R = R, a.L = L, a.M = M, a.T = T, a.x_stride = x_stride;
    a.obs_width = lay->S < 4 ? lay->S : 4;  // Vehicle.step returns x[0:num_states] (environment.py:518)
    a.n_sets = n_sets, a.n_start = n_start;
    a.theta = theta, a.stats = stats, a.set_base = set_base, a.x0 = x0, a.prev_a0 = prev_a0, a.leader = leader;
    a.start_idx = start_idx, a.high = high, a.lo = lo, a.hi = hi;
    a.inv_dt = 1.0f / sample_rate;  // host float32 division, as torch forms the reciprocal of a Python-scalar divisor
    a.counters = counters, a.n_trace = n_trace, a.trace_idx = trace_idx;
    a.tr_states = tr_states, a.tr_actions = tr_actions, a.tr_jerks = tr_jerks;
    if (res) {
        if (const int rc = residual_check(who, res->gains, res->scale, M, L)) return rc;
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute((const void*)eval_rollout_kernel<ResArgs>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(eval_rollout_kernel<ResArgs>, dim3(R), dim3(NTHREADS), lds, (hipStream_t)stream, a, *res);
        return check_launch(who);
    }
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute((const void*)eval_rollout_kernel<>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(eval_rollout_kernel<>, dim3(R), dim3(NTHREADS), lds, (hipStream_t)stream, a);
    return check_launch(who);
}

extern "C" int avd_eval_rollout_f32(const avd_mlp_layout* lay, const avd_env_consts* d_consts, int R, int L, int M, int T,
                                    const float* theta, const float* stats, int n_sets, const int32_t* set_base, const float* x0,
                                    const float* prev_a0, const float* leader, int n_start, const int32_t* start_idx, float high,
                                    float lo, float hi, float sample_rate, float* counters, int n_trace, const int32_t* trace_idx,
                                    float* tr_states, float* tr_actions, float* tr_jerks, void* stream) {
    return rollout_launch("avd_eval_rollout_f32", nullptr, lay, d_consts, R, L, M, T, theta, stats, n_sets, set_base, x0, prev_a0, leader,
                          n_start, start_idx, high, lo, hi, sample_rate, counters, n_trace, trace_idx, tr_states, tr_actions, tr_jerks, stream);
}

// The rollout of a residual policy: the actors' clipped action r enters the plant as residual_law(gains row, state, scale, r); the
// action trace holds that plant input. Decentralized agents only.
extern "C" int avd_eval_rollout_res_f32(const avd_mlp_layout* lay, const avd_env_consts* d_consts, int R, int L, int M, int T,
                                        const float* theta, const float* stats, int n_sets, const int32_t* set_base, const float* x0,
                                        const float* prev_a0, const float* leader, int n_start, const int32_t* start_idx, float high,
                                        float lo, float hi, float sample_rate, float* counters, int n_trace, const int32_t* trace_idx,
                                        float* tr_states, float* tr_actions, float* tr_jerks, const float* d_gains, float scale,
                                        void* stream) {
    const ResArgs res = {d_gains, scale};
    return rollout_launch("avd_eval_rollout_res_f32", &res, lay, d_consts, R, L, M, T, theta, stats, n_sets, set_base, x0, prev_a0, leader,
                          n_start, start_idx, high, lo, hi, sample_rate, counters, n_trace, trace_idx, tr_states, tr_actions, tr_jerks, stream);
}
