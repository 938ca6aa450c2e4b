// Split-operand fused shared-weight-set learner ("fsplit"): the same quantity as fset.hip -- Trainer.learn
// (workers/trainer.py:472-508) + the federated mean over the platoons (src/server/federated.py:47-63, 99-118;
// workers/trainer.py:400-431) for agents that SHARE their networks (interfrl, every step federated: trainer.py:121-128) at the
// reference widths 256 / 128 / 48 (src/config.py:112-117) -- but with f32-class results: the reference computes in float32
// (agent/model.py:26-36, 63-83) and single-rounded bf16 operands miss it by 1.7e-2 on the actor gradients (fset.hip).
//
// Every matrix product runs on v_mfma_f32_32x32x16_f16 with BOTH operands carried as fp16 PAIRS x = hi + lo
// (hi = rn16(x), lo = rn16(x - hi): |x - hi - lo| <= 2^-22 |x|, measured worst 2^-23; since r04 no operand is a bf16 pair --
// 2^-17 -- any more), accumulated in f32:
//     A . B  ~=  A_hi . B_hi + A_lo . B_hi + A_hi . B_lo          (the dropped lo . lo term is below the pairs' own residual)
// fp16's 5-bit exponent is handled by exact power-of-two scales folded into f32 constants (SW, SWC per set and net on the static
// second-layer operands; S1 = 64 on the first layers; 2^kg per set on the row factor |g3|, from the maximum the backward heads
// leave: set_gscale), and every conversion that could overflow is watched: *bad -> finalize writes NaN (see F16_OVERFLOW).
// Three structural facts keep this from costing 3x fset.hip:
//   * the output layers are one unit wide, so the second-layer gradient is rank one times a mask:
//         dZ2[row][n] = g3[row] * c3[n] * [z2[row][n] > 0]
//     The mask (with the sign of g3) is EXACT in fp16. The heads write it as one bit per element ("sm", 16 B per row:
//     HeadArgs::sm), and dw / dx / dxa expand it on staging to fp16 +-1 / 0, the sign taken from g3 (mask_chunk16, mask_pair);
//     c3[n] is folded into the other operand (dx: W2c[f][n] = c3[n] W2[f][n], split once per call) or applied at the end (dw: finalize), and
//     |g3[row]| is folded into the first-layer input (dw: relu(W1 (|g| x) + |g| b1) = |g| P1, one MFMA with split operands
//     like every first layer here) or multiplied onto the f32 result (dx). dw and dx then need TWO MFMAs per product, and the
//     heads split nothing on their way out.
//   * second-layer weights are split once per call (prep) and stay in LDS (heads: hi + lo images, 135 / 160 KB, stored in the
//     k order in which a first-layer accumulator tile IS the next MFMA's B operand: no cross-lane exchange of activations)
//     or in registers (dx); only the activations are split on the fly (4 VALU per pair, in the shadow of the MFMAs).
//   * the action gradient of the actor loss needs no dZ2 at all: dmu[row] = g3 sum_n c3[n] [z2 > 0] M[n][row] with
//     M = W2T[:, action features] . (mask_a * wa), a second product over the action k-steps with the weight fragments the
//     forward pass has just read.
// Kernel chain, workspace, partial-sum layouts and the deterministic two-stage reduction are fset.hip's (finalize_* are
// shared, fset_common.h). Tested against the float64 oracle at 2e-5 of each tensor's max (tests/test_gpu_fsplit.py,
// test_gpu_configs_full.py: 5 x tighter than the exact-f32 kernels' 1e-4) -- not the 2 % the bf16 learners are allowed.
#include <type_traits>

#include "fset_common.h"
#include "anchor.h"
#include "smooth.h"

namespace avd {
namespace fsplit {
using namespace fset;

struct ActorS {
    static constexpr int K = 256, KP = 256, NFT = 8, NKS = 16, LD = 264, NGT = 9, KG = 288;
    static constexpr bool critic = false;
};
struct CriticS {
    static constexpr int K = 304, KP = 320, NFT = 10, NKS = 19, LD = 312, NGT = 10, KG = 320;  // 256 state + 48 action features
    static constexpr bool critic = true;
};
constexpr int NGT_MAX = 10;

// compile-time loop: f(std::integral_constant<int, I>) for I = 0 .. N - 1 (every index a constant inside f: `if constexpr`,
// no reliance on the unroller for register arrays)
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// fp16 pairs (heads): 11 + 11 significant bits, |x - hi - lo| <= 2^-24 |x| -- an f32 value almost exactly. The heads need
// it: the hi + lo residual of a WEIGHT is the same for every batch row, so it biases q and y instead of averaging out, and
// the TD error q - y amplifies the bias by |q| / |q - y| (measured with bf16 pairs: 1e-3 of a gradient tensor's max at 51
// platoons, same for the mean of 51 single-platoon calls). fp16 has a 5-bit exponent, so the static operands are scaled by
// powers of two (exact) into its upper range and the scales are folded into f32 constants downstream: second-layer weights
// by SW (per set and net, max |W| SW in [2^12, 2^13)), first-layer weights and biases by S1 (activations then sit 2^6 higher,
// their lo parts stay normal numbers). An activation S1 P1 >= 65520 (P1 >= 1023.75) would round to fp16 inf -- and, the file being
// built with -fno-honor-nans (relu = one v_max_f32, which returns its non-NaN operand), the resulting NaN accumulators would
// silently become zeros. Every conversion to fp16 that can overflow is therefore TESTED: the scaled static operands in the prep
// kernels, the inputs in the pack role of front_kernel, and the running maximum of every first-layer accumulator tile in the forward heads
// (8 v_max3_f32 per tile); a hit sets *bad and finalize writes NaN into the whole gradient slab, like a non-finite input.
typedef _Float16 f16;
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr float S1 = 64.f;
constexpr float F16_OVERFLOW = 65520.f;  // the smallest float that rounds to fp16 infinity
// timing ablations (AVD_FSPLIT_ABL, results wrong by design) exist in the DIAGNOSTIC build only: in the product the bits are the
// constant 0 and every branch on them folds away
#if defined(FSPLIT_ABL_CONST)
#define FSPLIT_ABL(x) FSPLIT_ABL_CONST  // (A/B builds with the ablation compiled in: tools/fsplit_abl_const.sh)
#elif defined(AVD_DIAG)
#define FSPLIT_ABL(x) (x)
#else
#define FSPLIT_ABL(x) 0
#endif
__device__ __forceinline__ void split2h(float a, float b, unsigned& hi, unsigned& lo) {
    const f32x2 f = {a, b};
    const f16x2 h = __builtin_convertvector(f, f16x2);
    hi = __builtin_bit_cast(unsigned, h);
    // residuals a - hi.lo16, b - hi.hi16 in one v_fma_mix_f32 each (the f16 halves are read in place: no conversion back)
    f32x2 l;
#ifdef __HIP_DEVICE_COMPILE__
    asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(l[0]) : "v"(hi), "v"(a));
    asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l[1]) : "v"(hi), "v"(b));
#else
    l[0] = a - (float)h[0], l[1] = b - (float)h[1];
#endif
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(l, f16x2));
}
__device__ __forceinline__ void split1h(float x, f16& hi, f16& lo) {
    hi = (f16)x;
    lo = (f16)(x - (float)hi);
}
// an optimisation barrier on 16 accumulator registers: what was computed into them is computed HERE
template <class V>
__device__ __forceinline__ void pin16(V& x) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        float a = x[8 * q], b = x[8 * q + 1], c = x[8 * q + 2], d = x[8 * q + 3], e = x[8 * q + 4], f = x[8 * q + 5], g = x[8 * q + 6], h = x[8 * q + 7];
        asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h));
        x[8 * q] = a, x[8 * q + 1] = b, x[8 * q + 2] = c, x[8 * q + 3] = d, x[8 * q + 4] = e, x[8 * q + 5] = f, x[8 * q + 6] = g, x[8 * q + 7] = h;
    }
}
__device__ __forceinline__ f16x8 fragh(unsigned a, unsigned b, unsigned c, unsigned d) {
    uint4 o;
    o.x = a, o.y = b, o.z = c, o.w = d;
    return __builtin_bit_cast(f16x8, o);
}
__device__ __forceinline__ f32x16 mfmah(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
// the first-layer fragments, fp16 pairs (slot layout: make_xg below with g = 1; sc scales weights and bias)
__device__ __forceinline__ f16x8 make_xh(float x0, float x1, float x2, float x3, int h) {
    f16 a0, a1, a2, a3, l0, l1, l2, l3;
    split1h(x0, a0, l0), split1h(x1, a1, l1), split1h(x2, a2, l2), split1h(x3, a3, l3);
    const f16 one = (f16)1.f, zero = (f16)0.f;
    f16x8 v;
    v[0] = a0, v[1] = a1, v[2] = a2, v[3] = a3;
    v[4] = h ? one : l0, v[5] = h ? one : l1, v[6] = h ? zero : l2, v[7] = h ? zero : l3;
    return v;
}
__device__ __forceinline__ f16x8 make_wh(float w0, float w1, float w2, float w3, float b, float sc, int h) {
    f16 a0, a1, a2, a3, l0, l1, l2, l3, bh, bl;
    split1h(sc * w0, a0, l0), split1h(sc * w1, a1, l1), split1h(sc * w2, a2, l2), split1h(sc * w3, a3, l3), split1h(sc * b, bh, bl);
    const f16 zero = (f16)0.f;
    f16x8 v;
    v[0] = h ? l0 : a0, v[1] = h ? l1 : a1, v[2] = h ? l2 : a2, v[3] = h ? l3 : a3;
    v[4] = h ? bh : a0, v[5] = h ? bl : a1, v[6] = h ? bh : a2, v[7] = h ? zero : a3;  // (k slot 14 = b_hi: meets g_lo in dw_kernel, 0 in the heads)
    return v;
}
// dw_kernel's input fragment: the row factor g = |g3| 2^kg rides in the input, (g x) and g as fp16 pairs:
//   k slot      0..3        4..7        8..11       12       13       14      15
//   input  x:   (gx)_hi     (gx)_lo     (gx)_hi     g_hi     g_hi     g_lo    0
//   weight w:   w_hi        w_hi        w_lo        b_hi     b_lo     b_hi    0        (make_wh, scaled by S1)
// = S1 g (x . w + b): relu(W1 (g x) + g b1) = g relu(z1), one MFMA like every first layer here.
__device__ __forceinline__ f16x8 make_xg(float x0, float x1, float x2, float x3, float g, int h) {
    f16 a0, a1, a2, a3, l0, l1, l2, l3, gh, gl;
    split1h(x0, a0, l0), split1h(x1, a1, l1), split1h(x2, a2, l2), split1h(x3, a3, l3), split1h(g, gh, gl);
    const f16 zero = (f16)0.f;
    f16x8 v;
    v[0] = a0, v[1] = a1, v[2] = a2, v[3] = a3;
    v[4] = h ? gh : l0, v[5] = h ? gh : l1, v[6] = h ? gl : l2, v[7] = h ? zero : l3;
    return v;
}

template <int S>
__device__ __forceinline__ void load_x(const float* xa, long row, float (&x)[4]) {
    if (S == 4) {
        const float4 v = *(const float4*)(xa + 4 * row);
        x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = k < S ? xa[S * row + k] : 0.f;
    }
}

// position of feature f in the heads' weight image: inside each tile of 32, bits 2 and 3 of the index trade places. Element
// jj of lane half h of k-step s of a first-layer accumulator tile [feature][row] is feature 16 s + 8 (jj >> 2) + 4 h + (jj & 3)
// (cdna_hip_programming.md, "An accumulator tile as the next MFMA's operand"); stored at 16 s + 8 h + jj the weights of those 8
// features are ONE 16-byte LDS read of the A operand's lane (n, h).
__host__ __device__ constexpr int wpos(int f) { return (f & ~12) | ((f & 4) << 1) | ((f & 8) >> 1); }

// one network's operands (device pointers into the caller's slabs and the workspace)
struct NetP {
    const float* th;   // theta or theta_t (+ actor_size for a critic); set stride th_stride
    long th_stride;
    const f16* Whi;    // [sets][H2][K]   fp16 hi of SW * inv1[f] * W2[f][n] at [n][wpos(f)]: the heads' LDS image
    const f16* Wlo;    //                 its lo
    const f16* Wchi;   // [sets][KP][H2]  fp16 hi of SWC * c3[n] * W2[f][n], rows >= K zero: dx_kernel's resident operand (online nets)
    const f16* Wclo;   //                 its lo (SWC: vec[2 H2 + 2])
    const f16x8* wf1h; // [sets][NGT_MAX][64] first-layer weight fragments per feature tile and lane, fp16 pairs scaled by S1 (feature K:
                       // the constant one, relu(0 x + 1): its row of dw_kernel's G is db2)
    const float* vec;  // [sets][VEC]: b2'[128] = b2 + sh1 . W2, c3[128] = inv2 * w3, d3 = b3 + sh2 . w3, SW, SWC
    const unsigned* wap;  // [sets][2 hi/lo][2 h][3 k-steps][4] packed fp16 pairs of S1 * wa, the critic's action-layer weights (HEAD_BOTH's sweep B2)
};

// ---- pack: split first-layer input fragments of every batch row, once per learn call (+ the finiteness test) ----------
// outh: fp16 pairs (heads, dx_kernel); extra: the per-row scalar that travels with x (a: an fp16 fragment too; r: only tested)
// One launch packs both inputs of a learn call: blockIdx.y = 0 -> (s, a: the action travels as an fp16 fragment too), 1 -> (s2, r: only
// tested for finiteness).
struct PackArgs {
    const float* x[2];
    const float* extra[2];
    f16x8* outh[2];
    long rows;
};
// A role of front_kernel (below): block bx of input `which`. Nothing in that launch may set *bad -- one of its blocks clears it with
// a plain store -- so a hit is reported through the wave's own word of the front flags (front_flag), which prep_kernel ORs into *bad.
__device__ __forceinline__ void front_flag(unsigned* wave_flags, bool hit) {
    const bool any = __ballot(hit) != 0;
    if ((threadIdx.x & 63) == 0) wave_flags[threadIdx.x >> 6] = any;  // written by every wave, hit or not: no stale word survives a call
}
template <int S>
__device__ __forceinline__ void pack_x_role(const PackArgs& a, int which, long bx, unsigned* wave_flags) {
    const float* x = a.x[which];
    const float* extra = a.extra[which];
    const bool extra_is_action = which == 0;
    const long i = bx * 256 + threadIdx.x;
    bool nf = false;
    if (i < 2 * a.rows) {
        float v[4];
        load_x<S>(x, i >> 1, v);
        nf = not_finite(v[0]) || not_finite(v[1]) || not_finite(v[2]) || not_finite(v[3]);
        nf = nf || fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))) >= F16_OVERFLOW;  // (fp16 input fragments)
        if (!(i & 1)) {
            const float e = extra[i >> 1];  // a (an fp16 input fragment of the critic too) or r
            nf = nf || not_finite(e) || (extra_is_action && fabsf(e) >= F16_OVERFLOW);
        }
        a.outh[which][i] = make_xh(v[0], v[1], v[2], v[3], (int)(i & 1));
    }
    front_flag(wave_flags, nf);
}

// ---- operand preparation ---------------------------------------------------------------------------------------------
struct PrepArgs {
    avd_mlp_layout L;
    int S;
    const float *theta, *stats, *theta_t, *stats_t;
    f16 *Whi[4], *Wlo[4];  // net 0 actor, 1 critic, 2 target actor, 3 target critic
    f16 *Wchi[4], *Wclo[4];  // online nets only
    f16x8* wf1h[4];
    float* vec[4];
    unsigned* wap;
    unsigned* smax;  // [4 nets][sets][SCALE_SLICES][2] maxima of the scale role, one pair per slice block (plain stores)
    int* bad;        // cleared by the front launch, set from prep_kernel on
    unsigned* fflag; // [n_fflag] front flags: one word per wave of the prep1 and pack roles, non-zero = what used to set *bad there
    int n_fflag;
};
// SW per (net, set): the power of two that puts max |inv1[f] W2[f][n]| into [2^12, 2^13) -> vec[2 H2 + 1]; online nets also
// SWC, the same for dx_kernel's operand c3[n] W2[f][n] -> vec[2 H2 + 2]. Two steps: the scale role of front_kernel leaves the two
// maxima of each of 16 slices per (net, set) in smax (16 blocks per matrix, coalesced -- r03's one block per matrix walked 304 rows
// of 512 bytes with one thread each: 11 us, 33 with the second maximum; plain stores, r09: until then atomicMax into words that a
// memset had to zero first), every thread of prep_kernel takes the maximum of the 16 (on the bits of non-negative floats: order-
// independent, so deterministic) and turns it into the powers of two, block n = 0 writes them for the later kernels.
constexpr int SCALE_SLICES = 16;
__device__ __forceinline__ float pow2_for(float mx) {  // the power of two that puts mx into [2^12, 2^13)
    int e = 0;
    if (mx > 0.f && !not_finite(mx)) (void)frexpf(mx, &e);  // mx = fr * 2^e, fr in [0.5, 1)
    int k = 13 - e;
    k = k < -14 ? -14 : (k > 30 ? 30 : k);
    return ldexpf(1.f, k);
}
__device__ __forceinline__ void scale_role(const PrepArgs& a, int net, int set, int slice, int n_sets) {
    __shared__ float red[256], red2[256], c3a[H2], inva[CriticS::K];
    const int tid = threadIdx.x;
    const bool critic = net & 1, target = net >= 2;
    const avd_mlp_layout& L = a.L;
    const float* th = (target ? a.theta_t : a.theta) + (long)set * L.theta_size + (critic ? L.actor_size : 0);
    const float* st = (target ? a.stats_t : a.stats) + (long)set * L.stats_size;
    const int K = critic ? CriticS::K : ActorS::K, oW2 = critic ? L.cW2 : L.aW2;
    const int og2 = critic ? L.cg3 : L.ag2, omv2 = critic ? L.cmv3 : L.amv2, oW3 = critic ? L.cW3 : L.aW3;
    if (tid < H2) c3a[tid] = fabsf((1.0f / sqrtf(st[omv2 + tid] + BN_EPS)) * th[og2 + tid] * th[oW3 + tid]);  // |c3[n]| = |inv2[n] w3[n]|
    for (int f = tid; f < K; f += 256) {
        int og, omv, ff = f;
        if (!critic) og = L.ag1, omv = L.amv1;
        else if (f < H1) og = L.cgs, omv = L.cmvs;
        else og = L.cga, omv = L.cmva, ff = f - H1;
        inva[f] = fabsf((1.0f / sqrtf(st[omv + ff] + BN_EPS)) * th[og + ff]);
    }
    __syncthreads();
    const int total = K * H2, per = (total + SCALE_SLICES - 1) / SCALE_SLICES, lo = slice * per, hi = min(total, lo + per);
    float m = 0.f, m2 = 0.f;
    for (int i = lo + tid; i < hi; i += 256) {
        const float w = fabsf(th[oW2 + i]);
        m = fmaxf(m, inva[i / H2] * w);
        m2 = fmaxf(m2, c3a[i % H2] * w);
    }
    red[tid] = m, red2[tid] = m2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]), red2[tid] = fmaxf(red2[tid], red2[tid + o]);
        __syncthreads();
    }
    if (tid == 0) {
        unsigned* dst = a.smax + (((long)net * n_sets + set) * SCALE_SLICES + slice) * 2;
        dst[0] = __float_as_uint(red[0]);  // (non-negative floats order like their bits; a NaN / inf input lands on top and is
        dst[1] = __float_as_uint(red2[0]);  //  caught by the finiteness tests of prep_kernel)
    }
}
// one block per (output column n, net, set), one thread per feature f
__global__ __launch_bounds__(320) void prep_kernel(const PrepArgs a) {
    __shared__ float red[320];
    const int n = blockIdx.x, net = blockIdx.y, set = blockIdx.z, f = threadIdx.x;
    const bool critic = net & 1, target = net >= 2;
    const avd_mlp_layout& L = a.L;
    const float* th = (target ? a.theta_t : a.theta) + (long)set * L.theta_size + (critic ? L.actor_size : 0);
    const float* st = (target ? a.stats_t : a.stats) + (long)set * L.stats_size;
    const int K = critic ? CriticS::K : ActorS::K, KP = critic ? CriticS::KP : ActorS::KP;
    const int oW2 = critic ? L.cW2 : L.aW2, ob2 = critic ? L.cb2 : L.ab2, oW3 = critic ? L.cW3 : L.aW3, ob3 = critic ? L.cb3 : L.ab3;
    const int og2 = critic ? L.cg3 : L.ag2, obe2 = critic ? L.cbe3 : L.abe2, omm2 = critic ? L.cmm3 : L.amm2, omv2 = critic ? L.cmv3 : L.amv2;
    const float inv2n = (1.0f / sqrtf(st[omv2 + n] + BN_EPS)) * th[og2 + n], c3n = inv2n * th[oW3 + n];
    const unsigned* smax = a.smax + ((long)net * gridDim.z + set) * SCALE_SLICES * 2;
    unsigned mx = 0, mxc = 0;
#pragma unroll
    for (int sl = 0; sl < SCALE_SLICES; ++sl) mx = max(mx, smax[2 * sl]), mxc = max(mxc, smax[2 * sl + 1]);
    const float SW = pow2_for(__uint_as_float(mx)), SWC = pow2_for(__uint_as_float(mxc));
    // what the prep1 and pack roles of the front launch found (they cannot set *bad themselves: that launch clears it): the blocks of
    // net 0, set 0 share the words between them
    // (r14: four words per wait -- clamped index, masked value -- where a rolled loop waited for each word in turn)
    if (net == 0 && set == 0) {
        unsigned any = 0;
        for (int w0 = n * 320 + f; w0 < a.n_fflag; w0 += 4 * H2 * 320) {
            unsigned v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = a.fflag[min(w0 + u * H2 * 320, a.n_fflag - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u) any |= w0 + u * H2 * 320 < a.n_fflag ? v[u] : 0u;
        }
        if (any) atomicOr(a.bad, 1);
    }
    float shw = 0.f;
    if (f < KP) {
        float w = 0.f, inv = 0.f;
        if (f < K) {
            int og, obe, omm, omv, ff = f;
            if (!critic) og = L.ag1, obe = L.abe1, omm = L.amm1, omv = L.amv1;
            else if (f < H1) og = L.cgs, obe = L.cbes, omm = L.cmms, omv = L.cmvs;
            else og = L.cga, obe = L.cbea, omm = L.cmma, omv = L.cmva, ff = f - H1;
            inv = (1.0f / sqrtf(st[omv + ff] + BN_EPS)) * th[og + ff];
            const float sh = th[obe + ff] - st[omm + ff] * inv;
            w = th[oW2 + (long)f * H2 + n];
            shw = sh * w;
            if (not_finite(w) || not_finite(inv) || not_finite(sh)) atomicOr(a.bad, 1);
            f16 hi, lo;
            const float ws = SW * (inv * w);  // in [-2^13, 2^13] unless pow2_for had to clamp
            if (fabsf(ws) >= F16_OVERFLOW) atomicOr(a.bad, 1);
            split1h(ws, hi, lo);
            const long at = ((long)set * H2 + n) * K + wpos(f);
            a.Whi[net][at] = hi, a.Wlo[net][at] = lo;
        }
        if (!target) {
            // dx_kernel's static operand c3[n] W2[f][n]: an fp16 pair too (as a bf16 pair its 2^-17 residual, the same for every
            // batch row, stood at 1e-5 ... 2e-5 of max in the first-layer gradients: r04, tests/test_gpu_configs_full.py)
            f16 hi, lo;
            const float wc = SWC * (c3n * w);
            if (fabsf(wc) >= F16_OVERFLOW) atomicOr(a.bad, 1);
            split1h(wc, hi, lo);
            const long at = ((long)set * KP + f) * H2 + n;
            a.Wchi[net][at] = hi, a.Wclo[net][at] = lo;
        }
    }
    red[f] = shw;
    __syncthreads();
    if (f < 64) red[f] += red[f + 256];  // 320 = 256 + 64
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (f < o) red[f] += red[f + o];
        __syncthreads();
    }
    float* vec = a.vec[net] + (long)set * VEC;
    if (f == 0) {
        if (n == 0) vec[2 * H2 + 1] = SW, vec[2 * H2 + 2] = SWC;
        vec[n] = th[ob2 + n] + red[0];
        vec[H2 + n] = c3n;
        if (not_finite(vec[n]) || not_finite(c3n) || not_finite(th[ob3])) atomicOr(a.bad, 1);
    }
    if (n == 0) {  // d3 = b3 + sum_n sh2[n] w3[n]
        __syncthreads();
        float v = 0.f;
        if (f < H2) {
            const float inv2 = (1.0f / sqrtf(st[omv2 + f] + BN_EPS)) * th[og2 + f];
            v = (th[obe2 + f] - st[omm2 + f] * inv2) * th[oW3 + f];
        }
        red[f] = v;
        __syncthreads();
        for (int o = 64; o > 0; o >>= 1) {
            if (f < o) red[f] += red[f + o];
            __syncthreads();
        }
        if (f == 0) vec[2 * H2] = th[ob3] + red[0];
    }
}
// first-layer weight fragments: one wave per (feature tile, net, set), one thread per lane of the fragment; tiles >= 8 of a
// critic are its action layer; feature K of every net is the constant one relu(0 x + 1) (dw_kernel: its row of G is db2).
// A role of front_kernel, four to a block; returns whether an operand was non-finite or would overflow fp16 (-> the wave's front flag).
__device__ __forceinline__ bool prep1_role(const PrepArgs& a, int ft, int net, int set, int lane) {
    const int r = lane & 31, h = lane >> 5;
    bool hit = false;
    const bool critic = net & 1, target = net >= 2;
    const avd_mlp_layout& L = a.L;
    const float* th = (target ? a.theta_t : a.theta) + (long)set * L.theta_size + (critic ? L.actor_size : 0);
    const int K = critic ? CriticS::K : ActorS::K;
    const int f = 32 * ft + r;
    float w[4] = {0.f, 0.f, 0.f, 0.f}, b = 0.f;
    if (f == K) {
        b = 1.f;
    } else if (f < K) {
        if (critic && ft >= 8) {
            w[0] = th[L.cWa + (f - H1)], b = th[L.cba + (f - H1)];
        } else {
            const float* W = th + (critic ? L.cWs : L.aW1);
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = k < a.S ? W[k * H1 + f] : 0.f;
            b = th[(critic ? L.cbs : L.ab1) + f];
        }
        if (not_finite(w[0]) || not_finite(w[1]) || not_finite(w[2]) || not_finite(w[3]) || not_finite(b)) hit = true;
        // the heads' and dx's fragments carry S1 w, S1 b as fp16 pairs
        if (S1 * fmaxf(fmaxf(fabsf(w[0]), fabsf(w[1])), fmaxf(fmaxf(fabsf(w[2]), fabsf(w[3])), fabsf(b))) >= F16_OVERFLOW) hit = true;
    }
    a.wf1h[net][((long)set * NGT_MAX + ft) * 64 + lane] = make_wh(w[0], w[1], w[2], w[3], b, S1, h);
    if (net == 1 && ft == 0 && lane < 48) {
        // HEAD_BOTH's B operand of M = W2T[:, action] . (mask_a * wa): element jj of lane half hh of action k-step ks is action
        // feature fa = 16 ks + 8 (jj >> 2) + 4 hh + (jj & 3); entry [hl][hh][ks][m] packs elements jj = 2 m, 2 m + 1
        const int hl = lane / 24, hh = (lane / 12) & 1, ks = (lane / 4) % 3, m = lane & 3;
        unsigned v = 0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int jj = 2 * m + e, fa = 16 * ks + 8 * (jj >> 2) + 4 * hh + (jj & 3);
            f16 hi, lo;
            split1h(S1 * th[L.cWa + fa], hi, lo);
            v |= (unsigned)__builtin_bit_cast(unsigned short, hl ? lo : hi) << (16 * e);
        }
        a.wap[(long)set * 48 + lane] = v;
    }
    return hit;
}

// ---- the front launch (r09): everything of a learn call that depends on nothing but the call's inputs, in ONE launch ---------------
// scale, prep1 and pack_x have no dependence on one another, and the two memsets in front of them (the gradient slab; *bad and the
// maxima) were stream operations of their own: five dependent-looking operations, none of which fills the GPU for its whole
// duration. The block index selects the role; a block is one role from its first instruction to its last (the scale role's
// barriers are met by whole blocks). Workgroups are dispatched in index order, so the latency-bound roles come FIRST -- scale's
// 64 blocks per set walk a dependent chain of reductions, ~10 us however empty the GPU is -- and the streaming role (pack: 2 x
// ceil(rows / 128) blocks) fills every slot they leave and runs beside them; the other way round the small blocks would only start
// when the last pack blocks retire, and their latency would be a tail.
//   [0, n_scale)               scale: block -> (net, set, slice); two maxima per slice, plain stores (no zeroed word needed)
//   [.., + n_prep1)            prep1: wave -> (feature tile, net, set)
//   [.., + n_zero)             the gradient slab, 4096 floats per block: finalize never writes the padding between its tensors, and
//                              nothing reads or writes the slab between here and finalize; the first of them also clears *bad --
//                              safe because no role of this launch sets it (front flags: front_flag, prep_kernel)
//   [.., + 2 n_pack)           pack_x: (s, a) then (s2, r)
// prep_kernel needs the maxima and follows as the second launch.
struct FrontArgs {
    PrepArgs pa;
    PackArgs pk;
    float* grads;
    long n_grads;  // floats of the slab
    int n_sets, n_scale, n_prep1, n_zero, n_pack;
};
constexpr int ZERO_PER_BLOCK = 4096;
template <int S>
__global__ __launch_bounds__(256) void front_kernel(const FrontArgs a) {
    int b = blockIdx.x;
    if (b < a.n_scale) {
        scale_role(a.pa, b & 3, (b >> 2) % a.n_sets, (b >> 2) / a.n_sets, a.n_sets);
        return;
    }
    b -= a.n_scale;
    if (b < a.n_prep1) {
        const int q = 4 * b + (threadIdx.x >> 6);  // (feature tile, net, set), feature tile fastest
        bool hit = false;
        if (q < NGT_MAX * 4 * a.n_sets) hit = prep1_role(a.pa, q % NGT_MAX, (q / NGT_MAX) & 3, q / (NGT_MAX * 4), threadIdx.x & 63);
        front_flag(a.pa.fflag + 4 * (long)b, hit);
        return;
    }
    b -= a.n_prep1;
    if (b < a.n_zero) {
        if (b == 0 && threadIdx.x == 0) *a.pa.bad = 0;
        const long base = (long)b * ZERO_PER_BLOCK + threadIdx.x;
#pragma unroll
        for (int k = 0; k < ZERO_PER_BLOCK / 256; ++k)
            if (base + 256 * k < a.n_grads) a.grads[base + 256 * k] = 0.f;
        return;
    }
    b -= a.n_zero;
    const int which = b >= a.n_pack;
    pack_x_role<S>(a.pk, which, b - which * a.n_pack, a.pa.fflag + 4 * ((long)a.n_prep1 + b));
}

// ---- head: first layer -> second-layer GEMM (three MFMAs per product) -> output layer [-> its backward] -------------------
// (2..4 were r03's HEAD_CRITIC / HEAD_CONST / HEAD_ACTOR: two-launch critic heads and the second actor forward, gone in r04; today's
//  HEAD_CRITIC, 7, is HEAD_BOTH cut off behind its branch A: the TD-only call's critic head)
enum HeadMode { OUT_TANH = 0, OUT_TD = 1, HEAD_BOTH = 5, OUT_TANH_SAVE = 6, HEAD_CRITIC = 7 };
struct HeadArgs {
    unsigned long long* stamp;  // diagnostic build (-DAVD_STAMP) only: [8 waves][8] accumulated s_memtime deltas of workgroup 16
    NetP net;
    int n_agents, n_sets;
    const f16x8* xf;   // [n_agents][64][2] packed first-layer input fragments of the states, fp16 pairs (front_kernel: pack_x_role)
    const float* act;  // [n_agents][64] the critic's action input (a, a' or mu)
    const float* act2; // HEAD_BOTH: mu (act = a)
    const float* r;    // OUT_TD: rewards [n_agents][64]
    const float* yin;  // HEAD_BOTH, HEAD_CRITIC: TD targets
    const float* aw;   // per-agent factor on the loss seeds (weighted federated mean) or NULL
    float* out;        // OUT_*: per-row result
    unsigned* sm;      // HEAD_BOTH, OUT_TANH_SAVE: the relu mask [z2 > 0], one bit per element, [n_agents][64][4 words] (16 B per row;
                       // no sign: the readers take sign(g3) from g3). Word t of a row covers features [32 t, 32 t + 32), pair-interleaved:
                       // bit j = feature 32 t + 2 j, bit 16 + j = feature 32 t + 2 j + 1 (j = 0..15) -- so that fp16 pair j of a
                       // 16-feature chunk is one AND and one v_mul_u32_u24 away (mask_pair)
    float* g3;         // HEAD_BOTH: the row factor of dZ2 [n_agents][64]
    float* dmu;        // HEAD_BOTH: dLa/dmu per row [n_agents][64]
    float* part_s;     // HEAD_*: [grid][8 waves][2] sums of the seeds and of the loss terms
    float* part_s2;    // HEAD_BOTH: the same sums of the critic(s, mu) branch (the actor loss); HEAD_CRITIC: zeros
    float* part_m;     // backward modes: [grid][8 waves] max |g3| over the wave's rows (dw / dx scale their fp16 operands by it)
    float* tz;         // OUT_TANH_SAVE: tanh(z) per row [n_agents][64] (the actor's backward seed needs 1 - t^2: actor_seed_kernel)
    float gamma, high, inv_n;
    int* bad;          // set when an activation would overflow fp16 (S1 P1 >= 65520): finalize then writes NaN gradients
    int abl;           // diagnostic build only (AVD_FSPLIT_ABL bit 4; 0 in the product): the relu / hi-lo split VALU of every first-layer tile
                       // is skipped (raw bits as operands: WRONG results) -- what the heads' time owes to that VALU work
};
// Workgroup = 8 waves bound to one weight set; LDS holds the fp16 hi and lo images of its BN-folded, scaled second-layer
// weights for the workgroup's whole life. Wave w owns rows [32 (w & 1), +32) of every 4th tile. Per feature tile: the first layer of ITS rows
// on the matrix cores (lane = batch row, registers = features), relu, hi / lo split of the 16 values (VALU), and per k-step
// and 32-column tile three MFMAs (A = weight fragments from LDS, B = the split activations as they stand in the registers).
//
// Modes: OUT_TANH (target actor: a'), OUT_TANH_SAVE (actor: mu, + the relu masks and tanh(z) its backward pass needs), OUT_TD (target
// critic -> y) and HEAD_BOTH: critic(s, a) and critic(s, mu) see the same states through the same weights, so 8 of their 10
// first-layer tiles and 192 of their 228 second-layer MFMAs per 32 rows are the SAME work -- one pass over the state tiles, then
// three sweeps over the action k-steps on the one accumulator set: A (input a: TD seed, signed masks), B1 (input mu, by
// linearity), B2 (the action gradient through M).
// HEAD_CRITIC (avd_learn_set_split_td_f16x3: a call on which the actor does not move) is HEAD_BOTH up to and including branch A --
// the state tiles, the A sweep, g3, the masks, the loss sums -- and then the next tile: no mu input, no wap table, no B sweeps, no
// dmu; its part_s2 is zeros, so that finalize's actor-loss sum is defined. What it shares with HEAD_BOTH it computes the same way:
// same bits in g3, the masks and the partial sums.
// (r04, tried: the forward-only modes with 64 rows per wave -- both row halves against every weight fragment pair, six MFMAs per
// two LDS reads instead of three, 128 accumulator registers: OUT_TANH 190.9 us against 190, OUT_TD 220.8 against 223 on the same
// box. Halving the LDS bytes per MFMA buys nothing: the heads are not LDS-bound. Not kept.)
#ifndef HEAD_FAST
#define HEAD_FAST 5
#define HEAD_SLOW 3
#endif

// HP (OUT_TD of avd_learn_set_split_hp_f16x3): the TD epilogue's gamma is the workgroup's weight set's, row (set / block) % n_groups of
// the sweep table; nothing else differs from the scalar instantiation.
//
// The kernel's body is a device function over ONE raw, 16-byte aligned LDS buffer from which it carves its arrays (r15): the
// stand-alone kernel below declares the buffer and calls it, forward_kernel calls four of them in a row on the same buffer. A body
// never returns early: a workgroup without tiles falls through to its end like every other (the next phase's barrier expects it).
template <class NET, int MODE>
constexpr int head_lds_bytes() {
    return 2 * H2 * NET::LD * (int)sizeof(f16) + 2 * H2 * (int)sizeof(float) + (MODE == HEAD_BOTH ? 48 : 4) * (int)sizeof(unsigned);
}
template <int S, class NET, int MODE, bool HP = false, class... H>
__device__ __forceinline__ void head_body(const HeadArgs& p, unsigned char* lds, const int tid, H... hp) {
    constexpr int K = NET::K, NKS = NET::NKS, NFT = NET::NFT, LD = NET::LD;  // LD/2 = 4 (mod 8) dwords: conflict-free b128
    constexpr int NTH = NT;  // 8 waves: two per SIMD at <= 256 registers
    constexpr bool BOTH = (MODE == HEAD_BOTH);
    constexpr bool BA = BOTH || MODE == HEAD_CRITIC;  // the modes that run branch A (the critic loss and its backward seed)
    // (T1 = sum_rows g3 relu(z2) is not accumulated here: finalize derives it from dw_kernel's partials, FinArgs::t1_from_g)
    static_assert(!BA || NET::critic, "HEAD_BOTH and HEAD_CRITIC are critic modes");
    f16(*wimg)[H2 * LD] = (f16(*)[H2 * LD]) lds;                       // [2][H2 * LD]
    float* b2s = (float*)(lds + 2 * H2 * LD * sizeof(f16));            // [H2]
    float* c3s = b2s + H2;                                             // [H2]
    unsigned* waps = (unsigned*)(c3s + H2);                            // [BOTH ? 48 : 4]
    const int w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5, q = w >> 1, rh = w & 1;
    const int set = blockIdx.x % p.n_sets, j0 = blockIdx.x / p.n_sets, J = gridDim.x / p.n_sets, P = p.n_agents / p.n_sets;
#ifdef AVD_STAMP
    unsigned long long hacc[4] = {0, 0, 0, 0}, hlast = __builtin_amdgcn_s_memtime();
    const unsigned long long hstart = hlast;
#define HSTAMP(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); hacc[i] += t_ - hlast; hlast = t_; }
#else
#define HSTAMP(i)
#endif
    const float* vec = p.net.vec + (long)set * VEC;
    const f16x8* wf1 = p.net.wf1h + (long)set * NGT_MAX * 64 + lane;  // + 64 ft
    const f32x16 zero16 = {};
    const int ntile = j0 < P ? (P - j0 + J - 1) / J : 0;  // tiles of this workgroup: j0, j0 + J, ..
    const int row = 32 * rh + r;
    f16x8 nx = {};
    float na = 0.f, nb = 0.f, ny = 0.f, nw = 1.f;
    auto fetch_in = [&](int k) {  // one unit (32 rows of a tile) ahead
        const int agent = (j0 + k * J) * p.n_sets + set;
        const long ri = (long)agent * TILE + row;
        nx = p.xf[2 * ri + h];
        if (NET::critic) na = p.act[ri];
        if (BOTH) nb = p.act2[ri];
        if (MODE == OUT_TD) ny = p.r[ri];
        if (BA) ny = p.yin[ri];
        if (BA && p.aw) nw = p.aw[agent];
    };
    // The two waves of a SIMD (w and w + 4) are arbitrated oldest first: with equal shares, waves 0..3 ran 12.0 k cycles per unit
    // and waves 4..7 20.4 k until the old ones were done, then finished alone at 61 % of the matrix pipe (s_memtime stamps, r03;
    // s_setprio does not change it). The tiles are therefore dealt FAST : SLOW per wave pair in periods of 2 (FAST + SLOW) tiles
    // -- a static map, so the grouping of the partial sums (the bits of the result) stays a function of the plan.
    constexpr int FAST = HEAD_FAST, SLOW = HEAD_SLOW, PERIOD = 2 * (FAST + SLOW);
    const int qs = __builtin_amdgcn_readfirstlane(q);  // (scalar tile arithmetic)
    const int cnt = qs < 2 ? FAST : SLOW, start = qs < 2 ? qs * FAST : 2 * FAST + (qs - 2) * SLOW;
    int k = start, pos = 0;  // the wave pair's current tile and its place in the pair's group of cnt
    auto next_tile = [&](int kk, int pp) { return pp + 1 == cnt ? kk + PERIOD - cnt + 1 : kk + 1; };
    // Start-up (r14): EVERY load in front of the barrier is requested before the first of them is waited for -- the tables, the
    // first tile's first-layer fragments (only to have their lines near: the tile loop reads them itself), the wave's first inputs,
    // then the thread's whole share of the weight image (16 / 19 x 16 bytes in registers: the accumulators are not alive yet) --
    // and only then stored to LDS. As a rolled loop of load, wait, store the image alone was 16 / 19 dependent round trips of all
    // 51 workgroups of a set to the same lines, with the tables and the first fetch serially behind it.
    const float SW = vec[2 * H2 + 1], d3 = vec[2 * H2];
    const float vb = vec[tid & (H2 - 1)], vc = vec[H2 + (tid & (H2 - 1))];
    unsigned wv = 0;
    if constexpr (BOTH) wv = p.net.wap[(long)set * 48 + (tid < 48 ? tid : 47)];
    f16x8 warm0 = wf1[0], warm1 = wf1[64];
    if (k < ntile) fetch_in(k);
    // the image: thread tid takes the 16-byte chunks tid, tid + NTH, .. of [hi | lo][n][K / 8], contiguous in global memory
    constexpr int PER = H2 * (K / 8), NLD = 2 * PER / NTH;
    static_assert(2 * PER % NTH == 0, "the image is a whole number of chunks per thread");
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 img[NLD];
    static_for<0, NLD>([&](auto u_c) {  // (static_for: constant indices, the array never exists in memory)
        constexpr int u = decltype(u_c)::value;
        const int i = tid + u * NTH, hl = i / PER, rem = i - hl * PER;
        img[u] = *(const u32x4*)((hl ? p.net.Wlo : p.net.Whi) + (long)set * H2 * K + 8 * rem);
    });
    __builtin_amdgcn_sched_barrier(0);
    // acc = SW S1 z2: the scales of the fp16 operands are folded into the f32 tables (bias in, output weights out)
    const float sc = SW * S1, isc = 1.f / sc;
    if (tid < H2) b2s[tid] = vb * sc, c3s[tid] = vc * isc;
    if (BOTH && tid < 48) waps[tid] = wv;
    static_for<0, NLD>([&](auto u_c) {
        constexpr int u = decltype(u_c)::value;
        const int i = tid + u * NTH, hl = i / PER, rem = i - hl * PER, n = rem / (K / 8), c = rem - n * (K / 8);
        *(u32x4*)(&wimg[hl][n * LD + 8 * c]) = img[u];
    });
    asm volatile("" ::"v"(warm0), "v"(warm1));
    float Dacc = 0.f, Lacc = 0.f, Dacc2 = 0.f, Lacc2 = 0.f, gmax = 0.f;
    // fp16 overflow watch. An activation S1 P1 >= 65520 converts to the pair (hi, lo) = (+inf, -inf), and whatever the weights,
    // w_hi inf + w_lo inf - w_hi inf is NaN in EVERY second-layer accumulator of that batch row (0 inf is NaN too): one
    // accumulator per row and sweep is looked at (bit test: the file is built with -fno-honor-nans), |bits| max-accumulated.
    unsigned watch = 0;
    auto look = [&](float x) {
        unsigned u = __float_as_uint(x);
        asm volatile("" : "+v"(u));  // (keeps the no-nans optimiser from reasoning about the float)
        u &= 0x7fffffffu;
        watch = watch > u ? watch : u;
    };
    __syncthreads();

    const f16* whi0 = &wimg[0][r * LD + 8 * h];  // + 32 t LD + 16 ks
    const f16* wlo0 = &wimg[1][r * LD + 8 * h];
    // the sequence of feature tiles of a unit: tiles 0 .. NFT - 1; HEAD_BOTH: + the action tiles 8, 9 once more (input mu)
    constexpr int NSEQ = BA ? 8 : NFT;  // HEAD_BOTH, HEAD_CRITIC: the state tiles; the action tiles are streamed per column tile below
    HSTAMP(3);  // image fill, tables, first fetch (from the kernel's first instruction)
    for (int ui = 0; k < ntile; ++ui, k = next_tile(k, pos), pos = pos + 1 == cnt ? 0 : pos + 1) {
        const int agent = (j0 + k * J) * p.n_sets + set;
        const long ri = (long)agent * TILE + row;
        const f16x8 xs = nx, xa = make_xh(na, 0.f, 0.f, 0.f, h), xb = BOTH ? make_xh(nb, 0.f, 0.f, 0.f, h) : xa;
        const float ty = ny, tw = nw;
        if (next_tile(k, pos) < ntile) fetch_in(next_tile(k, pos));
        f32x16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 b = *(const float4*)(b2s + 32 * t + 8 * g + 4 * h);
                acc[t][4 * g] = b.x, acc[t][4 * g + 1] = b.y, acc[t][4 * g + 2] = b.z, acc[t][4 * g + 3] = b.w;
            }
        // relu + hi / lo split of a first-layer tile [feature][row] (row on the lane): pair m of k-step s = registers 8 s + 2 m, + 1
        unsigned ph[8], pl[8];
        auto split16 = [&](const f32x16& p1) {
            if (FSPLIT_ABL(p.abl) & 4) {  // (timing ablation: no VALU at all)
#pragma unroll
                for (int m = 0; m < 8; ++m) ph[m] = __float_as_uint(p1[2 * m]), pl[m] = __float_as_uint(p1[2 * m + 1]);
                return;
            }
#pragma unroll
            for (int m = 0; m < 8; ++m) split2h(relu(p1[2 * m]), relu(p1[2 * m + 1]), ph[m], pl[m]);
        };
        // ---- epilogues -----------------------------------------------------------------------------------------------
        // per 32-column tile t (the lane holds columns 32 t + 8 g + 4 h + j of its row, its partner the other half):
        auto zdot_t = [&](f32x16& a, int t) {  // relu in place; returns this lane's part of sum_n c3[n] relu(z2[n])
            float zp = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 c = *(const float4*)(c3s + 32 * t + 8 * g + 4 * h);
                const float cc[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a[4 * g + j] = relu(a[4 * g + j]);
                    zp = fmaf(a[4 * g + j], cc[j], zp);
                }
            }
            return zp;
        };
        auto zdot_nd = [&](const f32x16& a, int t) {  // the same without touching a
            float zp = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 c = *(const float4*)(c3s + 32 * t + 8 * g + 4 * h);
                const float cc[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) zp = fmaf(relu(a[4 * g + j]), cc[j], zp);
            }
            return zp;
        };
        // the relu mask of tile t (a = z2 or relu(z2)) as this lane's half of the tile's packed word (HeadArgs::sm): the lane holds
        // columns c = 8 g + 4 h + j, i.e. bits 4 g + 2 h + (j >> 1) + 16 (j & 1); built here as for h = 0 (mask_store shifts by 2 h)
        auto mask_t = [&](const f32x16& a) {
            unsigned b = 0;
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j) b |= a[4 * g + j] > 0.f ? 1u << (4 * g + (j >> 1) + 16 * (j & 1)) : 0u;
            return b;
        };
        // the row's four words (16 B) from the two lanes' halves: swapping (t, t + 2) across the lane halves leaves lane half h with
        // the h = 0 half and the h = 1 half of word 2 h + (t & 1) -- as (own, partner's) in half 0, (partner's, own) in half 1
        auto mask_store = [&](const unsigned (&b)[4], unsigned* dst) {
            const auto s0 = __builtin_amdgcn_permlane32_swap(b[0], b[2], false, false);
            const auto s1 = __builtin_amdgcn_permlane32_swap(b[1], b[3], false, false);
            uint2 o;
            o.x = s0[0] | (s0[1] << 2), o.y = s1[0] | (s1[1] << 2);
            *(uint2*)(dst + 2 * h) = o;
        };
        auto out_z = [&](f32x16 (&ac)[4]) {  // relu in place, output layer: z = d3 + sum_n c3[n] relu(z2[n])
            float zp = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) zp += zdot_t(ac[t], t);
            zp += __shfl_xor(zp, 32);
            return d3 + zp;
        };
        // ---- the tiles ---------------------------------------------------------------------------------------------------
        split16(mfmah(wf1[0], xs, zero16));
        f16x8 wfn = wf1[64];
        // Weight fragments are read ONE GROUP AHEAD (group = k-step x pair of column tiles: hi and lo of two tiles, 16
        // registers, six MFMAs): a ds_read_b128 issued right in front of the MFMA that consumes it exposes the LDS latency
        // four times per feature tile. wg[parity][2 t][hi, lo].
        f16x8 wg[2][2][2];
        auto read_group = [&](int g, f16x8 (&dst)[2][2]) {  // g = 2 ks + th
            const int ks = g >> 1, th = g & 1;
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                dst[tt][0] = *(const f16x8*)(whi0 + 32 * (2 * th + tt) * LD + 16 * ks);
                dst[tt][1] = *(const f16x8*)(wlo0 + 32 * (2 * th + tt) * LD + 16 * ks);
            }
        };
        read_group(0, wg[0]);
        auto tile = [&](auto si_c, f32x16 (&ac)[4]) {
            constexpr int si = decltype(si_c)::value;
            constexpr int ft = si;                          // feature tile
            // the first layer of the next tile of the sequence
            f32x16 p1n = zero16;
            if constexpr (si + 1 < NSEQ) {
                p1n = mfmah(wfn, (NET::critic && si + 1 >= 8) ? xa : xs, zero16);
                if constexpr (si + 2 < NSEQ) wfn = wf1[64 * (si + 2)];
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int ks = 2 * ft + s;
                if (ks >= NKS) continue;  // (the critic's last tile holds only 16 features)
                const f16x8 bhi = fragh(ph[4 * s], ph[4 * s + 1], ph[4 * s + 2], ph[4 * s + 3]);
                const f16x8 blo = fragh(pl[4 * s], pl[4 * s + 1], pl[4 * s + 2], pl[4 * s + 3]);
#pragma unroll
                for (int th = 0; th < 2; ++th) {
                    const int g = 2 * ks + th;
                    if (g + 1 < 2 * (BA ? 16 : NKS)) read_group(g + 1, wg[(g + 1) & 1]);
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt) {
                        const int t = 2 * th + tt;
                        const f16x8 whi = wg[g & 1][tt][0], wlo = wg[g & 1][tt][1];
                        ac[t] = mfmah(whi, bhi, ac[t]);
                        ac[t] = mfmah(wlo, bhi, ac[t]);
                        ac[t] = mfmah(whi, blo, ac[t]);
                    }
                }
            }
            if constexpr (si + 1 < NSEQ) split16(p1n);
            // Issue order inside the tile (an MFMA holds the SIMD's issue port for 8 of its 32 cycles: the next tile's relu /
            // split VALU goes INTO the gaps, the next group's four fragment reads in front of each group of six MFMAs)
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // first-layer MFMA of the next tile
#pragma unroll
            for (int gi = 0; gi < 4; ++gi) {
                __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
                }
            }
            // (tiles stay in program order: hoisting every tile's first-layer MFMA and weight reads costs hundreds of registers)
            __builtin_amdgcn_sched_barrier(0);
        };
        HSTAMP(0);  // unit start: inputs, bias
        static_for<0, NSEQ>([&](auto si_c) { tile(si_c, acc); });
        HSTAMP(1);  // the feature tiles
        if constexpr (BA) {
            // acc = the state part of z2 (+ bias); the action part is 3 k-steps. Three sweeps of 36 MFMAs over the four column
            // tiles, all on the ONE set of accumulators (acc + T1 + M never coexist: <= 256 registers, two waves per SIMD):
            //   A : acc += W2T[:, action] . f(a)             -> z, TD seed, masks, T1 (acc left as z2, not relu'd)
            //   B1: acc += W2T[:, action] . (f(mu) - f(a))   -> z2 of the mu branch by linearity: q and 64 relu bits per lane
            //   B2: M = W2T[:, action] . (mask_a (.) wa)     -> dmu
            // (an earlier form kept both branches' accumulators and M alive: 256 + 244 registers, one wave per SIMD, 456 us)
            f16x8 fh[3], fl[3];
            auto act_sweep = [&](f32x16 (&c)[4]) {  // c[t] += W2T[tile t, action k-steps] . (fh, fl)
                f16x8 wq[2][2][2];
                read_group(2 * 16, wq[0]);
#pragma unroll
                for (int g = 0; g < 6; ++g) {
                    if (g + 1 < 6) read_group(2 * 16 + g + 1, wq[(g + 1) & 1]);
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt) {
                        const int t = 2 * (g & 1) + tt;
                        const f16x8 whi = wq[g & 1][tt][0], wlo = wq[g & 1][tt][1];
                        c[t] = mfmah(whi, fh[g >> 1], c[t]);
                        c[t] = mfmah(wlo, fh[g >> 1], c[t]);
                        c[t] = mfmah(whi, fl[g >> 1], c[t]);
                    }
                }
            };
            // ---- branch A: critic(s, a) -> TD seed, masks, T1 (workers/trainer.py:494-498)
#pragma unroll
            for (int tl = 0; tl < 2; ++tl) {
                const f32x16 p1 = mfmah(wf1[64 * (8 + tl)], xa, zero16);
                split16(p1);
#pragma unroll
                for (int ss = 0; ss < 2 - tl; ++ss) {
                    fh[2 * tl + ss] = fragh(ph[4 * ss], ph[4 * ss + 1], ph[4 * ss + 2], ph[4 * ss + 3]);
                    fl[2 * tl + ss] = fragh(pl[4 * ss], pl[4 * ss + 1], pl[4 * ss + 2], pl[4 * ss + 3]);
                }
            }
            act_sweep(acc);
            look(acc[0][0]);
            {
                float zp = 0.f;
#pragma unroll
                for (int t = 0; t < 4; ++t) zp += zdot_nd(acc[t], t);
                zp += __shfl_xor(zp, 32);
                const float diff = d3 + zp - ty, g3a = 2.f * diff * p.inv_n * tw;
                if (h == 0) p.g3[ri] = g3a, Dacc += g3a, Lacc += diff * diff;
                gmax = fmaxf(gmax, fabsf(g3a));
                unsigned mb[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) mb[t] = mask_t(acc[t]);
                mask_store(mb, p.sm + ri * 4);
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (!BOTH) continue;  // HEAD_CRITIC: the critic loss alone -- on to the next tile
            // ---- branch B: critic(s, mu) -> the actor loss -mean(q) and its gradient w.r.t. the action (:501-504)
            f16x8 mh[3], ml[3];
#pragma unroll
            for (int tl = 0; tl < 2; ++tl) {
                const f32x16 pa = mfmah(wf1[64 * (8 + tl)], xa, zero16), pm = mfmah(wf1[64 * (8 + tl)], xb, zero16);
                unsigned dh[8], dl[8], mk[8];
#pragma unroll
                for (int m = 0; m < 4 * (2 - tl); ++m) {
                    split2h(relu(pm[2 * m]) - relu(pa[2 * m]), relu(pm[2 * m + 1]) - relu(pa[2 * m + 1]), dh[m], dl[m]);
                    mk[m] = (pm[2 * m] > 0.f ? 0xffffu : 0u) | (pm[2 * m + 1] > 0.f ? 0xffff0000u : 0u);
                }
#pragma unroll
                for (int ss = 0; ss < 2 - tl; ++ss) {
                    const int kk = 2 * tl + ss;
                    fh[kk] = fragh(dh[4 * ss], dh[4 * ss + 1], dh[4 * ss + 2], dh[4 * ss + 3]);
                    fl[kk] = fragh(dl[4 * ss], dl[4 * ss + 1], dl[4 * ss + 2], dl[4 * ss + 3]);
                    // B operand of M = mask_a * wa (hi, lo): the packed constants where the mu branch's activation is positive
                    const uint4 ch = *(const uint4*)(waps + (0 * 2 + h) * 12 + 4 * kk), cl = *(const uint4*)(waps + (1 * 2 + h) * 12 + 4 * kk);
                    mh[kk] = fragh(ch.x & mk[4 * ss], ch.y & mk[4 * ss + 1], ch.z & mk[4 * ss + 2], ch.w & mk[4 * ss + 3]);
                    ml[kk] = fragh(cl.x & mk[4 * ss], cl.y & mk[4 * ss + 1], cl.z & mk[4 * ss + 2], cl.w & mk[4 * ss + 3]);
                }
            }
            act_sweep(acc);
            look(acc[0][0]);  // (f(mu) - f(a) with f(mu) overflowed: +inf)
            float zq = 0.f;
            unsigned pos[2] = {0u, 0u};  // bit 16 (t & 1) + i of pos[t >> 1]: column i of tile t is active in the mu branch
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                zq += zdot_nd(acc[t], t);
#pragma unroll
                for (int i = 0; i < 16; ++i) pos[t >> 1] |= acc[t][i] > 0.f ? 1u << (16 * (t & 1) + i) : 0u;
            }
            zq += __shfl_xor(zq, 32);
            asm volatile("" : "+v"(pos[0]), "+v"(pos[1]));  // (acc dies here)
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) fh[kk] = mh[kk], fl[kk] = ml[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = zero16;
            act_sweep(acc);
            // dmu[row] = g3 sum_n c3[n] [z2 > 0] M[n][row] (the accumulators hold SW S1 M, c3s carries 1 / (SW S1))
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 c = *(const float4*)(c3s + 32 * t + 8 * g + 4 * h);
                    const float cc[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) sum += (pos[t >> 1] >> (16 * (t & 1) + 4 * g + j) & 1u) ? cc[j] * acc[t][4 * g + j] : 0.f;
                }
            sum += __shfl_xor(sum, 32);
            const float g3b = -p.inv_n * tw;
            if (h == 0) p.dmu[ri] = g3b * sum, Dacc2 += g3b, Lacc2 += d3 + zq;
            continue;
        }
        look(acc[0][0]);
        const float z = out_z(acc);
        if (MODE == OUT_TANH) {
            const float o = tanhf(z) * p.high;
            if (h == 0) p.out[ri] = o;
        } else if (MODE == OUT_TANH_SAVE) {
            // mu = actor(s) AND what the actor's backward pass needs from this forward pass: the relu mask of z2 (one bit per
            // element; the seed's sign is not known yet -- it rides on the row factor in dw / dx) and tanh(z). With them
            // r03's HEAD_ACTOR launch -- the same 200 MFMAs per 32 rows once more, 239 us -- is not needed at all (r04).
            const float t = tanhf(z);
            if (h == 0) p.out[ri] = t * p.high, p.tz[ri] = t;
            unsigned mb[4];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) mb[tt] = mask_t(acc[tt]);
            mask_store(mb, p.sm + ri * 4);
        } else {  // OUT_TD
            if constexpr (HP) {
                if (h == 0) p.out[ri] = ty + hp_of(set, hp...).gamma * z;
            } else {
                if (h == 0) p.out[ri] = ty + p.gamma * z;
            }
        }
        HSTAMP(2);  // epilogue
#ifdef AVD_STAMP
        if (blockIdx.x == 16 && lane == 0 && p.stamp && (w == 0 || w == 4) && ui < 28)
            p.stamp[64 + (w >> 2) * 28 + ui] = hlast - hstart;  // end time of every unit of waves 0 and 4
#endif
    }
#ifdef AVD_STAMP
    if (blockIdx.x == 16 && lane == 0 && p.stamp)
        for (int i = 0; i < 4; ++i) p.stamp[w * 8 + i] = hacc[i];
#endif
    if (watch >= 0x7f800000u) atomicOr(p.bad, 1);
    if (BA) {  // (HEAD_CRITIC: Dacc2 = Lacc2 = 0)
        // one partial per wave: sums over the 32 row lanes of each half (fixed shuffle tree), one writer per half
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            Dacc += __shfl_xor(Dacc, o), Lacc += __shfl_xor(Lacc, o);
            Dacc2 += __shfl_xor(Dacc2, o), Lacc2 += __shfl_xor(Lacc2, o);
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) gmax = fmaxf(gmax, __shfl_xor(gmax, o));
        if (lane == 0) {
            const long slot = (long)blockIdx.x * 8 + w;
            p.part_m[slot] = gmax;
            p.part_s[slot * 2] = Dacc, p.part_s[slot * 2 + 1] = Lacc;
            p.part_s2[slot * 2] = Dacc2, p.part_s2[slot * 2 + 1] = Lacc2;
        }
    }
}
template <int S, class NET, int MODE, bool HP = false, class... H>
__global__ __launch_bounds__(NT) void head_kernel(const HeadArgs p, H... hp) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[head_lds_bytes<NET, MODE>()];
    head_body<S, NET, MODE, HP, H...>(p, lds, threadIdx.x, hp...);
}

// ---- the actor's backward seed (r04: what is left of r03's HEAD_ACTOR launch) --------------------------------------------------
// g3[row] = d mu[row] * high * (1 - tanh(z)^2) (workers/trainer.py:502-506 through agent/model.py:34-36), from the d q / d mu the
// critic head left and the tanh(z) the mu pass stored; per wave max |g3| (set_gscale) and sum g3 (-> d b3) in head_kernel's layout.
struct SeedArgs {
    int n_agents, n_sets;
    const float *dmu, *tz;
    float high;
    float *g3, *part_m, *part_s;
};
__device__ __forceinline__ void seed_body(const SeedArgs& p, const int tid) {
    const int w = tid >> 6, lane = tid & 63;
    const int set = blockIdx.x % p.n_sets, j0 = blockIdx.x / p.n_sets, J = gridDim.x / p.n_sets, P = p.n_agents / p.n_sets;
    float gmax = 0.f, D = 0.f;
    for (int pi = j0 + w * J; pi < P; pi += 8 * J) {  // wave w: tiles j0 + w J, + 8 J, .. of the workgroup's set; lane = row
        const long ri = (long)(pi * p.n_sets + set) * TILE + lane;
        const float t = p.tz[ri], g = p.dmu[ri] * p.high * (1.f - t * t);
        p.g3[ri] = g;
        gmax = fmaxf(gmax, fabsf(g));
        D += g;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) gmax = fmaxf(gmax, __shfl_xor(gmax, o)), D += __shfl_xor(D, o);
    if (lane == 0) {
        p.part_m[(long)blockIdx.x * 8 + w] = gmax;
        p.part_s[((long)blockIdx.x * 8 + w) * 2] = D, p.part_s[((long)blockIdx.x * 8 + w) * 2 + 1] = 0.f;
    }
}
__global__ __launch_bounds__(NT) void actor_seed_kernel(const SeedArgs p) { seed_body(p, threadIdx.x); }

// ---- the row factor's scale --------------------------------------------------------------------------------------------------
// dw and dx carry |g3[row]| inside fp16 operands; g3 is 2 (q - y) / N or d mu * high * (1 - t^2): anything from 1e-12 to 1e-3. The
// backward heads leave max |g3| per wave (part_m); every workgroup of dw / dx reduces its set's J x 8 values to the power of two
// 2^kg with max |g3| 2^kg in [0.5, 1) (exact scaling; max() is order-independent: every workgroup gets the same bits) and
// divides it out of its partial sums at the end. With |g3| 2^kg < 1 an operand |g3| 2^kg S1 P1 stays below the S1 P1 the heads
// have already watched for fp16 overflow. Block-cooperative (one barrier); red: 8 floats of LDS.
__device__ __forceinline__ float set_gscale(const float* part_m, int set, int n_sets, int J, float* red, const int tid) {
    float m = 0.f;
    for (int i = tid; i < J * 8; i += NT) m = fmaxf(m, part_m[((long)(i >> 3) * n_sets + set) * 8 + (i & 7)]);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7])));
    int e = 0;
    if (m > 0.f && !not_finite(m)) (void)frexpf(m, &e);  // m = fr 2^e, fr in [0.5, 1)
    const int k = e > 100 ? -100 : (e < -100 ? 100 : -e);
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(ldexpf(1.f, k))));  // (uniform: keep it in an SGPR)
}

// ---- the packed relu mask (HeadArgs::sm) back to fp16 -----------------------------------------------------------------------
// fp16 pair j of a chunk whose word is already shifted so that its features' bits sit at j and 16 + j: low half = bit j, high half
// = bit 16 + j, each m or 0, with mj = m >> j and m = 0x3c00 (+1) or 0xbc00 (-1). Exact: m has its low 10 bits clear (m >> j for
// j <= 7 loses nothing), and both operands stay below 2^24 -- one v_and_b32 and one v_mul_u32_u24.
__device__ __forceinline__ unsigned mask_pair(unsigned d, int j, unsigned mj) { return __umul24(d & (0x10001u << j), mj); }
// the 16 features [16 c, 16 c + 16) of a row as 32 bytes of fp16 (the heads' old image, byte for byte): w = word c >> 1 of the row
__device__ __forceinline__ void mask_chunk16(unsigned w, int c, unsigned m, uint4& lo, uint4& hi) {
    const unsigned d = w >> (8 * (c & 1));
    lo.x = mask_pair(d, 0, m), lo.y = mask_pair(d, 1, m >> 1), lo.z = mask_pair(d, 2, m >> 2), lo.w = mask_pair(d, 3, m >> 3);
    hi.x = mask_pair(d, 4, m >> 4), hi.y = mask_pair(d, 5, m >> 5), hi.z = mask_pair(d, 6, m >> 6), hi.w = mask_pair(d, 7, m >> 7);
}
__device__ __forceinline__ unsigned mask_one(float g3, bool signed_) { return signed_ && g3 < 0.f ? 0xbc00u : 0x3c00u; }

// ---- dw: G[f][n] += sum_rows (|g3| P1)[row][f] * sm[row][n] over all tiles of the workgroup -------------------------------
struct DwArgs {
    NetP net;
    int n_agents, n_sets;
    const float* x;    // states [n_agents][64][S]
    const float* act;  // the critic's action input [n_agents][64]
    const float* g3;   // [n_agents][64]
    const float* part_m;  // [grid][8] max |g3| per wave of the kernel that wrote g3 (set_gscale)
    const unsigned* sm;  // the packed relu mask of the head (HeadArgs::sm), expanded on staging to fp16 sign(g3) / 0 (both nets; r07's actor
                       // staged 1 / 0 and put the sign onto the A operand: 48 v_xor per wave and tile against 8 VALU per thread here)
    float* partG;      // [grid][KG][128] (row K: the constant-one feature = sum over rows of g3 * mask -> db2 / c3)
    int abl;           // diagnostic build only (AVD_FSPLIT_ABL; 0 in the product): timing ablations with WRONG results -- 1: every tile
                       // fetch reads the workgroup's first tile (no HBM traffic), 2: no workgroup barrier in the tile loop
    unsigned long long* stamp;  // diagnostic build (-DAVD_STAMP) only: [8 waves][8] accumulated s_memtime deltas of workgroup 16
};
// Wave w owns feature tile w (both row halves, all four column tiles: 64 accumulator registers). The tiles past the eight
// state tiles (critic: the action tiles 8, 9; actor: the constant-one tile 8) are cut into eight equal pieces, one per wave
// (critic: tile x row half x pair of column tiles; actor: row half x column tile; 32 more accumulator registers), whose
// row-half partials meet in LDS at the end -- every wave then does the same work per tile. A first-layer tile is evaluated
// with the batch rows as the M index and the row factor |g3| 2^kg in its input fragment (fp16 pairs: make_xg; result: feature on
// the lane, rows in the registers = the A operand of G = Q^T . sm in permuted k order), relu'd and split ONCE into an fp16 pair
// (r04: was a bf16 pair, 2^-17 per row -- in a noise-dominated sum that IS the relative error of the result) and used against
// all four column tiles: 48 VALU per 17 MFMAs. The sm tile goes through LDS (row stride 320 B: conflict-free ds_read_b64_tr_b16), fetched
// TWO tiles ahead; the |g3|-scaled input fragments are built once per tile by 128 threads and shared through LDS.
constexpr int DW_LDZ = 160;
constexpr int DW_LDS_BYTES = 2 * TILE * DW_LDZ * (int)sizeof(f16) + 2 * 2 * TILE * 2 * 16 + 8 * (int)sizeof(float);
template <int S, class NET>
__device__ __forceinline__ void dw_body(const DwArgs& p, unsigned char* lds, const int tid) {
    constexpr int KG = NET::KG, LDZ = DW_LDZ;
    constexpr int XC = NET::critic ? 2 : 1;  // column tiles of a wave's extra piece
    f16(*smimg)[TILE * LDZ] = (f16(*)[TILE * LDZ]) lds;                                   // [2][TILE * LDZ] (40 KB: reused for the extra pieces' partial sums)
    f16x8(*fq)[TILE * 2] = (f16x8(*)[TILE * 2])(lds + 2 * TILE * LDZ * sizeof(f16));     // [2][TILE * 2] scaled input fragments [row][lane half] of the states
    f16x8(*fa)[TILE * 2] = fq + 2;                                                        // [2][TILE * 2] ... of the action (critic)
    float* gred = (float*)(fa + 2);                                                       // [8]
    const int w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int set = blockIdx.x % p.n_sets, j0 = blockIdx.x / p.n_sets, J = gridDim.x / p.n_sets, P = p.n_agents / p.n_sets;
    float gsc;  // 2^kg: set_gscale, below -- behind the requests for everything that does not depend on it
    const f16x8* wf1 = p.net.wf1h + (long)set * NGT_MAX * 64 + lane;
    // this wave's extra piece
    const int xt = NET::critic ? 8 + (w >> 2) : 8, xrh = NET::critic ? (w >> 1) & 1 : (w >> 2) & 1, xc0 = NET::critic ? 2 * (w & 1) : (w & 3);
    const f16x8 wf0 = wf1[64 * w], wfx = wf1[64 * xt];
    f32x16 G0[4], G1[XC];
    const f32x16 zero16 = {};
#pragma unroll
    for (int c = 0; c < 4; ++c) G0[c] = zero16;
#pragma unroll
    for (int c = 0; c < XC; ++c) G1[c] = zero16;

    // Staging. sm (21 MB per pass, from HBM; 335 MB as fp16 before the one-bit image): 64 rows x 8 chunks of 16 features, one chunk
    // per thread (a 32-bit word of the row, shared by two threads; critic: with its row's g3 for the sign), TWO tiles ahead in two
    // register sets used alternately, expanded to 32 bytes of fp16 on the way into LDS (mask_chunk16: two VALU per fp16 pair; the
    // critic's per-row sign adds the seven shifts of m). (fp16 image: one tile of lookahead did not cover the tail of the HBM latency over 512 threads and a barrier -- a
    // third of the kernel was the wait for it, tools/fsplit_ablate.sh @ tag r06-pre-prune.) The inputs
    // (states, g3, actions: 31 MB, L2 / Infinity-Cache resident): one tile ahead, threads 0..127 build the |g3|-scaled fragment
    // of (row, lane half) = (tid >> 1, tid & 1) once per tile.
    const int srow = tid >> 3, sch = tid & 7, frow = tid >> 1, fh = tid & 1;
    unsigned ma = 0, mb = 0;
    float sx[4] = {0.f, 0.f, 0.f, 0.f}, sg = 0.f, sa = 0.f, ga = 0.f, gb = 0.f;
    auto fetch_m = [&](int pl, unsigned& m, float& g) {
        const long ri = (long)(((FSPLIT_ABL(p.abl) & 1) ? j0 : pl) * p.n_sets + set) * TILE + srow;
        m = p.sm[ri * 4 + (sch >> 1)];
        g = p.g3[ri];
    };
    auto fetch_x = [&](int pl) {
        if (pl >= P || tid >= 2 * TILE) return;
        const long ri = (long)(pl * p.n_sets + set) * TILE + frow;
        load_x<S>(p.x, ri, sx);
        sg = p.g3[ri];
        if (NET::critic) sa = p.act[ri];
    };
    // (the mask expansion has no branch: past the last tile it writes stale words into a buffer nobody reads, so that compute()
    // can issue it between its last MFMAs)
    auto stage_m = [&](int buf, unsigned m, float g) {
        uint4* dst = (uint4*)(smimg[buf] + srow * LDZ + 16 * sch);
        mask_chunk16(m, sch, mask_one(g, true), dst[0], dst[1]);
    };
    auto stage_x = [&](int pl, int buf) {
        if (pl >= P) return;
        if (tid < 2 * TILE) {
            const float g = fabsf(sg) * gsc;  // in [0, 1)
            fq[buf][tid] = make_xg(g * sx[0], g * sx[1], g * sx[2], g * sx[3], g, fh);
            if (NET::critic) fa[buf][tid] = make_xg(g * sa, 0.f, 0.f, 0.f, g, fh);
        }
    };
    const int g4 = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    // Three units per tile and wave -- own tile row half 0, row half 1, the extra piece -- as a software pipeline: the relu /
    // split VALU of unit k + 1 is issued INTO the gaps between the MFMAs of unit k (sched_group_barrier). Issued one unit after
    // the other, the two waves of a SIMD run their VALU phases together and their MFMA phases together (same program, one
    // barrier per tile) and neither pipe overlaps the other: measured 5400 cycles per tile and SIMD for 2750 of MFMA.
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    auto read_tr = [&](const f16* at) {  // transposed 16-bit read (the type of the builtin's element is immaterial: bit pattern)
        return __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)at));
    };
    auto read_b = [&](int buf, int e, int s, f16x8 (&bfr)[4]) {  // sm fragments [column tile] of row half e, k-step s
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int R0 = 32 * e + 16 * s + 8 * hf + 4 * (g4 >> 1);
                const f16x4 t = read_tr(smimg[buf] + (R0 + q) * LDZ + 32 * c + 16 * (g4 & 1) + 4 * pp);
#pragma unroll
                for (int j = 0; j < 4; ++j) bfr[c][4 * hf + j] = t[j];
            }
    };
    auto split16e = [&](const f32x16& p1, unsigned (&qh)[8], unsigned (&ql)[8]) {
        if (FSPLIT_ABL(p.abl) & 4) {  // (timing ablation, diagnostic build: no relu / split VALU: WRONG results)
#pragma unroll
            for (int m = 0; m < 8; ++m) qh[m] = __float_as_uint(p1[2 * m]), ql[m] = __float_as_uint(p1[2 * m + 1]);
            return;
        }
#pragma unroll
        for (int m = 0; m < 8; ++m) split2h(relu(p1[2 * m]), relu(p1[2 * m + 1]), qh[m], ql[m]);
    };
    auto compute = [&](int buf, unsigned m, float g) {  // (m, g: the mask word of the tile after it, staged into buffer buf ^ 1)
        unsigned ah[8], al[8], bh[8], bl[8];
        // stage 0: first layer + split of row half 0 (exposed)
        split16e(mfmah(fq[buf][r * 2 + h], wf0, zero16), ah, al);
        __builtin_amdgcn_sched_barrier(0);
        // stage 1: MFMAs of row half 0 | first layer + split of row half 1
        {
            const f32x16 p1 = mfmah(fq[buf][(32 + r) * 2 + h], wf0, zero16);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                f16x8 bfr[4];
                read_b(buf, 0, s, bfr);
                const f16x8 hi = fragh(ah[4 * s], ah[4 * s + 1], ah[4 * s + 2], ah[4 * s + 3]);
                const f16x8 lo = fragh(al[4 * s], al[4 * s + 1], al[4 * s + 2], al[4 * s + 3]);
#pragma unroll
                for (int c = 0; c < 4; ++c) G0[c] = mfmah(hi, bfr[c], G0[c]), G0[c] = mfmah(lo, bfr[c], G0[c]);
            }
            split16e(p1, bh, bl);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // stage 2: MFMAs of row half 1 | first layer + split of the extra piece (input fragment of ITS row half)
        {
            const f16x8 xin = NET::critic ? fa[buf][(32 * xrh + r) * 2 + h] : fq[buf][(32 * xrh + r) * 2 + h];
            const f32x16 px = mfmah(xin, wfx, zero16);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                f16x8 bfr[4];
                read_b(buf, 1, s, bfr);
                const f16x8 hi = fragh(bh[4 * s], bh[4 * s + 1], bh[4 * s + 2], bh[4 * s + 3]);
                const f16x8 lo = fragh(bl[4 * s], bl[4 * s + 1], bl[4 * s + 2], bl[4 * s + 3]);
#pragma unroll
                for (int c = 0; c < 4; ++c) G0[c] = mfmah(hi, bfr[c], G0[c]), G0[c] = mfmah(lo, bfr[c], G0[c]);
            }
            split16e(px, ah, al);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // stage 3: MFMAs of the extra piece: column tile(s) xc0.. of row half xrh (runtime: the fragments are read at their
        // address, not selected from registers) | the mask expansion of the next tile (r07: after them, with no MFMA beside it)
        stage_m(buf ^ 1, m, g);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const f16x8 hi = fragh(ah[4 * s], ah[4 * s + 1], ah[4 * s + 2], ah[4 * s + 3]);
            const f16x8 lo = fragh(al[4 * s], al[4 * s + 1], al[4 * s + 2], al[4 * s + 3]);
#pragma unroll
            for (int c = 0; c < XC; ++c) {
                f16x8 bx;
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    const int R0 = 32 * xrh + 16 * s + 8 * hf + 4 * (g4 >> 1);
                    const f16x4 t = read_tr(smimg[buf] + (R0 + q) * LDZ + 32 * (xc0 + c) + 16 * (g4 & 1) + 4 * pp);
#pragma unroll
                    for (int j = 0; j < 4; ++j) bx[4 * hf + j] = t[j];
                }
                G1[c] = mfmah(hi, bx, G1[c]);
                G1[c] = mfmah(lo, bx, G1[c]);
            }
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 4 * XC, 0);
#pragma unroll
        for (int i = 0; i < 4 * XC; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    if (j0 < P) fetch_m(j0, ma, ga);
    fetch_x(j0);
    if (j0 + J < P) fetch_m(j0 + J, mb, gb);
    // (r14) the weight fragments and the first two tiles' operands are in flight while set_gscale loads, reduces and meets its
    // barrier: one round trip to memory in front of the tile loop, not two in a row
    gsc = set_gscale(p.part_m, set, p.n_sets, J, gred, tid);
    stage_m(0, ma, ga), stage_x(j0, 0);
    __syncthreads();
#ifdef AVD_STAMP
    unsigned long long tacc[4] = {0, 0, 0, 0}, tlast = __builtin_amdgcn_s_memtime();
#define STAMP(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); tacc[i] += t_ - tlast; tlast = t_; }
#else
#define STAMP(i)
#endif
    for (int pi = j0; pi < P; pi += 2 * J) {
        // tile pi from buffer 0; set a takes tile pi + 2J; set b (tile pi + J) goes to buffer 1
        fetch_x(pi + J);
        if (pi + 2 * J < P) fetch_m(pi + 2 * J, ma, ga);
        STAMP(0);
        compute(0, mb, gb);
        STAMP(1);
        stage_x(pi + J, 1);
        STAMP(2);
        if (!(FSPLIT_ABL(p.abl) & 2)) __syncthreads();
        STAMP(3);
        if (pi + J < P) {
            // tile pi + J from buffer 1; set b takes tile pi + 3J; set a (tile pi + 2J) goes to buffer 0
            fetch_x(pi + 2 * J);
            if (pi + 3 * J < P) fetch_m(pi + 3 * J, mb, gb);
            STAMP(0);
            compute(1, ma, ga);
            STAMP(1);
            stage_x(pi + 2 * J, 0);
            STAMP(2);
            if (!(FSPLIT_ABL(p.abl) & 2)) __syncthreads();
            STAMP(3);
        }
    }
#ifdef AVD_STAMP
    if (p.stamp && blockIdx.x == 16 && lane == 0)
        for (int i = 0; i < 4; ++i) p.stamp[w * 8 + i] = tacc[i];
#endif
    // the extra pieces: row-half partials summed through LDS (the sm images are dead now), fixed order: row half 0 + row half 1
    const float dsc = 1.f / (gsc * S1);  // (G holds 2^kg S1 G: exact powers of two)
    float* comb = (float*)&smimg[0][0];  // [4 pieces of row half 1][XC][16 registers][64 lanes] <= 32 KB
    const int cidx = NET::critic ? 2 * (w >> 2) + (w & 1) : (w & 3);  // the same for a piece's two row-half waves
    if (xrh == 1) {
#pragma unroll
        for (int c = 0; c < XC; ++c)
#pragma unroll
            for (int k = 0; k < 16; ++k) comb[((cidx * XC + c) * 16 + k) * 64 + lane] = G1[c][k];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float* dst = p.partG + ((long)blockIdx.x * KG + 32 * w) * H2 + 32 * c + r;
#pragma unroll
        for (int k = 0; k < 16; ++k) dst[(long)acc_row(k, h) * H2] = G0[c][k] * dsc;
    }
    if (xrh == 0) {
#pragma unroll
        for (int c = 0; c < XC; ++c) {
            float* dst = p.partG + ((long)blockIdx.x * KG + 32 * xt) * H2 + 32 * (xc0 + c) + r;
#pragma unroll
            for (int k = 0; k < 16; ++k) dst[(long)acc_row(k, h) * H2] = (G1[c][k] + comb[((cidx * XC + c) * 16 + k) * 64 + lane]) * dsc;
        }
    }
}
template <int S, class NET>
__global__ __launch_bounds__(NT) void dw_kernel(const DwArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[DW_LDS_BYTES];
    dw_body<S, NET>(p, lds, threadIdx.x);
}

// ---- dx: dC = |g3| (sm . W2c^T), BN/ReLU backward of the first layer and its parameter sums -----------------------------------
struct DxArgs {
    NetP net;
    int n_agents, n_sets;
    const f16x8* xfh;  // packed state fragments, fp16 pairs (front_kernel: pack_x_role): the rows' first-layer input AND (lane half 0: [x_hi | x_lo])
                       // the [k][row] image of V's B operand. The first layer's SIGN is the relu mask: as bf16 pairs (2^-16) about
                       // 1e-5 of the pre-activations landed on the wrong side of zero, and one flipped row moves an entry of dW1 / db1
                       // by ~1e-3 of the tensor's max (r03, measured); fp16 pairs put z1 at the f32 level
    const float* act;  // dxa_kernel: the per-row action input [n_agents][64]
    int L_cWa, L_cba;  // dxa_kernel: offsets of the critic's action-layer weights / bias inside net.th
    const float* g3;
    const float* part_m;  // [grid][8] max |g3| per wave of the kernel that wrote g3 (set_gscale)
    const unsigned* sm;  // the packed relu mask of the head (HeadArgs::sm)
    float* partV;      // [grid][KP][16]       sum_rows (dC * mask) * [x_hi | x_lo | 1] per feature
    int abl;           // diagnostic build only (see DwArgs)
    unsigned long long* stamp;  // diagnostic build (-DAVD_STAMP) only
};
// Wave w = state feature tile w (8 tiles), both row halves. Resident: fp16 hi and lo of the tile's rows of SWC W2c as B fragments
// (reduction over the 128 columns; A = the sm rows, exact). dC comes out [row][feature] (feature on the lane) like the
// recomputed first layer: the per-feature sums over rows are per-lane sums over the registers, and the masked gradient tile,
// scaled by vs = 2^kg SWC 2^-5 (|dC_s| <= 128 x 2^13, |g3| 2^kg < 1: below 2^15, cannot overflow) and split into an fp16 pair, is
// the A operand of V = (dC * mask)^T . [x_hi | x_lo | 1] -> dW1, db1 (k order permuted as in dw_kernel; the [k][row] image of the
// inputs is staged once per tile by waves 0 and 1). r04: every operand of V an fp16 pair (were bf16 pairs: 2^-17 per row, which in
// a noise-dominated sum over rows IS the relative error of the result -- 2e-5 on cWa at 4096 x 10).
//
// (r04: the critic's 48 action features were tried INSIDE this kernel, as one extra 32 x 32 unit per wave every second tile from
// the sm image in LDS -- correct, and slower than the two kernels: 409 us against 229 + 91. One barrier per tile makes every tile
// wait for the four waves that carry a unit, the unit is a serial chain -- LDS reads, 16 dependent MFMAs, ~150 VALU -- that no
// other wave of the workgroup can overlap, and its 20 persistent registers came back as scratch reloads in the tile loop. They
// stay in dxa_kernel.)
constexpr int DX_LDZ = 136;
constexpr int DX_LDS_BYTES = 2 * TILE * DX_LDZ * (int)sizeof(f16) + 3 * 2 * 32 * 32 * (int)sizeof(f16) + 3 * TILE * (int)sizeof(float) + 8 * (int)sizeof(float);
template <int S, class NET>
__device__ __forceinline__ void dx_body(const DxArgs& p, unsigned char* lds, const int tid) {
    constexpr int KP = NET::KP, LDZ = DX_LDZ;  // 272-byte rows: conflict-free b128 row reads
    constexpr float VSH = 1.f / 32.f;
    // sm images: two buffers (read by the dC products only, all before the barrier that ends their tile); input images and row
    // factors: three (the previous tile's row half 1 is still read after the barrier that publishes the next one: see the loop)
    f16(*smimg)[TILE * LDZ] = (f16(*)[TILE * LDZ]) lds;                                       // [2][TILE * LDZ]
    f16(*xt)[2][32 * 32] = (f16(*)[2][32 * 32])(lds + 2 * TILE * LDZ * sizeof(f16));         // [3][2][32 * 32] per slot, per row half: [k column][row]
    float(*g3s)[TILE] = (float(*)[TILE])(xt + 3);                                             // [3][TILE]
    float* gred = (float*)(g3s + 3);                                                          // [8]
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, r = lane & 31, h = lane >> 5, ft = w;
    const int set = blockIdx.x % p.n_sets, j0 = blockIdx.x / p.n_sets, J = gridDim.x / p.n_sets, P = p.n_agents / p.n_sets;
    const f32x16 zero16 = {};
    f16x8 wch[8], wcl[8];
    {
        const long at = ((long)set * KP + 32 * ft + r) * H2 + 8 * h;
#pragma unroll
        for (int s = 0; s < 8; ++s) wch[s] = *(const f16x8*)(p.net.Wchi + at + 16 * s), wcl[s] = *(const f16x8*)(p.net.Wclo + at + 16 * s);
    }
    // Everything behind dC runs in a SCALED domain: d_s = dC_s |g3| 2^kg / 32 = vs d with vs = 2^kg SWC / 32 (SWC: the power of two
    // on the fp16 W2c operand) -- |dC_s| <= 128 x 2^13 and |g3| 2^kg < 1 give |d_s| < 2^15: the fp16 pair of the masked gradient
    // cannot overflow -- and the per-feature sums are divided by vs once, at the end (powers of two: exact).
    const float swc = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(p.net.vec[(long)set * VEC + 2 * H2 + 2])));
    float gv, vs;  // gsc VSH, gsc swc VSH: behind set_gscale, which runs AFTER the first two tiles' fetches are out (below)
    const f16x8 wf = p.net.wf1h[((long)set * NGT_MAX + ft) * 64 + lane];  // (scaled by S1: p1 = S1 z1, U1 rescaled at the end)
    f32x16 V = zero16;
    for (int i = tid; i < 3 * 2 * 32 * 32; i += NT) {  // columns 9.. stay zero, column 8 is the ones column (bias)
        const int k = (i >> 5) & 31;
        (&xt[0][0][0])[i] = (f16)(k == 8 ? 1.f : 0.f);
    }
    // sm: thread (srow, sch) expands features [16 sch, +16) of row srow (mask_chunk16) into the fp16 image. Actor: as 1 / 0, the sign
    // of g3 rides in the row factor g3s; critic: signed by its row's g3 (gs), row factor |g3|. (The actor's form would save the
    // critic a load and eight VALU per thread and tile, but it is not bit-identical: an MFMA sum of negated products is not always
    // the negated sum -- measured, every dumped array of the bench differed.)
    const int srow = tid >> 3, sch = tid & 7;
    unsigned dm = 0;
    float gn = 0.f, gs = 0.f;
    // Every fetch reads a valid tile (past the last one: the last one again, staged into a buffer nobody reads), so the tile loop
    // has no branch but its own: the staging is scheduled into the MFMA phases below.
    auto fetch = [&](int pl) {
        if (FSPLIT_ABL(p.abl) & 1) pl = j0;
        const long agent = (long)pl * p.n_sets + set;
        dm = p.sm[(agent * TILE + srow) * 4 + (sch >> 1)];
        if (NET::critic) gs = p.g3[agent * TILE + srow];
        if (tid < TILE) gn = p.g3[agent * TILE + tid];
    };
    auto stage = [&](int buf, int slot) {
        uint4* dst = (uint4*)(smimg[buf] + srow * LDZ + 16 * sch);
        mask_chunk16(dm, sch, mask_one(gs, NET::critic), dst[0], dst[1]);
        if (tid < TILE) g3s[slot][tid] = (NET::critic ? fabsf(gn) : gn) * gv;
    };
    f16x8 xfn0 = {}, xfn1 = {};  // the rows' input fragments [x_hi | x_lo] (h = 0) / [x_hi | 1 1 0 0] (h = 1), both row halves (two
                                 // variables, not an array: LLVM merges the two image copies below into one indexed by the wave number
                                 // and then keeps the array in scratch memory)
    auto fetch_x = [&](int pl) {
        const long agent = (long)pl * p.n_sets + set;
        xfn0 = p.xfh[(agent * TILE + r) * 2 + h];
        xfn1 = p.xfh[(agent * TILE + 32 + r) * 2 + h];
    };
    auto stage_x = [&](int slot) {  // [k][row] image of [x_hi | x_lo]: the h = 0 fragments, transposed (waves 0, 1: one row half each)
        if (w < 2 && h == 0) {
            f16x8 src = xfn0;
            if (w == 1) src = xfn1;
            asm volatile("" : "+v"(src));  // (a register copy selected by the scalar wave number, not a memory index)
#pragma unroll
            for (int k = 0; k < 8; ++k) xt[slot][w][k * 32 + r] = src[k];
        }
    };
#ifdef AVD_STAMP
    unsigned long long dacc[4] = {0, 0, 0, 0}, dlast = __builtin_amdgcn_s_memtime();
#define DXSTAMP(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); dacc[i] += t_ - dlast; dlast = t_; }
#else
#define DXSTAMP(i)
#endif
    auto read_a = [&](int buf, int e, f16x8 (&smf)[8]) {
        const f16* arow = smimg[buf] + (32 * e + r) * LDZ + 8 * h;
#pragma unroll
        for (int s = 0; s < 8; ++s) smf[s] = *(const f16x8*)(arow + 16 * s);
    };
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    auto read_img = [&](const f16* img, f16x8 (&xb)[2]) {  // B operand of V from a [k][row] image
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const f16x4 lo = *(const f16x4*)(img + r * 32 + 16 * s + 4 * h);
            const f16x4 hi = *(const f16x4*)(img + r * 32 + 16 * s + 8 + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j) xb[s][j] = lo[j], xb[s][4 + j] = hi[j];
        }
    };
    auto dc_product = [&](const f16x8 (&smf)[8]) {  // dC of one row half: 16 MFMAs on one accumulator, k-steps in order
        f32x16 dc = zero16;
#pragma unroll
        for (int s = 0; s < 8; ++s) dc = mfmah(smf[s], wch[s], dc), dc = mfmah(smf[s], wcl[s], dc);
        return dc;
    };
    // BN/ReLU backward of the first layer: only the MASKED gradient is needed per element. The two unmasked per-feature sums of
    // r03 -- sum_rows dC (-> d beta1) and sum_rows dC relu(z1) (-> d gamma1): 3 of this kernel's ~8 VALU per element, and the
    // kernel is VALU-bound at 40 % of the matrix pipe -- are linear images of sums that exist anyway (r04, finalize_feat_kernel):
    //     sum_rows dC[row][f]           = sum_n W2[f][n] db2[n]                         (backprop of the row sum through the layer)
    //     sum_rows dC[row][f] relu(z1)  = sum_k W1[k][f] V[f][k] + b1[f] V[f][8]        (relu(z1) = mask z1, z1 = x . W1 + b1)
    auto backward = [&](int slot, int e, const f32x16& dc, const f32x16& p1, unsigned (&vh)[8], unsigned (&vl)[8]) {
        if (FSPLIT_ABL(p.abl) & 4) {  // (timing ablation, diagnostic build: the BN / ReLU backward + split VALU skipped, raw bits as operands: WRONG results)
#pragma unroll
            for (int m = 0; m < 8; ++m) vh[m] = __float_as_uint(dc[2 * m]) ^ __float_as_uint(p1[2 * m]), vl[m] = __float_as_uint(dc[2 * m + 1]);
            return;
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 gq = *(const float4*)(&g3s[slot][32 * e + 8 * g + 4 * h]);
            const float gg[4] = {gq.x, gq.y, gq.z, gq.w};
            float dm[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = 4 * g + j;
                dm[j] = p1[k] > 0.f ? dc[k] * gg[j] : 0.f;
            }
            split2h(dm[0], dm[1], vh[2 * g], vl[2 * g]);
            split2h(dm[2], dm[3], vh[2 * g + 1], vl[2 * g + 1]);
        }
    };
    auto v_product = [&](const unsigned (&vh)[8], const unsigned (&vl)[8], const f16x8 (&xb)[2]) {  // V += one row half: 4 MFMAs
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            V = mfmah(fragh(vh[4 * s], vh[4 * s + 1], vh[4 * s + 2], vh[4 * s + 3]), xb[s], V);
            V = mfmah(fragh(vl[4 * s], vl[4 * s + 1], vl[4 * s + 2], vl[4 * s + 3]), xb[s], V);
        }
    };
    // The tile loop is a software pipeline over row halves AND tiles. Tile t sits in sm buffer t & 1 and slot t % 3; each
    // iteration is three phases and one barrier:
    //   1: dC of row half 0 of tile t                    | backward + split VALU of row half 1 of tile t - 1
    //   2: V of row half 1 of tile t - 1, dC of half 1   | backward + split VALU of row half 0 of tile t, staging of tile t + 1
    //   3: V of row half 0 of tile t;  barrier
    // r07 issued the halves of one tile in turn: the dC of half 0 had no VALU beside it, half 1's VALU had only the 8 V MFMAs, and
    // the staging of the next tile came after all of them -- the two waves of a SIMD share the barrier, so they were always in the
    // same phase and the matrix and vector pipes hardly overlapped (5.9 k cycles per tile and SIMD for 2.7 k of MFMA). Each
    // accumulator still sees its MFMAs in the same order (V: half 0 of tile t, half 1 of tile t, half 0 of tile t + 1, ...), so the
    // results are bit-identical. The slot of tile t - 1 is read in phase 1 of iteration t, after the barrier that publishes tile
    // t; tile t + 1 is written in phase 2: a third slot keeps them apart. The sm buffers need no third: both dC of a tile come
    // before the barrier that ends its iteration.
    f16x8 xf0, xf1;  // tile t's input fragments (xfn*: tile t + 1)
    f32x16 dc1 = zero16, p11 = zero16;  // row half 1 of the previous tile, carried over the barrier
    auto iteration = [&](auto has_prev_c, int pi, int buf, int slot) {
        constexpr bool has_prev = decltype(has_prev_c)::value;
        const int pslot = slot == 0 ? 2 : slot - 1, nslot = slot == 2 ? 0 : slot + 1;
        const int nn = pi + 2 * J < P ? pi + 2 * J : (pi + J < P ? pi + J : pi);  // tile t + 2 (or the last valid one)
        DXSTAMP(0);
        // phase 1
        f16x8 smf[8], xb0[2], xb1[2];
        unsigned vh0[8], vl0[8], vh1[8], vl1[8];
        read_a(buf, 0, smf);
        const f32x16 dc0 = dc_product(smf);
        const f32x16 p10 = mfmah(xf0, wf, zero16);
        if constexpr (has_prev) {
            read_img(xt[pslot][1], xb1);
            backward(pslot, 1, dc1, p11, vh1, vl1);
            __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);
#pragma unroll
            for (int i = 0; i < 17; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        DXSTAMP(1);
        // phase 2
        if constexpr (has_prev) v_product(vh1, vl1, xb1);
        read_a(buf, 1, smf);
        read_img(xt[slot][0], xb0);
        dc1 = dc_product(smf);
        p11 = mfmah(xf1, wf, zero16);
        backward(slot, 0, dc0, p10, vh0, vl0);
        stage(buf ^ 1, nslot);
        stage_x(nslot);
        xf0 = xfn0, xf1 = xfn1;
        fetch(nn), fetch_x(nn);
        __builtin_amdgcn_sched_group_barrier(0x100, 16, 0);
#pragma unroll
        for (int i = 0; i < (has_prev ? 21 : 17); ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        // phase 3
        v_product(vh0, vl0, xb0);
        DXSTAMP(2);
        if (!(FSPLIT_ABL(p.abl) & 2)) __syncthreads();
        DXSTAMP(3);
    };
    // (r14) Start-up: the resident fragments (above), tile j0 and tile j0 + J are all requested before set_gscale's own loads, so
    // that ONE round trip to memory stands in front of the tile loop; until r14 the chain was scale -> barrier -> fragments and
    // tile j0 -> its staging -> tile j0 + J. The first tile waits in a second set of registers until the scale is known.
    unsigned dm0 = 0;
    float gn0 = 0.f, gs0 = 0.f;
    f16x8 xfa = {}, xfb = {};
    if (j0 < P) {
        fetch(j0), fetch_x(j0);
        dm0 = dm, gn0 = gn, gs0 = gs, xfa = xfn0, xfb = xfn1;
        const int n1 = j0 + J < P ? j0 + J : j0;
        fetch(n1), fetch_x(n1);
    }
    {
        const float gsc = set_gscale(p.part_m, set, p.n_sets, J, gred, tid);  // 2^kg (its barrier: also the zero / ones fill above before the first stage_x)
        gv = gsc * VSH, vs = gsc * swc * VSH;
    }
    if (j0 < P) {
        const unsigned dm1 = dm;
        const float gn1 = gn, gs1 = gs;
        const f16x8 xfc = xfn0, xfd = xfn1;
        dm = dm0, gn = gn0, gs = gs0, xfn0 = xfa, xfn1 = xfb;
        stage(0, 0), stage_x(0);
        xf0 = xfn0, xf1 = xfn1;
        dm = dm1, gn = gn1, gs = gs1, xfn0 = xfc, xfn1 = xfd;
    }
    __syncthreads();
    if (j0 < P) {
        iteration(std::false_type{}, j0, 0, 0);
        int buf = 1, slot = 1, pi = j0 + J;
        for (; pi < P; pi += J, buf ^= 1, slot = slot == 2 ? 0 : slot + 1) iteration(std::true_type{}, pi, buf, slot);
        // the last tile's row half 1
        const int pslot = slot == 0 ? 2 : slot - 1;
        f16x8 xb1[2];
        unsigned vh1[8], vl1[8];
        read_img(xt[pslot][1], xb1);
        backward(pslot, 1, dc1, p11, vh1, vl1);
        v_product(vh1, vl1, xb1);
    }
#ifdef AVD_STAMP
    if (p.stamp && blockIdx.x == 16 && lane == 0)
        for (int i = 0; i < 4; ++i) p.stamp[w * 8 + i] = dacc[i];
#endif
    const float ivs = 1.f / vs;  // (powers of two: exact)
    if (r < 16) {
        float* pv = p.partV + ((long)blockIdx.x * KP + 32 * ft) * 16 + r;
#pragma unroll
        for (int k = 0; k < 16; ++k) pv[(long)acc_row(k, h) * 16] = V[k] * ivs;
    }
}
template <int S, class NET>
__global__ __launch_bounds__(NT) void dx_kernel(const DxArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[DX_LDS_BYTES];
    dx_body<S, NET>(p, lds, threadIdx.x);
}

// ---- dxa: the critic's ACTION feature tiles (48 features = tiles 8, 9) of dC and their parameter sums ----------------------
// A quarter of dx_kernel's matrix work per tile. Every wave is on its own: wave w = (rh, ft, par) takes row half rh of feature tile
// 8 + ft of every second tile (parity par) of the workgroup and fetches its 32 packed mask rows (512 B, contiguous: lane (r, h)
// loads row r's 16 bytes) itself, TWO of its tiles ahead -- no workgroup barrier anywhere in the loop. Each lane expands its own
// A fragments from those words in registers (k-step s: word s >> 1 shifted by 8 (s & 1) + 4 h, four mask_pair; signed by its
// row's g3): the same fp16 operands that r04..r06 staged through a wave-private LDS image from an 8-KB fp16 fetch (then 66 us,
// bound by that read; r03 / early r04 read the fp16 fragments straight from global memory, 16 bytes of 32 different rows per
// load: 91-93 us. Also tried in r04: the tiles in pairs through a shared image, one barrier per pair like dx_kernel -- 118 us;
// and as extra units INSIDE dx_kernel -- 409 us against 229 + 91.)
// The action layer has ONE input (agent/model.py:68-71), so everything behind dC is f32 VALU work, no second product (r03: a
// first-layer MFMA, a [k][row] LDS image per wave, four more MFMAs and their operand splits per unit): p1 = relu(a wa + ba) as
// one fma + max -- the relu mask from an exact f32 pre-activation --, dWa = sum (dC mask) a, dba = sum (dC mask). The two
// parities and the two row halves are combined once, at the end, in a fixed order.
constexpr int DXA_LDS_BYTES = (8 * 2 * 2 * 32 + 8 * 64 * 2 + 8) * (int)sizeof(float);
template <int S>
__device__ __forceinline__ void dxa_body(const DxArgs& p, unsigned char* lds, const int tid) {
    typedef CriticS NET;
    constexpr int KP = NET::KP;
    constexpr float VSH = 1.f / 32.f;
    float(*ga)[2][2][32] = (float(*)[2][2][32]) lds;     // [8][2][2][32] per wave, per buffer: |g3| gv and a of its 32 rows
    float(*comb)[64][2] = (float(*)[64][2])(ga + 8);     // [8][64][2]
    float* gred = (float*)(comb + 8);                    // [8]
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int rh = w & 1, ftl = (w >> 1) & 1, par = w >> 2;
    const int set = blockIdx.x % p.n_sets, j0 = blockIdx.x / p.n_sets, J = gridDim.x / p.n_sets, P = p.n_agents / p.n_sets;
    const f32x16 zero16 = {};
    const int ft = 8 + ftl, f = 32 * ftl + r;  // this lane's action feature (f >= 48: padding, zero weights)
    f16x8 wch[8], wcl[8];
    {
        const long at = ((long)set * KP + 32 * ft + r) * H2 + 8 * h;
#pragma unroll
        for (int s = 0; s < 8; ++s) wch[s] = *(const f16x8*)(p.net.Wchi + at + 16 * s), wcl[s] = *(const f16x8*)(p.net.Wclo + at + 16 * s);
    }
    const float swc = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(p.net.vec[(long)set * VEC + 2 * H2 + 2])));
    const float* th = p.net.th + (long)set * p.net.th_stride;
    const float wa = f < HA ? th[p.L_cWa + f] : 0.f, ba = f < HA ? th[p.L_cba + f] : 0.f;
    float Sa = 0.f, Sb = 0.f;
    const int ntile = j0 < P ? (P - j0 + J - 1) / J : 0;
    // two register sets of prefetched operands, used alternately (k = par, par + 2, ..): the lane's row of the packed mask, its g3
    // and action. (Plain variables through macros: as arrays handed to lambdas by reference, r04's two sets ended up in scratch.)
    uint4 mA = {}, mB = {};
    float gA = 0.f, aA = 0.f, gB = 0.f, aB = 0.f;
#define DXA_FETCH(k_, m_, g_, a_)                                                                                   \
    {                                                                                                               \
        const long r0_ = (long)((j0 + (k_) * J) * p.n_sets + set) * TILE + 32 * rh;                                 \
        m_ = *(const uint4*)(p.sm + (r0_ + r) * 4);                                                                 \
        g_ = p.g3[r0_ + r], a_ = p.act[r0_ + r];                                                                    \
    }
#define DXA_PUT(buf_, g_, a_)                                                                                       \
    {                                                                                                               \
        if (h == 0) ga[w][buf_][0][r] = fabsf(g_) * gv, ga[w][buf_][1][r] = a_;                                     \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                                      \
        __builtin_amdgcn_wave_barrier();                                                                            \
    }
    auto unit = [&](int buf, const uint4 mw, float g) {
        f32x16 dc = zero16;  // [row][feature]: feature on the lane
        const unsigned m = mask_one(g, true);
        const unsigned mwt[4] = {mw.x >> (4 * h), mw.y >> (4 * h), mw.z >> (4 * h), mw.w >> (4 * h)};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            // A fragment: features 16 s + 8 h + 0..7 of the lane's row, pairs 4 h + 0..3 of chunk s (the fp16 image's row, 16 bytes)
            const unsigned d = mwt[s >> 1] >> (8 * (s & 1));
            const f16x8 af = fragh(mask_pair(d, 0, m), mask_pair(d, 1, m >> 1), mask_pair(d, 2, m >> 2), mask_pair(d, 3, m >> 3));
            dc = mfmah(af, wch[s], dc), dc = mfmah(af, wcl[s], dc);
        }
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 gq = *(const float4*)(&ga[w][buf][0][8 * q + 4 * h]), aq = *(const float4*)(&ga[w][buf][1][8 * q + 4 * h]);
            const float gg[4] = {gq.x, gq.y, gq.z, gq.w}, av[4] = {aq.x, aq.y, aq.z, aq.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float m = fmaf(av[j], wa, ba) > 0.f ? dc[4 * q + j] * gg[j] : 0.f;  // (the unmasked sums: finalize_feat_kernel, see dx_kernel)
                sa = fmaf(m, av[j], sa);
                sb += m;
            }
        }
        Sa += sa, Sb += sb;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (ga[w][buf] is rewritten by this wave's next unit)
        __builtin_amdgcn_wave_barrier();
    };
    if (par < ntile) DXA_FETCH(par, mA, gA, aA);
    if (par + 2 < ntile) DXA_FETCH(par + 2, mB, gB, aB);
    // (r14) the row factor's scale LAST: the resident fragments and both prefetched units are in flight under its loads and barrier
    const float gsc = set_gscale(p.part_m, set, p.n_sets, J, gred, tid);
    const float gv = gsc * VSH, vs = gsc * swc * VSH;  // the scaled domain of dx_kernel (nothing here needs it for range: one scale for both kernels)
    for (int k = par; k < ntile; k += 4) {
        DXA_PUT(0, gA, aA);
        {
            const uint4 mc = mA;  // (the set's registers are free again: its next fetch goes out before the unit's arithmetic)
            const float gc = gA;
            if (k + 4 < ntile) DXA_FETCH(k + 4, mA, gA, aA);
            unit(0, mc, gc);
        }
        if (k + 2 < ntile) {
            DXA_PUT(1, gB, aB);
            const uint4 mc = mB;
            const float gc = gB;
            if (k + 6 < ntile) DXA_FETCH(k + 6, mB, gB, aB);
            unit(1, mc, gc);
        }
    }
#undef DXA_FETCH
#undef DXA_PUT
    // combine: the two lane halves (16 rows each) and the four (rh, par) waves of a feature tile, fixed order; one writer per feature
    comb[w][lane][0] = Sa, comb[w][lane][1] = Sb;
    __syncthreads();
    if (rh == 0 && par == 0 && h == 0) {
        const int ws[4] = {w, w + 1, w + 4, w + 5};  // (rh 0, par 0), (rh 1, par 0), (rh 0, par 1), (rh 1, par 1)
        float t[2] = {0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 2; ++c) t[c] += comb[ws[i]][r][c] + comb[ws[i]][32 + r][c];
        const float ivs = 1.f / vs;  // (powers of two: exact)
        float* pv = p.partV + ((long)blockIdx.x * KP + 32 * ft + r) * 16;  // [feature][16]: 0 = sum (dC mask) a, 4 = its lo part (none), 8 = sum (dC mask)
#pragma unroll
        for (int c = 0; c < 9; ++c) pv[c] = c == 0 ? t[0] * ivs : (c == 8 ? t[1] * ivs : 0.f);
    }
}
template <int S>
__global__ __launch_bounds__(NT) void dxa_kernel(const DxArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[DXA_LDS_BYTES];
    dxa_body<S>(p, lds, threadIdx.x);
}

// ---- the fused launches (r15): the forward chain in one launch, the backward chain in one ---------------------------------------
// Every persistent kernel above runs the same grid, and workgroup b (set b % n_sets, j0 = b / n_sets) owns the same tiles j0, j0 + J, ..
// of its set in every one of them; the heads even share the static wave-pair map. What a kernel reads of an earlier one's output it
// reads from ITS OWN workgroup's tiles -- with two exceptions: the row factor's scale (set_gscale: part_m of every workgroup of the
// set) and the weight images of prep_kernel. So between OUT_TANH, OUT_TD, OUT_TANH_SAVE, HEAD_BOTH and the actor's seed, and between
// the five backward kernels (which do not depend on one another at all), a launch boundary orders nothing that a workgroup barrier
// does not: the bodies run back to back in one launch, and a workgroup that ends a phase early starts the next at once instead of
// idling until the slowest workgroup of the grid has drained. No workgroup ever waits for another: nothing here can hang.
// The seam between two phases is __syncthreads(): it frees the LDS buffer for the next phase's arrays, and it is HIP's guarantee that
// the global stores of the workgroup's waves in front of it (a2, y, mu, dmu, tz rows; the seed reads rows of OTHER waves of the
// workgroup) are seen by its loads behind it -- all of a workgroup's waves share one CU's L1, so no wider scope is involved; an
// agent-scope release / acquire pair would write back the XCD's L2 and invalidate the L1 at every seam for nothing. Every load of a
// phase, the one-unit-ahead fetch_in included, is issued behind the seam: the bodies are the stand-alone kernels' instruction for
// instruction, their per-wave arithmetic, tile maps and partial-sum grouping with them -- same bits.
__device__ __forceinline__ void phase_seam() {
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
}
// The thread index of one phase: the same number behind an optimisation barrier, so that what a phase derives from it -- lane offsets,
// addresses -- is computed in that phase. As one value for the whole launch the compiler shared such registers between the phases and
// kept them alive across the tile loops in between: 256 registers and spills around the loops (the phases' live ranges are disjoint).
__device__ __forceinline__ int phase_tid() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    __builtin_assume(t >= 0 && t < NT);
    return t;
}
struct FwdArgs {
    HeadArgs tanh_t, td, tanh_save, both;  // target actor -> a2, target critic -> y, actor -> mu (+ masks, tanh z), critic(s, a) and critic(s, mu)
    SeedArgs seed;                         // writes the actor's g3 into a buffer of its own (Plan::g3a): the critic's is still to be read
};
struct BwdArgs {
    DwArgs dw_c;
    DxArgs dx_c, dxa;
    DwArgs dw_a;
    DxArgs dx_a;
};
constexpr int FWD_LDS_BYTES = head_lds_bytes<CriticS, HEAD_BOTH>();
static_assert(FWD_LDS_BYTES >= head_lds_bytes<ActorS, OUT_TANH_SAVE>() && FWD_LDS_BYTES >= head_lds_bytes<CriticS, OUT_TD>(), "the largest phase");
constexpr int BWD_LDS_BYTES = DW_LDS_BYTES > DX_LDS_BYTES ? DW_LDS_BYTES : DX_LDS_BYTES;
static_assert(BWD_LDS_BYTES >= DXA_LDS_BYTES, "the largest phase");
template <int S>
__global__ __launch_bounds__(NT) void forward_kernel(const FwdArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[FWD_LDS_BYTES];
    head_body<S, ActorS, OUT_TANH>(a.tanh_t, lds, phase_tid());
    phase_seam();
    head_body<S, CriticS, OUT_TD>(a.td, lds, phase_tid());
    phase_seam();
    head_body<S, ActorS, OUT_TANH_SAVE>(a.tanh_save, lds, phase_tid());
    phase_seam();
    head_body<S, CriticS, HEAD_BOTH>(a.both, lds, phase_tid());
    phase_seam();
    seed_body(a.seed, phase_tid());
}
// (each phase carries its own set_gscale -- the critic's part_m, the actor's: both complete at the launch boundary in front -- and its
//  own partial outputs; no data flows from one phase to the next)
template <int S>
__global__ __launch_bounds__(NT) void backward_kernel(const BwdArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[BWD_LDS_BYTES];
    dw_body<S, CriticS>(a.dw_c, lds, phase_tid());
    phase_seam();
    dx_body<S, CriticS>(a.dx_c, lds, phase_tid());
    phase_seam();
    dxa_body<S>(a.dxa, lds, phase_tid());
    phase_seam();
    dw_body<S, ActorS>(a.dw_a, lds, phase_tid());
    phase_seam();
    dx_body<S, ActorS>(a.dx_a, lds, phase_tid());
}

// ---- host side ------------------------------------------------------------------------------------------------------
struct Plan {
    int grid, J;
    size_t Whi[4], Wlo[4], Wchi[2], Wclo[2], wf1h[4], vec[4], wap, a2, y, mu, dmu, g3, g3a, sm, sma, tz, t1p, s2raw, xfs, xfs2, partHs[3], partM[2],
        partV[2], partG[2], bad, smax, fflag, total;
    int n_prep1, n_pack, n_fflag;  // front_kernel: blocks of the prep1 role, of the pack role per input; front flag words
};
static Plan make_plan(int n_agents, int n_sets) {
    Plan pl;
    const int P = n_agents / n_sets;
    int J = cu_count() / n_sets;  // one 512-thread workgroup per CU, every workgroup bound to one set
    if (const char* e = AVD_DIAG_ENV("FSPLIT_J")) J = atoi(e);  // diagnostics
    if (J < 1) J = 1;
    if (J > P) J = P;
    pl.J = J, pl.grid = J * n_sets;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += (bytes + 255) / 256 * 256;
        return at;
    };
    for (int i = 0; i < 4; ++i) {
        const int K = (i & 1) ? CriticS::K : ActorS::K, KP = (i & 1) ? CriticS::KP : ActorS::KP;
        pl.Whi[i] = take(sizeof(f16) * (size_t)n_sets * H2 * K), pl.Wlo[i] = take(sizeof(f16) * (size_t)n_sets * H2 * K);
        pl.vec[i] = take(sizeof(float) * (size_t)n_sets * VEC);
        pl.wf1h[i] = take(16 * (size_t)n_sets * NGT_MAX * 64);
        if (i < 2) pl.Wchi[i] = take(sizeof(f16) * (size_t)n_sets * KP * H2), pl.Wclo[i] = take(sizeof(f16) * (size_t)n_sets * KP * H2);
    }
    pl.wap = take(4 * (size_t)n_sets * 48);
    const size_t rows = (size_t)n_agents * TILE;
    pl.a2 = take(4 * rows), pl.y = take(4 * rows), pl.mu = take(4 * rows), pl.dmu = take(4 * rows), pl.g3 = take(4 * rows);
    pl.g3a = take(4 * rows);  // the actor's row factor (its seed runs in the forward launch, before the critic's backward pass has read g3)
    pl.sm = take(16 * rows);   // the critic's relu masks, one bit per element (HEAD_BOTH)
    pl.sma = take(16 * rows);  // the actor's (OUT_TANH_SAVE: written before the critic's are used)
    pl.tz = take(4 * rows);
    pl.t1p = take(2 * 4 * (size_t)n_sets * CriticS::K * H2), pl.s2raw = take(2 * 4 * (size_t)n_sets * H2);  // (per net)
    pl.xfs = take(32 * rows), pl.xfs2 = take(32 * rows);
    for (int i = 0; i < 2; ++i) {
        const int KP = i ? CriticS::KP : ActorS::KP, KG = i ? CriticS::KG : ActorS::KG;
        pl.partM[i] = take(4 * (size_t)pl.grid * 8);
        pl.partV[i] = take(4 * (size_t)pl.grid * KP * 16);
        pl.partG[i] = take(4 * (size_t)pl.grid * KG * H2);
    }
    for (int i = 0; i < 3; ++i) pl.partHs[i] = take(4 * (size_t)pl.grid * 8 * 2);
    // nothing below is ever zeroed from the host: the front launch writes every word of it that a later kernel reads
    pl.n_prep1 = (NGT_MAX * 4 * n_sets + 3) / 4, pl.n_pack = (int)((2 * rows + 255) / 256);
    pl.n_fflag = 4 * (pl.n_prep1 + 2 * pl.n_pack);
    pl.bad = take(sizeof(int));
    pl.smax = take(sizeof(unsigned) * 4 * (size_t)n_sets * SCALE_SLICES * 2);
    pl.fflag = take(sizeof(unsigned) * (size_t)pl.n_fflag);
    pl.total = o;
    return pl;
}
static int check_shape(const avd_mlp_layout* L, int n_agents, int n_sets, const char* who) {
    AVD_REQUIRE(L, "%s: null layout", who);
    if (L->H1 != H1 || L->H2 != H2 || L->Ha != HA || L->A != 1 || (L->S != 3 && L->S != 4) || L->B != TILE) {
        set_error("%s: serves the reference widths only (layer1 256, layer2 128, action layer 48, A = 1, S in {3, 4}, B = 64); "
                  "got H1=%d H2=%d Ha=%d A=%d S=%d B=%d (avd_learn_shared_bf16 takes other widths)",
                  who, L->H1, L->H2, L->Ha, L->A, L->S, L->B);
        return AVD_E_UNSUPPORTED;
    }
    AVD_REQUIRE(n_sets > 0 && n_sets <= 64 && n_agents > 0 && n_agents % n_sets == 0, "%s: n_agents=%d n_sets=%d", who, n_agents,
                n_sets);
    return AVD_OK;
}

// The chain in two phases over one workspace (avd_learn_set_split_critic / _actor; avd_learn_set_split_f16x3 = both):
//   CRITIC: operand preparation, targets, mu, critic loss + gradients + the action gradient d q / d mu, finalize of the critic block
//   ACTOR : actor gradients from the d mu the critic phase left in the workspace, finalize of the actor block
// so that a multi-GPU caller can put the critic block's all-reduce on a side stream while the actor phase still runs
// (avddpg_amd/trainer.py; workers/trainer.py:400-431 averages the two gradient lists independently).
// Fifteen launches and no other stream operation in the single call as r09 left it (seven since r15, below; r08 issued 21: two memsets --
// three fills -- and 18 launches):
//   front_kernel (scale | prep1 | slab and *bad zeroing | pack_x, roles by block range: ~30 us where the five operations it replaces
//   took 54), prep_kernel, the four heads, dw / dx / dxa of the critic, actor_seed, dw / dx of the actor, then finalize in three
//   (fset.hip launch_finalize: column items; W2 rows | feature items; t1 -- 41 us where four launches took 48). Until r15 every
//   dependence was a launch boundary (r15, below: only the cross-WORKGROUP ones need one); the workspace and the slab may hold anything when
//   a call begins (tests/test_gpu_fsplit_glue.py).
//   Same box, 400-learn rounds alternated: 1785.5-1786.5 -> 1754.6-1757.0 us per learn (profiles/r09_glue_ab_learn_time.txt).
//   r14: what a workgroup of the ten persistent kernels does in front of its first tile. The heads filled their LDS weight image in a
//   rolled loop of load, wait, store -- 16 (actor) / 19 (critic) dependent round trips per thread, all workgroups of a set on the same
//   lines, the tables and the first fetch behind it; dw / dx / dxa ran set_gscale (loads, a reduction, a barrier) BEFORE they asked for
//   their resident fragments and first tiles. Now every load in front of the first barrier is requested before the first wait (heads:
//   21-28 in flight, the image held in registers the accumulators do not need yet) and set_gscale runs behind the requests. No
//   arithmetic, tile map or LDS layout changed: same bits (profiles/r14_startup_bit_identity.txt), same registers, no scratch
//   (r14_startup_static.txt). Heads' start-up 12.4-16.9 k -> 6.6-8.0 k cycles, 2.6-4.1 % -> 1.3-2.2 % of the kernel (r14_startup_stamps.txt);
//   same box, 400-learn rounds alternated: 1775.7-1780.6 -> 1727.4-1731.0 us per learn (r14_startup_ab_learn_time.txt).
//   Not done: finalize in TWO launches -- finalize_w2 is not independent of the column items (it adds sh1 * db2 read back from the
//   slab), so the column items keep a launch of their own.
//   r15: seven launches in the plain single call. Who reads what of whom, in the chain between prep and finalize:
//       consumer                      reads                         produced by                    scope
//       OUT_TD                        a2 rows                       OUT_TANH                       same workgroup, same tiles (same wave)
//       HEAD_BOTH                     mu, y rows                    OUT_TANH_SAVE, OUT_TD          same workgroup (same wave)
//       actor seed                    dmu, tz rows                  HEAD_BOTH, OUT_TANH_SAVE       same workgroup (other waves)
//       dw / dx / dxa (both nets)     sm, g3 rows of their tiles    heads / seed                   same workgroup
//       dw / dx / dxa                 part_m of the whole set       every workgroup of the set     SET-WIDE  (set_gscale)
//       finalize_*                    all partials                  every workgroup                SET-WIDE
//       heads                         weight images, tables         prep_kernel                    GLOBAL
//   dw<Critic>, dx<Critic>, dxa, dw<Actor>, dx<Actor> do not depend on one another. Three points need a device-wide boundary -- after
//   prep, after the last writer of part_m, before finalize -- where the chain had eleven. The eight others are now workgroup barriers
//   inside forward_kernel (four heads + the seed) and backward_kernel (five phases): above, "the fused launches". The seed runs before the
//   critic's backward pass now and writes the actor's row factor into a buffer of its own (Plan::g3a; the two-phase calls use it too).
//   What a boundary costs cannot be read from a kernel trace: the profiler's start stamp of a dispatch IS the end stamp of the one before
//   (every gap 0.00 us, profiles/r15_launch_boundaries_parent.txt) -- drain, end-of-kernel cache work, dispatch and start-up are all
//   inside the durations. The A/B is the measurement: same box, 400-learn rounds alternated, 1803.5-1805.0 -> 1771.0-1777.4 us per learn
//   (-29.2 us = -1.6 %: 3.6 us per boundary removed; profiles/r15_fused_launches_ab_learn_time.txt), same bits
//   (r15_fused_launches_bit_identity.txt, tests/test_gpu_fsplit_fused_launches.py against the two-phase calls, which keep the stand-alone
//   launches), 236 / 224 registers, no scratch, LDS of the largest phase, every tile loop the stand-alone kernel's instructions
//   (r15_fused_launches_static.txt). The seams are workgroup barriers, not the agent-scope release / acquire pairs first planned: no
//   dependence crosses a workgroup, and an agent-scope pair costs more per seam (L2 write-back, L1 invalidate) than the boundary it replaces.
enum Phase { PH_CRITIC = 1, PH_ACTOR = 2, PH_BOTH = 3, PH_TD = 4 };  // PH_TD: the TD-only call (alone, never or'ed with the others)
// What an entry point of the split learner asks for ("host side"). Every avd_learn_set_split_* wrapper makes one
// (AVD_SPLIT_CALL), attaches its variant's parts and hands it to split_run: the one place with the checks, the plan and the dispatch on S.
struct SplitCall {
    int phases;       // a Phase
    const char* who;  // the entry point, for messages
    const avd_mlp_layout* lay;
    int n_agents, n_sets;
    const float *theta, *stats, *theta_t, *stats_t, *s, *a, *r, *s2, *aw;  // (the actor phase alone: theta, stats and s only)
    float gamma, high, *grads, *losses;
    unsigned char* ws;
    size_t ws_bytes;
    hipStream_t st;
    const AnchorArgs* an;   // the anchored seed's own arguments, or null: actor_seed_kernel
    const SmoothArgs* smo;  // target policy smoothing's, or null; sigma 0: checked like any other, and no launch
    const HpRef* hp;        // a sweep's table (each set's gamma in OUT_TD's epilogue), or null: gamma
};
#ifdef AVD_STAMP
// Diagnostic build with -DAVD_STAMP: the heads' s_memtime stamps (head_kernel: HSTAMP; workgroup 16, per wave the cycles of 0 unit start,
// 1 feature tiles, 2 epilogue, 3 start-up) land in host-visible memory, one region of 128 words per net, and AVD_FSPLIT_STAMPS=1 prints
// them after every call (profiles/r14_startup_stamps.txt).
static unsigned long long* head_stamps() {
    static unsigned long long* m = nullptr;
    if (!m && hipHostMalloc(&m, 4 * 128 * 8, hipHostMallocDefault) == hipSuccess) memset(m, 0, 4 * 128 * 8);
    return m;
}
static void print_head_stamps(hipStream_t st) {
    (void)hipStreamSynchronize(st);
    static const char* who[4] = {"actor OUT_TANH_SAVE", "critic HEAD_BOTH", "target actor OUT_TANH", "target critic OUT_TD"};
    for (int ni = 0; ni < 4; ++ni)
        for (int w = 0; w < 8; ++w) {
            const unsigned long long* s = head_stamps() + 128 * ni + 8 * w;
            fprintf(stderr, "HSTAMP %-22s wave %d: start-up %8llu  unit-start %8llu  tiles %9llu  epilogue %8llu  start-up share %.4f\n", who[ni], w,
                    s[3], s[0], s[1], s[2], (double)s[3] / (double)(s[0] + s[1] + s[2] + s[3] + 1));
        }
}
#endif
// One call, checked and planned (split_run). Every kernel-argument record of the chain is built ONCE, each by its own function from the
// call and the plan (FwdArgs: the heads' and the seed's, BwdArgs: dw's and dx's), and then issued in one of two forms: FwdArgs and BwdArgs
// whole (two launches), or member by member with the variants' launches between. Same records, so the same bits.
template <int S>
static int run(const SplitCall& c, const Plan& pl) {
    const avd_mlp_layout& L = *c.lay;
    const int n_agents = c.n_agents, n_sets = c.n_sets;
    const float *theta = c.theta, *theta_t = c.theta_t, *s = c.s, *a = c.a;
    unsigned char* const ws = c.ws;
    const hipStream_t st = c.st;
    PrepArgs pa;
    pa.L = L, pa.S = S, pa.theta = theta, pa.stats = c.stats, pa.theta_t = theta_t, pa.stats_t = c.stats_t;
    pa.wap = (unsigned*)(ws + pl.wap), pa.bad = (int*)(ws + pl.bad), pa.smax = (unsigned*)(ws + pl.smax);
    pa.fflag = (unsigned*)(ws + pl.fflag), pa.n_fflag = pl.n_fflag;
    NetP net[4];
    for (int i = 0; i < 4; ++i) {
        const bool critic = i & 1, target = i >= 2;
        pa.Whi[i] = (f16*)(ws + pl.Whi[i]), pa.Wlo[i] = (f16*)(ws + pl.Wlo[i]), pa.vec[i] = (float*)(ws + pl.vec[i]);
        pa.wf1h[i] = (f16x8*)(ws + pl.wf1h[i]);
        pa.Wchi[i] = i < 2 ? (f16*)(ws + pl.Wchi[i]) : nullptr, pa.Wclo[i] = i < 2 ? (f16*)(ws + pl.Wclo[i]) : nullptr;
        NetP& n = net[i];
        n.th = (target ? theta_t : theta) + (critic ? L.actor_size : 0), n.th_stride = L.theta_size;
        n.Whi = pa.Whi[i], n.Wlo = pa.Wlo[i], n.Wchi = pa.Wchi[i], n.Wclo = pa.Wclo[i], n.wf1h = pa.wf1h[i], n.vec = pa.vec[i], n.wap = pa.wap;
    }
    const float inv_n = 1.0f / ((float)(n_agents / n_sets) * TILE);
    const long nrows = (long)n_agents * TILE;
    f16x8 *xfs = (f16x8*)(ws + pl.xfs), *xfs2 = (f16x8*)(ws + pl.xfs2);
    int* bad = (int*)(ws + pl.bad);
    float *a2 = (float*)(ws + pl.a2), *y = (float*)(ws + pl.y), *mu = (float*)(ws + pl.mu), *dmu = (float*)(ws + pl.dmu);
    float *g3 = (float*)(ws + pl.g3), *g3a = (float*)(ws + pl.g3a);  // the critic's row factor, the actor's
    unsigned *sm = (unsigned*)(ws + pl.sm), *sma = (unsigned*)(ws + pl.sma);
    auto F = [&](size_t off) { return (float*)(ws + off); };
    const dim3 grid(pl.grid), block(NT);
    const bool td = c.phases == PH_TD;
    const int abl = AVD_DIAG_ENV("FSPLIT_ABL") ? atoi(AVD_DIAG_ENV("FSPLIT_ABL")) : 0;
    static unsigned long long* d_stamp = nullptr;  // dw / dx: the stamped diagnostic build only
#ifdef AVD_STAMP
    if (!d_stamp) (void)hipMalloc(&d_stamp, 128 * 8);
#endif
    // the head of net ni: its input rows, what rides with them, its per-row result and the masks it writes (the modes that write any)
    const auto head_args = [&](int ni, const f16x8* x, const float* act, const float* rr, const float* yin, float* out, unsigned* masks) {
        HeadArgs h;
        h.net = net[ni], h.n_agents = n_agents, h.n_sets = n_sets, h.xf = x, h.act = act, h.act2 = nullptr, h.r = rr, h.yin = yin, h.aw = c.aw;
        h.out = out, h.sm = masks, h.g3 = g3, h.dmu = dmu, h.part_s = h.part_s2 = h.part_m = nullptr, h.tz = F(pl.tz);
        h.gamma = c.gamma, h.high = c.high, h.inv_n = inv_n, h.bad = bad, h.abl = abl, h.stamp = nullptr;
#ifdef AVD_STAMP
        h.stamp = head_stamps() + 128 * ni;  // one region per head launch (net index): read back below
#endif
        return h;
    };
    FwdArgs fw;
    fw.tanh_t = head_args(2, xfs2, nullptr, nullptr, nullptr, a2, sm);
    fw.td = head_args(3, xfs2, a2, c.r, nullptr, y, sm);
    fw.tanh_save = head_args(0, xfs, nullptr, nullptr, nullptr, mu, sma);  // (the actor's masks: written before the critic's are used)
    fw.both = head_args(1, xfs, a, nullptr, y, nullptr, sm);
    // critic(s, a) and critic(s, mu) in one head (HEAD_BOTH); the TD-only call's HEAD_CRITIC has no mu input
    fw.both.act2 = td ? nullptr : mu, fw.both.part_s = F(pl.partHs[1]), fw.both.part_s2 = F(pl.partHs[2]), fw.both.part_m = F(pl.partM[1]);
    SeedArgs& sd = fw.seed;
    sd.n_agents = n_agents, sd.n_sets = n_sets, sd.dmu = dmu, sd.tz = F(pl.tz), sd.high = c.high, sd.g3 = g3a, sd.part_m = F(pl.partM[0]),
    sd.part_s = F(pl.partHs[0]);
    // the backward kernels of net ni (1 critic, 0 actor) on that net's masks and row factor: the partials are the net's own
    const auto dw_args = [&](int ni, const float* act, const unsigned* masks, const float* row) {
        DwArgs d;
        d.net = net[ni], d.n_agents = n_agents, d.n_sets = n_sets, d.x = s, d.act = act, d.g3 = row, d.part_m = F(pl.partM[ni]), d.sm = masks;
        d.partG = F(pl.partG[ni]), d.abl = abl, d.stamp = d_stamp;
        return d;
    };
    const auto dx_args = [&](int ni, const float* act, const unsigned* masks, const float* row, bool action_layer) {
        DxArgs d;
        d.net = net[ni], d.n_agents = n_agents, d.n_sets = n_sets, d.xfh = xfs, d.act = act, d.g3 = row, d.part_m = F(pl.partM[ni]), d.sm = masks;
        d.L_cWa = action_layer ? L.cWa : 0, d.L_cba = action_layer ? L.cba : 0;  // (dxa_kernel alone reads them)
        d.partV = F(pl.partV[ni]), d.abl = abl, d.stamp = d_stamp;
        return d;
    };
    BwdArgs bw;
    bw.dw_c = dw_args(1, a, sm, g3), bw.dx_c = dx_args(1, a, sm, g3, false), bw.dxa = dx_args(1, a, sm, g3, true);
    bw.dw_a = dw_args(0, nullptr, sma, g3a), bw.dx_a = dx_args(0, nullptr, sma, g3a, false);
    FinArgs fa;
    fa.L = L, fa.n_sets = n_sets, fa.J = pl.J, fa.S = S, fa.nrh = 1, fa.theta = theta, fa.stats = c.stats, fa.grads = c.grads, fa.losses = c.losses;
    fa.inv_n = inv_n, fa.partLa = F(pl.partHs[2]), fa.bad = bad;
    for (int i = 0; i < 2; ++i)
        fa.partH[i] = nullptr, fa.partHs[i] = F(pl.partHs[i]), fa.partU[i] = nullptr, fa.partV[i] = F(pl.partV[i]),
        fa.partG[i] = F(pl.partG[i]), fa.c3[i] = F(pl.vec[i]);
    fa.t1_from_g[0] = fa.t1_from_g[1] = 1, fa.t1p = F(pl.t1p), fa.s2raw = F(pl.s2raw);  // T1 of both nets: from the weight-gradient partials
    // r15: the plain single call runs its ten persistent kernels and the seed as TWO launches (forward_kernel, backward_kernel: 7
    // launches per call where there were 15). Every other form keeps the stand-alone launches: a phase alone, the smoothed call (a
    // launch of its own sits between OUT_TANH and OUT_TD), the anchored call (its own seed launch), a sweep (OUT_TD's HP instantiation), the
    // stamped diagnostic build -- and, in the diagnostic build, AVD_FSPLIT_UNFUSED=1 for A/B runs of the two forms of one library.
    const bool smooth = c.smo && c.smo->sigma != 0.f;  // sigma 0: no launch, the call IS the un-smoothed one
    bool fused = c.phases == PH_BOTH && !c.an && !smooth && !c.hp;
#ifdef AVD_STAMP
    fused = false;
#endif
    if (AVD_DIAG_ENV("FSPLIT_UNFUSED")) fused = false;
    if (c.phases & (PH_CRITIC | PH_TD)) {
        // (r05, measured and not kept: the preparation chain -- three small dependent launches over 1.5 MB of weights, ~30 us -- on a side
        //  stream beside the input packing, forked and joined by events: 1969-1978 us per learn against 1957-1961 serial on the same
        //  box; the fork / join costs more than the overlap of two sub-30-us stages returns. r09: the same overlap without a fork --
        //  the independent pieces are roles of ONE launch, front_kernel, which also does what two memsets did)
        FrontArgs fr;
        fr.pa = pa, fr.grads = c.grads, fr.n_grads = (long)n_sets * L.theta_size, fr.n_sets = n_sets;
        fr.pk.x[0] = s, fr.pk.extra[0] = a, fr.pk.outh[0] = xfs, fr.pk.x[1] = c.s2, fr.pk.extra[1] = c.r, fr.pk.outh[1] = xfs2, fr.pk.rows = nrows;
        fr.n_scale = 4 * n_sets * SCALE_SLICES, fr.n_prep1 = pl.n_prep1, fr.n_pack = pl.n_pack;
        fr.n_zero = (int)((fr.n_grads + ZERO_PER_BLOCK - 1) / ZERO_PER_BLOCK);
        hipLaunchKernelGGL(front_kernel<S>, dim3((unsigned)(fr.n_scale + fr.n_prep1 + fr.n_zero + 2 * fr.n_pack)), dim3(256), 0, st, fr);
        hipLaunchKernelGGL(prep_kernel, dim3(H2, 4, n_sets), dim3(320), 0, st, pa);
    }
    const auto launch = [&](auto kern, const auto&... args) { hipLaunchKernelGGL(kern, grid, block, 0, st, args...); };
    if (fused) {
        launch(forward_kernel<S>, fw);
        launch(backward_kernel<S>, bw);
        launch_finalize(fa, st, 0, 2);
        return check_launch("avd_learn_set_split");
    }
    // The TD-only call (avd_learn_set_split_td_f16x3) is the critic phase without what only the actor phase reads: no mu pass
    // (OUT_TANH_SAVE), and the critic head in its loss-only mode (HEAD_CRITIC: no B sweeps, no d mu). dxa stays: the action layer's
    // parameter sums are the critic's own gradients. One launch sequence serves both.
    if (c.phases & (PH_CRITIC | PH_TD)) {
        // 1-2: targets
        launch(head_kernel<S, ActorS, OUT_TANH>, fw.tanh_t);
        if (smooth) {  // target policy smoothing: a2 in place, between its writer and its only reader (csrc/smooth.hip)
            SmoothArgs q = *c.smo;
            q.n_agents = n_agents, q.a2 = a2;
            launch_target_smooth(q, st);
        }
        if (c.hp) launch(head_kernel<S, CriticS, OUT_TD, true, HpRef>, fw.td, *c.hp);  // a sweep: each set's gamma (avd_learn_set_split_hp_f16x3)
        else launch(head_kernel<S, CriticS, OUT_TD>, fw.td);
        // 3: mu -- and the actor's relu masks + tanh(z) for its backward pass (no second actor forward: r03's HEAD_ACTOR)
        if (!td) launch(head_kernel<S, ActorS, OUT_TANH_SAVE>, fw.tanh_save);
        // 4-7: critic loss and gradients; critic(s, mu) and the action gradient ride in the same launch (HEAD_BOTH; TD-only: neither)
        if (td) launch(head_kernel<S, CriticS, HEAD_CRITIC>, fw.both);
        else launch(head_kernel<S, CriticS, HEAD_BOTH>, fw.both);
        launch(dw_kernel<S, CriticS>, bw.dw_c);
        launch(dx_kernel<S, CriticS>, bw.dx_c);
        launch(dxa_kernel<S>, bw.dxa);
        // 8: the critic block of the slab (+ both losses: the actor loss is the mean of q(s, mu), summed by HEAD_BOTH) -- when the
        // caller asked for this phase alone; the single call finalizes both blocks together at its end (three launches, not six)
        // (TD-only: the actor block stays the zeros of the front launch)
        if (c.phases == PH_CRITIC || td) launch_finalize(fa, st, 1, 1);
    }
    if (c.phases & PH_ACTOR) {
        // 9-11: actor gradients: the seed from d mu and the stored tanh(z) (into g3a, as in the fused launches), then dw / dx on the stored
        // (unsigned) masks
        if (c.an) {  // the anchored seed in actor_seed_kernel's place, then the anchor loss's reducer (one wave per set)
            AnchorArgs q = *c.an;
            q.n_agents = n_agents, q.n_sets = n_sets, q.S = S, q.J = pl.J, q.dmu = dmu, q.tz = sd.tz, q.high = c.high, q.g3 = g3a;
            q.part_m = sd.part_m, q.part_s = sd.part_s, q.mu = mu, q.s = s, q.aw = c.aw, q.inv_n = inv_n, q.c = 2.f * c.an->weight * inv_n;
            q.bad = bad;
            launch_anchor_seed(q, pl.grid, st);  // (csrc/anchor.hip)
        } else
            launch(actor_seed_kernel, sd);
        launch(dw_kernel<S, ActorS>, bw.dw_a);
        launch(dx_kernel<S, ActorS>, bw.dx_a);
        // 12: the actor block of the slab (the single call: both blocks)
        launch_finalize(fa, st, 0, c.phases == PH_ACTOR ? 1 : 2);
    }
#ifdef AVD_STAMP
    if (AVD_DIAG_ENV("FSPLIT_STAMPS")) print_head_stamps(st);
#endif
    return check_launch("avd_learn_set_split");
}

}  // namespace fsplit
}  // namespace avd

using namespace avd;

// Wave-level v_mfma_f32_32x32x16_f16 instructions (32 768 FLOP each) the chain ISSUES per 64-row tile (one agent's batch), from
// the kernels' loop structure -- every product of two f32-class operands is three MFMAs on 16-bit pairs (two where one operand is
// an exact +-1 / 0 mask), first layers ride on the matrix cores too:
//   head, per 32-row unit: first layer NFT + second layer 3 x 4 column tiles x NKS k-steps
//     OUT_TANH / OUT_TANH_SAVE (actor) 8 + 192 = 200, OUT_TD (critic) 10 + 228 = 238 (r03's HEAD_ACTOR, 200 more, is gone),
//     HEAD_BOTH 8 + 192 (state part, once) + (2 + 36) (branch A) + (4 + 36) (branch B1) + 36 (B2: M) = 314
//   dw, per tile: 8 waves x (2 first-layer + 2 row halves x 2 k-steps x 4 column tiles x 2) + the extra pieces 8 x (1 + 2 x XC x 2)
//   dx, per tile: 8 waves x (2 x 16 (dC) + 2 (first layer) + 2 x 4 (V));  dxa, per tile: 4 units x 16
namespace avd { namespace fsplit {
constexpr long MFMA_PER_TILE = 2 * (200 + 238 + 200 + 314)            /* four head launches, two 32-row units per tile */
                               + 8 * (2 + 32 + 1 + 2 * 2 * 2)         /* dw critic */
                               + 8 * (2 + 32 + 1 + 2 * 1 * 2)         /* dw actor */
                               + 2 * 8 * (32 + 2 + 8)                 /* dx critic, actor */
                               + 4 * 16;                              /* dxa */
static_assert(MFMA_PER_TILE == 3296, "update DESIGN.md 3.4 and the count above together");
// The TD-only call (avd_learn_set_split_td_f16x3): OUT_TANH, OUT_TD and HEAD_CRITIC = the state part 8 + 192 and branch A 2 + 36 = 238;
// the critic's dw, dx and dxa. (Without dxa, whose 64 are the critic's action-layer sums: 2032.)
constexpr long MFMA_PER_TILE_TD = 2 * (200 + 238 + 238)               /* three head launches */
                                  + 8 * (2 + 32 + 1 + 2 * 2 * 2)      /* dw critic */
                                  + 8 * (32 + 2 + 8)                  /* dx critic */
                                  + 4 * 16;                           /* dxa */
static_assert(MFMA_PER_TILE_TD == 2096 && MFMA_PER_TILE_TD - 4 * 16 == 2032, "update DESIGN.md 3.4 and the count above together");
}}
extern "C" int avd_learn_set_split_mfma_count(const avd_mlp_layout* lay, int n_agents, int n_sets, unsigned long long* mfma_32x32x16) {
    int rc = fsplit::check_shape(lay, n_agents, n_sets, "avd_learn_set_split_mfma_count");
    if (rc) return rc;
    AVD_REQUIRE(mfma_32x32x16, "avd_learn_set_split_mfma_count: null pointer");
    *mfma_32x32x16 = (unsigned long long)fsplit::MFMA_PER_TILE * (unsigned long long)n_agents;
    return AVD_OK;
}

extern "C" int avd_learn_set_split_workspace(const avd_mlp_layout* lay, int n_agents, int n_sets, size_t* bytes) {
    int rc = fsplit::check_shape(lay, n_agents, n_sets, "avd_learn_set_split_workspace");
    if (rc) return rc;
    AVD_REQUIRE(bytes, "avd_learn_set_split_workspace: null pointer");
    *bytes = fsplit::make_plan(n_agents, n_sets).total;
    return AVD_OK;
}

// StepCall's counterpart (csrc/env.hip): SplitCall c of the wrapper it stands in, from the parameter names that the signatures share.
// gamma_: the entry's gamma, or the sweep's 0 (its kernel reads each set's own).
#define AVD_SPLIT_CALL(c, phases_, who_, gamma_)                                                                                           \
    fsplit::SplitCall c = {};                                                                                                                \
    c.phases = phases_, c.who = who_, c.lay = lay, c.n_agents = n_agents, c.n_sets = n_sets, c.theta = theta, c.stats = stats;               \
    c.theta_t = theta_t, c.stats_t = stats_t, c.s = s, c.a = a, c.r = r, c.s2 = s2, c.aw = agent_weight, c.gamma = gamma_, c.high = high;    \
    c.grads = grads, c.losses = losses, c.ws = (unsigned char*)workspace, c.ws_bytes = workspace_bytes, c.st = (hipStream_t)stream

// The parts of a call, as the wrappers gather them from their arguments (anchor_args, smooth_args) and as split_run checks them once the
// shape has passed: the refusals keep their order -- shape, anchor, smoothing, null pointers, workspace size -- all before a HIP call.
static AnchorArgs anchor_args(const float* gains, int M, int model_a, float lo, float hi, float weight, float* anchor_loss) {
    AnchorArgs an{};
    an.gains = gains, an.M = M, an.model_a = model_a, an.lo = lo, an.hi = hi, an.weight = weight, an.anchor_loss = anchor_loss;
    return an;
}
static int check_anchor_args(const char* who, int n_sets, const AnchorArgs& an) {
    AVD_REQUIRE(an.gains && an.anchor_loss, "%s: null gains / anchor_loss", who);
    AVD_REQUIRE(an.M >= 1 && n_sets % an.M == 0, "%s: n_sets=%d M=%d (n_sets must be a multiple of M >= 1)", who, n_sets, an.M);
    unsigned wbits;  // (bit tests: this file is built with -fno-honor-nans) sign clear or -0, exponent not all ones
    memcpy(&wbits, &an.weight, sizeof wbits);
    AVD_REQUIRE((wbits & 0x7f800000u) != 0x7f800000u && (!(wbits >> 31) || wbits == 0x80000000u), "%s: weight=%g (must be finite and >= 0)",
                who, (double)an.weight);
    AVD_REQUIRE(an.lo <= an.hi, "%s: lo=%g > hi=%g", who, (double)an.lo, (double)an.hi);
    return AVD_OK;
}
// what the smoothed and the TD-only entries share: the smoothing arguments, checked for sigma 0 too (no launch then: fsplit::run) --
// the 16-byte workspace check with them, for those two entries alone
static SmoothArgs smooth_args(int M, int E, float sigma, float clip, float lo, float hi, uint64_t seed, uint64_t counter, const uint64_t* seeds) {
    SmoothArgs sm{};
    sm.M = M, sm.E = E, sm.sigma = sigma, sm.clip = clip, sm.lo = lo, sm.hi = hi, sm.seed = seed, sm.counter = counter, sm.seeds = seeds;
    return sm;
}
static int check_smooth_args(const fsplit::SplitCall& c) {
    const SmoothArgs& sm = *c.smo;
    if (const int rc = check_smooth(c.who, sm)) return rc;  // (csrc/smooth.hip: built without -fno-honor-nans: plain NaN comparisons)
    AVD_REQUIRE(c.n_sets % ((long)sm.E * sm.M) == 0, "%s: n_sets=%d M=%d E=%d (n_sets must be a multiple of E x M)", c.who, c.n_sets, sm.M, sm.E);
    AVD_REQUIRE(((uintptr_t)c.ws & 15) == 0, "%s: the workspace must be 16-byte aligned", c.who);
    return AVD_OK;
}

// Every check of a call, once and in one order; then the plan, and the chain for the layout's S
static int split_run(const fsplit::SplitCall& c) {
    int rc = fsplit::check_shape(c.lay, c.n_agents, c.n_sets, c.who);
    if (!rc && c.an) rc = check_anchor_args(c.who, c.n_sets, *c.an);
    if (!rc && c.smo) rc = check_smooth_args(c);
    if (rc) return rc;
    const bool cr = c.phases & (fsplit::PH_CRITIC | fsplit::PH_TD);
    AVD_REQUIRE(c.theta && c.stats && c.s && c.grads && c.ws && (!cr || (c.theta_t && c.stats_t && c.a && c.r && c.s2)), "%s: null pointer", c.who);
    const fsplit::Plan pl = fsplit::make_plan(c.n_agents, c.n_sets);
    AVD_REQUIRE(c.ws_bytes >= pl.total, "%s: workspace %zu B < %zu B", c.who, c.ws_bytes, pl.total);
    // (padding floats of the slab are never written by finalize: the critic phase's front launch zeroes the slab, like every other
    //  gradient producer keeps them zero)
    return c.lay->S == 4 ? fsplit::run<4>(c, pl) : fsplit::run<3>(c, pl);
}

extern "C" int avd_learn_set_split_f16x3(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                                          const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                                          const float* s2, const float* agent_weight, float gamma, float high, float* grads,
                                          float* losses, void* workspace, size_t workspace_bytes, void* stream) {
    AVD_SPLIT_CALL(c, fsplit::PH_BOTH, "avd_learn_set_split_f16x3", gamma);
    return split_run(c);
}

// the whole call with the anchored seed (anchor_seed_kernel) and the per-set anchor loss
extern "C" int avd_learn_set_split_anchor_f16x3(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                                                const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                                                const float* s2, const float* agent_weight, float gamma, float high, float* grads,
                                                float* losses, void* workspace, size_t workspace_bytes, const float* gains, int M,
                                                int model_a, float lo, float hi, float weight, float* anchor_loss, void* stream) {
    AVD_SPLIT_CALL(c, fsplit::PH_BOTH, "avd_learn_set_split_anchor_f16x3", gamma);
    const AnchorArgs an = anchor_args(gains, M, model_a, lo, hi, weight, anchor_loss);
    c.an = &an;
    return split_run(c);
}

// the whole call with target policy smoothing (csrc/smooth.hip) between the target actor's head and the target critic's; gains == null:
// the un-anchored seed. sigma == 0: no launch, the call IS the un-smoothed one.
extern "C" int avd_learn_set_split_smooth_f16x3(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                                                const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                                                const float* s2, const float* agent_weight, float gamma, float high, float* grads,
                                                float* losses, void* workspace, size_t workspace_bytes, const float* gains, int M,
                                                int model_a, float lo, float hi, float weight, float* anchor_loss, float sigma,
                                                float noise_clip, uint64_t seed, uint64_t counter, const uint64_t* d_seeds, int E,
                                                void* stream) {
    AVD_SPLIT_CALL(c, fsplit::PH_BOTH, "avd_learn_set_split_smooth_f16x3", gamma);
    const AnchorArgs an = anchor_args(gains, M, model_a, lo, hi, weight, anchor_loss);
    const SmoothArgs sm = smooth_args(M, E, sigma, noise_clip, lo, hi, seed, counter, d_seeds);
    c.an = gains ? &an : nullptr, c.smo = &sm;
    return split_run(c);
}

// a hyperparameter sweep: the whole call with each weight set's gamma from d_hp (set j: row (j / set_block) % n_groups) in the TD epilogue
extern "C" int avd_learn_set_split_hp_f16x3(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                                            const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                                            const float* s2, const float* agent_weight, float high, float* grads, float* losses,
                                            void* workspace, size_t workspace_bytes, const avd_hparams* d_hp, int n_groups, int set_block,
                                            void* stream) {
    AVD_REQUIRE_HP("avd_learn_set_split_hp_f16x3", d_hp, n_groups, set_block, n_sets);
    AVD_SPLIT_CALL(c, fsplit::PH_BOTH, "avd_learn_set_split_hp_f16x3", 0.f);
    const HpRef hp{d_hp, n_groups, set_block};
    c.hp = &hp;
    return split_run(c);
}

// deprecated alias (r03's name: the operand pairs were bf16 then; every pair has been fp16 since r04)
extern "C" int avd_learn_set_split_bf16x3(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                                          const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                                          const float* s2, const float* agent_weight, float gamma, float high, float* grads,
                                          float* losses, void* workspace, size_t workspace_bytes, void* stream) {
    return avd_learn_set_split_f16x3(lay, n_agents, n_sets, theta, stats, theta_t, stats_t, s, a, r, s2, agent_weight, gamma, high, grads,
                                     losses, workspace, workspace_bytes, stream);
}

extern "C" int avd_learn_set_split_critic(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                                          const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                                          const float* s2, const float* agent_weight, float gamma, float high, float* grads,
                                          float* losses, void* workspace, size_t workspace_bytes, void* stream) {
    AVD_SPLIT_CALL(c, fsplit::PH_CRITIC, "avd_learn_set_split_critic", gamma);
    return split_run(c);
}

// The TD-only call: the critic block and the critic loss, nothing of the actor's half of the chain (fsplit::run, PH_TD). The smoothing
// arguments as in avd_learn_set_split_smooth_f16x3; sigma == 0: no smoothing launch.
extern "C" int avd_learn_set_split_td_f16x3(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                                            const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                                            const float* s2, const float* agent_weight, float gamma, float high, float* grads,
                                            float* losses, void* workspace, size_t workspace_bytes, float sigma, float noise_clip, float lo,
                                            float hi, uint64_t seed, uint64_t counter, const uint64_t* d_seeds, int E, int M, void* stream) {
    AVD_SPLIT_CALL(c, fsplit::PH_TD, "avd_learn_set_split_td_f16x3", gamma);
    const SmoothArgs sm = smooth_args(M, E, sigma, noise_clip, lo, hi, seed, counter, d_seeds);
    c.smo = &sm;
    return split_run(c);
}

extern "C" int avd_learn_set_split_actor(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                                         const float* s, float high, float* grads, void* workspace, size_t workspace_bytes, void* stream) {
    const float *theta_t = nullptr, *stats_t = nullptr, *a = nullptr, *r = nullptr, *s2 = nullptr, *agent_weight = nullptr;  // (takes none of
    float* losses = nullptr;  // these: it reads the online weights, the states and what the critic phase left in the workspace)
    AVD_SPLIT_CALL(c, fsplit::PH_ACTOR, "avd_learn_set_split_actor", 0.f);
    return split_run(c);
}
