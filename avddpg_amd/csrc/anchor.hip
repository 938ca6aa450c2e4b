// The anchored seed (avd_learn_set_split_anchor_f16x3): fsplit.hip's actor_seed_kernel with a behaviour-cloning term
// on d mu. The actor minimises La' = -mean(w q(s, mu)) + beta mean(w (mu - u*)^2), u* the clipped linear law (eval_common.h's
// linear_law: the text and the rounding order of lin.hip's controller) of set j's gain row j % M on the sampled state, so
//   d mu'[row] = d mu[row] + (2 beta / N) w (mu - u*)        g3[row] = d mu' high (1 - tanh(z)^2)
// Same tile walk, same g3 / part_m / part_s layout as actor_seed_kernel. The second word of a wave's part_s slot -- 0.f from
// actor_seed_kernel, read by nobody: finalize_small_item (fset.hip) sums word 0 of the actor's slots and word 1 of the critic's two
// only -- carries the wave's sum of w (mu - u*)^2 to anchor_loss_kernel.
#include "anchor.h"
#include "eval_common.h"

namespace avd {

constexpr int ANCHOR_NT = 512;  // fsplit.hip's workgroup: 8 waves

template <int S>
// (no contract(off) here: g3's expression must compile to actor_seed_kernel's instructions -- 1 - t^2 is one fma there -- so that weight 0
//  gives the un-anchored call's bits; linear_law carries its own)
__global__ __launch_bounds__(ANCHOR_NT) void anchor_seed_kernel(const AnchorArgs p) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int set = blockIdx.x % p.n_sets, j0 = blockIdx.x / p.n_sets, J = gridDim.x / p.n_sets, P = p.n_agents / p.n_sets;
    const float* gr = p.gains + (long)(set % p.M) * 4;
    float4 gn;
    gn.x = gr[0], gn.y = gr[1], gn.z = gr[2], gn.w = gr[3];
    float gmax = 0.f, D = 0.f, A = 0.f;
    for (int pi = j0 + w * J; pi < P; pi += 8 * J) {  // wave w: tiles j0 + w J, + 8 J, .. of the workgroup's set; lane = row
        const int agent = pi * p.n_sets + set;
        const long ri = (long)agent * TILE + lane;
        const float* row = p.s + ri * S;
        float4 ob;
        ob.x = row[0], ob.y = row[1], ob.z = row[2], ob.w = 0.f;
        if constexpr (S > 3) ob.w = row[3];
        const float ustar = fminf(fmaxf(linear_law(gn, ob, p.model_a != 0), p.lo), p.hi);  // np.clip
        const float aw = p.aw ? p.aw[agent] : 1.f;
        const float d = p.mu[ri] - ustar;
        const float dm = p.dmu[ri] + (p.c * aw) * d;
        const float t = p.tz[ri], g = dm * p.high * (1.f - t * t);
        p.g3[ri] = g;
        gmax = fmaxf(gmax, fabsf(g));
        D += g;
        A += aw * (d * d);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) gmax = fmaxf(gmax, __shfl_xor(gmax, o)), D += __shfl_xor(D, o), A += __shfl_xor(A, o);
    if (lane == 0) {
        const long slot = (long)blockIdx.x * 8 + w;
        p.part_m[slot] = gmax;
        p.part_s[slot * 2] = D, p.part_s[slot * 2 + 1] = A;
    }
}

// one wave per set: lane l sums the partials l, l + 64, .. of the set's J x 8 waves in slot order, then a fixed shuffle tree
__global__ __launch_bounds__(64) void anchor_loss_kernel(const AnchorArgs p) {
    const int set = blockIdx.x, lane = threadIdx.x;
    float A = 0.f;
    for (int i = lane; i < p.J * 8; i += 64) A += p.part_s[(((long)(i >> 3) * p.n_sets + set) * 8 + (i & 7)) * 2 + 1];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) A += __shfl_xor(A, o);
    A *= p.inv_n;
    if (*p.bad) A = __uint_as_float(0x7fc00000u);  // non-finite input: NaN out, like the gradients and the losses
    if (lane == 0) p.anchor_loss[set] = A;
}

void launch_anchor_seed(const AnchorArgs& q, int grid, hipStream_t st) {
    if (q.S == 4) hipLaunchKernelGGL(anchor_seed_kernel<4>, dim3(grid), dim3(ANCHOR_NT), 0, st, q);
    else hipLaunchKernelGGL(anchor_seed_kernel<3>, dim3(grid), dim3(ANCHOR_NT), 0, st, q);
    hipLaunchKernelGGL(anchor_loss_kernel, dim3(q.n_sets), dim3(64), 0, st, q);
}

}  // namespace avd
