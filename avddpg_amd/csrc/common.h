// Shared helpers for the gfx950 hot-path kernels: error reporting, launch checks, Philox4x32-10.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/avddpg_hip.h"

namespace avd {

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return AVD_E_LAUNCH;
    }
    return AVD_OK;
}

// Let a kernel take `bytes` of dynamic LDS (above the 48 KB a launch gets without asking), per launch: no cache to go stale per device.
inline int opt_in_dynamic_lds(const void* fn, size_t bytes, const char* who) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        set_error("%s: hipFuncSetAttribute(%zu B LDS): %s", who, bytes, hipGetErrorString(e));
        return AVD_E_LAUNCH;
    }
    return AVD_OK;
}

// Diagnostic switches (kernel / tile choices for A/B runs and cross-checks, work-skipping ablations) exist ONLY in the
// diagnostic build (`make diag`: -DAVD_DIAG -> lib/libavddpg_hip_diag.so). The shipped library reads no environment
// variable: AVD_DIAG_ENV("X") is getenv("AVD_X") there and a null constant here (the name is not even in the binary;
// tests/test_abi_cpu.py asserts it).
#ifdef AVD_DIAG
#include <stdlib.h>
#define AVD_DIAG_ENV(name) getenv("AVD_" name)
#else
#define AVD_DIAG_ENV(name) ((const char*)nullptr)
#endif

#define AVD_REQUIRE(cond, ...)        \
    do {                              \
        if (!(cond)) {                \
            avd::set_error(__VA_ARGS__); \
            return AVD_E_INVALID;     \
        }                             \
    } while (0)

// ---- hyperparameter sweeps (the *_hp_* entry points) --------------------------------------
// The per-experiment table of a sweep: weight set / agent j belongs to experiment (j / block) % n_groups. The HP twins of a kernel
// take one HpRef as a trailing variadic argument (`HpRef... hp`, empty in the scalar instantiation, whose parameter list and code
// stay those of the original kernel) and read their values from it where the kernel already knows which experiment it serves.
struct HpRef {
    const avd_hparams* hp;
    int n_groups, block;
};
template <class... H>
__device__ __forceinline__ const avd_hparams& hp_of(int j, const H&... h) {
    const HpRef r{h...};
    return r.hp[(j / r.block) % r.n_groups];
}

#define AVD_REQUIRE_HP(who, d_hp, n_groups, set_block, count)                                                                  \
    AVD_REQUIRE((d_hp) && (n_groups) >= 1 && (set_block) >= 1 && (count) > 0 && (count) % ((n_groups) * (set_block)) == 0,    \
                "%s: d_hp=%p n_groups=%d set_block=%d count=%d (the count must be a multiple of n_groups x set_block)", who,     \
                (const void*)(d_hp), (int)(n_groups), (int)(set_block), (int)(count))

// ---- Philox4x32-10 (Salmon et al. 2011), counter-based: no state in HBM -------------------
struct u32x4 {
    uint32_t x, y, z, w;
};

__host__ __device__ inline u32x4 philox4x32_10(u32x4 c, uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)M0 * c.x;
        uint64_t p1 = (uint64_t)M1 * c.z;
        u32x4 n;
        n.x = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
        n.y = (uint32_t)p1;
        n.z = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
        n.w = (uint32_t)p0;
        c = n;
        k0 += W0;
        k1 += W1;
    }
    return c;
}

// counter = (index, stream id, call counter lo, call counter hi); key = seed
__device__ inline u32x4 philox_at(uint64_t seed, uint64_t counter, uint32_t index, uint32_t stream_id) {
    u32x4 c = {index, stream_id, (uint32_t)counter, (uint32_t)(counter >> 32)};
    return philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// Box-Muller on two 32-bit words: u1 in (0,1], u2 in [0,1). Returns n0 (cos branch); n1 via pointer.
__device__ inline float box_muller(uint32_t a, uint32_t b, float* n1) {
    const float u1 = (float)((a >> 8) + 1u) * (1.0f / 16777216.0f);
    const float u2 = (float)(b >> 8) * (1.0f / 16777216.0f);
    const float rad = sqrtf(-2.0f * logf(u1));
    const float ang = 6.283185307179586f * u2;
    if (n1) *n1 = rad * sinf(ang);
    return rad * cosf(ang);
}

__device__ inline float uniform_pm1(uint32_t a) {  // U[-1, 1)
    return (float)(a >> 8) * (2.0f / 16777216.0f) - 1.0f;
}

enum PhiloxStream : uint32_t {
    STREAM_RESET_A = 1,  // reset: words -> (x0, x1) normals
    STREAM_RESET_B = 2,  // reset: x2 normal, front_accel
    STREAM_OU = 3,
    STREAM_NORMAL = 4,
    STREAM_REPLAY = 5,
    STREAM_EVAL_OBS = 6,   // disturbed scenario evaluator: sensor noise, (counter, index) = (step, vehicle)
    STREAM_EVAL_LINK = 7,  // disturbed scenario evaluator: V2V loss, word x
    STREAM_TRAIN_OBS = 8,   // training under disturbances: sensor noise, (counter, index) = (observation counter, vehicle)
    STREAM_TRAIN_LINK = 9,  // training under disturbances: V2V loss, word x
    STREAM_SEARCH = 10,     // gain search: a candidate row's four normals, (counter, index) = (generation, candidate * R + row)
    STREAM_CLONE = 11,      // warm start: a fit row's state words, (counter, index) = (fit step, vehicle index * 64 + row)
    STREAM_SMOOTH = 12,     // target policy smoothing: four rows' normals, (counter, index) = (learner call, solo agent index * 16 + q)
};

}  // namespace avd
