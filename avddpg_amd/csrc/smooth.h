// Target policy smoothing of the split set learner (avd_learn_set_split_smooth_f16x3, avd_target_smooth_f32): what
// csrc/fsplit.hip hands to csrc/smooth.hip. The kernel and its argument checks live in a file of their own: fsplit.hip is built with
// -fno-honor-nans, under which a host test for a NaN argument is not reliable, and the draw needs no constant of the set learners'.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace avd {

struct SmoothArgs {
    int n_agents;    // filled in by the chain (the stand-alone entry: its argument)
    float* a2;       // [n_agents][64] target actions, updated in place (the chain: the workspace's a2)
    int M, E;        // agent v: vehicle v % M of experiment (v / M) % E, platoon v / (E M)
    float sigma, clip, lo, hi;
    uint64_t seed, counter;
    const uint64_t* seeds;  // [E] on the device, or null: `seed` for every experiment
};

// why these arguments are refused (AVD_E_INVALID, the text set), or AVD_OK; n_agents and a2 are the caller's to check. No HIP call.
int check_smooth(const char* who, const SmoothArgs& q);

// the smoothing launch: 16 threads per agent, q.n_agents agents
void launch_target_smooth(const SmoothArgs& q, hipStream_t st);

}  // namespace avd
