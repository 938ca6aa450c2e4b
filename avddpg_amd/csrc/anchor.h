// The anchored actor seed of the split set learner (avd_learn_set_split_anchor_f16x3): what csrc/fsplit.hip hands to csrc/anchor.hip.
// The kernels live in a file of their own because they call eval_common.h's linear_law, and that header's learner constants share
// names with the set learners' (fset_common.h).
#pragma once
#include <hip/hip_runtime.h>

namespace avd {

struct AnchorArgs {
    // actor_seed_kernel's arguments (fsplit.hip SeedArgs), filled in by the chain
    int n_agents, n_sets, S, J;
    const float *dmu, *tz;
    float high;
    float *g3, *part_m, *part_s;
    // the anchor's own
    const float *mu, *s, *aw, *gains;  // mu [n_agents][64], s [n_agents][64][S] as sampled, aw [n_agents] or null, gains [M][4]
    int M, model_a;
    float lo, hi;
    float weight;        // beta (the entry's argument)
    float inv_n, c;      // 1 / N, 2 beta / N with N = P * 64
    const int* bad;      // the chain's non-finite-input flag
    float* anchor_loss;  // [n_sets]
};

// the anchored seed on `grid` workgroups of 512 (the chain's grid: J per set), then the anchor loss's reducer on n_sets waves
void launch_anchor_seed(const AnchorArgs& q, int grid, hipStream_t st);

}  // namespace avd
