// The split set learner's host checks under a host sanitizer, without a GPU: every avd_learn_set_split_* entry point once with a refused
// argument and once with arguments that pass every host check up to the workspace-size refusal (what tests/test_abi_cpu.py reaches
// from Python). No pointer is dereferenced on that path, so host memory stands in for the device's. A stand-alone program: it links the
// library's objects, built with the host sanitizer, and has its own main.
//
//   in a COPY of the tree:  make -C avddpg_amd/csrc -j8 HIPCC="/opt/rocm/bin/hipcc -Xarch_host -fsanitize=address,undefined"
//   /opt/rocm/lib/llvm/bin/clang++ -fsanitize=address,undefined -std=c++17 -I include -c tools/fsplit_host_checks.cpp -o checks.o
//   /opt/rocm/bin/hipcc -fsanitize=address,undefined checks.o COPY/avddpg_amd/csrc/build/*.o -o checks
//   ./checks                 -> "16 of 16 as expected", exit status 0, and no sanitizer report
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "avddpg_hip.h"

static int n_ok = 0, n_all = 0;
static void expect(const char* entry, const char* what, int rc, int want, const char* needle) {
    const char* msg = avd_last_error();
    const bool ok = rc == want && msg && strstr(msg, needle) && strstr(msg, entry);
    printf("%-36s %-10s rc=%d  %s  %s\n", entry, what, rc, ok ? "as expected" : "UNEXPECTED", msg ? msg : "(no message)");
    n_ok += ok, ++n_all;
}

int main() {
    avd_mlp_layout lay;
    if (avd_mlp_layout_init(&lay, 4, 1, 256, 128, 48, 64) != AVD_OK) return 2;
    alignas(16) static float buf[64];  // stands in for every device pointer: never read or written
    static uint64_t seeds[2];
    float* p = buf;
    const avd_hparams* hp = (const avd_hparams*)(const void*)buf;
    const int NA = 8, NS = 2;
    const size_t no_bytes = 0;  // a workspace that is there and too small: the last host check
    const char* shape = "n_agents=";
    const char* small = "workspace 0 B <";
    for (int pass = 0; pass < 2; ++pass) {
        const int ns = pass ? NS : 0;  // n_sets 0: refused by the shape check
        const char* what = pass ? "too small" : "refused";
        const char* needle = pass ? small : shape;
        expect("avd_learn_set_split_f16x3", what,
               avd_learn_set_split_f16x3(&lay, NA, ns, p, p, p, p, p, p, p, p, nullptr, 0.99f, 1.f, p, p, p, no_bytes, nullptr), AVD_E_INVALID, needle);
        expect("avd_learn_set_split_f16x3", pass ? "alias" : "alias ref.",  // (the deprecated name reports as the entry it forwards to)
               avd_learn_set_split_bf16x3(&lay, NA, ns, p, p, p, p, p, p, p, p, nullptr, 0.99f, 1.f, p, p, p, no_bytes, nullptr), AVD_E_INVALID, needle);
        expect("avd_learn_set_split_critic", what,
               avd_learn_set_split_critic(&lay, NA, ns, p, p, p, p, p, p, p, p, nullptr, 0.99f, 1.f, p, p, p, no_bytes, nullptr), AVD_E_INVALID, needle);
        expect("avd_learn_set_split_actor", what, avd_learn_set_split_actor(&lay, NA, ns, p, p, p, 1.f, p, p, no_bytes, nullptr), AVD_E_INVALID,
               needle);
        // the anchored call: M = 3 does not divide n_sets = 2
        expect("avd_learn_set_split_anchor_f16x3", what,
               avd_learn_set_split_anchor_f16x3(&lay, NA, NS, p, p, p, p, p, p, p, p, nullptr, 0.99f, 1.f, p, p, p, no_bytes, p, pass ? 2 : 3, 1, -1.f,
                                                1.f, 0.5f, p, nullptr),
               AVD_E_INVALID, pass ? small : "multiple of M");
        // the smoothed call, anchored too: E x M = 4 does not divide n_sets = 2
        expect("avd_learn_set_split_smooth_f16x3", what,
               avd_learn_set_split_smooth_f16x3(&lay, NA, NS, p, p, p, p, p, p, p, p, nullptr, 0.99f, 1.f, p, p, p, no_bytes, p, pass ? 1 : 2, 1, -1.f,
                                                1.f, 0.5f, p, 0.2f, 0.5f, 0, 7, seeds, 2, nullptr),
               AVD_E_INVALID, pass ? small : "multiple of E x M");
        // the TD-only call with sigma 0: its workspace must still be 16-byte aligned
        expect("avd_learn_set_split_td_f16x3", what,
               avd_learn_set_split_td_f16x3(&lay, NA, NS, p, p, p, p, p, p, p, p, nullptr, 0.99f, 1.f, p, p, pass ? (void*)p : (void*)(p + 1),
                                            no_bytes, 0.f, 0.5f, -1.f, 1.f, 3, 7, nullptr, 1, 2, nullptr),
               AVD_E_INVALID, pass ? small : "16-byte aligned");
        // the sweep's call: a null table
        expect("avd_learn_set_split_hp_f16x3", what,
               avd_learn_set_split_hp_f16x3(&lay, NA, NS, p, p, p, p, p, p, p, p, nullptr, 1.f, p, p, p, no_bytes, pass ? hp : nullptr, 2, 1, nullptr),
               AVD_E_INVALID, pass ? small : "d_hp=");
    }
    printf("%d of %d as expected\n", n_ok, n_all);
    return n_ok == n_all ? 0 : 1;
}
