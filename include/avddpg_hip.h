/*
 * avddpg_hip.h -- C ABI of the MI355X (gfx950) hot-path library libavddpg_hip.so.
 *
 * The reference (cboin1996/avddpg) has no FFI: its hot path sits behind plain
 * Python objects.  Each entry point below is the batched, device-resident
 * replacement of one of those objects' methods; the reference interface it
 * replaces is cited per function (file:line under the reference tree).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (hipMalloc'ed / torch CUDA tensor
 *    data_ptr) unless it is named h_* or is an avd_* struct passed by pointer
 *    from the host (those are read on the host at call time);
 *  - sizes are explicit; nothing is allocated, nothing synchronises: the call
 *    enqueues kernels on `stream` (a hipStream_t passed as void*) and returns;
 *  - return value: 0 = ok, < 0 = error (AVD_E_*), message in avd_last_error();
 *  - layouts: platoon-major; vehicle state x[P][L][4] float32 (one 16-byte
 *    load per vehicle); per-agent vectors [P][L]; agent id v = p*L + m.
 *  - thread-compatible: calls on different streams may run concurrently.
 */
#ifndef AVDDPG_HIP_H
#define AVDDPG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
/* The library is built with -fvisibility=hidden: these declarations are its whole dynamic symbol table. */
#pragma GCC visibility push(default)
#endif

#define AVD_MAX_L 16 /* vehicles per platoon supported by the env kernels */

#define AVD_OK 0
#define AVD_E_INVALID (-1)     /* bad argument / unsupported dimension */
#define AVD_E_LAUNCH (-2)      /* HIP launch or runtime error */
#define AVD_E_UNSUPPORTED (-3) /* shape outside what the kernels implement */

/* ---- environment constants (reference src/config.py:39-107 and the matrices of
 *      src/environment.py:390-451, built on the host in float64 and rounded once) ---- */
typedef struct avd_env_consts {
    int32_t L;             /* pl_size */
    int32_t model_a;       /* 1: Model A exogenous chain (predecessor's post-step accel, environment.py:263-267);
                              0: Model B (predecessor's action this step, :257-261) */
    int32_t can_terminate; /* config.py:75 */
    int32_t uniform_reset; /* rand_gen == uniform (util.py:67-68), device-RNG reset only */
    float max_ep, max_ev;  /* config.py:57-58 */
    float abs_action_high; /* |action_high|, environment.py:475 */
    float two_max_a;       /* 2*action_high, environment.py:476 */
    float T;               /* sample_rate */
    float ca, cb, cc, cd;  /* reward coefficients a,b,c,d config.py:52-55 */
    float re_scalar, terminal_reward;
    float stand_still, timegap;                              /* environment.py:343, 502 */
    float reset_ep_max, reset_max_ev, reset_max_a;           /* config.py:60-62 */
    float reset_ep_eval, reset_ev_eval, reset_a_eval;        /* config.py:64-66 */
    float leader_reset_a;                                    /* config.py:41 */
    float A[AVD_MAX_L][16]; /* row-major 4x4 per vehicle index */
    float B[AVD_MAX_L][4];
    float C[AVD_MAX_L][4];
} avd_env_consts;

/* ---- actor/critic parameter slab layout (agent/model.py:4-85) ----
 * One weight set = theta[theta_size] (trainable: actor block then critic block,
 * every tensor starting on a 4-float boundary, padding kept at zero) plus
 * stats[stats_size] (the non-trainable BatchNormalization moving mean/var).
 * Dense kernels are stored like Keras: W[in][out], row-major. */
typedef struct avd_mlp_layout {
    int32_t S, A, H1, H2, Ha, B;
    /* actor trainables */
    int32_t aW1, ab1, ag1, abe1, aW2, ab2, ag2, abe2, aW3, ab3;
    int32_t actor_size; /* critic block starts here */
    /* critic trainables */
    int32_t cWs, cbs, cgs, cbes, cWa, cba, cga, cbea, cW2, cb2, cg3, cbe3, cW3, cb3;
    int32_t theta_size;
    /* non-trainable stats */
    int32_t amm1, amv1, amm2, amv2, cmms, cmvs, cmma, cmva, cmm3, cmv3;
    int32_t stats_size;
} avd_mlp_layout;

const char* avd_last_error(void);
int avd_version(void);
/* 0 for the shipped library: it reads NO environment variable. 1 for the diagnostic build (`make diag`,
 * libavddpg_hip_diag.so, -DAVD_DIAG), in which AVD_* switches select kernel variants for A/B runs and cross-checks
 * (csrc/common.h AVD_DIAG_ENV). bench.py refuses a diagnostic library unless --allow-diagnostics. */
int avd_diagnostics_enabled(void);

/* Fills `out` for the given network widths. S = num_states (<= 64), A = num_actions (<= 16; the centralized
 * framework has S = 4L, A = L), H1/H2 = layer1/layer2 size, Ha = critic action layer size (config.py:112-117),
 * B = batch_size (config.py:106). The MLP kernels need H1 and Ha to be multiples of 16 and H2 a multiple of 32:
 * other widths (e.g. the centralized 307/153/57) are zero-padded by the caller -- a padded unit has zero
 * weights/bias and BN beta = mean = 0, outputs 0, receives zero gradients and stays zero under Adam. */
int avd_mlp_layout_init(avd_mlp_layout* out, int S, int A, int H1, int H2, int Ha, int B);

/* ---- environment ------------------------------------------------------------
 * Replaces Platoon.step (src/environment.py:209-241) + Vehicle.step (:460-518)
 * + get_exogenous_info (:253-269) + get_reward (:271-282) for P platoons at once.
 *   x_in  [P][L][4]  state before the step      x_out [P][L][4] state after (may alias x_in)
 *   prev_a[P][L]     prev_x[2], in/out           cum_accel [P][L] in/out or NULL (velocity/headway aux)
 *   u     [P][L]     actions                     leader_exog [P]
 *   reward[P][L]     NEGATED reward (as returned by Vehicle.step)   term [P][L] (0/1) or NULL
 *   done  [P]        any(term) per platoon       reward_mean [P] centralized mean or NULL
 *   any_done         single int32 OR-accumulated over all platoons (trainer.py:268) or NULL;
 *                    the caller zeroes it. */
int avd_env_step_f32(const avd_env_consts* d_consts, int P, int L, const float* x_in, float* x_out, float* prev_a,
                     float* cum_accel, const float* u, const float* leader_exog, float* reward, uint8_t* term,
                     uint8_t* done, float* reward_mean, int32_t* any_done, void* stream);

/* Replaces Platoon.reset / Vehicle.reset (src/environment.py:284-301, 520-559).
 *   mode 0 = training (random states), 1 = evaluator constants, 2 = rand_states=False constants.
 *   draws [P][L][3] pre-drawn, already scaled values (host-RNG parity mode) or NULL = device Philox
 *   front_accel [P] pre-drawn leader accel or NULL (device RNG: N(0, leader_reset_a)).
 *   cond        device int32 or NULL: when given, the reset happens only if *cond != 0 (the
 *               any-terminal episode break of workers/trainer.py:268-269 without a host sync). */
int avd_env_reset_f32(const avd_env_consts* d_consts, int P, int L, float* x, float* prev_a, float* cum_accel,
                      const float* draws, const float* front_accel, int mode, uint64_t seed, uint64_t counter,
                      const int32_t* cond, void* stream);

/* Per-platoon episode end -- the vectorised-environment form of the episode loop (workers/trainer.py:232-273) for the
 * device-RNG throughput mode. The reference closes the episode of ALL platoons when any is terminal (:268-269; that form is
 * avd_env_reset_f32 with `cond`). Here, called once after every step, each platoon closes its OWN episode when its step was
 * terminal (done[p], src/environment.py:237-241) or its episode has reached `limit` steps (src/config.py:89):
 *   ep_len    [P] int32  steps of the running episode (+1 per call; 0 after a close)
 *   ep_reward [P*M] f32  the episodic reward counters of :249, 321 (M = L decentralized, 1 centralized); zeroed on close
 *   ret_sum / len_sum [P] f32, ep_cnt [P] int32: per platoon, over its closed episodes, the sum of the platoon-mean episodic
 *             reward (what :510-517 appends per episode), of the episode lengths, and the episode count -- running sums the
 *             caller reads and clears whenever it reports a curve point; nothing leaves the device per step
 *   any_reset int32 or NULL: set to 1 when any platoon was closed (states changed under already-computed actor outputs)
 * A closed platoon gets fresh states exactly like avd_env_reset_f32 (mode, seed, counter; device Philox draws). */
int avd_episode_end_f32(const avd_env_consts* d_consts, int P, int L, int M, float* x, float* prev_a, float* cum_accel,
                        const uint8_t* done, int32_t* ep_len, float* ep_reward, int limit, float* ret_sum, float* len_sum,
                        int32_t* ep_cnt, int32_t* any_reset, int mode, uint64_t seed, uint64_t counter, void* stream);

/* Aux read-outs used by the evaluator/renderer (environment.py:243-251, 477, 500-503), from the
 * PRE-step state that produced them: jerk = (x2 - prev_a)/T is computed by the caller from the
 * buffers; no kernel needed. */

/* ---- exploration noise + policy ----------------------------------------------
 * OUActionNoise.__call__ (src/noise.py:14-23) for n independent scalar processes.
 *   normals [n] pre-drawn N(0,1) or NULL = device Philox (seed, counter). */
int avd_ou_step_f32(int n, float* ou_state, const float* normals, float theta, float mean, float dt, float std_dev,
                    uint64_t seed, uint64_t counter, void* stream);

/* ddpgagent.policy (agent/ddpgagent.py:6-29): action = clip(actor_out + noise, lo, hi).
 *   noise [n] or NULL (evaluator: no noise). */
int avd_policy_f32(int n, const float* actor_out, const float* noise, float lo, float hi, float* action,
                   void* stream);

/* Leader exogenous input N(0, std) per platoon per step (workers/trainer.py:291-295), device Philox. */
int avd_normal_f32(int n, float* out, float std_dev, uint64_t seed, uint64_t counter, void* stream);

/* The same draw when conf.rand_gen == 'uniform': U(-half_width, half_width) (src/util.py:55-70 get_random_val,
 * workers/trainer.py:291-295), device Philox, same (seed, counter, index) addressing as avd_normal_f32. */
int avd_uniform_f32(int n, float* out, float half_width, uint64_t seed, uint64_t counter, void* stream);

/* ---- replay buffer (src/replaybuffer.py:5-63) ----------------------------------
 * ring [n_agents][cap][row] float32, row = [s(S) a(A) r(1) s2(S)], row = 2S+A+1.
 * add: writes slot (counter % cap) of every agent (:40-47).
 *   s_prev/s_next: [n_agents] rows of `x_stride` floats, first S used (Model A hides x[3], environment.py:518). */
int avd_replay_add_f32(int n_agents, int cap, int S, int A, float* ring, int64_t counter, const float* s_prev,
                       const float* s_next, int x_stride, const float* action, const float* reward, void* stream);

/* Uniform indices with replacement in [0, range) (np.random.choice(range, B), :52-54) from device
 * Philox: idx[a][b] = mulhi32(philox(seed, counter, a, b), range). Host-RNG parity mode uploads
 * numpy's own indices instead. */
int avd_replay_indices(int n_agents, int B, int range, uint64_t seed, uint64_t counter, int32_t* idx, void* stream);

/* gather (:57-61): s[n][B][S], a[n][B][A], r[n][B], s2[n][B][S] <- ring rows idx[n][B]. */
int avd_replay_gather_f32(int n_agents, int cap, int S, int A, int B, const float* ring, const int32_t* idx, float* s,
                          float* a, float* r, float* s2, void* stream);

/* ---- actor / critic -------------------------------------------------------------
 * Weight-set addressing shared by the calls below: agent v uses set (set_mod > 0 ? v % set_mod : v)
 * -- set_mod = 0: one weight set per agent (reference `nofrl`, workers/trainer.py:100-149);
 *    set_mod = M: one set per vehicle index shared by all platoons (interfrl+gradients keeps
 *    them bit-identical, workers/trainer.py:415-425). */

/* actor(state) (agent/model.py:26-36, called at workers/trainer.py:287-289): out[v] = tanh(.)*high
 * for n_agents rows of `x_stride` floats (first S used); out [n_agents][A]. */
int avd_actor_forward_f32(const avd_mlp_layout* lay, int n_agents, int set_mod, const float* theta, const float* stats,
                          const float* state, int x_stride, float high, float* out, void* stream);

/* The same, executed only when *run_if_nonzero != 0 (a device flag, e.g. the any-terminal flag of the previous step):
 * when a fused update has already left actor(next state) in `out` (avd_learn_update_act_f32) and no reset has changed
 * the states since, the launch returns at once and `out` stays. */
int avd_actor_forward_cond_f32(const avd_mlp_layout* lay, int n_agents, int set_mod, const float* theta,
                               const float* stats, const float* state, int x_stride, float high, float* out,
                               const int32_t* run_if_nonzero, void* stream);

/* critic([state, action]) -> q[n_agents][A] (agent/model.py:63-83; the output width is num_actions, :80);
 * action [n_agents][A]; rows as above, batch 1 per agent. */
int avd_critic_forward_f32(const avd_mlp_layout* lay, int n_agents, int set_mod, const float* theta,
                           const float* stats, const float* state, int x_stride, const float* action, float* q,
                           void* stream);

/* Trainer.learn (workers/trainer.py:472-508) for n_agents batches of B rows:
 *   y = r + gamma*Q'(s2, mu'(s2)); Lc = mean((y-Q(s,a))^2); La = -mean(Q(s, mu(s)))
 *   grads [n_agents][theta_size]: actor block = dLa/dactor, critic block = dLc/dcritic (pre-update weights)
 *   losses [n_agents][2] = (Lc, La) or NULL. */
int avd_learn_f32(const avd_mlp_layout* lay, int n_agents, int set_mod, const float* theta, const float* stats,
                  const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                  const float* s2, float gamma, float high, float* grads, float* losses, void* stream);

/* Supervised learner of the actor alone (imitation warm start): one 256-thread workgroup per weight set, B = 64.
 *   s [n_sets][64][S], u_target [n_sets][64][A];  Lb = mean over 64 * A of (mu(s) - u_target)^2, mu = tanh(.) * high, BatchNormalization
 *   in the inference form as everywhere.
 *   grads [n_sets][theta_size], the whole row written: actor block = dLb/dactor in avd_learn_f32's slab layout (alignment padding
 *   zero), critic block = zeros, so the slab goes straight into avd_adam_polyak_f32.  losses [n_sets] = Lb, or NULL.
 *   theta and stats are read only. The actor forward and the actor's backward pass of avd_learn_f32's general kernel, on the exact-f32
 *   matrix cores, with dLb/dmu = 2 (mu - u_target) / (64 A) as the upstream gradient. Shape domain: avd_learn_check_shape's; a shape
 *   outside it, B != 64 and null pointers are refused on the host before any HIP call. */
int avd_actor_clone_f32(const avd_mlp_layout* lay, int n_sets, const float* theta, const float* stats, const float* s,
                        const float* u_target, float high, float* grads, float* losses, void* stream);

/* One fit step's batch for avd_actor_clone_f32 (A = 1), one thread per (set j, row b): vehicle index m = j % M, experiment
 * e = (j / M) % E (E = 1 and d_seeds = NULL without a seed table);
 *   w = philox(d_seeds ? d_seeds[e] : seed, counter, m * 64 + b, stream 11);  counter = the fit step;
 *   s[j][b][c] = uniform_pm1(w_c) * d_box[c] for c < S (S in {3, 4}; d_box [4] in device memory; uniform_pm1 = U[-1, 1) from the
 *   word's top 24 bits, as avd_uniform_f32);
 *   u_target[j][b] = fminf(fmaxf(((g0 * s0 + g1 * s1) + g2 * s2) + g3 * s3, lo), hi), g = d_gains[m] ([M][4]); under model_a (and
 *   for S = 3) the g3 term is skipped. float32 without contraction: avd_eval_linear_f32's law.
 * The draw depends on neither the number of sets per (e, m) nor E: experiment e of a seed batch draws what its solo run draws.
 * AVD_E_INVALID: S not 3 or 4, M or E < 1, n_sets not a positive multiple of E * M, E > 1 without d_seeds, lo > hi, a null pointer. */
int avd_clone_sample_f32(int n_sets, int S, int M, const float* d_gains, const float* d_box, float lo, float hi, int model_a,
                         uint64_t seed, uint64_t counter, const uint64_t* d_seeds, int E, float* s, float* u_target, void* stream);

/* Whether avd_learn_f32 / avd_learn_update_f32 serve this shape, without launching anything: AVD_OK, or the status and
 * avd_last_error() message those calls would give for it (widths outside the domain above, B != 64, or a 64-row tile of the
 * general kernel that does not fit the 160 KiB of LDS). For callers that want to refuse a configuration when it is built. */
int avd_learn_check_shape(const avd_mlp_layout* lay);

/* Which kernel avd_learn_f32 / avd_learn_update_f32 / avd_learn_update_act_f32 (hp = 0) or their *_hp_* twins (hp != 0) run for this
 * shape, decided on the host by the function those entry points call, without any HIP call: *kernel = one of AVD_LEARN_*. A shape or
 * a combination they refuse: their status and message (avd_learn_check_shape's; the HP twins serve the reference widths
 * 256 / 128 / 48, A = 1, S in {3, 4} only). The product library reads no switch; the diagnostic build's AVD_LEARN_KERNEL=fast and
 * AVD_LEARN_GENERAL are read on every call. The counterpart of avd_learn_shared_path for the per-agent learner. */
#define AVD_LEARN_LEAN 0    /* learn_kernel_l (lean.hip): the reference widths, two workgroups per CU */
#define AVD_LEARN_FAST 1    /* learn_kernel_t (mlp.hip): the reference widths, one workgroup per CU (diagnostic build only) */
#define AVD_LEARN_CEN 2     /* learn_kernel_c (cen.hip): the centralized framework at L = 3 / 5 */
#define AVD_LEARN_GENERAL 3 /* learn_kernel_g (mlp.hip): every other shape */
int avd_learn_kernel(const avd_mlp_layout* lay, int hp, int* kernel);

/* Adam x2 (critic then actor; tf.keras.optimizers.Adam defaults, workers/trainer.py:138-139, 348-349)
 * followed by ddpgagent.update_target over ALL weights incl. BN stats (agent/ddpgagent.py:31-55;
 * workers/trainer.py:352-356), fused per element, for n_sets weight sets.
 *   grads [n_sets][theta_size]; step [n_sets] = Adam iteration count AFTER this update (>= 1). */
int avd_adam_polyak_f32(const avd_mlp_layout* lay, int n_sets, float* theta, float* stats, float* theta_t,
                        float* stats_t, float* m, float* v, const float* grads, const int32_t* step, float actor_lr,
                        float critic_lr, double tau, void* stream);

/* avd_adam_polyak_f32 behind a finiteness guard, for gradient slabs that come from the 16-bit set learners
 * (avd_learn_set_split_f16x3 / avd_learn_set_fused_bf16 turn a non-finite input, or a value fp16 cannot hold, into an ALL-NaN block of
 * the slab -- loud, but one such batch fed to Adam would poison the shared weight set for good, and through the all-reduce every rank's):
 * a set whose slab starts with a NaN in its actor block or in its critic block takes NO step -- weights, moments, targets and target
 * statistics untouched, step[set] (advanced by the caller, as for avd_adam_polyak_f32) put back by one, *skipped (optional, device
 * int32) incremented. Every other set: bit-identical to avd_adam_polyak_f32. (The reference's float32 Trainer.learn has no such range
 * limit, workers/trainer.py:472-508; states are bounded by max_ep / max_ev = 20, src/config.py:56-57, far below the limits.) */
int avd_adam_polyak_guarded_f32(const avd_mlp_layout* lay, int n_sets, float* theta, float* stats, float* theta_t, float* stats_t,
                                float* m, float* v, const float* grads, int32_t* step, float actor_lr, float critic_lr, double tau,
                                int32_t* skipped, void* stream);

/* avd_adam_polyak_guarded_f32 with TD3's delayed policy updates (tr --policy_delay): the two blocks of a set count their Adam
 * iterations apart -- step[set] is the CRITIC block's count, actor_step [n_sets] (device int32) the ACTOR block's -- and `policy`
 * (by value; nothing is read back) says which kind of call this is. Both counts are advanced by the caller BEFORE a call that uses them.
 *   policy == 0, a skipped call: the critic block takes its Adam step at iteration step[set]. NO target moves -- not the critic's,
 *     not the actor's, not the BN statistics' (stats_t): targets follow only on policy calls. The actor block is neither read nor
 *     written: weights, moments, target and its part of `grads`, which may hold anything (NaN included). The launch covers the
 *     critic block's float4 groups only; actor_step is not read.
 *   policy != 0, a policy call: the critic block steps at step[set], the actor block at actor_step[set], then the soft update of both
 *     blocks and of the statistics. Element arithmetic and step sizes are avd_adam_polyak_guarded_f32's: with actor_step == step
 *     every output bit is that call's (tested).
 * Always guarded: a non-finite head of the critic block -- on a policy call also of the actor block -- leaves the set untouched, puts
 * back step[set] (on a policy call actor_step[set] too) by one and increments *skipped (optional). On a skipped call the actor block's
 * head is not looked at.
 * Refused on the host before any launch (AVD_E_INVALID): a null pointer (skipped excepted), n_sets < 1 or > 65535, a layout whose
 * blocks are not 4-float aligned or that lacks one of them, a negative or non-finite step size, tau outside (0, 1]. */
int avd_adam_polyak_delayed_f32(const avd_mlp_layout* lay, int n_sets, float* theta, float* stats, float* theta_t, float* stats_t,
                                float* m, float* v, const float* grads, int32_t* step, int32_t* actor_step, int policy, float actor_lr,
                                float critic_lr, double tau, int32_t* skipped, void* stream);

/* Fused form of avd_learn_f32 + avd_adam_polyak_f32 for one weight set per agent (reference nofrl:
 * workers/trainer.py:325-356 learn, apply_gradients x2, update_target per agent): Adam and the soft update are
 * applied where each gradient is produced, so no gradient slab is written or read back.
 *   theta      [n_agents][theta_size] pre-update weights, READ ONLY for the whole call (both gradients are taken
 *              at the pre-update actor and critic, trainer.py:492-506)
 *   theta_out  [n_agents][theta_size] receives the updated weights; must not alias theta (callers ping-pong)
 *   theta_t, stats_t, m, v  updated in place;  step [n_agents] = Adam iteration AFTER this update;
 *   grads_scratch [n_agents][theta_size] workspace: receives only the gradients of the small tensors (biases, BN
 *              gamma/beta, first/last layers, ~6 % of the slab), consumed at the end of the same launch (learn_kernel_l)
 *              or by a second, range-restricted launch (learn_kernel_t);
 *   losses [n_agents][2] or NULL.  Same result as the two separate calls, bit for bit. Any shape avd_learn_f32 serves; B = 64.
 *   By shape: the reference widths take learn_kernel_l / learn_kernel_t (update applied where each gradient is produced); the
 *   centralized framework at L = 3 / 5 (S = 4 L, A = L, widths 320 / 160 / 64) runs as a PIPELINE -- learn kernels over chunks of
 *   256 agents in `stream`, each chunk's whole-row Adam + Polyak pass on a library-owned side stream under the next chunk's learn
 *   kernel, forked off and joined back into `stream` by events (work queued on `stream` afterwards sees every result; the call is
 *   capturable); there grads_scratch receives ALL gradients. Every other shape: the general kernel's fused form. */
int avd_learn_update_f32(const avd_mlp_layout* lay, int n_agents, const float* theta, const float* stats,
                         float* theta_out, float* theta_t, float* stats_t, float* m, float* v, const int32_t* step,
                         const float* s, const float* a, const float* r, const float* s2, float gamma, float high,
                         float actor_lr, float critic_lr, double tau, float* grads_scratch, float* losses,
                         void* stream);

/* How avd_learn_update_f32 will cut `n_agents` models of this shape into launches on the current device: the centralized
 * pipeline's chunk size (one learn workgroup per CU and chunk, at most 32 chunks), chunk count and the workgroups of its
 * Adam + Polyak pass; every other shape: one launch (chunk = n_agents, 1 chunk, 0). For callers that describe what they measured. */
int avd_learn_update_plan(const avd_mlp_layout* lay, int n_agents, int* chunk_agents, int* n_chunks, int* update_groups);

/* avd_learn_update_f32 plus the agents' NEXT actions (workers/trainer.py:287-289 of the following step, before noise
 * and clipping): next_action[v] = actor(next_state[v * x_stride ..]) with the UPDATED weights, evaluated by the
 * workgroup that has just written them (A = 1). Bit-identical to avd_actor_forward_f32 on theta_out afterwards. */
int avd_learn_update_act_f32(const avd_mlp_layout* lay, int n_agents, const float* theta, const float* stats,
                             float* theta_out, float* theta_t, float* stats_t, float* m, float* v, const int32_t* step,
                             const float* s, const float* a, const float* r, const float* s2, float gamma, float high,
                             float actor_lr, float critic_lr, double tau, float* grads_scratch, float* losses,
                             const float* next_state, int x_stride, float* next_action, void* stream);

/* update_target alone (agent/ddpgagent.py:31-55): t = w*tau + t*(1-tau) over n floats. */
int avd_polyak_f32(int64_t n, const float* w, float* t, double tau, void* stream);

/* ---- federated averaging (src/server/federated.py:18-122; workers/trainer.py:400-456) ----
 * Agents are rows of g[n_out*n_in][n]; row of (o, i) = o*stride_out + i*stride_in.
 *   interfrl (average vehicle m over platoons, trainer.py:186-187): n_out=M, n_in=P, stride_out=1, stride_in=M
 *   intrafrl (average the vehicles inside platoon p, :189-190):    n_out=P, n_in=M, stride_out=M, stride_in=1
 * out[o][j] = sum_i (w[row(o,i)] or 1) * g[row(o,i)][j], i ascending (reproducible) -- the local partial
 * sum a rank contributes to the RCCL all-reduce. weights [n_out*n_in] or NULL; wsum [n_out] or NULL. */
int avd_fed_sum_f32(int n_out, int n_in, int stride_out, int stride_in, int n, const float* g, const float* weights,
                    float* out, float* wsum, void* stream);
/* finalize: unweighted (wsum == NULL): out[o][j] /= count (tf.reduce_mean, federated.py:62);
 * weighted: out[o][j] *= (1/wsum[o]) (federated.py:110). */
int avd_fed_finalize_f32(int n_out, int n, float* out, float count, const float* wsum, void* stream);
/* scatter group rows back to agents: dst[row(o,i)][:] = src[o][:] for i >= i_begin
 * (each agent receives its group's average, trainer.py:415-425, 448-456; i_begin = 1 skips the lead
 * vehicle under intra_directional_averaging, :417-418). */
int avd_fed_scatter_f32(int n_out, int n_in, int stride_out, int stride_in, int i_begin, int n, const float* src,
                        float* dst, void* stream);

/* intrafrl + gradients in ONE pass over the gradient slab (workers/trainer.py:189-190, 341-342, 417-431): the M agents of
 * platoon p (rows p*M .. p*M + M - 1 of every slab) all take the Adam + Polyak step of avd_adam_polyak_f32 with the MEAN of
 * their M gradient rows -- avd_fed_sum_f32 + avd_fed_finalize_f32 (same summation order and scaling) + avd_fed_scatter_f32 +
 * avd_adam_polyak_f32 without the averaged slab and its copy back. weights [P*M] or NULL: the weighted mean
 * (federated.py:99-118). lead_skip != 0: intra_directional_averaging -- vehicle 0 of every platoon takes no step (no Adam, no
 * soft update, :417-418; the caller must not advance its step count either) while its gradient still enters the mean.
 * step [P*M]: the agents' Adam iteration counts, already advanced by the caller for the agents that step. */
int avd_adam_polyak_intra_f32(const avd_mlp_layout* lay, int P, int M, int lead_skip, float* theta, float* stats, float* theta_t,
                              float* stats_t, float* m, float* v, const float* grads, const int32_t* step, const float* weights,
                              float actor_lr, float critic_lr, double tau, void* stream);

/* ---- federated weights in the throughput modes (workers/trainer.py:385-398, 694; src/server/federated.py:99-118) ----
 * The reference weights agent (p, m) by |1 / mean(all_ep_reward_lists[p][m][-weighted_window:])| from `training_episode >=
 * weighted_window` on. With the episode bookkeeping on the device the history lives there too:
 *   ring [P*M][W] f32  the last W closed episodes' rewards of every agent (slot = episode number % W); hist_cnt [P] int32.
 * avd_fed_history_push_f32, once per step BEFORE the episode end / conditional reset: platoon p closes when `force` (the caller's
 * step limit), or *cond != 0 (the any-terminal flag: every platoon closes, :268-269), or -- `done` given -- done[p] or
 * ep_len[p] + 1 >= limit (per-platoon episodes: what avd_episode_end_f32 is about to apply; ep_len may be NULL). A closing
 * platoon's M counters ep_reward[p*M ..] go into its ring row (and are zeroed when zero_after: the all-platoons rule has no other
 * kernel doing it). */
int avd_fed_history_push_f32(int P, int M, int W, float* ep_reward, const uint8_t* done, const int32_t* ep_len, int limit,
                             const int32_t* cond, int force, int zero_after, float* ring, int32_t* hist_cnt, void* stream);
/* avd_fed_weights_f32: w_raw [P*M] = |1 / mean(ring row)| (get_weight, trainer.py:385-398), wsum [M] = sum over platoons
 * (fed_weight_sums), agent_weight [P*M] = w P / wsum -- the per-agent factor of avd_learn_set_split_f16x3 /
 * avd_learn_set_fused_bf16 (federated.py:99-118 as a weighted mean). host_enabled 1 / 0: weighted / plain mean (all ones,
 * wsum = P); < 0: decided here -- weighted once every platoon has closed W episodes (is_weighted_fed_enabled, :694). Deterministic
 * (fixed reduction tree). A zero episodic-reward mean gives an infinite weight, as in the reference. */
int avd_fed_weights_f32(int P, int M, int W, const float* ring, const int32_t* hist_cnt, int host_enabled, float* w_raw,
                        float* agent_weight, float* wsum, void* stream);

/* ---- one launch per training step (device-RNG mode, decentralized agents) ----------------------------------------
 * advance_environment + the replay add of train_all_models (workers/trainer.py:282-322) for all P platoons:
 *   noise  = OUActionNoise.__call__()                       src/noise.py:15-19        (= avd_ou_step_f32, Philox stream OU)
 *   action = clip(actor_out + noise, low, high)             agent/ddpgagent.py:22-27  (= avd_policy_f32)
 *   exog   = get_random_val(rand_gen, reset_max_u)          workers/trainer.py:291-295 (= avd_normal_f32 / avd_uniform_f32)
 *   states, rewards, terminal = Platoon.step(action, exog)  src/environment.py:209-241 (= avd_env_step_f32)
 *   ReplayBuffer.add((prev_state, action, reward, state))   src/replaybuffer.py:36-47  (= avd_replay_add_f32; ring may be NULL)
 *   episodic reward counters += reward                      workers/trainer.py:321     (ep_reward may be NULL)
 * Same draws (seed, call counters, indices) and the same unfused float32 arithmetic as the separate entry points: results are
 * bit-identical to calling them one after the other. any_done: this step's any-terminal flag (must be 0 on entry);
 * any_done_other (optional): a second flag word that is set to 0 (two flags used alternately need no clearing launch). */
int avd_step_fused_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out, float* prev_a,
                       float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done, int32_t* any_done_other,
                       const float* actor_out, float* ou_state, float* action, float* leader_exog, float ou_theta, float ou_mean,
                       float ou_dt, float ou_std_dev, float action_low, float action_high, float exog_scale, int exog_uniform,
                       uint64_t seed, uint64_t ou_counter, uint64_t exog_counter, float* ring, int cap, int64_t replay_counter,
                       float* ep_reward, void* stream);

/* ReplayBuffer.sample (src/replaybuffer.py:49-63) in one launch: avd_replay_indices (same Philox draws, bit for bit) + 
 * avd_replay_gather_f32, rows moved whole. range = min(buffer_counter, capacity). S in {3, 4}, A = 1, B a multiple of 4. */
int avd_replay_sample_f32(int n_agents, int cap, int S, int A, int B, const float* ring, int range, uint64_t seed, uint64_t counter,
                          int32_t* idx, float* s, float* a, float* r, float* s2, void* stream);

/* ---- experiment batches: many seeds in one launch chain (the reference runs one seed per process, src/config.py:136-137) ----
 * E = n_groups independent experiments of P / E platoons each, their platoons INTERLEAVED: experiment e's platoon p is platoon
 * g = p*E + e of the batch (agent (e, p, m) is v = g*M + m). d_seeds: E uint64 seeds in device memory. Every draw the solo run
 * of experiment e makes with (seed, counter, index) is made here with (d_seeds[e], the same counter, the same index of that solo
 * run): platoon g / E, vehicle (g / E)*L + i, replay thread ((g / E)*M + m)*(B/4) + q. So each experiment's slice of every
 * output is bit-identical to the scalar entry point called with its own seed on its own P / E platoons, and with n_groups = 1 the
 * result equals the scalar entry point's. Device-RNG mode only (no host draws). P (n_agents for the replay) must be a multiple of
 * n_groups (of n_groups x agents_per_platoon). */
/* avd_step_fused_f32 with a seed table: workers/trainer.py:282-322 (src/noise.py:15-19, src/environment.py:209-241,
 * src/replaybuffer.py:36-47) for E experiments at once. */
int avd_step_fused_seeds_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out, float* prev_a,
                             float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done, int32_t* any_done_other,
                             const float* actor_out, float* ou_state, float* action, float* leader_exog, float ou_theta,
                             float ou_mean, float ou_dt, float ou_std_dev, float action_low, float action_high, float exog_scale,
                             int exog_uniform, const uint64_t* d_seeds, int n_groups, uint64_t ou_counter, uint64_t exog_counter,
                             float* ring, int cap, int64_t replay_counter, float* ep_reward, void* stream);
/* avd_env_reset_f32 with a seed table (Platoon.reset, src/environment.py:284-301, 520-559; device draws only). */
int avd_env_reset_seeds_f32(const avd_env_consts* d_consts, int P, int L, float* x, float* prev_a, float* cum_accel, int mode,
                            const uint64_t* d_seeds, int n_groups, uint64_t counter, const int32_t* cond, void* stream);
/* avd_episode_end_f32 with a seed table (workers/trainer.py:232-273 per platoon; the fresh states of src/environment.py:284-301). */
int avd_episode_end_seeds_f32(const avd_env_consts* d_consts, int P, int L, int M, float* x, float* prev_a, float* cum_accel,
                              const uint8_t* done, int32_t* ep_len, float* ep_reward, int limit, float* ret_sum, float* len_sum,
                              int32_t* ep_cnt, int32_t* any_reset, int mode, const uint64_t* d_seeds, int n_groups, uint64_t counter,
                              void* stream);
/* avd_replay_sample_f32 with a seed table (ReplayBuffer.sample, src/replaybuffer.py:49-63); agents_per_platoon = M. */
int avd_replay_sample_seeds_f32(int n_agents, int cap, int S, int A, int B, const float* ring, int range, const uint64_t* d_seeds,
                                int n_groups, int agents_per_platoon, uint64_t counter, int32_t* idx, float* s, float* a, float* r,
                                float* s2, void* stream);

/* ---- hyperparameter sweeps: per-experiment scalars in one launch chain (src/config.py:97-105 per process in the reference) ----
 * An experiment batch (above) whose experiments also differ in the scalars the kernels take: d_hp is a table of n_groups
 * avd_hparams in device memory, one per experiment. Every derived value is formed on the host exactly as the scalar entry points
 * form it, so experiment e's slice of every output is bit-identical to the scalar entry point called with row e's values.
 * The learner / optimiser entries take (d_hp, n_groups, set_block): weight set or agent j belongs to experiment
 * (j / set_block) % n_groups (per-agent sets: agent (p*E + e)*M + m; shared sets: set e*M + m; set_block = M). The count of sets
 * or agents must be a multiple of n_groups * set_block. */
typedef struct avd_hparams {
    float actor_lr, critic_lr; /* Adam step sizes */
    float tau, one_minus_tau;  /* (float)tau, (float)(1.0 - tau) of the double tau */
    float gamma;               /* TD discount */
    float ou_theta, ou_scale;  /* OU mean reversion; (float)std_dev * (float)sqrt((double)ou_dt) */
    float reserved;
} avd_hparams;

/* avd_step_fused_seeds_f32 with experiment g % n_groups's ou_theta / ou_scale from d_hp (in place of ou_theta / ou_std_dev). */
int avd_step_fused_hp_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out, float* prev_a,
                          float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done, int32_t* any_done_other,
                          const float* actor_out, float* ou_state, float* action, float* leader_exog, float ou_mean, float ou_dt,
                          float action_low, float action_high, float exog_scale, int exog_uniform, const uint64_t* d_seeds,
                          const avd_hparams* d_hp, int n_groups, uint64_t ou_counter, uint64_t exog_counter, float* ring, int cap,
                          int64_t replay_counter, float* ep_reward, void* stream);
/* avd_learn_f32 with each agent's gamma from d_hp. Reference widths only (256/128/48, A = 1, B = 64, S in {3, 4}). */
int avd_learn_hp_f32(const avd_mlp_layout* lay, int n_agents, int set_mod, const float* theta, const float* stats,
                     const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r, const float* s2,
                     float high, float* grads, float* losses, const avd_hparams* d_hp, int n_groups, int set_block, void* stream);
/* avd_learn_update_f32 / avd_learn_update_act_f32 with each agent's gamma, step sizes and tau from d_hp. Reference widths only. */
int avd_learn_update_hp_f32(const avd_mlp_layout* lay, int n_agents, const float* theta, const float* stats, float* theta_out,
                            float* theta_t, float* stats_t, float* m, float* v, const int32_t* step, const float* s, const float* a,
                            const float* r, const float* s2, float high, float* grads_scratch, float* losses, const avd_hparams* d_hp,
                            int n_groups, int set_block, void* stream);
int avd_learn_update_act_hp_f32(const avd_mlp_layout* lay, int n_agents, const float* theta, const float* stats, float* theta_out,
                                float* theta_t, float* stats_t, float* m, float* v, const int32_t* step, const float* s,
                                const float* a, const float* r, const float* s2, float high, float* grads_scratch, float* losses,
                                const float* next_state, int x_stride, float* next_action, const avd_hparams* d_hp, int n_groups,
                                int set_block, void* stream);
/* avd_adam_polyak_f32 / avd_adam_polyak_guarded_f32 with each set's step sizes and tau from d_hp (the BN statistics' soft
 * update included). */
int avd_adam_polyak_hp_f32(const avd_mlp_layout* lay, int n_sets, float* theta, float* stats, float* theta_t, float* stats_t,
                           float* m, float* v, const float* grads, const int32_t* step, const avd_hparams* d_hp, int n_groups,
                           int set_block, void* stream);
int avd_adam_polyak_guarded_hp_f32(const avd_mlp_layout* lay, int n_sets, float* theta, float* stats, float* theta_t,
                                   float* stats_t, float* m, float* v, const float* grads, int32_t* step, int32_t* skipped,
                                   const avd_hparams* d_hp, int n_groups, int set_block, void* stream);

/* avd_learn_set_split_f16x3 (the whole call) with each weight set's gamma from d_hp in the target critic's TD epilogue (set j: row
 * (j / set_block) % n_groups; n_sets a multiple of n_groups x set_block). Everything else as avd_learn_set_split_f16x3. */
int avd_learn_set_split_hp_f16x3(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                                 const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r, const float* s2,
                                 const float* agent_weight, float high, float* grads, float* losses, void* workspace, size_t workspace_bytes,
                                 const avd_hparams* d_hp, int n_groups, int set_block, void* stream);

/* ---- population-based training: move learner state from one experiment to another (csrc/pbt.hip) ----
 * Weight set j belongs to experiment (j / set_block) % n_groups, as in the *_hp_* entry points (per-agent sets: set_block = M;
 * shared sets: E*M sets, set_block = M). For each of the n_pairs pairs[i] = (src, dst) of experiment indices (host memory), the k-th
 * set of dst receives the k-th set of src: its theta, theta_t, m and v rows, its stats and stats_t rows and its step counter, bit for
 * bit; nothing else is written. Refused (AVD_E_INVALID, before any launch, every slab unchanged): n_sets not a multiple of
 * n_groups x set_block, an index out of range, src == dst, a destination listed twice, a destination that is also a source, a null
 * or misaligned (16 B) slab pointer, a theta_size / stats_size that is not a multiple of 4. No copy between host and device and no
 * synchronisation: the call may be captured in a graph. */
int avd_copy_experiment_sets_f32(const avd_mlp_layout* lay, int n_sets, int n_groups, int set_block, const int32_t* pairs, int n_pairs,
                                 float* theta, float* stats, float* theta_t, float* stats_t, float* m, float* v, int32_t* step,
                                 void* stream);

/* ---- keep the best actors seen in training (csrc/best.hip) ----
 * A unit is one rollout group of the evaluator, addressed as avd_eval_rollout_f32 addresses it: unit u owns the M weight sets
 * set_base[u] .. set_base[u]+M-1 of the online slabs theta [n_sets, theta_size] / stats [n_sets, stats_size] and the NS rollouts whose
 * counters are counters[u][k][m] (the [n_units * NS, M] array the rollout just wrote). Its score is the float32 sum of those NS * M
 * counters in memory order -- from the first element, one unfused add at a time -- divided by (float)(NS * M). The unit improves iff
 * score > best_score[u]: strict (a tie keeps the older snapshot), and a NaN score never improves; start best_score at -inf and
 * best_step at -1. For a unit that improved, the actor span theta[set][0 : actor_size] of each of its sets goes to row u*M+m of
 * best_theta [n_units*M, actor_size], the actor's BN statistics stats[set][0 : cmms] to row u*M+m of best_stats [n_units*M, cmms],
 * best_score[u] = score, best_step[u] = step_now and improved[u] = 1; for every other unit improved[u] = 0 and nothing else is written.
 * The online slabs are only read. Two launches on `stream` (the per-unit decision, then the copy that reads improved[]), no copy
 * between host and device and no synchronisation. d_set_base is the device table the kernels read, h_set_base the caller's host copy
 * of it, checked here. Refused (AVD_E_INVALID, before any launch, every array unchanged): a null or empty layout, a null pointer, a
 * slab that is not 16-byte aligned, n_units / M / NS < 1, a set_base entry outside [0, n_sets - M]. */
int avd_keep_best_f32(const avd_mlp_layout* lay, int n_units, int M, int NS, int n_sets, const int32_t* d_set_base,
                      const int32_t* h_set_base, const float* counters, const float* theta, const float* stats, int64_t step_now,
                      float* best_theta, float* best_stats, float* best_score, int64_t* best_step, int32_t* improved, void* stream);

/* actor(state) for agents that SHARE n_sets weight sets (agent v uses set v % n_sets), reference widths, on the f32 matrix
 * cores (csrc/act.hip: v_mfma_f32_32x32x2_f32, exact f32 products -- agent/model.py:26-36 in the reference's arithmetic
 * class). Same values as avd_actor_forward_f32 with set_mod = n_sets up to the f32 summation order (1e-7 relative).
 * run_if_nonzero (optional): device flag; the launch does nothing when it reads 0. */
int avd_actor_forward_set_f32(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                              const float* states, int x_stride, float high, float* out, const int32_t* run_if_nonzero, void* stream);

/* ---- shared-weight-set learner (interfrl with every step federated; BASELINE config 5) -----------------
 * When the P platoons' vehicle-m agents share one weight set (workers/trainer.py:121-128, 400-431: identical initial
 * weights + identical averaged gradients every step), Trainer.learn (:472-508) followed by the federated mean
 * (src/server/federated.py:69-92) equals ONE learn over the set's P x B rows. This entry point computes that as
 * layer-wise bf16 MFMA GEMMs (f32 accumulation, f32 parameters and gradients):
 *   theta/stats/theta_t/stats_t [n_sets][...]   weight sets (same slabs as avd_learn_f32 with set_mod = n_sets)
 *   s, s2 [n_sets][rows][S], a [n_sets][rows][1], r [n_sets][rows]   SET-MAJOR batches, rows = (n_agents / n_sets) * B
 *   row_weight [n_sets][rows] or NULL   per-row factor on both loss seeds: w_p * P / sum_p w_p on platoon p's rows gives
 *                                Server.get_weighted_avg_params (src/server/federated.py:99-118); losses stay unweighted
 *   grads [n_sets][theta_size]   mean gradient per set (what avd_fed_sum + avd_fed_finalize give for per-agent gradients)
 *   losses [n_sets][2] or NULL   mean critic / actor loss per set
 *   workspace: device scratch of at least avd_learn_shared_workspace() bytes.
 * Widths: layer1/layer2 sizes multiples of 64, action layer multiple of 16, A == 1, S in {3, 4}, B multiple of 64. */
int avd_learn_shared_workspace(const avd_mlp_layout* lay, int n_agents, int n_sets, size_t* bytes);
int avd_learn_shared_bf16(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                          const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                          const float* s2, const float* row_weight, float gamma, float high, float* grads, float* losses,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Which kernels avd_learn_shared_bf16 runs at this shape, on the host, without a HIP call (csrc/wide.hip choose_path): *flags = the
 * AVD_PATH_* bits. All five: the fused rank-one chain (BASELINE config 5); none: the layer-wise GEMM chain. */
#define AVD_PATH_FUSED_FWD 1u   /* forward passes: one fused kernel per pass, not first layer + GEMM */
#define AVD_PATH_FUSED_DELTA 2u /* critic(s, mu) as a delta on critic(s, a)'s stored activations */
#define AVD_PATH_R1 4u          /* backward passes in the rank-one form, from the stored relu mask */
#define AVD_PATH_DUAL 8u        /* critic(s, a) and critic(s, mu) in one forward pass */
#define AVD_PATH_ACT_IN_DX 16u  /* the critic's action features inside the fused input-gradient kernel */
int avd_learn_shared_path(const avd_mlp_layout* lay, int n_agents, int n_sets, unsigned* flags);

/* The same quantity -- Trainer.learn (workers/trainer.py:472-508) + federated mean over the platoons
 * (src/server/federated.py:47-63, 99-118; workers/trainer.py:400-431) for agents sharing n_sets weight sets -- at the
 * REFERENCE widths (layer1 256, layer2 128, action layer 48; src/config.py:112-117), as persistent kernels that keep the
 * second-layer weights in registers and stream the agents' batches through them (csrc/fset.hip). Differences from
 * avd_learn_shared_bf16: batches are AGENT-MAJOR, exactly what avd_replay_gather_f32 writes
 *   s, s2 [n_agents][B][S], a [n_agents][B], r [n_agents][B]; agent v uses weight set v % n_sets;
 *   agent_weight [n_agents] or NULL: factor on both loss seeds of the agent's rows (w_p * P / sum_p w_p = the weighted mean);
 * the result is deterministic (per-workgroup partial sums combined in a fixed order, no float atomics on the gradients).
 * bf16 GEMM operands, f32 accumulation / parameters / gradients. Other widths: AVD_E_UNSUPPORTED. */
int avd_learn_set_fused_workspace(const avd_mlp_layout* lay, int n_agents, int n_sets, size_t* bytes);
int avd_learn_set_fused_bf16(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                             const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                             const float* s2, const float* agent_weight, float gamma, float high, float* grads, float* losses,
                             void* workspace, size_t workspace_bytes, void* stream);

/* avd_learn_set_fused_bf16 with f32-class results (csrc/fsplit.hip): same arguments, same workspace protocol, same
 * deterministic reduction, but every matrix-product operand is carried as an fp16 PAIR hi + lo (|x - hi - lo| <= 2^-22 |x|,
 * measured worst 2^-23; static operands and row factors scaled by exact powers of two into fp16's range) and each product runs
 * as A_hi B_hi + A_lo B_hi + A_hi B_lo on v_mfma_f32_32x32x16_f16 with f32 accumulation -- two MFMAs where one operand is the
 * exact relu mask: dZ2 = g3[row] c3[n] [z2 > 0] is rank one times a mask (the output layers are one unit wide). (avd_learn_set_split_bf16x3,
 * r03's name from when the pairs were bf16, remains as a deprecated alias of avd_learn_set_split_f16x3.) The reference computes Trainer.learn in float32
 * (agent/model.py:26-36, 63-83; workers/trainer.py:472-508): this entry point is tested at 2e-5 of each gradient tensor's max
 * against the float64 oracle (tests/test_gpu_fsplit.py: measured <= 1.1e-5 at 4096 x 5; the exact-f32 kernels are asserted at
 * 1e-4), which the single-rounded bf16 operands of avd_learn_set_fused_bf16 miss by three orders of magnitude on the actor
 * gradients. A non-finite input (weights, BN statistics, s, a, r, s2) or a value that fp16 cannot hold -- a first-layer
 * activation relu(z1) >= 1023.75, |S1 w1| or |x| >= 65520 -- gives an all-NaN gradient slab (tested), never silently wrong
 * finite gradients. avd_learn_set_split_mfma_count: the wave-level v_mfma_f32_32x32x16_f16 instructions (32 768 FLOP each) one
 * call issues, from the kernels' loop structure (bench.py prices the executed matrix work from it). */
int avd_learn_set_split_mfma_count(const avd_mlp_layout* lay, int n_agents, int n_sets, unsigned long long* mfma_32x32x16);
/* The same call in two phases over ONE workspace, for callers that exchange gradients between processes
 * (workers/trainer.py:400-431 averages the critic and the actor gradient lists independently, src/server/federated.py:47-63):
 *   avd_learn_set_split_critic  operand preparation, targets, mu, critic loss and gradients, d q / d mu; writes the CRITIC block
 *                               of every set of `grads` (zeroes the slab first) and both losses;
 *   avd_learn_set_split_actor   the actor gradients from what the critic phase left in the workspace; writes the ACTOR block.
 * critic, then actor, on the same stream with the same workspace and nothing else touching it in between, is bit-identical to
 * avd_learn_set_split_f16x3 (tested). Between the two the critic block is final: a multi-GPU caller MAY start its all-reduce on a
 * side stream there (avddpg_amd/dist.py exchange_two_phase; opt-in: measured on a one-rank RCCL communicator the persistent kernels of
 * the actor phase leave the collective no CU to run beside them). */
int avd_learn_set_split_critic(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                               const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                               const float* s2, const float* agent_weight, float gamma, float high, float* grads, float* losses,
                               void* workspace, size_t workspace_bytes, void* stream);
int avd_learn_set_split_actor(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                              const float* s, float high, float* grads, void* workspace, size_t workspace_bytes, void* stream);
int avd_learn_set_split_workspace(const avd_mlp_layout* lay, int n_agents, int n_sets, size_t* bytes);
int avd_learn_set_split_f16x3(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                               const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                               const float* s2, const float* agent_weight, float gamma, float high, float* grads, float* losses,
                               void* workspace, size_t workspace_bytes, void* stream);

/* avd_learn_set_split_f16x3 with a behaviour-cloning term in the actor loss (TD3+BC's; tr --anchor):
 *   La' = -mean(w q(s, mu(s))) + weight * mean(w (mu(s) - u*(s))^2),  u* = clip(linear law(gains[j % M], s), lo, hi)
 * over the P * 64 rows of set j (w: agent_weight's factor of the row's agent, 1 when null). gains [M][4] rows (kp, kv, ka, kf), set j
 * uses row j % M (the seed-batch layout set = e * M + m of avd_clone_sample_f32); model_a != 0 skips the feed-forward term, as the
 * evaluators' law does (csrc/eval_common.h linear_law: the same function, float32, no contraction). The chain is the un-anchored
 * call's with ONE kernel exchanged: in place of the actor's backward seed d mu * high * (1 - tanh(z)^2) runs the anchored seed
 * with d mu' = d mu + (2 weight / N) w (mu - u*), N = P * 64; one small launch more sums
 *   anchor_loss[j] = (1 / N) sum w (mu - u*)^2      (NOT times weight; written for weight == 0 too)
 * in a fixed order (per-wave partials, one wave per set): two calls give the same bits. The critic block of `grads` and both
 * `losses` are the un-anchored call's bit for bit (losses[j][1] stays the mean of q(s, mu)); with weight == 0 so is the actor block.
 * Same workspace as avd_learn_set_split_f16x3 (avd_learn_set_split_workspace). Refused on the host before any HIP call: everything
 * avd_learn_set_split_f16x3 refuses, null gains / anchor_loss, M < 1 or n_sets % M != 0, weight negative or non-finite, lo > hi.
 * There is no two-phase and no per-set-gamma form of this call. */
int avd_learn_set_split_anchor_f16x3(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                                     const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                                     const float* s2, const float* agent_weight, float gamma, float high, float* grads, float* losses,
                                     void* workspace, size_t workspace_bytes, const float* gains, int M, int model_a, float lo, float hi,
                                     float weight, float* anchor_loss, void* stream);

/* Target policy smoothing (TD3's; tr --target_noise), the kernel alone on a caller's buffer: a2 [n_agents][64] float32, 16-byte
 * aligned, the target actions mu'(s2) in the split set learner's agent-major layout, updated IN PLACE:
 *   a2'[v][4q + k] = min(max(a2[v][4q + k] + min(max(sigma * n_k, -noise_clip), noise_clip), lo), hi)      q = 0 .. 15, k = 0 .. 3
 *   w = philox(d_seeds ? d_seeds[e] : seed, counter, vs * 16 + q, stream 12);  (n_0, n_1) = box_muller(w.x, w.y) (cos, sin branch),
 *   (n_2, n_3) = box_muller(w.z, w.w)
 * float32 without contraction. Agent v belongs to weight set v % (E * M): vehicle m = v % M of experiment e = (v / M) % E, platoon
 * p = v / (E * M); vs = p * M + m is its index in the experiment's solo run, so experiment e of a seed batch draws what its solo
 * run draws (E = 1 and d_seeds = NULL without a seed table). noise_clip = +inf: no noise clip. A NaN in a2 stays a NaN (the outer
 * clip is written as two comparisons). One thread per four rows (one 16-byte load and store), no LDS, no atomics: two calls with the
 * same arguments give the same bits. It exists so that the draws can be checked without a learner around them.
 * Refused on the host before any HIP call (AVD_E_INVALID): null or misaligned a2, n_agents < 1 or > 2^24, M or E < 1, n_agents not a
 * multiple of E * M, E > 1 without d_seeds, sigma negative or non-finite, noise_clip NaN or <= 0, lo > hi. */
int avd_target_smooth_f32(int n_agents, int M, int E, float* a2, float sigma, float noise_clip, float lo, float hi, uint64_t seed,
                          uint64_t counter, const uint64_t* d_seeds, void* stream);

/* avd_learn_set_split_anchor_f16x3 with target policy smoothing: the critic is regressed onto
 *   y = r + gamma * Q'(s2, clip(mu'(s2) + clip(sigma n, -noise_clip, noise_clip), lo, hi))
 * The chain is the same with ONE launch more: avd_target_smooth_f32's kernel on the workspace's target actions, between the target
 * actor's head (their writer) and the target critic's (their only reader), with n_agents, M, E, lo, hi, seed, counter and d_seeds as
 * there (counter: the caller's learner-call count). None of the chain's own kernels changes. Only y changes, and through it the critic
 * block of `grads` and losses[j][0]: the actor block and losses[j][1] are the un-smoothed call's bit for bit.
 * gains == NULL selects the un-anchored seed: anchor_loss may then be NULL, model_a and weight are unread, and the call is
 * avd_learn_set_split_f16x3 with the smoothing launch; otherwise the anchored seed and the anchor loss run exactly as in
 * avd_learn_set_split_anchor_f16x3. sigma == 0 skips the launch on the host: the call is then avd_learn_set_split_f16x3's
 * (gains == NULL) or avd_learn_set_split_anchor_f16x3's, bit for bit. A non-finite input stays loud: the heads raise the chain's flag
 * from their own accumulators before the smoothing runs, and the slab and the losses come out all NaN.
 * Refused on the host before any HIP call: everything avd_learn_set_split_f16x3 refuses; with gains, everything
 * avd_learn_set_split_anchor_f16x3 refuses; M or E < 1, n_sets not a multiple of E * M, E > 1 without d_seeds, sigma negative or
 * non-finite, noise_clip NaN or <= 0, lo > hi, a workspace that is not 16-byte aligned.
 * There is no two-phase and no per-set-gamma form of this call. */
int avd_learn_set_split_smooth_f16x3(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                                     const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                                     const float* s2, const float* agent_weight, float gamma, float high, float* grads, float* losses,
                                     void* workspace, size_t workspace_bytes, const float* gains, int M, int model_a, float lo, float hi,
                                     float weight, float* anchor_loss, float sigma, float noise_clip, uint64_t seed, uint64_t counter,
                                     const uint64_t* d_seeds, int E, void* stream);

/* The TD-only learn call of the split set learner, for the calls of a delayed-policy run on which the actor does not move
 * (avd_adam_polyak_delayed_f32 with policy == 0): the critic block of `grads` and the critic loss, and nothing of the actor's half of
 * the chain -- no actor forward, no critic(s, mu), no action gradient, no actor backward pass. The chain: front, prep, the target
 * actor's head, the smoothing launch of avd_learn_set_split_smooth_f16x3 (sigma, noise_clip, lo, hi, seed, counter, d_seeds, E, M as
 * there; sigma == 0: no launch), the target critic's head, the critic head in its loss-only mode (HEAD_BOTH up to and including its
 * branch A), the critic's three backward kernels (dw, dx and dxa: the action layer's parameter sums are the critic's own) and the
 * critic block's finalize.
 *   grads : the critic block of every set is avd_learn_set_split_critic's bit for bit (smoothed: the critic block of
 *           avd_learn_set_split_smooth_f16x3 with the same key and counter); the actor block is all zero;
 *   losses: [n_sets][2], losses[j][0] the critic loss as there; losses[j][1] compares equal to 0 (finalize negates the zero sum: the
 *           sign bit is set, the value is -0.0f).
 * A non-finite input stays loud: an all-NaN critic block. Workspace: avd_learn_set_split_workspace's; it and the slab may hold
 * anything at entry. Refused on the host before any HIP call: everything avd_learn_set_split_critic refuses and everything the
 * smoothing arguments are refused for in avd_learn_set_split_smooth_f16x3. There is no anchored and no per-set-gamma form. */
int avd_learn_set_split_td_f16x3(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                                 const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                                 const float* s2, const float* agent_weight, float gamma, float high, float* grads, float* losses,
                                 void* workspace, size_t workspace_bytes, float sigma, float noise_clip, float lo, float hi, uint64_t seed,
                                 uint64_t counter, const uint64_t* d_seeds, int E, int M, void* stream);

/* Deprecated alias of avd_learn_set_split_f16x3 (same arguments, same results). */
int avd_learn_set_split_bf16x3(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta, const float* stats,
                               const float* theta_t, const float* stats_t, const float* s, const float* a, const float* r,
                               const float* s2, const float* agent_weight, float gamma, float high, float* grads, float* losses,
                               void* workspace, size_t workspace_bytes, void* stream);

/* actor(state) (agent/model.py:26-36, workers/trainer.py:286-289) for agents that share n_sets weight sets, as the same
 * bf16 GEMM chain: state [n_sets][rows][S] SET-MAJOR (rows = n_agents / n_sets, tightly packed S floats per row),
 * out [n_sets][rows] = tanh(.) * high. */
int avd_actor_forward_shared_workspace(const avd_mlp_layout* lay, int n_agents, int n_sets, size_t* bytes);
int avd_actor_forward_shared_bf16(const avd_mlp_layout* lay, int n_agents, int n_sets, const float* theta,
                                  const float* stats, const float* state, float high, float* out, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* ---- evaluator rollout (workers/evaluator.py:40-95, 145; run once per platoon by Trainer.run_simulations,
 *      workers/trainer.py:277-280, 537-550, and by esim, run.py:60-70) --------------------------------------------
 * R noise-free, deterministic-start episodes of T steps in ONE launch (one workgroup per rollout, no communication
 * between workgroups). Rollout r: models m = 0..M-1 use weight set set_base[r] + m (< n_sets); start state
 * x0[start_idx[r]] [L][4], prev_a0[start_idx[r]] [L] and leader inputs leader[start_idx[r]] [T] (start_idx < n_start).
 * Per step: actor forward of each model on its observation (4L / M floats apart, the first S read), action =
 * clip(out, lo, hi), Platoon.step (= avd_env_step_f32), counters[r][m] += reward (M == L) or += the platoon-mean reward
 * (M == 1, centralized). counters [R][M] are written, not accumulated. Bit-identical to the evaluator's per-step launches
 * (avd_actor_forward_f32 -> avd_policy_f32 -> avd_env_step_f32, float32 counters).
 * Traces for the n_trace rollouts trace_idx[j] (or n_trace = 0 and NULLs): tr_states [n_trace][T][L][min(4, S)] post-step
 * observations, tr_actions [n_trace][T][L] clipped actions, tr_jerks [n_trace][T][L] = (x_before[2] - prev_a_before) *
 * (1 / sample_rate) (Vehicle.get_jerk, environment.py:477). A set_base / start_idx out of range makes that rollout's
 * counters NaN and reads nothing. M must be L or 1, lay->A * M == L. */
int avd_eval_rollout_f32(const avd_mlp_layout* lay, const avd_env_consts* d_consts, int R, int L, int M, int T, const float* theta,
                         const float* stats, int n_sets, const int32_t* set_base, const float* x0, const float* prev_a0,
                         const float* leader, int n_start, const int32_t* start_idx, float high, float lo, float hi,
                         float sample_rate, float* counters, int n_trace, const int32_t* trace_idx, float* tr_states,
                         float* tr_actions, float* tr_jerks, void* stream);

/* ---- scenario evaluator: the evaluator rollout above for G groups x K cases in ONE launch, with control metrics reduced on the
 *      device. The reference's evaluator loops over an `input_opts` dict "for a variety of input responses" of which only the
 *      Gaussian one was filled in (workers/evaluator.py:55-70; config.py names zerofig_name / stepfig_name / rampfig_name beside
 *      guasfig_name) ------------------------------------------------------------------------------------------------------------
 * Group g is one platoon's weight sets set_base[g] .. set_base[g] + M - 1 (< n_sets); case k is the start state x0[k] [L][4],
 * prev_a0[k] [L] and the leader-input row leader[k] [T]. Every group runs every case. counters[g][k] [M] is bit-identical to what
 * avd_eval_rollout_f32 writes for a rollout with set_base = set_base[g], start_idx = k. metrics[g][k] [L][AVD_EVAL_NMETRIC] (or
 * NULL), per vehicle, float32, sums as sequential float32 adds in step order without contraction:
 *   0 max_abs_ep, 1 max_abs_ev, 2 max_abs_a  max over steps of |post-step state[0 / 1 / 2]|
 *   3 sum_u2                                 sum of the clipped action squared
 *   4 sum_jerk2                              sum of the jerk squared, jerk = (x_before[2] - prev_a_before) * (1 / sample_rate)
 *   5 term_steps, 6 first_term               steps on which the terminal test (pre-step state, environment.py:505-510) fired and the
 *                                            first of them (-1: none); the evaluator does not stop on it
 *   7 final_abs_ep                           |state[0]| after the last step
 * One workgroup per (group, block of avd_eval_cases_block(K, L) cases): each weight element is read once per block and applied to
 * all of its rows, with the per-row summation order of the rollout kernel. A set_base out of range makes that group's counters
 * and metrics NaN and reads nothing. M must be L or 1, lay->A * M == L. */
#define AVD_EVAL_NMETRIC 8
int avd_eval_cases_f32(const avd_mlp_layout* lay, const avd_env_consts* d_consts, int G, int K, int L, int M, int T,
                       const float* theta, const float* stats, int n_sets, const int32_t* set_base, const float* x0,
                       const float* prev_a0, const float* leader, float high, float lo, float hi, float sample_rate,
                       float* counters, float* metrics, void* stream);

/* The number of cases per workgroup avd_eval_cases_f32 uses for K cases of L vehicles (host only, no HIP call): the value itself
 * (>= 1), or AVD_E_INVALID for K < 1 or L outside 1..AVD_MAX_L. */
int avd_eval_cases_block(int K, int L);

/* ---- disturbed scenario evaluator: avd_eval_cases_f32 with one disturbance per case --------------------------------------------
 * The disturbance acts on what the actors observe and on the plant; counters and metrics come from the true state. Per step t and
 * vehicle v, with the true pre-step state x = (ep, ev, a, w), per-case tables in DEVICE memory:
 *   V2V link (w, the 4th observation): hist[j] = the true w at step j (x0's for j < 0); delayed = hist[t - delay[k]]; the sample is
 *     dropped iff (philox(noise_seed[k], t, v, stream 7).x >> 8) < drop_q[k] (drop_q = round(p * 2^24): 0 never, 2^24 always);
 *     received = dropped ? the last received value (x0's at first) : delayed.
 *   sensor noise: r = philox(noise_seed[k], t, v, stream 6); (n_ep, n_ev) = box_muller(r.x, r.y), n_a = box_muller(r.z, r.w) (cos);
 *     observed = x + sigma[k][c] * n_c without contraction; a zero sigma skips the add.
 *   plant: abc[k] [L][24] = the true plant's A (16, row-major), B (4), C (4) per vehicle; NULL: the constants block's for every case.
 * A case with sigma = 0, delay = 0, drop_q = 0 and the constants block's matrices is bit-identical to avd_eval_cases_f32's. The host
 * cannot read the tables: avd_eval_cases_dist_check validates HOST copies of them (sigma finite and >= 0, delay 0 ..
 * AVD_EVAL_MAX_DELAY, drop_q <= 2^24) before the caller uploads them; the kernel takes a delay modulo the ring and is memory-safe for
 * any value. Blocks of avd_eval_cases_dist_block(K, L) cases (smaller than the nominal kernel's: more LDS per case). */
#define AVD_EVAL_MAX_DELAY 15
int avd_eval_cases_dist_f32(const avd_mlp_layout* lay, const avd_env_consts* d_consts, int G, int K, int L, int M, int T,
                            const float* theta, const float* stats, int n_sets, const int32_t* set_base, const float* x0,
                            const float* prev_a0, const float* leader, float high, float lo, float hi, float sample_rate,
                            const float* sigma, const int32_t* delay, const uint32_t* drop_q, const uint64_t* noise_seed,
                            const float* abc, float* counters, float* metrics, void* stream);
int avd_eval_cases_dist_block(int K, int L);
/* host only, no HIP call: sigma [K][3], delay [K], drop_q [K] in HOST memory */
int avd_eval_cases_dist_check(int K, const float* sigma, const int32_t* delay, const uint32_t* drop_q);

/* ---- linear baseline of the scenario evaluator: the cases above under a static gain row per vehicle instead of an actor ------------
 * G gain sets x K cases in ONE launch. gains[g] [L][4] is gain set g's row (g0, g1, g2, g3) per vehicle; case k is x0[k] [L][4],
 * prev_a0[k] [L], leader[k] [T] and, disturbed, sigma[k] [3], delay[k], drop_q[k], noise_seed[k], abc[k] [L][24] exactly as
 * avd_eval_cases_dist_f32 reads them (DEVICE memory; avd_eval_cases_dist_check validates host copies). All five tables NULL: the
 * constants block's plant and a perfect observation; abc alone may be NULL; any other mix is AVD_E_INVALID. Per step and vehicle,
 * with ob the observed state formed as avd_eval_cases_dist_f32 forms it (same ring, same Philox streams, counter = step, index =
 * vehicle, a zero sigma skips its add):
 *   u = clip(((g0 * ob[0] + g1 * ob[1]) + g2 * ob[2]) + g3 * ob[3], lo, hi)   without contraction; Model A: the first three terms
 * then the platoon step, reward and terminal test of avd_eval_cases_f32 on the true state. counters[g][k] [L]: per vehicle, the
 * sequential float32 sum of the step's -reward (the decentralized convention). metrics[g][k] [L][AVD_EVAL_NMETRIC] (or NULL): the
 * eight metrics of avd_eval_cases_f32, same statements, same order. One lane per (gain set, case, vehicle), floor(64 / L) rollouts
 * per one-wave workgroup; a G x K that needs more than 2^31 - 1 workgroups is AVD_E_UNSUPPORTED. Every argument is checked on the
 * host before any HIP call. */
int avd_eval_linear_f32(const avd_env_consts* d_consts, int G, int K, int L, int T, const float* gains, const float* x0,
                        const float* prev_a0, const float* leader, float lo, float hi, float sample_rate, const float* sigma,
                        const int32_t* delay, const uint32_t* drop_q, const uint64_t* noise_seed, const float* abc, float* counters,
                        float* metrics, void* stream);
/* fitness[g] = (the sequential float32 sum of counters[g] [K][L] in (k, v) order) / (float)(K * L): one thread per gain set,
 * bit-identical to the same loop in NumPy float32. */
int avd_linear_fitness_f32(int G, int K, int L, const float* counters, float* fitness, void* stream);

/* ---- gain search: a cross-entropy search over gain tables around the two launches above (csrc/search.hip) -----------------------
 * A generation is avd_search_sample_f32 -> avd_eval_linear_f32 -> avd_linear_fitness_f32 -> avd_search_refit_f32 on one stream;
 * nothing comes back to the host between generations. R searched rows: R = L (one gain row per vehicle) or R = 1 (tied: every vehicle
 * takes row 0). mean, std, lo, hi, min_std, best_gains are [R][4] in DEVICE memory, dimension d = r * 4 + c. All arithmetic is float32
 * without contraction, in the order written here.
 *
 * avd_search_sample_f32: gains [G][L][4] (out), one thread per (candidate g, vehicle v), r = (R == 1 ? 0 : v):
 *   w = philox(seed, generation, g * R + r, stream 10); (n0, n1) = box_muller(w.x, w.y) (cos, sin), (n2, n3) = box_muller(w.z, w.w);
 *   x = mean[r][c] when g == 0 or std[r][c] == 0 (the add is skipped: exact), else mean[r][c] + std[r][c] * n_c;
 *   gains[g][v][c] = fminf(fmaxf(x, lo[r][c]), hi[r][c]).
 * Candidate 0 of every generation is the current mean. AVD_E_INVALID: a null pointer, G < 1, L outside 1 .. AVD_MAX_L, R not 1 or L.
 *
 * avd_search_refit_f32: two kernels. Rank: candidate i precedes j iff fitness[i] is not NaN and (fitness[j] is NaN or f_i > f_j or
 * (f_i == f_j and i < j)); among NaNs the lower index precedes. A candidate's rank is the number of candidates that precede it (a
 * permutation); elite_idx[rank] = i for rank < n_elite (int32 [n_elite], out: NaN candidates fill the places past the valid ones).
 * Refit, one wave, lane d: E = min(n_elite, the number of non-NaN fitnesses). E == 0: mean, std and best_* stay untouched,
 * history_row = {NaN, NaN, best_fitness, 0}. Otherwise, with x_k = gains[elite_idx[k]][r][c], k = 0 .. E - 1 in rank order:
 *   s = 0; for k: s = s + x_k;               m  = s / (float)E
 *   q = 0; for k: t = x_k - m; q = q + t * t;  sd = sqrtf(q / (float)E)
 *   if (std[d] != 0) { mean[d] = mean[d] + alpha * (m - mean[d]); std[d] = fmaxf(std[d] + alpha * (sd - std[d]), min_std[d]); }
 * (a frozen dimension, std == 0, never moves). Best-ever record: if best_gen[0] < 0 (none yet) or fitness[elite_idx[0]] >
 * best_fitness[0] (strict: the first generation that reaches a value keeps it), best_gains = that candidate's R rows, best_fitness
 * its fitness, best_gen = generation. history_row [4] (out) = {fitness[elite_idx[0]], (the sequential sum of the E elite fitnesses
 * in rank order) / (float)E, best_fitness after the update, (float)E}. Plain stores by the lanes that own the values; no atomics.
 * AVD_E_INVALID: a null pointer, G outside 1 .. 65536 (every pair of candidates is compared), L, R as above, n_elite outside 1 .. G,
 * alpha outside (0, 1], generation < 0. */
int avd_search_sample_f32(int G, int L, int R, const float* mean, const float* std, const float* lo, const float* hi, uint64_t seed,
                          uint64_t generation, float* gains, void* stream);
int avd_search_refit_f32(int G, int L, int R, int n_elite, float alpha, const float* gains, const float* fitness, const float* min_std,
                         float* mean, float* std, float* best_gains, float* best_fitness, int32_t* best_gen, int generation,
                         int32_t* elite_idx, float* history_row, void* stream);

/* ---- training under disturbances: the fused step with an observation model (domain randomisation) --------------------------------
 * The evaluator's observation model (above) at training time. A run has n_levels (1 .. AVD_TRAIN_MAX_LEVELS) disturbance levels;
 * platoon p trains under level p % n_levels (an experiment batch: the level of the solo run's platoon index, (g / n_groups) %
 * n_levels), fixed for the run. The TRUE state x advances as in avd_step_fused_f32, with the level's plant d_plant[level][L][24] (A
 * 16 row-major, B 4, C 4 per vehicle) in place of the constants block's matrices; reward, terminal flags, done, any_done, ep_reward,
 * prev_a and cum_accel come from the true state. The actors and the replay see the OBSERVATION o (a float4 per vehicle, laid out
 * like x) of a true state x, made with observation counter c and vehicle index v (of the solo run):
 *   sensor noise: r = philox(seed, c, v, stream 8); (n_ep, n_ev) = box_muller(r.x, r.y), n_a = box_muller(r.z, r.w) (cos);
 *     o[k] = x[k] + sigma[k] * n_k for k < 3, multiply and add unfused; a zero sigma keeps x[k]'s bits.
 *   V2V link (k = 3), a 16-slot ring link_hist[v] and a held value link_recv[v] per vehicle: hist[c & 15] = x.w; delayed =
 *     hist[(c - delay) & 15]; the sample is dropped iff drop_q != 0 and (philox(seed, c, v, stream 9).x >> 8) < drop_q; if it is not,
 *     recv = delayed; o.w = recv. Only levels with delay != 0 or drop_q != 0 touch the link state; link_hist and link_recv may both be
 *     NULL when no level does (o.w = x.w then).
 * avd_step_fused_dist_f32 observes the state it produces: obs_out = o(x_out) with obs_counter (the host passes step t's as t + 1).
 * The replay row is [obs_in[:S], action, -reward, obs_out[:S]]: what the agent saw. actor_out is expected to come from obs_in.
 * h_levels is the level table in HOST memory, checked on every call (sigma finite and >= 0, delay 0 .. 15, drop_q <= 2^24);
 * d_levels is the same table in device memory, which the kernel reads. With every level null and the configuration's plant, every
 * output avd_step_fused_f32 has is bit-identical to it and obs_out has x_out's bits. */
#define AVD_TRAIN_MAX_LEVELS 16
typedef struct avd_train_level {
    float sigma[3];       /* sensor-noise standard deviations of ep, ev, a */
    int32_t delay;        /* V2V delay in steps, 0 .. 15 */
    uint32_t drop_q;      /* V2V loss threshold, round(p * 2^24) */
    uint32_t reserved[3]; /* 32 bytes per level */
} avd_train_level;
int avd_step_fused_dist_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out, float* prev_a,
                            float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done, int32_t* any_done_other,
                            const float* actor_out, float* ou_state, float* action, float* leader_exog, float ou_theta, float ou_mean,
                            float ou_dt, float ou_std_dev, float action_low, float action_high, float exog_scale, int exog_uniform,
                            uint64_t seed, uint64_t ou_counter, uint64_t exog_counter, float* ring, int cap, int64_t replay_counter,
                            float* ep_reward, int n_levels, const avd_train_level* h_levels, const avd_train_level* d_levels,
                            const float* d_plant, const float* obs_in, float* obs_out, float* link_hist, float* link_recv,
                            uint64_t obs_counter, void* stream);
/* avd_step_fused_dist_f32 with a seed table (as avd_step_fused_seeds_f32). */
int avd_step_fused_dist_seeds_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out, float* prev_a,
                                  float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done,
                                  int32_t* any_done_other, const float* actor_out, float* ou_state, float* action, float* leader_exog,
                                  float ou_theta, float ou_mean, float ou_dt, float ou_std_dev, float action_low, float action_high,
                                  float exog_scale, int exog_uniform, const uint64_t* d_seeds, int n_groups, uint64_t ou_counter,
                                  uint64_t exog_counter, float* ring, int cap, int64_t replay_counter, float* ep_reward, int n_levels,
                                  const avd_train_level* h_levels, const avd_train_level* d_levels, const float* d_plant,
                                  const float* obs_in, float* obs_out, float* link_hist, float* link_recv, uint64_t obs_counter,
                                  void* stream);
/* (Re)observe FRESH states: obs = o(x) with the sensor noise of (seed, obs_counter, vehicle) and a fresh link -- the vehicle's ring
 * filled with its x.w, link_recv = x.w, o.w = x.w (a fresh link holds the start value, as in the evaluator). The host passes the
 * counter of the observation this one replaces. Two gates, both may be NULL (every platoon is observed then):
 *   only_where_zero [P]: platoon p is observed only where only_where_zero[p] == 0 (avd_episode_end_f32 leaves ep_len[p] == 0 exactly
 *     on the platoons it reset);
 *   run_if_nonzero: one device flag; the launch does nothing when it reads 0 (the any-terminal reset's env.any_done).
 * One thread per vehicle. d_levels in device memory (validated where the step's host copy is); link_hist / link_recv NULL: no link. */
int avd_observe_f32(int P, int L, const float* x, float* obs, int n_levels, const avd_train_level* d_levels, float* link_hist,
                    float* link_recv, uint64_t seed, uint64_t obs_counter, const int32_t* only_where_zero,
                    const int32_t* run_if_nonzero, void* stream);
int avd_observe_seeds_f32(int P, int L, const float* x, float* obs, int n_levels, const avd_train_level* d_levels, float* link_hist,
                          float* link_recv, const uint64_t* d_seeds, int n_groups, uint64_t obs_counter,
                          const int32_t* only_where_zero, const int32_t* run_if_nonzero, void* stream);

/* ---- training under leader manoeuvres: the fused step with the leader's input from a manoeuvre table -------------------------------
 * A run has n_manoeuvres (1 .. AVD_TRAIN_MAX_MANOEUVRES) training manoeuvres; platoon p trains under manoeuvre (q / n_levels) %
 * n_manoeuvres for the whole run, q its solo-run platoon index (an experiment batch: g / n_groups) and n_levels the disturbance level
 * count (1 without levels): levels and manoeuvres cross. Only the leader's exogenous input changes; leader_exog[p] receives the value
 * used, every other output and every Philox draw is avd_step_fused_f32's (avd_step_fused_dist_f32's). With d the unit draw the nominal
 * step makes for this platoon and step (same key, exog_counter, index, stream; uniform or normal by exog_uniform):
 *   d_gaussian[m] != 0: the input is d * d_noise[m] -- with d_noise[m] = exog_scale, bit for bit the nominal launch;
 *   otherwise: d_table[m][k], plus d_noise[m] * d (product rounded, then one add) when d_noise[m] != 0; k = ep_len[p], the step of the
 *     platoon's own episode as avd_episode_end_f32 maintains it, or ep_step for every platoon when ep_len is NULL; k is clamped to
 *     0 .. T - 1.
 * d_table [n_manoeuvres][T] float32, d_noise [n_manoeuvres] float32 and d_gaussian [n_manoeuvres] bytes are device memory, made on
 * the host (no transcendental is evaluated on the device); exog_scale is unread. Refused on the host: null tables, n_manoeuvres
 * outside 1 .. 16, T < 4, a null ep_len with ep_step outside [0, T), n_levels < 1. */
#define AVD_TRAIN_MAX_MANOEUVRES 16
int avd_step_fused_lead_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out, float* prev_a,
    float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done, int32_t* any_done_other, const float*
    actor_out, float* ou_state, float* action, float* leader_exog, float ou_theta, float ou_mean, float ou_dt, float ou_std_dev,
    float action_low, float action_high, float exog_scale, int exog_uniform, uint64_t seed, uint64_t ou_counter, uint64_t
    exog_counter, float* ring, int cap, int64_t replay_counter, float* ep_reward, int n_manoeuvres, int T, const float* d_table,
    const float* d_noise, const uint8_t* d_gaussian, const int32_t* ep_len, int ep_step, int n_levels, void* stream);
int avd_step_fused_lead_seeds_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out, float*
    prev_a, float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done, int32_t* any_done_other, const float*
    actor_out, float* ou_state, float* action, float* leader_exog, float ou_theta, float ou_mean, float ou_dt, float ou_std_dev,
    float action_low, float action_high, float exog_scale, int exog_uniform, const uint64_t* d_seeds, int n_groups, uint64_t
    ou_counter, uint64_t exog_counter, float* ring, int cap, int64_t replay_counter, float* ep_reward, int n_manoeuvres, int T,
    const float* d_table, const float* d_noise, const uint8_t* d_gaussian, const int32_t* ep_len, int ep_step, int n_levels, void*
    stream);
int avd_step_fused_dist_lead_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out, float*
    prev_a, float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done, int32_t* any_done_other, const float*
    actor_out, float* ou_state, float* action, float* leader_exog, float ou_theta, float ou_mean, float ou_dt, float ou_std_dev,
    float action_low, float action_high, float exog_scale, int exog_uniform, uint64_t seed, uint64_t ou_counter, uint64_t
    exog_counter, float* ring, int cap, int64_t replay_counter, float* ep_reward, int n_levels, const avd_train_level* h_levels,
    const avd_train_level* d_levels, const float* d_plant, const float* obs_in, float* obs_out, float* link_hist, float* link_recv,
    uint64_t obs_counter, int n_manoeuvres, int T, const float* d_table, const float* d_noise, const uint8_t* d_gaussian, const
    int32_t* ep_len, int ep_step, void* stream);
int avd_step_fused_dist_lead_seeds_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out, float*
    prev_a, float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done, int32_t* any_done_other, const float*
    actor_out, float* ou_state, float* action, float* leader_exog, float ou_theta, float ou_mean, float ou_dt, float ou_std_dev,
    float action_low, float action_high, float exog_scale, int exog_uniform, const uint64_t* d_seeds, int n_groups, uint64_t
    ou_counter, uint64_t exog_counter, float* ring, int cap, int64_t replay_counter, float* ep_reward, int n_levels, const
    avd_train_level* h_levels, const avd_train_level* d_levels, const float* d_plant, const float* obs_in, float* obs_out, float*
    link_hist, float* link_recv, uint64_t obs_counter, int n_manoeuvres, int T, const float* d_table, const float* d_noise, const
    uint8_t* d_gaussian, const int32_t* ep_len, int ep_step, void* stream);

/* ---- a residual policy on a static linear law: the fused step and the evaluators with the law in front of the plant ------------------
 * The agent's action r is a correction to a per-vehicle linear law. With ob what the agent observes of the pre-step state, (kp, kv,
 * ka, kf) = d_gains[vehicle] (DEVICE memory, [L][4] float32, 16-byte aligned; its values are the caller's to check) and scale in (0, 1]
 * the residual's authority, the plant receives, in float32 without contraction and in this order,
 *   z = (kp*ob.x + kv*ob.y) + ka*ob.z;   z = z + kf*ob.w (Model B only);   u = fminf(fmaxf(z + scale*r, action_low), action_high)
 * -- avd_eval_linear_f32's law plus scale * r. u drives the plant, the reward's norm_u term and the value chained to the follower; the
 * learners keep seeing r. Zero gains and scale = 1 give u = clip(r): every output is then the twin entry point's.
 *
 * avd_step_fused_res_f32: ONE entry point for avd_step_fused_f32 and its seed-batch, disturbed and manoeuvre twins. d_seeds NULL: the
 * scalar seed keys the draws (n_groups unread); otherwise the table of n_groups seeds does, as in the *_seeds_* twins (seed unread).
 * n_levels = 0: no disturbance levels (the level arguments unread, ob = x_in); otherwise avd_step_fused_dist_f32's arguments, and ob =
 * obs_in, the observation the replay row stores. n_manoeuvres = 0: the nominal leader input; otherwise avd_step_fused_lead_f32's
 * arguments (the level count the assignment divides by is n_levels, 1 without levels). r = clip(actor_out + OU noise), as in every
 * twin: action[] and the replay row [s, r, reward, s'] hold r; applied [P*L] (or NULL) receives u. Refused on the host, before any
 * launch: what the twins refuse, null or misaligned d_gains, a misaligned obs_in, scale outside (0, 1], negative counts.
 *
 * avd_eval_rollout_res_f32 / avd_eval_cases_res_f32: avd_eval_rollout_f32 / avd_eval_cases_dist_f32 with r = clip(tanh(.) * high) and
 * ob the vehicle's state (disturbed cases: its observation); the action trace, the reward and sum_u2 take u. The cases form serves both
 * kinds of run: all five disturbance tables NULL is the nominal evaluator (avd_eval_cases_f32's block sizes), otherwise only abc may be
 * NULL (avd_eval_cases_dist_f32's). Actors whose output is zero give avd_eval_linear_f32's counters and metrics for the same gains.
 * Decentralized agents only: M != L is AVD_E_UNSUPPORTED. */
int avd_step_fused_res_f32(const avd_env_consts* d_consts, int P, int L, int S, const float* x_in, float* x_out, float* prev_a,
    float* cum_accel, float* reward, uint8_t* term, uint8_t* done, int32_t* any_done, int32_t* any_done_other, const float*
    actor_out, float* ou_state, float* action, float* leader_exog, float ou_theta, float ou_mean, float ou_dt, float ou_std_dev,
    float action_low, float action_high, float exog_scale, int exog_uniform, uint64_t seed, uint64_t ou_counter, uint64_t
    exog_counter, float* ring, int cap, int64_t replay_counter, float* ep_reward, const uint64_t* d_seeds, int n_groups, int n_levels,
    const avd_train_level* h_levels, const avd_train_level* d_levels, const float* d_plant, const float* obs_in, float* obs_out,
    float* link_hist, float* link_recv, uint64_t obs_counter, int n_manoeuvres, int T, const float* d_table, const float* d_noise,
    const uint8_t* d_gaussian, const int32_t* ep_len, int ep_step, const float* d_gains, float scale, float* applied, void* stream);
int avd_eval_rollout_res_f32(const avd_mlp_layout* lay, const avd_env_consts* d_consts, int R, int L, int M, int T, const float* theta,
                             const float* stats, int n_sets, const int32_t* set_base, const float* x0, const float* prev_a0,
                             const float* leader, int n_start, const int32_t* start_idx, float high, float lo, float hi,
                             float sample_rate, float* counters, int n_trace, const int32_t* trace_idx, float* tr_states,
                             float* tr_actions, float* tr_jerks, const float* d_gains, float scale, void* stream);
int avd_eval_cases_res_f32(const avd_mlp_layout* lay, const avd_env_consts* d_consts, int G, int K, int L, int M, int T,
                           const float* theta, const float* stats, int n_sets, const int32_t* set_base, const float* x0,
                           const float* prev_a0, const float* leader, float high, float lo, float hi, float sample_rate,
                           const float* sigma, const int32_t* delay, const uint32_t* drop_q, const uint64_t* noise_seed,
                           const float* abc, const float* d_gains, float scale, float* counters, float* metrics, void* stream);

/* ---- frequency response: the scenario evaluators with a single-bin Fourier sum per vehicle and signal -------------------------------
 * A frequency sweep is a set of cases: case k's leader row is a sinusoid and basis[k] [T][2] (DEVICE memory, 8-byte aligned) holds,
 * per step, the pair (c, s) = (cos, sin) of the case's angle inside the measuring window and (0, 0) before it. At step t of case k,
 * for the four components of the post-step true state and for the step's plant input u, in float32 without contraction,
 *   re = re + x * c;   im = im + x * s        (sequential adds in step order, the product rounded first)
 * and spectrum[g][k] [L][AVD_EVAL_NSPEC] receives the raw sums (re, im) of ep, ev, a, w, u in that order; the host scales them
 * (scenarios.frequency_summary). Counters and metrics are the twin entry point's, bit for bit.
 * avd_eval_cases_freq_f32: avd_eval_cases_res_f32's arguments; all five disturbance tables NULL is the nominal plant
 * (avd_eval_cases_f32's block sizes), d_gains NULL means no residual law (scale unread, M = 1 allowed). A set_base out of range makes
 * the group's spectrum NaN as well. avd_eval_linear_freq_f32: avd_eval_linear_f32's arguments. Both refuse, on the host and before any
 * HIP call, what their twins refuse, a NULL basis or spectrum and a basis that is not 8-byte aligned. */
#define AVD_EVAL_NSPEC 10
int avd_eval_cases_freq_f32(const avd_mlp_layout* lay, const avd_env_consts* d_consts, int G, int K, int L, int M, int T,
                            const float* theta, const float* stats, int n_sets, const int32_t* set_base, const float* x0,
                            const float* prev_a0, const float* leader, float high, float lo, float hi, float sample_rate,
                            const float* sigma, const int32_t* delay, const uint32_t* drop_q, const uint64_t* noise_seed,
                            const float* abc, const float* d_gains, float scale, float* counters, float* metrics, const float* basis,
                            float* spectrum, void* stream);
int avd_eval_linear_freq_f32(const avd_env_consts* d_consts, int G, int K, int L, int T, const float* gains, const float* x0,
                             const float* prev_a0, const float* leader, float lo, float hi, float sample_rate, const float* sigma,
                             const int32_t* delay, const uint32_t* drop_q, const uint64_t* noise_seed, const float* abc,
                             float* counters, float* metrics, const float* basis, float* spectrum, void* stream);

/* D[M][Nc] (f32, ldd) = A[M][K] . B[Nc][K]^T with bf16 operands (K contiguous, K % 64 == 0) and f32 accumulation: the
 * GEMM under avd_learn_shared_bf16, exposed for parity tests. A and B must be readable up to the next multiple of 256
 * rows. */
int avd_gemm_bt_bf16(int M, int Nc, int K, const void* A, long lda, const void* B, long ldb, float* D, long ldd,
                     void* stream);

#ifdef __cplusplus
#pragma GCC visibility pop
}
#endif
#endif /* AVDDPG_HIP_H */
