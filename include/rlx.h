/*
 * rlx.h — C ABI of librlx.so, the MI355X (gfx950) hot-path library behind the
 * rl_coach-compatible Python adapters in coach_amd/.
 *
 * The reference (IntelLabs/coach, rl_coach 1.0.1) has NO C interface: its plug
 * points are Python classes.  Every entry point below therefore
 * cites the reference *Python* routine whose arithmetic it replaces (file:line under
 * /root/reference/rl_coach/), and INTEGRATION.md shows the ctypes stub a reference
 * maintainer would add to call it.
 *
 * Conventions
 *   - All pointers are DEVICE pointers unless the parameter name ends in _host.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - Every function returns RLX_OK (0) or a negative rlx_status; the human readable
 *     reason is available from rlx_last_error() (thread local).  The exceptions return a
 *     VALUE, and their names say so: rlx_abi_version and every rlx_*_supported (1 / 0)
 *     return an int that is no status; the `const char *` functions return a string.
 *     A binding tells the two apart by that naming rule alone.
 *   - No function allocates device memory or synchronises the device unless its
 *     name says so (rlx_*_sync / rlx_event_elapsed_ms): all are hipGraph-capturable.
 *   - Layouts are row-major, innermost dimension last (NHWC for images).
 *   - This header is also READ BY THE BINDING (coach_amd/_rlx.py builds its prototypes, ctypes
 *     structures and constants from it), so it keeps to a small grammar.  A structure is
 *     `typedef struct rlx_NAME { ... } rlx_NAME;` whose members are scalars (int, unsigned,
 *     unsigned char, float, double, long long, size_t, uint32_t, [u]int64_t), pointers to those, to
 *     void or to a (`struct`) rlx_* structure, or earlier rlx_* structures by value; several
 *     declarators per statement and several statements per line are fine.  No arrays,
 *     bit-fields, unions, function pointers or anonymous members.  A constant the binding needs
 *     is `#define RLX_NAME <integer>` or an enumerator with an explicit integer value.
 */
#ifndef RLX_H
#define RLX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rlx_status {
    RLX_OK = 0,
    RLX_ERR_INVALID_ARG = -1, /* bad size / null pointer / unsupported combination */
    RLX_ERR_HIP = -2,         /* a HIP runtime call or a kernel launch failed       */
    RLX_ERR_UNSUPPORTED = -3
} rlx_status;

/* ------------------------------------------------------------------ runtime -- */
/* What rlx_abi_version() returns; the binding refuses a library built from another value.  It bumps when a signature or
 * a structure changes (an added entry point does not count: the loader already refuses a library that lacks a declared
 * symbol).  11: rlx_normal_fill; 10: rlx_gemm_desc.kw_min_tiles, rlx_dqn_head_loss_backward;
 * 9: rlx_conv32_input_grad_per_update / rlx_splitk_reduce_jobs_per_update (rlx_per_update_desc),
 * rlx_imgreplay_gather_columns, conv_dw_u8 for one tower of 32 filters (2 B splits); 8: rlx_ppo_fc_rows /
 * rlx_ppo_heads_tail / rlx_splitk_reduce_jobs_ppo_tail, fused TD3 / SAC updates, rlx_conv_dw_*; 7: rlx_conv123_forward,
 * rlx_gemm_describe; 6: rlx_conv23_forward, rlx_gemm_multi_defer, rlx_gemm_big_tiles; 5: rlx_adam_tf1_step ticket =
 * RLX_ADAM_TICKET_WORDS words; 4: per_sample payload rows, libm pow; 3: gemm desc batch_inner, n_fold;
 * 2: adam_tf1_norm / sac head accumulate. */
#define RLX_ABI_VERSION 11
int rlx_abi_version(void);               /* RLX_ABI_VERSION of the header the library was built from */
const char *rlx_last_error(void);        /* message of the last failure (this thread) */
const char *rlx_build_arch(void);        /* "gfx950"                                  */
int rlx_device_count(int *count_host);   /* replaces coach.py:61-84 (cuDeviceGetCount) */
int rlx_stream_sync(void *stream);
int rlx_event_create(void **event_host);
int rlx_event_destroy(void *event);
int rlx_event_record(void *event, void *stream);
int rlx_event_elapsed_ms(void *start, void *stop, float *ms_host); /* syncs on stop */

/* Latency probe for bench.py's `box` block (no reference counterpart): one lane follows `steps` dependent 4-byte loads
 * i = chain[i] from `start` and stores the last index in *out; time it with events. */
int rlx_probe_chase(const int *chain, int start, int steps, int *out, void *stream);
/* Matrix-pipe clock probe (measurement utility): `workgroups` x 4 waves each run `iters` dependent
 * v_mfma_f32_32x32x2_f32; out[2 w] = shader-clock cycles and out[2 w + 1] = ticks of the constant 100 MHz counter that
 * workgroup w's chain took: cycles per MFMA, and the clock the shader really ran at under that load. */
int rlx_probe_mfma(int workgroups, int iters, long long *out, float *sink, void *stream);
/* The same for either fp32 MFMA shape (small_shape != 0: v_mfma_f32_16x16x4_f32) with `chains` (1, 2 or 4) independent
 * accumulators per wave issued round-robin, `iters` MFMAs per chain: chains = 1 is the dependent-accumulator latency,
 * chains >= 2 the issue rate of the matrix pipe. */
int rlx_probe_mfma_shape(int workgroups, int iters, int small_shape, int chains, long long *out, float *sink, void *stream);
/* Request-pipelining probe (measurement utility): every wave of `workgroups` workgroups issues `requests` (1, 2, 4 or 8)
 * back-to-back 16-byte-per-lane loads from src — global -> LDS requests (lds_dma != 0: what the GEMM ring issues) or
 * ordinary loads into registers — and waits for all of them; out[w] = shader-clock cycles of workgroup w.  src: at least
 * 8 MB + 4 KB * workgroups + 256 * round bytes. */
int rlx_probe_requests(int workgroups, int requests, int lds_dma, int round, const float *src, long long *out, float *sink,
                       void *stream);

/* In-process kernel timer: between rlx_profile_begin and rlx_profile_end every kernel this library launches (EAGER
 * launches on any stream; do not arm it inside a stream capture) carries its own start / stop event pair filled from
 * the dispatch's begin / end timestamps — the per-dispatch duration a kernel trace reports (the reference has no
 * counterpart: its TF timeline is the closest thing, architectures/tensorflow_components/architecture.py has none on
 * this path).  rlx_profile_read(i) returns the kernel's name (a static string: the template instance as written at
 * the launch site) and its duration in ms, in launch order; it waits for that kernel.  max_records bounds the trace:
 * launches beyond it go out untimed and rlx_profile_end then FAILS (the records taken stay readable). */
int rlx_profile_begin(int max_records);
int rlx_profile_end(int *n_records_host);
int rlx_profile_read(int index, const char **name_host, float *ms_host);

/* The second and third convolution of the Atari torso (embedder "Medium": 64 x 4 x 4 / 2 on 20 x 20 x 32, then 64 x 3 x 3 / 1)
 * as ONE launch: half an image of one tower per workgroup, the second layer's output stays in LDS and feeds the third
 * (tf.layers.conv2d twice, architectures/tensorflow_components/layers.py:108-121).  y2 / y3 receive both layers'
 * activations (the backward pass reads them).  wave_groups = 2 / 4: bit-identical to the two rlx_gemm launches it replaces
 * where those run on 32 x 64 tiles with two wave groups per K slab / on 32 x 32 tiles with four (coach_amd/csrc/conv_fused.hip).  rlx_conv23_forward_supported: 1 for
 * the geometry the kernel is compiled for. */
int rlx_conv23_forward_supported(int H, int W, int C, int k2, int s2, int c2, int k3, int s3, int c3);
/* weight slabs in rlx_conv23_forward's LDS ring (2, 3, 4, 6, 8) and slabs per synchronisation step (1, or 2 with depth
 * >= 4): process-wide, for same-process A/Bs */
int rlx_conv23_depth(int depth, int slabs_per_step);
/* diagnostics: while buffer != NULL every workgroup of rlx_conv23_forward records 10 ns ticks at [8 w + 0 .. 5]: entry,
 * conv2's first slab and the conv1 rows staged, conv2's slab loop done, conv3's first slab staged (conv2's epilogue done),
 * conv3's slab loop done, exit.  buffer: 16 * batch * towers 64-bit words. */
int rlx_conv23_debug_stamps(void *buffer);
int rlx_conv23_forward(const float *x1, long long x1_tower_stride, const float *w2, long long w2_tower_stride,
                       const float *b2, long long b2_tower_stride, const float *w3, long long w3_tower_stride,
                       const float *b3, long long b3_tower_stride, float *y2, long long y2_tower_stride, float *y3,
                       long long y3_tower_stride, int batch, int towers, int activation, int wave_groups, void *stream);
/* ... and the FIRST convolution (32 x 8 x 8 / 4 on 84 x 84 x 4 uint8 frames, rescaled by 1 / a_div:
 * architectures/embedder_parameters.py + observation rescaling filter) in front of them in the same launch: the frame rows
 * of a half image go to LDS as bytes, conv1's output feeds conv2 from LDS and is also written to y1 (the backward pass reads
 * it).  x0: [towers or 1][batch][84][84][4] (x0_tower_stride in BYTES, 0 = every tower reads the same frames).
 * conv1_chunks = 1 / 3: bit-identical to rlx_gemm's conv1 launch where that sums K = 256 in one chain (64 x 64 tiles) / in
 * three chains over 96-long K chunks combined by its split-K reduce launch (128 x 32 tiles, 200 of them) — with operands
 * staged by registers (rlx_gemm_describe reports all of that; coach_amd/nn/graph.py asks it before taking this launch). */
int rlx_conv123_forward_supported(int H, int W, int C, int k1, int s1, int c1);
int rlx_conv123_forward(const unsigned char *x0, long long x0_tower_stride, float a_div, const float *w1,
                        long long w1_tower_stride, const float *b1, long long b1_tower_stride, float *y1,
                        long long y1_tower_stride, const float *w2, long long w2_tower_stride, const float *b2,
                        long long b2_tower_stride, const float *w3, long long w3_tower_stride, const float *b3,
                        long long b3_tower_stride, float *y2, long long y2_tower_stride, float *y3,
                        long long y3_tower_stride, int batch, int towers, int activation, int wave_groups,
                        int conv1_chunks, void *stream);

/* The INPUT-GRADIENT chain of the same two layers in the backward pass as one launch (tf.gradients through the two
 * tf.layers.conv2d, layers.py:108-121; architecture.py:312-385 accumulate_gradients): per half image of a tower
 * dcol3 = dz3 W3^T -> dz2 = col2im(dcol3) * act'(y2) -> dcol2 = dz2 W2^T -> dz1 = col2im(dcol2) * act'(y1), both column
 * matrices in LDS (coach_amd/csrc/conv_bwd_fused.hip).  dz3: gradient at conv3's pre-activation [towers][batch * 49][64];
 * y2 / y1: the stored activations of conv2 / conv1; dz2 / dz1 (out): gradients at their pre-activations (what the layers'
 * weight-gradient products read).  Bit-identical to rlx_gemm (dcol) + rlx_col2im per layer where rlx_gemm_describe
 * reports the LDS-DMA ring without a K split for the dcol products. */
int rlx_conv32_input_grad_supported(int H, int W, int C, int k2, int s2, int c2, int k3, int s3, int c3);
int rlx_conv32_input_grad(const float *dz3, long long dz3_tower_stride, const float *w3, long long w3_tower_stride,
                          const float *y2, long long y2_tower_stride, float *dz2, long long dz2_tower_stride,
                          const float *w2, long long w2_tower_stride, const float *y1, long long y1_tower_stride,
                          float *dz1, long long dz1_tower_stride, int batch, int towers, int activation, void *stream);
/* The same launch with PrioritizedExperienceReplay.update_priorities (prioritized_experience_replay.py:203-217; called right
 * behind learn_from_batch, agents/dqn_agent.py:106-109) of the batch's n <= 64 sampled leaves as ONE MORE workgroup: the
 * arguments of rlx_per_update as a structure.  The DQN update (batch 32, one tower) fills 64 of 256 CUs with this launch; the
 * priority update — a 10 us chain of dependent round trips, so far a launch of its own behind every update — runs beside it.
 * Its inputs (the TD errors) exist since the head's loss and nothing reads the trees before the next sample(): trees
 * bit-identical to rlx_per_update's (same device code: coach_amd/csrc/per_update_body.hpp). */
typedef struct rlx_per_update_desc {
    double *sum_tree, *min_tree, *max_tree;
    int capacity;
    const int *idx;
    const double *td_errors;
    int n;
    double alpha, epsilon;
    double *max_priority;
    int *status;
} rlx_per_update_desc;
int rlx_conv32_input_grad_per_update(const float *dz3, long long dz3_tower_stride, const float *w3, long long w3_tower_stride,
                                     const float *y2, long long y2_tower_stride, float *dz2, long long dz2_tower_stride,
                                     const float *w2, long long w2_tower_stride, const float *y1, long long y1_tower_stride,
                                     float *dz1, long long dz1_tower_stride, int batch, int towers, int activation,
                                     const rlx_per_update_desc *per, void *stream);
/* diagnostics as rlx_conv23_debug_stamps: [8 w + 0 .. 5] = entry, first product's operands staged, its K loop done,
 * second product's operands staged (= first gather done), its K loop done, exit */
int rlx_conv32_debug_stamps(void *buffer);
/* Process-wide (default 1): 1 = the second row tile of both products (3 of 35, 13 of 45 positions) runs as a 16-row tile
 * on v_mfma_f32_16x16x4_f32 with two accumulator chains per wave — half the MFMA cycles of the padded 32-row tile; rows
 * >= 32 of a column matrix then sum k in another order (last bits: -3 us per Clipped-PPO update, profiles/r06_conv32_tail16.txt); 0 = 32-row tiles throughout, bit-identical to
 * rlx_gemm + rlx_col2im. */
int rlx_conv32_tail_tiles(int sixteen_rows);
/* how many jobs ahead a wave of that launch requests its weight operands: 1 (default) or 2 (one more register set; results
 * unchanged) */
int rlx_conv32_prefetch(int jobs_ahead);

/* --------------------------------------------- prioritized replay (K5 / K6) -- */
/* Trees are fp64 array-heaps of 2*capacity-1 nodes exactly as the reference's
 * SegmentTree (memories/non_episodic/prioritized_experience_replay.py:43-156);
 * capacity must be a power of two (:176-179).  max_priority is one device double
 * mirroring PrioritizedExperienceReplay.maximal_priority (:186,:201).  `status` is a
 * device int the kernels OR error bits into (1 = leaf index out of range -> the
 * reference's ValueError at :123-126; 2 = negative error -> ValueError at :195;
 * 4 = a priority outside the domain of the bit-exact pow, see rlx_libm_pow).
 * Every `p ** alpha` / `(N*P) ** -beta` below is evaluated with rlx::libm_pow
 * (csrc/libm_pow.hpp): glibc's pow algorithm on glibc's tables, so leaves and importance
 * weights are bit-identical to the reference's CPython `**` (= libm pow) — no host round trip. */
int rlx_per_init(double *sum_tree, double *min_tree, double *max_tree, int capacity,
                 double *max_priority, void *stream);               /* SegmentTree.__init__ :59-67 */
int rlx_per_store(double *sum_tree, double *min_tree, double *max_tree, int capacity,
                  int start_leaf, int n, double alpha, double *max_priority, int *status,
                  void *stream);                                     /* .store :264-283 (n consecutive adds) */
int rlx_per_store_value(double *sum_tree, double *min_tree, double *max_tree, int capacity,
                        int start_leaf, int n, double leaf_pa, double leaf_p,
                        double *max_priority, int *status,
                        void *stream);                               /* same, host-computed (p**alpha, p) */
int rlx_per_update(double *sum_tree, double *min_tree, double *max_tree, int capacity,
                   const int *idx, const double *errors, int n, double alpha, double epsilon,
                   double *max_priority, int *status, void *stream); /* .update_priorities :203-217 */
/* Updates of at most path_max_leaves leaves (default and maximum 256; 0 = never) run on the kernel whose threads meet
 * only in LDS instead of the level-synchronous one.  Both write bit-identical trees; the knob exists for same-process
 * A/B timing (tools/ab_per_update.py). */
int rlx_per_tuning(int path_max_leaves);
int rlx_per_update_leaves(double *sum_tree, double *min_tree, double *max_tree, int capacity,
                          const int *idx, const double *leaf_pa, const double *leaf_p, int n,
                          double *max_priority, int *status, void *stream); /* same, host-computed p**alpha */
int rlx_per_sample(const double *sum_tree, const double *min_tree, int capacity,
                   const double *uniforms, int batch, double num_transitions, double beta,
                   int *out_idx, double *out_weight, double *out_priority, long long stored_total,
                   long long payload_rows, int *out_rows,
                   void *stream);                                    /* .sample :229-255; uniforms[i] = random.random();
                                                                        out_rows (optional): payload-ring row of every sampled
                                                                        leaf when the ring holds payload_rows >= capacity rows
                                                                        and stored_total transitions were stored so far */
int rlx_per_sample_top_steps(int steps);   /* A/B knob: the most tree levels rlx_per_sample descends from LDS (0 .. 11, default 8) */

int rlx_libm_pow(const double *x, const double *y, double *out, int n, int *status,
                 void *stream);  /* out[i] = x[i] ** y[i] as the host libm rounds it (test hook of
                                    the priority arithmetic above; status bit 4 = outside its domain) */

/* ------------------------------------------------- replay storage (K1 / K4) -- */
/* A column of a struct-of-arrays transition store: `row_bytes` bytes per transition. */
#define RLX_MAX_COLUMNS 8
typedef struct rlx_column {
    const void *src;      /* device base of the source array      */
    void *dst;            /* device base of the destination array */
    long long row_bytes;  /* bytes per row (same on both sides)   */
} rlx_column;

/* Row r (0 <= r < n) of every column is copied from source row
 *   src_idx ? src_idx[r] : (src_start + r) mod src_rows      to destination row
 *   dst_idx ? dst_idx[r] : (dst_start + r) mod dst_rows.
 * gather  = ExperienceReplay.sample's `[self.transitions[i] for i in idx]` + Batch collation
 *           (memories/non_episodic/experience_replay.py:80-90, core_types.py:488-649);
 * append  = ExperienceReplay.store + _enforce_max_length as a ring (:117-150).
 * status bit 1 is set for an out-of-range row (the reference's IndexError). */
int rlx_copy_columns(const rlx_column *columns_host, int ncols, const int *src_idx,
                     const int *dst_idx, long long src_start, long long dst_start,
                     long long src_rows, long long dst_rows, int n, int *status, void *stream);

/* Frame-dedup image replay (ObservationStackingFilter + LazyStack,
 * filters/observation/observation_stacking_filter.py:27-41,89-101).
 * ring: u8 [n_env][ring_frames][frame_bytes]; env_fpos/env_epoff: int32[n_env] describe every
 * env's current stacked state; t_fpos (int32) / t_epoff (u8): per stored transition. */
int rlx_imgreplay_reset(unsigned char *ring, int *env_fpos, int *env_epoff,
                        const unsigned char *first_frame, int n_env, int ring_frames,
                        int frame_bytes, void *stream);              /* first observation: stack = [f0]*stack (:90-91) */
int rlx_imgreplay_append(unsigned char *ring, int *env_fpos, int *env_epoff, int *t_fpos,
                         unsigned char *t_epoff, const unsigned char *next_frame,
                         const unsigned char *reset_frame, const unsigned char *done, int n_env,
                         int ring_frames, int frame_bytes, int stack, long long cursor,
                         long long capacity, int record, void *stream); /* deque.append (:93-94) for n_env envs */
int rlx_imgreplay_gather(const unsigned char *ring, const int *t_fpos,
                         const unsigned char *t_epoff, const int *env_fpos, const int *env_epoff,
                         const int *idx, int batch, int n_env, int ring_frames, int frame_bytes,
                         int stack, long long capacity, unsigned char *out_state,
                         unsigned char *out_next, int *status,
                         void *stream);                              /* LazyStack.__array__ (:37-41) for a batch */
/* rlx_imgreplay_gather of sampled rows (stack == 4) + rlx_copy_columns(columns, src_idx = idx, n = batch) of the batch's
 * small columns (actions, rewards, game_overs: core_types.py:488-649) as ONE launch: the columns are gathered by one
 * more workgroup of the same grid (row_bytes * batch <= 65536 per column; the columns' tables have `capacity` rows). */
int rlx_imgreplay_gather_columns(const unsigned char *ring, const int *t_fpos, const unsigned char *t_epoff,
                                 const int *idx, int batch, int n_env, int ring_frames, int frame_bytes, int stack,
                                 long long capacity, unsigned char *out_state, unsigned char *out_next,
                                 const rlx_column *columns_host, int ncols, int *status, void *stream);

/* ------------------------------------- returns / GAE / episode stats (K8 / K12) -- */
/* n_seq independent trajectories of seq_len steps, contiguous; game_overs cut episodes inside a
 * trajectory.  fp64 arithmetic like the reference; `values` are V(s_t) as predicted (fp32).
 * Isolation rule: an episode is computed from its own steps only, as in the reference, which takes one episode at a
 * time.  Nothing behind a game_over reaches the steps before it: a reward or value of +-inf / NaN makes the outputs of
 * ITS episode non-finite (from that step back to the episode's first step) and of no other; bootstrap_values[q] is read
 * only where trajectory q ends without a game_over.  A discount of 0 is not a game_over: inside an episode r + 0 * inf is
 * NaN here as it is in the reference. */
int rlx_gae(const float *rewards, const float *values, const unsigned char *game_overs,
            const float *bootstrap_values, int n_seq, long long seq_len, double discount,
            double gae_lambda, double *advantages, float *value_targets,
            void *stream);   /* agents/actor_critic_agent.py:108-125 + clipped_ppo_agent.py:181-196 */
int rlx_discounted_returns(const float *rewards, const unsigned char *game_overs, int n_seq,
                           long long seq_len, double discount, double *returns64,
                           float *returns32, void *stream);          /* core_types.py:771-801 (n_step = -1) */
/* Signal statistics (utils.py:162-212, agent.py:548-552): table = fp64 [n_signals][5] = {count, sum, sum of
 * squares, max, min}; accumulate folds up to 8 device arrays (fp32 or fp64) into their signals' records in ONE
 * launch; the host reads the table when it logs an episode and resets it. */
typedef struct rlx_signal_source {
    const void *values;   /* device array */
    int n;                /* samples */
    int is_f64;           /* element type: 0 = float, 1 = double */
    int signal;           /* table row */
} rlx_signal_source;
int rlx_signals_reset(double *table, int n_signals, void *stream);
int rlx_signals_accumulate(const rlx_signal_source *sources_host, int n_sources, double *table, int n_signals,
                           void *stream);
int rlx_episode_nstep_returns(const float *rewards, double *out, double *compact_out, long long first_step,
                              int length, int env, int n_env, long long ring_steps, double discount, int n_step,
                              void *stream);   /* core_types.py:771-801 for any n_step, ONE completed episode stored
                                                  time-major (row = ((first_step + k) mod ring_steps) * n_env + env);
                                                  fp64, the reference's summation order (bit-identical).  out: a
                                                  column indexed like `rewards` (or NULL); compact_out: [length]
                                                  (or NULL) — the 'Discounted Return' signal's samples */
int rlx_standardize(const double *x, long long n, float *out32, double *out64, double *mean_std,
                    void *stream);                                   /* clipped_ppo_agent.py:201 (no epsilon) */
int rlx_episode_stats_init(double *ep_return, int *ep_len, int n_env, double *acc, void *stream);
int rlx_episode_stats_step(const float *reward, const unsigned char *game_over, double *ep_return,
                           int *ep_len, int n_env, double *acc, double *last_return,
                           int *last_len, void *stream);             /* agents/agent.py:558-601,509-556 totals */

/* Everything an agent does with one environment response (Agent.observe, agents/agent.py:905-973: reward filters,
 * episode totals, the transition store, the next current state) for up to 1024 vector-observation envs as ONE
 * launch: rlx_reward_filter -> rlx_episode_stats_step -> rlx_copy_columns (action, filtered reward, stored_game_over,
 * current state, next state -> replay row dst_rows[e]) -> rlx_select_rows (cur_state <- reset_obs where game_over).
 * mem_obs == NULL skips the store (evaluation).  Identical arithmetic to the four entry points it replaces. */
typedef struct rlx_observe_desc {
    const float *reward;                 /* [n_env] env rewards                                  */
    float *filtered_reward;              /* [n_env] out                                          */
    double reward_rescale;
    int has_clip;
    double clip_low, clip_high;
    const unsigned char *game_over;      /* [n_env] episode ends (statistics, next current state) */
    const unsigned char *stored_game_over; /* [n_env] what the replay records (TD3 clears time-limit ends) */
    double *ep_return; int *ep_len; double *acc; double *last_return; int *last_len;   /* rlx_episode_stats_step */
    const void *actions; long long action_row_bytes;
    void *cur_state; const void *next_obs; const void *reset_obs; long long obs_row_bytes;
    void *mem_action; float *mem_reward; unsigned char *mem_game_over; void *mem_obs; void *mem_next_obs;
    const int *dst_rows;                 /* [n_env] device: replay row of every env's transition  */
    long long mem_rows;
    int *status;                         /* bit 1: destination row out of range                   */
    int n_env;
} rlx_observe_desc;
int rlx_observe_step(const rlx_observe_desc *desc_host, void *stream);
/* The same for a lockstep rollout buffer (ClippedPPOAgent's acting step, agents/agent.py:905-973 + the episodic memory's
 * store): rlx_reward_filter -> rlx_episode_stats_step -> the step's action / filtered reward / game_over columns at rows
 * [row0, row0 + n_env) as ONE launch (frames go through rlx_imgreplay_append).  status bit 1: a row beyond mem_rows. */
int rlx_rollout_observe_step(const float *reward, float *filtered_reward, double reward_rescale, int has_clip,
                             double clip_low, double clip_high, const unsigned char *game_over, double *ep_return,
                             int *ep_len, double *acc, double *last_return, int *last_len, const void *actions,
                             long long action_row_bytes, void *mem_action, float *mem_reward,
                             unsigned char *mem_game_over, long long row0, long long mem_rows, int n_env, int *status,
                             void *stream);

/* --------------------------------------------------- agent targets (K7 / K10) -- */
/* td_targets holds Q_online(s,.) on entry (fp32 [batch, n_actions]); column actions[i] of row i is
 * replaced by r + (1-done)*discount*Q_target(s', argmax_a q_next_selector(s',a)); td_errors (fp64,
 * optional) receives |new_target - Q_online(s,a)|.  q_next_selector = NULL -> DQN (target net
 * selects, agents/dqn_agent.py:78-79), = Q_online(s',.) -> DDQN (agents/ddqn_agent.py:43).
 * The NaN rules are numpy's.  Selection is np.argmax: the FIRST maximum wins and a NaN counts as the maximum, so the
 * first NaN of a selector row is the greedy action (with the target net selecting, the target is then that NaN; with a
 * separate selector it is Q_target at the NaN's column).  This holds for every Q-row selection that restates this
 * arithmetic: rlx_dqn_head_loss, rlx_dqn_head_loss_backward, rlx_mlp_dqn_update, rlx_mixed_target_head_loss and
 * rlx_bootstrapped_dqn_head_loss.  A row whose action is outside [0, n_actions) sets bit 0 of *status and is left
 * unwritten (td_targets, td_errors). */
int rlx_dqn_targets(const float *q_next_target, const float *q_next_selector, float *td_targets,
                    const int *actions, const float *rewards, const unsigned char *game_overs,
                    double discount, int batch, int n_actions, double *td_errors, int *status,
                    void *stream);                                   /* agents/dqn_agent.py:92-103 */
/* The same targets, the QHead loss (MSE / Huber, importance weighted) and its gradient w.r.t.
 * Q_online in ONE launch: TD_targets equals Q_online except at the taken action, so loss and gradient
 * live at [b, actions[b]] only (dqn_agent.py:92-113, heads/q_head.py, head.py:172-181).
 * importance_weights: the fp64 weights of rlx_per_sample (rounded to fp32 like the TF placeholder) or
 * NULL.  td_errors / td_targets / loss_scalar are optional outputs. */
int rlx_dqn_head_loss(const float *q_online, long long ld_q, const float *q_next_target,
                      const float *q_next_selector, long long ld_next, const int *actions,
                      const float *rewards, const unsigned char *game_overs,
                      const double *importance_weights, double discount, int batch, int n_actions,
                      int huber, float grad_scale, float *dq, long long ld_dq, double *td_errors,
                      float *td_targets, long long ld_targets, float *loss_scalar, int *status,
                      void *stream);
/* DuelingQHead merge (architectures/tensorflow_components/heads/dueling_q_head.py:33-48):
 * q[b,a] = V[b] + (A[b,a] - mean_a A[b,:]); the backward entry point maps dL/dq to dL/dV (row sums)
 * and dL/dA (dq - row mean). */
int rlx_dueling_combine(const float *state_value, const float *action_advantage, int batch,
                        int n_actions, float *q, void *stream);
int rlx_dueling_combine_backward(const float *dq, int batch, int n_actions, float *dstate_value,
                                 float *daction_advantage, void *stream);
/* td_targets[i] = fp32(r + (1 - done) * discount * q_next[i * q_stride]) in float64, or, with
 * use_non_zero_discount_for_terminal_states, fp32(r + (double)((float)discount * q_next[i * q_stride])): the
 * reference's `discount * q_st_plus_1` (ddpg_agent.py:157, td3_agent.py:173) is a python float times an fp32 array, which
 * numpy evaluates as an fp32 product; only the sum with the rewards is float64.  game_overs is not used then.  The same
 * holds for rlx_ac_critic_losses and the fused actor-critic updates.
 * The clip is np.clip, here and in rlx_ac_critic_losses, rlx_td3_smooth_actions, rlx_ac_merge_inputs,
 * rlx_gaussian_action and the fused actor-critic updates: a NaN target, noise draw or action stays NaN (C's fmin / fmax
 * would return the bound and hide a diverged network behind a legal value); +-inf is clipped to the bound. */
int rlx_ac_td_targets(const float *rewards, const unsigned char *game_overs, const float *q_next,
                      int q_stride, double discount, int use_non_zero_discount_for_terminal_states,
                      int has_clip, double clip_low, double clip_high, int batch,
                      float *td_targets, void *stream);              /* agents/ddpg_agent.py:156-164, td3_agent.py:171-180, soft_actor_critic_agent.py:265-266 */
/* One launch for min(q_next1, q_next2) (q_next2 NULL: q_next1), rlx_ac_td_targets and the mean-squared-error
 * loss + gradient of n_streams critic outputs q [n_streams][batch] against those targets (rlx_regression_loss with
 * loss_weight, grad_scale 1): loss[t] per stream, loss[n_streams] = their sum in stream order (the logged total
 * critic loss, td3_agent.py:176-180 / sac_q_head.py:91-95).  q_min_out may be NULL.  batch <= 1024. */
int rlx_ac_critic_losses(const float *q_next1, const float *q_next2, const float *rewards,
                         const unsigned char *game_overs, double discount,
                         int use_non_zero_discount_for_terminal_states, int has_clip, double clip_low,
                         double clip_high, const float *q, int n_streams, int batch, float loss_weight,
                         float *q_min_out, float *td_targets, float *dq, float *loss, void *stream);
/* The critic's merged inputs (concat(action, observation embedding), general_network.py:251,270-277) of the online
 * pass on (s, a) and the target pass on (s', a'): merged2 [2][batch][action_dim + obs_dim]; a' = next_actions with
 * the TD3 target-policy smoothing of rlx_td3_smooth_actions when noise != NULL.  merged_obs_only (may be NULL)
 * [batch][action_dim + obs_dim]: only its observation columns are written (the input of the action-gradient pass,
 * whose action columns the caller fills with the online actor's output). */
int rlx_ac_merge_inputs(const float *actions, const float *obs, const float *next_actions, const double *noise,
                        double noise_clipping, const float *action_low, const float *action_high,
                        const float *next_obs, int batch, int action_dim, int obs_dim, float *merged2,
                        float *merged_obs_only, void *stream);
int rlx_td3_smooth_actions(const float *next_actions, const double *noise, double noise_clipping,
                           const float *action_low, const float *action_high, int batch,
                           int action_dim, float *out, void *stream); /* agents/td3_agent.py:162-165 */
int rlx_sac_value_targets(const float *q_min, const float *sampled_logprob, int batch,
                          float *value_targets, void *stream);       /* agents/soft_actor_critic_agent.py:244 */

/* --------------------------------------- observation / reward filters (K2 / K3) -- */
int rlx_rgb_to_y_u8(const unsigned char *rgb, unsigned char *out, long long n_pixels,
                    double input_low, double input_high,
                    void *stream);   /* filters/observation/observation_rgb_to_y_filter.py:41-47 + observation_to_uint8_filter.py:51-60 */
int rlx_resize_bilinear_u8(const unsigned char *in, unsigned char *out, int n, int H, int W, int C,
                           int OH, int OW,
                           void *stream);   /* filters/observation/observation_rescale_to_size_filter.py:62-79 (skimage resize, order 1) */
int rlx_max_over_frames_u8(const unsigned char *frames, unsigned char *out, int n_env, int n_frames,
                           long long frame_bytes,
                           void *stream);   /* environments/gym_environment.py:148-175: np.max over the newest frames of a frame-skip step */
/* NaN in the running statistics and the reward filter follows numpy / Python, like rlx_clip_by_value: a NaN stays a NaN.
 * rlx_running_stats_push / _merge: np.sqrt(np.maximum(var, epsilon)) — a column that has seen a NaN has NaN sums, mean
 * and std, the other columns are untouched.  rlx_running_stats_normalize: np.clip keeps a NaN input (and a NaN mean or
 * std) NaN in out32 and out64.  rlx_reward_filter, and the same filter inside rlx_observe_step, rlx_rollout_observe_step
 * and rlx_dataset_ingest: min(r, high) / max(r, low) take the bound only where the comparison holds, so a NaN reward is
 * stored as NaN, never as a clipping bound; +-inf clips like any other value. */
int rlx_running_stats_push(const void *samples, int samples_are_f64, long long n, int dim,
                           double *sum, double *sum_squares, double *count, double *mean,
                           double *std, double epsilon,
                           void *stream);                            /* utilities/shared_running_stats.py:130-140 */
/* Data-parallel running statistics (the reference shares them between workers through Redis pub/sub,
 * utilities/shared_running_stats.py:46-67): `delta` = [sum(dim) | sum_squares(dim) | count(1)] summed
 * over all ranks (one all-reduce of 2*dim+1 doubles) is added to the running totals and mean / std
 * are recomputed with the formulas of :137-140. */
int rlx_running_stats_merge(const double *delta, int dim, double *sum, double *sum_squares,
                            double *count, double *mean, double *std, double epsilon, void *stream);
int rlx_running_stats_normalize(const void *x, int x_is_f64, long long n, int dim,
                                const double *mean, const double *std, double clip_low,
                                double clip_high, float *out32, double *out64,
                                void *stream);                       /* utilities/shared_running_stats.py:162-164 */
int rlx_reward_filter(const float *rewards, float *out, long long n, double rescale_factor,
                      int has_clip, double clipping_low, double clipping_high,
                      void *stream);   /* filters/reward/reward_rescale_filter.py:37-39, reward_clipping_filter.py:41-49 */

/* ------------------------------------------- dense / conv layers (fp32 MFMA) -- */
/* RLX_ACT_LEAKY_RELU: v > 0 ? v : 0.2f * v (tf.nn.leaky_relu's default alpha, tensorflow_components/utils.py:34); its
 * derivative through the output is y > 0 ? 1 : 0.2f (alpha at 0, as TF's gradient).  Served by the rlx_dense_small_*
 * launches, rlx_act_backward and rlx_leaky_relu (a wide layer is rlx_gemm without an activation, then rlx_leaky_relu in
 * place); rlx_gemm's epilogue and every fused launch (conv, noisy dense, batch norm, the row chains and the fused MLP /
 * PPO updates) refuse an activation above 2 — the hot kernels compile as they did before the activation existed. */
enum { RLX_ACT_NONE = 0, RLX_ACT_RELU = 1, RLX_ACT_TANH = 2, RLX_ACT_LEAKY_RELU = 3 };

/* C[M,N] (+)= epilogue(A[M,K] * B[K,N]) for `batch` independent problems (strided).
 * A(m,k) = A[off_m + off_k] with off_* = index*stride or a lookup in an int32 table (implicit
 * im2col: rlx_conv_tables); one of the two indices must be contiguous in groups of 4.
 * epilogue: v = act(acc + bias[n]); if deriv_aux: v *= act'(deriv_aux[m][n]) (derivative written in
 * terms of the activation OUTPUT); C = accumulate ? C + v : v.
 * Replaces tf.layers.dense / tf.layers.conv2d and their gradients
 * (architectures/tensorflow_components/layers.py:108-121,168-185). */
struct rlx_small_dense_problem;   /* below: the narrow layers (heads) */
typedef struct rlx_gemm_desc {
    const void *A;            /* float (or uint8 when a_is_u8) */
    const int *a_row_tab;     /* offset per m (elements) or NULL -> m * a_row_stride */
    const int *a_k_tab;       /* offset per k or NULL -> k * a_k_stride            */
    const float *B;
    float *C;
    const float *bias;        /* [N] or NULL */
    const float *deriv_aux;   /* [M, aux_ld] or NULL */
    float *workspace;         /* split-K partials, or NULL to forbid splitting */
    float *colsum_out;        /* optional [N]: sum_k B[k][n] (the bias gradient rides on the dW GEMM) */
    long long a_row_stride, a_k_stride, a_batch_stride;
    long long b_k_stride, b_n_stride, b_batch_stride;
    long long ldc, c_batch_stride, bias_batch_stride;
    long long aux_ld, aux_batch_stride;
    long long workspace_floats;
    long long colsum_batch_stride;
    int M, N, K, batch;
    int a_is_u8;              /* A holds bytes; value = byte / a_div (embedders/embedder.py:107-108) */
    int a_vec_along_k;        /* with tables: 1 = 4 consecutive k are contiguous, 0 = 4 consecutive m */
    int a_tab_vec_ok;         /* with tables: groups of 4 are contiguous AND 16-byte (4-byte for u8) aligned */
    int activation, deriv_kind, accumulate;
    float a_div;
    /* two-level batch addressing of A, B and bias (0 = off): batch index b = bo * batch_inner + bi,
     * operand offset = bo * *_batch_stride2 + bi * *_batch_stride.  Lets the online and the target
     * copy of a multi-stream layer run as one launch (network_wrapper.py:188-213 parallel_prediction). */
    int batch_inner;
    long long a_batch_stride2, b_batch_stride2, bias_batch_stride2;
    /* n_fold > 0 (with batch == 1): N counts the columns of N / n_fold towers that SHARE the A operand;
     * column n uses tower n / n_fold: B, C, bias and colsum_out are addressed at
     * tower * *_batch_stride + (n % n_fold).  The separate value / policy networks of Clipped PPO
     * (clipped_ppo_agent.py:50) read the same observation: their first layer gathers it once. */
    int n_fold;
    /* Narrow layers that read ROWS of this product's output (the value / policy heads on the last dense layer of their
     * tower, heads/v_head.py:43-48, ppo_head.py:100-116): row_heads[i].x must be C + t * c_batch_stride for a batch entry
     * t (one head per entry at most), K = N of this product, M = M, towers = 1, N <= 16.  When the product is split over
     * K, the reduction pass that finishes a row (bias, activation) computes its head outputs right there — the row is in
     * LDS — instead of a separate launch; otherwise rlx_gemm runs rlx_dense_small_forward_multi(row_heads) behind the
     * product.  Either way y of every head is complete in stream order, with identical values.  NULL / 0: none. */
    const struct rlx_small_dense_problem *row_heads;
    int n_row_heads;
    /* 0: the library's rule (rlx_gemm_tuning's kw_min_tiles, default 192).  > 0: for THIS product, the fewest 32 x 64 / 32 x 32
     * tiles for which K is split over the waves of a workgroup (no partials, no reduce launch) rather than over workgroups.
     * A dense layer's input gradient at batch 32 (M = 32, N = 3136, K = 512: 98 tiles of 32 x 32) sits in the chain of the
     * update in front of the convolutions' backward pass: with 96 it is one launch of 13.7 us instead of 12.4 + a 4.7 us reduce
     * launch (coach_amd/nn/graph.py Dense.backward; profiles/r06_ab_c3_kw_min_tiles.txt). */
    int kw_min_tiles;
} rlx_gemm_desc;

int rlx_gemm(const rlx_gemm_desc *desc_host, void *stream);
int rlx_gemm_workspace_floats(int M, int N, int K, int batch, long long *floats_host);
/* Path selection of rlx_gemm (process-wide; defaults 192 / 192 / -1): a problem whose 64 x 64 tiling has fewer than
 * kw_below_tiles tiles runs on 32 x 64 / 32 x 32 tiles with the K slab split over the waves of a workgroup, if that
 * tiling has at least kw_min_tiles tiles.  xcd_mode: how the tiled kernels hand the tile order to the 8 XCDs (one L2
 * each): 0 = every 8th tile (the hardware's order), G = 2^k > 0: groups of G consecutive tiles round-robin, -1 = one
 * contiguous share per XCD — so that tiles sharing operand rows share an L2.
 * An explicit knob for same-process A/B measurements (tools/ab_c2.py); results are identical either way. */
int rlx_gemm_tuning(int kw_below_tiles, int kw_min_tiles, int xcd_mode);
/* the current values (NULL: not wanted) — what a caller that mirrors rlx_gemm's tile rule (coach_amd/nn/graph.py
 * _kw2_tiling: where rlx_conv23_forward is bit-identical to the tiled launches) must read instead of assuming the defaults */
int rlx_gemm_tuning_get(int *kw_below_tiles, int *kw_min_tiles, int *xcd_mode);
/* What rlx_gemm WOULD launch for this descriptor, without launching: out8 = {vector-load tiled kernel (else: thin / generic
 * paths, the other fields are then meaningless), tile rows, tile columns, wave groups per K slab, K chunks over workgroups
 * (> 1: partials + a reduce launch), chunk length, operands through the LDS-DMA ring (0: staged by registers — the order
 * of the fp32 sum inside a slab differs, see rlx_gemm_pipeline), thin kernel}.  For callers that replace a launch by a
 * fused one ONLY where the sums stay bit-identical (rlx_conv123_forward).  The answer is the plan of the product as one
 * member of a combined grid (rlx_gemm_pair, rlx_gemm_multi_defer) — the summation order, which is what such callers ask
 * about.  A launch of its own differs from it in two ways that leave every sum as it is: a product of at least 256 tiles
 * of 128 x 128 runs on those (rlx_gemm_big_tiles: bit-identical to the 64 x 64 tiling reported here), and the thin kernel
 * takes its 16 x 16 tiles up to twice as many 32 x 32 tiles.  All zeros: towers folded into N (n_fold) that have to run
 * as the equivalent batched product. */
int rlx_gemm_describe(const rlx_gemm_desc *desc, int *out8);
/* Main loop of the fast tiled kernels: 1 (default) = operand slabs go global -> LDS by DMA into a ring of two buffers,
 * one barrier per slab, three workgroups per CU (csrc/gemm.hip gemm_dma_body); 0 = the register-staged two-set pipeline
 * of rounds 1-3 (128 x 32 tiles always use it); 2 = the ring for uint8 operands too (4-byte requests; measured equal to 1).  Same products, same tiles; the order of the fp32 sum inside a 32-deep slab differs between the two
 * (both deterministic).  Process-wide, read at launch (or capture) time: exists for same-process A/B measurements. */
int rlx_gemm_pipeline(int lds_dma_ring);
/* 64 x 64 (or 64 x 32) per wave (2 x 2 / 2 x 1 accumulator tiles; 128 x 128 or 128 x 64 per workgroup) for products of at least 256 such tiles
 * without a K split: 1 (default: 128 x 128 for N >= 128) / 0 / 2 (also 128 x 64 for N <= 64, measured neutral on the
 * convolution layers of the whole-dataset passes).  Bit-identical results either way
 * (every element stays one chain over K); process-wide, for same-process A/Bs and tests. */
int rlx_gemm_big_tiles(int on);
/* The most K splits rlx_gemm cuts one product into (default 64; the workspace given with the descriptor bounds it as
 * well).  Process-wide, read at launch / capture time: a knob for same-process A/B measurements. */
int rlx_gemm_split_cap(int max_splits);

/* Input gradient of a VALID-padding NHWC convolution (tf.gradients of tf.layers.conv2d,
 * architectures/tensorflow_components/layers.py:108-121, architecture.py:187-220) as ONE product that gathers dY
 * directly — no column matrix in memory, no col2im pass:
 *   dx[t][b, iy, ix, c] = act'(x_out[t][b, iy, ix, c]) * sum_{ky, kx, co : iy = s*oy + ky, ix = s*ox + kx}
 *                         dy[t][b, oy, ox, co] * weights[t][ky, kx, c, co]
 * for `towers` independent networks (tower strides in elements).  The s*s phases (iy % s, ix % s) of the input are the
 * row blocks of one GEMM with M = s*s*rows, N = C, K = (KH/s)*(KW/s)*Co whose A operand is a windowed gather of dy
 * (fp32 MFMA, exact products).  Needs KH % s == 0, KW % s == 0, C % 4 == 0, Co % 4 == 0 and K <= 1024.
 * `tables`: int32 device buffer of rlx_conv_input_grad_tables_ints(...) entries filled once per geometry by
 * rlx_conv_input_grad_tables.  deriv_kind != 0 multiplies by the activation derivative of the producing layer's OUTPUT
 * x_out (same layout as dx). */
int rlx_conv_input_grad_tables_ints(int batch, int H, int W, int C, int KH, int KW, int stride, int Co,
                                    long long *ints_host);
int rlx_conv_input_grad_tables(int *tables, int batch, int H, int W, int C, int KH, int KW, int stride, int Co,
                               void *stream);
int rlx_conv_input_grad(const float *dy, const float *weights, float *dx, const float *x_out, int deriv_kind,
                        const int *tables, int batch, int H, int W, int C, int KH, int KW, int stride, int Co,
                        int towers, long long dy_tower_stride, long long w_tower_stride, long long dx_tower_stride,
                        void *stream);
/* A layer's weight gradient (dW = X^T dY) and input gradient (dX = dY W^T) — two independent products of the same
 * dY — as ONE launch when both take the tiled kernel or both the thin kernel (two launches otherwise).
 * Each descriptor is exactly what rlx_gemm would get; when both split K they need disjoint workspaces. */
int rlx_gemm_pair(const rlx_gemm_desc *weight_grad, const rlx_gemm_desc *input_grad, void *stream);

/* Deferred split-K reduction.  A weight gradient dW = X^T dY has a tiny output and a long reduction (the batch), so
 * its K is split over workgroups into partial sums [batch][split][M][N] in the workspace, and summing them is a second
 * launch.  Nobody reads a weight gradient before the optimiser does, so the backward pass of a network can leave
 * the partials of ALL its layers where they are and sum them in ONE launch at its end: rlx_gemm_defer /
 * rlx_gemm_pair_defer run the product(s) and, if K was split, describe the outstanding reduction in *job (job->splits
 * > 1) instead of launching it; rlx_splitk_reduce_jobs sums up to RLX_MAX_SPLITK_JOBS of them (fixed summation order:
 * reproducible).  The workspace of a deferred product must stay untouched until its job has run.  Only plain
 * products qualify (no bias / activation / derivative / accumulate epilogue — a weight gradient has none). */
#define RLX_MAX_SPLITK_JOBS 8
typedef struct rlx_splitk_job {
    const float *partials;        /* [batch][splits][M][N] */
    const float *colsum_partials; /* [batch][splits][N] or NULL */
    float *C;
    float *colsum_out;
    long long ldc, c_batch_stride, colsum_batch_stride;
    int M, N, batch, splits;      /* splits <= 1: nothing outstanding */
    int n_fold;
} rlx_splitk_job;
int rlx_gemm_defer(const rlx_gemm_desc *desc_host, rlx_splitk_job *job_host, void *stream);
int rlx_gemm_pair_defer(const rlx_gemm_desc *weight_grad, const rlx_gemm_desc *input_grad,
                        rlx_splitk_job *weight_grad_job_host, void *stream);
int rlx_splitk_reduce_jobs(const rlx_splitk_job *jobs_host, int n_jobs, void *stream);
/* Up to three weight-gradient products (the convolution layers' dW = cols^T dz of one backward pass,
 * architectures/tensorflow_components/architecture.py:187-220 tf.gradients) as ONE launch, each with the tiling and K split
 * rlx_gemm would give it alone (bit-identical sums) and its split-K reduction deferred into jobs[i] as rlx_gemm_defer
 * does (jobs[i].splits = 0: nothing to reduce).  Descriptors that do not qualify for the one-launch form (anything but
 * 64 x 64 tiles of an im2col-gathered A^T) are launched one by one. */
int rlx_gemm_multi_defer(const rlx_gemm_desc *descs, int n, rlx_splitk_job *jobs, void *stream);
/* Diagnostics (tools/gemm_timeline.py): while a device buffer of `capacity_u64` 64-bit words is registered, every
 * tiled-kernel launch of rlx_gemm records, per workgroup, four wall-clock ticks (10 ns: entry, first slab staged,
 * main loop done, exit) in its own region of the buffer; rlx_gemm_debug_calls lists the regions as rows of
 * {M, N, K, batch, splits, grid.x, grid.y, grid.z, offset}.  buffer == NULL switches the stamps off (the default). */
int rlx_gemm_debug_stamps(void *buffer, long long capacity_u64);
int rlx_gemm_debug_calls(long long *out_host, int max_calls, int *n_calls_host);
int rlx_colsum(const float *x, int M, int N, long long ld, float *out, int accumulate,
               float *workspace, long long workspace_floats, void *stream);  /* bias gradients */
int rlx_act_backward(float *dy, const float *y, long long n, int kind, void *stream); /* dy *= act'(y) */
int rlx_leaky_relu(float *y, long long n, void *stream);             /* y = y > 0 ? y : 0.2f * y, in place */
int rlx_conv_tables(int *rowbase, int *koff, int batch, int H, int W, int C, int KH, int KW,
                    int stride, void *stream);      /* VALID-padding NHWC im2col offsets */
int rlx_col2im(const float *dcol, float *dx, const float *x_out, int deriv_kind, int batch, int H,
               int W, int C, int KH, int KW, int stride, void *stream); /* conv input gradient */

/* Batch normalisation after a dense layer — the `use_batchnorm=True` DDPG networks (agents/ddpg_agent.py:37-60;
 * architectures/tensorflow_components/layers.py:26-55 -> tf.layers.batch_normalization: momentum 0.99, epsilon 1e-3).
 * x, y, dy, dx: [batch][channels] fp32, rows contiguous; gamma, beta, statistics: [channels].
 *   rlx_bn_forward   training != 0: batch mean / population variance (written to save_mean / save_var), else the moving
 *                    statistics;  y = act(x * inv + (beta - mean * inv)),  inv = rsqrt(var + eps) * gamma
 *   rlx_bn_backward  dy = d loss / d y: multiplies by act'(y) (activation 0: dy is already d loss / d u), writes dx and,
 *                    unless NULL, dgamma / dbeta (gradients_wrt_inputs passes need no weight gradients)
 *   rlx_bn_update_moving  m -= (m - batch) * (1 - momentum): the UPDATE_OPS that run before apply_gradients
 *                    (architecture.py:273-277) on the batch fed with it (ddpg_agent.py:178-193) */
int rlx_bn_forward(const float *x, const float *gamma, const float *beta, const float *moving_mean,
                   const float *moving_var, int batch, int channels, double epsilon, int training, int activation,
                   float *y, float *save_mean, float *save_var, void *stream);
int rlx_bn_backward(const float *dy, const float *y, const float *x, const float *gamma, const float *save_mean,
                    const float *save_var, int batch, int channels, double epsilon, int activation, float *dx,
                    float *dgamma, float *dbeta, void *stream);
int rlx_bn_update_moving(float *moving_mean, float *moving_var, const float *batch_mean, const float *batch_var,
                         int channels, double momentum, void *stream);

/* Fused small-MLP DQN update: DQNAgent.learn_from_batch (agents/dqn_agent.py:81-113) for a vector-observation
 * Q network  obs -> Dense(h1, relu) -> Dense(h2, relu) -> Dense(n_actions)  in ONE launch: online / target (/ Double
 * DQN selector) forward passes, TD targets, |TD errors|, MSE or Huber loss with importance weights
 * (heads/q_head.py, head.py:143-186), backward, TF1 Adam (general_network.py:390-394) and tf.global_norm.
 * h2 / 32 workgroups each own a 32-column slice of the wide layer; two in-kernel exchanges (csrc/mlp_fused.hip).
 * All pointers are device pointers; weights / target_weights / adam_m / adam_v are the network's flat buffers and
 * off_* the element offsets of the six tensors ([obs,h1] [h1] [h1,h2] [h2] [h2,A] [A], row-major) inside them.
 * sync_words: 3 zero-initialised uint32 owned by this network (the kernel leaves them zero).  status bits: 1 = action
 * out of range, 8 = an in-kernel barrier timed out (results invalid). */
typedef struct rlx_mlp_dqn_desc {
    float *weights; const float *target_weights; float *adam_m; float *adam_v; float *adam_state;
    const float *states; const float *next_states; const int *actions; const float *rewards;
    const unsigned char *game_overs; const double *importance_weights;   /* fp64 [batch] or NULL */
    float *workspace; unsigned int *sync_words;
    float *loss_out; float *norm_out; double *td_errors; int *status;
    long long workspace_floats;
    long long off_w1, off_b1, off_w2, off_b2, off_w3, off_b3;
    double discount;
    int batch, obs_dim, h1, h2, n_actions;
    int huber, double_dqn;
    float learning_rate, beta1, beta2, epsilon, grad_scale;
} rlx_mlp_dqn_desc;
int rlx_mlp_dqn_supported(int batch, int obs_dim, int h1, int h2, int n_actions);   /* 1 / 0 (a value, not a status) */
int rlx_mlp_dqn_workspace_floats(int h1, int h2, int n_actions, long long *floats_host);
int rlx_mlp_dqn_update(const rlx_mlp_dqn_desc *desc_host, void *stream);
/* Acting with the same network: q_out [n_env][n_actions] = Q(states) (may be NULL) and, when actions != NULL, the
 * epsilon-greedy choice of rlx_egreedy on those values — one launch of one workgroup for n_env <= 8 envs
 * (agents/dqn_agent.py choose_action + exploration_policies/e_greedy.py:84-101).  Weights at the element offsets
 * off_* of the flat parameter buffer, [in][out] storage. */
int rlx_mlp_q_act_supported(int n_env, int obs_dim, int h1, int h2, int n_actions);   /* 1 / 0 (a value) */
int rlx_mlp_q_act(const float *weights, long long off_w1, long long off_b1, long long off_w2, long long off_b2,
                  long long off_w3, long long off_b3, const float *states, int n_env, int obs_dim, int h1, int h2,
                  int n_actions, const double *explore_uniforms, const int *random_actions,
                  const double *tie_break_uniforms, double epsilon, float *q_out, int *actions, void *stream);

/* Narrow dense layers (1 <= N <= 16 outputs: value / policy / Q heads) as coalesced fp32 FMA
 * kernels instead of MFMA tiles (heads/v_head.py:43-48, ppo_head.py:100-116, q_head.py,
 * ddpg_actor_head.py:48-56, td3_v_head.py:40-60).  Tower t of every operand sits at
 * base + t * tower_stride (x_tower_stride = 0: one input shared by all towers).
 * forward : y = act(x W + b)
 * backward: dz = dy * act'(y) (y may be NULL when activation == NONE); dw = x^T dz; db = 1^T dz;
 *           dx = dz W^T, multiplied by lower_activation'(x) when lower_activation != NONE (dx is then
 *           the lower layer's dz).  dw/db or dx may be NULL. */
int rlx_dense_small_forward(const float *x, long long x_tower_stride, const float *w,
                            long long w_tower_stride, const float *bias, long long bias_tower_stride,
                            float *y, long long y_tower_stride, int towers, int M, int K, int N,
                            int activation, void *stream);
int rlx_dense_small_backward(const float *x, long long x_tower_stride, const float *w,
                             long long w_tower_stride, const float *dy, long long dy_tower_stride,
                             const float *y, long long y_tower_stride, float *dw,
                             long long dw_tower_stride, float *db, long long db_tower_stride, float *dx,
                             long long dx_tower_stride, int towers, int M, int K, int N, int activation,
                             int lower_activation, void *stream);

/* Up to 4 narrow layers of the same depth in ONE launch (e.g. the value and the policy head of
 * Clipped PPO, clipped_ppo_agent.py:41-58: separate towers, widths 1 and A).  Field meaning as the
 * single-layer calls; `y` is the forward output, and in backward the layer output needed for the
 * activation derivative (may be NULL when activation == NONE). */
typedef struct rlx_small_dense_problem {
    const float *x; long long x_tower_stride;
    const float *w; long long w_tower_stride;
    const float *bias; long long bias_tower_stride;
    float *y; long long y_tower_stride;
    const float *dy; long long dy_tower_stride;
    float *dw; long long dw_tower_stride;
    float *db; long long db_tower_stride;
    float *dx; long long dx_tower_stride;
    int towers, M, K, N, activation, lower_activation;
} rlx_small_dense_problem;
/* rlx_dqn_head_loss + the Q head's backward pass (rlx_dense_small_backward of q_head: dW, db, dx with the lower layer's
 * activation derivative; tf.gradients through the head, architecture.py:312-385) as ONE launch.  q_head: x, w, dy (receives
 * dQ), dw / db / dx as for rlx_dense_small_backward_multi, one linear tower with M = batch <= 256, N = n_actions <= 16.
 * Values: those of the two launches bit for bit (the same row arithmetic, the same reduction trees). */
int rlx_dqn_head_loss_backward(const rlx_small_dense_problem *q_head, const float *q_online, long long ld_q,
                               const float *q_next_target, const float *q_next_selector, long long ld_next,
                               const int *actions, const float *rewards, const unsigned char *game_overs,
                               const double *importance_weights, double discount, int batch, int n_actions, int huber,
                               float grad_scale, double *td_errors, float *loss_scalar, int *status, void *stream);
int rlx_dense_small_forward_multi(const rlx_small_dense_problem *problems_host, int n_problems, void *stream);
int rlx_dense_small_backward_multi(const rlx_small_dense_problem *problems_host, int n_problems, void *stream);
/* Discrete Clipped-PPO: the losses of both heads (heads/ppo_head.py:52-116, v_head.py:43-52, head.py:143-186) AND the
 * heads' backward pass (their share of accumulate_gradients, architecture.py:312-385) in ONE launch — what
 * rlx_ppo_discrete_value_losses followed by rlx_dense_small_backward_multi({value_head, policy_head}) computes, bit for bit
 * (every workgroup of the backward recomputes the batch's loss-gradient rows instead of reading them behind a launch
 * boundary).  Heads: one linear tower each over the `batch` <= 256 rows, value N = 1, policy N = n_actions <= 16; their .dy
 * (optional) receives dV / dlogits, .dw / .db / .dx as in the backward call.  scalars[5] = {surrogate loss, mean entropy,
 * mean KL(old||new), policy head total, value loss}; clip_scale: device scalar or NULL (see rlx_ppo_discrete_loss). */
int rlx_ppo_heads_loss_backward(const rlx_small_dense_problem *value_head, const rlx_small_dense_problem *policy_head,
                                const float *values, const float *value_targets, const float *logits,
                                const int *actions, const float *advantages, const float *old_probs, long long ld_old,
                                int batch, float clip_epsilon, const float *clip_scale, float beta_entropy,
                                float grad_scale, float *scalars, float *likelihood_ratio,
                                float *clipped_likelihood_ratio, int *status, void *stream);
/* The same update with the heads' work split by what it depends on (round 6).  Everything of rlx_ppo_heads_loss_backward that
 * is LOCAL TO A ROW — the head's forward on the finished row, the row's loss terms (heads/ppo_head.py:52-116, v_head.py:43-52,
 * head.py:143-186), the gradient at the head's outputs and dz = act'(h) (dy W_head^T), the gradient at the last dense layer's
 * pre-activation output (architecture.py:312-385) — runs in the workgroup that finishes that row of the dense layer
 * (layers.py:168-185: its K-split reduction, one workgroup per row and tower): rlx_ppo_fc_rows = rlx_gemm(fc) with
 * row_heads = {value_head, policy_head} + the row-local part.  What needs ALL rows and is read by nobody before the
 * optimizer step — dW / db of both heads, scalars[5] — is rlx_ppo_heads_tail, a launch of its own, or
 * rlx_splitk_reduce_jobs_ppo_tail: extra workgroups of the backward pass's deferred-reduction launch (rlx_splitk_reduce_jobs).
 * Two launches of the update's chain become none.  Values: those of rlx_gemm(row_heads) + rlx_ppo_heads_loss_backward bit for
 * bit (the same per-row arithmetic, the same chains and reduction trees).
 * value_head / policy_head as for rlx_ppo_heads_loss_backward, all of x, w, y, dy, dw, dx required: x = the tower's rows of
 * fc->C, y receives V / the logits, dy dV / dlogits, dx dz of the tower.  row_terms: [batch][4] floats of scratch that carries
 * {value loss term, surrogate, entropy, KL} of each row from the rows launch to the tail.
 * rlx_ppo_fc_rows_supported(fc, n_actions) -> 1 where rlx_gemm would split fc (two towers, <= 256 rows, N % 4 == 0,
 * N <= 1024, no row_heads of its own) into more than 16 K chunks, i.e. where the row-finishing reduction runs. */
typedef struct rlx_ppo_rows_desc {
    rlx_small_dense_problem value_head, policy_head;
    const float *value_targets;
    const int *actions;
    const float *advantages;
    const float *old_probs; long long ld_old;
    const float *clip_scale;               /* device scalar or NULL (see rlx_ppo_discrete_loss) */
    float clip_epsilon, beta_entropy, grad_scale;
    int batch;
    float *row_terms;
    float *scalars;                        /* [5] as in rlx_ppo_heads_loss_backward */
    float *likelihood_ratio, *clipped_likelihood_ratio;   /* [batch] or NULL */
    int *status;
} rlx_ppo_rows_desc;
int rlx_ppo_fc_rows_supported(const rlx_gemm_desc *fc, int n_actions);
int rlx_ppo_fc_rows(const rlx_gemm_desc *fc, const rlx_ppo_rows_desc *rows, void *stream);
int rlx_ppo_heads_tail(const rlx_ppo_rows_desc *rows, void *stream);
int rlx_splitk_reduce_jobs_ppo_tail(const rlx_splitk_job *jobs_host, int n_jobs, const rlx_ppo_rows_desc *rows, void *stream);
/* rlx_splitk_reduce_jobs + rlx_per_update(idx, td_errors, n <= 64) as ONE launch: PrioritizedExperienceReplay.
 * update_priorities (memories/non_episodic/prioritized_experience_replay.py:203-217; called right behind learn_from_batch,
 * agents/dqn_agent.py:106-109) is one workgroup, dispatched first, of the backward pass's deferred-reduction launch — the TD
 * errors exist since the head's loss, and nothing reads the trees before the next sample().  Trees bit-identical to
 * rlx_per_update's.  No deferred job with splits > 1: rlx_per_update as a launch of its own. */
int rlx_splitk_reduce_jobs_per_update(const rlx_splitk_job *jobs_host, int n_jobs, double *sum_tree, double *min_tree,
                                      double *max_tree, int capacity, const int *idx, const double *td_errors, int n,
                                      double alpha, double epsilon, double *max_priority, int *status, void *stream);

/* -------------------------------------------------------- head losses (K9) -- */
/* loss = mean_b(loss_weight * w_b * sum_j l(target, out)); kind 0 = MSE, 1 = Huber(delta 1).
 * grad (optional) = grad_scale * d loss / d out.  heads/head.py:143-186, q_head.py, v_head.py:43-52 */
int rlx_regression_loss(const float *out, long long ld_out, const float *target,
                        long long ld_target, const float *importance_weights, int batch, int dim,
                        int kind, float loss_weight, float grad_scale, float *grad,
                        long long ld_grad, float *loss_scalar, void *stream);
int rlx_softmax(const float *logits, long long ld, int batch, int n, float *probs,
                long long ld_out, void *stream);                    /* heads/ppo_head.py:108 */
/* scalars[4] = {surrogate loss, mean entropy, mean KL(old||new), total head loss}.
 * The clip range is clip_epsilon (clip_likelihood_ratio_using_epsilon) times the clip_param_rescaler placeholder
 * (heads/ppo_head.py:52-116, clipped_ppo_agent.py:266-268): pass the rescaler either folded into clip_epsilon
 * (clip_scale NULL) or as a DEVICE scalar clip_scale[0] — a captured hipGraph then serves a decaying
 * clipping_decay_schedule (presets/Mujoco_ClippedPPO.py) without being re-captured for every new value. */
int rlx_ppo_discrete_loss(const float *logits, long long ld, const int *actions,
                          const float *advantages, const float *old_probs, long long ld_old,
                          int batch, int n_actions, float clip_epsilon, float beta_entropy,
                          float grad_scale, float *dlogits, long long ld_grad, float *scalars,
                          float *likelihood_ratio, float *clipped_likelihood_ratio, int *status,
                          const float *clip_scale, void *stream);

/* rlx_ppo_discrete_loss and the VHead MSE loss (rlx_regression_loss, dim 1, weight 1) of the same
 * minibatch in ONE launch: values / value_targets / dvalues are [batch]. */
int rlx_ppo_discrete_value_losses(const float *logits, long long ld, const int *actions,
                                  const float *advantages, const float *old_probs, long long ld_old,
                                  int batch, int n_actions, float clip_epsilon, float beta_entropy,
                                  float grad_scale, float *dlogits, long long ld_grad, float *scalars,
                                  float *likelihood_ratio, float *clipped_likelihood_ratio, int *status,
                                  const float *values, const float *value_targets, float *dvalues,
                                  float *value_loss_scalar, const float *clip_scale, void *stream);

/* Continuous policy (heads/ppo_head.py:118-144): MultivariateNormalDiag(mean, exp(log_std) + eps),
 * log_std one state-independent vector [action_dim]; old_std is the old network's policy_std output.
 * dlog_std[action_dim] receives the batch-summed gradient.  scalars as rlx_ppo_discrete_loss. */
int rlx_ppo_continuous_loss(const float *mean, long long ld, const float *log_std, const float *actions,
                            const float *advantages, const float *old_mean, const float *old_std,
                            long long ld_old, int batch, int action_dim, float clip_epsilon,
                            float beta_entropy, float grad_scale, float *dmean, long long ld_grad,
                            float *dlog_std, float *scalars, float *likelihood_ratio,
                            float *clipped_likelihood_ratio, const float *clip_scale, void *stream);

/* PPO-penalty head (agents/ppo_agent.py; heads/ppo_head.py:52-98 without clipping): unclipped surrogate plus
 * kl_coefficient * KL + high_kl_penalty_coefficient * max(0, KL - kl_cutoff)^2 with KL the BATCH mean of
 * KL(old || new), so every gradient row carries c = kl_coefficient + 2 * high * max(0, KL - kl_cutoff).  One launch of
 * one workgroup, batch <= 1024, no float atomics.  Arguments as rlx_ppo_discrete_loss / rlx_ppo_continuous_loss without
 * the clip ones; kl_coefficient is a DEVICE scalar (read by the kernel, so a captured graph follows
 * rlx_ppo_kl_coefficient_update); kl_cutoff = 2 * target_kl_divergence; use_kl_regularization = 0 drops both KL terms.
 * scalars[5] = {surrogate loss, mean entropy, mean KL, total, c}.  accumulate (optional, 4 device floats) receives
 * += {mean KL, mean entropy, total, 1}: an epoch's running sums.  Every output is optional.
 * Discrete: 1 <= n_actions <= 18; an action outside [0, n_actions) sets status bit 0, and its row adds no term (the
 * means still divide by batch), gets a zero gradient row and a likelihood ratio of 0.
 * Continuous: 1 <= action_dim <= 32; dlog_std[action_dim] receives the batch-summed gradient. */
int rlx_ppo_kl_discrete_loss(const float *logits, long long ld, const int *actions, const float *advantages,
                             const float *old_probs, long long ld_old, int batch, int n_actions, float beta_entropy,
                             float grad_scale, const float *kl_coefficient, float kl_cutoff,
                             float high_kl_penalty_coefficient, int use_kl_regularization, float *dlogits,
                             long long ld_grad, float *scalars, float *likelihood_ratio, int *status, float *accumulate,
                             void *stream);
int rlx_ppo_kl_continuous_loss(const float *mean, long long ld, const float *log_std, const float *actions,
                               const float *advantages, const float *old_mean, const float *old_std, long long ld_old,
                               int batch, int action_dim, float beta_entropy, float grad_scale,
                               const float *kl_coefficient, float kl_cutoff, float high_kl_penalty_coefficient,
                               int use_kl_regularization, float *dmean, long long ld_grad, float *dlog_std,
                               float *scalars, float *likelihood_ratio, float *accumulate, void *stream);
/* update_kl_coefficient (agents/ppo_agent.py:329-353) on the device: mean KL = epoch_sums[0] / epoch_sums[3] (the
 * accumulate buffer above); kl_coefficient[0] *= 1.5 when it exceeds 1.3 * target_kl, /= 1.5 when it is below
 * 0.7 * target_kl (fp32 comparisons against the fp64 products rounded to fp32, fp32 product / quotient);
 * kl_mean_out (optional) receives the mean.  A count epoch_sums[3] of 0 (nothing accumulated) leaves the coefficient
 * as it is and writes a mean of 0.  target_kl is the python float itself: float(1.3 * 0.01) differs from
 * float(1.3 * float(0.01)). */
int rlx_ppo_kl_coefficient_update(const float *epoch_sums, double target_kl, float *kl_coefficient, float *kl_mean_out,
                                  void *stream);

/* ------------------------------------------ optimiser / target mixing (K11) -- */
/* state = {beta1_power, beta2_power} (2 device floats).  tf.train.AdamOptimizer as built in
 * architectures/tensorflow_components/general_network.py:390-394. */
int rlx_adam_init(float *m, float *v, long long n, float *state, float beta1, float beta2,
                  void *stream);
int rlx_adam_tf1(float *weights, const float *grads, float *m, float *v, long long n,
                 float learning_rate, float beta1, float beta2, float epsilon, float *state,
                 float grad_scale, void *stream);
/* rlx_adam_tf1 that also returns tf.global_norm of the (unscaled) gradients it consumed: the
 * per-workgroup sums of squares ride on the Adam pass (no second read of the gradients) and the
 * one-thread finish kernel that advances the beta powers also takes the square root and, when
 * n_acc > 0, adds acc_src[0..n_acc) (loss terms / the norm just written) onto the running sums
 * acc_dst (the per-epoch signal means of agents/agent.py:743-767, utils.py:162-212). */
int rlx_adam_tf1_norm(float *weights, const float *grads, float *m, float *v, long long n,
                      float learning_rate, float beta1, float beta2, float epsilon, float *state,
                      float grad_scale, float *norm_out, float *workspace, long long workspace_floats,
                      const float *acc_src, float *acc_dst, int n_acc, void *stream);
/* rlx_adam_tf1 / rlx_adam_tf1_norm with (target != NULL) the soft target update
 * target = rate * w_new + (1 - rate) * target (rlx_mix_weights' arithmetic) in the same elementwise pass.  Without
 * norm_out it is ONE launch: the last workgroup to finish (device ticket, no fence) advances the beta powers.  With
 * norm_out it is one launch as well when a workgroup's share fits its registers (up to 4.2 M parameters; larger buffers
 * take the two-launch form): the sums of squares are complete before the first store and are published without a
 * release fence (agent-scope atomics), and the workgroup that draws the last ticket does the finish — same arithmetic,
 * same order, bit-identical to the two-launch form.
 * ticket: RLX_ADAM_TICKET_WORDS zero-initialised 32-bit device words owned by this optimiser (a two-level last-arriver
 * count: 32 group words + 1, each on its own 128-byte line); the kernel re-arms them. */
#define RLX_ADAM_TICKET_WORDS 1056
int rlx_adam_tf1_step(float *weights, const float *grads, float *m, float *v, long long n, float learning_rate,
                      float beta1, float beta2, float epsilon, float *state, float grad_scale, float *norm_out,
                      float *workspace, long long workspace_floats, const float *acc_src, float *acc_dst, int n_acc,
                      float *target, double mix_rate, unsigned int *ticket, void *stream);
/* How rlx_adam_tf1_step finishes the gradient norm: 2 (default) inside the Adam launch, the workgroup's share held in
 * registers (falls back to 0 beyond 4.2 M parameters); 1: inside the grid-stride Adam launch (any size; measured equal to
 * 0); 0: the separate finish launch.  Process-wide, read at launch / capture time: for same-process A/Bs and tests. */
int rlx_adam_norm_in_kernel(int on);
/* The register-held one-launch step SPLIT over two launches.  Its grid is a list of VIRTUAL blocks (rlx_adam_step_blocks:
 * the grid rlx_adam_tf1_step would launch for n parameters and this workspace, 0 where it would not take that form); a
 * block's elements, its additions and its partial sum of squares do not depend on which launch runs it.  A block whose
 * gradients are final early — rlx_adam_split_blocks: every existing float4 of its four runs lies inside one of the float
 * ranges [lo, hi) of ranges_host (n_ranges pairs), and it owns none of the <= 3 elements behind the last float4 — can be
 * stepped by rlx_adam_tf1_step_early (`workgroups` workgroups, each looping over early blocks; no ticket; no target mix)
 * or by riders of the convolution weight-gradient launch (rlx_conv_dw_multi_adam) while the rest of the backward pass still
 * runs.  rlx_adam_tf1_step_late then runs the late blocks (never none: the split keeps one), and the workgroup that finishes
 * last sums the partials of ALL blocks in index order, writes the norm, advances the beta powers and adds the signal sums.
 * Weights, slots, state, norm and signal sums are bit-identical to rlx_adam_tf1_step's.  `partials` ([blocks] floats) must
 * stay untouched between the early and the late launch; early / late are device arrays (n_early + n_late == blocks), the
 * *_host outputs of rlx_adam_split_blocks have room for `blocks` entries each. */
typedef struct rlx_adam_split_desc {
    float *weights;
    const float *grads;
    float *m, *v;
    long long n;
    float learning_rate, beta1, beta2, epsilon, grad_scale;
    float *state;
    float *partials;
    int blocks;
    const int *early, *late;
    int n_early, n_late;
} rlx_adam_split_desc;
int rlx_adam_step_blocks(long long n, long long workspace_floats, int *blocks_host);
int rlx_adam_split_blocks(long long n, int blocks, const long long *ranges_host, int n_ranges, int *early_host,
                          int *n_early_host, int *late_host, int *n_late_host);
int rlx_adam_tf1_step_early(const rlx_adam_split_desc *desc_host, int workgroups, void *stream);
int rlx_adam_tf1_step_late(const rlx_adam_split_desc *desc_host, float *norm_out, const float *acc_src, float *acc_dst,
                           int n_acc, unsigned int *ticket, void *stream);
int rlx_mix_weights(float *target, const float *online, long long n, double rate,
                    void *stream);   /* architectures/tensorflow_components/architecture.py:598-607 */
int rlx_global_norm(const float *x, long long n, float *norm_out, float *workspace,
                    long long workspace_floats, void *stream);      /* tf.global_norm, architecture.py:194 */

/* tf.clip_by_global_norm (architectures/tensorflow_components/architecture.py:196-200, clip method
 * ClipByGlobalNorm): grads *= clip_norm * min(1 / global_norm, 1 / clip_norm), in place; global_norm is
 * the device scalar rlx_global_norm wrote.  min is TF's (y < x) ? y : x.  Pinned (tests/test_glue_kernels.py):
 * global_norm < clip_norm: the scale is clip_norm * (1 / clip_norm), which is 1 up to two roundings (exactly 1 for 40, 10,
 * 0.5 and every power of two); global_norm == 0: 1 / 0 = inf loses the min, the scale is the same; global_norm NaN: every
 * gradient becomes NaN (the reference's behaviour, and oracle/agents.py:205-210's); global_norm inf: the scale is 0. */
int rlx_clip_by_global_norm(float *grads, long long n, const float *global_norm, float clip_norm,
                            void *stream);
/* tf.clip_by_value(grad, -clip_value, clip_value) on every gradient (architecture.py:241-245, clip method
 * ClipByValue): an element-wise clamp of the flat gradient buffer, in place; a NaN stays a NaN. */
int rlx_clip_by_value(float *grads, long long n, float clip_value, void *stream);

/* ------------------------------------ continuous-control agents (DDPG / TD3 / SAC) -- */
/* dst[r][c] = scale * src[r][c]: concat / slice / negate / DDPGActorHead output_scale
 * (general_network.py:270-277, heads/ddpg_actor_head.py:48-56). */
int rlx_copy_2d(const float *src, long long src_ld, float *dst, long long dst_ld, int rows, int cols,
                float scale, void *stream);
int rlx_exp_rows(const float *log_std, float *out, int batch, int action_dim,
                 void *stream);                /* policy_std = tile(exp(policy_logstd)), heads/ppo_head.py:139 */
int rlx_axpby(float *out, float a, const float *x, float b, const float *y, long long n,
              void *stream);                   /* out = a*x + b*y (y may be NULL: then out = a*x whatever b is; out may be
                                                * x or y: in place); heads/sac_q_head.py:63-67 */
/* out_min = min(q1,q2); grad_i = grad_scale * d sum(min)/d q_i (tf.minimum: ties go to q1).  A NaN of either side is
 * the minimum, as in np.minimum (q1's where q1 is one), and takes the gradient.
 * heads/sac_q_head.py:84-88, heads/td3_v_head.py:54-58 */
int rlx_min_pair(const float *q1, const float *q2, float *out_min, float *grad1, float *grad2,
                 float grad_scale, int n, void *stream);
/* rlx_min_pair + rlx_sac_value_targets in one launch (soft_actor_critic_agent.py:198-200,216-217,244):
 * out_min = min(q1, q2), value_targets = out_min - sampled_logprob, grad_i = grad_scale * d sum(min) / d q_i. */
int rlx_sac_min_targets(const float *q1, const float *q2, const float *sampled_logprob, float grad_scale, int n,
                        float *out_min, float *value_targets, float *grad1, float *grad2, void *stream);
int rlx_select_rows(const unsigned char *mask, const void *if_set, const void *if_clear, void *out,
                    int n, long long row_bytes, void *stream);   /* out[r] = mask[r] ? if_set[r] : if_clear[r] */
/* SACPolicyHead (heads/sac_head.py:60-97): mu_logsig [batch, 2*action_dim] is the head's dense
 * output; standard_normals [batch, action_dim] are host draws (fp64).  Any output may be NULL. */
int rlx_sac_policy_head(const float *mu_logsig, long long ld, const double *standard_normals, int batch,
                        int action_dim, float *out_mean, float *out_log_std, float *out_raw_actions,
                        float *out_actions, float *out_logprob, void *stream);
/* d/d mu_logsig of  logprob_mean_weight * mean_b(logprob_b) + action_weight_scale *
 * sum(action_weights * actions)  (weighted_gradients[5] / [3], soft_actor_critic_agent.py:210-229);
 * accumulate != 0 adds onto d_mu_logsig (the passes of one update share the deterministic torso
 * output, so their head gradients can be summed before ONE backward pass through the torso). */
int rlx_sac_policy_head_backward(const float *mu_logsig, long long ld, const double *standard_normals,
                                 int batch, int action_dim, float logprob_mean_weight,
                                 const float *action_weights, float action_weight_scale,
                                 float *d_mu_logsig, long long ld_grad, int accumulate, void *stream);

/* -------------------------------------------------------- exploration policies -- */
int rlx_categorical_sample(const float *probs, long long ld, const double *uniforms, int n_env,
                           int n_actions, int *actions, void *stream); /* exploration_policies/categorical.py:45-48 */
/* rlx_softmax (tf.nn.softmax of the policy head's logits, heads/ppo_head.py:108) + rlx_categorical_sample on the
 * probabilities it produces, as ONE launch — the acting step of discrete Clipped PPO.  probs_out may be NULL. */
int rlx_softmax_categorical_sample(const float *logits, long long ld, const double *uniforms, int n_env,
                                   int n_actions, float *probs_out, long long ld_out, int *actions, void *stream);
int rlx_argmax_rows(const float *values, long long ld, int n_rows, int n_cols, int *out,
                    void *stream);            /* np.argmax per row: exploration_policies/categorical.py:50-52 */
int rlx_egreedy(const float *q_values, long long ld, const double *explore_uniforms,
                const int *random_actions, const double *tie_break_uniforms, double epsilon,
                int n_env, int n_actions, int *actions, void *stream); /* exploration_policies/e_greedy.py:84-101 */
int rlx_gaussian_action(const float *mean, const float *std_per_dim, const float *std_per_sample,
                        const double *standard_normals, const float *action_low,
                        const float *action_high, int n_env, int action_dim, float *actions,
                        void *stream);                              /* exploration_policies/additive_noise.py:75-111 */

/* ------------------------------------------------------------- Quantile-Regression DQN -- */
/* QuantileRegressionDQNAgent.learn_from_batch + the QuantileRegressionQHead loss (agents/qr_dqn_agent.py:99-137,
 * heads/quantile_regression_q_head.py:55-74) in ONE launch, one workgroup per batch row.  theta / theta_next_target:
 * the online / target head outputs [batch][A*N] (column a*N + j = atom j of action a).  Per row: a* = argmax of the
 * target's fp64 atom means (first maximum), T_j = fp32(r + (1 - done) * discount * theta'[a*, j]) in fp64, the
 * midpoints tau[i] = fp32(tau_hat[argsort(theta[a_b])[i]]) (the reference's indexing, stable ties), then
 * loss = sum_b sum_i sum_j |tau_i - 1{e_ij < 0}| * huber_kappa(e_ij) / N with e_ij = T_j - theta_i (a SUM over the batch),
 * dtheta[b][a_b*N + i] = -grad_scale / N * sum_j |tau_i - 1{e_ij < 0}| * sign(e_ij) * min(|e_ij|, kappa), zero elsewhere.
 * row_partials: [batch] floats of workspace; ticket: one zero-initialised word (left at zero); the loss is summed in a
 * fixed order (bit-identical run to run).  status |= 1 for an action outside [0, A).  targets_out / tau_out [batch][N]
 * and target_actions_out [batch] are optional (null).  N <= 256, A <= 18, batch <= 256. */
int rlx_qr_dqn_head_loss(const float *theta, long long ld_theta, const float *theta_next_target, long long ld_next,
                         const int *actions, const float *rewards, const unsigned char *game_overs, double discount,
                         float kappa, int n_atoms, int n_actions, int batch, float grad_scale, float *dtheta,
                         long long ld_dtheta, float *row_partials, unsigned int *ticket, float *loss_scalar,
                         int *status, float *targets_out, float *tau_out, int *target_actions_out, void *stream);
/* get_q_values (qr_dqn_agent.py:75-76: fp64 means of the atoms, summed in atom order) + rlx_egreedy's choice on them
 * with the isclose tie test in fp64 (e_greedy.py:84-101).  quantiles: [n_env][ld], ld >= A*N; the draws as rlx_egreedy
 * takes them; q_out [n_env][A] fp64 is optional (null). */
int rlx_quantile_egreedy(const float *quantiles, long long ld, int n_atoms, const double *explore_uniforms,
                         const int *random_actions, const double *tie_break_uniforms, double epsilon, int n_env,
                         int n_actions, double *q_out, int *actions, void *stream);

/* ------------------------------------------------------------------ Categorical DQN (C51) -- */
/* CategoricalDQNAgent.learn_from_batch + the CategoricalQHead loss (agents/categorical_dqn_agent.py:104-167,
 * heads/categorical_q_head.py:42-58) in ONE launch, one workgroup per batch row.  logits / logits_next_target: the online
 * head's Dense output on s / the target's on s', [batch][A*N] (column a*N + j = atom j of action a); z: the support,
 * [N] fp64 (np.linspace(v_min, v_max, N) from the host).  Softmax over the atoms: mx = max, e_j = fp32(exp((double)(x_j -
 * mx))), s = the e_j summed in atom order (fp32), p_j = e_j / s.  Per row: a* = argmax of the target's fp64 expectations
 * sum_j p'_j z_j (atom order, first maximum); the projection for j = 0 .. N-1 in this order, fp64:
 * tz = fmax(fmin(r + (1 - done) * discount * z_j, z_{N-1}), z_0), bj = (tz - z_0) / (z_1 - z_0), l = floor(bj),
 * u = ceil(bj), m[l] += p'[a*, j] (u - bj), m[u] += p'[a*, j] (bj - l), m rounded to fp32 once (an integer bj drops
 * that atom's mass, as the reference does; u == N, which rounding can produce at v_max on some supports and on which the
 * reference raises, is left out).  Labels: m for the taken action, the online softmax itself for the others;
 * loss = sum_b sum_a sum_j label_j (log s - (x_j - mx)) (a SUM over batch and actions);
 * dlogits[b][a_b*N + j] = grad_scale * (p_j - m_j), zero elsewhere.  per_errors [batch] fp64 (optional): the taken action's
 * cross entropy (0 for an invalid action).  row_partials: [batch] floats of workspace; ticket: one zero-initialised word
 * (left at zero); the loss is summed in a fixed order (bit-identical run to run).  status |= 1 for an action outside
 * [0, A).  m_out [batch][N], target_actions_out [batch] and action_losses_out [batch][A] are optional (null).
 * 2 <= N <= 256, A <= 18, batch <= 256. */
int rlx_c51_head_loss(const float *logits, long long ld_logits, const float *logits_next_target, long long ld_next,
                      const double *z, const int *actions, const float *rewards, const unsigned char *game_overs,
                      double discount, int n_atoms, int n_actions, int batch, float grad_scale, float *dlogits,
                      long long ld_dlogits, double *per_errors, float *row_partials, unsigned int *ticket,
                      float *loss_scalar, int *status, float *m_out, int *target_actions_out, float *action_losses_out,
                      void *stream);
/* distribution_prediction_to_q_values (categorical_dqn_agent.py:86-87: fp64 expectations of the softmax over z, summed
 * in atom order) + rlx_egreedy's choice on them with the isclose tie test in fp64 (e_greedy.py:84-101).  logits:
 * [n_env][ld], ld >= A*N; the draws as rlx_egreedy takes them; q_out [n_env][A] fp64 is optional (null).
 * 2 <= N <= 256, A <= 18. */
int rlx_categorical_egreedy(const float *logits, long long ld, const double *z, int n_atoms,
                            const double *explore_uniforms, const int *random_actions,
                            const double *tie_break_uniforms, double epsilon, int n_env, int n_actions, double *q_out,
                            int *actions, void *stream);

/* ---------------------------------------------------------------------------- Rainbow DQN -- */
/* RainbowDQNAgent.learn_from_batch + the RainbowQHead's loss and gradient (agents/rainbow_dqn_agent.py:88-137,
 * heads/rainbow_q_head.py:43-70) in ONE launch, one workgroup per batch row.  The head has two Dense outputs: the
 * state-value stream v [batch][N] and the action-advantage stream x [batch][A*N] (column a*N + j = atom j of action a),
 * each with its own leading dimension, on three passes: the online network on s (v, x), the target network on s'
 * (*_next_target) and the online network on s' (*_next_online).
 * Merge, fp32, per atom j, in rlx_dueling_combine's order (csrc/dfp_merge.hpp): s = 0.f, then += x[a][j] for a
 * ascending; mean = s / (float)A; y[a][j] = v[j] + (x[a][j] - mean).  (The reference framework's own reduce_mean order is not pinned.)
 * Softmax over the atoms of every action and the fp64 expectations are rlx_c51_head_loss's.  Per row: a* = the first
 * maximum of the ONLINE network's expectations on s' (Double DQN); the projection of the TARGET network's distribution
 * on s' at a*, for j = 0 .. N-1 in this order, fp64: tz = fmax(fmin(R + (boot * discount_n) * z_j, z_{N-1}), z_0) with
 * R = n_step_returns[b], boot = bootstrap[b] (should_bootstrap_next_state; game_over is not read) and discount_n the
 * host's discount ** n_step; bj, l, u, m and the dropped mass as in rlx_c51_head_loss; m rounded to fp32 once.
 * Labels: m for the taken action, the online softmax itself for the others; loss = the sum over batch and actions of the
 * softmax cross entropies, summed in a fixed order (row_partials: [batch] floats of workspace; ticket: one
 * zero-initialised word, left at zero).  dy[b][a_b][j] = grad_scale * (p_j - m_j), exactly 0 on the other actions; dy goes
 * back through the merge in rlx_dueling_combine_backward's arithmetic per atom: s = 0.f, then += dy[a][j] for a ascending;
 * dv[b][j] = s; dx[b][a*N + j] = dy[a][j] - s / (float)A.  per_errors [batch] fp64 (optional): the taken action's cross
 * entropy (0 for an invalid action), the row's new priority; importance weights are not an input (the head's loss_type
 * is empty).  status |= 1 for an action outside [0, A): that row gets a zero gradient.  m_out [batch][N],
 * target_actions_out [batch], action_losses_out [batch][A], merged_logits_out [batch][A*N] (y of the online network on
 * s) and dlogits_out [batch][A*N] (dy) are optional (null).  2 <= N <= 256, A <= 18, batch <= 256. */
int rlx_rainbow_head_loss(const float *v, long long ld_v, const float *x, long long ld_x, const float *v_next_target,
                          long long ld_v_next_target, const float *x_next_target, long long ld_x_next_target,
                          const float *v_next_online, long long ld_v_next_online, const float *x_next_online,
                          long long ld_x_next_online, const double *z, const int *actions,
                          const double *n_step_returns, const unsigned char *bootstrap, double discount_n, int n_atoms,
                          int n_actions, int batch, float grad_scale, float *dv, long long ld_dv, float *dx,
                          long long ld_dx, double *per_errors, float *row_partials, unsigned int *ticket,
                          float *loss_scalar, int *status, float *m_out, int *target_actions_out,
                          float *action_losses_out, float *merged_logits_out, float *dlogits_out, void *stream);
/* The head's acting reductions: the merge above, then what rlx_categorical_egreedy / rlx_categorical_argmax do on the
 * merged logits (one body, csrc/categorical_head.hpp): softmax, fp64 expectations, the epsilon-greedy choice with the
 * fp64 isclose tie test, or the first maximum.  v: [n_env][ld_v], x: [n_env][ld_x]; the draws as rlx_egreedy takes them;
 * q_out [n_env][A] fp64 is optional (null).  2 <= N <= 256, A <= 18. */
int rlx_rainbow_egreedy(const float *v, long long ld_v, const float *x, long long ld_x, const double *z, int n_atoms,
                        const double *explore_uniforms, const int *random_actions, const double *tie_break_uniforms,
                        double epsilon, int n_env, int n_actions, double *q_out, int *actions, void *stream);
int rlx_rainbow_argmax(const float *v, long long ld_v, const float *x, long long ld_x, const double *z, int n_atoms,
                       int n_env, int n_actions, double *q_out, int *actions, void *stream);
/* A finished episode's way into an n-step agent's replay (Episode.update_transitions_rewards_and_bootstrap_data,
 * core_types.py:803-820, and the store loop of agents/agent.py:571-574) in ONE launch.  Source: env's staged episode of
 * `length` = T rows, row k of columns laid out [n_env][stage_len] (observations obs_dim floats, actions action_words
 * 32-bit words per row).  Destination: T consecutive rows of a struct-of-arrays ring starting at dst0, modulo ring_rows.
 * With c = min(n_step, T), row k gets obs, action, reward and game_over of step k unchanged;
 * n_step_discounted_rewards = what rlx_episode_nstep_returns gives for the same rewards (one body,
 * csrc/episode_returns.hpp: bit-identical); if k + c < T: next_obs = obs of step k + c and
 * should_bootstrap_next_state = 1, else next_obs = next_obs of step T - 1 and the flag is 0. */
int rlx_nstep_episode_store(const float *staged_obs, const float *staged_next_obs, const int *staged_actions,
                            const float *staged_rewards, const unsigned char *staged_game_overs, int env, int n_env,
                            int stage_len, int length, int n_step, double discount, int obs_dim, int action_words,
                            float *obs, float *next_obs, int *actions, float *rewards, unsigned char *game_overs,
                            double *n_step_discounted_rewards, unsigned char *should_bootstrap_next_state,
                            long long dst0, long long ring_rows, void *stream);

/* ------------------------------------------------------------ Direct Future Prediction (DFP) -- */
/* The MeasurementsPredictionHead (heads/measurements_prediction_head.py:39-62) works on two Dense outputs: expectation
 * [rows][K] and action_stream [rows][A*K] (column a*K + k), K = n_steps * n_measurements (step s, measurement m is column
 * s*M + m).  The merge, fp32, for every column k (csrc/dfp_merge.hpp): s = 0.f, then plus X[a][k] for a = 0 .. A-1 in
 * this order; mean = s / (float)A; y[a][k] = E[k] + (X[a][k] - mean) — rlx_dueling_combine's order, bit-identical to it
 * for K = 1.
 *
 * rlx_dfp_head_loss: DFPAgent.learn_from_batch (agents/dfp_agent.py:150-167) + the head's loss in ONE launch, one
 * workgroup per batch row.  future_measurements [batch][K] fp32 may hold NaN.  The targets equal the prediction y
 * everywhere but in the taken action's row, which is future_measurements with every NaN replaced by the prediction.  On
 * the taken action's non-NaN entries d = target - y; loss = (sum over b in row order of (sum over k in index order of
 * d * d)) / (float)batch; g[k] = ((grad_scale * 2.f) * (y - target)) / (float)batch there and 0 elsewhere.
 * d_expectation[b][k] = g[k]; d_action_stream[b][a][k] = g[k] * ((a == a_b ? 1.f : 0.f) - 1.f / (float)A) (0 where g is
 * not formed).  row_partials: [batch] floats of workspace; ticket: one zero-initialised word (left at zero); the loss
 * does not depend on the order in which the workgroups finish.  status |= 1 for an action outside [0, A): that row adds no
 * term and gets a zero gradient.  y_out and targets_out, [batch][A*K], are optional (null).
 * 1 <= A <= 18, 1 <= K <= 64, batch <= 256. */
int rlx_dfp_head_loss(const float *expectation, long long ld_e, const float *action_stream, long long ld_x,
                      const int *actions, const float *future_measurements, int n_actions, int n_columns, int batch,
                      float grad_scale, float *d_expectation, long long ld_de, float *d_action_stream, long long ld_dx,
                      float *row_partials, unsigned int *ticket, float *loss_scalar, int *status, float *y_out,
                      float *targets_out, void *stream);
/* The acting step of DFPAgent.choose_action (dfp_agent.py:169-199) for n_env rows: the merge, then the fp64 score of every
 * action, v[a] = sum_{j = 0 .. W-1} (sum_{m = 0 .. M-1} (double)y[a][(S - W + j)*M + m] * goal[m]) * weights[j] (both sums
 * from 0.0 in index order: the last W steps), then rlx_categorical_egreedy's choice on the scores (the same code).  goal
 * [M] and weights [W] are fp64 device arrays, W <= S; the draws as rlx_egreedy takes them; q_out [n_env][A] fp64 is
 * optional (null).  A <= 18, S * M <= 64. */
int rlx_dfp_egreedy(const float *expectation, long long ld_e, const float *action_stream, long long ld_x,
                    const double *goal, const double *weights, int n_steps, int n_measurements, int n_weights,
                    const double *explore_uniforms, const int *random_actions, const double *tie_break_uniforms,
                    double epsilon, int n_env, int n_actions, double *q_out, int *actions, void *stream);
/* The same scores, np.argmax (the first maximum, no draws): ParameterNoise acting (parameter_noise.py:62-68). */
int rlx_dfp_argmax(const float *expectation, long long ld_e, const float *action_stream, long long ld_x,
                   const double *goal, const double *weights, int n_steps, int n_measurements, int n_weights, int n_env,
                   int n_actions, double *q_out, int *actions, void *stream);
/* DFPAgent._update_measurements_targets (dfp_agent.py:235-255) for ONE completed episode stored time-major (the addressing
 * of rlx_episode_nstep_returns: row of step k = ((first_step + k) mod ring_steps) * n_env + env).  measurements: the fp64
 * column [rows][M] of the STATE's measurements; future_measurements: the fp32 column [rows][S*M]; scale: [M] fp64 on the
 * device.  For transition i and step s, off = i + 2^s: off < length -> out[i][s][m] = (float)(scale[m] * (meas[off][m] -
 * meas[i][m])), fp64 rounded once; off >= length -> a quiet NaN (last_step_mode 0, HandlingTargetsAfterEpisodeEnd.NAN) or
 * off = length - 1, the LAST transition's state (last_step_mode 1, LastStep).  One thread per (i, s); S <= 8, M <= 8. */
int rlx_dfp_future_measurements(const double *measurements, float *future_measurements, const double *scale,
                                long long first_step, int length, int env, int n_env, long long ring_steps, int n_steps,
                                int n_measurements, int last_step_mode, void *stream);
/* use_accumulated_reward_as_measurement (agents/agent.py:920-925 injects the running sum of shaped rewards into the next
 * state BEFORE :958 adds the step's reward) for n_env envs after one vector step.  accumulated [n_env] fp64: the sum;
 * measurements [n_env][M] fp64 (and measurements32, its fp32 twin for the network, optional): the CURRENT state's
 * measurements, whose column `column` is the accumulated reward.  Per env: state_measurements_out[e] (optional, [n_env][M])
 * = measurements[e] (the state the step was taken in: the replay's column); measurements[e][column] = game_over ? 0 :
 * accumulated[e]; accumulated[e] = game_over ? 0 : accumulated[e] + rewards[e].  So the state after step t carries the
 * rewards of steps 1 .. t-1, and the first two states of an episode carry 0.  M <= 8. */
int rlx_dfp_accumulated_reward_step(const float *rewards, const unsigned char *game_overs, double *accumulated,
                                    double *measurements, float *measurements32, double *state_measurements_out, int n_env,
                                    int n_measurements, int column, void *stream);

/* ------------------------------------------------ synthetic vector environment -- */
/* Device-resident stand-in for Environment.step (environments/environment.py:276-327) on the
 * BASELINE workloads: fixed-length episodes, Philox4x32-10 observations/rewards keyed by
 * (seed, env id) and counted by (episode, step).  kind 0 = uint8 image frames, 1 = fp32 vectors.
 * episode/step: int32[n_env] state.  reset_obs[e] is written only where game_over[e] is set. */
int rlx_synth_env_reset(int kind, void *obs, int *episode, int *step, int n_env, int obs_elems,
                        unsigned int seed, unsigned int env_id0, void *stream);
int rlx_synth_env_step(int kind, void *next_obs, void *reset_obs, float *reward,
                       unsigned char *game_over, int *episode, int *step, int n_env, int obs_elems,
                       int episode_len, unsigned int seed, unsigned int env_id0, void *stream);

/* the same with a time limit per env (device int32[n_env]): envs whose episodes end on different steps, the
 * case a real simulator front end produces (environment.py:276-327 episode bookkeeping is per env) */
int rlx_synth_env_step_lengths(int kind, void *next_obs, void *reset_obs, float *reward,
                               unsigned char *game_over, int *episode, int *step, int n_env, int obs_elems,
                               const int *episode_len_per_env, unsigned int seed, unsigned int env_id0,
                               void *stream);

/* Standard normals from a counter-based generator, for the agents' noise_source = "device" mode (no reference
 * counterpart: the reference draws this noise with np.random.normal, td3_agent.py:162, additive_noise.py:106, and in
 * SAC's TF sampling op).  out[e][s][i] (n_events x n_streams x n doubles) = scale * z, z the i-th value of stream
 * stream0 + s at event events[e]: Philox4x32-10 with key (seed, rank) and counter (i / 2, stream, event low word,
 * event high word ^ a fixed tag that keeps it apart from the synthetic environment's streams), one Box-Muller pair
 * per call computed with correctly rounded IEEE operations only (csrc/noise.hip; bit-exact numpy twin:
 * tests/noise_ref.py).  Streams 0..4: 0 TD3 smoothing noise, 1-3 SAC's three per-update draws, 4 acting.  The event
 * indices are READ FROM DEVICE MEMORY (events: n_events int64), so a captured graph replayed after they were
 * rewritten draws new values. */
int rlx_normal_fill(double *out, const long long *events, int n_events, int stream0, int n_streams, int n,
                    unsigned int seed, unsigned int rank, double scale, void *stream);

/* ------------------------------------------------- factorised NoisyNet dense layers -- */
/* ParameterNoise (exploration_policies/parameter_noise.py) swaps a network's dense layers for the factorised noisy
 * layer of architectures/tensorflow_components/layers.py:196-257:
 *   f(v) = sign(v) sqrt(|v|);  W = weight_mean + weight_stddev * (f(e_in) outer f(e_out));
 *   b = bias_mean + bias_stddev * f(e_b);  y = act(x W + b), e_* standard normals drawn anew for every forward pass.
 * A layer's noise of one pass is ONE vector `noise` of K + 2 N floats: [f(e_in) (K) | f(e_out) (N) | f(e_b) (N)].
 *
 * rlx_noisy_sample fills it for up to RLX_NOISY_MAX_LAYERS layers in one launch (one workgroup per layer) from rlx_normal_fill's generator
 * (csrc/noise.hip), f applied in fp64 and the result rounded once to fp32 (f64, optional: the fp64 values).  Stream
 * assignment of that generator: 0..4 belong to rlx_normal_fill (above); layer L's vectors of pass P are the streams
 *   5 + 3 * (RLX_NOISY_PASSES * L + P) + {0: e_in, 1: e_out, 2: e_b},
 * value i of a vector being value i of its stream, at the event index held in counters[RLX_NOISY_PASSES * L + P]
 * (device int64), under the key (seed, rank).  The launch READS the counter from device memory and then advances it
 * by one, so every pass — also every replay of a captured graph — draws new values, and a draw is a function of
 * (seed, rank, layer, pass, counter) alone.  Passes: 0 acting, 1 the online network on s (the pass the loss is taken
 * on), 2 the target network on s', 3 the online network on s' (Double DQN's selection).
 * These entry points (and rlx_quantile_argmax / rlx_categorical_argmax below) were ADDED under ABI version 11: no
 * existing signature or structure changed, which is what rlx_abi_version counts, and the loader refuses a library that
 * does not export a symbol this header declares. */
#define RLX_NOISY_PASSES 4
#define RLX_NOISY_MAX_LAYERS 8
typedef struct rlx_noisy_layer {
    float *f;      /* [K + 2 N] */
    double *f64;   /* [K + 2 N] or NULL */
    int K, N;
    int layer;     /* the layer's index in its network (selects streams and counters) */
} rlx_noisy_layer;
int rlx_noisy_sample(const rlx_noisy_layer *layers_host, int n_layers, long long *counters, int pass,
                     unsigned int seed, unsigned int rank, void *stream);
/* y [M][ldy] = act(x Wm + ((x * f_in) Ws) * f_out + bias_mean + bias_stddev * f_b): two fp32 MFMA accumulators per
 * output tile, each weight matrix ([K][N] row-major) read once per 32 rows, the noisy matrix never formed (csrc/noisy_dense.hip).
 * K is split over workgroups by the shape alone; workspace: rlx_noisy_dense_workspace_floats(M, K, N) floats (the larger
 * of the forward and the input-gradient need).  Sums are bit-identical run to run. */
int rlx_noisy_dense_workspace_floats(int M, int K, int N, long long *floats_host);
int rlx_noisy_dense_forward(const float *x, long long ldx, const float *weight_mean, const float *weight_stddev,
                            const float *bias_mean, const float *bias_stddev, const float *noise, float *y,
                            long long ldy, int M, int K, int N, int activation, float *workspace,
                            long long workspace_floats, void *stream);
/* From dz [M][lddz] = dL/d(pre-activation) and the noise of the forward pass whose output the loss was taken on:
 * d_weight_mean = x^T dz, d_weight_stddev[k][n] = d_weight_mean[k][n] f_in[k] f_out[n], d_bias_mean = column sums of dz,
 * d_bias_stddev = d_bias_mean * f_b (one launch; all four or, with d_weight_mean NULL, none), and (dx not NULL)
 * dx [M][lddx] = (dz Wm^T + ((dz * f_out) Ws^T) * f_in) * act'(x) with the LOWER layer's activation lower_activation
 * (x is that layer's output). */
int rlx_noisy_dense_backward(const float *x, long long ldx, const float *weight_mean, const float *weight_stddev,
                             const float *dz, long long lddz, const float *noise, float *d_weight_mean,
                             float *d_weight_stddev, float *d_bias_mean, float *d_bias_stddev, float *dx,
                             long long lddx, int M, int K, int N, int lower_activation, float *workspace,
                             long long workspace_floats, void *stream);
/* ParameterNoise acting on the distributional heads (parameter_noise.py:62-68: np.argmax, the FIRST maximum, no draws)
 * over the fp64 action values of rlx_quantile_egreedy / rlx_categorical_egreedy; q_out [n_env][A] fp64 is optional.
 * (fp32 Q values: rlx_argmax_rows.) */
int rlx_quantile_argmax(const float *quantiles, long long ld, int n_atoms, int n_env, int n_actions, double *q_out,
                        int *actions, void *stream);
int rlx_categorical_argmax(const float *logits, long long ld, const double *z, int n_atoms, int n_env, int n_actions,
                           double *q_out, int *actions, void *stream);

/* -------------------------------------------------------------------- Bootstrapped DQN -- */
/* BootstrappedDQNAgent.learn_from_batch + the K QHead losses and their sum (agents/bootstrapped_dqn_agent.py:57-86,
 * heads/q_head.py, head.py:172-181) in ONE launch, one workgroup per batch row.  q_online / q_next_target /
 * q_next_online: the head layer's outputs on s (online), s' (target) and s' (online) [batch][K*A], column h*A + a =
 * action a of head h.  masks [batch]: bit h set = the transition trains head h.  Per (row, head) with its bit set: the
 * arithmetic of rlx_dqn_head_loss for that head alone with a selector and no importance weights (a* = first maximum of
 * the online s' values, fp64 TD target rounded to fp32 once, MSE or Huber, dq = grad_scale * l' / batch at the taken
 * action); with every bit set head h's slice of dq and head_losses[h] equal that call's outputs on columns
 * [h*A, (h+1)*A) bit for bit.  A cleared bit: dq = 0 and a zero loss term, the mean's denominator stays batch.
 * loss_scalar = the K head losses added in head order; every batch sum is taken in a fixed tree (bit-identical run to
 * run, no float atomics).  partials: [K*batch] floats of workspace; ticket: one zero-initialised word (left at zero).
 * status |= 1 for an action outside [0, A) (the row then has a zero gradient).  Optional outputs (null):
 * head_losses [K]; td_targets [batch][K] (the fp32 target at the taken action; the online prediction where the bit is
 * cleared); target_actions [batch][K] (a*, whatever the bit).  K <= 32, A <= 18, batch <= 256.
 * Added under ABI version 11, like the entry points above. */
int rlx_bootstrapped_dqn_head_loss(const float *q_online, long long ld_q, const float *q_next_target,
                                   const float *q_next_online, long long ld_next, const int *actions,
                                   const float *rewards, const unsigned char *game_overs, const uint32_t *masks,
                                   double discount, int batch, int n_heads, int n_actions, int huber, float grad_scale,
                                   float *dq, long long ld_dq, float *partials, unsigned int *ticket, float *loss_scalar,
                                   int *status, float *head_losses, float *td_targets, int *target_actions,
                                   void *stream);
/* Bootstrapped.get_action (exploration_policies/bootstrapped.py:72-85) + rlx_egreedy's choice, one wave per env.
 * q_values [n_env][ld], ld >= K*A.  vote == 0 (TRAIN): the action values are head selected_head[e]'s.  vote != 0: every
 * head votes for its first maximum, the most voted action wins (the lowest index on a tie) and the action values are
 * its one-hot vector; selected_head may then be null.  The draws as rlx_egreedy takes them, with its fp32 isclose tie
 * test.  values_out [n_env][A] (optional): the action values the choice was made on (last_action_values). */
int rlx_bootstrapped_egreedy(const float *q_values, long long ld, int n_heads, const int *selected_head, int vote,
                             const double *explore_uniforms, const int *random_actions,
                             const double *tie_break_uniforms, double epsilon, int n_env, int n_actions,
                             float *values_out, int *actions, void *stream);
/* UCB.get_action (exploration_policies/ucb.py:76-86) + rlx_egreedy's choice, one wave per env, on the same [K*A] rows
 * (K <= 32, A <= 18, ld >= K*A).  Per action a, in fp32, one rounding per operation and the heads in head order:
 * s = q[0][a], s += q[h][a]; mean = s / (float)K; d_h = q[h][a] - mean; acc = d_0 * d_0, acc += d_h * d_h;
 * std = sqrtf(acc / (float)K).  use_std != 0 (TRAIN): values = mean + lamb * std; use_std == 0: values = mean and std is
 * not computed.  values_out [n_env][A]: the action values the choice was made on; std_out [n_env][A] (optional, written
 * only with use_std); the draws and the fp32 isclose tie test as rlx_bootstrapped_egreedy takes them.  An added entry
 * point. */
int rlx_ucb_egreedy(const float *q_values, long long ld, int n_heads, float lamb, int use_std,
                    const double *explore_uniforms, const int *random_actions, const double *tie_break_uniforms,
                    double epsilon, int n_env, int n_actions, float *values_out, float *std_out, int *actions,
                    void *stream);

/* ------------------------------------------------- Normalized Advantage Functions (NAF) -- */
/* The NAFHead (architectures/tensorflow_components/heads/naf_head.py:45-86), NAFAgent's TD targets
 * (agents/naf_agent.py:83-90), the head's loss (head.py:143-186: mean squared error, or Huber with delta 1) and its
 * gradient in ONE launch: one wave per batch row, four rows per workgroup.
 * Inputs, each [batch] rows with its own leading dimension: v (the V layer's output), mu_unscaled [A] (the mu_unscaled
 * layer's ACTIVATED output), l_vector [A(A+1)/2] (column c of the lower-triangular L at i_c = sum_{k<c} (A - k):
 * L[c][c] = exp(l[i_c]), L[r][c] = l[i_c + r - c] for r > c), actions [A], v_next (the target network's V(s'));
 * output_scale [A]; rewards, game_overs [batch].
 * Arithmetic (fp32, every sum in ascending index order, no contraction; tests/naf_ref.py states it operation for
 * operation): mu = mu_unscaled * output_scale, d = u - mu, y_c = sum_{r>=c} L[r][c] d_r, Q = V - 0.5 sum_c y_c^2; the
 * TD target r + (1 - game_over) * discount * v_next in fp64, rounded to fp32 once (as rlx_dqn_head_loss does);
 * g = grad_scale * l'(Q - target) / batch; dv = g, dmu_unscaled_c = g (L y)_c output_scale_c (the gradient w.r.t. the
 * layer's activated output), dl_vector: dL[r][c] = -g y_c d_r, times L[c][c] on the diagonal.
 * loss_scalar = mean of the row terms, summed in a fixed tree by the workgroup that draws the last ticket (bit-identical
 * run to run, no float atomics).  partials: [batch] floats of workspace; ticket: one zero-initialised word (left at
 * zero).  Optional outputs (null): td_targets_out, q_out, adv_out [batch].  1 <= A <= 32, 1 <= batch <= 256.
 * Added under ABI version 11, like the entry points above. */
int rlx_naf_head_loss(const float *v, long long ld_v, const float *mu_unscaled, long long ld_mu, const float *l_vector,
                      long long ld_l, const float *output_scale, const float *actions, long long ld_act,
                      const float *v_next, long long ld_vnext, const float *rewards, const unsigned char *game_overs,
                      double discount, int batch, int action_dim, int huber, float grad_scale, float *dv,
                      long long ld_dv, float *dmu_unscaled, long long ld_dmu, float *dl_vector, long long ld_dl,
                      float *partials, unsigned int *ticket, float *loss_scalar, float *td_targets_out, float *q_out,
                      float *adv_out, void *stream);
/* The head's forward pass alone, for acting and for the Q / L / Advantage / Action / V signals
 * (agents/naf_agent.py:101-131).  actions null: u = mu, so Adv = 0 and Q = V.  Outputs (each optional, at least one):
 * mu_out [batch][A], q_out [batch], adv_out [batch], l_out [batch][A][A] (zeros above the diagonal).  1 <= A <= 32. */
int rlx_naf_head_forward(const float *v, long long ld_v, const float *mu_unscaled, long long ld_mu,
                         const float *l_vector, long long ld_l, const float *output_scale, const float *actions,
                         long long ld_act, int batch, int action_dim, float *mu_out, float *q_out, float *adv_out,
                         float *l_out, void *stream);

/* ------------------------------------ Persistent Advantage Learning / Mixed Monte Carlo -- */
/* PALAgent.learn_from_batch (agents/pal_agent.py:70-111) or MixedMonteCarloAgent.learn_from_batch
 * (agents/mmc_agent.py:57-83), the QHead loss (MSE / Huber) on their targets and its gradient w.r.t. Q_online in ONE
 * launch, modelled on rlx_dqn_head_loss: one workgroup, one row per thread, batch <= 1024, the batch mean in the same
 * fixed-order tree (no float atomics).  q_online and q_target_cur (the target network on s) [batch][ld_q];
 * q_next_target and q_next_selector (the target and the online network on s') [batch][ld_next]; total_returns [batch]
 * fp64: the rows' n_step_discounted_rewards.  Per row with taken action a: sel = first maximum of q_next_selector,
 * y = r + (1 - game_over) * discount * q_next_target[sel] in fp64 (the Double-DQN target), then
 *   q_target_cur given (PAL): T = fp32(y) - fp32(pal_alpha) * adv in fp32, adv = max q_target_cur - q_target_cur[a], or
 *       with persistent != 0 the smaller of it and max q_next_target - q_next_target[sel];
 *       T = fp32( fp64(fp32(1 - mixing_rate) * T) + mixing_rate * total_return );
 *   q_target_cur NULL (MMC): T = fp32( (1 - mixing_rate) * y + mixing_rate * total_return ), all fp64; pal_alpha and
 *       persistent are ignored.
 * (tests/pal_ref.py states every rounding; they are the reference's under numpy >= 2.)  With pal_alpha = 0 and
 * mixing_rate = 0 dq, td_targets and loss_scalar equal rlx_dqn_head_loss's with that selector and no importance weights,
 * bit for bit.  dq[b][a_b] = grad_scale * l'(Q - T) / batch, zero elsewhere.  status |= 1 for an action outside
 * [0, n_actions) (the row then contributes nothing and its dq row is left unwritten, as in rlx_dqn_head_loss).
 * td_targets (Q_online with T at the taken action) and loss_scalar are optional outputs. */
int rlx_mixed_target_head_loss(const float *q_online, long long ld_q, const float *q_target_cur,
                               const float *q_next_target, const float *q_next_selector, long long ld_next,
                               const int *actions, const float *rewards, const unsigned char *game_overs,
                               const double *total_returns, double discount, double pal_alpha, int persistent,
                               double mixing_rate, int batch, int n_actions, int huber, float grad_scale, float *dq,
                               long long ld_dq, float *td_targets, long long ld_targets, float *loss_scalar, int *status,
                               void *stream);

/* ------------------------------------------------------------ CartPole-v0 / -v1 -- */
/* N CartPole environments per GPU: gym 0.12.5's physics (gym/envs/classic_control/cartpole.py `step`, fp64, Euler)
 * behind gym's TimeLimit (max_episode_steps), i.e. what `GymVectorEnvironment(level='CartPole-v0')` steps through
 * rl_coach/environments/gym_environment.py:418-474 (presets/CartPole_DQN.py:46, CartPole_ClippedPPO.py:59).
 * state: fp64[n_env][4] (x, x_dot, theta, theta_dot) — after a step it holds the state the NEXT step starts from
 * (the new episode's first state where game_over is set).  next_obs / reset_obs: fp32[n_env][4] views of the stepped
 * state / the new episode's first state (reset_obs is written only where game_over is set); next_state64 (optional):
 * the stepped state in fp64.  reward = 1.0 per step.  Reset states are Philox draws keyed by (seed, env_id0 + e)
 * and counted by the episode number.  status: bit 0 = a pole angle outside rlx::libm_sin's table domain, bit 1 = an
 * action outside {0, 1}.  next_episode != 0: forced reset mid-episode (every env starts its next episode now). */
int rlx_cartpole_reset(double *state, float *obs, int *episode, int *steps, int n_env, unsigned int seed,
                       unsigned int env_id0, int next_episode, void *stream);
int rlx_cartpole_step(const int *action, double *state, int *episode, int *steps, float *next_obs, float *reset_obs,
                      double *next_state64, float *reward, unsigned char *game_over, int n_env,
                      int max_episode_steps, unsigned int seed, unsigned int env_id0, int *status, void *stream);
/* sin / cos rounded like the host libm's (csrc/libm_sincos.hpp) — exposed for tests/test_cartpole.py */
int rlx_libm_sincos(const double *x, double *sin_out, double *cos_out, int n, int *status, void *stream);


/* ------------------------------------------------------------ fused continuous-control updates (ac_fused.hip) -- */
/* A 2-hidden-layer MLP inside a flat parameter buffer: float offsets of the three layers' kernels ([in][out], TF layout)
 * and biases for tower 0, and the offset between the towers of each layer's parameter group (twin critics). */
typedef struct rlx_mlp3 {
    long long off_w1, off_b1, off_w2, off_b2, off_w3, off_b3;
    long long tower_stride1, tower_stride2, tower_stride3;
    int d_in, h1, h2, d_out;
} rlx_mlp3;
/* One network's flat buffers and optimiser as the fused updates drive them (TF1 Adam of rlx_adam_tf1; mix_rate >= 0: the
 * soft target update w_t <- rate w + (1 - rate) w_t rides in the same pass; norm_out: tf.global_norm of the update's raw
 * gradients or null; ticket: >= 1 zeroed 32-bit word, re-armed by every launch). */
typedef struct rlx_fused_net {
    float *weights, *target_weights, *adam_m, *adam_v, *adam_state, *grads, *norm_out;
    unsigned int *ticket;
    float learning_rate, beta1, beta2, epsilon, grad_scale, mix_rate;
} rlx_fused_net;
/* TD3Agent.learn_from_batch (rl_coach/agents/td3_agent.py:148-209) on MLP actor / twin-critic networks (td3_agent.py:36-68:
 * actor obs -> h1 -> h2 -> tanh head x actor_scale, critic concat(action, obs) -> h1 -> h2 -> Dense(1) per stream; relu).
 * obs / next_obs [batch][obs_dim], actions [batch][act_dim], rewards [batch], game_overs [batch] (as stored),
 * noise [batch][act_dim] fp64: the host's np.random.normal(0, policy_noise) draw BEFORE clipping (:162) or null.
 * Outputs: td_targets [batch], q_min [batch] (output #2 of the target critic), loss [3] = stream losses and their sum,
 * neg_action_grad [batch][act_dim] = -actor_scale * d mean(Q_1) / d a (actor step). */
typedef struct rlx_td3_fused_desc {
    rlx_fused_net actor, critic;
    rlx_mlp3 actor_mlp, critic_mlp;
    const float *obs, *next_obs, *actions, *rewards;
    const unsigned char *game_overs;
    const double *noise;
    const float *action_low, *action_high;
    double noise_clip, discount, clip_low, clip_high;
    int use_non_zero_discount_for_terminal_states, has_clip;
    float actor_scale;
    int batch, obs_dim, act_dim;
    float *workspace; long long workspace_floats;
    float *td_targets, *q_min, *loss, *neg_action_grad;
} rlx_td3_fused_desc;
int rlx_td3_fused_supported(const rlx_td3_fused_desc *desc_host);           /* 1 / 0: shapes only (pointers not read) */
/* Measurement switch (no reference counterpart): workgroup 0 of every chain kernel records s_memtime at its phase
 * boundaries into the LAST 96 int64 words of the workspace. */
int rlx_fused_phase_stamps(int enable);
int rlx_td3_fused_workspace_floats(const rlx_td3_fused_desc *desc_host, long long *floats_host);
/* The critic half (:157-184) as three launches: target chain + online forward, loss + input-gradient chain, weight
 * gradients + Adam (+ norm, + soft target update when critic.mix_rate >= 0).  write_grads != 0: the weight gradients go
 * to critic.grads and no optimiser step is taken (data parallel: the caller all-reduces and steps). */
int rlx_td3_fused_critic_update(const rlx_td3_fused_desc *desc_host, int write_grads, void *stream);
/* The actor half (:186-207) as two launches; uses the critic's CURRENT (already updated) online weights. */
int rlx_td3_fused_actor_update(const rlx_td3_fused_desc *desc_host, int write_grads, void *stream);


/* SoftActorCriticAgent.learn_from_batch (rl_coach/agents/soft_actor_critic_agent.py:168-280) on the Mujoco_SAC topology:
 * policy obs -> h1 -> h2 -> [mu | log sigma] (heads/sac_head.py:60-97), V obs -> h1 -> h2 -> 1 with a target copy, twin Q
 * towers relu(obs_fc s) + relu(act_fc a) -> fc -> 1 (heads/sac_q_head.py:46-96; q_* = float offsets of tower 0's tensors in
 * q.weights and the towers' strides).  normals [3][batch][act_dim] fp64: the host's standard-normal draws of the three
 * policy passes (resample_noise_per_pass == 0: only the first is used).  Outputs: value_targets, log_target = min(Q1, Q2),
 * td_targets [batch], dq_da [batch][act_dim], q_loss [3] = the towers' losses and their sum, v_loss [1].
 * policy.ticket: >= 1 zeroed word.  Six launches. */
typedef struct rlx_sac_fused_desc {
    rlx_fused_net policy, q, v;
    rlx_mlp3 policy_mlp, v_mlp;
    long long q_off_obs_w, q_off_obs_b, q_off_act_w, q_off_act_b, q_off_fc_w, q_off_fc_b, q_off_out_w, q_off_out_b;
    long long q_stride_obs, q_stride_act, q_stride_fc, q_stride_out;
    const float *obs, *next_obs, *actions, *rewards;
    const unsigned char *game_overs;
    const double *normals;
    double discount;
    int resample_noise_per_pass, batch, obs_dim, act_dim, q_hidden, reserved;
    float *workspace; long long workspace_floats;
    float *value_targets, *log_target, *td_targets, *dq_da, *q_loss, *v_loss;
} rlx_sac_fused_desc;
int rlx_sac_fused_supported(const rlx_sac_fused_desc *desc_host);
int rlx_sac_fused_workspace_floats(const rlx_sac_fused_desc *desc_host, long long *floats_host);
int rlx_sac_fused_update(const rlx_sac_fused_desc *desc_host, int write_grads, void *stream);

/* ------------------------------------------------- first convolution's weight gradient from uint8 frames -- */
/* dW1 = cols(frames)^T dz1 and db1 = column sums of dz1 for the first convolution of an image torso whose towers read the
 * SAME uint8 frames (rl_coach/architectures/tensorflow_components/embedders/image_embedder.py:33-40, layers.py:108-121;
 * the tf.gradients pass of architecture.py:187-220) — what rlx_gemm computed as an implicit-im2col product on its
 * register-staged uint8 loop.  frames [B][H][W][C] uint8 (network input = byte / a_div), dz [towers][B * OH * OW][filters]
 * (tower stride dz_tower_stride floats).  One workgroup per (image, pair of kernel rows); the images' partial sums go to
 * `workspace` and *job_host describes their outstanding reduction (one split per image, summed in image order) for
 * rlx_splitk_reduce_jobs: dw [KH * KW * C][filters] per tower (tower stride dw_tower_stride), db [filters] per tower or
 * NULL.  Shapes: KW * C == 32, KH even, towers * filters == 64, 2 <= B <= 128 (rlx_conv_dw_u8_supported). */
int rlx_conv_dw_u8_supported(int B, int H, int W, int C, int KH, int KW, int S, int filters, int towers);   /* 1 / 0 */
int rlx_conv_dw_u8_workspace_floats(int B, int H, int W, int C, int KH, int KW, int S, int filters, int towers,
                                    long long *floats_host);
int rlx_conv_dw_u8(const unsigned char *frames, float a_div, const float *dz, long long dz_tower_stride, int B, int H, int W,
                   int C, int KH, int KW, int S, int filters, int towers, float *dw, long long dw_tower_stride, float *db,
                   long long db_tower_stride, float *workspace, long long workspace_floats, rlx_splitk_job *job_host,
                   void *stream);
/* Measurement switch (no reference counterpart): workgroup 0 records s_memtime at its phase boundaries into 5 int64 words. */
int rlx_conv_dw_u8_stamps(long long *device_words5);

/* The same for an inner convolution layer with fp32 input activations x [towers][B][H][W][C] (tower stride x_tower_stride)
 * and 64 filters — the Atari torso's conv2 (4 x 4 x 32 stride 2 on 20 x 20) and conv3 (3 x 3 x 64 stride 1 on 9 x 9): one
 * workgroup per (tower, pair of images, kernel row), one deferred split per image pair.  dw [KH * KW * C][64] per tower. */
int rlx_conv_dw_f32_supported(int B, int H, int W, int C, int KH, int KW, int S, int filters, int towers);   /* 1 / 0 */
int rlx_conv_dw_f32_workspace_floats(int B, int H, int W, int C, int KH, int KW, int S, int filters, int towers,
                                     long long *floats_host);
int rlx_conv_dw_f32(const float *x, long long x_tower_stride, const float *dz, long long dz_tower_stride, int B, int H, int W,
                    int C, int KH, int KW, int S, int filters, int towers, float *dw, long long dw_tower_stride, float *db,
                    long long db_tower_stride, float *workspace, long long workspace_floats, rlx_splitk_job *job_host,
                    void *stream);
int rlx_conv_dw_f32_stamps(long long *device_words4);

/* The weight gradients of up to three convolution layers of one backward pass — independent once the input-gradient chain
 * has passed — as ONE launch: items[i] is what rlx_conv_dw_u8 (x_is_u8, x = frames) or rlx_conv_dw_f32 would get, jobs[i]
 * receives its outstanding reduction.  The one-launch form takes at most one uint8 item of the Atari geometry and two fp32
 * items; any other combination is issued item by item (same results either way). */
typedef struct rlx_conv_dw_item {
    const void *x; long long x_tower_stride;
    int x_is_u8; float a_div;
    const float *dz; long long dz_tower_stride;
    int B, H, W, C, KH, KW, S, filters, towers;
    float *dw; long long dw_tower_stride;
    float *db; long long db_tower_stride;
    float *workspace; long long workspace_floats;
} rlx_conv_dw_item;
int rlx_conv_dw_multi(const rlx_conv_dw_item *items_host, rlx_splitk_job *jobs_host, int n_items, void *stream);
/* rlx_conv_dw_multi + rlx_adam_tf1_step_early(adam, riders) as ONE launch: the grid of the one-launch form, taken with the
 * four-pass bodies whatever rlx_conv_dw_passes says (<= 50 KB of LDS: three workgroups per CU, of which the convolution
 * workgroups only ever fill two), plus `riders` workgroups that step the early blocks in the slot left over — dispatched
 * in front of the convolution workgroups (riders_first) or behind them.  Gradients and jobs as rlx_conv_dw_multi's, the
 * Adam step as rlx_adam_tf1_step_early's.  Items that do not take the one-launch form go out item by item and the early
 * step as a launch of its own behind them.  Every call applies the early step: never replay one. */
int rlx_conv_dw_multi_adam(const rlx_conv_dw_item *items_host, rlx_splitk_job *jobs_host, int n_items,
                           const rlx_adam_split_desc *adam_host, int riders, int riders_first, void *stream);
/* Process-wide (default 2): 2 = the one-launch form stages conv1's and conv2's operands in TWO passes over the output rows
 * (79 KB of LDS per workgroup instead of 157 KB: two workgroups per CU, one's fills under the other's products).  Weight
 * gradients identical; the inner layer's bias gradient sums its positions in another grouping (last bits).  -6 us per Clipped-PPO
 * update (profiles/r06_ab_conv_dw_passes.txt).  1 = the bodies of rlx_conv_dw_u8 / rlx_conv_dw_f32 as they are. */
int rlx_conv_dw_passes(int passes);
/* Process-wide, multi-pass forms only: image pairs an fp32 item's workgroup takes one after the other into the same
 * accumulators.  2: half the splits of the conv2 / conv3 weight gradients — 8.9 MB less partial sums written and read back per
 * Clipped-PPO minibatch update at the same launch time — at half the workgroups; 1: a split per pair; 0 (default): 2 where an
 * item has >= 64 (tower, pair) units, else 1 (profiles/r06_ab_conv_dw_pairs.txt). */
int rlx_conv_dw_pairs_per_workgroup(int pairs);

/* ------------------------------------------------- Clipped PPO: last dense layer + heads + losses, one launch -- */
/* The middleware's Dense(units) of both towers (tower 0 = value, tower 1 = policy; layers.py:168-185), VHead / discrete
 * PPOHead forward (heads/v_head.py:43-52, heads/ppo_head.py:52-116), both head losses (head.py:143-186) and the heads'
 * backward pass (architecture.py:312-385) — what rlx_gemm (row_heads) + rlx_ppo_heads_loss_backward did in three launches.
 * x [2][batch][in_features]; weights [in][units] / bias [units] per tower; value_w [units][1], policy_w [units][n_actions].
 * Outputs: h (the layer's output) and dz = d loss / d (its pre-activation) [2][batch][units]; values [batch], logits
 * [batch][n_actions] and their gradients; the heads' weight / bias gradients; scalars [5] = surrogate, entropy, KL, policy
 * total, value loss.  workspace / tickets: rlx_ppo_fc_heads_workspace (tickets zeroed once; every launch re-arms them). */
typedef struct rlx_ppo_fc_heads_desc {
    const float *x; long long x_tower_stride;
    const float *weights; long long weight_tower_stride;
    const float *bias; long long bias_tower_stride;
    const float *value_w, *value_b, *policy_w, *policy_b;
    const float *value_targets, *advantages, *old_probs; long long ld_old;
    const int *actions;
    const float *clip_scale;                 /* device scalar multiplying clip_epsilon, or null */
    float clip_epsilon, beta_entropy, grad_scale;
    int batch, in_features, units, n_actions, activation;
    float *h, *dz, *values, *logits, *dvalues, *dlogits;
    float *d_value_w, *d_value_b, *d_policy_w, *d_policy_b;
    float *scalars, *likelihood_ratio, *clipped_likelihood_ratio;
    int *status;
    float *workspace; long long workspace_floats;
    unsigned int *tickets;
} rlx_ppo_fc_heads_desc;
int rlx_ppo_fc_heads_supported(int batch, int in_features, int units, int n_actions);      /* 1 / 0 */
int rlx_ppo_fc_heads_workspace(int units, long long *floats_host, long long *ticket_words_host);
int rlx_ppo_fc_heads(const rlx_ppo_fc_heads_desc *desc_host, void *stream);
/* Measurement switch: workgroup 0 and the last arrivers record s_memtime into the workspace's last 16 int64. */
int rlx_ppo_fc_heads_stamps(int enable);

/* ------------------------------------------------- BitFlip on the device + hindsight relabelling (added entry points) -- */
/* The reference's toy problem (environments/toy_problems/bit_flip.py:54-90) for n_env envs, shaped like rlx_cartpole_*.
 * bits: uint8[n_env][2 * bit_length], [goal | state]; obs / next_obs / reset_obs: fp32[n_env][2 * bit_length] in the same
 * layout, 0 / 1 or, with mean_zero, -1 / +1.  Action a flips state bit a; reward 0 when state == goal else -1; game over
 * when they are equal or after max_steps steps.  next_obs is the stepped (terminal) observation; reset_obs (written only
 * where game_over is set) the first observation of the env's next episode.  Reset draws: Philox, key (seed, env_id0 + e),
 * counter (episode, word index, 0, 3), one bit per state / goal bit, low bit first; the goal is redrawn from the following
 * words while it equals the state, at most 32 times, then its bit 0 is flipped (csrc/bit_flip.hip).  status bit 1 = an
 * action outside [0, bit_length): nothing is flipped.  next_episode != 0: forced reset (every env starts its next episode). */
int rlx_bitflip_reset(unsigned char *bits, float *obs, int *episode, int *steps, int n_env, int bit_length,
                      int mean_zero, unsigned int seed, unsigned int env_id0, int next_episode, void *stream);
int rlx_bitflip_step(const int *action, unsigned char *bits, int *episode, int *steps, float *next_obs,
                     float *reset_obs, float *reward, unsigned char *game_over, int n_env, int bit_length,
                     int max_steps, int mean_zero, unsigned int seed, unsigned int env_id0, int *status,
                     void *stream);
/* EpisodicHindsightExperienceReplay.store_episode (episodic_hindsight_experience_replay.py:108-145) for ONE finished
 * episode of `length` steps stored time-major (row r(t) = ((first_step + t) mod ring_steps) * n_env + env < R =
 * n_env * ring_steps); every column has (1 + k) * R rows and copy j of real row r is row R + r * k + j.  For base
 * transition t < n_base and copy j, selected_steps[t * k + j] (device int32, in [0, length)) is the step whose STATE's
 * achieved slice [achieved_at, +goal_dim) becomes the goal: it replaces [goal_at, +goal_dim) of obs and next_obs in the
 * copy; the action row is copied; (reward, game_over) = distance(goal, achieved slice of next_obs[r(t)]) <= threshold ?
 * (goal_reaching_reward, 1) : (default_reward, 0), the distance in fp64 summed in index order.  status bit 2 = a
 * selected step outside the episode (that copy is not written). */
#define RLX_HER_EUCLIDEAN 0
#define RLX_HER_MANHATTAN 2
int rlx_her_relabel_episode(float *obs, float *next_obs, void *action, float *reward, unsigned char *game_over,
                            const int *selected_steps, long long first_step, int length, int n_base, int k, int env,
                            int n_env, long long ring_steps, int obs_dim, int goal_at, int achieved_at, int goal_dim,
                            int action_row_bytes, int metric, double threshold, float goal_reaching_reward,
                            float default_reward, int *status, void *stream);

/* ------------------------------------------------- ExplorationChain on the device (added entry points) -- */
/* The reference's toy problem (environments/toy_problems/exploration_chain.py:24-94) for n_env envs, shaped like
 * rlx_bitflip_*.  state / steps: int32[n_env]; obs / next_obs / reset_obs: fp32[n_env][chain_length], ones at [0, state]
 * (therm != 0) or at state alone (therm == 0).  Action 0 moves left unless state == 0, action 1 right unless state ==
 * chain_length - 1; reward after the move: left_state_reward at state 0, right_state_reward at the last state, else 0;
 * game over when steps >= max_steps.  next_obs is the stepped (terminal) observation; reset_obs (written only where
 * game_over is set) the observation of start_state.  No random draws: every episode lasts exactly max_steps steps.
 * status bit 1 = an action other than 0 / 1: nothing moves (the step counts).  chain_length > 3, 0 <= start_state <
 * chain_length. */
int rlx_chain_reset(int *state, int *steps, float *obs, int n_env, int chain_length, int start_state, int therm,
                    void *stream);
int rlx_chain_step(const int *action, int *state, int *steps, float *next_obs, float *reset_obs, float *reward,
                   unsigned char *game_over, int n_env, int chain_length, int start_state, int max_steps, int therm,
                   float left_state_reward, float right_state_reward, int *status, void *stream);

/* ------------------------------------------------------- Policy Gradients (added entry points) -- */
/* One update window of PolicyOptimizationAgent.train for a PolicyGradientsAgent (agents/policy_optimization_agent.py:
 * 85-135, agents/policy_gradients_agent.py:98-126), one workgroup, fp64 in the reference's operation order:
 *   returns_out[0 .. length)   Episode.update_discounted_rewards with n_step -1 over the WHOLE episode so far
 *                              (core_types.py:780-801; the sum of rlx_episode_nstep_returns) — bit-identical;
 *   the two normalised rescalers: update_episode_statistics (:72-83) over the whole episode: episodes_seen[i] += 1,
 *                              m[i] -= m[i] / n[i]; m[i] += r[i] / n[i] (bit-identical), and the episode's np.mean /
 *                              np.std into stats_out[2], [3] (numpy's pairwise summation restated; 0, 0 otherwise);
 *   rescaled_out[i], i < length - start: the rescaling loop on the window episode[start:] — TOTAL_RETURN copies entry 0
 *                              of the window, FUTURE_RETURN_NORMALIZED_BY_TIMESTEP subtracts mean_over_episodes[i] with i
 *                              the position in the BATCH, FUTURE_RETURN_NORMALIZED_BY_EPISODE gives 0 when std == 0;
 *   advantages_out[i]          the same value rounded to fp32 once (the head's placeholder);
 *   stats_out[0], [1]          'Returns Mean' = np.mean, 'Returns Variance' = np.std of rescaled_out.
 * rewards: the episode's filtered rewards [length], contiguous.  mean_over_episodes / episodes_seen / returns_out /
 * rescaled_out / advantages_out have max_length entries; an episode longer than max_length raises
 * RLX_PG_STATUS_EPISODE_TOO_LONG in *status and nothing else is read or written. */
#define RLX_PG_TOTAL_RETURN 0
#define RLX_PG_FUTURE_RETURN 1
#define RLX_PG_FUTURE_RETURN_NORMALIZED_BY_EPISODE 2
#define RLX_PG_FUTURE_RETURN_NORMALIZED_BY_TIMESTEP 3
#define RLX_PG_STATUS_EPISODE_TOO_LONG 2
int rlx_pg_episode_window(const float *rewards, int length, int start, double discount, int rescaler,
                          double *mean_over_episodes, double *episodes_seen, int max_length, double *returns_out,
                          double *rescaled_out, float *advantages_out, double *stats_out, int *status, void *stream);
/* PolicyHead, discrete branch (architectures/tensorflow_components/heads/policy_head.py:75-100) as one launch of one
 * workgroup.  logits [rows][ld]; rows [true_rows, rows) are padding (zero gradient, no term); every mean divides by
 * true_rows.  Per row, fp32, eps = np.finfo(np.float32).eps: p = softmax(z) as rlx_c51_head_loss defines it, q = p + eps,
 * S = sum q (index order), log pi = log q - log S with log x = (float)log((double)x) (tf Categorical(probs = q)),
 * H = -sum (q / S) log pi.  scalars[0] = loss = -(1/T) sum_b log pi_b(a_b) adv_b - beta_entropy * scalars[1],
 * scalars[1] = (1/T) sum_b H_b (thread partials in row order, then a fixed tree: no atomics); dlogits = dloss/dz.
 * status bit 0 = an action outside [0, n_actions): that row has no term and a zero gradient.  1 <= n_actions <= 18. */
int rlx_pg_head_loss(const float *logits, long long ld, const int *actions, const float *advantages, float beta_entropy,
                     int rows, int true_rows, int n_actions, float *dlogits, long long ld_dlogits, float *scalars,
                     int *status, void *stream);
/* The 'Entropy' sample of PolicyOptimizationAgent.choose_action (policy_optimization_agent.py:154), per env, fp32:
 * -sum_j p_j * log(p_j + eps) on action probabilities [n_env][ld]. */
int rlx_action_entropy(const float *probs, long long ld, int n_env, int n_actions, float *entropy_out, void *stream);

/* ------------------------------------------------------- Actor-Critic / A3C (added entry point) -- */
/* ActorCriticAgent.learn_from_batch (agents/actor_critic_agent.py:127-186) between the forward and the backward pass of
 * one update window of T transitions, one launch of one workgroup.  The forward pass ran on `rows` states: rows = T + 1
 * when the window bootstraps (the last row is the last next state), rows = T is allowed when the last transition is a
 * game over.  *game_over is that transition's flag, read on the device.
 *   targets_out / advantages_out [T], fp64, the reference's operation order (a sequential reverse recurrence):
 *     RLX_A3C_A_VALUE  R = 0 on a game over, else V[T];  R = r_i + discount * R;  target_i = R, adv_i = R - V_i (:145-154);
 *     RLX_A3C_GAE      values = V[0 .. T] with values[T] = 0 on a game over; deltas = r + discount * values[1:] -
 *                      values[:-1]; adv = the lfilter recurrence y_i = x_i + discount * gae_lambda * y_{i+1} over the
 *                      deltas; targets = adv + V when estimate_state_value_using_gae, else the same recurrence with
 *                      `discount` over the rewards extended by values[T], without its last element (:108-125, :156-165).
 *     `discount * <fp32 V>` is an fp32 product where the reference's is (tests/a3c_ref.py names the lines).
 *     RLX_A3C_TARGETS_GIVEN  both arrays are INPUTS (what Architecture.accumulate_gradients is handed, :175-177);
 *                      rewards and game_over are not read (they may be null) and nothing is bootstrapped.
 *   The heads read both rounded to fp32 once.  Every mean divides by T; the bootstrap row has no term, dV = 0, dlogits = 0.
 *   V head (VHead, heads/head.py:170-181): scalars[1] = value loss = (1/T) sum_b v_loss_weight * (V_b - target_b)^2,
 *     dV_b = v_loss_weight * 2 (V_b - target_b) / T.
 *   Policy head: the row arithmetic, status bit 0 and dlogits of rlx_pg_head_loss with these advantages (one shared
 *     definition, csrc/policy_head.hpp).  scalars[2] = policy loss = -(1/T) sum_b log pi_b(a_b) adv_b,
 *     scalars[3] = mean entropy, scalars[0] = total = scalars[1] + (scalars[2] - beta_entropy * scalars[3]).
 *   Batch sums: thread partials in row order, then a fixed tree (no atomics).
 * A window that is not a game over with rows = T raises RLX_A3C_STATUS_NO_BOOTSTRAP_ROW and nothing else is read or
 * written.  V / dV are read and written at strides ld_v / ld_dv.  1 <= n_actions <= 18. */
#define RLX_A3C_A_VALUE 5             /* PolicyGradientRescaler.A_VALUE */
#define RLX_A3C_GAE 8                 /* PolicyGradientRescaler.GAE */
#define RLX_A3C_TARGETS_GIVEN -1
#define RLX_A3C_STATUS_NO_BOOTSTRAP_ROW 2
int rlx_a3c_window_loss(const float *V, long long ld_v, const float *logits, long long ld, const int *actions,
                        const float *rewards, const unsigned char *game_over, int T, int rows, int n_actions,
                        double discount, double gae_lambda, int rescaler, int estimate_state_value_using_gae,
                        float beta_entropy, float v_loss_weight, double *targets_out, double *advantages_out, float *dV,
                        long long ld_dv, float *dlogits, long long ld_dlogits, float *scalars, int *status,
                        void *stream);

/* ------------------------------------------------------------- N-step Q (added entry point) -- */
/* NStepQAgent.learn_from_batch (agents/n_step_q_agent.py:99-140) between the forward and the backward pass of one update
 * window of T transitions, one launch of one workgroup.  q_online [T][ld_q] is the online network on the window's
 * states; q_target [rows_t][ld_t] the TARGET network on the state behind the window (RLX_NSTEPQ_N_STEP: one row) or on
 * the T next states (RLX_NSTEPQ_ONE_STEP: T rows).  *game_over is the last transition's flag, read on the device (a
 * window never spans episodes, so only its last row can be terminal).
 *   targets [T], fp32: the value written into column actions[i] of row i of the online prediction:
 *     RLX_NSTEPQ_N_STEP    R = 0 on a game over, else max_a q_target[0][a];  R = r_i + discount * R backwards (a
 *                          sequential fp64 recurrence whose FIRST product is fp32, as the reference's is);
 *                          target_i = R rounded to fp32 once (:116-125).  A game over reads no target row.
 *     RLX_NSTEPQ_ONE_STEP  target_i = r_i + ((1 - game_over_i) * discount) * max_a q_target[i][a], fp64 on the widened
 *                          maximum, rounded to fp32 once (:107-114).
 *     RLX_NSTEPQ_TARGETS_GIVEN  targets is an INPUT (the taken column of what Architecture.accumulate_gradients is
 *                          handed, :134); no target row, reward or game-over flag is read (they may be null).
 *     tests/n_step_q_ref.py names the reference's line of every rounding point.
 *   td_targets [T][ld_tt], optional (may be null): the full state_value_head_targets matrix — q_online with that column
 *     replaced — the 'Q Values' signal.
 *   Q head (csrc/losses_body.hpp, the convention of rlx_regression_loss): e_b = q_online[b][a_b] - target_b, MSE or
 *     (huber != 0) Huber with delta 1; scalars[0] = loss = (1/T) sum_b l_b; dq[b][a_b] = g_b / T and every other entry of
 *     dq is exactly 0: the target matrix equals the online prediction there (as for rlx_dqn_head_loss).
 *   Batch sum: thread partials in row order, then a fixed tree (no atomics).
 * An action outside [0, n_actions) raises RLX_NSTEPQ_STATUS_BAD_ACTION: the row has no term, a zero dq row, its
 * td_targets row is the online row and its targets entry is untouched; the mean still divides by T.  A window that is
 * not a game over with rows_t < 1 (N_STEP), or any window with rows_t < T (ONE_STEP), raises
 * RLX_NSTEPQ_STATUS_NO_TARGET_ROWS and nothing else is read or written. */
#define RLX_NSTEPQ_N_STEP 0           /* targets_horizon = 'N-Step' */
#define RLX_NSTEPQ_ONE_STEP 1         /* targets_horizon = '1-Step' */
#define RLX_NSTEPQ_TARGETS_GIVEN -1
#define RLX_NSTEPQ_STATUS_BAD_ACTION 1
#define RLX_NSTEPQ_STATUS_NO_TARGET_ROWS 2
int rlx_nstep_q_window_loss(const float *q_online, long long ld_q, const float *q_target, long long ld_t, int rows_t,
                            const int *actions, const float *rewards, const unsigned char *game_over, int T,
                            int n_actions, double discount, int horizon, int huber, float *targets, float *td_targets,
                            long long ld_tt, float *dq, long long ld_dq, float *scalars, int *status, void *stream);

/* ------------------------------------------------------------------ ACER (added entry point) -- */
/* ACERAgent._learn_from_batch (agents/acer_agent.py:118-165) between the forward and the backward pass of one update
 * window of T transitions, one launch of one workgroup.  q / logits [rows][ld] are the online network's Q head and policy
 * head: rows = T + 1 when the window bootstraps (the last row is the state behind the window), rows = T is allowed when
 * the last transition is a game over.  avg_logits [T][ld] is the average (target) network's policy head on the T
 * states, mu [T][ld_mu] the behaviour policy's stored probabilities.  *game_over is the last transition's flag, read on
 * the device.
 *   Phase 1, per row (arrays that are outputs; the 'Values' signal reads V):
 *     p = softmax(logits) and avg_policy = softmax(avg_logits) as csrc/policy_head.hpp defines it;
 *     V_b = np.sum(p * Q) in numpy's own order (a plain loop below 8 actions, eight accumulators from 8 on);
 *     rho = p / (mu + eps);  rho_i = rho[b][a_b];  *bootstrap_value = np.sum(Q * p) of row T (0 on a game over).
 *   Phase 2, q_retrace [T], fp32: Qret = 0 on a game over, else *bootstrap_value; backwards, sequentially,
 *     Qret = r_i + discount * Qret (fp64, but the FIRST product is fp32, as the reference's is); q_retrace_i = Qret
 *     rounded to fp32 once; Qret = min(1, rho_i) * (Qret - Q[i][a_i]) + V_i in fp64.  tests/acer_ref.py names the
 *     reference's line of every rounding point.
 *   td_targets [T][ld_tt], optional (may be null): q with the taken entries replaced by q_retrace — the Q head's target
 *     AND, because the reference aliases the two arrays, the Q values the policy head is fed (Q').
 *   Phase 3, per row.  Q head (csrc/losses_body.hpp, the convention of rlx_regression_loss): e_b = q[b][a_b] -
 *     q_retrace_b, MSE; scalars[1] = (1/T) sum_b q_loss_weight * e_b^2; dq[b][a_b] = q_loss_weight * 2 e_b / T and every
 *     other entry of dq exactly 0.  ACER policy head (csrc/acer_head.hpp; acer_policy_head.py:47-113), with log pi, H of
 *     the discrete policy row:
 *       scalars[3] = probability loss     = -(1/T) sum_b log pi_b(a_b) (q_retrace_b - V_b) min(truncation, rho_i_b)
 *       scalars[4] = bias-correction loss = -(1/T) sum_b sum_k log(p_k + eps) (Q'_k - V_b) relu(1 - truncation /
 *                                            (rho_k + eps)) p_k   (the trailing p_k under stop_gradient)
 *       scalars[2] = policy loss = scalars[3] + scalars[4];   scalars[6] = mean entropy;
 *       scalars[5] = (1/T) sum_b KL(Categorical(avg_policy + eps) || Categorical(p + eps)), logged only;
 *       scalars[0] = total = scalars[1] + (scalars[2] - beta_entropy * scalars[6]).
 *     dlogits = dz_j = p_j (g_j - sum_k g_k p_k) with g = dL/dp of the row.  With RLX_ACER_TRUST_REGION in `mode`, g first
 *     goes through the reference's trust_region_layer gradient (g' = -g T; k = -avg_policy / (p + eps); adj = relu((sum
 *     k g' - max_kl) / (sum k^2 + eps)); g' -= adj k; g = -g' / T).  The reference's own graph never routes a gradient
 *     through that layer, so the faithful mode is without the bit.
 *   Every mean divides by T; the bootstrap row has no term and exactly zero dq and dlogits rows.  Batch sums: thread
 *   partials in row order, then a fixed tree (no atomics).
 * RLX_ACER_TARGETS_GIVEN in `mode`: phases 1 and 2 are skipped; V, rho, rho_i, avg_policy and q_retrace are INPUTS (what
 *   Architecture.accumulate_gradients is handed: target 1, output_1_1, output_1_2, output_1_5, output_1_4), td_targets,
 *   when not null, is read as Q' (output_1_3), else Q' is q with the taken entry replaced; avg_logits, mu, rewards,
 *   game_over and bootstrap_value are not touched (they may be null) and nothing is bootstrapped.
 * An action outside [0, n_actions) raises RLX_ACER_STATUS_BAD_ACTION: the row has no term and zero gradient rows, its
 * td_targets row is the online row, and the recurrence passes V_i on (rho_i = 0); the means still divide by T.  A window
 * that is not a game over with rows = T raises RLX_ACER_STATUS_NO_BOOTSTRAP_ROW and nothing else is read or written.
 * 1 <= n_actions <= 18, any T >= 1. */
#define RLX_ACER_TRUST_REGION 1
#define RLX_ACER_TARGETS_GIVEN 2
#define RLX_ACER_STATUS_BAD_ACTION 1
#define RLX_ACER_STATUS_NO_BOOTSTRAP_ROW 2
int rlx_acer_window_loss(const float *q, long long ld_q, const float *logits, long long ld_logits, int rows,
                         const float *avg_logits, long long ld_avg_logits, const float *mu, long long ld_mu,
                         const int *actions, const float *rewards, const unsigned char *game_over, int T, int n_actions,
                         double discount, float truncation, float max_kl, float beta_entropy, float q_loss_weight,
                         int mode, float *V, float *rho, long long ld_rho, float *rho_i, float *avg_policy,
                         long long ld_avg_policy, float *q_retrace, float *bootstrap_value, float *td_targets,
                         long long ld_tt, float *dq, long long ld_dq, float *dlogits, long long ld_dlogits,
                         float *scalars, int *status, void *stream);

/* ------------------------------------------------- Batch RL: DDQN-BCQ's action mask -- */
/* (csrc/bcq.hip; bit-exact numpy twin: tests/bcq_ref.py.  Entry points ADDED under ABI version 11: no existing
 * signature or structure changed.)
 *
 * rlx_nn_min_distance: what AnnoyDictionary._get_k_nearest_neighbors_indices(keys, 1) returns as distances
 * (memories/non_episodic/differentiable_neural_dictionary.py, as agents/ddqn_bcq_agent.py:109-111 and :212-214 use it),
 * computed EXACTLY instead of by an approximate forest.  keys is one fp32 matrix [n_keys][ld_k]; rows set_offsets[s] ..
 * set_offsets[s + 1] - 1 are set s (one set per action; set_offsets: device int32 [n_sets + 1], non-decreasing; the
 * launch clamps it to [0, n_keys], so a bad table cannot read past the keys).  dist_out[i][s] (fp32 [n_queries][ld_out])
 * is the Euclidean distance from query i to its nearest key of set s:
 *   per (query, key) pair acc = 0.f; for w = 0 .. width - 1 in this order t = q[w] - k[w]; acc = acc + t * t (separate
 *   fp32 roundings, no FMA); the set's value is min over its keys of acc, then one correctly rounded sqrtf.
 * Identical vectors give exactly 0.0f; an empty set gives +inf.  Input range: every |q[w] - k[w]| below 2^63 / sqrt(width),
 * so that no difference and no accumulator overflows (network embeddings are far inside it); beyond it a pair's inf - inf is a
 * NaN, whose bit pattern sorts above +inf in the unsigned minimum and is dropped, where numpy's min would return NaN.  The keys are split over
 * workgroups in chunks of RLX_NN_KEY_CHUNK and the partial minima meet in an integer atomicMin on the bit pattern of
 * the non-negative squared distance: deterministic.  Three launches (fill, search, square root), all capturable.
 * 1 <= width <= 512, 1 <= n_sets <= 18, n_queries >= 1, ld_q, ld_k >= width, ld_out >= n_sets. */
#define RLX_NN_KEY_CHUNK 128
int rlx_nn_min_distance(const float *queries, long long ld_q, int n_queries, int width, const float *keys,
                        long long ld_k, long long n_keys, const int *set_offsets, int n_sets, float *dist_out,
                        long long ld_out, void *stream);
/* DDQNBCQAgent.select_actions up to its argmax (agents/ddqn_bcq_agent.py:107-133): sel_out[b][a] = q_next_online[b][a],
 * or -inf where (double)familiarity[b][a] > threshold (threshold = average_dist_coefficient * average_dist, a double).
 * A row whose maximum is then -inf (every action masked) gets sel_out[b][a] = u(b, a) instead: uniforms in [0, 1), the
 * top 24 bits of word 0 of Philox4x32-10 under the key (seed, rank) at the counter (event low word, event high word, b,
 * a), times 2^-24.  (The reference draws np.random.rand(number of such rows, A) on the host; that number is device
 * data here.)  event is READ FROM DEVICE MEMORY (one int64), so a captured graph follows it.  zero_rows_out (optional
 * device int): the number of such rows.  sel_out is the q_next_selector operand of rlx_dqn_head_loss, whose argmax
 * (first maximum) is the reference's np.argmax.  One workgroup: batch <= 1024, 1 <= n_actions <= 18. */
int rlx_bcq_masked_selector(const float *q_next_online, long long ld_q, const float *familiarity, long long ld_f,
                            double threshold, int batch, int n_actions, unsigned int seed, unsigned int rank,
                            const long long *event, float *sel_out, long long ld_sel, int *zero_rows_out, void *stream);
/* The reward model's regression targets (agents/value_optimization_agent.py:173-180): targets = prediction with
 * targets[b][actions[b]] = rewards[b].  targets may be prediction itself (same pointer AND ld_t == ld_p).  status bit 1: an action outside [0, n_actions)
 * (that row stays the prediction). */
int rlx_reward_model_targets(const float *prediction, long long ld_p, const int *actions, const float *rewards, int batch,
                             int n_actions, float *targets, long long ld_t, int *status, void *stream);

/* ------------------------------------------------- Batch RL: off-policy evaluation -- */
/* (csrc/ope.hip; numpy restatement: tests/ope_ref.py.  Entry points ADDED under ABI version 11: no existing signature
 * or structure changed.)  All three are capturable, deterministic (no floating-point atomics: the same bits on a second
 * call), synchronise nothing with the host, serve 1 <= n_actions <= RLX_OPE_MAX_ACTIONS and accept padded leading
 * dimensions.
 *
 * The fp32 softmax both sides share (heads/q_head.py:56-68, softmax(q / temperature)): z[k] = q[k] / (float)temperature;
 * m = max z; e[k] = expf(z[k] - m); s = e[0] + e[1] + ... in action order from 0.f; p[k] = e[k] / s — every operation
 * rounded to fp32 on its own.
 *
 * rlx_behaviour_probabilities: what the reference stores as all_action_probabilities while a dataset is collected
 * (agents/value_optimization_agent.py:98-102, exploration_policies/e_greedy.py:84-101, spaces.py:458).  Per env e,
 * probs_out[e][.] is the uniform vector 1.0f / (float)n_actions when force_uniform != 0 (random heat-up) or
 * explore_uniforms[e] < epsilon (rlx_egreedy's comparison on the same staged draw), else the softmax above of
 * q_values[e].  With force_uniform != 0, q_values and explore_uniforms may be null. */
#define RLX_OPE_MAX_ACTIONS 18
int rlx_behaviour_probabilities(const float *q_values, long long ld_q, const double *explore_uniforms, double epsilon,
                                int force_uniform, double temperature, int n_env, int n_actions, float *probs_out,
                                long long ld_out, void *stream);
/* OpeManager._prepare_ope_shared_stats and the per-row terms of DoublyRobust.evaluate (off_policy_evaluators/
 * ope_manager.py:49-101, bandits/doubly_robust.py:34-38), one lane per evaluation row j of n_rows.  pi_out[j][.] is the
 * softmax above of q_values[j].  row_columns is fp64 [RLX_OPE_ROW_COLUMNS][n_rows] (plane c at row_columns + c * n_rows),
 * every value computed in fp64 from fp32 values widened once, sums over the actions in action order from 0.0:
 *   RHO      rho_j = pi[j][a_j] / mu[j][a_j]                 (mu = behaviour_probs; a zero there is not special-cased:
 *                                                             the IEEE inf, or NaN of 0 / 0, propagates as in numpy)
 *   V        v_j   = sum_a pi[j][a] * q[j][a]
 *   Q_TAKEN  q[j][a_j]
 *   IPS      rho_j * r_j
 *   DM       sum_a pi[j][a] * reward_model[j / dm_row_divisor][a]
 *   DR       rho_j * (r_j - reward_model[j][a_j])
 * dm_row_divisor >= 1: 1 is the direct method of the paper; the reference multiplies every row of inference batch i by
 * the reward model's output for dataset row i (ope_manager.py:80), which is dm_row_divisor = its batch size.
 * An action outside [0, n_actions) sets status bit 1 and its row's six values are 0 (pi_out is still written). */
#define RLX_OPE_ROW_COLUMNS 6
#define RLX_OPE_COL_RHO 0
#define RLX_OPE_COL_V 1
#define RLX_OPE_COL_Q_TAKEN 2
#define RLX_OPE_COL_IPS 3
#define RLX_OPE_COL_DM 4
#define RLX_OPE_COL_DR 5
int rlx_ope_rows(const float *q_values, long long ld_q, const float *reward_model, long long ld_rm,
                 long long dm_row_divisor, const int *actions, const float *rewards, const float *behaviour_probs,
                 long long ld_mu, double temperature, long long n_rows, int n_actions, float *pi_out, long long ld_pi,
                 double *row_columns, int *status, void *stream);
/* The five estimates from rlx_ope_rows' columns (bandits/doubly_robust.py:34-38, rl/sequential_doubly_robust.py:40-51,
 * rl/weighted_importance_sampling.py:41-55).  episode_offsets: device int32 [n_episodes + 1] into the evaluation rows
 * (clamped to [0, n_rows]); rewards fp32 [n_rows]; returns fp64 [n_rows], of which the first row of every episode is
 * read (its n_step_discounted_rewards).  episode_columns is fp64 [RLX_OPE_EPISODE_COLUMNS][n_episodes]:
 *   SEQ_DR  the value at the episode's first row of acc_j = A_j + B_j * acc_{j+1}, acc past the last row = 0, with
 *           B_j = discount * rho_j and A_j = v_j + rho_j * (r_j - q[j][a_j]) — as the composition of the rows' affine
 *           maps, 64 rows per pass of one wave, the passes folded in row order
 *   W       w_e = the product of rho_j over the episode (the same tree)
 *   WR      w_e * returns[first row]   (0 for an episode without rows)
 * out is fp64 [RLX_OPE_OUT]: {IPS = sum IPS_j / n, DM = sum DM_j / n, DR = sum DR_j / n + DM, sequential DR = sum
 * SEQ_DR_e / E, WIS = sum WR_e / sum W_e or 0 when sum W_e == 0, sum W_e, E}; the six sums are fixed-shape fp64 trees.
 * Two launches.  Where a rho is not finite the composed map may hold a NaN where the reference's row-by-row loop holds
 * an infinity (inf * 0 inside the composition). */
#define RLX_OPE_EPISODE_COLUMNS 3
#define RLX_OPE_EP_SEQ_DR 0
#define RLX_OPE_EP_W 1
#define RLX_OPE_EP_WR 2
#define RLX_OPE_OUT 7
int rlx_ope_reduce(const int *episode_offsets, int n_episodes, long long n_rows, const double *row_columns,
                   const float *rewards, const double *returns, double discount, double *episode_columns, double *out,
                   void *stream);

/* ------------------------------------------------- Batch RL: a logged dataset becomes replay rows -- */
/* (csrc/dataset.hip; bit-exact numpy twin: tests/dataset_ref.py.  An entry point ADDED under ABI version 11.)
 *
 * The device half of EpisodicExperienceReplay.load_csv (memories/episodic/episodic_experience_replay.py:440-495).  The
 * file's rows arrive as flat tables — features fp64 [n_rows][ld_features] (D used), actions int32 [n_rows], rewards fp64
 * [n_rows], probabilities fp32 [n_rows][ld_probabilities] (A used) or NULL — and transition t of n_transitions takes its
 * state, action, reward and probabilities from file row src[t], its next state from file row src_next[t].  It is written
 * to row first_row + t of the memory's columns (mem_obs / mem_next_obs fp32 [mem_rows][D], mem_action int32, mem_reward
 * fp32, mem_game_over u8, mem_probabilities fp32 [mem_rows][A] or NULL — NULL exactly when probabilities is):
 *   obs, next_obs   (float)feature: rounded to fp32 once, to nearest even
 *   reward          (float)reward, then rlx_reward_filter's arithmetic on that fp32 value (rescale_factor, has_clip,
 *                   clipping_low, clipping_high as there: a bound of 0 is not applied)
 *   game_over       last[t] != 0 && is_episodic
 * status bits (rows that raise one are still written): 1 an action outside [0, A) (stored as 0); 2 a feature or a reward
 * that is not finite as fp32; 4 a src / src_next outside [0, n_rows) (the cells it would have read are written as 0).
 * 1 <= D <= 4096, 1 <= A <= 18, n_transitions >= 1, 0 <= first_row, first_row + n_transitions <= mem_rows,
 * ld_features >= D, ld_probabilities >= A, n_rows < 2^31. */
int rlx_dataset_ingest(const double *features, long long ld_features, const int *actions, const double *rewards,
                       const float *probabilities, long long ld_probabilities, long long n_rows, int D, int A,
                       const int *src, const int *src_next, const unsigned char *last, long long n_transitions,
                       int is_episodic, long long first_row, long long mem_rows, double rescale_factor, int has_clip,
                       double clipping_low, double clipping_high, float *mem_obs, float *mem_next_obs, int *mem_action,
                       float *mem_reward, unsigned char *mem_game_over, float *mem_probabilities, int *status,
                       void *stream);

/* ------------------------------------------ Wolpertinger: exact k-NN action lookup, critic re-ranking -- */
/* (csrc/wolpertinger.hip; bit-exact numpy twin: tests/wolpertinger_ref.py.  Entry points ADDED under ABI version 11.)
 *
 * rlx_knn_topk: AnnoyDictionary.query as WolpertingerAgent.choose_action uses it (agents/wolpertinger_agent.py:92-100),
 * exact instead of approximate.  For every query row the k keys of smallest squared Euclidean distance:
 * idx_out int32 [n_queries][k] and, where dist2_out is not NULL, the squared distances fp32 [n_queries][k], both
 * ascending in the pair (squared distance, key index): equal distances go to the lower index, a NaN distance sorts
 * behind +inf, by index, and is written as the quiet NaN 0x7fc00000.  The squared distance is rlx_nn_min_distance's:
 * acc = 0, then for w = 0 .. width-1 in order t = q[w] - key[w], acc = acc + t * t, each operation rounded to fp32 on
 * its own, no FMA; never |q|^2 + |k|^2 - 2 q.k — a query that IS a key has distance exactly 0.
 * Deterministic: every pair is one 64-bit word (distance bits, index) ordered as an unsigned integer; the keys are
 * split over workgroups in chunks of RLX_KNN_KEY_CHUNK, each leaving its k smallest words in `scratch`, and merge passes
 * over RLX_KNN_KEY_CHUNK / k lists at a time follow until one list is left: 1 + ceil(log_{CHUNK / k}(chunks)) launches,
 * no atomics, no allocation, no synchronisation (capturable).  queries [n_queries][ld_q], keys [n_keys][ld_k]: 16-byte
 * loads where base and leading dimension allow them (and across four keys of a width-1, ld_k = 1 table), scalar loads
 * otherwise.  scratch: device memory, 8-byte aligned, of at least rlx_knn_topk_scratch_bytes(...) bytes (0 when the keys
 * fit one chunk: scratch may then be NULL); its contents mean nothing between calls.
 * 1 <= k <= 64, k <= n_keys <= 2^31 - 1, 1 <= width <= 64, ld_q, ld_k >= width, 1 <= n_queries <= 65535. */
#define RLX_KNN_KEY_CHUNK 2048
int rlx_knn_topk_scratch_bytes(int n_queries, long long n_keys, int k, long long *bytes_out);
int rlx_knn_topk(const float *queries, long long ld_q, int n_queries, int width, const float *keys, long long ld_k,
                 long long n_keys, int k, int *idx_out, float *dist2_out, void *scratch, long long scratch_bytes,
                 void *stream);
/* The critic's two inputs for the n_env * k candidates (agents/wolpertinger_agent.py:103-105: np.tile of the observation,
 * nn_action_embeddings): row e * k + j of obs_out [n_env * k][ld_obs_out] is observations[e][0 .. obs_dim), row e * k + j
 * of action_out [n_env * k][ld_action_out] is keys[idx[e][j]][0 .. width) (zeros for an index outside [0, n_keys)).
 * A launch of its own, after rlx_knn_topk's last pass.  k <= 64, width <= 64. */
int rlx_wolpertinger_candidates(const int *idx, const float *keys, long long ld_k, long long n_keys, int width,
                                const float *observations, long long ld_obs, int obs_dim, int n_env, int k,
                                float *obs_out, long long ld_obs_out, float *action_out, long long ld_action_out,
                                void *stream);
/* action_out[e] = idx[e][np.argmax_j q[(e * k + j) * q_stride]] (agents/wolpertinger_agent.py:106-107; the first
 * maximum, and a NaN counts as the maximum: the first NaN wins) and env_action_out[e][0 .. action_dim) =
 * target_actions[action_out[e]][0 .. action_dim), BoxDiscretization's filter (zeros for an action outside
 * [0, n_actions)).  q_stride: elements between two candidates' Q values.  k <= 64. */
int rlx_wolpertinger_select(const float *q, long long q_stride, const int *idx, int n_env, int k,
                            const float *target_actions, long long ld_t, long long n_actions, int action_dim,
                            int *action_out, float *env_action_out, long long ld_env, void *stream);
/* WolpertingerAgent.learn_from_batch's conversion (agents/wolpertinger_agent.py:77-83): out[b][0 .. action_dim) =
 * target_actions[actions[b]][0 .. action_dim).  status bit 1: an action outside [0, n_actions); its row is zero. */
int rlx_discrete_to_box(const int *actions, int batch, const float *target_actions, long long ld_t, long long n_actions,
                        int action_dim, float *out, long long ld_out, int *status, void *stream);

/* ------------------------------------ Imitation learning: classification head, BCQ's imitation-model mask -- */
/* (csrc/imitation.hip; bit-exact numpy twin: tests/imitation_ref.py.  Entry points ADDED under ABI version 11: no
 * existing signature or structure changed.)  Both are one launch of one workgroup, one row per thread, capturable,
 * deterministic (no atomics in any sum), and share ONE softmax with rlx_pg_head_loss (csrc/policy_head.hpp, softmax_row):
 *   mx = max_j z_j;  e_j = (float)exp((double)(z_j - mx));  s = sum_j e_j in index order;  p_j = e_j / s      (all fp32)
 *
 * rlx_classification_head_loss: ClassificationHead (architectures/tensorflow_components/heads/classification_head.py)
 * between the forward and the backward pass.  logits [rows][ld]; the target is EITHER actions (int32 [rows]: the one-hot
 * row, never formed) OR labels (fp32 [rows][ld_labels], the dense matrix Architecture.train_on_batch is handed): exactly
 * one of the two is not NULL.  Per row, fp32:
 *   log p_j = (z_j - mx) - (float)log((double)s)
 *   actions: loss_b = -log p_a                         labels: loss_b = -(sum_j l_j * log p_j), index order from 0.f
 *   dlogits[b][j] = (p_j - l_j) * grad_scale           (tf.nn.softmax_cross_entropy_with_logits: no sum-of-labels
 *                                                       factor; l is the one-hot row in actions mode)
 * The head hands the per-row vector to tf.losses.add_loss and general_network.py:360 takes its tf.reduce_sum, so
 * scalars[0] = SUM_b loss_b — not a mean, and dlogits carries no 1 / rows — summed through the tree of a workgroup of
 * T = max(64, rows rounded up to a power of two) threads (thread b holds loss_b, 0.f beyond the batch; for d = T / 2,
 * T / 4 .. 1: v[b] += v[b + d] for b < d).  The head's loss_weight is not applied, as in the reference.
 * scalars[1] = the number of rows whose first-maximum argmax of p equals the action (labels: the labels' first maximum).
 * Optional outputs: probs_out [rows][ld_probs] = p (the head's output, what predict returns), row_loss_out [rows].
 * status bit 0: an action outside [0, n_actions); that row has no term (row_loss_out 0), a zero gradient and is not
 * counted.  Columns [n_actions, ld) of every output are not written.  1 <= rows <= 1024, 1 <= n_actions <= 18. */
int rlx_classification_head_loss(const float *logits, long long ld, const int *actions, const float *labels,
                                 long long ld_labels, float grad_scale, int rows, int n_actions, float *dlogits,
                                 long long ld_dlogits, float *probs_out, long long ld_probs, float *row_loss_out,
                                 float *scalars, int *status, void *stream);
/* DDQNBCQAgent.select_actions, NNImitationModelParameters branch, up to its argmax (agents/ddqn_bcq_agent.py:115-133).
 * imitation [batch][ld_i] is the imitation model's output on the next states: its logits (familiarity = the softmax
 * above, hence the bits of the network's predict), or with RLX_IMITATION_INPUT_PROBS in flags the probabilities
 * themselves.  familiarity_out (optional, [batch][ld_f]) receives the familiarity.  sel_out[b][a] = q_next_online[b][a],
 * or -inf where familiarity[b][a] < threshold: an fp32 comparison, as numpy compares a float32 array with a Python
 * float (the host passes np.float32(mask_out_actions_threshold)); a NaN familiarity is not masked.  A row that keeps no
 * action gets rlx_bcq_masked_selector's draws on the same (seed, rank, event) — one definition,
 * csrc/bcq_selector_tail.hpp — and is counted in zero_rows_out (optional device int).  event is READ FROM DEVICE
 * MEMORY.  One workgroup: batch <= 1024, 1 <= n_actions <= 18. */
#define RLX_IMITATION_INPUT_PROBS 1
int rlx_bcq_imitation_selector(const float *q_next_online, long long ld_q, const float *imitation, long long ld_i,
                               float threshold, int flags, int batch, int n_actions, unsigned int seed,
                               unsigned int rank, const long long *event, float *sel_out, long long ld_sel,
                               float *familiarity_out, long long ld_f, int *zero_rows_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RLX_H */
