/* ranslice.h -- C ABI of libranslice.so, the MI355X-native batched RAN-slice simulator.
 *
 * The reference (jjalcaraz-upct/network-slicing) has no FFI: its boundary for this path is
 * the Python class surface gym_ran_slice.RanSlice.reset()/step() (reference
 * gym-ran_slice/gym_ran_slice/ran_slice.py:30-54) over NodeB.reset()/step()
 * (reference node_b.py:17-22, 59-91).  The entry points below are what a ctypes binding of
 * that surface needs; each cites the reference method it stands in for.  All pointers are
 * plain host pointers unless the name ends in _device; no torch types appear.
 *
 * Every function returns RS_OK (0) or a negative error code; rs_last_error() gives text.
 * A handle is bound to one HIP device and one stream and is not thread-safe.
 */
#ifndef RANSLICE_H
#define RANSLICE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_OK 0
#define RS_EINVAL (-1)    /* bad argument / action shape or sum (reference Q9: silently mis-slices) */
#define RS_EOVERFLOW (-2) /* a fixed capacity (UEs per slice, bursts per UE, mMTC queue) was exceeded */
#define RS_EHIP (-3)      /* HIP runtime error */
#define RS_ESTATE (-4)    /* call order error (e.g. step before reset / fading not loaded) */

#define RS_N_EMBB_VARS 10 /* reference scenario_creator.py:80-82 */
#define RS_N_MMTC_VARS 3  /* reference scenario_creator.py:92 */
#define RS_MAX_MCS 32
#define RS_MAX_SET 8
#define RS_N_TRACES 3 /* reference channel_models.py:29-33 */

/* Immutable description of one scenario.  Field values come from the reference's
 * module-level constants (scenario_creator.py:26-96,115-134; channel_models.py:21-27,
 * 268-270; schedulers.py:13; datasets/mcs_codeset.csv); the Python host fills it. */
typedef struct rs_config {
    int32_t n_envs;         /* independent env replicas simulated by this handle */
    int32_t n_prbs;         /* scenario_creator.py:26-50 */
    int32_t n_embb;         /* eMBB slices come first, then mMTC (scenario_creator.py:158-166) */
    int32_t n_mmtc;
    int32_t slots_per_step; /* scenario_creator.py:100 (50); 1 .. 63 (the per-step statistics of a task are packed) */
    int32_t max_ue;         /* capacity: UEs per eMBB slice (0 -> 32) */
    int32_t max_bursts;     /* capacity: VBR bursts running at once per UE (0 -> 16) */
    int32_t max_mtc_queue;  /* capacity: backlogged mMTC devices per slice (0 -> 1024) */
    double slot_length;     /* 1e-3 s */
    double penalty;         /* ran_slice.py:19 */
    /* eMBB traffic (scenario_creator.py:55-69) */
    double cbr_lambda, cbr_t_mean, cbr_bit_rate;
    double vbr_lambda, vbr_t_mean, vbr_p_size, vbr_b_size, vbr_b_rate;
    /* eMBB SLA (scenario_creator.py:71-78): cbr_th, cbr_prb, cbr_queue, vbr_th, vbr_prb, vbr_queue */
    double sla_embb[6];
    /* normalisation of the 10 eMBB state variables, in state order (scenario_creator.py:115-126) */
    double norm_embb[RS_N_EMBB_VARS];
    /* mMTC (scenario_creator.py:86-96,130-134) */
    int32_t mtc_n_devices;
    int32_t mtc_n_rep, mtc_n_period;
    int32_t mtc_rep_set[RS_MAX_SET];
    int32_t mtc_period_set[RS_MAX_SET];
    double sla_mtc_delay;
    double norm_mmtc[RS_N_MMTC_VARS]; /* devices, avg_rep, delay */
    /* propagation (channel_models.py:84-97,121-124): L = A + B log10(R) */
    double prop_A, prop_B;
    /* proportional-fair scheduler (schedulers.py:13) */
    int32_t pf_granularity, pf_window, sym_per_prb;
    /* MCS table (datasets/mcs_codeset.csv; channel_models.py:260-270) */
    int32_t n_mcs;
    double mcs_rate[RS_MAX_MCS];
    double mcs_snr[RS_MAX_MCS];
    int32_t mcs_order[RS_MAX_MCS];
    int32_t mcs_mod[RS_MAX_MCS]; /* 0 qpsk, 1 16qam, 2 64qam */
    double mi_x0[3], mi_k[3];    /* mutual-information sigmoid parameters per modulation */
    /* create_env(..., L1_level) (scenario_creator.py:156-177).  0 = L1_level=True: one L1 slice per RAN slice, the
     * action has n_embb + n_mmtc entries.  1 = L1_level=False: the eMBB RAN slices share ONE L1 slice (one UE list,
     * one PF scheduler, one PRB range) and the mMTC RAN slices ONE FIFO; the action has one entry per L1 slice
     * ((n_embb > 0) + (n_mmtc > 0)), labels/violations likewise (violations = RAN slices in breach), the observation
     * and rs_get_info keep one block per RAN slice; UE capacity is 64 per L1 slice. */
    int32_t l1_multiplex;
    int32_t reserved_;
} rs_config;

typedef struct rs_handle rs_handle;

/* per-slot, per-UE record for bit-exact allocation checks (debug / parity only) */
typedef struct rs_alloc_rec {
    int32_t serial; /* arrival serial of the UE inside its slice, >= 1; 0 = empty entry */
    int32_t type;   /* 0 CBR, 1 VBR */
    int32_t e_snr;  /* UE.e_snr after the slot (slice_ran.py:45) */
    int32_t prbs;   /* UE.prbs after the slot (schedulers.py:68) */
    int64_t bits;   /* UE.bits after transmission_step (slice_ran.py:51-55) */
    double queue;   /* UE.queue after the slot */
    double th;      /* UE.th after the slot */
    double p;       /* UE.p, reception probability of this slot's allocation (0 if none) */
} rs_alloc_rec;

/* Build the simulator for cfg->n_envs replicas on HIP device `device`.
 * Stands in for scenario_creator.create_env (scenario_creator.py:100-183) minus file I/O. */
int rs_create(const rs_config* cfg, int device, rs_handle** out);

/* Upload fading trace `trace_id` (0..2), given in the reference's CSV layout: row-major
 * [rows = PRB][cols = time], dB, NaN allowed.  Rows are wrapped up to n_prbs as in
 * SINRSelectiveFading.__init__ (channel_models.py:141-150).  Data is copied. */
int rs_load_fading(rs_handle* h, int trace_id, const double* data, int rows, int cols);

/* RanSlice.reset()/NodeB.reset() (ran_slice.py:30-36, node_b.py:17-22) for every replica.
 * seeds[n_envs]: one 64-bit stream seed per replica (Evaluator.evaluate's default_rng(seed=i),
 * experiments_kbrl.py:46).  obs (may be NULL) receives zeros [n_envs][n_vars]. */
int rs_reset(rs_handle* h, const uint64_t* seeds, float* obs);

/* RanSlice.step(action) for every replica (ran_slice.py:38-54, node_b.py:59-91).
 * actions [n_envs][n_slices] PRBs per slice; must be >= 0 with row sums <= n_prbs.
 * Outputs (any may be NULL): obs f32 [n_envs][n_vars]; reward f64 [n_envs];
 * labels i32 [n_envs][n_slices] (+1/-1, node_b.py:51-57); violations i32 [n_envs][n_slices]. */
int rs_step(rs_handle* h, const int32_t* actions, float* obs, double* reward, int32_t* labels,
            int32_t* violations);

/* Same step, but actions are already resident in the handle's device action buffer
 * (filled by rs_random_actions) and nothing is copied back: the timed path of bench.py. */
int rs_step_resident(rs_handle* h);

/* Fill the device action buffer with i.i.d. multinomial(n_prbs; 1/(S+1) per slice and one
 * "unused" bin) draws per replica, from Philox stream (seed, step_index).  Used by bench.py
 *  and reproduced by the oracle for the CPU baseline. */
int rs_random_actions(rs_handle* h, uint64_t seed, uint64_t step_index);

/* Copy the results of the last step (resident or not) to host buffers (any may be NULL). */
int rs_fetch(rs_handle* h, int32_t* actions, float* obs, double* reward, int32_t* labels,
             int32_t* violations);

/* info['l1_info'] accumulators of the last step (node_b.py:46-49): f64 [n_envs][n_slices][10]
 * (eMBB: cbr_traffic, cbr_th, cbr_prb, cbr_queue, cbr_snr, vbr_...; mMTC: delay, avg_rep,
 * devices, rest 0). */
int rs_get_info(rs_handle* h, double* info);

/* n_steps x { rs_random_actions(seed, step_index0 + i); rs_step_resident(); } enqueued by one call.  With
 * use_graph != 0 the loop body is captured once as a hipGraph (two consecutive steps) and replayed; the slot
 * clock and the script index live in device memory, so results are identical with and without the graph. */
int rs_run_random(rs_handle* h, uint64_t seed, uint64_t step_index0, int n_steps, int use_graph);

/* Enable (capacity > 0) or disable per-slot allocation tracing.  When enabled every step
 * records [n_envs][n_embb][slots_per_step][max_ue] rs_alloc_rec entries. */
int rs_set_alloc_trace(rs_handle* h, int enable);
int rs_get_alloc_trace(rs_handle* h, rs_alloc_rec* out);

/* Counters maintained by the step kernels since the last rs_reset: [0] = sum over replicas,
 * slots, eMBB slices of n_ue * n_prbs (fading samples read; SURVEY.md §8d algorithmic bytes),
 * [1] = env-steps executed, [2] = PF loop iterations, [3] = UE-slots. */
int rs_get_counters(rs_handle* h, uint64_t counters[4]);

/* The reception step (slice_l1.py:219-224: `rng.random() < mcs_codeset.response(mcs, snr)`, channel_models.py:297-313) is
 * decided without forming the probability whenever a float32 evaluation of both sides leaves no doubt (rs_embb.hip:
 * fast_sigmoid; the outcome is the exact comparison's in every case).  Since the last rs_reset, per-slice step kernels
 * without allocation tracing: out[0] = reception tests, out[1] = those that evaluated the exact probability, out[2] = 1 if
 * the short test is available for this configuration (mcsA > 0, every MI slope k > 0, 1 <= mcsA / k <= 1e4).  The two counts
 * share one 64-bit word per task (32 bits each: they wrap after ~2e7 steps of one task). */
int rs_get_rx_stats(rs_handle* h, uint64_t out[3]);

/* Average device time of the dominant step kernel over the launches since the last call,
 * measured with HIP events on the handle's stream (bench.py roofline leg). */
int rs_kernel_time_ms(rs_handle* h, double* avg_ms, int64_t* launches);
/* The same with the spread: out = {mean, min, max} ms over those launches (a 20-step driver run rests on 20 of them). */
int rs_kernel_time_stats_ms(rs_handle* h, double out[3], int64_t* launches);
int rs_set_kernel_timing(rs_handle* h, int enable);

/* Lanes of the step loop.  A lane is a contiguous range of replicas with a stream of its own.  rs_random_actions opens a
 * handle whose mode engages lanes; until another entry point closes it, rs_random_actions / rs_step_resident (and the loop of
 * rs_run_random without a graph) enqueue every lane's launches on the lane's stream and do NOT join the lanes between steps,
 * so one lane's last waves run under another lane's launch.  Every other function that takes the handle first makes h's stream
 * wait for all lanes; results, counters and the saved state are those of a single-lane handle, bit for bit.
 * n = 0 (default): automatic -- per-slice L1, no mMTC slices, no allocation trace, 16 lanes per task, an ordered launch,
 * between one round of waves (4 tasks x SIMDs of the device) and the split step's 49,152 tasks: two lanes (DESIGN.md
 * section 4; every other handle: one).  n = 1: off.  n >= 2: that many lanes (at most 8, at most one per
 * replica) wherever the first three conditions hold; RS_EINVAL on multiplexed handles and handles with mMTC slices. */
int rs_set_lanes(rs_handle* h, int n);
/* Kernel timing with lanes: the sample of a step (rs_kernel_time_ms, rs_kernel_time_stats_ms) is the SUM of its lanes' bracketed
 * launch durations -- what a kernel trace adds up; overlapped launches each run longer, so the sum can only understate a
 * roofline fraction derived from it.  rs_get_lane_info, over the window rs_kernel_time_stats_ms drained last (or the pairs not
 * drained yet): out[0] = lanes in use, out[1] = sum of the lanes' launch durations per step (ms), out[2] = length of the union of
 * all bracketed intervals of the window / steps (ms), out[3] = 1 - union / sum, the share of step-kernel time that ran under
 * another lane's launch.  Timestamps are hipEventElapsedTime against one reference event (rs_set_kernel_timing records it). */
int rs_get_lane_info(rs_handle* h, double out[4]);

/* Lanes per (replica, eMBB slice) task in the primary step launch: 8, 16 or 32 (default: 32 up to 6144 tasks,
 * 16 above).  Tasks that need
 * more UE lanes are replayed by the 32-lane instance; results are identical for every setting. */
int rs_set_group_size(rs_handle* h, int lanes);

/* Scheduling hint.  mode 1: allocations come from a learning agent (the carrier is concentrated on few, wide slices);
 * the 16-lane step uses its BLOCK instance, which hands out the RB pairs of wide contested slices in block rounds
 * (every backlogged UE steps ahead in parallel) instead of one leader run at a time.  mode 0: the plain instance
 * (trip loop only; faster on the 30-50-RB slices of an even split).  mode < 0 (default): automatic -- rs_step looks at
 * the allocations it is handed, kb_step_resident asks for the BLOCK instance for the environment it drives, the
 * on-device random script goes by its average slice width.  Results do not depend on it (both are exact against the
 * reference loop, tests/test_gpu_parity.py::test_block_round_allocations). */
int rs_set_schedule_hint(rs_handle* h, int mode);

/* Developer aid: cycle sums per code section of the eMBB step kernel (zeros in normal builds). */
int rs_get_section_profile(rs_handle* h, uint64_t out[16]);
/* Developer aid (profile builds): per eMBB task [n_envs * n_embb][4] = cycles of the task's wave in the last step,
 * UEs and RBs at its start, contested PF loop trips; then 16 more values: the section cycle sums of the slowest
 * wave seen so far (out must hold 4 * n_tasks + 16 values). */
int rs_get_task_profile(rs_handle* h, uint64_t* out);

int rs_synchronize(rs_handle* h);
/* HIP devices visible to this process, or RS_EHIP */
int rs_device_count(void);
/* Free and total bytes of a device's memory (hipMemGetInfo), e.g. to size kb_config.pool_bytes. */
int rs_device_mem_info(int device, uint64_t* free_bytes, uint64_t* total_bytes);
int rs_n_vars(const rs_handle* h);
/* Checkpoint / restore (no reference counterpart: a run of experiments_kbrl.py that dies starts over).  The state of a handle
 * -- every device array behind it except the tables (fading traces, constants), plus its slot clock -- as one blob of
 * rs_state_bytes bytes; rs_load_state accepts a blob saved by a handle of the same configuration, on any device.  Loading
 * and stepping on reproduces the steps the saving handle would have made, bit for bit. */
int rs_state_bytes(rs_handle* h, uint64_t* bytes);
int rs_save_state(rs_handle* h, void* blob, uint64_t bytes);
int rs_load_state(rs_handle* h, const void* blob, uint64_t bytes);
/* Replica fork (no reference counterpart).  dst replica j := src replica src_index[j] (host array of dst->n_envs entries,
 * 0 <= index < src->n_envs, repeats allowed).  Same rs_config except n_envs; same device; identical fading tables; src must be
 * reset.  dst takes src's slot clock and becomes reset.  Stepping dst replica j with action a gives, bit for bit, what stepping
 * src replica src_index[j] with a would give (every draw is keyed by the replica's seed and counters in its state, never by its
 * index in the batch).  Copied per replica: the simulator state (per-task and per-UE arrays, VBR bursts, seed, sticky error
 * flags; the mMTC tables and queues) and the outputs of the last step.  Not copied: the per-task scheduling key and the
 * diagnostic counters (dst's restart, as after rs_reset); no result depends on either.  Ordered after src's queued work, and
 * src's later work after the copy; no host synchronisation.  RS_EINVAL: configurations differ or an index is out of range;
 * RS_ESTATE: src not reset, fading tables not identical, or different devices. */
int rs_fork(rs_handle* dst, rs_handle* src, const int32_t* src_index);
/* Lookahead capacity: up to max_branches forked replicas per search launch (at least n_prbs + 1; the library owns the branch
 * handle, created lazily with h's configuration and reading h's fading tables).  0 frees it. */
int rs_set_lookahead(rs_handle* h, int max_branches);
/* One step of every replica under the clairvoyant rule (no reference code; DESIGN.md section "Clairvoyant baseline"): for
 * each replica the action entries are decided in order s = 0 .. n_act-1; entry s takes the candidate k in [0, R_s],
 * R_s = n_prbs - (a_0 + ... + a_{s-1}), that minimises (violations[s], k) lexicographically, where violations[s] is what
 * one step of a fork of the replica gives under the action (a_0 .. a_{s-1}, k, 0 .. 0).  So it is the smallest k that meets
 * the SLA when one does, else the cheapest among the least-violating.  Then the replica steps for real with
 * (a_0 .. a_{n_act-1}).  actions_out [n_envs][n_act] (may be NULL) receives the chosen allocation; the other outputs are
 * rs_step's.  RS_EOVERFLOW also when a capacity was exceeded in one of a replica's branches; RS_ESTATE without lookahead
 * capacity (rs_set_lookahead) or before rs_reset. */
int rs_step_clairvoyant(rs_handle* h, int32_t* actions_out, float* obs, double* reward, int32_t* labels,
                        int32_t* violations);
/* The rule's second key when no candidate of a slice meets its SLA (a slice with a feasible candidate always takes the
 * smallest feasible k).  mode 0 (default): the cheapest among the least-violating, as above.  mode 1 ("widest"): the largest
 * among the least-violating -- a slice that cannot be served within one step gets what is left instead of nothing (the
 * default starves an mMTC slice whose backlog is already too old for one step to fix, until its queue overflows). */
int rs_set_clairvoyant_fallback(rs_handle* h, int mode);
int rs_n_slices(const rs_handle* h);
/* ---- device-resident policy interface (no reference counterpart; DESIGN.md section "Device-resident policy interface").
 * A policy that runs on the same GPU -- a torch module, a kernel of the caller's -- hands its actions over as a device pointer
 * and reads the outputs of the step in place: no host copy, no host wait.  Action kinds of rs_step_device: */
#define RS_ACT_PRBS   0   /* int32 [n_envs][n_slices]      PRBs per slice, as rs_step takes them            */
#define RS_ACT_SHARES 1   /* float [n_envs][n_slices + 1]  ReportWrapper's simplex (wrapper.py:77-82)       */
#define RS_ACT_INDEX  2   /* int64 [n_envs]                row of the action table (DQNWrapper, wrapper.py:136-154) */

typedef struct rs_device_view {   /* device pointers owned by the handle, valid until rs_destroy */
    int32_t device, n_envs, n_slices, n_vars;
    void*    stream;              /* the handle's hipStream_t */
    /* inputs a caller may fill instead of bringing its own buffer */
    int32_t* in_prbs;  float* in_shares;  int64_t* in_index;
    /* the action the last step executed (= the buffer rs_step_resident reads) and its row sum */
    int32_t* actions;  int32_t* resources;          /* [n_envs][n_slices], [n_envs] */
    /* outputs of the last step */
    float*   obs;       float* obs_norm;            /* raw, and clip(obs,-0.5,1.5)-0.5 in float32 (wrapper.py:87-89) */
    double*  reward;    int32_t* labels;  int32_t* violations;  int32_t* total_violations;   /* [n_envs] */
    int64_t* rejected;                              /* one counter: action rows refused since rs_reset */
} rs_device_view;

/* The buffers behind the view that this interface adds (in_*, resources, obs_norm, total_violations, rejected), the action
 * table and the report histories are created by the first call of this group.  They are NOT part of a checkpoint
 * (rs_save_state / rs_load_state) and are NOT copied by rs_fork; resources, obs_norm and total_violations are written by
 * rs_step_device only (rs_step / rs_step_resident leave them as they are). */
int rs_get_device_view(rs_handle* h, rs_device_view* out);
/* RanSlice.step for every replica, the actions read from device memory.
 * Input and stream ordering.  actions_device: any device pointer on the handle's device -- one of the view's in_* buffers or
 * the caller's own (a torch tensor's data_ptr()), laid out as `kind` says, C-contiguous.  caller_stream: the hipStream_t the
 * caller produced the actions on and will consume the outputs on; NULL is the null stream (torch's default stream).  The call
 * records an event on caller_stream, the handle's stream waits for it; then the rows are decoded and validated, the replicas
 * step, the outputs are post-processed; an event recorded after everything the step queued (the side streams the step forks
 * and joins included) is waited for by caller_stream.  With caller_stream == the handle's own stream both events are skipped.
 * THE HOST WAITS FOR NOTHING AND NOTHING IS COPIED TO OR FROM THE HOST: the outputs stay in the view's buffers.
 * Decoding.  RS_ACT_PRBS: the row as it is.  RS_ACT_SHARES: PRBs_i = floor((n_prbs * |a_i|) / t), t = sum |a| over all
 * n_slices + 1 entries, t = 1 when that sum is 0, in float64 on the float32 inputs widened exactly and with the row sum taken
 * in the order numpy takes it over a contiguous axis (left to right below 8 entries; for 8 and 9 entries
 * ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7)), then + a8): bit-equal to ranslice.report.simplex_to_prbs on the same C-contiguous
 * float32 array.  RS_ACT_INDEX: the row is table[idx] (rs_set_action_table).
 * Validation, on the device (rs_step does it on the host and returns RS_EINVAL).  A row with a negative entry, a sum above
 * n_prbs, an index outside the table, or shares without an integer image (NaN, infinite) is REFUSED: it is replaced by all
 * zeros, *rejected is incremented, and the replica steps with the zero allocation exactly as rs_step would with a zero row.
 * A refused row is never silently mis-sliced.  Capacity overflows stay sticky in the state's error words as ever and surface
 * at the next rs_fetch (RS_EOVERFLOW).
 * Schedule hint.  In automatic mode the step-kernel instance is the on-device script's (rs_set_schedule_hint); results do
 * not depend on it.
 * Outputs.  Besides rs_step_resident's (obs, reward, labels, violations, l1_info): resources (row sums of the executed
 * action), obs_norm, total_violations; and, when a report history is open and its cursor is below `steps`, one column of it.
 * RS_ESTATE before rs_reset, and for RS_ACT_INDEX without a table; RS_EINVAL for an unknown kind. */
int rs_step_device(rs_handle* h, int kind, const void* actions_device, void* caller_stream);
/* caller_stream waits for everything queued on the handle so far (e.g. after rs_reset, before reading the view on it) */
int rs_stream_join(rs_handle* h, void* caller_stream);
/* The action table of RS_ACT_INDEX: host array [n_actions][n_slices] (n_slices = rs_n_slices(h): one entry per L1 slice on an
 * L1-multiplexed handle; the width is implied, so a binding that knows the table's shape must refuse any other width --
 * ranslice.vec_env raises ValueError).  Copied to the device; waits for the steps in flight.  Rows are validated when used. */
int rs_set_action_table(rs_handle* h, const int32_t* table /* host [n_actions][n_slices] */, int32_t n_actions);
/* The histories of ReportWrapper (wrapper.py:54-57,106-109) kept on the device, like kb_history_begin: violation int16,
 * reward f64, resources int16, [n_envs][steps], zeroed.  Every rs_step_device advances a cursor that lives in device memory
 * and records column `cursor` while cursor < steps.  rs_reset takes the cursor back to 0 and keeps the columns, as
 * ReportWrapper.reset does.  rs_report_extend is set_evaluation (wrapper.py:125-130): cursor := steps, steps += eval_steps,
 * the new columns zero.  rs_report_fetch copies the arrays (any may be NULL) and min(cursor, steps) to the host and waits. */
int rs_report_begin(rs_handle* h, int32_t steps);
int rs_report_extend(rs_handle* h, int32_t eval_steps);
int rs_report_fetch(rs_handle* h, int16_t* violation, double* reward, int16_t* resources, int32_t* n_recorded);  /* [n_envs][steps] */
/* Copy between host memory and device memory of the handle's device, on the handle's stream: ordered after the steps queued so
 * far.  to_device == 0: device -> host, and the call waits for the copy; otherwise host -> device, without waiting for the
 * device (the host buffer may be reused when the call returns). */
int rs_device_copy(rs_handle* h, void* dst, const void* src, uint64_t bytes, int to_device);
const char* rs_last_error(const rs_handle* h);
void rs_destroy(rs_handle* h);


/* ------------------------------------------------------------------------------------------
 * KBRL agent (hot path B).  Stands in for kbrl_control.KBRL_Control over
 * algorithms.projectron.Projectron(GaussianKernel(SVvariable)) (reference kbrl_control.py:23-114,
 * algorithms/projectron.py:23-64, algorithms/kernel.py:3-34), one independent agent per replica.
 * ------------------------------------------------------------------------------------------ */
#define KB_MAX_SLICES 8
#define KB_CAPACITY_MAX 65536

typedef struct kb_config {
    int32_t n_envs;               /* agents (one per env replica) */
    int32_t n_slices;             /* learners per agent */
    int32_t n_prbs;               /* <= 255: the candidates 0 .. n_prbs of a learner fill four 64-lane groups (rs_create takes carriers
                                     of up to 256 PRBs; an agent for a 256-PRB carrier is refused by kb_create with RS_EINVAL) */
    int32_t capacity;             /* most landmarks a dictionary may hold (<= KB_CAPACITY_MAX); storage is taken from the
                                     pool 64 landmarks at a time as dictionaries grow, so this is a limit, not a reservation */
    int32_t dims[KB_MAX_SLICES];  /* state variables of learner s: 10 eMBB / 3 mMTC (scenario_creator.py:209-235) */
    double alfa;                  /* scenario_creator.py:187 */
    double acc_lo, acc_hi;        /* accuracy_range */
    double gamma, eta;            /* scenario_creator.py:218, projectron.py:25 */
    int32_t shared_dictionary;    /* 0: one agent per replica (the reference); 1: one dictionary per slice shared by all
                                     replicas (build-defined extension) */
    int32_t first_env;            /* shared mode: global id of this handle's replica 0 (rank * n_envs) */
    int64_t pool_bytes;           /* device memory all dictionaries of the handle grow in (landmarks, coefficients, Kinv:
                                     SVvariable / Projectron.Kinv, projectron.py:3-30, which the reference grows without
                                     bound).  0: the smallest of every dictionary at its capacity, 1 GB + 2 MB per
                                     dictionary, and half of the free device memory */
} kb_config;

typedef struct kb_handle kb_handle;

int kb_create(const kb_config* cfg, int device, kb_handle** out);
void kb_destroy(kb_handle* k);
const char* kb_last_error(const kb_handle* k);
/* KBRL_Control.__init__ state (kbrl_control.py:28-39): initial_action / security_factor [n_envs][S];
 * seeds[n_envs] feed the tie-break stream of GaussianKernel.predict (kernel.py:26-27).  Also clears the hits of the last
 * learning step, which an inference-mode history column repeats (kb_set_learning): "none yet" reads as zeros.  RS_ESTATE on
 * an inference-only handle (kb_deploy). */
int kb_reset(kb_handle* k, const int32_t* initial_action, const int32_t* security_factor, const uint64_t* seeds);
/* KBRL_Control.update_control(state, action, labels) -> hits (kbrl_control.py:80-114), all agents */
int kb_update_control(kb_handle* k, const float* state, const int32_t* action, const int32_t* labels, int32_t* hits);
/* KBRL_Control.select_action(state) -> (action, adjusted) (kbrl_control.py:41-78), all agents */
int kb_select_action(kb_handle* k, const float* state, int32_t* action, int32_t* adjusted);
/* One closed-loop agent step entirely on the device (KBRL_Control.run body, kbrl_control.py:129-134):
 * update_control(previous obs, the action just executed by `env`, its SLA labels) followed by
 * select_action(new obs); the selected action is written into env's device action buffer. */
int kb_step_resident(kb_handle* k, rs_handle* env);
/* n_steps of that loop body followed each by the simulator's step -- n x (kb_step_resident(k, env); rs_step_resident(env)) --
 * enqueued by one call; with use_graph two consecutive steps are captured once into a hipGraph and replayed (one graph launch
 * per two steps instead of ~50 kernel launches).  Identical results either way. */
int kb_run_resident(kb_handle* k, rs_handle* env, int n_steps, int use_graph);
/* Projectron.predict(x) / update(x, y) on learner `s` of agent `e` (projectron.py:32-60).
 * branch: 0 none, 1 projection, 2 dictionary grew. */
int kb_predict(kb_handle* k, int e, int s, const double* x, int32_t* y_pred, double* f);
int kb_update(kb_handle* k, int e, int s, const double* x, int32_t y, int32_t* branch, double* delta);
/* GaussianKernel.k(x) (kernel.py:13-20) of the last kb_predict on learner (e, s): its kernel row, m entries (the third
 * return value of GaussianKernel.predict, kernel.py:28).  row may be NULL to ask for m only. */
int kb_get_kernel_row(kb_handle* k, int e, int s, int32_t* m, double* row);
/* Dictionary of learner (e, s): m landmarks [m][dims+1], coeff [m], Kinv [m][m] (any may be NULL) */
int kb_get_learner(kb_handle* k, int e, int s, int32_t* m, double* landmarks, double* coeff, double* kinv);
/* margins / security_factors / current action [n_envs][S], adjusted [n_envs], accuracies [n_envs][S][n_prbs] */
int kb_get_control(kb_handle* k, int32_t* margins, int32_t* security, int32_t* action, int32_t* adjusted,
                   double* accuracies);
int kb_set_adjusted(kb_handle* k, const int32_t* adjusted);
/* ---- shared-dictionary mode (kb_config.shared_dictionary = 1).  One learning step = round 0, 1, ...:
 *   kb_shared_scan   every replica looks for its first mistake (augmentation order, kbrl_control.py:103-112)
 *                    against the frozen shared dictionaries; round 0 also does update_control's bookkeeping
 *                    (hits, accuracies, security factors) and needs state/action/labels (later rounds: NULL).
 *                    counts[S] = local proposers per slice; props[S][budget][KB_PROP_WIDTH] = the first
 *                    `budget` of them in replica order (global replica id, packed candidate/label, state).
 *   (caller)         all-gather props/counts over RCCL, merge by global replica id, keep the first `budget`.
 *   kb_shared_apply  apply a merged list (same on every rank) in order through Projectron.predict/update.
 *   kb_shared_commit n_accept[S] = how many of this handle's proposers (in replica order) were in the merged
 *                    list: they move on to their next candidate; the others propose again next round. */
#define KB_PROP_WIDTH 18
int kb_shared_scan(kb_handle* k, const float* state, const int32_t* action, const int32_t* labels, int32_t round,
                   int32_t budget, int32_t* hits, int32_t* counts, double* props);
int kb_shared_apply(kb_handle* k, const int32_t* counts, const double* props, int32_t budget);
int kb_shared_commit(kb_handle* k, const int32_t* n_accept);

/* The same learning step with the exchange kept on the device: every round scans, packs this rank's proposals,
 * all-gathers the blocks of all ranks with ncclAllGather (RCCL, bound at run time, on the agent's stream), merges by
 * global replica id, applies and commits -- until no rank proposes anything or max_rounds rounds were made
 * (rounds_out).  Only a 4-byte "anything left" flag per round returns to the host.  kb_comm_unique_id: 128 bytes
 * from ncclGetUniqueId, generated by ONE rank and handed to the others by the launcher; kb_comm_init joins the
 * communicator (rank = the handle's index among the `world` agents that share their dictionaries; kb_config.first_env
 * must be rank * n_envs).  Without kb_comm_init the handle is its own world (no RCCL needed).
 * Every rank of a group must have set the same kb_set_shared_plus value (below) before the same step: the rule the merged
 * list is applied by is host state of each handle and nothing checks it across ranks. */
int kb_comm_unique_id(void* id128);
int kb_comm_init(kb_handle* k, const void* id128, int rank, int world);
/* What the live communicator itself reports (ncclCommUserRank / ncclCommCount); (0, 1) for a handle that never joined one.
 * After the communicator was aborted (a failed or timed-out exchange: kb_shared_step returned RS_EHIP) this and every
 * shared step return RS_ESTATE until kb_comm_init joins a new one -- the handle does not quietly become a world of its own. */
int kb_comm_info(kb_handle* k, int* rank, int* world);
int kb_shared_step(kb_handle* k, const float* state, const int32_t* action, const int32_t* labels, int32_t budget,
                   int32_t max_rounds, int32_t* hits, int32_t* rounds_out);
/* kb_step_resident for a shared-dictionary agent: the learning step above on the simulator's own device buffers (previous
 * observation, the action `env` just executed, its labels), then select_action of the new observation into the
 * simulator's action buffer.  Only the per-round "anything left" flag crosses PCIe; with rounds_out == NULL the host
 * does not wait for the last permitted round's flag either (the whole step is enqueued and the call returns). */
int kb_shared_step_resident(kb_handle* k, rs_handle* env, int32_t budget, int32_t max_rounds, int32_t* rounds_out);
/* The merge of kb_shared_step on a caller-supplied gathered buffer (what ncclAllGather delivers): `world` blocks of
 * [S proposer counts][S][budget][KB_PROP_WIDTH] doubles -> merged proposals [S][budget][KB_PROP_WIDTH], their counts [S],
 * how many of rank `me`'s made it [S], and the proposers of all ranks.  Lets a single process check the device merge
 * for any world size against the host rule (ranslice.kbrl_dev.merge_proposals). */
int kb_shared_merge(kb_handle* k, const double* gathered, int32_t world, int32_t me, int32_t budget, double* merged,
                    int32_t* counts, int32_t* taken, int32_t* total);

/* Histories of KBRL_Control.run (kbrl_control.py:119-124,135-141) kept on the device: after kb_history_begin(steps)
 * every kb_step_resident records one column per replica -- reward f64, resources (sum of the newly selected action),
 * hits [S], adjusted, SLA (sum of labels), violation (total), all int16 as in the reference -- so a whole run needs no
 * per-step read-back.  kb_history_fetch: [n_envs][steps] arrays (hits [n_envs][S][steps]) and the columns recorded. */
int kb_history_begin(kb_handle* k, int32_t steps);
int kb_history_fetch(kb_handle* k, double* reward, int16_t* resources, int16_t* hits, int16_t* adjusted, int16_t* sla,
                     int16_t* violation, int32_t* n_recorded);

/* sums over learners since kb_reset: [0] predicts, [1] mistakes, [2] insertions, [3] kernel evaluations */
int kb_get_stats(kb_handle* k, uint64_t stats[4]);
/* landmarks in every dictionary: i32 [n_envs][S] (one agent per replica) or [S] (shared dictionaries) */
int kb_get_sizes(kb_handle* k, int32_t* m);
/* the dictionary pool: bytes in use / in total, replicas with a dictionary at its capacity, replicas that found the pool
 * exhausted (both keep learning by projection -- build-defined, the reference's SVvariable is unbounded; any may be NULL) */
int kb_get_pool(kb_handle* k, uint64_t* used_bytes, uint64_t* total_bytes, int32_t* n_saturated, int32_t* n_pool_full);
/* per-replica flag words [n_envs] behind kb_get_pool's counts: bit 8 a dictionary of the replica reached its capacity, bit 16
 * it found the pool exhausted, bit 32 the budget stage of the loop (kb_set_online_prune) met a dictionary of the replica whose
 * Kinv diagonal is not finite and positive, or whose coefficient is not finite, and left it unpruned.  All three are sticky,
 * travel with the agent as the word does (kb_fork, checkpoints, agent files), and none is an error to kb_synchronize */
int kb_get_flags(kb_handle* k, int32_t* flags);
/* bytes behind the repair rounds of the large dictionaries since kb_reset (projectron.py:42 Kinv @ K_f, :54-58 the rank-1
 * update), as their kernels count them: work[0] tiles of Kinv the mat-vec kernel read (32,768 bytes each), work[1] units of
 * the rank-1 kernel (8,192 bytes read + 8,192 written each), work[2] / work[3] launches of either that had work; work[4] scoring passes that
 * evaluated landmarks' exponentials one by one (outlier states, off-grid landmarks), work[5] the landmarks they evaluated --
 * both counted by developer builds only (-DKB_COUNT_DIRECT), 0 otherwise; work[6] the samples that ran the mat-vec in the closed
 * loop's Projectron++ mode (kb_set_control_plus: branches 1-4 of its candidates) -- that mode queues no repair, so work[0..3] stay
 * as they are while it runs; on a shared-dictionary handle under kb_set_shared_plus the proposals whose branch was 1-4 */
int kb_get_repair_work(kb_handle* k, uint64_t work[8]);
int kb_kernel_time_ms(kb_handle* k, double* avg_ms, int64_t* launches);
/* the same per phase: ms[0] / n[0] the update phase (update_control_kernel and its repair kernels; shared mode: the scan
 * kernels), ms[1] / n[1] select_kernel */
int kb_phase_times_ms(kb_handle* k, double ms[2], int64_t n[2]);
int kb_set_kernel_timing(kb_handle* k, int enable);
/* mean duration of one launch of the two kernels that stream Kinv in the repair rounds -- ms[0] / n[0] the mat-vec, ms[1] /
 * n[1] the rank-1 update -- over the span the last kb_phase_times_ms call covered (for their HBM roofline) */
int kb_repair_times_ms(kb_handle* k, double ms[2], int64_t n[2]);
/* the same for every kernel that has a roofline entry of its own in the bench record: mean duration of ONE launch over that
 * span -- [2] heavy_matvec_kernel, [3] heavy_rank1_kernel, [4] the binning pass of select_action (select_bin_kernel alone, or select_bin_big_kernel + select_bin_kernel + big_list_kernel once large learners are listed), [5] heavy_finish_kernel, [6] select_gemm_kernel,
 * [7] update_small_kernel; [0], [1] repeat the two phases of kb_phase_times_ms */
int kb_kernel_times_ms(kb_handle* k, double ms[8], int64_t n[8]);
/* Checkpoint / restore of the agents: the per-learner tables, the control state, the part of the dictionary pool in use and
 * the recorded histories, as one blob (kb_state_bytes waits for the stream and sizes it); kb_load_state takes a blob saved by
 * a handle of the same configuration whose dictionaries fit this handle's pool.  The flag words travel with the agents; "the
 * pool was exhausted" (bit 16) is dropped only when this handle's pool is strictly larger than the one the blob came from. */
int kb_state_bytes(kb_handle* k, uint64_t* bytes);
int kb_save_state(kb_handle* k, void* blob, uint64_t bytes);
int kb_load_state(kb_handle* k, const void* blob, uint64_t bytes);
/* waits for the agent's stream and reports an internal error flag raised by any kernel since kb_reset (the
 * device-resident loop kb_step_resident does not check on its own); dictionaries at capacity are not errors (kb_get_pool) */
int kb_synchronize(kb_handle* k);

/* ---- agent fork and deployment (one agent per replica only: handles with shared_dictionary == 1 are out of scope and get
 * RS_EINVAL from all three calls).
 *
 * Device-side gather of agents: agent j of dst := agent src_index[j] of src (src_index: host array of dst->n_envs entries,
 * 0 <= index < src->n_envs, repeats allowed).  Same kb_config except n_envs and pool_bytes; same device; src must be reset.
 * dst's previous dictionaries are dropped as by kb_reset and dst becomes reset.  Copied per agent: every dictionary in full
 * (vector pages, Kinv tiles and their partial-sum areas), the per-dictionary tables (sizes, newest-landmark heads, the
 * off-grid / float32 marks, versions; the owner of the cached kernel row remapped to the new task id), the cached (f, m) of
 * the last kb_predict, the control state (action, security factors, margins, adjusted, accuracies), the tie-break stream
 * (seed and counters), the observation the resident loop chose its last action in, and the flag word VERBATIM (a source agent
 * that found its pool exhausted stays flagged in dst).  Restarted as after kb_reset: the statistics, the repair-work counters,
 * the launch-order lists and the stored select scores -- no result depends on any of them.  dst's pool layout is an exclusive
 * scan of the shell sizes in (dictionary, shell) order, so two forks with the same arguments give byte-identical kb_save_state
 * blobs.  Continuing dst agent j gives, bit for bit, what continuing src agent src_index[j] would.  Ordered after src's queued
 * work, and src's later work after the gather; the host waits once, for the scan's total.  RS_EINVAL: configurations differ,
 * an index out of range, a shared-dictionary handle; RS_ESTATE: src not reset, different devices, an inference-only handle on
 * either side; RS_EOVERFLOW: the dictionaries do not fit dst's pool -- dst is then left reset, with the control state of the
 * sources and empty dictionaries. */
int kb_fork(kb_handle* dst, kb_handle* src, const int32_t* src_index);
/* Creates an INFERENCE-ONLY handle of n agents, agent j := agent src_index[j] of src (a learning handle, or an inference-only
 * one: a deployed agent can be fanned out again).  Its dictionaries are the vector pages alone (landmarks, coefficients: 15,360
 * bytes per 64 landmarks; no Kinv), in a pool sized exactly -- 512 bytes + 15,360 x the shells of the chosen dictionaries --
 * which kb_get_pool reports.  Control state, tie-break stream and flags are copied as by kb_fork.  Learning is permanently
 * off: kb_step_resident / kb_run_resident / kb_select_action / kb_predict work; kb_update_control, kb_update,
 * kb_set_learning(k, 1), kb_get_learner with kinv != NULL, kb_save_state, kb_load_state, kb_fork and kb_reset (which would
 * empty dictionaries that can never be learned again) return RS_ESTATE. */
int kb_deploy(kb_handle* src, const int32_t* src_index, int32_t n, kb_handle** out);
/* kb_deploy BY REFERENCE: an inference-only handle of n replicas whose dictionaries are stored ONCE per distinct agent of
 * src_index (vector pages only; agents nobody names are not stored), read-only and shared by all the replicas that name the
 * agent.  Same arguments and checks as kb_deploy; src is a learning handle or a copy-deployed inference-only one.  Private per
 * replica, copied exactly as kb_deploy copies it: control state (action, security factors, margins, adjusted, accuracies),
 * tie-break stream (seed and counters), the observation the resident loop chose its last action in, the flag word verbatim;
 * history buffers (kb_history_begin) are the handle's own, per replica.  kb_get_pool reports the store: exactly 512 bytes +
 * 15,360 x the shells of the DISTINCT (agent, slice) dictionaries -- 30 agents fanned out onto 65,536 replicas cost 30
 * agents' landmarks, not 65,536.  Selection is one fused
 * kernel that scores up to sixteen replicas of an agent per pass over its landmarks and writes nothing into a dictionary's
 * page; every replica's scores, action, margin, tie draws and counters are bit for bit those of a kb_deploy handle given the
 * same src_index and states.  Works: kb_select_action, kb_step_resident, kb_run_resident (plain and hipGraph), kb_get_control,
 * kb_set_adjusted, kb_get_stats, kb_get_flags, kb_get_pool, kb_history_begin / kb_history_fetch, kb_get_sizes and
 * kb_get_learner with kinv == NULL (per replica, through the map), kb_synchronize, kb_destroy.  RS_ESTATE: everything a
 * kb_deploy handle refuses; kb_predict and kb_get_kernel_row (they would write a cached row into a shared page); kb_prune;
 * kb_deploy, kb_deploy_ref and kb_fork with the by-reference handle as source.  RS_EINVAL: a shared-dictionary src, an index
 * out of range, n <= 0.  Ordered as kb_deploy: after src's queued work, and src's later work after the gather. */
int kb_deploy_ref(kb_handle* src, const int32_t* src_index, int32_t n, kb_handle** out);
/* ---- agent files: trained agents leave the process in the form they are deployed in, and come back as inference-only handles.
 *
 * The file ("KBAGENT1", little-endian, every array 8-byte aligned; DESIGN.md §8e, ranslice/agent_file.py reads and writes the
 * same bytes on the host): a 120-byte header (magic, total bytes, FNV-1a of everything behind the hash field, agents n, and
 * n_slices, n_prbs, capacity, dims[8], alfa, acc_lo, acc_hi, gamma, eta of kb_config, then the doubles of all dictionaries
 * together); dense agent-major tables of what kb_fork copies per agent (sizes m[n][S], the float32 marks, action, security
 * factors, margins, adjusted, accuracies, seeds, tie-break counters, the observation the resident loop chose its last action
 * in, the flag word verbatim); then per dictionary, in (agent, slice) order, landmarks[m][dims[s] + 1] as f64 landmark-major
 * (the shape kb_get_learner returns) and coeff[m].  Slot j of the file is slot j of the dictionary.  No Kinv, no shell
 * offsets, no padding: landmarks, coefficients and control state -- what scoring reads.
 *
 * kb_export_bytes / kb_export_agents: agent j of the file := agent src_index[j] of src (repeats and permutations allowed).
 * Arguments and checks are kb_deploy's; src is a learning handle or a copy-deployed inference-only one.  The blob must be
 * exactly *bytes of kb_export_bytes long.  The file is a function of the arguments and the agents' state alone: two exports
 * give identical bytes, and so does the export of a handle imported from the file.  Nothing in src is written.  Ordered on
 * src's stream, after its queued work; the host waits once for the sizes in kb_export_bytes, and in kb_export_agents for the
 * scan's totals and for the copy.  RS_ESTATE: a by-reference handle (export from its source instead), src not reset.
 * RS_EINVAL: a shared-dictionary handle, an index out of range, n <= 0, `bytes` other than kb_export_bytes' (blob untouched).
 *
 * kb_agents_info: host only, no device call; the one function that parses untrusted bytes.  Validates a blob and returns the
 * configuration kb_import_agents would create (n_envs = the file's agents, pool_bytes = 512 + 15,360 x the started 64
 * landmarks of its dictionaries, shared_dictionary = 0) and, where m != NULL, the dictionary sizes [agents][S].  Checked, in
 * this order and each before anything behind it is read: the magic, the length against the header's, kb_create's limits
 * (<= 8 learners, n_prbs <= 255, 2 <= capacity <= 65536, dims <= 15), finite alfa, gamma, eta and accuracy range, the size the
 * header's own fields imply against `bytes`, the hash, 0 <= m <= capacity with the sizes adding up to the header's total, and
 * 0 <= action <= n_prbs.  RS_EINVAL otherwise; with no handle to hold the reason it is left in a per-thread string that
 * kb_last_error(NULL) returns (also after a failed kb_import_agents).
 *
 * kb_import_agents: runs kb_agents_info, then creates an inference-only handle on `device` that holds the file's agents in
 * file order, in a pool of exactly the pool_bytes above: an ordinary kb_deploy handle -- what works and what is refused is
 * that list, and kb_deploy / kb_deploy_ref fan it out.  Pages are written whole: coordinates, their float32 copy (dims == 10),
 * coefficients, the grid index of the last coordinate as an insertion computes it, zeros everywhere else and in every lane
 * from m on; the newest-landmark heads, the chain links and the off-grid counts are rebuilt; the float32 mark is recomputed
 * from the values and ORed with the file's.  Restarted as after kb_reset / kb_fork: statistics, stored select scores, the
 * cache of the last kb_predict, versions, retained hits -- no result depends on them, so every score, action, margin, tie
 * draw and counter is bit for bit that of kb_deploy(src, src_index) of the exported agents.  A coordinate or coefficient
 * that is not finite: RS_EINVAL.  On any failure *out stays NULL and nothing stays allocated. */
int kb_export_bytes(kb_handle* src, const int32_t* src_index, int32_t n, uint64_t* bytes);
int kb_export_agents(kb_handle* src, const int32_t* src_index, int32_t n, void* blob, uint64_t bytes);
int kb_agents_info(const void* blob, uint64_t bytes, kb_config* cfg, int32_t* m /* [agents][S], may be NULL */);
int kb_import_agents(const void* blob, uint64_t bytes, int device, kb_handle** out);
/* Device time (HIP events around the one launch) of the transposing kernel of this thread's last kb_export_agents (ms[0],
 * the pack) and kb_import_agents (ms[1], the build), and the bytes its work plan counts, read plus written: the pack reads
 * dims + 2 whole rows of every vector page and writes the file's dictionaries; the build reads those and writes whole pages. */
int kb_agents_kernel_times(double ms[2], uint64_t bytes[2]);
/* ---- resuming learning on agents that hold no Kinv (a kb_deploy handle, a kb_import_agents handle).
 *
 * kb_fork_rebuild: kb_fork for such sources -- agent j of dst := agent src_index[j] of src, and dst's Kinv is REBUILT on the
 * device.  dst: a learning handle (kb_create), same kb_config as src except n_envs and pool_bytes, same device.  src: a
 * copy-deployed inference-only handle, an imported one, or a learning handle (whose Kinv is then ignored).  Travels, as with
 * kb_fork: the vector pages (coordinates, their float32 copy, coefficients, grid index and chain links), sizes, heads, the
 * off-grid / float32 marks, versions, the control state, the tie-break stream, the observation the resident loop chose its last
 * action in, and the flag word verbatim.  Restarts: everything kb_fork restarts, and the cache of the last kb_predict (the
 * replay uses its rows: kb_update answers RS_ESTATE until a new kb_predict).  Layout: kb_fork's (full shells at an exclusive
 * scan of their sizes); Kinv tiles and their partial-sum areas are zeroed, then filled by replaying the insertions in slot
 * order -- step j inserts landmark j into the dictionary of landmarks 0 .. j - 1 with the arithmetic of Projectron.update's
 * insertion branch, statement for statement (the float32 roundings of the first pair included); coefficients, versions,
 * flags and chains are the copied ones and are not written.  Over landmarks that were never reordered (no kb_prune, not packed
 * on the host in another order) the result is the source's Kinv BIT FOR BIT, and continuing dst agent j gives, bit for bit,
 * what continuing the learning handle the agent came from would.  Over any other slot order the same recurrence yields the
 * landmarks' inverse Gram matrix to rounding.  Ordered as kb_fork, by events on both streams; never captured into a graph;
 * the host waits for the scan's total (and the sizes), and once for the result words.
 * RS_EINVAL: everything kb_fork returns it for.  RS_ESTATE: a by-reference handle on either side, src not reset, different
 * devices, an inference-only dst, or a step of the replay that met a delta that is not finite or not above zero (a host-packed
 * file with a repeated landmark): the other dictionaries finish, dst is then left reset with the sources' control state and
 * empty dictionaries, kb_get_rebuild still reports every min_delta and kb_last_error counts the dictionaries and names the
 * first.  RS_EOVERFLOW: the full shells do not fit dst's pool -- dst is left as kb_fork leaves it.
 * kb_get_rebuild: per dictionary of the last kb_fork_rebuild into k that replayed, the smallest delta met, [n_envs][S] (1.0
 * below two landmarks).  A min_delta at or below eta is legitimate: it says that the slot order is not one the Projectron
 * inserted in (the dictionary was pruned, or it is foreign), not that Kinv is wrong.  work, counted from the plan: [0] Kinv
 * tiles (32 KB + 1 KB of partial sums) read by the mat-vecs, [1] rank-1 units (8 KB read, 8 KB written), [2] rounds (steps
 * that ran chip-wide, beyond the first 192 of every dictionary), [3] dictionaries that hold a landmark.  RS_ESTATE: no replay
 * ran into k (never called, or the last call ended before it: a refusal, an overflow).
 * kb_rebuild_time_ms: with kb_set_kernel_timing on in dst at the call, device ms of the last call's replay (one pair of HIP
 * events around it, on dst's stream); 0 otherwise. */
int kb_fork_rebuild(kb_handle* dst, kb_handle* src, const int32_t* src_index);
int kb_get_rebuild(kb_handle* k, double* min_delta /* [n_envs][S] */, uint64_t work[4]);
int kb_rebuild_time_ms(kb_handle* k, double* ms);
/* ---- the bridge between shared-dictionary handles (kb_config.shared_dictionary = 1) and per-replica ones.
 * kb_fork, kb_deploy, kb_deploy_ref, kb_export_agents, kb_fork_rebuild, kb_prune and kb_set_learning keep refusing shared
 * handles; kb_unshare is the way to all of them, kb_share the way back.  The two storages differ in Kinv alone: a per-replica
 * dictionary keeps the lower block triangle and a partial-sum area per tile, a shared one both triangles.
 *
 * kb_unshare: agent j of dst receives a private copy of each of src's S dictionaries, and the control state of src's replica
 * src_index[j] (host array of dst->n_envs entries, 0 <= index < src->n_envs, repeats allowed).  src: a shared-dictionary handle,
 * reset.  dst: a per-replica LEARNING handle (kb_create), same kb_config as src except n_envs, pool_bytes, shared_dictionary,
 * first_env and capacity (every dictionary must fit dst's); same device.  Per dictionary: the vector pages whole (coordinates,
 * their float32 copy, coefficients, grid index and chain links), Kinv as the lower block triangle, copied tile for tile from
 * the full storage, the partial-sum areas zeroed (scratch that every mat-vec writes before it reads), and the sizes, heads,
 * off-grid / float32 marks and versions.  Per agent, from replica src_index[j], exactly what kb_fork copies: action, security
 * factors, margins, adjusted, accuracies, the tie-break stream (seed and counters), the observation the resident loop chose its
 * last action in, and the flag word verbatim.  Restarted as after kb_fork: statistics, repair-work counters, launch-order
 * lists, stored select scores -- and the cache of the last kb_predict (kb_update answers RS_ESTATE until a new kb_predict).
 * Layout: kb_fork's (full shells at an exclusive scan of their sizes in (dictionary, shell) order), so two calls with the same
 * arguments give byte-identical kb_save_state blobs.  The DATA crosses bit for bit; CONTINUING does not promise the bits the
 * shared handle would have produced -- the triangle forms d* = Kinv K_f in another summation order than the full storage.
 * Ordered as kb_fork, by events on both streams: after src's queued work, src's later work after the gather; the host waits once,
 * for the scan's total; never captured into a graph.  src is not written, and a handle whose communicator was aborted can
 * still be unshared: that is how its dictionaries are rescued.
 * RS_EINVAL: src is not a shared-dictionary handle or dst is one, the configurations differ, an index out of range.
 * RS_ESTATE: src not reset, dst inference-only, a by-reference handle on either side, different devices, src between
 * kb_shared_scan and kb_shared_commit of a round (proposals scanned or applied, the round not committed).  RS_EOVERFLOW: the
 * shells do not fit dst's pool, or a dictionary exceeds dst's capacity -- dst is then left as kb_fork leaves it: reset, with
 * the sources' control state and empty dictionaries.
 *
 * kb_share: the other direction.  dst: a shared-dictionary LEARNING handle; src: a per-replica learning handle (it holds Kinv;
 * an inference-only source goes through kb_fork_rebuild first), same kb_config except n_envs, pool_bytes, shared_dictionary and
 * first_env; same device.  dst's S dictionaries become those of src agent dict_agent: pages whole, the lower tiles as they
 * are, every upper tile (bi, bj), bi < bj, the transpose of the lower tile (bj, bi) -- what the shared mode's own symmetric
 * update would have stored --, and the sizes, heads, marks and versions.  Control state, tie-break stream, last observation and
 * flag word of dst replica j come from src agent ctl_index[j] (host array of dst->n_envs entries; NULL: dict_agent for every
 * replica).  dst becomes reset; its previous dictionaries are dropped as by kb_reset, and everything the shared mode derives
 * from a dictionary (the scoring operands and products, the proposal cursors) is rebuilt by the next step.  The call does not
 * touch dst's communicator and nothing in it depends on the rank: ranks that each call it with identical sources hold
 * identical dictionaries.  Ordering, restarts and the one host wait (here: the S sizes) as kb_unshare.  RS_EINVAL: dst is not
 * a shared-dictionary handle or src is one, the configurations differ (a different capacity included: dst is not touched),
 * dict_agent or an index out of range.  RS_ESTATE: as kb_unshare (here dst is the handle that must not be inside a round).
 * RS_EOVERFLOW: the shells do not fit dst's pool -- dst is left reset, with the sources' control state and empty dictionaries.
 *
 * kb_bridge_time_ms: of the last kb_unshare / kb_share into k -- with kb_set_kernel_timing on in k at the call, device ms of
 * its gather (one pair of HIP events on k's stream around the table and shell kernels; 0 otherwise), and the bytes its work
 * plan counts: bytes[0] read, bytes[1] written. */
int kb_unshare(kb_handle* dst, kb_handle* src, const int32_t* src_index);
int kb_share(kb_handle* dst, kb_handle* src, int32_t dict_agent, const int32_t* ctl_index);
int kb_bridge_time_ms(kb_handle* k, double* ms, uint64_t bytes[2]);
/* on = 0: the resident loop (kb_step_resident, each step of kb_run_resident) runs select_action(new obs) only -- the
 * reference's loop body past learning_time (kbrl_control.py:131-133): dictionaries, accuracies and security factors stay as
 * they are; margins, adjusted, action and the tie-break counters move as select_action moves them; a history column is still
 * recorded, its hits repeating those of the last learning step (zeros if there was none since kb_reset / kb_fork).  on = 1
 * resumes learning.  The host entry points (kb_update_control, ...) are not affected. */
int kb_set_learning(kb_handle* k, int on);

/* Budgeted dictionaries.  kb_prune leaves every dictionary that holds more than `target` landmarks with exactly `target`
 * and does not touch the others; *removed_total (may be NULL) = landmarks removed by the call.  One landmark leaves at a
 * time: with P = Kinv of the live landmarks and c their coefficients, r = argmin_j (c_j c_j) / P[j][j] (lowest j on a tie);
 * every survivor's coefficient takes c_i + c_r * ((-P[i][r]) / P[r][r]) -- the best approximation of c_r k(l_r, .) by the
 * survivors, squared error c_r^2 / P[r][r] --; P[i][j] takes P[i][j] - (P[i][r] * P[j][r]) / P[r][r], the survivors' inverse
 * Gram matrix exactly; landmark m - 1 moves into slot r (vector-page rows, row and column of Kinv) and the vacated slot and
 * Kinv row are cleared to zeros.  The result does not depend on which other dictionaries the call prunes.  Per touched
 * dictionary afterwards: the newest-landmark heads and chain links are rebuilt, the off-grid count recounted, the version
 * bumped (stored select scores are not reused), the cache of the last kb_predict invalidated (kb_update then answers
 * RS_ESTATE until a new kb_predict); the float32 mark, the control state, the tie-break stream and the flag word stay (bit
 * 16 is sticky).  Shells are kept: growing back to the old size allocates nothing, and kb_get_pool reports the same bytes in
 * use.  Ordered on the agent's stream, between kb_run_resident calls (never captured); the host waits for it.
 * RS_EINVAL: target < 64 or target > capacity.  RS_ESTATE: a shared-dictionary handle (kb_shared_prune), an inference-only handle, kb_reset
 * missing, or dictionaries with a diagonal entry of Kinv that is not finite and positive -- those are left as they are (the
 * others are pruned; kb_last_error counts them).
 * kb_get_pruned: landmarks removed per dictionary [n_envs][S] since kb_reset / kb_load_state / kb_fork into the handle (the
 * counters are not part of a checkpoint: kb_state_bytes and the blobs are what they were).
 * kb_prune_time_ms: with kb_set_kernel_timing on, device time (HIP events) summed over the launches since the last call of
 * [0] the choose, [1] the downdate, [2] the move kernel, and the launches n.
 * kb_get_prune_work: the downdate's work since kb_reset / kb_load_state / kb_fork into the handle, counted from its work plan:
 * [0] units of 8,192 bytes read and 8,192 written (only units that hold rows), [1] launches with work.  Like the pruned
 * counters it is not part of a checkpoint. */
int kb_prune(kb_handle* k, int32_t target, uint64_t* removed_total);
int kb_get_pruned(kb_handle* k, int64_t* removed /* [n_dictionaries] since kb_reset */);
int kb_prune_time_ms(kb_handle* k, double ms[3], int64_t n[3]);   /* choose, downdate, move: HIP events, when kernel timing is on */
int kb_get_prune_work(kb_handle* k, uint64_t work[2]);
/* Budgeted SHARED dictionaries.  kb_shared_prune is kb_prune on a shared-dictionary handle
 * (kb_config.shared_dictionary = 1): each of its S dictionaries that holds more than `target` landmarks is left with exactly
 * `target`, by kb_prune's rule to the letter -- the same victim, the same expressions in the same operation order, nothing
 * summed -- on the storage the handle has: both block triangles of Kinv are downdated in place, the upper one staying the
 * exact transpose of the lower.  One dictionary comes out, bit for bit, as kb_prune leaves its unshared copy (kb_unshare):
 * landmarks, slots, coefficients and the lower triangle.  Per touched dictionary afterwards: heads and chain links rebuilt, the
 * off-grid count recounted (a dictionary whose last off-grid landmark left is scored on the wide path again), the version
 * bumped, and the cache of the last kb_predict invalidated for EVERY replica of the slice.  Everything the shared mode
 * derives from a dictionary (the scoring operands and products, the proposal cursors) is rebuilt by the next step, as after
 * kb_share.  Control state, tie-break streams, flag words and shells stay (kb_get_pool reports the same bytes before, after,
 * and after growing back); the communicator is not touched.  Nothing in the call depends on the rank: ranks that call it with
 * the same target at the same step keep bit-identical dictionaries with no collective.  Ordered on the agent's stream, never
 * captured; the host waits twice, as kb_prune does.  kb_get_pruned ([S] entries), kb_prune_time_ms and kb_get_prune_work
 * report it as they report kb_prune (here a dictionary's work line is its whole block square: twice the triangle's units).
 * RS_EINVAL: target < 64 or target > capacity.  RS_ESTATE: a handle that is not shared-dictionary (kb_prune is the call
 * there), kb_reset missing, a round open between kb_shared_scan and kb_shared_commit, or dictionaries with a diagonal entry of
 * Kinv that is not finite and positive -- those are left as they are, the others are pruned.  The handle stays usable. */
int kb_shared_prune(kb_handle* k, int32_t target, uint64_t* removed_total);
/* ---- The online budget (csrc/kb_online_prune.hip): kb_prune's rule inside the closed loop.
 * kb_set_online_prune(k, target, rounds): target 0 = off, the default.  When on, every update phase -- enqueued by
 * kb_update_control, kb_step_resident or kb_run_resident, plain or captured into its graph, under Projectron's rule or under
 * Projectron++ (kb_set_control_plus, with or without its batch and wide switches) -- is followed by a budget stage, before
 * anything else reads the dictionaries (in the resident step: between the update phase and select_action, so the action is
 * chosen by the classifier the agent keeps and the scores select leaves for the next update phase stay valid).  Every
 * dictionary with m > target loses min(m - target, rounds) landmarks, each by kb_prune's removal in its operation order, and is
 * then finished once as kb_prune finishes a touched dictionary (chains, off-grid count, version, stored scores, predict cache).
 * No sum is formed: a dictionary comes out bit for bit as kb_prune(k, target) at the same point leaves it whenever `rounds`
 * covers its excess, whatever the launch and whichever other dictionaries are over the target.  What a stage leaves above the
 * target the following stages take (carry).  A stage runs only behind an update phase: with kb_set_learning(k, 0) nothing
 * grows and nothing is pruned.  kb_fit, kb_fit_steps and kb_update are not followed by one (kb_prune is the call there).
 * Nothing in the stage waits for the host: 2 + 3 * rounds launches of a geometry fixed by the setter, which return at once
 * while nothing is over the target.  A step that inserts more than capacity - m landmarks saturates and is flagged (bit 8)
 * as without the switch.  A dictionary whose Kinv diagonal is not finite and positive, or whose coefficient is not finite, is
 * left exactly as kb_prune leaves it (untouched if met in the stage's first removal, stopped after the completed ones
 * otherwise), its replica gets bit 32 of its flag word (kb_get_flags), the others are pruned and the loop goes on.
 * kb_get_pruned counts the stage's removals with kb_prune's.
 * The setting is host state of the handle like the other switches: not written by kb_save_state, and kb_load_state, kb_fork,
 * kb_unshare and kb_import_agents leave the destination's setting alone.  Setting or changing it drops a captured loop (the
 * handle waits for its stream first); the next kb_run_resident captures the new sequence.
 * RS_EINVAL: target neither 0 nor in 64 .. capacity - 64 (one shell of headroom for a step's insertions); rounds outside
 * 1 .. 64.  RS_ESTATE: a shared-dictionary handle (kb_shared_prune between steps is the call there), an inference-only or
 * by-reference handle (set it on the learning handle and deploy again), kb_reset missing.
 * kb_get_online_prune: the setting ((0, 2) on a handle it was never set on).
 * kb_online_prune_info, counted on the device since kb_reset / kb_load_state / kb_fork into the handle: work[0] stages
 * enqueued, [1] landmarks removed, [2] dictionary-stages left above the target (carry), [3] the largest excess a stage met,
 * [4] dictionaries flagged (each once), [5] units of the downdate that held rows (8,192 bytes read + 8,192 written each);
 * [6], [7] reserved (0). */
int kb_set_online_prune(kb_handle* k, int32_t target, int32_t rounds);
int kb_get_online_prune(kb_handle* k, int32_t* target, int32_t* rounds);
int kb_online_prune_info(kb_handle* k, uint64_t work[8]);
/* ---- The online budget of a SHARED-dictionary handle (csrc/kb_shared_online_prune.hip): kb_shared_prune's rule
 * as the last stage of every shared learning step.
 * kb_set_shared_online_prune(k, target, rounds): target 0 = off, the default.  When on, every kb_shared_step and
 * kb_shared_step_resident that returns RS_OK from its rounds has enqueued, on the agent's stream behind its last round and in
 * front of whatever reads the dictionaries next (in the resident step: select_action, whose scores the next step's first scan
 * reuses), a budget stage: every shared dictionary with m > target loses min(m - target, rounds) landmarks by kb_prune's removal
 * on full storage and is finished once as kb_shared_prune finishes it (chains, off-grid count, version, the predict cache of
 * EVERY replica of the slice).  No sum is formed: a dictionary comes out bit for bit as kb_shared_prune(k, target) at the same
 * point leaves it whenever `rounds` covers its excess; what is left above the target the following stages take (carry).
 * Nothing in the stage waits for the host: 2 + 3 * rounds launches, the same whatever the dictionaries hold, which return at
 * once while nothing is over the target; a step that leaves with RS_EHIP enqueues none.  A dictionary whose Kinv diagonal is
 * not finite and positive, or whose coefficient is not finite, is left as kb_shared_prune leaves it and EVERY local replica
 * gets bit 32 of its flag word (kb_get_flags): the dictionary serves them all.  kb_get_pruned counts the removals.
 * The setting is host state of the handle: in no kb_save_state blob, kept by kb_reset and by kb_load_state into the handle; a
 * handle made by kb_create (what kb_share fills) starts with it off.  Nothing depends on rank or communicator and nothing is
 * exchanged: ranks that set the same value keep bit-identical dictionaries, as with kb_set_shared_plus, and like there nothing
 * checks the value across ranks -- the caller sets the same one on every rank before the same step.
 * RS_EINVAL: target neither 0 nor in 64 .. capacity - 1 (a shared dictionary at its capacity projects: no headroom shell);
 * rounds outside 1 .. 64.  RS_ESTATE: a per-replica handle (kb_set_online_prune is the call there), kb_reset missing, a round
 * open between kb_shared_scan and kb_shared_commit.  A refusal leaves the earlier setting in place.
 * kb_get_shared_online_prune: the setting ((0, 2) on a handle it was never set on).
 * kb_shared_online_prune_info: kb_online_prune_info's words for these stages, restarted wherever kb_get_pruned's counters are (kb_reset, kb_load_state):
 * work[0] stages enqueued, [1] landmarks removed, [2] dictionary-stages left above the target (carry), [3] the largest excess a
 * stage met, [4] dictionaries flagged (each once), [5] units of the downdate that held rows; [6], [7] reserved (0).
 * kb_shared_online_prune_stage: enqueues ONE stage with the handle's setting and returns without waiting -- for the host-driven
 * rounds (kb_shared_scan / kb_shared_apply / kb_shared_commit), where only the caller knows that a step's rounds are over.
 * RS_ESTATE while the switch is off, while a round is open, or on a per-replica handle. */
int kb_set_shared_online_prune(kb_handle* k, int32_t target, int32_t rounds);
int kb_get_shared_online_prune(kb_handle* k, int32_t* target, int32_t* rounds);
int kb_shared_online_prune_info(kb_handle* k, uint64_t work[8]);
int kb_shared_online_prune_stage(kb_handle* k);
/* ---- the learner's own surface, batched (csrc/kb_fit.hip): sample sequences in, trained learners out; query
 * sets in, scores out.  Build-defined: the reference has Projectron.predict(x) / update(x, y), one sample per call.
 *
 * kb_fit: teacher-forced online learning.  task[i] = e * n_slices + s names learner i of the call (all distinct); it owns rows
 * first[i] .. first[i + 1] - 1 of x ([first[n]][16] doubles per row, entries past dims[s] + 1 ignored) and y (+1 / -1).  For
 * every listed learner, independently, for its samples in order: (y_pred, f) = predict(x_t), then update(x_t, y_t) -- exactly
 * the sequence kb_predict(e, s, x_t); kb_update(e, s, x_t, y_t), with every rule it carries (the float32 roundings while one
 * landmark is held, f y <= 0 as the mistake test, projection against insertion on delta > eta, saturation at the capacity and
 * pool exhaustion -- which flag the replica and project --, the float32 mark and grid index of an inserted landmark, the chain
 * links and version bump, an exact tie f == 0 with a populated dictionary drawing from the learner's tie stream, the
 * per-learner statistics).  One 256-thread workgroup per learner runs the same device functions as the two one-sample
 * kernels, so dictionaries (landmarks, coefficients, all of Kinv, sizes), tie counters, statistics, flags and every returned
 * value are BIT FOR BIT what the one-by-one sequence leaves, whenever the pool suffices for both (with learners growing in
 * parallel, WHICH learner meets the end of the pool is not the sequential one; each learner then still equals some one-by-one
 * run with its flag set).  chunk: most samples of one learner per kernel launch (0: the default, 256) -- launches are enqueued
 * back to back, no result depends on it.  y_pred, f, branch (0 none, 1 projection, 2 dictionary grew), delta and m_after (the
 * dictionary's size after the sample) are [first[n]] each, written at the same rows as the samples; any may be NULL.
 * Afterwards the cache of the last kb_predict of every learner that was given samples is invalid (kb_update answers RS_ESTATE
 * until a new kb_predict), stored select scores are not reused (the version moved), and learners not listed or listed with no
 * samples are untouched bit for bit.  The host waits for the call.
 * RS_EINVAL: a task out of range or listed twice, y not +1 / -1, first decreasing, n or chunk negative.  RS_ESTATE: kb_reset
 * missing; an inference-only handle (kb_deploy, kb_import_agents); a by-reference handle (kb_deploy_ref); a shared-dictionary
 * handle (several tasks map to one dictionary).
 *
 * kb_score: read-only scoring.  Same (task, n, first, x) layout; task may repeat.  f[q] is bit for bit the f kb_predict would
 * return for that learner and point; y_pred (may be NULL) its sign, 0 on an exact tie or an empty dictionary.  NOTHING is
 * written into the handle -- no kernel row, no cache, no counter, no tie draw -- so it works on every kind of handle: learning,
 * kb_deploy, kb_import_agents, kb_deploy_ref (where kb_predict is refused) and shared-dictionary.  One launch per call.
 * RS_EINVAL: a task out of range, first decreasing, n negative.  RS_ESTATE: kb_reset missing.
 *
 * kb_fit_time_ms: of the last calls on the handle.  ms[0]: device time (HIP events) summed over the launches of the last kb_fit,
 * ms[1]: of the last kb_score's launch -- both 0 unless kb_set_kernel_timing was on at the call.  work[0] samples, work[1]
 * mistakes, work[2] insertions of the last kb_fit; work[3] kernel evaluations (landmarks x samples) of the last kb_fit plus
 * those (landmarks x queries) of the last kb_score. */
int kb_fit(kb_handle* k, const int32_t* task, int32_t n, const int64_t* first, const double* x, const int8_t* y, int32_t chunk,
           int32_t* y_pred, double* f, int32_t* branch, double* delta, int32_t* m_after);
int kb_score(kb_handle* k, const int32_t* task, int32_t n, const int64_t* first, const double* x, double* f, int32_t* y_pred);
int kb_fit_time_ms(kb_handle* k, double ms[2], uint64_t work[4]);

/* ---- the update rule of the learner's own surface.  KB_ALG_PROJECTRON (the default): Projectron.update
 * (projectron.py:39-60), an update on a mistake f y <= 0 only.  KB_ALG_PROJECTRON_PLUS: ProjectronPlus.update (projectron.py:
 * 71-107, Projectron++): a mistake is handled as Projectron handles it, and a sample classified correctly inside the margin,
 * 0 < f y < 1, gives a scaled projection coeff += (alpha y) d* when loss - delta / eta > 0 (loss = 1 - f y; alpha = min(min(loss /
 * norm, 1), 2 (loss - delta / eta) / norm), norm = max(1 - delta, 0)) -- it never adds a landmark -- and nothing otherwise.
 * kb_update and kb_fit then report branch 3 (margin update: coefficients changed, version bumped) and 4 (margin test, nothing
 * written) beside 0, 1, 2, and delta for branches 1-4; a "mistake" of the per-learner statistics and of kb_fit_time_ms's work[1]
 * is a sample that changed the dictionary (branches 1-3).
 * The algorithm is a property of the HANDLE -- how its next kb_update / kb_fit are done --, not of its dictionaries: it is not
 * part of kb_save_state blobs or agent files, and kb_fork, kb_deploy, kb_import_agents, kb_unshare and kb_share do not carry it
 * over (the destination keeps its own).  While a handle is in Projectron++ mode the closed control loop does not learn through
 * it: kb_update_control, and kb_step_resident / kb_run_resident with learning on, answer RS_ESTATE (kb_set_learning(k, 0), or
 * kb_set_algorithm back, lifts that; so does kb_set_control_plus(k, 1), below, under which the loop learns by this rule);
 * everything that only reads dictionaries or moves them works as before.
 * kb_set_algorithm: RS_EINVAL for an unknown value; RS_ESTATE for KB_ALG_PROJECTRON_PLUS on an inference-only, a by-reference
 * or a shared-dictionary handle (they do not learn through kb_update / kb_fit). */
#define KB_ALG_PROJECTRON 0
#define KB_ALG_PROJECTRON_PLUS 1
int kb_set_algorithm(kb_handle* k, int32_t alg);
/* (on a shared-dictionary handle always KB_ALG_PROJECTRON: not the rule its rounds learn by, which kb_get_shared_plus reports) */
int kb_get_algorithm(kb_handle* k, int32_t* alg);

/* ---- kb_fit for learners that hold large dictionaries: chip-wide rounds (csrc/kb_fit_wide.hip).  kb_fit teaches
 * one learner per workgroup; against a dictionary of thousands of landmarks every mistake is an O(m^2) mat-vec and rank-1 update
 * that this one workgroup streams alone.  kb_set_fit_wide(k, min_landmarks, window): min_landmarks = 0 (the default) leaves
 * kb_fit exactly as it is; min_landmarks >= 2 hands every listed learner whose dictionary holds at least that many landmarks AT
 * THE START OF A CHUNK (kb_fit's `chunk`) to rounds of plain launches for that chunk -- a scan of the next `window` samples, the
 * first mistake, its mat-vec and rank-1 update spread over the whole chip by cost -- while the others go through the one-workgroup
 * kernel as before.  A dictionary that grows past the threshold inside a call changes path at a chunk boundary.  Every returned
 * value, dictionary (landmarks, coefficients, all of Kinv), tie counter, statistic and flag, and kb_fit_time_ms's work[4], are BIT
 * FOR BIT those of the narrow path, whatever min_landmarks, window and chunk; only the time differs.  window: samples per learner
 * a round scores ahead, 1 .. 256, 0 = the default (64).  The value 1 for min_landmarks is refused: the float32 regime of a single
 * landmark stays in the narrow path.  In Projectron++ mode (kb_set_algorithm) kb_fit takes the narrow path whatever this setting
 * says, and kb_fit_wide_info reports zeros, UNLESS kb_set_fit_wide_plus(k, 1) has been called as well (below).
 * Like the algorithm, the setting is host state of the HANDLE: not part of kb_save_state blobs or agent files, not carried over
 * by kb_fork, kb_deploy, kb_import_agents, kb_share or kb_unshare.  Off by default.
 * kb_set_fit_wide: RS_EINVAL for a negative value, for min_landmarks = 1 and for a window above 256; RS_ESTATE on an
 * inference-only, a by-reference or a shared-dictionary handle (they do not learn through kb_fit).
 * kb_fit_wide_info: of the last kb_fit on the handle -- work[0] samples taught by rounds, work[1] mat-vecs the rounds ran (the
 * mistakes taught there; in Projectron++ mode every sample of branches 1-4 taught there, branch 4 included), work[2] tiles of Kinv
 * those mat-vecs read (n_b (n_b + 1) / 2 each, n_b = ceil(m / 64); 32,768 bytes a tile), work[3] kernel evaluations of the window
 * scans (samples scored x landmarks; the rescans after a mistake -- in Projectron++ mode after any sample of branches 1-4 -- are
 * counted here and not in kb_fit_time_ms's work[3]).
 *
 * kb_set_fit_wide_plus(k, on): whether the rounds also teach in Projectron++ mode.  on = 0 (the default): as above, narrow.
 * on = 1: while the handle is in Projectron++ mode and kb_set_fit_wide's min_landmarks is 2 or more, learners holding that many
 * landmarks at the start of a chunk are taught by the same rounds; a round then stops at the first sample with not (y f >= 1),
 * every such sample -- mistake or margin -- gets its mat-vec over the whole chip, and the margin rule (branches 3, 4) follows it
 * as it follows the one-workgroup mat-vec.  The bits are the narrow path's, as for Projectron.  After a branch 4 (nothing
 * written) the next round scans again; no score of a window is reused.  In Projectron mode the switch has no effect.  Host state
 * of the handle like kb_set_fit_wide's: not saved, not carried over.  A switch of its own, so that kb_set_fit_wide means what it
 * meant.  RS_EINVAL for any value but 0 and 1; RS_ESTATE on an inference-only, a by-reference or a shared-dictionary handle.
 * Measured on G17's stream in Projectron++ mode and on G18's rev stream; not measured: hardware counters, more
 * than eight large learners in one call, thresholds below 64. */
int kb_set_fit_wide(kb_handle* k, int32_t min_landmarks, int32_t window);
int kb_get_fit_wide(kb_handle* k, int32_t* min_landmarks, int32_t* window);
int kb_fit_wide_info(kb_handle* k, uint64_t work[4]);   /* of the last kb_fit */
int kb_set_fit_wide_plus(kb_handle* k, int32_t on);
int kb_get_fit_wide_plus(kb_handle* k, int32_t* on);

/* ---- kb_fit for logs of control steps (csrc/kb_fit_steps.hip): the sample augmentation of kbrl_control.py:103-112
 * on the device.  agent[i] (all distinct, 0 .. n_envs - 1) owns log rows first[i] .. first[i + 1] - 1, in order (first[0] = 0);
 * rows may come from anywhere -- one replica's history, several replicas' histories one after the other.  A row is what a
 * control step logged: state [nv] float32 observations, action [n_slices] PRBs each slice held, labels [n_slices] +1 fulfilled,
 * -1 not, 0 "this learner skips the row".  Learner s of a listed agent is taught every row in row order, independently of the
 * others, and for each row exactly the samples ranslice.kbrl_dev.augmented_samples makes of it: x = ((double)state[its
 * variables], (double)a / (double)n_prbs) with the row's label, for a = action .. n_prbs on +1 and a = 0 .. action on -1, in
 * that order, each through kb_fit's per-sample sequence in the handle's algorithm (kb_set_algorithm) with every rule kb_fit
 * carries.  For each listed agent the call leaves BIT FOR BIT what kb_fit leaves when given augmented_samples of the same rows --
 * landmarks, coefficients, all of Kinv, sizes, statistics, flags, the tie stream's position -- with kb_fit's one exception
 * (which learner meets an exhausted pool, and the pool offsets).  The kernel forms the part of each kernel distance that the
 * state coordinates contribute once per landmark and row, not once per landmark and sample; kb_fit's summation order makes
 * that the same double.
 * Outputs, [first[n]][n_slices] each, any may be NULL -- per (row, learner), not per sample: f_at, the learner's f at the logged
 * allocation (state, action / n_prbs) BEFORE the row's first sample (what update_control's hit test looks at; read-only, no tie
 * draw; on +1 it is the f of the row's first sample); y_at its sign, 0 on an exact tie or an empty dictionary (kb_score's
 * convention); changed, the row's samples that changed the dictionary (kb_fit's "mistakes": branches 1-2, in Projectron++ mode
 * 1-3); grown, its insertions; m_after, the size after the row.  A skipped entry reports 0, 0, 0, 0 and the current size.
 * chunk: most log rows of one agent per launch; 0: the default, max(1, 256 / (n_prbs + 1)), about kb_fit's default in samples.
 * No result depends on it.  The log is staged once: rows x (4 nv + 8 n_slices) bytes in, the summaries out.
 * Afterwards, as after kb_fit: the cached kb_predict of every learner that received a sample is invalid and versions have
 * moved; agents not listed, agents without rows and learners whose entries are all 0 are not touched at all.  kb_fit_time_ms
 * reports the call as it reports a kb_fit (ms[0]; work[0..3] samples, mistakes, insertions, kernel evaluations; the f_at columns
 * are not counted).  The chip-wide rounds are not used: a learner is taught by one workgroup (one per learner; in Projectron++
 * mode under kb_set_fit_steps_batch, below, at most 1024 per launch, which take the learners in turn), kb_set_fit_wide and
 * kb_set_fit_wide_plus have no effect on this call, and kb_fit_wide_info keeps describing the last kb_fit.
 * RS_EINVAL, before anything is changed: an agent out of range or listed twice, first[0] != 0 or first decreasing, a label
 * outside {-1, 0, 1}, an action outside 0 .. n_prbs where the label is not 0, n or chunk negative.  RS_ESTATE: kb_reset missing;
 * an inference-only, a by-reference or a shared-dictionary handle (kb_fit's reasons). */
int kb_fit_steps(kb_handle* k, const int32_t* agent, int32_t n, const int64_t* first /* [n + 1] */,
                 const float* state /* [rows][nv] */, const int32_t* action /* [rows][S] */, const int32_t* labels /* [rows][S] */,
                 int32_t chunk, double* f_at, int32_t* y_at, int32_t* changed, int32_t* grown, int32_t* m_after);

/* ---- the closed control loop in Projectron++ mode (csrc/kb_control_plus.hip).  kb_set_control_plus(k, on):
 * on = 0 (the default): as above -- while the handle is in Projectron++ mode kb_update_control, and kb_step_resident /
 * kb_run_resident with learning on, answer RS_ESTATE.  on = 1: while the handle is in Projectron++ mode those three calls run
 * and learn by the margin rule: per learner the step's row (the state the action was taken in, the executed allocation, its SLA
 * label) goes through exactly what kb_fit_steps does with that row in Projectron++ mode -- the candidates a = action .. n_prbs
 * on +1, 0 .. action on -1, in that order, each through ProjectronPlus.update -- after update_control's bookkeeping
 * (kbrl_control.py:88-101): y_pred from f at the executed allocation (kb_fit_steps's f_at; an exact 0 against a populated
 * dictionary draws from the learner's stream), the hit, the accuracy table, the security factor.  Landmarks, coefficients, all
 * of Kinv, sizes, flags and the per-learner statistics the step adds are BIT FOR BIT kb_fit_steps's for the same rows; hits ==
 * (labels == y_at) wherever f_at != 0.  One 256-thread workgroup per learner, one launch per step, inside the update phase's
 * timing span (kb_phase_times_ms, kb_kernel_times_ms kind 0); the repair queue and the chip-wide rounds are not used and
 * kb_get_repair_work reports zeros for them.  The captured loop of kb_run_resident carries the same launch; setting this
 * switch or kb_set_algorithm to another value drops a captured loop.  In Projectron mode the switch has no effect: kernels,
 * launches and bits stay what they are.  Host state of the handle like the algorithm: not part of kb_save_state blobs or agent
 * files, not carried over by kb_fork, kb_deploy, kb_import_agents, kb_share or kb_unshare.  RS_EINVAL for any value but 0 and 1;
 * RS_ESTATE on an inference-only, a by-reference or a shared-dictionary handle.
 * Cost: late in learning many times Projectron's loop -- one workgroup walks Kinv once per candidate inside the margin
 * (kb_set_control_plus_batch, below, forms the d* of several candidates in one walk). */
int kb_set_control_plus(kb_handle* k, int32_t on);
int kb_get_control_plus(kb_handle* k, int32_t* on);

/* ---- one pass over Kinv for a group of candidates (csrc/kb_control_plus_batch.hip).
 * kb_set_control_plus_batch(k, width, max_landmarks): width = 0 (the default): the update phase of kb_set_control_plus as above,
 * every kernel, launch and bit.  width = 2, 4 or 8: while the handle is in Projectron++ mode AND kb_set_control_plus is on,
 * kb_update_control, kb_step_resident and kb_run_resident (plain and captured) launch control_plus_batch_kernel instead: the same
 * row, but the d* = Kinv K_f of the next `width` candidates are formed together from ONE read of the stored triangle -- they
 * depend on the landmarks and Kinv alone, which only an insertion changes -- and the walk goes on in order with the coefficients
 * as they are; a group nobody of which lies inside the margin (y f >= 1 for all) makes no pass; an insertion ends its group behind
 * itself.  Every sum keeps the one-by-one walk's order: landmarks, coefficients, all of Kinv, the control state, the statistics
 * and kb_get_repair_work are BIT FOR BIT those of width 0.  max_landmarks: a multiple of 64, at least 64 and at most the handle's
 * capacity (ignored when width is 0): the largest dictionary whose candidates are grouped; a larger one, and one of fewer than two
 * landmarks (the float32 regime), takes its candidates one by one inside the same kernel.
 * Scratch: all of it is allocated by this call (the first launch may be inside a stream capture), freed when the width returns
 * to 0 and at kb_destroy, and bounded whatever the fleet -- at most 1024 workgroups per launch take the learners from a ticket,
 * each with an arena for its group's K_f and d* columns:
 *     scratch_bytes = 128 + min(n_envs * n_slices, 1024) * 2 * width * max_landmarks * 8        (0 while the width is 0)
 * A change of either value waits for the agent's stream and drops a captured loop, as kb_set_control_plus does.  Host state of the
 * handle like that switch: not part of kb_save_state blobs or agent files, carried over by no transfer call.  (Blobs saved under
 * different widths may differ in the K_f / d* rows and the tiles' partial-sum slots: scratch every reader rewrites first.)
 * RS_EINVAL for any other width or max_landmarks (the message names the accepted values); RS_ESTATE on an inference-only, a
 * by-reference or a shared-dictionary handle.
 * kb_control_plus_batch_info: work[8] since the switch was last set (zeros while the width is 0): [0] groups formed, [1] groups
 * skipped (nobody inside the margin), [2] passes over Kinv, [3] tiles those passes read (n_b (n_b + 1) / 2 per pass, n_b =
 * ceil(m / 64)), [4] d* columns formed, [5] columns discarded behind an insertion, [6] candidates that went one by one, [7] of
 * those, the ones that ran the mat-vec (branches 1-4). */
int kb_set_control_plus_batch(kb_handle* k, int32_t width, int32_t max_landmarks);
int kb_get_control_plus_batch(kb_handle* k, int32_t* width, int32_t* max_landmarks, uint64_t* scratch_bytes);
int kb_control_plus_batch_info(kb_handle* k, uint64_t work[8]);

/* ---- the large learners' passes spread over the chip (csrc/kb_control_plus_wide.hip).
 * kb_set_control_plus_wide(k, min_landmarks, max_landmarks, rounds): min_landmarks = 0 (the default): the update phase as above,
 * every kernel, launch and bit; the scratch is freed.  Otherwise 2 <= min_landmarks <= max_landmarks, max_landmarks a multiple of
 * 64 in 64 .. capacity, 1 <= rounds <= 256: while the handle is in Projectron++ mode AND kb_set_control_plus is on AND
 * kb_set_control_plus_batch's width is 2, 4 or 8, the learners that hold min_landmarks .. max_landmarks at the start of an update
 * phase -- and no more than kb_set_control_plus_batch's max_landmarks, beyond which that walk takes the candidates one by one --
 * in task order the first min(n_envs * n_slices, 1024) of them, are HEAVY: behind the head of their row (the state, f at
 * the executed allocation, the decision, the bookkeeping) they leave the batch kernel and advance in `rounds` rounds of launches as
 * wide as the chip -- the pass d* = Kinv K_f of a group of candidates, one wave per output block of 64 entries, whatever learner it
 * belongs to; the walk of the group's members, one workgroup per learner, which ends the learner's round at an insertion and
 * otherwise goes on to the next group that needs a pass; the rank-1 update of Kinv of the learners that inserted -- and one more
 * launch finishes, a workgroup per row, whatever the rounds left open (a learner an insertion took past the smaller of the two
 * max_landmarks among them), in the batch kernel's arenas and by its max_landmarks: grouped or one by one as it would be there.
 * Everybody else stays on the batch kernel's row.  No kernel waits for another and nothing on the host waits, so the results do
 * not depend on `rounds` and a captured loop (kb_run_resident, use_graph = 1) carries the whole sequence.  Groups begin and end
 * where the batch kernel's do and every sum keeps its order: landmarks, coefficients, all of Kinv, the control state, the tie
 * streams, kb_get_stats, kb_get_repair_work and all eight counters of kb_control_plus_batch_info are BIT FOR BIT those of the same
 * width with this switch off.  In every other state of the three settings named above every launch is what it is without it.
 * Scratch: all of it is allocated by this call (the first launch may be inside a stream capture), apart from the repair queue's
 * and from kb_set_control_plus_batch's, freed at min_landmarks = 0 and at kb_destroy; with T = n_envs * n_slices and slots =
 * min(T, 1024) -- a slot is a record of 256 bytes and an arena for a group's K_f and d* columns, always eight wide:
 *     scratch_bytes = 128 + slots * 256 + 2 * (slots + 1) * 8 + 8 * ceil(T / 2) + slots * 2 * 8 * max_landmarks * 8    (0 while off)
 * A change of any value waits for the agent's stream and drops a captured loop, as kb_set_control_plus_batch does.  Host state of
 * the handle like the batch width: not part of kb_save_state blobs or agent files, carried over by no transfer call.  RS_EINVAL
 * for any other value (the message names the accepted ones); RS_ESTATE on an inference-only, a by-reference or a shared-dictionary
 * handle.
 * kb_control_plus_wide_info: work[8] since the switch was last set (zeros while it is off): [0] heavy rows taken, [1] learners
 * turned away because the slots were full, [2] learner-rounds that made a spread pass, [3] tiles read in them (n_b (n_b + 1) / 2
 * per pass), [4] rank-1 units spread (16 rows of a tile each), [5] rows that reached the finisher unfinished, [6] candidates the
 * finisher walked, [7] update phases launched in this mode. */
int kb_set_control_plus_wide(kb_handle* k, int32_t min_landmarks, int32_t max_landmarks, int32_t rounds);
int kb_get_control_plus_wide(kb_handle* k, int32_t* min_landmarks, int32_t* max_landmarks, int32_t* rounds, uint64_t* scratch_bytes);
int kb_control_plus_wide_info(kb_handle* k, uint64_t work[8]);

/* ---- the same pass for the rows of kb_fit_steps (csrc/kb_fit_steps_batch.hip).
 * kb_set_fit_steps_batch(k, width, max_landmarks): width = 0 (the default): kb_fit_steps as above, every kernel, launch and bit.
 * width = 2, 4 or 8: while the handle is in Projectron++ mode kb_fit_steps launches fit_steps_batch_kernel instead: every row's
 * candidates go through the group walk of kb_set_control_plus_batch -- the d* of the next `width` candidates of the row from ONE
 * read of the stored triangle, a group nobody of which lies inside the margin makes no pass, an insertion ends its group behind
 * itself, a group never spans rows.  Landmarks, coefficients, all of Kinv, sizes, statistics, flags, the tie stream's position,
 * all five returned summaries (f_at included) and kb_fit_time_ms's work[0..3] are BIT FOR BIT those of width 0, whatever the
 * chunk; kb_get_repair_work is not added to, as at width 0.  In Projectron mode the setting has no effect.  max_landmarks as for
 * kb_set_control_plus_batch: a multiple of 64, at least 64 and at most the handle's capacity (ignored when width is 0); a larger
 * dictionary, and one of fewer than two landmarks, takes its candidates one by one inside the same kernel.
 * Scratch: the setter's own -- not kb_set_control_plus_batch's, whose report it does not change -- sized for the handle and not
 * for a call, allocated here, freed when the width returns to 0 and at kb_destroy:
 *     scratch_bytes = 128 + min(n_envs * n_slices, 1024) * 2 * width * max_landmarks * 8        (0 while the width is 0)
 * A launch has min(n * n_slices, 1024) workgroups, which take the call's learners from a ticket.  A change of either value waits
 * for the agent's stream.  Host state of the handle: not part of kb_save_state blobs or agent files, carried over by no transfer
 * call.  RS_EINVAL for any other width or max_landmarks (the message names the accepted values); RS_ESTATE on an inference-only,
 * a by-reference or a shared-dictionary handle.
 * kb_fit_steps_batch_info: work[8] of the last kb_fit_steps on the handle, zeroed when a call opens (zeros while the width is 0
 * and in Projectron mode): kb_control_plus_batch_info's eight -- [0] groups formed, [1] groups skipped, [2] passes over Kinv,
 * [3] tiles those passes read, [4] d* columns formed, [5] columns discarded behind an insertion, [6] candidates that went one by
 * one, [7] of those, the ones that ran the mat-vec. */
int kb_set_fit_steps_batch(kb_handle* k, int32_t width, int32_t max_landmarks);
int kb_get_fit_steps_batch(kb_handle* k, int32_t* width, int32_t* max_landmarks, uint64_t* scratch_bytes);
int kb_fit_steps_batch_info(kb_handle* k, uint64_t work[8]);   /* of the last kb_fit_steps */

/* ---- Projectron++ for the shared-dictionary rounds (csrc/kb_shared_plus.hip).  kb_set_shared_plus(k, on):
 * on = 0 (the default): kb_shared_scan, kb_shared_apply, kb_shared_step and kb_shared_step_resident learn by Projectron's rule,
 * every kernel, launch and bit as above.  on = 1: they learn by ProjectronPlus.update (projectron.py:66-107); with one replica
 * that is the reference's sequential loop (kbrl_control.py:103-112) with a ProjectronPlus learner.
 *   scan   round 0's bookkeeping is unchanged (the sign of f at the executed allocation); a replica proposes its first
 *          candidate, in augmentation order from its cursor, with y f < 1 instead of y f <= 0.  The proposal word, collect,
 *          merge and commit are unchanged: a proposer that was not taken scans again from its candidate, a taken one moves past
 *          it whichever branch its sample took.
 *   apply  a dictionary that can still grow predicts the remaining proposals together, as before, and the first in list order
 *          with y f < 1 goes through the margin rule with that f (branches 1-4, float32 while one landmark is held); the rest
 *          are predicted again.  A dictionary at its capacity forms KF, d*, F0 and the Gram block A of the whole list as before
 *          and walks it: f_p = F0_p + g_p, margin = y_p f_p; margin >= 1 nothing; margin <= 0 the projection with w_p = y_p;
 *          otherwise delta = max(1 - A[p][p], 0), norm = max(1 - delta, 0), loss = 1 - margin, slack = loss - delta / eta, and
 *          when slack > 0 the weight w_p = min(min(loss / norm, 1), 2 slack / norm) y_p.  An applied p adds w_p A[q][p] to g_q
 *          of the later q, and the coefficients take c + w_p d*_p in list order.
 * Under KBRL_SERIAL_APPLY=1 (test build) the one-by-one path forms f_p as a fresh k . coeff, so in this mode its coefficient
 * bits differ from the batched walk's; the decisions agree and the values agree within DESIGN.md §2's tolerances.
 * Counters: kb_get_stats[1] counts the samples that changed a dictionary (branches 1-3), [2] the insertions; kb_get_repair_work's
 * work[6] the samples whose branch was 1-4; the saturation flag is raised by mistakes only.
 * Host state of the handle like kb_set_control_plus: off by default, not part of kb_save_state blobs, neither carried nor
 * changed by kb_share, kb_unshare and kb_shared_prune.  kb_get_algorithm keeps answering KB_ALG_PROJECTRON on a shared handle:
 * it names the rule of kb_update / kb_fit, not the fleet's -- this switch does.  Every rank of a group (kb_comm_init) must set
 * the same value before the same step; nothing checks it across ranks.  With equal switches the merged list and the rule are
 * deterministic, so the ranks' dictionaries stay bit-identical without a collective.
 * RS_EINVAL for a null handle or a value other than 0 and 1; RS_ESTATE for a handle that is not shared-dictionary (there
 * kb_set_control_plus is the call meant) and while a round is open between kb_shared_scan and kb_shared_commit. */
int kb_set_shared_plus(kb_handle* k, int32_t on);
int kb_get_shared_plus(kb_handle* k, int32_t* on);

/* ---- Chip-wide passes for shared dictionaries that still grow under the margin rule (csrc/kb_shared_plus_batch.hip, DESIGN.md
 * §8r).  kb_set_shared_plus_batch(k, min_landmarks, segments): min_landmarks = 0 (the default) off -- every launch, kernel and
 * byte as kb_set_shared_plus leaves them.  Otherwise, while kb_set_shared_plus is on and KBRL_SERIAL_APPLY is not set (test
 * build), a merged list of at least one proposal whose dictionary holds min_landmarks <= m < capacity landmarks when the apply
 * begins is ENGAGED and applied in segments (between two insertions the landmarks and Kinv are fixed):
 *   1. for the proposals that remain, against the dictionary as it stands, KF, d* = Kinv KF, F0 = KF . coeff and the lower block
 *      triangle of A = KF d*^T, each value summed as kb_shared_apply sums it for a dictionary at its capacity, by kernels as wide as
 *      the chip (the mat-vec on the matrix cores where m is a multiple of 64);
 *   2. one wave walks them by that dictionary's rule (above: f_p = F0_p + g_p with g = 0 at the segment's start, branches 0, 1, 3
 *      and 4) with one addition: a mistake with max(1 - A[p][p], 0) > eta while m < capacity stops the walk before it is applied;
 *      a mistake that does not stop projects with w_p = y_p, and the saturation flag is raised only at the capacity;
 *   3. the coefficients take c + w_p d*_p of the applied proposals in list order;
 *   4. the sample the walk stopped at goes through the one-by-one update with the walk's f_p: its own residual decides between
 *      projection and insertion, its capacity and pool rules apply; the next segment starts behind it.
 * A list whose dictionary reaches its capacity in the middle stays with the segments to its end.  Lists that are not engaged go as
 * without this switch (m < min_landmarks one by one, the float32 regime of m <= 1 included; m >= capacity the full-batch walk).
 * `segments` (0 .. 16) segment rounds are enqueued per apply, then a finishing launch that takes what they left in the same
 * segments with the same arithmetic: the results do not depend on `segments`, which may differ between the ranks of a group;
 * min_landmarks must be the same on every rank, and nothing checks it.  Nothing waits on the host.
 * As for a dictionary at its capacity, f_p is F0_p plus a chain of fused multiply-adds, not a fresh k . coeff: the results are
 * defined as bits by tests/shared_plus_batch_mirror.py; against the switch off every branch is equal, coefficients and Kinv agree
 * within DESIGN.md §2's tolerances.  Counters as above (kb_get_stats[1], [2], work[6] of kb_get_repair_work).
 * Host state like kb_set_shared_plus: in no kb_save_state blob, left alone by kb_share, kb_unshare and kb_shared_prune; it is
 * remembered while kb_set_shared_plus is off and acts only while that is on.
 * RS_EINVAL for a null handle, min_landmarks other than 0 or 2 .. capacity, segments outside 0 .. 16; RS_ESTATE for a handle that
 * is not shared-dictionary and while a round is open between kb_shared_scan and kb_shared_commit.
 * kb_shared_plus_batch_info, since kb_reset: work[0] engaged lists, [1] segments walked, [2] proposals covered by the segments'
 * wide passes (the sum of the proposals that remained, over the segments), [3] segments ended by a stop, [4] segments run by the
 * finishing launch; the rest 0. */
int kb_set_shared_plus_batch(kb_handle* k, int32_t min_landmarks, int32_t segments);
int kb_get_shared_plus_batch(kb_handle* k, int32_t* min_landmarks, int32_t* segments);
int kb_shared_plus_batch_info(kb_handle* k, uint64_t work[8]);   /* since kb_reset */

#ifdef __cplusplus
}
#endif

#endif /* RANSLICE_H */
