/*
 * hafgrasp.h -- C-ABI of the MI355X grasp-scoring engine (libhafgrasp.so).
 *
 * Drop-in boundary for the hot path of haf_grasping's CalcGraspPointsServer action server: the body of
 * CCalc_Grasppoints::loop_control() (reference src/calc_grasppoints_action_server.cpp:335-402) after
 * read_pc_cb() (250-329) has put the cloud into the base frame and before the result is published
 * (396-401).  Plain C types only; the caller owns every input/output buffer, the engine owns device
 * memory.  One engine handle may be used by one thread at a time (the reference runs one goal at a time on
 * actionlib's execute thread, server.cpp:182); several handles may coexist (no global state).
 *
 * Every entry point returns 0 on success or a negative HAF_E_* code; haf_last_error() gives the text.
 * The reference itself has no error convention on this path (system() failures are only logged,
 * server.cpp:778-796); a ROS shim maps a non-zero status to setAborted().
 *
 * The engine REQUIRES a HIP device.  There is no CPU fallback: haf_create() fails with HAF_E_DEVICE when
 * no gfx950 device is usable.
 */
#ifndef HAFGRASP_H_
#define HAFGRASP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HAF_ABI_VERSION 2

enum {
    HAF_OK = 0,
    HAF_E_ARG = -1,        /* bad argument / unsupported configuration                         */
    HAF_E_IO = -2,         /* cannot read or parse Features.txt / range file / model file      */
    HAF_E_DEVICE = -3,     /* no usable HIP device, HIP runtime error                          */
    HAF_E_CAPACITY = -4,   /* request exceeds the capacity the engine was created with         */
    HAF_E_BUDGET = -5,     /* (not returned any more: a negative budget yields the reference's empty result, see haf_grasp_input) */
    HAF_E_INTERNAL = -6
};

/* Construction-time inputs: the four ROS params of the server (server.cpp:217-225) plus the reference's
 * compile-time constants generalised to fields (server.cpp:92-101, 202-214). */
typedef struct haf_config {
    const char *feature_file;        /* feature_file_path, default <pkg>/data/Features.txt (626-628)     */
    const char *range_file;          /* range_file_path, default <pkg>/data/range21062012_allfeatures (767-769) */
    const char *model_file;          /* svmmodel_file_path, default <pkg>/data/all_features.txt.scale.model (771-773) */
    int32_t nr_features_without_shaf;/* 302 (224)                                                         */
    int32_t grid_h, grid_w;          /* HEIGHT, WIDTH = 56 cells of 1 cm (92-93); must be equal (681-682)  */
    int32_t n_rolls;                 /* ROLL_MAX_DEGREE/ROLL_STEPS_DEGREE = 12 (101, 345)                 */
    int32_t roll_step_deg;           /* ROLL_STEPS_DEGREE = 15 (95)                                       */
    float   z_shift;                 /* trans_z_after_pc_transform = 0.15 (214)                           */
    int32_t graspval_top;            /* 119 (203): early-exit threshold with show_only_best_grasp         */
    int32_t device;                  /* HIP device ordinal                                                */
    int32_t max_clouds;              /* capacity: clouds per batch call                                   */
    int64_t max_points;              /* capacity: total points per batch call                             */
    uint32_t flags;                  /* HAF_FLAG_*                                                        */
    int32_t graspval_th;             /* 70 (202): a roll whose best vote exceeds it is published as its own hypothesis
                                        when show_only_best_grasp is off (962-969; haf_roll_pose)                          */
    int32_t max_rolls_per_call;      /* capacity: rolls per haf_score_rolls call; 0 = n_rolls.  A roll-sharded engine (one
                                        of N GPUs) only ever scores ceil(n_rolls / N) rolls at a time: its working buffers
                                        are sized for that, the roll geometry still uses the global roll index           */
} haf_config;

#define HAF_FLAG_KEEP_DEBUG 1u       /* keep per-roll intermediates for haf_debug_fetch()                 */
#define HAF_FLAG_PROFILE    2u       /* record HIP events per stage (haf_get_stage_ms)                    */
#define HAF_FLAG_FP32_MFMA  4u       /* RBF contraction as ONE fp32 MFMA pass for every evaluation: same labels, slowest   */
#define HAF_FLAG_SPLIT_F16  8u       /* three fp16 MFMA passes on the hi/lo halves of the fp32 operands for EVERY evaluation
                                        (fp32-grade decision values everywhere).  Default (neither flag): a single-pass fp16
                                        screening kernel decides every evaluation outside a rigorous guard band and only
                                        the rest goes through the three-pass kernel and the fp64 tiers: same labels, same
                                        grasps, about 2.5x the rate                                                       */

#define HAF_FLAG_PROBABILITY 16u     /* svm_with_probability (server.cpp:383 passes false; 791, 831-841): labels and cell values
                                        from "svm-predict -b 1" (svm_predict_probability, svm.cpp:2550-2587) as
                                        show_predicted_gps reads them -- each masked cell takes the prediction of the masked cell
                                        before it -- and the fp32 vote with an int topval.  Needs a model with probA/probB
                                        (svm-train -b 1).  Every decision value comes from the strict tier: complete, not fast */
#define HAF_FLAG_FULL_RANK  32u      /* the screening pass never runs in its low-rank form (haf_screen_low_rank): same labels; for A/B
                                      * measurements and for a deployment that prefers the ten-step kernels it has run so far          */

/* GraspInput (reference msg/GraspInput.msg:3-15) minus the cloud and the frame id: the cloud is passed
 * separately, already in the base frame (server.cpp:316) -- or as a sensor frame the engine puts there (haf_frame, below). */
typedef struct haf_grasp_input {
    double  grasp_area_center[3];        /* geometry_msgs/Point, metres (258-260)                         */
    float   grasp_area_length_x;         /* "in m" in the .msg, used as integer cm incl. the +14 border    */
    float   grasp_area_length_y;         /*   (server.cpp:266-267 truncates to int; client.cpp:183-184)    */
    double  approach_vector[3];          /* normalised by the engine as server.cpp:270-273                 */
    double  max_calculation_time;        /* seconds (277), truncated to int like server.cpp:337.  The reference tests it
                                            at the START of every roll with time()'s 1 s resolution (367-374); this engine
                                            starts all rolls of a request together, so every roll sees 0 s elapsed and
                                            the budget only stops a request whose truncated value is negative: like the
                                            reference (break before roll 0, the goal still succeeds) the call returns HAF_OK
                                            with rolls_done = 0, best_roll = -1, eval = -1020 -- it never cuts the roll set
                                            of a request that has begun                                                   */
    int32_t show_only_best_grasp;        /* changes the result: early exit at >= graspval_top (362-365)    */
    int32_t threshold_grasp_evaluation;  /* carried for API parity; the reference server never reads it    */
    int32_t gripper_opening_width;       /* x-scale factor (281, 433)                                      */
} haf_grasp_input;

/* GraspOutput (reference msg/GraspOutput.msg:1-7) without the header, plus the grid-space winner. */
typedef struct haf_grasp_output {
    int32_t eval;                   /* best vote - 20; -20 = nothing found (390, 1388, 1418)              */
    double  grasp_point1[3];        /* 1389-1391 */
    double  grasp_point2[3];        /* 1392-1394 */
    double  averaged_grasp_point[3];/* 1395-1397 */
    double  approach_vector[3];     /* 1398-1400 */
    float   roll;                   /* radians (1401) */
    int32_t best_row, best_col, best_roll, best_vote;   /* id_row/col_top_overall, nr_roll_top_overall, topval_gp_overall */
    int32_t rolls_done;             /* rolls the sequential reference loop would have executed             */
    int64_t n_evals;                /* masked (cell, roll) pairs scored = SVM evaluations                  */
    int64_t n_rechecked;            /* evaluations re-done in fp64 (guard band of the fast contraction)     */
} haf_grasp_output;

/* One roll's outcome: what show_predicted_gps() leaves behind (server.cpp:865-932) plus the z estimate
 * transform_gp_in_wcs_and_publish() would read from that roll's height grid (1342-1351).  16 bytes: the
 * unit exchanged between GPUs when rolls are sharded. */
typedef struct haf_roll_record {
    int32_t vote;      /* topval_gp of the roll                                   */
    int16_t row, col;  /* after longest-run centring (904-932)                    */
    float   h_locmax;  /* max height in rows row-4..row+4, cols col-4..col+3      */
    int32_t n_evals;   /* masked cells of this roll                               */
} haf_roll_record;

typedef struct haf_cloud {
    const float *xyz;        /* x,y,z fp32 triples                                                        */
    size_t       n_points;
    size_t       stride_floats; /* 3 for packed xyz, 4 for pcl::PointXYZ                                  */
    int32_t      on_device;  /* 0: host memory (copied over PCIe inside the call); 1: HBM resident: ordered on the engine's
                                current stream before the call, or finished (the stream contract at haf_set_stream);
                                2: host memory inside a buffer registered with haf_register_host_cloud (packed xyz, stride 3):
                                the DMA engine reads it where it lies -- no staging copy on the host (a 1.2 MB cloud: 30 us
                                instead of 75); anything else about it as for 0                                        */
} haf_cloud;

typedef struct haf_engine haf_engine;

/* defaults of the reference: 56x56, 12 rolls of 15 deg, z_shift 0.15, nshaf 302, top 119 */
void haf_config_default(haf_config *cfg);
void haf_grasp_input_default(haf_grasp_input *in);   /* centre 0, 32x44, av (0,0,1), 50 s, width 1 (server.cpp:191-215) */

int  haf_create(const haf_config *cfg, haf_engine **out);
void haf_destroy(haf_engine *e);
const char *haf_last_error(const haf_engine *e);     /* e == NULL: error of the last failed haf_create in this thread */

/* Page-locks a host buffer the caller keeps reusing for its clouds (e.g. the PCL buffer of the action server's subscriber) so that
 * clouds inside it can be passed with on_device = 2.  The buffer must stay valid until haf_unregister_host_cloud or haf_destroy.
 * A cloud passed with on_device = 2 that does not lie inside a registered buffer is an error (HAF_E_ARG). */
int haf_register_host_cloud(haf_engine *e, const void *ptr, size_t bytes);
int haf_unregister_host_cloud(haf_engine *e, const void *ptr);

/* GraspInput -> GraspOutput for one cloud: replaces loop_control() (server.cpp:335-402). */
int haf_score(haf_engine *e, const haf_cloud *cloud, const haf_grasp_input *in, haf_grasp_output *out);
/* Batched clouds (BASELINE configs C4/C5): all clouds and all rolls go through the device together. */
int haf_score_batch(haf_engine *e, int32_t n_clouds, const haf_cloud *clouds, const haf_grasp_input *in,
                    haf_grasp_output *out);

/* Roll-sharded form for multi-GPU: score rolls [roll_first, roll_first+roll_count) only and return their
 * records (records[c*roll_count + i]); no cross-roll rule applied.  Gather the records of all shards (one
 * all-gather of n_rolls*16 bytes per cloud) and call haf_finalize(). */
int haf_score_rolls(haf_engine *e, int32_t n_clouds, const haf_cloud *clouds, const haf_grasp_input *in,
                    int32_t roll_first, int32_t roll_count, haf_roll_record *records);
/* Sequential cross-roll rule (strict '>' keeps the lowest roll, early exit at >= graspval_top when
 * show_only_best_grasp; server.cpp:362-365, 953-960) and the grasp pose (1274-1401) from n_rolls records. */
int haf_finalize(haf_engine *e, const haf_grasp_input *in, const haf_roll_record *records, haf_grasp_output *out);

/* One roll's own hypothesis: what show_predicted_gps() hands to transform_gp_in_wcs_and_publish() for that roll when
 * show_only_best_grasp is off and the roll's best vote exceeds graspval_th (server.cpp:962-969): pose from the roll's
 * record, eval = max(vote - 20, 10).  *published = 1 when the reference would publish it, 0 otherwise (out is filled
 * either way, with the clamped eval).  records = the n_rolls records of one cloud (haf_score_rolls / an all-gather). */
int haf_roll_pose(haf_engine *e, const haf_grasp_input *in, const haf_roll_record *records, int32_t roll,
                  haf_grasp_output *out, int32_t *published);

/* Ranked top-K grasp candidates of the LAST scored batch, for a planner whose best grasp fails IK or a collision check.  Defined on the
 * vote and height grids that batch left on the device (no new request; records, roll grids, debug data and counters stay as they were):
 *  1. runs: in every (cloud, roll) each maximal horizontal run of equal vote v >= min_vote; its cell is (row, end - len/2), the
 *     reference's centring (server.cpp:904-932);
 *  2. order: vote desc, roll asc, len desc, row asc, col asc.  A roll's first candidate is its record; the overall first is
 *     haf_finalize's best when show_only_best_grasp is off (strict '>' keeps the lowest roll, 362-365, 953-960);
 *  3. in-roll suppression: walking a roll's candidates in order, one within Chebyshev distance <= cell_radius cells of a kept candidate
 *     of the SAME roll is dropped (0: none);
 *  4. pose: the candidate's record {vote, row, col, h_locmax of the 9x8 window, n_evals of its roll} through haf_roll_pose's pose, then
 *     eval = vote - 20 (390): rank 1 equals haf_score's output in every pose and identity field;
 *  5. cross-roll suppression: merging the rolls in key order, a candidate is dropped when a kept candidate of a DIFFERENT roll lies
 *     1..roll_window roll steps away (circularly when n_rolls * roll_step_deg == 180) and its averaged_grasp_point within min_dist_m
 *     (squared distance in double, <=).  roll_window = 0 or min_dist_m = 0 switches it off.  The two stages are separate: a candidate
 *     dropped in its roll stays dropped even when the one that dropped it is removed across rolls;
 *  6. stop at k kept candidates or when none is left.
 * Every roll the last call scored counts (global roll indices [roll_first, roll_first + roll_count) of a haf_score_rolls call): the
 * ranking does NOT apply show_only_best_grasp's early exit.  A cloud whose budget truncates to a negative value gets 0 candidates.
 * HAF_E_ARG: no scored batch, an engine created with HAF_FLAG_PROBABILITY, a parameter out of range or min_dist_m NaN. */
typedef struct haf_top_params {
    int32_t k;            /* 1..1024 candidates per cloud; default 8                                                    */
    int32_t min_vote;     /* >= 1; default graspval_th + 1 (the hypothesis threshold, 960-962)                         */
    int32_t cell_radius;  /* >= 0; in-roll Chebyshev suppression radius in cells; default 7                           */
    int32_t roll_window;  /* >= 0; cross-roll suppression window in roll steps; default 1                             */
    double  min_dist_m;   /* >= 0; cross-roll suppression distance in metres; default 0.02                            */
} haf_top_params;
typedef struct haf_grasp_candidate {
    haf_grasp_output grasp;   /* pose + best_row/col/roll/vote of the candidate, eval = vote - 20, rolls_done = roll + 1,
                                 n_evals of its roll, n_rechecked 0                                                             */
    int32_t run_length;
    float   h_locmax;
} haf_grasp_candidate;
/* e may be NULL: min_vote then comes from haf_config_default's graspval_th */
void haf_top_params_default(const haf_engine *e, haf_top_params *p);
/* every cloud c of the last scored batch: out[c * p->k + i] for i < n_found[c] */
int  haf_top_grasps(haf_engine *e, const haf_top_params *p, haf_grasp_candidate *out, int32_t *n_found);

/* ---- several GPUs of one node in ONE process (csrc/multi.cpp) ---------------------------------------------------------
 * For a C++ host such as the action server: one engine, one host thread and one HIP stream per entry of devices[], one RCCL
 * communicator over the distinct devices (ncclCommInitAll), collectives over xGMI.  What is sharded is what the reference
 * leaves independent: the rolls of one request (the body of the roll loop, server.cpp:343-386) or the clouds of a batch.
 * A device may appear more than once in devices[] (several shards on one GPU share its rank); every device must then appear
 * the same number of times.  cfg->device is ignored; cfg->max_clouds / n_rolls are the capacity of the WHOLE handle. */
enum { HAF_SHARD_ROLLS = 0,    /* haf_score_sharded: rolls of one request split 5,5,5,5,4,4,4,4-style over the shards   */
       HAF_SHARD_CLOUDS = 1 }; /* haf_score_batch_sharded: cloud b of a batch goes to shard b % n                       */
typedef struct haf_multi haf_multi;
int  haf_create_multi(const haf_config *cfg, const int32_t *devices, int32_t n_devices, int32_t shard_mode, haf_multi **out);
void haf_destroy_multi(haf_multi *m);
const char *haf_multi_last_error(const haf_multi *m);   /* m == NULL: error of the last failed haf_create_multi in this thread */

/* GraspInput -> GraspOutput for one cloud with the rolls sharded: every shard scores its rolls (haf_score_rolls), ONE
 * ncclAllGather exchanges the 16-byte roll records so that every rank holds all n_rolls of them, then the sequential
 * cross-roll rule and the pose (haf_finalize; server.cpp:362-365, 953-960, 1274-1401).  Same result as haf_score.
 * A host cloud is copied to every GPU over that GPU's own PCIe link; a device-resident one (on_device = 1) must live on
 * devices[0] and reaches the other GPUs by one ncclBroadcast. */
int haf_score_sharded(haf_multi *m, const haf_cloud *cloud, const haf_grasp_input *in, haf_grasp_output *out);
/* Batch of host clouds, cloud b on shard b % n, no data-path exchange; ONE ncclAllReduce(max) of a packed 64-bit
 * (vote, cloud) key elects the best grasp of the batch: *best_cloud = its index (highest vote, then lowest index). */
int haf_score_batch_sharded(haf_multi *m, int32_t n_clouds, const haf_cloud *clouds, const haf_grasp_input *in,
                            haf_grasp_output *out, int32_t *best_cloud);
int haf_multi_info(const haf_multi *m, int32_t *n_shards, int32_t *n_ranks, int32_t *rccl_version);
/* The partition haf_create_multi would build for devices[], WITHOUT touching a device: per shard its RCCL rank (distinct devices in
 * order of first appearance) and its slot on that rank, and for HAF_SHARD_ROLLS its contiguous roll range (36 rolls over 8 shards:
 * 5,5,5,5,4,4,4,4).  Arrays of n_devices entries, any of them may be NULL.  Same argument checks, same error texts
 * (haf_multi_last_error(NULL)). */
int haf_multi_plan(const int32_t *devices, int32_t n_devices, int32_t shard_mode, int32_t n_rolls, int32_t *rank_of, int32_t *slot_of,
                   int32_t *roll_first, int32_t *roll_count, int32_t *n_ranks);
/* Host wall-clock of the parts of the last haf_score_sharded / haf_score_batch_sharded call: the whole call, the ncclBroadcast of a
 * device-resident cloud (0 for a host cloud), the collective (all-gather incl. every rank's copy of the records to the host, or the
 * all-reduce), and every shard's own haf_score_rolls / haf_score_batch (shard_ms: n_shards floats).  Any pointer may be NULL. */
int haf_multi_last_timing(const haf_multi *m, float *total_ms, float *bcast_us, float *collective_us, float *shard_ms);
haf_engine *haf_multi_engine(haf_multi *m, int32_t shard);      /* the shard's engine (stage timings, counters, roll grids) */
/* rank `rank`'s copy of the n_rolls gathered records of the last haf_score_sharded call (all ranks hold the same) */
int haf_multi_last_records(const haf_multi *m, int32_t rank, haf_roll_record *records);

/* Per-roll vote grid and mask of the LAST scored batch, for the marker grid the ROS shim publishes
 * (publish_grasp_grid, server.cpp:901-902, 979-1016).  eval_grid: H*W floats, mask: H*W bytes; either may be NULL.
 * (Integer-valued votes; with HAF_FLAG_PROBABILITY the fp32 votes of the probability branch.) */
int haf_get_roll_grid(haf_engine *e, int32_t cloud, int32_t roll, float *eval_grid, uint8_t *mask);

/* Intermediates of the last scored batch (needs HAF_FLAG_KEEP_DEBUG).  dst sizes per (cloud, roll):
 * HEIGHTS H*W f32, INTEGRAL (H+1)*(W+1) f32, MASK H*W u8, LABELS H*W i8 (-1 unmasked, else label text value),
 * DECISION H*W f64 (NaN unmasked), TRANSFORM 16 f32. */
enum { HAF_DBG_HEIGHTS = 0, HAF_DBG_INTEGRAL = 1, HAF_DBG_MASK = 2, HAF_DBG_LABELS = 3, HAF_DBG_DECISION = 4,
       HAF_DBG_TRANSFORM = 5,
       HAF_DBG_SCREEN_MARGIN = 6,    /* H*W f32, default mode: |dec^| / guard band for the cells the screening tier decided
                                        (> 1 by construction), 0 for the cells it handed on, NaN elsewhere */
       HAF_DBG_PROBABILITY = 7,      /* HAF_FLAG_PROBABILITY: H*W*2 f64, the two probabilities of the cell's own output line as
                                        atof reads them ("%g" text), NaN unmasked */
       HAF_DBG_GRASPSGRID = 8,       /* HAF_FLAG_PROBABILITY: H*W f32, the grid show_predicted_gps builds (831-841) */
       HAF_DBG_ROI = 9 };            /* H*W u8, 0 / 1: the ROI cells S_r of the last batch as the device marked them; HAF_E_ARG when that
                                        batch was not haf_score_frames_roi's or haf_score_views_roi's */
int haf_debug_fetch(haf_engine *e, int32_t what, int32_t cloud, int32_t roll, void *dst, size_t dst_bytes);

/* The attribute pipeline of the masked cells of one (cloud, roll) of the last scored batch, as the exact-form feature
 * kernels left it (HAF_FLAG_KEEP_DEBUG; engines of up to 2 GiB of records): per masked cell, in the row-major order of the
 * reference's feature file (server.cpp:637-643), 324 records of
 *   feature  the fp32 HAF/SHAF value (fv.cpp:141-199),
 *   q4       the double svm-scale reads back from its "%.4g" text (fv.cpp:133 -> svm-scale.c:270),
 *   scaled   the double svm-predict reads back from svm-scale's "%g" text (svm-scale.c:344-350 -> svm-predict.c:108);
 *            0 where svm-scale omits the attribute.
 * cells: row, col per masked cell; computed[i] = 1 when an exact-form feature kernel evaluated cell i in the last call
 * (every cell with HAF_FLAG_SPLIT_F16 / HAF_FLAG_FP32_MFMA; in the default mode only the cells the screening pass
 * handed on).  Returns the number of masked cells in *n_cells; fills at most max_cells entries. */
typedef struct haf_attr_record { float feature; float pad; double q4; double scaled; } haf_attr_record;
int haf_debug_fetch_attr(haf_engine *e, int32_t cloud, int32_t roll, int32_t max_cells, int32_t *cells /* [max_cells][2] */,
                         haf_attr_record *attr /* [max_cells][324] */, uint8_t *computed /* [max_cells] */, int32_t *n_cells);

/* THE STREAM CONTRACT (every on_device and out_on_device comment in this header points here).
 *
 * An engine has one CURRENT stream.  haf_create makes a non-blocking stream of the engine's own and makes it current; the engine
 * keeps that stream until haf_destroy, whichever stream is current.  haf_set_stream makes the caller's hipStream_t current; NULL is
 * HIP's default (legacy null) stream -- a stream like any other, what torch.cuda.default_stream() is -- not "no stream".  The caller
 * keeps ownership of a stream it hands over and keeps it alive for as long as it is current.  haf_get_stream returns the current
 * handle (NULL for the default stream, and for a null engine), so
 *     void *old = haf_get_stream(e);  haf_set_stream(e, mine);  ...;  haf_set_stream(e, old);
 * switches to the caller's stream and back to the engine's own.  Handing over the current handle does nothing.  Any other switch
 * first synchronises the stream it leaves (the engine leaves work of its own there: the clear of the next request's counters), so
 * nothing of the engine is left running on a stream once haf_set_stream has returned and the caller may destroy it.
 *
 * What a caller may rely on, on whichever stream is current:
 *   - every kernel, copy and fill of every call that touches a caller's device memory or depends on it is enqueued on the current
 *     stream, and on no other;
 *   - a device-resident input (on_device = 1: clouds, frames, masks, label images) need only be ORDERED on that stream before the
 *     call, or finished: work the caller enqueued on the stream before the call -- a kernel that renders the frame, a copy that has
 *     not completed -- is seen by the call, and no host synchronisation is needed.  Memory written on ANOTHER stream must be finished,
 *     or that stream joined to the current one (an event wait), before the call;
 *   - a device output (out_on_device = 1, the engine's own images) is written on the current stream, behind whatever the caller
 *     enqueued there before the call, and is complete when the call returns: every call synchronises the current stream before it
 *     returns, so host outputs are complete then too.
 * The getters of the last batch (haf_get_roll_grid, haf_debug_fetch*) read state that a finished call left, with blocking copies.
 * HAF_E_ARG for a null engine. */
int haf_set_stream(haf_engine *e, void *hip_stream);
void *haf_get_stream(haf_engine *e);

/* Stage timings of the last call in milliseconds (HAF_FLAG_PROFILE): HIP events on the current stream. */
enum { HAF_ST_UPLOAD = 0, HAF_ST_BIN, HAF_ST_INTEGRAL, HAF_ST_MASK, HAF_ST_FEATURES, HAF_ST_SVM, HAF_ST_REFINE,
       HAF_ST_RECHECK, HAF_ST_VOTE, HAF_ST_DOWNLOAD, HAF_ST_COUNT };   /* REFINE: three-pass kernel on the screened-out rest */
int haf_get_stage_ms(haf_engine *e, float *ms /* HAF_ST_COUNT */);

/* Counters of the last scored batch: masked (cell, roll) pairs; how many fell inside the guard band of the fast
 * contraction and were re-evaluated by the fp64 MFMA tier; how many of those were still too close to zero and were
 * re-evaluated in libsvm's strict fp64 summation order. */
int haf_last_counts(const haf_engine *e, int64_t *n_evals, int64_t *n_rechecked, int64_t *n_strict);

/* The same with the screening tier of the default mode: evaluations the single-pass screening kernel could not decide
 * (they went through the three-pass kernel; 0 in the other modes), then the fp64 MFMA tier, then the strict tier. */
int haf_last_tiers(const haf_engine *e, int64_t *n_evals, int64_t *n_refined, int64_t *n_rechecked, int64_t *n_strict);

/* The exact tiers of the last scored batch (both counted in n_rechecked of haf_last_tiers): evaluations that went through the
 * exact-integer tier (int8 digit planes on the matrix cores, no accumulation error; 0 when the model's support vectors do not
 * fit its fixed-point range), and those still inside its quantisation band that went on to the fp64 MFMA tier. */
int haf_last_exact_tiers(const haf_engine *e, int64_t *n_integer, int64_t *n_fp64);

/* Strict tier of the last scored batch: evaluations whose libsvm-order decision value lay within a last-bit exp error of zero
 * (2^-44 sum|coef|) and were therefore decided on the host with the C library's exp, the function svm-predict itself calls
 * (svm.cpp:364).  None in any run so far. */
int haf_last_strict_host(const haf_engine *e, int64_t *n_host);

/* Pre-stages of the last scored batch: (cloud, roll) grids whose integral image had to be summed in the reference's
 * sequential fp64 order because a parallel partial sum was not exact (normally 0; the result is bit-identical either way). */
int haf_last_prestage(const haf_engine *e, int64_t *n_inexact_grids);

/* Model facts for reporting: support vectors, attribute dimension, feature rows (incl. phantom rows). */
int haf_model_info(const haf_engine *e, int32_t *n_sv, int32_t *dim, int32_t *n_features);

/* Which form of the single-pass screening kernel serves this model in the default mode (chosen at haf_create on a synthetic scene,
 * re-chosen when a request leaves too much undecided): 0 plain, 1 with the measured |w|_2, 2 / 3 the centred-remainder form with the
 * exp / the polynomial epilogue (models with a large C, whose decisions are 1e-5..1e-8 of sum|coef|K); *active = 0 when no form can
 * decide enough and every evaluation takes the three-pass kernel.  Labels are identical in every case; for reporting only. */
int haf_screen_form(const haf_engine *e, int32_t *form, int32_t *active);

/* The low-rank form of the centred-remainder screening pass (round 4): the HAF attributes are linear functionals of the 15x15 window
 * (fv.cpp:141-199) spanning *rank dimensions (158 for the reference's Features.txt), so whole requests on large grids are swept on a
 * projected operand of rank + SHAF slots <= 192 instead of 320.  *available: the engine has the tables; *last_used: the last request's
 * screening pass ran in this form.  Labels are identical in every case; for reporting only. */
int haf_screen_low_rank(const haf_engine *e, int32_t *available, int32_t *rank, int32_t *last_used);

/* PCD v0.7 reader (ascii / binary / binary_compressed; pcl::io::loadPCDFile in client.cpp:141).
 * Returns a malloc'ed packed xyz array (free with haf_free) and the point count. */
int  haf_pcd_load(const char *path, float **xyz, size_t *n_points, char *err, size_t err_cap);
void haf_free(void *p);

/* ---- sensor frames: what a driver hands over, deprojected and put into the base frame ON THE DEVICE (csrc/frames.hip) ---------
 * haf_score / haf_score_batch take packed xyz already in the base frame, i.e. the cloud AFTER read_pc_cb's
 * pcl_ros::transformPointCloud (server.cpp:307-316).  A haf_frame is the step before: a 16-bit or float depth image with the pinhole
 * intrinsics of its camera, or an organised sensor-frame cloud, plus the sensor-to-base transform (rows 0..2 of the TF matrix).  The
 * engine uploads the raw pixels (2 or 4 bytes each instead of 12) and one kernel writes the base-frame points where a staged host
 * cloud would lie; everything downstream is the cloud path, unchanged.
 *
 * The arithmetic, per pixel (u, v) -- point index v * width + u -- every step ONE correctly rounded fp32 operation, in this order,
 * never a fused multiply-add (csrc/frame_points.h, compiled for host and device):
 *   U16:   invalid when d == 0; else z = (float)d * depth_scale
 *   F32:   invalid when d is not finite or d <= 0; else z = d * depth_scale
 *   both:  invalid when z is not finite, z < min_depth (if min_depth > 0) or z > max_depth (if max_depth > 0)
 *          xc = (((float)u - cx) * ifx) * z,  yc = (((float)v - cy) * ify) * z,  ifx = 1.0f / fx and ify = 1.0f / fy once per frame
 *   XYZ:   (xc, yc, z) = the three floats at the pixel; invalid when any is not finite; intrinsics, scale and limits are ignored
 *   base:  p[r] = ((t[r][0] * xc + t[r][1] * yc) + t[r][2] * z) + t[r][3], left to right, t = sensor_to_base
 *   an invalid pixel is the point (NaN, NaN, NaN), all three words 0x7FC00000; so is any component whose result is a NaN.
 * An invalid pixel still yields a point (NaN never passes the binning comparisons), so order and count are those of the pixels:
 * the engine bins width * height points per frame, it does not compact them.  With HAF_FRAME_XYZ_F32 the transform takes the place of
 * pcl_ros::transformPointCloud; PCL's own operation order is not pinned here, the order above is the definition.  No lens distortion. */
enum { HAF_FRAME_DEPTH_U16 = 0, HAF_FRAME_DEPTH_F32 = 1, HAF_FRAME_XYZ_F32 = 2 };
typedef struct haf_frame {
    const void *data;
    int32_t kind, width, height;
    int32_t on_device;           /* 0 host, 1 device-resident (ordered on the current stream or finished: haf_set_stream); 2 is HAF_E_ARG */
    size_t  row_stride_bytes;    /* >= width * element size, a multiple of the element size */
    size_t  point_stride_bytes;  /* XYZ only: >= 12, multiple of 4 (16 = pcl::PointXYZ, 32 = PointXYZRGB) */
    float   fx, fy, cx, cy;      /* pinhole intrinsics in pixels; depth kinds only */
    float   depth_scale;         /* metres per unit: 0.001 for the usual 16UC1 millimetres, 1 for 32FC1 metres */
    float   min_depth, max_depth;/* metres; 0 = no limit on that side; depth kinds only */
    float   sensor_to_base[12];  /* rows 0..2 of the 4x4, row-major: the TF step of server.cpp:316 */
} haf_frame;
/* (element size: 2 / 4 bytes for the depth kinds, point_stride_bytes for XYZ, whose data must be 4-byte aligned) */

void haf_frame_default(haf_frame *f);                       /* identity pose, scale 0.001, no limits, zeros elsewhere */
/* The HOST definition of record of the arithmetic above: width * height * 3 floats from a host frame (on_device = 0).  No device, no
 * engine; HAF_E_ARG for a frame haf_score_frames would refuse for its own fields. */
int  haf_frame_points(const haf_frame *f, float *xyz);
/* haf_score_batch with frames in place of clouds: in[b] and out[b] per frame, the same last-batch state afterwards (haf_top_grasps,
 * haf_get_roll_grid, haf_debug_fetch*, haf_last_*, haf_get_stage_ms; the deprojection kernel counts as HAF_ST_UPLOAD).  Checked before
 * any device work -- HAF_E_ARG: a null argument, n < 1, a null data pointer, an unknown kind, on_device not 0 or 1, a non-positive
 * dimension, a stride too small or misaligned, data not aligned to its element, for the depth kinds fx or fy zero or not finite, a cx,
 * cy, limit or matrix entry that is not finite, depth_scale not finite or not positive; HAF_E_CAPACITY: a frame of more than INT32_MAX
 * pixels, sum of width * height > max_points, n > max_clouds.  A refused call leaves the engine as it was.  An engine created with
 * HAF_FLAG_PROBABILITY takes frames like any other (only the source of the cloud differs).  Not through haf_score_rolls or the sharded
 * multi-GPU calls. */
int  haf_score_frames(haf_engine *e, int32_t n, const haf_frame *frames, const haf_grasp_input *in, haf_grasp_output *out);
/* Cloud `cloud` of the last scored batch as the device kernels read it: n_points >= its point count, packed xyz (HAF_FLAG_KEEP_DEBUG).
 * Frames and staged host clouds; HAF_E_ARG for a device-resident xyz cloud, which the engine never copies. */
int  haf_debug_fetch_points(haf_engine *e, int32_t cloud, float *xyz, size_t n_points);
/* ---- several views of one scene as ONE cloud (csrc/frames.hip: k_view_points) ------------------------------------------------
 * A second camera, or a second pose of the same one, fills the holes one view leaves behind every object.  The fused cloud of a
 * request is the set of VALID points of its views, formed on the device: the points are compacted as they are deprojected, so the
 * later stages read only them (haf_score_frames keeps width * height points per frame, invalid ones included).
 *
 * Host definition of record: the VALID points of frames[0..n_views) -- frame after frame, pixel order inside a frame, each point
 * exactly haf_frame_points' words -- packed into xyz (capacity cap_points; NULL = count only); *n_valid = their number.
 * A pixel is dropped when haf_frame_points gives it any component that is not finite (the all-NaN invalid pixel included).
 * Why that rule changes no result: in every binning kernel and in the bucket sort (k_bin, k_bin_lds, k_bin_tiles, k_small_pre,
 * point_bucket) a point with a NaN or infinite component makes the transformed px or py NaN or infinite, and every range test on
 * them fails; such a point can never reach a height grid.
 * Host frames only (on_device = 0).  HAF_E_ARG: a null frames or n_valid, n_views < 1 or > HAF_MAX_VIEWS, a frame haf_frame_points
 * would refuse; HAF_E_CAPACITY: a frame of more than INT32_MAX pixels, more valid points than cap_points (nothing is written past
 * it).  Every view is checked before a point is written; the message, which names the view, is haf_last_error(NULL)'s. */
#define HAF_MAX_VIEWS 16
int  haf_view_points(const haf_frame *frames, int32_t n_views, float *xyz, size_t cap_points, size_t *n_valid);
/* n requests; request b fuses frames[first_b .. first_b + views_per_request[b]), first_b = sum of the counts before it.
 * Identical in every output and in all last-batch state to haf_score_batch on the clouds haf_view_points defines, except that the
 * ORDER of the points haf_debug_fetch_points returns is unspecified (their multiset and their count are exact).
 * n_points (may be NULL): valid points per request (-1 when every budget of the batch is negative: no roll runs, nothing is counted).
 * The views of one request may mix kinds, host and device residence, sizes, intrinsics and poses.  Checked before any device work,
 * a refused call leaves the engine as it was -- per frame as haf_score_frames checks it, the message naming the request and the
 * view; HAF_E_ARG: a null argument (n_points excepted), n < 1, a view count < 1 or > HAF_MAX_VIEWS; HAF_E_CAPACITY: n > max_clouds,
 * the sum of all pixels > max_points.  HAF_FLAG_PROBABILITY engines take views like any other.  Not through haf_score_rolls or the
 * sharded multi-GPU calls.  The first call with a host XYZ view allocates that kind's raw area (12 bytes x max_points). */
int  haf_score_views(haf_engine *e, int32_t n, const int32_t *views_per_request, const haf_frame *frames,
                     const haf_grasp_input *in, haf_grasp_output *out, int64_t *n_points);
/* Binary PGM ("P5") with 16-bit samples, the usual file form of a 16UC1 depth image: maxval 256..65535, big-endian samples, '#' comments
 * in the header.  Returns a malloc'ed width * height array in host byte order (free with haf_free); HAF_E_IO and a message for anything
 * else, a truncated or over-long file included. */
int  haf_pgm16_load(const char *path, uint16_t **depth, int32_t *width, int32_t *height, char *err, size_t err_cap);

/* ---- per-pixel grasp maps: the votes and rolls of the last scored batch in a sensor frame's image space (csrc/graspmap.hip) ------
 * Every result above lives in the rotated 1 cm grids of the rolls.  A grasp map answers in the caller's pixels: for pixel (u, v) of any
 * haf_frame -- the scored one, another camera, the registered RGB view -- the best vote any roll gives the cell the pixel's point falls
 * into, that roll, and that cell.
 *
 * Host definitions of record (no device, no engine):
 * haf_point_cells: cell[i] = row * grid_w + col of point i (xyz + i * stride_floats) under roll `roll` (global index) of request input
 * `in`, or -1.  The arithmetic is the binning kernel's (server.cpp:488, 510-514), csrc/grasp_cells.h: the roll's fp32 transform,
 * p[r] = ((m[r][0] x + m[r][1] y) + m[r][2] z) + m[r][3] left to right, every step one correctly rounded fp32 operation and never a
 * fused multiply-add; a cell only when -r_row < p[0] < r_row, -r_col < p[1] < r_col (strict; r_row = (float)((0.5 * (float)grid_h) / 100.0))
 * and p[2] is not a NaN; row = (int)floorf(100 * (p[0] + r_row)), col likewise, both inside the grid.
 * HAF_E_ARG: a null argument, grid_h / grid_w / n_rolls < 1, roll outside [0, n_rolls), stride_floats < 3; HAF_E_CAPACITY: n > INT32_MAX.
 *
 * haf_grasp_map_ref: eval_grids = roll_count x grid_h x grid_w floats as haf_get_roll_grid returns them for the rolls roll_first ..
 * roll_first + roll_count - 1 of one request.  For pixel (u, v) of the host frame -- index v * width + u -- the point is
 * haf_frame_points' words; the rolls are walked in ascending order, wherever the point has a cell the vote is (int)eval_grid[cell]
 * (votes are signed), and the largest vote is kept with a strict '>': the lowest roll wins a tie.  vote / roll / cell = that vote, its
 * GLOBAL roll index and its cell.  A pixel gets HAF_MAP_NO_CELL, roll -1 and cell -1 when it is invalid or its point has a component
 * that is not finite (the rule of haf_view_points), or when it has no cell in any roll.  Any output pointer may be NULL.
 * HAF_E_ARG: a null cfg, in or frame, null eval_grids with roll_count > 0, a roll range outside [0, n_rolls] (roll_count = 0 is the
 * request no roll ran for), a frame haf_frame_points would refuse; HAF_E_CAPACITY: a frame of more than INT32_MAX pixels. */
#define HAF_MAP_NO_CELL (-32768)
int  haf_point_cells(const haf_config *cfg, const haf_grasp_input *in, int32_t roll, const float *xyz, size_t n, size_t stride_floats,
                     int32_t *cell);
int  haf_grasp_map_ref(const haf_config *cfg, const haf_grasp_input *in, int32_t roll_first, int32_t roll_count, const float *eval_grids,
                       const haf_frame *frame, int16_t *vote, int16_t *roll, int32_t *cell);
/* The map of request `request` of the LAST scored batch for `frame` (host or device-resident, any kind), computed on the device from
 * the vote grids that batch left there: equal to haf_grasp_map_ref on the request's haf_get_roll_grid grids in every pixel.  vote, roll,
 * cell: width * height packed images in host memory, or in device memory when out_on_device = 1 (written on the current stream, haf_set_stream, and
 * complete when the call returns); any of them may be NULL.  A request whose budget was negative (no roll ran) yields HAF_MAP_NO_CELL
 * everywhere.  Leaves all last-batch state as it was (records, grids, counters, debug data), like haf_top_grasps.
 * HAF_E_ARG: a null frame, no scored batch, request out of range, out_on_device not 0 or 1, an engine created with
 * HAF_FLAG_PROBABILITY (fp32 votes), a frame haf_score_frames would refuse; HAF_E_CAPACITY: width * height > max_points. */
int  haf_grasp_map(haf_engine *e, int32_t request, const haf_frame *frame, int16_t *vote, int16_t *roll, int32_t *cell,
                   int32_t out_on_device);
/* The pose of an arbitrary cell of the last scored batch: the record {vote at the cell, row, col, h_locmax of the 9x8 window as
 * haf_top_grasps computes it, n_evals of the roll} through haf_top_grasps' pose with eval = vote - 20 and run_length 0.  roll is the
 * global roll index.  HAF_E_ARG: no scored batch, HAF_FLAG_PROBABILITY, request / roll / row / col outside the last batch or the grid,
 * a request no roll ran for. */
int  haf_cell_pose(haf_engine *e, int32_t request, int32_t roll, int32_t row, int32_t col, haf_grasp_candidate *out);
/* The best pixel of haf_grasp_map(request, frame) under a host mask (mask[v * mask_row_stride + u] != 0 selects pixel (u, v); NULL:
 * every pixel; mask_row_stride in bytes, >= width) among the pixels whose vote is >= min_vote: vote descending, then roll ascending,
 * then v ascending, then u ascending.  *found = 1 and *out = haf_cell_pose of that pixel's (roll, cell), *u / *v its position (either
 * may be NULL); *found = 0 when no pixel qualifies (out, u, v untouched).  Refusals as haf_grasp_map, plus a null out or found and a
 * mask_row_stride < width with a mask. */
int  haf_grasp_map_best(haf_engine *e, int32_t request, const haf_frame *frame, const uint8_t *mask, size_t mask_row_stride,
                        int32_t min_vote, haf_grasp_candidate *out, int32_t *u, int32_t *v, int32_t *found);

/* ---- the best grasp per object from an instance-label image, in one device pass (csrc/graspmap.hip: k_map_labels) ---------------
 * An instance segmenter's output is one label image: 0 for the background, 1..n_labels for the instances.  One call answers for all of
 * them what haf_grasp_map_best answers for one mask.  A pixel QUALIFIES for label l when its label is l, haf_grasp_map gives it a roll
 * (roll >= 0) and its vote is >= min_vote and above HAF_MAP_NO_CELL (haf_grasp_map_best's rule).  The pick of label l is the qualifying pixel that is best in haf_grasp_map_best's order --
 * vote descending, then roll ascending, then v ascending, then u ascending: picks[l - 1] is what haf_grasp_map_best returns for the
 * mask `labels == l`.  order[0 .. *n_found) lists the found labels, best pick first, in the same key order (pixel indices differ between
 * labels: the order is total).
 *
 * haf_label_best_ref: the host definition of record, no device, no engine, on top of haf_grasp_map_ref's per-pixel rule.  The grids and
 * the frame are those of haf_grasp_map_ref, the label image is a host image (on_device = 0).  order and n_found may be NULL.
 * HAF_E_ARG: everything haf_grasp_map_ref refuses, a null labels, data or picks, elem_bytes not 1 or 2, on_device not 0, a stride too
 * small or misaligned, misaligned uint16 data, n_labels outside 1..HAF_MAX_LABELS.  A refused call writes nothing.
 *
 * haf_grasp_map_labels: the same for request `request` of the LAST scored batch, on the device.  The frame may be host or device
 * resident and of any kind; so may the label image, and a device-resident one is read where it lies, with its stride.  picks equals
 * haf_label_best_ref on the request's haf_get_roll_grid grids in every field.  poses may be NULL; poses[l - 1] is haf_cell_pose(request,
 * roll, cell / grid_w, cell % grid_w) of the pick, zeroed when the label is not found.  One device-to-host copy and one synchronisation
 * whatever n_labels is.  Leaves all last-batch state as it was, like haf_grasp_map.  A request whose budget was negative finds nothing
 * and returns HAF_OK.  Checked before any device work, the engine left as it was: everything haf_grasp_map refuses (an engine created
 * with HAF_FLAG_PROBABILITY included), a null labels, data or picks, elem_bytes not 1 or 2, a stride too small or misaligned,
 * misaligned uint16 data, on_device not 0 or 1, n_labels outside 1..HAF_MAX_LABELS.
 *
 * With haf_score_frames_roi: after a ROI request with the mask `labels != 0` every labelled pixel's cell lies in S_r, so V'_r = V_r
 * there, and picks and order are those of the full request; the poses differ only in n_evals. */
#define HAF_MAX_LABELS 4096
typedef struct haf_label_image {   /* goes with a haf_frame of the same width x height */
    const void *data;              /* 0 = background; 1..n_labels = instance; anything larger is ignored like background */
    int32_t elem_bytes;            /* 1 (uint8) or 2 (uint16, host byte order) */
    int32_t on_device;             /* 0 host, 1 device-resident (ordered on the current stream or finished: haf_set_stream) */
    size_t  row_stride_bytes;      /* >= width * elem_bytes, a multiple of elem_bytes; data aligned to elem_bytes */
} haf_label_image;
typedef struct haf_label_pick {    /* label l is entry l - 1 */
    int32_t found;                 /* 0: no pixel of the label qualifies; then u = v = roll = cell = -1, vote = HAF_MAP_NO_CELL, n_pixels = 0 */
    int32_t u, v, vote, roll, cell;/* the best pixel, and its haf_grasp_map values */
    int32_t n_pixels;              /* pixels of the label that qualify */
} haf_label_pick;
int  haf_label_best_ref(const haf_config *cfg, const haf_grasp_input *in, int32_t roll_first, int32_t roll_count, const float *eval_grids,
                        const haf_frame *frame, const haf_label_image *labels, int32_t n_labels, int32_t min_vote, haf_label_pick *picks,
                        int32_t *order, int32_t *n_found);
int  haf_grasp_map_labels(haf_engine *e, int32_t request, const haf_frame *frame, const haf_label_image *labels, int32_t n_labels,
                          int32_t min_vote, haf_label_pick *picks, haf_grasp_candidate *poses, int32_t *order, int32_t *n_found);

/* ---- scoring only under a pixel mask: "grasp THIS object" without scoring the whole search area (csrc/roi.hip) ------------------
 * haf_score_frames with, per request, an image-space mask over its frame (a segmenter's output).  The cloud of request b is exactly
 * haf_score_frames' cloud of frames[b]: every pixel goes in, masked or not, because the height grids need the whole scene.  What the
 * mask restricts is the set of cells that get a feature vector, a decision and a label.  Per roll r (global index):
 *   ROI cells S_r     the cells haf_point_cells gives the haf_frame_points points of the pixels whose mask byte is not zero and whose
 *                     point is finite in all three components (the rule of haf_view_points);
 *   footprint T       the 29 taps of the vote (server.cpp:873-878): |dr| <= 2 and |dc| <= 2, plus dr = 0 and |dc| = 3, 4; T = -T;
 *   evaluated E_r     the cells c the full request would evaluate (its mask: pnt_in_box, unchanged) with c + t in S_r for some t in T.
 *                     Only these get a label; every other cell keeps label -1;
 *   votes V'_r        the full request's vote V_r(c) for c in S_r, 0 elsewhere.  This holds by construction: a vote reads only c + T,
 *                     all of which is in E_r or outside the full request's mask in both requests, and the labels on E_r are the full
 *                     request's (decision VALUES are not part of the contract: another request composition may be decided by
 *                     another tier);
 *   record of roll r  the reference's rule (first-wins argmax, longest-run centring, 9x8 z window; server.cpp:882-932, 1342-1351)
 *                     applied to V'_r, n_evals = |E_r|;
 *   output            haf_finalize on those records.
 * Consequence: the best vote over the rolls' records equals the maximum of the FULL request's haf_grasp_map vote over the masked
 * pixels whenever that maximum is > 0.  An S_r that is empty in every roll gives the reference's "nothing found" (eval = -20,
 * n_evals = 0) and HAF_OK.
 *
 * haf_roi_cells: the host definition of record, no device, no engine.  roi = S_r, eval = the T-dilation of S_r BEFORE the test of the
 * full request's mask (E_r = eval AND that mask); grid_h * grid_w bytes each, 0 / 1, either may be NULL.  roll is the global index.
 * HAF_E_ARG: a null cfg, in, frame or mask, grid_h / grid_w / n_rolls < 1, roll outside [0, n_rolls), mask_row_stride < width, a frame
 * haf_frame_points would refuse (a device-resident one included); HAF_E_CAPACITY: a frame of more than INT32_MAX pixels. */
typedef struct haf_roi {
    const uint8_t *mask;      /* width x height of the frame it goes with; != 0 selects the pixel */
    size_t  row_stride_bytes; /* >= width */
    int32_t on_device;        /* 0 host, 1 device-resident (ordered on the current stream or finished: haf_set_stream) */
} haf_roi;
int  haf_roi_cells(const haf_config *cfg, const haf_grasp_input *in, int32_t roll, const haf_frame *frame, const uint8_t *mask,
                   size_t mask_row_stride, uint8_t *roi, uint8_t *eval);
/* rois[b] goes with frames[b].  Afterwards the last-batch state is the ROI request's: haf_get_roll_grid returns V'_r and E_r, and
 * haf_top_grasps, haf_grasp_map, haf_cell_pose, haf_grasp_map_best, haf_grasp_map_labels, haf_debug_fetch*, haf_last_* and haf_get_stage_ms work on it
 * unchanged (the ROI kernels count as HAF_ST_MASK).  A request never changes which form of the screening pass serves the engine
 * (haf_screen_form): the calls after it take the paths they would have taken without it.  Checked before any device work, a refused
 * call leaves the engine as it was, the message names the request -- HAF_E_ARG: everything haf_score_frames refuses, a null rois or
 * mask, on_device not 0 or 1, a row stride smaller than the width, an engine created with HAF_FLAG_PROBABILITY; HAF_E_CAPACITY as
 * haf_score_frames.  The first call allocates the ROI cell sets (one bit per cell of max_clouds x max_rolls_per_call grids) and the
 * area of uploaded host masks (max_points bytes).  Fused views take masks through haf_score_views_roi, below.  Not through
 * haf_score_rolls or the sharded multi-GPU calls. */
int  haf_score_frames_roi(haf_engine *e, int32_t n, const haf_frame *frames, const haf_roi *rois, const haf_grasp_input *in,
                          haf_grasp_output *out);
/* ---- fused views under per-view masks (csrc/roi.hip: k_roi_mark_view) -------------------------------------------------------
 * haf_score_views with a mask per VIEW: the fused scene of two cameras, evaluated only near one object.  rois[i] goes with frames[i],
 * the flat view index of haf_score_views.  A view whose rois[i].mask is NULL contributes its points and selects nothing (a camera
 * without a segmenter); its on_device and row_stride_bytes are ignored.
 *   cloud             of request b: exactly haf_score_views' cloud, every valid point of every view, masked or not;
 *   ROI cells S_r     the UNION over the request's views of the cells haf_point_cells gives the haf_frame_points points of that view's
 *                     masked pixels whose point is finite in all three components;
 *   E_r, V'_r, the record of roll r, n_evals and the output follow from S_r word for word as above, V being the vote of the full
 *                     haf_score_views request on the same views.
 * This is NOT haf_score_frames_roi on one of the cameras: the height grids are the fused scene's, so labels and votes differ wherever
 * the second camera fills what the first one does not see.  n_points as in haf_score_views.  A request whose S_r is empty in every roll
 * (every mask NULL, zero, or over invalid pixels only) returns "nothing found" (eval = -20, n_evals = 0) and HAF_OK.  Afterwards the
 * last-batch state is the restricted request's for every call that reads it, as after haf_score_frames_roi, and the call never
 * re-chooses the form of the screening pass.  One kernel launch per frame kind present in the batch marks the cells of all its views.
 * Checked before any device work, a refused call leaves the engine as it was, the message names the request and the view; view after
 * view, a view's frame before its mask: everything haf_score_views refuses; HAF_E_ARG: a null rois, an engine created with
 * HAF_FLAG_PROBABILITY, for a non-null mask an on_device that is not 0 or 1 or a row stride smaller than the width.  Shares the ROI
 * buffers of haf_score_frames_roi (the masks' area: max_points bytes and 16 per view).
 *
 * haf_roi_cells_views: the host definition of record, no device, no engine.  roi = the OR of haf_roi_cells over the views that have a
 * mask, eval = its T-dilation; either may be NULL; all zero when no view has a mask.  Host frames and host masks only.  Refusals per
 * view as haf_roi_cells (a NULL mask is no refusal here), plus a null frames or rois and n_views outside 1..HAF_MAX_VIEWS; every view is
 * checked before anything is written. */
int  haf_score_views_roi(haf_engine *e, int32_t n, const int32_t *views_per_request, const haf_frame *frames, const haf_roi *rois,
                         const haf_grasp_input *in, haf_grasp_output *out, int64_t *n_points);
int  haf_roi_cells_views(const haf_config *cfg, const haf_grasp_input *in, int32_t roll, const haf_frame *frames, const haf_roi *rois,
                         int32_t n_views, uint8_t *roi, uint8_t *eval);

/* ---- conditioning depth frames on the device: 1..8 exposures of one camera -> one depth image (csrc/depthfilter.hip) -------------
 * frames[0..n_frames) are exposures of ONE depth camera in one pose: the same kind (U16 or F32), width, height, depth_scale, min_depth
 * and max_depth (floats compared by value); strides and residence may differ.  The result is one depth image of that kind, just
 * another haf_frame for every call above.  Two stages, one pass:
 *
 * Stage T, temporal selection.  Per pixel the VALID samples of the exposures -- valid exactly as haf_frame defines it above: U16
 * d != 0, F32 d finite and > 0, both z = (float)d * depth_scale finite and inside min_depth / max_depth.  c = their number.  c <
 * min_valid: the pixel is invalid.  Otherwise M = the LOWER MEDIAN, the sample of 0-based rank (c - 1) / 2 in ascending order (U16
 * compare as integers, F32 as floats).  M is one of the input samples bit for bit; no arithmetic is performed.
 *
 * Stage S, spatial support.  For a pixel p with a valid M_p: z_p = (float)M_p * depth_scale, t_p = tol_abs + tol_rel * z_p;
 * support(p) = the number of pixels q != p with |u_q - u_p| <= radius, |v_q - v_p| <= radius, inside the image, M_q valid and
 * fabs(z_q - z_p) <= t_p.  Every step one correctly rounded fp32 operation, never a fused multiply-add; fabs clears the sign bit.
 * Pixels outside the image do not count (a corner with radius 1 has 3 candidates).  p is kept when support(p) >= min_support;
 * min_support = 0 switches the stage off.  Support is counted on stage T's image, not on the filtered one.
 *
 * Output: M_p for a kept pixel; for every other pixel the invalid sample -- 0 (U16), the word 0x7FC00000 (F32).  Every output sample
 * is therefore invalid or valid under the same frame parameters.
 *
 * stats (may be NULL): [0] pixels, [1] pixels valid after stage T, [2] pixels kept.
 * out: samples of the input kind, rows out_row_stride_bytes apart (>= width * element size, a multiple of the element size, data
 * aligned to the element); bytes between a row's end and the next row are not written; must not overlap an input.
 *
 * haf_filter_depth_ref: the host definition of record -- no device, no engine, host frames and host output only.
 * haf_filter_depth: equal to it in every word and in stats.  out_on_device = 1: out is the caller's device memory, written on the
 * current stream (haf_set_stream) and complete when the call returns; out == NULL with out_on_device = 1: the engine writes a packed image of its own
 * (4 bytes x max_points, allocated by the first call that asks for it, valid until the next haf_filter_depth or haf_destroy).
 * out_frame (may be NULL): a copy of frames[0] whose data, on_device and row_stride_bytes describe the output.  The call neither reads
 * nor changes last-batch state or stage timings, and works with HAF_FLAG_PROBABILITY and before any request.
 * Refusals, all before any device work, nothing written, the message naming the frame -- HAF_E_ARG: everything haf_score_frames
 * refuses for a frame, a null frames or p, n_frames outside 1..HAF_MAX_STACK, an XYZ frame, a frame that differs from frames[0] in a
 * field named above, a parameter outside its range or not finite, out_on_device not 0 or 1, out == NULL with out_on_device = 0, a
 * stride or alignment fault of out, out overlapping an input of the same residence, for the _ref form a device-resident frame;
 * HAF_E_CAPACITY: width * height > max_points, or the pixels of the host-resident frames plus one image for a host out > max_points
 * (what the raw staging area of haf_score_frames holds). */
#define HAF_MAX_STACK 8
typedef struct haf_depth_filter {
    int32_t radius;       /* 1..3: window (2 radius + 1)^2                                   */
    int32_t min_support;  /* 0..(2 radius + 1)^2 - 1; 0 = stage S off                        */
    float   tol_abs;      /* metres (units of z), finite, >= 0                               */
    float   tol_rel;      /* per metre of z_p, finite, >= 0                                  */
    int32_t min_valid;    /* 1..n_frames                                                     */
} haf_depth_filter;
void haf_depth_filter_default(haf_depth_filter *p);   /* 2, 6, 0.004f, 0.01f, 1 */
int  haf_filter_depth_ref(const haf_frame *frames, int32_t n_frames, const haf_depth_filter *p,
                          void *out, size_t out_row_stride_bytes, int64_t *stats /* [3], may be NULL */);
int  haf_filter_depth(haf_engine *e, const haf_frame *frames, int32_t n_frames, const haf_depth_filter *p,
                      void *out, size_t out_row_stride_bytes, int32_t out_on_device,
                      haf_frame *out_frame /* may be NULL */, int64_t *stats /* [3], may be NULL */);

/* ---- a depth frame into object labels on the device: geometric tabletop clustering (csrc/segment.hip) ---------------------------
 * The classic organised-cloud clustering, for the caller with one camera over a table and no segmenter: the label image every
 * haf_label_image and (as uint8) every haf_roi mask above asks for, from the frame itself.  It is geometry only -- a height band
 * over a plane the CALLER supplies (haf_fit_plane, below, estimates one from the same frame) and a distance between neighbouring
 * pixels' points; touching objects are one object.
 *
 *   point       pixel i = v * width + u has haf_frame_points' three words; any kind of frame.
 *   foreground  all three words finite (the rule of haf_view_points) and, with
 *               h = ((plane[0] x + plane[1] y) + plane[2] z) + plane[3], every step ONE correctly rounded fp32 operation in this order,
 *               never a fused multiply-add: h is no NaN, h >= min_height, and max_height <= 0 or h <= max_height.
 *   link        foreground pixels p, q that are horizontal or vertical neighbours inside the image: dx = x_q - x_p, dy, dz likewise,
 *               d2 = ((dx dx + dy dy) + dz dz), rounded as above; linked when d2 is finite and d2 <= gap2, gap2 = max_gap * max_gap
 *               formed once on the host in fp32.  Symmetric by construction: a - b = -(b - a) exactly.
 *   component   a connected component of the link graph; its ANCHOR is its lowest pixel index.
 *   labels      components of fewer than min_pixels pixels are background; the others are numbered 1, 2, ... in ascending order of
 *               anchor; those numbered above max_labels are background too.  *n_labels = min(kept, max_labels).  Every pixel of a
 *               numbered component carries its number, every other pixel 0.
 *   info[l - 1] the component's pixel count, its anchor and its inclusive bounding box (first *n_labels entries written).
 *   stats       [0] pixels, [1] foreground pixels, [2] components before the size rule, [3] components that pass it, before the cap.
 *   labels      elem_bytes 1 (uint8) or 2 (uint16, host byte order) per pixel, rows row_stride_bytes apart: strides and alignment as
 *               haf_label_image; bytes between rows are not written; must not overlap the frame.  A uint8 image is at the same time
 *               a valid haf_roi mask (a non-zero byte selects the pixel).
 * Nothing above depends on an order of evaluation: the result is one image, whoever computes it.
 *
 * haf_segment_ref: the host definition of record -- no device, no engine, a host frame and a host output only.
 * haf_segment_frame: equal to it in every label word, every info field, n_labels and stats.  out_on_device = 1: labels is the caller's
 * device memory, written on the current stream (haf_set_stream) and complete when the call returns; labels == NULL with out_on_device = 1: a packed
 * image the engine owns (2 bytes x max_points, allocated by the first call that asks for it), valid until the next haf_segment_frame,
 * haf_segment_cells, haf_transfer_labels or haf_destroy -- ACROSS scoring and map calls, which is its purpose.  out_image (may be NULL) describes the result for
 * haf_grasp_map_labels; its data as a uint8 image is a haf_roi mask.  The first call allocates the scratch: 8 bytes x max_points of
 * parent and size words, the per-label table and the copy-back block.  Like haf_filter_depth the call neither reads nor changes
 * last-batch state or stage timings, and works before any request and with HAF_FLAG_PROBABILITY.
 * Refusals, all before any device work, nothing written -- HAF_E_ARG: everything haf_score_frames refuses for a frame, a null frame, p
 * or n_labels, a plane entry or height that is not finite, max_gap not finite or not > 0, min_pixels < 1, max_labels outside
 * 1..HAF_MAX_LABELS (1..255 with elem_bytes 1), elem_bytes not 1 or 2, a stride or alignment fault of labels, out_on_device not 0 or
 * 1, labels == NULL with out_on_device = 0, labels overlapping a frame of the same residence, for the _ref form a device-resident
 * frame; HAF_E_CAPACITY: width * height > max_points. */
typedef struct haf_segment_params {
    float   plane[4];     /* height above the support, base frame: h = ((plane[0] x + plane[1] y) + plane[2] z) + plane[3] */
    float   min_height;   /* metres; foreground needs h >= min_height                                  */
    float   max_height;   /* metres; > 0: foreground needs h <= max_height; <= 0: no upper limit       */
    float   max_gap;      /* metres, finite, > 0: 4-neighbours closer than this are one object         */
    int32_t min_pixels;   /* >= 1: smaller components become background                                */
    int32_t max_labels;   /* 1..HAF_MAX_LABELS (1..255 when the output is uint8)                       */
} haf_segment_params;
typedef struct haf_segment_info {   /* label l is entry l - 1 */
    int32_t n_pixels, anchor_u, anchor_v, u_min, v_min, u_max, v_max;
} haf_segment_info;
void haf_segment_default(haf_segment_params *p);   /* (0,0,1,0), 0.01f, 0, 0.02f, 50, 255 */
int  haf_segment_ref(const haf_frame *frame, const haf_segment_params *p, void *labels, int32_t elem_bytes, size_t row_stride_bytes,
                     haf_segment_info *info /* [max_labels], may be NULL */, int32_t *n_labels, int64_t *stats /* [4], may be NULL */);
int  haf_segment_frame(haf_engine *e, const haf_frame *frame, const haf_segment_params *p, void *labels, int32_t elem_bytes,
                       size_t row_stride_bytes, int32_t out_on_device, haf_label_image *out_image /* may be NULL */,
                       haf_segment_info *info /* [max_labels], may be NULL */, int32_t *n_labels, int64_t *stats /* [4], may be NULL */);

/* ---- the support plane of a depth frame, estimated on the device (csrc/plane.hip) -------------------------------------------------
 * haf_segment_params.plane from the frame itself: the DOMINANT plane of the frame's points by a fixed set of three-point hypotheses
 * and an exact integer refit of the winner's inliers.  One plane per call; no multi-plane bins, no smoothing over time.
 *
 *   usable point  pixel i = v * width + u has haf_frame_points' three words.  It is usable when all three are finite, |x|, |y|, |z|
 *                 <= 16 m, and the mask -- a haf_roi over the frame, NULL or a NULL mask pointer meaning every pixel -- has a non-zero
 *                 byte there.  n_usable counts them; the RANK of a usable pixel is its position among them in raster order.
 *   sample        hypothesis k in [0, n_hyp), corner j in {0, 1, 2}: the usable pixel of rank
 *                 (uint64(mix32(seed + 3 k + j)) * n_usable) >> 32, seed + 3 k + j wrapping in 32 bits,
 *                 mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16  (uint32 throughout).
 *   hypothesis    a = p1 - p0, b = p2 - p0 componentwise; n = a x b, n0 = a1 b2 - a2 b1, n1 = a2 b0 - a0 b2, n2 = a0 b1 - a1 b0;
 *                 d = -((n0 x0 + n1 y0) + n2 z0); nn = (n0 n0 + n1 n1) + n2 n2.  Every step ONE correctly rounded fp32 operation in
 *                 the order written, never a fused multiply-add; the negation flips the sign bit.  VOID when two of its ranks coincide,
 *                 nn is not finite, nn <= min_area2, or -- up not all zero -- with c = (n0 up0 + n1 up1) + n2 up2 NOT
 *                 c c >= cos2 (nn uu); cos2 = (float)(cos(max_tilt)^2) and uu = (up0 up0 + up1 up1) + up2 up2 formed once on the host.
 *   score         usable point p: r = ((n0 x + n1 y) + n2 z) + d; an inlier of k when r r <= tol2 nn, tol2 = tol * tol formed once on
 *                 the host in fp32.  count[k] = the inliers of k, 0 for a void k.
 *   winner        the largest count[k], ties to the lowest k.  found = count[winner] >= min_inliers and n_usable >= 3.
 *   refit         over the winner's inliers, q = round-to-nearest-even(coordinate * 4096) as int32 (the product is exact, |q| <= 2^16):
 *                 the ten int64 moments N, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz of (qx, qy, qz).  All zero for a void winner.
 *   plane         found only; else plane = 0, rms = 0.  From the moments' covariance numerators N Sab - Sa Sb (exact, 128 bits) the
 *                 eigenvector of the smallest eigenvalue in double, d through the centroid, metres; oriented so that n . up > 0 when up
 *                 is given and not perpendicular, else so that the sensor's origin (sensor_to_base[3], [7], [11]) has h > 0; rounded to
 *                 float.  Where N < 3 or the two smallest eigenvalues coincide: the winning hypothesis, normalised and oriented.  rms =
 *                 sqrt of the inliers' mean squared distance to the plane, metres.  plane is a haf_segment_params.plane as it stands.
 *   stats         [0] pixels, [1] n_usable, [2] hypotheses that are not void, [3] count[winner].
 *   counts, hyps  (either may be NULL) count[k], and per k the four words n0, n1, n2, d (any NaN as 0x7FC00000; four such words when
 *                 n_usable = 0): what the two entry points are compared in.
 * Counts and moments are integers: no result depends on an order of evaluation.
 *
 * haf_fit_plane_ref: the host definition of record -- no device, no engine, a host frame and a host mask only.
 * haf_fit_plane: equal to it in every word of the result, of counts and of hyps; a host or device-resident frame, a host or
 * device-resident mask.  Like haf_segment_frame the call neither reads nor changes last-batch state or stage timings, works before any
 * request and with HAF_FLAG_PROBABILITY, and allocates its scratch (13 bytes x max_points, the copy-back block) on first use.
 * Refusals, all before any device work, nothing written -- HAF_E_ARG: everything haf_score_frames refuses for a frame, a null frame, p
 * or out, a parameter that is not finite, tol <= 0, min_area2 < 0, n_hyp outside 1..HAF_MAX_PLANE_HYP, min_inliers < 3, max_tilt
 * outside [0, pi/2], a mask stride smaller than the width, a mask's on_device not 0 or 1, for the _ref form a device-resident frame or
 * mask; HAF_E_CAPACITY: a frame of more than 2^28 pixels, width * height > max_points. */
#define HAF_MAX_PLANE_HYP 1024
typedef struct haf_plane_params {
    float    tol;         /* metres, finite, > 0: a point within tol of a hypothesis is its inlier                */
    float    min_area2;   /* m^4, finite, >= 0: hypotheses with |a x b|^2 <= this are void (collinear triples)   */
    float    up[3];       /* base frame; all zero: no tilt test, the normal points at the sensor                 */
    float    max_tilt;    /* radians in [0, pi/2]: largest angle between the plane's normal and +-up              */
    int32_t  n_hyp;       /* 1..HAF_MAX_PLANE_HYP                                                                */
    int32_t  min_inliers; /* >= 3                                                                                */
    uint32_t seed;
} haf_plane_params;
typedef struct haf_plane_result {
    float   plane[4];
    int32_t found, winner, n_inliers, reserved;
    double  rms;
    int64_t stats[4];
    int64_t moments[10];
} haf_plane_result;
void haf_plane_default(haf_plane_params *p);   /* 0.005f, 1e-6f, (0,0,0), 0, 256, 100, 1 */
int  haf_fit_plane_ref(const haf_frame *frame, const haf_roi *mask /* may be NULL */, const haf_plane_params *p, haf_plane_result *out,
                       int32_t *counts /* [n_hyp], may be NULL */, float *hyps /* [n_hyp][4], may be NULL */);
int  haf_fit_plane(haf_engine *e, const haf_frame *frame, const haf_roi *mask /* may be NULL */, const haf_plane_params *p,
                   haf_plane_result *out, int32_t *counts /* [n_hyp], may be NULL */, float *hyps /* [n_hyp][4], may be NULL */);

/* ---- every object's box in the base frame, and a request per object (csrc/labelshape.hip) ----------------------------------------
 * What a label image lacks to become one request per object: WHERE each object is (the centre of its request), how LARGE it is (the
 * request's window) and how WIDE it is at its narrowest, in which direction (does the gripper span it, which roll is plausible).
 * haf_segment_info only has pixel counts and pixel boxes; this is the geometry per label in the base frame.
 *
 *   point       pixel i = v * width + u has haf_frame_points' three words; any kind of frame.
 *   label       l = the label image's value at i, read as haf_grasp_map_labels reads it; 0 and values above n_labels are ignored.
 *   usable      all three words finite and of magnitude <= 16 m (haf_fit_plane's rule).
 *   words       q = round-to-nearest-even(coordinate * 4096) as int32, haf_fit_plane's refit word: exact product, |q| <= 2^16.
 *   per label   in integers only -- n_pixels: all pixels carrying l; over the USABLE ones: n_points, sum[3] (int64 sums of qx, qy,
 *               qz), q_min[3], q_max[3], and for k in [0, HAF_SHAPE_DIRS): t_k = C[k] qx + S[k] qy in int32, t_min[k], t_max[k].
 *   directions  (C, S)[k] = round(8192 (cos, sin)(15 deg k)): HAF_SHAPE_COS, HAF_SHAPE_SIN below, their squared norms HAF_SHAPE_NN.
 *               (C, S)[k + 6] = (-S, C)[k] exactly: k and (k + 6) mod 12 are perpendicular and of equal norm.  |t| <= 2^16 x 11586
 *               < 2^30: no overflow.
 *   height      with a plane[4] (may be NULL): h = ((plane[0] x + plane[1] y) + plane[2] z) + plane[3], haf_segment_frame's height to
 *               the bit; h_max = the largest non-NaN h of the usable pixels, -0 below +0.
 *   empty       a label without a usable point: sums 0, mins INT32_MAX, maxes INT32_MIN, h_max the word 0x7FC00000 -- as h_max of
 *               every label is without a plane.
 * No value depends on an order of evaluation, the float maximum included.
 *
 * The derived fields come from those integers through ONE host function both entry points call, in double, rounded once to float:
 * found = n_points > 0; centroid = sum / (4096 n_points); box_min / box_max = q / 4096; width[k] = (t_max - t_min) / (4096
 * sqrt(nn[k])); narrow_dir = the k that minimises (t_max - t_min)^2 / nn[k], compared exactly by 128-bit cross products, ties to the
 * lowest k; narrow_width = width[narrow_dir], long_width = width[(narrow_dir + 6) % 12], yaw = narrow_dir x 15 deg in radians,
 * diameter = the largest width[k], height = h_max.  All of them zero when not found.
 * This is the minimum-width box over a FIXED FAN of twelve directions, not the exact minimum-area rectangle, and the extents are those
 * of the QUANTISED points in the base frame's xy plane: meant for approach vectors near the base z.  It says nothing about how well a
 * sensor saw the object.
 *
 * haf_measure_labels_ref: the host definition of record -- no device, no engine, a host frame and a host image only.
 * haf_measure_labels: equal to it in every word of every entry.  The frame and the label image may each be host or device resident; a
 * device-resident one is read where it lies, with its strides -- the image haf_segment_frame left in the engine included.  One
 * device-to-host copy and one synchronisation whatever n_labels is.  Like haf_fit_plane the call neither reads nor changes last-batch
 * state or stage timings, works before any request and with HAF_FLAG_PROBABILITY, and allocates its table and copy-back block (160
 * bytes x HAF_MAX_LABELS and 2 bytes x max_points for a host image) on first use.
 * Refusals, all before any device work, nothing written -- HAF_E_ARG: everything haf_grasp_map_labels refuses for a frame and a label
 * image, a null shapes, a plane entry that is not finite, for the _ref form a device-resident frame or image; HAF_E_CAPACITY: width *
 * height > max_points.
 *
 * haf_object_input: pure host.  *out = *base with grasp_area_center[0], [1] = the midpoint of the box, (q_min + q_max) / 8192 in double
 * (z is base's), and grasp_area_length_x = grasp_area_length_y = 2 (ceil(50 diameter) + margin_cells + 7) clamped to [16, the even part
 * of min(grid_h, grid_w)]: the search interior 2 (length / 2 - 7) of the request then covers the object and the margin under every
 * roll.  *fits = 0 when the upper clamp acted, else 1.  HAF_E_ARG: a shape that is not found, margin_cells outside 0..64, a null
 * argument. */
#define HAF_SHAPE_DIRS 12
#define HAF_SHAPE_COS { 8192, 7913, 7094, 5793, 4096, 2120, 0, -2120, -4096, -5793, -7094, -7913 }
#define HAF_SHAPE_SIN { 0, 2120, 4096, 5793, 7094, 7913, 8192, 7913, 7094, 5793, 4096, 2120 }
#define HAF_SHAPE_NN  { 67108864, 67109969, 67102052, 67117698, 67102052, 67109969, 67108864, 67109969, 67102052, 67117698, 67102052, 67109969 }
typedef struct haf_label_shape {    /* label l is entry l - 1 */
    int64_t sum[3];                 /* of qx, qy, qz over the usable pixels */
    int32_t found, n_pixels, n_points, narrow_dir;
    int32_t q_min[3], q_max[3];
    int32_t t_min[HAF_SHAPE_DIRS], t_max[HAF_SHAPE_DIRS];
    float   h_max;                  /* 0x7FC00000: no plane, or no usable point */
    float   centroid[3], box_min[3], box_max[3];   /* metres, base frame */
    float   width[HAF_SHAPE_DIRS];  /* metres: the extent along direction k */
    float   narrow_width, long_width, yaw, diameter, height;
    int32_t reserved;               /* 0 */
} haf_label_shape;
int  haf_measure_labels_ref(const haf_frame *frame, const haf_label_image *labels, int32_t n_labels, const float *plane /* [4], may be NULL */,
                            haf_label_shape *shapes /* [n_labels] */);
int  haf_measure_labels(haf_engine *e, const haf_frame *frame, const haf_label_image *labels, int32_t n_labels,
                        const float *plane /* [4], may be NULL */, haf_label_shape *shapes /* [n_labels] */);
int  haf_object_input(const haf_config *cfg, const haf_grasp_input *base, const haf_label_shape *shape, int32_t margin_cells,
                      haf_grasp_input *out, int32_t *fits);

/* ---- every labelled object scored in one call (csrc/engine_objects.cpp, csrc/roi.hip: k_roi_mark_objects, csrc/graspmap.hip:
 * k_map_labels_objects) --------------------------------------------------------------------------------------------------------
 * The last link of filter -> plane -> segment -> measure -> one request per object: ONE frame, ONE instance-label image, and per
 * listed object b its label object_labels[b] and its own request in[b] (haf_object_input's).  The definition of record is a
 * composition of calls that exist; no new arithmetic is defined:
 *   request b     haf_score_frames_roi(e, 1, frame, &roi_b, &in[b], &out[b]) with roi_b the 8-bit mask `labels == object_labels[b]`;
 *   picks[b]      entry object_labels[b] - 1 of haf_grasp_map_labels(e, 0, frame, labels, n_labels, min_vote, ...) after that request,
 *   poses[b]      and its pose (zeroed when not found);
 *   order         order[0 .. *n_found) lists the INDICES b of the found objects, best first by haf_grasp_map_labels' key (vote
 *                 descending, roll ascending, pixel index ascending).
 * The call equals that composition in every field of out, picks, poses, order and n_found, n_evals of the records included -- which is
 * why the mask of request b is its own object's label and not `labels != 0`.  The one field that is counted per BATCH, as in every
 * batched call, is n_rechecked: out[0] carries the batch's, the others 0 (which tier decides an evaluation is no part of any contract
 * here, see haf_score_frames_roi).  Two further facts:
 *   * the picks, though not n_evals, also equal those of one request per object under the mask `labels != 0`: every labelled pixel's
 *     cell lies in S_r under either mask, so V'_r = V_r there (the argument under haf_grasp_map_labels);
 *   * request b evaluates only the cells near its own object: E_r of request b follows from the pixels of label object_labels[b] alone.
 * A label of the image that is not listed, and a value above n_labels, select nothing in any request.
 *
 * Afterwards the last scored batch is a batch of n_objects ROI requests, exactly as haf_score_frames_roi(e, n_objects, {frame x n},
 * {roi_b}, in, out) leaves it: haf_top_grasps, haf_grasp_map, haf_cell_pose, haf_get_roll_grid, haf_last_counts,
 * haf_debug_fetch(HAF_DBG_ROI) and haf_debug_fetch_points describe request b.  Like every ROI call it never re-chooses the form of the
 * screening pass.
 *
 * What is done once instead of n_objects times: a host frame is packed and uploaded once, a device-resident one read where it lies;
 * the frame is deprojected once and every request reads that one set of points; the frame counts ONCE against max_points (width x
 * height <= max_points whatever n_objects is); a host label image is uploaded once, a device-resident one -- the image
 * haf_segment_frame left in the engine included -- is read in place with its stride; one launch marks the cell sets of all requests;
 * one launch pair, one device-to-host copy and one synchronisation give all picks, behind the request path's own copy and wait.
 *
 * Refusals, all before any device work, the engine left as it was -- everything haf_score_frames_roi refuses for a frame and an input;
 * everything haf_grasp_map_labels refuses for a label image and n_labels (an engine created with HAF_FLAG_PROBABILITY included);
 * HAF_E_ARG: n_objects < 1, a null object_labels, in, out or picks, an object_labels[b] outside 1..n_labels, a label listed twice;
 * HAF_E_CAPACITY: n_objects > max_clouds.  A request whose budget is negative finds nothing and the call returns HAF_OK.  Not through
 * haf_score_rolls or the sharded multi-GPU calls.  Shares the ROI buffers of haf_score_frames_roi and the block of haf_grasp_map. */
int  haf_score_objects(haf_engine *e, const haf_frame *frame, const haf_label_image *labels, int32_t n_labels, int32_t n_objects,
                       const int32_t *object_labels /* [n_objects] */, const haf_grasp_input *in /* [n_objects] */, int32_t min_vote,
                       haf_grasp_output *out /* [n_objects] */, haf_label_pick *picks /* [n_objects] */,
                       haf_grasp_candidate *poses /* [n_objects], may be NULL */, int32_t *order /* [n_objects], may be NULL */,
                       int32_t *n_found /* may be NULL */);

/* ---- objects of any cloud by top-down cell clustering (csrc/cellsegment.hip) -------------------------------------------------------
 * haf_segment_frame links neighbouring PIXELS, so it needs an image: an unorganised cloud has none, an object cut in two in the image
 * becomes two labels, and neighbours of clearly different height are one.  This segmenter's neighbourhood is the scene's: it clusters
 * the occupied cells of the top-down grid, the view a height-accumulated feature has of the world.  A frame of any shape is accepted
 * -- an N x 1 HAF_FRAME_XYZ_F32 frame with the identity pose is an unorganised cloud -- and the label image has the frame's shape, so
 * haf_measure_labels and haf_score_objects follow as they follow haf_segment_frame.  The rules are csrc/cell_segment_rules.h's; every
 * floating-point step is ONE correctly rounded fp32 operation in the stated order, never fused.
 *
 *   point       pixel i = v * width + u has haf_frame_points' three words; any kind and shape of frame.
 *   foreground  each word finite and |w| <= 16 m (haf_fit_plane's usable point) and haf_segment_frame's height band: plane,
 *               min_height and max_height have exactly its meaning.
 *   cell        fx = (x - x0) * inv_cell, fy = (y - y0) * inv_cell, inv_cell = 1.0f / cell formed once on the host.  The point is in
 *               the grid when fx >= 0 && fx < (float)nx and likewise fy; then ix = (int)floorf(fx), iy = (int)floorf(fy) and the cell
 *               index is iy * nx + ix.  A point just below x0 is outside the grid, never cell 0.
 *   per cell    count = the number of its foreground points; top = their largest h; occupied when count > 0.
 *   link        two occupied cells that share an edge -- or also a corner with connectivity 8 -- are linked when max_step <= 0 or
 *               fabsf(top_a - top_b) <= max_step; the difference is one subtraction, so the rule is symmetric.
 *   component   a connected component of the link graph; its ANCHOR is its lowest cell index.
 *   labels      components whose summed count is below min_points are background; the others are numbered 1, 2, ... in ascending
 *               order of anchor; those numbered above max_labels are background too.  *n_labels = min(kept, max_labels).  A pixel
 *               carries its cell's number when it is foreground and in the grid, 0 otherwise.
 *   info[l - 1] n_points, n_cells, the anchor cell, the inclusive box of its cells and top, the largest top of its cells (first
 *               *n_labels entries written).
 *   stats       [0] pixels, [1] foreground, [2] foreground outside the grid, [3] occupied cells, [4] components, [5] components that
 *               pass the size rule, before the cap.
 *   cell_labels may be NULL; host memory, uint16 [ny][nx] packed: the top-down label grid.
 *   labels      as haf_segment_frame's: elem_bytes 1 or 2, strides, alignment, bytes between rows not written, no overlap.
 * Counts are integer sums, heights maxima through an ordered key, unions minima: nothing depends on an order of arrival.
 *
 * haf_segment_cells_ref: the host definition of record -- no device, no engine, a host frame and host outputs only.
 * haf_segment_cells: equal to it in every label word, info field, cell_labels word, n_labels and stat.  The output conventions are
 * exactly haf_segment_frame's, the engine's own image (labels == NULL with out_on_device = 1) is the SAME image for both segmenters.
 * Scratch is allocated at first use and grown when nx * ny or the frame grows: one int32 cell word per pixel; count, top key, parent
 * and size / label words per cell; the per-label tables and the copy-back block.  The call neither reads nor changes last-batch
 * state or stage timings, and works before any request and with HAF_FLAG_PROBABILITY.
 * Refusals, all before any device work, nothing written -- everything haf_segment_frame refuses for its frame and its label output;
 * HAF_E_ARG: a plane entry, height or max_step that is not finite, cell outside 0.001..1, |x0| or |y0| > 64 (or not finite), nx or
 * ny outside 1..4096, nx * ny > 2^22, connectivity not 4 or 8, min_points < 1, max_labels as haf_segment_params, for the _ref form
 * a device-resident frame; HAF_E_CAPACITY: width * height > max_points. */
#define HAF_MAX_CELLS (1 << 22)
typedef struct haf_cell_segment_params {
    float   plane[4];      /* as haf_segment_params.plane                                              */
    float   min_height;    /* as haf_segment_params                                                    */
    float   max_height;    /* as haf_segment_params: <= 0 is no upper limit                            */
    float   cell;          /* metres, 0.001..1: the edge of a grid cell                                */
    float   x0, y0;        /* base frame, |.| <= 64: the corner of cell (0, 0)                         */
    int32_t nx, ny;        /* 1..4096 each, nx * ny <= HAF_MAX_CELLS                                   */
    int32_t connectivity;  /* 4 or 8                                                                   */
    float   max_step;      /* metres, finite; > 0: neighbours whose tops differ by more do not link    */
    int32_t min_points;    /* >= 1: components of fewer foreground points become background            */
    int32_t max_labels;    /* 1..HAF_MAX_LABELS (1..255 when the output is uint8)                      */
} haf_cell_segment_params;
typedef struct haf_cell_segment_info {   /* label l is entry l - 1 */
    int32_t n_points, n_cells, anchor_ix, anchor_iy, ix_min, iy_min, ix_max, iy_max;
    float   top;
} haf_cell_segment_info;
void haf_cell_segment_default(haf_cell_segment_params *p);   /* (0,0,1,0), 0.01f, 0, 0.01f, (-5.12f, -5.12f), 1024 x 1024, 8, 0, 50, 255 */
int  haf_segment_cells_ref(const haf_frame *frame, const haf_cell_segment_params *p, void *labels, int32_t elem_bytes,
                           size_t row_stride_bytes, uint16_t *cell_labels /* [ny][nx], may be NULL */,
                           haf_cell_segment_info *info /* [max_labels], may be NULL */, int32_t *n_labels,
                           int64_t *stats /* [6], may be NULL */);
int  haf_segment_cells(haf_engine *e, const haf_frame *frame, const haf_cell_segment_params *p, void *labels, int32_t elem_bytes,
                       size_t row_stride_bytes, int32_t out_on_device, haf_label_image *out_image /* may be NULL */,
                       uint16_t *cell_labels /* [ny][nx], host, may be NULL */, haf_cell_segment_info *info /* [max_labels], may be NULL */,
                       int32_t *n_labels, int64_t *stats /* [6], may be NULL */);

/* ---- another camera's label image on a depth frame (csrc/transfer.hip) -------------------------------------------------------------
 * Every object-level call above takes a label image that lies on the depth frame's pixels.  An instance segmenter runs on the COLOUR
 * image: another camera, with its own intrinsics, a baseline of some centimetres against the depth sensor, often another resolution.
 * This call carries such an image over, and it is not a nearest-pixel lookup: a depth pixel the colour camera cannot see, because an
 * object stands in front of it, must not take that object's label (the table behind a mug would become "mug").  So it is the classic
 * two passes: a z-buffer of the depth frame's points in the camera's image, then a gather that keeps a label only where the point is
 * the one the camera sees.  The rules are csrc/transfer_rules.h's.  Only the transform into the camera's frame is floating point --
 * ONE correctly rounded fp32 operation per step, never fused; everything behind it is integer arithmetic, so no result depends on a
 * division unit or on the order in which atomics arrive.
 *
 * Constants, formed once on the host in double (rne: round to nearest even): FX = rne(fx * 256), FY, CX, CY likewise, as int32;
 * NEAR = max(1, rne(near_m * 65536)); TA = rne(tol_abs * 65536) clamped to int32; TR = rne(tol_rel * 65536).
 * Per pixel i = v * width + u of the DEPTH frame, which may be of any kind:
 *   point       p = haf_frame_points' three words; the pixel is unlabelled (output 0) unless all three are finite.
 *   camera      q[r] = ((m[r][0] p0 + m[r][1] p1) + m[r][2] p2) + m[r][3], m = base_to_camera, left to right.  Unlabelled unless every
 *               q[r] is finite and |q[r]| <= 16.  Q[r] = rne(q[r] * 65536) as int32 (the product is exact, |Q| <= 2^20).  Unlabelled
 *               unless Qz >= NEAR; the pixels that pass are stats[1].
 *   projection  in int64: d = 256 Qz, nu = FX Qx + (CX + 128) Qz, nv = FY Qy + (CY + 128) Qz.  The point PROJECTS when
 *               0 <= nu < width_c d and 0 <= nv < height_c d; then uc = nu div d, vc = nv div d -- the nearest pixel to fx x / z + cx.
 *               Projecting pixels are stats[2].
 *   z-buffer    Z[vc'][uc'] = the minimum of Qz over all projecting pixels and all (uc', vc') with |uc' - uc| <= splat and
 *               |vc' - vc| <= splat inside the camera image; a word no point reached holds INT32_MAX.
 *   visible     Qz - Z[vc][uc] <= TA + ((int64)TR * Z[vc][uc] >> 16).  Visible pixels are stats[3].
 *   label       L = the camera label image's value at (uc, vc), read as haf_grasp_map_labels reads a haf_label_image (0 and values
 *               above n_labels count as 0).  The output pixel is L when visible, else 0; non-zero outputs are stats[4].  stats[0] is
 *               the number of pixels.
 * Outputs: the label image on the depth frame with exactly haf_segment_frame's conventions -- uint8 (n_labels <= 255) or uint16; a
 * host image with a stride, the caller's device image, or (labels == NULL with out_on_device = 1) the engine's own image, which is the
 * SAME one image the two segmenters use, valid until the next call of any of the three; out_image describes the result.  zbuffer (may
 * be NULL): host memory, int32 [height_c][width_c], the words of Z.
 *
 * haf_invert_pose: pure host.  The inverse of the general 3x4 affine, in double by the adjugate, rounded once to float; HAF_E_ARG for
 * an entry that is not finite or a determinant whose magnitude is below 1e-12.  base_to_camera = the inverse of the camera's
 * sensor_to_base.
 * haf_transfer_labels_ref: the host definition of record -- no device, no engine, a host frame, host images and host outputs only.
 * haf_transfer_labels: equal to it in every label word, every zbuffer word and every stat.  The depth frame and the camera label image
 * may each be host or device resident; a device-resident one is read where it lies, with its strides.  A fill, two launches and one
 * copy back on the current stream.  Like the segmenters the call neither reads nor changes last-batch state or stage timings, and
 * works before any request and with HAF_FLAG_PROBABILITY.  Scratch, allocated on first use: 4 bytes per camera pixel, grown on
 * demand, and the copy-back block (a host output image and a host camera label image, 2 bytes x max_points each).
 * Refusals, all before any device work, nothing written -- everything haf_segment_frame refuses for its frame and its label output;
 * everything haf_grasp_map_labels refuses for a label image and n_labels (and n_labels > 255 with a uint8 output); HAF_E_ARG: a null
 * cam, cam_labels or p, a camera or parameter field outside the ranges below or not finite, the camera label image overlapping the
 * output in the same residence (the engine's own image given as BOTH included), for the _ref form anything device-resident;
 * HAF_E_CAPACITY: width * height of the depth frame or of the camera > max_points. */
typedef struct haf_camera {            /* the camera the label image belongs to: a rectified pinhole image */
    int32_t width, height;             /* 1..32768 each */
    float   fx, fy, cx, cy;            /* pixels; fx, fy in [1/256, 32768], |cx|, |cy| <= 32768, all finite */
    float   base_to_camera[12];        /* rows 0..2 of the 4x4, row-major: base frame -> this camera's frame */
} haf_camera;
typedef struct haf_transfer_params {
    float   near_m;                    /* metres, finite, in [0.001, 16]: points nearer to the camera plane are not projected */
    float   tol_abs, tol_rel;          /* metres, and per metre of the z-buffer's value; finite, >= 0, tol_rel <= 1 */
    int32_t splat;                     /* 0..2: a point enters the z-buffer in the (2 splat + 1)^2 pixels around its own */
} haf_transfer_params;
void haf_transfer_default(haf_transfer_params *p);      /* 0.05f, 0.01f, 0.01f, 1 */
int  haf_invert_pose(const float pose[12], float inverse[12]);
int  haf_transfer_labels_ref(const haf_frame *depth, const haf_camera *cam, const haf_label_image *cam_labels, int32_t n_labels,
                             const haf_transfer_params *p, void *labels, int32_t elem_bytes, size_t row_stride_bytes,
                             int32_t *zbuffer /* [height_c][width_c], may be NULL */, int64_t *stats /* [5], may be NULL */);
int  haf_transfer_labels(haf_engine *e, const haf_frame *depth, const haf_camera *cam, const haf_label_image *cam_labels, int32_t n_labels,
                         const haf_transfer_params *p, void *labels, int32_t elem_bytes, size_t row_stride_bytes, int32_t out_on_device,
                         haf_label_image *out_image /* may be NULL */, int32_t *zbuffer /* host, may be NULL */,
                         int64_t *stats /* [5], may be NULL */);

/* ---- does the gripper fit at a grasp pose: clearance against the scene's points, on the device (csrc/clearance.hip) ----------------
 * haf_score*, haf_top_grasps, haf_grasp_map_labels and haf_score_objects hand out grasp POSES; a vote says the height profile around a
 * cell resembles the graspable examples.  It does not say how far the object extends between the fingers, whether the fingertips land
 * in the table or in a neighbour, or whether the palm hits something taller beside the grasp.  This call counts the scene's points
 * inside the boxes of ONE parallel-jaw gripper placed at each of n_grasps poses.  Integers throughout: no result depends on an order
 * of evaluation.
 *
 *   scene point   pixel i of one haf_frame of any kind (an N x 1 HAF_FRAME_XYZ_F32 frame under the identity pose is an unorganised
 *                 cloud) has haf_frame_points' three words.  It is usable by haf_fit_plane's rule -- all three finite, magnitudes <= 16 m,
 *                 and the mask, a haf_roi over the frame (NULL or a NULL mask pointer: every pixel), non-zero there -- and enters as
 *                 its three words q = round-to-nearest-even(coordinate * 4096), haf_fit_plane's refit word.
 *   grasp         read from four fields of a haf_grasp_output, in double: a = approach_vector / |a|; g = grasp_point2 - grasp_point1;
 *                 c = g - (g . a) a, normalised: the closing axis; b = a x c.  Nine axis words A, B, C = lrint(16384 component), three
 *                 origin words o = lrint(4096 averaged_grasp_point).  VOID when any of the twelve doubles is not finite, |a| < 1e-6,
 *                 |g| < 1e-6, |c| < 1e-3 |g| or an |averaged_grasp_point_j| > 16: a void grasp counts nothing and comes back with free =
 *                 -1 and zeros elsewhere (the "nothing found" output of a request is one); it does not refuse the call.
 *   gripper       metres.  Along c: the fingers' inner faces at +-opening / 2, each finger_thickness thick.  Along b: finger_breadth,
 *                 centred.  Along a (u grows with approach_vector, which points from the scene toward the palm): the tips reach
 *                 tip_depth BELOW the grasp point, the fingers run finger_length from the tips up to the palm, a box of palm_width (c)
 *                 x palm_breadth (b) x palm_height (a) on top of them.  Bounds W(x) = llrint(x 2^26), formed once per call in double;
 *                 U0 = -W(tip_depth), U1 = W(finger_length - tip_depth).
 *   near          d = q - o.  A point is NEAR a grasp when |d_j| <= reach_q for j = 0, 1, 2; reach_q = ceil(4096 r) + 3 with r the
 *                 radius about the grasp point of the box that bounds all four regions.  Only near points are counted; no point inside
 *                 a region fails the test (csrc/clearance_rules.h has the proof).
 *   regions       of a near point: s = C . d, t = B . d, u = A . d, int32 dot products in units of 2^-26 m.  At most one of
 *                   between   -W(opening/2) < s < W(opening/2),  |t| <= W(finger_breadth/2),  U0 <= u < U1
 *                   finger 0  -W(opening/2 + finger_thickness) <= s <= -W(opening/2),  t and u as between
 *                   finger 1   W(opening/2) <= s <= W(opening/2 + finger_thickness),   t and u as between
 *                   palm      |s| <= W(palm_width/2),  |t| <= W(palm_breadth/2),  U1 <= u <= U1 + W(palm_height)
 *                 (tested in this order: it matters only for an opening below 2^-26 m.)
 *   row           n_near, n_finger[2], n_palm, n_between, and s_min, s_max, u_max over the between points (0 without one).
 *   derived       by ONE host function both entry points call: width_m = (s_max - s_min) 2^-26, the object's extent along the closing
 *                 axis; offset_m = (s_max + s_min) 2^-27, its centre's offset from the grasp point; top_m = u_max 2^-26, how far it
 *                 rises toward the palm; all 0 without a between point.  free = 1 when n_finger[0] + n_finger[1] + n_palm <= max_hits
 *                 and n_between >= min_between, else 0.  order (may be NULL): the indices of the grasps with free = 1, in input order;
 *                 *n_free (may be NULL) their number.
 * The defaults of haf_gripper_default are NOMINAL figures, no real gripper's drawing.  Not modelled: other gripper shapes, the arm
 * behind the palm.  An opening per grasp and the search for the smallest free one are haf_fit_openings' (below), not this call's.
 * Points are tested, not surfaces: a sparse cloud can let a finger through.
 *
 * grasps points at the first haf_grasp_output; grasp i is read at grasps + i * grasp_stride_bytes, so a haf_grasp_candidate[] of
 * haf_top_grasps or haf_grasp_map_labels goes in as it is with its sizeof as the stride.
 * haf_check_grasps_ref: the host definition of record -- no device, no engine, a host frame and a host mask only.
 * haf_check_grasps: equal to it in every word of every entry, of order and of n_free; a host or device-resident frame, a host or
 * device-resident mask; two launches, ONE copy back and ONE synchronisation.  Like haf_fit_plane the call neither reads nor changes
 * last-batch state or stage timings, works before any request and with HAF_FLAG_PROBABILITY, and allocates its scratch (12 bytes x
 * max_points, the copy-back block) on first use.
 * Refusals, all before any device work, nothing written -- HAF_E_ARG: everything haf_fit_plane refuses for a frame and a mask, a null
 * frame, gripper, grasps or out, a gripper dimension that is negative or not finite, opening <= 0, a reach r above 1 m, n_grasps
 * outside 1..HAF_MAX_CHECK_GRASPS, a stride below sizeof(haf_grasp_output) or not a multiple of 8, for the _ref form a device-resident
 * frame or mask; HAF_E_CAPACITY: a frame of more than 2^28 pixels, width * height > max_points. */
#define HAF_MAX_CHECK_GRASPS 4096
typedef struct haf_gripper {
    float   opening;            /* > 0: between the fingers' inner faces                                          */
    float   finger_thickness;   /* along the closing axis                                                        */
    float   finger_breadth;     /* across the closing axis and the approach vector                               */
    float   tip_depth;          /* how far the tips reach below the grasp point, against the approach vector     */
    float   finger_length;      /* from the tips up to the palm                                                  */
    float   palm_width, palm_breadth, palm_height;   /* along the closing axis, across it, along the approach vector */
    int32_t max_hits;           /* free: at most this many points in the fingers and the palm together           */
    int32_t min_between;        /* free: at least this many points between the fingers                           */
} haf_gripper;
typedef struct haf_grasp_clearance {
    int32_t free;               /* 1 free, 0 not, -1 a void grasp */
    int32_t n_near, n_finger[2], n_palm, n_between;
    int32_t s_min, s_max, u_max;   /* units of 2^-26 m, over the between points */
    int32_t reserved;
    double  width_m, offset_m, top_m;
} haf_grasp_clearance;
void haf_gripper_default(haf_gripper *g);   /* 0.08f, 0.01f, 0.02f, 0.03f, 0.06f, palm 0.12f x 0.04f x 0.04f, 0, 1 */
int  haf_check_grasps_ref(const haf_frame *frame, const haf_roi *mask /* may be NULL */, const haf_gripper *gripper, int32_t n_grasps,
                          const void *grasps, size_t grasp_stride_bytes, haf_grasp_clearance *out /* [n_grasps] */,
                          int32_t *order /* [n_grasps], may be NULL */, int32_t *n_free /* may be NULL */);
int  haf_check_grasps(haf_engine *e, const haf_frame *frame, const haf_roi *mask /* may be NULL */, const haf_gripper *gripper,
                      int32_t n_grasps, const void *grasps, size_t grasp_stride_bytes, haf_grasp_clearance *out /* [n_grasps] */,
                      int32_t *order /* [n_grasps], may be NULL */, int32_t *n_free /* may be NULL */);

/* ---- the smallest free opening at a grasp pose, and the sideways shift that goes with it (csrc/opening.hip) -------------------------
 * haf_check_grasps tests ONE opening, centred on the grasp point.  This call answers, for each of n_grasps poses and in one pass over
 * the scene's points, which is the smallest opening of the same gripper -- moved sideways along the closing axis by at most max_shift --
 * at which nothing lies in the fingers or the palm and the object lies between the fingers.  Integers throughout.
 *
 *   inputs        haf_check_grasps': one haf_frame of any kind, an optional haf_roi, a haf_gripper whose `opening`, max_hits and
 *                 min_between are NOT read, n_grasps in 1..HAF_MAX_CHECK_GRASPS read at a stride.  Scene points, the usable rule, a
 *                 grasp's twelve words, void grasps, s / t / u and every bound W() are exactly that call's (above).
 *   params        haf_opening_params: min_opening, max_opening, max_shift in metres; max_hits, min_between as haf_gripper's.
 *   slabs         of a near point.  finger slab: U0 <= u < U1, |t| <= W(finger_breadth/2).  palm slab: U1 <= u <= U1 + W(palm_height),
 *                 |t| <= W(palm_breadth/2).  Neither depends on the opening, and a point is in at most one.
 *   bin width     E = max(W(max_opening/2) + W(finger_thickness), W(palm_width/2)) + W(max_shift); shift = the smallest value >= 0 with
 *                 (E >> shift) + 2 <= 64; B = 1 << shift, in units of 2^-26 m; half_bins = (E >> shift) + 2.  (The default gripper and
 *                 parameters: shift 16, a bin of 0.98 mm; with max_shift = 1 cm: shift 17.)
 *   bin           bin(s) = s >= 0 ? s >> shift : ~((-s) >> shift), symmetric about 0: bin j >= 0 is [jB, (j+1)B), bin -j-1 is
 *                 (-(j+1)B, -jB].  A point at s = -jB belongs to finger 0 and one at s = +jB to finger 1, as in haf_check_grasps.
 *   histograms    per grasp two of HAF_OPEN_BINS = 128 uint32 words, finger slab then palm slab, word = bin + 64; only points with
 *                 -half_bins <= bin < half_bins are counted.
 *   near          haf_check_grasps' test with reach_q from the box es = half_bins B 2^-26 m along c, et and eu as there; a reach
 *                 above 1 m is refused.  No counted point fails it (csrc/opening_rules.h).
 *   placement     (j, c): a half opening of j bins, shifted by c bins.  tb = (W(finger_thickness) >> shift) + 1, pb = (W(palm_width/2)
 *                 >> shift) + 1, c_max = W(max_shift) >> shift, j_min = max(1, (W(min_opening/2) + B - 1) >> shift), j_max =
 *                 W(max_opening/2) >> shift.  Its bin sets: between = finger-slab bins [c-j, c+j); finger 0 = [c-j-tb, c-j); finger 1 =
 *                 [c+j, c+j+tb); palm = palm-slab bins [c-pb, c+pb).  All of them lie inside [-63, 63) (csrc/opening_rules.h).
 *   result        a placement is FREE when finger 0 + finger 1 + palm <= max_hits and between >= min_between.  The result is the first
 *                 free placement in the order j ascending, |c| ascending, c ascending over j_min..j_max, -c_max..c_max; sym_j is the
 *                 first free j with c = 0, 0 when there is none.
 *   row           found (1, 0, or -1 for a void grasp, zeros elsewhere), j, c, sym_j, the four counts at the chosen placement (0
 *                 without one), the two slabs' totals over the counted bins, and by ONE host function both entry points call:
 *                 opening_m = 2 j B 2^-26, shift_m = c B 2^-26, sym_opening_m = 2 sym_j B 2^-26.
 *   order         (may be NULL) the indices of the grasps with found = 1, in input order; *n_found (may be NULL) their number.
 *   info          (may be NULL) shift, half_bins, tb, pb, j_min, j_max, c_max and bin_m = B 2^-26.
 *   hist          (may be NULL) uint32 [n_grasps][2][HAF_OPEN_BINS]: the histograms, copied back only when asked for.
 * Relation to haf_check_grasps: with opening = sym_opening_m (exact in float32), max_hits and min_between the parameters' and all else
 * equal, that call reports the same n_between, n_finger[i] <= ours and n_palm <= ours (its finger is W(finger_thickness) thick against
 * tb B > that, its palm W(palm_width/2) wide against pb B > that): found at c = 0 implies free = 1 there.
 * Not modelled: a thickness or a palm per finger (one of each is shared), shapes other than boxes, surfaces (points are tested: a sparse
 * cloud can let a finger through); the resolution of an opening and of a shift is one bin.
 *
 * haf_fit_openings_ref: the host definition of record -- no device, no engine, a host frame and a host mask only.
 * haf_fit_openings: equal to it in every word of every row, of order, n_found, info and the histograms; a host or device-resident
 * frame and mask; three launches on the engine's stream (the points' words, grasps x points into the histograms, one wave's search per
 * grasp), ONE copy back and ONE synchronisation.  Like haf_check_grasps it neither reads nor changes last-batch state or stage
 * timings and shares that call's block and scratch (12 bytes x max_points and 1 KiB per grasp).
 * haf_apply_opening (host only, double): *out = *in with averaged_grasp_point moved by shift_m along the closing axis (the c of
 * haf_check_grasps' grasp, from in's own fields) and grasp_point1 / 2 at -+ opening_m / 2 about it; everything else copied.
 * HAF_E_ARG for a null pointer, an opening with found != 1 or a void grasp.
 * Refusals, all before any work, nothing written -- everything haf_check_grasps refuses (the gripper's opening aside), and HAF_E_ARG
 * for null params, a parameter that is not finite or negative, min_opening > max_opening, j_max < j_min, a reach above 1 m. */
#define HAF_OPEN_BINS 128
typedef struct haf_opening_params {
    float   min_opening, max_opening;   /* between the fingers' inner faces, metres                                  */
    float   max_shift;                  /* the gripper's centre may move this far from the grasp point, either way   */
    int32_t max_hits, min_between;      /* as haf_gripper's                                                          */
} haf_opening_params;
typedef struct haf_grasp_opening {
    int32_t found;                      /* 1 a free placement, 0 none, -1 a void grasp */
    int32_t j, c, sym_j;                /* bins */
    int32_t n_between, n_finger[2], n_palm;      /* at the chosen placement */
    int32_t n_finger_slab, n_palm_slab;          /* the histograms' totals  */
    double  opening_m, shift_m, sym_opening_m;
} haf_grasp_opening;
typedef struct haf_opening_info {
    int32_t shift, half_bins, tb, pb, j_min, j_max, c_max, reserved;
    double  bin_m;
} haf_opening_info;
void haf_opening_default(haf_opening_params *p);   /* 0.01f, 0.08f, 0.0f, 0, 1 */
int  haf_fit_openings_ref(const haf_frame *frame, const haf_roi *mask /* may be NULL */, const haf_gripper *gripper,
                          const haf_opening_params *params, int32_t n_grasps, const void *grasps, size_t grasp_stride_bytes,
                          haf_grasp_opening *out /* [n_grasps] */, int32_t *order /* [n_grasps], may be NULL */,
                          int32_t *n_found /* may be NULL */, haf_opening_info *info /* may be NULL */, uint32_t *hist /* may be NULL */);
int  haf_fit_openings(haf_engine *e, const haf_frame *frame, const haf_roi *mask /* may be NULL */, const haf_gripper *gripper,
                      const haf_opening_params *params, int32_t n_grasps, const void *grasps, size_t grasp_stride_bytes,
                      haf_grasp_opening *out /* [n_grasps] */, int32_t *order /* [n_grasps], may be NULL */,
                      int32_t *n_found /* may be NULL */, haf_opening_info *info /* may be NULL */, uint32_t *hist /* host, may be NULL */);
int  haf_apply_opening(const haf_grasp_output *in, const haf_grasp_opening *opening, haf_grasp_output *out);

/* ---- is the gripper's volume SEEN to be empty: sample points against depth views, on the device (csrc/space.hip) --------------------
 * haf_check_grasps and haf_fit_openings test points, not surfaces: where a depth camera returned nothing -- behind an object, under an
 * overhang, where it got no return -- they count zero points and report a free gripper.  This call asks the opposite question: a
 * finger may only go where a camera has seen THROUGH the space.  A depth pixel's ray is empty up to its depth, hits a surface at its
 * depth and is unknown behind it; a second view turns "unknown" into "seen empty".  For each of n_grasps poses the call lays a fixed
 * lattice of sample points inside the gripper's four boxes and classifies every sample against 1..HAF_MAX_SPACE_VIEWS depth views.
 * The rules are csrc/space_rules.h's.  Everything behind one fp32 transform per view is integer arithmetic: no result depends on an
 * order of evaluation or on the order in which atomics arrive.
 *
 *   views         views[n_views], HAF_FRAME_DEPTH_U16 or HAF_FRAME_DEPTH_F32 (an XYZ frame has no rays), each with its own size,
 *                 intrinsics, pose and residence.  View k is read as the camera haf_transfer_labels would call haf_camera{width,
 *                 height, fx, fy, cx, cy, base_to_camera = haf_invert_pose(sensor_to_base)}: FX, FY, CX, CY as there, and NEAR, TA, TR
 *                 from this call's near_m, tol_abs, tol_rel as there.  Pixel (u, v) has depth z by haf_frame's depth rule (depth_scale,
 *                 min_depth, max_depth; d == 0, a d that is not finite or <= 0 invalid); its observed word is Zobs = rne(z * 65536),
 *                 and 2^20 for a valid z above 16 m.
 *   grasps        haf_check_grasps': the twelve words A, B, C, o of a grasp, the void rule, the bounds W() of the haf_gripper (max_hits
 *                 and min_between are NOT read), a reach above 1 m refused.
 *   lattice       one per call, the same for every grasp.  S = W(sample_step).  Boxes in (s, t, u), units of 2^-26 m:
 *                   between   [-W(opening/2), W(opening/2)] x [-W(finger_breadth/2), W(finger_breadth/2)] x [U0, U1]
 *                   finger 0  [-W(opening/2 + finger_thickness), -W(opening/2)] x the same t and u
 *                   finger 1  [W(opening/2), W(opening/2 + finger_thickness)] x the same t and u
 *                   palm      [-W(palm_width/2), W(palm_width/2)] x [-W(palm_breadth/2), W(palm_breadth/2)] x [U1, U1 + W(palm_height)]
 *                 Per axis of a box [lo, hi]: n = max(1, (hi - lo) / S); sample k of n lies at lo + ((2k + 1)(hi - lo)) / (2n), int64,
 *                 both divisions truncating.  A region with a dimension of 0 has no samples (its three n are 0).  Sample index:
 *                 region-major in the order above, then u, then t, with s fastest.  N = all samples <= HAF_MAX_SPACE_SAMPLES.
 *   sample point  in int64, units of 2^-40 m: P_j = o_j 2^28 + s C_j + t B_j + u A_j;  Pq_j = (P_j + 2^23) >> 24, an arithmetic
 *                 shift: a word of 1/65536 m;  p_j = (float)Pq_j * (1.0f / 65536), exact.
 *   per view      haf_transfer_labels' projection of p, unchanged: q = base_to_camera p in twelve rounded fp32 operations, Q = rne(q *
 *                 65536), Qz >= NEAR, the pixel (uc, vc).  The sample is UNSEEN in the view when it does not project or the pixel is
 *                 invalid.  Otherwise tol = TA + ((int64)TR * Zobs >> 16) and D = Qz - Zobs:  D > tol HIDDEN (behind the surface the
 *                 ray hit);  D < -tol FREE (the ray went through it);  else HIT.
 *   over views    rank UNSEEN 0 < HIDDEN 1 < FREE 2 < HIT 3; a sample's state is the maximum over the views: a view that sees a
 *                 surface at the sample wins over one that sees past it, one that sees past it over one that cannot tell.
 *   row           n[region][state], regions between, finger 0, finger 1, palm.  clear = -1 for a void grasp, with all counts 0;
 *                 clear = 1 when, over the fingers and the palm, hit <= max_hit and hidden + unseen <= max_unknown, and
 *                 n[between][HIT] >= min_between_hit; else 0.  By ONE host function both entry points call.
 *   order         (may be NULL) the indices of the grasps with clear = 1, in input order; *n_clear (may be NULL) their number.
 *   info          (may be NULL) S, the twelve n and N.
 *   states        (may be NULL) host memory, uint8 [n_grasps][N]: every sample's final rank (0 for a void grasp's).  Offered only when
 *                 n_grasps * N <= 2^22; a buffer of min(n_grasps * HAF_MAX_SPACE_SAMPLES, 2^22) bytes holds whatever is offered.
 * The defaults of haf_space_default are NOMINAL figures like the gripper's.  Not modelled: a mask for the robot's own arm, lens
 * distortion, anything between lattice points, grippers other than haf_gripper, the arm behind the palm, a free choice of which view
 * wins (HIT beats FREE by definition).
 *
 * haf_check_space_ref: the host definition of record -- no device, no engine, host views only.
 * haf_check_space: equal to it in every word of every row, of order, n_clear, info and states; every view host or device-resident, a
 * device-resident one read where it lies; host views go up through the raw area of haf_score_frames, each at a multiple of 16 bytes;
 * one memset, ONE launch (k_space_samples: a lane per sample, a workgroup per 256 samples of one grasp), ONE copy back and ONE
 * synchronisation.  Like haf_check_grasps it neither reads nor changes last-batch state or stage timings, works before any request
 * and with HAF_FLAG_PROBABILITY, and shares that call's block and scratch (128 bytes per grasp; n_grasps * N bytes with states).
 * Refusals, all before any device work, nothing written -- everything haf_check_grasps refuses for gripper, grasps, stride and out;
 * per view everything haf_score_frames refuses for a frame's own fields and haf_transfer_labels for a camera of the view's size and
 * intrinsics; HAF_E_ARG: a null views or params, an XYZ view, haf_invert_pose failing, n_views outside 1..HAF_MAX_SPACE_VIEWS,
 * sample_step not finite or outside [0.0005, 1], near_m, tol_abs or tol_rel outside haf_transfer_params' ranges, N above the cap, for
 * the _ref form a device-resident view; HAF_E_CAPACITY: states with n_grasps * N > 2^22, a view of more pixels than max_points, the
 * host views' pixels together above max_points. */
#define HAF_MAX_SPACE_VIEWS 8
#define HAF_MAX_SPACE_SAMPLES 65536
enum { HAF_SPACE_BETWEEN = 0, HAF_SPACE_FINGER0 = 1, HAF_SPACE_FINGER1 = 2, HAF_SPACE_PALM = 3 };
enum { HAF_SPACE_UNSEEN = 0, HAF_SPACE_HIDDEN = 1, HAF_SPACE_FREE = 2, HAF_SPACE_HIT = 3 };
typedef struct haf_space_params {
    float   sample_step;                /* metres between lattice points, finite, in [0.0005, 1]                              */
    float   near_m, tol_abs, tol_rel;   /* as haf_transfer_params': [0.001, 16]; >= 0; [0, 1] per metre of the observed depth */
    int32_t max_hit;                    /* clear: at most this many HIT samples in the fingers and the palm together          */
    int32_t max_unknown;                /* clear: at most this many HIDDEN or UNSEEN samples there                            */
    int32_t min_between_hit;            /* clear: at least this many HIT samples between the fingers                          */
} haf_space_params;
typedef struct haf_grasp_space {
    int32_t clear;                      /* 1 clear, 0 not, -1 a void grasp */
    int32_t n[4][4];                    /* [HAF_SPACE_BETWEEN .. PALM][HAF_SPACE_UNSEEN .. HIT] */
    int32_t reserved[3];
} haf_grasp_space;
typedef struct haf_space_info {
    int32_t step;                       /* S, units of 2^-26 m */
    int32_t n[4][3];                    /* per region: samples along s, t, u */
    int32_t n_samples;                  /* N */
    int32_t reserved[2];
} haf_space_info;
void haf_space_default(haf_space_params *p);   /* 0.004f, 0.05f, 0.004f, 0.002f, 0, 0, 1 */
int  haf_check_space_ref(const haf_frame *views, int32_t n_views, const haf_gripper *gripper, const haf_space_params *params,
                         int32_t n_grasps, const void *grasps, size_t grasp_stride_bytes, haf_grasp_space *out /* [n_grasps] */,
                         int32_t *order /* [n_grasps], may be NULL */, int32_t *n_clear /* may be NULL */,
                         haf_space_info *info /* may be NULL */, uint8_t *states /* [n_grasps][N], may be NULL */);
int  haf_check_space(haf_engine *e, const haf_frame *views, int32_t n_views, const haf_gripper *gripper, const haf_space_params *params,
                     int32_t n_grasps, const void *grasps, size_t grasp_stride_bytes, haf_grasp_space *out /* [n_grasps] */,
                     int32_t *order /* [n_grasps], may be NULL */, int32_t *n_clear /* may be NULL */,
                     haf_space_info *info /* may be NULL */, uint8_t *states /* host, [n_grasps][N], may be NULL */);

int haf_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HAFGRASP_H_ */
