// engine_state.h -- the engine object and what the host-side translation units of libhafgrasp.so share:
//   engine.cpp           create / destroy, calibration of the screening pass at creation, the C-ABI entry points
//   engine_tables.cpp    build_tables: the builder's inputs, the builder, upload_tables (the one upload of the model tables); buffers
//   model_tables.cpp     model, range and feature tables -> the host image of every device table and the constants of every guard band,
//                        as named stages (no device, no environment: model_tables.h)
//   engine_request.cpp   one request: stage launches, decision tiers, host resolution of the residual cases, the batch wrapper
//   engine_geometry.cpp  per-roll transforms, the rotated-rectangle scalars, the final grasp pose (host fp32, glibc)
//   engine_debug.cpp     haf_get_roll_grid / haf_debug_fetch* (intermediate stages for the parity tests)
//   engine_topgrasps.cpp haf_top_grasps: ranked, suppressed grasp candidates of the last scored batch
//   engine_graspmap.cpp  haf_grasp_map / haf_cell_pose / haf_grasp_map_best: the last batch's votes in a sensor frame's pixels
//   engine_objects.cpp   haf_score_objects: every object of a label image as a request of its own, on one shared frame (k_roi_mark_objects, k_map_labels_objects)
//   engine_roi.cpp       haf_score_frames_roi / haf_score_views_roi: the checks, the ROI buffers, the masks' upload, the launch of k_roi_mark / k_roi_mark_view
//   engine_depthfilter.cpp haf_filter_depth: exposures of one depth camera -> one conditioned depth image (k_depth_filter)
//   engine_segment.cpp   haf_segment_frame: one frame -> an image of object labels (segment.hip)
//   engine_cellsegment.cpp haf_segment_cells: one frame of any shape -> object labels by top-down cell clustering (cellsegment.hip)
//   engine_plane.cpp     haf_fit_plane: one frame -> its dominant plane (plane.hip)
//   engine_clearance.cpp haf_check_grasps: one frame, one gripper, n grasp poses -> the points in the gripper's boxes (clearance.hip)
//   engine_opening.cpp  haf_fit_openings: the same inputs -> the smallest free opening and its sideways shift per pose (opening.hip)
//   engine_space.cpp    haf_check_space: 1..8 depth views, one gripper, n grasp poses -> what the views have seen of the gripper's volume (space.hip)
//   engine_labelshape.cpp haf_measure_labels: one frame and its label image -> every label's box in the base frame (labelshape.hip)
//   engine_transfer.cpp  haf_transfer_labels: another camera's label image onto a depth frame's pixels, behind a z-buffer (transfer.hip)
//   engine_testing.cpp   haf_test_* hooks (libhafgrasp_testing.so only)
//   engine_stage.cpp     what the calls that take a haf_frame share: first-use buffers, a host frame's and a side image's upload, the single-frame input, a label image's way out;
//                        and the one block and one scratch of every call outside the request path: call_buffers, call_finish
//   frame_stage.cpp      a haf_frame on its way to the device: descriptor, row packing, upload pieces, batch checks (no device: frame_stage.h, which also holds the checks of label and output images)
// Private to csrc/: not installed, nothing here is part of the ABI (include/hafgrasp.h).  Every engine*.cpp unit above is
// compiled twice, without and with -DHAF_TESTING (test_env below), for the product and the testing library.
#pragma once
#include "../../include/hafgrasp.h"
#include "kernels.h"
#include "parsers.h"
#include "model_tables.h"
#include "frame_stage.h"
#include "decq.h"
#include "engine_internal.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

using namespace haf;

namespace haf_host {

// variable must not be able to scale them in the library a server links.
#ifdef HAF_TESTING
inline const char *test_env(const char *name) { return getenv(name); }
#else
inline const char *test_env(const char *) { return nullptr; }
#endif
// A guard-band scale from the testing build's environment (HAF_GUARD0_REL, HAF_GUARD_REL, HAF_GUARD_I8_REL, HAF_GUARD2_REL).  A value
// below 1e30 scales the band, as the diagnosis tools pass it.  1e30 AND BEYOND IS NOT A SCALE: it means "wide open", every evaluation
// goes on to the next tier, and becomes an infinity.  A finite scale cannot do that: the band of an evaluation whose sum|coef|K is
// exactly 0 (every kernel value underflows) is relative to that 0.  With an infinite scale its band is inf * 0 = NaN, and this
// relies on every tier deciding by the form !(|dec| > band), which a NaN band leaves undecided (screen.hip screen_tail_vals,
// contraction.hip, exact8.hip k_recheck_i8_combine, recheck.hip, features.hip k_small_direct): a tier written as |dec| <= band
// would decide such an evaluation.  The product library never gets here (test_env returns nullptr).
inline double guard_knob(const char *v) { const double g = atof(v); return g >= 1e30 ? (double)INFINITY : g; }

constexpr double kPi = 3.141592653;   // server.cpp:94 -- the reference's truncated constant, NOT M_PI

struct Mat4 {
    float a[4][4];
    static Mat4 identity()
    {
        Mat4 m;
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) m.a[i][j] = (i == j) ? 1.0f : 0.0f;
        return m;
    }
};

struct NormalisedInput {
    double av[3];      // approach vector after server.cpp:270-273
    int sx, sy;        // grasp_search_area_size_{x,y}_dir (266-267)
    int width;         // gripper_opening_width (281)
};

// engine_geometry.cpp
Mat4 operator*(const Mat4 &l, const Mat4 &r);
NormalisedInput normalise(const haf_grasp_input &in);
Mat4 roll_transform(const haf_config &cfg, const haf_grasp_input &in, const NormalisedInput &n, int roll, bool from_float_av,
                    Mat4 *pre_roll = nullptr, float *roll_cs = nullptr);
void fill_roll_geo(const haf_config &cfg, const haf_grasp_input &in, const NormalisedInput &n, int roll, RollGeo &g, float *m0 = nullptr);
bool invert(const Mat4 &m, Mat4 &inv);
// graspmap_host.cpp: rows 0..2 of the transforms of rolls roll_first .. roll_first + roll_count - 1 (fill_roll_geo's), 64 bytes each
void fill_cell_geo(const haf_config &cfg, const haf_grasp_input &in, int roll_first, int roll_count, haf_cell_math::CellGeo *geo);
// graspmap_host.cpp, shared by haf_label_best_ref and haf_grasp_map_labels: the not-found pick; a pick's key (pick_rules.h: its maximum
// is the best pick); the ids id_of(k) of the found ones among picks[0..n), best pick first
void label_pick_none(haf_label_pick *p);
unsigned long long label_pick_key(const haf_label_pick &p, int32_t width);
void label_order(const haf_label_pick *picks, int32_t n, const std::function<int32_t(int32_t)> &id_of, int32_t width, int32_t *order,
                 int32_t *n_found);

// Testing build: every device buffer lies between two guard zones filled with kCanaryByte -- kCanaryGuard bytes in front, and from
// the buffer's last byte to the next multiple of kCanaryGuard plus kCanaryGuard behind -- and is registered with the source line that
// allocated it (engine_testing.cpp: canary_check).  A kernel that writes one element past a list, an operand image or a flag-word
// array changes a guard byte; read as a list entry the pattern is a NEGATIVE evaluation id (0xA5A5A5A5), which no consumer may follow.
// The check is opt-in: with HAF_CANARY_CHECK set the engine checks the zones after every request (the tests that drive the lists into
// their capacities set it; `HAF_CANARY_CHECK=1 pytest -m gpu` runs the whole suite so), haf_test_check_canaries on demand.  The product
// library allocates exactly what is asked for.
#ifdef HAF_TESTING
constexpr size_t kCanaryGuard = 256;
constexpr int kCanaryByte = 0xA5;
void canary_register(void *user, size_t bytes, const char *file, int line);
void canary_unregister(void *user);
int canary_check(std::string *report);          // number of buffers with a damaged guard zone (engine_testing.cpp)
int check_guards(haf_engine *e);                // with HAF_CANARY_CHECK set: HAF_E_INTERNAL and canary_check's report when it finds damage
#else
inline int check_guards(haf_engine *) { return HAF_OK; }
#endif

// A device array that frees itself: the engine's are released by `delete e` (haf_destroy), in no list of names.  A failed alloc() leaves
// it empty (p == nullptr, n == 0), so n tells whether it can be used.  Move-only.  (file, line: the allocating source line, which the
// testing build's guard report names; ensure_dev passes its caller's on, upload_tables the table's name in the file's place)
template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }      // (o frees what this held)
    ~DevBuf() { release(); }
#ifdef HAF_TESTING
    hipError_t alloc(size_t count, const char *file = __builtin_FILE(), int line = __builtin_LINE())
    {
        if (!count) return hipSuccess;
        const size_t bytes = count * sizeof(T), padded = (bytes + kCanaryGuard - 1) / kCanaryGuard * kCanaryGuard;
        char *raw = nullptr;
        hipError_t rc = hipMalloc((void **)&raw, kCanaryGuard + padded + kCanaryGuard);
        if (rc != hipSuccess) return rc;
        rc = hipMemset(raw, kCanaryByte, kCanaryGuard);
        if (rc == hipSuccess) rc = hipMemset(raw + kCanaryGuard + bytes, kCanaryByte, padded - bytes + kCanaryGuard);
        if (rc != hipSuccess) { (void)hipFree(raw); return rc; }
        p = reinterpret_cast<T *>(raw + kCanaryGuard);
        n = count;
        canary_register(p, bytes, file, line);
        return hipSuccess;
    }
    void release()
    {
        if (p) { canary_unregister(p); (void)hipFree(reinterpret_cast<char *>(p) - kCanaryGuard); }
        p = nullptr; n = 0;
    }
#else
    hipError_t alloc(size_t count, const char * = nullptr, int = 0)
    {
        if (!count) return hipSuccess;
        const hipError_t rc = hipMalloc((void **)&p, count * sizeof(T));
        if (rc == hipSuccess) n = count; else p = nullptr;
        return rc;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
#endif
};
static_assert(!std::is_copy_constructible_v<DevBuf<char>> && !std::is_copy_assignable_v<DevBuf<char>>, "a DevBuf has one owner");

// The model on the device: the tables as device arrays and the constants that go with them (model_tables.h)
struct DeviceModel : TableSet<DevBuf>, ModelConsts {};

// A device block and its pinned host twin of the same size, freed with the object.  ensure() gets both halves or neither: when either
// allocation fails the pair it had stays in place and usable (the engine left as it was); growing replaces the pair, not its
// contents, once both exist
struct StageBuf {
    DevBuf<char> dev;                // dev.n: bytes of either half
    char *host = nullptr;
    bool pinned_failed = false;      // the last ensure() failed for want of the pinned half, not of the device half
    StageBuf() = default;
    StageBuf(const StageBuf &) = delete;
    StageBuf &operator=(const StageBuf &) = delete;
    ~StageBuf() { release(); }
    hipError_t ensure(size_t bytes)
    {
        pinned_failed = false;
        if (dev.n >= bytes) return hipSuccess;
        DevBuf<char> d;
        char *h = nullptr;
        hipError_t rc = d.alloc(bytes);
        pinned_failed = rc == hipSuccess && (rc = hipHostMalloc((void **)&h, bytes, hipHostMallocDefault)) != hipSuccess;
        if (rc != hipSuccess) return rc;                 // (d frees the device half it may have got)
        release();
        dev = std::move(d); host = h;
        return hipSuccess;
    }
    void release() { dev.release(); if (host) (void)hipHostFree(host); host = nullptr; }
};
static_assert(!std::is_copy_constructible_v<StageBuf> && !std::is_copy_assignable_v<StageBuf>, "a StageBuf has one owner");

// What the last scored call leaves for the getters (engine.cpp) and the debug reads (engine_debug.cpp, engine_testing.cpp).  A call
// that scores nothing the caller asked for (the calibration requests, a batch whose every budget is negative) resets it: e->last = {}.
struct LastCall {
    int B = 0, R = 0, roll_first = 0;
    int evals = 0;
    int flagged0 = 0;            // what left the screening passes
    int flagged = 0;             // what entered the exact tiers (the exact-integer tier's input list when i8)
    int flaggedi = 0;            // evaluations that entered the fp64 MFMA tier
    int bypass = 0;              // ... of them through the short-list gate (engine_request.cpp), around tier 1 and the exact-integer tier
    int flagged2 = 0;            // the strict tier's list
    int host_resolved = 0;       // strict-tier decisions made on the host with the C library's exp
    int inexact = 0;             // (cloud, roll) grids whose integral image needed the sequential order
    bool screened = false;       // the labels came through the screening tier (not its three-pass fallback)
    bool lr = false;             // the screening pass ran in the low-rank form
    bool i8 = false;             // tier 2a ran (then d_dec_exact holds ITS values and d_dec_exacti the fp64 tier's)
    std::vector<haf_grasp_input> inputs;
    // where the kernels read every cloud of the batch (haf_debug_fetch_points): its first float inside the points area of in_block and its
    // point count; staged = false for a device-resident xyz cloud, which lies in the caller's memory
    struct CloudSrc { size_t float_off = 0; size_t n = 0; bool staged = false; };
    std::vector<CloudSrc> clouds;
    bool roi = false;            // the batch was an ROI request: d_roi_cells holds its B x R cell sets (HAF_DBG_ROI)
};

// which forms of the pre-stages the launchers chose for the last request that reached them (kernels.h: BinForm, IntegralForm); read by
// the testing build's haf_test_prestage_forms only
struct PrestageForms { int bin = -1, integral = -1; bool bucket_refused = false; };

// haf_score_frames_roi / haf_score_views_roi: what the request path (engine_request.cpp) needs of the call, filled by engine_roi.cpp.
// Per VIEW, by the flat view index (haf_score_frames_roi: one view per request); a view of haf_score_views_roi may have no mask
struct RoiCall {
    const haf_roi *rois = nullptr;       // rois[k] goes with frame k
    std::vector<long> masked;            // per REQUEST: the non-zero bytes of its host masks, -1 when any of its masks is device-resident
    std::vector<size_t> off;             // per view: where a host mask lies in roi_mask (packed rows, 16-byte aligned)
    // a view's mask goes through the staging area (roi_mask): it has one and it lies in host memory
    static bool staged(const haf_roi &r) { return r.mask != nullptr && r.on_device != 1; }
};

// haf_score_objects: the requests of the batch share ONE frame (frames[0]; one upload, one k_frame_points, one set of points that every
// CloudDev points at, counted once against max_points) and their masks are the instances of one label image: request b's is
// `labels == the label of object b`.  Filled by engine_objects.cpp, which has uploaded the image and the table before the request path
// starts; the request path (engine_request.cpp) reads it where an ROI call's masks would be uploaded and marked
struct ObjectsCall {
    const void *d_labels = nullptr;      // the label image on the device: the caller's, or the staged copy
    size_t label_stride = 0;             // bytes between its rows
    int label_bytes = 1, n_labels = 0;
    const int *d_req_of_label = nullptr; // [n_labels] on the device: label l -> its request, -1 for none
};

// Where a request's points come from when not from the caller's clouds (the request path takes a pointer, null for clouds)
struct FrameSource {
    const haf_frame *frames = nullptr;   // cloud b's points are frame b's, deprojected on the device; clouds[b] only carries its point count
    const int32_t *views = nullptr;      // ... are the valid points of views[b] consecutive frames; clouds[b].n_points is their pixel count
    const RoiCall *roi = nullptr;        // haf_score_frames_roi, haf_score_views_roi (with views): only the cells near the masked pixels' cells are evaluated
    const ObjectsCall *objects = nullptr;// haf_score_objects (with roi, whose rois is null and whose masked[] counts each object's pixels): frames[0] serves every request
};

}  // namespace haf_host

using namespace haf_host;

struct haf_engine {
    haf_config cfg{};
    std::string feature_file, range_file, model_file;
    std::vector<FeatureRow> features;
    RangeTable range;
    SvmModel model;
    // the model as haf_create made it: every device table (model_tables.h: TableSet, for_each_table), every parameter struct, every scalar
    // and flag of the table work.  upload_tables fills it; nothing writes to it afterwards
    DeviceModel mdl;
    std::string error;

    // stream: the CURRENT stream, on which every operation of every call is enqueued (haf_set_stream; null is HIP's default stream).
    // own_stream: the one the engine created, alive from haf_create to haf_destroy whichever stream is current
    hipStream_t stream = nullptr, own_stream = nullptr;
    bool has_own_stream = false;    // creation got as far as a device and its stream (haf_destroy of a half-built engine touches no device)
    hipEvent_t ev[HAF_ST_COUNT + 1] = {};
    float stage_ms[HAF_ST_COUNT] = {};

    long max_evals = 0, max_evals_pad = 0;
    int max_rolls = 0;      // rolls per haf_score_rolls call the buffers are sized for (cfg.max_rolls_per_call, default n_rolls)
    // Tier lists hold one entry per evaluation of the largest request (list_cap), so no request can overflow them.  flag_cap
    // is the WINDOW of the fp64 MFMA tier: what its operand image (2.6 KB per evaluation) is sized for.  A request that flags
    // more walks the list window by window (decide(), below): slower, never an error.
    int list_cap = 0;
    int flag_cap = 0;
    int flag0_cap = 0;      // screening pass: evaluations that go on to the three-pass kernel
    bool generic_kernel = false; // the model's kernel is not RBF: every evaluation through the libsvm-order tier (engine.cpp, engine_request.cpp)
    bool screen_active = true;   // starts as mdl.screen_active.  Default mode only: cleared once more than 60 % of a call's evaluations fell inside the band of every
                                 // form of the screening pass -- for such a model the single pass is wasted work.  Not for good: every
                                 // reprobe_every-th full-size request afterwards tries the pass again (the judgement may have come from
                                 // the synthetic calibration scene or from one unusual cloud) and switches it back on when it pays
    int inactive_calls = 0;      // full-size requests served without the screening pass since it was switched off / last re-tried
    int reprobe_every = 64;      // (testing build: HAF_REPROBE_EVERY)
    // which form of the screening pass serves this model (kernels.h: SCREEN_*): chosen at creation (calibrate()) and re-chosen
    // by the adaptive rule when a call leaves too much undecided.  PLAIN: |w|_2 through its bound; SUMSQ: |w|_2 measured
    // (ill-conditioned models: large coefficients whose kernel values are small); CR_EXP / CR_POLY: the centred-remainder
    // form (round 4: trained models with a large C, whose decisions are 1e-5..1e-8 of sum|coef|K)
    int screen_variant = SCREEN_PLAIN;
    bool variant_forced = false; // testing build: HAF_SCREEN_VARIANT pins the variant (no adaptive rule)
    bool variant_settled = false;   // every form has been seen (at calibration or on requests) and the engine has chosen: no more switching
    // "tier 0b": behind the PLAIN / SUMSQ form, the centred-remainder form (SCREEN_CR_EXP) runs once more on the first pass's LIST --
    // a few per cent of the evaluations at the price of a per cent of the first pass -- when calibration saw it decide much more.
    // t1_skip: what the screening passes leave goes straight to the exact tiers (tier 1's band has a worst-case floor since round 4 --
    // 76 u of sum|x s| -- and decides little of what a centred-remainder pass could not: measured at calibration)
    bool use_t0b = false, t1_skip = false;
    DevBuf<int> d_flag0b_list;
    // partial class sums of the screening kernel's PART form (requests that do not fill the chip are split over SV ranges: screen.hip)
    DevBuf<char> d_screen_part;
    int screen_parts = 0;        // 0: by the live evaluation count; testing build (HAF_SCREEN_PARTS): 1 = never, n = forced
    double variant_share[SCREEN_VARIANTS] = {-1.0, -1.0, -1.0, -1.0};   // undecided share of each variant on the calibration scene (-1: not tried)
    DevBuf<double> d_t1_L;       // tier 1 in the centred-remainder form (mdl.svt_h_cr, mdl.t1_tab): L per list slot
    size_t cells_cap = 0;   // B*R*H*W

    // ONE input block per request: [CloudDev x B][RollGeo x B*R][host clouds' points], packed at call time so that a single
    // host-to-device copy carries everything (a small request is bound by the number of stream operations); the
    // pinned half has the same layout
    StageBuf in_block;
    size_t in_hdr_cap = 0;          // bytes reserved for the header arrays (CloudDev, RollGeo, FrameDev, RoiViewDev)
    // haf_score_frames: the raw pixels of host depth frames, 2 or 4 bytes each, go through their own pinned block and device area
    // (raw: 4 bytes x max_points, every frame at a multiple of 16 bytes); k_frame_points writes their points into the points area of in_block.
    // Never converted inside the points area itself: a point's 12-byte slot overlaps raw pixels other lanes have not read yet
    StageBuf raw;
    // haf_score_views: the raw area of staged host XYZ views, 12 bytes x max_points, allocated by the first call that has one.  Such a
    // view cannot be converted in place as haf_score_frames does: compaction writes where other lanes have not read yet
    StageBuf raw_xyz;
    // ONE output block: [counters][roll records], fetched with a single device-to-host copy (d_counters / d_rec, h_counters / h_rec point into it)
    StageBuf out_block;
    bool counters_clean = false;    // the counters were zeroed behind the previous request's copy-out (off the next request's critical path)
    DevBuf<float> d_sorted;         // bucket-sorted copy of the clouds (binning of large grids, prestages.hip)
    DevBuf<int> d_bkt;              // 3 x max_clouds x kBktInts bucket counters / offsets / cursors
    int bkt_ints = 0;
    DevBuf<int> d_heights;          // ordered keys during binning, fp32 heights afterwards
    DevBuf<double> d_rowsum;        // integral image: band totals of the parallel form / row sums of the sequential fallback
    DevBuf<int> d_inexact;          // per (cloud, roll): the parallel integral image was not exact -> sequential order (prestages.hip)
    DevBuf<float> d_ii;
    DevBuf<uint8_t> d_mask;
    DevBuf<int> d_rowcount, d_rowoff, d_brcount, d_evalcell, d_flag_list, d_flag2_list;
    DevBuf<unsigned char> d_t1_flags;          // tier 1: one "undecided" byte per entry (list slot, or evaluation in the all-evaluations modes)
    DevBuf<unsigned long long> d_tier_words;   // exact tiers: one "undecided" bit per entry of a window, for the ordered hand-over lists
    DevBuf<unsigned long long> d_brslot;   // k_small_pre: per (cloud, roll) {request epoch, evaluations} in one word (ordered evaluation list)
    unsigned pre_epoch = 0;
    PrestageForms pre_forms;        // run_prestages (engine_request.cpp)
    int feature_form = FEAT_NONE;   // the FeatureForm that served the last screening feature pass (launch_screening; FEAT_NONE: none ran yet)
    // ... and, while the testing build's snapshot is on (snap_on), the ScreenParams set it read (SP_PLAIN / SP_CR / SP_LRP) as it was handed
    // over.  Members of every build: graspmap_host.cpp and roi_host.cpp are compiled once for both libraries, so the layout must not differ
    int feature_sp_kind = -1;
    ScreenParams feature_sp{};
    struct View { int *p = nullptr; } d_counters;      // inside out_block
    DevBuf<float> d_X, d_ax, d_dec;
    // low-rank form of the centred-remainder pass (mdl.lr_available; kernels.h: kLrK; large requests only)
    bool lr_enabled = true;          // testing build: HAF_NO_LR switches it off; HAF_LR_ALWAYS lifts the request-size rule
    bool lr_always = false;
    DevBuf<unsigned long long> d_iiabs;   // per (cloud, roll): sum of |height| in units of 2^-20 m (k_integral_totals)
    DevBuf<float> d_X1, d_ax1, d_gband;   // three-pass operand images / a_x of the screened-out rest; per-evaluation guard band
    DevBuf<int> d_flag0_list;
    DevBuf<unsigned long long> d_flag0_words;   // one bit per evaluation: undecided by the screening pass
    DevBuf<int> d_flag0_wgcount;                // popcounts per 256 words, for the ordered compaction
    DevBuf<int8_t> d_labels;
    DevBuf<double> d_dec_exact, d_dec_exact2, d_x64, d_part64;
    DevBuf<double> d_strict_terms;   // strict tier, spread form: kStrictSlots x n_sv_pad products coef K (launch_recheck_known)
    // tier 2a, the exact-integer tier (exact8.hip; mdl.i8_active): its hand-over list to the fp64 MFMA tier and that tier's decision
    // values for it (d_dec_exact then holds tier 2a's values, in the order of d_flag_list)
    DevBuf<int> d_flagi_list;
    DevBuf<double> d_dec_exacti;
    bool short_gate = true;         // testing build: HAF_NO_SHORT_GATE switches the gate off
    DevBuf<short> d_ev16;
    DevBuf<float> d_margin;         // HAF_FLAG_KEEP_DEBUG, default mode: |dec^| / band of every evaluation the screening tier decided
    DevBuf<AttrRecord> d_attr;      // HAF_FLAG_KEEP_DEBUG: [max_evals][kKP] attribute records of the exact-form feature kernels
    struct RecView { RollRecordDev *p = nullptr; } d_rec;   // inside out_block, behind the counters
    DevBuf<unsigned long long> d_topkey;
    DevBuf<int> d_rowmax;           // best vote per grid row (k_vote_cells -> k_vote_pick)
    // probability-output mode (HAF_FLAG_PROBABILITY, prob.hip): per-cell value of the cell's own output line, the grid
    // show_predicted_gps builds from them, the fp32 votes, and the two "%g" probabilities per evaluation
    DevBuf<float> d_own, d_gridf, d_evf;
    DevBuf<double> d_ptext;
    DevBuf<double> d_part1;
    long part1_stride = 0;
    // requests with at least this many evaluation slots take the thread-per-evaluation feature kernel: its floor is one thread's
    // chain of 324 attributes (~0.2 ms), the cooperative kernel costs ~1.3 us per 1000 evaluations (crossover measured at ~3e5)
    long large_evals = kLargeEvals;

    // views into the pinned half of out_block
    RollRecordDev *h_rec = nullptr;
    int *h_counters = nullptr;
    // requests whose whole SVM work (evaluations x support vectors) is at most this go straight to tier 2's arithmetic in one
    // launch (k_small_direct): cheaper than a feature kernel, a fast contraction and the rechecks behind it (C2: 3 760 x 172 in
    // 36 us against 21 + 30 + 30 us; measured the other way round at C3's 31 093 x 172: 203 us against 186)
    long direct_work = 1L << 21;
    bool calibrated = false;        // the screening variant was chosen at creation (calibrate())
    double mfma_kappa = 12.0;       // error of one v_mfma_f32_16x16x32_f16 in units of 2^-24 (|c| + sum|a b|): max(12, 1.5 x probe_mfma_rounding())
    double mfma_kappa16 = 12.0;     // the same for v_mfma_f32_16x16x16f16 (the K tail of the three-pass kernel)
    double mfma_kappa_measured = 0.0, mfma_kappa16_measured = 0.0;
    bool no_bucket_sort = false;    // set (for good) when a tile of the bucket-sorted binning path overflowed its candidate list
    bool no_fused_pre = false;      // testing build: HAF_NO_FUSED_PRE keeps the separate pre-stage kernels on small grids too

    std::vector<std::pair<const char *, size_t>> host_regs;   // haf_register_host_cloud: page-locked caller buffers

    // how often a request met a list smaller than what it had to hold (the overflow campaigns read them: haf_test_overflow_stats)
    long stat_flag0_overflows = 0;  // the screening passes left more undecided than their list holds: decision stage redone
    long stat_extra_windows = 0;    // windows of the exact tiers' lists beyond the first
    LastCall last;
    // testing library (engine_testing.cpp: haf_test_snapshot_screen): copies of what the screening feature pass of a request left --
    // the operand images, the raw band sums and a_x -- taken right behind its launch, before the sweep and the later tiers reuse the buffers
    bool snap_on = false;
    long snap_cap = 0;              // evaluation slots the last snapshot covers
    DevBuf<char> snap_X;
    DevBuf<float> snap_gband, snap_ax;
    // ... and of what every SWEEP launch of a request left (launch_screening: [0] the first pass, [1] tier 0b), taken right behind the
    // launch, before a later tier writes dec, margin, the flag words or the lists again; `form` is what the launcher said it launched
    // (kept whether or not the snapshot is on).  in_*: tier 0b's list-indexed operand images, bands and a_x (its feature kernel's output)
    struct SweepSnap {
        SweepForm form{};
        long cap = 0;               // evaluation slots the launch covered (its max_evals); 0: the launch did not run in the last request
        long dec_cap = 0;           // entries of dec and margin that were copied (they go by evaluation id: the request's slots)
        long list_cap = 0;          // entries of the output list that were copied
        long part_bytes = 0;        // bytes of part_buf that were copied (PART form only)
        DevBuf<float> dec, margin;
        DevBuf<unsigned long long> words;
        DevBuf<int> list, counters;
        DevBuf<char> part, in_X;
        DevBuf<float> in_gband, in_ax;
        DevBuf<int8_t> labels;      // the label grids right behind the launch (every cell of the engine's grids)
        DevBuf<float> raw;          // low-rank form: the raw sums as the sweep read them (behind k_project in the two-launch form)
        DevBuf<char> Y;             // low-rank form, two launches: the projected 6-step operand images k_project wrote
        long raw_cap = 0, y_bytes = 0;
    } snap_sweep[2];
    // The calls that run outside the request path -- haf_segment_frame, haf_segment_cells, haf_fit_plane, haf_check_grasps,
    // haf_fit_openings, haf_check_space, haf_measure_labels, haf_transfer_labels, the haf_grasp_map family with haf_cell_pose, haf_score_objects and haf_top_grasps -- share
    // ONE block with its pinned twin and ONE device-only scratch (call_buffers, engine_stage.cpp): allocated by the first call that needs
    // them, grown to the largest need seen, laid out by the call that is running, and nobody's once it has returned.  A call writes every
    // region before it reads it (DESIGN.md 4 has the table): what it finds there is any other call's leftovers
    StageBuf call_io;
    DevBuf<char> call_scratch;
    // haf_score_frames_roi (engine_roi.cpp), allocated on its first call: the ROI cell sets -- one bit per cell, max_clouds x max_rolls
    // grids of H x roi_row_words(W) 64-bit words (roi.hip) -- and the area of uploaded host masks (max_points bytes and 16 bytes of slack
    // per view, every mask at a multiple of 16 bytes) with its pinned twin.  haf_score_views_roi shares both
    DevBuf<unsigned long long> d_roi_cells;
    StageBuf roi_mask;
    // haf_filter_depth (engine_depthfilter.cpp) with out == NULL: the engine's own output image, 4 bytes x max_points, allocated by the
    // first call that asks for it.  Everything else of that call -- staged host exposures, the counters, a host output image -- passes
    // through the raw area above
    DevBuf<char> d_filter_image;
    // haf_segment_frame, haf_segment_cells and haf_transfer_labels with labels == NULL: the engine's own label image (2 bytes x max_points),
    // allocated by the first call that asks for it.  Unlike the call's block it outlives its call: the caller reads it afterwards
    DevBuf<char> d_seg_image;
};

namespace haf_host {

#define HIPCHK(e, call)                                                                                   \
    do {                                                                                                  \
        hipError_t err__ = (call);                                                                        \
        if (err__ != hipSuccess) {                                                                        \
            (e)->error = std::string(#call) + ": " + hipGetErrorString(err__);                            \
            return HAF_E_DEVICE;                                                                          \
        }                                                                                                 \
    } while (0)

// Cost model of the screening pass's forms, in units of the plain kernel's time per evaluation (measured at C5, nSV 4096: plain 14.1 ms,
// SUMSQ 15.8, CR_EXP 15.5, CR_POLY 16.3); an undecided evaluation costs ~8.5 screened ones in the three-pass tier and the exact tiers
// behind it (seed 11 of the bench generator: 5.8 ms for 378 k evaluations against 14.1 ms for 7.9 M)
constexpr double kVariantCost[SCREEN_VARIANTS] = {1.0, 1.12, 1.10, 1.16};
constexpr double kUndecidedCost = 8.5;
// with the low-rank form (kernels.h: kLrK) serving the engine's full-size requests, in units of the TEN-step plain kernel (13.8 ms at C5,
// 4096 SVs; the feature kernel's 0.8 ms of noise bounds included): plain epilogue 10.3 + 0.8, CR_EXP 11.6 + 0.8, CR_POLY 24.3 + 0.8
// against 28.9 ms (plain equivalent at 8964 SVs); SUMSQ has no low-rank form
constexpr double kVariantCostLr[SCREEN_VARIANTS] = {0.80, 1.12, 0.90, 0.87};

constexpr int kShortListGate = 256;  // the short-list gate (engine_request.cpp): lists of at most this many entries in front of tier 1 ...
constexpr int kShortGateMinSv = 2048; // ... of a model with at least this many support vectors go straight to the fp64 MFMA tier
constexpr int kStrictSlots = 64;     // evaluations per pass of the strict tier's spread form (a few per request reach it at most)

constexpr size_t kCntBytes = up16(CNT_COUNT * sizeof(int));                 // the counters' share of the output block (out_block)

// does the low-rank form serve this engine's full-size requests?  (engine_request.cpp applies it per request: whole requests of at
// least large_evals evaluations on grids that go through the parallel integral image)
inline bool lr_typical(const haf_engine *e)
{
    const haf_config &c = e->cfg;
    return e->mdl.lr_available && e->lr_enabled && (long)c.grid_h * c.grid_w > 8192 &&
           (long)(c.grid_h - 14) * (c.grid_w - 14) * e->max_rolls >= e->large_evals;
}
inline double variant_cost(const haf_engine *e, int v)
{
    if (!lr_typical(e) || (v == SCREEN_PLAIN && !e->mdl.lr_plain_available)) return kVariantCost[v];
    return kVariantCostLr[v];
}
// (contraction_mode and its MODE_* values: model_tables.h)

// ---- the routing of one decision stage (engine_request.cpp: plan_tiers) ----
// The tier lists by name; each list's length lives in its own counter (list_counter), CNT_T1_N being the one re-count (what tier 1
// reads as its list's length behind the short-list gate).  engine_request.cpp: list_buf maps a name to the engine's buffer.
enum ListId { L_NONE = -1, L_FLAG0 = 0, L_FLAG0B, L_FLAG, L_FLAGI, L_FLAG2 };
inline int list_counter(int l)
{
    static const int cnt[] = {CNT_FLAGGED0, CNT_FLAGGED0B, CNT_FLAGGED, CNT_FLAGGEDI, CNT_FLAGGED2};
    return l == L_NONE ? -1 : cnt[l];
}
// what the routing depends on: the engine's state and the request's classification (tier_facts and haf_test_tier_plan fill it in
// declaration order)
struct TierFacts {
    int screen_variant = SCREEN_PLAIN;
    bool cr_available = false, lr_available = false, lr_enabled = false, lr_plain_available = false, lr_fused = false;
    bool use_t0b = false, t1_skip = false, t1_cr_available = false, i8_active = false, calibrated = false, short_gate = false;
    bool generic_kernel = false;
    int n_sv = 0;
    bool t0b_no_gather = false;      // testing build: HAF_T0B_NO_GATHER
    int mode = MODE_SCREEN;
    bool reuse_operands = false, direct = false, small_exact = false, large = false, fused_pre = false;
    long hw = 0, evals_cap = 0;
};
enum { PATH_GENERIC, PATH_DIRECT, PATH_SCREEN, PATH_SPLIT, PATH_F32 };
enum { SP_PLAIN, SP_CR, SP_LRP };               // ScreenParams set of the screening pass: screen / screen_cr / screen_lrp
enum { T0B_NONE, T0B_GATHER, T0B_FEATURES };    // tier 0b: not run / the low-rank sweep's gather form / feature kernel + sweep
enum { FP64_NONE, FP64_SMALL, FP64_MFMA };      // window 0 of the fp64 tier: none / k_small_direct in list mode / k_recheck_mfma
// Which tiers run in which form, and for every producer the list it writes, for every consumer the list (and counter) it reads.
// The stages run in this order: first pass, tier 0b, gate, tier 1, exact-integer tier, fp64 MFMA tier, strict tier.
struct TierPlan {
    int path = PATH_SCREEN;
    int sp = SP_PLAIN;
    bool cr = false, lr = false;     // the screening pass: centred-remainder form, low-rank form
    bool reuse = false;              // ... on the previous pass's operand images (no feature kernel)
    int pass0_out = L_NONE;          // the first pass: the screening pass, the contraction over every evaluation, the generic / direct tier
    int t0b = T0B_NONE, t0b_in = L_NONE, t0b_out = L_NONE;
    bool gate = false;
    int gate_in = L_NONE, gate_out = L_NONE;
    bool t1 = false, t1cr = false;
    int t1_in = L_NONE, t1_cnt = -1, t1_out = L_NONE;
    bool i8 = false;
    int i8_in = L_NONE, i8_out = L_NONE;
    int fp64 = FP64_NONE, fp64_in = L_NONE, fp64_out = L_NONE;
    int strict_in = L_FLAG2;
};
TierPlan plan_tiers(const TierFacts &f);

inline int fail(haf_engine *e, int code, const std::string &msg)
{
    e->error = msg;
    return code;
}

// ---- no C++ exception may cross the C-ABI: a corrupt input file or an exhausted host must come back as a status the ROS
// shim can turn into setAborted(), not as std::terminate() of the action server ----
template <class F> int guarded(std::string *err, F &&f)
{
    try {
        return f();
    } catch (const std::bad_alloc &) {
        if (err) *err = "out of host memory";
    } catch (const std::exception &ex) {
        if (err) *err = std::string("internal error: ") + ex.what();
    } catch (...) {
        if (err) *err = "internal error (unknown exception)";
    }
    return HAF_E_INTERNAL;
}

inline void mark(haf_engine *e, int idx)
{
    if (e->cfg.flags & HAF_FLAG_PROFILE) (void)hipEventRecord(e->ev[idx], e->stream);
}

// engine_tables.cpp (label_grid_value, header_grid_value, sigma_upper_bound: model_tables.h)
TableSwitches table_switches();       // the testing build's environment switches of the table work
int build_tables(haf_engine *e);
int upload_tables(haf_engine *e, const ModelTables &t);
int alloc_buffers(haf_engine *e);
// engine_request.cpp
int score_rolls_impl(haf_engine *e, int32_t n_clouds, const haf_cloud *clouds, const haf_grasp_input *in, int32_t roll_first,
                     int32_t roll_count, haf_roll_record *records, const FrameSource *from = nullptr);
int score_batch_impl(haf_engine *e, int32_t n_clouds, const haf_cloud *clouds, const haf_grasp_input *in, haf_grasp_output *out,
                     const FrameSource *from = nullptr);
int score_frames_impl(haf_engine *e, int32_t n, const haf_frame *frames, const haf_grasp_input *in, haf_grasp_output *out);
// (clouds[b].n_points is the UPPER bound there, the pixels of the request's views)
int score_views_impl(haf_engine *e, int32_t n, const int32_t *views_per_request, const haf_frame *frames, const haf_grasp_input *in,
                     haf_grasp_output *out, int64_t *n_points);
// engine_stage.cpp: the first-use buffers and the staging of the calls that take a haf_frame; the policies are described there.
// `who`: the message's prefix, "haf_<call>: "; `what`: the site's words for the buffer ("no device memory for <what>: ...")
// at least `count` elements in b (a larger need replaces it: the contents are nobody's)
template <class T> int ensure_dev(haf_engine *e, DevBuf<T> &b, size_t count, const std::string &who, const char *what, const char *file = __builtin_FILE(), int line = __builtin_LINE())
{
    if (b.n >= count) return HAF_OK;
    b.release();
    const hipError_t rc = b.alloc(count, file, line);
    return rc == hipSuccess ? HAF_OK : fail(e, HAF_E_DEVICE, who + "no device memory for " + what + ": " + hipGetErrorString(rc));
}
// at least `bytes` in both halves of b (StageBuf::ensure: the old pair stays usable when growing fails)
int ensure_stage(haf_engine *e, StageBuf &b, size_t bytes, const std::string &who, const char *what);
int ensure_raw_xyz(haf_engine *e, const std::string &who);      // the raw area of staged host XYZ views, on the first call that has one
// a host frame's packed rows to host_at (pinned) and from there to dev_at, in pieces; no synchronisation
int upload_frame(haf_engine *e, const haf_frame &f, char *host_at, char *dev_at, hipStream_t s);
// ONE checked frame as a call's input.  prepare: its refusals and the raw area it goes through (*area), no stream operation.
// upload: a host frame goes up; *fd = the frame as the kernels read it
int frame_input_prepare(haf_engine *e, const haf_frame &f, const std::string &who, StageBuf **area);
int frame_input_upload(haf_engine *e, const haf_frame &f, StageBuf &area, hipStream_t s, FrameDev *fd);
// The way in and the way out of a call that runs outside the request path.  call_buffers, before the call's first stream operation:
// hipSetDevice, then at least scratch_bytes of the shared scratch (0, nullptr: the call has none) and io_bytes of the shared block
// (haf_engine::call_io); *out = the engine's stream and where the three lie.  Their contents are whatever the last such call left.
// NOTHING ON THE REQUEST PATH MAY CALL IT (engine_request.cpp, engine_roi.cpp, the calibration of engine.cpp): haf_score_objects keeps
// its label table and its staged label image in the block while its batch is scored (objects_mark_cells reads them there), and a
// call_buffers in between could replace the block under it.
// call_finish, behind the call's last launch: hipGetLastError, ONE copy of back_bytes at back_at from the block's device half to the
// same place of its pinned half (none when 0), ONE synchronisation, then the testing build's guard check
struct CallBuffers {
    hipStream_t stream = nullptr;
    char *dev = nullptr, *host = nullptr, *scratch = nullptr;
};
int call_buffers(haf_engine *e, const std::string &who, size_t io_bytes, const char *what_io, size_t scratch_bytes, const char *what_scratch,
                 CallBuffers *out);
int call_finish(haf_engine *e, const CallBuffers &cb, size_t back_bytes, size_t back_at = 0);
// a side image of frame f (f.height x f.width elements): a host one through the call's block at `at`, one copy; *id = where the kernels read it
int upload_image(haf_engine *e, const haf_frame &f, const void *data, int on_device, size_t row_stride_bytes, size_t elem_bytes, const CallBuffers &cb, size_t at, ImageDev *id);
// the label image a call writes for frame f.  prepare, before the call's first stream operation: the engine's own image on its first use
// when `labels` is null; *o = where the kernels write, a host image packed at packed_at inside the block the call copies back.  finish, after
// the call's ONE copy back and ONE synchronisation: a host image's rows from host_packed_at, packed_at's pinned twin, to the caller's; *out_image (may be null) filled
int label_output_prepare(haf_engine *e, const haf_frame &f, void *labels, int32_t elem_bytes, size_t row_stride_bytes, int32_t out_on_device, void *packed_at, const std::string &who, OutputDev *o);
void label_output_finish(const OutputDev &o, const haf_frame &f, int32_t elem_bytes, const char *host_packed_at, haf_label_image *out_image);
// engine_roi.cpp
int score_frames_roi_impl(haf_engine *e, int32_t n, const haf_frame *frames, const haf_roi *rois, const haf_grasp_input *in, haf_grasp_output *out);
int score_views_roi_impl(haf_engine *e, int32_t n, const int32_t *views_per_request, const haf_frame *frames, const haf_roi *rois,
                         const haf_grasp_input *in, haf_grasp_output *out, int64_t *n_points);
// the staged host masks of the call's n_views views to the device (no synchronisation)
int roi_upload_masks(haf_engine *e, const RoiCall &roi, const haf_frame *frames, int n_views, hipStream_t s);
// haf_score_views_roi: the descriptors of the call's views (views[b] per request) for k_roi_mark_view, into the request's header block
void roi_describe_views(const haf_engine *e, const RoiCall &roi, const haf_frame *frames, const int32_t *views, int B, int R, int H, int W,
                        const RollGeo *d_geo, RoiViewDev *out);
// What roi_mark_cells needs of a request with views: its FrameDev and RoiViewDev arrays, device and pinned (null: haf_score_frames_roi)
struct RoiViews {
    const FrameDev *d_frames = nullptr, *h_frames = nullptr;
    const RoiViewDev *d_roi = nullptr, *h_roi = nullptr;
    int n_views = 0;
};
// clears the B * R ROI cell sets and marks them: k_roi_mark per request, on the points k_frame_points left at h_clouds[b].xyz; with
// views, k_roi_mark_view over every view of the batch, on the raw pixels k_view_points read
int roi_mark_cells(haf_engine *e, const RoiCall &roi, const haf_frame *frames, const CloudDev *h_clouds, const RollGeo *d_geo, const Dims &d,
                   float r_row, float r_col, hipStream_t s, const RoiViews *views = nullptr);
// engine_objects.cpp: haf_score_objects.  objects_mark_cells: roi_mark_cells for an objects call -- clears the B * R cell sets and marks
// them all with ONE launch of k_roi_mark_objects on the points k_frame_points left at h_clouds[0].xyz
int score_objects_impl(haf_engine *e, const haf_frame *frame, const haf_label_image *labels, int32_t n_labels, int32_t n_objects,
                       const int32_t *object_labels, const haf_grasp_input *in, int32_t min_vote, haf_grasp_output *out, haf_label_pick *picks,
                       haf_grasp_candidate *poses, int32_t *order, int32_t *n_found);
int objects_mark_cells(haf_engine *e, const ObjectsCall &oc, const haf_frame &frame, const CloudDev *h_clouds, const RollGeo *d_geo, const Dims &d,
                       float r_row, float r_col, hipStream_t s);
// engine_roi.cpp: the ROI cell sets and the masks' area, on the first call that needs them
int ensure_roi_buffers(haf_engine *e, const std::string &who);
// engine_graspmap.cpp: the host tail of a label pass (haf_grasp_map_labels, haf_score_objects).  got[k], k < n: what the record kernel
// left for entry k, which belongs to request request_of(k) of the last batch and is listed in `order` as id_of(k).  EVERY entry is
// checked before the first one is handed over (HAF_E_INTERNAL, `who` in front of the text); then picks[k], poses[k] (null: not wanted;
// the cell's record as a candidate, haf_cell_pose's pose of it) and the found ids, best pick first (label_order)
int hand_over_picks(haf_engine *e, const std::string &who, const LabelOutDev *got, int32_t n, const std::function<int(int32_t)> &request_of,
                    const std::function<int32_t(int32_t)> &id_of, int32_t width, haf_label_pick *picks, haf_grasp_candidate *poses,
                    int32_t *order, int32_t *n_found);
// engine_geometry.cpp
int finalize_impl(const haf_config &c, const haf_grasp_input *in, const haf_roll_record *rec, haf_grasp_output *out, std::string &error);
int roll_pose_impl(const haf_config &c, const haf_grasp_input *in, const haf_roll_record *rec, int roll, haf_grasp_output *out,
                   int32_t *published, std::string &error);
int candidate_pose_impl(const haf_config &c, const haf_grasp_input *in, const haf_roll_record &r, int roll, haf_grasp_output *out,
                        std::string &error);
// engine_topgrasps.cpp: steps 4-6 of haf_top_grasps over one cloud's per-roll greedy sequences (lists in ascending roll order)
struct TopList {
    int roll = 0;                     // global roll index
    int n = 0;                        // entries of the sequence present
    bool more = false;                // the sequence may go on beyond them
    const haf_roll_record *rec = nullptr;   // n records {vote, row, col, h_locmax, n_evals of the roll}
    const int32_t *len = nullptr;     // n run lengths
};
int top_merge(const haf_config &c, const haf_grasp_input *in, const std::vector<TopList> &lists, int k, int roll_window, double min_dist_m,
              haf_grasp_candidate *out, int32_t *n_found, bool *need_more, std::string &error);

}  // namespace haf_host
