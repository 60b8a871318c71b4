// engine_testing.cpp -- the haf_test_* hooks of libhafgrasp_testing.so (tests/ only; the product library does not contain this file).
#include "engine_state.h"
#include "screen_finish.h"
#include "screen_band.h"

#ifndef HAF_TESTING
#error "engine_testing.cpp belongs to the testing build (-DHAF_TESTING)"
#endif

// ---- guard zones around every device buffer (engine_state.h: DevBuf) ----
namespace haf_host {
namespace {
struct CanaryRec { char *user; size_t bytes; const char *file; int line; };
std::mutex g_canary_mu;
std::vector<CanaryRec> g_canary;
}
void canary_register(void *user, size_t bytes, const char *file, int line)
{
    std::lock_guard<std::mutex> lk(g_canary_mu);
    g_canary.push_back(CanaryRec{static_cast<char *>(user), bytes, file, line});
}
void canary_unregister(void *user)
{
    std::lock_guard<std::mutex> lk(g_canary_mu);
    for (size_t i = 0; i < g_canary.size(); i++)
        if (g_canary[i].user == user) { g_canary[i] = g_canary.back(); g_canary.pop_back(); return; }
}
// Copies both zones of every registered buffer back and compares them with the pattern; the report names each damaged buffer by the
// source line that allocated it, the side, the first damaged byte's offset from the buffer's end (or start) and the 4 bytes found there.
// Synchronises the device first: every kernel of the requests so far has finished.
int canary_check(std::string *report)
{
    std::lock_guard<std::mutex> lk(g_canary_mu);
    if (hipDeviceSynchronize() != hipSuccess) { if (report) *report += "hipDeviceSynchronize failed; "; return -1; }
    int bad = 0;
    std::vector<unsigned char> h;
    for (const CanaryRec &r : g_canary) {
        const size_t padded = (r.bytes + kCanaryGuard - 1) / kCanaryGuard * kCanaryGuard, back = padded - r.bytes + kCanaryGuard;
        bool hit = false;
        for (int side = 0; side < 2; side++) {
            const size_t len = side ? back : kCanaryGuard;
            const char *src = side ? r.user + r.bytes : r.user - kCanaryGuard;
            h.resize(len);
            if (hipMemcpy(h.data(), src, len, hipMemcpyDeviceToHost) != hipSuccess) { if (report) *report += "hipMemcpy of a guard zone failed; "; return -1; }
            for (size_t i = 0; i < len; i++)
                if (h[i] != (unsigned char)kCanaryByte) {
                    hit = true;
                    if (report) {
                        char buf[256];
                        const size_t w = i / 4 * 4;
                        unsigned word = 0;
                        memcpy(&word, h.data() + w, std::min<size_t>(4, len - w));
                        snprintf(buf, sizeof buf, "%s:%d (%zu bytes): %s guard damaged at %s%zu, word there 0x%08x; ", r.file, r.line, r.bytes,
                                 side ? "back" : "front", side ? "end+" : "start-", side ? i : kCanaryGuard - i, word);
                        *report += buf;
                    }
                    break;
                }
        }
        bad += hit ? 1 : 0;
    }
    return bad;
}
// what every entry point of the testing build ends with (engine_state.h): opt-in, the guard zones around every device buffer
int check_guards(haf_engine *e)
{
    if (!test_env("HAF_CANARY_CHECK")) return HAF_OK;
    std::string rep;
    const int bad = canary_check(&rep);
    if (bad != 0) return fail(e, HAF_E_INTERNAL, "device buffer guard zones damaged (" + std::to_string(bad) + "): " + rep);
    return HAF_OK;
}
}  // namespace haf_host

extern "C" {

// number of device buffers whose guard zones were written (0 = intact, < 0: HIP failure); msg (cap bytes) names them.  Covers every
// engine of the process.
int haf_test_check_canaries(char *msg, int cap)
{
    std::string rep;
    const int bad = canary_check(&rep);
    if (msg && cap > 0) { strncpy(msg, rep.c_str(), (size_t)cap - 1); msg[cap - 1] = 0; }
    return bad;
}
// how many buffers are registered (the test checks that the hook sees the engine's buffers at all)
int haf_test_canary_buffers()
{
    std::lock_guard<std::mutex> lk(g_canary_mu);
    return (int)g_canary.size();
}
// the device lists of the last request as they lie in memory: 0 the evaluation list (cell ids), 1 the exact tiers' input list, 2 the
// exact-integer tier's hand-over list, 3 the strict tier's list, 4 the screening pass's list.  *n = entries the list holds.
int haf_test_fetch_list(haf_engine *e, int which, int *out, int cap, int *n)
{
    if (!e || !out || !n || cap < 0) return HAF_E_ARG;
    const int *src = nullptr;
    int cnt = 0;
    switch (which) {
        case 0: src = e->d_evalcell.p; cnt = e->last.evals; break;
        case 1: src = e->d_flag_list.p; cnt = std::min(e->last.flagged, e->list_cap); break;
        case 2: src = e->d_flagi_list.p; cnt = e->last.i8 ? std::min(e->last.flaggedi, e->list_cap) : 0; break;
        case 3: src = e->d_flag2_list.p; cnt = std::min(e->last.flagged2, e->list_cap); break;
        case 4: src = e->d_flag0_list.p; cnt = std::min(e->last.flagged0, e->flag0_cap); break;
        default: return HAF_E_ARG;
    }
    *n = cnt;
    if (!src || cnt <= 0) { *n = 0; return HAF_OK; }
    if (hipDeviceSynchronize() != hipSuccess) return HAF_E_DEVICE;
    return hipMemcpy(out, src, (size_t)std::min(cnt, cap) * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess ? HAF_OK : HAF_E_DEVICE;
}
int haf_test_overflow_stats(haf_engine *e, long long *out2)
{
    if (!e || !out2) return HAF_E_ARG;
    out2[0] = e->stat_flag0_overflows; out2[1] = e->stat_extra_windows;
    return HAF_OK;
}
// which pre-stage kernels served the last request, as run_prestages got it from the launchers (kernels.h: BinForm, IntegralForm):
// out[0] the binning form -- 0 k_bin, 1 k_bin_lds, 2 bucket-sorted k_bin_tiles, 3 inside k_small_pre<true>, 4 k_bin_lds followed by
// k_small_pre<false>; out[1] the integral form -- 0 k_integral_small, 1 band form, 2 inside k_small_pre; out[2] 1 when launch_bin refused the
// bucket-sorted path because the bucket grid exceeds kBktMaxBuckets; out[3] n_inexact_grids.  -1, -1, 0, 0 before the first request.
int haf_test_prestage_forms(haf_engine *e, int *out4)
{
    if (!e || !out4) return HAF_E_ARG;
    out4[0] = e->pre_forms.bin; out4[1] = e->pre_forms.integral; out4[2] = e->pre_forms.bucket_refused ? 1 : 0; out4[3] = e->last.inexact;
    return HAF_OK;
}
// Snapshot of the screening feature pass: with on != 0 every later request whose screening tier runs its feature kernel copies what that
// kernel wrote -- the fp16 operand images (20 KiB per tile of 32 evaluations), the 8 band floats per evaluation (the RAW sums in the
// low-rank form) and a_x -- aside before the sweep, the projection and the later tiers reuse the buffers.  Sized for the engine's
// largest request.
int haf_test_snapshot_screen(haf_engine *e, int on)
{
    if (!e) return HAF_E_ARG;
    if (on && !e->snap_X.p) {
        if (e->snap_X.alloc((size_t)(e->max_evals_pad / kTile) * (size_t)kS0MatBytes) != hipSuccess ||
            e->snap_gband.alloc((size_t)e->max_evals_pad * kBandFloats) != hipSuccess || e->snap_ax.alloc((size_t)e->max_evals_pad) != hipSuccess)
            return HAF_E_DEVICE;
    }
    // ... and of what the sweep launches leave (engine_request.cpp: snapshot_sweep): [0] the first pass, [1] tier 0b with its list-indexed input
    for (int k = 0; on && k < 2; k++) {
        haf_engine::SweepSnap &sn = e->snap_sweep[k];
        if (sn.dec.p) continue;
        const size_t pad = (size_t)e->max_evals_pad, part = std::min<size_t>(e->d_screen_part.n, (size_t)16 * pad * 16);
        if (sn.dec.alloc(pad) != hipSuccess || sn.margin.alloc(pad) != hipSuccess || sn.words.alloc(pad / 64 + 1) != hipSuccess ||
            sn.list.alloc((size_t)std::max(e->flag0_cap, 1)) != hipSuccess || sn.counters.alloc(CNT_COUNT) != hipSuccess || sn.part.alloc(part) != hipSuccess)
            return HAF_E_DEVICE;
        if (sn.labels.alloc(e->d_labels.n) != hipSuccess || sn.raw.alloc(pad * kBandFloats) != hipSuccess ||
            (k == 0 && e->mdl.lr_available && sn.Y.alloc((size_t)(e->max_evals_pad / kTile) * (size_t)kLrMatBytes) != hipSuccess))
            return HAF_E_DEVICE;
        if (k == 1 && (sn.in_X.alloc((size_t)(e->max_evals_pad / kTile) * (size_t)kS0MatBytes) != hipSuccess ||
                       sn.in_gband.alloc(pad * kBandFloats) != hipSuccess || sn.in_ax.alloc(pad) != hipSuccess))
            return HAF_E_DEVICE;
    }
    e->snap_on = on != 0;
    if (!on) e->snap_cap = 0;
    return HAF_OK;
}
// bytes [offset, offset + bytes) of the last snapshot: which = 0 operand images, 1 band floats, 2 a_x; *avail = bytes the snapshot holds
int haf_test_fetch_snapshot(haf_engine *e, int which, long long offset, void *out, long long bytes, long long *avail)
{
    if (!e || !avail || offset < 0 || bytes < 0 || which < 0 || which > 2) return HAF_E_ARG;
    const char *src = which == 0 ? e->snap_X.p : which == 1 ? reinterpret_cast<const char *>(e->snap_gband.p) : reinterpret_cast<const char *>(e->snap_ax.p);
    const long long have = which == 0 ? (long long)((e->snap_cap + kTile - 1) / kTile) * kS0MatBytes
                                      : (long long)e->snap_cap * (which == 1 ? kBandFloats : 1) * (long long)sizeof(float);
    *avail = src ? have : 0;
    if (!bytes) return HAF_OK;
    if (!src || !out || offset + bytes > have) return HAF_E_ARG;
    if (hipDeviceSynchronize() != hipSuccess) return HAF_E_DEVICE;
    return hipMemcpy(out, src + offset, (size_t)bytes, hipMemcpyDeviceToHost) == hipSuccess ? HAF_OK : HAF_E_DEVICE;
}
// Which sweep launch `slot` (0 the first pass, 1 tier 0b) of the last request was, as its launcher reported it (kernels.h: SweepForm):
// out [9] = variant (-1: no such launch), lr, part, fused, gather, list, compaction (0 one workgroup, 1 two launches), blocks, and the
// evaluation slots the launch covered.
int haf_test_sweep_form(haf_engine *e, int slot, long long *out9)
{
    if (!e || !out9 || slot < 0 || slot > 1) return HAF_E_ARG;
    const haf_engine::SweepSnap &sn = e->snap_sweep[slot];
    const SweepForm &f = sn.form;
    const long long v[9] = {f.variant, f.lr, f.part, f.fused, f.gather, f.list, f.compaction, f.blocks, sn.cap};
    memcpy(out9, v, sizeof v);
    return HAF_OK;
}
// bytes [offset, offset + bytes) of what sweep launch `slot` of the last request left while the snapshot was on: which = 0 dec, 1 margin
// (HAF_FLAG_KEEP_DEBUG), 2 the flag words, 3 the output list (flag0_cap entries, whatever the counter says), 4 the counters right behind
// the launch, 5 part_buf (PART form: slice k at float4 index k * blocks * 256), 6 / 7 / 8 tier 0b's list-indexed operand images, bands
// and a_x (slot 1, list-image form), 9 the label grids (int8, every cell of the engine's grids), 10 the raw sums as a low-rank sweep read
// them, 11 the projected 6-step images k_project wrote (low-rank form in two launches).  *avail = bytes held.
int haf_test_fetch_sweep(haf_engine *e, int slot, int which, long long offset, void *out, long long bytes, long long *avail)
{
    if (!e || !avail || slot < 0 || slot > 1 || offset < 0 || bytes < 0 || which < 0 || which > 11) return HAF_E_ARG;
    const haf_engine::SweepSnap &sn = e->snap_sweep[slot];
    const long pad = (sn.cap + kS0BlockEvals - 1) / kS0BlockEvals * kS0BlockEvals;
    const char *src = nullptr;
    long long have = 0;
    switch (which) {
        case 0: src = (const char *)sn.dec.p; have = sn.dec_cap * 4; break;
        case 1: src = (const char *)sn.margin.p; have = e->d_margin.p ? sn.dec_cap * 4 : 0; break;
        case 2: src = (const char *)sn.words.p; have = std::min<long long>(pad / 64, (long long)sn.words.n) * 8; break;
        case 3: src = (const char *)sn.list.p; have = sn.list_cap * 4; break;
        case 4: src = (const char *)sn.counters.p; have = sn.cap ? CNT_COUNT * 4 : 0; break;
        case 5: src = sn.part.p; have = sn.part_bytes; break;
        case 6: src = sn.in_X.p; have = sn.in_X.p ? std::min<long long>((sn.cap + kTile - 1) / kTile * (long long)kS0MatBytes, (long long)sn.in_X.n) : 0; break;
        case 7: src = (const char *)sn.in_gband.p; have = sn.in_gband.p ? sn.cap * kBandFloats * 4 : 0; break;
        case 8: src = (const char *)sn.in_ax.p; have = sn.in_ax.p ? sn.cap * 4 : 0; break;
        case 9: src = (const char *)sn.labels.p; have = sn.cap ? (long long)sn.labels.n : 0; break;
        case 10: src = (const char *)sn.raw.p; have = sn.raw_cap * kBandFloats * 4; break;
        default: src = sn.Y.p; have = sn.y_bytes; break;
    }
    *avail = src ? have : 0;
    if (!bytes) return HAF_OK;
    if (!src || !out || offset + bytes > have) return HAF_E_ARG;
    if (hipDeviceSynchronize() != hipSuccess) return HAF_E_DEVICE;
    return hipMemcpy(out, src + offset, (size_t)bytes, hipMemcpyDeviceToHost) == hipSuccess ? HAF_OK : HAF_E_DEVICE;
}
// writes `count` ints of value `v` at int offset `at` relative to the END of the d_flag0_list buffer (at >= 0) of this engine -- the
// canary test's own "bug": what a producer that ignores its capacity does
int haf_test_poke_flag0_list(haf_engine *e, int at, int count, int v)
{
    if (!e || !e->d_flag0_list.p) return HAF_E_ARG;
    std::vector<int> h((size_t)count, v);
    return hipMemcpy(e->d_flag0_list.p + e->d_flag0_list.n + at, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice) == hipSuccess ? HAF_OK : HAF_E_DEVICE;
}

// the last scored batch as haf_test_revote sees it: *B clouds x *R rolls (0 x 0 before the first request)
int haf_test_last_batch(haf_engine *e, int *B, int *R)
{
    if (!e || !B || !R) return HAF_E_ARG;
    *B = e->last.B; *R = e->last.R;
    return HAF_OK;
}

// Votes again on host-chosen grids: the last scored batch's B x R grids of grid_h x grid_w are replaced by `labels` (int8, a plain
// engine) or `gridf` (fp32, an engine with HAF_FLAG_PROBABILITY) -- exactly one of the two, B*R*H*W values -- and, when given, the
// height grids by `heights` (B*R*H*W floats) and the ROI cell sets by `roi_words` (B*R*H*roi_row_words(W) words, the layout of
// haf_roi_cells; the engine must have served an ROI request before).  Then the request path's own launchers run on the engine's
// stream: launch_vote, launch_vote_roi with roi_words, launch_probability_vote for gridf.  records_out: the B x R roll records.  The
// device's records, vote grids and heights stay, so haf_get_roll_grid, haf_top_grasps, haf_grasp_map, haf_grasp_map_best and
// haf_cell_pose describe the re-voted grids (they read the device's records; the pinned host copy is refreshed all the same).
static int revote_impl(haf_engine *e, const int8_t *labels, const float *gridf, const float *heights, const unsigned long long *roi_words,
                       haf_roll_record *records_out)
{
    if (!records_out || (labels != nullptr) == (gridf != nullptr)) return fail(e, HAF_E_ARG, "haf_test_revote: exactly one of labels and gridf, and records_out");
    if ((gridf != nullptr) != e->mdl.prob_mode) return fail(e, HAF_E_ARG, "haf_test_revote: labels go with a plain engine, gridf with HAF_FLAG_PROBABILITY");
    if (roi_words && !labels) return fail(e, HAF_E_ARG, "haf_test_revote: roi_words go with labels");
    const LastCall &last = e->last;
    if (last.B < 1 || last.R < 1 || last.B > e->cfg.max_clouds || last.R > e->max_rolls) return fail(e, HAF_E_ARG, "haf_test_revote: no scored batch");
    const int H = e->cfg.grid_h, W = e->cfg.grid_w, BR = last.B * last.R;
    const size_t cells = (size_t)BR * H * W, words = (size_t)BR * H * (size_t)roi_row_words(W);
    if (cells > e->cells_cap || e->d_heights.n < cells || (labels ? e->d_labels.n < cells || e->d_ev16.n < cells : e->d_gridf.n < cells || e->d_evf.n < cells) ||
        e->d_brcount.n < (size_t)BR || (labels && (H * W > 16384) && (e->d_topkey.n < (size_t)2 * BR || e->d_rowmax.n < (size_t)BR * H)))
        return fail(e, HAF_E_ARG, "haf_test_revote: the batch does not fit the engine's buffers");
    if (roi_words && (!e->d_roi_cells.p || e->d_roi_cells.n < words)) return fail(e, HAF_E_ARG, "haf_test_revote: no ROI cell sets (no ROI request yet)");
    HIPCHK(e, hipSetDevice(e->cfg.device));
    const hipStream_t s = e->stream;
    HIPCHK(e, hipStreamSynchronize(s));
    if (labels) HIPCHK(e, hipMemcpyAsync(e->d_labels.p, labels, cells, hipMemcpyHostToDevice, s));
    if (gridf) HIPCHK(e, hipMemcpyAsync(e->d_gridf.p, gridf, cells * sizeof(float), hipMemcpyHostToDevice, s));
    if (heights) HIPCHK(e, hipMemcpyAsync(e->d_heights.p, heights, cells * sizeof(float), hipMemcpyHostToDevice, s));
    if (roi_words) HIPCHK(e, hipMemcpyAsync(e->d_roi_cells.p, roi_words, words * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    Dims d{};
    d.H = H; d.W = W; d.R = last.R; d.B = last.B; d.nf = e->mdl.nf; d.n_sv = e->model.n_sv; d.n_sv_tiles = e->mdl.n_sv_tiles; d.sv_tile_neg = e->mdl.sv_tile_neg;
    const float *hts = reinterpret_cast<const float *>(e->d_heights.p);
    if (gridf)
        launch_probability_vote(e->d_gridf.p, hts, e->d_brcount.p, e->d_evf.p, e->d_rec.p, d, s);
    else if (roi_words)
        launch_vote_roi(e->d_labels.p, hts, e->d_brcount.p, e->d_ev16.p, e->d_topkey.p, e->d_rowmax.p, e->d_rec.p, e->d_roi_cells.p, d, s);
    else
        launch_vote(e->d_labels.p, hts, e->d_brcount.p, e->d_ev16.p, e->d_topkey.p, e->d_rowmax.p, e->d_rec.p, d, s);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(e->h_rec, e->d_rec.p, (size_t)BR * sizeof(RollRecordDev), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    for (int i = 0; i < BR; i++) {
        records_out[i].vote = e->h_rec[i].vote;
        records_out[i].row = e->h_rec[i].row;
        records_out[i].col = e->h_rec[i].col;
        records_out[i].h_locmax = e->h_rec[i].h_locmax;
        records_out[i].n_evals = e->h_rec[i].n_evals;
    }
    return HAF_OK;
}
int haf_test_revote(haf_engine *e, const int8_t *labels, const float *gridf, const float *heights, const unsigned long long *roi_words,
                    haf_roll_record *records_out)
{
    if (!e) return HAF_E_ARG;
    return guarded(&e->error, [&] { return revote_impl(e, labels, gridf, heights, roi_words, records_out); });
}

// host-only hooks: parsers, per-roll geometry and the cross-roll rule/pose, none of which touches a device
int haf_test_feature_table(const char *path, int *n, int *reg /* cap*16 */, float *w /* cap*4 */, int cap)
{
    std::vector<FeatureRow> rows;
    std::string err;
    if (!load_features(path, rows, err)) return HAF_E_IO;
    *n = (int)rows.size();
    for (int i = 0; i < *n && i < cap; i++) {
        memcpy(reg + i * 16, rows[(size_t)i].reg, sizeof rows[0].reg);
        memcpy(w + i * 4, rows[(size_t)i].w, sizeof rows[0].w);
    }
    return HAF_OK;
}

int haf_test_range_table(const char *path, double *lower, double *upper, int *max_index, double *fmin, double *fmax,
                         unsigned char *present, int cap)
{
    RangeTable rt;
    std::string err;
    if (!load_range(path, rt, err)) return HAF_E_IO;
    *lower = rt.lower; *upper = rt.upper; *max_index = rt.max_index;
    for (int i = 0; i <= rt.max_index && i < cap; i++) { fmin[i] = rt.fmin[(size_t)i]; fmax[i] = rt.fmax[(size_t)i]; present[i] = rt.present[(size_t)i]; }
    return HAF_OK;
}

int haf_test_model(const char *path, double *gamma, double *rho, int *n_sv, int *dim, int *n_sv_class, int *label, double *coef,
                   double *sv, long cap_sv_values)
{
    SvmModel m;
    std::string err;
    if (!load_model(path, m, err)) return HAF_E_IO;
    *gamma = m.gamma; *rho = m.rho; *n_sv = m.n_sv; *dim = m.dim;
    n_sv_class[0] = m.n_sv_class[0]; n_sv_class[1] = m.n_sv_class[1];
    label[0] = m.label[0]; label[1] = m.label[1];
    if (coef && sv && (long)m.sv.size() <= cap_sv_values) {
        memcpy(coef, m.coef.data(), m.coef.size() * sizeof(double));
        memcpy(sv, m.sv.data(), m.sv.size() * sizeof(double));
    }
    return HAF_OK;
}

int haf_test_model_kernel(const char *path, int *kernel_type, int *degree, double *coef0, double *gamma)
{
    SvmModel m;
    std::string err;
    if (!load_model(path, m, err)) return HAF_E_IO;
    *kernel_type = m.kernel_type; *degree = m.degree; *coef0 = m.coef0; *gamma = m.gamma;
    return HAF_OK;
}

// out: 12 transform floats, then sa, ca, cx1, cy1, cx2, cy2, cx3, cy3, cx4, cy4; full 4x4 (generate_grid form) in m16
int haf_test_roll_geo(const haf_config *cfg, const haf_grasp_input *in, int roll, float *out22, float *m16, float *m16_pose)
{
    NormalisedInput n = normalise(*in);
    RollGeo g;
    fill_roll_geo(*cfg, *in, n, roll, g);
    memcpy(out22, g.m, 12 * 4);
    const float tail[10] = {g.sa, g.ca, g.cx1, g.cy1, g.cx2, g.cy2, g.cx3, g.cy3, g.cx4, g.cy4};
    memcpy(out22 + 12, tail, sizeof tail);
    if (m16) { Mat4 m = roll_transform(*cfg, *in, n, roll, true); memcpy(m16, m.a, 64); }
    if (m16_pose) { Mat4 m = roll_transform(*cfg, *in, n, roll, false); memcpy(m16_pose, m.a, 64); }
    return HAF_OK;
}

int haf_test_finalize(const haf_config *cfg, const haf_grasp_input *in, const haf_roll_record *rec, haf_grasp_output *out)
{
    std::string err;
    return finalize_impl(*cfg, in, rec, out, err);
}

int haf_test_roll_pose(const haf_config *cfg, const haf_grasp_input *in, const haf_roll_record *rec, int roll, haf_grasp_output *out,
                       int32_t *published)
{
    std::string err;
    return roll_pose_impl(*cfg, in, rec, roll, out, published, err);
}

// steps 4-6 of haf_top_grasps without a device: n_lists per-roll greedy sequences (ascending roll order), list i holding n_cand[i]
// records (concatenated in rec / run_len) of global roll roll[i], more[i] = its sequence may go on.  *need_more = 1: a list ran out while
// its sequence may go on (haf_top_grasps redoes its device pass with a larger depth then; out is not final).
int haf_test_top_merge(const haf_config *cfg, const haf_grasp_input *in, int n_lists, const int32_t *roll, const int32_t *n_cand,
                       const int32_t *more, const haf_roll_record *rec, const int32_t *run_len, int k, int roll_window, double min_dist_m,
                       haf_grasp_candidate *out, int32_t *n_found, int32_t *need_more)
{
    if (!cfg || !in || n_lists < 0 || k < 1 || !out || !n_found || !need_more) return HAF_E_ARG;
    std::vector<TopList> lists((size_t)n_lists);
    size_t at = 0;
    for (int i = 0; i < n_lists; i++) {
        lists[(size_t)i].roll = roll[i];
        lists[(size_t)i].n = n_cand[i];
        lists[(size_t)i].more = more[i] != 0;
        lists[(size_t)i].rec = rec + at;
        lists[(size_t)i].len = run_len + at;
        at += (size_t)n_cand[i];
    }
    std::string err;
    bool nm = false;
    const int rc = top_merge(*cfg, in, lists, k, roll_window, min_dist_m, out, n_found, &nm, err);
    *need_more = nm ? 1 : 0;
    return rc;
}

// ---- test hooks (host and device builds of the decimal round-trip arithmetic; see tests/) ----
double haf_test_decq_host(double x, int digits) { return digits == 40 ? hafq::decq4_float((float)x) : hafq::decq(x, digits); }
double haf_test_scale_host(double q4, double fmin, double fmax, double lower, double upper)
{
    const double range = fmax - fmin;
    return hafq::scale_q6(q4, fmin, fmax, range, 1.0 / range, lower, upper);
}

// host-side pieces of the screening band (tests/test_host_cpu.py)
double haf_test_sigma_upper(const double *M, int n, int d) { return sigma_upper_bound(M, n, d); }
}  // extern "C"

// ---- digests of the model tables (tests/test_tables_gpu.py, tests/golden/table_digests.json) ----
// One line "name=<64-bit FNV-1a, 16 hex digits>" per device table, per parameter struct and one for the scalars and flags that the
// table work sets.  A table's digest is that of its bytes as they lie in memory (an unallocated table: the digest of nothing).  A
// parameter struct is hashed member by member, so that neither its device pointers nor its padding bytes count.
namespace {
struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void add(const void *p, size_t n)
    {
        const unsigned char *b = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    }
    template <class T> Fnv &operator<<(const T &x) { static_assert(std::is_arithmetic_v<T>, "one member at a time"); add(&x, sizeof x); return *this; }
};
struct DigestText {
    std::string text;
    void line(const char *name, const Fnv &f)
    {
        char buf[96];
        snprintf(buf, sizeof buf, "%s=%016llx\n", name, (unsigned long long)f.h);
        text += buf;
    }
};
Fnv digest_of(const ScreenParams &p)
{
    Fnv f;
    f << p.c << p.v_max << p.dv_max << p.das_max << p.as_max << p.sigma_v << p.sigma_dv << p.sqrt_cmax << p.scale << p.eta_abs << p.sigma_dk
      << p.ck_max << p.ubar2 << p.acc_rel << p.g_norm << p.hd_norm << p.fast_groups << p.extra_groups << p.cr << p.cr_poly << p.cr_nN << p.cr_nM
      << p.cr_nHabs << p.cr_nDabs << p.cr_nHaa << p.cr_Ca << p.cr_Cq1 << p.cr_Cqq << p.cr_Babs << p.cr_qmax << p.cr_dqmax << p.cr_gnorm
      << p.cr_mu_norm << p.cr_mu_norm_t << p.lr << p.lr_rho;
    return f;
}
Fnv digest_of(const LrBand &p)
{
    Fnv f;
    f << p.sigB << p.sigAbsB << p.acc10 << p.acc6 << p.qmax << p.dqmax << p.rmax << p.nN1 << p.nM1 << p.nN2 << p.nHabs << p.nDabs << p.nRabs
      << p.sQb << p.sQtaa << p.Ca << p.Cq1 << p.Cqq << p.Babs << p.gnorm << p.mu_norm << p.mu_norm_t << p.eta_abs << p.scale << p.poly << p.pad
      << p.sig_q << p.sig_dq << p.sig_r << p.sbq << p.sbr << p.rho_norm << p.gt_norm << p.bg_norm << p.bh_norm << p.gabsB;
    return f;
}
Fnv digest_of(const CrParams &p) { Fnv f; f << p.B0 << p.rho; return f; }
Fnv digest_of(const CrT1Params &p)
{
    Fnv f;
    f << p.B0 << p.rho << p.c << p.nN << p.nM << p.nHabs << p.nDabs << p.nHaa << p.Ca << p.Cqq << p.Babs << p.qmax << p.dqmax << p.acc_rel
      << p.dp_rel << p.dp_abs << p.sum_rel << p.scale << p.guard_abs << p.gv0 << p.gv1 << p.pad;
    return f;
}
Fnv digest_of(const SvmParams &p)
{
    Fnv f;
    f << p.two_gamma2 << p.neg_gamma2 << p.rho << p.guard_acc << p.guard_dot << p.guard_abs << p.as_max << p.guard_dot_p << p.guard_acc0
      << p.guard_acc0_s << p.guard_acc_l << p.gv0 << p.gv1 << p.sqrt_cmax;
    return f;
}
Fnv digest_of(const ExactParams &p)
{
    Fnv f;
    f << p.gamma << p.rho << p.lower << p.upper << p.guard2 << p.as_max1 << p.gamma2 << p.n_sv << p.n_sv_pad << p.kx << p.gv0 << p.gv1
      << p.kernel_type << p.degree << p.coef0;
    return f;
}
Fnv digest_of(const I8Params &p)
{
    Fnv f;
    f << p.gamma << p.rho << p.gamma2 << p.drop << p.delta << p.dq_scale << p.s_max << p.guard_scale << p.n_sv_pad << p.gv0 << p.gv1 << p.pad;
    return f;
}
Fnv digest_of(const ProbParams &p) { Fnv f; f << p.A << p.B << p.gv0 << p.gv1 << p.hdr << p.host_all << p.dec_slack; return f; }
// the parameter structs, then the scalars and flags in ModelConsts' order, flags as one byte each
void digest_consts(DigestText &t, const ModelConsts &c)
{
    t.line("screen", digest_of(c.screen)); t.line("screen_cr", digest_of(c.screen_cr)); t.line("screen_lrp", digest_of(c.screen_lrp));
    t.line("lr_band", digest_of(c.lr_band)); t.line("crp", digest_of(c.crp)); t.line("crt1", digest_of(c.crt1)); t.line("svm", digest_of(c.svm));
    t.line("exact", digest_of(c.exact)); t.line("i8", digest_of(c.i8)); t.line("prob", digest_of(c.prob));
    Fnv f;
    f << c.nf << c.kx << c.n_sv_tiles << c.sv_tile_neg << c.n_sv_pad << c.sum_abs_coef << c.screen_active << c.cr_available << c.lr_available
      << c.lr_fused << c.lr_plain_available << c.t1_cr_available << c.i8_active << c.lr_rank << c.gv0 << c.gv1 << c.prob_mode << c.host_exp_thr;
    t.line("scalars", f);
}
int digest_hand_over(const DigestText &t, char *out, int cap)
{
    if (!out || cap <= 0 || t.text.size() + 1 > (size_t)cap) return HAF_E_CAPACITY;
    memcpy(out, t.text.c_str(), t.text.size() + 1);
    return HAF_OK;
}
// a table's bytes as they lie in memory, on the device or on the host, into f; false: they could not be read
template <class T> bool add_table(Fnv &f, const DevBuf<T> &b)
{
    std::vector<char> h(b.p ? b.n * sizeof(T) : 0);
    if (!h.empty() && hipMemcpy(h.data(), b.p, h.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
    f.add(h.data(), h.size());
    return true;
}
template <class T> bool add_table(Fnv &f, const std::vector<T> &v) { f.add(v.data(), v.size() * sizeof(T)); return true; }
// the digest text of a model, DeviceModel or ModelTables: one line "d_<name>" per table, then the constants'
template <class Model> bool digest_model(DigestText &t, const Model &m)
{
    bool ok = true;
    for_each_table([&](const char *name, const auto &b) {
        Fnv f;
        ok = ok && add_table(f, b);
        t.line((std::string("d_") + name).c_str(), f);
    }, m);
    digest_consts(t, m);
    return ok;
}
}  // namespace

// what the device-free builder (model_tables.cpp) makes of cfg's files and flags under the testing build's environment switches, as
// haf_create would ask for it; a file that does not load or a refusal of the builder comes back as its code, with its text in err
static int host_tables(const haf_config *cfg, double kappa, double kappa16, ModelTables &m, std::string &err)
{
    std::vector<FeatureRow> features;
    RangeTable range;
    SvmModel model;
    if (!load_features(cfg->feature_file, features, err) || !load_range(cfg->range_file, range, err) || !load_model(cfg->model_file, model, err))
        return HAF_E_IO;
    TableInputs in;
    in.cfg = *cfg;
    in.features = &features; in.range = &range; in.model = &model;
    in.mfma_kappa = kappa; in.mfma_kappa16 = kappa16;
    in.generic_kernel = model.kernel_type != HAF_KERNEL_RBF;
    if (in.generic_kernel) in.cfg.flags = (in.cfg.flags & ~(uint32_t)HAF_FLAG_FP32_MFMA) | HAF_FLAG_SPLIT_F16;      // (as haf_create does)
    in.sw = table_switches();
    const TableError refused = build_model_tables(in, m);
    if (refused.code != HAF_OK) { err = refused.msg; return refused.code; }
    return HAF_OK;
}

extern "C" {

// the tables of a created engine as they lie on the device, its parameter structs and its scalars -> text of at most cap bytes
int haf_test_table_digest(haf_engine *e, char *out, int cap)
{
    if (!e) return HAF_E_ARG;
    if (hipSetDevice(e->cfg.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return HAF_E_DEVICE;
    DigestText t;
    if (!digest_model(t, e->mdl)) return HAF_E_DEVICE;
    return digest_hand_over(t, out, cap);
}

// The same digests, under the same names, of what the device-free builder makes of cfg's files and flags (model_tables.cpp): no device
// is touched.  kappa, kappa16: haf_engine::mfma_kappa*; the environment switches are the testing build's.  A file that does not load
// or a refusal of the builder comes back as its code, with its text in msg (msg_cap bytes).
int haf_test_host_table_digest(const haf_config *cfg, double kappa, double kappa16, char *out, int cap, char *msg, int msg_cap)
{
    if (!cfg || !cfg->feature_file || !cfg->range_file || !cfg->model_file) return HAF_E_ARG;
    std::string err;
    auto say = [&](int code) {
        if (msg && msg_cap > 0) { strncpy(msg, err.c_str(), (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; }
        return code;
    };
    const int rc = guarded(&err, [&]() {
        ModelTables m;
        const int built = host_tables(cfg, kappa, kappa16, m, err);
        if (built != HAF_OK) return say(built);
        DigestText t;
        digest_model(t, m);
        return digest_hand_over(t, out, cap);
    });
    return rc == HAF_E_INTERNAL ? say(rc) : rc;       // (an exception's text)
}

// The slot descriptors the screening feature kernels read, from the same device-free build (no device is touched): for each of the kS0K
// slots of one ScreenParams instance -- form 0 `screen`, 1 `screen_cr`, 2 `screen_lrp` -- attr: the representative attribute (row of the
// feature file; -1 for an unused slot), skip / shaf: as its FeatDesc holds them, desc [kS0K][4]: {scr_mul, scr_add, extra, pad} as the
// floats ScrDesc holds, corr [kS0K][3]: the slot's ScrCorr {g, hd, ub}, mu [kS0K]: the centre the centred forms fold into scr_add (0 in
// form 0).  scalars [7]: c, lr_rho, ubar2, eta_abs, cr (0 / 1), cr_mu_norm, cr_mu_norm_t; groups [2]: fast_groups, extra_groups.  *available = 0: the model did not get this form's tables (the arrays are left alone).
int haf_test_host_slot_table(const haf_config *cfg, double kappa, double kappa16, int form, int *attr, int *skip, int *shaf, float *desc,
                             float *corr, double *mu, double *scalars, unsigned long long *groups, int *available, char *msg, int msg_cap)
{
    if (!cfg || !cfg->feature_file || !cfg->range_file || !cfg->model_file || form < 0 || form > 2 || !attr || !skip || !shaf || !desc || !corr || !mu ||
        !scalars || !groups || !available)
        return HAF_E_ARG;
    std::string err;
    auto say = [&](int code) {
        if (msg && msg_cap > 0) { strncpy(msg, err.c_str(), (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; }
        return code;
    };
    const int rc = guarded(&err, [&]() {
        ModelTables m;
        const int built = host_tables(cfg, kappa, kappa16, m, err);
        if (built != HAF_OK) return say(built);
        // (as upload_tables pairs them: the low-rank form's plain epilogue reads the centred descriptors with correction vectors of its own)
        const ScreenParams &sp = form == 0 ? m.screen : form == 1 ? m.screen_cr : m.screen_lrp;
        const std::vector<ScrDesc> &sd = form == 0 ? m.sd : m.sd_cr;
        const std::vector<FeatDesc> &fds = form == 0 ? m.fd_slot : m.fd_slot_cr;
        const std::vector<ScrCorr> &sc = form == 0 ? m.corr : form == 1 ? m.corr_cr : m.corr_lrp;
        *available = m.screen_active && (form == 0 || (form == 1 && m.cr_available) || (form == 2 && m.lr_available)) &&
                     sd.size() >= (size_t)kS0K && fds.size() >= (size_t)kS0K && sc.size() >= (size_t)kS0K;
        if (!*available) return (int)HAF_OK;
        for (int s = 0; s < kS0K; s++) {
            attr[s] = (s < (int)m.slot_rep.size() && !fds[(size_t)s].skip) ? m.slot_rep[(size_t)s] : -1;
            skip[s] = fds[(size_t)s].skip; shaf[s] = fds[(size_t)s].shaf;
            desc[4 * s] = sd[(size_t)s].scr_mul; desc[4 * s + 1] = sd[(size_t)s].scr_add; desc[4 * s + 2] = sd[(size_t)s].extra; desc[4 * s + 3] = sd[(size_t)s].pad;
            mu[s] = (form != 0 && s < (int)m.slot_mu.size()) ? m.slot_mu[(size_t)s] : 0.0;
            corr[3 * s] = sc[(size_t)s].g; corr[3 * s + 1] = sc[(size_t)s].hd; corr[3 * s + 2] = sc[(size_t)s].ub;
        }
        scalars[0] = sp.c; scalars[1] = sp.lr_rho; scalars[2] = sp.ubar2; scalars[3] = sp.eta_abs; scalars[4] = sp.cr;
        scalars[5] = sp.cr_mu_norm; scalars[6] = sp.cr_mu_norm_t;
        groups[0] = sp.fast_groups; groups[1] = sp.extra_groups;
        return (int)HAF_OK;
    });
    return rc == HAF_E_INTERNAL ? say(rc) : rc;
}

// The tables the sweep kernels read, from the same device-free build (no device is touched).  which = 0 svt0, 1 svt0_cr, 2 svt_lr,
// 3 lr_btiles: its bytes into out (cap bytes; *bytes = its size, 0 when the model did not get it).  ints [4]:
// n_sv_tiles, sv_tile_neg, gv0, gv1.  scalars [12]: SvmParams rho, guard_acc0, guard_acc0_s, guard_abs, sqrt_cmax; CrParams B0, rho;
// acc_rel of `screen` and of `screen_cr`; LrBand acc6, acc10; the flag words up to which the one-workgroup list compaction serves.
int haf_test_host_sweep_tables(const haf_config *cfg, double kappa, double kappa16, int which, void *out, long long cap, long long *bytes,
                               int *ints, double *scalars, char *msg, int msg_cap)
{
    if (!cfg || !cfg->feature_file || !cfg->range_file || !cfg->model_file || which < 0 || which > 3 || !bytes || !ints || !scalars || cap < 0) return HAF_E_ARG;
    std::string err;
    auto say = [&](int code) {
        if (msg && msg_cap > 0) { strncpy(msg, err.c_str(), (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; }
        return code;
    };
    const int rc = guarded(&err, [&]() {
        ModelTables m;
        const int built = host_tables(cfg, kappa, kappa16, m, err);
        if (built != HAF_OK) return say(built);
        const std::vector<char> *tab[4] = {&m.svt0, &m.svt0_cr, &m.svt_lr, &m.lr_btiles};
        const bool have = which == 0 ? m.screen_active : which == 1 ? m.screen_active && m.cr_available : m.screen_active && m.lr_available;
        const void *src = tab[which]->data();
        const size_t n = have ? tab[which]->size() : 0;
        *bytes = (long long)n;
        if (out && n && (long long)n <= cap) memcpy(out, src, n);
        else if (out && n) { err = "haf_test_host_sweep_tables: the table is larger than the caller's buffer"; return say(HAF_E_CAPACITY); }
        ints[0] = m.n_sv_tiles; ints[1] = m.sv_tile_neg; ints[2] = m.svm.gv0; ints[3] = m.svm.gv1;
        const double sc[12] = {m.svm.rho, m.svm.guard_acc0, m.svm.guard_acc0_s, m.svm.guard_abs, m.svm.sqrt_cmax, m.crp.B0, m.crp.rho,
                               m.screen.acc_rel, m.screen_cr.acc_rel, m.lr_band.acc6, m.lr_band.acc10, (double)haf::screen_compact_small_words()};
        memcpy(scalars, sc, sizeof sc);
        return (int)HAF_OK;
    });
    return rc == HAF_E_INTERNAL ? say(rc) : rc;
}

// screen_finish (screen_finish.h) with the constants of the same device-free build: form 0 `screen`, 1 `screen_cr` (cr_poly as given),
// as launch_screening hands them to the ten-step feature pass.  sums [n][5]: su2, sd2, sx2, cr, ub -> band [n][8], nax [n].  No device.
int haf_test_host_screen_finish(const haf_config *cfg, double kappa, double kappa16, int form, int cr_poly, const double *sums, int n,
                                float *band, float *nax, char *msg, int msg_cap)
{
    if (!cfg || !cfg->feature_file || !cfg->range_file || !cfg->model_file || form < 0 || form > 1 || !sums || !band || !nax || n < 0) return HAF_E_ARG;
    std::string err;
    auto say = [&](int code) {
        if (msg && msg_cap > 0) { strncpy(msg, err.c_str(), (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; }
        return code;
    };
    const int rc = guarded(&err, [&]() {
        ModelTables m;
        const int built = host_tables(cfg, kappa, kappa16, m, err);
        if (built != HAF_OK) return say(built);
        if (!m.screen_active || (form == 1 && !m.cr_available)) { err = "haf_test_host_screen_finish: the model did not get this form"; return say(HAF_E_ARG); }
        ScreenParams sp = form == 1 ? m.screen_cr : m.screen;
        sp.cr_poly = form == 1 && cr_poly;
        for (int i = 0; i < n; i++) {
            const double *s = sums + (size_t)5 * i;
            screen_finish(s[0], s[1], s[2], s[3], s[4], sp, band + (size_t)kBandFloats * i, nax[i]);
        }
        return (int)HAF_OK;
    });
    return rc == HAF_E_INTERNAL ? say(rc) : rc;
}

// lr_finish_band / lr_finish_band_plain (screen_band.h) on the host with the LrBand of the same device-free build: raw [n][8] as the
// low-rank sweep reads them -> out [n][8]: form 0 the plain epilogue's {gA, gB, gC, cm, corr, abs_c, 0, 0}, 1 / 2 the centred-remainder
// form's {L, c_abs, k_psi, cm, 0, 0, 0, 0} with the exp / the polynomial epilogue.  No device.
int haf_test_lr_finish_band(const haf_config *cfg, double kappa, double kappa16, const float *raw, int n, int form, float *out, char *msg, int msg_cap)
{
    if (!cfg || !cfg->feature_file || !cfg->range_file || !cfg->model_file || form < 0 || form > 2 || !raw || !out || n < 0) return HAF_E_ARG;
    std::string err;
    auto say = [&](int code) {
        if (msg && msg_cap > 0) { strncpy(msg, err.c_str(), (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; }
        return code;
    };
    const int rc = guarded(&err, [&]() {
        ModelTables m;
        const int built = host_tables(cfg, kappa, kappa16, m, err);
        if (built != HAF_OK) return say(built);
        if (!m.screen_active || !m.lr_available || (form == 0 && !m.lr_plain_available)) { err = "haf_test_lr_finish_band: the model did not get this form"; return say(HAF_E_ARG); }
        LrBand lb = m.lr_band;
        lb.poly = form == 2;
        for (int i = 0; i < n; i++) {
            const float *r = raw + (size_t)kBandFloats * i;
            float *o = out + (size_t)kBandFloats * i;
            for (int k = 0; k < kBandFloats; k++) o[k] = 0.0f;
            if (form == 0) {
                float4 g, g2;
                lr_finish_band_plain(r, lb, g, g2);
                o[0] = g.x; o[1] = g.y; o[2] = g.z; o[3] = g.w; o[4] = g2.x; o[5] = g2.y;
            } else {
                lr_finish_band(r, lb, o[0], o[1], o[2], o[3]);
            }
        }
        return (int)HAF_OK;
    });
    return rc == HAF_E_INTERNAL ? say(rc) : rc;
}

// the request sizes launch_features' choice turns on (kernels.h): kSmallEvals, kWaves16Evals, kLargeEvals
int haf_test_feature_thresholds(long long *out3)
{
    if (!out3) return HAF_E_ARG;
    out3[0] = kSmallEvals; out3[1] = kWaves16Evals; out3[2] = kLargeEvals;
    return HAF_OK;
}

// Which feature kernel served the last request's screening pass -- form [3]: the FeatureForm (kernels.h; -1: none ran), the ScreenParams
// set it read (0 `screen`, 1 `screen_cr`, 2 `screen_lrp`; kept only while haf_test_snapshot_screen is on, else -1) and that set's cr_poly -- and, with flags / iiabs given (cap entries each), what
// the pre-stages left per (cloud, roll) of that request for the low-rank form: the flags word (bit 1: the grid holds a negative height)
// and the sum of |height| in units of 2^-20 m.  *n = clouds x rolls of the last request.
int haf_test_feature_form(haf_engine *e, int *form, int *flags, unsigned long long *iiabs, int cap, int *n)
{
    if (!e || !form) return HAF_E_ARG;
    form[0] = e->feature_form; form[1] = e->feature_sp_kind; form[2] = e->feature_sp.cr_poly;
    const int br = e->last.B * e->last.R;
    if (n) *n = br;
    if (!flags && !iiabs) return HAF_OK;
    if (br <= 0 || br > cap) return HAF_E_ARG;
    if (hipDeviceSynchronize() != hipSuccess) return HAF_E_DEVICE;
    if (flags && (!e->d_inexact.p || (size_t)br > e->d_inexact.n ||
                  hipMemcpy(flags, e->d_inexact.p, (size_t)br * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)) return HAF_E_DEVICE;
    if (iiabs && (!e->d_iiabs.p || (size_t)br > e->d_iiabs.n ||
                  hipMemcpy(iiabs, e->d_iiabs.p, (size_t)br * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)) return HAF_E_DEVICE;
    return HAF_OK;
}

// screen_finish (screen_finish.h) on the host, with the very constants the last screening feature pass of this engine was launched with
// (haf_engine::feature_sp).  sums [n][5]: su2, sd2, sx2, cr, ub -> band [n][8], nax [n].
int haf_test_screen_finish(haf_engine *e, const double *sums, int n, float *band, float *nax)
{
    if (!e || e->feature_sp_kind < 0 || !sums || !band || !nax || n < 0) return HAF_E_ARG;
    for (int i = 0; i < n; i++) {
        const double *s = sums + (size_t)5 * i;
        screen_finish(s[0], s[1], s[2], s[3], s[4], e->feature_sp, band + (size_t)kBandFloats * i, nax[i]);
    }
    return HAF_OK;
}

double haf_test_split3(double a, float *parts)
{
    _Float16 h[3];
    const double rep = split3_f16(a, h);
    for (int i = 0; i < 3; i++) parts[i] = (float)h[i];
    return rep;
}

double haf_test_decq4_scr(float v)
{
    static unsigned long long tab[hafq::kScrTabWords];
    static bool init = false;
    if (!init) {
        for (int i = 0; i < hafq::kScrTabWords; i++) tab[i] = hafq::scr_tab_word(i);
        init = true;
    }
    hafq::ScrTabs st;
    st.w = tab;
    return hafq::decq4_float_scr(v, st);
}
// the same for n values at once (a test that needs 10^5 of them)
int haf_test_decq4_scr_n(const float *in, double *out, int n)
{
    if (!in || !out || n < 0) return HAF_E_ARG;
    for (int i = 0; i < n; i++) out[i] = haf_test_decq4_scr(in[i]);
    return HAF_OK;
}

// runs the screening kernel's MFMA chain on host-chosen data (testkernels.hip); a, b: fp16 bit patterns
int haf_test_mfma_accum(const uint16_t *a, const uint16_t *b, const float *c0, float *out, int trials)
{
    void *da = nullptr, *db = nullptr;
    float *dc = nullptr, *dout = nullptr;
    const size_t na = (size_t)trials * 16 * 320 * 2, nc = (size_t)trials * 16 * 4, no = (size_t)trials * 256 * 4;
    if (hipMalloc(&da, na) != hipSuccess || hipMalloc(&db, na) != hipSuccess || hipMalloc((void **)&dc, nc) != hipSuccess ||
        hipMalloc((void **)&dout, no) != hipSuccess) return HAF_E_DEVICE;
    (void)hipMemcpy(da, a, na, hipMemcpyHostToDevice);
    (void)hipMemcpy(db, b, na, hipMemcpyHostToDevice);
    (void)hipMemcpy(dc, c0, nc, hipMemcpyHostToDevice);
    haf::launch_mfma_accum_test(da, db, dc, dout, trials, nullptr);
    const hipError_t rc = hipMemcpy(out, dout, no, hipMemcpyDeviceToHost);
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dc); (void)hipFree(dout);
    return rc == hipSuccess ? HAF_OK : HAF_E_DEVICE;
}

// bare v_mfma_f32_16x16x32_f16 loop on `device` for about `iters` * 0.55 us: executed TFLOP/s by HIP events (bench.py context)
int haf_test_mfma_rate(int device, int iters, double *tflops)      // iters < 0: v_mfma_i32_16x16x64_i8 (TOP/s), else v_mfma_f32_16x16x32_f16
{
    if (!tflops || iters == 0) return HAF_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return HAF_E_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return HAF_E_DEVICE;
    const int blocks = 2 * prop.multiProcessorCount;
    std::vector<uint16_t> h(65536 * 8);
    uint32_t x = 12345u;
    for (auto &v : h) { x = x * 1664525u + 1013904223u; v = (uint16_t)(0x3000u | ((x >> 9) & 0x83FFu)); }   // +-[0.125, 0.25): random mantissas and signs
    void *din = nullptr;
    float *dout = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = HAF_E_DEVICE;
    float ms = 0.0f;
    if (hipMalloc(&din, h.size() * 2) == hipSuccess && hipMalloc((void **)&dout, (size_t)blocks * 256 * 4) == hipSuccess &&
        hipMemcpy(din, h.data(), h.size() * 2, hipMemcpyHostToDevice) == hipSuccess && hipEventCreate(&e0) == hipSuccess &&
        hipEventCreate(&e1) == hipSuccess) {
        haf::launch_mfma_rate_test(din, dout, blocks, iters < 0 ? -64 : 64, nullptr);    // warm the code path
        (void)hipEventRecord(e0, nullptr);
        haf::launch_mfma_rate_test(din, dout, blocks, iters, nullptr);
        (void)hipEventRecord(e1, nullptr);
        if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms > 0.0f) {
            *tflops = (double)blocks * 4.0 * std::abs(iters) * 32.0 * (iters < 0 ? 32768.0 : 16384.0) / (ms * 1e-3) / 1e12;
            rc = HAF_OK;
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(din); (void)hipFree(dout);
    return rc;
}

// timing model of the screening kernel's inner loop with mb = 4 or 8 row blocks per wave (testkernels.hip): executed TFLOP/s
int haf_test_mfma_model(int device, int mb, int tiles, double *tflops)
{
    if (!tflops || tiles < 1 || (mb != 4 && mb != 5 && mb != 8 && mb != 9)) return HAF_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return HAF_E_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return HAF_E_DEVICE;
    const int blocks = (mb >= 5 ? 1 : 2) * prop.multiProcessorCount * 8;          // eight rounds of workgroups
    const int mbe = mb == 9 ? 8 : (mb == 5 ? 8 : mb);                              // (9 = the hand-placed form of 8; 5 = 4 row blocks x 8 waves: same flop per workgroup as 8)
    std::vector<uint16_t> h(65536 * 8);
    uint32_t x = 777u;
    for (auto &v : h) { x = x * 1664525u + 1013904223u; v = (uint16_t)(0x2800u | ((x >> 9) & 0x83FFu)); }
    void *din = nullptr;
    float *dout = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = HAF_E_DEVICE;
    float ms = 0.0f;
    // (out holds one float per thread of the widest form: 512 threads per workgroup)
    if (hipMalloc(&din, h.size() * 2) == hipSuccess && hipMalloc((void **)&dout, (size_t)blocks * 512 * 4) == hipSuccess &&
        hipMemcpy(din, h.data(), h.size() * 2, hipMemcpyHostToDevice) == hipSuccess && hipEventCreate(&e0) == hipSuccess &&
        hipEventCreate(&e1) == hipSuccess) {
        haf::launch_mfma_model_test(din, dout, mb, blocks, 2, nullptr);
        (void)hipEventRecord(e0, nullptr);
        haf::launch_mfma_model_test(din, dout, mb, blocks, tiles, nullptr);
        (void)hipEventRecord(e1, nullptr);
        if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms > 0.0f) {
            *tflops = (double)blocks * 4.0 * tiles * 20.0 * mbe * 16384.0 / (ms * 1e-3) / 1e12;
            rc = HAF_OK;
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(din); (void)hipFree(dout);
    return rc;
}

// v_mfma_i32_16x16x64_i8 on host-chosen int8 data: a [16][64], b [64][16] row-major -> c [16][16] (testkernels.hip)
int haf_test_i8_mfma(const signed char *a, const signed char *b, int *c)
{
    void *da = nullptr, *db = nullptr;
    int *dc = nullptr;
    if (hipMalloc(&da, 1024) != hipSuccess || hipMalloc(&db, 1024) != hipSuccess || hipMalloc((void **)&dc, 1024) != hipSuccess) return HAF_E_DEVICE;
    (void)hipMemcpy(da, a, 1024, hipMemcpyHostToDevice);
    (void)hipMemcpy(db, b, 1024, hipMemcpyHostToDevice);
    haf::launch_i8_layout_probe(da, db, dc, nullptr);
    const hipError_t rc = hipMemcpy(c, dc, 1024, hipMemcpyDeviceToHost);
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dc);
    return rc == hipSuccess ? HAF_OK : HAF_E_DEVICE;
}

// which form of the screening pass serves the model, whether the pass is on, and the undecided shares calibrate() saw per form
int haf_test_screen_state(haf_engine *e, int *variant, int *active, double *shares /* [4] */)
{
    if (!e) return HAF_E_ARG;
    if (variant) *variant = e->screen_variant | (e->use_t0b ? 16 : 0) | (e->t1_skip ? 32 : 0) | (e->last.lr ? 64 : 0);
    if (active) *active = e->screen_active ? 1 : 0;
    if (shares) for (int i = 0; i < SCREEN_VARIANTS; i++) shares[i] = e->variant_share[i];
    return HAF_OK;
}

// plan_tiers over `rows` sets of facts, each given as 23 integers (TierFacts in declaration order) -> each plan as 24 integers
// (TierPlan in declaration order, booleans as 0 / 1); n_facts / n_plan: the row widths the caller assumes.  No device.
int haf_test_tier_plan(const long long *facts, int n_facts, int *plan, int n_plan, int rows)
{
    if (!facts || !plan || n_facts != 23 || n_plan != 24 || rows < 0) return HAF_E_ARG;
    for (int r = 0; r < rows; r++) {
        const long long *x = facts + (size_t)r * 23;
        TierFacts f;
        f.screen_variant = (int)*x++;
        for (bool *b : {&f.cr_available, &f.lr_available, &f.lr_enabled, &f.lr_plain_available, &f.lr_fused, &f.use_t0b, &f.t1_skip,
                        &f.t1_cr_available, &f.i8_active, &f.calibrated, &f.short_gate, &f.generic_kernel}) *b = *x++ != 0;
        f.n_sv = (int)*x++;
        f.t0b_no_gather = *x++ != 0;
        f.mode = (int)*x++;
        for (bool *b : {&f.reuse_operands, &f.direct, &f.small_exact, &f.large, &f.fused_pre}) *b = *x++ != 0;
        f.hw = (long)*x++;
        f.evals_cap = (long)*x++;
        const TierPlan p = plan_tiers(f);
        const int out[24] = {p.path, p.sp, p.cr, p.lr, p.reuse, p.pass0_out, p.t0b, p.t0b_in, p.t0b_out, p.gate, p.gate_in, p.gate_out,
                             p.t1, p.t1cr, p.t1_in, p.t1_cnt, p.t1_out, p.i8, p.i8_in, p.i8_out, p.fp64, p.fp64_in, p.fp64_out, p.strict_in};
        memcpy(plan + (size_t)r * 24, out, sizeof out);
    }
    return HAF_OK;
}

// switches the screening pass off as the adaptive rule would after a request that every form of the pass failed on (tests of the
// periodic re-try)
int haf_test_set_screen_inactive(haf_engine *e)
{
    if (!e) return HAF_E_ARG;
    e->screen_active = false;
    e->inactive_calls = 0;
    return HAF_OK;
}

// the engine's matrix-core rounding constant: what the probe measured and what the bands use
int haf_test_mfma_kappa(haf_engine *e, double *measured, double *used)      // [0]: 16x16x32, [1]: 16x16x16
{
    if (!e) return HAF_E_ARG;
    measured[0] = e->mfma_kappa_measured; used[0] = e->mfma_kappa;
    measured[1] = e->mfma_kappa16_measured; used[1] = e->mfma_kappa16;
    return HAF_OK;
}

// v_mfma_f32_16x16x32_f16 on host-chosen data (testkernels.hip: k_f16_mfma_probe)
int haf_test_f16_mfma(const unsigned short *a, const unsigned short *b, const float *c, float *d, int trials, int chain)
{
    void *da = nullptr, *db = nullptr;
    float *dc = nullptr, *dd = nullptr;
    const size_t na = (size_t)trials * 1024, nc = (size_t)trials * 1024;
    if (hipMalloc(&da, na) != hipSuccess || hipMalloc(&db, na) != hipSuccess || hipMalloc((void **)&dc, nc) != hipSuccess ||
        hipMalloc((void **)&dd, nc) != hipSuccess) return HAF_E_DEVICE;
    (void)hipMemcpy(da, a, na, hipMemcpyHostToDevice);
    (void)hipMemcpy(db, b, na, hipMemcpyHostToDevice);
    (void)hipMemcpy(dc, c, nc, hipMemcpyHostToDevice);
    haf::launch_f16_mfma_probe(da, db, dc, dd, trials, chain, nullptr);
    const hipError_t rc = hipMemcpy(d, dd, nc, hipMemcpyDeviceToHost);
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dc); (void)hipFree(dd);
    return rc == hipSuccess ? HAF_OK : HAF_E_DEVICE;
}

int haf_test_decq_device(const double *in, double *out, int n, int digits)
{
    double *di = nullptr, *dout = nullptr;
    if (hipMalloc((void **)&di, (size_t)n * 8) != hipSuccess || hipMalloc((void **)&dout, (size_t)n * 8) != hipSuccess) return HAF_E_DEVICE;
    (void)hipMemcpy(di, in, (size_t)n * 8, hipMemcpyHostToDevice);
    launch_decq_test(di, dout, n, digits, nullptr);
    hipError_t rc = hipMemcpy(out, dout, (size_t)n * 8, hipMemcpyDeviceToHost);
    (void)hipFree(di); (void)hipFree(dout);
    return rc == hipSuccess ? HAF_OK : HAF_E_DEVICE;
}

int haf_test_scale_device(const double *q4, const double *fmin, const double *fmax, double lower, double upper, double *out, int n)
{
    double *d[4] = {nullptr, nullptr, nullptr, nullptr};
    for (auto &p : d) if (hipMalloc((void **)&p, (size_t)n * 8) != hipSuccess) return HAF_E_DEVICE;
    (void)hipMemcpy(d[0], q4, (size_t)n * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(d[1], fmin, (size_t)n * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(d[2], fmax, (size_t)n * 8, hipMemcpyHostToDevice);
    launch_scale_test(d[0], d[1], d[2], lower, upper, d[3], n, nullptr);
    hipError_t rc = hipMemcpy(out, d[3], (size_t)n * 8, hipMemcpyDeviceToHost);
    for (auto &p : d) (void)hipFree(p);
    return rc == hipSuccess ? HAF_OK : HAF_E_DEVICE;
}

}  // extern "C"
