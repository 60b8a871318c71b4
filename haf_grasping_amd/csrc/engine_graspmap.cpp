// engine_graspmap.cpp -- haf_grasp_map, haf_cell_pose, haf_grasp_map_best and haf_grasp_map_labels: the votes of the last scored batch in the pixels of a
// sensor frame (include/hafgrasp.h).  The device pass (graspmap.hip) reads the vote grids that batch left on the device and, for
// haf_cell_pose, its height grids and records; nothing here writes to any of them, to the request's input block or to the raw areas
// of haf_score_frames / haf_score_views: the frame's pixels, the roll transforms, the images and the mask live in the call's block
// (call_io, the one every call outside the request path shares), laid out here as [best key + cell record: 64 bytes][R x CellGeo]
// [vote | roll | cell images][mask bytes][a host frame's pixels][a host label image][label table: keys, counts][label output entries].
// The roll transforms are recomputed from the inputs the batch was scored with (LastCall::inputs) through
// fill_roll_geo: the header of the request's input block may have been overwritten since.  Built with -ffp-contract=off.
#include "engine_state.h"

namespace haf_host {

using haf_cell_math::CellGeo;

namespace {

constexpr size_t kMapHdr = 64;            // [0] the best key of k_map_best, [16] the record of k_cell_record
constexpr size_t kMapRecOff = 16;

struct MapLayout {
    size_t geo = 0, vote = 0, roll = 0, cell = 0, mask = 0, raw = 0, labels = 0, ltab = 0, lout = 0, total = 0;
};

// the block for images of n_img pixels, a mask of n_mask bytes and raw_bytes of a staged host frame's pixels (each may be 0); for
// haf_grasp_map_labels also label_bytes of a staged host label image and, per label, the table's key and count and the output entry
MapLayout map_layout(const haf_engine *e, size_t n_img, size_t n_mask, size_t raw_bytes, size_t label_bytes = 0, size_t n_labels = 0)
{
    MapLayout l;
    l.geo = kMapHdr;
    l.vote = l.geo + (size_t)std::max(1, e->max_rolls) * sizeof(CellGeo);
    l.roll = l.vote + up16(n_img * 2);
    l.cell = l.roll + up16(n_img * 2);
    l.mask = l.cell + up16(n_img * 4);
    l.raw = l.mask + up16(n_mask);
    l.labels = l.raw + up16(raw_bytes);
    l.ltab = l.labels + up16(label_bytes);
    l.lout = l.ltab + up16(n_labels * 12);                  // [n_labels] 64-bit keys, then [n_labels] counts
    l.total = l.lout + up16(n_labels * sizeof(LabelOutDev));
    return l;
}

// what every entry point here asks of the last batch; *rolls = the rolls that ran for the request (0: its budget was negative)
int check_last(haf_engine *e, const char *who, int32_t request, int *rolls)
{
    const std::string name(who);
    if (e->mdl.prob_mode) return fail(e, HAF_E_ARG, name + ": not available with HAF_FLAG_PROBABILITY (fp32 votes)");
    const LastCall &last = e->last;
    if (last.B < 1 || last.R < 1 || (int)last.inputs.size() < last.B) return fail(e, HAF_E_ARG, name + ": no scored batch");
    if (request < 0 || request >= last.B) return fail(e, HAF_E_ARG, name + ": request not in the last scored batch");
    *rolls = (int)last.inputs[(size_t)request].max_calculation_time < 0 ? 0 : last.R;      // the reference scores none of its rolls
    return HAF_OK;
}

int check_map_frame(haf_engine *e, const char *who, const haf_frame *f)
{
    const std::string name(who);
    if (!f) return fail(e, HAF_E_ARG, name + ": null frame");
    const FrameBatch chk = check_frame_batch(f, 1, nullptr, e->cfg.max_points);
    if (chk.code != HAF_OK) return fail(e, chk.code, name + ": " + (chk.text.empty() ? "more pixels than max_points" : chk.text));
    return HAF_OK;
}

// What every device pass over one checked frame starts with: the zeroed header and the roll transforms go up, a host frame's pixels are
// staged (upload_frame, engine_stage.cpp); *fd = the frame as the kernels read it.  No synchronisation.
int stage_map(haf_engine *e, const CallBuffers &cb, int request, int rolls, const haf_frame &f, const MapLayout &l, FrameDev *fd_out)
{
    const LastCall &last = e->last;
    memset(cb.host, 0, kMapHdr);
    fill_cell_geo(e->cfg, last.inputs[(size_t)request], last.roll_first, rolls, reinterpret_cast<CellGeo *>(cb.host + l.geo));
    HIPCHK(e, hipMemcpyAsync(cb.dev, cb.host, l.geo + (size_t)rolls * sizeof(CellGeo), hipMemcpyHostToDevice, cb.stream));
    *fd_out = describe_frame(f, cb.dev + l.raw);
    return f.on_device == 1 ? HAF_OK : upload_frame(e, f, cb.host + l.raw, cb.dev + l.raw, cb.stream);
}

// stage_map, then k_grasp_map on the engine's stream.  d_vote / d_roll / d_cell: where the images go (null: not wanted).  No synchronisation.
int launch_map(haf_engine *e, const CallBuffers &cb, int request, int rolls, const haf_frame &f, const MapLayout &l, short *d_vote, short *d_roll,
               int *d_cell)
{
    const haf_config &c = e->cfg;
    const LastCall &last = e->last;
    FrameDev fd;
    int rc;
    if ((rc = stage_map(e, cb, request, rolls, f, l, &fd)) != HAF_OK) return rc;
    const int H = c.grid_h, W = c.grid_w;
    float r_row, r_col;
    haf_pick_math::cell_reach(H, W, &r_row, &r_col);
    const short *ev = e->d_ev16.p + (size_t)request * last.R * (size_t)H * W;
    launch_grasp_map(fd, reinterpret_cast<const CellGeo *>(cb.dev + l.geo), rolls, last.roll_first, ev, H, W, r_row, r_col, d_vote, d_roll, d_cell,
                     cb.stream);
    HIPCHK(e, hipGetLastError());
    return HAF_OK;
}

int grasp_map_impl(haf_engine *e, int32_t request, const haf_frame *f, int16_t *vote, int16_t *roll, int32_t *cell, int32_t out_on_device)
{
    int rolls = 0, rc;
    if ((rc = check_last(e, "haf_grasp_map", request, &rolls)) != HAF_OK) return rc;
    if (out_on_device != 0 && out_on_device != 1) return fail(e, HAF_E_ARG, "haf_grasp_map: out_on_device must be 0 (host) or 1 (device)");
    if ((rc = check_map_frame(e, "haf_grasp_map", f)) != HAF_OK) return rc;
    const size_t n = (size_t)f->width * (size_t)f->height;
    // (device outputs: the images are the caller's, the block only holds the header, the transforms and a host frame's pixels)
    const MapLayout use = map_layout(e, out_on_device ? 0 : n, 0, f->on_device == 1 ? 0 : n * frame_pixel_bytes(f->kind));
    CallBuffers cb;
    if ((rc = call_buffers(e, "haf_grasp_map: ", use.total, "the map block", 0, nullptr, &cb)) != HAF_OK) return rc;
    char *d = cb.dev;
    short *dv = !vote ? nullptr : out_on_device ? vote : reinterpret_cast<short *>(d + use.vote);
    short *dr = !roll ? nullptr : out_on_device ? roll : reinterpret_cast<short *>(d + use.roll);
    int *dc = !cell ? nullptr : out_on_device ? cell : reinterpret_cast<int *>(d + use.cell);
    if ((rc = launch_map(e, cb, request, rolls, *f, use, dv, dr, dc)) != HAF_OK) return rc;
    // (host outputs: three images, three copies; the last one is call_finish's)
    const bool back = !out_on_device;
    if (back && vote) HIPCHK(e, hipMemcpyAsync(cb.host + use.vote, d + use.vote, n * 2, hipMemcpyDeviceToHost, cb.stream));
    if (back && roll) HIPCHK(e, hipMemcpyAsync(cb.host + use.roll, d + use.roll, n * 2, hipMemcpyDeviceToHost, cb.stream));
    if ((rc = call_finish(e, cb, back && cell ? n * 4 : 0, use.cell)) != HAF_OK) return rc;
    if (back && vote) memcpy(vote, cb.host + use.vote, n * 2);
    if (back && roll) memcpy(roll, cb.host + use.roll, n * 2);
    if (back && cell) memcpy(cell, cb.host + use.cell, n * 4);
    return HAF_OK;
}

}  // namespace

// a cell's record as a candidate: haf_top_grasps' pose of it, run_length 0 (a cell is not a run)
static int record_candidate(haf_engine *e, int request, int roll, const RollRecordDev &q, haf_grasp_candidate *out)
{
    haf_roll_record rec;
    rec.vote = q.vote; rec.row = q.row; rec.col = q.col; rec.h_locmax = q.h_locmax; rec.n_evals = q.n_evals;
    haf_grasp_candidate cand;
    memset(&cand, 0, sizeof cand);
    const int rc = candidate_pose_impl(e->cfg, &e->last.inputs[(size_t)request], rec, roll, &cand.grasp, e->error);
    if (rc != HAF_OK) return rc;
    cand.run_length = 0;
    cand.h_locmax = rec.h_locmax;
    *out = cand;
    return HAF_OK;
}

int hand_over_picks(haf_engine *e, const std::string &who, const LabelOutDev *got, int32_t n, const std::function<int(int32_t)> &request_of,
                    const std::function<int32_t(int32_t)> &id_of, int32_t width, haf_label_pick *picks, haf_grasp_candidate *poses,
                    int32_t *order, int32_t *n_found)
{
    const int cells = e->cfg.grid_h * e->cfg.grid_w;
    // every entry is checked before the first one is handed over
    for (int32_t k = 0; k < n; k++) {
        const LabelOutDev &o = got[k];
        if (!o.found) continue;
        if (o.cell < 0 || o.cell >= cells || o.n_pixels < 1) return fail(e, HAF_E_INTERNAL, who + "malformed key");
        if (o.rec.vote != o.vote) return fail(e, HAF_E_INTERNAL, who + "the record's vote is not the key's");
    }
    for (int32_t k = 0; k < n; k++) {
        const LabelOutDev &o = got[k];
        if (!o.found) continue;
        haf_label_pick &p = picks[k];
        p.found = 1; p.u = o.u; p.v = o.v; p.vote = o.vote; p.roll = o.roll; p.cell = o.cell; p.n_pixels = o.n_pixels;
        int rc;
        if (poses && (rc = record_candidate(e, request_of(k), o.roll, o.rec, &poses[k])) != HAF_OK) return rc;
    }
    label_order(picks, n, id_of, width, order, n_found);
    return HAF_OK;
}

namespace {

int cell_pose_checked(haf_engine *e, int request, int roll, int row, int col, haf_grasp_candidate *out)
{
    const haf_config &c = e->cfg;
    const LastCall &last = e->last;
    int rc;
    CallBuffers cb;                                         // (inside haf_grasp_map_best: the block is there and larger, nothing moves)
    if ((rc = call_buffers(e, "haf_cell_pose: ", kMapHdr, "the record's block", 0, nullptr, &cb)) != HAF_OK) return rc;
    const int br = request * last.R + (roll - last.roll_first);
    RollRecordDev *d_rec = reinterpret_cast<RollRecordDev *>(cb.dev + kMapRecOff);
    launch_cell_record(e->d_ev16.p, reinterpret_cast<const float *>(e->d_heights.p), e->d_rec.p, br, row, col, c.grid_h, c.grid_w, d_rec, cb.stream);
    if ((rc = call_finish(e, cb, sizeof(RollRecordDev), kMapRecOff)) != HAF_OK) return rc;
    RollRecordDev q;
    memcpy(&q, cb.host + kMapRecOff, sizeof q);
    return record_candidate(e, request, roll, q, out);
}

int cell_pose_impl(haf_engine *e, int32_t request, int32_t roll, int32_t row, int32_t col, haf_grasp_candidate *out)
{
    int rolls = 0, rc;
    if (!out) return fail(e, HAF_E_ARG, "haf_cell_pose: null argument");
    if ((rc = check_last(e, "haf_cell_pose", request, &rolls)) != HAF_OK) return rc;
    if (rolls == 0) return fail(e, HAF_E_ARG, "haf_cell_pose: no roll ran for this request (negative budget)");
    if (roll < e->last.roll_first || roll >= e->last.roll_first + e->last.R) return fail(e, HAF_E_ARG, "haf_cell_pose: roll not in the last scored batch");
    if (row < 0 || row >= e->cfg.grid_h || col < 0 || col >= e->cfg.grid_w) return fail(e, HAF_E_ARG, "haf_cell_pose: cell outside the grid");
    return cell_pose_checked(e, request, roll, row, col, out);
}

int map_best_impl(haf_engine *e, int32_t request, const haf_frame *f, const uint8_t *mask, size_t mask_row_stride, int32_t min_vote,
                  haf_grasp_candidate *out, int32_t *u, int32_t *v, int32_t *found)
{
    int rolls = 0, rc;
    if (!out || !found) return fail(e, HAF_E_ARG, "haf_grasp_map_best: null argument");
    if ((rc = check_last(e, "haf_grasp_map_best", request, &rolls)) != HAF_OK) return rc;
    if ((rc = check_map_frame(e, "haf_grasp_map_best", f)) != HAF_OK) return rc;
    if (mask && mask_row_stride < (size_t)f->width) return fail(e, HAF_E_ARG, "haf_grasp_map_best: mask_row_stride smaller than a row");
    const size_t n = (size_t)f->width * (size_t)f->height;
    const MapLayout l = map_layout(e, n, mask ? n : 0, f->on_device == 1 ? 0 : n * frame_pixel_bytes(f->kind));
    CallBuffers cb;
    if ((rc = call_buffers(e, "haf_grasp_map_best: ", l.total, "the map block", 0, nullptr, &cb)) != HAF_OK) return rc;
    char *d = cb.dev;
    short *dv = reinterpret_cast<short *>(d + l.vote), *dr = reinterpret_cast<short *>(d + l.roll);
    int *dc = reinterpret_cast<int *>(d + l.cell);
    if ((rc = launch_map(e, cb, request, rolls, *f, l, dv, dr, dc)) != HAF_OK) return rc;
    ImageDev md;                                            // (a host mask; k_map_best reads it packed)
    if ((rc = upload_image(e, *f, mask, 0, mask_row_stride, 1, cb, l.mask, &md)) != HAF_OK) return rc;
    unsigned long long *d_key = reinterpret_cast<unsigned long long *>(d);      // (zeroed by launch_map's header copy)
    launch_map_best(dv, dr, static_cast<const unsigned char *>(md.src), (unsigned)n, min_vote, d_key, cb.stream);
    if ((rc = call_finish(e, cb, 8)) != HAF_OK) return rc;
    unsigned long long key;
    memcpy(&key, cb.host, 8);
    if (key == 0ull) { *found = 0; return HAF_OK; }
    const size_t i = (size_t)haf_pick_math::pick_key_pixel(key);
    const int roll = haf_pick_math::pick_key_roll(key);
    if (i >= n || roll < e->last.roll_first || roll >= e->last.roll_first + e->last.R) return fail(e, HAF_E_INTERNAL, "haf_grasp_map_best: malformed key");
    int32_t ci = -1;
    HIPCHK(e, hipMemcpyAsync(cb.host + 8, dc + i, 4, hipMemcpyDeviceToHost, cb.stream));      // (the best pixel's cell: a second, 4-byte round trip)
    HIPCHK(e, hipStreamSynchronize(cb.stream));
    memcpy(&ci, cb.host + 8, 4);
    const int W = e->cfg.grid_w;
    if (ci < 0 || ci >= e->cfg.grid_h * W) return fail(e, HAF_E_INTERNAL, "haf_grasp_map_best: malformed cell");
    haf_grasp_candidate cand;
    if ((rc = cell_pose_checked(e, request, roll, ci / W, ci % W, &cand)) != HAF_OK) return rc;
    *out = cand;
    if (u) *u = (int32_t)(i % (size_t)f->width);
    if (v) *v = (int32_t)(i / (size_t)f->width);
    *found = 1;
    return HAF_OK;
}

// haf_grasp_map_labels: k_map_labels over the frame, k_label_records over the labels, ONE copy back and ONE synchronisation
int map_labels_impl(haf_engine *e, int32_t request, const haf_frame *f, const haf_label_image *labels, int32_t n_labels, int32_t min_vote,
                    haf_label_pick *picks, haf_grasp_candidate *poses, int32_t *order, int32_t *n_found)
{
    int rolls = 0, rc;
    if ((rc = check_last(e, "haf_grasp_map_labels", request, &rolls)) != HAF_OK) return rc;
    if ((rc = check_map_frame(e, "haf_grasp_map_labels", f)) != HAF_OK) return rc;
    std::string why;
    if (!picks || check_label_image(labels, f->width, n_labels, why) != HAF_OK) return fail(e, HAF_E_ARG, "haf_grasp_map_labels: " + (picks ? why : "null picks"));
    const haf_config &c = e->cfg;
    const LastCall &last = e->last;
    for (int32_t l = 0; l < n_labels; l++) label_pick_none(&picks[l]);
    if (poses) memset(poses, 0, (size_t)n_labels * sizeof *poses);
    if (n_found) *n_found = 0;
    if (rolls == 0) return HAF_OK;                          // (a negative budget: no roll ran, no pixel has a roll)
    const size_t n = (size_t)f->width * (size_t)f->height, eb = (size_t)labels->elem_bytes, nl = (size_t)n_labels;
    const MapLayout l = map_layout(e, 0, 0, f->on_device == 1 ? 0 : n * frame_pixel_bytes(f->kind), labels->on_device != 1 ? n * eb : 0, nl);
    CallBuffers cb;
    if ((rc = call_buffers(e, "haf_grasp_map_labels: ", l.total, "the map block", 0, nullptr, &cb)) != HAF_OK) return rc;
    char *d = cb.dev;
    const hipStream_t s = cb.stream;
    FrameDev fd;
    if ((rc = stage_map(e, cb, request, rolls, *f, l, &fd)) != HAF_OK) return rc;
    ImageDev ld;
    if ((rc = upload_image(e, *f, labels->data, labels->on_device, labels->row_stride_bytes, eb, cb, l.labels, &ld)) != HAF_OK) return rc;
    unsigned long long *d_key = reinterpret_cast<unsigned long long *>(d + l.ltab);
    unsigned *d_cnt = reinterpret_cast<unsigned *>(d + l.ltab + nl * 8);
    LabelOutDev *d_out = reinterpret_cast<LabelOutDev *>(d + l.lout);
    HIPCHK(e, hipMemsetAsync(d + l.ltab, 0, nl * 12, s));
    const int H = c.grid_h, W = c.grid_w;
    const size_t HW = (size_t)H * W, br0 = (size_t)request * last.R;
    float r_row, r_col;
    haf_pick_math::cell_reach(H, W, &r_row, &r_col);
    const CellGeo *d_geo = reinterpret_cast<const CellGeo *>(d + l.geo);
    const short *ev = e->d_ev16.p + br0 * HW;
    launch_map_labels(fd, d_geo, rolls, last.roll_first, ev, H, W, r_row, r_col, ld.src, (size_t)ld.row_stride, (int)eb, n_labels, min_vote, d_key, d_cnt, s);
    HIPCHK(e, hipGetLastError());
    launch_label_records(fd, d_geo, rolls, last.roll_first, ev, reinterpret_cast<const float *>(e->d_heights.p) + br0 * HW, e->d_rec.p + br0, H, W,
                         r_row, r_col, n_labels, d_key, d_cnt, d_out, s);
    if ((rc = call_finish(e, cb, nl * sizeof(LabelOutDev), l.lout)) != HAF_OK) return rc;
    return hand_over_picks(e, "haf_grasp_map_labels: ", reinterpret_cast<const LabelOutDev *>(cb.host + l.lout), n_labels,
                           [&](int32_t) { return (int)request; }, [](int32_t k) { return k + 1; }, f->width, picks, poses, order, n_found);
}

}  // namespace

}  // namespace haf_host

extern "C" {

int haf_grasp_map(haf_engine *e, int32_t request, const haf_frame *frame, int16_t *vote, int16_t *roll, int32_t *cell, int32_t out_on_device)
{
    if (!e) return HAF_E_ARG;
    return guarded(&e->error, [&] { return grasp_map_impl(e, request, frame, vote, roll, cell, out_on_device); });
}

int haf_cell_pose(haf_engine *e, int32_t request, int32_t roll, int32_t row, int32_t col, haf_grasp_candidate *out)
{
    if (!e) return HAF_E_ARG;
    return guarded(&e->error, [&] { return cell_pose_impl(e, request, roll, row, col, out); });
}

int haf_grasp_map_best(haf_engine *e, int32_t request, const haf_frame *frame, const uint8_t *mask, size_t mask_row_stride, int32_t min_vote,
                       haf_grasp_candidate *out, int32_t *u, int32_t *v, int32_t *found)
{
    if (!e) return HAF_E_ARG;
    return guarded(&e->error, [&] { return map_best_impl(e, request, frame, mask, mask_row_stride, min_vote, out, u, v, found); });
}

int haf_grasp_map_labels(haf_engine *e, int32_t request, const haf_frame *frame, const haf_label_image *labels, int32_t n_labels,
                         int32_t min_vote, haf_label_pick *picks, haf_grasp_candidate *poses, int32_t *order, int32_t *n_found)
{
    if (!e) return HAF_E_ARG;
    return guarded(&e->error, [&] { return map_labels_impl(e, request, frame, labels, n_labels, min_vote, picks, poses, order, n_found); });
}

}  // extern "C"
