// engine_objects.cpp -- haf_score_objects (include/hafgrasp.h): every listed object of an instance-label image as an ROI request of its own
// on ONE shared frame, and every object's pick from its own request, in one call.  The definition is a composition of calls that exist
// (haf_score_frames_roi under the mask `labels == the object's label`, then that label's entry of haf_grasp_map_labels); what this unit
// adds is doing once what the composition repeats per object:
//   * the frame is checked, packed, uploaded and deprojected once: the request path (engine_request.cpp) runs k_frame_points for one
//     FrameDev and lets every CloudDev of the batch point at that one set of points (FrameSource::objects);
//   * the label image goes up once, into the call's block, and serves both passes; a device-resident one is read where it lies;
//   * ONE launch of k_roi_mark_objects marks the cell sets of all requests, where the composition has a mask upload and a launch each;
//   * ONE launch pair (k_map_labels_objects, k_object_records), one copy back and one synchronisation give every object's pick, behind
//     the request path's own copy back and wait.
// Every refusal comes before the first stream operation and before any buffer is touched.  The call's block (call_io, the one every call
// outside the request path shares; this call HOLDS it across the request path, which therefore never asks for it: call_buffers) is laid
// out here as [64 bytes unused][B * R x CellGeo][label -> request, for the cell sets][label -> request, for the picks][B keys][B counts]
// [B x LabelOutDev][a host label image]: everything up to the keys goes up with one copy.  Built with -ffp-contract=off.
#include "engine_state.h"

namespace haf_host {

using haf_cell_math::CellGeo;

namespace {

struct ObjLayout {
    size_t geo = 64, mark = 0, pick = 0, keys = 0, cnt = 0, out = 0, labels = 0, total = 0;
};

ObjLayout obj_layout(size_t B, size_t R, size_t n_labels, size_t label_bytes)
{
    ObjLayout l;
    l.mark = l.geo + up16(B * R * sizeof(CellGeo));
    l.pick = l.mark + up16(n_labels * sizeof(int));
    l.keys = l.pick + up16(n_labels * sizeof(int));
    l.cnt = l.keys + up16(B * 8);
    l.out = l.cnt + up16(B * 4);
    l.labels = l.out + up16(B * sizeof(LabelOutDev));
    l.total = l.labels + up16(label_bytes);
    return l;
}

// the pixels of every listed object in a HOST label image (classify_request: the bound a host mask gives an ROI request)
void count_object_pixels(const haf_label_image &img, int width, int height, int n_labels, const std::vector<int> &req_of_label, std::vector<long> &masked)
{
    const char *base = static_cast<const char *>(img.data);
    for (int v = 0; v < height; v++) {
        const char *row = base + (size_t)v * img.row_stride_bytes;
        for (int u = 0; u < width; u++) {
            unsigned lab;
            if (img.elem_bytes == 1) lab = (unsigned char)row[u];
            else { uint16_t w; memcpy(&w, row + (size_t)u * 2, 2); lab = w; }
            if (lab < 1u || lab > (unsigned)n_labels) continue;
            const int b = req_of_label[lab - 1u];
            if (b >= 0) masked[(size_t)b]++;
        }
    }
}

}  // namespace

int objects_mark_cells(haf_engine *e, const ObjectsCall &oc, const haf_frame &frame, const CloudDev *h_clouds, const RollGeo *d_geo, const Dims &d,
                       float r_row, float r_col, hipStream_t s)
{
    const size_t grid_words = (size_t)d.H * (size_t)roi_row_words(d.W);
    HIPCHK(e, hipMemsetAsync(e->d_roi_cells.p, 0, (size_t)d.B * d.R * grid_words * sizeof(unsigned long long), s));
    launch_roi_mark_objects(oc.d_labels, oc.label_stride, oc.label_bytes, frame.width, frame.width * frame.height, h_clouds[0].xyz,
                            oc.d_req_of_label, oc.n_labels, d_geo, d.R, e->d_roi_cells.p, d.H, d.W, r_row, r_col, s);
    HIPCHK(e, hipGetLastError());
    return HAF_OK;
}

int score_objects_impl(haf_engine *e, const haf_frame *frame, const haf_label_image *labels, int32_t n_labels, int32_t n_objects,
                       const int32_t *object_labels, const haf_grasp_input *in, int32_t min_vote, haf_grasp_output *out, haf_label_pick *picks,
                       haf_grasp_candidate *poses, int32_t *order, int32_t *n_found)
{
    if (!e) return HAF_E_ARG;
    const std::string who = "haf_score_objects: ";
    if (!frame || !object_labels || !in || !out || n_objects < 1) return fail(e, HAF_E_ARG, who + "null or empty argument");
    if (e->mdl.prob_mode) return fail(e, HAF_E_ARG, who + "not available with HAF_FLAG_PROBABILITY");
    if (n_objects > e->cfg.max_clouds) return fail(e, HAF_E_CAPACITY, who + "more objects than max_clouds");
    if (e->cfg.n_rolls > e->max_rolls) return fail(e, HAF_E_CAPACITY, who + "more rolls in one call than max_rolls_per_call");
    // the frame counts ONCE against max_points, whatever n_objects is
    const FrameBatch chk = check_frame_batch(frame, 1, nullptr, e->cfg.max_points);
    if (chk.code != HAF_OK) return fail(e, chk.code, who + (chk.text.empty() ? "more pixels than max_points" : chk.text));
    std::string why;
    int rc;
    if (!picks || check_label_image(labels, frame->width, n_labels, why) != HAF_OK) return fail(e, HAF_E_ARG, who + (picks ? why : "null picks"));
    const int B = n_objects, R = e->cfg.n_rolls;
    std::vector<int> mark((size_t)n_labels, -1);
    for (int b = 0; b < B; b++) {
        const int32_t l = object_labels[b];
        if (l < 1 || l > n_labels) return fail(e, HAF_E_ARG, who + "object " + std::to_string(b) + ": label outside 1..n_labels");
        if (mark[(size_t)l - 1] >= 0) return fail(e, HAF_E_ARG, who + "object " + std::to_string(b) + ": its label is listed twice");
        mark[(size_t)l - 1] = b;
    }
    const haf_config &c = e->cfg;
    const size_t n = (size_t)frame->width * (size_t)frame->height, eb = (size_t)labels->elem_bytes;
    const bool host_labels = labels->on_device != 1;
    const ObjLayout l = obj_layout((size_t)B, (size_t)R, (size_t)n_labels, host_labels ? n * eb : 0);
    if ((rc = ensure_roi_buffers(e, who)) != HAF_OK) return rc;
    CallBuffers cb;
    if ((rc = call_buffers(e, who, l.total, "the call's block", 0, nullptr, &cb)) != HAF_OK) return rc;

    for (int b = 0; b < B; b++) label_pick_none(&picks[b]);
    if (poses) memset(poses, 0, (size_t)B * sizeof *poses);
    if (n_found) *n_found = 0;
    // a request whose budget is negative runs no roll (server.cpp:367-374): its object marks its cells like any other, and has no pick
    std::vector<int> pick(mark);
    bool any_runs = false;
    for (int b = 0; b < B; b++) {
        if ((int)in[b].max_calculation_time < 0) pick[(size_t)object_labels[b] - 1] = -1;
        else any_runs = true;
    }
    RoiCall call;
    call.masked.assign((size_t)B, host_labels ? 0 : -1);
    ObjectsCall oc;
    const hipStream_t s = cb.stream;
    char *d = cb.dev;
    if (any_runs) {                                       // (a batch whose every budget is negative runs nothing on the device)
        if (host_labels) count_object_pixels(*labels, frame->width, frame->height, n_labels, mark, call.masked);
        for (int b = 0; b < B; b++) fill_cell_geo(c, in[b], 0, R, reinterpret_cast<CellGeo *>(cb.host + l.geo) + (size_t)b * R);
        memcpy(cb.host + l.mark, mark.data(), (size_t)n_labels * sizeof(int));
        memcpy(cb.host + l.pick, pick.data(), (size_t)n_labels * sizeof(int));
        HIPCHK(e, hipMemcpyAsync(d + l.geo, cb.host + l.geo, l.keys - l.geo, hipMemcpyHostToDevice, s));
        HIPCHK(e, hipMemsetAsync(d + l.keys, 0, l.out - l.keys, s));
        ImageDev ld;
        if ((rc = upload_image(e, *frame, labels->data, labels->on_device, labels->row_stride_bytes, eb, cb, l.labels, &ld)) != HAF_OK) return rc;
        oc.d_labels = ld.src; oc.label_stride = (size_t)ld.row_stride; oc.label_bytes = (int)eb; oc.n_labels = n_labels;
        oc.d_req_of_label = reinterpret_cast<const int *>(d + l.mark);
    }
    const std::vector<haf_cloud> clouds((size_t)B, chk.clouds[0]);
    const FrameSource from{frame, nullptr, &call, &oc};
    if ((rc = score_batch_impl(e, B, clouds.data(), in, out, &from)) != HAF_OK) return rc;
    if (!any_runs) return HAF_OK;

    // the label pass across the requests, on the points the request path left in its input block
    const LastCall &last = e->last;
    if (last.B != B || last.R != R || last.clouds.empty() || !last.clouds[0].staged) return fail(e, HAF_E_INTERNAL, who + "the scored batch is not the call's");
    const float *xyz = reinterpret_cast<const float *>(e->in_block.dev.p) + last.clouds[0].float_off;
    const int H = c.grid_h, W = c.grid_w;
    float r_row, r_col;
    haf_pick_math::cell_reach(H, W, &r_row, &r_col);
    const CellGeo *d_geo = reinterpret_cast<const CellGeo *>(d + l.geo);
    unsigned long long *d_key = reinterpret_cast<unsigned long long *>(d + l.keys);
    unsigned *d_cnt = reinterpret_cast<unsigned *>(d + l.cnt);
    LabelOutDev *d_out = reinterpret_cast<LabelOutDev *>(d + l.out);
    launch_map_labels_objects(xyz, frame->width, (int)n, d_geo, B, R, last.roll_first, e->d_ev16.p, H, W, r_row, r_col, oc.d_labels, oc.label_stride,
                              oc.label_bytes, n_labels, reinterpret_cast<const int *>(d + l.pick), min_vote, d_key, d_cnt, s);
    HIPCHK(e, hipGetLastError());
    launch_object_records(xyz, frame->width, (int)n, d_geo, B, R, last.roll_first, e->d_ev16.p, reinterpret_cast<const float *>(e->d_heights.p),
                          e->d_rec.p, H, W, r_row, r_col, d_key, d_cnt, d_out, s);
    if ((rc = call_finish(e, cb, (size_t)B * sizeof(LabelOutDev), l.out)) != HAF_OK) return rc;
    // best first by haf_grasp_map_labels' key (pixel indices differ between objects: the order is total)
    return hand_over_picks(e, who, reinterpret_cast<const LabelOutDev *>(cb.host + l.out), B, [](int32_t b) { return (int)b; },
                           [](int32_t b) { return b; }, frame->width, picks, poses, order, n_found);
}

}  // namespace haf_host

extern "C" {

int haf_score_objects(haf_engine *e, const haf_frame *frame, const haf_label_image *labels, int32_t n_labels, int32_t n_objects,
                      const int32_t *object_labels, const haf_grasp_input *in, int32_t min_vote, haf_grasp_output *out, haf_label_pick *picks,
                      haf_grasp_candidate *poses, int32_t *order, int32_t *n_found)
{
    return guarded(e ? &e->error : nullptr, [&] {
        return score_objects_impl(e, frame, labels, n_labels, n_objects, object_labels, in, min_vote, out, picks, poses, order, n_found);
    });
}

}  // extern "C"
