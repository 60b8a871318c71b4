// engine_labelshape.cpp -- haf_measure_labels (include/hafgrasp.h): every label's box in the base frame, on the device.  Every refusal
// comes before any device work (check_measure of labelshape_host.cpp, then the capacity); then the frame goes through the single-frame
// input of engine_stage.cpp and a host label image through its upload_image, the table is zeroed, the one launch of labelshape.hip runs
// on the engine's stream, ONE copy brings back the n_labels rows and ONE synchronisation ends the call.  The shapes are shape_from_row's
// (labelshape_host.cpp) -- the code haf_measure_labels_ref ends with, on the same integers.  Nothing of the last scored batch is read or
// written: the stage timings are not touched; the block is the one every such call shares (call_io).
#include "engine_state.h"

namespace haf_host {

using namespace haf_shape_math;

namespace {

// the call's block, device and pinned: [HAF_MAX_LABELS rows of the table][the packed bytes of a host label image]
constexpr size_t kShapeRowBytes = (size_t)kShapeRowWords * 4;
constexpr size_t kShapeLabelsAt = up16((size_t)HAF_MAX_LABELS * kShapeRowBytes);

int measure_labels_impl(haf_engine *e, const haf_frame *frame, const haf_label_image *labels, int32_t n_labels, const float *plane,
                        haf_label_shape *shapes)
{
    const std::string who = "haf_measure_labels: ";
    std::string why;
    int rc;
    if ((rc = check_measure(frame, labels, n_labels, plane, shapes, why)) != HAF_OK) return fail(e, rc, who + why);
    const haf_frame &f = *frame;
    const size_t eb = (size_t)labels->elem_bytes, nl = (size_t)n_labels;
    StageBuf *in = nullptr;
    if ((rc = frame_input_prepare(e, f, who, &in)) != HAF_OK) return rc;
    CallBuffers cb;
    if ((rc = call_buffers(e, who, kShapeLabelsAt + (size_t)e->cfg.max_points * 2, "the copy-back block", 0, nullptr, &cb)) != HAF_OK) return rc;
    const hipStream_t s = cb.stream;
    char *const dev = cb.dev, *const host = cb.host;

    ShapeDev d;
    memset(&d, 0, sizeof d);
    if ((rc = frame_input_upload(e, f, *in, s, &d.f)) != HAF_OK) return rc;
    ImageDev ld;
    if ((rc = upload_image(e, f, labels->data, labels->on_device, labels->row_stride_bytes, eb, cb, kShapeLabelsAt, &ld)) != HAF_OK) return rc;
    d.labels = ld.src; d.label_stride = ld.row_stride;
    d.label_bytes = labels->elem_bytes;
    d.n_labels = n_labels;
    if (plane) memcpy(d.plane, plane, sizeof d.plane);
    d.use_plane = plane ? 1 : 0;
    d.table = reinterpret_cast<unsigned *>(dev);
    HIPCHK(e, hipMemsetAsync(dev, 0, nl * kShapeRowBytes, s));      // the rows are accumulated into: the block carries some earlier call's bytes
    launch_label_shape(d, s);
    if ((rc = call_finish(e, cb, nl * kShapeRowBytes)) != HAF_OK) return rc;
    for (size_t l = 0; l < nl; l++) shape_from_row(reinterpret_cast<const uint32_t *>(host + l * kShapeRowBytes), &shapes[l]);
    return HAF_OK;
}

}  // namespace

}  // namespace haf_host

extern "C" {

int haf_measure_labels(haf_engine *e, const haf_frame *frame, const haf_label_image *labels, int32_t n_labels, const float *plane,
                       haf_label_shape *shapes)
{
    if (!e) return HAF_E_ARG;
    return guarded(&e->error, [&] { return measure_labels_impl(e, frame, labels, n_labels, plane, shapes); });
}

}  // extern "C"
