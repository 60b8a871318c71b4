// engine_labelshape.cpp -- haf_measure_labels (include/hafgrasp.h): every label's box in the base frame, on the device.  Every refusal
// comes before any device work (check_measure of labelshape_host.cpp, then the capacity); then a host frame is staged through
// stage_frame as haf_fit_plane's is, a host label image is packed into the pinned half of the call's block and sent behind it, the
// table is zeroed, the one launch of labelshape.hip runs on the engine's stream, ONE copy brings back the n_labels rows and ONE
// synchronisation ends the call.  The shapes are shape_from_row's (labelshape_host.cpp) -- the code haf_measure_labels_ref ends with, on
// the same integers.  Nothing of the last scored batch is read or written: the raw areas are only read inside the request that filled
// them, the stage timings are not touched, and the block is this call's own.
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
    const haf_config &c = e->cfg;
    const haf_frame &f = *frame;
    const size_t px = (size_t)f.width * (size_t)f.height, eb = (size_t)labels->elem_bytes, nl = (size_t)n_labels;
    if ((int64_t)px > (int64_t)c.max_points) return fail(e, HAF_E_CAPACITY, who + "more pixels than max_points");
    const bool host_in = f.on_device == 0, xyz = f.kind == HAF_FRAME_XYZ_F32, host_labels = labels->on_device == 0;
    HIPCHK(e, hipSetDevice(c.device));
    if (host_in && xyz && (rc = ensure_raw_xyz(e, "haf_measure_labels")) != HAF_OK) return rc;
    StageBuf &in = xyz ? e->raw_xyz : e->raw;
    if (host_in && staged_bytes(f) > in.dev.n) return fail(e, HAF_E_CAPACITY, who + "the raw staging area is too small");
    const hipError_t arc = e->shape_io.ensure(kShapeLabelsAt + (size_t)c.max_points * 2);
    if (e->shape_io.pinned_failed) return fail(e, HAF_E_DEVICE, who + "no pinned memory for the copy-back block");
    if (arc != hipSuccess) return fail(e, HAF_E_DEVICE, who + "no device memory for the copy-back block: " + hipGetErrorString(arc));
    const hipStream_t s = e->stream;
    char *const dev = e->shape_io.dev.p, *const host = e->shape_io.host;

    if (host_in) {
        const auto send = [&](size_t o, size_t bytes) { return hipMemcpyAsync(in.dev.p + o, in.host + o, bytes, hipMemcpyHostToDevice, s); };
        HIPCHK(e, stage_frame(in.host, f, send));
    }
    if (host_labels) {                                    // packed rows: the bytes between the caller's rows are not read
        pack_rows(host + kShapeLabelsAt, static_cast<const char *>(labels->data), (size_t)f.height, (size_t)f.width, eb, eb, labels->row_stride_bytes);
        HIPCHK(e, hipMemcpyAsync(dev + kShapeLabelsAt, host + kShapeLabelsAt, px * eb, hipMemcpyHostToDevice, s));
    }
    ShapeDev d;
    memset(&d, 0, sizeof d);
    d.f = describe_frame(f, in.dev.p);
    d.labels = host_labels ? dev + kShapeLabelsAt : labels->data;
    d.label_stride = host_labels ? (unsigned long long)f.width * eb : (unsigned long long)labels->row_stride_bytes;
    d.label_bytes = labels->elem_bytes;
    d.n_labels = n_labels;
    if (plane) memcpy(d.plane, plane, sizeof d.plane);
    d.use_plane = plane ? 1 : 0;
    d.table = reinterpret_cast<unsigned *>(dev);
    HIPCHK(e, hipMemsetAsync(dev, 0, nl * kShapeRowBytes, s));      // a reused table must not carry the last call's rows
    launch_label_shape(d, s);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(host, dev, nl * kShapeRowBytes, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    if ((rc = check_guards(e)) != HAF_OK) return rc;
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
