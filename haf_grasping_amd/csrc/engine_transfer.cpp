// engine_transfer.cpp -- haf_transfer_labels (include/hafgrasp.h): another camera's label image carried over to a depth frame's pixels,
// on the device.  Every refusal comes before any device work (check_transfer of transfer_host.cpp, then the engine's own image given as
// both images, then the capacities); then the frame goes through the single-frame input of engine_stage.cpp and a host camera label
// image through its upload_image, the fill and the two launches of transfer.hip run on the engine's stream, ONE copy brings back the
// counters -- and, for a host `labels`, the packed image behind them -- and ONE synchronisation ends the call.  A `zbuffer` that was
// asked for is a debugging output and a copy of its own.  The constants are transfer_rules' (transfer_host.cpp), the function
// haf_transfer_labels_ref forms them with.  Nothing of the last scored batch is read or written: the stage timings are not touched; the
// block and the scratch, which is the z-buffer, are the ones every such call shares (call_io, call_scratch); the engine's own label
// image is the segmenters'.
#include "engine_state.h"

namespace haf_host {

namespace {

constexpr size_t kTransferCounterBytes = up16(TRANSFER_CNT_WORDS * sizeof(unsigned));

int transfer_labels_impl(haf_engine *e, const haf_frame *depth, const haf_camera *cam, const haf_label_image *cam_labels, int32_t n_labels,
                         const haf_transfer_params *p, void *labels, int32_t elem_bytes, size_t row_stride_bytes, int32_t out_on_device,
                         haf_label_image *out_image, int32_t *zbuffer, int64_t *stats)
{
    const std::string who = "haf_transfer_labels: ";
    std::string why;
    int rc;
    if ((rc = check_transfer(depth, cam, cam_labels, n_labels, p, labels, elem_bytes, row_stride_bytes, out_on_device, why)) != HAF_OK) return fail(e, rc, who + why);
    const haf_frame &f = *depth;
    const haf_label_image &cl = *cam_labels;
    const size_t px = (size_t)f.width * (size_t)f.height, elem = (size_t)elem_bytes, mp = (size_t)e->cfg.max_points;
    const size_t cam_px = (size_t)cam->width * (size_t)cam->height, ceb = (size_t)cl.elem_bytes;
    const bool host_out = out_on_device == 0;
    // (the engine's own image, packed, as the camera's AND as the output)
    if (!labels && cl.on_device == 1 && e->d_seg_image.p && spans_overlap(image_span(e->d_seg_image.p, 1, 0, px * elem), label_span(cl, cam->width, cam->height)))
        return fail(e, HAF_E_ARG, who + "the engine's own image is both the camera's label image and the output");
    if (cam_px > mp) return fail(e, HAF_E_CAPACITY, who + "more camera pixels than max_points");
    StageBuf *in = nullptr;
    if ((rc = frame_input_prepare(e, f, who, &in)) != HAF_OK) return rc;
    // the call's block, device and pinned: [counters][a host output image, packed][a host camera label image, packed]
    const size_t img_at = kTransferCounterBytes, cam_at = up16(img_at + mp * 2);
    CallBuffers cb;
    if ((rc = call_buffers(e, who, cam_at + mp * 2, "the copy-back block", cam_px * sizeof(int32_t), "the z-buffer", &cb)) != HAF_OK) return rc;
    const hipStream_t s = cb.stream;
    char *const dev = cb.dev, *const host = cb.host;
    OutputDev o;
    if ((rc = label_output_prepare(e, f, labels, elem_bytes, row_stride_bytes, out_on_device, dev + img_at, who, &o)) != HAF_OK) return rc;

    TransferDev d;
    memset(&d, 0, sizeof d);
    if ((rc = frame_input_upload(e, f, *in, s, &d.f)) != HAF_OK) return rc;
    haf_frame cam_shape{};                                // (upload_image reads a frame's width and height only)
    cam_shape.width = cam->width; cam_shape.height = cam->height;
    ImageDev ld;
    if ((rc = upload_image(e, cam_shape, cl.data, cl.on_device, cl.row_stride_bytes, ceb, cb, cam_at, &ld)) != HAF_OK) return rc;
    d.r = transfer_rules(*cam, *p);
    d.z = reinterpret_cast<int *>(cb.scratch);
    d.labels = ld.src; d.label_stride = ld.row_stride;
    d.label_bytes = cl.elem_bytes;
    d.n_labels = n_labels;
    d.out = o.dst; d.out_stride = o.dst_stride;
    d.elem_bytes = elem_bytes;
    d.counters = reinterpret_cast<unsigned *>(dev);
    HIPCHK(e, hipMemsetAsync(d.counters, 0, kTransferCounterBytes, s));
    HIPCHK(e, launch_transfer(d, s));
    HIPCHK(e, hipGetLastError());
    if (zbuffer) HIPCHK(e, hipMemcpyAsync(zbuffer, d.z, cam_px * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if ((rc = call_finish(e, cb, img_at + (host_out ? px * elem : 0))) != HAF_OK) return rc;
    label_output_finish(o, f, elem_bytes, host + img_at, out_image);
    unsigned cnt[TRANSFER_CNT_WORDS];
    memcpy(cnt, host, sizeof cnt);
    if (stats) {
        stats[0] = (int64_t)px; stats[1] = (int64_t)cnt[TRANSFER_CNT_FRONT]; stats[2] = (int64_t)cnt[TRANSFER_CNT_PROJECTS];
        stats[3] = (int64_t)cnt[TRANSFER_CNT_VISIBLE]; stats[4] = (int64_t)cnt[TRANSFER_CNT_LABELLED];
    }
    return HAF_OK;
}

}  // namespace

}  // namespace haf_host

extern "C" {

int haf_transfer_labels(haf_engine *e, const haf_frame *depth, const haf_camera *cam, const haf_label_image *cam_labels, int32_t n_labels,
                        const haf_transfer_params *p, void *labels, int32_t elem_bytes, size_t row_stride_bytes, int32_t out_on_device,
                        haf_label_image *out_image, int32_t *zbuffer, int64_t *stats)
{
    if (!e) return HAF_E_ARG;
    return guarded(&e->error, [&] {
        return transfer_labels_impl(e, depth, cam, cam_labels, n_labels, p, labels, elem_bytes, row_stride_bytes, out_on_device, out_image,
                                    zbuffer, stats);
    });
}

}  // extern "C"
