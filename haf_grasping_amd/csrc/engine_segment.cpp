// engine_segment.cpp -- haf_segment_frame (include/hafgrasp.h): one sensor frame -> an image of object labels, on the device.  Every
// refusal comes before any device work (check_segment of segment_host.cpp, then the capacity); then the frame goes through the
// single-frame input of engine_stage.cpp, the seven launches of segment.hip run on the engine's stream, ONE copy brings back the counters
// and the per-label table -- and, for a host `labels`, the packed image behind them -- and ONE synchronisation ends the call.  Nothing of
// the last scored batch is read or written: the stage timings are not touched; the block and the scratch are the ones every such call
// shares (call_io, call_scratch), and the engine's own label image is a buffer only haf_segment_cells and haf_transfer_labels share.
#include "engine_state.h"

namespace haf_host {

namespace {

constexpr size_t kSegCounterBytes = 16;       // foreground pixels, components, components that pass the size rule; 16 bytes so that the table is aligned
constexpr size_t kSegInfoBytes = sizeof(haf_segment_info);
static_assert(kSegInfoBytes == 28, "the kernels write a table entry as seven ints");

int segment_frame_impl(haf_engine *e, const haf_frame *frame, const haf_segment_params *p, void *labels, int32_t elem_bytes,
                       size_t row_stride_bytes, int32_t out_on_device, haf_label_image *out_image, haf_segment_info *info, int32_t *n_labels,
                       int64_t *stats)
{
    const std::string who = "haf_segment_frame: ";
    std::string why;
    int rc;
    if ((rc = check_segment(frame, p, labels, elem_bytes, row_stride_bytes, out_on_device, n_labels, why)) != HAF_OK) return fail(e, rc, who + why);
    const haf_frame &f = *frame;
    const size_t px = (size_t)f.width * (size_t)f.height, elem = (size_t)elem_bytes;
    const bool host_out = out_on_device == 0;
    StageBuf *in = nullptr;
    if ((rc = frame_input_prepare(e, f, who, &in)) != HAF_OK) return rc;
    const size_t mp = (size_t)e->cfg.max_points;
    // the scratch: [parent][size: a word per pixel each][the scan's block totals], all read and written word by word
    CallBuffers cb;
    if ((rc = call_buffers(e, who, up16(kSegCounterBytes + (size_t)HAF_MAX_LABELS * kSegInfoBytes) + mp * 2, "the copy-back block",
                           (2 * mp + segment_scan_blocks(mp)) * sizeof(int), "the parent and size words", &cb)) != HAF_OK) return rc;
    const hipStream_t s = cb.stream;
    char *const dev = cb.dev, *const host = cb.host;
    // the copy-back block of this call: [counters][max_labels table entries][a host output image, packed]
    const size_t tab_at = kSegCounterBytes, img_at = up16(tab_at + (size_t)p->max_labels * kSegInfoBytes);
    OutputDev o;
    if ((rc = label_output_prepare(e, f, labels, elem_bytes, row_stride_bytes, out_on_device, dev + img_at, who, &o)) != HAF_OK) return rc;

    SegmentDev d;
    memset(&d, 0, sizeof d);
    if ((rc = frame_input_upload(e, f, *in, s, &d.f)) != HAF_OK) return rc;
    d.height = f.height;
    d.r = segment_rules(*p);
    d.min_pixels = p->min_pixels; d.max_labels = p->max_labels;
    d.parent = reinterpret_cast<int *>(cb.scratch);
    d.size = d.parent + px;
    d.totals = d.size + px;
    d.counters = reinterpret_cast<unsigned *>(dev);
    d.table = reinterpret_cast<int *>(dev + tab_at);
    d.out = o.dst; d.out_stride = o.dst_stride;
    d.elem_bytes = elem_bytes;
    HIPCHK(e, hipMemsetAsync(d.counters, 0, kSegCounterBytes, s));
    launch_segment(d, s);
    if ((rc = call_finish(e, cb, img_at + (host_out ? px * elem : 0))) != HAF_OK) return rc;
    label_output_finish(o, f, elem_bytes, host + img_at, out_image);
    unsigned cnt[4];
    memcpy(cnt, host, sizeof cnt);
    const int32_t n = (int32_t)std::min<unsigned>(cnt[2], (unsigned)p->max_labels);
    *n_labels = n;
    if (info && n > 0) memcpy(info, host + tab_at, (size_t)n * kSegInfoBytes);
    if (stats) { stats[0] = (int64_t)px; stats[1] = (int64_t)cnt[0]; stats[2] = (int64_t)cnt[1]; stats[3] = (int64_t)cnt[2]; }
    return HAF_OK;
}

}  // namespace

}  // namespace haf_host

extern "C" {

int haf_segment_frame(haf_engine *e, const haf_frame *frame, const haf_segment_params *p, void *labels, int32_t elem_bytes,
                      size_t row_stride_bytes, int32_t out_on_device, haf_label_image *out_image, haf_segment_info *info, int32_t *n_labels,
                      int64_t *stats)
{
    if (!e) return HAF_E_ARG;
    return guarded(&e->error, [&] {
        return segment_frame_impl(e, frame, p, labels, elem_bytes, row_stride_bytes, out_on_device, out_image, info, n_labels, stats);
    });
}

}  // extern "C"
