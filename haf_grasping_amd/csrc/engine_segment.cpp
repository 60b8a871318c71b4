// engine_segment.cpp -- haf_segment_frame (include/hafgrasp.h): one sensor frame -> an image of object labels, on the device.  Every
// refusal comes before any device work (check_segment of segment_host.cpp, then the capacity); then a host frame is staged through
// stage_frame -- a depth frame into the raw area of haf_score_frames, an XYZ frame into that of haf_score_views -- the seven launches of
// segment.hip run on the engine's stream, ONE copy brings back the counters and the per-label table -- and, for a host `labels`, the
// packed image behind them -- and ONE synchronisation ends the call.  Nothing of the last scored batch is read or written: the raw areas
// are only read inside the request that filled them, the stage timings are not touched, and the engine's own label image is a buffer no
// other call knows.
#include "engine_state.h"

namespace haf_host {

namespace {

constexpr size_t kSegCounterBytes = 16;       // foreground pixels, components, components that pass the size rule; 16 bytes so that the table is aligned
constexpr size_t kSegInfoBytes = sizeof(haf_segment_info);
static_assert(kSegInfoBytes == 28, "the kernels write a table entry as seven ints");

int segment_buffers(haf_engine *e, const std::string &who, bool own_image)
{
    const size_t mp = (size_t)e->cfg.max_points;
    if (!e->d_seg_words.p) {
        const hipError_t rc = e->d_seg_words.alloc(2 * mp + segment_scan_blocks(mp));
        if (rc != hipSuccess) {
            e->d_seg_words.release();
            return fail(e, HAF_E_DEVICE, who + "no device memory for the parent and size words: " + hipGetErrorString(rc));
        }
    }
    const hipError_t rc = e->seg_out.ensure(up16(kSegCounterBytes + (size_t)HAF_MAX_LABELS * kSegInfoBytes) + mp * 2);
    if (e->seg_out.pinned_failed) return fail(e, HAF_E_DEVICE, who + "no pinned memory for the copy-back block");
    if (rc != hipSuccess) return fail(e, HAF_E_DEVICE, who + "no device memory for the copy-back block: " + hipGetErrorString(rc));
    if (own_image && !e->d_seg_image.p) {
        const hipError_t irc = e->d_seg_image.alloc(mp * 2);
        if (irc != hipSuccess) {
            e->d_seg_image.release();
            return fail(e, HAF_E_DEVICE, who + "no device memory for the engine's label image: " + hipGetErrorString(irc));
        }
    }
    return HAF_OK;
}

int segment_frame_impl(haf_engine *e, const haf_frame *frame, const haf_segment_params *p, void *labels, int32_t elem_bytes,
                       size_t row_stride_bytes, int32_t out_on_device, haf_label_image *out_image, haf_segment_info *info, int32_t *n_labels,
                       int64_t *stats)
{
    const std::string who = "haf_segment_frame: ";
    std::string why;
    int rc;
    if ((rc = check_segment(frame, p, labels, elem_bytes, row_stride_bytes, out_on_device, n_labels, why)) != HAF_OK) return fail(e, rc, who + why);
    const haf_config &c = e->cfg;
    const haf_frame &f = *frame;
    const size_t px = (size_t)f.width * (size_t)f.height, elem = (size_t)elem_bytes;
    if ((int64_t)px > (int64_t)c.max_points) return fail(e, HAF_E_CAPACITY, who + "more pixels than max_points");
    const bool host_out = out_on_device == 0, host_in = f.on_device == 0, xyz = f.kind == HAF_FRAME_XYZ_F32;
    HIPCHK(e, hipSetDevice(c.device));
    if (host_in && xyz && (rc = ensure_raw_xyz(e, "haf_segment_frame")) != HAF_OK) return rc;
    StageBuf &in = xyz ? e->raw_xyz : e->raw;
    if (host_in && staged_bytes(f) > in.dev.n) return fail(e, HAF_E_CAPACITY, who + "the raw staging area is too small");
    if ((rc = segment_buffers(e, who, !labels)) != HAF_OK) return rc;
    const hipStream_t s = e->stream;
    char *const dev = e->seg_out.dev.p, *const host = e->seg_out.host;
    // the copy-back block of this call: [counters][max_labels table entries][a host output image, packed]
    const size_t tab_at = kSegCounterBytes, img_at = up16(tab_at + (size_t)p->max_labels * kSegInfoBytes);

    if (host_in) {
        const auto send = [&](size_t o, size_t bytes) { return hipMemcpyAsync(in.dev.p + o, in.host + o, bytes, hipMemcpyHostToDevice, s); };
        HIPCHK(e, stage_frame(in.host, f, send));
    }
    SegmentDev d;
    memset(&d, 0, sizeof d);
    d.f = describe_frame(f, in.dev.p);
    d.height = f.height;
    d.r = segment_rules(*p);
    d.min_pixels = p->min_pixels; d.max_labels = p->max_labels;
    d.parent = e->d_seg_words.p;
    d.size = d.parent + px;
    d.totals = d.size + px;
    d.counters = reinterpret_cast<unsigned *>(dev);
    d.table = reinterpret_cast<int *>(dev + tab_at);
    d.out = host_out ? dev + img_at : labels ? labels : e->d_seg_image.p;
    d.out_stride = (host_out || !labels) ? (unsigned long long)f.width * elem : (unsigned long long)row_stride_bytes;
    d.elem_bytes = elem_bytes;
    HIPCHK(e, hipMemsetAsync(d.counters, 0, kSegCounterBytes, s));
    launch_segment(d, s);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(host, dev, img_at + (host_out ? px * elem : 0), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    if ((rc = check_guards(e)) != HAF_OK) return rc;
    if (host_out) {                                      // the packed rows into the caller's: the bytes between them are not written
        const size_t row = (size_t)f.width * elem;
        for (size_t v = 0; v < (size_t)f.height; v++) memcpy(static_cast<char *>(labels) + v * row_stride_bytes, host + img_at + v * row, row);
    }
    unsigned cnt[4];
    memcpy(cnt, host, sizeof cnt);
    const int32_t n = (int32_t)std::min<unsigned>(cnt[2], (unsigned)p->max_labels);
    *n_labels = n;
    if (info && n > 0) memcpy(info, host + tab_at, (size_t)n * kSegInfoBytes);
    if (stats) { stats[0] = (int64_t)px; stats[1] = (int64_t)cnt[0]; stats[2] = (int64_t)cnt[1]; stats[3] = (int64_t)cnt[2]; }
    if (out_image) {
        out_image->data = host_out ? labels : d.out;
        out_image->elem_bytes = elem_bytes;
        out_image->on_device = host_out ? 0 : 1;
        out_image->row_stride_bytes = host_out ? row_stride_bytes : (size_t)d.out_stride;
    }
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
