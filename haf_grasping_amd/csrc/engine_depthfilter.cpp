// engine_depthfilter.cpp -- haf_filter_depth (include/hafgrasp.h): 1..8 exposures of one depth camera -> one conditioned depth image, on
// the device.  Every refusal comes before any device work (check_depth_stack / check_depth_out of depthfilter_host.cpp, then the
// capacities); then the host exposures go up (upload_frame of engine_stage.cpp) into the raw area of haf_score_frames, each at a multiple
// of 16 bytes, ONE launch of k_depth_filter (depthfilter.hip) runs on the engine's stream, ONE copy brings back the counters -- and, for a host
// `out`, the packed image behind them -- and ONE synchronisation ends the call.  Nothing of the last scored batch is read or written: the
// raw area is only read inside the request that filled it, the stage timings are not touched.
#include "engine_state.h"

namespace haf_host {

namespace {

constexpr size_t kFiltCounterBytes = 16;      // two unsigned counters (valid after stage T, kept), 16 bytes so that the image behind them is aligned

int filter_depth_impl(haf_engine *e, const haf_frame *frames, int32_t n_frames, const haf_depth_filter *p, void *out, size_t out_row_stride_bytes,
                      int32_t out_on_device, haf_frame *out_frame, int64_t *stats)
{
    const std::string who = "haf_filter_depth: ";
    std::string why;
    int rc;
    if ((rc = check_depth_stack(frames, n_frames, p, why)) != HAF_OK) return fail(e, rc, who + why);
    if ((rc = check_depth_out(frames, n_frames, out, out_row_stride_bytes, out_on_device, why)) != HAF_OK) return fail(e, rc, who + why);
    const haf_config &c = e->cfg;
    const haf_frame &f0 = frames[0];
    const size_t px = (size_t)f0.width * (size_t)f0.height, elem = frame_pixel_bytes(f0.kind);
    if ((int64_t)px > (int64_t)c.max_points) return fail(e, HAF_E_CAPACITY, who + "frame 0: more pixels than max_points");
    const bool host_out = out_on_device == 0;
    // the raw area: [host exposures, each at a multiple of 16 bytes][counters][a host output image, packed]
    size_t off[HAF_MAX_STACK] = {}, at = 0, images = host_out ? 1 : 0;
    for (int k = 0; k < n_frames; k++) {
        if (frames[k].on_device == 1) continue;
        off[k] = at;
        at += staged_bytes(frames[k]);
        if ((int64_t)(++images * px) > (int64_t)c.max_points)
            return fail(e, HAF_E_CAPACITY, who + "frame " + std::to_string(k) + ": the host frames" + (host_out ? " and the host output image" : "") +
                                               " hold more pixels than max_points");
    }
    const size_t cnt_at = at, img_at = at + kFiltCounterBytes;
    if (img_at + (host_out ? px * elem : 0) > e->raw.dev.n) return fail(e, HAF_E_CAPACITY, who + "the raw staging area is too small");
    HIPCHK(e, hipSetDevice(c.device));
    if (!out && (rc = ensure_dev(e, e->d_filter_image, (size_t)c.max_points * 4, who, "the engine's output image")) != HAF_OK) return rc;
    const hipStream_t s = e->stream;
    char *const dev = e->raw.dev.p, *const host = e->raw.host;

    DepthStackDev d;
    memset(&d, 0, sizeof d);
    for (int k = 0; k < n_frames; k++) {
        const haf_frame &f = frames[k];
        const FrameDev fd = describe_frame(f, dev + off[k]);
        d.src[k] = fd.src;
        d.row_stride[k] = fd.row_stride;
        if (f.on_device != 1 && (rc = upload_frame(e, f, host + off[k], dev + off[k], s)) != HAF_OK) return rc;
    }
    const OutputDev o = describe_output(out, out_on_device, out_row_stride_bytes, (size_t)f0.width, elem, dev + img_at, e->d_filter_image.p);
    d.out = o.dst; d.out_stride = o.dst_stride;
    d.counters = reinterpret_cast<unsigned *>(dev + cnt_at);
    d.width = f0.width; d.height = f0.height; d.n_frames = n_frames;
    d.min_valid = p->min_valid; d.min_support = p->min_support;
    d.tol_abs = p->tol_abs; d.tol_rel = p->tol_rel;
    d.m = frame_math(f0);
    HIPCHK(e, hipMemsetAsync(d.counters, 0, kFiltCounterBytes, s));
    launch_depth_filter(d, f0.kind, p->radius, s);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(host + cnt_at, dev + cnt_at, kFiltCounterBytes + (host_out ? px * elem : 0), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    if ((rc = check_guards(e)) != HAF_OK) return rc;
    if (host_out) unpack_rows(static_cast<char *>(out), out_row_stride_bytes, host + img_at, (size_t)f0.height, (size_t)f0.width * elem);
    if (stats) {
        unsigned cnt[2];
        memcpy(cnt, host + cnt_at, sizeof cnt);
        stats[0] = (int64_t)px; stats[1] = (int64_t)cnt[0]; stats[2] = (int64_t)cnt[1];
    }
    if (out_frame) {
        *out_frame = f0;
        out_frame->data = o.data; out_frame->on_device = o.on_device; out_frame->row_stride_bytes = o.row_stride_bytes;
    }
    return HAF_OK;
}

}  // namespace

}  // namespace haf_host

extern "C" {

int haf_filter_depth(haf_engine *e, const haf_frame *frames, int32_t n_frames, const haf_depth_filter *p, void *out, size_t out_row_stride_bytes,
                     int32_t out_on_device, haf_frame *out_frame, int64_t *stats)
{
    if (!e) return HAF_E_ARG;
    return guarded(&e->error, [&] { return filter_depth_impl(e, frames, n_frames, p, out, out_row_stride_bytes, out_on_device, out_frame, stats); });
}

}  // extern "C"
