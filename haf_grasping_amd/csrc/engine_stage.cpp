// engine_stage.cpp -- what the calls that take a haf_frame share on the engine's side (the device-free half: frame_stage.h):
//   * a buffer on a call's first use (ensure_dev, ensure_stage, ensure_raw_xyz): allocated, or grown, before the call's first stream
//     operation; a failure is HAF_E_DEVICE and leaves a StageBuf as it was and a DevBuf empty, so the next call tries again;
//   * the way in and the way out of the calls that run outside the request path (call_buffers, call_finish): ONE block with its pinned
//     twin and ONE device-only scratch serve them all, since each is live only inside one call and the calls run on one stream; the
//     layout of both stays with the call, and so does writing every region before reading it;
//   * a host frame's way up (upload_frame): its rows packed into the pinned half of a block and sent in pieces of kStagePiece, the DMA
//     engine moving one while the host packs the next;
//   * the single-frame input (frame_input_prepare, frame_input_upload): a depth frame through the raw area of haf_score_frames, an XYZ
//     frame through that of haf_score_views, allocated on first need.  Two steps, so that every refusal comes before any stream operation
//     and the call's own buffers exist before the upload is enqueued.  The raw areas are only read inside the call that filled them;
//   * a side image's way to the kernels (upload_image): a host one's rows packed into the pinned half of the call's block and sent with
//     ONE copy, the bytes between the caller's rows not read; a device-resident one is read where it lies (describe_image);
//   * a label image's way out (label_output_prepare, label_output_finish): the engine's own image on first need and where the kernels
//     write (describe_output); behind the call's one copy back, a host image's rows to the caller's (unpack_rows) and the descriptor handed
//     back.  The block's layout stays with the call.  haf_filter_depth's image leaves through describe_output and unpack_rows itself.
#include "engine_state.h"

namespace haf_host {

int ensure_stage(haf_engine *e, StageBuf &b, size_t bytes, const std::string &who, const char *what)
{
    const hipError_t rc = b.ensure(bytes);
    if (b.pinned_failed) return fail(e, HAF_E_DEVICE, who + "no pinned memory for " + what);
    return rc == hipSuccess ? HAF_OK : fail(e, HAF_E_DEVICE, who + "no device memory for " + what + ": " + hipGetErrorString(rc));
}

// 12 bytes x max_points, every view at a multiple of 16 bytes: an engine that never sees a host XYZ view never pays for them
int ensure_raw_xyz(haf_engine *e, const std::string &who)
{
    if (e->raw_xyz.host) return HAF_OK;
    HIPCHK(e, hipSetDevice(e->cfg.device));
    return ensure_stage(e, e->raw_xyz, (size_t)e->cfg.max_points * 12 + (size_t)e->cfg.max_clouds * HAF_MAX_VIEWS * 16, who, "the raw area of host XYZ views");
}

int call_buffers(haf_engine *e, const std::string &who, size_t io_bytes, const char *what_io, size_t scratch_bytes, const char *what_scratch,
                 CallBuffers *out)
{
    HIPCHK(e, hipSetDevice(e->cfg.device));
    int rc;
    if ((rc = ensure_dev(e, e->call_scratch, scratch_bytes, who, what_scratch)) != HAF_OK) return rc;
    if ((rc = ensure_stage(e, e->call_io, io_bytes, who, what_io)) != HAF_OK) return rc;
    *out = CallBuffers{e->stream, e->call_io.dev.p, e->call_io.host, e->call_scratch.p};
    return HAF_OK;
}

int call_finish(haf_engine *e, const CallBuffers &cb, size_t back_bytes, size_t back_at)
{
    HIPCHK(e, hipGetLastError());
    if (back_bytes) HIPCHK(e, hipMemcpyAsync(cb.host + back_at, cb.dev + back_at, back_bytes, hipMemcpyDeviceToHost, cb.stream));
    HIPCHK(e, hipStreamSynchronize(cb.stream));
    return check_guards(e);
}

int upload_frame(haf_engine *e, const haf_frame &f, char *host_at, char *dev_at, hipStream_t s)
{
    const auto send = [&](size_t o, size_t bytes) { return hipMemcpyAsync(dev_at + o, host_at + o, bytes, hipMemcpyHostToDevice, s); };
    HIPCHK(e, stage_frame(host_at, f, send));
    return HAF_OK;
}

int frame_input_prepare(haf_engine *e, const haf_frame &f, const std::string &who, StageBuf **area)
{
    const haf_config &c = e->cfg;
    if ((int64_t)f.width * (int64_t)f.height > (int64_t)c.max_points) return fail(e, HAF_E_CAPACITY, who + "more pixels than max_points");
    const bool host = f.on_device == 0, xyz = f.kind == HAF_FRAME_XYZ_F32;
    HIPCHK(e, hipSetDevice(c.device));
    if (const int rc = host && xyz ? ensure_raw_xyz(e, who) : HAF_OK) return rc;
    *area = xyz ? &e->raw_xyz : &e->raw;
    if (host && staged_bytes(f) > (*area)->dev.n) return fail(e, HAF_E_CAPACITY, who + "the raw staging area is too small");
    return HAF_OK;
}

int frame_input_upload(haf_engine *e, const haf_frame &f, StageBuf &area, hipStream_t s, FrameDev *fd)
{
    if (const int rc = f.on_device == 0 ? upload_frame(e, f, area.host, area.dev.p, s) : HAF_OK) return rc;
    *fd = describe_frame(f, area.dev.p);
    return HAF_OK;
}

int upload_image(haf_engine *e, const haf_frame &f, const void *data, int on_device, size_t row_stride_bytes, size_t elem_bytes, const CallBuffers &cb, size_t at, ImageDev *id)
{
    const size_t w = (size_t)f.width, h = (size_t)f.height;
    *id = describe_image(data, on_device, row_stride_bytes, w, elem_bytes, cb.dev + at);
    if (!data || on_device == 1) return HAF_OK;
    pack_rows(cb.host + at, static_cast<const char *>(data), h, w, elem_bytes, elem_bytes, row_stride_bytes);
    HIPCHK(e, hipMemcpyAsync(cb.dev + at, cb.host + at, h * w * elem_bytes, hipMemcpyHostToDevice, cb.stream));
    return HAF_OK;
}

int label_output_prepare(haf_engine *e, const haf_frame &f, void *labels, int32_t elem_bytes, size_t row_stride_bytes, int32_t out_on_device, void *packed_at, const std::string &who, OutputDev *o)
{
    if (const int rc = labels ? HAF_OK : ensure_dev(e, e->d_seg_image, (size_t)e->cfg.max_points * 2, who, "the engine's label image")) return rc;
    *o = describe_output(labels, out_on_device, row_stride_bytes, (size_t)f.width, (size_t)elem_bytes, packed_at, e->d_seg_image.p);
    return HAF_OK;
}

void label_output_finish(const OutputDev &o, const haf_frame &f, int32_t elem_bytes, const char *host_packed_at, haf_label_image *out_image)
{
    if (o.on_device == 0) unpack_rows(static_cast<char *>(o.data), o.row_stride_bytes, host_packed_at, (size_t)f.height, (size_t)f.width * (size_t)elem_bytes);
    if (out_image) *out_image = o.label_image(elem_bytes);
}

}  // namespace haf_host
