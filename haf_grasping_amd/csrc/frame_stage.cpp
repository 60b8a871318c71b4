// frame_stage.cpp -- frame_stage.h's definitions.  No device, no engine: tests/sanitize/stage_paths.cpp drives every line here over
// exactly sized heap blocks under the address and undefined-behaviour sanitizers.
#include "frame_stage.h"

namespace haf {

FrameDev describe_frame(const haf_frame &f, const void *staged_at)
{
    FrameDev fd;
    memset(&fd, 0, sizeof fd);
    fd.width = f.width; fd.n = f.width * f.height; fd.kind = f.kind;
    fd.m = frame_math(f);
    const size_t px = frame_pixel_bytes(f.kind);
    const bool resident = f.on_device == 1;
    fd.src = resident ? f.data : staged_at;
    fd.row_stride = resident ? f.row_stride_bytes : (unsigned long long)f.width * px;
    fd.point_stride = (unsigned)(resident ? frame_elem_bytes(f) : px);
    return fd;
}

size_t staged_bytes(const haf_frame &f)
{
    return f.on_device == 1 ? 0 : up16((size_t)f.width * (size_t)f.height * frame_pixel_bytes(f.kind));
}

void pack_rows(char *dst, const char *src, size_t height, size_t width, size_t elem_bytes, size_t elem_stride, size_t row_stride)
{
    const size_t row_bytes = width * elem_bytes;
    for (size_t v = 0; v < height; v++, dst += row_bytes, src += row_stride) {
        if (elem_stride == elem_bytes) memcpy(dst, src, row_bytes);
        else for (size_t u = 0; u < width; u++) memcpy(dst + u * elem_bytes, src + u * elem_stride, elem_bytes);
    }
}

void unpack_rows(char *dst, size_t dst_row_stride, const char *src_packed, size_t height, size_t row_bytes)
{
    for (size_t v = 0; v < height; v++) memcpy(dst + v * dst_row_stride, src_packed + v * row_bytes, row_bytes);
}

ImageDev describe_image(const void *data, int on_device, size_t row_stride_bytes, size_t width, size_t elem_bytes, const void *staged_at)
{
    if (!data) return {nullptr, 0};
    if (on_device == 1) return {data, (unsigned long long)row_stride_bytes};
    return {staged_at, (unsigned long long)width * elem_bytes};
}

OutputDev describe_output(void *out, int out_on_device, size_t out_row_stride_bytes, size_t width, size_t elem_bytes, void *packed_at, void *own)
{
    const unsigned long long packed = (unsigned long long)width * elem_bytes;
    if (out_on_device == 0) return {packed_at, packed, out, 0, out_row_stride_bytes};
    if (out) return {out, (unsigned long long)out_row_stride_bytes, out, 1, out_row_stride_bytes};
    return {own, packed, own, 1, (size_t)packed};
}

FrameBatch check_frame_batch(const haf_frame *frames, int32_t n, const int32_t *views_per_request, int64_t max_points)
{
    FrameBatch r;
    r.clouds.resize((size_t)n);
    int64_t total = 0;
    for (int b = 0, k = 0; b < n; b++) {
        size_t upper = 0;
        const int views = views_per_request ? views_per_request[b] : 1;
        for (int v = 0; v < views; v++, k++) {
            r.request = b; r.view = v;
            if ((r.code = check_frame(frames[k], r.text)) != HAF_OK) return r;
            const size_t px = (size_t)frames[k].width * (size_t)frames[k].height;
            total += (int64_t)px;
            if (total > max_points) { r.code = HAF_E_CAPACITY; return r; }
            upper += px;
            r.host_xyz = r.host_xyz || (frames[k].kind == HAF_FRAME_XYZ_F32 && frames[k].on_device == 0);
        }
        r.clouds[(size_t)b] = haf_cloud{static_cast<const float *>(frames[k - 1].data), upper, 3, 0};
    }
    return r;
}

}  // namespace haf
