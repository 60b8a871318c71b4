// frames_host.cpp -- the host side of sensor frames that needs neither a device nor an engine: haf_frame_default, the argument checks
// of a frame's own fields, haf_frame_points (the definition of record of frame_points.h's arithmetic; the device kernel of frames.hip is
// tested against it bit for bit) and the C wrapper of the PGM reader.  Built with -ffp-contract=off like every unit (build.py: FLAGS).
#include "frames.h"
#include "parsers.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

namespace haf {

using haf_frame_math::FrameMath;

size_t frame_elem_bytes(const haf_frame &f)
{
    switch (f.kind) {
        case HAF_FRAME_DEPTH_U16: return 2;
        case HAF_FRAME_DEPTH_F32: return 4;
        case HAF_FRAME_XYZ_F32: return f.point_stride_bytes;
        default: return 0;
    }
}

size_t frame_pixel_bytes(int kind) { return kind == HAF_FRAME_DEPTH_U16 ? 2 : kind == HAF_FRAME_DEPTH_F32 ? 4 : 12; }

int check_frame(const haf_frame &f, std::string &err)
{
    auto refuse = [&](int code, const char *msg) { err = std::string("haf_frame: ") + msg; return code; };
    if (f.kind != HAF_FRAME_DEPTH_U16 && f.kind != HAF_FRAME_DEPTH_F32 && f.kind != HAF_FRAME_XYZ_F32) return refuse(HAF_E_ARG, "unknown kind");
    if (f.on_device != 0 && f.on_device != 1) return refuse(HAF_E_ARG, "on_device must be 0 (host) or 1 (device-resident)");
    if (f.width < 1 || f.height < 1) return refuse(HAF_E_ARG, "width and height must be positive");
    if (!f.data) return refuse(HAF_E_ARG, "null data");
    if ((int64_t)f.width * (int64_t)f.height > (int64_t)INT32_MAX) return refuse(HAF_E_CAPACITY, "more than INT32_MAX pixels");
    const bool xyz = f.kind == HAF_FRAME_XYZ_F32;
    if (xyz && (f.point_stride_bytes < 12 || f.point_stride_bytes % 4 != 0)) return refuse(HAF_E_ARG, "point_stride_bytes must be >= 12 and a multiple of 4");
    const size_t elem = frame_elem_bytes(f), align = xyz ? 4 : elem;
    // (a point stride is bounded so that width * stride cannot wrap: no organised cloud has megabyte points)
    if (elem > ((size_t)1 << 20)) return refuse(HAF_E_ARG, "point_stride_bytes too large");
    if (f.row_stride_bytes < (size_t)f.width * elem) return refuse(HAF_E_ARG, "row_stride_bytes smaller than a row");
    if (f.row_stride_bytes % align != 0) return refuse(HAF_E_ARG, "row_stride_bytes is not a multiple of the element size");
    if (reinterpret_cast<uintptr_t>(f.data) % align != 0) return refuse(HAF_E_ARG, "data is not aligned to its element size");
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(f.sensor_to_base[i])) return refuse(HAF_E_ARG, "sensor_to_base has an entry that is not finite");
    if (!xyz) {
        if (!std::isfinite(f.fx) || !std::isfinite(f.fy) || f.fx == 0.0f || f.fy == 0.0f) return refuse(HAF_E_ARG, "fx and fy must be finite and not zero");
        if (!std::isfinite(f.cx) || !std::isfinite(f.cy)) return refuse(HAF_E_ARG, "cx and cy must be finite");
        if (!std::isfinite(f.depth_scale) || !(f.depth_scale > 0.0f)) return refuse(HAF_E_ARG, "depth_scale must be finite and positive");
        if (!std::isfinite(f.min_depth) || !std::isfinite(f.max_depth)) return refuse(HAF_E_ARG, "min_depth and max_depth must be finite");
    }
    return HAF_OK;
}

FrameMath frame_math(const haf_frame &f)
{
    FrameMath m;
    memset(&m, 0, sizeof m);
    if (f.kind != HAF_FRAME_XYZ_F32) {
        m.ifx = 1.0f / f.fx;
        m.ify = 1.0f / f.fy;
        m.cx = f.cx; m.cy = f.cy;
        m.depth_scale = f.depth_scale;
        m.min_depth = f.min_depth; m.max_depth = f.max_depth;
    }
    memcpy(m.t, f.sensor_to_base, sizeof m.t);
    return m;
}

static int frame_points_impl(const haf_frame *f, float *xyz)
{
    if (!f || !xyz) return HAF_E_ARG;
    std::string err;
    const int rc = check_frame(*f, err);
    if (rc != HAF_OK) return rc;
    if (f->on_device != 0) return HAF_E_ARG;               // (host memory only: this function touches no device)
    const FrameMath m = frame_math(*f);
    const char *base = static_cast<const char *>(f->data);
    const size_t W = (size_t)f->width;
    for (uint32_t v = 0; v < (uint32_t)f->height; v++) {
        const char *row = base + (size_t)v * f->row_stride_bytes;
        float *dst = xyz + (size_t)v * W * 3;
        for (uint32_t u = 0; u < (uint32_t)f->width; u++, dst += 3) {
            if (f->kind == HAF_FRAME_DEPTH_U16) {
                uint16_t d;
                memcpy(&d, row + (size_t)u * 2, 2);
                haf_frame_math::point_u16(m, u, v, d, dst);
            } else if (f->kind == HAF_FRAME_DEPTH_F32) {
                float d;
                memcpy(&d, row + (size_t)u * 4, 4);
                haf_frame_math::point_f32(m, u, v, d, dst);
            } else {
                float p[3];
                memcpy(p, row + (size_t)u * f->point_stride_bytes, 12);
                haf_frame_math::point_xyz(m, p[0], p[1], p[2], dst);
            }
        }
    }
    return HAF_OK;
}

// haf_view_points: frame after frame, pixel after pixel as frame_points_impl walks them, the points whose three words are finite kept
// in that order.  Every view is checked before the first point is written
int view_points_impl(const haf_frame *frames, int32_t n_views, float *xyz, size_t cap_points, size_t *n_valid, std::string &err)
{
    if (!frames || !n_valid) { err = "haf_view_points: null argument"; return HAF_E_ARG; }
    if (n_views < 1 || n_views > HAF_MAX_VIEWS) { err = "haf_view_points: view count outside [1, HAF_MAX_VIEWS]"; return HAF_E_ARG; }
    for (int v = 0; v < n_views; v++) {
        std::string msg;
        int rc = check_frame(frames[v], msg);
        if (rc == HAF_OK && frames[v].on_device != 0) { rc = HAF_E_ARG; msg = "haf_frame: host memory only"; }
        if (rc != HAF_OK) { err = "haf_view_points: view " + std::to_string(v) + ": " + msg; return rc; }
    }
    using haf_frame_math::f_finite;
    size_t n = 0;
    for (int v = 0; v < n_views; v++) {
        const haf_frame &f = frames[v];
        const FrameMath m = frame_math(f);
        for (uint32_t r = 0; r < (uint32_t)f.height; r++) {
            const char *src = static_cast<const char *>(f.data) + (size_t)r * f.row_stride_bytes;
            for (uint32_t u = 0; u < (uint32_t)f.width; u++) {
                float p[3], dst[3];
                if (f.kind == HAF_FRAME_DEPTH_U16) {
                    uint16_t d;
                    memcpy(&d, src + (size_t)u * 2, 2);
                    haf_frame_math::point_u16(m, u, r, d, dst);
                } else if (f.kind == HAF_FRAME_DEPTH_F32) {
                    float d;
                    memcpy(&d, src + (size_t)u * 4, 4);
                    haf_frame_math::point_f32(m, u, r, d, dst);
                } else {
                    memcpy(p, src + (size_t)u * f.point_stride_bytes, 12);
                    haf_frame_math::point_xyz(m, p[0], p[1], p[2], dst);
                }
                if (!(f_finite(dst[0]) && f_finite(dst[1]) && f_finite(dst[2]))) continue;
                if (xyz) {
                    if (n >= cap_points) { err = "haf_view_points: xyz holds fewer points than the views have valid ones"; return HAF_E_CAPACITY; }
                    memcpy(xyz + n * 3, dst, 12);
                }
                n++;
            }
        }
    }
    *n_valid = n;
    return HAF_OK;
}

static int pgm16_load_impl(const char *path, uint16_t **depth, int32_t *width, int32_t *height, char *err, size_t err_cap)
{
    if (!path || !depth || !width || !height) return HAF_E_ARG;
    std::vector<unsigned short> v;
    std::string msg;
    int w = 0, h = 0;
    if (!load_pgm16(path, v, w, h, msg)) {
        if (err && err_cap) snprintf(err, err_cap, "%s", msg.c_str());
        return HAF_E_IO;
    }
    *depth = (uint16_t *)malloc(std::max<size_t>(1, v.size()) * sizeof(uint16_t));
    if (!*depth) return HAF_E_INTERNAL;
    memcpy(*depth, v.data(), v.size() * sizeof(uint16_t));
    *width = w;
    *height = h;
    return HAF_OK;
}

}  // namespace haf

extern "C" {

void haf_frame_default(haf_frame *f)
{
    if (!f) return;
    memset(f, 0, sizeof *f);
    f->depth_scale = 0.001f;
    f->sensor_to_base[0] = f->sensor_to_base[5] = f->sensor_to_base[10] = 1.0f;
}

// (here, with the other entry points that need no device, so that a host-only program can link the readers and their release)
void haf_free(void *p) { free(p); }

int haf_frame_points(const haf_frame *f, float *xyz) { return haf::frame_points_impl(f, xyz); }

// (no C++ exception may cross the C-ABI: a file too large for the host comes back as a status)
int haf_pgm16_load(const char *path, uint16_t **depth, int32_t *width, int32_t *height, char *err, size_t err_cap)
{
    try {
        return haf::pgm16_load_impl(path, depth, width, height, err, err_cap);
    } catch (const std::bad_alloc &) {
        if (err && err_cap) snprintf(err, err_cap, "out of host memory");
    } catch (...) {
        if (err && err_cap) snprintf(err, err_cap, "internal error");
    }
    return HAF_E_INTERNAL;
}

}  // extern "C"
