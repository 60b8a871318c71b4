// depthfilter_host.cpp -- the host side of haf_filter_depth that needs neither a device nor an engine: haf_depth_filter_default, the
// checks of an exposure stack, of the filter's parameters and of the output image (both entry points apply them), and
// haf_filter_depth_ref, the definition of record of depth_filter.h's rules; the device kernel of depthfilter.hip is tested against it
// word for word.  Built with -ffp-contract=off like every unit (build.py: FLAGS).
#include "frame_stage.h"
#include "depth_filter.h"

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace haf {

using namespace haf_depth_filter_math;

int check_depth_stack(const haf_frame *frames, int32_t n_frames, const haf_depth_filter *p, std::string &err)
{
    if (!frames || !p) { err = "null frames or parameters"; return HAF_E_ARG; }
    if (n_frames < 1 || n_frames > HAF_MAX_STACK) { err = "frame count outside [1, HAF_MAX_STACK]"; return HAF_E_ARG; }
    const haf_frame &f0 = frames[0];
    for (int k = 0; k < n_frames; k++) {
        const haf_frame &f = frames[k];
        const std::string at = "frame " + std::to_string(k) + ": ";
        std::string msg;
        const int rc = check_frame(f, msg);
        if (rc != HAF_OK) { err = at + msg; return rc; }
        if (f.kind == HAF_FRAME_XYZ_F32) { err = at + "an XYZ frame is no depth image"; return HAF_E_ARG; }
        if (f.kind != f0.kind || f.width != f0.width || f.height != f0.height) { err = at + "kind, width or height differs from frame 0's"; return HAF_E_ARG; }
        if (f.depth_scale != f0.depth_scale || f.min_depth != f0.min_depth || f.max_depth != f0.max_depth) {
            err = at + "depth_scale, min_depth or max_depth differs from frame 0's";
            return HAF_E_ARG;
        }
    }
    if (p->radius < 1 || p->radius > 3) { err = "haf_depth_filter: radius outside [1, 3]"; return HAF_E_ARG; }
    const int window = (2 * p->radius + 1) * (2 * p->radius + 1);
    if (p->min_support < 0 || p->min_support > window - 1) { err = "haf_depth_filter: min_support outside [0, (2 radius + 1)^2 - 1]"; return HAF_E_ARG; }
    if (!std::isfinite(p->tol_abs) || !std::isfinite(p->tol_rel) || p->tol_abs < 0.0f || p->tol_rel < 0.0f) {
        err = "haf_depth_filter: tol_abs and tol_rel must be finite and not negative";
        return HAF_E_ARG;
    }
    if (p->min_valid < 1 || p->min_valid > n_frames) { err = "haf_depth_filter: min_valid outside [1, n_frames]"; return HAF_E_ARG; }
    return HAF_OK;
}

int check_depth_out(const haf_frame *frames, int32_t n_frames, const void *out, size_t out_row_stride_bytes, int32_t out_on_device, std::string &err)
{
    const haf_frame &f0 = frames[0];
    const size_t elem = frame_elem_bytes(f0);
    if (check_output_image(out, out_on_device, out_row_stride_bytes, f0.width, elem, "out", err) != HAF_OK) return HAF_E_ARG;
    if (!out) return HAF_OK;
    const ByteSpan o = image_span(out, (size_t)f0.height, out_row_stride_bytes, (size_t)f0.width * elem);
    for (int k = 0; k < n_frames; k++)
        if (frames[k].on_device == out_on_device && spans_overlap(o, frame_span(frames[k]))) { err = "out overlaps frame " + std::to_string(k); return HAF_E_ARG; }
    return HAF_OK;
}

namespace {

int filter_depth_ref_impl(const haf_frame *frames, int32_t n_frames, const haf_depth_filter *p, void *out, size_t out_row_stride_bytes,
                          int64_t *stats)
{
    std::string err;
    int rc = check_depth_stack(frames, n_frames, p, err);
    if (rc != HAF_OK) return rc;
    for (int k = 0; k < n_frames; k++)
        if (frames[k].on_device != 0) return HAF_E_ARG;   // (host memory only: this function touches no device)
    if ((rc = check_depth_out(frames, n_frames, out, out_row_stride_bytes, 0, err)) != HAF_OK) return rc;
    const haf_frame &f0 = frames[0];
    const bool u16 = f0.kind == HAF_FRAME_DEPTH_U16;
    const FrameMath m = frame_math(f0);
    const size_t W = (size_t)f0.width, H = (size_t)f0.height;
    // stage T: the whole image first -- stage S counts on it, never on what it has filtered
    std::vector<uint32_t> key(W * H);
    std::vector<float> z(W * H);
    int64_t valid = 0, kept = 0;
    for (size_t v = 0; v < H; v++)
        for (size_t u = 0; u < W; u++) {
            uint32_t k[kMaxStack];
            for (int j = 0; j < kMaxStack; j++) {
                k[j] = kInvalidKey;
                if (j >= n_frames) continue;
                const char *s = static_cast<const char *>(frames[j].data) + v * frames[j].row_stride_bytes + u * (u16 ? 2 : 4);
                if (u16) { uint16_t d; memcpy(&d, s, 2); k[j] = sample_key_u16(d, m); }
                else { uint32_t w; memcpy(&w, s, 4); k[j] = sample_key_f32(w, m); }
            }
            const uint32_t med = lower_median(k, p->min_valid);
            key[v * W + u] = med;
            z[v * W + u] = u16 ? key_z_u16(med, m) : key_z_f32(med, m);
            valid += med != kInvalidKey;
        }
    // stage S
    const long R = p->radius;
    for (long v = 0; v < (long)H; v++)
        for (long u = 0; u < (long)W; u++) {
            const size_t i = (size_t)v * W + (size_t)u;
            bool keep = key[i] != kInvalidKey;
            if (keep) {
                const float zp = z[i], tp = support_tolerance(p->tol_abs, p->tol_rel, zp);
                int support = 0;
                for (long dv = -R; dv <= R; dv++)
                    for (long du = -R; du <= R; du++) {
                        const long qv = v + dv, qu = u + du;
                        if ((dv == 0 && du == 0) || qv < 0 || qv >= (long)H || qu < 0 || qu >= (long)W) continue;
                        support += supports(z[(size_t)qv * W + (size_t)qu], zp, tp);
                    }
                keep = support >= p->min_support;
            }
            kept += keep;
            char *d = static_cast<char *>(out) + (size_t)v * out_row_stride_bytes + (size_t)u * (u16 ? 2 : 4);
            if (u16) { const uint16_t s = keep ? (uint16_t)key[i] : (uint16_t)0; memcpy(d, &s, 2); }
            else { const uint32_t w = keep ? key[i] : kInvalidWord; memcpy(d, &w, 4); }
        }
    if (stats) { stats[0] = (int64_t)(W * H); stats[1] = valid; stats[2] = kept; }
    return HAF_OK;
}

}  // namespace

}  // namespace haf

extern "C" {

void haf_depth_filter_default(haf_depth_filter *p)
{
    if (!p) return;
    p->radius = 2; p->min_support = 6; p->tol_abs = 0.004f; p->tol_rel = 0.01f; p->min_valid = 1;
}

// (no C++ exception may cross the C-ABI: an image too large for the host comes back as a status)
int haf_filter_depth_ref(const haf_frame *frames, int32_t n_frames, const haf_depth_filter *p, void *out, size_t out_row_stride_bytes,
                         int64_t *stats)
{
    try {
        return haf::filter_depth_ref_impl(frames, n_frames, p, out, out_row_stride_bytes, stats);
    } catch (...) {
    }
    return HAF_E_INTERNAL;
}

}  // extern "C"
