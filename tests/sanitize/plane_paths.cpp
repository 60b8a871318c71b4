// plane_paths.cpp -- sanitizer driver of the plane fit's host units (tests/test_plane_cpu.py builds it with -fsanitize=address,undefined
// together with plane_host.cpp, frames_host.cpp and parsers.cpp; host only, a program of its own): haf_fit_plane_ref over frames of all
// three kinds, widths 1 / 3 / 61 / 67, heights 1 / 5 / 33, with the frame, the mask, the counts and the hypothesis words in EXACTLY sized
// heap blocks -- padded rows, the last row ending with its allocation, counts and hyps n_hyp entries long -- so that one byte read or
// written past any of them is a report; any bit pattern in the float kinds (NaNs, infinities, 3e38: the int32 conversion of the refit
// and the 128-bit products must never see them); the properties a result must have whatever the pixels hold; and the refusals that must
// come before the first pixel is read.
#include "../../include/hafgrasp.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int failures = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static uint32_t lcg_state = 2026u;
static uint32_t lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }

static haf_frame make_frame(int kind, int w, int h, size_t stride, size_t point_stride, const void *data)
{
    haf_frame f;
    haf_frame_default(&f);
    f.kind = kind; f.width = w; f.height = h; f.row_stride_bytes = stride; f.point_stride_bytes = point_stride; f.data = data;
    f.fx = f.fy = 100.0f; f.cx = 0.5f * (float)w; f.cy = 0.5f * (float)h;
    f.depth_scale = kind == HAF_FRAME_DEPTH_U16 ? 0.001f : 1.0f;
    return f;
}

static void run_frame(int kind, int w, int h, size_t in_pad, size_t mask_pad, bool masked, int n_hyp, bool with_up)
{
    const size_t point = kind == HAF_FRAME_XYZ_F32 ? 12 + 4 * in_pad : 0;
    const size_t elem = kind == HAF_FRAME_DEPTH_U16 ? 2 : kind == HAF_FRAME_DEPTH_F32 ? 4 : point;
    const size_t last = kind == HAF_FRAME_XYZ_F32 ? (size_t)(w - 1) * point + 12 : (size_t)w * elem;      // an XYZ row ends with its last point's z
    const size_t stride = (size_t)w * elem + in_pad * 4, bytes = (size_t)(h - 1) * stride + last;
    unsigned char *pix = (unsigned char *)malloc(bytes);
    for (size_t i = 0; i < bytes; i++) pix[i] = (unsigned char)lcg();          // any bit pattern; U16: depths up to 65 m
    for (int v = 0; v < h; v++)
        for (int u = 0; u < w; u++) {
            if (lcg() % 5 == 0) continue;
            const float z = (lcg() % 3) ? 0.70f : 0.62f;
            const uint16_t d = (uint16_t)(z * 1000.0f);
            if (kind == HAF_FRAME_DEPTH_U16) memcpy(pix + (size_t)v * stride + (size_t)u * 2, &d, 2);
            else if (kind == HAF_FRAME_DEPTH_F32) memcpy(pix + (size_t)v * stride + (size_t)u * 4, &z, 4);
            else {
                const float p[3] = {0.007f * (float)u, 0.007f * (float)v, z};
                memcpy(pix + (size_t)v * stride + (size_t)u * point, p, 12);
            }
        }
    const haf_frame f = make_frame(kind, w, h, stride, point, pix);
    const size_t mstride = (size_t)w + mask_pad, mbytes = (size_t)(h - 1) * mstride + (size_t)w;
    uint8_t *m = (uint8_t *)malloc(mbytes);
    for (size_t i = 0; i < mbytes; i++) m[i] = (uint8_t)(lcg() % 4 ? 1 + lcg() % 255 : 0);
    const haf_roi roi = {m, mstride, 0};
    haf_plane_params p;
    haf_plane_default(&p);
    p.n_hyp = n_hyp; p.min_inliers = 3; p.seed = lcg();
    if (with_up) { p.up[2] = -1.0f; p.max_tilt = 0.3f; }
    int32_t *counts = (int32_t *)malloc(sizeof(int32_t) * (size_t)n_hyp);
    float *hyps = (float *)malloc(sizeof(float) * 4 * (size_t)n_hyp);
    haf_plane_result r;
    memset(&r, 0x77, sizeof r);
    const int rc = haf_fit_plane_ref(&f, masked ? &roi : nullptr, &p, &r, counts, hyps);
    EXPECT(rc == HAF_OK);
    if (rc == HAF_OK) {
        const int64_t px = (int64_t)w * h;
        EXPECT(r.stats[0] == px && r.stats[1] >= 0 && r.stats[1] <= px && r.stats[2] >= 0 && r.stats[2] <= n_hyp);
        EXPECT(r.winner >= 0 && r.winner < n_hyp && r.n_inliers == counts[r.winner] && r.stats[3] == r.n_inliers && r.reserved == 0);
        int live = 0;
        for (int k = 0; k < n_hyp; k++) {
            EXPECT(counts[k] >= 0 && counts[k] <= r.stats[1] && counts[k] <= counts[r.winner]);
            EXPECT(k >= r.winner || counts[k] < counts[r.winner]);          // ties go to the lowest k
            live += counts[k] > 0;
        }
        EXPECT(live <= r.stats[2]);
        EXPECT(r.moments[0] == r.n_inliers && r.moments[4] >= 0 && r.moments[7] >= 0 && r.moments[9] >= 0);
        EXPECT(r.found == ((r.n_inliers >= p.min_inliers && r.stats[1] >= 3) ? 1 : 0));
        if (r.found) {
            const double len = std::sqrt((double)r.plane[0] * r.plane[0] + (double)r.plane[1] * r.plane[1] + (double)r.plane[2] * r.plane[2]);
            EXPECT(std::fabs(len - 1.0) < 1e-6 && std::isfinite(r.plane[3]) && r.rms >= 0.0 && r.rms < 0.0053);      // (within tol of the hypothesis, and half a fixed-point step)
            if (with_up) EXPECT(r.plane[2] < 0.0f);
        } else {
            EXPECT(r.plane[0] == 0.0f && r.plane[1] == 0.0f && r.plane[2] == 0.0f && r.plane[3] == 0.0f && r.rms == 0.0);
        }
        // counts and hyps are optional, and the result does not depend on them
        haf_plane_result r2;
        memset(&r2, 0x11, sizeof r2);
        EXPECT(haf_fit_plane_ref(&f, masked ? &roi : nullptr, &p, &r2, nullptr, nullptr) == HAF_OK && memcmp(&r, &r2, sizeof r) == 0);
    }
    free(hyps); free(counts); free(m); free(pix);
}

static void refusals()
{
    uint16_t *d = (uint16_t *)malloc(12 * 2);
    for (int i = 0; i < 12; i++) d[i] = 700;
    uint8_t *m = (uint8_t *)malloc(12);
    memset(m, 1, 12);
    const haf_frame f = make_frame(HAF_FRAME_DEPTH_U16, 4, 3, 8, 0, d);
    haf_plane_params p;
    haf_plane_default(&p);
    haf_plane_result r;
    const float nan = std::nanf("");
    haf_plane_params q = p; q.tol = 0.0f;                         EXPECT(haf_fit_plane_ref(&f, nullptr, &q, &r, nullptr, nullptr) == HAF_E_ARG);
    q = p; q.tol = nan;                                           EXPECT(haf_fit_plane_ref(&f, nullptr, &q, &r, nullptr, nullptr) == HAF_E_ARG);
    q = p; q.n_hyp = 0;                                           EXPECT(haf_fit_plane_ref(&f, nullptr, &q, &r, nullptr, nullptr) == HAF_E_ARG);
    q = p; q.n_hyp = HAF_MAX_PLANE_HYP + 1;                       EXPECT(haf_fit_plane_ref(&f, nullptr, &q, &r, nullptr, nullptr) == HAF_E_ARG);
    q = p; q.min_inliers = 2;                                     EXPECT(haf_fit_plane_ref(&f, nullptr, &q, &r, nullptr, nullptr) == HAF_E_ARG);
    q = p; q.max_tilt = 1.6f;                                     EXPECT(haf_fit_plane_ref(&f, nullptr, &q, &r, nullptr, nullptr) == HAF_E_ARG);
    q = p; q.up[1] = nan;                                         EXPECT(haf_fit_plane_ref(&f, nullptr, &q, &r, nullptr, nullptr) == HAF_E_ARG);
    haf_roi roi = {m, 3, 0};                                      EXPECT(haf_fit_plane_ref(&f, &roi, &p, &r, nullptr, nullptr) == HAF_E_ARG);
    roi.row_stride_bytes = 4; roi.on_device = 1;                  EXPECT(haf_fit_plane_ref(&f, &roi, &p, &r, nullptr, nullptr) == HAF_E_ARG);
    haf_frame g = f; g.on_device = 1;                             EXPECT(haf_fit_plane_ref(&g, nullptr, &p, &r, nullptr, nullptr) == HAF_E_ARG);
    g = f; g.data = nullptr;                                      EXPECT(haf_fit_plane_ref(&g, nullptr, &p, &r, nullptr, nullptr) == HAF_E_ARG);
    g = f; g.width = 1 << 15; g.height = (1 << 13) + 1; g.row_stride_bytes = 2 << 15;      // 2^28 + 2^15 pixels over a 24-byte block
    EXPECT(haf_fit_plane_ref(&g, nullptr, &p, &r, nullptr, nullptr) == HAF_E_CAPACITY);
    EXPECT(haf_fit_plane_ref(nullptr, nullptr, &p, &r, nullptr, nullptr) == HAF_E_ARG);
    EXPECT(haf_fit_plane_ref(&f, nullptr, nullptr, &r, nullptr, nullptr) == HAF_E_ARG);
    EXPECT(haf_fit_plane_ref(&f, nullptr, &p, nullptr, nullptr, nullptr) == HAF_E_ARG);
    roi.on_device = 0;
    q = p; q.min_inliers = 3;
    EXPECT(haf_fit_plane_ref(&f, &roi, &q, &r, nullptr, nullptr) == HAF_OK && r.stats[1] == 12);
    free(m); free(d);
}

int main()
{
    const int kinds[3] = {HAF_FRAME_DEPTH_U16, HAF_FRAME_DEPTH_F32, HAF_FRAME_XYZ_F32};
    const int widths[4] = {1, 3, 61, 67}, heights[3] = {1, 5, 33}, hyps[4] = {1, 64, 65, HAF_MAX_PLANE_HYP};
    int n = 0;
    for (int kind : kinds)
        for (int w : widths)
            for (int h : heights) {
                run_frame(kind, w, h, (size_t)(n % 3), (size_t)(n % 4), n % 2 == 0, hyps[n % 4], n % 5 == 0);
                n++;
            }
    refusals();
    if (failures) { fprintf(stderr, "%d failure(s)\n", failures); return 1; }
    printf("plane sanitizer job ok: %d frames\n", n);
    return 0;
}
