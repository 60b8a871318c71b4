// segment_paths.cpp -- sanitizer driver of the segmentation's host units (tests/test_segment_cpu.py builds it with
// -fsanitize=address,undefined together with segment_host.cpp, frames_host.cpp and parsers.cpp; host only, a program of its own):
// haf_segment_ref over frames of all three kinds, widths 1 / 3 / 61 / 64 / 65, heights 1 / 5 / 17, both element sizes, with the frame,
// the label image and the info table in EXACTLY sized heap blocks -- padded rows, the last row ending with its allocation, the table
// max_labels entries long -- so that one byte read or written past any of them is a report; the properties a label image must have
// whatever the pixels hold; and the refusals that must come before the first pixel is read.
#include "../../include/hafgrasp.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static uint32_t lcg_state = 2025u;
static uint32_t lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }

static haf_frame make_frame(int kind, int w, int h, size_t stride, size_t point_stride, const void *data)
{
    haf_frame f;
    haf_frame_default(&f);
    f.kind = kind; f.width = w; f.height = h; f.row_stride_bytes = stride; f.point_stride_bytes = point_stride; f.data = data;
    f.fx = f.fy = 525.0f; f.cx = 0.5f * (float)w; f.cy = 0.5f * (float)h;
    f.depth_scale = kind == HAF_FRAME_DEPTH_U16 ? 0.001f : 1.0f;
    return f;
}

static void run_frame(int kind, int w, int h, int elem_bytes, size_t in_pad, size_t out_pad, int min_pixels, int max_labels)
{
    const size_t point = kind == HAF_FRAME_XYZ_F32 ? 12 + 4 * in_pad : 0;
    const size_t elem = kind == HAF_FRAME_DEPTH_U16 ? 2 : kind == HAF_FRAME_DEPTH_F32 ? 4 : point;
    const size_t last = kind == HAF_FRAME_XYZ_F32 ? (size_t)(w - 1) * point + 12 : (size_t)w * elem;      // an XYZ row ends with its last point's z
    const size_t stride = (size_t)w * elem + in_pad * 4, bytes = (size_t)(h - 1) * stride + last;
    unsigned char *pix = (unsigned char *)malloc(bytes);
    if (kind == HAF_FRAME_DEPTH_U16) {
        // a table at 700 mm with blocks 50 and 120 mm above it, holes, and any bit pattern now and then
        for (int v = 0; v < h; v++)
            for (int u = 0; u < w; u++) {
                const uint32_t r = lcg() % 100;
                uint16_t d = r < 50 ? (uint16_t)(((u / 5 + v / 3) & 1) ? 650 : 580) : r < 90 ? 700 : r < 95 ? 0 : (uint16_t)lcg();
                memcpy(pix + (size_t)v * stride + (size_t)u * 2, &d, 2);
            }
    } else {
        for (size_t i = 0; i < bytes; i++) pix[i] = (unsigned char)lcg();      // any bit pattern: NaNs, infinities, subnormals
        for (int v = 0; v < h; v++)
            for (int u = 0; u < w; u++) {
                if (lcg() % 4 == 0) continue;
                const float z = (lcg() % 2) ? 0.65f : 0.70f;
                if (kind == HAF_FRAME_DEPTH_F32) memcpy(pix + (size_t)v * stride + (size_t)u * 4, &z, 4);
                else {
                    const float p[3] = {0.001f * (float)u, 0.001f * (float)v, z};
                    memcpy(pix + (size_t)v * stride + (size_t)u * point, p, 12);
                }
            }
    }
    const haf_frame f = make_frame(kind, w, h, stride, point, pix);
    const size_t row = (size_t)w * (size_t)elem_bytes, out_stride = row + out_pad * (size_t)elem_bytes, out_bytes = (size_t)(h - 1) * out_stride + row;
    unsigned char *out = (unsigned char *)malloc(out_bytes);
    memset(out, 0xEE, out_bytes);
    haf_segment_params p;
    haf_segment_default(&p);
    p.plane[2] = -1.0f; p.plane[3] = 0.70f;
    p.min_pixels = min_pixels; p.max_labels = max_labels;
    haf_segment_info *info = (haf_segment_info *)malloc(sizeof(haf_segment_info) * (size_t)max_labels);
    int32_t n = -1;
    int64_t stats[4] = {-1, -1, -1, -1};
    EXPECT(haf_segment_ref(&f, &p, out, elem_bytes, out_stride, info, &n, stats) == HAF_OK);
    EXPECT(stats[0] == (int64_t)w * h && stats[1] <= stats[0] && stats[2] <= stats[1] && stats[3] <= stats[2]);
    EXPECT(n >= 0 && n <= max_labels && n == (stats[3] < max_labels ? stats[3] : max_labels));
    std::vector<haf_segment_info> seen((size_t)(n > 0 ? n : 0));
    for (auto &s : seen) { s.n_pixels = 0; s.anchor_u = s.anchor_v = -1; s.u_min = w; s.v_min = h; s.u_max = s.v_max = -1; }
    for (int v = 0; v < h; v++) {
        for (int u = 0; u < w; u++) {
            uint32_t l = 0;
            memcpy(&l, out + (size_t)v * out_stride + (size_t)u * (size_t)elem_bytes, (size_t)elem_bytes);
            EXPECT(l <= (uint32_t)n);
            if (l == 0 || l > (uint32_t)n) continue;
            haf_segment_info &s = seen[l - 1];
            if (s.n_pixels++ == 0) { s.anchor_u = u; s.anchor_v = v; }
            if (u < s.u_min) s.u_min = u;
            if (u > s.u_max) s.u_max = u;
            if (v < s.v_min) s.v_min = v;
            if (v > s.v_max) s.v_max = v;
        }
        for (size_t i = (size_t)v * out_stride + row; v + 1 < h && i < (size_t)(v + 1) * out_stride; i++) EXPECT(out[i] == 0xEE);
    }
    long prev = -1;
    for (int l = 0; l < n; l++) {
        EXPECT(memcmp(&seen[(size_t)l], &info[l], sizeof(haf_segment_info)) == 0);
        EXPECT(info[l].n_pixels >= min_pixels);
        const long anchor = (long)info[l].anchor_v * w + info[l].anchor_u;
        EXPECT(anchor > prev);
        prev = anchor;
    }
    // (info and stats may be NULL)
    EXPECT(haf_segment_ref(&f, &p, out, elem_bytes, out_stride, nullptr, &n, nullptr) == HAF_OK);
    free(info);
    free(out);
    free(pix);
}

int main()
{
    const int widths[] = {1, 3, 61, 64, 65}, heights[] = {1, 5, 17};
    for (int kind : {HAF_FRAME_DEPTH_U16, HAF_FRAME_DEPTH_F32, HAF_FRAME_XYZ_F32})
        for (int w : widths)
            for (int h : heights)
                for (int elem_bytes : {1, 2}) {
                    run_frame(kind, w, h, elem_bytes, 0, 0, 1, elem_bytes == 1 ? 255 : HAF_MAX_LABELS);
                    run_frame(kind, w, h, elem_bytes, 3, 2, 2, 3);
                }
    // refusals that must come before the first pixel is read or written: these blocks are one byte long
    {
        unsigned char *one = (unsigned char *)malloc(1), *out = (unsigned char *)malloc(1);
        *out = 0xEE;
        haf_segment_params p;
        haf_segment_default(&p);
        int32_t n = -7;
        const haf_frame f = make_frame(HAF_FRAME_DEPTH_U16, 4, 3, 8, 0, one);
        haf_frame g = f;
        EXPECT(haf_segment_ref(nullptr, &p, out, 1, 4, nullptr, &n, nullptr) == HAF_E_ARG);
        EXPECT(haf_segment_ref(&f, nullptr, out, 1, 4, nullptr, &n, nullptr) == HAF_E_ARG);
        EXPECT(haf_segment_ref(&f, &p, out, 1, 4, nullptr, nullptr, nullptr) == HAF_E_ARG);
        EXPECT(haf_segment_ref(&f, &p, nullptr, 1, 4, nullptr, &n, nullptr) == HAF_E_ARG);
        EXPECT(haf_segment_ref(&f, &p, out, 3, 4, nullptr, &n, nullptr) == HAF_E_ARG);
        EXPECT(haf_segment_ref(&f, &p, out, 1, 3, nullptr, &n, nullptr) == HAF_E_ARG);
        EXPECT(haf_segment_ref(&f, &p, out, 2, 9, nullptr, &n, nullptr) == HAF_E_ARG);
        EXPECT(haf_segment_ref(&f, &p, one, 1, 4, nullptr, &n, nullptr) == HAF_E_ARG);              // labels is the frame
        g.on_device = 1;
        EXPECT(haf_segment_ref(&g, &p, out, 1, 4, nullptr, &n, nullptr) == HAF_E_ARG);
        g = f; g.width = 65536; g.height = 32768; g.row_stride_bytes = 131072;
        EXPECT(haf_segment_ref(&g, &p, out, 1, 65536, nullptr, &n, nullptr) == HAF_E_CAPACITY);
        haf_segment_params q = p;
        q.plane[1] = NAN;
        EXPECT(haf_segment_ref(&f, &q, out, 1, 4, nullptr, &n, nullptr) == HAF_E_ARG);
        q = p; q.max_gap = 0.0f;
        EXPECT(haf_segment_ref(&f, &q, out, 1, 4, nullptr, &n, nullptr) == HAF_E_ARG);
        q = p; q.min_pixels = 0;
        EXPECT(haf_segment_ref(&f, &q, out, 1, 4, nullptr, &n, nullptr) == HAF_E_ARG);
        q = p; q.max_labels = 256;
        EXPECT(haf_segment_ref(&f, &q, out, 1, 4, nullptr, &n, nullptr) == HAF_E_ARG);
        EXPECT(*out == 0xEE && n == -7);
        haf_segment_default(nullptr);
        free(out);
        free(one);
    }
    if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    printf("segment sanitizer job ok\n");
    return 0;
}
