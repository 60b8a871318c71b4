// shape_paths.cpp -- sanitizer driver of the label measurement's host units (tests/test_label_shape_cpu.py builds it with
// -fsanitize=address,undefined together with labelshape_host.cpp, frames_host.cpp and parsers.cpp; host only, a program of its own):
// haf_measure_labels_ref over frames of all three kinds, widths 1 / 3 / 61 / 67, heights 1 / 5 / 33, with the frame, the label image and
// the shapes in EXACTLY sized heap blocks -- padded rows, the last row ending with its allocation, shapes n_labels entries long -- so
// that one byte read or written past any of them is a report; any bit pattern in the float kinds (NaNs, infinities, 3e38: the int32
// conversion of the words must never see them) and any label value; the properties a result must have whatever the pixels hold;
// haf_object_input on what comes out; and the refusals that must come before the first pixel is read.
#include "../../include/hafgrasp.h"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int failures = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static uint32_t lcg_state = 2027u;
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

static void run_frame(int kind, int w, int h, size_t in_pad, size_t label_pad, int elem, int n_labels, bool with_plane)
{
    const size_t point = kind == HAF_FRAME_XYZ_F32 ? 12 + 4 * in_pad : 0;
    const size_t pe = kind == HAF_FRAME_DEPTH_U16 ? 2 : kind == HAF_FRAME_DEPTH_F32 ? 4 : point;
    const size_t last = kind == HAF_FRAME_XYZ_F32 ? (size_t)(w - 1) * point + 12 : (size_t)w * pe;      // an XYZ row ends with its last point's z
    const size_t stride = (size_t)w * pe + in_pad * 4, bytes = (size_t)(h - 1) * stride + last;
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
                const float p[3] = {0.007f * (float)u - 0.2f, 0.007f * (float)v, z};
                memcpy(pix + (size_t)v * stride + (size_t)u * point, p, 12);
            }
        }
    const haf_frame f = make_frame(kind, w, h, stride, point, pix);
    const size_t lstride = ((size_t)w + label_pad) * (size_t)elem, lbytes = (size_t)(h - 1) * lstride + (size_t)w * (size_t)elem;
    unsigned char *lab = (unsigned char *)malloc(lbytes);
    for (size_t i = 0; i < lbytes; i++) lab[i] = (unsigned char)lcg();         // (uint16: values up to 65535, most of them above n_labels)
    for (int v = 0; v < h; v++)
        for (int u = 0; u < w; u++) {
            if (lcg() % 4 == 0) continue;
            const unsigned l = lcg() % (unsigned)(n_labels + 2);               // 0 and n_labels + 1 among them
            if (elem == 1) lab[(size_t)v * lstride + (size_t)u] = (unsigned char)(l > 255 ? 255 : l);
            else { const uint16_t l16 = (uint16_t)l; memcpy(lab + (size_t)v * lstride + (size_t)u * 2, &l16, 2); }
        }
    const haf_label_image img = {lab, elem, 0, lstride};
    const float plane[4] = {0.0f, 0.0f, -1.0f, 0.7f};
    haf_label_shape *shapes = (haf_label_shape *)malloc(sizeof(haf_label_shape) * (size_t)n_labels);
    memset(shapes, 0x77, sizeof(haf_label_shape) * (size_t)n_labels);
    const int rc = haf_measure_labels_ref(&f, &img, n_labels, with_plane ? plane : nullptr, shapes);
    EXPECT(rc == HAF_OK);
    if (rc == HAF_OK) {
        long long pixels = 0;
        haf_config cfg;                                    // (haf_object_input reads the grid's sides of it and nothing else)
        memset(&cfg, 0, sizeof cfg);
        cfg.grid_h = 56; cfg.grid_w = 60;
        haf_grasp_input in, out;
        memset(&in, 0, sizeof in);
        in.grasp_area_center[2] = 0.25; in.grasp_area_length_x = 32.0f; in.grasp_area_length_y = 44.0f; in.approach_vector[2] = 1.0;
        for (int l = 0; l < n_labels; l++) {
            const haf_label_shape &s = shapes[l];
            pixels += s.n_pixels;
            EXPECT(s.n_pixels >= s.n_points && s.n_points >= 0 && s.found == (s.n_points > 0) && s.reserved == 0);
            int32_t fits = -1;
            if (!s.found) {
                EXPECT(s.sum[0] == 0 && s.q_min[0] == INT32_MAX && s.q_max[2] == INT32_MIN && s.t_min[11] == INT32_MAX && s.t_max[0] == INT32_MIN);
                EXPECT(s.diameter == 0.0f && s.narrow_width == 0.0f && s.height == 0.0f && s.h_max != s.h_max);
                EXPECT(haf_object_input(&cfg, &in, &s, 4, &out, &fits) == HAF_E_ARG && fits == -1);
                continue;
            }
            EXPECT(s.narrow_dir >= 0 && s.narrow_dir < HAF_SHAPE_DIRS && s.narrow_width == s.width[s.narrow_dir] && s.narrow_width <= s.long_width * 1.0001f + 1e-3f);
            for (int k = 0; k < HAF_SHAPE_DIRS; k++) EXPECT(s.t_min[k] <= s.t_max[k] && s.width[k] <= s.diameter && s.width[k] >= 0.0f);
            for (int j = 0; j < 3; j++) EXPECT(s.q_min[j] <= s.q_max[j] && s.box_min[j] <= s.centroid[j] && s.centroid[j] <= s.box_max[j] && std::fabs(s.box_max[j]) <= 16.0f);
            EXPECT(with_plane ? (s.h_max == s.h_max && s.height == s.h_max) : (s.h_max != s.h_max));
            EXPECT(haf_object_input(&cfg, &in, &s, 4, &out, &fits) == HAF_OK && (fits == 0 || fits == 1));
            EXPECT(out.grasp_area_length_x == out.grasp_area_length_y && out.grasp_area_length_x >= 16.0f && out.grasp_area_center[2] == in.grasp_area_center[2]);
        }
        EXPECT(pixels <= (long long)w * h);
    }
    free(shapes); free(lab); free(pix);
}

static void refusals()
{
    uint16_t *d = (uint16_t *)malloc(12 * 2);
    for (int i = 0; i < 12; i++) d[i] = 700;
    uint8_t *m = (uint8_t *)malloc(12);
    memset(m, 1, 12);
    const haf_frame f = make_frame(HAF_FRAME_DEPTH_U16, 4, 3, 8, 0, d);
    haf_label_shape s[2];
    const float nan = std::nanf("");
    const float bad[4] = {0.0f, nan, 1.0f, 0.0f};
    haf_label_image l = {m, 1, 0, 4};
    EXPECT(haf_measure_labels_ref(&f, &l, 2, nullptr, s) == HAF_OK && s[0].n_pixels == 12 && s[0].n_points == 12 && s[1].found == 0);
    EXPECT(haf_measure_labels_ref(&f, &l, 2, bad, s) == HAF_E_ARG);
    EXPECT(haf_measure_labels_ref(&f, &l, 0, nullptr, s) == HAF_E_ARG);
    EXPECT(haf_measure_labels_ref(&f, &l, HAF_MAX_LABELS + 1, nullptr, s) == HAF_E_ARG);
    EXPECT(haf_measure_labels_ref(&f, &l, 2, nullptr, nullptr) == HAF_E_ARG);
    EXPECT(haf_measure_labels_ref(&f, nullptr, 2, nullptr, s) == HAF_E_ARG);
    EXPECT(haf_measure_labels_ref(nullptr, &l, 2, nullptr, s) == HAF_E_ARG);
    haf_label_image q = l; q.row_stride_bytes = 3;                EXPECT(haf_measure_labels_ref(&f, &q, 2, nullptr, s) == HAF_E_ARG);
    q = l; q.elem_bytes = 4;                                      EXPECT(haf_measure_labels_ref(&f, &q, 2, nullptr, s) == HAF_E_ARG);
    q = l; q.on_device = 1;                                       EXPECT(haf_measure_labels_ref(&f, &q, 2, nullptr, s) == HAF_E_ARG);
    q = l; q.data = nullptr;                                      EXPECT(haf_measure_labels_ref(&f, &q, 2, nullptr, s) == HAF_E_ARG);
    q = l; q.elem_bytes = 2; q.row_stride_bytes = 9;              EXPECT(haf_measure_labels_ref(&f, &q, 2, nullptr, s) == HAF_E_ARG);
    q = l; q.elem_bytes = 2; q.data = m + 1; q.row_stride_bytes = 8;   EXPECT(haf_measure_labels_ref(&f, &q, 2, nullptr, s) == HAF_E_ARG);
    haf_frame g = f; g.on_device = 1;                             EXPECT(haf_measure_labels_ref(&g, &l, 2, nullptr, s) == HAF_E_ARG);
    g = f; g.data = nullptr;                                      EXPECT(haf_measure_labels_ref(&g, &l, 2, nullptr, s) == HAF_E_ARG);
    free(m); free(d);
}

int main()
{
    const int kinds[3] = {HAF_FRAME_DEPTH_U16, HAF_FRAME_DEPTH_F32, HAF_FRAME_XYZ_F32};
    const int widths[4] = {1, 3, 61, 67}, heights[3] = {1, 5, 33}, labels[4] = {1, 7, 255, HAF_MAX_LABELS};
    int n = 0;
    for (int kind : kinds)
        for (int w : widths)
            for (int h : heights) {
                const int elem = n % 2 ? 2 : 1, nl = elem == 1 && labels[n % 4] > 255 ? 255 : labels[n % 4];
                run_frame(kind, w, h, (size_t)(n % 3), (size_t)(n % 4), elem, nl, n % 3 != 0);
                n++;
            }
    refusals();
    if (failures) { fprintf(stderr, "%d failure(s)\n", failures); return 1; }
    printf("shape sanitizer job ok: %d frames\n", n);
    return 0;
}
