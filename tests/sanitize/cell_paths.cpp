// cell_paths.cpp -- sanitizer driver of the cell segmenter's host units (tests/test_cell_segment_cpu.py builds it with
// -fsanitize=address,undefined together with cellsegment_host.cpp, segment_host.cpp, frames_host.cpp and parsers.cpp; host only, a
// program of its own): haf_segment_cells_ref over N x 1 clouds and small organised frames of all three kinds, both element sizes, with
// the frame, the label image, the label grid and the info table in EXACTLY sized heap blocks -- padded rows, the last row ending with
// its allocation, the table max_labels entries long, the grid nx * ny words -- so that one byte read or written past any of them is a
// report; the properties a result must have whatever the points hold; and the refusals that must come before the first point is read.
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

static uint32_t lcg_state = 2026u;
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

static void run_frame(int kind, int w, int h, int elem_bytes, size_t in_pad, size_t out_pad, int nx, int ny, int connectivity, int min_points,
                      int max_labels)
{
    const size_t point = kind == HAF_FRAME_XYZ_F32 ? 12 + 4 * in_pad : 0;
    const size_t elem = kind == HAF_FRAME_DEPTH_U16 ? 2 : kind == HAF_FRAME_DEPTH_F32 ? 4 : point;
    const size_t last = kind == HAF_FRAME_XYZ_F32 ? (size_t)(w - 1) * point + 12 : (size_t)w * elem;
    const size_t stride = (size_t)w * elem + in_pad * 4, bytes = (size_t)(h - 1) * stride + last;
    unsigned char *pix = (unsigned char *)malloc(bytes);
    for (size_t i = 0; i < bytes; i++) pix[i] = (unsigned char)lcg();          // any bit pattern: NaNs, infinities, huge and tiny values
    for (int v = 0; v < h; v++)
        for (int u = 0; u < w; u++) {
            if (lcg() % 5 == 0) continue;
            if (kind == HAF_FRAME_DEPTH_U16) { const uint16_t d = (uint16_t)(600 + lcg() % 100); memcpy(pix + (size_t)v * stride + (size_t)u * 2, &d, 2); }
            else if (kind == HAF_FRAME_DEPTH_F32) { const float z = 0.6f + 0.001f * (float)(lcg() % 100); memcpy(pix + (size_t)v * stride + (size_t)u * 4, &z, 4); }
            else {
                // around and beyond the grid's four edges, three heights
                const float p[3] = {0.01f * (float)((int)(lcg() % (unsigned)(nx + 4)) - 2), 0.01f * (float)((int)(lcg() % (unsigned)(ny + 4)) - 2),
                                    0.65f + 0.03f * (float)(lcg() % 3)};
                memcpy(pix + (size_t)v * stride + (size_t)u * point, p, 12);
            }
        }
    const haf_frame f = make_frame(kind, w, h, stride, point, pix);
    const size_t row = (size_t)w * (size_t)elem_bytes, out_stride = row + out_pad * (size_t)elem_bytes, out_bytes = (size_t)(h - 1) * out_stride + row;
    unsigned char *out = (unsigned char *)malloc(out_bytes);
    memset(out, 0xEE, out_bytes);
    haf_cell_segment_params p;
    haf_cell_segment_default(&p);
    p.plane[2] = -1.0f; p.plane[3] = 0.70f;
    p.x0 = kind == HAF_FRAME_XYZ_F32 ? 0.0f : -0.01f * (float)(nx / 2); p.y0 = kind == HAF_FRAME_XYZ_F32 ? 0.0f : -0.01f * (float)(ny / 2);
    p.nx = nx; p.ny = ny; p.connectivity = connectivity; p.max_step = 0.02f; p.min_points = min_points; p.max_labels = max_labels;
    haf_cell_segment_info *info = (haf_cell_segment_info *)malloc(sizeof(haf_cell_segment_info) * (size_t)max_labels);
    uint16_t *grid = (uint16_t *)malloc(sizeof(uint16_t) * (size_t)nx * (size_t)ny);
    int32_t n = -1;
    int64_t stats[6] = {-1, -1, -1, -1, -1, -1};
    EXPECT(haf_segment_cells_ref(&f, &p, out, elem_bytes, out_stride, grid, info, &n, stats) == HAF_OK);
    EXPECT(stats[0] == (int64_t)w * h && stats[1] <= stats[0] && stats[2] <= stats[1] && stats[3] <= stats[1] - stats[2] && stats[5] <= stats[4] && stats[4] <= stats[3]);
    EXPECT(n >= 0 && n <= max_labels && n == (stats[5] < max_labels ? stats[5] : max_labels));
    std::vector<int64_t> points((size_t)(n > 0 ? n : 0), 0), cells((size_t)(n > 0 ? n : 0), 0);
    for (int v = 0; v < h; v++) {
        for (int u = 0; u < w; u++) {
            uint32_t l = 0;
            memcpy(&l, out + (size_t)v * out_stride + (size_t)u * (size_t)elem_bytes, (size_t)elem_bytes);
            EXPECT(l <= (uint32_t)n);
            if (l >= 1 && l <= (uint32_t)n) points[l - 1]++;
        }
        for (size_t i = (size_t)v * out_stride + row; v + 1 < h && i < (size_t)(v + 1) * out_stride; i++) EXPECT(out[i] == 0xEE);
    }
    long prev = -1;
    for (int iy = 0; iy < ny; iy++)
        for (int ix = 0; ix < nx; ix++) {
            const uint16_t l = grid[(size_t)iy * (size_t)nx + (size_t)ix];
            EXPECT(l <= n);
            if (l < 1 || l > n) continue;
            const haf_cell_segment_info &s = info[l - 1];
            if (cells[l - 1]++ == 0) EXPECT(s.anchor_ix == ix && s.anchor_iy == iy);
            EXPECT(ix >= s.ix_min && ix <= s.ix_max && iy >= s.iy_min && iy <= s.iy_max);
        }
    for (int l = 0; l < n; l++) {
        EXPECT(info[l].n_points == points[(size_t)l] && info[l].n_cells == cells[(size_t)l] && info[l].n_points >= min_points);
        EXPECT(std::isfinite(info[l].top) && info[l].top >= p.min_height);
        const long anchor = (long)info[l].anchor_iy * nx + info[l].anchor_ix;
        EXPECT(anchor > prev);
        prev = anchor;
    }
    // (the grid, info and stats may be NULL)
    EXPECT(haf_segment_cells_ref(&f, &p, out, elem_bytes, out_stride, nullptr, nullptr, &n, nullptr) == HAF_OK);
    free(grid);
    free(info);
    free(out);
    free(pix);
}

int main()
{
    for (int elem_bytes : {1, 2}) {
        for (int n : {1, 63, 65, 1000}) {                                      // N x 1 clouds
            run_frame(HAF_FRAME_XYZ_F32, n, 1, elem_bytes, 0, 0, 20, 12, 8, 1, elem_bytes == 1 ? 255 : HAF_MAX_LABELS);
            run_frame(HAF_FRAME_XYZ_F32, n, 1, elem_bytes, 2, 0, 1, 7, 4, 2, 3);
            run_frame(HAF_FRAME_XYZ_F32, n, 1, elem_bytes, 0, 0, 7, 1, 8, 2, 3);
        }
        for (int kind : {HAF_FRAME_DEPTH_U16, HAF_FRAME_DEPTH_F32, HAF_FRAME_XYZ_F32})
            for (int w : {1, 13, 61})
                for (int h : {1, 7}) run_frame(kind, w, h, elem_bytes, 3, 2, 16, 9, (w & 1) ? 8 : 4, 2, 5);
    }
    // refusals that must come before the first point is read or written: these blocks are one byte long
    {
        unsigned char *one = (unsigned char *)malloc(1), *out = (unsigned char *)malloc(1);
        *out = 0xEE;
        haf_cell_segment_params p;
        haf_cell_segment_default(&p);
        int32_t n = -7;
        const haf_frame f = make_frame(HAF_FRAME_DEPTH_U16, 4, 3, 8, 0, one);
        haf_frame g = f;
        EXPECT(haf_segment_cells_ref(nullptr, &p, out, 1, 4, nullptr, nullptr, &n, nullptr) == HAF_E_ARG);
        EXPECT(haf_segment_cells_ref(&f, nullptr, out, 1, 4, nullptr, nullptr, &n, nullptr) == HAF_E_ARG);
        EXPECT(haf_segment_cells_ref(&f, &p, out, 1, 4, nullptr, nullptr, nullptr, nullptr) == HAF_E_ARG);
        EXPECT(haf_segment_cells_ref(&f, &p, nullptr, 1, 4, nullptr, nullptr, &n, nullptr) == HAF_E_ARG);
        EXPECT(haf_segment_cells_ref(&f, &p, out, 3, 4, nullptr, nullptr, &n, nullptr) == HAF_E_ARG);
        EXPECT(haf_segment_cells_ref(&f, &p, out, 1, 3, nullptr, nullptr, &n, nullptr) == HAF_E_ARG);
        EXPECT(haf_segment_cells_ref(&f, &p, one, 1, 4, nullptr, nullptr, &n, nullptr) == HAF_E_ARG);      // labels is the frame
        g.on_device = 1;
        EXPECT(haf_segment_cells_ref(&g, &p, out, 1, 4, nullptr, nullptr, &n, nullptr) == HAF_E_ARG);
        haf_cell_segment_params q = p;
        q.cell = 0.0f;
        EXPECT(haf_segment_cells_ref(&f, &q, out, 1, 4, nullptr, nullptr, &n, nullptr) == HAF_E_ARG);
        q = p; q.nx = 4096; q.ny = 4096;
        EXPECT(haf_segment_cells_ref(&f, &q, out, 1, 4, nullptr, nullptr, &n, nullptr) == HAF_E_ARG);
        q = p; q.connectivity = 6;
        EXPECT(haf_segment_cells_ref(&f, &q, out, 1, 4, nullptr, nullptr, &n, nullptr) == HAF_E_ARG);
        q = p; q.max_step = NAN;
        EXPECT(haf_segment_cells_ref(&f, &q, out, 1, 4, nullptr, nullptr, &n, nullptr) == HAF_E_ARG);
        EXPECT(*out == 0xEE && n == -7);
        haf_cell_segment_default(nullptr);
        free(out);
        free(one);
    }
    if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    printf("cell segment sanitizer job ok\n");
    return 0;
}
