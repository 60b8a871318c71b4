// space_paths.cpp -- the CPU sanitizer job of haf_check_space_ref (tests/test_space_cpu.py builds it with -fsanitize=address,undefined
// together with space_host.cpp, clearance_host.cpp, transfer_host.cpp, frames_host.cpp, frame_stage.cpp and parsers.cpp: a program of its
// own, nothing is loaded into an interpreter).  Every buffer is a heap block of exactly the bytes the call may touch: both depth kinds,
// widths 1 / 5 / 9, heights 1 / 4 / 7, padded rows whose last row ends with its allocation, any bit pattern in the pixels, grasps read
// at both strides with void ones among them, rows, order and states of exactly n_grasps and n_grasps * N entries, and the refusals that
// must come before the first pixel is read.  Any report fails the job.
#include "../../include/hafgrasp.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

static unsigned rnd_state = 12345;
static unsigned rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

// a depth image of exactly (h - 1) * stride + w * elem bytes
static void *image_block(int kind, int w, int h, int pad, size_t *stride, bool wild)
{
    const size_t elem = kind == HAF_FRAME_DEPTH_U16 ? 2 : 4;
    *stride = (size_t)(w + pad) * elem;
    const size_t bytes = (size_t)(h - 1) * *stride + (size_t)w * elem;
    unsigned char *p = static_cast<unsigned char *>(malloc(bytes));
    for (size_t i = 0; i < bytes; i++) p[i] = (unsigned char)rnd();
    if (!wild)
        for (int v = 0; v < h; v++)
            for (int u = 0; u < w; u++) {
                unsigned char *at = p + (size_t)v * *stride + (size_t)u * elem;
                const unsigned mm = (rnd() % 7 == 0) ? 0 : 400 + rnd() % 300;
                if (kind == HAF_FRAME_DEPTH_U16) { const uint16_t d = (uint16_t)mm; memcpy(at, &d, 2); }
                else { const float d = mm ? 0.001f * (float)mm : NAN; memcpy(at, &d, 4); }
            }
    return p;
}

static haf_frame frame_of(int kind, const void *data, int w, int h, size_t stride, float shift)
{
    haf_frame f;
    haf_frame_default(&f);
    f.kind = kind; f.data = data; f.width = w; f.height = h; f.row_stride_bytes = stride;
    f.fx = f.fy = 2.5f * (float)(w > 1 ? w : 2); f.cx = (float)(w - 1) / 2; f.cy = (float)(h - 1) / 2;
    f.depth_scale = kind == HAF_FRAME_DEPTH_U16 ? 0.001f : 1.0f;
    f.sensor_to_base[3] = shift;
    return f;
}

static void fill_grasp(haf_grasp_output *g, int i)
{
    memset(g, 0, sizeof *g);
    if (i % 3 == 2) return;                               // the "nothing found" output: a void grasp
    g->grasp_point1[0] = -0.02; g->grasp_point2[0] = 0.02; g->grasp_point2[1] = 0.003 * i;
    g->averaged_grasp_point[2] = 0.5 + 0.02 * i;
    g->approach_vector[0] = 0.05 * i; g->approach_vector[2] = -1.0;
}

int main()
{
    haf_gripper grip;
    haf_gripper_default(&grip);
    haf_space_params p;
    haf_space_default(&p);
    p.sample_step = 0.01f;
    const int sizes[3][2] = {{1, 1}, {5, 4}, {9, 7}};
    for (int kind = HAF_FRAME_DEPTH_U16; kind <= HAF_FRAME_DEPTH_F32; kind++)
        for (int si = 0; si < 3; si++)
            for (int wild = 0; wild < 2; wild++)
                for (int cand = 0; cand < 2; cand++) {
                    const int w = sizes[si][0], h = sizes[si][1], n_views = 1 + si, n = 1 + 2 * si;
                    void *img[3];
                    haf_frame views[3];
                    for (int k = 0; k < n_views; k++) {
                        size_t stride;
                        img[k] = image_block(kind, w, h, k, &stride, wild != 0);
                        views[k] = frame_of(kind, img[k], w, h, stride, 0.01f * (float)k);
                    }
                    const size_t gstride = cand ? sizeof(haf_grasp_candidate) : sizeof(haf_grasp_output);
                    // the last grasp's block ends with its haf_grasp_output: what lies behind it in a candidate is not the call's to read
                    char *grasps = static_cast<char *>(malloc((size_t)(n - 1) * gstride + sizeof(haf_grasp_output)));
                    for (int i = 0; i < n; i++) {
                        haf_grasp_output g;
                        fill_grasp(&g, i);
                        memcpy(grasps + (size_t)i * gstride, &g, sizeof g);
                    }
                    haf_grasp_space *rows = static_cast<haf_grasp_space *>(malloc((size_t)n * sizeof(haf_grasp_space)));
                    int32_t *order = static_cast<int32_t *>(malloc((size_t)n * sizeof(int32_t)));
                    int32_t n_clear = -1;
                    haf_space_info info;
                    EXPECT(haf_check_space_ref(views, n_views, &grip, &p, n, grasps, gstride, rows, order, &n_clear, &info, nullptr) == HAF_OK);
                    EXPECT(info.n_samples == 189 && n_clear >= 0 && n_clear <= n);
                    uint8_t *states = static_cast<uint8_t *>(malloc((size_t)n * (size_t)info.n_samples));
                    haf_grasp_space *again = static_cast<haf_grasp_space *>(malloc((size_t)n * sizeof(haf_grasp_space)));
                    EXPECT(haf_check_space_ref(views, n_views, &grip, &p, n, grasps, gstride, again, nullptr, nullptr, nullptr, states) == HAF_OK);
                    EXPECT(memcmp(rows, again, (size_t)n * sizeof(haf_grasp_space)) == 0);
                    for (int i = 0; i < n; i++) {
                        int64_t total = 0;
                        for (int r = 0; r < 4; r++)
                            for (int s = 0; s < 4; s++) total += rows[i].n[r][s];
                        EXPECT(i % 3 == 2 ? (rows[i].clear == -1 && total == 0) : (rows[i].clear >= 0 && total == info.n_samples));
                    }
                    // refusals come before the first pixel is read: a null data pointer elsewhere is never dereferenced
                    haf_frame bad = views[0];
                    bad.kind = HAF_FRAME_XYZ_F32; bad.point_stride_bytes = 12;
                    EXPECT(haf_check_space_ref(&bad, 1, &grip, &p, n, grasps, gstride, rows, order, &n_clear, &info, states) == HAF_E_ARG);
                    EXPECT(haf_check_space_ref(views, 0, &grip, &p, n, grasps, gstride, rows, order, &n_clear, &info, states) == HAF_E_ARG);
                    EXPECT(haf_check_space_ref(views, n_views, &grip, &p, n, grasps, gstride - 4, rows, order, &n_clear, &info, states) == HAF_E_ARG);
                    haf_space_params q = p;
                    q.sample_step = 0.0001f;
                    EXPECT(haf_check_space_ref(views, n_views, &grip, &q, n, grasps, gstride, rows, order, &n_clear, &info, states) == HAF_E_ARG);
                    free(again); free(states); free(order); free(rows); free(grasps);
                    for (int k = 0; k < n_views; k++) free(img[k]);
                }
    printf(failures ? "FAILED: %d\n" : "space sanitizer job ok\n", failures);
    return failures ? 1 : 0;
}
