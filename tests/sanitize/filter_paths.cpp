// filter_paths.cpp -- sanitizer driver of the depth filter's host units (tests/test_depth_filter_cpu.py builds it with
// -fsanitize=address,undefined together with depthfilter_host.cpp, frames_host.cpp and parsers.cpp; host only, a program of its own):
// haf_filter_depth_ref over stacks of 1 and 8 exposures of both kinds, widths 1 / 3 / 61 / 64, heights 1 / 5, every radius, with the
// exposures and the output in EXACTLY sized heap blocks -- padded rows, the last row ending with its allocation -- so that one byte read
// or written past either is a report; the refusals that must come before the first sample is read; and depth_filter.h's median network
// against std::sort on every pattern of valid and invalid keys.
#include "../../include/hafgrasp.h"
#include "../../haf_grasping_amd/csrc/depth_filter.h"

#include <algorithm>
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

static uint32_t lcg_state = 2024u;
static uint32_t lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }

static haf_frame depth_frame(int kind, int w, int h, size_t stride, const void *data)
{
    haf_frame f;
    haf_frame_default(&f);
    f.kind = kind; f.width = w; f.height = h; f.row_stride_bytes = stride; f.data = data;
    f.fx = f.fy = 525.0f; f.cx = 0.5f * (float)w; f.cy = 0.5f * (float)h;
    f.depth_scale = kind == HAF_FRAME_DEPTH_U16 ? 0.001f : 1.0f;
    f.min_depth = 0.3f; f.max_depth = 40.0f;
    return f;
}

// one stack through the reference: every block holds exactly the bytes its frame describes
static void run_stack(int kind, int w, int h, int n, int radius, size_t in_pad, size_t out_pad)
{
    const size_t elem = kind == HAF_FRAME_DEPTH_U16 ? 2 : 4, row = (size_t)w * elem;
    std::vector<unsigned char *> blocks;
    std::vector<haf_frame> frames;
    for (int k = 0; k < n; k++) {
        const size_t stride = row + (in_pad + (size_t)(k % 2)) * elem, bytes = (size_t)(h - 1) * stride + row;
        unsigned char *pix = (unsigned char *)malloc(bytes);
        for (size_t i = 0; i < bytes; i++) pix[i] = (unsigned char)lcg();      // any bit pattern: NaNs, infinities, subnormals, zeros
        blocks.push_back(pix);
        frames.push_back(depth_frame(kind, w, h, stride, pix));
    }
    const size_t out_stride = row + out_pad * elem, out_bytes = (size_t)(h - 1) * out_stride + row;
    unsigned char *out = (unsigned char *)malloc(out_bytes);
    memset(out, 0xEE, out_bytes);
    haf_depth_filter p;
    haf_depth_filter_default(&p);
    p.radius = radius; p.min_support = radius; p.tol_abs = 5.0f; p.tol_rel = 0.5f; p.min_valid = 1 + (n > 1);
    int64_t stats[3] = {-1, -1, -1};
    EXPECT(haf_filter_depth_ref(frames.data(), n, &p, out, out_stride, stats) == HAF_OK);
    EXPECT(stats[0] == (int64_t)w * h && stats[1] >= stats[2] && stats[2] >= 0 && stats[1] <= stats[0]);
    int64_t kept = 0;
    for (int v = 0; v < h; v++) {
        for (int u = 0; u < w; u++) {
            uint32_t word = 0;
            memcpy(&word, out + (size_t)v * out_stride + (size_t)u * elem, elem);
            const bool valid = kind == HAF_FRAME_DEPTH_U16 ? word != 0 : word != 0x7FC00000u;
            kept += valid;
            bool among = false;
            for (int k = 0; k < n && valid; k++) among = among || memcmp(&word, blocks[(size_t)k] + (size_t)v * frames[(size_t)k].row_stride_bytes + (size_t)u * elem, elem) == 0;
            EXPECT(!valid || among);
        }
        for (size_t i = (size_t)v * out_stride + row; v + 1 < h && i < (size_t)(v + 1) * out_stride; i++) EXPECT(out[i] == 0xEE);
    }
    EXPECT(kept == stats[2]);
    free(out);
    for (unsigned char *b : blocks) free(b);
}

static void median_network()
{
    using namespace haf_depth_filter_math;
    for (int pattern = 0; pattern < 256; pattern++)
        for (int trial = 0; trial < 8; trial++) {
            uint32_t k[kMaxStack];
            std::vector<uint32_t> valid;
            for (int j = 0; j < kMaxStack; j++) {
                k[j] = (pattern >> j) & 1 ? lcg() % (trial < 4 ? 5u : 0x7F800000u) : kInvalidKey;      // (small ranges: equal keys)
                if (k[j] != kInvalidKey) valid.push_back(k[j]);
            }
            std::sort(valid.begin(), valid.end());
            const int c = (int)valid.size();
            for (int min_valid = 1; min_valid <= kMaxStack; min_valid++) {
                uint32_t copy[kMaxStack];
                memcpy(copy, k, sizeof copy);
                const uint32_t want = c >= min_valid && c > 0 ? valid[(size_t)((c - 1) / 2)] : kInvalidKey;
                EXPECT(lower_median(copy, min_valid) == want);
            }
        }
}

int main()
{
    median_network();
    const int widths[] = {1, 3, 61, 64}, heights[] = {1, 5};
    for (int kind : {HAF_FRAME_DEPTH_U16, HAF_FRAME_DEPTH_F32})
        for (int w : widths)
            for (int h : heights)
                for (int n : {1, 8})
                    for (int radius = 1; radius <= 3; radius++) {
                        run_stack(kind, w, h, n, radius, 0, 0);
                        run_stack(kind, w, h, n, radius, 3, 2);
                    }
    // refusals that must come before the first sample is read or written: these blocks are one byte long
    {
        unsigned char *one = (unsigned char *)malloc(1), *out = (unsigned char *)malloc(1);
        *out = 0xEE;
        haf_depth_filter p;
        haf_depth_filter_default(&p);
        haf_frame f = depth_frame(HAF_FRAME_DEPTH_U16, 4, 3, 8, one), g = f;
        EXPECT(haf_filter_depth_ref(nullptr, 1, &p, out, 8, nullptr) == HAF_E_ARG);
        EXPECT(haf_filter_depth_ref(&f, 1, nullptr, out, 8, nullptr) == HAF_E_ARG);
        EXPECT(haf_filter_depth_ref(&f, 0, &p, out, 8, nullptr) == HAF_E_ARG);
        EXPECT(haf_filter_depth_ref(&f, HAF_MAX_STACK + 1, &p, out, 8, nullptr) == HAF_E_ARG);
        EXPECT(haf_filter_depth_ref(&f, 1, &p, nullptr, 8, nullptr) == HAF_E_ARG);
        EXPECT(haf_filter_depth_ref(&f, 1, &p, out, 6, nullptr) == HAF_E_ARG);
        EXPECT(haf_filter_depth_ref(&f, 1, &p, one, 8, nullptr) == HAF_E_ARG);                // out is the input
        g.on_device = 1;
        EXPECT(haf_filter_depth_ref(&g, 1, &p, out, 8, nullptr) == HAF_E_ARG);
        g = f; g.kind = HAF_FRAME_XYZ_F32; g.point_stride_bytes = 12; g.row_stride_bytes = 48;
        EXPECT(haf_filter_depth_ref(&g, 1, &p, out, 8, nullptr) == HAF_E_ARG);
        g = f; g.width = 65536; g.height = 32768; g.row_stride_bytes = 131072;
        EXPECT(haf_filter_depth_ref(&g, 1, &p, out, 131072, nullptr) == HAF_E_CAPACITY);
        haf_frame two[2] = {f, f};
        two[1].depth_scale = 0.002f;
        EXPECT(haf_filter_depth_ref(two, 2, &p, out, 8, nullptr) == HAF_E_ARG);
        p.radius = 4;
        EXPECT(haf_filter_depth_ref(&f, 1, &p, out, 8, nullptr) == HAF_E_ARG);
        p.radius = 2; p.tol_abs = NAN;
        EXPECT(haf_filter_depth_ref(&f, 1, &p, out, 8, nullptr) == HAF_E_ARG);
        p.tol_abs = 0.0f; p.min_valid = 2;
        EXPECT(haf_filter_depth_ref(&f, 1, &p, out, 8, nullptr) == HAF_E_ARG);
        EXPECT(*out == 0xEE);
        haf_depth_filter_default(nullptr);
        free(out);
        free(one);
    }
    if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    printf("filter sanitizer job ok\n");
    return 0;
}
