// frame_paths.cpp -- sanitizer driver of the sensor-frame entry points that need no device (tests/test_frames_cpu.py builds it with
// -fsanitize=address,undefined, host only): haf_pgm16_load over hostile, truncated and bit-flipped files, haf_frame_points over frames of
// every kind, shape, stride and refusal with the pixels and the points in EXACTLY sized heap blocks, so that one byte read or written
// past either is a report.  argv: a good PGM, a scratch directory, then any number of hostile files.
#include "../../include/hafgrasp.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static uint32_t lcg_state = 12345u;
static uint32_t lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }

static std::string slurp(const char *path)
{
    std::string s;
    FILE *f = fopen(path, "rb");
    if (!f) return s;
    char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
    fclose(f);
    return s;
}
static void spit(const std::string &path, const std::string &data)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (f) { fwrite(data.data(), 1, data.size(), f); fclose(f); }
}

// the loader on one file: a refusal carries a message, a success a block of exactly width * height samples
static int load(const char *path)
{
    uint16_t *d = nullptr;
    int32_t w = -1, h = -1;
    char err[64] = "";                                     // (short on purpose: the message is cut, never overrun)
    const int rc = haf_pgm16_load(path, &d, &w, &h, err, sizeof err);
    if (rc == HAF_OK) {
        EXPECT(d && w > 0 && h > 0);
        unsigned long sum = 0;
        for (size_t i = 0; i < (size_t)w * (size_t)h; i++) sum += d[i];   // every sample is readable
        (void)sum;
        haf_free(d);
    } else {
        EXPECT(rc == HAF_E_IO && err[0] != 0 && d == nullptr);
    }
    return rc;
}

// one frame through haf_frame_points: pixels and points in heap blocks of exactly the bytes the frame describes
static void run_frame(int kind, int w, int h, size_t row_pad_elems, size_t point_stride, int expect)
{
    haf_frame f;
    haf_frame_default(&f);
    const size_t elem = kind == HAF_FRAME_DEPTH_U16 ? 2 : kind == HAF_FRAME_DEPTH_F32 ? 4 : point_stride;
    const size_t align = kind == HAF_FRAME_XYZ_F32 ? 4 : elem;
    f.kind = kind; f.width = w; f.height = h;
    f.row_stride_bytes = (size_t)w * elem + row_pad_elems * align;
    f.point_stride_bytes = kind == HAF_FRAME_XYZ_F32 ? point_stride : 0;
    f.fx = 525.0f; f.fy = -525.0f; f.cx = 0.5f * (float)w; f.cy = 0.5f * (float)h;
    f.min_depth = 0.3f; f.max_depth = 3.0f;
    const float t[12] = {0.36f, 0.48f, -0.8f, 0.1f, -0.8f, 0.6f, 0.0f, -0.2f, 0.48f, 0.64f, 0.6f, 0.9f};
    memcpy(f.sensor_to_base, t, sizeof t);
    // the last row ends with its last pixel: no padding behind it, and an XYZ point's last pixel ends with its third float
    const size_t last = kind == HAF_FRAME_XYZ_F32 ? (size_t)(w - 1) * elem + 12 : (size_t)w * elem;
    const size_t bytes = (size_t)(h - 1) * f.row_stride_bytes + last;
    unsigned char *pix = (unsigned char *)malloc(bytes);
    for (size_t i = 0; i < bytes; i++) pix[i] = (unsigned char)lcg();          // any bit pattern: NaNs, infinities, subnormals
    f.data = pix;
    float *out = (float *)malloc((size_t)w * h * 12);
    const int rc = haf_frame_points(&f, out);
    EXPECT(rc == expect);
    if (rc == HAF_OK)
        for (size_t i = 0; i < (size_t)w * h * 3; i++) {
            uint32_t bits;
            memcpy(&bits, &out[i], 4);
            EXPECT(!std::isnan(out[i]) || bits == 0x7FC00000u);
        }
    free(out);
    free(pix);
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: frame_paths good.pgm scratch_dir [hostile.pgm ...]\n"); return 2; }
    const std::string good = slurp(argv[1]), dir = argv[2];
    EXPECT(!good.empty() && load(argv[1]) == HAF_OK);
    for (int i = 3; i < argc; i++) EXPECT(load(argv[i]) == HAF_E_IO);
    // every prefix of the good file, and single bit flips all over it: refused or loaded, never a report
    const std::string tmp = dir + "/sanitize_tmp.pgm";
    for (size_t n = 0; n < good.size(); n++) {
        spit(tmp, good.substr(0, n));
        EXPECT(load(tmp.c_str()) == HAF_E_IO);
    }
    for (int k = 0; k < 400; k++) {
        std::string s = good;
        s[lcg() % s.size()] ^= (char)(1u << (lcg() % 8));
        if (k % 3 == 0) s[lcg() % 12 % s.size()] = (char)lcg();                // (the header most of all)
        spit(tmp, s);
        (void)load(tmp.c_str());
    }
    remove(tmp.c_str());
    // null arguments
    {
        uint16_t *d = nullptr;
        int32_t w, h;
        EXPECT(haf_pgm16_load(nullptr, &d, &w, &h, nullptr, 0) == HAF_E_ARG);
        EXPECT(haf_pgm16_load(argv[1], nullptr, &w, &h, nullptr, 0) == HAF_E_ARG);
        EXPECT(haf_pgm16_load(tmp.c_str(), &d, &w, &h, nullptr, 0) == HAF_E_IO);   // (removed above; no buffer for the text)
        haf_frame f;
        haf_frame_default(&f);
        float p[3];
        EXPECT(haf_frame_points(nullptr, p) == HAF_E_ARG && haf_frame_points(&f, nullptr) == HAF_E_ARG && haf_frame_points(&f, p) == HAF_E_ARG);
        haf_frame_default(nullptr);
    }
    // frames: every kind on small and odd shapes, with and without row padding, the point strides of PCL
    const int shapes[][2] = {{1, 1}, {7, 3}, {61, 5}, {1, 9}, {17, 1}, {640, 48}};
    for (auto &s : shapes)
        for (size_t pad = 0; pad < 4; pad += 3) {
            run_frame(HAF_FRAME_DEPTH_U16, s[0], s[1], pad, 0, HAF_OK);
            run_frame(HAF_FRAME_DEPTH_F32, s[0], s[1], pad, 0, HAF_OK);
            for (size_t ps : {12, 16, 32}) run_frame(HAF_FRAME_XYZ_F32, s[0], s[1], pad, ps, HAF_OK);
        }
    run_frame(HAF_FRAME_XYZ_F32, 4, 3, 0, 8, HAF_E_ARG);
    run_frame(HAF_FRAME_XYZ_F32, 4, 3, 0, 14, HAF_E_ARG);
    run_frame(3, 4, 3, 0, 12, HAF_E_ARG);
    // refusals that must come before the first pixel is read: the data pointer of these frames is one byte long
    {
        unsigned char *one = (unsigned char *)malloc(1);
        float *out = (float *)malloc(12);
        haf_frame f;
        haf_frame_default(&f);
        f.data = one; f.kind = HAF_FRAME_DEPTH_U16; f.fx = f.fy = 500.0f;
        f.width = 65536; f.height = 32768; f.row_stride_bytes = 131072;
        EXPECT(haf_frame_points(&f, out) == HAF_E_CAPACITY);
        f.width = 4; f.height = 3; f.row_stride_bytes = 6;
        EXPECT(haf_frame_points(&f, out) == HAF_E_ARG);
        f.row_stride_bytes = 8; f.fx = 0.0f;
        EXPECT(haf_frame_points(&f, out) == HAF_E_ARG);
        f.fx = 500.0f; f.depth_scale = -1.0f;
        EXPECT(haf_frame_points(&f, out) == HAF_E_ARG);
        f.depth_scale = 0.001f; f.sensor_to_base[7] = NAN;
        EXPECT(haf_frame_points(&f, out) == HAF_E_ARG);
        f.sensor_to_base[7] = 0.0f; f.on_device = 1;
        EXPECT(haf_frame_points(&f, out) == HAF_E_ARG);
        free(out);
        free(one);
    }
    if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    printf("frame sanitizer job ok\n");
    return 0;
}
