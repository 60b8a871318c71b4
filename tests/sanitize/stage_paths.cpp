// stage_paths.cpp -- sanitizer driver of the sensor-frame staging code that needs no device (csrc/frame_stage.h; tests/test_frame_stage_cpu.py
// builds it with -fsanitize=address,undefined, host only): pack_rows and stage_rows over frames and masks of every kind, shape and stride
// against a byte-by-byte loop, unpack_rows into padded targets whose bytes between the rows must stay, the pieces stage_rows sends against
// the upload loop it replaced, describe_frame / staged_bytes / describe_image / describe_output and the label image an OutputDev hands
// back field by field, image_span / frame_span / label_span and spans_overlap at their edges, store_label / load_label round trips,
// check_label_image / check_output_image / check_label_output over one accepted case and every refusal, check_frame_batch over the
// refusals of tests/frame_cases.py.  Every source and destination is a heap block of EXACTLY the bytes
// the frame describes -- the last source row ends at its last kept element -- so one byte read or written past either is a report.
// argv: the file of refusal frames (records of {int32 code, int32 data: 0 null / 1 aligned / 2 misaligned by one, haf_frame}).
#include "../../haf_grasping_amd/csrc/frame_stage.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

using namespace haf;

static int failures = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static uint32_t lcg_state = 2024u;
static uint32_t lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }

typedef std::vector<std::pair<size_t, size_t>> Calls;      // (offset, bytes) of every send

// the bytes a source of these strides occupies when its last row ends at its last kept element
static size_t source_bytes(size_t h, size_t w, size_t elem_bytes, size_t elem_stride, size_t row_stride)
{
    return (h - 1) * row_stride + (w - 1) * elem_stride + elem_bytes;
}

// The upload loop of upload_frames as it stood before frame_stage.h (engine_request.cpp), restated: packs into host, records the copies
static Calls old_upload_loop(char *host, const haf_frame &f)
{
    constexpr size_t kPiece = 256 * 1024;
    Calls calls;
    const bool xyz = f.kind == HAF_FRAME_XYZ_F32;
    const size_t row_bytes = (size_t)f.width * frame_pixel_bytes(f.kind);
    size_t staged = 0, sent = 0;
    for (int v = 0; v < f.height; v++) {
        const char *row = static_cast<const char *>(f.data) + (size_t)v * f.row_stride_bytes;
        char *dst = host + staged;
        if (!xyz || f.point_stride_bytes == 12) memcpy(dst, row, row_bytes);
        else for (int u = 0; u < f.width; u++) memcpy(dst + (size_t)u * 12, row + (size_t)u * f.point_stride_bytes, 12);
        staged += row_bytes;
        if (staged - sent >= kPiece || v + 1 == f.height) {
            calls.emplace_back(sent, staged - sent);
            sent = staged;
        }
    }
    return calls;
}

// what every sequence of sends must satisfy: contiguous from 0, the packed length exactly, whole rows, only the last piece short
static void check_calls(const Calls &calls, size_t total, size_t row_bytes)
{
    size_t at = 0;
    for (size_t i = 0; i < calls.size(); i++) {
        EXPECT(calls[i].first == at && calls[i].second > 0);
        at += calls[i].second;
        EXPECT(at % row_bytes == 0);
        if (i + 1 < calls.size()) EXPECT(calls[i].second >= kStagePiece);
    }
    EXPECT(at == total && !calls.empty());
}

// one source through pack_rows and stage_rows into exactly sized blocks, against a byte-by-byte loop
static void run_pack(size_t h, size_t w, size_t elem_bytes, size_t elem_stride, size_t row_stride)
{
    const size_t src_bytes = source_bytes(h, w, elem_bytes, elem_stride, row_stride), total = h * w * elem_bytes;
    char *src = (char *)malloc(src_bytes), *want = (char *)malloc(total), *got = (char *)malloc(total), *got2 = (char *)malloc(total);
    for (size_t i = 0; i < src_bytes; i++) src[i] = (char)lcg();
    for (size_t v = 0; v < h; v++)
        for (size_t u = 0; u < w; u++)
            for (size_t k = 0; k < elem_bytes; k++) want[(v * w + u) * elem_bytes + k] = src[v * row_stride + u * elem_stride + k];
    memset(got, 0x5A, total);
    pack_rows(got, src, h, w, elem_bytes, elem_stride, row_stride);
    EXPECT(memcmp(got, want, total) == 0);
    memset(got2, 0x5A, total);
    Calls calls;
    size_t packed_at_send = 0;
    const int rc = stage_rows(got2, src, h, w, elem_bytes, elem_stride, row_stride, [&](size_t off, size_t bytes) {
        EXPECT(memcmp(got2 + off, want + off, bytes) == 0);          // what a piece names is packed when it is sent
        packed_at_send = off + bytes;
        calls.emplace_back(off, bytes);
        return 0;
    });
    EXPECT(rc == 0 && packed_at_send == total && memcmp(got2, want, total) == 0);
    check_calls(calls, total, w * elem_bytes);
    EXPECT(calls.size() == 1);                                       // (all of these are shorter than a piece)
    free(src); free(want); free(got); free(got2);
}

// packed rows through unpack_rows into a target of EXACTLY (h - 1) * stride + row_bytes bytes -- its last row ends at row_bytes, not at the
// stride -- against a byte-by-byte loop; the bytes between the rows are pre-filled and must be unchanged
static void run_unpack(size_t h, size_t w, size_t elem_bytes, size_t pad_bytes)
{
    const size_t row_bytes = w * elem_bytes, stride = row_bytes + pad_bytes, total = (h - 1) * stride + row_bytes;
    char *src = (char *)malloc(h * row_bytes), *want = (char *)malloc(total), *got = (char *)malloc(total);
    for (size_t i = 0; i < h * row_bytes; i++) src[i] = (char)lcg();
    for (size_t i = 0; i < total; i++) want[i] = got[i] = (char)(0xC3 ^ i);
    for (size_t v = 0; v < h; v++)
        for (size_t i = 0; i < row_bytes; i++) want[v * stride + i] = src[v * row_bytes + i];
    unpack_rows(got, stride, src, h, row_bytes);
    EXPECT(memcmp(got, want, total) == 0);
    // the inverse of pack_rows: packing the target again gives the source
    char *back = (char *)malloc(h * row_bytes);
    pack_rows(back, got, h, w, elem_bytes, elem_bytes, stride);
    EXPECT(memcmp(back, src, h * row_bytes) == 0);
    free(src); free(want); free(got); free(back);
}

// a side image (a mask, a label image) and an output image as the kernels get them, field by field
static void run_describe_images()
{
    char *image = (char *)malloc(16), *staged = (char *)malloc(16), *own = (char *)malloc(16);
    for (size_t eb : {1, 2}) {
        ImageDev d = describe_image(image, 0, 61 * eb + 7, 61, eb, staged);          // host: its packed copy
        EXPECT(d.src == staged && d.row_stride == 61 * eb);
        d = describe_image(image, 1, 61 * eb + 7, 61, eb, staged);                   // resident: where it lies, the caller's stride
        EXPECT(d.src == image && d.row_stride == 61 * eb + 7);
        for (int on_device = 0; on_device < 2; on_device++) {                        // no image: whatever the other fields say
            d = describe_image(nullptr, on_device, 61 * eb + 7, 61, eb, staged);
            EXPECT(d.src == nullptr && d.row_stride == 0);
        }
    }
    for (size_t eb : {1, 2, 4}) {
        const size_t stride = 61 * eb + 12;
        OutputDev o = describe_output(image, 0, stride, 61, eb, staged, own);        // host: written packed into the call's block
        EXPECT(o.dst == staged && o.dst_stride == 61 * eb && o.data == image && o.on_device == 0 && o.row_stride_bytes == stride);
        o = describe_output(image, 1, stride, 61, eb, staged, own);                  // the caller's device image, its stride
        EXPECT(o.dst == image && o.dst_stride == stride && o.data == image && o.on_device == 1 && o.row_stride_bytes == stride);
        o = describe_output(nullptr, 1, 0, 61, eb, staged, own);                     // the engine's own image, packed
        EXPECT(o.dst == own && o.dst_stride == 61 * eb && o.data == own && o.on_device == 1 && o.row_stride_bytes == 61 * eb);
    }
    for (int32_t eb : {1, 2}) {                                                      // the descriptor handed back, for the three residences
        const size_t stride = 61 * (size_t)eb + 12;
        haf_label_image l = describe_output(image, 0, stride, 61, (size_t)eb, staged, own).label_image(eb);
        EXPECT(l.data == image && l.elem_bytes == eb && l.on_device == 0 && l.row_stride_bytes == stride);
        l = describe_output(image, 1, stride, 61, (size_t)eb, staged, own).label_image(eb);
        EXPECT(l.data == image && l.elem_bytes == eb && l.on_device == 1 && l.row_stride_bytes == stride);
        l = describe_output(nullptr, 1, 0, 61, (size_t)eb, staged, own).label_image(eb);
        EXPECT(l.data == own && l.elem_bytes == eb && l.on_device == 1 && l.row_stride_bytes == 61 * (size_t)eb);
    }
    free(image); free(staged); free(own);
}

static haf_frame make_frame(int kind, int w, int h, size_t pad_elems, size_t point_stride, int on_device);

// the bytes an image and a frame span, and whether two spans share one
static void run_spans()
{
    char *block = (char *)malloc(8192);                                              // (only its addresses are used)
    // 5 rows of 61 uint16, packed: ends at its last element; the next byte starts the second image
    const size_t a_bytes = 4 * 122 + 122;
    ByteSpan a = image_span(block, 5, 122, 122);
    EXPECT(a.begin == (uintptr_t)block && a.end == a.begin + a_bytes);
    EXPECT(!spans_overlap(a, image_span(block + a_bytes, 5, 122, 122)) && !spans_overlap(image_span(block + a_bytes, 5, 122, 122), a));
    EXPECT(spans_overlap(a, image_span(block + a_bytes - 1, 5, 122, 122)) && spans_overlap(image_span(block + a_bytes - 1, 5, 122, 122), a));
    EXPECT(spans_overlap(a, a));
    // padded rows (stride 160): the span ends at the last element, not at height * stride, so an image inside the padding behind the
    // last row shares nothing with it; one inside the padding of an earlier row does
    a = image_span(block, 5, 160, 122);
    EXPECT(a.end == a.begin + 4 * 160 + 122);
    EXPECT(!spans_overlap(a, image_span(block + 4 * 160 + 122, 1, 38, 38)) && !spans_overlap(image_span(block + 4 * 160 + 122, 1, 38, 38), a));
    EXPECT(spans_overlap(a, image_span(block + 3 * 160 + 122, 1, 38, 38)));
    // height 1: the stride does not count
    a = image_span(block + 100, 1, 4000, 7);
    EXPECT(a.begin == (uintptr_t)block + 100 && a.end == a.begin + 7);
    EXPECT(!spans_overlap(a, image_span(block + 107, 1, 0, 1)) && spans_overlap(a, image_span(block + 106, 1, 0, 1)) && !spans_overlap(a, image_span(block, 1, 0, 100)));
    // frames: a depth row ends at its last sample; an XYZ frame 12 bytes into its last point whatever lies between two points
    haf_frame f = make_frame(HAF_FRAME_DEPTH_U16, 61, 5, 7, 0, 0);
    f.data = block;
    EXPECT(frame_span(f).begin == (uintptr_t)block && frame_span(f).end == (uintptr_t)block + 4 * (122 + 14) + 122);
    f = make_frame(HAF_FRAME_DEPTH_F32, 3, 1, 7, 0, 1);
    f.data = block;
    EXPECT(frame_span(f).end == (uintptr_t)block + 12);
    f = make_frame(HAF_FRAME_XYZ_F32, 61, 5, 2, 20, 0);
    f.data = block;
    a = frame_span(f);
    EXPECT(f.row_stride_bytes == 61 * 20 + 8 && a.end == a.begin + 4 * f.row_stride_bytes + 60 * 20 + 12);
    EXPECT(!spans_overlap(a, image_span((const char *)a.end, 1, 0, 8)) && spans_overlap(a, image_span((const char *)a.end - 1, 1, 0, 8)));
    // a label image's span
    const haf_label_image l = {block + 2, 2, 0, 20};
    a = label_span(l, 7, 3);
    EXPECT(a.begin == (uintptr_t)block + 2 && a.end == a.begin + 2 * 20 + 14);
    free(block);
}

// labels through store_label and load_label in a heap block of EXACTLY (h - 1) * stride + w * elem bytes; the bytes between the rows
// are pre-filled and must be unchanged
static void run_labels(size_t h, size_t w, int32_t elem, size_t pad_bytes)
{
    const size_t row_bytes = w * (size_t)elem, stride = row_bytes + pad_bytes, total = (h - 1) * stride + row_bytes;
    char *block = (char *)malloc(total);
    const uint32_t values[5] = {0, 1, 255, 256, 65535};
    const size_t n_values = elem == 1 ? 3 : 5;
    for (size_t first = 0; first < n_values; first++) {
        for (size_t i = 0; i < total; i++) block[i] = (char)(0xC3 ^ i);
        for (size_t v = 0; v < h; v++)
            for (size_t u = 0; u < w; u++) store_label(block, stride, elem, u, v, values[(first + v * w + u) % n_values]);
        const haf_label_image l = {block, elem, 0, stride};
        for (size_t v = 0; v < h; v++) {
            for (size_t u = 0; u < w; u++) {
                const uint32_t want = values[(first + v * w + u) % n_values];
                EXPECT(load_label(l, u, v) == want);
                if (elem == 1) EXPECT((uint8_t)block[v * stride + u] == want);
                else { uint16_t word; memcpy(&word, block + v * stride + u * 2, 2); EXPECT(word == want); }
            }
            for (size_t i = v * stride + row_bytes; v + 1 < h && i < (v + 1) * stride; i++) EXPECT(block[i] == (char)(0xC3 ^ i));
        }
    }
    free(block);
}

// check_label_image: one accepted image and every refusal of its list; check_output_image and check_label_output likewise
static void run_image_checks()
{
    char *block = (char *)malloc(8192);                                              // (only its addresses are used)
    std::string err;
    for (int32_t eb : {1, 2}) {
        const size_t row = 61 * (size_t)eb;
        const haf_label_image good = {block, eb, 0, row};                            // a stride of exactly a row
        EXPECT(check_label_image(&good, 61, 1, err) == HAF_OK && check_label_image(&good, 61, HAF_MAX_LABELS, err) == HAF_OK);
        haf_label_image l = good;
        l.on_device = 1; l.row_stride_bytes = row + 8;
        EXPECT(check_label_image(&l, 61, 7, err) == HAF_OK);
        const auto refused = [&](const haf_label_image *p, int32_t width, int32_t n_labels) {
            err.clear();
            return check_label_image(p, width, n_labels, err) == HAF_E_ARG && !err.empty();
        };
        EXPECT(refused(nullptr, 61, 1));
        l = good; l.data = nullptr; EXPECT(refused(&l, 61, 1));
        for (int32_t bad : {0, 3, 4, -1}) { l = good; l.elem_bytes = bad; l.row_stride_bytes = 1024; EXPECT(refused(&l, 61, 1)); }
        for (int32_t bad : {2, -1}) { l = good; l.on_device = bad; EXPECT(refused(&l, 61, 1)); }
        l = good; l.row_stride_bytes = row - 1; EXPECT(refused(&l, 61, 1));          // one byte short
        EXPECT(refused(&good, 62, 1));                                               // (the same image against a wider frame)
        EXPECT(refused(&good, 61, 0) && refused(&good, 61, HAF_MAX_LABELS + 1) && refused(&good, 61, -1));
        if (eb == 2) {
            l = good; l.row_stride_bytes = row + 1; EXPECT(refused(&l, 61, 1));      // no multiple of the element
            l = good; l.data = block + 1; EXPECT(refused(&l, 61, 1));                // misaligned
        }
    }
    for (size_t eb : {1, 2, 4}) {
        const size_t row = 61 * eb;
        EXPECT(check_output_image(block, 0, row, 61, eb, "out", err) == HAF_OK);     // a stride of exactly a row
        EXPECT(check_output_image(block, 1, row + 4 * eb, 61, eb, "out", err) == HAF_OK);
        EXPECT(check_output_image(nullptr, 1, 0, 61, eb, "out", err) == HAF_OK);     // the engine's own: nothing more is looked at
        const auto refused = [&](const void *out, int32_t on_device, size_t stride, const char *name) {
            err.clear();
            return check_output_image(out, on_device, stride, 61, eb, name, err) == HAF_E_ARG && !err.empty();
        };
        EXPECT(refused(block, 2, row, "out") && refused(block, -1, row, "out") && refused(nullptr, 2, row, "out"));
        EXPECT(refused(nullptr, 0, row, "labels") && err.find("labels") != std::string::npos);
        EXPECT(refused(block, 0, row - 1, "labels") && err.find("labels") != std::string::npos);
        EXPECT(refused(block, 1, row - 1, "out") && err.find("out") != std::string::npos);
        if (eb > 1) {
            EXPECT(refused(block, 0, row + 1, "out"));                               // no multiple of the element
            EXPECT(refused(block + 1, 0, row, "out") && refused(block + 1, 1, row, "out"));
        }
    }
    // a label output of a frame: the element size, check_output_image's list, and no byte shared with a frame of the same residence
    haf_frame f = make_frame(HAF_FRAME_XYZ_F32, 61, 5, 2, 20, 0);
    f.data = block;
    const ByteSpan fs = frame_span(f);
    char *behind = (char *)fs.end + (fs.end & 1);
    for (int32_t eb : {1, 2}) {
        const size_t row = 61 * (size_t)eb;
        EXPECT(check_label_output(f, behind, eb, row, 0, err) == HAF_OK && check_label_output(f, nullptr, eb, 0, 1, err) == HAF_OK);
        EXPECT(check_label_output(f, (char *)fs.end - eb, eb, row, 0, err) == HAF_E_ARG);        // the frame's last bytes
        EXPECT(check_label_output(f, (char *)fs.end - eb, eb, row, 1, err) == HAF_OK);           // (another residence: another memory)
        EXPECT(check_label_output(f, block, eb, row, 0, err) == HAF_E_ARG);
        EXPECT(check_label_output(f, behind, eb, row - 1, 0, err) == HAF_E_ARG && check_label_output(f, nullptr, eb, row, 0, err) == HAF_E_ARG);
        EXPECT(check_label_output(f, behind, eb, row, 2, err) == HAF_E_ARG);
    }
    for (int32_t bad : {0, 3, 4, -1}) EXPECT(check_label_output(f, behind, bad, 1024, 0, err) == HAF_E_ARG);
    free(block);
}

static haf_frame make_frame(int kind, int w, int h, size_t pad_elems, size_t point_stride, int on_device)
{
    haf_frame f;
    haf_frame_default(&f);
    const size_t elem = kind == HAF_FRAME_DEPTH_U16 ? 2 : kind == HAF_FRAME_DEPTH_F32 ? 4 : point_stride;
    f.kind = kind; f.width = w; f.height = h; f.on_device = on_device;
    f.row_stride_bytes = (size_t)w * elem + pad_elems * (kind == HAF_FRAME_XYZ_F32 ? 4 : elem);
    f.point_stride_bytes = kind == HAF_FRAME_XYZ_F32 ? point_stride : 0;
    f.fx = 525.0f; f.fy = -500.0f; f.cx = 0.5f * (float)w; f.cy = 0.25f * (float)h;
    f.depth_scale = 0.002f; f.min_depth = 0.3f; f.max_depth = 3.0f;
    const float t[12] = {0.36f, 0.48f, -0.8f, 0.1f, -0.8f, 0.6f, 0.0f, -0.2f, 0.48f, 0.64f, 0.6f, 0.9f};
    memcpy(f.sensor_to_base, t, sizeof t);
    return f;
}

// a host frame through stage_frame: the same bytes and the same copies as the loop it replaced; -> the copies
static Calls run_pieces(int kind, int w, int h, size_t pad_elems, size_t point_stride)
{
    haf_frame f = make_frame(kind, w, h, pad_elems, point_stride, 0);
    const size_t px = frame_pixel_bytes(kind), total = (size_t)w * h * px;
    const size_t src_bytes = source_bytes((size_t)h, (size_t)w, px, frame_elem_bytes(f), f.row_stride_bytes);
    char *src = (char *)malloc(src_bytes), *want = (char *)malloc(total), *got = (char *)malloc(total);
    for (size_t i = 0; i < src_bytes; i++) src[i] = (char)lcg();
    f.data = src;
    const Calls old = old_upload_loop(want, f);
    Calls calls;
    EXPECT(stage_frame(got, f, [&](size_t off, size_t bytes) { calls.emplace_back(off, bytes); return 0; }) == 0);
    EXPECT(calls == old && memcmp(got, want, total) == 0);
    check_calls(calls, total, (size_t)w * px);
    EXPECT(staged_bytes(f) == (total + 15) / 16 * 16);
    // a send that fails ends the staging with its code, at once
    int n_sends = 0;
    EXPECT(stage_frame(got, f, [&](size_t, size_t) { n_sends++; return -7; }) == -7 && n_sends == 1);
    free(src); free(want); free(got);
    return calls;
}

static void run_describe(int kind, size_t point_stride)
{
    const size_t px = kind == HAF_FRAME_DEPTH_U16 ? 2 : kind == HAF_FRAME_DEPTH_F32 ? 4 : 12;
    char *pixels = (char *)malloc(64), *area = (char *)malloc(64);
    for (int on_device = 0; on_device < 2; on_device++) {
        haf_frame f = make_frame(kind, 61, 5, 7, point_stride, on_device);
        f.data = pixels;
        const FrameDev fd = describe_frame(f, area);
        const haf_frame_math::FrameMath m = frame_math(f);
        EXPECT(fd.width == 61 && fd.n == 305 && fd.kind == kind && memcmp(&fd.m, &m, sizeof m) == 0);
        EXPECT(fd.dst == nullptr && fd.count == nullptr);
        if (on_device) {                                             // read where it lies, with the caller's strides
            EXPECT(fd.src == pixels && fd.row_stride == f.row_stride_bytes && fd.point_stride == (kind == HAF_FRAME_XYZ_F32 ? point_stride : px));
            EXPECT(staged_bytes(f) == 0);
        } else {                                                     // read where its packed rows were staged
            EXPECT(fd.src == area && fd.row_stride == 61 * px && fd.point_stride == px);
            EXPECT(staged_bytes(f) == (305 * px + 15) / 16 * 16);
        }
    }
    free(pixels); free(area);
}

static void run_batches(const char *refusal_file)
{
    char *block = (char *)malloc(64);
    haf_frame good = make_frame(HAF_FRAME_DEPTH_U16, 4, 3, 0, 0, 0);
    good.data = block;
    // the refusals of tests/frame_cases.py: alone, behind a good frame, and as the second view of a request
    FILE *fp = fopen(refusal_file, "rb");
    EXPECT(fp != nullptr);
    int n_refusals = 0;
    for (int32_t head[2]; fp && fread(head, sizeof head, 1, fp) == 1; n_refusals++) {
        haf_frame bad;
        EXPECT(fread(&bad, sizeof bad, 1, fp) == 1);
        bad.data = head[1] == 0 ? nullptr : head[1] == 1 ? block : block + 1;
        std::string own;
        EXPECT(check_frame(bad, own) == head[0] && !own.empty());
        const haf_frame two[2] = {good, bad};
        FrameBatch r = check_frame_batch(&bad, 1, nullptr, 1 << 20);
        EXPECT(r.code == head[0] && r.request == 0 && r.view == 0 && r.text == own);
        r = check_frame_batch(two, 2, nullptr, 1 << 20);
        EXPECT(r.code == head[0] && r.request == 1 && r.view == 0 && r.text == own);
        const int32_t views[1] = {2};
        r = check_frame_batch(two, 1, views, 1 << 20);
        EXPECT(r.code == head[0] && r.request == 0 && r.view == 1 && r.text == own);
    }
    if (fp) fclose(fp);
    EXPECT(n_refusals >= 60);
    // max_points: one frame over it, two frames over it only together, exactly at it
    const haf_frame two[2] = {good, good};
    FrameBatch r = check_frame_batch(two, 1, nullptr, 11);
    EXPECT(r.code == HAF_E_CAPACITY && r.request == 0 && r.view == 0 && r.text.empty());
    r = check_frame_batch(two, 2, nullptr, 23);
    EXPECT(r.code == HAF_E_CAPACITY && r.request == 1 && r.view == 0 && r.text.empty());
    r = check_frame_batch(two, 2, nullptr, 24);
    EXPECT(r.code == HAF_OK && r.clouds.size() == 2 && !r.host_xyz);
    // views 3 + 1: the upper bound of a request is the pixel sum of its views; its stand-in cloud points at the last of them
    haf_frame v[4] = {make_frame(HAF_FRAME_DEPTH_U16, 4, 3, 0, 0, 0), make_frame(HAF_FRAME_DEPTH_F32, 3, 2, 1, 0, 1),
                      make_frame(HAF_FRAME_XYZ_F32, 2, 1, 0, 16, 1), make_frame(HAF_FRAME_XYZ_F32, 5, 4, 2, 12, 0)};
    for (int i = 0; i < 4; i++) v[i].data = block + 16 * i;
    const int32_t views[2] = {3, 1};
    r = check_frame_batch(v, 2, views, 40);
    EXPECT(r.code == HAF_OK && r.clouds.size() == 2 && r.host_xyz);
    EXPECT(r.clouds[0].n_points == 12 + 6 + 2 && r.clouds[0].xyz == (const float *)v[2].data && r.clouds[0].stride_floats == 3 && r.clouds[0].on_device == 0);
    EXPECT(r.clouds[1].n_points == 20 && r.clouds[1].xyz == (const float *)v[3].data && r.clouds[1].stride_floats == 3 && r.clouds[1].on_device == 0);
    r = check_frame_batch(v, 2, views, 39);
    EXPECT(r.code == HAF_E_CAPACITY && r.request == 1 && r.view == 0 && r.text.empty());
    r = check_frame_batch(v, 1, views, 40);                          // (a device-resident XYZ view is not a host XYZ view)
    EXPECT(r.code == HAF_OK && !r.host_xyz && r.clouds.size() == 1);
    free(block);
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: stage_paths refusal_frames.bin\n"); return 2; }
    static_assert(up16(0) == 0 && up16(1) == 16 && up16(16) == 16 && up16(17) == 32 && kStagePiece == 256 * 1024, "frame_stage.h constants");
    for (size_t w : {1, 3, 61, 64})
        for (size_t h : {1, 5})
            for (size_t pad : {0, 7}) {
                run_pack(h, w, 2, 2, w * 2 + pad * 2);                                   // U16
                run_pack(h, w, 4, 4, w * 4 + pad * 4);                                   // F32
                for (size_t ps : {12, 16, 20}) run_pack(h, w, 12, ps, w * ps + pad * 4); // XYZ
                if (pad == 0) { run_pack(h, w, 1, 1, w); run_pack(h, w, 1, 1, w + 5); }  // masks
                for (size_t eb : {1, 2, 4}) run_unpack(h, w, eb, pad);                   // output images: labels, depth
                for (int kind : {HAF_FRAME_DEPTH_U16, HAF_FRAME_DEPTH_F32}) EXPECT(run_pieces(kind, (int)w, (int)h, pad, 0).size() == 1);
                for (size_t ps : {12, 16, 20}) EXPECT(run_pieces(HAF_FRAME_XYZ_F32, (int)w, (int)h, pad, ps).size() == 1);
            }
    // the pieces: one row under a piece, exactly a piece, one row over, and a 640 x 480 depth image
    Calls c = run_pieces(HAF_FRAME_DEPTH_U16, 64, 2047, 0, 0);
    EXPECT(c.size() == 1 && c[0].second == 262016);
    c = run_pieces(HAF_FRAME_DEPTH_U16, 64, 2048, 0, 0);
    EXPECT(c.size() == 1 && c[0].second == 262144);
    c = run_pieces(HAF_FRAME_DEPTH_U16, 64, 2049, 0, 0);
    EXPECT(c.size() == 2 && c[0].second == 262144 && c[1].second == 128);
    c = run_pieces(HAF_FRAME_DEPTH_U16, 640, 480, 3, 0);
    EXPECT(c.size() == 3 && c[0].second + c[1].second + c[2].second == 614400);
    c = run_pieces(HAF_FRAME_XYZ_F32, 200, 120, 2, 20);               // (the XYZ frame of tests/test_frame_stage_gpu.py)
    EXPECT(c.size() == 2 && c[0].second + c[1].second == 288000);
    run_describe(HAF_FRAME_DEPTH_U16, 0);
    run_describe(HAF_FRAME_DEPTH_F32, 0);
    run_describe(HAF_FRAME_XYZ_F32, 12);
    run_describe(HAF_FRAME_XYZ_F32, 20);
    run_describe_images();
    run_spans();
    for (size_t w : {1, 3, 61})
        for (size_t h : {1, 5})
            for (int32_t elem : {1, 2})
                for (size_t pad : {0, 7}) run_labels(h, w, elem, pad * (size_t)elem);
    run_image_checks();
    run_batches(argv[1]);
    if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    printf("stage sanitizer job ok\n");
    return 0;
}
