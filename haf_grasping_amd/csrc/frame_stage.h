// frame_stage.h -- a sensor frame (haf_frame) on its way to the device, without a device: its descriptor (FrameDev, frames.h), the packing
// of a host frame's or mask's rows into a pinned block and their upload in pieces, the checks of a batch before any device work; and the
// images that travel with it: where the kernels read a mask or a label image, where they write an output image and how its packed rows
// reach the caller's; THE refusals of an input label image (check_label_image) and of an output image (check_output_image,
// check_label_output), the bytes an image or a frame spans and whether two spans overlap, and one label of a host image read or written
// (load_label, store_label).  Every entry point that takes a haf_frame goes through here; engine_stage.cpp is the half that needs an
// engine.  Needs neither HIP nor an engine: tests/sanitize/stage_paths.cpp drives it.
#pragma once
#include "frames.h"

#include <cstring>
#include <vector>

namespace haf {

constexpr size_t up16(size_t x) { return (x + 15) / 16 * 16; }      // every staged frame, mask and header array starts at a multiple of 16 bytes
constexpr size_t kStagePiece = 256 * 1024;                          // packed bytes per upload: the DMA engine moves one piece while the host packs the next

// the descriptor of a checked frame, dst and count left null for the caller: a device-resident frame is read where it lies, with the
// caller's strides; a host frame at staged_at, where its rows lie packed (pack_rows)
FrameDev describe_frame(const haf_frame &f, const void *staged_at);
// what a host frame takes of its staging area, the 16-byte alignment of the next one included; 0 for a device-resident frame
size_t staged_bytes(const haf_frame &f);

// height rows of width elements (elem_stride bytes apart, rows row_stride bytes apart) to dst, packed: of every element its first
// elem_bytes bytes.  Reads (width - 1) * elem_stride + elem_bytes bytes of a source row and no more: the caller's last row may end there
void pack_rows(char *dst, const char *src, size_t height, size_t width, size_t elem_bytes, size_t elem_stride, size_t row_stride);

// the inverse, for an output image: writes exactly row_bytes per row and nothing between the rows: the caller's last row may end there
void unpack_rows(char *dst, size_t dst_row_stride, const char *src_packed, size_t height, size_t row_bytes);

// a side image of a frame `width` pixels wide (a haf_roi's mask, a haf_label_image) as the kernels read it: a device-resident one where it
// lies, with the caller's stride; a host one at staged_at, where its rows lie packed; no image (data == nullptr): null and 0
struct ImageDev { const void *src; unsigned long long row_stride; };
ImageDev describe_image(const void *data, int on_device, size_t row_stride_bytes, size_t width, size_t elem_bytes, const void *staged_at);

// an output image `width` elements wide: a host one (out_on_device == 0) is written packed at packed_at, inside the block the call copies
// back, and unpack_rows takes it to `out`; the caller's device image where it lies; without one (out == nullptr) the engine's own, packed
struct OutputDev {
    void *dst; unsigned long long dst_stride;                   // the kernel's
    void *data; int32_t on_device; size_t row_stride_bytes;     // the descriptor handed back: a haf_frame's own three fields, or
    haf_label_image label_image(int32_t elem_bytes) const { return {data, elem_bytes, on_device, row_stride_bytes}; }
};
OutputDev describe_output(void *out, int out_on_device, size_t out_row_stride_bytes, size_t width, size_t elem_bytes, void *packed_at, void *own);

// the bytes [begin, end) of an image: its last row ends at its last element, last_row_bytes into it, not at the stride; of a checked
// frame: an XYZ frame's last pixel is 12 bytes whatever lies between two points; of a label image; and whether two of them share a byte
struct ByteSpan { uintptr_t begin, end; };
inline ByteSpan image_span(const void *data, size_t height, size_t row_stride, size_t last_row_bytes)
{
    const uintptr_t begin = reinterpret_cast<uintptr_t>(data);
    return {begin, begin + (height - 1) * row_stride + last_row_bytes};
}
inline ByteSpan frame_span(const haf_frame &f) { return image_span(f.data, (size_t)f.height, f.row_stride_bytes, (size_t)(f.width - 1) * frame_elem_bytes(f) + frame_pixel_bytes(f.kind)); }
inline ByteSpan label_span(const haf_label_image &l, int32_t width, int32_t height) { return image_span(l.data, (size_t)height, l.row_stride_bytes, (size_t)width * (size_t)l.elem_bytes); }
inline bool spans_overlap(ByteSpan a, ByteSpan b) { return a.begin < b.end && b.begin < a.end; }

// The three checks below are inline: every *_host.cpp unit applies them, and each is built alone with frames_host.cpp by its sanitizer job.
// THE refusals, all HAF_E_ARG, of an input label image and its n_labels.  width: the frame's, or for haf_transfer_labels the CAMERA's
inline int check_label_image(const haf_label_image *l, int32_t width, int32_t n_labels, std::string &err)
{
    if (!l || !l->data) { err = "null label image or label data"; return HAF_E_ARG; }
    if (l->elem_bytes != 1 && l->elem_bytes != 2) { err = "label elem_bytes must be 1 or 2"; return HAF_E_ARG; }
    if (l->on_device != 0 && l->on_device != 1) { err = "label on_device must be 0 (host) or 1 (device)"; return HAF_E_ARG; }
    const size_t eb = (size_t)l->elem_bytes;
    if (l->row_stride_bytes < (size_t)(width > 0 ? width : 0) * eb || l->row_stride_bytes % eb != 0) { err = "label row stride too small or misaligned"; return HAF_E_ARG; }
    if (reinterpret_cast<uintptr_t>(l->data) % eb != 0) { err = "label data not aligned to its element"; return HAF_E_ARG; }
    if (n_labels < 1 || n_labels > HAF_MAX_LABELS) { err = "n_labels outside 1..HAF_MAX_LABELS"; return HAF_E_ARG; }
    return HAF_OK;
}
// ... of an output image `width` elements wide; `name`: the argument's, for the text.  What it may not overlap is the caller's to say
inline int check_output_image(const void *out, int32_t out_on_device, size_t row_stride_bytes, int32_t width, size_t elem_bytes, const char *name, std::string &err)
{
    const std::string n = name;
    if (out_on_device != 0 && out_on_device != 1) { err = "out_on_device must be 0 (host) or 1 (device)"; return HAF_E_ARG; }
    if (!out) {
        if (out_on_device == 0) { err = "null " + n + " in host memory"; return HAF_E_ARG; }
        return HAF_OK;                                    // (the engine's own image: packed)
    }
    if (row_stride_bytes < (size_t)width * elem_bytes) { err = "row stride of " + n + " smaller than a row"; return HAF_E_ARG; }
    if (row_stride_bytes % elem_bytes != 0) { err = "row stride of " + n + " is not a multiple of the element size"; return HAF_E_ARG; }
    if (reinterpret_cast<uintptr_t>(out) % elem_bytes != 0) { err = n + " is not aligned to its element size"; return HAF_E_ARG; }
    return HAF_OK;
}
// ... of a label output for a checked frame: its element size, check_output_image's, a byte shared with a frame of its residence
inline int check_label_output(const haf_frame &frame, const void *labels, int32_t elem_bytes, size_t row_stride_bytes, int32_t out_on_device, std::string &err)
{
    if (elem_bytes != 1 && elem_bytes != 2) { err = "elem_bytes must be 1 or 2"; return HAF_E_ARG; }
    const size_t elem = (size_t)elem_bytes;
    if (check_output_image(labels, out_on_device, row_stride_bytes, frame.width, elem, "labels", err) != HAF_OK) return HAF_E_ARG;
    if (!labels || frame.on_device != out_on_device) return HAF_OK;
    if (!spans_overlap(image_span(labels, (size_t)frame.height, row_stride_bytes, (size_t)frame.width * elem), frame_span(frame))) return HAF_OK;
    err = "labels overlaps the frame";
    return HAF_E_ARG;
}

// one label of a host image: uint8, or uint16 in host byte order
inline uint32_t load_label(const haf_label_image &l, size_t u, size_t v)
{
    const char *at = static_cast<const char *>(l.data) + v * l.row_stride_bytes + u * (size_t)l.elem_bytes;
    if (l.elem_bytes == 1) return *reinterpret_cast<const uint8_t *>(at);
    uint16_t w;
    memcpy(&w, at, 2);
    return w;
}
inline void store_label(void *labels, size_t row_stride_bytes, int32_t elem_bytes, size_t u, size_t v, uint32_t l)
{
    char *at = static_cast<char *>(labels) + v * row_stride_bytes + u * (size_t)elem_bytes;
    if (elem_bytes == 1) { const uint8_t b = (uint8_t)l; memcpy(at, &b, 1); }
    else { const uint16_t w = (uint16_t)l; memcpy(at, &w, 2); }
}

// pack_rows row after row, with send(offset into dst, bytes) whenever at least kStagePiece packed bytes are unsent and after the last
// row: every piece ends at a row's end.  Stops at the first send that does not return 0 and returns what it returned (an int, a hipError_t)
template <class Send>
auto stage_rows(char *dst, const char *src, size_t height, size_t width, size_t elem_bytes, size_t elem_stride, size_t row_stride, const Send &send)
    -> decltype(send(size_t(), size_t()))
{
    const size_t row_bytes = width * elem_bytes;
    size_t staged = 0, sent = 0;
    for (size_t v = 0; v < height; v++) {
        pack_rows(dst + staged, src + v * row_stride, 1, width, elem_bytes, elem_stride, row_stride);
        staged += row_bytes;
        if (staged - sent >= kStagePiece || v + 1 == height) {
            const auto rc = send(sent, staged - sent);
            if (rc != 0) return rc;
            sent = staged;
        }
    }
    return {};
}
// a host frame's pixels: 2 / 4 bytes of a depth sample, the three floats of an XYZ point
template <class Send> auto stage_frame(char *dst, const haf_frame &f, const Send &send) -> decltype(send(size_t(), size_t()))
{
    return stage_rows(dst, static_cast<const char *>(f.data), (size_t)f.height, (size_t)f.width, frame_pixel_bytes(f.kind), frame_elem_bytes(f),
                      f.row_stride_bytes, send);
}

// The frames of a batch before any device work: request b has views_per_request[b] consecutive frames (null: one each).  Every frame
// through check_frame, the running pixel total against max_points
struct FrameBatch {
    int code = HAF_OK;                // HAF_OK, or the refusal of the frame at ...
    int request = 0, view = 0;        // ... this place, with
    std::string text;                 // check_frame's text; empty: the pixels up to and including this frame are more than max_points
    bool host_xyz = false;            // a host XYZ frame is among them
    // per request {the last view's data, its pixels, 3, 0}: the UPPER bound of its points; on_device = 0 reserves their place in the points area; xyz is never read
    std::vector<haf_cloud> clouds;
};
FrameBatch check_frame_batch(const haf_frame *frames, int32_t n, const int32_t *views_per_request, int64_t max_points);

}  // namespace haf
