// frame_stage.h -- a sensor frame (haf_frame) on its way to the device, without a device: its descriptor (FrameDev, frames.h), the packing
// of a host frame's or mask's rows into a pinned block and their upload in pieces, the checks of a batch before any device work; and the
// images that travel with it: where the kernels read a mask or a label image, where they write an output image and how its packed rows
// reach the caller's.  Every entry point that takes a haf_frame goes through here; engine_stage.cpp is the half that needs an engine.
// Needs neither HIP nor an engine: tests/sanitize/stage_paths.cpp drives it.
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
    void *data; int32_t on_device; size_t row_stride_bytes;     // the descriptor handed back
};
OutputDev describe_output(void *out, int out_on_device, size_t out_row_stride_bytes, size_t width, size_t elem_bytes, void *packed_at, void *own);

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
