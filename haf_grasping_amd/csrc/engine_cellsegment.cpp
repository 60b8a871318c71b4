// engine_cellsegment.cpp -- haf_segment_cells (include/hafgrasp.h): one sensor frame of any shape -> an image of object labels by
// top-down cell clustering, on the device.  Every refusal comes before any device work (check_cell_segment of cellsegment_host.cpp, then
// the capacity); then the frame goes through the single-frame input of engine_stage.cpp, the nine launches of cellsegment.hip run on the
// engine's stream, ONE copy brings back the counters and the per-label tables -- and, behind them, a host `labels` image and the
// top-down grid when they were asked for -- and ONE synchronisation ends the call.  Nothing of the last scored batch is read or
// written: the stage timings are not touched; the block and the scratch are the ones every such call shares (call_io, call_scratch);
// the engine's own label image is haf_segment_frame's.
#include "engine_state.h"

namespace haf_host {

namespace {

constexpr size_t kCellCounterBytes = CELL_CNT_WORDS * sizeof(unsigned);
constexpr size_t kCellTableBytes = 7 * sizeof(int32_t);           // k_segment_number's entry: points, anchor, box
constexpr size_t kCellExtraBytes = 2 * sizeof(uint32_t);          // k_cell_table's: cells, largest top
static_assert(sizeof(haf_cell_segment_info) == 36 && kCellCounterBytes % 16 == 0, "the layout the copy-back block is read by");

int segment_cells_impl(haf_engine *e, const haf_frame *frame, const haf_cell_segment_params *p, void *labels, int32_t elem_bytes,
                       size_t row_stride_bytes, int32_t out_on_device, haf_label_image *out_image, uint16_t *cell_labels,
                       haf_cell_segment_info *info, int32_t *n_labels, int64_t *stats)
{
    using namespace haf_shape_math;
    const std::string who = "haf_segment_cells: ";
    std::string why;
    int rc;
    if ((rc = check_cell_segment(frame, p, labels, elem_bytes, row_stride_bytes, out_on_device, n_labels, why)) != HAF_OK) return fail(e, rc, who + why);
    const haf_frame &f = *frame;
    const size_t px = (size_t)f.width * (size_t)f.height, elem = (size_t)elem_bytes, nc = (size_t)p->nx * (size_t)p->ny;
    const size_t nl = (size_t)p->max_labels;
    const bool host_out = out_on_device == 0;
    StageBuf *in = nullptr;
    if ((rc = frame_input_prepare(e, f, who, &in)) != HAF_OK) return rc;
    // the scratch: [a cell word per pixel, whole 16-byte pieces: k_cell_bin stores them so][count][top][parent][size: a word per cell
    // each][the scan's block totals]; px4 words keep everything behind the cell words at a multiple of 16 bytes
    const size_t px4 = (px + 3) / 4 * 4;
    // the copy-back block of this call: [counters][cells and top per label][table entries][a host output image, packed][the top-down grid]
    const size_t extra_at = kCellCounterBytes, tab_at = up16(extra_at + nl * kCellExtraBytes), img_at = up16(tab_at + nl * kCellTableBytes);
    const size_t grid_at = up16(img_at + (host_out ? px * elem : 0)), end_at = grid_at + (cell_labels ? nc * 2 : 0);
    CallBuffers cb;
    if ((rc = call_buffers(e, who, end_at, "the copy-back block", (px4 + 4 * nc + segment_scan_blocks(nc)) * sizeof(int), "the cell words", &cb)) != HAF_OK) return rc;
    const hipStream_t s = cb.stream;
    char *const dev = cb.dev, *const host = cb.host;
    OutputDev o;
    if ((rc = label_output_prepare(e, f, labels, elem_bytes, row_stride_bytes, out_on_device, dev + img_at, who, &o)) != HAF_OK) return rc;

    CellSegDev d;
    memset(&d, 0, sizeof d);
    if ((rc = frame_input_upload(e, f, *in, s, &d.f)) != HAF_OK) return rc;
    d.r = cell_rules(*p);
    d.min_points = p->min_points; d.max_labels = p->max_labels;
    d.cell = reinterpret_cast<int *>(cb.scratch);
    d.count = reinterpret_cast<unsigned *>(d.cell + px4);
    d.top = d.count + nc;
    d.parent = reinterpret_cast<int *>(d.top + nc);
    d.size = d.parent + nc;
    d.totals = d.size + nc;
    d.counters = reinterpret_cast<unsigned *>(dev);
    d.extra = reinterpret_cast<unsigned *>(dev + extra_at);
    d.table = reinterpret_cast<int *>(dev + tab_at);
    d.cell_labels = cell_labels ? reinterpret_cast<uint16_t *>(dev + grid_at) : nullptr;
    d.out = o.dst; d.out_stride = o.dst_stride;
    d.elem_bytes = elem_bytes;
    HIPCHK(e, hipMemsetAsync(dev, 0, tab_at, s));                                     // the counters, and every label's cells and top
    HIPCHK(e, hipMemsetAsync(d.count, 0, 2 * nc * sizeof(unsigned), s));            // every cell's count and top
    launch_cell_segment(d, s);
    if ((rc = call_finish(e, cb, cell_labels ? end_at : img_at + (host_out ? px * elem : 0))) != HAF_OK) return rc;
    label_output_finish(o, f, elem_bytes, host + img_at, out_image);
    if (cell_labels) memcpy(cell_labels, host + grid_at, nc * 2);
    unsigned cnt[CELL_CNT_WORDS];
    memcpy(cnt, host, sizeof cnt);
    const int32_t n = (int32_t)std::min<unsigned>(cnt[CELL_CNT_KEPT], (unsigned)p->max_labels);
    *n_labels = n;
    for (int32_t l = 0; info && l < n; l++) {
        int32_t t[7];
        uint32_t x[2];
        memcpy(t, host + tab_at + (size_t)l * kCellTableBytes, sizeof t);
        memcpy(x, host + extra_at + (size_t)l * kCellExtraBytes, sizeof x);
        haf_cell_segment_info &i = info[l];
        i.n_points = t[0]; i.n_cells = (int32_t)x[0];
        i.anchor_ix = t[1]; i.anchor_iy = t[2]; i.ix_min = t[3]; i.iy_min = t[4]; i.ix_max = t[5]; i.iy_max = t[6];
        i.top = key_height(shape_dec(x[1]));
    }
    if (stats) {
        stats[0] = (int64_t)px; stats[1] = (int64_t)cnt[CELL_CNT_FG]; stats[2] = (int64_t)cnt[CELL_CNT_OUTSIDE];
        stats[3] = (int64_t)cnt[CELL_CNT_OCCUPIED]; stats[4] = (int64_t)cnt[CELL_CNT_COMPS]; stats[5] = (int64_t)cnt[CELL_CNT_KEPT];
    }
    return HAF_OK;
}

}  // namespace

}  // namespace haf_host

extern "C" {

int haf_segment_cells(haf_engine *e, const haf_frame *frame, const haf_cell_segment_params *p, void *labels, int32_t elem_bytes,
                      size_t row_stride_bytes, int32_t out_on_device, haf_label_image *out_image, uint16_t *cell_labels,
                      haf_cell_segment_info *info, int32_t *n_labels, int64_t *stats)
{
    if (!e) return HAF_E_ARG;
    return guarded(&e->error, [&] {
        return segment_cells_impl(e, frame, p, labels, elem_bytes, row_stride_bytes, out_on_device, out_image, cell_labels, info, n_labels, stats);
    });
}

}  // extern "C"
