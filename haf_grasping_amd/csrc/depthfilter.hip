// depthfilter.hip -- k_depth_filter<KIND, RADIUS>: 1..8 exposures of one depth camera -> one depth image (haf_filter_depth,
// include/hafgrasp.h).  The per-pixel rules are depth_filter.h's, the same source haf_filter_depth_ref runs on the host: the two agree
// word for word (tests/test_depth_filter_gpu.py).
//
// One workgroup of 256 lanes per 64 x 16 tile of the output, lanes along rows: lane t owns column t & 63 of rows (t >> 6) + 4 i, i < 4.
//   * stage T: a lane forms the lower median of its own four pixels -- the eight keys in registers, a fixed compare-exchange network,
//     the rank picked by compare-select (depth_filter.h: lower_median) -- keeps each M_p in a register for the store and writes its z as
//     fp32 into an LDS tile of (64 + 2 R) x (16 + 2 R) words.  The halo cells (516 at R = 3) are shared out over the lanes afterwards.
//     An invalid pixel and a pixel outside the image are a NaN there: as a neighbour it fails `<=` by itself;
//   * stage S: per neighbour one LDS read, one subtraction, one comparison, one addition;
//   * the counters: a ballot / popcount per wave, the waves' totals meet in LDS, one integer atomic per workgroup and counter.
// The exposures' descriptors are kernel arguments, indexed by constants only: scalar loads.  Halo and tile samples are single-sample
// loads -- the kernel moves a few bytes per pixel and is bound by its launch, so it is kept simple.
// Bounds: a sample is loaded and a pixel stored only inside the image; every LDS index is inside the tile by construction.
#include "frame_group.h"
#include "depth_filter.h"
#include "kernels.h"

namespace haf {

using namespace haf_depth_filter_math;

constexpr int kFiltTileW = 64, kFiltTileH = 16, kFiltThreads = 256;
constexpr int kFiltRowsPerLane = kFiltTileW * kFiltTileH / kFiltThreads;      // 4

// stage T of pixel (u, v): kInvalidKey outside the image
template <int KIND> __device__ __forceinline__ uint32_t stack_median(const DepthStackDev &d, int u, int v)
{
    if (u < 0 || v < 0 || u >= d.width || v >= d.height) return kInvalidKey;
    constexpr size_t E = KIND == HAF_FRAME_DEPTH_U16 ? 2 : 4;
    uint32_t k[kMaxStack];
#pragma unroll
    for (int j = 0; j < kMaxStack; j++) {
        k[j] = kInvalidKey;
        if (j < d.n_frames) {
            const char *s = static_cast<const char *>(d.src[j]) + (size_t)v * d.row_stride[j] + (size_t)u * E;
            if constexpr (KIND == HAF_FRAME_DEPTH_U16) k[j] = sample_key_u16(*as_global<const uint16_t>(s), d.m);
            else k[j] = sample_key_f32(*as_global<const unsigned>(s), d.m);
        }
    }
    return lower_median(k, d.min_valid);
}

template <int KIND> __device__ __forceinline__ float key_z(uint32_t key, const FrameMath &m)
{
    if constexpr (KIND == HAF_FRAME_DEPTH_U16) return key_z_u16(key, m);
    else return key_z_f32(key, m);
}

template <int KIND, int R>
__global__ __launch_bounds__(kFiltThreads) void k_depth_filter(const DepthStackDev d)
{
    constexpr int TW = kFiltTileW + 2 * R, TH = kFiltTileH + 2 * R;
    constexpr int kHalo = TW * TH - kFiltTileW * kFiltTileH, kBand = 2 * R * TW;      // the rows above and below come first, then the sides
    __shared__ float s_z[TH * TW];
    __shared__ unsigned s_cnt[kFiltThreads / 64][2];
    const int tiles_x = (d.width + kFiltTileW - 1) / kFiltTileW;
    const int u0 = (int)(blockIdx.x % (unsigned)tiles_x) * kFiltTileW, v0 = (int)(blockIdx.x / (unsigned)tiles_x) * kFiltTileH;
    const int lx = (int)(threadIdx.x & 63u), ly = (int)(threadIdx.x >> 6);

    uint32_t own[kFiltRowsPerLane];
#pragma unroll
    for (int i = 0; i < kFiltRowsPerLane; i++) {
        const int y = ly + 4 * i;
        own[i] = stack_median<KIND>(d, u0 + lx, v0 + y);
        s_z[(y + R) * TW + lx + R] = key_z<KIND>(own[i], d.m);
    }
    for (int h = (int)threadIdx.x; h < kHalo; h += kFiltThreads) {
        int tx, ty;
        if (h < kBand) {
            const int row = h / TW;
            tx = h - row * TW;
            ty = row < R ? row : row + kFiltTileH;
        } else {
            const int g = h - kBand, row = g / (2 * R), c = g - row * (2 * R);
            ty = R + row;
            tx = c < R ? c : c + kFiltTileW;
        }
        s_z[ty * TW + tx] = key_z<KIND>(stack_median<KIND>(d, u0 + tx - R, v0 + ty - R), d.m);
    }
    __syncthreads();

    const bool in_x = u0 + lx < d.width;
    unsigned n_valid = 0, n_kept = 0;                    // the wave's totals (uniform)
    constexpr size_t E = KIND == HAF_FRAME_DEPTH_U16 ? 2 : 4;
#pragma unroll
    for (int i = 0; i < kFiltRowsPerLane; i++) {
        const int y = ly + 4 * i;
        const bool inside = in_x && v0 + y < d.height, valid = own[i] != kInvalidKey;      // (outside the image own[i] is invalid)
        const float *c = s_z + (y + R) * TW + lx + R;
        const float zp = c[0], tp = support_tolerance(d.tol_abs, d.tol_rel, zp);
        int support = 0;
#pragma unroll
        for (int dy = -R; dy <= R; dy++)
#pragma unroll
            for (int dx = -R; dx <= R; dx++)
                if (dy != 0 || dx != 0) support += supports(c[dy * TW + dx], zp, tp) ? 1 : 0;
        const bool keep = valid && support >= d.min_support;
        n_valid += (unsigned)__popcll(__ballot(valid));
        n_kept += (unsigned)__popcll(__ballot(keep));
        if (inside) {
            char *o = static_cast<char *>(d.out) + (size_t)(v0 + y) * d.out_stride + (size_t)(u0 + lx) * E;
            if constexpr (KIND == HAF_FRAME_DEPTH_U16) *as_global<uint16_t>(o) = keep ? (uint16_t)own[i] : (uint16_t)0;
            else *as_global<unsigned>(o) = keep ? own[i] : kInvalidWord;
        }
    }
    if (lx == 0) { s_cnt[ly][0] = n_valid; s_cnt[ly][1] = n_kept; }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < kFiltThreads / 64; w++) total += s_cnt[w][threadIdx.x];
        if (total) atomicAdd(d.counters + threadIdx.x, total);
    }
}

template <int KIND> static void launch_kind(const DepthStackDev &d, int radius, unsigned tiles, hipStream_t s)
{
    const dim3 grid(tiles), block(kFiltThreads);
    if (radius == 1) hipLaunchKernelGGL((k_depth_filter<KIND, 1>), grid, block, 0, s, d);
    else if (radius == 2) hipLaunchKernelGGL((k_depth_filter<KIND, 2>), grid, block, 0, s, d);
    else hipLaunchKernelGGL((k_depth_filter<KIND, 3>), grid, block, 0, s, d);
}

void launch_depth_filter(const DepthStackDev &d, int kind, int radius, hipStream_t s)
{
    // (width * height < 2^31, so the tiles of the image are fewer than 2^31 / 64 + 2^31 / 16: they fit grid.x)
    const unsigned tiles = (unsigned)((d.width + kFiltTileW - 1) / kFiltTileW) * (unsigned)((d.height + kFiltTileH - 1) / kFiltTileH);
    if (kind == HAF_FRAME_DEPTH_U16) launch_kind<HAF_FRAME_DEPTH_U16>(d, radius, tiles, s);
    else launch_kind<HAF_FRAME_DEPTH_F32>(d, radius, tiles, s);
}

}  // namespace haf
