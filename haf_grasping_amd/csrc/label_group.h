// label_group.h -- the labels of a lane's group of pixels (frame_group.h), written once for the kernels that read an instance-label image
// by groups: graspmap.hip (k_map_labels), object_group.h (group_requests: k_roi_mark_objects, k_map_labels_objects) and labelshape.hip
// (k_label_shape).  Device code only.
#pragma once
#include "frame_group.h"

namespace haf {

// lab[k] = the label of pixel i0 + k of an image of n pixels, `width` to a row, LB bytes per label, rows label_stride bytes apart: one
// load of G * LB bytes (4, 8 or 16) where the group lies inside one row at an address aligned to that, element by element elsewhere.
// 0 for a pixel past the image's end and for a label above n_labels: ignored like background, before it indexes anything.  Bounds: a
// label is read for a pixel inside the image only
template <unsigned G, int LB>
__device__ __forceinline__ void group_labels(const void *__restrict__ labels, unsigned long long label_stride, unsigned width, unsigned n,
                                             unsigned i0, int n_labels, unsigned (&lab)[G])
{
    static_assert(G * LB == 4 || G * LB == 8 || G * LB == 16, "a group's labels are one load");
#pragma unroll
    for (unsigned k = 0; k < G; k++) lab[k] = 0u;
    if (i0 >= n) return;
    const unsigned v0 = i0 / width, u0 = i0 - v0 * width;
    const char *a = static_cast<const char *>(labels) + (size_t)v0 * label_stride + (size_t)u0 * LB;
    if (i0 + G <= n && u0 + G <= width && (reinterpret_cast<uintptr_t>(a) & (G * LB - 1u)) == 0) {
        unsigned w[G * LB / 4];                           // the group's labels in one load of G * LB bytes: inside one row
        if constexpr (G * LB == 16) { const v4u q = *as_global<const v4u>(a); w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w; }
        else if constexpr (G * LB == 8) { const v2u q = *as_global<const v2u>(a); w[0] = q.x; w[1] = q.y; }
        else w[0] = *as_global<const unsigned>(a);
#pragma unroll
        for (unsigned k = 0; k < G; k++) {
            if constexpr (LB == 2) lab[k] = (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
            else lab[k] = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
        }
    } else {
        unsigned u = u0, v = v0;
#pragma unroll
        for (unsigned k = 0; k < G; k++) {
            if (i0 + k < n) {                             // (v < height: inside the label image)
                const char *s = static_cast<const char *>(labels) + (size_t)v * label_stride + (size_t)u * LB;
                if constexpr (LB == 2) lab[k] = *as_global<const uint16_t>(s);
                else lab[k] = *as_global<const unsigned char>(s);
            }
            if (++u == width) { u = 0; v++; }
        }
    }
#pragma unroll
    for (unsigned k = 0; k < G; k++)
        if (lab[k] > (unsigned)n_labels) lab[k] = 0u;
}

}  // namespace haf
