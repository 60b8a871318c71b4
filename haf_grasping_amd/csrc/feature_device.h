// feature_device.h -- one feature value / one scaled attribute from the 15x15 integral window: the device functions shared by the
// feature kernels (features.hip) and the exact re-evaluation kernels (recheck.hip).
//   CIntImage_to_Featurevec::calc_featurevalue (fv.cpp:141-199), the "%.4g" text round trip (fv.cpp:133 -> svm-scale.c:270),
//   svm-scale restore+output (svm-scale.c:333-353) and the "%g" round trip (svm-scale.c:350 -> svm-predict.c:108)
#pragma once
#include "device_common.h"

namespace haf {

// ---------------------------------------------------------------------------------------------------
// a5/a6: one feature value from the 15x15 integral window (fv.cpp:141-199).  fp32, strict order, unfused.
// ---------------------------------------------------------------------------------------------------
// Integral-image reads go through a buffer descriptor: address = descriptor base + 32-bit VGPR byte offset (the window
// origin of the lane's cell) + SGPR byte offset (the region corner from the wave-uniform feature descriptor), i.e.
// `buffer_load_dword v, v_off, s[rsrc], s_off offen` with NO vector address arithmetic per load.  UNI = false (feature
// index differs per lane: recheck kernels) folds the corner offset into the VGPR instead.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t make_ii_rsrc(const float *ii, Dims d)
{
    const unsigned bytes = (unsigned)d.B * (unsigned)d.R * (unsigned)((d.H + 1) * (d.W + 1)) * 4u;   // < 2^32, checked in haf_create
    return __builtin_amdgcn_make_buffer_rsrc((void *)ii, 0, (int)bytes, 0x00020000);
}

template <bool UNI>
__device__ __forceinline__ float ii_load(rsrc_t r, unsigned w0b, int off)
{
    if (UNI) return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)w0b, off * 4, 0));
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)(w0b + (unsigned)off * 4u), 0, 0));
}

// Where the corners of a feature's regions come from: the integral image through the buffer descriptor (corner offset in
// an SGPR when the feature is wave-uniform, UNI, else folded into the VGPR), or a copy of the evaluation's 15x15 window in
// LDS (k_features).  Same values, same arithmetic.
template <bool UNI>
struct SrcBuf {
    rsrc_t r;
    unsigned w0b;
    template <class FD>
    __device__ __forceinline__ float corner(const FD &f, int k, int j) const { return ii_load<UNI>(r, w0b, f.off[k][j]); }
};
struct SrcWin {
    const float *win;             // this lane's window, row pitch 15
    template <class FD>
    __device__ __forceinline__ float corner(const FD &f, int k, int j) const { return win[f.offw[k][j]]; }
};

// LDS forms of a descriptor for the workgroups whose lanes take DIFFERENT attributes (k_features_small, k_small_direct: the attribute
// index differs between the quarters of a wave, so the descriptor words are vector loads).  Read from global memory where they are
// needed they were seven dependent round trips per attribute -- corner offsets, weight, the next region's, the scaling constants --
// and those round trips, not the arithmetic, were the kernels' time (round 5: k_small_direct 35 us for 4 072 evaluations).  The
// workgroup copies what its mode reads once; window offsets fit a byte (15 x 15 - 1 = 224).  Same members, same values.
struct FeatDescX {                // exact attributes (attribute_value_rec): 64 bytes
    unsigned char offw[3][4];
    unsigned char active, shaf, skip, pad;
    float w[3];
    float pad1;
    double fmin, fmax, range, inv_range;
};
struct FeatDescS {                // screening attributes (screen_attribute): 48 bytes
    unsigned char offw[3][4];
    unsigned char active, shaf, skip, pad;
    float w[3];
    float scr_extra;
    double scr_mul, scr_add;
};
template <int THREADS>
__device__ __forceinline__ void stage_descriptors(const FeatDesc *__restrict__ fd, int n, FeatDescX *s_fd)
{
    for (int f = threadIdx.x; f < n; f += THREADS) {
        const FeatDesc &F = fd[f];
        FeatDescX L;
#pragma unroll
        for (int k = 0; k < 3; k++) {
#pragma unroll
            for (int j = 0; j < 4; j++) L.offw[k][j] = (unsigned char)F.offw[k][j];
            L.w[k] = F.w[k];
        }
        L.active = (unsigned char)F.active; L.shaf = F.shaf ? 1 : 0; L.skip = F.skip ? 1 : 0; L.pad = 0; L.pad1 = 0.0f;
        L.fmin = F.fmin; L.fmax = F.fmax; L.range = F.range; L.inv_range = F.inv_range;
        s_fd[f] = L;
    }
}
template <int THREADS>
__device__ __forceinline__ void stage_descriptors(const FeatDesc *__restrict__ fd, int n, FeatDescS *s_fd)
{
    for (int f = threadIdx.x; f < n; f += THREADS) {
        const FeatDesc &F = fd[f];
        FeatDescS L;
#pragma unroll
        for (int k = 0; k < 3; k++) {
#pragma unroll
            for (int j = 0; j < 4; j++) L.offw[k][j] = (unsigned char)F.offw[k][j];
            L.w[k] = F.w[k];
        }
        L.active = (unsigned char)F.active; L.shaf = F.shaf ? 1 : 0; L.skip = F.skip ? 1 : 0; L.pad = 0;
        L.scr_extra = F.scr_extra; L.scr_mul = F.scr_mul; L.scr_add = F.scr_add;
        s_fd[f] = L;
    }
}

template <class Src, class FD>
__device__ __forceinline__ float region_sum(const Src &src, const FD &f, int k)
{
    float s = __fsub_rn(src.corner(f, k, 0), src.corner(f, k, 1));
    s = __fsub_rn(s, src.corner(f, k, 2));
    return __fadd_rn(s, src.corner(f, k, 3));                            // fv.cpp:161-162 / 183-184
}

template <class Src, class FD>
__device__ __forceinline__ float feature_value(const Src &src, const FD &f)
{
    if (!f.shaf) {
        float rv = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; k++)
            if (f.active & (1 << k)) rv = __fadd_rn(rv, __fmul_rn(f.w[k], region_sum(src, f, k)));
        return rv;
    }
    float r[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (f.active & (1 << k)) r[k] = __fmul_rn(f.w[k], region_sum(src, f, k));
    if (r[1] > r[0] && r[1] > r[2]) {                                    // fv.cpp:187-191
        float a = __fsub_rn(r[1], r[0]), b = __fsub_rn(r[1], r[2]);
        return (b < a) ? b : a;
    }
    return -1.0f;
}

// fp32 feature -> attribute value svm-predict would parse (both decimal text round trips emulated exactly)
template <class Src, class FD, class Tabs>
__device__ __forceinline__ double attribute_value(const Src &src, const FD &f, double lower, double upper, const Tabs &tb)
{
    float v = feature_value(src, f);
    double q4 = hafq::decq4_float(v, tb);
    return hafq::scale_q6(q4, f.fmin, f.fmax, f.range, f.inv_range, lower, upper, tb);
}

// The same, leaving the three stages of the attribute behind for haf_debug_fetch_attr (HAF_FLAG_KEEP_DEBUG): rec == nullptr in
// every production call.  An attribute svm-scale drops (f.skip) is 0 for the contraction; its feature and "%.4g" value are
// still what fv.cpp writes into the text file, so the record keeps them.
template <class Src, class FD, class Tabs>
__device__ __forceinline__ double attribute_value_rec(const Src &src, const FD &f, double lower, double upper, const Tabs &tb,
                                                      AttrRecord *rec)
{
    if (f.skip && !rec) return 0.0;
    const float v = feature_value(src, f);
    const double q4 = hafq::decq4_float(v, tb);
    const double x = f.skip ? 0.0 : hafq::scale_q6(q4, f.fmin, f.fmax, f.range, f.inv_range, lower, upper, tb);
    if (rec) { rec->feature = v; rec->pad = 0.0f; rec->q4 = q4; rec->scaled = x; }
    return x;
}

// Attribute for the SCREENING pass only, already multiplied by c (kernels.h: ScreenParams): the "%.4g" round trip through the
// table-driven decq4_float_scr, svm-scale's formula in plain fp64 with the constants folded on the host (u' = fma(q4,
// scr_mul, scr_add): one instruction with two scalar operands), and NO "%g" round trip.  With x the value svm-predict would parse and u = c x, the result u' satisfies
// |u' - u| <= 5e-6 |u'| (six significant decimal digits: half a unit of the sixth digit is <= 5e-6 relative) plus, in norm over
// the attributes, ScreenParams::eta_abs (engine.cpp: the fp64 roundings of both evaluations of the formula, the exact-zero
// omission and the min/max shortcuts).  screen_finish() carries that difference through the guard band; evaluations the
// screening pass cannot decide get the exact attributes in the three-pass tier.  An fp32 feature outside the decimal
// path's range comes back NaN and poisons the norms: that evaluation is never trusted.
// (round 5: + 3 u for the fp32 scaling -- fl32(q4), the product's and the sum's rounding inside the fma are one, the constants' own roundings --
// relative to |u'|; the part relative to |scr_add| is in eta_abs)
// (the constant itself: screen_finish.h, kScreenEtaRel = 5.0e-6 * (1.0 + 1e-6) + 1.8e-7)
template <class Src, class FD>
__device__ __forceinline__ float screen_attribute(const Src &src, const FD &f, const hafq::ScrTabs &st)
{
    const float v = feature_value(src, f);
    return fmaf((float)hafq::decq4_float_scr(v, st), (float)f.scr_mul, (float)f.scr_add);     // (the same floats ScrDesc holds: model_tables.cpp, describe_slot)
}

// The same with the low-rank form's noise bound (kernels.h: kLrK; features.hip: k_features_serial, LR) for a lane of a wave that is
// not a run of neighbours: nb >= |u' - u_lin| -- the "%.4g" rounding, the products' rounding errors (exact, by fma) and the sums'
// -- and, for a region whose sum is not provably EXACT in the reference's order ((a - b) - c) + d, the worst its three roundings can
// add (region_round_bound).  The exactness test, per region, for a grid without negative heights (monotone integral image, R >= 0):
// a - b by Sterbenz (a <= 2b) or b = 0; then s2 = s1 - c = R - d and s3 = R are multiples of ulp(d) below d when R < d
// (c = d = 0: nothing to round).  A SHAF slot (pad2 = 0) is passed through as it is and needs none.
// what the three roundings of ((a - b) - c) + d can add up to when the region does not pass the exactness test: u (|s1| + |s2| + |R|)
// (each operation is off by at most half an ulp of its own result) -- 0 when it passes.
// The test is LOCAL -- on the four corners and the computed sum alone, no assumption about the rest of the grid: a - b is exact by
// Sterbenz (b/2 <= a <= 2b) or with b = 0; a, b, c >= d >= 0 makes a, b, c and therefore s1 and s2 = s1 - c = R - d multiples of
// ulp(d), and 0 <= R < d keeps |s2| <= d and s3 = R below 2^24 ulp(d): representable.  (Were the arithmetic inexact the computed R
// could not pass 0 <= R < d with a true R outside: s2 = fl(s1 - c) keeps the sign of s1 - c.)
__device__ __forceinline__ float region_round_bound(float a, float b, float c, float d, float s1, float s2, float R)
{
    const bool e1 = (a <= 2.0f * b && b <= 2.0f * a) || b == 0.0f;
    const bool e2 = (c == 0.0f && d == 0.0f) || (d >= 0.0f && fminf(fminf(a, b), c) >= d && R >= 0.0f && R < d);
    return (e1 && e2) ? 0.0f : 6.1e-8f * (fabsf(s1) + fabsf(s2) + fabsf(R));
}
template <class Src>
__device__ __forceinline__ float screen_attribute_lr(const Src &src, const FeatDesc &f, const hafq::ScrTabs &st, float &nb)
{
    if (f.shaf) { nb = 0.0f; return screen_attribute(src, f, st); }
    float rv = 0.0f, ee = 0.0f, esum = 0.0f;
    bool first = true;
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (f.active & (1 << k)) {
            const float a = src.corner(f, k, 0), b = src.corner(f, k, 1), c = src.corner(f, k, 2), d = src.corner(f, k, 3);
            const float s1 = __fsub_rn(a, b), s2 = __fsub_rn(s1, c);
            const float R = __fadd_rn(s2, d);
            esum = fmaf(fabsf(f.w[k]), region_round_bound(a, b, c, d, s1, s2, R), esum);
            const float p = __fmul_rn(f.w[k], R);
            ee += fmaf(f.w[k], R, -p);
            rv = __fadd_rn(rv, p);
            if (!first) esum = fmaf(6.1e-8f, fabsf(rv), esum);           // (0 + p is exact; every later addition rounds its result once)
            first = false;
        }
    const float q4f = (float)hafq::decq4_float_scr(rv, st);
    nb = f.pad2 * (fabsf(q4f - rv) + fabsf(ee) * 1.000001f + esum + 6.1e-8f * fabsf(rv));
    return fmaf(q4f, (float)f.scr_mul, (float)f.scr_add);
}

// ---- the fast form of the screening feature pass ------------------------------------------------------------------
// What bounds the per-lane form (buffer loads at window origin + corner offset) is the vector L1: the texture addresser
// coalesces 16 lanes at a time, 64 consecutive floats at an arbitrary alignment cost ~7.5 tag accesses per load, and with
// ~2400 loads per evaluation the TA is 97 % busy (profiles/README.md).  So a wave whose 64 evaluations are 64 neighbouring
// cells of one row (k_scan's order makes that the rule) first copies the band of the integral image its windows cover --
// 15 rows x 78 columns -- into LDS, and then reads every corner with ds_read_addtid_b32: LDS address = M0 + lane * 4, M0 =
// band + corner offset from the wave-uniform descriptor, so a corner costs two scalar instructions and one conflict-free
// LDS read, no vector address arithmetic, no L1 traffic.
constexpr int kBandRows = 15;
constexpr int kBandFloats4 = kBandRows * kBandPitch;  // per wave

// The eight attribute slots of a "fast" group (ScreenParams::fast_groups: plain HAF features of at most two regions), two slots
// at a time (screen_group below), and nothing branches.  An inactive region has weight 0 and its corners at the window origin: it adds
// 0.0f * 0.0f, which leaves the sum of fv.cpp:164 as it is.
// hipcc does not know that the asm reads are asynchronous: the registers are handed on only through the s_waitcnt statements.
// The descriptors are read through the constant address space: the memory clobbers around the band would otherwise make
// hipcc fetch every wave-uniform descriptor word with a vector load.
typedef const ScrDesc __attribute__((address_space(4))) *ScrDescK;
__device__ __forceinline__ ScrDescK constant_ptr(const ScrDesc *p) { return (ScrDescK)(unsigned long long)p; }

// NB (low-rank form, kernels.h: kLrK): nb[q] >= |u' - u_lin| of the slot, u_lin the EXACTLY linear functional of the window behind
// the attribute -- the "%.4g" rounding |q4 - v| (formed in fp32: its cast costs another u |q4|) plus the fp32 roundings of the
// products and of their sum (<= 3.1 u sum|w_k R_k|), valid when the region sums themselves are exact (k_features_serial checks that
// per wave), times |scr_mul| (ScrDesc::pad, rounded up; 0 for a SHAF slot, which is passed through as it is).
// u = 2^-24: 3 u (1 + 1e-3) and 4 u (1 + 1e-3), rounded up (the fp32 roundings of the bound's own three operations included)
constexpr float kNbRound = 1.80e-7f, kNbRound3 = 2.40e-7f;
// The wait state between an SALU write of M0 and the add-TID read that uses it (a read issued directly behind the write would use the
// previous M0 and return wrong corners silently).  HAF_SLOT_PAD2: a timing probe that doubles every pad (build.py --variant).
#ifdef HAF_SLOT_PAD2
#define HAF_SLOT_PAD "s_nop 0\n\ts_nop 0\n\t"
#else
#define HAF_SLOT_PAD "s_nop 0\n\t"
#endif
#define HAF_CORNER_READ(dst, off, band) "s_add_i32 m0, %" #off ", %" #band "\n\t" HAF_SLOT_PAD "ds_read_addtid_b32 %" #dst "\n\t"
// The eight corner reads of one slot in ONE statement: M0 = band + corner offset is written by the add itself (no temporary, no move),
// and hipcc puts nothing between the reads (between two statements that clobber M0 it pads a wait state of its own).
template <class OffK>
__device__ __forceinline__ void corner_reads8(unsigned band, OffK off, float *c)
{
    asm volatile(HAF_CORNER_READ(0, 8, 16) HAF_CORNER_READ(1, 9, 16) HAF_CORNER_READ(2, 10, 16) HAF_CORNER_READ(3, 11, 16)
                 HAF_CORNER_READ(4, 12, 16) HAF_CORNER_READ(5, 13, 16) HAF_CORNER_READ(6, 14, 16) HAF_CORNER_READ(7, 15, 16)
                 : "=v"(c[0]), "=v"(c[1]), "=v"(c[2]), "=v"(c[3]), "=v"(c[4]), "=v"(c[5]), "=v"(c[6]), "=v"(c[7])
                 : "s"(off[0]), "s"(off[1]), "s"(off[2]), "s"(off[3]), "s"(off[4]), "s"(off[5]), "s"(off[6]), "s"(off[7]), "s"(band)
                 : "m0", "scc");
}
template <class OffK>
__device__ __forceinline__ void corner_reads4(unsigned band, OffK off, float *c)
{
    asm volatile(HAF_CORNER_READ(0, 4, 8) HAF_CORNER_READ(1, 5, 8) HAF_CORNER_READ(2, 6, 8) HAF_CORNER_READ(3, 7, 8)
                 : "=v"(c[0]), "=v"(c[1]), "=v"(c[2]), "=v"(c[3])
                 : "s"(off[0]), "s"(off[1]), "s"(off[2]), "s"(off[3]), "s"(band)
                 : "m0", "scc");
}
// ---- a fast group of eight slots as four PAIRS, software-pipelined three deep -------------------------------------------------------
// pair p + 2: its descriptor words are on their way (scalar loads issued by hand, so that nothing waits for them where they are issued);
// pair p + 1: its sixteen corner reads are in flight; pair p: its sums, products, "%.4g" lookups and bounds execute.  The one full wait
// of a pair (pair_wait) stands where everything older has long been drained by the lookups of the pair before, and the two lookups of a
// pair's slots are formed side by side, so that they share their two LDS round trips.  Round 6, at C5, A/B on one box: 3.19-3.21 -> 2.99-3.03 ms
// (profiles/r06_slot_loop_ab.txt).  What did NOT matter is the length of the instruction stream: doubling every pad of the old loop
// (64 more s_nop per group) cost 0.02 ms; one slot at a time with a counted wait (lgkmcnt(8)) for the slot in front reached 3.07 ms;
// six waves per SIMD 3.12 ms.  No operation on a value changed: tests/test_slot_loop_gpu.py holds the kernel to the bits it wrote before.
typedef int s_int8 __attribute__((ext_vector_type(8)));
typedef float s_float4 __attribute__((ext_vector_type(4)));
struct PairDesc { s_int8 off0, off1; s_float4 k0, k1; float pad0, pad1; };      // per slot: off[8], {w[0], w[1], scr_mul, scr_add}, pad
static_assert(offsetof(ScrDesc, off) == 0 && offsetof(ScrDesc, w) == 0x20 && offsetof(ScrDesc, scr_mul) == 0x28 && offsetof(ScrDesc, scr_add) == 0x2c &&
              offsetof(ScrDesc, pad) == 0x34 && sizeof(ScrDesc) == 0x40, "pair_desc_load reads ScrDesc by byte offsets");
// hipcc does not know that these loads are asynchronous: the registers are handed on only through pair_wait / desc_wait
__device__ __forceinline__ void pair_desc_load(ScrDescK sd, PairDesc &d)
{
    asm volatile("s_load_dwordx8 %0, %6, 0x0\n\ts_load_dwordx4 %2, %6, 0x20\n\ts_load_dword %4, %6, 0x34\n\t"
                 "s_load_dwordx8 %1, %6, 0x40\n\ts_load_dwordx4 %3, %6, 0x60\n\ts_load_dword %5, %6, 0x74"
                 : "=&s"(d.off0), "=&s"(d.off1), "=&s"(d.k0), "=&s"(d.k1), "=&s"(d.pad0), "=&s"(d.pad1) : "s"(sd));
}
__device__ __forceinline__ void desc_wait(PairDesc &d)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(d.off0), "+s"(d.off1), "+s"(d.k0), "+s"(d.k1), "+s"(d.pad0), "+s"(d.pad1));
}
// everything in flight has to be back: pair p's sixteen corners (c) and pair p + 1's descriptor words (d)
__device__ __forceinline__ void pair_wait(float *c, PairDesc &d)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7]),
                                          "+s"(d.off0), "+s"(d.off1), "+s"(d.k0), "+s"(d.k1), "+s"(d.pad0), "+s"(d.pad1));
    asm volatile("" : "+v"(c[8]), "+v"(c[9]), "+v"(c[10]), "+v"(c[11]), "+v"(c[12]), "+v"(c[13]), "+v"(c[14]), "+v"(c[15]));
}
__device__ __forceinline__ void pair_wait(float *c)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7]));
    asm volatile("" : "+v"(c[8]), "+v"(c[9]), "+v"(c[10]), "+v"(c[11]), "+v"(c[12]), "+v"(c[13]), "+v"(c[14]), "+v"(c[15]));
}
struct VecOff { s_int8 v; __device__ __forceinline__ int operator[](int j) const { return v[j]; } };
__device__ __forceinline__ void pair_reads(unsigned band, const PairDesc &d, float *c)
{
    corner_reads8(band, VecOff{d.off0}, c);
    corner_reads8(band, VecOff{d.off1}, c + 8);
}
template <int NB>
__device__ __forceinline__ void pair_math(const float *c, const PairDesc &d, const hafq::ScrTabs &st, float *ud, float &nu2, float &rmin)
{
    float ar[2] = {0.0f, 0.0f}, q4f[2];
    // the two slots side by side in the halves of packed fp32 instructions (v_pk_add_f32 / v_pk_mul_f32: the same IEEE operation per half)
    typedef float v2f __attribute__((ext_vector_type(2)));
    const v2f w0 = {d.k0[0], d.k1[0]}, w1 = {d.k0[1], d.k1[1]};
    const v2f c0 = {c[0], c[8]}, c1 = {c[1], c[9]}, c2 = {c[2], c[10]}, c3 = {c[3], c[11]}, c4 = {c[4], c[12]}, c5 = {c[5], c[13]}, c6 = {c[6], c[14]},
              c7 = {c[7], c[15]};
    const v2f s10 = c0 - c1, s20 = s10 - c2, s11 = c4 - c5, s21 = s11 - c6;
    const v2f R0 = s20 + c3, R1 = s21 + c7;
    const v2f r0 = w0 * R0, r1 = w1 * R1;
    const v2f v = r0 + r1;                  // 0.0f + r0 first (fv.cpp:164) only turns a -0 into +0: same decimal, same u'
    if (NB == 2)                            // a wave that did not pass the exactness test as a whole (features.hip)
#pragma unroll
        for (int i = 0; i < 2; i++)
            ar[i] = fabsf(w0[i]) * region_round_bound(c0[i], c1[i], c2[i], c3[i], s10[i], s20[i], R0[i]) +
                    fabsf(w1[i]) * region_round_bound(c4[i], c5[i], c6[i], c7[i], s11[i], s21[i], R1[i]);
#pragma unroll
    for (int i = 0; i < 2; i++) q4f[i] = (float)hafq::decq4_float_scr(v[i], st);
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const s_float4 k = i ? d.k1 : d.k0;
        ud[i] = fmaf(q4f[i], k[2], k[3]);
        if (NB) {
            // round 5: the fp32 roundings BOUNDED instead of measured -- two products (u |r_k| each), their sum (u |v|) and the cast of q4
            // (u |q4| <= 1.0005 u |v|), |v| <= (1 + u)(|r0| + |r1|): at most kNbRound (|r0| + |r1|), a thousandth of the "%.4g" term beside
            // it (|q4 - v| ~ 1e-4 |v|).  Six vector instructions per slot instead of eleven.
            float nbq = fmaf(kNbRound, fabsf(r0[i]) + fabsf(r1[i]), fabsf(q4f[i] - v[i]));
            if (NB == 2) nbq += ar[i];
            // path A (NB == 1, the wave passed the exactness test as a whole): that test takes R >= 0 from the monotone integral image, which
            // holds for the TRUE sums; the fp32-rounded corners can leave a near-empty region at -1..-3 ulp(d), and then (a - b) - c may have
            // rounded.  The smallest computed R of the evaluation rides along (one v_min3 per slot); a negative one voids the
            // evaluation's screening pass (features.hip)
            if (NB == 1) rmin = fminf(fminf(R0[i], R1[i]), rmin);
            nbq *= i ? d.pad1 : d.pad0;
            nu2 = fmaf(nbq, nbq, nu2);
        }
    }
    // (the sum is tied to the sequence of the volatile LDS reads: left to float, the temporaries of eight slots stay alive until the sums
    // are finally formed)
    if (NB) asm volatile("" : "+v"(nu2));
}
template <int NB>
__device__ __forceinline__ void screen_group(unsigned band, ScrDescK sd, const hafq::ScrTabs &st, float *ud, float &nu2, float &rmin)
{
    PairDesc d[3];
    float c[2][16];
    pair_desc_load(sd, d[0]);
    desc_wait(d[0]);
    pair_reads(band, d[0], c[0]);
    pair_desc_load(sd + 2, d[1]);
#pragma unroll
    for (int p = 0; p < 4; p++) {
        if (p < 3) {
            pair_wait(c[p & 1], d[(p + 1) % 3]);
            pair_reads(band, d[(p + 1) % 3], c[(p + 1) & 1]);
        } else {
            pair_wait(c[p & 1]);
        }
        if (p < 2) pair_desc_load(sd + 2 * (p + 2), d[(p + 2) % 3]);
        pair_math<NB>(c[p & 1], d[p % 3], st, ud + 2 * p, nu2, rmin);
    }
}
__device__ __forceinline__ void screen_group(unsigned band, ScrDescK sd, const hafq::ScrTabs &st, float *ud) { float dummy = 0.0f, dmin = 0.0f; screen_group<0>(band, sd, st, ud, dummy, dmin); }

// Two attribute slots of any other group, from the band: three regions each, the HAF sum or the SHAF rule (feature_value).
// A slot of a dropped or absent attribute has scr_mul = scr_add = 0: its u' is 0 (NaN if its feature value left the decimal
// path's range, which only costs that evaluation the screening pass).
typedef const ScrDesc3 __attribute__((address_space(4))) *ScrDesc3K;
__device__ __forceinline__ ScrDesc3K constant_ptr(const ScrDesc3 *p) { return (ScrDesc3K)(unsigned long long)p; }

// (NQ slots per call: two in the plain form; ONE with the low-rank form's noise bound, whose temporaries would otherwise cost the
// kernel 48 registers -- a wave of occupancy -- for the four groups of 40 that take this path)
template <int NB, int NQ>
__device__ __forceinline__ void screen_pair3(unsigned band, ScrDesc3K sd, const hafq::ScrTabs &st, float *ud, float &nu2, float &rmin)
{
    float c[NQ][12];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        corner_reads8(band, sd[q].off, c[q]);
        corner_reads4(band, sd[q].off + 8, c[q] + 8);
    }
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(c[0][0]), "+v"(c[0][1]), "+v"(c[0][2]), "+v"(c[0][3]), "+v"(c[0][4]), "+v"(c[0][5]), "+v"(c[0][6]), "+v"(c[0][7]),
                   "+v"(c[0][8]), "+v"(c[0][9]), "+v"(c[0][10]), "+v"(c[0][11]));
    if (NQ > 1)
        asm volatile("" : "+v"(c[NQ - 1][0]), "+v"(c[NQ - 1][1]), "+v"(c[NQ - 1][2]), "+v"(c[NQ - 1][3]), "+v"(c[NQ - 1][4]), "+v"(c[NQ - 1][5]), "+v"(c[NQ - 1][6]), "+v"(c[NQ - 1][7]),
                          "+v"(c[NQ - 1][8]), "+v"(c[NQ - 1][9]), "+v"(c[NQ - 1][10]), "+v"(c[NQ - 1][11]));
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        float r[3], Rk[3], ar = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float s1 = __fsub_rn(c[q][4 * k], c[q][4 * k + 1]), s2 = __fsub_rn(s1, c[q][4 * k + 2]);
            Rk[k] = __fadd_rn(s2, c[q][4 * k + 3]);
            r[k] = __fmul_rn(sd[q].w[k], Rk[k]);
            if (NB == 2) ar = fmaf(fabsf(sd[q].w[k]), region_round_bound(c[q][4 * k], c[q][4 * k + 1], c[q][4 * k + 2], c[q][4 * k + 3], s1, s2, Rk[k]), ar);
        }
        float v;
        if (sd[q].shaf) {                                              // wave-uniform
            v = -1.0f;
            if (r[1] > r[0] && r[1] > r[2]) {                          // fv.cpp:187-191
                const float a = __fsub_rn(r[1], r[0]), b = __fsub_rn(r[1], r[2]);
                v = (b < a) ? b : a;
            }
        } else {
            v = __fadd_rn(__fadd_rn(r[0], r[1]), r[2]);
        }
        const float q4f = (float)hafq::decq4_float_scr(v, st);
        ud[q] = fmaf(q4f, sd[q].scr_mul, sd[q].scr_add);
        if (NB) {
            // (HAF slots only -- pad[0] = 0 for SHAF: three products, the partial sum r0 + r1, the total and the cast of q4 rounded once each:
            // at most 4 u (|r0| + |r1| + |r2|) <= kNbRound3 of it)
            const float nbq = sd[q].pad[0] * (fmaf(kNbRound3, (fabsf(r[0]) + fabsf(r[1])) + fabsf(r[2]), fabsf(q4f - v)) + ar);
            nu2 = fmaf(nbq, nbq, nu2);
            if (NB == 1 && !sd[q].shaf) rmin = fminf(fminf(Rk[0], Rk[1]), fminf(Rk[2], rmin));   // (as in screen_group; a SHAF slot is passed through, not bounded)
            asm volatile("" : "+v"(nu2));
        }
    }
}
__device__ __forceinline__ void screen_pair3(unsigned band, ScrDesc3K sd, const hafq::ScrTabs &st, float *ud) { float dummy = 0.0f, dmin = 0.0f; screen_pair3<0, 2>(band, sd, st, ud, dummy, dmin); }

// the decimal tables (95 doubles) in LDS: call from every thread of the workgroup before any divergent return
__device__ __forceinline__ hafq::PtrTabs load_decimal_tables(double *lds_tab)
{
    if (threadIdx.x < hafq::kTabDoubles) lds_tab[threadIdx.x] = hafq::tab_entry((int)threadIdx.x);
    __syncthreads();
    hafq::PtrTabs tb;
    tb.t = lds_tab;
    return tb;
}

// the screening decimal tables (decq.h: 256 exponent entries + 15 pairs, 2288 bytes) in LDS; workgroups of >= 256 threads
__device__ __forceinline__ hafq::ScrTabs load_screen_tables(unsigned long long *lds_tab)
{
    if (threadIdx.x < hafq::kScrExpEntries) lds_tab[threadIdx.x] = hafq::scr_tab_word((int)threadIdx.x);
    if (threadIdx.x < 2 * hafq::kScrPairs) lds_tab[hafq::kScrExpEntries + threadIdx.x] = hafq::scr_tab_word(hafq::kScrExpEntries + (int)threadIdx.x);
    __syncthreads();
    hafq::ScrTabs st;
    st.w = lds_tab;
    return st;
}

// BYTE offset of the 15x15 window origin II[i-7][j-7] of a cell id (br*H + i)*W + j inside the integral-image buffer
__device__ __forceinline__ unsigned window_origin(int cell, int H, int W)
{
    const int br = cell / (H * W);
    const int rem = cell - br * H * W;
    const int i = rem / W, j = rem - i * W;
    return ((unsigned)br * (unsigned)((H + 1) * (W + 1)) + (unsigned)((i - 7) * (W + 1) + (j - 7))) * 4u;
}

// X image, fp32 form: tiles of 32 evals, k-major inside a tile ([tile][kDP][32] fp32) -- the exact register image of
// the fp32 MFMA A operand, so the contraction kernel fills its A fragments with fully coalesced 256-byte loads.

}  // namespace haf
