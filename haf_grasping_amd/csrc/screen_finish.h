// screen_finish.h -- the guard band of the PLAIN, SUMSQ and centred-remainder forms of the screening pass (kernels.h: ScreenParams):
// screen_finish() turns the sums the feature kernels accumulate per evaluation (features.hip: su2, sd2, sx2, cr, ub) into the eight band
// floats and a_x.  Host and device: the feature kernels call it per evaluation; the testing build evaluates it on a reference's fp64 sums
// (haf_test_screen_finish, tests/test_screen_operands_gpu.py).  The low-rank form's band is screen_band.h.
#pragma once
#include "kernels.h"

#include <math.h>
#include <string.h>

namespace haf {

// |u' - u| <= kScreenEtaRel |u'| + ScreenParams::eta_abs for the screening attribute u' (feature_device.h: screen_attribute, where the claim is derived)
constexpr double kScreenEtaRel = 5.0e-6 * (1.0 + 1e-6) + 1.8e-7;

// Upper bound of sqrt(x) to 1e-9 relative without a transcendental instruction (the guard band is never checked bit for
// bit by a test, so nothing in it may hang on the v_exp/v_rsq result hazard described in screen.hip): 1/sqrt(x) by the
// exponent-halving bit trick and four Newton steps r <- r (1.5 - 0.5 x r^2), which only multiply and add.
HAF_FRAME_HD double sqrt_upper(double x)
{
    if (!(x > 0.0)) return x == 0.0 ? 0.0 : x + x;      // -0/+0 -> 0; negative or NaN -> NaN (the evaluation is then never trusted)
#if defined(__HIP_DEVICE_COMPILE__)
    double r = __longlong_as_double(0x5FE6EB50C7B537A9LL - (__double_as_longlong(x) >> 1));
#else
    long long xb;
    memcpy(&xb, &x, sizeof xb);
    xb = 0x5FE6EB50C7B537A9LL - (xb >> 1);
    double r;
    memcpy(&r, &xb, sizeof r);
#endif
#pragma unroll
    for (int it = 0; it < 4; it++) r = r * fma(-0.5 * x * r, r, 1.5);
    return x * r * (1.0 + 1e-9);
}
// 2^z - 1 <= ln2 z + 0.26 z^2 for 0 <= z < 0.05 (y = z ln2: e^y - 1 <= y + y^2/2 e^y)
HAF_FRAME_HD double exp2m1_upper(double z) { return 0.69314718056 * z + 0.26 * z * z; }


// guard band of an evaluation (and -|u|^2/2 for the common factor).  u' = c x' is what the
// feature kernel has (screen_attribute), u = c x the true operand: |u' - u| <= eta := 5e-6 |u'| + tiny, component-wise
// and therefore in norm.  With e_n the error of the exp2 argument of SV n,
//   dec^ + rho = 2^D * sum_n c_n K_n 2^e_n,
//   e_n = (u^-u).w^_n + u.(w^_n - w_n) + [fl32(t_n) - t_n + fp32 accumulation in the matrix core]   (slot space, kernels.h),
//   D   = the error of the common factor 2^(-|u|^2/2) (computed from u' in fp32): the SAME factor for every SV.
// Common factor: dec^ - dec = (2^D - 1)(dec + rho) + 2^D E with E = sum_n c_n K_n (2^e_n - 1); it costs
// (2^D - 1)(|dec^| + |rho|), next to nothing where it matters (dec near 0), instead of D * S.
// E = ln2 * sum_n c_n K_n e_n + second order.  The bilinear part of e_n sums to (u^-u).(V^' w) + u.(dV' w), w_n = c_n K_n,
// and is bounded TWICE:
//   (a) per SV by Cauchy-Schwarz:   <= (|u^-u| max|v^_n| + |u| max|v^_n - v_n|) * S                          =: d_max * S
//   (b) through the spectral norms: <= (|u^-u| sigma(V^) + |u| sigma(dV)) * |w|_2,  |w|_2^2 <= max|c_n| * S   (K_n <= 1)
// (b) grows with sqrt(S) only and is ~7x tighter on a 4096-SV model; the kernel takes the smaller of the two.
// |u^-u| <= |u^-u'| + eta and |u| <= |u'| + eta (norms; |u^-u'| and |u'| are accumulated exactly in fp64).
// Second order: |2^e - 1 - ln2 e| <= 0.6 (ln2 e)^2 for |e| < 0.05.  The bracket is bounded per unit of S: norm split exactly
// (das_max), matrix-core accumulation generously (ten accumulating instructions, kappa u of |c| + sum|products| each:
// ScreenParams::acc_rel).  The kernel measures S^ = 2^D sum|c_n| K_n 2^e_n: the true S is at most S^ * 2^(|D| + max|e_n|),
// folded into the outputs.  Output {gA, gB, gC, cm} (kernels.h), scaled by sp.scale:
//   |dec^ - dec| <= [min(gA |w|_2^, gC S^) + (guard_acc0' + gB) S^ + cm (|dec^| + |rho|)] * 1.002,
//   |w|_2^ = sqrt(max|c_n| S^) or, in the kernel's SUMSQ variant, the measured sqrt(sum_n (c_n K_n)^2)

// The band of the CENTRED-REMAINDER form (kernels.h: ScreenParams::cr; derivation in DESIGN.md 2).  The feature kernels are the same
// code: p' = u' - mu through the descriptors' scr_add, su2 / sd2 / sx2 are the norms of p', p^ - p' and p' over all attributes,
// lsum = sum fl32(p'_s) fl32(ln2 g_s) = L in fp32.  With p the TRUE centred operand, dp = p^ - p, dq_n = q^_n - q_n, a_n the rounding of the
// matrix core's fp32 accumulation (|a_n| <= acc_rel |p^||q^_n|), eps_n = dp.q^_n + p.dq_n + a_n the error of z_n:
//   R^ - R = sum b_n (psi(z_n + eps_n) - psi(z_n)),  psi(z) = (ln2 z)^2/2 + psi3(z),  psi3' = ln2 psi >= 0
//   quadratic part:  ln2^2 [p'N dp + p'M p + sum b_n z_n a_n] + ln2^2/2 sum b_n eps_n^2
//                    |.| <= ln2^2 (|N||p||dp| + |M_s||p|^2 + acc_rel |p^||p| C_a) + 1.5 ln2^2 (|H_abs||dp|^2 + |D_abs||p|^2 + acc_rel^2|p^|^2 C_qq)
//   the rest:        |sum b_n (psi3(z^_n) - psi3(z_n))| <= ln2 eps_max sum|b_n| psi(xi_n),  psi(xi) <= psi(z^) + ln2 (2^zmax - 1) eps_max
// Output {L, c_abs, k_psi, cm}: the contraction kernel forms dec^ = A^ (B0 + L + R^) - rho and trusts it when
//   |dec^| > [A^ (c_abs + (guard_acc0' + k_psi) S_psi^) + cm (|dec^| + |rho|)] * 1.002 + guard_abs,   S_psi^ = sum|b_n| psi^(z^_n) as measured.
HAF_FRAME_HD void screen_finish_cr(double su2, double sd2, double sx2, double lsum, const ScreenParams &sp, float *band, float &nax)
{
    constexpr double kF32Acc = 326.0 * 5.9604644775390625e-08 * 1.01;
    const double ln2 = 0.69314718056;
    const double a_x = 0.5 * sx2;
    nax = (float)(-a_x);
    const double un_t = sqrt_upper(sx2 * (1.0 + kF32Acc));                                     // |p'| over all attributes
    const double eta_t = kScreenEtaRel * (un_t + sp.cr_mu_norm_t) + sp.eta_abs;                // |p' - p| = |u' - u| <= 5e-6 |u'| + ..., |u'| <= |p'| + |mu|
    const double un1 = sqrt_upper(su2 * (1.0 + kF32Acc));                                      // |p'| in slot space
    const double dn1 = sqrt_upper(sd2 * (1.0 + kF32Acc)) + 5.97e-8 * un1 + 1e-17;              // |p^ - p'|
    const double eta = kScreenEtaRel * (un1 + sp.cr_mu_norm) + sp.eta_abs;
    const double un = un1 + eta, dn = dn1 + eta, ph = un1 + dn1;                               // |p|, |p^ - p|, |p^|
    const double D = (kF32Acc + 6.0e-8) * a_x + un_t * eta_t + 0.5 * eta_t * eta_t + 6.0e-7;   // error of the common factor's exponent (screen_finish)
    const double eps = dn * sp.cr_qmax + un * sp.cr_dqmax + sp.acc_rel * ph * sp.cr_qmax;      // sup_n |eps_n|
    const double zmax = ph * sp.cr_qmax + eps;                                                 // sup_n of |z^_n| and |z_n|
    const double zf = floor(zmax);
    const double p2 = (zmax < 60.0) ? ldexp(1.0 + (zmax - zf), (int)zf) : (double)__builtin_inff();   // >= 2^zmax (chord of the convex 2^x)
    // accumulation inside the matrix core: |a_n| <= acc_rel sum_k|p^_k q^_nk|; per SV through Cauchy-Schwarz (C_a) or over the SVs
    // through the spectral norms of sqrt|b| Q and sqrt|b| |Q^| (kernels.h: cr_nHaa), whichever is smaller
    const double sHq = sqrt_upper(sp.cr_nHabs) + sqrt_upper(sp.cr_nDabs);
    const double acc_sum = fmin(ph * un * sp.cr_Ca, sHq * un * sqrt_upper(sp.cr_nHaa) * ph);
    const double quad1 = ln2 * ln2 * (sp.cr_nN * un * dn + sp.cr_nM * un * un + sp.acc_rel * acc_sum);
    const double quad2 = 1.5 * ln2 * ln2 * (sp.cr_nHabs * dn * dn + sp.cr_nDabs * un * un + sp.acc_rel * sp.acc_rel * ph * ph * sp.cr_Cqq);
    const double cub2 = ln2 * ln2 * (p2 - 1.0) * eps * eps * sp.cr_Babs * 1.01;
    // L: fl32 of p' and of ln2 g, 320 fp32 fmas (|sum of the terms' magnitudes| <= |p'||g|), p' against p
    const double cL = ln2 * sp.cr_gnorm * (eta + 330.0 * 5.97e-8 * un1) * 1.01 + 1.2e-7 * fabs(lsum);
    double c_abs = quad1 + quad2 + cub2 + cL;
    double k_psi = ln2 * eps * 1.01;
    if (sp.cr_poly) {
        // psi(t) = t^2 (1/2 + t/6 + t^2/24 + t^3/120), t = z ln2: the dropped tail is at most 4.1 t^4/360 of psi for |t| <= 1; the fp32
        // roundings per element -- z^2, the four constants b a_k (folded per block), three Horner steps whose partial sums are at most
        // 1.95 P(z) for z < 0 -- come to less than 8 u of |b| psi; 10 u charged
        const double t = ln2 * zmax;
        k_psi += 4.1 * t * t * t * t / 360.0 + 10.0 * 5.97e-8;
        if (!(t <= 1.0)) k_psi = (double)__builtin_inff();
    } else {
        // 2^z by v_exp_f32 (an ulp of 2^z: taken as 2^-22), the constant ln2 in fp32: relative to sum|b_n| 2^z_n <= S_psi + B_abs + ln2 sum|b_n||z_n|
        const double uexp = 2.4e-7;
        k_psi += uexp;
        c_abs += uexp * (sp.cr_Babs + ln2 * ph * sp.cr_Cq1) * 1.01;
    }
    const double infl = 1.0 + exp2m1_upper(D);
    band[0] = (float)lsum;
    band[1] = (float)(c_abs * infl * sp.scale * (1.0 + 1e-6));
    band[2] = (float)(k_psi * infl * sp.scale * (1.0 + 1e-6));
    band[3] = (float)(exp2m1_upper(D) * sp.scale);
    band[4] = 0.0f; band[5] = 0.0f; band[6] = 0.0f; band[7] = 0.0f;
    if (!(D < 0.05) || !(a_x < 30.0) || !(zmax < 60.0)) band[1] = __builtin_inff();
}

HAF_FRAME_HD void screen_finish(double su2, double sd2, double sx2, double cr, double ubd, const ScreenParams &sp, float *band,
                                              float &nax)
{
    if (sp.cr) {                                         // wave-uniform: the centred-remainder form has its own band
        screen_finish_cr(su2, sd2, sx2, cr, sp, band, nax);
        return;
    }
    // su2 = sum over the SLOTS of fl32(u')^2 and sd2 = sum over the slots of (u^ - fl32(u'))^2: the two norms of the operand the
    // contraction sees (kernels.h: attributes that share a slot are one operand).  sx2 = su2 + the squares of the attributes
    // beyond the first of every slot = |u'|^2 over ALL attributes, which is what the common factor 2^(-|u|^2/2) needs.
    // All three are fp32 sums (screen_operand) of at most 324 squares of fp32-rounded terms: off by at most 326 * 2^-24
    // relative.  For the norms that is an inflation; for a_x it is one more part of D, the error of the common factor, and costs
    // (2^D - 1)(|dec^| + |rho|) like the rest of D.
    constexpr double kF32Acc = 326.0 * 5.9604644775390625e-08 * 1.01;
    const double a_x = 0.5 * sx2;
    nax = (float)(-a_x);                                 // k_svm_screen multiplies both class sums by exp2(nax)
    const double un_t = sqrt_upper(sx2 * (1.0 + kF32Acc));                        // |u'| over all attributes
    const double eta_t = kScreenEtaRel * un_t + sp.eta_abs;                      // |u' - u| over all attributes
    const double un1 = sqrt_upper(su2 * (1.0 + kF32Acc));                         // |u'| in slot space
    const double dn1 = sqrt_upper(sd2 * (1.0 + kF32Acc)) + 5.97e-8 * un1 + 1e-17;  // |u^ - u'| <= |u^ - fl32(u')| + 2^-24 |u'|
    const double eta = kScreenEtaRel * un1 + sp.eta_abs;                        // |u' - u| in slot space
    const double un = un1 + eta, dn = dn1 + eta;                                // |u|, |u^ - u|
    const double ln2 = 0.69314718056;
    const double d_max = dn * sp.v_max + (un + dn) * sp.dv_max;
    // fp32 accumulation inside the matrix core: ten accumulating instructions per element, each off by at most kappa u of its
    // |c| + sum|products| <= |t_n| + |u||w^_n| (the chain starts at t_n; kappa: the measured property of screen.hip's
    // probe_mfma_rounding() with its margin, 8.2 on the devices seen so far: sp.acc_rel = 82 u)
    const double acc = sp.acc_rel * (un * sp.v_max + sp.as_max);
    // D = | log2 of (the factor the kernel applies / 2^(-|u|^2/2)) |: a_x from the fp32 sums and u' instead of u, its cast to
    // fp32, v_exp_f32 and the two products (3 * 2^-23 relative = 5.2e-7 in the exponent)
    const double D = (kF32Acc + 6.0e-8) * a_x + un_t * eta_t + 0.5 * eta_t * eta_t + 6.0e-7;
    const double e_max = d_max + sp.das_max + acc;
    const double infl = 1.0 + exp2m1_upper(e_max + D);   // meaningful below 0.05 only: beyond it the band is infinite anyway
    const double gA = ln2 * (dn * sp.sigma_v + (un + dn) * sp.sigma_dv);   // per unit of |w|_2, which the contraction kernel supplies
    const double gB = ln2 * (sp.das_max + acc) + 0.6 * (ln2 * e_max) * (ln2 * e_max);
    band[0] = (float)(gA * infl * sp.scale);             // (|w|_2 measured: inflated like S; bounded through sqrt(S): sqrt(infl) <= infl)
    band[1] = (float)(gB * infl * sp.scale);             // scale = 1.001: the roundings of these expressions and of the casts are far inside 0.1 %
    band[2] = (float)(ln2 * d_max * infl * sp.scale);
    band[3] = (float)(exp2m1_upper(D) * sp.scale);
    // outside the range the bounds were derived for, or a common factor 2^(a_x) that fp32 sums could overflow on: never trusted
    // (2^(2 a_x) must stay finite in fp32 for the SUMSQ variant's sum of squares)
    if (!(e_max + D < 0.05) || !(a_x < 30.0)) band[1] = __builtin_inff();
    // ---- the centred estimate dec^ - corr * sc (kernels.h: ScreenParams; derivation in DESIGN.md 2) ----
    // w_n = c_n K_n = sc c_n kappa_n + sc c_n (k_n - kappa_n), kappa_n = 2^(t_n + ubar.w^_n), k_n = 2^(t_n + u.w_n) (raw space, TRUE
    // operands).  First-order error of the first part: ln2 sc [(u^-u).G + u.Hd], known up to u' - u and fp32 roundings: corrected.
    // Second part: k_n - kappa_n = kappa_n (2^zeta_n - 1), zeta_n = u.w_n - ubar.w^_n = (u^ - ubar).w^_n - e_n with e_n the bilinear
    // part of the exp2 argument's error, |e|_2 <= |u^-u| sigma(W^) + |u| sigma(dW) =: e2 and |e_n| <= d_max.  With
    // |2^zeta - 1| <= ln2 |zeta| 2^|zeta|:   |c (k - kappa)|_2 <= ln2 2^zmax (sigma(diag(c kappa) W^) |u^ - ubar| + max|c kappa| e2).
    band[4] = 0.0f; band[5] = __builtin_inff(); band[6] = 0.0f; band[7] = 0.0f;
    if (sp.sigma_dk < 1e300) {
        // |fl32(u') - ubar|^2 from the fp32 sums: each is off by at most kF32Acc of the sum of its terms' magnitudes
        const double ubn = sqrt_upper(sp.ubar2);
        double du2 = su2 - 2.0 * ubd + sp.ubar2 + kF32Acc * (su2 + 2.0 * un1 * ubn) + 1e-30;
        if (!(du2 > 0.0)) du2 = (du2 == du2) ? 0.0 : du2;                        // (NaN stays NaN: never trusted)
        const double dun = sqrt_upper(du2) + dn1;                                // |u^ - ubar| <= |fl32(u') - ubar| + |u^ - fl32(u')|
        const double e2 = dn * sp.sigma_v + (un + dn) * sp.sigma_dv;
        const double zmax = dun * sp.v_max + e_max;                              // sup_n |zeta_n|
        const double zf = floor(zmax);
        // 2^zmax <= (1 + frac) 2^floor: the chord of the convex 2^x over [0, 1] (no transcendental instruction: see sqrt_upper)
        const double p2 = (zmax < 60.0) ? ldexp(1.0 + (zmax - zf), (int)zf) : (double)__builtin_inff();
        const double dev = ln2 * p2 * (sp.sigma_dk * dun + sp.ck_max * e2);
        // what the computed correction misses: u' against u in both dot products ((u'-u).(G - Hd)), the 2 x 320 fp32 roundings of
        // its accumulation and the fp32 rounding of the constants
        const double cerr = ln2 * (eta * (sp.g_norm + sp.hd_norm) + 4.2e-5 * (dn1 * sp.g_norm + un1 * sp.hd_norm));
        band[4] = (float)(ln2 * cr);
        band[5] = (float)((ln2 * e2 * dev * infl + cerr) * sp.scale);
        if (!(e_max + D < 0.05) || !(a_x < 30.0) || !(zmax < 60.0)) band[5] = __builtin_inff();
    }
}

}  // namespace haf
