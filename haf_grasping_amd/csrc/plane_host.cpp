// plane_host.cpp -- the host side of haf_fit_plane that needs neither a device nor an engine: haf_plane_default, the checks of the frame,
// the mask and the parameters (both entry points apply them), plane_from_moments -- THE plane of a fit from its integer moments, which
// both entry points call -- and haf_fit_plane_ref, the definition of record of plane_rules.h's rules and of the integer rules behind them
// (ranks, counts, the winner, the moments); the device kernels of plane.hip are tested against it word for word.  Built with
// -ffp-contract=off like every unit (build.py: FLAGS).
#include "frames.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace haf {

using namespace haf_plane_math;

namespace {
constexpr double kHalfPi = 1.57079632679489661923;     // (max_tilt is compared with its float: a caller's (float)(pi / 2) passes)
constexpr int64_t kPlaneMaxPixels = (int64_t)1 << 28;     // the moments' bound: each magnitude <= 2^32 N < 2^63
}  // namespace

int check_plane(const haf_frame *frame, const haf_roi *mask, const haf_plane_params *p, const haf_plane_result *out, std::string &err)
{
    if (!frame || !p || !out) { err = "null frame, parameters or result"; return HAF_E_ARG; }
    const int rc = check_frame(*frame, err);
    if (rc != HAF_OK) return rc;
    const float fl[] = {p->tol, p->min_area2, p->up[0], p->up[1], p->up[2], p->max_tilt};
    for (float x : fl)
        if (!std::isfinite(x)) { err = "haf_plane_params: a parameter is not finite"; return HAF_E_ARG; }
    if (!(p->tol > 0.0f)) { err = "haf_plane_params: tol must be positive"; return HAF_E_ARG; }
    if (p->min_area2 < 0.0f) { err = "haf_plane_params: min_area2 < 0"; return HAF_E_ARG; }
    if (p->n_hyp < 1 || p->n_hyp > HAF_MAX_PLANE_HYP) { err = "haf_plane_params: n_hyp outside 1..HAF_MAX_PLANE_HYP"; return HAF_E_ARG; }
    if (p->min_inliers < 3) { err = "haf_plane_params: min_inliers < 3"; return HAF_E_ARG; }
    if (p->max_tilt < 0.0f || p->max_tilt > (float)kHalfPi) { err = "haf_plane_params: max_tilt outside [0, pi/2]"; return HAF_E_ARG; }
    if (mask && mask->mask) {
        if (mask->on_device != 0 && mask->on_device != 1) { err = "the mask's on_device must be 0 (host) or 1 (device)"; return HAF_E_ARG; }
        if (mask->row_stride_bytes < (size_t)frame->width) { err = "the mask's row stride is smaller than the width"; return HAF_E_ARG; }
    }
    if ((int64_t)frame->width * (int64_t)frame->height > kPlaneMaxPixels) { err = "a frame of more than 2^28 pixels"; return HAF_E_CAPACITY; }
    return HAF_OK;
}

PlaneRules plane_rules(const haf_plane_params &p)
{
    PlaneRules r;
    r.tol2 = f_mul(p.tol, p.tol);
    r.min_area2 = p.min_area2;
    memcpy(r.up, p.up, sizeof r.up);
    const double c = std::cos((double)p.max_tilt);
    r.cos2 = (float)(c * c);
    r.uu = dot3(p.up, p.up[0], p.up[1], p.up[2]);
    r.use_up = (p.up[0] != 0.0f || p.up[1] != 0.0f || p.up[2] != 0.0f) ? 1 : 0;
    r.n_hyp = p.n_hyp;
    r.seed = p.seed;
    return r;
}

int plane_winner(const int32_t *counts, int32_t n_hyp)
{
    int w = 0;
    for (int k = 1; k < n_hyp; k++)
        if (counts[k] > counts[w]) w = k;
    return w;
}

namespace {

// eigenvalues (ascending) and unit eigenvectors (columns of v) of a symmetric 3 x 3 matrix: cyclic Jacobi rotations in double
void eigen_sym3(double a[3][3], double lam[3], double v[3][3])
{
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; sweep++) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        const double diag = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
        if (off <= 1e-60 * diag || off == 0.0) break;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                if (a[p][q] == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; k++) {             // A <- A J
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq; a[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; k++) {             // A <- J' A
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; k++) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq; v[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int order[3] = {0, 1, 2};
    for (int i = 0; i < 2; i++)
        for (int j = i + 1; j < 3; j++)
            if (a[order[j]][order[j]] < a[order[i]][order[i]]) { const int t = order[i]; order[i] = order[j]; order[j] = t; }
    double vs[3][3];
    for (int i = 0; i < 3; i++) {
        lam[i] = a[order[i]][order[i]];
        for (int k = 0; k < 3; k++) vs[k][i] = v[k][order[i]];
    }
    memcpy(v, vs, sizeof vs);
}

}  // namespace

void plane_from_moments(const int64_t *m, const float *hyp, const float *up, const float *origin, float *plane, double *rms)
{
    const __int128 N = m[0];
    const double q = (double)kPlaneQuantum;
    // covariance in units of (1/4096 m)^2: (N Sab - Sa Sb) / N^2, the numerators exact
    const int first[3][3] = {{4, 5, 6}, {5, 7, 8}, {6, 8, 9}};
    double cov[3][3] = {}, mean[3] = {};
    if (m[0] > 0) {
        const double n2 = (double)m[0] * (double)m[0];
        for (int i = 0; i < 3; i++) {
            mean[i] = (double)m[1 + i] / (double)m[0] / q;            // metres
            for (int j = 0; j < 3; j++) cov[i][j] = (double)(N * (__int128)m[first[i][j]] - (__int128)m[1 + i] * (__int128)m[1 + j]) / n2;
        }
    }
    double n[3], d;
    bool fitted = false;
    if (m[0] >= 3) {
        double a[3][3], lam[3], v[3][3];
        memcpy(a, cov, sizeof a);
        eigen_sym3(a, lam, v);
        if (lam[2] > 0.0 && lam[1] - lam[0] > 1e-12 * lam[2]) {
            const double len = std::sqrt(v[0][0] * v[0][0] + v[1][0] * v[1][0] + v[2][0] * v[2][0]);
            for (int i = 0; i < 3; i++) n[i] = v[i][0] / len;
            d = -(n[0] * mean[0] + n[1] * mean[1] + n[2] * mean[2]);
            fitted = true;
        }
    }
    if (!fitted) {                                        // the winning hypothesis as it stands, normalised
        const double len = std::sqrt((double)hyp[0] * hyp[0] + (double)hyp[1] * hyp[1] + (double)hyp[2] * hyp[2]);
        for (int i = 0; i < 3; i++) n[i] = (double)hyp[i] / len;
        d = (double)hyp[3] / len;
    }
    // the mean squared distance of the inliers to the plane: n' C n + (n . mean + d)^2
    double var = 0.0;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) var += n[i] * cov[i][j] * n[j];
    const double off = n[0] * mean[0] + n[1] * mean[1] + n[2] * mean[2] + d;
    *rms = m[0] > 0 ? std::sqrt(std::max(0.0, var) / (q * q) + off * off) : 0.0;
    const double c_up = n[0] * up[0] + n[1] * up[1] + n[2] * up[2];
    const double h0 = n[0] * origin[0] + n[1] * origin[1] + n[2] * origin[2] + d;
    const bool flip = c_up != 0.0 ? c_up < 0.0 : h0 < 0.0;
    for (int i = 0; i < 3; i++) plane[i] = (float)(flip ? -n[i] : n[i]);
    plane[3] = (float)(flip ? -d : d);
}

void plane_finish(const haf_frame &f, const haf_plane_params &p, const int32_t *counts, const float *hyps, haf_plane_result *out)
{
    const int w = plane_winner(counts, p.n_hyp);
    out->winner = w;
    out->n_inliers = counts[w];
    out->reserved = 0;
    out->stats[3] = counts[w];
    out->found = (counts[w] >= p.min_inliers && out->stats[1] >= 3) ? 1 : 0;
    out->plane[0] = out->plane[1] = out->plane[2] = out->plane[3] = 0.0f;
    out->rms = 0.0;
    if (out->found) {
        const float origin[3] = {f.sensor_to_base[3], f.sensor_to_base[7], f.sensor_to_base[11]};
        plane_from_moments(out->moments, hyps + 4 * (size_t)w, p.up, origin, out->plane, &out->rms);
    }
}

namespace {

int fit_plane_ref_impl(const haf_frame *frame, const haf_roi *mask, const haf_plane_params *p, haf_plane_result *out, int32_t *counts,
                       float *hyps)
{
    std::string err;
    int rc = check_plane(frame, mask, p, out, err);
    if (rc != HAF_OK) return rc;
    const bool masked = mask && mask->mask;
    if (frame->on_device != 0 || (masked && mask->on_device != 0)) return HAF_E_ARG;      // (host memory only: this function touches no device)
    const size_t W = (size_t)frame->width, H = (size_t)frame->height, n = W * H;
    std::vector<float> xyz(n * 3);
    if ((rc = haf_frame_points(frame, xyz.data())) != HAF_OK) return rc;
    const PlaneRules r = plane_rules(*p);
    std::vector<uint32_t> usable;                          // the usable pixels in raster order: usable[rank] = pixel
    for (size_t i = 0; i < n; i++)
        if (point_usable(&xyz[3 * i]) && (!masked || mask->mask[(i / W) * mask->row_stride_bytes + i % W] != 0)) usable.push_back((uint32_t)i);
    const uint32_t nu = (uint32_t)usable.size();
    const size_t K = (size_t)p->n_hyp;
    std::vector<PlaneHyp> hyp(K);
    std::vector<int32_t> cnt(K, 0);
    std::vector<float> words(K * 4);
    int64_t live = 0;
    for (size_t k = 0; k < K; k++) {
        PlaneHyp &h = hyp[k];
        if (nu == 0) {
            h.n[0] = h.n[1] = h.n[2] = h.d = h.thr = f_from_bits(kInvalidWord);
        } else {
            uint32_t rk[3];
            for (uint32_t j = 0; j < 3; j++) rk[j] = sample_rank(r.seed, (uint32_t)k, j, nu);
            const bool same = rk[0] == rk[1] || rk[0] == rk[2] || rk[1] == rk[2];
            live += !make_hypothesis(&xyz[3 * (size_t)usable[rk[0]]], &xyz[3 * (size_t)usable[rk[1]]], &xyz[3 * (size_t)usable[rk[2]]], same, r, h);
        }
        memcpy(&words[4 * k], h.n, 12);
        words[4 * k + 3] = h.d;
        if (f_nan(h.thr)) continue;
        int32_t c = 0;
        for (uint32_t i : usable) c += inlier(h, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
        cnt[k] = c;
    }
    const int w = plane_winner(cnt.data(), p->n_hyp);
    long long m[kPlaneMoments] = {};
    if (!f_nan(hyp[(size_t)w].thr))
        for (uint32_t i : usable)
            if (inlier(hyp[(size_t)w], xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]))
                add_moments(m, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
    for (int i = 0; i < kPlaneMoments; i++) out->moments[i] = (int64_t)m[i];
    out->stats[0] = (int64_t)n; out->stats[1] = (int64_t)nu; out->stats[2] = live;
    plane_finish(*frame, *p, cnt.data(), words.data(), out);
    if (counts) memcpy(counts, cnt.data(), K * sizeof(int32_t));
    if (hyps) memcpy(hyps, words.data(), K * 4 * sizeof(float));
    return HAF_OK;
}

}  // namespace

}  // namespace haf

extern "C" {

void haf_plane_default(haf_plane_params *p)
{
    if (!p) return;
    p->tol = 0.005f; p->min_area2 = 1e-6f; p->up[0] = p->up[1] = p->up[2] = 0.0f; p->max_tilt = 0.0f;
    p->n_hyp = 256; p->min_inliers = 100; p->seed = 1u;
}

// (no C++ exception may cross the C-ABI: an image too large for the host comes back as a status)
int haf_fit_plane_ref(const haf_frame *frame, const haf_roi *mask, const haf_plane_params *p, haf_plane_result *out, int32_t *counts,
                      float *hyps)
{
    try {
        return haf::fit_plane_ref_impl(frame, mask, p, out, counts, hyps);
    } catch (...) {
    }
    return HAF_E_INTERNAL;
}

}  // extern "C"
