// engine_request.cpp -- one request through the engine: stage launches on the engine's stream, the decision tiers (screening pass,
// second screening pass, three-pass tier, exact-integer tier, fp64 MFMA tier, strict order), the host resolution of the residual
// cases with glibc's exp, the adaptive choice of the screening form, and the batch wrapper (loop_control, server.cpp:335-402).
#include "engine_state.h"

namespace haf_host {

// One kernel value K(x, s_n) on the HOST exactly as svm-predict forms it (Kernel::k_function, svm.cpp:318-371) with the C library's
// exp / tanh: x = the device's attributes (stride 16 doubles: one column of the fp64 image), s_n in model order.  -ffp-contract=off.
static double host_kernel_value(const SvmModel &m, const double *xg, int n, int kx)
{
    double acc = 0.0;
    if (m.kernel_type == HAF_KERNEL_RBF) {
        for (int k = 0; k < kx; k++) {                           // svm.cpp:333-347: index order, a missing entry is 0
            const double sv = k < m.dim ? m.sv[(size_t)n * m.dim + k] : 0.0;
            const double dd = xg[(size_t)k * 16] - sv;
            acc += dd * dd;
        }
        return std::exp(-m.gamma * acc);                         // svm.cpp:364: glibc's exp
    }
    for (int k = 0; k < kx; k++) {                               // Kernel::dot, svm.cpp:299-316 (a zero on either side adds +-0)
        const double sv = k < m.dim ? m.sv[(size_t)n * m.dim + k] : 0.0;
        acc += xg[(size_t)k * 16] * sv;
    }
    if (m.kernel_type == HAF_KERNEL_POLY) {                      // powi, svm.cpp:26-36
        double tmp = m.gamma * acc + m.coef0, ret = 1.0;
        for (int t = m.degree; t > 0; t /= 2) { if (t % 2 == 1) ret *= tmp; tmp = tmp * tmp; }
        return ret;
    }
    if (m.kernel_type == HAF_KERNEL_SIGMOID) return std::tanh(m.gamma * acc + m.coef0);   // svm.cpp:367: glibc's tanh
    return acc;                                                  // LINEAR
}

// libsvm's decision value (svm.cpp:2509-2513: both classes' terms in model order) on the HOST from one column of the fp64 image
static double host_decision(const SvmModel &m, const double *xg, int kx)
{
    double sum = 0.0;
    for (int n = 0; n < m.n_sv; n++) sum += m.coef[(size_t)n] * host_kernel_value(m, xg, n, kx);
    return sum - m.rho;
}

// The fp64 attribute image ([group of 16][324][16]) of the entries [off, off + n) of a list -- counters[cnt] entries long -- through
// the feature kernel, then to the host: column i of x64 (attr_column) holds entry off + i
static int fetch_attributes64(haf_engine *e, const Dims &d, hipStream_t s, const int *list, int cnt, int off, int n, std::vector<double> &x64)
{
    launch_features(e->d_ii.p, e->d_evalcell.p, e->d_counters.p, e->mdl.fd.p, reinterpret_cast<float *>(e->d_x64.p), nullptr, d, e->range.lower,
                    e->range.upper, 0.0f, n, XMODE_F64, ScreenParams{}, list + off, cnt, n, false, n, nullptr, nullptr, s, off);
    x64.assign(((size_t)n + 15) / 16 * kKP * 16, 0.0);
    HIPCHK(e, hipMemcpyAsync(x64.data(), e->d_x64.p, x64.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    return HAF_OK;
}
static const double *attr_column(const std::vector<double> &x64, int i) { return x64.data() + (size_t)(i >> 4) * kKP * 16 + (i & 15); }

// The strict tier (k_recheck) restates libsvm's summation order operation for operation, but its exp() is the device's, not
// glibc's.  Both are within an ulp of the true value, so the two sums differ by at most 2^-52 sum|coef|; a strict-tier decision
// value closer to zero than host_exp_thr (256 x that) is therefore evaluated once more HERE, on the host, with the C library's
// exp -- the very function the reference's svm-predict calls (svm.cpp:325-365, 2478-2532) -- from the attributes the device
// computed (the decimal round trips are bit-pinned to glibc, tests/).  Nothing has come this far in any run; the path exists so
// that "the labels are libsvm's" has no residual.  *resolved = the number of evaluations decided here; *changed = a label moved.
static int host_resolve_strict(haf_engine *e, const Dims &d, hipStream_t s, bool *changed, int *resolved)
{
    *changed = false;
    *resolved = 0;
    const int n2 = std::min(e->h_counters[CNT_FLAGGED2], e->list_cap);
    if (n2 <= 0 || e->mdl.prob_mode) return HAF_OK;
    std::vector<double> dec((size_t)n2);
    std::vector<int> ev((size_t)n2);
    HIPCHK(e, hipMemcpyAsync(dec.data(), e->d_dec_exact2.p, (size_t)n2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(ev.data(), e->d_flag2_list.p, (size_t)n2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    std::vector<double> x64;
    for (int off = 0; off < n2; off += e->flag_cap) {            // (the attribute image holds one window of the list at a time)
        const int nw = std::min(e->flag_cap, n2 - off);
        std::vector<int> cand;
        for (int i = off; i < off + nw; i++) if (!(std::fabs(dec[(size_t)i]) > e->mdl.host_exp_thr)) cand.push_back(i);
        if (cand.empty()) continue;
        const int rc = fetch_attributes64(e, d, s, e->d_flag2_list.p, CNT_FLAGGED2, off, nw, x64);
        if (rc != HAF_OK) return rc;
        for (int i : cand) {
            const double dv = host_decision(e->model, attr_column(x64, i - off), e->mdl.kx);
            const int8_t lab = (int8_t)(dv > 0.0 ? e->mdl.gv0 : e->mdl.gv1);
            int cell = 0;
            int8_t old = 0;
            HIPCHK(e, hipMemcpy(&cell, e->d_evalcell.p + ev[(size_t)i], sizeof(int), hipMemcpyDeviceToHost));
            HIPCHK(e, hipMemcpy(&old, e->d_labels.p + cell, 1, hipMemcpyDeviceToHost));
            if (old != lab) *changed = true;
            HIPCHK(e, hipMemcpy(e->d_labels.p + cell, &lab, 1, hipMemcpyHostToDevice));
            HIPCHK(e, hipMemcpy(e->d_dec_exact2.p + i, &dv, sizeof(double), hipMemcpyHostToDevice));
            (*resolved)++;
        }
    }
    return HAF_OK;
}

// svm_predict_probability for two classes on the HOST, operation for operation as svm.cpp:2550-2587 (sigmoid_predict 1818-1826 with
// the C library's exp, the [1e-7, 1 - 1e-7] clamp, multiclass_probability 1829-1888 for k = 2); this TU is built with -ffp-contract=off
static int host_probability(double dec, double A, double B, double p[2])
{
    const double fApB = dec * A + B;
    double s = fApB >= 0.0 ? std::exp(-fApB) / (1.0 + std::exp(-fApB)) : 1.0 / (1.0 + std::exp(fApB));
    const double min_prob = 1e-7;
    s = std::min(std::max(s, min_prob), 1.0 - min_prob);
    const int k = 2;
    double r[2][2] = {{0.0, s}, {1.0 - s, 0.0}}, Q[2][2], Qp[2], pQp;
    const double eps = 0.005 / k;
    for (int t = 0; t < k; t++) {
        p[t] = 1.0 / k;
        Q[t][t] = 0.0;
        for (int j = 0; j < t; j++) { Q[t][t] += r[j][t] * r[j][t]; Q[t][j] = Q[j][t]; }
        for (int j = t + 1; j < k; j++) { Q[t][t] += r[j][t] * r[j][t]; Q[t][j] = -r[j][t] * r[t][j]; }
    }
    for (int iter = 0; iter < 100; iter++) {
        pQp = 0.0;
        for (int t = 0; t < k; t++) {
            Qp[t] = 0.0;
            for (int j = 0; j < k; j++) Qp[t] += Q[t][j] * p[j];
            pQp += p[t] * Qp[t];
        }
        double max_error = 0.0;
        for (int t = 0; t < k; t++) max_error = std::max(max_error, std::fabs(Qp[t] - pQp));
        if (max_error < eps) break;
        for (int t = 0; t < k; t++) {
            const double diff = (-Qp[t] + pQp) / Q[t][t];
            p[t] += diff;
            pQp = (pQp + diff * (diff * Q[t][t] + 2.0 * Qp[t])) / (1.0 + diff) / (1.0 + diff);
            for (int j = 0; j < k; j++) { Qp[j] = (Qp[j] + diff * Q[t][j]) / (1.0 + diff); p[j] /= (1.0 + diff); }
        }
    }
    return p[1] > p[0] ? 1 : 0;
}

// Probability mode: the estimates k_prob_eval could not vouch for (a last-bit difference between the device's exp and glibc's could
// move their label or a printed digit; CNT_FLAGGED / d_flag_list) are finished HERE: the libsvm-order decision value with the C
// library's exp from the device's attributes (as host_resolve_strict does), svm_predict_probability with the C library's exp, the
// "%g" forms by the host build of decq (pinned to glibc's printf + strtod).  Writes what k_prob_eval writes.
static int host_resolve_probability(haf_engine *e, const Dims &d, hipStream_t s, int *resolved)
{
    *resolved = 0;
    const int n = std::min(e->h_counters[CNT_FLAGGED], e->list_cap);
    if (n <= 0) return HAF_OK;
    std::vector<int> ev((size_t)n);
    HIPCHK(e, hipMemcpyAsync(ev.data(), e->d_flag_list.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    std::vector<double> x64;
    for (int off = 0; off < n; off += e->flag_cap) {
        const int nw = std::min(e->flag_cap, n - off);
        const int rc = fetch_attributes64(e, d, s, e->d_flag_list.p, CNT_FLAGGED, off, nw, x64);
        if (rc != HAF_OK) return rc;
        for (int i = 0; i < nw; i++) {
            const double dv = host_decision(e->model, attr_column(x64, i), e->mdl.kx);
            double p[2];
            const int idx = host_probability(dv, e->mdl.prob.A, e->mdl.prob.B, p);
            const double q[2] = {hafq::decq(p[0], 6), hafq::decq(p[1], 6)};
            const int res = idx ? e->mdl.prob.gv1 : e->mdl.prob.gv0;
            const float own = (float)res * (float)(res > 0 ? q[1] : q[0]);
            const int8_t lab = (int8_t)res;
            const int evi = ev[(size_t)(off + i)];
            int cell = 0;
            HIPCHK(e, hipMemcpy(&cell, e->d_evalcell.p + evi, sizeof(int), hipMemcpyDeviceToHost));
            HIPCHK(e, hipMemcpy(e->d_own.p + cell, &own, sizeof(float), hipMemcpyHostToDevice));
            HIPCHK(e, hipMemcpy(e->d_labels.p + cell, &lab, 1, hipMemcpyHostToDevice));
            HIPCHK(e, hipMemcpy(e->d_ptext.p + 2 * (size_t)evi, q, 2 * sizeof(double), hipMemcpyHostToDevice));
            HIPCHK(e, hipMemcpy(e->d_dec_exact2.p + evi, &dv, sizeof(double), hipMemcpyHostToDevice));
            (*resolved)++;
        }
    }
    return HAF_OK;
}

// ---- the routing of one decision stage: pure, no device (tests/test_host_cpu.py enumerates it through haf_test_tier_plan) ----
TierPlan plan_tiers(const TierFacts &f)
{
    TierPlan p;
    if (f.generic_kernel || f.direct) {
        // a model whose kernel is not RBF: every evaluation on the strict tier's list, libsvm's own arithmetic for all of them.
        // A tiny request: exact attributes, fp64 MFMA decision and label of EVERY evaluation in one launch (k_small_direct), what it
        // leaves on the strict tier's list
        p.path = f.generic_kernel ? PATH_GENERIC : PATH_DIRECT;
        p.pass0_out = L_FLAG2;
        return p;
    }
    p.path = f.mode == MODE_SCREEN ? PATH_SCREEN : f.mode == MODE_SPLIT ? PATH_SPLIT : PATH_F32;
    const int v = f.screen_variant;
    const bool cr_poly_t1 = p.path == PATH_SCREEN && v == SCREEN_CR_POLY && f.t1_cr_available;
    // tier 2a in front of the fp64 MFMA tier (exact8.hip): the same evaluations on EXACT integer dot products (int8 digit planes); what
    // it cannot decide either -- |dec| inside the operands' quantisation, ~1e-7 S -- is the fp64 MFMA tier's list.
    // (behind the centred-remainder form of tier 1 the exact-integer tier has nothing to add: its band is the quantisation of the
    // operands relative to sum|coef|K -- 8e-9 S for the trained model, 0.14 -- and tier 1's is relative to S_psi, 0.02: measured,
    // it decided 8 of 9984 evaluations in 4.6 ms.  What tier 1 leaves goes straight to the fp64 MFMA tier)
    p.i8 = f.i8_active && !f.small_exact && !cr_poly_t1;
    if (p.i8) { p.i8_in = L_FLAG; p.i8_out = L_FLAGI; }
    p.fp64 = f.small_exact ? FP64_SMALL : FP64_MFMA;
    p.fp64_in = p.i8 ? L_FLAGI : L_FLAG;
    p.fp64_out = L_FLAG2;
    p.pass0_out = L_FLAG;
    if (p.path != PATH_SCREEN) return p;

    // tier 0: single-pass fp16 screening of every evaluation; tier 1: the three-pass kernel on what it could not decide
    // (the centred-remainder variants have their own operand images: translated attributes, centred support vectors)
    p.cr = v == SCREEN_CR_EXP || v == SCREEN_CR_POLY;
    p.reuse = f.reuse_operands;
    // Low-rank form of the centred-remainder pass (kernels.h: kLrK): whole requests large enough for the thread-per-evaluation
    // feature kernel on grids that went through the parallel integral image (whose pass records negative heights), when the
    // centred-remainder form serves the model; the 10-step images go through k_project, the sweep runs on 6-step images.
    const bool lr_plain = v == SCREEN_PLAIN && f.lr_plain_available;      // the plain epilogue on the projected (centred) operands
    p.lr = (p.cr || lr_plain) && f.large && f.lr_available && f.lr_enabled && !f.fused_pre && f.hw > 8192 && !f.reuse_operands;
    p.sp = p.lr && lr_plain ? SP_LRP : p.cr ? SP_CR : SP_PLAIN;
    // Tier 0b: the centred-remainder form once more on the first pass's list, behind a PLAIN / SUMSQ first pass or a low-rank CR_EXP
    // one (the waves it cannot bound -- the borders of the grid, waves that are not a run of neighbours -- and what its slightly wider
    // band leaves).  Round 5: behind a LOW-RANK first pass with the plain epilogue it is the low-rank sweep itself with the
    // centred-remainder epilogue in its GATHER form -- the first pass's operand images and raw sums by evaluation id, no second
    // feature kernel.
    if (f.use_t0b && f.cr_available && !f.small_exact && (!p.cr || (p.lr && v == SCREEN_CR_EXP)))
        p.t0b = p.sp == SP_LRP && f.lr_fused && !f.t0b_no_gather ? T0B_GATHER : T0B_FEATURES;
    // A small request with a small model (small_exact): what the screening passes leave goes STRAIGHT to the one-launch exact kernel
    // (k_small_direct in list mode: exact attributes + fp64 MFMA decision, 9 ns per listed evaluation at 192 SVs) -- the list is
    // written where that kernel reads it.  Tier 1 in between was a feature kernel and a contraction launch at their latency floors
    // (C3: 44 + 36 us for 4 072 evaluations, of which it decided nine tenths) in front of the same exact kernel.  The same hand-over
    // when calibration found tier 1 of little use behind the screening passes (t1_skip).
    const bool straight = f.small_exact || f.t1_skip;
    if (p.t0b != T0B_NONE) {
        p.pass0_out = L_FLAG0;
        p.t0b_in = L_FLAG0;
        p.t0b_out = straight ? L_FLAG : L_FLAG0B;
    } else {
        p.pass0_out = straight ? L_FLAG : L_FLAG0;
    }
    p.t1 = !straight;
    if (!p.t1) return p;
    p.t1_in = p.t0b != T0B_NONE ? L_FLAG0B : L_FLAG0;
    p.t1_cnt = list_counter(p.t1_in);
    p.t1_out = L_FLAG;
    // behind the polynomial centred-remainder form (a model whose decisions are 1e-7 of sum|coef|K) tier 1 runs in that form too:
    // the plain three-pass kernel's band is relative to sum|coef|K and could decide nothing there
    p.t1cr = cr_poly_t1;
    // Round 5, the short-list gate: a SMALL request against a BIG model leaves the screening passes a handful of evaluations (C3
    // against the headline's 4 096-SV model: 31), and tier 1 and the exact-integer tier behind it are then ~120 us of launches and
    // minimum chains -- feature kernels, sweeps over thousands of SVs by a few workgroups -- for nothing the fp64 tier would
    // not do in the one pass it makes anyway.  At most kShortListGate entries go straight to its list; tier 1 reads its list's
    // length from CNT_T1_N (0 then), the exact-integer tier finds an empty input.  Not while the engine calibrates (the
    // calibration measures what tier 1 decides).
    p.gate = f.calibrated && f.short_gate && f.n_sv >= kShortGateMinSv && f.evals_cap <= 65536;
    if (p.gate) {
        p.gate_in = p.t1_in;
        p.gate_out = p.fp64_in;
        p.t1_cnt = CNT_T1_N;
    }
    return p;
}

static int *list_buf(haf_engine *e, int l)
{
    int *const buf[] = {e->d_flag0_list.p, e->d_flag0b_list.p, e->d_flag_list.p, e->d_flagi_list.p, e->d_flag2_list.p};
    return l == L_NONE ? nullptr : buf[l];
}
static size_t list_len(const haf_engine *e, int l)
{
    const size_t n[] = {e->d_flag0_list.n, e->d_flag0b_list.n, e->d_flag_list.n, e->d_flagi_list.n, e->d_flag2_list.n};
    return l == L_NONE ? 0 : n[l];
}
// a pass that writes the exact tiers' input list publishes its length in that list's counter too (screen.hip: also_counter)
static int handover_counter(int l) { return l == L_FLAG ? CNT_FLAGGED : -1; }

// ---- one request: what its stages share ----
struct Request {
    int B = 0, R = 0, max_n = 0;
    long total_n = 0;
    bool bucket_ok = true;
    size_t pts_off = 0;                  // the points area of the input block: [CloudDev x B][RollGeo x B*R]([FrameDev x n_frames]([RoiViewDev x n_frames]))[points of the host clouds]
    FrameSource from;                    // (views: the host sizes everything by the UPPER bound clouds[b].n_points, the live count is CloudDev::n on the device)
    int n_frames = 0;                    // entries of frames / h_frames: B, or the sum of views
    FrameDev *h_frames = nullptr;
    const FrameDev *d_frames = nullptr;
    RoiViewDev *h_roi_views = nullptr;   // views under masks (haf_score_views_roi): one per view, behind the FrameDev array
    const RoiViewDev *d_roi_views = nullptr;
    std::vector<LastCall::CloudSrc> src; // where every cloud's points lie (LastCall::clouds)
    CloudDev *h_clouds = nullptr;
    const CloudDev *d_clouds = nullptr;
    const RollGeo *d_geo = nullptr;
    hipStream_t s = nullptr;
    Dims d{};
    float r_row = 0.0f, r_col = 0.0f;
    long evals_cap = 0, evals_sel = 0;
    bool direct = false, short_request = false, small_exact = false, large = false, fused_pre = false;
    // what the last decide() ran, for the adaptive rule and the record of the call
    bool i8_used = false, t0b_used = false;
    bool lr_used = false;                // (of the last decide() with a screening pass)
    int host_resolved = 0;
};

static int check_request(haf_engine *e, int32_t n_clouds, const haf_cloud *clouds, const haf_grasp_input *in, int32_t roll_first,
                         int32_t roll_count, const haf_roll_record *records, Request &q)
{
    if (!clouds || !in || !records || n_clouds < 1) return fail(e, HAF_E_ARG, "haf_score_rolls: null or empty argument");
    const haf_config &c = e->cfg;
    if (n_clouds > c.max_clouds) return fail(e, HAF_E_CAPACITY, "more clouds than max_clouds");
    if (roll_first < 0 || roll_count < 1 || roll_first + roll_count > c.n_rolls) return fail(e, HAF_E_ARG, "roll range outside [0, n_rolls)");
    if (roll_count > e->max_rolls) return fail(e, HAF_E_CAPACITY, "more rolls in one call than max_rolls_per_call");
    HIPCHK(e, hipSetDevice(c.device));
    q.B = n_clouds;
    q.R = roll_count;
    size_t host_pts = 0;
    for (int b = 0; b < q.B; b++) {
        if (clouds[b].n_points && !clouds[b].xyz) return fail(e, HAF_E_ARG, "cloud with null xyz");
        if (clouds[b].stride_floats < 3) return fail(e, HAF_E_ARG, "stride_floats must be >= 3");
        if (clouds[b].n_points > (size_t)INT32_MAX) return fail(e, HAF_E_CAPACITY, "cloud too large");
        if (clouds[b].on_device == 2) {
            const char *p0 = reinterpret_cast<const char *>(clouds[b].xyz), *p1 = p0 + clouds[b].n_points * 12;
            bool inside = false;
            for (auto &r : e->host_regs) inside = inside || (p0 >= r.first && p1 <= r.first + r.second);
            if (clouds[b].stride_floats != 3 || (clouds[b].n_points && !inside))
                return fail(e, HAF_E_ARG, "on_device = 2 needs a packed xyz cloud inside a buffer registered with haf_register_host_cloud");
        }
        if (clouds[b].on_device != 1 && !(q.from.objects && b > 0)) host_pts += clouds[b].n_points;      // (an objects call: every cloud is frame 0's points)
        q.max_n = std::max(q.max_n, (int)clouds[b].n_points);
    }
    if (host_pts > (size_t)c.max_points) return fail(e, HAF_E_CAPACITY, "more host points than max_points");
    return HAF_OK;
}

// the request's input block (in_block): the two header arrays on the host, one copy carries them with the points
static void pack_headers(haf_engine *e, const haf_cloud *clouds, const haf_grasp_input *in, int roll_first, Request &q)
{
    const haf_config &c = e->cfg;
    const int B = q.B, R = q.R;
    const haf_frame *const frames = q.from.frames;
    const int32_t *const views = q.from.views;
    const size_t geo_off = up16((size_t)B * sizeof(CloudDev));
    const size_t frames_off = geo_off + up16((size_t)B * R * sizeof(RollGeo));
    q.n_frames = 0;
    const bool shared = q.from.objects != nullptr;       // haf_score_objects: ONE frame, whose points every cloud of the batch points at
    for (int b = 0; frames && b < (shared ? 1 : B); b++) q.n_frames += views ? views[b] : 1;
    const size_t roi_off = frames_off + up16((size_t)q.n_frames * sizeof(FrameDev));
    const bool roi_views = views && q.from.roi;
    q.pts_off = roi_off + (roi_views ? up16((size_t)q.n_frames * sizeof(RoiViewDev)) : 0);
    if (roi_views) {
        q.h_roi_views = reinterpret_cast<RoiViewDev *>(e->in_block.host + roi_off);
        q.d_roi_views = reinterpret_cast<const RoiViewDev *>(e->in_block.dev.p + roi_off);
    }
    q.h_frames = reinterpret_cast<FrameDev *>(e->in_block.host + frames_off);
    q.d_frames = reinterpret_cast<const FrameDev *>(e->in_block.dev.p + frames_off);
    q.src.assign((size_t)B, LastCall::CloudSrc{});
    q.h_clouds = reinterpret_cast<CloudDev *>(e->in_block.host);
    RollGeo *h_geo = reinterpret_cast<RollGeo *>(e->in_block.host + geo_off);
    q.d_clouds = reinterpret_cast<const CloudDev *>(e->in_block.dev.p);
    q.d_geo = reinterpret_cast<const RollGeo *>(e->in_block.dev.p + geo_off);
    const float *d_points = reinterpret_cast<const float *>(e->in_block.dev.p + q.pts_off);
    size_t off = 0;
    for (int b = 0; b < B; b++) {
        NormalisedInput n = normalise(in[b]);
        CloudDev &cd = q.h_clouds[b];
        for (int r = 0; r < R; r++) fill_roll_geo(c, in[b], n, roll_first + r, h_geo[b * R + r], r == 0 ? cd.m0 : nullptr);
        if (n.width == 0) q.bucket_ok = false;           // x-scale 0: every point lands in row H/2, whatever its distance
        cd.sorted_off = (int)q.total_n;
        cd.bucket_off = b * e->bkt_ints;
        q.total_n += (long)clouds[b].n_points;
        cd.n = views ? 0 : (int)clouds[b].n_points;      // (views: the kernels count the valid points)
        if (shared && b > 0) {
            cd.xyz = q.h_clouds[0].xyz;
            cd.stride = 3;
            q.src[(size_t)b] = q.src[0];
        } else if (clouds[b].on_device == 1) {
            cd.xyz = clouds[b].xyz;
            cd.stride = (int)clouds[b].stride_floats;
        } else {
            if (frames) off = (off + 3) / 4 * 4;         // a frame's points start 16-byte aligned: k_frame_points stores whole dwordx4
            cd.xyz = d_points + off * 3;
            cd.stride = 3;
            q.src[(size_t)b] = LastCall::CloudSrc{q.pts_off / sizeof(float) + off * 3, clouds[b].n_points, true};
            off += clouds[b].n_points;
        }
    }
    // the frames' descriptors: device-resident frames are read where they lie; a host XYZ frame is packed where its points go and
    // transformed in place; a host depth frame's pixels go through the raw area, every frame at a multiple of 16 bytes.
    // Views: compaction writes where other lanes have not read yet, so a host XYZ view is NOT staged in the points area but in a raw
    // area of its own (raw_xyz); the views of a request share its region and its counter
    size_t raw = 0, raw_xyz = 0;
    for (int b = 0, k = 0; frames && b < (shared ? 1 : B); b++) {
        for (int v = 0; v < (views ? views[b] : 1); v++, k++) {
            const haf_frame &f = frames[k];
            const bool xyz = f.kind == HAF_FRAME_XYZ_F32;
            FrameDev &fd = q.h_frames[k];
            fd = describe_frame(f, !xyz ? e->raw.dev.p + raw : views ? e->raw_xyz.dev.p + raw_xyz : reinterpret_cast<const char *>(q.h_clouds[b].xyz));
            fd.dst = const_cast<float *>(q.h_clouds[b].xyz);
            fd.count = views ? const_cast<int *>(&q.d_clouds[b].n) : nullptr;
            (xyz ? raw_xyz : raw) += staged_bytes(f);
        }
    }
    if (roi_views) roi_describe_views(e, *q.from.roi, frames, views, B, R, c.grid_h, c.grid_w, q.d_geo, q.h_roi_views);
}

// Host frames go to the device as upload_clouds sends host clouds, in pieces, the DMA engine moving one while the host packs the rows
// of the next (upload_frame, engine_stage.cpp).  Then ONE launch per kind writes the points of every frame of the batch (frames.hip).
static int upload_frames(haf_engine *e, const Request &q)
{
    const hipStream_t s = q.s;
    const bool views = q.from.views != nullptr;
    HIPCHK(e, hipMemcpyAsync(e->in_block.dev.p, e->in_block.host, q.pts_off, hipMemcpyHostToDevice, s));      // the three header arrays
    for (int b = 0; b < q.n_frames; b++) {
        const haf_frame &f = q.from.frames[b];
        if (f.on_device == 1) continue;
        const bool xyz = f.kind == HAF_FRAME_XYZ_F32;
        char *const dev = !xyz ? e->raw.dev.p : views ? e->raw_xyz.dev.p : e->in_block.dev.p, *const host = !xyz ? e->raw.host : views ? e->raw_xyz.host : e->in_block.host;
        const size_t at = (size_t)(static_cast<const char *>(q.h_frames[b].src) - dev);      // the frame's place in its block, device and pinned alike
        if (const int rc = upload_frame(e, f, host + at, dev + at, s)) return rc;
    }
    if (!views) {
        launch_frame_points(q.d_frames, q.h_frames, q.n_frames, s);      // (a frame per request; one for all of them in an objects call)
        return HAF_OK;
    }
    launch_view_points(q.d_frames, q.h_frames, q.n_frames, s);
    // the live counts, for n_points and the debug fetch: the CloudDev array back into the pinned header, where the host's copy of
    // CloudDev::n lies.  The call's own synchronisation (vote_and_wait) completes it: no wait here
    HIPCHK(e, hipMemcpyAsync(e->in_block.host, e->in_block.dev.p, (size_t)q.B * sizeof(CloudDev), hipMemcpyDeviceToHost, s));
    return HAF_OK;
}

// Host clouds go through the pinned block in pieces: while the DMA engine moves one piece the host packs the next (a 1.2 MB
// cloud -- C3 -- costs ~100 us of host memcpy; its transfer hides behind that).  The first copy carries the two header arrays.
static int upload_clouds(haf_engine *e, const haf_cloud *clouds, const Request &q)
{
    const hipStream_t s = q.s;
    const size_t pts_off = q.pts_off;
    size_t staged = 0, sent = 0;                              // bytes of the points area packed / handed to the DMA engine
    bool header_sent = false;
    auto flush = [&]() -> int {
        if (!header_sent) {
            HIPCHK(e, hipMemcpyAsync(e->in_block.dev.p, e->in_block.host, pts_off + staged, hipMemcpyHostToDevice, s));
            header_sent = true;
        } else if (staged > sent) {
            HIPCHK(e, hipMemcpyAsync(e->in_block.dev.p + pts_off + sent, e->in_block.host + pts_off + sent, staged - sent, hipMemcpyHostToDevice, s));
        }
        sent = staged;
        return HAF_OK;
    };
    for (int b = 0; b < q.B; b++) {
        if (clouds[b].on_device == 1 || clouds[b].n_points == 0) continue;
        if (clouds[b].on_device == 2 && clouds[b].n_points * 12 >= kStagePiece) {
            // (a small cloud is cheaper packed into the one staged copy than as a DMA transfer of its own: ~10 us each)
            // page-locked caller memory: whatever has been packed so far goes out, then the DMA engine takes this cloud from
            // where it lies (the staging block keeps the same layout, its share of it stays unused)
            const int rc = flush();
            if (rc != HAF_OK) return rc;
            const size_t bytes = clouds[b].n_points * 12;
            HIPCHK(e, hipMemcpyAsync(e->in_block.dev.p + pts_off + staged, clouds[b].xyz, bytes, hipMemcpyHostToDevice, s));
            staged += bytes;
            sent = staged;
            continue;
        }
        const float *src = clouds[b].xyz;
        const size_t st = clouds[b].stride_floats, n = clouds[b].n_points;
        for (size_t i0 = 0; i0 < n;) {
            const size_t room = std::max<size_t>(1, (kStagePiece - (staged - sent)) / 12);
            const size_t cnt = std::min(n - i0, room);
            float *dst = reinterpret_cast<float *>(e->in_block.host + pts_off + staged);
            if (st == 3) memcpy(dst, src + i0 * 3, cnt * 12);
            else for (size_t i = 0; i < cnt; i++) { dst[i * 3] = src[(i0 + i) * st]; dst[i * 3 + 1] = src[(i0 + i) * st + 1]; dst[i * 3 + 2] = src[(i0 + i) * st + 2]; }
            staged += cnt * 12;
            i0 += cnt;
            if (staged - sent >= kStagePiece) { const int rc = flush(); if (rc != HAF_OK) return rc; }
        }
    }
    return flush();
}

static void classify_request(const haf_engine *e, const haf_grasp_input *in, Request &q)
{
    const int B = q.B, R = q.R, H = e->cfg.grid_h, W = e->cfg.grid_w;
    Dims &d = q.d;
    d.H = H; d.W = W; d.R = R; d.B = B; d.nf = e->mdl.nf; d.n_sv = e->model.n_sv; d.n_sv_tiles = e->mdl.n_sv_tiles; d.sv_tile_neg = e->mdl.sv_tile_neg;
    haf_pick_math::cell_reach(H, W, &q.r_row, &q.r_col);
    q.evals_cap = (long)B * R * (H - 14) * (W - 14);
    // For choosing between the feature kernels only: the masked cells of a roll lie inside the rotated search rectangle of
    // half sizes sx/2 - 7, sy/2 - 7 (pnt_in_box 687-688), at most (a + 2)(b + 2) lattice points for sides a, b -- usually far
    // fewer than the grid could hold (the client's default 32 x 44 area on the 56 x 56 grid: a third).
    for (int b = 0; b < B; b++) {
        const long a2 = std::max(0, 2 * ((int)in[b].grasp_area_length_x / 2 - 7)) + 2, b2 = std::max(0, 2 * ((int)in[b].grasp_area_length_y / 2 - 7)) + 2;
        long sel = std::min<long>((long)(H - 14) * (W - 14), a2 * b2);
        // an ROI request with a HOST mask: a masked pixel puts at most the 29 cells of the vote's footprint on a roll's list (the mask is
        // an argument of the call: identical calls still take identical paths; a device-resident mask keeps the area bound)
        if (q.from.roi && q.from.roi->masked[(size_t)b] >= 0) sel = std::min<long>(sel, 29 * q.from.roi->masked[(size_t)b]);
        q.evals_sel += (long)R * sel;
    }
    const long work = q.evals_sel * (long)e->mdl.n_sv_pad;
    // A request whose whole SVM work is tiny goes straight to the fp64 MFMA tier (every evaluation enters its list): same
    // labels by construction -- the tier decides outside its own band and hands the rest to the strict tier -- and three
    // launches instead of a feature kernel, a contraction kernel and the rechecks behind them.
    q.direct = !e->mdl.prob_mode && !e->generic_kernel && e->direct_work > 0 && work <= e->direct_work;
    q.short_request = work <= (1L << 26) && q.total_n <= (1L << 20);
    // A small engine with a small model behind one of the fast contractions: what that contraction flags goes through the SAME one-launch
    // kernel in list mode (exact attributes + fp64 MFMA decision, tier 2's arithmetic) instead of tier 2a's three launches and tier 2's
    // three -- at a few thousand evaluations x a few hundred SVs the six launches and two more attribute kernels cost more than the
    // exact work (C3: 81 -> 30 us; the kernel costs ~9 ns per listed evaluation at 192 SVs, so it wins up to ~8 000 of them: a request
    // of up to 2^25 evaluation x SV pairs, of which a trained model flags around a tenth).  Decided from the request's search areas and
    // the model's size, so identical calls take identical paths.
    q.small_exact = !q.direct && !e->mdl.prob_mode && e->direct_work > 0 && work <= 16 * e->direct_work;
    q.large = q.evals_sel >= e->large_evals;              // enough evaluations to fill the chip with one thread each
}

static int run_prestages(haf_engine *e, Request &q)
{
    const haf_config &c = e->cfg;
    const hipStream_t s = q.s;
    const Dims &d = q.d;
    // (the counters were zeroed behind the previous request's copy-out; after an error they may not have been)
    if (!e->counters_clean) HIPCHK(e, hipMemsetAsync(e->d_counters.p, 0, CNT_COUNT * sizeof(int), s));
    e->counters_clean = false;
    if (e->d_attr.p) HIPCHK(e, hipMemsetAsync(e->d_attr.p, 0xFF, e->d_attr.n * sizeof(AttrRecord), s));   // debug: "not computed"
    mark(e, HAF_ST_BIN);
    // small grids: a1 (tail) + a2 + a3 + a4 in ONE launch (k_small_pre); the probability branch needs k_scan's row-major order
    // (an ROI request, of frames or of views, takes the general pre-stage kernels, which serve small grids too: k_small_pre stays what it is)
    int fused_bin = -1;
    if (!e->mdl.prob_mode && !e->no_fused_pre && !q.from.roi)
        fused_bin = launch_small_pre(q.d_clouds, q.d_geo, q.max_n, e->d_heights.p, e->d_ii.p, e->d_mask.p, e->d_rowcount.p, e->d_brcount.p,
                                     e->d_labels.p, e->d_evalcell.p, e->d_counters.p, e->d_flag_list.p, q.direct, d, q.r_row, q.r_col, s,
                                     e->d_brslot.p, ++e->pre_epoch);
    q.fused_pre = fused_bin >= 0;
    if (q.fused_pre) {
        e->pre_forms = PrestageForms{fused_bin, INTEGRAL_FUSED, false};
        mark(e, HAF_ST_INTEGRAL);
        mark(e, HAF_ST_MASK);
        return HAF_OK;
    }
    HIPCHK(e, hipMemsetAsync(e->d_labels.p, 0xFF, (size_t)q.B * q.R * d.H * d.W, s));   // -1: no feature vector for this cell (server.cpp:828-829)
    BinScratch bs{};
    bs.sorted = e->d_sorted.p; bs.sorted_cap = e->d_sorted.p ? (long)c.max_points : 0;
    bs.bkt_count = e->d_bkt.p; bs.bkt_off = e->d_bkt.p ? e->d_bkt.p + (size_t)c.max_clouds * e->bkt_ints : nullptr;
    bs.bkt_cursor = e->d_bkt.p ? e->d_bkt.p + (size_t)2 * c.max_clouds * e->bkt_ints : nullptr;
    bs.bkt_cap = e->d_bkt.p ? c.max_clouds * e->bkt_ints : 0;
    const BinChoice bin = launch_bin(q.d_clouds, q.h_clouds, q.max_n, q.total_n, q.d_geo, e->d_heights.p, d, q.r_row, q.r_col,
                                     q.bucket_ok && !e->no_bucket_sort, bs, e->d_counters.p, s);
    mark(e, HAF_ST_INTEGRAL);
    const int integral = launch_integral(e->d_heights.p, e->d_rowsum.p, e->d_ii.p, e->d_inexact.p, e->d_counters.p, d, s, e->mdl.lr_available ? e->d_iiabs.p : nullptr);
    e->pre_forms = PrestageForms{bin.form, integral, bin.bucket_refused};
    mark(e, HAF_ST_MASK);
    if (q.from.objects) {
        const int rc = objects_mark_cells(e, *q.from.objects, q.from.frames[0], q.h_clouds, q.d_geo, d, q.r_row, q.r_col, s);
        if (rc != HAF_OK) return rc;
        launch_mask_count_roi(e->d_ii.p, q.d_geo, e->d_roi_cells.p, e->d_mask.p, e->d_rowcount.p, d, s);
    } else if (q.from.roi) {
        const RoiViews rv{q.d_frames, q.h_frames, q.d_roi_views, q.h_roi_views, q.n_frames};
        const int rc = roi_mark_cells(e, *q.from.roi, q.from.frames, q.h_clouds, q.d_geo, d, q.r_row, q.r_col, s, q.from.views ? &rv : nullptr);
        if (rc != HAF_OK) return rc;
        launch_mask_count_roi(e->d_ii.p, q.d_geo, e->d_roi_cells.p, e->d_mask.p, e->d_rowcount.p, d, s);
    } else {
        launch_mask_count(e->d_ii.p, q.d_geo, e->d_mask.p, e->d_rowcount.p, d, s);
    }
    launch_scan(e->d_rowcount.p, e->d_rowoff.p, e->d_brcount.p, e->d_counters.p, d, s);
    launch_compact(e->d_mask.p, e->d_rowcount.p, e->d_rowoff.p, e->d_evalcell.p, d, s);
    if (q.direct) launch_prob_list(e->d_counters.p, CNT_FLAGGED, e->d_flag_list.p, e->list_cap, s);
    return HAF_OK;
}

static TierFacts tier_facts(const haf_engine *e, const Request &q, int mode, bool reuse_operands)
{
    return TierFacts{e->screen_variant, e->mdl.cr_available, e->mdl.lr_available, e->lr_enabled, e->mdl.lr_plain_available, e->mdl.lr_fused,
                     e->use_t0b, e->t1_skip, e->mdl.t1_cr_available, e->mdl.i8_active, e->calibrated, e->short_gate, e->generic_kernel,
                     e->model.n_sv, test_env("HAF_T0B_NO_GATHER") != nullptr, mode, reuse_operands, q.direct, q.small_exact, q.large,
                     q.fused_pre, (long)q.d.H * q.d.W, q.evals_cap};
}

// Testing library only (haf_test_snapshot_screen): what sweep launch `slot` (0 the first pass, 1 tier 0b) of this request left, copied
// aside on the request's stream right behind the launch -- dec, margin, the flag words, the output list, the counters and, in the PART
// form, the partial sums.  The buffers are sized by haf_test_snapshot_screen; nothing happens while the snapshot is off.
static void snapshot_sweep(haf_engine *e, int slot, const SweepForm &form, long cap, long evals_cap, int out_l, hipStream_t s)
{
    haf_engine::SweepSnap &sn = e->snap_sweep[slot];
    sn.form = form;
    sn.cap = sn.dec_cap = sn.list_cap = sn.part_bytes = sn.raw_cap = sn.y_bytes = 0;
    if (!e->snap_on || form.variant < 0 || !sn.dec.p) return;
    cap = std::min<long>(std::min<long>(cap, e->max_evals_pad), (long)sn.dec.n);
    const long pad = std::min<long>((cap + kS0BlockEvals - 1) / kS0BlockEvals * kS0BlockEvals, (long)sn.dec.n);
    sn.cap = cap;
    // (dec and margin go by evaluation id in every launch, a list launch's too: the request's evaluation slots, not the list's)
    sn.dec_cap = std::min<long>(std::min<long>(evals_cap, e->max_evals_pad), (long)std::min(sn.dec.n, e->d_dec.n));
    (void)hipMemcpyAsync(sn.dec.p, e->d_dec.p, (size_t)sn.dec_cap * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e->d_margin.p && sn.margin.p)
        (void)hipMemcpyAsync(sn.margin.p, e->d_margin.p, std::min<size_t>((size_t)sn.dec_cap, std::min(sn.margin.n, e->d_margin.n)) * sizeof(float), hipMemcpyDeviceToDevice, s);
    (void)hipMemcpyAsync(sn.words.p, e->d_flag0_words.p, std::min<size_t>(std::min(sn.words.n, e->d_flag0_words.n), (size_t)(pad / 64)) * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s);
    (void)hipMemcpyAsync(sn.counters.p, e->d_counters.p, CNT_COUNT * sizeof(int), hipMemcpyDeviceToDevice, s);
    if (sn.labels.p) (void)hipMemcpyAsync(sn.labels.p, e->d_labels.p, std::min(sn.labels.n, e->d_labels.n), hipMemcpyDeviceToDevice, s);
    if (form.lr && sn.raw.p) {
        sn.raw_cap = std::min<long>(sn.dec_cap, (long)std::min(sn.raw.n, e->d_gband.n) / kBandFloats);
        (void)hipMemcpyAsync(sn.raw.p, e->d_gband.p, (size_t)sn.raw_cap * kBandFloats * sizeof(float), hipMemcpyDeviceToDevice, s);
        if (!form.fused && sn.Y.p) {
            // (k_project's images lie behind the 10-step images of the engine's largest request: launch_screening's y_img)
            const size_t off = (size_t)(e->max_evals_pad / kTile) * (size_t)kS0MatBytes, have = e->d_X.n * sizeof(float);
            const size_t want = (size_t)((sn.dec_cap + kTile - 1) / kTile) * (size_t)kLrMatBytes;
            sn.y_bytes = (long)std::min(std::min(want, sn.Y.n), have > off ? have - off : 0);
            (void)hipMemcpyAsync(sn.Y.p, reinterpret_cast<const char *>(e->d_X.p) + off, (size_t)sn.y_bytes, hipMemcpyDeviceToDevice, s);
        }
    }
    if (const int *out_list = list_buf(e, out_l)) {
        sn.list_cap = std::min<long>(e->flag0_cap, (long)std::min(sn.list.n, list_len(e, out_l)));
        (void)hipMemcpyAsync(sn.list.p, out_list, (size_t)sn.list_cap * sizeof(int), hipMemcpyDeviceToDevice, s);
    }
    if (form.part && e->d_screen_part.p && sn.part.p) {
        // (slice k of the launch lies at float4 index k * blocks * 256: the first kS0MaxParts slices of `blocks` workgroups are contiguous)
        sn.part_bytes = (long)std::min<size_t>(sn.part.n, std::min<size_t>(e->d_screen_part.n, (size_t)16 * form.blocks * kS0BlockEvals * 16));
        (void)hipMemcpyAsync(sn.part.p, e->d_screen_part.p, (size_t)sn.part_bytes, hipMemcpyDeviceToDevice, s);
    }
}

// the screening pass (tier 0), tier 0b, the short-list gate and tier 1 of a PATH_SCREEN plan
static void launch_screening(haf_engine *e, const Request &q, const TierPlan &p)
{
    const hipStream_t s = q.s;
    const Dims &d = q.d;
    const long evals_cap = q.evals_cap;
    ScreenParams sp_now = p.sp == SP_LRP ? e->mdl.screen_lrp : p.sp == SP_CR ? e->mdl.screen_cr : e->mdl.screen;
    if (p.sp != SP_LRP) sp_now.cr_poly = e->screen_variant == SCREEN_CR_POLY;
    if (p.lr) { sp_now.lr = 1; sp_now.lr_negflags = e->d_inexact.p; sp_now.lr_iiabs = e->d_iiabs.p; }
    if (e->snap_on && !p.reuse) { e->feature_sp_kind = p.sp; e->feature_sp = sp_now; }      // (testing library only, as the snapshot below)
    if (!p.reuse)
        e->feature_form = launch_features(e->d_ii.p, e->d_evalcell.p, e->d_counters.p, e->mdl.fd.p, e->d_X.p, e->d_gband.p, d, e->range.lower,
                                          e->range.upper, e->mdl.svm.neg_gamma2, evals_cap, XMODE_SCREEN, sp_now, nullptr, 0, 0, q.large, q.evals_sel, nullptr, e->d_ax.p, s);
    if (e->snap_on && !p.reuse) {        // (testing library only: haf_test_snapshot_screen)
        const long cap = std::min<long>(evals_cap, e->max_evals_pad);
        e->snap_cap = cap;
        (void)hipMemcpyAsync(e->snap_X.p, e->d_X.p, (size_t)((cap + kTile - 1) / kTile) * (size_t)kS0MatBytes, hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(e->snap_gband.p, e->d_gband.p, (size_t)cap * kBandFloats * sizeof(float), hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(e->snap_ax.p, e->d_ax.p, (size_t)cap * sizeof(float), hipMemcpyDeviceToDevice, s);
    }
    char *y_img = reinterpret_cast<char *>(e->d_X.p) + (size_t)(e->max_evals_pad / kTile) * (size_t)kS0MatBytes;   // behind the 10-step images (the buffer holds the 42 KiB three-pass form)
    mark(e, HAF_ST_SVM);
    SweepForm form0, form1;
    if (p.lr && !e->mdl.lr_fused) launch_project(e->d_X.p, e->mdl.lr_btiles.p, y_img, e->d_gband.p, e->d_counters.p, evals_cap, s);   // (counted with the sweep it feeds)
    if (p.lr)
        form0 = launch_svm_screen_lr(e->mdl.lr_fused ? reinterpret_cast<char *>(e->d_X.p) : y_img, e->d_gband.p, e->d_ax.p, e->mdl.svt_lr.p, e->d_evalcell.p, e->d_counters.p, e->mdl.svm, e->d_dec.p, e->d_labels.p,
                             e->d_flag0_words.p, e->d_flag0_wgcount.p, list_buf(e, p.pass0_out), e->flag0_cap, e->d_counters.p, d,
                             evals_cap, e->d_margin.p, e->screen_variant, e->mdl.crp, e->mdl.lr_band, s, handover_counter(p.pass0_out),
                             e->mdl.lr_fused ? e->mdl.lr_btiles_in.p : nullptr);
    else
        form0 = launch_svm_screen(e->d_X.p, e->d_gband.p, e->d_ax.p, p.cr ? e->mdl.svt0_cr.p : e->mdl.svt0.p, e->d_evalcell.p, e->d_counters.p, e->mdl.svm, e->d_dec.p, e->d_labels.p,
                          e->d_flag0_words.p, e->d_flag0_wgcount.p, list_buf(e, p.pass0_out), e->flag0_cap, e->d_counters.p, d, evals_cap, e->d_margin.p,
                          e->screen_variant, e->mdl.crp, s, handover_counter(p.pass0_out), nullptr, CNT_EVALS, CNT_FLAGGED0, e->d_screen_part.p, e->screen_parts);
    snapshot_sweep(e, 0, form0, evals_cap, evals_cap, p.pass0_out, s);
    mark(e, HAF_ST_REFINE);
    const long list_cap = std::min<long>(e->flag0_cap, evals_cap);
    if (p.t0b == T0B_GATHER) {
        form1 = launch_svm_screen_lr(reinterpret_cast<char *>(e->d_X.p), e->d_gband.p, e->d_ax.p, e->mdl.svt_lr.p, e->d_evalcell.p, e->d_counters.p, e->mdl.svm, e->d_dec.p,
                             e->d_labels.p, e->d_flag0_words.p, e->d_flag0_wgcount.p, list_buf(e, p.t0b_out), e->flag0_cap,
                             e->d_counters.p, d, list_cap, e->d_margin.p, SCREEN_CR_EXP, e->mdl.crp, e->mdl.lr_band, s, handover_counter(p.t0b_out),
                             e->mdl.lr_btiles_in.p, list_buf(e, p.t0b_in), list_counter(p.t0b_in), CNT_FLAGGED0B);
    } else if (p.t0b == T0B_FEATURES) {
        // tier 0b: the centred-remainder form on the LIST of the first pass (its own operand images: translated attributes,
        // centred support vectors; band, common factor and images indexed by list slot)
        ScreenParams sp_b = e->mdl.screen_cr;
        sp_b.cr_poly = 0;
        // (the group-parallel feature kernel even for lists of 10^5: one evaluation per lane on SCATTERED cells -- k_features_serial in
        // list mode -- was measured at 7.7 ns per evaluation against 2.1 ns, its 2 400 corner loads per lane being 64 separate
        // L1 accesses each)
        launch_features(e->d_ii.p, e->d_evalcell.p, e->d_counters.p, e->mdl.fd.p, e->d_X1.p, e->d_gband.p, d, e->range.lower,
                        e->range.upper, e->mdl.svm.neg_gamma2, list_cap, XMODE_SCREEN, sp_b, list_buf(e, p.t0b_in), list_counter(p.t0b_in), e->flag0_cap,
                        false, list_cap, nullptr, e->d_ax.p, s);
        if (e->snap_on && e->snap_sweep[1].in_X.p) {         // (testing library only: tier 0b's own, list-indexed feature output)
            haf_engine::SweepSnap &sn = e->snap_sweep[1];
            const size_t tiles = std::min<size_t>((size_t)((list_cap + kTile - 1) / kTile), sn.in_X.n / (size_t)kS0MatBytes);
            const size_t slots = std::min<size_t>((size_t)list_cap, sn.in_ax.n);
            (void)hipMemcpyAsync(sn.in_X.p, e->d_X1.p, tiles * (size_t)kS0MatBytes, hipMemcpyDeviceToDevice, s);
            (void)hipMemcpyAsync(sn.in_gband.p, e->d_gband.p, slots * kBandFloats * sizeof(float), hipMemcpyDeviceToDevice, s);
            (void)hipMemcpyAsync(sn.in_ax.p, e->d_ax.p, slots * sizeof(float), hipMemcpyDeviceToDevice, s);
        }
        form1 = launch_svm_screen(e->d_X1.p, e->d_gband.p, e->d_ax.p, e->mdl.svt0_cr.p, e->d_evalcell.p, e->d_counters.p, e->mdl.svm, e->d_dec.p, e->d_labels.p,
                          e->d_flag0_words.p, e->d_flag0_wgcount.p, list_buf(e, p.t0b_out), e->flag0_cap, e->d_counters.p, d,
                          list_cap, e->d_margin.p, SCREEN_CR_EXP, e->mdl.crp, s, handover_counter(p.t0b_out), list_buf(e, p.t0b_in), list_counter(p.t0b_in),
                          CNT_FLAGGED0B, e->d_screen_part.p, e->screen_parts);
    }
    snapshot_sweep(e, 1, form1, list_cap, evals_cap, p.t0b_out, s);
    // (the gate's count goes to CNT_FLAGGEDI only when it writes the exact-integer tier's output list)
    if (p.gate)
        launch_short_list_gate(e->d_counters.p, list_counter(p.gate_in), list_buf(e, p.gate_in), e->flag0_cap, list_buf(e, p.gate_out),
                               CNT_FLAGGEDI, p.gate_out == L_FLAGI, std::min(kShortListGate, e->flag_cap), s);
    if (!p.t1) return;
    // (the list is short whenever screening is worth its while: always the group-parallel feature kernel, whose
    // workgroups beyond the list's end exit at once)
    ScreenParams sp_t1 = e->mdl.screen;
    if (p.t1cr) { sp_t1.cr_t1_tab = e->mdl.t1_tab.p; sp_t1.cr_t1_L = e->d_t1_L.p; }
    launch_features(e->d_ii.p, e->d_evalcell.p, e->d_counters.p, e->mdl.fd.p, e->d_X1.p, e->d_ax1.p, d, e->range.lower,
                    e->range.upper, e->mdl.svm.neg_gamma2, list_cap, XMODE_SPLIT, sp_t1, list_buf(e, p.t1_in), p.t1_cnt,
                    e->flag0_cap, false, list_cap, e->d_attr.p, nullptr, s);
    launch_svm_h(e->d_X1.p, e->d_ax1.p, p.t1cr ? e->mdl.svt_h_cr.p : e->mdl.svt_h.p, e->d_evalcell.p, e->d_counters.p, e->mdl.svm, e->d_dec.p, e->d_labels.p,
                 list_buf(e, p.t1_out), e->list_cap, e->d_counters.p, d, list_cap, list_buf(e, p.t1_in), p.t1_cnt, e->flag0_cap,
                 e->d_part1.p, e->part1_stride, s, p.t1cr ? &e->mdl.crt1 : nullptr, p.t1cr ? e->d_t1_L.p : nullptr, e->d_t1_flags.p);
}

// the first pass of every other path: the generic / direct tier, or a contraction over every evaluation
static void launch_first_pass(haf_engine *e, const Request &q, const TierPlan &p)
{
    const hipStream_t s = q.s;
    const Dims &d = q.d;
    if (p.path == PATH_GENERIC) {
        launch_prob_list(e->d_counters.p, list_counter(p.pass0_out), list_buf(e, p.pass0_out), e->list_cap, s);
        launch_recheck(e->d_ii.p, e->d_evalcell.p, e->mdl.fd.p, e->mdl.sv64.p, e->mdl.coef64.p, e->mdl.exact, list_buf(e, p.strict_in), e->list_cap,
                       e->d_counters.p, list_counter(p.strict_in), e->d_dec_exact2.p, e->d_labels.p, d, s);
        mark(e, HAF_ST_SVM);
    } else if (p.path == PATH_DIRECT) {
        // every evaluation counts as rechecked (k_small_pre / k_prob_list have put them on the exact tier's list)
        launch_small_direct(e->d_ii.p, e->d_evalcell.p, e->d_counters.p, e->mdl.fd.p, e->mdl.sv64.p, e->mdl.exact, d, std::min<long>(q.evals_cap, e->list_cap),
                            e->d_dec_exact.p, e->d_labels.p, list_buf(e, p.pass0_out), e->list_cap, e->d_attr.p, s);
        mark(e, HAF_ST_SVM);
    } else if (p.path == PATH_SPLIT) {
        launch_features(e->d_ii.p, e->d_evalcell.p, e->d_counters.p, e->mdl.fd.p, e->d_X.p, e->d_ax.p, d, e->range.lower,
                        e->range.upper, e->mdl.svm.neg_gamma2, q.evals_cap, XMODE_SPLIT, e->mdl.screen, nullptr, 0, 0, q.large, q.evals_sel, e->d_attr.p, nullptr, s);
        mark(e, HAF_ST_SVM);
        launch_svm_h(e->d_X.p, e->d_ax.p, e->mdl.svt_h.p, e->d_evalcell.p, e->d_counters.p, e->mdl.svm, e->d_dec.p, e->d_labels.p,
                     list_buf(e, p.pass0_out), e->list_cap, e->d_counters.p, d, q.evals_cap, nullptr, 0, 0, nullptr, 0, s, nullptr, nullptr, e->d_t1_flags.p);
    } else {
        launch_features(e->d_ii.p, e->d_evalcell.p, e->d_counters.p, e->mdl.fd.p, e->d_X.p, e->d_ax.p, d, e->range.lower,
                        e->range.upper, e->mdl.svm.neg_gamma2, q.evals_cap, XMODE_F32, e->mdl.screen, nullptr, 0, 0, q.large, q.evals_sel, e->d_attr.p, nullptr, s);
        mark(e, HAF_ST_SVM);
        launch_svm(e->d_X.p, e->d_ax.p, e->mdl.svt.p, e->d_evalcell.p, e->d_counters.p, e->mdl.svm, e->d_dec.p, e->d_labels.p,
                   list_buf(e, p.pass0_out), e->list_cap, e->d_counters.p, d, q.evals_cap, s, e->d_t1_flags.p);
    }
    mark(e, HAF_ST_REFINE);
}

// One window [off, off + flag_cap) of the exact tiers' input lists.  Tier 2: fp64 MFMA (GEMM form) for the guard band of the fast
// contraction; tier 2a in front of it: the exact-integer tier (plan_tiers)
static void fp64_window(haf_engine *e, const Request &q, const TierPlan &p, int off)
{
    if (p.fp64 == FP64_SMALL)
        launch_small_direct(e->d_ii.p, e->d_evalcell.p, e->d_counters.p, e->mdl.fd.p, e->mdl.sv64.p, e->mdl.exact, q.d, e->flag_cap, e->d_dec_exact.p,
                            e->d_labels.p, list_buf(e, p.fp64_out), e->list_cap, nullptr, q.s, list_buf(e, p.fp64_in), list_counter(p.fp64_in), off);
    else
        launch_recheck_mfma(e->d_ii.p, e->d_evalcell.p, e->mdl.fd.p, e->mdl.sv64.p, e->mdl.exact, list_buf(e, p.fp64_in), e->flag_cap, off, e->d_counters.p,
                            e->d_x64.p, e->d_part64.p, p.i8 ? e->d_dec_exacti.p : e->d_dec_exact.p, e->d_labels.p, list_buf(e, p.fp64_out), e->list_cap,
                            q.d, q.s, nullptr, false, list_counter(p.fp64_in), e->d_tier_words.p);
}
static void i8_window(haf_engine *e, const Request &q, const TierPlan &p, int off)
{
    launch_recheck_i8(e->d_ii.p, e->d_evalcell.p, e->mdl.fd.p, e->mdl.sv_i8.p, e->mdl.i8, e->range.lower, e->range.upper, list_buf(e, p.i8_in), e->flag_cap,
                      off, e->d_counters.p, e->d_x64.p, e->d_part64.p, e->d_dec_exact.p, e->d_labels.p, list_buf(e, p.i8_out), e->list_cap, q.d, q.s,
                      e->d_tier_words.p);
}

// the vote, then the counters and the roll records to the host (one copy), and the wait for them
static int vote_and_wait(haf_engine *e, const Request &q)
{
    const hipStream_t s = q.s;
    mark(e, HAF_ST_VOTE);
    if (q.from.roi)
        launch_vote_roi(e->d_labels.p, reinterpret_cast<const float *>(e->d_heights.p), e->d_brcount.p, e->d_ev16.p, e->d_topkey.p, e->d_rowmax.p,
                        e->d_rec.p, e->d_roi_cells.p, q.d, s);
    else
        launch_vote(e->d_labels.p, reinterpret_cast<const float *>(e->d_heights.p), e->d_brcount.p, e->d_ev16.p, e->d_topkey.p, e->d_rowmax.p, e->d_rec.p, q.d, s);
    mark(e, HAF_ST_DOWNLOAD);
    HIPCHK(e, hipMemcpyAsync(e->out_block.host, e->out_block.dev.p, kCntBytes + (size_t)q.B * q.R * sizeof(RollRecordDev), hipMemcpyDeviceToHost, s));   // counters + records
    mark(e, HAF_ST_COUNT);
    // a short request (tens to hundreds of microseconds on the device) is waited for by polling: the wake-up of a
    // blocked host thread costs more than the request's last kernels
    if (q.short_request) {
        hipError_t r;
        while ((r = hipStreamQuery(s)) == hipErrorNotReady) __builtin_ia32_pause();   // (spin politely: the sibling hyper-thread may be the driver's)
        HIPCHK(e, r);
    } else {
        HIPCHK(e, hipStreamSynchronize(s));
    }
    HIPCHK(e, hipGetLastError());
    return HAF_OK;
}

// What the counters that came back with the roll records ask for: the exact tiers' further windows, the strict tier, the host
static int finish_exact_tiers(haf_engine *e, Request &q, const TierPlan &p)
{
    const hipStream_t s = q.s;
    int rc = HAF_OK;
    bool strict_ran = false;
    q.host_resolved = 0;
    const int flagged = e->h_counters[CNT_FLAGGED];
    const bool lists_valid = p.fp64 != FP64_NONE && !(p.path == PATH_SCREEN && e->h_counters[CNT_FLAGGED0] > e->flag0_cap);
    const bool more_i8 = lists_valid && p.i8 && flagged > e->flag_cap;
    const bool more_fp64 = lists_valid && e->h_counters[list_counter(p.fp64_in)] > e->flag_cap;
    if (more_i8 || more_fp64) {
        // More evaluations inside a guard band than one window of an exact tier holds (an ill-conditioned model): the
        // reference never fails a goal on this path (server.cpp:778-796), so neither does the engine -- the remaining
        // windows of the lists go through the same kernels one after the other, then the strict tier over its whole list,
        // then the vote again.  Slower, same labels.
        int done_fp64 = e->flag_cap;                  // entries of its list the fp64 tier has seen (window 0)
        if (more_i8) {
            for (int off = e->flag_cap; off < flagged; off += e->flag_cap) { i8_window(e, q, p, off); e->stat_extra_windows++; }
            // the fp64 tier's list has grown behind its first window: all of it again from the start (its results and the
            // strict tier's list are rebuilt; both are idempotent)
            HIPCHK(e, hipMemsetAsync(e->d_counters.p + list_counter(p.fp64_out), 0, sizeof(int), s));
            HIPCHK(e, hipMemcpyAsync(e->out_block.host, e->out_block.dev.p, kCntBytes, hipMemcpyDeviceToHost, s));
            HIPCHK(e, hipStreamSynchronize(s));
            done_fp64 = 0;
        }
        const int n_fp64 = e->h_counters[list_counter(p.fp64_in)];
        for (int off = done_fp64; off < n_fp64; off += e->flag_cap) { fp64_window(e, q, p, off); e->stat_extra_windows++; }
        launch_recheck(e->d_ii.p, e->d_evalcell.p, e->mdl.fd.p, e->mdl.sv64.p, e->mdl.coef64.p, e->mdl.exact, list_buf(e, p.strict_in), e->list_cap,
                       e->d_counters.p, list_counter(p.strict_in), e->d_dec_exact2.p, e->d_labels.p, q.d, s);
        if ((rc = vote_and_wait(e, q)) != HAF_OK) return rc;
        strict_ran = e->h_counters[list_counter(p.strict_in)] > 0;
    } else if (p.path == PATH_GENERIC) {
        strict_ran = true;                            // (it has run, on everything; what is left is the C library's tanh near zero)
    } else if (e->h_counters[list_counter(p.strict_in)] > 0) {
        // (the host knows the list's length here: the spread form of the tier, recheck.hip)
        launch_recheck_known(e->d_ii.p, e->d_evalcell.p, e->mdl.fd.p, e->mdl.sv64.p, e->mdl.coef64.p, e->mdl.exact, list_buf(e, p.strict_in),
                             std::min(e->h_counters[list_counter(p.strict_in)], e->list_cap), e->d_strict_terms.p, kStrictSlots, e->d_dec_exact2.p,
                             e->d_labels.p, q.d, s);
        if ((rc = vote_and_wait(e, q)) != HAF_OK) return rc;
        strict_ran = true;
    }
    if (strict_ran) {
        // what the strict tier left within a last-bit exp error of zero: glibc's exp on the host, then the vote once more
        bool changed = false;
        if ((rc = host_resolve_strict(e, q.d, s, &changed, &q.host_resolved)) != HAF_OK) return rc;
        if (changed && (rc = vote_and_wait(e, q)) != HAF_OK) return rc;
    }
    return HAF_OK;
}

// features -> decision tiers -> vote -> records on the host, for one contraction mode
static int decide(haf_engine *e, Request &q, int mode, bool reuse_operands)
{
    mark(e, HAF_ST_FEATURES);
    const TierPlan p = plan_tiers(tier_facts(e, q, mode, reuse_operands));
    if (p.path == PATH_SCREEN) {
        q.lr_used = p.lr;
        launch_screening(e, q, p);
    } else {
        launch_first_pass(e, q, p);
    }
    q.t0b_used = p.t0b != T0B_NONE;
    q.i8_used = p.i8;
    mark(e, HAF_ST_RECHECK);
    // Window 0 of the exact tiers' lists goes with every request; the strict tier (libsvm's order, for what is still within 2^-40 of
    // zero: practically nothing) is launched only when the counters that come back with the roll records say it has work
    if (p.fp64 != FP64_NONE) {
        if (p.i8) i8_window(e, q, p, 0);
        fp64_window(e, q, p, 0);
    }
    const int rc = vote_and_wait(e, q);
    if (rc != HAF_OK) return rc;
    return finish_exact_tiers(e, q, p);
}

// probability-output mode: every evaluation through the strict tier (libsvm's own order), then svm_predict_probability,
// the output lines as show_predicted_gps reads them, the fp32 vote (prob.hip)
static int decide_probability(haf_engine *e, Request &q)
{
    const hipStream_t s = q.s;
    const Dims &d = q.d;
    mark(e, HAF_ST_FEATURES); mark(e, HAF_ST_SVM); mark(e, HAF_ST_REFINE); mark(e, HAF_ST_RECHECK);
    launch_prob_list(e->d_counters.p, CNT_FLAGGED2, e->d_flag2_list.p, e->list_cap, s);
    launch_recheck(e->d_ii.p, e->d_evalcell.p, e->mdl.fd.p, e->mdl.sv64.p, e->mdl.coef64.p, e->mdl.exact, e->d_flag2_list.p, e->list_cap,
                   e->d_counters.p, CNT_FLAGGED2, e->d_dec_exact2.p, e->d_labels.p, d, s);
    // the estimates; those a last-bit exp difference could move come back as a list and are finished on the host (round 4)
    launch_probability_eval(e->d_dec_exact2.p, e->d_evalcell.p, e->d_counters.p, e->mdl.prob, e->d_labels.p, e->d_own.p, e->d_ptext.p,
                            e->d_flag_list.p, e->list_cap, e->d_counters.p, q.evals_cap, s);
    HIPCHK(e, hipMemcpyAsync(e->out_block.host, e->out_block.dev.p, kCntBytes, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    const int rc = host_resolve_probability(e, d, s, &q.host_resolved);
    if (rc != HAF_OK) return rc;
    mark(e, HAF_ST_VOTE);
    launch_probability(e->d_dec_exact2.p, e->d_evalcell.p, e->d_counters.p, e->mdl.prob, e->d_labels.p, e->d_mask.p, e->d_rowcount.p,
                       e->d_brcount.p, reinterpret_cast<const float *>(e->d_heights.p), e->d_own.p, e->d_ptext.p, e->d_gridf.p,
                       e->d_evf.p, e->d_rec.p, q.evals_cap, d, s);
    mark(e, HAF_ST_DOWNLOAD);
    HIPCHK(e, hipMemcpyAsync(e->out_block.host, e->out_block.dev.p, kCntBytes + (size_t)q.B * q.R * sizeof(RollRecordDev), hipMemcpyDeviceToHost, s));
    mark(e, HAF_ST_COUNT);
    HIPCHK(e, hipStreamSynchronize(s));
    HIPCHK(e, hipGetLastError());
    return HAF_OK;
}

// the next form of the screening pass to try when the one in use leaves too much undecided: PLAIN -> SUMSQ (the same operand
// images: only the decision stage is redone) -> CR_EXP -> CR_POLY (their own images) -> none
static int next_variant(const haf_engine *e, int v)
{
    if (v == SCREEN_PLAIN) return SCREEN_SUMSQ;
    if (v == SCREEN_SUMSQ && e->mdl.cr_available) return SCREEN_CR_EXP;
    if (v == SCREEN_CR_EXP) return SCREEN_CR_POLY;
    return -1;
}

// The adaptive choice of the screening form, behind a request that ran the screening pass (*mode: MODE_SPLIT when this request's
// labels came from the three-pass fallback)
static int adapt_screen_form(haf_engine *e, Request &q, int *mode, bool reprobe)
{
    auto undecided = [&]() { return e->h_counters[CNT_FLAGGED0]; };
    const int ne = e->h_counters[CNT_EVALS];
    // More undecided evaluations than the refinement list holds: this pass's labels are incomplete.  Remedy: the next form, and
    // stay with it; when none is left (or the variant is pinned by a test), the three-pass kernel for every evaluation of
    // this call (same labels by construction) -- and, unless pinned, no screening pass for this model from now on.
    if (undecided() > e->flag0_cap) e->stat_flag0_overflows++;
    while (undecided() > e->flag0_cap && !e->variant_forced && next_variant(e, e->screen_variant) >= 0) {
        const bool reuse = e->screen_variant == SCREEN_PLAIN && !q.t0b_used && !q.lr_used;     // (tier 0b writes its bands where the first pass's were; the low-rank form's images are the centred ones)
        e->screen_variant = next_variant(e, e->screen_variant);
        HIPCHK(e, hipMemsetAsync(e->d_counters.p + 1, 0, (CNT_COUNT - 1) * sizeof(int), q.s));
        const int rc = decide(e, q, MODE_SCREEN, reuse);
        if (rc != HAF_OK) return rc;
    }
    if (undecided() > e->flag0_cap) {
        if (!e->variant_forced) e->screen_active = false;
        *mode = MODE_SPLIT;
        HIPCHK(e, hipMemsetAsync(e->d_counters.p + 1, 0, (CNT_COUNT - 1) * sizeof(int), q.s));
        return decide(e, q, MODE_SPLIT, false);
    }
    if (reprobe) {
        const double share = ne > 0 ? (double)undecided() / (double)ne : 1.0;
        e->variant_share[e->screen_variant] = share;
        if (ne >= 256 && share <= 0.6) e->screen_active = true;
    } else if (ne >= 256 && !e->variant_forced && !e->variant_settled) {
        // Adaptive rule on real requests (an engine that was not calibrated, or whose calibration scene misjudged the model): a form
        // that leaves more than a quarter undecided makes room for the next untried one; when all have been seen the engine
        // settles on the one with the lowest cost -- or on none, if even that one leaves more than 60 %.
        const double share = (double)undecided() / (double)ne;
        e->variant_share[e->screen_variant] = share;
        if (share > 0.25) {
            int nv = next_variant(e, e->screen_variant);
            while (nv >= 0 && e->variant_share[nv] >= 0.0) nv = next_variant(e, nv);       // (already seen: at calibration or on a request)
            if (nv >= 0) {
                e->screen_variant = nv;
            } else {
                int best = e->screen_variant;
                double best_cost = 1e30;
                for (int v = 0; v < SCREEN_VARIANTS; v++) {
                    if (e->variant_share[v] < 0.0) continue;
                    const double cost = variant_cost(e, v) + kUndecidedCost * e->variant_share[v];
                    if (cost < best_cost) { best_cost = cost; best = v; }
                }
                e->screen_variant = best;
                e->variant_settled = true;
                if (e->variant_share[best] > 0.6) e->screen_active = false;
            }
        }
    }
    return HAF_OK;
}

// An ROI request says nothing about how the model behaves on whole requests: it neither judges nor changes the screening form.  Only
// when its screening pass left more undecided than the refinement list holds -- its labels are incomplete then -- the three-pass kernel
// decides every evaluation of THIS call (same labels by construction); the engine's choice stays as it was
static int roi_screen_overflow(haf_engine *e, Request &q, int *mode)
{
    if (e->h_counters[CNT_FLAGGED0] <= e->flag0_cap) return HAF_OK;
    e->stat_flag0_overflows++;
    *mode = MODE_SPLIT;
    HIPCHK(e, hipMemsetAsync(e->d_counters.p + 1, 0, (CNT_COUNT - 1) * sizeof(int), q.s));
    return decide(e, q, MODE_SPLIT, false);
}

static int record_outcome(haf_engine *e, const Request &q, int mode, int inexact_grids, int roll_first, const haf_grasp_input *in,
                          haf_roll_record *records)
{
    if (e->cfg.flags & HAF_FLAG_PROFILE)
        for (int i = 0; i < HAF_ST_COUNT; i++) (void)hipEventElapsedTime(&e->stage_ms[i], e->ev[i], e->ev[i + 1]);
    const int *h = e->h_counters;
    LastCall &l = e->last;
    l.B = q.B; l.R = q.R; l.roll_first = roll_first;
    l.evals = h[CNT_EVALS];
    l.flagged = e->mdl.prob_mode ? 0 : h[CNT_FLAGGED];      // (probability mode: the counter holds the estimates the host finished)
    l.flagged2 = h[CNT_FLAGGED2];
    l.lr = q.lr_used;
    l.flagged0 = q.t0b_used ? std::min(h[CNT_FLAGGED0B], h[CNT_FLAGGED0]) : h[CNT_FLAGGED0];   // what leaves the screening passes
    l.flaggedi = q.i8_used ? h[CNT_FLAGGEDI] : h[CNT_FLAGGED];
    l.bypass = h[CNT_BYPASS];                            // (the short-list gate: entries that went around tier 1 and the exact-integer tier)
    l.inexact = inexact_grids;
    l.screened = (mode == MODE_SCREEN) && !e->mdl.prob_mode && !q.direct && h[CNT_FLAGGED0] <= e->flag0_cap;
    l.host_resolved = q.host_resolved;
    l.i8 = q.i8_used;
    l.inputs.assign(in, in + q.B);
    l.clouds = q.src;
    l.roi = q.from.roi != nullptr;
    for (int b = 0; q.from.views && b < q.B; b++) l.clouds[(size_t)b].n = (size_t)q.h_clouds[b].n;      // (upload_frames: the live counts)
    // zero the counters for the next request now, behind this one's copy-out: off that request's critical path
    if (hipMemsetAsync(e->d_counters.p, 0, CNT_COUNT * sizeof(int), q.s) == hipSuccess) e->counters_clean = true;
    // (the tier lists hold every evaluation of a request: list_cap >= last.evals >= last.flagged >= last.flagged2)
    if (l.flagged > e->list_cap || l.flagged2 > e->list_cap || l.flaggedi > e->list_cap) return fail(e, HAF_E_INTERNAL, "recheck list counters exceed the number of evaluations");
    if (const int rc = check_guards(e)) return rc;       // (testing build, opt-in: the guard zones around every device buffer after EVERY request)
    for (int i = 0; i < q.B * q.R; i++) {
        records[i].vote = e->h_rec[i].vote;
        records[i].row = e->h_rec[i].row;
        records[i].col = e->h_rec[i].col;
        records[i].h_locmax = e->h_rec[i].h_locmax;
        records[i].n_evals = e->h_rec[i].n_evals;
    }
    return HAF_OK;
}

int score_rolls_impl(haf_engine *e, int32_t n_clouds, const haf_cloud *clouds, const haf_grasp_input *in, int32_t roll_first,
                     int32_t roll_count, haf_roll_record *records, const FrameSource *from)
{
    if (!e) return HAF_E_ARG;
    Request q;
    if (from) q.from = *from;
    const RoiCall *const roi = q.from.roi;
    int rc = check_request(e, n_clouds, clouds, in, roll_first, roll_count, records, q);
    if (rc != HAF_OK) return rc;
    pack_headers(e, clouds, in, roll_first, q);
    q.s = e->stream;
    mark(e, 0);
    if ((rc = q.from.frames ? upload_frames(e, q) : upload_clouds(e, clouds, q)) != HAF_OK) return rc;
    if (roi && !q.from.objects && (rc = roi_upload_masks(e, *roi, q.from.frames, q.n_frames, q.s)) != HAF_OK) return rc;
    classify_request(e, in, q);
    if ((rc = run_prestages(e, q)) != HAF_OK) return rc;
    int mode = contraction_mode(e->cfg);
    bool reprobe = false;
    if (mode == MODE_SCREEN && !e->screen_active) {
        // (the switch-off used to be for the engine's lifetime) every reprobe_every-th request that is large enough to judge by
        // runs the screening pass again; it costs that request one wasted pass at worst
        if (!roi && !e->variant_forced && !e->mdl.prob_mode && !q.direct && q.evals_sel >= 4096 && ++e->inactive_calls >= e->reprobe_every) {
            e->inactive_calls = 0;
            reprobe = true;
        } else {
            mode = MODE_SPLIT;
        }
    }
    rc = e->mdl.prob_mode ? decide_probability(e, q) : decide(e, q, mode, false);
    if (rc != HAF_OK) return rc;
    if (e->h_counters[CNT_ERROR] != 0 && !e->no_bucket_sort) {
        // a tile of k_bin_tiles had more candidate buckets than its list holds (never observed; the bound is geometric): the
        // height grids of this call may miss points.  Serve the request -- and this engine from now on -- with k_bin instead.
        e->no_bucket_sort = true;
        e->counters_clean = false;
        return score_rolls_impl(e, n_clouds, clouds, in, roll_first, roll_count, records, from);
    }
    const int inexact_grids = e->h_counters[CNT_INEXACT];     // (a redo of the decision stage below resets the counters)
    if (mode == MODE_SCREEN && !e->mdl.prob_mode && !q.direct &&
        (rc = roi ? roi_screen_overflow(e, q, &mode) : adapt_screen_form(e, q, &mode, reprobe)) != HAF_OK) return rc;
    return record_outcome(e, q, mode, inexact_grids, roll_first, in, records);
}

int score_batch_impl(haf_engine *e, int32_t n_clouds, const haf_cloud *clouds, const haf_grasp_input *in, haf_grasp_output *out,
                     const FrameSource *from)
{
    if (!e) return HAF_E_ARG;
    if (!out) return fail(e, HAF_E_ARG, "haf_score_batch: null output");
    std::vector<haf_roll_record> rec((size_t)std::max(1, n_clouds) * e->cfg.n_rolls);
    // A request whose every budget is negative runs no roll in the reference (server.cpp:367-374: the loop breaks before roll 0 and the
    // goal still succeeds with the untouched overall best): nothing for the device to do -- empty records, finalised below
    bool none_runs = in != nullptr && clouds != nullptr && n_clouds >= 1 && n_clouds <= e->cfg.max_clouds;
    for (int b = 0; none_runs && b < n_clouds; b++) none_runs = (int)in[b].max_calculation_time < 0;
    int rc = HAF_OK;
    if (none_runs)
        e->last = LastCall{};
    else if (from)
        rc = score_rolls_impl(e, n_clouds, clouds, in, 0, e->cfg.n_rolls, rec.data(), from);
    else
        rc = haf_score_rolls(e, n_clouds, clouds, in, 0, e->cfg.n_rolls, rec.data());
    if (rc != HAF_OK) return rc;
    for (int b = 0; b < n_clouds; b++) {
        rc = haf_finalize(e, &in[b], rec.data() + (size_t)b * e->cfg.n_rolls, &out[b]);
        if (rc != HAF_OK) return rc;
    }
    // rechecks are counted per batch; attribute them to the first cloud's output and leave the others at 0
    out[0].n_rechecked = e->last.flagged + (e->last.i8 ? e->last.bypass : 0);
    return HAF_OK;
}

// haf_score_frames: every refusal before any device work, then the batch path with frame b as the source of cloud b's points
int score_frames_impl(haf_engine *e, int32_t n, const haf_frame *frames, const haf_grasp_input *in, haf_grasp_output *out)
{
    if (!e) return HAF_E_ARG;
    if (!frames || !in || !out || n < 1) return fail(e, HAF_E_ARG, "haf_score_frames: null or empty argument");
    if (n > e->cfg.max_clouds) return fail(e, HAF_E_CAPACITY, "haf_score_frames: more frames than max_clouds");
    const FrameBatch chk = check_frame_batch(frames, n, nullptr, e->cfg.max_points);
    if (chk.code != HAF_OK && chk.text.empty()) return fail(e, chk.code, "haf_score_frames: more pixels than max_points");
    if (chk.code != HAF_OK) return fail(e, chk.code, "haf_score_frames: frame " + std::to_string(chk.request) + ": " + chk.text);
    const FrameSource from{frames, nullptr, nullptr};
    return score_batch_impl(e, n, chk.clouds.data(), in, out, &from);
}

// haf_score_views: every refusal before any device work, then the batch path with the views of request b as the source of cloud b's
// points.  clouds[b].n_points is the UPPER bound, the pixels of the request's views: it sizes the request's region, sorted_off, max_n,
// total_n and every launch grid; the kernels stop at the live count on the device
int score_views_impl(haf_engine *e, int32_t n, const int32_t *views_per_request, const haf_frame *frames, const haf_grasp_input *in,
                     haf_grasp_output *out, int64_t *n_points)
{
    if (!e) return HAF_E_ARG;
    if (!views_per_request || !frames || !in || !out || n < 1) return fail(e, HAF_E_ARG, "haf_score_views: null or empty argument");
    if (n > e->cfg.max_clouds) return fail(e, HAF_E_CAPACITY, "haf_score_views: more requests than max_clouds");
    for (int b = 0; b < n; b++)
        if (views_per_request[b] < 1 || views_per_request[b] > HAF_MAX_VIEWS)
            return fail(e, HAF_E_ARG, "haf_score_views: request " + std::to_string(b) + ": view count outside [1, HAF_MAX_VIEWS]");
    const FrameBatch chk = check_frame_batch(frames, n, views_per_request, e->cfg.max_points);
    if (chk.code != HAF_OK && chk.text.empty()) return fail(e, chk.code, "haf_score_views: more pixels than max_points");
    if (chk.code != HAF_OK) return fail(e, chk.code, "haf_score_views: request " + std::to_string(chk.request) + " view " + std::to_string(chk.view) + ": " + chk.text);
    int rc0 = HAF_OK;
    if (chk.host_xyz && (rc0 = ensure_raw_xyz(e, "haf_score_views: ")) != HAF_OK) return rc0;
    const FrameSource from{frames, views_per_request, nullptr};
    const int rc = score_batch_impl(e, n, chk.clouds.data(), in, out, &from);
    if (rc != HAF_OK) return rc;
    // (a batch whose every budget is negative runs nothing, on the device either: no count exists)
    for (int b = 0; n_points && b < n; b++) n_points[b] = (size_t)b < e->last.clouds.size() ? (int64_t)e->last.clouds[(size_t)b].n : -1;
    return HAF_OK;
}

}  // namespace haf_host
