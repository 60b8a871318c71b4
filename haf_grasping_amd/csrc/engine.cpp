// engine.cpp -- host side of libhafgrasp.so: the C-ABI of include/hafgrasp.h over the gfx950 kernels.
//
// What stays on the host, and why: the per-roll 4x4 transform and the rotated-rectangle scalars of pnt_in_box
// (a few dozen fp32 operations per roll that use glibc sinf/cosf/atan2f exactly as the reference does), the
// sequential cross-roll rule, and the final grasp pose (once per goal).  Everything that scales with points, cells
// or support vectors runs in the .hip translation units next to this file.  There is no CPU implementation of those stages in this library.
#include "engine_state.h"

namespace {

thread_local std::string g_create_error;

}  // namespace

// ---- engine_internal.h ----
namespace haf {
static_assert(sizeof(RollRecordDev) == sizeof(haf_roll_record) && sizeof(haf_roll_record) == 16, "roll records travel as 16 bytes");
static_assert(sizeof(AttrRecord) == sizeof(haf_attr_record) && sizeof(haf_attr_record) == 24, "attribute debug record layout");
const void *engine_records_dev(const haf_engine *e) { return e->d_rec.p; }
hipStream_t engine_stream(const haf_engine *e) { return e->stream; }
const haf_config *engine_config(const haf_engine *e) { return &e->cfg; }
void engine_set_error(haf_engine *e, const char *msg) { e->error = msg; }
}  // namespace haf

// ---------------------------------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------------------------------
extern "C" {

int haf_abi_version(void) { return HAF_ABI_VERSION; }

void haf_config_default(haf_config *c)
{
    memset(c, 0, sizeof *c);
    c->nr_features_without_shaf = 302;
    c->grid_h = 56; c->grid_w = 56;
    c->n_rolls = 190 / 15;
    c->roll_step_deg = 15;
    c->z_shift = 0.15f;
    c->graspval_top = 119;
    c->graspval_th = 70;
    c->max_rolls_per_call = 0;
    c->device = 0;
    c->max_clouds = 1;
    c->max_points = 1 << 20;
    c->flags = 0;
}

void haf_grasp_input_default(haf_grasp_input *in)
{
    memset(in, 0, sizeof *in);
    in->grasp_area_length_x = 32;
    in->grasp_area_length_y = 44;
    in->approach_vector[2] = 1.0;
    in->max_calculation_time = 50.0;
    in->gripper_opening_width = 1;
}

const char *haf_last_error(const haf_engine *e) { return e ? e->error.c_str() : g_create_error.c_str(); }

void haf_destroy(haf_engine *e)
{
    if (!e) return;
    if (e->has_own_stream) (void)hipStreamSynchronize(e->stream); // (a half-built engine touches no device; a null handle is HIP's default stream, not "no stream")
    for (auto &r : e->host_regs) (void)hipHostUnregister((void *)r.first);
    e->host_regs.clear();
    for (auto &ev : e->ev) if (ev) (void)hipEventDestroy(ev);
    if (e->has_own_stream) (void)hipStreamDestroy(e->own_stream);   // (idle: haf_set_stream synchronised it when it switched away)
    delete e;      // frees every DevBuf and StageBuf member: the stream was synchronised above, so nothing still runs on them
}
// Default mode: which screening variant serves this MODEL is found out here, at creation, not on the first goals of a fresh
// action server: up to three requests on a synthetic table scene (a plane with a few dozen boxes and domes of 2-12 cm, a point
// per grid cell) run through the same adaptive rule as every later call (plain variant -> the variant that measures |w|_2 when
// more than a quarter of the evaluations stay undecided -> no screening pass when that still leaves more than 60 %).  On the
// committed surrogate the scene classifies like the real clouds do (plain 94 % undecided, measuring variant 66 %: screening
// off); a model the scene misjudges is still re-classified by the rule on its first real requests, as before.
static int calibrate(haf_engine *e)
{
    const haf_config &c = e->cfg;
    if (contraction_mode(c) != MODE_SCREEN || !e->screen_active || e->mdl.prob_mode) return HAF_OK;
    const int G = c.grid_h;
    const long cells = (long)G * G;
    const long stride = std::max<long>(1, (cells + c.max_points - 1) / c.max_points);
    std::vector<float> xyz;
    xyz.reserve((size_t)(cells / stride + 1) * 3);
    uint32_t lcg = 0x9E3779B9u;
    auto rnd = [&]() { lcg = lcg * 1664525u + 1013904223u; return (float)((lcg >> 8) & 0xFFFFFF) / 16777216.0f; };
    struct Obj { float cx, cy, sx, sy, h, ct, st; int dome; };
    std::vector<Obj> objs((size_t)std::max<long>(4, cells / 400));
    const float half = 0.005f * (float)G;
    for (size_t k = 0; k < objs.size(); k++) {
        Obj &o = objs[k];
        o.cx = (2.0f * rnd() - 1.0f) * half; o.cy = (2.0f * rnd() - 1.0f) * half;
        o.sx = 0.015f + 0.045f * rnd(); o.sy = 0.015f + 0.045f * rnd();
        o.h = 0.02f + 0.10f * rnd();
        const float th = 3.14159265f * rnd();
        o.ct = std::cos(th); o.st = std::sin(th);
        o.dome = (k % 3) == 0;
    }
    // (objects only reach a few cells: a coarse bucket grid keeps the scene of a 512 x 512 engine cheap to build)
    const int nbk = std::max(1, G / 16);
    std::vector<std::vector<int>> bk((size_t)nbk * nbk);
    for (size_t k = 0; k < objs.size(); k++) {
        const float r = 1.5f * std::max(objs[k].sx, objs[k].sy);
        const int i0 = std::max(0, (int)((objs[k].cx - r + half) / (2 * half) * nbk)), i1 = std::min(nbk - 1, (int)((objs[k].cx + r + half) / (2 * half) * nbk));
        const int j0 = std::max(0, (int)((objs[k].cy - r + half) / (2 * half) * nbk)), j1 = std::min(nbk - 1, (int)((objs[k].cy + r + half) / (2 * half) * nbk));
        for (int i = i0; i <= i1; i++) for (int j = j0; j <= j1; j++) bk[(size_t)i * nbk + j].push_back((int)k);
    }
    for (long cell = 0; cell < cells; cell += stride) {
        const int i = (int)(cell / G), j = (int)(cell % G);
        const float x = ((float)i + 0.5f) * 0.01f - half, y = ((float)j + 0.5f) * 0.01f - half;
        float z = 0.0f;
        for (int k : bk[(size_t)std::min(nbk - 1, i * nbk / G) * nbk + std::min(nbk - 1, j * nbk / G)]) {
            const Obj &o = objs[(size_t)k];
            const float u = (x - o.cx) * o.ct + (y - o.cy) * o.st, v = -(x - o.cx) * o.st + (y - o.cy) * o.ct;
            if (o.dome) {
                const float q = u * u / (o.sx * o.sx) + v * v / (o.sy * o.sy);
                if (q < 1.0f) z = std::max(z, o.h * std::sqrt(std::max(0.0f, 1.0f - 0.5f * q)));
            } else if (std::fabs(u) < o.sx && std::fabs(v) < o.sy) {
                z = std::max(z, o.h);
            }
        }
        xyz.push_back(x); xyz.push_back(y); xyz.push_back(z + 0.002f * rnd());
    }
    haf_cloud cl{};
    cl.xyz = xyz.data(); cl.n_points = xyz.size() / 3; cl.stride_floats = 3; cl.on_device = 0;
    haf_grasp_input in;
    haf_grasp_input_default(&in);
    in.grasp_area_length_x = (float)G; in.grasp_area_length_y = (float)G;
    const int R = std::min(e->max_rolls, 2);
    std::vector<haf_roll_record> rec((size_t)R);
    const long keep_direct = e->direct_work;
    e->direct_work = 0;                                   // the tiers themselves, also on a small grid
    // Every form the engine has is tried on the scene (pinned, so that the adaptive rule does not interfere), cheapest kernel first;
    // a form that leaves next to nothing undecided ends the search.  The choice minimises kernel cost + what the undecided
    // evaluations cost behind it, in units of the plain kernel's time per evaluation (SUMSQ and CR_EXP: three VALU instructions
    // behind the exp instead of one, measured 1.085; CR_POLY: six and no exp, ~1.2; an undecided evaluation costs ~8.5 screened
    // ones in the three-pass tier and the exact tiers behind it: seed 11 of the bench generator).
    int rc = HAF_OK;
    const bool forced0 = e->variant_forced;
    const int variant0 = e->screen_variant;
    if (!forced0) {
        static const int order[SCREEN_VARIANTS] = {SCREEN_PLAIN, SCREEN_CR_EXP, SCREEN_SUMSQ, SCREEN_CR_POLY};   // cheapest kernel first
        double best_cost = 1e30;
        int best = -1;
        e->variant_forced = true;
        for (int oi = 0; oi < SCREEN_VARIANTS && rc == HAF_OK; oi++) {
            const int v = order[oi];
            if (v >= SCREEN_CR_EXP && !e->mdl.cr_available) continue;
            e->screen_variant = v;
            e->screen_active = true;
            rc = score_rolls_impl(e, 1, &cl, &in, 0, R, rec.data());
            if (rc != HAF_OK) break;
            const double ne = (double)std::max(1, e->last.evals);
            const double share = e->last.screened ? (double)e->last.flagged0 / ne : 1.0;
            e->variant_share[v] = share;
            if (share < 0.001) break;                    // nothing a later form could win back
        }
        // The choice: kernel cost + what the undecided evaluations cost behind it.  A PLAIN / SUMSQ first pass may have the
        // centred-remainder form as a SECOND pass on its list (tier 0b: ~1.6 screened evaluations per listed one -- its own feature
        // kernel and a contraction launch at a fraction of the chip), after which only what that form leaves is undecided: for a
        // well-conditioned model (a few per cent after the first pass) cheaper than the centred-remainder form over everything.
        for (int v = 0; v < SCREEN_VARIANTS && rc == HAF_OK; v++) {
            const double share = e->variant_share[v];
            if (share < 0.0) continue;
            double cost = variant_cost(e, v) + kUndecidedCost * share;
            const double s_cr = e->variant_share[SCREEN_CR_EXP];
            if ((v == SCREEN_PLAIN || v == SCREEN_SUMSQ) && e->mdl.cr_available && s_cr >= 0.0 && s_cr < share)
                cost = std::min(cost, variant_cost(e, v) + 1.6 * share + kUndecidedCost * s_cr);
            if (cost < best_cost) { best_cost = cost; best = v; }
        }
        e->variant_forced = false;
        if (rc == HAF_OK) {
            e->screen_variant = best >= 0 ? best : variant0;
            e->screen_active = best >= 0 && e->variant_share[best] <= 0.6;
        }
    } else {
        rc = score_rolls_impl(e, 1, &cl, &in, 0, R, rec.data());
    }
    if (rc == HAF_OK && e->screen_active) {
        // tier 0b behind a PLAIN / SUMSQ first pass: when the centred-remainder form left less than half as much undecided on the scene
        const int v = e->screen_variant;
        const char *f0b = test_env("HAF_T0B"), *fsk = test_env("HAF_T1_SKIP");
        // (the scene is small and tame -- the C5 bench leaves five times the share of the 56 x 56 scene undecided -- so the rule is
        // "whenever it decided more there", not a threshold)
        e->use_t0b = e->mdl.cr_available && (v == SCREEN_PLAIN || v == SCREEN_SUMSQ) && e->variant_share[SCREEN_CR_EXP] >= 0.0 &&
                     e->variant_share[SCREEN_CR_EXP] < e->variant_share[v];
        if (f0b) e->use_t0b = atoi(f0b) != 0 && e->mdl.cr_available;
        // is tier 1 of use behind the screening passes of this model?  One request in the final configuration: how much of what they
        // left did the three-pass kernel decide
        const bool forced1 = e->variant_forced;
        e->variant_forced = true;
        e->t1_skip = false;
        rc = score_rolls_impl(e, 1, &cl, &in, 0, R, rec.data());
        e->variant_forced = forced1;
        if (rc == HAF_OK && e->last.screened && e->last.flagged0 >= 32)
            e->t1_skip = (double)(e->last.flagged0 - e->last.flagged) < 0.35 * (double)e->last.flagged0;
        if (fsk) e->t1_skip = atoi(fsk) != 0;
    }
    e->direct_work = keep_direct;
    e->calibrated = true;
    e->last = LastCall{};                                 // (the calibration requests are not a "last scored batch")
    return rc;
}

static int create_impl(const haf_config *cfg, haf_engine **out)
{
    if (out) *out = nullptr;
    if (!cfg || !out) { g_create_error = "haf_create: null argument"; return HAF_E_ARG; }
    haf_engine *e = new haf_engine();
    struct Guard { haf_engine *e; ~Guard() { if (e) haf_destroy(e); } } guard{e};      // an exception below must not leak the engine
    auto bail = [&](int code) { g_create_error = e->error; return code; };
    e->cfg = *cfg;
    if (!cfg->feature_file || !cfg->range_file || !cfg->model_file) { e->error = "feature_file, range_file and model_file are required"; return bail(HAF_E_ARG); }
    e->feature_file = cfg->feature_file; e->range_file = cfg->range_file; e->model_file = cfg->model_file;
    e->cfg.feature_file = e->feature_file.c_str(); e->cfg.range_file = e->range_file.c_str(); e->cfg.model_file = e->model_file.c_str();
    if (cfg->grid_h != cfg->grid_w) { e->error = "grid_h must equal grid_w (the reference's mask geometry assumes a square grid, server.cpp:681-682, 705)"; return bail(HAF_E_ARG); }
    if (cfg->grid_h < 15 || cfg->grid_h > 4096) { e->error = "grid size must be in [15, 4096]"; return bail(HAF_E_ARG); }
    if (cfg->n_rolls < 1 || cfg->n_rolls > 4096 || cfg->max_clouds < 1 || cfg->max_points < 1) { e->error = "n_rolls, max_clouds and max_points must be positive"; return bail(HAF_E_ARG); }
    // integral images are read through a buffer descriptor (32-bit byte offsets): all of them must fit 4 GiB
    if (cfg->max_rolls_per_call < 0) { e->error = "max_rolls_per_call must be >= 0"; return bail(HAF_E_ARG); }
    {
        const int rolls_cap = (cfg->max_rolls_per_call > 0) ? std::min(cfg->max_rolls_per_call, cfg->n_rolls) : cfg->n_rolls;
        if ((double)cfg->max_clouds * rolls_cap * (cfg->grid_h + 1) * (cfg->grid_w + 1) * 4.0 >= 4294967296.0) { e->error = "max_clouds*rolls per call*grid cells exceeds 2^30"; return bail(HAF_E_CAPACITY); }
    }

    if (!load_features(e->feature_file, e->features, e->error)) return bail(HAF_E_IO);
    if (!load_range(e->range_file, e->range, e->error)) return bail(HAF_E_IO);
    if (!load_model(e->model_file, e->model, e->error)) return bail(HAF_E_IO);
    // libsvm's other vector kernels (linear, polynomial, sigmoid): svm-predict serves them, so the drop-in does -- through the tier that
    // IS libsvm's arithmetic (k_recheck: every evaluation in the library's own order, then the C library's tanh near zero).  The fast tiers
    // are built for the RBF kernel (the reference's model is an easy.py product); their tables are not built for such a model.
    e->generic_kernel = e->model.kernel_type != HAF_KERNEL_RBF;
    if (e->generic_kernel) {
        e->cfg.flags &= ~(uint32_t)HAF_FLAG_FP32_MFMA;
        e->cfg.flags |= HAF_FLAG_SPLIT_F16;                // (no screening tables, no calibration; the request path never looks at the contraction mode)
        e->direct_work = 0;
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { e->error = "no HIP device available: this engine has no CPU fallback"; return bail(HAF_E_DEVICE); }
    if (cfg->device < 0 || cfg->device >= ndev) { e->error = "device ordinal out of range"; return bail(HAF_E_DEVICE); }
    if (hipSetDevice(cfg->device) != hipSuccess) { e->error = "hipSetDevice failed"; return bail(HAF_E_DEVICE); }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) { e->error = "hipGetDeviceProperties failed"; return bail(HAF_E_DEVICE); }
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) { e->error = std::string("device is ") + prop.gcnArchName + ", the kernels are built for gfx950 only"; return bail(HAF_E_DEVICE); }
    if (hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking) != hipSuccess) { e->error = "hipStreamCreate failed"; return bail(HAF_E_DEVICE); }
    e->has_own_stream = true;
    e->stream = e->own_stream;
    for (auto &ev : e->ev) if (hipEventCreate(&ev) != hipSuccess) { e->error = "hipEventCreate failed"; return bail(HAF_E_DEVICE); }

#ifndef HAF_FLUSH_F16_SUBNORMALS
    if (contraction_mode(e->cfg) == MODE_SCREEN) {
        // the screening operands keep fp16 subnormals (features.hip: screen_operand): make sure the matrix core does too
        static std::mutex probe_mutex;                // one probe per DEVICE and process, whichever thread gets there first
        static int probed[64];                        // 0: not yet; else result + 2
        int keeps;
        {
            std::lock_guard<std::mutex> lock(probe_mutex);
            const int slot = cfg->device & 63;
            if (cfg->device >= 64 || probed[slot] == 0) {
                keeps = probe_f16_subnormal_mfma(e->stream);
                if (cfg->device < 64 && keeps >= 0) probed[slot] = keeps + 2;
            } else {
                keeps = probed[slot] - 2;
            }
        }
        if (keeps < 0) { e->error = "fp16 subnormal probe failed to run"; return bail(HAF_E_DEVICE); }
        if (keeps == 0) { e->error = "this device flushes fp16 subnormal MFMA operands: rebuild with -DHAF_FLUSH_F16_SUBNORMALS"; return bail(HAF_E_DEVICE); }
    }
#endif
    if (contraction_mode(e->cfg) != MODE_F32) {
        // the guard bands of the fp16 tiers carry the rounding of the matrix core as a MEASURED constant (screen.hip:
        // probe_mfma_rounding): once per device and process
        static std::mutex kappa_mutex;
        static double kappa_of[64], kappa16_of[64];   // 0: not yet
        double meas, meas16 = 0.0;
        {
            std::lock_guard<std::mutex> lock(kappa_mutex);
            const int slot = cfg->device & 63;
            if (cfg->device >= 64 || kappa_of[slot] == 0.0) {
                meas = probe_mfma_rounding(e->stream, &meas16);
                if (cfg->device < 64 && meas > 0.0) { kappa_of[slot] = meas; kappa16_of[slot] = meas16; }
            } else {
                meas = kappa_of[slot];
                meas16 = kappa16_of[slot];
            }
        }
        if (!(meas > 0.0) || !(meas16 > 0.0)) { e->error = "matrix-core rounding probe failed to run"; return bail(HAF_E_DEVICE); }
        e->mfma_kappa_measured = meas;
        e->mfma_kappa16_measured = meas16;
        // floor 12 (round 4; 8 before): the largest value seen by any search so far is 9.1 -- one product of order 1 over 31 products
        // with 22-bit mantissas, tests/test_engine_gpu.py::test_matrix_core_rounding_adversarial_search -- and the reading that fits
        // every measurement (terms aligned to the largest exponent, two guard bits, one final rounding) allows 33 x 0.25 + 1 = 9.25
        e->mfma_kappa = std::max(12.0, 1.5 * meas);
        e->mfma_kappa16 = std::max(12.0, 1.5 * meas16);
        // testing build: a matrix core that rounds worse than any seen, injected -- the bands must widen with it, the labels must not
        // move, and from 64 on the engine must refuse the device (tests/test_engine_gpu.py)
        if (const char *k = test_env("HAF_KAPPA")) e->mfma_kappa = e->mfma_kappa16 = atof(k);
        if (!(e->mfma_kappa < 64.0) || !(e->mfma_kappa16 < 64.0)) { e->error = "this device's fp16 MFMA rounds far worse than the guard bands allow for (probe_mfma_rounding)"; return bail(HAF_E_DEVICE); }
    }
    if (const char *v = test_env("HAF_LARGE_EVALS")) e->large_evals = atol(v);      // experiments
    if (e->cfg.flags & HAF_FLAG_FULL_RANK) e->lr_enabled = false;
    // the tests that scale a guard band or force a tier mean the tiers themselves, also on a tiny request
    if (test_env("HAF_NO_DIRECT") || test_env("HAF_GUARD_REL") || test_env("HAF_GUARD0_REL") || test_env("HAF_GUARD2_REL") ||
        test_env("HAF_LARGE_EVALS") || test_env("HAF_NO_FAST_GROUPS") || test_env("HAF_SCREEN_NO_CENTRE") || test_env("HAF_FLAG_WINDOW") ||
        test_env("HAF_HOST_EXP_ALL") || test_env("HAF_NO_I8") || test_env("HAF_GUARD_I8_REL") || test_env("HAF_FLAG0_CAP"))
        e->direct_work = 0;
    if (test_env("HAF_NO_FUSED_PRE")) e->no_fused_pre = true;
    if (const char *v = test_env("HAF_REPROBE_EVERY")) e->reprobe_every = std::max(1, atoi(v));
    if (const char *v = test_env("HAF_SCREEN_PARTS")) e->screen_parts = std::max(0, atoi(v));
    if (test_env("HAF_NO_SHORT_GATE")) e->short_gate = false;
    if (const char *v = test_env("HAF_SCREEN_VARIANT")) { e->screen_variant = std::max(0, std::min(SCREEN_VARIANTS - 1, atoi(v))); e->variant_forced = true; e->direct_work = 0; }
    int rc = build_tables(e);
    if (rc != HAF_OK) return bail(rc);
    if (e->screen_variant >= SCREEN_CR_EXP && !e->mdl.cr_available) e->screen_variant = SCREEN_PLAIN;   // (a pinned form the model has no tables for)
    rc = alloc_buffers(e);
    if (rc != HAF_OK) return bail(rc);
    // (a test that scales the screening band wants the tiers and the adaptive rule as they are, not a model classified under that band)
    if (!test_env("HAF_NO_CALIBRATE") && !test_env("HAF_GUARD0_REL")) {
        rc = calibrate(e);
        if (rc != HAF_OK) return bail(rc);
    }
    guard.e = nullptr;
    *out = e;
    return HAF_OK;
}

int haf_model_info(const haf_engine *e, int32_t *n_sv, int32_t *dim, int32_t *n_features)
{
    if (!e) return HAF_E_ARG;
    if (n_sv) *n_sv = e->model.n_sv;
    if (dim) *dim = e->model.dim;
    if (n_features) *n_features = e->mdl.nf;
    return HAF_OK;
}

int haf_register_host_cloud(haf_engine *e, const void *ptr, size_t bytes)
{
    if (!e) return HAF_E_ARG;
    if (!ptr || !bytes) return fail(e, HAF_E_ARG, "haf_register_host_cloud: null or empty buffer");
    HIPCHK(e, hipSetDevice(e->cfg.device));
    for (auto &r : e->host_regs) if (r.first == ptr) return fail(e, HAF_E_ARG, "haf_register_host_cloud: buffer is registered already");
    HIPCHK(e, hipHostRegister(const_cast<void *>(ptr), bytes, hipHostRegisterDefault));
    e->host_regs.emplace_back(reinterpret_cast<const char *>(ptr), bytes);
    return HAF_OK;
}

int haf_unregister_host_cloud(haf_engine *e, const void *ptr)
{
    if (!e) return HAF_E_ARG;
    for (size_t i = 0; i < e->host_regs.size(); i++)
        if (e->host_regs[i].first == ptr) {
            (void)hipStreamSynchronize(e->stream);
            HIPCHK(e, hipHostUnregister(const_cast<void *>(ptr)));
            e->host_regs.erase(e->host_regs.begin() + (long)i);
            return HAF_OK;
        }
    return fail(e, HAF_E_ARG, "haf_unregister_host_cloud: buffer was not registered");
}

int haf_screen_form(const haf_engine *e, int32_t *form, int32_t *active)
{
    if (!e) return HAF_E_ARG;
    const bool on = contraction_mode(e->cfg) == MODE_SCREEN && e->screen_active && !e->mdl.prob_mode;
    if (form) *form = e->screen_variant;
    if (active) *active = on ? 1 : 0;
    return HAF_OK;
}

int haf_screen_low_rank(const haf_engine *e, int32_t *available, int32_t *rank, int32_t *last_used)
{
    if (!e) return HAF_E_ARG;
    if (available) *available = (e->mdl.lr_available && e->lr_enabled) ? 1 : 0;
    if (rank) *rank = e->mdl.lr_rank;
    if (last_used) *last_used = e->last.lr ? 1 : 0;
    return HAF_OK;
}

int haf_last_counts(const haf_engine *e, int64_t *n_evals, int64_t *n_rechecked, int64_t *n_strict)
{
    if (!e) return HAF_E_ARG;
    if (n_evals) *n_evals = e->last.evals;
    if (n_rechecked) *n_rechecked = e->last.flagged + (e->last.i8 ? e->last.bypass : 0);   // (the short-list gate's entries skip the exact-integer tier's input list)
    if (n_strict) *n_strict = e->last.flagged2;
    return HAF_OK;
}

int haf_last_tiers(const haf_engine *e, int64_t *n_evals, int64_t *n_refined, int64_t *n_rechecked, int64_t *n_strict)
{
    if (!e) return HAF_E_ARG;
    if (n_evals) *n_evals = e->last.evals;
    if (n_refined) *n_refined = e->last.flagged0;
    if (n_rechecked) *n_rechecked = e->last.flagged + (e->last.i8 ? e->last.bypass : 0);   // (the short-list gate's entries skip the exact-integer tier's input list)
    if (n_strict) *n_strict = e->last.flagged2;
    return HAF_OK;
}

int haf_last_exact_tiers(const haf_engine *e, int64_t *n_integer, int64_t *n_fp64)
{
    if (!e) return HAF_E_ARG;
    if (n_integer) *n_integer = e->last.i8 ? e->last.flagged : 0;
    if (n_fp64) *n_fp64 = e->last.flaggedi;
    return HAF_OK;
}

int haf_last_strict_host(const haf_engine *e, int64_t *n_host)
{
    if (!e) return HAF_E_ARG;
    if (n_host) *n_host = e->last.host_resolved;
    return HAF_OK;
}

int haf_last_prestage(const haf_engine *e, int64_t *n_inexact_grids)
{
    if (!e) return HAF_E_ARG;
    if (n_inexact_grids) *n_inexact_grids = e->last.inexact;
    return HAF_OK;
}

int haf_set_stream(haf_engine *e, void *s)
{
    if (!e) return HAF_E_ARG;
    if ((hipStream_t)s == e->stream) return HAF_OK;                // the current stream: nothing to order
    // every request leaves, unsynchronised, the memset that zeroes the next request's counters on the old stream: the new stream
    // must not start before it.  A null handle is HIP's default stream and is synchronised like any other
    HIPCHK(e, hipSetDevice(e->cfg.device));
    (void)hipStreamSynchronize(e->stream);
    e->stream = (hipStream_t)s;                                    // (the engine's own stream lives until haf_destroy: its handle switches back)
    return HAF_OK;
}

void *haf_get_stream(haf_engine *e) { return e ? (void *)e->stream : nullptr; }
int haf_finalize(haf_engine *e, const haf_grasp_input *in, const haf_roll_record *rec, haf_grasp_output *out)
{
    if (!e) return HAF_E_ARG;
    if (!in || !rec || !out) return fail(e, HAF_E_ARG, "haf_finalize: null argument");
    return finalize_impl(e->cfg, in, rec, out, e->error);
}
int haf_get_stage_ms(haf_engine *e, float *ms)
{
    if (!e || !ms) return HAF_E_ARG;
    if (!(e->cfg.flags & HAF_FLAG_PROFILE)) return fail(e, HAF_E_ARG, "engine was created without HAF_FLAG_PROFILE");
    memcpy(ms, e->stage_ms, sizeof e->stage_ms);
    return HAF_OK;
}

static int pcd_load_impl(const char *path, float **xyz, size_t *n_points, char *err, size_t err_cap)
{
    if (!path || !xyz || !n_points) return HAF_E_ARG;
    std::vector<float> v;
    std::string msg;
    if (!load_pcd(path, v, msg)) {
        if (err && err_cap) snprintf(err, err_cap, "%s", msg.c_str());
        return HAF_E_IO;
    }
    *n_points = v.size() / 3;
    *xyz = (float *)malloc(std::max<size_t>(1, v.size()) * sizeof(float));
    if (!*xyz) return HAF_E_INTERNAL;
    memcpy(*xyz, v.data(), v.size() * sizeof(float));
    return HAF_OK;
}

int haf_create(const haf_config *cfg, haf_engine **out)
{
    return guarded(&g_create_error, [&] { return create_impl(cfg, out); });
}

int haf_score_rolls(haf_engine *e, int32_t n_clouds, const haf_cloud *clouds, const haf_grasp_input *in, int32_t roll_first,
                    int32_t roll_count, haf_roll_record *records)
{
    return guarded(e ? &e->error : nullptr, [&] { return score_rolls_impl(e, n_clouds, clouds, in, roll_first, roll_count, records); });
}

int haf_roll_pose(haf_engine *e, const haf_grasp_input *in, const haf_roll_record *rec, int32_t roll, haf_grasp_output *out,
                  int32_t *published)
{
    if (!e) return HAF_E_ARG;
    if (!in || !rec || !out) return fail(e, HAF_E_ARG, "haf_roll_pose: null argument");
    return roll_pose_impl(e->cfg, in, rec, roll, out, published, e->error);
}

int haf_score_batch(haf_engine *e, int32_t n_clouds, const haf_cloud *clouds, const haf_grasp_input *in, haf_grasp_output *out)
{
    return guarded(e ? &e->error : nullptr, [&] { return score_batch_impl(e, n_clouds, clouds, in, out); });
}

int haf_score_frames(haf_engine *e, int32_t n, const haf_frame *frames, const haf_grasp_input *in, haf_grasp_output *out)
{
    return guarded(e ? &e->error : nullptr, [&] { return score_frames_impl(e, n, frames, in, out); });
}

int haf_score_frames_roi(haf_engine *e, int32_t n, const haf_frame *frames, const haf_roi *rois, const haf_grasp_input *in, haf_grasp_output *out)
{
    return guarded(e ? &e->error : nullptr, [&] { return score_frames_roi_impl(e, n, frames, rois, in, out); });
}

int haf_score_views_roi(haf_engine *e, int32_t n, const int32_t *views_per_request, const haf_frame *frames, const haf_roi *rois,
                        const haf_grasp_input *in, haf_grasp_output *out, int64_t *n_points)
{
    return guarded(e ? &e->error : nullptr, [&] { return score_views_roi_impl(e, n, views_per_request, frames, rois, in, out, n_points); });
}

int haf_score_views(haf_engine *e, int32_t n, const int32_t *views_per_request, const haf_frame *frames, const haf_grasp_input *in,
                    haf_grasp_output *out, int64_t *n_points)
{
    return guarded(e ? &e->error : nullptr, [&] { return score_views_impl(e, n, views_per_request, frames, in, out, n_points); });
}

// (no engine to carry the message: it goes where haf_create's does, haf_last_error(NULL))
int haf_view_points(const haf_frame *frames, int32_t n_views, float *xyz, size_t cap_points, size_t *n_valid)
{
    return guarded(&g_create_error, [&] { return view_points_impl(frames, n_views, xyz, cap_points, n_valid, g_create_error); });
}

int haf_score(haf_engine *e, const haf_cloud *cloud, const haf_grasp_input *in, haf_grasp_output *out)
{
    return haf_score_batch(e, 1, cloud, in, out);
}

int haf_pcd_load(const char *path, float **xyz, size_t *n_points, char *err, size_t err_cap)
{
    std::string msg;
    const int rc = guarded(&msg, [&] { return pcd_load_impl(path, xyz, n_points, err, err_cap); });
    if (rc == HAF_E_INTERNAL && !msg.empty() && err && err_cap) snprintf(err, err_cap, "%s", msg.c_str());
    return rc;
}

}  // extern "C"
