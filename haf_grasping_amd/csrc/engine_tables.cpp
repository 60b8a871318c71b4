// engine_tables.cpp -- haf_create's table work on the device side: build_tables hands the parsed feature / range / model files to the
// device-free builder (model_tables.cpp: every table's host image, every guard band's constants) and uploads what it made
// (upload_tables, the one place that allocates and copies a model table); alloc_buffers sizes the engine's working buffers.
#include "engine_state.h"

namespace haf_host {

// the testing build's environment, read here and nowhere else on the way to the tables (the product build: every switch at its default)
TableSwitches table_switches()
{
    TableSwitches s;
    s.no_cr = test_env("HAF_NO_CR") != nullptr;
    s.no_lr = test_env("HAF_NO_LR") != nullptr;
    s.cr_no_centre = test_env("HAF_CR_NO_CENTRE") != nullptr;
    s.no_cr_t1 = test_env("HAF_NO_CR_T1") != nullptr;
    s.no_i8 = test_env("HAF_NO_I8") != nullptr;
    s.no_fast_groups = test_env("HAF_NO_FAST_GROUPS") != nullptr;
    s.screen_no_centre = test_env("HAF_SCREEN_NO_CENTRE") != nullptr;
    s.lr_unfused = test_env("HAF_LR_UNFUSED") != nullptr;
    s.no_lr_plain = test_env("HAF_NO_LR_PLAIN") != nullptr;
    s.kappa_t1_measured = test_env("HAF_KAPPA_T1_MEASURED") != nullptr;
    s.prob_host_all = test_env("HAF_PROB_HOST_ALL") != nullptr;
    s.host_exp_all = test_env("HAF_HOST_EXP_ALL") != nullptr;
    if (const char *g = test_env("HAF_GUARD_REL")) { s.guard_rel_set = true; s.guard_rel = guard_knob(g); }
    if (const char *g = test_env("HAF_GUARD0_REL")) { s.guard0_rel_set = true; s.guard0_rel = guard_knob(g); }
    if (const char *g = test_env("HAF_GUARD2_REL")) { s.guard2_rel_set = true; s.guard2_rel = guard_knob(g); }
    if (const char *g = test_env("HAF_GUARD_I8_REL")) { s.guard_i8_rel_set = true; s.guard_i8_rel = guard_knob(g); }
    return s;
}

static TableInputs table_inputs(const haf_engine *e)
{
    TableInputs in;
    in.cfg = e->cfg;
    in.features = &e->features;
    in.range = &e->range;
    in.model = &e->model;
    in.mfma_kappa = e->mfma_kappa;
    in.mfma_kappa16 = e->mfma_kappa16;
    in.generic_kernel = e->generic_kernel;
    in.sw = table_switches();
    return in;
}

template <class T> static hipError_t copy_up(const DevBuf<T> &d, const std::vector<T> &h)
{
    return h.empty() ? hipSuccess : hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

// Everything is allocated before anything is copied or handed over: a creation that fails here leaves an engine without a table, a
// parameter struct or a flag of the model.  (A table the model does not get is empty and stays unallocated: DevBuf::alloc(0).)
int upload_tables(haf_engine *e, const ModelTables &t)
{
    DeviceModel &m = e->mdl;
    bool ok = true;
    // (the table's name where alloc takes the allocating file: the testing build's guard report says which table a damaged zone belongs to)
    for_each_table([&](const char *name, auto &d, const auto &h) { ok = ok && hipSuccess == d.alloc(h.size(), name); }, m, t);
    if (!ok) return fail(e, HAF_E_DEVICE, std::string("hipMalloc of the model tables failed: ") + hipGetErrorString(hipGetLastError()));

    hipError_t rc = hipSuccess;
    const char *failed = "";
    for_each_table([&](const char *name, auto &d, const auto &h) { if (rc == hipSuccess && (rc = copy_up(d, h)) != hipSuccess) failed = name; }, m, t);
    if (rc != hipSuccess) return fail(e, HAF_E_DEVICE, std::string("upload of the model table ") + failed + ": " + hipGetErrorString(rc));

    static_cast<ModelConsts &>(m) = t;
    e->screen_active = m.screen_active;

    // the parameter structs' device pointers, which the builder left null
    auto pairs = [](const ScrCorr *p) { return p ? reinterpret_cast<const ScrCorr2 *>(p + kS0K) : nullptr; };
    m.screen.sd = m.sd.p; m.screen.sd3 = m.sd3.p; m.screen.fd_slot = m.fd_slot.p;
    m.screen.corr = m.corr.p; m.screen.corr2 = pairs(m.corr.p);
    // screen_cr began as a copy of screen (model_tables.cpp: cr_centre) and keeps the plain form's tables where the model did not
    // get the centred ones; screen_lrp is a copy of screen_cr with correction vectors of its own (lr_commit)
    if (t.screen_cr.cr) {
        m.screen_cr.sd = m.screen.sd; m.screen_cr.sd3 = m.screen.sd3; m.screen_cr.fd_slot = m.screen.fd_slot;
        m.screen_cr.corr = m.screen.corr; m.screen_cr.corr2 = m.screen.corr2;
    }
    if (t.cr_available) {
        m.screen_cr.sd = m.sd_cr.p; m.screen_cr.sd3 = m.sd3_cr.p; m.screen_cr.fd_slot = m.fd_slot_cr.p;
        m.screen_cr.corr = m.corr_cr.p; m.screen_cr.corr2 = pairs(m.corr_cr.p);
    }
    if (t.lr_available) {
        m.screen_lrp.sd = m.screen_cr.sd; m.screen_lrp.sd3 = m.screen_cr.sd3; m.screen_lrp.fd_slot = m.screen_cr.fd_slot;
        m.screen_lrp.corr = m.corr_lrp.p; m.screen_lrp.corr2 = pairs(m.corr_lrp.p);
    }
    return HAF_OK;
}

int build_tables(haf_engine *e)
{
    const TableInputs in = table_inputs(e);
    ModelTables t;
    const TableError err = build_model_tables(in, t);
    if (err.code != HAF_OK) return fail(e, err.code, err.msg);
    return upload_tables(e, t);
}

int alloc_buffers(haf_engine *e)
{
    const haf_config &c = e->cfg;
    e->max_rolls = (c.max_rolls_per_call > 0) ? std::min(c.max_rolls_per_call, c.n_rolls) : c.n_rolls;
    const size_t B = (size_t)c.max_clouds, R = (size_t)e->max_rolls, H = (size_t)c.grid_h, W = (size_t)c.grid_w;
    e->cells_cap = B * R * H * W;
    e->max_evals = (long)(B * R * (H - 14) * (W - 14));
    e->max_evals_pad = (e->max_evals + kS0BlockEvals - 1) / kS0BlockEvals * kS0BlockEvals;
    e->list_cap = (int)e->max_evals_pad;             // (< 2^31: cells are 32-bit ids, checked in haf_create)
    e->flag_cap = (int)std::min<long>(std::max<long>(4096, e->max_evals / 4), 1L << 22);
    if (const char *v = test_env("HAF_FLAG_WINDOW")) e->flag_cap = std::max(64, atoi(v));     // tests: many small windows
    // a whole number of 64-entry blocks: the exact tiers' feature kernels finish whole blocks, padding entries included, and a FULL window
    // whose length was not a multiple of 64 had them write up to 63 doubles past the last row of d_part64 (found by the guard zones of
    // the testing build, round 5: every request of the GPU suite under HAF_CANARY_CHECK)
    e->flag_cap = std::max(64, e->flag_cap / 64 * 64);
    const int mode = contraction_mode(c);
    // screening pass: up to half of the evaluations may go on to the three-pass kernel; a model that sends more is served by
    // the three-pass kernel alone from then on (haf_score_rolls)
    e->flag0_cap = mode == MODE_SCREEN ? (int)std::min<long>(std::max<long>(4096, (e->max_evals / 2 + 255) / 256 * 256), 1L << 23) : 0;
    // testing build, the overflow campaigns (tools/fuzz_parity.py --overflow): a screening list far smaller than a request, so that every
    // producer of it runs into its capacity and every consumer meets a counter beyond it (the engine's answer to such an overflow: the
    // next form, then the three-pass kernel for everything).  The windows of the exact tiers shrink with HAF_FLAG_WINDOW above.  The
    // TIER lists (list_cap) are not shrunk: they hold one entry per evaluation of the largest request, no producer can overrun them,
    // and their window-by-window consumers rely on exactly that (a counter never exceeds the list).
    if (const char *v = test_env("HAF_FLAG0_CAP")) e->flag0_cap = mode == MODE_SCREEN ? (int)std::min<long>(e->list_cap, std::max(256, atoi(v) / 256 * 256)) : 0;
    bool ok = true;
    e->in_hdr_cap = up16(B * sizeof(CloudDev)) + up16(B * R * sizeof(RollGeo)) + up16(B * HAF_MAX_VIEWS * sizeof(FrameDev)) + up16(B * HAF_MAX_VIEWS * sizeof(RoiViewDev));     // (haf_score_views: up to HAF_MAX_VIEWS descriptors per request)
    // (+ 48 bytes per cloud: the points of a frame start at a multiple of four points, pack_headers)
    ok &= hipSuccess == e->in_block.ensure(e->in_hdr_cap + (size_t)c.max_points * 3 * sizeof(float) + B * 48);
    ok &= hipSuccess == e->raw.ensure((size_t)c.max_points * 4 + B * HAF_MAX_VIEWS * 16);
    ok &= hipSuccess == e->out_block.ensure(kCntBytes + B * R * sizeof(RollRecordDev));
    if (ok) {
        e->d_counters.p = reinterpret_cast<int *>(e->out_block.dev.p);
        e->d_rec.p = reinterpret_cast<RollRecordDev *>(e->out_block.dev.p + kCntBytes);
    }
    {
        const int nb = bin_bucket_grid(c.grid_h, nullptr);
        e->bkt_ints = nb * nb + 1;
        if ((size_t)c.grid_h * c.grid_w > 16384) {           // grids k_bin_lds cannot hold: the bucket-sorted binning path
            ok &= hipSuccess == e->d_sorted.alloc((size_t)c.max_points * 3);
            ok &= hipSuccess == e->d_bkt.alloc((size_t)3 * B * e->bkt_ints);
        }
    }
    ok &= hipSuccess == e->d_heights.alloc(e->cells_cap);
    ok &= hipSuccess == e->d_rowsum.alloc(e->cells_cap);
    ok &= hipSuccess == e->d_inexact.alloc(B * R);
    ok &= hipSuccess == e->d_iiabs.alloc(B * R);
    ok &= hipSuccess == e->d_ii.alloc(B * R * (H + 1) * (W + 1));
    ok &= hipSuccess == e->d_mask.alloc(e->cells_cap);
    ok &= hipSuccess == e->d_rowcount.alloc(B * R * H);
    ok &= hipSuccess == e->d_rowoff.alloc(2 * (B * R * H + 1));      // whole-chunk and left-over starts (k_scan)
    ok &= hipSuccess == e->d_brcount.alloc(B * R);
    ok &= hipSuccess == e->d_brslot.alloc(B * R);
    if (ok) ok &= hipSuccess == hipMemsetAsync(e->d_brslot.p, 0, B * R * sizeof(unsigned long long), e->stream);   // epoch 0: no request yet (on the engine's stream: in front of its first kernel)
    ok &= hipSuccess == e->d_evalcell.alloc((size_t)e->max_evals_pad);
    ok &= hipSuccess == e->d_flag_list.alloc((size_t)e->list_cap);
    if (mode == MODE_SCREEN) {
        // sized for the three-pass form as well: a model whose decisions crowd inside the screening band is served by
        // the three-pass kernel alone (screen_active)
        ok &= hipSuccess == e->d_X.alloc((size_t)(e->max_evals_pad / kTile) * (size_t)(kHXTileBytes / 4));
        const size_t slots = ((size_t)e->flag0_cap + kSvmBlockEvals - 1) / kSvmBlockEvals * kSvmBlockEvals;
        ok &= hipSuccess == e->d_X1.alloc(slots / kTile * (size_t)(kHXTileBytes / 4));
        ok &= hipSuccess == e->d_ax1.alloc(slots);
        e->part1_stride = (long)slots;
        ok &= hipSuccess == e->d_part1.alloc(slots * 2 * kHListParts);      // class sums per SV tile range (k_svm_h_combine)
        if (e->mdl.t1_cr_available) ok &= hipSuccess == e->d_t1_L.alloc(slots);
        ok &= hipSuccess == e->d_gband.alloc((size_t)e->max_evals_pad * kBandFloats);
        ok &= hipSuccess == e->d_flag0_list.alloc((size_t)e->flag0_cap);
        if (e->mdl.cr_available) ok &= hipSuccess == e->d_flag0b_list.alloc((size_t)e->flag0_cap);
        ok &= hipSuccess == e->d_screen_part.alloc(screen_part_bytes());
        ok &= hipSuccess == e->d_flag0_words.alloc((size_t)e->max_evals_pad / 64);
        ok &= hipSuccess == e->d_flag0_wgcount.alloc((size_t)e->max_evals_pad / 64 / 256 + 1);
    } else {
        ok &= hipSuccess == e->d_X.alloc((size_t)(e->max_evals_pad / kTile) * (size_t)std::max<int>(kTileFloats, kHXTileBytes / 4));
    }
    ok &= hipSuccess == e->d_ax.alloc((size_t)e->max_evals_pad);
    ok &= hipSuccess == e->d_dec.alloc((size_t)e->max_evals_pad);
    ok &= hipSuccess == e->d_labels.alloc(e->cells_cap);
    ok &= hipSuccess == e->d_dec_exact.alloc((size_t)e->list_cap);
    ok &= hipSuccess == e->d_part64.alloc((size_t)e->flag_cap * kRecheckPartRows);
    ok &= hipSuccess == e->d_tier_words.alloc(((size_t)e->flag_cap + 63) / 64 + 4);
    ok &= hipSuccess == e->d_t1_flags.alloc(t1_flag_bytes(e->max_evals_pad));    // (a default-mode engine can fall back to three passes for every evaluation)
    // k_recheck_mfma reads whole workgroups of 64 evaluations (4 groups of 16): round the image up accordingly
    ok &= hipSuccess == e->d_x64.alloc(((size_t)e->flag_cap + 63) / 64 * 64 * kKP);
    ok &= hipSuccess == e->d_flag2_list.alloc((size_t)e->list_cap);
    if (e->mdl.i8_active) {
        ok &= hipSuccess == e->d_flagi_list.alloc((size_t)e->list_cap);
        ok &= hipSuccess == e->d_dec_exacti.alloc((size_t)e->list_cap);
    }
    ok &= hipSuccess == e->d_dec_exact2.alloc((size_t)e->list_cap);
    if (!e->mdl.prob_mode) ok &= hipSuccess == e->d_strict_terms.alloc((size_t)kStrictSlots * e->mdl.n_sv_pad);
    if ((c.flags & HAF_FLAG_KEEP_DEBUG) && mode == MODE_SCREEN) ok &= hipSuccess == e->d_margin.alloc((size_t)e->max_evals_pad);
    if (c.flags & HAF_FLAG_KEEP_DEBUG) {
        // attribute records of the exact-form feature kernels (haf_debug_fetch_attr): 7.6 KB per evaluation, so only for
        // engines of reference size (up to 2 GiB); a larger debug engine runs without them and the fetch says so
        const size_t bytes = (size_t)e->max_evals * kKP * sizeof(AttrRecord);
        if (bytes <= (2ull << 30)) ok &= hipSuccess == e->d_attr.alloc((size_t)e->max_evals * kKP);
    }
    ok &= hipSuccess == e->d_ev16.alloc(e->cells_cap);
    if (e->mdl.prob_mode) {
        ok &= hipSuccess == e->d_own.alloc(e->cells_cap);
        ok &= hipSuccess == e->d_gridf.alloc(e->cells_cap);
        ok &= hipSuccess == e->d_evf.alloc(e->cells_cap);
        ok &= hipSuccess == e->d_ptext.alloc(2 * (size_t)e->list_cap);
    }
    ok &= hipSuccess == e->d_rowmax.alloc(B * R * H);
    ok &= hipSuccess == e->d_topkey.alloc(3 * B * R);          // top vote key, longest-run key, completion counter (k_vote_*)
    if (!ok) return fail(e, HAF_E_DEVICE, std::string("hipMalloc of working buffers failed: ") + hipGetErrorString(hipGetLastError()));
    e->h_counters = reinterpret_cast<int *>(e->out_block.host);
    e->h_rec = reinterpret_cast<RollRecordDev *>(e->out_block.host + kCntBytes);
    HIPCHK(e, hipMemsetAsync(e->d_counters.p, 0, CNT_COUNT * sizeof(int), e->stream));
    e->counters_clean = true;
    return HAF_OK;
}

}  // namespace haf_host
