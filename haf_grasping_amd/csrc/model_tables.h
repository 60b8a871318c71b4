// model_tables.h -- the model tables without a device: the parsed feature / range / model files -> the host image of every device
// table, every parameter struct (device pointers null) and the scalars and flags that go with them (model_tables.cpp).  No HIP runtime
// call and no environment read: engine_tables.cpp uploads the result (upload_tables), the testing build digests it on a CPU
// (haf_test_host_table_digest) and tests/sanitize/table_paths.cpp runs it under the sanitizers.
#pragma once
#include "../../include/hafgrasp.h"
#include "kernels.h"
#include "parsers.h"

#include <string>
#include <vector>

using namespace haf;

namespace haf_host {

// contraction mode: default = screening pass + three-pass refinement; HAF_FLAG_SPLIT_F16 = three passes for everything;
// HAF_FLAG_FP32_MFMA = one fp32 MFMA pass for everything
enum { MODE_SCREEN = 0, MODE_SPLIT = 1, MODE_F32 = 2 };
inline int contraction_mode(const haf_config &c)
{
    if (c.flags & HAF_FLAG_FP32_MFMA) return MODE_F32;
    if (c.flags & HAF_FLAG_SPLIT_F16) return MODE_SPLIT;
    return MODE_SCREEN;
}

// The testing build's environment switches that the table work depends on, one member per HAF_... variable.  engine_tables.cpp fills
// them from test_env in one place (table_switches); the product build leaves every one at its default.
struct TableSwitches {
    bool no_cr = false;                 // HAF_NO_CR
    bool no_lr = false;                 // HAF_NO_LR
    bool cr_no_centre = false;          // HAF_CR_NO_CENTRE
    bool no_cr_t1 = false;              // HAF_NO_CR_T1
    bool no_i8 = false;                 // HAF_NO_I8
    bool no_fast_groups = false;        // HAF_NO_FAST_GROUPS
    bool screen_no_centre = false;      // HAF_SCREEN_NO_CENTRE
    bool lr_unfused = false;            // HAF_LR_UNFUSED
    bool no_lr_plain = false;           // HAF_NO_LR_PLAIN
    bool kappa_t1_measured = false;     // HAF_KAPPA_T1_MEASURED
    bool prob_host_all = false;         // HAF_PROB_HOST_ALL
    bool host_exp_all = false;          // HAF_HOST_EXP_ALL
    // the guard-band scales (engine_state.h: guard_knob): *_set = the variable is there, the value = guard_knob of its text
    bool guard_rel_set = false, guard0_rel_set = false, guard2_rel_set = false, guard_i8_rel_set = false;
    double guard_rel = 1.0, guard0_rel = 1.0, guard2_rel = 1.0, guard_i8_rel = 1.0;
};

struct TableInputs {
    haf_config cfg{};                           // (feature_file: named in a refusal)
    const std::vector<FeatureRow> *features = nullptr;
    const RangeTable *range = nullptr;
    const SvmModel *model = nullptr;
    double mfma_kappa = 12.0, mfma_kappa16 = 12.0;      // haf_engine::mfma_kappa*
    bool generic_kernel = false;
    TableSwitches sw;
};

// The model's tables, declared once for the host (Buf = std::vector: the builder's images) and for the device (Buf = DevBuf,
// engine_state.h: what upload_tables makes of them).  A table that the model does not get stays empty (and is not allocated); a form
// whose tables are missing has its *_available false.
template <template <class> class Buf> struct TableSet {
    Buf<FeatDesc> fd;                   // (scr_mul / scr_add filled in the default mode)
    Buf<float> svt;
    Buf<char> svt_h;                    // split-fp16 SV tile images
    Buf<ScrDesc> sd, sd_cr;
    Buf<ScrDesc3> sd3, sd3_cr;
    Buf<FeatDesc> fd_slot, fd_slot_cr;
    // per-slot constants of the centred screening band (kS0K per-slot entries, then the pair form); corr_lrp: the low-rank form's
    // own correction vectors for the PLAIN epilogue (screen_lrp)
    Buf<ScrCorr> corr, corr_cr, corr_lrp;
    Buf<char> svt0;                     // screening-pass SV tile images
    Buf<char> svt0_cr;                  // the same for the centred-remainder form: fp16(w_n - mu), t_n = 0, coefficient b_n
    // low-rank form of the centred-remainder pass (kernels.h: kLrK; large requests only): projection tiles (rows of B^'), 6-step SV
    // tile images of q~_n
    Buf<char> lr_btiles, svt_lr;
    Buf<char> lr_btiles_in;             // the projection matrix by input k-step (fused form: the projection is the sweep's prologue)
    // tier 1 (three-pass list kernel) in the centred-remainder form, behind SCREEN_CR_POLY: its own SV images (s - m), the centre /
    // linear-term table of the exact-form feature kernel
    Buf<char> svt_h_cr;
    Buf<double> t1_tab;
    Buf<double> sv64, coef64;
    Buf<char> sv_i8;                    // tier 2a, the exact-integer tier (exact8.hip): int8 digit images of the support vectors
};
// THE list of the tables: f(name, the table of every set given), in the order of the digest lines (tests/golden/table_digests.json).
// Everything that handles every table -- the upload, the digests, the sanitizer job's byte sum -- goes through here.
template <class F, class... Set> constexpr void for_each_table(F &&f, Set &...s)
{
    f("fd", s.fd...); f("svt", s.svt...); f("svt_h", s.svt_h...); f("sd", s.sd...); f("sd3", s.sd3...); f("fd_slot", s.fd_slot...);
    f("corr", s.corr...); f("svt0", s.svt0...); f("svt0_cr", s.svt0_cr...); f("sd_cr", s.sd_cr...); f("sd3_cr", s.sd3_cr...);
    f("fd_slot_cr", s.fd_slot_cr...); f("corr_cr", s.corr_cr...); f("lr_btiles", s.lr_btiles...); f("lr_btiles_in", s.lr_btiles_in...);
    f("svt_lr", s.svt_lr...); f("corr_lrp", s.corr_lrp...); f("svt_h_cr", s.svt_h_cr...); f("t1_tab", s.t1_tab...); f("sv64", s.sv64...);
    f("coef64", s.coef64...); f("sv_i8", s.sv_i8...);
}
// ... and it names every member: a table added to the set and not to the list does not compile (TableSlot: a set of one-byte members)
template <class T> struct TableSlot { char c; };
constexpr int table_count()
{
    TableSet<TableSlot> s{};
    int n = 0;
    for_each_table([&n](const char *, auto &) { n++; }, s);
    return n;
}
static_assert(table_count() == (int)sizeof(TableSet<TableSlot>), "for_each_table must visit every member of TableSet");

// The parameter structs (device pointers null until upload_tables sets them) and the scalars and flags that the table work sets.
// Nothing writes to the engine's copy after upload_tables.
struct ModelConsts {
    ScreenParams screen{};
    ScreenParams screen_cr{};    // the centred-remainder form's constants and descriptor tables
    ScreenParams screen_lrp{};   // the feature kernel's constants for the PLAIN epilogue in the low-rank form (centred descriptors, own correction vectors)
    LrBand lr_band{};            // the low-rank form's band constants
    CrParams crp{};
    CrT1Params crt1{};
    SvmParams svm{};
    ExactParams exact{};
    I8Params i8{};
    // probability-output mode (HAF_FLAG_PROBABILITY, prob.hip)
    ProbParams prob{};

    // the scalars and flags, in the order of the "scalars" digest line
    int nf = 0, kx = 0, n_sv_tiles = 0, sv_tile_neg = 0, n_sv_pad = 0;
    double sum_abs_coef = 0;
    bool screen_active = true;           // as the table work sets it; haf_engine::screen_active starts from it and is the one that changes
    bool cr_available = false;           // the centred-remainder tables exist (screen_cr, svt0_cr, ...)
    bool lr_available = false;
    bool lr_fused = true;                // testing build: HAF_LR_UNFUSED = k_project + sweep as two launches
    bool lr_plain_available = false;
    bool t1_cr_available = false, i8_active = false;
    int lr_rank = 0;                     // dimension of the HAF slots' linear span (158 for the reference's Features.txt)
    int gv0 = 0, gv1 = 0;
    bool prob_mode = false;
    // strict tier: an evaluation whose libsvm-order decision value is within this of zero is decided on the HOST with glibc's exp
    // (the device's exp may differ from it in the last bit: 2^-52 per kernel value, i.e. at most 2^-52 sum|coef| in the sum)
    double host_exp_thr = 0.0;
};

template <class T> using HostBuf = std::vector<T>;
// what the builder makes: the host image of every table and the constants
struct ModelTables : TableSet<HostBuf>, ModelConsts {
    // host only, for the testing build's slot-table hook (built once per engine; kept in this struct because the builder is one unit for both
    // libraries): the representative attribute (row of the feature file) of every used slot, and the centred forms' centre per slot
    std::vector<int> slot_rep;
    std::vector<double> slot_mu;
};

// A refusal of the builder: what haf_create hands to fail().  code == HAF_OK: none.
struct TableError {
    int code = HAF_OK;
    std::string msg;
};

TableError build_model_tables(const TableInputs &in, ModelTables &t);

int label_grid_value(int label);
float header_grid_value(int label0, int label1);
double sigma_upper_bound(const double *M, int n, int d);

}  // namespace haf_host
