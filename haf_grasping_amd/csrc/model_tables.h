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

// A table that the model does not get stays empty (and is not allocated); a form whose tables are missing has its *_available false.
struct ModelTables {
    std::vector<FeatDesc> fd;                   // -> d_fd (scr_mul / scr_add filled in the default mode)
    std::vector<float> svt;                     // -> d_svt
    std::vector<char> svt_h;                    // -> d_svt_h
    std::vector<ScrDesc> sd, sd_cr;             // -> d_sd, d_sd_cr
    std::vector<ScrDesc3> sd3, sd3_cr;          // -> d_sd3, d_sd3_cr
    std::vector<FeatDesc> fd_slot, fd_slot_cr;  // -> d_fd_slot, d_fd_slot_cr
    std::vector<ScrCorr> corr, corr_cr, corr_lrp;   // -> d_corr, d_corr_cr, d_corr_lrp (kS0K per-slot entries, then the pair form)
    // host only, for the testing build's slot-table hook (built once per engine; kept in this struct because the builder is one unit for both
    // libraries): the representative attribute (row of the feature file) of every used slot, and the centred forms' centre per slot
    std::vector<int> slot_rep;
    std::vector<double> slot_mu;
    std::vector<char> svt0, svt0_cr;            // -> d_svt0, d_svt0_cr
    std::vector<char> lr_btiles, lr_btiles_in, svt_lr;   // -> d_lr_btiles, d_lr_btiles_in, d_svt_lr
    std::vector<char> svt_h_cr;                 // -> d_svt_h_cr
    std::vector<double> t1_tab;                 // -> d_t1_tab
    std::vector<double> sv64, coef64;           // -> d_sv64, d_coef64
    std::vector<char> sv_i8;                    // -> d_sv_i8

    ScreenParams screen{}, screen_cr{}, screen_lrp{};
    LrBand lr_band{};
    CrParams crp{};
    CrT1Params crt1{};
    SvmParams svm{};
    ExactParams exact{};
    I8Params i8{};
    ProbParams prob{};

    int nf = 0, kx = 0, n_sv_tiles = 0, sv_tile_neg = 0, n_sv_pad = 0;
    double sum_abs_coef = 0;
    bool screen_active = true, cr_available = false, lr_available = false, lr_fused = true, lr_plain_available = false;
    bool t1_cr_available = false, i8_active = false;
    int lr_rank = 0;
    int gv0 = 0, gv1 = 0;
    bool prob_mode = false;
    double host_exp_thr = 0.0;
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
