// table_paths.cpp -- CPU sanitizer job of the model tables (tests/test_tables_cpu.py): model_tables.cpp + parsers.cpp built with
// -fsanitize=address,undefined and driven by this program, which has its own main and touches no device.
//   table_paths MANIFEST
// Every line of MANIFEST is "feature_file range_file model_file flags grid expected_code": the files are parsed, the builder runs with
// every switch at its default and kappa 12, and its code must be the expected one (0: the tables are built; else the refusal's).  Every
// image of a built case is then read from its first to its last byte, so that the sanitizer sees the vectors' true extents.
#include "../../haf_grasping_amd/csrc/model_tables.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

using namespace haf_host;

template <class T> static unsigned long long sum_bytes(const std::vector<T> &v)
{
    unsigned long long s = 0;
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); i++) s += p[i];
    return s;
}

static int run_line(const std::string &line)
{
    std::istringstream is(line);
    std::string ff, rf, mf;
    unsigned flags = 0;
    int grid = 0, want = 0;
    if (!(is >> ff >> rf >> mf >> flags >> grid >> want)) { fprintf(stderr, "malformed manifest line: %s\n", line.c_str()); return 1; }
    std::vector<FeatureRow> features;
    RangeTable range;
    SvmModel model;
    std::string err;
    if (!load_features(ff, features, err) || !load_range(rf, range, err) || !load_model(mf, model, err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 1;
    }
    TableInputs in;
    in.cfg.feature_file = ff.c_str(); in.cfg.range_file = rf.c_str(); in.cfg.model_file = mf.c_str();
    in.cfg.flags = flags;
    in.cfg.grid_h = in.cfg.grid_w = grid;
    in.cfg.nr_features_without_shaf = 302;          // haf_config_default
    in.features = &features; in.range = &range; in.model = &model;
    in.generic_kernel = model.kernel_type != HAF_KERNEL_RBF;
    ModelTables t;
    const TableError e = build_model_tables(in, t);
    unsigned long long s = 0;
    if (e.code == HAF_OK)
        s = sum_bytes(t.fd) + sum_bytes(t.svt) + sum_bytes(t.svt_h) + sum_bytes(t.sd) + sum_bytes(t.sd_cr) + sum_bytes(t.sd3) + sum_bytes(t.sd3_cr) +
            sum_bytes(t.fd_slot) + sum_bytes(t.fd_slot_cr) + sum_bytes(t.corr) + sum_bytes(t.corr_cr) + sum_bytes(t.corr_lrp) + sum_bytes(t.svt0) +
            sum_bytes(t.svt0_cr) + sum_bytes(t.lr_btiles) + sum_bytes(t.lr_btiles_in) + sum_bytes(t.svt_lr) + sum_bytes(t.svt_h_cr) +
            sum_bytes(t.t1_tab) + sum_bytes(t.sv64) + sum_bytes(t.coef64) + sum_bytes(t.sv_i8);
    printf("%s flags %u grid %d: code %d (%s) cr %d lr %d t1 %d i8 %d bytes %llu\n", mf.c_str(), flags, grid, e.code, e.msg.c_str(),
           (int)t.cr_available, (int)t.lr_available, (int)t.t1_cr_available, (int)t.i8_active, s);
    if (e.code != want) { fprintf(stderr, "expected code %d, got %d: %s\n", want, e.code, e.msg.c_str()); return 1; }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: table_paths MANIFEST\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    int lines = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        if (run_line(line) != 0) return 1;
        lines++;
    }
    printf("table sanitizer job ok (%d cases)\n", lines);
    return 0;
}
