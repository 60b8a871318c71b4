// table_paths.cpp -- CPU sanitizer job of the model tables (tests/test_tables_cpu.py): model_tables.cpp + parsers.cpp built with
// -fsanitize=address,undefined and driven by this program, which has its own main and touches no device.
//   table_paths MANIFEST [sweep]
// Every line of MANIFEST is "feature_file range_file model_file flags grid expected_code": the files are parsed, the builder runs with
// every switch at its default and kappa 12, and its code must be the expected one (0: the tables are built; else the refusal's).  Every
// image of a built case is then read from its first to its last byte, so that the sanitizer sees the vectors' true extents.
// With `sweep` the SV tile images of the screening sweep (svt0, svt0_cr, svt_lr) are also walked the way the sweep's tables are handed
// out and decoded (tests/sweep_cases.py): tile by tile, every (SV, slot) half at h_image_offset and the tail piece's 64 floats; the
// padding columns must hold zeros, the coefficients of the tiles before sv_tile_neg must be >= 0 and those behind it < 0.
#include "../../haf_grasping_amd/csrc/model_tables.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// one tile table in the sweep's layout: `steps` k-steps of 32 slots, `tile_bytes` per tile, the tail piece behind `mat_bytes`
static int walk_tiles(const std::vector<char> &img, int n_tiles, int neg, int slots, int mat_bytes, int tile_bytes, int n_sv, const char *name)
{
    if (img.empty()) return 0;
    if (img.size() != (size_t)n_tiles * (size_t)tile_bytes) { fprintf(stderr, "%s: %zu bytes for %d tiles\n", name, img.size(), n_tiles); return 1; }
    int live = 0;
    for (int t = 0; t < n_tiles; t++) {
        const char *tile = img.data() + (size_t)t * tile_bytes;
        float tail[64];
        memcpy(tail, tile + mat_bytes, sizeof tail);
        for (int j = 0; j < 32; j++) {
            const float coef = tail[32 + j];
            unsigned any = 0;
            for (int k = 0; k < slots; k++) {
                unsigned short h;
                memcpy(&h, tile + haf::h_image_offset(j, k), 2);
                any |= (unsigned)(h & 0x7fffu);
            }
            if (coef == 0.0f) {
                if (any || tail[j] != 0.0f) { fprintf(stderr, "%s: padding column %d of tile %d is not zero\n", name, j, t); return 1; }
                continue;
            }
            live++;
            if ((t < neg) != (coef >= 0.0f)) { fprintf(stderr, "%s: coefficient %g in tile %d (first negative tile %d)\n", name, (double)coef, t, neg); return 1; }
        }
    }
    if (live != n_sv) { fprintf(stderr, "%s: %d live columns for %d support vectors\n", name, live, n_sv); return 1; }
    return 0;
}

static int run_line(const std::string &line, bool sweep)
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
    if (e.code == HAF_OK) for_each_table([&s](const char *, const auto &v) { s += sum_bytes(v); }, t);
    printf("%s flags %u grid %d: code %d (%s) cr %d lr %d t1 %d i8 %d bytes %llu\n", mf.c_str(), flags, grid, e.code, e.msg.c_str(),
           (int)t.cr_available, (int)t.lr_available, (int)t.t1_cr_available, (int)t.i8_active, s);
    if (e.code != want) { fprintf(stderr, "expected code %d, got %d: %s\n", want, e.code, e.msg.c_str()); return 1; }
    if (sweep && e.code == HAF_OK) {
        printf("  sweep tables: %d tiles, first negative %d\n", t.n_sv_tiles, t.sv_tile_neg);
        if (walk_tiles(t.svt0, t.n_sv_tiles, t.sv_tile_neg, haf::kS0K, haf::kS0MatBytes, haf::kS0SvTileBytes, model.n_sv, "svt0") ||
            walk_tiles(t.svt0_cr, t.n_sv_tiles, t.sv_tile_neg, haf::kS0K, haf::kS0MatBytes, haf::kS0SvTileBytes, model.n_sv, "svt0_cr") ||
            walk_tiles(t.svt_lr, t.n_sv_tiles, t.sv_tile_neg, haf::kLrK, haf::kLrMatBytes, haf::kLrSvTileBytes, model.n_sv, "svt_lr"))
            return 1;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2 && !(argc == 3 && std::string(argv[2]) == "sweep")) { fprintf(stderr, "usage: table_paths MANIFEST [sweep]\n"); return 2; }
    const bool sweep = argc == 3;
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    int lines = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        if (run_line(line, sweep) != 0) return 1;
        lines++;
    }
    printf("table sanitizer job ok (%d cases)\n", lines);
    return 0;
}
