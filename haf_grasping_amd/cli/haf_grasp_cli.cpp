// haf_grasp_cli -- ROS-free stand-in for the demo flow of the reference (README:29-41): the client
// (src/calc_grasppoints_action_client.cpp) loads a .pcd, fills a GraspInput from its parameters and waits for the
// GraspOutput.  This tool does the same against libhafgrasp.so through the C-ABI, in C++ like the reference's host code.
//
// Parameter surface = the client's ROS params/services (client.cpp:79-118, 214-300):
//   --center x y z            grasp_search_center            (default 0 0 0)
//   --search-size x y         grasp_search_size_x/y in cm WITHOUT the border; the client adds 14 (client.cpp:183-184)
//   --approach x y z          gripper_approach_vector        (default 0 0 1)
//   --max-time s              max_calculation_time           (default 50)
//   --show-only-best          show_only_best_grasp
//   --gripper-width w         gripper_width                  (default 1)
// plus the engine's generalisations: --grid N, --rolls N, --roll-step deg, and
//   --gpus N [--shard rolls|clouds]   N GPUs of this node in ONE process through haf_create_multi: the rolls of every request
//                                     sharded with one RCCL all-gather of the roll records (default), or the clouds given on
//                                     the command line sharded with one RCCL all-reduce(max) electing the best grasp
//   --shards-per-gpu K                K shards on every GPU (they share its RCCL rank)
//   --probability                     svm_with_probability: "svm-predict -b 1" output as show_predicted_gps reads it (model with probA/probB)
//   --hypotheses                      also print the per-roll hypotheses the server publishes when show_only_best is off
//   --top-k N                         after the normal output, "top <rank> <hypothesis>" for the N best distinct candidates of the
//                                     goal (haf_top_grasps); --top-radius cells, --top-rolls steps, --top-dist metres set its suppression
//                                     (server.cpp:962-969), in its string format
//   --gripper default|OPEN,THICK,BREADTH,TIP,LENGTH,PALM_W,PALM_B,PALM_H   with --top-k: after the "top" lines one line per candidate,
//                                     "clear <rank> <free> fingers <n0> <n1> palm <n> between <n> width <w> offset <o> top <t>": the
//                                     scene's points inside the boxes of that parallel-jaw gripper (metres; the default is nominal, no
//                                     real gripper's) placed at the candidate (haf_check_grasps).  The scene is the --depth frame, or
//                                     the .pcd cloud as an N x 1 frame.  Without it no output line changes
//   --fit-opening default|MIN,MAX[,SHIFT]   with --top-k: behind the "top" and "clear" lines one line per candidate,
//                                     "open <rank> <found> opening <m> shift <m> between <n> hits <n> sym <m>": the smallest free opening
//                                     between MIN and MAX metres of the --gripper (the default one without it; its own opening is not
//                                     read), moved sideways by at most SHIFT, the points between the fingers and in the fingers and
//                                     the palm there, and the smallest free opening without a shift (haf_fit_openings; same scene)
//   --check-space default|STEP,TOL_ABS,TOL_REL[,MAX_HIT,MAX_UNKNOWN]   with --top-k and one or more --depth views: behind the "top", "clear"
//                                     and "open" lines one line per candidate, "space <rank> <clear> hit <n> hidden <n> unseen <n> free
//                                     <n> between-hit <n>": the sample points of the --gripper's volume (the default one without it) that
//                                     the views saw a surface at, could not see behind a surface, did not see at all and saw through,
//                                     over the fingers and the palm, and the ones between the fingers with a surface (haf_check_space,
//                                     through hafshim::seen_free_hypotheses, whose strings of the clear candidates go to stderr as
//                                     "<file>: seen free: <hypothesis>")
//   --map-out PREFIX                  with --depth: the goal's votes in the pixels of the (first) depth image (haf_grasp_map), written as
//                                     PREFIX.vote.pgm and PREFIX.roll.pgm: 16-bit binary PGMs of the image's size, sample = value + 32768
//                                     (a pixel without a cell: vote -32768 -> 0, roll -1 -> 32767)
//   --mask FILE.pgm                   with --depth: an 8-bit binary PGM of the image's size; after the normal output one line
//                                     "mask <u> <v> <hypothesis>" for the best pixel under its non-zero samples whose vote is at
//                                     least --mask-min-vote (default 1), or "mask none" (haf_grasp_map_best)
//   --labels FILE.pgm                 with --depth: an 8- or 16-bit binary PGM of the image's size, an instance-label image (0 background,
//                                     1.. the objects); after the normal output one line "object <label> <u> <v> <hypothesis>" per object
//                                     that has a pixel whose vote is at least --mask-min-vote, best first (haf_grasp_map_labels: one
//                                     device pass for all objects); may be combined with --roi-mask
//   --labels FILE.pgm --measure       no request is scored: one line "shape <label> found <0|1> pixels <n> points <n> centroid <x y z> box
//                                     <xmin ymin zmin xmax ymax zmax> width <narrow_width> long <long_width> yaw <deg> diameter <d>
//                                     height <h>" per label 1..max (haf_measure_labels; --plane A B C D gives the heights, else nan)
//   --segment ... --per-object [MARGIN]   instead of the one request around --center: one request per segmented object, centred on its
//                                     box with a grasp area that covers it and MARGIN (default 4) more cells (haf_measure_labels,
//                                     haf_object_input, batched haf_score_frames_roi under the label image); one line "object <label>
//                                     <u> <v> <hypothesis> width <narrow_width> yaw <deg> height <h>" per object, best first
//   --segment ... --per-object [MARGIN] --fused   the same lines from ONE haf_score_objects call per chunk of max_clouds objects: the
//                                     frame is staged and deprojected once and every request evaluates only near its own object
//   --segment MIN_H,MAX_H,GAP,MIN_PX | default
//                                     with --depth: no segmenter at hand -- the first view is clustered into objects on the device
//                                     (haf_segment_frame: pixels MIN_H..MAX_H metres above the support plane, MAX_H <= 0: no upper limit;
//                                     4-neighbours closer than GAP metres are one object; objects of fewer than MIN_PX pixels are dropped;
//                                     at most 255 objects).  --plane A B C D: the plane, height = A x + B y + C z + D in the base frame
//                                     (default: through --center, normal = the approach vector: the caller owns the table height).
//                                     --plane fit[,TOL,N_HYP]: the plane is the view's dominant plane, fitted on the device
//                                     (haf_fit_plane: points within TOL metres, N_HYP hypotheses; defaults 0.005, 256); --plane-mask
//                                     FILE.pgm: only the pixels under its non-zero samples take part in the fit.  One line
//                                     "plane <a> <b> <c> <d> inliers <n> rms <r>" goes to stdout before everything else; where no plane
//                                     is found ("plane none") the default plane stands in.
//                                     Without --labels the label image feeds the "object" lines; --labels-out FILE.pgm writes it as an
//                                     8-bit PGM; --segment-roi also scores only under it (with ONE --depth, not with --roi-mask)
//   --segment-cells MIN_H,MAX_H,CELL,MIN_PTS[,STEP] | default   --segment with haf_segment_cells as the segmenter: the objects are
//                                     connected occupied cells of the top-down grid (CELL metres; STEP > 0: neighbouring cells whose
//                                     tops differ by more do not link) instead of neighbouring pixels.  Combines with --plane,
//                                     --per-object [MARGIN] --fused and --labels-out like --segment and prints the same "object" lines;
//                                     --cell-labels-out FILE.pgm writes the top-down label grid as an 8-bit PGM.  Works with --depth
//                                     and, in its place, with ONE .pcd: the cloud as an N x 1 frame in the base frame
//   --labels FILE.pgm --labels-camera FX FY CX CY [--labels-pose <12 floats>] [--transfer NEAR,TOL_ABS,TOL_REL,SPLAT]
//                                     the label image is ANOTHER camera's (the colour camera an instance segmenter ran on): any size,
//                                     that camera's intrinsics, --labels-pose the rows 0..2 of ITS sensor-to-base matrix (default
//                                     identity).  haf_transfer_labels carries it over to the first view's pixels behind a z-buffer
//                                     (--transfer: its parameters, default 0.05,0.01,0.01,1) in front of the plain --labels pick, of
//                                     --measure, and of --per-object [MARGIN] --fused (then without --segment: the objects are the
//                                     image's; --plane A B C D gives their heights); --labels-out FILE.pgm writes the transferred
//                                     image.  Without --labels-camera every option behaves as before
//   --roi-mask FILE.pgm               with ONE --depth: an 8-bit binary PGM of the image's size; only the cells near the cells of the
//                                     pixels under its non-zero samples are scored (haf_score_frames_roi) and the grasp printed is the
//                                     best one there; --hypotheses, --top-k and --map-out work behind it on the restricted request
//   --view-roi-mask FILE.pgm          behind a --depth: the same kind of mask for the VIEW opened last, of as many views as there are; the
//                                     fused request is scored only near the cells of the masked pixels of all masked views
//                                     (haf_score_views_roi); a view without the option contributes its points and selects nothing.
//                                     Not together with --roi-mask; --hypotheses, --top-k, --map-out and --labels work behind it
//   --stack FILE.pgm                  behind a --depth: a further exposure of that view (same camera, same pose, same size), up to
//                                     HAF_MAX_STACK per view; read only with --depth-filter
//   --depth-filter RADIUS,SUPPORT,TOL_ABS,TOL_REL[,MIN_VALID]   ("default": 2,6,0.004,0.01,1) every view's exposures go through
//                                     haf_filter_depth -- per pixel the lower median of the valid samples, then the spatial support
//                                     test -- and the filtered image is scored in the view's place; --filtered-out FILE.pgm writes
//                                     the first view's filtered image as a 16-bit PGM.  Without --depth-filter nothing changes
//   --depth FILE.pgm --intrinsics fx fy cx cy   in place of the .pcd arguments: a 16-bit depth image (binary PGM) as the sensor
//                                     delivers it, deprojected and transformed on the device (haf_score_frames); optional
//                                     --depth-scale S (metres per unit, default 0.001), --depth-range MIN MAX (metres, 0 = no limit),
//                                     --sensor-pose with the 12 floats of rows 0..2 of the sensor-to-base matrix (default identity).
//                                     --hypotheses and --top-k work with it (the per-roll hypotheses are then read from the ranked
//                                     candidates of haf_top_grasps, one per roll: the same records through the same pose).
//                                     A repeated --depth opens a further VIEW of the one request (a second camera, or a second pose):
//                                     the valid points of all views are fused into one cloud on the device (haf_score_views).
//                                     --intrinsics, --depth-scale, --depth-range and --sensor-pose apply to the view opened last; a view
//                                     inherits the previous view's values until it overrides them; given before the first --depth
//                                     they apply to the first view
#include "../../include/hafgrasp.h"

#include "shim_core.h"

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

static void usage();

// --gpus N: the same requests through the multi-device front end of the C-ABI
static int run_multi(haf_config cfg, const haf_grasp_input &in, int gpus, int shards_per_gpu, const std::string &shard, int argc, char **argv,
                     int first_cloud)
{
    // shards_per_gpu > 1: every GPU carries several shards (they share its RCCL rank): also how a one-GPU machine runs sharded
    std::vector<int32_t> devices;
    for (int k = 0; k < shards_per_gpu; k++)
        for (int g = 0; g < gpus; g++) devices.push_back(g);
    gpus = (int)devices.size();
    const bool by_cloud = shard == "clouds";
    const int n_clouds = argc - first_cloud;
    if (by_cloud) cfg.max_clouds = n_clouds;
    haf_multi *m = nullptr;
    if (haf_create_multi(&cfg, devices.data(), gpus, by_cloud ? HAF_SHARD_CLOUDS : HAF_SHARD_ROLLS, &m) != HAF_OK) {
        fprintf(stderr, "haf_create_multi: %s\n", haf_multi_last_error(nullptr));
        return 1;
    }
    int32_t n_shards = 0, n_ranks = 0, ver = 0;
    haf_multi_info(m, &n_shards, &n_ranks, &ver);
    fprintf(stderr, "%d shards on %d RCCL ranks (RCCL %d), sharding %s\n", n_shards, n_ranks, ver, by_cloud ? "clouds" : "rolls");
    int rc = 0;
    std::vector<float *> xyz((size_t)n_clouds, nullptr);
    std::vector<haf_cloud> clouds((size_t)n_clouds);
    for (int i = 0; i < n_clouds; i++) {
        size_t n = 0;
        char err[256];
        if (haf_pcd_load(argv[first_cloud + i], &xyz[(size_t)i], &n, err, sizeof err) != HAF_OK) { fprintf(stderr, "%s: %s\n", argv[first_cloud + i], err); return 1; }
        clouds[(size_t)i] = haf_cloud{xyz[(size_t)i], n, 3, 0};
    }
    std::vector<haf_grasp_output> out((size_t)n_clouds);
    if (by_cloud) {
        std::vector<haf_grasp_input> ins((size_t)n_clouds, in);
        int32_t best = -1;
        if (haf_score_batch_sharded(m, n_clouds, clouds.data(), ins.data(), out.data(), &best) != HAF_OK) { fprintf(stderr, "%s\n", haf_multi_last_error(m)); rc = 1; }
        else {
            for (int i = 0; i < n_clouds; i++) printf("%s\n", hafshim::hypothesis_string(out[(size_t)i], cfg.roll_step_deg).c_str());
            fprintf(stderr, "best grasp of the batch: cloud %d (%s), vote %d\n", best, argv[first_cloud + best], out[(size_t)best].best_vote);
        }
    } else {
        for (int i = 0; i < n_clouds; i++) {
            if (haf_score_sharded(m, &clouds[(size_t)i], &in, &out[(size_t)i]) != HAF_OK) { fprintf(stderr, "%s: %s\n", argv[first_cloud + i], haf_multi_last_error(m)); rc = 1; continue; }
            printf("%s\n", hafshim::hypothesis_string(out[(size_t)i], cfg.roll_step_deg).c_str());
            fprintf(stderr, "%s: %lld evaluations, best vote %d at row %d col %d roll %d\n", argv[first_cloud + i], (long long)out[(size_t)i].n_evals,
                    out[(size_t)i].best_vote, out[(size_t)i].best_row, out[(size_t)i].best_col, out[(size_t)i].best_roll);
        }
    }
    for (float *p : xyz) haf_free(p);
    haf_destroy_multi(m);
    return rc;
}

static void usage()
{
    fprintf(stderr,
            "usage: haf_grasp_cli --features F --range R --model M [options] cloud.pcd [cloud2.pcd ...]\n"
            "       haf_grasp_cli --features F --range R --model M [options] --depth FILE.pgm --intrinsics fx fy cx cy\n"
            "                     [--depth-scale S] [--depth-range MIN MAX] [--sensor-pose m00 m01 ... m23]\n"
            "                     [--depth FILE2.pgm [its --intrinsics, --depth-scale, --depth-range, --sensor-pose] ...]\n"
            "  --center x y z  --search-size x y  --approach x y z  --max-time s  --show-only-best  --gripper-width w\n"
            "  --grid N  --rolls N  --roll-step deg  --device d  --per-roll  --hypotheses  --probability  --grid-out FILE\n"
            "  --top-k N [--top-radius cells] [--top-rolls steps] [--top-dist m] [--gripper default|OPEN,THICK,BREADTH,TIP,LENGTH,PALM_W,PALM_B,PALM_H]\n"
            "           [--fit-opening default|MIN,MAX[,SHIFT]]\n"
            "           [--check-space default|STEP,TOL_ABS,TOL_REL[,MAX_HIT,MAX_UNKNOWN]]   (with --top-k and one or more --depth views)\n"
            "  --map-out PREFIX  --mask FILE.pgm  --labels FILE.pgm [--mask-min-vote N]      (with --depth)\n"
            "  --roi-mask FILE.pgm                                         (with one --depth)\n"
            "  --stack FILE.pgm                                            (behind a --depth: a further exposure of that view)\n"
            "  --depth-filter RADIUS,SUPPORT,TOL_ABS,TOL_REL[,MIN_VALID] | default   [--filtered-out FILE.pgm]\n"
            "  --view-roi-mask FILE.pgm                                    (behind a --depth: the mask of that view)\n"
            "  --labels FILE.pgm --measure [--plane A B C D]     --segment ... --per-object [MARGIN] [--fused]      (with ONE --depth)\n"
            "  --segment-cells MIN_H,MAX_H,CELL,MIN_PTS[,STEP] | default  [--plane ...] [--per-object [MARGIN] [--fused]] [--labels-out FILE.pgm] [--cell-labels-out FILE.pgm]   (with --depth, or with one cloud.pcd)\n"
            "  --segment MIN_H,MAX_H,GAP,MIN_PX | default  [--plane A B C D | --plane fit[,TOL,N_HYP] [--plane-mask FILE.pgm]] [--labels-out FILE.pgm] [--segment-roi]   (with --depth)\n"
            "  --labels FILE.pgm --labels-camera FX FY CX CY [--labels-pose m00 m01 ... m23] [--transfer NEAR,TOL_ABS,TOL_REL,SPLAT] [--labels-out FILE.pgm]\n"
            "                     (with --depth: the labels are ANOTHER camera's; alone, with --measure, or with --per-object [MARGIN] --fused)\n"
            "  --gpus N [--shard rolls|clouds] [--shards-per-gpu K]\n");
}

// --gripper: the clearance of the ranked candidates (haf_check_grasps) against `scene`
// --fit-opening: their smallest free openings (haf_fit_openings) against the same scene
// --check-space: what the depth views have SEEN of the gripper's volume at the candidates (haf_check_space), every --depth view a view
struct ClearOptions { bool on = false; haf_gripper gripper; bool fit = false; haf_opening_params opening; bool space = false; haf_space_params seen; };

// --gripper default | OPEN,THICK,BREADTH,TIP,LENGTH,PALM_W,PALM_B,PALM_H (metres; max_hits and min_between stay the library's)
static bool parse_gripper(const char *arg, haf_gripper *g)
{
    haf_gripper_default(g);
    if (strcmp(arg, "default") == 0) return true;
    float v[8];
    char tail = 0;
    if (sscanf(arg, "%f,%f,%f,%f,%f,%f,%f,%f%c", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &tail) != 8) return false;
    g->opening = v[0]; g->finger_thickness = v[1]; g->finger_breadth = v[2]; g->tip_depth = v[3]; g->finger_length = v[4];
    g->palm_width = v[5]; g->palm_breadth = v[6]; g->palm_height = v[7];
    return true;
}

// --fit-opening default | MIN,MAX[,SHIFT] (metres; max_hits and min_between stay the library's)
static bool parse_opening(const char *arg, haf_opening_params *p)
{
    haf_opening_default(p);
    if (strcmp(arg, "default") == 0) return true;
    float v[3] = {0.0f, 0.0f, 0.0f};
    char tail = 0;
    const int n = sscanf(arg, "%f,%f,%f%c", &v[0], &v[1], &v[2], &tail);
    if (n != 2 && n != 3) return false;
    p->min_opening = v[0]; p->max_opening = v[1]; p->max_shift = v[2];
    return true;
}

// --check-space default | STEP,TOL_ABS,TOL_REL[,MAX_HIT,MAX_UNKNOWN] (metres; near_m and min_between_hit stay the library's)
static bool parse_space(const char *arg, haf_space_params *p)
{
    haf_space_default(p);
    if (strcmp(arg, "default") == 0) return true;
    float v[3];
    int m[2] = {p->max_hit, p->max_unknown};
    char tail = 0;
    // (three fields or five, nothing behind them: the shorter form is scanned on its own so that "a,b,c,1" and "a,b,cx" are refused)
    if (sscanf(arg, "%f,%f,%f,%d,%d%c", &v[0], &v[1], &v[2], &m[0], &m[1], &tail) != 5 && sscanf(arg, "%f,%f,%f%c", &v[0], &v[1], &v[2], &tail) != 3) return false;
    p->sample_step = v[0]; p->tol_abs = v[1]; p->tol_rel = v[2]; p->max_hit = m[0]; p->max_unknown = m[1];
    return true;
}

static void print_openings(haf_engine *eng, const char *what, const ClearOptions &clear, const haf_frame &scene, int32_t n,
                           const haf_grasp_candidate *cands, int *rc);
static void print_top(haf_engine *eng, const haf_config &cfg, const char *what, int top_k, int top_radius, int top_rolls, double top_dist, int *rc,
                      const ClearOptions *clear = nullptr, const haf_frame *scene = nullptr, int32_t n_scene_views = 1)
{
    haf_top_params tp;
    haf_top_params_default(eng, &tp);
    tp.k = top_k;
    if (top_radius >= 0) tp.cell_radius = top_radius;
    if (top_rolls >= 0) tp.roll_window = top_rolls;
    if (top_dist >= 0.0) tp.min_dist_m = top_dist;
    std::vector<std::string> top;
    std::string serr;
    if (hafshim::top_hypotheses(eng, cfg, tp, &top, &serr) != HAF_OK) {
        fprintf(stderr, "%s: %s\n", what, serr.c_str());
        *rc = 1;
    }
    for (size_t t = 0; t < top.size(); t++) printf("top %zu %s\n", t + 1, top[t].c_str());
    if (!clear || !(clear->on || clear->fit || clear->space) || !scene) return;
    // the same candidates once more, as poses: "clear <rank> <free> fingers <n0> <n1> palm <n> between <n> width <w> offset <o> top <t>"
    std::vector<haf_grasp_candidate> cand((size_t)std::max(1, cfg.max_clouds) * (size_t)std::max(1, tp.k));
    std::vector<int32_t> found((size_t)std::max(1, cfg.max_clouds), 0);
    if (haf_top_grasps(eng, &tp, cand.data(), found.data()) != HAF_OK) { fprintf(stderr, "%s: --gripper: %s\n", what, haf_last_error(eng)); *rc = 1; return; }
    const int32_t n = found[0];
    if (n < 1) return;
    std::vector<haf_grasp_clearance> rows((size_t)n);
    if (clear->on && haf_check_grasps(eng, scene, nullptr, &clear->gripper, n, cand.data(), sizeof(haf_grasp_candidate), rows.data(), nullptr, nullptr) != HAF_OK) {
        fprintf(stderr, "%s: --gripper: %s\n", what, haf_last_error(eng));
        *rc = 1;
        return;
    }
    for (int32_t t = 0; clear->on && t < n; t++) {
        const haf_grasp_clearance &c = rows[(size_t)t];
        printf("clear %d %d fingers %d %d palm %d between %d width %.9g offset %.9g top %.9g\n", t + 1, c.free, c.n_finger[0], c.n_finger[1], c.n_palm,
               c.n_between, c.width_m, c.offset_m, c.top_m);
    }
    if (clear->fit) print_openings(eng, what, *clear, *scene, n, cand.data(), rc);
    if (!clear->space || *rc) return;
    // and once more: "space <rank> <clear> hit <n> hidden <n> unseen <n> free <n> between-hit <n>", the first four over fingers and palm
    if (scene->kind == HAF_FRAME_XYZ_F32) { fprintf(stderr, "%s: --check-space needs --depth views\n", what); *rc = 1; return; }
    haf_gripper grip = clear->gripper;
    if (!clear->on) haf_gripper_default(&grip);
    // through the shim, as an adapter would ask: every candidate's row, and the clear ones as hypothesis strings (to stderr: stdout
    // keeps one line per candidate)
    std::vector<haf_grasp_space> seen;
    std::vector<std::string> seen_free;
    if (hafshim::seen_free_hypotheses(eng, cfg, tp, scene, n_scene_views, grip, clear->seen, &seen_free, &serr, &seen) != HAF_OK || seen.size() != (size_t)n) {
        fprintf(stderr, "%s: --check-space: %s\n", what, serr.c_str());
        *rc = 1;
        return;
    }
    for (size_t t = 0; t < seen_free.size(); t++) fprintf(stderr, "%s: seen free: %s\n", what, seen_free[t].c_str());
    for (int32_t t = 0; t < n; t++) {
        const haf_grasp_space &g = seen[(size_t)t];
        int64_t st[4] = {0, 0, 0, 0};
        for (int r = HAF_SPACE_FINGER0; r <= HAF_SPACE_PALM; r++)
            for (int k = 0; k < 4; k++) st[k] += g.n[r][k];
        printf("space %d %d hit %lld hidden %lld unseen %lld free %lld between-hit %d\n", t + 1, g.clear, (long long)st[HAF_SPACE_HIT],
               (long long)st[HAF_SPACE_HIDDEN], (long long)st[HAF_SPACE_UNSEEN], (long long)st[HAF_SPACE_FREE], g.n[HAF_SPACE_BETWEEN][HAF_SPACE_HIT]);
    }
}

// "open <rank> <found> opening <m> shift <m> between <n> hits <n> sym <m>" per candidate
static void print_openings(haf_engine *eng, const char *what, const ClearOptions &clear, const haf_frame &scene, int32_t n, const haf_grasp_candidate *cands,
                           int *rc)
{
    haf_gripper gripper = clear.gripper;
    if (!clear.on) haf_gripper_default(&gripper);
    std::vector<haf_grasp_opening> fits((size_t)n);
    if (haf_fit_openings(eng, &scene, nullptr, &gripper, &clear.opening, n, cands, sizeof(haf_grasp_candidate), fits.data(), nullptr, nullptr,
                         nullptr, nullptr) != HAF_OK) {
        fprintf(stderr, "%s: --fit-opening: %s\n", what, haf_last_error(eng));
        *rc = 1;
        return;
    }
    for (int32_t t = 0; t < n; t++) {
        const haf_grasp_opening &o = fits[(size_t)t];
        printf("open %d %d opening %.9g shift %.9g between %d hits %d sym %.9g\n", t + 1, o.found, o.opening_m, o.shift_m, o.n_between,
               o.n_finger[0] + o.n_finger[1] + o.n_palm, o.sym_opening_m);
    }
}

// --depth: one goal whose cloud is a depth image, deprojected on the device.  stdout as for a .pcd: with --hypotheses every roll's own
// hypothesis first (server.cpp:962-969: !show_only_best, vote > graspval_th, the rolls the sequential loop would have executed), then
// the overall best.  A roll's hypothesis is its record through haf_roll_pose's pose; haf_score_frames keeps the records on the
// device, and haf_top_grasps hands them back: with an in-roll radius of the whole grid and no cross-roll suppression its candidates
// are exactly one per roll whose vote exceeds graspval_th, eval = vote - 20 (> 10, so the reference's clamp never acts).
// Several --depth: the views of the one goal, fused on the device (haf_score_views); one --depth is haf_score_frames as ever.
struct DepthView { std::string path; haf_frame frame; std::string roi_path; std::vector<std::string> stack; };      // roi_path: --view-roi-mask of this view; stack: its --stack exposures
// --map-out / --mask: the goal's votes in the pixels of the FIRST view (haf_grasp_map, haf_grasp_map_best)
// --roi-mask: the request itself is restricted to the cells near the masked pixels' cells (haf_score_frames_roi)
// --view-roi-mask: the same for a fused request, a mask per view (haf_score_views_roi)
// --labels: the best grasp per object of an instance-label image over the first view (haf_grasp_map_labels)
// --depth-filter: every view's exposures (its --depth and its --stack files) through haf_filter_depth before the view is scored;
// --filtered-out: the filtered image of the first view
struct MapOptions {
    ClearOptions clear;            // --gripper: with --top-k, the candidates' clearance against the (first) frame
    std::string out_prefix, mask_path, roi_path, labels_path;
    int min_vote = 1;
    bool filter = false;
    haf_depth_filter filter_params;
    std::string filtered_out;
    // --segment: the first view is clustered into objects (haf_segment_frame, a uint8 image: at most 255 objects) after the filter and
    // before the request; without --labels its image feeds the "object" lines; --segment-roi scores under labels != 0; --plane: the
    // support plane (default: through --center with the approach vector as its normal); --labels-out: the image as an 8-bit PGM
    bool segment = false, segment_roi = false, have_plane = false;
    haf_segment_params segment_params;
    float plane[4] = {0, 0, 1, 0};
    // --plane fit[,TOL,N_HYP]: the plane is haf_fit_plane's of the first view; --plane-mask: the haf_roi of that fit
    bool fit_plane = false;
    haf_plane_params plane_params;
    std::string plane_mask;
    std::string labels_out;
    std::vector<uint8_t> seg_labels;     // filled by run_depth
    int32_t seg_n = 0;
    float seg_plane[4] = {0, 0, 1, 0};   // the plane the segmentation ran over (filled by run_depth)
    // --per-object [MARGIN]: a request per segmented object; --measure: the shapes of --labels, no request
    bool per_object = false, measure = false;
    bool fused = false;                  // --per-object --fused: one haf_score_objects call per chunk
    int margin_cells = 4;
    // --segment-cells: the segmenter is haf_segment_cells (connected cells of the top-down grid) instead of haf_segment_frame; everything
    // behind the label image is the same.  It also takes ONE .pcd in place of --depth: the cloud as an N x 1 XYZ frame under the
    // identity pose.  --cell-labels-out: the top-down label grid as an 8-bit PGM, nx x ny
    bool cells = false;
    haf_cell_segment_params cell_params;
    std::string cell_labels_out;
    // --labels-camera FX FY CX CY [--labels-pose 12 floats] [--transfer NEAR,TOL_ABS,TOL_REL,SPLAT]: --labels is ANOTHER camera's image (any
    // size); haf_transfer_labels carries it over to the first view before --measure, --per-object --fused or the plain --labels pick
    // read it, and --labels-out writes the transferred image
    bool labels_camera = false;
    haf_camera camera;
    float labels_pose[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    haf_transfer_params transfer_params;
    std::vector<uint8_t> xfer8;          // the transferred image (filled by run_depth): uint8 up to 255 labels, uint16 above
    std::vector<uint16_t> xfer16;
    int32_t xfer_n = 0;
};

// --transfer NEAR,TOL_ABS,TOL_REL,SPLAT
static bool parse_transfer(const char *arg, haf_transfer_params *p)
{
    float a = 0, b = 0, c = 0;
    int s = 0;
    char tail = 0;
    if (sscanf(arg, "%f,%f,%f,%d%c", &a, &b, &c, &s, &tail) != 4) return false;
    p->near_m = a; p->tol_abs = b; p->tol_rel = c; p->splat = s;
    return true;
}

// --segment MIN_H,MAX_H,GAP,MIN_PX or "default"
static bool parse_segment(const char *arg, haf_segment_params *p)
{
    haf_segment_default(p);
    if (strcmp(arg, "default") == 0) return true;
    float min_h = 0, max_h = 0, gap = 0;
    int min_px = 0;
    char tail = 0;
    if (sscanf(arg, "%f,%f,%f,%d%c", &min_h, &max_h, &gap, &min_px, &tail) != 4) return false;
    p->min_height = min_h; p->max_height = max_h; p->max_gap = gap; p->min_pixels = min_px;
    return true;
}

// --segment-cells MIN_H,MAX_H,CELL,MIN_PTS[,STEP] or "default"
static bool parse_segment_cells(const char *arg, haf_cell_segment_params *p)
{
    haf_cell_segment_default(p);
    if (strcmp(arg, "default") == 0) return true;
    float min_h = 0, max_h = 0, cell = 0, step = 0;
    int min_pts = 0;
    char tail = 0;
    int commas = 0;
    for (const char *c = arg; *c; c++) commas += *c == ',';
    const int got = sscanf(arg, "%f,%f,%f,%d,%f%c", &min_h, &max_h, &cell, &min_pts, &step, &tail);
    if ((got != 4 && got != 5) || commas != got - 1) return false;      // ("0.03,0,0.01,50," or "...,50,x")
    p->min_height = min_h; p->max_height = max_h; p->cell = cell; p->min_points = min_pts;
    if (got == 5) p->max_step = step;
    return true;
}

// --plane fit[,TOL[,N_HYP]]
static bool parse_plane_fit(const char *arg, haf_plane_params *p)
{
    haf_plane_default(p);
    if (strcmp(arg, "fit") == 0) return true;
    float tol = 0;
    int n_hyp = 0;
    char tail = 0;
    const int got = sscanf(arg, "fit,%f,%d%c", &tol, &n_hyp, &tail);
    if (got != 1 && got != 2) return false;
    if (got == 1 && strchr(arg + 4, ',')) return false;   // ("fit,0.005," or "fit,0.005,x")
    p->tol = tol;
    if (got == 2) p->n_hyp = n_hyp;
    return true;
}

static bool write_pgm8(const std::string &path, const uint8_t *img, int w, int h)
{
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) return false;
    fprintf(fp, "P5\n%d %d\n255\n", w, h);
    const size_t n = (size_t)w * (size_t)h;
    const bool ok = fwrite(img, 1, n, fp) == n;
    return fclose(fp) == 0 && ok;
}

// --depth-filter RADIUS,SUPPORT,TOL_ABS,TOL_REL[,MIN_VALID] or "default"
static bool parse_depth_filter(const char *arg, haf_depth_filter *p)
{
    haf_depth_filter_default(p);
    if (strcmp(arg, "default") == 0) return true;
    int radius = 0, support = 0, min_valid = 1;
    float tol_abs = 0, tol_rel = 0;
    char tail = 0;
    const int n = sscanf(arg, "%d,%d,%f,%f,%d%c", &radius, &support, &tol_abs, &tol_rel, &min_valid, &tail);
    if (n != 4 && n != 5) return false;
    p->radius = radius; p->min_support = support; p->tol_abs = tol_abs; p->tol_rel = tol_rel; p->min_valid = n == 5 ? min_valid : 1;
    return true;
}

// a depth image as a 16-bit binary PGM, samples as they are
static bool write_depth_pgm16(const std::string &path, const uint16_t *img, int w, int h)
{
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) return false;
    fprintf(fp, "P5\n%d %d\n65535\n", w, h);
    std::vector<unsigned char> row((size_t)w * 2);
    bool ok = true;
    for (int v = 0; v < h && ok; v++) {
        for (int u = 0; u < w; u++) {
            const unsigned x = img[(size_t)v * w + u];
            row[2 * (size_t)u] = (unsigned char)(x >> 8);
            row[2 * (size_t)u + 1] = (unsigned char)(x & 255u);
        }
        ok = fwrite(row.data(), 1, row.size(), fp) == row.size();
    }
    return fclose(fp) == 0 && ok;
}

static bool write_pgm16(const std::string &path, const int16_t *img, int w, int h)
{
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) return false;
    fprintf(fp, "P5\n%d %d\n65535\n", w, h);
    std::vector<unsigned char> row((size_t)w * 2);
    bool ok = true;
    for (int v = 0; v < h && ok; v++) {
        for (int u = 0; u < w; u++) {
            const unsigned x = (unsigned)((int)img[(size_t)v * w + u] + 32768);
            row[2 * (size_t)u] = (unsigned char)(x >> 8);
            row[2 * (size_t)u + 1] = (unsigned char)(x & 255u);
        }
        ok = fwrite(row.data(), 1, row.size(), fp) == row.size();
    }
    return fclose(fp) == 0 && ok;
}

// binary PGM with 8-bit samples (maxval <= 255), '#' comments in the header
static bool read_pgm8(const std::string &path, std::vector<uint8_t> &img, int &w, int &h)
{
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) return false;
    auto token = [&](long &val) {
        int c = fgetc(fp);
        for (;;) {
            while (c == ' ' || c == '\t' || c == '\n' || c == '\r') c = fgetc(fp);
            if (c != '#') break;
            while (c != '\n' && c != EOF) c = fgetc(fp);
        }
        if (c < '0' || c > '9') return false;
        val = 0;
        while (c >= '0' && c <= '9' && val < (1L << 30)) { val = val * 10 + (c - '0'); c = fgetc(fp); }
        return c == ' ' || c == '\t' || c == '\n' || c == '\r';
    };
    long W = 0, H = 0, maxval = 0;
    bool ok = fgetc(fp) == 'P' && fgetc(fp) == '5' && token(W) && token(H) && token(maxval) && W >= 1 && H >= 1 && maxval >= 1 && maxval <= 255 &&
              W * H <= (1L << 30);
    if (ok) {
        img.resize((size_t)(W * H));
        ok = fread(img.data(), 1, img.size(), fp) == img.size();
        w = (int)W; h = (int)H;
    }
    fclose(fp);
    return ok;
}

static int run_map(haf_engine *eng, const haf_config &cfg, const haf_frame &f, const MapOptions &mo)
{
    const size_t n = (size_t)f.width * (size_t)f.height;
    if (mo.labels_path.empty() && mo.segment && mo.seg_n > 0) {      // --segment without --labels: the objects are the segmentation's
        const haf_label_image img = {mo.seg_labels.data(), 1, 0, (size_t)f.width};
        std::vector<std::string> lines;
        std::string serr;
        if (hafshim::label_hypotheses(eng, cfg, f, img, mo.seg_n, mo.min_vote, &lines, &serr) != HAF_OK) {
            fprintf(stderr, "--segment: %s\n", serr.c_str());
            return 1;
        }
        for (const std::string &l : lines) printf("object %s\n", l.c_str());
    }
    if (!mo.out_prefix.empty()) {
        std::vector<int16_t> vote(n), roll(n);
        if (haf_grasp_map(eng, 0, &f, vote.data(), roll.data(), nullptr, 0) != HAF_OK) { fprintf(stderr, "--map-out: %s\n", haf_last_error(eng)); return 1; }
        if (!write_pgm16(mo.out_prefix + ".vote.pgm", vote.data(), f.width, f.height) || !write_pgm16(mo.out_prefix + ".roll.pgm", roll.data(), f.width, f.height)) {
            fprintf(stderr, "--map-out: cannot write %s.vote.pgm / .roll.pgm\n", mo.out_prefix.c_str());
            return 1;
        }
    }
    if (!mo.mask_path.empty()) {
        std::vector<uint8_t> mask;
        int w = 0, h = 0;
        if (!read_pgm8(mo.mask_path, mask, w, h)) { fprintf(stderr, "%s: not a binary 8-bit PGM\n", mo.mask_path.c_str()); return 1; }
        if (w != f.width || h != f.height) { fprintf(stderr, "%s: %d x %d, the depth image has %d x %d\n", mo.mask_path.c_str(), w, h, f.width, f.height); return 1; }
        haf_grasp_candidate best;
        int32_t u = -1, v = -1, found = 0;
        if (haf_grasp_map_best(eng, 0, &f, mask.data(), (size_t)w, mo.min_vote, &best, &u, &v, &found) != HAF_OK) {
            fprintf(stderr, "--mask: %s\n", haf_last_error(eng));
            return 1;
        }
        if (found) printf("mask %d %d %s\n", u, v, hafshim::hypothesis_string(best.grasp, cfg.roll_step_deg).c_str());
        else printf("mask none\n");
    }
    if (mo.labels_camera) {                               // --labels through --labels-camera: the transferred image, already on this frame
        const bool wide = !mo.xfer16.empty();
        const haf_label_image img = {wide ? (const void *)mo.xfer16.data() : (const void *)mo.xfer8.data(), wide ? 2 : 1, 0, (size_t)f.width * (wide ? 2 : 1)};
        std::vector<std::string> lines;
        std::string serr;
        if (hafshim::label_hypotheses(eng, cfg, f, img, mo.xfer_n, mo.min_vote, &lines, &serr) != HAF_OK) {
            fprintf(stderr, "--labels: %s\n", serr.c_str());
            return 1;
        }
        for (const std::string &l : lines) printf("object %s\n", l.c_str());
    } else if (!mo.labels_path.empty()) {
        // 8-bit samples as they are, 16-bit ones through the library's reader; labels above HAF_MAX_LABELS are ignored like background
        std::vector<uint8_t> lab8;
        uint16_t *lab16 = nullptr;
        int32_t w = 0, h = 0;
        char err[256];
        int w8 = 0, h8 = 0;
        if (read_pgm8(mo.labels_path, lab8, w8, h8)) { w = w8; h = h8; }
        else if (haf_pgm16_load(mo.labels_path.c_str(), &lab16, &w, &h, err, sizeof err) != HAF_OK) {
            fprintf(stderr, "%s: not a binary 8- or 16-bit PGM (%s)\n", mo.labels_path.c_str(), err);
            return 1;
        }
        int rc = 0;
        if (w != f.width || h != f.height) {
            fprintf(stderr, "%s: %d x %d, the depth image has %d x %d\n", mo.labels_path.c_str(), w, h, f.width, f.height);
            rc = 1;
        } else {
            unsigned top = 0;
            for (size_t i = 0; i < n; i++) top = std::max(top, lab16 ? (unsigned)lab16[i] : (unsigned)lab8[i]);
            const haf_label_image img = {lab16 ? (const void *)lab16 : (const void *)lab8.data(), lab16 ? 2 : 1, 0, (size_t)w * (lab16 ? 2 : 1)};
            std::vector<std::string> lines;
            std::string serr;
            if (top > 0 && hafshim::label_hypotheses(eng, cfg, f, img, (int32_t)std::min(top, (unsigned)HAF_MAX_LABELS), mo.min_vote, &lines, &serr) != HAF_OK) {
                fprintf(stderr, "--labels: %s\n", serr.c_str());
                rc = 1;
            }
            for (const std::string &l : lines) printf("object %s\n", l.c_str());
        }
        if (lab16) haf_free(lab16);
        if (rc) return rc;
    }
    return 0;
}

// an 8- or 16-bit binary PGM of w x h label samples -> the image as the library reads it; *lab16 is the caller's to haf_free
static bool load_labels(const std::string &path, int w, int h, std::vector<uint8_t> &lab8, uint16_t **lab16, haf_label_image *img, unsigned *top)
{
    int w8 = 0, h8 = 0;
    int32_t w16 = 0, h16 = 0;
    char err[256];
    *lab16 = nullptr;
    if (read_pgm8(path, lab8, w8, h8)) { w16 = w8; h16 = h8; }
    else if (haf_pgm16_load(path.c_str(), lab16, &w16, &h16, err, sizeof err) != HAF_OK) {
        fprintf(stderr, "%s: not a binary 8- or 16-bit PGM (%s)\n", path.c_str(), err);
        return false;
    }
    if (w16 != w || h16 != h) { fprintf(stderr, "%s: %d x %d, the depth image has %d x %d\n", path.c_str(), (int)w16, (int)h16, w, h); return false; }
    *top = 0;
    for (size_t i = 0; i < (size_t)w * (size_t)h; i++) *top = std::max(*top, *lab16 ? (unsigned)(*lab16)[i] : (unsigned)lab8[i]);
    *img = haf_label_image{*lab16 ? (const void *)*lab16 : (const void *)lab8.data(), *lab16 ? 2 : 1, 0, (size_t)w * (*lab16 ? 2 : 1)};
    return true;
}

// --labels FILE.pgm --measure: the shapes of the label image over the frame, no request
static int run_measure(haf_engine *eng, const haf_frame &f, const MapOptions &mo)
{
    std::vector<uint8_t> lab8;
    uint16_t *lab16 = nullptr;
    haf_label_image img;
    unsigned top = 0;
    if (mo.labels_camera) {                               // the transferred image, already on this frame
        const bool wide = !mo.xfer16.empty();
        img = haf_label_image{wide ? (const void *)mo.xfer16.data() : (const void *)mo.xfer8.data(), wide ? 2 : 1, 0, (size_t)f.width * (wide ? 2 : 1)};
        top = (unsigned)mo.xfer_n;
    } else if (!load_labels(mo.labels_path, f.width, f.height, lab8, &lab16, &img, &top)) { if (lab16) haf_free(lab16); return 1; }
    const int32_t n = (int32_t)std::min(std::max(top, 1u), (unsigned)HAF_MAX_LABELS);
    std::vector<haf_label_shape> shapes((size_t)n);
    const int rc = haf_measure_labels(eng, &f, &img, n, mo.have_plane ? mo.plane : nullptr, shapes.data());
    if (lab16) haf_free(lab16);
    if (rc != HAF_OK) { fprintf(stderr, "--measure: %s\n", haf_last_error(eng)); return 1; }
    for (int32_t l = 0; l < n; l++) {
        const haf_label_shape &s = shapes[(size_t)l];
        printf("shape %d found %d pixels %d points %d centroid %.9g %.9g %.9g box %.9g %.9g %.9g %.9g %.9g %.9g width %.9g long %.9g yaw %d diameter %.9g height %.9g\n",
               (int)l + 1, (int)s.found, (int)s.n_pixels, (int)s.n_points, s.centroid[0], s.centroid[1], s.centroid[2], s.box_min[0], s.box_min[1],
               s.box_min[2], s.box_max[0], s.box_max[1], s.box_max[2], s.narrow_width, s.long_width, (int)s.narrow_dir * 15, s.diameter, s.height);
    }
    return 0;
}

// --segment ... --per-object: one request per object of the segmentation (mo.seg_labels, mo.seg_n, mo.seg_plane), each centred on its
// object, in chunks of cfg.max_clouds requests that share the frame and the label image as their mask
static int run_per_object(haf_engine *eng, const haf_config &cfg, const haf_grasp_input &in, const haf_frame &f, const MapOptions &mo)
{
    if (mo.seg_n < 1) return 0;
    const size_t n = (size_t)mo.seg_n;
    const haf_label_image img = {mo.seg_labels.data(), 1, 0, (size_t)f.width};
    std::vector<haf_label_shape> shapes(n);
    if (haf_measure_labels(eng, &f, &img, mo.seg_n, mo.seg_plane, shapes.data()) != HAF_OK) { fprintf(stderr, "--per-object: %s\n", haf_last_error(eng)); return 1; }
    struct Todo { int32_t label; haf_grasp_input in; int32_t fits; };
    std::vector<Todo> todo;
    for (size_t l = 0; l < n; l++) {
        Todo t;
        t.label = (int32_t)l + 1;
        if (shapes[l].found && haf_object_input(&cfg, &in, &shapes[l], mo.margin_cells, &t.in, &t.fits) == HAF_OK) todo.push_back(t);
    }
    const size_t px = (size_t)f.width * (size_t)f.height;
    // (--fused: the frame counts once against max_points whatever the chunk holds)
    const size_t chunk = mo.fused ? std::max<size_t>(1, (size_t)cfg.max_clouds)
                                  : std::max<size_t>(1, std::min<size_t>((size_t)cfg.max_clouds, (size_t)cfg.max_points / std::max<size_t>(1, px)));
    struct Hit { unsigned long long key; std::string line; };
    std::vector<Hit> hits;
    std::vector<haf_label_pick> picks(n);
    std::vector<haf_grasp_candidate> poses(n);
    const auto add_hit = [&](int32_t label, const haf_label_pick &p, const haf_grasp_candidate &pose) {
        const size_t l = (size_t)label - 1;
        const unsigned i = (unsigned)((size_t)p.v * (size_t)f.width + (size_t)p.u);      // haf_grasp_map_labels' key: vote, then roll, then pixel
        const unsigned long long key = ((unsigned long long)(unsigned)(p.vote + 32768) << 48) | ((unsigned long long)(unsigned)(65535 - p.roll) << 32) |
                                       (unsigned long long)(0xFFFFFFFFu - i);
        char tail[128];
        snprintf(tail, sizeof tail, " width %.9g yaw %d height %.9g", shapes[l].narrow_width, (int)shapes[l].narrow_dir * 15, shapes[l].height);
        hits.push_back(Hit{key, "object " + std::to_string(label) + " " + std::to_string(p.u) + " " + std::to_string(p.v) + " " +
                                    hafshim::hypothesis_string(pose.grasp, cfg.roll_step_deg) + tail});
    };
    for (size_t c0 = 0; c0 < todo.size(); c0 += chunk) {
        const size_t k = std::min(chunk, todo.size() - c0);
        if (mo.fused) {                                   // ONE call: every object of the chunk a request of its own on the shared frame
            std::vector<int32_t> object_labels(k);
            std::vector<haf_grasp_input> ins(k);
            std::vector<haf_grasp_output> outs(k);
            for (size_t b = 0; b < k; b++) { object_labels[b] = todo[c0 + b].label; ins[b] = todo[c0 + b].in; }
            if (haf_score_objects(eng, &f, &img, mo.seg_n, (int32_t)k, object_labels.data(), ins.data(), mo.min_vote, outs.data(), picks.data(),
                                  poses.data(), nullptr, nullptr) != HAF_OK) {
                fprintf(stderr, "--per-object --fused: %s\n", haf_last_error(eng));
                return 1;
            }
            for (size_t b = 0; b < k; b++)
                if (picks[b].found) add_hit(object_labels[b], picks[b], poses[b]);
            continue;
        }
        std::vector<haf_frame> frames(k, f);
        std::vector<haf_roi> rois(k, haf_roi{mo.seg_labels.data(), (size_t)f.width, 0});
        std::vector<haf_grasp_input> ins(k);
        std::vector<haf_grasp_output> outs(k);
        for (size_t b = 0; b < k; b++) ins[b] = todo[c0 + b].in;
        if (haf_score_frames_roi(eng, (int32_t)k, frames.data(), rois.data(), ins.data(), outs.data()) != HAF_OK) {
            fprintf(stderr, "--per-object: %s\n", haf_last_error(eng));
            return 1;
        }
        for (size_t b = 0; b < k; b++) {
            if (haf_grasp_map_labels(eng, (int32_t)b, &f, &img, mo.seg_n, mo.min_vote, picks.data(), poses.data(), nullptr, nullptr) != HAF_OK) {
                fprintf(stderr, "--per-object: %s\n", haf_last_error(eng));
                return 1;
            }
            const size_t l = (size_t)todo[c0 + b].label - 1;
            if (picks[l].found) add_hit(todo[c0 + b].label, picks[l], poses[l]);
        }
    }
    std::sort(hits.begin(), hits.end(), [](const Hit &a, const Hit &b) { return a.key > b.key; });
    for (const Hit &h : hits) printf("%s\n", h.line.c_str());
    return 0;
}

static int run_depth(haf_engine *eng, const haf_config &cfg, const haf_grasp_input &in, const std::vector<DepthView> &views,
                     bool hypotheses, int top_k, int top_radius, int top_rolls, double top_dist, MapOptions &mo)
{
    std::vector<uint16_t *> images;
    std::vector<haf_frame> frames;
    auto release = [&]() { for (uint16_t *p : images) haf_free(p); };
    char err[256];
    for (const DepthView &v : views) {
        haf_frame f = v.frame;
        if (f.kind == HAF_FRAME_XYZ_F32 && f.data) {       // --segment-cells with a .pcd: the cloud as main() wrapped it, its points main()'s
            images.push_back(nullptr);
            frames.push_back(f);
            continue;
        }
        uint16_t *depth = nullptr;
        if (haf_pgm16_load(v.path.c_str(), &depth, &f.width, &f.height, err, sizeof err) != HAF_OK) { fprintf(stderr, "%s: %s\n", v.path.c_str(), err); release(); return 1; }
        images.push_back(depth);
        f.kind = HAF_FRAME_DEPTH_U16;
        f.data = depth;
        f.row_stride_bytes = (size_t)f.width * 2;
        frames.push_back(f);
    }
    // --depth-filter: the exposures of every view -> one image that takes the view's place (haf_filter_depth, into host memory: every
    // view keeps its own image until the request is scored)
    for (size_t v = 0; mo.filter && v < views.size(); v++) {
        std::vector<uint16_t *> extra;
        std::vector<haf_frame> stack(1, frames[v]);
        int bad = 0;
        for (const std::string &sp : views[v].stack) {
            haf_frame f = frames[v];
            uint16_t *depth = nullptr;
            if (haf_pgm16_load(sp.c_str(), &depth, &f.width, &f.height, err, sizeof err) != HAF_OK) { fprintf(stderr, "%s: %s\n", sp.c_str(), err); bad = 1; break; }
            extra.push_back(depth);
            f.data = depth;
            f.row_stride_bytes = (size_t)f.width * 2;
            stack.push_back(f);
        }
        uint16_t *filtered = bad ? nullptr : (uint16_t *)malloc(std::max<size_t>(1, (size_t)frames[v].width * (size_t)frames[v].height) * 2);
        int64_t stats[3] = {0, 0, 0};
        if (!bad && (!filtered || stack.size() > (size_t)HAF_MAX_STACK ||
                     haf_filter_depth(eng, stack.data(), (int32_t)stack.size(), &mo.filter_params, filtered, (size_t)frames[v].width * 2, 0, nullptr, stats) != HAF_OK)) {
            fprintf(stderr, "%s: --depth-filter: %s\n", views[v].path.c_str(),
                    !filtered ? "out of host memory" : stack.size() > (size_t)HAF_MAX_STACK ? "more than HAF_MAX_STACK exposures" : haf_last_error(eng));
            bad = 1;
        }
        for (uint16_t *p : extra) haf_free(p);
        if (bad) { free(filtered); release(); return 1; }
        haf_free(images[v]);
        images[v] = filtered;                              // (haf_free is free)
        frames[v].data = filtered;
        fprintf(stderr, "%s: %d exposure(s) filtered: %lld of %lld pixels valid, %lld kept\n", views[v].path.c_str(), (int)stack.size(),
                (long long)stats[1], (long long)stats[0], (long long)stats[2]);
    }
    if (mo.filter && !mo.filtered_out.empty() && !write_depth_pgm16(mo.filtered_out, images[0], frames[0].width, frames[0].height)) {
        fprintf(stderr, "--filtered-out: cannot write %s\n", mo.filtered_out.c_str());
        release();
        return 1;
    }
    // --labels-camera: the other camera's label image onto the first view (filtered or not), before anything reads labels
    if (mo.labels_camera) {
        std::vector<uint8_t> lab8;
        uint16_t *lab16 = nullptr;
        int w8 = 0, h8 = 0;
        int32_t wc = 0, hc = 0;
        if (read_pgm8(mo.labels_path, lab8, w8, h8)) { wc = w8; hc = h8; }
        else if (haf_pgm16_load(mo.labels_path.c_str(), &lab16, &wc, &hc, err, sizeof err) != HAF_OK) {
            fprintf(stderr, "%s: not a binary 8- or 16-bit PGM (%s)\n", mo.labels_path.c_str(), err);
            release();
            return 1;
        }
        unsigned top = 0;
        for (size_t i = 0; i < (size_t)wc * (size_t)hc; i++) top = std::max(top, lab16 ? (unsigned)lab16[i] : (unsigned)lab8[i]);
        mo.xfer_n = (int32_t)std::min(std::max(top, 1u), (unsigned)HAF_MAX_LABELS);
        const bool wide = mo.xfer_n > 255;
        const size_t px = (size_t)frames[0].width * (size_t)frames[0].height;
        if (wide) mo.xfer16.assign(px, 0); else mo.xfer8.assign(px, 0);
        haf_camera cam = mo.camera;
        cam.width = wc; cam.height = hc;
        const haf_label_image cl = {lab16 ? (const void *)lab16 : (const void *)lab8.data(), lab16 ? 2 : 1, 0, (size_t)wc * (lab16 ? 2 : 1)};
        int64_t ts[5] = {0, 0, 0, 0, 0};
        int trc = haf_invert_pose(mo.labels_pose, cam.base_to_camera);
        if (trc != HAF_OK) fprintf(stderr, "--labels-pose: not finite, or singular\n");
        else if ((trc = haf_transfer_labels(eng, &frames[0], &cam, &cl, mo.xfer_n, &mo.transfer_params, wide ? (void *)mo.xfer16.data() : (void *)mo.xfer8.data(),
                                            wide ? 2 : 1, (size_t)frames[0].width * (wide ? 2 : 1), 0, nullptr, nullptr, ts)) != HAF_OK)
            fprintf(stderr, "%s: --labels-camera: %s\n", mo.labels_path.c_str(), haf_last_error(eng));
        if (lab16) haf_free(lab16);
        if (trc != HAF_OK) { release(); return 1; }
        fprintf(stderr, "%s: %d x %d labels transferred: %lld of %lld pixels in front of the camera, %lld project, %lld visible, %lld labelled\n",
                mo.labels_path.c_str(), (int)wc, (int)hc, (long long)ts[1], (long long)ts[0], (long long)ts[2], (long long)ts[3], (long long)ts[4]);
        if (!mo.labels_out.empty() && !(wide ? write_depth_pgm16(mo.labels_out, mo.xfer16.data(), frames[0].width, frames[0].height)
                                             : write_pgm8(mo.labels_out, mo.xfer8.data(), frames[0].width, frames[0].height))) {
            fprintf(stderr, "--labels-out: cannot write %s\n", mo.labels_out.c_str());
            release();
            return 1;
        }
        if (mo.per_object) {                              // the objects of --per-object --fused are the transferred image's
            if (wide) { fprintf(stderr, "--per-object: more than 255 labels\n"); release(); return 1; }
            mo.seg_labels = mo.xfer8;
            mo.seg_n = mo.xfer_n;
            if (mo.have_plane) memcpy(mo.seg_plane, mo.plane, sizeof mo.seg_plane);
            else {
                hafshim::GoalFields g;
                haf_segment_params from_goal;
                for (int k = 0; k < 3; k++) { g.center[k] = in.grasp_area_center[k]; g.approach_vector[k] = in.approach_vector[k]; }
                hafshim::segment_params_from_goal(g, &from_goal);
                memcpy(mo.seg_plane, from_goal.plane, sizeof mo.seg_plane);
            }
        }
    }
    if (mo.measure) {
        const int mrc = run_measure(eng, frames[0], mo);
        release();
        return mrc;
    }
    // --segment: the first view (filtered or not) into a label image, before the request: the call needs no scored batch
    if (mo.segment) {
        haf_segment_params sp = mo.segment_params;
        if (mo.have_plane) memcpy(sp.plane, mo.plane, sizeof sp.plane);
        else {                                             // (also the fall-back of --plane fit)
            hafshim::GoalFields g;
            haf_segment_params from_goal;
            for (int k = 0; k < 3; k++) { g.center[k] = in.grasp_area_center[k]; g.approach_vector[k] = in.approach_vector[k]; }
            hafshim::segment_params_from_goal(g, &from_goal);
            memcpy(sp.plane, from_goal.plane, sizeof sp.plane);
        }
        if (mo.fit_plane) {
            std::vector<uint8_t> pm;
            haf_roi roi = {nullptr, 0, 0};
            if (!mo.plane_mask.empty()) {
                int w = 0, h = 0;
                if (!read_pgm8(mo.plane_mask, pm, w, h)) { fprintf(stderr, "%s: not a binary 8-bit PGM\n", mo.plane_mask.c_str()); release(); return 1; }
                if (w != frames[0].width || h != frames[0].height) { fprintf(stderr, "%s: %d x %d, the depth image is %d x %d\n", mo.plane_mask.c_str(), w, h, frames[0].width, frames[0].height); release(); return 1; }
                roi.mask = pm.data(); roi.row_stride_bytes = (size_t)w;
            }
            haf_plane_result fit;
            if (haf_fit_plane(eng, &frames[0], roi.mask ? &roi : nullptr, &mo.plane_params, &fit, nullptr, nullptr) != HAF_OK) {
                fprintf(stderr, "%s: --plane fit: %s\n", views[0].path.c_str(), haf_last_error(eng));
                release();
                return 1;
            }
            if (fit.found) {
                memcpy(sp.plane, fit.plane, sizeof sp.plane);
                printf("plane %.9g %.9g %.9g %.9g inliers %d rms %.6g\n", fit.plane[0], fit.plane[1], fit.plane[2], fit.plane[3], (int)fit.n_inliers, fit.rms);
            } else printf("plane none\n");
        }
        memcpy(mo.seg_plane, sp.plane, sizeof mo.seg_plane);
        mo.seg_labels.assign((size_t)frames[0].width * (size_t)frames[0].height, 0);
        int64_t stats[4] = {0, 0, 0, 0};
        if (mo.cells) {
            haf_cell_segment_params cp = mo.cell_params;
            memcpy(cp.plane, sp.plane, sizeof cp.plane);
            std::vector<uint16_t> grid(mo.cell_labels_out.empty() ? 0 : (size_t)std::max(cp.nx, 0) * (size_t)std::max(cp.ny, 0));
            int64_t cs[6] = {0, 0, 0, 0, 0, 0};
            if (haf_segment_cells(eng, &frames[0], &cp, mo.seg_labels.data(), 1, (size_t)frames[0].width, 0, nullptr, grid.empty() ? nullptr : grid.data(),
                                  nullptr, &mo.seg_n, cs) != HAF_OK) {
                fprintf(stderr, "%s: --segment-cells: %s\n", views[0].path.c_str(), haf_last_error(eng));
                release();
                return 1;
            }
            fprintf(stderr, "%s: segmented by cells: %d object(s); %lld of %lld points foreground, %lld outside the grid, %lld cell(s), %lld component(s), %lld pass the size rule\n",
                    views[0].path.c_str(), (int)mo.seg_n, (long long)cs[1], (long long)cs[0], (long long)cs[2], (long long)cs[3], (long long)cs[4], (long long)cs[5]);
            std::vector<uint8_t> grid8(grid.begin(), grid.end());      // (a uint8 label image: at most 255 labels)
            if (!grid.empty() && !write_pgm8(mo.cell_labels_out, grid8.data(), cp.nx, cp.ny)) {
                fprintf(stderr, "--cell-labels-out: cannot write %s\n", mo.cell_labels_out.c_str());
                release();
                return 1;
            }
        } else if (haf_segment_frame(eng, &frames[0], &sp, mo.seg_labels.data(), 1, (size_t)frames[0].width, 0, nullptr, nullptr, &mo.seg_n, stats) != HAF_OK) {
            fprintf(stderr, "%s: --segment: %s\n", views[0].path.c_str(), haf_last_error(eng));
            release();
            return 1;
        }
        if (!mo.cells)
            fprintf(stderr, "%s: segmented: %d object(s); %lld of %lld pixels foreground, %lld component(s), %lld pass the size rule\n", views[0].path.c_str(),
                    (int)mo.seg_n, (long long)stats[1], (long long)stats[0], (long long)stats[2], (long long)stats[3]);
        if (!mo.labels_out.empty() && !write_pgm8(mo.labels_out, mo.seg_labels.data(), frames[0].width, frames[0].height)) {
            fprintf(stderr, "--labels-out: cannot write %s\n", mo.labels_out.c_str());
            release();
            return 1;
        }
    }
    if (mo.per_object) {
        const int prc = run_per_object(eng, cfg, in, frames[0], mo);
        release();
        return prc;
    }
    // what the messages below are about: the file of a single view; every file of a fused request ("a.pgm + b.pgm"), in view order, so
    // that the library's "request 0 view V" finds its file
    std::string path = views[0].path;
    for (size_t v = 1; v < views.size(); v++) path += " + " + views[v].path;
    long long pixels = 0;
    for (const haf_frame &f : frames) pixels += (long long)f.width * f.height;
    int rc = 0;
    haf_grasp_output out;
    const int32_t n_views = (int32_t)frames.size();
    int64_t n_points = 0;
    std::vector<uint8_t> roi_mask;
    if (!mo.roi_path.empty()) {
        int w = 0, h = 0;
        if (!read_pgm8(mo.roi_path, roi_mask, w, h)) { fprintf(stderr, "%s: not a binary 8-bit PGM\n", mo.roi_path.c_str()); release(); return 1; }
        if (w != frames[0].width || h != frames[0].height) {
            fprintf(stderr, "%s: %d x %d, the depth image has %d x %d\n", mo.roi_path.c_str(), w, h, frames[0].width, frames[0].height);
            release();
            return 1;
        }
    }
    const bool seg_roi = mo.segment && mo.segment_roi;      // (labels != 0 selects: the uint8 label image IS the mask)
    const haf_roi roi = {seg_roi ? mo.seg_labels.data() : roi_mask.data(), (size_t)frames[0].width, 0};
    // --view-roi-mask: a mask per view, null for a view without one
    std::vector<std::vector<uint8_t>> view_masks(views.size());
    std::vector<haf_roi> view_rois(views.size(), haf_roi{nullptr, 0, 0});
    bool view_roi = false;
    for (size_t v = 0; v < views.size(); v++) {
        if (views[v].roi_path.empty()) continue;
        int w = 0, h = 0;
        if (!read_pgm8(views[v].roi_path, view_masks[v], w, h)) { fprintf(stderr, "%s: not a binary 8-bit PGM\n", views[v].roi_path.c_str()); release(); return 1; }
        if (w != frames[v].width || h != frames[v].height) {
            fprintf(stderr, "%s: %d x %d, the depth image %s has %d x %d\n", views[v].roi_path.c_str(), w, h, views[v].path.c_str(), frames[v].width, frames[v].height);
            release();
            return 1;
        }
        view_rois[v] = haf_roi{view_masks[v].data(), (size_t)w, 0};
        view_roi = true;
    }
    if ((!mo.roi_path.empty() || seg_roi ? haf_score_frames_roi(eng, 1, frames.data(), &roi, &in, &out)
         : view_roi ? haf_score_views_roi(eng, 1, &n_views, frames.data(), view_rois.data(), &in, &out, &n_points)
         : n_views == 1 ? haf_score_frames(eng, 1, frames.data(), &in, &out)
                        : haf_score_views(eng, 1, &n_views, frames.data(), &in, &out, &n_points)) != HAF_OK) {
        fprintf(stderr, "%s: %s\n", path.c_str(), haf_last_error(eng));
        release();
        return 1;
    }
    if (hypotheses && !in.show_only_best_grasp) {
        haf_top_params tp;
        haf_top_params_default(eng, &tp);
        tp.k = std::min(cfg.n_rolls, 1024);
        tp.min_vote = cfg.graspval_th + 1;
        tp.cell_radius = cfg.grid_h;
        tp.roll_window = 0;
        std::vector<haf_grasp_candidate> cand((size_t)tp.k);
        int32_t n = 0;
        if (cfg.n_rolls > 1024 || haf_top_grasps(eng, &tp, cand.data(), &n) != HAF_OK) {
            fprintf(stderr, "%s: --hypotheses: %s\n", path.c_str(), cfg.n_rolls > 1024 ? "more than 1024 rolls" : haf_last_error(eng));
            rc = 1;
            n = 0;
        }
        std::sort(cand.begin(), cand.begin() + n, [](const haf_grasp_candidate &a, const haf_grasp_candidate &b) { return a.grasp.best_roll < b.grasp.best_roll; });
        for (int32_t i = 0; i < n; i++)
            if (cand[(size_t)i].grasp.best_roll < out.rolls_done) printf("hypothesis %s\n", hafshim::hypothesis_string(cand[(size_t)i].grasp, cfg.roll_step_deg).c_str());
    }
    printf("%s\n", hafshim::hypothesis_string(out, cfg.roll_step_deg).c_str());
    if (top_k > 0) print_top(eng, cfg, path.c_str(), top_k, top_radius, top_rolls, top_dist, &rc, &mo.clear, &frames[0], n_views);
    if (run_map(eng, cfg, frames[0], mo) != 0) rc = 1;
    char size[96];
    if (n_views == 1) snprintf(size, sizeof size, "%d x %d pixels", frames[0].width, frames[0].height);
    else snprintf(size, sizeof size, "%lld pixels in %d views", pixels, n_views);
    fprintf(stderr, "%s: %s, %lld evaluations (%lld re-evaluated in fp64), best vote %d at row %d col %d roll %d\n", path.c_str(), size,
            (long long)out.n_evals, (long long)out.n_rechecked, out.best_vote, out.best_row, out.best_col, out.best_roll);
    if (n_views > 1 || view_roi) fprintf(stderr, "%d views fused: %lld valid points\n", n_views, (long long)n_points);
    release();
    return rc;
}

int main(int argc, char **argv)
{
    haf_config cfg;
    haf_config_default(&cfg);
    haf_grasp_input in;
    haf_grasp_input_default(&in);
    double sx = 18, sy = 30;                       // launch defaults (launch/haf_grasping_all.launch:25-65)
    bool per_roll = false, hypotheses = false;
    int top_k = 0, top_radius = -1, top_rolls = -1;       // --top-k: ranked candidates (haf_top_grasps); -1: the library's default
    double top_dist = -1.0;
    std::string grid_out;                          // --grid-out FILE: the per-roll grasp grid the shim's callback delivers (979-1016)
    int gpus = 0, shards_per_gpu = 1;
    std::string shard = "rolls";
    std::string features, range, model;
    std::vector<DepthView> views;                  // --depth: 16-bit PGMs in place of the .pcd arguments, the views of one request
    bool have_intrinsics = false, have_labels_pose = false, have_transfer = false;
    MapOptions map_opt;
    haf_transfer_default(&map_opt.transfer_params);
    memset(&map_opt.camera, 0, sizeof map_opt.camera);
    haf_frame frame;                               // the sensor options as they stand: what the next view opened inherits
    haf_frame_default(&frame);
    int first_cloud = argc;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto need = [&](int n) { if (i + n >= argc) { usage(); exit(2); } };
        if (a == "--features") { need(1); features = argv[++i]; }
        else if (a == "--range") { need(1); range = argv[++i]; }
        else if (a == "--model") { need(1); model = argv[++i]; }
        else if (a == "--center") { need(3); for (int k = 0; k < 3; k++) in.grasp_area_center[k] = atof(argv[++i]); }
        else if (a == "--search-size") { need(2); sx = atof(argv[++i]); sy = atof(argv[++i]); }
        else if (a == "--approach") { need(3); for (int k = 0; k < 3; k++) in.approach_vector[k] = atof(argv[++i]); }
        else if (a == "--max-time") { need(1); in.max_calculation_time = atof(argv[++i]); }
        else if (a == "--show-only-best") in.show_only_best_grasp = 1;
        else if (a == "--gripper-width") { need(1); in.gripper_opening_width = atoi(argv[++i]); }
        else if (a == "--grid") { need(1); cfg.grid_h = cfg.grid_w = atoi(argv[++i]); }
        else if (a == "--rolls") { need(1); cfg.n_rolls = atoi(argv[++i]); }
        else if (a == "--roll-step") { need(1); cfg.roll_step_deg = atoi(argv[++i]); }
        else if (a == "--device") { need(1); cfg.device = atoi(argv[++i]); }
        else if (a == "--per-roll") per_roll = true;
        else if (a == "--hypotheses") hypotheses = true;
        else if (a == "--grid-out") { need(1); grid_out = argv[++i]; }
        else if (a == "--top-k") { need(1); top_k = atoi(argv[++i]); }
        else if (a == "--fit-opening") { need(1); if (!parse_opening(argv[++i], &map_opt.clear.opening)) { usage(); return 2; } map_opt.clear.fit = true; }
        else if (a == "--check-space") { need(1); if (!parse_space(argv[++i], &map_opt.clear.seen)) { usage(); return 2; } map_opt.clear.space = true; }
        else if (a == "--gripper") { need(1); if (!parse_gripper(argv[++i], &map_opt.clear.gripper)) { usage(); return 2; } map_opt.clear.on = true; }
        else if (a == "--top-radius") { need(1); top_radius = atoi(argv[++i]); }
        else if (a == "--top-rolls") { need(1); top_rolls = atoi(argv[++i]); }
        else if (a == "--top-dist") { need(1); top_dist = atof(argv[++i]); }
        else if (a == "--map-out") { need(1); map_opt.out_prefix = argv[++i]; }
        else if (a == "--mask") { need(1); map_opt.mask_path = argv[++i]; }
        else if (a == "--roi-mask") { need(1); map_opt.roi_path = argv[++i]; }
        else if (a == "--view-roi-mask") { need(1); if (views.empty()) { usage(); return 2; } views.back().roi_path = argv[++i]; }
        else if (a == "--labels") { need(1); map_opt.labels_path = argv[++i]; }
        else if (a == "--mask-min-vote") { need(1); map_opt.min_vote = atoi(argv[++i]); }
        else if (a == "--depth") { need(1); views.push_back(DepthView{argv[++i], frame, std::string(), {}}); }
        else if (a == "--stack") { need(1); if (views.empty()) { usage(); return 2; } views.back().stack.push_back(argv[++i]); }
        else if (a == "--depth-filter") { need(1); if (!parse_depth_filter(argv[++i], &map_opt.filter_params)) { usage(); return 2; } map_opt.filter = true; }
        else if (a == "--filtered-out") { need(1); map_opt.filtered_out = argv[++i]; }
        else if (a == "--segment") { need(1); if (!parse_segment(argv[++i], &map_opt.segment_params)) { usage(); return 2; } map_opt.segment = true; }
        else if (a == "--segment-cells") { need(1); if (!parse_segment_cells(argv[++i], &map_opt.cell_params)) { usage(); return 2; } map_opt.segment = map_opt.cells = true; }
        else if (a == "--cell-labels-out") { need(1); map_opt.cell_labels_out = argv[++i]; }
        else if (a == "--segment-roi") map_opt.segment_roi = true;
        else if (a == "--fused") map_opt.fused = true;
        else if (a == "--per-object") { map_opt.per_object = true; if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') map_opt.margin_cells = atoi(argv[++i]); }
        else if (a == "--measure") map_opt.measure = true;
        else if (a == "--plane" && i + 1 < argc && strncmp(argv[i + 1], "fit", 3) == 0) { if (!parse_plane_fit(argv[++i], &map_opt.plane_params)) { usage(); return 2; } map_opt.fit_plane = true; }
        else if (a == "--plane-mask") { need(1); map_opt.plane_mask = argv[++i]; }
        else if (a == "--plane") { need(4); for (int k = 0; k < 4; k++) map_opt.plane[k] = (float)atof(argv[++i]); map_opt.have_plane = true; }
        else if (a == "--labels-out") { need(1); map_opt.labels_out = argv[++i]; }
        else if (a == "--labels-camera") {
            need(4);
            map_opt.camera.fx = (float)atof(argv[++i]); map_opt.camera.fy = (float)atof(argv[++i]); map_opt.camera.cx = (float)atof(argv[++i]); map_opt.camera.cy = (float)atof(argv[++i]);
            map_opt.labels_camera = true;
        }
        else if (a == "--labels-pose") { need(12); for (int k = 0; k < 12; k++) map_opt.labels_pose[k] = (float)atof(argv[++i]); have_labels_pose = true; }
        else if (a == "--transfer") { need(1); if (!parse_transfer(argv[++i], &map_opt.transfer_params)) { usage(); return 2; } have_transfer = true; }
        else if (a == "--intrinsics") { need(4); frame.fx = (float)atof(argv[++i]); frame.fy = (float)atof(argv[++i]); frame.cx = (float)atof(argv[++i]); frame.cy = (float)atof(argv[++i]); have_intrinsics = true; }
        else if (a == "--depth-scale") { need(1); frame.depth_scale = (float)atof(argv[++i]); }
        else if (a == "--depth-range") { need(2); frame.min_depth = (float)atof(argv[++i]); frame.max_depth = (float)atof(argv[++i]); }
        else if (a == "--sensor-pose") { need(12); for (int k = 0; k < 12; k++) frame.sensor_to_base[k] = (float)atof(argv[++i]); }
        else if (a == "--probability") cfg.flags |= HAF_FLAG_PROBABILITY;     // svm_with_probability (server.cpp:383, 791, 831-841)
        else if (a == "--gpus") { need(1); gpus = atoi(argv[++i]); }
        else if (a == "--shard") { need(1); shard = argv[++i]; }
        else if (a == "--shards-per-gpu") { need(1); shards_per_gpu = atoi(argv[++i]); if (shards_per_gpu < 1) shards_per_gpu = 1; }
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else { first_cloud = i; break; }
        if (!views.empty()) views.back().frame = frame;       // (a sensor option applies to the view opened last)
    }
    // --segment-cells with a .pcd: that one cloud takes the place of the --depth view (wrapped below, once it is loaded)
    const bool cloud_cells = map_opt.cells && views.empty() && first_cloud + 1 == argc && gpus == 0 && !map_opt.filter && map_opt.plane_mask.empty();
    if (cloud_cells) { views.push_back(DepthView{argv[first_cloud], frame, "", {}}); first_cloud = argc; have_intrinsics = true; }
    const bool from_depth = !views.empty();
    if (features.empty() || range.empty() || model.empty() || (!from_depth && (!map_opt.out_prefix.empty() || !map_opt.mask_path.empty() || !map_opt.labels_path.empty())) ||
        (!map_opt.roi_path.empty() && (views.size() != 1 || !views[0].roi_path.empty())) ||
        (map_opt.segment && !from_depth) || (!map_opt.segment && (map_opt.segment_roi || (map_opt.have_plane && !map_opt.measure && !map_opt.labels_camera) || map_opt.fit_plane || (!map_opt.labels_out.empty() && !map_opt.labels_camera))) ||
        (map_opt.labels_camera ? (map_opt.labels_path.empty() || map_opt.segment || (map_opt.per_object && !map_opt.fused)) : (have_labels_pose || have_transfer)) ||
        (map_opt.fused && !map_opt.per_object) || (!map_opt.cells && !map_opt.cell_labels_out.empty()) ||
        (map_opt.per_object && ((!map_opt.segment && !map_opt.labels_camera) || views.size() != 1 || map_opt.segment_roi || map_opt.measure || !map_opt.roi_path.empty() ||
                                (!map_opt.labels_path.empty() && !map_opt.labels_camera))) ||
        (map_opt.measure && (map_opt.labels_path.empty() || views.size() != 1 || map_opt.segment || map_opt.fit_plane)) ||
        (map_opt.fit_plane && map_opt.have_plane) || (!map_opt.fit_plane && !map_opt.plane_mask.empty()) ||
        (map_opt.segment_roi && (views.size() != 1 || !views[0].roi_path.empty() || !map_opt.roi_path.empty())) ||
        (from_depth ? (first_cloud < argc || !have_intrinsics || gpus > 0 || views.size() > (size_t)HAF_MAX_VIEWS) : first_cloud >= argc)) { usage(); return 2; }
    in.grasp_area_length_x = (float)(sx + 14);     // client.cpp:183-184
    in.grasp_area_length_y = (float)(sy + 14);
    cfg.feature_file = features.c_str();
    cfg.range_file = range.c_str();
    cfg.model_file = model.c_str();
    cfg.max_points = 1 << 22;
    if (map_opt.per_object) cfg.max_clouds = std::max(cfg.max_clouds, 8);      // requests of one chunk

    if (gpus > 0) return run_multi(cfg, in, gpus, shards_per_gpu, shard, argc, argv, first_cloud);

    haf_engine *eng = nullptr;
    if (haf_create(&cfg, &eng) != HAF_OK) { fprintf(stderr, "haf_create: %s\n", haf_last_error(nullptr)); return 1; }
    int rc = 0;
    float *cloud_xyz = nullptr;
    if (cloud_cells) {
        size_t n = 0;
        char err[256];
        if (haf_pcd_load(views[0].path.c_str(), &cloud_xyz, &n, err, sizeof err) != HAF_OK) { fprintf(stderr, "%s: %s\n", views[0].path.c_str(), err); haf_destroy(eng); return 1; }
        if (n < 1 || n > (size_t)cfg.max_points) { fprintf(stderr, "%s: %zu points: none, or more than max_points\n", views[0].path.c_str(), n); haf_free(cloud_xyz); haf_destroy(eng); return 1; }
        haf_frame &f = views[0].frame;
        haf_frame_default(&f);                             // (the identity pose: the cloud is in the base frame)
        f.kind = HAF_FRAME_XYZ_F32; f.data = cloud_xyz; f.width = (int32_t)n; f.height = 1;
        f.point_stride_bytes = 12; f.row_stride_bytes = n * 12;
    }
    if (from_depth) {
        // (the goal goes through the adapter's fields like every other: goal_to_input rounds the duration through float, 277)
        hafshim::GoalFields goal;
        for (int k = 0; k < 3; k++) { goal.center[k] = in.grasp_area_center[k]; goal.approach_vector[k] = in.approach_vector[k]; }
        goal.length_x = in.grasp_area_length_x; goal.length_y = in.grasp_area_length_y;
        goal.max_calculation_time = in.max_calculation_time;
        goal.show_only_best_grasp = in.show_only_best_grasp != 0;
        goal.gripper_opening_width = in.gripper_opening_width;
        haf_grasp_input gin;
        hafshim::goal_to_input(goal, &gin);
        rc = run_depth(eng, cfg, gin, views, hypotheses, top_k, top_radius, top_rolls, top_dist, map_opt);
        haf_free(cloud_xyz);
        haf_destroy(eng);
        return rc;
    }
    for (int i = first_cloud; i < argc; i++) {
        float *xyz = nullptr;
        size_t n = 0;
        char err[256];
        if (haf_pcd_load(argv[i], &xyz, &n, err, sizeof err) != HAF_OK) { fprintf(stderr, "%s: %s\n", argv[i], err); rc = 1; continue; }
        haf_cloud cloud = {xyz, n, 3, 0};
        // the goal goes the way the ROS adapter sends it: GoalFields -> hafshim::run_goal (ros_shim/shim_core.h).  stdout gets
        // what the server publishes on /haf_grasping/grasp_hypothesis_with_eval: with --hypotheses every roll's own
        // hypothesis first (server.cpp:962-969), always the overall best last (390 -> 1384, 1419)
        hafshim::GoalFields goal;
        for (int k = 0; k < 3; k++) { goal.center[k] = in.grasp_area_center[k]; goal.approach_vector[k] = in.approach_vector[k]; }
        goal.length_x = in.grasp_area_length_x; goal.length_y = in.grasp_area_length_y;
        goal.max_calculation_time = in.max_calculation_time;
        goal.show_only_best_grasp = in.show_only_best_grasp != 0;
        goal.gripper_opening_width = in.gripper_opening_width;
        std::vector<std::string> lines;
        hafshim::ResultFields res;
        haf_grasp_output out;
        std::string serr;
        FILE *gf = grid_out.empty() ? nullptr : fopen(grid_out.c_str(), i == first_cloud ? "w" : "a");
        hafshim::GridFn on_grid;
        if (gf) on_grid = [&](int roll, const std::vector<hafshim::GridCell> &cells) {
            for (const hafshim::GridCell &c : cells)
                fprintf(gf, "%d %d %d %.9g %.9g %.9g %.9g\n", roll, c.row, c.col, c.x, c.y, c.z, c.value);
        };
        const int grc = hafshim::run_goal(eng, cfg, goal, cloud, [&](const std::string &l) { lines.push_back(l); }, &res, &out, &serr, on_grid);
        if (gf) fclose(gf);
        if (grc != HAF_OK) {
            fprintf(stderr, "%s: %s\n", argv[i], serr.c_str());
            rc = 1;
            haf_free(xyz);
            continue;
        }
        for (size_t l = 0; l + 1 < lines.size(); l++)
            if (hypotheses) printf("hypothesis %s\n", lines[l].c_str());
        printf("%s\n", lines.back().c_str());
        (void)res;
        haf_frame scene;                                  // --gripper: the cloud as an N x 1 frame in the base frame
        haf_frame_default(&scene);
        scene.data = xyz; scene.kind = HAF_FRAME_XYZ_F32; scene.width = (int32_t)n; scene.height = 1;
        scene.row_stride_bytes = n * 12; scene.point_stride_bytes = 12;
        if (top_k > 0) print_top(eng, cfg, argv[i], top_k, top_radius, top_rolls, top_dist, &rc, &map_opt.clear, &scene);
        fprintf(stderr, "%s: %zu points, %lld evaluations (%lld re-evaluated in fp64), best vote %d at row %d col %d roll %d\n", argv[i], n,
                (long long)out.n_evals, (long long)out.n_rechecked, out.best_vote, out.best_row, out.best_col, out.best_roll);
        if (per_roll) {
            haf_roll_record *rec = (haf_roll_record *)malloc(sizeof(haf_roll_record) * (size_t)cfg.n_rolls);
            if (haf_score_rolls(eng, 1, &cloud, &in, 0, cfg.n_rolls, rec) == HAF_OK)
                for (int r = 0; r < cfg.n_rolls; r++)
                    fprintf(stderr, "  roll %3d deg: vote %4d at (%d, %d), %d cells\n", r * cfg.roll_step_deg, rec[r].vote, rec[r].row, rec[r].col, rec[r].n_evals);
            free(rec);
        }
        haf_free(xyz);
    }
    haf_destroy(eng);
    return rc;
}
