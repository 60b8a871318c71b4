// shim_core.h -- everything of the action-server shim that does not need ROS: goal fields -> haf_grasp_input, the roll-by-roll
// hypothesis publication rule, GraspOutput fields, and the text of /haf_grasping/grasp_hypothesis_with_eval.  Header-only,
// C++11, depends on include/hafgrasp.h alone, so it is compiled and tested in this repository (haf_grasp_cli uses it;
// tests/test_engine_gpu.py::test_cli_and_server_mirror, tests/test_host_cpu.py) although ROS is not installed here.
// ros_shim/calc_grasppoints_action_server_hip.cpp is the thin adapter that fills GoalFields from the ROS message and
// copies ResultFields back.
//
// Reference lines (src/calc_grasppoints_action_server.cpp): goal parsing 258-301, roll loop 343-386 (preemption 350-357), per-roll
// grasp grid 901-902 / 979-1016, per-roll publication 962-969, result fields and string 1384-1401, final call 390.
#ifndef HAF_SHIM_CORE_H_
#define HAF_SHIM_CORE_H_

#include <hafgrasp.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <sstream>
#include <string>
#include <vector>

namespace hafshim {

// msg/GraspInput.msg:3-15 without the cloud (passed separately, already in the base frame: server.cpp:316)
struct GoalFields {
    std::string goal_frame_id;               // "" -> "/base_link" (294-301)
    double center[3] = {0, 0, 0};            // grasp_area_center
    float  length_x = 32, length_y = 44;     // grasp_area_length_x/y: cm incl. the +14 border (client.cpp:183-184)
    double max_calculation_time = 50;        // ros::Duration::toSec()
    bool   show_only_best_grasp = false;
    int    threshold_grasp_evaluation = 0;   // never read by the reference server
    double approach_vector[3] = {0, 0, 1};
    int    gripper_opening_width = 1;
};

// msg/GraspOutput.msg:1-7 (header.stamp is the adapter's business)
struct ResultFields {
    std::string frame_id;
    int    eval = -20;
    double grasp_point1[3] = {0, 0, 0}, grasp_point2[3] = {0, 0, 0}, averaged_grasp_point[3] = {0, 0, 0};
    double approach_vector[3] = {0, 0, 0};
    float  roll = 0;
};

// One cell of the per-roll grasp grid as publish_grasp_grid (979-1016) hands it to gp_to_marker: every cell of
// point_inside_box_grid (the mask), its position in the base frame (987-989, 996) and graspseval[row][col] (865-880).
struct GridCell {
    int row, col;
    float x, y, z;
    float value;
};
typedef std::function<void(int roll, const std::vector<GridCell> &)> GridFn;
typedef std::function<bool()> PreemptFn;             // as_.isPreemptRequested() || !ros::ok() (350)
enum { HAF_SHIM_PREEMPTED = 1 };                      // run_goal: the goal was preempted -> setPreempted() (354-356)

inline std::string base_frame(const GoalFields &g) { return g.goal_frame_id.empty() ? std::string("/base_link") : g.goal_frame_id; }   // 294-301

// read_pc_cb 258-284.  The engine normalises the approach vector (270-273) and truncates the lengths to int (266-267)
// itself, exactly as the server does, so the fields go over unchanged; the duration goes through float like 277.
inline void goal_to_input(const GoalFields &g, haf_grasp_input *in)
{
    haf_grasp_input_default(in);
    for (int k = 0; k < 3; k++) in->grasp_area_center[k] = g.center[k];                    // 258-260
    in->grasp_area_length_x = g.length_x;                                                  // 266-267
    in->grasp_area_length_y = g.length_y;
    for (int k = 0; k < 3; k++) in->approach_vector[k] = g.approach_vector[k];             // 270-273
    in->max_calculation_time = (double)(float)g.max_calculation_time;                      // 277
    in->gripper_opening_width = g.gripper_opening_width;                                   // 281
    in->show_only_best_grasp = g.show_only_best_grasp ? 1 : 0;                             // 284
    in->threshold_grasp_evaluation = g.threshold_grasp_evaluation;
}

// 1386-1401
inline void output_to_result(const haf_grasp_output &o, const std::string &frame_id, ResultFields *r)
{
    r->frame_id = frame_id;
    r->eval = o.eval;
    for (int k = 0; k < 3; k++) {
        r->grasp_point1[k] = o.grasp_point1[k];
        r->grasp_point2[k] = o.grasp_point2[k];
        r->averaged_grasp_point[k] = o.averaged_grasp_point[k];
        r->approach_vector[k] = o.approach_vector[k];
    }
    r->roll = o.roll;
}

// The string of server.cpp:1384: "<eval> <gp1 xyz> <gp2 xyz> <approach xyz> <averaged xyz> <roll in degrees>".  The reference
// streams Eigen floats (gp1_wcs, gp2_wcs, appr_vec) and doubles (the averages, (float + float) / 2.0) into a default
// std::stringstream; the same stream with the same types gives the same text (6 significant digits).
inline std::string hypothesis_string(const haf_grasp_output &o, int roll_step_deg)
{
    std::stringstream ss;
    ss << o.eval << " " << (float)o.grasp_point1[0] << " " << (float)o.grasp_point1[1] << " " << (float)o.grasp_point1[2] << " "
       << (float)o.grasp_point2[0] << " " << (float)o.grasp_point2[1] << " " << (float)o.grasp_point2[2] << " "
       << (float)o.approach_vector[0] << " " << (float)o.approach_vector[1] << " " << (float)o.approach_vector[2] << " "
       << o.averaged_grasp_point[0] << " " << o.averaged_grasp_point[1] << " " << o.averaged_grasp_point[2] << " "
       << o.best_roll * roll_step_deg;
    return ss.str();
}

// One goal, as read_pc_cb + loop_control run it once the cloud is in the base frame: every roll is scored (one call), the
// hypotheses the server would publish roll by roll (962-969: !show_only_best and vote > graspval_th, eval = max(vote-20, 10))
// are handed to `publish` in roll order for the rolls the sequential loop would have executed (early exit 362-365), then
// the overall best (390) -- which the server publishes on the same topic (1419) -- and the result fields.
// Returns the engine's status; on failure *err carries haf_last_error().
// `grid` (optional) receives, for every roll the sequential loop would have executed and in roll order, the cells of that roll's
// grasp grid (901-902): what the reference turns into rviz markers.  `preempted` (optional) is asked where the reference asks
// (350: at the top of a roll -- here all rolls of a goal are scored in ONE call of a few hundred microseconds to milliseconds, so
// that is before the call and again before anything is published); a preempted goal returns HAF_SHIM_PREEMPTED and publishes nothing.
inline int run_goal(haf_engine *engine, const haf_config &cfg, const GoalFields &goal, const haf_cloud &cloud,
                    const std::function<void(const std::string &)> &publish, ResultFields *result, haf_grasp_output *raw,
                    std::string *err, const GridFn &grid = GridFn(), const PreemptFn &preempted = PreemptFn())
{
    haf_grasp_input in;
    goal_to_input(goal, &in);
    if (preempted && preempted()) return HAF_SHIM_PREEMPTED;
    std::vector<haf_roll_record> rec((size_t)cfg.n_rolls);
    int rc = haf_score_rolls(engine, 1, &cloud, &in, 0, cfg.n_rolls, rec.data());
    haf_grasp_output out;
    if (rc == HAF_OK) rc = haf_finalize(engine, &in, rec.data(), &out);
    if (rc != HAF_OK) {
        if (err) *err = haf_last_error(engine);
        return rc;
    }
    if (preempted && preempted()) return HAF_SHIM_PREEMPTED;
    if (grid) {
        const size_t HW = (size_t)cfg.grid_h * cfg.grid_w;
        std::vector<float> ev(HW);
        std::vector<uint8_t> mask(HW);
        std::vector<GridCell> cells;
        const int gw = in.gripper_opening_width;
        // publish_grasp_grid 987-989 (float arithmetic on the double centre, integer division HEIGHT/2/gripperwidth inside 0.01*...)
        const float x0 = (float)(in.grasp_area_center[0] - 0.01 * cfg.grid_h / 2 / gw);
        const float y0 = (float)(in.grasp_area_center[1] - 0.01 * cfg.grid_w / 2);
        const float z0 = (float)(in.grasp_area_center[2] + cfg.z_shift);
        for (int r = 0; r < out.rolls_done; r++) {
            rc = haf_get_roll_grid(engine, 0, r, ev.data(), mask.data());
            if (rc != HAF_OK) {
                if (err) *err = haf_last_error(engine);
                return rc;
            }
            cells.clear();
            for (int row = 0; row < cfg.grid_h; row++)
                for (int col = 0; col < cfg.grid_w; col++)
                    if (mask[(size_t)row * cfg.grid_w + col])                                           // 993-995
                        cells.push_back(GridCell{row, col, (float)(x0 + 0.01 / gw * row), (float)(y0 + 0.01 * col), z0,
                                                 ev[(size_t)row * cfg.grid_w + col]});                  // 996
            grid(r, cells);
        }
    }
    for (int r = 0; r < out.rolls_done; r++) {
        haf_grasp_output ro;
        int32_t pub = 0;
        rc = haf_roll_pose(engine, &in, rec.data(), r, &ro, &pub);
        if (rc != HAF_OK) {
            if (err) *err = haf_last_error(engine);
            return rc;
        }
        if (pub && publish) publish(hypothesis_string(ro, cfg.roll_step_deg));
    }
    if (publish) publish(hypothesis_string(out, cfg.roll_step_deg));                      // 390 -> 1419
    if (result) output_to_result(out, base_frame(goal), result);
    if (raw) *raw = out;
    return HAF_OK;
}

// The ranked top-k candidates of the engine's last scored goal (haf_top_grasps; run_goal scores one cloud per call) as hypothesis
// strings, best first -- the next-best DISTINCT grasps for a planner whose first choice fails IK or a collision check.  An adapter
// would publish them after the goal's own result, or hand them back in a service reply.  Returns the engine's status; on failure
// *err carries haf_last_error().
inline int top_hypotheses(haf_engine *engine, const haf_config &cfg, const haf_top_params &p, std::vector<std::string> *lines,
                          std::string *err)
{
    const size_t clouds = (size_t)(cfg.max_clouds > 0 ? cfg.max_clouds : 1), k = (size_t)(p.k > 0 ? p.k : 1);
    std::vector<haf_grasp_candidate> cand(clouds * k);
    std::vector<int32_t> n(clouds, 0);
    const int rc = haf_top_grasps(engine, &p, cand.data(), n.data());
    if (rc != HAF_OK) {
        if (err) *err = haf_last_error(engine);
        return rc;
    }
    for (int32_t i = 0; i < n[0]; i++) lines->push_back(hypothesis_string(cand[(size_t)i].grasp, cfg.roll_step_deg));
    return HAF_OK;
}

// top_hypotheses for a parallel-jaw gripper: the same ranked candidates, each with the smallest free opening of `gripper` against the
// scene's points in `scene` (haf_fit_openings; the gripper's own opening is not read) APPLIED -- the grasp points that opening apart about
// a centre moved sideways by the shift found (haf_apply_opening) --, as hypothesis strings, best first; a candidate without a free
// opening is left out.  An adapter would publish them where it publishes top_hypotheses', for a planner that commands the gripper's
// opening from the distance of the two grasp points.  Returns the engine's status; on failure *err carries haf_last_error().
inline int fitted_hypotheses(haf_engine *engine, const haf_config &cfg, const haf_top_params &p, const haf_frame &scene, const haf_gripper &gripper,
                             const haf_opening_params &opening, std::vector<std::string> *lines, std::string *err)
{
    const size_t clouds = (size_t)(cfg.max_clouds > 0 ? cfg.max_clouds : 1), k = (size_t)(p.k > 0 ? p.k : 1);
    std::vector<haf_grasp_candidate> cand(clouds * k);
    std::vector<int32_t> n(clouds, 0);
    int rc = haf_top_grasps(engine, &p, cand.data(), n.data());
    if (rc == HAF_OK && n[0] > 0) {
        std::vector<haf_grasp_opening> fits((size_t)n[0]);
        rc = haf_fit_openings(engine, &scene, nullptr, &gripper, &opening, n[0], cand.data(), sizeof(haf_grasp_candidate), fits.data(), nullptr,
                              nullptr, nullptr, nullptr);
        for (int32_t i = 0; rc == HAF_OK && i < n[0]; i++) {
            haf_grasp_output applied;
            if (fits[(size_t)i].found == 1 && haf_apply_opening(&cand[(size_t)i].grasp, &fits[(size_t)i], &applied) == HAF_OK)
                lines->push_back(hypothesis_string(applied, cfg.roll_step_deg));
        }
    }
    if (rc != HAF_OK && err) *err = haf_last_error(engine);
    return rc;
}

// top_hypotheses for a planner that may only go where a camera has looked: the same ranked candidates, each checked against the depth
// views `views` (haf_check_space: the sample points of `gripper`'s volume seen free, hit, hidden or not at all), as hypothesis strings,
// best first; a candidate whose row does not say clear == 1 is left out.  An adapter with one or more depth topics would publish them
// where it publishes top_hypotheses'.  rows (may be null): every candidate's row, in rank order, the ones that are not clear included.
// Returns the engine's status; on failure *err carries haf_last_error().
inline int seen_free_hypotheses(haf_engine *engine, const haf_config &cfg, const haf_top_params &p, const haf_frame *views, int32_t n_views,
                                const haf_gripper &gripper, const haf_space_params &space, std::vector<std::string> *lines, std::string *err,
                                std::vector<haf_grasp_space> *rows_out = nullptr)
{
    const size_t clouds = (size_t)(cfg.max_clouds > 0 ? cfg.max_clouds : 1), k = (size_t)(p.k > 0 ? p.k : 1);
    std::vector<haf_grasp_candidate> cand(clouds * k);
    std::vector<int32_t> n(clouds, 0);
    int rc = haf_top_grasps(engine, &p, cand.data(), n.data());
    if (rc == HAF_OK && n[0] > 0) {
        std::vector<haf_grasp_space> rows((size_t)n[0]);
        rc = haf_check_space(engine, views, n_views, &gripper, &space, n[0], cand.data(), sizeof(haf_grasp_candidate), rows.data(), nullptr, nullptr,
                             nullptr, nullptr);
        for (int32_t i = 0; rc == HAF_OK && i < n[0]; i++)
            if (rows[(size_t)i].clear == 1) lines->push_back(hypothesis_string(cand[(size_t)i].grasp, cfg.roll_step_deg));
        if (rc == HAF_OK && rows_out) *rows_out = rows;
    }
    if (rc != HAF_OK && err) *err = haf_last_error(engine);
    return rc;
}

// The best grasp per object of the engine's last scored goal from an instance-label image that goes with `frame` (haf_grasp_map_labels):
// one line "<label> <u> <v> <hypothesis string>" per object that has a pixel with a vote >= min_vote, best first -- the next OBJECT for a
// planner whose first choice fails, where top_hypotheses gives the next grasp.  An adapter with a label topic synchronised with the depth
// topic would publish them after the goal's own result.  Returns the engine's status; on failure *err carries haf_last_error().
inline int label_hypotheses(haf_engine *engine, const haf_config &cfg, const haf_frame &frame, const haf_label_image &labels, int32_t n_labels,
                            int32_t min_vote, std::vector<std::string> *lines, std::string *err)
{
    const size_t n = (size_t)(n_labels > 0 ? n_labels : 1);
    std::vector<haf_label_pick> picks(n);
    std::vector<haf_grasp_candidate> poses(n);
    std::vector<int32_t> order(n, 0);
    int32_t n_found = 0;
    const int rc = haf_grasp_map_labels(engine, 0, &frame, &labels, n_labels, min_vote, picks.data(), poses.data(), order.data(), &n_found);
    if (rc != HAF_OK) {
        if (err) *err = haf_last_error(engine);
        return rc;
    }
    for (int32_t k = 0; k < n_found; k++) {
        const size_t l = (size_t)order[(size_t)k] - 1;
        lines->push_back(std::to_string(order[(size_t)k]) + " " + std::to_string(picks[l].u) + " " + std::to_string(picks[l].v) + " " +
                         hypothesis_string(poses[l].grasp, cfg.roll_step_deg));
    }
    return HAF_OK;
}

// No segmenter on the robot: the parameters of haf_segment_frame for a goal.  The support plane passes through the goal's grasp area
// centre c with the goal's unit approach vector n as its normal, plane = (n, -n.c), so a point's height is its distance from that plane
// along the approach direction; the other fields are the library's defaults.  THE CALLER OWNS THE TABLE HEIGHT: the centre must lie on
// the support surface, or min_height must make up for it.  The adapter segments the depth frame into the engine's uint8 image, scores
// with haf_score_frames_roi under that image as the device mask, and hands the same image to label_hypotheses.
inline void segment_params_from_goal(const GoalFields &g, haf_segment_params *p)
{
    haf_segment_default(p);
    double n[3] = {g.approach_vector[0], g.approach_vector[1], g.approach_vector[2]};
    double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(len > 0.0)) { n[0] = 0.0; n[1] = 0.0; n[2] = 1.0; len = 1.0; }                     // (a zero or NaN vector: the default approach, +z)
    double d = 0.0;
    for (int k = 0; k < 3; k++) { n[k] /= len; d -= n[k] * g.center[k]; }
    for (int k = 0; k < 3; k++) p->plane[k] = (float)n[k];
    p->plane[3] = (float)d;
}

// The same without owning the table height: the support plane is the frame's dominant plane, fitted on the device (haf_fit_plane) with
// `fit` (null: the library's defaults).  p comes in filled -- by segment_params_from_goal, say -- and only its plane changes, and only
// when a plane was found: with *found == 0 the goal's plane stays, the fall-back.  result (may be null): the whole fit.  Returns
// haf_fit_plane's status; on an error p is untouched and *found is 0.
inline int segment_params_from_fit(haf_engine *e, const haf_frame *frame, haf_segment_params *p, int *found,
                                   const haf_plane_params *fit = nullptr, haf_plane_result *result = nullptr)
{
    haf_plane_params defaults;
    haf_plane_default(&defaults);
    haf_plane_result r;
    *found = 0;
    const int rc = haf_fit_plane(e, frame, nullptr, fit ? fit : &defaults, &r, nullptr, nullptr);
    if (rc != HAF_OK) return rc;
    *found = r.found;
    if (r.found) memcpy(p->plane, r.plane, sizeof p->plane);
    if (result) *result = r;
    return HAF_OK;
}

}  // namespace hafshim
#endif  // HAF_SHIM_CORE_H_
