// frames.h -- what the host units share about sensor frames (haf_frame, include/hafgrasp.h): the descriptor the kernels read, the argument
// checks every entry point applies to a frame's own fields, and the per-frame constants of the arithmetic (frame_points.h).  frames_host.cpp defines them and
// needs neither HIP nor an engine.
#pragma once
#include "../../include/hafgrasp.h"
#include "frame_points.h"
#include "segment_rules.h"
#include "plane_rules.h"
#include "label_shape.h"
#include "cell_segment_rules.h"
#include "transfer_rules.h"
#include "clearance_rules.h"
#include "opening_rules.h"
#include "space_rules.h"

#include <string>

namespace haf {

// per sensor frame of a haf_score_frames batch (frames.hip): where its pixels lie and where its points go.  The array rides in the
// request's header block behind the RollGeo array.  dst is 16-byte aligned (the points of a frame start at a multiple of four points).
// haf_score_views: one entry per VIEW; dst is the start of the request's region (all its views share it) and count the request's live
// point counter on the device, CloudDev::n, which k_view_points advances (null on the haf_score_frames path)
struct FrameDev {
    const void *src;                 // first pixel: the raw area (staged host depth frames), dst itself (staged host XYZ frames: in place), or the caller's device memory
    float *dst;                      // packed xyz, width * height points: CloudDev::xyz of the same index
    int *count;                      // views only: CloudDev::n of the request
    unsigned long long row_stride;   // bytes between rows of src
    unsigned point_stride;           // bytes between pixels of a row
    int width, n;                    // n = width * height
    int kind;                        // HAF_FRAME_*
    haf_frame_math::FrameMath m;
};

// bytes between two pixels of a row: 2 / 4 for the depth kinds, point_stride_bytes for XYZ; 0 for an unknown kind
size_t frame_elem_bytes(const haf_frame &f);
// bytes of a pixel the engine moves: 2 / 4 / 12
size_t frame_pixel_bytes(int kind);
// HAF_OK, HAF_E_ARG or HAF_E_CAPACITY with a message: every refusal of a frame that needs no engine
int check_frame(const haf_frame &f, std::string &err);
// ifx = 1.0f / fx, ify = 1.0f / fy: formed once per frame, here
haf_frame_math::FrameMath frame_math(const haf_frame &f);
// haf_view_points (include/hafgrasp.h) with its refusal's text: the valid points of host frames, in order
int view_points_impl(const haf_frame *frames, int32_t n_views, float *xyz, size_t cap_points, size_t *n_valid, std::string &err);
// depthfilter_host.cpp, shared by haf_filter_depth_ref and haf_filter_depth: every refusal of an exposure stack and of the filter's
// parameters that needs no engine (the text names the frame), and every refusal of the output image that goes with a checked stack
// (frame_stage.h: check_output_image, then no byte shared with an exposure; out may be null only with out_on_device = 1)
int check_depth_stack(const haf_frame *frames, int32_t n_frames, const haf_depth_filter *p, std::string &err);
int check_depth_out(const haf_frame *frames, int32_t n_frames, const void *out, size_t out_row_stride_bytes, int32_t out_on_device, std::string &err);
// segment_host.cpp, shared by haf_segment_ref and haf_segment_frame: every refusal of a frame, of the parameters and of the label image
// that needs no engine (the image's: frame_stage.h's check_label_output; labels may be null only with out_on_device = 1); the
// predicates' constants, gap2 formed here
int check_segment(const haf_frame *frame, const haf_segment_params *p, const void *labels, int32_t elem_bytes, size_t row_stride_bytes,
                  int32_t out_on_device, const int32_t *n_labels, std::string &err);
haf_segment_math::SegmentRules segment_rules(const haf_segment_params &p);
// cellsegment_host.cpp, shared by haf_segment_cells_ref and haf_segment_cells: every refusal of a frame, of the parameters and of the
// label image that needs no engine (check_frame, check_label_output); the rules' constants, inv_cell formed here
int check_cell_segment(const haf_frame *frame, const haf_cell_segment_params *p, const void *labels, int32_t elem_bytes, size_t row_stride_bytes,
                       int32_t out_on_device, const int32_t *n_labels, std::string &err);
haf_cell_math::CellRules cell_rules(const haf_cell_segment_params &p);
// plane_host.cpp, shared by haf_fit_plane_ref and haf_fit_plane: every refusal of a frame, of the mask and of the parameters that needs
// no engine; the rules' constants, tol2, cos2 and uu formed here; the winner of a count array (largest count, ties to the lowest k)
int check_plane(const haf_frame *frame, const haf_roi *mask, const haf_plane_params *p, const haf_plane_result *out, std::string &err);
haf_plane_math::PlaneRules plane_rules(const haf_plane_params &p);
int plane_winner(const int32_t *counts, int32_t n_hyp);
// THE plane of a fit, from integers only: the ten moments of the winner's inliers, the winner's four hypothesis words (the fall-back),
// up (all zero: none) and the sensor's origin in the base frame -> plane[4] in metres, rounded to float, and the inliers' rms distance.
// Both entry points call this one function on the same integers, so its double arithmetic need not be pinned across machines
void plane_from_moments(const int64_t *moments, const float *hyp, const float *up, const float *origin, float *plane, double *rms);
// everything of a result that follows the counts, the hypothesis words and the moments -- out->moments and stats[0..2] are filled by the caller
void plane_finish(const haf_frame &f, const haf_plane_params &p, const int32_t *counts, const float *hyps, haf_plane_result *out);
// labelshape_host.cpp, shared by haf_measure_labels_ref and haf_measure_labels: every refusal of a frame, of the label image, of the plane
// and of the output that needs no engine
int check_measure(const haf_frame *frame, const haf_label_image *labels, int32_t n_labels, const float *plane, const haf_label_shape *shapes,
                  std::string &err);
// THE derived fields of a shape, from its integers and h_max only (found .. height; reserved = 0).  Both entry points call this one
// function on the same integers, so its double arithmetic need not be pinned across machines
void shape_finish(haf_label_shape *s);
// a label's row of the device table (label_shape.h: kShapeRowWords words, as copied back) -> its integers and h_max, then shape_finish
void shape_from_row(const uint32_t *row, haf_label_shape *s);
// transfer_host.cpp, shared by haf_transfer_labels_ref and haf_transfer_labels: every refusal of the depth frame, the camera, its label
// image, the parameters and the label output that needs no engine (check_frame, check_label_output, and check_label_image with the
// CAMERA's width; labels may be null only with out_on_device = 1); THE constants of a call, formed here in double
int check_transfer(const haf_frame *depth, const haf_camera *cam, const haf_label_image *cam_labels, int32_t n_labels,
                   const haf_transfer_params *p, const void *labels, int32_t elem_bytes, size_t row_stride_bytes, int32_t out_on_device,
                   std::string &err);
haf_transfer_math::TransferRules transfer_rules(const haf_camera &cam, const haf_transfer_params &p);
// ... its refusals of a camera's own fields, and of near_m, tol_abs and tol_rel (name: the parameter struct's, for the text); haf_check_space
// applies both to every view
int check_camera(const haf_camera &cam, std::string &err);
int check_projection_params(const char *name, float near_m, float tol_abs, float tol_rel, std::string &err);
// clearance_host.cpp, shared by haf_check_grasps_ref and haf_check_grasps: every refusal of the frame, the mask, the gripper and the
// grasp list that needs no engine (*bounds filled when the gripper passes); THE integer bounds and the reach of a gripper, false for one
// the call refuses; THE twelve words of a grasp, in double (reach_q = -1 for a void one); the words of n grasps read at a stride
int check_clearance(const haf_frame *frame, const haf_roi *mask, const haf_gripper *gripper, int32_t n_grasps, const void *grasps,
                    size_t grasp_stride_bytes, const haf_grasp_clearance *out, haf_clear_math::ClearBounds *bounds, std::string &err);
// ... its refusals of the gripper, n_grasps and the stride alone (*bounds filled when the gripper passes); haf_check_space applies them
int check_grasp_list(const haf_gripper *gripper, int32_t n_grasps, size_t grasp_stride_bytes, haf_clear_math::ClearBounds *bounds, std::string &err);
bool gripper_rules(const haf_gripper &g, haf_clear_math::ClearBounds *b);
// the unit axes of a grasp in double: a along the approach vector, c the closing axis, b = a x c; false for a void grasp
bool grasp_axes(const haf_grasp_output &g, double *a, double *b, double *c);
void grasp_frame(const haf_grasp_output &g, int32_t reach_q, haf_clear_math::GraspWords *w);
void grasp_frames(const void *grasps, size_t stride, int32_t n, int32_t reach_q, haf_clear_math::GraspWords *w);
// a grasp's row of the device table (clearance_rules.h: kClearRowWords words, as copied back) -> the plain integers of the host's row
void clearance_row_decode(const uint32_t *dev_row, int32_t *row);
// THE derived fields of every grasp from its integer row (rows: n x kClearRowWords host words), order and n_free (either may be null)
void clearance_finish(const haf_gripper &g, const haf_clear_math::GraspWords *w, const int32_t *rows, int32_t n, haf_grasp_clearance *out,
                      int32_t *order, int32_t *n_free);
// opening_host.cpp, shared by haf_fit_openings_ref and haf_fit_openings: every refusal that needs no engine -- check_clearance's for the
// gripper at max_opening, then the parameters' (*rules filled when all pass); THE integers of a call from the gripper's and the
// parameters' doubles, false with the reason for what the call refuses; what a caller is told about them
int check_openings(const haf_frame *frame, const haf_roi *mask, const haf_gripper *gripper, const haf_opening_params *params, int32_t n_grasps,
                   const void *grasps, size_t grasp_stride_bytes, const haf_grasp_opening *out, haf_open_math::OpenRules *rules, std::string &err);
bool opening_rules(const haf_gripper &g, const haf_opening_params &p, haf_open_math::OpenRules *r, std::string &why);
void opening_info(const haf_open_math::OpenRules &r, haf_opening_info *info);
// THE derived fields of every grasp from its integer row (rows: n x kOpenRowWords host words; a void grasp's is not read), order and
// n_found (either may be null)
void opening_finish(const haf_open_math::OpenRules &r, const haf_clear_math::GraspWords *w, const int32_t *rows, int32_t n,
                    haf_grasp_opening *out, int32_t *order, int32_t *n_found);
// space_host.cpp, shared by haf_check_space_ref and haf_check_space: every refusal that needs no engine -- check_grasp_list's, the
// parameters', then per view check_frame's, the kind, haf_invert_pose's and check_camera's, the lattice's size and the size of `states`
// (*call filled when all pass: the gripper's bounds, the lattice and every view's rules); what a caller is told about the lattice
struct SpaceCall {
    haf_clear_math::ClearBounds b;
    haf_space_math::SpaceLattice l;
    haf_space_math::SpaceViewRules v[haf_space_math::kSpaceMaxViews];
};
int check_space(const haf_frame *views, int32_t n_views, const haf_gripper *gripper, const haf_space_params *params, int32_t n_grasps,
                const void *grasps, size_t grasp_stride_bytes, const haf_grasp_space *out, const uint8_t *states, SpaceCall *call, std::string &err);
// THE lattice of a call from the gripper's bounds and the step's word (N = l->first[4] may exceed the cap: check_space refuses it)
void space_lattice(const haf_clear_math::ClearBounds &b, int32_t S, haf_space_math::SpaceLattice *l);
void space_info(const haf_space_math::SpaceLattice &l, haf_space_info *info);
// THE row of every grasp from its sixteen counts (rows: n x kSpaceRowWords host words; a void grasp's is not read), clear, order and
// n_clear (either may be null)
void space_finish(const haf_space_params &p, const haf_clear_math::GraspWords *w, const int32_t *rows, int32_t n, haf_grasp_space *out,
                  int32_t *order, int32_t *n_clear);

}  // namespace haf
