"""Host-side mirror of the reference's action interface for the hot path.

Reference: action/CalcGraspPointsServer.action:1-8 (goal GraspInput, result GraspOutput),
msg/GraspInput.msg:3-15, msg/GraspOutput.msg:1-7, and the server object CCalc_Grasppoints
(src/calc_grasppoints_action_server.cpp:107-229).  Field names and meanings are the reference's; the point
cloud is a float32 [N, 3] array already in the base frame (the server transforms it at :316 before the hot path).
"""
import ctypes as C
import dataclasses
from typing import Sequence

import numpy as np

from . import capi


@dataclasses.dataclass
class GraspInputMsg:
    """msg/GraspInput.msg.  grasp_area_length_* are declared 'in m' but the server uses them as integer
    centimetres including the 14 cm border (server.cpp:266-267; client.cpp:183-184 sends size + 14)."""
    input_pc: np.ndarray = None
    goal_frame_id: str = ""
    grasp_area_center: Sequence[float] = (0.0, 0.0, 0.0)
    grasp_area_length_x: float = 32.0
    grasp_area_length_y: float = 44.0
    max_calculation_time: float = 50.0
    show_only_best_grasp: bool = False
    threshold_grasp_evaluation: int = 0
    approach_vector: Sequence[float] = (0.0, 0.0, 1.0)
    gripper_opening_width: int = 1

    def to_c(self):
        return capi.default_input(grasp_area_center=tuple(self.grasp_area_center),
                                  grasp_area_length_x=float(self.grasp_area_length_x),
                                  grasp_area_length_y=float(self.grasp_area_length_y),
                                  approach_vector=tuple(self.approach_vector),
                                  max_calculation_time=float(self.max_calculation_time),
                                  show_only_best_grasp=int(bool(self.show_only_best_grasp)),
                                  threshold_grasp_evaluation=int(self.threshold_grasp_evaluation),
                                  gripper_opening_width=int(self.gripper_opening_width))


@dataclasses.dataclass
class GraspOutputMsg:
    """msg/GraspOutput.msg (header.frame_id = base frame, server.cpp:1386-1387)."""
    frame_id: str
    eval: int
    graspPoint1: tuple
    graspPoint2: tuple
    averagedGraspPoint: tuple
    approachVector: tuple
    roll: float

    def hypothesis_string(self, roll_step_deg=15):
        """The string the server publishes on /haf_grasping/grasp_hypothesis_with_eval (server.cpp:1384)."""
        g1, g2, av, avg = self.graspPoint1, self.graspPoint2, self.approachVector, self.averagedGraspPoint
        vals = [self.eval, *g1, *g2, *av, *avg]
        return " ".join("%g" % v for v in vals) + " %d" % int(round(np.degrees(self.roll) / roll_step_deg) * roll_step_deg)


class CalcGraspPointsServer:
    """Stands where CCalc_Grasppoints stands: construct once with the three data files (the ROS params of
    server.cpp:217-225), then execute(goal) per GraspInput.  No ROS here: the catkin shim that forwards the real
    action to the C-ABI is shown in INTEGRATION.md."""

    def __init__(self, feature_file_path, range_file_path, svmmodel_file_path, nr_features_without_shaf=302,
                 svm_with_probability=False, **cfg):
        if svm_with_probability:                     # the literal `false` of server.cpp:383, as a parameter (HAF_FLAG_PROBABILITY)
            cfg["flags"] = cfg.get("flags", 0) | capi.FLAG_PROBABILITY
        self.engine = capi.Engine(feature_file_path, range_file_path, svmmodel_file_path,
                                  nr_features_without_shaf=nr_features_without_shaf, **cfg)
        self.base_frame_id = "/base_link"            # server.cpp:294-301

    def execute(self, goal: GraspInputMsg) -> GraspOutputMsg:
        if goal.goal_frame_id:
            self.base_frame_id = goal.goal_frame_id
        out = self.engine.score(np.asarray(goal.input_pc, dtype=np.float32), goal.to_c())
        return GraspOutputMsg(self.base_frame_id, out["eval"], out["grasp_point1"], out["grasp_point2"],
                              out["averaged_grasp_point"], out["approach_vector"], out["roll"])

    def execute_frame(self, goal: GraspInputMsg, frame, roi_mask=None) -> GraspOutputMsg:
        """execute() for a goal whose cloud is still what the sensor delivered: `frame` is a capi.depth_frame (a 16UC1 / 32FC1 depth
        image with the camera's K and the sensor-to-base transform) or a capi.xyz_frame (an organised cloud in the sensor frame);
        goal.input_pc is not read.  The engine deprojects and transforms on the device (haf_score_frames): the step the reference does
        with pcl_ros::transformPointCloud before the hot path (server.cpp:307-316).  top_grasps() works afterwards as after execute().
        roi_mask: uint8 [height, width] (e.g. a segmenter's instance mask synchronised with the depth topic), or (device_ptr,
        row_stride_bytes): the whole frame still builds the scene, but only the cells near the cells of the masked pixels are scored
        and the result is the best grasp there (haf_score_frames_roi); top_grasps(), grasp_map() and best_in_mask() then answer for
        the restricted request."""
        if goal.goal_frame_id:
            self.base_frame_id = goal.goal_frame_id
        if roi_mask is not None:
            out = self.engine.score_frames_roi([frame], [roi_mask], [goal.to_c()])[0]
        else:
            out = self.engine.score_frames([frame], [goal.to_c()])[0]
        return GraspOutputMsg(self.base_frame_id, out["eval"], out["grasp_point1"], out["grasp_point2"],
                              out["averaged_grasp_point"], out["approach_vector"], out["roll"])

    def execute_frame_filtered(self, goal: GraspInputMsg, frames, params=None, roi_mask=None) -> GraspOutputMsg:
        """execute_frame() on the conditioned image of `frames`: 1..capi.MAX_STACK capi.depth_frame exposures of one depth camera in
        one pose (N synchronised depth messages of a static scene).  The engine takes, per pixel, the lower median of the valid samples
        and drops every pixel that too few of its neighbours support (haf_filter_depth; params: a capi.depth_filter(), default the
        library's); the filtered image stays on the device and is scored from there.  self.last_filter_stats = [pixels, valid after
        the temporal stage, kept]."""
        frame, self.last_filter_stats = self.engine.filter_depth(frames, params)
        return self.execute_frame(goal, frame, roi_mask=roi_mask)

    def execute_views(self, goal: GraspInputMsg, frames, roi_masks=None) -> GraspOutputMsg:
        """execute_frame() for a goal seen by several sensors, or by one sensor from several poses: `frames` is a list of up to
        capi.MAX_VIEWS capi.depth_frame / capi.xyz_frame, each with its own intrinsics and sensor-to-base transform.  The engine fuses
        the valid points of all of them into one cloud on the device (haf_score_views); the result is execute()'s on
        capi.view_points(frames).
        roi_masks: one entry per frame -- a mask as execute_frame() takes it, or None for a camera without a segmenter: every view
        still builds the scene, but only the cells near the cells of the masked pixels of the masked views are scored
        (haf_score_views_roi), and what follows answers for the restricted request."""
        if goal.goal_frame_id:
            self.base_frame_id = goal.goal_frame_id
        if roi_masks is not None:
            out = self.engine.score_views_roi([list(frames)], [list(roi_masks)], [goal.to_c()])[0][0]
        else:
            out = self.engine.score_views([list(frames)], [goal.to_c()])[0][0]
        return GraspOutputMsg(self.base_frame_id, out["eval"], out["grasp_point1"], out["grasp_point2"],
                              out["averaged_grasp_point"], out["approach_vector"], out["roll"])

    def top_grasps(self, k=None, **params):
        """Ranked top-k grasp candidates of the last execute() (haf_top_grasps: in-roll and cross-roll suppression, rank 1 = the
        result execute() returned when show_only_best_grasp is off) as GraspOutputMsgs, best first.  params: min_vote, cell_radius,
        roll_window, min_dist_m (haf_top_params)."""
        if k is not None:
            params["k"] = k
        cands = self.engine.top_grasps(**params)[0]
        return [GraspOutputMsg(self.base_frame_id, c["eval"], c["grasp_point1"], c["grasp_point2"], c["averaged_grasp_point"],
                               c["approach_vector"], c["roll"]) for c in cands]

    def free_grasps(self, frame, k=None, gripper=None, mask=None, **top_params):
        """The ranked candidates of the last execute*() at which the gripper FITS (haf_check_grasps on haf_top_grasps' output): the
        scene's points in `frame` (any Frame, e.g. the one just scored; capi.cloud_frame(xyz) for a cloud) are counted inside the boxes of
        one parallel-jaw gripper (capi.gripper(...); the default is a nominal figure, no real gripper's) placed at every candidate, and
        those with no point in the fingers or the palm and at least one between the fingers are returned as (GraspOutputMsg, clearance)
        pairs, best first; clearance: one capi.CLEARANCE_DTYPE record (counts, width_m, offset_m, top_m).  mask: uint8 [height, width]
        or (device_ptr, row_stride_bytes), a non-zero byte admits the pixel -- e.g. to keep the robot's own arm out.  top_params: min_vote,
        cell_radius, roll_window, min_dist_m (haf_top_params).  The ranking itself is top_grasps()', unchanged."""
        if k is not None:
            top_params["k"] = k
        cands = self.engine.top_grasps(**top_params)[0]
        if not cands:
            return []
        rows, order = self.engine.check_grasps(frame, cands, gripper, mask)
        return [(GraspOutputMsg(self.base_frame_id, cands[i]["eval"], cands[i]["grasp_point1"], cands[i]["grasp_point2"],
                                cands[i]["averaged_grasp_point"], cands[i]["approach_vector"], cands[i]["roll"]), rows[i].copy()) for i in order]

    def fitted_grasps(self, frame, k=None, gripper=None, params=None, mask=None, **top_params):
        """The ranked candidates of the last execute*() for which SOME opening of the gripper fits (haf_fit_openings on haf_top_grasps'
        output): per candidate the smallest free opening between params.min_opening and params.max_opening, the gripper moved sideways
        by at most params.max_shift (capi.opening_params(...); the gripper's own opening is not read).  The found ones are returned
        as (GraspOutputMsg, opening) pairs, best first: the message carries the APPLIED opening -- averaged_grasp_point moved by shift_m
        along the closing axis, the grasp points opening_m apart about it (capi.apply_opening) --, opening is one capi.OPENING_DTYPE
        record.  frame, mask and top_params as free_grasps takes them; the ranking itself is top_grasps()', unchanged."""
        if k is not None:
            top_params["k"] = k
        cands = self.engine.top_grasps(**top_params)[0]
        if not cands:
            return []
        rows, order, _ = self.engine.fit_openings(frame, cands, gripper, params, mask)
        out = []
        for i in order:
            g = capi.apply_opening(cands[i], rows[i])
            out.append((GraspOutputMsg(self.base_frame_id, g["eval"], g["grasp_point1"], g["grasp_point2"], g["averaged_grasp_point"],
                                       g["approach_vector"], g["roll"]), rows[i].copy()))
        return out

    def seen_free_grasps(self, frames, k=None, gripper=None, params=None, **top_params):
        """The ranked candidates of the last execute*() whose gripper volume the cameras have SEEN to be empty (haf_check_space on
        haf_top_grasps' output): a lattice of sample points inside the gripper's boxes at every candidate is classified against 1..8
        depth views `frames` (a capi.depth_frame or a list of them: the scored view, a second camera) as unseen, hidden, free or hit,
        and the candidates with clear == 1 -- by params (capi.space_params(...)): at most max_hit hit and max_unknown hidden or unseen
        samples in the fingers and the palm, at least min_between_hit hit samples between the fingers -- are returned as
        (GraspOutputMsg, space) pairs, best first; space: one capi.SPACE_DTYPE record.  Where free_grasps counts no point and says
        "free" -- behind an object, under an overhang -- this says "not seen".  top_params as free_grasps takes them; the ranking itself
        is top_grasps()', unchanged."""
        if k is not None:
            top_params["k"] = k
        cands = self.engine.top_grasps(**top_params)[0]
        if not cands:
            return []
        rows, order, _ = self.engine.check_space(frames, cands, gripper, params)
        return [(GraspOutputMsg(self.base_frame_id, cands[i]["eval"], cands[i]["grasp_point1"], cands[i]["grasp_point2"],
                                cands[i]["averaged_grasp_point"], cands[i]["approach_vector"], cands[i]["roll"]), rows[i].copy()) for i in order]

    def grasp_map(self, frame, want=("vote", "roll")):
        """The last execute*()'s votes in the pixels of `frame` (haf_grasp_map): any capi.depth_frame / capi.xyz_frame -- the scored
        view, another camera, the registered RGB view -- -> dict of [height, width] images: vote int16 (capi.MAP_NO_CELL where no roll
        has a cell for the pixel), roll int16 (the winning roll, -1), cell int32 when asked for."""
        return self.engine.grasp_map(0, frame, want=want)

    def best_in_mask(self, frame, mask=None, min_vote=1):
        """The best grasp of the last execute*() inside an image-space mask (uint8 [height, width], e.g. a segmenter's instance mask
        synchronised with the depth topic; None: the whole image) -> (GraspOutputMsg, u, v) of the best pixel, or None when no pixel
        under the mask has a vote >= min_vote (haf_grasp_map_best)."""
        hit = self.engine.best_in_mask(0, frame, mask, min_vote)
        if hit is None:
            return None
        c, u, v = hit
        return GraspOutputMsg(self.base_frame_id, c["eval"], c["grasp_point1"], c["grasp_point2"], c["averaged_grasp_point"],
                              c["approach_vector"], c["roll"]), u, v

    def best_per_object(self, frame, labels, min_vote=1, n_labels=None):
        """The best grasp of the last execute*() for every object of an instance-label image (uint8 / uint16 [height, width]: 0
        background, 1.. the instances; e.g. a segmenter's output synchronised with the depth topic) in one device pass
        (haf_grasp_map_labels) -> list of (label, GraspOutputMsg, u, v) for the objects that have a pixel with a vote >= min_vote,
        best first: what best_in_mask(frame, labels == label) gives for each, ranked."""
        res = self.engine.best_per_label(0, frame, labels, n_labels=n_labels, min_vote=min_vote)
        out = []
        for label in res["order"]:
            c, p = res["poses"][label - 1], res["picks"][label - 1]
            out.append((label, GraspOutputMsg(self.base_frame_id, c["eval"], c["grasp_point1"], c["grasp_point2"], c["averaged_grasp_point"],
                                              c["approach_vector"], c["roll"]), int(p["u"]), int(p["v"])))
        return out

    def execute_frame_objects(self, goal: GraspInputMsg, frame, labels, min_vote=1):
        """execute_frame() with roi_mask = (labels != 0), then best_per_object(): only the cells near the labelled pixels' cells are
        scored, and every object gets its own best grasp -> (GraspOutputMsg of the request, best_per_object()'s list).  labels: a host
        uint8 / uint16 [height, width] array."""
        lab = np.asarray(labels)
        res = self.execute_frame(goal, frame, roi_mask=(lab != 0).astype(np.uint8))
        return res, self.best_per_object(frame, lab, min_vote=min_vote)

    @staticmethod
    def segment_params_from_goal(goal: GraspInputMsg, **kw):
        """capi.segment_params() whose support plane is the plane through the goal's grasp area centre c with the goal's unit approach
        vector n as its normal: plane = (n, -n.c), so a point's height is its distance from that plane along the approach direction.
        THE CALLER OWNS THE TABLE HEIGHT: the centre of the grasp area must lie on the support surface (or min_height must make up for
        it).  kw: the other fields (min_height, max_height, max_gap, min_pixels, max_labels) over the library's defaults."""
        n = np.asarray(goal.approach_vector, np.float64)
        n = n / np.linalg.norm(n) if np.linalg.norm(n) > 0 else np.array([0.0, 0.0, 1.0])
        c = np.asarray(goal.grasp_area_center, np.float64)
        return capi.segment_params(plane=[n[0], n[1], n[2], -float(n @ c)], **kw)

    def execute_frame_segmented(self, goal: GraspInputMsg, frame, params=None, min_vote=1, plane=None):
        """execute_frame_objects() without a segmenter: the frame is clustered into objects on the device (haf_segment_frame: geometric
        tabletop clustering -- a height band over the support plane, 4-neighbours closer than max_gap are one object; touching objects
        are one object), the request is scored under that image as the device mask (haf_score_frames_roi) and every object gets its own
        best grasp from the same device image (haf_grasp_map_labels); the label image never leaves the device
        -> (GraspOutputMsg of the request, best_per_object()'s list).  params: a capi.segment_params(); None:
        segment_params_from_goal(goal), whose plane passes through the goal's grasp area centre -- the caller owns the table height,
        unless plane="fit" takes it from the frame.
        self.last_segment_infos / self.last_segment_stats: the objects' pixel counts, anchors and boxes, and [pixels, foreground,
        components, components that pass the size rule].
        plane: None -- the plane of `params` as it stands; "fit" or a capi.plane_params() -- the frame's dominant plane, fitted on the
        device (haf_fit_plane) with the library's defaults or with those parameters, replaces it when one is found (else the plane of
        `params` stays: the fall-back).  self.last_plane_fit: that fit's dict, None without one."""
        p = params if params is not None else self.segment_params_from_goal(goal)
        self.last_plane_fit = None
        if plane is not None:
            if isinstance(plane, str) and plane != "fit":
                raise ValueError("plane: None, \"fit\" or a capi.plane_params()")
            self.last_plane_fit = self.engine.fit_plane(frame, None if isinstance(plane, str) else plane)
            if self.last_plane_fit["found"]:
                p = capi.SegmentParams.from_buffer_copy(p)
                p.plane = (C.c_float * 4)(*self.last_plane_fit["plane"])
        img, self.last_segment_infos, self.last_segment_stats = self.engine.segment(frame, p, np.uint8, device_out=True)
        res = self.execute_frame(goal, frame, roi_mask=(img.data, img.row_stride_bytes))
        n = len(self.last_segment_infos)
        return res, (self.best_per_object(frame, img, min_vote=min_vote, n_labels=n) if n else [])

    @staticmethod
    def cell_segment_params_from_goal(goal: GraspInputMsg, **kw):
        """capi.cell_segment_params() with segment_params_from_goal()'s support plane; kw: the other fields over the library's defaults"""
        return capi.cell_segment_params(plane=list(CalcGraspPointsServer.segment_params_from_goal(goal).plane), **kw)

    def execute_frame_per_object(self, goal: GraspInputMsg, frame, params=None, plane=None, min_vote=1, margin_cells=4, fused=False,
                                 segmenter="pixels"):
        """execute_frame_segmented() for objects ANYWHERE in the frame: one request per object, each centred on its object, instead of
        the one grid around the goal's grasp_area_center (objects outside that grid have no grasp there: no height grid contains
        them).  The frame is segmented into the engine's device image (params, plane: as execute_frame_segmented takes them), every
        label's box in the base frame is measured from that image (haf_measure_labels, heights over the segmentation's plane), every
        found object gets the goal re-centred on its box with a square grasp area that covers it and margin_cells more
        (haf_object_input; the goal keeps its z, approach vector and every other field), and the requests are scored in chunks that
        respect max_clouds and max_points -- each chunk ONE haf_score_frames_roi call whose requests share the frame and the device
        mask -- followed by one haf_grasp_map_labels call per request, of which only the entry of that request's object is read.
        -> list of (label, GraspOutputMsg, u, v, shape dict, fits), best first in haf_grasp_map_labels' order (vote descending, then
        roll, then pixel index ascending); objects without a pixel of vote >= min_vote are left out.  fits is False when the grasp
        area had to be cut to the engine's grid.  self.last_shapes: the capi.LABEL_SHAPE_DTYPE array of all labels; the other last_*
        attributes as execute_frame_segmented leaves them.
        THE COST of that route: a host frame is staged and deprojected once per request of a chunk (a device-resident frame is read
        where it lies, and still deprojected per request), every request marks the cells of all objects, and there is one label call
        per object.
        fused=True: the same list from ONE haf_score_objects call per chunk of max_clouds objects -- the frame is staged and
        deprojected once per chunk and counts once against max_points (the chunk rule has no max_points term), request b marks and
        evaluates only the cells near its own object (mask `labels == label`; the picks are those of `labels != 0`, include/hafgrasp.h),
        and one label pass serves the chunk.
        segmenter="cells": the objects come from haf_segment_cells -- connected occupied cells of the top-down grid instead of
        neighbouring pixels, so an object cut in two in the image stays one object and the frame may have any shape (an N x 1 cloud:
        execute_cloud_per_object).  params is then a capi.cell_segment_params() (None: cell_segment_params_from_goal(goal)), and
        self.last_segment_infos / self.last_segment_stats are that call's."""
        if segmenter not in ("pixels", "cells"):
            raise ValueError("segmenter: \"pixels\" or \"cells\"")
        cells = segmenter == "cells"
        if goal.goal_frame_id:
            self.base_frame_id = goal.goal_frame_id
        if params is not None:
            p = params
        else:
            p = self.cell_segment_params_from_goal(goal) if cells else self.segment_params_from_goal(goal)
        self.last_plane_fit = None
        if plane is not None:
            if isinstance(plane, str) and plane != "fit":
                raise ValueError("plane: None, \"fit\" or a capi.plane_params()")
            self.last_plane_fit = self.engine.fit_plane(frame, None if isinstance(plane, str) else plane)
            if self.last_plane_fit["found"]:
                p = type(p).from_buffer_copy(p)
                p.plane = (C.c_float * 4)(*self.last_plane_fit["plane"])
        segment = self.engine.segment_cells if cells else self.engine.segment
        img, self.last_segment_infos, self.last_segment_stats = segment(frame, p, np.uint8, device_out=True)
        n = len(self.last_segment_infos)
        self.last_shapes = np.zeros(0, capi.LABEL_SHAPE_DTYPE)
        if not n:
            return []
        self.last_shapes = self.engine.measure_labels(frame, img, n_labels=n, plane=list(p.plane))
        cfg, base = self.engine.cfg, goal.to_c()
        todo = [(l + 1,) + capi.object_input(cfg, base, self.last_shapes[l], margin_cells) for l in range(n) if self.last_shapes["found"][l]]
        hits = []

        def hit(label, fits, pick, c):
            msg = GraspOutputMsg(self.base_frame_id, c["eval"], c["grasp_point1"], c["grasp_point2"], c["averaged_grasp_point"],
                                 c["approach_vector"], c["roll"])
            key = (-int(pick["vote"]), int(pick["roll"]), int(pick["v"]) * frame.width + int(pick["u"]))
            hits.append((key, (label, msg, int(pick["u"]), int(pick["v"]), capi.shape_to_dict(self.last_shapes[label - 1]), fits)))

        if fused:
            chunk = max(1, int(cfg.max_clouds))
            for c0 in range(0, len(todo), chunk):
                part = todo[c0:c0 + chunk]
                _, picks, poses, _ = self.engine.score_objects(frame, img, n, [label for label, _, _ in part], [inp for _, inp, _ in part],
                                                               min_vote=min_vote)
                for b, (label, _, fits) in enumerate(part):
                    if picks["found"][b]:
                        hit(label, fits, picks[b], poses[b])
            return [h for _, h in sorted(hits, key=lambda kh: kh[0])]
        chunk = max(1, min(int(cfg.max_clouds), int(cfg.max_points) // max(1, frame.width * frame.height)))
        mask = (img.data, img.row_stride_bytes)
        for c0 in range(0, len(todo), chunk):
            part = todo[c0:c0 + chunk]
            self.engine.score_frames_roi([frame] * len(part), [mask] * len(part), [inp for _, inp, _ in part])
            for b, (label, _, fits) in enumerate(part):
                res = self.engine.best_per_label(b, frame, img, n_labels=n, min_vote=min_vote)
                pick, c = res["picks"][label - 1], res["poses"][label - 1]
                if pick["found"]:
                    hit(label, fits, pick, c)
        return [h for _, h in sorted(hits, key=lambda kh: kh[0])]

    def execute_cloud_per_object(self, goal: GraspInputMsg, xyz, params=None, plane=None, min_vote=1, margin_cells=4):
        """execute_frame_per_object() for an UNORGANISED base-frame cloud (float32 [N, >= 3]: a PointCloud2 goal's points), which has no
        image for haf_segment_frame: the cloud is wrapped as an N x 1 XYZ frame under the identity pose (capi.cloud_frame), clustered
        by haf_segment_cells, and measured and scored as a frame is -- haf_measure_labels, haf_object_input, one haf_score_objects
        call per chunk of max_clouds objects.  params: a capi.cell_segment_params(); plane: as execute_frame_segmented takes it.
        -> the list execute_frame_per_object gives, with u = the index of the pick's point in `xyz` and v = 0."""
        frame = capi.cloud_frame(np.ascontiguousarray(xyz, np.float32))
        return self.execute_frame_per_object(goal, frame, params=params, plane=plane, min_vote=min_vote, margin_cells=margin_cells, fused=True,
                                             segmenter="cells")

    def execute_frame_labelled(self, goal: GraspInputMsg, frame, camera, cam_labels, n_labels=None, params=None, plane=None, min_vote=1,
                               margin_cells=4):
        """execute_frame_per_object(fused=True) with the objects of a LEARNED instance segmenter in place of the engine's own: cam_labels
        is the label image of another camera (the colour camera the segmenter ran on; `camera`: a capi.camera() with that camera's
        intrinsics and its base -> camera transform, cam_labels: what capi.label_image() takes, n_labels: its largest label).  The
        image is carried over to the depth frame's pixels behind a z-buffer (haf_transfer_labels; params: a capi.transfer_params()) into
        the engine's device image; from there the chain is the fused one: haf_measure_labels, haf_object_input per found object, one
        haf_score_objects call per chunk of max_clouds objects.  plane: None (the shapes carry no height), four floats, "fit" or a
        capi.plane_params() (haf_fit_plane on the frame; without a plane found, no height).
        -> the list execute_frame_per_object gives.  self.last_transfer_stats: [pixels, in front of the camera, projecting, visible,
        labelled]; self.last_shapes and self.last_plane_fit as execute_frame_per_object leaves them."""
        if goal.goal_frame_id:
            self.base_frame_id = goal.goal_frame_id
        _, n = capi.label_image(cam_labels, camera, n_labels)
        self.last_plane_fit = None
        if isinstance(plane, str) and plane != "fit":
            raise ValueError("plane: None, four floats, \"fit\" or a capi.plane_params()")
        if isinstance(plane, (str, capi.PlaneParams)):
            self.last_plane_fit = self.engine.fit_plane(frame, None if isinstance(plane, str) else plane)
            plane = list(self.last_plane_fit["plane"]) if self.last_plane_fit["found"] else None
        img, self.last_transfer_stats = self.engine.transfer_labels(frame, camera, cam_labels, n, params, np.uint8 if n <= 255 else np.uint16,
                                                                    device_out=True)
        self.last_shapes = self.engine.measure_labels(frame, img, n_labels=n, plane=plane)
        cfg, base = self.engine.cfg, goal.to_c()
        todo = [(l + 1,) + capi.object_input(cfg, base, self.last_shapes[l], margin_cells) for l in range(n) if self.last_shapes["found"][l]]
        hits = []
        chunk = max(1, int(cfg.max_clouds))
        for c0 in range(0, len(todo), chunk):
            part = todo[c0:c0 + chunk]
            _, picks, poses, _ = self.engine.score_objects(frame, img, n, [label for label, _, _ in part], [inp for _, inp, _ in part],
                                                           min_vote=min_vote)
            for b, (label, _, fits) in enumerate(part):
                if picks["found"][b]:
                    pick, c = picks[b], poses[b]
                    msg = GraspOutputMsg(self.base_frame_id, c["eval"], c["grasp_point1"], c["grasp_point2"], c["averaged_grasp_point"],
                                         c["approach_vector"], c["roll"])
                    key = (-int(pick["vote"]), int(pick["roll"]), int(pick["v"]) * frame.width + int(pick["u"]))
                    hits.append((key, (label, msg, int(pick["u"]), int(pick["v"]), capi.shape_to_dict(self.last_shapes[label - 1]), fits)))
        return [h for _, h in sorted(hits, key=lambda kh: kh[0])]

    def close(self):
        self.engine.close()
