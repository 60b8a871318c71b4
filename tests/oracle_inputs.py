"""The oracle's request for an engine request given as keywords of haf_grasp_input; shared by the CPU and the GPU tests."""
from oracle import oracle as O


def oracle_input(kw):
    return O.make_input(center=kw.get("grasp_area_center", (0, 0, 0)), length_x=kw.get("grasp_area_length_x", 32),
                        length_y=kw.get("grasp_area_length_y", 44), approach=kw.get("approach_vector", (0, 0, 1)),
                        show_only_best=kw.get("show_only_best_grasp", 0), gripper_width=kw.get("gripper_opening_width", 1))
