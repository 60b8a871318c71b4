"""The engines whose model tables tests/golden/table_digests.json holds digests of (test_tables_gpu.py, test_tables_cpu.py; data only).

Every case runs in the testing library with HAF_KAPPA=12 (the measured matrix-core constant differs from card to card) and
HAF_NO_CALIBRATE=1 (calibration may switch screen_active by what it measures; the digests are of the table work alone), on the
golden Features.txt and range file."""
import contextlib
import ctypes as C
import json
import os

import models
from haf_grasping_amd import capi

KTILE = 32                      # csrc/kernels.h: kTile
FIXTURE = "table_digests.json"
BASE_ENV = {"HAF_KAPPA": "12", "HAF_NO_CALIBRATE": "1"}
# every switch that the table work reads (csrc/model_tables.h: TableSwitches) or that haf_create reads on the way to it
KNOBS = ("HAF_KAPPA", "HAF_NO_CALIBRATE", "HAF_NO_CR", "HAF_NO_LR", "HAF_CR_NO_CENTRE", "HAF_NO_CR_T1", "HAF_NO_I8", "HAF_NO_FAST_GROUPS",
         "HAF_SCREEN_NO_CENTRE", "HAF_LR_UNFUSED", "HAF_NO_LR_PLAIN", "HAF_KAPPA_T1_MEASURED", "HAF_GUARD_REL", "HAF_GUARD0_REL",
         "HAF_GUARD2_REL", "HAF_GUARD_I8_REL", "HAF_PROB_HOST_ALL", "HAF_HOST_EXP_ALL")

# name -> (model, flags, grid, extra environment)
CASES = {
    "a": ("surrogate", 0, 56, {}),
    "b": ("clustered", 0, 96, {}),
    "c": ("clustered", 0, 96, {"HAF_NO_LR": "1"}),
    "d": ("clustered", 0, 96, {"HAF_CR_NO_CENTRE": "1"}),
    "e": ("surrogate", capi.FLAG_SPLIT_F16, 56, {}),
    "f": ("surrogate", capi.FLAG_FP32_MFMA, 56, {}),
    "g": ("heart_prob", capi.FLAG_PROBABILITY, 56, {}),
    "h": ("ragged", 0, 56, {}),
    "i": ("surrogate", 0, 56, {"HAF_GUARD0_REL": "2", "HAF_GUARD_REL": "2"}),
}


def files(data_dir):
    return os.path.join(data_dir, "Features.txt"), os.path.join(data_dir, "range21062012_allfeatures")


def model_path(kind, golden_dir, tmp_dir):
    if kind == "surrogate":
        return os.path.join(golden_dir, "surrogate.model")
    if kind == "heart_prob":
        return os.path.join(golden_dir, "heart_scale_prob.model")
    path = os.path.join(str(tmp_dir), kind + ".model")
    if not os.path.exists(path):
        if kind == "clustered":
            models.write_clustered_model(path, 260, seed=5)
        elif kind == "ragged":
            models.write_random_model(path, 2 * KTILE + 3, balanced=True, density=0.5)
        else:
            raise KeyError(kind)
    return path


@contextlib.contextmanager
def case_env(extra):
    """The environment of one case: BASE_ENV and `extra`, none of the other switches; put back afterwards."""
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(BASE_ENV)
        os.environ.update(extra)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def parse(text):
    return dict(line.split("=", 1) for line in text.strip().splitlines())


def device_digests(name, data_dir, golden_dir, tmp_dir):
    """Creates the engine of case `name` (a GPU) and returns {table / struct / "scalars": 16 hex digits} of haf_test_table_digest."""
    kind, flags, grid, extra = CASES[name]
    f, r = files(data_dir)
    with case_env(extra):
        eng = capi.Engine(f, r, model_path(kind, golden_dir, tmp_dir), testing=True, flags=flags, grid_h=grid, grid_w=grid)
        try:
            buf = C.create_string_buffer(8192)
            rc = capi.testlib().haf_test_table_digest(eng._h, buf, len(buf))
            assert rc == 0, rc
            return parse(buf.value.decode())
        finally:
            eng.close()


def host_build(feature_file, range_file, model_file, flags=0, grid=56, kappa=12.0, kappa16=12.0, **cfg):
    """The device-free builder (haf_test_host_table_digest) on these files under the current environment -> (code, digests or
    None, the refusal's text)"""
    c = capi.default_config(feature_file=feature_file, range_file=range_file, model_file=model_file, flags=flags, grid_h=grid, grid_w=grid,
                            **cfg)
    buf, msg = C.create_string_buffer(8192), C.create_string_buffer(512)
    rc = capi.testlib().haf_test_host_table_digest(C.byref(c), kappa, kappa16, buf, len(buf), msg, len(msg))
    return rc, (parse(buf.value.decode()) if rc == 0 else None), msg.value.decode()


def host_digests(name, data_dir, golden_dir, tmp_dir):
    """Case `name` through the device-free builder: no GPU.  The kappas are the 12 that HAF_KAPPA=12 gives the engine."""
    kind, flags, grid, extra = CASES[name]
    f, r = files(data_dir)
    with case_env(extra):
        rc, got, msg = host_build(f, r, model_path(kind, golden_dir, tmp_dir), flags=flags, grid=grid)
    assert rc == 0, (rc, msg)
    return got


def load_fixture(golden_dir):
    with open(os.path.join(golden_dir, FIXTURE)) as fh:
        return json.load(fh)
