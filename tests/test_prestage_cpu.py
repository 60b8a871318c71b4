"""The cases of prestage_cases are what they claim -- every condition here is a condition on the REFERENCE alone, checked without a device,
and has to hold before tests/test_prestage_gpu.py means anything: the numpy mirror equals the oracle's stage functions word for word on
every case, the hostile clouds are hostile in the way their names say, and the mirror of the launchers' thresholds sends the case list
through every form of the binning and of the integral image."""
import numpy as np
import pytest

import prestage_cases as pc

U32 = np.uint32


def _named(H, name):
    return next(c for c in pc.cases(H) if c[0] == name)


@pytest.mark.parametrize("H", pc.SIZES)
def test_mirror_equals_the_oracle_word_for_word(H):
    """binning (float32, left to right, unfused; max per cell; < -0.99 -> 0) and the integral image (float64 running row sum plus the row
    above, narrowed to float32) restated in numpy give the words of hafo_height_grid and hafo_integral, on every cloud and roll"""
    for case in pc.cases(H):
        name, _, cfg_kw, in_kw, clouds, rolls = case
        ref = pc.case_reference(case)
        for b, cloud in enumerate(clouds):
            r = ref["per_cloud"][b]
            for k in range(rolls[1]):
                h = pc.mirror_heights(cloud, r["M"][k], H)
                assert (h.view(U32) == r["heights"][k].view(U32)).all(), (name, b, k, "heights")
                assert (pc.mirror_integral(h).view(U32) == r["integral"][k].view(U32)).all(), (name, b, k, "integral")


@pytest.mark.parametrize("H", pc.SIZES)
def test_every_roll_has_a_mask(H):
    """... except where emptiness is the point: the empty cloud of uneven_batch"""
    for case in pc.cases(H):
        masks = pc.case_reference(case)["masks"]
        for b, cloud in enumerate(case[4]):
            for k in range(case[5][1]):
                assert (masks[b, k].sum() > 0) == (len(cloud) > 0), (case[0], b, k)


@pytest.mark.parametrize("H", [56, 63, 70, 128, 129, 192, 576])
def test_borders_lie_on_borders(H):
    """for at least a quarter of the cloud's points, under at least one roll, 100 * (p + r) evaluated in float32 is within 2 ulps of an
    integer in one of its two coordinates; and some point sits within 2 ulps of the outermost border on either side"""
    case = _named(H, "borders")
    cloud, r = case[4][0], pc.half(H)
    ref = pc.case_reference(case)["per_cloud"][0]
    near = np.zeros(len(cloud), bool)
    outer = [False, False]
    for k in range(case[5][1]):
        px, py, _ = pc.mirror_points(cloud, ref["M"][k])
        for p in (px, py):
            v = np.float32(100) * (p + r)
            assert v.dtype == np.float32
            near |= np.abs(v - np.rint(v)) <= 2 * np.spacing(np.abs(v))
            outer[0] |= bool((np.abs(v) <= 2 * np.spacing(np.float32(1))).any())
            outer[1] |= bool((np.abs(v - np.float32(H)) <= 2 * np.spacing(np.float32(H))).any())
    assert near.mean() >= 0.25, near.mean()
    assert all(outer)


@pytest.mark.parametrize("H", [56, 71, 128, 192, 576, 601, 1100])
def test_one_cell_and_one_bucket_are_one_bucket(H):
    """every one of the 40 000 points lies in one bucket by the rule of point_bucket; one_cell's also in one cell at roll 0"""
    for name in ("one_cell", "one_bucket"):
        found = [c for c in pc.cases(H) if c[0] == name]
        for case in found:
            cloud = case[4][0][:40000]
            m0 = pc.transform(case[2], dict(case[3], gripper_opening_width=1), 0)
            q = pc.mirror_bucket(cloud, H, m0)
            assert q.min() >= 0 and (q == q[0]).all(), (name, np.unique(q))
            if name == "one_cell":
                _, ix, iy, _ = pc.mirror_cells(cloud, pc.transform(case[2], case[3], 0), H)
                assert ix.size == 40000 and (ix == ix[0]).all() and (iy == iy[0]).all()
    assert any(c[0] in ("one_cell", "one_bucket") for c in pc.cases(H))


@pytest.mark.parametrize("H", [56, 128, 192, 576])
def test_row_counts_hold_the_edges(H):
    """the oracle's mask of roll 0 has rows of exactly every target count the grid has room for (all of 0, 1, 63, 64, 65, 127, 128, 129 from
    192 cells on), and an empty row on either side of each"""
    case = _named(H, "row_counts")
    cnt = pc.case_reference(case)["masks"][0, 0].sum(axis=1)
    targets = pc.row_count_targets(H)
    if H >= 192:
        assert tuple(targets) == pc.ROW_TARGETS
    assert {0, *targets} <= set(cnt.tolist()), sorted(set(cnt.tolist()))
    for t in targets:
        i = int(np.flatnonzero(cnt == t)[0])
        assert cnt[i - 1] == 0 and cnt[i + 1] == 0, (t, i)


@pytest.mark.parametrize("H", [56, 64, 128, 192, 576])
def test_negatives_are_negative(H):
    """some cell ends in (-0.99, 0), some cell that received points is cleared by the -0.99 rule, -inf and -1e30 are in the cloud, and
    a cell's maximum is an exact duplicate"""
    case = _named(H, "negatives")
    cloud = case[4][0]
    ref = pc.case_reference(case)["per_cloud"][0]
    assert np.isneginf(cloud[:, 2]).any() and (cloud[:, 2] == np.float32(-1e30)).any()
    assert len(np.unique(cloud[-900:], axis=0)) == 300
    for k in range(case[5][1]):
        h = ref["heights"][k]
        raw = pc.mirror_heights(cloud, ref["M"][k], H, raw=True)
        assert ((h > -0.99) & (h < 0)).any(), k
        _, ix, iy, _ = pc.mirror_cells(cloud, ref["M"][k], H)
        hit = np.zeros((H, H), bool)
        hit[ix, iy] = True
        assert (hit & (raw.astype(np.float64) < -0.99) & (raw != -1) & (h == 0)).any(), k
        assert (h == np.float32(0.5 + pc.Z_SHIFT)).any() or k > 0


@pytest.mark.parametrize("H", [56, 128, 192, 576])
def test_far_centre_lands_in_the_grid(H):
    case = _named(H, "far_centre")
    cloud = case[4][0]
    assert np.abs(cloud[:, 0]).min() > 30 and np.abs(cloud[:, 1]).min() > 20
    ref = pc.case_reference(case)["per_cloud"][0]
    for k in range(case[5][1]):
        assert pc.mirror_cells(cloud, ref["M"][k], H)[0].size > len(cloud) // 2, k


def test_bad_values_are_bad():
    for s in (4, 8):
        cloud = _named(192, "bad_values_s%d" % s)[4][0]
        assert cloud.shape[1] == s and np.isnan(cloud[:, 3:]).all()
        for c in range(3):
            assert np.isnan(cloud[:, c]).sum() == 100
        for c in range(2):
            assert np.isposinf(cloud[:, c]).sum() == 50 and np.isneginf(cloud[:, c]).sum() == 50


def test_eval_list_definition():
    """rows of 0, 1, 63, 64, 65 and 129 cells on two grids: whole chunks of all rows first, a row's remainder from the row's start"""
    m = np.zeros((1, 2, 6, 300), np.uint8)
    for g in range(2):
        for i, n in enumerate((0, 1, 63, 64, 65, 129)):
            m[0, g, i, 3:3 + 2 * n:2] = 1
    lst = pc.eval_list(m)
    assert lst.size == m.sum() and np.unique(lst).size == lst.size and m.reshape(-1)[lst].all()
    n_a = 2 * (64 + 64 + 128)
    a, b = lst[:n_a], lst[n_a:]
    assert (a[:64] == 3 * 300 + 3 + 2 * np.arange(64)).all()                 # row 3 of grid 0: all 64
    assert (a[64:128] == 4 * 300 + 3 + 2 * np.arange(1, 65)).all()           # row 4: its last 64
    assert (a[128:256] == 5 * 300 + 3 + 2 * np.arange(1, 129)).all()
    assert (a[256:320] == (6 + 3) * 300 + 3 + 2 * np.arange(64)).all()       # grid 1 follows
    assert b[0] == 1 * 300 + 3 and (b[1:64] == 2 * 300 + 3 + 2 * np.arange(63)).all() and b[64] == 4 * 300 + 3 and b[65] == 5 * 300 + 3


def test_expected_forms_cover_every_form():
    """the case list runs all five binning forms and all three integral forms; 601 is refused the bucket-sorted path, 576 and 1100 are not;
    the fused kernel ends at 63 and k_integral_small at 70"""
    seen_bin, seen_int = set(), set()
    refused = {}
    for H, case in [(H, c) for H in pc.SIZES for c in pc.cases(H)]:
        f = pc.expected_forms(H, [len(c) for c in case[4]])
        seen_bin.add(f["bin"])
        seen_int.add(f["integral"])
        refused[H] = refused.get(H, False) or f["bucket_refused"]
    assert seen_bin == {0, 1, 2, 3, 4} and seen_int == {0, 1, 2}
    assert refused[601] and not refused[576] and not refused[1100]
    assert [H for H in range(16, 200) if pc.small_pre_lds(H, H) <= pc.LDS_LIMIT][-1] == 63
    assert [H for H in range(16, 200) if pc.integral_small_lds(H, H) <= pc.LDS_LIMIT][-1] == 70
    big = 40000
    assert [pc.expected_forms(H, [big])["bin"] for H in (56, 63, 64, 128, 129, 192, 576, 601, 1100)] == [4, 4, 1, 1, 2, 2, 2, 0, 2]
    assert [pc.expected_forms(H, [1000])["integral"] for H in (63, 64, 70, 71)] == [2, 0, 0, 1]
    assert [pc.expected_forms(128, [n])["bin"] for n in (8191, 8192)] == [0, 1]
    assert [pc.expected_forms(56, [n])["bin"] for n in (16384, 16385)] == [3, 4]
    assert [pc.expected_forms(192, [n])["bin"] for n in (32767, 32768)] == [0, 2]
    # the grid sizes whose bucket grid exceeds the LDS histogram (csrc/prestages.hip: kBktMaxBuckets)
    bad = [H for H in range(129, 4097) if pc.bucket_grid(H)[0] ** 2 + 1 > pc.K_BKT_MAX_BUCKETS]
    assert len(bad) == 718 and bad[0] == 527 and bad[-1] == 2303 and 575 in bad and 576 not in bad and 592 in bad
