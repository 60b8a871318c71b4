"""build.py's checks of the screening feature kernel's slot loop (check_slot_loop), on the cross-compiled library and on listings
written here: no GPU needed."""
import pytest

from haf_grasping_amd import build as b


def test_slot_loop_of_the_built_library_passes_its_guard():
    """k_features_serial<2, true> as built: the loop body of a fast group holds the 64 corner reads of its eight slots, at most
    MAX_SLOT_LOOP_OVERHEAD scalar-side instructions (SALU, s_nop, s_waitcnt) per read -- 3.05 as built, 4.52 before the loop was
    re-scheduled -- and in both screening instances no instruction touches a register of an LDS read or scalar load still in flight."""
    if not b.up_to_date():
        b.build()
    rep = b.check_slot_loop()
    assert rep["reads"] == 64 and rep["block"]["addtid"] == 64, rep
    assert 2.0 < rep["overhead"] <= b.MAX_SLOT_LOOP_OVERHEAD < 4.52, rep
    assert len(rep["inflight"]) == 2 and all(n > 100 and not bad for n, bad in rep["inflight"].values()), rep["inflight"]


def test_guard_refuses_the_old_loop_and_a_touched_register(monkeypatch):
    old = {"block": {"salu": 144, "nop": 116, "wait": 29, "addtid": 64, "valu": 180, "lds": 16, "smem": 24, "branch": 4}, "reads": 64,
           "overhead": (144 + 116 + 29) / 64.0, "inflight": {"a" + b.SLOT_LOOP_AUDITED[0]: (719, []), "a" + b.SLOT_LOOP_AUDITED[1]: (418, [])}}
    monkeypatch.setattr(b, "slot_loop_report", lambda lib=None: old)
    with pytest.raises(RuntimeError, match="per corner read"):
        b.check_slot_loop()
    ok = dict(old, overhead=3.05)
    monkeypatch.setattr(b, "slot_loop_report", lambda lib=None: ok)
    assert b.check_slot_loop() is ok
    touched = dict(ok, inflight={"a": (719, [(7, "s_mov_b32 s4, s12", [("s", 12)])]), "b": (418, [])})
    monkeypatch.setattr(b, "slot_loop_report", lambda lib=None: touched)
    with pytest.raises(RuntimeError, match="in flight"):
        b.check_slot_loop()
    monkeypatch.setattr(b, "slot_loop_report", lambda lib=None: dict(ok, reads=0))
    with pytest.raises(RuntimeError, match="not found"):
        b.check_slot_loop()


def test_inflight_audit_follows_the_lgkm_counter():
    reads = ["s_add_i32 m0, s8, s33", "s_nop 0", "ds_read_addtid_b32 v1", "s_add_i32 m0, s9, s33", "s_nop 0", "ds_read_addtid_b32 v2"]
    # a full wait covers everything
    assert b.inflight_violations(reads + ["s_waitcnt lgkmcnt(0)", "v_sub_f32_e32 v3, v1, v2"]) == (2, [])
    # LDS reads return in order: lgkmcnt(1) covers the first read only
    n, bad = b.inflight_violations(reads + ["s_waitcnt lgkmcnt(1)", "v_mov_b32_e32 v3, v1", "v_mov_b32_e32 v4, v2"])
    assert n == 2 and [(i, r) for i, _, r in bad] == [(8, [("v", 2)])]
    # a scalar load is retired by lgkmcnt(0) only, whatever was issued behind it; its address registers are free at once
    code = ["s_load_dwordx4 s[4:7], s[2:3], 0x20", "s_mov_b32 s2, 0", "ds_read_b64 v[6:7], v0", "s_waitcnt lgkmcnt(1)", "v_mov_b32_e32 v1, s5",
            "s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v1, s5", "v_mov_b32_e32 v2, v7"]
    n, bad = b.inflight_violations(code)
    assert n == 2 and [(i, r) for i, _, r in bad] == [(4, [("s", 5)])]
    # a copy of a register in flight (what a spill or a coalescing copy between the asm statements would be) is reported; a branch ends the search
    assert len(b.inflight_violations(["ds_read_addtid_b32 v9", "v_mov_b32_e32 v10, v9"])[1]) == 1
    assert b.inflight_violations(["ds_read_addtid_b32 v9", "s_cbranch_scc0 L4", "v_mov_b32_e32 v10, v9"])[1] == []
