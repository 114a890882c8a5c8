"""Host side of the concat forms of the GroupNorm kernels (no GPU): the launch planner is untouched, the new entry points are declared
and exported, they refuse what they cannot run before any launch, and ops.group_norm_act_cat takes its two-step path where it must."""
import ctypes
import os
import re

import pytest
import torch

import gn_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adm_gn_fwd_cat_amax", "adm_gn_bwd_add_cat_amax")


def _lib():
    from adm_amd import hip
    return hip.lib()


@pytest.mark.parametrize("row", gn_cases.GRID, ids=gn_cases.row_id)
def test_plans_are_what_the_grid_says(row):
    """adm_gn_plan answers every row of gn_cases.GRID as before (thread maps, slabs, templates and splits are not touched), and the
    multi-pass query under adm_gn_fused(0) still says Cc = 0."""
    H, W, C, _, _, _, want = row
    lib, G = _lib(), gn_cases.groups_of(row)
    out = (ctypes.c_int * 5)()
    assert lib.adm_gn_plan(H * W, C, G, out) == 0 and tuple(out) == want
    if not want[0]:
        assert lib.adm_gn_splits(H * W, C) == want[4]
    assert lib.adm_gn_fused(0) == 1
    try:
        assert lib.adm_gn_plan(H * W, C, G, out) == 0 and out[0] == 0 and out[4] == lib.adm_gn_splits(H * W, C)
    finally:
        lib.adm_gn_fused(1)


def test_new_entry_points_are_declared_and_exported():
    from adm_amd import hip
    header = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    lib = _lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in hip.EXPORTS and hasattr(lib, name)
        assert len(hip._SIGS[name]) == header.split(name + "(")[1].split(");")[0].count(",") + 1, name
    for name in ("adm_concat2", "adm_split2", "adm_gn_fwd_amax", "adm_gn_bwd_add_amax"):      # the two-step path stays
        assert name in hip.EXPORTS


def test_entry_points_refuse_bad_halves_before_any_launch():
    """Null halves, a half that is no whole number of channel quads, a zero half: ADM_EINVAL (-22), decided on the host."""
    lib = _lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd = lambda a, ca, b, cb, z: lib.adm_gn_fwd_cat_amax(a, ca, b, cb, 1.0, z, None, p, p, p, p, None, 0, p, None, 1, 1, 2, 1e-5, 1, 0.0, 0, None)
    bwd = lambda da, ca, db, cb: lib.adm_gn_bwd_add_cat_amax(p, p, p, p, p, None, 0, None, da, ca, db, cb, 1.0, None, None, None, p, None, 1, 1, 2,
                                                            1, 0.0, 0, None)
    assert fwd(None, 4, p, 4, p) == -22 and fwd(p, 4, None, 4, p) == -22 and fwd(p, 4, p, 4, None) == -22
    assert fwd(p, 6, p, 2, p) == -22 and fwd(p, 0, p, 8, p) == -22 and fwd(p, 8, p, 0, p) == -22
    assert bwd(None, 4, p, 4) == -22 and bwd(p, 4, None, 4) == -22
    assert bwd(p, 6, p, 2) == -22 and bwd(p, 0, p, 8) == -22 and bwd(p, 8, p, 0) == -22


def test_the_op_takes_the_two_step_path_where_the_fused_kernels_do_not_apply(monkeypatch):
    import types
    from adm_amd import ops
    a, b = torch.zeros(1, 2, 2, 8), torch.zeros(1, 2, 2, 8)
    assert not ops._gn_cat_ok(a, b, 0)                                   # not on the GPU

    def pair(ca, cb):         # what _gn_cat_ok looks at of two GPU tensors
        t = lambda c: types.SimpleNamespace(is_cuda=True, dim=lambda: 4, shape=torch.Size((1, 2, 2, c)), dtype=torch.float32)
        return t(ca), t(cb)
    monkeypatch.setattr(ops, "GN_CONCAT", True)
    monkeypatch.setattr(ops, "COMPUTE", "f32")
    assert ops._gn_cat_ok(*pair(8, 8), 0)
    assert not ops._gn_cat_ok(*pair(6, 10), 0)                           # halves that are no whole channel quads
    assert not ops._gn_cat_ok(*pair(8, 8), 3)                            # a shape the GroupNorm kernels refuse (C % G)
    monkeypatch.setattr(ops, "GN_CONCAT", False)                         # the switch
    assert not ops._gn_cat_ok(*pair(8, 8), 0)
    monkeypatch.setattr(ops, "GN_CONCAT", True)
    monkeypatch.setattr(ops, "COMPUTE", "bf16")                          # the bf16 storage mode
    monkeypatch.setattr(ops, "BF16_STORAGE", True)
    assert not ops._gn_cat_ok(*pair(8, 8), 0)
