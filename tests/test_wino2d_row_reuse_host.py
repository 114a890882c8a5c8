"""CPU-only: the row-reuse switch of the 3x3 Winograd kernel (adm_wino2d_x6_row_reuse) as a host call."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_reuse_switch_is_declared_exported_and_toggles():
    from adm_amd import hip
    header = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    name = "adm_wino2d_x6_row_reuse"
    assert re.search(r"^int\s+%s\s*\(int v\);" % name, header, flags=re.M)
    assert name in hip.EXPORTS and name in hip.NO_STREAM
    fn = getattr(hip.lib(), name)
    start = fn(-1)                        # a negative value only queries
    try:
        assert start in (0, 1) and fn(-1) == start
        assert fn(0) == start             # returns the previous value ...
        assert fn(-1) == 0                # ... and sets the new one
        assert fn(1) == 0 and fn(-1) == 1
        assert fn(7) == 1 and fn(-1) == 1      # any positive value is "on"
    finally:
        fn(start)
    assert fn(-1) == start
    if os.environ.get("ADM_X6_ROW_REUSE") is None:
        assert start == 1, "the default is on"
