"""GPU: the fp16-format 3x3 weight gradient (conv_wgrad_x6.hip) on the split counts its time model picks, through the C ABI.

The launch with splits = 0 must take the count the host query adm_conv_wgrad_x6_h3_plan names, and its result must be the kernel's
result at that count: with one split (plain stores) bit for bit, with several (float atomics, whose order is free) at the bar of
tests/parity.py::close, as the bias gradient always is (its partial sums meet in float atomics at any count).  The same result is compared with the f32-MFMA kernel adm_conv_wgrad_wino2d, which splits nothing and shares no
code with it.  The two shapes are the smallest production ones whose plan the model moved (5 -> 1 and 7 -> 3 splits); the accuracy of
every production plan against fp64 is tests/test_hip_accuracy.py's."""
import functools

import pytest
import torch

from parity import close  # noqa: E402  (tests/parity.py: the north_star tolerance, elementwise)

pytestmark = pytest.mark.gpu

# name -> (B, H = W, Cin, Cout, the split count the time model takes, the fill rule's count)
CASES = {"one-split": (128, 4, 768, 384, 1, 5), "three-splits": (128, 8, 384, 384, 3, 7)}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip, ops as _ops
    hip.lib()        # raises if the HIP library is missing: no fallback
    return _ops


@functools.lru_cache(maxsize=None)
def _data(name):
    B, H, cin, cout, _, _ = CASES[name]
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.rand(B, H, H, cin, device="cuda", generator=g) * 2 - 1
    dy = (torch.rand(B, H, H, cout, device="cuda", generator=g) * 2 - 1) * 0.05
    return x, dy


def _h3(ops, name, splits):
    """(dwp2[Cout][12][Cin], dbias[Cout]) of adm_conv_wgrad_x6_h3 in the atomic mode at that split count (0: the launcher's own)"""
    from adm_amd import hip
    B, H, cin, cout, _, _ = CASES[name]
    x, dy = _data(name)
    dw = torch.full((cout, 12, cin), 7.0, device="cuda")      # (the launcher clears it where it accumulates, and overwrites it where not)
    db = torch.zeros(cout, device="cuda")
    ax, ady = ops.amax_vector(x), ops.amax_vector(dy)      # (both alive until the launch has been queued)
    hip.call("adm_conv_wgrad_x6_h3", hip.ptr(x), hip.ptr(dy), hip.ptr(dw), hip.ptr(db), B, H, H, cin, cin, cout, cout, splits, 0, 0,
             hip.ptr(ax), hip.ptr(ady))
    torch.cuda.synchronize()
    return dw, db


@functools.lru_cache(maxsize=None)
def _f32(name):
    from adm_amd import hip
    B, H, cin, cout, _, _ = CASES[name]
    x, dy = _data(name)
    dw = torch.zeros(cout, 12, cin, device="cuda")
    db = torch.zeros(cout, device="cuda")
    hip.call("adm_conv_wgrad_wino2d", hip.ptr(x), hip.ptr(dy), hip.ptr(dw), hip.ptr(db), B, H, H, cin, cin, cout, cout, 0)
    torch.cuda.synchronize()
    return dw, db


@pytest.mark.parametrize("name", list(CASES))
def test_auto_launch_takes_the_queried_count(ops, name):
    from adm_amd import hip
    B, H, cin, cout, want, fill = CASES[name]
    assert hip.lib().adm_conv_wgrad_x6_h3_plan(B, H, H, cin, cout) == want
    dw0, db0 = _h3(ops, name, 0)
    dw1, db1 = _h3(ops, name, want)
    dwf, dbf = _h3(ops, name, fill)
    ref_w, ref_b = _f32(name)
    if want == 1:
        assert torch.equal(dw0, dw1)
    else:
        close(dw0, dw1)
    close(db0, db1)      # (the bias sums meet in float atomics at any split count)
    for dw, db in ((dw0, db0), (dwf, dbf)):
        close(dw, ref_w)
        close(db, ref_b)
