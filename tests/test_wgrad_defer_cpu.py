"""CPU (no GPU): the host side of the deferred weight-gradient sums (ops.wgrad_defer_*, cx_wgrad_defer, cx_wgrad_defer_take) and
`ordered_sum`, the fp32 restatement of dw_reduce_body's association (csrc/elementwise.hip) that tests/test_wgrad_defer_gpu.py
compares cx_dw_reduce_table with bit for bit."""
import ctypes as C
import threading

import numpy as np

F32 = np.float32


def ordered_sum(slab, dw):
    """dw + the sum over the rows of `slab` (splits, total) in dw_reduce_body's order, every step in fp32: eight lanes each add a
    contiguous range of `per = ceil(splits / 8)` rows in order from 0.0f (a range may be empty), then the eight partial sums are
    added in lane order from 0.0f, then dw is added."""
    slab = np.ascontiguousarray(slab, dtype=F32)
    splits, total = slab.shape
    per = (splits + 7) >> 3
    part = []
    for j in range(8):
        a = np.zeros(total, F32)
        for s in range(j * per, min(j * per + per, splits)):
            a = a + slab[s]
        part.append(a)
    t = np.zeros(total, F32)
    for j in range(8):
        t = t + part[j]
    out = np.asarray(dw, dtype=F32).reshape(total) + t
    assert out.dtype == F32
    return out


def _data(seed, splits, total):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (splits, total)).astype(F32)


def test_ordered_sum_agrees_with_the_float64_sum():
    """Within `splits` ulps of the largest partial sum: an addition to 0.0f is exact, which leaves `splits` additions that round
    (splits - lanes inside the lanes, lanes - 1 across them, one for dw), each by at most half an ulp of its result, and no partial
    result exceeds the sum of the absolute values."""
    for seed, splits, total in ((1, 1, 5), (2, 7, 64), (3, 8, 33), (4, 9, 100), (5, 61, 257), (6, 200, 31)):
        slab, dw = _data(seed, splits, total), _data(seed + 100, 1, total)[0]
        got = ordered_sum(slab, dw)
        want = dw.astype(np.float64) + slab.astype(np.float64).sum(0)
        largest = (np.abs(dw.astype(np.float64)) + np.abs(slab.astype(np.float64)).sum(0)).max()
        bound = splits * np.spacing(F32(largest))
        assert np.abs(got.astype(np.float64) - want).max() <= bound, (splits, total)


def test_ordered_sum_is_not_the_left_to_right_sum():
    """splits = 61: eight lanes of eight rows (the last of five) are another association than one running sum, and on random data
    some element shows it in its last bit -- which is what lets a bit-exact comparison with the kernel tell the two apart."""
    slab = _data(7, 61, 512)
    dw = np.zeros(512, F32)
    plain = np.zeros(512, F32)
    for s in range(61):
        plain = plain + slab[s]
    got = ordered_sum(slab, dw)
    assert (got != plain).any(), "choose another seed: no element tells the two associations apart"
    assert np.abs(got.astype(np.float64) - plain).max() <= 61 * np.spacing(F32(np.abs(slab).sum(0).max()))      # rounding, no more
    # ... and nine rows leave three lanes empty: per = 2, lanes 0..3 take two rows each, lane 4 one, lanes 5..7 none
    slab9 = _data(8, 9, 64)
    want = ((((slab9[0] + slab9[1]) + (slab9[2] + slab9[3])) + (slab9[4] + slab9[5])) + (slab9[6] + slab9[7])) + slab9[8]
    assert np.array_equal(ordered_sum(slab9, np.zeros(64, F32)), (F32(0) + want))


def _lib():
    from chexpert_amd import _lib as L
    return L, L.lib()


def test_defer_switch_returns_the_previous_state():
    L, lib = _lib()
    lib.cx_wgrad_defer(-1)
    try:
        assert [lib.cx_wgrad_defer(v) for v in (1, 1, 0, -1)] == [0, 1, 1, 0]
        assert lib.cx_wgrad_defer(0) == 0
    finally:
        lib.cx_wgrad_defer(-1)


def test_defer_take_on_an_empty_list():
    L, lib = _lib()
    lib.cx_wgrad_defer(-1)
    arr = (L.CxReduceDesc * 4)()
    blocks = C.c_int64(12345)
    assert lib.cx_wgrad_defer_take(arr, 4, C.byref(blocks)) == 0
    assert blocks.value == 0
    assert lib.cx_wgrad_defer_take(None, 0, None) == 0          # nothing to hand over: not an error either


def test_defer_state_is_thread_local():
    L, lib = _lib()
    lib.cx_wgrad_defer(-1)
    seen = {}

    def other():
        seen["before"] = lib.cx_wgrad_defer(1)        # this thread's own switch: off, whatever the main thread did
        seen["after"] = lib.cx_wgrad_defer(1)
        lib.cx_wgrad_defer(-1)
    try:
        assert lib.cx_wgrad_defer(1) == 0
        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert seen == {"before": 0, "after": 1}
        assert lib.cx_wgrad_defer(1) == 1, "another thread's cx_wgrad_defer(-1) switched this thread's deferral off"
        lib.cx_wgrad_defer(0)
        seen.clear()
        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert lib.cx_wgrad_defer(0) == 0, "another thread's cx_wgrad_defer(1) switched this thread's deferral on"
    finally:
        lib.cx_wgrad_defer(-1)


def test_defer_is_a_no_op_without_the_slab_workspace(monkeypatch):
    """ops.WGRAD_SCRATCH_FLOATS == 0 (atomic mode): begin says so, flush and abort do nothing, and none of them creates an arena
    (which would be a device allocation)."""
    import torch
    from chexpert_amd import ops
    L, lib = _lib()
    lib.cx_wgrad_defer(-1)
    monkeypatch.setattr(ops, "WGRAD_SCRATCH_FLOATS", 0)
    monkeypatch.setattr(ops, "_arenas", {})
    dev = torch.device("cuda", 0)
    assert ops.wgrad_defer_begin(dev) is False
    assert lib.cx_wgrad_defer(0) == 0, "begin switched the C side on"
    ops.wgrad_defer_flush(dev)
    ops.wgrad_defer_flush(dev, keep=True)
    ops.wgrad_defer_abort(dev)
    assert ops._arenas == {}
    assert ops._wgrad_ws(dev) == (None, None, False)
    assert lib.cx_wgrad_defer(0) == 0
