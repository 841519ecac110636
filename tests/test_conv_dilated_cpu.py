"""CPU: the case tables and float64 references of the dilated / grouped 3x3 convolution tests (tests/conv_dilated_cases.py) checked
by themselves -- the conditions test_conv_dilated_gpu.py relies on hold here and on the GPU machine alike."""
import pytest
import torch

import conv_dilated_cases as cd
from conv_dilated_cases import BF16, CASES, EXACT, F32, GROUPED, cid

ALL = CASES + GROUPED + EXACT


@pytest.mark.parametrize("c", ALL, ids=cid)
def test_tables_pass_the_library_shape_checks(c):
    """cx_conv_gemm / cx_conv_wgrad accept every case as listed (3x3, pad = dil): output size, the transposed-stride form of the
    input gradient, channel counts and slice offsets of both storage types."""
    assert cd.lib_forward_size(c) == (c.Ho, c.Wo)
    assert cd.lib_accepts_dgrad(c) and cd.lib_accepts_wgrad(c)
    assert c.stride in (1, 2) and c.dil >= 1
    kg, ng = c.K // c.groups, c.N // c.groups
    assert c.K % c.groups == 0 and c.N % c.groups == 0 and kg % 8 == 0 and ng % 8 == 0           # bf16: 16-byte channel chunks
    assert c.B * max(c.H * c.W, c.Ho * c.Wo) < 1 << 20


def test_tables_reach_what_they_are_there_for():
    by = {cid(c): c for c in CASES}
    assert len(by) == len(CASES)
    tiles = {cd.gemm_bn(c.N) for c in CASES} | {cd.gemm_bn(c.K) for c in CASES}
    assert tiles == {32, 64, 128}
    assert {cd.wgrad_tile(c.N) for c in CASES} == {(32, 128), (64, 64), (128, 64)}
    assert cd.wgrad_tile(72) == (64, 64) and cd.wgrad_tile(104) == (128, 64) and cd.wgrad_tile(96) == (128, 64)
    assert any(c.B * c.Ho * c.Wo > 128 and (c.B * c.Ho * c.Wo) % 128 for c in CASES), "more than one pixel tile, the last one ragged"
    assert any(c.K % 32 for c in CASES), "a partial last K step"
    assert any(c.dil % 2 and c.dil > 1 for c in CASES), "an odd dilation"
    strided = [c for c in CASES if c.stride == 2]
    assert {c.H % 2 for c in strided} == {0, 1} and all(c.dil > 1 for c in strided)
    for c in strided:                                # most input pixels of a strided dilated convolution receive no tap
        assert 0.72 <= cd.untouched_fraction(c) <= 0.735, (cid(c), cd.untouched_fraction(c))
    assert {(c.K // c.groups, c.dil) for c in GROUPED} == {(32, 1), (32, 2), (8, 1), (8, 2)} and all(c.groups == 4 for c in GROUPED)
    assert {(c.dil, c.stride) for c in EXACT} == {(2, 1), (2, 2), (4, 1)}


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("c", CASES + GROUPED, ids=cid)
def test_references_are_self_consistent(c, dt):
    """autograd's input gradient against conv_transpose2d with output_padding = (H - 1) % s; the operands hold storage-type
    values; the prologue shift is positive on every channel."""
    d, r = cd.data(c, dt), cd.refs(c, dt)
    for t in (d.x, d.w, d.u, d.v, d.ex, d.old):
        assert t.dtype == torch.float64 and torch.equal(cd.stored(t, dt), t)
    assert d.pb.min().item() >= 0.2
    for dy, dx in ((d.u, r.dx_plain), (r.dy, r.dx_pro)):
        other = cd.transposed_input_grad(c, d.w, dy)
        assert other.shape == dx.shape == d.x.shape
        assert (other - dx).abs().max().item() <= 1e-12 * dx.abs().max().item()
    if c.stride == 2:                                # the pixels off the stride grid: exact zeros
        assert (r.dx_plain[:, :, 1::2] == 0).all() and (r.dx_plain[:, :, :, 1::2] == 0).all()
        assert (r.dx_plain[:, :, ::2, ::2] != 0).all()
    # a padded tap filled with relu(pb) would move the output by far more than the bound: the border of a is not near zero
    assert r.a[:, :, 0].min().item() >= 0 and r.a[:, :, 0].mean().item() > 0.2
    for t in (r.y_plain, r.y_pro, r.g, r.dw_plain, r.dw_pro, r.S1, r.S2):
        assert torch.isfinite(t).all() and t.abs().max().item() > 0.1


@pytest.mark.parametrize("dt", [BF16, F32])
def test_six_of_nine_taps_are_padding_on_the_4x5_map(dt):
    """dil = 4 on a 4x5 map: the kernel rows ky = 0 and ky = 2 read only padding, so their weight gradient is exactly 0."""
    c = next(c for c in CASES if (c.H, c.W, c.dil) == (4, 5, 4))
    r = cd.refs(c, dt)
    for dw in (r.dw_plain, r.dw_pro):
        assert (dw[:, :, [0, 2], :] == 0).all() and (dw[:, :, 1, :].abs().amax((0, 1)) > 0).all()
    e = cd.exact(next(c for c in EXACT if c.dil == 4))
    assert (e.dw[:, :, [0, 2], :] == 0).all() and (e.dw[:, :, 1, :] != 0).any()


@pytest.mark.parametrize("c", EXACT, ids=cid)
def test_exact_runs_round_nothing(c):
    """Every reference value of a bf16-stored output is an integer of magnitude <= 256; every partial sum of the weight gradient
    stays below 2^24; the impulses sit on the four corners and the centre, one per image, at distinct channels."""
    e = cd.exact(c)
    assert e.w.max().item() <= 256 and torch.equal(e.w, e.w.to(torch.bfloat16).double())
    assert len(set(cd.EXACT_CH_IN)) == c.B == len(set(cd.EXACT_CH_OUT)) and max(cd.EXACT_CH_IN) < c.K and max(cd.EXACT_CH_OUT) < c.N
    assert len(set(cd.corners_and_centre(c.H, c.W))) == 5 and len(set(cd.corners_and_centre(c.Ho, c.Wo))) == 5
    for t in (e.x, e.u):
        assert t.sum().item() == c.B and (t.sum((1, 2, 3)) == 1).all()
    for t in (e.y, e.dx):
        assert t.abs().max().item() <= 256 and torch.equal(t, t.round()) and torch.equal(t, t.to(torch.bfloat16).double())
        assert (t != 0).any()
    assert e.dw_abs_bound < 1 << 24 and torch.equal(e.dw, e.dw.round()) and torch.equal(e.dw, e.dw.float().double())
    assert e.xi.abs().max().item() == 2 and e.gi.abs().max().item() == 2
    # the taps tell apart: an output pixel that one impulse reaches through one tap holds that tap's weight
    y0 = e.y[0, :, 0, 0]                             # image 0: impulse at the top-left corner, read by the centre tap at output (0, 0)
    assert torch.equal(y0, e.w[:, cd.EXACT_CH_IN[0], 1, 1])
