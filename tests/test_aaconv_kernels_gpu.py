"""GPU: every compiled instance of the relative-position attention kernels of AAConv2d (head width dk/nh = 20) at the map edges.

Two families compute one function: the row kernels of csrc/aaconv_row.hip (MFMA, bf16 storage, W in {20, 40}, H <= 64,
dv/nh in {1, 2, 3, 4, 6}) and the generic kernels of csrc/aaconv.hip (one lane per query, dv/nh = 1 .. 13, bf16 or fp32 storage).
Every case names the family it means to run and asserts the tag the launcher recorded (ops.last_kernel()), then compares o, the
log-sum-exp and all five gradients with float64 autograd through oracle.aaconv.attention_logits on the values as stored: qkv is
rounded to bf16 first, and the _f32 entry points get the same bf16-representable values in an fp32 tensor, so both storage types
and both families see identical numbers.

Bounds.  bf16 entry points: the bounds of tests/test_aaconv_gpu.py::test_attention_forward_backward -- 2e-4 of max|want| for o and
the weights, 1e-3 for each gradient -- and 1e-4 absolute for the log-sum-exp.  _f32 entry points: 4 x the worst error measured over
all fp32 cases of this module against float64 (MI355X, ROCm 7), never looser than the bf16 bound.  The margin is for __expf / __logf
differences between ROCm builds.  Every worst case is the peaked softmax at 18 x 18 (logit range 66); the plain cases measure
1e-6 and below.  The generic bf16 kernels measure the same figures (same arithmetic, same values); the row kernels measure up to
2.5e-4 on dq and 4.2e-4 on dk (the fp16 dS operand, 2^-12 per term) and 7e-6 and below everywhere else:

    quantity      worst measured     bound
    o             3.75e-06           1.5e-05
    lse (abs)     7.03e-06           2.8e-05
    weights       1.06e-06           4.3e-06
    dq            2.24e-06           9.0e-06
    dk            5.25e-06           2.1e-05
    dv            3.17e-06           1.3e-05
    d key_rel_h   1.59e-06           6.4e-06
    d key_rel_w   1.67e-06           6.7e-06
"""
import functools
import math
import types

import pytest
import torch

from chexpert_amd import synth

pytestmark = pytest.mark.gpu

DKH = 20
ROW_DVH = (1, 2, 3, 4, 6)
QUANT = ("o", "lse", "dq", "dk", "dv", "drh", "drw")
BF16_LIM = dict(o=2e-4, lse=1e-4, w=2e-4, dq=1e-3, dk=1e-3, dv=1e-3, drh=1e-3, drw=1e-3)
F32_LIM = dict(o=1.5e-5, lse=2.8e-5, w=4.3e-6, dq=9.0e-6, dk=2.1e-5, dv=1.3e-5, drh=6.4e-6, drw=6.7e-6)
assert all(F32_LIM[k] <= BF16_LIM[k] for k in BF16_LIM)
LIM = {"bf16": BF16_LIM, "f32": F32_LIM}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from chexpert_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def bf(t):
    return t.to(torch.bfloat16).float()


# ------------------------------------------------------------------------------------------------ the float64 reference
@functools.lru_cache(maxsize=None)
def problem(B, H, W, nh, dvh, qmul=1.0, kind="plain", keep_p=False):
    """Inputs of one case (as test_attention_forward_backward draws them) and their float64 results; computed once per shape and
    shared, never modified.  kind: "plain", "notables" (zero relative tables), "q0" (q = 0), "do0" (dO = 0 on one (image, head)),
    "wg0small" (dO of the first 128 queries of every image times 2^-30)."""
    from oracle import aaconv
    dk, dv, HW = DKH * nh, dvh * nh, H * W
    Cq = 2 * dk + dv
    qkv = synth.uniform(1, (B, H, W, Cq), -1.5, 1.5)
    qkv[..., :dk] *= 0.0 if kind == "q0" else qmul
    qkv = bf(qkv)
    rel_h = synth.uniform(2, (DKH, 2 * H - 1), -1, 1) + dk ** -0.5
    rel_w = synth.uniform(3, (DKH, 2 * W - 1), -1, 1) + dk ** -0.5
    if kind == "notables":
        rel_h, rel_w = torch.zeros_like(rel_h), torch.zeros_like(rel_w)
    d_o = synth.uniform(4, (B, HW, dv), -1, 1)
    zb, zn = B - 1, nh // 2
    if kind == "do0":
        d_o.view(B, HW, nh, dvh)[zb, :, zn] = 0.0
    if kind == "wg0small":
        d_o[:, :128] *= 2.0 ** -30
    t = qkv.double().permute(0, 3, 1, 2).clone().requires_grad_(True)               # (B,Cq,H,W)
    rh, rw = rel_h.double().requires_grad_(True), rel_w.double().requires_grad_(True)
    q = t[:, :dk].reshape(B, nh, DKH, H, W) * DKH ** -0.5
    k = t[:, dk:2 * dk].reshape(B, nh, DKH, H, W)
    v = t[:, 2 * dk:].reshape(B, nh, dvh, HW)
    S = aaconv.attention_logits(q, k, rh, rw).reshape(B, nh, HW, HW)
    P = torch.softmax(S, -1)
    o = torch.einsum("bnqk,bndk->bqnd", P, v).reshape(B, HW, dv)                     # channels head-major n*dvh+d
    (o * d_o.double()).sum().backward()
    g = t.grad.permute(0, 2, 3, 1).reshape(B, HW, Cq)
    with torch.no_grad():
        want = dict(o=o.detach(), lse=torch.logsumexp(S, -1).reshape(B * nh, HW), dq=g[..., :dk], dk=g[..., dk:2 * dk],
                    dv=g[..., 2 * dk:], drh=rh.grad, drw=rw.grad)
        rowmax = P.max(-1).values.flatten()
        return types.SimpleNamespace(B=B, H=H, W=W, nh=nh, dvh=dvh, dk=dk, dv=dv, HW=HW, Cq=Cq, qkv=qkv, rel_h=rel_h, rel_w=rel_w,
                                     d_o=d_o, want=want, P=P.detach() if keep_p else None, zb=zb, zn=zn,
                                     rowmax_median=rowmax.median().item(), rowmax_over_09=(rowmax > 0.9).double().mean().item(),
                                     key=(B, H, W, nh, dvh, qmul, kind))


# ------------------------------------------------------------------------------------------------ one run of the library
def hold(p, storage, dev, off=0, extra=0):
    """qkv in the storage type as a channel slice [off, off + Cq) of a buffer of pitch ceil4(Cq) + extra whose other columns are NaN
    (the launchers take pitches that are multiples of four elements; Cq itself is not one for nh in {1, 2, 3} and odd dv/nh)."""
    dt = torch.bfloat16 if storage == "bf16" else torch.float32
    ld = (p.Cq + 3) // 4 * 4 + extra
    assert off % 4 == 0 and off + p.Cq <= ld
    buf = torch.full((p.B, p.H, p.W, ld), float("nan"), dtype=dt, device=dev)
    buf[..., off:off + p.Cq] = p.qkv.to(dt).to(dev)
    return buf[..., off:off + p.Cq]


def forward(p, storage, dev, off=0, extra=0):
    from chexpert_amd import ops
    qd = hold(p, storage, dev, off, extra)
    rel_h, rel_w = p.rel_h.to(dev), p.rel_w.to(dev)
    o = torch.full((p.B, p.HW, p.dv), float("nan"), device=dev)
    lse = torch.full((p.B * p.nh, p.HW), float("nan"), device=dev)
    ops.aa_attention_fwd(qd, rel_h, rel_w, o, lse, p.nh, p.dk, p.dv)
    return qd, rel_h, rel_w, o, lse, ops.last_kernel()


def _run(p, storage, dev, det=False, off=0, extra=0):
    from chexpert_amd import ops
    qd, rel_h, rel_w, o, lse, tag_f = forward(p, storage, dev, off, extra)
    dqkv = torch.full((p.B, p.HW, p.Cq), 7.0, device=dev)                          # the sentinel: every element is overwritten
    drh, drw = torch.zeros_like(rel_h), torch.zeros_like(rel_w)
    saved = ops.WGRAD_SCRATCH_FLOATS
    try:
        ops.set_det_wgrad(det)
        ops.aa_attention_bwd(qd, rel_h, rel_w, o, p.d_o.to(dev), lse, dqkv, drh, drw, p.nh, p.dk, p.dv)
        tag_b = ops.last_kernel()
    finally:
        ops.WGRAD_SCRATCH_FLOATS = saved
    d = dqkv.cpu()
    got = dict(o=o.cpu(), lse=lse.cpu(), dq=d[..., :p.dk], dk=d[..., p.dk:2 * p.dk], dv=d[..., 2 * p.dk:], drh=drh.cpu(), drw=drw.cpu())
    return types.SimpleNamespace(got=got, dqkv=d, tags=(tag_f, tag_b))


_runs = {}


def run(p, storage, dev, det=False):
    """The dense run of a case, once per (case, storage, reduction mode): the row-against-generic and the layout tests reuse it."""
    key = (p.key, storage, det)
    if key not in _runs:
        _runs[key] = _run(p, storage, dev, det)
    return _runs[key]


def tags_of(family, storage, dvh, W):
    if family == "row":
        return "aa_row_fwd<%d,%d>" % (dvh, W), "aa_row_bwd<%d,%d>" % (dvh, W)
    return "aa_fwd<%s,%d>" % (storage, dvh), "aa_bwd<%s,%d>" % (storage, dvh)


def scale_of(p, k):
    """What an error of quantity k is relative to: max|want|; 1 for the log-sum-exp (absolute).  A map of one row (column) has a
    key_rel_h (key_rel_w) table of ONE column, and its gradient sum_i q_i sum_j dS_ij is zero analytically, because every row of
    dS = P (dP - delta) sums to zero: float64 returns 1e-17 there, which is no scale.  The kernel adds the same terms dS_ij q_i
    that make up the other table's gradient, only grouped differently, so its rounding error is measured against that table."""
    if k == "lse":
        return 1.0
    if (k == "drh" and p.H == 1) or (k == "drw" and p.W == 1):
        k = "drw" if k == "drh" else "drh"
    return p.want[k].abs().max().item() + 1e-300


def errors(p, r):
    return {k: (r.got[k].double() - p.want[k]).abs().max().item() / scale_of(p, k) for k in QUANT}


def verify(p, r, storage, family, what):
    lim = LIM[storage]
    e = errors(p, r)
    print("AAK %-44s %-5s %-4s %s" % (what, storage, family, " ".join("%s=%.2e" % (k, e[k]) for k in QUANT)))
    assert r.tags == tags_of(family, storage, p.dvh, p.W), r.tags
    for k in QUANT:
        assert torch.isfinite(r.got[k]).all().item(), "%s: %s is not finite" % (what, k)
    assert (r.dqkv != 7.0).all().item(), "%s: %d elements of dqkv were not written" % (what, (r.dqkv == 7.0).sum().item())
    bad = ["%s %.3e > %.1e" % (k, e[k], lim[k]) for k in QUANT if not e[k] <= lim[k]]
    assert not bad, "%s (%s, %s): %s" % (what, storage, family, "; ".join(bad))
    return e


def name(B, H, W, nh, dvh):
    return "B%d %dx%d nh%d dvh%d" % (B, H, W, nh, dvh)


# ------------------------------------------------------------------------------------------------ row kernels
# (W, dvh, B, H, nh).  All ten <DVH, WW> instances at the square production map with two images (the image stride), then each
# instance at edge heights, every height for both widths:
#   H = 1              one key row, HW = 20 / 40: a single partial workgroup, one / two query tiles on the key side
#   H = 2, 4, 5 (W 20) and H = 2, 3 (W 40): ntl = ceil(HW / 32) in {2, 3, 4} -- all three residues of the key side's three-deep buffer
#   H = 7              HW = 140 / 280, a multiple of neither 128 nor 32: clamped queries and keys in the last workgroup
#   H = W + 3          the H > W + 1 layout of the query side's LDS (the key image moves)
#   H = 64             the dispatch limit: the largest relative tables
ROW_SQUARE = [(20, d, 2, 20, 8) for d in ROW_DVH] + [(40, d, 2, 40, 2) for d in ROW_DVH]
ROW_EDGES = [(20, 1, 2, 1, 8), (20, 2, 2, 2, 8), (20, 3, 2, 4, 8), (20, 4, 2, 5, 8), (20, 6, 2, 7, 3), (20, 4, 2, 1, 3),
             (20, 1, 1, 23, 2), (20, 6, 1, 23, 2), (20, 2, 1, 64, 1), (20, 3, 1, 64, 2),
             (40, 1, 2, 1, 8), (40, 2, 2, 2, 8), (40, 3, 2, 3, 8), (40, 4, 2, 7, 3), (40, 6, 2, 2, 8),
             (40, 6, 1, 43, 1), (40, 2, 1, 43, 2), (40, 1, 1, 64, 1), (40, 4, 1, 64, 2)]


@pytest.mark.parametrize("W,dvh,B,H,nh", ROW_SQUARE + ROW_EDGES)
def test_row_kernels(dev, W, dvh, B, H, nh):
    p = problem(B, H, W, nh, dvh)
    verify(p, run(p, "bf16", dev), "bf16", "row", name(B, H, W, nh, dvh))


def test_height_65_leaves_the_row_kernels(dev):
    """H = 65 is past the row kernels' tables.  W = 20: the generic kernels take it (62.4 KB of LDS in the forward) and agree with
    float64 all the same.  W = 40: the generic forward's own LDS check refuses it (75.5 KB > 64 KB) with CX_ESHAPE, before any launch."""
    p = problem(1, 65, 20, 1, 3)
    verify(p, run(p, "bf16", dev), "bf16", "generic", name(1, 65, 20, 1, 3))
    wide = types.SimpleNamespace(B=1, H=65, W=40, nh=1, dk=DKH, dv=3, HW=65 * 40, Cq=2 * DKH + 3, qkv=torch.zeros(1, 65, 40, 2 * DKH + 3),
                                 rel_h=torch.zeros(DKH, 2 * 65 - 1), rel_w=torch.zeros(DKH, 2 * 40 - 1))
    with pytest.raises(RuntimeError, match=r"cx_aa_attention_fwd failed: unsupported shape \(code -3\)"):
        forward(wide, "bf16", dev)


# ------------------------------------------------------------------------------------------------ generic kernels
# 18 x 18 is not a row width, HW = 324 leaves a partial third workgroup, and H + W = 36 is the smallest square whose query-side
# backward asks for more than 64 KB of LDS (1344 (H + W) + 17600 + 256 dvh bytes): every instance has to have had its limit raised.
GEN_18 = [(2, 18, 18, 8, d) for d in range(1, 14)]
GEN_BF16 = GEN_18 + [(2, 20, 20, 2, 5), (2, 20, 20, 2, 11), (1, 40, 40, 2, 5), (1, 40, 40, 2, 11)]      # v = 0.32 / 0.7 transitions at 320^2
GEN_F32 = GEN_18 + [(2, 20, 20, 2, d) for d in (1, 3, 6)] + [(1, 40, 40, 2, d) for d in (1, 3, 6)]      # fp32 parity mode of aadensenet121


@pytest.mark.parametrize("B,H,W,nh,dvh", GEN_BF16)
def test_generic_kernels_bf16(dev, B, H, W, nh, dvh):
    p = problem(B, H, W, nh, dvh)
    verify(p, run(p, "bf16", dev), "bf16", "generic", name(B, H, W, nh, dvh))


@pytest.mark.parametrize("B,H,W,nh,dvh", GEN_F32)
def test_generic_kernels_f32(dev, B, H, W, nh, dvh):
    p = problem(B, H, W, nh, dvh)
    verify(p, run(p, "f32", dev), "f32", "generic", name(B, H, W, nh, dvh))


@pytest.mark.parametrize("W,dvh,B,H,nh", ROW_SQUARE)
def test_row_against_generic(dev, W, dvh, B, H, nh):
    """Two independent implementations of one function on identical values: the bf16 row result and the _f32 generic result differ
    by no more than the sum of their two bounds.  (When a case above misses a bound, this says which kernel owns the error.)"""
    p = problem(B, H, W, nh, dvh)
    a, b = run(p, "bf16", dev), run(p, "f32", dev)
    assert a.tags == tags_of("row", "bf16", dvh, W) and b.tags == tags_of("generic", "f32", dvh, W), (a.tags, b.tags)
    e = {k: (a.got[k].double() - b.got[k].double()).abs().max().item() / scale_of(p, k) for k in QUANT}
    print("AAK row-generic %-32s %s" % (name(B, H, W, nh, dvh), " ".join("%s=%.2e" % (k, e[k]) for k in QUANT)))
    bad = ["%s %.3e" % (k, e[k]) for k in QUANT if not e[k] <= BF16_LIM[k] + F32_LIM[k]]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the attention maps
@pytest.mark.parametrize("storage", ["bf16", "f32"])
@pytest.mark.parametrize("B,H,W,nh,dvh", [(2, 20, 20, 2, 3), (2, 5, 7, 8, 1), (2, 12, 20, 8, 2)])
def test_attention_weights(dev, storage, B, H, W, nh, dvh):
    from chexpert_amd import ops
    p = problem(B, H, W, nh, dvh, keep_p=True)
    qd, rel_h, rel_w, o, lse, _ = forward(p, storage, dev)
    wts = ops.aa_attention_weights(qd, rel_h, rel_w, lse, p.nh, p.dk, p.dv)
    assert ops.last_kernel() == "aa_weights<%s>" % storage, ops.last_kernel()
    assert wts.shape == (B, nh, H * W, H * W) and torch.isfinite(wts).all().item()
    err = (wts.cpu().double() - p.P).abs().max().item() / p.P.abs().max().item()
    rows = (wts.double().sum(-1) - 1).abs().max().item()
    print("AAK weights %-32s %-5s w=%.2e rows=%.2e" % (name(B, H, W, nh, dvh), storage, err, rows))
    assert err <= LIM[storage]["w"], err
    assert rows < 1e-4, rows


# ------------------------------------------------------------------------------------------------ layout of qkv
@pytest.mark.parametrize("storage,B,H,W,nh,dvh", [("bf16", 2, 20, 20, 8, 3), ("bf16", 2, 18, 18, 8, 5), ("f32", 2, 18, 18, 8, 5),
                                                  ("f32", 2, 20, 20, 8, 3)])
def test_pitched_qkv(dev, storage, B, H, W, nh, dvh):
    """qkv as a channel slice of a wider buffer (offset 4 channels, pitch Cq + 12, every other column NaN): the same bits as the
    dense run, nothing non-finite.  (Slab mode, so that the table gradients are sums in a fixed order too.)"""
    p = problem(B, H, W, nh, dvh)
    assert p.Cq % 4 == 0
    dense, pitched = run(p, storage, dev, det=True), _run(p, storage, dev, det=True, off=4, extra=12)
    family = "row" if storage == "bf16" and W == 20 else "generic"
    verify(p, pitched, storage, family, "pitched " + name(B, H, W, nh, dvh))
    assert dense.tags == pitched.tags
    for k in QUANT:
        assert torch.equal(dense.got[k], pitched.got[k]), k


@pytest.mark.parametrize("storage", ["bf16", "f32"])
@pytest.mark.parametrize("entry", ["fwd", "weights", "bwd"])
def test_out_of_contract_pitch_is_refused_before_any_launch(dev, storage, entry):
    """A pitch that is no multiple of four elements (the kernels read q and k in chunks of four), or one below 2 dk + dv, comes back
    as CX_ESHAPE from the launcher's own check: nothing is launched (outputs keep their prefill)."""
    from chexpert_amd import ops
    dt = torch.bfloat16 if storage == "bf16" else torch.float32
    B, H, W, nh, dvh = 1, 4, 20, 2, 3
    dk, dv = DKH * nh, dvh * nh
    Cq = 2 * dk + dv                                                                 # 86
    tabs = torch.zeros(DKH, 2 * H - 1, device=dev), torch.zeros(DKH, 2 * W - 1, device=dev)
    o = torch.full((B, H * W, dv), 5.0, device=dev)
    lse = torch.full((B * nh, H * W), 5.0, device=dev)
    dqkv = torch.full((B, H * W, Cq), 7.0, device=dev)
    d_t = torch.zeros_like(tabs[0]), torch.zeros_like(tabs[1])

    def call(qd, dv_):
        if entry == "fwd":
            ops.aa_attention_fwd(qd, *tabs, o, lse, nh, dk, dv_)
        elif entry == "weights":
            ops.aa_attention_weights(qd, *tabs, lse, nh, dk, dv_)
        else:
            ops.aa_attention_bwd(qd, *tabs, o, o, lse, dqkv, *d_t, nh, dk, dv_)

    for ld, dv_ in ((Cq + 1, dv), (Cq + 3, dv), (Cq + 2, dv + 2 * nh)):               # pitch 87, 89; pitch 88 under 2 dk + dv = 90
        qd = torch.zeros(B, H, W, ld, dtype=dt, device=dev)[..., :Cq]
        with pytest.raises(RuntimeError, match=r"unsupported shape \(code -3\)"):
            call(qd, dv_)
    torch.cuda.synchronize()
    assert (o == 5.0).all().item() and (lse == 5.0).all().item() and (dqkv == 7.0).all().item()


# ------------------------------------------------------------------------------------------------ degenerate inputs
DEGENERATE = [("bf16", "row", 2, 20, 20, 8, 3), ("bf16", "generic", 2, 18, 18, 8, 6), ("f32", "generic", 2, 18, 18, 8, 6)]


@pytest.mark.parametrize("storage,family,B,H,W,nh,dvh", DEGENERATE)
def test_zero_relative_tables(dev, storage, family, B, H, W, nh, dvh):
    """attn_params["relative"] = False: the kernels run with zero position tables (plain q . k logits)."""
    p = problem(B, H, W, nh, dvh, kind="notables")
    verify(p, run(p, storage, dev), storage, family, "no tables " + name(B, H, W, nh, dvh))


@pytest.mark.parametrize("storage,family,B,H,W,nh,dvh", DEGENERATE)
def test_zero_queries_give_a_uniform_softmax(dev, storage, family, B, H, W, nh, dvh):
    p = problem(B, H, W, nh, dvh, kind="q0")
    r = run(p, storage, dev)
    verify(p, r, storage, family, "q = 0 " + name(B, H, W, nh, dvh))
    lim = LIM[storage]
    v = p.qkv[..., 2 * p.dk:].reshape(B, p.HW, p.dv).double()
    mean = v.mean(1, keepdim=True).expand(B, p.HW, p.dv)
    assert (r.got["o"].double() - mean).abs().max().item() <= lim["o"] * mean.abs().max().item()
    assert (r.got["lse"].double() - math.log(p.HW)).abs().max().item() <= lim["lse"]


@pytest.mark.parametrize("storage,family,B,H,W,nh,dvh", DEGENERATE)
def test_zero_gradient_on_one_head(dev, storage, family, B, H, W, nh, dvh):
    """dO = 0 on one whole (image, head): its dq, dk and dv are exactly zero (the amax = 0 branch of the row kernels' power-of-two
    gradient scale), and every other (image, head) comes out bit for bit as without the zeros."""
    p0, p = problem(B, H, W, nh, dvh), problem(B, H, W, nh, dvh, kind="do0")
    base, r = run(p0, storage, dev), run(p, storage, dev)
    verify(p, r, storage, family, "dO = 0 on a head " + name(B, H, W, nh, dvh))
    for k, w in (("dq", DKH), ("dk", DKH), ("dv", dvh)):
        got = r.got[k].view(B, p.HW, nh, w)
        ref = base.got[k].view(B, p.HW, nh, w)
        assert (got[p.zb, :, p.zn] == 0).all().item(), "%s of the head without a gradient" % k
        keep = torch.ones(B, nh, dtype=torch.bool)
        keep[p.zb, p.zn] = False
        assert torch.equal(got.permute(0, 2, 1, 3)[keep], ref.permute(0, 2, 1, 3)[keep]), "%s of the other heads" % k


@pytest.mark.parametrize("storage,family,B,H,W,nh,dvh", [("bf16", "row", 2, 20, 20, 8, 3), ("bf16", "row", 1, 40, 40, 2, 1),
                                                         ("bf16", "generic", 2, 18, 18, 8, 6)])
def test_gradient_magnitude_differs_between_workgroups(dev, storage, family, B, H, W, nh, dvh):
    """dO of the first 128 queries (the first query-side workgroup of every (image, head)) is 2^-30 of the others'.  The row kernels
    carry dS as an fp16 operand under a power-of-two scale.  On the query side the scale is the workgroup's own: dq of those 128
    queries is as accurate, relative to ITS size, as any other (a scale per (image, head) would leave their dS at 2^-30, below the
    fp16 subnormals).  On the key side every key meets every query, so the scale is that of the whole (image, head): taken from
    the workgroup's own 128 queries it would push the others' dS to 2^30, past the largest fp16."""
    p = problem(B, H, W, nh, dvh, kind="wg0small")
    r = run(p, storage, dev)
    verify(p, r, storage, family, "small dO in workgroup 0 " + name(B, H, W, nh, dvh))
    want = p.want["dq"][:, :128]
    err = (r.got["dq"][:, :128].double() - want).abs().max().item() / want.abs().max().item()
    print("AAK    dq of the first 128 queries against their own size: %.2e (max|want| %.2e)" % (err, want.abs().max().item()))
    assert err <= LIM[storage]["dq"], err


# ------------------------------------------------------------------------------------------------ peaked softmax
@pytest.mark.parametrize("storage,family,B,H,W,nh,dvh", [("bf16", "row", 2, 20, 20, 8, 3), ("bf16", "row", 1, 40, 40, 2, 1),
                                                         ("bf16", "generic", 2, 18, 18, 8, 6), ("f32", "generic", 2, 18, 18, 8, 6)])
def test_peaked_softmax(dev, storage, family, B, H, W, nh, dvh):
    """q scaled by 6 before rounding: logits span ~66, half the rows put more than half of their mass on one key -- the running
    maximum is replaced many times per row (the online rescale) and most exponentials underflow."""
    p = problem(B, H, W, nh, dvh, qmul=6.0)
    print("AAK peaked %s: median row maximum %.3f, rows above 0.9: %.1f %%" % (name(B, H, W, nh, dvh), p.rowmax_median, 100 * p.rowmax_over_09))
    assert p.rowmax_median >= 0.5, p.rowmax_median
    verify(p, run(p, storage, dev), storage, family, "peaked " + name(B, H, W, nh, dvh))


# ------------------------------------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("storage,family,B,H,W,nh,dvh", [("bf16", "row", 2, 20, 20, 8, 3), ("bf16", "generic", 2, 18, 18, 8, 6),
                                                         ("f32", "generic", 2, 18, 18, 8, 6)])
def test_backward_is_reproducible_with_the_slab_workspace(dev, storage, family, B, H, W, nh, dvh):
    """ops.set_det_wgrad(True): the workgroups' table partials go to slabs and are added in workgroup order -- two backward passes
    give the same bits in all five gradients.  Off (fp32 atomics): within the bounds.  (_run restores the setting in a finally.)"""
    from chexpert_amd import ops
    saved = ops.WGRAD_SCRATCH_FLOATS
    p = problem(B, H, W, nh, dvh)
    a, b = _run(p, storage, dev, det=True), _run(p, storage, dev, det=True)
    verify(p, a, storage, family, "slabs " + name(B, H, W, nh, dvh))
    for k in QUANT:
        assert torch.equal(a.got[k], b.got[k]), k
    verify(p, _run(p, storage, dev, det=False), storage, family, "atomics " + name(B, H, W, nh, dvh))
    assert ops.WGRAD_SCRATCH_FLOATS == saved
