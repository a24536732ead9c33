"""The split-fp16 kernels across the dynamic range of their power-of-two scale.

Every split consumer scales an operand by 2^e, e = clamp(14 - floor(log2 max|x|), -100, 100) (``split_exp`` in
csrc/split16.h), splits it into fp16 hi + lo and undoes the scale in the epilogue with
``ldexpf(1, -(e1 + e2))``.  The scale is a power of two, so the following hold exactly and are asserted with
``torch.equal``, no tolerance:

* equivariance: op(s x, t w) == (s t) op(x, w) for s, t in {2^-40, 1, 2^40}: the max bits change in the exponent field
  only, split_exp moves by the same amount (|14 - k| stays far inside the clamp), the planes are the same bytes, and
  the epilogue's scaling is exact while the result is a normal fp32 (2^+-80 times a unit-scale result is);
* zeros: an all-zero operand (max bits 0) gives all-zero planes and an exactly zero output, no NaN, no Inf;
* a max supplied by the producing kernel gives the same bytes as the consumer's own absmax pass, also at 2^-40.

No bias is passed anywhere: a bias is not scaled.  Shapes: one small ragged shape per kernel from the dirty-memory table.
"""
import functools
import math

import pytest
import torch

import test_gpu_bn_bwd_fused as tbn
from oracle.det_init import det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
LO, HI = 2.0 ** -40, 2.0 ** 40
FACTORS = [(LO, 1.0), (1.0, LO), (HI, 1.0), (1.0, HI), (LO, LO), (HI, HI)]


def K():
    from avse_challenge_amd import kernels
    return kernels


def dev(t, fmt=None):
    t = t.to(DEV)
    return t if fmt is None else t.contiguous(memory_format=fmt)


def ibits(n=1):
    return torch.empty(n, device=DEV, dtype=torch.int32)


# ------------------------------------------------------------------ the consumers: (x, w) -> {out, planes, mbs}

def _dconv(transposed, x, w):
    k = K()
    mb = ibits(2)
    xq = k.split16(x, mb)
    wq = k.dconv_wprep(w, transposed, mb)
    y = k.dconv_fwd(x, w, 8, transposed=transposed, split=(xq, mb), wq=wq)
    return dict(out=[y], planes=[xq, wq], mbs=[mb[:1].clone(), mb[1:].clone()])


def _dconv_wgrad16(x, dy):
    k = K()
    xm, dm = ibits(2), ibits(2)
    xq, dq = k.split16(x, xm), k.split16(dy, dm)
    dw, db = k.dconv_wgrad16((xq, xm[:1]), (dq, dm[:1]), tuple(x.shape), 8, bias_grad=True)
    return dict(out=[dw], out_second=[db], planes=[xq, dq], mbs=[xm[:1].clone(), dm[:1].clone()])


def _sconv_fwd(x, w):
    k = K()
    xm, wm = ibits(), ibits()
    xq = k.split_nhwc(x, xm)
    wq = k.sconv_wprep(w, False, wm)
    return dict(out=[k.sconv_fwd((xq, xm), tuple(x.shape), w, 1)], planes=[xq, wq], mbs=[xm, wm])


def _sconv_dgrad2(dy, w):
    k = K()
    dm = ibits()
    dq = k.split_nhwc(dy, dm)
    return dict(out=[k.sconv_dgrad2((dq, dm), (3, 64, 1, 9), w)], planes=[dq], mbs=[dm])


def _sconv_wgrad(x, dy):
    k = K()
    xm, dm = ibits(), ibits()
    xq, dq = k.split_nhwc(x, xm), k.split_nhwc(dy, dm)
    return dict(out=[k.sconv_wgrad((xq, xm), (dq, dm), tuple(x.shape), dy.shape[1], 1)], planes=[xq, dq], mbs=[xm, dm])


def _conv3d_fwd(x, w):
    y, xmax = K().conv3d_fwd(x, w, return_xmax=True)
    return dict(out=[y], planes=[], mbs=[xmax.clone()])


def _conv3d_wgrad(x, dy):
    return dict(out=[K().conv3d_wgrad(x, dy, (5, 7, 7), (2, 3, 3))], planes=[], mbs=[])


def _gemm_f32s(P, Q):
    k = K()
    ps, qs = k.split_planes(P), k.split_planes(Q)
    out = k.gemm_f32s_split(ps, qs, torch.empty(2, 127, 132, device=DEV)[..., :129])
    return dict(out=[out], planes=[ps.hi, ps.lo, qs.hi, qs.lo], mbs=[ps.mb, qs.mb])


def _rows_tn(a, b):
    k = K()
    sa, sb = k.split_planes(a), k.split_planes(b)
    return dict(out=[k.gemm_f32s_rows_tn(sa, sb, 5)], planes=[sa.hi, sa.lo, sb.hi, sb.lo], mbs=[sa.mb, sb.mb])


def _time_chunks(P, Q):
    k = K()
    sp, sq = k.split_rows8(P), k.split_rows8(Q)
    return dict(out=[k.gemm_f32s_time_chunks(sp, sq)], planes=[sp.hi, sp.lo, sq.hi, sq.lo], mbs=[sp.mb, sq.mb])


def _n(shape, seed, fmt=None):
    return dev(det_input(shape, seed), fmt)


# name -> (op, first operand, second operand); the second operand is the weight, or dy for the weight gradients
OPS = {
    "dconv_fwd": (functools.partial(_dconv, False), lambda: _n((1, 64, 40, 257), 1, CL),
                  lambda: 0.03 * _n((64, 64, 5, 5), 2)),
    "dconv_dgrad": (functools.partial(_dconv, True), lambda: _n((1, 64, 40, 257), 3, CL),
                    lambda: 0.03 * _n((64, 64, 5, 5), 4)),
    "dconv_wgrad16": (_dconv_wgrad16, lambda: _n((1, 64, 40, 257), 5, CL), lambda: _n((1, 64, 40, 257), 6, CL)),
    "sconv_fwd": (_sconv_fwd, lambda: _n((1, 64, 5, 7), 7, CL), lambda: 0.05 * _n((192, 64, 3, 3), 8)),
    "sconv_dgrad2": (_sconv_dgrad2, lambda: _n((3, 64, 1, 5), 9, CL), lambda: 0.05 * _n((64, 64, 3, 3), 10)),
    "sconv_wgrad": (_sconv_wgrad, lambda: _n((1, 64, 5, 7), 11, CL), lambda: _n((1, 192, 5, 7), 12, CL)),
    "conv3d_fwd": (_conv3d_fwd, lambda: _n((2, 1, 1, 112, 112), 13), lambda: 0.02 * _n((64, 1, 5, 7, 7), 14)),
    "conv3d_wgrad": (_conv3d_wgrad, lambda: _n((2, 1, 5, 16, 16), 15), lambda: _n((2, 64, 5, 8, 8), 16)),
    "gemm_f32s": (_gemm_f32s, lambda: _n((2, 129, 64), 17), lambda: _n((2, 127, 64), 18)),
    "gemm_f32s_rows_tn": (_rows_tn, lambda: _n((1, 385, 40), 19), lambda: _n((1, 385, 24), 20)),
    "gemm_f32s_time_chunks": (_time_chunks, lambda: _n((2, 129, 61), 21), lambda: _n((2, 127, 61), 22)),
}


@functools.lru_cache(maxsize=None)
def _unit(name):
    op, a, b = OPS[name]
    a, b = a(), b()
    return a, b, op(a, b)


def _exponent_only(mb_scaled, mb_unit):
    """The two max words differ in the exponent field only (sign and mantissa bits equal)."""
    return ((int(mb_scaled.item()) ^ int(mb_unit.item())) & 0x807FFFFF) == 0


@pytest.mark.parametrize("name", list(OPS))
def test_power_of_two_equivariance(name):
    a, b, base = _unit(name)
    op = OPS[name][0]
    assert all(bool(torch.isfinite(o).all()) and float(o.abs().max()) > 0 for o in base["out"])
    for s, t in FACTORS:
        got = op(a * s, b * t)
        for o, o1 in zip(got["out"], base["out"]):
            want = o1 * (s * t)
            assert torch.equal(o, want), (name, s, t, int((o != want).sum()), float((o - want).abs().max()))
        for o, o1 in zip(got.get("out_second", []), base.get("out_second", [])):        # of the second operand only
            assert torch.equal(o, o1 * t), (name, s, t, "second operand's own sum")
        for i, (p, p1) in enumerate(zip(got["planes"], base["planes"])):
            assert torch.equal(p, p1), (name, s, t, f"plane {i} is not the same bytes")
        for i, (m, m1) in enumerate(zip(got["mbs"], base["mbs"])):
            assert _exponent_only(m, m1), (name, s, t, i, hex(int(m.item())), hex(int(m1.item())))
            shift = ((int(m.item()) >> 23) & 0xFF) - ((int(m1.item()) >> 23) & 0xFF)
            assert shift == int(math.log2((s, t)[i])), (name, s, t, i, shift)


@pytest.mark.parametrize("name", list(OPS))
def test_zero_operands(name):
    a, b, base = _unit(name)
    op = OPS[name][0]
    for za, zb in ((True, False), (False, True), (True, True)):
        got = op(torch.zeros_like(a) if za else a, torch.zeros_like(b) if zb else b)
        for o in got["out"]:
            assert bool((o == 0).all()), (name, za, zb, int((o != 0).sum()), int(torch.isnan(o).sum()))
        if zb:
            for o in got.get("out_second", []):
                assert bool((o == 0).all()), (name, "second operand's own sum")
        planes = got["planes"]
        if planes:
            half = len(planes) // 2
            zero_planes = (planes[:half] if za else []) + (planes[half:] if zb else [])
            if len(planes) == 1:
                zero_planes = planes if za else []
            for p in zero_planes:
                assert bool((p.view(torch.uint8) == 0).all()), (name, za, zb, "planes of a zero operand")
        for m, z in zip(got["mbs"], (za, zb)):
            assert (int(m.item()) == 0) == z, (name, za, zb, hex(int(m.item())))


def test_zero_gradient_into_the_exact_fp32_weight_gradient():
    x = _n((2, 64, 37, 257), 30, CL)
    dw, db = K().dconv_wgrad(x, torch.zeros_like(x), 2, bias_grad=True)
    assert bool((dw == 0).all()) and bool((db == 0).all())
    xu = dev(det_input((2, 3, 1, 96, 96), 31, "uint8"))
    dwu = K().conv3d_wgrad(xu, torch.zeros(2, 64, 1, 48, 48, device=DEV), (5, 7, 7), (2, 3, 3))
    assert bool((dwu == 0).all())


@pytest.mark.parametrize("kind", ["dilated", "trunk"])
def test_zero_gradient_into_the_batchnorm_epilogues(kind):
    """dconv_dgrad_bn / sconv_dgrad1_bn on an all-zero dy: dx and the BatchNorm backward sums (and max |dz|) the launch
    leaves in the rows workspace are exact zeros, and so is what bnact_bwd_rows makes of them."""
    k = K()
    if kind == "dilated":
        shape = (2, 64, 6, 257)
        x, gam, bet, alpha, code, stats = tbn._bn_inputs(shape, 0.0, 1.0, "relu")
        w = dev(0.05 * det_input((64, 64, 5, 5), 761))
        mb, mbd = ibits(2), ibits(2)
        g = torch.zeros(shape, device=DEV).contiguous(memory_format=CL)
        gq = k.split16(g, mbd)
        _, wq_t = k.dconv_wprep2(w, mb, mbd)
        dx, rows, ws = k.dconv_dgrad_bn(shape, 2, (gq, mbd), wq_t, x, stats, gam, bet, code, True)
    else:
        shape = (5, 64, 6, 6)
        x, gam, bet, alpha, code, stats = tbn._bn_inputs(shape, 0.0, 1.0, "prelu_c")
        w = dev(0.05 * det_input((64, 64, 3, 3), 763))
        gs = k.split_q(torch.zeros(shape, device=DEV).contiguous(memory_format=CL))
        assert int(gs[1].item()) == 0 and bool((gs[0] == 0).all())
        dx, rows, ws = k.sconv_dgrad1_bn(gs, shape, w, x, stats, gam, bet, code, alpha, True)
    assert bool((dx == 0).all())
    sums = ws[:rows * 4 * 64]
    assert bool((sums == 0).all()), (int((sums != 0).sum()), int(torch.isnan(sums).sum()))
    out = k.bnact_bwd_rows(x, dx, stats, gam, bet, code, alpha, True, rows, ws, q_out=True)
    assert int(getattr(out[0], k.ABSMAX_ATTR).item()) == 0
    assert bool((k.q_view(out[0]).view(torch.float16) == 0).all())
    for t in out[2:]:
        assert t is None or bool((t == 0).all())


# ------------------------------------------------------------------ producer-supplied max at 2^-40

def test_bnact_fwd_max_feeds_the_split_at_small_scale():
    """bnact_fwd's published max |y| with gamma, beta (so y) scaled by 2^-40: exactly max |y|, and split16 / split_q
    from it (avse_split16_known) give the bytes of their own absmax pass on a copy, which are the unit-scale bytes."""
    k = K()
    shape, C = (2, 64, 9, 11), 64
    g = torch.Generator().manual_seed(5)
    x = dev(det_input(shape, 750), CL)
    gam, bet = dev(0.5 + torch.rand(C, generator=g)), dev(0.1 * torch.randn(C, generator=g))
    alpha = dev(0.1 + 0.3 * torch.rand(C, generator=g))
    images = []
    for s in (1.0, LO):
        y, _ = k.bnact_fwd(x, gam * s, bet * s, torch.zeros(C, device=DEV), torch.ones(C, device=DEV), True, 0.1, 1e-5,
                           k.ACT_PRELU, alpha)
        pub = getattr(y, k.ABSMAX_ATTR)
        assert int(pub.item()) == int(y.abs().max().view(torch.int32).item())
        mk, mo = ibits(2), ibits(2)
        known, own = k.split16(y, mk), k.split16(y.clone(memory_format=torch.preserve_format), mo)
        assert torch.equal(known, own) and int(mk[0].item()) == int(mo[0].item())
        qk, qm = k.split_q(y)
        qo, qmo = k.split_q(y.clone(memory_format=torch.preserve_format))
        assert torch.equal(qk, qo) and torch.equal(qm, qmo)
        images.append((y, known, mk[:1].clone()))
    (y1, q1, m1), (ys, qs, ms) = images
    assert torch.equal(ys, y1 * LO) and torch.equal(qs, q1) and _exponent_only(ms, m1)


def test_add_rmsnorm_max_feeds_the_split_at_small_scale():
    """add_rmsnorm_fwd's published max |y| with the weight scaled by 2^-40 -> split_planes (avse_split16_planes_known)
    vs its own absmax pass on a copy, and vs the unit-scale planes."""
    k = K()
    rows, n = 37, 128
    h, r, w = dev(det_input((rows, n), 400)), dev(det_input((rows, n), 401)), dev(1.0 + 0.1 * det_input((n,), 402))
    planes = []
    for s in (1.0, LO):
        y, _, _ = k.add_rmsnorm_fwd(h, r, w * s, 1e-5)
        pub = getattr(y, k.ABSMAX_ATTR)
        assert int(pub.item()) == int(y.abs().max().view(torch.int32).item())
        v = y.view(1, rows, n)
        setattr(v, k.ABSMAX_ATTR, pub)
        known, own = k.split_planes(v), k.split_planes(v.clone())
        assert torch.equal(known.hi, own.hi) and torch.equal(known.lo, own.lo) and torch.equal(known.mb, own.mb)
        planes.append((y, known))
    (y1, p1), (ys, ps) = planes
    assert torch.equal(ys, y1 * LO) and torch.equal(ps.hi, p1.hi) and torch.equal(ps.lo, p1.lo)
    assert _exponent_only(ps.mb, p1.mb)


def test_prelu_gln_bwd_planes_at_small_scale():
    """prelu_gln_bwd(planes=True) writes dx as the planes of the GEMM that consumes it, under a bound of max |dx| it
    computes itself.  With dy scaled by 2^-40: the planes are the unit-scale bytes and the bound moves in the exponent
    only; the consumer's own pass over the fp32 path's dx (split_rows8 under that same bound) gives the same bytes; and
    the GEMM on the producer's planes is 2^-40 times the unit-scale GEMM exactly."""
    k = K()
    shape, C = (2, 64, 37), 64
    x, dy = dev(1.5 * det_input(shape, 900) + 0.3), dev(det_input(shape, 902))
    a = dev(torch.tensor([0.25]))
    gam = dev(0.5 + torch.rand(C, generator=torch.Generator().manual_seed(3)))
    bet = dev(0.1 * det_input((C,), 901))
    wmat = dev(0.1 * det_input((1, 24, C), 903))
    _, st = k.prelu_gln_fwd(x, a, gam, bet)
    runs = []
    for s in (1.0, LO):
        plain = k.prelu_gln_bwd(x, a, gam, st, dy * s)
        q = k.prelu_gln_bwd(x, a, gam, st, dy * s, planes=True)
        sp = k.planes_of(q[0])
        bound = float(sp.mb.view(torch.float32).item())
        m = float(plain[0].abs().max())
        assert m <= bound <= 16 * m, (m, bound)
        dx = plain[0].clone()
        setattr(dx, k.ABSMAX_ATTR, sp.mb.clone())                 # the consumer's pass under the producer's bound
        own = k.split_rows8(dx)
        assert torch.equal(own.hi, sp.hi) and torch.equal(own.lo, sp.lo)
        out = k.gemm_f32s_split(sp.t(), k.split_planes(wmat), torch.empty(2, 24, 40, device=DEV)[..., :37])
        runs.append((plain, sp, out))
    (g1, p1, o1), (gs, ps, os_) = runs
    assert torch.equal(ps.hi, p1.hi) and torch.equal(ps.lo, p1.lo) and _exponent_only(ps.mb, p1.mb)
    assert torch.equal(os_, o1 * LO)
    for u, v in zip(gs, g1):
        assert torch.equal(u, v * LO)
