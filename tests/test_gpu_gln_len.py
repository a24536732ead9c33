"""The length-aware forwards of ragged avse4 batches (csrc/gln.hip avse_prelu_gln_fwd_len, avse_dwconv_gln_fwd_len /
_q_len; csrc/dwconv.hip avse_dwconv_fwd_len; csrc/upsample.hip avse_upsample_linear_len).

Sample b of a (B, C, K) batch with lengths[b] valid columns must come out as the dense kernel gives it on the contiguous
slice x[b:b+1, :, :lengths[b]] -- bit for bit, statistics included -- with exact zeros behind it, whatever the padding
columns of x hold (1e30, NaN).  K = 2500 with lengths around 2048 covers the 2048-element loop step, lengths 1 / 2 / 4 /
5 rows shorter than a quadruple and than the dilation halo, 2047 / 2049 / 2499 row tails that are no multiple of 4,
2500 the full row.  Outputs and workspaces are allocated dirty (tests/_dirty.py)."""
import pytest
import torch
import torch.nn.functional as F

from _dirty import dirty
from oracle.det_init import det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
KMAX = 2500
LENGTHS = ([1, 2047, 2049, 2500], [5, 2048, 4, 2499])
FILLS = (1e30, float("nan"))


def K():
    from avse_challenge_amd import kernels
    return kernels


def padded(x, lengths, fill):
    """x (B, C, K) with the columns past lengths[b] overwritten by fill."""
    x = x.clone()
    for b, n in enumerate(lengths):
        x[b, :, n:] = fill
    return x


def gln64(p, gamma, beta):
    """GlobalLayerNorm of baseline/avse4/model.py:225-252 in fp64 on (1, C, L)."""
    mean = p.mean((1, 2), keepdim=True)
    var = ((p - mean) ** 2).mean((1, 2), keepdim=True)
    return gamma.double().view(1, -1, 1) * (p - mean) / (var + 1e-8) ** 0.5 + beta.double().view(1, -1, 1)


def params(C, seed):
    alpha = torch.tensor([0.25])
    gamma = 1.0 + 0.3 * det_input((C,), seed)
    beta = 0.1 * det_input((C,), seed + 1)
    return alpha, gamma, beta


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("lengths", LENGTHS)
@pytest.mark.parametrize("C", [3, 130])
def test_prelu_gln_fwd_len(C, lengths, fill, monkeypatch):
    x = 1.5 * det_input((4, C, KMAX), 4100 + C) + 0.3
    alpha, gamma, beta = params(C, 4110)
    xg = padded(x, lengths, fill).to(DEV)
    ag, gg, bg = alpha.to(DEV), gamma.to(DEV), beta.to(DEV)
    with dirty(monkeypatch):
        y, st = K().prelu_gln_fwd(xg, ag, gg, bg, lengths=lengths)
        y2, st2 = K().prelu_gln_fwd(xg, ag, gg, bg, lengths=lengths)
    assert torch.equal(y, y2) and torch.equal(st, st2), "not repeatable"
    for b, n in enumerate(lengths):
        yd, sd = K().prelu_gln_fwd(x[b:b + 1, :, :n].contiguous().to(DEV), ag, gg, bg)
        assert torch.equal(y[b, :, :n], yd[0]), f"sample {b} (len {n}) differs from the dense kernel on its slice"
        assert torch.equal(st[b], sd[0]), f"sample {b}: statistics"
        assert bool((y[b, :, n:] == 0).all()) and not bool(torch.signbit(y[b, :, n:]).any()), f"sample {b}: tail"
        ref = gln64(F.prelu(x[b:b + 1, :, :n].double(), alpha.double()), gamma, beta)
        for got in (y[b:b + 1, :, :n], yd):                      # the bound of test_prelu_gln_vs_fp64
            torch.testing.assert_close(got.double().cpu(), ref, atol=2e-5, rtol=1e-5)


def dw_ref64(xs, w, dil, alpha, gamma, beta):
    y1 = F.conv1d(xs.double(), w.double(), padding=(w.shape[-1] - 1) // 2 * dil, dilation=dil, groups=xs.shape[1])
    return gln64(torch.where(y1 > 0, y1, alpha.double() * y1), gamma, beta)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("lengths", LENGTHS)
@pytest.mark.parametrize("dil", [1, 128])
@pytest.mark.parametrize("C", [3, 130])
def test_dwconv_gln_fwd_len(C, dil, lengths, fill, monkeypatch):
    x = det_input((4, C, KMAX), 4200 + C + dil)
    w = 0.5 * det_input((C, 1, 3), 4201)
    alpha, gamma, beta = params(C, 4210)
    xg = padded(x, lengths, fill).to(DEV)
    wg, ag, gg, bg = w.to(DEV), alpha.to(DEV), gamma.to(DEV), beta.to(DEV)
    with dirty(monkeypatch):
        y, y1, st = K().dwconv_gln_fwd(xg, wg, dil, ag, gg, bg, lengths=lengths)
        y2, _, st2 = K().dwconv_gln_fwd(xg, wg, dil, ag, gg, bg, lengths=lengths)
    assert torch.equal(y, y2) and torch.equal(st, st2), "not repeatable"
    for b, n in enumerate(lengths):
        yd, y1d, sd = K().dwconv_gln_fwd(x[b:b + 1, :, :n].contiguous().to(DEV), wg, dil, ag, gg, bg)
        assert torch.equal(y[b, :, :n], yd[0]), f"sample {b} (len {n}) differs from the dense kernel on its slice"
        assert torch.equal(y1[b, :, :n], y1d[0]) and torch.equal(st[b], sd[0]), f"sample {b}: y1 / statistics"
        assert bool((y[b, :, n:] == 0).all()) and not bool(torch.signbit(y[b, :, n:]).any()), f"sample {b}: tail"
        ref = dw_ref64(x[b:b + 1, :, :n], w, dil, alpha, gamma, beta)
        bound = 1e-5 * max(1e-6, float(ref.abs().max()))         # the bound of test_dwconv_prelu_gln_fused_vs_fp64
        for got in (y[b:b + 1, :, :n], yd):
            assert float((got.double().cpu() - ref).abs().max()) <= bound


def plane_tail_is_zero(sp, first):
    """The planes' columns first[b] .. kp - 1 of every row of sample b hold 0."""
    cp = sp.hi.stride(1)
    for pl in (sp.hi, sp.lo):
        for b, n in enumerate(first):
            tail = torch.as_strided(pl, (pl.shape[1], cp - n), (cp, 1), pl.storage_offset() + b * pl.stride(0) + n)
            if not bool((tail == 0).all()):
                return False
    return True


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("n,dil", [(2047, 128), (5, 1), (2499, 1)])
def test_dwconv_gln_planes_len_one_sample_is_the_dense_call(n, dil, fill, monkeypatch):
    """B = 1, len < K: the planes, their bound, y1 and the statistics are those of avse_dwconv_gln_fwd_q on the slice,
    bit for bit; the planes are 0 from len up to the padded row length kp."""
    C = 130
    x = det_input((1, C, KMAX), 4300 + n)
    w = 0.5 * det_input((C, 1, 3), 4301)
    alpha, gamma, beta = params(C, 4310)
    wg, ag, gg, bg = w.to(DEV), alpha.to(DEV), gamma.to(DEV), beta.to(DEV)
    with dirty(monkeypatch):
        yq, y1, st = K().dwconv_gln_fwd(padded(x, [n], fill).to(DEV), wg, dil, ag, gg, bg, planes=True, lengths=[n])
    yd, y1d, sd = K().dwconv_gln_fwd(x[:, :, :n].contiguous().to(DEV), wg, dil, ag, gg, bg, planes=True)
    sp, sq = K().planes_of(yq), K().planes_of(yd)
    assert sp.hi.stride(1) == (KMAX + 7) // 8 * 8
    assert torch.equal(sp.mb, sq.mb) and torch.equal(st, sd) and torch.equal(y1[:, :, :n], y1d)
    assert torch.equal(sp.hi[:, :, :n], sq.hi) and torch.equal(sp.lo[:, :, :n], sq.lo)
    assert plane_tail_is_zero(sp, [n])


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("lengths", LENGTHS)
def test_dwconv_gln_planes_len_batch(lengths, fill, monkeypatch):
    """B = 4: the planes decode to the fp32-output result within 2^-21 of max |y| under a bound that is >= max |y| and
    within 0.1 % of it (the asserts of test_dwconv_gln_planes_output), zeros past each length; y1 / statistics equal."""
    C, dil = 130, 128
    x = det_input((4, C, KMAX), 4400)
    w = 0.5 * det_input((C, 1, 3), 4401)
    alpha, gamma, beta = params(C, 4410)
    xg = padded(x, lengths, fill).to(DEV)
    wg, ag, gg, bg = w.to(DEV), alpha.to(DEV), gamma.to(DEV), beta.to(DEV)
    with dirty(monkeypatch):
        y, y1, st = K().dwconv_gln_fwd(xg, wg, dil, ag, gg, bg, lengths=lengths)
        yq, y1q, stq = K().dwconv_gln_fwd(xg, wg, dil, ag, gg, bg, planes=True, lengths=lengths)
    assert torch.equal(st, stq)
    for b, n in enumerate(lengths):
        assert torch.equal(y1[b, :, :n], y1q[b, :, :n])
    sp = K().planes_of(yq)
    bound, m = float(sp.mb.view(torch.float32).item()), float(y.abs().max())
    assert m <= bound <= 1.001 * m, (m, bound)
    bits = int(sp.mb.item())
    e = max(-100, min(100, 14 - (((bits >> 23) & 0xFF) - 127)))
    dec = (sp.hi.double() + sp.lo.double()) * 2.0 ** -e
    assert float((dec - y.double()).abs().max()) <= 2.0 ** -21 * m
    assert plane_tail_is_zero(sp, lengths)


@pytest.mark.parametrize("Kn,lengths,dil", [(75, [1, 3, 75, 14], 1), (2500, [2047, 2049, 2500, 1], 1),
                                            (300, [5, 300, 130, 257], 128)])
def test_dwconv_fwd_len_vs_torch(Kn, lengths, dil, monkeypatch):
    """avse_dwconv_fwd_len against F.conv1d in fp64 on each slice (the bound of test_dwconv_vs_fp64), NaN behind every
    length: it reads 0 there and writes 0 there."""
    C = 7
    x = det_input((4, C, Kn), 4500 + Kn)
    w = det_input((C, 1, 3), 4501)
    with dirty(monkeypatch):
        y = K().dwconv_fwd(padded(x, lengths, float("nan")).to(DEV), w.to(DEV), dil, lengths=lengths)
    for b, n in enumerate(lengths):
        ref = F.conv1d(x[b:b + 1, :, :n].double(), w.double(), padding=dil, dilation=dil, groups=C)
        torch.testing.assert_close(y[b:b + 1, :, :n].double().cpu(), ref, atol=1e-5, rtol=1e-6)
        assert bool((y[b, :, n:] == 0).all())


def upsample_ref64(v, n_in, n_out, Kn, up=32):
    r = F.interpolate(v[:, :, :n_in].double(), scale_factor=up, mode="linear")
    r = F.pad(r, (0, max(0, n_out - r.shape[-1])))[:, :, :n_out]         # model.py:174-176: pad or crop
    return F.pad(r, (0, Kn - n_out))


@pytest.mark.parametrize("klen", [[20, 90, 2390], [40, 100, 2500], [32, 96, 2400]])
def test_upsample_linear_len_vs_torch(klen, monkeypatch):
    """n_in = 1 / 3 / 75 video frames to n_out below, above and at 32 n_in, written into a channel slice of a wider
    tensor.  The weights are exact multiples of 1/64, so against fp64 the error is two product roundings (together
    <= 2^-24 M, the weights sum to 1) and one of the sum (<= 2^-24 M), M = max(|v0|, |v1|) <= the row's max: the
    assert is 2^-23 of the row's max |v| (1 % slack for the second-order terms); integer-valued frames give sums of
    multiples of 1/64 below 2^24 and must come out exactly."""
    C, Tv, Kn, vlen = 5, 75, 2500, [1, 3, 75]
    v = det_input((3, C, Tv), 4600)
    vi = torch.randint(-8, 9, (3, C, Tv), generator=torch.Generator().manual_seed(4601)).float()
    for src, exact in ((v, False), (vi, True)):
        wide = torch.full((3, C + 3, Kn), 7.0, device=DEV)
        with dirty(monkeypatch):
            out = K().upsample_linear_len(padded(src, vlen, float("nan")).to(DEV), vlen, klen, 32, wide[:, 2:2 + C])
        assert out.data_ptr() == wide[:, 2:2 + C].data_ptr()
        assert bool((wide[:, :2] == 7).all()) and bool((wide[:, 2 + C:] == 7).all()), "wrote outside its slice"
        for b in range(3):
            ref = upsample_ref64(src[b:b + 1], vlen[b], klen[b], Kn)
            got = wide[b:b + 1, 2:2 + C].double().cpu()
            if exact:
                assert torch.equal(got, ref)
            else:
                tol = 1.01 * 2.0 ** -23 * src[b, :, :vlen[b]].abs().amax(-1).double().view(1, C, 1)
                assert bool(((got - ref).abs() <= tol).all()), float(((got - ref).abs() / tol).max())
            assert bool((got[:, :, min(32 * vlen[b], klen[b]):] == 0).all())
