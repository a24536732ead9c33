"""Channels-last GroupNorm(1, N) with a per-row valid extent (csrc/gln_cl.hip avse_gln_cl_fwd_len, kernels.gln_cl_fwd):
the intra / inter / input norms of DPMamba's ragged path.

Row b of x (B, R, C, N) is valid for r < lengths[b] (axis 0) or c < lengths[b] (axis 1).  It must come out as the same
entry point gives it on the row cropped and alone (B = 1, the axis cut to lengths[b], contiguous) -- bit for bit,
statistics included -- with +0 at every invalid position, whatever x and res hold there (1e30, NaN), and must agree
with fp64 GroupNorm over the valid elements to the bound the project holds gLN to (atol 2e-5, rtol 1e-5 on inputs of
scale 1.5 det_input + 0.3: tests/test_gpu_kernels.py::test_prelu_gln_vs_fp64).  N = 5, 130 and 301 take the dword
accesses, N = 64 and 600 the 16-B ones; 301 and 600 give a lane more than one quadruple of a line (a wave covers 256
channels per trip).  (7, 10) = 70 lines are four workgroups of 16 and a partial one, (40, 50) = 2000 lines cross the
1024-thread loop of the row statistics; the lengths hold a full row, a single line group and an empty row.  Outputs
and workspaces are allocated dirty."""
import pytest
import torch

from _dirty import dirty
from oracle.det_init import det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILLS = (1e30, float("nan"))
# (B, R, C) as axis 0 sees it, lengths; axis 1 takes the small shape with R and C swapped
CASES = [((5, 7, 10), 5, (7, 6, 1, 0, 3)), ((5, 7, 10), 64, (7, 6, 1, 0, 3)), ((5, 7, 10), 130, (7, 6, 1, 0, 3)),
         ((2, 40, 50), 64, (40, 33)), ((2, 3, 5), 301, (3, 1)), ((2, 3, 5), 600, (3, 1))]


def K():
    from avse_challenge_amd import kernels
    return kernels


def valid_mask(shape, lengths, axis):
    B, R, C = shape
    idx = torch.arange(R)[None, :, None].expand(B, R, C) if axis == 0 else torch.arange(C)[None, None, :].expand(B, R, C)
    return idx < torch.tensor(lengths)[:, None, None]


def crop(t, b, n, axis):
    """Row b's valid part of a (B, R, C, N) tensor (axis: the tensor's own ragged axis), contiguous, B = 1."""
    return (t[b:b + 1, :n] if axis == 0 else t[b:b + 1, :, :n]).contiguous()


def gn64(x, gamma, beta):
    """nn.GroupNorm(1, N, eps=1e-8) in fp64 over all of x (..., N)."""
    x = x.double()
    mean = x.mean()
    var = ((x - mean) ** 2).mean()
    return (x - mean) / (var + 1e-8) ** 0.5 * gamma.double() + beta.double()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_gln_cl_fwd_len(case, axis, fill, monkeypatch):
    (B, R, C), N, lengths = case
    if axis == 1 and (R, C) == (7, 10):
        R, C = C, R
    shape = (B, R, C)
    x = 1.5 * det_input((B, R, C, N), 4300 + N + axis) + 0.3
    res_n = 1.5 * det_input((B, R, C, N), 4400 + N + axis) + 0.3          # res in the plain output layout
    gamma = 1.0 + 0.3 * det_input((N,), 4310)
    beta = 0.1 * det_input((N,), 4311)
    ok = valid_mask(shape, lengths, axis)
    fillt = torch.tensor(fill)
    xg = torch.where(ok[..., None], x, fillt).to(DEV)
    gg, bg = gamma.to(DEV), beta.to(DEV)
    ldev = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    for with_res in (False, True):
        for tr in (False, True):
            # the output's layout: (B, C, R, N) when transposed, where the ragged axis is the other one
            oax = 1 - axis if tr else axis
            ook = ok.transpose(1, 2) if tr else ok
            res = (res_n.transpose(1, 2).contiguous() if tr else res_n) if with_res else None
            rg = torch.where(ook[..., None], res, fillt).to(DEV) if with_res else None
            what = f"axis {axis}, res {with_res}, transpose_out {tr}"
            with dirty(monkeypatch):
                y, st = K().gln_cl_fwd(xg, gg, bg, 1e-8, ldev, axis, res=rg, transpose_out=tr)
                y2, st2 = K().gln_cl_fwd(xg, gg, bg, 1e-8, list(lengths), axis, res=rg, transpose_out=tr)
            assert y.shape == ((B, C, R, N) if tr else (B, R, C, N)) and st.shape == (B, 2)
            assert torch.equal(y, y2) and torch.equal(st, st2), f"{what}: not repeatable"
            assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(st).all()), what
            inv = ~ook.to(DEV)
            assert bool((y[inv] == 0).all()) and not bool(torch.signbit(y[inv]).any()), f"{what}: invalid positions"
            for b, n in enumerate(lengths):
                if n == 0:
                    assert not bool(y[b].any()) and not bool(st[b].any()), f"{what}: the empty row"
                    continue
                with dirty(monkeypatch):
                    yd, sd = K().gln_cl_fwd(crop(x, b, n, axis).to(DEV), gg, bg, 1e-8, [n], axis,
                                            res=crop(res, b, n, oax).to(DEV) if with_res else None, transpose_out=tr)
                got = crop(y, b, n, oax)
                assert torch.equal(got, yd), f"{what}: row {b} (len {n}) differs from the call on its crop"
                assert torch.equal(st[b], sd[0]), f"{what}: row {b} statistics"
                ref = gn64(crop(x, b, n, axis), gamma, beta)
                ref = ref.transpose(1, 2) if tr else ref
                if with_res:
                    ref = ref + crop(res, b, n, oax).double()
                torch.testing.assert_close(got.double().cpu(), ref, atol=2e-5, rtol=1e-5)
                xv = crop(x, b, n, axis).double()
                torch.testing.assert_close(st[b].double().cpu(),
                                           torch.stack([xv.mean(), (xv.var(unbiased=False) + 1e-8) ** -0.5]),
                                           atol=2e-5, rtol=1e-5)


def test_argument_checks():
    x = torch.zeros(2, 3, 4, 8, device=DEV)
    g = torch.ones(8, device=DEV)
    with pytest.raises(ValueError):
        K().gln_cl_fwd(x, g, g, 1e-8, [3, 3], 2)
    with pytest.raises(ValueError):
        K().gln_cl_fwd(x, g, g, 1e-8, [3, 4], 0)                          # past the axis
    with pytest.raises(ValueError):
        K().gln_cl_fwd(x, g, g, 1e-8, [3], 0)
    with pytest.raises(ValueError):
        K().gln_cl_fwd(x, g, g, 1e-8, [3, 3], 0, res=x, transpose_out=True)       # res in the output's layout
    ldev = torch.tensor([9, -1], dtype=torch.int32, device=DEV)           # a device tensor is clamped: 4, 0
    y, st = K().gln_cl_fwd(x, g, torch.zeros_like(g), 1e-8, ldev, 1)
    assert y.shape == x.shape and not bool(y.any()) and st[:, 0].tolist() == [0.0, 0.0]
