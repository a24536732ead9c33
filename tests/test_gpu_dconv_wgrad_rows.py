"""GPU tests of the dilated-conv weight gradient that walks the rows of one residue class h mod d in steps of the
dilation (csrc/dconv.hip rows::wgrad_rows_kernel behind avse_dconv_wgrad16): a unit = (image, class, column chunk,
input-channel half) keeps the five input-row segments of a step in a ring of 6 LDS slots and stages one new segment per
step; persistent workgroups take several units each and restart the ring between them.

Bar: that of test_gpu_kernels.py::test_dconv_wgrad16_vs_fp64 (the project's fp32 class): every element of dW within
1e-5 of its fp64 sum of |terms| against torch.nn.grad.conv2d_weight in fp64 on the CPU, db within 1e-5 of sum |dy|;
inputs as there (det_input x exp(3 det_input))."""
import functools

import pytest
import torch

from oracle.det_init import det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last

# (N, H, W, d).  Ring wrap: a class of >= 7 rows passes the 6-slot wrap, at every dilation.
WRAP = [(1, 15, 64, 2), (1, 29, 64, 4), (1, 57, 64, 8), (1, 113, 64, 16)]
# classes of unequal length, empty classes (H < d), a single row
CLASSES = [(2, 37, 257, 4), (2, 33, 257, 16), (1, 3, 65, 8), (1, 1, 64, 16), (2, 2, 257, 16)]
# column chunks at H = 9: one chunk, a 1-pixel fifth k-step, a partial chunk that is no multiple of 16, the C2 width
# (64, 64, 64, 65), 4 chunks and a partial one; at a dilation whose classes have 4-5 rows and at one with single rows
CHUNKS = [(1, 9, w, d) for w in (64, 65, 127, 257, 300) for d in (2, 16)]
# more units than workgroups (800 > 256: several units per workgroup, the ring restarts), fewer (4)
SCHED = [(5, 20, 300, 16), (1, 4, 64, 2)]
RANDOM = WRAP + CLASSES + CHUNKS + SCHED
STALE = [(2, 37, 257, 4), (1, 113, 64, 16)]
EDGES = [(2, 2 * d + 1, 64, d) for d in (2, 16)] + [(2, 3, 64, d) for d in (2, 16)]


def K():
    from avse_challenge_amd import kernels
    return kernels


def _split(t):
    m = torch.empty(2, device=DEV, dtype=torch.int32)
    return K().split16(t.to(DEV).contiguous(memory_format=CL), m), m[:1]


def _truth(x, dy, d):
    xd, dyd = x.double(), dy.double()
    truth = torch.nn.grad.conv2d_weight(xd, (64, 64, 5, 5), dyd, 1, 2 * d, d)
    bound = torch.nn.grad.conv2d_weight(xd.abs(), (64, 64, 5, 5), dyd.abs(), 1, 2 * d, d)
    return truth, bound


def _worst(got, truth, bound):
    return float(((got.double().cpu() - truth).abs() / (bound + 1e-30)).max())


@functools.lru_cache(maxsize=None)
def _case(N, H, W, d):
    """Inputs over several decades, the fp64 truth and sum of |terms|, the split operands and the kernel's result with
    the bias gradient: computed once per shape and left unchanged."""
    seed = 6100 + 13 * d + 7 * H + W + N
    x = det_input((N, 64, H, W), seed) * torch.exp(3.0 * det_input((N, 64, H, W), seed + 1))
    dy = det_input((N, 64, H, W), seed + 2)
    truth, bound = _truth(x, dy, d)
    xs, dys = _split(x), _split(dy)
    dw, db = K().dconv_wgrad16(xs, dys, (N, 64, H, W), d, bias_grad=True)
    return dy, truth, bound, xs, dys, dw, db


@pytest.mark.parametrize("N,H,W,d", RANDOM)
def test_rows_walk_vs_fp64(N, H, W, d):
    dy, truth, bound, _, _, dw, db = _case(N, H, W, d)
    worst = _worst(dw, truth, bound)
    dyd = dy.double()
    worst_b = float(((db.double().cpu() - dyd.sum((0, 2, 3))).abs() / dyd.abs().sum((0, 2, 3))).max())
    print(f"dconv wgrad rows {N, H, W, d}: dW {worst:.2e} of sum|terms|, db {worst_b:.2e} of sum|dy|")
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    assert worst <= 1e-5, worst
    assert worst_b <= 1e-5, worst_b


@pytest.mark.parametrize("N,H,W,d", WRAP + SCHED + [(2, 33, 257, 16), (1, 9, 127, 2)])
def test_two_calls_are_bit_identical(N, H, W, d):
    _, _, _, xs, dys, dw, db = _case(N, H, W, d)
    dw2, db2 = K().dconv_wgrad16(xs, dys, (N, 64, H, W), d, bias_grad=True)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)
    dw3 = K().dconv_wgrad16(xs, dys, (N, 64, H, W), d)
    dw4 = K().dconv_wgrad16(xs, dys, (N, 64, H, W), d)
    assert torch.equal(dw4, dw3)
    assert torch.equal(dw3, dw)          # the bias tile is a separate accumulator


@pytest.mark.parametrize("rows", ["first", "last", "both"])
@pytest.mark.parametrize("N,H,W,d", EDGES)
def test_vertical_edges_are_exact(N, H, W, d, rows):
    """x nonzero (1e2-sized) only in every image's first row, last row, or both; dy all ones.  A tap whose input row
    lies outside the image, or in no nonzero row, has an fp64 sum of |terms| of exactly 0 and must come out as exactly
    0.0: a ring slot that still held the previous unit's or the neighbouring image's row adds 1e2-sized terms there."""
    x = torch.zeros((N, 64, H, W))
    edge = 1e2 * (1.0 + det_input((N, 64, 2, W), 6000 + H + d).abs())
    if rows != "last":
        x[:, :, 0, :] = edge[:, :, 0, :]
    if rows != "first":
        x[:, :, H - 1, :] = edge[:, :, 1, :]
    dy = torch.ones((N, 64, H, W))
    truth, bound = _truth(x, dy, d)
    xs, dys = _split(x), _split(dy)
    got = K().dconv_wgrad16(xs, dys, (N, 64, H, W), d)
    zero = bound == 0
    leaked = int((got.cpu()[zero] != 0).sum())
    worst = _worst(got, truth, bound)
    print(f"dconv wgrad rows edge {N, H, W, d} {rows}: {int(zero.sum())} exact-zero elements, {leaked} of them "
          f"nonzero; {worst:.2e} of sum|terms|")
    if H == 3 or rows != "both":                   # (H = 2 d + 1 with both rows: every kernel row meets one of them)
        assert int(zero.sum()) >= 2 * 5 * 64 * 64  # two kernel rows of taps or more see no nonzero row
    assert leaked == 0
    assert worst <= 1e-5, worst


@pytest.mark.parametrize("N,H,W,d", STALE)
def test_stale_lds_does_not_reach_the_result(N, H, W, d):
    """A launch whose split operands are fp16 NaN bit patterns throughout leaves them in every ring slot and dY buffer;
    the launch on clean operands right after it is finite and bit-identical to the run without it."""
    _, _, _, xs, dys, dw, db = _case(N, H, W, d)
    nan_x, nan_dy = torch.empty_like(xs[0]), torch.empty_like(dys[0])
    nan_x.view(torch.int16).fill_(0x7E00)
    nan_dy.view(torch.int16).fill_(0x7E00)
    dirty = K().dconv_wgrad16((nan_x, xs[1]), (nan_dy, dys[1]), (N, 64, H, W), d)
    got, gdb = K().dconv_wgrad16(xs, dys, (N, 64, H, W), d, bias_grad=True)
    print(f"dconv wgrad rows stale {N, H, W, d}: NaN launch finite elements {int(torch.isfinite(dirty).sum())}")
    assert not torch.isfinite(dirty).any()
    assert torch.isfinite(got).all() and torch.isfinite(gdb).all()
    assert torch.equal(got, dw) and torch.equal(gdb, db)
