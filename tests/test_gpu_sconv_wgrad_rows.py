"""GPU tests of the stride-1 trunk weight gradient that handles all 9 taps in one workgroup (csrc/sconv.hip
wgrad9_kernel): a 64-pixel chunk stages its dY rows once and the input rows of the flat (n, h) raster from one row
above its first output row to one row below its last, so where a chunk spans several frames the staged row above a
frame's first row (below its last) belongs to the neighbouring frame and must read as zeros.

Bar: that of test_gpu_sconv.py::test_sconv_wgrad_vs_fp64 (the project's fp32 class): every element within 1e-5 of its
fp64 sum of |terms| against torch.nn.grad.conv2d_weight in fp64."""
import functools

import pytest
import torch

from oracle.det_init import det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last

# (N, ci, H, W, co), all stride 1
EDGE_SHAPES = [(4, 64, 3, 3, 64), (3, 128, 4, 5, 128), (5, 64, 1, 24, 64)]   # the last: every row is top and bottom
CUT_SHAPES = [(37, 128, 12, 12, 128),      # 83.25 chunks: the last partial, a range boundary inside a frame
              (150, 512, 3, 3, 512),       # 21.1 chunks, more ranges than chunks per range (one-chunk ranges)
              (1, 64, 3, 3, 64),           # 9 pixels: less than one chunk
              (2, 64, 28, 28, 64),         # the widest staged segment
              (1, 64, 5, 7, 192)]          # co no multiple of 128
STALE_SHAPES = [(37, 128, 12, 12, 128), (1, 64, 5, 7, 192)]


def K():
    from avse_challenge_amd import kernels
    return kernels


def _split(t):
    m = torch.empty(1, device=DEV, dtype=torch.int32)
    return K().split_nhwc(t.to(DEV).contiguous(memory_format=CL), m), m


def _wgrad(x, dy):
    co = dy.shape[1]
    return K().sconv_wgrad(_split(x), _split(dy), tuple(x.shape), co, 1)


def _truth(x, dy):
    shape = (dy.shape[1], x.shape[1], 3, 3)
    truth = torch.nn.grad.conv2d_weight(x.double(), shape, dy.double(), 1, 1)
    bound = torch.nn.grad.conv2d_weight(x.double().abs(), shape, dy.double().abs(), 1, 1)
    return truth, bound


@functools.lru_cache(maxsize=None)
def _random_case(N, ci, H, W, co):
    """Inputs spanning several decades, their fp64 weight gradient and sum of |terms|, and the kernel's result: computed
    once per shape and left unchanged."""
    seed = 5100 + ci + co + 7 * H + W
    x = det_input((N, ci, H, W), seed) * torch.exp(3.0 * det_input((N, ci, H, W), seed + 1))
    dy = det_input((N, co, H, W), seed + 2)
    truth, bound = _truth(x, dy)
    return x, dy, truth, bound, _wgrad(x, dy)


def _worst(got, truth, bound):
    return float(((got.double().cpu() - truth).abs() / (bound + 1e-30)).max())


@pytest.mark.parametrize("rows", ["both", "first", "last"])
@pytest.mark.parametrize("N,ci,H,W,co", EDGE_SHAPES)
def test_frame_edge_rows_do_not_leak(N, ci, H, W, co, rows):
    """x nonzero (1e2-sized) only on every frame's first and last row ("both"), dy all ones: a tap that read the
    neighbouring frame's row through a chunk's staged halo adds 1e2-sized terms, also where the fp64 sum of |terms| is
    exactly 0 (single-row frames: every kh = 0 and kh = 2 tap).  "first" / "last" keep only that row, which makes the
    kh = 2 / kh = 0 taps exact zeros at every frame height, so the leak from the next / previous frame shows bare."""
    x = torch.zeros((N, ci, H, W))
    edge = 1e2 * (1.0 + det_input((N, ci, 2, W), 5000 + H + W).abs())
    if rows != "last":
        x[:, :, 0, :] = edge[:, :, 0, :]
    if rows != "first":
        x[:, :, H - 1, :] = edge[:, :, 1, :]
    dy = torch.ones((N, co, H, W))
    truth, bound = _truth(x, dy)
    got = _wgrad(x, dy)
    zero = bound == 0
    leaked = int((got.cpu()[zero] != 0).sum())
    worst = _worst(got, truth, bound)
    print(f"wgrad edge {N, ci, H, W, co} {rows}: {int(zero.sum())} exact-zero elements, {leaked} of them nonzero; "
          f"{worst:.2e} of sum|terms|")
    if H == 1 or rows != "both":
        assert int(zero.sum()) >= 3 * co * ci       # at least one kernel row of taps
    assert leaked == 0
    assert worst <= 1e-5, worst
    assert torch.equal(_wgrad(x, dy), got)


@pytest.mark.parametrize("N,ci,H,W,co", CUT_SHAPES)
def test_range_and_chunk_cuts_vs_fp64(N, ci, H, W, co):
    _, _, truth, bound, got = _random_case(N, ci, H, W, co)
    worst = _worst(got, truth, bound)
    print(f"wgrad cuts {N, ci, H, W, co}: {worst:.2e} of sum|terms|")
    assert worst <= 1e-5, worst


@pytest.mark.parametrize("N,ci,H,W,co", CUT_SHAPES)
def test_two_calls_are_bit_identical(N, ci, H, W, co):
    x, dy, _, _, got = _random_case(N, ci, H, W, co)
    assert torch.equal(_wgrad(x, dy), got)


def test_rows_too_wide_for_the_merged_stage_take_the_per_row_kernel():
    """40-pixel rows: the chunk's rows and the two around them do not fit the 9-tap kernel's stage, so the per-row
    kernel (the stride-2 shapes' kernel) still serves them."""
    _, _, truth, bound, got = _random_case(1, 64, 3, 40, 64)
    worst = _worst(got, truth, bound)
    print(f"wgrad wide rows: {worst:.2e} of sum|terms|")
    assert worst <= 1e-5, worst


@pytest.mark.parametrize("N,ci,H,W,co", STALE_SHAPES)
def test_stale_lds_does_not_reach_the_result(N, ci, H, W, co):
    """A split kernel run on all-NaN tensors of the same shape leaves NaN bit patterns in LDS; the weight gradient of
    clean inputs launched right after it is finite and bit-identical to a run without the NaN launch."""
    x, dy, _, _, clean = _random_case(N, ci, H, W, co)
    xs, dys = _split(x), _split(dy)
    nan_x = _split(torch.full((N, ci, H, W), float("nan")))
    nan_dy = _split(torch.full((N, co, H, W), float("nan")))
    dirty = K().sconv_wgrad(nan_x, nan_dy, (N, ci, H, W), co, 1)
    got = K().sconv_wgrad(xs, dys, (N, ci, H, W), co, 1)
    print(f"wgrad stale {N, ci, H, W, co}: NaN launch finite elements {int(torch.isfinite(dirty).sum())}")
    assert torch.isfinite(got).all()
    assert torch.equal(got, clean)
