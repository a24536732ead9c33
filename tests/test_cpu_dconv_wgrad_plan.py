"""Host plan of the dilated-conv weight gradient (csrc/dconv.hip rows::make_plan behind avse_dconv_wgrad16_plan): units,
steps, 1-KB LDS-DMA pieces per launch, partial slabs, LDS bytes per workgroup, workgroups.  No GPU.

The decomposition: unit = (image n, residue class rho of h mod d, column chunk, input-channel half ib), listed in that
order with ib fastest; a column chunk is 64 columns, the last one the rest of the row, or 64 + the rest where the rest is
at most 16 columns; a unit of T > 0 output rows stages T + 4 input segments of (16 ks + 4 d) / 8 pieces and T dY segments
of 4 ks pieces (ks = the chunk's k-steps of 16 pixels), an empty unit nothing.

DMA pieces per launch at the C2 shape (32, 376, 257) against the kernel this one replaced, whose 48,320 chunks each
cost 5 workgroups 32 + 2 d pieces (computed below, not chosen):
    d = 2: 2,570,240 / 8,697,600 = 0.296      d = 4: 2,690,048 / 9,664,000 = 0.278
    d = 8: 2,941,952 / 11,596,800 = 0.254     d = 16: 3,494,912 / 15,462,400 = 0.226"""
import ctypes
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "avse_challenge_amd", "libavse_hip.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libavse_hip.so not built (run __graft_entry__.build)")

C2 = (32, 376, 257)
DILS = (2, 4, 8, 16)
SLAB_BYTES = 4 * (25 * 64 * 64 + 64)          # one partial dW slab and its db row


def _lib():
    from avse_challenge_amd import _lib
    return _lib.lib()


def _plan(N, H, W, d):
    out = (ctypes.c_int64 * 6)()
    assert _lib().avse_dconv_wgrad16_plan(N, H, W, d, out) == 0, (N, H, W, d)
    return dict(zip(("units", "steps", "pieces", "slabs", "lds", "workgroups"), out))


def _chunks(W):
    """(first column, width) of a row's column chunks."""
    q, r = divmod(W, 64)
    n = q + (1 if r > 16 else 0)
    return [(64 * c, W - 64 * c if c == n - 1 else 64) for c in range(n)]


def _units(N, H, W, d):
    """The unit list in launch order: (n, rho, first column, width, ib, output rows)."""
    return [(n, rho, w0, cw, ib, list(range(rho, H, d)))
            for n in range(N) for rho in range(d) for (w0, cw) in _chunks(W) for ib in range(2)]


def _unit_pieces(rows, cw, d):
    ks = (cw + 15) // 16
    return (len(rows) + 4) * ((16 * ks + 4 * d) // 8) + len(rows) * 4 * ks if rows else 0


@pytest.mark.parametrize("d", DILS)
def test_c2_pieces_equal_the_closed_form_and_undercut_the_old_kernel(d):
    N, H, W = C2
    p = _plan(N, H, W, d)
    assert _chunks(W) == [(0, 64), (64, 64), (128, 64), (192, 65)]
    assert p["units"] == N * 4 * d * 2
    assert p["steps"] == N * 4 * 2 * H
    # every step stages one dY segment (16 pieces) and one input segment (8 + d / 2) ...
    steady = p["steps"] * (16 + 8 + d // 2)
    # ... every unit 4 more input segments than it has steps (the ring's warm-up; all d classes are non-empty) ...
    warmup = p["units"] * 4 * (8 + d // 2)
    # ... and the 65-column chunk a fifth k-step: 4 more dY pieces a step, 2 more pieces per input segment
    wide = N * 2 * (H * 4 + (H + 4 * d) * 2)
    assert p["pieces"] == steady + warmup + wide
    old = N * ((H * W + 63) // 64) * 5 * (32 + 2 * d)
    assert N * ((H * W + 63) // 64) == 48_320
    print(f"d = {d}: {p['pieces']} pieces, old kernel {old}, ratio {p['pieces'] / old:.3f}")
    assert p["pieces"] < old


@pytest.mark.parametrize("d", DILS)
def test_c2_lds_workgroups_and_workspace(d):
    N, H, W = C2
    p = _plan(N, H, W, d)
    assert p["lds"] <= 163_840
    assert p["lds"] == 6 * (80 + 4 * d) * 128 + 2 * 80 * 256          # the ring and two dY buffers, 5 k-steps wide
    assert p["workgroups"] == 256 and p["slabs"] == 128
    nb = _lib().avse_dconv_wgrad16_workspace_bytes(N, H, W)
    assert nb % SLAB_BYTES == 0                                        # whole slabs
    assert nb == p["slabs"] * SLAB_BYTES


@pytest.mark.parametrize("N,H,W,d", [(2, 37, 257, 4), (1, 3, 65, 8), (5, 20, 300, 16), (1, 9, 127, 2)])
def test_units_cover_every_pixel_once(N, H, W, d):
    """The plan enumerated in Python: for each ib, the units' rows x columns cover every (n, h, column) exactly once;
    units, steps and pieces are the library's; the workspace covers this launch's slabs."""
    p = _plan(N, H, W, d)
    units = _units(N, H, W, d)
    assert len(units) == p["units"]
    assert sum(len(u[5]) for u in units) == p["steps"]
    assert sum(_unit_pieces(u[5], u[3], d) for u in units) == p["pieces"]
    for ib in range(2):
        seen = {}
        for (n, rho, w0, cw, b, rows) in units:
            if b != ib:
                continue
            assert 1 <= cw <= 80 and w0 + cw <= W
            for h in rows:
                for w in range(w0, w0 + cw):
                    seen[(n, h, w)] = seen.get((n, h, w), 0) + 1
        assert len(seen) == N * H * W and set(seen.values()) == {1}
    assert p["workgroups"] == min(256, p["units"]) and p["workgroups"] % 2 == 0
    assert p["slabs"] == p["workgroups"] // 2
    assert _lib().avse_dconv_wgrad16_workspace_bytes(N, H, W) >= p["slabs"] * SLAB_BYTES


def test_shapes_the_entry_point_refuses_have_no_plan():
    out = (ctypes.c_int64 * 6)()
    assert _lib().avse_dconv_wgrad16_plan(1, 8, 63, 2, out) != 0          # W < 64
    assert _lib().avse_dconv_wgrad16_plan(1, 8, 64, 3, out) != 0          # dilation
    assert _lib().avse_dconv_wgrad16_plan(0, 8, 64, 2, out) != 0
