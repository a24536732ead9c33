"""Length-aware eval BatchNorm -> act (avse_bnact_fwd_len / avse_bnact_fwd_q_len; kernels.bnact_fwd with lengths) and
the lip-to-audio gather (avse_gather_nearest_len) against the dense kernels / torch on each row cropped to its length.

BatchNorm: C = 64, T = 9, F = 5, lengths (9, 4, 1), NaN in the input's padding.  Every layout the avse1 ragged path uses
-- contiguous (B, C, T, F) and (B, C, T, 1, F), channels-last (B, T, F, C) and (B, T, 1, F, C), frame-major
(B T, C, 1, F) in both formats, and the TCN's time-major rows with the window offset of its symmetric chomp -- with
each activation; the split ("q") output for the channels-last 4-D forms, compared with the split of the dense output
under the same max word.  With C S = 2880 the contiguous forms run the 4-vector kernel with vectors that straddle time
steps (5 values per step).  All GPU work allocates dirty (tests/_dirty.py)."""
import pytest
import torch

import _dirty
from oracle.det_init import det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, C, T, F = 3, 64, 9, 5
LEN = (9, 4, 1)
ACTS = ("none", "relu", "prelu")


def to_layout(x, layout):
    """x (b, t, F, C) logical -> (tensor in `layout`, frames argument)."""
    b, t = x.shape[:2]
    if layout == "nchw":
        return x.permute(0, 3, 1, 2).contiguous(), None
    if layout == "nhwc":
        return x.contiguous().permute(0, 3, 1, 2), None
    if layout == "ncdhw":
        return x.permute(0, 3, 1, 2).contiguous().view(b, C, t, 1, F), None
    if layout == "ndhwc":
        return x.contiguous().view(b, t, 1, F, C).permute(0, 4, 1, 2, 3), None
    if layout == "frames_nchw":
        return x.permute(0, 1, 3, 2).contiguous().view(b * t, C, 1, F), t
    if layout == "frames_nhwc":
        return x.contiguous().view(b * t, 1, F, C).permute(0, 3, 1, 2), t
    raise KeyError(layout)


def from_layout(y, layout, b, t):
    """back to (b, t, F, C) logical."""
    if layout in ("nchw", "nhwc"):
        return y.permute(0, 2, 3, 1)
    if layout == "ncdhw":
        return y.reshape(b, C, t, F).permute(0, 2, 3, 1)
    if layout == "ndhwc":
        return y.permute(0, 2, 3, 4, 1).reshape(b, t, F, C)
    if layout == "frames_nchw":
        return y.reshape(b, t, C, F).permute(0, 1, 3, 2)
    return y.permute(0, 2, 3, 1).reshape(b, t, F, C)


@pytest.fixture(scope="module")
def bn():
    """BatchNorm parameters and the (B, T, F, C) input, NaN at t >= LEN[b]; made once."""
    x = (2.0 * det_input((B, T, F, C), 6200) + 0.3).to(DEV)
    for b, n in enumerate(LEN):
        x[b, n:] = float("nan")
    p = dict(gamma=(1.0 + 0.2 * det_input((C,), 6201)).to(DEV), beta=(0.3 * det_input((C,), 6202)).to(DEV),
             rm=(0.2 * det_input((C,), 6203)).to(DEV), rv=(1.0 + 0.5 * det_input((C,), 6204).abs()).to(DEV),
             alpha=(0.25 + 0.1 * det_input((C,), 6205)).to(DEV))
    return x, p


def run(K, x, p, act, **kw):
    code = ACTS.index(act)
    return K.bnact_fwd(x, p["gamma"], p["beta"], p["rm"], p["rv"], False, 0.1, 1e-5, code,
                       p["alpha"] if act == "prelu" else None, **kw)[0]


def max_bits(t):
    return int(t.abs().max().view(torch.int32))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("layout", ["nchw", "nhwc", "ncdhw", "ndhwc", "frames_nchw", "frames_nhwc"])
def test_plain_output(bn, layout, act, monkeypatch):
    from avse_challenge_amd import kernels as K
    x, p = bn
    xl, frames = to_layout(x, layout)
    with _dirty.dirty(monkeypatch):
        y = run(K, xl, p, act, lengths=LEN, frames=frames)
    assert y.shape == xl.shape and y.stride() == xl.stride()
    got = from_layout(y, layout, B, T)
    want_max = 0
    for b, n in enumerate(LEN):
        ref = run(K, to_layout(x[b:b + 1, :n], layout)[0], p, act)          # the dense kernel on the cropped row
        ref = from_layout(ref, layout, 1, n)
        assert torch.equal(got[b, :n], ref[0]), (b, n)
        assert not got[b, n:].any(), (b, n)                                 # exact zeros where the input is NaN
        want_max = max(want_max, max_bits(ref))
    assert int(K._known_absmax(y)) == want_max                              # the max of the valid elements only


@pytest.mark.parametrize("act", ACTS)
def test_split_output(bn, act, monkeypatch):
    from avse_challenge_amd import kernels as K
    x, p = bn
    xl, _ = to_layout(x, "nhwc")
    with _dirty.dirty(monkeypatch):
        y = run(K, xl, p, act, lengths=LEN, q_out=True)
        plain = run(K, xl, p, act, lengths=LEN)
    assert K.is_split_q(y)
    mb = K._known_absmax(y)
    assert int(mb) == int(K._known_absmax(plain))                           # the exact valid max, not a bound
    q = K.q_view(y).view(B, T * F, 4 * C)
    for b, n in enumerate(LEN):
        ref = run(K, to_layout(x[b:b + 1, :n], "nhwc")[0], p, act)
        K._set_absmax(ref, mb)                                              # split under the batch's max word
        rq, _ = K.split_q(ref)
        assert torch.equal(q[b, :n * F], rq), (b, n)
        assert not q[b, n * F:].any(), (b, n)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("q_out", [False, True], ids=["plain", "q"])
def test_time_major_rows_with_the_chomp_window(act, q_out, monkeypatch):
    """The TCN's form: (B, To, C) time-major rows read as a (B, C, To, 1) channels-last view, BatchNorm over the conv's
    unchomped To = T + 4 rows, valid window [2, 2 + len_b)."""
    from avse_challenge_amd import kernels as K
    from avse_challenge_amd.layers import time_major_4d
    h, To = 2, T + 4
    x = (det_input((B, To, C), 6210) + 0.1).to(DEV)
    p = dict(gamma=(1.0 + 0.2 * det_input((C,), 6211)).to(DEV), beta=(0.3 * det_input((C,), 6212)).to(DEV),
             rm=(0.2 * det_input((C,), 6213)).to(DEV), rv=(1.0 + 0.5 * det_input((C,), 6214).abs()).to(DEV),
             alpha=(0.25 + 0.1 * det_input((C,), 6215)).to(DEV))
    ref = run(K, time_major_4d(x), p, act).squeeze(3).transpose(1, 2)       # dense, finite input
    xn = x.clone()
    for b, n in enumerate(LEN):
        xn[b, :h] = float("nan")
        xn[b, h + n:] = float("nan")
    with _dirty.dirty(monkeypatch):
        y = run(K, time_major_4d(xn), p, act, lengths=LEN, t_off=h, q_out=q_out)
    assert K.is_split_q(y) == q_out
    want = torch.zeros_like(ref)
    for b, n in enumerate(LEN):
        want[b, h:h + n] = ref[b, h:h + n]
    assert int(K._known_absmax(y)) == max_bits(want)
    if q_out:
        w4 = time_major_4d(want.contiguous())
        K._set_absmax(w4, K._known_absmax(y))
        assert torch.equal(K.q_view(y), K.split_q(w4)[0])
    else:
        assert torch.equal(y.squeeze(3).transpose(1, 2), want)


def test_wrapper_refusals(bn):
    from avse_challenge_amd import kernels as K
    x, p = bn
    xl, _ = to_layout(x, "nhwc")
    with pytest.raises(RuntimeError):                                        # training mode
        K.bnact_fwd(xl, p["gamma"], p["beta"], p["rm"], p["rv"], True, 0.1, 1e-5, 1, None, lengths=LEN)
    with pytest.raises(RuntimeError):                                        # a residual
        K.bnact_fwd(xl, p["gamma"], p["beta"], p["rm"], p["rv"], False, 0.1, 1e-5, 1, None, res=xl, lengths=LEN)
    with pytest.raises(ValueError):
        run(K, xl, p, "relu", lengths=(9, 4, 10))                            # longer than the time axis
    with pytest.raises(ValueError):
        run(K, xl, p, "relu", lengths=(9, 4))


# ---- the nearest gather
G_T, G_TV = (126, 72, 47, 7), (25, 14, 9, 12)             # the last row has fewer audio frames than lip frames


@pytest.mark.parametrize("c,extra", [(512, 1028), (6, 1)], ids=["vec4", "scalar"])
def test_gather_nearest_matches_the_dense_index(c, extra, monkeypatch):
    from avse_challenge_amd import kernels as K
    vis = det_input((len(G_T), max(G_TV), c), 6220).to(DEV)
    for b, tv in enumerate(G_TV):
        vis[b, tv:] = float("nan")
    with _dirty.dirty(monkeypatch):
        out = K.gather_nearest_len(vis, G_TV, G_T, max(G_T), extra=extra)
    assert out.shape == (len(G_T), max(G_T), c + extra)
    assert bool(torch.isnan(out[:, :, c:]).all())                           # the right columns are the caller's
    for b, (t, tv) in enumerate(zip(G_T, G_TV)):
        idx = torch.div(torch.arange(t, device=DEV) * tv, t, rounding_mode="floor")      # avse1.AVNet.forward
        assert torch.equal(out[b, :t, :c], vis[b].index_select(0, idx)), b
        assert not out[b, t:, :c].any(), b
    with pytest.raises(ValueError):
        K.gather_nearest_len(vis, (26, 14, 9, 12), G_T, max(G_T))          # more lip frames than the tensor holds
    with pytest.raises(ValueError):
        K.gather_nearest_len(vis, (25, 14, 0, 12), G_T, max(G_T))          # no lip frame
