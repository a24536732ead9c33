"""Length-aware Mamba kernels for ragged batches (avse_scan_fwd_len, avse_cconv_fwd_len[_bf16]; kernels.selective_scan_fwd
and kernels.causal_conv1d_fwd with lengths=): row b of a zero-padded batch is processed exactly as the dense kernel
processes the row cropped to lengths[b] columns.

Scan: b = 6, d = 80 (one full and one partial 64-channel block), seqlen 300, lengths (300, 257, 192, 65, 1, 0): a full
row, one past a chunk, a chunk multiple, one chunk plus 1, a single step and an empty row; z, D, bias and the softplus on.
Conv: width 4 with SiLU, seqlen 200 with lengths (200, 64, 3, 1, 0) and seqlen 300 with (300, 257, 256, 3, 1, 0): both
sides of the dense code's 256 boundary, and rows shorter than the kernel.

The dense conv kernels share the order of the sum (bias, then the taps ascending) but not its rounding: vectorised rows
longer than 256 accumulate with fma, the short-row and the generic kernel round each product and then add.  The
length-aware kernel follows the dense launch's rule per row, so the bitwise comparison crops each row in place (the
layout the batch has); a contiguous copy of the 257-column row would send the dense call itself to its generic kernel
and to the other rounding.  That copy is still compared, to the oracle's tolerance.
All GPU work allocates dirty (tests/_dirty.py)."""
import numpy as np
import pytest
import torch

import _dirty
from oracle import mamba_ref
from oracle.det_init import det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, D, L = 6, 80, 300
LENS = (300, 257, 192, 65, 1, 0)
DTYPES = [torch.float32, torch.bfloat16]


def K():
    from avse_challenge_amd import kernels
    return kernels


def is_plus_zero(t):
    """every element's bits are those of +0"""
    return not bool(t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).any())


def fill_padding(t, lens, fill):
    """a copy of t (b, *, l) with the columns from lens[b] on set to fill"""
    t = t.clone()
    for b, n in enumerate(lens):
        t[b, ..., n:] = fill
    return t


def scan_inputs(dtype, fill=0.0):
    ins = {"u": det_input((B, D, L), 41), "delta": 0.3 * det_input((B, D, L), 42), "B": det_input((B, 16, L), 44),
           "C": det_input((B, 16, L), 45), "z": det_input((B, D, L), 47)}
    ins = {k: fill_padding(v.to(dtype), LENS, fill).to(DEV) for k, v in ins.items()}
    ins.update(A=-torch.exp(0.3 * det_input((D, 16), 43)).to(DEV), D=det_input((D,), 46).to(DEV),
               delta_bias=(0.3 * det_input((D,), 48)).to(DEV))
    return ins


def crop(ins, b, n):
    """row b of the batch cropped to n columns, contiguous: what the dense call gets"""
    return {k: (v[b:b + 1, ..., :n].contiguous() if k in ("u", "delta", "B", "C", "z") else v) for k, v in ins.items()}


@pytest.fixture(scope="module")
def scan_runs():
    """(dtype, reverse) -> (inputs, out, out_z) of the length-aware call on the zero-padded batch, computed once"""
    runs = {}
    mp = pytest.MonkeyPatch()
    for dtype in DTYPES:
        for reverse in (False, True):
            ins = scan_inputs(dtype)
            with _dirty.dirty(mp):
                out, x, out_z = K().selective_scan_fwd(**ins, delta_softplus=True, reverse=reverse, lengths=LENS)
            assert x is None and out.shape == out_z.shape == (B, D, L) and out.dtype == out_z.dtype == dtype
            runs[dtype, reverse] = (ins, out, out_z)
    return runs


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_b_scan_rows_are_bitwise_the_dense_scan_of_the_cropped_row(scan_runs, dtype, reverse, monkeypatch):
    ins, out, out_z = scan_runs[dtype, reverse]
    for b, n in enumerate(LENS):
        assert is_plus_zero(out[b, :, n:]) and is_plus_zero(out_z[b, :, n:]), (b, n)
        if n == 0:
            continue
        with _dirty.dirty(monkeypatch):
            o1, _, oz1 = K().selective_scan_fwd(**crop(ins, b, n), delta_softplus=True, reverse=reverse)
        assert torch.equal(out_z[b, :, :n], oz1[0]), (b, n)
        assert torch.equal(out[b, :, :n], o1[0]), (b, n)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_c_scan_nan_in_the_padding_is_not_used(scan_runs, dtype, reverse, monkeypatch):
    _, out0, oz0 = scan_runs[dtype, reverse]
    ins = scan_inputs(dtype, float("nan"))
    assert bool(torch.isnan(ins["u"][1, :, LENS[1]:]).all()) and bool(torch.isnan(ins["B"][5]).all())
    with _dirty.dirty(monkeypatch):
        out, _, out_z = K().selective_scan_fwd(**ins, delta_softplus=True, reverse=reverse,
                                               lengths=torch.tensor(LENS, dtype=torch.int32, device=DEV))
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(out_z).all())
    assert torch.equal(out, out0) and torch.equal(out_z, oz0)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_d_scan_rows_match_the_fp64_oracle(scan_runs, dtype, reverse):
    """oracle.mamba_ref.selective_scan in fp64 on the cropped rows (flipped for reverse), with the dense scan's
    tolerances of tests/test_gpu_kernels.py: fp32 2e-5 abs + rel, bf16 within 2 bf16 ulp (|err| / (|ref| + 1e-2))."""
    ins, out, out_z = scan_runs[dtype, reverse]
    fl = (lambda t: t.flip(-1)) if reverse else (lambda t: t)
    for b, n in enumerate(LENS):
        if n == 0:
            continue
        c = {k: v.double().cpu() for k, v in crop(ins, b, n).items()}
        c = {k: (fl(v) if k in ("u", "delta", "B", "C", "z") else v) for k, v in c.items()}
        for got, z in ((out_z, c["z"]), (out, None)):
            ref = fl(mamba_ref.selective_scan(c["u"], c["delta"], c["A"], c["B"], c["C"], c["D"], z, c["delta_bias"],
                                              True, acc_dtype=torch.float64))[0].numpy()
            g = got[b, :, :n].double().cpu().numpy()
            if dtype == torch.float32:
                np.testing.assert_allclose(g, ref, atol=2e-5, rtol=2e-5, err_msg=f"row {b} ({n} columns)")
            else:
                rel = np.abs(g - ref) / (np.abs(ref) + 1e-2)
                assert rel.max() <= 2 * 2 ** -8 + 1e-6, (b, n, rel.max())


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_e_scan_accumulates_over_the_valid_columns_only(scan_runs, dtype, reverse, monkeypatch):
    """out_z_acc: valid columns hold acc + the gated output (bitwise the dense accumulating call on the cropped row;
    fp32: bitwise acc + out_z), the columns past them keep acc's bits (1e30 here), and out_z_max is the maximum over
    the valid columns alone."""
    ins, _, oz_with_out = scan_runs[dtype, reverse]
    acc0 = fill_padding(det_input((B, D, L), 49).to(dtype), LENS, 1e30).to(DEV)
    acc = acc0.clone()
    mx = torch.zeros(1, device=DEV, dtype=torch.int32)
    with _dirty.dirty(monkeypatch):
        none, _, oz = K().selective_scan_fwd(**ins, delta_softplus=True, reverse=reverse, return_out=False,
                                             lengths=LENS)
        _, _, got = K().selective_scan_fwd(**ins, delta_softplus=True, reverse=reverse, return_out=False,
                                           out_z_acc=acc, out_z_max=mx, lengths=LENS)
    assert none is None and got.data_ptr() == acc.data_ptr()
    assert torch.equal(oz, oz_with_out)          # writing the pre-gate out or not changes nothing
    top = 0.0
    for b, n in enumerate(LENS):
        assert torch.equal(acc[b, :, n:], acc0[b, :, n:]), (b, n)
        if n == 0:
            continue
        a1 = acc0[b:b + 1, :, :n].clone()          # a copy also for the full row: the dense call adds in place
        with _dirty.dirty(monkeypatch):
            K().selective_scan_fwd(**crop(ins, b, n), delta_softplus=True, reverse=reverse, return_out=False,
                                   out_z_acc=a1)
        assert torch.equal(acc[b, :, :n], a1[0]), (b, n)
        if dtype == torch.float32:
            assert torch.equal(acc[b, :, :n], acc0[b, :, :n] + oz[b, :, :n]), (b, n)
        top = max(top, float(acc[b, :, :n].float().abs().max()))
    assert top < 1e3
    if dtype == torch.float32:
        assert int(mx.cpu()[0]) == int(torch.tensor([top], dtype=torch.float32).view(torch.int32)[0])


def test_scan_wrapper_refuses_lengths_with_a_carried_state():
    ins = scan_inputs(torch.float32)
    h0 = torch.zeros(B, D, 16, device=DEV)
    with pytest.raises(RuntimeError):
        K().selective_scan_fwd(**ins, delta_softplus=True, lengths=LENS, initial_state=h0)
    with pytest.raises(RuntimeError):
        K().selective_scan_fwd(**ins, delta_softplus=True, lengths=LENS, return_last_state=True)
    with pytest.raises(ValueError):
        K().selective_scan_fwd(**ins, delta_softplus=True, lengths=LENS[:3])
    with pytest.raises(RuntimeError):
        K().causal_conv1d_fwd(ins["u"], torch.zeros(D, 4, device=DEV), lengths=LENS,
                              conv_state=torch.zeros(B, D, 4, device=DEV))


# ------------------------------------------------------------------ causal conv

CONV_CASES = [(200, (200, 64, 3, 1, 0)), (300, (300, 257, 256, 3, 1, 0))]
CD, CW = 48, 4


def conv_inputs(l, lens, dtype, fill=0.0):
    x = fill_padding(det_input((len(lens), CD, l), 60 + l).to(dtype), lens, fill).to(DEV)
    return x, det_input((CD, CW), 61).to(DEV), det_input((CD,), 62).to(DEV)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("l,lens", CONV_CASES)
def test_f_conv_rows_are_the_dense_conv_of_the_cropped_row(l, lens, dtype, reverse, monkeypatch):
    x, w, bias = conv_inputs(l, lens, dtype)
    xn = conv_inputs(l, lens, dtype, float("nan"))[0]
    with _dirty.dirty(monkeypatch):
        out = K().causal_conv1d_fwd(x, w, bias, silu=True, reverse=reverse, lengths=lens)
        outn = K().causal_conv1d_fwd(xn, w, bias, silu=True, reverse=reverse,
                                     lengths=torch.tensor(lens, dtype=torch.int32, device=DEV))
    assert out.shape == x.shape and out.dtype == dtype
    assert bool(torch.isfinite(outn).all()) and torch.equal(out, outn)            # (c): NaN padding is not used
    fl = (lambda t: t.flip(-1)) if reverse else (lambda t: t)
    for b, n in enumerate(lens):
        assert is_plus_zero(out[b, :, n:]), (b, n)
        if n == 0:
            continue
        with _dirty.dirty(monkeypatch):
            dense = K().causal_conv1d_fwd(x[b:b + 1, :, :n], w, bias, silu=True, reverse=reverse)     # cropped in place
            copy = K().causal_conv1d_fwd(x[b:b + 1, :, :n].contiguous(), w, bias, silu=True, reverse=reverse)
        assert torch.equal(out[b, :, :n], dense[0]), (b, n)                      # (b): bit for bit
        ref = fl(mamba_ref.causal_conv1d(fl(x[b:b + 1, :, :n].double().cpu()), w.double().cpu(), bias.double().cpu(),
                                         True))[0].numpy()
        rtol = 1e-5 if dtype == torch.float32 else 2 ** -8
        for got in (out[b, :, :n], copy[0]):
            np.testing.assert_allclose(got.double().cpu().numpy(), ref, atol=1e-5, rtol=rtol, err_msg=f"row {b} ({n})")


@pytest.mark.parametrize("dtype", DTYPES)
def test_f_conv_on_the_padded_time_stride(dtype, monkeypatch):
    """the Mamba layout (kernels.bdl_empty's padded time stride, x a channel slice of xz): the vectorised row access,
    bitwise the dense call on each row cropped in place, in both directions."""
    l, lens = 299, (299, 257, 256, 3, 1, 0)                 # rows of 299 columns get a stride of 300
    xz = K().bdl_empty(len(lens), 2 * CD, l, dtype, torch.device(DEV))
    _dirty.poison_(xz)
    xz.copy_(det_input((len(lens), 2 * CD, l), 63).to(dtype))
    x = xz[:, :CD]
    assert x.stride(1) % 4 == 0 and x.stride(1) > l
    _, w, bias = conv_inputs(l, lens, dtype)
    for reverse in (False, True):
        with _dirty.dirty(monkeypatch):
            out = K().causal_conv1d_fwd(x, w, bias, silu=True, reverse=reverse, lengths=lens)
        for b, n in enumerate(lens):
            assert is_plus_zero(out[b, :, n:]), (b, n)
            if n:
                with _dirty.dirty(monkeypatch):
                    dense = K().causal_conv1d_fwd(x[b:b + 1, :, :n], w, bias, silu=True, reverse=reverse)
                assert torch.equal(out[b, :, :n], dense[0]), (b, n, reverse)


# ------------------------------------------------------------------ one resolver for the three ways to give lengths

def test_g_a_list_a_lengths_and_a_device_tensor_give_the_same_bits(monkeypatch):
    """selective_scan_fwd, causal_conv1d_fwd and gln_cl_fwd (the smallest shape of tests/test_gpu_gln_cl_len.py) with the
    same lengths as a list, a Lengths and an int32 device tensor; each set holds a full and an empty row."""
    ins = scan_inputs(torch.float32)
    x, w, bias = conv_inputs(*CONV_CASES[0], torch.float32)
    gl = (7, 6, 1, 0, 3)
    gx = (1.5 * det_input((5, 7, 10, 5), 4305) + 0.3).to(DEV)
    gg, gb = (1.0 + 0.3 * det_input((5,), 4310)).to(DEV), (0.1 * det_input((5,), 4311)).to(DEV)

    def three_ways(lens):
        return [list(lens), K().Lengths(lens, torch.device(DEV, 0)), torch.tensor(lens, dtype=torch.int32, device=DEV)]
    with _dirty.dirty(monkeypatch):
        scans = [K().selective_scan_fwd(**ins, delta_softplus=True, lengths=ln) for ln in three_ways(LENS)]
        convs = [K().causal_conv1d_fwd(x, w, bias, silu=True, lengths=ln) for ln in three_ways(CONV_CASES[0][1])]
        glns = [K().gln_cl_fwd(gx, gg, gb, 1e-8, ln, 0) for ln in three_ways(gl)]
    for other in (1, 2):
        assert torch.equal(scans[0][0], scans[other][0]) and torch.equal(scans[0][2], scans[other][2]), other
        assert torch.equal(convs[0], convs[other]), other
        assert torch.equal(glns[0][0], glns[other][0]) and torch.equal(glns[0][1], glns[other][1]), other
    assert bool(scans[0][2][0].any()) and bool(convs[0][0].any()) and bool(glns[0][0][0].any())     # the full rows ran
