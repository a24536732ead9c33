"""GPU parity tests: HIP kernels (through the C ABI) vs the golden vectors and the CPU oracle.

Tolerances (fp32 path): the reference arithmetic is fp32; our kernels use fp32 with a different
summation order and exp2-based exponentials, so element-wise agreement is ~1e-6 relative.
Stated per test; BASELINE north_star bar for waveforms is RMS <= 1e-4.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from oracle import mamba_ref, stft_ref
from oracle.det_init import det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"


def K():
    from avse_challenge_amd import kernels
    return kernels


def g2t(a, dtype=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(DEV, dtype)


def close(a, b, atol, rtol=0.0, what=""):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    np.testing.assert_allclose(a, b, atol=atol, rtol=rtol, err_msg=what)


# ------------------------------------------------------------------ selective scan: goldens

def test_scan_fwd_golden_fp32():
    g = load_golden("scan_fp32")
    ins = {k: g2t(g[k]) for k in ("u", "delta", "A", "B", "C", "D", "z", "delta_bias")}
    out, x, out_z = K().selective_scan_fwd(**ins, delta_softplus=True)
    close(out_z, g["out_z"], 2e-5, 2e-5, "out_z")
    close(x[:, :, -1, 1::2], g["last_state"], 2e-5, 2e-5, "last state")
    out2, _, none = K().selective_scan_fwd(**{**ins, "z": None}, delta_softplus=True)
    assert none is None
    close(out2, g["out_noz"], 2e-5, 2e-5, "out (no z)")
    out3, _, _ = K().selective_scan_fwd(ins["u"], ins["delta"].abs(), ins["A"], ins["B"][:, 0], ins["C"][:, 0])
    close(out3, g["out_3d_nodz"], 2e-5, 2e-5, "3-d B/C, no D/bias/softplus")


def test_scan_bwd_golden_fp32():
    g = load_golden("scan_fp32")
    ins = {k: g2t(g[k]) for k in ("u", "delta", "A", "B", "C", "D", "z", "delta_bias")}
    out, x, out_z = K().selective_scan_fwd(**ins, delta_softplus=True)
    res = K().selective_scan_bwd(ins["u"], ins["delta"], ins["A"], ins["B"], ins["C"], ins["D"], ins["z"],
                                 ins["delta_bias"], g2t(g["dout"]), x, out, None, True, True)
    du, ddelta, dA, dB, dC, dD, dbias, dz, oz = res
    close(oz, g["out_z"], 2e-5, 2e-5, "recomputed out_z")
    for name, v in (("du", du), ("ddelta", ddelta), ("dA", dA), ("dB", dB), ("dC", dC), ("dD", dD),
                    ("ddelta_bias", dbias), ("dz", dz)):
        ref = g["d" + name[1:]] if name != "ddelta_bias" else g["ddelta_bias"]
        scale = max(1.0, float(np.abs(ref).max()))
        close(v, ref, 5e-5 * scale, 1e-4, name)


def test_scan_fwd_golden_bf16():
    g = load_golden("scan_bf16")
    bf = lambda k: g2t(g[k], torch.bfloat16)
    out, _, out_z = K().selective_scan_fwd(bf("u"), bf("delta"), g2t(g["A"]), bf("B"), bf("C"), g2t(g["D"]), bf("z"),
                                           g2t(g["delta_bias"]), True)
    assert out_z.dtype == torch.bfloat16
    ref = g["out_z"]
    rel = np.abs(out_z.float().cpu().numpy() - ref) / (np.abs(ref) + 1e-2)
    assert rel.max() <= 2 * 2 ** -8 + 1e-6, rel.max()   # within 2 bf16 ulp of the fp32-accumulated reference


@pytest.mark.parametrize("reverse", [False, True])
def test_scan_bwd_bf16_vs_oracle(reverse):
    """bf16 u/delta/z/B/C/dout (C5): every gradient vs fp64 autograd through the oracle on the same bf16 values.
    fp32 outputs (dA, dB, dC, dD, ddelta_bias) as tight as the fp32 test; bf16 outputs (du, ddelta, dz)
    within one bf16 rounding (2^-8 relative) of the fp64 value plus 5e-5 of the tensor's scale."""
    from oracle import mamba_ref
    g = load_golden("scan_bf16")
    bf = lambda k: g2t(g[k], torch.bfloat16)
    ins = {k: bf(k) for k in ("u", "delta", "B", "C", "z")}
    A, D, bias = g2t(g["A"]), g2t(g["D"]), g2t(g["delta_bias"])
    dout = det_input(tuple(ins["u"].shape), 991).to(DEV).to(torch.bfloat16)
    _, x, _ = K().selective_scan_fwd(ins["u"], ins["delta"], A, ins["B"], ins["C"], D, ins["z"], bias, True,
                                     reverse=reverse, return_out=False)
    du, ddelta, dA, dB, dC, dD, dbias, dz, _ = K().selective_scan_bwd(
        ins["u"], ins["delta"], A, ins["B"], ins["C"], D, ins["z"], bias, dout, x, None, None, True, False,
        reverse=reverse)
    assert du.dtype == ddelta.dtype == dz.dtype == torch.bfloat16
    fl = (lambda t: t.flip(-1)) if reverse else (lambda t: t)
    r = {k: fl(v.double().cpu()).requires_grad_(True) for k, v in ins.items()}
    rA, rD, rb = (t.double().cpu().requires_grad_(True) for t in (A, D, bias))
    out_z = mamba_ref.selective_scan(r["u"], r["delta"], rA, r["B"], r["C"], rD, r["z"], rb, True,
                                     acc_dtype=torch.float64)
    out_z.backward(fl(dout.double().cpu()))
    for name, v, ref, tol in (("du", du, fl(r["u"].grad), 2 ** -8), ("ddelta", ddelta, fl(r["delta"].grad), 2 ** -8),
                              ("dz", dz, fl(r["z"].grad), 2 ** -8), ("dA", dA, rA.grad, 1e-4),
                              ("dB", dB.reshape(r["B"].shape), fl(r["B"].grad), 1e-4),
                              ("dC", dC.reshape(r["C"].shape), fl(r["C"].grad), 1e-4),
                              ("dD", dD, rD.grad, 1e-4), ("ddelta_bias", dbias, rb.grad, 1e-4)):
        ref = ref.detach().numpy()
        scale = max(1.0, float(np.abs(ref).max()))
        close(v.float(), ref, 5e-5 * scale, tol, name)


# ------------------------------------------------------------------ dt_proj + softplus (csrc/dtproj.hip)

def _softplus64(v):
    return torch.where(v > 20, v, torch.log1p(torch.exp(v)))


@pytest.mark.parametrize("b,D,R,l,dtype", [(2, 1024, 32, 3999, torch.float32), (2, 1024, 32, 5999, torch.bfloat16),
                                           (3, 100, 7, 301, torch.float32), (1, 64, 1, 5, torch.float32),
                                           (2, 130, 64, 257, torch.bfloat16), (4, 512, 16, 36, torch.float32)])
def test_dtproj_vs_fp64(b, D, R, l, dtype):
    """delta = softplus(W x + bias) (selective_scan_interface.py:187 + the scan's softplus, :110-112) from the fused
    kernel vs fp64 on the same (dtype-rounded) operands.  x is a row slice of a wider padded-stride tensor, as the model
    passes x_proj's output; fp32 within 1e-5 of the output's scale; bf16 within one bf16 rounding (2^-8) + 1e-5."""
    seed = b + D + R + l
    xfull = K().bdl_empty(b, R + 32, l, dtype, torch.device(DEV))
    xfull.copy_(det_input((b, R + 32, l), seed).to(DEV, dtype))
    x = xfull[:, :R]
    w = ((R ** -0.5) * det_input((D, R), seed + 1)).to(DEV, dtype)
    bias = (-4.0 + det_input((D,), seed + 2)).to(DEV)
    y = K().dtproj(w, x, bias)
    assert y.dtype == dtype and y.shape == (b, D, l) and y.stride(2) == 1
    ref = _softplus64(torch.einsum("dr,brl->bdl", w.double().cpu(), x.double().cpu()) + bias.double().cpu()[None, :, None])
    tol = 1e-5 if dtype == torch.float32 else 2 ** -8
    close(y.float(), ref, 1e-5 * float(ref.abs().max()), tol, "delta")
    y0 = K().dtproj(w, x, None, softplus=False)
    ref0 = torch.einsum("dr,brl->bdl", w.double().cpu(), x.double().cpu())
    close(y0.float(), ref0, 1e-5 * float(ref0.abs().max()), tol, "affine, no bias")


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("b,d,l", [(2, 128, 300), (1, 64, 65)])
def test_scan_mode2_bitwise_equals_mode1_fp32(b, d, l, reverse):
    """delta_softplus = 2 (delta already softplus(W x + bias), the model's path) against the reference's call (mode 1:
    raw W x + delta_bias, softplus inside the scan): both stage the same fp32 step sizes (the same softplus of the same
    sum), so out_z, the checkpoints and every gradient (ddelta and ddelta_bias w.r.t. the raw value and the bias) are
    bit-identical."""
    seed = 7 * b + d + l
    xr = det_input((b, 8, l), seed).to(DEV)
    w = (0.3 * det_input((d, 8), seed + 1)).to(DEV)
    bias = (-3.0 + det_input((d,), seed + 2)).to(DEV)
    raw = K().dtproj(w, xr, None, softplus=False)
    dt = K().dtproj(w, xr, bias)
    u, z, dout = (det_input((b, d, l), seed + i).to(DEV) for i in (3, 4, 5))
    A = -torch.exp(0.5 * det_input((d, 16), seed + 6)).to(DEV)
    Bm, Cm = (det_input((b, 16, l), seed + i).to(DEV) for i in (7, 8))
    D = det_input((d,), seed + 9).to(DEV)
    _, x1, o1 = K().selective_scan_fwd(u, raw, A, Bm, Cm, D, z, bias, True, reverse=reverse, return_out=False)
    _, x2, o2 = K().selective_scan_fwd(u, dt, A, Bm, Cm, D, z, None, 2, reverse=reverse, return_out=False)
    assert torch.equal(o1, o2) and torch.equal(x1, x2)
    g1 = K().selective_scan_bwd(u, raw, A, Bm, Cm, D, z, bias, dout, x1, None, None, True, False, reverse=reverse)
    g2 = K().selective_scan_bwd(u, dt, A, Bm, Cm, D, z, None, dout, x2, None, None, 2, False, reverse=reverse)
    for name, a_, b_ in zip(("du", "ddelta", "dA", "dB", "dC", "dD", "ddelta_bias", "dz"), g1[:8], g2[:8]):
        assert torch.equal(a_, b_), name
    with pytest.raises(RuntimeError):
        K().selective_scan_fwd(u, dt, A, Bm, Cm, D, z, bias, 2)            # mode 2 takes no bias


def test_scan_mode2_bf16_vs_oracle():
    """C5 dtype, the model's path: dt = softplus(W x + bias) rounded once to bf16 by the fused kernel (its own bar:
    test_dtproj_vs_fp64), scanned in mode 2.  The oracle (fp64) runs on the same bf16 step sizes with no softplus; the
    kernel's ddelta / ddelta_bias are w.r.t. the pre-softplus value and the bias, i.e. the oracle's d(dt) times the
    softplus derivative 1 - exp(-dt) (summed over (b, l) for the bias).  Bars as test_scan_bwd_bf16_vs_oracle: bf16
    outputs within one bf16 rounding (2^-8) + 5e-5 of the tensor's scale, fp32 outputs within 1e-4."""
    b, d, l = 2, 128, 400
    xr = det_input((b, 8, l), 5150).to(DEV, torch.bfloat16)
    w = (0.3 * det_input((d, 8), 5151)).to(DEV, torch.bfloat16)
    bias = (-3.0 + det_input((d,), 5152)).to(DEV)
    dt = K().dtproj(w, xr, bias)
    u, z, dout = (det_input((b, d, l), 5153 + i).to(DEV, torch.bfloat16) for i in range(3))
    A = -torch.exp(0.5 * det_input((d, 16), 5156)).to(DEV)
    Bm, Cm = (det_input((b, 16, l), 5157 + i).to(DEV, torch.bfloat16) for i in range(2))
    D = det_input((d,), 5159).to(DEV)
    _, x, out_z = K().selective_scan_fwd(u, dt, A, Bm, Cm, D, z, None, 2, return_out=False)
    du, ddelta, dA, dB, dC, dD, dbias, dz, _ = K().selective_scan_bwd(u, dt, A, Bm, Cm, D, z, None, dout, x, None, None,
                                                                      2, False)
    leaves = {k: v.double().cpu().requires_grad_(True) for k, v in (("u", u), ("dt", dt), ("B", Bm), ("C", Cm),
                                                                   ("z", z))}
    rA, rD = A.double().cpu().requires_grad_(True), D.double().cpu().requires_grad_(True)
    ref = mamba_ref.selective_scan(leaves["u"], leaves["dt"], rA, leaves["B"], leaves["C"], rD, leaves["z"], None,
                                   False, acc_dtype=torch.float64)
    ref.backward(dout.double().cpu())
    sig = 1.0 - torch.exp(-leaves["dt"].detach())
    draw = leaves["dt"].grad * sig
    for name, v, r_, tol in (("out_z", out_z, ref.detach(), 2 ** -8), ("du", du, leaves["u"].grad, 2 ** -8),
                             ("ddelta", ddelta, draw, 2 ** -8), ("dz", dz, leaves["z"].grad, 2 ** -8),
                             ("dA", dA, rA.grad, 1e-4), ("dB", dB.reshape(b, 16, l), leaves["B"].grad, 1e-4),
                             ("dC", dC.reshape(b, 16, l), leaves["C"].grad, 1e-4), ("dD", dD, rD.grad, 1e-4),
                             ("ddelta_bias", dbias, draw.sum((0, 2)), 1e-4)):
        r_ = r_.detach()
        close(v.float(), r_, 5e-5 * max(1.0, float(r_.abs().max())), tol, name)


# ------------------------------------------------------------------ selective scan: edge shapes vs oracle

@pytest.mark.parametrize("b,d,l", [(1, 64, 1), (2, 64, 63), (1, 96, 65), (3, 130, 129), (1, 64, 200)])
@pytest.mark.parametrize("flags", ["full", "noz", "bare"])
def test_scan_edges_vs_oracle(b, d, l, flags):
    seed = b * 1000 + d * 10 + l
    u = det_input((b, d, l), seed)
    delta = 0.5 * det_input((b, d, l), seed + 1)
    A = -torch.exp(0.5 * det_input((d, 16), seed + 2))
    Bm = det_input((b, 1, 16, l), seed + 3)
    Cm = det_input((b, 1, 16, l), seed + 4)
    D = det_input((d,), seed + 5) if flags != "bare" else None
    z = det_input((b, d, l), seed + 6) if flags == "full" else None
    bias = 0.3 * det_input((d,), seed + 7) if flags != "bare" else None
    sp = flags != "bare"
    if not sp:
        delta = delta.abs()
    ref_leaves = {"u": u, "delta": delta, "A": A, "B": Bm, "C": Cm, "D": D, "z": z, "delta_bias": bias}
    leaves = {k: (v.clone().double().requires_grad_(True) if v is not None else None) for k, v in ref_leaves.items()}
    ref = mamba_ref.selective_scan(**leaves, delta_softplus=sp, acc_dtype=torch.float64)
    dout = det_input((b, d, l), seed + 8).double()
    ref.backward(dout)
    gpu = {k: (v.to(DEV) if v is not None else None) for k, v in ref_leaves.items()}
    out, x, out_z = K().selective_scan_fwd(**gpu, delta_softplus=sp)
    got = out_z if z is not None else out
    close(got, ref, 1e-4, 1e-4, "fwd")
    res = K().selective_scan_bwd(gpu["u"], gpu["delta"], gpu["A"], gpu["B"], gpu["C"], gpu["D"], gpu["z"],
                                 gpu["delta_bias"], dout.float().to(DEV), x, out, None, sp, False)
    names = ["u", "delta", "A", "B", "C", "D", "delta_bias", "z"]
    outs = dict(zip(names, [res[0], res[1], res[2], res[3], res[4], res[5], res[6], res[7]]))
    for k in names:
        if leaves[k] is None:
            continue
        refg = leaves[k].grad
        scale = max(1.0, float(refg.abs().max()))
        close(outs[k], refg, 1e-4 * scale, 1e-4, f"d{k}")


def test_scan_strided_views_and_inplace_dz():
    # u/z as chunk views of one xz buffer (MambaInnerFnNoOutProj layout), dz written into a view
    b, d, l = 2, 64, 150
    xz = det_input((b, 2 * d, l), 77).to(DEV)
    u, z = xz.chunk(2, dim=1)
    delta = (0.5 * det_input((b, d, l), 78)).to(DEV)
    A = (-torch.exp(0.5 * det_input((d, 16), 79))).to(DEV)
    Bm, Cm = det_input((b, 16, l), 80).to(DEV), det_input((b, 16, l), 81).to(DEV)
    D = torch.ones(d, device=DEV)
    out, x, out_z = K().selective_scan_fwd(u, delta, A, Bm, Cm, D, z, None, True)
    ref = mamba_ref.selective_scan(u.cpu(), delta.cpu(), A.cpu(), Bm.cpu(), Cm.cpu(), D.cpu(), z.cpu(), None, True)
    close(out_z, ref, 1e-5, 1e-5)
    dxz = torch.zeros_like(xz)
    dx, dz = dxz.chunk(2, dim=1)
    res = K().selective_scan_bwd(u, delta, A, Bm, Cm, D, z, None, torch.ones_like(u), x, out, dz, True, False)
    assert res[7].data_ptr() == dz.data_ptr()
    assert float(dz.abs().sum()) > 0 and float(dx.abs().sum()) == 0.0


@pytest.mark.slow
def test_scan_full_size_properties():
    """BASELINE C3 (Mamba-TasNet-L) shape class: d_inner 1024, L 3999 — fwd vs fp64 oracle on 2 rows."""
    b, d, l = 2, 1024, 3999
    u = det_input((b, d, l), 90).to(DEV)
    delta = (0.2 * det_input((b, d, l), 91)).to(DEV)
    A = (-torch.exp(0.5 * det_input((d, 16), 92))).to(DEV)
    Bm, Cm = det_input((b, 1, 16, l), 93).to(DEV), det_input((b, 1, 16, l), 94).to(DEV)
    D = det_input((d,), 95).to(DEV)
    z = det_input((b, d, l), 96).to(DEV)
    bias = (0.3 * det_input((d,), 97)).to(DEV)
    out, x, out_z = K().selective_scan_fwd(u, delta, A, Bm, Cm, D, z, bias, True)
    sl = slice(0, 64)   # oracle on a 64-channel slice (B/C are shared across d)
    ref, last = mamba_ref.selective_scan(u[:, sl].cpu(), delta[:, sl].cpu(), A[sl].cpu(), Bm.cpu(), Cm.cpu(),
                                         D[sl].cpu(), z[:, sl].cpu(), bias[sl].cpu(), True, return_last_state=True)
    close(out_z[:, sl], ref, 2e-4, 1e-4)
    close(x[:, sl, -1, 1::2], last, 2e-4, 1e-4)
    # determinism: bitwise identical on rerun (no atomics anywhere)
    out_b, _, out_z_b = K().selective_scan_fwd(u, delta, A, Bm, Cm, D, z, bias, True)
    assert torch.equal(out_z, out_z_b)
    dres = K().selective_scan_bwd(u, delta, A, Bm, Cm, D, z, bias, torch.ones_like(u), x, out, None, True, False)
    dres2 = K().selective_scan_bwd(u, delta, A, Bm, Cm, D, z, bias, torch.ones_like(u), x, out, None, True, False)
    for a_, b_ in zip(dres, dres2):
        if a_ is not None:
            assert torch.equal(a_, b_)
            assert torch.isfinite(a_).all()


# ------------------------------------------------------------------ causal conv1d

@pytest.mark.parametrize("w", [2, 3, 4])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("b,d,l", [(2, 64, 1), (3, 70, 34), (2, 33, 250), (1, 5, 256), (1, 5, 257), (2, 40, 300), (1, 8, 4100)])
def test_cconv_vs_oracle(b, d, l, w, silu):
    x = det_input((b, d, l), 300 + l).double().requires_grad_(True)
    wt = det_input((d, w), 301).double().requires_grad_(True)
    bias = det_input((d,), 302).double().requires_grad_(True)
    ref = mamba_ref.causal_conv1d(x, wt, bias, silu)
    gy = det_input((b, d, l), 303).double()
    ref.backward(gy)
    out = K().causal_conv1d_fwd(x.detach().float().to(DEV), wt.detach().float().to(DEV),
                                bias.detach().float().to(DEV), silu)
    close(out, ref, 1e-5, 1e-5, "fwd")
    dx, dw, db = K().causal_conv1d_bwd(x.detach().float().to(DEV), wt.detach().float().to(DEV),
                                       bias.detach().float().to(DEV), gy.float().to(DEV), silu=silu)
    close(dx, x.grad, 1e-5, 1e-5, "dx")
    close(dw, wt.grad, 1e-3, 1e-5, "dweight")
    close(db, bias.grad, 1e-3, 1e-5, "dbias")


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("b,d,l", [(2, 33, 250), (2, 40, 3000)])
def test_cconv_bf16_vs_oracle(b, d, l, reverse):
    """bf16 activations (C5): fp64 oracle on the same bf16 values; out / dx within one bf16 rounding (2^-8 relative)
    plus 1e-5, dweight / dbias (fp32 outputs) as tight as the fp32 test."""
    bf = lambda t: t.to(torch.bfloat16).double()
    fl = (lambda t: t.flip(-1)) if reverse else (lambda t: t)
    x0, gy0 = bf(det_input((b, d, l), 310 + l)), bf(det_input((b, d, l), 311))
    x = fl(x0).requires_grad_(True)
    wt = det_input((d, 4), 312).double().requires_grad_(True)
    bias = det_input((d,), 313).double().requires_grad_(True)
    ref = mamba_ref.causal_conv1d(x, wt, bias, True)
    ref.backward(fl(gy0))
    xg = x0.to(DEV, torch.bfloat16)
    out = K().causal_conv1d_fwd(xg, wt.detach().float().to(DEV), bias.detach().float().to(DEV), True, reverse=reverse)
    assert out.dtype == torch.bfloat16
    close(out.float(), fl(ref.detach()), 1e-5, 2 ** -8, "fwd")
    dx, dw, db = K().causal_conv1d_bwd(xg, wt.detach().float().to(DEV), bias.detach().float().to(DEV),
                                       gy0.to(DEV, torch.bfloat16), silu=True, reverse=reverse)
    assert dx.dtype == torch.bfloat16 and dw.dtype == torch.float32
    close(dx.float(), fl(x.grad), 1e-5, 2 ** -8, "dx")
    close(dw, wt.grad, 1e-3, 1e-5, "dweight")
    close(db, bias.grad, 1e-3, 1e-5, "dbias")


# ------------------------------------------------------------------ add + RMSNorm

@pytest.mark.parametrize("n", [32, 128, 512, 1024])
@pytest.mark.parametrize("with_res", [False, True])
def test_add_rmsnorm_vs_oracle(n, with_res):
    rows = 333
    h = det_input((rows, n), 400 + n).double().requires_grad_(True)
    r = det_input((rows, n), 401).double().requires_grad_(True) if with_res else None
    w = (1.0 + 0.1 * det_input((n,), 402)).double().requires_grad_(True)
    res = h + r if with_res else h
    y = mamba_ref.rms_norm(res, w, 1e-5)
    gy, gr = det_input((rows, n), 403).double(), det_input((rows, n), 404).double()
    (y * gy).sum().backward(retain_graph=True)
    (res * gr).sum().backward()
    yk, rk, rstd = K().add_rmsnorm_fwd(h.detach().float().to(DEV), r.detach().float().to(DEV) if with_res else None,
                                        w.detach().float().to(DEV), 1e-5)
    close(yk, y, 1e-5, 1e-5, "y")
    close(rk, res, 1e-6, 0, "res")
    dx, dw = K().rmsnorm_bwd(gy.float().to(DEV), gr.float().to(DEV), rk, w.detach().float().to(DEV), rstd)
    close(dx, h.grad, 1e-5, 1e-5, "dx")
    close(dw, w.grad, 1e-3, 1e-5, "dw")
    # the producer-side max the split-fp16 projections take instead of an absmax pass: exactly max |y| / |dx|, and the
    # planes split from it equal split_planes' own (split16_planes_known vs split16_planes)
    for t in (yk, dx):
        mb = getattr(t, K().ABSMAX_ATTR)
        assert int(mb.item()) == int(t.abs().max().view(torch.int32).item())
        v = t.view(1, *t.shape)
        setattr(v, K().ABSMAX_ATTR, mb)
        sk = K().split_planes(v)
        sf = K().split_planes(v.clone())
        assert torch.equal(sk.hi, sf.hi) and torch.equal(sk.lo, sf.lo) and torch.equal(sk.mb, sf.mb)


@pytest.mark.parametrize("n", [512, 256])
def test_add_rmsnorm_bf16_rows_equal_fp32_path(n):
    """bf16 rows (the C5 Block under autocast, avse_add_rmsnorm_fwd2 / avse_rmsnorm_bwd2): h read as bf16 and y written
    in bf16 give bit for bit the fp32 path's results on h.float() with y rounded once; a bf16 dy gives the fp32 path's
    dx / dweight on dy.float()."""
    rows = 333
    h = det_input((rows, n), 410).to(DEV).to(torch.bfloat16)
    r = det_input((rows, n), 411).to(DEV)
    w = (1.0 + 0.1 * det_input((n,), 412)).to(DEV)
    y32, r32, s32 = K().add_rmsnorm_fwd(h.float(), r, w, 1e-5)
    y16, r16, s16 = K().add_rmsnorm_fwd(h, r, w, 1e-5, out_dtype=torch.bfloat16)
    assert y16.dtype == torch.bfloat16 and r16.dtype == torch.float32
    assert torch.equal(y16, y32.to(torch.bfloat16)) and torch.equal(r16, r32) and torch.equal(s16, s32)
    gy = det_input((rows, n), 413).to(DEV).to(torch.bfloat16)
    gr = det_input((rows, n), 414).to(DEV)
    d32, w32 = K().rmsnorm_bwd(gy.float(), gr, r32, w, s32)
    d16, w16 = K().rmsnorm_bwd(gy, gr, r32, w, s32)
    assert torch.equal(d16, d32) and torch.equal(w16, w32)


# ------------------------------------------------------------------ STFT / iSTFT (librosa 0.8.1 semantics)

@pytest.mark.parametrize("T", [48000, 16000, 1000])
def test_stft_vs_oracle(T):
    y = (0.1 * det_input((3, T), 500 + T)).numpy()
    mag, spec = K().stft(torch.from_numpy(y).to(DEV), return_complex=True)
    ref = stft_ref.stft(y)                                   # (3, 257, frames) complex64
    assert mag.shape == (3, 1 + T // 128, 257)
    scale = float(np.abs(ref).max())
    close(mag, np.abs(ref).transpose(0, 2, 1), 2e-6 * scale, 0, "|X|")
    close(torch.view_as_real(spec), np.stack([ref.real, ref.imag], -1).transpose(0, 2, 1, 3), 2e-6 * scale, 0, "X")


def test_istft_vs_oracle_and_roundtrip():
    T = 48000
    y = (0.1 * det_input((2, T), 510)).numpy()
    mag, spec = K().stft(torch.from_numpy(y).to(DEV), return_complex=True)
    # enhancement-style input: a different magnitude with the noisy phase (test.py:85-88)
    m2 = mag * (0.5 + torch.rand_like(mag))
    out = K().istft(m2, spec, T)
    S = spec.cpu().numpy().transpose(0, 2, 1)
    ref = stft_ref.istft(m2.cpu().numpy().transpose(0, 2, 1) * np.exp(1j * np.angle(S)), length=T)
    err = np.sqrt(np.mean((out.cpu().numpy() - ref) ** 2))
    assert err <= 1e-6, err
    rt = K().istft(mag, spec, T)
    assert float(torch.sqrt(torch.mean((rt.cpu() - torch.from_numpy(y)) ** 2))) <= 1e-6


def test_kernels_reject_cpu_tensors():
    with pytest.raises(RuntimeError):
        K().stft(torch.zeros(1, 1000))


# ------------------------------------------------------------------ lip front-end Conv3d weight gradient

@pytest.mark.parametrize("cin,T,H,W", [(3, 6, 20, 18), (1, 5, 16, 16), (3, 3, 96, 96), (1, 3, 112, 112), (2, 2, 130, 40)])
def test_conv3d_wgrad_vs_fp64(cin, T, H, W):
    x = det_input((2, cin, T, H, W), 700 + cin, "uniform", 255.0)
    w = det_input((64, cin, 5, 7, 7), 701) / 50
    y = torch.nn.functional.conv3d(x.double(), w.double(), None, (1, 2, 2), (2, 3, 3))
    dy = det_input(tuple(y.shape), 702)
    ref = torch.nn.grad.conv3d_weight(x.double(), w.shape, dy.double(), (1, 2, 2), (2, 3, 3))
    got = K().conv3d_wgrad(x.to(DEV), dy.to(DEV), (5, 7, 7), (2, 3, 3))
    scale = float(ref.abs().max())
    close(got, ref, 2e-6 * scale * (1 + x.numel() / 1e5) ** 0.5, 0, "dW")
    got2 = K().conv3d_wgrad(x.to(DEV), dy.to(DEV), (5, 7, 7), (2, 3, 3), out=got.clone(), accumulate=True)
    close(got2, 2 * ref, 4e-6 * scale * (1 + x.numel() / 1e5) ** 0.5, 0, "dW accumulate")
    # the split kernel (x and dy split into hi + lo fp16 under their maxima, round 6) against each element's sum of
    # |terms|, as the uint8 test bounds it; and the exact-fp32 kernel (C3W_F16 = False) to the same bar as before
    bound = torch.nn.grad.conv3d_weight(x.double().abs(), w.shape, dy.double().abs(), (1, 2, 2), (2, 3, 3))
    worst = float(((got.double().cpu() - ref).abs() / (bound + 1e-30)).max())
    print(f"conv3d wgrad fp32 split {cin}x{H}x{W}: {worst:.2e} of sum|terms|")
    assert worst <= 1e-5, worst
    xm = x.abs().amax().reshape(1).view(torch.int32).to(DEV)
    assert torch.equal(got, K().conv3d_wgrad(x.to(DEV), dy.to(DEV), (5, 7, 7), (2, 3, 3), xmax=xm))
    old = K().C3W_F16
    try:
        K().C3W_F16 = False
        ex = K().conv3d_wgrad(x.to(DEV), dy.to(DEV), (5, 7, 7), (2, 3, 3))
    finally:
        K().C3W_F16 = old
    close(ex, ref, 2e-6 * scale * (1 + x.numel() / 1e5) ** 0.5, 0, "dW exact fp32")


@pytest.mark.parametrize("T", [5, 1])
def test_conv3d_wgrad_uint8_vs_fp64(T):
    """avse_conv3d_wgrad_u8(_split) reads the uint8 lip frames themselves (no fp32 copy of the clip) at the avse1
    96 x 96 shape: the f16 MFMA path (frames exact in fp16, dy split into hi + lo under its max, given by the producing
    BatchNorm backward or computed here) vs fp64, every element within 1e-5 of its sum of |terms| (the fp32 class);
    kernels.C3W_F16 = False's exact-fp32 kernel is bitwise the fp32-frames kernel (same products, same order); deterministic."""
    import importlib
    g = torch.Generator().manual_seed(704 + T)
    xu = torch.randint(0, 256, (2, 3, T, 96, 96), generator=g, dtype=torch.uint8)
    y = torch.nn.functional.conv3d(xu.double(), det_input((64, 3, 5, 7, 7), 705).double(), None, (1, 2, 2), (2, 3, 3))
    dy = det_input(tuple(y.shape), 706) * torch.exp(2.0 * det_input(tuple(y.shape), 707))
    truth = torch.nn.grad.conv3d_weight(xu.double(), (64, 3, 5, 7, 7), dy.double(), (1, 2, 2), (2, 3, 3))
    bound = torch.nn.grad.conv3d_weight(xu.double(), (64, 3, 5, 7, 7), dy.double().abs(), (1, 2, 2), (2, 3, 3))
    a = K().conv3d_wgrad(xu.to(DEV), dy.to(DEV), (5, 7, 7), (2, 3, 3))
    worst = float(((a.double().cpu() - truth).abs() / (bound + 1e-30)).max())
    print(f"conv3d wgrad u8 split vs fp64: {worst:.2e} of sum|terms|")
    assert worst <= 1e-5, worst
    assert torch.equal(a, K().conv3d_wgrad(xu.to(DEV), dy.to(DEV), (5, 7, 7), (2, 3, 3)))
    dyg = dy.to(DEV)
    setattr(dyg, K().ABSMAX_ATTR, dyg.abs().amax().reshape(1).view(torch.int32))   # a producer's max: same result
    assert torch.equal(a, K().conv3d_wgrad(xu.to(DEV), dyg, (5, 7, 7), (2, 3, 3)))
    old = K().C3W_F16
    try:
        K().C3W_F16 = False
        b = K().conv3d_wgrad(xu.to(DEV), dy.to(DEV), (5, 7, 7), (2, 3, 3))
        c = K().conv3d_wgrad(xu.to(DEV).float(), dy.to(DEV), (5, 7, 7), (2, 3, 3))
    finally:
        K().C3W_F16 = old
    assert torch.equal(b, c)


@pytest.mark.parametrize("dtype,T,cin,hw", [(torch.uint8, 7, 3, 96), (torch.float32, 6, 3, 96), (torch.uint8, 1, 3, 96),
                                             (torch.float32, 5, 1, 112), (torch.float32, 1, 1, 112)])
def test_conv3d_fwd_vs_fp64(dtype, T, cin, hw):
    """K.conv3d_fwd (csrc/conv3d_fwd.hip) vs the fp64 Conv3d(cin, 64, (5,7,7), (1,2,2), (2,3,3)) of the avse1 lip
    front-end (baseline/avse1/model.py:29-34, 3 x 96 x 96) and the avse4 one (baseline/avse4/utils.py:97-118, 1 x 112
    x 112 normalised frames): every output within 1e-6 of its sum of |terms| (the f16 MFMA against the weights split
    into hi + lo fp16, 22 bits; uint8 frames read as stored, exact in fp16; fp32 frames split as well under their
    max, round 6), fp32 accumulation; clips of 1 .. 7 frames cover the zero time padding on both sides."""
    g = torch.Generator().manual_seed(707 + T + cin)
    if dtype == torch.uint8:
        x = torch.randint(0, 256, (2, cin, T, hw, hw), generator=g, dtype=torch.uint8)
    elif cin == 3:
        x = det_input((2, cin, T, hw, hw), 708, "uniform", 255.0)
    else:      # avse4: (x / 255 - 0.421) / 0.165 grey values, with a few frames of much smaller contrast
        x = (det_input((2, cin, T, hw, hw), 708, "uniform", 1.0) - 0.421) / 0.165
        x[:, :, :1] *= 1e-3
    w = det_input((64, cin, 5, 7, 7), 709) / 50
    truth = torch.nn.functional.conv3d(x.double(), w.double(), None, (1, 2, 2), (2, 3, 3))
    bound = torch.nn.functional.conv3d(x.double().abs(), w.double().abs(), None, (1, 2, 2), (2, 3, 3))
    assert K().conv3d_fwd_supported(x, w, (1, 2, 2), (2, 3, 3))
    got = K().conv3d_fwd(x.to(DEV), w.to(DEV))
    assert got.shape == truth.shape and got.dtype == torch.float32
    worst = float(((got.double().cpu() - truth).abs() / (bound + 1e-30)).max())
    print(f"conv3d fwd {dtype} {cin}x{hw}: {worst:.2e} of sum|terms|")
    assert worst <= 1e-6, worst
    assert torch.equal(got, K().conv3d_fwd(x.to(DEV), w.to(DEV)))          # deterministic
    if dtype == torch.float32:
        y2, xmax = K().conv3d_fwd(x.to(DEV), w.to(DEV), return_xmax=True)
        assert torch.equal(y2, got)
        assert int(xmax.cpu()[0]) == int(x.abs().amax().reshape(1).view(torch.int32)[0])


def test_conv3d_fwd_unsupported_shapes():
    x = torch.zeros(1, 1, 5, 88, 88, dtype=torch.uint8)
    assert not K().conv3d_fwd_supported(x, torch.zeros(64, 1, 5, 7, 7), (1, 2, 2), (2, 3, 3))
    assert not K().conv3d_fwd_supported(torch.zeros(1, 3, 5, 96, 96, dtype=torch.float64), torch.zeros(64, 3, 5, 7, 7),
                                        (1, 2, 2), (2, 3, 3))
    with pytest.raises(RuntimeError):
        K().conv3d_fwd(x.to(DEV), torch.zeros(64, 1, 5, 7, 7, device=DEV))


def test_lip_conv3d_module_uint8_frames():
    """LipConv3d on the uint8 frames (the HIP forward and weight gradient on the f16 MFMA, frames read as stored) and
    on their float values (the same kernels with the frames split into hi + lo fp16 as well, round 6) both hold the
    fp32 class against fp64: output within 1e-6 and
    weight gradient within 1e-5 of each element's sum of |terms| (round 5: the two paths no longer share products, so
    they agree to that bar, not bitwise)."""
    from avse_challenge_amd.layers import LipConv3d
    m = LipConv3d(3, 64, (5, 7, 7)).to(DEV)
    g = torch.Generator().manual_seed(711)
    xu = torch.randint(0, 256, (2, 3, 4, 96, 96), generator=g, dtype=torch.uint8).to(DEV)
    y = m(xu)
    gy = torch.randn_like(y)
    y.backward(gy)
    w1 = m.weight.grad.clone()
    m.weight.grad = None
    y2 = m(xu.float())
    y2.backward(gy)
    x64, w64, g64 = xu.double().cpu(), m.weight.detach().double().cpu(), gy.double().cpu()
    conv = lambda a, b: torch.nn.functional.conv3d(a, b, None, (1, 2, 2), (2, 3, 3))  # noqa: E731
    wgr = lambda a, d: torch.nn.grad.conv3d_weight(a, tuple(w64.shape), d, (1, 2, 2), (2, 3, 3))  # noqa: E731
    yt, yb = conv(x64, w64), conv(x64, w64.abs())
    dwt, dwb = wgr(x64, g64), wgr(x64, g64.abs())
    for out, dw in ((y, w1), (y2, m.weight.grad)):
        assert float(((out.detach().double().cpu() - yt).abs() / (yb + 1e-30)).max()) <= 1e-6
        assert float(((dw.double().cpu() - dwt).abs() / (dwb + 1e-30)).max()) <= 1e-5


def test_lip_conv3d_module_grad():
    from avse_challenge_amd.layers import LipConv3d
    m = LipConv3d(3, 64, (5, 7, 7)).to(DEV)
    x = det_input((2, 3, 4, 24, 24), 710, "uniform", 255.0).to(DEV)
    y = m(x)
    gy = torch.randn_like(y)
    y.backward(gy)
    ref = torch.nn.grad.conv3d_weight(x.double().cpu(), m.weight.shape, gy.double().cpu(), (1, 2, 2), (2, 3, 3))
    close(m.weight.grad, ref, 1e-5 * float(ref.abs().max()), 0)


# ------------------------------------------------------------------ PReLU

@pytest.mark.parametrize("shape,npar", [((4, 64, 10, 12), 64), ((3, 512, 75), 512), ((2, 8, 7), 1), ((5, 16, 33), 16)])
def test_prelu_vs_torch(shape, npar):
    from avse_challenge_amd.layers import PReLU
    x = det_input(shape, 720).double().requires_grad_(True)
    a = (0.1 + torch.rand(npar, generator=torch.Generator().manual_seed(1))).double().requires_grad_(True)
    y = torch.nn.functional.prelu(x, a)
    gy = det_input(shape, 721).double()
    y.backward(gy)
    m = PReLU(npar).to(DEV)
    with torch.no_grad():
        m.weight.copy_(a.detach().float())
    xg = x.detach().float().to(DEV).requires_grad_(True)
    yg = m(xg)
    close(yg, y, 1e-6, 1e-6, "y")
    yg.backward(gy.float().to(DEV))
    close(xg.grad, x.grad, 1e-6, 1e-6, "dx")
    close(m.weight.grad, a.grad, 1e-4, 1e-5, "da")


@pytest.mark.parametrize("shape,npar", [((6, 64, 24, 24), 64), ((10, 512, 3, 3), 512), ((7, 128, 5, 5), 1),
                                        ((3, 256, 6, 6), 256), ((2, 16, 4, 3), 16)])
def test_prelu_channels_last_vs_torch(shape, npar):
    """Channels-last (NHWC) activations take avse_prelu_nhwc_*; output keeps the channels-last strides."""
    from avse_challenge_amd.layers import PReLU
    x = det_input(shape, 730).double().requires_grad_(True)
    a = (0.1 + torch.rand(npar, generator=torch.Generator().manual_seed(2))).double().requires_grad_(True)
    y = torch.nn.functional.prelu(x, a)
    gy = det_input(shape, 731).double()
    y.backward(gy)
    m = PReLU(npar).to(DEV)
    with torch.no_grad():
        m.weight.copy_(a.detach().float())
    xg = x.detach().float().to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    yg = m(xg)
    assert yg.is_contiguous(memory_format=torch.channels_last) and not yg.is_contiguous()
    close(yg, y, 1e-6, 1e-6, "y")
    yg.backward(gy.float().to(DEV).contiguous(memory_format=torch.channels_last))
    close(xg.grad, x.grad, 1e-6, 1e-6, "dx")
    close(m.weight.grad, a.grad, 1e-4, 1e-5, "da")


# ------------------------------------------------------------------ BatchNorm -> [+ res] -> act (bnact.hip)

BNACT_CASES = [
    ((4, 64, 10, 12), False, "prelu_c", True, True),     # ResNet bn2 + shortcut -> PReLU (NCHW)
    ((6, 64, 3, 3), False, "prelu_c", False, True),      # layer4-like 3x3 maps
    ((2, 16, 5, 7, 7), False, "prelu_c", False, True),   # frontend BatchNorm3d -> PReLU (NCDHW)
    ((4, 64, 10, 12), True, "relu", False, True),        # audio net BatchNorm2d -> ReLU, channels-last
    ((3, 4, 9, 11), True, "relu", True, True),           # 4 channels (one 4-wide column per row), + res
    ((2, 1, 37, 29), False, None, False, True),          # bn0: one channel, no act
    ((3, 3, 5, 7), False, "prelu_1", True, True),        # odd C*S: scalar path, single slope
    ((5, 32, 6, 6), False, "prelu_c", True, False),      # eval mode (running statistics)
    ((4, 8, 50), False, None, False, True),              # BatchNorm1d-shaped
]


@pytest.mark.parametrize("mean,scale", [(30.0, 2.0), (100.0, 0.01)])
@pytest.mark.parametrize("shape,cl,act,res,training", BNACT_CASES)
def test_bnact_vs_fp64(shape, cl, act, res, training, mean, scale):
    """act(BatchNorm(x) [+ res]) through layers.bn_act vs torch fp64 modules: output, every gradient and the
    running-statistic update (momentum 0.1, unbiased variance).  mean / std up to 1e4 (the mean is carried as
    a float pair, so the activation mask does not flip on the rounding of the mean)."""
    from avse_challenge_amd.layers import PReLU, bn_act
    C = shape[1]
    bn_cls = {3: torch.nn.BatchNorm1d, 4: torch.nn.BatchNorm2d, 5: torch.nn.BatchNorm3d}[len(shape)]
    gen = torch.Generator().manual_seed(11)
    # large-mean input (as raw-pixel Conv3d outputs): the shifted statistics must not cancel
    # fp32-representable inputs: the reference sees exactly the values the kernels read
    x = (scale * det_input(shape, 740) + mean).float().double().requires_grad_(True)
    r = det_input(shape, 741).double().requires_grad_(True) if res else None
    gy = det_input(shape, 742).double()
    ref = bn_cls(C).double()
    with torch.no_grad():
        ref.weight.copy_(0.5 + torch.rand(C, generator=gen))
        ref.bias.copy_(0.1 * torch.randn(C, generator=gen))
        ref.running_mean.copy_(mean + scale * torch.randn(C, generator=gen))
        ref.running_var.copy_(scale * scale * (1.0 + torch.rand(C, generator=gen)))
    npar = {"prelu_c": C, "prelu_1": 1}.get(act, 0)
    a = (0.1 + 0.3 * torch.rand(max(npar, 1), generator=gen)).double().requires_grad_(True)
    bn = bn_cls(C).to(DEV)
    bn.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    ref.train(training)
    bn.train(training)
    z = ref(x) + (r if res else 0.0)
    y = torch.relu(z) if act == "relu" else (torch.nn.functional.prelu(z, a) if npar else z)
    y.backward(gy)
    m_act = None
    if npar:
        m_act = PReLU(npar).to(DEV)
        with torch.no_grad():
            m_act.weight.copy_(a.detach().float())
    elif act == "relu":
        m_act = "relu"
    fmt = torch.channels_last if cl else torch.contiguous_format
    xg = x.detach().float().to(DEV).contiguous(memory_format=fmt).requires_grad_(True)
    rg = r.detach().float().to(DEV).contiguous(memory_format=fmt).requires_grad_(True) if res else None
    yg = bn_act(xg, bn, m_act, res=rg)
    assert yg.stride() == xg.stride()
    close(yg, y, 2e-5, 1e-5, "y")
    # the producer-side max the split convolutions take instead of an absmax pass: exactly max |y| as stored
    assert int(getattr(yg, K().ABSMAX_ATTR).item()) == int(yg.detach().abs().max().view(torch.int32).item())
    yg.backward(gy.float().to(DEV).contiguous(memory_format=fmt))
    gs = float(x.grad.abs().max())
    close(xg.grad, x.grad, 2e-5 * gs, 1e-4, "dx")
    mb = getattr(xg.grad, K().ABSMAX_ATTR, None)          # the backward's dx max (when autograd kept the object)
    if mb is not None:
        assert int(mb.item()) == int(xg.grad.abs().max().view(torch.int32).item())
    if res:
        close(rg.grad, r.grad, 1e-6, 1e-6, "dres")
    close(bn.weight.grad, ref.weight.grad, 1e-4 * float(ref.weight.grad.abs().max()), 1e-4, "dgamma")
    close(bn.bias.grad, ref.bias.grad, 1e-4 * float(ref.bias.grad.abs().max()), 1e-4, "dbeta")
    if npar:
        close(m_act.weight.grad, a.grad, 1e-4 * float(a.grad.abs().max()) + 1e-7, 1e-4, "dalpha")
    close(bn.running_mean, ref.running_mean, 1e-5, 1e-6, "running_mean")
    close(bn.running_var, ref.running_var, 1e-5, 1e-5, "running_var")
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked)


def _q_decode(t):
    """A split-output (N, C, H, W) tensor -> fp64 values (hi + lo) 2^-e, e from its bound (split16.h split_exp)."""
    q = K().q_view(t).view(torch.float16).reshape(-1, t.shape[1] // 16, 2, 16).double()
    bits = int(getattr(t, K().ABSMAX_ATTR).item())
    e = max(-100, min(100, 14 - (((bits >> 23) & 0xFF) - 127))) if bits else 0
    v = (q[:, :, 0, :] + q[:, :, 1, :]) * 2.0 ** -e
    n, c, h, w = t.shape
    return v.reshape(n, h, w, c).permute(0, 3, 1, 2)


@pytest.mark.parametrize("act", ["relu", "prelu_c", "none"])
@pytest.mark.parametrize("shape,mean,scale", [((4, 64, 24, 24), 0.0, 1.0), ((2, 128, 9, 11), 30.0, 0.02),
                                              ((3, 64, 7, 257), -2.0, 5.0)])
def test_bnact_split_output_vs_fp32(shape, mean, scale, act):
    """bnact with q_out (csrc/bnact.hip QOUT passes, round 5): the output / input gradient written straight as the fp16
    hi / lo split the split-fp16 convolutions read.  Against the fp32 passes on the same inputs: same statistics
    (bitwise), the bound published for the split scale >= max |y| (|dx|) and within 2^6 of it, and every decoded value
    within 2^-21 of the tensor's max of the fp32 value (the split's 22 bits); split16 / split_q hand the bytes on
    without a pass."""
    C = shape[1]
    g = torch.Generator().manual_seed(C + shape[-1])
    x = (scale * det_input(shape, 750) + mean).float().to(DEV).contiguous(memory_format=torch.channels_last)
    gam = (0.5 + torch.rand(C, generator=g)).to(DEV)
    bet = (0.1 * torch.randn(C, generator=g)).to(DEV)
    code = {"relu": K().ACT_RELU, "prelu_c": K().ACT_PRELU, "none": K().ACT_NONE}[act]
    alpha = (0.1 + 0.3 * torch.rand(C, generator=g)).to(DEV) if act == "prelu_c" else None
    rms = [(torch.zeros(C, device=DEV), torch.ones(C, device=DEV)) for _ in range(2)]
    y, st = K().bnact_fwd(x, gam, bet, *rms[0], True, 0.1, 1e-5, code, alpha)
    yq, stq = K().bnact_fwd(x, gam, bet, *rms[1], True, 0.1, 1e-5, code, alpha, q_out=True)
    assert K().is_split_q(yq) and not K().is_split_q(y)
    assert torch.equal(st, stq) and torch.equal(rms[0][0], rms[1][0]) and torch.equal(rms[0][1], rms[1][1])
    for ref, q in ((y, yq),):
        m = float(ref.abs().max())
        bound = float(getattr(q, K().ABSMAX_ATTR).view(torch.float32).item())
        assert m <= bound <= 64 * m + 1e-30, (m, bound)
        err = float((_q_decode(q).cpu() - ref.double().cpu()).abs().max())
        assert err <= 2.0 ** -21 * m, (err, m)
    mb = torch.empty(2, device=DEV, dtype=torch.int32)
    assert K().split16(yq, mb).data_ptr() == yq.data_ptr() if C == 64 else True
    xq, xm = K().split_q(yq)
    assert xq.data_ptr() == yq.data_ptr() and int(xm.item()) == int(getattr(yq, K().ABSMAX_ATTR).item())
    dy = det_input(shape, 751).float().to(DEV).contiguous(memory_format=torch.channels_last)
    dx, _, dg, db, da = K().bnact_bwd(x, None, dy, st, gam, bet, code, alpha, True)
    dxq, _, dgq, dbq, daq = K().bnact_bwd(x, None, dy, st, gam, bet, code, alpha, True, q_out=True)
    assert K().is_split_q(dxq) and torch.equal(dg, dgq) and torch.equal(db, dbq)
    if alpha is not None:
        assert torch.equal(da, daq)
    m = float(dx.abs().max())
    bound = float(getattr(dxq, K().ABSMAX_ATTR).view(torch.float32).item())
    assert m <= bound <= 64 * m, (m, bound)
    err = float((_q_decode(dxq).cpu() - dx.double().cpu()).abs().max())
    assert err <= 2.0 ** -21 * m, (err, m)


@pytest.mark.parametrize("shape,k,s,p", [((2, 3, 4, 48, 48), 3, 2, 1), ((1, 2, 3, 7, 9), 3, 2, 1),
                                         ((2, 2, 2, 10, 11), 2, 2, 0), ((1, 1, 2, 5, 6), 3, 1, 1),
                                         ((1, 2, 3, 9, 10), 3, 2, 1), ((1, 1, 1, 1, 2), 3, 2, 1),
                                         ((1, 2, 2, 7, 8), 3, 2, 1), ((1, 1, 1, 1, 4), 3, 2, 1)])
def test_maxpool3d_planes_vs_torch(shape, k, s, p):
    """nn.MaxPool3d((1,k,k), (1,s,s), (0,p,p)) through layers.maxpool3d vs torch fp64 (values with exact ties and a
    NaN-free plateau: the first maximum wins, as torch); dx vs torch's backward."""
    from avse_challenge_amd.layers import maxpool3d
    pool = torch.nn.MaxPool3d((1, k, k), (1, s, s), (0, p, p))
    x = torch.round(4 * det_input(shape, 750)).double().requires_grad_(True)      # many ties
    y = pool(x)
    gy = det_input(y.shape, 751).double()
    y.backward(gy)
    xg = x.detach().float().to(DEV).requires_grad_(True)
    yg = maxpool3d(xg, pool)
    close(yg, y, 0, 0, "y")
    yg.backward(gy.float().to(DEV))
    close(xg.grad, x.grad, 1e-6, 1e-6, "dx")


# ------------------------------------------------------------------ flip-by-index (BiMamba v2 backward direction)

@pytest.mark.parametrize("l", [1, 64, 150, 257])
def test_scan_and_cconv_reverse_equal_flipped(l):
    b, d = 2, 64
    u = det_input((b, d, l), 800 + l).to(DEV)
    delta = (0.5 * det_input((b, d, l), 801)).to(DEV)
    A = (-torch.exp(0.5 * det_input((d, 16), 802))).to(DEV)
    Bm, Cm = det_input((b, 1, 16, l), 803).to(DEV), det_input((b, 1, 16, l), 804).to(DEV)
    D = det_input((d,), 805).to(DEV)
    z = det_input((b, d, l), 806).to(DEV)
    bias = (0.3 * det_input((d,), 807)).to(DEV)
    f = lambda t: t.flip(-1)
    out_r, x_r, oz_r = K().selective_scan_fwd(u, delta, A, Bm, Cm, D, z, bias, True, reverse=True)
    out_f, x_f, oz_f = K().selective_scan_fwd(f(u), f(delta), A, f(Bm), f(Cm), D, f(z), bias, True)
    close(oz_r, f(oz_f), 1e-6, 1e-6, "scan fwd reverse")
    close(x_r, x_f, 1e-6, 1e-6, "checkpoints")
    g = det_input((b, d, l), 808).to(DEV)
    gr = K().selective_scan_bwd(u, delta, A, Bm, Cm, D, z, bias, g, x_r, out_r, None, True, False, reverse=True)
    gf = K().selective_scan_bwd(f(u), f(delta), A, f(Bm), f(Cm), D, f(z), bias, f(g), x_f, out_f, None, True, False)
    for i, name in enumerate(["du", "ddelta", "dA", "dB", "dC", "dD", "dbias", "dz"]):
        flipped = gf[i].flip(-1) if name in ("du", "ddelta", "dB", "dC", "dz") else gf[i]
        close(gr[i], flipped, 1e-5, 1e-5, name)
    w, cb = det_input((d, 4), 809).to(DEV), det_input((d,), 810).to(DEV)
    co_r = K().causal_conv1d_fwd(u, w, cb, True, reverse=True)
    close(co_r, f(K().causal_conv1d_fwd(f(u), w, cb, True)), 1e-6, 1e-6, "cconv fwd reverse")
    dr = K().causal_conv1d_bwd(u, w, cb, g, silu=True, reverse=True)
    df = K().causal_conv1d_bwd(f(u), w, cb, f(g), silu=True)
    close(dr[0], f(df[0]), 1e-5, 1e-5, "cconv dx")
    close(dr[1], df[1], 1e-4, 1e-5, "cconv dw")
    close(dr[2], df[2], 1e-4, 1e-5, "cconv db")


def test_encoder_decoder_framing_gemm_vs_golden():
    from avse_challenge_amd import mamba_tasnet as M
    from oracle.det_init import det_init_
    g = load_golden("encdec")
    enc = det_init_(M.Encoder(16, 64), 14).to(DEV)
    dec = det_init_(M.Decoder(64, 1, 16, stride=8, bias=False), 15).to(DEV)
    mix = g2t(g["mix"]).requires_grad_(True)
    w = enc(mix)
    close(w, g["mix_w"], 1e-5, 1e-5, "encoder")
    y = dec(w)
    close(y, g["dec"], 1e-5, 1e-5, "decoder")
    # gradients vs torch's reference conv ops in fp64 on CPU
    y.sum().backward()
    mix64 = torch.from_numpy(g["mix"]).double().requires_grad_(True)
    w64 = torch.relu(torch.nn.functional.conv1d(mix64[:, None], enc.conv1d.weight.detach().cpu().double(), stride=8))
    y64 = torch.nn.functional.conv_transpose1d(w64, dec.weight.detach().cpu().double(), stride=8)
    y64.sum().backward()
    close(mix.grad, mix64.grad, 1e-4, 1e-5, "d mix")


# ------------------------------------------------------------------ avse4 TCN: fused PReLU->gLN, depthwise dilated conv1d

@pytest.mark.parametrize("shape", [(2, 256, 300), (1, 512, 4001), (3, 8, 1), (2, 64, 2049), (6, 512, 4001)])
def test_prelu_gln_vs_fp64(shape):
    """gLN(PReLU(x)) of baseline/avse4/model.py:225-252 (eps 1e-8) vs the fp64 oracle; fwd + all grads (K = 1, odd K:
    the vectorized passes' partial last quadruple)."""
    from avse_challenge_amd.layers import prelu_gln
    from oracle.avse4_ref import GlobalLayerNorm
    C = shape[1]
    x = (1.5 * det_input(shape, 900) + 0.3).double().requires_grad_(True)
    a = torch.tensor([0.25], dtype=torch.float64, requires_grad=True)
    gln = GlobalLayerNorm(C).double()
    with torch.no_grad():
        gln.gamma.copy_(0.5 + torch.rand(1, C, 1, generator=torch.Generator().manual_seed(3)))
        gln.beta.copy_(0.1 * det_input((1, C, 1), 901))
    y = gln(torch.nn.functional.prelu(x, a))
    gy = det_input(shape, 902).double()
    y.backward(gy)
    xg = x.detach().float().to(DEV).requires_grad_(True)
    ag = a.detach().float().to(DEV).requires_grad_(True)
    gg = gln.gamma.detach().float().to(DEV).requires_grad_(True)
    bg = gln.beta.detach().float().to(DEV).requires_grad_(True)
    yg = prelu_gln(xg, ag, gg, bg)
    close(yg, y, 2e-5, 1e-5, "y")
    yg.backward(gy.float().to(DEV))
    n = shape[0] * shape[1] * shape[2]
    close(xg.grad, x.grad, 2e-5 * max(1.0, float(x.grad.abs().max())), 1e-4, "dx")
    close(ag.grad, a.grad, 1e-4 * max(1.0, float(a.grad.abs().max())) + 1e-7 * n, 1e-4, "dalpha")
    close(gg.grad, gln.gamma.grad, 1e-4 * max(1.0, float(gln.gamma.grad.abs().max())), 1e-4, "dgamma")
    close(bg.grad, gln.beta.grad, 1e-4 * max(1.0, float(gln.beta.grad.abs().max())), 1e-4, "dbeta")


@pytest.mark.parametrize("B,C,Kn,P,dil", [(2, 256, 300, 3, 4), (1, 512, 4001, 3, 128), (2, 16, 5, 3, 8),
                                           (3, 512, 75, 3, 1), (1, 7, 2500, 5, 3), (2, 4, 1, 7, 1),
                                           (1, 64, 2048, 3, 1), (2, 32, 4099, 1, 1)])
def test_dwconv_vs_fp64(B, C, Kn, P, dil):
    """Depthwise dilated 'same' conv1d (model.py:278-285, :191-198) vs torch fp64 conv1d; fwd, dx, dw.
    Covers K < halo, K = 1, K a multiple / non-multiple of the LDS tile, P in {1,3,5,7}."""
    from avse_challenge_amd.layers import dwconv1d
    x = det_input((B, C, Kn), 910).double().requires_grad_(True)
    w = det_input((C, 1, P), 911).double().requires_grad_(True)
    y = torch.nn.functional.conv1d(x, w, None, 1, (P - 1) // 2 * dil, dil, C)
    gy = det_input((B, C, Kn), 912).double()
    y.backward(gy)
    xg = x.detach().float().to(DEV).requires_grad_(True)
    wg = w.detach().float().to(DEV).requires_grad_(True)
    yg = dwconv1d(xg, wg, dil)
    close(yg, y, 1e-5, 1e-6, "y")
    yg.backward(gy.float().to(DEV))
    close(xg.grad, x.grad, 1e-5, 1e-6, "dx")
    close(wg.grad, w.grad, 1e-6 * B * Kn + 1e-5, 1e-5, "dw")


def test_scan_fwd_without_out_matches():
    """return_out=False (training fwd, pre-gate out not written) gives the same out_z / checkpoints."""
    g = load_golden("scan_fp32")
    ins = {k: g2t(g[k]) for k in ("u", "delta", "A", "B", "C", "D", "z", "delta_bias")}
    out, x, oz = K().selective_scan_fwd(**ins, delta_softplus=True)
    out2, x2, oz2 = K().selective_scan_fwd(**ins, delta_softplus=True, return_out=False)
    assert out2 is None
    assert torch.equal(oz, oz2) and torch.equal(x, x2)


@pytest.mark.parametrize("dtype,reverse", [(torch.float32, False), (torch.bfloat16, True), (torch.bfloat16, False)])
def test_scan_fwd_out_z_accumulate(dtype, reverse):
    """out_z_acc (round 6, the serial BiMamba v2 direction sum): the flush adds the gated output to the given tensor in
    place -- fp32: bitwise acc + out_z (one fp32 add of the same values); bf16: within one bf16 rounding of
    (acc + out_z in fp32), one rounding fewer than the separate add of the two bf16 tensors.  Chunk tail (l = 200)."""
    b, d, l = 2, 80, 200
    ins = {"u": det_input((b, d, l), 31), "delta": 0.2 * det_input((b, d, l), 32), "A": -torch.exp(0.5 * det_input((d, 16), 33)),
           "B": det_input((b, 1, 16, l), 34), "C": det_input((b, 1, 16, l), 35), "D": det_input((d,), 36),
           "z": det_input((b, d, l), 37), "delta_bias": 0.3 * det_input((d,), 38)}
    ins = {k: (v.to(dtype) if k in ("u", "delta", "B", "C", "z") else v).to(DEV) for k, v in ins.items()}
    _, x0, oz = K().selective_scan_fwd(**ins, delta_softplus=True, reverse=reverse, return_out=False)
    acc = det_input((b, d, l), 39).to(dtype).to(DEV)
    acc0 = acc.clone()
    mx = torch.zeros(1, device=DEV, dtype=torch.int32)
    _, x1, oz1 = K().selective_scan_fwd(**ins, delta_softplus=True, reverse=reverse, return_out=False, out_z_acc=acc,
                                        out_z_max=mx)
    assert oz1.data_ptr() == acc.data_ptr() and torch.equal(x0, x1)
    if dtype == torch.float32:              # the producer-side max: max |acc| over the logical elements, as float bits
        assert int(mx.cpu()[0]) == int(acc.abs().amax().reshape(1).view(torch.int32).cpu()[0])
    want = acc0.float() + oz.float()
    if dtype == torch.float32:
        assert torch.equal(acc, want)
    else:
        # oz is the bf16-rounded gated output; the flush adds the fp32 value: |diff| <= one bf16 ulp of the result + oz's
        err = (acc.float() - want).abs()
        tol = 2.0 ** -7 * (want.abs() + oz.float().abs()) + 1e-30
        assert bool((err <= tol).all()), float((err / tol).max())
    with pytest.raises(RuntimeError):
        K().selective_scan_fwd(**ins, delta_softplus=True, return_out=False, out_z_acc=acc[:, :, :100])


@pytest.mark.parametrize("dtype,l,padded,reverse", [(torch.float32, 300, True, False), (torch.bfloat16, 300, True, True),
                                                    (torch.float32, 200, True, True), (torch.bfloat16, 301, False, False)])
def test_cconv_bwd_dx_accumulate(dtype, l, padded, reverse):
    """dx_accumulate (round 6, the serial BiMamba directions' shared xz gradient): dx += the input gradient, on the
    vectorised rows (padded time stride), the short-row kernel (l <= 256) and the generic one (odd stride):
    fp32 bitwise buf + dx, bf16 within one rounding of (buf + dx) in fp32; dweight / dbias unchanged."""
    b, d, w = 2, 48, 4
    x = det_input((b, d, l), 41).to(dtype).to(DEV)
    g = det_input((b, d, l), 42).to(dtype).to(DEV)
    wt, cb = (0.3 * det_input((d, w), 43)).to(DEV), det_input((d,), 44).to(DEV)
    dx0, dw0, db0 = K().causal_conv1d_bwd(x, wt, cb, g, silu=True, reverse=reverse)
    lp = (l + 31) // 32 * 32 if padded else l
    store = det_input((b, d, lp), 45).to(dtype).to(DEV)
    buf = store[:, :, :l]
    buf0 = buf.clone()
    mx = torch.zeros(1, device=DEV, dtype=torch.int32)
    dx1, dw1, db1 = K().causal_conv1d_bwd(x, wt, cb, g, dx=buf, silu=True, reverse=reverse, dx_accumulate=True,
                                          dx_max=mx)
    assert dx1.data_ptr() == buf.data_ptr()
    if dtype == torch.float32:              # max |dx| over the logical elements as float bits (fp32: the stored values)
        assert int(mx.cpu()[0]) == int(buf.abs().amax().reshape(1).view(torch.int32).cpu()[0])
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)
    want = buf0.float() + dx0.float()
    if dtype == torch.float32:
        assert torch.equal(buf, want)
    else:
        err = (buf.float() - want).abs()
        assert bool((err <= 2.0 ** -7 * (want.abs() + dx0.float().abs()) + 1e-30).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_scan_bwd_dz_accumulate(dtype):
    """dz_accumulate (round 6): the scan backward adds dz into the given view; every other output unchanged."""
    b, d, l = 2, 80, 200
    ins = {"u": det_input((b, d, l), 51), "delta": 0.2 * det_input((b, d, l), 52), "A": -torch.exp(0.5 * det_input((d, 16), 53)),
           "B": det_input((b, 1, 16, l), 54), "C": det_input((b, 1, 16, l), 55), "D": det_input((d,), 56),
           "z": det_input((b, d, l), 57), "delta_bias": 0.3 * det_input((d,), 58)}
    ins = {k: (v.to(dtype) if k in ("u", "delta", "B", "C", "z") else v).to(DEV) for k, v in ins.items()}
    _, x, _ = K().selective_scan_fwd(**ins, delta_softplus=True, return_out=False)
    dout = det_input((b, d, l), 59).to(dtype).to(DEV)
    args = [ins[k] for k in ("u", "delta", "A", "B", "C", "D", "z", "delta_bias")] + [dout, x]
    r0 = K().selective_scan_bwd(*args, None, None, True)
    buf = det_input((b, d, l), 60).to(dtype).to(DEV)
    buf0 = buf.clone()
    mx = torch.zeros(1, device=DEV, dtype=torch.int32)
    r1 = K().selective_scan_bwd(*args, None, buf, True, dz_accumulate=True, dz_max=mx)
    for i in (0, 1, 2, 3, 4, 5, 6):
        assert torch.equal(r0[i], r1[i]), i
    if dtype == torch.float32:
        assert int(mx.cpu()[0]) == int(buf.abs().amax().reshape(1).view(torch.int32).cpu()[0])
    assert r1[7].data_ptr() == buf.data_ptr()
    want = buf0.float() + r0[7].float()
    if dtype == torch.float32:
        assert torch.equal(buf, want)
    else:
        err = (buf.float() - want).abs()
        assert bool((err <= 2.0 ** -7 * (want.abs() + r0[7].float().abs()) + 1e-30).all())
    with pytest.raises(RuntimeError):
        K().selective_scan_bwd(*args, None, None, True, dz_accumulate=True)


# ------------------------------------------------------------------ C5 production shape (bf16, d_inner 1024, L 5999)

def _c5_scan_inputs(b, d, l, seed):
    bf = torch.bfloat16
    ins = {"u": det_input((b, d, l), seed).to(bf), "delta": (0.2 * det_input((b, d, l), seed + 1)).to(bf),
           "B": det_input((b, 1, 16, l), seed + 2).to(bf), "C": det_input((b, 1, 16, l), seed + 3).to(bf),
           "z": det_input((b, d, l), seed + 4).to(bf)}
    A = -torch.exp(0.5 * det_input((d, 16), seed + 5))
    D, bias = det_input((d,), seed + 6), 0.3 * det_input((d,), seed + 7)
    dout = det_input((b, d, l), seed + 8).to(bf)
    return ins, A, D, bias, dout


def test_c5_scan_bf16_production_shape_vs_oracle():
    """C5 shape (b=2, d_inner=1024, L=5999, bf16 u/delta/z/B/C/dout, fp32 A/D/bias/state): the training
    forward (return_out=False, as the model runs it) and the backward on the full width, checked against
    the fp64 oracle (forward recurrence and its explicit adjoint) on the SAME bf16 values for channels 0..63 (du, ddelta, dz, dA, dD,
    ddelta_bias); dB / dC (sums over all 1024 channels) are checked by linearity — the full-width kernel's
    dB / dC equal the sum of the kernel's per-64-channel-slice dB / dC — and slice 0's dB / dC against the
    oracle. Tolerances as test_scan_bwd_bf16_vs_oracle (bf16 outputs: one bf16 rounding 2^-8 relative)."""
    b, d, l, sl = 2, 1024, 5999, slice(0, 64)
    ins, A, D, bias, dout = _c5_scan_inputs(b, d, l, 1200)
    gi = {k: v.to(DEV) for k, v in ins.items()}
    gA, gD, gb, gdo = A.to(DEV), D.to(DEV), bias.to(DEV), dout.to(DEV)
    _, x, out_z = K().selective_scan_fwd(gi["u"], gi["delta"], gA, gi["B"], gi["C"], gD, gi["z"], gb, True,
                                         return_out=False)
    du, ddelta, dA, dB, dC, dD, dbias, dz, _ = K().selective_scan_bwd(
        gi["u"], gi["delta"], gA, gi["B"], gi["C"], gD, gi["z"], gb, gdo, x, None, None, True, False)
    sl_in = {k: (v[:, sl] if k in ("u", "delta", "z") else v).double() for k, v in ins.items()}
    ref = mamba_ref.selective_scan(**sl_in, A=A[sl], D=D[sl], delta_bias=bias[sl], delta_softplus=True,
                                   acc_dtype=torch.float64)
    rel = (out_z[:, sl].double().cpu() - ref).abs() / (ref.abs() + 1e-2)
    assert float(rel.max()) <= 2 * 2 ** -8 + 1e-6, float(rel.max())
    # fp64 truth: the explicit adjoint (pinned against the reference's autograd by test_oracle_golden.py)
    rg = mamba_ref.selective_scan_grads(**sl_in, A=A[sl], D=D[sl], delta_bias=bias[sl], delta_softplus=True,
                                        dout=dout[:, sl])
    for name, v, key, tol in (("du", du[:, sl], "du", 2 ** -8), ("ddelta", ddelta[:, sl], "ddelta", 2 ** -8),
                              ("dz", dz[:, sl], "dz", 2 ** -8), ("dA", dA[sl], "dA", 1e-4),
                              ("dD", dD[sl], "dD", 1e-4), ("ddelta_bias", dbias[sl], "ddelta_bias", 1e-4)):
        ref_g = rg[key].numpy()
        close(v.float(), ref_g, 5e-5 * max(1.0, float(np.abs(ref_g).max())), tol, name)
    # dB / dC: linearity over channel slices, slice 0 vs the oracle
    sdB, sdC = torch.zeros_like(dB), torch.zeros_like(dC)
    for c0 in range(0, d, 64):
        s = slice(c0, c0 + 64)
        _, xs, _ = K().selective_scan_fwd(gi["u"][:, s], gi["delta"][:, s], gA[s], gi["B"], gi["C"], gD[s],
                                          gi["z"][:, s], gb[s], True, return_out=False)
        res = K().selective_scan_bwd(gi["u"][:, s], gi["delta"][:, s], gA[s], gi["B"], gi["C"], gD[s], gi["z"][:, s],
                                     gb[s], gdo[:, s], xs, None, None, True, False)
        if c0 == 0:
            for name, v, key in (("dB slice0", res[3], "dB"), ("dC slice0", res[4], "dC")):
                ref_g = rg[key].numpy()
                close(v, ref_g, 5e-5 * max(1.0, float(np.abs(ref_g).max())), 1e-4, name)
        sdB += res[3]
        sdC += res[4]
    for name, full, summed in (("dB", dB, sdB), ("dC", dC, sdC)):
        close(full, summed, 1e-5 * max(1.0, float(summed.abs().max())), 1e-4, name + " linearity")
    assert all(torch.isfinite(t).all() for t in (du, ddelta, dz, dA, dB, dC, dD, dbias))


def test_c5_cconv_bf16_production_shape_vs_oracle():
    """C5 causal conv at full width: (2, 1024, 5999) bf16 activations, fp32 weights, SiLU; fwd / dx within one
    bf16 rounding of fp64 on the same bf16 values, dweight / dbias (fp32) to 1e-5 relative."""
    b, d, l = 2, 1024, 5999
    x0 = det_input((b, d, l), 1300).to(torch.bfloat16).double()
    gy0 = det_input((b, d, l), 1301).to(torch.bfloat16).double()
    x = x0.clone().requires_grad_(True)
    wt = (0.5 * det_input((d, 4), 1302)).double().requires_grad_(True)
    bias = det_input((d,), 1303).double().requires_grad_(True)
    ref = mamba_ref.causal_conv1d(x, wt, bias, True)
    ref.backward(gy0)
    xg = x0.to(DEV, torch.bfloat16)
    out = K().causal_conv1d_fwd(xg, wt.detach().float().to(DEV), bias.detach().float().to(DEV), True)
    close(out.float(), ref.detach(), 1e-5, 2 ** -8, "fwd")
    dx, dw, db = K().causal_conv1d_bwd(xg, wt.detach().float().to(DEV), bias.detach().float().to(DEV),
                                       gy0.to(DEV, torch.bfloat16), silu=True)
    close(dx.float(), x.grad, 1e-5, 2 ** -8, "dx")
    sw, sb = float(wt.grad.abs().max()), float(bias.grad.abs().max())
    close(dw, wt.grad, 1e-5 * sw, 1e-5, "dweight")
    close(db, bias.grad, 1e-5 * sb, 1e-5, "dbias")


# ------------------------------------------------------------------ LSTM recurrence (avse1 FusionNet, avse2 DPRNN)

@pytest.mark.parametrize("group", ["1", "0"])
@pytest.mark.parametrize("B,T,I,H,bidir", [(2, 376, 1540, 257, False), (3, 40, 1028, 257, False), (2, 17, 64, 128, True),
                                           (5, 9, 30, 61, True), (1, 1, 8, 5, False)])
def test_lstm_vs_torch_fp64(B, T, I, H, bidir, group, monkeypatch):
    """layers.HipLSTM (one HIP launch per direction and pass; group "1": the grouped kernels of lstm_group.hip, "0":
    one workgroup per sequence, lstm.hip) vs torch.nn.LSTM in fp64 on the CPU with the same weights: output and the
    gradients of the input and every parameter (max error relative to the tensor's max <= 2e-5 for the output,
    5e-5 for gradients: fp32 accumulation over T steps)."""
    from avse_challenge_amd.layers import HipLSTM
    monkeypatch.setattr(K(), "LSTM_GROUP", group == "1")
    torch.manual_seed(T + H)
    ref = torch.nn.LSTM(I, H, 1, batch_first=True, bidirectional=bidir).double()
    ours = HipLSTM(I, H, 1, batch_first=True, bidirectional=bidir).to(DEV)
    ours.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    x = det_input((B, T, I), 1600 + H)
    gy = det_input((B, T, H * (2 if bidir else 1)), 1601 + H)
    xr = x.double().requires_grad_(True)
    yr, (hnr, cnr) = ref(xr)
    (yr * gy.double()).sum().backward()
    xg = x.to(DEV).requires_grad_(True)
    y, (hn, cn) = ours(xg)
    (y * gy.to(DEV)).sum().backward()
    sc = lambda t: max(1e-6, float(t.abs().max()))                                                 # noqa: E731
    close(y, yr, 2e-5 * sc(yr), 0, "h")
    close(hn[0], yr[:, -1, :H], 2e-5 * sc(yr), 0, "h_n")
    assert hn.shape == hnr.shape and cn.shape == cnr.shape          # nn.LSTM's (h_n, c_n) contract
    close(hn, hnr, 2e-5 * sc(hnr), 0, "h_n (both directions)")
    close(cn, cnr, 2e-5 * sc(cnr), 0, "c_n")
    close(xg.grad, xr.grad, 5e-5 * sc(xr.grad), 0, "dx")
    rp = dict(ref.named_parameters())
    for k, p in ours.named_parameters():
        close(p.grad, rp[k].grad, 5e-5 * sc(rp[k].grad), 0, k)
    K().raise_if_kernel_error()


def test_lstm_group_kernels_at_the_avse1_shape(monkeypatch):
    """The grouped recurrence at the avse1 C2 FusionNet shape (B = 32 sequences x G = 8 workgroups = 256, the whole
    chip, T = 376, H = 257) vs lstm.hip's one workgroup per sequence: h, c, gates and the backward gate gradients
    within 1e-5 of them relative to their max (the dot products are summed in a different order); deterministic;
    every hand-off completed."""
    B, T, H = 32, 376, 257
    assert K()._lib.lib().avse_lstm_group_size(B, H) == 8
    gx = det_input((B, T, 4 * H), 1620).to(DEV)
    w = (0.06 * det_input((4 * H, H), 1621)).to(DEV)
    dh = det_input((B, T, H), 1622).to(DEV)
    monkeypatch.setattr(K(), "LSTM_GROUP", True)
    h1, c1, g1 = K().lstm_fwd(gx, w)
    d1 = K().lstm_bwd(dh, g1, c1, w)
    for rev in (False, True):
        hr, cr, gr = K().lstm_fwd(gx, w, reverse=rev)
        dr = K().lstm_bwd(dh, gr, cr, w, reverse=rev)
        K().raise_if_kernel_error()
        monkeypatch.setattr(K(), "LSTM_GROUP", False)
        h0, c0, g0 = K().lstm_fwd(gx, w, reverse=rev)
        d0 = K().lstm_bwd(dh, g0, c0, w, reverse=rev)
        monkeypatch.setattr(K(), "LSTM_GROUP", True)
        for a_, b_, n_ in ((hr, h0, "h"), (cr, c0, "c"), (gr, g0, "gates")):
            close(a_, b_, 1e-5 * float(b_.abs().max()), 0, f"{n_} reverse={rev}")
        close(dr, d0, 1e-5 * float(d0.abs().max()), 0, f"dgates reverse={rev}")
    assert torch.equal(K().lstm_fwd(gx, w)[0], h1) and torch.equal(K().lstm_bwd(dh, g1, c1, w), d1)   # deterministic


def test_lstm_group_residency_guard(monkeypatch):
    """The grouped kernels run only when a launch's B * G workgroups fit the device at once: the capacity query
    (occupancy x CUs) covers the avse1 grid (32 x 8 = 256, one 136 KB-LDS workgroup per CU); a device that holds fewer
    (kernels.LSTM_GROUP_CAPACITY_LIMIT stands in for it) takes lstm.hip's kernels instead, with their exact results."""
    L = K()._lib.lib()
    B, T, H = 32, 24, 257
    assert L.avse_lstm_group_capacity(H, 0) >= 256 and L.avse_lstm_group_capacity(H, 1) >= 256
    gx = det_input((B, T, 4 * H), 1630).to(DEV)
    w = (0.06 * det_input((4 * H, H), 1631)).to(DEV)
    dh = det_input((B, T, H), 1632).to(DEV)
    monkeypatch.setattr(K(), "LSTM_GROUP", False)
    h0, c0, g0 = K().lstm_fwd(gx, w)
    d0 = K().lstm_bwd(dh, g0, c0, w)
    monkeypatch.setattr(K(), "LSTM_GROUP", True)
    monkeypatch.setattr(K(), "LSTM_GROUP_CAPACITY_LIMIT", 255)
    h1, c1, g1 = K().lstm_fwd(gx, w)
    d1 = K().lstm_bwd(dh, g1, c1, w)
    assert torch.equal(h1, h0) and torch.equal(c1, c0) and torch.equal(d1, d0)      # the single-workgroup kernels
    monkeypatch.setattr(K(), "LSTM_GROUP_CAPACITY_LIMIT", None)
    h2, _, _ = K().lstm_fwd(gx, w)
    assert not torch.equal(h2, h0)          # the grouped kernels again (different summation order)
    close(h2, h0, 1e-5 * float(h0.abs().max()), 0, "h")
    K().raise_if_kernel_error()


def test_lstm_group_error_flag_raises():
    """The loud-failure path of the grouped LSTM (csrc/lstm_group.hip): a hand-off wait that times out writes
    0x71000000 + step into the device's sticky error flag (the launch's outputs are then invalid).  With that value in
    the flag — written here directly, as the kernel would — kernels.raise_if_kernel_error and ddp.Trainer's lagged
    per-step check both raise HipKernelError, and a reported error is cleared.  (Forcing a real non-resident grid was
    tried with a bounded CU-occupying kernel from the same and from another process, tools/lstm_hog_probe.py @ 8f1eec2: this
    pool's GPU never dispatched the LSTM beside it, so the launch only ever ran after the occupier — no timeout.)"""
    import bench
    from avse_challenge_amd import layers
    dev = torch.device(DEV)
    B, T, H = 32, 6, 257
    K().lstm_fwd(torch.randn(B, T, 4 * H, device=dev), 0.06 * torch.randn(4 * H, H, device=dev))
    torch.cuda.synchronize()
    K().raise_if_kernel_error()
    flag = K()._kernel_error_flag(dev)
    flag.fill_(0x71000000 + 3)
    with pytest.raises(K().HipKernelError, match="timed out"):
        K().raise_if_kernel_error()
    K().raise_if_kernel_error()                   # reported once, then cleared

    class Step:
        def __init__(self):
            self.model = layers.HipLSTM(16, H, 1, batch_first=True).to(dev)
            self.x = torch.randn(B, T, 16, device=dev)
            self.lr, self.clip = 1e-3, None

        def loss(self):
            return self.model(self.x)[0].square().mean()

    for graph in (False, True):
        st = Step()
        tr = bench.Trainer(st, 1, dev, use_graph=graph)
        tr()
        tr.capture()
        torch.cuda.synchronize()
        tr()                                      # enqueues the found copy it checks on the next step
        torch.cuda.synchronize()
        before = [p.detach().clone() for p in st.model.parameters()]
        flag.fill_(0x71000000 + 5)
        torch.cuda.synchronize()
        tr()                                      # sees the previous (clean) copy; its own update is skipped on device
        torch.cuda.synchronize()
        assert all(torch.equal(a, p) for a, p in zip(before, st.model.parameters())), "update not gated on the flag"
        with pytest.raises(K().HipKernelError, match="timed out"):
            tr()
        K().raise_if_kernel_error()               # cleared by the trainer's report
        tr()
        torch.cuda.synchronize()
        assert not all(torch.equal(a, p) for a, p in zip(before, st.model.parameters())), "update after the report"


# ------------------------------------------------------------------ fused dwconv <-> PReLU -> gLN (avse4 TCN)

@pytest.mark.parametrize("B,C,Kn,P,dil", [(2, 512, 3999, 3, 128), (3, 64, 300, 3, 4), (2, 40, 2500, 3, 1), (1, 8, 17, 5, 2),
                                          (2, 16, 5000, 3, 256), (2, 24, 1001, 5, 4), (1, 8, 13, 3, 4), (2, 8, 2050, 7, 64),
                                          (6, 512, 3999, 3, 128)])
def test_dwconv_prelu_gln_fused_vs_fp64(B, C, Kn, P, dil):
    """layers.dwconv_prelu_gln (two fused passes each way) vs the fp64 composition of the reference ops
    (model.py:278-292: depthwise conv1d, PReLU, gLN with EPS 1e-8 inside the sqrt): output and the gradients of
    x, the conv weight, the PReLU slope and gamma / beta (max error relative to the tensor's max: 1e-5, 1e-4)."""
    from avse_challenge_amd.layers import dwconv_prelu_gln
    x = det_input((B, C, Kn), 1700 + Kn)
    w = 0.5 * det_input((C, 1, P), 1701)
    alpha = torch.tensor([0.2])
    gamma = 1 + 0.1 * det_input((1, C, 1), 1702)
    beta = 0.1 * det_input((1, C, 1), 1703)
    gy = det_input((B, C, Kn), 1704)
    leaves = [t.double().requires_grad_(True) for t in (x, w, alpha, gamma, beta)]
    xr, wr, ar, gr, br = leaves
    y1 = torch.nn.functional.conv1d(xr, wr, padding=(P - 1) // 2 * dil, dilation=dil, groups=C)
    p = torch.where(y1 > 0, y1, ar * y1)
    mean = p.mean((1, 2), keepdim=True)
    var = ((p - mean) ** 2).mean((1, 2), keepdim=True)
    ref = gr * (p - mean) / (var + 1e-8) ** 0.5 + br
    (ref * gy.double()).sum().backward()
    g_leaves = [t.to(DEV).requires_grad_(True) for t in (x, w, alpha, gamma, beta)]
    y = dwconv_prelu_gln(*g_leaves, dil)
    (y * gy.to(DEV)).sum().backward()
    sc = lambda t: max(1e-6, float(t.abs().max()))                                         # noqa: E731
    close(y, ref, 1e-5 * sc(ref), 0, "y")
    for name, a_, r_ in zip(("dx", "dw", "dalpha", "dgamma", "dbeta"), g_leaves, leaves):
        close(a_.grad, r_.grad, 1e-4 * sc(r_.grad), 0, name)


# ------------------------------------------------------------------ dilated Conv2d weight gradient (avse1 AudioFeatNet)

@pytest.mark.parametrize("N,H,W,dil", [(2, 37, 257, 2), (2, 37, 257, 4), (1, 40, 257, 8), (2, 33, 257, 16),
                                       (1, 9, 64, 16), (1, 5, 65, 2), (3, 7, 130, 8), (1, 3, 31, 4), (2, 70, 100, 16)])
def test_dconv_wgrad_vs_fp64(N, H, W, dil):
    """K.dconv_wgrad (csrc/dconv_wgrad.hip) vs the fp64 weight gradient of Conv2d(64, 64, 5, padding=2d, dilation=d)
    (baseline/avse1/model.py:199-215) on channels-last inputs: every element within 1e-6 of its sum of |terms| (the
    exact-f32 MFMA accumulates one rounding per product: 1e-7 .. 3e-7 of it measured, cdna_hip_programming.md 'FP32-input MFMA'),
    which covers rows shorter than the dilation halo, pieces of 31..66 pixels and images smaller than the kernel."""
    x = det_input((N, 64, H, W), 1800 + dil + W)
    dy = det_input((N, 64, H, W), 1801 + dil + H)
    xd, dyd = x.double(), dy.double()
    truth = torch.nn.grad.conv2d_weight(xd, (64, 64, 5, 5), dyd, 1, 2 * dil, dil)
    bound = torch.nn.grad.conv2d_weight(xd.abs(), (64, 64, 5, 5), dyd.abs(), 1, 2 * dil, dil)
    cl = torch.channels_last
    got = K().dconv_wgrad(x.to(DEV).contiguous(memory_format=cl), dy.to(DEV).contiguous(memory_format=cl), dil)
    err = (got.double().cpu() - truth).abs()
    worst = float((err / (bound + 1e-30)).max())
    assert worst <= 1e-6, worst
    # NCHW inputs are converted, same result; deterministic (no atomics): bitwise equal on rerun
    got2 = K().dconv_wgrad(x.to(DEV), dy.to(DEV), dil)
    assert torch.equal(got, got2)
    # the bias gradient from the same pass: dy's channel sums, within 1e-6 of the sum of |dy|
    got3, db = K().dconv_wgrad(x.to(DEV).contiguous(memory_format=cl), dy.to(DEV).contiguous(memory_format=cl), dil,
                               bias_grad=True)
    assert torch.equal(got3, got)
    dbt, dbb = dyd.sum((0, 2, 3)), dyd.abs().sum((0, 2, 3))
    assert float(((db.double().cpu() - dbt).abs() / dbb).max()) <= 1e-6


@pytest.mark.parametrize("N,H,W,dil", [(2, 37, 257, 2), (2, 37, 257, 4), (1, 40, 257, 8), (2, 33, 257, 16),
                                       (1, 5, 300, 16), (3, 9, 256, 2), (1, 3, 513, 8), (2, 2, 257, 16)])
@pytest.mark.parametrize("transposed", [False, True])
def test_dconv_split_fwd_vs_fp64(N, H, W, dil, transposed):
    """K.dconv_fwd (csrc/dconv.hip: fp16x3 split-operand MFMA) vs fp64: the forward conv2d(x, W, padding=2d, dilation=d)
    and the input gradient conv_transpose2d(dy, W, ...) (baseline/avse1/model.py:199-215).  Every element within 1e-5 of
    its sum of |terms| (22-bit operands, fp32 accumulation), 256- or 512-pixel tiles spanning one to three rows, images shorter than the kernel, rows wider than two tiles.  The input mixes scales over 9
    decades (the power-of-two scale follows the tensor's max) and the result is bit-identical on rerun.  The bar is the
    fp32 class: 1e-5 of sum |terms| (an fp32 K = 1600 dot product rounds to ~2e-6 of it typically, ~1e-4 worst case;
    MIOpen's fp32 measured 3.4e-6 here), with MIOpen's own error printed beside it."""
    import torch.nn.functional as F
    x = det_input((N, 64, H, W), 1900 + dil + W + H)
    x = x * torch.exp(4.0 * det_input((N, 64, H, W), 1901 + dil))          # |x| from ~1e-7 to ~1e2
    w = 0.03 * det_input((64, 64, 5, 5), 1902 + dil)
    b = det_input((64,), 1903)
    xd, wd = x.double(), w.double()
    op = F.conv_transpose2d if transposed else F.conv2d
    truth = op(xd, wd, None, 1, 2 * dil, dilation=dil)
    bound = op(xd.abs(), wd.abs(), None, 1, 2 * dil, dilation=dil)
    cl = torch.channels_last
    xg = x.to(DEV).contiguous(memory_format=cl)
    got = K().dconv_fwd(xg, w.to(DEV), dil, transposed=transposed)
    assert got.is_contiguous(memory_format=cl) and got.shape == truth.shape
    worst = float(((got.double().cpu() - truth).abs() / (bound + 1e-30)).max())
    lib = op(xg, w.to(DEV), None, 1, 2 * dil, dilation=dil)
    worst_lib = float(((lib.double().cpu() - truth).abs() / (bound + 1e-30)).max())
    print(f"dconv split vs fp64: {worst:.2e} of sum|terms| (MIOpen fp32: {worst_lib:.2e})")
    assert worst <= 1e-5, (worst, worst_lib)
    assert torch.equal(K().dconv_fwd(xg, w.to(DEV), dil, transposed=transposed), got)
    if not transposed:
        gb = K().dconv_fwd(xg, w.to(DEV), dil, bias=b.to(DEV))
        close(gb - got, b.to(DEV)[None, :, None, None].expand_as(got), 1e-5 * float(got.abs().max()), 0, "bias")


@pytest.mark.parametrize("N,H,W,dil", [(2, 37, 257, 2), (2, 37, 257, 4), (1, 40, 257, 8), (2, 33, 257, 16),
                                       (1, 5, 300, 16), (3, 9, 64, 2), (1, 3, 65, 8), (2, 2, 257, 16)])
def test_dconv_wgrad16_vs_fp64(N, H, W, dil):
    """K.dconv_wgrad16 (csrc/dconv.hip: fp16x3 split MFMA from the split input and output gradient) vs the fp64 weight
    gradient of Conv2d(64, 64, 5, padding=2d, dilation=d) and dy's channel sums (the bias gradient from the same pass):
    every element within 1e-5 of its sum of |terms| (the split operands carry 22 bits; fp32 accumulation over the
    pixels: the fp32 class, as test_dconv_split_fwd_vs_fp64); 64-pixel chunks spanning one or two rows and the images'
    partial last chunks; deterministic."""
    x = det_input((N, 64, H, W), 1950 + dil + W) * torch.exp(3.0 * det_input((N, 64, H, W), 1951))
    dy = det_input((N, 64, H, W), 1952 + dil + H)
    xd, dyd = x.double(), dy.double()
    truth = torch.nn.grad.conv2d_weight(xd, (64, 64, 5, 5), dyd, 1, 2 * dil, dil)
    bound = torch.nn.grad.conv2d_weight(xd.abs(), (64, 64, 5, 5), dyd.abs(), 1, 2 * dil, dil)
    cl = torch.channels_last
    xm = torch.empty(2, device=DEV, dtype=torch.int32)
    dm = torch.empty(2, device=DEV, dtype=torch.int32)
    xq = K().split16(x.to(DEV).contiguous(memory_format=cl), xm)
    dq = K().split16(dy.to(DEV).contiguous(memory_format=cl), dm)
    dw, db = K().dconv_wgrad16((xq, xm[:1]), (dq, dm[:1]), (N, 64, H, W), dil, bias_grad=True)
    worst = float(((dw.double().cpu() - truth).abs() / (bound + 1e-30)).max())
    print(f"dconv wgrad16 vs fp64: {worst:.2e} of sum|terms|")
    assert worst <= 1e-5, worst
    dbt, dbb = dyd.sum((0, 2, 3)), dyd.abs().sum((0, 2, 3))
    assert float(((db.double().cpu() - dbt).abs() / dbb).max()) <= 1e-5
    dw2 = K().dconv_wgrad16((xq, xm[:1]), (dq, dm[:1]), (N, 64, H, W), dil)
    assert torch.equal(dw2, dw)


def test_dilated_conv2d_module_split_path_vs_torch():
    """layers.DilatedConv2d at the avse1 spectrogram width (W = 257: the split-fp16 path of csrc/dconv.hip for the
    output, the input gradient and the weight / bias gradients) vs nn.Conv2d in fp64 on the same parameters; the
    bias-free form (bias_to_bn=True) returns the bias gradient all the same."""
    from avse_challenge_amd.layers import DilatedConv2d
    torch.manual_seed(4)
    for dil in (2, 16):
        ref = torch.nn.Conv2d(64, 64, 5, padding=2 * dil, dilation=dil).double()
        ours = DilatedConv2d(64, 64, 5, padding=2 * dil, dilation=dil).to(DEV)
        ours.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
        ours.to(memory_format=torch.channels_last)
        x = det_input((2, 64, 20, 257), 1960 + dil)
        gy = det_input((2, 64, 20, 257), 1961 + dil)
        xr = x.double().requires_grad_(True)
        yr = ref(xr)
        (yr * gy.double()).sum().backward()
        xg = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        assert ours.hip_ok(xg)
        y = ours(xg)
        (y * gy.to(DEV)).sum().backward()
        sc = lambda t: max(1e-6, float(t.abs().max()))                                             # noqa: E731
        close(y, yr, 2e-5 * sc(yr), 0, f"y d={dil}")
        close(xg.grad, xr.grad, 2e-5 * sc(xr.grad), 0, f"dx d={dil}")
        close(ours.weight.grad, ref.weight.grad, 2e-5 * sc(ref.weight.grad), 0, f"dw d={dil}")
        close(ours.bias.grad, ref.bias.grad, 2e-5 * sc(ref.bias.grad), 0, f"db d={dil}")


def test_audiofeat_bias_folded_into_batchnorm():
    """AudioFeatNet (channels-last, training mode) with the conv2..conv5 biases folded into their BatchNorms
    (DilatedConv2d bias_to_bn + bn_act folded_bias) vs the same net with the biases added by the library convolution
    (layers.HIP_DCONV = False): output and BatchNorm running statistics agree to fp32 rounding."""
    import copy
    from avse_challenge_amd import avse1
    torch.manual_seed(5)
    a = avse1.AudioFeatNet().to(DEV).use_channels_last()
    for m in a.modules():
        if isinstance(m, torch.nn.Conv2d) and m.bias is not None:
            torch.nn.init.uniform_(m.bias, -0.5, 0.5)            # a bias large enough to matter
    b = copy.deepcopy(a)
    spec = det_input((2, 1, 40, 70), 1860).abs().to(DEV)
    gy = det_input((2, 40, 280), 1861).to(DEV)
    assert a.conv2.hip_ok(torch.empty(1, 64, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last))
    ya = a(spec)
    (ya * gy).sum().backward()
    from avse_challenge_amd import layers
    old = layers.HIP_DCONV
    layers.HIP_DCONV = False
    try:
        yb = b(spec)
        (yb * gy).sum().backward()
    finally:
        layers.HIP_DCONV = old
    sc = lambda t: max(1e-6, float(t.detach().abs().max()))                                        # noqa: E731
    close(ya, yb, 1e-4 * sc(yb), 0, "y")
    # gradients: the two fp32 runs round differently, so single ReLU masks flip and the strongly cancelling sums
    # below them (bn0's 1-element weight gradient: 0.5 % of the whole vector moved) differ by more than any
    # rounding bar.  The folded model's gradients are checked against the fp64 oracle with the masks imposed
    # (test_gpu_models.py::test_avse1_wave_frontend_and_train_step_vs_oracle[True]); here: every conv2..conv5 bias
    # gradient is its output gradient's channel sum, which BatchNorm makes ~0 (<< the weight gradient's scale)
    pa = dict(a.named_parameters())
    for i in range(2, 6):
        assert float(pa[f"conv{i}.bias"].grad.abs().max()) <= 1e-4 * sc(pa[f"conv{i}.weight"].grad), i
    ba, bb = dict(a.named_buffers()), dict(b.named_buffers())
    for k in ba:
        close(ba[k].float(), bb[k].float(), 1e-5 * sc(bb[k].float()), 0, k)


def test_dilated_conv2d_module_grads_vs_torch():
    """layers.DilatedConv2d (AudioFeatNet conv2..conv5 module, channels-last): output, input / weight / bias gradients
    vs nn.Conv2d in fp64 on the same parameters."""
    from avse_challenge_amd.layers import DilatedConv2d
    torch.manual_seed(3)
    ref = torch.nn.Conv2d(64, 64, 5, padding=8, dilation=4).double()
    ours = DilatedConv2d(64, 64, 5, padding=8, dilation=4).to(DEV)
    ours.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    ours.to(memory_format=torch.channels_last)
    x = det_input((2, 64, 30, 70), 1850)
    gy = det_input((2, 64, 30, 70), 1851)
    xr = x.double().requires_grad_(True)
    (ref(xr) * gy.double()).sum().backward()
    xg = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ours(xg)
    (y * gy.to(DEV)).sum().backward()
    sc = lambda t: max(1e-6, float(t.abs().max()))                                                 # noqa: E731
    close(y, ref(xr), 2e-5 * sc(ref(xr)), 0, "y")
    close(xg.grad, xr.grad, 2e-5 * sc(xr.grad), 0, "dx")
    close(ours.weight.grad, ref.weight.grad, 2e-5 * sc(ref.weight.grad), 0, "dw")
    close(ours.bias.grad, ref.bias.grad, 2e-5 * sc(ref.bias.grad), 0, "db")


@pytest.mark.parametrize("shape", [(2, 64, 75, 24, 24), (3, 5, 7, 9, 11), (1, 70, 3, 5, 13)])
def test_frames_nhwc_transpose(shape):
    """layers.frames_nhwc on csrc/transpose.hip: (B, C, T, H, W) -> (B*T, C, H, W) channels-last equals torch's
    permute exactly, and its backward is the exact inverse permutation (tiles not dividing C or T*H*W included)."""
    from avse_challenge_amd.layers import frames_nhwc
    B, C, T, H, W = shape
    x = det_input(shape, 1870).to(DEV).requires_grad_(True)
    y = frames_nhwc(x)
    ref = x.detach().permute(0, 2, 3, 4, 1).reshape(B * T, H, W, C).permute(0, 3, 1, 2)
    assert y.is_contiguous(memory_format=torch.channels_last) and torch.equal(y, ref)
    gy = det_input((B * T, C, H, W), 1871).to(DEV).contiguous(memory_format=torch.channels_last)
    (gx,) = torch.autograd.grad(y, x, gy)
    assert torch.equal(gx, gy.view(B, T, C, H, W).permute(0, 2, 1, 3, 4))


@pytest.mark.parametrize("N,H,W", [(2, 376, 257), (3, 37, 130)])
def test_conv1_module_nhwc_vs_torch(N, H, W):
    """AudioFeatNet.conv1 (DilatedConv2d(1, 64, 5, padding=2) with nhwc_out: layers._Conv1Fn on csrc/conv1.hip) at the
    avse1 spectrogram shape and a ragged one (partial row tiles and 8 x 32 gradient tiles): channels-last output, and
    output / input / weight / bias gradients vs nn.Conv2d in fp64; with bias_to_bn the bias is left out of the output
    and its gradient is unchanged."""
    from avse_challenge_amd.layers import DilatedConv2d
    torch.manual_seed(4)
    ref = torch.nn.Conv2d(1, 64, 5, padding=2).double()
    ours = DilatedConv2d(1, 64, 5, padding=2, dilation=1).to(DEV)
    ours.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    ours.nhwc_out = True
    x = det_input((N, 1, H, W), 1860)
    gy = det_input((N, 64, H, W), 1861)
    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    (yr * gy.double()).sum().backward()
    sc = lambda t: max(1e-6, float(t.abs().max()))                                                 # noqa: E731
    for bias_to_bn in (False, True):
        ours.zero_grad()
        xg = x.to(DEV).requires_grad_(True)
        y = ours(xg, bias_to_bn=bias_to_bn)
        assert y.is_contiguous(memory_format=torch.channels_last)
        want = yr - ref.bias.view(1, -1, 1, 1) if bias_to_bn else yr
        close(y, want, 2e-6 * sc(want), 0, "y")
        (y * gy.to(DEV)).sum().backward()
        close(xg.grad, xr.grad, 2e-5 * sc(xr.grad), 0, "dx")
        close(ours.weight.grad, ref.weight.grad, 2e-5 * sc(ref.weight.grad), 0, "dw")
        close(ours.bias.grad, ref.bias.grad, 2e-5 * sc(ref.bias.grad), 0, "db")


@pytest.mark.parametrize("N,H,W", [(2, 376, 257), (3, 7, 13)])
def test_convf_vs_fp64(N, H, W):
    """AudioFeatNet.convf = Conv2d(64, 4, 1) on channels-last activations (layers.conv1x1_to4 -> csrc/convf.hip): output,
    input, weight and bias gradients vs nn.Conv2d in fp64 (fp32 class: 1e-5 of each quantity's sum of |terms|), at the
    avse1 C2 frame shape and a ragged pixel count; deterministic on rerun."""
    from avse_challenge_amd.layers import conv1x1_to4
    torch.manual_seed(6)
    ref = torch.nn.Conv2d(64, 4, 1).double()
    ours = torch.nn.Conv2d(64, 4, 1).to(DEV)
    ours.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    x = det_input((N, 64, H, W), 1880) * torch.exp(det_input((N, 64, H, W), 1881))
    gy = det_input((N, 4, H, W), 1882)
    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    (yr * gy.double()).sum().backward()
    aw, ab = ref.weight.detach().abs(), ref.bias.detach().abs()
    bound_y = F.conv2d(x.double().abs(), aw, ab)
    bound_dx = torch.nn.grad.conv2d_input(x.shape, aw, gy.double().abs())
    bound_dw = torch.nn.grad.conv2d_weight(x.double().abs(), aw.shape, gy.double().abs())
    runs = []
    for _ in range(2):
        ours.zero_grad()
        xg = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        y = conv1x1_to4(xg, ours)
        assert y.grad_fn is not None and "ConvF" in type(y.grad_fn).__name__, type(y.grad_fn).__name__
        assert y.is_contiguous(memory_format=torch.channels_last)
        (y * gy.to(DEV)).sum().backward()
        runs.append((y.detach().clone(), xg.grad.clone(), ours.weight.grad.clone(), ours.bias.grad.clone()))
    y, dx, dw, db = runs[0]
    for got, want, bound, what in ((y, yr, bound_y, "y"), (dx, xr.grad, bound_dx, "dx"),
                                   (dw, ref.weight.grad, bound_dw, "dw"), (db, ref.bias.grad, gy.double().abs().sum((0, 2, 3)), "db")):
        err = float(((got.double().cpu() - want.detach()).abs() / (bound + 1e-30)).max())
        assert err <= 1e-5, (what, err)
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))


def test_trunk_conv2d_module_grads_vs_torch():
    """layers.TrunkConv2d (stride 2, NCHW: the library path) and the same conv on channels-last activations (csrc/sconv.hip
    forward, weight gradient and stride-2 input gradient): output and input / weight gradients vs nn.Conv2d in fp64."""
    from avse_challenge_amd.layers import TrunkConv2d
    torch.manual_seed(4)
    ref = torch.nn.Conv2d(64, 128, 3, stride=2, padding=1, bias=False).double()
    ours = TrunkConv2d(64, 128, 2).to(DEV)
    ours.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    x = det_input((3, 64, 24, 24), 1950)
    gy = det_input((3, 128, 12, 12), 1951)
    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    (yr * gy.double()).sum().backward()
    sc = lambda t: max(1e-6, float(t.abs().max()))                                                 # noqa: E731
    for fmt in (torch.contiguous_format, torch.channels_last):
        ours.to(memory_format=fmt)
        ours.zero_grad()
        xg = x.to(DEV).contiguous(memory_format=fmt).requires_grad_(True)
        y = ours(xg)
        (y * gy.to(DEV)).sum().backward()
        close(y, yr, 2e-5 * sc(yr), 0, f"y {fmt}")
        close(xg.grad, xr.grad, 2e-5 * sc(xr.grad), 0, f"dx {fmt}")
        close(ours.weight.grad, ref.weight.grad, 2e-5 * sc(ref.weight.grad), 0, f"dw {fmt}")


def test_conv3d_fwd_avse4_frontend_vs_fp64():
    """The avse4 lip front-end Conv3d(1, 64, (5, 7, 7), stride (1, 2, 2), padding (2, 3, 3)) forward on the exact-fp32
    MFMA kernel (conv3d_fwd.hip, 112 x 112 normalised grey frames; baseline/avse4/utils.py:97-118) vs fp64: within 1e-5
    of sum |w x| per output, partial last tile of each plane included (56 x 56 = 3136 = 8 x 384 + 64 pixels)."""
    import torch.nn.functional as F
    k = K()
    g = torch.Generator(device="cuda").manual_seed(11)
    x = (torch.rand(2, 1, 7, 112, 112, device="cuda", generator=g) - 0.4161) / 0.1688
    w = 0.05 * torch.randn(64, 1, 5, 7, 7, device="cuda", generator=g)
    assert k.conv3d_fwd_supported(x, w, (1, 2, 2), (2, 3, 3))
    y = k.conv3d_fwd(x, w)
    ref = F.conv3d(x.double(), w.double(), None, (1, 2, 2), (2, 3, 3))
    mag = F.conv3d(x.double().abs(), w.double().abs(), None, (1, 2, 2), (2, 3, 3))
    assert y.shape == ref.shape
    assert float(((y.double() - ref).abs() / (mag + 1e-30)).max()) <= 1e-5
