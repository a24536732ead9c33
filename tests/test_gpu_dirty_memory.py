"""Every kernel family on dirty memory: each wrapper runs once on the allocator's memory as it comes and once with every
``torch.empty`` of the package poisoned (tests/_dirty.py: NaN as fp16 / bf16 / fp32, a large positive int32), on the same
inputs.  The dirty run must be NaN-free over the logical extent of every result and bit-equal to the clean run
(``torch.equal``), attached max words, split planes and in-place-updated arguments included: the float kernels use no
float atomics and atomicMax does not depend on the order, so nothing else is acceptable.  What this finds: a first-stage
workgroup that skipped its partial sum, a max word read before its reset, a pad column that reached a sum.

The clean run is held to a reference at the same shape: the shapes are parametrisations of the existing fp64 / oracle
tests (named in each case), which test_replay_under_dirty_memory also runs again on poisoned memory; where a shape or
an option has no such test the case carries its own fp64 reference (``ref=``).

Integer / uint8 buffers: the max words (ymax, dxmax, mb, mbd, wm, xm: written by atomicMax after a stream-ordered
reset, read only as a scale exponent that split_exp clamps), the pool argmax bytes (compared with window positions,
never added to an address), the xq / wq images (data) and the grouped LSTM's hand-off workspace (zeroed by a memset in
its entry point, in stream order, before the launch) are all poisoned: none of them is used as an address, an offset
or a trip count before the kernel that owns it has written it.  Caller-zeroed words (``dz_max``, ``dx_max``,
``out_z_max``: include/avse_hip.h) are passed zeroed, as the models pass them.

Not covered: ``layers._Conv1Fn._rows`` allocates with ``x.new_empty`` (not the module's ``torch``); it is the
narrow-frame torch path and the two assignments that follow write every element before anything reads it.
conv3d_fwd is compiled for the two lip front-end frame sizes only, so its cases are those (one frame deep).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _dirty
import test_gpu_bn_bwd_fused as tbn
import test_gpu_frontend_fused as tff
import test_gpu_kernels as tk
import test_gpu_projgemm as tpg
import test_gpu_sconv as tsc
import test_gpu_stream_kernels as tst
from oracle import mamba_ref, stft_ref
from oracle.det_init import det_init_, det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
close = tk.close


def K():
    from avse_challenge_amd import kernels
    return kernels


def E(*shape, dtype=torch.float32):
    """A buffer the test itself hands to a wrapper: from the kernels module's allocator, so poisoned in the dirty run."""
    return K().torch.empty(*shape, device=DEV, dtype=dtype)


def dev(t, fmt=None):
    if t is None:
        return None
    t = t.to(DEV)
    return t if fmt is None else t.contiguous(memory_format=fmt)


# ------------------------------------------------------------------ comparison

def _leaves(obj, name="out"):
    """(name, tensor) for every tensor in a result: attached max words, split planes and split-output bytes included."""
    k = K()
    if obj is None:
        return
    if isinstance(obj, k.Split):
        yield name + ".hi", obj.hi
        yield name + ".lo", obj.lo
        yield name + ".mb", obj.mb
    elif torch.is_tensor(obj):
        sp = k.planes_of(obj)
        if sp is not None:                       # a carrier's own elements are not values: its planes are
            yield from _leaves(sp, name + ".planes")
            return
        if k.is_split_q(obj):
            yield name + ".q", k.q_view(obj).view(torch.float16)
        else:
            yield name, obj
        mb = getattr(obj, k.ABSMAX_ATTR, None)
        if torch.is_tensor(mb):
            yield name + ".absmax", mb
    elif isinstance(obj, dict):
        for key, v in obj.items():
            yield from _leaves(v, f"{name}.{key}")
    elif isinstance(obj, (tuple, list)):
        for i, v in enumerate(obj):
            yield from _leaves(v, f"{name}[{i}]")
    else:
        raise TypeError(f"{name}: {type(obj)}")


def assert_same(clean, dirty):
    a, b = list(_leaves(clean)), list(_leaves(dirty))
    assert [n for n, _ in a] == [n for n, _ in b]
    assert a, "nothing compared"
    for (name, x), (_, y) in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and x.stride() == y.stride(), name
        if y.dtype.is_floating_point:
            assert not bool(torch.isnan(y).any()), f"{name}: NaN in the dirty run ({int(torch.isnan(y).sum())} elements)"
        if not torch.equal(x, y):
            d = (x.double() - y.double()).abs()
            raise AssertionError(f"{name}: dirty run differs from the clean run in {int((x != y).sum())} of "
                                 f"{x.numel()} elements (max |diff| {float(d.max()):.3e})")


def _full_rows(t):
    """The padded rows of a (b, r, c) plane whose pad columns the kernel writes as zeros."""
    return t.as_strided((t.shape[0], t.shape[1], t.stride(1)), t.stride(), t.storage_offset())


# ------------------------------------------------------------------ the cases: name -> () -> (run, ref or None)

CASES = {}


def case(name):
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return deco


def _params(fn, rows, fmt):
    for r in rows:
        case(fmt.format(*r))(functools.partial(fn, *r))


# ---- selective scan (reference at these shapes: tk.test_scan_edges_vs_oracle["full"]; the carried-state and
# accumulate options: ref below)

def _scan_inputs(b, d, l, extra=0):
    seed = b * 1000 + d * 10 + l
    lt = l + extra
    ins = dict(u=det_input((b, d, lt), seed), delta=0.5 * det_input((b, d, lt), seed + 1),
               A=-torch.exp(0.5 * det_input((d, 16), seed + 2)), B=det_input((b, 1, 16, lt), seed + 3),
               C=det_input((b, 1, 16, lt), seed + 4), D=det_input((d,), seed + 5), z=det_input((b, d, lt), seed + 6),
               delta_bias=0.3 * det_input((d,), seed + 7))
    return ins, det_input((b, d, l), seed + 8)


SCAN_SHAPES = [(3, 130, 129), (1, 64, 1)]


def _scan_fwd(b, d, l):
    ins, _ = _scan_inputs(b, d, l)
    gpu = {k: dev(v) for k, v in ins.items()}
    flipped = {k: (v.flip(-1).contiguous() if k in ("u", "delta", "B", "C", "z") else v) for k, v in gpu.items()}
    acc0 = dev(det_input((b, d, l), 39))

    def run():
        k = K()
        plain = k.selective_scan_fwd(**gpu, delta_softplus=True)
        rev = k.selective_scan_fwd(**gpu, delta_softplus=True, reverse=True)
        acc, mx = acc0.clone(), torch.zeros(1, device=DEV, dtype=torch.int32)      # the caller zeroes out_z_max
        k.selective_scan_fwd(**gpu, delta_softplus=True, return_out=False, out_z_acc=acc, out_z_max=mx)
        return plain, rev, acc, mx

    def ref(res):
        """The options the edge-shape test does not take, by the bars of their own tests at other shapes:
        test_scan_and_cconv_reverse_equal_flipped (1e-6) and test_scan_fwd_out_z_accumulate (exact in fp32)."""
        plain, rev, acc, mx = res
        fl = K().selective_scan_fwd(**flipped, delta_softplus=True)
        close(rev[2], fl[2].flip(-1), 1e-6, 1e-6, "reverse out_z")
        close(rev[1], fl[1], 1e-6, 1e-6, "reverse checkpoints")
        assert torch.equal(acc, acc0 + plain[2])
        assert int(mx.item()) == int(acc.abs().amax().reshape(1).view(torch.int32).item())
    return run, ref


def _scan_state(b, d, l):
    """initial_state / return_last_state / checkpoints: the fp64 oracle over a 5-step prefix and the sequence gives the
    state after the prefix (the kernel's initial state), the outputs after it and the last state; bars of
    test_scan_edges_vs_oracle (1e-4)."""
    p = 5
    ins, _ = _scan_inputs(b, d, l, extra=p)
    time = ("u", "delta", "B", "C", "z")
    d64 = {k: v.double() for k, v in ins.items()}
    pre = {k: (v[..., :p] if k in time else v) for k, v in d64.items()}
    h0 = mamba_ref.selective_scan(**pre, delta_softplus=True, return_last_state=True, acc_dtype=torch.float64)[1]
    full, last = mamba_ref.selective_scan(**d64, delta_softplus=True, return_last_state=True, acc_dtype=torch.float64)
    gpu = {k: dev(v[..., p:].contiguous() if k in time else v) for k, v in ins.items()}
    h0g = dev(h0.float().contiguous())

    def run():
        dst = E(b, d, 16)
        a = K().selective_scan_fwd(**gpu, delta_softplus=True, initial_state=h0g, return_last_state=True)
        c = K().selective_scan_fwd(**gpu, delta_softplus=True, initial_state=h0g, return_last_state=dst,
                                   checkpoints=False)
        return a, c

    def ref(res):
        (out, x, out_z, st), (_, x2, out_z2, st2) = res
        assert x2 is None and x is not None
        close(out_z, full[..., p:], 1e-4, 1e-4, "out_z from the carried state")
        close(st, last, 1e-4, 1e-4, "last state")
        assert torch.equal(out_z, out_z2) and torch.equal(st, st2)
    return run, ref


def _scan_bwd(b, d, l, accumulate):
    ins, dout = _scan_inputs(b, d, l)
    gpu = {k: dev(v) for k, v in ins.items()}
    out, x, out_z = K().selective_scan_fwd(**gpu, delta_softplus=True)
    args = [gpu[k] for k in ("u", "delta", "A", "B", "C", "D", "z", "delta_bias")] + [dev(dout), x, out]
    if not accumulate:
        def run():                              # all nine outputs (recompute_out_z) and the workspace
            return K().selective_scan_bwd(*args, None, True, True)

        def ref(res):
            close(res[8], out_z, 1e-5, 1e-5, "recomputed out_z")
        return run, ref
    base = K().selective_scan_bwd(*args, None, True, False)
    buf0 = dev(det_input((b, d, l), 61))

    def run():
        buf, mx = buf0.clone(), torch.zeros(1, device=DEV, dtype=torch.int32)      # the caller zeroes dz_max
        res = K().selective_scan_bwd(*args, buf, True, False, dz_accumulate=True, dz_max=mx)
        return res, buf, mx

    def ref(r):
        res, buf, mx = r
        assert res[7].data_ptr() == buf.data_ptr() and torch.equal(buf, buf0 + base[7])
        assert int(mx.item()) == int(buf.abs().amax().reshape(1).view(torch.int32).item())
        for i in range(7):
            assert torch.equal(res[i], base[i]), i
    return run, ref


_params(_scan_fwd, SCAN_SHAPES, "scan-fwd-{}x{}x{}")
_params(_scan_state, SCAN_SHAPES, "scan-state-{}x{}x{}")
_params(_scan_bwd, [s + (False,) for s in SCAN_SHAPES], "scan-bwd-{}x{}x{}")
_params(_scan_bwd, [s + (True,) for s in SCAN_SHAPES], "scan-bwd-dz-accumulate-{}x{}x{}")


# ---- dtproj (tk.test_dtproj_vs_fp64 has these rows, (2, 130, 64, 257) in bf16)

def _dtproj(b, D, R, l, dtype):
    seed = b + D + R + l
    xfull = K().bdl_empty(b, R + 32, l, dtype, torch.device(DEV))
    xfull.copy_(det_input((b, R + 32, l), seed).to(DEV, dtype))
    x = xfull[:, :R]
    w = ((R ** -0.5) * det_input((D, R), seed + 1)).to(DEV, dtype)
    bias = (-4.0 + det_input((D,), seed + 2)).to(DEV)
    return (lambda: (K().dtproj(w, x, bias), K().dtproj(w, x, None, softplus=False))), None


_params(_dtproj, [(3, 100, 7, 301, torch.float32), (2, 130, 64, 257, torch.bfloat16), (1, 64, 1, 5, torch.float32)],
        "dtproj-{}x{}x{}x{}-{}")


# ---- causal conv1d (tk.test_cconv_vs_oracle has the shapes, w = 4, SiLU; conv_state and dx_accumulate: ref below)

def _cconv(b, d, l, dtype):
    w = 4
    x = det_input((b, d, l), 300 + l).to(dtype)
    wt, bias, gy = det_input((d, w), 301), det_input((d,), 302), det_input((b, d, l), 303).to(dtype)
    conv0 = det_input((b, d, w), 304).to(dtype)
    cat = torch.cat([conv0, x], -1).double()
    ref_state = mamba_ref.causal_conv1d(cat, wt.double(), bias.double(), True)[..., w:]
    xg, wg, bg, gg = dev(x), dev(wt), dev(bias), dev(gy)
    dx0 = K().causal_conv1d_bwd(xg, wg, bg, gg, silu=True)[0]
    lp = (l + 31) // 32 * 32
    store0 = dev(det_input((b, d, lp), 305).to(dtype))

    def run():
        out = K().causal_conv1d_fwd(xg, wg, bg, True)
        grads = K().causal_conv1d_bwd(xg, wg, bg, gg, silu=True)
        st = dev(conv0).clone()
        out_s = K().causal_conv1d_fwd(xg, wg, bg, True, conv_state=st)
        store, mx = store0.clone(), torch.zeros(1, device=DEV, dtype=torch.int32)     # the caller zeroes dx_max
        acc = K().causal_conv1d_bwd(xg, wg, bg, gg, dx=store[..., :l], silu=True, dx_accumulate=True, dx_max=mx)
        into = E(b, d, lp, dtype=dtype)[..., :l]                   # dx written into a passed (dirty) view
        K().causal_conv1d_bwd(xg, wg, bg, gg, dx=into, silu=True)
        rev = K().causal_conv1d_fwd(xg, wg, bg, True, reverse=True), \
            K().causal_conv1d_bwd(xg, wg, bg, gg, silu=True, reverse=True)
        return out, grads, out_s, st, acc, mx, into, rev

    def ref(res):
        out, grads, out_s, st, acc, mx, into, rev = res
        rtol = 1e-5 if dtype == torch.float32 else 2 ** -8
        fx, fg = xg.flip(-1).contiguous(), gg.flip(-1).contiguous()      # reverse == flip(forward(flip)), its test's bars
        close(rev[0].float(), K().causal_conv1d_fwd(fx, wg, bg, True).flip(-1).float(), 1e-6,
              1e-6 if dtype == torch.float32 else 2 ** -8, "reverse fwd")
        fr = K().causal_conv1d_bwd(fx, wg, bg, fg, silu=True)
        close(rev[1][0].float(), fr[0].flip(-1).float(), 1e-5, rtol, "reverse dx")
        close(rev[1][1], fr[1], 1e-4, 1e-5, "reverse dw")
        close(rev[1][2], fr[2], 1e-4, 1e-5, "reverse db")
        close(out_s.float(), ref_state, 1e-5, rtol, "out from conv_state")
        assert torch.equal(st, dev(cat[..., -w:].to(dtype)))
        assert torch.equal(acc[1], grads[1]) and torch.equal(acc[2], grads[2]) and torch.equal(into, grads[0])
        if dtype == torch.float32:
            assert torch.equal(acc[0], store0[..., :l] + dx0)
            assert int(mx.item()) == int(acc[0].abs().amax().reshape(1).view(torch.int32).item())
    return run, ref


_params(_cconv, [(3, 70, 34, torch.float32), (1, 5, 257, torch.float32), (2, 33, 250, torch.float32),
                 (1, 8, 4100, torch.float32), (2, 33, 250, torch.bfloat16)], "cconv-{}x{}x{}-{}")


def _step_ops(dtype):
    """causal_conv1d_update / selective_state_update, b 3, d 70 (tst.test_step_ops_vs_oracle[3-70]): three steps from
    non-zero states, both states updated in place."""
    b, d, w, steps, seed = 3, 70, 4, 3, 7000 + 30 + 70
    xs, zs = det_input((steps, b, d), seed).to(dtype), det_input((steps, b, d), seed + 1).to(dtype)
    dts = (0.5 * det_input((steps, b, d), seed + 2)).to(dtype)
    Bs, Cs = det_input((steps, b, 16), seed + 3).to(dtype), det_input((steps, b, 16), seed + 4).to(dtype)
    A = dev(-torch.exp(0.5 * det_input((d, 16), seed + 5)))
    D, dt_bias = dev(det_input((d,), seed + 6)), dev(0.3 * det_input((d,), seed + 7))
    wt, cb = dev(det_input((d, w), seed + 8)), dev(det_input((d,), seed + 9))
    conv0, ssm0 = dev(det_input((b, d, w), seed + 10).to(dtype)), dev(det_input((b, d, 16), seed + 11))
    xs, zs, dts, Bs, Cs = (dev(t) for t in (xs, zs, dts, Bs, Cs))

    def run():
        conv_s, ssm_s, outs = conv0.clone(), ssm0.clone(), []
        for t in range(steps):
            outs.append(K().causal_conv1d_update(xs[t], conv_s, wt, cb, silu=True))
            outs.append(K().selective_state_update(ssm_s, xs[t], dts[t], A, Bs[t], Cs[t], D, zs[t], dt_bias, True))
        return outs, conv_s, ssm_s
    return run, None


_params(_step_ops, [(torch.float32,), (torch.bfloat16,)], "step-ops-3x70-{}")


# ---- add + RMSNorm: rows 37, n 32 and 1024 (the existing test has 333 rows: fp64 reference here, its bars)

def _rmsnorm(n, bf16):
    rows = 37
    h = det_input((rows, n), 400 + n)
    r, w = det_input((rows, n), 401), 1.0 + 0.1 * det_input((n,), 402)
    gy, gr = det_input((rows, n), 403), det_input((rows, n), 404)
    if bf16:
        h, gy = h.to(torch.bfloat16), gy.to(torch.bfloat16)
    hd, rd, wd = h.double().requires_grad_(True), r.double().requires_grad_(True), w.double().requires_grad_(True)
    res = hd + rd
    y = res * torch.rsqrt(res.pow(2).mean(-1, keepdim=True) + 1e-5) * wd          # mamba_ref.rms_norm, kept in fp64
    (y * gy.double()).sum().backward(retain_graph=True)
    (res * gr.double()).sum().backward()
    hg, rg, wg, gyg, grg = (dev(t) for t in (h, r, w, gy, gr))

    def run():
        yk, rk, rstd = K().add_rmsnorm_fwd(hg, rg, wg, 1e-5, out_dtype=torch.bfloat16 if bf16 else None)
        y0, r0, rstd0 = K().add_rmsnorm_fwd(hg, None, wg, 1e-5)
        dx, dw = K().rmsnorm_bwd(gyg, grg, rk, wg, rstd)
        return yk, rk, rstd, y0, r0, rstd0, dx, dw

    def ref(out):
        yk, rk, rstd, y0, r0, rstd0, dx, dw = out
        close(yk.float(), y, 1e-5, 2 ** -8 if bf16 else 1e-5, "y")
        close(rk, res, 1e-6, 0, "res")
        close(dx, hd.grad, 1e-5, 1e-5, "dx")
        close(dw, wd.grad, 1e-3, 1e-5, "dw")
        for t in (y0, dx):
            assert int(getattr(t, K().ABSMAX_ATTR).item()) == int(t.abs().max().view(torch.int32).item())
    return run, ref


_params(_rmsnorm, [(32, False), (1024, False), (32, True), (1024, True)], "rmsnorm-37x{}-bf16rows-{}")


# ---- STFT / iSTFT at T = 1000 (tk.test_stft_vs_oracle[1000]; the iSTFT against the oracle here, its 1e-6 rms bar)

@case("stft-istft-1000")
def _stft():
    T = 1000
    y = (0.1 * det_input((3, T), 500 + T)).numpy()
    wave = torch.from_numpy(y).to(DEV)
    gain = dev(0.5 + det_input((3, 1 + T // 128, 257), 511, "uniform"))

    def run():
        mag, spec = K().stft(wave, return_complex=True)
        return mag, torch.view_as_real(spec), K().stft(wave), K().istft(mag * gain, spec, T)

    def ref(res):
        mag, spec, mag2, out = res
        r = stft_ref.stft(y)
        close(mag, np.abs(r).transpose(0, 2, 1), 2e-6 * float(np.abs(r).max()), 0, "|X|")
        assert torch.equal(mag, mag2)
        S = torch.view_as_complex(spec).cpu().numpy().transpose(0, 2, 1)
        want = stft_ref.istft((mag * gain).cpu().numpy().transpose(0, 2, 1) * np.exp(1j * np.angle(S)), length=T)
        assert np.sqrt(np.mean((out.cpu().numpy() - want) ** 2)) <= 1e-6
    return run, ref


# ---- lip Conv3d (tk.test_conv3d_wgrad_vs_fp64 / _uint8_vs_fp64[1] / test_conv3d_fwd_vs_fp64 have these rows)

def _conv3d_wgrad(cin, T, H, W):
    x = dev(det_input((2, cin, T, H, W), 700 + cin, "uniform", 255.0))
    dy = dev(det_input((2, 64, T, (H - 1) // 2 + 1, (W - 1) // 2 + 1), 702))
    base = dev(det_input((64, cin, 5, 7, 7), 703))

    def run():
        k = K()
        a = k.conv3d_wgrad(x, dy, (5, 7, 7), (2, 3, 3))
        b = k.conv3d_wgrad(x, dy, (5, 7, 7), (2, 3, 3), out=base.clone(), accumulate=True)
        c = k.conv3d_wgrad(x, dy, (5, 7, 7), (2, 3, 3), out=E(64, cin, 5, 7, 7))
        old = k.C3W_F16
        try:
            k.C3W_F16 = False
            d = k.conv3d_wgrad(x, dy, (5, 7, 7), (2, 3, 3))
        finally:
            k.C3W_F16 = old
        return a, b, c, d

    def ref(res):
        a, b, c, _ = res
        assert torch.equal(a, c)
        close(b, base + a, 4e-6 * float(a.abs().max()), 0, "accumulate")
    return run, ref


_params(_conv3d_wgrad, [(2, 2, 130, 40), (1, 5, 16, 16)], "conv3d-wgrad-{}x{}x{}x{}")


@case("conv3d-wgrad-uint8-T1")
def _conv3d_wgrad_u8():
    g = torch.Generator().manual_seed(705)
    xu = dev(torch.randint(0, 256, (2, 3, 1, 96, 96), generator=g, dtype=torch.uint8))
    dy = dev(det_input((2, 64, 1, 48, 48), 706) * torch.exp(2.0 * det_input((2, 64, 1, 48, 48), 707)))
    return (lambda: K().conv3d_wgrad(xu, dy, (5, 7, 7), (2, 3, 3))), None


def _conv3d_fwd(dtype, cin, hw):
    g = torch.Generator().manual_seed(708 + cin)
    if dtype == torch.uint8:
        x = torch.randint(0, 256, (2, cin, 1, hw, hw), generator=g, dtype=torch.uint8)
    else:
        x = (det_input((2, cin, 1, hw, hw), 708, "uniform", 1.0) - 0.421) / 0.165
    x, w = dev(x), dev(det_input((64, cin, 5, 7, 7), 709) / 50)

    def run():
        y, xmax = K().conv3d_fwd(x, w, return_xmax=True)
        return y, None if xmax is None else xmax.clone()
    return run, None


_params(_conv3d_fwd, [(torch.uint8, 3, 96), (torch.float32, 1, 112)], "conv3d-fwd-{}-{}x{}")


# ---- dilated 64 -> 64 convs (tk.test_dconv_split_fwd_vs_fp64 / _wgrad_vs_fp64 / _wgrad16_vs_fp64 have these rows)

DCONV_SHAPES = [(2, 37, 257, 2), (1, 40, 257, 8), (2, 33, 257, 16)]


def _dconv(N, H, W, dil):
    x = det_input((N, 64, H, W), 1900 + dil + W + H) * torch.exp(4.0 * det_input((N, 64, H, W), 1901 + dil))
    dy = det_input((N, 64, H, W), 1952 + dil + H)
    x, dy, w = dev(x, CL), dev(dy, CL), dev(0.03 * det_input((64, 64, 5, 5), 1902 + dil))
    shape = (N, 64, H, W)

    def run():
        k = K()
        mb, mbd = E(2, dtype=torch.int32), E(2, dtype=torch.int32)        # as layers._DilatedConvFn allocates them
        xq = k.split16(x, mb)
        wq, wq_t = k.dconv_wprep2(w, mb, mbd)
        y = k.dconv_fwd(x, w, dil, split=(xq, mb), wq=wq)
        dyq = k.split16(dy, mbd)
        dx = k.dconv_fwd(dy, w, dil, transposed=True, split=(dyq, mbd), wq=wq_t)
        dw16 = k.dconv_wgrad16((xq, mb[:1]), (dyq, mbd[:1]), shape, dil, bias_grad=True)
        own = k.dconv_fwd(x, w, dil), k.dconv_fwd(dy, w, dil, transposed=True)    # the wrapper's own split and wprep
        return xq, wq, wq_t, y, dyq, dx, dw16, mb, mbd, own, k.dconv_wgrad(x, dy, dil, bias_grad=True)

    def ref(res):
        assert torch.equal(res[3], res[9][0]) and torch.equal(res[5], res[9][1])
    return run, ref


_params(_dconv, DCONV_SHAPES, "dconv-{}x{}x{}-d{}")


# ---- AudioFeatNet conv1 / convf (tk.test_conv1_module_nhwc_vs_torch[3-37-130], tk.test_convf_vs_fp64[3-7-13])

@case("conv1-3x37x130")
def _conv1():
    x, dy = dev(det_input((3, 1, 37, 130), 1860)), dev(det_input((3, 64, 37, 130), 1861), CL)
    w, b = dev(0.2 * det_input((64, 1, 5, 5), 1862)), dev(det_input((64,), 1863))
    return (lambda: (K().conv1_fwd(x, w, b), K().conv1_fwd(x, w), K().conv1_bwd(x, w, dy))), None


@case("convf-3x7x13")
def _convf():
    x = dev(det_input((3, 64, 7, 13), 1880) * torch.exp(det_input((3, 64, 7, 13), 1881)), CL)
    dy = dev(det_input((3, 4, 7, 13), 1882), CL)
    w, b = dev(0.1 * det_input((4, 64, 1, 1), 1883)), dev(det_input((4,), 1884))
    return (lambda: (K().convf_fwd(x, w, b), K().convf_bwd(x, w, dy))), None


# ---- ResNet trunk 3x3 convs (tsc.SHAPES / DGRAD2_SHAPES; (3, 64, 1, 9, 64, 2) is a dgrad2 row only: fp64 there)

def _sconv(N, ci, H, W, co, s):
    x, w = tsc._inputs(N, ci, H, W, co, 2100 + ci + co + H)
    ho, wo = (H - 1) // s + 1, (W - 1) // s + 1
    dy = det_input((N, co, ho, wo), 2253 + co) * torch.exp(2.0 * det_input((N, co, ho, wo), 2254))
    xg, dyg, wg = dev(x, CL), dev(dy, CL), dev(w)
    listed = (N, ci, H, W, co, s) in tsc.SHAPES
    full = K().sconv_ok(xg, co, s)            # False for the dgrad2-only row (rows too narrow for the forward's tile)
    assert full or not listed
    xshape = (N, ci, H, W)

    def run():
        k = K()
        xm, dm = E(1, dtype=torch.int32), E(1, dtype=torch.int32)
        xq, dq = k.split_nhwc(xg, xm), k.split_nhwc(dyg, dm)
        y = k.sconv_fwd((xq, xm), xshape, wg, s) if full else None
        if s == 1:
            dx = k.sconv_fwd((dq, dm), tuple(dy.shape), wg, 1, transposed=True)
        else:
            dx = k.sconv_dgrad2((dq, dm), xshape, wg)
        dw = k.sconv_wgrad((xq, xm), (dq, dm), xshape, co, s) if full else None
        return xq, xm, dq, dm, k.split_q(xg), y, dx, dw

    def ref(res):
        if listed:
            return
        y, dx, dw = res[5:]
        xd, wd, dyd = x.double(), w.double(), dy.double()
        for got, truth, bound, what in (
                (y, F.conv2d(xd, wd, None, s, 1), F.conv2d(xd.abs(), wd.abs(), None, s, 1), "y"),
                (dw, torch.nn.grad.conv2d_weight(xd, wd.shape, dyd, s, 1),
                 torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, dyd.abs(), s, 1), "dw"),
                (dx, torch.nn.grad.conv2d_input(xshape, wd, dyd, s, 1),
                 torch.nn.grad.conv2d_input(xshape, wd.abs(), dyd.abs(), s, 1), "dx")):
            assert got is None or tsc._rel(got, truth, bound) <= 1e-5, what
    return run, ref


_params(_sconv, [(1, 64, 5, 7, 192, 1), (3, 64, 1, 9, 64, 2), (2, 64, 24, 24, 128, 2), (11, 512, 3, 3, 512, 1)],
        "sconv-{}x{}x{}x{}-{}-s{}")


# ---- PReLU (tk.test_prelu_vs_torch / test_prelu_channels_last_vs_torch have these rows)

def _prelu(shape, npar, cl):
    fmt = CL if cl else torch.contiguous_format
    x, dy = dev(det_input(shape, 720), fmt), dev(det_input(shape, 721), fmt)
    a = dev(0.1 + torch.rand(npar, generator=torch.Generator().manual_seed(1)))
    return (lambda: (K().prelu_fwd(x, a), K().prelu_bwd(x, a, dy))), None


_params(_prelu, [((2, 8, 7), 1, False), ((5, 16, 33), 16, False), ((7, 128, 5, 5), 1, True)], "prelu-{}-{}-cl{}")


# ---- max pooling over planes and the (C, P) transpose (tk.test_maxpool3d_planes_vs_torch[(1, 2, 3, 7, 9)],
# tk.test_frames_nhwc_transpose[(3, 5, 7, 9, 11)]; the other shape of each: exact torch reference here)

def _pool(shape):
    x = dev(torch.round(4 * det_input(shape, 750)))
    B, C, T, H, W = shape
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = dev(det_input((B, C, T, ho, wo), 751))
    flat = x.reshape(B, C, T * H * W)

    def run():
        y, idx = K().maxpool_planes_fwd(x, (3, 3), (2, 2), (1, 1))
        return y, idx, K().maxpool_planes_bwd(dy, idx, x.shape, (3, 3), (2, 2), (1, 1)), K().transpose_cp(flat)

    def ref(res):
        y, idx, dx, tr = res
        xr = x.double().reshape(B * C * T, 1, H, W).requires_grad_(True)
        yr = F.max_pool2d(xr, 3, 2, 1)
        yr.backward(dy.double().reshape(yr.shape))
        assert torch.equal(y.double().reshape(yr.shape), yr.detach())
        close(dx.reshape(xr.shape), xr.grad, 1e-6, 1e-6, "dx")
        assert torch.equal(tr, flat.transpose(1, 2).contiguous())
    return run, ref


_params(_pool, [((1, 2, 3, 7, 9),), ((3, 5, 7, 9, 11),)], "pool-transpose-{}")


# ---- BatchNorm -> [+ res] -> act (every tk.BNACT_CASES row through tk.test_bnact_vs_fp64 at mean 30, scale 2; the
# split output at tk.test_bnact_split_output_vs_fp32's two shapes)

def _bnact(i, q_out=False, shape=None):
    if q_out:
        cl, act, res, training = True, "prelu_c", False, True
    else:
        shape, cl, act, res, training = tk.BNACT_CASES[i]
    C = shape[1]
    fmt = CL if cl else torch.contiguous_format
    gen = torch.Generator().manual_seed(11)
    x, dy = dev(2.0 * det_input(shape, 740) + 30.0, fmt), dev(det_input(shape, 742), fmt)
    r = dev(det_input(shape, 741), fmt) if res else None
    gam, bet = dev(0.5 + torch.rand(C, generator=gen)), dev(0.1 * torch.randn(C, generator=gen))
    rm0, rv0 = dev(30.0 + 2.0 * torch.randn(C, generator=gen)), dev(4.0 * (1.0 + torch.rand(C, generator=gen)))
    npar = {"prelu_c": C, "prelu_1": 1}.get(act, 0)
    alpha = dev(0.1 + 0.3 * torch.rand(max(npar, 1), generator=gen)) if npar else None
    code = K().ACT_PRELU if npar else (K().ACT_RELU if act == "relu" else K().ACT_NONE)

    def run():
        k = K()
        rm, rv = rm0.clone(), rv0.clone()
        y, stats = k.bnact_fwd(x, gam, bet, rm, rv, training, 0.1, 1e-5, code, alpha, r, q_out=q_out)
        assert k.is_split_q(y) == q_out
        grads = k.bnact_bwd(x, r, dy, stats, gam, bet, code, alpha, training, q_out=q_out)
        assert k.is_split_q(grads[0]) == q_out
        return y, stats, rm, rv, grads
    return run, None


_params(_bnact, [(i,) for i in range(len(tk.BNACT_CASES))], "bnact-case{}")
_params(_bnact, [(0, True, (4, 64, 24, 24)), (1, True, (2, 128, 9, 11))], "bnact-q_out-{}-{}-{}")


# ---- BatchNorm3d -> act -> pool -> frames (tff.test_forward_bit_equal / test_backward have these shapes)

def _bnpool(shape):
    c = tff._case(shape, "prelu_c", True)

    def run():
        y, idx, stats, rm, rv = tff._fused_fwd(c)
        return y, idx, stats, rm, rv, tff._fused_bwd(c, idx, stats)
    return run, None


_params(_bnpool, [((2, 64, 3, 8, 8),), ((1, 128, 2, 8, 12),)], "bnpool-{}")


# ---- PReLU -> gLN, depthwise conv, and the fused pair (tk.test_prelu_gln_vs_fp64, tk.test_dwconv_vs_fp64,
# tk.test_dwconv_prelu_gln_fused_vs_fp64 have these rows; the planes outputs are held to the fp32 outputs by
# tpg.test_prelu_gln_bwd_planes_output / test_dwconv_gln_planes_output's bar, here at these shapes)

def _decode(sp):
    bits = int(sp.mb.item())
    e = max(-100, min(100, 14 - (((bits >> 23) & 0xFF) - 127))) if bits else 0
    return (sp.hi.double() + sp.lo.double()) * 2.0 ** -e


def _prelu_gln(shape):
    C = shape[1]
    x, dy = dev(1.5 * det_input(shape, 900) + 0.3), dev(det_input(shape, 902))
    a = dev(torch.tensor([0.25]))
    gam = dev(0.5 + torch.rand(C, generator=torch.Generator().manual_seed(3)))
    bet = dev(0.1 * det_input((C,), 901))

    def run():
        y, st = K().prelu_gln_fwd(x, a, gam, bet)
        return y, st, K().prelu_gln_bwd(x, a, gam, st, dy), K().prelu_gln_bwd(x, a, gam, st, dy, planes=True)

    def ref(res):
        _, _, plain, q = res
        sp = K().planes_of(q[0])
        m = float(plain[0].abs().max())
        assert float((_decode(sp) - plain[0].double()).abs().max()) <= 2.0 ** -21 * m
        assert all(torch.equal(u, v) for u, v in zip(plain[1:], q[1:]))
        for pl in (sp.hi, sp.lo):
            assert bool((_full_rows(pl)[..., shape[2]:] == 0).all())
    return run, ref


_params(_prelu_gln, [((3, 8, 1),), ((2, 64, 2049),)], "prelu-gln-{}")


@case("dwconv-2x16x5-P3-d8")
def _dwconv():
    x, w, dy = dev(det_input((2, 16, 5), 910)), dev(det_input((16, 1, 3), 911)), dev(det_input((2, 16, 5), 912))
    return (lambda: (K().dwconv_fwd(x, w, 8), K().dwconv_bwd(x, w, dy, 8))), None


def _dwconv_gln(B, C, Kn, P, dil):
    x, w = dev(det_input((B, C, Kn), 1700 + Kn)), dev(0.5 * det_input((C, 1, P), 1701))
    alpha, gam, bet = dev(torch.tensor([0.2])), dev(1 + 0.1 * det_input((C,), 1702)), dev(0.1 * det_input((C,), 1703))
    dy = dev(det_input((B, C, Kn), 1704))

    def run():
        y, y1, st = K().dwconv_gln_fwd(x, w, dil, alpha, gam, bet)
        q = K().dwconv_gln_fwd(x, w, dil, alpha, gam, bet, planes=True)
        return y, y1, st, q, K().dwconv_gln_bwd(x, w, dil, y1, alpha, gam, st, dy)

    def ref(res):
        y, y1, st, q, _ = res
        sp = K().planes_of(q[0])
        assert torch.equal(y1, q[1]) and torch.equal(st, q[2])
        assert float((_decode(sp) - y.double()).abs().max()) <= 2.0 ** -21 * float(y.abs().max())
        for pl in (sp.hi, sp.lo):
            assert bool((_full_rows(pl)[..., Kn:] == 0).all())
    return run, ref


_params(_dwconv_gln, [(1, 8, 17, 5, 2), (3, 64, 300, 3, 4)], "dwconv-gln-{}x{}x{}-P{}-d{}")


# ---- LSTM recurrence (tk.test_lstm_vs_torch_fp64[(2, 17, 64, 128, True)] with the grouped kernels and without)

def _lstm(grouped):
    B, T, H = 2, 17, 128
    gx, dh = dev(det_input((B, T, 4 * H), 1620)), dev(det_input((B, T, H), 1622))
    w = dev(0.06 * det_input((4 * H, H), 1621))

    def run():
        k = K()
        old = k.LSTM_GROUP
        k.LSTM_GROUP = grouped
        try:
            res = []
            for rev in (False, True):
                both_dirs = E(B, T, 2 * H)                       # the bidirectional layer's strided output halves
                h, c, gates = k.lstm_fwd(gx, w, hout=both_dirs[..., rev * H:(rev + 1) * H], reverse=rev)
                res += [h, c, gates, k.lstm_bwd(dh, gates, c, w, reverse=rev), k.lstm_fwd(gx, w, reverse=rev)]
            with k.no_grouped_lstm():
                res.append(k.lstm_fwd(gx, w))
            k.raise_if_kernel_error()
        finally:
            k.LSTM_GROUP = old
        return res

    def ref(res):
        assert torch.equal(res[0], res[4][0]) and torch.equal(res[5], res[9][0])
    return run, ref


_params(_lstm, [(True,), (False,)], "lstm-2x17x128-grouped-{}")


# ---- projection GEMMs and their helpers (tpg.test_gemm_bf16_edge_shapes / test_gemm_f32s_edge_shapes_and_fold
# [(129, 127, 64)], tpg.test_gemm_f32s_rows_tn_vs_fp64[(385, 5, 40, 24)]; time chunks: fp64 here, the same bar)

@case("gemm-bf16-129x127x64")
def _gemm_bf16():
    g = torch.Generator(device=DEV).manual_seed(129 * 31 + 127)
    P, Q = tpg._operand(2, 129, 64, True, g), tpg._operand(2, 127, 64, False, g, shared=True)

    def run():
        out = E(2, 127, 132, dtype=torch.bfloat16)[..., :129]
        out32 = E(1, 127, 132)[..., :129]
        return K().gemm_bf16(P, Q, out), K().gemm_bf16(P, Q, out32, 0.5, fold=2)

    def ref(res):
        tpg._check(res[0], P, Q, 1.0, 129)
    return run, ref


@case("gemm-f32s-129x127x64")
def _gemm_f32s():
    g = torch.Generator(device=DEV).manual_seed(129 * 37 + 127 + 1)
    P, Q = tpg._operand32(2, 129, 64, True, g), tpg._operand32(2, 127, 64, False, g)

    def run():
        k = K()
        a = k.gemm_f32s(P, Q, E(2, 127, 132)[..., :129])
        ps, qs = k.split_planes(P), k.split_planes(Q)
        b = k.gemm_f32s_split(ps, qs, E(2, 127, 132)[..., :129], 0.5)
        c = k.gemm_f32s(P, Q, E(1, 127, 132)[..., :129], fold=2, ps=ps, qs=qs)
        return a, b, c, ps, qs

    def ref(res):
        assert tpg._check32(res[0], P, Q, 1.0, 129) <= 1e-5 and tpg._check32(res[1], P, Q, 0.5, 129) <= 1e-5
        assert tpg._check32(res[2], P, Q, 1.0, 129, 2) <= 1e-5
    return run, ref


@case("gemm-f32s-rows-tn-385x5x40x24")
def _rows_tn():
    g = torch.Generator(device=DEV).manual_seed(385 + 40)
    a = torch.randn(385, 40, device=DEV, generator=g) * torch.exp(2.0 * torch.randn(385, 40, device=DEV, generator=g))
    b = torch.randn(385, 24, device=DEV, generator=g)
    return (lambda: K().gemm_f32s_rows_tn(K().split_planes(a[None]), K().split_planes(b[None]), 5)), None


@case("gemm-f32s-time-chunks-129x127x61")
def _time_chunks():
    g = torch.Generator(device=DEV).manual_seed(61)
    P = torch.randn(2, 129, 61, device=DEV, generator=g) * torch.exp(2.0 * torch.randn(2, 129, 61, device=DEV, generator=g))
    Q = torch.randn(2, 127, 61, device=DEV, generator=g)

    def run():
        sp, sq = K().split_rows8(P), K().split_rows8(Q)
        return K().gemm_f32s_time_chunks(sp, sq, 0.5), _full_rows(sp.hi), _full_rows(sp.lo), sp.mb

    def ref(res):
        want = 0.5 * torch.einsum("bpt,bqt->qp", P.double(), Q.double())
        mag = 0.5 * torch.einsum("bpt,bqt->qp", P.double().abs(), Q.double().abs())
        assert float(((res[0].double() - want).abs() / mag).max()) <= 1e-5
        assert bool((res[1][..., 61:] == 0).all()) and bool((res[2][..., 61:] == 0).all())
    return run, ref


def _add_split(b, c, l):
    """add_max on padded rows whose pad columns hold NaN, add_max_flat, split_planes, split_rows8
    (tpg.test_add_max_padded_rows has (3, 40, 17) and (1, 8, 4); exact references here)."""
    k = K()
    g = torch.Generator(device=DEV).manual_seed(b * c + l)
    a, bb = (k.bdl_empty(b, c, l, torch.float32, torch.device(DEV)) for _ in range(2))
    fa, fb = (t.as_strided((b, c, t.stride(1)), t.stride()) for t in (a, bb))
    fa.fill_(float("nan"))
    fb.fill_(float("nan"))
    a.copy_(torch.randn(b, c, l, device=DEV, generator=g))
    bb.copy_(3 * torch.randn(b, c, l, device=DEV, generator=g))
    ac, bc = a.contiguous(), bb.contiguous()

    def run():
        y, yf = K().add_max(fa, fb, l), K().add_max_flat(ac, bc)
        s8 = K().split_rows8(ac)
        return y, yf, K().split_planes(y), K().split_planes(ac), K().split_planes(a), s8, _full_rows(s8.hi), \
            _full_rows(s8.lo)

    def ref(res):
        y, yf, sy, sc, sa, s8 = res[:6]
        assert torch.equal(y, a + bb) and torch.equal(yf, a + bb)
        for t in (y, yf):
            assert int(getattr(t, K().ABSMAX_ATTR).item()) == int((a + bb).abs().max().view(torch.int32).item())
        assert torch.equal(sc.hi, s8.hi) and torch.equal(sc.lo, s8.lo) and torch.equal(sc.mb, s8.mb)
        assert torch.equal(sc.hi, sa.hi) and torch.equal(sc.lo, sa.lo) and torch.equal(sc.mb, sa.mb)
        assert float((_decode(sc) - ac.double()).abs().max()) <= 2.0 ** -22 * float(ac.abs().max())
        assert bool((res[6][..., l:] == 0).all()) and bool((res[7][..., l:] == 0).all())
    return run, ref


_params(_add_split, [(3, 40, 17), (1, 8, 4)], "add-max-split-{}x{}x{}")


# ---- autograd level: one forward and backward per module that allocates for itself, all four modules patched.
# References and bars are those of the layers' module tests (named in each case).

def _grads(params, *outs):
    return [t.detach().clone() for t in outs] + [p.grad.detach().clone() for p in params]


def _rel_close(got, want, rel, what):
    err = float((got.detach().double().cpu() - want.detach().double().cpu()).abs().max())
    sc = max(1e-6, float(want.detach().abs().max()))
    assert err <= rel * sc, (what, err, sc)


def _bn_conv_pair(kind):
    """layers: bn_act(q_fwd) -> DilatedConv2d (the paired BatchNorm backward from the conv's rows) / -> TrunkConv2d
    block, as tbn.test_paired_autograd_uses_rows builds them; fp64: BatchNorm -> act -> conv in torch, bars of
    tk.test_dilated_conv2d_module_split_path_vs_torch (2e-5 of the max) and tk.test_bnact_vs_fp64 (1e-4)."""
    from avse_challenge_amd import layers
    torch.manual_seed(3)
    if kind == "dilated":
        shape, act = (2, 64, 6, 257), "relu"
        conv = layers.DilatedConv2d(64, 64, 5, padding=4, dilation=2).to(DEV)
    else:
        shape, act = (5, 64, 6, 6), layers.PReLU(64).to(DEV)
        conv = layers.TrunkConv2d(64, 64).to(DEV)
    bn = torch.nn.BatchNorm2d(64).to(DEV).train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0.0, 0.1)
    x0, gy = dev(det_input(shape, 765), CL), dev(det_input(shape, 766), CL)
    params = [p for p in list(bn.parameters()) + list(conv.parameters()) + ([act.weight] if kind == "trunk" else [])]
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()

    def run():
        for p in params:
            p.grad = None
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
        x = x0.clone(memory_format=torch.preserve_format).requires_grad_(True)
        h = layers.bn_act(x, bn, act, q_fwd=conv.q_ok(x))
        assert K().is_split_q(h)
        y = conv(h)
        y.backward(gy)
        return _grads(params, y, x.grad, bn.running_mean, bn.running_var)

    def ref(res):
        xd = x0.double().cpu().requires_grad_(True)
        ps = [p.detach().double().cpu().requires_grad_(True) for p in params]
        z = F.batch_norm(xd, None, None, ps[0], ps[1], True, 0.1, 1e-5)
        if kind == "dilated":
            y = F.conv2d(torch.relu(z), ps[2], ps[3], 1, 4, 2)
        else:
            y = F.conv2d(F.prelu(z, ps[3]), ps[2], None, 1, 1)
        y.backward(gy.double().cpu())
        _rel_close(res[0], y, 2e-5, "y")
        _rel_close(res[1], xd.grad, 1e-4, "dx")
        for got, p in zip(res[4:], ps):
            _rel_close(got, p.grad, 1e-4, "parameter gradient")
    return run, ref


_params(_bn_conv_pair, [("dilated",), ("trunk",)], "autograd-layers-bn-conv-{}")


@case("autograd-layers-time-conv1d")
def _time_conv():
    """layers.time_conv1d as tpg.test_time_conv1d_split_gemm_backward_vs_fp64 (its 2e-5 bar), two utterances."""
    from avse_challenge_amd.layers import time_conv1d
    torch.manual_seed(5)
    B, T, C, k, dil = 2, 75, 512, 3, 4
    conv = torch.nn.Conv1d(C, C, k, padding=(k - 1) * dil, dilation=dil).double()
    x, gy = torch.randn(B, T, C, dtype=torch.float64), torch.randn(B, T + (k - 1) * dil, C, dtype=torch.float64)
    cg = torch.nn.Conv1d(C, C, k, padding=(k - 1) * dil, dilation=dil).to(DEV)
    cg.load_state_dict({n: v.float() for n, v in conv.state_dict().items()})
    gyg = dev(gy.float())

    def run():
        cg.zero_grad(set_to_none=True)
        xg = dev(x.float()).requires_grad_(True)
        y = time_conv1d(xg, cg)
        (y * gyg).sum().backward()
        return _grads(cg.parameters(), y, xg.grad)

    def ref(res):
        xr = x.clone().requires_grad_(True)
        yr = conv(xr.transpose(1, 2)).transpose(1, 2)
        (yr * gy).sum().backward()
        for got, want, what in zip(res, (yr, xr.grad, conv.weight.grad, conv.bias.grad), ("y", "dx", "dw", "db")):
            _rel_close(got, want, 2e-5, what)
    return run, ref


@case("autograd-avse4-pointwise-k125")
def _pointwise():
    """avse4._PointwiseFn at the visual K = 125 (tpg.test_avse4_pointwise_conv_split_vs_fp64[False-125] has the
    reference at this shape)."""
    from avse_challenge_amd import avse4
    g = torch.Generator(device=DEV).manual_seed(125)
    x0 = torch.randn(3, 256, 125, device=DEV, generator=g)
    w = (0.05 * torch.randn(512, 256, device=DEV, generator=g)).requires_grad_(True)
    dy = torch.randn(3, 512, 125, device=DEV, generator=g)

    def run():
        w.grad = None
        x = x0.clone().requires_grad_(True)
        y = avse4._PointwiseFn.apply(w, x)
        y.backward(dy)
        return _grads([w], y, x.grad)
    return run, None


def _bimamba(bf16):
    """mamba_tasnet: one BiMamba block at (b, d_inner, l) = (2, 64, 129).  fp32 against the fp64 oracle block on the
    same weights with the bars of test_gpu_models.test_bimamba_block_fwd_bwd_golden; bf16 autocast against the fp32 run
    with test_gpu_avmamba.test_avmamba_bf16_autocast_vs_fp32's gradient bar (cosine > 0.95)."""
    from avse_challenge_amd import mamba_tasnet as M
    blk = det_init_(M.Block(32, M.BiMambaV2(32)), 12).to(DEV)
    hs0, res0, gout = (dev(det_input((2, 129, 32), 8100 + i)) for i in range(3))
    params = list(blk.parameters())

    def step(autocast):
        for p in params:
            p.grad = None
        hs, res = hs0.clone().requires_grad_(True), res0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast, cache_enabled=False):
            oh, orr = blk(hs, res)
        (oh.float() * gout).sum().backward()
        return _grads(params, oh, orr, hs.grad, res.grad)

    def ref(out):
        if bf16:
            want = step(False)
            assert all(bool(torch.isfinite(t).all()) for t in out)
            for i, (a, b) in enumerate(zip(out[2:], want[2:])):
                cos = F.cosine_similarity(a.double().reshape(-1), b.double().reshape(-1), 0)
                assert float(cos) > 0.95, (i, float(cos))
            return
        rb = det_init_(mamba_ref.Block(32, mamba_ref.BiMambaV2(32)), 12).double()
        hs, res = hs0.double().cpu().requires_grad_(True), res0.double().cpu().requires_grad_(True)
        oh, orr = rb(hs, res)
        (oh * gout.double().cpu()).sum().backward()
        close(out[0], oh, 2e-5, 1e-5, "hidden")
        close(out[1], orr, 1e-6, 0, "residual")
        close(out[2], hs.grad, 5e-5, 1e-4, "g_hidden")
        close(out[3], res.grad, 5e-5, 1e-4, "g_residual")
        rp = dict(rb.named_parameters())
        for (name, _), got in zip(blk.named_parameters(), out[4:]):
            r = rp[name].grad
            close(got, r, 1e-4 * max(1.0, float(r.abs().max())), 1e-4, name)
    return (lambda: step(bf16)), ref


_params(_bimamba, [(False,), (True,)], "autograd-mamba-bimamba-2x64x129-bf16-{}")


# ------------------------------------------------------------------ the tests

def test_poison_reaches_gpu_allocations(monkeypatch):
    """The helper on the device: every byte of a poisoned GPU allocation (pads included) holds the pattern, and the
    comparison notices a single poisoned or differing element."""
    k = K()
    with _dirty.dirty(monkeypatch):
        v = k.bdl_empty(2, 3, 250, torch.float32, torch.device(DEV))
        assert v.is_cuda and v.stride(1) == 256 and bool(torch.isnan(_full_rows(v)).all())
        assert int(k.torch.empty(1, device=DEV, dtype=torch.int32).item()) == 0x7FC07FC0
        assert k.torch.empty(3, device=DEV, dtype=torch.uint8).tolist() == [0xC0, 0x7F, 0xC0]
        x = torch.zeros(2, 8, 3, 5, device=DEV).contiguous(memory_format=CL)
        y = k.torch.empty_like(x)
        assert y.stride() == x.stride() and bool(torch.isnan(y).all())
        assert bool(torch.isnan(k.torch.empty(7, device=DEV, dtype=torch.bfloat16)).all())
    assert k.torch is torch and not bool(torch.isnan(torch.zeros(3, device=DEV)).any())
    a = torch.ones(4, device=DEV)
    for bad in (float("nan"), 1.0 + 2.0 ** -23):
        b = a.clone()
        b[2] = bad
        with pytest.raises(AssertionError):
            assert_same([a], [b])
    assert_same([a, None], [a.clone(), None])


@pytest.mark.parametrize("name", list(CASES))
def test_dirty_run_equals_clean_run(name, monkeypatch):
    """One family at one shape: clean run (held to its reference), dirty run, NaN-free and bit-equal."""
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    run, ref = CASES[name]()
    clean, dirty = _dirty.both(run, monkeypatch)
    if ref is not None:
        ref(clean)
    assert_same(clean, dirty)


REPLAYS = [
    ("scan", lambda mp: tk.test_scan_edges_vs_oracle(3, 130, 129, "full")),
    ("scan-l1", lambda mp: tk.test_scan_edges_vs_oracle(1, 64, 1, "full")),
    ("dtproj", lambda mp: tk.test_dtproj_vs_fp64(2, 130, 64, 257, torch.bfloat16)),
    ("cconv", lambda mp: tk.test_cconv_vs_oracle(1, 5, 257, 4, True)),
    ("cconv-bf16", lambda mp: tk.test_cconv_bf16_vs_oracle(2, 33, 250, True)),
    ("step-ops", lambda mp: tst.test_step_ops_vs_oracle(3, 70, torch.bfloat16)),
    ("rmsnorm", lambda mp: tk.test_add_rmsnorm_vs_oracle(32, True)),
    ("stft", lambda mp: tk.test_stft_vs_oracle(1000)),
    ("conv3d-wgrad", lambda mp: tk.test_conv3d_wgrad_vs_fp64(2, 2, 130, 40)),
    ("conv3d-wgrad-u8", lambda mp: tk.test_conv3d_wgrad_uint8_vs_fp64(1)),
    ("conv3d-fwd", lambda mp: tk.test_conv3d_fwd_vs_fp64(torch.float32, 1, 1, 112)),
    ("dconv-fwd", lambda mp: tk.test_dconv_split_fwd_vs_fp64(2, 33, 257, 16, False)),
    ("dconv-dgrad", lambda mp: tk.test_dconv_split_fwd_vs_fp64(1, 40, 257, 8, True)),
    ("dconv-wgrad", lambda mp: tk.test_dconv_wgrad_vs_fp64(2, 37, 257, 2)),
    ("dconv-wgrad16", lambda mp: tk.test_dconv_wgrad16_vs_fp64(2, 37, 257, 2)),
    ("conv1", lambda mp: tk.test_conv1_module_nhwc_vs_torch(3, 37, 130)),
    ("convf", lambda mp: tk.test_convf_vs_fp64(3, 7, 13)),
    ("sconv-fwd", lambda mp: tsc.test_sconv_fwd_vs_fp64(1, 64, 5, 7, 192, 1)),
    ("sconv-dgrad2", lambda mp: tsc.test_sconv_dgrad2_vs_fp64(3, 64, 1, 9, 64, 2)),
    ("sconv-wgrad", lambda mp: tsc.test_sconv_wgrad_vs_fp64(11, 512, 3, 3, 512, 1)),
    ("prelu", lambda mp: tk.test_prelu_vs_torch((5, 16, 33), 16)),
    ("prelu-cl", lambda mp: tk.test_prelu_channels_last_vs_torch((7, 128, 5, 5), 1)),
    ("maxpool", lambda mp: tk.test_maxpool3d_planes_vs_torch((1, 2, 3, 7, 9), 3, 2, 1)),
    ("frames", lambda mp: tk.test_frames_nhwc_transpose((3, 5, 7, 9, 11))),
    ("bnact-q", lambda mp: tk.test_bnact_split_output_vs_fp32((2, 128, 9, 11), 30.0, 0.02, "prelu_c")),
    ("bnpool", lambda mp: tff.test_backward((1, 128, 2, 8, 12), "prelu_c", True, mp)),
    ("dgrad-bn-rows", lambda mp: tbn.test_dilated_dgrad_bn_rows(2, 0.0, 1.0, True, mp)),
    ("prelu-gln", lambda mp: tk.test_prelu_gln_vs_fp64((2, 64, 2049))),
    ("dwconv", lambda mp: tk.test_dwconv_vs_fp64(2, 16, 5, 3, 8)),
    ("dwconv-gln", lambda mp: tk.test_dwconv_prelu_gln_fused_vs_fp64(1, 8, 17, 5, 2)),
    ("lstm-grouped", lambda mp: tk.test_lstm_vs_torch_fp64(2, 17, 64, 128, True, "1", mp)),
    ("lstm-plain", lambda mp: tk.test_lstm_vs_torch_fp64(2, 17, 64, 128, True, "0", mp)),
    ("gemm-bf16", lambda mp: tpg.test_gemm_bf16_edge_shapes(129, 127, 64)),
    ("gemm-f32s", lambda mp: tpg.test_gemm_f32s_edge_shapes_and_fold(129, 127, 64, 1)),
    ("rows-tn", lambda mp: tpg.test_gemm_f32s_rows_tn_vs_fp64(77 * 5, 5, 40, 24)),
    ("add-max", lambda mp: tpg.test_add_max_padded_rows(3, 40, 17)),
    ("split-rows8", lambda mp: tpg.test_split_rows8_planes(3, 16, 17)),
    ("pointwise-k125", lambda mp: tpg.test_avse4_pointwise_conv_split_vs_fp64(125, False)),
    ("dilated-module", lambda mp: tk.test_dilated_conv2d_module_split_path_vs_torch()),
    ("trunk-module", lambda mp: tk.test_trunk_conv2d_module_grads_vs_torch()),
]
REPLAYS += [(f"bnact-case{i}", lambda mp, c=c: tk.test_bnact_vs_fp64(*c, 30.0, 2.0)) for i, c in enumerate(tk.BNACT_CASES)]


@pytest.mark.parametrize("name", [n for n, _ in REPLAYS])
def test_replay_under_dirty_memory(name, monkeypatch):
    """The existing fp64 / oracle test of the family, at the dirty-memory shape, run again on poisoned memory: the
    dirty run itself holds the reference's bar."""
    fn = dict(REPLAYS)[name]
    with _dirty.dirty(monkeypatch):
        fn(monkeypatch)
