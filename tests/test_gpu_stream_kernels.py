"""Streaming kernels vs the fp64 oracle: avse_scan_fwd_state, avse_cconv_fwd_state[_bf16], avse_cconv_update,
avse_ssm_step.

The expected values come from the oracle (oracle/mamba_ref.py, fp64) run ONCE over the whole sequence: outputs are
sliced per chunk, states are the oracle's last state over each prefix.  The bars are those of the existing tests of
the same kernels (test_gpu_kernels.py): scan fp32 1e-4 / 1e-4 (test_scan_edges_vs_oracle), scan bf16
|d| / (|ref| + 1e-2) <= 2 * 2^-8 + 1e-6 against fp64 on the bf16 values (test_scan_fwd_golden_bf16), conv fp32
1e-5 / 1e-5 and bf16 1e-5 + 2^-8 relative (test_cconv_vs_oracle, test_cconv_bf16_vs_oracle).  The carried SSM state is
fp32 whatever the activation dtype and is held to the fp32 bar; conv states are copies of inputs and must be equal
bit for bit.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mamba_ref
from oracle.det_init import det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16_REL = 2 * 2 ** -8 + 1e-6


def K():
    from avse_challenge_amd import kernels
    return kernels


def close(a, b, atol, rtol=0.0, what=""):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    np.testing.assert_allclose(a, b, atol=atol, rtol=rtol, err_msg=what)


def bf16_rel(got, ref, what=""):
    rel = (got.detach().double().cpu() - ref.double()).abs() / (ref.double().abs() + 1e-2)
    assert float(rel.max()) <= BF16_REL, (what, float(rel.max()))


def _q(t, dtype):
    """the values the kernel sees, as fp64 (bf16: rounded first)"""
    return None if t is None else t.to(dtype).double()


# ------------------------------------------------------------------ scan with carried state

SCAN_B, SCAN_D, SCAN_L = 2, 96, 200          # d = 96: a partial 64-channel block, two blocks per row
SCAN_SPLITS = [1, 63, 64, 65, 7]             # l = 1, one short of a chunk, a chunk, one over, a short tail


@functools.lru_cache(maxsize=None)
def _scan_case(flags, dtype):
    b, d, l = SCAN_B, SCAN_D, SCAN_L
    seed = 4000
    act = dict(u=det_input((b, d, l), seed), delta=0.5 * det_input((b, d, l), seed + 1),
               B=det_input((b, 1, 16, l), seed + 3), C=det_input((b, 1, 16, l), seed + 4),
               z=det_input((b, d, l), seed + 6) if flags == "full" else None)
    par = dict(A=-torch.exp(0.5 * det_input((d, 16), seed + 2)),
               D=det_input((d,), seed + 5) if flags != "bare" else None,
               delta_bias=0.3 * det_input((d,), seed + 7) if flags != "bare" else None)
    sp = flags != "bare"
    if not sp:
        act["delta"] = act["delta"].abs()
    act = {k: (None if v is None else v.to(dtype)) for k, v in act.items()}
    ref_in = {**{k: _q(v, dtype) for k, v in act.items()}, **{k: _q(v, torch.float32) for k, v in par.items()}}
    ref = mamba_ref.selective_scan(**ref_in, delta_softplus=sp, acc_dtype=torch.float64)
    states, t = [], 0
    for c in SCAN_SPLITS:                    # the oracle's last state over each prefix
        t += c
        pre = {k: (v[..., :t] if (v is not None and k in act) else v) for k, v in ref_in.items()}
        states.append(mamba_ref.selective_scan(**pre, delta_softplus=sp, return_last_state=True,
                                               acc_dtype=torch.float64)[1])
    gpu = {k: (None if v is None else v.to(DEV)) for k, v in {**act, **par}.items()}
    return gpu, sp, ref, states


def _run_chunks(gpu, sp, inplace, checkpoints):
    """the sequence pushed through selective_scan_fwd chunk by chunk -> (per-chunk outputs, per-chunk states)"""
    b, d = SCAN_B, SCAN_D
    state = torch.zeros(b, d, 16, device=DEV)
    outs, states, t = [], [], 0
    for i, c in enumerate(SCAN_SPLITS):
        sl = {k: (v[..., t:t + c] if (v is not None and k in ("u", "delta", "B", "C", "z")) else v)
              for k, v in gpu.items()}
        h0 = None if i == 0 else state
        dst = state if inplace else torch.full((b, d, 16), float("nan"), device=DEV)
        out, x, out_z, last = K().selective_scan_fwd(**sl, delta_softplus=sp, initial_state=h0, return_last_state=dst,
                                                     checkpoints=checkpoints)
        assert last is dst and (x is None) == (not checkpoints)
        state = last
        outs.append((out_z if sl["z"] is not None else out).clone())
        states.append(state.clone())
        t += c
    return outs, states


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("flags", ["full", "noz", "bare"])
def test_scan_state_chunks_vs_oracle(flags, dtype):
    gpu, sp, ref, ref_states = _scan_case(flags, dtype)
    outs, states = _run_chunks(gpu, sp, inplace=True, checkpoints=False)
    got = torch.cat(outs, -1)
    assert got.dtype == dtype and got.shape == ref.shape
    if dtype == torch.float32:
        close(got, ref, 1e-4, 1e-4, "out")
    else:
        bf16_rel(got, ref, "out")
    for i, (s, r) in enumerate(zip(states, ref_states)):
        assert s.dtype == torch.float32
        close(s, r, 1e-4, 1e-4, f"state after chunk {i}")
    # out-of-place states, checkpoints written, and a rerun: all bit for bit the same
    for inplace, ck in ((False, False), (True, True), (True, False)):
        outs2, states2 = _run_chunks(gpu, sp, inplace=inplace, checkpoints=ck)
        for a, b_ in zip(outs + states, outs2 + states2):
            assert torch.equal(a, b_), (inplace, ck)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("flags", ["full", "noz", "bare"])
def test_scan_state_unsplit_equals_stateless(flags, dtype):
    gpu, sp, _, _ = _scan_case(flags, dtype)
    out0, x0, oz0 = K().selective_scan_fwd(**gpu, delta_softplus=sp)
    out1, x1, oz1, last = K().selective_scan_fwd(**gpu, delta_softplus=sp, return_last_state=True)
    assert torch.equal(out0, out1) and torch.equal(x0, x1)
    assert (oz0 is None and oz1 is None) or torch.equal(oz0, oz1)
    assert torch.equal(last, x0[..., -1, 1::2])
    # zero initial state given explicitly: the same bits again
    out2, _, oz2, last2 = K().selective_scan_fwd(**gpu, delta_softplus=sp, initial_state=torch.zeros_like(last),
                                                 return_last_state=True, checkpoints=False)
    assert torch.equal(out0, out2) and torch.equal(last, last2)


def test_scan_state_argument_checks():
    gpu, sp, _, _ = _scan_case("full", torch.float32)
    with pytest.raises(RuntimeError):
        K().selective_scan_fwd(**gpu, delta_softplus=sp, reverse=True, return_last_state=True)
    with pytest.raises(RuntimeError):
        K().selective_scan_fwd(**gpu, delta_softplus=sp, initial_state=torch.zeros(SCAN_B, SCAN_D, 8, device=DEV))
    with pytest.raises(RuntimeError):
        K().selective_scan_fwd(**gpu, delta_softplus=sp,
                               initial_state=torch.zeros(SCAN_B, SCAN_D, 16, device=DEV, dtype=torch.bfloat16))


# ------------------------------------------------------------------ causal conv with carried left context

CC_B, CC_D = 2, 33
CC_SPLITS = [1, 2, 1, 5, 256, 257, 2100]     # l < w - 1, both sides of the short-path limit, more than one 2048 tile
CC_L = sum(CC_SPLITS)


@functools.lru_cache(maxsize=None)
def _cc_case(w, silu, dtype):
    x = det_input((CC_B, CC_D, CC_L), 5300 + w).to(dtype)
    wt, bias = det_input((CC_D, w), 5301), det_input((CC_D,), 5302)
    ref = mamba_ref.causal_conv1d(x.double(), wt.double(), bias.double(), silu)
    return x.to(DEV), wt.to(DEV), bias.to(DEV), ref


def _cc_fwd_state(x, wt, bias, silu, state_in, state_out):
    """avse_cconv_fwd_state through the C ABI with separate input / output states (kernels.causal_conv1d_fwd only
    updates in place)"""
    from avse_challenge_amd import _lib
    L = _lib.lib()
    b, d, l = x.shape
    out = K().bdl_empty(b, d, l, x.dtype, x.device)
    fn = L.avse_cconv_fwd_state if x.dtype == torch.float32 else L.avse_cconv_fwd_state_bf16
    _lib.check(fn(b, d, l, wt.shape[1], _lib.ptr(x), x.stride(0), x.stride(1), _lib.ptr(wt), _lib.ptr(bias),
                  _lib.ptr(out), out.stride(0), out.stride(1), int(silu), _lib.ptr(state_in), _lib.ptr(state_out),
                  state_out.stride(0), state_out.stride(1), _lib.stream_ptr(x.device)), "avse_cconv_fwd_state")
    return out


@pytest.mark.parametrize("layout", ["view", "padded"])     # > 256 frames: the tiled path / the vector path
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("w", [2, 3, 4])
def test_cconv_state_chunks_vs_oracle(w, silu, dtype, layout):
    x, wt, bias, ref = _cc_case(w, silu, dtype)
    state = torch.zeros(CC_B, CC_D, w, device=DEV, dtype=dtype)
    state2 = state.clone()
    padded = torch.cat([torch.zeros(CC_B, CC_D, w, device=DEV, dtype=dtype), x], -1)
    t = 0
    for c in CC_SPLITS:
        xc = x[..., t:t + c]
        if layout == "padded":
            buf = K().bdl_empty(CC_B, CC_D, c, dtype, DEV)
            buf.copy_(xc)
            xc = buf
        out = K().causal_conv1d_fwd(xc, wt, bias, silu, conv_state=state)
        assert out.dtype == dtype
        if dtype == torch.float32:
            close(out, ref[..., t:t + c], 1e-5, 1e-5, f"out at {t}")
        else:
            close(out.float(), ref[..., t:t + c], 1e-5, 2 ** -8, f"out at {t}")
        t += c
        assert torch.equal(state, padded[..., t:t + w]), f"state after {t} frames"     # the last w inputs, exactly
        # out of place: a fresh output state from a read-only input state, bit for bit the in-place result
        nxt = torch.full_like(state2, float("nan"))
        out2 = _cc_fwd_state(xc, wt, bias, silu, state2, nxt)
        assert torch.equal(out, out2) and torch.equal(nxt, state)
        state2 = nxt


def test_cconv_state_none_is_zero_context():
    x, wt, bias, _ = _cc_case(4, True, torch.float32)
    for l in (3, 300, 2622):
        xs = x[..., :l].contiguous()
        a = K().causal_conv1d_fwd(xs, wt, bias, True)
        nxt = torch.empty(CC_B, CC_D, 4, device=DEV)
        b_ = _cc_fwd_state(xs, wt, bias, True, None, nxt)
        close(b_, a, 1e-6, 1e-6, f"l = {l}")
        assert torch.equal(nxt, F.pad(xs, (4, 0))[..., -4:])


# ------------------------------------------------------------------ single-frame updates

def _silu64(t):
    return t * torch.sigmoid(t)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", [64, 70])
@pytest.mark.parametrize("b", [1, 3])
def test_step_ops_vs_oracle(b, d, dtype):
    """20 consecutive steps from a non-zero state against the fp64 recurrence of bimamba.py:328-358, and the same 20
    frames as one avse_scan_fwd_state call: both held to the oracle (not to each other)."""
    steps, w, seed = 20, 4, 7000 + 10 * b + d
    xs = det_input((steps, b, d), seed).to(dtype)
    zs = det_input((steps, b, d), seed + 1).to(dtype)
    dts = (0.5 * det_input((steps, b, d), seed + 2)).to(dtype)
    Bs, Cs = det_input((steps, b, 16), seed + 3).to(dtype), det_input((steps, b, 16), seed + 4).to(dtype)
    A = -torch.exp(0.5 * det_input((d, 16), seed + 5))
    D, dt_bias = det_input((d,), seed + 6), 0.3 * det_input((d,), seed + 7)
    wt, cb = det_input((d, w), seed + 8), det_input((d,), seed + 9)
    conv0 = det_input((b, d, w), seed + 10).to(dtype)
    ssm0 = det_input((b, d, 16), seed + 11)

    # fp64 reference: the reference's fallback, statement for statement
    conv_r, ssm_r = conv0.double(), ssm0.double()
    ref_conv_out, ref_y = [], []
    for t in range(steps):
        conv_r = torch.roll(conv_r, shifts=-1, dims=-1)
        conv_r[:, :, -1] = xs[t].double()
        ref_conv_out.append(_silu64(torch.sum(conv_r * wt.double(), dim=-1) + cb.double()))
        x, dt = xs[t].double(), F.softplus(dts[t].double() + dt_bias.double())
        dA = torch.exp(torch.einsum("bd,dn->bdn", dt, A.double()))
        dB = torch.einsum("bd,bn->bdn", dt, Bs[t].double())
        ssm_r = ssm_r * dA + x[:, :, None] * dB
        y = torch.einsum("bdn,bn->bd", ssm_r, Cs[t].double()) + D.double() * x
        ref_y.append(y * _silu64(zs[t].double()))

    g = lambda t: t.to(DEV)      # noqa: E731
    conv_s, ssm_s = g(conv0).clone(), g(ssm0).clone()
    for t in range(steps):
        co = K().causal_conv1d_update(g(xs[t]), conv_s, g(wt), g(cb), silu=True)
        y = K().selective_state_update(ssm_s, g(xs[t]), g(dts[t]), g(A), g(Bs[t]), g(Cs[t]), g(D), g(zs[t]),
                                       g(dt_bias), True)
        assert co.dtype == dtype and y.dtype == dtype and co.shape == y.shape == (b, d)
        if dtype == torch.float32:
            close(co, ref_conv_out[t], 1e-5, 1e-5, f"conv step {t}")
            close(y, ref_y[t], 1e-4, 1e-4, f"ssm step {t}")
        else:
            close(co.float(), ref_conv_out[t], 1e-5, 2 ** -8, f"conv step {t}")
            bf16_rel(y, ref_y[t], f"ssm step {t}")
    assert torch.equal(conv_s, g(conv_r.to(dtype)))
    close(ssm_s, ssm_r, 1e-4, 1e-4, "ssm state after the steps")

    # the same frames as one chunk through the carried-state scan
    tm = lambda t: g(t.permute(1, 2, 0).contiguous())      # noqa: E731  (steps, b, c) -> (b, c, steps)
    ssm_c = g(ssm0).clone()
    _, _, out_z, last = K().selective_scan_fwd(tm(xs), tm(dts), g(A), tm(Bs), tm(Cs), g(D), tm(zs), g(dt_bias), True,
                                               initial_state=ssm_c, return_last_state=ssm_c, checkpoints=False)
    ref_seq = torch.stack(ref_y, -1)
    if dtype == torch.float32:
        close(out_z, ref_seq, 1e-4, 1e-4, "chunk out")
    else:
        bf16_rel(out_z, ref_seq, "chunk out")
    close(last, ssm_r, 1e-4, 1e-4, "chunk state")
    # without gate, skip and bias; dt taken as given
    s1 = g(ssm0).clone()
    y1 = K().selective_state_update(s1, g(xs[0]), g(dts[0]).abs(), g(A), g(Bs[0]), g(Cs[0]))
    dt = dts[0].double().abs()
    s_ref = ssm0.double() * torch.exp(dt[:, :, None] * A.double()) + (dt * xs[0].double())[:, :, None] * Bs[0].double()[:, None]
    y_ref = torch.einsum("bdn,bn->bd", s_ref, Cs[0].double())
    close(s1, s_ref, 1e-4, 1e-4, "bare state")
    if dtype == torch.float32:
        close(y1, y_ref, 1e-4, 1e-4, "bare out")
    else:
        bf16_rel(y1, y_ref, "bare out")
