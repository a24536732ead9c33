"""Length-aware entry points of the Mamba kernels (avse_scan_fwd_len, avse_cconv_fwd_len, avse_cconv_fwd_len_bf16):
declared, bound, and validating on the host before any launch.  No GPU: every call below must return before a kernel is
enqueued."""
import ctypes
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIB = os.path.join(REPO, "avse_challenge_amd", "libavse_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libavse_hip.so not built")
D = ctypes.c_void_p(64)              # non-null, 16-B aligned, never dereferenced on the host
NAMES = ("avse_scan_fwd_len", "avse_cconv_fwd_len", "avse_cconv_fwd_len_bf16")


def scan_args(**over):
    """avse_scan_fwd_args of a valid z-gated fp32 call on dummy pointers; over: fields to change."""
    from avse_challenge_amd import _lib
    a = _lib.ScanFwdArgs()
    a.batch, a.dim, a.seqlen, a.dstate = 2, 80, 300, 16
    a.in_dtype, a.delta_softplus, a.reverse = _lib.AVSE_F32, 1, 0
    for name in ("u", "delta", "A", "B", "C", "z", "out_z"):
        setattr(a, name, 64)
    for name in ("u", "delta", "z", "out_z"):
        setattr(a, name + "_bs", 80 * 300)
        setattr(a, name + "_ds", 300)
    a.B_bs = a.C_bs = 16 * 300
    a.B_ns = a.C_ns = 300
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_entry_points_are_declared_and_bound():
    from avse_challenge_amd import _lib
    hdr = open(os.path.join(REPO, "include", "avse_hip.h")).read()
    for name in NAMES:
        assert name + "(" in hdr, name
        assert name in _lib.SIGNATURES, name


@needs_lib
def test_abi_version_is_unchanged():
    from avse_challenge_amd import _lib
    L = _lib.lib()                                           # binds every symbol of SIGNATURES, the new ones included
    assert L.avse_abi_version() == 2
    for name in NAMES:
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]


@needs_lib
def test_scan_validates_on_the_host():
    from avse_challenge_amd import _lib
    f = _lib.lib().avse_scan_fwd_len                         # args, lengths, stream
    assert f(scan_args(), None, None) == -1                  # null lengths
    assert f(None, D, None) == -1
    for name in ("u", "delta", "A", "B", "C", "out_z"):      # a null required pointer (x is not one: never written)
        assert f(scan_args(**{name: None}), D, None) == -1, name
    assert f(scan_args(z=None, out_z=None), D, None) == -1   # no z: out is the required output
    for name in ("batch", "dim", "seqlen"):
        assert f(scan_args(**{name: 0}), D, None) == -2, name
    assert f(scan_args(dstate=8), D, None) == -2
    assert f(scan_args(in_dtype=7), D, None) == -3
    assert f(scan_args(delta_softplus=3), D, None) == -1


@needs_lib
def test_conv_validates_on_the_host():
    from avse_challenge_amd import _lib
    L = _lib.lib()
    for f in (L.avse_cconv_fwd_len, L.avse_cconv_fwd_len_bf16):
        # batch dim seqlen width x x_bs x_ds lengths weight bias out out_bs out_ds silu reverse stream
        assert f(2, 8, 300, 4, D, 2400, 300, None, D, D, D, 2400, 300, 1, 0, None) == -1
        assert f(2, 8, 300, 4, None, 2400, 300, D, D, D, D, 2400, 300, 1, 0, None) == -1
        assert f(2, 8, 300, 4, D, 2400, 300, D, None, D, D, 2400, 300, 1, 0, None) == -1
        assert f(2, 8, 300, 4, D, 2400, 300, D, D, D, None, 2400, 300, 1, 0, None) == -1
        assert f(0, 8, 300, 4, D, 2400, 300, D, D, D, D, 2400, 300, 1, 0, None) == -2
        assert f(2, 0, 300, 4, D, 2400, 300, D, D, D, D, 2400, 300, 1, 0, None) == -2
        assert f(2, 8, 0, 4, D, 2400, 300, D, D, D, D, 2400, 300, 1, 0, None) == -2
        assert f(2, 8, 300, 5, D, 2400, 300, D, D, D, D, 2400, 300, 1, 0, None) == -2
        assert f(2, 8, 300, 0, D, 2400, 300, D, D, D, D, 2400, 300, 1, 0, None) == -2
