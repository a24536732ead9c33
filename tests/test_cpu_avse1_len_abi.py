"""Length-aware entry points of the avse1 ragged path (avse_stft_fwd_len, avse_istft_len, avse_bnact_fwd_len,
avse_bnact_fwd_q_len, avse_gather_nearest_len): declared, bound, and validating on the host before any launch.  No
GPU: every call below must return before a kernel is enqueued."""
import ctypes
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIB = os.path.join(REPO, "avse_challenge_amd", "libavse_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libavse_hip.so not built")
D = ctypes.c_void_p(64)              # non-null, 16-B aligned, never dereferenced on the host
NAMES = ("avse_stft_fwd_len", "avse_istft_len", "avse_bnact_fwd_len", "avse_bnact_fwd_q_len",
         "avse_gather_nearest_len")


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
def test_stft_and_istft_validate_on_the_host():
    from avse_challenge_amd import _lib
    L = _lib.lib()
    f = L.avse_stft_fwd_len                                  # batch T wave lengths mag spec stream
    assert f(3, 1151, D, None, D, D, None) == -1
    assert f(3, 1151, None, D, D, D, None) == -1
    assert f(3, 1151, D, D, None, D, None) == -1
    assert f(0, 1151, D, D, D, None, None) == -2
    assert f(3, 256, D, D, D, None, None) == -2              # no room for the reflect pad
    assert f(1 << 20, 1 << 20, D, D, D, None, None) == -2
    g = L.avse_istft_len                                     # batch frames length mag phase lengths fbuf out stream
    assert g(3, 9, 1151, D, D, None, D, D, None) == -1
    assert g(3, 9, 1151, None, D, D, D, D, None) == -1
    assert g(3, 9, 1151, D, D, D, None, D, None) == -1
    assert g(3, 9, 1151, D, D, D, D, None, None) == -1
    assert g(3, 0, 1151, D, D, D, D, D, None) == -2
    assert g(3, 9, 0, D, D, D, D, D, None) == -2
    assert g(0, 9, 1151, D, D, D, D, D, None) == -2


def _bn(fn, N=3 * 9 * 5, C=64, S=1, x=D, act=1, alpha=None, alpha_n=0, training=0, rm=D, rv=D, stats=D, y=D, ymax=D,
        lengths=D, B=3, T=9, inner=5, t_off=0, rows=1):
    # N C S x gamma beta act alpha alpha_n training eps rm rv stats y ymax lengths B T inner t_off time_in_rows stream
    return fn(N, C, S, x, D, D, act, alpha, alpha_n, training, 1e-5, rm, rv, stats, y, ymax, lengths, B, T, inner,
              t_off, rows, None)


@needs_lib
def test_bnact_len_validates_on_the_host():
    from avse_challenge_amd import _lib
    L = _lib.lib()
    for fn in (L.avse_bnact_fwd_len, L.avse_bnact_fwd_q_len):
        assert _bn(fn, lengths=None) == -1
        assert _bn(fn, x=None) == -1
        assert _bn(fn, y=None) == -1
        assert _bn(fn, rm=None) == -1                        # eval mode needs the running statistics
        assert _bn(fn, training=1) == -1                     # training mode is refused
        assert _bn(fn, act=2) == -1                          # PReLU without its slopes
        assert _bn(fn, act=2, alpha=D, alpha_n=3) == -2
        assert _bn(fn, act=3) == -2
        assert _bn(fn, N=3 * 9 * 5 + 1) == -2                # rows do not factor into B T inner
        assert _bn(fn, t_off=9) == -2
        assert _bn(fn, B=0) == -2
    f, q = L.avse_bnact_fwd_len, L.avse_bnact_fwd_q_len
    assert _bn(f, N=3, S=45, rows=0, ymax=None, lengths=None) == -1
    assert _bn(f, N=3, S=44, rows=0) == -2                   # columns do not factor into T inner
    assert _bn(f, N=4, S=45, rows=0) == -2                   # one row per sample in the column form
    assert _bn(q, ymax=None) == -1                           # the split output needs its max word
    assert _bn(q, C=32) == -2                                # C % 64
    assert _bn(q, N=3, S=45, rows=0) == -2                   # channels-last only
    assert _bn(q, y=ctypes.c_void_p(72)) == -2               # unaligned: no 4-vector form


@needs_lib
def test_gather_validates_on_the_host():
    from avse_challenge_amd import _lib
    u = _lib.lib().avse_gather_nearest_len                   # B C n_in T v v_bs v_ts vlen tlen out o_bs o_ts stream
    assert u(3, 512, 25, 126, None, 25 * 512, 512, D, D, D, 126 * 1540, 1540, None) == -1
    assert u(3, 512, 25, 126, D, 25 * 512, 512, None, D, D, 126 * 1540, 1540, None) == -1
    assert u(3, 512, 25, 126, D, 25 * 512, 512, D, None, D, 126 * 1540, 1540, None) == -1
    assert u(3, 512, 25, 126, D, 25 * 512, 512, D, D, None, 126 * 1540, 1540, None) == -1
    assert u(3, 512, 0, 126, D, 25 * 512, 512, D, D, D, 126 * 1540, 1540, None) == -2
    assert u(3, 0, 25, 126, D, 25 * 512, 512, D, D, D, 126 * 1540, 1540, None) == -2
    assert u(3, 512, 25, 126, D, 25 * 512, 511, D, D, D, 126 * 1540, 1540, None) == -2      # input rows overlap
    assert u(3, 512, 25, 126, D, 24 * 512, 512, D, D, D, 126 * 1540, 1540, None) == -2      # input samples overlap
    assert u(3, 512, 25, 126, D, 25 * 512, 512, D, D, D, 126 * 1540, 511, None) == -2       # output rows overlap
    assert u(3, 512, 25, 126, D, 25 * 512, 512, D, D, D, 125 * 1540, 1540, None) == -2      # output samples overlap
