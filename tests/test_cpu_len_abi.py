"""Length-aware entry points of the C ABI (avse_*_fwd_len, avse_upsample_linear_len): declared, bound, and validating
on the host before any launch.  No GPU: every call below must return before a kernel is enqueued."""
import ctypes
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIB = os.path.join(REPO, "avse_challenge_amd", "libavse_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libavse_hip.so not built")
D = ctypes.c_void_p(64)              # non-null, 16-B aligned, never dereferenced on the host
NAMES = ("avse_prelu_gln_fwd_len", "avse_dwconv_gln_fwd_len", "avse_dwconv_gln_fwd_q_len", "avse_dwconv_fwd_len",
         "avse_upsample_linear_len")


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
def test_gln_forwards_validate_on_the_host():
    from avse_challenge_amd import _lib
    L = _lib.lib()
    f = L.avse_prelu_gln_fwd_len                             # B C K x len alpha gamma beta eps y stats ws stream
    assert f(2, 8, 100, D, None, D, D, D, 1e-8, D, D, D, None) == -1
    assert f(2, 8, 100, None, D, D, D, D, 1e-8, D, D, D, None) == -1
    assert f(2, 8, 100, D, D, D, D, D, 1e-8, None, D, D, None) == -1
    assert f(0, 8, 100, D, D, D, D, D, 1e-8, D, D, D, None) == -2
    assert f(2, 8, 0, D, D, D, D, D, 1e-8, D, D, D, None) == -2
    assert f(1 << 20, 1 << 20, 100, D, D, D, D, D, 1e-8, D, D, D, None) == -2
    g = L.avse_dwconv_gln_fwd_len                            # B C K P dil x len w alpha gamma beta eps y1 y stats ws
    assert g(2, 8, 100, 3, 1, D, None, D, D, D, D, 1e-8, D, D, D, D, None) == -1
    assert g(2, 8, 100, 3, 1, D, D, D, D, D, D, 1e-8, None, D, D, D, None) == -1
    assert g(2, 8, 100, 4, 1, D, D, D, D, D, D, 1e-8, D, D, D, D, None) == -2          # even kernel
    assert g(2, 8, 100, 3, 513, D, D, D, D, D, D, 1e-8, D, D, D, D, None) == -2        # halo > 512
    assert g(2, 0, 100, 3, 1, D, D, D, D, D, D, 1e-8, D, D, D, D, None) == -2
    q = L.avse_dwconv_gln_fwd_q_len                          # ... y1 hi lo kp maxbits stats ws stream
    assert q(2, 8, 100, 3, 1, D, None, D, D, D, D, 1e-8, D, D, D, 104, D, D, D, None) == -1
    assert q(2, 8, 100, 3, 1, D, D, D, D, D, D, 1e-8, D, D, D, 104, None, D, D, None) == -1
    assert q(2, 8, 100, 3, 1, D, D, D, D, D, D, 1e-8, D, D, D, 96, D, D, D, None) == -2     # kp < K
    assert q(2, 8, 100, 3, 1, D, D, D, D, D, D, 1e-8, D, D, D, 100, D, D, D, None) == -2    # kp % 8
    assert q(2, 8, 100, 3, 1, D, D, D, D, D, D, 1e-8, D, ctypes.c_void_p(72), D, 104, D, D, D, None) == -5   # alignment


@needs_lib
def test_dwconv_and_upsample_validate_on_the_host():
    from avse_challenge_amd import _lib
    L = _lib.lib()
    f = L.avse_dwconv_fwd_len                                # B C K P dil x len w y stream
    assert f(2, 8, 25, 3, 1, D, None, D, D, None) == -1
    assert f(2, 8, 25, 3, 1, D, D, D, None, None) == -1
    assert f(2, 8, 25, 2, 1, D, D, D, D, None) == -2
    assert f(2, 8, 0, 3, 1, D, D, D, D, None) == -2
    u = L.avse_upsample_linear_len                           # B C n_in K up v v_bs v_cs vlen klen out o_bs o_cs stream
    assert u(2, 8, 25, 799, 32, None, 200, 25, D, D, D, 16 * 799, 799, None) == -1
    assert u(2, 8, 25, 799, 32, D, 200, 25, D, None, D, 16 * 799, 799, None) == -1
    assert u(2, 8, 25, 799, 0, D, 200, 25, D, D, D, 16 * 799, 799, None) == -2
    assert u(2, 8, 25, 799, 32, D, 200, 24, D, D, D, 16 * 799, 799, None) == -2        # input rows overlap
    assert u(2, 8, 25, 799, 32, D, 200, 25, D, D, D, 16 * 799, 798, None) == -2        # output rows overlap
    assert u(2, 8, 25, 799, 32, D, 200, 25, D, D, D, 7 * 799, 799, None) == -2         # output samples overlap
