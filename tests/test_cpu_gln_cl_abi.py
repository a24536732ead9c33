"""The channels-last GroupNorm(1, N) entry point of the DPMamba ragged path (avse_gln_cl_fwd_len): declared, bound, and
validating on the host before any launch.  No GPU: every call below must return before a kernel is enqueued."""
import ctypes
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIB = os.path.join(REPO, "avse_challenge_amd", "libavse_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libavse_hip.so not built")
D = ctypes.c_void_p(64)              # non-null, 16-B aligned, never dereferenced on the host
NAMES = ("avse_gln_cl_fwd_len", "avse_gln_cl_workspace_bytes")


def args(**over):
    """A valid call on dummy pointers, in the order of the header: B R C N x lengths len_axis gamma beta eps res
    transpose_out y stats workspace stream; over: arguments to change."""
    a = dict(B=2, R=7, C=10, N=64, x=D, lengths=D, len_axis=0, gamma=D, beta=D, eps=1e-8, res=None, transpose_out=0,
             y=D, stats=D, workspace=D, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return tuple(a.values())


def test_entry_points_are_declared_and_bound():
    from avse_challenge_amd import _lib
    hdr = open(os.path.join(REPO, "include", "avse_hip.h")).read()
    for name in NAMES:
        assert name + "(" in hdr, name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["avse_gln_cl_fwd_len"][1]) == len(args())


@needs_lib
def test_abi_version_is_unchanged():
    from avse_challenge_amd import _lib
    L = _lib.lib()                                           # binds every symbol of SIGNATURES, the new ones included
    assert L.avse_abi_version() == 2
    for name in NAMES:
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert L.avse_gln_cl_workspace_bytes(16, 34, 250) == 16 * 34 * 250 * 8


@needs_lib
def test_validates_on_the_host():
    from avse_challenge_amd import _lib
    f = _lib.lib().avse_gln_cl_fwd_len
    for name in ("x", "lengths", "gamma", "beta", "y", "stats", "workspace"):      # res is optional
        assert f(*args(**{name: None})) == -1, name
    for name in ("B", "R", "C", "N"):
        assert f(*args(**{name: 0})) == -2, name
        assert f(*args(**{name: -3})) == -2, name
    for axis in (-1, 2):
        assert f(*args(len_axis=axis)) == -2, axis
        assert f(*args(len_axis=axis, res=D, transpose_out=1)) == -2, axis
    assert f(*args(x=None, N=0)) == -1                       # pointers first, as the other entry points
