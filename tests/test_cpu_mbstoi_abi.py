"""MBSTOI entry points of the C ABI (avse_mbstoi_*): declared, bound, and validating on the host before any launch.
No GPU: every call below must return before a kernel is enqueued."""
import ctypes
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIB = os.path.join(REPO, "avse_challenge_amd", "libavse_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libavse_hip.so not built")
DUMMY = ctypes.c_void_p(64)          # non-null, never dereferenced on the host
NAMES = ("avse_mbstoi_frames", "avse_mbstoi_workspace_bytes", "avse_mbstoi_gate", "avse_mbstoi_bands",
         "avse_mbstoi_ec", "avse_mbstoi_score")


def test_entry_points_are_declared_and_bound():
    from avse_challenge_amd import _lib
    hdr = open(os.path.join(REPO, "include", "avse_hip.h")).read()
    for name in NAMES:
        assert name + "(" in hdr, name
        assert name in _lib.SIGNATURES, name
    for cite in ("mbstoi.py:31-334", "mbstoi_utils.py:392-484", "mbstoi_utils.py:361-389", "mbstoi_utils.py:17-224",
                 "mbstoi.py:279-329"):
        assert cite in hdr, cite


@needs_lib
def test_sizes():
    from avse_challenge_amd import _lib
    L = _lib.lib()
    assert L.avse_abi_version() == 2                         # the new entry points are additive
    # len(range(0, n - 256, 128)): the end is exclusive
    assert L.avse_mbstoi_frames(256 + 128 * 40) == 40 and L.avse_mbstoi_frames(256 + 128 * 40 + 1) == 41
    assert L.avse_mbstoi_frames(256) == 0 and L.avse_mbstoi_frames(257) == 1 and L.avse_mbstoi_frames(0) == 0
    assert L.avse_mbstoi_frames(6001) == 45 and L.avse_mbstoi_frames(30001) == 233
    assert L.avse_mbstoi_workspace_bytes(3, 6001) == 3 * 2 * 45 * 8
    assert L.avse_mbstoi_workspace_bytes(0, 6001) == 0


@needs_lib
def test_gate_and_bands_validate_on_the_host():
    from avse_challenge_amd import _lib
    L = _lib.lib()
    assert L.avse_mbstoi_gate(1, 6001, None, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, None) == -1
    assert L.avse_mbstoi_gate(1, 6001, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, None, None) == -1
    assert L.avse_mbstoi_gate(0, 6001, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, None) == -2
    assert L.avse_mbstoi_gate(1, 0, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, None) == -2
    assert L.avse_mbstoi_gate(1, 1 << 31, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, None) == -2
    assert L.avse_mbstoi_bands(1, 6001, DUMMY, DUMMY, DUMMY, DUMMY, None, None) == -1
    assert L.avse_mbstoi_bands(1, 6001, None, DUMMY, DUMMY, DUMMY, DUMMY, None) == -1
    assert L.avse_mbstoi_bands(0, 6001, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, None) == -2
    assert L.avse_mbstoi_bands(1, 384, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, None) == -2      # one frame: no STFT frame


@needs_lib
def test_ec_and_score_validate_on_the_host():
    from avse_challenge_amd import _lib
    L = _lib.lib()
    ok = (DUMMY, DUMMY, DUMMY, DUMMY)
    assert L.avse_mbstoi_ec(1, 44, None, 1, 100, 40, *ok, None, None, None, None) == -1
    assert L.avse_mbstoi_ec(1, 44, DUMMY, 1, 100, 40, DUMMY, DUMMY, DUMMY, None, None, None, None, None) == -1
    assert L.avse_mbstoi_ec(0, 44, DUMMY, 1, 100, 40, *ok, None, None, None, None) == -2
    assert L.avse_mbstoi_ec(1, 29, DUMMY, 1, 100, 40, *ok, None, None, None, None) == -2   # no full segment
    assert L.avse_mbstoi_ec(1, 44, DUMMY, 1, 0, 40, *ok, None, None, None, None) == -2
    assert L.avse_mbstoi_ec(1, 44, DUMMY, 1, 100, 65, *ok, None, None, None, None) == -2   # gamma columns: one mask word
    assert L.avse_mbstoi_ec(1, 44, DUMMY, 2, 100, 40, *ok, None, None, None, None) == -2
    assert L.avse_mbstoi_score(1, 44, DUMMY, 1, DUMMY, None, None) == -1
    assert L.avse_mbstoi_score(1, 29, DUMMY, 1, DUMMY, DUMMY, None) == -2
    assert L.avse_mbstoi_score(0, 44, DUMMY, 0, DUMMY, DUMMY, None) == -2


def test_cpu_tensors_are_refused():
    import torch
    from avse_challenge_amd import metrics
    x = torch.zeros(1, 2, 9600)
    with pytest.raises(RuntimeError, match="GPU only"):
        metrics.mbstoi(x, x)
    with pytest.raises(RuntimeError, match="GPU only"):
        metrics.ec_stage(torch.zeros(1, 40, 15, 8, dtype=torch.float64))
