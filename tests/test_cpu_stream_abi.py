"""Streaming entry points of the C ABI (avse_scan_fwd_state, avse_ssm_step, avse_cconv_fwd_state[_bf16],
avse_cconv_update): host-side validation before any launch, and the drop-in names the reference's stateful path
imports (bimamba.py:19,29).  No GPU: every call below must return before a kernel is enqueued."""
import ctypes
import importlib
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIB = os.path.join(REPO, "avse_challenge_amd", "libavse_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libavse_hip.so not built")
DUMMY = ctypes.c_void_p(64)          # a non-null, 16-B aligned address that is never dereferenced on the host


def _scan_args(_lib):
    sa = _lib.ScanFwdStateArgs()
    a = sa.s
    for f in ("u", "delta", "A", "B", "C", "out"):
        setattr(a, f, DUMMY)
    a.batch, a.dim, a.seqlen, a.dstate, a.in_dtype = 1, 64, 10, 16, 0
    return sa


@needs_lib
def test_scan_fwd_state_validates_on_the_host():
    from avse_challenge_amd import _lib
    L = _lib.lib()
    assert L.avse_abi_version() == 2                         # the new entry points are additive
    assert L.avse_scan_fwd_state(None, None) == -1
    assert L.avse_scan_fwd_state(_lib.ScanFwdStateArgs(), None) == -1      # null pointers
    sa = _scan_args(_lib)
    sa.s.dstate = 8
    assert L.avse_scan_fwd_state(sa, None) == -2             # dstate != 16
    sa = _scan_args(_lib)
    sa.s.in_dtype = 7
    assert L.avse_scan_fwd_state(sa, None) == -3             # dtype
    sa = _scan_args(_lib)
    sa.s.reverse = 1
    assert L.avse_scan_fwd_state(sa, None) == -1             # carried state runs forwards only
    sa = _scan_args(_lib)
    sa.s.z, sa.s.out_z, sa.s.out_z_accumulate = DUMMY, DUMMY, 1
    assert L.avse_scan_fwd_state(sa, None) == -1             # no direction sum in the state variant
    sa = _scan_args(_lib)
    sa.s.z, sa.s.out_z, sa.s.out_z_max = DUMMY, DUMMY, DUMMY
    assert L.avse_scan_fwd_state(sa, None) == -1
    sa = _scan_args(_lib)
    sa.h0, sa.h0_bs, sa.h0_ds = ctypes.c_void_p(68), 64 * 16, 16
    assert L.avse_scan_fwd_state(sa, None) == -5             # state rows are read as 16-B vectors
    sa = _scan_args(_lib)
    sa.s.delta_softplus = 3
    assert L.avse_scan_fwd_state(sa, None) == -1


def _step_args(_lib):
    a = _lib.SsmStepArgs()
    for f in ("state", "x", "dt", "A", "B", "C", "out"):
        setattr(a, f, DUMMY)
    a.batch, a.dim, a.dstate, a.dtype = 2, 64, 16, 0
    a.state_bs, a.state_ds = 64 * 16, 16
    return a


@needs_lib
def test_ssm_step_validates_on_the_host():
    from avse_challenge_amd import _lib
    L = _lib.lib()
    assert L.avse_ssm_step(None, None) == -1
    assert L.avse_ssm_step(_lib.SsmStepArgs(), None) == -1   # null pointers
    a = _step_args(_lib)
    a.dstate = 8
    assert L.avse_ssm_step(a, None) == -2
    a = _step_args(_lib)
    a.dtype = 7
    assert L.avse_ssm_step(a, None) == -3
    a = _step_args(_lib)
    a.state_ds = 18
    assert L.avse_ssm_step(a, None) == -5


@needs_lib
def test_cconv_state_and_update_validate_on_the_host():
    from avse_challenge_amd import _lib
    L = _lib.lib()
    for fn in (L.avse_cconv_fwd_state, L.avse_cconv_fwd_state_bf16):
        assert fn(1, 8, 16, 4, None, 16, 16, None, None, None, 16, 16, 1, None, None, 32, 4, None) == -1
        assert fn(1, 8, 16, 5, DUMMY, 16, 16, DUMMY, None, DUMMY, 16, 16, 1, DUMMY, DUMMY, 40, 5, None) == -2
        assert fn(1, 8, 0, 4, DUMMY, 16, 16, DUMMY, None, DUMMY, 16, 16, 1, DUMMY, DUMMY, 32, 4, None) == -2
    up = L.avse_cconv_update
    assert up(1, 8, 4, 0, None, 8, None, 32, 4, None, None, None, 8, 1, None) == -1
    assert up(1, 8, 5, 0, DUMMY, 8, DUMMY, 40, 5, DUMMY, None, DUMMY, 8, 1, None) == -2
    assert up(1, 8, 4, 7, DUMMY, 8, DUMMY, 32, 4, DUMMY, None, DUMMY, 8, 1, None) == -3


def test_new_entry_points_are_declared_and_bound():
    from avse_challenge_amd import _lib
    hdr = open(os.path.join(REPO, "include", "avse_hip.h")).read()
    for name in ("avse_scan_fwd_state", "avse_ssm_step", "avse_cconv_fwd_state", "avse_cconv_fwd_state_bf16",
                 "avse_cconv_update"):
        assert name + "(" in hdr, name
        assert name in _lib.SIGNATURES, name
    # the state struct starts with the forward scan's own fields, unchanged
    assert _lib.ScanFwdStateArgs.s.offset == 0
    assert _lib.ScanFwdStateArgs.h0.offset == ctypes.sizeof(_lib.ScanFwdArgs)


def test_dropin_streaming_names():
    from avse_challenge_amd import dropin
    path = dropin.install()
    try:
        for name in ("causal_conv1d", "mamba_ssm", "mamba_ssm.ops.triton.selective_state_update",
                     "mamba_ssm.utils.generation"):
            sys.modules.pop(name, None)
        cc = importlib.import_module("causal_conv1d")
        assert cc.__file__.startswith(path) and callable(cc.causal_conv1d_update)
        ssu = importlib.import_module("mamba_ssm.ops.triton.selective_state_update")
        assert ssu.__file__.startswith(path) and callable(ssu.selective_state_update)
        gen = importlib.import_module("mamba_ssm.utils.generation")
        ip = gen.InferenceParams(max_seqlen=16, max_batch_size=2)
        assert ip.seqlen_offset == 0 and ip.key_value_memory_dict == {}
        from avse_challenge_amd import mamba_tasnet
        assert importlib.import_module("mamba_ssm").Mamba is mamba_tasnet.Mamba
    finally:
        sys.path.remove(path)


def test_cpu_tensors_are_refused():
    import torch
    from avse_challenge_amd import kernels as K
    x = torch.zeros(1, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        K.causal_conv1d_update(x, torch.zeros(1, 8, 4), torch.zeros(8, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        K.selective_state_update(torch.zeros(1, 8, 16), x, x, torch.zeros(8, 16), torch.zeros(1, 16), torch.zeros(1, 16))
    with pytest.raises(RuntimeError, match="GPU only"):
        K.causal_conv1d_fwd(torch.zeros(1, 8, 5), torch.zeros(8, 4), conv_state=torch.zeros(1, 8, 4))
