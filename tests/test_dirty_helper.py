"""CPU tests of the dirty-memory helper (tests/_dirty.py) and of three host functions no other test referenced."""
import numpy as np
import pytest
import torch

import _dirty


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.int32, torch.uint8])
def test_poison_pattern_per_dtype(dtype):
    t = _dirty.poison_(torch.empty((3, 5), dtype=dtype))
    if dtype.is_floating_point:
        assert bool(torch.isnan(t).all())
        raw = t.view(torch.int16)
        assert bool((raw == _dirty.POISON16).all())
    elif dtype == torch.int32:
        assert bool((t == 0x7FC07FC0).all()) and int(t.min()) > 0      # an unreset atomicMax target keeps it
    else:
        assert t.flatten().tolist() == [0xC0, 0x7F] * 7 + [_dirty.POISON_TAIL]      # 15 bytes: the odd tail


def test_poison_covers_the_storage_not_only_the_view():
    full = torch.zeros((2, 3, 8))
    view = full[..., :5]
    _dirty.poison_(view)
    assert bool(torch.isnan(full).all())
    assert _dirty.poison_(torch.empty(0)).numel() == 0


def test_proxy_forwards_and_poisons(monkeypatch):
    from avse_challenge_amd import kernels as K
    real_empty = torch.empty((4,)).new_zeros(1)          # torch itself is untouched
    with _dirty.dirty(monkeypatch):
        for mod in _dirty.package_modules():
            assert isinstance(mod.torch, _dirty.PoisonTorch)
        assert isinstance(real_empty, K.torch.Tensor) and K.torch.float32 is torch.float32
        v = K._bdl_empty(2, 3, 250, torch.float32, "cpu")            # 250 -> 256 columns
        assert tuple(v.shape) == (2, 3, 250) and v.stride() == (3 * 256, 256, 1)
        full = torch.empty(0).set_(v.untyped_storage(), 0, (2, 3, 256), (3 * 256, 256, 1))
        assert bool(torch.isnan(full).all())                         # the pads too
        x = torch.zeros((2, 8, 3, 5)).contiguous(memory_format=torch.channels_last)
        y = K.torch.empty_like(x)
        assert y.stride() == x.stride() and bool(torch.isnan(y).all())
        z = K.torch.empty_strided((2, 3), (4, 1), dtype=torch.bfloat16)
        assert z.stride() == (4, 1) and bool(torch.isnan(z).all())
        m = K.torch.empty(1, dtype=torch.int32)
        assert int(m) == 0x7FC07FC0
    for mod in _dirty.package_modules():
        assert mod.torch is torch
    with _dirty.clean():
        assert K.torch is torch


def test_both_runs_clean_then_dirty(monkeypatch):
    from avse_challenge_amd import kernels as K
    a, b = _dirty.both(lambda: K.torch.empty(3).sum().item(), monkeypatch)
    assert np.isnan(b) and K.torch is torch


# ------------------------------------------------------------------ host functions without a test of their own

def test_stft_frames_equals_the_oracle_frame_count():
    from avse_challenge_amd import kernels as K
    from oracle import stft_ref
    for T in (1000, 16000, 127, 128):
        assert K.stft_frames(T) == stft_ref.stft_mag_T(np.zeros((1, T), np.float32)).shape[1]


def test_kernel_error_message_names_the_code():
    from avse_challenge_amd import kernels as K
    assert "0x71000005" in K.kernel_error_message(0x71000005)


def test_dconv_split_ok_is_false_off_the_gpu():
    from avse_challenge_amd import kernels as K
    assert K.dconv_split_ok(torch.zeros((1, 64, 4, 256)), 2) is False            # the supported shape, on the CPU
    assert K.dconv_split_ok(torch.empty((1, 64, 4, 256), device="meta"), 2) is False
