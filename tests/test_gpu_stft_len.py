"""Length-aware STFT / iSTFT (avse_stft_fwd_len, avse_istft_len; kernels.stft / istft with lengths) against the dense
kernels on each row cropped to its own length, bit for bit.

One padded batch of three rows: T = 1000 (8 frames, 1000 % 128 = 104), 1151 = 8 * 128 + 127 (9 frames: the longest
row, one sample short of a tenth frame) and 257 (the smallest legal length: 3 frames, the reflect pad of 256 samples
reaches the row's first sample from both ends).  All GPU work allocates dirty (tests/_dirty.py)."""
import pytest
import torch

import _dirty
from oracle.det_init import det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_LEN = (1000, 1151, 257)
F_LEN = tuple(1 + t // 128 for t in T_LEN)
TMAX = max(T_LEN)


def padded(fill):
    w = torch.full((len(T_LEN), TMAX), fill)
    for b, t in enumerate(T_LEN):
        w[b, :t] = 0.1 * det_input((t,), 6100 + b)
    return w.to(DEV)


@pytest.fixture(scope="module")
def dense():
    """The dense kernels on each row alone: (mag, complex spectrum) per row, computed once."""
    from avse_challenge_amd import kernels as K
    w = padded(0.0)
    return [K.stft(w[b:b + 1, :t].contiguous(), return_complex=True) for b, t in enumerate(T_LEN)]


def test_frame_counts():
    assert F_LEN == (8, 9, 3) and 1 + TMAX // 128 == 9


@pytest.mark.parametrize("fill", [0.0, float("nan")], ids=["zeros", "nan_padding"])
def test_stft_len_is_the_dense_stft_of_the_cropped_row(dense, fill, monkeypatch):
    from avse_challenge_amd import kernels as K
    with _dirty.dirty(monkeypatch):
        mag, spec = K.stft(padded(fill), return_complex=True, lengths=T_LEN)
        mag_only = K.stft(padded(fill), lengths=T_LEN)
    assert mag.shape == (3, 9, 257) and spec.shape == (3, 9, 257)
    assert torch.equal(mag, mag_only)
    sr = torch.view_as_real(spec)
    for b, f in enumerate(F_LEN):
        assert torch.equal(mag[b, :f], dense[b][0][0]), b
        assert torch.equal(sr[b, :f], torch.view_as_real(dense[b][1][0])), b
        assert not mag[b, f:].any() and not sr[b, f:].any(), b             # exact zeros, not NaN


@pytest.mark.parametrize("fill", [0.0, float("nan")], ids=["zeros", "nan_padding"])
def test_istft_len_is_the_dense_istft_of_the_cropped_row(dense, fill, monkeypatch):
    from avse_challenge_amd import kernels as K
    mag = torch.full((3, 9, 257), fill, device=DEV)
    spec = torch.full((3, 9, 257, 2), fill, device=DEV)
    for b, f in enumerate(F_LEN):
        mag[b, :f] = 0.5 * dense[b][0][0] + 0.01                            # not the noisy magnitude itself
        spec[b, :f] = torch.view_as_real(dense[b][1][0])
    spec = torch.view_as_complex(spec)
    with _dirty.dirty(monkeypatch):
        out = K.istft(mag, spec, TMAX + 5, lengths=T_LEN)                   # an output wider than the longest row
    assert out.shape == (3, TMAX + 5)
    for b, (t, f) in enumerate(zip(T_LEN, F_LEN)):
        ref = K.istft(mag[b:b + 1, :f].contiguous(), spec[b:b + 1, :f].contiguous(), t)
        assert torch.equal(out[b, :t], ref[0]), b
        assert not out[b, t:].any(), b
        assert bool(out[b, :t].abs().max() > 0)


def test_bad_lengths_raise():
    from avse_challenge_amd import kernels as K
    w = padded(0.0)
    with pytest.raises(ValueError):
        K.stft(w, lengths=(1000, 1151, 256))                                # no room for the reflect pad
    with pytest.raises(ValueError):
        K.stft(w, lengths=(1000, 1152, 257))                                # longer than the rows
    with pytest.raises(ValueError):
        K.stft(w, lengths=(1000, 1151))                                     # one length per row
    mag, spec = K.stft(w, return_complex=True, lengths=T_LEN)
    with pytest.raises(ValueError):
        K.istft(mag, spec, TMAX, lengths=(1000, 1151, 256))
    with pytest.raises(ValueError):
        K.istft(mag, spec, TMAX, lengths=(1000, 1152, 257))                 # longer than the output
    with pytest.raises(ValueError):
        K.istft(mag[:, :8].contiguous(), spec[:, :8].contiguous(), TMAX, lengths=T_LEN)     # 9 frames needed, 8 held
