"""Objective metrics on the MI355X: MBSTOI, the score the AVSE-4 challenge ranks binaural output by.

Counterpart of evaluation/avse4/objective_evaluation.py:60-69 and its vendored evaluation/avse4/mbstoi package
(mbstoi.py:31-334, mbstoi_utils.py:17-540), with the reference's defaults and quirks (the exclusive frame range, the
never-filled last better-ear segment, the `-1` rule, numpy's first-maximum order).  fp64 throughout:

  resample to 10 kHz   torch.fft in fp64 (scipy.signal.resample restated on rfft / irfft), grouped by length
  silent-frame gate    csrc/mbstoi.hip avse_mbstoi_gate   (energies, 40 dB gate, compacted frame list, on the device)
  STFT + band sums     csrc/mbstoi.hip avse_mbstoi_bands  (re-stitch, window, FFT-512, 8 numbers per frame and band)
  EC grid + better ear csrc/mbstoi.hip avse_mbstoi_ec     (one wave per (utterance, band, segment) cell)
  mean                 csrc/mbstoi.hip avse_mbstoi_score

STOI and PESQ (pystoi / pesq in the reference's script) are third-party packages and stay out of scope.
"""
import functools
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .kernels import _need_gpu

FS, NWIN, HOP, NBANDS, NSEG = 10000, 256, 128, 15, 30


def grid_tables(gridcoarseness=1):
    """The (tau, gamma) grid of the EC stage with its jitter factors, in numpy fp64 by the reference's formulas
    (mbstoi.py:97-98, :200-212, mbstoi_utils.py:78-95): (window (256,), tau_table (15, n_taus, 6), gamma_table
    (n_gammas, 6)) in the layout include/avse_hip.h gives for avse_mbstoi_ec."""
    n_taus, n_gammas = math.ceil(100 / gridcoarseness), math.ceil(40 / gridcoarseness)
    taus = np.linspace(-0.001, 0.001, n_taus)
    gammas = np.linspace(-20, 20, n_gammas)
    sigma_epsilon = np.sqrt(2) * 1.5 * (1 + (abs(gammas) / 13) ** 1.6) / 20
    gammas = gammas / 20
    sigma_delta = np.sqrt(2) * 65e-6 * (1 + (abs(taus) / 1.6e-3))
    omega = 2 * math.pi * (np.power(2.0 ** (1.0 / 3), np.arange(NBANDS, dtype=np.float64)) * 150)
    tt = np.empty((NBANDS, n_taus, 6))
    for i, w in enumerate(omega):
        tauexp, tauexp2 = np.exp(-1j * w * taus), np.exp(-1j * 2 * w * taus)
        tt[i, :, 0], tt[i, :, 1], tt[i, :, 2], tt[i, :, 3] = tauexp.real, tauexp.imag, tauexp2.real, tauexp2.imag
        tt[i, :, 4] = np.exp(-2 * w ** 2 * sigma_delta ** 2)
        tt[i, :, 5] = np.exp(0.5 * (-w ** 2 * sigma_delta ** 2))
    gt = np.stack([10.0 ** gammas, 10.0 ** -gammas, 10.0 ** (2 * gammas), 10.0 ** (-2 * gammas),
                   np.exp(2 * np.log(10) ** 2 * sigma_epsilon ** 2),
                   np.exp(0.5 * np.log(10) ** 2 * sigma_epsilon ** 2)], axis=1)
    return np.hanning(NWIN + 2)[1:-1].copy(), tt, gt


@functools.lru_cache(maxsize=8)
def _device_tables(gridcoarseness, device):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in grid_tables(gridcoarseness))


def frames_of(length):
    """len(range(0, length - 256, 128))"""
    return int(_lib.lib().avse_mbstoi_frames(int(length)))


def resample_10k(x, sr):
    """x (G, C, T) fp64 -> (G, C, m), m = int(T * 10000 / sr + 1): scipy.signal.resample of mbstoi.py:107-124 restated
    as rfft, copy of the first min(T, m) // 2 + 1 bins (the Nyquist bin folded as scipy folds it), irfft(n=m), m / T."""
    if sr == FS:
        return x
    T = x.shape[-1]
    m = int(T * (float(FS) / sr) + 1)
    X = torch.fft.rfft(x, dim=-1)
    N = min(T, m)
    Y = torch.zeros(x.shape[:-1] + (m // 2 + 1,), dtype=X.dtype, device=x.device)
    Y[..., :N // 2 + 1] = X[..., :N // 2 + 1]
    if N % 2 == 0 and m != T:
        Y[..., N // 2] *= 2.0 if m < T else 0.5
    return torch.fft.irfft(Y, n=m, dim=-1) * (float(m) / float(T))


def gate(sig, lengths10k):
    """sig (B, 4, M) fp64, lengths10k (B,) int32 on the device -> (kept (B, F) int32, K (B,) int32)."""
    B, _, M = sig.shape
    L = _lib.lib()
    F = frames_of(M)
    win = _device_tables(1, sig.device)[0]
    ws = torch.empty(max(1, L.avse_mbstoi_workspace_bytes(B, M) // 8), device=sig.device, dtype=torch.float64)
    kept = torch.empty((B, F), device=sig.device, dtype=torch.int32)
    K = torch.empty((B,), device=sig.device, dtype=torch.int32)
    check(L.avse_mbstoi_gate(B, M, ptr(sig), ptr(lengths10k), ptr(win), ptr(ws), ptr(kept), ptr(K),
                             stream_ptr(sig.device)), "avse_mbstoi_gate")
    return kept, K


def bands(sig, kept, K):
    """The 8 band quantities of every STFT frame of the re-stitched signals: (B, F - 1, 15, 8) fp64."""
    B, _, M = sig.shape
    F = frames_of(M)
    win = _device_tables(1, sig.device)[0]
    bq = torch.empty((B, F - 1, NBANDS, 8), device=sig.device, dtype=torch.float64)
    check(_lib.lib().avse_mbstoi_bands(B, M, ptr(sig), ptr(win), ptr(kept), ptr(K), ptr(bq), stream_ptr(sig.device)),
          "avse_mbstoi_bands")
    return bq


def ec_stage(bq, frames=None, gridcoarseness=1, frames_offset=0, return_intermediates=False):
    """The EC grid search, the better-ear selection and the mean from band quantities bq (B, F, 15, 8) fp64.

    frames (B,) int32 on the device: utterance b has frames[b] - frames_offset STFT frames (default: all F).
    Returns the (B,) scores, or with return_intermediates a dict with score, d, d_ec, p_ec (B, 15, F - 29) and winner
    (int32: tau index * n_gammas + gamma index, -1 where the `-1` rule fired)."""
    _need_gpu(bq, frames)
    if bq.dim() != 4 or tuple(bq.shape[2:]) != (NBANDS, 8) or bq.dtype != torch.float64:
        raise RuntimeError("ec_stage expects (B, frames, 15, 8) fp64 band quantities")
    bq = bq.contiguous()
    B, F = bq.shape[:2]
    dev = bq.device
    if frames is None:
        frames, frames_offset = torch.full((B,), F, device=dev, dtype=torch.int32), 0
    S = F - NSEG + 1
    if S <= 0:                                  # the mean of no cells
        score = torch.full((B,), float("nan"), device=dev, dtype=torch.float64)
        empty = torch.zeros((B, NBANDS, 0), device=dev, dtype=torch.float64)
        return dict(score=score, d=empty, d_ec=empty, p_ec=empty, winner=empty.int()) if return_intermediates else score
    _, tt, gt = _device_tables(gridcoarseness, dev)
    d = torch.empty((B, NBANDS, S), device=dev, dtype=torch.float64)
    d_ec = torch.empty_like(d) if return_intermediates else None
    p_ec = torch.empty_like(d) if return_intermediates else None
    winner = torch.empty((B, NBANDS, S), device=dev, dtype=torch.int32) if return_intermediates else None
    score = torch.empty((B,), device=dev, dtype=torch.float64)
    L = _lib.lib()
    check(L.avse_mbstoi_ec(B, F, ptr(frames), frames_offset, tt.shape[1], gt.shape[0], ptr(bq), ptr(tt), ptr(gt), ptr(d),
                           ptr(d_ec), ptr(p_ec), ptr(winner), stream_ptr(dev)), "avse_mbstoi_ec")
    check(L.avse_mbstoi_score(B, F, ptr(frames), frames_offset, ptr(d), ptr(score), stream_ptr(dev)), "avse_mbstoi_score")
    if return_intermediates:
        return dict(score=score, d=d, d_ec=d_ec, p_ec=p_ec, winner=winner)
    return score


def _host_lengths(lengths, B, T):
    if lengths is None:
        return [T] * B
    if torch.is_tensor(lengths):
        lengths = lengths.tolist()              # grouping by length is decided on the host
    lengths = [int(v) for v in lengths]
    if len(lengths) != B or any(v <= 0 or v > T for v in lengths):
        raise RuntimeError(f"lengths must hold {B} sample counts in 1..{T}")
    return lengths


def prepare(clean, processed, sr=16000, lengths=None):
    """The four signals of every utterance at 10 kHz: (sig (B, 4, M) fp64, lengths10k (B,) int32 on the device).
    Utterances of equal length are resampled together; sig is defined up to each utterance's own length only."""
    _need_gpu(clean, processed)
    if clean.dim() != 3 or clean.shape[1] != 2 or clean.shape != processed.shape:
        raise RuntimeError("mbstoi expects clean and processed of one shape (B, 2, T)")
    if not (clean.is_floating_point() and processed.is_floating_point()):
        raise RuntimeError("mbstoi expects floating-point signals")
    B, _, T = clean.shape
    host = _host_lengths(lengths, B, T)
    m_of = {n: (n if sr == FS else int(n * (float(FS) / sr) + 1)) for n in set(host)}
    M = max(m_of.values())
    sig = torch.empty((B, 4, M), device=clean.device, dtype=torch.float64)
    for n in sorted(m_of):
        idx = [b for b, v in enumerate(host) if v == n]
        sel = idx if len(idx) < B else slice(None)
        x = torch.cat([clean[sel, :, :n].double(), processed[sel, :, :n].double()], dim=1)
        sig[sel, :, :m_of[n]] = resample_10k(x, sr)
    lengths10k = torch.tensor([m_of[n] for n in host], dtype=torch.int32).to(clean.device, non_blocking=True)
    return sig, lengths10k


def mbstoi(clean, processed, sr=16000, lengths=None, gridcoarseness=1, return_intermediates=False):
    """MBSTOI of a batch: clean, processed (B, 2, T) GPU tensors of any float dtype (left, right), promoted to fp64.

    sr: their sample rate (resampled to 10 kHz when it differs); lengths: per-utterance sample counts of a padded
    batch; gridcoarseness: as the reference's (ceil(100 / gc) taus x ceil(40 / gc) gammas).  Returns the (B,) fp64
    scores on the device (NaN for an utterance with fewer than 30 STFT frames, as the reference's mean of nothing).
    With return_intermediates a dict: score, sig, lengths10k, kept, K, bq, d, d_ec, p_ec, winner."""
    sig, lengths10k = prepare(clean, processed, sr, lengths)
    B = sig.shape[0]
    F = frames_of(sig.shape[2])
    if F >= 1:
        kept, K = gate(sig, lengths10k)
    else:                                       # too short for one frame
        kept = torch.zeros((B, 0), device=sig.device, dtype=torch.int32)
        K = torch.zeros((B,), device=sig.device, dtype=torch.int32)
    if F >= 2:
        bq = bands(sig, kept, K)
    else:
        bq = torch.zeros((B, 0, NBANDS, 8), device=sig.device, dtype=torch.float64)
    res = ec_stage(bq, K, gridcoarseness, frames_offset=1, return_intermediates=return_intermediates)
    if not return_intermediates:
        return res
    res.update(sig=sig, lengths10k=lengths10k, kept=kept, K=K, bq=bq)
    return res
