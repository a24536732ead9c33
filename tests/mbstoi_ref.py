"""MBSTOI in vectorised fp64 numpy: the test-side restatement of the reference metric (a helper module, no tests).

Restates evaluation/avse4/mbstoi (mbstoi.py:31-334, mbstoi_utils.py:17-224, :361-540) with the reference's quirks:
the exclusive frame range, the never-filled last better-ear segment, the ``-1`` rule and numpy's first-maximum order.
The EC stage works from 8 band quantities per (frame, band) and inner products of length 30 instead of the
spectra; tests/test_mbstoi_ref.py holds it to the goldens recorded from the reference itself.  It also reports, per
cell, the relative gap between the best and the second-best ``p`` of the grid, which bounds the tolerance a GPU
comparison may use before a flipped winner could pass.
"""
import math

import numpy as np

FS, NWIN, HOP, NFFT, NBANDS, NSEG, DYN = 10000, 256, 128, 512, 15, 30, 40.0
EPS = np.finfo(np.float64).eps


def window():
    return np.hanning(NWIN + 2)[1:-1]


def n_frames(m):
    """len(range(0, m - 256, 128)): the end is exclusive, so m = 256 + 128 k gives k frames."""
    return len(range(0, m - NWIN, HOP))


def band_bins():
    """(15, 2) first and one-past-last FFT bin of each third-octave band, and the 15 centre frequencies in Hz."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(NBANDS, dtype=np.float64)
    cf = np.power(2.0 ** (1.0 / 3), k) * 150
    lo = 150 * np.power(2.0, (2 * k - 1) / 6)
    hi = 150 * np.power(2.0, (2 * k + 1) / 6)
    bins = np.array([[np.argmin(np.square(f - lo[i])), np.argmin(np.square(f - hi[i]))] for i in range(NBANDS)])
    return bins, cf


def resample(x, sr):
    """scipy.signal.resample of a real signal to int(T * 10000 / sr + 1) points, restated on rfft / irfft."""
    x = np.asarray(x, dtype=np.float64)
    if sr == FS:
        return x
    T = x.shape[-1]
    m = int(T * (FS / sr) + 1)
    X = np.fft.rfft(x, axis=-1)
    N = min(T, m)
    Y = np.zeros(x.shape[:-1] + (m // 2 + 1,), dtype=np.complex128)
    Y[..., :N // 2 + 1] = X[..., :N // 2 + 1]
    if N % 2 == 0:
        if m < T:
            Y[..., N // 2] *= 2.0
        elif T < m:
            Y[..., N // 2] *= 0.5
    return np.fft.irfft(Y, n=m, axis=-1) * (float(m) / float(T))


def gate(sig):
    """sig (4, m) [clean L, clean R, processed L, processed R] -> (energies (2, frames) in dB, kept frame indices)."""
    m = sig.shape[-1]
    nf = n_frames(m)
    idx = np.arange(nf)[:, None] * HOP + np.arange(NWIN)[None]
    fr = sig[:2][:, idx] * window()
    e = 20 * np.log10(np.sqrt(np.sum(fr * fr, axis=-1)) + EPS)
    mask = ((e[0].max() - DYN - e[0]) < 0) | ((e[1].max() - DYN - e[1]) < 0)
    return e, np.nonzero(mask)[0]


def restitch(sig, kept):
    """Overlap-add of the kept windowed frames at hop 128: (4, (K - 1) * 128 + 256)."""
    K = len(kept)
    idx = kept[:, None] * HOP + np.arange(NWIN)[None]
    fr = sig[:, idx] * window()
    out = np.zeros((sig.shape[0], (K - 1) * HOP + NWIN))
    for i in range(K):
        out[:, i * HOP:i * HOP + NWIN] += fr[:, i]
    return out


def band_quantities(sil):
    """sil (4, n) re-stitched signals -> (frames, 15, 8): PL, PR, Re rho, Im rho of the clean pair, then of the
    processed pair, with PL = sum |X_L|^2, PR = sum |X_R|^2, rho = sum conj(X_R) X_L over the band's bins."""
    nf = n_frames(sil.shape[-1])
    idx = np.arange(nf)[:, None] * HOP + np.arange(NWIN)[None]
    X = np.fft.fft(sil[:, idx] * window(), n=NFFT, axis=-1)[..., :NFFT // 2 + 1]
    bins, _ = band_bins()
    out = np.zeros((nf, NBANDS, 8))
    for i, (lo, hi) in enumerate(bins):
        for p in range(2):
            L, R = X[2 * p, :, lo:hi], X[2 * p + 1, :, lo:hi]
            rho = np.sum(np.conj(R) * L, axis=-1)
            out[:, i, 4 * p + 0] = np.sum(np.abs(L) ** 2, axis=-1)
            out[:, i, 4 * p + 1] = np.sum(np.abs(R) ** 2, axis=-1)
            out[:, i, 4 * p + 2] = rho.real
            out[:, i, 4 * p + 3] = rho.imag
    return out


def grid_tables(gridcoarseness=1):
    """The tau and gamma grids and their jitter factors (mbstoi.py:200-212, mbstoi_utils.py:78-95).

    Returns (tau_table (15, n_taus, 6), gamma_table (n_gammas, 6)):
      tau_table[i, t]  = cos(w tau), -sin(w tau), cos(2 w tau), -sin(2 w tau), deltexp, exp(-w^2 sigma_delta^2 / 2)
      gamma_table[g]   = 10^gamma, 10^-gamma, 10^(2 gamma), 10^(-2 gamma), epsexp, exp(ln(10)^2 sigma_eps^2 / 2)
    so that tauexp = tt[0] + i tt[1], tauexp2 = tt[2] + i tt[3] and epsdelexp[t, g] = tt[5] * gt[5].
    """
    n_taus, n_gammas = math.ceil(100 / gridcoarseness), math.ceil(40 / gridcoarseness)
    taus = np.linspace(-0.001, 0.001, n_taus)
    gammas = np.linspace(-20, 20, n_gammas)
    sigma_eps = np.sqrt(2) * 1.5 * (1 + (abs(gammas) / 13) ** 1.6) / 20
    gammas = gammas / 20
    sigma_del = np.sqrt(2) * 65e-6 * (1 + abs(taus) / 1.6e-3)
    _, cf = band_bins()
    w = 2 * math.pi * cf
    tt = np.zeros((NBANDS, n_taus, 6))
    for i in range(NBANDS):
        te, te2 = np.exp(-1j * w[i] * taus), np.exp(-1j * 2 * w[i] * taus)
        tt[i, :, 0], tt[i, :, 1], tt[i, :, 2], tt[i, :, 3] = te.real, te.imag, te2.real, te2.imag
        tt[i, :, 4] = np.exp(-2 * w[i] ** 2 * sigma_del ** 2)
        tt[i, :, 5] = np.exp(0.5 * (-w[i] ** 2 * sigma_del ** 2))
    gt = np.stack([10.0 ** gammas, 10.0 ** -gammas, 10.0 ** (2 * gammas), 10.0 ** (-2 * gammas),
                   np.exp(2 * np.log(10) ** 2 * sigma_eps ** 2), np.exp(0.5 * np.log(10) ** 2 * sigma_eps ** 2)], axis=1)
    return tt, gt


def _grid(tt, gt, a, b, c1, c2, u, v, w, z):
    """E[s, tau, gamma] from the inner products of one band's segments (each (S,), u v z complex)."""
    te, te2 = tt[:, 0] + 1j * tt[:, 1], tt[:, 2] + 1j * tt[:, 3]
    first = (gt[:, 2] * a[:, None] + gt[:, 3] * b[:, None]) * gt[:, 4]                      # (S, G)
    first = first[:, None, :] + c1[:, None, None] + c2[:, None, None]
    ed = tt[:, 5][:, None] * gt[:, 5][None]                                                  # (T, G)
    second = 2.0 * np.real(te[None] * u[:, None])[:, :, None] * gt[:, 0] * ed
    third = 2.0 * np.real(te[None] * v[:, None])[:, :, None] * gt[:, 1] * ed
    fourth = 2.0 * (w[:, None] + tt[:, 4][None] * np.real(te2[None] * z[:, None]))
    return first - second - third + fourth[:, :, None]


def ec_better_ear(bq, gridcoarseness=1):
    """bq (frames, 15, 8) -> dict of (15, S) arrays, S = frames - 29:
    d_ec (after the EC stage), p_ec, winner (flat tau * n_gammas + gamma, -1 where the -1 rule fired), d (after the
    better-ear selection) and gap (relative distance of the best p from the second best)."""
    F = bq.shape[0]
    S = F - NSEG + 1
    keys = ("d_ec", "p_ec", "winner", "d", "gap")
    if S <= 0:
        return {k: np.zeros((NBANDS, 0), dtype=np.int64 if k == "winner" else np.float64) for k in keys}
    tt, gt = grid_tables(gridcoarseness)
    nt, ng = tt.shape[1], gt.shape[0]
    seg = np.lib.stride_tricks.sliding_window_view(bq, NSEG, axis=0)          # (S, 15, 8, 30)
    out = {k: np.zeros((NBANDS, S), dtype=np.int64 if k == "winner" else np.float64) for k in keys}
    dot = lambda p, q: np.sum(p * q, axis=-1)                                 # noqa: E731
    with np.errstate(all="ignore"):
        for i in range(NBANDS):
            s = seg[:, i]
            s = s - np.mean(s, axis=-1, keepdims=True)
            Lx, Rx, Ly, Ry = s[:, 0], s[:, 1], s[:, 4], s[:, 5]
            rx, ry = s[:, 2] + 1j * s[:, 3], s[:, 6] + 1j * s[:, 7]
            exy = _grid(tt[i], gt, dot(Lx, Ly), dot(Rx, Ry), dot(Lx, Ry), dot(Rx, Ly), dot(Lx, ry) + dot(Ly, rx),
                        dot(Rx, ry) + dot(Ry, rx), np.real(dot(ry, np.conj(rx))), dot(ry, rx))
            exx = _grid(tt[i], gt, dot(Lx, Lx), dot(Rx, Rx), dot(Lx, Rx), dot(Rx, Lx), 2 * dot(Lx, rx),
                        2 * dot(Rx, rx), np.real(dot(rx, np.conj(rx))), dot(rx, rx))
            eyy = _grid(tt[i], gt, dot(Ly, Ly), dot(Ry, Ry), dot(Ly, Ry), dot(Ry, Ly), 2 * dot(Ly, ry),
                        2 * dot(Ry, ry), np.real(dot(ry, np.conj(ry))), dot(ry, ry))
            fired = ~np.all(np.min(np.abs(exx * eyy), axis=1).astype(bool), axis=-1)         # (S,)
            p = exx / eyy
            idx1 = p.argmax(axis=1)                                            # (S, G): first tau with the maximum
            tmp = p.max(axis=1)
            idx2 = tmp.argmax(axis=1)                                          # first gamma with the maximum of those
            ar = np.arange(S)
            t_w = idx1[ar, idx2]
            d = exy[ar, t_w, idx2] / np.sqrt(exx[ar, t_w, idx2] * eyy[ar, t_w, idx2])
            best = tmp[ar, idx2]
            flat = p.reshape(S, -1)
            second = np.partition(flat, flat.shape[1] - 2, axis=1)[:, -2] if flat.shape[1] > 1 else best
            out["d_ec"][i] = np.where(fired, -1.0, d)
            out["p_ec"][i] = np.where(fired, 0.0, best)
            out["winner"][i] = np.where(fired, -1, t_w * ng + idx2)
            out["gap"][i] = np.where(fired, np.inf, (best - second) / np.abs(best))
            # better ear: the last segment is never filled (mbstoi.py:280-282) and keeps its zeros
            li, ri = dot(Lx, Lx) / dot(Ly, Ly), dot(Rx, Rx) / dot(Ry, Ry)
            dl = dot(Lx, Ly) / (np.sqrt(dot(Lx, Lx)) * np.sqrt(dot(Ly, Ly)))
            dr = dot(Rx, Ry) / (np.sqrt(dot(Rx, Rx)) * np.sqrt(dot(Ry, Ry)))
            for arr in (li, ri, dl, dr):
                arr[-1] = 0.0
            dl[~np.isfinite(dl)] = 0
            dr[~np.isfinite(dr)] = 0
            p_be = np.maximum(li, ri)
            dbe = np.where(li > ri, dl, dr)
            out["d"][i] = np.where(p_be > out["p_ec"][i], dbe, out["d_ec"][i])
    return out


def mbstoi(clean, processed, sr=16000, gridcoarseness=1):
    """clean, processed (2, T) -> dict: sig (4, m) resampled, energies, kept, K, bq, the ec_better_ear arrays, score."""
    sig = resample(np.concatenate([np.asarray(clean, np.float64), np.asarray(processed, np.float64)], axis=0), sr)
    energies, kept = gate(sig)
    bq = band_quantities(restitch(sig, kept))
    res = ec_better_ear(bq, gridcoarseness)
    with np.errstate(all="ignore"):
        score = float(np.mean(res["d"])) if res["d"].size else float("nan")
    res.update(sig=sig, energies=energies, kept=kept, K=len(kept), bq=bq, score=score)
    return res
