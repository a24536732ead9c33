"""Golden outputs of the reference's MBSTOI (evaluation/avse4/mbstoi) -> tests/golden/mbstoi.npz (inputs and results),
mbstoi_sig.npz (the resampled signals, fp64, kept apart for the size limit of a committed file) and
manifest_mbstoi.json.

Run on the build machine only: it imports the reference's ``mbstoi`` package from the reference checkout and writes
numbers only.  The reference's ``mbstoi()`` runs unchanged; its ``remove_silent_frames`` and
``equalisation_cancellation`` are wrapped to record what goes in and what comes out (the resampled signals, the
re-stitched signals, the spectra, ``d`` after the EC stage, ``p_ec_max``), and the array the EC stage returns is the
one ``mbstoi()`` then updates in place with the better-ear values, so it is read again after the call.  The EC-level
case E swaps the two front stages for prepared spectra in which one band is exactly zero over one full segment, so
that the reference's own EC and better-ear code see it.

Beside each reference result the test-side restatement (tests/mbstoi_ref.py) is run on the same input and the
manifest records, per case: ``ref_spread`` = max |d_restatement - d_reference|, ``min_gap`` = the smallest relative
distance between the best and second-best p of any cell, and ``threshold_margin_db`` = the smallest distance of any
frame energy from the 40 dB gate.  tests/test_gpu_mbstoi.py derives its bar from these.

    python tests/golden/make_golden_mbstoi.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("AVSE_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REFERENCE, "evaluation", "avse4"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mbstoi.mbstoi as M  # noqa: E402  (the reference)
import mbstoi.mbstoi_utils as U  # noqa: E402
import mbstoi_ref as R  # noqa: E402  (the restatement)

ARRAYS, SIGNALS, MANIFEST = {}, {}, {}


def signals(T, seed, sr, quiet=None):
    """Speech-like binaural pair: low-passed noise under a slow envelope; the right ear is the left delayed by a few
    samples (ITD) and attenuated (ILD); the processed pair adds independent noise per ear.  float32."""
    g = np.random.default_rng(seed)
    itd = 3 if sr == 10000 else 5
    src = np.convolve(g.standard_normal(T + 64), np.hanning(9) / 4.0, mode="same")
    env = 0.25 + np.abs(np.sin(2 * np.pi * 3.1 * np.arange(T + 64) / sr + 0.4 * seed))
    src = 0.1 * src * env
    left, right = src[16:16 + T], 0.6 * src[16 - itd:16 - itd + T]
    clean = np.stack([left, right])
    proc = clean + 0.03 * g.standard_normal((2, T)) * np.array([[1.0], [0.7]])
    if quiet is not None:
        clean[:, quiet[0]:quiet[1]] *= 1e-4
        proc[:, quiet[0]:quiet[1]] *= 1e-4
    return clean.astype(np.float32), proc.astype(np.float32)


def band_quantities_from_spectra(spec, fids):
    """spec: four (257, frames) single-sided spectra as the reference's EC stage receives them -> (frames, 15, 8)."""
    xl, xr, yl, yr = spec
    out = np.zeros((xl.shape[1], fids.shape[0], 8))
    for i in range(fids.shape[0]):
        sl = slice(int(fids[i, 0] - 1), int(fids[i, 1]))
        for p, (L, Rr) in enumerate(((xl[sl], xr[sl]), (yl[sl], yr[sl]))):
            rho = np.sum(np.conj(Rr) * L, axis=0)
            out[:, i, 4 * p + 0] = np.sum(np.conj(L) * L, axis=0).real
            out[:, i, 4 * p + 1] = np.sum(np.conj(Rr) * Rr, axis=0).real
            out[:, i, 4 * p + 2], out[:, i, 4 * p + 3] = rho.real, rho.imag
    return out


def run_reference(clean, proc, sr, gridcoarseness=1, spectra=None):
    """The reference's mbstoi() with recording wrappers; spectra: four (frames, 512) arrays that replace the gate and
    the STFT (case E)."""
    rec = {}
    real_rsf, real_ec, real_stft = M.remove_silent_frames, M.equalisation_cancellation, M.stft

    def rsf(xl, xr, yl, yr, *a):
        rec["sig"] = np.stack([xl, xr, yl, yr]).copy()
        if spectra is not None:
            return xl, xr, yl, yr
        out = real_rsf(xl, xr, yl, yr, *a)
        rec["sil"] = np.stack(out).copy()
        return out

    feed = list(spectra) if spectra is not None else None

    def stft(sig, n, nfft):
        return feed.pop(0) if feed is not None else real_stft(sig, n, nfft)

    def ec(xl, xr, yl, yr, nb, nfr, fids, *rest):
        rec["bq"] = band_quantities_from_spectra((xl, xr, yl, yr), fids)
        d, p = real_ec(xl, xr, yl, yr, nb, nfr, fids, *rest)
        rec["d_ec"], rec["d_live"], rec["p_ec"] = d.copy(), d, p
        return d, p

    M.remove_silent_frames, M.equalisation_cancellation, M.stft = rsf, ec, stft
    try:
        with np.errstate(all="ignore"):
            rec["score"] = float(M.mbstoi(clean[0].astype(np.float64), clean[1].astype(np.float64),
                                          proc[0].astype(np.float64), proc[1].astype(np.float64), sr,
                                          gridcoarseness=gridcoarseness))
    finally:
        M.remove_silent_frames, M.equalisation_cancellation, M.stft = real_rsf, real_ec, real_stft
    rec["d"] = rec.pop("d_live").copy()
    return rec


def record(name, note, clean, proc, sr, gridcoarseness=1, store_input=True):
    ref = run_reference(clean, proc, sr, gridcoarseness)
    own = R.mbstoi(clean, proc, sr, gridcoarseness)
    # the kept indices are certified by the reference's own output: re-stitching exactly these frames gives its bits
    assert np.array_equal(R.restitch(ref["sig"], own["kept"]), ref["sil"]), name
    K = (ref["sil"].shape[1] - R.NWIN) // R.HOP + 1
    assert K == own["K"]
    e = own["energies"]
    margin = float(np.min(np.abs(e.max(axis=1, keepdims=True) - R.DYN - e)))
    if store_input:
        ARRAYS[name + ".clean"], ARRAYS[name + ".processed"] = clean, proc
    if sr != R.FS and store_input:                 # at 10 kHz the resampled signals are the inputs themselves
        SIGNALS[name + ".sig"] = ref["sig"]
    ARRAYS[name + ".kept"] = own["kept"].astype(np.int32)
    for k in ("bq", "d_ec", "d", "p_ec"):
        ARRAYS[f"{name}.{k}"] = ref[k]
    ARRAYS[name + ".score"] = np.float64(ref["score"])
    spread = float(np.max(np.abs(own["d"] - ref["d"])))
    MANIFEST[name] = {
        "note": note, "sr": sr, "gridcoarseness": gridcoarseness, "samples": int(clean.shape[1]),
        "frames": int(R.n_frames(ref["sig"].shape[1])), "K": int(K), "segments": int(ref["d"].shape[1]),
        "ref_spread": spread, "ref_spread_p_ec": float(np.max(np.abs(own["p_ec"] - ref["p_ec"]))),
        "ref_spread_score": abs(own["score"] - ref["score"]),
        "ref_spread_bq_rel": float(np.max(np.abs(own["bq"] - ref["bq"]).max(axis=0) / np.abs(ref["bq"]).max(axis=0))),
        "min_gap": float(np.min(own["gap"])), "threshold_margin_db": margin,
        "better_ear_cells": int(np.sum(ref["d"] != ref["d_ec"])), "score": ref["score"],
    }
    print(name, json.dumps(MANIFEST[name]))
    return ref


def record_ec_level():
    """Case E: spectra of a 41-frame pair in which band 5 is exactly zero over the frames of segment 3."""
    clean, proc = signals(R.NWIN + R.HOP * 41, 5, 10000)
    sig = np.concatenate([clean, proc]).astype(np.float64)
    spectra = [U.stft(s, R.NWIN, R.NFFT) for s in sig]
    bins, _ = R.band_bins()
    lo, hi = bins[5]
    for s in spectra:
        s[3:3 + R.NSEG, lo:hi] = 0
        s[3:3 + R.NSEG, R.NFFT - hi + 1:R.NFFT - lo + 1] = 0
    ref = run_reference(clean, proc, 10000, spectra=spectra)
    own = R.ec_better_ear(ref["bq"])
    assert ref["d"][5, 3] == -1.0 and ref["p_ec"][5, 3] == 0.0
    for k in ("bq", "d_ec", "d", "p_ec"):
        ARRAYS[f"E.{k}"] = ref[k]
    ARRAYS["E.score"] = np.float64(ref["score"])
    MANIFEST["E"] = {
        "note": "EC level: band 5 exactly zero over segment 3 (the -1 rule, NaN better-ear ratios); input is E.bq",
        "gridcoarseness": 1, "frames": int(ref["bq"].shape[0]), "segments": int(ref["d"].shape[1]),
        "ref_spread": float(np.max(np.abs(own["d"] - ref["d"]))),
        "ref_spread_p_ec": float(np.max(np.abs(own["p_ec"] - ref["p_ec"]))),
        "ref_spread_score": abs(float(np.mean(own["d"])) - ref["score"]),
        "min_gap": float(np.min(own["gap"])), "minus_one_cells": int(np.sum(ref["d"] == -1.0)),
        "better_ear_cells": int(np.sum(ref["d"] != ref["d_ec"])), "score": ref["score"],
    }
    print("E", json.dumps(MANIFEST["E"]))


def main():
    a = signals(9600, 1, 16000)
    record("A", "9600 samples at 16 kHz, no frame removed", *a, 16000)
    b = signals(12800, 2, 16000, quiet=(5200, 8100))
    record("B", "12800 samples at 16 kHz, samples 5200..8100 attenuated by 1e-4: frames removed", *b, 16000)
    c = signals(R.NWIN + R.HOP * 40, 3, 10000)
    record("C", "sr 10000, m = 256 + 128 * 40: the exclusive frame range gives 40 frames", *c, 10000)
    d3 = signals(8000, 4, 16000)
    record("D3", "8000 samples at 16 kHz: the third length of the padded batch D = (A, B, D3)", *d3, 16000)
    record_ec_level()
    record("F", "case A with gridcoarseness 4 (input: A.clean / A.processed)", *a, 16000, gridcoarseness=4,
           store_input=False)
    path = os.path.join(HERE, "mbstoi.npz")
    np.savez_compressed(path, **ARRAYS)
    sig_path = os.path.join(HERE, "mbstoi_sig.npz")
    np.savez_compressed(sig_path, **SIGNALS)
    MANIFEST["_file"] = {"name": "mbstoi.npz", "bytes": os.path.getsize(path),
                         "signals": "mbstoi_sig.npz", "signals_bytes": os.path.getsize(sig_path),
                         "input_bytes_float32": int(sum(v.nbytes for k, v in ARRAYS.items()
                                                        if k.endswith((".clean", ".processed"))))}
    with open(os.path.join(HERE, "manifest_mbstoi.json"), "w") as f:
        json.dump(MANIFEST, f, indent=1, sort_keys=True)
        f.write("\n")
    print(MANIFEST["_file"])


if __name__ == "__main__":
    main()
