"""Throughput of GPU MBSTOI scoring (avse_challenge_amd/metrics.py): B = 32 utterances of 48000 samples at 16 kHz.

    python tools/mbstoi_bench.py [--batch 32 --samples 48000 --iters 200 --warmup 5] [--out profiles/mbstoi_bench.json]

Prints one JSON line: utterances/s of the whole call (resampling included) from device events around `iters` calls,
the time of each stage (resample, gate, bands, ec + mean) from device events around `iters` calls of that stage
alone, and the time of the test-side numpy restatement (tests/mbstoi_ref.py) for ONE utterance on this machine's
CPU.  A run without a GPU fails; nothing here falls back.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from avse_challenge_amd import metrics  # noqa: E402


def _events_ms(fn, iters):
    """Mean milliseconds of fn() over `iters` back-to-back calls, by device events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def signals(batch, samples, seed=0):
    """Speech-like binaural pairs: low-passed noise under a slow envelope, a delayed and attenuated right ear, a
    processed pair with independent noise per ear (float32, on the host)."""
    g = np.random.default_rng(seed)
    src = g.standard_normal((batch, samples + 16))
    k = np.hanning(9) / 4.0
    src = np.stack([np.convolve(s, k, mode="same") for s in src])
    env = 0.25 + np.abs(np.sin(2 * np.pi * 3.1 * np.arange(samples + 16) / 16000 + g.uniform(0, 3, (batch, 1))))
    src = 0.1 * src * env
    clean = np.stack([src[:, 8:8 + samples], 0.6 * src[:, 3:3 + samples]], axis=1)
    proc = clean + 0.03 * g.standard_normal(clean.shape)
    return clean.astype(np.float32), proc.astype(np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy restatement's time")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mbstoi_bench needs the GPU")
    dev = torch.device("cuda", 0)
    clean_h, proc_h = signals(a.batch, a.samples)
    clean, proc = torch.from_numpy(clean_h).to(dev), torch.from_numpy(proc_h).to(dev)

    def whole():
        return metrics.mbstoi(clean, proc, sr=a.sr)

    for _ in range(a.warmup):
        scores = whole()
    torch.cuda.synchronize()
    total_ms = _events_ms(whole, a.iters)
    # the stages, each alone on the inputs the stage before it produced
    sig, lengths10k = metrics.prepare(clean, proc, a.sr)
    kept, K = metrics.gate(sig, lengths10k)
    bq = metrics.bands(sig, kept, K)
    stages = {
        "resample_ms": _events_ms(lambda: metrics.prepare(clean, proc, a.sr), a.iters),
        "gate_ms": _events_ms(lambda: metrics.gate(sig, lengths10k), a.iters),
        "bands_ms": _events_ms(lambda: metrics.bands(sig, kept, K), a.iters),
        "ec_and_mean_ms": _events_ms(lambda: metrics.ec_stage(bq, K, 1, frames_offset=1), a.iters),
    }
    frames = int(K.max().item()) - 1
    rec = {
        "metric": "mbstoi_utterances_per_s", "value": round(a.batch / (total_ms * 1e-3), 1), "unit": "utterances/s",
        "batch": a.batch, "samples": a.samples, "sr": a.sr, "iters": a.iters, "warmup": a.warmup,
        "ms_per_batch": round(total_ms, 4), **{k: round(v, 4) for k, v in stages.items()},
        "stft_frames": frames, "cells_per_utterance": 15 * max(frames - 29, 0), "grid": [100, 40],
        "mean_score": float(scores.mean().item()), "device": torch.cuda.get_device_name(0),
    }
    if not a.no_cpu:
        import mbstoi_ref
        mbstoi_ref.mbstoi(clean_h[0], proc_h[0], a.sr)               # warm numpy's FFT plans
        t0 = time.perf_counter()
        ref = mbstoi_ref.mbstoi(clean_h[0], proc_h[0], a.sr)
        rec["cpu_restatement_s_per_utterance"] = round(time.perf_counter() - t0, 3)
        rec["gpu_minus_cpu_restatement_score"] = float(scores[0].item()) - ref["score"]
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
