"""MBSTOI of a directory of enhanced binaural wavs on the GPU: the counterpart of the reference's
evaluation/avse4/objective_evaluation.py (its compute_mbstoi, :60-69, and run_metrics, :72-103).

    python tools/mbstoi_eval.py --scenes scenes.dev.json --enhanced out/ --target scenes/ \\
        --enhanced-suffix _mix --target-suffix _target_anechoic --results objective_evaluation/

Reads `<scene><suffix>.wav` pairs with ckpt_io.read_wav (two channels: left, right), raises on a length mismatch as
the reference does, skips scenes with a missing file, scores utterances of equal length together on the GPU and
writes `<results>/objective_metrics.csv` with the header `scene,mbstoi` and one row per scored scene in the order of
the scenes json.  STOI and PESQ of the reference's script are not computed (third-party packages, out of scope).
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avse_challenge_amd import ckpt_io, metrics  # noqa: E402


def _read_binaural(path):
    audio, sr = ckpt_io.read_wav(path, always_2d=True)
    if audio.shape[1] != 2:
        raise ValueError(f"{path}: MBSTOI needs a binaural (two-channel) file, got {audio.shape[1]} channel(s)")
    return audio, sr


def evaluate(scenes, enhanced, target, enhanced_suffix="_mix", target_suffix="_target_anechoic", results=None, sr=16000,
             batch_size=32, device="cuda"):
    """scenes: path of a json list of {"scene": name, ...} (or the list itself).  Returns [(scene, mbstoi), ...] in
    json order and, with `results`, writes <results>/objective_metrics.csv."""
    if isinstance(scenes, (str, os.PathLike)):
        with open(scenes) as f:
            scenes = json.load(f)
    names, pairs = [], {}
    for entry in scenes:
        name = entry["scene"]
        enh_file = os.path.join(enhanced, f"{name}{enhanced_suffix}.wav")
        tgt_file = os.path.join(target, f"{name}{target_suffix}.wav")
        if not (os.path.isfile(enh_file) and os.path.isfile(tgt_file)):
            continue                                        # objective_evaluation.py:83-84
        enh, sr_e = _read_binaural(enh_file)
        clean, sr_c = _read_binaural(tgt_file)
        if len(clean) != len(enh):
            raise Exception(f"Wav files {enh_file} and {tgt_file} should have the same length")
        if sr_e != sr or sr_c != sr:
            raise ValueError(f"{name}: files are at {sr_e} / {sr_c} Hz, expected {sr}")
        names.append(name)
        pairs[name] = (clean.T, enh.T)
    scores = {}
    by_len = {}
    for name in names:
        by_len.setdefault(pairs[name][0].shape[1], []).append(name)
    for group in by_len.values():
        for i in range(0, len(group), batch_size):
            chunk = group[i:i + batch_size]
            clean = torch.from_numpy(np.stack([pairs[n][0] for n in chunk])).to(device)
            proc = torch.from_numpy(np.stack([pairs[n][1] for n in chunk])).to(device)
            for n, s in zip(chunk, metrics.mbstoi(clean, proc, sr=sr).tolist()):
                scores[n] = s
    rows = [(n, scores[n]) for n in names]
    if results is not None:
        os.makedirs(results, exist_ok=True)
        with open(os.path.join(results, "objective_metrics.csv"), "w", newline="") as f:
            w = csv.writer(f, delimiter=",", quotechar='"', quoting=csv.QUOTE_MINIMAL)
            w.writerow(["scene", "mbstoi"])
            w.writerows(rows)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", required=True, help="scenes json (a list of {'scene': name})")
    ap.add_argument("--enhanced", required=True, help="directory of the enhanced wavs")
    ap.add_argument("--target", required=True, help="directory of the target wavs")
    ap.add_argument("--enhanced-suffix", default="_mix")
    ap.add_argument("--target-suffix", default="_target_anechoic")
    ap.add_argument("--results", required=True, help="output directory of objective_metrics.csv")
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--batch-size", type=int, default=32)
    a = ap.parse_args(argv)
    rows = evaluate(a.scenes, a.enhanced, a.target, a.enhanced_suffix, a.target_suffix, a.results, a.fs, a.batch_size)
    print(f"{len(rows)} scenes -> {os.path.join(a.results, 'objective_metrics.csv')}")


if __name__ == "__main__":
    main()
