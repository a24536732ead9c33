"""Separate a directory of mixture wavs with a Mamba-TasNet or DPMamba checkpoint in ragged batches on the GPU: the
counterpart of the reference's save_results / save_audio (train_wsj0mix.py:503-642), which separate and score one
utterance per step.

    python tools/mamba_separate.py --hparams results/.../hyperparams.yaml --ckpt-dir results/.../save \\
        --mix wsj0-mix/2speakers/wav8k/min/tt/mix --out separated/ \\
        [--targets .../tt/s1 .../tt/s2] [--batch-size B --max-pad-ratio 1.25 --sample-rate 8000]

For every `<id>.wav` in --mix it writes `<out>/item<id>_source<k>hat.wav` (k = 1 .. n_spk; PCM_16, each source divided
by its peak as save_audio does) unless all of an utterance's files exist already.  Utterances are sorted by length
and cut into batches by ragged.plan_ragged_batches; each batch is one forward_ragged call of the model the hparams
describe (MambaTasNet.separate_batch, DPMambaTasNet.separate_batch).  With --targets (one directory per speaker,
holding `<id>.wav` too) it also writes `<out>/test_results.csv` with the columns snt_id, si-snr, si-snr_i and a final
avg row, from losses.si_snr_pit on the unnormalised estimates, for the utterances separated in this run.  The
reference's sdr / sdr_i columns need mir_eval's bss_eval_sources, which this project does not depend on: they are left
out.  --batch-size defaults to the fastest measured size of the model: 16 for Mamba-TasNet, 4 for DPMamba (DESIGN
§4.11, §4.13).
"""
import argparse
import csv
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avse_challenge_amd import ckpt_io, losses  # noqa: E402

CSV_COLUMNS = ["snt_id", "si-snr", "si-snr_i"]
DEFAULT_BATCH_SIZE = {"MambaTasNet": 16, "DPMambaTasNet": 4}


def out_paths(out_dir, snt_id, n_spk):
    return [os.path.join(out_dir, f"item{snt_id}_source{k + 1}hat.wav") for k in range(n_spk)]


def find_mixtures(mix_dir, out_dir, n_spk):
    """Ids (file stems) of the wavs in mix_dir whose separated files do not all exist yet, sorted."""
    ids = []
    for f in sorted(os.listdir(mix_dir)):
        if f.endswith(".wav") and not all(os.path.isfile(p) for p in out_paths(out_dir, f[:-4], n_spk)):
            ids.append(f[:-4])
    return ids


def load_wav(path, sample_rate):
    audio, sr = ckpt_io.read_wav(path)
    if audio.ndim != 1 or (sample_rate is not None and sr != sample_rate):
        raise ValueError(f"{path}: shape {audio.shape} at {sr} Hz, expected mono" +
                         (f" at {sample_rate} Hz" if sample_rate is not None else ""))
    return np.ascontiguousarray(audio, dtype=np.float32), sr


def score(mix, est, targets):
    """(si-snr, si-snr_i) in dB of one utterance: mix (T,), est and targets (T, n_spk); permutation-invariant."""
    t = torch.from_numpy(targets)[None].double()
    sisnr = -losses.si_snr_pit(t, torch.from_numpy(est)[None].double())
    base = -losses.si_snr_pit(t, torch.from_numpy(mix)[None, :, None].double().expand_as(t))
    return float(sisnr[0]), float(sisnr[0] - base[0])


def separate_dir(model, mix_dir, out_dir, batch_size=16, max_pad_ratio=1.25, sample_rate=8000, target_dirs=None):
    """Writes the separated sources of every mixture found (find_mixtures) and, with target_dirs, test_results.csv;
    returns the ids written, sorted."""
    os.makedirs(out_dir, exist_ok=True)
    n_spk = model.num_spks
    if target_dirs is not None and len(target_dirs) != n_spk:
        raise ValueError(f"{len(target_dirs)} target directories for a model of {n_spk} speakers")
    ids = find_mixtures(mix_dir, out_dir, n_spk)
    mixes = [load_wav(os.path.join(mix_dir, i + ".wav"), sample_rate) for i in ids]
    ests = model.separate_batch([m for m, _ in mixes], batch_size=batch_size, max_pad_ratio=max_pad_ratio)
    rows = []
    for snt_id, (mix, sr), est in zip(ids, mixes, ests):
        for k, path in enumerate(out_paths(out_dir, snt_id, n_spk)):
            peak = float(np.max(np.abs(est[:, k])))
            ckpt_io.write_wav(path, est[:, k] / peak if peak > 0 else est[:, k], sr)      # save_audio: signal / peak
        if target_dirs is not None:
            tg = np.stack([load_wav(os.path.join(d, snt_id + ".wav"), sr)[0] for d in target_dirs], axis=-1)
            if tg.shape[0] != mix.shape[0]:
                raise ValueError(f"{snt_id}: targets of {tg.shape[0]} samples for a mixture of {mix.shape[0]}")
            s, si = score(mix, est, tg)
            rows.append({"snt_id": snt_id, "si-snr": s, "si-snr_i": si})
    if target_dirs is not None:
        with open(os.path.join(out_dir, "test_results.csv"), "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=CSV_COLUMNS)
            w.writeheader()
            w.writerows(rows)
            if rows:
                w.writerow({"snt_id": "avg", "si-snr": float(np.mean([r["si-snr"] for r in rows])),
                            "si-snr_i": float(np.mean([r["si-snr_i"] for r in rows]))})
    return ids


def load_model(hparams, ckpt_dir, device="cuda"):
    model = ckpt_io.model_from_hparams(ckpt_io.read_hparams(hparams))     # a MambaTasNet or a DPMambaTasNet
    ckpt = ckpt_dir if os.path.isfile(os.path.join(ckpt_dir, "CKPTMETA.yaml")) \
        else ckpt_io.find_speechbrain_checkpoint(ckpt_dir)
    if ckpt is None:
        raise SystemExit(f"mamba_separate: no CKPT+* directory under {ckpt_dir}")
    ckpt_io.load_speechbrain_checkpoint(ckpt, ckpt_io.speechbrain_modules(model))
    return model.to(device).eval()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hparams", required=True, help="the run's hyperparams.yaml")
    ap.add_argument("--ckpt-dir", required=True, help="a CKPT+* directory, or the save folder holding them")
    ap.add_argument("--mix", required=True, help="directory of the mixture wavs")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--targets", nargs="*", default=None, help="one directory of clean wavs per speaker")
    ap.add_argument("--batch-size", type=int, default=None, help="default: 16 (Mamba-TasNet), 4 (DPMamba)")
    ap.add_argument("--max-pad-ratio", type=float, default=1.25)
    ap.add_argument("--sample-rate", type=int, default=8000)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mamba_separate needs the GPU")
    model = load_model(a.hparams, a.ckpt_dir)
    batch_size = a.batch_size or DEFAULT_BATCH_SIZE[type(model).__name__]
    written = separate_dir(model, a.mix, a.out, batch_size, a.max_pad_ratio, a.sample_rate, a.targets or None)
    print(f"{len(written)} utterances -> {a.out}")


if __name__ == "__main__":
    main()
