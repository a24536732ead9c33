"""Enhance a directory of noisy binaural wavs with an avse4 checkpoint in ragged batches on the GPU: the counterpart of
the reference's baseline/avse4/test.py (:39-46), which calls `model.enhance(data)` on one utterance at a time.

    python tools/avse4_enhance.py --ckpt model.ckpt --noisy scenes/ --lips lips/ --out enhanced/ \\
        [--noisy-suffix _mix --batch-size 16 --max-pad-ratio 1.25]

For every `<scene><noisy-suffix>.wav` in --noisy with a `<scene>.npy` in --lips -- the preprocessed lip frames,
(Tv, 112, 112) float32 as the reference's dataset.process_frames (dataset.py:157-170) makes them from the scene's
mp4; decoding the mp4 is left to the caller -- it writes `<out>/<scene>.wav` (PCM_16, 16 kHz, ckpt_io.write_wav) unless
that file exists already, as test.py does.  Scenes are sorted by length and cut into batches by
ragged.plan_ragged_batches; each batch is one AVSE4BaselineModule.enhance_batch call.  The output directory is what
tools/mbstoi_eval.py reads (with --enhanced-suffix "").
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avse_challenge_amd import avse4, ckpt_io, ragged  # noqa: E402

SAMPLE_RATE = 16000


def find_scenes(noisy, lips, out, noisy_suffix="_mix"):
    """Scene names with a noisy wav and a lip array whose enhanced file does not exist yet, sorted."""
    names = []
    for f in sorted(os.listdir(noisy)):
        if not f.endswith(noisy_suffix + ".wav"):
            continue
        name = f[:-len(noisy_suffix + ".wav")]
        if os.path.isfile(os.path.join(lips, name + ".npy")) and not os.path.isfile(os.path.join(out, name + ".wav")):
            names.append(name)
    return names


def load_item(noisy, lips, name, noisy_suffix="_mix", num_channels=2):
    audio, sr = ckpt_io.read_wav(os.path.join(noisy, name + noisy_suffix + ".wav"), always_2d=True)
    if sr != SAMPLE_RATE or audio.shape[1] != num_channels:
        raise ValueError(f"{name}: {audio.shape[1]} channel(s) at {sr} Hz, expected {num_channels} at {SAMPLE_RATE}")
    frames = np.load(os.path.join(lips, name + ".npy"), allow_pickle=False)
    if frames.ndim != 3 or frames.shape[1:] != (112, 112):
        raise ValueError(f"{name}: lip array {frames.shape}, expected (Tv, 112, 112)")
    return {"scene": name, "noisy_audio": np.ascontiguousarray(audio.T, dtype=np.float32),
            "vis_feat": frames.astype(np.float32)[None]}


def enhance_dir(model, noisy, lips, out, noisy_suffix="_mix", batch_size=16, max_pad_ratio=1.25):
    """Writes <out>/<scene>.wav for every scene found; returns the scene names written."""
    os.makedirs(out, exist_ok=True)
    names = find_scenes(noisy, lips, out, noisy_suffix)
    items = [load_item(noisy, lips, n, noisy_suffix, model.num_channels) for n in names]

    def run(batch):
        for i, (_, _, est) in zip(batch, model.enhance_batch([items[i] for i in batch])):
            ckpt_io.write_wav(os.path.join(out, names[i] + ".wav"), est.T, SAMPLE_RATE)      # test.py:46
        return [names[i] for i in batch]
    return ragged.run_planned([d["noisy_audio"].shape[-1] for d in items], batch_size, max_pad_ratio, run)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ckpt", required=True, help="Lightning checkpoint of AVSE4BaselineModule")
    ap.add_argument("--noisy", required=True, help="directory of the noisy wavs")
    ap.add_argument("--lips", required=True, help="directory of the <scene>.npy lip arrays")
    ap.add_argument("--out", required=True, help="output directory of the enhanced wavs")
    ap.add_argument("--noisy-suffix", default="_mix")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--max-pad-ratio", type=float, default=1.25)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("avse4_enhance needs the GPU")
    model = avse4.AVSE4BaselineModule.load_from_checkpoint(a.ckpt).to("cuda").eval()
    model.visual_frontend.use_channels_last()
    written = enhance_dir(model, a.noisy, a.lips, a.out, a.noisy_suffix, a.batch_size, a.max_pad_ratio)
    print(f"{len(written)} scenes -> {a.out}")


if __name__ == "__main__":
    main()
