"""Enhance a directory of noisy mono wavs with an avse1 checkpoint in ragged batches on the GPU: the counterpart of the
reference's baseline/avse1/test.py (:58-89), which runs the model on one scene at a time (`clipped_batch` is off in
test mode, so every scene keeps its own length) and writes `<save_root>/<model_uid>/<scene>.wav`.

    python tools/avse1_enhance.py --ckpt model.ckpt --noisy scenes/ --lips lips/ --save-root out/ --model-uid avse1 \\
        [--noisy-suffix _mix --batch-size 16 --max-pad-ratio 1.25 --a-only]
    python tools/avse1_enhance.py --bench [--utterances 64 --min-s 3 --max-s 9 --batch-sizes 4,16,32 --repeats 3] \\
        [--out profiles/avse1_enhance_bench.json]

For every `<scene><noisy-suffix>.wav` in --noisy with a `<scene>.npy` in --lips -- the lip frames as the reference's
dataset hands them to the model, (3, Tv, H, W) uint8 or float (dataset.py:120-152; decoding the mp4 is left to the
caller; not needed with --a-only) -- it writes `<save-root>/<model-uid>/<scene>.wav` (PCM_16, 16 kHz,
ckpt_io.write_wav) unless that file exists already, as test.py does.  Scenes are sorted by length and cut into batches
by ragged.plan_ragged_batches inside AVNet.enhance_batch.

--bench times, on a seeded synthetic set (noise at 16 kHz, lengths uniform in [min-s, max-s], 25 fps uint8 lips of
96 x 96) and the default-size model with det_init_ weights in eval mode with the channels-last trunks, the loop of
`enhance()` at batch 1 against `enhance_batch` at several batch sizes: one untimed pass per arm, then `repeats` timed
passes between two device events with the arms alternating; host-side padding, the upload and the download are inside
the timed span for both arms.  Prints one JSON line.  A run without a GPU fails; nothing here falls back.
"""
import argparse
import os
import sys

os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC", "1")           # channels-last library convs, as bench.py
os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC_BATCHNORM", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools")]
import ragged_bench  # noqa: E402
from avse_challenge_amd import avse1, ckpt_io  # noqa: E402

SAMPLE_RATE = 16000


def find_scenes(noisy, lips, out, noisy_suffix="_mix", a_only=False):
    """Scene names with a noisy wav (and a lip array) whose enhanced file does not exist yet, sorted."""
    names = []
    for f in sorted(os.listdir(noisy)):
        if not f.endswith(noisy_suffix + ".wav"):
            continue
        name = f[:-len(noisy_suffix + ".wav")]
        if (a_only or os.path.isfile(os.path.join(lips, name + ".npy"))) \
                and not os.path.isfile(os.path.join(out, name + ".wav")):
            names.append(name)
    return names


def load_item(noisy, lips, name, noisy_suffix="_mix", a_only=False):
    audio, sr = ckpt_io.read_wav(os.path.join(noisy, name + noisy_suffix + ".wav"))
    if sr != SAMPLE_RATE or audio.ndim != 1:
        raise ValueError(f"{name}: shape {audio.shape} at {sr} Hz, expected mono at {SAMPLE_RATE}")
    item = {"scene": name, "noisy_audio": np.ascontiguousarray(audio, dtype=np.float32)}
    if not a_only:
        frames = np.load(os.path.join(lips, name + ".npy"), allow_pickle=False)
        if frames.ndim != 4 or frames.shape[0] != 3:
            raise ValueError(f"{name}: lip array {frames.shape}, expected (3, Tv, H, W)")
        item["lip_images"] = frames
    return item


def enhance_dir(model, noisy, lips, out, noisy_suffix="_mix", batch_size=16, max_pad_ratio=1.25):
    """Writes <out>/<scene>.wav for every scene found; returns the scene names written."""
    os.makedirs(out, exist_ok=True)
    names = find_scenes(noisy, lips, out, noisy_suffix, model.a_only)
    items = [load_item(noisy, lips, n, noisy_suffix, model.a_only) for n in names]
    for name, est in zip(names, model.enhance_batch(items, batch_size, max_pad_ratio)):
        ckpt_io.write_wav(os.path.join(out, name + ".wav"), est, SAMPLE_RATE)             # test.py:89
    return names


def synthetic_set(n, min_s, max_s, hw=96, seed=0):
    g = np.random.default_rng(seed)
    items = []
    for _ in range(n):
        t = int(g.integers(int(min_s * SAMPLE_RATE), int(max_s * SAMPLE_RATE) + 1))
        tv = max(1, t * 25 // SAMPLE_RATE)
        items.append({"noisy_audio": (0.1 * g.standard_normal(t)).astype(np.float32),
                      "lip_images": g.integers(0, 256, (3, tv, hw, hw), dtype=np.uint8)})
    return items


def bench(a):
    from oracle.det_init import det_init_
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    items = synthetic_set(a.utterances, a.min_s, a.max_s)
    lengths = [d["noisy_audio"].shape[0] for d in items]
    model = det_init_(avse1.AVNet(), 0).to("cuda").eval()
    model.net_audiofeat.use_channels_last()
    model.net_visualfeat.use_channels_last()

    def loop():
        for d in items:
            model.enhance(torch.from_numpy(d["noisy_audio"])[None].to("cuda"),
                          torch.from_numpy(d["lip_images"])[None].to("cuda"))[0].cpu().numpy()

    ragged_bench.run(a, {"metric": "avse1_enhance_utterances_per_s", "unit": "utterances/s", "model": "avse1 AVNet"},
                     lengths, SAMPLE_RATE, "enhance_loop", loop, "enhance_batch",
                     lambda bs, plan: model.enhance_batch(items, bs, a.max_pad_ratio),
                     extra={"max_stft_frames": 1 + max(lengths) // 128})


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ckpt", help="Lightning checkpoint of AVNet")
    ap.add_argument("--noisy", help="directory of the noisy wavs")
    ap.add_argument("--lips", help="directory of the <scene>.npy lip arrays")
    ap.add_argument("--save-root", help="output root (test.py --save_root)")
    ap.add_argument("--model-uid", default="avse1", help="sub-directory of the enhanced wavs (test.py --model_uid)")
    ap.add_argument("--noisy-suffix", default="_mix")
    ap.add_argument("--a-only", action="store_true", help="the audio-only net (test.py --a_only)")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--max-pad-ratio", type=float, default=1.25)
    ap.add_argument("--bench", action="store_true", help="time enhance_batch against the enhance() loop")
    ragged_bench.add_args(ap, repeats=3, out_help="--bench: also write the line to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("avse1_enhance needs the GPU")
    if a.bench:
        return bench(a)
    if not (a.ckpt and a.noisy and a.save_root and (a.lips or a.a_only)):
        ap.error("--ckpt, --noisy, --save-root and --lips (or --a-only) are needed")
    model = avse1.AVNet.load_from_checkpoint(a.ckpt, a_only=a.a_only).to("cuda").eval()
    model.net_audiofeat.use_channels_last()
    if not a.a_only:
        model.net_visualfeat.use_channels_last()
    out = os.path.join(a.save_root, a.model_uid)
    written = enhance_dir(model, a.noisy, a.lips, out, a.noisy_suffix, a.batch_size, a.max_pad_ratio)
    print(f"{len(written)} scenes -> {out}")


if __name__ == "__main__":
    main()
