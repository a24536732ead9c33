"""Utterances/s of avse4 enhancement over a ragged set: the `enhance()` loop of the reference's test.py (one utterance
per forward) against `enhance_batch` on avse4.plan_ragged_batches at several batch sizes, same build, same process.

    python tools/avse4_enhance_bench.py [--utterances 64 --min-s 3 --max-s 9 --batch-sizes 4,16,32 --repeats 2] \\
        [--out profiles/avse4_enhance_bench.json]

A seeded synthetic set (binaural noise at 16 kHz, 25 fps lip frames of 112 x 112, lengths uniform in [min-s, max-s]),
the default-size model with det_init_ weights in eval mode, the lip ResNet channels-last.  Every arm gets one untimed
pass over the whole set (allocator, code objects), then `repeats` timed passes between two device events; host-side
padding, the upload and the download are inside the timed span for both arms, as a tool run pays them.  Arms alternate
within a repeat.  Prints one JSON line.  A run without a GPU fails; nothing here falls back.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from avse_challenge_amd import avse4  # noqa: E402
from oracle.det_init import det_init_  # noqa: E402


def synthetic_set(n, min_s, max_s, seed=0, sr=16000, fps=25):
    g = np.random.default_rng(seed)
    items = []
    for _ in range(n):
        t = int(g.integers(int(min_s * sr), int(max_s * sr) + 1))
        tv = max(1, round(t * fps / sr))
        items.append({"noisy_audio": (0.1 * g.standard_normal((2, t))).astype(np.float32),
                      "vis_feat": g.random((1, tv, 112, 112), dtype=np.float32),
                      "clean": np.zeros((2, t), np.float32)})
    return items


def _timed_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=3.0)
    ap.add_argument("--max-s", type=float, default=9.0)
    ap.add_argument("--batch-sizes", default="4,16,32")
    ap.add_argument("--max-pad-ratio", type=float, default=1.25)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("avse4_enhance_bench needs the GPU")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    items = synthetic_set(a.utterances, a.min_s, a.max_s)
    lengths = [d["noisy_audio"].shape[-1] for d in items]
    model = det_init_(avse4.AVSE4BaselineModule(num_channels=2), 0).to("cuda").eval()
    model.visual_frontend.use_channels_last()
    plans = {bs: avse4.plan_ragged_batches(lengths, bs, a.max_pad_ratio) for bs in map(int, a.batch_sizes.split(","))}

    def loop():
        for d in items:
            model.enhance(d)

    def batched(plan):
        for batch in plan:
            model.enhance_batch([items[i] for i in batch])

    arms = {"enhance_loop": loop, **{f"enhance_batch_{bs}": (lambda p=p: batched(p)) for bs, p in plans.items()}}
    for fn in arms.values():                                 # the untimed pass
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.repeats):
        for k, fn in arms.items():
            ms[k].append(_timed_ms(fn))
    rec = {"metric": "avse4_enhance_utterances_per_s", "unit": "utterances/s", "utterances": a.utterances,
           "seconds_of_audio": round(sum(lengths) / 16000, 1), "min_s": a.min_s, "max_s": a.max_s,
           "max_pad_ratio": a.max_pad_ratio, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "arms": {}}
    for k, v in ms.items():
        rec["arms"][k] = {"utterances_per_s": round(a.utterances / (min(v) * 1e-3), 2),
                          "ms_per_pass": [round(x, 1) for x in v]}
    for bs, p in plans.items():
        pad = sum(max(lengths[i] for i in b) * len(b) for b in p) / sum(lengths)
        rec["arms"][f"enhance_batch_{bs}"].update(batches=len(p), padded_over_useful=round(pad, 3))
    rec["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
