"""Utterances/s of Mamba-TasNet or DPMamba separation over a ragged set: the loop of `model(mix[None])` (one utterance
per forward, as the reference's save_results scores WSJ0-mix) against `separate_batch` on avse4.plan_ragged_batches at
several batch sizes, same build, same process.

    python tools/mamba_separate_bench.py [--utterances 64 --min-s 3 --max-s 9 --batch-sizes 4,16,32 --repeats 2] \\
        [--model mamba|dpmamba --size L --out profiles/mamba_separate_bench.json]

A seeded synthetic set (noise at 8 kHz, lengths uniform in [min-s, max-s]), Mamba-TasNet-L (or DPMamba-L: --model
dpmamba) with det_init_ weights in eval mode, fp32.  Every arm gets one untimed pass over the whole set (allocator,
code objects), then `repeats` timed passes between two device events; host-side padding, the upload and the download
are inside the timed span for both arms, as a tool run pays them.  Arms alternate within a repeat.  Prints one JSON
line.  A run without a GPU fails; nothing here falls back.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from avse_challenge_amd import avse4, dpmamba, mamba_tasnet  # noqa: E402
from oracle.det_init import det_init_  # noqa: E402

SAMPLE_RATE = 8000
MODELS = {"mamba": ("Mamba-TasNet", mamba_tasnet.MambaTasNet, mamba_tasnet.MAMBA_TASNET_SIZES),
          "dpmamba": ("DPMamba", dpmamba.DPMambaTasNet, dpmamba.DPMAMBA_SIZES)}


def synthetic_set(n, min_s, max_s, seed=0):
    g = np.random.default_rng(seed)
    return [(0.1 * g.standard_normal(int(g.integers(int(min_s * SAMPLE_RATE), int(max_s * SAMPLE_RATE) + 1))))
            .astype(np.float32) for _ in range(n)]


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
    ap.add_argument("--model", default="mamba", choices=sorted(MODELS))
    ap.add_argument("--size", default="L", choices=sorted(mamba_tasnet.MAMBA_TASNET_SIZES))
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mamba_separate_bench needs the GPU")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    mixes = synthetic_set(a.utterances, a.min_s, a.max_s)
    lengths = [m.shape[0] for m in mixes]
    name, cls, table = MODELS[a.model]
    model = det_init_(cls(**table[a.size]), 0).to("cuda").eval()
    sizes = [int(v) for v in a.batch_sizes.split(",")]
    plans = {bs: avse4.plan_ragged_batches(lengths, bs, a.max_pad_ratio) for bs in sizes}

    def loop():
        with torch.no_grad():
            for m in mixes:
                model(torch.from_numpy(m)[None].to("cuda"))[0].cpu().numpy()

    arms = {"forward_loop": loop,
            **{f"separate_batch_{bs}": (lambda bs=bs: model.separate_batch(mixes, bs, a.max_pad_ratio)) for bs in sizes}}
    for fn in arms.values():                                 # the untimed pass
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.repeats):
        for k, fn in arms.items():
            ms[k].append(_timed_ms(fn))
    rec = {"metric": "mamba_separate_utterances_per_s", "unit": "utterances/s", "model": f"{name}-{a.size}",
           "utterances": a.utterances, "seconds_of_audio": round(sum(lengths) / SAMPLE_RATE, 1), "min_s": a.min_s,
           "max_s": a.max_s, "max_pad_ratio": a.max_pad_ratio, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "arms": {}}
    for k, v in ms.items():
        rec["arms"][k] = {"utterances_per_s": round(a.utterances / (min(v) * 1e-3), 2),
                          "ms_per_pass": [round(x, 1) for x in v]}
    for bs, p in plans.items():
        pad = sum(max(lengths[i] for i in b) * len(b) for b in p) / sum(lengths)
        rec["arms"][f"separate_batch_{bs}"].update(batches=len(p), padded_over_useful=round(pad, 3))
    rec["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
