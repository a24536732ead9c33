"""Utterances/s of Mamba-TasNet or DPMamba separation over a ragged set: the loop of `model(mix[None])` (one utterance
per forward, as the reference's save_results scores WSJ0-mix) against `separate_batch` on ragged.plan_ragged_batches at
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
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools")]
import ragged_bench  # noqa: E402
from avse_challenge_amd import dpmamba, mamba_tasnet  # noqa: E402
from oracle.det_init import det_init_  # noqa: E402

SAMPLE_RATE = 8000
MODELS = {"mamba": ("Mamba-TasNet", mamba_tasnet.MambaTasNet, mamba_tasnet.MAMBA_TASNET_SIZES),
          "dpmamba": ("DPMamba", dpmamba.DPMambaTasNet, dpmamba.DPMAMBA_SIZES)}


def synthetic_set(n, min_s, max_s, seed=0):
    g = np.random.default_rng(seed)
    return [(0.1 * g.standard_normal(int(g.integers(int(min_s * SAMPLE_RATE), int(max_s * SAMPLE_RATE) + 1))))
            .astype(np.float32) for _ in range(n)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ragged_bench.add_args(ap, repeats=2)
    ap.add_argument("--max-pad-ratio", type=float, default=1.25)
    ap.add_argument("--model", default="mamba", choices=sorted(MODELS))
    ap.add_argument("--size", default="L", choices=sorted(mamba_tasnet.MAMBA_TASNET_SIZES))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mamba_separate_bench needs the GPU")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    mixes = synthetic_set(a.utterances, a.min_s, a.max_s)
    name, cls, table = MODELS[a.model]
    model = det_init_(cls(**table[a.size]), 0).to("cuda").eval()

    def loop():
        with torch.no_grad():
            for m in mixes:
                model(torch.from_numpy(m)[None].to("cuda"))[0].cpu().numpy()

    header = {"metric": "mamba_separate_utterances_per_s", "unit": "utterances/s", "model": f"{name}-{a.size}"}
    ragged_bench.run(a, header, [m.shape[0] for m in mixes], SAMPLE_RATE, "forward_loop", loop, "separate_batch",
                     lambda bs, plan: model.separate_batch(mixes, bs, a.max_pad_ratio))


if __name__ == "__main__":
    main()
