"""What the ragged-batch benches share (avse4_enhance_bench.py, mamba_separate_bench.py, avse1_enhance.py --bench): a
loop of one utterance per forward against the batched call on ragged.plan_ragged_batches at several batch sizes, same
build, same process.  Every arm gets one untimed pass over the whole set (allocator, code objects), then `repeats` timed
passes between two device events, the arms alternating within a repeat; host-side padding, the upload and the download
are inside the timed span for both arms, as a tool run pays them.  One JSON line comes out."""
import json
import os

import torch

from avse_challenge_amd.ragged import plan_ragged_batches


def add_args(ap, repeats, out_help="also write the line to this file"):
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--min-s", type=float, default=3.0)
    ap.add_argument("--max-s", type=float, default=9.0)
    ap.add_argument("--batch-sizes", default="4,16,32")
    ap.add_argument("--repeats", type=int, default=repeats)
    ap.add_argument("--out", default=None, help=out_help)


def _timed_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def padded_over_useful(lengths, plan):
    return sum(max(lengths[i] for i in b) * len(b) for b in plan) / sum(lengths)


def run(a, header, lengths, sample_rate, loop_name, loop, batched_name, batched, extra=()):
    """Times loop() and batched(batch_size, plan) for each of a.batch_sizes over the set whose per-item sample counts
    are `lengths`, and prints (and writes to a.out) the record: header (metric, unit, model), the set and the settings
    (a: the parsed add_args flags and max_pad_ratio), extra, the device, the arms (utterances_per_s of the fastest pass,
    ms_per_pass; batches and padded_over_useful for the batched ones) and max_mem_gb."""
    plans = {bs: plan_ragged_batches(lengths, bs, a.max_pad_ratio) for bs in map(int, a.batch_sizes.split(","))}
    arms = {loop_name: loop, **{f"{batched_name}_{bs}": (lambda bs=bs, p=p: batched(bs, p)) for bs, p in plans.items()}}
    for fn in arms.values():                                 # the untimed pass
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.repeats):
        for k, fn in arms.items():
            ms[k].append(_timed_ms(fn))
    rec = {**header, "utterances": len(lengths), "seconds_of_audio": round(sum(lengths) / sample_rate, 1),
           "min_s": a.min_s, "max_s": a.max_s, "max_pad_ratio": a.max_pad_ratio, "repeats": a.repeats, **dict(extra),
           "device": torch.cuda.get_device_name(0), "arms": {}}
    for k, v in ms.items():
        rec["arms"][k] = {"utterances_per_s": round(len(lengths) / (min(v) * 1e-3), 2),
                          "ms_per_pass": [round(x, 1) for x in v]}
    for bs, p in plans.items():
        rec["arms"][f"{batched_name}_{bs}"].update(batches=len(p),
                                                   padded_over_useful=round(padded_over_useful(lengths, p), 3))
    rec["max_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
