"""Streaming-inference bench of the causal Mamba-TasNet (StreamingSeparator) on the MI355X.

    python tools/stream_bench.py [--sizes S,L] [--batches 1,16] [--frames 1,8,32,128] [--seconds 1.0] [--out FILE]

Per configuration (size, fp32 / bf16 autocast, batch, frames per push): ms per push by device events after warm-up
over at least --seconds of pushes, the real-time factor (one frame = hop samples at 8 kHz = 1 ms of audio; RTF =
compute time / audio time, below 1 keeps up), the kernel launches per push (counted by torch's profiler on one push) and
the bytes a push must move, computed from shapes.  It also times l single-frame step calls against one l-frame chunk
call of one mixer.  GPU only: without a device the measurement fails, it does not fall back.  One JSON line per
configuration on stdout (and in --out); a markdown table at the end.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avse_challenge_amd import mamba_tasnet as M  # noqa: E402

SAMPLE_RATE = 8000


def push_bytes(model, batch, frames, act_bytes):
    """Bytes one push must move at the least, from shapes: every weight once (fp32 masters; bf16 autocast re-casts
    them per call, not counted), the layers' states read and written once, and the activations of the push at one read
    and one write per tensor between kernels (xz, conv_out, x_dbl, delta, out_z, the block output and residual)."""
    weights = 4 * sum(p.numel() for p in model.parameters())
    mix = model.masknet.mamba_net.layers[0].mixer
    di, dm, r, n, w = mix.d_inner, mix.d_model, mix.dt_rank, mix.d_state, mix.d_conv
    n_layers = len(model.masknet.mamba_net.layers)
    states = 2 * batch * n_layers * (di * n * 4 + di * w * act_bytes)
    per_frame_layer = act_bytes * (2 * di + di + (r + 2 * n) + di + di + dm) + 4 * 2 * dm      # + fp32 residual
    N, S = model.encoder.conv1d.out_channels, model.num_spks
    per_frame_io = 4 * (model.encoder.conv1d.kernel_size[0] + 2 * N + 2 * S * N + S * model.encoder.conv1d.kernel_size[0])
    acts = 2 * batch * frames * (n_layers * per_frame_layer + per_frame_io)
    return {"weights": weights, "states": states, "activations": acts, "total": weights + states + acts}


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def time_pushes(fn, seconds, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(10, int(seconds / max(time.perf_counter() - t0, 1e-5)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, reps


def bench_config(size, autocast, batch, frames, seconds):
    torch.manual_seed(0)
    model = M.MambaTasNet(**M.MAMBA_TASNET_SIZES[size], bidirectional=False).cuda().eval()
    hop = model.encoder.conv1d.stride[0]
    sep = M.StreamingSeparator(model, batch)
    chunk = 0.1 * torch.randn(batch, frames * hop, device="cuda")
    ctx = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if autocast else (lambda: torch.autocast("cuda", enabled=False))

    def push():
        with ctx():
            return sep.push(chunk)

    push()                                            # the first push (one frame fewer, zero state) is not timed
    ms, reps = time_pushes(push, seconds)
    launches = count_launches(push)
    by = push_bytes(model, batch, frames, 2 if autocast else 4)
    audio_ms = frames * hop / SAMPLE_RATE * 1e3
    return {"size": size, "dtype": "bf16" if autocast else "fp32", "batch": batch, "frames": frames,
            "ms_per_push": round(ms, 4), "pushes_timed": reps, "audio_ms_per_push": audio_ms,
            "rtf": round(ms / audio_ms, 4), "launches_per_push": launches,
            "us_per_launch": round(1e3 * ms / max(launches, 1), 2), "bytes_per_push": by,
            "gbytes_per_s": round(by["total"] / (ms * 1e-3) / 1e9, 2)}


def bench_step_vs_chunk(size, batch, l, seconds):
    """l single-frame step() calls against one l-frame chunk call of one mixer (fp32), both from a warm state"""
    torch.manual_seed(0)
    dm = M.MAMBA_TASNET_SIZES[size]["N"]
    mix = M.Mamba(dm, layer_idx=0).cuda().eval()
    h = torch.randn(batch, l, dm, device="cuda")
    params = M.InferenceParams()
    mix(h, inference_params=params)
    params.seqlen_offset = l
    conv, ssm = params.key_value_memory_dict[0]

    def steps():
        for t in range(l):
            mix.step(h[:, t:t + 1], conv, ssm)

    def chunk():
        mix(h, inference_params=params)

    ms_steps, _ = time_pushes(steps, seconds / 2)
    ms_chunk, _ = time_pushes(chunk, seconds / 2)
    return {"size": size, "batch": batch, "frames": l, "ms_steps": round(ms_steps, 4), "ms_chunk": round(ms_chunk, 4),
            "launches_steps": count_launches(steps), "launches_chunk": count_launches(chunk)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="S,L")
    p.add_argument("--batches", default="1,16")
    p.add_argument("--frames", default="1,8,32,128")
    p.add_argument("--seconds", type=float, default=1.0)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench measures on the GPU; no device found")
    rows, svc = [], []
    out = open(a.out, "w") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for size in a.sizes.split(","):
        for autocast in (False, True):
            for batch in map(int, a.batches.split(",")):
                for frames in map(int, a.frames.split(",")):
                    rows.append(bench_config(size, autocast, batch, frames, a.seconds))
                    emit(rows[-1])
        for batch in map(int, a.batches.split(",")):
            for l in (8, 32, 128):
                svc.append(bench_step_vs_chunk(size, batch, l, a.seconds))
                emit({"step_vs_chunk": svc[-1]})
    print("\n| size | dtype | B | frames/push | ms/push | RTF | launches/push | us/launch | MB/push | GB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['size']} | {r['dtype']} | {r['batch']} | {r['frames']} | {r['ms_per_push']:.3f} | {r['rtf']:.3f} | "
              f"{r['launches_per_push']} | {r['us_per_launch']:.1f} | {r['bytes_per_push']['total'] / 1e6:.1f} | "
              f"{r['gbytes_per_s']:.1f} |")
    print("\n| size | B | frames | l x step (ms) | one chunk (ms) | launches (steps / chunk) |")
    print("|---|---|---|---|---|---|")
    for r in svc:
        print(f"| {r['size']} | {r['batch']} | {r['frames']} | {r['ms_steps']:.3f} | {r['ms_chunk']:.3f} | "
              f"{r['launches_steps']} / {r['launches_chunk']} |")


if __name__ == "__main__":
    main()
