"""Isolated HIP-event timings of the input-gradient convolutions with and without the BatchNorm-backward epilogue
(csrc/bnact_cols.h) and of the BatchNorm backward with and without its reduction pass, at the avse1 C2 step's shapes.
One JSON line per site (median of --iters launches after --warmup), in the format of
profiles/r07_conv_epilogue_probe.jsonl.

python tools/bn_bwd_epilogue_probe.py [--iters 20 --warmup 5 --out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avse_challenge_amd import kernels as K  # noqa: E402

DEV = "cuda"


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def site(kind, shape, d, args):
    n, c, h, w = shape
    g = torch.Generator(device=DEV).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)                                 # noqa: E731
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)                           # noqa: E731
    x, gy = cl(rnd(*shape)), cl(rnd(*shape))
    gam, bet = 0.5 + torch.rand(c, device=DEV, generator=g), 0.1 * rnd(c)
    act = K.ACT_RELU if kind == "dconv" else K.ACT_PRELU
    alpha = None if kind == "dconv" else 0.1 + 0.3 * torch.rand(c, device=DEV, generator=g)
    _, stats = K.bnact_fwd(x, gam, bet, torch.zeros(c, device=DEV), torch.ones(c, device=DEV), True, 0.1, 1e-5, act,
                           alpha, q_out=True)
    if kind == "dconv":
        wt = 0.05 * rnd(64, 64, 5, 5)
        mb, mbd = (torch.empty(2, device=DEV, dtype=torch.int32) for _ in range(2))
        gq = K.split16(gy, mbd)
        _, wq_t = K.dconv_wprep2(wt, mb, mbd)
        plain = lambda: K.dconv_fwd(gy, wt, d, transposed=True, split=(gq, mbd), wq=wq_t)        # noqa: E731
        fused = lambda q: K.dconv_dgrad_bn(shape, d, (gq, mbd), wq_t, x, stats, gam, bet, act, q)  # noqa: E731
    else:
        wt = 0.05 * rnd(c, c, 3, 3)
        gs = K.split_q(gy)
        plain = lambda: K.sconv_fwd(gs, shape, wt, 1, transposed=True)                           # noqa: E731
        fused = lambda q: K.sconv_dgrad1_bn(gs, shape, wt, x, stats, gam, bet, act, alpha, q)    # noqa: E731
    rec = {"kernel": kind, "shape": list(shape) + [d]}
    rec["dgrad_ms"] = timed(plain, args.iters, args.warmup)
    rec["dgrad_epi_ms"] = timed(lambda: fused(False), args.iters, args.warmup)
    rec["dgrad_epi_max_ms"] = timed(lambda: fused(True), args.iters, args.warmup)
    dy = plain()
    for q in (False, True):
        _, rows, ws = fused(q)
        key = "_q" if q else ""
        rec["bn_bwd" + key + "_ms"] = timed(lambda: K.bnact_bwd(x, None, dy, stats, gam, bet, act, alpha, True, q_out=q),
                                            args.iters, args.warmup)
        rec["bn_bwd_rows" + key + "_ms"] = timed(
            lambda: K.bnact_bwd_rows(x, dy, stats, gam, bet, act, alpha, True, rows, ws, q_out=q), args.iters,
            args.warmup)
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    sites = [("dconv", (32, 64, 376, 257), d) for d in (2, 4, 8, 16)]
    sites += [("sconv", (2400, 64, 24, 24), 1), ("sconv", (2400, 128, 12, 12), 1), ("sconv", (2400, 256, 6, 6), 1),
              ("sconv", (2400, 512, 3, 3), 1)]
    lines = []
    for s in sites:
        lines.append(json.dumps(site(*s, args)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
