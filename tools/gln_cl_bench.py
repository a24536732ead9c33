"""Micro-benchmark of the channels-last GroupNorm(1, N) with per-row extents (kernels.gln_cl_fwd) at DPMamba-L's
dual-path shape, B = 16, S = 34, K = 250, N = 512 (HIP events, best of 3 x 20), next to dpmamba._gln_cl (the dense
forward's torch var_mean passes, plus the residual add / transposed add the kernel folds in) on the same tensor:

    intra: x (B, S, K, N), len_axis 0, res = the block input           y (B, S, K, N)
    inter: x (B, K, S, N), len_axis 1, res = intra, transpose_out      y (B, S, K, N)

Full rows (every chunk valid) and a ragged set of chunk counts.  frac = algorithmic bytes of the valid lines (x read once,
res read, y written: 12 B/element; the +0 stores of invalid lines are not counted) / time / 8 TB/s.  Prints one JSON
line; --out also writes it to a file."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avse_challenge_amd import kernels as K  # noqa: E402
from avse_challenge_amd.dpmamba import _gln_cl  # noqa: E402


def ev_ms(fn, n=20):
    fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / n
        best = ms if best is None else min(best, ms)
    return best


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="16,34,250,512", help="B,S,K,N")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("gln_cl_bench needs the GPU")
    B, S, Kc, N = (int(v) for v in a.shape.split(","))
    g = torch.Generator(device="cuda").manual_seed(0)
    x_intra = torch.randn(B, S, Kc, N, device="cuda", generator=g)
    x_inter = torch.randn(B, Kc, S, N, device="cuda", generator=g)
    res = torch.randn(B, S, Kc, N, device="cuda", generator=g)
    gm = torch.rand(N, device="cuda", generator=g) + 0.5
    bt = torch.randn(N, device="cuda", generator=g)
    full = torch.full((B,), S, dtype=torch.int32, device="cuda")
    ragged_host = [max(2, S - 2 * (b % 8)) for b in range(B)]
    ragged = torch.tensor(ragged_host, dtype=torch.int32, device="cuda")
    out = {"shape": [B, S, Kc, N], "device": torch.cuda.get_device_name(0), "ragged_chunks": ragged_host}
    arms = (("intra_full", lambda: K.gln_cl_fwd(x_intra, gm, bt, 1e-8, full, 0, res=res), B * S),
            ("inter_full", lambda: K.gln_cl_fwd(x_inter, gm, bt, 1e-8, full, 1, res=res, transpose_out=True), B * S),
            ("intra_ragged", lambda: K.gln_cl_fwd(x_intra, gm, bt, 1e-8, ragged, 0, res=res), sum(ragged_host)),
            ("inter_ragged", lambda: K.gln_cl_fwd(x_inter, gm, bt, 1e-8, ragged, 1, res=res, transpose_out=True),
             sum(ragged_host)),
            ("torch_intra_dense", lambda: _gln_cl(x_intra, gm, bt, 1e-8) + res, B * S),
            ("torch_inter_dense", lambda: res + _gln_cl(x_inter, gm, bt, 1e-8).transpose(1, 2), B * S))
    for name, fn, chunks in arms:
        ms = ev_ms(fn)
        out[name] = {"ms": round(ms, 4), "frac_of_8TBps": round(12 * chunks * Kc * N / (ms * 1e-3) / 8e12, 4)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
