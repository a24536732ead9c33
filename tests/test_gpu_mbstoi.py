"""MBSTOI on the GPU (avse_challenge_amd/metrics.py, csrc/mbstoi.hip) against the goldens recorded from the reference
(tests/golden/mbstoi.npz, made by make_golden_mbstoi.py) and against the test-side restatement (tests/mbstoi_ref.py).

The bar of a case is 1024 x ref_spread, ref_spread = max |d_restatement - d_reference| of that case from the manifest:
the restatement differs from the reference by summation order alone, on the same FFT; the GPU adds another FFT
algorithm (own radix-4 kernel, rocFFT for the 9600- and 6001-point resampling transforms, against pocketfft), another
summation order and the cancellation of the centred sums.  The bar stays below 0.01 x min_gap (the smallest relative
distance between the best and the second-best p of any cell), so a flipped grid winner cannot pass.  d, p_ec_max and the
score are held to it in absolute terms (|d| <= 1; p = exx / eyy is of order 1, at most 2.3 in the goldens); the band
quantities to bar_rel = 1024 x max(the restatement's own relative spread of them, 2^-52), relative
to each quantity's largest magnitude in its band.  No cell is left out.

Measured on an MI355X (max |GPU - golden|): see DESIGN.md, section 4, MBSTOI.
"""
import csv
import functools
import json
import os

import numpy as np
import pytest
import torch

import _dirty
import mbstoi_ref as R
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR = 1024
SIGNAL_CASES = ("A", "B", "C", "D3", "F")


@functools.lru_cache(maxsize=None)
def manifest():
    with open(os.path.join(GOLDEN, "manifest_mbstoi.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def gold():
    g = load_golden("mbstoi")
    g.update(load_golden("mbstoi_sig"))
    g["F.clean"], g["F.processed"], g["F.sig"] = g["A.clean"], g["A.processed"], g["A.sig"]
    g["C.sig"] = np.concatenate([g["C.clean"], g["C.processed"]]).astype(np.float64)
    return g


def bar(case):
    return FACTOR * manifest()[case]["ref_spread"]


def bar_rel(case):
    return FACTOR * max(manifest()[case]["ref_spread_bq_rel"], 2.0 ** -52)


def M():
    from avse_challenge_amd import metrics
    return metrics


def _inputs(case):
    g = gold()
    return torch.from_numpy(g[case + ".clean"])[None].to(DEV), torch.from_numpy(g[case + ".processed"])[None].to(DEV)


def _cpu(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def run(case):
    """One utterance of a golden case through the public entry point, intermediates on the host (computed once)."""
    m = manifest()[case]
    clean, proc = _inputs(case)
    return _cpu(M().mbstoi(clean, proc, sr=m["sr"], gridcoarseness=m["gridcoarseness"], return_intermediates=True))


@pytest.mark.parametrize("case", SIGNAL_CASES + ("E",))
def test_bar_cannot_pass_a_flipped_winner(case):
    m = manifest()[case]
    assert 0 < bar(case) < 0.01 * m["min_gap"], (bar(case), m["min_gap"])
    if case != "E":
        assert m["threshold_margin_db"] > 1.0        # no frame energy near the 40 dB gate: K is not a coin toss


@pytest.mark.parametrize("case", SIGNAL_CASES)
def test_case_vs_golden(case):
    g, m, r = gold(), manifest()[case], run(case)
    K = int(r["K"][0])
    frames = R.n_frames(int(r["lengths10k"][0]))
    assert frames == m["frames"] and int(r["lengths10k"][0]) == g[case + ".sig"].shape[1]
    assert K == m["K"] and r["kept"].shape == (1, frames)
    assert np.array_equal(r["kept"][0, :K], g[case + ".kept"]) and np.all(r["kept"][0, K:] == -1)
    sig_err = float(np.abs(r["sig"][0] - g[case + ".sig"]).max() / np.abs(g[case + ".sig"]).max())
    bq, want = r["bq"][0, :K - 1], g[case + ".bq"]
    assert bq.shape == want.shape and not np.any(r["bq"][0, K - 1:])
    scale = np.abs(want).max(axis=0)                               # (15, 8): per band and quantity
    bq_err = float((np.abs(bq - want).max(axis=0) / scale).max())
    S = m["segments"]
    assert r["d"].shape == (1, 15, frames - 1 - 29) and S == K - 1 - 29
    errs = {k: float(np.abs(r[k][0, :, :S] - g[f"{case}.{k}"]).max()) for k in ("d_ec", "d", "p_ec")}
    errs["score"] = abs(float(r["score"][0]) - float(g[case + ".score"]))
    print(f"\nmbstoi {case}: resample rel {sig_err:.2e}  bq rel {bq_err:.2e} (bar_rel {bar_rel(case):.2e})  "
          + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f"  (bar {bar(case):.2e})")
    assert bq_err <= bar_rel(case)
    for k, v in errs.items():
        assert v <= bar(case), (k, v, bar(case))
    for k in ("d", "d_ec", "p_ec"):
        assert not np.any(r[k][0, :, S:])                         # outside the utterance's own segments: zeros
    assert np.all(r["winner"][0, :, S:] == -1)


@pytest.mark.parametrize("case", ("A", "B", "F"))
def test_winner_is_the_first_maximum(case):
    """The flat winner index (tau * n_gammas + gamma) is the one numpy's order picks on the GPU's own band quantities,
    p_ec_max is the grid's value there, and -1 marks exactly the cells of the `-1` rule."""
    m, r = manifest()[case], run(case)
    K = int(r["K"][0])
    own = R.ec_better_ear(r["bq"][0, :K - 1], m["gridcoarseness"])
    S = m["segments"]
    assert np.array_equal(r["winner"][0, :, :S], own["winner"])
    assert float(np.abs(r["p_ec"][0, :, :S] - own["p_ec"]).max()) <= bar(case)
    fired = r["winner"][0, :, :S] == -1
    assert np.array_equal(fired, r["d_ec"][0, :, :S] == -1.0) and np.all(r["p_ec"][0, :, :S][fired] == 0.0)
    n_taus, n_gammas = -(-100 // m["gridcoarseness"]), -(-40 // m["gridcoarseness"])
    assert int(r["winner"].max()) < n_taus * n_gammas


def test_ec_level_minus_one_rule():
    """Case E: band 5 exactly zero over segment 3 gives d = -1 exactly there (NaN better-ear ratios do not replace it);
    every cell within the bar."""
    g, m = gold(), manifest()["E"]
    bq = torch.from_numpy(g["E.bq"])[None].to(DEV)
    r = _cpu(M().ec_stage(bq, return_intermediates=True))
    assert r["d"][0, 5, 3] == -1.0 and r["d_ec"][0, 5, 3] == -1.0 and r["p_ec"][0, 5, 3] == 0.0
    assert r["winner"][0, 5, 3] == -1 and int((r["d"] == -1.0).sum()) == m["minus_one_cells"]
    errs = {k: float(np.abs(r[k][0] - g["E." + k]).max()) for k in ("d_ec", "d", "p_ec")}
    errs["score"] = abs(float(r["score"][0]) - float(g["E.score"]))
    print(f"\nmbstoi E: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f"  (bar {bar('E'):.2e})")
    assert int((r["d"][0] != r["d_ec"][0]).sum()) == m["better_ear_cells"]
    for k, v in errs.items():
        assert v <= bar("E"), (k, v, bar("E"))


def _batch_d(dtype=torch.float32):
    g = gold()
    names = ("A", "B", "D3")
    lengths = [g[n + ".clean"].shape[1] for n in names]
    clean = torch.zeros((3, 2, max(lengths)), dtype=dtype)
    proc = torch.full((3, 2, max(lengths)), 0.25, dtype=dtype)           # the padding must not matter
    for i, n in enumerate(names):
        clean[i, :, :lengths[i]] = torch.from_numpy(g[n + ".clean"])
        proc[i, :, :lengths[i]] = torch.from_numpy(g[n + ".processed"])
    return names, lengths, clean.to(DEV), proc.to(DEV)


def _same_valid(batch, i, single, K, what):
    F = int(single["kept"].shape[1])
    S = max(K - 30, 0)
    assert int(batch["K"][i]) == K
    assert np.array_equal(batch["kept"][i, :F], single["kept"][0]) and np.all(batch["kept"][i, F:] == -1), what
    assert np.array_equal(batch["bq"][i, :K - 1], single["bq"][0, :K - 1]) and not np.any(batch["bq"][i, K - 1:]), what
    for k in ("d", "d_ec", "p_ec", "winner"):
        assert np.array_equal(batch[k][i, :, :S], single[k][0, :, :S]), (what, k)
    assert batch["score"][i].tobytes() == single["score"][0].tobytes(), what


def test_padded_batch_bitwise_equals_single_runs():
    """Case D: A, B and D3 padded into one batch with `lengths` give the bits of the three single-utterance runs."""
    names, lengths, clean, proc = _batch_d()
    batch = _cpu(M().mbstoi(clean, proc, sr=16000, lengths=lengths, return_intermediates=True))
    for i, n in enumerate(names):
        _same_valid(batch, i, run(n), manifest()[n]["K"], n)
        assert abs(float(batch["score"][i]) - float(gold()[n + ".score"])) <= bar(n)
    plain = M().mbstoi(clean, proc, sr=16000, lengths=torch.tensor(lengths))
    assert plain.dtype == torch.float64 and plain.is_cuda and np.array_equal(plain.cpu().numpy(), batch["score"])


def test_two_runs_bitwise_equal():
    clean, proc = _inputs("B")
    a = _cpu(M().mbstoi(clean, proc, return_intermediates=True))
    b = run("B")
    for k in a:
        if k != "sig":
            assert np.array_equal(a[k], b[k], equal_nan=True), k
    n = int(a["lengths10k"][0])
    assert np.array_equal(a["sig"][..., :n], b["sig"][..., :n])


def test_dirty_memory_gives_the_bits_of_a_clean_run(monkeypatch):
    """As tests/test_gpu_dirty_memory.py does for the other wrappers: every torch.empty of metrics.py poisoned (the
    16-bit pattern 0x7FC0: 2.3e307 as fp64, a large int32), same inputs; every output but the undefined tails of `sig`
    bit-equal and NaN-free."""
    names, lengths, clean, proc = _batch_d()
    metrics = M()

    def once():
        return _cpu(metrics.mbstoi(clean, proc, sr=16000, lengths=lengths, return_intermediates=True))
    want = once()
    with monkeypatch.context() as mp:
        mp.setattr(metrics, "torch", _dirty.PoisonTorch(torch))
        probe = metrics.torch.empty(3, device=DEV, dtype=torch.float64)
        assert bool((probe.view(torch.int16) == _dirty.POISON16).all()) and float(probe[0]) > 1e307
        got = once()
    assert metrics.torch is torch
    for k in want:
        if k == "sig":
            for i, n in enumerate(want["lengths10k"]):
                assert np.array_equal(want[k][i, :, :n], got[k][i, :, :n])
        else:
            assert not (got[k].dtype.kind == "f" and np.isnan(got[k]).any()), k
            assert np.array_equal(want[k], got[k]), k


def test_fewer_than_30_frames_is_nan():
    """18 frames (4000 samples at 16 kHz) cannot fill one segment: NaN, alone and beside a scored utterance."""
    g = gold()
    clean, proc = _inputs("A")
    short = M().mbstoi(clean[..., :4000], proc[..., :4000])
    assert short.shape == (1,) and bool(torch.isnan(short).all())
    tiny = M().mbstoi(clean[..., :300], proc[..., :300])                  # not even one frame at 10 kHz
    assert bool(torch.isnan(tiny).all())
    both = M().mbstoi(torch.cat([clean, clean]), torch.cat([proc, proc]), lengths=[9600, 4000]).cpu().numpy()
    assert np.isnan(both[1]) and both[0].tobytes() == run("A")["score"][0].tobytes()
    assert abs(both[0] - float(g["A.score"])) <= bar("A")


def test_random_shape_vs_restatement():
    """An odd length with a quiet stretch (frames removed), float64 input, against tests/mbstoi_ref.py on this
    machine's CPU.  Bar: 1024 x the largest ref_spread of the manifest (the restatement's distance from the
    reference), and below 0.01 x this input's own smallest top-2 gap."""
    rng = np.random.default_rng(77)
    T = 11003
    src = np.convolve(rng.standard_normal(T + 8), np.hanning(7) / 3.0, mode="same") * (
        0.3 + np.abs(np.sin(np.arange(T + 8) / 900.0)))
    clean = np.stack([src[6:6 + T], 0.5 * src[2:2 + T]]) * 0.1
    proc = clean + 0.02 * rng.standard_normal((2, T))
    clean[:, 3000:4300] *= 1e-4
    proc[:, 3000:4300] *= 1e-4
    want = R.mbstoi(clean, proc, 16000)
    b = FACTOR * max(v["ref_spread"] for k, v in manifest().items() if not k.startswith("_"))
    assert b < 0.01 * float(want["gap"].min())
    e = want["energies"]
    assert float(np.abs(e.max(axis=1, keepdims=True) - 40.0 - e).min()) > 1.0 and want["K"] < e.shape[1]
    r = _cpu(M().mbstoi(torch.from_numpy(clean)[None].to(DEV), torch.from_numpy(proc)[None].to(DEV),
                        return_intermediates=True))
    K = want["K"]
    assert int(r["K"][0]) == K and np.array_equal(r["kept"][0, :K], want["kept"])
    S = K - 30
    err = {k: float(np.abs(r[k][0, :, :S] - want[k]).max()) for k in ("d", "d_ec", "p_ec")}
    err["score"] = abs(float(r["score"][0]) - want["score"])
    print(f"\nmbstoi random 11003: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()) + f"  (bar {b:.2e})")
    assert np.array_equal(r["winner"][0, :, :S], want["winner"])
    for k, v in err.items():
        assert v <= b, (k, v, b)


def test_module_mbstoi_equals_metric_of_its_own_forward():
    from avse_challenge_amd import avse4
    from oracle.det_init import det_init_, det_input
    kw = dict(N=64, L=40, B=64, H=128, P=3, X=3, R=2, C=2)
    m = det_init_(avse4.AVSE4BaselineModule(num_channels=2, **kw), 61).to(DEV).eval()
    batch = {"noisy_audio": 0.1 * det_input((2, 2, 9600), 911), "vis_feat": det_input((2, 1, 15, 112, 112), 912, "uniform"),
             "clean": 0.1 * det_input((2, 2, 9600), 913)}
    batch = {k: v.to(DEV) for k, v in batch.items()}
    seen = []                      # the forward inside m.mbstoi itself (a second forward need not repeat its bits)
    hook = m.register_forward_hook(lambda mod, args, out: seen.append(out))
    got = m.mbstoi(batch)
    hook.remove()
    assert len(seen) == 1 and seen[0].shape == (2, 2, 9600) and not seen[0].requires_grad
    est = seen[0] / seen[0].abs().amax(dim=(1, 2), keepdim=True)
    assert float(est.abs().amax()) == 1.0
    want = M().mbstoi(batch["clean"], est, sr=16000)
    assert got.shape == (2,) and got.dtype == torch.float64 and torch.equal(got, want)
    assert bool(torch.isfinite(got).all()) and not any(p.grad is not None for p in m.parameters())


def test_eval_tool_writes_the_csv(tmp_path):
    """tools/mbstoi_eval.py on two temporary scenes (and one with a missing file): rows, order, values."""
    import importlib.util
    from avse_challenge_amd import ckpt_io
    spec = importlib.util.spec_from_file_location(
        "mbstoi_eval", os.path.join(os.path.dirname(GOLDEN), os.pardir, "tools", "mbstoi_eval.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    g = gold()
    enh, tgt = tmp_path / "enh", tmp_path / "tgt"
    enh.mkdir()
    tgt.mkdir()
    scenes = [{"scene": "S00002"}, {"scene": "S00009"}, {"scene": "S00001"}]
    for name, case in (("S00002", "B"), ("S00001", "A")):
        ckpt_io.write_wav(str(tgt / f"{name}_target_anechoic.wav"), g[case + ".clean"].T, 16000, subtype="FLOAT")
        ckpt_io.write_wav(str(enh / f"{name}_mix.wav"), g[case + ".processed"].T, 16000, subtype="FLOAT")
    ckpt_io.write_wav(str(tgt / "S00009_target_anechoic.wav"), g["A.clean"].T, 16000, subtype="FLOAT")
    with open(tmp_path / "scenes.json", "w") as f:
        json.dump(scenes, f)
    tool.main(["--scenes", str(tmp_path / "scenes.json"), "--enhanced", str(enh), "--target", str(tgt),
               "--results", str(tmp_path / "out")])
    with open(tmp_path / "out" / "objective_metrics.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["scene", "mbstoi"] and [r[0] for r in rows[1:]] == ["S00002", "S00001"]
    assert abs(float(rows[1][1]) - float(g["B.score"])) <= bar("B")
    assert abs(float(rows[2][1]) - float(g["A.score"])) <= bar("A")
    ckpt_io.write_wav(str(enh / "S00009_mix.wav"), g["A.processed"][:, :9000].T, 16000, subtype="FLOAT")
    with pytest.raises(Exception, match="same length"):
        tool.evaluate(scenes, str(enh), str(tgt))
