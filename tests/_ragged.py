"""What the tests/test_gpu_*_ragged.py files share: the error measure of tests/test_gpu_fullsize.py, the padded batch
and the settings every fixture starts from.  A helper module like tests/_dirty.py, not a conftest."""
import importlib.util
import os

import numpy as np
import torch

from oracle.losses_ref import si_sdr_db


def errors(est, ref, clean, time_first=False):
    """(RMS error, its bar, max |dSI-SDR| in dB) of test_gpu_fullsize.check_waveforms; time is the last axis, or the
    first of (T, n_spk) arrays with time_first."""
    est, ref, clean = (torch.as_tensor(np.asarray(a)).double() for a in (est, ref, clean))
    if time_first:
        est, ref, clean = est.T, ref.T, clean.T
    rms = float((est - ref).pow(2).mean().sqrt())
    bar = 1e-4 * max(1.0, float(ref.pow(2).mean().sqrt()))
    d = float((si_sdr_db(clean, est) - si_sdr_db(clean, ref)).abs().max())
    return rms, bar, d


def padded(mixes, fill, device="cuda"):
    """The 1-D tensors stacked into (len(mixes), longest) rows, `fill` past each one's end."""
    mix = torch.full((len(mixes), max(m.shape[0] for m in mixes)), fill)
    for b, m in enumerate(mixes):
        mix[b, :m.shape[0]] = m
    return mix.to(device)


def fp32_math():
    """No TF32 in the library GEMMs and convolutions, 16 host threads for the fp64 oracle."""
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    torch.set_num_threads(16)


def load_tool(name):
    """tools/<name>.py as a module."""
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location(name, os.path.join(here, "..", "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def check_separate_dir(model, mixes, clean, tmp_path):
    """tools/mamba_separate.py (separate_dir: all of main() behind the checkpoint load) on three mixtures: two files per
    mixture, each the peak-normalised separate_batch estimate of what the tool read (the PCM_16 mixture) to the PCM_16
    step; an existing output is left alone, a second run finds nothing to do, and with targets the csv holds one row
    per utterance and the avg row."""
    from avse_challenge_amd import ckpt_io
    tool = load_tool("mamba_separate")
    mix, out, s1, s2 = (str(tmp_path / d) for d in ("mix", "out", "s1", "s2"))
    for d in (mix, out, s1, s2):
        os.mkdir(d)
    for b, x in enumerate(mixes):
        ckpt_io.write_wav(os.path.join(mix, f"u{b}.wav"), x.numpy(), 8000)
        for k, d in enumerate((s1, s2)):
            ckpt_io.write_wav(os.path.join(d, f"u{b}.wav"), clean[b][:, k].numpy(), 8000)
    for k in (1, 2):                                                      # there already: not redone
        ckpt_io.write_wav(os.path.join(out, f"itemu2_source{k}hat.wav"), np.zeros(10), 8000)
    assert tool.separate_dir(model, mix, out, batch_size=2, target_dirs=[s1, s2]) == ["u0", "u1"]
    assert sorted(os.listdir(out)) == sorted([f"itemu{b}_source{k}hat.wav" for b in range(3) for k in (1, 2)] +
                                             ["test_results.csv"])
    assert ckpt_io.read_wav(os.path.join(out, "itemu2_source1hat.wav"))[0].shape == (10,)
    read = [tool.load_wav(os.path.join(mix, f"u{b}.wav"), 8000)[0] for b in (0, 1)]
    for b, est in enumerate(model.separate_batch(read, batch_size=2)):
        for k in (0, 1):
            wav, sr = ckpt_io.read_wav(os.path.join(out, f"itemu{b}_source{k + 1}hat.wav"))
            assert sr == 8000 and wav.shape == (mixes[b].shape[0],)
            assert float(np.abs(wav - est[:, k] / np.max(np.abs(est[:, k]))).max()) <= 1.5 / 32768
    rows = open(os.path.join(out, "test_results.csv")).read().strip().splitlines()
    assert rows[0] == "snt_id,si-snr,si-snr_i" and [r.split(",")[0] for r in rows[1:]] == ["u0", "u1", "avg"]
    assert all(np.isfinite(float(v)) for r in rows[1:] for v in r.split(",")[1:])
    assert tool.find_mixtures(mix, out, 2) == [] and tool.separate_dir(model, mix, out, batch_size=2) == []
