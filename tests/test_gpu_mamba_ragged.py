"""Length-aware batched separation of a ragged Mamba-TasNet batch (MambaTasNet.forward_ragged, separate_batch,
BiMambaV2.forward_ragged; tools/mamba_separate.py) against the fp64 oracle on each utterance alone.

Reduced model (N = 64, kernel 16, 3 BiMamba blocks, 2 speakers), det_init_ seed 91, eval.  Three mixtures
0.1 det_input((t,), 6100 + b) of T = (4000, 2307, 3000) samples: (499, 287, 374) encoder frames, and 3 samples lie past
the last frame of utterance 1.  The bar is that of tests/test_gpu_fullsize.py: waveform RMS <= 1e-4 max(1, RMS(ref)) and
|dSI-SDR| <= 0.01 dB against 0.1 det_input((t, 2), 6120 + b) as the clean signals.  On the CPU the oracle run on the
zero-padded batch misses that bar by 19x (2307 samples) and 43x (3000 samples): the time-reversed direction of every
BiMamba block starts in the padding, and the padded encoder frame past an utterance's last one is overlap-added into
its last hop samples.  The oracle runs once (module fixture); all GPU work allocates dirty."""
import functools

import numpy as np
import pytest
import torch

import _dirty
import _ragged
from _ragged import padded
from oracle import mamba_ref
from oracle.det_init import det_init_, det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
KW = dict(N=64, kernel_size=16, n_mamba=3, n_spk=2)
T_LEN = (4000, 2307, 3000)
K_LEN = tuple((t - 16) // 8 + 1 for t in T_LEN)


errors = functools.partial(_ragged.errors, time_first=True)               # all (T, n_spk)


@pytest.fixture(scope="module")
def case():
    from avse_challenge_amd import mamba_tasnet as M
    _ragged.fp32_math()
    mixes = [0.1 * det_input((t,), 6100 + b) for b, t in enumerate(T_LEN)]
    clean = [0.1 * det_input((t, 2), 6120 + b) for b, t in enumerate(T_LEN)]
    m = det_init_(M.MambaTasNet(**KW), 91).to(DEV).eval()
    r = det_init_(mamba_ref.MambaTasNet(**KW), 91).double().eval()
    with torch.no_grad():
        refs = [r(x[None].double())[0].numpy() for x in mixes]          # the oracle on each utterance alone, fp64
    mp = pytest.MonkeyPatch()
    with _dirty.dirty(mp):
        out = m.forward_ragged(padded(mixes, 0.0), T_LEN)
    return dict(m=m, mixes=mixes, clean=clean, refs=refs, out=out)


def test_a_each_row_matches_the_oracle_on_the_utterance_alone(case):
    assert K_LEN == (499, 287, 374) and case["out"].shape == (3, 4000, 2)
    for b, t in enumerate(T_LEN):
        rms, bar, dsdr = errors(case["out"][b, :t].cpu(), case["refs"][b], case["clean"][b])
        print(f"\nutterance {b}: RMS error {rms:.2e} (bar {bar:.1e}), |dSI-SDR| {dsdr:.2e} dB")
        assert rms <= bar, f"utterance {b}: RMS waveform error {rms:.3e} > {bar:.1e}"
        assert dsdr <= 0.01, f"utterance {b}: SI-SDR differs by {dsdr:.4f} dB"


def test_b_what_the_padding_holds_is_not_used(case, monkeypatch):
    with _dirty.dirty(monkeypatch):
        got = case["m"].forward_ragged(padded(case["mixes"], float("nan")), torch.tensor(T_LEN))
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, case["out"])


def test_c_the_tail_is_the_reference_pad(case):
    assert [t - (8 * (k - 1) + 16) for t, k in zip(T_LEN, K_LEN)] == [0, 3, 0]
    for b, (t, k) in enumerate(zip(T_LEN, K_LEN)):
        row, end = case["out"][b], 8 * (k - 1) + 16
        assert not bool(row[end:].any()) and not bool(row[t:].any())
        assert bool(row[end - 8:end].any(dim=0).all())                  # the last frame's own hop is there
        assert not case["refs"][b][end:].any()                           # ... and alone the same samples are 0


def test_d_zero_padding_alone_misses_the_bar(case):
    """Negative control: the dense forward on the zero-padded batch misses bar (a) for the two shorter utterances, so
    (a) cannot pass by accident of the inputs."""
    with torch.no_grad():
        est = case["m"](padded(case["mixes"], 0.0))
    for b in (1, 2):
        rms, bar, dsdr = errors(est[b, :T_LEN[b]].cpu(), case["refs"][b], case["clean"][b])
        print(f"\ndense forward on the padded batch, utterance {b}: RMS {rms:.2e} (bar {bar:.1e}), |dSI-SDR| {dsdr:.2e} dB")
        assert not (rms <= bar and dsdr <= 0.01)


def test_e_separate_batch_returns_the_rows_in_input_order(case, monkeypatch):
    m = case["m"]
    with _dirty.dirty(monkeypatch):
        got = m.separate_batch([case["mixes"][0], case["mixes"][1].numpy(), case["mixes"][2]], batch_size=2)
    assert len(got) == 3
    for b, (t, est) in enumerate(zip(T_LEN, got)):
        assert est.shape == (t, 2) and est.dtype == np.float32
        rms, bar, dsdr = errors(est, case["refs"][b], case["clean"][b])
        print(f"\nseparate_batch, utterance {b}: RMS {rms:.2e} (bar {bar:.1e}), |dSI-SDR| {dsdr:.2e} dB")
        assert rms <= bar and dsdr <= 0.01, (b, rms, bar, dsdr)
        with torch.no_grad():
            alone = m(case["mixes"][b][None].to(DEV))[0].cpu()
        rms, bar, dsdr = errors(est, alone, case["clean"][b])
        print(f"  vs model(mix[None]): RMS {rms:.2e} (bar {bar:.1e}), |dSI-SDR| {dsdr:.2e} dB")
        assert rms <= bar and dsdr <= 0.01, (b, rms, bar, dsdr)
    with pytest.raises(ValueError):
        m.forward_ragged(padded(case["mixes"], 0.0), (4000, 15, 3000))   # shorter than one encoder window


def test_f_causal_model(case, monkeypatch):
    """bidirectional=False: the dense causal kernels never look ahead into the padding; only the input and decoder
    masking is new.  Against the model's own batch-1 forward."""
    from avse_challenge_amd import mamba_tasnet as M
    m = det_init_(M.MambaTasNet(N=64, kernel_size=16, n_mamba=2, n_spk=2, bidirectional=False), 92).to(DEV).eval()
    with _dirty.dirty(monkeypatch):
        got = m.forward_ragged(padded(case["mixes"], float("nan")), T_LEN)
    assert bool(torch.isfinite(got).all())
    for b, t in enumerate(T_LEN):
        with torch.no_grad():
            alone = m(case["mixes"][b][None].to(DEV))[0].cpu()
        rms, bar, dsdr = errors(got[b, :t].cpu(), alone, case["clean"][b])
        print(f"\ncausal, utterance {b}: RMS {rms:.2e} (bar {bar:.1e}), |dSI-SDR| {dsdr:.2e} dB")
        assert rms <= bar and dsdr <= 0.01, (b, rms, bar, dsdr)
        assert not bool(got[b, 8 * (K_LEN[b] - 1) + 16:].any())


def test_g_the_tool_separates_a_directory(case, tmp_path):
    """tools/mamba_separate.py (separate_dir: all of main() behind the checkpoint load) on the three mixtures: two
    files per mixture, each the peak-normalised separate_batch estimate of what the tool read (the PCM_16 mixture) to
    the PCM_16 step; an existing output is left alone, a second run finds nothing to do, and with targets the csv holds
    one row per utterance and the avg row."""
    _ragged.check_separate_dir(case["m"], case["mixes"], case["clean"], tmp_path)
