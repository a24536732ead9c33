"""Length-aware batched enhancement of a ragged avse4 batch (AVSE4BaselineModule.enhance_batch, Separator.forward_ragged,
VisualFrontend.forward_ragged) against the fp64 oracle on each utterance alone.

Reduced separator (N = B = 64, H = 128, X = 3: dilations 1, 2, 4, R = 2) with the full VisualFrontend (its ResNet
trunk channels-last, i.e. on csrc/sconv.hip as in the benchmark), det_init_, eval.  Three utterances:
    T = 16000 (K = 799) with 25 video frames (32 Tv = 800, cropped by one)
    T =  9215 (K = 459) with 14 video frames (32 Tv = 448 < K: padded); (T - 40) % 20 = 15, so the encoder frame
                        past its last one still overlaps 15 valid samples, and 15 samples follow its estimate's end
    T = 12000 (K = 599) with 20 video frames (32 Tv = 640 > K: cropped)
The bar is that of tests/test_gpu_fullsize.py: waveform RMS <= 1e-4 max(1, RMS(ref)) and |dSI-SDR| <= 0.01 dB, on the
peak-normalised estimates enhance returns.  The oracle runs once (module fixture); all GPU work allocates dirty."""
import numpy as np
import pytest
import torch

import _dirty
import _ragged
from _ragged import errors
from oracle import avse4_ref
from oracle.det_init import det_init_, det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
KW = dict(N=64, L=40, B=64, H=128, P=3, X=3, R=2, C=2)
T_LEN, TV_LEN = (16000, 9215, 12000), (25, 14, 20)
K_LEN = tuple((t - 40) // 20 + 1 for t in T_LEN)


def passes(est, ref, clean):
    rms, bar, d = errors(est, ref, clean)
    return rms <= bar and d <= 0.01


def padded_inputs(items, fill):
    audio = torch.full((3, 2, max(T_LEN)), fill)
    video = torch.full((3, 1, max(TV_LEN), 112, 112), fill)
    for b, d in enumerate(items):
        audio[b, :, :T_LEN[b]] = d["noisy_audio"]
        video[b, :, :TV_LEN[b]] = d["vis_feat"]
    return audio.to(DEV), video.to(DEV)


@pytest.fixture(scope="module")
def case():
    from avse_challenge_amd import avse4
    _ragged.fp32_math()
    items = [{"noisy_audio": 0.1 * det_input((2, t), 5100 + b),
              "vis_feat": det_input((1, tv, 112, 112), 5110 + b, "uniform"),
              "clean": 0.1 * det_input((2, t), 5120 + b)} for b, (t, tv) in enumerate(zip(T_LEN, TV_LEN))]
    m = det_init_(avse4.AVSE4BaselineModule(num_channels=2, **KW), 81).to(DEV).eval()
    m.visual_frontend.use_channels_last()
    r = det_init_(avse4_ref.AVSE4BaselineModule(num_channels=2, **KW), 81).double().eval()
    refs = []
    with torch.no_grad():
        for d in items:                                      # the oracle on each utterance alone, fp64 (model.py:335-352)
            e = r.model(d["noisy_audio"][None].double(), r.visual_frontend(d["vis_feat"][None].double()))[0]
            refs.append((e / e.abs().max()).numpy())
    mp = pytest.MonkeyPatch()
    with _dirty.dirty(mp):
        out = m.enhance_batch(items)
    return dict(m=m, items=items, refs=refs, out=out)


def test_a_each_estimate_matches_the_oracle_on_the_utterance_alone(case):
    for b, (d, ref, (_, _, est)) in enumerate(zip(case["items"], case["refs"], case["out"])):
        rms, bar, dsdr = errors(est, ref, d["clean"])
        print(f"\nutterance {b}: RMS error {rms:.2e} (bar {bar:.1e}), |dSI-SDR| {dsdr:.2e} dB")
        assert rms <= bar, f"utterance {b}: RMS waveform error {rms:.3e} > {bar:.1e}"
        assert dsdr <= 0.01, f"utterance {b}: SI-SDR differs by {dsdr:.4f} dB"


def test_b_what_the_padding_holds_is_not_used(case, monkeypatch):
    """NaN in the audio and video padding: bitwise the estimates of the zero-padded call, which are enhance_batch's."""
    m = case["m"]
    got = []
    for fill in (0.0, float("nan")):
        audio, video = padded_inputs(case["items"], fill)
        with _dirty.dirty(monkeypatch):
            feats = m.visual_frontend.forward_ragged(video, TV_LEN)
            got.append(m.model.forward_ragged(audio, feats, T_LEN, TV_LEN))
    assert bool(torch.isfinite(got[1]).all())
    assert torch.equal(got[0], got[1])
    for b, (_, _, est) in enumerate(case["out"]):
        e = got[1][b, :, :T_LEN[b]].cpu().numpy()
        assert np.array_equal(e / np.max(np.abs(e)), est)


def test_c_each_estimate_matches_enhance(case):
    for b, (d, (clean, noisy, est)) in enumerate(zip(case["items"], case["out"])):
        c1, n1, e1 = case["m"].enhance(d)
        assert np.array_equal(clean, c1) and np.array_equal(noisy, n1)
        rms, bar, dsdr = errors(est, e1, d["clean"])
        print(f"\nutterance {b} vs enhance(): RMS {rms:.2e} (bar {bar:.1e}), |dSI-SDR| {dsdr:.2e} dB")
        assert rms <= bar and dsdr <= 0.01, (b, rms, bar, dsdr)


def test_d_length_peak_and_the_reference_pad(case):
    assert [t - (20 * (k - 1) + 40) for t, k in zip(T_LEN, K_LEN)] == [0, 15, 0]
    for t, k, (_, _, est) in zip(T_LEN, K_LEN, case["out"]):
        assert est.shape == (2, t) and est.dtype == np.float32
        assert float(np.max(np.abs(est))) == 1.0
        assert 20 * (k - 1) + 40 <= t and not est[:, 20 * (k - 1) + 40:].any()     # model.py:92-93 F.pad
        assert est[:, 20 * (k - 1) + 20:20 * (k - 1) + 40].any()                    # the last frame itself is there


def test_e_zero_padding_alone_misses_the_bar(case):
    """Negative control: the dense forward on the zero-padded batch misses bar (a) for the shortest utterance (gLN
    over the padding, the shifts read back by the dilated convs, the clamped upsampling edge), so (a) cannot pass by
    accident of the inputs."""
    audio, video = padded_inputs(case["items"], 0.0)
    with torch.no_grad():
        est = case["m"]({"noisy_audio": audio, "vis_feat": video})
    b = int(np.argmin(T_LEN))
    e = est[b, :, :T_LEN[b]].cpu().numpy()
    e = e / np.max(np.abs(e))
    rms, bar, dsdr = errors(e, case["refs"][b], case["items"][b]["clean"])
    print(f"\ndense forward on the padded batch, utterance {b}: RMS {rms:.2e} (bar {bar:.1e}), |dSI-SDR| {dsdr:.2e} dB")
    assert not passes(e, case["refs"][b], case["items"][b]["clean"])


def test_f_the_tool_enhances_a_directory(case, tmp_path):
    """tools/avse4_enhance.py (enhance_dir: all of main() behind the checkpoint load, which test_gpu_ckpt_io.py covers
    for the default-size model) on the three utterances: scenes found -> planned batches -> <scene>.wav; each file is
    the enhance_batch estimate of what the tool read (the PCM_16 noisy wav) to the PCM_16 step, an existing file is
    left alone, and a second run finds nothing to do."""
    import os

    from avse_challenge_amd import ckpt_io
    tool = _ragged.load_tool("avse4_enhance")
    noisy, lips, out = (str(tmp_path / d) for d in ("noisy", "lips", "out"))
    for d in (noisy, lips, out):
        os.mkdir(d)
    for b, d in enumerate(case["items"]):
        ckpt_io.write_wav(os.path.join(noisy, f"S{b}_mix.wav"), d["noisy_audio"].numpy().T, 16000)
        np.save(os.path.join(lips, f"S{b}.npy"), d["vis_feat"][0].numpy())
    ckpt_io.write_wav(os.path.join(out, "S2.wav"), np.zeros((10, 2)), 16000)            # there already: not redone
    assert sorted(tool.enhance_dir(case["m"], noisy, lips, out, batch_size=2)) == ["S0", "S1"]
    assert sorted(os.listdir(out)) == ["S0.wav", "S1.wav", "S2.wav"]
    assert ckpt_io.read_wav(os.path.join(out, "S2.wav"))[0].shape == (10, 2)
    items = [tool.load_item(noisy, lips, f"S{b}") for b in (0, 1)]
    for b, (_, _, est) in enumerate(case["m"].enhance_batch(items)):
        wav, sr = ckpt_io.read_wav(os.path.join(out, f"S{b}.wav"))
        assert sr == 16000 and wav.shape == (T_LEN[b], 2)
        assert float(np.abs(wav - est.T).max()) <= 1.5 / 32768
    assert tool.find_scenes(noisy, lips, out) == []
    # an estimate computed from the quantised wav is not the fixture's, but close to it: the tool read the right files
    assert float(np.abs(ckpt_io.read_wav(os.path.join(out, "S0.wav"))[0].T - case["out"][0][2]).max()) < 0.05
