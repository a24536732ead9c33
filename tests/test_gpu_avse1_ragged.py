"""Length-aware batched enhancement of a ragged avse1 batch (AVNet.enhance_batch / forward_ragged,
AudioFeatNet.forward_ragged, VisualFeatNet.forward_ragged) against the fp64 oracle on each utterance alone.

The full AVNet, det_init_, eval, channels-last (NHWC audio convs on csrc/dconv.hip, lip trunk on csrc/sconv.hip).  Lips
are 96 x 96 uint8: the smallest H = W at which the lip Conv3d (csrc/conv3d_fwd.hip is compiled for 96 x 96) and every
3x3 conv of the channels-last trunk (kernels.sconv_fwd_fits down to its 3 x 3 maps) run on the project's own kernels;
smaller frames send part of the trunk to the library.  Three utterances:
    T = 16000: 126 STFT frames, 25 lip frames
    T =  9215:  72 frames (9215 % 128 = 127), 14 lip frames
    T =  6000:  47 frames, fewer than the 62 the five dilated convs reach, and 9 lip frames, fewer than the TCN's 30
The bar is that of tests/test_gpu_fullsize.py: waveform RMS <= 1e-4 max(1, RMS(ref)) and |dSI-SDR| <= 0.01 dB, with
stft_ref in front of and behind the oracle as there.  The oracle runs once (module fixture); all GPU work allocates
dirty (tests/_dirty.py)."""
import numpy as np
import pytest
import torch

import _dirty
import _ragged
from _ragged import errors
from oracle import avse1_ref, stft_ref
from oracle.det_init import det_init_, det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_LEN, TV_LEN, HW = (16000, 9215, 6000), (25, 14, 9), 96
F_LEN = tuple(1 + t // 128 for t in T_LEN)
PAD_RATIO = 2.0           # 3 x 16000 padded / 31215 useful samples = 1.54: the planner keeps the three in one batch


def oracle_enhance(ref, noisy, lips):
    """test.py:79-89 on one utterance in fp64: stft_ref -> oracle AVNet -> noisy phase -> stft_ref.istft."""
    spec = stft_ref.stft(noisy.numpy()[None])                                  # (1, 257, frames) complex
    mag_T = np.swapaxes(np.abs(spec), -1, -2).astype(np.float32)               # dataset.py:112-118
    inp = {"noisy_audio_spec": torch.from_numpy(mag_T).double()[:, None]}
    if lips is not None:
        inp["lip_images"] = lips[None]
    with torch.no_grad():
        pred = ref(inp)[:, 0]
    phase = np.angle(spec)
    est_spec = np.swapaxes(pred.numpy(), -1, -2) * (np.cos(phase) + 1j * np.sin(phase))
    return stft_ref.istft(est_spec, length=noisy.shape[-1])[0]


def padded_inputs(items, audio_fill, lip_fill, lip_dtype):
    audio = torch.full((3, max(T_LEN)), audio_fill)
    lips = torch.full((3, 3, max(TV_LEN), HW, HW), lip_fill, dtype=lip_dtype)
    for b, d in enumerate(items):
        audio[b, :T_LEN[b]] = d["noisy_audio"]
        lips[b, :, :TV_LEN[b]] = d["lip_images"].to(lip_dtype)
    return audio.to(DEV), lips.to(DEV)


def run_padded(m, audio, lips):
    """What enhance_batch does with one padded batch, from tensors the test padded itself."""
    from avse_challenge_amd import kernels as K
    wl = K.Lengths(T_LEN, DEV)
    mag, spec = K.stft(audio, return_complex=True, lengths=wl)
    inp = {"noisy_audio_spec": mag.unsqueeze(1)}
    if lips is not None:
        inp["lip_images"] = lips
    pred = m.forward_ragged(inp, F_LEN, None if lips is None else TV_LEN)[:, 0]
    return K.istft(pred, spec, max(T_LEN), lengths=wl)


@pytest.fixture(scope="module")
def case():
    from avse_challenge_amd import avse1
    _ragged.fp32_math()
    items = [{"noisy_audio": 0.1 * det_input((t,), 7100 + b), "clean": 0.1 * det_input((t,), 7120 + b),
              "lip_images": det_input((3, tv, HW, HW), 7110 + b, "uint8")}
             for b, (t, tv) in enumerate(zip(T_LEN, TV_LEN))]
    m = det_init_(avse1.AVNet(), 91).to(DEV).eval()
    m.net_audiofeat.use_channels_last()
    m.net_visualfeat.use_channels_last()
    r = det_init_(avse1_ref.AVNet(), 91).double().eval()
    refs = [oracle_enhance(r, d["noisy_audio"], d["lip_images"]) for d in items]     # each utterance alone, fp64
    mp = pytest.MonkeyPatch()
    with _dirty.dirty(mp):
        out = m.enhance_batch(items, batch_size=3, max_pad_ratio=PAD_RATIO)
    return dict(m=m, items=items, refs=refs, out=out)


def test_a_each_estimate_matches_the_oracle_on_the_utterance_alone(case):
    assert F_LEN == (126, 72, 47)
    for b, (d, ref, est) in enumerate(zip(case["items"], case["refs"], case["out"])):
        assert est.shape == (T_LEN[b],) and est.dtype == np.float32
        rms, bar, dsdr = errors(est, ref, d["clean"])
        print(f"\nutterance {b}: RMS error {rms:.2e} (bar {bar:.1e}), |dSI-SDR| {dsdr:.2e} dB")
        assert rms <= bar, f"utterance {b}: RMS waveform error {rms:.3e} > {bar:.1e}"
        assert dsdr <= 0.01, f"utterance {b}: SI-SDR differs by {dsdr:.4f} dB"


def test_b_what_the_padding_holds_is_not_used(case, monkeypatch):
    """NaN in the audio padding and 255 (uint8 lips) / NaN (float lips) in the lip padding: bitwise the estimates of
    the zero-padded call, which for the uint8 lips are enhance_batch's."""
    m = case["m"]
    for dtype, fill in ((torch.uint8, 255), (torch.float32, float("nan"))):
        got = []
        for af, lf in ((0.0, 0), (float("nan"), fill)):
            audio, lips = padded_inputs(case["items"], af, lf, dtype)
            with _dirty.dirty(monkeypatch):
                got.append(run_padded(m, audio, lips))
        assert bool(torch.isfinite(got[1]).all()), dtype
        assert torch.equal(got[0], got[1]), dtype
        for b, t in enumerate(T_LEN):
            assert not got[1][b, t:].any()
            if dtype == torch.uint8:
                assert np.array_equal(got[1][b, :t].cpu().numpy(), case["out"][b])
            else:                                            # fp32 frames go through the Conv3d's fp32 split instead
                rms, bar, dsdr = errors(got[1][b, :t].cpu(), case["refs"][b], case["items"][b]["clean"])
                assert rms <= bar and dsdr <= 0.01, (b, rms, bar, dsdr)


def test_b2_the_plain_path(case, monkeypatch):
    """The NCHW model (library convs, maxpool3d, the contiguous forms of the length-aware BatchNorm) on float lips with
    NaN padding: each estimate within the bar of the oracle."""
    from avse_challenge_amd import avse1
    m = det_init_(avse1.AVNet(), 91).to(DEV).eval()
    audio, lips = padded_inputs(case["items"], float("nan"), float("nan"), torch.float32)
    with _dirty.dirty(monkeypatch):
        got = run_padded(m, audio, lips)
    for b, t in enumerate(T_LEN):
        rms, bar, dsdr = errors(got[b, :t].cpu(), case["refs"][b], case["items"][b]["clean"])
        print(f"\nplain path, utterance {b}: RMS {rms:.2e} (bar {bar:.1e}), |dSI-SDR| {dsdr:.2e} dB")
        assert rms <= bar and dsdr <= 0.01, (b, rms, bar, dsdr)
        assert not got[b, t:].any()


def test_c_batch_composition(case, monkeypatch):
    """The longest row of the batch of three against enhance() on it alone: within the bar (not bitwise: the split-fp16
    convolutions and GEMMs scale their operands by the maximum over the whole batch).  A batch of one is enhance() bit
    for bit: no padding exists, every length-aware kernel runs the dense kernel's arithmetic on every element, and the
    split BatchNorm output is the split of the dense output under the same (exact) maximum."""
    m = case["m"]
    d = case["items"][0]
    with _dirty.dirty(monkeypatch):
        alone = m.enhance(d["noisy_audio"][None].to(DEV), d["lip_images"][None].to(DEV))[0].cpu().numpy()
    rms, bar, dsdr = errors(case["out"][0], alone, d["clean"])
    print(f"\nlongest row vs enhance(): RMS {rms:.2e} (bar {bar:.1e}), |dSI-SDR| {dsdr:.2e} dB")
    assert rms <= bar and dsdr <= 0.01
    for b in (0, 2):
        d = case["items"][b]
        with _dirty.dirty(monkeypatch):
            one = m.enhance_batch([(d["noisy_audio"], d["lip_images"])])[0]
            ref = m.enhance(d["noisy_audio"][None].to(DEV), d["lip_images"][None].to(DEV))[0].cpu().numpy()
        assert np.array_equal(one, ref), b


def test_d_zero_padding_alone_misses_the_bar(case):
    """Negative control: dense enhance() on the zero-padded batch misses bar (a) for both shorter utterances (bn0's
    shift read back by the dilated convs, the gather over the padded T and Tv, the TCN looking into non-zero padding,
    the reflect pad and the window sum at the padded row's end), so (a) cannot pass by accident of the inputs."""
    audio, lips = padded_inputs(case["items"], 0.0, 0, torch.uint8)
    est = case["m"].enhance(audio, lips).cpu().numpy()
    for b in (1, 2):
        e, d = est[b, :T_LEN[b]], case["items"][b]
        rms, bar, dsdr = errors(e, case["refs"][b], d["clean"])
        print(f"\ndense enhance() on the padded batch, utterance {b}: RMS {rms:.2e} (bar {bar:.1e}, {rms / bar:.0f}x), "
              f"|dSI-SDR| {dsdr:.2e} dB")
        assert not (rms <= bar and dsdr <= 0.01), b


def test_e_audio_only(case, monkeypatch):
    """a_only=True on the same audio: the fp64 oracle on the shortest utterance alone, enhance() on each."""
    from avse_challenge_amd import avse1
    m = det_init_(avse1.AVNet(a_only=True), 92).to(DEV).eval()
    m.net_audiofeat.use_channels_last()
    items = [{"noisy_audio": d["noisy_audio"]} for d in case["items"]]
    with _dirty.dirty(monkeypatch):
        out = m.enhance_batch(items, batch_size=3, max_pad_ratio=PAD_RATIO)
        padded = run_padded(m, padded_inputs(case["items"], float("nan"), 0, torch.uint8)[0], None)
    r = det_init_(avse1_ref.AVNet(a_only=True), 92).double().eval()
    d = case["items"][2]
    rms, bar, dsdr = errors(out[2], oracle_enhance(r, d["noisy_audio"], None), d["clean"])
    print(f"\naudio-only, utterance 2 vs the oracle: RMS {rms:.2e} (bar {bar:.1e}), |dSI-SDR| {dsdr:.2e} dB")
    assert rms <= bar and dsdr <= 0.01
    for b, d in enumerate(case["items"]):
        assert np.array_equal(padded[b, :T_LEN[b]].cpu().numpy(), out[b])          # NaN audio padding: same bits
        alone = m.enhance(d["noisy_audio"][None].to(DEV))[0].cpu().numpy()
        rms, bar, dsdr = errors(out[b], alone, d["clean"])
        assert rms <= bar and dsdr <= 0.01, (b, rms, bar, dsdr)


def test_f_refusals(case):
    m, d = case["m"], case["items"][2]
    pair = (d["noisy_audio"], d["lip_images"])
    with pytest.raises(RuntimeError):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            m.enhance_batch([pair])
    m.train()
    try:
        with pytest.raises(RuntimeError):
            m.enhance_batch([pair])
    finally:
        m.eval()
    with pytest.raises(ValueError):
        m.enhance_batch([pair, (d["noisy_audio"][:256], d["lip_images"])])       # no room for the reflect pad
    with pytest.raises(ValueError):
        m.enhance_batch([pair, (d["noisy_audio"], d["lip_images"][:, :0])])      # no video frame
    with pytest.raises(ValueError):
        m.enhance_batch([(d["noisy_audio"], None)])                              # lips missing
    assert m.enhance_batch([]) == []
    assert len(m.enhance_batch([(d["noisy_audio"][:257], d["lip_images"])])[0]) == 257       # the shortest legal one
