"""StreamingSeparator's framing bookkeeping, on the CPU: with the mask network replaced by a stateless stub (an
all-ones mask) the streamed output must equal the offline encoder -> decoder, whatever the push sizes.  What is
checked is the carried half window of input samples, the carried half frame of the decoder's overlap-add, the
frame count per push and the flush; the stateful layers are the GPU tests' business."""
import pytest
import torch

from avse_challenge_amd import mamba_tasnet as M
from oracle.det_init import det_init_, det_input


class _OnesMask(torch.nn.Module):
    def __init__(self, n_spk):
        super().__init__()
        self.n_spk = n_spk
        self.calls = []

    def forward(self, mix_w, inference_params=None):
        self.calls.append((mix_w.shape[-1], None if inference_params is None else inference_params.seqlen_offset))
        return torch.ones(self.n_spk, *mix_w.shape)


def _model(k=16):
    m = det_init_(M.MambaTasNet(N=24, kernel_size=k, n_mamba=1, bidirectional=False), 31)
    m.masknet = _OnesMask(m.num_spks)
    return m.eval()


@pytest.mark.parametrize("pushes", [[8, 24, 800, 8, 760], [8, 8, 8, 16, 1560], [1600], [16] * 100])
def test_streamed_framing_equals_offline(pushes):
    m = _model()
    T = sum(pushes)
    assert T >= 16 and (T - 16) % 8 == 0
    mix = 0.1 * det_input((2, T), 601)
    with torch.no_grad():
        ref = m(mix)
    sep = M.StreamingSeparator(m, batch=2)
    m.masknet.calls.clear()
    outs, t = [], 0
    for c in pushes:
        outs.append(sep.push(mix[:, t:t + c]))
        t += c
    outs.append(sep.flush())
    got = torch.cat(outs, 1)
    assert got.shape == ref.shape == (2, T, 2)
    torch.testing.assert_close(got, ref, atol=1e-6, rtol=0)
    # the first push yields one frame fewer than its hops (none for a single hop); later ones one frame per hop
    assert outs[0].shape[1] == pushes[0] - 8
    for c, o in zip(pushes[1:], outs[1:-1]):
        assert o.shape[1] == c
    assert outs[-1].shape[1] == 8
    # the frame offset handed to the layers advances by the frames pushed so far
    frames = [f for f, _ in m.masknet.calls]
    assert [o for _, o in m.masknet.calls] == [sum(frames[:i]) for i in range(len(frames))]
    assert sum(frames) == T // 8 - 1


def test_reset_and_argument_checks():
    m = _model()
    sep = M.StreamingSeparator(m, batch=2)
    mix = 0.1 * det_input((2, 64), 602)
    a = torch.cat([sep.push(mix[:, :24]), sep.push(mix[:, 24:]), sep.flush()], 1)
    assert sep.params.seqlen_offset == 0 and sep.in_tail is None and sep.out_tail is None   # flush resets
    sep.push(mix[:, :8])
    sep.reset()
    b = torch.cat([sep.push(mix), sep.flush()], 1)
    torch.testing.assert_close(a, b, atol=1e-6, rtol=0)
    assert sep.flush().shape == (2, 0, 2)                    # nothing pushed: an empty tail
    for bad in (mix[:, :7], mix[:, :0], mix[:1, :8]):
        with pytest.raises(ValueError):
            sep.push(bad)
    with pytest.raises(ValueError):
        M.StreamingSeparator(M.MambaTasNet(N=24, n_mamba=1), batch=1)      # bidirectional: not causal


def test_bidirectional_default_keeps_keys():
    a = M.MambaTasNet(N=24, n_mamba=2)
    b = M.MambaTasNet(N=24, n_mamba=2, bidirectional=True)
    assert list(a.state_dict()) == list(b.state_dict())
    c = M.MambaTasNet(N=24, n_mamba=2, bidirectional=False)
    assert list(c.state_dict()) == [k for k in a.state_dict() if "_b." not in k and "_b_log" not in k
                                    and not k.endswith(".D_b")]
