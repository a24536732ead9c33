"""GPU tests of the flat absmax pass of split_planes (csrc/projgemm.hip) and of the one-launch weight preparation of
the dilated convs (avse_dconv_wprep2, csrc/dconv.hip).  Both changes move no arithmetic, so every check is bit-exact:
the max bits equal torch's abs().max(), the planes and the weight images equal a torch restatement of the split."""
import pytest
import torch

from oracle.det_init import det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last


def K():
    from avse_challenge_amd import kernels
    return kernels


# ------------------------------------------------------------------ split_planes' absmax on short rows

def _split_ref(x):
    """torch restatement of the planes split (projgemm.hip): scale 2^e with max |x| 2^e in [2^14, 2^15)."""
    bits = int(x.abs().max().view(torch.int32).item())
    k = ((bits >> 23) & 0xFF) - 127 if (bits >> 23) & 0xFF else -127
    e = max(-100, min(100, 14 - k)) if bits else 0
    s = x * 2.0 ** e                                      # exact: a power of two
    hi = s.to(torch.float16)
    lo = (s - hi.float()).to(torch.float16)
    return bits, hi, lo


def _check_planes(sp, x):
    bits, hi, lo = _split_ref(x)
    assert int(sp.mb.item()) == bits
    assert torch.equal(sp.hi.view(torch.int16), hi.view(torch.int16))
    assert torch.equal(sp.lo.view(torch.int16), lo.view(torch.int16))


@pytest.mark.parametrize("rows,c", [(10, 64), (70, 64), (128, 64), (33, 130), (3, 1536), (8, 1536)])
def test_split_planes_contiguous_rows(rows, c):
    """n < 4096, n % 4096 != 0 and n % 4096 == 0; rows of 16 float4, rows that are not 16-B aligned, long rows.  The
    largest element sits in the tail (the last n % 4 elements / the last row)."""
    x = det_input((1, rows, c), 3600 + rows + c).to(DEV)
    x[0, -1, -1] = 7.5
    _check_planes(K().split_planes(x), x)
    x[0, -1, -1] = 0.25
    x[0, rows // 2, 1] = -9.0
    _check_planes(K().split_planes(x), x)


def test_split_planes_strided_and_padded():
    base = det_input((2, 5, 200), 3700).to(DEV)
    v = base[:, :, :132]                                  # strided rows (16-B aligned): the row walk, 1 row per 64 threads
    base[1, 4, 150] = 50.0                                # outside the view: must not be seen
    v[1, 3, 131] = -6.0
    _check_planes(K().split_planes(v), v)
    base2 = det_input((1, 100, 72), 3701).to(DEV)
    v2 = base2[:, :, :64]                                 # 16 float4 per row: 64 rows in flight per workgroup
    base2[0, 50, 70] = 50.0
    v2[0, 99, 63] = 8.0
    _check_planes(K().split_planes(v2), v2)
    v3 = base2[:, :, 1:66]                                # rows that are not 16-B aligned: the scalar row walk
    v3[0, 77, 64] = -11.0
    _check_planes(K().split_planes(v3), v3)
    x = det_input((2, 33, 130), 3702).to(DEV)             # padded output rows (130 -> 136): contiguous input, flat max
    x[1, 32, 129] = 12.0
    _check_planes(K().split_rows8(x), x)


# ------------------------------------------------------------------ one-launch weight preparation

def _wimage_ref(w, transposed):
    """torch restatement of dconv.hip's weight image: [stage = kh * 4 + q][kw][o][hi 16 | lo 16] of channel i = 16 q + c;
    transposed: W'[o][i][kh][kw] = W[i][o][4 - kh][4 - kw]."""
    bits, _, _ = _split_ref(w)
    k = ((bits >> 23) & 0xFF) - 127
    e = max(-100, min(100, 14 - k))
    v = w.permute(1, 0, 2, 3).flip(2, 3) if transposed else w
    v = v.permute(2, 1, 3, 0).reshape(5, 4, 16, 5, 64).permute(0, 1, 3, 4, 2)           # (kh, q, kw, o, c)
    s = v.contiguous() * 2.0 ** e
    hi = s.to(torch.float16)
    lo = (s - hi.float()).to(torch.float16)
    return bits, torch.cat([hi, lo], -1).reshape(-1).view(torch.int16)


@pytest.mark.parametrize("spike", [False, True])
def test_dconv_wprep2_images(spike):
    w = (0.05 * det_input((64, 64, 5, 5), 3800)).to(DEV)
    if spike:
        w[17, 45, 3, 1] = -3.0                            # a single large element: the others fall into fp16 subnormals
    mb = torch.zeros(2, device=DEV, dtype=torch.int32)
    mbd = torch.zeros(2, device=DEV, dtype=torch.int32)
    wq, wq_t = K().dconv_wprep2(w, mb, mbd)
    for got, tr in ((wq, False), (wq_t, True)):
        bits, ref = _wimage_ref(w, tr)
        assert int(mb[1].item()) == bits and int(mbd[1].item()) == bits
        assert torch.equal(got.view(torch.int16), ref)
        old_mb = torch.zeros(2, device=DEV, dtype=torch.int32)
        assert torch.equal(K().dconv_wprep(w, tr, old_mb), got) and int(old_mb[1].item()) == bits
    only, none = K().dconv_wprep2(w, mb)                  # no input gradient asked for: the forward image alone
    assert none is None and torch.equal(only, wq)


def test_dilated_conv_keeps_transposed_image_only_for_an_input_gradient():
    """layers.DilatedConv2d: with an input that needs a gradient the forward's one launch also prepares the backward's
    transposed image; without, only the forward image.  The weight and bias gradients are the same bits either way."""
    from avse_challenge_amd import layers
    conv = layers.DilatedConv2d(64, 64, 5, padding=4, dilation=2).to(DEV).to(memory_format=CL)
    x = det_input((1, 64, 3, 257), 3900).to(DEV).contiguous(memory_format=CL)
    gy = det_input((1, 64, 3, 257), 3901).to(DEV).contiguous(memory_format=CL)
    grads = []
    for need in (True, False):
        conv.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(need)
        y = conv(xi)
        assert len(y.grad_fn.saved_tensors) == (5 if need else 3)
        y.backward(gy)
        assert (xi.grad is not None) == need
        grads.append((y.detach(), conv.weight.grad.clone(), conv.bias.grad.clone()))
    for a, b in zip(*grads):
        assert torch.equal(a, b)
