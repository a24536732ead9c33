"""The fused lip front-end chain BatchNorm3d -> ReLU / PReLU -> MaxPool3d((1, 3, 3), (1, 2, 2), (0, 1, 1)) -> channels-last
frames (csrc/bnact.hip namespace pool, layers.bn_act_pool_frames) against the unfused bn_act -> maxpool3d -> frames_nhwc
and torch fp64.

Shapes (B, C, T, H, W): (2, 64, 3, 8, 8) every window touches an edge; (2, 64, 2, 12, 16) interior windows, H != W, a
ragged last row band; (1, 128, 2, 8, 12) two channel tiles; (1, 64, 2, 48, 48) and (1, 64, 1, 56, 56) the two real plane
sizes; (2, 64, 2, 8, 10) has W % 4 != 0 and must take the three functions.

Inputs: x on a 0.5 grid (ties inside windows), gamma with negative entries and one zero, PReLU slopes with a zero and a
negative one (neither map is then monotone: pooling x first would pick other elements), ReLU as well, training and eval.

Bars.  Forward: bit-equal (the pre-activation has one definition, the scan order is maxpool.hip's).  Backward against
the unfused chain: the un-pooled gradient is the same value and the masks are the same bits, only the two per-channel
means move by the rounding of a re-ordered fp32 sum: dx within 1e-6 max |dx|, dgamma / dbeta / dalpha within 1e-5 of
their max (the bars of tests/test_gpu_bn_bwd_fused.py).  Against torch fp64: the bars of test_bnact_vs_fp64."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle.det_init import det_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
POOL = ((3, 3), (2, 2), (1, 1))
SHAPES = [(2, 64, 3, 8, 8), (2, 64, 2, 12, 16), (1, 128, 2, 8, 12), (1, 64, 2, 48, 48), (1, 64, 1, 56, 56)]
FALLBACK_SHAPE = (2, 64, 2, 8, 10)
CASES = [(s, a, t) for s in SHAPES for a in ("prelu_c", "relu") for t in (True, False)]
IDS = ["x".join(map(str, s)) + f"-{a}-{'train' if t else 'eval'}" for s, a, t in CASES]


def K():
    from avse_challenge_amd import kernels
    return kernels


def _params(C, act):
    gen = torch.Generator().manual_seed(C + 17)
    gam = 0.5 + torch.rand(C, generator=gen)
    gam[1::5] *= -1.0
    gam[3] = 0.0
    bet = 0.1 * torch.randn(C, generator=gen)
    alpha = None
    if act == "prelu_c":
        alpha = 0.1 + 0.3 * torch.rand(C, generator=gen)
        alpha[0], alpha[2] = 0.0, -0.25
    rm = 0.7 + 0.2 * torch.randn(C, generator=gen)
    rv = 2.0 * (1.0 + torch.rand(C, generator=gen))
    return gam, bet, alpha, rm, rv


def _x(shape):
    return torch.round(2.0 * (1.5 * det_input(shape, 770) + 0.7)) / 2.0       # multiples of 0.5


def _g(shape):
    """The gradient of the frames (B T, C, Ho, Wo), channels-last, three quarters of it zeros."""
    B, C, T, H, W = shape
    fs = (B * T, C, H // 2, W // 2)
    g = det_input(fs, 771) * (det_input(fs, 772, "uniform") < 0.25)
    return g.float().contiguous(memory_format=torch.channels_last)


def _dev(t):
    return None if t is None else t.float().to(DEV)


def _unfused_fwd(k, x, gam, bet, alpha, rm, rv, training, code):
    from avse_challenge_amd.layers import frames_nhwc
    y, stats = k.bnact_fwd(x, gam, bet, rm, rv, training, 0.1, 1e-5, code, alpha)
    yp, idx = k.maxpool_planes_fwd(y, *POOL)
    return frames_nhwc(yp), idx, stats


def _unfused_bwd(k, x, g, idx, stats, gam, bet, alpha, training, code):
    B, C, T, H, W = x.shape
    d = g.permute(0, 2, 3, 1).contiguous().view(B, T * (H // 2) * (W // 2), C)
    gp = k.transpose_cp(d).view(B, C, T, H // 2, W // 2)
    du = k.maxpool_planes_bwd(gp, idx, x.shape, *POOL)
    dx, _, dg, db, da = k.bnact_bwd(x, None, du, stats, gam, bet, code, alpha, training)
    return dx, dg, db, da


def _fp64(x, g, gam, bet, alpha, rm, rv, training):
    B, C, T, H, W = x.shape
    xd = x.double().requires_grad_(True)
    gd, bd = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    z = F.batch_norm(xd, rm.double().clone(), rv.double().clone(), gd, bd, training, 0.1, 1e-5)
    ad = None if alpha is None else alpha.double().requires_grad_(True)
    y = torch.relu(z) if alpha is None else F.prelu(z, ad)
    yp = F.max_pool3d(y, (1, 3, 3), (1, 2, 2), (0, 1, 1))
    yp.permute(0, 2, 1, 3, 4).reshape(B * T, C, H // 2, W // 2).backward(g.double())
    return xd.grad, gd.grad, bd.grad, None if ad is None else ad.grad


@functools.lru_cache(maxsize=None)
def _case(shape, act, training):
    """Inputs, the unfused chain's results and the fp64 gradients of one case: computed once, read by every test."""
    k = K()
    C = shape[1]
    gam, bet, alpha, rm, rv = _params(C, act)
    x, g = _x(shape), _g(shape)
    code = k.ACT_PRELU if act == "prelu_c" else k.ACT_RELU
    dv = dict(x=_dev(x), g=_dev(g).contiguous(memory_format=torch.channels_last), gam=_dev(gam), bet=_dev(bet),
              alpha=_dev(alpha), code=code, training=training, rm=rm, rv=rv)
    rm_u, rv_u = _dev(rm), _dev(rv)
    y, idx, stats = _unfused_fwd(k, dv["x"], dv["gam"], dv["bet"], dv["alpha"], rm_u, rv_u, training, code)
    dx, dg, db, da = _unfused_bwd(k, dv["x"], dv["g"], idx, stats, dv["gam"], dv["bet"], dv["alpha"], training, code)
    dv.update(y=y, idx=idx, stats=stats, rm_u=rm_u, rv_u=rv_u, dx=dx, dg=dg, db=db, da=da,
              dxmax=int(getattr(dx, k.ABSMAX_ATTR).item()), ref=_fp64(x, g, gam, bet, alpha, rm, rv, training))
    return dv


def _fused_fwd(c):
    rm, rv = _dev(c["rm"]), _dev(c["rv"])
    y, idx, stats = K().bnact_pool_frames_fwd(c["x"], c["gam"], c["bet"], rm, rv, c["training"], 0.1, 1e-5, c["code"],
                                              c["alpha"])
    return y, idx, stats, rm, rv


def _fused_bwd(c, idx, stats):
    return K().bnact_pool_frames_bwd(c["x"], c["g"], idx, stats, c["gam"], c["bet"], c["code"], c["alpha"],
                                     c["training"])


def _close(a, b, atol, rtol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs()
    print(f"{what}: max err {float(err.max()):.3e} (atol {atol:.3e})")
    assert bool((err <= atol + rtol * b.abs()).all()), (what, float(err.max()), atol)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("shape,act,training", CASES, ids=IDS)
def test_forward_bit_equal(shape, act, training):
    """Frames, argmax (maxpool.hip's plane layout and window encoding), statistics and running statistics."""
    c = _case(shape, act, training)
    assert K().bnpool_ok(c["x"], *POOL)
    y, idx, stats, rm, rv = _fused_fwd(c)
    assert y.shape == c["y"].shape and y.stride() == c["y"].stride()
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(_bits(y), _bits(c["y"]))
    assert torch.equal(idx, c["idx"])                      # kh << 4 | kw per pooled element: the same window positions
    assert torch.equal(_bits(stats), _bits(c["stats"]))
    assert torch.equal(rm, c["rm_u"]) and torch.equal(rv, c["rv_u"])


@pytest.mark.parametrize("shape,act,training", CASES, ids=IDS)
def test_backward(shape, act, training, monkeypatch):
    k = K()
    c = _case(shape, act, training)
    _, idx, stats, _, _ = _fused_fwd(c)
    first = _fused_bwd(c, idx, stats)
    real = k._bnpool_ws                                     # a slice no workgroup wrote shows in every sum
    monkeypatch.setattr(k, "_bnpool_ws", lambda *a: real(*a).fill_(float("nan")))
    dx, dg, db, da = _fused_bwd(c, idx, stats)
    for a, b in zip(first, (dx, dg, db, da)):               # deterministic, and the workspace's content is not read
        assert (a is None and b is None) or torch.equal(_bits(a), _bits(b))
    m = float(c["dx"].abs().max())
    _close(dx, c["dx"], 1e-6 * m, 0.0, "dx vs unfused")
    _close(dg, c["dg"], 1e-5 * float(c["dg"].abs().max()), 0.0, "dgamma vs unfused")
    _close(db, c["db"], 1e-5 * float(c["db"].abs().max()), 0.0, "dbeta vs unfused")
    if da is not None:
        _close(da, c["da"], 1e-5 * float(c["da"].abs().max()), 0.0, "dalpha vs unfused")
    rdx, rdg, rdb, rda = c["ref"]
    _close(dx, rdx, 2e-5 * float(rdx.abs().max()), 1e-4, "dx vs fp64")
    _close(dg, rdg, 1e-4 * float(rdg.abs().max()), 1e-4, "dgamma vs fp64")
    _close(db, rdb, 1e-4 * float(rdb.abs().max()), 1e-4, "dbeta vs fp64")
    if da is not None:
        _close(da, rda, 1e-4 * float(rda.abs().max()) + 1e-7, 1e-4, "dalpha vs fp64")
    # the published max |dx|: the maximum of the values as stored (the apply pass takes it as bwd_apply_kernel does),
    # so never below the true one; the unfused chain's differs from it by the same rounding as dx
    pub = int(getattr(dx, k.ABSMAX_ATTR).item())
    assert pub == int(dx.abs().max().view(torch.int32).item())
    pf, uf = (torch.tensor([v], dtype=torch.int32).view(torch.float32).item() for v in (pub, c["dxmax"]))
    assert abs(pf - uf) <= 1e-6 * m, (pf, uf)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", [SHAPES[0], FALLBACK_SHAPE], ids=["fused", "fallback"])
def test_layer_function(shape, training, monkeypatch):
    """layers.bn_act_pool_frames with modules: the running statistics and num_batches_tracked of bn_act, the old
    functions not called on the fused path, all three called for W % 4 != 0."""
    from avse_challenge_amd import layers
    k = K()
    C = shape[1]
    gam, bet, alpha, rm, rv = _params(C, "prelu_c")

    def make():
        bn = torch.nn.BatchNorm3d(C).to(DEV).train(training)
        act = layers.PReLU(C).to(DEV)
        with torch.no_grad():
            bn.weight.copy_(gam), bn.bias.copy_(bet), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
            act.weight.copy_(alpha)
        return bn, act

    pool = torch.nn.MaxPool3d((1, 3, 3), (1, 2, 2), (0, 1, 1))
    x = _dev(_x(shape))
    bn_u, act_u = make()
    want = layers.frames_nhwc(layers.maxpool3d(layers.bn_act(x, bn_u, act_u), pool))
    calls = {"bnact_fwd": 0, "maxpool_planes_fwd": 0, "transpose_cp": 0}
    for name in calls:
        real = getattr(k, name)
        monkeypatch.setattr(k, name, lambda *a, _n=name, _r=real, **kw: (calls.__setitem__(_n, calls[_n] + 1),
                                                                         _r(*a, **kw))[1])
    bn_f, act_f = make()
    got = layers.bn_act_pool_frames(x, bn_f, act_f, pool)
    fused = k.bnpool_ok(x, *POOL)
    assert fused == (shape != FALLBACK_SHAPE)
    assert calls == dict.fromkeys(calls, 0 if fused else 1), calls
    assert got.stride() == want.stride() and torch.equal(_bits(got), _bits(want))
    assert torch.equal(bn_f.running_mean, bn_u.running_mean) and torch.equal(bn_f.running_var, bn_u.running_var)
    assert int(bn_f.num_batches_tracked) == int(bn_u.num_batches_tracked) == (1 if training else 0)


def test_frontend_autograd(monkeypatch):
    """Conv3d -> BN -> PReLU -> pool -> frames -> one TrunkConv2d: fused against the three functions."""
    from avse_challenge_amd import layers
    k = K()
    torch.manual_seed(5)
    conv = layers.LipConv3d(3, 64, (5, 7, 7), (1, 2, 2), (2, 3, 3)).to(DEV)
    bn = torch.nn.BatchNorm3d(64).to(DEV).train()
    act = layers.PReLU(64).to(DEV)
    pool = torch.nn.MaxPool3d((1, 3, 3), (1, 2, 2), (0, 1, 1))
    trunk = layers.TrunkConv2d(64, 64).to(DEV).to(memory_format=torch.channels_last)
    gam, bet, alpha, _, _ = _params(64, "prelu_c")
    with torch.no_grad():
        bn.weight.copy_(gam), bn.bias.copy_(bet), act.weight.copy_(alpha)
    lips = det_input((2, 3, 3, 24, 32), 773, "uint8").float().to(DEV)          # conv output (2, 64, 3, 12, 16)
    gy = det_input((6, 64, 6, 8), 774).float().to(DEV).contiguous(memory_format=torch.channels_last)
    params = [conv.weight, bn.weight, bn.bias, act.weight, trunk.weight]
    calls = {"bnact_fwd": 0, "maxpool_planes_fwd": 0, "transpose_cp": 0}
    for name in calls:
        real = getattr(k, name)
        monkeypatch.setattr(k, name, lambda *a, _n=name, _r=real, **kw: (calls.__setitem__(_n, calls[_n] + 1),
                                                                         _r(*a, **kw))[1])

    def run(fused):
        for p in params:
            p.grad = None
        h = conv(lips)
        if fused:
            f = layers.bn_act_pool_frames(h, bn, act, pool)
        else:
            f = layers.frames_nhwc(layers.maxpool3d(layers.bn_act(h, bn, act), pool))
        loss = (trunk(f) * gy).sum()
        loss.backward()
        return loss.detach(), [p.grad.clone() for p in params]

    loss_f, gf = run(True)
    assert calls == dict.fromkeys(calls, 0), calls
    loss_u, gu = run(False)
    assert calls["bnact_fwd"] == 1 and calls["maxpool_planes_fwd"] == 1 and calls["transpose_cp"] == 2, calls
    assert torch.equal(_bits(loss_f), _bits(loss_u))
    assert torch.equal(gf[4], gu[4])                                          # the trunk conv sees the same frames
    _close(gf[0], gu[0], 1e-5 * float(gu[0].abs().max()), 0.0, "conv3d dW")   # linear in dx (1e-6 max |dx|)
    for a, b, what in zip(gf[1:4], gu[1:4], ("dgamma", "dbeta", "dalpha")):
        _close(a, b, 1e-5 * float(b.abs().max()), 0.0, what)
