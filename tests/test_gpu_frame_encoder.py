"""The frame encoder on HIP (csrc/frame_enc.hip, nfdpf.ops.frame_encoder) and its route from
DPF._frame_encodings: against the reference's own outputs, per layer against a derived bound, end
to end against float64, and for placement independence, strides, routing and refusals.  Every
reference is computed on the CPU (MIOpen's first-use search can take a minute); the only MIOpen
calls are the routing test's own comparison paths, on two frames."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from _frame_enc import device_blob, stack, trained_like
from _util import group, load

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHUNK = 256  # frames per pass over the layers (csrc/frame_enc.hpp kChunk)
CHANNELS = (3, 16, 32, 64, 128, 256)


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from nfdpf import _lib
    _lib.load()
    assert torch.cuda.is_available()


def _frames(n, seed=21):
    return torch.rand(n, 3, 128, 128, generator=torch.Generator().manual_seed(seed))


class _Case:
    """A trained-like encoder of width H, 37 frames ~ U(0, 1) and our encodings and layer
    activations for them (one call, [1, 37]), computed once and left unchanged."""

    def __init__(self, H):
        from nfdpf import ops
        self.H = H
        self.enc = trained_like(stack(H, seed=40 + H)).eval()
        self.blob = device_blob(self.enc, DEV)
        self.frames = _frames(37)
        self.dev_frames = self.frames.to(DEV)
        out, layers = ops.frame_encoder(self.blob, self.dev_frames[None], H, keep_layers=True)
        torch.cuda.synchronize()
        self.out = out[0].cpu()
        self.layers = [l[0].cpu() for l in layers]


_cases = {}


def _case(H):
    if H not in _cases:
        _cases[H] = _Case(H)
    return _cases[H]


# ----------------------------------------------------------------------------------------------
# 1. the reference's own outputs
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,benc,H", [("h32", "build_encoder", 32), ("cglow", "build_encoder_cglow", 192)])
def test_reference_eval_features(tag, benc, H):
    """tests/golden/autoencoder.npz `eval/feature`: the reference's encoder (seed 301) on its four
    frames (seed 303) in eval mode, AFTER the fixture's train-mode pass -- which calls the
    encoder twice (enc(img), then autoencoder_loss's own enc(img)): two running-statistics
    updates, replayed here on the CPU.  Bar: the one test_autoencoder_gpu gives MIOpen."""
    import model.models as mm
    from nfdpf import ops
    fx = group(load("autoencoder.npz"), tag)
    torch.manual_seed(301)
    enc = getattr(mm, benc)(H)
    img = torch.rand(2, 2, 3, 128, 128, generator=torch.Generator().manual_seed(303))
    enc.train()
    with torch.no_grad():
        f = enc(img.reshape(4, 3, 128, 128))
        enc(img.reshape(4, 3, 128, 128))
    np.testing.assert_allclose(f.numpy(), fx["train/feature"], rtol=1e-5, atol=1e-6)  # (the replay is the fixture's)
    enc.eval()
    out = ops.frame_encoder(device_blob(enc, DEV), img.to(DEV), H)
    assert out.shape == (2, 2, H)
    np.testing.assert_allclose(out.reshape(4, H).cpu().numpy(), fx["eval/feature"], rtol=2e-4, atol=2e-5)


# ----------------------------------------------------------------------------------------------
# 2. per layer, against a derived bound
# ----------------------------------------------------------------------------------------------
def _check_layers(enc, frames, out, layers, what):
    """Feed OUR layer l-1 activation (promoted to float64) to the float64 CPU layer l and compare
    with our layer l element by element."""
    convs = [m for m in enc if isinstance(m, nn.Conv2d)]
    bns = [m for m in enc if isinstance(m, nn.BatchNorm2d)]
    lin = enc[-1]
    x = frames.double()
    for l, (conv, bn) in enumerate(zip(convs, bns)):
        w = conv.weight.detach().double()
        K = 16 * CHANNELS[l]
        r = torch.relu(F.conv2d(x, w, stride=2, padding=1))
        s = F.conv2d(x.abs(), w.abs(), stride=2, padding=1)  # sum |w x| of every output element
        a = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
        b = bn.bias.detach().double() - bn.running_mean.double() * a
        a, b = a[None, :, None, None], b[None, :, None, None]
        ref = a * r + b
        bound = a.abs() * K * 2.0 ** -23 * s + 2.0 ** -21 * ((a * r).abs() + b.abs())
        d = (layers[l].double() - ref).abs()
        print(f"{what} conv{l + 1}: max |d| {float(d.max()):.3e}, max |d| / bound {float((d / bound).max()):.3f}")
        assert bool((d <= bound).all()), f"{what}: conv layer {l + 1} off its bound at {int((d > bound).sum())} elements"
        x = layers[l].double()
    w = lin.weight.detach().double()
    flat = x.flatten(1)
    ref = flat @ w.t() + lin.bias.detach().double()
    bound = 4096 * 2.0 ** -23 * (flat.abs() @ w.abs().t()) + 2.0 ** -22 * ref.abs()
    d = (out.double() - ref).abs()
    print(f"{what} linear: max |d| {float(d.max()):.3e}, max |d| / bound {float((d / bound).max()):.3f}")
    assert bool((d <= bound).all()), f"{what}: the Linear off its bound at {int((d > bound).sum())} elements"


@pytest.mark.parametrize("H", (32, 192))
@pytest.mark.parametrize("n", (5, 37))
def test_layers_within_derived_bound(H, n):
    """Every layer of ours against the float64 layer applied to OUR previous activation -- the
    test that catches a wrong tap, stride, padding edge or fragment order, one layer at a time.

    Bound, conv layers:  |d| <= |a_c| K 2^-23 sum|w x| + 2^-21 (|a_c r| + |b_c|), r the float64 ReLU
    output, sum|w x| the same convolution run on |w|, |x|, K = 16 cin.
    Bound, the Linear:   |d| <= 4096 2^-23 sum|w x| + 2^-22 |out|.
    Derivation: a length-K fp32 fmaf chain in ANY order errs by at most K u sum|w x| with u = 2^-24
    (each partial sum is rounded once, and is itself bounded by sum|w x| to first order); taken
    twice for slack, K 2^-23 sum|w x|.  ReLU is 1-Lipschitz, so the chain's error passes through
    it undiminished at most, and the affine scales it by |a_c|.  The affine a relu + b adds the
    host fold's roundings of a and b (u |a r|, u |b|) and the device fma's own (u |a r + b|):
    under 2^-23 (|a r| + |b|), taken four times for slack.  The Linear's bias add is one rounding,
    u |out|, taken four times.  Nothing here is measured."""
    from nfdpf import ops
    c = _case(H)
    if n == 37:
        out, layers = c.out, c.layers
    else:  # a ragged part of one row tile, as a [n, 1] call
        o, ls = ops.frame_encoder(c.blob, c.dev_frames[:n, None], H, keep_layers=True)
        out, layers = o[:, 0].cpu(), [l[:, 0].cpu() for l in ls]
    assert out.shape == (n, H) and [tuple(l.shape[1:]) for l in layers] == \
        [(16, 64, 64), (32, 32, 32), (64, 16, 16), (128, 8, 8), (256, 4, 4)]
    _check_layers(c.enc, c.frames[:n], out, layers, f"H={H} n={n}")


# ----------------------------------------------------------------------------------------------
# 3. end to end
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", (32, 192))
def test_end_to_end_against_float64(H):
    """37 frames through all six layers against float64 CPU PyTorch; float32 CPU PyTorch's own
    error err32 sizes the bar: every element within 4 |err32| + 2e-4 max|ref| (the per-element
    term of _check in test_gpu_cglow_levels_backward.py, applied to ALL elements)."""
    c = _case(H)
    with torch.no_grad():
        ref = copy.deepcopy(c.enc).double()(c.frames.double())
        err32 = (c.enc(c.frames).double() - ref).abs()
    d = (c.out.double() - ref).abs()
    bar = 4 * err32 + 2e-4 * float(ref.abs().max())
    print(f"H={H}: max |d| {float(d.max()):.3e}, max err32 {float(err32.max()):.3e}, max|ref| {float(ref.abs().max()):.3e}")
    assert bool((d <= bar).all()), f"{int((d > bar).sum())} of {d.numel()} elements off the bar"


# ----------------------------------------------------------------------------------------------
# 4. placement independence and repeatability
# ----------------------------------------------------------------------------------------------
def test_placement_independence_and_repeatability():
    """A frame's encoding is one fmaf chain fixed by its own indices: the same bits alone, in a
    [1, 37] or a [37, 1] call, in a second identical call, and in a call of more than one chunk."""
    from nfdpf import ops
    c = _case(32)
    base = c.out
    again = ops.frame_encoder(c.blob, c.dev_frames[None], 32)
    assert torch.equal(again[0].cpu(), base)
    col = ops.frame_encoder(c.blob, c.dev_frames[:, None], 32)
    assert torch.equal(col[:, 0].cpu(), base)
    solo = {}
    for j in (0, 17, 33, 34, 36):
        solo[j] = ops.frame_encoder(c.blob, c.dev_frames[j][None, None], 32)[0, 0].cpu()
    for j in (0, 17, 36):
        assert torch.equal(solo[j], base[j]), j
    # one call of CHUNK + 3 frames: the last of the first chunk, the first and the last of the second
    idx = torch.arange(CHUNK + 3) % 37
    big = ops.frame_encoder(c.blob, c.dev_frames[idx.to(DEV)][None], 32)[0].cpu()
    for j in (CHUNK - 1, CHUNK, CHUNK + 2):
        assert torch.equal(big[j], solo[int(idx[j])]), j
    assert torch.equal(big[:37], base)


def test_capturable_in_a_graph():
    """Stream-ordered, no allocation or synchronisation inside the library: the call is captured
    into a graph and replayed on new frames, with the bits of the plain call."""
    from nfdpf import ops
    c = _case(32)
    static = c.dev_frames[:5][None].clone()
    ops.frame_encoder(c.blob, static, 32)  # (the cached workspace exists before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.frame_encoder(c.blob, static, 32)
    static.copy_(c.dev_frames[5:10][None])
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0].cpu(), c.out[5:10])


# ----------------------------------------------------------------------------------------------
# 5. strides
# ----------------------------------------------------------------------------------------------
def test_strided_frames_and_output():
    from nfdpf import ops
    c = _case(32)
    obs = c.dev_frames[:21].reshape(3, 7, 3, 128, 128)
    view = obs[:, :5]
    assert not view.is_contiguous()
    ref = ops.frame_encoder(c.blob, view.contiguous(), 32)
    got = ops.frame_encoder(c.blob, view, 32)
    assert torch.equal(got, ref)
    assert torch.equal(ref.cpu(), c.out[:21].reshape(3, 7, 32)[:, :5])
    buf = torch.full((3, 9, 32), 7.0, device=DEV)
    ret = ops.frame_encoder(c.blob, view, 32, out=buf[:, :5])
    assert ret.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:, :5], ref) and bool((buf[:, 5:] == 7.0).all())


# ----------------------------------------------------------------------------------------------
# 6. routing
# ----------------------------------------------------------------------------------------------
def _dpf(measurement, H, B, N, T):
    from arguments import parse_args
    from DPFs import DPF
    a = parse_args([])
    a.NF_dyn, a.NF_cond, a.measurement, a.resampler_type = True, True, measurement, "soft"
    a.hiddensize, a.num_particles, a.batchsize, a.sequence_length = H, N, B, T
    torch.manual_seed(3)
    dpf = DPF(a)
    trained_like(dpf.encoder)
    return dpf.to(DEV).eval()


class _Spy:
    def __init__(self, fn):
        self.fn, self.calls, self.ret = fn, 0, None

    def __call__(self, *a, **k):
        self.calls += 1
        self.ret = self.fn(*a, **k)
        return self.ret


def _inputs(B, T, extra=2):
    g = torch.Generator().manual_seed(8)
    obs = torch.rand(B, T + extra, 3, 128, 128, generator=g)  # longer than the filter reads: obs[:, :T] in place
    start = torch.cat([torch.rand(B, 2, generator=g) * 100, torch.randn(B, 2, generator=g)], 1)
    vel = torch.randn(B, T + extra, 2, generator=g)
    return obs, start, vel


@pytest.mark.parametrize("measurement,H", [("cos", 32), ("CGLOW", 192)])
def test_filtering_pos_routes_to_the_hip_encoder(measurement, H, monkeypatch):
    """DPF.filtering_pos with its real encoder, eval mode, no_grad: exactly one ops.frame_encoder
    call, whose encodings equal the module's own loop on a CPU copy within bar 1's tolerance."""
    from nfdpf import ops
    B, N, T = 2, 64, 3
    dpf = _dpf(measurement, H, B, N, T)
    obs, start, vel = _inputs(B, T)
    spy = _Spy(ops.frame_encoder)
    monkeypatch.setattr(ops, "frame_encoder", spy)
    monkeypatch.delenv("NFDPF_HIP_ENCODER", raising=False)  # the default: on
    with torch.no_grad():
        out = dpf.filtering_pos(obs.to(DEV), start.to(DEV), vel.to(DEV))
    torch.cuda.synchronize()
    assert spy.calls == 1
    cpu_enc = copy.deepcopy(dpf.encoder).cpu()
    with torch.no_grad():
        ref = torch.stack([cpu_enc(obs[:, t]) for t in range(T)], dim=1)
    assert spy.ret.shape == (B, T, H)
    np.testing.assert_allclose(spy.ret.cpu().numpy(), ref.numpy(), rtol=2e-4, atol=2e-5)
    particles, weights = out[0], out[1]
    assert particles.shape == (B, T, N, 2) and weights.shape == (B, T, N)
    assert bool(torch.isfinite(particles).all()) and bool(torch.isfinite(weights).all())


@pytest.fixture(scope="module")
def _route_dpf():
    return _dpf("cos", 32, 1, 64, 2)


@pytest.mark.parametrize("case", ["env_off", "train", "autograd", "identity", "tiny"])
def test_other_paths_keep_their_loop(case, monkeypatch, _route_dpf):
    """Everything but (real conv stack, eval, no autograd, switch on) keeps the parent's loop: no
    ops.frame_encoder call, and _frame_encodings returns what the loop restated here returns."""
    from _tiny import TinyEncoder
    from nfdpf import ops
    dpf, B, T = _route_dpf, 1, 2
    obs = _inputs(B, T)[0].to(DEV)
    spy = _Spy(ops.frame_encoder)
    monkeypatch.setattr(ops, "frame_encoder", spy)
    monkeypatch.delenv("NFDPF_HIP_ENCODER", raising=False)
    real = dpf.encoder
    grad = False
    if case == "env_off":
        monkeypatch.setenv("NFDPF_HIP_ENCODER", "0")
    elif case == "train":
        monkeypatch.setattr(dpf, "encoder", copy.deepcopy(real).train())
    elif case == "autograd":
        grad = True
    elif case == "identity":
        monkeypatch.setattr(dpf, "encoder", nn.Identity())
        obs = torch.rand(B, T + 2, 32, generator=torch.Generator().manual_seed(9)).to(DEV)
    elif case == "tiny":
        torch.manual_seed(4)
        monkeypatch.setattr(dpf, "encoder", TinyEncoder(32).to(DEV).eval())
    with torch.set_grad_enabled(grad):
        got = dpf._frame_encodings(obs, T)
        if case == "identity":
            want = obs[:, :T].float()
        else:
            want = torch.stack([dpf.encoder(obs[:, t].float()) for t in range(T)], dim=1)
    torch.cuda.synchronize()
    assert spy.calls == 0
    assert got.shape == want.shape and torch.equal(got, want)
    if case == "autograd":
        assert got.requires_grad


# ----------------------------------------------------------------------------------------------
# 7. refusals
# ----------------------------------------------------------------------------------------------
def test_refusals():
    from nfdpf import _lib, ops
    from nfdpf._lib import NfdpfError, ptr
    c = _case(32)
    lib = _lib.lib()
    frames = c.dev_frames[:1][None]
    out = torch.full((1, 1, 32), 7.0, device=DEV)
    ws = torch.empty(int(lib.nfdpf_frame_encoder_workspace_bytes(1)), dtype=torch.uint8, device=DEV)
    st = _lib.stream_ptr(DEV)
    n = 3 * 128 * 128

    def call(params, H, B, T):
        return lib.nfdpf_frame_encoder(params, H, ptr(frames), B, T, n, n, ptr(out), 32, 32, None, ptr(ws), st)
    assert call(ptr(c.blob), 48, 1, 1) == _lib.NFDPF_EINVAL and b"48" in lib.nfdpf_last_error()
    assert call(ptr(c.blob), 32, -1, 1) == _lib.NFDPF_EINVAL and b"negative" in lib.nfdpf_last_error()
    assert call(None, 32, 1, 1) == _lib.NFDPF_EINVAL and b"null" in lib.nfdpf_last_error()
    assert call(ptr(c.blob), 32, 0, 5) == _lib.NFDPF_OK and call(ptr(c.blob), 32, 5, 0) == _lib.NFDPF_OK
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(ptr(c.blob), 32, 1, 1) == _lib.NFDPF_OK  # (the same call with good arguments does write)
    torch.cuda.synchronize()
    assert torch.equal(out[0, 0].cpu(), c.out[0])
    assert ops.frame_encoder(c.blob, c.dev_frames[:0][None], 32).shape == (1, 0, 32)
    with pytest.raises(NfdpfError, match="blob"):
        ops.frame_encoder(c.blob[:-1], frames, 32)
    with pytest.raises(NfdpfError, match="blob"):
        ops.frame_encoder(c.blob, frames, 192)
    with pytest.raises(NfdpfError, match="float32"):
        ops.frame_encoder(c.blob, frames.double(), 32)
    with pytest.raises(NfdpfError, match="HIP device"):
        ops.frame_encoder(c.blob, frames.cpu(), 32)
    with pytest.raises(NfdpfError, match="widths"):
        ops.frame_encoder(c.blob, frames, 48)
