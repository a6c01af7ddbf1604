"""The frame encoder's parameter blob (nfdpf.pack.frame_encoder_tensors; layout:
csrc/frame_enc.hpp) on the CPU: its size against the library's query, the BatchNorm fold, the
cache key that follows the running statistics, and the packed order read back the way the
kernel reads it."""
import pytest
import torch
from torch import nn

from _frame_enc import stack as _stack, trained_like as _trained_like

WIDTHS = (16, 32, 64, 192)
CHANNELS = (3, 16, 32, 64, 128, 256)


@pytest.mark.parametrize("H", WIDTHS)
def test_blob_size_matches_library(H):
    from nfdpf import _lib
    from nfdpf.pack import frame_encoder_tensors
    n = sum(t.numel() for t in frame_encoder_tensors(_stack(H)))
    assert n == int(_lib.load().nfdpf_frame_encoder_params_size(H))
    assert n == sum(16 * a * b + 2 * b for a, b in zip(CHANNELS[:-1], CHANNELS[1:])) + 4096 * H + H


@pytest.mark.parametrize("H", (0, 8, 48, 256))
def test_size_query_refuses_other_widths(H):
    from nfdpf import _lib
    assert int(_lib.load().nfdpf_frame_encoder_params_size(H)) == -1


def test_workspace_query():
    from nfdpf import _lib
    lib = _lib.load()
    per = 4 * (16 * 64 * 64 + 32 * 32 * 32)
    assert int(lib.nfdpf_frame_encoder_workspace_bytes(5)) >= 5 * per
    # one chunk's worth however many frames the call has
    assert int(lib.nfdpf_frame_encoder_workspace_bytes(3200)) == int(lib.nfdpf_frame_encoder_workspace_bytes(256))
    assert int(lib.nfdpf_frame_encoder_workspace_bytes(-1)) == -1


def test_argument_errors_without_device():
    """Bad arguments are refused before any launch (so this needs no GPU)."""
    from nfdpf import _lib
    lib = _lib.load()
    assert lib.nfdpf_frame_encoder(None, 48, None, 1, 1, 0, 0, None, 0, 0, None, None, None) == _lib.NFDPF_EINVAL
    assert b"48" in lib.nfdpf_last_error()
    assert lib.nfdpf_frame_encoder(None, 32, None, -1, 1, 0, 0, None, 0, 0, None, None, None) == _lib.NFDPF_EINVAL
    assert b"negative" in lib.nfdpf_last_error()
    assert lib.nfdpf_frame_encoder(None, 32, None, 1, 1, 0, 0, None, 0, 0, None, None, None) == _lib.NFDPF_EINVAL
    assert b"null" in lib.nfdpf_last_error()
    assert lib.nfdpf_frame_encoder(None, 32, None, 0, 7, 0, 0, None, 0, 0, None, None, None) == _lib.NFDPF_OK


def test_bn_fold_reproduces_eval_batchnorm():
    """y = a x + b against BatchNorm2d.eval() to 4 ulp of the larger term: the module computes
    (x - mean) / sqrt(var + eps) * gamma + beta, the fold a x + b with a, b rounded once each --
    a handful of roundings either way, each relative to a term no larger than max(|a x|, |b|,
    |y|)."""
    from nfdpf.pack import bn_fold
    g = torch.Generator().manual_seed(5)
    bn = nn.BatchNorm2d(32)
    with torch.no_grad():
        bn.weight.copy_(torch.empty(32).uniform_(0.5, 1.5, generator=g))
        bn.bias.copy_(torch.randn(32, generator=g) * 0.2)
        bn.running_mean.copy_(torch.empty(32).uniform_(0.0, 0.5, generator=g))
        bn.running_var.copy_(torch.empty(32).uniform_(0.5, 2.0, generator=g))
    bn.eval()
    x = torch.randn(3, 32, 8, 8, generator=g)
    a, b = bn_fold(bn)
    assert a.dtype == torch.float32 and b.dtype == torch.float32
    with torch.no_grad():
        ref = bn(x)
    ours = a[None, :, None, None] * x + b[None, :, None, None]
    larger = torch.maximum(torch.maximum((a[None, :, None, None] * x).abs(), b[None, :, None, None].abs().expand_as(x)),
                           ref.abs())
    assert bool(((ours - ref).abs() <= 4 * 2.0 ** -23 * larger).all())


def test_train_mode_forward_repacks():
    """A train-mode forward changes the running statistics and no parameter: the cache key lists
    the buffers, so pack.blob must return a different blob."""
    from nfdpf.pack import blob, frame_encoder_sources, frame_encoder_tensors
    enc = _stack(16)
    owner = nn.Module()
    cpu = torch.device("cpu")
    get = lambda: blob(owner, "frame_encoder", frame_encoder_sources(enc), lambda: frame_encoder_tensors(enc), cpu)  # noqa: E731
    b0 = get()
    assert get() is b0  # unchanged module: the cached blob
    params = [p.detach().clone() for p in enc.parameters()]
    enc.train()
    with torch.no_grad():
        enc(torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(1)))
    enc.eval()
    assert all(torch.equal(p, q) for p, q in zip(params, enc.parameters()))
    b1 = get()
    assert b1 is not b0 and b1.shape == b0.shape and not torch.equal(b1, b0)
    # and only the folded (a, b) moved: conv1's weights are the blob's first 768 floats
    assert torch.equal(b1[:768], b0[:768])


def _unpack(frag, K, N, bn):
    """Read a frame_enc_frag block back the way the kernel's lanes do (csrc/frame_enc.hpp)."""
    f = frag.reshape(N // bn, K // 16, bn // 16, 64, 4)
    wk = torch.empty(K, N, dtype=frag.dtype)
    for lane in range(64):
        g, r = lane >> 4, lane & 15
        for i in range(4):
            # k = 16 q + 4 g + i for every q; n = bn nb + 16 nt + r for every (nb, nt)
            blk = f[:, :, :, lane, i]  # [nb][q][nt]
            wk[4 * g + i::16, r::16] = blk.permute(1, 0, 2).reshape(K // 16, N // 16)
    return wk


@pytest.mark.parametrize("H", (32, 192))
def test_blob_read_in_kernel_order_reproduces_the_module(H):
    """The blob, read back by the documented fragment map and applied as the kernel applies it --
    a GEMM over k = (4 kh + kw) cin + c on channels-last activations with zero padding, then
    a relu + b; the Linear over k = 256 (4 h + w) + c -- reproduces the eval-mode module on a
    frame (float64 GEMMs, so only the fold's and the module's own float32 rounding remain)."""
    from nfdpf.pack import frame_encoder_tensors
    enc = _trained_like(_stack(H)).eval()
    ts = frame_encoder_tensors(enc)
    x = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        ref = enc(x)
    act = x[0].permute(1, 2, 0).double()  # [h][w][c]
    for l in range(5):
        cin, cout = CHANNELS[l], CHANNELS[l + 1]
        wk = _unpack(ts[3 * l], 16 * cin, cout, min(cout, 64)).double()
        a, b = ts[3 * l + 1].double(), ts[3 * l + 2].double()
        hi = act.shape[0]
        pad = torch.zeros(hi + 2, hi + 2, cin, dtype=torch.float64)
        pad[1:-1, 1:-1] = act
        ho = hi // 2
        cols = torch.stack([pad[kh:kh + 2 * ho:2, kw:kw + 2 * ho:2] for kh in range(4) for kw in range(4)], dim=2)
        A = cols.reshape(ho * ho, 16 * cin)  # k = (4 kh + kw) cin + c
        act = (a * torch.relu(A @ wk) + b).reshape(ho, ho, cout)
    wk = _unpack(ts[15], 4096, H, 16).double()
    out = act.reshape(1, 4096) @ wk + ts[16].double()
    assert torch.allclose(out.float(), ref, rtol=2e-4, atol=2e-5)


def test_structure_check_accepts_only_the_conv_stack():
    """nfdpf.ops.frame_encoder_width: H for exactly model.models._conv_stack(H) with H built, None
    for anything else; frame_encoder_supported is false off the device."""
    from _tiny import TinyEncoder
    from nfdpf import ops
    for H in WIDTHS:
        assert ops.frame_encoder_width(_stack(H)) == H
    assert ops.frame_encoder_width(_stack(48)) is None  # a width the library is not built for
    assert ops.frame_encoder_width(nn.Identity()) is None
    assert ops.frame_encoder_width(TinyEncoder(32)) is None
    enc = _stack(32)
    enc[3] = nn.Conv2d(16, 32, kernel_size=4, stride=2, padding=1, bias=True)
    assert ops.frame_encoder_width(enc) is None
    enc = _stack(32)
    enc[5] = nn.BatchNorm2d(32, track_running_stats=False)
    assert ops.frame_encoder_width(enc) is None
    enc = _stack(32)
    enc[1] = nn.LeakyReLU()
    assert ops.frame_encoder_width(enc) is None
    assert ops.frame_encoder_width(_stack(32).double()) is None
    assert not ops.frame_encoder_supported(_stack(32).eval(), torch.zeros(1, 1, 3, 128, 128))  # a CPU tensor
