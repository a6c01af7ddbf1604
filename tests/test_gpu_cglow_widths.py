"""The conditional-GLOW measurement and flow at the hidden sizes of csrc/cglow_widths.hpp
(--x_hidden_channels XH in {8, 16}, --x_hidden_size XS in {16, 32}, --y_hidden_channels YH in
{8, 16, 32}) and at other --y_bins on the width-general HIP kernel (csrc/cglow_wide.hip),
against the reference's own runs at these sizes (tests/golden/cglow_widths.npz,
cglow_widths_l2.npz; tests/golden/gen_cglow_widths.py).  GPU box only.

The bounds are those of test_gpu_cglow_levels.py, unchanged: elementwise z |d| <= max(1e-5 |ref|
+ 2e-5, 4 x the fixture's err_abs/z), nll |d| <= max(1e-5 |ref| + 2e-6, 4 x err_abs/nll), and
against the float64 values at most 4 x the reference's own float32 error; lik:
assert_close(1e-5, 5e-5) after the row-max shift, widened by the same 4 x term; gradients:
test_gpu_cglow_depth._grad_close.  The fixtures' per-sample 1x1-conv matrices have cond(W) <=
124 (asserted < 2e4 by the generator), so log|det W| is a fair yardstick in float32.

The figures measured on an MI355X are in the tests' docstrings (each test prints its own)."""
import itertools

import numpy as np
import pytest
import torch

from _util import assert_close, group, load, t, weights
from test_gpu_cglow_depth import _grad_close, _param_grads_close, _vs_f64
from test_gpu_cglow_levels import _close_or_ref_err, _count, _forward_bounds, _pe_blob

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FX = {}
DEFAULT = (8, 16, 8)
# the fixtures: case -> ((XH, XS, YH), K, L, learn_top, y_bins)
CASES = {
    "a": ((16, 32, 16), 1, 1, False, 256),
    "b": ((8, 16, 32), 2, 2, True, 256),
    "c": ((16, 32, 32), 1, 2, True, 256),
    "d": ((8, 16, 8), 1, 1, False, 32),
    "e": ((16, 16, 8), 1, 1, False, 256),
}
NO_FIXTURE = [w for w in itertools.product((8, 16), (16, 32), (8, 16, 32)) if w not in {c[0] for c in CASES.values()}]
BACKWARDS = ("cglow_flow_backward", "cglow_measurement_backward", "cglow_levels_flow_backward",
             "cglow_levels_measurement_backward")


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from nfdpf import _lib
    _lib.load()
    assert torch.cuda.is_available()
    FX.update(load("cglow_widths.npz"))
    FX.update(load("cglow_widths_l2.npz"))


def _args(widths=DEFAULT, K=1, L=1, top=False, bins=256, **kw):
    from arguments import parse_args
    a = parse_args([])
    a.x_hidden_channels, a.x_hidden_size, a.y_hidden_channels = widths
    a.flow_depth, a.num_levels, a.learn_top, a.y_bins = K, L, top, bins
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _fixture_model(case):
    """This package's CondGlowModel holding the reference's weights of a fixture."""
    from nf.cglow.CGlowModel import CondGlowModel
    m = CondGlowModel(_args(*CASES[case]))
    m.load_state_dict(weights(group(FX, case)))
    return m.to(DEV)


def _random_model(widths, K, L, top, seed, bins=256):
    """Seeded init, every parameter replaced by N(0, 0.1^2) draws (as the fixture generator)."""
    from nf.cglow.CGlowModel import CondGlowModel
    torch.manual_seed(seed)
    m = CondGlowModel(_args(widths, K, L, top, bins))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        if not top:
            m.new_mean.zero_()
            m.new_logs.zero_()
    return m


def _blob(m):
    from nfdpf.pack import cglow_levels_tensors
    return torch.cat([a.detach().reshape(-1) for a in cglow_levels_tensors(m)]).contiguous()


def _max_cond(m, x):
    """max over steps and samples of cond(W) of the per-sample 1x1-conv matrix, in float64 on the CPU."""
    import copy
    md = copy.deepcopy(m).cpu().double()
    worst = 0.0
    with torch.no_grad():
        for layer in md.flow.layers:
            inv = getattr(layer, "invconv", None)
            if inv is not None:
                w = inv.x_Linear(inv.x_Con(x.cpu().double()).view(x.size(0), -1))
                C = int(round(w.size(1) ** 0.5))
                worst = max(worst, float(torch.linalg.cond(w.view(-1, C, C)).max()))
    return worst


# ---- 1. flow forward vs the reference ----
@pytest.mark.parametrize("case", sorted(CASES))
def test_flow_forward_vs_reference(case):
    """Measured on an MI355X, max |ours - ref32| (z, nll) and max |ours - f64| (nll, z) against
    the reference's own float32 error:
      a: z 2.4e-7, nll 1.9e-6; f64: nll 8.1e-7 (reference 1.4e-6), z 2.6e-7 (1.9e-7)
      b: z 1.0e-7, nll 1.9e-6; f64: nll 1.8e-6 (reference 2.2e-6), z 9.8e-8 (8.4e-8)
      c: z 1.8e-7, nll 1.9e-6; f64: nll 1.1e-6 (reference 1.7e-6), z 1.9e-7 (1.4e-7)
      d: z 3.6e-7, nll 1.9e-6; f64: nll 1.1e-6 (reference 1.9e-6), z 4.0e-7 (1.8e-7)
      e: z 2.4e-7, nll 9.5e-7; f64: nll 9.1e-7 (reference 1.5e-6), z 2.2e-7 (1.7e-7)"""
    from nfdpf import ops
    widths, K, L, top, bins = CASES[case]
    fx = group(FX, case)
    m = _fixture_model(case)
    assert m.wide_kernel_supported() and not m.kernel_supported() and not m.levels_kernel_supported()
    x, y = t(fx["x"]).to(DEV), t(fx["y"]).to(DEV)
    with torch.no_grad():
        z, nll = m(x, y)
    zk, nk = ops.cglow_wide_flow(_blob(m), x, y, K=K, L=L, learn_top=top, widths=widths, y_bins=bins)
    assert torch.equal(z, zk) and torch.equal(nll, nk), "CondGlowModel.forward is not the width-general kernel"
    z, nll = z.cpu().numpy(), nll.cpu().numpy()
    assert z.shape == fx["z"].shape
    z64 = fx["z"].astype(np.float64) + fx["f64d/z"].astype(np.float64)
    _forward_bounds(z, nll, fx["z"], fx["nll"], fx["err_abs/z"], fx["err_abs/nll"], f"case {case} {widths}")
    _vs_f64(nll, fx["f64/nll"], fx["err_abs/nll"], f"case {case} nll")
    _vs_f64(z, z64, fx["err_abs/z"], f"case {case} z")


# ---- 2. bins ----
def test_bins_shift_nll_by_three_bits():
    """Case d (the default sizes, y_bins = 32) is within test 1's bounds of its fixture; the same
    weights at y_bins = 256 on the levels kernel give nll exactly log2(256 / 32) = 3.0 higher,
    within 2e-6, and the same z within test 1's bound.
    Measured on an MI355X: max |nll(256) - nll(32) - 3| 1.9e-6 (one float32 ulp of nll, 8 .. 16),
    max |z - z(levels kernel)| 1.2e-7."""
    from nfdpf import ops
    fx = group(FX, "d")
    m = _fixture_model("d")
    x, y = t(fx["x"]).to(DEV), t(fx["y"]).to(DEV)
    with torch.no_grad():
        z, nll = m(x, y)
    _forward_bounds(z.cpu().numpy(), nll.cpu().numpy(), fx["z"], fx["nll"], fx["err_abs/z"], fx["err_abs/nll"], "case d")
    z2, n2 = ops.cglow_levels_flow(_blob(m), x, y, K=1, L=1, learn_top=False)
    d = (n2.double() - nll.double() - 3.0).abs().max().item()
    print(f"bins: max |nll(256, levels kernel) - nll(32) - 3| {d:.3e}, max |z - z(levels kernel)| "
          f"{(z2 - z).abs().max().item():.3e}")
    assert d <= 2e-6
    _close_or_ref_err(z.cpu(), z2.cpu(), 1e-5, 2e-5, fx["err_abs/z"], "z vs the levels kernel")


# ---- 3. the triples without a fixture ----
@pytest.mark.parametrize("widths", NO_FIXTURE, ids=lambda w: "-".join(map(str, w)))
def test_flow_forward_vs_float64_restatement(widths):
    """(K, L, top) = (1, 2, on), M = 37, against this package's torch_forward in float64 on the
    CPU (test_cglow_widths_pack pins it to the reference), with the float32 torch_forward's own
    error against float64 in the place of the fixture's err_abs.
    Measured on an MI355X, max |nll - f64| (the float32 restatement's), max |z - f64| (its):
      (8, 16, 16):  nll 1.1e-6 (2.0e-6), z 1.9e-7 (1.8e-7)
      (8, 32, 8):   nll 1.5e-6 (1.9e-6), z 1.5e-7 (1.5e-7)
      (8, 32, 16):  nll 7.5e-6 (4.9e-6), z 2.2e-7 (2.2e-7)
      (8, 32, 32):  nll 1.2e-6 (1.8e-6), z 2.4e-7 (1.7e-7)
      (16, 16, 16): nll 1.2e-6 (1.9e-6), z 1.7e-7 (1.4e-7)
      (16, 16, 32): nll 1.0e-6 (1.8e-6), z 1.4e-7 (1.3e-7)
      (16, 32, 8):  nll 9.8e-7 (1.6e-6), z 2.4e-7 (1.4e-7)"""
    import copy
    assert len(NO_FIXTURE) == 7
    K, L, top = 1, 2, True
    # (the seeds' base was chosen on the CPU for the condition below: cond(W) <= 3.3e3 over the seven)
    m = _random_model(widths, K, L, top, 7600 + 100 * widths[0] + 10 * widths[1] + widths[2])
    g = torch.Generator().manual_seed(9)
    M = 37
    x, y = torch.randn(M, 3, 8, 8, generator=g), torch.randn(M, 3, 8, 8, generator=g)
    assert _max_cond(m, x) < 2e4
    with torch.no_grad():
        z32, n32 = m.torch_forward(x, y)
        z64, n64 = copy.deepcopy(m).double().torch_forward(x.double(), y.double())
    err_z = float((z32.double() - z64).abs().max())
    err_n = float((n32.double() - n64).abs().max())
    m = m.to(DEV)
    assert m.wide_kernel_supported() and not m.levels_kernel_supported()
    with torch.no_grad():
        z, nll = m(x.to(DEV), y.to(DEV))
    z, nll = z.cpu().numpy(), nll.cpu().numpy()
    assert z.shape == (M, 24, 2, 2)
    _forward_bounds(z, nll, z64.numpy(), n64.numpy(), err_z, err_n, f"{widths} vs float64")
    _vs_f64(nll, n64.numpy(), err_n, f"{widths} nll")
    _vs_f64(z, z64.numpy(), err_z, f"{widths} z")


# ---- 4. measurement form ----
def _meas_dpf(bins=256, **kw):
    from DPFs import DPF
    torch.manual_seed(0)
    kw = dict(dict(num_particles=21, batchsize=3), **kw)
    dpf = DPF(_args((16, 32, 16), 1, 1, False, bins, measurement="CGLOW", hiddensize=192, **kw))
    sd = dpf.state_dict()
    w = weights(group(FX, "meas"))
    assert set(w) <= set(sd)
    sd.update(w)
    dpf.load_state_dict(sd)
    return dpf.to(DEV)


def test_measurement_forward():
    """a's sizes, B = 3 rows of N = 21 particles, the encodings' rows strided (a [B, T, 192] view).
    Measured on an MI355X: max |lik - ref32| 1.9e-6; max |lik - f64| 2.1e-6, the reference's 1.9e-6."""
    from nfdpf import ops
    fx = group(FX, "meas")
    dpf = _meas_dpf()
    pe, glow = _pe_blob(dpf.particle_encoder), _blob(dpf.cglow_measurement)
    x = t(fx["x"]).to(DEV)
    enc3 = torch.full((3, 4, 192), 9.0, device=DEV)
    enc3[:, 2] = t(fx["enc"]).to(DEV)
    enc = enc3[:, 2]
    assert enc.stride(0) == 4 * 192
    kw = dict(K=1, L=1, learn_top=False, widths=(16, 32, 16), y_bins=256)
    raw = ops.cglow_wide_measurement(pe, glow, enc, x, **kw)
    lik = (raw - raw.max(dim=-1, keepdim=True)[0]).cpu().numpy()
    print(f"meas a: max |lik - ref32| {np.abs(lik - fx['lik']).max():.3e}; "
          f"max |lik - f64| {np.abs(lik - fx['f64/lik']).max():.3e}, the reference's {float(fx['err_abs/lik']):.3e}")
    _close_or_ref_err(lik, fx["lik"], 1e-5, 5e-5, fx["err_abs/lik"], "CGLOW a lik")
    assert torch.equal(raw, ops.cglow_wide_measurement(pe, glow, enc.contiguous(), x, **kw)), "strided rows"
    # into out= (rows of a wider buffer): identical bits, nothing else written
    buf = torch.full((3, 32), 7.0, device=DEV)
    out = buf[:, 5:26]
    assert ops.cglow_wide_measurement(pe, glow, enc, x, out=out, **kw) is out
    assert torch.equal(out, raw) and bool((buf[:, :5] == 7.0).all()) and bool((buf[:, 26:] == 7.0).all())
    # and through the module API: the same bits
    with torch.no_grad():
        lik2 = dpf.measurement_model(enc, x)
    assert np.array_equal(lik2.cpu().numpy(), lik)


# ---- 5. persistent tiles and placement ----
def test_persistent_tiles_and_placement():
    """Case c's configuration ((16, 32, 32), K = 1, L = 2, top on), M = 4 x CUs x 16 + 21 samples:
    every workgroup (one per CU) runs more than one tile and the last tile is ragged (5 of 16).
    The PyTorch restatement on the device is evaluated on tiles 0-2, one tile in the middle and
    the last two tiles, within test 1's bounds with case c's recorded float32 error.  The first
    37 samples equal an M = 37 call bit for bit; a sample keeps its bits at another index; M = 1
    works; M = 0 returns empty outputs.
    Measured on an MI355X: M = 16 405; max |z - torch| 2.7e-7, max |nll - torch| 2.9e-6 on the 101 samples."""
    from nfdpf import ops
    widths, K, L, top, bins = CASES["c"]
    kw = dict(K=K, L=L, learn_top=top, widths=widths, y_bins=bins)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M = 4 * cus * 16 + 21
    m = _random_model(widths, K, L, top, 77).to(DEV)
    blob = _blob(m)
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(M, 3, 8, 8, generator=g).to(DEV), torch.randn(M, 3, 8, 8, generator=g).to(DEV)
    z, nll = ops.cglow_wide_flow(blob, x, y, **kw)
    assert tuple(z.shape) == (M, 24, 2, 2)
    mid = 16 * (2 * cus)
    sel = torch.cat([torch.arange(0, 48), torch.arange(mid, mid + 16), torch.arange(4 * cus * 16 - 16, M)]).to(DEV)
    with torch.no_grad():
        zr, nr = m.torch_forward(x[sel], y[sel])
    fx = group(FX, "c")
    _forward_bounds(z[sel].cpu(), nll[sel].cpu(), zr.cpu(), nr.cpu(), fx["err_abs/z"], fx["err_abs/nll"],
                    f"M={M}, {sel.numel()} samples vs torch")
    z37, n37 = ops.cglow_wide_flow(blob, x[:37].contiguous(), y[:37].contiguous(), **kw)
    assert torch.equal(z37, z[:37]) and torch.equal(n37, nll[:37]), "the first 37 samples depend on M"
    # sample 5 moved to index M - 3 (another tile, another lane group, another workgroup)
    perm = torch.arange(M, device=DEV)
    perm[5], perm[M - 3] = M - 3, 5
    zp, np_ = ops.cglow_wide_flow(blob, x[perm].contiguous(), y[perm].contiguous(), **kw)
    assert torch.equal(zp[M - 3], z[5]) and torch.equal(np_[M - 3], nll[5]), "a sample's bits depend on its index"
    assert torch.equal(zp[perm], z) and torch.equal(np_[perm], nll)
    z1, n1 = ops.cglow_wide_flow(blob, x[11:12].contiguous(), y[11:12].contiguous(), **kw)
    assert torch.equal(z1[0], z[11]) and torch.equal(n1[0], nll[11]), "M = 1"
    z0, n0 = ops.cglow_wide_flow(blob, x[:0].contiguous(), y[:0].contiguous(), **kw)
    assert tuple(z0.shape) == (0, 24, 2, 2) and tuple(n0.shape) == (0,)


# ---- 6. the inference filter stays one engine call ----
def test_engine_path_wide_other_bins():
    """DPF at a's sizes with y_bins = 64: filtering_pos runs the engine, whose likelihood history
    is the width-general kernel's on the recorded particles, bit for bit."""
    from DPFs import DPF
    from nfdpf import ops
    B, N, T = 2, 40, 3
    widths, bins = (16, 32, 16), 64
    torch.manual_seed(5)
    dpf = DPF(_args(widths, 1, 1, False, bins, measurement="CGLOW", hiddensize=192, num_particles=N, batchsize=B,
                    sequence_length=T))
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for p in dpf.cglow_measurement.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    dpf.encoder = torch.nn.Identity()
    dpf.to(DEV).eval()
    assert dpf._fused_supported()
    enc = torch.randn(B, T, 192, generator=g).to(DEV)
    start = (torch.randn(B, 4, generator=g) * 10).to(DEV)
    vel = (torch.randn(B, T, 2, generator=g) * 3).to(DEV)
    with torch.no_grad():
        dpf.filtering_pos(enc, start, vel)
        res = getattr(dpf, "last_filter_result", None)
        assert res is not None, "filtering_pos went through _filtering_modules, not the engine"
        pe, glow = _pe_blob(dpf.particle_encoder), _blob(dpf.cglow_measurement)
        for s in range(T):
            xs = res.particles[:, s].contiguous()
            raw = ops.cglow_wide_measurement(pe, glow, enc[:, s].contiguous(), xs, K=1, L=1, learn_top=False,
                                             widths=widths, y_bins=bins)
            lik = raw - raw.max(dim=-1, keepdim=True)[0]
            assert torch.equal(res.lik[:, s], lik), f"slot {s}: the engine's likelihood is not the wide kernel's"
            assert torch.equal(dpf.measurement_model(enc[:, s], xs), lik), f"slot {s}: measurement_model differs"
            rt = dpf.measurement_model.torch_forward_raw(enc[:, s], xs)
            rt = rt - rt.max(dim=-1, keepdim=True)[0]
            assert_close(lik.cpu(), rt.cpu(), 1e-5, 5e-5, f"slot {s} vs the PyTorch restatement")


# ---- 7. autograd wiring ----
def test_flow_autograd(monkeypatch):
    """The forward value is the width-general kernel's, bit for bit; the backward is the recompute
    of torch_forward: none of the HIP backward kernels is called.
    Measured on an MI355X: worst max |d| / max |ref| over the tensors 7.3e-7."""
    from nfdpf import ops
    calls = []
    for name in ("cglow_wide_flow", "cglow_levels_flow", "cglow_flow") + BACKWARDS:
        _count(monkeypatch, ops, name, calls)
    fx = group(FX, "a")
    m = _fixture_model("a")
    x, y = t(fx["x"]).to(DEV).requires_grad_(True), t(fx["y"]).to(DEV).requires_grad_(True)
    z, nll = m(x, y)
    assert calls == ["cglow_wide_flow"], calls
    assert z.requires_grad and nll.requires_grad
    zk, nk = ops.cglow_wide_flow(_blob(m), x.detach(), y.detach(), K=1, L=1, widths=(16, 32, 16))
    assert torch.equal(z.detach(), zk) and torch.equal(nll.detach(), nk)
    calls.clear()
    ((z * t(fx["g_z"]).to(DEV)).sum() + (nll * t(fx["g_nll"]).to(DEV)).sum()).backward()
    assert calls == [], calls
    named = list(m.named_parameters())
    worst = max(_grad_close(x.grad, fx["dx"], fx["err_abs/dx"], "dL/dx"),
                _grad_close(y.grad, fx["dy"], fx["err_abs/dy"], "dL/dy"),
                _param_grads_close(fx, named, "a"))
    print(f"flow autograd a: worst max|d| / max|ref| over the tensors {worst:.3e}")


def test_measurement_autograd(monkeypatch):
    """Measured on an MI355X: worst max |d| / max |ref| over the tensors 1.1e-5."""
    from nfdpf import ops
    calls = []
    for name in ("cglow_wide_measurement", "cglow_levels_measurement", "cglow_measurement") + BACKWARDS:
        _count(monkeypatch, ops, name, calls)
    fx = group(FX, "meas")
    mm = _meas_dpf().measurement_model
    enc, x = t(fx["enc"]).to(DEV).requires_grad_(True), t(fx["x"]).to(DEV).requires_grad_(True)
    lik = mm(enc, x)
    _close_or_ref_err(lik.detach().cpu(), fx["lik"], 1e-5, 5e-5, fx["err_abs/lik"], "lik under autograd")
    with torch.no_grad():
        assert torch.equal(lik.detach(), mm(enc.detach(), x.detach()))
    (lik * t(fx["gl"]).to(DEV)).sum().backward()
    assert calls == ["cglow_wide_measurement"] * 2, calls
    named = list(mm.named_parameters())
    worst = max(_grad_close(enc.grad, fx["denc"], fx["err_abs/denc"], "dL/denc"),
                _grad_close(x.grad, fx["dx"], fx["err_abs/dx"], "dL/dx"),
                _param_grads_close(fx, named, "meas a"))
    print(f"measurement autograd a: worst max|d| / max|ref| over the tensors {worst:.3e}")


def test_recompute_bound_is_inherited():
    """Above 16 384 particles per call the backward refuses instead of stalling the device."""
    from nfdpf._lib import NfdpfError
    mm = _meas_dpf(num_particles=16400, batchsize=1).measurement_model
    g = torch.Generator().manual_seed(8)
    enc = torch.randn(1, 192, generator=g).to(DEV)
    x = (torch.randn(1, 16400, 2, generator=g) * 30).to(DEV).requires_grad_(True)
    lik = mm(enc, x)
    assert tuple(lik.shape) == (1, 16400) and bool(torch.isfinite(lik).all())
    with pytest.raises(NfdpfError, match="bounded to 16384"):
        lik.sum().backward()
    m = _fixture_model("a")
    xf = torch.randn(16400, 3, 8, 8, generator=g).to(DEV).requires_grad_(True)
    _, nll = m(xf, xf.detach())
    with pytest.raises(NfdpfError, match="bounded to 16384"):
        nll.sum().backward()


# ---- 8. refusals ----
def test_refusals():
    from nfdpf import _lib, ops
    from nfdpf._lib import NfdpfError, ptr
    f = dict(device=DEV, dtype=torch.float32)
    x = torch.zeros(4, 3, 8, 8, **f)
    a = torch.zeros(18300, **f)  # (16, 32, 16), K = 1, L = 1, no top
    kw = dict(K=1, L=1, widths=(16, 32, 16))
    with pytest.raises(NfdpfError, match="does not match"):  # a blob of another triple
        ops.cglow_wide_flow(torch.zeros(11548, **f), x, x, **kw)
    with pytest.raises(NfdpfError, match="does not match"):
        ops.cglow_wide_flow(a, x, x, K=1, L=1, learn_top=True, widths=(16, 32, 16))
    for widths in ((8, 24, 8), (4, 8, 4), (16, 32)):
        with pytest.raises(NfdpfError, match="x_hidden_channels"):
            ops.cglow_wide_flow(a, x, x, K=1, L=1, widths=widths)
    for K, L in ((0, 1), (5, 1), (1, 0), (1, 3)):
        with pytest.raises(NfdpfError, match=r"1\.\.4.*1\.\.2"):
            ops.cglow_wide_flow(a, x, x, K=K, L=L, widths=(16, 32, 16))
    for bins in (0, -1, float("inf"), float("nan")):
        with pytest.raises(NfdpfError, match="y_bins"):
            ops.cglow_wide_flow(a, x, x, y_bins=bins, **kw)
    with pytest.raises(NfdpfError, match="3, 8, 8"):
        ops.cglow_wide_flow(a, torch.zeros(4, 3, 4, 4, **f), torch.zeros(4, 3, 4, 4, **f), **kw)
    pe = torch.zeros(8192, **f)
    with pytest.raises(NfdpfError, match="192 wide"):
        ops.cglow_wide_measurement(pe, a, torch.zeros(2, 32, **f), torch.zeros(2, 8, 2, **f), **kw)
    with pytest.raises(NfdpfError, match="does not match"):
        ops.cglow_wide_measurement(pe, torch.zeros(7980, **f), torch.zeros(2, 192, **f), torch.zeros(2, 8, 2, **f), **kw)
    # the library's own checks: EINVAL, nothing launched, no output touched
    lib = _lib.load()
    z, nll = torch.full((4, 192), 7.0, **f), torch.full((4,), 7.0, **f)
    ld0 = -1064.6740693
    for K, L, widths in ((5, 1, (16, 32, 16)), (1, 3, (16, 32, 16)), (1, 1, (8, 24, 8))):
        rc = lib.nfdpf_cglow_wide_flow(ptr(a), K, L, None, ptr(x), ptr(x), 4, ptr(z), ptr(nll), *widths, ld0, None)
        assert rc == _lib.NFDPF_EINVAL, (K, L, widths)
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()) and bool((nll == 7.0).all())
