"""The conditional-GLOW measurement and flow with two levels (-L 2) and / or a learnt top prior
(--learn_top True) on the HIP levels kernel (csrc/cglow_levels.hip), against the reference's own
runs (tests/golden/cglow_levels.npz, cglow_levels_top.npz; tests/golden/gen_cglow_levels.py).
GPU box only.

Forward bounds, elementwise: z |d| <= max(1e-5 |ref| + 2e-5, 4 x the fixture's err_abs/z), nll
|d| <= max(1e-5 |ref| + 2e-6, 4 x err_abs/nll) -- the depth tests' bars, widened only by 4 x the
reference's own recorded float32-vs-float64 error (at depth that error passes the fixed 2e-6:
the reference itself is 2e-6 .. 4e-6 from float64 on nll at L = 2) -- and against the fixture's
float64 values at most 4 x the reference's own float32 error (the _vs_f64 yardstick of
test_gpu_cglow_depth: ulp-level libm differences between the CPU and the device).  lik:
assert_close(1e-5, 5e-5) after the row-max shift, widened by the same 4 x term.  Gradients:
test_gpu_cglow_depth._grad_close.

The figures measured on an MI355X are in the tests' docstrings (each test prints its own)."""
import numpy as np
import pytest
import torch

from _util import assert_close, group, load, t, weights
from test_gpu_cglow_depth import _grad_close, _param_grads_close, _vs_f64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FX = {}


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from nfdpf import _lib
    _lib.load()
    assert torch.cuda.is_available()
    FX.update(load("cglow_levels.npz"))
    FX.update(load("cglow_levels_top.npz"))


def _args(K, L, top, **kw):
    from arguments import parse_args
    a = parse_args([])
    a.flow_depth, a.num_levels, a.learn_top = K, L, top
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _pre(K, L, top):
    return f"k{K}l{L}t{int(top)}"


def _flow_model(K, L, top):
    """This package's CondGlowModel holding the reference's weights."""
    from nf.cglow.CGlowModel import CondGlowModel
    m = CondGlowModel(_args(K, L, top))
    m.load_state_dict(weights(group(FX, _pre(K, L, top))))
    return m.to(DEV)


def _random_model(K, L, top, seed):
    """Seeded init, every parameter replaced by N(0, 0.1^2) draws (as the fixture generator)."""
    from nf.cglow.CGlowModel import CondGlowModel
    torch.manual_seed(seed)
    m = CondGlowModel(_args(K, L, top))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        if not top:
            m.new_mean.zero_()
            m.new_logs.zero_()
    return m.to(DEV)


def _blob(m):
    from nfdpf.pack import cglow_levels_tensors
    return torch.cat([a.detach().reshape(-1) for a in cglow_levels_tensors(m)]).contiguous()


def _pe_blob(enc):
    from nfdpf.pack import encoder_tensors
    return torch.cat([a.detach().reshape(-1) for a in encoder_tensors(enc)]).contiguous()


def _close_or_ref_err(ours, ref, rtol, atol, ref_err, what):
    """|d| <= max(rtol |ref| + atol, 4 x the reference's own float32 error), elementwise."""
    o, r = np.asarray(ours, np.float64), np.asarray(ref, np.float64)
    assert o.shape == r.shape, (what, o.shape, r.shape)
    assert np.isfinite(o).all(), f"{what}: non-finite"
    d = np.abs(o - r)
    bound = np.maximum(rtol * np.abs(r) + atol, 4 * float(ref_err))
    assert bool((d <= bound).all()), f"{what}: max |d| {float(d.max()):.3e}, worst excess {float((d - bound).max()):.3e}"


def _forward_bounds(z, nll, zr, nr, err_z, err_nll, what):
    print(f"{what}: max |z - ref| {np.abs(np.asarray(z) - np.asarray(zr)).max():.3e}, "
          f"max |nll - ref| {np.abs(np.asarray(nll) - np.asarray(nr)).max():.3e}")
    _close_or_ref_err(z, zr, 1e-5, 2e-5, err_z, f"{what} z")
    _close_or_ref_err(nll, nr, 1e-5, 2e-6, err_nll, f"{what} nll")


# ---- 1. flow forward vs the reference ----
@pytest.mark.parametrize("K,L,top", [(1, 2, False), (2, 2, True), (1, 1, True)])
def test_flow_forward_vs_reference(K, L, top):
    """Measured on an MI355X, max |ours - ref32| (z, nll) and max |ours - f64| (nll, z) against
    the reference's own float32 error:
      (1, 2, off): z 1.2e-7, nll 1.9e-6; f64: nll 1.3e-6 (reference 1.6e-6), z 1.8e-7 (1.4e-7)
      (2, 2, on):  z 6.0e-8, nll 3.8e-6; f64: nll 2.4e-6 (reference 4.1e-6), z 5.9e-8 (5.2e-8)
      (1, 1, on):  z 2.4e-7, nll 1.9e-6; f64: nll 1.2e-6 (reference 1.4e-6), z 2.6e-7 (2.1e-7)"""
    fx = group(FX, _pre(K, L, top))
    m = _flow_model(K, L, top)
    with torch.no_grad():
        z, nll = m(t(fx["x"]).to(DEV), t(fx["y"]).to(DEV))
    z, nll = z.cpu().numpy(), nll.cpu().numpy()
    assert z.shape == fx["z"].shape
    z64 = fx["z"].astype(np.float64) + fx["f64d/z"].astype(np.float64)
    _forward_bounds(z, nll, fx["z"], fx["nll"], fx["err_abs/z"], fx["err_abs/nll"], f"(K, L, top) = ({K}, {L}, {top})")
    _vs_f64(nll, fx["f64/nll"], fx["err_abs/nll"], f"({K}, {L}, {top}) nll")
    _vs_f64(z, z64, fx["err_abs/z"], f"({K}, {L}, {top}) z")


# ---- 2. measurement forward at K = 1, L = 2, top on, B = 3, N = 21 ----
def _meas_dpf():
    from DPFs import DPF
    torch.manual_seed(0)
    dpf = DPF(_args(1, 2, True, measurement="CGLOW", hiddensize=192, num_particles=21, batchsize=3))
    sd = dpf.state_dict()
    w = weights(group(FX, "meas"))
    assert set(w) <= set(sd)
    sd.update(w)
    dpf.load_state_dict(sd)
    return dpf.to(DEV)


def test_measurement_forward_l2_top():
    """Measured on an MI355X: max |lik - ref32| 2.9e-6; max |lik - f64| 1.4e-6, the reference's 2.5e-6."""
    from nfdpf import ops
    fx = group(FX, "meas")
    dpf = _meas_dpf()
    raw = ops.cglow_levels_measurement(_pe_blob(dpf.particle_encoder), _blob(dpf.cglow_measurement),
                                       t(fx["enc"]).to(DEV), t(fx["x"]).to(DEV), K=1, L=2, learn_top=True)
    lik = (raw - raw.max(dim=-1, keepdim=True)[0]).cpu().numpy()
    print(f"meas (1, 2, on): max |lik - ref32| {np.abs(lik - fx['lik']).max():.3e}; "
          f"max |lik - f64| {np.abs(lik - fx['f64/lik']).max():.3e}, the reference's {float(fx['err_abs/lik']):.3e}")
    _close_or_ref_err(lik, fx["lik"], 1e-5, 5e-5, fx["err_abs/lik"], "CGLOW (1, 2, on) lik")
    # and through the module API: the same bits
    with torch.no_grad():
        lik2 = dpf.measurement_model(t(fx["enc"]).to(DEV), t(fx["x"]).to(DEV))
    assert np.array_equal(lik2.cpu().numpy(), lik)


# ---- 3. persistent tile loop, ragged last tile ----
def test_flow_persistent_tiles_vs_restatement():
    """(K, L, top) = (2, 2, on), M = 4 x CUs x 16 + 21 samples: every workgroup runs more than one
    tile at any residency <= 3 per CU, and the last tile is ragged (5 of 16).  The PyTorch
    restatement (CondGlowModel.torch_forward, same device; test_cglow_levels_pack pins it to the
    reference) is evaluated on tiles 0-2, one tile in the middle and the last two tiles, within
    the bounds of test 1 with the reference's float32 error of the (2, 2, on) fixture; and EVERY
    sample must equal, bit for bit, the same kernel run on the batch in four pieces (other grids,
    other tile-to-workgroup assignments).
    Measured on an MI355X: M = 16 405; max |z - torch| 6.0e-8, max |nll - torch| 3.8e-6 on the 101 samples."""
    from nfdpf import ops
    K, L, top = 2, 2, True
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M = 4 * cus * 16 + 21
    m = _random_model(K, L, top, 52)
    blob = _blob(m)
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(M, 3, 8, 8, generator=g).to(DEV), torch.randn(M, 3, 8, 8, generator=g).to(DEV)
    z, nll = ops.cglow_levels_flow(blob, x, y, K=K, L=L, learn_top=top)
    assert tuple(z.shape) == (M, 24, 2, 2)
    mid = 16 * (2 * cus)
    sel = torch.cat([torch.arange(0, 48), torch.arange(mid, mid + 16), torch.arange(4 * cus * 16 - 16, M)]).to(DEV)
    with torch.no_grad():
        zr, nr = m.torch_forward(x[sel], y[sel])
    fx = group(FX, _pre(K, L, top))
    _forward_bounds(z[sel].cpu(), nll[sel].cpu(), zr.cpu(), nr.cpu(), fx["err_abs/z"], fx["err_abs/nll"],
                    f"M={M}, {sel.numel()} samples vs torch")
    cuts = [0, 1000, M // 2 + 3, M - 40, M]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        zp, np_ = ops.cglow_levels_flow(blob, x[lo:hi].contiguous(), y[lo:hi].contiguous(), K=K, L=L, learn_top=top)
        assert torch.equal(zp, z[lo:hi]) and torch.equal(np_, nll[lo:hi]), f"samples {lo}..{hi}"


# ---- 4. L = 1 without learn_top is untouched ----
def test_single_level_routing_untouched():
    """A K = 2, L = 1, learn_top-off model still runs csrc/cglow.hip (bits of ops.cglow_flow), and the
    levels kernel at (K, 1, no top) agrees with it within the bounds of test 1 (the reference's
    float32 error taken from the (1, 1, on) fixture, the single-level one).
    Measured on an MI355X: max |z - cglow_flow| 8.9e-8, max |nll - cglow_flow| 1.9e-6."""
    from nfdpf import ops
    from nfdpf.pack import cglow_tensors
    m = _random_model(2, 1, False, 61)
    assert m.kernel_supported()
    g = torch.Generator().manual_seed(4)
    M = 53
    x, y = torch.randn(M, 3, 8, 8, generator=g).to(DEV), torch.randn(M, 3, 8, 8, generator=g).to(DEV)
    old = torch.cat([a.detach().reshape(-1) for a in cglow_tensors(m)]).contiguous()
    z0, n0 = ops.cglow_flow(old, x, y, K=2)
    with torch.no_grad():
        z1, n1 = m(x, y)
    assert torch.equal(z0, z1) and torch.equal(n0, n1), "CondGlowModel.forward left the single-level kernel"
    assert torch.equal(_blob(m), old)
    z2, n2 = ops.cglow_levels_flow(old, x, y, K=2, L=1, learn_top=False)
    fx = group(FX, _pre(1, 1, True))
    _forward_bounds(z2.cpu(), n2.cpu(), z0.cpu(), n0.cpu(), fx["err_abs/z"], fx["err_abs/nll"], "levels (2, 1, off) vs cglow_flow")


# ---- 5. the inference filter stays one engine call ----
def test_engine_path_l2_top():
    from DPFs import DPF
    from nfdpf import ops
    B, N, T = 2, 40, 3
    torch.manual_seed(5)
    dpf = DPF(_args(1, 2, True, measurement="CGLOW", hiddensize=192, num_particles=N, batchsize=B, sequence_length=T))
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
            raw = ops.cglow_levels_measurement(pe, glow, enc[:, s].contiguous(), xs, K=1, L=2, learn_top=True)
            lik = raw - raw.max(dim=-1, keepdim=True)[0]
            assert torch.equal(res.lik[:, s], lik), f"slot {s}: the engine's likelihood is not the levels kernel's"
            rt = dpf.measurement_model.torch_forward_raw(enc[:, s], xs)
            rt = rt - rt.max(dim=-1, keepdim=True)[0]
            assert_close(lik.cpu(), rt.cpu(), 1e-5, 5e-5, f"slot {s} vs the PyTorch restatement")


# ---- 6. autograd wiring ----
def _count(monkeypatch, ops, name, calls):
    real = getattr(ops, name)
    monkeypatch.setattr(ops, name, lambda *a, **k: calls.append(name) or real(*a, **k))


def test_flow_autograd_l2_top(monkeypatch):
    """The forward value is the levels kernel's; the backward is the recompute of torch_forward
    (no HIP backward at L = 2 / learn_top), never the single-level backward kernels.
    Measured on an MI355X: worst max |d| / max |ref| over the tensors 2.2e-6."""
    from nfdpf import ops
    calls = []
    for name in ("cglow_levels_flow", "cglow_flow", "cglow_flow_backward", "cglow_measurement_backward"):
        _count(monkeypatch, ops, name, calls)
    fx = group(FX, _pre(1, 2, True))
    m = _flow_model(1, 2, True)
    x, y = t(fx["x"]).to(DEV).requires_grad_(True), t(fx["y"]).to(DEV).requires_grad_(True)
    z, nll = m(x, y)
    assert calls == ["cglow_levels_flow"], calls
    _forward_bounds(z.detach().cpu(), nll.detach().cpu(), fx["z"], fx["nll"], fx["err_abs/z"], fx["err_abs/nll"],
                    "(1, 2, on) under autograd")
    ((z * t(fx["g_z"]).to(DEV)).sum() + (nll * t(fx["g_nll"]).to(DEV)).sum()).backward()
    assert calls == ["cglow_levels_flow"], calls
    named = list(m.named_parameters())
    got = {n for n, p in named if p.grad is not None}
    assert {"new_mean", "new_logs", "flow.layers.2.conv.0.weight", "flow.layers.2.conv.0.bias"} <= got
    worst = max(_grad_close(x.grad, fx["dx"], fx["err_abs/dx"], "dL/dx"),
                _grad_close(y.grad, fx["dy"], fx["err_abs/dy"], "dL/dy"),
                _param_grads_close(fx, named, "(1, 2, on)"))
    print(f"flow autograd (1, 2, on): worst max|d| / max|ref| over the tensors {worst:.3e}")


def test_flow_forward_value_under_autograd_is_the_kernels():
    from nfdpf import ops
    fx = group(FX, _pre(1, 2, True))
    m = _flow_model(1, 2, True)
    x, y = t(fx["x"]).to(DEV), t(fx["y"]).to(DEV)
    zk, nk = ops.cglow_levels_flow(_blob(m), x, y, K=1, L=2, learn_top=True)
    z, nll = m(x.clone().requires_grad_(True), y)
    assert z.requires_grad and nll.requires_grad
    assert torch.equal(z.detach(), zk) and torch.equal(nll.detach(), nk)


def test_measurement_autograd_l2_top(monkeypatch):
    """Measured on an MI355X: worst max |d| / max |ref| over the tensors 2.6e-5."""
    from nfdpf import ops
    calls = []
    for name in ("cglow_levels_measurement", "cglow_measurement", "cglow_flow_backward", "cglow_measurement_backward"):
        _count(monkeypatch, ops, name, calls)
    fx = group(FX, "meas")
    mm = _meas_dpf().measurement_model
    enc, x = t(fx["enc"]).to(DEV).requires_grad_(True), t(fx["x"]).to(DEV).requires_grad_(True)
    lik = mm(enc, x)
    _close_or_ref_err(lik.detach().cpu(), fx["lik"], 1e-5, 5e-5, fx["err_abs/lik"], "lik under autograd")
    (lik * t(fx["gl"]).to(DEV)).sum().backward()
    assert calls == ["cglow_levels_measurement"], calls
    named = list(mm.named_parameters())
    got = {n for n, p in named if p.grad is not None}
    assert {"CGLOW.new_mean", "CGLOW.new_logs", "CGLOW.flow.layers.2.conv.0.weight"} <= got
    worst = max(_grad_close(enc.grad, fx["denc"], fx["err_abs/denc"], "dL/denc"),
                _grad_close(x.grad, fx["dx"], fx["err_abs/dx"], "dL/dx"),
                _param_grads_close(fx, named, "meas (1, 2, on)"))
    print(f"measurement autograd (1, 2, on): worst max|d| / max|ref| over the tensors {worst:.3e}")


# ---- 7. argument checks ----
@pytest.mark.parametrize("K,L", [(0, 1), (5, 2), (1, 0), (2, 3)])
def test_bad_depth_or_levels_is_einval(K, L):
    from nfdpf import _lib
    from nfdpf._lib import ptr
    lib = _lib.load()
    M = 16
    f = dict(device=DEV, dtype=torch.float32)
    glow, pe = torch.zeros(4 * (7980 + 21168) + 660 + 384, **f), torch.zeros(8192, **f)
    x8, y8 = torch.zeros(M, 192, **f), torch.zeros(M, 192, **f)
    enc, xp = torch.zeros(1, 192, **f), torch.zeros(1, M, 2, **f)
    z, nll, lik = torch.full((M, 192), 7.0, **f), torch.full((M,), 7.0, **f), torch.full((M,), 7.0, **f)
    rcs = [
        lib.nfdpf_cglow_levels_measurement(ptr(pe), ptr(glow), K, L, None, ptr(enc), 192, ptr(xp), 2 * M, 1, M,
                                           ptr(lik), M, None),
        lib.nfdpf_cglow_levels_flow(ptr(glow), K, L, None, ptr(x8), ptr(y8), M, ptr(z), ptr(nll), None),
    ]
    assert rcs == [_lib.NFDPF_EINVAL] * 2, rcs
    msg = lib.nfdpf_last_error()
    assert b"1..4" in msg and b"1..2" in msg, msg
    torch.cuda.synchronize()
    for o in (z, nll, lik):  # nothing launched: no output touched
        assert bool((o == 7.0).all())


def test_ops_refuse_a_blob_of_another_configuration():
    from nfdpf import ops
    from nfdpf._lib import NfdpfError
    f = dict(device=DEV, dtype=torch.float32)
    x = torch.zeros(4, 3, 8, 8, **f)
    with pytest.raises(NfdpfError, match="does not match"):
        ops.cglow_levels_flow(torch.zeros(7980 + 660 + 21168, **f), x, x, K=1, L=2, learn_top=True)
    with pytest.raises(NfdpfError, match="1..2"):
        ops.cglow_levels_flow(torch.zeros(7980, **f), x, x, K=1, L=3)
