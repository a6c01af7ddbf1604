"""The conditional-GLOW measurement and flow at depth K = 2..4 on the HIP kernels
(csrc/cglow.hip: K steps inside one launch; csrc/cglow_bwd.hip: one launch per step, last step
first), against the reference's own K = 2, 3 runs (tests/golden/cglow_depth.npz, written by
tests/golden/gen_cglow_depth.py).  GPU box only.

Forward bounds are those of the K = 1 tests, unchanged: z |d| <= 1e-5 |ref| + 2e-5 and nll
|d| <= 1e-5 |ref| + 2e-6 (test_gpu_dpf_api.test_cond_glow_model_forward_kernel), lik
assert_close(1e-5, 5e-5) after the row-max shift (test_gpu_parity.test_cglow_measurement_golden);
and our error against the fixture's float64 values is at most 4 x the reference's own recorded
float32 error for the same quantity (ulp-level libm differences between the CPU and the device).

Gradient bound, per tensor, elementwise: the larger of
  * the K = 1 reference-pinned bar (test_gpu_grad_golden._close): 1e-3 |ref| + 2e-4 max|ref|,
  * 4 x the reference's recorded float32-vs-float64 max error of that tensor.
The first is the larger one for every tensor of the fixture (the reference's float32 error is
at most ~1e-6 of a tensor's scale).  Measured on an MI355X (worst over the tensors of max |d| /
max|ref|; each test prints its own figures):
  flow form K = 2: 1.3e-6, K = 3: 1.7e-5; measurement form K = 2: 1.5e-5."""
import numpy as np
import pytest
import torch

from _util import assert_close, group, load, t, weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FX = {}


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from nfdpf import _lib
    _lib.load()
    assert torch.cuda.is_available()
    FX.update(load("cglow_depth.npz"))


def _args(K, **kw):
    from arguments import parse_args
    a = parse_args([])
    a.flow_depth = K
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _flow_model(K):
    """This package's CondGlowModel holding the reference's K-step weights."""
    from nf.cglow.CGlowModel import CondGlowModel
    m = CondGlowModel(_args(K))
    m.load_state_dict(weights(group(FX, f"k{K}")))
    return m.to(DEV)


def _random_model(K, seed):
    """Seeded init, every parameter replaced by N(0, 0.1^2) draws (as the fixture generator)."""
    from nf.cglow.CGlowModel import CondGlowModel
    torch.manual_seed(seed)
    m = CondGlowModel(_args(K))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        m.new_mean.zero_()
        m.new_logs.zero_()
    return m.to(DEV)


def _blob(m):
    from nfdpf.pack import cglow_tensors
    return torch.cat([a.detach().reshape(-1) for a in cglow_tensors(m)]).contiguous()


def _vs_f64(ours, ref64, ref_err, what):
    e = float(np.abs(np.asarray(ours, np.float64) - ref64).max())
    print(f"{what}: max |ours - f64| {e:.3e}; the reference's float32 {float(ref_err):.3e}")
    assert e <= 4 * float(ref_err), f"{what}: |ours - f64| {e:.3e} above 4 x the reference's {float(ref_err):.3e}"


def _grad_close(ours, ref, ref_err, what):
    """|d| <= max(1e-3 |ref| + 2e-4 max|ref|, 4 x the reference's float32 error); returns the
    worst |d| relative to the tensor's scale."""
    o = ours.detach().double().cpu().numpy()
    r = np.asarray(ref, np.float64)
    assert o.shape == r.shape, (what, o.shape, r.shape)
    assert np.isfinite(o).all(), f"{what}: non-finite"
    scale = float(np.abs(r).max())
    d = np.abs(o - r)
    bound = np.maximum(1e-3 * np.abs(r) + 2e-4 * scale, 4 * float(ref_err))
    assert bool((d <= bound).all()), \
        f"{what}: max |d| {float(d.max()):.3e} (scale {scale:.3e}, reference f32 error {float(ref_err):.3e})"
    return float(d.max()) / max(scale, 1e-30)


def _param_grads_close(fx, named, what):
    names = [str(n) for n in fx["g_names"]]
    ref, off, worst = {}, 0, 0.0
    shapes = {n: p.shape for n, p in named}
    for i, n in enumerate(names):
        k = int(np.prod(shapes[n]))
        ref[n] = (fx["g_flat"][off:off + k].reshape(tuple(shapes[n])), fx["g_err_abs"][i])
        off += k
    assert off == fx["g_flat"].size
    for n, p in named:
        if n not in ref:
            assert p.grad is None, (what, n)
            continue
        assert p.grad is not None, (what, n)
        worst = max(worst, _grad_close(p.grad, ref[n][0], ref[n][1], f"{what} d/d{n}"))
    return worst


# ---- 1. flow forward vs the reference ----
@pytest.mark.parametrize("K", [2, 3])
def test_flow_forward_vs_reference(K):
    fx = group(FX, f"k{K}")
    m = _flow_model(K)
    with torch.no_grad():
        z, nll = m(t(fx["x"]).to(DEV), t(fx["y"]).to(DEV))
    z, nll = z.cpu().numpy(), nll.cpu().numpy()
    assert z.shape == fx["z"].shape
    z64 = fx["z"].astype(np.float64) + fx["f64d/z"].astype(np.float64)
    print(f"K={K}: max |z - ref32| {np.abs(z - fx['z']).max():.3e}, max |nll - ref32| {np.abs(nll - fx['nll']).max():.3e}")
    assert_close(z, fx["z"], 1e-5, 2e-5, "z")
    assert_close(nll, fx["nll"], 1e-5, 2e-6, "nll")
    _vs_f64(nll, fx["f64/nll"], fx["err_abs/nll"], f"K={K} nll")
    _vs_f64(z, z64, fx["err_abs/z"], f"K={K} z")


# ---- 2. measurement forward at K = 2, B = 3, N = 21 ----
def _meas_dpf():
    from DPFs import DPF
    torch.manual_seed(0)
    dpf = DPF(_args(2, measurement="CGLOW", hiddensize=192, num_particles=21, batchsize=3))
    sd = dpf.state_dict()
    w = weights(group(FX, "meas2"))
    assert set(w) <= set(sd)
    sd.update(w)
    dpf.load_state_dict(sd)
    return dpf.to(DEV)


def test_measurement_forward_k2():
    from nfdpf import ops
    from nfdpf.pack import encoder_tensors
    fx = group(FX, "meas2")
    dpf = _meas_dpf()
    pe = torch.cat([a.detach().reshape(-1) for a in encoder_tensors(dpf.particle_encoder)]).contiguous()
    raw = ops.cglow_measurement(pe, _blob(dpf.cglow_measurement), t(fx["enc"]).to(DEV), t(fx["x"]).to(DEV), K=2)
    lik = (raw - raw.max(dim=-1, keepdim=True)[0]).cpu().numpy()
    print(f"meas K=2: max |lik - ref32| {np.abs(lik - fx['lik']).max():.3e}; "
          f"max |lik - f64| {np.abs(lik - fx['f64/lik']).max():.3e}, the reference's {float(fx['err_abs/lik']):.3e}")
    assert_close(lik, fx["lik"], 1e-5, 5e-5, "CGLOW K=2 lik")
    # and through the module API
    with torch.no_grad():
        lik2 = dpf.measurement_model(t(fx["enc"]).to(DEV), t(fx["x"]).to(DEV))
    assert np.array_equal(lik2.cpu().numpy(), lik)


# ---- 3. persistent tile loop, ragged last tile, K = 4 ----
@pytest.mark.parametrize("K", [2, 4])
def test_flow_persistent_tiles_vs_restatement(K):
    """M = 3 x CUs x 16 + 21 samples: two tiles more than the resident grid of 3 workgroups per
    CU, so workgroups 0 and 1 run a second tile, and the last tile is ragged (5 of 16).

    The PyTorch restatement (CondGlowModel.torch_forward, same device; tests 1-2 pin it to the
    reference at K = 2, 3) costs seconds per thousand samples on the device (a batched 12x12
    slogdet per step), and a sample's output does not depend on the others.  So the restatement
    is evaluated on the samples of the tiles this test is about -- tiles 0-2 (the first trip of
    the workgroups that run two), one tile in the middle, and the two second-trip tiles with
    the ragged one -- and EVERY sample of the big launch must equal, bit for bit, the same
    kernel run on the batch in four pieces (other grids, other tile-to-workgroup assignments)."""
    from nfdpf import ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M = 3 * cus * 16 + 21
    m = _random_model(K, 40 + K)
    blob = _blob(m)
    g = torch.Generator().manual_seed(K)
    x, y = torch.randn(M, 3, 8, 8, generator=g).to(DEV), torch.randn(M, 3, 8, 8, generator=g).to(DEV)
    z, nll = ops.cglow_flow(blob, x, y, K=K)
    mid = 16 * (3 * cus // 2)
    sel = torch.cat([torch.arange(0, 48), torch.arange(mid, mid + 16), torch.arange(3 * cus * 16 - 16, M)]).to(DEV)
    with torch.no_grad():
        zr, nr = m.torch_forward(x[sel], y[sel])
    print(f"K={K} M={M}: max |z - torch| {float((z[sel] - zr).abs().max()):.3e}, "
          f"max |nll - torch| {float((nll[sel] - nr).abs().max()):.3e} on {sel.numel()} samples")
    assert_close(z[sel].cpu(), zr.cpu(), 1e-5, 2e-5, "z")
    assert_close(nll[sel].cpu(), nr.cpu(), 1e-5, 2e-6, "nll")
    cuts = [0, 1000, M // 2 + 3, M - 40, M]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        zp, np_ = ops.cglow_flow(blob, x[lo:hi].contiguous(), y[lo:hi].contiguous(), K=K)
        assert torch.equal(zp, z[lo:hi]) and torch.equal(np_, nll[lo:hi]), f"samples {lo}..{hi}"


# ---- 4. backward, flow form ----
@pytest.mark.parametrize("K", [2, 3])
def test_flow_backward_vs_reference(K, monkeypatch):
    from nfdpf import ops
    calls = []
    real = ops.cglow_flow_backward
    monkeypatch.setattr(ops, "cglow_flow_backward", lambda *a, **k: calls.append(k.get("K")) or real(*a, **k))
    fx = group(FX, f"k{K}")
    m = _flow_model(K)
    x, y = t(fx["x"]).to(DEV).requires_grad_(True), t(fx["y"]).to(DEV).requires_grad_(True)
    z, nll = m(x, y)
    ((z * t(fx["g_z"]).to(DEV)).sum() + (nll * t(fx["g_nll"]).to(DEV)).sum()).backward()
    assert calls == [K], "the backward did not run through nfdpf_cglow_flow_backward"
    worst = max(_grad_close(x.grad, fx["dx"], fx["err_abs/dx"], "dL/dx"),
                _grad_close(y.grad, fx["dy"], fx["err_abs/dy"], "dL/dy"),
                _param_grads_close(fx, list(m.named_parameters()), f"K={K}"))
    print(f"flow backward K={K}: worst max|d| / max|ref| over the tensors {worst:.3e}")


# ---- 5. backward, measurement form ----
def test_measurement_backward_k2_vs_reference(monkeypatch):
    from nfdpf import ops
    calls = []
    real = ops.cglow_measurement_backward
    monkeypatch.setattr(ops, "cglow_measurement_backward", lambda *a, **k: calls.append(k.get("K")) or real(*a, **k))
    fx = group(FX, "meas2")
    mm = _meas_dpf().measurement_model
    enc, x = t(fx["enc"]).to(DEV).requires_grad_(True), t(fx["x"]).to(DEV).requires_grad_(True)
    (mm(enc, x) * t(fx["gl"]).to(DEV)).sum().backward()
    assert calls == [2], "the backward did not run through nfdpf_cglow_measurement_backward"
    worst = max(_grad_close(enc.grad, fx["denc"], fx["err_abs/denc"], "dL/denc"),
                _grad_close(x.grad, fx["dx"], fx["err_abs/dx"], "dL/dx"),
                _param_grads_close(fx, list(mm.named_parameters()), "meas K=2"))
    print(f"measurement backward K=2: worst max|d| / max|ref| over the tensors {worst:.3e}")


# ---- 6. determinism ----
def test_backward_deterministic_k3():
    from nfdpf import ops
    m = _random_model(3, 77)
    blob = _blob(m)
    M = 1000
    g = torch.Generator().manual_seed(9)
    x, y = torch.randn(M, 3, 8, 8, generator=g).to(DEV), torch.randn(M, 3, 8, 8, generator=g).to(DEV)
    gz, gn = torch.randn(M, 12, 4, 4, generator=g).to(DEV), torch.randn(M, generator=g).to(DEV)
    a = ops.cglow_flow_backward(blob, x, y, gz, gn, K=3)
    b = ops.cglow_flow_backward(blob, x, y, gz, gn, K=3)
    for u, v, what in zip(a, b, ("g_x", "g_y", "g_glow")):
        assert torch.isfinite(u).all(), what
        assert torch.equal(u, v), what


# ---- 7. the inference filter stays one engine call ----
def test_engine_path_k2():
    from DPFs import DPF
    from nfdpf import ops
    from nfdpf.pack import encoder_tensors
    B, N, T = 2, 40, 3
    torch.manual_seed(5)
    dpf = DPF(_args(2, measurement="CGLOW", hiddensize=192, num_particles=N, batchsize=B, sequence_length=T))
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for p in dpf.cglow_measurement.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        dpf.cglow_measurement.new_mean.zero_()
        dpf.cglow_measurement.new_logs.zero_()
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
        pe = torch.cat([a.detach().reshape(-1) for a in encoder_tensors(dpf.particle_encoder)]).contiguous()
        glow = _blob(dpf.cglow_measurement)
        for s in range(T):
            xs = res.particles[:, s].contiguous()
            raw = ops.cglow_measurement(pe, glow, enc[:, s].contiguous(), xs, K=2)
            lik = raw - raw.max(dim=-1, keepdim=True)[0]
            assert torch.equal(res.lik[:, s], lik), f"slot {s}: the engine's likelihood is not the K = 2 kernel's"
            rt = dpf.measurement_model.torch_forward_raw(enc[:, s], xs)
            rt = rt - rt.max(dim=-1, keepdim=True)[0]
            assert_close(lik.cpu(), rt.cpu(), 1e-5, 5e-5, f"slot {s} vs the PyTorch restatement")


# ---- 8. argument checks ----
@pytest.mark.parametrize("K", [0, 5])
def test_bad_depth_is_einval(K):
    from nfdpf import _lib
    from nfdpf._lib import ptr
    lib = _lib.load()
    M = 16
    f = dict(device=DEV, dtype=torch.float32)
    glow, pe = torch.zeros(4 * 7980, **f), torch.zeros(8192, **f)
    x8, y8 = torch.zeros(M, 192, **f), torch.zeros(M, 192, **f)
    enc, xp = torch.zeros(1, 192, **f), torch.zeros(1, M, 2, **f)
    ws = torch.zeros(1 << 20, **f)
    outs = [torch.full((M, 192), 7.0, **f) for _ in range(4)] + [torch.full((4 * 7980,), 7.0, **f),
                                                                 torch.full((8192,), 7.0, **f),
                                                                 torch.full((M,), 7.0, **f), torch.full((M, 2), 7.0, **f)]
    z, gx, gy, gy2, gg, gpe, nll, gxp = outs
    g1 = torch.ones(M, **f)
    rcs = [
        lib.nfdpf_cglow_measurement(ptr(pe), ptr(glow), K, ptr(enc), 192, ptr(xp), 2 * M, 1, M, ptr(nll), M, None),
        lib.nfdpf_cglow_flow(ptr(glow), K, ptr(x8), ptr(y8), M, ptr(z), ptr(nll), None),
        lib.nfdpf_cglow_measurement_backward(ptr(pe), ptr(glow), K, ptr(enc), 192, ptr(xp), 2 * M, 1, M, ptr(g1), M,
                                             ptr(gxp), ptr(gy2), ptr(gg), ptr(gpe), ptr(ws), None),
        lib.nfdpf_cglow_flow_backward(ptr(glow), K, ptr(x8), ptr(y8), M, None, ptr(g1), ptr(gx), ptr(gy), ptr(gg),
                                      ptr(ws), None),
    ]
    assert rcs == [_lib.NFDPF_EINVAL] * 4, rcs
    assert b"1..4" in lib.nfdpf_last_error()
    torch.cuda.synchronize()
    for o in outs:  # nothing launched: no output touched
        assert bool((o == 7.0).all())
