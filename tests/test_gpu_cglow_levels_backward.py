"""HIP backward of the conditional-GLOW measurement and flow with two levels (-L 2) and / or a
learnt top prior (--learn_top True), -K 1..4: csrc/cglow_levels_bwd.hip,
nfdpf_cglow_levels_measurement_backward / nfdpf_cglow_levels_flow_backward, against PyTorch
autograd of the same math in float64, with the float32 autograd's own error sizing the bar
(the bar and the helpers of test_gpu_cglow_backward.py, copied).  GPU box only.

test_flow_autograd_l2_top and test_measurement_autograd_l2_top in test_gpu_cglow_levels.py now
run through these kernels too (against the reference's fixture gradients); their docstrings,
which say "the backward is the recompute", are stale -- that file is left as it is.

Sizes: 2 x 2 500 particles = 313 level-1 tiles of 16 and 625 level-2 tiles of 8 over at most 256
workgroups (the parameter accumulators carry across tiles, the last tiles are ragged), 79 rows
of the top prior's partials with a ragged last row; 3 x 37 has ragged rows.

Bar, per tensor: |d| <= 4 |err32| + 2e-4 max|ref| on 95 % of the elements, and a global cap
|d| <= 2e-3 |ref| + 2e-4 max|ref|.

The draw of the N(0, 0.1^2) perturbation: seed 11 at L = 1 (as test_gpu_cglow_backward.py), seed
12 at L = 2.  With seed 11 the L = 2 models' level-1 step 0 gets a 1x1-conv net whose per-sample
12 x 12 W reaches a condition number of 1.2e6 .. 2.5e7 on these inputs (float64, every other W
stays below 1e3); d log|det W| / dW = W^-T then carries cond x 2^-24 of relative error in any
float32 evaluation, and the float32 autograd reference itself breaks the global cap there
(measured: 398 elements of dL/dx at (1, 2, off), rows 572, 604, 765; the kernel 499, the same
rows).  With seed 12 every step's W has cond <= 1e3 on every input used here, which
_assert_well_conditioned checks on the float64 reference before any comparison."""
import copy
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _perturb(m, scale, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_((torch.randn(p.shape, generator=g) * scale).to(p.device))


def _check(ours, r32, r64, what):
    o, a, b = ours.detach().double().cpu(), r32.detach().double().cpu(), r64.detach().double().cpu()
    assert torch.isfinite(o).all(), f"{what}: non-finite"
    scale = float(b.abs().max())
    d = (o - b).abs()
    e32 = (a - b).abs()
    ok = d <= 4 * e32 + 2e-4 * scale
    cap = d <= 2e-3 * b.abs() + 2e-4 * scale
    assert bool(cap.all()), f"{what}: max |d| {float(d.max()):.3e} scale {scale:.3e}"
    frac = float(ok.double().mean())
    assert frac >= 0.95, f"{what}: only {frac:.4f} within 4x the fp32 autograd error (max |d| {float(d.max()):.3e})"


def _args(K, L, top, **kw):
    from arguments import parse_args
    a = parse_args([])
    a.flow_depth, a.num_levels, a.learn_top = K, L, top
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _glow(K, L, top):
    from nf.cglow.CGlowModel import CondGlowModel
    torch.manual_seed(3)
    m = CondGlowModel(_args(K, L, top))
    _perturb(m, 0.1, 11 if L == 1 else 12)  # the reference init zeroes the coupling's output convs: move off it
    return m


def _assert_well_conditioned(glow64, x64):
    """The test's own inputs: every step's per-sample W (float64) has cond < 2e4 -- the range in
    which a float32 evaluation of W^-T can meet the bar (module docstring)."""
    with torch.no_grad():
        for st in [l for l in glow64.flow.layers if hasattr(l, "affine")]:
            outs = [mm for mm in st.invconv.x_Linear.modules() if hasattr(mm, "out_features")]
            C = int(round(outs[-1].out_features ** 0.5))
            w = st.invconv.get_weight(x64, x64.new_zeros(x64.shape[0], C, 1, 1), False)[0]
            cond = float(torch.linalg.cond(w).max())
            assert cond < 2e4, f"test input: a per-sample W with cond {cond:.3g}"


def _spy(monkeypatch, ops, name):
    calls = []
    real = getattr(ops, name)
    monkeypatch.setattr(ops, name, lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


def _check_params(m, refs):
    for (name, p), g32, g64 in zip(m.named_parameters(), refs[torch.float32], refs[torch.float64]):
        if g64 is None:
            assert p.grad is None, name
            continue
        assert p.grad is not None, name
        _check(p.grad, g32, g64, f"dL/d{name}")


# ---- 1. flow form against float64 autograd ----
@pytest.mark.parametrize("K,L,top", [(1, 1, True), (3, 1, True), (1, 2, False), (1, 2, True), (2, 2, True)])
def test_levels_flow_backward_vs_autograd(K, L, top, monkeypatch):
    """CondGlowModel.forward(x, y) -> (z, nll), both outputs used; the backward runs through
    ops.cglow_levels_flow_backward exactly once."""
    from nfdpf import ops
    calls = _spy(monkeypatch, ops, "cglow_levels_flow_backward")
    m = _glow(K, L, top)
    ref = copy.deepcopy(m)
    m = m.to(DEV)
    M = 1000
    g = torch.Generator().manual_seed(7 + K + 10 * L)
    x, y = torch.randn(M, 3, 8, 8, generator=g), torch.randn(M, 3, 8, 8, generator=g)
    gz = torch.randn((M, 24, 2, 2) if L == 2 else (M, 12, 4, 4), generator=g)
    gn = torch.randn(M, generator=g)
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    z, nll = m(xd, yd)
    ((z * gz.to(DEV)).sum() + (nll * gn.to(DEV)).sum()).backward()
    assert len(calls) == 1, "the backward did not run through nfdpf_cglow_levels_flow_backward"
    refs = {}
    for dt in (torch.float32, torch.float64):
        r = copy.deepcopy(ref).to(DEV, dt)
        xr, yr = x.to(DEV, dt).requires_grad_(True), y.to(DEV, dt).requires_grad_(True)
        if dt == torch.float64:
            _assert_well_conditioned(r, xr.detach())
        zr, nr = r.torch_forward(xr, yr)
        ((zr * gz.to(DEV, dt)).sum() + (nr * gn.to(DEV, dt)).sum()).backward()
        refs[dt] = (xr.grad, yr.grad, [p.grad for p in r.parameters()])
    _check(xd.grad, refs[torch.float32][0], refs[torch.float64][0], "dL/dx")
    _check(yd.grad, refs[torch.float32][1], refs[torch.float64][1], "dL/dy")
    if top:
        assert m.new_mean.grad is not None and m.new_logs.grad is not None
    else:
        assert m.new_mean.grad is None and m.new_logs.grad is None
    _check_params(m, {dt: refs[dt][2] for dt in refs})


def test_levels_flow_backward_nll_only(monkeypatch):
    """z unused (g_z = NULL at the ABI): the gradient of nll alone."""
    from nfdpf import ops
    calls = _spy(monkeypatch, ops, "cglow_levels_flow_backward")
    m = _glow(2, 2, True)
    ref = copy.deepcopy(m)
    m = m.to(DEV)
    M = 53
    g = torch.Generator().manual_seed(9)
    x, y = torch.randn(M, 3, 8, 8, generator=g), torch.randn(M, 3, 8, 8, generator=g)
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    m(xd, yd)[1].sum().backward()
    assert len(calls) == 1
    refs = {}
    for dt in (torch.float32, torch.float64):
        r = copy.deepcopy(ref).to(DEV, dt)
        xr, yr = x.to(DEV, dt).requires_grad_(True), y.to(DEV, dt).requires_grad_(True)
        r.torch_forward(xr, yr)[1].sum().backward()
        refs[dt] = (xr.grad, yr.grad, [p.grad for p in r.parameters()])
    _check(xd.grad, refs[torch.float32][0], refs[torch.float64][0], "dL/dx")
    _check(yd.grad, refs[torch.float32][1], refs[torch.float64][1], "dL/dy")
    _check_params(m, {dt: refs[dt][2] for dt in refs})


# ---- 2. measurement form against float64 autograd ----
@pytest.mark.parametrize("K,L,top,B,N", [(1, 2, True, 2, 2500), (1, 2, True, 3, 37), (2, 2, False, 3, 37),
                                         (1, 1, True, 2, 2500), (2, 1, True, 3, 37)])
def test_levels_measurement_backward_vs_autograd(K, L, top, B, N, monkeypatch):
    from model.models import build_particle_encoder_cglow, measurement_model_cglow
    from nfdpf import ops
    calls = _spy(monkeypatch, ops, "cglow_levels_measurement_backward")
    glow = _glow(K, L, top)
    torch.manual_seed(5)
    pe = build_particle_encoder_cglow(192, 2)
    ref = measurement_model_cglow(copy.deepcopy(pe), copy.deepcopy(glow))
    m = measurement_model_cglow(pe, glow).to(DEV)
    g = torch.Generator().manual_seed(B * 1000 + N)
    enc = torch.randn(B, 192, generator=g)
    x = torch.randn(B, N, 2, generator=g) * 20
    gl = torch.randn(B, N, generator=g)
    encd, xd = enc.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    lik = m(encd, xd)
    (lik * gl.to(DEV)).sum().backward()
    assert len(calls) == 1, "the backward did not run through nfdpf_cglow_levels_measurement_backward"
    am = (lik.detach() == 0).float().argmax(-1).cpu()
    refs = {}
    # the references run on the CPU: on the GPU, autograd of the L = 2 model at 5 000 samples spends
    # about 70 s in the convolution library's first-use search (1.5 s + 0.8 s here)
    for dt in (torch.float32, torch.float64):
        r = copy.deepcopy(ref).to(dt)
        er, xr = enc.clone().to(dt).requires_grad_(True), x.clone().to(dt).requires_grad_(True)
        es = r.particle_encoder(xr.reshape(-1, 2)).reshape(B * N, 3, 8, 8)
        eo = er[:, None, :].repeat(1, N, 1).reshape(B * N, 3, 8, 8)
        if dt == torch.float64:
            _assert_well_conditioned(r.CGLOW, es.detach())
        u = -r.CGLOW.torch_forward(es, eo)[1].reshape(B, N)
        lr = u - u.gather(1, am[:, None])  # the row max at OUR argmax (ties at the init)
        (lr * gl.to(dt)).sum().backward()
        refs[dt] = (xr.grad, er.grad, [p.grad for p in r.parameters()])
    _check(xd.grad, refs[torch.float32][0], refs[torch.float64][0], "dL/dx")
    _check(encd.grad, refs[torch.float32][1], refs[torch.float64][1], "dL/denc")
    _check_params(m, {dt: refs[dt][2] for dt in refs})


def _blobs(K, L, top):
    from model.models import build_particle_encoder_cglow
    from nfdpf.pack import cglow_levels_tensors, encoder_tensors
    glow = _glow(K, L, top).to(DEV)
    torch.manual_seed(1)
    pe = build_particle_encoder_cglow(192, 2).to(DEV)
    peb = torch.cat([t.detach().reshape(-1) for t in encoder_tensors(pe)]).contiguous()
    glb = torch.cat([t.detach().reshape(-1) for t in cglow_levels_tensors(glow)]).contiguous()
    return peb, glb


# ---- 3. determinism ----
def test_levels_backward_deterministic():
    """Two runs give bit-identical gradients (fixed-order partials, no atomics)."""
    from nfdpf import ops
    peb, glb = _blobs(2, 2, True)
    g = torch.Generator().manual_seed(2)
    enc = torch.randn(4, 192, generator=g).to(DEV)
    x = (torch.randn(4, 3001, 2, generator=g) * 20).to(DEV)
    gl = torch.randn(4, 3001, generator=g).to(DEV)
    a = ops.cglow_levels_measurement_backward(peb, glb, enc, x, gl, K=2, L=2, learn_top=True)
    b = ops.cglow_levels_measurement_backward(peb, glb, enc, x, gl, K=2, L=2, learn_top=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert bool((a[2][-192:] != 0).any()), "the top prior's gradient was not written"


# ---- 4. the recompute's bound is lifted ----
def test_levels_backward_above_the_recompute_bound(monkeypatch):
    """18 000 particles > the recompute's 16 384: refused with the HIP backward off, taken with
    it on (on the parent the second half raised too)."""
    from model.models import build_particle_encoder_cglow, measurement_model_cglow
    from nfdpf import autograd
    from nfdpf._lib import NfdpfError
    m = measurement_model_cglow(build_particle_encoder_cglow(192, 2), _glow(1, 2, True)).to(DEV)
    B, N = 2, 9000
    enc = torch.randn(B, 192, device=DEV)
    x = (torch.randn(B, N, 2, device=DEV) * 20).requires_grad_(True)
    monkeypatch.setattr(autograd, "HIP_BACKWARD", False)
    with pytest.raises(NfdpfError, match="recompute"):
        m(enc, x).sum().backward()
    monkeypatch.setattr(autograd, "HIP_BACKWARD", True)
    x.grad = None
    m(enc, x).sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and bool((x.grad != 0).any())


# ---- 5. argument checks ----
@pytest.mark.parametrize("K,L", [(5, 1), (5, 2), (1, 3), (1, 0), (0, 2)])
def test_levels_backward_bad_depth_or_levels_is_einval(K, L):
    """K outside 1..4 or L outside 1..2: EINVAL with a message, nothing launched."""
    from nfdpf import _lib
    from nfdpf._lib import ptr
    lib = _lib.load()
    M = 16
    f = dict(device=DEV, dtype=torch.float32)
    glow, pe = torch.zeros(4 * (7980 + 21168) + 660 + 384, **f), torch.zeros(8192, **f)
    x8, y8 = torch.zeros(M, 192, **f), torch.zeros(M, 192, **f)
    enc, xp, gl = torch.zeros(1, 192, **f), torch.zeros(1, M, 2, **f), torch.zeros(1, M, **f)
    ws = torch.zeros(1 << 22, **f)
    outs = [torch.full(s, 7.0, **f) for s in ((M, 2), (M, 192), (glow.numel(),), (8192,), (M, 192), (M, 192))]
    gxp, gy, gg, gpe, gx8, gy8 = outs
    assert lib.nfdpf_cglow_levels_backward_workspace(M, K, L) == -1
    rcs = [
        lib.nfdpf_cglow_levels_measurement_backward(ptr(pe), ptr(glow), K, L, None, ptr(enc), 192, ptr(xp), 2 * M, 1, M,
                                                    ptr(gl), M, ptr(gxp), ptr(gy), ptr(gg), ptr(gpe), ptr(ws), None),
        lib.nfdpf_cglow_levels_flow_backward(ptr(glow), K, L, None, ptr(x8), ptr(y8), M, None, ptr(gl), ptr(gx8),
                                             ptr(gy8), ptr(gg), ptr(ws), None),
    ]
    assert rcs == [_lib.NFDPF_EINVAL] * 2, rcs
    msg = lib.nfdpf_last_error()
    assert b"1..4" in msg and b"1..2" in msg, msg
    torch.cuda.synchronize()
    for o in outs:  # nothing launched: no output touched
        assert bool((o == 7.0).all())


def test_levels_backward_ops_refuse_bad_arguments():
    from nfdpf import ops
    from nfdpf._lib import NfdpfError
    f = dict(device=DEV, dtype=torch.float32)
    x = torch.zeros(4, 3, 8, 8, **f)
    enc, xp, gl, pe = torch.zeros(1, 192, **f), torch.zeros(1, 4, 2, **f), torch.zeros(1, 4, **f), torch.zeros(8192, **f)
    with pytest.raises(NfdpfError, match="does not match"):  # the (1, 1, off) blob
        ops.cglow_levels_flow_backward(torch.zeros(7980, **f), x, x, None, None, K=1, L=1, learn_top=True)
    with pytest.raises(NfdpfError, match="does not match"):  # the (1, 2, on) blob
        ops.cglow_levels_measurement_backward(pe, torch.zeros(30000, **f), enc, xp, gl, K=1, L=1, learn_top=True)
    for K, L in ((5, 1), (1, 3), (1, 0)):
        with pytest.raises(NfdpfError, match="1..2"):
            ops.cglow_levels_flow_backward(torch.zeros(7980 + 384, **f), x, x, None, None, K=K, L=L, learn_top=True)
        with pytest.raises(NfdpfError, match="1..2"):
            ops.cglow_levels_measurement_backward(pe, torch.zeros(7980 + 384, **f), enc, xp, gl, K=K, L=L,
                                                  learn_top=True)
    with pytest.raises(NfdpfError, match="does not match"):  # the (1, 2, off) blob at (1, 2, on)
        ops.cglow_levels_flow_backward(torch.zeros(30000 - 192, **f), x, x, None, None, K=1, L=2, learn_top=True)
    with pytest.raises(NfdpfError, match="g_z"):
        ops.cglow_levels_flow_backward(torch.zeros(30000, **f), x, x, torch.zeros(4, 12, 4, 4, **f), None, K=1, L=2,
                                       learn_top=True)
    with pytest.raises(NfdpfError, match="g_z"):
        ops.cglow_levels_flow_backward(torch.zeros(7980 + 384, **f), x, x, torch.zeros(4, 24, 2, 2, **f), None, K=1,
                                       L=1, learn_top=True)


def test_levels_backward_zero_rows():
    """B = 0 and M = 0: the parameter gradients come back zeroed."""
    from nfdpf import ops
    peb, glb = _blobs(1, 2, True)
    f = dict(device=DEV, dtype=torch.float32)
    g_enc, gx, g_glow, g_pe = ops.cglow_levels_measurement_backward(
        peb, glb, torch.zeros(0, 192, **f), torch.zeros(0, 5, 2, **f), torch.zeros(0, 5, **f), K=1, L=2, learn_top=True)
    assert g_enc.shape == (0, 192) and gx.shape == (0, 5, 2)
    assert g_glow.numel() == 30000 and bool((g_glow == 0).all()) and bool((g_pe == 0).all())
    gx, gy, g_glow = ops.cglow_levels_flow_backward(glb, torch.zeros(0, 3, 8, 8, **f), torch.zeros(0, 3, 8, 8, **f),
                                                    None, None, K=1, L=2, learn_top=True)
    assert gx.shape == (0, 3, 8, 8) and bool((g_glow == 0).all())


# ---- 6. through DPF ----
def test_dpf_training_pass_hip_backward_matches_recompute(monkeypatch):
    """One supervised training loss through DPF(-K 1 -L 2 --learn_top True, CGLOW): the parameters
    that get a gradient and their gradients agree between the HIP backward and the recompute
    (same HIP forward) under the bar of test_gpu_backward.py's training-pass comparison.  A
    self-comparison: it checks the wiring; parity is the tests above."""
    import torch.nn as nn
    from nfdpf import autograd as ag
    from nfdpf import ops
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import make_args, synthetic_disk
    from DPFs import DPF
    calls = _spy(monkeypatch, ops, "cglow_levels_measurement_backward")
    B, N, T = 2, 64, 3
    flags = dict(NF_dyn=True, NF_cond=True, measurement="CGLOW", hiddensize=192, resampler_type="soft",
                 flow_depth=1, num_levels=2, learn_top=True)
    torch.manual_seed(5)
    a = make_args(flags, B, N, T, {})
    dpf = DPF(a)
    _perturb(dpf.cglow_measurement, 0.1, 13)  # off the reference's zero-initialised output convs
    dpf = dpf.to(DEV)
    dpf.encoder = nn.Identity()
    start, state, vel_in, enc = (x.to(DEV) for x in synthetic_disk(B, T, 3, a.hiddensize))
    grads, ncalls = {}, {}
    for mode in (True, False):
        monkeypatch.setattr(ag, "HIP_BACKWARD", mode)
        del calls[:]
        dpf.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        out = dpf.filtering_pos(enc, start, vel_in)
        xs, ps = out[0], out[1]
        pred = (xs * ps[..., None]).sum(2)
        loss = ((pred - state[:, :, :2]) ** 2).mean() + 0.01 * out[-1]
        loss.backward()
        ncalls[mode] = len(calls)
        grads[mode] = {n: p.grad.detach().clone() for n, p in dpf.named_parameters() if p.grad is not None}
    assert ncalls[True] >= 1 and ncalls[False] == 0, ncalls
    assert any("new_mean" in k for k in grads[True]) and set(grads[True]) == set(grads[False])
    for k in grads[False]:
        a_, b_ = grads[True][k].double(), grads[False][k].double()
        scale = float(b_.abs().max()) + 1e-30
        d = float((a_ - b_).abs().max())
        assert d <= 2e-3 * scale + 1e-7, f"{k}: max |d| {d:.3g} vs scale {scale:.3g}"
