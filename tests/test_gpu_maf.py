"""The MAF stack kernels -- nfdpf_maf_stack (csrc/flows.hip, maf_forward / maf_inverse of
csrc/flows.hpp) and nfdpf_maf_stack_backward (csrc/maf_bwd.hip) -- against a plain out-of-place
restatement of NormalizingFlowModel over MAF flows (nf/models.py:13-30, nf/flows.py:241-284) in
float64, with the same restatement in float32 sizing the envelope.  GPU box only.

The restatement (_ref_flow / _ref_stack) shares no code with the package: it reads the weights off
the modules' nn.Linear layers and builds the columns in a list, so autograd differentiates the
inverse too (the reference's own MAF.inverse writes x in place while reading it, and raises).

Bars.  Values, per element: |ours - f64| <= max(4 |f32 - f64|, floor), floor 1e-5 |f64| + 1e-5 for
the output and 1e-5 |f64| + 1e-6 for the log-det (the floors of test_gpu_parity.test_maf_golden);
at std = 1.0 each floor is raised by TANH_EPS x _tanh_sensitivity, for the reason and with the
figures in test_maf_stack_values_vs_f64's docstring.
Gradients: test_gpu_backward._check, per element
|ours - f64| <= max(4 |f32 - f64| + 1e-6 scale, 2e-4 |f64| + 2e-5 scale).

Worst ratio of |ours - f64| to its envelope measured on an MI355X (each test prints its own; 1.0
is the bar), forward / inverse:

  values (D, flows, std, rows)      z            log-det
    (2, 1, 0.3, 1)                0.010 / 0.013     0.008 / 0.005
    (2, 2, 0.0, 1000)             0.018 / 0.018     0.094 / 0.113
    (2, 2, 0.3, 255)              0.020 / 0.069     0.025 / 0.029
    (2, 4, 0.3, 257)              0.091 / 0.264     0.074 / 0.038
    (3, 2, 0.3, 100)              0.033 / 0.037     0.138 / 0.168
    (4, 2, 0.3, 256)              0.059 / 0.035     0.278 / 0.235
    (4, 3, 0.3, 65)               0.061 / 0.065     0.216 / 0.301
    (6, 2, 0.3, 100)              0.056 / 0.066     0.203 / 0.106
    (8, 2, 0.3, 129)              0.067 / 0.049     0.400 / 0.224
    (2, 2, 1.0, 1000)             0.537 / 0.227     0.636 / 0.267   (floors raised by the tanh term)
    (4, 2, 1.0, 257)              0.445 / 0.507     0.480 / 0.477   (floors raised by the tanh term)
    saturated (2, 2, 0.3, 257)    0.022 / 0.104     0.029 / 0.057
  gradients (D, flows, std, rows)   worst tensor
    (2, 1, 0.3, 1)                0.002 / 0.069
    (2, 2, 0.3, 63)               0.021 / 0.011
    (2, 2, 0.3, 64)               0.018 / 0.060
    (2, 4, 0.3, 65)               0.035 / 0.052
    (2, 2, 0.0, 1000)             0.019 / 0.009
    (2, 2, 1.0, 1000)             0.100 / 0.165
    (4, 1, 0.3, 129)              0.030 / 0.026
    (4, 2, 0.3, 257)              0.036 / 0.032
    (4, 2, 1.0, 257)              0.692 / 0.640
  declined (D, flows)               worst tensor (PyTorch-recompute backward)
    (3, 2)                        0.020 / 0.010
    (4, 3)                        0.021 / 0.034
    (8, 1)                        0.014 / 0.024
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from test_gpu_backward import _check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BLOCK = 256  # kStackBlock, the forward kernels' workgroup size (csrc/flows.hip)
H = 8


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from nfdpf import _lib
    _lib.load()


# ------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------
def _ref_net(fcnn, u, dt, taps=None):
    """FCNN (nf/flows.py:101-114).  With ``taps`` a zero leaf is added to every tanh output and
    collected there: d(output)/d(tap) is the output's sensitivity to that unit's tanh."""
    l0, l2, l4 = [m for m in fcnn.network if isinstance(m, torch.nn.Linear)]
    h = u
    for lin in (l0, l2):
        h = torch.tanh(F.linear(h, lin.weight.to(dt), lin.bias.to(dt)))
        if taps is not None:
            taps.append(torch.zeros_like(h, requires_grad=True))
            h = h + taps[-1]
    return F.linear(h, l4.weight.to(dt), l4.bias.to(dt))


def _ref_flow(f, v, inverse, dt, taps=None):
    """One MAF flow (nf/flows.py:259-284), out of place: (output, log-det)."""
    rows, D = v.shape
    ip = f.initial_param.to(dt)
    src = v.flip(1) if inverse else v
    cols, ld = [], torch.zeros(rows, dtype=dt)
    for i in range(D):
        if i == 0:
            mu, alpha = ip[0].expand(rows), ip[1].expand(rows)
        else:
            # the net of dimension i sees the first i INPUTS (forward) or the first i outputs
            # already produced (inverse)
            o = _ref_net(f.layers[i - 1], torch.stack(cols, 1) if inverse else v[:, :i], dt, taps)
            mu, alpha = o[:, 0], o[:, 1]
        if inverse:
            cols.append(mu + torch.exp(alpha) * src[:, i])
            ld = ld + alpha
        else:
            cols.append((src[:, i] - mu) / torch.exp(alpha))
            ld = ld - alpha
    out = torch.stack(cols, 1)
    return (out if inverse else out.flip(1)), ld


def _ref_stack(flows, v, inverse, dt, taps=None):
    """NormalizingFlowModel.forward / .inverse (nf/models.py:13-30): (output, log-det)."""
    ld = torch.zeros(v.shape[0], dtype=dt)
    for f in (flows[::-1] if inverse else flows):
        v, l = _ref_flow(f, v, inverse, dt, taps)
        ld = ld + l
    return v, ld


# ------------------------------------------------------------------------------------------
# models, inputs, envelopes
# ------------------------------------------------------------------------------------------
def _build(D, n_flows, std, seed=None):
    """MAF(D) flows with their own initialisation plus N(0, std^2) on every parameter (CPU)."""
    from nf.flows import MAF
    seed = D * 1000 + n_flows * 10 + int(std * 10) if seed is None else seed
    torch.manual_seed(seed)
    flows = [MAF(D, H) for _ in range(n_flows)]
    g = torch.Generator().manual_seed(seed + 1)
    if std:
        with torch.no_grad():
            for f in flows:
                for p in f.parameters():
                    p.add_(torch.randn(p.shape, generator=g) * std)
    return flows


def _blob(flows):
    from nfdpf.pack import flows_tensors
    if not flows:
        return torch.zeros(1, device=DEV)
    return torch.cat([a.detach().reshape(-1) for a in flows_tensors(flows)]).float().contiguous().to(DEV)


def _inputs(rows, D, seed=None):
    """x = 2 randn, cotangents randn for the output and the log-det (CPU, float32)."""
    g = torch.Generator().manual_seed(rows * 10 + D if seed is None else seed)
    return (torch.randn(rows, D, generator=g) * 2, torch.randn(rows, D, generator=g),
            torch.randn(rows, generator=g))


def _ref_values(flows, x, inverse):
    with torch.no_grad():
        return [_ref_stack([copy.deepcopy(f).to(dt) for f in flows], x.to(dt), inverse, dt)
                for dt in (torch.float32, torch.float64)]


TANH_EPS = 6e-8  # absolute error of tanh_fast (1 - 2 / (1 + e^{2x}), csrc/common.hpp)


def _tanh_sensitivity(flows, x, inverse):
    """Per row and output, sum over every tanh unit of the stack of |d output / d tanh| in float64
    (output [rows, D], log-det [rows]): times TANH_EPS, a first-order bound of what an absolute
    error of TANH_EPS in each tanh does to that output."""
    dt = torch.float64
    taps = []
    out, ld = _ref_stack([copy.deepcopy(f).to(dt) for f in flows], x.to(dt), inverse, dt, taps)

    def l1(y):
        gs = torch.autograd.grad(y.sum(), taps, retain_graph=True, allow_unused=True)  # rows are independent
        return sum(g.abs().sum(1) for g in gs if g is not None)
    return torch.stack([l1(out[:, k]) for k in range(out.shape[1])], 1), l1(ld)


def _value_check(ours, r32, r64, rel, ab, what, extra=None):
    """|ours - f64| <= max(4 |f32 - f64|, rel |f64| + ab [+ extra]) per element."""
    ours, r32, r64 = ours.double().cpu(), r32.double(), r64.double()
    assert bool(torch.isfinite(r32).all()) and bool(torch.isfinite(r64).all()), f"{what}: reference not finite"
    assert bool(torch.isfinite(ours).all()), f"{what}: kernel output not finite"
    d = (ours - r64).abs()
    floor = rel * r64.abs() + ab
    env = torch.maximum(4 * (r32 - r64).abs(), floor if extra is None else floor + extra)
    ratio = float((d / env).max()) if d.numel() else 0.0
    print(f"ratio {what}: {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: {int((d > env).sum())}/{d.numel()} outside; worst |d| / envelope {ratio:.3g}"


def _values_vs_f64(flows, x, what, tanh_term=False):
    from nfdpf import ops
    b = _blob(flows)
    for inverse in (False, True):
        out, ld = ops.maf_stack(b, len(flows), x.shape[1], H, x.to(DEV), inverse)
        (o32, l32), (o64, l64) = _ref_values(flows, x, inverse)
        s_out, s_ld = _tanh_sensitivity(flows, x, inverse) if tanh_term else (None, None)
        tag = f"{what} {'inv' if inverse else 'fwd'}"
        _value_check(out, o32, o64, 1e-5, 1e-5, tag + " z", None if s_out is None else TANH_EPS * s_out)
        _value_check(ld, l32, l64, 1e-5, 1e-6, tag + " logdet", None if s_ld is None else TANH_EPS * s_ld)


def _ref_grads(flows, x, inverse, w_out, w_ld):
    """Per dtype: [d/dx] + [d/dp for every parameter, flows in order] of the reference loss
    sum(out w_out) + sum(ld w_ld); a term whose weight is None is left out."""
    res = []
    for dt in (torch.float32, torch.float64):
        rf = [copy.deepcopy(f).cpu().to(dt) for f in flows]
        xr = x.detach().cpu().to(dt).requires_grad_(True)
        out, ld = _ref_stack(rf, xr, inverse, dt)
        loss = 0
        if w_out is not None:
            loss = loss + (out * w_out.to(dt)).sum()
        if w_ld is not None:
            loss = loss + (ld * w_ld.to(dt)).sum()
        wrt = [xr] + [p for f in rf for p in f.parameters()]
        gs = torch.autograd.grad(loss, wrt, allow_unused=True)
        res.append([torch.zeros_like(t) if g is None else g for g, t in zip(gs, wrt)])
    return res


def _grad_ratio(ours, r32, r64):
    """|ours - f64| over the envelope of test_gpu_backward._check (figures for the docstring)."""
    ours, r32, r64 = ours.double().cpu(), r32.double().cpu(), r64.double().cpu()
    scale = float(r64.abs().max()) + 1e-30
    env = torch.maximum(4 * (r32 - r64).abs() + 1e-6 * scale, 2e-4 * r64.abs() + 2e-5 * scale)
    return float(((ours - r64).abs() / env).max()) if ours.numel() else 0.0


def _count_backward(monkeypatch):
    """Wrap ops.maf_stack_backward: every call's result is appended to the returned list."""
    from nfdpf import ops
    got = []
    real = ops.maf_stack_backward

    def wrapped(*a, **k):
        r = real(*a, **k)
        got.append(r)
        return r
    monkeypatch.setattr(ops, "maf_stack_backward", wrapped)
    return got


def _module_grads_vs_f64(D, n_flows, std, rows, inverse, monkeypatch, expect_kernel):
    from nf.models import NormalizingFlowModel
    got = _count_backward(monkeypatch)
    flows = _build(D, n_flows, std)
    ref_flows = copy.deepcopy(flows)
    x, w_out, w_ld = _inputs(rows, D)
    model = NormalizingFlowModel(None, flows, device=DEV)
    xd = x.to(DEV).requires_grad_(True)
    if inverse:
        out, ld = model.inverse(xd)
    else:
        out, _, ld = model.forward(xd)
    loss = (out * w_out.to(DEV)).sum() + (ld * w_ld.to(DEV)).sum()
    params = [p for f in flows for p in f.parameters()]
    ours = torch.autograd.grad(loss, [xd] + params)
    assert len(got) == 1, "the backward did not go through ops.maf_stack_backward exactly once"
    if expect_kernel:
        assert got[0] is not None, "nfdpf_maf_stack_backward declined: the recompute ran instead"
    else:
        assert got[0] is None, "nfdpf_maf_stack_backward was expected to decline these sizes"
    r32, r64 = _ref_grads(ref_flows, x, inverse, w_out, w_ld)
    names = ["x"] + [f"flow{i}.{n}" for i, f in enumerate(flows) for n, _ in f.named_parameters()]
    what = f"D={D} flows={n_flows} std={std} rows={rows} {'inv' if inverse else 'fwd'}"
    worst = max(_grad_ratio(a, b, c) for a, b, c in zip(ours, r32, r64))
    print(f"ratio grads {what}: {worst:.3f}")
    for name, a, b, c in zip(names, ours, r32, r64):
        assert a is not None, name
        _check(a, b, c, f"{name} ({what})")


# ------------------------------------------------------------------------------------------
# 1. forward and inverse values
# ------------------------------------------------------------------------------------------
VALUE_CASES = [  # (D, n_flows, std, rows)
    (2, 1, 0.3, 1),
    (2, 2, 0.0, 1000),         # the reference initialisation untouched
    (2, 2, 0.3, BLOCK - 1),
    (2, 4, 0.3, BLOCK + 1),    # a second block of one row
    (3, 2, 0.3, 100),
    (4, 2, 0.3, BLOCK),
    (4, 3, 0.3, 65),
    (6, 2, 0.3, 100),
    (8, 2, 0.3, 129),
    (2, 2, 1.0, 1000),
    (4, 2, 1.0, 257),
]


@pytest.mark.parametrize("D,n_flows,std,rows", VALUE_CASES)
def test_maf_stack_values_vs_f64(D, n_flows, std, rows):
    """The floors are those of test_maf_golden, except at std = 1.0, where each floor is raised by
    TANH_EPS x _tanh_sensitivity.  Reason: the kernels' tanh_fast has an absolute error near 6e-8
    by design (csrc/common.hpp) and the floors leave it no room once the weights are ~N(0, 1): a
    unit's error reaches mu and alpha times |W3| (and |W3| |W2| from the first layer), and z
    times e^{-alpha} / the log-det summed over D x flows nets.  The term is computed from the
    float64 reference alone; it reaches 34 x the z floor and 11 x the log-det floor on the worst
    rows of these two cases (0.02 .. 2.7 x at std <= 0.3, where the floors stay as they are).
    Measured on an MI355X against the unraised floors (max(4 |f32 - f64|, floor)), worst
    |ours - f64| / envelope: forward z 1.48 at D = 2 and 1.31 at D = 4 with the float32
    restatement evaluated on the GPU host; the same kernel outputs against a restatement evaluated
    on another host (the 4 x term moves with the host's float32 rounding): D = 2 forward 1.16 (z)
    and 1.33 (log-det); D = 4 forward 1.48 / 2.27, inverse 8.2 / 4.1 -- in the last, row 102:
    |d| 2.7e-4 on z = 2.26, where a float32 evaluation with the tanh_fast formula and
    float64-accurate dot products is 1.3e-4 off, one with an exact tanh 4.7e-5, and the float32
    restatement 3e-7 (the placement of its rounding is arbitrary on such a row).  The kernel's
    arithmetic is what its header says; the floor was what did not fit.  With the raised floors
    the worst ratios are those of the module docstring (0.2 .. 0.7)."""
    _values_vs_f64(_build(D, n_flows, std), _inputs(rows, D)[0], f"values D={D} flows={n_flows} std={std} rows={rows}",
                   tanh_term=std >= 1.0)


SAT_SCALE = 100.0


def _saturated(D, n_flows):
    flows = _build(D, n_flows, 0.3)
    with torch.no_grad():
        for f in flows:
            for net in f.layers:
                net.network[0].weight.mul_(SAT_SCALE)
    return flows


def test_maf_stack_values_saturated_nets():
    """First-layer weights of every net x 100: over half of the pre-activations lie past
    +-44, where the e^{2x} of tanh_fast (1 - 2 / (1 + e^{2x}), csrc/common.hpp) overflows to inf
    or underflows to 0, and they reach +-700; the outputs stay finite and inside the envelope of
    the value cases (unraised floors).  D = 2 and two flows keep the case about the overflow:
    with more inputs per net, a unit that is NOT saturated has a pre-activation that is a small
    difference of products ~ +-200, whose float32 rounding (ulp 1.5e-5) no float32 evaluation
    keeps inside this envelope (at D = 4 one with an exact tanh and float64-accurate dot products
    misses it too, by 1.07); and every further flow multiplies the error reaching such a unit by
    its weight ~100 (four flows at D = 2: 1.24 on one element of 514, a float32 evaluation with
    float64-accurate dot products 0.20).  Both would test conditioning, not the overflow.  The
    float64 outputs reach 43."""
    D, n_flows, rows = 2, 2, 257
    flows = _saturated(D, n_flows)
    x = _inputs(rows, D)[0]
    with torch.no_grad():
        pre = F.linear(x[:, :1], flows[0].layers[0].network[0].weight, flows[0].layers[0].network[0].bias)
    assert float(pre.abs().max()) > 100.0 and float((pre.abs() > 44.0).float().mean()) > 0.5
    _values_vs_f64(flows, x, f"values saturated D={D} flows={n_flows} rows={rows}")


def test_maf_stack_zero_flows_is_identity():
    from nfdpf import ops
    x = _inputs(BLOCK + 1, 4)[0].to(DEV)
    for inverse in (False, True):
        out, ld = ops.maf_stack(_blob([]), 0, 4, H, x, inverse)
        assert torch.equal(out, x) and bool((ld == 0).all())


def test_maf_stack_zero_rows():
    from nfdpf import ops
    out, ld = ops.maf_stack(_blob(_build(2, 2, 0.3)), 2, 2, H, torch.zeros(0, 2, device=DEV), True)
    assert out.shape == (0, 2) and ld.shape == (0,)


@pytest.mark.parametrize("D,hidden", [(5, 8), (2, 16)])
def test_maf_stack_unsupported_arguments(D, hidden):
    """Refused by the checked return of nfdpf_maf_stack, which precedes every launch: the error
    names the sets the library is built for."""
    from nfdpf import ops
    from nfdpf._lib import NfdpfError
    with pytest.raises(NfdpfError) as e:
        ops.maf_stack(torch.zeros(4096, device=DEV), 2, D, hidden, torch.zeros(10, D, device=DEV), False)
    assert "{2,3,4,6,8}" in str(e.value) and "hidden 8" in str(e.value)
    assert f"dim={D}, hidden={hidden}" in str(e.value)


# ------------------------------------------------------------------------------------------
# 2. the HIP backward through the modules
# ------------------------------------------------------------------------------------------
GRAD_CASES = [  # (D, n_flows, std, rows)
    (2, 1, 0.3, 1),
    (2, 2, 0.3, 63),
    (2, 2, 0.3, 64),           # exactly one wave (kMafRows, csrc/maf_bwd.hip)
    (2, 4, 0.3, 65),           # kMafMaxFlows; the second wave has one valid lane
    (2, 2, 0.0, 1000),
    (2, 2, 1.0, 1000),
    (4, 1, 0.3, 129),
    (4, 2, 0.3, 257),
    (4, 2, 1.0, 257),
]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("D,n_flows,std,rows", GRAD_CASES)
def test_maf_stack_backward_vs_f64(D, n_flows, std, rows, inverse, monkeypatch):
    _module_grads_vs_f64(D, n_flows, std, rows, inverse, monkeypatch, expect_kernel=True)


# ------------------------------------------------------------------------------------------
# 3. the decline path
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("D,n_flows", [(3, 2), (4, 3), (8, 1)])
def test_maf_stack_backward_declines_to_recompute(D, n_flows, inverse, monkeypatch):
    """Sizes the kernel does not cover: ops.maf_stack_backward returns None and autograd
    differentiates the PyTorch recompute, whose gradients meet the kernel's envelope."""
    _module_grads_vs_f64(D, n_flows, 0.3, 100, inverse, monkeypatch, expect_kernel=False)


def test_maf_stack_backward_c_abi_refuses():
    from nfdpf import _lib as L
    lib = L.lib()
    for n_flows, dim, hidden in [(2, 3, 8), (2, 2, 16), (0, 2, 8), (5, 2, 8)]:
        assert lib.nfdpf_maf_stack_backward_workspace(n_flows, dim, hidden, 100) == -1
    # dim 4, three flows: 3 x 110 factors x 64 rows x 4 B = 84 480 B of LDS > 65 536
    flows = _build(4, 3, 0.3)
    b = _blob(flows)
    x, go, gl = (a.to(DEV) for a in _inputs(100, 4))
    nbytes = lib.nfdpf_maf_stack_backward_workspace(3, 4, H, 100)
    assert nbytes > 0
    ws = torch.empty(nbytes // 4, device=DEV)
    gx = torch.full_like(x, float("nan"))
    gb = torch.full_like(b, float("nan"))
    rc = lib.nfdpf_maf_stack_backward(b.data_ptr(), 3, 4, H, x.data_ptr(), 100, 1, go.data_ptr(), gl.data_ptr(),
                                      gx.data_ptr(), gb.data_ptr(), ws.data_ptr(), L.stream_ptr(DEV))
    assert rc == L.NFDPF_EINVAL
    assert "LDS factor budget" in lib.nfdpf_last_error().decode()
    assert bool(torch.isnan(gx).all()) and bool(torch.isnan(gb).all()), "refused, yet something was written"


# ------------------------------------------------------------------------------------------
# 4. the backward's contract
# ------------------------------------------------------------------------------------------
def _ops_case(D, n_flows, rows, std=0.3):
    flows = _build(D, n_flows, std)
    x, go, gl = _inputs(rows, D)
    return flows, _blob(flows), x, go, gl


def test_maf_stack_backward_deterministic():
    """Fixed-order partial sums (csrc/maf_bwd.hip header): two calls give identical bits."""
    from nfdpf import ops
    _, b, x, go, gl = _ops_case(4, 2, 1000)
    first = ops.maf_stack_backward(b, 2, 4, H, x.to(DEV), True, go.to(DEV), gl.to(DEV))
    again = ops.maf_stack_backward(b, 2, 4, H, x.to(DEV), True, go.to(DEV), gl.to(DEV))
    for u, v in zip(first, again):
        assert torch.equal(u, v)


@pytest.mark.parametrize("D", [2, 4])
def test_maf_stack_backward_zero_rows(D):
    from nfdpf import ops
    b = _blob(_build(D, 2, 0.3))
    gx, gb = ops.maf_stack_backward(b, 2, D, H, torch.zeros(0, D, device=DEV), True, torch.zeros(0, D, device=DEV),
                                    torch.zeros(0, device=DEV))
    assert gx.shape == (0, D) and gb.shape == b.shape and bool((gb == 0).all())


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("D,n_flows,rows", [(2, 2, 100), (4, 2, 65)])
def test_maf_stack_backward_null_cotangents(D, n_flows, rows, inverse):
    """A null g_out / g_logdet is a zero cotangent, bit for bit, and the result is the gradient
    of the loss with the other term alone (float64 envelope, blob layout)."""
    from nfdpf import ops
    from nfdpf.pack import flows_tensors
    flows, b, x, go, gl = _ops_case(D, n_flows, rows)
    xd, go_d, gl_d = x.to(DEV), go.to(DEV), gl.to(DEV)
    for name, null_args, zero_args, w_out, w_ld in [
            ("g_out", (None, gl_d), (torch.zeros_like(go_d), gl_d), None, gl),
            ("g_logdet", (go_d, None), (go_d, torch.zeros_like(gl_d)), go, None)]:
        gx, gb = ops.maf_stack_backward(b, n_flows, D, H, xd, inverse, *null_args)
        gx0, gb0 = ops.maf_stack_backward(b, n_flows, D, H, xd, inverse, *zero_args)
        assert torch.equal(gx, gx0) and torch.equal(gb, gb0), f"null {name} != zero {name}"
        refs = []
        for gs in _ref_grads(flows, x, inverse, w_out, w_ld):
            # the reference's parameter gradients gathered into the blob's layout
            by_param = {id(p): g for p, g in zip([p for f in flows for p in f.parameters()], gs[1:])}
            packed = flows_tensors(flows, lambda p: by_param[id(p)])
            refs.append((gs[0], torch.cat([a.reshape(-1) for a in packed])))
        what = f"null {name} D={D} {'inv' if inverse else 'fwd'}"
        _check(gx, refs[0][0], refs[1][0], "g_x, " + what)
        _check(gb, refs[0][1], refs[1][1], "g_blob, " + what)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("D,n_flows", [(2, 4), (4, 2)])
def test_maf_stack_backward_writes_every_output(D, n_flows, inverse):
    """The C entry point on NaN-filled g_x, g_params and workspace (ops passes torch.empty
    buffers): 65 rows, so the second wave has one valid lane.  Every element of the three is
    overwritten, and the outputs are what ops.maf_stack_backward returns."""
    from nfdpf import _lib as L
    from nfdpf import ops
    lib = L.lib()
    rows = 65
    _, b, x, go, gl = _ops_case(D, n_flows, rows)
    x, go, gl = x.to(DEV), go.to(DEV), gl.to(DEV)
    want_gx, want_gb = ops.maf_stack_backward(b, n_flows, D, H, x, inverse, go, gl)
    nbytes = int(lib.nfdpf_maf_stack_backward_workspace(n_flows, D, H, rows))
    assert nbytes == 4 * 2 * b.numel()  # two waves' partial sums of every parameter
    nan = float("nan")
    ws = torch.full((nbytes // 4,), nan, device=DEV)
    gx, gb = torch.full_like(x, nan), torch.full_like(b, nan)
    rc = lib.nfdpf_maf_stack_backward(b.data_ptr(), n_flows, D, H, x.data_ptr(), rows, int(inverse), go.data_ptr(),
                                      gl.data_ptr(), gx.data_ptr(), gb.data_ptr(), ws.data_ptr(), L.stream_ptr(DEV))
    assert rc == L.NFDPF_OK, lib.nfdpf_last_error().decode()
    assert bool(torch.isfinite(want_gx).all()) and bool(torch.isfinite(want_gb).all())
    assert torch.equal(gx, want_gx) and torch.equal(gb, want_gb)
    assert bool(torch.isfinite(ws).all()), "part of the partial-sum workspace was not written"


@pytest.mark.parametrize("inverse", [False, True])
def test_maf_stack_noncontiguous_input(inverse):
    """A column slice of a wider tensor gives what its contiguous copy gives."""
    from nfdpf import ops
    D, n_flows, rows = 4, 2, 100
    _, b, _, go, gl = _ops_case(D, n_flows, rows)
    wide = _inputs(rows, D + 3)[0].to(DEV)
    x = wide[:, 1:1 + D]
    assert not x.is_contiguous()
    for u, v in zip(ops.maf_stack(b, n_flows, D, H, x, inverse), ops.maf_stack(b, n_flows, D, H, x.contiguous(), inverse)):
        assert torch.equal(u, v)
    go, gl = go.to(DEV), gl.to(DEV)
    for u, v in zip(ops.maf_stack_backward(b, n_flows, D, H, x, inverse, go, gl),
                    ops.maf_stack_backward(b, n_flows, D, H, x.contiguous(), inverse, go, gl)):
        assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------
# 5. one training pass with MAF dynamics
# ------------------------------------------------------------------------------------------
def test_training_step_maf_dynamics_hip_backward_matches_recompute(monkeypatch):
    """test_gpu_backward.test_training_step_hip_backward_matches_recompute with the MAF dynamic
    flow (BASELINE configuration C4's dynamics): parameter gradients of one training pass with the
    HIP MAF backward == with the PyTorch-recompute backward, and the kernel did run."""
    import torch.nn as nn
    from bench import make_args, synthetic_disk
    from DPFs import DPF
    from nfdpf import autograd as ag
    got = _count_backward(monkeypatch)
    B, N, T = 4, 200, 4
    flags = dict(NF_dyn=True, NF_cond=True, NF_dyn_flow="MAF", measurement="cos", resampler_type="soft",
                 force_resample=True)
    torch.manual_seed(5)
    a = make_args(flags, B, N, T, {})
    dpf = DPF(a).to(DEV)
    dpf.encoder = nn.Identity()
    start, state, vel_in, enc = (x.to(DEV) for x in synthetic_disk(B, T, 3, a.hiddensize))
    grads, calls = {}, {}
    for mode in (True, False):
        monkeypatch.setattr(ag, "HIP_BACKWARD", mode)
        del got[:]
        dpf.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        out = dpf.filtering_pos(enc, start, vel_in)
        xs, ps = out[0], out[1]
        pred = (xs * ps[..., None]).sum(2)
        loss = ((pred - state[:, :, :2]) ** 2).mean() + 0.01 * out[-1]
        loss.backward()
        calls[mode] = list(got)
        grads[mode] = {n: p.grad.detach().clone() for n, p in dpf.named_parameters() if p.grad is not None}
    assert calls[True] and all(r is not None for r in calls[True]), "the MAF backward kernel did not run"
    assert not calls[False]
    assert any(k.startswith("nf_dyn.") for k in grads[True]) and set(grads[True]) == set(grads[False])
    for k in grads[False]:
        a_, b_ = grads[True][k].double(), grads[False][k].double()
        scale = float(b_.abs().max()) + 1e-30
        d = float((a_ - b_).abs().max())
        assert d <= 2e-3 * scale + 1e-7, f"{k}: max |d| {d:.3g} vs scale {scale:.3g}"
