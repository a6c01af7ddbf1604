"""Generate tests/golden/cglow_widths.npz and cglow_widths_l2.npz by RUNNING THE REFERENCE on the
CPU (build container only, like gen_cglow_levels.py, whose ``_record`` and gen_golden.py helpers
this uses): the conditional GLOW at hidden sizes other than the default 8 / 16 / 8
(--x_hidden_channels XH, --x_hidden_size XS, --y_hidden_channels YH) and at another --y_bins.

Flow form -- keys ``<case>/...``, the keys of gen_cglow_levels.py (``w/``, x, y, z, nll,
``err_abs/*``, ``f64/nll``, ``f64d/z``, and for case a g_z, g_nll, dx, dy, ``g_flat``):

    case  (XH, XS, YH)   K  L  learn_top  y_bins  gradients   file
    a     (16, 32, 16)   1  1  off        256     yes         cglow_widths.npz
    b     (8, 16, 32)    2  2  on         256     no          cglow_widths_l2.npz
    c     (16, 32, 32)   1  2  on         256     no          cglow_widths_l2.npz
    d     (8, 16, 8)     1  1  off        32      no          cglow_widths.npz
    e     (16, 16, 8)    1  1  off        256     no          cglow_widths.npz

(b and c are 378 KB and 287 KB of state, random floats barely compress, and a committed file
stays under 1 MiB: hence two files.)  Every parameter is replaced by N(0, 0.1^2) draws; M = 37
samples (two full 16-sample tiles and a ragged one of 5).

Measurement form (cglow_widths.npz) -- keys ``meas/...``: the reference's DPF(measurement=CGLOW,
hiddensize=192) at a's sizes, B = 3 rows of N = 21 particles: enc, x, lik (with the row-max
shift), and for a seeded gl the gradients denc, dx and parameter gradients.

log|det W| of the per-sample 1x1-conv matrix is a bad yardstick in float32 where W is badly
conditioned: cond(W) is computed in float64 for every step and sample, asserted < 2e4, and its
maximum recorded (``<case>/cond_max``).

    python tests/golden/gen_cglow_widths.py
"""
import copy
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from gen_golden import import_reference, make_args, perturb, sd_np  # noqa: E402
from gen_cglow_depth import _zero_top  # noqa: E402
from gen_cglow_levels import _record  # noqa: E402

COND_CAP = 2e4
CASES = {  # case: (XH, XS, YH), K, L, learn_top, y_bins, gradients
    "a": ((16, 32, 16), 1, 1, False, 256, True),
    "b": ((8, 16, 32), 2, 2, True, 256, False),
    "c": ((16, 32, 32), 1, 2, True, 256, False),
    "d": ((8, 16, 8), 1, 1, False, 32, False),
    "e": ((16, 16, 8), 1, 1, False, 256, False),
}


def width_args(widths, **kw):
    xh, xs, yh = widths
    return make_args(x_hidden_channels=xh, x_hidden_size=xs, y_hidden_channels=yh, **kw)


def max_cond(glow, x):
    """max over steps and samples of cond(W), W the per-sample 1x1-conv matrix, in float64."""
    import torch
    m = copy.deepcopy(glow).double()
    worst = 0.0
    with torch.no_grad():
        for layer in m.flow.layers:
            inv = getattr(layer, "invconv", None)
            if inv is None:
                continue
            w = inv.x_Linear(inv.x_Con(x.double()).view(x.size(0), -1))
            C = int(round(w.size(1) ** 0.5))
            worst = max(worst, float(torch.linalg.cond(w.view(-1, C, C)).max()))
    return worst


def gen_flow(out, case):
    import torch
    from nf.cglow.CGlowModel import CondGlowModel
    widths, K, L, top, bins, grads = CASES[case]
    g = torch.Generator().manual_seed(7300)
    torch.manual_seed(7400)
    m = CondGlowModel(width_args(widths, flow_depth=K, num_levels=L, learn_top=top, y_bins=bins))
    perturb(m, 0.1, g)
    if not top:
        _zero_top(m)
    M = 37
    x = torch.randn(M, 3, 8, 8, generator=g)
    y = torch.randn(M, 3, 8, 8, generator=g)
    g_z = torch.randn((M,) + tuple(m.new_mean.shape[1:]), generator=g)
    g_nll = torch.randn(M, generator=g)
    cond = max_cond(m, x)
    assert cond < COND_CAP, f"case {case}: cond(W) = {cond}"
    out.update({f"{case}/w/{k}": v for k, v in sd_np(m).items()})
    out.update({f"{case}/x": x.numpy(), f"{case}/y": y.numpy(), f"{case}/cond_max": np.float64(cond),
                f"{case}/config": np.array(list(widths) + [K, L, int(top), bins])})
    if grads:
        out.update({f"{case}/g_z": g_z.numpy(), f"{case}/g_nll": g_nll.numpy()})

    def run(model, dt):
        xr, yr = x.clone().to(dt).requires_grad_(True), y.clone().to(dt).requires_grad_(True)
        z, nll = model(xr, yr)
        res = {"z": z, "nll": nll}
        gr = {}
        if grads:
            ((z * g_z.to(dt)).sum() + (nll * g_nll.to(dt)).sum()).backward()
            res.update({"dx": xr.grad, "dy": yr.grad})
            gr = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
        return ({k: v.detach().numpy() for k, v in res.items()}, {k: v.detach().numpy() for k, v in gr.items()})

    r32, g32 = run(m, torch.float32)
    r64, g64 = run(copy.deepcopy(m).double(), torch.float64)
    _record(out, case, r32, r64, g32, g64)
    print(case, widths, "params", sum(p.numel() for p in m.parameters()), "nll", float(r32["nll"].mean()), "cond", cond,
          "err nll", float(out[f"{case}/err_abs/nll"]), "err z", float(out[f"{case}/err_abs/z"]), "param grads", len(g32))


def gen_meas(out):
    import torch
    from DPFs import DPF
    widths = CASES["a"][0]
    g = torch.Generator().manual_seed(8300)
    torch.manual_seed(8400)
    B, N = 3, 21
    dpf = DPF(width_args(widths, measurement="CGLOW", hiddensize=192, num_particles=N, batchsize=B, flow_depth=1,
                         num_levels=1, learn_top=False))
    perturb(dpf.particle_encoder, 0.3, g)
    perturb(dpf.cglow_measurement, 0.1, g)
    _zero_top(dpf.cglow_measurement)
    enc = torch.randn(B, 192, generator=g)
    x = torch.randn(B, N, 2, generator=g) * 30
    gl = torch.randn(B, N, generator=g)
    pre = "meas"
    for kk, v in sd_np(dpf).items():
        if kk.split(".")[0] in ("particle_encoder", "cglow_measurement"):
            out[f"{pre}/w/{kk}"] = v
    out.update({f"{pre}/enc": enc.numpy(), f"{pre}/x": x.numpy(), f"{pre}/gl": gl.numpy()})
    with torch.no_grad():
        es = dpf.particle_encoder(x.reshape(-1, 2)).reshape(B * N, 3, 8, 8)
    cond = max_cond(dpf.cglow_measurement, es)
    assert cond < COND_CAP, f"meas: cond(W) = {cond}"
    out[f"{pre}/cond_max"] = np.float64(cond)

    def run(mm, dt):
        er, xr = enc.clone().to(dt).requires_grad_(True), x.clone().to(dt).requires_grad_(True)
        if dt == torch.float32:
            lik = mm(er, xr)
        else:
            # the reference's forward (model/models.py:286-303) casts the particles and their
            # encoder to float32; the float64 yardstick composes the same modules without the cast
            es = mm.particle_encoder(xr.reshape(-1, 2)).reshape(B * N, 3, 8, 8)
            eo = er[:, None, :].repeat(1, N, 1).reshape(B * N, 3, 8, 8)
            lik = -mm.CGLOW(es, eo)[1].reshape(B, N)
            lik = lik - lik.max(dim=-1, keepdim=True)[0]
        (lik * gl.to(dt)).sum().backward()
        res = {"lik": lik, "denc": er.grad, "dx": xr.grad}
        grads = {n: p.grad for n, p in mm.named_parameters() if p.grad is not None}
        return ({k: v.detach().numpy() for k, v in res.items()}, {k: v.detach().numpy() for k, v in grads.items()})

    mm = dpf.measurement_model
    r32, g32 = run(mm, torch.float32)
    r64, g64 = run(copy.deepcopy(mm).double(), torch.float64)
    _record(out, pre, r32, r64, g32, g64)
    print(pre, "cond", cond, "err lik", float(out[f"{pre}/err_abs/lik"]), "err denc", float(out[f"{pre}/err_abs/denc"]),
          "err dx", float(out[f"{pre}/err_abs/dx"]), "param grads", len(g32))


def main():
    import_reference()
    for name, cases, meas in (("cglow_widths.npz", "ade", True), ("cglow_widths_l2.npz", "bc", False)):
        out = {}
        for case in cases:
            gen_flow(out, case)
        if meas:
            gen_meas(out)
        path = os.path.join(OUT, name)
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
