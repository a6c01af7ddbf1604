"""Generate tests/golden/cglow_depth.npz by RUNNING THE REFERENCE on the CPU (build container
only, like gen_golden.py, whose helpers this uses): the conditional GLOW at flow depth K > 1.

Flow form, K in (2, 3) -- keys ``k{K}/...``: the reference's CondGlowModel(args with
flow_depth = K), seeded init, every parameter replaced by N(0, 0.1^2) draws (gen_golden.perturb,
as gen_cglow_flow: without it the zero-initialised layers make every step near-identity),
new_mean / new_logs zeroed.  Recorded: the state_dict (``w/``), x, y [37, 3, 8, 8] (two full
16-sample tiles and a ragged one of 5), float32 z and nll, and for seeded g_z, g_nll the float32
autograd dx, dy and parameter gradients (``g/<name>``).

Measurement form, K = 2 -- keys ``meas2/...``: the reference's DPF(measurement=CGLOW,
hiddensize=192, flow_depth=2), B = 3 rows of N = 21 particles (63: row boundaries fall inside
16-particle tiles, the last tile is ragged): enc, x, lik (with the row-max shift), and for a
seeded gl the gradients denc, dx and parameter gradients.

Parameter gradients are one flat float32 array ``g_flat`` (the parameters that got a gradient,
in named_parameters order, names in ``g_names``), which keeps the archive's entry count down.

Every quantity is also computed by the same model in float64, and ``err_abs/<q>`` = max |f32 -
f64|, ``err_rel/<q>`` = err_abs / max |f64| record the reference's own float32 error, the
yardstick of tests/test_gpu_cglow_depth.py (per parameter gradient: ``g_err_abs`` / ``g_err_rel``,
aligned with ``g_names``).  The float64 values themselves are kept where a test compares against
them -- ``f64/nll``, ``f64/lik``, and z as ``f64d/z`` = float32(z64 - z32) (z64 = z32 + f64d to
~1e-14) -- the float64 gradients are not: weights, float32 gradients and float64 gradients
together would pass the 1 MiB limit on a committed file.

    python tests/golden/gen_cglow_depth.py
"""
import copy
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from gen_golden import import_reference, make_args, perturb, sd_np  # noqa: E402


def _err(v32, v64):
    e = float(np.abs(np.asarray(v32).astype(np.float64) - v64).max())
    return e, e / max(float(np.abs(v64).max()), 1e-300)


def _record(out, pre, r32, r64, g32, g64):
    for k, v in r32.items():
        out[f"{pre}/{k}"] = v
        ea, er = _err(v, r64[k])
        out[f"{pre}/err_abs/{k}"], out[f"{pre}/err_rel/{k}"] = np.float64(ea), np.float64(er)
        if k in ("nll", "lik"):
            out[f"{pre}/f64/{k}"] = r64[k]
        elif k == "z":
            out[f"{pre}/f64d/{k}"] = (r64[k] - v.astype(np.float64)).astype(np.float32)
    names = list(g32)
    errs = [_err(g32[n], g64[n]) for n in names]
    out[f"{pre}/g_names"] = np.array(names)
    out[f"{pre}/g_flat"] = np.concatenate([g32[n].reshape(-1) for n in names])
    out[f"{pre}/g_err_abs"] = np.array([e[0] for e in errs])
    out[f"{pre}/g_err_rel"] = np.array([e[1] for e in errs])


def _zero_top(m):
    import torch
    with torch.no_grad():
        m.new_mean.zero_()
        m.new_logs.zero_()


def gen_flow(out, K):
    import torch
    from nf.cglow.CGlowModel import CondGlowModel
    g = torch.Generator().manual_seed(5100 + K)
    torch.manual_seed(5200 + K)
    m = CondGlowModel(make_args(flow_depth=K))
    perturb(m, 0.1, g)
    _zero_top(m)
    M = 37
    x = torch.randn(M, 3, 8, 8, generator=g)
    y = torch.randn(M, 3, 8, 8, generator=g)
    g_z = torch.randn(M, 12, 4, 4, generator=g)
    g_nll = torch.randn(M, generator=g)
    pre = f"k{K}"
    out.update({f"{pre}/w/{k}": v for k, v in sd_np(m).items()})
    out.update({f"{pre}/x": x.numpy(), f"{pre}/y": y.numpy(), f"{pre}/g_z": g_z.numpy(), f"{pre}/g_nll": g_nll.numpy()})

    def run(model, dt):
        xr, yr = x.clone().to(dt).requires_grad_(True), y.clone().to(dt).requires_grad_(True)
        z, nll = model(xr, yr)
        ((z * g_z.to(dt)).sum() + (nll * g_nll.to(dt)).sum()).backward()
        res = {"z": z, "nll": nll, "dx": xr.grad, "dy": yr.grad}
        grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
        return ({k: v.detach().numpy() for k, v in res.items()}, {k: v.detach().numpy() for k, v in grads.items()})

    r32, g32 = run(m, torch.float32)
    r64, g64 = run(copy.deepcopy(m).double(), torch.float64)
    _record(out, pre, r32, r64, g32, g64)
    print(pre, "nll", float(r32["nll"].mean()), "err nll", float(out[f"{pre}/err_abs/nll"]),
          "err z", float(out[f"{pre}/err_abs/z"]), "param grads", len(g32))


def gen_meas(out, K=2):
    import torch
    from DPFs import DPF
    g = torch.Generator().manual_seed(6100 + K)
    torch.manual_seed(6200 + K)
    B, N = 3, 21
    dpf = DPF(make_args(measurement="CGLOW", hiddensize=192, num_particles=N, batchsize=B, flow_depth=K))
    perturb(dpf.particle_encoder, 0.3, g)
    perturb(dpf.cglow_measurement, 0.1, g)
    _zero_top(dpf.cglow_measurement)
    enc = torch.randn(B, 192, generator=g)
    x = torch.randn(B, N, 2, generator=g) * 30
    gl = torch.randn(B, N, generator=g)
    pre = f"meas{K}"
    for kk, v in sd_np(dpf).items():
        if kk.split(".")[0] in ("particle_encoder", "cglow_measurement"):
            out[f"{pre}/w/{kk}"] = v
    out.update({f"{pre}/enc": enc.numpy(), f"{pre}/x": x.numpy(), f"{pre}/gl": gl.numpy()})

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
    print(pre, "err lik", float(out[f"{pre}/err_abs/lik"]), "err denc", float(out[f"{pre}/err_abs/denc"]),
          "err dx", float(out[f"{pre}/err_abs/dx"]), "param grads", len(g32))


def main():
    import_reference()
    out = {}
    for K in (2, 3):
        gen_flow(out, K)
    gen_meas(out, 2)
    path = os.path.join(OUT, "cglow_depth.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
