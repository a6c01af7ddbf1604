"""Generate tests/golden/cglow_levels.npz and cglow_levels_top.npz by RUNNING THE REFERENCE on
the CPU (build container only, like gen_cglow_depth.py, whose conventions and gen_golden.py
helpers this uses): the conditional GLOW with two levels (-L 2) and / or a learnt top prior
(--learn_top True).

Flow form, (K, L, top) in (1, 2, off), (2, 2, on), (1, 1, on) (cglow_levels.npz) and (1, 2, on)
(cglow_levels_top.npz) -- keys ``k{K}l{L}t{0|1}/...``: the reference's CondGlowModel, seeded
init, every parameter replaced by N(0, 0.1^2) draws -- new_mean / new_logs included where learn_top is on, zeroed where
it is off.  Recorded: the state_dict (``w/``), x, y [37, 3, 8, 8] (two full 16-sample tiles and
a ragged one of 5), float32 z (the FINAL z: [37, 24, 2, 2] at L = 2) and nll.  For (1, 2, on) and
(1, 1, on) also seeded g_z, g_nll and the float32 autograd dx, dy and parameter gradients
(``g_flat`` in named_parameters order, names in ``g_names``).

Measurement form (cglow_levels_top.npz, next to the flow form of the same configuration: one
file for everything would pass the 1 MiB limit on a committed file) -- keys ``meas/...``: the
reference's DPF(measurement=CGLOW, hiddensize=192, flow_depth=1, num_levels=2, learn_top=True), B = 3 rows of N = 21 particles:
enc, x, lik (with the row-max shift), and for a seeded gl the gradients denc, dx and parameter
gradients.

Every quantity is also computed by the same model in float64: ``err_abs/<q>``, ``err_rel/<q>``,
``f64/nll``, ``f64/lik``, ``f64d/z``, ``g_err_abs`` / ``g_err_rel`` as in gen_cglow_depth.py.

    python tests/golden/gen_cglow_levels.py
"""
import copy
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from gen_golden import import_reference, make_args, perturb, sd_np  # noqa: E402
from gen_cglow_depth import _err, _zero_top  # noqa: E402


def _record(out, pre, r32, r64, g32, g64):
    for k, v in r32.items():
        out[f"{pre}/{k}"] = v
        ea, er = _err(v, r64[k])
        out[f"{pre}/err_abs/{k}"], out[f"{pre}/err_rel/{k}"] = np.float64(ea), np.float64(er)
        if k in ("nll", "lik"):
            out[f"{pre}/f64/{k}"] = r64[k]
        elif k == "z":
            out[f"{pre}/f64d/{k}"] = (r64[k] - v.astype(np.float64)).astype(np.float32)
    if g32:
        names = list(g32)
        errs = [_err(g32[n], g64[n]) for n in names]
        out[f"{pre}/g_names"] = np.array(names)
        out[f"{pre}/g_flat"] = np.concatenate([g32[n].reshape(-1) for n in names])
        out[f"{pre}/g_err_abs"] = np.array([e[0] for e in errs])
        out[f"{pre}/g_err_rel"] = np.array([e[1] for e in errs])


def gen_flow(out, K, L, top, grads):
    import torch
    from nf.cglow.CGlowModel import CondGlowModel
    seed = 100 * K + 10 * L + int(top)
    g = torch.Generator().manual_seed(7100 + seed)
    torch.manual_seed(7200 + seed)
    m = CondGlowModel(make_args(flow_depth=K, num_levels=L, learn_top=top))
    perturb(m, 0.1, g)
    if not top:
        _zero_top(m)
    M = 37
    x = torch.randn(M, 3, 8, 8, generator=g)
    y = torch.randn(M, 3, 8, 8, generator=g)
    g_z = torch.randn((M,) + tuple(m.new_mean.shape[1:]), generator=g)
    g_nll = torch.randn(M, generator=g)
    pre = f"k{K}l{L}t{int(top)}"
    out.update({f"{pre}/w/{k}": v for k, v in sd_np(m).items()})
    out.update({f"{pre}/x": x.numpy(), f"{pre}/y": y.numpy()})
    if grads:
        out.update({f"{pre}/g_z": g_z.numpy(), f"{pre}/g_nll": g_nll.numpy()})

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
    _record(out, pre, r32, r64, g32, g64)
    print(pre, "params", sum(p.numel() for p in m.parameters()), "nll", float(r32["nll"].mean()), "err nll",
          float(out[f"{pre}/err_abs/nll"]), "err z", float(out[f"{pre}/err_abs/z"]), "param grads", len(g32))


def gen_meas(out):
    import torch
    from DPFs import DPF
    g = torch.Generator().manual_seed(8100)
    torch.manual_seed(8200)
    B, N = 3, 21
    dpf = DPF(make_args(measurement="CGLOW", hiddensize=192, num_particles=N, batchsize=B, flow_depth=1,
                        num_levels=2, learn_top=True))
    perturb(dpf.particle_encoder, 0.3, g)
    perturb(dpf.cglow_measurement, 0.1, g)
    enc = torch.randn(B, 192, generator=g)
    x = torch.randn(B, N, 2, generator=g) * 30
    gl = torch.randn(B, N, generator=g)
    pre = "meas"
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
    for K, L, top, grads in ((1, 2, False, False), (2, 2, True, False), (1, 1, True, True)):
        gen_flow(out, K, L, top, grads)
    path = os.path.join(OUT, "cglow_levels.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    out = {}
    gen_flow(out, 1, 2, True, True)
    gen_meas(out)
    path = os.path.join(OUT, "cglow_levels_top.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
