"""Timings by frame-encoding width (--hiddensize), one JSON line each:

  1. one nfdpf_measurement launch (ops.measurement) per kind (cos, CRNVP, NN, gaussian) at
     E = 16, 32, 64 on the C3 shape (B = 64 rows of N = 1000 particles), hipEvents around the
     launch (nfdpf.prof.EventPair): median / min / max ms of REPS launches after WARM;
  2. FilterEngine passes on the C2 shape (NF_dyn + NF_cond, cos, soft; B 64, N 1000, T 50) and the
     C3 shape (no flows, CRNVP, OT; same sizes) at E = 64 -- the external-measurement step path --
     and at E = 32 with the one-launch pass turned off (the step launches): particle-steps/s from
     the wall time of synchronised passes.

    python scripts/meas_width_time.py [kernel|engine ...]   (default: both)
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "normalizing-flows-dpfs_amd"), ROOT]
import torch  # noqa: E402

B, N, T, WARM, REPS = 64, 1000, 50, 5, 30


class Mods(torch.nn.Module):
    def __init__(self, H, g):
        super().__init__()
        from model.models import build_conditional_nf, build_likelihood, build_particle_encoder
        self.nf_dyn = build_conditional_nf(2, 4, 2)
        self.cond_model = build_conditional_nf(2, 4 + H, 2)
        self.particle_encoder = build_particle_encoder(H, 2)
        self.cnf_measurement = build_conditional_nf(2, H, H, prior_std=2.5)
        self.likelihood_est = build_likelihood(H, 2)
        with torch.no_grad():  # trained-like scales
            for p in self.particle_encoder.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            for p in self.cnf_measurement.flows.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            for p in self.likelihood_est.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)


def time_kernels(dev):
    from nfdpf import ops
    from nfdpf.pack import encoder_tensors, flows_tensors, paired_mlp_tensors
    from nfdpf.prof import EventPair
    cat = lambda ts: torch.cat([a.detach().reshape(-1).float() for a in ts]).to(dev)  # noqa: E731
    for E in (16, 32, 64):
        g = torch.Generator().manual_seed(E)
        m = Mods(E, g)
        enc = torch.randn(B, E, generator=g).to(dev)
        x = (torch.randn(B, N, 2, generator=g) * 30).to(dev)
        pe = cat(encoder_tensors(m.particle_encoder))
        blobs = {"cos": None, "gaussian": None, "CRNVP": cat(flows_tensors(m.cnf_measurement.flows)),
                 "NN": cat(paired_mlp_tensors(m.likelihood_est))}
        out = torch.empty(B, N, device=dev)
        for kind in ("cos", "CRNVP", "NN", "gaussian"):
            for _ in range(WARM):
                ops.measurement(kind, pe, blobs[kind], 2, enc, x, 2.5, out=out)
            ms = []
            for _ in range(REPS):
                ev = EventPair()
                ev.record_start(dev)
                ops.measurement(kind, pe, blobs[kind], 2, enc, x, 2.5, out=out)
                ev.record_end(dev)
                ms.append(ev.ms())
                ev.close()
            assert bool(torch.isfinite(out).all())
            print(json.dumps({"what": "nfdpf_measurement", "kind": kind, "E": E, "B": B, "N": N,
                              "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
                              "reps": REPS}), flush=True)


def time_engine(dev):
    import warnings
    from nfdpf.engine import FilterConfig, FilterEngine
    shapes = {"c2": dict(NF_dyn=True, NF_cond=True, measurement="cos", resampler="soft"),
              "c3": dict(NF_dyn=False, NF_cond=False, measurement="CRNVP", resampler="ot")}
    for name, flags in shapes.items():
        for E in (32, 64):
            g = torch.Generator().manual_seed(10 + E)
            m = Mods(E, g).to(dev)
            enc = torch.randn(B, T, E, generator=g).to(dev)
            start = (torch.randn(B, 4, generator=g) * 10).to(dev)
            vel = (torch.randn(B, T, 2, generator=g) * 3).to(dev)
            eng = FilterEngine(FilterConfig(N=N, seed=7, **flags), m)
            eng.pass_disabled = E == 32  # E = 32: the step launches, the figure to put next to E = 64
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                for _ in range(2):
                    eng.run(enc, start, vel)
                torch.cuda.synchronize()
                secs = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    eng.run(enc, start, vel)
                    torch.cuda.synchronize()
                    secs.append(time.perf_counter() - t0)
            s = statistics.median(secs)
            print(json.dumps({"what": "engine_pass", "shape": name, "E": E, "B": B, "N": N, "T": T,
                              "path": "external measurement steps" if E != 32 else "step launches",
                              "one_launch_pass": bool(eng.last_pass), "s_median": s, "s_min": min(secs),
                              "particle_steps_per_s": B * N * T / s}), flush=True)


if __name__ == "__main__":
    from nfdpf import _lib
    _lib.load()
    what = sys.argv[1:] or ["kernel", "engine"]
    d = torch.device("cuda:0")
    if "kernel" in what:
        time_kernels(d)
    if "engine" in what:
        time_engine(d)
