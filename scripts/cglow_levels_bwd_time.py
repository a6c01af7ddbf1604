"""Time of the CGLOW measurement's backward (measurement_model_cglow under autograd: the time
of ``backward()`` alone, hipEvents around it, nfdpf.prof.EventPair) for the configurations of
csrc/cglow_levels_bwd.hip, (K, L, learn_top) = (1, 1, on), (1, 2, on), (2, 2, on).

    python scripts/cglow_levels_bwd_time.py cap [REPS]   (default 10)
        4 x 4 096 particles, the PyTorch recompute's cap and so the largest size at which both
        paths run: every configuration with the HIP backward and with the recompute
        (nfdpf.autograd.HIP_BACKWARD off: the parent's path).
    python scripts/cglow_levels_bwd_time.py c5 [REPS]    (default 5)
        the C5 shape, 64 x 10 000 particles, HIP only, next to the single-level backward
        (csrc/cglow_bwd.hip, K = 1, L = 1, learn_top off).

The lines are alternated: after a warm-up of every line, each round times one backward of each, so
drift of the device's clocks falls on all of them alike.  Prints one JSON line per line: the
median, min and max of the timed backwards in ms, and the workspace the C ABI asks for."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "normalizing-flows-dpfs_amd"), ROOT]
import torch  # noqa: E402

WARM = 2


def main():
    from arguments import parse_args
    from model.models import build_particle_encoder_cglow, measurement_model_cglow
    from nf.cglow.CGlowModel import CondGlowModel
    from nfdpf import _lib, autograd
    from nfdpf.prof import EventPair
    lib = _lib.load()
    shape = sys.argv[1] if len(sys.argv) > 1 else "cap"
    B, N = (4, 4096) if shape == "cap" else (64, 10000)
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else (10 if shape == "cap" else 5)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    enc = torch.randn(B, 192, generator=g).to(dev)
    x = (torch.randn(B, N, 2, generator=g) * 30).to(dev).requires_grad_(True)
    gl = torch.randn(B, N, generator=g).to(dev)

    def model(K, L, top):
        a = parse_args([])
        a.flow_depth, a.num_levels, a.learn_top = K, L, top
        torch.manual_seed(2)
        m = measurement_model_cglow(build_particle_encoder_cglow(192, 2), CondGlowModel(a))
        with torch.no_grad():
            for p in m.CGLOW.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        return m.to(dev)

    def backward(m, hip):
        """One forward (not timed) and one timed backward; -> ms."""
        autograd.HIP_BACKWARD = hip
        try:
            for p in m.parameters():
                p.grad = None
            x.grad = None
            loss = (m(enc, x) * gl).sum()
            ev = EventPair()
            ev.record_start(dev)
            loss.backward()
            ev.record_end(dev)
            ms = ev.ms()
            ev.close()
        finally:
            autograd.HIP_BACKWARD = True
        assert bool(torch.isfinite(x.grad).all())
        return ms

    lines = []
    if shape != "cap":
        m = model(1, 1, False)
        ws = int(lib.nfdpf_cglow_backward_workspace_k(B * N, 1))
        lines.append((dict(what="cglow_measurement backward", K=1, L=1, learn_top=False, path="hip", workspace_bytes=ws),
                      lambda m=m: backward(m, True)))
    for K, L, top in ((1, 1, True), (1, 2, True), (2, 2, True)):
        m = model(K, L, top)
        ws = int(lib.nfdpf_cglow_levels_backward_workspace(B * N, K, L))
        for hip in ((True, False) if shape == "cap" else (True,)):
            lines.append((dict(what="cglow_levels_measurement backward", K=K, L=L, learn_top=top,
                               path="hip" if hip else "recompute", workspace_bytes=ws if hip else 0),
                          lambda m=m, hip=hip: backward(m, hip)))
    for _ in range(WARM):
        for _, run in lines:
            run()
    ms = [[] for _ in lines]
    for _ in range(reps):
        for i, (_, run) in enumerate(lines):
            ms[i].append(run())
    for (tag, _), v in zip(lines, ms):
        print(json.dumps(dict(tag, B=B, N=N, ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v), reps=reps)),
              flush=True)


if __name__ == "__main__":
    main()
