"""Time of one CGLOW measurement launch at the C5 shape (B = 64 rows of N = 10 000 particles),
hipEvents around the launch (nfdpf.prof.EventPair), for the single-level kernel
(ops.cglow_measurement, csrc/cglow.hip) at K = 1, 2 and the levels kernel
(ops.cglow_levels_measurement, csrc/cglow_levels.hip) at (K, L, learn_top) = (1, 1, on),
(1, 2, on), (2, 2, on).  The lines are alternated: after a warm-up of every line, each round times
one launch of each, so drift of the device's clocks falls on all of them alike.  Prints one JSON
line per configuration: the median, min and max of the timed launches in ms.

    python scripts/cglow_levels_time.py [REPS]   (default 50)
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "normalizing-flows-dpfs_amd"), ROOT]
import torch  # noqa: E402

B, N, WARM = 64, 10000, 3


def main():
    from arguments import parse_args
    from model.models import build_particle_encoder_cglow
    from nf.cglow.CGlowModel import CondGlowModel
    from nfdpf import _lib, ops
    from nfdpf.pack import cglow_levels_tensors, cglow_tensors, encoder_tensors
    from nfdpf.prof import EventPair
    _lib.load()
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    enc = torch.randn(B, 192, generator=g).to(dev)
    x = (torch.randn(B, N, 2, generator=g) * 30).to(dev)
    torch.manual_seed(2)
    pe = torch.cat([t.detach().reshape(-1) for t in encoder_tensors(build_particle_encoder_cglow(192, 2))]).to(dev)
    out = torch.empty(B, N, device=dev)

    def model(K, L, top):
        a = parse_args([])
        a.flow_depth, a.num_levels, a.learn_top = K, L, top
        m = CondGlowModel(a)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        return m

    lines = []
    for K in (1, 2):
        glow = torch.cat([t.detach().reshape(-1) for t in cglow_tensors(model(K, 1, False))]).to(dev)
        lines.append((dict(what="cglow_measurement", K=K, L=1, learn_top=False),
                      lambda glow=glow, K=K: ops.cglow_measurement(pe, glow, enc, x, K=K, out=out)))
    for K, L, top in ((1, 1, True), (1, 2, True), (2, 2, True)):
        glow = torch.cat([t.detach().reshape(-1) for t in cglow_levels_tensors(model(K, L, top))]).to(dev)
        lines.append((dict(what="cglow_levels_measurement", K=K, L=L, learn_top=top),
                      lambda glow=glow, K=K, L=L, top=top: ops.cglow_levels_measurement(pe, glow, enc, x, K=K, L=L,
                                                                                         learn_top=top, out=out)))
    for _ in range(WARM):
        for _, run in lines:
            run()
    ms = [[] for _ in lines]
    for _ in range(reps):
        for i, (_, run) in enumerate(lines):
            ev = EventPair()
            ev.record_start(dev)
            run()
            ev.record_end(dev)
            ms[i].append(ev.ms())
            ev.close()
    assert bool(torch.isfinite(out).all())
    for (tag, _), v in zip(lines, ms):
        print(json.dumps(dict(tag, B=B, N=N, ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v), reps=reps)),
              flush=True)


if __name__ == "__main__":
    main()
