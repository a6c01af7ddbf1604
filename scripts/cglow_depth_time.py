"""Time of one CGLOW measurement launch (ops.cglow_measurement, csrc/cglow.hip) at the C5 shape
(B = 64 rows of N = 10 000 particles) by flow depth K, hipEvents around the launch
(nfdpf.prof.EventPair).  Prints one JSON line per K: the median, min and max of the timed
launches in ms.  Expectation: time ~ encoder + K x step.

    python scripts/cglow_depth_time.py [K ...]   (default 1 2 4)
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "normalizing-flows-dpfs_amd"), ROOT]
import torch  # noqa: E402

B, N, WARM, REPS = 64, 10000, 5, 20


def main():
    from arguments import parse_args
    from model.models import build_particle_encoder_cglow
    from nf.cglow.CGlowModel import CondGlowModel
    from nfdpf import _lib, ops
    from nfdpf.pack import cglow_tensors, encoder_tensors
    from nfdpf.prof import EventPair
    _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    enc = torch.randn(B, 192, generator=g).to(dev)
    x = (torch.randn(B, N, 2, generator=g) * 30).to(dev)
    torch.manual_seed(2)
    pe = torch.cat([t.detach().reshape(-1) for t in encoder_tensors(build_particle_encoder_cglow(192, 2))]).to(dev)
    for K in [int(a) for a in sys.argv[1:]] or [1, 2, 4]:
        a = parse_args([])
        a.flow_depth = K
        m = CondGlowModel(a)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        glow = torch.cat([t.detach().reshape(-1) for t in cglow_tensors(m)]).to(dev)
        out = torch.empty(B, N, device=dev)
        for _ in range(WARM):
            ops.cglow_measurement(pe, glow, enc, x, K=K, out=out)
        ms = []
        for _ in range(REPS):
            ev = EventPair()
            ev.record_start(dev)
            ops.cglow_measurement(pe, glow, enc, x, K=K, out=out)
            ev.record_end(dev)
            ms.append(ev.ms())
            ev.close()
        assert bool(torch.isfinite(out).all())
        print(json.dumps({"what": "cglow_measurement", "B": B, "N": N, "K": K, "ms_median": statistics.median(ms),
                          "ms_min": min(ms), "ms_max": max(ms), "reps": REPS}), flush=True)


if __name__ == "__main__":
    main()
