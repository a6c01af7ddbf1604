"""Time of one CGLOW measurement launch at the C5 shape (B = 64 rows of N = 10 000 particles),
hipEvents around the launch (nfdpf.prof.EventPair), for the width-general kernel
(ops.cglow_wide_measurement, csrc/cglow_wide.hip) at the fixtures' configurations a, b, c
(tests/golden/gen_cglow_widths.py) and at the default hidden sizes with y_bins = 32, next to the
levels kernel (ops.cglow_levels_measurement) at the same (K, L, learn_top) = (1, 2, on) and
default sizes -- that pair is the price of the general mapping -- and the single-level kernel
(ops.cglow_measurement) at K = 1 for scale.  The lines are alternated: after a warm-up of every
line, each round times one launch of each, so drift of the device's clocks falls on all of them
alike.  Prints one JSON line per configuration: the median, min and max of the timed launches
in ms.

    python scripts/cglow_widths_time.py [REPS]   (default 50)
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "normalizing-flows-dpfs_amd"), ROOT]
import torch  # noqa: E402

B, N, WARM = 64, 10000, 3
DEFAULT = (8, 16, 8)


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

    def model(widths, K, L, top):
        a = parse_args([])
        a.x_hidden_channels, a.x_hidden_size, a.y_hidden_channels = widths
        a.flow_depth, a.num_levels, a.learn_top = K, L, top
        m = CondGlowModel(a)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        return m

    def blob(tensors):
        return torch.cat([t.detach().reshape(-1) for t in tensors]).to(dev)

    lines = []
    for widths, K, L, top, bins in (((16, 32, 16), 1, 1, False, 256), ((8, 16, 32), 2, 2, True, 256),
                                    ((16, 32, 32), 1, 2, True, 256), (DEFAULT, 1, 2, True, 32)):
        glow = blob(cglow_levels_tensors(model(widths, K, L, top)))
        lines.append((dict(what="cglow_wide_measurement", widths=list(widths), K=K, L=L, learn_top=top, y_bins=bins),
                      lambda glow=glow, widths=widths, K=K, L=L, top=top, bins=bins: ops.cglow_wide_measurement(
                          pe, glow, enc, x, K=K, L=L, learn_top=top, widths=widths, y_bins=bins, out=out)))
    glow = blob(cglow_levels_tensors(model(DEFAULT, 1, 2, True)))
    lines.append((dict(what="cglow_levels_measurement", widths=list(DEFAULT), K=1, L=2, learn_top=True, y_bins=256),
                  lambda glow=glow: ops.cglow_levels_measurement(pe, glow, enc, x, K=1, L=2, learn_top=True, out=out)))
    glow = blob(cglow_tensors(model(DEFAULT, 1, 1, False)))
    lines.append((dict(what="cglow_measurement", widths=list(DEFAULT), K=1, L=1, learn_top=False, y_bins=256),
                  lambda glow=glow: ops.cglow_measurement(pe, glow, enc, x, K=1, out=out)))
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
