"""Generate the measurement fixtures at --hiddensize 16 and 64 by RUNNING THE REFERENCE (build
container only, like gen_golden.py, whose helpers this uses).

    python tests/golden/gen_meas_widths.py       # writes tests/golden/meas_widths.npz

For each width H in (16, 64) and each of cos / CRNVP / NN / gaussian: the reference's
DPF(args).measurement_model on B = 3 frame encodings [B, H] and N = 40 particles [B, N, 2], at
trained-like weight scales (particle encoder N(0, 0.5^2), CRNVP flows N(0, 0.1^2), likelihood_est
N(0, 0.02^2) -- wider, its sigmoid saturates and most log-likelihoods are exactly 0; at init the
likelihood is flat and hides errors).  Stored under "<meas>_<H>/": enc,
x, lik and the state dict of the measurement's sub-modules (w/...).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, import_reference, make_args, perturb, sd_np  # noqa: E402

WIDTHS = (16, 64)
KINDS = ("cos", "CRNVP", "NN", "gaussian")


def main():
    import_reference()
    import torch
    from DPFs import DPF
    out = {}
    g = torch.Generator().manual_seed(1664)
    B, N = 3, 40
    for H in WIDTHS:
        for meas in KINDS:
            torch.manual_seed(400 + H)
            dpf = DPF(make_args(measurement=meas, hiddensize=H, num_particles=N, batchsize=B))
            perturb(dpf.particle_encoder, 0.5, g)
            if meas == "CRNVP":
                perturb(dpf.cnf_measurement.flows, 0.1, g)
            if meas == "NN":
                perturb(dpf.likelihood_est, 0.02, g)
            enc = torch.randn(B, H, generator=g)
            x = torch.randn(B, N, 2, generator=g) * 30
            with torch.no_grad():
                lik = dpf.measurement_model(enc, x)
            k = f"{meas}_{H}"
            for kk, v in sd_np(dpf).items():
                if kk.split(".")[0] in ("particle_encoder", "cnf_measurement", "likelihood_est"):
                    out[f"{k}/w/{kk}"] = v
            out[f"{k}/enc"], out[f"{k}/x"], out[f"{k}/lik"] = enc.numpy(), x.numpy(), lik.numpy()
    np.savez_compressed(os.path.join(OUT, "meas_widths.npz"), **out)


if __name__ == "__main__":
    main()
