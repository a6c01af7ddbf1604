"""Parity of the HIP path (through the C ABI) against the reference's golden vectors and
the CPU oracle.  GPU box only.

Tolerances: indices bit-exact; log-dets / weights |d| <= 1e-5 |ref| + atol
with atol 1e-6 (D = 2) and 5e-6 (D = 32 with std-0.3 weights) -- pure relative error is
meaningless on near-zero log-dets (the reference's own fp32-vs-fp64 gap is ~1e-2 relative
there).
"""
import numpy as np
import pytest
import torch

from _util import assert_close, e2e_cfg, group, load, t, TapeRNG, weights
from oracle import dpf_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _flow_blob(w, n_flows):
    """Coupling nets in the kernel layout (include/nfdpf.h), from a state dict: per coupling
    half the {t, s} pairs of [W1[:, :half], W2, b2, W3, b3, W1[:, half:], b1]."""
    from nfdpf.pack import pair
    parts = []
    for i in range(n_flows):
        pre = "" if n_flows == 1 else f"flows.{i}."
        for tn, sn in (("t1", "s1"), ("t2", "s2")):
            g = lambda net, layer, k: w[f"{pre}{net}.network.{layer}.{k}"]  # noqa: E731
            half = g(tn, 4, "weight").shape[0]
            tw1, sw1 = g(tn, 0, "weight"), g(sn, 0, "weight")
            parts += [pair(tw1[:, :half], sw1[:, :half])]
            parts += [pair(g(tn, layer, k), g(sn, layer, k)) for layer, k in
                      ((2, "weight"), (2, "bias"), (4, "weight"), (4, "bias"))]
            parts += [pair(tw1[:, half:], sw1[:, half:]), pair(g(tn, 0, "bias"), g(sn, 0, "bias"))]
    return torch.cat([p.reshape(-1) for p in parts]).to(DEV)


def _maf_blob(w, n_flows, D):
    parts = []
    for i in range(n_flows):
        parts.append(w[f"flows.{i}.initial_param"])
        for j in range(D - 1):
            for layer in (0, 2, 4):
                parts += [w[f"flows.{i}.layers.{j}.network.{layer}.weight"],
                          w[f"flows.{i}.layers.{j}.network.{layer}.bias"]]
    return torch.cat([p.reshape(-1) for p in parts]).to(DEV)


def _enc_blob(w, prefix="particle_encoder"):
    """Particle encoder in the kernel layout (W1 row_pairs, W2 / W3 col_pairs)."""
    from nfdpf.pack import col_pairs, row_pairs
    W = [w[f"{prefix}.{layer}.weight"] for layer in (0, 2, 4)]
    b = [w[f"{prefix}.{layer}.bias"] for layer in (0, 2, 4)]
    parts = [row_pairs(W[0]), b[0], col_pairs(W[1]), b[1], col_pairs(W[2]), b[2]]
    return torch.cat([p.reshape(-1) for p in parts]).to(DEV)


def _mlp_blob(w, prefix):
    """Particle encoder / likelihood_est in the kernel layout: weights with an even number of
    outputs in row_pairs order, biases plain."""
    from nfdpf.pack import row_pairs
    parts = []
    for layer in (0, 2, 4):
        W = w[f"{prefix}.{layer}.weight"]
        parts += [row_pairs(W) if W.shape[0] % 2 == 0 else W, w[f"{prefix}.{layer}.bias"]]
    return torch.cat([p.reshape(-1) for p in parts]).to(DEV)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from nfdpf import _lib
    _lib.load()
    assert torch.cuda.is_available()


@pytest.mark.parametrize("D,O_", [(2, 4), (2, 36), (2, 196), (32, 32)])
@pytest.mark.parametrize("tag", ["init", "wide"])
def test_realnvp_cond_golden(D, O_, tag):
    from nfdpf import ops
    fx = group(load("flows.npz"), f"D{D}_O{O_}_{tag}")
    w = weights(fx)
    b = _flow_blob(w, 1)
    atol = 5e-6 if D == 32 else 1e-6
    x, c = t(fx["x"]).to(DEV), t(fx["c"]).to(DEV)
    z, ld, _ = ops.cond_stack(b, 1, D, O_, 8, x, c, 1, False)
    assert_close(ld.cpu(), fx["ld_fwd"], 1e-5, atol, "logdet fwd")
    assert_close(z.cpu(), fx["z"], 1e-5, 1e-5, "z")
    xi, ldi, _ = ops.cond_stack(b, 1, D, O_, 8, x, c, 1, True)
    assert_close(ldi.cpu(), fx["ld_inv"], 1e-5, atol, "logdet inv")
    assert_close(xi.cpu(), fx["xinv"], 1e-5, 1e-5, "x inv")


@pytest.mark.parametrize("case,D,O_", [("cond_D2_O4", 2, 4), ("cond_D2_O36", 2, 36), ("cond_D32_O32", 32, 32)])
def test_cond_stack_golden(case, D, O_):
    from nfdpf import ops
    fx = group(load("stacks.npz"), case)
    w = weights(fx)
    b = _flow_blob(w, 2)
    x, c = t(fx["x"]).to(DEV), t(fx["c"]).to(DEV)
    atol = 5e-6 if D == 32 else 1e-6
    z, ld, lp = ops.cond_stack(b, 2, D, O_, 8, x, c, 1, False, 0.0, float(fx["prior_std"]), want_prior=True)
    assert_close(ld.cpu(), fx["ld_fwd"], 1e-5, atol, "logdet")
    assert_close(z.cpu(), fx["z"], 1e-5, 1e-5, "z")
    assert_close(lp.cpu(), fx["lp"], 1e-5, 1e-5, "prior log-prob")
    xi, ldi, _ = ops.cond_stack(b, 2, D, O_, 8, x, c, 1, True)
    assert_close(ldi.cpu(), fx["ld_inv"], 1e-5, atol, "logdet inv")
    assert_close(xi.cpu(), fx["xinv"], 1e-5, 1e-5, "x inv")


def test_cond_stack_broadcast_context_matches_per_row():
    """cond_group = N (per-batch context, never materialised) == the per-row expansion."""
    from nfdpf import ops
    fx = group(load("stacks.npz"), "cond_D2_O36")
    b = _flow_blob(weights(fx), 2)
    B, N = 6, 333
    x = torch.randn(B * N, 2, device=DEV) * 10
    c = torch.randn(B, 36, device=DEV)
    z1, l1, _ = ops.cond_stack(b, 2, 2, 36, 8, x, c, N, True)
    z2, l2, _ = ops.cond_stack(b, 2, 2, 36, 8, x, c.repeat_interleave(N, 0), 1, True)
    assert torch.equal(z1, z2) and torch.equal(l1, l2)


@pytest.mark.parametrize("D", [2, 4])
def test_maf_golden(D):
    from nfdpf import ops
    fx = group(load("stacks.npz"), f"maf_D{D}")
    b = _maf_blob(weights(fx), 2, D)
    x = t(fx["x"]).to(DEV)
    z, ld = ops.maf_stack(b, 2, D, 8, x, False)
    assert_close(z.cpu(), fx["z"], 1e-5, 1e-5, "z")
    assert_close(ld.cpu(), fx["ld_fwd"], 1e-5, 1e-6, "logdet")
    xi, ldi = ops.maf_stack(b, 2, D, 8, x, True)
    assert_close(xi.cpu(), fx["xinv"], 1e-5, 1e-5, "x inv")
    assert_close(ldi.cpu(), fx["ld_inv"], 1e-5, 1e-6, "logdet inv")


def test_soft_resampler_bit_exact_golden():
    from nfdpf import ops
    fx = load("soft.npz")
    for i in range(int(fx["n_cases"])):
        c = group(fx, f"c{i}")
        x, p = t(c["x"]), t(c["p"])
        xo, wo, idx = ops.soft_resample(x.to(DEV), p.to(DEV), float(c["alpha"]), t(c["offsets"]).to(DEV))
        np.testing.assert_array_equal(idx.cpu().numpy(), c["idx"].astype(np.int64), err_msg=f"case {i}")
        np.testing.assert_array_equal(wo.cpu().numpy(), c["w"], err_msg=f"case {i} weights")
        B, N = p.shape
        np.testing.assert_array_equal(xo.cpu().numpy(), x.reshape(B * N, 2)[idx.cpu()].numpy())


def test_soft_resampler_bit_exact_random_vs_oracle():
    """Larger random sweep (incl. N = 10000) against the oracle's dense O(N^2) matching."""
    from nfdpf import ops
    g = torch.Generator().manual_seed(5)
    # (2, 16000): above the LDS-staged kernel's N <= 13 312 (csrc/resample_soft.hip): the
    # global-memory variant
    for B, N, scale in ((64, 1000, 3.0), (4, 10000, 5.0), (16, 100, 30.0), (8, 4000, 1.0), (2, 16000, 2.0)):
        p = torch.softmax(torch.randn(B, N, generator=g) * scale, -1) + 1e-12
        x = torch.randn(B, N, 2, generator=g)
        off = torch.empty(B).uniform_(0, 1.0 / N, generator=g)
        _, wo, idx = ops.soft_resample(x.to(DEV), p.to(DEV), 0.5, off.to(DEV))
        _, wr, idr = O.soft_resample(x, p, 0.5, off)
        assert torch.equal(idx.cpu(), idr.long()), (B, N)
        assert torch.equal(wo.cpu(), wr), (B, N)


def test_ot_resampler_golden():
    from nfdpf import ops
    fx = load("ot.npz")
    for i in range(int(fx["n_cases"])):
        c = group(fx, f"c{i}")
        xo, wo, idx, it = ops.ot_resample(t(c["x"]).to(DEV), t(c["p"]).to(DEV))
        assert int(it.item()) == int(c["iters"]), f"case {i}: iterations {int(it.item())} vs {int(c['iters'])}"
        # fp32 Sinkhorn vs the reference's fp64: positions ~1e2, agree to ~1e-3 absolute
        assert_close(xo.cpu(), c["xr"], 1e-4, 2e-3, f"OT x' case {i}")
        np.testing.assert_array_equal(wo.cpu().numpy(), c["wr"])
        B, N = c["p"].shape
        np.testing.assert_array_equal(idx.cpu().numpy(), np.arange(B * N).reshape(B, N))


@pytest.mark.parametrize("B,N,kind", [(2, 1000, "peaked"), (3, 777, "outliers"), (2, 1500, "uniform"),
                                      (4, 64, "peaked"), (1, 300, "clusters")])
def test_ot_resampler_vs_oracle_stress(B, N, kind):
    """Sliced kernel sums (csrc/resample_ot.hip) against the reference's fp64 Sinkhorn
    restated by the oracle: concentrated weights (every sum of a lane underflows against the
    slice shifts at small epsilon unless the exact fallback takes over), isolated outliers,
    well separated clusters, ragged N (partial table slices).  Same bar as the golden cases:
    iteration count equal, x' within 1e-4 rel + 2e-3 abs of the fp64 result (positions ~1e2)."""
    from nfdpf import ops
    g = torch.Generator().manual_seed(N + B)
    x = torch.randn(B, N, 2, generator=g) * 30
    if kind == "outliers":
        x[:, :5] *= 40
    if kind == "clusters":
        x[:, : N // 2] += 400
    s = {"peaked": 12.0, "outliers": 3.0, "uniform": 0.0, "clusters": 2.0}[kind]
    p = torch.softmax(torch.randn(B, N, generator=g) * s, -1) + 1e-12
    xo, wo, idx, it = ops.ot_resample(x.to(DEV), p.to(DEV))
    xr, wr, _, info = O.ot_resample(x.double(), p.double(), return_info=True)
    assert int(it.item()) == int(info["iters"]), (int(it.item()), int(info["iters"]))
    assert_close(xo.cpu(), xr, 1e-4, 2e-3, f"OT x' {kind} B={B} N={N}")
    assert torch.all(wo.cpu() == 1.0 / N)


@pytest.mark.parametrize("B,N,kind", [(64, 1000, "peaked"), (3, 777, "outliers"), (8, 1500, "clusters")])
def test_ot_iter_waves_bit_identical(B, N, kind, monkeypatch):
    """The 8-wave Sinkhorn iteration launch (small grids; waves w and w + 4 split the lanes' i
    over the same slices, csrc/resample_ot.hip wg_iter_sums) returns the 4-wave launch's result
    bit for bit, iteration count included, on a C3-shaped batch (64 rows x N=1000) and ragged N."""
    from nfdpf import ops
    g = torch.Generator().manual_seed(7 * N + B)
    x = torch.randn(B, N, 2, generator=g) * 30
    if kind == "outliers":
        x[:, :5] *= 40
    if kind == "clusters":
        x[:, : N // 2] += 400
    s = {"peaked": 12.0, "outliers": 3.0, "clusters": 2.0}[kind]
    p = torch.softmax(torch.randn(B, N, generator=g) * s, -1) + 1e-12
    out = {}
    for w in ("4", "8"):
        monkeypatch.setenv("NFDPF_OT_ITER_WAVES", w)
        out[w] = [u.cpu() for u in ops.ot_resample(x.to(DEV), p.to(DEV))]
    for u, v in zip(out["4"], out["8"]):
        assert torch.equal(u, v)


def test_ot_strided_rows_match_contiguous():
    """One step of a [B, T, N, 2] history read in place (nfdpf_ot_resample_rs, the engine's OT
    input) gives the contiguous call's outputs bit for bit, gate on and off."""
    from nfdpf import ops
    g = torch.Generator().manual_seed(23)
    B, T, N = 6, 3, 777
    hx = (torch.randn(B, T, N, 2, generator=g) * 20).to(DEV)
    hp = torch.softmax(torch.randn(B, T, N, generator=g) * 3, -1).to(DEV)
    xs, ps = hx[:, 1], hp[:, 1]
    assert not xs.is_contiguous() and not ps.is_contiguous()
    a = ops.ot_resample(xs, ps, row_base=5)
    b = ops.ot_resample(xs.contiguous(), ps.contiguous(), row_base=5)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    off = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert int(ops.ot_resample(xs, ps, gate=off)[3].item()) == 0


def test_ot_poll_matches_enqueue_all():
    """poll=1 (host follows the loop and stops enqueueing) gives the bit-identical result of
    poll=0 (all max_iter - 1 launches enqueued, graph-capturable), gate on and off."""
    from nfdpf import ops
    c = group(load("ot.npz"), "c1")
    x, p = t(c["x"]).to(DEV), t(c["p"]).to(DEV)
    a = ops.ot_resample(x, p, poll=False)
    b = ops.ot_resample(x, p, poll=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    off = torch.zeros(1, dtype=torch.int32, device=DEV)
    z = ops.ot_resample(x, p, gate=off, poll=True)
    assert int(z[3].item()) == 0


def _ot_two_phase(parts, max_iter=100):
    """A batch split over 'ranks' the way ops.ot_resample_sharded runs it, the ranks simulated
    in turn: every part's local loop (private workspace + potential history), the MIN of the
    counts (the all-reduce), every part's tail at that state."""
    from nfdpf import ops
    st = []
    for xx, pp, rb in parts:
        B, N, _ = xx.shape
        ws, hist = ops.ot_workspace(B, N, DEV), ops.ot_history(B, N, max_iter, DEV)
        st.append((ws, hist, ops.ot_sinkhorn_local(xx, pp, 0.1, 0.75, 1e-3, max_iter, ws, hist)))
    local = [int(s_[2].item()) for s_ in st]
    stop = torch.tensor([min(local)], dtype=torch.int32, device=DEV)
    outs = [ops.ot_sinkhorn_finish(xx, 0.1, 0.75, 1e-3, max_iter, rb, ws, hist, stop)
            for (xx, pp, rb), (ws, hist, _) in zip(parts, st)]
    return outs, local, min(local)


@pytest.mark.parametrize("kind", ["fixture", "mixed"])
def test_ot_sharded_stop_matches_unsharded(kind):
    """A batch split over 'ranks' reproduces the unsharded Sinkhorn loop bit for bit
    (resamplers.py:126-129): each part runs its rows with the local
    stop rule keeping every state's potentials, the MIN of the counts is the batch-global stop,
    and each part finishes at that state -- no iteration runs twice.  'mixed' gives the parts
    clouds of different spread, so one part's own rule stops later than the global MIN and its
    tail must resume from the history (its tables were overwritten since); also the old
    two-pass form (rerun with stop_at) for comparison."""
    from nfdpf import ops
    if kind == "fixture":
        c = group(load("ot.npz"), "c1")
        x, p = t(c["x"]).to(DEV), t(c["p"]).to(DEV)
    else:
        g = torch.Generator().manual_seed(17)
        B, N = 6, 700
        spread = torch.tensor([1.0, 1.0, 1.0, 30.0, 60.0, 90.0])[:, None, None]
        x = (torch.randn(B, N, 2, generator=g) * spread).to(DEV)
        p = torch.softmax(torch.randn(B, N, generator=g) * 2, -1).to(DEV)
    B = x.shape[0]
    full, wfull, ifull, it_full = ops.ot_resample(x, p)
    h = B // 2
    parts = [(x[:h].contiguous(), p[:h].contiguous(), 0), (x[h:].contiguous(), p[h:].contiguous(), h)]
    outs, local, stop = _ot_two_phase(parts)
    assert stop == int(it_full.item()), (local, int(it_full.item()))
    assert torch.equal(torch.cat([outs[0][0], outs[1][0]]), full)
    assert torch.equal(torch.cat([outs[0][1], outs[1][1]]), wfull)
    assert torch.equal(torch.cat([outs[0][2], outs[1][2]]), ifull)
    if kind == "mixed":
        assert max(local) > stop, local  # a part resumed behind its own stop
    # the two-pass form (local run, rerun to the MIN) agrees
    its = [ops.ot_resample(xx, pp, row_base=rb)[3] for xx, pp, rb in parts]
    mn = torch.minimum(its[0], its[1])
    rerun = [ops.ot_resample(xx, pp, row_base=rb, stop_at=mn)[0] for xx, pp, rb in parts]
    assert torch.equal(torch.cat(rerun), full)


@pytest.mark.parametrize("meas", ["cos", "CRNVP", "NN", "gaussian"])
def test_measurement_golden(meas):
    from nfdpf import ops
    fx = group(load("meas.npz"), meas)
    w = weights(fx)
    pe = _enc_blob(w)
    mb = None
    if meas == "CRNVP":
        mb = _flow_blob({k[len("cnf_measurement."):]: v for k, v in w.items() if k.startswith("cnf_measurement.")}, 2)
    elif meas == "NN":
        mb = _mlp_blob(w, "likelihood_est")
    lik = ops.measurement(meas, pe, mb, 2, t(fx["enc"]).to(DEV), t(fx["x"]).to(DEV), 2.5)
    assert_close(lik.cpu(), fx["lik"], 1e-5, 2e-5, meas)


def _glow_module(w, prefix="cglow_measurement."):
    """CondGlowModel with the default arguments (K = 1, L = 1) holding the fixture weights."""
    from arguments import parse_args
    from nf.cglow.CGlowModel import CondGlowModel
    m = CondGlowModel(parse_args([]))
    sd = m.state_dict()
    sd.update({k[len(prefix):]: v for k, v in w.items() if k.startswith(prefix)})
    m.load_state_dict(sd)
    return m


def _oracle_cglow64(w, enc, x):
    """The oracle's CGLOW likelihood in float64 (row-max shifted)."""
    with O.precision(torch.float64):
        p = O.cast_params(w, torch.float64)
        return O.meas_cglow(O.sub(p, "particle_encoder"), O.sub(p, "cglow_measurement"), 1,
                            enc.double(), x.double()).numpy()


def test_cglow_measurement_golden():
    """measurement_model_cglow (model/models.py:280-303) on the reference's golden vectors:
    one HIP kernel (csrc/cglow.hip) vs the reference's float32 output, and both against the
    oracle in float64 (the reference's own float32 error is the yardstick)."""
    from nfdpf import ops
    from nfdpf.pack import cglow_tensors
    fx = group(load("meas.npz"), "CGLOW")
    w = weights(fx)
    pe = _enc_blob(w)
    glow = torch.cat([a.detach().reshape(-1) for a in cglow_tensors(_glow_module(w))]).to(DEV)
    enc, x = t(fx["enc"]), t(fx["x"])
    raw = ops.cglow_measurement(pe, glow, enc.to(DEV), x.to(DEV))
    lik = (raw - raw.max(dim=-1, keepdim=True)[0]).cpu().numpy()
    ref64 = _oracle_cglow64(w, enc, x)
    e_ours = np.abs(lik - ref64)
    e_ref = np.abs(fx["lik"] - ref64)
    print(f"CGLOW: max |ours - f64| {e_ours.max():.3e} mean {e_ours.mean():.3e}; "
          f"reference f32 max {e_ref.max():.3e} mean {e_ref.mean():.3e}")
    assert e_ours.max() <= 4 * e_ref.max() + 1e-5
    assert e_ours.mean() <= 2.5 * e_ref.mean() + 1e-6
    assert_close(lik, fx["lik"], 1e-5, 5e-5, "CGLOW lik")


def test_cglow_module_matches_kernel():
    """measurement_model_cglow.forward (the reference module API) runs the same kernel."""
    from model.models import build_particle_encoder_cglow, measurement_model_cglow
    fx = group(load("meas.npz"), "CGLOW")
    w = weights(fx)
    pe = build_particle_encoder_cglow(192, 2)
    pe.load_state_dict({k[len("particle_encoder."):]: v for k, v in w.items() if k.startswith("particle_encoder.")})
    m = measurement_model_cglow(pe, _glow_module(w)).to(DEV)
    lik = m(t(fx["enc"]).to(DEV), t(fx["x"]).to(DEV)).detach().cpu()
    assert_close(lik, fx["lik"], 1e-5, 5e-5, "CGLOW module")


class _Models(torch.nn.Module):
    """Minimal holder with the DPF attribute names the engine reads."""

    def __init__(self, w, cfg):
        super().__init__()
        from model.models import (build_conditional_nf, build_likelihood, build_maf_dyn, build_particle_encoder,
                                  build_particle_encoder_cglow)
        H = cfg.get("H", 32)
        self.nf_dyn = build_maf_dyn(2, 2) if cfg.get("dyn_flow") == "MAF" else build_conditional_nf(2, 4, 2)
        self.cond_model = build_conditional_nf(2, 4 + H, 2)
        if cfg["measurement"] == "CGLOW":
            self.particle_encoder = build_particle_encoder_cglow(H, 2)
            self.cglow_measurement = _glow_module(w)
        else:
            self.particle_encoder = build_particle_encoder(32, 2)
        if cfg["measurement"] == "CRNVP":
            self.cnf_measurement = build_conditional_nf(2, 32, 32, prior_std=2.5)
        if cfg["measurement"] == "NN":
            self.likelihood_est = build_likelihood(32, 2)
        sd = self.state_dict()
        sd.update({k: v for k, v in w.items() if k in sd})
        self.load_state_dict(sd)
        self.to(DEV)


KERNELS = ["fused", "tiled"]


def _engine(fx, kernel="tiled"):
    from nfdpf.engine import FilterConfig, FilterEngine
    c = e2e_cfg(fx)
    cfg = FilterConfig(N=c["N"], NF_dyn=c["NF_dyn"], NF_cond=c["NF_cond"], measurement=c["measurement"],
                       resampler=c["resampler"], rng_mode="host", kernel=kernel, dyn_flow=c["dyn_flow"])
    return FilterEngine(cfg, _Models(weights(fx), c)), c


class _TapeDraws:
    def __init__(self, fx):
        self.tape = TapeRNG(fx)

    def offsets(self, B, N):
        return self.tape.offsets(B, N)

    def noise(self, B, N, std):
        return self.tape.noise(B, N, std)


E2E_FUSED = ["c1", "c2", "c2w", "c3", "c3n", "c4", "c5"]


def _oracle64_one_step(fx, monkeypatch):
    """The reference's step t from its own step t-1 state, evaluated in float64 by the oracle
    (resampling indices taken in float32, i.e. the reference's own).  |ref64 - ref32| is the
    reference's rounding envelope for that step."""
    cfg = e2e_cfg(fx)
    T = int(fx["T"])
    soft32 = O.soft_resample

    def soft64(x, p, alpha, offsets=None, gen=None):
        with O.precision(torch.float32):
            _, _, idx = soft32(x.float(), p.float(), alpha, offsets.float())
        B, N = p.shape
        q = alpha * p + (1 - alpha) / N
        q = q / q.sum(-1, keepdim=True)
        w = (p / q).reshape(B * N)[idx]
        return x.reshape(B * N, -1)[idx], w / w.sum(-1, keepdim=True), idx

    monkeypatch.setattr(O, "soft_resample", soft64)
    out = {k: [] for k in ("x", "p", "lik", "jac", "prior")}
    with O.precision(torch.float64):
        w = O.cast_params(weights(fx), torch.float64)
        meas = O.make_measurement(cfg, w)
        rng = TapeRNG(fx)
        x, p = t(fx["init_x"]).double(), O.normalize_log_probs(t(fx["logw0"]).double())
        vel = t(fx["start"]).double()[:, 2:]
        for s in range(T):
            r = O.filter_step(cfg, w, meas, x, p, vel, t(fx["enc"]).double()[:, s], rng)
            for k in out:
                out[k].append(r[k])
            x, p = t(fx["x"][:, s]).double(), t(fx["p"][:, s]).double()
            vel = t(fx["vel"]).double()[:, s]
    return {k: torch.stack(v, 1).numpy() for k, v in out.items()}


def _check_envelope(ours, ref32, ref64, rtol, atol, what, k_max=4.0, k_mean=2.5, k_row=16.0):
    """Ours must be as accurate as the reference's own float32 run, both measured against the
    float64 evaluation of the same step (ref64):

      max  |ours - ref64| <= k_max  * max  |ref32 - ref64| + atol      (whole case)
      mean |ours - ref64| <= k_mean * mean |ref32 - ref64| + atol
      |ours - ref64| <= k_row * E_row + rtol |ref64| + atol             (every element)

    E_row = max over the N particles of |ref32 - ref64| on that (batch row, step): the
    particles of a row share its context and normalisation, so the row's rounding noise is
    one quantity; k_row covers rows where the reference's own error happens to be small
    (measured on MI355X over c1-c3n: worst row ratio 12.6, case max ratio 3.2 -- the cosine
    likelihood -log(1e-7 + 1 - cos) near cos = 1 --, case mean ratio 1.0-2.0 above atol)."""
    ours, ref32, ref64 = (np.asarray(a, dtype=np.float64) for a in (ours, ref32, ref64))
    e_ref = np.abs(ref32 - ref64)
    e_ours = np.abs(ours - ref64)
    assert e_ours.max() <= k_max * e_ref.max() + atol, \
        f"{what}: max err {e_ours.max():.3e} vs reference float32 {e_ref.max():.3e}"
    assert e_ours.mean() <= k_mean * e_ref.mean() + atol, \
        f"{what}: mean err {e_ours.mean():.3e} vs reference float32 {e_ref.mean():.3e}"
    env = e_ref.max(axis=2, keepdims=True) if e_ref.ndim >= 3 else e_ref
    bound = k_row * env + rtol * np.abs(ref64) + atol
    assert np.all(e_ours <= bound), f"{what}: worst excess {(e_ours - bound).max():.3e} (env {env.max():.3e})"
    return float(np.mean(e_ours <= rtol * np.abs(ref64) + atol))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", E2E_FUSED)
def test_filter_step_one_step_parity(name, kernel, monkeypatch):
    """Each fused step started from the reference's own previous state (teacher forcing).

    Exact: gate decisions, resampling indices, noise.  Floating point: within the
    reference's own float32 rounding envelope (|ref64 - ref32|, e.g. the cosine likelihood
    is -log(1 - <a,b>) and loses digits as particles align) plus 1e-5 relative."""
    fx = load(f"e2e_{name}.npz")
    eng, c = _engine(fx, kernel)
    res = eng.run(t(fx["enc"]).to(DEV), t(fx["start"]).to(DEV), t(fx["vel"]).to(DEV),
                  host=_TapeDraws(fx), init=(t(fx["init_x"]), t(fx["logw0"])),
                  teacher={"x": t(fx["x"]), "p": t(fx["p"])})
    assert res.fired == [bool(f) for f in fx["fired"]]
    np.testing.assert_array_equal(res.index.cpu().numpy(), fx["idx"].astype(np.int64))
    np.testing.assert_array_equal(res.noise.cpu().numpy(), fx["noise"])
    r64 = _oracle64_one_step(fx, monkeypatch)
    _check_envelope(res.particles.cpu(), fx["x"], r64["x"], 1e-5, 1e-4, "particles")
    _check_envelope(res.probs.cpu(), fx["p"], r64["p"], 1e-5, 1e-9, "weights")
    _check_envelope(res.lik.cpu(), fx["lik"], r64["lik"], 1e-5, 2e-5, "likelihood")
    if c["NF_dyn"]:
        _check_envelope(res.jac.cpu(), fx["jac"], r64["jac"], 1e-5, 1e-6, "jac")
        _check_envelope(res.prior.cpu(), fx["prior"], r64["prior"], 1e-5, 1e-5, "prior")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["c1", "c2", "c3", "c4", "c5"])
def test_filtering_free_running(name, kernel):
    """Whole sequences from the reference's initial state and draws."""
    fx = load(f"e2e_{name}.npz")
    eng, c = _engine(fx, kernel)
    res = eng.run(t(fx["enc"]).to(DEV), t(fx["start"]).to(DEV), t(fx["vel"]).to(DEV),
                  host=_TapeDraws(fx), init=(t(fx["init_x"]), t(fx["logw0"])))
    assert res.fired == [bool(f) for f in fx["fired"]]
    np.testing.assert_array_equal(res.index.cpu().numpy(), fx["idx"].astype(np.int64))
    assert_close(res.particles.cpu(), fx["x"], 1e-4, 1e-3, "particles")
    assert_close(res.probs.cpu(), fx["p"], 1e-4, 1e-7, "weights")
    assert abs(float(res.obs_likelihood) - float(fx["obs_lik"])) <= 1e-4 * abs(float(fx["obs_lik"])) + 1e-3
    rm, _ = O.rmse(res.particles.cpu(), res.probs.cpu(), t(fx["state"]))
    assert abs(float(rm) - float(fx["rmse"])) <= 1e-4 * float(fx["rmse"])
    pred = res.pred.cpu()
    _, pr = O.rmse(res.particles.cpu(), res.probs.cpu(), t(fx["state"]))
    assert_close(pred, pr, 1e-5, 1e-3, "fused prediction")


@pytest.mark.parametrize("kernel", KERNELS)
def test_device_rng_shard_invariance(kernel):
    """Device RNG is keyed on the GLOBAL row: rows [4,8) of a B=8 run equal a B=4 run with
    row_base = 4 (what each rank computes under batch sharding) when the gate is global."""
    from nfdpf.engine import FilterConfig, FilterEngine, ShardInfo
    fx = load("e2e_c2.npz")
    c = e2e_cfg(fx)
    models = _Models(weights(fx), c)
    N, T = 256, 6
    cfg = FilterConfig(N=N, NF_dyn=True, NF_cond=True, measurement="cos", resampler="soft", force_resample=True,
                       seed=1234, kernel=kernel)
    g = torch.Generator().manual_seed(3)
    enc = torch.randn(8, T, 32, generator=g).to(DEV)
    start = (torch.randn(8, 4, generator=g) * 10).to(DEV)
    vel = (torch.randn(8, T, 2, generator=g) * 3).to(DEV)
    full = FilterEngine(cfg, models).run(enc, start, vel)
    half = FilterEngine(cfg, models).run(enc[4:], start[4:], vel[4:], shard=ShardInfo(1, 0, 4, 4, None))
    assert torch.equal(full.particles[4:], half.particles)
    assert torch.equal(full.probs[4:], half.probs)
    assert torch.equal(full.index[4:], half.index)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("meas,res,nfd,nfc", [("cos", "soft", True, True), ("CRNVP", "ot", False, False),
                                              ("NN", "soft", True, False), ("gaussian", "soft", False, True)])
def test_device_rng_sanity(meas, res, nfd, nfc, kernel):
    """Device-RNG runs of each fused variant: finite, normalised, valid indices, repeatable."""
    from nfdpf.engine import FilterConfig, FilterEngine
    from model.models import build_likelihood
    fx = load("e2e_c3.npz" if meas == "CRNVP" else "e2e_c2.npz")
    c = dict(e2e_cfg(fx), measurement=meas)
    models = _Models(weights(fx), c)
    B, N, T = 8, 300, 5
    cfg = FilterConfig(N=N, NF_dyn=nfd, NF_cond=nfc, measurement=meas, resampler=res, force_resample=True, seed=9,
                       kernel=kernel)
    g = torch.Generator().manual_seed(4)
    enc = torch.randn(B, T, 32, generator=g).to(DEV)
    start = (torch.randn(B, 4, generator=g) * 10).to(DEV)
    vel = (torch.randn(B, T, 2, generator=g) * 3).to(DEV)
    a = FilterEngine(cfg, models).run(enc, start, vel)
    b = FilterEngine(cfg, models).run(enc, start, vel)
    assert torch.equal(a.particles, b.particles) and torch.equal(a.probs, b.probs)
    assert torch.isfinite(a.particles).all() and torch.isfinite(a.probs).all()
    s = a.probs.sum(-1)
    assert torch.allclose(s, torch.ones_like(s) + N * 1e-12, atol=1e-5)
    rows = torch.arange(B, device=DEV)[:, None, None] * N
    assert ((a.index >= rows) & (a.index < rows + N)).all()


@pytest.mark.parametrize("gated", [True, False])
def test_tiled_matches_fused(gated):
    """The tiled pipeline and the row-per-workgroup kernel compute the same step (same device
    RNG draws); only reduction orders differ.  N = 1000 spans 4 tiles per row."""
    from nfdpf.engine import FilterConfig, FilterEngine
    fx = load("e2e_c2.npz")
    models = _Models(weights(fx), e2e_cfg(fx))
    B, N, T = 6, 1000, 8
    g = torch.Generator().manual_seed(8)
    enc = torch.randn(B, T, 32, generator=g).to(DEV)
    start = (torch.randn(B, 4, generator=g) * 10).to(DEV)
    vel = (torch.randn(B, T, 2, generator=g) * 3).to(DEV)
    out = {}
    for k in KERNELS:
        cfg = FilterConfig(N=N, NF_dyn=True, NF_cond=True, measurement="cos", resampler="soft",
                           force_resample=not gated, seed=21, kernel=k)
        out[k] = FilterEngine(cfg, models).run(enc, start, vel)
    a, b = out["fused"], out["tiled"]
    assert torch.equal(a.noise, b.noise)
    agree = (a.index == b.index).float().mean().item()
    # resampling every step: a marker within rounding of a CDF step flips one index and the
    # row's later steps then follow different particles -- rounding-level differences
    # compound (the teacher-forced one-step tests pin each step exactly)
    assert agree > (0.999 if gated else 0.99), agree
    assert torch.allclose(a.particles[:, :2], b.particles[:, :2], rtol=1e-4, atol=1e-2)
    assert torch.allclose(a.pred[:, :2], b.pred[:, :2], rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("gated", [True, False])
def test_split_nets_match_pair_layout(gated):
    """Coupling nets on wave pairs (csrc/split.hpp: t-nets and s-nets on partner waves, LDS
    hand-off) against the one-wave pair layout: same device-RNG draws, only the order of the
    output layer's sum differs."""
    from nfdpf.engine import FilterConfig, FilterEngine
    fx = load("e2e_c2.npz")
    models = _Models(weights(fx), e2e_cfg(fx))
    B, N, T = 6, 1000, 8
    g = torch.Generator().manual_seed(18)
    enc = torch.randn(B, T, 32, generator=g).to(DEV)
    start = (torch.randn(B, 4, generator=g) * 10).to(DEV)
    vel = (torch.randn(B, T, 2, generator=g) * 3).to(DEV)
    out = {}
    for split in (False, True):
        cfg = FilterConfig(N=N, NF_dyn=True, NF_cond=True, measurement="cos", resampler="soft",
                           force_resample=not gated, seed=31, kernel="tiled", split_nets=split)
        out[split] = FilterEngine(cfg, models).run(enc, start, vel)
    a, b = out[False], out[True]
    assert torch.equal(a.noise, b.noise)
    agree = (a.index == b.index).float().mean().item()
    assert agree > (0.999 if gated else 0.99), agree  # see test_tiled_matches_fused
    assert torch.allclose(a.particles[:, :2], b.particles[:, :2], rtol=1e-4, atol=1e-2)
    assert torch.allclose(a.jac[:, :2], b.jac[:, :2], rtol=1e-4, atol=1e-4)
    assert torch.allclose(a.prior[:, :2], b.prior[:, :2], rtol=1e-4, atol=1e-3)
    assert torch.allclose(a.pred[:, :2], b.pred[:, :2], rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("gated", [True, False])
def test_split_prop_long_rows(gated):
    """The wave-pair layout on rows too long for the merged front launch (N > 4096: use_merged
    is false, use_split and use_rows hold), against the one-wave pair layout.  With split_nets
    each step launches tiled_rows_kernel, tiled_front_kernel<true>, tiled_dyn_kernel<true> and
    tiled_prop_split_kernel -- the only shape that reaches the last one (rows up to 4096 take the
    quad launch).  N = 4100: 17 tiles, the last with 4 valid lanes, so the softmax partials of
    waves without a valid lane are merged too."""
    from nfdpf.engine import FilterConfig, FilterEngine
    fx = load("e2e_c2.npz")
    models = _Models(weights(fx), e2e_cfg(fx))
    B, N, T = 2, 4100, 3
    g = torch.Generator().manual_seed(18)
    enc = torch.randn(B, T, 32, generator=g).to(DEV)
    start = (torch.randn(B, 4, generator=g) * 10).to(DEV)
    vel = (torch.randn(B, T, 2, generator=g) * 3).to(DEV)
    out = {}
    for split in (False, True):
        cfg = FilterConfig(N=N, NF_dyn=True, NF_cond=True, measurement="cos", resampler="soft",
                           force_resample=not gated, seed=31, kernel="tiled", split_nets=split)
        out[split] = FilterEngine(cfg, models).run(enc, start, vel)
    a, b = out[False], out[True]
    assert torch.equal(a.noise, b.noise)
    agree = (a.index == b.index).float().mean().item()
    assert agree > (0.999 if gated else 0.99), agree  # see test_tiled_matches_fused
    assert torch.allclose(a.particles[:, :2], b.particles[:, :2], rtol=1e-4, atol=1e-2)
    assert torch.allclose(a.jac[:, :2], b.jac[:, :2], rtol=1e-4, atol=1e-4)
    assert torch.allclose(a.prior[:, :2], b.prior[:, :2], rtol=1e-4, atol=1e-3)
    assert torch.allclose(a.pred[:, :2], b.pred[:, :2], rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("aligned", [False, True])
def test_speculative_gate_matches_exchange(aligned, monkeypatch):
    """Speculative-gate mode (every gate assumed off, verified after the pass from all steps'
    partials, rerun on a fired gate) returns exactly the per-step-gate pass: bit-identical
    histories and obs-likelihood.  aligned=True uses the fixture's encodings aligned with the
    true state, on which the gate fires -- the verification must catch it and rerun.  The
    step-by-step speculative launches (NFDPF_PASS=0; the one-launch pass: tests/test_gpu_pass.py)."""
    from nfdpf.engine import FilterConfig, FilterEngine
    monkeypatch.setenv("NFDPF_PASS", "0")
    fx = load("e2e_c2.npz")
    c = e2e_cfg(fx)
    models = _Models(weights(fx), c)
    if aligned:
        enc, start, vel = t(fx["enc"]).to(DEV), t(fx["start"]).to(DEV), t(fx["vel"]).to(DEV)
        N = int(fx["N"])
    else:
        g = torch.Generator().manual_seed(5)
        B, T, N = 6, 8, 1000
        enc = torch.randn(B, T, 32, generator=g).to(DEV)
        start = (torch.randn(B, 4, generator=g) * 10).to(DEV)
        vel = (torch.randn(B, T, 2, generator=g) * 3).to(DEV)
    out = {}
    for spec in (False, True):
        cfg = FilterConfig(N=N, NF_dyn=True, NF_cond=True, measurement="cos", resampler="soft", seed=77,
                           kernel="tiled", speculate_gate=spec)
        out[spec] = FilterEngine(cfg, models).run(enc, start, vel)
    a, b = out[False], out[True]
    for f in ("particles", "probs", "noise", "lik", "index", "jac", "prior", "pred"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert torch.equal(a.obs_likelihood, b.obs_likelihood)
    B, T = enc.shape[0], enc.shape[1]
    ident = torch.arange(N, device=DEV) + N * torch.arange(B, device=DEV)[:, None]
    fired = int((a.index != ident[:, None, :]).any(-1).any(0).sum())
    assert (fired > 0) == aligned, fired


def test_gate_batch_matches_single():
    """nfdpf_ess_gate_tiled_batch == nfdpf_ess_gate_tiled step by step (both branches)."""
    from nfdpf import ops
    g = torch.Generator().manual_seed(6)
    T, B, N = 7, 5, 1000
    tiles = ops.tiled_tiles(N)
    parts = torch.zeros(T, B, tiles, 4, dtype=torch.float64)
    parts[..., 0] = torch.randn(T, B, tiles, generator=g, dtype=torch.float64) * 0.01
    parts[..., 1] = 250.0 * (1 + 0.1 * torch.rand(T, B, tiles, generator=g, dtype=torch.float64))
    # sum e^2 ~ sum e (spread weights, 1/sum p^2 ~ N: gate off) or ~ (sum e)^2 (peaked: on)
    peak = (torch.arange(T) % 2 == 1)[:, None, None]
    parts[..., 2] = torch.where(peak, parts[..., 1] ** 2, parts[..., 1])
    parts = parts.to(DEV)
    batch = ops.ess_gate_tiled_batch(parts, N, 0, False).cpu()
    single = torch.stack([ops.ess_gate_tiled(parts[k].contiguous(), N, k).cpu()[0] for k in range(T)])
    assert torch.equal(batch, single)
    assert 0 < int(batch.sum()) < T


@pytest.mark.parametrize("N,force", [(2000, True), (2000, False), (700, True)])
def test_rows_kernel_matches_per_tile_resampling(N, force, monkeypatch):
    """Long rows (soft resampler off the merged path): tiled_rows_kernel takes the gate, the
    deferred row normaliser and the row's resampling once per row; the per-tile path does all
    three in every tile.  Same arithmetic, so the passes are bit-identical (both forced through
    NFDPF_TILED_ROWS_MIN_N)."""
    import _fullsize as F
    from nfdpf.engine import FilterConfig, FilterEngine
    wl = F.workload("c2_full", B=6, N=N, T=6)
    models = wl["models"].to(DEV)
    out = {}
    for min_n in (0, 1 << 30):  # rows kernel for every N / never
        monkeypatch.setenv("NFDPF_TILED_ROWS_MIN_N", str(min_n))
        # NF_cond off: not the merged C2 path, so the front launch is tiled_front_kernel
        cfg = FilterConfig(N=N, NF_dyn=True, NF_cond=False, measurement="cos", resampler="soft",
                           force_resample=force, seed=5, kernel="tiled")
        out[min_n] = FilterEngine(cfg, models).run(wl["enc"].to(DEV), wl["start"].to(DEV), wl["vel"].to(DEV))
    a, b = out[0], out[1 << 30]
    for f in ("particles", "probs", "noise", "lik", "index", "jac", "prior", "pred"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    ident = torch.arange(N, device=DEV) + N * torch.arange(6, device=DEV)[:, None]
    fired = int((a.index != ident[:, None, :]).any(-1).any(0).sum())
    print(f"\nN={N} force={force}: resampled in {fired} of 6 steps")
    if force:  # step 0 resamples uniform weights: the identity map, not counted here
        assert fired >= 5


@pytest.mark.gpu
@pytest.mark.parametrize("N,nf_dyn,resampler,force", [(1000, False, "ot", True), (777, True, "soft", False),
                                                      (65, False, "ot", False)])
def test_crnvp_mfma_matches_valu(N, nf_dyn, resampler, force, monkeypatch):
    """CRNVP without --NF-cond: the step launch's measurement on f32 MFMA (64 particles per wave,
    csrc/crnvp_mfma.hpp, the default) against the per-lane VALU measurement (NFDPF_CM_MFMA=0) on
    the same step: the same function with the tanh algebra folded into the weights and other
    summation orders, so the likelihoods agree to rounding at step 0, whose inputs are identical
    (later steps follow the resampler, which these differences can tip).
    Ragged N (65: one full wave and one particle) included."""
    import _fullsize as F
    from nfdpf.engine import FilterConfig, FilterEngine
    wl = F.workload("c3_full", B=5, N=N, T=4)
    models = wl["models"].to(DEV)
    out = {}
    for mf in ("1", "0"):
        monkeypatch.setenv("NFDPF_CM_MFMA", mf)
        monkeypatch.setenv("NFDPF_PASS", "0")  # the step launches
        cfg = FilterConfig(N=N, NF_dyn=nf_dyn, NF_cond=False, measurement="CRNVP", resampler=resampler,
                           force_resample=force, seed=7, kernel="tiled")
        out[mf] = FilterEngine(cfg, models).run(wl["enc"].to(DEV), wl["start"].to(DEV), wl["vel"].to(DEV))
        torch.cuda.synchronize()
    a, b = out["1"], out["0"]
    assert torch.isfinite(a.lik).all()
    assert torch.equal(a.noise[:, 0], b.noise[:, 0])
    # the stored likelihood is shifted by the row max of the raw one, whose magnitude (~1e3 at
    # these weights) sets the rounding: 4e-6 of the row's likelihood scale, besides 1e-5 relative
    la, lb = a.lik[:, 0].cpu(), b.lik[:, 0].cpu()
    scale = lb.abs().amax(-1, keepdim=True)
    tol = 1e-5 * lb.abs() + 4e-6 * scale + 1e-4
    assert bool(((la - lb).abs() <= tol).all()), float(((la - lb).abs() / (lb.abs() + scale)).max())
    # a likelihood error d moves its weight by the factor e^d (and the row's normaliser by at most the
    # largest such factor): twice the likelihood bound, relative
    pa, pb = a.probs[:, 0].cpu(), b.probs[:, 0].cpu()
    assert bool(((pa - pb).abs() <= 2 * tol.amax(-1, keepdim=True) * pb + 1e-9).all())
    # ... and both against the reference: step 0 of the oracle (float32 and float64) from the same
    # initial particles (the engine's device draw, seed 7: particle_init's) and the launch's own
    # noise.  Step 0's weights are uniform, so its gate is off unless forced; forced, the oracle
    # resamples them as the launch does (OT: its own FP64 Sinkhorn, one call at this size).
    # Both launches must sit inside the float32 oracle's own error envelope against float64
    # (_check_envelope, the constants of test_gpu_pass_cm.test_cm_pass_vs_oracle), which says
    # which side is nearer the truth, not only that the two agree.
    from nfdpf import ops
    from test_gpu_pass import _Replay
    B = wl["B"]
    start = wl["start"].to(DEV)
    x0, logw0 = ops.particle_init(start[:, :2], B, N, 128.0, False, 7, 0, DEV)
    if not nf_dyn and not force:  # the bootstrap proposal: x_0 = (x0 + vel) + eps, the same two adds
        assert torch.equal(a.particles[:, 0], (x0 + start[:, None, 2:4]) + a.noise[:, 0]), "not the engine's initial draw"
    c = F.cfg_dict(dict(wl["flags"], NF_dyn=nf_dyn, resampler=resampler), N)
    w = {k: v.detach().float().cpu() for k, v in models.state_dict().items()}
    refs = {}
    for dt in (torch.float32, torch.float64):
        with O.precision(dt), torch.no_grad():
            r = O.filtering(c, O.cast_params(w, dt), wl["enc"][:, :1].cpu().to(dt), wl["start"].cpu().to(dt),
                            wl["vel"][:, :1].cpu().to(dt), rng=_Replay(a.noise[:, :1]), force_resample=force,
                            init=(x0.cpu().to(dt), logw0.cpu().to(dt)))
        refs[dt] = (r[3].double().numpy(), r[1].double().numpy())  # lik, probs: [B, 1, N]
    (l32, p32), (l64, p64) = refs[torch.float32], refs[torch.float64]
    print(f"\nCRNVP step 0 vs oracle, N={N} nf_dyn={nf_dyn} {resampler} force={force}: float32 oracle max err "
          f"lik {np.abs(l32 - l64).max():.3e} weights {np.abs(p32 - p64).max():.3e}")
    ours = {tag: (run.lik[:, :1].cpu().double().numpy(), run.probs[:, :1].cpu().double().numpy())
            for tag, run in (("mfma", a), ("valu", b))}
    for tag, (lo, po) in ours.items():  # (every figure before any assertion)
        print(f"  {tag}: max err lik {np.abs(lo - l64).max():.3e} weights {np.abs(po - p64).max():.3e}")
    for tag, (lo, po) in ours.items():
        _check_envelope(lo, l32, l64, 1e-5, 2e-5, f"{tag} likelihood")
        _check_envelope(po, p32, p64, 1e-5, 1e-9, f"{tag} weights")
