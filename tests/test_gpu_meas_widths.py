"""Frame-encoding widths 16 and 64 (--hiddensize) of the cos / CRNVP / NN / gaussian measurements
on the HIP kernels (csrc/measure.hip, the width-templated backwards of measure_bwd.hip /
nn_bwd.hip, nfdpf_cond_stack[_backward] at dim 16 / 64): kernel, module, FilterEngine and
DPF(args).  GPU box only.

Weights are at trained-like scales -- particle encoder N(0, 0.5^2), flows N(0, 0.1^2),
likelihood_est N(0, 0.02^2) (wider, its sigmoid saturates to log-likelihood 0) -- since at the
reference init the likelihood is flat and hides errors.

Tolerances are the project's own: the raw likelihoods use tests/test_gpu_parity.py's
_check_envelope with its factors (ours against the float64 oracle, within those factors of the
float32 oracle's own error, rtol 1e-5 / atol 2e-5, one row of N particles = one envelope); the
fixtures test_measurement_golden's 1e-5 / 2e-5; the backwards the bounds tests/test_gpu_backward.py
uses for the same kernels at 32 (_soft_check for cos and NN, _check_tensor for CRNVP and -- the
same row-max cancellation -- gaussian); the engine cases the assert_close values of
test_filtering_free_running, the likelihood history at the obs-likelihood's 1e-4 / 1e-3 (the
obs-likelihood is a mean of log-weights that the likelihood enters with weight 1).
"""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from _util import assert_close, group, load, t, weights
from oracle import dpf_oracle as O
from test_gpu_backward import _check_tensor, _ref_stack, _soft_check
from test_gpu_parity import _check_envelope

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = ["cos", "CRNVP", "NN", "gaussian"]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from nfdpf import _lib
    _lib.load()
    assert torch.cuda.is_available()


def _perturb(module, std, gen):
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * std)


class _Mods(nn.Module):
    """The DPF sub-modules the engine and the measurement kernels read, at width H, trained-like."""

    def __init__(self, H, seed=0):
        super().__init__()
        from model.models import build_conditional_nf, build_likelihood, build_particle_encoder
        g = torch.Generator().manual_seed(seed)
        self.nf_dyn = build_conditional_nf(2, 4, 2)
        self.cond_model = build_conditional_nf(2, 4 + H, 2)
        self.particle_encoder = build_particle_encoder(H, 2)
        self.cnf_measurement = build_conditional_nf(2, H, H, prior_std=2.5)
        self.likelihood_est = build_likelihood(H, 2)
        _perturb(self.particle_encoder, 0.5, g)
        for m in (self.nf_dyn, self.cond_model, self.cnf_measurement):
            _perturb(m.flows, 0.1, g)
        _perturb(self.likelihood_est, 0.02, g)

    def sd(self):
        return {k: v.detach().cpu().clone() for k, v in self.state_dict().items()}


def _blobs(mods, kind):
    from nfdpf.pack import encoder_tensors, flows_tensors, paired_mlp_tensors
    cat = lambda ts: torch.cat([a.detach().reshape(-1).float() for a in ts]).to(DEV)  # noqa: E731
    pe = cat(encoder_tensors(mods.particle_encoder))
    mb = None
    if kind == "CRNVP":
        mb = cat(flows_tensors(mods.cnf_measurement.flows))
    elif kind == "NN":
        mb = cat(paired_mlp_tensors(mods.likelihood_est))
    return pe, mb


def _oracle_meas(kind, sd, enc, x, dt):
    with O.precision(dt):
        w = O.cast_params(sd, dt)
        return O.make_measurement(dict(measurement=kind, n_flows=2), w)(enc.to(dt), x.to(dt))


_FWD = {}


def _fwd_case(E):
    """One set of modules, inputs and float32 / float64 oracle likelihoods per width, shared."""
    if E not in _FWD:
        mods = _Mods(E, seed=E)
        g = torch.Generator().manual_seed(100 + E)
        B, N = 3, 257
        enc = torch.randn(B, E, generator=g)
        x = torch.randn(B, N, 2, generator=g) * 30
        sd = mods.sd()
        refs = {k: (_oracle_meas(k, sd, enc, x, torch.float32), _oracle_meas(k, sd, enc, x, torch.float64))
                for k in KINDS}
        _FWD[E] = (mods, enc, x, refs)
    return _FWD[E]


@pytest.mark.parametrize("E", [16, 64, 32])
@pytest.mark.parametrize("kind", KINDS)
def test_measurement_forward_vs_oracle(kind, E):
    """nfdpf_measurement at B = 3, N = 257 (one past the 256-thread block: the strided tail, and a
    row max over a partly filled block) against the float64 oracle; E = 32 is the control."""
    from nfdpf import ops
    mods, enc, x, refs = _fwd_case(E)
    pe, mb = _blobs(mods, kind)
    lik = ops.measurement(kind, pe, mb, 2, enc.to(DEV), x.to(DEV), 2.5)
    r32, r64 = refs[kind]
    assert torch.isfinite(lik).all()
    e_o = (lik.cpu().double() - r64).abs()
    print(f"{kind} E={E}: max |ours - f64| {float(e_o.max()):.3e}, float32 oracle {float((r32.double() - r64).abs().max()):.3e}, "
          f"max |lik| {float(r64.abs().max()):.3e}")
    _check_envelope(lik.cpu()[:, None], r32[:, None], r64[:, None], 1e-5, 2e-5, f"{kind} E={E}")


def _fixture_module(kind, E, fx):
    from model.models import (build_conditional_nf, build_likelihood, build_particle_encoder,
                              measurement_model_cnf, measurement_model_cosine_distance,
                              measurement_model_Gaussian, measurement_model_NN)
    w = weights(fx)
    pe = build_particle_encoder(E, 2)
    pe.load_state_dict({k[len("particle_encoder."):]: v for k, v in w.items() if k.startswith("particle_encoder.")})
    if kind == "cos":
        return measurement_model_cosine_distance(pe).to(DEV)
    if kind == "gaussian":
        dist = torch.distributions.MultivariateNormal(torch.ones(E).to(DEV), 100 * torch.eye(E).to(DEV))
        return measurement_model_Gaussian(pe.to(DEV), dist)
    if kind == "NN":
        le = build_likelihood(E, 2)
        le.load_state_dict({k[len("likelihood_est."):]: v for k, v in w.items() if k.startswith("likelihood_est.")})
        return measurement_model_NN(pe, le).to(DEV)
    cnf = build_conditional_nf(2, E, E, prior_std=2.5)
    sd = cnf.state_dict()
    sd.update({k[len("cnf_measurement."):]: v for k, v in w.items() if k.startswith("cnf_measurement.")})
    cnf.load_state_dict(sd)
    return measurement_model_cnf(pe, cnf).to(DEV)


@pytest.mark.parametrize("E", [16, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_measurement_reference_fixture(kind, E):
    """ops.measurement and the measurement_model_* module against the reference's own output at
    --hiddensize 16 / 64 (tests/golden/gen_meas_widths.py), at test_measurement_golden's tolerance."""
    from nfdpf import ops
    from nfdpf.pack import encoder_tensors, flows_tensors, paired_mlp_tensors
    fx = group(load("meas_widths.npz"), f"{kind}_{E}")
    m = _fixture_module(kind, E, fx)
    cat = lambda ts: torch.cat([a.detach().reshape(-1).float() for a in ts]).to(DEV)  # noqa: E731
    pe = cat(encoder_tensors(m.particle_encoder))
    mb = cat(flows_tensors(m.CNF.flows)) if kind == "CRNVP" else \
        cat(paired_mlp_tensors(m.likelihood_estimator)) if kind == "NN" else None
    enc, x = t(fx["enc"]).to(DEV), t(fx["x"]).to(DEV)
    lik = ops.measurement(kind, pe, mb, 2, enc, x, 2.5)
    assert_close(lik.cpu(), fx["lik"], 1e-5, 2e-5, f"{kind} E={E} kernel")
    with torch.no_grad():
        lm = m(enc, x)
    assert_close(lm.cpu(), fx["lik"], 1e-5, 2e-5, f"{kind} E={E} module")


def _ref_lik(kind, E, pe, extra, enc, x, dt, am=None):
    """The module's torch_forward math in dtype dt on the CPU (model/models.py:206-278)."""
    B, N = x.shape[:2]
    es = pe(x)
    eo = enc[:, None, :].repeat(1, N, 1)
    if kind == "cos":
        cosd = 1.0 - (torch.nn.functional.normalize(eo, p=2, dim=-1, eps=1e-12) *
                      torch.nn.functional.normalize(es, p=2, dim=-1, eps=1e-12)).sum(-1)
        return (1 / (1e-7 + cosd)).log(), None
    if kind == "NN":
        return extra(torch.cat([eo, es], dim=-1))[..., 0].log(), None
    if kind == "gaussian":
        d = eo - es - 1.0
        u = -0.5 * (d * d).sum(-1) / 100.0 - 0.5 * E * np.log(2 * np.pi * 100.0)
    else:
        _, ld, lp = _ref_stack(extra, eo.reshape(-1, E), es.reshape(-1, E), False, (0.0, 2.5), dt)
        u = (lp + ld).reshape(B, N)
    # the row max at OUR argmax (lik == 0 there exactly), as test_crnvp_measurement_backward_vs_autograd
    return u - u.gather(1, am[:, None]), u


@pytest.mark.parametrize("E", [16, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_measurement_backward_vs_autograd(kind, E, monkeypatch):
    """The module under autograd (HIP backward at width E) == float64 autograd of its
    torch_forward math: d/d encodings, particles and every parameter, at B = 2, N = 70 (rows not
    a multiple of the 64-particle workgroups); the backward run twice is bit-equal."""
    from model.models import (build_conditional_nf, build_likelihood, build_particle_encoder,
                              measurement_model_cnf, measurement_model_cosine_distance,
                              measurement_model_Gaussian, measurement_model_NN)
    from nfdpf import ops
    calls = []
    real = ops.particle_encoder_backward if kind != "cos" else ops.cos_measurement_backward
    name = "particle_encoder_backward" if kind != "cos" else "cos_measurement_backward"
    monkeypatch.setattr(ops, name, lambda *a, **k: calls.append(1) or real(*a, **k))
    g = torch.Generator().manual_seed(7 * E + len(kind))
    B, N = 2, 70
    pe = build_particle_encoder(E, 2)
    _perturb(pe, 0.5, g)
    extra = None
    if kind == "cos":
        m = measurement_model_cosine_distance(copy.deepcopy(pe).to(DEV))
    elif kind == "gaussian":
        dist = torch.distributions.MultivariateNormal(torch.ones(E).to(DEV), 100 * torch.eye(E).to(DEV))
        m = measurement_model_Gaussian(copy.deepcopy(pe).to(DEV), dist)
    elif kind == "NN":
        extra = build_likelihood(E, 2)
        _perturb(extra, 0.02, g)
        m = measurement_model_NN(copy.deepcopy(pe).to(DEV), copy.deepcopy(extra).to(DEV))
    else:
        cnf = build_conditional_nf(2, E, E, prior_std=2.5)
        _perturb(cnf.flows, 0.1, g)
        extra = [copy.deepcopy(f).cpu() for f in cnf.flows]
        m = measurement_model_cnf(copy.deepcopy(pe).to(DEV), cnf.to(DEV))
    enc = torch.randn(B, E, generator=g)
    x = torch.randn(B, N, 2, generator=g) * 5
    gl = torch.randn(B, N, generator=g)

    def ours():
        m.zero_grad()
        encd, xd = enc.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
        lik = m(encd, xd)
        (lik * gl.to(DEV)).sum().backward()
        return lik.detach(), encd.grad, xd.grad, [p.grad.clone() for p in m.parameters()]
    lik, g_enc, g_x, g_p = ours()
    assert len(calls) == 1, f"the backward did not run through ops.{name}"
    lik2, g_enc2, g_x2, g_p2 = ours()
    assert torch.equal(g_enc, g_enc2) and torch.equal(g_x, g_x2), "the backward is not deterministic"
    assert all(torch.equal(a, b) for a, b in zip(g_p, g_p2)), "the parameter gradients are not deterministic"
    am = (lik == 0).float().argmax(-1).cpu() if kind in ("CRNVP", "gaussian") else None
    refs = {}
    for dt in (torch.float32, torch.float64):
        rpe = copy.deepcopy(pe).to(dt)
        rex = None if extra is None else ([copy.deepcopy(f).to(dt) for f in extra] if kind == "CRNVP"
                                          else copy.deepcopy(extra).to(dt))
        er, xr = enc.to(dt).clone().requires_grad_(True), x.to(dt).clone().requires_grad_(True)
        lr, u = _ref_lik(kind, E, rpe, rex, er, xr, dt, am)
        (lr * gl.to(dt)).sum().backward()
        ps = list(rpe.parameters())
        if kind == "CRNVP":
            ps += [p for f in rex for p in f.parameters()]
        elif kind == "NN":
            ps += list(rex.parameters())
        refs[dt] = (lr.detach(), u, er.grad, xr.grad, [p.grad for p in ps])
    lr64, u64, ge64, gx64, p64 = refs[torch.float64]
    _, _, ge32, gx32, p32 = refs[torch.float32]
    names = [n for n, _ in m.named_parameters()]
    assert len(names) == len(p64)
    if kind in ("cos", "NN"):
        _soft_check(lik, lr64, "lik")
        _soft_check(g_x, gx64, "dL/dx")
        _soft_check(g_enc, ge64, "dL/denc")
        for n, a, r in zip(names, g_p, p64):
            _soft_check(a, r, f"dL/d{n}")
    else:
        # lik is a difference of two log-densities: its fp32 error scales with |u|, not |lik|
        d = (lik.double().cpu() - lr64).abs()
        assert float(d.max()) <= 1e-6 * float(u64.detach().abs().max()) + 1e-6, f"lik: max |d| {float(d.max()):.3g}"
        _check_tensor(g_x, gx32, gx64, "dL/dx")
        _check_tensor(g_enc, ge32, ge64, "dL/denc")
        for n, a, r32, r64 in zip(names, g_p, p32, p64):
            _check_tensor(a, r32, r64, f"dL/d{n}")


class _Recorder:
    """O.HostRNG that keeps its draws: step t's noise, and its offsets where the step resampled."""

    def __init__(self, seed):
        self.rng = O.HostRNG(torch.Generator().manual_seed(seed))
        self.gen = self.rng.gen
        self.noises, self.offs = [], {}

    def offsets(self, B, N):
        v = self.rng.offsets(B, N)
        self.offs[len(self.noises)] = v.clone()
        return v

    def noise(self, B, N, std):
        v = self.rng.noise(B, N, std)
        self.noises.append(v.clone())
        return v


class _Replay:
    """The recorded draws, in the engine's host-RNG interface (nfdpf.engine.HostDraws)."""

    def __init__(self, rec):
        self.rec, self.k = rec, 0

    def offsets(self, B, N):
        return self.rec.offs.get(self.k, torch.zeros(B)).clone()

    def noise(self, B, N, std):
        self.k += 1
        return self.rec.noises[self.k - 1].clone()


ENGINE_CASES = {
    # name: (NF_dyn, NF_cond, measurement, resampler, force_resample, frame encodings)
    # Encodings: "aligned" = the particle encoder on the true positions + 30 % noise, as a trained
    # frame encoder would give; "normal<k>" = k x N(0, 1).
    #
    # The CRNVP + OT cases take normal encodings: aligned ones are ~1e2 per component at these
    # encoder scales, the CRNVP prior then puts the raw likelihood at ~4e3, which float32 resolves
    # to ~1e-3 -- the weights collapse onto one particle and the OT plan amplifies that noise: the
    # float32 ORACLE itself then differs from its float64 run by 1.2e-2 in the particles (E = 64;
    # 2.6e-3 at the tuned E = 32), ten times the tolerance, so the check could tell nothing.
    # Measured on the CPU, oracle float32 against oracle float64 on the same draws, as the excess
    # over each tolerance (negative = inside):
    #   4 x N(0, 1), gated:  E = 16 particles -9.8e-4, weights -1.0e-7 (the ESS falls to 0.17 N after
    #                        step 1: the OT resampler runs at step 2);
    #                        E = 64 weights +3.5e-7 (3 x N(0, 1): +3.3e-7): the oracle's own float32
    #                        error is outside the weights' bound wherever the gate fires by itself;
    #   N(0, 1), forced:     E = 64 particles -9.8e-4, weights -1.7e-7 (the OT resampler runs at
    #                        every step; the raw likelihood is ~2, the weights <= 8e-3).
    # So the gated case runs at E = 16 and the forced one at both widths.
    "c2_cos_soft_forced": (True, True, "cos", "soft", True, "aligned"),
    "c3_crnvp_ot": (False, False, "CRNVP", "ot", False, "normal4"),
    "c3_crnvp_ot_forced": (False, False, "CRNVP", "ot", True, "normal1"),
    "nn_soft": (True, False, "NN", "soft", False, "aligned"),
    "gaussian_soft": (False, True, "gaussian", "soft", False, "aligned"),
}


def _run_engine_case(name, E, kernel):
    from nfdpf.engine import FilterConfig, FilterEngine
    nfd, nfc, meas, res, force, encodings = ENGINE_CASES[name]
    B, N, T = 2, 300, 3
    mods = _Mods(E, seed=1000 + E)
    g = torch.Generator().manual_seed(5 + E)
    state = torch.cat([torch.randn(B, T, 2, generator=g) * 20, torch.randn(B, T, 2, generator=g) * 3], -1)
    start = torch.cat([state[:, 0, :2] + torch.randn(B, 2, generator=g), state[:, 0, 2:]], -1)
    with torch.no_grad():  # frame encodings near the true positions' particle encodings ("aligned")
        enc = mods.particle_encoder(state[..., :2])
        enc = enc * (1 + 0.3 * torch.randn(enc.shape, generator=g))
    if encodings.startswith("normal"):
        enc = float(encodings[len("normal"):]) * torch.randn(B, T, E, generator=g)
    vel = state[..., 2:].contiguous()
    x0 = (torch.rand(B, N, 2, generator=g) - 0.5) * 128
    lw0 = torch.log(torch.ones(B, N) / N)
    cfg = dict(N=N, NF_dyn=nfd, NF_cond=nfc, measurement=meas, resampler=res, alpha=0.5, eps=0.1, scaling=0.75,
               threshold=1e-3, max_iter=100, pos_noise=20.0, vel_noise=20.0, width=128, n_flows=2)
    rec = _Recorder(11)
    ref = O.filtering(cfg, mods.sd(), enc, start, vel, rng=rec, force_resample=force, init=(x0, lw0))
    eng = FilterEngine(FilterConfig(N=N, NF_dyn=nfd, NF_cond=nfc, measurement=meas, resampler=res, rng_mode="host",
                                    kernel=kernel, force_resample=force), mods.to(DEV))
    out = eng.run(enc.to(DEV), start.to(DEV), vel.to(DEV), host=_Replay(rec), init=(x0, lw0))
    torch.cuda.synchronize()
    x, p, _, lik, _, idx, _, _, obs = ref
    assert str(E) in (eng.pass_fallback_reason or ""), eng.pass_fallback_reason
    print(f"{name} E={E} {kernel}: fired {out.fired}, max |lik| {float(lik.abs().max()):.3e}, "
          f"max |dlik| {float((out.lik.cpu() - lik).abs().max()):.3e}, obs {float(out.obs_likelihood):.6f} / {float(obs):.6f}")
    if res == "ot":
        assert any(out.fired), "the OT resampler never ran"
    np.testing.assert_array_equal(out.index.cpu().numpy(), idx.numpy().astype(np.int64))
    assert_close(out.particles.cpu(), x, 1e-4, 1e-3, "particles")
    assert_close(out.probs.cpu(), p, 1e-4, 1e-7, "weights")
    assert_close(out.lik.cpu(), lik, 1e-4, 1e-3, "likelihood")
    assert abs(float(out.obs_likelihood) - float(obs)) <= 1e-4 * abs(float(obs)) + 1e-3
    _, pr = O.rmse(out.particles.cpu(), out.probs.cpu(), state)
    assert_close(out.pred.cpu(), pr, 1e-5, 1e-3, "prediction")


@pytest.mark.parametrize("name,E", [("c2_cos_soft_forced", 16), ("c2_cos_soft_forced", 64), ("c3_crnvp_ot", 16),
                                    ("c3_crnvp_ot_forced", 16), ("c3_crnvp_ot_forced", 64)])
def test_engine_tiled_vs_oracle(name, E):
    """FilterEngine (tiled step launches, the measurement as the EXTERNAL phase) against
    oracle.filtering on the same host draws: B = 2, N = 300 (two tiles, ragged), T = 3.  The cos
    case compares lik and the obs-likelihood: a row-max shift applied to it would show there."""
    _run_engine_case(name, E, "tiled")


@pytest.mark.parametrize("name", ["nn_soft", "gaussian_soft"])
def test_engine_fused_vs_oracle(name):
    """The same through the one-workgroup-per-row step kernel (kernel="fused") at E = 64."""
    _run_engine_case(name, 64, "fused")


@pytest.mark.parametrize("kind", ["cos", "NN"])
def test_step_likelihood_equals_standalone_at_32(kind):
    """The step kernels and the standalone kernel instantiate one measure<E, MEAS> (csrc/measure.hpp)
    at E = 32: the likelihood history of FilterEngine's step launches (kernel="tiled", the one-launch
    pass off, device RNG; B = 2, N = 300 -- two tiles, the second partial -- T = 2) against
    ops.measurement on the same encodings and the history's own particles.  cos and NN: phase 2
    applies no row-max shift to them, so the history holds the raw value."""
    from nfdpf import ops
    from nfdpf.engine import FilterConfig, FilterEngine
    E, B, N, T = 32, 2, 300, 2
    mods = _Mods(E, seed=2000)
    g = torch.Generator().manual_seed(21)
    state = torch.cat([torch.randn(B, T, 2, generator=g) * 20, torch.randn(B, T, 2, generator=g) * 3], -1)
    with torch.no_grad():  # "aligned" frame encodings, as _run_engine_case
        enc = mods.particle_encoder(state[..., :2])
        enc = (enc * (1 + 0.3 * torch.randn(enc.shape, generator=g))).to(DEV)
    pe, mb = _blobs(mods, kind)
    eng = FilterEngine(FilterConfig(N=N, measurement=kind, resampler="soft", kernel="tiled", seed=5), mods.to(DEV))
    eng.pass_disabled = True  # the step launches
    out = eng.run(enc, state[:, 0].to(DEV), state[..., 2:].contiguous().to(DEV))
    torch.cuda.synchronize()
    assert not eng.last_pass and torch.isfinite(out.lik).all()
    for t_ in range(T):
        lik = ops.measurement(kind, pe, mb, 2, enc[:, t_].contiguous(), out.particles[:, t_].contiguous(), 2.5)
        print(f"{kind} t={t_}: max |step - standalone| {float((out.lik[:, t_] - lik).abs().max()):.3e}, "
              f"max |lik| {float(lik.abs().max()):.3e}")
        assert torch.equal(out.lik[:, t_], lik), f"{kind}, step {t_}"


def _dpf(meas, H=64, B=2, N=50, T=3):
    from _tiny import TinyDecoder, TinyEncoder
    from arguments import parse_args
    from DPFs import DPF
    a = parse_args([])
    a.measurement, a.hiddensize, a.num_particles, a.batchsize, a.sequence_length = meas, H, N, B, T
    a.NF_dyn, a.NF_cond = True, True
    torch.manual_seed(3)
    dpf = DPF(a)
    dpf.encoder, dpf.decoder = TinyEncoder(H), TinyDecoder(H)
    g = torch.Generator().manual_seed(4)
    _perturb(dpf.particle_encoder, 0.5, g)
    if meas == "CRNVP":
        _perturb(dpf.cnf_measurement.flows, 0.1, g)
    return dpf.to(DEV), a


@pytest.mark.parametrize("meas", ["cos", "CRNVP"])
def test_dpf_hiddensize_64(meas):
    """DPF(args) at --hiddensize 64: filtering_pos under no_grad runs FilterEngine (the external-
    measurement step path, its fallback reason naming the width); a training forward + backward
    leaves finite, nonzero gradients on the particle encoder and the measurement's parameters."""
    B, N, T = 2, 50, 3
    dpf, a = _dpf(meas, 64, B, N, T)
    g = torch.Generator().manual_seed(9)
    img = torch.rand(B, T, 128, 128, 3, generator=g)
    state = torch.cat([torch.randn(B, T, 2, generator=g) * 20, torch.randn(B, T, 2, generator=g) * 3], -1)
    start = state[:, 0].clone()
    with torch.no_grad(), pytest.warns(RuntimeWarning, match="64"):
        out = dpf.filtering_pos(img.permute(0, 1, 4, 2, 3).to(DEV), start.to(DEV), state[..., 2:].to(DEV))
    assert getattr(dpf, "_engine", None) is not None
    assert "64" in dpf._engine.pass_fallback_reason
    assert out[0].shape == (B, T, N, 2) and torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all()
    assert torch.allclose(out[1].sum(-1), torch.ones(B, T, device=DEV), atol=1e-4)
    dpf.train()
    inputs = (img[:, 0], start, img, state, torch.zeros(B, T), torch.ones(B, T))
    np.random.seed(0)
    torch.manual_seed(0)
    res = dpf.forward(inputs, train=True)
    dpf.zero_grad()
    res[0].backward()
    mods = [dpf.particle_encoder] + ([dpf.cnf_measurement] if meas == "CRNVP" else [])
    for m in mods:
        for n, p in m.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
        assert any(bool(p.grad.any()) for p in m.parameters()), "all-zero gradients"


def test_unsupported_width_on_device():
    """E = 24 with real device buffers: NFDPF_EINVAL before any launch, the widths in the message."""
    from nfdpf import _lib, ops
    mods = _Mods(32)
    pe, _ = _blobs(mods, "cos")
    with pytest.raises(_lib.NfdpfError, match="16 32 64"):
        ops.measurement("cos", pe, None, 2, torch.zeros(2, 24, device=DEV), torch.zeros(2, 8, 2, device=DEV))
