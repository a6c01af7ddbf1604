"""The C3 one-launch pass with the CRNVP measurement on f32 MFMA (csrc/crnvp_mfma.hpp, the
default C3 path) against the CPU oracle at TRAINED-LIKE weight scales, every gate held off on both
sides.  GPU box only.

With every gate off the C3 pass has no discrete decision: nothing resamples, the index map is the
identity and x_t = (x_{t-1} + vel_t) + eps_t, so a free-running comparison is clean at any weight
scale.  Ours is the raw speculative pass (run(speculate=True, finish=False): what the launch
wrote, before any verification or rerun); the oracle runs with ``gates=[False] * T`` (its
test-only override) on the same initial particles and the pass's own device noise, in float32 and
float64.  At the reference's init weights (tests/test_gpu_pass_cm.py) the coupling nets are near
zero and the likelihood nearly flat: a wrong fragment entry, a wrong folded constant or swapped
t / s rows barely move the result there.  Here they do (tests/_fullsize.CASES):

  c3_full  encoder 0.5, measurement flows 0.1: sharp -- ESS / N ~ 0.005 after one step, |lik| ~ 2e3
  c3_mid   encoder 0.2: ESS / N decays slowly, hundreds of particles carry weight, mixed gates

The kernels reached, each oracle-checked here at trained scales:
  tiled_pass_cm_kernel<CRNVP, true, 3>   test_cm_trained_pass_vs_oracle, every case ("mfma" ids)
  tiled_pass_cm_kernel<CRNVP, true, 2>   ... [mfma_k2-*] (NFDPF_CM_K=2)
  tiled_pass_cm_kernel<CRNVP, false, 2>  ... [valu-*] (NFDPF_CM_MFMA=0): the control -- the harness
                                         favours neither measurement
  the MFMA step launch (filter_tiled.hip, NFDPF_PASS=0)   test_cm_trained_step_launch_vs_oracle
(A one-flow model: FilterEngine takes n_flows from its FilterConfig, not from the model's flow
list; the one-flow blob is checked by tests/test_crnvp_mfma_pack.py.)
"""
import os

import numpy as np
import pytest
import torch

import _fullsize as F
from oracle import dpf_oracle as O
from test_gpu_parity import _check_envelope
from test_gpu_pass import _Replay, _fractions
from test_gpu_pass_cm import _engine

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# the verified gates must be the float64 oracle's wherever its ESS is this far (relative) from 0.5 N
GATE_MARGIN = 1e-3


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from nfdpf import _lib
    _lib.load()
    assert torch.cuda.is_available()


def oracle_gates_off(wl, N, x0, logw0, noise):
    """The oracle on the workload ``wl`` with every gate held off, replaying ``noise`` [B, T, N, 2],
    in float32 and float64 -> {dtype: dict(x, p, noise, lik, idx, obs, pred, ess [T])}; ess is the
    reference's own expression, evaluated (not acted on) at every step."""
    c = F.cfg_dict(wl["flags"], N)
    w = {k: v.detach().float().cpu() for k, v in wl["models"].state_dict().items()}
    T = wl["enc"].shape[1]
    outs = {}
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    step = O.filter_step
    for dt in (torch.float32, torch.float64):
        ess = []

        def step_rec(*a, **k):
            r = step(*a, **k)
            ess.append(float(r["ess"]))
            return r
        O.filter_step = step_rec
        try:
            with O.precision(dt), torch.no_grad():
                r = O.filtering(c, O.cast_params(w, dt), wl["enc"].cpu().to(dt), wl["start"].cpu().to(dt),
                                wl["vel"].cpu().to(dt), rng=_Replay(noise), init=(x0.cpu().to(dt), logw0.cpu().to(dt)),
                                gates=[False] * T)
        finally:
            O.filter_step = step
        x, p = r[0].double(), r[1].double()
        outs[dt] = dict(x=x.numpy(), p=p.numpy(), noise=r[2], lik=r[3].double().numpy(), idx=r[5].numpy(),
                        obs=float(r[8]), pred=(x * p[..., None]).sum(2).numpy(), ess=np.asarray(ess))
    return outs


def _compare(tag, res, obs, r32, r64):
    """Index, noise, and the envelope of particles, weights, likelihood, prediction, obs-likelihood."""
    B, T, N = res.probs.shape
    ident = (torch.arange(N) + N * torch.arange(B)[:, None])[:, None, :].expand(B, T, N)
    assert torch.equal(res.index.cpu(), ident), "the gates-off pass resamples nothing"
    np.testing.assert_array_equal(r32["idx"], ident.numpy())
    assert torch.equal(res.noise.cpu(), r32["noise"]), "the oracle replayed other noise"
    print(f"\n{tag}: max |lik| {np.abs(r64['lik']).max():.3e}, oracle ESS / N "
          f"{' '.join(f'{e / N:.3f}' for e in r64['ess'])}")
    for what, ours, key, rtol, atol in (("particles", res.particles, "x", 1e-5, 1e-4),
                                        ("weights", res.probs, "p", 1e-5, 1e-9),
                                        ("likelihood", res.lik, "lik", 1e-5, 2e-5),
                                        ("prediction", res.pred, "pred", 1e-5, 1e-4)):
        ours = ours.cpu().double().numpy()
        assert np.isfinite(ours).all(), what
        _fractions(what, ours, r32[key], r64[key], 1e-5, 0.0)
        _check_envelope(ours, r32[key], r64[key], rtol, atol, what)
    o64 = r64["obs"]
    print(f"  obs-likelihood: ours {float(obs):.6e}, float32 {r32['obs']:.6e}, float64 {o64:.6e}")
    assert abs(float(obs) - o64) <= 4 * abs(r32["obs"] - o64) + 1e-5 * abs(o64) + 1e-4


VARIANTS = {"mfma": {}, "mfma_k2": {"NFDPF_CM_K": "2"}, "valu": {"NFDPF_CM_MFMA": "0"}}
SHAPES = {  # id: (B, N, T, scale) -- the smallest shapes at which each mechanism can break
    "4x1000x7-full": (4, 1000, 7, "c3_full"),  # a C3 row of 4 tiles; every K = 3 wave runs >= 2 steps; T % 3 = 1
    "4x1000x7-mid": (4, 1000, 7, "c3_mid"),
    # one full wave + one particle, three particle groups idle; a one-tile row through the global
    # granules (the MFMA kernel compiles the LDS exchange out); T % 3 = 2
    "3x65x5-full": (3, 65, 5, "c3_full"),
    "3x257x2-mid": (3, 257, 2, "c3_mid"),      # a second tile of one particle; T < K: the k = 2 waves only normalise
    "2x1024x1-full": (2, 1024, 1, "c3_full"),  # maximum N; T = 1: no chain, the k = 1 waves normalise the only slot
    "2x2x4-full": (2, 2, 4, "c3_full"),        # minimum N: 62 invalid MFMA columns per wave
    "3x300x6-mid": (3, 300, 6, "c3_mid"),      # T % 3 = 0; a ragged second tile
}
CASES = [("mfma", s) for s in SHAPES] + [(v, s) for v in ("mfma_k2", "valu") for s in ("4x1000x7-full", "4x1000x7-mid",
                                                                                      "3x65x5-full")]


@pytest.mark.parametrize("variant,shape", CASES, ids=[f"{v}-{s}" for v, s in CASES])
def test_cm_trained_pass_vs_oracle(variant, shape, monkeypatch):
    """The raw one-launch C3 pass (gates speculated off, unverified) against the gates-off oracle.

    Index and noise exact; particles, weights, the shifted likelihood and the prediction sum p x
    inside the float32 oracle's own error envelope against float64 (test_gpu_parity.
    _check_envelope: 4x max, 2.5x mean, 16x row, with test_cm_pass_vs_oracle's rtol / atol); the
    obs-likelihood as there.  The gates the pass's epilogue evaluates must be the float64
    oracle's ``ess < 0.5 N`` at every step whose ESS is at least 1e-3 (relative) away from
    0.5 N -- and for N >= 3 every step must be (the workloads are fixed so that the oracle alone
    meets this; at N = 2 a collapsed row has ESS = 1 = 0.5 N exactly, so only step 0's gate is
    compared).  finish_pending then reports "fired" exactly when an oracle gate is on, and never
    a hand-off fault (a timed-out pass must not pass for a result)."""
    from nfdpf import ops
    from nfdpf.engine import FilterEngine
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    B, N, T, scale = SHAPES[shape]
    wl = F.workload(scale, B=B, N=N, T=T)
    models = wl["models"].to(DEV)
    enc, start, vel = wl["enc"].to(DEV), wl["start"].to(DEV), wl["vel"].to(DEV)
    x0, logw0 = ops.particle_init(start[:, :2], B, N, 128.0, False, 5, 0, DEV)
    eng = _engine(models, N, 5)
    assert eng._meas_mfma() == (variant != "valu")
    res = eng.run(enc, start, vel, init=(x0, logw0), speculate=True, finish=False)
    torch.cuda.synchronize()
    assert eng.pass_launches == 1 and eng.last_pass, "the one-launch C3 pass did not run"
    pending = eng.take_pending()
    st = FilterEngine.pending_pass_state(pending)
    gates = st["gates"].cpu().numpy().astype(bool)
    assert st["flags"][2] == 1 and st["flags"][1] == 0, f"pass flags {st['flags']}"
    assert st["parts"].shape[:2] == (T, B) and bool(torch.isfinite(st["parts"]).all())
    outs = oracle_gates_off(wl, N, x0, logw0, res.noise)
    r32, r64 = outs[torch.float32], outs[torch.float64]
    _compare(f"C3 pass ({variant}) vs gates-off oracle, B={B} N={N} T={T} {scale}", res, st["obs"], r32, r64)
    want = r64["ess"] < 0.5 * N
    clear = np.abs(r64["ess"] - 0.5 * N) >= GATE_MARGIN * 0.5 * N
    print(f"  gates: ours {gates.astype(int).tolist()}, oracle {want.astype(int).tolist()}, closest ESS to 0.5 N "
          f"{np.abs(r64['ess'] / (0.5 * N) - 1).min():.3f} relative")
    if N >= 3:
        assert clear.all(), "a step's oracle ESS lies within the margin of 0.5 N: choose another workload seed"
    else:
        clear[1:] = False
    np.testing.assert_array_equal(gates[clear], want[clear])
    ok = eng.finish_pending(pending)
    assert eng.last_verify != "fault"
    if N >= 3:
        assert (ok, eng.last_verify) == ((False, "fired") if want.any() else (True, "ok"))
    else:
        assert (ok, eng.last_verify) == ((False, "fired") if gates.any() else (True, "ok"))


@pytest.mark.parametrize("N,scale", [(65, "c3_full"), (1000, "c3_full"), (65, "c3_mid"), (1000, "c3_mid")])
def test_cm_trained_step_launch_vs_oracle(N, scale, monkeypatch):
    """The MFMA step launch (filter_tiled.hip's step kernels with crnvp_lik_mfma, NFDPF_PASS=0)
    at T = 1 -- step 0's gate is always off, uniform weights -- against the same oracle: one
    ragged wave pair (65) and a full C3 row (1000).

    At c3_full this is the check of the step launches' softmax partials: formed from
    log p + the RAW likelihood (~ -2e3) they were rounded at that magnitude and a collapsed row's
    top weight came out 1 +- 4e-4 (weights max err 4.1e-04 against the float32 oracle's 1.6e-05);
    tiled_prop_kernel now forms them relative to the wave's max raw likelihood, as the pass."""
    from nfdpf import ops
    monkeypatch.setenv("NFDPF_PASS", "0")
    B, T = 3, 1
    wl = F.workload(scale, B=B, N=N, T=T)
    models = wl["models"].to(DEV)
    enc, start, vel = wl["enc"].to(DEV), wl["start"].to(DEV), wl["vel"].to(DEV)
    x0, logw0 = ops.particle_init(start[:, :2], B, N, 128.0, False, 5, 0, DEV)
    eng = _engine(models, N, 5)
    assert eng._meas_mfma()
    res = eng.run(enc, start, vel, init=(x0, logw0))
    torch.cuda.synchronize()
    assert eng.pass_launches == 0 and not eng.last_pass, "the step launches did not run"
    outs = oracle_gates_off(wl, N, x0, logw0, res.noise)
    _compare(f"MFMA step launch vs oracle, B={B} N={N} T={T} {scale}", res, res.obs_likelihood,
             outs[torch.float32], outs[torch.float64])
