"""Graph replay of the C2 step launches (tiled_fdyn_kernel + tiled_prop_quad_kernel per step, the
one-launch pass switched off) on the C2 bench workload (B=64, N=1000, device RNG).  GPU box only.

This file used to compare the one-launch fused step (tiled_step_fused_kernel, NFDPF_FUSED_STEP=1)
with these two launches; that kernel is retired and its comparisons went with it.
What remains is the check that never depended on it:

* a captured pass replayed twice gives the same bits twice, and the bits of the pass launched
  from Python;
* no wave-pair hand-off gave up (the device fault counter stays 0).

The oracle parity of this path is covered by the rest of the GPU suite, which runs it for every
C2-shaped case (tests/test_gpu_parity*.py, tests/test_gpu_dpf_api.py).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FIELDS = ("particles", "probs", "lik", "index", "noise", "jac", "prior", "pred")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from nfdpf import _lib
    _lib.load()
    assert torch.cuda.is_available()


def _setup(T=12, B=64, N=1000):
    import bench
    from DPFs import DPF
    from nfdpf.engine import FilterEngine
    flags = dict(bench.CONFIGS["c2"][0])
    torch.manual_seed(2)
    a = bench.make_args(flags, B, N, T, {"force_resample": False})
    dpf = DPF(a).to(DEV).eval()
    start, state, vel, enc = (x.to(DEV) for x in bench.synthetic_disk(B, T, 2, a.hiddensize))
    return FilterEngine(dpf.filter_config(), dpf), (enc, start, vel)


def _run(eng, inputs, monkeypatch):
    from nfdpf import _lib
    monkeypatch.setenv("NFDPF_PASS", "0")  # the step launches (the one-launch pass would take over)
    res = eng.run(*inputs)
    torch.cuda.synchronize()
    assert not eng.last_fused
    assert _lib.lib().nfdpf_split_fault(1, _lib.stream_ptr(DEV)) == 0
    return {k: getattr(res, k).clone() for k in FIELDS}, float(res.obs_likelihood)


def test_fused_step_graph_replay(monkeypatch):
    monkeypatch.setenv("NFDPF_PASS", "0")
    eng, inp = _setup(T=8)
    eng.run(*inp)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = eng.run(*inp)
    outs = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        outs.append({k: getattr(res, k).clone() for k in FIELDS})
    ref, _ = _run(eng, inp, monkeypatch)
    for k in FIELDS:
        assert torch.equal(outs[0][k], outs[1][k]), k
        assert torch.equal(outs[0][k], ref[k]), k
    from nfdpf import _lib
    assert _lib.lib().nfdpf_split_fault(1, _lib.stream_ptr(DEV)) == 0
