"""The speculative one-launch pass's row exchanges (A: x_phys sums, B: x_dyn sums) at the shapes
where their publish / sweep / context code takes another path, pinned bit for bit to the gated
pass's.

The exchanges' wave reductions (common.hpp wave_sum_dpp_n) are shared by every pass mode and the
step launches; the speculative pass publishes and sweeps them through its own code (the
pre-published A, the held fold weights).  The gated pass on a workload whose gate stays quiet takes
the speculative pass's arithmetic through the kModeGate code path, so equality of every returned
tensor shows that neither path changed a bit of an exchange; the step launches bound both from
outside.  (The file's name is the check a two-part publish of an exchange -- component 0's sums
ahead of component 1's, measured and not kept, DESIGN section 3 -- has to pass.)  (One flow per
stack is not covered: the e2e_c2 fixture's weights come as two-flow stacks.)"""
import pytest
import torch

from _util import assert_close
from test_gpu_pass import _inputs, _models, _run

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FIELDS = ("particles", "probs", "noise", "lik", "index", "jac", "prior", "pred", "obs_likelihood")

# (B, N, T): the minimum N; a wave with one valid lane (65); empty wave groups (100); a tile with
# one particle (257); the bench's tile count (1000); the maximum N (1024); T = 1 (no pre-published A)
SHAPES = [(1, 2, 1), (2, 65, 2), (3, 100, 3), (2, 257, 3), (2, 1000, 3), (1, 1024, 2)]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from nfdpf import _lib
    _lib.load()
    assert torch.cuda.is_available()


@pytest.fixture(scope="module")
def models():
    return _models("e2e_c2.npz")


@pytest.mark.parametrize("B,N,T", SHAPES)
def test_speculative_pass_exchanges(B, N, T, models, monkeypatch):
    enc, start, vel = _inputs(B, T, seed=B * 1000 + N)
    eng_s, s = _run(models, N, enc, start, vel, spec=True)
    assert eng_s.last_pass and not eng_s.last_gate_pass and eng_s.pass_launches == 1
    # determinism: a second speculative pass, bit for bit
    eng_2, s2 = _run(models, N, enc, start, vel, spec=True)
    assert eng_2.last_pass and not eng_2.last_gate_pass
    for f in FIELDS:
        assert torch.equal(getattr(s, f), getattr(s2, f)), f"second run: {f}"
    # the quiet gated pass (the kModeGate code path), bit for bit
    eng_g, g = _run(models, N, enc, start, vel, spec=False)
    assert eng_g.last_pass and eng_g.last_gate_pass
    assert int(eng_g.last_gates.sum()) == 0, "the gate fired on the e2e_c2 flows"
    for f in FIELDS:
        assert torch.equal(getattr(s, f), getattr(g, f)), f"gated pass: {f}"
    # the step launches, under test_pass_matches_step_launches's tolerances
    _, b = _run(models, N, enc, start, vel, spec=False, env="0", monkeypatch=monkeypatch)
    assert torch.equal(s.noise, b.noise)
    assert torch.equal(s.index, b.index)
    assert_close(s.particles.cpu(), b.particles.cpu(), 1e-5, 1e-4, "particles")
    assert_close(s.probs.cpu(), b.probs.cpu(), 1e-4, 1e-9, "weights")
    assert_close(s.lik.cpu(), b.lik.cpu(), 1e-4, 1e-5, "likelihood")
    assert_close(s.jac.cpu(), b.jac.cpu(), 1e-5, 1e-5, "jac")
    assert_close(s.prior.cpu(), b.prior.cpu(), 1e-5, 1e-4, "prior")
    assert_close(s.pred.cpu(), b.pred.cpu(), 1e-5, 1e-3, "prediction")
    assert abs(float(s.obs_likelihood) - float(b.obs_likelihood)) <= 1e-5 * abs(float(b.obs_likelihood)) + 1e-4
