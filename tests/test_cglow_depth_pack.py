"""CPU: the CGLOW parameter blob at flow depth K > 1 (nfdpf.pack.cglow_tensors, csrc/cglow.hpp):
K steps in model order, step k at k * 7980 floats in the K = 1 per-step layout; a pure gather
(blob_source_index is a permutation into the packed parameters); and the gates above it
(CondGlowModel.kernel_supported, nfdpf_cglow_params_size) take K in 1..4 and nothing else.
Weights: the reference's K = 2, 3 models (tests/golden/cglow_depth.npz)."""
import os

import pytest
import torch

from _util import assert_close, group, load, t, weights

KSTEP = 7980


def _model(K, L=1):
    from arguments import parse_args
    from nf.cglow.CGlowModel import CondGlowModel
    a = parse_args([])
    a.flow_depth, a.num_levels = K, L
    return CondGlowModel(a)


def _fixture_model(K):
    m = _model(K)
    sd = m.state_dict()
    w = weights(group(load("cglow_depth.npz"), f"k{K}"))
    assert set(w) == set(sd), sorted(set(w) ^ set(sd))[:5]
    m.load_state_dict(w)
    return m


def _blob(m):
    from nfdpf.pack import cglow_tensors
    return torch.cat([t.detach().reshape(-1) for t in cglow_tensors(m)])


@pytest.mark.parametrize("K", [2, 3])
def test_blob_is_k_single_step_blobs(K):
    m = _fixture_model(K)
    b = _blob(m)
    assert b.numel() == K * KSTEP
    sd = m.state_dict()
    for k in range(K):
        one = _model(1)
        # step k is flow.layers[1 + k] (layers[0] is the squeeze); a K = 1 model holds it at layers[1]
        src = {n.replace(f"flow.layers.{1 + k}.", "flow.layers.1."): v for n, v in sd.items()
               if n.startswith(f"flow.layers.{1 + k}.")}
        assert src
        osd = one.state_dict()
        assert set(src) <= set(osd)
        osd.update(src)
        one.load_state_dict(osd)
        assert torch.equal(b[k * KSTEP:(k + 1) * KSTEP], _blob(one)), f"step {k}"


@pytest.mark.parametrize("K", [2, 3])
def test_blob_source_index_is_a_permutation(K):
    from nfdpf.pack import blob_param_grads, blob_source_index, cglow_tensors
    m = _fixture_model(K)
    packed = [p for n, p in m.named_parameters() if n not in ("new_mean", "new_logs")]
    idx = blob_source_index(packed, lambda get: cglow_tensors(m, get))
    n = sum(p.numel() for p in packed)
    assert n == K * KSTEP and idx.numel() == n
    assert torch.equal(torch.sort(idx)[0], torch.arange(n))
    # and the gather it describes is the packing
    flat = torch.cat([p.detach().reshape(-1) for p in packed])
    assert torch.equal(flat[idx], _blob(m))
    # a blob-layout gradient scatters back to every packed parameter, None for the top Gaussian's
    grads = blob_param_grads(m, "glow_grad", list(m.parameters()), lambda get: cglow_tensors(m, get), _blob(m))
    for (name, p), g in zip(m.named_parameters(), grads):
        if name in ("new_mean", "new_logs"):
            assert g is None
        else:
            assert torch.equal(g, p.detach()), name


@pytest.mark.parametrize("K", [2, 3])
def test_torch_restatement_matches_reference(K):
    """CondGlowModel.torch_forward (what tests/test_gpu_cglow_depth.py compares the K = 4 kernel
    against) is the reference's K-step forward: the bounds of test_cglow_torch at K = 1."""
    fx = group(load("cglow_depth.npz"), f"k{K}")
    with torch.no_grad():
        z, nll = _fixture_model(K).torch_forward(t(fx["x"]), t(fx["y"]))
    assert_close(z, fx["z"], 1e-6, 1e-6, "z")
    assert_close(nll, fx["nll"], 1e-6, 1e-6, "nll")


def test_kernel_supported_depths():
    for K in (1, 2, 3, 4):
        assert _model(K).kernel_supported(), K
    assert not _model(5).kernel_supported()
    assert not _model(1, L=2).kernel_supported()
    assert not _model(2, L=2).kernel_supported()


def test_pack_rejects_depth_5():
    from nfdpf.pack import cglow_tensors
    with pytest.raises(ValueError, match="1..4"):
        cglow_tensors(_model(5))


def test_params_size_by_depth():
    from nfdpf import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libnfdpf.so is not built")
    lib = _lib.load()
    for K in (1, 2, 3, 4):
        assert int(lib.nfdpf_cglow_params_size(K)) == K * KSTEP
    for K in (0, 5, -1):
        assert int(lib.nfdpf_cglow_params_size(K)) == -1
    # the workspace of the K-step backward: K = 1 is the single-step size, bad K refused
    assert int(lib.nfdpf_cglow_backward_workspace_k(100, 1)) == int(lib.nfdpf_cglow_backward_workspace(100))
    assert int(lib.nfdpf_cglow_backward_workspace_k(100, 3)) > int(lib.nfdpf_cglow_backward_workspace(100))
    for K in (0, 5):
        assert int(lib.nfdpf_cglow_backward_workspace_k(100, K)) == -1
