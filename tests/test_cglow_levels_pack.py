"""CPU: the parameter blob of the CGLOW levels kernel (nfdpf.pack.cglow_levels_tensors,
csrc/cglow_levels.hpp) -- K level-1 steps in cglow_tensors' layout, at L = 2 the Split2d conv and
K level-2 steps of 21 168 floats, with learn_top the tail [new_mean | new_logs]; a pure gather;
the gates above it (CondGlowModel.levels_kernel_supported, nfdpf_cglow_levels_params_size); and
the PyTorch restatement the GPU tests lean on, against the reference's own L = 2 / learn_top runs
(tests/golden/cglow_levels.npz, cglow_levels_top.npz; written by tests/golden/gen_cglow_levels.py)."""
import os

import pytest
import torch

from _util import assert_close, group, load, t, weights

KSTEP, KSPLIT, KSTEP2 = 7980, 660, 21168
CONFIGS = [(1, 2, False), (2, 2, True), (1, 1, True), (1, 2, True)]  # the fixtures' (K, L, learn_top)


def _size(K, L, top):
    return K * KSTEP + (KSPLIT + K * KSTEP2 if L == 2 else 0) + (2 * (96 if L == 2 else 192) if top else 0)


def _model(K, L=1, top=False):
    from arguments import parse_args
    from nf.cglow.CGlowModel import CondGlowModel
    a = parse_args([])
    a.flow_depth, a.num_levels, a.learn_top = K, L, top
    return CondGlowModel(a)


def _fx(K, L, top):
    name = "cglow_levels_top.npz" if (K, L, top) == (1, 2, True) else "cglow_levels.npz"
    return group(load(name), f"k{K}l{L}t{int(top)}")


def _fixture_model(K, L, top):
    m = _model(K, L, top)
    w = weights(_fx(K, L, top))
    assert set(w) == set(m.state_dict()), sorted(set(w) ^ set(m.state_dict()))[:5]
    m.load_state_dict(w)
    return m


def _blob(m):
    from nfdpf.pack import cglow_levels_tensors
    return torch.cat([a.detach().reshape(-1) for a in cglow_levels_tensors(m)])


def test_parameter_counts():
    """The issue's counts: 30 000 = 7 980 + 660 + 21 168 + 192 at (1, 2, on), 59 148 at K = 2."""
    assert sum(p.numel() for p in _model(1, 2, True).parameters()) == 30000 == _size(1, 2, True)
    assert sum(p.numel() for p in _model(2, 2, True).parameters()) == 59148 == _size(2, 2, True)


@pytest.mark.parametrize("K,L,top", CONFIGS)
def test_blob_sizes_and_tail(K, L, top):
    m = _fixture_model(K, L, top)
    b = _blob(m)
    assert b.numel() == _size(K, L, top)
    if top:
        n = m.new_mean.numel()
        assert n == (96 if L == 2 else 192)
        assert torch.equal(b[-2 * n:-n], m.new_mean.detach().reshape(-1))
        assert torch.equal(b[-n:], m.new_logs.detach().reshape(-1))


@pytest.mark.parametrize("K,L,top", [(1, 2, False), (2, 2, True)])
def test_level1_part_is_cglow_tensors(K, L, top):
    """The first K * 7980 floats are cglow_tensors of the same steps loaded into an L = 1 model;
    then the Split2d conv tap-major ([kh][kw][in][out]) and its bias."""
    from nfdpf.pack import cglow_tensors
    m = _fixture_model(K, L, top)
    b = _blob(m)
    one = _model(K, 1)
    sd = one.state_dict()
    src = {n: v for n, v in m.state_dict().items() if n in sd and n not in ("new_mean", "new_logs")}
    assert len(src) == len(sd) - 2  # layers 0 .. K are the squeeze and the level-1 steps in both
    sd.update(src)
    one.load_state_dict(sd)
    assert torch.equal(b[:K * KSTEP], torch.cat([a.detach().reshape(-1) for a in cglow_tensors(one)]))
    conv = m.flow.layers[1 + K].conv[0]
    assert tuple(conv.weight.shape) == (12, 6, 3, 3)
    assert torch.equal(b[K * KSTEP:K * KSTEP + 648], conv.weight.detach().permute(2, 3, 1, 0).reshape(-1))
    assert torch.equal(b[K * KSTEP + 648:K * KSTEP + KSPLIT], conv.bias.detach())


@pytest.mark.parametrize("K,L,top", CONFIGS)
def test_blob_source_index_is_a_permutation(K, L, top):
    from nfdpf.pack import blob_source_index, cglow_levels_tensors
    m = _fixture_model(K, L, top)
    packed = [p for n, p in m.named_parameters() if top or n not in ("new_mean", "new_logs")]
    names = [n for n, _ in m.named_parameters()]
    if L == 2:
        assert f"flow.layers.{1 + K}.conv.0.weight" in names  # the Split2d conv is among them
    idx = blob_source_index(packed, lambda get: cglow_levels_tensors(m, get))
    n = sum(p.numel() for p in packed)
    assert n == _size(K, L, top) and idx.numel() == n
    assert torch.equal(torch.sort(idx)[0], torch.arange(n))
    flat = torch.cat([p.detach().reshape(-1) for p in packed])
    assert torch.equal(flat[idx], _blob(m))


def test_levels_kernel_supported():
    for K in (1, 2, 3, 4):
        for L in (1, 2):
            for top in (False, True):
                m = _model(K, L, top)
                assert m.levels_kernel_supported(), (K, L, top)
                # kernel_supported keeps its meaning: the single-level kernel without learn_top
                assert m.kernel_supported() == (L == 1 and not top), (K, L, top)
    assert not _model(5).levels_kernel_supported()
    assert not _model(5, 2).levels_kernel_supported()
    assert not _model(1, 3).levels_kernel_supported()
    assert not _model(1, 3).kernel_supported()


def test_pack_rejects_what_the_kernel_does_not_take():
    from nfdpf.pack import cglow_levels_tensors
    with pytest.raises(ValueError, match="1..4"):
        cglow_levels_tensors(_model(5))
    with pytest.raises(ValueError, match="1..2"):
        cglow_levels_tensors(_model(1, 3))


def test_dpf_refuses_three_levels():
    from arguments import parse_args
    from DPFs import DPF
    from nfdpf._lib import NfdpfError
    a = parse_args([])
    a.measurement, a.hiddensize, a.num_levels = "CGLOW", 192, 3
    with pytest.raises(NfdpfError, match="1..2"):
        DPF(a)


def test_params_size():
    from nfdpf import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libnfdpf.so is not built")
    lib = _lib.load()
    for K in (1, 2, 3, 4):
        for L in (1, 2):
            for top in (0, 1):
                assert int(lib.nfdpf_cglow_levels_params_size(K, L, top)) == _size(K, L, bool(top))
        assert int(lib.nfdpf_cglow_levels_params_size(K, 1, 0)) == int(lib.nfdpf_cglow_params_size(K))
    for K, L in ((0, 1), (5, 1), (-1, 2), (1, 0), (1, 3), (5, 3)):
        assert int(lib.nfdpf_cglow_levels_params_size(K, L, 0)) == -1
    for K, L, top in CONFIGS:
        assert int(lib.nfdpf_cglow_levels_params_size(K, L, int(top))) == _blob(_model(K, L, top)).numel()


@pytest.mark.parametrize("K,L,top", CONFIGS)
def test_torch_restatement_matches_reference(K, L, top):
    """CondGlowModel.torch_forward is the reference's forward at L = 2 / learn_top (the bounds of
    test_cglow_depth_pack): tests/test_gpu_cglow_levels.py compares the kernel with it."""
    fx = _fx(K, L, top)
    with torch.no_grad():
        z, nll = _fixture_model(K, L, top).torch_forward(t(fx["x"]), t(fx["y"]))
    assert tuple(z.shape) == fx["z"].shape == ((37, 24, 2, 2) if L == 2 else (37, 12, 4, 4))
    assert_close(z, fx["z"], 1e-6, 1e-6, "z")
    assert_close(nll, fx["nll"], 1e-6, 1e-6, "nll")
