"""CPU-side checks for the levels backward (csrc/cglow_levels_bwd.hip): the scatter that takes a
gradient in the levels blob's layout back to the parameters is the inverse of the gather that
packed them, and the new entry points' ctypes signatures load and validate without a device."""
import pytest
import torch


def _model(K, L, top):
    from arguments import parse_args
    from nf.cglow.CGlowModel import CondGlowModel
    a = parse_args([])
    a.flow_depth, a.num_levels, a.learn_top = K, L, top
    torch.manual_seed(K * 10 + L)
    return CondGlowModel(a)


@pytest.mark.parametrize("K,L,top", [(1, 2, True), (2, 2, False), (1, 1, True)])
def test_blob_param_grads_inverts_the_levels_gather(K, L, top):
    """A blob-shaped tensor of distinct values lands on exactly the parameters the gather read,
    element for element; a parameter the blob does not pack gets None."""
    from nfdpf.pack import blob_param_grads, cglow_levels_tensors
    m = _model(K, L, top)
    params = list(m.parameters())
    with torch.no_grad():  # distinct values everywhere: the gather of them names every source
        off = 0
        for p in params:
            p.copy_(torch.arange(off, off + p.numel(), dtype=torch.float32).view(p.shape))
            off += p.numel()
    assert off < 2 ** 24  # exact in float32
    packed = torch.cat([t.detach().reshape(-1) for t in cglow_levels_tensors(m)])
    n = K * 7980 + (660 + K * 21168 if L == 2 else 0) + (2 * (96 if L == 2 else 192) if top else 0)
    assert packed.numel() == n
    g_blob = packed + 0.5  # distinct, and tied to the source element's own value
    grads = blob_param_grads(m, "t", params, lambda get: cglow_levels_tensors(m, get), g_blob)
    assert len(grads) == len(params)
    used = 0
    for (name, p), g in zip(m.named_parameters(), grads):
        if name in ("new_mean", "new_logs") and not top:
            assert g is None, name
            continue
        assert g is not None and g.shape == p.shape, name
        assert torch.equal(g, p.detach() + 0.5), name
        used += p.numel()
    assert used == n  # a pure gather: every blob entry has one source and every source one entry


def test_levels_backward_signatures_load_and_validate():
    from nfdpf import _lib
    lib = _lib.load()
    for s in ("nfdpf_cglow_levels_backward_workspace", "nfdpf_cglow_levels_measurement_backward",
              "nfdpf_cglow_levels_flow_backward"):
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
    q = lib.nfdpf_cglow_levels_backward_workspace
    assert q(0, 1, 1) > 0 and q(1000, 3, 1) > q(1000, 1, 1) > 5 * 1000 * 192 * 4
    assert q(1000, 1, 2) > q(1000, 1, 1) + 2 * 1000 * 96 * 4
    for M, K, L in ((-1, 1, 1), (16, 0, 1), (16, 5, 1), (16, 1, 0), (16, 1, 3)):
        assert q(M, K, L) == -1, (M, K, L)
    # the range checks come before any pointer is read: EINVAL, nothing launched
    for K, L in ((5, 1), (1, 3), (1, 0)):
        rc = lib.nfdpf_cglow_levels_flow_backward(None, K, L, None, None, None, 16, None, None, None, None, None, None,
                                                  None)
        assert rc == _lib.NFDPF_EINVAL
        msg = lib.nfdpf_last_error()
        assert b"1..4" in msg and b"1..2" in msg, msg
        rc = lib.nfdpf_cglow_levels_measurement_backward(None, None, K, L, None, None, 192, None, 32, 1, 16, None, 16,
                                                         None, None, None, None, None, None)
        assert rc == _lib.NFDPF_EINVAL
    rc = lib.nfdpf_cglow_levels_flow_backward(None, 1, 1, None, None, None, 16, None, None, None, None, None, None, None)
    assert rc == _lib.NFDPF_EINVAL and b"null" in lib.nfdpf_last_error()
