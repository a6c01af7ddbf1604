"""CPU: the one kernel choice of the conditional GLOW (CondGlowModel.hip_kernel): which of
csrc/cglow.hip, cglow_levels.hip and cglow_wide.hip takes a configuration, with the blob key, the
pack function, the ops and their keyword arguments the callers use; and that the three
predicates (kernel_supported, levels_kernel_supported, wide_kernel_supported) are the ladder
"cglow, else levels, else wide" over it."""
import pytest

DEFAULT = (8, 16, 8)


def _model(widths=DEFAULT, K=1, L=1, top=False, bins=256):
    from arguments import parse_args
    from nf.cglow.CGlowModel import CondGlowModel
    from nfdpf import _lib
    _lib.load()  # (cglow_widths_supported asks the library; no device)
    a = parse_args([])
    a.x_hidden_channels, a.x_hidden_size, a.y_hidden_channels = widths
    a.flow_depth, a.num_levels, a.learn_top, a.y_bins = K, L, top, bins
    return CondGlowModel(a)


def _ladder(m):
    """The kernel the callers' if / elif ladder over the three predicates names."""
    if m.kernel_supported():
        return "cglow"
    if m.levels_kernel_supported():
        return "levels"
    if m.wide_kernel_supported():
        return "wide"
    return None


CASES = [  # (model arguments, the kernel)
    (dict(K=1), "cglow"), (dict(K=2), "cglow"), (dict(K=3), "cglow"), (dict(K=4), "cglow"),
    (dict(top=True), "levels"),
    (dict(L=2), "levels"),
    (dict(L=2, top=True), "levels"),
    (dict(bins=32), "wide"),
    (dict(widths=(16, 32, 16)), "wide"),
    (dict(widths=(8, 16, 32), L=2), "wide"),
]


@pytest.mark.parametrize("kw,name", CASES, ids=[f"{n}-{'-'.join(f'{k}{v}' for k, v in kw.items())}" for kw, n in CASES])
def test_hip_kernel_names_the_ladders_kernel(kw, name):
    from nfdpf import ops
    from nfdpf.pack import cglow_levels_tensors, cglow_tensors
    m = _model(**kw)
    k = m.hip_kernel()
    assert k is not None and k.name == name == _ladder(m)
    # the predicates keep their meanings: cglow's configurations are the levels kernel's too, and
    # every configuration with a kernel is in the wide kernel's set
    assert m.kernel_supported() == (name == "cglow")
    assert m.levels_kernel_supported() == (name in ("cglow", "levels"))
    assert m.wide_kernel_supported()
    K, L, top = kw.get("K", 1), kw.get("L", 1), kw.get("top", False)
    if name == "cglow":
        assert (k.blob_key, k.pack) == ("glow", cglow_tensors)
        assert (k.measurement, k.flow) == (ops.cglow_measurement, ops.cglow_flow)
        assert (k.measurement_backward, k.flow_backward) == (ops.cglow_measurement_backward, ops.cglow_flow_backward)
        assert k.kwargs == dict(K=K)
    elif name == "levels":
        assert (k.blob_key, k.pack) == ("glow_levels", cglow_levels_tensors)
        assert (k.measurement, k.flow) == (ops.cglow_levels_measurement, ops.cglow_levels_flow)
        assert (k.measurement_backward, k.flow_backward) == (ops.cglow_levels_measurement_backward,
                                                             ops.cglow_levels_flow_backward)
        assert k.kwargs == dict(K=K, L=L, learn_top=top)
    else:
        assert (k.blob_key, k.pack) == ("glow_levels", cglow_levels_tensors)
        assert (k.measurement, k.flow) == (ops.cglow_wide_measurement, ops.cglow_wide_flow)
        assert k.measurement_backward is None and k.flow_backward is None
        assert k.kwargs == dict(K=K, L=L, learn_top=top, widths=kw.get("widths", DEFAULT), y_bins=kw.get("bins", 256))


@pytest.mark.parametrize("kw", [dict(widths=(8, 24, 8)), dict(L=3)], ids=["x_hidden_size24", "L3"])
def test_no_kernel(kw):
    m = _model(**kw)  # (the model builds: the refusal is the callers')
    assert m.hip_kernel() is None and _ladder(m) is None
