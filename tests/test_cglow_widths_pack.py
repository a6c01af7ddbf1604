"""CPU: the conditional GLOW at the hidden sizes of csrc/cglow_widths.hpp (--x_hidden_channels XH
in {8, 16}, --x_hidden_size XS in {16, 32}, --y_hidden_channels YH in {8, 16, 32}) and at other
--y_bins: the blob sizes the width-general kernel (csrc/cglow_wide.hip) expects against
nfdpf.pack.cglow_levels_tensors, the gates above it (CondGlowModel.wide_kernel_supported, DPF's
refusal at construction), the argument checks of the new entry points, and the PyTorch
restatement the recompute backward differentiates, against the reference's own runs at these
sizes (tests/golden/cglow_widths.npz, cglow_widths_l2.npz; tests/golden/gen_cglow_widths.py)."""
import itertools

import pytest
import torch

from _util import assert_close, group, load, t, weights

TRIPLES = list(itertools.product((8, 16), (16, 32), (8, 16, 32)))
DEFAULT = (8, 16, 8)
# the fixtures: case -> (file, (XH, XS, YH), K, L, learn_top, y_bins)
CASES = {
    "a": ("cglow_widths.npz", (16, 32, 16), 1, 1, False, 256),
    "b": ("cglow_widths_l2.npz", (8, 16, 32), 2, 2, True, 256),
    "c": ("cglow_widths_l2.npz", (16, 32, 32), 1, 2, True, 256),
    "d": ("cglow_widths.npz", (8, 16, 8), 1, 1, False, 32),
    "e": ("cglow_widths.npz", (16, 16, 8), 1, 1, False, 256),
}


def _args(widths=DEFAULT, K=1, L=1, top=False, bins=256, **kw):
    from arguments import parse_args
    a = parse_args([])
    a.x_hidden_channels, a.x_hidden_size, a.y_hidden_channels = widths
    a.flow_depth, a.num_levels, a.learn_top, a.y_bins = K, L, top, bins
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _model(widths=DEFAULT, K=1, L=1, top=False, bins=256):
    from nf.cglow.CGlowModel import CondGlowModel
    return CondGlowModel(_args(widths, K, L, top, bins))


def _blob(m):
    from nfdpf.pack import cglow_levels_tensors
    return torch.cat([a.detach().reshape(-1) for a in cglow_levels_tensors(m)])


def _lib():
    from nfdpf import _lib
    return _lib.load()


def test_params_size_is_the_pack_length():
    lib = _lib()
    for widths in TRIPLES:
        assert int(lib.nfdpf_cglow_wide_supported(*widths)) == 1
        for K, L, top in ((1, 1, False), (2, 2, True)):
            n = int(lib.nfdpf_cglow_wide_params_size(K, L, int(top), *widths))
            assert n == _blob(_model(widths, K, L, top)).numel(), (widths, K, L, top)
    for (K, L, top, widths), n in (((1, 1, 0, (16, 32, 16)), 18300), ((1, 1, 0, (16, 16, 8)), 11548),
                                   ((2, 2, 1, (8, 16, 32)), 94476), ((1, 2, 1, (16, 32, 32)), 71696),
                                   ((1, 1, 0, DEFAULT), 7980)):
        assert int(lib.nfdpf_cglow_wide_params_size(K, L, top, *widths)) == n
    # the default sizes: the levels kernel's own counts
    for K, L, top in itertools.product((1, 4), (1, 2), (0, 1)):
        assert int(lib.nfdpf_cglow_wide_params_size(K, L, top, *DEFAULT)) == int(lib.nfdpf_cglow_levels_params_size(K, L, top))


def test_params_size_outside_the_set():
    lib = _lib()
    for widths in ((8, 24, 8), (4, 8, 4), (8, 16, 64), (32, 16, 8), (0, 16, 8)):
        assert int(lib.nfdpf_cglow_wide_supported(*widths)) == 0
        assert int(lib.nfdpf_cglow_wide_params_size(1, 1, 0, *widths)) == -1
    for K, L in ((5, 1), (0, 1), (1, 3), (1, 0)):
        assert int(lib.nfdpf_cglow_wide_params_size(K, L, 0, 16, 32, 16)) == -1


def test_kernel_gates():
    for widths in TRIPLES:
        for K, L, top in ((1, 1, False), (4, 2, True)):
            m = _model(widths, K, L, top)
            assert m.hidden_sizes() == widths
            assert m.wide_kernel_supported(), (widths, K, L, top)
            if widths != DEFAULT:
                assert not m.kernel_supported() and not m.levels_kernel_supported(), widths
    # unchanged on the default sizes
    assert _model().kernel_supported() and _model().levels_kernel_supported()
    assert not _model(top=True).kernel_supported() and _model(top=True).levels_kernel_supported()
    assert not _model(L=2).kernel_supported() and _model(L=2).levels_kernel_supported()
    # other bins: only the width-general kernel
    m = _model(bins=32)
    assert not m.kernel_supported() and not m.levels_kernel_supported() and m.wide_kernel_supported()
    for bad in (0, -4, float("inf"), float("nan")):
        assert not _model(bins=bad).wide_kernel_supported(), bad
    # outside the set, K, L
    assert not _model((8, 24, 8)).wide_kernel_supported()
    assert not _model((4, 8, 4)).wide_kernel_supported()
    assert not _model((16, 32, 16), K=5).wide_kernel_supported()
    assert not _model((16, 32, 16), L=3).wide_kernel_supported()


def test_dpf_refuses_sizes_outside_the_set_at_construction():
    from DPFs import DPF
    from nfdpf._lib import NfdpfError
    with pytest.raises(NfdpfError, match=r"8 / 24 / 8.*x_hidden_size in \[16, 32\]"):
        DPF(_args((8, 24, 8), measurement="CGLOW", hiddensize=192))
    dpf = DPF(_args((16, 32, 16), measurement="CGLOW", hiddensize=192, x_bins=7.0))  # (x_bins is not read)
    assert dpf._fused_supported()
    assert dpf.cglow_measurement.wide_kernel_supported() and not dpf.cglow_measurement.kernel_supported()


def test_forward_outside_every_kernel_raises_on_the_sizes():
    """The error names the sizes, before any device is touched."""
    from nfdpf._lib import NfdpfError
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(NfdpfError, match="x_hidden_size in"):
        _model((8, 24, 8))(x, x)


@pytest.mark.parametrize("case", sorted(CASES))
def test_torch_restatement_matches_reference(case):
    """CondGlowModel.torch_forward is the reference's forward at these sizes and bins (the float32
    bounds of test_cglow_torch.py): the recompute backward differentiates it, and
    tests/test_gpu_cglow_widths.py compares the kernel with it."""
    name, widths, K, L, top, bins = CASES[case]
    fx = group(load(name), case)
    assert [int(v) for v in fx["config"]] == list(widths) + [K, L, int(top), bins]
    m = _model(widths, K, L, top, bins)
    w = weights(fx)
    assert set(w) == set(m.state_dict())
    m.load_state_dict(w)
    assert _blob(m).numel() == int(_lib().nfdpf_cglow_wide_params_size(K, L, int(top), *widths))
    with torch.no_grad():
        z, nll = m.torch_forward(t(fx["x"]), t(fx["y"]))
    assert tuple(z.shape) == fx["z"].shape == ((37, 24, 2, 2) if L == 2 else (37, 12, 4, 4))
    assert_close(z, fx["z"], 1e-6, 1e-6, "z")
    assert_close(nll, fx["nll"], 1e-6, 1e-6, "nll")


def test_measurement_restatement_matches_reference():
    from DPFs import DPF
    fx = group(load("cglow_widths.npz"), "meas")
    dpf = DPF(_args((16, 32, 16), measurement="CGLOW", hiddensize=192, num_particles=21, batchsize=3))
    sd = dpf.state_dict()
    w = weights(fx)
    assert set(w) <= set(sd)
    sd.update(w)
    dpf.load_state_dict(sd)
    with torch.no_grad():
        raw = dpf.cpu().measurement_model.torch_forward_raw(t(fx["enc"]), t(fx["x"]))
    assert_close(raw - raw.max(-1, keepdim=True)[0], fx["lik"], 1e-6, 1e-6, "CGLOW likelihood")


def test_entry_points_check_their_arguments_without_a_device():
    """NFDPF_EINVAL with a message before anything is launched or any pointer read."""
    import ctypes
    from nfdpf import _lib as L
    lib = L.load()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ld0 = -1064.6740693
    ok = (16, 32, 16)

    def meas(pe=p, glow=p, K=1, Lv=1, enc=p, x=p, B=1, N=1, lik=p, widths=ok, ld=ld0):
        return lib.nfdpf_cglow_wide_measurement(pe, glow, K, Lv, None, enc, 192, x, 2, B, N, lik, 1, *widths, ld, None)

    def flow(glow=p, K=1, Lv=1, x=p, y=p, M=1, nll=p, widths=ok, ld=ld0):
        return lib.nfdpf_cglow_wide_flow(glow, K, Lv, None, x, y, M, None, nll, *widths, ld, None)

    for kw, word in ((dict(glow=None), b"null"), (dict(x=None), b"null"), (dict(K=5), b"1..4"), (dict(K=0), b"1..4"),
                     (dict(Lv=3), b"1..2"), (dict(Lv=0), b"1..2"), (dict(widths=(8, 24, 8)), b"x_hidden_size"),
                     (dict(widths=(4, 8, 4)), b"x_hidden_channels"), (dict(ld=float("-inf")), b"finite"),
                     (dict(ld=float("nan")), b"finite")):
        for fn in (meas, flow):
            assert fn(**kw) == L.NFDPF_EINVAL, (fn.__name__, kw)
            assert word in lib.nfdpf_last_error(), (fn.__name__, kw, lib.nfdpf_last_error())
    assert meas(lik=None) == L.NFDPF_EINVAL and meas(enc=None) == L.NFDPF_EINVAL and meas(pe=None) == L.NFDPF_EINVAL
    assert flow(nll=None) == L.NFDPF_EINVAL and flow(y=None) == L.NFDPF_EINVAL
    assert meas(B=-1) == L.NFDPF_EINVAL and meas(N=0) == L.NFDPF_EINVAL and flow(M=-1) == L.NFDPF_EINVAL
    # nothing to do: OK without a launch (and so without a device)
    assert meas(B=0) == L.NFDPF_OK and flow(M=0) == L.NFDPF_OK
