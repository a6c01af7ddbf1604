"""Frame-encoding widths (--hiddensize) of the measurement kernels, the parts that need no GPU:
the library's width query and refusals (nothing is launched for a width that is not built), the
construction-time check of DPF(args), and the CPU oracle against the reference's fixtures at
widths 16 and 64 (tests/golden/gen_meas_widths.py)."""
import ctypes

import pytest

from _util import assert_close, group, load, t, weights
from oracle import dpf_oracle as O


@pytest.mark.parametrize("E", [16, 64])
@pytest.mark.parametrize("meas", ["cos", "CRNVP", "NN", "gaussian"])
def test_oracle_matches_reference_at_width(meas, E):
    """The oracle is width-generic: the reference's own likelihoods at --hiddensize 16 / 64, at
    test_oracle_golden's tolerance."""
    fx = group(load("meas_widths.npz"), f"{meas}_{E}")
    w = weights(fx)
    enc, x = t(fx["enc"]), t(fx["x"])
    assert enc.shape == (3, E) and x.shape == (3, 40, 2)
    lik = O.make_measurement(dict(measurement=meas, n_flows=2), w)(enc, x)
    assert_close(lik, fx["lik"], 1e-5, 1e-5, f"{meas} E={E}")


def test_width_query():
    from nfdpf import _lib
    lib = _lib.load()
    for kind in ("cos", "CRNVP", "NN", "gaussian"):
        for E, ok in ((16, True), (32, True), (64, True), (24, False), (128, False), (0, False), (-16, False)):
            assert bool(lib.nfdpf_meas_width_supported(_lib.MEAS[kind], E)) is ok, (kind, E)
            assert _lib.meas_width_supported(kind, E) is ok
        assert _lib.meas_widths(kind) == [16, 32, 64]
    # the EXTERNAL "kind" has no kernel of its own, an unknown name none either
    assert not lib.nfdpf_meas_width_supported(_lib.MEAS_EXTERNAL, 32)
    assert not _lib.meas_width_supported("CGLOW", 192)


def test_unsupported_width_is_refused_before_any_launch():
    """E = 24 -> NFDPF_EINVAL with the built widths in the message, forward and backward entry
    points alike (no device is touched: the pointers are never dereferenced)."""
    from nfdpf import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = lib.nfdpf_measurement(_lib.MEAS["cos"], p, None, 2, p, p, 1, 2, 24, 2.5, p, None)
    assert rc == _lib.NFDPF_EINVAL
    msg = lib.nfdpf_last_error().decode()
    assert "24" in msg and "16 32 64" in msg, msg
    rc = lib.nfdpf_cos_measurement_backward(p, p, p, p, 1, 2, 24, p, p, p, p, None)
    assert rc == _lib.NFDPF_EINVAL and "16 32 64" in lib.nfdpf_last_error().decode()
    rc = lib.nfdpf_nn_measurement_backward(p, p, p, p, 1, 2, 24, p, p, p, p, None)
    assert rc == _lib.NFDPF_EINVAL and "16 32 64" in lib.nfdpf_last_error().decode()
    rc = lib.nfdpf_particle_encoder_e(0, p, p, 1, 2, 24, None, p, None, None, None, None)
    assert rc == _lib.NFDPF_EINVAL and "16 32 64" in lib.nfdpf_last_error().decode()
    assert lib.nfdpf_cos_measurement_backward_workspace_e(1, 2, 24) == -1
    assert lib.nfdpf_nn_measurement_backward_workspace_e(1, 2, 24) == -1


def test_gradient_sizes_follow_the_width():
    from nfdpf import _lib, ops
    lib = _lib.load()
    assert ops.encoder_param_count(32) == 1648 and ops.nn_head_param_count(32) == 8385
    for E in (16, 32, 64):
        nblk = 2  # N = 70: two 64-particle workgroups per row
        assert lib.nfdpf_cos_measurement_backward_workspace_e(3, 70, E) == 3 * nblk * (ops.encoder_param_count(E) + E) * 4
        assert lib.nfdpf_nn_measurement_backward_workspace_e(3, 70, E) == 3 * nblk * (ops.nn_head_param_count(E) + E) * 4
    assert lib.nfdpf_cos_measurement_backward_workspace_e(3, 70, 32) == lib.nfdpf_cos_measurement_backward_workspace(3, 70)
    assert lib.nfdpf_nn_measurement_backward_workspace_e(3, 70, 32) == lib.nfdpf_nn_measurement_backward_workspace(3, 70)


def test_cond_stack_backward_supported_query():
    """The CRNVP measurement's stack backward (dim = obser_dim = E): built at 16, 32 and 64; at 64
    the LDS bound (57344 + 32768 n_flows bytes <= 160 KB) holds up to three flows (the reference's
    n_sequence is 2) and refuses four."""
    from nfdpf import _lib
    lib = _lib.load()
    for E in (16, 32):
        assert all(lib.nfdpf_cond_stack_backward_supported(n, E, E, 8) for n in (1, 2, 3, 4))
    assert all(lib.nfdpf_cond_stack_backward_supported(n, 64, 64, 8) for n in (1, 2, 3))
    assert not lib.nfdpf_cond_stack_backward_supported(4, 64, 64, 8)
    assert not lib.nfdpf_cond_stack_backward_supported(2, 24, 24, 8)
    assert not lib.nfdpf_cond_stack_backward_supported(2, 32, 32, 16)
    assert not lib.nfdpf_cond_stack_backward_supported(5, 2, 4, 8)


@pytest.mark.parametrize("meas", ["cos", "CRNVP", "NN", "gaussian"])
def test_dpf_refuses_unsupported_width_at_construction(meas):
    from arguments import parse_args
    from DPFs import DPF
    from nfdpf._lib import NfdpfError
    a = parse_args([])
    a.measurement, a.hiddensize = meas, 24
    with pytest.raises(NfdpfError, match="16, 32, 64"):
        DPF(a)


def test_filter_desc_has_the_external_flag():
    """lik_ext_asis is the descriptor's last field and zero by default (today's row-max shift)."""
    from nfdpf import _lib
    assert _lib.FilterDesc._fields_[-1][0] == "lik_ext_asis"
    assert _lib.FilterDesc().lik_ext_asis == 0
