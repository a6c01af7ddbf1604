"""The kernels' fp64 wave reduction (common.hpp wave_sum_dpp / wave_sum_dpp_n, behind the test
entry point nfdpf_wave_sum_dpp) against a NumPy evaluation in the same pairing order, bit for bit:
lane pairs (xor 1), quads (xor 2), the half-row mirror, the row mirror, then the four 16-lane rows
as (r0 + r16) + (r32 + r48).  Every lane must hold the wave's sum."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _reference(x):
    """x [..., 64] float64 -> the wave's sum in the kernels' order."""
    lane = np.arange(64)
    v = x.copy()
    v = v + v[..., lane ^ 1]
    v = v + v[..., lane ^ 2]
    v = v + v[..., (lane & ~7) | (7 - (lane & 7))]
    v = v + v[..., (lane & ~15) | (15 - (lane & 15))]
    return (v[..., 0] + v[..., 16]) + (v[..., 32] + v[..., 48])


def _inputs(B, K, seed):
    """float64 values drawn from float32, and their squares, over exponents -20 .. +20 (what the
    exchanges sum); zeros in masked lanes (lanes past N); a signed zero; one 1e30 outlier."""
    g = np.random.default_rng(seed)
    f = (g.standard_normal((B, K, 64)) * np.exp2(g.integers(-20, 21, (B, K, 64)))).astype(np.float32)
    x = f.astype(np.float64)
    x[:, 1::2] = x[:, 1::2] * x[:, 1::2]                      # odd values: squares (exact in f64)
    nv = g.integers(0, 65, B)                                 # valid lanes of the row's wave
    x[np.broadcast_to(np.arange(64)[None, None, :] >= nv[:, None, None], x.shape)] = 0.0
    x[0] = np.abs(x[0]) + 1.0                                 # a full wave of positive terms
    x[1, :, :] = 0.0
    x[1, :, 5] = -0.0                                         # zeros with one signed zero
    x[2, :, :] = -0.0                                         # all negative zeros: the sum is -0.0
    x[3, 0, 37] = 1e30                                        # the outlier swallows its row
    return x


@pytest.mark.parametrize("K", [1, 2, 4])
def test_wave_sum_dpp_equals_numpy_order(K):
    from nfdpf import _lib
    _lib.load()
    B = 48
    x = _inputs(B, K, seed=K)
    xd = torch.from_numpy(x).to(DEV).contiguous()
    out = torch.empty_like(xd)
    _lib.check(_lib.lib().nfdpf_wave_sum_dpp(xd.data_ptr(), B, K, out.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "wave_sum_dpp")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ref = _reference(x)
    assert np.signbit(ref[2]).all() and (ref[2] == 0).all()   # the reference keeps the sign of zero
    np.testing.assert_array_equal(got.view(np.int64), np.broadcast_to(ref[..., None], got.shape).copy().view(np.int64))
