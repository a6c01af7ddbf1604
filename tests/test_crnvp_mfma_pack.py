"""The MFMA fragment blob of the CRNVP measurement (nfdpf.pack.crnvp_mfma_tensors) against the
oracle, on the CPU: a float64 emulator of crnvp_lik_mfma (csrc/crnvp_mfma.hpp) that reads
nothing but the blob -- the offsets restated below from the header's comments -- and follows the
kernel's documented data flow, compared with oracle.meas_crnvp in float64.

What it pins: the fragment order [M tile][lane][K step], the t / s hidden-row interleave, the
block-diagonal layers 2 and 3 (t outputs over K-steps 0-1, s outputs over K-steps 2-3), the
folded tanh constants and biases, one and two flows.  The GPU kernel's arithmetic is not run
here (tests/test_gpu_cm_trained.py does that); the emulator is its layout, in float64.
"""
import numpy as np
import pytest
import torch

from oracle import dpf_oracle as O

# ---- the blob's layout (floats), restated from csrc/crnvp_mfma.hpp's kCmf* comments ------------
EW1 = 0                      # encoder layer 1: W1 [16][2], then b1 [16] (plain)
EW2 = 48                     # layer 2: [2 MT][64][4]
EB2 = EW2 + 2 * 64 * 4       # [32]
EW3 = EB2 + 32               # layer 3: [2 MT][64][8]
EB3 = EW3 + 2 * 64 * 8       # [32]
ENC = EB3 + 32               # encoder floats
WC = 0                       # per coupling half: fold over e [64][8]
W1 = WC + 64 * 8             # layer 1 over u [64][4]
W2 = W1 + 64 * 4             # [64][4]
W3 = W2 + 64 * 4             # [2 MT][64][4]
B1 = W3 + 2 * 64 * 4         # [16]
B2 = B1 + 16                 # [16]
B3 = B2 + 16                 # [32]
HALF = B3 + 32

U32 = 2.0 ** -24             # unit roundoff of the blob's float32
# float64 evaluation (both sides) and the packer's float64 folding: every value is a dot product
# of at most 49 terms or one correctly-rounded-to-an-ulp function of one, gamma_n = n u / (1 - n u)
# of sum |w||x| each -- modelled as a further relative weight perturbation, twice (two sides)
G64 = 2 * 64 * 2.0 ** -53
LN2 = float(np.log(2.0))
LOG2E = 1.0 / LN2


def test_layout_constants_match_header():
    """The offsets above are the header's: the blob's length is kCmfEnc + 2 n_flows kCmfHalf
    (1648 + 3200 n_flows, the figures in its comments)."""
    assert (ENC, HALF) == (1648, 1600)
    for n in (1, 2):
        models = _models(n, None)
        assert sum(t.numel() for t in _blob_tensors(models)) == ENC + 2 * n * HALF


def _dense(frag, steps=None):
    """The matrix a fragment [MT][64][S] applies: the A operand of M tile MT, lane l, K-step s
    multiplies feature k(s, g) = 16 (s >> 2) + 4 g + (s & 3) (g = l >> 4) of the previous layer
    into output row 16 MT + (l & 15).  ``steps``: the K-steps the kernel issues (all by default)."""
    MT, L, S = frag.shape
    assert L == 64
    w = np.zeros((16 * MT, 4 * S))
    for mt in range(MT):
        for l in range(64):
            g = l >> 4
            for s in (range(S) if steps is None else steps):
                w[16 * mt + (l & 15), 16 * (s >> 2) + 4 * g + (s & 3)] += frag[mt, l, s]
    return w


class _Val:
    """A batch of activations with a bound on their error: v [..., K], d >= |v - exact|."""

    def __init__(self, v, d=None):
        self.v, self.d = v, np.zeros_like(v) if d is None else d


def _linear(w, b, x, u):
    """y = W x + b with every entry of W and b off by at most u relative (the blob's rounding):
    |W^ x^ - W x| <= |W^| dx + |W^ - W| |x|, |W^ - W| <= u1 |W^|, |x| <= |x^| + dx."""
    u1 = u / (1.0 - u)
    aw = np.abs(w)
    y = x.v @ w.T + b
    d = x.d @ aw.T + u1 * ((np.abs(x.v) + x.d) @ aw.T + np.abs(b))
    return _Val(y, d)


def _relu(x):
    return _Val(np.maximum(x.v, 0.0), x.d)  # 1-Lipschitz


def _sig_r(y):
    """r = 1 / (1 + 2^y), |r'| = ln 2 r (1 - r), largest at the point of [y - d, y + d] nearest 0;
    and r in (0, 1), so no error exceeds 1."""
    with np.errstate(over="ignore"):  # (2^y = inf: r = 0, the saturated unit)
        r = 1.0 / (1.0 + np.exp2(y.v))
        y0 = np.maximum(np.abs(y.v) - y.d, 0.0)
        r0 = 1.0 / (1.0 + np.exp2(y0))
    return _Val(r, np.minimum(LN2 * r0 * (1.0 - r0) * y.d, 1.0))


def emulate(blob, n_flows, prior_std, enc, x, u=U32 + G64):
    """crnvp_lik_mfma's data flow in float64 on the blob (float32 values, held exactly).
    enc [R, 32], x [R, P, 2] -> (raw likelihood [R, P], a bound on |it - the exact-weight value|
    [R, P], where the blob's entries carry at most ``u`` relative error each)."""
    W = np.asarray(blob, dtype=np.float64)
    R, P, _ = x.shape
    # encoder: layer 1 plain, layers 2 and 3 fragments
    h = _relu(_linear(W[EW1:EW1 + 32].reshape(16, 2), W[EW1 + 32:EW1 + 48], _Val(x.astype(np.float64)), u))
    h = _relu(_linear(_dense(W[EW2:EB2].reshape(2, 64, 4)), W[EB2:EB2 + 32], h, u))
    e = _linear(_dense(W[EW3:EB3].reshape(2, 64, 8)), W[EB3:EB3 + 32], h, u)
    encb = np.broadcast_to(enc.astype(np.float64)[:, None, :], (R, P, 32))
    lo, up = _Val(encb[..., :16].copy()), _Val(encb[..., 16:].copy())
    ld = _Val(np.zeros((R, P)))
    for f in range(n_flows):
        for n in range(2):
            H = W[ENC + (2 * f + n) * HALF:ENC + (2 * f + n + 1) * HALF]
            uu, vv = (lo, up) if n == 0 else (up, lo)
            # fold over e + layer 1 over u: one accumulator, 12 K-steps
            w1 = np.concatenate([_dense(H[WC:W1].reshape(1, 64, 8)), _dense(H[W1:W2].reshape(1, 64, 4))], 1)
            eu = _Val(np.concatenate([e.v, uu.v], -1), np.concatenate([e.d, uu.d], -1))
            hh = _sig_r(_linear(w1, H[B1:B1 + 16], eu, u))
            hh = _sig_r(_linear(_dense(H[W2:W3].reshape(1, 64, 4)), H[B2:B2 + 16], hh, u))
            a3 = H[W3:B1].reshape(2, 64, 4)
            t = _linear(_dense(a3[0:1], steps=(0, 1)), H[B3:B3 + 16], hh, u)       # t: K-steps 0-1
            s = _linear(_dense(a3[1:2], steps=(2, 3)), H[B3 + 16:B3 + 32], hh, u)  # s: K-steps 2-3
            es = np.exp2(s.v * LOG2E)
            # |v^ e^s^ - v e^s| <= e^s^ dv + (|v^| + dv) e^s^ (e^ds - 1)
            nd = t.d + es * vv.d + (np.abs(vv.v) + vv.d) * es * np.expm1(s.d)
            vv.v, vv.d = t.v + vv.v * es, nd
            ld = _Val(ld.v + s.v.sum(-1), ld.d + s.d.sum(-1))
    z = _Val(np.concatenate([lo.v, up.v], -1), np.concatenate([lo.d, up.d], -1))
    m = ((z.v / prior_std) ** 2).sum(-1)
    md = (z.d * (2 * np.abs(z.v) + z.d)).sum(-1) / prior_std ** 2  # |z^2 - z'^2| <= dz (2 |z| + dz)
    lp = -0.5 * (32 * np.log(2 * np.pi) + m) - 32 * np.log(prior_std)
    return lp + ld.v, 0.5 * md + ld.d


def _models(n_flows, stds, seed=0):
    """(particle encoder, cnf_measurement with n_flows flows) on the CPU; stds = (encoder std,
    flow std) for a seeded N(0, std^2) draw of every parameter as tests/_fullsize does, or None:
    the reference init (default Linear encoder, flows N(0, 0.01^2))."""
    from model.models import build_conditional_nf, build_particle_encoder
    torch.manual_seed(100 + seed)
    pe = build_particle_encoder(32, 2).cpu()
    cnf = build_conditional_nf(n_flows, 32, 32, prior_std=2.5).cpu()
    if stds is not None:
        g = torch.Generator().manual_seed(200 + seed)
        with torch.no_grad():
            for mod, std in ((pe, stds[0]), (cnf.flows, stds[1])):
                for p in mod.parameters():
                    p.copy_(torch.randn(p.shape, generator=g) * std)
    return pe, cnf


def _blob_tensors(models):
    from nfdpf.pack import crnvp_mfma_tensors
    pe, cnf = models
    return crnvp_mfma_tensors(pe, list(cnf.flows))


def _points(P=300, R=3, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(R, P, 2, generator=g) * 128.0 - 64.0
    edge = torch.tensor([[-64.0, -64.0], [-64.0, 64.0], [64.0, -64.0], [64.0, 64.0], [0.0, 0.0]])
    x = torch.cat([x, edge[None].expand(R, -1, -1)], 1)
    return x, g


def _oracle64(models, n_flows, enc, x):
    pe, cnf = models
    with O.precision(torch.float64):
        pp = O.cast_params({k: v.detach() for k, v in pe.state_dict().items()}, torch.float64)
        cp = O.cast_params({k: v.detach() for k, v in cnf.state_dict().items()}, torch.float64)
        with torch.no_grad():
            return O.meas_crnvp(pp, cp, n_flows, enc.double(), x.double(), prior_std=2.5).numpy()


# the reference init; the c3_full scales (tests/_fullsize.CASES: encoder 0.5, measurement flows
# 0.1); flows at 0.5: every tanh saturated
SCALES = {"init": None, "c3_full": (0.5, 0.1), "saturated": (0.5, 0.5)}


def _swap_t_s_rows(blob, n_flows):
    """The blob with the t and s hidden rows of the first coupling half's layer 1 exchanged
    (output rows 4 j + {0, 1} <-> 4 j + {2, 3} of the fold, of layer 1 over u and of b1): what a
    packer with pt and ps swapped there would write.  Output row p is lane column l & 15."""
    b = blob.copy()
    lane = np.arange(64)
    src = (lane & ~3) | ((lane & 3) ^ 2)  # (bits 0-1 of the lane are bits 0-1 of its column)
    for off, S in ((WC, 8), (W1, 4)):
        v = b[ENC + off:ENC + off + 64 * S].reshape(64, S)
        b[ENC + off:ENC + off + 64 * S] = v[src].reshape(-1)
    b[ENC + B1:ENC + B1 + 16] = b[ENC + B1:ENC + B1 + 16][src[:16]]
    return b


def _transpose_fragment(blob, n_flows):
    """The blob with the last coupling half's layer-2 fragment [64 lanes][4 K-steps] written
    [K step][lane]: a wrong fragment order."""
    b = blob.copy()
    o = ENC + (2 * n_flows - 1) * HALF + W2
    b[o:o + 256] = b[o:o + 256].reshape(64, 4).T.reshape(-1)
    return b


@pytest.mark.parametrize("n_flows", [1, 2])
@pytest.mark.parametrize("scale", list(SCALES))
def test_mfma_blob_matches_oracle(scale, n_flows):
    """The emulator on the blob == oracle.meas_crnvp (float64) on the modules' own weights.
    meas_crnvp subtracts the row's maximum, the raw value of the row's best particle k (where
    it returns 0): the same particle's raw value is subtracted from the emulator's row.

    Bound (derived; no measured constant).  The packer folds in float64 and rounds once to
    float32, so every blob entry w^ = w (1 + delta), |delta| <= 2^-24 =: u; the emulator holds w^
    exactly and computes in float64.  Carrying d >= |a^ - a| for every activation a:
      linear   d_y = |W^| d_x + u/(1-u) (|W^| (|x^| + d_x) + |b^|)   -- the measured sum |w||x|
      relu     d unchanged (1-Lipschitz)
      r form   d_r = min(1, ln2 r0 (1 - r0) d_y), r0 = r at the point of [y^ - d_y, y^ + d_y] nearest 0
      coupling d_v' = d_t + e^s^ d_v + (|v^| + d_v) e^s^ (e^d_s - 1);  d_logdet += sum d_s
      prior    d_lp = sum d_z (2 |z^| + d_z) / (2 prior_std^2)
    through the encoder's three layers and 2 n_flows coupling halves of three layers each, giving
    D_i >= |lik^_i - lik_i| per particle.  The float64 rounding of both evaluations (dot products
    of <= 49 terms: gamma_64 = 64 2^-53 of the same sum |w||x|, on two sides) enters as a further
    1.4e-14 on u.  With particle k's value subtracted on both sides,
        |(lik^_i - lik^_k) - (lik_i - lik_k)| <= D_i + D_k.
    The bound is a worst case over the signs of ~4.5 k roundings and holds per particle: it is
    loose (the observed error is printed beside it), and where a coupling multiplies |v| ~ 1e3
    by e^s it is looser still -- the function is that ill-conditioned there (saturated weights).

    Negative controls, in the same test: the t and s hidden rows of a coupling half's layer 1
    exchanged (what swapping pt and ps there writes), and one fragment transposed, must each
    miss the oracle by more than 100 x this bound at some particle -- the emulator follows the
    layout, and the two sides do not simply share code (the oracle reads the state dict, the
    emulator the blob)."""
    models = _models(n_flows, SCALES[scale])
    blob = torch.cat([t.reshape(-1) for t in _blob_tensors(models)]).numpy()
    assert blob.dtype == np.float32 and blob.size == ENC + 2 * n_flows * HALF
    x, g = _points()
    R = x.shape[0]
    with torch.no_grad():  # frame encodings near the particle encoder's own range, as _fullsize's
        enc = models[0](torch.rand(R, 2, generator=g) * 100.0 - 50.0)
        enc = enc + 0.3 * enc.abs().mean() * torch.randn(enc.shape, generator=g)
    ref = _oracle64(models, n_flows, enc, x)
    assert np.isfinite(ref).all()

    k = ref.argmax(-1)[:, None]  # the row's best particle: meas_crnvp's shift is its raw value
    assert np.all(np.take_along_axis(ref, k, -1) == 0.0)

    def shifted(b):
        with np.errstate(over="ignore"):
            lik, D = emulate(b, n_flows, 2.5, enc.numpy(), x.numpy())
        return lik - np.take_along_axis(lik, k, -1), D + np.take_along_axis(D, k, -1), lik

    ours, bound, raw = shifted(blob)
    err = np.abs(ours - ref)
    print(f"\nmfma blob vs oracle ({scale}, {n_flows} flow(s)): max |raw lik| {np.abs(raw).max():.3e}, "
          f"max err {err.max():.3e}, bound median {np.median(bound):.3e} max {bound.max():.3e}, "
          f"worst err / bound {(err / bound).max():.2e}")
    assert np.all(err <= bound), f"worst excess {(err - bound).max():.3e} at err / bound {(err / bound).max():.3f}"
    for what, wrong in (("t/s rows swapped", _swap_t_s_rows), ("fragment transposed", _transpose_fragment)):
        bad, _, _ = shifted(wrong(blob, n_flows))
        miss = np.abs(bad - ref) / bound
        print(f"  control ({what}): max err {np.abs(bad - ref).max():.3e}, worst err / bound {miss.max():.3e}")
        assert miss.max() > 100.0, f"control ({what}) not detected: worst err / bound {miss.max():.3e}"
