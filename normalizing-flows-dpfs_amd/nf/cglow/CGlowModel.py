"""Conditional GLOW (nf/cglow/CGlowModel.py of the reference): same modules and state_dict
keys (flow.layers.{k}...., new_mean, new_logs), same forward / reverse API.

``CondGlowModel.forward(x, y)`` -- the likelihood the DPF's CGLOW measurement evaluates (squeeze
-> K x [cond-actnorm, cond-1x1 conv with a per-sample 12x12 slogdet, cond-affine coupling] ->
Gaussian log-prob, CGlowModel.py:167-176) -- runs as one HIP kernel (csrc/cglow.hip,
nfdpf_cglow_flow) for the configuration the reference's flags give (K in 1..4, L = 1, x_size =
y_size = (3, 8, 8), learn_top off) and returns the reference's (z, nll); with L = 2 (Split2d and
a second level on 24 x 2 x 2) and / or learn_top it runs as one launch of csrc/cglow_levels.hip
(nfdpf_cglow_levels_flow); at the other hidden sizes of csrc/cglow_widths.hpp
(--x_hidden_channels / --x_hidden_size / --y_hidden_channels) or another --y_bins as one launch of
csrc/cglow_wide.hip (nfdpf_cglow_wide_flow), forward only.  --x_bins is not read, as in the
reference.  Under autograd the backward is the HIP one: csrc/cglow_bwd.hip at
L = 1 without learn_top, csrc/cglow_levels_bwd.hip at L = 2 and / or with learn_top; at the
sizes and bins of csrc/cglow_wide.hip it is the PyTorch recompute below.  With
NFDPF_HIP_BACKWARD=0 it differentiates ``torch_forward`` instead, a PyTorch restatement of the
same math run on the saved inputs (nfdpf.autograd; the forward value is the kernel's).
``reverse=True`` (sampling; the DPF never calls it) runs the layers' PyTorch reverse."""
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from nf.cglow import modules
from nfdpf import autograd as _ag
from nfdpf._lib import NfdpfError


class CondGlowStep(nn.Module):
    def __init__(self, x_size, y_size, x_hidden_channels, x_hidden_size, y_hidden_channels):
        super().__init__()
        self.actnorm = modules.CondActNorm(x_size=x_size, y_channels=y_size[0], x_hidden_channels=x_hidden_channels,
                                           x_hidden_size=x_hidden_size)
        self.invconv = modules.Cond1x1Conv(x_size=x_size, x_hidden_channels=x_hidden_channels,
                                           x_hidden_size=x_hidden_size, y_channels=y_size[0])
        self.affine = modules.CondAffineCoupling(x_size=x_size, y_size=[y_size[0] // 2, y_size[1], y_size[2]],
                                                 hidden_channels=y_hidden_channels)

    def forward(self, x, y, logdet=None, reverse=False):
        """actnorm -> 1x1 conv -> affine coupling, or the reverse chain (CGlowModel.py:24-54)."""
        stages = (self.actnorm, self.invconv, self.affine)
        for st in (reversed(stages) if reverse else stages):
            y, logdet = st(x, y, logdet, reverse=reverse)
        return y, logdet


class CondGlow(nn.Module):
    def __init__(self, x_size, y_size, x_hidden_channels, x_hidden_size, y_hidden_channels, K, L):
        super().__init__()
        self.layers = nn.ModuleList()
        self.output_shapes = []
        self.K, self.L = K, L
        C, H, W = y_size
        for level in range(L):
            C, H, W = C * 4, H // 2, W // 2
            self.layers.append(modules.SqueezeLayer(factor=2))
            self.output_shapes.append([-1, C, H, W])
            for _ in range(K):
                self.layers.append(CondGlowStep(x_size, [C, H, W], x_hidden_channels, x_hidden_size,
                                                y_hidden_channels))
                self.output_shapes.append([-1, C, H, W])
            if level < L - 1:
                self.layers.append(modules.Split2d(num_channels=C))
                self.output_shapes.append([-1, C // 2, H, W])
                C = C // 2

    def forward(self, x, y, logdet=0.0, reverse=False, eps_std=1.0):
        """encode (squeeze / steps / split in order) or decode (reversed), CGlowModel.py:98-120."""
        if not reverse:
            for layer in self.layers:
                if isinstance(layer, (modules.Split2d, modules.SqueezeLayer)):
                    y, logdet = layer(y, logdet, reverse=False)
                else:
                    y, logdet = layer(x, y, logdet, reverse=False)
            return y, logdet
        for layer in reversed(self.layers):
            if isinstance(layer, modules.Split2d):
                y, logdet = layer(y, logdet=logdet, reverse=True, eps_std=eps_std)
            elif isinstance(layer, modules.SqueezeLayer):
                y, logdet = layer(y, logdet=logdet, reverse=True)
            else:
                y, logdet = layer(x, y, logdet=logdet, reverse=True)
        return y, logdet


class HipKernel(NamedTuple):
    """What CondGlowModel.hip_kernel() answers: the HIP kernel that takes the model, and what a
    caller needs to use it.  ``kwargs`` go to every op; the backward ops are None where the
    kernel has no HIP backward."""
    name: str                      # "cglow" | "levels" | "wide": csrc/cglow.hip, cglow_levels.hip, cglow_wide.hip
    blob_key: str                  # the nfdpf.pack.blob cache key of the packed parameters
    pack: Callable                 # nfdpf.pack.cglow_tensors | cglow_levels_tensors
    measurement: Callable          # nfdpf.ops.cglow*_measurement
    flow: Callable                 # nfdpf.ops.cglow*_flow
    kwargs: dict                   # K; and L, learn_top; and widths, y_bins -- as the kernel takes them
    measurement_backward: Optional[Callable] = None
    flow_backward: Optional[Callable] = None

    def blob(self, owner, model, device):
        """The model's packed parameters on ``device``, cached on ``owner`` under blob_key."""
        from nfdpf.pack import blob
        return blob(owner, self.blob_key, model, lambda: self.pack(model), device)

    def param_grads(self, owner, model, g_blob):
        """The blob-layout gradient g_blob as the model's parameter gradients."""
        from nfdpf.pack import blob_param_grads
        return blob_param_grads(owner, self.blob_key + "_grad", list(model.parameters()),
                                lambda get: self.pack(model, get), g_blob)


class _FlowRunner:
    """nfdpf.autograd runner of CondGlowModel.forward on the kernel ``kern`` (a HipKernel): the
    HIP forward; the HIP backward where the kernel has one (csrc/cglow_bwd.hip, or
    csrc/cglow_levels_bwd.hip inside the configurations it is built for); else, and with
    NFDPF_HIP_BACKWARD=0, the PyTorch recompute of torch_forward, which is general in L,
    learn_top, the sizes and y_bins.  The wide kernel's recompute is bounded to RECOMPUTE_ROWS
    samples like the measurement form's (model.models._CglowRunner)."""

    RECOMPUTE_ROWS = 16384

    def __init__(self, model, kern):
        self.model, self.kern = model, kern
        # (nfdpf.autograd reads the attribute: None is "unbounded")
        self.recompute_limit = (lambda x, y: (self.RECOMPUTE_ROWS, x.shape[0])) if kern.name == "wide" else None

    def hip(self, x, y):
        m, k = self.model, self.kern
        return k.flow(k.blob(m, m, x.device), x, y, **k.kwargs)

    def torch(self, x, y):
        return self.model.torch_forward(x, y)

    def hip_backward(self, x, y, gouts):
        """d/d(x, y, parameters) on the kernel's flow backward; None (recompute) where it has none."""
        m, k = self.model, self.kern
        if k.flow_backward is None or tuple(x.shape[1:]) != (3, 8, 8) or tuple(y.shape) != tuple(x.shape):
            return None
        g_z, g_nll = gouts
        gx, gy, g_glow = k.flow_backward(k.blob(m, m, x.device), x, y, g_z, g_nll, **k.kwargs)
        return (gx, gy), k.param_grads(m, m, g_glow)


class CondGlowModel(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.flow = CondGlow(x_size=args.x_size, y_size=args.y_size, x_hidden_channels=args.x_hidden_channels,
                             x_hidden_size=args.x_hidden_size, y_hidden_channels=args.y_hidden_channels,
                             K=args.flow_depth, L=args.num_levels)
        self.learn_top = args.learn_top
        shp = self.flow.output_shapes[-1]
        self.register_parameter("new_mean", nn.Parameter(torch.zeros([1, shp[1], shp[2], shp[3]])))
        self.register_parameter("new_logs", nn.Parameter(torch.zeros([1, shp[1], shp[2], shp[3]])))
        self.n_bins = args.y_bins

    def prior(self):
        """(mean, logs) of the top Gaussian: learnt when learn_top, else zeros (:161-166)."""
        if self.learn_top:
            return self.new_mean, self.new_logs
        return torch.zeros_like(self.new_mean), torch.zeros_like(self.new_mean)

    def hidden_sizes(self):
        """(x_hidden_channels, x_hidden_size, y_hidden_channels) the model was built with (its first step's)."""
        st = next(l for l in self.flow.layers if isinstance(l, CondGlowStep))
        lin = [m for m in st.actnorm.x_Linear if isinstance(m, nn.Linear)]
        return lin[0].in_features, lin[0].out_features, st.affine.f[0].out_channels

    def hip_kernel(self) -> Optional[HipKernel]:
        """THE kernel choice: the HIP kernel that takes this model, or None.  x and y are 3x8x8 and
        K is in 1..4 for all three; then
        cglow   csrc/cglow.hip: the reference's defaults (arguments.py:61-70): L = 1, learn_top
                off, 256 bins, hidden 8 / 16 / 8;
        levels  csrc/cglow_levels.hip: L in 1..2, any learn_top, 256 bins, hidden 8 / 16 / 8;
        wide    csrc/cglow_wide.hip: L in 1..2, any learn_top, hidden sizes in the set of
                csrc/cglow_widths.hpp (every combination of x_hidden_channels in {8, 16},
                x_hidden_size in {16, 32}, y_hidden_channels in {8, 16, 32}), any finite y_bins > 0.
        x_bins is not read, as in the reference."""
        from nfdpf import ops
        from nfdpf._lib import cglow_widths_supported
        from nfdpf.pack import cglow_levels_tensors, cglow_tensors
        f = self.flow
        if not (1 <= f.K <= 4 and 1 <= f.L <= 2
                and list(f.output_shapes[-1][1:]) == ([12, 4, 4] if f.L == 1 else [24, 2, 2])):
            return None
        nb, widths = float(self.n_bins), self.hidden_sizes()
        levels = dict(K=f.K, L=f.L, learn_top=self.learn_top)
        if nb == 256.0 and widths == (8, 16, 8):
            if f.L == 1 and not self.learn_top:
                return HipKernel("cglow", "glow", cglow_tensors, ops.cglow_measurement, ops.cglow_flow, dict(K=f.K),
                                 ops.cglow_measurement_backward, ops.cglow_flow_backward)
            bwd = ops.cglow_levels_backward_supported(f.K, f.L)  # (what csrc/cglow_levels_bwd.hip is built for)
            return HipKernel("levels", "glow_levels", cglow_levels_tensors, ops.cglow_levels_measurement,
                             ops.cglow_levels_flow, levels, ops.cglow_levels_measurement_backward if bwd else None,
                             ops.cglow_levels_flow_backward if bwd else None)
        if np.isfinite(nb) and nb > 0 and cglow_widths_supported(*widths):
            return HipKernel("wide", "glow_levels", cglow_levels_tensors, ops.cglow_wide_measurement,
                             ops.cglow_wide_flow, dict(levels, widths=widths, y_bins=self.n_bins))
        return None

    def kernel_supported(self) -> bool:
        """The configuration csrc/cglow.hip is built for (hip_kernel: cglow)."""
        k = self.hip_kernel()
        return k is not None and k.name == "cglow"

    def levels_kernel_supported(self) -> bool:
        """The configurations csrc/cglow_levels.hip is built for (hip_kernel: levels, and cglow's,
        which it takes as well)."""
        k = self.hip_kernel()
        return k is not None and k.name in ("cglow", "levels")

    def wide_kernel_supported(self) -> bool:
        """The configurations csrc/cglow_wide.hip is built for: every one that has a kernel (the
        default sizes at 256 bins are in its set; cglow.hip / cglow_levels.hip run them)."""
        return self.hip_kernel() is not None

    def forward(self, x=0.0, y=None, eps_std=1.0, reverse=False):
        """reverse=False: (z, nll) of y given the condition x (CGlowModel.py:167-176), on the
        HIP kernel: csrc/cglow.hip at L = 1 without learn_top, csrc/cglow_levels.hip at L = 2
        and / or with learn_top (z is the final z, [M, 24, 2, 2] at L = 2), csrc/cglow_wide.hip
        at hidden sizes other than 8 / 16 / 8 or y_bins other than 256.
        reverse=True: a sample (or the inverse of a given y) and its log-det
        (:178-184), PyTorch (off the DPF path)."""
        if reverse:
            with torch.no_grad():
                mean, logs = self.prior()
                if y is None:
                    y = modules.GaussianDiag.batchsample(x.size(0), mean, logs, eps_std)
                return self.flow(x, y, eps_std=eps_std, reverse=True)
        kern = self.hip_kernel()
        if kern is None:
            raise NfdpfError("CondGlowModel.forward: the HIP kernels are built for K in 1..4, L in 1..2, 3x8x8 "
                             "inputs, x_hidden_channels in {8, 16}, x_hidden_size in {16, 32}, y_hidden_channels "
                             "in {8, 16, 32} and finite y_bins > 0")
        runner = _FlowRunner(self, kern)
        z, nll = _ag.apply(runner, (x.float().contiguous(), y.float().contiguous()), list(self.parameters()))
        return z, nll

    def torch_forward(self, x, y):
        """The PyTorch restatement of forward (CGlowModel.py:167-176) -- the backward of the
        kernel path differentiates this on the saved inputs."""
        dims = y.size(1) * y.size(2) * y.size(3)
        logdet = torch.zeros_like(y[:, 0, 0, 0]) + float(-np.log(self.n_bins) * dims)
        z, obj = self.flow(x, y, logdet=logdet, reverse=False)
        mean, logs = self.prior()
        obj = obj + modules.GaussianDiag.logp(mean, logs, z)
        return z, -obj / float(np.log(2.0) * dims)
