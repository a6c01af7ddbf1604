"""Helpers shared by the frame-encoder tests (test_frame_encoder_pack.py, test_gpu_frame_encoder.py)."""
import torch
from torch import nn


def stack(H, seed=11):
    """model.models._conv_stack(H) with its default initialisation under ``seed``."""
    import model.models as mm
    torch.manual_seed(seed)
    return mm._conv_stack(H)


def trained_like(enc, seed=12):
    """Give every BatchNorm statistics as after training -- gamma ~ U(0.5, 1.5), beta ~ N(0, 0.2^2),
    running_mean ~ U(0, 0.5), running_var ~ U(0.5, 2) -- in place.  The fresh module's mean 0 /
    var 1 / gamma 1 / beta 0 would hide a wrong fold."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in enc:
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.empty(m.num_features).uniform_(0.5, 1.5, generator=g))
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                m.running_mean.copy_(torch.empty(m.num_features).uniform_(0.0, 0.5, generator=g))
                m.running_var.copy_(torch.empty(m.num_features).uniform_(0.5, 2.0, generator=g))
    return enc


def device_blob(enc, device):
    """The module's parameter blob (nfdpf.pack.frame_encoder_tensors) on ``device``."""
    from nfdpf.pack import frame_encoder_tensors
    return torch.cat([t.reshape(-1).float() for t in frame_encoder_tensors(enc)]).to(device)
