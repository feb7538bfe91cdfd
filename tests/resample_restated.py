"""torchaudio.functional.resample (sinc_interp_hann / sinc_interp_kaiser), restated from its published implementation as test infrastructure.

torchaudio is not available to this project; this is the oracle the GPU resampler (audiolm-pytorch_amd/resample.py + csrc/resample.hip) is checked
against, written independently of the product (nothing here imports it).  `dtype` selects the float type the table and the correlation run in:
fp32 is torchaudio's path for an fp32 input, fp64 the high-precision yardstick.
"""
import math

import torch
import torch.nn.functional as F

KAISER_BETA = 14.769656459379492


def geometry(orig, new, lw=6, rolloff=0.99):
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    base = min(o, n) * rolloff
    W = math.ceil(lw * o / base)
    return o, n, W, 2 * W + o


def table(orig, new, lw=6, rolloff=0.99, method='sinc_interp_hann', beta=None, dtype=torch.float32):
    """K [n, T] in `dtype`, the operations in torchaudio's order"""
    o, n, W, _ = geometry(orig, new, lw, rolloff)
    base = min(o, n) * rolloff
    idx = torch.arange(-W, W + o, dtype=dtype)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=dtype)[:, None, None] / n + idx
    t *= base
    t = t.clamp_(-lw, lw)
    if method == 'sinc_interp_hann':
        window = torch.cos(t * math.pi / lw / 2) ** 2
    else:
        b = torch.tensor(float(KAISER_BETA if beta is None else beta))
        window = torch.i0(b * torch.sqrt(1 - (t / lw) ** 2)) / torch.i0(b)
    t *= math.pi
    scale = base / o
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kernels *= window * scale
    return kernels[:, 0]


def out_len(L, orig, new):
    o, n, _, _ = geometry(orig, new)
    return (n * L + o - 1) // o


def resample(x, orig, new, lw=6, rolloff=0.99, method='sinc_interp_hann', beta=None, dtype=torch.float32):
    """x [..., L] (CPU) -> [..., ceil(n L / o)] in `dtype`: pad (W, W + o), conv1d with stride o, phases interleaved, truncated"""
    if int(orig) == int(new):
        return x
    o, n, W, _ = geometry(orig, new, lw, rolloff)
    K = table(orig, new, lw, rolloff, method, beta, dtype)
    lead, L = x.shape[:-1], x.shape[-1]
    w = x.reshape(-1, L).to(dtype)
    w = F.pad(w, (W, W + o))
    y = F.conv1d(w[:, None], K[:, None], stride=o)
    y = y.transpose(1, 2).reshape(w.shape[0], -1)[..., :(n * L + o - 1) // o]
    return y.reshape(*lead, y.shape[-1])
