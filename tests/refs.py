"""Plain double-precision references of the operations behind the C-ABI (include/adp.h), shared by the tests that
place operands themselves (test_operand_placement.py).  Everything here is torch on the CPU in float64; nothing calls
a kernel.  The mel spectrogram and the STFT loss have their restatements next to their own tests
(test_vocoder.mel_ref, test_stft_loss.mrstft_ref); they are imported from there, not repeated."""
import math

import torch
import torch.nn.functional as F


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def gn_stats(x, G, eps=1e-5):
    """[B, G, 2] = (mean, rstd) of each group, biased variance."""
    B = x.shape[0]
    xv = x.double().reshape(B, G, -1)
    return torch.stack([xv.mean(-1), (xv.var(-1, unbiased=False) + eps).rsqrt()], -1)


def gn_silu_as_given(x, G, gamma, beta, eps=1e-5):
    """SiLU(GroupNorm(x)) in the precision of its arguments (test_kernels.py passes float32 or float64)."""
    return F.silu(F.group_norm(x, G, gamma, beta, eps=eps))


def gn_silu(x, G, gamma, beta, eps=1e-5):
    return gn_silu_as_given(x.double(), G, gamma.double(), beta.double(), eps)


def ln_stats(x, eps=1e-5):
    """[B, L, 2] = (mean, rstd) over channels of x [B, C, L]."""
    xv = x.double()
    return torch.stack([xv.mean(1), (xv.var(1, unbiased=False) + eps).rsqrt()], -1)


def ln_chan(x, gamma=None, beta=None, eps=1e-5):
    """LayerNorm over the channels of [B, C, L]."""
    C = x.shape[1]
    g = gamma.double() if gamma is not None else None
    b = beta.double() if beta is not None else None
    return F.layer_norm(x.double().transpose(1, 2), (C,), g, b, eps=eps).transpose(1, 2)


def modulation(x, scale, shift, eps=1e-5):
    """LayerNorm over channels without affine, then * (1 + scale[b, c]) + shift[b, c]."""
    return ln_chan(x, eps=eps) * (1 + scale.double()[:, :, None]) + shift.double()[:, :, None]


def act(x, kind):
    return {0: lambda t: t, 1: F.silu, 2: F.gelu}[kind](x.double() if not x.requires_grad else x)


def conv_input(x, x2=None, prologue=0, stats_groups=8, gamma=None, beta=None, up=1):
    """Xv of adp_conv_desc before the zero padding: channel concat, prologue, nearest upsample."""
    a = x.double() if x2 is None else torch.cat([x.double(), x2.double()], 1)
    if prologue == 1:
        a = gn_silu(a, stats_groups, gamma, beta)
    elif prologue == 2:
        a = ln_chan(a, gamma, beta)
    if up > 1:
        a = a.repeat_interleave(up, dim=2)
    return a


def conv(a, w, *, stride=1, dil=1, pad=0, transposed=False):
    """sum_{r,t} A(m,r,t) a[b, r, n*stride + t*dil - pad] with A = w[m][r][t], or w[r][m][KT-1-t] when transposed."""
    wd = w.double()
    if transposed:
        wd = wd.transpose(0, 1).flip(2)
    return F.conv1d(a, wd.contiguous(), None, stride=stride, padding=pad, dilation=dil)


def conv_wgrad(a, dy, KT, *, stride=1, dil=1, pad=0):
    """(dw [M, R, KT], dbias [M]) of conv(a, w) for the output gradient dy; a = conv_input(...)."""
    M, R = dy.shape[1], a.shape[1]
    w = torch.zeros(M, R, KT, dtype=torch.float64, requires_grad=True)
    y = F.conv1d(a, w, None, stride=stride, padding=pad, dilation=dil)
    assert y.shape == dy.shape, (y.shape, dy.shape)
    (dw,) = torch.autograd.grad(y, w, dy.double())
    return dw, dy.double().sum((0, 2))


def gn_silu_bwd(x, dact, G, gamma, beta, eps=1e-5):
    """(dx, dgamma, dbeta, ds*xhat row sums, ds row sums) of SiLU(GroupNorm(x)) for the output gradient dact."""
    xd = x.double().requires_grad_()
    g, b = gamma.double().requires_grad_(), beta.double().requires_grad_()
    y = gn_silu(xd, G, g, b, eps)
    dx, dg, db = torch.autograd.grad(y, (xd, g, b), dact.double())
    B, C, L = x.shape
    st = gn_stats(x, G, eps)
    mean = st[..., 0].repeat_interleave(C // G, dim=1)[:, :, None]
    rstd = st[..., 1].repeat_interleave(C // G, dim=1)[:, :, None]
    xhat = (x.double() - mean) * rstd
    h = xhat * gamma.double()[None, :, None] + beta.double()[None, :, None]
    sig = torch.sigmoid(h)
    ds = dact.double() * sig * (1 + h * (1 - sig))
    return dx, dg, db, ds * xhat, ds


def attention(q, k, v, H, D):
    """q [B, H*D, n], k / v [B, H*D, m] -> (o [B, H*D, n], lse [B, H, n]); differentiable."""
    B, mid, n = q.shape
    m = k.shape[2]
    qh = q.reshape(B, H, D, n).transpose(2, 3)
    kh = k.reshape(B, H, D, m).transpose(2, 3)
    vh = v.reshape(B, H, D, m).transpose(2, 3)
    s = torch.einsum("bhnd,bhmd->bhnm", qh, kh) * D ** -0.5
    o = torch.einsum("bhnm,bhmd->bhnd", torch.softmax(s, dim=-1), vh).transpose(2, 3).reshape(B, mid, n)
    return o, torch.logsumexp(s, dim=-1)


def time_fourier(t, w):
    f = t.double()[:, None] * w[None, :] * 2 * math.pi
    return torch.cat([t.double()[:, None], f.sin(), f.cos()], -1)


def v_step(x, v, a0, b0, a1, b1):
    return a1 * (a0 * x.double() - b0 * v.double()) + b1 * (b0 * x.double() + a0 * v.double())


def resample(x, kern, fi, fo, width, out_len):
    """out[row, l*fo + k] = sum_j kern[k, j] * xpad[row, l*fi + j]; x [rows, length], kern [fo, J]."""
    xp = F.pad(x.double()[:, None], (width, width + fi))
    y = F.conv1d(xp, kern.double()[:, None], stride=fi)          # [rows, fo, l]
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :out_len]


def adamw(p, g, m, v, ema, *, clip, decay, one_minus_beta1, beta2, one_minus_beta2, inv_bc2_sqrt, eps, step_size,
          ema_weight):
    """One step of adp_adamw_step's recurrence on double tensors."""
    g = g * clip
    p = p * decay
    m = m + (g - m) * one_minus_beta1
    v = v * beta2 + one_minus_beta2 * g * g
    p = p - step_size * m / (v.sqrt() * inv_bc2_sqrt + eps)
    if ema is not None:
        ema = ema + ema_weight * (p - ema)
    return p, m, v, ema
