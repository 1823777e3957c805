"""fp64 references and seeded input builders for the trainable SigLIP tower (PatchEmbedFn, SiglipLayerFn, BilinearL2NormFn and the
LayerNorm / column-sum / bilinear kernels under them).  Plain torch on the CPU; nothing here calls project code.

Every builder rounds to bf16 before either side sees the values, so the kernels and the references start from the same numbers.
The hand-written backward formulas are checked against torch.autograd in tests/test_tower_refs_host.py.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
U = 2.0 ** -24                                               # unit roundoff of one fp32 operation (round to nearest)


def to_bf16(t):
    """fp64 / fp32 -> bf16 (through fp32, as a kernel's final store does)"""
    return t.to(torch.float32).to(BF16)


def bf16_step(t):
    """distance between neighbouring bf16 values at |t| (fp64): 2^(floor(log2 |t|) - 7); the smallest normal step below that"""
    a = t.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


# ------------------------------------------------------------------------------------------------ input builders

def siglip_like_rows(M, h, seed):
    """[M, h] bf16 rows shaped like a SigLIP residual stream: an N(0,1) base, about 0.5 % of the channels (at least one) scaled by
    30 .. 100 with a non-zero per-channel mean, about 1 % of the rows (at least one) shifted by +-20.
    Returns (rows, outlier channel indices, shifted row indices)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, h, generator=g, dtype=torch.float64)
    n_ch = max(1, round(0.005 * h))
    ch = torch.randperm(h, generator=g)[:n_ch]
    scale = 30.0 + 70.0 * torch.rand(n_ch, generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand(n_ch, generator=g) < 0.5, -1.0, 1.0).double()
    mean = sign * (10.0 + 30.0 * torch.rand(n_ch, generator=g, dtype=torch.float64))
    x[:, ch] = x[:, ch] * scale + mean
    n_r = max(1, round(0.01 * M))
    rows = torch.randperm(M, generator=g)[:n_r]
    rsign = torch.where(torch.rand(n_r, generator=g) < 0.5, -1.0, 1.0).double()
    x[rows] += 20.0 * rsign[:, None]
    return to_bf16(x), ch, rows


HOSTILE_KINDS = ("offset", "constant", "zero", "tiny", "one_spike")


def hostile_rows(kind, M, h):
    """[M, h] bf16 rows that stress the mean / variance arithmetic of a LayerNorm:
      offset     mean 100, standard deviation 0.1 (bf16 keeps steps of 0.5 there: most elements are exactly 100, a few 99.5 / 100.5)
      constant   every element of a row equal (a different, non-power-of-two value per row)
      zero       all zero
      tiny       N(0,1) * 1e-19 (the variance, 1e-38, is far below eps and below the smallest normal fp32)
      one_spike  N(0,1) with one element of 3e4 per row"""
    g = torch.Generator().manual_seed(1000 + HOSTILE_KINDS.index(kind))
    if kind == "offset":
        x = 100.0 + 0.1 * torch.randn(M, h, generator=g, dtype=torch.float64)
    elif kind == "constant":
        c = torch.tensor([(-1.0) ** r * (3.140625 + 1.71875 * r) for r in range(M)], dtype=torch.float64)
        x = c[:, None].expand(M, h).clone()
    elif kind == "zero":
        x = torch.zeros(M, h, dtype=torch.float64)
    elif kind == "tiny":
        x = 1e-19 * torch.randn(M, h, generator=g, dtype=torch.float64)
    elif kind == "one_spike":
        x = torch.randn(M, h, generator=g, dtype=torch.float64)
        x[torch.arange(M), (7 * torch.arange(M) + 3) % h] = 3e4
    else:
        raise ValueError(kind)
    return to_bf16(x)


def norm_params(h, seed):
    """LayerNorm weight N(1, 0.3) and bias N(0, 0.5), bf16"""
    g = torch.Generator().manual_seed(seed)
    w = 1.0 + 0.3 * torch.randn(h, generator=g, dtype=torch.float64)
    b = 0.5 * torch.randn(h, generator=g, dtype=torch.float64)
    return to_bf16(w), to_bf16(b)


def grad_rows_along(x, seed, eps=1e-6):
    """Upstream gradient for a LayerNorm backward over rows x: N(0,1) + a per-row mean of about 0.5 + 0.7 xhat, bf16.  With it the
    mean-subtraction terms mean(g) and mean(g xhat) of the backward pass are of the order of |g| itself."""
    g = torch.Generator().manual_seed(seed)
    M, h = x.shape
    _, xh, _ = layernorm_ref(x, torch.ones(h), torch.zeros(h), eps)
    row_mean = 0.5 + 0.1 * torch.randn(M, 1, generator=g, dtype=torch.float64)
    return to_bf16(torch.randn(M, h, generator=g, dtype=torch.float64) + row_mean + 0.7 * xh)


def rows_with_column_mean(M, N, seed):
    """[M, N] bf16, N(0,1) plus a per-column mean in +-2: column sums that do not cancel to noise"""
    g = torch.Generator().manual_seed(seed)
    mean = 4.0 * torch.rand(N, generator=g, dtype=torch.float64) - 2.0
    return to_bf16(torch.randn(M, N, generator=g, dtype=torch.float64) + mean)


# ------------------------------------------------------------------------------------------------ LayerNorm

def layernorm_ref(x, w, b, eps):
    """y = xhat * w + b in fp64 (two-pass mean / biased variance).  Returns (y, xhat, rstd [M, 1])."""
    x, w, b = x.double(), w.double(), b.double()
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    xh = d * rstd
    return xh * w + b, xh, rstd


def layernorm_bwd_ref(dy, x, w, eps, dres=None):
    """g = dy w;  dx = dres + rstd (g - mean(g) - xhat mean(g xhat));  dw = sum_r dy xhat;  db = sum_r dy.
    Returns (dx, dw, db, sum_r |dy xhat|, sum_r |dy|), all fp64."""
    dy = dy.double()
    _, xh, rstd = layernorm_ref(x, w, torch.zeros_like(w), eps)
    g = dy * w.double()
    sg = g.mean(-1, keepdim=True)
    sgx = (g * xh).mean(-1, keepdim=True)
    dx = rstd * (g - sg - xh * sgx)
    if dres is not None:
        dx = dx + dres.double()
    t = dy * xh
    return dx, t.sum(0), dy.sum(0), t.abs().sum(0), dy.abs().sum(0)


# ------------------------------------------------------------------------------------------------ bilinear reduction + L2 norm

def _lerp_table(si, so):
    """(i0, i1, w1) per output index, the align_corners=False source rule evaluated in fp32 like the kernel (for every side pair the
    product uses, si / so and all weights are short binary fractions: fp32 and fp64 agree exactly)"""
    i0s, i1s, w1s = [], [], []
    scale = np.float32(si) / np.float32(so)
    for o in range(so):
        src = scale * (np.float32(o) + np.float32(0.5)) - np.float32(0.5)
        src = max(src, np.float32(0.0))
        i0 = int(src)
        i0s.append(i0)
        i1s.append(i0 + (1 if i0 < si - 1 else 0))
        w1s.append(float(np.float32(src) - np.float32(i0)))
    return torch.tensor(i0s), torch.tensor(i1s), torch.tensor(w1s, dtype=torch.float64)


def _corners(si, so):
    """flat source index [4, so * so] and weight [4, so * so] of the four corners of every output token (identity: one corner, weight 1)"""
    if si == so:
        idx = torch.arange(si * si)
        z = torch.zeros(si * si, dtype=torch.float64)
        return torch.stack([idx, idx, idx, idx]), torch.stack([z + 1.0, z, z, z])
    i0, i1, w1 = _lerp_table(si, so)
    y0, y1, ly = i0[:, None].expand(so, so), i1[:, None].expand(so, so), w1[:, None].expand(so, so)
    x0, x1, lx = i0[None, :].expand(so, so), i1[None, :].expand(so, so), w1[None, :].expand(so, so)
    idx = torch.stack([y0 * si + x0, y0 * si + x1, y1 * si + x0, y1 * si + x1]).reshape(4, so * so)
    wgt = torch.stack([(1 - lx) * (1 - ly), lx * (1 - ly), (1 - lx) * ly, lx * ly]).reshape(4, so * so)
    return idx, wgt


def _interp_rows(x64, si, so):
    """interpolated rows r [N, so^2, C] in fp64 (unrounded) and sum_corners w |src|"""
    idx, wgt = _corners(si, so)
    r = sum(x64[:, idx[k]] * wgt[k][None, :, None] for k in range(4))
    s = sum(x64[:, idx[k]].abs() * wgt[k][None, :, None] for k in range(4))
    return r, s


def _bf16_norm(ss):
    return to_bf16(torch.sqrt(ss)).double().clamp_min(1e-12)


def bilinear_l2norm_ref(x, si, so, normalize):
    """[N, si^2, C] -> [N, so^2, C]: bilinear interpolation (align_corners=False) and an optional L2 normalisation with the kernel's
    rounding points: the interpolated row is rounded to bf16, the norm sqrt(sum r^2) is rounded to bf16 and clamped at 1e-12;
    everything else is fp64.  Returns (y fp64 (not yet rounded to bf16), r [bf16 values in fp64], norm [N, so^2, 1] or None)."""
    r64, _ = _interp_rows(x.double(), si, so)
    r = to_bf16(r64).double()
    if not normalize:
        return r, r, None
    nrm = _bf16_norm((r * r).sum(-1, keepdim=True))
    return r / nrm, r, nrm


def bilinear_l2norm_bwd_ref(x, dy, si, so, normalize):
    """Gradient of bilinear_l2norm_ref w.r.t. x for the upstream gradient dy [N, so^2, C], with the rounding points treated as
    identities (as the kernel does): dr = (dy - r (r . dy) / n^2) / n, scattered to the four corners with their weights.
    Returns a dict, all fp64:
      din       [N, si^2, C]   the gradient
      count     [si^2]         number of non-zero-weight addends a source pixel receives
      abs_sum   [N, si^2, C]   sum over those addends of w (|dy| + |r| |r . dy| / n^2) / n  (the magnitude before the cancellation
                               of dy against its projection)
      extra     [N, si^2, C]   what the kernel's fp32 chain ahead of the scatter may move the addends by (see below)
    `extra` is derived from operation counts only.  With c = 8 ceil(C / 512) + 8 the length of a lane's sum plus the six-level wave
    tree: the dot product r . dy is off by <= c U sum |r dy|; sum r^2 by <= c U relative; a row element within 4 U sum w |src| of
    a bf16 rounding boundary may round to the neighbour (changing r, r . dy and sum r^2); and where sqrt(sum r^2) then lies on a
    bf16 boundary, the rounded norm may be the neighbouring bf16 value."""
    x64, g = x.double(), dy.double()
    N, _, C = x64.shape
    idx, wgt = _corners(si, so)
    r64, s64 = _interp_rows(x64, si, so)
    r = to_bf16(r64).double()
    if normalize:
        c = 8 * math.ceil(C / 512) + 8
        dr_flip = (to_bf16(r64 + 4 * U * s64).double() - to_bf16(r64 - 4 * U * s64).double()).abs() if si != so else torch.zeros_like(r)
        ss = (r * r).sum(-1, keepdim=True)
        e_ss = c * U * ss + (2 * r.abs() * dr_flip + dr_flip * dr_flip).sum(-1, keepdim=True)
        nrm = _bf16_norm(ss)
        n_lo, n_hi = _bf16_norm((ss - e_ss).clamp_min(0) * (1 - 4 * U)), _bf16_norm((ss + e_ss) * (1 + 4 * U))
        inv, inv_lo, inv_hi = 1 / nrm, 1 / n_hi, 1 / n_lo
        dot = (r * g).sum(-1, keepdim=True)
        d_dot = c * U * (r * g).abs().sum(-1, keepdim=True) + (dr_flip * g.abs()).sum(-1, keepdim=True)
        D = dot * inv * inv
        d_D = d_dot * inv_hi * inv_hi + dot.abs() * (inv_hi * inv_hi - inv_lo * inv_lo) + 3 * U * D.abs()
        dr = (g - r * D) * inv
        dr_abs = (g.abs() + (r * D).abs()) * inv
        dr_extra = (r.abs() * d_D + dr_flip * D.abs() + 2 * U * (g.abs() + (r * D).abs())) * inv_hi + (g - r * D).abs() * (inv_hi - inv_lo)
    else:
        dr, dr_abs, dr_extra = g, g.abs(), torch.zeros_like(g)
    din, abs_sum, extra = torch.zeros_like(x64), torch.zeros_like(x64), torch.zeros_like(x64)
    count = torch.zeros(si * si, dtype=torch.float64)
    for k in range(4):
        wk = wgt[k][None, :, None]
        din.index_add_(1, idx[k], dr * wk)
        abs_sum.index_add_(1, idx[k], dr_abs * wk)
        extra.index_add_(1, idx[k], dr_extra * wk)
        count.index_add_(0, idx[k], (wgt[k] != 0).double())
    return dict(din=din, count=count, abs_sum=abs_sum, extra=extra)


def bilinear_l2norm_autograd(x, si, so, normalize):
    """the same operation as plain differentiable torch (no rounding points): F.interpolate + F.normalize, in x's dtype"""
    N, _, C = x.shape
    y = x
    if si != so:
        y = F.interpolate(x.view(N, si, si, C).permute(0, 3, 1, 2), size=(so, so), mode="bilinear", align_corners=False)
        y = y.permute(0, 2, 3, 1).reshape(N, so * so, C)
    return F.normalize(y, p=2, dim=-1) if normalize else y


# ------------------------------------------------------------------------------------------------ encoder layer and patch embedding

LAYER_PARAM_NAMES = tuple(f"{m}.{p}" for m in ("layer_norm1", "self_attn.k_proj", "self_attn.v_proj", "self_attn.q_proj", "self_attn.out_proj",
                                                "layer_norm2", "mlp.fc1", "mlp.fc2") for p in ("weight", "bias"))


def siglip_layer_ref(x, params, N, P, heads, eps, stats=None):
    """One HF SiglipEncoderLayer on rows x [N * P, h] in the dtype of its inputs (fp64 for the reference, bf16 for the yardstick):
    x + out_proj(softmax(q k^T / sqrt(d)) v) of layer_norm1(x), then + fc2(gelu_tanh(fc1(layer_norm2(.)))).  `params` maps the
    module's parameter names (LAYER_PARAM_NAMES) to tensors.  `stats`, if a dict, receives the ranges of the attention logits and of
    the fc1 pre-activations."""
    h = x.shape[-1]
    d = h // heads
    p = params
    h1 = F.layer_norm(x, (h,), p["layer_norm1.weight"], p["layer_norm1.bias"], eps)

    def split(t):
        return t.view(N, P, heads, d).transpose(1, 2)          # [N, heads, P, d]
    q = split(F.linear(h1, p["self_attn.q_proj.weight"], p["self_attn.q_proj.bias"]))
    k = split(F.linear(h1, p["self_attn.k_proj.weight"], p["self_attn.k_proj.bias"]))
    v = split(F.linear(h1, p["self_attn.v_proj.weight"], p["self_attn.v_proj.bias"]))
    s = torch.matmul(q, k.transpose(-1, -2)) * d ** -0.5
    a = torch.softmax(s, dim=-1)
    o = torch.matmul(a, v).transpose(1, 2).reshape(N * P, h)
    x2 = x + F.linear(o, p["self_attn.out_proj.weight"], p["self_attn.out_proj.bias"])
    h2 = F.layer_norm(x2, (h,), p["layer_norm2.weight"], p["layer_norm2.bias"], eps)
    f_pre = F.linear(h2, p["mlp.fc1.weight"], p["mlp.fc1.bias"])
    if stats is not None:
        sd = s.detach().double()
        stats.update(logit_min=float(sd.min()), logit_max=float(sd.max()), logit_row_span=float((sd.max(-1).values - sd.min(-1).values).median()),
                     fc1_min=float(f_pre.detach().min()), fc1_max=float(f_pre.detach().max()))
    return x2 + F.linear(F.gelu(f_pre, approximate="tanh"), p["mlp.fc2.weight"], p["mlp.fc2.bias"])


def patch_embed_ref(images, w, b, pos):
    """conv2d(kernel = stride = patch) + bias, tokens in row-major patch order, + the position table: [N, P, h]"""
    y = F.conv2d(images, w, b, stride=w.shape[-1])
    return y.flatten(2).transpose(1, 2) + pos


def rel_fro(got, ref):
    """relative Frobenius error of `got` to the fp64 reference"""
    ref = ref.detach().double()
    return float((got.detach().double().cpu() - ref).norm() / ref.norm().clamp_min(1e-300))
