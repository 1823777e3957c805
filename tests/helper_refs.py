"""Test infrastructure: plain fp64 references and error bounds for the step's helper kernels (metamorph_amd/csrc/elementwise.hip,
losses.hip and ce_rows / cosine_loss of rowwise.hip), written in torch so that they run on whichever device their inputs live on.

Every reference takes the bf16- or fp32-rounded values the kernel gets and evaluates the operation in fp64.  Where a kernel documents a
rounding point inside its chain (round_bf(x * inv_temp), round_bf(sqrt(pp)), round_bf(p / pn), the bf16 q of the soft cross-entropy, the
bf16 silu of SwiGLU) the reference rounds there too: such a rounding is part of WHAT is computed, not an error of computing it.  Two kinds
of rounding points exist:

  * one IEEE fp32 operation on bf16 / fp32 operands followed by RNE to bf16 (x * inv_temp, t - p, p / pn, g * gs): the reference performs
    the same fp32 operation (it has one correctly rounded result, on every machine) and rounds it -- reproduced exactly
  * the end of an fp32 CHAIN (sqrt of a 1152-term sum, exp(z - m) / s, silu): the chain's fp32 value differs from fp64 by its own rounding
    error, so an fp64 value closer to a bf16 tie than that error can legitimately round either way.  `near_tie` finds such values; the
    tests either build inputs that have none (row norms) or add the effect of a flip to the bound (q of the soft cross-entropy).

The "reference stack" evaluations (`stack_*`) are torch on the CPU in the precision the reference model runs in.  They are what the
constants below were measured on (tests/test_helper_refs_host.py measures them again and asserts them); the GPU tests allow the kernels a
fixed multiple of them.  Nothing here is derived from a kernel's output.
"""
import math

import numpy as np
import torch

F64 = torch.float64
U24 = 2.0 ** -24            # fp32 unit roundoff (half an ulp, relative): the error of one correctly rounded fp32 operation
BF_STEP = 2.0 ** -8         # one bf16 step, relative (the issue's figure for the final rounding)
TINY = 2.0 ** -126          # smallest normal bf16 / fp32 magnitude

GELU_ERF, GELU_TANH = 0, 1

# ---- measured on the reference stack by tests/test_helper_refs_host.py (torch CPU, fp32 math, bf16 result), asserted there --------------
# smallest c under which the stack's own evaluation over all 65 536 bf16 inputs satisfies `act_bound`; the kernels get 4x.  These are the
# figures of torch's vectorised CPU paths (AVX2 and AVX-512 agree); its scalar path (ATEN_CPU_CAPABILITY=default) evaluates tanh through
# libm and needs half (0.2461 / 1.745), everything else is the same to three digits.
STACK_C = {
    "gelu_fwd_erf": 0.7905, "gelu_fwd_tanh": 0.4942, "gelu_bwd_erf": 0.06128, "gelu_bwd_tanh": 3.403,
    "swiglu_fwd": 3.72e-32, "swiglu_dgate": 3.69e-32, "swiglu_dup": 3.72e-32,      # the tail g <= -89, where exp(-g) overflows fp32
}
# finite inputs at which the stack's own result is not finite (excluded from the bound; a known property of the fp32 formulas)
# erf forward: the top 128 patterns (x * (1 + erf) overflows before the 0.5); tanh gradient: |x| >= 2^64 (x^3 overflows, 0 * inf);
# SwiGLU forward: the products with u = 3 * 2^10 that overflow bf16
STACK_EXCLUDED = {"gelu_fwd_erf": 128, "gelu_fwd_tanh": 0, "gelu_bwd_erf": 0, "gelu_bwd_tanh": 16384, "swiglu_fwd": 1493,
                  "swiglu_dgate": 0, "swiglu_dup": 0}
# max |stack - fp64| / max |fp64| of the stack's bf16 evaluation of the row gradients (existing cases' shapes); the kernels get 2x
STACK_GRAD_DIST = {"softmax_bwd": 0.00549, "soft_ce_norm": 0.0098, "soft_ce_raw": 0.005411, "cosine_norm": 0.007305, "cosine_raw": 0.007252}
KERNEL_C_FACTOR = 4.0
KERNEL_GRAD_FACTOR = 2.0


# ------------------------------------------------------------------------------------------------ bf16 plumbing

def all_bf16():
    """all 65 536 bf16 bit patterns, pattern i at index i"""
    return torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def bits(t):
    """int32 bit patterns (0 .. 65535) of a bf16 tensor"""
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def round_bf(x):
    """fp64 -> nearest bf16 (ties to even) -> fp64, in ONE rounding: the value goes through fp32 rounded to odd, which keeps the sticky
    information a plain fp64 -> fp32 -> bf16 cast loses (a double rounding, wrong for about one value in 2^16)."""
    x = x.to(F64)
    f = x.to(torch.float32)
    back = f.to(F64)
    b = f.view(torch.int32).clone()
    mag = b & 0x7FFFFFFF
    fin = torch.isfinite(x)
    over = fin & (back.abs() > x.abs())
    mag = torch.where(over, mag - 1, mag)                      # towards zero ...
    mag = torch.where(fin & (back != x), mag | 1, mag)         # ... and odd when inexact
    r = mag + 0x7FFF + ((mag >> 16) & 1)
    r = (r >> 16) << 16
    r = torch.where(torch.isnan(x), mag, r)
    out = (r | (b & -0x80000000)).to(torch.int32).view(torch.float32)
    return out.to(F64)


def near_tie(x, rel):
    """True where a relative perturbation of `rel` moves round_bf(x): the rounding is not decided by an fp32 chain with that error"""
    x = x.to(F64)
    return round_bf(x * (1.0 - rel)) != round_bf(x * (1.0 + rel))


def subnormal(x):
    """bf16 / fp32 subnormal (nonzero below 2^-126)"""
    a = x.to(F64).abs()
    return (a > 0) & (a < TINY)


def classes(t):
    """0 NaN, 1 +inf, 2 -inf, 3 zero (either sign), 4 finite nonzero"""
    t = t.to(F64)
    c = torch.full(t.shape, 4, dtype=torch.int32, device=t.device)
    c[t == 0] = 3
    c[torch.isposinf(t)] = 1
    c[torch.isneginf(t)] = 2
    c[torch.isnan(t)] = 0
    return c


def f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------ activations (fp64)

_S2PI = math.sqrt(2.0 / math.pi)


def gelu64(x, kind):
    x = x.to(F64)
    if kind == GELU_ERF:
        return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))
    u = _S2PI * (x + 0.044715 * x * x * x)
    return x * torch.sigmoid(2.0 * u)                          # 0.5 (1 + tanh u) = sigmoid(2u), without the cancellation


def gelu_grad64(x, kind):
    x = x.to(F64)
    if kind == GELU_ERF:
        return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    u = _S2PI * (x + 0.044715 * x * x * x)
    du = _S2PI * (1.0 + 3.0 * 0.044715 * x * x)
    s = torch.sigmoid(2.0 * u)
    return s + x * (2.0 * s * (1.0 - s)) * du                  # 1 - tanh^2 = 4 s (1 - s)


def swiglu_fwd64(g, u):
    """the reference stack's order: silu -> bf16, times up -> (the caller compares with the kernel's bf16 result)"""
    g, u = g.to(F64), u.to(F64)
    return round_bf(g * torch.sigmoid(g)) * u


def swiglu_bwd64(g, u, da):
    """(dgate, dup): dup through the bf16-rounded silu, dgate from the fp64 derivative"""
    g, u, da = g.to(F64), u.to(F64), da.to(F64)
    sg = torch.sigmoid(g)
    return da * u * (sg * (1.0 + g * (1.0 - sg))), da * round_bf(g * sg)


def act_bound(ref, x, factor, c, steps=1):
    """steps * 2^-8 |ref| (bf16 roundings on the way) + c * 2^-24 * max(|x|, 1) * |factor| (the fp32 cancellation in 1 + erf, 1 + tanh,
    1 - sg) + 2^-126 where the result is subnormal"""
    ref, x = ref.to(F64), x.to(F64)
    factor = torch.as_tensor(factor, dtype=F64, device=ref.device)
    return steps * BF_STEP * ref.abs() + c * U24 * x.abs().clamp_min(1.0) * factor.abs() + TINY * (ref.abs() < TINY)


def smallest_c(got, ref, x, factor, steps, mask):
    """the smallest c for which `got` meets act_bound on the masked elements"""
    got, ref, x = got.to(F64), ref.to(F64), x.to(F64)
    factor = torch.as_tensor(factor, dtype=F64, device=ref.device).expand_as(ref)
    over = (got - ref).abs() - act_bound(ref, x, factor, 0.0, steps)
    den = U24 * x.abs().clamp_min(1.0) * factor.abs()
    m = mask & (over > 0)
    if not bool(m.any()):
        return 0.0
    assert bool((den[m] > 0).all()), "the bound has no room where the factor is zero"
    return float((over[m] / den[m]).max())


# the reference stack: torch on the CPU, fp32 math, result rounded to bf16

def stack_gelu_fwd(x_bf, kind):
    return torch.nn.functional.gelu(x_bf.float(), approximate="none" if kind == GELU_ERF else "tanh").bfloat16()


def stack_gelu_bwd(x_bf, dy_bf, kind):
    x = x_bf.float().requires_grad_(True)
    y = torch.nn.functional.gelu(x, approximate="none" if kind == GELU_ERF else "tanh")
    g, = torch.autograd.grad(y, x, dy_bf.float().expand_as(y))
    return g.bfloat16()


def stack_swiglu_fwd(g_bf, u_bf):
    return (torch.nn.functional.silu(g_bf.float()).bfloat16().float() * u_bf.float()).bfloat16()


def stack_swiglu_bwd(g_bf, u_bf, da_bf):
    g = g_bf.float().requires_grad_(True)
    s = torch.nn.functional.silu(g)
    dg, = torch.autograd.grad(s, g, (da_bf.float() * u_bf.float()).expand_as(s))
    return dg.bfloat16(), (da_bf.float() * s.detach().bfloat16().float()).bfloat16()


def swiglu_domain(uvals, davals=None):
    """gu [M, 1024] (I = 512) in which every bf16 gate pattern meets every up value (and every dact value): 128 rows per combination"""
    pat = all_bf16().view(128, 512)
    combos = [(u, d) for d in (davals or [None]) for u in uvals]
    gu = torch.empty(128 * len(combos), 1024, dtype=torch.bfloat16)
    da = torch.empty(128 * len(combos), 512, dtype=torch.bfloat16) if davals else None
    for k, (u, d) in enumerate(combos):
        gu[128 * k:128 * (k + 1), :512] = pat
        gu[128 * k:128 * (k + 1), 512:] = u
        if davals:
            da[128 * k:128 * (k + 1)] = d
    return gu, da


# ------------------------------------------------------------------------------------------------ row-per-wave kernels (fp64)

def inv_temp_f32(temperature):
    return np.float32(1.0) / np.float32(temperature)


def _z(x_bf, inv_temp):
    """round_bf(x * inv_temp): one fp32 multiply, then RNE"""
    return (x_bf.float() * float(inv_temp)).bfloat16().to(F64)


def softmax_rows64(x_bf, temperature=0.07):
    return torch.softmax(_z(x_bf, inv_temp_f32(temperature)), -1)


def softmax_rows_bwd64(y_bf, dy_bf, temperature=0.07):
    y, dy = y_bf.to(F64), dy_bf.to(F64)
    return y * (dy - (y * dy).sum(-1, keepdim=True)) * float(inv_temp_f32(temperature))


def lane_adds(C, per_elem=1):
    """rounded fp32 additions (and multiplies, per_elem = 2) one lane performs on a row of C elements: 8 per 16-byte vector, a vector
    every 64"""
    return 8 * per_elem * (-(-(C // 8) // 64))


def row_sum_adds(R):
    """mm_sum_rows_kernel: 1024 threads stride the rows, then a 10-level tree, the scale and the prefill (test_sum_rows_f32_through_ctypes)"""
    return -(-R // 1024) + 12


def mean_abs64(p_bf, t_bf):
    """(sum |round_bf(t - p)|, dpred = -sign(d) / (R C), sum of |terms| for the bound)"""
    d = (t_bf.float() - p_bf.float()).bfloat16().to(F64)       # the bf16 subtraction of the reference stack
    Rr, C = p_bf.shape
    return d.abs().sum(), -torch.sign(d) / (Rr * C), d.abs().sum()


def _unit(p_bf, normalize):
    """(u, pn, pp): F.normalize on a bf16 tensor -- norm rounded to bf16, clamp 1e-12, one fp32 divide, RNE"""
    p = p_bf.to(F64)
    pp = (p * p).sum(-1, keepdim=True)
    if not normalize:
        return p, torch.ones_like(pp), pp
    pn = round_bf(pp.sqrt()).clamp_min(f32(1e-12))
    u = (p / pn).to(torch.float32).bfloat16().to(F64)
    return u, pn, pp


def row_norm_near_tie(p_bf):
    """rows whose norm an fp32 sum of C squares (error <= (adds + tree) 2^-24, halved by the root, plus the root's own) cannot place on one
    side of a bf16 tie: the tests rebuild such rows instead of guessing"""
    C = p_bf.shape[-1]
    pp = (p_bf.to(F64) ** 2).sum(-1)
    return near_tie(pp.sqrt(), (lane_adds(C, 2) + 8) * U24)


def cosine64(p_bf, t_bf, normalize):
    """(sum_r cos_r, dpred, sum_r sum_j |t u| / (nt nu)) exactly as cosine_loss_kernel documents it"""
    t = t_bf.to(F64)
    u, pn, pp = _unit(p_bf, normalize)
    Rr = p_bf.shape[0]
    nt = (t * t).sum(-1, keepdim=True).sqrt().clamp_min(f32(1e-8))
    nu = (u * u).sum(-1, keepdim=True).sqrt().clamp_min(f32(1e-8))
    c = (t * u).sum(-1, keepdim=True) / (nt * nu)
    w = (t / nt - c * u / nu) / nu
    if normalize:
        p = p_bf.to(F64)
        pnorm = pp.sqrt().clamp_min(f32(1e-20))
        pw = (p * w).sum(-1, keepdim=True) / pnorm
        g = (-1.0 / Rr) * (w - (p / pnorm) * pw) / pn
    else:
        g = (-1.0 / Rr) * w
    return c.sum(), g, ((t * u).abs().sum(-1, keepdim=True) / (nt * nu)).sum()


def soft_ce64(p_bf, t_bf, normalize, temperature=0.07):
    """(sum_r loss_r, dpred, sum of |terms|, flip slack): q = round_bf(softmax(round_bf(u * inv_temp))); loss_r = -sum t log(q + 1e-10).
    flip slack = sum over the q an fp32 exp / sum chain cannot place on one side of a bf16 tie of t * 2^-7 (a flipped q moves its log by
    one bf16 step)."""
    it = inv_temp_f32(temperature)
    t = t_bf.to(F64)
    u, pn, pp = _unit(p_bf, normalize)
    Rr, C = p_bf.shape
    z = (u.to(torch.float32) * float(it)).bfloat16().to(F64)
    sm = torch.softmax(z, -1)
    q = round_bf(sm)
    eps = f32(1e-10)
    terms = t * torch.log(q + eps)
    # exp(a), a = z - m <= 0: the argument's product with log2 e and v_exp_f32 give |a| 2^-22 + 2^-22 relative, the sum (adds + tree) 2^-24
    a = (z - z.max(-1, keepdim=True).values).abs()
    amb = near_tie(sm, a * 2.0 ** -22 + 2.0 ** -22 + (lane_adds(C) + 8) * U24)
    slack = (amb * t.abs()).sum() * 2.0 ** -7
    gq = -(t * q / (q + eps)).sum(-1, keepdim=True)
    du = q * (-t / (q + eps) - gq) * (float(it) / Rr)
    if normalize:
        p = p_bf.to(F64)
        pnorm = pp.sqrt().clamp_min(f32(1e-20))
        ud = ((p / pnorm) * du).sum(-1, keepdim=True)
        g = (du - (p / pnorm) * ud) / pnorm
    else:
        g = du
    return -terms.sum(), g, terms.abs().sum(), slack


def loss_bound(C, R, abs_terms, per_elem=1, extra_ops=0):
    """(adds per lane + 6 tree levels + per-term operations + the row sum's adds) * 2^-24 * sum |terms|"""
    return (lane_adds(C, per_elem) + 6 + extra_ops + row_sum_adds(R)) * U24 * float(abs_terms)


def ce_rows64(logits_bf, targets, V, grad_scale):
    """(sum of lse - x[target] over live rows, gradient [R, ld] with zero padding and zero ignored rows, sum of |lse| + |x[target]|)"""
    x = logits_bf[:, :V].to(F64)
    live = targets >= 0
    lse = torch.logsumexp(x, -1)
    tg = targets.clamp_min(0).long()
    picked = x.gather(1, tg[:, None])[:, 0]
    g = torch.exp(x - lse[:, None])
    g[torch.arange(x.shape[0], device=x.device), tg] -= 1.0
    g = g * grad_scale * live[:, None]
    full = torch.zeros(logits_bf.shape, dtype=F64, device=x.device)
    full[:, :V] = g
    return (lse - picked)[live].sum(), full, (lse.abs() + picked.abs())[live].sum()


# ------------------------------------------------------------------------------------------------ AdamW (fp64 replay of one step)

def adamw_replay64(p, m, v, g_bf, lr, b1, b2, eps, wd, step, gs):
    """One step from the fp32 state (p, m, v), every scalar formed as ops.adamw_shard_ and the kernel form it (Python floats -> fp32), the
    element arithmetic in fp64.  gr = fp32(g * gs) is a single fp32 multiply and is taken as the kernel's input.
    Returns (p', m', v', bound_p, bound_m, bound_v); see test_adamw_every_output for the derivation of the bounds."""
    F = np.float32
    lr32, b132, b232, eps32, wd32 = F(lr), F(b1), F(b2), F(eps), F(wd)
    bc1, bc2 = F(1.0 - b1 ** step), F(1.0 - b2 ** step)
    decay = float(F(1.0) - lr32 * wd32)
    omb1, omb2 = float(F(1.0) - b132), float(F(1.0) - b232)
    stepsz = float(lr32 / bc1)
    isb = 1.0 / math.sqrt(float(bc2))
    gr = (g_bf.float() * float(F(gs))).to(F64) if gs is not None else g_bf.to(F64)
    p, m, v = p.to(F64), m.to(F64), v.to(F64)
    tm = (m * float(b132)).abs() + (omb1 * gr).abs()
    tv = (v * float(b232)).abs() + omb2 * gr * gr
    mi = m * float(b132) + omb1 * gr
    vi = v * float(b232) + omb2 * gr * gr
    denom = vi.sqrt() * isb + float(eps32)
    upd = stepsz * (mi / denom)
    pn = p * decay - upd
    sub = 3 * 2.0 ** -150                                      # three operations, half a subnormal step each, where a result underflows
    bm = 3 * U24 * tm + sub
    bv = 3 * U24 * tv + sub
    bp = U24 * (2 * (p * decay).abs() + pn.abs()) + 11.5 * U24 * upd.abs() + 3 * U24 * stepsz * tm / denom + sub
    return pn, mi, vi, bp, bm, bv
