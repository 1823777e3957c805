"""Tensor-level wrappers over the C ABI (include/mm355.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; every arithmetic op below is a
hand-written gfx950 kernel in libmm355.so reached through ctypes with raw pointers.  Nothing in this
module computes with torch ops, and nothing falls back to them.
"""
from __future__ import annotations

import os

import torch

from . import lib as _lib

BF16 = torch.bfloat16

GEMM_BIAS, GEMM_GELU_ERF, GEMM_GELU_TANH, GEMM_RESIDUAL, GEMM_ACCUMULATE, GEMM_OUT_F32 = 1, 2, 4, 8, 16, 32
GELU_ERF, GELU_TANH = 0, 1


def _L():
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk_dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.Mm355Unavailable("metamorph_amd ops run only on an MI355X HIP device; got a CPU tensor "
                                        "(there is no CPU fallback)")


def _p(t):
    return 0 if t is None else t.data_ptr()


def _rows2d(t):
    """(ptr, rows, cols, ld) of a 2-D view whose last dim is contiguous."""
    assert t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1), (t.shape, t.stride())
    return t.data_ptr(), t.shape[0], t.shape[1], t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


# ------------------------------------------------------------------------------------------------ GEMM

def gemm(a, b, out=None, *, bias=None, residual=None, res_row_mod=0, gelu=None, accumulate=False,
         out_f32=False, variant=0, n=None):
    """out[M,N] = epilogue(a[M,K] . b[N,K]^T).  a/b/out may be row-strided 2-D views (bf16)."""
    _chk_dev(a, b, out, bias, residual)
    assert a.dtype == BF16 and b.dtype == BF16
    pa, M, K, lda = _rows2d(a)
    pb, N, Kb, ldb = _rows2d(b)
    assert K == Kb, (a.shape, b.shape)
    if n is not None:
        N = n
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32 if out_f32 else BF16)
    po, Mo, No, ldc = _rows2d(out)
    assert Mo == M and No >= N, (out.shape, M, N)
    flags = 0
    if bias is not None:
        flags |= GEMM_BIAS
        assert bias.dtype == BF16 and bias.is_contiguous() and bias.numel() >= N
    if gelu == "erf":
        flags |= GEMM_GELU_ERF
    elif gelu == "tanh":
        flags |= GEMM_GELU_TANH
    elif gelu is not None:
        raise ValueError(gelu)
    ldr = 0
    if residual is not None:
        flags |= GEMM_RESIDUAL
        assert residual.dtype == BF16
        _, _, _, ldr = _rows2d(residual)
    if accumulate:
        flags |= GEMM_ACCUMULATE
    if out.dtype == torch.float32:
        flags |= GEMM_OUT_F32
    else:
        assert out.dtype == BF16
    rc = _L().mm355_gemm_bf16(pa, lda, pb, ldb, po, ldc, M, N, K, _p(bias), _p(residual), ldr, res_row_mod,
                              flags, variant, _stream())
    _lib.check(rc, f"mm355_gemm_bf16 M={M} N={N} K={K} lda={lda} ldb={ldb} ldc={ldc} flags={flags} variant={variant}")
    return out


def gemm_splitk(a, b, residual=None, out=None):
    """out[M, N] = a[M, K] . b[N, K]^T (+ residual), K cut into slices that run side by side (mm355_gemm_splitk_bf16): the prompt-pass form --
    a few hundred rows against one weight, where the plain kernels are a latency chain over K.  Shapes it would not split go to the plain
    kernel inside the library.  Another fp32 summation order than ops.gemm: equal to accumulation accuracy, not bit for bit."""
    _chk_dev(a, b, residual, out)
    assert a.dtype == BF16 and b.dtype == BF16
    pa, M, K, lda = _rows2d(a)
    pb, N, Kb, ldb = _rows2d(b)
    assert K == Kb
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=BF16)
    po, _, _, ldc = _rows2d(out)
    pr, ldr = 0, 0
    if residual is not None:
        pr, Mr, Nr, ldr = _rows2d(residual)
        assert (Mr, Nr) == (M, N)
    n_ws = int(_L().mm355_gemm_splitk_ws_floats(M, N, K))
    ws = torch.empty((max(n_ws, 4),), device=a.device, dtype=torch.float32)
    _lib.check(_L().mm355_gemm_splitk_bf16(pa, lda, pb, ldb, po, ldc, M, N, K, pr, ldr, ws.data_ptr(), n_ws, _stream()),
               f"mm355_gemm_splitk_bf16 M={M} N={N} K={K}")
    return out


def gemm_splitk_splits(M, N, K):
    """mm355_gemm_splitk_bf16 would cut this problem into K slices (else it forwards to the plain kernel)."""
    return int(_L().mm355_gemm_splitk_ws_floats(M, N, K)) > 0


def _splitk_ws(n_floats, device):
    return torch.empty((max(int(n_floats), 4),), device=device, dtype=torch.float32)


def gemm_splitk_norm(a, b, norm_w, eps, residual=None):
    """(c, y): c[M, N] = a . b^T (+ residual) through the split-K GEMM, y = RMSNorm(c; norm_w, eps) formed by the reduce launch
    (mm355_gemm_splitk_norm_bf16: the bits of gemm_splitk -> rmsnorm_fwd, one launch less)."""
    _chk_dev(a, b, norm_w, residual)
    pa, M, K, lda = _rows2d(a)
    pb, N, Kb, ldb = _rows2d(b)
    assert K == Kb and a.dtype == BF16 and b.dtype == BF16 and norm_w.numel() == N
    c = torch.empty((M, N), device=a.device, dtype=BF16)
    y = torch.empty((M, N), device=a.device, dtype=BF16)
    pr, ldr = 0, 0
    if residual is not None:
        pr, Mr, Nr, ldr = _rows2d(residual)
        assert (Mr, Nr) == (M, N)
    n_ws = int(_L().mm355_gemm_splitk_ws_floats(M, N, K))
    ws = _splitk_ws(n_ws, a.device)
    _lib.check(_L().mm355_gemm_splitk_norm_bf16(pa, lda, pb, ldb, c.data_ptr(), M, N, K, pr, ldr, norm_w.data_ptr(), float(eps), y.data_ptr(),
                                                ws.data_ptr(), n_ws, _stream()), f"mm355_gemm_splitk_norm_bf16 M={M} N={N} K={K}")
    return c, y


def gemm_splitk_swiglu(x, wgu, I):
    """act[M, I] = SiLU(g) * u, [g | u] = x . wgu^T through the split-K GEMM, SwiGLU in the reduce launch (mm355_gemm_splitk_swiglu_bf16: the
    bits of gemm_splitk -> swiglu_fwd)."""
    _chk_dev(x, wgu)
    px, M, K, ldx = _rows2d(x)
    pw, N, Kw, ldw = _rows2d(wgu)
    assert K == Kw and N == 2 * I and x.dtype == BF16 and wgu.dtype == BF16
    act = torch.empty((M, I), device=x.device, dtype=BF16)
    n_ws = int(_L().mm355_gemm_splitk_swiglu_ws_floats(M, I, K))
    ws = _splitk_ws(n_ws, x.device)
    _lib.check(_L().mm355_gemm_splitk_swiglu_bf16(px, ldx, pw, ldw, act.data_ptr(), act.stride(0), M, I, K, ws.data_ptr(), n_ws, _stream()),
               f"mm355_gemm_splitk_swiglu_bf16 M={M} I={I} K={K}")
    return act


def gemm_splitk_rope_append(x, wqkv, Hq, Hkv, d, cos, sin, positions, k_cache, v_cache):
    """One new q|k|v row per sequence through the split-K GEMM; RoPE at positions[m] (int32, device) and the KV-cache append in the reduce
    launch (mm355_gemm_splitk_rope_append_bf16: the bits of gemm_splitk -> rope_kv_append_).  Returns the row buffer [M, (Hq+2Hkv)*d] whose
    q columns are valid."""
    _chk_dev(x, wqkv, cos, sin, positions, k_cache, v_cache)
    px, M, K, ldx = _rows2d(x)
    pw, N, Kw, ldw = _rows2d(wqkv)
    assert K == Kw and N == (Hq + 2 * Hkv) * d and positions.dtype == torch.int32
    assert k_cache.stride() == v_cache.stride() and k_cache.stride(2) == 1
    out = torch.empty((M, N), device=x.device, dtype=BF16)
    n_ws = int(_L().mm355_gemm_splitk_ws_floats(M, N, K))
    ws = _splitk_ws(n_ws, x.device)
    _lib.check(_L().mm355_gemm_splitk_rope_append_bf16(px, ldx, pw, ldw, out.data_ptr(), out.stride(0), M, Hq, Hkv, d, K, cos.data_ptr(), sin.data_ptr(),
                                                       positions.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(1),
                                                       k_cache.stride(0), ws.data_ptr(), n_ws, _stream()), "mm355_gemm_splitk_rope_append_bf16")
    return out


def gemm_pair_supported(a0, b0, a1, b1):
    """Both problems fit mm355_gemm_pair_bf16 (plain NT operands, whole pairs of K tiles, 31-bit operand offsets)."""
    return (a0.shape[1] == b0.shape[1] and a1.shape[1] == b1.shape[1]
            and gemm_pp_operands_ok(a0.shape[1], a0, b0) and gemm_pp_operands_ok(a1.shape[1], a1, b1))


def gemm_pair(a0, b0, out0, acc0, a1, b1, out1, acc1):
    """out0[M0,N0] (+)= a0 . b0^T and out1[M1,N1] (+)= a1 . b1^T in ONE launch (fills the partial last wave of workgroups that
    each problem leaves on its own).  Raises Mm355Error(-2) when a problem is not eligible: check gemm_pair_supported first."""
    _chk_dev(a0, b0, out0, a1, b1, out1)
    probs = []
    for a, b, out, acc in ((a0, b0, out0, acc0), (a1, b1, out1, acc1)):
        assert a.dtype == BF16 and b.dtype == BF16
        pa, M, K, lda = _rows2d(a)
        pb, N, Kb, ldb = _rows2d(b)
        assert K == Kb, (a.shape, b.shape)
        po, Mo, No, ldc = _rows2d(out)
        assert (Mo, No) == (M, N), (out.shape, M, N)
        assert out.dtype in (BF16, torch.float32)
        flags = (GEMM_ACCUMULATE if acc else 0) | (GEMM_OUT_F32 if out.dtype == torch.float32 else 0)
        probs += [pa, lda, pb, ldb, po, ldc, M, N, K, flags]
    _lib.check(_L().mm355_gemm_pair_bf16(*probs, _stream()),
               f"mm355_gemm_pair_bf16 {tuple(a0.shape)}x{tuple(b0.shape)} + {tuple(a1.shape)}x{tuple(b1.shape)}")
    return out0, out1


def gemm_pp_operands_ok(K, *mats):
    """The ping-pong 256x256 kernel wants whole pairs of 64-wide K tiles and 31-bit byte offsets over one 256-row panel of each
    (row-major) operand."""
    return K >= 128 and K % 128 == 0 and all(256 * m.stride(0) * 2 < 2 ** 31 - 2 ** 20 for m in mats)


def gemv_supported(x, w):
    """mm355_gemv_bf16 takes this (x [M, K], w [N, K]) pair: up to 4 rows always; 5 - 16 rows (the MFMA form; 17 - 32 on wide weights) only while the weight and
    the x rows are addressable with 32-bit byte offsets (< 3.75 GiB; gemv_mfma_addressable in csrc/decode.hip) -- beyond that the call
    returns MM355_EUNSUPPORTED and callers use the GEMM."""
    _, M, K, ldx = _rows2d(x)
    _, N, _, ldw = _rows2d(w)
    if M > 32 or (M > 16 and not gemv_rows32_units((N + 3) // 4)):
        return False
    return M <= 4 or ((N - 1) * ldw * 2 + K * 2 < 0xf0000000 and (M - 1) * ldx * 2 + K * 2 < 0xf0000000)


def gemv_rows32_units(units):
    """17 .. 32 rows ride on the MFMA GEMVs (two x row groups per workgroup) on shapes whose workgroups each own one K range -- more than
    1280 groups of four 4-row units (gemv_mfma_shape in csrc/decode.hip): gate|up (I / 2 units), lm_head (V / 4); not q|k|v, o, down."""
    return (units + 3) // 4 > 1280


def _gemv_out(x, M, N, out, bias, residual, gelu):
    """What every plain GEMV takes behind its weight: the output (made here if None) and the epilogue as (out, po, ldy, pr, ldr, flags)."""
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=BF16)
    po, Mo, No, ldy = _rows2d(out)
    assert (Mo, No) == (M, N)
    flags = GEMM_OUT_F32 if out.dtype == torch.float32 else 0
    pr, ldr = 0, 0
    if bias is not None:
        flags |= GEMM_BIAS
    if gelu is not None:
        flags |= {"erf": GEMM_GELU_ERF, "tanh": GEMM_GELU_TANH}[gelu]
    if residual is not None:
        pr, Mr, Nr, ldr = _rows2d(residual)
        assert (Mr, Nr) == (M, N)
        flags |= GEMM_RESIDUAL
    return out, po, ldy, pr, ldr, flags


def gemv(x, w, out=None, bias=None, residual=None, gelu=None):
    """out[M,N] = x[M,K] . w[N,K]^T for M <= 16 rows (decode shape): streams the weight once at HBM rate (1 - 2 rows: vector ALU; 3 - 16: MFMA)."""
    _chk_dev(x, w, out, bias, residual)
    px, M, K, ldx = _rows2d(x)
    pw, N, Kw, ldw = _rows2d(w)
    assert K == Kw and x.dtype == BF16 and w.dtype == BF16
    out, po, ldy, pr, ldr, flags = _gemv_out(x, M, N, out, bias, residual, gelu)
    _lib.check(_L().mm355_gemv_bf16(px, ldx, pw, ldw, po, ldy, M, N, K, _p(bias), pr, ldr, flags, _stream()), f"mm355_gemv_bf16 M={M} N={N} K={K}")
    return out


def gemv_swiglu(x, wgu, I, norm_w=None, eps=0.0, out=None):
    """act[M, I] = SiLU(g) * u, [g | u] = n . wgu^T, n = RMSNorm(x; norm_w, eps) (norm_w None: n = x); M <= 16 (decode shape)."""
    _chk_dev(x, wgu, norm_w, out)
    px, M, K, ldx = _rows2d(x)
    pw, N, Kw, ldw = _rows2d(wgu)
    assert K == Kw and N == 2 * I and x.dtype == BF16 and wgu.dtype == BF16
    out = torch.empty((M, I), device=x.device, dtype=BF16) if out is None else out
    _lib.check(_L().mm355_gemv_swiglu_bf16(px, ldx, pw, ldw, out.data_ptr(), out.stride(0), M, I, K, _p(norm_w), float(eps), _stream()),
               "mm355_gemv_swiglu_bf16")
    return out


def gemv_rope_append(x, wqkv, Hq, Hkv, d, cos, sin, positions, k_cache, v_cache, norm_w=None, eps=0.0, out=None):
    """The fused q|k|v projection of M <= 16 new rows (optionally of RMSNorm(x)), RoPE at positions[m] (int32, device), rotated k and v
    straight into cache row positions[m]; returns the row buffer [M, (Hq+2Hkv)*d] whose q columns are valid."""
    _chk_dev(x, wqkv, norm_w, cos, sin, positions, k_cache, v_cache, out)
    px, M, K, ldx = _rows2d(x)
    pw, N, Kw, ldw = _rows2d(wqkv)
    assert K == Kw and N == (Hq + 2 * Hkv) * d and positions.dtype == torch.int32
    assert k_cache.stride() == v_cache.stride() and k_cache.stride(2) == 1
    out = torch.empty((M, N), device=x.device, dtype=BF16) if out is None else out
    _lib.check(_L().mm355_gemv_rope_append_bf16(px, ldx, pw, ldw, out.data_ptr(), out.stride(0), M, Hq, Hkv, d, K, _p(norm_w), float(eps),
                                                cos.data_ptr(), sin.data_ptr(), positions.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                                                k_cache.stride(1), k_cache.stride(0), _stream()), "mm355_gemv_rope_append_bf16")
    return out


# ------------------------------------------------------------------------------------------------ weight-only FP8 (decode)

W8_E4M3 = 1                                                  # MM355_W8_E4M3
W8_FORMATS = {"fp8_e4m3": W8_E4M3}
E4M3_MAX = 448.0


def quantize_w8(w, pow2_scales=False):
    """w [N, K] -> (q uint8 [N, K], scale f32 [N]) of format "fp8_e4m3": scale[n] = amax_k |w[n, k]| / 448 (a row of zeros: 1; pow2_scales:
    rounded UP to a power of two, the dequantised weights are then exact in bf16), q = the OCP e4m3fn byte of RNE(w / scale), saturating at
    +-448, never a NaN encoding.  Not a hot path: torch ops, on whatever device w lives on."""
    assert w.dim() == 2
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    if pow2_scales:
        m, e = torch.frexp(scale)                            # scale = m * 2^e, m in [0.5, 1)
        scale = torch.where(m == 0.5, scale, torch.ldexp(torch.ones_like(scale), e))
    scale = scale.clamp_min(2.0 ** -126)
    q = (wf / scale[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).contiguous(), scale.contiguous()


def _w8_operands(wq, scale, K):
    assert wq.dtype == torch.uint8 and wq.dim() == 2 and wq.stride(1) == 1 and wq.shape[1] == K, (wq.dtype, wq.shape, K)
    assert scale.dtype == torch.float32 and scale.is_contiguous() and scale.numel() == wq.shape[0]
    return wq.data_ptr(), wq.shape[0], wq.stride(0) if wq.shape[0] > 1 else max(wq.stride(0), K)


# ------------------------------------------------------------------------------------------------ weight-only MXFP4 (decode)

W4_MXFP4 = 2                                                 # MM355_W4_MXFP4
W4_FORMATS = {"mxfp4": W4_MXFP4}
QUANT_FORMATS = {**W8_FORMATS, **W4_FORMATS}                 # what quantize_decoder_ accepts
E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)         # |value| of the codes 0 .. 7; bit 3 of a nibble is the sign


def quantize_w4(w):
    """w [N, K], K % 32 == 0 -> (q uint8 [N, K/2], s uint8 [N, K/32]) of format "mxfp4" (OCP MX): per group of 32 consecutive k the e8m0
    scale 2^e, e = clamp(floor(log2(amax)) - 2, -125, 125) stored as s = e + 127 (a group of zeros: e = 0), and per element the e2m1 code
    of RNE(w / 2^e) (ties to the even code, saturating at +-6) with the sign of w in bit 3; byte j of a row holds k = 2j in bits 3:0 and
    k = 2j+1 in bits 7:4.  Every dequantised value is exactly a bf16 value.  Not a hot path: torch ops, on whatever device w lives on."""
    assert w.dim() == 2 and w.shape[1] % 32 == 0, tuple(w.shape)
    N, K = w.shape
    wf = w.detach().float().view(N, K // 32, 32)
    amax = wf.abs().amax(dim=2)
    _, ex = torch.frexp(amax)                                # amax = m * 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
    e = torch.where(amax > 0, (ex - 3).clamp(-125, 125), torch.zeros_like(ex))
    v = torch.ldexp(wf.abs(), -e[:, :, None])                # exact: a power-of-two factor
    # RNE onto the grid: steps of 0.5 below 2, of 1 below 4, of 2 above; torch.round is half-to-even, which is the even CODE on every piece
    r = torch.where(v < 2, torch.round(v * 2) / 2, torch.where(v < 4, torch.round(v), torch.round(v / 2) * 2)).clamp_max(6.0)
    code = torch.bucketize(r, torch.tensor(E2M1_GRID, device=w.device, dtype=torch.float32)).to(torch.uint8)
    code = code | (torch.signbit(wf).to(torch.uint8) << 3)
    code = code.view(N, K // 2, 2)
    q = code[:, :, 0] | (code[:, :, 1] << 4)
    return q.contiguous(), (e + 127).to(torch.uint8).contiguous()


def dequant_w4_reference(q, s):
    """fp32 [N, K] of (q, s) in format "mxfp4", in torch ops (the definition; every value is exactly a bf16 value): what
    mm355_dequant_w4_bf16 writes and what the w4 GEMVs multiply."""
    N, K2 = q.shape
    grid = torch.tensor(E2M1_GRID + tuple(-g for g in E2M1_GRID), device=q.device, dtype=torch.float32)
    nib = torch.stack((q & 15, q >> 4), 2).view(N, K2 * 2).long()
    return torch.ldexp(grid[nib].view(N, K2 // 16, 32), (s.int() - 127)[:, :, None]).view(N, K2 * 2)


def _w4_operands(wq, s, K):
    assert K % 32 == 0, K
    assert wq.dtype == torch.uint8 and wq.dim() == 2 and wq.stride(1) == 1 and wq.shape[1] == K // 2, (wq.dtype, wq.shape, K)
    assert s.dtype == torch.uint8 and s.dim() == 2 and s.stride(1) == 1 and tuple(s.shape) == (wq.shape[0], K // 32), (s.dtype, s.shape, K)
    N = wq.shape[0]
    return wq.data_ptr(), N, (wq.stride(0) if N > 1 else max(wq.stride(0), K // 2)), s.data_ptr(), (s.stride(0) if N > 1 else max(s.stride(0), K // 32))


# ------------------------------------------------------------------------------------------------ one wrapper per quantised-weight operation

class _WFormat:
    """One weight-only format as the wrappers below need it: the suffix of its C symbols (mm355_gemv_<sfx>, mm355_gemm_<sfx>_norm, ...),
    weight columns per byte of wq, and `operands(wq, s, K)`: the format's own checks of the pair (wq, s) against K columns -> (N, the C
    operands that follow x in every call of the format, its MM355_* constant last)."""

    def __init__(self, sfx, cols_per_byte, operands):
        self.sfx, self.cols_per_byte, self.operands = sfx, cols_per_byte, operands

    def sym(self, pattern):
        """"gemv_{}" -> mm355_gemv_w8, "gemm_{}_norm" -> mm355_gemm_w8_norm: (the library's function, its name for messages)."""
        name = "mm355_" + pattern.format(self.sfx)
        return getattr(_L(), name), name


def _w8_c_operands(wq, scale, K):
    pw, N, ldw = _w8_operands(wq, scale, K)
    return N, (pw, ldw, scale.data_ptr(), W8_E4M3)


def _w4_c_operands(wq, s, K):
    pw, N, ldw, ps, lds = _w4_operands(wq, s, K)
    return N, (pw, ldw, ps, lds, W4_MXFP4)


_W8 = _WFormat("w8", 1, _w8_c_operands)
_W4 = _WFormat("w4", 2, _w4_c_operands)


def _wq_dequant(fmt, wq, s, out):
    _chk_dev(wq, s, out)
    K = wq.shape[1] * fmt.cols_per_byte
    N, cw = fmt.operands(wq, s, K)
    out = torch.empty((N, K), device=wq.device, dtype=BF16) if out is None else out
    assert out.dtype == BF16 and tuple(out.shape) == (N, K) and out.stride(1) == 1
    fn, name = fmt.sym("dequant_{}_bf16")
    _lib.check(fn(*cw, out.data_ptr(), out.stride(0) if N > 1 else max(out.stride(0), K), N, K, _stream()), f"{name} N={N} K={K}")
    return out


def _wq_gemv(fmt, x, wq, s, out, bias, residual, gelu):
    _chk_dev(x, wq, s, out, bias, residual)
    px, M, K, ldx = _rows2d(x)
    assert x.dtype == BF16
    N, cw = fmt.operands(wq, s, K)
    out, po, ldy, pr, ldr, flags = _gemv_out(x, M, N, out, bias, residual, gelu)
    fn, name = fmt.sym("gemv_{}")
    _lib.check(fn(px, ldx, *cw, po, ldy, M, N, K, _p(bias), pr, ldr, flags, _stream()), f"{name} M={M} N={N} K={K}")
    return out


def _wq_gemv_swiglu(fmt, x, wq, s, I, norm_w, eps, out):
    _chk_dev(x, wq, s, norm_w, out)
    px, M, K, ldx = _rows2d(x)
    assert x.dtype == BF16
    N, cw = fmt.operands(wq, s, K)
    assert N == 2 * I
    out = torch.empty((M, I), device=x.device, dtype=BF16) if out is None else out
    fn, name = fmt.sym("gemv_swiglu_{}")
    _lib.check(fn(px, ldx, *cw, out.data_ptr(), out.stride(0), M, I, K, _p(norm_w), float(eps), _stream()), name)
    return out


def _wq_gemv_rope_append(fmt, x, wq, s, Hq, Hkv, d, cos, sin, positions, k_cache, v_cache, norm_w, eps, out):
    _chk_dev(x, wq, s, norm_w, cos, sin, positions, k_cache, v_cache, out)
    px, M, K, ldx = _rows2d(x)
    assert x.dtype == BF16
    N, cw = fmt.operands(wq, s, K)
    assert N == (Hq + 2 * Hkv) * d and positions.dtype == torch.int32
    assert k_cache.stride() == v_cache.stride() and k_cache.stride(2) == 1
    out = torch.empty((M, N), device=x.device, dtype=BF16) if out is None else out
    fn, name = fmt.sym("gemv_rope_append_{}")
    _lib.check(fn(px, ldx, *cw, out.data_ptr(), out.stride(0), M, Hq, Hkv, d, K, _p(norm_w), float(eps), cos.data_ptr(), sin.data_ptr(),
                  positions.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(1), k_cache.stride(0), _stream()), name)
    return out


def _wq_gemm_supported(M, K):
    return K % 64 == 0 and 0 < M <= 4096


def _wq_ws(fmt, query, device, *mnk):
    """The fp32 workspace a GEMM form asks for at this problem: (tensor, floats)."""
    n_ws = int(fmt.sym(query)[0](*mnk))
    return _splitk_ws(n_ws, device), n_ws


def _wq_gemm(fmt, x, wq, s, residual, out, out_f32):
    _chk_dev(x, wq, s, residual, out)
    px, M, K, ldx = _rows2d(x)
    assert x.dtype == BF16
    N, cw = fmt.operands(wq, s, K)
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=torch.float32 if out_f32 else BF16)
    po, Mo, No, ldc = _rows2d(out)
    assert (Mo, No) == (M, N) and out.dtype in (BF16, torch.float32)
    flags = GEMM_OUT_F32 if out.dtype == torch.float32 else 0
    pr, ldr = 0, 0
    if residual is not None:
        pr, Mr, Nr, ldr = _rows2d(residual)
        assert (Mr, Nr) == (M, N) and residual.dtype == BF16
        flags |= GEMM_RESIDUAL
    ws, n_ws = (_splitk_ws(0, x.device), 0) if flags & GEMM_OUT_F32 else _wq_ws(fmt, "gemm_{}_ws_floats", x.device, M, N, K)
    fn, name = fmt.sym("gemm_{}")
    _lib.check(fn(px, ldx, *cw, po, ldc, M, N, K, pr, ldr, flags, ws.data_ptr(), n_ws, _stream()), f"{name} M={M} N={N} K={K}")
    return out


def _wq_gemm_norm(fmt, x, wq, s, norm_w, eps, residual):
    _chk_dev(x, wq, s, norm_w, residual)
    px, M, K, ldx = _rows2d(x)
    N, cw = fmt.operands(wq, s, K)
    assert x.dtype == BF16 and norm_w.numel() == N
    c = torch.empty((M, N), device=x.device, dtype=BF16)
    y = torch.empty((M, N), device=x.device, dtype=BF16)
    pr, ldr = 0, 0
    if residual is not None:
        pr, Mr, Nr, ldr = _rows2d(residual)
        assert (Mr, Nr) == (M, N)
    ws, n_ws = _wq_ws(fmt, "gemm_{}_ws_floats", x.device, M, N, K)
    fn, name = fmt.sym("gemm_{}_norm")
    _lib.check(fn(px, ldx, *cw, c.data_ptr(), M, N, K, pr, ldr, norm_w.data_ptr(), float(eps), y.data_ptr(), ws.data_ptr(), n_ws, _stream()),
               f"{name} M={M} N={N} K={K}")
    return c, y


def _wq_gemm_swiglu(fmt, x, wq, s, I):
    _chk_dev(x, wq, s)
    px, M, K, ldx = _rows2d(x)
    N, cw = fmt.operands(wq, s, K)
    assert N == 2 * I and x.dtype == BF16
    act = torch.empty((M, I), device=x.device, dtype=BF16)
    ws, n_ws = _wq_ws(fmt, "gemm_{}_swiglu_ws_floats", x.device, M, I, K)
    fn, name = fmt.sym("gemm_{}_swiglu")
    _lib.check(fn(px, ldx, *cw, act.data_ptr(), act.stride(0), M, I, K, ws.data_ptr(), n_ws, _stream()), f"{name} M={M} I={I} K={K}")
    return act


def _wq_gemm_rope_append(fmt, x, wq, s, Hq, Hkv, d, cos, sin, positions, k_cache, v_cache):
    _chk_dev(x, wq, s, cos, sin, positions, k_cache, v_cache)
    px, M, K, ldx = _rows2d(x)
    N, cw = fmt.operands(wq, s, K)
    assert x.dtype == BF16 and N == (Hq + 2 * Hkv) * d and positions.dtype == torch.int32
    assert k_cache.stride() == v_cache.stride() and k_cache.stride(2) == 1
    out = torch.empty((M, N), device=x.device, dtype=BF16)
    ws, n_ws = _wq_ws(fmt, "gemm_{}_ws_floats", x.device, M, N, K)
    fn, name = fmt.sym("gemm_{}_rope_append")
    _lib.check(fn(px, ldx, *cw, out.data_ptr(), out.stride(0), M, Hq, Hkv, d, K, cos.data_ptr(), sin.data_ptr(), positions.data_ptr(),
                  k_cache.data_ptr(), v_cache.data_ptr(), k_cache.stride(1), k_cache.stride(0), ws.data_ptr(), n_ws, _stream()), name)
    return out


# ---- the public names: format "fp8_e4m3" (e4m3 bytes wq [N, K], one fp32 scale per row) ...

def dequant_w8(wq, scale, out=None):
    """bf16 [N, K] = RNE(fp32(wq) * scale[:, None]) (mm355_dequant_w8_bf16): the operand of the bf16 GEMMs on the routes gemm_w8* do not take."""
    return _wq_dequant(_W8, wq, scale, out)


def gemv_w8(x, wq, scale, out=None, bias=None, residual=None, gelu=None):
    """out[M,N] = epilogue(scale[n] * x[M,K] . fp32(wq[N,K])^T) for M <= 16 rows: gemv() over e4m3 weight bytes with one fp32 scale per row."""
    return _wq_gemv(_W8, x, wq, scale, out, bias, residual, gelu)


def gemv_swiglu_w8(x, wq, scale, I, norm_w=None, eps=0.0, out=None):
    """gemv_swiglu() over the e4m3 bytes of the fused gate|up weight."""
    return _wq_gemv_swiglu(_W8, x, wq, scale, I, norm_w, eps, out)


def gemv_rope_append_w8(x, wq, scale, Hq, Hkv, d, cos, sin, positions, k_cache, v_cache, norm_w=None, eps=0.0, out=None):
    """gemv_rope_append() over the e4m3 bytes of the fused q|k|v weight."""
    return _wq_gemv_rope_append(_W8, x, wq, scale, Hq, Hkv, d, cos, sin, positions, k_cache, v_cache, norm_w, eps, out)


def gemm_w8_supported(M, K):
    """mm355_gemm_w8* take this problem (whole 64-wide K tiles, at most 4096 rows)."""
    return _wq_gemm_supported(M, K)


def gemm_w8(x, wq, scale, residual=None, out=None, out_f32=False):
    """out[M, N] = scale[n] * x[M, K] . fp32(wq[N, K])^T (+ residual): gemm_splitk() over e4m3 weight bytes (mm355_gemm_w8) -- the same K
    slices and summation order, the bytes widened in registers.  out_f32 (or an fp32 `out`): fp32 output in one slice (the lm_head)."""
    return _wq_gemm(_W8, x, wq, scale, residual, out, out_f32)


def gemm_w8_norm(x, wq, scale, norm_w, eps, residual=None):
    """gemm_splitk_norm() over e4m3 weight bytes (mm355_gemm_w8_norm): (c, y)."""
    return _wq_gemm_norm(_W8, x, wq, scale, norm_w, eps, residual)


def gemm_w8_swiglu(x, wq, scale, I):
    """gemm_splitk_swiglu() over the e4m3 bytes of the fused gate|up weight (mm355_gemm_w8_swiglu)."""
    return _wq_gemm_swiglu(_W8, x, wq, scale, I)


def gemm_w8_rope_append(x, wq, scale, Hq, Hkv, d, cos, sin, positions, k_cache, v_cache):
    """gemm_splitk_rope_append() over the e4m3 bytes of the fused q|k|v weight (mm355_gemm_w8_rope_append)."""
    return _wq_gemm_rope_append(_W8, x, wq, scale, Hq, Hkv, d, cos, sin, positions, k_cache, v_cache)


# ---- ... and format "mxfp4" (e2m1 nibbles wq [N, K/2], e8m0 group scales s [N, K/32])

def dequant_w4(wq, s, out=None):
    """bf16 [N, K] of (wq, s) in format "mxfp4", exact (mm355_dequant_w4_bf16): the operand of the bf16 GEMMs on the routes gemm_w4* do not take."""
    return _wq_dequant(_W4, wq, s, out)


def gemv_w4(x, wq, s, out=None, bias=None, residual=None, gelu=None):
    """out[M,N] = epilogue(x[M,K] . Wd[N,K]^T) for M <= 16 rows: gemv() over MXFP4 weights (e2m1 nibbles wq [N, K/2], e8m0 group scales s [N, K/32])."""
    return _wq_gemv(_W4, x, wq, s, out, bias, residual, gelu)


def gemv_swiglu_w4(x, wq, s, I, norm_w=None, eps=0.0, out=None):
    """gemv_swiglu() over the MXFP4 form of the fused gate|up weight."""
    return _wq_gemv_swiglu(_W4, x, wq, s, I, norm_w, eps, out)


def gemv_rope_append_w4(x, wq, s, Hq, Hkv, d, cos, sin, positions, k_cache, v_cache, norm_w=None, eps=0.0, out=None):
    """gemv_rope_append() over the MXFP4 form of the fused q|k|v weight."""
    return _wq_gemv_rope_append(_W4, x, wq, s, Hq, Hkv, d, cos, sin, positions, k_cache, v_cache, norm_w, eps, out)


def gemm_w4_supported(M, K):
    """mm355_gemm_w4* take this problem (whole 64-wide K tiles, at most 4096 rows)."""
    return _wq_gemm_supported(M, K)


def gemm_w4(x, wq, s, residual=None, out=None, out_f32=False):
    """out[M, N] = x[M, K] . Wd[N, K]^T (+ residual): gemm_splitk() over MXFP4 weights (mm355_gemm_w4; e2m1 nibbles wq [N, K/2], e8m0 group
    scales s [N, K/32]) -- the same K slices and summation order, the nibbles widened in registers with the scale inside the conversion:
    the bits of gemm_splitk(x, dequant_w4(wq, s)).  out_f32 (or an fp32 `out`): fp32 output in one slice."""
    return _wq_gemm(_W4, x, wq, s, residual, out, out_f32)


def gemm_w4_norm(x, wq, s, norm_w, eps, residual=None):
    """gemm_splitk_norm() over MXFP4 weights (mm355_gemm_w4_norm): (c, y)."""
    return _wq_gemm_norm(_W4, x, wq, s, norm_w, eps, residual)


def gemm_w4_swiglu(x, wq, s, I):
    """gemm_splitk_swiglu() over the MXFP4 form of the fused gate|up weight (mm355_gemm_w4_swiglu)."""
    return _wq_gemm_swiglu(_W4, x, wq, s, I)


def gemm_w4_rope_append(x, wq, s, Hq, Hkv, d, cos, sin, positions, k_cache, v_cache):
    """gemm_splitk_rope_append() over the MXFP4 form of the fused q|k|v weight (mm355_gemm_w4_rope_append)."""
    return _wq_gemm_rope_append(_W4, x, wq, s, Hq, Hkv, d, cos, sin, positions, k_cache, v_cache)


# ------------------------------------------------------------------------------------------------ FP8 KV cache (decode)

KV8_E4M3 = 1                                                 # MM355_KV8_E4M3
KV_FORMATS = ("bf16", "fp8_e4m3")


def quantize_kv8(rows, Hkv, d):
    """rows [..., Hkv*d] bf16 -> (q uint8 [..., Hkv*d], scale f32 [..., Hkv]) of KV format "fp8_e4m3": per head-row (the d values of one KV
    head of one token) scale = the smallest power of two with amax / scale <= 448 (zeros: 1), q = the OCP e4m3fn byte of RNE(x / scale) -- an
    exact shift, nothing saturates.  The contract mm355_kv_quant_f8 / mm355_rope_kv_append_f8 are tested against.  Not a hot path: torch ops,
    on whatever device rows lives on."""
    assert rows.dtype == BF16 and rows.shape[-1] == Hkv * d
    x = rows.detach().float().reshape(*rows.shape[:-1], Hkv, d)
    amax = x.abs().amax(dim=-1)
    m, e = torch.frexp(amax)                                 # amax = m * 2^e, m in [0.5, 1); 448 = 0.875 * 2^9
    sh = torch.where(amax > 0, e - 9 + (m > 0.875).to(e.dtype), torch.zeros_like(e))
    q = torch.ldexp(x, -sh[..., None]).to(torch.float8_e4m3fn)
    scale = torch.ldexp(torch.ones_like(amax), sh)
    return q.view(torch.uint8).reshape(rows.shape).contiguous(), scale.contiguous()


def dequant_kv8(q, scale, Hkv, d):
    """bf16 [..., Hkv*d] = fp32(q) * scale per head-row: exact, and exactly a bf16 value (torch ops: tests and tools)."""
    assert q.dtype == torch.uint8 and q.shape[-1] == Hkv * d and scale.shape[-1] == Hkv
    x = q.contiguous().view(torch.float8_e4m3fn).float().reshape(*q.shape[:-1], Hkv, d) * scale.float()[..., None]
    return x.reshape(q.shape).to(BF16)


def _kv8_cache(c8, sc, Hkv, d):
    """(ld bytes, batch stride bytes, ld scale, batch stride scale) of a cache [B, Lmax, Hkv*d] uint8 with scales [B, Lmax, Hkv] f32"""
    assert c8.dtype == torch.uint8 and c8.dim() == 3 and c8.shape[2] == Hkv * d and c8.stride(2) == 1, (c8.dtype, c8.shape, c8.stride())
    assert sc.dtype == torch.float32 and sc.dim() == 3 and tuple(sc.shape) == (c8.shape[0], c8.shape[1], Hkv) and sc.stride(2) == 1
    return c8.stride(1), c8.stride(0), sc.stride(1), sc.stride(0)


def kv_quant_f8(src, Hkv, d, dst, dst_scale, row0=0, rows_per_seq=None):
    """src [R, Hkv*d] bf16 (already rotated; may be a column block of a wider tensor) -> cache rows: source row r goes to row
    row0 + r % rows_per_seq of sequence r // rows_per_seq of dst [B, Lmax, Hkv*d] uint8 / dst_scale [B, Lmax, Hkv] f32
    (mm355_kv_quant_f8; rows_per_seq None: all rows belong to sequence 0)."""
    _chk_dev(src, dst, dst_scale)
    ps, R, W, lds = _rows2d(src)
    assert src.dtype == BF16 and W == Hkv * d
    ldb, bsb, ldsc, bssc = _kv8_cache(dst, dst_scale, Hkv, d)
    rps = R if rows_per_seq is None else int(rows_per_seq)
    assert R % rps == 0 and R // rps <= dst.shape[0] and row0 + rps <= dst.shape[1], (R, rps, row0, dst.shape)
    _lib.check(_L().mm355_kv_quant_f8(ps, lds, R, rps, Hkv, d, dst.data_ptr(), ldb, dst_scale.data_ptr(), ldsc, bsb, bssc, int(row0), KV8_E4M3,
                                      _stream()), f"mm355_kv_quant_f8 R={R} Hkv={Hkv} d={d}")


# ------------------------------------------------------------------------------------------------ one wrapper per KV-cache operation

class _KVFormat:
    """One KV-cache format as the wrappers below need it: the suffix of its C symbols and of the public names (mm355_attn_extend<sfx>,
    ops.attn_extend<sfx>), `cache(kv, B, Hkv, d)`: the format's own checks of its cache tensors kv (bf16: k, v; e4m3: k8, v8, k_scale,
    v_scale) for B sequences -> (rows, the C operands that describe the cache in every call of the format, its MM355_* constant last), and
    `prefix(sh, Hkv, d)`: the same for the rows of a prefix stored once (k_shared, v_shared and, e4m3, their scales)."""

    def __init__(self, sfx, cache, prefix):
        self.sfx, self.cache, self.prefix = sfx, cache, prefix

    def sym(self, pattern):
        """"attn_extend{}" -> mm355_attn_extend_f8: (the library's function, its name for messages)."""
        name = "mm355_" + pattern.format(self.sfx)
        return getattr(_L(), name), name


def _bf16_kv_operands(kv, B, Hkv, d):
    """k / v [>= B, rows, Hkv*d] bf16 with the same strides"""
    k, v = kv
    assert k.dim() == 3 and k.dtype == BF16 and k.shape == v.shape and k.stride(2) == 1 and v.stride() == k.stride() and k.shape[2] == Hkv * d
    assert k.shape[0] >= B
    return k.shape[1], (k.data_ptr(), v.data_ptr(), k.stride(1), k.stride(0))


def _f8_kv_operands(kv, B, Hkv, d):
    """_kv8_cache() of two caches [>= B, rows, Hkv*d] with the same strides"""
    k8, v8, k_scale, v_scale = kv
    assert k8.shape == v8.shape and k8.stride() == v8.stride() and k_scale.stride() == v_scale.stride() and k8.shape[0] >= B
    _kv8_cache(v8, v_scale, Hkv, d)
    ldb, bsb, ldsc, bssc = _kv8_cache(k8, k_scale, Hkv, d)
    return k8.shape[1], (k8.data_ptr(), v8.data_ptr(), ldb, bsb, k_scale.data_ptr(), v_scale.data_ptr(), ldsc, bssc, KV8_E4M3)


def _bf16_prefix_operands(sh, Hkv, d, dtype=BF16):
    """the prefix stored once: k_shared / v_shared [rows, Hkv*d] of `dtype` with the same strides"""
    k_sh, v_sh = sh
    assert k_sh.dim() == 2 and k_sh.dtype == dtype and k_sh.shape == v_sh.shape and k_sh.stride() == v_sh.stride()
    assert k_sh.stride(1) == 1 and k_sh.shape[1] == Hkv * d
    return k_sh.shape[0], (k_sh.data_ptr(), v_sh.data_ptr(), k_sh.stride(0))


def _f8_prefix_operands(sh, Hkv, d):
    """_bf16_prefix_operands() of e4m3 bytes, and their scales [rows, Hkv] f32"""
    rows, csh = _bf16_prefix_operands(sh[:2], Hkv, d, torch.uint8)
    ks, vs = sh[2:]
    assert ks.dtype == torch.float32 and tuple(ks.shape) == (rows, Hkv) and ks.stride(1) == 1
    assert vs.dtype == torch.float32 and vs.shape == ks.shape and vs.stride() == ks.stride()
    return rows, (*csh, ks.data_ptr(), vs.data_ptr(), ks.stride(0))


_KV_BF16 = _KVFormat("", _bf16_kv_operands, _bf16_prefix_operands)
_KV_F8 = _KVFormat("_f8", _f8_kv_operands, _f8_prefix_operands)


def _kv_rope_append(fmt, qkv, Hq, Hkv, d, cos, sin, positions, kv):
    _chk_dev(qkv, cos, sin, positions, *kv)
    assert positions.dtype == torch.int32
    B = qkv.shape[0]
    _, ckv = fmt.cache(kv, B, Hkv, d)
    fn, name = fmt.sym("rope_kv_append{}")
    _lib.check(fn(qkv.data_ptr(), qkv.stride(0), B, Hq, Hkv, d, cos.data_ptr(), sin.data_ptr(), positions.data_ptr(), *ckv, _stream()), name)
    return qkv


def _row_tables(qkv, positions, blocks, n_blocks):
    """positions / blocks int32 [R] of the rows of qkv (blocks None: block r for row r) -> the blocks pointer"""
    R = qkv.shape[0]
    assert positions.dtype == torch.int32 and positions.dim() == 1 and positions.shape[0] == R and positions.is_contiguous()
    if blocks is None:
        assert n_blocks >= R, (n_blocks, R)
        return None
    assert blocks.dtype == torch.int32 and blocks.dim() == 1 and blocks.shape[0] == R and blocks.is_contiguous()
    return blocks.data_ptr()


def _kv_rope_append_rows(fmt, qkv, Hq, Hkv, d, cos, sin, positions, blocks, kv):
    _chk_dev(qkv, cos, sin, positions, blocks, *kv)
    rows, ckv = fmt.cache(kv, 0, Hkv, d)                      # (any number of blocks: the table names them)
    n_blocks = kv[0].shape[0]
    pb = _row_tables(qkv, positions, blocks, n_blocks)
    fn, name = fmt.sym("rope_kv_append_rows{}")
    _lib.check(fn(qkv.data_ptr(), qkv.stride(0), qkv.shape[0], Hq, Hkv, d, cos.data_ptr(), sin.data_ptr(), positions.data_ptr(), pb, n_blocks,
                  rows, *ckv, _stream()), name)
    return qkv


def _kv_attn_decode(fmt, q, kv, kv_lens, max_kv_len, Hq, Hkv, d, scale, out, workspace, variant):
    _chk_dev(q, *kv, kv_lens)
    B = q.shape[0]
    rows, ckv = fmt.cache(kv, B, Hkv, d)
    assert kv_lens.dtype == torch.int32 and max_kv_len <= rows
    out = torch.empty((B, Hq * d), device=q.device, dtype=BF16) if out is None else out
    ws = workspace
    if ws is None:
        ws = torch.zeros(int(_L().mm355_attn_decode_ws_floats(B, Hq, d, max_kv_len)), device=q.device, dtype=torch.float32)   # arrival counters start at 0
    _, name = fmt.sym("attn_decode{}")
    _lib.check(getattr(_L(), name + "_variant")(q.data_ptr(), q.stride(0), *ckv, kv_lens.data_ptr(), max_kv_len, out.data_ptr(), out.stride(0), B,
                                                Hq, Hkv, d, scale, ws.data_ptr(), int(variant), _stream()), name)
    return out


def _cache_attn_args(q, lens, n, max_kv_len, rows, Hq, Hkv, d, out, workspace, ws_floats, shared_len=None, shared_rows=None, row_start=None):
    """What the cache-attention wrappers below hand to the C side: n query rows per sequence (None: the decode forms, one row and no such
    argument), lens the entry point's int32 [B] (past or kv_lens), ws_floats the name of its mm355_*_ws_floats, shared_len / shared_rows
    where a prefix is stored once.  row_start (the ragged forms): int32 [B + 1] on the device next to lens, sequence b brings the rows
    row_start[b] .. row_start[b + 1] - 1 of q, at most n >= 1 of them.  -> (B, q pointer, ld, out, its pointer, ld, workspace or None, its
    floats)"""
    B = lens.shape[0]
    pq, R, W, ldq = _rows2d(q)
    nn, sh = (() if n is None else (n,)), (() if shared_len is None else (shared_len,))      # what the entry point takes of the two
    assert q.dtype == BF16 and (R == B * (n or 1) or row_start is not None) and W == Hq * d, (q.shape, B, *nn, Hq, d)
    assert row_start is None or (n >= 1 and row_start.dtype == torch.int32 and row_start.dim() == 1 and row_start.shape[0] == B + 1 and
                                 row_start.is_contiguous()), (n, row_start.dtype, row_start.shape, B)
    assert lens.dtype == torch.int32 and (n is None or n <= max_kv_len) and max_kv_len <= rows and \
        (shared_len is None or 0 <= shared_len <= max_kv_len and shared_len <= shared_rows), (*nn, *sh, max_kv_len, rows)
    out = torch.empty((R, W), device=q.device, dtype=BF16) if out is None else out
    po, Ro, Wo, ldo = _rows2d(out)
    assert out.dtype == BF16 and (Ro, Wo) == (R, W)
    n_ws = int(getattr(_L(), ws_floats)(B, *nn, Hq, Hkv, d, *sh, max_kv_len))
    ws = workspace
    if n_ws and (ws is None or ws.numel() < n_ws):
        ws = torch.empty(n_ws, device=q.device, dtype=torch.float32)
    return B, pq, ldq, out, po, ldo, ws, (0 if ws is None else ws.numel())


def _kv_attn_extend(fmt, q, kv, past, n, max_kv_len, Hq, Hkv, d, scale, out, workspace):
    _chk_dev(q, *kv, past, out)
    rows, ckv = fmt.cache(kv, past.shape[0], Hkv, d)
    B, pq, ldq, out, po, ldo, ws, n_ws = _cache_attn_args(q, past, n, max_kv_len, rows, Hq, Hkv, d, out, workspace, "mm355_attn_extend_ws_floats")
    fn, name = fmt.sym("attn_extend{}")
    _lib.check(fn(pq, ldq, *ckv, past.data_ptr(), n, max_kv_len, po, ldo, B, Hq, Hkv, d, scale, _p(ws), n_ws, _stream()),
               f"{name} B={B} n={n} Hq={Hq} Hkv={Hkv} d={d}")
    return out


def _kv_attn_extend_ragged(fmt, q, kv, past, row_start, n_max, max_kv_len, Hq, Hkv, d, scale, out, workspace):
    _chk_dev(q, *kv, past, row_start, out)
    rows, ckv = fmt.cache(kv, past.shape[0], Hkv, d)
    B, pq, ldq, out, po, ldo, ws, n_ws = _cache_attn_args(q, past, n_max, max_kv_len, rows, Hq, Hkv, d, out, workspace,
                                                          "mm355_attn_extend_ragged_ws_floats", row_start=row_start)
    R = q.shape[0]
    fn, name = fmt.sym("attn_extend_ragged{}")
    _lib.check(fn(pq, ldq, *ckv, past.data_ptr(), row_start.data_ptr(), n_max, R, max_kv_len, po, ldo, B, Hq, Hkv, d, scale, _p(ws), n_ws,
                  _stream()), f"{name} B={B} n_max={n_max} rows={R} Hq={Hq} Hkv={Hkv} d={d}")
    return out


def _own_block(own_block, B):
    """the table of mm355_attn_decode_shared_idx: uint8 [>= B, columns] on the device, rows contiguous -> (pointer, row stride)"""
    assert own_block.dtype == torch.uint8 and own_block.dim() == 2 and own_block.stride(1) == 1 and own_block.shape[0] >= B and B <= 255
    assert own_block.shape[1] >= 1
    return own_block.data_ptr(), own_block.stride(0)


def _kv_attn_shared(fmt, q, sh, kv, lens, n, shared_len, max_kv_len, Hq, Hkv, d, scale, out, workspace, own_block=None):
    """attention over a prefix stored once (sh) and every sequence's own rows (kv): n None: the decode step, one row per sequence and lens
    = kv_lens (mm355_attn_decode_shared, with own_block mm355_attn_decode_shared_idx); else n rows per sequence and lens = past
    (mm355_attn_extend_shared)."""
    _chk_dev(q, *sh, *kv, lens, out, own_block)
    rows, ckv = fmt.cache(kv, lens.shape[0], Hkv, d)
    shared_rows, csh = fmt.prefix(sh, Hkv, d)
    op = "attn_decode_shared" if n is None else "attn_extend_shared"
    B, pq, ldq, out, po, ldo, ws, n_ws = _cache_attn_args(q, lens, n, max_kv_len, rows, Hq, Hkv, d, out, workspace, f"mm355_{op}_ws_floats",
                                                          shared_len, shared_rows)
    nn, tbl = (() if n is None else (n,)), (() if own_block is None else _own_block(own_block, B))
    fn, name = fmt.sym(op + ("_idx{}" if tbl else "{}"))
    _lib.check(fn(pq, ldq, *csh, *ckv, lens.data_ptr(), *tbl, *nn, shared_len, max_kv_len, po, ldo, B, Hq, Hkv, d, scale, _p(ws), n_ws, _stream()),
               f"{name} B={B}{''.join(f' n={v}' for v in nn)} Hq={Hq} Hkv={Hkv} d={d} shared_len={shared_len}")
    return out


# ------------------------------------------------------------------------------------------------ the KV-cache operations by name, per format

def rope_kv_append_(qkv, Hq, Hkv, d, cos, sin, positions, k_cache, v_cache):
    """qkv [B, (Hq+2Hkv)*d] new rows: rotate q (in place) and k at positions[b] (int32, device); k, v -> cache row positions[b]."""
    return _kv_rope_append(_KV_BF16, qkv, Hq, Hkv, d, cos, sin, positions, (k_cache, v_cache))


def rope_kv_append_f8_(qkv, Hq, Hkv, d, cos, sin, positions, k8, v8, k_scale, v_scale):
    """rope_kv_append_() into an e4m3 cache: q rotated in place (the same bits), the rotated k row (rounded to bf16 as the bf16 cache would
    hold it) and the v row quantised into row positions[b] of k8 / v8 [B, Lmax, Hkv*d] uint8 and k_scale / v_scale [B, Lmax, Hkv] f32."""
    return _kv_rope_append(_KV_F8, qkv, Hq, Hkv, d, cos, sin, positions, (k8, v8, k_scale, v_scale))


def rope_kv_append_rows_(qkv, Hq, Hkv, d, cos, sin, positions, blocks, k_cache, v_cache):
    """rope_kv_append_() with a block per row (mm355_rope_kv_append_rows): qkv [R, (Hq+2Hkv)*d] new rows, any R: q (in place) and k rotated at
    positions[r]; k, v -> row positions[r] of block blocks[r] of k_cache / v_cache [blocks, rows, Hkv*d] (int32 [R] each, on the device;
    blocks None: block r).  Out-of-range entries are clamped into the cache."""
    return _kv_rope_append_rows(_KV_BF16, qkv, Hq, Hkv, d, cos, sin, positions, blocks, (k_cache, v_cache))


def rope_kv_append_rows_f8_(qkv, Hq, Hkv, d, cos, sin, positions, blocks, k8, v8, k_scale, v_scale):
    """rope_kv_append_rows_() into an e4m3 cache (mm355_rope_kv_append_rows_f8): bytes and scales of row positions[r] of block blocks[r],
    quantised as rope_kv_append_f8_() quantises them."""
    return _kv_rope_append_rows(_KV_F8, qkv, Hq, Hkv, d, cos, sin, positions, blocks, (k8, v8, k_scale, v_scale))


def attn_decode(q, k_cache, v_cache, kv_lens, max_kv_len, Hq, Hkv, d, scale, out=None, workspace=None, variant=0):
    """q [B, Hq*d]; caches [B, Lmax, Hkv*d]; kv_lens int32 [B] on the device (valid rows incl. the current one)."""
    return _kv_attn_decode(_KV_BF16, q, (k_cache, v_cache), kv_lens, max_kv_len, Hq, Hkv, d, scale, out, workspace, variant)


def attn_decode_f8(q, k8, v8, k_scale, v_scale, kv_lens, max_kv_len, Hq, Hkv, d, scale, out=None, workspace=None, variant=0):
    """attn_decode() over an e4m3 cache: k8 / v8 [B, Lmax, Hkv*d] uint8, k_scale / v_scale [B, Lmax, Hkv] f32 (variants 0 and 2)."""
    return _kv_attn_decode(_KV_F8, q, (k8, v8, k_scale, v_scale), kv_lens, max_kv_len, Hq, Hkv, d, scale, out, workspace, variant)


def attn_extend(q, k, v, past, n, max_kv_len, Hq, Hkv, d, scale, out=None, workspace=None):
    """n new rows per sequence against a filled cache (mm355_attn_extend): q [B*n, Hq*d] bf16, already rotated, row (b, i) at b*n + i (may be
    a column block of a wider tensor); k / v [B, rows, Hkv*d] bf16 already holding the chunk's own rows at past[b] .. past[b]+n-1; past int32
    [B] on the device; max_kv_len a host bound with past[b] + n <= max_kv_len <= rows.  Row (b, i) attends the keys j <= past[b] + i."""
    return _kv_attn_extend(_KV_BF16, q, (k, v), past, n, max_kv_len, Hq, Hkv, d, scale, out, workspace)


def attn_extend_f8(q, k8, v8, k_scale, v_scale, past, n, max_kv_len, Hq, Hkv, d, scale, out=None, workspace=None):
    """attn_extend() over an e4m3 cache: k8 / v8 [B, rows, Hkv*d] uint8, k_scale / v_scale [B, rows, Hkv] f32 (mm355_attn_extend_f8): equal to
    attn_extend() on dequant_kv8() of the cache bit for bit."""
    return _kv_attn_extend(_KV_F8, q, (k8, v8, k_scale, v_scale), past, n, max_kv_len, Hq, Hkv, d, scale, out, workspace)


def attn_extend_supported(Hq, Hkv, d):
    """the head shapes mm355_attn_extend takes (else MM355_EUNSUPPORTED): d % 8 == 0, d <= 128, a GQA group of 1, 2, 4 or 8"""
    return d % 8 == 0 and d <= 128 and Hq % Hkv == 0 and Hq // Hkv in (1, 2, 4, 8)


def attn_extend_ragged_supported(Hq, Hkv, d):
    """the head shapes mm355_attn_extend_ragged takes (else MM355_EUNSUPPORTED): those of mm355_attn_extend"""
    return d % 8 == 0 and d <= 128 and Hq % Hkv == 0 and Hq // Hkv in (1, 2, 4, 8)


def attn_extend_ragged(q, k, v, past, row_start, n_max, max_kv_len, Hq, Hkv, d, scale, out=None, workspace=None):
    """n_b = row_start[b+1] - row_start[b] new rows of sequence b against its cache (mm355_attn_extend_ragged): q [rows, Hq*d] bf16, already
    rotated, the rows of sequence b packed at row_start[b] + i (may be a column block of a wider tensor); k / v [B, rows, Hkv*d] bf16 already
    holding them at past[b] .. past[b]+n_b-1; past int32 [B], row_start int32 [B + 1] on the device; n_max >= every n_b and max_kv_len >= every
    past[b] + n_b are host bounds.  Row (b, i) attends the keys j <= past[b] + i of block b; n_b == 0 and past[b] == 0 are right."""
    return _kv_attn_extend_ragged(_KV_BF16, q, (k, v), past, row_start, n_max, max_kv_len, Hq, Hkv, d, scale, out, workspace)


def attn_extend_ragged_f8(q, k8, v8, k_scale, v_scale, past, row_start, n_max, max_kv_len, Hq, Hkv, d, scale, out=None, workspace=None):
    """attn_extend_ragged() over an e4m3 cache: k8 / v8 [B, rows, Hkv*d] uint8, k_scale / v_scale [B, rows, Hkv] f32
    (mm355_attn_extend_ragged_f8): equal to attn_extend_ragged() on dequant_kv8() of the cache bit for bit."""
    return _kv_attn_extend_ragged(_KV_F8, q, (k8, v8, k_scale, v_scale), past, row_start, n_max, max_kv_len, Hq, Hkv, d, scale, out, workspace)


def attn_decode_shared_supported(Hq, Hkv, d):
    """the head shapes mm355_attn_decode_shared takes (else MM355_EUNSUPPORTED): d % 8 == 0, d <= 128, a GQA group of 1, 2, 4 or 8"""
    return d % 8 == 0 and d <= 128 and Hq % Hkv == 0 and Hq // Hkv in (1, 2, 4, 8)


def attn_decode_shared(q, k_shared, v_shared, k_cache, v_cache, kv_lens, shared_len, max_kv_len, Hq, Hkv, d, scale, out=None, workspace=None,
                       own_block=None):
    """The decode step's attention for B sequences whose first shared_len cached rows are the same rows, stored once
    (mm355_attn_decode_shared): q [B, Hq*d] bf16, already rotated (may be a column block of a wider tensor); k_shared / v_shared [>= shared_len,
    Hkv*d] bf16; k_cache / v_cache [B, rows, Hkv*d] bf16 whose rows [shared_len, kv_lens[b]) are sequence b's own; kv_lens int32 [B] on the
    device, kv_lens[b] >= shared_len; shared_len and max_kv_len host bounds.  Rows [0, shared_len) of the own blocks are never read.
    own_block (uint8 [B, columns] on the device; the beams of a beam search): own row j of query b is row j of block own_block[b, j -
    shared_len] (mm355_attn_decode_shared_idx); None is the identity."""
    return _kv_attn_shared(_KV_BF16, q, (k_shared, v_shared), (k_cache, v_cache), kv_lens, None, shared_len, max_kv_len, Hq, Hkv, d, scale, out,
                           workspace, own_block)


def attn_decode_shared_f8(q, k_shared, v_shared, k_shared_scale, v_shared_scale, k8, v8, k_scale, v_scale, kv_lens, shared_len, max_kv_len, Hq,
                          Hkv, d, scale, out=None, workspace=None, own_block=None):
    """attn_decode_shared() over e4m3 bytes: k_shared / v_shared [>= shared_len, Hkv*d] uint8 with scales [>= shared_len, Hkv] f32, k8 / v8 [B,
    rows, Hkv*d] uint8 with k_scale / v_scale [B, rows, Hkv] f32 (mm355_attn_decode_shared_f8): equal to attn_decode_shared() on dequant_kv8()
    of the same bytes bit for bit.  own_block: as for attn_decode_shared (mm355_attn_decode_shared_idx_f8), bytes and scales follow it."""
    return _kv_attn_shared(_KV_F8, q, (k_shared, v_shared, k_shared_scale, v_shared_scale), (k8, v8, k_scale, v_scale), kv_lens, None, shared_len,
                           max_kv_len, Hq, Hkv, d, scale, out, workspace, own_block)


def attn_extend_shared_supported(Hq, Hkv, d):
    """the head shapes mm355_attn_extend_shared takes (else MM355_EUNSUPPORTED): those of mm355_attn_decode_shared"""
    return attn_decode_shared_supported(Hq, Hkv, d)


def attn_extend_shared(q, k_shared, v_shared, k_cache, v_cache, past, n, shared_len, max_kv_len, Hq, Hkv, d, scale, out=None, workspace=None):
    """n new rows per sequence for B sequences whose first shared_len cached rows are the same rows, stored once (mm355_attn_extend_shared):
    q [B*n, Hq*d] bf16, already rotated, row (b, i) at b*n + i (may be a column block of a wider tensor); k_shared / v_shared [>= shared_len,
    Hkv*d] bf16; k_cache / v_cache [B, rows, Hkv*d] bf16 already holding sequence b's new rows at past[b] .. past[b]+n-1; past int32 [B] on the
    device, past[b] >= shared_len; n, shared_len and max_kv_len host bounds.  Row (b, i) attends the shared rows and then rows [shared_len,
    past[b] + i] of block b.  Rows [0, shared_len) of the own blocks are never read."""
    return _kv_attn_shared(_KV_BF16, q, (k_shared, v_shared), (k_cache, v_cache), past, n, shared_len, max_kv_len, Hq, Hkv, d, scale, out, workspace)


def attn_extend_shared_f8(q, k_shared, v_shared, k_shared_scale, v_shared_scale, k8, v8, k_scale, v_scale, past, n, shared_len, max_kv_len, Hq,
                          Hkv, d, scale, out=None, workspace=None):
    """attn_extend_shared() over e4m3 bytes: k_shared / v_shared [>= shared_len, Hkv*d] uint8 with scales [>= shared_len, Hkv] f32, k8 / v8 [B,
    rows, Hkv*d] uint8 with k_scale / v_scale [B, rows, Hkv] f32 (mm355_attn_extend_shared_f8): equal to attn_extend_shared() on dequant_kv8()
    of the same bytes bit for bit."""
    return _kv_attn_shared(_KV_F8, q, (k_shared, v_shared, k_shared_scale, v_shared_scale), (k8, v8, k_scale, v_scale), past, n, shared_len,
                           max_kv_len, Hq, Hkv, d, scale, out, workspace)


def transpose(x, out=None, ld_out=None):
    """out[c, r] = x[r, c]"""
    _chk_dev(x, out)
    px, R, C, ld = _rows2d(x)
    if out is None:
        ldo = ld_out or ((R + 7) // 8 * 8)
        buf = torch.empty((C, ldo), device=x.device, dtype=BF16)
        out = buf[:, :R]
    po, Co, Ro, ldo = _rows2d(out)
    assert Co == C and Ro == R
    _lib.check(_L().mm355_transpose_bf16(px, ld, R, C, po, ldo, _stream()), "mm355_transpose_bf16")
    return out


def colsum_f32(dy, out_f32):
    _chk_dev(dy, out_f32)
    p, M, N, ld = _rows2d(dy)
    assert out_f32.dtype == torch.float32 and out_f32.numel() >= N
    _lib.check(_L().mm355_colsum_bf16(p, ld, M, N, out_f32.data_ptr(), _stream()), "mm355_colsum_bf16")
    return out_f32


# ------------------------------------------------------------------------------------------------ norms

def rmsnorm_fwd(x, w, eps, out=None, want_rstd=False):
    """y = w * bf16(x * rstd); want_rstd: returns (y, rstd fp32 [M]) -- what `rmsnorm_apply_t` needs in the backward pass"""
    _chk_dev(x, w)
    assert x.is_contiguous() and x.dtype == BF16 and w.dtype == BF16
    h = x.shape[-1]
    M = x.numel() // h
    out = torch.empty_like(x) if out is None else out
    if not want_rstd:
        _lib.check(_L().mm355_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), out.data_ptr(), M, h, eps, _stream()), "mm355_rmsnorm_fwd")
        return out
    rstd = torch.empty((M,), device=x.device, dtype=torch.float32)
    _lib.check(_L().mm355_rmsnorm_fwd_rstd(x.data_ptr(), w.data_ptr(), out.data_ptr(), rstd.data_ptr(), M, h, eps, _stream()),
               "mm355_rmsnorm_fwd_rstd")
    return out, rstd


def rmsnorm_apply_t(x, w, rstd, Rp=None):
    """(w * bf16(x * rstd))^T as [h, Rp] (Rp >= M, padding columns zeroed): the normalised activations, contraction-major"""
    _chk_dev(x, w, rstd)
    assert x.is_contiguous() and x.dtype == BF16 and w.dtype == BF16 and rstd.dtype == torch.float32 and x.dim() == 2
    M, h = x.shape
    assert rstd.numel() == M
    Rp = (M + 7) // 8 * 8 if Rp is None else Rp
    assert Rp >= M and Rp % 8 == 0
    out = torch.empty((h, Rp), device=x.device, dtype=BF16)
    if Rp != M:
        out[:, M:].zero_()
    _lib.check(_L().mm355_rmsnorm_apply_t(x.data_ptr(), w.data_ptr(), rstd.data_ptr(), M, h, out.data_ptr(), Rp, _stream()),
               "mm355_rmsnorm_apply_t")
    return out


def rmsnorm_bwd(dy, x, w, eps, dres=None, dw_f32=None, dx=None, atomic=False):
    _chk_dev(dy, x, w)
    assert dy.is_contiguous() and x.is_contiguous()
    h = x.shape[-1]
    M = x.numel() // h
    dx = torch.empty_like(x) if dx is None else dx
    ws = None
    if dw_f32 is not None and atomic is False:               # deterministic two-stage weight-gradient sum
        ws = torch.empty(int(_L().mm355_rmsnorm_bwd_ws_floats(M, h)), dtype=torch.float32, device=x.device)
    _lib.check(_L().mm355_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), _p(dres), dx.data_ptr(), _p(dw_f32), _p(ws),
                                      M, h, eps, _stream()), "mm355_rmsnorm_bwd")
    return dx


def rmsnorm_bwd_wgrad(dy, x, w, eps, w_grad, accumulate, dres=None, dx=None):
    """dx as rmsnorm_bwd; the weight gradient goes straight into the bf16 buffer `w_grad` ((+)= when accumulate)."""
    _chk_dev(dy, x, w, w_grad)
    assert dy.is_contiguous() and x.is_contiguous() and w_grad.is_contiguous() and w_grad.dtype == BF16
    h = x.shape[-1]
    M = x.numel() // h
    dx = torch.empty_like(x) if dx is None else dx
    ws = torch.empty(int(_L().mm355_rmsnorm_bwd_ws_floats(M, h)), dtype=torch.float32, device=x.device)
    _lib.check(_L().mm355_rmsnorm_bwd_wgrad(dy.data_ptr(), x.data_ptr(), w.data_ptr(), _p(dres), dx.data_ptr(), w_grad.data_ptr(), int(bool(accumulate)),
                                            ws.data_ptr(), M, h, eps, _stream()), "mm355_rmsnorm_bwd_wgrad")
    return dx


def layernorm_fwd(x, w, b, eps, out=None):
    _chk_dev(x, w, b)
    assert x.is_contiguous()
    h = x.shape[-1]
    M = x.numel() // h
    out = torch.empty_like(x) if out is None else out
    _lib.check(_L().mm355_layernorm_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), M, h, eps, _stream()),
               "mm355_layernorm_fwd")
    return out


def layernorm_bwd(dy, x, w, eps, dw_f32, db_f32, dres=None, dx=None):
    """dx = (dres or 0) + d layernorm / dx; dw_f32 += sum dy*xhat, db_f32 += sum dy (deterministic two-stage sums)."""
    _chk_dev(dy, x, w, dw_f32, db_f32)
    assert dy.is_contiguous() and x.is_contiguous() and dw_f32.dtype == torch.float32 and db_f32.dtype == torch.float32
    h = x.shape[-1]
    M = x.numel() // h
    dx = torch.empty_like(x) if dx is None else dx
    ws = torch.empty(int(_L().mm355_layernorm_bwd_ws_floats(M, h)), dtype=torch.float32, device=x.device)
    _lib.check(_L().mm355_layernorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), _p(dres), dx.data_ptr(), dw_f32.data_ptr(), db_f32.data_ptr(),
                                        ws.data_ptr(), M, h, eps, _stream()), "mm355_layernorm_bwd")
    return dx


# ------------------------------------------------------------------------------------------------ rope / attention

def rope_table(L, d, theta, device):
    """cos / sin [L, d] bf16 of the unscaled RoPE from theta alone (mm355_rope_table): tests, tools and benchmarks.  The inverse frequencies
    come from powf on the device and may differ from HF's host-computed inv_freq by an ulp, which the position multiplies: against
    rope_table_freq on HF's inv_freq, 0.1 % of the entries differ below row 4096, 1.7 % from row 65536 on (3 % at row 131071, up to two bf16
    steps; tests/test_kv_long_context_gpu.py prints the figures).  Guaranteed: both halves of a row equal, row 0 exact.  The model builds its
    tables with rope_table_freq (metamorph_amd.rope), which is pinned to HF's arithmetic up to row 131071."""
    cos = torch.empty((L, d), device=device, dtype=BF16)
    sin = torch.empty((L, d), device=device, dtype=BF16)
    _chk_dev(cos)
    _lib.check(_L().mm355_rope_table(cos.data_ptr(), sin.data_ptr(), L, d, theta, _stream()), "mm355_rope_table")
    return cos, sin


def rope_table_freq(L, d, inv_freq, attention_scaling, device):
    """cos / sin [L, d] bf16 from host-computed inverse frequencies (float32 [d/2]: numpy array or tensor) -- metamorph_amd.rope."""
    inv = torch.as_tensor(inv_freq, dtype=torch.float32).reshape(-1).to(device)
    assert inv.numel() * 2 == d, (inv.numel(), d)
    cos = torch.empty((L, d), device=device, dtype=BF16)
    sin = torch.empty((L, d), device=device, dtype=BF16)
    _chk_dev(cos, inv)
    _lib.check(_L().mm355_rope_table_freq(cos.data_ptr(), sin.data_ptr(), L, d, inv.data_ptr(), float(attention_scaling), _stream()),
               "mm355_rope_table_freq")
    return cos, sin


def rope_qk_(qkv, B, L, Hq, Hkv, d, cos, sin, inverse=False, pos_offset=None):
    """In place on the q (first Hq*d columns) and k (next Hkv*d columns) blocks of qkv [B*L, ld]; pos_offset (int32 [B], device):
    position of row (b, l) is l + pos_offset[b] (the caller guarantees the tables are long enough)."""
    _chk_dev(qkv, cos, sin, pos_offset)
    p, M, _, ld = _rows2d(qkv)
    assert M == B * L and cos.shape[0] >= L
    if pos_offset is None:
        _lib.check(_L().mm355_rope_qk(p, ld, B, L, Hq, Hkv, d, cos.data_ptr(), sin.data_ptr(), int(inverse), _stream()), "mm355_rope_qk")
    else:
        assert pos_offset.dtype == torch.int32 and pos_offset.numel() == B
        _lib.check(_L().mm355_rope_qk_pos(p, ld, B, L, Hq, Hkv, d, cos.data_ptr(), sin.data_ptr(), pos_offset.data_ptr(), int(inverse), _stream()),
                   "mm355_rope_qk_pos")
    return qkv


def gemm_rope_supported(x, wqkv, Hq, Hkv, d, cos):
    """mm355_gemm_rope_bf16 takes this problem (head size 128, whole 256-column tiles, at least one wave of 256 x 256 tiles)."""
    M, K = x.shape
    N = wqkv.shape[0]
    return (d == 128 and N == (Hq + 2 * Hkv) * d and N % 256 == 0 and K >= 128 and K % 128 == 0 and wqkv.shape[1] == K
            and wqkv.is_contiguous() and x.is_contiguous() and cos.shape[1] == 128 and ((M + 255) // 256) * (N // 256) >= 200)


def gemm_rope(x, wqkv, B, L, Hq, Hkv, d, cos, sin, pos_offset=None):
    """qkv [B*L, (Hq + 2 Hkv) d] = fused q|k|v projection + RoPE on the q / k blocks: the bits of gemm(x, wqkv) followed by rope_qk_."""
    _chk_dev(x, wqkv, cos, sin, pos_offset)
    M, K = x.shape
    N = wqkv.shape[0]
    assert M == B * L and x.dtype == BF16 and wqkv.dtype == BF16 and cos.shape[0] >= L
    if pos_offset is not None:
        assert pos_offset.dtype == torch.int32 and pos_offset.numel() == B
    qkv = torch.empty((M, N), device=x.device, dtype=BF16)
    _lib.check(_L().mm355_gemm_rope_bf16(x.data_ptr(), K, wqkv.data_ptr(), K, qkv.data_ptr(), N, cos.data_ptr(), sin.data_ptr(), _p(pos_offset),
                                         M, N, K, L, (Hq + Hkv) * d, _stream()), f"mm355_gemm_rope_bf16 M={M} N={N} K={K}")
    return qkv


def attn_fwd(q2d, k2d, v2d, B, L, Hq, Hkv, d, scale, causal, seqlens=None, out=None, variant=0, lse=None):
    """q2d/k2d/v2d: [B*L, ld] views starting at the q / k / v column blocks (k and v share the leading dimension).
    out / lse: optional destinations ([B*L, >= Hq*d] bf16 view, contiguous [B, Hq, L] fp32).
    variant != 0 (tests / tools only) picks the kernel generation: mm355_attn_fwd_variant in include/mm355.h."""
    _chk_dev(q2d, k2d, v2d, out, lse)
    pq, M, _, ldq = _rows2d(q2d)
    pk, _, _, ldk = _rows2d(k2d)
    pv, _, _, ldv = _rows2d(v2d)
    assert ldv == ldk and M == B * L
    if out is None:
        out = torch.empty((M, Hq * d), device=q2d.device, dtype=BF16)
    if lse is None:
        lse = torch.empty((B, Hq, L), device=q2d.device, dtype=torch.float32)
    else:
        assert lse.shape == (B, Hq, L) and lse.dtype == torch.float32 and lse.is_contiguous()
    if variant:
        _lib.check(_L().mm355_attn_fwd_variant(pq, pk, pv, ldq, ldk, out.data_ptr(), out.stride(0), lse.data_ptr(), _p(seqlens),
                                               B, L, Hq, Hkv, d, scale, int(causal), int(variant), _stream()), "mm355_attn_fwd_variant")
        return out, lse
    _lib.check(_L().mm355_attn_fwd(pq, pk, pv, ldq, ldk, out.data_ptr(), out.stride(0), lse.data_ptr(), _p(seqlens),
                                   B, L, Hq, Hkv, d, scale, int(causal), _stream()), "mm355_attn_fwd")
    return out, lse


def attn_fwd_debug(q2d, k2d, v2d, B, L, Hq, Hkv, d, scale, causal, seqlens=None, variant=4):
    """attn_fwd through mm355_attn_fwd_debug (d == 128 stream, variant 4 or its serialised twin 41) -> (o, lse, rescale_counts):
    rescale_counts int32 [B, Hq, ceil(L / 256), 4] = how often each wave took the deferred-rescale branch.  Tests only."""
    _chk_dev(q2d, k2d, v2d)
    pq, M, _, ldq = _rows2d(q2d)
    pk, _, _, ldk = _rows2d(k2d)
    pv, _, _, ldv = _rows2d(v2d)
    assert ldv == ldk and M == B * L
    out = torch.empty((M, Hq * d), device=q2d.device, dtype=BF16)
    lse = torch.empty((B, Hq, L), device=q2d.device, dtype=torch.float32)
    counts = torch.zeros((B, Hq, (L + 255) // 256, 4), device=q2d.device, dtype=torch.int32)
    _lib.check(_L().mm355_attn_fwd_debug(pq, pk, pv, ldq, ldk, out.data_ptr(), out.stride(0), lse.data_ptr(), _p(seqlens),
                                         B, L, Hq, Hkv, d, scale, int(causal), int(variant), counts.data_ptr(), _stream()), "mm355_attn_fwd_debug")
    return out, lse, counts


def attn_bwd_rope_supported(d):
    """The d == 128 kernels can rotate dq / dk back through RoPE in their epilogues (mm355_attn_bwd_rope)."""
    return d == 128


def attn_bwd(q2d, k2d, v2d, o, d_o, lse, B, L, Hq, Hkv, d, scale, causal, seqlens, dq2d, dk2d, dv2d, rope=None, variant=0):
    """Writes dq / dk / dv (bf16) into the given column-block views.  rope = (cos, sin, pos_offset | None): q / k are post-RoPE and dq /
    dk are wanted as gradients of the PRE-RoPE projections -- the inverse rotation runs in the kernels' epilogues (d == 128 only).
    variant != 0 (tests / tools only) picks the kernel generation: mm355_attn_bwd_variant in include/mm355.h."""
    _chk_dev(q2d, k2d, v2d, o, d_o, dq2d, dk2d, dv2d)
    pq, M, _, ldq = _rows2d(q2d)
    pk, _, _, ldk = _rows2d(k2d)
    pv, _, _, ldv = _rows2d(v2d)
    assert ldv == ldk
    assert o.is_contiguous() and d_o.is_contiguous()
    delta = torch.empty((B, Hq, L), device=o.device, dtype=torch.float32)
    _lib.check(_L().mm355_attn_bwd_prep(o.data_ptr(), d_o.data_ptr(), o.stride(0), delta.data_ptr(), B, L, Hq, d, _stream()),
               "mm355_attn_bwd_prep")
    n_ws = int(_L().mm355_attn_bwd_ws_floats(B, L, Hq, Hkv, d, max(ldq, ldk, d_o.stride(0))))
    if variant == 2 and Hq != Hkv:                           # the generic kernels sum a GQA group from fp32 per-query-head partials
        n_ws = max(n_ws, 2 * B * L * Hq * d)
    ws = torch.empty(n_ws, device=o.device, dtype=torch.float32) if n_ws else None     # d = 128: per-row constants; generic-d GQA: partials
    pdq, _, _, lddq = _rows2d(dq2d)
    pdk, _, _, lddk = _rows2d(dk2d)
    pdv, _, _, lddv = _rows2d(dv2d)
    assert lddk == lddv
    cos = sin = pos_offset = None
    if rope is not None:
        cos, sin, pos_offset = rope
        _chk_dev(cos, sin, pos_offset)
        assert cos.shape[1] == d and cos.shape[0] >= L and (pos_offset is None or (pos_offset.dtype == torch.int32 and pos_offset.numel() == B))
    _lib.check(_L().mm355_attn_bwd_variant(pq, pk, pv, ldq, ldk, d_o.data_ptr(), d_o.stride(0), lse.data_ptr(), delta.data_ptr(), _p(seqlens),
                                           pdq, lddq, pdk, pdv, lddk, B, L, Hq, Hkv, d, scale, int(causal), _p(cos), _p(sin), _p(pos_offset),
                                           _p(ws), int(variant), _stream()), "mm355_attn_bwd_variant")


def cast_f32_to_bf16_2d(src_f32, dst2d):
    _chk_dev(src_f32, dst2d)
    pd, R, C, ldd = _rows2d(dst2d)
    assert src_f32.dim() == 2 and src_f32.shape == (R, C) and src_f32.stride(1) == 1
    _lib.check(_L().mm355_cast_f32_bf16_2d(src_f32.data_ptr(), src_f32.stride(0), pd, ldd, R, C, _stream()), "mm355_cast_f32_bf16_2d")
    return dst2d


# ------------------------------------------------------------------------------------------------ elementwise

def gemm_swiglu_supported(x, wgu, I):
    """mm355_gemm_swiglu_bf16 takes this problem (whole 128-channel tiles and K-tile pairs, a launch of at least one wave of
    256 x 256 tiles -- smaller problems go through mm355_gemm_bf16's small-tile kernels + mm355_swiglu_fwd)."""
    M, K = x.shape
    tiles = ((M + 255) // 256) * ((2 * I + 255) // 256)
    return (I % 128 == 0 and K >= 128 and K % 128 == 0 and wgu.shape[0] == 2 * I and wgu.is_contiguous() and x.is_contiguous()
            and tiles >= 200 and (2 * I * K + K) * 2 < 0x7fffffff)


def gemm_swiglu(x, wgu, I):
    """(gu [M, 2I], act [M, I]) = fused gate|up GEMM + SwiGLU: the bits of gemm(x, wgu) and swiglu_fwd(gu, I) in one launch."""
    _chk_dev(x, wgu)
    M, K = x.shape
    assert x.dtype == BF16 and wgu.dtype == BF16 and wgu.shape == (2 * I, K)
    gu = torch.empty((M, 2 * I), device=x.device, dtype=BF16)
    act = torch.empty((M, I), device=x.device, dtype=BF16)
    _lib.check(_L().mm355_gemm_swiglu_bf16(x.data_ptr(), K, wgu.data_ptr(), K, gu.data_ptr(), 2 * I, act.data_ptr(), I, M, I, K, _stream()),
               f"mm355_gemm_swiglu_bf16 M={M} I={I} K={K}")
    return gu, act


def gemm_swiglu_bwd_supported(dy, wdT, gu, I):
    """mm355_gemm_swiglu_bwd_bf16 takes this problem (and it is big enough for the 256 x 256 ping-pong tiles)."""
    M, K = dy.shape
    tiles = ((M + 255) // 256) * ((I + 255) // 256)
    return (I % 64 == 0 and M % 64 == 0 and K >= 128 and K % 128 == 0 and wdT.shape[0] == I and wdT.shape[1] == K and wdT.is_contiguous()
            and dy.is_contiguous() and gu.is_contiguous() and gu.shape == (M, 2 * I) and tiles >= 200)


def gemm_swiglu_bwd(dy, wdT, gu, I):
    """(dgu [M, 2I], actT [I, M], dguT [2I, M]) = SwiGLU backward of d act = dy . wdT^T, fused into that GEMM's epilogue: the bits of
    gemm(dy, wdT) followed by swiglu_bwd_t(gu, d act, I), without the d act round trip through HBM."""
    _chk_dev(dy, wdT, gu)
    M, K = dy.shape
    assert dy.dtype == BF16 and wdT.dtype == BF16 and gu.dtype == BF16
    dgu = torch.empty_like(gu)
    actT = torch.empty((I, M), device=gu.device, dtype=BF16)
    dguT = torch.empty((2 * I, M), device=gu.device, dtype=BF16)
    _lib.check(_L().mm355_gemm_swiglu_bwd_bf16(dy.data_ptr(), K, wdT.data_ptr(), K, gu.data_ptr(), 2 * I, dgu.data_ptr(), 2 * I,
                                               actT.data_ptr(), dguT.data_ptr(), M, M, I, K, _stream()),
               f"mm355_gemm_swiglu_bwd_bf16 M={M} I={I} K={K}")
    return dgu, actT, dguT


def swiglu_fwd(gu, I):
    _chk_dev(gu)
    assert gu.is_contiguous() and gu.shape[-1] == 2 * I
    M = gu.numel() // (2 * I)
    act = torch.empty((M, I), device=gu.device, dtype=BF16)
    _lib.check(_L().mm355_swiglu_fwd(gu.data_ptr(), act.data_ptr(), M, I, _stream()), "mm355_swiglu_fwd")
    return act


def swiglu_bwd(gu, dact, I, want_act=True):
    _chk_dev(gu, dact)
    assert gu.is_contiguous() and dact.is_contiguous()
    M = gu.numel() // (2 * I)
    dgu = torch.empty_like(gu)
    act = torch.empty((M, I), device=gu.device, dtype=BF16) if want_act else None
    _lib.check(_L().mm355_swiglu_bwd(gu.data_ptr(), dact.data_ptr(), dgu.data_ptr(), _p(act), M, I, _stream()), "mm355_swiglu_bwd")
    return dgu, act


def swiglu_bwd_t(gu, dact, I):
    """(dgu [M,2I], actT [I,M], dguT [2I,M]) -- SwiGLU backward that also writes the transposed copies for the dW GEMMs."""
    _chk_dev(gu, dact)
    assert gu.is_contiguous() and dact.is_contiguous()
    M = gu.numel() // (2 * I)
    dgu = torch.empty_like(gu)
    actT = torch.empty((I, M), device=gu.device, dtype=BF16)
    dguT = torch.empty((2 * I, M), device=gu.device, dtype=BF16)
    _lib.check(_L().mm355_swiglu_bwd_t(gu.data_ptr(), dact.data_ptr(), dgu.data_ptr(), actT.data_ptr(), dguT.data_ptr(), M, I, _stream()),
               "mm355_swiglu_bwd_t")
    return dgu, actT, dguT


def gelu_fwd(x, kind=GELU_ERF):
    _chk_dev(x)
    assert x.is_contiguous()
    y = torch.empty_like(x)
    _lib.check(_L().mm355_gelu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), kind, _stream()), "mm355_gelu_fwd")
    return y


def gelu_bwd(x, dy, kind=GELU_ERF):
    _chk_dev(x, dy)
    assert x.is_contiguous() and dy.is_contiguous()
    dx = torch.empty_like(x)
    _lib.check(_L().mm355_gelu_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), kind, _stream()), "mm355_gelu_bwd")
    return dx


def scale_(x, s_dev=None, s_host=1.0):
    _chk_dev(x)
    assert x.is_contiguous() and x.dtype == BF16
    if s_dev is not None:
        assert s_dev.dtype == torch.float32
    _lib.check(_L().mm355_scale_bf16(x.data_ptr(), x.numel(), _p(s_dev), s_host, _stream()), "mm355_scale_bf16")
    return x


def axpy_(y, x, s_dev=None, s_host=1.0, accumulate=True):
    """y (+)= s * x ; y bf16, x bf16 or f32 (contiguous, same numel)."""
    _chk_dev(y, x)
    assert y.is_contiguous() and x.is_contiguous() and y.numel() == x.numel() and y.dtype == BF16
    if x.dtype == torch.float32:
        if s_dev is None:
            _lib.check(_L().mm355_axpy_f32_to_bf16(y.data_ptr(), x.data_ptr(), y.numel(), s_host, int(accumulate), _stream()), "mm355_axpy_f32_to_bf16")
        else:
            assert s_dev.dtype == torch.float32
            _lib.check(_L().mm355_axpy_f32_to_bf16_dev(y.data_ptr(), x.data_ptr(), y.numel(), s_dev.data_ptr(), s_host, int(accumulate), _stream()),
                       "mm355_axpy_f32_to_bf16_dev")
    else:
        _lib.check(_L().mm355_axpy_bf16(y.data_ptr(), x.data_ptr(), y.numel(), _p(s_dev), s_host, int(accumulate), _stream()), "mm355_axpy_bf16")
    return y


# ------------------------------------------------------------------------------------------------ losses

def linear_ce(hidden, rows, targets, weight, need_dh=True, need_dw=True, dw_f32=None):
    """mm355_linear_ce: mean NLL of softmax(hidden[rows] . weight^T) at `targets`, plus d loss / d hidden[rows] (compact [n, h] bf16) and
    d loss / d weight ([V, h]; fp32 when more than one 8192-row chunk accumulates into it, else bf16) -> (loss f32 [1], d_hidden | None,
    dW | None).  hidden [M, h] bf16 (row-strided view allowed); rows / targets int32 [n] on the device (rows None: the first n rows)."""
    _chk_dev(hidden, rows, targets, weight)
    ph, M, h, ldh = _rows2d(hidden)
    pw, V, hw, ldw = _rows2d(weight)
    n = int(targets.numel())
    assert hw == h and hidden.dtype == BF16 and weight.dtype == BF16 and targets.dtype == torch.int32 and n > 0
    assert rows is None or (rows.dtype == torch.int32 and rows.numel() == n)
    dev = hidden.device
    if dw_f32 is None:
        dw_f32 = n > 8192
    loss = torch.empty((1,), device=dev, dtype=torch.float32)
    dh = torch.empty((n, h), device=dev, dtype=BF16) if need_dh else None
    dw = torch.empty((V, h), device=dev, dtype=torch.float32 if dw_f32 else BF16) if need_dw else None
    nbytes = int(_L().mm355_linear_ce_ws_bytes(n, V, h, int(rows is not None), int(need_dh), int(need_dw)))
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    _lib.check(_L().mm355_linear_ce(ph, ldh, _p(rows), targets.data_ptr(), n, pw, ldw, V, h, loss.data_ptr(), _p(dh), _p(dw), int(bool(dw_f32)),
                                    ws.data_ptr(), nbytes, _stream()), f"mm355_linear_ce n={n} V={V} h={h}")
    return loss, dh, dw


def _row_ws(R, device, deterministic=True):
    """R floats for the per-row loss values (summed in a fixed order -> bit-reproducible loss scalars); None = atomics (tests only)."""
    return torch.empty((R,), device=device, dtype=torch.float32) if deterministic else None


def ce_rows_(logits2d, targets_i32, V, grad_scale, loss_sum_f32, deterministic=True):
    _chk_dev(logits2d, targets_i32, loss_sum_f32)
    p, R, _, ld = _rows2d(logits2d)
    assert targets_i32.dtype == torch.int32 and targets_i32.numel() >= R
    ws = _row_ws(R, logits2d.device, deterministic)
    _lib.check(_L().mm355_ce_rows(p, ld, targets_i32.data_ptr(), R, V, grad_scale, loss_sum_f32.data_ptr(), _p(ws), _stream()), "mm355_ce_rows")


def cosine_loss(pred_raw, target, normalize, want_grad=True):
    _chk_dev(pred_raw, target)
    assert pred_raw.is_contiguous() and target.is_contiguous() and pred_raw.shape == target.shape
    R, C = pred_raw.shape
    cos_sum = torch.zeros((1,), device=pred_raw.device, dtype=torch.float32)
    dpred = torch.empty_like(pred_raw) if want_grad else None
    _lib.check(_L().mm355_cosine_loss(pred_raw.data_ptr(), target.data_ptr(), R, C, int(normalize), cos_sum.data_ptr(), _p(dpred),
                                      _p(_row_ws(R, pred_raw.device)), _stream()), "mm355_cosine_loss")
    return cos_sum, dpred


def mean_abs_loss(pred, target, want_grad=True):
    """(sum |target - pred| as a 1-element f32 tensor, d mean|t - p| / d pred or None)  -- reference `mse_loss_fn`."""
    _chk_dev(pred, target)
    assert pred.is_contiguous() and target.is_contiguous() and pred.shape == target.shape and pred.dtype == BF16 and target.dtype == BF16
    R, C = pred.shape
    abs_sum = torch.zeros((1,), device=pred.device, dtype=torch.float32)
    dpred = torch.empty_like(pred) if want_grad else None
    _lib.check(_L().mm355_mean_abs_loss(pred.data_ptr(), target.data_ptr(), R, C, abs_sum.data_ptr(), _p(dpred), _p(_row_ws(R, pred.device)),
                                        _stream()), "mm355_mean_abs_loss")
    return abs_sum, dpred


def soft_ce_loss(pred_raw, target, normalize, temperature=0.07, want_grad=True):
    """(sum_r -sum_j t log(softmax(u / temperature) + 1e-10), d (that / R) / d pred_raw or None)."""
    _chk_dev(pred_raw, target)
    assert pred_raw.is_contiguous() and target.is_contiguous() and pred_raw.shape == target.shape
    assert pred_raw.dtype == BF16 and target.dtype == BF16
    R, C = pred_raw.shape
    loss_sum = torch.zeros((1,), device=pred_raw.device, dtype=torch.float32)
    dpred = torch.empty_like(pred_raw) if want_grad else None
    _lib.check(_L().mm355_soft_ce_loss(pred_raw.data_ptr(), target.data_ptr(), R, C, int(bool(normalize)), float(temperature),
                                       loss_sum.data_ptr(), _p(dpred), _p(_row_ws(R, pred_raw.device)), _stream()), "mm355_soft_ce_loss")
    return loss_sum, dpred


def softmax_rows(x2d, temperature=0.07):
    _chk_dev(x2d)
    assert x2d.is_contiguous() and x2d.dtype == BF16 and x2d.dim() == 2
    y = torch.empty_like(x2d)
    _lib.check(_L().mm355_softmax_rows(x2d.data_ptr(), y.data_ptr(), x2d.shape[0], x2d.shape[1], float(temperature), _stream()), "mm355_softmax_rows")
    return y


def softmax_rows_bwd(y2d, dy2d, temperature=0.07):
    _chk_dev(y2d, dy2d)
    assert y2d.is_contiguous() and dy2d.is_contiguous() and y2d.shape == dy2d.shape and y2d.dtype == BF16 and dy2d.dtype == BF16
    dx = torch.empty_like(y2d)
    _lib.check(_L().mm355_softmax_rows_bwd(y2d.data_ptr(), dy2d.data_ptr(), dx.data_ptr(), y2d.shape[0], y2d.shape[1], float(temperature),
                                           _stream()), "mm355_softmax_rows_bwd")
    return dx


# ------------------------------------------------------------------------------------------------ splice / rows

def splice_gather(embed, proj2d, src_i32, h):
    _chk_dev(embed, proj2d, src_i32)
    rows = src_i32.numel()
    out = torch.empty((rows, h), device=embed.device, dtype=BF16)
    assert embed.is_contiguous() and (proj2d is None or proj2d.is_contiguous())
    _lib.check(_L().mm355_splice_gather(embed.data_ptr(), _p(proj2d), src_i32.data_ptr(), out.data_ptr(), rows, h, _stream()), "mm355_splice_gather")
    return out


def rows_gather(x2d, idx_i32, out=None):
    _chk_dev(x2d, idx_i32)
    p, _, h, ld = _rows2d(x2d)
    R = idx_i32.numel()
    if out is None:
        out = torch.empty((R, h), device=x2d.device, dtype=BF16)
    _lib.check(_L().mm355_rows_gather(p, ld, idx_i32.data_ptr(), out.data_ptr(), out.stride(0), R, h, _stream()), "mm355_rows_gather")
    return out


# ------------------------------------------------------------------------------------------------ greedy loop tail (csrc/greedy.hip)

GREEDY_MAX_EOS = 8                                           # MM355_GREEDY_MAX_EOS


def argmax_rows_ws(R, C, device):
    """the workspace of argmax_rows for [R, C] logits (mm355_argmax_rows_ws_bytes)"""
    return torch.empty(int(_L().mm355_argmax_rows_ws_bytes(R, C)), device=device, dtype=torch.uint8)


def argmax_rows(x2d, out=None, ws=None):
    """out[r] (int32) = torch.argmax(x2d[r]) of contiguous fp32 rows: lowest index among equal maxima, NaN beats every number."""
    _chk_dev(x2d, out, ws)
    assert x2d.dim() == 2 and x2d.is_contiguous() and x2d.dtype == torch.float32
    R, C = x2d.shape
    if out is None:
        out = torch.empty(R, device=x2d.device, dtype=torch.int32)
    if ws is None:
        ws = argmax_rows_ws(R, C, x2d.device)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() == R
    _lib.check(_L().mm355_argmax_rows_f32(x2d.data_ptr(), R, C, out.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), _stream()),
               f"mm355_argmax_rows_f32 R={R} C={C}")
    return out


def sample_rows_ws(R, C, device):
    """the workspace of sample_rows for [R, C] logits (mm355_sample_rows_ws_bytes)"""
    return torch.empty(int(_L().mm355_sample_rows_ws_bytes(R, C)), device=device, dtype=torch.uint8)


def sample_rows(x2d, inv_temperature, top_k, top_p, u, out=None, stats=None, ws=None):
    """out[r] (int32) = one draw from softmax(x2d[r] * inv_temperature) after top-k and top-p (HF's order; top_k 0 and top_p 1 are off)
    with the uniform u[r] in [0, 1) (mm355_sample_rows_f32; the model of it is functional.sample_row_host).  stats: optional fp32 [R, 2],
    receives (tau, Z) per row."""
    _chk_dev(x2d, u, out, stats, ws)
    assert x2d.dim() == 2 and x2d.is_contiguous() and x2d.dtype == torch.float32
    R, C = x2d.shape
    assert u.dtype == torch.float32 and u.is_contiguous() and u.numel() == R
    if out is None:
        out = torch.empty(R, device=x2d.device, dtype=torch.int32)
    if ws is None:
        ws = sample_rows_ws(R, C, x2d.device)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() == R
    assert stats is None or (stats.dtype == torch.float32 and stats.is_contiguous() and tuple(stats.shape) == (R, 2))
    _lib.check(_L().mm355_sample_rows_f32(x2d.data_ptr(), R, C, float(inv_temperature), int(top_k), float(top_p), u.data_ptr(), out.data_ptr(),
                                          _p(stats), _p(ws) if ws.numel() else 0, ws.numel() * ws.element_size(), _stream()),
               f"mm355_sample_rows_f32 R={R} C={C} inv_temperature={inv_temperature} top_k={top_k} top_p={top_p}")
    return out


def philox_uniform_rows(seed, stream_ids, counters, out=None):
    """out[r] (fp32 in [0, 1)) = the Philox4x32-10 uniform of (seed, stream_ids[r], counters[r]) (int32 device arrays;
    mm355_philox_uniform_rows, on the host functional.philox_uniform_host)"""
    _chk_dev(stream_ids, counters, out)
    R = stream_ids.numel()
    assert stream_ids.dtype == torch.int32 and counters.dtype == torch.int32 and counters.numel() == R
    assert stream_ids.is_contiguous() and counters.is_contiguous()
    if out is None:
        out = torch.empty(R, device=stream_ids.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == R
    _lib.check(_L().mm355_philox_uniform_rows(int(seed) & (2**64 - 1), stream_ids.data_ptr(), counters.data_ptr(), out.data_ptr(), R, _stream()),
               f"mm355_philox_uniform_rows R={R}")
    return out


def rows_select(mask_i32, a2d, b2d, out=None):
    """out[r] = a2d[r] if mask_i32[r] else b2d[r] (bf16 rows, int32 mask on the device)"""
    _chk_dev(mask_i32, a2d, b2d, out)
    pa, R, h, lda = _rows2d(a2d)
    pb, Rb, hb, ldb = _rows2d(b2d)
    assert (R, h) == (Rb, hb) and a2d.dtype == BF16 and b2d.dtype == BF16 and mask_i32.dtype == torch.int32 and mask_i32.numel() == R
    if out is None:
        out = torch.empty((R, h), device=a2d.device, dtype=BF16)
    po, _, _, ldo = _rows2d(out)
    _lib.check(_L().mm355_rows_select_bf16(pa, lda, pb, ldb, mask_i32.data_ptr(), po, ldo, R, h, _stream()), "mm355_rows_select_bf16")
    return out


def greedy_advance(tok, C, state, live, embed, fed, pred_z, x_in, tok_log, z_log, start_id, end_id, num_image_tokens, max_new_tokens,
                   eos_ids):
    """One transition of the greedy loop for every sequence on the device (mm355_greedy_advance; the model of it on plain ints is
    functional.greedy_advance_host).  tok [B] int32: this step's argmax over C logits; state: int32 [6, B] rows in_image, n_img, total_out,
    done, n_tokens, n_z; live: int32 [1]; embed [rows >= C, h]; fed [B, h] / pred_z [B, Dz]: the lm_head input rows and the image head's
    rows; writes x_in [B, h], tok_log [B, token_cap] int32 and z_log [B, z_cap, Dz] bf16."""
    _chk_dev(tok, state, live, embed, fed, pred_z, x_in, tok_log, z_log)
    B = tok.numel()
    assert tok.dtype == torch.int32 and state.dtype == torch.int32 and tuple(state.shape) == (6, B) and state.is_contiguous()
    assert live.dtype == torch.int32 and tok_log.dtype == torch.int32 and tok_log.is_contiguous() and z_log.is_contiguous() and z_log.dtype == BF16
    pe, rows, h, lde = _rows2d(embed)
    pf, _, _, ldf = _rows2d(fed)
    pz, _, Dz, ldz = _rows2d(pred_z)
    px, _, _, ldx = _rows2d(x_in)
    assert fed.shape == x_in.shape == (B, h) and pred_z.shape[0] == B and tok_log.shape[0] == B and z_log.shape[0] == B and z_log.shape[2] == Dz
    eos = [int(e) for e in eos_ids]
    arr = (_lib.ctypes.c_int32 * max(len(eos), 1))(*eos)
    s = [state[i].data_ptr() for i in range(6)]
    _lib.check(_L().mm355_greedy_advance(tok.data_ptr(), B, int(C), *s, live.data_ptr(), pe, lde, rows, pf, ldf, pz, ldz, px, ldx, h, Dz,
                                         tok_log.data_ptr(), tok_log.shape[1], z_log.data_ptr(), z_log.shape[1], int(start_id), int(end_id),
                                         int(num_image_tokens), int(max_new_tokens), _lib.ctypes.addressof(arr), len(eos), _stream()),
               f"mm355_greedy_advance B={B} C={C} eos={len(eos)}")


# ------------------------------------------------------------------------------------------------ prompt-lookup speculation (csrc/spec.hip)

SPEC_MAX_DRAFT = 15                                          # MM355_SPEC_MAX_DRAFT
SPEC_MAX_NGRAM = 8                                           # MM355_SPEC_MAX_NGRAM


def _i32(*ts):
    assert all(t.dtype == torch.int32 and t.is_contiguous() for t in ts), [(t.dtype, t.shape) for t in ts]


def ngram_draft_rows(hist, hist_len, state, pos, K, N, C, embed, drafts, n_draft, x_in, pos_rows, mask_rows):
    """The drafts of every sequence and the next step's input rows (mm355_ngram_draft_rows; the model of it is
    functional.prompt_lookup_host).  hist [B, hist_cap] / hist_len [B] int32: the ids the drafts are looked up in; state: the greedy loop's
    int32 [6, B] (done and in_image are read); pos [B]: the cache's write positions.  Writes drafts [B, K], n_draft [B], rows b * (K + 1) + 1
    .. of x_in [B * (K + 1), h] (embed rows of the drafts, zero rows behind them), pos_rows and mask_rows [B * (K + 1)]."""
    _chk_dev(hist, hist_len, state, pos, embed, drafts, n_draft, x_in, pos_rows, mask_rows)
    B, n = hist.shape[0], int(K) + 1
    _i32(hist, hist_len, state, pos, drafts, n_draft, pos_rows, mask_rows)
    assert hist.dim() == 2 and tuple(state.shape) == (6, B) and hist_len.numel() == B and pos.numel() == B and n_draft.numel() == B
    assert tuple(drafts.shape) == (B, K) and pos_rows.numel() == B * n and mask_rows.numel() == B * n
    pe, rows, h, lde = _rows2d(embed)
    px, Rx, hx, ldx = _rows2d(x_in)
    assert (Rx, hx) == (B * n, h) and embed.dtype == BF16 and x_in.dtype == BF16
    _lib.check(_L().mm355_ngram_draft_rows(hist.data_ptr(), hist.shape[1], hist_len.data_ptr(), state[3].data_ptr(), state[0].data_ptr(),
                                           pos.data_ptr(), B, int(K), int(N), int(C), pe, lde, rows, drafts.data_ptr(), n_draft.data_ptr(), px, ldx,
                                           h, pos_rows.data_ptr(), mask_rows.data_ptr(), _stream()),
               f"mm355_ngram_draft_rows B={B} K={K} N={N} C={C}")


def spec_verify_advance(tok, drafts, n_draft, C, state, live, embed, fed, pred_z, x_in, tok_log, z_log, hist, hist_len, pos, length, acc_log,
                        n_steps, start_id, end_id, num_image_tokens, max_new_tokens, eos_ids, count_step=True):
    """greedy_advance over the n = K + 1 rows of every sequence for as long as its drafts hold (mm355_spec_verify_advance; the model of it is
    functional.spec_advance_host).  tok [B * n]: the argmax of every row; drafts [B, K] / n_draft [B] as ngram_draft_rows wrote them; fed
    [B * n, h] / pred_z [B * n, Dz]; state, live, embed, tok_log, z_log as greedy_advance takes them; hist / hist_len receive the logged ids;
    pos / length: the cache's pos_dev / len_dev, advanced by the iterations run; acc_log [B, cap] / n_steps [B] log that count per step.
    count_step=False: the first iteration on the prompt's last row -- pos, length, acc_log and n_steps are left alone.  Writes row b * n of
    x_in [B * n, h]."""
    _chk_dev(tok, drafts, n_draft, state, live, embed, fed, pred_z, x_in, tok_log, z_log, hist, hist_len, pos, length, acc_log, n_steps)
    B, K = drafts.shape
    n = K + 1
    _i32(tok, drafts, n_draft, state, live, tok_log, hist, hist_len, pos, length, acc_log, n_steps)
    assert tok.numel() == B * n and tuple(state.shape) == (6, B) and z_log.is_contiguous() and z_log.dtype == BF16
    pe, rows, h, lde = _rows2d(embed)
    pf, _, _, ldf = _rows2d(fed)
    pz, _, Dz, ldz = _rows2d(pred_z)
    px, _, _, ldx = _rows2d(x_in)
    assert fed.shape == x_in.shape == (B * n, h) and pred_z.shape[0] == B * n and tok_log.shape[0] == B and z_log.shape[0] == B
    assert z_log.shape[2] == Dz and hist.shape[0] == B and acc_log.shape[0] == B and n_draft.numel() == hist_len.numel() == B
    assert pos.numel() == length.numel() == n_steps.numel() == B
    eos = [int(e) for e in eos_ids]
    arr = (_lib.ctypes.c_int32 * max(len(eos), 1))(*eos)
    s = [state[i].data_ptr() for i in range(6)]
    _lib.check(_L().mm355_spec_verify_advance(tok.data_ptr(), drafts.data_ptr(), n_draft.data_ptr(), B, K, int(C), *s, live.data_ptr(), pe, lde,
                                              rows, pf, ldf, pz, ldz, px, ldx, h, Dz, tok_log.data_ptr(), tok_log.shape[1], z_log.data_ptr(),
                                              z_log.shape[1], hist.data_ptr(), hist.shape[1], hist_len.data_ptr(), pos.data_ptr(),
                                              length.data_ptr(), acc_log.data_ptr(), acc_log.shape[1], n_steps.data_ptr(), int(bool(count_step)),
                                              int(start_id), int(end_id), int(num_image_tokens), int(max_new_tokens),
                                              _lib.ctypes.addressof(arr), len(eos), _stream()),
               f"mm355_spec_verify_advance B={B} K={K} C={C} eos={len(eos)}")


# ------------------------------------------------------------------------------------------------ beam search in the device loop (csrc/beam.hip)

BEAM_MAX = 8                                                 # MM355_BEAM_MAX


def beam_select_rows_ws(K, V, M, device):
    """the workspace of beam_select_rows (mm355_beam_select_rows_ws_bytes)"""
    return torch.empty(int(_L().mm355_beam_select_rows_ws_bytes(K, V, M)), device=device, dtype=torch.uint8)


def beam_select_rows(x2d, running, M, stats=None, cand_val=None, cand_idx=None, ws=None):
    """Step 1 of a beam step on the contiguous fp32 logits x2d [K, V] and the beams' scores running [K] (mm355_beam_select_rows_f32; the
    model of it is functional.beam_select_host on beam_logprob_rows_host of the statistics): -> (stats [K, 2] = (row maximum, ln sum
    exp(x - maximum)), cand_val [M] fp32, cand_idx [M] int32): the M best of ((x - m) - lse) + running over all K * V entries, sorted by
    value descending, then flat index ascending."""
    _chk_dev(x2d, running, stats, cand_val, cand_idx, ws)
    assert x2d.dim() == 2 and x2d.is_contiguous() and x2d.dtype == torch.float32
    K, V = x2d.shape
    M = int(M)
    dev = x2d.device
    assert running.dtype == torch.float32 and running.is_contiguous() and running.numel() == K
    stats = torch.empty((K, 2), device=dev, dtype=torch.float32) if stats is None else stats
    cand_val = torch.empty(M, device=dev, dtype=torch.float32) if cand_val is None else cand_val
    cand_idx = torch.empty(M, device=dev, dtype=torch.int32) if cand_idx is None else cand_idx
    ws = beam_select_rows_ws(K, V, M, dev) if ws is None else ws
    assert stats.dtype == torch.float32 and stats.is_contiguous() and tuple(stats.shape) == (K, 2)
    assert cand_val.dtype == torch.float32 and cand_val.is_contiguous() and cand_val.numel() == M
    assert cand_idx.dtype == torch.int32 and cand_idx.is_contiguous() and cand_idx.numel() == M
    _lib.check(_L().mm355_beam_select_rows_f32(x2d.data_ptr(), K, V, running.data_ptr(), M, stats.data_ptr(), cand_val.data_ptr(),
                                               cand_idx.data_ptr(), _p(ws) if ws.numel() else 0, ws.numel() * ws.element_size(), _stream()),
               f"mm355_beam_select_rows_f32 K={K} V={V} M={M}")
    return stats, cand_val, cand_idx


def beam_advance(cand_val, cand_idx, V, state, len_pow, max_new_tokens, length_penalty, early_stopping, eos_ids, embed=None, x_in=None):
    """Steps 2 - 6 of a beam step for the M sorted candidates on device-resident state (mm355_beam_advance; the model of it, bit for bit,
    is functional.beam_step_host).  state: a dict of device tensors in functional.beam_state_host's layout (running, fin_score fp32 [K];
    fin_flag [K], fin_end [K, 3], scal [2], live [1], tok, parent [K], tok_log, parent_log [cap, K] int32; own_block uint8 [K, columns] or
    None); len_pow fp32 [max_new_tokens] on the device (functional.beam_len_pow); early_stopping 0 / 1 / 2 (False / True / "never");
    embed [rows >= V, h] and x_in [K, h]: the next input rows, or both None."""
    s = state
    tbl = s.get("own_block")
    _chk_dev(cand_val, cand_idx, len_pow, embed, x_in, *[t for t in s.values() if t is not None])
    K, M = s["running"].numel(), cand_val.numel()
    assert cand_val.dtype == torch.float32 and cand_idx.dtype == torch.int32 and cand_idx.numel() == M
    assert cand_val.is_contiguous() and cand_idx.is_contiguous()
    for n, dt, shape in (("running", torch.float32, (K,)), ("fin_score", torch.float32, (K,)), ("fin_flag", torch.int32, (K,)),
                         ("fin_end", torch.int32, (K, 3)), ("scal", torch.int32, (2,)), ("live", torch.int32, (1,)),
                         ("tok", torch.int32, (K,)), ("parent", torch.int32, (K,))):
        assert s[n].dtype == dt and tuple(s[n].shape) == shape and s[n].is_contiguous(), n
    cap = s["tok_log"].shape[0]
    for n in ("tok_log", "parent_log"):
        assert s[n].dtype == torch.int32 and tuple(s[n].shape) == (cap, K) and s[n].is_contiguous(), n
    assert len_pow.dtype == torch.float32 and len_pow.is_contiguous() and len_pow.numel() >= int(max_new_tokens)
    pt, ldt = (0, 0)
    if tbl is not None:
        assert tbl.dtype == torch.uint8 and tbl.dim() == 2 and tbl.stride(1) == 1 and tbl.shape[0] == K
        pt, ldt = tbl.data_ptr(), tbl.stride(0)
        assert tbl.shape[1] >= int(max_new_tokens)
    pe = lde = rows = px = ldx = h = 0
    if x_in is not None:
        pe, rows, h, lde = _rows2d(embed)
        px, Kx, hx, ldx = _rows2d(x_in)
        assert (Kx, hx) == (K, h) and embed.dtype == BF16 and x_in.dtype == BF16
    eos = [int(e) for e in eos_ids]
    arr = (_lib.ctypes.c_int32 * max(len(eos), 1))(*eos)
    _lib.check(_L().mm355_beam_advance(cand_val.data_ptr(), cand_idx.data_ptr(), K, M, int(V), s["running"].data_ptr(), s["fin_score"].data_ptr(),
                                       s["fin_flag"].data_ptr(), s["fin_end"].data_ptr(), s["scal"].data_ptr(), s["live"].data_ptr(),
                                       s["tok"].data_ptr(), s["parent"].data_ptr(), s["tok_log"].data_ptr(), s["parent_log"].data_ptr(), cap,
                                       pt, ldt, pe, lde, rows, px, ldx, h, len_pow.data_ptr(), int(max_new_tokens), float(length_penalty),
                                       int(early_stopping), _lib.ctypes.addressof(arr), len(eos), _stream()),
               f"mm355_beam_advance K={K} M={M} V={V} eos={len(eos)}")


# ------------------------------------------------------------------------------------------------ logits processors, log-probabilities (csrc/logits.hip)

def seen_words(C):
    """32-bit words per row of the bitmap of seen ids over C logits: bit (i & 31) of word (i >> 5) is id i"""
    return (int(C) + 31) // 32


def _chk_seen(seen, R, C):
    """a bitmap of R rows: 32-bit words (torch.int32 or torch.uint32 storage of the same bits), contiguous -> words per row"""
    assert seen.dtype in (torch.int32, torch.uint32) and seen.dim() == 2 and seen.is_contiguous() and seen.shape[0] == R
    assert seen.shape[1] >= seen_words(C), f"{seen.shape[1]} bitmap words per row for {C} logits"
    return seen.shape[1]


def logits_process_rows(x2d, penalty=1.0, seen=None, total_out=None, min_new_tokens=0, eos_ids=(), suppress_ids=None):
    """Edits the contiguous fp32 logits x2d [R, C] in place (mm355_logits_process_rows_f32; the model of it, bit for bit, is
    functional.logits_process_host), per row in HF's order: ids marked in seen [R, >= seen_words(C)] times / over `penalty` (1: off), the
    eos ids -inf while total_out[r] (int32 [R]) < min_new_tokens (0: off), the ids of suppress_ids (int32 device tensor) -inf."""
    _chk_dev(x2d, seen, total_out, suppress_ids)
    assert x2d.dim() == 2 and x2d.is_contiguous() and x2d.dtype == torch.float32
    R, C = x2d.shape
    words = _chk_seen(seen, R, C) if seen is not None else 0
    assert total_out is None or (total_out.dtype == torch.int32 and total_out.is_contiguous() and total_out.numel() == R)
    assert suppress_ids is None or (suppress_ids.dtype == torch.int32 and suppress_ids.is_contiguous() and suppress_ids.dim() == 1)
    eos = [int(e) for e in eos_ids]
    arr = (_lib.ctypes.c_int32 * max(len(eos), 1))(*eos)
    n_sup = 0 if suppress_ids is None else suppress_ids.numel()
    _lib.check(_L().mm355_logits_process_rows_f32(x2d.data_ptr(), R, C, float(penalty), _p(seen), words, _p(total_out), int(min_new_tokens),
                                                  _lib.ctypes.addressof(arr), len(eos), _p(suppress_ids) if n_sup else 0, n_sup, _stream()),
               f"mm355_logits_process_rows_f32 R={R} C={C} penalty={penalty} min_new_tokens={min_new_tokens} eos={len(eos)} suppress={n_sup}")
    return x2d


def token_note_rows(x2d, tok, state, num_image_tokens, token_cap=None, seen=None, logp_log=None):
    """After the pick and before greedy_advance (mm355_token_note_rows_f32; functional.token_note_host): for every row that is about to log
    tok[r] -- state: the int32 [6, R] rows of greedy_advance -- sets the id's bit in seen [R, >= seen_words(C)] and writes its
    log-probability under the fp32 logits x2d [R, C] as they stand to logp_log[r, n_tokens[r]] (fp32 [R, token_cap])."""
    _chk_dev(x2d, tok, state, seen, logp_log)
    assert x2d.dim() == 2 and x2d.is_contiguous() and x2d.dtype == torch.float32
    R, C = x2d.shape
    assert tok.dtype == torch.int32 and tok.is_contiguous() and tok.numel() == R
    assert state.dtype == torch.int32 and tuple(state.shape) == (6, R) and state.is_contiguous()
    words = _chk_seen(seen, R, C) if seen is not None else 0
    if logp_log is not None:
        assert logp_log.dtype == torch.float32 and logp_log.is_contiguous() and logp_log.dim() == 2 and logp_log.shape[0] == R
        assert token_cap is None or int(token_cap) == logp_log.shape[1]
        token_cap = logp_log.shape[1]
    assert token_cap is not None, "token_cap: the rows of the token log (taken from logp_log where that is given)"
    in_image, n_img, _, done, n_tokens, _ = (state[i].data_ptr() for i in range(6))
    _lib.check(_L().mm355_token_note_rows_f32(x2d.data_ptr(), R, C, tok.data_ptr(), in_image, n_img, done, n_tokens, int(num_image_tokens),
                                              int(token_cap), _p(seen), words, _p(logp_log), _stream()),
               f"mm355_token_note_rows_f32 R={R} C={C} token_cap={token_cap}")


def rows_scatter_add_(dst2d, src2d, idx_i32):
    _chk_dev(dst2d, src2d, idx_i32)
    ps, R, h, lds = _rows2d(src2d)
    pd, _, _, ldd = _rows2d(dst2d)
    _lib.check(_L().mm355_rows_scatter_add(ps, lds, idx_i32.data_ptr(), pd, ldd, R, h, _stream()), "mm355_rows_scatter_add")
    return dst2d


def embed_grad_(dembed, dout2d, tok_i32, seg_i32, pos_i32, accumulate):
    _chk_dev(dembed, dout2d)
    assert dout2d.is_contiguous() and dembed.is_contiguous()
    n_seg = tok_i32.numel()
    if n_seg == 0:
        return dembed
    _lib.check(_L().mm355_embed_grad(dout2d.data_ptr(), tok_i32.data_ptr(), seg_i32.data_ptr(), pos_i32.data_ptr(), n_seg,
                                     dembed.data_ptr(), dembed.shape[1], int(accumulate), _stream()), "mm355_embed_grad")
    return dembed


# ------------------------------------------------------------------------------------------------ vision

def im2col_patch(images, p, Kp):
    _chk_dev(images)
    assert images.is_contiguous() and images.dim() == 4 and images.shape[1] == 3
    N, _, H, W = images.shape
    is_f32 = images.dtype == torch.float32
    assert is_f32 or images.dtype == BF16
    out = torch.empty((N * (H // p) * (W // p), Kp), device=images.device, dtype=BF16)
    _lib.check(_L().mm355_im2col_patch(images.data_ptr(), int(is_f32), N, H, W, p, out.data_ptr(), Kp, _stream()), "mm355_im2col_patch")
    return out


def bilinear_l2norm(feat, side_in, side_out, normalize):
    _chk_dev(feat)
    assert feat.is_contiguous()
    N, P, C = feat.shape
    assert P == side_in * side_in
    out = torch.empty((N, side_out * side_out, C), device=feat.device, dtype=BF16)
    _lib.check(_L().mm355_bilinear_l2norm(feat.data_ptr(), out.data_ptr(), N, side_in, side_out, C, int(normalize), _stream()), "mm355_bilinear_l2norm")
    return out


def bilinear_l2norm_bwd(x, dy, side_in, side_out, normalize):
    """Gradient of bilinear_l2norm w.r.t. x [N, side_in^2, C] (bf16) from dy [N, side_out^2, C]; returns bf16."""
    _chk_dev(x, dy)
    assert x.is_contiguous() and dy.is_contiguous()
    N, _, C = x.shape
    acc = torch.zeros(x.shape, device=x.device, dtype=torch.float32)
    _lib.check(_L().mm355_bilinear_l2norm_bwd(x.data_ptr(), dy.data_ptr(), acc.data_ptr(), N, side_in, side_out, C, int(bool(normalize)),
                                              _stream()), "mm355_bilinear_l2norm_bwd")
    out = torch.empty_like(x)
    cast_f32_to_bf16_2d(acc.view(-1, C), out.view(-1, C))
    return out


# ------------------------------------------------------------------------------------------------ optimizer

def adamw_shard_(p32, m, v, g, p_out, lr, beta1, beta2, eps, wd, step, grad_scale_dev=None):
    _chk_dev(p32, m, v, g, p_out)
    n = p32.numel()
    assert m.numel() == n and v.numel() == n and g.numel() == n and p_out.numel() == n
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    _lib.check(_L().mm355_adamw_shard(p32.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), p_out.data_ptr(), n, lr, beta1, beta2,
                                      eps, wd, bc1, bc2, _p(grad_scale_dev), _stream()), "mm355_adamw_shard")


SUMSQ_PARTIALS = 2048            # MM355_SUMSQ_PARTIALS (include/mm355.h)
_sumsq_partials = {}


def sumsq_(x, out_f32, partials=None):
    """out_f32[0] += sum(x^2), deterministic (two launches, no atomics).  `partials`: fp32 scratch of SUMSQ_PARTIALS elements; by
    default one buffer per (device, stream), so launches on different streams never share it."""
    _chk_dev(x, out_f32)
    assert x.is_contiguous()
    if partials is None:
        key = (x.device, _stream())
        partials = _sumsq_partials.get(key)
        if partials is None:
            partials = _sumsq_partials[key] = torch.empty(SUMSQ_PARTIALS, dtype=torch.float32, device=x.device)
    assert partials.dtype == torch.float32 and partials.numel() >= SUMSQ_PARTIALS and partials.device == x.device
    _lib.check(_L().mm355_sumsq_bf16(x.data_ptr(), x.numel(), out_f32.data_ptr(), partials.data_ptr(), _stream()), "mm355_sumsq_bf16")
    return out_f32


def clip_coef(sumsq_f32, max_norm, pre_scale, out_f32):
    _chk_dev(sumsq_f32, out_f32)
    _lib.check(_L().mm355_clip_coef(sumsq_f32.data_ptr(), max_norm, pre_scale, out_f32.data_ptr(), _stream()), "mm355_clip_coef")
    return out_f32
