"""Test infrastructure for the fused GEMM store (gemm_epilogue -> epi_store8 / epi_scalar, metamorph_amd/csrc/gemm_common.h): the fp64
oracle of the epilogue chain, its derived per-element bound, a checker that says WHICH store body a bad column went through, and the
output / residual geometries that steer a launch onto the vector body, the ragged tail or the all-scalar path.  Written in torch, so it
runs on whichever device its inputs live on; tests/test_gemm_epilogue_host.py proves on the CPU that the bound separates a right
epilogue from eight wrong ones, tests/test_gemm_epilogue_gpu.py applies it to the kernels.  Nothing here is derived from a kernel's output.

The store has two bodies.  The VECTOR body takes eight columns with 16-byte accesses when  c + 8 <= N,  ldc % 8 == 0  and (with a
residual)  ldr % 8 == 0;  everything else goes one element at a time through the SCALAR body: the last chunk of a row when N % 8 != 0,
and every chunk of every row when ldc or ldr is no multiple of 8.
"""
from collections import namedtuple

import torch

from helper_refs import F64, GELU_ERF, GELU_TANH, gelu64

# ------------------------------------------------------------------------------------------------ the cases (the issue's table)

M_FULL, N_FULL, N_EVEN = 531, 523, 520       # two 256-row tiles + 19 rows = 3 * 177;  N % 8 = 3;  the same problem cut at a chunk edge
RES_MOD = 177                                # no multiple of the 16-row fragment group: the residual row wraps inside a group

# out: allocation [M + extra_rows, out_cols], the launch writes [0:M, col0:col0 + N];  residual: allocation [rows, res_cols], first N columns
Geometry = namedtuple("Geometry", "name M N out_cols col0 extra_rows res_cols")
GEOMETRIES = [
    Geometry("G1", M_FULL, N_EVEN, 520, 0, 0, 520),       # vector body everywhere (the baseline of the bit comparisons)
    Geometry("G2", M_FULL, N_FULL, 528, 0, 0, 528),       # vector chunks + one 3-column scalar tail per row
    Geometry("G3", M_FULL, N_FULL, 523, 0, 0, 523),       # ldc % 8 != 0: scalar everywhere (the lm_head case)
    Geometry("G4", M_FULL, N_EVEN, 520, 0, 0, 523),       # scalar because of ldr alone (only with a residual)
    Geometry("G5", 19, 5, 8, 0, 0, 8),                    # fewer columns than one chunk, fewer rows than one tile
    Geometry("G6", M_FULL, N_FULL, 1024, 64, 3, 528),     # a column view of a wider buffer (the SigLIP q/k/v launches)
]
GEO = {g.name: g for g in GEOMETRIES}

Flags = namedtuple("Flags", "name bias gelu res mod acc")
FLAG_SETS = [
    Flags("none", False, None, False, False, False),
    Flags("bias", True, None, False, False, False),
    Flags("bias_erf", True, "erf", False, False, False),
    Flags("bias_tanh", True, "tanh", False, False, False),
    Flags("res", False, None, True, False, False),
    Flags("res_mod", False, None, True, True, False),
    Flags("bias_erf_res", True, "erf", True, False, False),
    Flags("bias_res_mod", True, None, True, True, False),          # the patch-embedding combination
    Flags("acc", False, None, False, False, True),
    Flags("bias_tanh_res_acc", True, "tanh", True, False, True),
]
FLAGS = {f.name: f for f in FLAG_SETS}

VECTOR, TAIL, SCALAR = 0, 1, 2
CLASS_NAMES = ("vector chunk", "tail chunk", "all-scalar")


def column_classes(geo, with_residual):
    """per output column: VECTOR (16-byte body), TAIL (the row's last, partial chunk: scalar body) or SCALAR (ldc or ldr no multiple of 8:
    the scalar body takes every chunk) -- by construction, from N % 8, ldc % 8 and ldr % 8"""
    if geo.out_cols % 8 or (with_residual and geo.res_cols % 8):
        return torch.full((geo.N,), SCALAR, dtype=torch.int64)
    c = torch.arange(geo.N)
    return torch.where(c < geo.N - geo.N % 8, VECTOR, TAIL)


def tail_columns(geo):
    """columns of the row's last, partial chunk (empty when N % 8 == 0), whichever body stores them"""
    return torch.arange(geo.N - geo.N % 8, geo.N)


def problem(K, seed=0):
    """The one problem every geometry is a window of (CPU tensors): a [531, K], b [523, K], bias [523], a full and a 177-row residual,
    the old C in bf16 and in fp32.  |a . b| ~ 0.09 sqrt(K): O(1), where both GELU forms bend."""
    g = torch.Generator().manual_seed(1000 + 7 * K + seed)

    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale
    return dict(K=K, a=rnd(M_FULL, K, scale=0.3).bfloat16(), b=rnd(N_FULL, K, scale=0.3).bfloat16(), bias=rnd(N_FULL, scale=0.5).bfloat16(),
                res=rnd(M_FULL, N_FULL).bfloat16(), res_mod=rnd(RES_MOD, N_FULL).bfloat16(), c0_bf16=rnd(M_FULL, N_FULL).bfloat16(),
                c0_f32=rnd(M_FULL, N_FULL))


# ------------------------------------------------------------------------------------------------ the oracle and its bound

def epilogue_ref64(a, b, bias=None, res=None, res_row_mod=0, gelu=None, c0=None):
    """fp64 on the bf16 inputs, in the kernel's order: a . b^T, + bias, GELU (erf or tanh form, the constants of mm355_common.h), + res[row %
    res_row_mod] (res[row] without a modulus), + c0 when accumulating"""
    x = a.to(F64) @ b.to(F64).t()
    if bias is not None:
        x = x + bias.to(F64)[None, :x.shape[1]]
    if gelu is not None:
        x = gelu64(x, {"erf": GELU_ERF, "tanh": GELU_TANH}[gelu])
    if res is not None:
        rows = torch.arange(x.shape[0], device=x.device)
        if res_row_mod:
            rows = rows % res_row_mod
        x = x + res.to(F64)[rows, :x.shape[1]]
    if c0 is not None:
        x = x + c0.to(F64)
    return x


def accumulation_bound(a, b):
    """4 K 2^-24 (|a| . |b|^T): the fp32 accumulation of exact bf16 products (test_gemm_fp32_output_tight's bound, per element)"""
    return 4.0 * a.shape[1] * 2.0 ** -24 * (a.to(F64).abs() @ b.to(F64).abs().t())


def epilogue_bound(ref64, accb, gelu, out_f32):
    """fp32 output: L accb + 2^-18 (|ref| + 1), L = 1.13 (just above max |GELU'|) behind a GELU, else 1; 2^-18 covers the few fp32 roundings
    of the epilogue and erff / tanhf to 16 ulp (2^-19 on the factor).  bf16 output: + 2^-8 |ref| for the one final rounding."""
    bound = (1.13 if gelu is not None else 1.0) * accb + 2.0 ** -18 * (ref64.abs() + 1.0)
    return bound if out_f32 else bound + 2.0 ** -8 * ref64.abs()


def check(got, ref64, bound, what, classes=None):
    """Every element of `got` within `bound` of `ref64` (a NaN is beyond any bound); else an AssertionError with the count, the worst element,
    its (row, col) and, given the columns' classes, which store body wrote that column and how the bad elements spread over the classes.
    Returns the largest |error| / bound."""
    assert got.shape == ref64.shape == bound.shape, (what, tuple(got.shape), tuple(ref64.shape), tuple(bound.shape))
    err = (got.to(F64) - ref64).abs()
    ratio = err / bound
    bad = ~(err <= bound)
    if bool(bad.any()):
        score = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        r, c = divmod(int(score.argmax()), got.shape[1])
        where = ""
        if classes is not None:
            cls = classes.to(bad.device)
            per = ", ".join(f"{int(bad[:, cls == k].sum())} in {CLASS_NAMES[k]} columns" for k in range(3) if bool((cls == k).any()))
            where = f" [{CLASS_NAMES[int(cls[c])]} column; {per}]"
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound; worst at ({r}, {c}){where}: got "
                             f"{float(got[r, c]):.9g}, fp64 {float(ref64[r, c]):.9g}, |err| {float(err[r, c]):.3e}, bound {float(bound[r, c]):.3e}")
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------ output buffers with a canary

CANARY = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA5A5A5)}      # quiet NaNs no arithmetic here produces


def canary_out(geo, dtype, device):
    """(allocation, the view a launch writes): every element of the allocation, the view's inside too, holds the canary NaN"""
    ity, pat = CANARY[dtype]
    alloc = torch.full((geo.M + geo.extra_rows, geo.out_cols), pat, dtype=ity, device=device).view(dtype)
    return alloc, alloc[:geo.M, geo.col0:geo.col0 + geo.N]


def check_untouched(alloc, geo, what):
    """the allocation, compared as integers: every element outside [0:M, col0:col0 + N] still holds the canary"""
    ity, pat = CANARY[alloc.dtype]
    outside = torch.ones(alloc.shape, dtype=torch.bool, device=alloc.device)
    outside[:geo.M, geo.col0:geo.col0 + geo.N] = False
    hit = outside & (alloc.view(ity) != pat)
    if bool(hit.any()):
        r, c = divmod(int(hit.view(-1).int().argmax()), alloc.shape[1])
        raise AssertionError(f"{what}: {int(hit.sum())} elements outside the [{geo.M}, {geo.N}] window at column {geo.col0} were written; "
                             f"first at ({r}, {c}) of the [{alloc.shape[0]}, {alloc.shape[1]}] allocation")


RES_PAD = 1.0e4       # what the residual's padding columns hold: finite, and 10^4 bounds away if a launch reads one


def residual_view(res, geo):
    """the first N columns of `res` as a view with the geometry's leading dimension; the padding columns hold RES_PAD"""
    buf = torch.full((res.shape[0], geo.res_cols), RES_PAD, dtype=res.dtype, device=res.device)
    buf[:, :geo.N] = res[:, :geo.N]
    return buf[:, :geo.N]
