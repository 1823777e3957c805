"""The fused GEMM store (gemm_epilogue -> epi_store8 / epi_scalar, csrc/gemm_common.h) on its ragged-edge and unaligned paths: every
epilogue flag set, bf16 and fp32 output, on six output / residual geometries that reach the 16-byte vector body, the scalar tail of a row
and the all-scalar path (tests/gemm_epilogue_refs.py has the table), through variants 1, 2, 7, 9, 11 and the dispatcher.
Needs an MI355X:  pytest -m gpu

Per launch: (1) every element within the DERIVED bound of the fp64 oracle (gemm_epilogue_refs.epilogue_bound; test_gemm_epilogue_host.py
shows that the bound rejects eight wrong stores), (4) nothing outside the [M, N] window written and, unless the launch accumulates,
everything inside it written -- the whole allocation is prefilled with a canary NaN and compared as integers.  Per flag set and output type:
(2) the two store bodies agree -- columns [0, 520) of G2, G3, G4 and G6 are the bits G1 writes, (3) the variants agree -- 2, 7, 9, 11 and the
dispatcher write the bits of variant 1 on every geometry.  Variant 7 (the pipelined 256 x 256 kernel, also what 11 runs at K = 192) is held
to the same equality: it adds the 32-wide MFMA steps of an output element in the same K order as the others.
Both equalities hold exactly, the tanh-GELU cases included: no allowance is made anywhere.  (5) Misaligned bases, both GELU flags and a
pair launch with a fused flag are refused with MM355_EINVAL, the LDS-DMA variants at K = 72 with MM355_EUNSUPPORTED.
Besides: ops.gemm's n= argument, windows / bias / residual at exactly 16-byte alignment, and the pair launch accumulating into ragged
bf16 and fp32 windows against variant 11 launched per problem."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_epilogue_refs as E  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
VARIANTS = (1, 2, 7, 9, 11, 0)


@pytest.fixture(scope="module")
def ops():
    from metamorph_amd import ops as _ops
    from metamorph_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _ops


@functools.lru_cache(maxsize=None)
def prob(K):
    """the shared problem: CPU tensors under their names, device copies under name + '_d', the accumulation bound (fp64, CPU)"""
    p = E.problem(K)
    p["accb"] = E.accumulation_bound(p["a"], p["b"])
    for k in ("a", "b", "bias", "res", "res_mod", "c0_bf16", "c0_f32"):
        p[k + "_d"] = p[k].to(DEV)
    return p


@functools.lru_cache(maxsize=None)
def reference(K, flag_name, out_f32):
    """(fp64 reference [531, 523], bound) of one flag set, evaluated once on the CPU and kept on the device: every geometry is a window"""
    p, fl = prob(K), E.FLAGS[flag_name]
    res = (p["res_mod"] if fl.mod else p["res"]) if fl.res else None
    c0 = (p["c0_f32"] if out_f32 else p["c0_bf16"]) if fl.acc else None
    ref = E.epilogue_ref64(p["a"], p["b"], p["bias"] if fl.bias else None, res, E.RES_MOD if fl.mod else 0, fl.gelu, c0)
    return ref.to(DEV), E.epilogue_bound(ref, p["accb"], fl.gelu, out_f32).to(DEV)


@functools.lru_cache(maxsize=None)
def residual(K, geo_name, mod):
    """the residual as the geometry lays it out (first N columns of a [rows, res_cols] buffer), built once and never written"""
    p = prob(K)
    return E.residual_view(p["res_mod_d"] if mod else p["res_d"][:E.GEO[geo_name].M], E.GEO[geo_name])


def launch(ops, K, geo, fl, out_f32, variant, n_arg=False, res=None, bias=None):
    """one ops.gemm into a canary-filled allocation -> (allocation, the [M, N] view written); `res`, `bias`: other views of the same values"""
    p = prob(K)
    alloc, view = E.canary_out(geo, torch.float32 if out_f32 else BF16, DEV)
    if fl.acc:
        view.copy_((p["c0_f32_d"] if out_f32 else p["c0_bf16_d"])[:geo.M, :geo.N])
    if fl.res and res is None:
        res = residual(K, geo.name, fl.mod)
    if bias is None:
        bias = p["bias_d"]
    kw = dict(bias=bias[:geo.N] if fl.bias else None, gelu=fl.gelu, residual=res if fl.res else None,
              res_row_mod=E.RES_MOD if fl.mod else 0, accumulate=fl.acc, variant=variant)
    if n_arg:                                                    # the weight and the output wider than the problem: n= cuts both
        assert alloc.shape[1] - geo.col0 > geo.N
        ops.gemm(p["a_d"][:geo.M], p["b_d"], out=alloc[:geo.M, geo.col0:], n=geo.N, **kw)
    else:
        ops.gemm(p["a_d"][:geo.M], p["b_d"][:geo.N], out=view, **kw)
    return alloc, view


def same_bits(x, y, what):
    ity = E.CANARY[x.dtype][0]
    diff = x.contiguous().view(ity) != y.contiguous().view(ity)
    if bool(diff.any()):
        r, c = divmod(int(diff.view(-1).int().argmax()), x.shape[1])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} elements differ in their bits; first at ({r}, {c}): "
                             f"{float(x[r, c]):.9g} against {float(y[r, c]):.9g}")


def run_cell(ops, K, fl, out_f32, variants):
    """every geometry x variant of one (K, flag set, output type): assertions 1 and 4 per launch -> {(geometry, variant): the window written}"""
    ref, bound = reference(K, fl.name, out_f32)
    got, worst = {}, 0.0
    for geo in E.GEOMETRIES:
        cls = E.column_classes(geo, fl.res)
        for v in variants:
            what = f"{geo.name} {fl.name} {'fp32' if out_f32 else 'bf16'} K={K} variant {v}"
            alloc, view = launch(ops, K, geo, fl, out_f32, v)
            E.check_untouched(alloc, geo, what)
            worst = max(worst, E.check(view, ref[:geo.M, :geo.N], bound[:geo.M, :geo.N], what, cls))
            got[geo.name, v] = view.clone()
    print(f"{fl.name} {'fp32' if out_f32 else 'bf16'} K={K}: largest |error| / bound {worst:.3f}")
    return got


def bodies_agree(got, variants, what):
    """assertion 2: columns [0, 520) of the tail, all-scalar and column-view geometries are the bits of the all-vector G1"""
    for v in variants:
        for name in ("G2", "G3", "G4", "G6"):
            same_bits(got[name, v][:, :E.N_EVEN], got["G1", v], f"{what} variant {v}: {name}[:, :520] against G1")


def variants_agree(got, variants, what):
    """assertion 3: every variant writes the bits of variant 1, on every geometry"""
    for geo in E.GEOMETRIES:
        for v in variants:
            if v != 1:
                same_bits(got[geo.name, v], got[geo.name, 1], f"{what} {geo.name}: variant {v} against variant 1")


@pytest.mark.parametrize("out_f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("fl", E.FLAG_SETS, ids=lambda f: f.name)
@pytest.mark.parametrize("K", [256, 192])
def test_gemm_epilogue_store_bodies_and_variants(ops, K, fl, out_f32):
    """K = 256: whole pairs of K tiles, variant 11 is the ping-pong kernel; K = 192: it falls back to the pipelined 256 x 256 kernel."""
    got = run_cell(ops, K, fl, out_f32, VARIANTS)
    what = f"{fl.name} {'fp32' if out_f32 else 'bf16'} K={K}"
    bodies_agree(got, VARIANTS, what)
    variants_agree(got, VARIANTS, what)


@pytest.mark.parametrize("out_f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("fl", E.FLAG_SETS, ids=lambda f: f.name)
def test_gemm_epilogue_at_a_ragged_k_runs_on_the_register_staged_kernel_only(ops, fl, out_f32):
    """K = 72 (no whole 64-wide K tile): variant 1 and the dispatcher (which picks it) run; 2, 7, 9 and 11 refuse with MM355_EUNSUPPORTED
    and write nothing."""
    from metamorph_amd.lib import Mm355Error
    K = 72
    got = run_cell(ops, K, fl, out_f32, (1, 0))
    what = f"{fl.name} {'fp32' if out_f32 else 'bf16'} K={K}"
    bodies_agree(got, (1, 0), what)
    variants_agree(got, (1, 0), what)
    geo = E.GEO["G2"]
    p = prob(K)
    for v in (2, 7, 9, 11):
        alloc, view = E.canary_out(geo, torch.float32 if out_f32 else BF16, DEV)
        before = alloc.clone()
        with pytest.raises(Mm355Error, match=r"\(-2\)$"):
            ops.gemm(p["a_d"], p["b_d"], out=view, variant=v)
        same_bits(alloc, before, f"refused variant {v}")


@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm_n_argument_cuts_a_wider_weight_and_output(ops, variant):
    """ops.gemm(n=) with n below out.shape[1] (and, for G5, far below b.shape[0]): the launch must stop at column n -- the output's columns
    beyond it, and the weight's rows beyond it, are there to be used by a launch that takes N from a shape."""
    K = 256
    for gname, fname, out_f32 in (("G6", "bias_res_mod", False), ("G2", "bias_tanh_res_acc", True), ("G5", "bias_erf", False)):
        geo, fl = E.GEO[gname], E.FLAGS[fname]
        ref, bound = reference(K, fl.name, out_f32)
        what = f"n= {gname} {fname} variant {variant}"
        alloc, view = launch(ops, K, geo, fl, out_f32, variant, n_arg=True)
        E.check_untouched(alloc, geo, what)
        E.check(view, ref[:geo.M, :geo.N], bound[:geo.M, :geo.N], what, E.column_classes(geo, fl.res))
        same_bits(view, launch(ops, K, geo, fl, out_f32, variant)[1], what + " against the launch on the cut operands")


@pytest.mark.parametrize("out_f32", [False, True], ids=["bf16", "fp32"])
def test_gemm_window_bias_and_residual_at_the_least_alignment_taken(ops, out_f32):
    """Bases exactly 16 bytes into an aligned row -- the least the entry point accepts -- for the output window (column 8 of a bf16 buffer,
    column 4 of an fp32 one), the bias and the residual (column 8 of a 536-wide buffer): the vector body's 16-byte accesses then sit on
    16-byte and no coarser boundaries.  The bits of the 128-byte-aligned window G6, the fp64 bound, the canary."""
    K, g6 = 256, E.GEO["G6"]
    geo = g6._replace(name="G6 at 16 bytes", col0=4 if out_f32 else 8, res_cols=536)
    p = prob(K)
    bias_buf = torch.cat([torch.full((8,), E.RES_PAD, dtype=BF16, device=DEV), p["bias_d"]])
    for fname in ("bias_res_mod", "bias_erf_res", "bias_tanh_res_acc"):
        fl = E.FLAGS[fname]
        src = p["res_mod_d"] if fl.mod else p["res_d"]
        res_buf = torch.full((src.shape[0], 536), E.RES_PAD, dtype=BF16, device=DEV)
        res_buf[:, 8:8 + geo.N] = src
        res = res_buf[:, 8:8 + geo.N]
        ref, bound = reference(K, fname, out_f32)
        for v in VARIANTS:
            what = f"{geo.name} {fname} {'fp32' if out_f32 else 'bf16'} variant {v}"
            alloc, view = launch(ops, K, geo, fl, out_f32, v, res=res, bias=bias_buf[8:])
            assert view.data_ptr() % 32 == 16 and bias_buf[8:].data_ptr() % 32 == 16 and res.data_ptr() % 32 == 16
            E.check_untouched(alloc, geo, what)
            E.check(view, ref, bound, what, E.column_classes(geo, True))
            same_bits(view, launch(ops, K, g6, fl, out_f32, v)[1], what + " against G6")


def test_gemm_pair_accumulates_into_ragged_windows(ops):
    """mm355_gemm_pair_bf16 with accumulate: a bf16 target whose rows are 523 apart (scalar body everywhere) beside an fp32 target that is
    the first 523 columns of a 528-wide buffer (vector chunks + tail), then the two swapped: the bits of variant 11 launched per problem,
    nothing outside either window."""
    K, fl = 256, E.FLAGS["acc"]
    p = prob(K)
    for g0, g1 in ((E.GEO["G3"], E.GEO["G2"]), (E.GEO["G2"], E.GEO["G3"]), (E.GEO["G5"], E.GEO["G6"])):
        a0, v0 = E.canary_out(g0, BF16, DEV)
        a1, v1 = E.canary_out(g1, torch.float32, DEV)
        v0.copy_(p["c0_bf16_d"][:g0.M, :g0.N])
        v1.copy_(p["c0_f32_d"][:g1.M, :g1.N])
        if not ops.gemm_pair_supported(p["a_d"][:g0.M], p["b_d"][:g0.N], p["a_d"][:g1.M], p["b_d"][:g1.N]):
            pytest.fail("K = 256 operands must be eligible for the pair launch")
        ops.gemm_pair(p["a_d"][:g0.M], p["b_d"][:g0.N], v0, True, p["a_d"][:g1.M], p["b_d"][:g1.N], v1, True)
        what = f"pair {g0.name} bf16 + {g1.name} fp32"
        E.check_untouched(a0, g0, what)
        E.check_untouched(a1, g1, what)
        for geo, view, out_f32 in ((g0, v0, False), (g1, v1, True)):
            ref, bound = reference(K, "acc", out_f32)
            E.check(view, ref[:geo.M, :geo.N], bound[:geo.M, :geo.N], f"{what}: {geo.name}", E.column_classes(geo, False))
            same_bits(view, launch(ops, K, geo, fl, out_f32, 11)[1], f"{what}: {geo.name} against variant 11")


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("out_cols", [128258, 128264], ids=["all_scalar", "vector_and_tail"])
def test_gemm_fp32_logits_past_2_31_elements(ops, out_cols, variant):
    """The lm_head's store at a size only an evaluation pass reaches: 16 800 rows of V = 128 258 fp32 logits, 2.15e9 elements (8.6 GB), so
    the element index grow * ldc + c passes 2^31 at row 16 743 -- a fault that can show at no smaller size.  Rows 128 258 apart send
    every element through the scalar body, rows 128 264 apart through the vector body and a 2-column tail.  With a bias, so that the store
    has work to do.  Row windows at the start, across the 2^31 mark and at the end hold the bits of the same launch on those
    rows alone and meet the fp64 bound; every element of the window is written, the padding columns keep the canary."""
    M, N, K = 16800, 128258, 64
    g = torch.Generator(device=DEV).manual_seed(77)
    a = (torch.randn(M, K, generator=g, device=DEV) * 0.3).bfloat16()
    b = (torch.randn(N, K, generator=g, device=DEV) * 0.3).bfloat16()
    bias = (torch.randn(N, generator=g, device=DEV) * 0.5).bfloat16()
    geo = E.Geometry("logits", M, N, out_cols, 0, 0, out_cols)
    assert M * out_cols > 2 ** 31 and (2 ** 31 // out_cols) + 40 < M
    alloc, view = E.canary_out(geo, torch.float32, DEV)
    ops.gemm(a, b, out=view, bias=bias, variant=variant)
    assert not bool(torch.isnan(view).any()), "an element of the window was not written"
    if out_cols > N:
        assert bool((alloc[:, N:].view(torch.int32) == E.CANARY[torch.float32][1]).all()), "a padding column was written"
    cross = 2 ** 31 // out_cols - 32
    for lo in (0, cross, M - 64):
        rows = slice(lo, lo + 64)
        small, sview = E.canary_out(geo._replace(M=64), torch.float32, DEV)
        ops.gemm(a[rows], b, out=sview, bias=bias, variant=variant)
        same_bits(view[rows], sview, f"rows {lo} .. {lo + 64} against the launch on those rows")
        ref = E.epilogue_ref64(a[rows], b, bias)
        E.check(view[rows], ref, E.epilogue_bound(ref, E.accumulation_bound(a[rows], b), None, True), f"rows {lo} .. {lo + 64}",
                E.column_classes(geo, False))


def test_gemm_refuses_misaligned_bases_and_contradictory_flags(ops):
    """MM355_EINVAL (-1), never an approximation, and nothing written: an output view, a bias or a residual whose base is not 16-byte
    aligned; both GELU flags; a pair launch with any flag other than accumulate / fp32 output."""
    from metamorph_amd import lib
    from metamorph_amd.lib import Mm355Error
    L = lib.load()
    K, geo = 256, E.GEO["G2"]
    p = prob(K)
    a, b, M, N = p["a_d"], p["b_d"], geo.M, geo.N
    st = torch.cuda.current_stream().cuda_stream
    for dtype in (BF16, torch.float32):
        big = E.canary_out(E.GEO["G6"], dtype, DEV)[0]
        before = big.clone()
        off = 4 if dtype == BF16 else 2                          # 8 bytes into a row
        assert big[:, off:off + N].data_ptr() % 16 == 8
        with pytest.raises(Mm355Error, match=r"\(-1\)$"):
            ops.gemm(a, b, out=big[:M, off:off + N])
        wide_bias = torch.zeros(N + 8, dtype=BF16, device=DEV)
        wide_res = torch.zeros(M, 536, dtype=BF16, device=DEV)
        with pytest.raises(Mm355Error, match=r"\(-1\)$"):
            ops.gemm(a, b, out=big[:M, 64:64 + N], bias=wide_bias[4:4 + N])
        with pytest.raises(Mm355Error, match=r"\(-1\)$"):
            ops.gemm(a, b, out=big[:M, 64:64 + N], residual=wide_res[:, 4:4 + N])
        f32 = ops.GEMM_OUT_F32 if dtype == torch.float32 else 0
        out = big[:M, 64:64 + N]
        for variant in VARIANTS:
            rc = L.mm355_gemm_bf16(a.data_ptr(), K, b.data_ptr(), K, out.data_ptr(), out.stride(0), M, N, K, wide_bias.data_ptr(), 0, 0, 0,
                                   ops.GEMM_BIAS | ops.GEMM_GELU_ERF | ops.GEMM_GELU_TANH | f32, variant, st)
            assert rc == -1, (variant, rc)
        big1, out1 = E.canary_out(geo, dtype, DEV)               # the pair's second problem: the same product into a G2 window
        before1 = big1.clone()
        p0 = [a.data_ptr(), K, b.data_ptr(), K, out.data_ptr(), out.stride(0), M, N, K]
        p1 = p0[:4] + [out1.data_ptr(), out1.stride(0), M, N, K]
        for bad in (ops.GEMM_BIAS, ops.GEMM_GELU_ERF, ops.GEMM_GELU_TANH, ops.GEMM_RESIDUAL, ops.GEMM_BIAS | ops.GEMM_ACCUMULATE, 64):
            for flags in ((bad | f32, f32), (f32, bad | f32)):     # the offending flag on either problem
                rc = L.mm355_gemm_pair_bf16(*p0, flags[0], *p1, flags[1], st)
                assert rc == -1, (bad, flags, rc)
        torch.cuda.synchronize()
        same_bits(big, before, "refused launches")
        same_bits(big1, before1, "refused launches, second problem")
        # the same pair call without the flag is taken (the refusals above are the flag's doing) and stores through the same two bodies
        assert L.mm355_gemm_pair_bf16(*p0, f32, *p1, f32, st) == 0
        E.check_untouched(big, E.GEO["G6"], "pair launch")
        E.check_untouched(big1, geo, "pair launch, second problem")
        ref, bound = reference(K, "none", dtype == torch.float32)
        E.check(out, ref, bound, "pair launch", E.column_classes(E.GEO["G6"], False))
        same_bits(out1, out, "pair launch: the two problems")
        same_bits(out, launch(ops, K, E.GEO["G6"], E.FLAGS["none"], dtype == torch.float32, 11)[1], "pair launch against variant 11")
