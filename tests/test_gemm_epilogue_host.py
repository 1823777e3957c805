"""CPU-only: the oracle, bound and checker of tests/gemm_epilogue_refs.py, proved on an fp32 emulation of the fused GEMM store before they
judge a kernel.  The emulation is the kernel's order of operations on an fp32 accumulator (bias, GELU, residual, accumulate, one
round-to-nearest-even to bf16 at the end), written without the fp64 oracle's code.  It must pass `check` on every geometry, flag set and
output type of tests/test_gemm_epilogue_gpu.py; each of eight emulated mutants -- the ways a rewritten store goes wrong on its ragged
edge -- must fail it on every case the mutation touches and on no other.  So the derived bound separates a wrong store from a right one
in every cell of the table, and a GPU failure names a defect of the kernel, not of the yardstick.  Only the emulation is ever mutated."""
import functools
import re

import pytest
import torch

import gemm_epilogue_refs as E

K_HOST = 256


@functools.lru_cache(maxsize=None)
def prob(K):
    p = E.problem(K)
    p["acc32"] = p["a"].float() @ p["b"].float().t()
    p["accb"] = E.accumulation_bound(p["a"], p["b"])
    return p


def gelu32(x, kind):
    """mm355_common.h's gelu_erf_f / gelu_tanh_f, operation by operation in fp32"""
    assert x.dtype == torch.float32
    if kind == "erf":
        return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))
    return 0.5 * x * (1.0 + torch.tanh(0.79788456080286535588 * (x + 0.044715 * x * x * x)))


MUTANTS = {      # name -> the cases it changes: (geometry, flags, out_f32) -> bool
    "res_tail_dropped": lambda g, f, o32: f.res and g.N % 8 != 0,
    "res_row_unwrapped": lambda g, f, o32: f.mod and g.M > E.RES_MOD,
    "res_row_mod16": lambda g, f, o32: f.mod and g.M > 16,
    "gelu_before_bias": lambda g, f, o32: f.bias and f.gelu is not None,
    "bias_tail_off_by_one": lambda g, f, o32: f.bias and g.N % 8 != 0,
    "c0_ignored": lambda g, f, o32: f.acc,
    "f32_through_bf16": lambda g, f, o32: o32,
    "k_missing": lambda g, f, o32: True,
}


def emulate(p, geo, fl, out_f32, mutant=None):
    """the store's chain on the fp32 accumulator -> [M, N] of the output type"""
    M, N = geo.M, geo.N
    a, b = p["a"][:M], p["b"][:N]
    x = p["acc32"][:M, :N].clone()
    tail = E.tail_columns(geo)
    if mutant == "k_missing":                                   # one K element never reaches the sum
        x -= a[:, 37].float()[:, None] * b[:, 37].float()[None, :]
    bias = None
    if fl.bias:
        bias = p["bias"].float()[:N].clone()
        if mutant == "bias_tail_off_by_one":                    # the tail chunk reads bias[c + 1]
            nxt = torch.cat([p["bias"].float(), torch.tensor([0.75])])
            bias[tail] = nxt[tail + 1]
    if bias is not None and mutant != "gelu_before_bias":
        x += bias
    if fl.gelu is not None:
        x = gelu32(x, fl.gelu)
    if bias is not None and mutant == "gelu_before_bias":
        x += bias
    if fl.res:
        rows = torch.arange(M)
        if fl.mod:
            res = p["res_mod"]
            if mutant == "res_row_unwrapped":                   # row instead of row % res_row_mod: whatever lies behind the 177 rows
                res = torch.cat([res, p["res"][E.RES_MOD:]])
            elif mutant == "res_row_mod16":                     # the row inside the 16-row fragment group instead of the global row
                rows = (rows % 16) % E.RES_MOD
            else:
                rows = rows % E.RES_MOD
        else:
            res = p["res"]
        r = res.float()[rows, :N]
        if mutant == "res_tail_dropped":
            r[:, tail] = 0.0
        x += r
    if fl.acc and mutant != "c0_ignored":                       # (ignored: the old C is read after the store overwrote it, or not at all)
        x += (p["c0_f32"] if out_f32 else p["c0_bf16"].float())[:M, :N]
    if out_f32:
        return x.bfloat16().float() if mutant == "f32_through_bf16" else x
    return x.bfloat16()


@functools.lru_cache(maxsize=None)
def reference(K, flag_name, out_f32):
    """(fp64 reference [531, 523], bound) of one flag set: every geometry is a window of them"""
    p, fl = prob(K), E.FLAGS[flag_name]
    res = (p["res_mod"] if fl.mod else p["res"]) if fl.res else None
    c0 = (p["c0_f32"] if out_f32 else p["c0_bf16"]) if fl.acc else None
    ref = E.epilogue_ref64(p["a"], p["b"], p["bias"] if fl.bias else None, res, E.RES_MOD if fl.mod else 0, fl.gelu, c0)
    return ref, E.epilogue_bound(ref, p["accb"], fl.gelu, out_f32)


def judge(K, geo, fl, out_f32, mutant=None):
    ref, bound = reference(K, fl.name, out_f32)
    got = emulate(prob(K), geo, fl, out_f32, mutant)
    what = f"{geo.name} {fl.name} {'fp32' if out_f32 else 'bf16'} K={K}" + (f" mutant {mutant}" if mutant else "")
    return E.check(got, ref[:geo.M, :geo.N], bound[:geo.M, :geo.N], what, E.column_classes(geo, fl.res))


def test_the_geometries_reach_the_store_bodies_the_table_says():
    V, T, S = E.VECTOR, E.TAIL, E.SCALAR
    want = {  # name: (classes without a residual, with one)
        "G1": ({V}, {V}), "G2": ({V, T}, {V, T}), "G3": ({S}, {S}), "G4": ({V}, {S}), "G5": ({T}, {T}), "G6": ({V, T}, {V, T})}
    for g in E.GEOMETRIES:
        for with_res in (False, True):
            cls = E.column_classes(g, with_res)
            assert set(cls.tolist()) == want[g.name][with_res], (g.name, with_res)
            if T in want[g.name][with_res]:
                assert cls.tolist() == [V] * (g.N - g.N % 8) + [T] * (g.N % 8)
        assert g.out_cols >= g.col0 + g.N and g.res_cols >= g.N and (g.col0 * 2) % 16 == 0
    assert E.M_FULL == 2 * 256 + 19 == 3 * E.RES_MOD and E.RES_MOD % 16 != 0 and E.N_FULL % 8 == 3 and E.N_EVEN % 8 == 0
    assert len(E.FLAG_SETS) == 10 and len(E.GEOMETRIES) == 6


@pytest.mark.parametrize("K", [256, 192, 72])
@pytest.mark.parametrize("fl", E.FLAG_SETS, ids=lambda f: f.name)
def test_the_fp32_emulation_meets_the_derived_bound_everywhere(fl, K):
    worst = 0.0
    for geo in E.GEOMETRIES:
        for out_f32 in (False, True):
            worst = max(worst, judge(K, geo, fl, out_f32))
    print(f"{fl.name} K={K}: largest |error| / bound of the emulation {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_every_mutant_fails_wherever_it_changes_the_store(mutant):
    touched, caught = [], []
    for geo in E.GEOMETRIES:
        for fl in E.FLAG_SETS:
            for out_f32 in (False, True):
                if not MUTANTS[mutant](geo, fl, out_f32):
                    continue                                    # the mutation is the identity here
                case = (geo.name, fl.name, out_f32)
                touched.append(case)
                try:
                    judge(K_HOST, geo, fl, out_f32, mutant)
                except AssertionError as e:
                    caught.append(case)
                    if mutant in ("res_tail_dropped", "bias_tail_off_by_one"):
                        want = "all-scalar column" if geo.name == "G3" else "tail chunk column"
                        assert want in str(e) and not re.search(r"[1-9]\d* in vector chunk columns", str(e)), str(e)
    assert touched and caught == touched, (mutant, sorted(set(touched) - set(caught)))


def test_the_tail_mutants_are_reported_in_tail_columns_only():
    """the report names the body: a tail defect on G2 shows 0 bad elements in vector-chunk columns"""
    with pytest.raises(AssertionError, match=r"worst at \(\d+, 52[0-2]\) \[tail chunk column; 0 in vector chunk columns, \d+ in tail chunk columns\]"):
        judge(K_HOST, E.GEO["G2"], E.FLAGS["res"], True, "res_tail_dropped")
    with pytest.raises(AssertionError, match=r"\[all-scalar column; \d+ in all-scalar columns\]"):
        judge(K_HOST, E.GEO["G3"], E.FLAGS["bias"], False, "bias_tail_off_by_one")


def test_check_counts_an_unwritten_element_and_the_canary_sees_a_stray_write():
    geo, fl = E.GEO["G6"], E.FLAGS["bias_res_mod"]
    ref, bound = reference(K_HOST, fl.name, False)
    for dtype in (torch.bfloat16, torch.float32):
        alloc, view = E.canary_out(geo, dtype, "cpu")
        assert bool(torch.isnan(alloc).all()) and view.data_ptr() % 16 == 0
        view.copy_(emulate(prob(K_HOST), geo, fl, dtype == torch.float32))
        E.check_untouched(alloc, geo, "clean")
        assert not bool(torch.isnan(view).any())
        for r, c in ((geo.M, geo.col0), (5, geo.col0 - 1), (5, geo.col0 + geo.N), (geo.M + 2, 1023)):
            stray = alloc.clone()
            stray[r, c] = 1.0
            with pytest.raises(AssertionError, match=rf"first at \({r}, {c}\)"):
                E.check_untouched(stray, geo, "stray")
    alloc, view = E.canary_out(geo, torch.bfloat16, "cpu")
    view.copy_(emulate(prob(K_HOST), geo, fl, False))
    ity, pat = E.CANARY[torch.bfloat16]
    view.view(ity)[300, 521] = pat                              # an element the launch never wrote
    with pytest.raises(AssertionError, match=r"1 of \d+ elements beyond the bound; worst at \(300, 521\) \[tail chunk"):
        E.check(view, ref[:geo.M, :geo.N], bound[:geo.M, :geo.N], "hole", E.column_classes(geo, True))


def test_the_residual_view_pads_with_a_value_no_bound_absorbs():
    p = prob(K_HOST)
    for geo in E.GEOMETRIES:
        v = E.residual_view(p["res_mod"], geo)
        assert v.shape == (E.RES_MOD, geo.N) and v.stride(0) == geo.res_cols and torch.equal(v, p["res_mod"][:, :geo.N])
    ref, bound = reference(K_HOST, "res", False)
    assert float(bound.max()) < 1e-3 * E.RES_PAD
