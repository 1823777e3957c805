"""CPU-only: the constructions of tests/transposed_refs.py that tests/test_transposed_outputs_gpu.py relies on, asserted without a kernel, so
that a failure on the GPU can only be the kernel's:

  framed            the view is 16-byte aligned, has the leading dimension asked for, and the check sees one stray element anywhere outside
                    it (front guard, back guard, the gap behind any row) and none inside
  random_bits       the transposes' input holds NaN payloads, both zeros, subnormals and infinities
  apply_t_ref       the torch fp32 reference equals an fp64 evaluation rounded with helper_refs.round_bf at the same two points, and no
                    intermediate is subnormal
  probe channels    silu(1.28125) rounds to bf16 1.0, and no fp32 evaluation can round it elsewhere
  exact operands    d act of all eight cases of the fused SwiGLU-backward GEMM is an integer of magnitude <= 256 (exact in bf16, and the same
                    under every summation order)
"""
import pytest
import torch

import helper_refs as H
import transposed_refs as T


@pytest.mark.parametrize("shape,ld,misalign", [((5, 7), 7, 0), ((5, 7), 16, 0), ((1, 1), 1, 0), ((64, 203), 208, 0), ((3, 8), 8, 4), ((9, 130), 131, 0)])
def test_framed_view_and_its_check(shape, ld, misalign):
    rows, cols = shape
    for s in T.SENTINELS:
        f = T.framed(shape, ld, s, misalign=misalign)
        assert f.view.shape == shape and f.view.stride() == (ld, 1) and f.view.dtype == torch.bfloat16
        assert f.view.data_ptr() % 16 == 2 * misalign
        assert f.start >= T.GUARD and f.bits.numel() - (f.start + rows * ld) >= T.GUARD
        assert int(f.outside().sum()) == f.bits.numel() - rows * cols
        assert bool((H.bits(f.view) == s).all())
        f.check_untouched()
        f.check_all_sentinel()
        f.view.copy_(T.random_bits(rows, cols, seed=3))                                 # the whole view, and nothing else
        f.check_untouched()
        if bool((H.bits(f.view) != s).any()):
            with pytest.raises(AssertionError):
                f.check_all_sentinel()
        # one stray element at each kind of place outside the view
        places = [0, f.start - 1, f.start + rows * ld - 1 + (1 if ld == cols else 0), f.bits.numel() - 1]
        if ld > cols:
            places += [f.start + cols, f.start + (rows - 1) * ld + cols, f.start + (rows // 2) * ld + ld - 1]
        for p in places:
            keep = int(f.bits[p])
            f.bits[p] = keep ^ 0x100
            with pytest.raises(AssertionError):
                f.check_untouched()
            f.bits[p] = keep
            f.check_untouched()


def test_sentinels_differ_and_are_ordinary_values():
    a, b = T.SENTINELS
    assert a != b
    v = torch.tensor([T._i16(a), T._i16(b)], dtype=torch.int16).view(torch.bfloat16)
    assert bool(torch.isfinite(v.float()).all()) and bool((H.bits(v) == torch.tensor([a, b])).all())


def test_leading_dimensions_of_the_grids():
    for n in range(1, 300):
        assert T.ceil8(n) % 8 == 0 and 0 <= T.ceil8(n) - n < 8
        assert T.ragged_ld(n) % 8 != 0 and 0 <= T.ragged_ld(n) - n <= 1
    grid = list(T.transpose_grid())
    assert len(grid) == 8 * 8 * 2 * 3
    assert any(c % 8 and lo % 8 for _, c, _, lo in grid) and all(li % 8 == 0 and li >= c and lo >= r for r, c, li, lo in grid)


def test_random_bits_hold_every_class():
    """the strided-input case of the GPU test (a column block of a [777, 3456] matrix): NaNs with many payloads, +0, -0, subnormals, both
    infinities -- a transpose that goes through arithmetic, or flushes, changes some of them"""
    wide = T.random_bits(777, 3456, seed=11)
    b = H.bits(wide[:, 1152:2304])
    f = wide[:, 1152:2304].float()
    nan = torch.isnan(f)
    assert len(torch.unique(b[nan])) > 200
    assert bool((b == 0x0000).any()) and bool((b == 0x8000).any())
    assert bool((b == 0x7F80).any()) and bool((b == 0xFF80).any())
    assert int(H.subnormal(wide[:, 1152:2304]).sum()) > 1000
    # uniform: every one of the 256 high bytes occurs
    assert len(torch.unique(b >> 8)) == 256
    # the same numbers on every call, and a view with a gap is a view of the same flat draw
    assert T.same_bits(wide, T.random_bits(777, 3456, seed=11))
    v = T.random_bits(9, 7, ld=16, seed=2)
    assert v.stride() == (16, 1) and v.shape == (9, 7)


@pytest.mark.parametrize("M", T.APPLY_T_M)
@pytest.mark.parametrize("h", T.APPLY_T_H)
def test_apply_t_reference_is_the_fp64_evaluation(M, h):
    x, w, rstd = T.apply_t_inputs(M, h)
    assert rstd.dtype == torch.float32 and bool((rstd > 0).all()) and float(rstd.min()) >= 0.125 and float(rstd.max()) < 8.0
    ref = T.apply_t_ref(x, w, rstd)
    ref64, t32, t = T.apply_t_ref64(x, w, rstd)
    assert ref.shape == (h, M) and ref.dtype == torch.bfloat16
    assert torch.equal(ref.double(), ref64)
    assert bool(torch.isfinite(ref64).all())
    for name, v in (("x", x), ("w", w), ("rstd", rstd), ("x * rstd", t32), ("bf16(x * rstd)", t), ("result", ref64)):
        assert not bool(H.subnormal(v).any()), name
        assert bool((v.double() != 0).all()), name
    if M > 1:
        # a neighbouring row's rstd gives other bits in (nearly) every element: the reference can tell which row's rstd was used
        other = T.apply_t_ref(x, w, torch.roll(rstd, -1))
        assert float((H.bits(other) != H.bits(ref)).float().mean()) > 0.9


def test_probe_gate_rounds_to_one():
    g = torch.tensor([T.PROBE_GATE], dtype=H.F64)
    assert float(g.to(torch.bfloat16).double()) == T.PROBE_GATE                       # a bf16 value
    silu = g * torch.sigmoid(g)
    assert abs(float(silu) - 1.00279) < 1e-5
    assert float(H.round_bf(silu)) == 1.0
    assert not bool(H.near_tie(silu, 1e-4).any())                                        # an fp32 chain is within ~1e-6: it cannot round elsewhere
    assert float(H.swiglu_fwd64(g, torch.tensor([0.37], dtype=H.F64))) == 0.37
    assert float(H.swiglu_bwd64(g, torch.tensor([0.37], dtype=H.F64), torch.tensor([-3.0], dtype=H.F64))[1]) == -3.0
    for I in (64, 192, 4672):
        pc = T.probe_channels(I)
        assert bool((pc % 16 == 5).all()) and len(pc) == I // 16 and int(pc[-1]) == I - 11
        gu = T.swb_gu(16, I, 2 * I + 8, seed=I)
        assert gu.shape == (16, 2 * I) and gu.stride() == (2 * I + 8, 1)
        assert bool((gu[:, pc].double() == T.PROBE_GATE).all())
        rest = torch.ones(2 * I, dtype=torch.bool)
        rest[pc] = False
        assert bool(torch.isfinite(gu[:, rest].float()).all()) and float(gu[:, rest].float().std()) > 1.3
        assert not bool((gu[:, I:].double() == T.PROBE_GATE).all())                  # the up half is left as drawn


@pytest.mark.parametrize("k", range(len(T.SWB_CASES)))
def test_exact_operands_give_integers_bf16_holds(k):
    M, I, K, pgu, pdgu, pT = T.SWB_CASES[k]
    assert M % 8 == 0 and I % 64 == 0 and K % 128 == 0 and pgu % 8 == 0 and pdgu % 8 == 0 and pT % 8 == 0
    dy, wdT = T.swb_operands(M, I, K, T.swb_seed(k, True), exact=True)
    assert dy.shape == (M, K) and wdT.shape == (I, K)
    for t in (dy, wdT):
        assert set(torch.unique(t.double()).tolist()) == {-1.0, 0.0, 1.0}
    da = T.dact64(dy, wdT)
    assert torch.equal(da, da.round())
    m = float(da.abs().max())
    print(f"[exact] case {k + 1}: max |d act| = {m:g}")
    assert 0 < m <= T.EXACT_MAX
    assert torch.equal(da.to(torch.bfloat16).double(), da)                               # exact in bf16
    # random mode: other numbers, of the scale of test_gemm_fp32_output_tight
    ry, rw = T.swb_operands(M, I, K, T.swb_seed(k, False), exact=False)
    assert 0.9 < float(ry.float().std()) < 1.1 and 0.9 < float(rw.float().std()) < 1.1


def test_case_table_reaches_what_it_claims():
    """tile counts and the XCD remainder (total & 7) of the 256 x 256 tile grid, the raster groups of four row tiles, the 8-row cuts"""
    tiles = [((M + 255) // 256, (I + 255) // 256) for M, I, *_ in T.SWB_CASES]
    assert tiles == [(1, 1), (2, 1), (1, 1), (2, 2), (3, 3), (6, 3), (8, 1), (11, 19)]
    assert [(a * b) & 7 for a, b in tiles] == [1, 2, 1, 4, 1, 2, 0, 1]
    assert [M % 256 for M, *_ in T.SWB_CASES] == [8, 8, 200, 136, 8, 8, 8, 64]       # 136 = 128 + 8: wm = 1 has 8 live rows
    assert T.SWB_CASES[2][1] % 256 == 192 and T.SWB_CASES[2][0] % 64 != 0
    assert T.SWB_CASES[4][2] == 3 * 128
    M, I, K = T.SWB_CASES[7][:3]
    assert M % 64 == 0 and ((M + 255) // 256) * ((I + 255) // 256) >= 200 > ((M - 64 + 255) // 256) * ((I + 255) // 256)
