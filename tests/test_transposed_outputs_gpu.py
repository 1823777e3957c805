"""The four kernels that write the contraction-major copies the decoder's weight-gradient GEMMs read -- mm355_transpose_bf16,
mm355_rmsnorm_apply_t, mm355_swiglu_bwd_t and mm355_gemm_swiglu_bwd_bf16 -- at the edges of their store paths: ragged rows and columns,
every leading dimension padded, the scalar load / store branches, 8-row cuts inside a wave's 128 rows, a wave column outside I, tile counts
of every XCD remainder, byte offsets past 2^31.  Needs an MI355X:  pytest -m gpu

Every output lives inside a sentinel-filled buffer (transposed_refs.framed): nothing outside the view may change, and each call runs over two
different sentinels with the reference's bits required both times, so every element of the view is shown to be written.  The C entry points
are driven through ctypes wherever the ops wrapper would hide a path (it zeroes padding, fixes ldT = M, packs gu).

References: bit-exact torch (x.t(), the two-rounding fp32 chain of rmsnorm_apply_t), the fp64 SwiGLU of helper_refs under the bounds
test_helpers_gpu._swiglu_case already uses, an fp64 matrix product under the bound of test_gemm_fp32_output_tight, and -- only next to
those -- the project's own unfused chain under the allowance test_gemm_swiglu_bwd_fused_equals_two_launches grants.  No tolerance is new.
tests/test_transposed_refs_host.py asserts the constructions on the CPU.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import helper_refs as H  # noqa: E402
import test_helpers_gpu as G  # noqa: E402  (_domain_check, UVALS, DAVALS: the gate-domain check of swiglu_bwd, unchanged)
import transposed_refs as T  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
KC = H.KERNEL_C_FACTOR
CF, CG, CU = (KC * H.STACK_C[k] for k in ("swiglu_fwd", "swiglu_dgate", "swiglu_dup"))
EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def ops():
    from metamorph_amd import ops as _ops
    from metamorph_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _ops


@pytest.fixture(scope="module")
def L(ops):
    from metamorph_amd import lib
    return lib.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits_eq(got, want, what):
    if not T.same_bits(got, want):
        assert got.shape == want.shape, (what, got.shape, want.shape)
        bad = H.bits(got) != H.bits(want)
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements differ in bits; first at {i}: got {int(H.bits(got)[i]):#06x} "
                             f"want {int(H.bits(want)[i]):#06x}")


# ================================================================================================ A. mm355_transpose_bf16

def _transpose(L, x, rows, cols, ld_in, out, ld_out):
    return L.mm355_transpose_bf16(x.data_ptr(), ld_in, rows, cols, out.data_ptr(), ld_out, _stream())


def test_transpose_small_grid_bit_for_bit(L):
    """rows in {1, 7, 8, 9, 63, 64, 65, 130} x cols in {1, 7, 8, 9, 63, 64, 65, 203} x ld_in in {ceil8, ceil8 + 8} x ld_out in {ceil8, ceil8 + 8,
    ragged}: uniformly random 16-bit patterns (NaN payloads, +-0, subnormals) must arrive as x.t() bit for bit.  cols % 8 != 0 takes the
    scalar loads, a ragged ld_out the scalar stores."""
    n = 0
    for rows, cols, ld_in, ld_out in T.transpose_grid():
        x = T.random_bits(rows, cols, ld_in, seed=1000 * rows + cols, device=DEV)
        for s in T.SENTINELS:
            f = T.framed((cols, rows), ld_out, s, DEV)
            what = f"transpose {rows}x{cols} ld_in {ld_in} ld_out {ld_out} sentinel {s:#06x}"
            assert _transpose(L, x, rows, cols, ld_in, f.view, ld_out) == 0, what
            _bits_eq(f.view, x.t(), what)
            f.check_untouched(what)
            n += 1
    assert n == 768


def test_transpose_strided_input_into_padded_output(L):
    """functional.transpose_padded's call: a column block wide[:, 1152:2304] of [777, 3456] into [:, :777] of a [1152, 896] buffer"""
    wide = T.random_bits(777, 3456, seed=11, device=DEV)
    x = wide[:, 1152:2304]
    for s in T.SENTINELS:
        f = T.framed((1152, 777), 896, s, DEV)
        assert _transpose(L, x, 777, 1152, 3456, f.view, 896) == 0
        _bits_eq(f.view, x.t(), "strided transpose")
        f.check_untouched("strided transpose")


def test_transpose_byte_offsets_past_2_31(L):
    """rows = 16392, cols = 65544 (both ragged by 8): 1.074 G elements, the last row starts past 2 GiB on both sides -- the smallest
    such shape, and the size of the 70B lm_head transpose in linear_ce.hip.  Compared on the device."""
    rows, cols = 16392, 65544
    assert (rows - 1) * cols * 2 > 2 ** 31 and (cols - 1) * rows * 2 > 2 ** 31
    x = T.random_bits(rows, cols, seed=5, device=DEV)
    f = T.framed((cols, rows), rows, T.SENTINELS[0], DEV)
    assert _transpose(L, x, rows, cols, cols, f.view, rows) == 0
    assert torch.equal(f.view.view(torch.int16), x.view(torch.int16).t())
    f.check_untouched("2 GiB transpose")


def test_transpose_refusals_touch_nothing(L):
    """ld_out < rows, ld_in % 8 != 0, a base pointer 8 bytes past a 16-byte boundary (either side), rows = 0: MM355_EINVAL, output unwritten"""
    rows, cols = 16, 8
    xbuf = T.random_bits(64, 64, seed=1, device=DEV)
    f = T.framed((64, 64), 64, T.SENTINELS[0], DEV)
    fm = T.framed((64, 64), 64, T.SENTINELS[1], DEV, misalign=4)
    x_off = xbuf.view(-1)[4:]
    assert x_off.data_ptr() % 16 == 8 and fm.view.data_ptr() % 16 == 8
    assert _transpose(L, xbuf, rows, cols, 64, f.view, 8) == EINVAL                    # ld_out < rows
    assert _transpose(L, xbuf, rows, cols, 12, f.view, 16) == EINVAL                   # ld_in % 8 != 0
    assert _transpose(L, x_off, rows, cols, 64, f.view, 16) == EINVAL                  # misaligned input
    assert _transpose(L, xbuf, rows, cols, 64, fm.view, 16) == EINVAL                  # misaligned output
    assert _transpose(L, xbuf, 0, cols, 64, f.view, 16) == EINVAL                      # rows = 0
    torch.cuda.synchronize()
    f.check_all_sentinel("transpose refusals")
    fm.check_all_sentinel("transpose refusals")
    assert _transpose(L, xbuf, rows, cols, 64, f.view, 16) == 0                        # the same buffers are taken once the arguments are right
    _bits_eq(f.buf.as_strided((cols, rows), (16, 1), f.start), xbuf[:rows, :cols].t(), "transpose after refusals")


# ================================================================================================ B. mm355_rmsnorm_apply_t

def _apply_t(L, x, w, rstd, M, h, out, ld_out):
    return L.mm355_rmsnorm_apply_t(x.data_ptr(), w.data_ptr(), rstd.data_ptr(), M, h, out.data_ptr(), ld_out, _stream())


@pytest.mark.parametrize("M", T.APPLY_T_M)
def test_rmsnorm_apply_t_raw_call_bit_for_bit(L, M):
    """M in {1, 8, 63, 65, 300} x h in {8, 64, 72, 1160} (h % 64 != 0: column blocks partly outside) x ld_out in {ceil8(M), ceil8(M) + 128,
    ragged}, the C entry point alone: rstd is ARBITRARY positive fp32 (not x's), the reference the torch fp32 chain with its two roundings
    (transposed_refs.apply_t_ref, shown equal to fp64 + round_bf on the host).  The raw call does not zero: padding columns [M, ld_out) keep
    the sentinel, like everything else outside the view."""
    for h in T.APPLY_T_H:
        x, w, rstd = T.apply_t_inputs(M, h)
        want = T.apply_t_ref(x, w, rstd).to(DEV)
        x, w, rstd = x.to(DEV), w.to(DEV), rstd.to(DEV)
        for ld_out in (T.ceil8(M), T.ceil8(M) + 128, T.ragged_ld(M)):
            for s in T.SENTINELS:
                f = T.framed((h, M), ld_out, s, DEV)
                what = f"rmsnorm_apply_t M {M} h {h} ld_out {ld_out} sentinel {s:#06x}"
                assert _apply_t(L, x, w, rstd, M, h, f.view, ld_out) == 0, what
                _bits_eq(f.view, want, what)
                f.check_untouched(what)


@pytest.mark.parametrize("M,h", [(65, 72), (300, 1160)])
def test_rmsnorm_apply_t_equals_forward_transposed_at_ragged_shapes(ops, M, h):
    x, w, _ = T.apply_t_inputs(M, h, DEV)
    y, rstd = ops.rmsnorm_fwd(x, w, 1e-5, want_rstd=True)
    yt = ops.rmsnorm_apply_t(x, w, rstd)
    assert yt.shape == (h, T.ceil8(M))
    _bits_eq(yt[:, :M], y.t(), f"apply_t vs forward {M}x{h}")
    assert not bool(yt[:, M:].any())
    _bits_eq(yt[:, :M], T.apply_t_ref(x, w, rstd), f"apply_t vs torch chain {M}x{h}")


def test_rmsnorm_apply_t_refusals_touch_nothing(L):
    """h % 8 != 0, ld_out < M, a misaligned output: MM355_EINVAL, output unwritten"""
    M, h = 16, 64
    x, w, rstd = T.apply_t_inputs(M, h, DEV)
    f = T.framed((h, 32), 32, T.SENTINELS[0], DEV)
    fm = T.framed((h, 32), 32, T.SENTINELS[1], DEV, misalign=4)
    assert _apply_t(L, x, w, rstd, M, 12, f.view, 16) == EINVAL
    assert _apply_t(L, x, w, rstd, M, h, f.view, 8) == EINVAL
    assert _apply_t(L, x, w, rstd, M, h, fm.view, 16) == EINVAL
    torch.cuda.synchronize()
    f.check_all_sentinel("apply_t refusals")
    fm.check_all_sentinel("apply_t refusals")
    assert _apply_t(L, x, w, rstd, M, h, f.view, 32) == 0
    _bits_eq(f.view[:, :M], T.apply_t_ref(x, w, rstd), "apply_t after refusals")


# ================================================================================================ C. mm355_swiglu_bwd_t

def _swiglu_bwd_t_framed(L, gu, dact, M, I, s):
    fd, fa, ft = T.framed((M, 2 * I), 2 * I, s, DEV), T.framed((I, M), M, s, DEV), T.framed((2 * I, M), M, s, DEV)
    rc = L.mm355_swiglu_bwd_t(gu.data_ptr(), dact.data_ptr(), fd.view.data_ptr(), fa.view.data_ptr(), ft.view.data_ptr(), M, I, _stream())
    return rc, fd, fa, ft


def _check_swiglu_outputs(dgu, actT, dguT, g, u, da, I, what):
    """the three outputs against fp64 under the bounds of test_helpers_gpu._swiglu_case (two bf16 steps for act and the up half, one for
    the gate half), and dguT's halves as the bit transposes of dgu's"""
    ref_act = H.swiglu_fwd64(g, u)
    rg, ru = H.swiglu_bwd64(g, u, da)
    T.within(dgu[:, :I], rg, H.act_bound(rg, g, u.double() * da.double(), CG, 1), f"{what}: dgu gate half")
    T.within(dgu[:, I:], ru, H.act_bound(ru, g, da.double(), CU, 2), f"{what}: dgu up half")
    T.within(actT.t(), ref_act, H.act_bound(ref_act, g, u.double(), CF, 2), f"{what}: actT")
    _bits_eq(dguT[:I], dgu[:, :I].t(), f"{what}: dguT gate half vs dgu")
    _bits_eq(dguT[I:], dgu[:, I:].t(), f"{what}: dguT up half vs dgu")


@pytest.mark.parametrize("M,I", [(64, 64), (128, 192), (320, 64), (64 * 1025, 64)])
def test_swiglu_bwd_t_against_fp64_and_swiglu_bwd(ops, L, M, I):
    """one tile, several tiles each way, and 1025 row blocks in blockIdx.y; inputs and bounds of _swiglu_case"""
    gu = G.rnd(M, 2 * I, seed=M, scale=1.5, device=DEV)
    da = G.rnd(M, I, seed=M + 1, device=DEV)
    g, u = gu[:, :I], gu[:, I:]
    dgu0, act0 = ops.swiglu_bwd(gu, da, I)
    for s in T.SENTINELS:
        what = f"swiglu_bwd_t {M}x{I} sentinel {s:#06x}"
        rc, fd, fa, ft = _swiglu_bwd_t_framed(L, gu, da, M, I, s)
        assert rc == 0, what
        _check_swiglu_outputs(fd.view, fa.view, ft.view, g, u, da, I, what)
        _bits_eq(fd.view, dgu0, f"{what}: dgu vs swiglu_bwd")
        _bits_eq(fa.view, act0.t(), f"{what}: actT vs swiglu_bwd")
        for f in (fd, fa, ft):
            f.check_untouched(what)


def test_swiglu_bwd_t_over_all_bf16_gates(ops):
    """every bf16 gate pattern against every up value and every dact value (helper_refs.swiglu_domain: M = 128 * 18, I = 512) through
    swiglu_bwd_t, held to the masks and bounds test_swiglu_over_all_bf16_gates holds swiglu_bwd to"""
    I = 512
    gu, da = H.swiglu_domain(G.UVALS, G.DAVALS)
    g, u, d = gu[:, :I].reshape(-1), gu[:, I:].reshape(-1), da.reshape(-1)
    dgu, actT, dguT = ops.swiglu_bwd_t(gu.to(DEV), da.to(DEV), I)
    rg, ru = H.swiglu_bwd64(g, u, d)
    sg, su = H.stack_swiglu_bwd(g, u, d)
    G._domain_check("swiglu_dgate", dgu[:, :I].reshape(-1), rg, g, u.double() * d.double(), 1, sg, False)
    G._domain_check("swiglu_dup", dgu[:, I:].reshape(-1), ru, g, d.double(), 2, su, True)
    n = 65536 * len(G.UVALS)                                    # act does not depend on dact: the rows of the first dact value, as there
    G._domain_check("swiglu_fwd", actT.t().reshape(-1)[:n], H.swiglu_fwd64(g, u)[:n], g[:n], u.double()[:n], 2, H.stack_swiglu_fwd(g, u)[:n], True)
    # the transposed copies carry the same bits, NaN payloads included
    _bits_eq(dguT[:I], dgu[:, :I].t(), "domain: dguT gate half")
    _bits_eq(dguT[I:], dgu[:, I:].t(), "domain: dguT up half")
    # against swiglu_bwd over the whole domain: bit for bit, a NaN for a NaN (another kernel may pick the other operand's payload)
    dgu0, act0 = ops.swiglu_bwd(gu.to(DEV), da.to(DEV), I)
    for got, want in ((dgu, dgu0), (actT, act0.t())):
        assert bool(((H.bits(got) == H.bits(want)) | (torch.isnan(got) & torch.isnan(want))).all())


def test_swiglu_bwd_t_refusals_touch_nothing(L):
    """M = 72 or I = 72 (not whole 64 x 64 tiles): MM355_EUNSUPPORTED, outputs unwritten"""
    gu = G.rnd(128, 256, seed=1, device=DEV)
    da = G.rnd(128, 128, seed=2, device=DEV)
    for M, I in ((72, 64), (64, 72)):
        rc, fd, fa, ft = _swiglu_bwd_t_framed(L, gu, da, M, I, T.SENTINELS[0])
        assert rc == EUNSUPPORTED, (M, I, rc)
        torch.cuda.synchronize()
        for f in (fd, fa, ft):
            f.check_all_sentinel(f"swiglu_bwd_t refused M {M} I {I}")


# ================================================================================================ D. mm355_gemm_swiglu_bwd_bf16

def _swb_call(L, dy, wdT, gu, fd, fa, ft, M, I, K, ldT=None, dguT_ptr=None):
    return L.mm355_gemm_swiglu_bwd_bf16(dy.data_ptr(), dy.stride(0), wdT.data_ptr(), wdT.stride(0), gu.data_ptr(), gu.stride(0), fd.view.data_ptr(),
                                        fd.ld, fa.view.data_ptr(), ft.view.data_ptr() if dguT_ptr is None else dguT_ptr,
                                        ft.ld if ldT is None else ldT, M, I, K, _stream())


def _swb_runs(ops, L, k, dy, wdT, gu):
    """[(dgu, actT, dguT)] of two calls.  Cases 1-7: the C entry point, each output framed with the case's leading dimensions, one call per
    sentinel, frames checked.  Case 8: ops.gemm_swiglu_bwd (packed, ldT = M), which gemm_swiglu_bwd_supported must admit."""
    M, I, K, pgu, pdgu, pT = T.SWB_CASES[k]
    assert gu.stride(0) == 2 * I + pgu
    if k == 7:
        assert pgu == pdgu == pT == 0 and ops.gemm_swiglu_bwd_supported(dy, wdT, gu, I)
        return [ops.gemm_swiglu_bwd(dy, wdT, gu, I) for _ in range(2)]
    runs = []
    for s in T.SENTINELS:
        fd, fa, ft = T.framed((M, 2 * I), 2 * I + pdgu, s, DEV), T.framed((I, M), M + pT, s, DEV), T.framed((2 * I, M), M + pT, s, DEV)
        what = f"gemm_swiglu_bwd case {k + 1} sentinel {s:#06x}"
        assert _swb_call(L, dy, wdT, gu, fd, fa, ft, M, I, K) == 0, what
        torch.cuda.synchronize()
        for f, name in ((fd, "dgu"), (fa, "actT"), (ft, "dguT")):
            f.check_untouched(f"{what}: {name}")
        runs.append((fd.view, fa.view, ft.view))
    return runs


def _swb_inputs(k, exact):
    M, I, K, pgu, pdgu, pT = T.SWB_CASES[k]
    seed = T.swb_seed(k, exact)
    dy, wdT = T.swb_operands(M, I, K, seed, exact, DEV)
    gu = T.swb_gu(M, I, 2 * I + pgu, seed + 1, DEV)
    return dy, wdT, gu


@pytest.mark.parametrize("k", range(len(T.SWB_CASES)))
def test_gemm_swiglu_bwd_exact_operands(ops, L, k):
    """dy, wdT from {-1, 0, 1}: d act is an integer <= 64 in magnitude that every summation order gives exactly, so the reference is
    independent of the kernel's K order and of every other kernel of the project.
      * probe channels (gate 1.28125, bf16 silu exactly 1): the up half of dgu IS d act, actT[c] IS u[:, c], bit for bit
      * all channels: dgu's halves and actT.t() against swiglu_bwd64 / swiglu_fwd64 of the exact d act, bounds of _swiglu_case
      * dguT's halves are the bit transposes of dgu's; everything outside the three views untouched; every element written (two
        sentinels); the second call gives the bits of the first"""
    M, I, K = T.SWB_CASES[k][:3]
    dy, wdT, gu = _swb_inputs(k, True)
    da = T.dact64(dy, wdT)
    assert float(da.abs().max()) <= T.EXACT_MAX
    g, u = gu[:, :I], gu[:, I:]
    pc = T.probe_channels(I, DEV)
    runs = _swb_runs(ops, L, k, dy, wdT, gu)
    for r, (dgu, actT, dguT) in enumerate(runs):
        what = f"exact case {k + 1} call {r}"
        _bits_eq(dgu[:, I:][:, pc], da[:, pc].to(BF16), f"{what}: probe channels, dgu up half vs d act")
        _bits_eq(actT[pc], u[:, pc].t(), f"{what}: probe channels, actT vs u")
        _check_swiglu_outputs(dgu, actT, dguT, g, u, da, I, what)
    for a, b, name in zip(runs[0], runs[1], ("dgu", "actT", "dguT")):
        _bits_eq(b, a, f"exact case {k + 1}: second call, {name}")


def test_gemm_swiglu_bwd_random_operands(ops, L):
    """dy, wdT ~ N(0, 1), all eight cases.
      * probe channels: the up half of dgu equals ops.gemm(dy, wdT, variant=11) bit for bit (the same gemm_pp_tile main loop, rounded to bf16
        once), and is within 2^-8 |ref| + 4 K 2^-24 of the fp64 product (the bound of test_gemm_fp32_output_tight)
      * all three outputs against gemm(variant=11) -> swiglu_bwd -> torch transposes under the allowance the existing fused test grants:
        differing elements < 1e-3 of all elements, pooled over the eight cases, each differing element <= 2^-7 relative
      * dguT's halves are the bit transposes of dgu's, frames untouched, two calls agree"""
    pooled = {name: [0, 0] for name in ("dgu", "actT", "dguT")}
    for k, (M, I, K, *_) in enumerate(T.SWB_CASES):
        dy, wdT, gu = _swb_inputs(k, False)
        g, u = gu[:, :I], gu[:, I:]
        pc = T.probe_channels(I, DEV)
        dact = ops.gemm(dy, wdT, variant=11)
        ref = T.dact64(dy, wdT)[:, pc]
        dgu_c, act_c = ops.swiglu_bwd(gu.contiguous(), dact, I)
        chain = (dgu_c, act_c.t(), torch.cat([dgu_c[:, :I].t(), dgu_c[:, I:].t()]))
        runs = _swb_runs(ops, L, k, dy, wdT, gu)
        for r, outs in enumerate(runs):
            dgu, actT, dguT = outs
            what = f"random case {k + 1} call {r}"
            _bits_eq(dgu[:, I:][:, pc], dact[:, pc], f"{what}: probe channels, dgu up half vs gemm variant 11")
            T.within(dgu[:, I:][:, pc], ref, 2.0 ** -8 * ref.abs() + 4 * K * 2.0 ** -24, f"{what}: probe channels vs fp64 product")
            _bits_eq(actT[pc], u[:, pc].t(), f"{what}: probe channels, actT vs u")
            _bits_eq(dguT[:I], dgu[:, :I].t(), f"{what}: dguT gate half vs dgu")
            _bits_eq(dguT[I:], dgu[:, I:].t(), f"{what}: dguT up half vs dgu")
            for name, got, want in zip(("dgu", "actT", "dguT"), outs, chain):
                assert got.shape == want.shape, (what, name)
                d = (got.float() - want.float()).abs()
                ndiff = int((H.bits(got) != H.bits(want)).sum())
                if r == 0:
                    pooled[name][0] += ndiff
                    pooled[name][1] += got.numel()
                if ndiff:
                    rel = float((d / want.float().abs().clamp_min(1e-6)).max())
                    print(f"[fused vs chain] {what} {name}: {ndiff}/{got.numel()} differ, max relative {rel:.3g}")
                    assert rel <= 2.0 ** -7, (what, name, rel)
        for a, b, name in zip(runs[0], runs[1], ("dgu", "actT", "dguT")):
            _bits_eq(b, a, f"random case {k + 1}: second call, {name}")
    for name, (nd, nt) in pooled.items():
        print(f"[fused vs chain] {name}: {nd}/{nt} elements differ over the eight cases")
        assert nd < 1e-3 * nt, (name, nd, nt)


def test_gemm_swiglu_bwd_refusals_touch_nothing(L):
    """I = 96, M = 12, K = 64, K = 192: MM355_EUNSUPPORTED; ldT = M - 8, ldT = M + 4, dguT 8 bytes past a 16-byte boundary: MM355_EINVAL.
    Return code only, the three outputs all sentinel afterwards."""
    M, I, K = 64, 128, 256
    dy, wdT = T.swb_operands(M, I, K, 1, False, DEV)
    gu = T.swb_gu(M, I, 2 * I, 2, DEV)
    s = T.SENTINELS[0]
    fd, fa, ft = T.framed((M, 2 * I), 2 * I, s, DEV), T.framed((I, M + 8), M + 8, s, DEV), T.framed((2 * I, M + 8), M + 8, s, DEV)
    call = lambda m, i, kk, **kw: _swb_call(L, dy, wdT, gu, fd, fa, ft, m, i, kk, **kw)  # noqa: E731
    assert call(M, 96, K, ldT=M) == EUNSUPPORTED
    assert call(12, I, K, ldT=16) == EUNSUPPORTED
    assert call(M, I, 64, ldT=M) == EUNSUPPORTED
    assert call(M, I, 192, ldT=M) == EUNSUPPORTED
    assert call(M, I, K, ldT=M - 8) == EINVAL
    assert call(M, I, K, ldT=M + 4) == EINVAL
    assert call(M, I, K, ldT=M, dguT_ptr=ft.view.data_ptr() + 8) == EINVAL
    torch.cuda.synchronize()
    for f in (fd, fa, ft):
        f.check_all_sentinel("gemm_swiglu_bwd refusals")
    assert call(M, I, K) == 0                                                             # the same buffers are taken once the arguments are right
    torch.cuda.synchronize()
    for f in (fd, fa, ft):
        f.check_untouched("gemm_swiglu_bwd after refusals")
    assert not bool((H.bits(ft.view[:, :M]) == s).all())
