"""The kernels under the trainable SigLIP tower (LayerNorm forward / backward, column sums, bilinear token reduction + L2 norm) against the
fp64 references of tests/tower_refs.py, in every class their launches have.  Needs an MI355X:  pytest -m gpu

Classes (csrc/rowwise.hip, csrc/gemm_bf16.hip), each named in a test id:
  * row kernels keep VPT = 1 / 2 / 4 / 8 vectors of 8 columns per thread (dispatch_vpt: h <= 2048 / 4096 / 8192 / 16384), refuse wider rows;
  * layernorm_bwd_kernel walks rpb = 1 / 8 / 32 rows per workgroup (M < 1024 / < 8192 / >= 8192);
  * column sums: colsum_kernel (4 row phases; M < 256 or unaligned) and colsum8_kernel (128 row phases, 16-byte loads);
  * the bilinear kernels run one wave per output token, four per workgroup, C / 8 vectors over 64 lanes.

Bounds are derived from operation counts and number formats (U = 2^-24 is the unit roundoff of one fp32 operation; "one bf16
rounding" is half a bf16 step at the reference value, between 2^-9 and 2^-8 relative), never from what the kernels return; every test
prints the largest error / bound ratio it saw.
"""
import ctypes
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tower_refs as T  # noqa: E402

DEV = "cuda"
U = T.U
EPS = 1e-6


@pytest.fixture(scope="module")
def ops():
    from metamorph_amd import ops as _ops
    from metamorph_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _ops


def _lib():
    from metamorph_amd import lib
    return lib.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def vpt_of(h):
    nv = h // 8
    return 1 if nv <= 256 else 2 if nv <= 512 else 4 if nv <= 1024 else 8


def rpb_of(M):
    return 32 if M >= 8192 else 8 if M >= 1024 else 1


def _rows(kind, M, h, seed):
    return T.siglip_like_rows(M, h, seed)[0] if kind == "siglip" else T.hostile_rows(kind, M, h)


def _worst(err, tol):
    """largest err / tol and where; an element with tol == 0 must have err == 0"""
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), i


def _chain_constants(h):
    """c_sum: a block sum of h values is 8 VPT adds per thread, 6 wave-shuffle levels, 3 adds over the four waves, one division, one
    spare = 8 VPT + 11 rounded operations, so it is off by <= c_sum U sum |addend|.
    c_hat: xhat = (x - mean) rstd carries, relative to itself, the subtraction (1), rstd = rsqrtf(ss / h + eps): half of [squares (2),
    the sum's chain (c_sum), + eps (1)] plus rsqrtf's own ulp (2), the product (1), and for the results built on it one more
    multiplication and one addition (2):  c_hat = 4 VPT + 16 >= 1 + (2 + 8 VPT + 11 + 1) / 2 + 2 + 1 + 2."""
    v = vpt_of(h)
    return 8 * v + 11, 4 * v + 16


# ------------------------------------------------------------------------------------------------ LayerNorm forward

LN_WIDTHS = [8, 1152, 2048, 2056, 4096, 4104, 8192, 8200, 16384]


@pytest.mark.parametrize("kind", ("siglip",) + T.HOSTILE_KINDS)
@pytest.mark.parametrize("M", [1, 50])
@pytest.mark.parametrize("h", LN_WIDTHS, ids=lambda h: f"h{h}-vpt{vpt_of(h)}")
def test_layernorm_fwd_against_fp64(ops, h, M, kind):
    """mm355_layernorm_fwd per element against fp64:  |y - ref| <= 0.5 step_bf16(ref)                    (the one rounding of the store)
                                                               + (c_hat U + s^2 / 2) (|xhat w| + |b|)      (fp32 chain)
                                                               + s |w|                                     (the mean's own error)
    with c_sum = 8 VPT + 11 and c_hat = 4 VPT + 16 (see _chain_constants) and s = c_sum U mean|x| rstd: the fp32 mean is off by
    <= c_sum U mean|x|, which moves every xhat of the row by s and (through the variance, + delta^2) rstd by s^2 / 2 relative.
    Rows of equal elements: sums of <= 16384 equal 8-bit significands are exact in fp32, so xhat = 0 exactly and y must be b bit for bit."""
    x, (w, b) = _rows(kind, M, h, seed=h + M), T.norm_params(h, seed=h)
    ref, xh, rstd = T.layernorm_ref(x, w, b, EPS)
    c_sum, c_hat = _chain_constants(h)
    s = c_sum * U * x.double().abs().mean(-1, keepdim=True) * rstd
    tol = 0.5 * T.bf16_step(ref) + (c_hat * U + 0.5 * s * s) * ((xh * w.double()).abs() + b.double().abs()) + s * w.double().abs()
    y = ops.layernorm_fwd(x.to(DEV), w.to(DEV), b.to(DEV), EPS)
    torch.cuda.synchronize()
    got = y.double().cpu()
    assert bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    worst, i = _worst(err, tol)
    print(f"\n   layernorm_fwd h={h} VPT={vpt_of(h)} M={M} {kind}: max |err| {float(err.max()):.3e}, max err/bound {worst:.3f}")
    assert worst <= 1.0, (h, M, kind, i, float(err.flatten()[i]), float(tol.flatten()[i]))
    if kind in ("constant", "zero"):
        assert torch.equal(y.cpu(), b.expand(M, h)), (h, M, kind)


@pytest.mark.parametrize("h,code", [(16392, -2), (1150, -1)], ids=["h16392-wider-than-vpt8", "h1150-not-a-multiple-of-8"])
def test_layernorm_fwd_refuses_rows_it_cannot_hold(ops, h, code):
    """h > 16384 (more than 8 vectors per thread) is MM355_EUNSUPPORTED and h % 8 != 0 MM355_EINVAL; the output buffer is not touched"""
    from metamorph_amd.lib import Mm355Error
    x, w = T.siglip_like_rows(2, h, seed=1)[0].to(DEV), torch.ones(h, dtype=T.BF16, device=DEV)
    out = torch.full((2, h), -7.5, dtype=T.BF16, device=DEV)
    with pytest.raises(Mm355Error, match=rf"\({code}\)$"):
        ops.layernorm_fwd(x, w, w, EPS, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.5).all())


# ------------------------------------------------------------------------------------------------ LayerNorm backward

LN_BWD_SHAPES = [(M, 1152) for M in (1, 1023, 1024, 1025, 1458, 8191, 8193)] + [(37, h) for h in (8, 2056, 4104, 8200, 16384)]


@pytest.mark.parametrize("kind", ["siglip", "offset", "constant"])
@pytest.mark.parametrize("shape", LN_BWD_SHAPES, ids=lambda s: f"M{s[0]}-rpb{rpb_of(s[0])}-h{s[1]}-vpt{vpt_of(s[1])}")
def test_layernorm_bwd_against_fp64(ops, shape, kind):
    """mm355_layernorm_bwd in every rows-per-workgroup class (edges at M = 1024 and 8192, ragged last workgroups, the tower's M = 1458)
    and every VPT class, with dres and without, dw / db accumulated onto non-zero values.

    dx per element, with g = dy w, SG = mean|g|, SGX = mean|g xhat|, and c_sum, c_hat, s as in the forward test:
        |dx - ref| <= 0.5 step_bf16(ref) + U |dres|
                      + (c_sum + 2 c_hat + 6) U rstd (|g| + SG + |xhat| SGX)      (the two row sums, xhat and rstd, the final chain)
                      + s rstd (SGX + |xhat| SG)                                  (xhat moved by the mean's error, in mean(g xhat) and in xhat mean(g xhat))
    dw, db per column, the bound form of test_rmsnorm_bwd_rows_per_block_classes: rpb adds in registers, then G partials in a fixed
    tree, then the start value -- at most rpb + G + 34 rounded adds of <= U of the running absolute sum:
        |dw - ref| <= (rpb + G + 34) U (sum_r |dy xhat| + |start|) + sum_r |dy| (c_hat U |xhat| + s_r)      (xhat's own fp32 error)
        |db - ref| <= (rpb + G + 34) U (sum_r |dy| + |start|)
    rpb and G are read back through mm355_layernorm_bwd_ws_floats (G 2 h floats).  A second launch (through ctypes, on a workspace of
    exactly that many floats followed by a poisoned tail) must give the same bits and leave the tail alone.  dx starts as NaN: a row
    the launch skips stays NaN."""
    M, h = shape
    L = _lib()
    x, (w, _) = _rows(kind, M, h, seed=M + h), T.norm_params(h, seed=h + 1)
    dy = T.grad_rows_along(x, seed=M + h + 1)
    dres = T.rows_with_column_mean(M, h, seed=M + h + 2)
    g0 = torch.Generator().manual_seed(M + h + 3)
    dw0, db0 = torch.randn(h, generator=g0) * 3.0 + 0.25, torch.randn(h, generator=g0) * 3.0 - 0.5
    rpb = rpb_of(M)
    n_ws = int(L.mm355_layernorm_bwd_ws_floats(M, h))
    G = n_ws // (2 * h)
    assert n_ws == G * 2 * h and G == -(-M // rpb), (M, h, n_ws, rpb)

    dx_ref, dw_ref, db_ref, dw_abs, db_abs = T.layernorm_bwd_ref(dy, x, w, EPS, None)
    _, xh, rstd = T.layernorm_ref(x, w, torch.zeros_like(w), EPS)
    c_sum, c_hat = _chain_constants(h)
    s = c_sum * U * x.double().abs().mean(-1, keepdim=True) * rstd
    g = (dy.double() * w.double()).abs()
    SG, SGX = g.mean(-1, keepdim=True), (g * xh.abs()).mean(-1, keepdim=True)
    chain = (c_sum + 2 * c_hat + 6) * U * rstd * (g + SG + xh.abs() * SGX) + s * rstd * (SGX + xh.abs() * SG)
    n_add = rpb + G + 34
    tol_dw = n_add * U * (dw_abs + dw0.double().abs()) + (dy.double().abs() * (c_hat * U * xh.abs() + s)).sum(0)
    tol_db = n_add * U * (db_abs + db0.double().abs())

    xd, dyd, wd = x.to(DEV), dy.to(DEV), w.to(DEV)
    for with_dres in (True, False):
        dresd = dres.to(DEV) if with_dres else None
        ref = dx_ref + dres.double() if with_dres else dx_ref
        tol_dx = 0.5 * T.bf16_step(ref) + (U * dres.double().abs() if with_dres else 0) + chain
        dw, db = dw0.to(DEV), db0.to(DEV)
        dx = torch.full((M, h), float("nan"), dtype=T.BF16, device=DEV)
        ops.layernorm_bwd(dyd, xd, wd, EPS, dw, db, dres=dresd, dx=dx)
        torch.cuda.synchronize()
        worst = {}
        for name, got, want, tol in (("dx", dx, ref, tol_dx), ("dw", dw, dw_ref + dw0.double(), tol_dw), ("db", db, db_ref + db0.double(), tol_db)):
            got = got.double().cpu()
            assert bool(torch.isfinite(got).all()), (name, M, h, kind, with_dres, int((~torch.isfinite(got)).sum()))
            err = (got - want).abs()
            worst[name], i = _worst(err, tol)
            assert worst[name] <= 1.0, (name, M, h, kind, with_dres, i, float(err.flatten()[i]), float(tol.flatten()[i]), float(want.flatten()[i]))
        print(f"\n   layernorm_bwd M={M} rpb={rpb} G={G} h={h} VPT={vpt_of(h)} {kind} dres={with_dres}: max err/bound "
              f"dx {worst['dx']:.3f} dw {worst['dw']:.3f} db {worst['db']:.3f}")
        # second launch: same bits, workspace of exactly n_ws floats, tail untouched
        tail = 4096
        ws = torch.full((n_ws + tail,), 1234.5, device=DEV)
        dw2, db2 = dw0.to(DEV), db0.to(DEV)
        dx2 = torch.full((M, h), float("nan"), dtype=T.BF16, device=DEV)
        rc = L.mm355_layernorm_bwd(dyd.data_ptr(), xd.data_ptr(), wd.data_ptr(), dresd.data_ptr() if with_dres else None, dx2.data_ptr(),
                                   dw2.data_ptr(), db2.data_ptr(), ws.data_ptr(), M, h, EPS, _stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert bool((ws[n_ws:] == 1234.5).all()), (M, h, "workspace written past mm355_layernorm_bwd_ws_floats")
        assert torch.equal(dx2.view(torch.int16), dx.view(torch.int16)) and torch.equal(dw2, dw) and torch.equal(db2, db), (M, h, kind, with_dres)


# ------------------------------------------------------------------------------------------------ column sums

P_TOK, HV, IV = 729, 1152, 4304
COLSUM_CASES = [  # id, kernel, M, N, how the operand is cut from its buffer
    ("colsum8-fc1-bias-1458x4304", 8, 2 * P_TOK, IV, "plain"),
    ("colsum8-bias-1458x1152", 8, 2 * P_TOK, HV, "plain"),
    ("colsum8-dqkv-block0-1458x1152-of-3456", 8, 2 * P_TOK, HV, 0),
    ("colsum8-dqkv-block1-1458x1152-of-3456", 8, 2 * P_TOK, HV, 1),
    ("colsum8-dqkv-block2-1458x1152-of-3456", 8, 2 * P_TOK, HV, 2),
    ("colsum-M255-below-the-switch", 1, 255, HV, "plain"),
    ("colsum8-M256-at-the-switch", 8, 256, HV, "plain"),
    ("colsum-pos-embed-3x839808", 1, 3, P_TOK * HV, "plain"),
    ("colsum-pos-embed-2x839808-view-of-1458x1152", 1, 2, P_TOK * HV, "view"),
]


@pytest.mark.parametrize("case", COLSUM_CASES, ids=lambda c: c[0])
def test_colsum_at_the_tower_shapes(ops, case):
    """mm355_colsum_bf16 (bias gradients of the tower's Linears, of the patch embedding, and the position-table gradient) per column
    against fp64, accumulated onto a non-zero `out`, inputs with a non-zero column mean:
        |out - ref| <= (n + 8) U (sum_r |x| + |start|),   n = the longest chain of adds one output goes through:
        colsum8_kernel: ceil(M / 128) per thread, 128 phases, the accumulate;   colsum_kernel: ceil(M / 4) per thread, 3, the accumulate.
    Which kernel runs follows mm355_colsum_bf16's rule (N % 8 == 0, ld % 8 == 0, 16-byte aligned, M >= 256), restated here per case.
    A second launch gives the same bits."""
    name, kernel, M, N, cut = case
    if cut == "plain":
        xh = T.rows_with_column_mean(M, N, seed=M + N)
        xd = xh.to(DEV)
        ld = N
    elif cut == "view":
        xh = T.rows_with_column_mean(M * P_TOK, HV, seed=M + N).view(M, N)
        xd = xh.view(M * P_TOK, HV).to(DEV).view(M, N)
        ld = N
    else:
        buf = T.rows_with_column_mean(M, 3 * N, seed=M + N)
        xh = buf[:, cut * N:(cut + 1) * N]
        xd = buf.to(DEV)[:, cut * N:(cut + 1) * N]
        ld = 3 * N
    takes8 = N % 8 == 0 and ld % 8 == 0 and xd.data_ptr() % 16 == 0 and M >= 256
    assert takes8 == (kernel == 8), (name, "the case does not reach the kernel its id names")
    n = (-(-M // 128) + 128 + 1) if kernel == 8 else (-(-M // 4) + 3 + 1)
    start = torch.linspace(-1.0, 1.0, N) + 0.5
    x64 = xh.double()
    want = x64.sum(0) + start.double()
    tol = (n + 8) * U * (x64.abs().sum(0) + start.double().abs())
    assert float(x64.mean(0).abs().mean()) > 0.5                # the column means are not noise
    outs = []
    for _ in range(2):
        out = start.to(DEV)
        ops.colsum_f32(xd, out)
        torch.cuda.synchronize()
        outs.append(out.cpu())
    err = (outs[0].double() - want).abs()
    worst, i = _worst(err, tol)
    print(f"\n   {name}: chain {n}, max |err| {float(err.max()):.3e}, max err/bound {worst:.3f}")
    assert worst <= 1.0, (name, i, float(err[i]), float(tol[i]), float(want[i]))
    assert torch.equal(outs[0], outs[1]), name


# ------------------------------------------------------------------------------------------------ bilinear reduction + L2 norm

BIL_SIDES = [(27, 1), (27, 2), (27, 4), (27, 8), (27, 12), (27, 16), (27, 27), (4, 2)]


@pytest.mark.parametrize("normalize", [True, False], ids=["l2norm", "plain"])
@pytest.mark.parametrize("N", [1, 3], ids=["N1", "N3-one-zero-image"])
@pytest.mark.parametrize("C", [8, 64, 1152, 1160])
@pytest.mark.parametrize("sides", BIL_SIDES, ids=lambda s: f"{s[0]}to{s[1]}-{s[1] * s[1]}tok")
def test_bilinear_l2norm_fwd_bwd_against_fp64(ops, sides, C, N, normalize):
    """mm355_bilinear_l2norm and mm355_bilinear_l2norm_bwd for every token count a 27-side grid is reduced to (1 .. 729; with N = 1 or 3
    the counts 1, 3, 729, 2187 are no multiple of a workgroup's four waves), C of 1 vector, 8, 144 and 145 vectors (the last two leave the
    64-lane loop ragged), one all-zero image when N = 3 (the 1e-12 norm clamp: forward 0, backward dy 1e12).

    forward: at most one bf16 step from tower_refs.bilinear_l2norm_ref, which rounds where the kernel rounds.
    backward (fp32 sums of atomics, read before any cast to bf16), per source element:
        |din - ref| <= (addends + 8) U sum |addend| + extra
    addends / sum |addend| / extra as tower_refs.bilinear_l2norm_bwd_ref documents them (the magnitudes are taken before dy cancels
    against its projection; `extra` is the fp32 chain of r . dy and sum r^2 and a bf16 norm or row element on a rounding boundary).
    With l2norm a second gradient, dy = 3 y, is parallel to the output: the exact gradient is a cancellation residue and the same
    absolute bound must hold."""
    si, so = sides
    L = _lib()
    g = torch.Generator().manual_seed(si * 1000 + so * 10 + C + N)
    x = T.to_bf16(torch.randn(N, si * si, C, generator=g) + 0.25)
    if N == 3:
        x[1] = 0
    dy = T.to_bf16(torch.randn(N, so * so, C, generator=g) + 0.1)
    y_ref, _, _ = T.bilinear_l2norm_ref(x, si, so, normalize)
    xd = x.to(DEV)
    y = ops.bilinear_l2norm(xd, si, so, normalize)
    torch.cuda.synchronize()
    got, want = y.double().cpu(), T.to_bf16(y_ref).double()
    steps = (got - want).abs() / T.bf16_step(torch.maximum(got.abs(), want.abs()))
    print(f"\n   bilinear {si}->{so} C={C} N={N} normalize={normalize}: forward {float((steps > 0).double().mean()):.2e} of the elements one step off, "
          f"max {float(steps.max()):.2f} steps")
    assert bool(torch.isfinite(got).all()) and float(steps.max()) <= 1.0 + 1e-9
    if N == 3:
        assert float(got[1].abs().max()) == 0.0
    grads = [("random", dy)] + ([("parallel", T.to_bf16(3.0 * y_ref))] if normalize else [])
    for what, gy in grads:
        ref = T.bilinear_l2norm_bwd_ref(x, gy, si, so, normalize)
        tol = (ref["count"][None, :, None] + 8) * U * ref["abs_sum"] + ref["extra"]
        acc = torch.zeros((N, si * si, C), device=DEV)
        rc = L.mm355_bilinear_l2norm_bwd(xd.data_ptr(), gy.to(DEV).data_ptr(), acc.data_ptr(), N, si, so, C, int(normalize), _stream())
        torch.cuda.synchronize()
        assert rc == 0
        din = acc.double().cpu()
        assert bool(torch.isfinite(din).all())
        err = (din - ref["din"]).abs()
        worst, i = _worst(err, tol)
        print(f"   bilinear bwd {si}->{so} C={C} N={N} normalize={normalize} dy={what}: max err/bound {worst:.3f}, "
              f"max |ref| / sum|addend| {float((ref['din'].abs() / ref['abs_sum'].clamp_min(1e-300)).max()):.2e}")
        assert worst <= 1.0, (what, sides, C, N, normalize, i, float(err.flatten()[i]), float(tol.flatten()[i]), float(ref["din"].flatten()[i]))
        if what == "parallel":                                  # the gradient really is a cancellation: far below its addends
            live = ref["abs_sum"][0] > 0
            assert float((ref["din"][0][live].abs() / ref["abs_sum"][0][live]).max()) <= 2.0 ** -5
        if N == 3 and normalize and what == "random":           # clamp path: dy / 1e-12 through the corner weights
            lin = T.bilinear_l2norm_bwd_ref(x[1:2], gy[1:2], si, so, False)
            assert bool(((din[1] - lin["din"][0] * 1e12).abs() <= (ref["count"][:, None] + 8) * U * lin["abs_sum"][0] * 1e12).all())
