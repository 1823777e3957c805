"""The step's helper kernels (csrc/elementwise.hip, csrc/losses.hip, ce_rows / cosine_loss of csrc/rowwise.hip) against the fp64 references
of tests/helper_refs.py: the whole bf16 domain of the activation functions, every grid-stride loop past one grid pass (grid_for caps the
grid at 4096 workgroups of 256 threads: a second pass starts above 1 048 576 work items) with a ragged last pass, the row-per-wave kernels
across widths, row counts and views, every output of AdamW, im2col on images that are neither square nor multiples of the patch.
Needs an MI355X:  pytest -m gpu

Every bound is a derivation (written beside it) or a fixed multiple of a figure measured on the reference stack by
tests/test_helper_refs_host.py (helper_refs.STACK_*); none is fitted to what a kernel returned.  The large references are evaluated by
torch in fp64 on the device (plain torch, not this library) to keep each case at a few seconds.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helper_refs as H  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
CAP = 4096 * 256                     # work items of one grid pass
KC = H.KERNEL_C_FACTOR


@pytest.fixture(scope="module")
def ops():
    from metamorph_amd import ops as _ops
    from metamorph_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _ops


def rnd(*shape, seed=0, scale=1.0, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=device) * scale).to(BF16)


def bf(v):
    return torch.tensor(v, dtype=BF16)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def within(got, ref, bound, what):
    got, ref = got.to(H.F64), ref.to(H.F64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= bound)                                       # a NaN anywhere is bad
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        b = bound if bound.dim() == 0 else bound.expand_as(err)[i]
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} outside the bound; first at {i}: got {float(got[i]):.9g} "
                             f"ref {float(ref[i]):.9g} bound {float(b):.3g}")


# ================================================================================================ 1. the whole bf16 domain

DY = [1.0, -1.0, 0.37, 2.0 ** -20, 2.0 ** 20]
UVALS = [1.0, -1.0, 0.37, 0.0, -0.0, 3.0 * 2 ** 10]
DAVALS = [1.0, -0.5, 0.0]


def _domain_check(name, got, ref, x, factor, steps, stack, scales_with_x):
    """got / stack: bf16 results of the kernel / of the reference stack; ref: fp64; x: the bf16 input the function is unary in; factor: dy, u
    or dact * u.  The masks come from the input and the stack alone."""
    got, stack = got.cpu(), stack.cpu()
    finite_in = torch.isfinite(x.float())
    sub = H.subnormal(x)
    excluded = finite_in & ~torch.isfinite(stack.float())
    assert int(excluded.sum()) == H.STACK_EXCLUDED[name], (name, int(excluded.sum()))
    held = finite_in & ~excluded & ~sub
    factor = torch.as_tensor(factor, dtype=H.F64).expand_as(ref)
    c = KC * H.STACK_C[name]
    bound = H.act_bound(ref, x, factor, c, steps)
    meas = H.smallest_c(got, ref, x, factor, steps, held)
    print(f"[domain] {name}: kernel needs c = {meas:.4g}, allowed {c:.4g} (stack {H.STACK_C[name]:.4g}), {int(held.sum())} elements held")
    g, r, b = got.double()[held], ref[held], bound[held]
    within(g, r, b, name)
    # subnormal inputs (254 patterns per factor): finite; a result proportional to x stays below 2^-126 |factor|; a gradient with respect to
    # x is continuous there (gelu'(0) = silu'(0) = 0.5), so it is held to the ordinary bound
    assert bool(torch.isfinite(got.float()[sub]).all()), name
    if scales_with_x:
        assert bool((got.double()[sub].abs() <= H.TINY * factor[sub].abs()).all()), name
    else:
        within(got.double()[sub], ref[sub], bound[sub], name + " (subnormal x)")


@pytest.mark.parametrize("kind", [H.GELU_ERF, H.GELU_TANH])
def test_gelu_over_all_bf16_inputs(ops, kind):
    """gelu_fwd and gelu_bwd on all 65 536 bf16 patterns against fp64 (erf: 0.5 x erfc(-x / sqrt 2); tanh: x sigmoid(2u), the tanh formula
    without its cancellation), |got - ref| <= 2^-8 |ref| + c 2^-24 max(|x|, 1) |dy| (+ 2^-126 for subnormal results), every element.
    c = 4 x the smallest c the reference stack (torch CPU, fp32 math -> bf16) needs: stack 0.7905 / 0.4942 (forward erf / tanh) and
    0.06128 / 3.403 (gradient erf / tanh), so the kernels get 3.162 / 1.977 / 0.2451 / 13.61.
    Known properties, excluded because the stack's own result is not finite at a finite input: erf forward on the top 128 patterns
    (x (1 + erf) overflows), tanh gradient for |x| >= 2^64 (16 384 patterns: x^3 overflows, 0 * inf).  Nothing else is excluded."""
    tag = "erf" if kind == H.GELU_ERF else "tanh"
    x = H.all_bf16()
    xd = x.to(DEV)
    _domain_check(f"gelu_fwd_{tag}", ops.gelu_fwd(xd, kind), H.gelu64(x, kind), x, 1.0, 1, H.stack_gelu_fwd(x, kind), True)
    grad = H.gelu_grad64(x, kind)
    for dy in DY:
        dyb = bf(dy)
        got = ops.gelu_bwd(xd, dyb.expand(65536).contiguous().to(DEV), kind)
        _domain_check(f"gelu_bwd_{tag}", got, float(dyb) * grad, x, float(dyb), 1, H.stack_gelu_bwd(x, dyb, kind), False)


def test_swiglu_over_all_bf16_gates(ops):
    """swiglu_fwd / swiglu_bwd with the gate over all 65 536 patterns against every up value in {1, -1, 0.37, 0, -0, 3 * 2^10} (and dact in
    {1, -0.5, 0}), gu laid out as rows of I = 512.  Reference: silu in fp64 -> bf16, times u (act), dact times the bf16 silu (dup), the
    fp64 derivative (dgate).  act and dup carry two bf16 roundings (a flip of the inner one moves the product by a step, the outer adds
    half a step): 2 * 2^-8 |ref|; dgate one.  The c term only matters on the tail g <= -89 where exp(-g) overflows fp32 and silu comes out
    0 instead of ~1e-37: stack c = 3.72e-32 (act, dup) and 3.69e-32 (dgate), kernels 4x.  Excluded: the 1 493 products with u = 3 * 2^10
    that overflow bf16 on the stack."""
    gu, _ = H.swiglu_domain(UVALS)
    g, u = gu[:, :512].reshape(-1), gu[:, 512:].reshape(-1)
    act = ops.swiglu_fwd(gu.to(DEV), 512).reshape(-1)
    _domain_check("swiglu_fwd", act, H.swiglu_fwd64(g, u), g, u.double(), 2, H.stack_swiglu_fwd(g, u), True)
    gu, da = H.swiglu_domain(UVALS, DAVALS)
    g, u, d = gu[:, :512].reshape(-1), gu[:, 512:].reshape(-1), da.reshape(-1)
    dgu, act2 = ops.swiglu_bwd(gu.to(DEV), da.to(DEV), 512)
    rg, ru = H.swiglu_bwd64(g, u, d)
    sg, su = H.stack_swiglu_bwd(g, u, d)
    _domain_check("swiglu_dgate", dgu[:, :512].reshape(-1), rg, g, u.double() * d.double(), 1, sg, False)
    _domain_check("swiglu_dup", dgu[:, 512:].reshape(-1), ru, g, d.double(), 2, su, True)
    # the recomputed act against the forward's over the WHOLE gate domain (silu depends on the gate alone): bit for bit, a NaN for a NaN
    a2 = act2.reshape(-1)[:65536 * len(UVALS)]
    assert bool(((H.bits(a2) == H.bits(act)) | (torch.isnan(a2) & torch.isnan(act))).all())
    _domain_check("swiglu_fwd", act2.reshape(-1)[:65536 * len(UVALS)], H.swiglu_fwd64(g, u)[:65536 * len(UVALS)], g[:65536 * len(UVALS)],
                  u.double()[:65536 * len(UVALS)], 2, H.stack_swiglu_fwd(g, u)[:65536 * len(UVALS)], True)


@pytest.mark.parametrize("fn", ["gelu_fwd_erf", "gelu_fwd_tanh", "gelu_bwd_erf", "gelu_bwd_tanh", "swiglu_fwd", "swiglu_bwd"])
def test_activations_on_non_finite_inputs(ops, fn):
    """+-inf and the 254 NaN patterns: the result is of the same class (NaN, +inf, -inf, zero, finite) as torch's CPU result (fp32 math,
    torch.nn.functional.gelu / silu as in helper_refs.stack_*).
    One known property, pinned: the erf GELU forward at x = +inf is +inf, the limit of the function.  torch's vectorised fp32 CPU
    kernel returns NaN there while its one-element fp32 call and its fp64 call return +inf (shown by
    test_helper_refs_host.test_non_finite_inputs_have_a_class_on_the_stack), so torch's CPU result has no single class at that input.
    torch's class holds everywhere else."""
    x = H.all_bf16()
    nf = ~torch.isfinite(x.float())
    xs = x[nf]
    n = xs.numel()                                              # 256 = 32 vectors
    if fn.startswith("gelu"):
        kind = H.GELU_ERF if fn.endswith("erf") else H.GELU_TANH
        if "fwd" in fn:
            stack = H.stack_gelu_fwd(xs, kind)
            if kind == H.GELU_ERF:
                stack[H.bits(xs) == 0x7F80] = float("inf")
            pairs = [(ops.gelu_fwd(xs.to(DEV), kind), stack, "fwd")]
        else:
            pairs = [(ops.gelu_bwd(xs.to(DEV), bf(dy).expand(n).contiguous().to(DEV), kind), H.stack_gelu_bwd(xs, bf(dy), kind), dy) for dy in DY]
    else:
        pairs = []
        for u in UVALS:
            gu = torch.cat([xs, bf(u).expand(n)]).view(1, 2 * n).contiguous()
            if fn == "swiglu_fwd":
                pairs.append((ops.swiglu_fwd(gu.to(DEV), n).reshape(-1), H.stack_swiglu_fwd(xs, bf(u).expand(n)), u))
            else:
                for da in DAVALS:
                    dgu, _ = ops.swiglu_bwd(gu.to(DEV), bf(da).expand(1, n).contiguous().to(DEV), n)
                    sg, su = H.stack_swiglu_bwd(xs, bf(u).expand(n), bf(da).expand(n))
                    pairs += [(dgu[0, :n], sg, (u, da, "dgate")), (dgu[0, n:], su, (u, da, "dup"))]
    for got, stack, what in pairs:
        a, b = H.classes(got.cpu()), H.classes(stack)
        bad = (a != b).nonzero().reshape(-1).tolist()
        assert not bad, (fn, what, [(hex(int(H.bits(xs)[i])), int(a[i]), int(b[i])) for i in bad[:4]], len(bad))


# ================================================================================================ 2. past one grid pass

def _swiglu_case(ops, M, I, seed):
    gu = rnd(M, 2 * I, seed=seed, scale=1.5, device=DEV)
    da = rnd(M, I, seed=seed + 1, device=DEV)
    g, u = gu[:, :I], gu[:, I:]
    cf, cg, cu = (KC * H.STACK_C[k] for k in ("swiglu_fwd", "swiglu_dgate", "swiglu_dup"))
    ref_act = H.swiglu_fwd64(g, u)
    act = ops.swiglu_fwd(gu, I)
    within(act, ref_act, H.act_bound(ref_act, g, u.double(), cf, 2), f"swiglu_fwd {M}x{I}")
    assert same_bits(act, ops.swiglu_fwd(gu, I))
    rg, ru = H.swiglu_bwd64(g, u, da)
    dgu, act2 = ops.swiglu_bwd(gu, da, I)
    within(dgu[:, :I], rg, H.act_bound(rg, g, u.double() * da.double(), cg, 1), f"swiglu dgate {M}x{I}")
    within(dgu[:, I:], ru, H.act_bound(ru, g, da.double(), cu, 2), f"swiglu dup {M}x{I}")
    within(act2, ref_act, H.act_bound(ref_act, g, u.double(), cf, 2), f"swiglu_bwd act {M}x{I}")
    dgu_again, act_again = ops.swiglu_bwd(gu, da, I)
    assert same_bits(dgu_again, dgu) and same_bits(act_again, act2)
    dgu_alone, none = ops.swiglu_bwd(gu, da, I, want_act=False)
    assert none is None and same_bits(dgu_alone, dgu)


@pytest.mark.parametrize("M,I", [(650, 14336), (1100000, 8)])
def test_swiglu_past_one_grid_pass(ops, M, I):
    """1 164 800 vectors (650 x 14 336) and 1 100 000 one-vector rows: the second grid pass is partly empty.  Bounds as in section 1 (two
    bf16 steps for act and dup, one for dgate); forward, backward with and without act, each twice with identical bits."""
    assert M * (I // 8) > CAP
    _swiglu_case(ops, M, I, seed=M)


@pytest.mark.parametrize("kind", [H.GELU_ERF, H.GELU_TANH])
def test_gelu_past_one_grid_pass(ops, kind):
    n = 8 * 1049600
    tag = "erf" if kind == H.GELU_ERF else "tanh"
    x, dy = rnd(n, seed=3, scale=2.0, device=DEV), rnd(n, seed=4, device=DEV)
    ref = H.gelu64(x, kind)
    y = ops.gelu_fwd(x, kind)
    within(y, ref, H.act_bound(ref, x, 1.0, KC * H.STACK_C[f"gelu_fwd_{tag}"]), f"gelu_fwd {tag}")
    rg = dy.double() * H.gelu_grad64(x, kind)
    dx = ops.gelu_bwd(x, dy, kind)
    within(dx, rg, H.act_bound(rg, x, dy.double(), KC * H.STACK_C[f"gelu_bwd_{tag}"]), f"gelu_bwd {tag}")
    assert same_bits(y, ops.gelu_fwd(x, kind)) and same_bits(dx, ops.gelu_bwd(x, dy, kind))


@pytest.mark.parametrize("n", [8 * 1048576 + 8 * 777 + 5, 5, 8])
@pytest.mark.parametrize("with_dev", [True, False])
def test_scale_is_bit_exact(ops, n, with_dev):
    """x *= (s_dev ? *s_dev : 1) * s_host: two fp32 multiplications and one RNE, no contraction freedom -> the bits of the same two
    multiplications in torch fp32 on the CPU.  A view offset by one element is refused before anything is launched."""
    from metamorph_amd.lib import Mm355Error
    x = rnd(n, seed=n % 1000 + 1)
    s_dev, s_host = np.float32(0.37), np.float32(-1.7)
    s = (s_dev if with_dev else np.float32(1.0)) * s_host
    want = (x.float() * float(s)).bfloat16()
    sd = torch.tensor([float(s_dev)], device=DEV) if with_dev else None
    outs = [ops.scale_(x.to(DEV).clone(), sd, float(s_host)) for _ in range(2)]
    assert same_bits(outs[0].cpu(), want), int((outs[0].cpu().float() != want.float()).sum())
    assert same_bits(outs[0], outs[1])
    buf = torch.zeros(n + 9, device=DEV, dtype=BF16)
    with pytest.raises(Mm355Error):
        ops.scale_(buf[1:1 + n], sd, float(s_host))
    torch.cuda.synchronize()
    assert float(buf.float().abs().max()) == 0


@pytest.mark.parametrize("entry", ["bf16", "f32", "f32_dev"])
def test_axpy_past_one_grid_pass(ops, entry):
    """y (+)= s x at n = 2 * 1 048 576 + 3 with y a view offset by one element (scalar accesses: no alignment promised).
    |got - ref| <= 2^-8 |ref| + 2^-23 (|s x| + |y|): the product and the sum are one fp32 rounding each (2 * 2^-24 of their magnitudes),
    then RNE to bf16.  Without accumulate, y's previous contents (NaN here) do not matter.  s = s_dev * s_host is formed in fp32 as the
    kernel forms it."""
    n = 2 * CAP + 3
    ybuf = rnd(n + 2, seed=5, device=DEV)
    x = rnd(n, seed=6, device=DEV) if entry == "bf16" else torch.randn(n, generator=torch.Generator(device=DEV).manual_seed(7), device=DEV)
    s_dev, s_host = np.float32(0.37), np.float32(-2.5)
    use_dev = entry != "f32"
    s = float((s_dev if use_dev else np.float32(1.0)) * s_host)
    sd = torch.tensor([float(s_dev)], device=DEV) if use_dev else None
    for accumulate in (True, False):
        buf = ybuf.clone()
        if not accumulate:
            buf[1:1 + n] = float("nan")
        y0 = ybuf[1:1 + n].double() if accumulate else torch.zeros(n, dtype=H.F64, device=DEV)
        ref = s * x.double() + y0
        outs = []
        for _ in range(2):
            b = buf.clone()
            ops.axpy_(b[1:1 + n], x, sd, float(s_host), accumulate)
            outs.append(b)
        got = outs[0]
        within(got[1:1 + n], ref, H.BF_STEP * ref.abs() + 2.0 ** -23 * ((s * x.double()).abs() + y0.abs()), f"axpy {entry} acc={accumulate}")
        assert same_bits(got[:1], ybuf[:1]) and same_bits(got[n + 1:], ybuf[n + 1:])
        assert same_bits(outs[0], outs[1])


def test_cast_2d_past_one_grid_pass_in_column_blocks(ops):
    """4 100 x 2 056 (1 053 700 vectors), source and destination column blocks of wider buffers: the bits of .bfloat16() (ties, values
    that round up to inf, -0 included); the columns outside the block keep their bits."""
    Rr, C = 4100, 2056
    src = torch.randn(Rr, C + 8, generator=torch.Generator().manual_seed(8))
    src[0, 4:20] = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -23, 3.4e38, -3.4e38, -0.0, 0.0,
                                 float("inf"), -float("inf"), 65280.0, 65408.0, 1e-30, -1e-30, 0.1, 1.0 - 2.0 ** -9])
    dst = rnd(Rr, C + 16, seed=9).to(DEV)
    before = dst.clone()
    ops.cast_f32_to_bf16_2d(src.to(DEV)[:, 4:4 + C], dst[:, 8:8 + C])
    assert same_bits(dst[:, 8:8 + C].cpu(), src[:, 4:4 + C].bfloat16())
    assert same_bits(dst[:, :8], before[:, :8]) and same_bits(dst[:, 8 + C:], before[:, 8 + C:])
    again = before.clone()
    ops.cast_f32_to_bf16_2d(src.to(DEV)[:, 4:4 + C], again[:, 8:8 + C])
    assert same_bits(again, dst)


# ================================================================================================ 3. row-per-wave kernels

WIDTHS = [8, 64, 512, 520, 1152, 4096]          # narrower than one wave pass (512), exactly one, one vector past it, 2.25, eight
ROWS = [1, 5, 4099]                             # one wave of a workgroup, a partial last workgroup, many
GA = {k: H.KERNEL_GRAD_FACTOR * v for k, v in H.STACK_GRAD_DIST.items()}


def _unit_rows(Rr, C, seed):
    x = torch.randn(Rr, C, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV)
    return (x / x.norm(dim=-1, keepdim=True)).to(BF16)


def _settle_norms(p):
    """rebuild rows whose norm sits too close to a bf16 tie for an fp32 sum to decide (helper_refs.row_norm_near_tie)"""
    for _ in range(8):
        bad = H.row_norm_near_tie(p)
        if not bool(bad.any()):
            return p
        p[bad] = (p[bad].float() * 1.03).to(BF16)
    raise AssertionError("could not move the row norms off the bf16 ties")


def _row_max_bound(ref, a):
    return a * ref.abs().max(-1, keepdim=True).values + H.TINY


@pytest.mark.parametrize("Rr", ROWS)
@pytest.mark.parametrize("C", WIDTHS)
def test_softmax_rows_across_widths(ops, C, Rr):
    """softmax(round_bf(x / 0.07)) against fp64 on the same rounded logits: |got - ref| <= 2^-8 ref + 2^-126 (RNE to bf16 is 2^-9; exp's
    argument product and v_exp_f32 add |z - m| 2^-22 <= 7e-6 relative for |z| <= 14.3, the row sum (C / 64 + 6) 2^-24); every row sums to 1
    within C 2^-9.  Backward from the bf16 y of the reference: relative to the row's largest gradient, 2x the distance of the reference
    stack's bf16 evaluation from fp64 (0.00549 -> 0.01098; the existing case allows 5e-2 |ref| + 3e-2 max), plus y / 0.07 times the fp32
    error of the dot product.  Rows: unit vectors; one-hot after the temperature (1, -1, -1, ...); constant."""
    x = _unit_rows(Rr, C, seed=C + Rr)
    if Rr >= 5:
        x[0] = -1.0
        x[0, C // 2] = 1.0
        x[1] = 0.5
    ref = H.softmax_rows64(x)
    y = ops.softmax_rows(x, 0.07)
    within(y, ref, H.BF_STEP * ref + H.TINY, f"softmax_rows C={C} R={Rr}")
    assert bool(((y.double().sum(-1) - 1.0).abs() <= min(C * 2.0 ** -9, 2.0 ** -8)).all())     # (2^-8: the element bounds summed over a row)
    assert same_bits(y, ops.softmax_rows(x, 0.07))
    yb, dy = H.round_bf(ref).to(BF16), rnd(Rr, C, seed=C + Rr + 1, device=DEV)
    rb = H.softmax_rows_bwd64(yb, dy)
    dx = ops.softmax_rows_bwd(yb, dy, 0.07)
    # dy - dot cancels on a saturated row (y one-hot: dot = dy_k up to 1e-12); what survives is the fp32 error of dot, a sum of C products
    dot_err = (H.lane_adds(C, 2) + 7) * H.U24 * (yb.double() * dy.double()).abs().sum(-1, keepdim=True)
    bound = _row_max_bound(rb, min(3e-2, GA["softmax_bwd"])) + yb.double() * float(H.inv_temp_f32(0.07)) * dot_err
    within(dx, rb, bound, f"softmax_rows_bwd C={C} R={Rr}")
    assert same_bits(dx, ops.softmax_rows_bwd(yb, dy, 0.07))


@pytest.mark.parametrize("Rr", ROWS)
@pytest.mark.parametrize("C", WIDTHS)
def test_mean_abs_loss_across_widths(ops, C, Rr):
    """sum |round_bf(t - p)| against fp64 of the same rounded differences: (8 adds per vector a lane takes + 6 tree levels + the row sum's
    ceil(R / 1024) + 12) 2^-24 sum |terms|.  dpred = -sign(d) / (R C) within 2^-8 (one fp32 reciprocal, RNE), exactly zero on a row that
    equals its target.  Two calls, identical bits."""
    p, t = rnd(Rr, C, seed=C + Rr, device=DEV), rnd(Rr, C, seed=C + Rr + 7, device=DEV)
    if Rr >= 5:
        t[2] = p[2]
    s64, g64, a64 = H.mean_abs64(p, t)
    s, dp = ops.mean_abs_loss(p, t)
    bound = H.loss_bound(C, Rr, a64)
    print(f"[mean_abs] C={C} R={Rr} err {abs(float(s) - float(s64)):.3g} bound {bound:.3g}")
    assert abs(float(s) - float(s64)) <= bound, (float(s), float(s64), bound)
    within(dp, g64, H.BF_STEP * g64.abs(), f"mean_abs grad C={C} R={Rr}")
    if Rr >= 5:
        assert float(dp[2].float().abs().max()) == 0
    s2, dp2 = ops.mean_abs_loss(p, t)
    assert torch.equal(s, s2) and same_bits(dp, dp2)


@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("Rr", ROWS)
@pytest.mark.parametrize("C", WIDTHS)
def test_cosine_loss_across_widths(ops, C, Rr, normalize):
    """sum_r cos(t_r, u_r), u = F.normalize on bf16 (norm -> bf16, clamp, fp32 divide -> bf16) or the raw row, against fp64 through the same
    rounding points.  A row's cosine is tu / (nt nu): three fp32 sums of products (16 operations per vector a lane takes + 6 tree levels
    each; the two norms enter through a root, half each), two roots, a product, a quotient, two clamps -> (2 (16 v + 6) + 6) 2^-24 of
    sum |t u| / (nt nu), plus the row sum's adds.  Gradient relative to the row's largest: 2x the stack's distance (0.007305 normalised,
    0.007252 raw -> 0.01461 / 0.0145; existing 3e-2 |ref| + 2e-2 max).  Rows: N(0,1); all zero; constant."""
    p = rnd(Rr, C, seed=C + Rr + 20, device=DEV)
    t = _unit_rows(Rr, C, seed=C + Rr + 21)
    if Rr >= 5:
        p[1] = 0.0
        p[3] = 0.75
    p = _settle_norms(p)
    c64, g64, a64 = H.cosine64(p, t, normalize)
    cs, dp = ops.cosine_loss(p, t, normalize)
    ops_per_row = 2 * (H.lane_adds(C, 2) + 6) + 6
    bound = (ops_per_row + H.row_sum_adds(Rr)) * H.U24 * float(a64)
    print(f"[cosine] C={C} R={Rr} n={normalize} err {abs(float(cs) - float(c64)):.3g} bound {bound:.3g}")
    assert abs(float(cs) - float(c64)) <= bound, (float(cs), float(c64), bound)
    fin = torch.isfinite(g64)
    assert bool(torch.isfinite(dp.float()[fin]).all())
    a = min(2e-2, GA["cosine_norm" if normalize else "cosine_raw"])
    within(torch.where(fin, dp.double(), 0.0), torch.where(fin, g64, 0.0), _row_max_bound(torch.where(fin, g64, 0.0), a),
           f"cosine grad C={C} R={Rr} n={normalize}")
    cs2, dp2 = ops.cosine_loss(p, t, normalize)
    assert torch.equal(cs, cs2) and same_bits(dp, dp2)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("Rr", ROWS)
@pytest.mark.parametrize("C", WIDTHS)
def test_soft_ce_loss_across_widths(ops, C, Rr, normalize):
    """-sum t log(q + 1e-10), q = round_bf(softmax(round_bf(u / 0.07))), against fp64 through the same rounding points.  Per term: the sum
    of C exponentials behind q, q + eps, the logarithm (v_log_f32 and the ln 2 product), the product with t -> 6 operations beside the
    lane's 8 adds per vector, 6 tree levels and the row sum.  q ends an fp32 chain, so a q whose fp64 value lies within that chain's error
    of a bf16 tie may round either way; each such q adds t 2^-7 (one bf16 step of q moves its logarithm by 2^-8) -- helper_refs.soft_ce64.
    Gradient relative to the row's largest: 2x the stack's distance (0.0098 normalised, 0.005411 raw -> 0.0196 / 0.01082; existing
    5e-2 |ref| + 3e-2 max).  Rows: N(0,1) (x 0.03 raw); one-hot after the temperature; an exactly one-hot target; all zero; constant."""
    p = rnd(Rr, C, seed=C + Rr + 30, scale=1.0 if normalize else 0.03, device=DEV)
    t = H.round_bf(torch.softmax(_unit_rows(Rr, C, seed=C + Rr + 31).double() / 0.07, -1)).to(BF16)
    if Rr >= 5:
        p[0] = -1.0
        p[0, C // 3] = 1.0
        t[1] = 0.0
        t[1, C - 1] = 1.0
        p[2] = 0.0
        p[3] = 0.25
    p = _settle_norms(p) if normalize else p
    s64, g64, a64, slack = H.soft_ce64(p, t, normalize)
    s, dp = ops.soft_ce_loss(p, t, normalize)
    bound = H.loss_bound(C, Rr, a64, 1, 6) + float(slack)
    print(f"[soft_ce] C={C} R={Rr} n={normalize} err {abs(float(s) - float(s64)):.3g} bound {bound:.3g} (tie slack {float(slack):.3g})")
    assert abs(float(s) - float(s64)) <= bound, (float(s), float(s64), bound)
    fin = torch.isfinite(g64)
    assert bool(torch.isfinite(dp.float()[fin]).all())
    a = min(3e-2, GA["soft_ce_norm" if normalize else "soft_ce_raw"])
    within(torch.where(fin, dp.double(), 0.0), torch.where(fin, g64, 0.0), _row_max_bound(torch.where(fin, g64, 0.0), a),
           f"soft-CE grad C={C} R={Rr} n={normalize}")
    s2, dp2 = ops.soft_ce_loss(p, t, normalize)
    assert torch.equal(s, s2) and same_bits(dp, dp2)


HS = [8, 512, 520, 4096]
NROWS = [1, 6, 8193]


@pytest.mark.parametrize("Rr", NROWS)
@pytest.mark.parametrize("h", HS)
def test_gathers_and_scatter_add_across_widths(ops, h, Rr):
    """splice_gather (proj2d = None, sources >= -1), rows_gather and rows_scatter_add_ on column blocks of wider buffers, negative indices
    interleaved with valid ones inside every workgroup (4 rows): gathers bit for bit, the scatter-add exactly fp64 add -> RNE (one add of
    two bf16 values), everything outside the blocks untouched.  Indices stay inside their contract (unique for the scatter-add)."""
    V = 61
    g = torch.Generator().manual_seed(h + Rr)
    emb = rnd(V, h, seed=h, device=DEV)
    src = torch.randint(0, V, (Rr,), generator=g, dtype=torch.int32)
    src[1::3] = -1
    out = ops.splice_gather(emb, None, src.to(DEV), h)
    want = torch.where((src >= 0)[:, None].to(DEV), emb[src.clamp_min(0).long().to(DEV)], torch.zeros((), dtype=BF16, device=DEV))
    assert same_bits(out, want)
    # rows_gather: in = a column block of a [V, h + 16] buffer, out = a column block of a [R, h + 24] buffer
    wide = rnd(V, h + 16, seed=h + 1, device=DEV)
    obuf = rnd(Rr, h + 24, seed=h + 2, device=DEV)
    before = obuf.clone()
    ops.rows_gather(wide[:, 8:8 + h], src.to(DEV), out=obuf[:, 16:16 + h])
    want = torch.where((src >= 0)[:, None].to(DEV), wide[:, 8:8 + h][src.clamp_min(0).long().to(DEV)], torch.zeros((), dtype=BF16, device=DEV))
    assert same_bits(obuf[:, 16:16 + h], want)
    assert same_bits(obuf[:, :16], before[:, :16]) and same_bits(obuf[:, 16 + h:], before[:, 16 + h:])
    # rows_scatter_add_: R source rows into R + 3 destination rows, a permutation with holes
    dbuf = rnd(Rr + 3, h + 16, seed=h + 3, device=DEV)
    sbuf = rnd(Rr, h + 8, seed=h + 4, device=DEV)
    idx = torch.randperm(Rr + 3, generator=g)[:Rr].to(torch.int32)
    idx[2::4] = -1
    dbefore = dbuf.clone()
    ops.rows_scatter_add_(dbuf[:, 8:8 + h], sbuf[:, :h], idx.to(DEV))
    ref = dbefore[:, 8:8 + h].double()
    live = (idx >= 0).to(DEV)
    ref[idx.long().to(DEV)[live]] += sbuf[:, :h].double()[live]
    assert torch.equal(dbuf[:, 8:8 + h].double(), H.round_bf(ref))
    assert same_bits(dbuf[:, :8], dbefore[:, :8]) and same_bits(dbuf[:, 8 + h:], dbefore[:, 8 + h:])
    untouched = torch.ones(Rr + 3, dtype=torch.bool)
    untouched[idx[idx >= 0].long()] = False
    assert same_bits(dbuf[untouched.to(DEV)], dbefore[untouched.to(DEV)])


@pytest.mark.parametrize("h", HS)
def test_embed_grad_long_segments(ops, h):
    """300 segments (unique token ids) with lengths from 1 to 3 000 (geometrically spaced), their positions shuffled over the rows of dout:
    fp64 sum, |got - ref| <= 2^-8 |ref| + len 2^-24 sum |terms| (len sequential fp32 adds, then RNE); accumulate = True starts from the
    bf16 value already there (one more term); rows of dembed whose token does not occur keep a sentinel pattern; identical bits twice."""
    V, nseg = 1000, 300
    g = torch.Generator().manual_seed(h)
    lens = torch.from_numpy(np.round(np.geomspace(1, 3000, nseg)).astype(np.int64))
    assert int(lens.min()) == 1 and int(lens.max()) == 3000
    lens = lens[torch.randperm(nseg, generator=g)]
    n = int(lens.sum())
    seg = torch.zeros(nseg + 1, dtype=torch.int32)
    seg[1:] = lens.cumsum(0).to(torch.int32)
    pos = torch.randperm(n, generator=g).to(torch.int32)
    tok = torch.randperm(V, generator=g)[:nseg].to(torch.int32)
    dout = rnd(n, h, seed=h + 1, device=DEV)
    tok_of_p = torch.repeat_interleave(tok.long(), lens).to(DEV)
    rows = dout[pos.long().to(DEV)].double()
    ssum = torch.zeros(V, h, dtype=H.F64, device=DEV).index_add_(0, tok_of_p, rows)
    sabs = torch.zeros(V, h, dtype=H.F64, device=DEV).index_add_(0, tok_of_p, rows.abs())
    del rows
    cnt = torch.zeros(V, dtype=H.F64, device=DEV).index_add_(0, tok.long().to(DEV), lens.double().to(DEV))[:, None]
    occurs = (cnt[:, 0] > 0)
    sentinel = torch.full((V, h), 0x1235, dtype=torch.int16, device=DEV).view(BF16)
    args = (dout, tok.to(DEV), seg.to(DEV), pos.to(DEV))
    de = sentinel.clone()
    ops.embed_grad_(de, *args, False)
    within(de[occurs], ssum[occurs], (H.BF_STEP * ssum.abs() + cnt * H.U24 * sabs)[occurs], f"embed_grad h={h}")
    assert same_bits(de[~occurs], sentinel[~occurs])
    de2 = sentinel.clone()
    ops.embed_grad_(de2, *args, False)
    assert same_bits(de, de2)
    prev = rnd(V, h, seed=h + 2, device=DEV)
    prev[~occurs] = sentinel[~occurs]
    acc = prev.clone()
    ops.embed_grad_(acc, *args, True)
    ref = prev.double() + ssum
    within(acc[occurs], ref[occurs], (H.BF_STEP * ref.abs() + (cnt + 1) * H.U24 * (sabs + prev.double().abs()))[occurs], f"embed_grad accumulate h={h}")
    assert same_bits(acc[~occurs], sentinel[~occurs])


CE_GEO = [(8192, 8192), (8185, 8192), (8, 8), (40000, 40064)]


def _ce_logits(V, ld):
    """12 rows: random (x3), rising by 30 over the row (each thread's running maximum moves at every vector it takes), falling, the first
    4 096 columns -inf (each thread's first vector is fully masked, a finite one follows), with ignored rows between the live ones and NaN
    in the padding.  Targets in column 0, column V - 1 and the last partial vector."""
    Rr = 12
    g = torch.Generator().manual_seed(V)
    col = torch.arange(V, dtype=torch.float32)
    x = torch.randn(Rr, V, generator=g) * 3.0
    ramp = 30.0 * col / V
    x[2] = -20.0 + ramp + 0.01 * x[2]
    x[3] = -20.0 + ramp + 0.01 * x[3]
    x[5] = 10.0 - ramp + 0.01 * x[5]
    x[6] = 10.0 - ramp + 0.01 * x[6]
    if V > 4096:
        x[8, :4096] = -float("inf")
        x[9, :4096] = -float("inf")
    lg = torch.full((Rr, ld), float("nan"), dtype=BF16)
    lg[:, :V] = x.to(BF16)
    tg = torch.randint(0, V, (Rr,), generator=g, dtype=torch.int32)
    tg[0], tg[2], tg[5] = 0, V - 1, V - 1 - (V - 1) % 8
    tg[3], tg[6], tg[8] = V - 1, 0, V - 1
    tg[9] = 4096 if V > 4096 else 0
    tg[1] = tg[4] = tg[7] = tg[10] = -100
    return lg, tg


@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("V,ld", CE_GEO)
def test_ce_rows_geometries_and_online_rescale(ops, V, ld, deterministic):
    """ce_rows_ against fp64 (loss and gradient) where a thread takes several vectors (V = 8 192: two; V = 40 000: ten), with logits that
    rise and fall along the row, a fully masked first vector per thread, a padding tail inside the last vector (NaN filled) and ignored rows.
    Loss: a row's value is gmax + log(gsum) - x_t.  gsum is 8 adds and up to 8 rescaled terms per vector a thread takes, 6 + 8 tree levels
    and the final rescale (16 v + 24 operations), each exponential |a| 2^-22 relative with |a| <= the row's spread; the logarithm and the
    two additions 3 * 2^-24 (|lse| + |x_t|); then the row sum's adds (R for the atomics form) on sum |loss_r|.
    Gradient: rtol 1e-2, atol 2e-4 * grad_scale as in test_ce_rows."""
    lg, tg = _ce_logits(V, ld)
    gs = 0.25
    s64, g64, a64 = H.ce_rows64(lg, tg, V, gs)
    live = tg >= 0
    x = lg[:, :V].double()
    fin = torch.where(torch.isfinite(x), x, torch.nan)
    spread = (torch.nan_to_num(fin, nan=-1e30).max(-1).values - torch.nan_to_num(fin, nan=1e30).min(-1).values)[live]
    v = -(-(ld // 8) // 512)
    lse = torch.logsumexp(x, -1)[live]
    xt = x.gather(1, tg.clamp_min(0).long()[:, None])[:, 0][live]
    per_row = (16 * v + 24) * H.U24 + spread * 2.0 ** -22 + 3 * H.U24 * (lse.abs() + xt.abs())
    Rr = lg.shape[0]
    bound = float(per_row.sum()) + (H.row_sum_adds(Rr) if deterministic else Rr) * H.U24 * float((lse - xt).abs().sum())
    outs = []
    for _ in range(2):
        dev = lg.to(DEV).clone()
        ls = torch.zeros(1, device=DEV)
        ops.ce_rows_(dev, tg.to(DEV), V, gs, ls, deterministic=deterministic)
        outs.append((ls.cpu(), dev.cpu()))
    ls, dev = outs[0]
    print(f"[ce_rows] V={V} ld={ld} det={deterministic} err {abs(float(ls) - float(s64)):.3g} bound {bound:.3g}")
    assert abs(float(ls) - float(s64)) <= bound, (float(ls), float(s64), bound)
    within(dev[:, :V], g64[:, :V], 1e-2 * g64[:, :V].abs() + 2e-4 * gs, f"ce grad V={V}")
    assert float(dev[:, V:].float().abs().max() if ld > V else 0.0) == 0
    assert float(dev[~live].float().abs().max()) == 0
    assert same_bits(outs[0][1], outs[1][1])
    if deterministic:
        assert torch.equal(outs[0][0], outs[1][0])


# ================================================================================================ 4. AdamW, every output

def _adamw_grads(n, step, device):
    g = rnd(n, seed=100 + step, device=device)
    q = n // 8
    g[:q] = 0.0                                                 # zero from the first step: denom = eps, p only decays
    sign = torch.where(torch.arange(q, device=device) % 2 == 0, 1.0, -1.0).to(BF16)
    g[q:2 * q] = sign * 2.0 ** 15                               # gr^2 = 2^30 (2^28 scaled): large, finite
    g[2 * q:3 * q] = sign * 2.0 ** -60                          # (1 - b2) gr^2 ~ 2^-124.3, with grad_scale 0.5 ~ 2^-126.3: v goes subnormal
    return g


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("with_scale", [True, False])
def test_adamw_every_output(ops, with_scale, wd):
    """Ten launches of one trajectory (steps 1 .. 9, then 10 000: bias corrections 0.1 / 0.05 at step 1, ~1 at the end) at
    n = 2 * 1 048 576 + 7; after each, p32, m, v and p_out against an fp64 replay of that update from the device's own fp32 state before
    it (helper_refs.adamw_replay64: scalars formed in fp32 as the kernel forms them, gr = fp32(g * gs) taken as input).  With u = 2^-24:
      m' = m b1 + (1 - b1) gr, v' = v b2 + ((1 - b2) gr) gr: products and one sum, <= 3 u (|m b1| + |(1 - b1) gr|) resp. the same of v
      (+ 3 * 2^-150, half a subnormal step per operation, where v underflows: the 2^-60 block, where the reference gives v' ~ 2^-124 .. 2^-127 and a denominator
      of eps, so p only decays by 1 - lr wd and moves by ~1e-12 per step, below its resolution)
      p' = p (1 - lr wd) - (lr / bc1) (m' / (sqrt(v') rsqrt(bc2) + eps)):
        the decay scalar (one possibly contracted fp32 operation) and the product 2 u |p (1 - lr wd)|; the final subtraction u |p'|;
        sqrt(v'): v' is 3 u relative (its terms are positive) -> 1.5 u, sqrtf 1 ulp = 2 u, rsqrtf 1 ulp = 2 u, their product u, + eps u
        -> 7.5 u on the denominator; the quotient 1 ulp = 2 u, lr / bc1 and the product with it u each -> 11.5 u |update|;
        m' carries 3 u (|m b1| + |(1 - b1) gr|) absolutely -> times (lr / bc1) / denominator.
      The replay asserts this is never looser than the existing rtol 1e-5 (+ 1e-6).
    p_out is p32.bfloat16() of the device's own master bit for bit.  A second run of the trajectory gives identical bits everywhere."""
    n = 2 * CAP + 7
    lr, b1, b2, eps = 1e-2, 0.9, 0.95, 1e-8
    steps = list(range(1, 10)) + [10000]
    gsv = 0.5 if with_scale else None
    coef = torch.tensor([0.5], device=DEV) if with_scale else None
    final = []
    for run in range(2):
        p = torch.randn(n, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV)
        m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        pout = torch.empty(n, device=DEV, dtype=BF16)
        for step in steps:
            gr = _adamw_grads(n, step, DEV)
            if run == 0:
                rp, rm, rv, bp, bm, bv = H.adamw_replay64(p, m, v, gr, lr, b1, b2, eps, wd, step, gsv)
                assert bool((bp <= 1e-5 * rp.abs() + 1e-6).all()), step
            ops.adamw_shard_(p, m, v, gr, pout, lr, b1, b2, eps, wd, step, coef)
            if run == 0:
                within(m, rm, bm, f"adamw m step {step}")
                within(v, rv, bv, f"adamw v step {step}")
                within(p, rp, bp, f"adamw p32 step {step}")
                assert same_bits(pout, p.bfloat16()), step
        final.append((p, m, v, pout))
    for a, b in zip(*final):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16),
                           b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16))
    q = n // 8
    p, m, v, _ = final[0]
    assert float(m[:q].abs().max()) == 0 and float(v[:q].abs().max()) == 0          # the zero block never moved its moments


# ================================================================================================ 5. im2col

@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("geo", [(3, 378, 378, 14, 608), (2, 56, 84, 14, 608), (2, 84, 56, 14, 592), (1, 60, 75, 14, 588)])
def test_im2col_on_images_that_are_not_square(ops, geo, dtype):
    """bit for bit against torch.nn.functional.unfold on the image cropped to whole patches (a "valid" convolution drops the remainder),
    padding columns zero: 3 x 378 x 378 (1 329 696 elements: a second grid pass), wide and tall images, Kp exactly 3 p^2 with H and W no
    multiples of p."""
    N, Hh, W, p, Kp = geo
    img = torch.randn(N, 3, Hh, W, generator=torch.Generator().manual_seed(Hh + W)).to(dtype)
    gh, gw, k = Hh // p, W // p, 3 * p * p
    cols = ops.im2col_patch(img.to(DEV), p, Kp)
    assert cols.shape == (N * gh * gw, Kp)
    ref = torch.nn.functional.unfold(img.bfloat16().float()[:, :, :gh * p, :gw * p], p, stride=p).transpose(1, 2).reshape(-1, k)
    assert same_bits(cols[:, :k].cpu(), ref.bfloat16())
    if Kp > k:
        assert int(H.bits(cols[:, k:].cpu()).max()) == 0
    assert same_bits(cols, ops.im2col_patch(img.to(DEV), p, Kp))


# ================================================================================================ 6. the recomputed act

def test_recomputed_act_equals_the_forward(ops):
    """swiglu_bwd's act output and swiglu_bwd_t's actT (the operand of down_proj's weight gradient) against swiglu_fwd on 650 x 14 336
    (640 rows for the tiled kernel) N(0, 1.5^2) gates: bit for bit.  The backward forms silu as g * (1 / (1 + e)), the forward as
    g / (1 + e); measured on MI355X: 0 of 9 318 400 (swiglu_bwd) and 0 of 9 175 040 (swiglu_bwd_t) elements differ."""
    I = 14336
    for M in (650, 640):
        gu = rnd(M, 2 * I, seed=7, scale=1.5, device=DEV)
        da = rnd(M, I, seed=8, device=DEV)
        act = ops.swiglu_fwd(gu, I)
        _, act2 = ops.swiglu_bwd(gu, da, I)
        diff = int((act.view(torch.int16) != act2.view(torch.int16)).sum())
        print(f"[recomputed act] swiglu_bwd M={M}: {diff} of {act.numel()} elements differ from swiglu_fwd")
        assert diff == 0, (M, diff, act.numel())
        if M % 64 == 0:
            _, actT, _ = ops.swiglu_bwd_t(gu, da, I)
            diff = int((act.t().contiguous().view(torch.int16) != actT.view(torch.int16)).sum())
            print(f"[recomputed act] swiglu_bwd_t M={M}: {diff} of {act.numel()} elements differ from swiglu_fwd")
            assert diff == 0, (M, diff, act.numel())
