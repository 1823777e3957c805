"""The references of tests/tower_refs.py checked on the CPU: every hand-written backward formula against torch.autograd in fp64 (1e-10
relative), the bilinear index / weight rule against F.interpolate, and the input builders against the statistics they claim.  No GPU."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tower_refs as T  # noqa: E402


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("M,h", [(5, 8), (7, 40), (33, 136)])
@pytest.mark.parametrize("with_dres", [True, False])
def test_layernorm_refs_against_autograd(M, h, with_dres):
    eps = 1e-6
    x, _, _ = T.siglip_like_rows(M, h, seed=M)
    w, b = T.norm_params(h, seed=h)
    dy = T.grad_rows_along(x, seed=M + 1)
    dres = T.rows_with_column_mean(M, h, seed=M + 2) if with_dres else None
    xa, wa, ba = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    ya = F.layer_norm(xa, (h,), wa, ba, eps)
    y, xh, rstd = T.layernorm_ref(x, w, b, eps)
    assert _rel(y, ya.detach()) <= 1e-10
    assert float((xh.mean(-1)).abs().max()) <= 1e-12 and _rel((xh * xh).mean(-1) + eps * rstd[:, 0] ** 2, torch.ones(M, dtype=torch.float64)) <= 1e-12
    ya.backward(dy.double())
    dx, dw, db, dw_abs, db_abs = T.layernorm_bwd_ref(dy, x, w, eps, dres)
    want_dx = xa.grad + (dres.double() if with_dres else 0)
    assert _rel(dx, want_dx) <= 1e-10 and _rel(dw, wa.grad) <= 1e-10 and _rel(db, ba.grad) <= 1e-10
    assert bool((dw_abs >= dw.abs() - 1e-12).all()) and bool((db_abs >= db.abs() - 1e-12).all())
    assert _rel(db_abs, dy.double().abs().sum(0)) <= 1e-14


SIDES = [(27, 1), (27, 2), (27, 4), (27, 8), (27, 12), (27, 16), (27, 27), (4, 2)]


@pytest.mark.parametrize("sides", SIDES, ids=lambda s: f"{s[0]}to{s[1]}")
def test_bilinear_ref_indices_and_scatter_against_torch(sides):
    """Without the normalisation the operation is linear: the forward reference is F.interpolate's result rounded once to bf16, and
    the backward reference (a scatter of dy with the corner weights) is autograd's gradient exactly."""
    si, so = sides
    N, C = 2, 8
    g = torch.Generator().manual_seed(si * 100 + so)
    x = T.to_bf16(torch.randn(N, si * si, C, generator=g))
    dy = T.to_bf16(torch.randn(N, so * so, C, generator=g))
    xa = x.double().requires_grad_(True)
    ya = T.bilinear_l2norm_autograd(xa, si, so, False)
    y, r, nrm = T.bilinear_l2norm_ref(x, si, so, False)
    assert nrm is None and torch.equal(y, r) and torch.equal(T.to_bf16(y).double(), y)
    assert bool(((y - ya.detach()).abs() <= 0.5 * T.bf16_step(ya.detach()) * (1 + 1e-12)).all())
    ya.backward(dy.double())
    ref = T.bilinear_l2norm_bwd_ref(x, dy, si, so, False)
    assert _rel(ref["din"], xa.grad) <= 1e-10
    assert float(ref["extra"].abs().max()) == 0.0
    # every output token has between one (identity) and four non-zero corner weights; each weight set sums to one
    assert so * so <= float(ref["count"].sum()) <= 4 * so * so
    ones = T.bilinear_l2norm_bwd_ref(x, torch.ones(N, so * so, C), si, so, False)
    assert abs(float(ones["din"][0, :, 0].sum()) - so * so) <= 1e-9 and torch.equal(ones["din"], ones["abs_sum"])


@pytest.mark.parametrize("sides", [(3, 3), (4, 2)], ids=lambda s: f"{s[0]}to{s[1]}")
def test_bilinear_normalised_backward_formula_against_autograd(sides):
    """With rows whose interpolated values and norm are exact in bf16 (every 2 x 2 source block constant, all magnitudes of a token one
    power of two, C = 16: norm = 4 * 2^a) the rounding points are identities, and the reference must equal autograd through
    F.interpolate + F.normalize to 1e-10 -- this pins dr = (dy - r (r . dy) / n^2) / n and its scatter."""
    si, so = sides
    N, C = 2, 16
    g = torch.Generator().manual_seed(si)
    blk = si // so
    sign = torch.where(torch.rand(N, so, so, C, generator=g) < 0.5, -1.0, 1.0)
    mag = torch.exp2(torch.randint(-3, 4, (N, so, so, 1), generator=g).float())
    x = (sign * mag).repeat_interleave(blk, 1).repeat_interleave(blk, 2).reshape(N, si * si, C).to(T.BF16)
    dy = T.to_bf16(torch.randn(N, so * so, C, generator=g) + 0.3)
    xa = x.double().requires_grad_(True)
    ya = T.bilinear_l2norm_autograd(xa, si, so, True)
    y, r, nrm = T.bilinear_l2norm_ref(x, si, so, True)
    assert _rel(y, ya.detach()) <= 1e-12 and _rel((y * y).sum(-1), torch.ones(N, so * so, dtype=torch.float64)) <= 1e-12
    ya.backward(dy.double())
    ref = T.bilinear_l2norm_bwd_ref(x, dy, si, so, True)
    assert _rel(ref["din"], xa.grad) <= 1e-10
    assert bool((ref["abs_sum"] >= ref["din"].abs() - 1e-12).all()) and bool((ref["extra"] >= 0).all())
    # the fp32-chain budget stays a small fraction of the addends' magnitude (no rounding boundary is in reach on these inputs)
    assert float((ref["extra"] / ref["abs_sum"].clamp_min(1e-300)).median()) <= 64 * T.U


def test_bilinear_ref_clamp_and_parallel_gradient():
    """a zero token: forward 0, backward dy * 1e12 (norm clamped at 1e-12); dy = 3 y: the normalised gradient is the rounding residue
    of a cancellation, far below the magnitude of its addends"""
    si, so, N, C = 4, 2, 2, 16
    g = torch.Generator().manual_seed(5)
    x = T.to_bf16(torch.randn(N, si * si, C, generator=g))
    x[1] = 0
    dy = T.to_bf16(torch.randn(N, so * so, C, generator=g))
    y, _, nrm = T.bilinear_l2norm_ref(x, si, so, True)
    assert float(y[1].abs().max()) == 0.0 and bool((nrm[1] == 1e-12).all())
    ref = T.bilinear_l2norm_bwd_ref(x, dy, si, so, True)
    lin = T.bilinear_l2norm_bwd_ref(x, dy, si, so, False)
    assert _rel(ref["din"][1], lin["din"][1] * 1e12) <= 1e-12
    par = T.bilinear_l2norm_bwd_ref(x, T.to_bf16(3 * y), si, so, True)
    assert float((par["din"][0].abs() / par["abs_sum"][0]).max()) <= 2.0 ** -6


def test_one_bf16_rounding_is_half_a_step_between_2_pow_minus_9_and_2_pow_minus_8_relative():
    """bf16 keeps 8 significant bits: a correctly rounded result is within half a step, 2^(e - 8) for |ref| in [2^e, 2^(e + 1)).  That is
    2^-8 |ref| just above a power of two and 2^-9 |ref| just below the next one, so `0.5 * bf16_step(ref)` is the bound the GPU tests
    use for "one bf16 rounding"; a flat 2^-9 |ref| would refuse correctly rounded values in the lower half of every binade."""
    ref = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20, 2.0 - 2.0 ** -8 - 2.0 ** -20, 3e4, 1e-19], dtype=torch.float64)
    err = (T.to_bf16(ref).double() - ref).abs()
    assert bool((err <= 0.5 * T.bf16_step(ref)).all())
    assert float(err[0] / ref[0]) > 2.0 ** -8 * 0.99 and float(err[1] / ref[1]) < 2.0 ** -9 * 1.01
    assert bool((0.5 * T.bf16_step(ref) <= 2.0 ** -8 * ref).all()) and bool((0.5 * T.bf16_step(ref) > 2.0 ** -9 * ref * (1 - 1e-12)).all())


def test_patch_embed_ref_against_unfold_matmul():
    N, p, side, hv = 2, 14, 3, 24
    g = torch.Generator().manual_seed(2)
    img = torch.randn(N, 3, p * side, p * side, generator=g, dtype=torch.float64)
    w = torch.randn(hv, 3, p, p, generator=g, dtype=torch.float64)
    b, pos = torch.randn(hv, generator=g, dtype=torch.float64), torch.randn(side * side, hv, generator=g, dtype=torch.float64)
    want = F.unfold(img, p, stride=p).transpose(1, 2) @ w.reshape(hv, -1).t() + b + pos
    assert _rel(T.patch_embed_ref(img, w, b, pos), want) <= 1e-10


def test_siglip_layer_ref_is_the_documented_composition():
    """the layer reference against the same composition written out with explicit per-head loops and no torch.nn.functional norms"""
    N, P, heads, h, I, eps = 2, 5, 2, 16, 24, 1e-6
    g = torch.Generator().manual_seed(3)
    shapes = {"layer_norm1": (h,), "layer_norm2": (h,), "self_attn.q_proj": (h, h), "self_attn.k_proj": (h, h), "self_attn.v_proj": (h, h),
              "self_attn.out_proj": (h, h), "mlp.fc1": (I, h), "mlp.fc2": (h, I)}
    p = {}
    for name, shp in shapes.items():
        p[name + ".weight"] = torch.randn(*shp, generator=g, dtype=torch.float64) * (0.3 if len(shp) == 2 else 1.0)
        p[name + ".bias"] = torch.randn(shp[0], generator=g, dtype=torch.float64) * 0.2
    assert set(p) == set(T.LAYER_PARAM_NAMES)
    x = torch.randn(N * P, h, generator=g, dtype=torch.float64)
    stats = {}
    y = T.siglip_layer_ref(x, p, N, P, heads, eps, stats)
    h1, _, _ = T.layernorm_ref(x, p["layer_norm1.weight"], p["layer_norm1.bias"], eps)
    q, k, v = (h1 @ p[f"self_attn.{n}_proj.weight"].t() + p[f"self_attn.{n}_proj.bias"] for n in "qkv")
    d = h // heads
    o = torch.zeros_like(x)
    for n in range(N):
        for hd in range(heads):
            rows, cols = slice(n * P, (n + 1) * P), slice(hd * d, (hd + 1) * d)
            s = q[rows, cols] @ k[rows, cols].t() / d ** 0.5
            e = torch.exp(s - s.max(-1, keepdim=True).values)
            o[rows, cols] = (e / e.sum(-1, keepdim=True)) @ v[rows, cols]
    x2 = x + o @ p["self_attn.out_proj.weight"].t() + p["self_attn.out_proj.bias"]
    h2, _, _ = T.layernorm_ref(x2, p["layer_norm2.weight"], p["layer_norm2.bias"], eps)
    f = h2 @ p["mlp.fc1.weight"].t() + p["mlp.fc1.bias"]
    gelu = 0.5 * f * (1 + torch.tanh(0.7978845608028654 * (f + 0.044715 * f ** 3)))
    want = x2 + gelu @ p["mlp.fc2.weight"].t() + p["mlp.fc2.bias"]
    assert _rel(y, want) <= 1e-10
    assert stats["logit_min"] < stats["logit_max"] and stats["fc1_min"] == float(f.min())


@pytest.mark.parametrize("M,h", [(50, 1152), (1458, 1152), (37, 8), (37, 16384)])
def test_siglip_like_rows_have_the_claimed_statistics(M, h):
    x, ch, rows = T.siglip_like_rows(M, h, seed=7)
    assert x.dtype == T.BF16 and x.shape == (M, h)
    assert len(ch) == max(1, round(0.005 * h)) and len(rows) == max(1, round(0.01 * M))
    x = x.double()
    rest = torch.ones(h, dtype=torch.bool)
    rest[ch] = False
    keep = torch.ones(M, dtype=torch.bool)
    keep[rows] = False
    if M >= 37:
        # outlier channels: tens of times the scale of the rest, and a mean that is not zero
        assert float(x[keep][:, ch].std(0).min()) >= 20 * float(x[keep][:, rest].std()) if rest.any() else True
    if M >= 1000:                                               # (the sample mean of a channel of scale s is only good to s / sqrt(M))
        assert float(x[keep][:, ch].mean(0).abs().min()) >= 3.0
    if rest.any():
        assert abs(float(x[keep][:, rest].std()) - 1.0) <= 0.02 + 4.0 / (2 * int(keep.sum()) * int(rest.sum())) ** 0.5
        # shifted rows: a row mean of +-20 over the ordinary channels
        assert bool(((x[rows][:, rest].mean(-1).abs() - 20.0).abs() <= 1.5).all())
    x2, _, _ = T.siglip_like_rows(M, h, seed=7)
    assert torch.equal(x2.double(), x)                          # seeded


@pytest.mark.parametrize("h", [8, 1152, 16384])
def test_hostile_rows_have_the_claimed_statistics(h):
    M = 50
    off = T.hostile_rows("offset", M, h).double()
    assert abs(float(off.mean()) - 100.0) <= 0.1
    assert bool((off.var(-1, unbiased=False) > 0).all()) if h >= 1152 else bool((off.var(-1, unbiased=False) > 0).any())
    assert bool(((off - 100.0).abs() <= 1.0).all())
    con = T.hostile_rows("constant", M, h).double()
    assert bool((con == con[:, :1]).all()) and bool((con[:, 0] != 0).all()) and len(set(con[:, 0].tolist())) == M
    assert float(T.hostile_rows("zero", M, h).double().abs().max()) == 0.0
    tiny = T.hostile_rows("tiny", M, h).double()
    assert 0 < float(tiny.abs().max()) <= 1e-18 and float(tiny.abs().median()) >= 1e-20
    sp = T.hostile_rows("one_spike", M, h).double()
    assert bool(((sp == T.to_bf16(torch.tensor(3e4)).double()).sum(-1) == 1).all()) and float(sp.abs().median()) < 2.0
    for kind in T.HOSTILE_KINDS:
        assert torch.equal(T.hostile_rows(kind, M, h), T.hostile_rows(kind, M, h)) and T.hostile_rows(kind, M, h).dtype == T.BF16


def test_gradient_rows_make_the_mean_terms_large():
    """grad_rows_along: mean(g) and mean(g xhat) of the LayerNorm backward are of the order of |g| (they are a few percent of it for
    N(0,1) gradients)"""
    x, _, _ = T.siglip_like_rows(64, 1152, seed=3)
    dy = T.grad_rows_along(x, seed=4).double()
    _, xh, _ = T.layernorm_ref(x, torch.ones(1152), torch.zeros(1152), 1e-6)
    assert float(dy.mean(-1).min()) >= 0.15 and abs(float(dy.mean()) - 0.5) <= 0.05 and float((dy * xh).mean(-1).min()) >= 0.5
