"""The autograd nodes of the trainable SigLIP tower (functional.PatchEmbedFn, SiglipLayerFn, BilinearL2NormFn) at so400m geometry --
h = 1152, 16 heads of d = 72, I = 4304, image 378 / patch 14 (P = 729 tokens, k = 588 padded to 592), N = 2 images -- against fp64
autograd through tests/tower_refs.py.  Needs an MI355X:  pytest -m gpu

At this size the node drives what the tiny-geometry tower test cannot: weight- and input-gradient GEMMs at K = 1458 and N = 4304 (both
ragged), attn_bwd non-causal at d = 72 / L = 729 / 16 heads, gemm(residual=, res_row_mod=729), the 8-row LayerNorm-backward class and
the column sums of 1458 rows.

Tolerances are set against a yardstick that does not involve the code under test: the same layer evaluated by plain torch on the CPU
in bf16 (modules and autograd in torch.bfloat16 -- what the reference stack computes).  Its relative Frobenius error to the fp64
reference is measured per tensor, and each of our tensors must satisfy  rel_err <= 1.5 x yardstick + 1e-3  (the margin the project
uses for this kind of comparison: two correct bf16 implementations differ in accumulation order).  Both columns are printed."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tower_refs as T  # noqa: E402

DEV = "cuda"
GEO = dict(hidden_size=1152, intermediate_size=4304, num_attention_heads=16, image_size=378, patch_size=14, layer_norm_eps=1e-6)
HV, IV, HEADS, P, EPS = 1152, 4304, 16, 729, 1e-6
N_IMG = 2
MARGIN, FLOOR = 1.5, 1e-3


@pytest.fixture(scope="module")
def ops():
    from metamorph_amd import ops as _ops
    from metamorph_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _ops


def _layer_values():
    """seeded bf16 values: Linear weights scaled so that the attention logits span several units and the fc1 pre-activations reach both
    GELU tails, LayerNorm weights N(1, 0.3), every bias non-zero, x a SigLIP-like residual stream, an upstream gradient with a mean"""
    g = torch.Generator().manual_seed(11)
    std = {"self_attn.q_proj": 0.05, "self_attn.k_proj": 0.05, "self_attn.v_proj": 0.03, "self_attn.out_proj": 0.03, "mlp.fc1": 0.04, "mlp.fc2": 0.02}
    shape = {"self_attn.q_proj": (HV, HV), "self_attn.k_proj": (HV, HV), "self_attn.v_proj": (HV, HV), "self_attn.out_proj": (HV, HV),
             "mlp.fc1": (IV, HV), "mlp.fc2": (HV, IV)}
    p = {}
    for name in T.LAYER_PARAM_NAMES:
        mod, kind = name.rsplit(".", 1)
        if mod.startswith("layer_norm"):
            v = (1.0 if kind == "weight" else 0.0) + (0.3 if kind == "weight" else 0.2) * torch.randn(HV, generator=g)
        elif kind == "weight":
            v = std[mod] * torch.randn(*shape[mod], generator=g)
        else:
            v = 0.3 * torch.randn(shape[mod][0], generator=g) + 0.05
        p[name] = T.to_bf16(v)
    x = T.siglip_like_rows(N_IMG * P, HV, seed=12)[0]
    dy = T.to_bf16(torch.randn(N_IMG * P, HV, generator=g) + 0.3)
    dz = T.to_bf16(torch.randn(N_IMG, 256, HV, generator=g) + 0.3)
    return p, x, dy, dz


def _autograd_layer(p, x, dy, dz, dtype):
    """plain torch in `dtype`: layer output and gradients for dy, then (a second graph) the layer input's gradient through the 27 -> 16
    bilinear reduction + L2 norm for dz (interpolation in fp32 as the reference stack does it, when dtype is bf16)"""
    pp = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    stats = {}
    y = T.siglip_layer_ref(xx, pp, N_IMG, P, HEADS, EPS, stats)
    y.backward(dy.to(dtype))
    out = {"y": y.detach(), "dx": xx.grad.clone()}
    out.update({k: v.grad.clone() for k, v in pp.items()})
    xx.grad = None
    y = T.siglip_layer_ref(xx, pp, N_IMG, P, HEADS, EPS).view(N_IMG, P, HV)
    wide = torch.float32 if dtype == torch.bfloat16 else dtype
    z = T.bilinear_l2norm_autograd(y.to(wide), 27, 16, False).to(dtype)
    z = torch.nn.functional.normalize(z, p=2, dim=-1)
    z.backward(dz.to(dtype))
    out["z"], out["dx_through_bilinear"] = z.detach(), xx.grad.clone()
    return out, stats


@pytest.fixture(scope="module")
def layer_case():
    """values, the fp64 reference and the bf16 CPU yardstick's relative Frobenius errors, computed once"""
    p, x, dy, dz = _layer_values()
    ref, stats = _autograd_layer(p, x, dy, dz, torch.float64)
    yard, _ = _autograd_layer(p, x, dy, dz, torch.bfloat16)
    yardstick = {k: T.rel_fro(yard[k], ref[k]) for k in ref}
    return dict(p=p, x=x, dy=dy, dz=dz, ref=ref, yardstick=yardstick, stats=stats)


def _device_layer(p):
    from metamorph_amd.model.multimodal_encoder.siglip_encoder import _EncoderLayer
    layer = _EncoderLayer(GEO)
    layer.load_state_dict({k: v.float() for k, v in p.items()})
    return layer.to(DEV).to(torch.bfloat16)


def _run_layer(layer, x, dy, recompute, clear=True, dz=None):
    """one forward + backward through SiglipLayerFn (and BilinearL2NormFn 27 -> 16 when dz is given); everything cloned, since the
    gradient buffers are reused by the next backward"""
    from metamorph_amd import functional as Fn
    if clear:
        for q in layer.parameters():
            q.grad = None
    geo = Fn.SiglipGeo(N_IMG, P, HEADS, HV // HEADS, EPS, recompute=recompute)
    xin = x.detach().to(DEV).requires_grad_(True)
    y = Fn.SiglipLayerFn.apply(xin, layer, geo, *layer.parameters())
    if dz is None:
        y.backward(dy.to(DEV))
    else:
        z = Fn.BilinearL2NormFn.apply(y.view(N_IMG, P, HV), 27, 16, True)
        z.backward(dz.to(DEV))
    torch.cuda.synchronize()
    out = {"y": y.detach().clone(), "dx": xin.grad.clone()}
    out.update({k: v.grad.clone() for k, v in layer.named_parameters()})
    if dz is not None:
        out["z"] = z.detach().clone()
    return out


@pytest.fixture(scope="module")
def layer_runs(ops, layer_case):
    c = layer_case
    layer = _device_layer(c["p"])
    saved = _run_layer(layer, c["x"], c["dy"], recompute=False)
    recomputed = _run_layer(layer, c["x"], c["dy"], recompute=True)
    twice = _run_layer(layer, c["x"], c["dy"], recompute=True, clear=False)
    through = _run_layer(layer, c["x"], None, recompute=False, dz=c["dz"])
    return dict(saved=saved, recomputed=recomputed, twice=twice, through=through)


def _judge(rows):
    """rows: (name, our rel err, yardstick rel err); prints the table, then asserts every line"""
    print(f"\n   {'tensor':34s} {'ours':>10s} {'bf16 CPU':>10s} {'limit':>10s}")
    for name, e, yd in rows:
        print(f"   {name:34s} {e:10.3e} {yd:10.3e} {MARGIN * yd + FLOOR:10.3e}")
    for name, e, yd in rows:
        assert e <= MARGIN * yd + FLOOR, (name, e, yd)


def test_siglip_layer_inputs_are_hostile_enough(layer_case):
    """what the seeded weights were scaled for, read from the fp64 reference: logits spanning several units within a softmax row, fc1
    pre-activations in both GELU tails"""
    s = layer_case["stats"]
    print(f"\n   logits [{s['logit_min']:.1f}, {s['logit_max']:.1f}], median span within a row {s['logit_row_span']:.1f}; "
          f"fc1 pre-activations [{s['fc1_min']:.1f}, {s['fc1_max']:.1f}]")
    assert s["logit_row_span"] >= 4.0 and s["fc1_min"] <= -4.0 and s["fc1_max"] >= 4.0


def test_siglip_layer_fn_against_fp64(layer_case, layer_runs):
    """SiglipLayerFn: output, dx and the parameter gradients against siglip_layer_ref, each within 1.5 x the bf16 CPU yardstick + 1e-3.
    k_proj.bias is judged as test_trainable_vision_tower_gradients_against_oracle judges it: softmax is invariant to a shift of all keys
    along q, so its exact gradient is zero (the fp64 reference shows 1e-16 noise) and ours must be bf16 noise next to q_proj.bias's."""
    ref, yard, got = layer_case["ref"], layer_case["yardstick"], layer_runs["saved"]
    names = ["y", "dx"] + [n for n in T.LAYER_PARAM_NAMES if n != "self_attn.k_proj.bias"]
    _judge([(n, T.rel_fro(got[n], ref[n]), yard[n]) for n in names])
    qb = float(ref["self_attn.q_proj.bias"].norm())
    kb_ref, kb = float(ref["self_attn.k_proj.bias"].norm()), float(got["self_attn.k_proj.bias"].float().norm())
    print(f"   k_proj.bias: |grad| ours {kb:.3e}, fp64 {kb_ref:.3e}, next to |q_proj.bias grad| {qb:.3e}")
    assert kb_ref <= 1e-4 * qb and kb <= 5e-2 * qb
    assert len(names) + 1 == 2 + 16


def test_siglip_layer_fn_recompute_gives_the_same_bits(layer_runs):
    """recompute=True (gradient checkpointing: only x is saved, the forward runs again in backward) equals recompute=False bit for bit"""
    a, b = layer_runs["saved"], layer_runs["recomputed"]
    assert set(a) == set(b) and len(a) == 18
    for k in a:
        assert torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)), k


def test_siglip_layer_fn_second_backward_accumulates(layer_runs):
    """a second backward onto the existing .grad: every parameter gradient becomes bf16(g1 + v) with g1 = bf16(v), so it is 2 g1 within one
    bf16 rounding of the sum (half a step of 2 g1) plus g1's own rounding (half a step of g1)"""
    one, two = layer_runs["recomputed"], layer_runs["twice"]
    for k in T.LAYER_PARAM_NAMES:
        g1, g2 = one[k].double().cpu(), two[k].double().cpu()
        tol = 0.5 * T.bf16_step(2 * g1) + 0.5 * T.bf16_step(g1)
        bad = (g2 - 2 * g1).abs() > tol
        assert not bool(bad.any()), (k, int(bad.sum()), float((g2 - 2 * g1).abs().max()))
        assert float(g1.abs().max()) > 0
    assert torch.equal(one["dx"], two["dx"]) and torch.equal(one["y"], two["y"])


def test_bilinear_l2norm_fn_after_the_layer(layer_case, layer_runs):
    """BilinearL2NormFn (27 -> 16, normalised) on the layer's output: z, and dx of the layer INPUT through both nodes, against the composed
    fp64 reference with the same yardstick rule"""
    ref, yard, got = layer_case["ref"], layer_case["yardstick"], layer_runs["through"]
    _judge([("z (27->16, l2norm)", T.rel_fro(got["z"], ref["z"]), yard["z"]),
            ("dx through layer + bilinear", T.rel_fro(got["dx"], ref["dx_through_bilinear"]), yard["dx_through_bilinear"])])


@pytest.mark.parametrize("N", [2, 3])
def test_patch_embed_fn_against_fp64(ops, N):
    """PatchEmbedFn at 378 / 14 (k = 588 -> 592, res_row_mod = 729): output and the gradients of the patch weight, its bias and the position
    table (a 2- or 3-row column sum over 839 808 columns) against patch_embed_ref, yardstick rule as above"""
    from metamorph_amd import functional as Fn
    from metamorph_amd.model.multimodal_encoder.siglip_encoder import _Embeddings
    g = torch.Generator().manual_seed(20 + N)
    vals = {"patch_embedding.weight": T.to_bf16(0.03 * torch.randn(HV, 3, 14, 14, generator=g)),
            "patch_embedding.bias": T.to_bf16(0.3 * torch.randn(HV, generator=g) + 0.05),
            "position_embedding.weight": T.to_bf16(0.5 * torch.randn(P, HV, generator=g))}
    images = T.to_bf16(torch.randn(N, 3, 378, 378, generator=g) + 0.2)
    dy = T.to_bf16(torch.randn(N * P, HV, generator=g) + 0.3)

    def autograd(dtype):
        q = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in vals.items()}
        y = T.patch_embed_ref(images.to(dtype), q["patch_embedding.weight"], q["patch_embedding.bias"], q["position_embedding.weight"])
        y.backward(dy.view(N, P, HV).to(dtype))
        out = {k: v.grad for k, v in q.items()}
        out["y"] = y.detach().reshape(N * P, HV)
        return out
    ref, yard = autograd(torch.float64), autograd(torch.bfloat16)
    emb = _Embeddings(GEO)
    emb.load_state_dict({k: v.float() for k, v in vals.items()})
    emb = emb.to(DEV).to(torch.bfloat16)
    y = Fn.PatchEmbedFn.apply(images.to(DEV), emb, *emb.parameters())
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    got = {k: v.grad for k, v in emb.named_parameters()}
    got["y"] = y.detach()
    _judge([(f"N={N} {k}", T.rel_fro(got[k], ref[k]), T.rel_fro(yard[k], ref[k])) for k in ("y",) + tuple(vals)])
