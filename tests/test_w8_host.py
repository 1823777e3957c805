"""Weight-only FP8 (e4m3) decode, the parts that need no GPU: the quantiser's contract, the C ABI's validation and the refusals of
MetaMorphLlamaForCausalLM.quantize_decoder_."""
import ctypes
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hostile_rows():
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(12, 256, generator=g) * 0.05).bfloat16()
    w[2] = 0                                                     # a row of zeros: scale 1
    w[5, 17] = float(w[5].float().abs().mean()) * 1e4            # one outlier 1e4 x the rest: the rest falls into the subnormals / to zero
    w[7] = (torch.randn(256, generator=g) * 2.0 ** -20).bfloat16()
    w[7, 3] = 1.0                                                # values below the e4m3 subnormal step (2^-9 x scale)
    w[9] = (torch.randn(256, generator=g) * 300).bfloat16()
    return w


@pytest.mark.parametrize("pow2", [False, True])
def test_quantiser_contract(pow2):
    """|dequant - w| <= max(2^-4 |w|, 2^-10 scale): half an ulp of a 3-bit mantissa, half the subnormal step 2^-9 (in units of the scale);
    1e-5 relative on top for the fp32 division.  With pow2_scales the scale is rounded UP, which only shrinks w / scale: same bounds."""
    from metamorph_amd import ops
    w = _hostile_rows()
    q, scale = ops.quantize_w8(w, pow2_scales=pow2)
    assert q.dtype == torch.uint8 and q.shape == w.shape and scale.dtype == torch.float32 and scale.shape == (w.shape[0],)
    assert not ((q == 0x7f) | (q == 0xff)).any(), "a NaN encoding"
    amax = w.float().abs().amax(1)
    if pow2:
        assert torch.equal(torch.frexp(scale)[0], torch.full_like(scale, 0.5))          # powers of two ...
        ok = scale >= torch.where(amax > 0, amax / 448, torch.ones_like(amax))           # ... not below amax / 448 ...
        assert ok.all() and (scale[amax > 0] < 2 * amax[amax > 0] / 448).all()           # ... and the nearest such
    else:
        assert torch.equal(scale, torch.where(amax > 0, amax / 448, torch.ones_like(amax)))
    assert float(scale[2]) == 1.0 and not q[2].any()
    dq = q.view(torch.float8_e4m3fn).double() * scale.double()[:, None]
    wd = w.double()
    bound = torch.maximum(2.0 ** -4 * wd.abs(), 2.0 ** -10 * scale.double()[:, None]) * (1 + 1e-5)
    err = (dq - wd).abs()
    assert (err <= bound).all(), (float((err - bound).max()), int((err > bound).sum()))
    if pow2:
        assert torch.equal(dq.float().bfloat16().double(), dq), "pow2 scales: the dequantised weights are bf16 values"


def test_w8_symbols_and_validation_without_a_gpu():
    from metamorph_amd import lib
    names = lib.exported_symbols()
    new = ("mm355_gemv_w8", "mm355_gemv_swiglu_w8", "mm355_gemv_rope_append_w8", "mm355_dequant_w8_bf16")
    for n in new:
        assert n in names, n
    text = open(os.path.join(REPO, "include", "mm355.h")).read()
    assert "metamorph/model/builder.py:13-25" in text
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(lib.LIB_PATH)
    for n in new:
        assert hasattr(so, n), n
    L = lib.load()
    P = 4096                                                     # a non-null, 16-byte aligned stand-in: no kernel is launched on the error path
    #                   x  ldx Wq ldw scale fmt y  ldy M  N   K  bias res ldr flags stream
    assert L.mm355_gemv_w8(P, 64, P, 64, P, 7, P, 64, 1, 8, 64, 0, 0, 0, 0, 0) == -1          # a format that does not exist
    assert L.mm355_gemv_w8(P, 64, P, 64, P, 1, P, 64, 1, 8, 24, 0, 0, 0, 0, 0) == -1          # K % 16
    assert L.mm355_gemv_w8(P, 64, P, 64, 0, 1, P, 64, 1, 8, 64, 0, 0, 0, 0, 0) == -1          # no scales
    assert L.mm355_gemv_w8(P, 64, P + 8, 64, P, 1, P, 64, 1, 8, 64, 0, 0, 0, 0, 0) == -1      # misaligned weight bytes
    assert L.mm355_gemv_w8(P, 64, P, 64, P, 1, P, 64, 17, 8, 64, 0, 0, 0, 0, 0) == -2         # more than 16 rows: the dequant route
    assert L.mm355_gemv_swiglu_w8(P, 64, P, 64, P, 2, P, 8, 1, 4, 64, 0, 0.0, 0) == -1
    assert L.mm355_gemv_swiglu_w8(P, 64, P, 64, P, 1, P, 8, 1, 3, 64, 0, 0.0, 0) == -2        # odd I, as the bf16 form
    assert L.mm355_gemv_rope_append_w8(P, 64, P, 64, P, 0, P, 64, 1, 2, 1, 16, 64, 0, 0.0, P, P, P, P, P, 16, 64, 0) == -1
    assert L.mm355_dequant_w8_bf16(P, 64, P, 3, P, 64, 8, 64, 0) == -1
    assert L.mm355_dequant_w8_bf16(P, 64, P, 1, P, 64, 8, 40, 0) == -1


def _tiny_cpu_model(**llm_kw):
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
               rms_norm_eps=1e-5, rope_theta=500000.0)
    llm.update(llm_kw)
    geo = dict(hidden_size=64, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14)
    return build_model(llm, geo, num_image_tokens=4, max_length=64)


def test_quantize_decoder_refusals_by_name():
    model = _tiny_cpu_model()
    with pytest.raises(ValueError, match="unknown format"):
        model.quantize_decoder_(fmt="int4")
    assert model.w8_format is None
    before = sum(p.numel() * p.element_size() for l in model.model.layers for p in l.parameters())
    assert model.quantize_decoder_(lm_head=True) is model and not model.training
    layer = model.model.layers[0]
    assert layer.w8.qkv[0].dtype == torch.uint8 and layer.w8.qkv[0].shape == (64 + 2 * 32, 64) and layer.w8.down[0].shape == (64, 128)
    assert layer.self_attn.q_proj.weight.numel() == 0 and model.lm_head.weight.numel() == 0         # bf16 storage released
    assert model.model.embed_tokens.weight.dtype == torch.bfloat16 and model.model.embed_tokens.weight.numel() == 320 * 64
    assert sum(p.numel() * p.element_size() for l in model.model.layers for p in l.parameters()) < 0.01 * before
    with pytest.raises(RuntimeError, match="already quantised"):
        model.quantize_decoder_()
    with pytest.raises(RuntimeError, match="state_dict of a decoder quantised"):
        model.state_dict()
    with pytest.raises(NotImplementedError, match="forward without past_key_values on a decoder quantised"):
        model.llm_forward(inputs_embeds=torch.zeros(1, 4, 64, dtype=torch.bfloat16), return_dict=True)
    from metamorph_amd.zero2 import Zero2AdamW
    from metamorph_amd.zero3 import Zero3AdamW
    for opt in (Zero2AdamW, Zero3AdamW):
        with pytest.raises(RuntimeError, match="quantised with quantize_decoder_"):
            opt(model.parameters())


def test_quantize_decoder_refuses_a_tied_lm_head_and_keeps_bf16_on_request():
    tied = _tiny_cpu_model(tie_word_embeddings=True)
    with pytest.raises(ValueError, match="tied embeddings"):
        tied.quantize_decoder_(lm_head=True)
    assert tied.w8_format is None and not hasattr(tied.model.layers[0], "w8")
    model = _tiny_cpu_model()
    w = model.model.layers[1].mlp.down_proj.weight.data.clone()
    model.quantize_decoder_(keep_bf16=True, pow2_scales=True)
    assert torch.equal(model.model.layers[1].mlp.down_proj.weight.data, w)
    assert "model.layers.1.mlp.down_proj.weight" in model.state_dict()
    q, s = model.model.layers[1].w8.down
    from metamorph_amd import ops
    q2, s2 = ops.quantize_w8(w, pow2_scales=True)
    assert torch.equal(q, q2) and torch.equal(s, s2)
