"""Weight-only MXFP4 decode, the parts that need no GPU: the quantiser's contract (ops.quantize_w4), the C ABI's symbols and validation and
the refusals of MetaMorphLlamaForCausalLM.quantize_decoder_(fmt="mxfp4")."""
import ctypes
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _hostile():
    g = torch.Generator().manual_seed(11)
    mag = 2.0 ** (torch.rand(12, 8, generator=g) * 40 - 30)          # groups from 2^-30 to 2^10 inside one row
    w = (torch.randn(12, 8, 32, generator=g) * mag[:, :, None]).view(12, 256).bfloat16()
    w[2] = 0                                                         # a row of zero groups
    w[5, 17] = 1e4 * float(w[5, :32].float().abs().mean())           # one outlier: the rest of its group rounds to zero
    w[7, 32:64] = 0
    w[7, 40] = -3.0                                                  # a group with one non-zero element
    return w


def _codes(q):
    return torch.stack((q & 15, q >> 4), 2).view(q.shape[0], -1)


def test_quantiser_contract():
    from metamorph_amd import ops
    w = _hostile()
    q, s = ops.quantize_w4(w)
    N, K = w.shape
    assert q.dtype == torch.uint8 and tuple(q.shape) == (N, K // 2) and s.dtype == torch.uint8 and tuple(s.shape) == (N, K // 32)
    assert int(s.min()) >= 2 and int(s.max()) <= 252, "exponents stay in [-125, 125]; never 0xFF"
    dq = ops.dequant_w4_reference(q, s)
    assert torch.equal(dq.bfloat16().float(), dq), "every dequantised value is a bf16 value"
    # the OCP rule: e = floor(log2(amax)) - 2 per group (zeros: 0)
    wf = w.float().view(N, K // 32, 32)
    amax = wf.abs().amax(2)
    e = torch.where(amax > 0, torch.floor(torch.log2(amax.double())).long() - 2, torch.zeros(N, K // 32, dtype=torch.long))
    assert torch.equal(s.long() - 127, e)
    assert (s[2] == 127).all() and not q[2].any()
    # each element within half a grid step of w / 2^e, or saturated at +-6
    v = (wf.double() / (2.0 ** e.double())[:, :, None]).view(N, K)
    code = _codes(q)
    mag = GRID[(code & 7).long()].double()
    nearest = (GRID.double()[None, None, :] - v.abs()[:, :, None]).abs().amin(2)     # no grid point is nearer: within half a step
    ok = ((mag - v.abs()).abs() == nearest) | ((mag == 6) & (v.abs() > 6))
    assert ok.all(), int((~ok).sum())
    assert torch.equal(((code >> 3) == 1), torch.signbit(w.float())), "the sign is kept"
    # every non-zero group's largest code is 4 or 6 (codes 6 and 7)
    top = (code & 7).view(N, K // 32, 32).amax(2)
    assert ((top[amax > 0] == 6) | (top[amax > 0] == 7)).all()
    # a fixed point
    q2, s2 = ops.quantize_w4(dq)
    assert torch.equal(q2, q) and torch.equal(s2, s)


def test_quantiser_known_answers():
    """amax 6 -> e = 0, S = 127; ties go to the even code; the low nibble is the even k; a zero group has S = 127."""
    from metamorph_amd import ops
    w = torch.zeros(2, 64)
    w[0, :10] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -6.0, -0.5, 1.5])
    #            codes          0     2     2     4     4    6    6   15     9    3
    w[1, 32:36] = torch.tensor([-48.0, 7.9, 8.1, 20.0])              # amax 48: e = 3; 7.9 / 8 -> 1, 8.1 / 8 -> 1, 20 / 8 = 2.5 -> 2
    q, s = ops.quantize_w4(w.bfloat16())
    assert q[0, :5].tolist() == [0x20, 0x42, 0x64, 0xf6, 0x39] and not q[0, 5:].any()
    assert s.tolist() == [[127, 127], [127, 130]]
    assert q[1, 16:18].tolist() == [0x2f, 0x42] and not q[1, :16].any()
    assert ops.dequant_w4_reference(q, s)[1, 32:36].tolist() == [-48.0, 8.0, 8.0, 16.0]


def test_w4_symbols_and_validation_without_a_gpu():
    from metamorph_amd import lib
    names = lib.exported_symbols()
    new = ("mm355_gemv_w4", "mm355_gemv_swiglu_w4", "mm355_gemv_rope_append_w4", "mm355_dequant_w4_bf16")
    for n in new:
        assert n in names, n
    text = open(os.path.join(REPO, "include", "mm355.h")).read()
    assert "#define MM355_W4_MXFP4 2" in text
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(lib.LIB_PATH)
    for n in new:
        assert hasattr(so, n), n
    L = lib.load()
    P = 4096                                                     # a non-null, 16-byte aligned stand-in: no kernel is launched on the error path
    #                   x  ldx Wq ldw S  lds fmt y ldy M  N   K  bias res ldr flags stream
    assert L.mm355_gemv_w4(P, 64, P, 32, P, 2, 1, P, 64, 1, 8, 64, 0, 0, 0, 0, 0) == -1          # the w8 format number
    assert L.mm355_gemv_w4(P, 64, P, 32, P, 2, 2, P, 64, 1, 8, 48, 0, 0, 0, 0, 0) == -1          # K % 32
    assert L.mm355_gemv_w4(P, 64, P, 24, P, 2, 2, P, 64, 1, 8, 64, 0, 0, 0, 0, 0) == -1          # ldw_bytes % 16
    assert L.mm355_gemv_w4(P, 64, P, 32, P, 1, 2, P, 64, 1, 8, 64, 0, 0, 0, 0, 0) == -1          # lds_bytes < K / 32
    assert L.mm355_gemv_w4(P, 64, P, 32, 0, 2, 2, P, 64, 1, 8, 64, 0, 0, 0, 0, 0) == -1          # no scales
    assert L.mm355_gemv_w4(P, 64, P + 8, 32, P, 2, 2, P, 64, 1, 8, 64, 0, 0, 0, 0, 0) == -1      # misaligned weight bytes
    assert L.mm355_gemv_w4(P, 64, P, 32, P, 2, 2, P, 64, 17, 8, 64, 0, 0, 0, 0, 0) == -2         # more than 16 rows: the dequant route
    assert L.mm355_gemv_w4(P, 64, P, 1 << 20, P, 2, 2, P, 64, 1, 3840, 64, 0, 0, 0, 0, 0) == -2  # N * ldw_bytes = 3.75 GiB
    assert L.mm355_gemv_swiglu_w4(P, 64, P, 32, P, 2, 1, P, 8, 1, 4, 64, 0, 0.0, 0) == -1
    assert L.mm355_gemv_swiglu_w4(P, 64, P, 32, P, 2, 2, P, 8, 1, 3, 64, 0, 0.0, 0) == -2        # odd I, as the bf16 form
    assert L.mm355_gemv_swiglu_w4(P, 8192, P, 4096, P, 256, 2, P, 8, 16, 4, 8192, P, 1e-5, 0) == -2   # norm_w, 16 rows beyond 140 KiB
    #                               x  ldx Wq ldw S lds fmt qkv ld M Hq Hkv d  K  nw  eps  cos sin pos kc vc ldkv bs stream
    assert L.mm355_gemv_rope_append_w4(P, 64, P, 32, P, 2, 0, P, 64, 1, 2, 1, 16, 64, 0, 0.0, P, P, P, P, P, 16, 64, 0) == -1
    assert L.mm355_gemv_rope_append_w4(P, 64, P, 32, P, 2, 2, P, 64, 1, 2, 1, 6, 64, 0, 0.0, P, P, P, P, P, 16, 64, 0) == -2   # d % 4
    assert L.mm355_dequant_w4_bf16(P, 32, P, 2, 1, P, 64, 8, 64, 0) == -1
    assert L.mm355_dequant_w4_bf16(P, 32, P, 2, 2, P, 64, 8, 48, 0) == -1


def _tiny_cpu_model(**llm_kw):
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
               rms_norm_eps=1e-5, rope_theta=500000.0)
    llm.update(llm_kw)
    geo = dict(hidden_size=64, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14)
    return build_model(llm, geo, num_image_tokens=4, max_length=64)


def test_quantize_decoder_mxfp4_refusals_by_name():
    from metamorph_amd import functional as F
    model = _tiny_cpu_model()
    with pytest.raises(ValueError, match="unknown format"):
        model.quantize_decoder_(fmt="nf4")
    with pytest.raises(ValueError, match="4-bit lm_head is not supported"):
        model.quantize_decoder_(fmt="mxfp4", lm_head=True)
    odd = _tiny_cpu_model(intermediate_size=144)
    with pytest.raises(ValueError, match="multiples of 32"):
        odd.quantize_decoder_(fmt="mxfp4")
    assert model.w8_format is None and not hasattr(model.model.layers[0], "w8") and not hasattr(odd.model.layers[0], "w8")
    assert model.quantize_decoder_(fmt="mxfp4", pow2_scales=True) is model and not model.training      # (pow2_scales: accepted, no effect)
    assert model.w8_format == "mxfp4" and model.w8_lm_head is None
    layer = model.model.layers[0]
    assert isinstance(layer.w8, F.W4Layer) and layer.w8.NAMES == F.W8Layer.NAMES
    q, s = layer.w8.qkv
    assert q.dtype == torch.uint8 and tuple(q.shape) == (64 + 2 * 32, 32) and s.dtype == torch.uint8 and tuple(s.shape) == (128, 2)
    assert tuple(layer.w8.down[0].shape) == (64, 64) and tuple(layer.w8.down[1].shape) == (64, 4)
    assert layer.self_attn.q_proj.weight.numel() == 0 and model.lm_head.weight.numel() == 320 * 64      # bf16 storage released; the head stays
    assert F.w8_on_gemm(layer, 64) == frozenset() and F.w8_on_gemm(layer, 512) == frozenset()           # no w4 GEMM: the scratch route
    with pytest.raises(RuntimeError, match="already quantised"):
        model.quantize_decoder_(fmt="mxfp4")
    with pytest.raises(RuntimeError, match="state_dict of a decoder quantised"):
        model.state_dict()
    with pytest.raises(NotImplementedError, match="forward without past_key_values on a decoder quantised"):
        model.llm_forward(inputs_embeds=torch.zeros(1, 4, 64, dtype=torch.bfloat16), return_dict=True)
    from metamorph_amd.zero2 import Zero2AdamW
    from metamorph_amd.zero3 import Zero3AdamW
    for opt in (Zero2AdamW, Zero3AdamW):
        with pytest.raises(RuntimeError, match="quantised with quantize_decoder_"):
            opt(model.parameters())


def test_quantize_decoder_mxfp4_keeps_bf16_on_request():
    from metamorph_amd import ops
    model = _tiny_cpu_model()
    w = model.model.layers[1].mlp.down_proj.weight.data.clone()
    model.quantize_decoder_(fmt="mxfp4", keep_bf16=True)
    assert torch.equal(model.model.layers[1].mlp.down_proj.weight.data, w)
    assert "model.layers.1.mlp.down_proj.weight" in model.state_dict()
    q, s = model.model.layers[1].w8.down
    q2, s2 = ops.quantize_w4(w)
    assert torch.equal(q, q2) and torch.equal(s, s2)
