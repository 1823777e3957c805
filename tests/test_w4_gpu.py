"""Weight-only MXFP4 decode on the device: mm355_gemv*_w4 and mm355_dequant_w4_bf16 against the fp64 evaluation of their contract
(y = epilogue(sum_k fp32(Wd[n][k]) * fp32(x[m][k])), Wd = e2m1(nibble) * 2^(S - 127)), the fused forms against the launch sequences they
replace, and a model quantised with quantize_decoder_(fmt="mxfp4") against a bf16 model holding the same (dequantised) weights."""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.ref_model import OracleConfig, init_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from metamorph_amd import ops as o
    return o


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).bfloat16()


def close(got, ref, rtol, atol, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    print(f"{what}: max abs err {float(err.max()):.3e}, max |ref| {float(ref.abs().max()):.3e}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} off, max abs err {float(err.max())}"


@functools.lru_cache(maxsize=None)
def quantised(N, K, seed):
    """A weight whose GROUPS of 32 span magnitudes 2^-12 .. 2^3 within every row (so do its group scales): a scale index that slips by one
    group, a forgotten scale or one taken from the neighbouring row fails.  -> (q, s, fp64 dequantised weight), computed once per shape."""
    from metamorph_amd import ops as o
    g = torch.Generator().manual_seed(seed)
    mag = 2.0 ** (torch.rand(N, K // 32, generator=g) * 15 - 12)
    w = (torch.randn(N, K // 32, 32, generator=g) * 0.3 * mag[:, :, None]).view(N, K).bfloat16()
    q, s = o.quantize_w4(w)
    return q, s, o.dequant_w4_reference(q, s).double()


def gelu_erf64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


@pytest.mark.parametrize("NK", [(8, 32), (64, 512), (130, 1056), (6144, 4096), (1000, 14336), (4096, 64), (40, 16896)])
@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 7, 8, 13, 16])
def test_gemv_w4(ops, M, NK):
    """test_gemv_w8's row grid and bars (the same arithmetic class: exact products summed in fp32, the fp64 reference differs by the
    summation order only)."""
    N, K = NK
    q, s, wd = quantised(N, K, 2)
    x, b, r = rnd(M, K, seed=1, scale=0.5), rnd(N, seed=3), rnd(M, N, seed=4)
    ref = x.double() @ wd.t()
    xd, qd, sd = x.to(DEV), q.to(DEV), s.to(DEV)
    close(ops.gemv_w4(xd, qd, sd), ref, 1e-2, 0.02, f"gemv_w4 {M}x{N}x{K}")
    close(ops.gemv_w4(xd, qd, sd, bias=b.to(DEV), gelu="erf"), gelu_erf64(ref + b.double()), 1e-2, 0.02, "gemv_w4 bias+gelu")
    close(ops.gemv_w4(xd, qd, sd, residual=r.to(DEV)), ref + r.double(), 1e-2, 0.03, "gemv_w4 residual")
    of = torch.empty(M, N, device=DEV, dtype=torch.float32)
    close(ops.gemv_w4(xd, qd, sd, out=of), ref, 1e-4, 2e-3, "gemv_w4 f32")
    wide = torch.zeros(N, K // 2 + 64, dtype=torch.uint8)
    wide[:, 32:32 + K // 2] = q                                   # strided weight rows ...
    swide = torch.full((N, K // 32 + 7), 200, dtype=torch.uint8)
    swide[:, 3:3 + K // 32] = s                                   # ... and strided scale rows
    close(ops.gemv_w4(xd, wide.to(DEV)[:, 32:32 + K // 2], swide.to(DEV)[:, 3:3 + K // 32]), ref, 1e-2, 0.02, "gemv_w4 strided")


@pytest.mark.parametrize("M", [1, 3, 4, 6, 16])
def test_gemv_w4_decodes_every_code_exactly(ops, M):
    """16 weight rows of 256 columns, row r holding code (k + r) % 16 at column k: all 16 codes at every nibble, byte and dword position of
    a 16-byte load.  Group scales from 2^-20 to 2^10, one-hot x rows: the fp32 output is Wd exactly -- a nibble or byte order slip inside
    the packed conversion, a sign slip or a scale taken from the wrong group shows."""
    k = torch.arange(256)
    code = (k[None, :] + torch.arange(16)[:, None]) % 16
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8).contiguous()
    e = torch.tensor([-20, 10, 0, -7, 3, -1, -13, 5])
    s = ((e[None, :] + torch.arange(16)[:, None] * 3) % 31 - 20 + 127).to(torch.uint8)
    s[0] = (e + 127).to(torch.uint8)
    assert int(s.min()) == 107 and int(s.max()) == 137               # 2^-20 and 2^10 are there
    val = ops.dequant_w4_reference(q, s)
    qd, sd = q.to(DEV), s.to(DEV)
    for c0 in range(0, 256, M):
        cols = [(c0 + m) % 256 for m in range(M)]
        x = torch.zeros(M, 256, dtype=torch.bfloat16)
        for m, c in enumerate(cols):
            x[m, c] = 1.0
        out = ops.gemv_w4(x.to(DEV), qd, sd, out=torch.empty(M, 16, device=DEV, dtype=torch.float32)).cpu()
        want = val[:, cols].t()
        assert torch.equal(out, want), (M, c0, out, want)


@pytest.mark.parametrize("M", [1, 4, 8, 16])
def test_fused_w4_forms_equal_their_launch_sequences(ops, M):
    for (I, K) in ((14336, 4096), (40, 64)):
        q, s, _ = quantised(2 * I, K, 6)
        q, s = q.to(DEV), s.to(DEV)
        x = rnd(M, K, seed=5).to(DEV)
        nw = (1.0 + 0.1 * rnd(K, seed=4).float()).bfloat16().to(DEV)
        assert torch.equal(ops.gemv_swiglu_w4(x, q, s, I), ops.swiglu_fwd(ops.gemv_w4(x, q, s), I)), ("swiglu", M, I, K)
        n = ops.rmsnorm_fwd(x, nw, 1e-5)
        assert torch.equal(ops.gemv_swiglu_w4(x, q, s, I, norm_w=nw, eps=1e-5), ops.swiglu_fwd(ops.gemv_w4(n, q, s), I)), ("norm + swiglu", M, I, K)
    for (Hq, Hkv, d, K) in ((32, 8, 128, 4096), (3, 1, 32, 96)):
        N, Lmax = (Hq + 2 * Hkv) * d, 50
        q, s, _ = quantised(N, K, 8)
        q, s = q.to(DEV), s.to(DEV)
        x = rnd(M, K, seed=7).to(DEV)
        nw = (1.0 + 0.1 * rnd(K, seed=4).float()).bfloat16().to(DEV)
        cos, sin = ops.rope_table(Lmax, d, 10000.0, DEV)
        pos = torch.tensor([(7 * m + 3) % Lmax for m in range(M)], dtype=torch.int32, device=DEV)
        for norm in (False, True):
            k0, v0 = rnd(M, Lmax, Hkv * d, seed=9).to(DEV), rnd(M, Lmax, Hkv * d, seed=10).to(DEV)
            k1, v1 = k0.clone(), v0.clone()
            qkv = ops.gemv_w4(ops.rmsnorm_fwd(x, nw, 1e-5) if norm else x, q, s)
            ops.rope_kv_append_(qkv, Hq, Hkv, d, cos, sin, pos, k0, v0)
            got = ops.gemv_rope_append_w4(x, q, s, Hq, Hkv, d, cos, sin, pos, k1, v1, norm_w=nw if norm else None, eps=1e-5)
            assert torch.equal(got[:, :Hq * d], qkv[:, :Hq * d]), ("q rows", M, Hq, d, norm)
            assert torch.equal(k1, k0) and torch.equal(v1, v0), ("cache rows", M, Hq, d, norm)


def test_dequant_w4_bit_for_bit(ops):
    for (N, K) in ((130, 1056), (6144, 4096), (5, 32)):
        q, s, _ = quantised(N, K, 12)
        want = ops.dequant_w4_reference(q, s)
        assert torch.equal(want.bfloat16().float(), want)
        got = ops.dequant_w4(q.to(DEV), s.to(DEV)).cpu()
        assert torch.equal(got.view(torch.int16), want.bfloat16().view(torch.int16)), (N, K)


def test_w4_error_codes(ops):
    from metamorph_amd import lib
    L = lib.load()
    x = torch.zeros(17, 64, device=DEV, dtype=torch.bfloat16)
    q = torch.zeros(8, 32, device=DEV, dtype=torch.uint8)
    s = torch.full((8, 2), 127, device=DEV, dtype=torch.uint8)
    y = torch.empty(17, 8, device=DEV, dtype=torch.bfloat16)
    args = lambda M, K: (x.data_ptr(), 64, q.data_ptr(), 32, s.data_ptr(), 2, ops.W4_MXFP4, y.data_ptr(), 8, M, 8, K, 0, 0, 0, 0, 0)
    assert L.mm355_gemv_w4(*args(16, 64)) == 0
    assert L.mm355_gemv_w4(*args(17, 64)) == -2                   # MM355_EUNSUPPORTED: more than 16 rows
    assert L.mm355_gemv_w4(*args(1, 48)) == -1                    # MM355_EINVAL: K % 32
    with pytest.raises(lib.Mm355Error):
        ops.gemv_w4(x, q, s)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the model
def tiny_cfg(**kw):
    base = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                num_key_value_heads=1, vocab_size=128258, v_layers=2, v_intermediate=144, v_image=56,
                num_image_tokens=4, tokenizer_model_max_length=64)
    base.update(kw)
    return OracleConfig(**base)


def hip_model(cfg, sd):
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_hidden_layers,
               num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads,
               vocab_size=cfg.vocab_size, rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta,
               max_position_embeddings=cfg.max_position_embeddings, tie_word_embeddings=cfg.tie_word_embeddings)
    geo = dict(hidden_size=cfg.v_hidden, intermediate_size=cfg.v_intermediate, num_hidden_layers=cfg.v_layers,
               num_attention_heads=cfg.v_heads, image_size=cfg.v_image, patch_size=cfg.v_patch, layer_norm_eps=cfg.v_ln_eps)
    return build_model(llm, geo, num_image_tokens=cfg.num_image_tokens, use_vision_ar=cfg.use_vision_ar,
                       normalize_vision=cfg.normalize_vision, apply_softmax=cfg.apply_softmax, image_start_id=cfg.image_start_id,
                       mm_projector_type=cfg.mm_projector_type, image_token_reduction=cfg.image_token_reduction,
                       vision_coef=cfg.vision_coef, max_length=cfg.tokenizer_model_max_length,
                       padding_side=cfg.tokenizer_padding_side, state_dict=sd, device=DEV)


def _decode_model(**kw):
    cfg = tiny_cfg(num_key_value_heads=1, **kw)
    sd = init_state_dict(cfg, seed=5)
    return cfg, hip_model(cfg, sd).eval()


def _pair():
    """A: quantised to "mxfp4".  B: a bf16 model whose weights are A's dequantised weights -- exact in bf16 by format, so A and B evaluate
    the same function and differ by summation order (and by where bf16 roundings of intermediates fall)."""
    from metamorph_amd import functional as F, ops as o
    cfg, a = _decode_model()
    _, b = _decode_model()
    a.quantize_decoder_(fmt="mxfp4")
    assert a.w8_format == "mxfp4" and a.w8_lm_head is None

    def deq(rec):
        w = o.dequant_w4_reference(*rec)
        assert torch.equal(w.bfloat16().float(), w)
        return w.bfloat16()
    for la, lb in zip(a.model.layers, b.model.layers):
        assert isinstance(la.w8, F.W4Layer) and not F.w8_on_gemm(la, 20) and not F.w8_on_gemm(la, 512)
        for name, params in (("qkv", [lb.self_attn.q_proj, lb.self_attn.k_proj, lb.self_attn.v_proj]), ("o", [lb.self_attn.o_proj]),
                             ("gu", [lb.mlp.gate_proj, lb.mlp.up_proj]), ("down", [lb.mlp.down_proj])):
            w, off = deq(getattr(la.w8, name)), 0
            for p in params:
                p.weight.data.copy_(w[off:off + p.weight.shape[0]])
                off += p.weight.shape[0]
    return cfg, a, b


def _prefill(model, cfg, seqs, cap, fmt="bf16"):
    """seqs: one [L_b, h] prompt per sequence -> (cache, meta, cos, sin, last hidden row per sequence [B, h])"""
    from metamorph_amd import functional as F
    B = len(seqs)
    _, meta = model._decode_meta(max(s.shape[0] for s in seqs))
    cos, sin = model.model.rope_tables(cap, DEV)
    meta.cos, meta.sin = cos, sin
    cache = F.KVCache(cfg.num_hidden_layers, cap, meta.Hkv * meta.d, DEV, Hq=meta.Hq, d=meta.d, batch=B, fmt=fmt)
    last = []
    for b, s in enumerate(seqs):
        _, mb = model._decode_meta(s.shape[0])
        mb.cos, mb.sin = cos, sin
        last.append(F.decoder_prefill(s.contiguous(), model.model.layers, mb, cache, row=b)[-1:])
    return cache, meta, cos, sin, torch.cat(last, 0).contiguous()


@pytest.mark.parametrize("lens,kv", [((21,), "bf16"), ((21, 9, 15), "bf16"), ((21,) * 20, "bf16"), ((21, 9, 15), "fp8_e4m3")],
                         ids=["one", "batch3_ragged", "batch20_scratch_route", "batch3_fp8_cache"])
def test_w4_decode_matches_bf16_model_of_the_dequantised_weights(lens, kv):
    """Teacher-forced: prefill, then feed 19 more rows per sequence; at EVERY position A's logits against B's within 2e-2 x the logit scale
    (the project's bar for two summation orders).  Batch 20 takes the scratch route (dequantised GEMMs); one case runs both models on an
    fp8_e4m3 KV cache."""
    from metamorph_amd import functional as F
    cfg, a, b = _pair()
    h, B, steps = cfg.hidden_size, len(lens), 19
    g = torch.Generator().manual_seed(3)
    emb = (torch.randn(B, max(lens) + steps, h, generator=g) * 0.5).bfloat16().to(DEV)
    with torch.no_grad():
        st = {}
        for name, m in (("a", a), ("b", b)):
            st[name] = _prefill(m, cfg, [emb[i, :n] for i, n in enumerate(lens)], max(lens) + steps + 2, fmt=kv)
        xa, xb = st["a"][4], st["b"][4]
        for t in range(steps + 1):
            la, lb = a._rows_logits(xa), b._rows_logits(xb)
            scale = float(lb.abs().max())
            err = float((la - lb).abs().max())
            print(f"step {t}: max logit diff {err:.4e}, scale {scale:.4e}")
            assert err <= 2e-2 * scale, f"step {t}: logits differ by {err} (scale {scale})"
            if t < steps:
                rows = torch.stack([emb[i, n + t] for i, n in enumerate(lens)], 0).contiguous()
                xa = F.decoder_decode_row(rows, a.model.layers, st["a"][1], st["a"][0], st["a"][2], st["a"][3])
                xb = F.decoder_decode_row(rows, b.model.layers, st["b"][1], st["b"][0], st["b"][2], st["b"][3])
        assert st["a"][0].lengths == [n + steps for n in lens]


def test_w4_decode_graph_replay_equals_eager():
    from metamorph_amd import functional as F
    cfg, a, _ = _pair()
    h = cfg.hidden_size
    g = torch.Generator().manual_seed(4)
    emb = (torch.randn(1, 30, h, generator=g) * 0.5).bfloat16().to(DEV)
    with torch.no_grad():
        c1, meta, cos, sin, _ = _prefill(a, cfg, [emb[0, :21]], 40)
        c2, _, _, _, _ = _prefill(a, cfg, [emb[0, :21]], 40)
        stepper = F.DecodeStepGraph(a.model.layers, meta, c2, cos, sin, h, DEV)
        assert stepper.graph is not None
        for t in range(21, 30):
            row = emb[0, t:t + 1].contiguous()
            eager = F.decoder_decode_row(row, a.model.layers, meta, c1, cos, sin)
            assert torch.equal(stepper.step(row), eager), t
        assert torch.equal(c1.k[:, :, :30], c2.k[:, :, :30]) and torch.equal(c1.v[:, :, :30], c2.v[:, :, :30])


def test_hf_generate_greedy_on_the_w4_model():
    """Plumbing: HF generate() (greedy, HipKVCache) returns the ids of the model's own per-row loop over forward(past_key_values=...)."""
    from metamorph_amd.model.language_model.metamorph_llama import HipKVCache
    cfg, a = _decode_model()
    a.quantize_decoder_(fmt="mxfp4")
    ids = torch.randint(0, 127000, (1, 11), generator=torch.Generator().manual_seed(9)).to(DEV)
    new = 6
    with torch.no_grad():
        cache = HipKVCache(capacity=11 + new + 2)
        out = a(input_ids=ids, past_key_values=cache, use_cache=True)
        mine = []
        for _ in range(new):
            tok = out.logits[:, -1].argmax(-1)
            mine.append(int(tok))
            out = a(input_ids=tok.view(1, 1), past_key_values=cache, use_cache=True)
        got = a.generate(inputs=ids, use_customize_greedy=False, do_sample=False, max_new_tokens=new, eos_token_id=None, pad_token_id=0)
    assert got[0, -new:].tolist() == mine, (got.tolist(), mine)


def test_w4_decoder_holds_a_quarter_of_the_bytes():
    """4 bits + 8 / 32 bits per weight against 16: 4.25 / 16 = 0.2656, so <= 0.27 x."""
    cfg = tiny_cfg(hidden_size=1024, intermediate_size=2048, num_attention_heads=8, num_key_value_heads=2, num_hidden_layers=3)
    model = hip_model(cfg, init_state_dict(cfg, seed=23, dtype=torch.bfloat16)).eval()

    def held():
        n = 0
        for l in model.model.layers:
            for p in (l.self_attn.q_proj, l.self_attn.k_proj, l.self_attn.v_proj, l.self_attn.o_proj, l.mlp.gate_proj, l.mlp.up_proj, l.mlp.down_proj):
                n += p.weight.numel() * p.weight.element_size()
            rec = getattr(l, "w8", None)
            if rec is not None:
                n += sum(t.numel() * t.element_size() for name in rec.NAMES for t in getattr(rec, name))
        return n
    before = held()
    model.quantize_decoder_(fmt="mxfp4")
    after = held()
    print(f"projection bytes: {before} -> {after} ({after / before:.4f})")
    assert after <= 0.27 * before
