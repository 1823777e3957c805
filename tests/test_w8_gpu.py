"""Weight-only FP8 (e4m3) decode on the device: mm355_gemv*_w8 and mm355_dequant_w8_bf16 against the fp64 evaluation of their contract
(y = epilogue(scale[n] * sum_k fp32(Q[n][k]) * fp32(x[m][k]))), the fused forms against the launch sequences they replace, and a model
quantised with quantize_decoder_ against a bf16 model holding the same (dequantised) weights."""
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


def quantised(N, K, seed):
    """A weight whose rows span magnitudes 2^-12 .. 2^3 (so do its scales, up to the factor 448): a forgotten or misplaced scale fails."""
    from metamorph_amd import ops as o
    g = torch.Generator().manual_seed(seed)
    mag = 2.0 ** (torch.rand(N, generator=g) * 15 - 12)
    w = (torch.randn(N, K, generator=g) * 0.3 * mag[:, None]).bfloat16()
    q, s = o.quantize_w8(w)
    return q, s, q.view(torch.float8_e4m3fn).double() * s.double()[:, None]


def gelu_erf64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


@pytest.mark.parametrize("NK", [(64, 512), (130, 1040), (6144, 4096), (1000, 14336), (4096, 64), (40, 16896)])
@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 7, 8, 13, 16])
def test_gemv_w8(ops, M, NK):
    """test_gemv's shape x row grid and its bars (the kernel and the fp64 reference differ by the fp32 summation order only, as there)."""
    N, K = NK
    q, s, wd = quantised(N, K, seed=2)
    x, b, r = rnd(M, K, seed=1, scale=0.5), rnd(N, seed=3), rnd(M, N, seed=4)
    ref = x.double() @ wd.t()
    xd, qd, sd = x.to(DEV), q.to(DEV), s.to(DEV)
    close(ops.gemv_w8(xd, qd, sd), ref, 1e-2, 0.02, f"gemv_w8 {M}x{N}x{K}")
    close(ops.gemv_w8(xd, qd, sd, bias=b.to(DEV), gelu="erf"), gelu_erf64(ref + b.double()), 1e-2, 0.02, "gemv_w8 bias+gelu")
    close(ops.gemv_w8(xd, qd, sd, residual=r.to(DEV)), ref + r.double(), 1e-2, 0.03, "gemv_w8 residual")
    of = torch.empty(M, N, device=DEV, dtype=torch.float32)
    close(ops.gemv_w8(xd, qd, sd, out=of), ref, 1e-4, 2e-3, "gemv_w8 f32")
    wide = torch.zeros(N, K + 64, dtype=torch.uint8)
    wide[:, 32:32 + K] = q                                        # strided weight rows
    close(ops.gemv_w8(xd, wide.to(DEV)[:, 32:32 + K], sd), ref, 1e-2, 0.02, "gemv_w8 strided")


@pytest.mark.parametrize("M", [1, 3, 4, 6, 16])
def test_gemv_w8_decodes_every_byte_exactly(ops, M):
    """A 256-column weight row holding every encoding (the two NaNs replaced by zero), one-hot x rows: the fp32 output is float(e4m3) *
    scale exactly -- an fnuz decode, a byte-order slip inside the packed conversion or a sign slip shows."""
    enc = torch.arange(256, dtype=torch.uint8)
    enc[0x7f] = 0
    enc[0xff] = 0
    q = torch.stack([enc, enc.flip(0), enc.roll(37), enc.roll(-101), enc.roll(5)], 0).contiguous()
    s = torch.tensor([1.0, 0.37, 2.0 ** -9, 3.0, 1.7e-3])
    val = q.view(torch.float8_e4m3fn).float()
    for c0 in range(0, 256, M):
        cols = [(c0 + m) % 256 for m in range(M)]
        x = torch.zeros(M, 256, dtype=torch.bfloat16)
        for m, c in enumerate(cols):
            x[m, c] = 1.0
        out = ops.gemv_w8(x.to(DEV), q.to(DEV), s.to(DEV), out=torch.empty(M, 5, device=DEV, dtype=torch.float32)).cpu()
        want = (val[:, cols] * s[:, None]).t()
        assert torch.equal(out, want), (M, c0)


@pytest.mark.parametrize("M", [1, 4, 8, 16])
def test_fused_w8_forms_equal_their_launch_sequences(ops, M):
    for (I, K) in ((14336, 4096), (40, 48)):           # (mm355_swiglu_fwd takes I % 8 == 0)
        q, s, _ = quantised(2 * I, K, seed=6)
        q, s = q.to(DEV), s.to(DEV)
        x = rnd(M, K, seed=5).to(DEV)
        nw = (1.0 + 0.1 * rnd(K, seed=4).float()).bfloat16().to(DEV)
        assert torch.equal(ops.gemv_swiglu_w8(x, q, s, I), ops.swiglu_fwd(ops.gemv_w8(x, q, s), I)), ("swiglu", M, I, K)
        n = ops.rmsnorm_fwd(x, nw, 1e-5)
        assert torch.equal(ops.gemv_swiglu_w8(x, q, s, I, norm_w=nw, eps=1e-5), ops.swiglu_fwd(ops.gemv_w8(n, q, s), I)), ("norm + swiglu", M, I, K)
    for (Hq, Hkv, d, K) in ((32, 8, 128, 4096), (3, 1, 32, 80)):    # (mm355_rope_kv_append takes d % 16 == 0)
        N, Lmax = (Hq + 2 * Hkv) * d, 50
        q, s, _ = quantised(N, K, seed=8)
        q, s = q.to(DEV), s.to(DEV)
        x = rnd(M, K, seed=7).to(DEV)
        nw = (1.0 + 0.1 * rnd(K, seed=4).float()).bfloat16().to(DEV)
        cos, sin = ops.rope_table(Lmax, d, 10000.0, DEV)
        pos = torch.tensor([(7 * m + 3) % Lmax for m in range(M)], dtype=torch.int32, device=DEV)
        for norm in (False, True):
            k0, v0 = rnd(M, Lmax, Hkv * d, seed=9).to(DEV), rnd(M, Lmax, Hkv * d, seed=10).to(DEV)
            k1, v1 = k0.clone(), v0.clone()
            qkv = ops.gemv_w8(ops.rmsnorm_fwd(x, nw, 1e-5) if norm else x, q, s)
            ops.rope_kv_append_(qkv, Hq, Hkv, d, cos, sin, pos, k0, v0)
            got = ops.gemv_rope_append_w8(x, q, s, Hq, Hkv, d, cos, sin, pos, k1, v1, norm_w=nw if norm else None, eps=1e-5)
            assert torch.equal(got[:, :Hq * d], qkv[:, :Hq * d]), ("q rows", M, Hq, d, norm)
            assert torch.equal(k1, k0) and torch.equal(v1, v0), ("cache rows", M, Hq, d, norm)


def test_dequant_w8_bit_for_bit(ops):
    for (N, K) in ((130, 1040), (6144, 4096), (5, 16)):
        q, s, _ = quantised(N, K, seed=12)
        q, s = q.to(DEV), s.to(DEV)
        assert torch.equal(ops.dequant_w8(q, s), (q.view(torch.float8_e4m3fn).float() * s[:, None]).bfloat16()), (N, K)


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
    """A: quantised with power-of-two scales (lm_head too).  B: a bf16 model whose weights are A's dequantised weights -- exact in bf16 by
    construction, so A and B evaluate the same function and differ by summation order (and by where bf16 roundings of intermediates fall)."""
    cfg, a = _decode_model()
    _, b = _decode_model()
    a.quantize_decoder_(pow2_scales=True, lm_head=True)

    def deq(rec):
        q, s = rec
        w = q.view(torch.float8_e4m3fn).float() * s[:, None]
        assert torch.equal(w.bfloat16().float(), w)
        return w.bfloat16()
    for la, lb in zip(a.model.layers, b.model.layers):
        for name, params in (("qkv", [lb.self_attn.q_proj, lb.self_attn.k_proj, lb.self_attn.v_proj]), ("o", [lb.self_attn.o_proj]),
                             ("gu", [lb.mlp.gate_proj, lb.mlp.up_proj]), ("down", [lb.mlp.down_proj])):
            w, off = deq(getattr(la.w8, name)), 0
            for p in params:
                p.weight.data.copy_(w[off:off + p.weight.shape[0]])
                off += p.weight.shape[0]
    b.lm_head.weight.data.copy_(deq(a.w8_lm_head))
    return cfg, a, b


def _prefill(model, cfg, seqs, cap):
    """seqs: one [L_b, h] prompt per sequence -> (cache, meta, cos, sin, last hidden row per sequence [B, h])"""
    from metamorph_amd import functional as F
    B = len(seqs)
    _, meta = model._decode_meta(max(s.shape[0] for s in seqs))
    cos, sin = model.model.rope_tables(cap, DEV)
    meta.cos, meta.sin = cos, sin
    cache = F.KVCache(cfg.num_hidden_layers, cap, meta.Hkv * meta.d, DEV, Hq=meta.Hq, d=meta.d, batch=B)
    last = []
    for b, s in enumerate(seqs):
        _, mb = model._decode_meta(s.shape[0])
        mb.cos, mb.sin = cos, sin
        last.append(F.decoder_prefill(s.contiguous(), model.model.layers, mb, cache, row=b)[-1:])
    return cache, meta, cos, sin, torch.cat(last, 0).contiguous()


@pytest.mark.parametrize("lens", [(21,), (21, 9, 15), (21,) * 20], ids=["one", "batch3_ragged", "batch20_scratch_route"])
def test_quantised_decode_matches_bf16_model_of_the_dequantised_weights(lens):
    """Teacher-forced: prefill, then feed 19 more rows per sequence; at EVERY position A's logits against B's within 2e-2 x the logit scale
    (test_cached_decode_matches_full_forward's bar for two summation orders).  Batch 20 takes the scratch route (dequantised GEMMs)."""
    from metamorph_amd import functional as F
    cfg, a, b = _pair()
    h, B, steps = cfg.hidden_size, len(lens), 19
    g = torch.Generator().manual_seed(3)
    emb = (torch.randn(B, max(lens) + steps, h, generator=g) * 0.5).bfloat16().to(DEV)
    with torch.no_grad():
        st = {}
        for name, m in (("a", a), ("b", b)):
            st[name] = _prefill(m, cfg, [emb[i, :n] for i, n in enumerate(lens)], max(lens) + steps + 2)
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


def test_quantised_decode_graph_replay_equals_eager():
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


def test_hf_generate_greedy_on_the_quantised_model():
    """Plumbing: HF generate() (greedy, HipKVCache) returns the ids of the model's own per-row loop over forward(past_key_values=...)."""
    from metamorph_amd.model.language_model.metamorph_llama import HipKVCache
    cfg, a = _decode_model()
    a.quantize_decoder_(lm_head=True)
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


def test_quantised_decoder_holds_half_the_bytes():
    """1 byte + 4 / K per weight against 2: 0.502 at K = 1024 (every K >= 1024 here), so <= 0.51 x."""
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
    model.quantize_decoder_()
    after = held()
    print(f"projection bytes: {before} -> {after} ({after / before:.4f})")
    assert after <= 0.51 * before
