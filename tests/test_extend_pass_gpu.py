"""The extend pass on the device: functional.decoder_extend (n new rows of one sequence on its filled cache in one pass over the weights),
the chunked prompt pass built on it, and the model's `_extend_batch` hook.  The tiny decoders of tests/test_kv8_gpu.py (h = 256, 2 / 1 heads
of 128; h = 1024, 8 / 2 heads, 3 layers), on bf16 and on quantize_decoder_ weights.  The yardstick for logits is the one of
test_cached_decode_matches_full_forward: one llm_forward over all rows, err <= 2e-2 * scale and the argmax equal or a near tie."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.ref_model import OracleConfig, init_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
FMT = "fp8_e4m3"


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


_MODELS = {}


def _build(size):
    cfg = tiny_cfg() if size == "tiny" else tiny_cfg(hidden_size=1024, intermediate_size=2048, num_attention_heads=8,
                                                     num_key_value_heads=2, num_hidden_layers=3)
    return cfg, hip_model(cfg, init_state_dict(cfg, seed=5 if size == "tiny" else 23, dtype=torch.bfloat16)).eval()


def model_of(size, weights):
    """(cfg, model, reference model), built once per module.  "tiny": tiny_cfg(); "h1024": h = 1024, 8 / 2 heads, 3 layers.  "w8": quantised
    with power-of-two scales (lm_head too); its reference -- a quantised decoder has no llm_forward -- is a bf16 build holding the
    dequantised weights, exact in bf16 by construction (the pair of tests/test_w8_gpu.py).  "bf16": the model is its own reference."""
    key = (size, weights)
    if key not in _MODELS:
        cfg, a = _build(size)
        ref = a
        if weights == "w8":
            _, ref = _build(size)
            a.quantize_decoder_(pow2_scales=True, lm_head=True)

            def deq(rec):
                q, sc = rec
                w = q.view(torch.float8_e4m3fn).float() * sc[:, None]
                assert torch.equal(w.bfloat16().float(), w)
                return w.bfloat16()
            for la, lb in zip(a.model.layers, ref.model.layers):
                for name, params in (("qkv", [lb.self_attn.q_proj, lb.self_attn.k_proj, lb.self_attn.v_proj]), ("o", [lb.self_attn.o_proj]),
                                     ("gu", [lb.mlp.gate_proj, lb.mlp.up_proj]), ("down", [lb.mlp.down_proj])):
                    w, off = deq(getattr(la.w8, name)), 0
                    for p in params:
                        p.weight.data.copy_(w[off:off + p.weight.shape[0]])
                        off += p.weight.shape[0]
            ref.lm_head.weight.data.copy_(deq(a.w8_lm_head))
        _MODELS[key] = (cfg, a, ref)
    return _MODELS[key]


def embeds(B, L, h, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, L, h, generator=g) * 0.5).bfloat16().to(DEV)


def new_cache(model, cfg, cap, fmt="bf16", batch=1, fill=None):
    from metamorph_amd import functional as F
    _, meta = model._decode_meta(1)
    cos, sin = model.model.rope_tables(cap, DEV)
    meta.cos, meta.sin = cos, sin
    cache = F.KVCache(cfg.num_hidden_layers, cap, meta.Hkv * meta.d, DEV, Hq=meta.Hq, d=meta.d, batch=batch, fmt=fmt)
    if fill is not None:
        cache.k.fill_(fill)
        cache.v.fill_(-fill)
    return cache, meta, cos, sin


def check_logits(got, full, what):
    """the criterion of test_cached_decode_matches_full_forward, for every row"""
    scale = float(full.abs().max())
    err = (got - full).abs().amax(-1)
    print(f"   {what}: max logit err {float(err.max()):.4f} against 2e-2 * {scale:.3f}")
    assert float(err.max()) <= 2e-2 * scale, f"{what}: logits differ by {float(err.max())} (scale {scale})"
    for t in range(got.shape[0]):
        assert int(got[t].argmax()) == int(full[t].argmax()) or float(full[t].topk(2).values.diff().abs()) < 2e-2 * scale, (what, t)


_FULL = {}


def full_logits(size, weights, emb, tag):
    """ONE llm_forward of the reference model over all rows: made once per (model, input) and left unchanged"""
    key = (size, weights, tag)
    if key not in _FULL:
        with torch.no_grad():
            _FULL[key] = model_of(size, weights)[2].llm_forward(inputs_embeds=emb, return_dict=True).logits[0].clone()
    return _FULL[key]


@pytest.mark.parametrize("weights", ["bf16", "w8"])
@pytest.mark.parametrize("size", ["tiny", "h1024"])
def test_one_extend_pass_gives_the_logits_of_a_full_forward(size, weights, monkeypatch):
    """Prefill 21 rows, then rows 21 .. 39 in ONE decoder_extend: all 19 positions against one llm_forward over the 40 rows (41 for the
    captured decode step that follows), no decode step taken on the way; the cache rows behind row 40 untouched, lengths and device
    positions in step, and the layer-0 K / V rows 21 .. 39 those of a one-shot 40-row prompt pass."""
    from metamorph_amd import functional as F
    cfg, m, _ = model_of(size, weights)
    h, L0, L = cfg.hidden_size, 21, 40
    emb = embeds(1, L + 1, h, seed=3)
    full = full_logits(size, weights, emb, "41 rows")
    calls = []
    real_step, real_row = F.DecodeStepGraph.step, F.decoder_decode_row
    monkeypatch.setattr(F.DecodeStepGraph, "step", lambda self, rows: calls.append("step") or real_step(self, rows))
    monkeypatch.setattr(F, "decoder_decode_row", lambda *a, **k: calls.append("row") or real_row(*a, **k))
    with torch.no_grad():
        cache, meta, cos, sin = new_cache(m, cfg, L + 6, fill=7.0)
        F.decoder_prefill(emb[0, :L0].contiguous(), m.model.layers, model_meta(m, L0, cos, sin), cache)
        rows = F.decoder_extend(emb[0, L0:L].contiguous(), m.model.layers, meta, cache)
        assert calls == [] and tuple(rows.shape) == (L - L0, h)
        check_logits(m._rows_logits(rows), full[L0:L], f"{size} {weights} extend 21 -> 40")
        # cache discipline
        assert cache.lengths == [L] and cache.pos_dev.tolist() == [L] and cache.len_dev.tolist() == [L + 1]
        assert bool((cache.k[:, :, L:] == 7.0).all()) and bool((cache.v[:, :, L:] == -7.0).all())
        one, meta1, _, _ = new_cache(m, cfg, L + 6)
        F.decoder_prefill(emb[0, :L].contiguous(), m.model.layers, model_meta(m, L, cos, sin), one)
        for a, b, what in ((cache.k, one.k, "k"), (cache.v, one.v, "v")):
            r = rel(a[0, 0, L0:L], b[0, 0, L0:L])
            print(f"   layer-0 {what} rows 21 .. 39 against the one-shot prompt pass: rel {r:.2e}")
            assert r < 6e-3, (what, r)
        # one captured decode step on top
        monkeypatch.setattr(F.DecodeStepGraph, "step", real_step)
        monkeypatch.setattr(F, "decoder_decode_row", real_row)
        stepper = F.DecodeStepGraph(m.model.layers, meta, cache, cos, sin, h, DEV)
        x = stepper.step(emb[0, L:L + 1].contiguous())
        check_logits(m._rows_logits(x.clone()), full[L:L + 1], f"{size} {weights} decode step after the extend pass")
        assert cache.lengths == [L + 1]


def model_meta(m, L, cos, sin):
    _, meta = m._decode_meta(L)
    meta.cos, meta.sin = cos, sin
    return meta


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


@pytest.mark.parametrize("weights", ["bf16", "w8"])
def test_chunked_prompt_pass(weights):
    """A 300-row prompt in slices of 128 (128 + 128 + 44) on the h = 1024 model: through functional directly and through _cached_forward with
    HipKVCache(prefill_chunk=128); greedy generate gives the ids of the unchunked run up to a near tie."""
    from metamorph_amd import functional as F
    from metamorph_amd.model.language_model.metamorph_llama import HipKVCache
    cfg, m, _ = model_of("h1024", weights)
    h, L = cfg.hidden_size, 300
    emb = embeds(1, L, h, seed=8)
    full = full_logits("h1024", weights, emb, "300 rows")
    with torch.no_grad():
        cache, meta, cos, sin = new_cache(m, cfg, L + 4)
        rows = F.decoder_prefill_chunked(emb[0].contiguous(), m.model.layers, model_meta(m, L, cos, sin), cache, 128)
        assert cache.lengths == [L] and tuple(rows.shape) == (L, h)
        check_logits(m._rows_logits(rows[-1:].contiguous()), full[-1:], f"{weights} chunked prompt, functional")
        c = HipKVCache(capacity=L + 12, prefill_chunk=128)
        out = m(inputs_embeds=emb, past_key_values=c, use_cache=True)
        assert c.kv.lengths == [L] and c.get_seq_length() == L
        check_logits(out.logits[0, -1:], full[-1:], f"{weights} chunked prompt, _cached_forward")
        # greedy generate: the chunked run against the unchunked one
        ids = torch.randint(0, 127000, (1, L), generator=torch.Generator().manual_seed(9)).to(DEV)
        kw = dict(inputs=ids, use_customize_greedy=False, do_sample=False, max_new_tokens=8, eos_token_id=None, pad_token_id=0,
                  return_dict_in_generate=True, output_scores=True)
        plain = m.generate(past_key_values=HipKVCache(capacity=L + 12), **kw)
        chunked = m.generate(past_key_values=HipKVCache(capacity=L + 12, prefill_chunk=128), **kw)
        a, b = plain.sequences[0].tolist(), chunked.sequences[0].tolist()
        a, b = a[-8:], b[-8:]
        if a != b:
            t = next(i for i in range(8) if a[i] != b[i])
            sc = plain.scores[t][0].float()
            gap, scale = float(sc.topk(2).values.diff().abs()), float(sc[torch.isfinite(sc)].abs().max())
            print(f"   ids differ at step {t}: top-2 gap of the unchunked run {gap:.4f} against 2e-2 * {scale:.3f}")
            assert gap < 2e-2 * scale, (a, b, t, gap, scale)
    m.config.mm355_prefill_chunk_rows = 0
    try:
        with pytest.raises(ValueError, match="mm355_prefill_chunk_rows"):
            m(inputs_embeds=emb, past_key_values=HipKVCache(capacity=L + 12), use_cache=True)
    finally:
        del m.config.mm355_prefill_chunk_rows
    with pytest.raises(ValueError, match="prefill_chunk"):
        HipKVCache(prefill_chunk=0)


@pytest.mark.parametrize("weights", ["bf16", "w8"])
@pytest.mark.parametrize("size", ["tiny", "h1024"])
def test_extend_pass_on_an_fp8_cache(size, weights):
    """The new rows enter an fp8_e4m3 cache as the quantised form of the rows the bf16-cache run caches (layer 0: its inputs are the same in
    both runs), and are attended from there: the logits against n decode steps on the same fp8 cache."""
    from metamorph_amd import functional as F, ops
    cfg, m, _ = model_of(size, weights)
    h, L0, L = cfg.hidden_size, 21, 40
    emb = embeds(1, L, h, seed=3)
    with torch.no_grad():
        c8, meta, cos, sin = new_cache(m, cfg, L + 6, fmt=FMT)
        cb, _, _, _ = new_cache(m, cfg, L + 6)
        cs, _, _, _ = new_cache(m, cfg, L + 6, fmt=FMT)
        for c in (c8, cb, cs):
            F.decoder_prefill(emb[0, :L0].contiguous(), m.model.layers, model_meta(m, L0, cos, sin), c)
        r8 = F.decoder_extend(emb[0, L0:L].contiguous(), m.model.layers, meta, c8)
        F.decoder_extend(emb[0, L0:L].contiguous(), m.model.layers, meta, cb)
        assert c8.lengths == cb.lengths == [L]
        for t8, ts, tb in ((c8.k, c8.k_scale, cb.k), (c8.v, c8.v_scale, cb.v)):
            qh, sh = ops.quantize_kv8(tb[0, 0, L0:L].cpu(), meta.Hkv, meta.d)
            assert torch.equal(t8[0, 0, L0:L].cpu(), qh) and torch.equal(ts[0, 0, L0:L].cpu(), sh)
        steps = torch.cat([F.decoder_decode_row(emb[0, t:t + 1].contiguous(), m.model.layers, meta, cs, cos, sin) for t in range(L0, L)], 0)
        check_logits(m._rows_logits(r8), m._rows_logits(steps), f"{size} {weights} extend on an fp8 cache against {L - L0} decode steps")


@pytest.mark.parametrize("weights", ["bf16", "w8"])
def test_extend_batch_of_three_sequences(weights):
    """Three sequences with 21 / 9 / 15 cached rows, five new rows each through the model's _extend_batch hook: the sequences run one after
    the other, so every one equals its run alone bit for bit; with the extend pass switched off the same call is five decode steps (the
    logits criterion)."""
    from metamorph_amd import functional as F
    from metamorph_amd.model.language_model.metamorph_llama import HipKVCache
    cfg, m, _ = model_of("tiny", weights)
    h, past, n = cfg.hidden_size, (21, 9, 15), 5
    emb = embeds(3, 21 + n, h, seed=7)
    seqs = [emb[b, :p] for b, p in enumerate(past)]
    new = torch.stack([emb[b, p:p + n] for b, p in enumerate(past)], 0)
    with torch.no_grad():
        c = HipKVCache(capacity=40)
        c.pads = [0, 0, 0]
        m._prefill_batch(seqs, c)
        got = m._extend_batch(new, c)
        assert tuple(got.shape) == (3, n, h) and c.kv.lengths == [p + n for p in past]
        for b in range(3):
            alone = HipKVCache(capacity=40)
            alone.pads = [0]
            m._prefill_batch([seqs[b]], alone)
            assert torch.equal(m._extend_batch(new[b:b + 1], alone)[0], got[b]), b
        c2 = HipKVCache(capacity=40)
        c2.pads = [0, 0, 0]
        m._prefill_batch(seqs, c2)
        old = F.set_variant("extend_pass", False)
        try:
            stepped = m._extend_batch(new, c2)
        finally:
            F.set_variant("extend_pass", old)
        assert c2.kv.lengths == [p + n for p in past]
        for b in range(3):
            check_logits(m._rows_logits(got[b].contiguous()), m._rows_logits(stepped[b].contiguous()), f"{weights} sequence {b}: one pass against {n} steps")


def test_extend_refusals_name_their_reason():
    from metamorph_amd import functional as F
    from metamorph_amd.model.language_model.metamorph_llama import HipKVCache
    cfg, m, _ = model_of("tiny", "bf16")
    emb = embeds(1, 30, cfg.hidden_size, seed=2)
    with torch.no_grad():
        cache, meta, cos, sin = new_cache(m, cfg, 24)
        with pytest.raises(ValueError, match="decoder_prefill"):                              # past == 0
            F.decoder_extend(emb[0, :5].contiguous(), m.model.layers, meta, cache)
        F.decoder_prefill(emb[0, :21].contiguous(), m.model.layers, model_meta(m, 21, cos, sin), cache)
        with pytest.raises(ValueError, match="capacity of 24 rows"):                          # 21 + 5 > 24
            F.decoder_extend(emb[0, 21:26].contiguous(), m.model.layers, meta, cache)
        assert cache.lengths == [21]
        c = HipKVCache(capacity=24)
        m(inputs_embeds=emb[:, :21], past_key_values=c, use_cache=True)
        with pytest.raises(ValueError, match="HipKVCache capacity 24"):
            m(inputs_embeds=emb[:, 21:26], past_key_values=c, use_cache=True)
        assert c.kv.lengths == [21]
    with pytest.raises(ValueError, match="prefill_chunk"):
        HipKVCache(prefill_chunk=0)
