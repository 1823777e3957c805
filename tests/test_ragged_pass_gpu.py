"""functional.decoder_extend_ragged on the device: a ragged batch of prompts, and of follow-up turns, as ONE packed pass over the weights.
The seeded tiny decoder of tests/test_extend_pass_gpu.py (h = 256, 2 / 1 heads of 128, 2 layers).  The yardstick is an fp32 evaluation of
the same layers in stock torch on the device (_ref_layers below): the hidden rows and the cached K / V rows of the ragged route and of the
sequential route (decoder_prefill / decoder_extend per sequence) are both compared with it, and the ragged route's max relative error
(max |got - ref| / max |ref|) may be at most 1.5 x the sequential route's own on the same inputs; both errors are printed.
On an fp8_e4m3 cache the comparison is the SECOND of the two the route's semantics allow: the ragged pass on uniform lengths (five new rows
on filled caches of 21 / 9 / 15 rows) against decoder_extend per sequence, by test_extend_pass_gpu's logits criterion -- a prompt's first
row attends its own QUANTISED v row on this route, which no existing pass does, so there is no sequential run to hold a prompt to."""
import pytest
import torch

from test_extend_pass_gpu import check_logits, embeds, model_meta, model_of, new_cache

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMT = "fp8_e4m3"
PROMPTS = (9, 21, 12, 17, 14)                                     # five prompts of 9 .. 21 rows
TURN_PAST, TURN_NEW = (21, 9, 15), (4, 11, 1)


def _ref_layers(ref, x, cos, sin):
    """x [L, h] (the bf16 input rows) through the decoder layers of `ref` in fp32, stock torch: -> (hidden rows [L, h] pre final norm, per
    layer the post-RoPE k and the v rows [L, Hkv*d]).  HF LlamaDecoderLayer: RMSNorm, rotate_half RoPE on the model's own tables, causal
    softmax(q k^T d^-0.5) v with the GQA group sharing a KV head, SwiGLU."""
    cfg = ref.config
    Hq, Hkv, eps = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.rms_norm_eps
    L = x.shape[0]
    d = cfg.hidden_size // Hq
    x = x.float()
    c, s = cos[:L].float()[:, None, :], sin[:L].float()[:, None, :]
    W = lambda m: m.weight.detach().float()
    norm = lambda t, w: t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps) * w.detach().float()
    rot = lambda t: t * c + torch.cat([-t[..., d // 2:], t[..., :d // 2]], -1) * s
    causal = torch.ones(L, L, dtype=torch.bool, device=x.device).tril()
    kv = []
    for layer in ref.model.layers:
        att, mlp = layer.self_attn, layer.mlp
        n1 = norm(x, layer.input_layernorm.weight)
        q = rot((n1 @ W(att.q_proj).T).view(L, Hq, d))
        k = rot((n1 @ W(att.k_proj).T).view(L, Hkv, d))
        v = (n1 @ W(att.v_proj).T).view(L, Hkv, d)
        kv.append((k.reshape(L, Hkv * d), v.reshape(L, Hkv * d)))
        kk, vv = k.repeat_interleave(Hq // Hkv, 1).transpose(0, 1), v.repeat_interleave(Hq // Hkv, 1).transpose(0, 1)      # [Hq, L, d]
        sc = (q.transpose(0, 1) @ kk.transpose(1, 2)) * d ** -0.5
        o = (torch.softmax(sc.masked_fill(~causal, float("-inf")), -1) @ vv).transpose(0, 1).reshape(L, Hq * d)
        x = x + o @ W(att.o_proj).T
        n2 = norm(x, layer.post_attention_layernorm.weight)
        x = x + (torch.nn.functional.silu(n2 @ W(mlp.gate_proj).T) * (n2 @ W(mlp.up_proj).T)) @ W(mlp.down_proj).T
    return x, kv


def _rel(got, ref):
    return float((got.float() - ref).abs().max() / ref.abs().max())


def _bar(what, ragged, sequential):
    print(f"   {what}: max rel err ragged {ragged:.4e}, sequential {sequential:.4e}")
    assert ragged <= 1.5 * sequential, f"{what}: ragged {ragged} > 1.5 x sequential {sequential}"


def _compare(what, refs, lens, new, out_r, out_s, cache_r, cache_s, n_layers):
    """hidden rows (the last new[b] of each reference) and cache rows [0, lens[b]) of every layer, both routes against the fp32 reference"""
    ref_h = torch.cat([refs[b][0][lens[b] - new[b]:] for b in range(len(lens))], 0)
    _bar(f"{what} hidden rows", _rel(torch.cat(list(out_r), 0), ref_h), _rel(torch.cat(list(out_s), 0), ref_h))
    for i in range(n_layers):
        for t, name in ((0, "k"), (1, "v")):
            ref_c = torch.cat([refs[b][1][i][t] for b in range(len(lens))], 0)
            rows = lambda c: torch.cat([(c.k, c.v)[t][i, b, :lens[b]] for b in range(len(lens))], 0)
            _bar(f"{what} layer {i} {name} rows", _rel(rows(cache_r), ref_c), _rel(rows(cache_s), ref_c))


def _prefill_each(m, seqs, cache, cos, sin):
    from metamorph_amd import functional as F
    return [F.decoder_prefill(x.contiguous(), m.model.layers, model_meta(m, x.shape[0], cos, sin), cache, row=b) for b, x in enumerate(seqs)]


def _discipline(cache, lens, fill=7.0):
    assert cache.lengths == list(lens) and cache.pos_dev.tolist() == list(lens) and cache.len_dev.tolist() == [n + 1 for n in lens]
    for b, n in enumerate(lens):
        assert bool((cache.k[:, b, n:] == fill).all()) and bool((cache.v[:, b, n:] == -fill).all()), f"sequence {b}: rows >= {n} were written"


@pytest.mark.parametrize("weights", ["bf16", "w8"])
def test_ragged_prompts_and_turns(weights, monkeypatch):
    """Five prompts of 9 .. 21 rows in one pass on a fresh cache, then n = (4, 11, 1) new rows on filled caches of 21 / 9 / 15 rows; on
    bf16 and on w8-quantised layers (the reference: the bf16 build holding the dequantised weights).  Per layer exactly one
    rope_kv_append_rows and one attn_extend_ragged launch, and the first layer's input norm runs once, on all rows."""
    from metamorph_amd import functional as F, ops
    cfg, m, ref = model_of("tiny", weights)
    h, NL, cap = cfg.hidden_size, cfg.num_hidden_layers, 40
    emb = embeds(len(PROMPTS), max(PROMPTS), h, seed=13)
    seqs = [emb[b, :n].contiguous() for b, n in enumerate(PROMPTS)]
    counts = {"rope_kv_append_rows_": 0, "attn_extend_ragged": 0, "first_norm": [], "other": 0}
    real = {n: getattr(ops, n) for n in ("rope_kv_append_rows_", "attn_extend_ragged", "rmsnorm_fwd", "rope_kv_append_", "attn_extend", "rope_qk_")}
    w0 = m.model.layers[0].input_layernorm.weight

    def counted(name):
        def f(*a, **kw):
            if name == "rmsnorm_fwd":
                if a[1].data_ptr() == w0.data_ptr():
                    counts["first_norm"].append(a[0].shape[0])
            elif name in counts:
                counts[name] += 1
            else:
                counts["other"] += 1
            return real[name](*a, **kw)
        return f
    with torch.no_grad():
        cr, meta, cos, sin = new_cache(m, cfg, cap, batch=len(PROMPTS), fill=7.0)
        cs, _, _, _ = new_cache(m, cfg, cap, batch=len(PROMPTS), fill=7.0)
        refs = [_ref_layers(ref, x, cos, sin) for x in seqs]
        for n in real:
            monkeypatch.setattr(ops, n, counted(n))
        out_r = F.decoder_extend_ragged(seqs, m.model.layers, meta, cr)
        for n in real:
            monkeypatch.setattr(ops, n, real[n])
        assert counts["rope_kv_append_rows_"] == NL and counts["attn_extend_ragged"] == NL and counts["other"] == 0, counts
        assert counts["first_norm"] == [sum(PROMPTS)], counts
        out_s = _prefill_each(m, seqs, cs, cos, sin)
        assert [tuple(o.shape) for o in out_r] == [(n, h) for n in PROMPTS]
        _discipline(cr, PROMPTS)
        _compare(f"{weights} prompts", refs, PROMPTS, PROMPTS, out_r, out_s, cr, cs, NL)

        # follow-up turns: the sequences named out of order, every one at its own cached length
        B = len(TURN_PAST)
        lens = [p + n for p, n in zip(TURN_PAST, TURN_NEW)]
        emb = embeds(B, max(lens), h, seed=17)
        cr, meta, cos, sin = new_cache(m, cfg, cap, batch=B, fill=7.0)
        cs, _, _, _ = new_cache(m, cfg, cap, batch=B, fill=7.0)
        for c in (cr, cs):
            _prefill_each(m, [emb[b, :p] for b, p in enumerate(TURN_PAST)], c, cos, sin)
        new = [emb[b, p:p + n].contiguous() for b, (p, n) in enumerate(zip(TURN_PAST, TURN_NEW))]
        refs = [_ref_layers(ref, emb[b, :lens[b]], cos, sin) for b in range(B)]
        order = [2, 0, 1]
        got = F.decoder_extend_ragged([new[b] for b in order], m.model.layers, meta, cr, rows=order)
        out_r = [got[order.index(b)] for b in range(B)]
        out_s = [F.decoder_extend(new[b], m.model.layers, meta, cs, row=b) for b in range(B)]
        assert [tuple(o.shape) for o in out_r] == [(n, h) for n in TURN_NEW]
        _discipline(cr, lens)
        _compare(f"{weights} turns", refs, lens, TURN_NEW, out_r, out_s, cr, cs, NL)
        # a subset: sequence 1 alone gets three more rows, the others keep their rows and lengths
        before = (cr.k.clone(), cr.v.clone())
        more = embeds(1, 3, h, seed=19)[0]
        one = F.decoder_extend_ragged([more], m.model.layers, meta, cr, rows=[1])
        alone = F.decoder_extend(more, m.model.layers, meta, cs, row=1)
        assert cr.lengths == [lens[0], lens[1] + 3, lens[2]]
        for b in (0, 2):
            assert torch.equal(cr.k[:, b], before[0][:, b]) and torch.equal(cr.v[:, b], before[1][:, b])
        check_logits(m._rows_logits(one[0].contiguous()), m._rows_logits(alone), f"{weights} one sequence of three, 3 more rows")


def test_ragged_pass_on_an_fp8_cache():
    """Uniform lengths on an fp8_e4m3 cache against decoder_extend per sequence (see the module docstring): the logits criterion, and the
    new rows of layer 0 -- whose inputs are the same in both runs -- enter the cache as the quantised form of the rows a bf16-cache run
    of the same pass caches."""
    from metamorph_amd import functional as F, ops
    cfg, m, _ = model_of("tiny", "bf16")
    h, past, n = cfg.hidden_size, (21, 9, 15), 5
    emb = embeds(3, 21 + n, h, seed=7)
    new = [emb[b, p:p + n].contiguous() for b, p in enumerate(past)]
    with torch.no_grad():
        c8, meta, cos, sin = new_cache(m, cfg, 40, fmt=FMT, batch=3)
        cs, _, _, _ = new_cache(m, cfg, 40, fmt=FMT, batch=3)
        cb, _, _, _ = new_cache(m, cfg, 40, batch=3)
        for c in (c8, cs, cb):
            _prefill_each(m, [emb[b, :p] for b, p in enumerate(past)], c, cos, sin)
        got = F.decoder_extend_ragged(new, m.model.layers, meta, c8)
        F.decoder_extend_ragged(new, m.model.layers, meta, cb)
        want = [F.decoder_extend(new[b], m.model.layers, meta, cs, row=b) for b in range(3)]
        assert c8.lengths == cs.lengths == cb.lengths == [p + n for p in past]
        for b, p in enumerate(past):
            check_logits(m._rows_logits(got[b].contiguous()), m._rows_logits(want[b]), f"fp8 cache, sequence {b}: ragged pass against decoder_extend")
            for t8, ts, tb in ((c8.k, c8.k_scale, cb.k), (c8.v, c8.v_scale, cb.v)):
                qh, sh = ops.quantize_kv8(tb[0, b, p:p + n].cpu(), meta.Hkv, meta.d)
                assert torch.equal(t8[0, b, p:p + n].cpu(), qh) and torch.equal(ts[0, b, p:p + n].cpu(), sh), b


def test_ragged_refusals_name_their_reason():
    from metamorph_amd import functional as F
    cfg, m, _ = model_of("tiny", "bf16")
    h = cfg.hidden_size
    xs = [embeds(1, n, h, seed=n)[0] for n in (5, 3)]
    with torch.no_grad():
        cache, meta, cos, sin = new_cache(m, cfg, 24, batch=2)
        L = m.model.layers
        with pytest.raises(ValueError, match="distinct sequences"):
            F.decoder_extend_ragged(xs, L, meta, cache, rows=[0, 0])
        with pytest.raises(ValueError, match="distinct sequences"):
            F.decoder_extend_ragged(xs, L, meta, cache, rows=[0, 2])
        with pytest.raises(ValueError, match="row blocks"):
            F.decoder_extend_ragged(xs[:1], L, meta, cache)
        with pytest.raises(ValueError, match="n_j >= 1"):
            F.decoder_extend_ragged([xs[0], xs[1][:0]], L, meta, cache)
        with pytest.raises(ValueError, match="capacity of 24 rows"):
            F.decoder_extend_ragged([embeds(1, 25, h, seed=1)[0], xs[1]], L, meta, cache)
        bad = model_meta(m, 1, cos, sin)
        bad.Hq, bad.Hkv = 6, 2
        with pytest.raises(ValueError, match="no kernel"):
            F.decoder_extend_ragged(xs, L, bad, cache)
        cache.set_lengths([4, 4])
        cache.shared_len = 2                                      # (as KVCache.set_shared leaves it)
        with pytest.raises(ValueError, match="shared prefix"):
            F.decoder_extend_ragged(xs, L, meta, cache)
        cache.shared_len = 0
        cache.set_lengths([0, 0])
    with pytest.raises(RuntimeError, match="inference pass"), torch.enable_grad():
        F.decoder_extend_ragged(xs, L, meta, cache)
    assert cache.lengths == [0, 0]
