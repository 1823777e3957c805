"""Decode over an FP8 (e4m3) KV cache on the device.  The yardstick is bit identity: mm355_kv_quant_f8 / mm355_rope_kv_append_f8 against the
host quantiser ops.quantize_kv8, mm355_attn_decode_f8 against mm355_attn_decode on the dequantised cache (the scales are powers of two, so
every fp32 value of the bf16 kernel is reproduced exactly), and the model-level routes against the bf16-cache model."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.ref_model import OracleConfig, init_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
FMT = "fp8_e4m3"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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


def bf16_next_up(x):
    return (x.to(BF16).view(torch.int16) + 1).view(BF16)


# ------------------------------------------------------------------ 1. the quantiser
@pytest.mark.parametrize("mag", [0.01, 1.0, 300.0])
@pytest.mark.parametrize("Hkv_d", [(2, 128), (4, 64), (16, 72)])
@pytest.mark.parametrize("R", [1, 5, 300])
def test_kv_quant_f8_equals_the_host_quantiser(ops, R, Hkv_d, mag):
    Hkv, d = Hkv_d
    W = Hkv * d
    x = rnd(R, W, seed=R + d, scale=mag)
    r = R - 1
    x[r, :d] = 0                                             # a zero head-row (head 0 of the last row)
    if Hkv > 1:
        x[r, d:2 * d] = rnd(d, seed=3, scale=0.1)
        x[r, d + 1] = 448.0 * 2.0 ** -3                      # amax exactly 448 * 2^k
        x[r, d + 2] = -0.0
    if R > 1:
        x[0, :d] = rnd(d, seed=4, scale=0.1)
        x[0, 1] = bf16_next_up(torch.tensor(448.0 * 2.0 ** 2))   # one bf16 ulp above 448 * 2^k
        h = (Hkv - 1) * d                                    # half-way points of both parities, target subnormals, -0 (scale pinned to 1)
        x[1, h:h + d] = 0
        vals = [448.0, 136.0, 152.0, -168.0, 17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, -5 * 2.0 ** -10, 2.0 ** -11, 2.0 ** -6 + 2.0 ** -10, -0.0,
                2.0 ** -9, -7 * 2.0 ** -9, 2.0 ** -7 + 2.0 ** -10]
        x[1, h:h + len(vals)] = torch.tensor(vals).bfloat16()
    qh, sh = ops.quantize_kv8(x, Hkv, d)
    if R > 1:
        assert float(sh[1, Hkv - 1]) == 1.0 and qh[1, h + 1:h + 6].tolist() == [0x70, 0x72, 0xf2, 0x58, 0x5a]
    # the source as columns of a wider tensor; the destination with sentinel-filled guard rows (and sequences) around it
    wide = torch.full((R, W + 48), 7.0, dtype=BF16)
    wide[:, 16:16 + W] = x
    src = wide.to(DEV)[:, 16:16 + W]
    for rps in ([R] if R < 300 else [R, 100]):
        nseq, row0 = R // rps, 2
        dst = torch.full((nseq + 1, rps + 5, W), 0xA5, dtype=torch.uint8, device=DEV)
        dsc = torch.full((nseq + 1, rps + 5, Hkv), -7.0, dtype=torch.float32, device=DEV)
        ops.kv_quant_f8(src, Hkv, d, dst, dsc, row0=row0, rows_per_seq=rps)
        assert torch.equal(dst[:nseq, row0:row0 + rps].reshape(R, W).cpu(), qh), (R, rps)
        assert torch.equal(dsc[:nseq, row0:row0 + rps].reshape(R, Hkv).cpu(), sh), (R, rps)
        assert bool((dst[:, :row0] == 0xA5).all()) and bool((dst[:, row0 + rps:] == 0xA5).all()) and bool((dst[nseq] == 0xA5).all())
        assert bool((dsc[:, :row0] == -7).all()) and bool((dsc[:, row0 + rps:] == -7).all()) and bool((dsc[nseq] == -7).all())


def test_kv8_entry_points_check_their_arguments(ops):
    from metamorph_amd.lib import Mm355Error
    L = ops._L()
    x = rnd(4, 256, seed=1).to(DEV)
    dst = torch.zeros(1, 8, 256, dtype=torch.uint8, device=DEV)
    sc = torch.zeros(1, 8, 2, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert L.mm355_kv_quant_f8(x.data_ptr(), 256, 4, 4, 2, 128, dst.data_ptr(), 256, sc.data_ptr(), 2, 2048, 16, 0, 7, st) == -1     # fmt
    assert L.mm355_kv_quant_f8(x.data_ptr(), 256, 4, 4, 2, 128, dst.data_ptr(), 256, 0, 2, 2048, 16, 0, 1, st) == -1                 # NULL scale
    assert L.mm355_kv_quant_f8(x.data_ptr() + 2, 256, 4, 4, 2, 128, dst.data_ptr(), 256, sc.data_ptr(), 2, 2048, 16, 0, 1, st) == -1  # alignment
    assert L.mm355_kv_quant_f8(x.data_ptr(), 256, 4, 4, 2, 128, dst.data_ptr(), 252, sc.data_ptr(), 2, 2048, 16, 0, 1, st) == -1      # stride
    assert L.mm355_kv_quant_f8(x.data_ptr(), 256, 4, 4, 2, 124, dst.data_ptr(), 256, sc.data_ptr(), 2, 2048, 16, 0, 1, st) == -2      # d % 8
    assert L.mm355_kv_quant_f8(x.data_ptr(), 256, 4, 4, 1, 256, dst.data_ptr(), 256, sc.data_ptr(), 2, 2048, 16, 0, 1, st) == -2      # d > 128
    q = rnd(1, 256, seed=2).to(DEV)
    kv = torch.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(Mm355Error, match=r"\(-1\)$"):
        ops.attn_decode_f8(q, dst, dst.clone(), sc, sc.clone(), kv, 8, 2, 2, 128, 0.1, variant=1)
    with pytest.raises(ValueError, match="fp4"):
        from metamorph_amd import functional as F
        F.KVCache(1, 8, 128, DEV, d=128, fmt="fp4")


# ------------------------------------------------------------------ 2. RoPE + quantising append
@pytest.mark.parametrize("B", [1, 3, 20])
@pytest.mark.parametrize("shape", [(2, 1, 128), (8, 2, 64), (4, 4, 32)])
def test_rope_kv_append_f8_equals_append_then_quantise(ops, B, shape):
    Hq, Hkv, d = shape
    Lmax, W = 50, Hkv * d
    qkv = rnd(B, (Hq + 2 * Hkv) * d, seed=B, scale=2.0).to(DEV)
    qkv[0, Hq * d:Hq * d + d] = 0                            # a zero K head-row
    cos, sin = ops.rope_table(Lmax, d, 10000.0, DEV)
    pos = torch.tensor([(7 * b + 3) % Lmax for b in range(B)], dtype=torch.int32, device=DEV)
    kb, vb = torch.zeros(B, Lmax, W, device=DEV, dtype=BF16), torch.zeros(B, Lmax, W, device=DEV, dtype=BF16)
    ref = ops.rope_kv_append_(qkv.clone(), Hq, Hkv, d, cos, sin, pos, kb, vb)
    k8 = torch.full((B, Lmax, W), 0xA5, dtype=torch.uint8, device=DEV)
    v8 = k8.clone()
    ks = torch.full((B, Lmax, Hkv), -7.0, dtype=torch.float32, device=DEV)
    vs = ks.clone()
    got = ops.rope_kv_append_f8_(qkv.clone(), Hq, Hkv, d, cos, sin, pos, k8, v8, ks, vs)
    assert torch.equal(got[:, :Hq * d], ref[:, :Hq * d]), "q bits"
    assert torch.equal(got[:, Hq * d:], qkv[:, Hq * d:]), "the k / v columns of the row buffer are left alone"
    for b in range(B):
        p = int(pos[b])
        for c8, cs, cb in ((k8, ks, kb), (v8, vs, vb)):
            qh, sh = ops.quantize_kv8(cb[b, p:p + 1].cpu(), Hkv, d)
            assert torch.equal(c8[b, p].cpu(), qh[0]) and torch.equal(cs[b, p].cpu(), sh[0]), (b, p)
            c8[b, p] = 0xA5
            cs[b, p] = -7.0
    for c8, cs in ((k8, ks), (v8, vs)):
        assert bool((c8 == 0xA5).all()) and bool((cs == -7).all()), "rows that were not addressed are unchanged"


# ------------------------------------------------------------------ 3. attention over the bytes
def kv8_cache(B, Lmax, Hkv, d, seed):
    """An e4m3 cache whose scales are drawn per key and head over 2^-6 .. 2^6 (the bytes so that the dequantised values stay ~ N(0, 1)):
    a dropped, shared or misindexed scale changes the result by factors of two."""
    g = torch.Generator().manual_seed(seed)

    def one():
        e = torch.randint(-6, 7, (B, Lmax, Hkv), generator=g)
        s = torch.ldexp(torch.ones(B, Lmax, Hkv), e)
        y = (torch.randn(B, Lmax, Hkv, d, generator=g) / s[..., None]).clamp(-448, 448)
        return y.to(torch.float8_e4m3fn).view(torch.uint8).reshape(B, Lmax, Hkv * d).contiguous(), s.contiguous()
    return one() + one()


CASES = [(1, 8, 2, 128, [700]), (3, 4, 4, 64, [1, 256, 300]), (2, 32, 4, 128, [513, 77]), (1, 16, 16, 72, [40]), (2, 8, 2, 128, [2500, 1030]),
         (2, 16, 2, 128, [1024, 1025]), (1, 4, 2, 64, [4000]), (3, 32, 8, 128, [128, 129, 127]), (3, 8, 1, 128, [0, 300, 0]), (1, 2, 2, 64, [0])]


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("case", CASES)
def test_attn_decode_f8_equals_attn_decode_on_the_dequantised_cache(ops, case, variant):
    B, Hq, Hkv, d, lens = case
    cap = max(max(lens), 1) + 3
    if max(lens) + 1 <= 1024:
        cap = max(cap, 1030)                                 # room for both bounds: 1024 (one key group) and the capacity
    k8, ks, v8, vs = (t.to(DEV) for t in kv8_cache(B, cap, Hkv, d, seed=sum(lens) + d))
    kb, vb = ops.dequant_kv8(k8, ks, Hkv, d), ops.dequant_kv8(v8, vs, Hkv, d)
    q = rnd(B, Hq * d, seed=5).to(DEV)
    kv = torch.tensor(lens, dtype=torch.int32, device=DEV)
    ws = torch.zeros(int(ops._L().mm355_attn_decode_ws_floats(B, Hq, d, cap)), device=DEV, dtype=torch.float32)
    for bound in ([1024, cap] if max(lens) <= 1024 else [cap]):
        ref = ops.attn_decode(q, kb, vb, kv, bound, Hq, Hkv, d, d ** -0.5, variant=variant)
        got = ops.attn_decode_f8(q, k8, v8, ks, vs, kv, bound, Hq, Hkv, d, d ** -0.5, workspace=ws, variant=variant)
        assert torch.equal(got, ref), (case, bound)
        for b, n in enumerate(lens):
            if n == 0:
                assert float(got[b].float().abs().max()) == 0, "an empty sequence gives a zero row"
        again = ops.attn_decode_f8(q, k8, v8, ks, vs, kv, bound, Hq, Hkv, d, d ** -0.5, workspace=ws, variant=variant)
        assert torch.equal(again, got), "the same workspace again: the counters are back at zero"
        assert int(ws[:B * Hq].view(torch.int32).abs().max()) == 0
    # a q view without 16-byte alignment
    buf = torch.zeros(B, Hq * d + 8, device=DEV, dtype=BF16)
    buf[:, 1:1 + Hq * d] = q
    assert torch.equal(ops.attn_decode_f8(buf[:, 1:1 + Hq * d], k8, v8, ks, vs, kv, cap, Hq, Hkv, d, d ** -0.5, variant=variant),
                       ops.attn_decode(q, kb, vb, kv, cap, Hq, Hkv, d, d ** -0.5, variant=variant))


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("kind", ["sink", "cliff"])
def test_attn_decode_f8_on_hostile_scores(ops, kind, variant):
    """The sink and cliff caches of test_attn_decode_on_hostile_scores, quantised: against the fp64 evaluation of the contract formula
    (s_j = k_scale[j] * sum_c K8 * q * scale, o = sum_j p_j * v_scale[j] * V8 / l) at that test's 2^-7, and against the bf16 twin bit for bit."""
    B, Hq, Hkv, d, lens = 2, 32, 8, 128, [2500, 700]
    Lmax = max(lens) + 3
    g = torch.Generator().manual_seed(11)
    q = (torch.randn(B, Hq, d, generator=g) * 0.5).bfloat16()
    kc = (torch.randn(B, Lmax, Hkv, d, generator=g) * 0.5).bfloat16()
    vc = torch.randn(B, Lmax, Hkv, d, generator=g).bfloat16()
    unit = d ** -0.5 * 8.0
    q[..., 0] = 8.0
    kc[..., 0] = 0
    if kind == "sink":
        kc[:, 0, :, 0] = 40.0 / unit
    else:
        kc[..., 0] = -40.0 / unit
        for b in range(B):
            kc[b, lens[b] - 7, :, 0] = 40.0 / unit
    k8, ks = ops.quantize_kv8(kc.view(B, Lmax, Hkv * d), Hkv, d)
    v8, vs = ops.quantize_kv8(vc.view(B, Lmax, Hkv * d), Hkv, d)
    kv = torch.tensor(lens, dtype=torch.int32, device=DEV)
    dev = [t.to(DEV) for t in (k8, v8, ks, vs)]
    out = ops.attn_decode_f8(q.view(B, Hq * d).to(DEV), *dev, kv, max(lens), Hq, Hkv, d, d ** -0.5, variant=variant)
    kd = k8.view(torch.float8_e4m3fn).double().view(B, Lmax, Hkv, d)
    vd = v8.view(torch.float8_e4m3fn).double().view(B, Lmax, Hkv, d)
    for b in range(B):
        n = lens[b]
        kk = kd[b, :n].transpose(0, 1).repeat_interleave(Hq // Hkv, dim=0)                    # [Hq, n, d]
        vv = vd[b, :n].transpose(0, 1).repeat_interleave(Hq // Hkv, dim=0)
        ksj = ks[b, :n].double().t().repeat_interleave(Hq // Hkv, dim=0)                      # [Hq, n]
        vsj = vs[b, :n].double().t().repeat_interleave(Hq // Hkv, dim=0)
        s = ksj * ((q[b].double() * d ** -0.5)[:, None] @ kk.transpose(1, 2))[:, 0]
        p = torch.softmax(s, dim=-1)
        ref = ((p * vsj)[:, None] @ vv)[:, 0].reshape(Hq * d)
        close(out[b], ref, 2.0 ** -7, 2.0 ** -7, f"attn_decode_f8 {kind} sample {b}")
    twin = ops.attn_decode(q.view(B, Hq * d).to(DEV), ops.dequant_kv8(dev[0], dev[2], Hkv, d), ops.dequant_kv8(dev[1], dev[3], Hkv, d), kv,
                           max(lens), Hq, Hkv, d, d ** -0.5, variant=variant)
    assert torch.equal(out, twin)


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


_MODELS = {}


def model_of(weights):
    """The tiny decoder of tests/test_w8_gpu.py, on bf16 or on quantize_decoder_ weights (built once per module)."""
    if weights not in _MODELS:
        cfg = tiny_cfg()
        m = hip_model(cfg, init_state_dict(cfg, seed=5)).eval()
        if weights == "w8":
            m.quantize_decoder_(lm_head=True)
        _MODELS[weights] = (cfg, m)
    return _MODELS[weights]


def prefill(model, cfg, seqs, cap, fmt):
    """seqs: one [L_b, h] prompt per sequence -> (cache, meta, cos, sin, hidden rows per sequence); prompts of one length go as ONE batch"""
    from metamorph_amd import functional as F
    B = len(seqs)
    _, meta = model._decode_meta(max(s.shape[0] for s in seqs))
    cos, sin = model.model.rope_tables(cap, DEV)
    meta.cos, meta.sin = cos, sin
    cache = F.KVCache(cfg.num_hidden_layers, cap, meta.Hkv * meta.d, DEV, Hq=meta.Hq, d=meta.d, batch=B, fmt=fmt)
    if B > 1 and len({s.shape[0] for s in seqs}) == 1:
        _, mb = model._decode_meta(seqs[0].shape[0])
        mb.B, mb.cos, mb.sin = B, cos, sin
        rows = [F.decoder_prefill(torch.cat(seqs, 0).contiguous(), model.model.layers, mb, cache)]
    else:
        rows = []
        for b, s in enumerate(seqs):
            _, mb = model._decode_meta(s.shape[0])
            mb.cos, mb.sin = cos, sin
            rows.append(F.decoder_prefill(s.contiguous(), model.model.layers, mb, cache, row=b))
    return cache, meta, cos, sin, rows


def embeds(B, L, h, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, L, h, generator=g) * 0.5).bfloat16().to(DEV)


def assert_cache_is_quantised(ops, c8, cb, lens, Hkv, d):
    for b, n in enumerate(lens):
        for t8, ts, tb in ((c8.k, c8.k_scale, cb.k), (c8.v, c8.v_scale, cb.v)):
            qh, sh = ops.quantize_kv8(tb[:, b, :n].cpu(), Hkv, d)
            assert torch.equal(t8[:, b, :n].cpu(), qh) and torch.equal(ts[:, b, :n].cpu(), sh), b


@pytest.mark.parametrize("weights", ["bf16", "w8"])
@pytest.mark.parametrize("lens", [(21,), (21, 9, 15), (21,) * 20], ids=["fused", "per_sequence", "batched"])
def test_prompt_pass_on_an_fp8_cache(ops, lens, weights):
    """4. The prompt pass attends on the unquantised K / V: hidden rows bit-identical to the bf16-cache model's, the cache rows its rows quantised."""
    cfg, m = model_of(weights)
    emb = embeds(len(lens), max(lens), cfg.hidden_size, seed=3)
    seqs = [emb[i, :n] for i, n in enumerate(lens)]
    with torch.no_grad():
        c8, meta, _, _, r8 = prefill(m, cfg, seqs, 40, FMT)
        cb, _, _, _, rb = prefill(m, cfg, seqs, 40, "bf16")
    assert c8.k.dtype == torch.uint8 and cb.k.dtype == BF16 and c8.lengths == cb.lengths == list(lens)
    for a, b in zip(r8, rb):
        assert torch.equal(a, b)
    assert_cache_is_quantised(ops, c8, cb, lens, meta.Hkv, meta.d)


@pytest.mark.parametrize("weights", ["bf16", "w8"])
@pytest.mark.parametrize("B", [1, 6, 20])
def test_decode_step_on_an_fp8_cache_equals_the_unfused_sequence_on_dequantised_rows(ops, B, weights, monkeypatch):
    """5. The step (VALU GEMV / MFMA GEMV / split-K GEMM routes) against the project's own unfused launch sequence on a bf16 cache preloaded
    with the dequantised rows, the freshly appended row replaced by dequant(quantize(row)) before attn_decode reads it."""
    from metamorph_amd import functional as F
    cfg, m = model_of(weights)
    lens = [21 - (b % 3) * 5 for b in range(B)]
    emb = embeds(B, 21 + 3, cfg.hidden_size, seed=7)
    real = ops.rope_kv_append_

    def append_then_round(qkv, Hq, Hkv, d, cos, sin, positions, kc, vc):
        real(qkv, Hq, Hkv, d, cos, sin, positions, kc, vc)
        bi, pi = torch.arange(kc.shape[0], device=DEV), positions.long()
        for c in (kc, vc):
            q8, s8 = ops.quantize_kv8(c[bi, pi].cpu(), Hkv, d)
            c[bi, pi] = ops.dequant_kv8(q8, s8, Hkv, d).to(DEV)
        return qkv
    with torch.no_grad():
        c8, meta, cos, sin, _ = prefill(m, cfg, [emb[i, :n] for i, n in enumerate(lens)], 40, FMT)
        cb = F.KVCache(cfg.num_hidden_layers, 40, meta.Hkv * meta.d, DEV, Hq=meta.Hq, d=meta.d, batch=B)
        cb.k.copy_(ops.dequant_kv8(c8.k, c8.k_scale, meta.Hkv, meta.d))
        cb.v.copy_(ops.dequant_kv8(c8.v, c8.v_scale, meta.Hkv, meta.d))
        cb.set_lengths(lens)
        for t in range(3):
            rows = torch.stack([emb[i, n + t] for i, n in enumerate(lens)], 0).contiguous()
            got = F.decoder_decode_row(rows, m.model.layers, meta, c8, cos, sin)
            old = (F.set_variant("decode_fused", False), F.set_variant("decode_wide_fused", False))
            monkeypatch.setattr(ops, "rope_kv_append_", append_then_round)
            try:
                ref = F.decoder_decode_row(rows, m.model.layers, meta, cb, cos, sin)
            finally:
                monkeypatch.setattr(ops, "rope_kv_append_", real)
                F.set_variant("decode_fused", old[0])
                F.set_variant("decode_wide_fused", old[1])
            assert torch.equal(got, ref), (B, t)
        now = [n + 3 for n in lens]
        assert c8.lengths == now
        for b, n in enumerate(now):                          # (values, not bytes: quantising a dequantised row again may pick a smaller scale)
            assert torch.equal(ops.dequant_kv8(c8.k[:, b, :n], c8.k_scale[:, b, :n], meta.Hkv, meta.d), cb.k[:, b, :n]), b
            assert torch.equal(ops.dequant_kv8(c8.v[:, b, :n], c8.v_scale[:, b, :n], meta.Hkv, meta.d), cb.v[:, b, :n]), b


@pytest.mark.parametrize("weights", ["bf16", "w8"])
def test_fp8_cache_graph_replay_equals_eager(ops, weights):
    """6. Replay == eager launches over several steps; a prompt of 1020 rows + 8 steps takes the bound from 1024 to the capacity."""
    from metamorph_amd import functional as F
    cfg, m = model_of(weights)
    h = cfg.hidden_size
    for L0, steps, cap in ((21, 6, 40), (1020, 8, 1040)):
        emb = embeds(1, L0 + steps, h, seed=4)
        with torch.no_grad():
            c1, meta, cos, sin, _ = prefill(m, cfg, [emb[0, :L0]], cap, FMT)
            c2, _, _, _, _ = prefill(m, cfg, [emb[0, :L0]], cap, FMT)
            stepper = F.DecodeStepGraph(m.model.layers, meta, c2, cos, sin, h, DEV)
            assert stepper.graph is not None
            for t in range(L0, L0 + steps):
                row = emb[0, t:t + 1].contiguous()
                eager = F.decoder_decode_row(row, m.model.layers, meta, c1, cos, sin)
                assert torch.equal(stepper.step(row), eager), t
            n = L0 + steps
            assert torch.equal(c1.k[:, :, :n], c2.k[:, :, :n]) and torch.equal(c1.v[:, :, :n], c2.v[:, :, :n])
            assert torch.equal(c1.k_scale[:, :, :n], c2.k_scale[:, :, :n]) and torch.equal(c1.v_scale[:, :, :n], c2.v_scale[:, :, :n])
            if L0 == 1020:
                assert sorted(stepper.graphs) == [1024, cap]


@pytest.mark.parametrize("weights", ["bf16", "w8"])
def test_hf_generate_on_an_fp8_cache(weights):
    """7. generate(use_customize_greedy=False), greedy and three beams, with config.mm355_kv_cache_format: the same ids with the captured
    step and with eager launches; 8. without the key the cache is bf16."""
    from metamorph_amd import functional as F
    from metamorph_amd.model.language_model.metamorph_llama import HipKVCache
    cfg, m = model_of(weights)
    ids = torch.randint(0, 127000, (1, 11), generator=torch.Generator().manual_seed(9)).to(DEV)
    kw = dict(inputs=ids, use_customize_greedy=False, do_sample=False, max_new_tokens=6, eos_token_id=None, pad_token_id=0)
    assert not hasattr(m.config, "mm355_kv_cache_format")
    with torch.no_grad():
        plain = HipKVCache(capacity=20)
        m(input_ids=ids, past_key_values=plain, use_cache=True)
        assert plain.kv.k.dtype == BF16 and plain.kv.kv8 is None                     # the default
        m.config.mm355_kv_cache_format = FMT
        try:
            c = HipKVCache(capacity=20)
            m(input_ids=ids, past_key_values=c, use_cache=True)
            assert c.kv.k.dtype == torch.uint8 and c.kv.fmt == FMT
            forced = HipKVCache(capacity=20, kv_format="bf16")
            m(input_ids=ids, past_key_values=forced, use_cache=True)
            assert forced.kv.k.dtype == BF16
            for beams in (1, 3):
                a = m.generate(num_beams=beams, **kw)
                old = F.set_variant("decode_graph", False)
                try:
                    b = m.generate(num_beams=beams, **kw)
                finally:
                    F.set_variant("decode_graph", old)
                assert a.shape[1] >= 6 and a.tolist() == b.tolist(), (beams, a.tolist(), b.tolist())
            m.config.mm355_kv_cache_format = "fp4"
            with pytest.raises(ValueError, match="fp4"):
                m(input_ids=ids, past_key_values=HipKVCache(capacity=20), use_cache=True)
        finally:
            del m.config.mm355_kv_cache_format


def test_reorder_cache_moves_bytes_scales_and_lengths():
    from metamorph_amd.model.language_model.metamorph_llama import HipKVCache
    cfg, m = model_of("bf16")
    ids = torch.randint(0, 127000, (3, 9), generator=torch.Generator().manual_seed(2)).to(DEV)
    with torch.no_grad():
        c = HipKVCache(capacity=16, kv_format=FMT)
        m(input_ids=ids, past_key_values=c, use_cache=True)
    kv = c.kv
    kv.set_lengths([9, 7, 8])
    before = [t.clone() for t in (kv.k, kv.v, kv.k_scale, kv.v_scale)]
    idx = [2, 0, 0]
    c.reorder_cache(torch.tensor(idx, device=DEV))
    assert kv.lengths == [8, 9, 9]
    for t, t0 in zip((kv.k, kv.v, kv.k_scale, kv.v_scale), before):
        for i, j in enumerate(idx):
            assert torch.equal(t[:, i, :9], t0[:, j, :9]), i


def test_greedy_decode_runs_through_image_mode_on_an_fp8_cache():
    """The recorded text -> <image_start> -> four continuous image tokens -> text loop (tests/golden/n1_decode_text.npz) on an fp8 cache: the
    state machine emits its four image rows, and the captured step gives what eager launches give."""
    from metamorph_amd import functional as F
    from oracle.ref_model import decode_fixture_state_dict
    g = np.load(os.path.join(GOLDEN, "n1_decode_text.npz"))
    cfg = tiny_cfg(num_image_tokens=4, **(json.loads(str(g["cfg_json"])) if "cfg_json" in g else {}))
    model = hip_model(cfg, decode_fixture_state_dict(g, cfg, torch.bfloat16)).eval()
    model.config.mm355_kv_cache_format = FMT
    kw = dict(inputs=torch.from_numpy(np.asarray(g["input_ids"])).to(DEV), images=None, output_image=True, max_new_tokens=int(g["max_new_tokens"]),
              use_cache=True)
    out, emb = model.generate(**kw)
    old = F.set_variant("decode_graph", False)
    try:
        out2, emb2 = model.generate(**kw)
    finally:
        F.set_variant("decode_graph", old)
    print(f"   ids on the fp8 cache {out[0].tolist()}, recorded on bf16 {g['tokens'].tolist()}")
    assert emb.shape == tuple(g["pred_z"].shape) and bool(torch.isfinite(emb.float()).all())
    assert out[0].tolist() == out2[0].tolist() and torch.equal(emb, emb2)
