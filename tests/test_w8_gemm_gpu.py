"""The weight-only FP8 split-K GEMM on the device (mm355_gemm_w8*): against the fp64 evaluation of the format's contract, bit for bit against
the bf16 split-K kernels on power-of-two scales (the summation order is the same by construction), every e4m3 encoding, and the routes of a
quantised model: steps of more than 16 sequences, the prompt pass and the lm_head run on the bytes and dequantise nothing."""
import functools
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
    got, ref = got.detach().double(), ref.detach().double().to(got.device)
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    print(f"{what}: max abs err {float(err.max()):.3e}, max |ref| {float(ref.abs().max()):.3e}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} off, max abs err {float(err.max())}"


@functools.lru_cache(maxsize=1)
def quantised(N, K, seed):
    """tests/test_w8_gpu.py's helper: a weight whose rows span magnitudes 2^-12 .. 2^3 (so do its scales, up to the factor 448): a forgotten
    or misplaced scale fails.  Drawn and quantised on the device; returns (bytes, scales, fp64 dequantised weight), all on the device."""
    from metamorph_amd import ops as o
    g = torch.Generator(device=DEV).manual_seed(seed)
    mag = 2.0 ** (torch.rand(N, generator=g, device=DEV) * 15 - 12)
    w = (torch.randn(N, K, generator=g, device=DEV).mul_(0.3).mul_(mag[:, None])).bfloat16()
    q, s = o.quantize_w8(w)
    return q, s, q.view(torch.float8_e4m3fn).double() * s.double()[:, None]


@functools.lru_cache(maxsize=1)
def quantised_pow2(N, K, seed):
    """Power-of-two scales in 2^-10 .. 2^4 (row maxima 1.2 x 2^-1 .. 2^12 or so: amax / 448 rounded up to a power of two) -> (bytes, scales,
    the dequantised weight, exact in bf16).  With x ~ 0.5 N(0, 1) no partial sum leaves the normal fp32 range."""
    from metamorph_amd import ops as o
    g = torch.Generator(device=DEV).manual_seed(seed)
    mag = 2.0 ** (torch.rand(N, generator=g, device=DEV) * 13 - 1)
    w = (torch.randn(N, K, generator=g, device=DEV).mul_(0.3).mul_(mag[:, None])).bfloat16()
    q, s = o.quantize_w8(w, pow2_scales=True)
    assert float(s.min()) >= 2.0 ** -10 and float(s.max()) <= 2.0 ** 4
    wd = o.dequant_w8(q, s)
    assert torch.equal(wd.float(), q.view(torch.float8_e4m3fn).float() * s[:, None])
    return q, s, wd


SHAPES = [(6144, 4096), (4096, 4096), (4096, 14336), (28672, 4096), (136, 512), (128256, 4096)]


# ------------------------------------------------------------------ a. against fp64
@pytest.mark.parametrize("NK", SHAPES)
def test_gemm_w8_against_fp64(ops, NK):
    """test_gemv_w8's bars: the kernel and the fp64 reference differ by the fp32 summation order only, as there."""
    N, K = NK
    q, s, wd = quantised(N, K, 2)
    wide = torch.zeros(N, K + 64, dtype=torch.uint8, device=DEV)
    wide[:, 32:32 + K] = q                                       # strided weight rows (ldw_bytes > K)
    for M in ((17,) if N == 128256 else (17, 24, 32, 33, 64, 100, 512)):
        x, r = rnd(M, K, seed=1, scale=0.5).to(DEV), rnd(M, N, seed=4).to(DEV)
        ref = x.double() @ wd.t()
        close(ops.gemm_w8(x, q, s), ref, 1e-2, 0.02, f"gemm_w8 {M}x{N}x{K}")
        close(ops.gemm_w8(x, q, s, residual=r), ref + r.double(), 1e-2, 0.03, f"gemm_w8 {M}x{N}x{K} residual")
        close(ops.gemm_w8(x, q, s, out_f32=True), ref, 1e-4, 2e-3, f"gemm_w8 {M}x{N}x{K} f32")
        close(ops.gemm_w8(x, wide[:, 32:32 + K], s), ref, 1e-2, 0.02, f"gemm_w8 {M}x{N}x{K} strided")
        del ref
    quantised.cache_clear()


# ------------------------------------------------------------------ b. bit for bit against the bf16 split-K kernels
ROWS_B = (17, 32, 64, 512)


@pytest.mark.parametrize("NK", SHAPES)
def test_gemm_w8_equals_the_bf16_split_k_kernel_on_pow2_scales(ops, NK):
    """Scaling by a power of two commutes with every rounding, so the same K order gives the same bits: a slip in the slices, the tile
    order, the byte order inside a fragment or the place of the scale shows."""
    N, K = NK
    q, s, wd = quantised_pow2(N, K, 21)
    for M in ((17,) if N == 128256 else ROWS_B):
        x, r = rnd(M, K, seed=3, scale=0.5).to(DEV), rnd(M, N, seed=5).to(DEV)
        assert torch.equal(ops.gemm_w8(x, q, s, residual=r), ops.gemm_splitk(x, wd, residual=r)), (M, N, K, "residual")
        assert torch.equal(ops.gemm_w8(x, q, s), ops.gemm_splitk(x, wd)), (M, N, K)
    quantised_pow2.cache_clear()


@pytest.mark.parametrize("NK", [(4096, 4096), (4096, 14336), (136, 512)])
def test_gemm_w8_norm_equals_gemm_splitk_norm(ops, NK):
    N, K = NK
    q, s, wd = quantised_pow2(N, K, 22)
    nw = (1.0 + 0.1 * rnd(N, seed=4).float()).bfloat16().to(DEV)
    for M in ROWS_B:
        x, r = rnd(M, K, seed=3, scale=0.5).to(DEV), rnd(M, N, seed=5).to(DEV)
        for res in (r, None):
            c8, y8 = ops.gemm_w8_norm(x, q, s, nw, 1e-5, residual=res)
            c, y = ops.gemm_splitk_norm(x, wd, nw, 1e-5, residual=res)
            assert torch.equal(c8, c) and torch.equal(y8, y), (M, N, K, res is not None)
    quantised_pow2.cache_clear()


@pytest.mark.parametrize("IK", [(14336, 4096), (64, 512)])
def test_gemm_w8_swiglu_equals_gemm_splitk_swiglu(ops, IK):
    I, K = IK
    q, s, wd = quantised_pow2(2 * I, K, 23)
    for M in ROWS_B:
        x = rnd(M, K, seed=3, scale=0.5).to(DEV)
        assert torch.equal(ops.gemm_w8_swiglu(x, q, s, I), ops.gemm_splitk_swiglu(x, wd, I)), (M, I, K)
    quantised_pow2.cache_clear()


@pytest.mark.parametrize("geo", [(32, 8, 128, 4096), (2, 1, 32, 512)])
def test_gemm_w8_rope_append_equals_gemm_splitk_rope_append(ops, geo):
    Hq, Hkv, d, K = geo
    N, Lmax = (Hq + 2 * Hkv) * d, 12
    q, s, wd = quantised_pow2(N, K, 24)
    cos, sin = ops.rope_table(Lmax, d, 10000.0, DEV)
    for M in ROWS_B:
        x = rnd(M, K, seed=7, scale=0.5).to(DEV)
        pos = torch.tensor([(7 * m + 3) % Lmax for m in range(M)], dtype=torch.int32, device=DEV)
        k0, v0 = rnd(M, Lmax, Hkv * d, seed=9).to(DEV), rnd(M, Lmax, Hkv * d, seed=10).to(DEV)
        k1, v1 = k0.clone(), v0.clone()
        want = ops.gemm_splitk_rope_append(x, wd, Hq, Hkv, d, cos, sin, pos, k0, v0)
        got = ops.gemm_w8_rope_append(x, q, s, Hq, Hkv, d, cos, sin, pos, k1, v1)
        assert torch.equal(got[:, :Hq * d], want[:, :Hq * d]), ("q rows", M, geo)
        assert torch.equal(k1, k0) and torch.equal(v1, v0), ("cache rows", M, geo)
    quantised_pow2.cache_clear()


# ------------------------------------------------------------------ c. every byte
@pytest.mark.parametrize("M", [17, 64])
def test_gemm_w8_decodes_every_byte_exactly(ops, M):
    """A 256-column weight row holding every encoding (the two NaNs replaced by zero), one-hot x rows: the fp32 output is float(e4m3) *
    scale exactly.  17 rows: the 32-row tile, 64 rows: the 64-row tile."""
    enc = torch.arange(256, dtype=torch.uint8)
    enc[0x7f] = 0
    enc[0xff] = 0
    q = torch.stack([enc, enc.flip(0), enc.roll(37), enc.roll(-101), enc.roll(5)], 0).contiguous()
    s = torch.tensor([1.0, 0.37, 2.0 ** -9, 3.0, 1.7e-3])
    val = q.view(torch.float8_e4m3fn).float()
    qd, sd = q.to(DEV), s.to(DEV)
    for c0 in range(0, 256, M):
        cols = [(c0 + m) % 256 for m in range(M)]
        x = torch.zeros(M, 256, dtype=torch.bfloat16)
        for m, c in enumerate(cols):
            x[m, c] = 1.0
        out = ops.gemm_w8(x.to(DEV), qd, sd, out_f32=True).cpu()
        want = (val[:, cols] * s[:, None]).t()
        assert torch.equal(out, want), (M, c0)


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


@pytest.fixture(scope="module")
def split_model():
    """A released quantised model (power-of-two scales, lm_head too) whose four projections the split-K GEMM splits at 17 .. 64 rows:
    h = 1024, I = 2048 -- q|k|v 1536 x 1024, o 1024 x 1024, gate|up 4096 x 1024, down 1024 x 2048."""
    from metamorph_amd import ops as o
    cfg = tiny_cfg(hidden_size=1024, intermediate_size=2048, num_attention_heads=8, num_key_value_heads=2)
    model = hip_model(cfg, init_state_dict(cfg, seed=5, dtype=torch.bfloat16)).eval()
    model.quantize_decoder_(pow2_scales=True, lm_head=True)
    for rows in (20, 21, 40):
        for (N, K) in ((1536, 1024), (1024, 1024), (4096, 1024), (1024, 2048)):
            assert o.gemm_splitk_splits(rows, N, K), (rows, N, K)
    return cfg, model


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


def _embeds(B, L, h, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, L, h, generator=g) * 0.5).bfloat16().to(DEV)


# ------------------------------------------------------------------ d. routes
def test_wide_steps_prompt_pass_and_lm_head_dequantise_nothing(split_model, monkeypatch):
    from metamorph_amd import functional as F, ops as o
    cfg, a = split_model

    def refuse(*args, **kw):
        raise AssertionError("ops.dequant_w8 was called: a route that has a w8 kernel dequantised a projection")
    monkeypatch.setattr(o, "dequant_w8", refuse)
    a.model.layers[0].w8.scratch.bufs = None                     # (another test may have forced the scratch route on this model)
    assert 21 <= F.PROMPT_GU_SPLITK_ROWS
    with torch.no_grad():
        for B in (20, 40):
            emb = _embeds(B, 22, cfg.hidden_size, seed=B)
            cache, meta, cos, sin, last = _prefill(a, cfg, [emb[i, :21] for i in range(B)], 30)      # B one-sequence prompt passes of 21 rows
            y = F.decoder_decode_row(emb[:, 21].contiguous(), a.model.layers, meta, cache, cos, sin)
            assert y.shape == (B, cfg.hidden_size) and bool(torch.isfinite(y.float()).all())
            assert cache.lengths == [22] * B
        logits = a._rows_logits(last[:20].contiguous())
        assert logits.shape == (20, cfg.vocab_size) and logits.dtype == torch.float32 and bool(torch.isfinite(logits).all())
    torch.cuda.synchronize()
    assert a.model.layers[0].w8.scratch.bufs is None


# ------------------------------------------------------------------ e. against the scratch route
def test_wide_w8_step_equals_the_scratch_route_on_pow2_scales(split_model):
    from metamorph_amd import functional as F
    cfg, a = split_model
    B = 20
    emb = _embeds(B, 23, cfg.hidden_size, seed=7)
    with torch.no_grad():
        c1, meta, cos, sin, _ = _prefill(a, cfg, [emb[i, :21] for i in range(B)], 30)
        c2, _, _, _, _ = _prefill(a, cfg, [emb[i, :21] for i in range(B)], 30)
        assert torch.equal(c1.k[:, :, :21], c2.k[:, :, :21]) and torch.equal(c1.v[:, :, :21], c2.v[:, :, :21])   # (rows beyond: never written)
        for t in (21, 22):
            rows = emb[:, t].contiguous()
            y8 = F.decoder_decode_row(rows, a.model.layers, meta, c1, cos, sin)
            old = F.set_variant("w8_gemm", False)
            try:
                ys = F.decoder_decode_row(rows, a.model.layers, meta, c2, cos, sin)
            finally:
                F.set_variant("w8_gemm", old)
            assert torch.equal(y8, ys), t
        assert torch.equal(c1.k[:, :, :23], c2.k[:, :, :23]) and torch.equal(c1.v[:, :, :23], c2.v[:, :, :23])
    assert a.model.layers[0].w8.scratch.bufs is not None          # (the forced route did dequantise)


# ------------------------------------------------------------------ f. graph replay
def test_wide_w8_step_graph_replay_equals_eager(split_model):
    from metamorph_amd import functional as F
    cfg, a = split_model
    B, h = 20, cfg.hidden_size
    emb = _embeds(B, 30, h, seed=8)
    with torch.no_grad():
        c1, meta, cos, sin, _ = _prefill(a, cfg, [emb[i, :21] for i in range(B)], 40)
        c2, _, _, _, _ = _prefill(a, cfg, [emb[i, :21] for i in range(B)], 40)
        stepper = F.DecodeStepGraph(a.model.layers, meta, c2, cos, sin, h, DEV)
        assert stepper.graph is not None
        for t in range(21, 29):
            rows = emb[:, t].contiguous()
            eager = F.decoder_decode_row(rows, a.model.layers, meta, c1, cos, sin)
            assert torch.equal(stepper.step(rows), eager), t
        assert torch.equal(c1.k[:, :, :29], c2.k[:, :, :29]) and torch.equal(c1.v[:, :, :29], c2.v[:, :, :29])


# ------------------------------------------------------------------ g. the single-slice store on a ragged window
@pytest.mark.parametrize("M", [19, 70])
def test_gemm_w8_single_slice_store_on_a_ragged_window(ops, M):
    """N = 523 into the first columns of an [M, 528] buffer, residual rows 528 apart: gemm_epilogue's 16-byte body on columns [0, 520) and its
    scalar body on the last three, from the 32-row tile (M = 19) and the 64-row tile (M = 70), for bf16 and fp32 output, with and without
    the residual.  N % 8 != 0 is never split (the workspace query says so), so the store under test is the one that ran.  Against the fp64
    product of the dequantised weight under the derived bound of tests/gemm_epilogue_refs.py; the allocation is prefilled with a canary NaN:
    every element of the window is written, nothing outside it."""
    import gemm_epilogue_refs as E
    from metamorph_amd import lib
    N, K = 523, 256
    assert int(lib.load().mm355_gemm_w8_ws_floats(M, N, K)) == 0
    geo = E.Geometry("w8", M, N, 528, 0, 0, 528)
    q, s, wd = quantised(N, K, 31)
    x, r = rnd(M, K, seed=1, scale=0.5).to(DEV), rnd(M, N, seed=4).to(DEV)
    accb = E.accumulation_bound(x, wd)
    for with_res in (False, True):
        ref = x.double() @ wd.t() + (r.double() if with_res else 0.0)
        for out_f32 in (False, True):
            what = f"gemm_w8 {M}x{N}x{K} {'fp32' if out_f32 else 'bf16'}{' residual' if with_res else ''}"
            alloc, view = E.canary_out(geo, torch.float32 if out_f32 else torch.bfloat16, DEV)
            ops.gemm_w8(x, q, s, residual=E.residual_view(r, geo) if with_res else None, out=view)
            E.check_untouched(alloc, geo, what)
            worst = E.check(view, ref, E.epilogue_bound(ref, accb, None, out_f32), what, E.column_classes(geo, with_res))
            print(f"{what}: largest |error| / bound {worst:.3f}")
    quantised.cache_clear()
