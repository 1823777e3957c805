"""The weight-only MXFP4 split-K GEMM on the device (mm355_gemm_w4*).  Every dequantised MXFP4 value is exactly a bf16 value and the group
scale sits inside the widening conversion, so the kernel must return the BITS of the bf16 split-K kernels on the dequantised weight, for
any scales (a); besides: against the fp64 evaluation of the format's contract (b), every e2m1 code under extreme group scales (c), and the
routes of a model quantised with quantize_decoder_(fmt="mxfp4"): steps of more than 16 sequences, one-sequence prompt passes and
decoder_extend run on the nibbles and dequantise nothing (d), equal the scratch route bit for bit (e), replay in a captured graph (f) and
give generate() the same tokens (g)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.ref_model import OracleConfig, init_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (N, K) -> K slices at 17 .. 100 rows: not split (one slice, N tail), two slices, 17 K tiles in uneven slices of 9 + 8, four slices
SHAPES = {(136, 512): 1, (136, 1024): 2, (264, 1088): 2, (520, 2048): 4}
ROWS = (17, 32, 33, 64, 100)                                     # the 32-row tile, its edge, the 64-row tile, a row tail in two tiles


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
    """tests/test_w4_gpu.py's helper: a weight whose GROUPS of 32 span magnitudes 2^-12 .. 2^3 within every row (so do its group scales): a
    scale index that slips by one group, a forgotten scale or one taken from the neighbouring row fails.  -> (q, s, fp64 dequantised
    weight), computed once per shape."""
    from metamorph_amd import ops as o
    g = torch.Generator().manual_seed(seed)
    mag = 2.0 ** (torch.rand(N, K // 32, generator=g) * 15 - 12)
    w = (torch.randn(N, K // 32, 32, generator=g) * 0.3 * mag[:, :, None]).view(N, K).bfloat16()
    q, s = o.quantize_w4(w)
    return q, s, o.dequant_w4_reference(q, s).double()


@functools.lru_cache(maxsize=None)
def on_device(N, K, seed):
    """-> (q, s, the dequantised bf16 weight as mm355_dequant_w4_bf16 writes it), on the device; the group scales are ordinary ones."""
    from metamorph_amd import ops as o
    q, s, wd = quantised(N, K, seed)
    assert len(set(s.flatten().tolist())) > 8                    # (many different group scales, none of them special)
    q, s = q.to(DEV), s.to(DEV)
    w = o.dequant_w4(q, s)
    assert torch.equal(w.double().cpu(), wd)
    return q, s, w


def slices_of(ops, M, N, K):
    """K slices of the split-K rule for this problem (1: not split), from the workspace the bf16 form asks for"""
    from metamorph_amd import lib
    n = int(lib.load().mm355_gemm_splitk_ws_floats(M, N, K)) // (M * N) or 1
    assert ops.gemm_splitk_splits(M, N, K) == (n > 1)
    return n


# ------------------------------------------------------------------ a. bit for bit against the bf16 twin
@pytest.mark.parametrize("NK", list(SHAPES))
def test_gemm_w4_equals_the_bf16_split_k_kernel(ops, NK):
    """The same slices, tiles, MFMA order and fragments: the same bits, with and without residual.  A slip in the slices, the tile order, the
    nibble order inside a fragment or the scale group shows."""
    N, K = NK
    q, s, w = on_device(N, K, 21)
    for M in ROWS:
        assert slices_of(ops, M, N, K) == SHAPES[NK], (M, N, K)
        x, r = rnd(M, K, seed=3, scale=0.5).to(DEV), rnd(M, N, seed=5).to(DEV)
        assert torch.equal(ops.gemm_w4(x, q, s), ops.gemm_splitk(x, w)), (M, N, K)
        assert torch.equal(ops.gemm_w4(x, q, s, residual=r), ops.gemm_splitk(x, w, residual=r)), (M, N, K, "residual")


@pytest.mark.parametrize("NK", list(SHAPES))
def test_gemm_w4_norm_equals_gemm_splitk_norm(ops, NK):
    N, K = NK
    q, s, w = on_device(N, K, 22)
    nw = (1.0 + 0.1 * rnd(N, seed=4).float()).bfloat16().to(DEV)
    for M in ROWS:
        x, r = rnd(M, K, seed=3, scale=0.5).to(DEV), rnd(M, N, seed=5).to(DEV)
        for res in (r, None):
            c4, y4 = ops.gemm_w4_norm(x, q, s, nw, 1e-5, residual=res)
            c, y = ops.gemm_splitk_norm(x, w, nw, 1e-5, residual=res)
            assert torch.equal(c4, c) and torch.equal(y4, y), (M, N, K, res is not None)


@pytest.mark.parametrize("I", [68, 260])
def test_gemm_w4_swiglu_equals_gemm_splitk_swiglu(ops, I):
    K = 1024
    q, s, w = on_device(2 * I, K, 23)
    for M in ROWS:
        assert slices_of(ops, M, 2 * I, K) == 2
        x = rnd(M, K, seed=3, scale=0.5).to(DEV)
        assert torch.equal(ops.gemm_w4_swiglu(x, q, s, I), ops.gemm_splitk_swiglu(x, w, I)), (M, I, K)


def test_swiglu_reduce_of_unaligned_rows_equals_the_vector_reduce(ops):
    """I = 68 and 260 are no multiples of 8: their reduce launch writes one output per thread.  That launch against the 16-byte one on a shape
    both take (I = 72; act rows 76 apart select the former): the same bits, for the w4 and the bf16 form."""
    from metamorph_amd import lib
    L = lib.load()
    I, K, ld = 72, 1024, 76
    q, s, w = on_device(2 * I, K, 25)
    for M in (17, 100):
        assert slices_of(ops, M, 2 * I, K) == 2
        x = rnd(M, K, seed=3, scale=0.5).to(DEV)
        want = ops.gemm_w4_swiglu(x, q, s, I)
        n_ws = int(L.mm355_gemm_w4_swiglu_ws_floats(M, I, K))
        ws = torch.empty(n_ws, device=DEV, dtype=torch.float32)
        for form in ("w4", "bf16"):
            wide = torch.zeros(M, ld, device=DEV, dtype=torch.bfloat16)
            if form == "w4":
                rc = L.mm355_gemm_w4_swiglu(x.data_ptr(), K, q.data_ptr(), K // 2, s.data_ptr(), K // 32, ops.W4_MXFP4, wide.data_ptr(), ld, M, I, K,
                                            ws.data_ptr(), n_ws, torch.cuda.current_stream().cuda_stream)
            else:
                rc = L.mm355_gemm_splitk_swiglu_bf16(x.data_ptr(), K, w.data_ptr(), K, wide.data_ptr(), ld, M, I, K, ws.data_ptr(), n_ws,
                                                     torch.cuda.current_stream().cuda_stream)
            assert rc == 0, (form, rc)
            assert torch.equal(wide[:, :I], want) and not bool(wide[:, I:].any()), (form, M)


@pytest.mark.parametrize("geo", [(2, 1, 32, 1024), (4, 2, 64, 1088)])
def test_gemm_w4_rope_append_equals_gemm_splitk_rope_append(ops, geo):
    Hq, Hkv, d, K = geo
    N, Lmax = (Hq + 2 * Hkv) * d, 12
    q, s, w = on_device(N, K, 24)
    cos, sin = ops.rope_table(Lmax, d, 10000.0, DEV)
    for M in ROWS:
        assert slices_of(ops, M, N, K) == 2
        x = rnd(M, K, seed=7, scale=0.5).to(DEV)
        pos = torch.tensor([(7 * m + 3) % Lmax for m in range(M)], dtype=torch.int32, device=DEV)
        k0, v0 = rnd(M, Lmax, Hkv * d, seed=9).to(DEV), rnd(M, Lmax, Hkv * d, seed=10).to(DEV)
        k1, v1 = k0.clone(), v0.clone()
        want = ops.gemm_splitk_rope_append(x, w, Hq, Hkv, d, cos, sin, pos, k0, v0)
        got = ops.gemm_w4_rope_append(x, q, s, Hq, Hkv, d, cos, sin, pos, k1, v1)
        assert torch.equal(got[:, :Hq * d], want[:, :Hq * d]), ("q rows", M, geo)
        assert torch.equal(k1, k0) and torch.equal(v1, v0), ("cache rows", M, geo)


# ------------------------------------------------------------------ b. against fp64
@pytest.mark.parametrize("NK", list(SHAPES))
def test_gemm_w4_against_fp64(ops, NK):
    """test_gemv_w4's bars for bf16 output and test_gemm_w8_against_fp64's for fp32 output (exact products summed in fp32: the fp64
    reference differs by the summation order only); weight and scale rows strided (ldw_bytes > K / 2, lds_bytes > K / 32, the latter odd).
    The fp32 output runs as ONE slice also where the bf16 output is split ((136, 1024) among them)."""
    N, K = NK
    q, s, wd = quantised(N, K, 2)
    wide = torch.zeros(N, K // 2 + 64, dtype=torch.uint8)
    wide[:, 32:32 + K // 2] = q
    swide = torch.full((N, K // 32 + 7), 200, dtype=torch.uint8)
    swide[:, 3:3 + K // 32] = s
    assert swide.stride(0) % 2 == 1
    qs, ss = wide.to(DEV)[:, 32:32 + K // 2], swide.to(DEV)[:, 3:3 + K // 32]
    qd, sd = q.to(DEV), s.to(DEV)
    for M in ROWS:
        x, r = rnd(M, K, seed=1, scale=0.5), rnd(M, N, seed=4)
        ref = x.double() @ wd.t()
        xd = x.to(DEV)
        close(ops.gemm_w4(xd, qd, sd), ref, 1e-2, 0.02, f"gemm_w4 {M}x{N}x{K}")
        close(ops.gemm_w4(xd, qs, ss), ref, 1e-2, 0.02, f"gemm_w4 {M}x{N}x{K} strided")
        close(ops.gemm_w4(xd, qs, ss, residual=r.to(DEV)), ref + r.double(), 1e-2, 0.03, f"gemm_w4 {M}x{N}x{K} strided, residual")
        close(ops.gemm_w4(xd, qs, ss, out_f32=True), ref, 1e-4, 2e-3, f"gemm_w4 {M}x{N}x{K} strided, f32")
        assert torch.equal(ops.gemm_w4(xd, qs, ss), ops.gemm_w4(xd, qd, sd)), (M, N, K, "strides change nothing")


# ------------------------------------------------------------------ c. every code
@pytest.mark.parametrize("M", [17, 64])
def test_gemm_w4_decodes_every_code_exactly(ops, M):
    """16 weight rows of 256 columns, row r holding code (k + r) % 16 at column k: all 16 codes in both halves of every byte position of a
    fragment.  The scale bytes 2, 100, 127 and 252 (2^-125 .. 2^125: the ends of what the format guarantees to be a bf16 value) laid across
    the eight groups of a row, shifted from row to row.  One-hot x rows: the fp32 output is Wd exactly.  17 rows: the 32-row tile, 64 rows:
    the 64-row tile."""
    k = torch.arange(256)
    code = (k[None, :] + torch.arange(16)[:, None]) % 16
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8).contiguous()
    for b in range(128):                                         # every nibble value in both halves of a byte
        assert set((q[:, b] & 15).tolist()) == set(range(16)) and set((q[:, b] >> 4).tolist()) == set(range(16))
    sset = torch.tensor([2, 100, 127, 252], dtype=torch.uint8)
    s = sset[(torch.arange(8)[None, :] + torch.arange(16)[:, None]) % 4].contiguous()
    val = ops.dequant_w4_reference(q, s)
    assert bool(torch.isfinite(val).all()) and torch.equal(val.bfloat16().float(), val) and float(val.abs().max()) == 6.0 * 2.0 ** 125
    assert float(val[val != 0].abs().min()) == 0.5 * 2.0 ** -125
    qd, sd = q.to(DEV), s.to(DEV)
    for c0 in range(0, 256, M):
        cols = [(c0 + m) % 256 for m in range(M)]
        x = torch.zeros(M, 256, dtype=torch.bfloat16)
        for m, c in enumerate(cols):
            x[m, c] = 1.0
        out = ops.gemm_w4(x.to(DEV), qd, sd, out_f32=True).cpu()
        want = val[:, cols].t()
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
    """A released "mxfp4" model whose four projections the split-K GEMM splits at 5 .. 64 rows (the geometry of
    tests/test_w8_gemm_gpu.py::split_model): h = 1024, I = 2048 -- q|k|v 1536 x 1024, o 1024 x 1024, gate|up 4096 x 1024, down 1024 x 2048."""
    from metamorph_amd import functional as F, ops as o
    cfg = tiny_cfg(hidden_size=1024, intermediate_size=2048, num_attention_heads=8, num_key_value_heads=2)
    model = hip_model(cfg, init_state_dict(cfg, seed=5, dtype=torch.bfloat16)).eval()
    model.quantize_decoder_(fmt="mxfp4")
    assert all(isinstance(l.w8, F.W4Layer) and l.w8.released for l in model.model.layers)
    for rows in (5, 20, 21, 40):
        for (N, K) in ((1536, 1024), (1024, 1024), (4096, 1024), (1024, 2048)):
            assert o.gemm_splitk_splits(rows, N, K), (rows, N, K)
    return cfg, model


@pytest.fixture
def caps(monkeypatch):
    """The routing under test: every split projection on the w4 GEMM up to its 4096 rows, unsplit ones on the scratch route."""
    from metamorph_amd import functional as F
    monkeypatch.setattr(F, "W4_GEMM_MAX_ROWS", {n: 4096 for n in F.W8Layer.NAMES})
    monkeypatch.setattr(F, "W4_GEMM_UNSPLIT_MAX_ROWS", {n: 0 for n in F.W8Layer.NAMES})
    monkeypatch.setitem(F.VARIANTS, "w4_gemm", True)


def _meta(model, L, cos, sin):
    _, m = model._decode_meta(L)
    m.cos, m.sin = cos, sin
    return m


def _prefill(model, cfg, seqs, cap, fmt="bf16"):
    """seqs: one [L_b, h] prompt per sequence -> (cache, meta, cos, sin, last hidden row per sequence [B, h])"""
    from metamorph_amd import functional as F
    B = len(seqs)
    cos, sin = model.model.rope_tables(cap, DEV)
    meta = _meta(model, max(s.shape[0] for s in seqs), cos, sin)
    cache = F.KVCache(cfg.num_hidden_layers, cap, meta.Hkv * meta.d, DEV, Hq=meta.Hq, d=meta.d, batch=B, fmt=fmt)
    last = []
    for b, s in enumerate(seqs):
        last.append(F.decoder_prefill(s.contiguous(), model.model.layers, _meta(model, s.shape[0], cos, sin), cache, row=b)[-1:])
    return cache, meta, cos, sin, torch.cat(last, 0).contiguous()


def _embeds(B, L, h, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, L, h, generator=g) * 0.5).bfloat16().to(DEV)


def _same_cache(c1, c2, rows):
    for name in ("k", "v", "k_scale", "v_scale"):
        t1, t2 = getattr(c1, name, None), getattr(c2, name, None)
        if t1 is not None:
            assert torch.equal(t1[:, :, :rows], t2[:, :, :rows]), name


def _without_w4_gemm(fn):
    from metamorph_amd import functional as F
    old = F.set_variant("w4_gemm", False)
    try:
        return fn()
    finally:
        F.set_variant("w4_gemm", old)


# ------------------------------------------------------------------ d. routes
def test_wide_steps_prompt_passes_and_extend_dequantise_nothing(split_model, caps, monkeypatch):
    from metamorph_amd import functional as F, ops as o
    cfg, a = split_model

    def refuse(*args, **kw):
        raise AssertionError("dequant_w4 was called: a route that has a w4 kernel dequantised a projection")
    monkeypatch.setattr(o, "dequant_w4", refuse)
    monkeypatch.setattr(F.W4Layer, "dequant", staticmethod(refuse))   # (the record's own handle on it)
    a.model.layers[0].w8.scratch.bufs = None                     # (another test may have forced the scratch route on this model)
    assert 21 <= F.PROMPT_GU_SPLITK_ROWS
    assert F.w8_on_gemm(a.model.layers[0], 20) == frozenset(F.W8Layer.NAMES)
    with torch.no_grad():
        for B in (20, 40):
            emb = _embeds(B, 22, cfg.hidden_size, seed=B)
            cache, meta, cos, sin, last = _prefill(a, cfg, [emb[i, :21] for i in range(B)], 30)      # B one-sequence prompt passes of 21 rows
            assert bool(torch.isfinite(last.float()).all())
            y = F.decoder_decode_row(emb[:, 21].contiguous(), a.model.layers, meta, cache, cos, sin)
            assert y.shape == (B, cfg.hidden_size) and bool(torch.isfinite(y.float()).all())
            assert cache.lengths == [22] * B
        emb = _embeds(1, 26, cfg.hidden_size, seed=3)
        cache, meta, cos, sin, _ = _prefill(a, cfg, [emb[0, :21]], 30)
        rows = F.decoder_extend(emb[0, 21:26].contiguous(), a.model.layers, _meta(a, 1, cos, sin), cache)
        assert rows.shape == (5, cfg.hidden_size) and bool(torch.isfinite(rows.float()).all())
        assert cache.lengths == [26]
    torch.cuda.synchronize()
    assert a.model.layers[0].w8.scratch.bufs is None


# ------------------------------------------------------------------ e. against the scratch route
@pytest.mark.parametrize("kv", ["bf16", "fp8_e4m3"])
def test_wide_w4_step_equals_the_scratch_route(split_model, caps, kv):
    """The dequantisation is exact and the K order that of the bf16 kernel: the same bits, whatever the scales.  A wrong K order, nibble
    order or scale group shows here."""
    from metamorph_amd import functional as F
    cfg, a = split_model
    B = 20
    emb = _embeds(B, 23, cfg.hidden_size, seed=7)
    with torch.no_grad():
        c1, meta, cos, sin, _ = _prefill(a, cfg, [emb[i, :21] for i in range(B)], 30, fmt=kv)
        c2 = _without_w4_gemm(lambda: _prefill(a, cfg, [emb[i, :21] for i in range(B)], 30, fmt=kv)[0])
        _same_cache(c1, c2, 21)                                  # (rows beyond: never written) -- the prompt passes agree too
        for t in (21, 22):
            rows = emb[:, t].contiguous()
            y4 = F.decoder_decode_row(rows, a.model.layers, meta, c1, cos, sin)
            ys = _without_w4_gemm(lambda: F.decoder_decode_row(rows, a.model.layers, meta, c2, cos, sin))
            assert torch.equal(y4, ys), t
        _same_cache(c1, c2, 23)
    assert a.model.layers[0].w8.scratch.bufs is not None          # (the forced route did dequantise)


def test_w4_extend_pass_equals_the_scratch_route(split_model, caps):
    from metamorph_amd import functional as F
    cfg, a = split_model
    emb = _embeds(1, 26, cfg.hidden_size, seed=11)
    with torch.no_grad():
        c1, _, cos, sin, _ = _prefill(a, cfg, [emb[0, :21]], 30)
        c2 = _prefill(a, cfg, [emb[0, :21]], 30)[0]
        new = emb[0, 21:26].contiguous()
        r4 = F.decoder_extend(new, a.model.layers, _meta(a, 1, cos, sin), c1)
        rs = _without_w4_gemm(lambda: F.decoder_extend(new, a.model.layers, _meta(a, 1, cos, sin), c2))
        assert torch.equal(r4, rs) and c1.lengths == c2.lengths == [26]
        _same_cache(c1, c2, 26)


# ------------------------------------------------------------------ f. graph replay
def test_wide_w4_step_graph_replay_equals_eager(split_model, caps):
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
        _same_cache(c1, c2, 29)


# ------------------------------------------------------------------ g. generate()
def test_hf_generate_of_20_prompts_gives_the_same_tokens_on_either_route(split_model, caps):
    cfg, a = split_model
    ids = torch.randint(0, 127000, (20, 11), generator=torch.Generator().manual_seed(9)).to(DEV)
    kw = dict(inputs=ids, use_customize_greedy=False, do_sample=False, max_new_tokens=6, eos_token_id=None, pad_token_id=0)
    with torch.no_grad():
        on = a.generate(**kw)
        off = _without_w4_gemm(lambda: a.generate(**kw))
    assert on.shape[0] == 20 and on.shape[1] >= 6 and on.tolist() == off.tolist()


# ------------------------------------------------------------------ h. the single-slice store on a ragged window
@pytest.mark.parametrize("M", [19, 70])
def test_gemm_w4_single_slice_store_on_a_ragged_window(ops, M):
    """N = 523 into the first columns of an [M, 528] buffer, residual rows 528 apart: gemm_epilogue's 16-byte body on columns [0, 520) and its
    scalar body on the last three, from the 32-row tile (M = 19) and the 64-row tile (M = 70), for bf16 and fp32 output, with and without
    the residual.  N % 8 != 0 is never split (the workspace query says so), so the store under test is the one that ran.  Against the fp64
    product of the dequantised weight under the derived bound of tests/gemm_epilogue_refs.py; the allocation is prefilled with a canary NaN:
    every element of the window is written, nothing outside it."""
    import gemm_epilogue_refs as E
    from metamorph_amd import lib
    N, K = 523, 256
    assert int(lib.load().mm355_gemm_w4_ws_floats(M, N, K)) == 0
    geo = E.Geometry("w4", M, N, 528, 0, 0, 528)
    q, s, wd = quantised(N, K, 31)
    qd, sd, wd = q.to(DEV), s.to(DEV), wd.to(DEV)
    x, r = rnd(M, K, seed=1, scale=0.5).to(DEV), rnd(M, N, seed=4).to(DEV)
    accb = E.accumulation_bound(x, wd)
    for with_res in (False, True):
        ref = x.double() @ wd.t() + (r.double() if with_res else 0.0)
        for out_f32 in (False, True):
            what = f"gemm_w4 {M}x{N}x{K} {'fp32' if out_f32 else 'bf16'}{' residual' if with_res else ''}"
            alloc, view = E.canary_out(geo, torch.float32 if out_f32 else torch.bfloat16, DEV)
            ops.gemm_w4(x, qd, sd, residual=E.residual_view(r, geo) if with_res else None, out=view)
            E.check_untouched(alloc, geo, what)
            worst = E.check(view, ref, E.epilogue_bound(ref, accb, None, out_f32), what, E.column_classes(geo, with_res))
            print(f"{what}: largest |error| / bound {worst:.3f}")
