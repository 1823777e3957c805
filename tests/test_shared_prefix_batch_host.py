"""A batch of prompts over one prefix cache, the parts that need no GPU: the C ABI's symbols, the workspace size and the refusals of
mm355_attn_extend_shared / _f8 by return code; the refusals of functional.decoder_extend_shared, greedy_decode(shared_prefix_rows=...) and
generate() by name; generate()'s routing of the keyword; the prefix finder on CPU tensors."""
import ctypes
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mm355_attn_extend_shared_ws_floats", "mm355_attn_extend_shared", "mm355_attn_extend_shared_f8")
BF16 = torch.bfloat16


def test_extend_shared_symbols_workspace_and_refusals_without_a_gpu():
    from metamorph_amd import build, lib, ops
    names = lib.exported_symbols()
    header = open(os.path.join(REPO, "include", "mm355.h")).read()
    for n in NEW:
        assert n in names and f"{n}(" in header, n
    assert "attn_extend_shared.hip" in build.SOURCES
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(lib.LIB_PATH)
    for n in NEW:
        assert hasattr(so, n), n
    assert hasattr(ops, "attn_extend_shared") and hasattr(ops, "attn_extend_shared_f8")
    L = lib.load()
    P = 4096                                                     # a non-null, 16-byte aligned stand-in: no kernel is launched on the error path
    B, n, Hq, Hkv, d, rows, S = 3, 5, 8, 2, 128, 512, 300
    ld, bs = Hkv * d, rows * Hkv * d
    wsf = L.mm355_attn_extend_shared_ws_floats
    need = wsf(B, n, Hq, Hkv, d, S, rows)
    assert need > 0 and wsf(B, n, Hq, Hkv, d, 0, rows) > 0       # the own partial is always written
    assert wsf(B, n, Hq, Hkv, d, rows + 1, rows) == 0 and wsf(B, n, Hq, Hkv, d, -1, rows) == 0 and wsf(B, 0, Hq, Hkv, d, S, rows) == 0
    assert wsf(B, rows + 1, Hq, Hkv, d, S, rows) == 0
    # positive and monotone in shared_len and in n; a function of the launch arguments alone, never of max_kv_len
    for a, b in zip((0, 1, 64, 65, 300, 1100, 5000), (1, 64, 65, 300, 1100, 5000, 20000)):
        assert 0 < wsf(B, n, Hq, Hkv, d, a, 20000) <= wsf(B, n, Hq, Hkv, d, b, 20000), (a, b)
    for a, b in zip((1, 2, 5, 16, 17, 100), (2, 5, 16, 17, 100, 400)):
        assert 0 < wsf(B, a, Hq, Hkv, d, S, rows) <= wsf(B, b, Hq, Hkv, d, S, rows), (a, b)
    assert wsf(B, 1, Hq, Hkv, d, S, rows) < wsf(B, 400, Hq, Hkv, d, S, rows) and wsf(B, n, Hq, Hkv, d, 1, 20000) < wsf(B, n, Hq, Hkv, d, 5000, 20000)
    assert wsf(B, n, Hq, Hkv, d, S, rows) == wsf(B, n, Hq, Hkv, d, S, 4 * rows)
    # n == 1 is the decode-shared launch: the same key runs, the same workspace
    assert wsf(B, 1, Hq, Hkv, d, S, rows) == L.mm355_attn_decode_shared_ws_floats(B, Hq, Hkv, d, S, rows)

    def bf(q=P, ldq=Hq * d, ksh=P, vsh=P, ldsh=ld, k=P, v=P, ldkv=ld, bskv=bs, past=P, n_=n, S_=S, bound=rows, o=P, ldo=Hq * d, Hq_=Hq, d_=d,
           ws=P, nws=need):
        return L.mm355_attn_extend_shared(q, ldq, ksh, vsh, ldsh, k, v, ldkv, bskv, past, n_, S_, bound, o, ldo, B, Hq_, Hkv, d_, 0.1, ws, nws, 0)

    def f8(fmt=1, ksh=P, kshs=P, vshs=P, ldsh=ld, ldshs=Hkv, k=P, ks=P, vs=P, ldkv=ld, ldsc=Hkv, n_=n, S_=S, d_=d, Hq_=Hq, ws=P, nws=need):
        return L.mm355_attn_extend_shared_f8(P, Hq_ * d, ksh, P, ldsh, kshs, vshs, ldshs, k, P, ldkv, bs, ks, vs, ldsc, rows * Hkv, fmt, P, n_, S_,
                                             rows, P, Hq_ * d, B, Hq_, Hkv, d_, 0.1, ws, nws, 0)
    for null in ("q", "ksh", "vsh", "k", "v", "past", "o"):      # NULL pointers
        assert bf(**{null: 0}) == -1, null
    assert bf(q=P + 2) == -1 and bf(o=P + 8) == -1 and bf(k=P + 8) == -1 and bf(ksh=P + 8) == -1     # misaligned pointers
    assert bf(ldq=Hq * d + 4) == -1 and bf(ldo=Hq * d + 2) == -1 and bf(ldkv=ld + 4) == -1 and bf(bskv=bs + 4) == -1 and bf(ldsh=ld + 4) == -1
    assert bf(ldkv=ld - 8) == -1 and bf(ldsh=ld - 8) == -1       # a row stride shorter than a row
    assert bf(S_=-1) == -1 and bf(S_=rows + 1) == -1             # shared_len outside [0, max_kv_len]
    assert bf(n_=0) == -1 and bf(n_=-3) == -1 and bf(n_=rows + 1) == -1 and bf(n_=7, bound=6, S_=2) == -1     # n outside [1, max_kv_len]
    assert bf(ws=0) == -1 and bf(nws=need - 1) == -1 and bf(ws=P + 4) == -1 and bf(S_=0, ws=0) == -1   # the workspace: missing, short, misaligned
    assert bf(Hq_=5) == -1                                       # Hq % Hkv
    assert bf(d_=124) == -2 and bf(d_=136) == -2                 # d % 8, d > 128
    assert bf(Hq_=6, ldq=6 * d, ldo=6 * d) == -2 and bf(Hq_=32, ldq=32 * d, ldo=32 * d) == -2          # GQA groups of 3 and 16
    assert f8(fmt=7) == -1 and f8(ks=0) == -1 and f8(vs=0) == -1 and f8(kshs=0) == -1 and f8(vshs=0) == -1   # a format that does not exist, NULL scales
    assert f8(k=P + 4) == -1 and f8(ksh=P + 4) == -1 and f8(ldkv=ld + 4) == -1 and f8(ldsh=ld + 4) == -1     # 8-byte cache alignment
    assert f8(ks=P + 2) == -1 and f8(kshs=P + 2) == -1 and f8(ldsc=Hkv - 1) == -1 and f8(ldshs=Hkv - 1) == -1   # 4-byte scales, short scale rows
    assert f8(S_=-1) == -1 and f8(S_=rows + 1) == -1 and f8(ws=0) == -1 and f8(nws=need - 1) == -1 and f8(n_=0) == -1 and f8(n_=rows + 1) == -1
    assert f8(d_=124) == -2 and f8(Hq_=6) == -2
    assert ops.attn_extend_shared_supported(8, 2, 128) and not ops.attn_extend_shared_supported(6, 2, 128)
    assert not ops.attn_extend_shared_supported(8, 2, 136) and not ops.attn_extend_shared_supported(8, 2, 124)


def _tiny_cpu_model():
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
               rms_norm_eps=1e-5, rope_theta=500000.0)
    geo = dict(hidden_size=64, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14)
    return build_model(llm, geo, num_image_tokens=4, max_length=64)


def test_decoder_extend_shared_refusals_name_their_reason():
    from metamorph_amd import functional as F
    assert F.VARIANTS["shared_prefix_min_rows"] >= 1
    meta = F.LayerMeta(1, 8, 2, 1, 32, 128, 1e-5, None, None, None)
    kv = F.KVCache(1, 16, 32, "cpu", Hq=None, d=None, batch=3)
    x = torch.zeros(3, 4, 64, dtype=BF16)
    with torch.no_grad():
        with pytest.raises(ValueError, match="needs a cache with a shared prefix"):
            F.decoder_extend_shared(x, [], meta, kv)
        with pytest.raises(ValueError, match=r"x \[batch, n, h\] with batch = 3"):
            F.decoder_extend_shared(x[:2], [], meta, kv)
        kv.lengths, kv.shared_len = [6, 6, 6], 6                  # (a shared cache without its device parts: the refusals come first)
        with pytest.raises(ValueError, match=r"new rows at \[6, 5, 6\] on a shared prefix of 6 rows"):
            F.decoder_extend_shared(x, [], meta, kv, past=[6, 5, 6])
        with pytest.raises(ValueError, match="capacity of 16 rows is too small for 13 cached \\+ 4 new rows"):
            F.decoder_extend_shared(x, [], meta, kv, past=[6, 13, 6])
    with torch.enable_grad(), pytest.raises(RuntimeError, match="inference pass"):
        F.decoder_extend_shared(x, [], meta, kv)
    assert kv.lengths == [6, 6, 6]


def test_greedy_decode_refuses_bad_shared_prefix_calls_by_name():
    model = _tiny_cpu_model().eval()
    emb = torch.zeros(3, 5, 64, dtype=BF16)

    def call(e=emb, **kw):
        return model.greedy_decode(None, None, e, max_new_tokens=4, **kw)
    for bad in (-1, 2.0, 1.5, "3", "Auto", True, [2]):
        with pytest.raises(ValueError, match="shared_prefix_rows.*non-negative integer or \"auto\""):
            call(shared_prefix_rows=bad)
    for S in (2, "auto"):
        with pytest.raises(ValueError, match="shared_prefix_rows=.*use_cache=False"):
            call(shared_prefix_rows=S, use_cache=False)
        with pytest.raises(ValueError, match="shared_prefix_rows=.*num_return_sequences=3"):
            call(emb[:1], shared_prefix_rows=S, num_return_sequences=3, do_sample=True, temperature=0.7)
    with pytest.raises(ValueError, match="shared_prefix_rows = 5 leaves a sequence of 5 rows no row of its own \\(at most 4"):
        call(shared_prefix_rows=5)
    mask = torch.ones(3, 5, dtype=torch.long)
    mask[1, :2] = 0                                              # sequence 1 holds 3 rows: at most 2 are shared
    with pytest.raises(ValueError, match="shared_prefix_rows = 3 leaves a sequence of 3 rows"):
        model.greedy_decode(None, mask, emb, max_new_tokens=4, shared_prefix_rows=3)
    with pytest.raises(ValueError, match="shared_prefix_rows = 5 leaves"):          # one prompt: validated all the same
        call(emb[:1], shared_prefix_rows=5)
    broken = emb.clone()
    broken[2, 1, 7] = 1.0
    with pytest.raises(ValueError, match="shared_prefix_rows = 3, but sequence 2 differs from sequence 0 at row 1"):
        call(broken, shared_prefix_rows=3)


def test_generate_routes_the_keyword_and_refuses_the_two_other_routes(monkeypatch):
    model = _tiny_cpu_model().eval()
    seen = {}

    def fake(**kw):
        seen.update(kw)
        return "routed"
    monkeypatch.setattr(model, "greedy_decode", fake)
    embed = model.get_model().embed_tokens                       # (the embedding gather is a HIP kernel: stand in for it on the CPU)
    monkeypatch.setattr(type(embed), "forward", lambda self, i: torch.zeros(tuple(i.shape) + (64,), dtype=BF16))
    ids = torch.zeros(2, 5, dtype=torch.long)
    assert model.generate(inputs=ids, shared_prefix_rows=3, max_new_tokens=2) == "routed"
    assert seen["shared_prefix_rows"] == 3 and seen["max_new_tokens"] == 2 and tuple(seen["inputs_embeds"].shape) == (2, 5, 64)
    seen.clear()
    assert model.generate(inputs=ids, shared_prefix_rows="auto") == "routed" and seen["shared_prefix_rows"] == "auto"
    seen.clear()
    assert model.generate(inputs=ids, shared_prefix_rows=None) == "routed" and "shared_prefix_rows" not in seen
    with pytest.raises(ValueError, match="shared_prefix_rows=3.*use_customize_greedy=False"):
        model.generate(inputs=ids, shared_prefix_rows=3, use_customize_greedy=False)
    with pytest.raises(ValueError, match="shared_prefix_rows='auto'.*device_beam_search=True"):
        model.generate(inputs=ids, shared_prefix_rows="auto", device_beam_search=True, num_beams=2)


def test_the_prefix_finder_on_cpu_tensors(monkeypatch):
    from metamorph_amd import functional as F
    from metamorph_amd.model.language_model.metamorph_llama import MetaMorphLlamaForCausalLM as M
    assert F.VARIANTS["shared_prefix_min_rows"] == 512            # (the measured default; the finder itself from 1 row on)
    monkeypatch.setitem(F.VARIANTS, "shared_prefix_min_rows", 1)
    g = torch.Generator().manual_seed(3)
    B, n, h = 4, 12, 16
    base = torch.randn(n, h, generator=g).bfloat16()
    same = base[None].repeat(B, 1, 1)
    none = [0] * B
    assert M._first_differing_rows(same, none, 11) == [11] * 4                       # equal rows
    assert M._shared_prefix_of("auto", same, none) == 11                             # ... capped at min L_b - 1
    assert M._shared_prefix_of(11, same, none) == 11 and M._shared_prefix_of(0, same, none) is None
    with pytest.raises(ValueError, match="shared_prefix_rows = 12 leaves a sequence of 12 rows"):
        M._shared_prefix_of(12, same, none)
    x = same.clone()
    x[2, 0, 5] += 1.0                                                                # a break at row 0
    assert M._first_differing_rows(x, none, 11) == [11, 11, 0, 11] and M._shared_prefix_of("auto", x, none) is None
    with pytest.raises(ValueError, match="sequence 2 differs from sequence 0 at row 0"):
        M._shared_prefix_of(4, x, none)
    x = same.clone()
    x[1, 10, 0] += 1.0                                                               # a break at the last row that may be shared
    x[3, 11, 0] += 1.0                                                               # (row 11 is always an own row)
    assert M._first_differing_rows(x, none, 11) == [11, 10, 11, 11] and M._shared_prefix_of("auto", x, none) == 10
    assert M._shared_prefix_of(10, x, none) == 10
    with pytest.raises(ValueError, match="sequence 1 differs from sequence 0 at row 10"):
        M._shared_prefix_of(11, x, none)
    # left padding: sequence b holds n - pads[b] rows at the end; its stripped rows are compared, whatever the padding rows hold
    pads = [0, 3, 5, 1]
    x = torch.randn(B, n, h, generator=g).bfloat16()
    for b, p in enumerate(pads):
        x[b, p:p + 6] = base[:6]
    assert M._shared_prefix_of("auto", x, pads) == 6 and M._shared_prefix_of(6, x, pads) == 6       # min L_b = 7: the cap
    x[2, pads[2] + 4] = base[7]
    assert M._first_differing_rows(x, pads, 6) == [6, 6, 4, 6] and M._shared_prefix_of("auto", x, pads) == 4
    with pytest.raises(ValueError, match="sequence 2 differs from sequence 0 at row 4"):
        M._shared_prefix_of(5, x, pads)
    with pytest.raises(ValueError, match="leaves a sequence of 7 rows"):
        M._shared_prefix_of(7, x, pads)
    # "auto" below the measured minimum is the ordinary batch; one prompt is the call without the argument
    old = F.set_variant("shared_prefix_min_rows", 5)
    try:
        assert M._shared_prefix_of("auto", x, pads) is None and M._shared_prefix_of(4, x, pads) == 4
    finally:
        F.set_variant("shared_prefix_min_rows", old)
    assert M._shared_prefix_of("auto", same[:1], [0]) is None and M._shared_prefix_of(7, same[:1], [0]) is None
    monkeypatch.setitem(F.VARIANTS, "shared_prefix_min_rows", 512)
    assert M._shared_prefix_of("auto", same, none) is None and M._shared_prefix_of(11, same, none) == 11     # an int S is taken at its word
