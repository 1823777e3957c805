"""n continuations of one prompt over a shared prompt cache, the parts that need no GPU: the C ABI's symbols and the refusals of
mm355_attn_decode_shared / _f8 by return code, and greedy_decode's refusals of bad num_return_sequences calls by name."""
import ctypes
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mm355_attn_decode_shared_ws_floats", "mm355_attn_decode_shared", "mm355_attn_decode_shared_f8")


def test_shared_prefix_symbols_and_refusals_without_a_gpu():
    from metamorph_amd import lib, ops
    names = lib.exported_symbols()
    header = open(os.path.join(REPO, "include", "mm355.h")).read()
    for n in NEW:
        assert n in names and f"{n}(" in header, n
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(lib.LIB_PATH)
    for n in NEW:
        assert hasattr(so, n), n
    assert hasattr(ops, "attn_decode_shared") and hasattr(ops, "attn_decode_shared_f8")
    L = lib.load()
    P = 4096                                                     # a non-null, 16-byte aligned stand-in: no kernel is launched on the error path
    B, Hq, Hkv, d, rows, S = 3, 8, 2, 128, 512, 300
    ld, bs = Hkv * d, rows * Hkv * d
    need = L.mm355_attn_decode_shared_ws_floats(B, Hq, Hkv, d, S, rows)
    assert need > 0 and L.mm355_attn_decode_shared_ws_floats(B, Hq, Hkv, d, 0, rows) > 0      # the own partial is always written
    assert L.mm355_attn_decode_shared_ws_floats(B, Hq, Hkv, d, rows + 1, rows) == 0 and L.mm355_attn_decode_shared_ws_floats(B, Hq, Hkv, d, -1, rows) == 0

    def bf(q=P, ldq=Hq * d, ksh=P, vsh=P, ldsh=ld, k=P, v=P, ldkv=ld, bskv=bs, lens=P, S_=S, bound=rows, o=P, ldo=Hq * d, Hq_=Hq, d_=d, ws=P,
           nws=need):
        return L.mm355_attn_decode_shared(q, ldq, ksh, vsh, ldsh, k, v, ldkv, bskv, lens, S_, bound, o, ldo, B, Hq_, Hkv, d_, 0.1, ws, nws, 0)

    def f8(fmt=1, ksh=P, kshs=P, vshs=P, ldsh=ld, ldshs=Hkv, k=P, ks=P, vs=P, ldkv=ld, ldsc=Hkv, S_=S, d_=d, Hq_=Hq, ws=P, nws=need):
        return L.mm355_attn_decode_shared_f8(P, Hq_ * d, ksh, P, ldsh, kshs, vshs, ldshs, k, P, ldkv, bs, ks, vs, ldsc, rows * Hkv, fmt, P, S_, rows,
                                             P, Hq_ * d, B, Hq_, Hkv, d_, 0.1, ws, nws, 0)
    for null in ("q", "ksh", "vsh", "k", "v", "lens", "o"):      # NULL pointers
        assert bf(**{null: 0}) == -1, null
    assert bf(q=P + 2) == -1 and bf(o=P + 8) == -1 and bf(k=P + 8) == -1 and bf(ksh=P + 8) == -1     # misaligned pointers
    assert bf(ldq=Hq * d + 4) == -1 and bf(ldo=Hq * d + 2) == -1 and bf(ldkv=ld + 4) == -1 and bf(bskv=bs + 4) == -1 and bf(ldsh=ld + 4) == -1
    assert bf(ldkv=ld - 8) == -1 and bf(ldsh=ld - 8) == -1       # a row stride shorter than a row
    assert bf(S_=-1) == -1 and bf(S_=rows + 1) == -1             # shared_len outside [0, max_kv_len]
    assert bf(ws=0) == -1 and bf(nws=need - 1) == -1 and bf(ws=P + 4) == -1 and bf(S_=0, ws=0) == -1   # the workspace: missing, short, misaligned
    assert bf(Hq_=5) == -1                                       # Hq % Hkv
    assert bf(d_=124) == -2 and bf(d_=136) == -2                 # d % 8, d > 128
    assert bf(Hq_=6, ldq=6 * d, ldo=6 * d) == -2 and bf(Hq_=32, ldq=32 * d, ldo=32 * d) == -2          # GQA groups of 3 and 16
    assert f8(fmt=7) == -1 and f8(ks=0) == -1 and f8(vs=0) == -1 and f8(kshs=0) == -1 and f8(vshs=0) == -1   # a format that does not exist, NULL scales
    assert f8(k=P + 4) == -1 and f8(ksh=P + 4) == -1 and f8(ldkv=ld + 4) == -1 and f8(ldsh=ld + 4) == -1     # 8-byte cache alignment
    assert f8(ks=P + 2) == -1 and f8(kshs=P + 2) == -1 and f8(ldsc=Hkv - 1) == -1 and f8(ldshs=Hkv - 1) == -1   # 4-byte scales, short scale rows
    assert f8(S_=-1) == -1 and f8(S_=rows + 1) == -1 and f8(ws=0) == -1 and f8(nws=need - 1) == -1
    assert f8(d_=124) == -2 and f8(Hq_=6) == -2
    assert ops.attn_decode_shared_supported(8, 2, 128) and not ops.attn_decode_shared_supported(6, 2, 128)
    assert not ops.attn_decode_shared_supported(8, 2, 136) and not ops.attn_decode_shared_supported(8, 2, 124)


def _tiny_cpu_model():
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
               rms_norm_eps=1e-5, rope_theta=500000.0)
    geo = dict(hidden_size=64, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14)
    return build_model(llm, geo, num_image_tokens=4, max_length=64)


def test_greedy_decode_refuses_bad_num_return_sequences_calls_by_name():
    model = _tiny_cpu_model().eval()
    emb = torch.zeros(1, 5, 64, dtype=torch.bfloat16)
    sample = dict(do_sample=True, temperature=0.7)

    def call(e=emb, **kw):
        return model.greedy_decode(None, None, e, max_new_tokens=4, **kw)
    for kw in ({}, dict(do_sample=True), dict(do_sample=True, temperature=0.0), dict(do_sample=False, temperature=0.7)):
        with pytest.raises(ValueError, match="num_return_sequences=3.*active sampler"):
            call(num_return_sequences=3, **kw)
    with pytest.raises(ValueError, match="num_return_sequences=3.*one prompt"):
        call(torch.zeros(2, 5, 64, dtype=torch.bfloat16), num_return_sequences=3, **sample)
    for bad in (0, -2, 2.0, 1.5, "3", True):
        with pytest.raises(ValueError, match="num_return_sequences.*positive integer"):
            call(num_return_sequences=bad, **sample)
    with pytest.raises(ValueError, match="num_return_sequences=3.*use_cache=False"):
        call(num_return_sequences=3, use_cache=False, **sample)
    with pytest.raises(ValueError, match="stream_ids"):
        call(num_return_sequences=3, stream_ids=[0, 1], **sample)
    with pytest.raises(ValueError, match="num_beams"):
        call(num_return_sequences=3, num_beams=2, **sample)
    assert type(model)._copies_of(None) == 1 and type(model)._copies_of(1) == 1 and type(model)._copies_of(17) == 17


def test_a_shared_prefix_is_refused_where_the_cache_cannot_hold_it():
    from metamorph_amd import functional as F
    assert F.VARIANTS["shared_prefix_attn"] in (True, False)
    kv = F.KVCache(1, 16, 128, "cpu", batch=3)                   # (no Hq / d: no attention workspace can be sized)
    assert kv.shared_len == 0 and kv.shared is None
    with pytest.raises(ValueError, match="every sequence must hold the shared rows"):
        kv.set_shared(4)
    with pytest.raises(ValueError, match="Hq and d"):
        kv.lengths = [4, 4, 5]
        kv.set_shared(4)
