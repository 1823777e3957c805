"""Control flow of the extend pass on CPU: which compute hook `_cached_forward` calls with which rows when n > 1 rows arrive on a filled
`HipKVCache` (`_extend_batch`, never `_decode_batch`), how `HipKVCache(prefill_chunk=N)` slices a prompt, and how
`generate(inputs=<whole conversation>, past_key_values=<cache holding a prefix>)` hands the decoder only the uncached rows.  The CPU oracle
stands in for the compute hooks, in the manner of tests/test_hf_generate_plumbing.py (whose stand-in model this file extends with the new
hook); the kernels behind the hooks are tested on the GPU (tests/test_attn_extend_gpu.py, tests/test_extend_pass_gpu.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from oracle import ref_model as RM, ref_ops as R
from oracle.ref_model import OracleConfig, decode_fixture_state_dict
from test_hf_generate_plumbing import _cpu_model


def _model():
    g = np.load(os.path.join(GOLDEN, "hfgen_text.npz"))
    model, calls = _cpu_model(g)
    calls["extend"] = []                                          # (sequences, their rows, cached rows before) of every call
    calls["prefill_rows"] = []
    ocfg = OracleConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                        vocab_size=128258, v_layers=2, v_intermediate=144, v_image=56, num_image_tokens=4, tokenizer_model_max_length=64)
    sd = decode_fixture_state_dict(g, ocfg, torch.float32)

    def decoder_rows(x):                                          # the stand-in decoder of that file: [L, h] fp32 -> hidden rows
        cos, sin = R.rope_tables(torch.arange(x.shape[0])[None], ocfg.head_dim, ocfg.rope_theta, x.dtype)
        h = x[None]
        for i in range(ocfg.num_hidden_layers):
            h = RM.llama_layer(sd, ocfg, i, h, None, cos, sin)
        return h[0]

    inner_prefill = model._prefill_batch

    def prefill(seqs, cache):
        calls["prefill_rows"].append([x.clone() for x in seqs])
        return inner_prefill(seqs, cache)

    def extend(x, cache, rows=None):
        B, n, h = x.shape
        rows = list(range(len(cache.kv.lengths))) if rows is None else list(rows)
        assert n > 1 and len(rows) == B
        calls["extend"].append((rows, x.clone(), [cache.kv.lengths[b] for b in rows]))
        out = []
        for j, b in enumerate(rows):
            m = cache.kv.lengths[b]
            assert m >= 1 and m + n <= cache.kv.max_len
            cache.kv.k[0, b, m:m + n] = x[j].float()
            cache.kv.lengths[b] = m + n
            out.append(decoder_rows(cache.kv.k[0, b, :m + n])[-n:].bfloat16())
        return torch.stack(out, 0)

    model._prefill_batch = prefill
    model._extend_batch = extend
    return model, calls, torch.from_numpy(g["input_ids"]), decoder_rows


def _cache(**kw):
    from metamorph_amd.model.language_model.metamorph_llama import HipKVCache
    return HipKVCache(**kw)


def test_rows_on_a_filled_cache_take_the_extend_hook_once():
    model, calls, ids, decoder_rows = _model()
    emb = model.model.embed_tokens(ids.repeat(1, 3))[:, :15]      # [1, 15, h]
    L = emb.shape[1]
    cache = _cache(capacity=64)
    model(inputs_embeds=emb[:, :L - 6], past_key_values=cache, use_cache=True)
    out = model(inputs_embeds=emb[:, L - 6:], past_key_values=cache, use_cache=True)
    assert calls["prefill"] == 1 and calls["decode"] == 0 and len(calls["extend"]) == 1
    rows, x, before = calls["extend"][0]
    assert rows == [0] and before == [L - 6] and torch.equal(x, emb[:, L - 6:])
    assert cache.kv.lengths == [L] and cache.get_seq_length() == L and tuple(out.logits.shape[:2]) == (1, 6)
    whole = model._rows_logits(decoder_rows(emb[0].float()).bfloat16())
    torch.testing.assert_close(out.logits[0], whole[-6:], rtol=2e-2, atol=2e-2)
    # one more row is a decode step again
    model(inputs_embeds=emb[:, :1], past_key_values=cache, use_cache=True)
    assert calls["decode"] == 1 and len(calls["extend"]) == 1


def test_prefill_chunk_slices_the_prompt():
    model, calls, ids, _ = _model()
    emb = model.model.embed_tokens(ids.repeat(1, 3))[:, :11]      # an 11-row prompt
    assert emb.shape[1] == 11
    cache = _cache(capacity=32, prefill_chunk=4)
    out = model(inputs_embeds=emb, past_key_values=cache, use_cache=True)
    assert calls["prefill"] == 1 and calls["decode"] == 0
    assert len(calls["prefill_rows"]) == 1 and torch.equal(calls["prefill_rows"][0][0], emb[0, :4])
    assert [(r, tuple(x.shape[:2]), before) for r, x, before in calls["extend"]] == [([0], (1, 4), [4]), ([0], (1, 3), [8])]
    assert torch.equal(calls["extend"][0][1][0], emb[0, 4:8]) and torch.equal(calls["extend"][1][1][0], emb[0, 8:11])
    assert cache.kv.lengths == [11] and tuple(out.logits.shape[:2]) == (1, 11)
    # the same through the configuration, read when the cache object has none; a prompt within one slice is one prompt pass
    model2, calls2, _, _ = _model()
    model2.config.mm355_prefill_chunk_rows = 8
    model2(inputs_embeds=emb, past_key_values=_cache(capacity=32), use_cache=True)
    assert [tuple(x.shape[:2]) for _, x, _ in calls2["extend"]] == [(1, 3)] and calls2["prefill_rows"][0][0].shape[0] == 8
    model2(inputs_embeds=emb[:, :8], past_key_values=_cache(capacity=32), use_cache=True)
    assert len(calls2["extend"]) == 1 and calls2["prefill_rows"][1][0].shape[0] == 8
    with pytest.raises(ValueError, match="prefill_chunk"):
        _cache(prefill_chunk=0)
    model2.config.mm355_prefill_chunk_rows = 0
    with pytest.raises(ValueError, match="mm355_prefill_chunk_rows"):
        model2(inputs_embeds=emb, past_key_values=_cache(capacity=32), use_cache=True)


def test_generate_continues_a_conversation_from_its_cached_prefix():
    model, calls, ids, _ = _model()
    conv = ids.repeat(1, 3)[:, :14]                        # the whole conversation
    L = conv.shape[1]
    kw = dict(use_customize_greedy=False, do_sample=False, max_new_tokens=4, eos_token_id=128009, pad_token_id=128001)
    want = model.generate(inputs=conv, **kw)[0].tolist()          # uncached: one prompt pass over all L rows
    assert calls["prefill"] == 1 and calls["prefill_rows"][0][0].shape[0] == L and not calls["extend"]
    cache = _cache(capacity=L + 8)
    model(inputs_embeds=model.model.embed_tokens(conv[:, :9]), past_key_values=cache, use_cache=True)      # the first 9 rows are cached
    n_dec = calls["decode"]
    got = model.generate(inputs=conv, past_key_values=cache, **kw)[0].tolist()
    assert got == want, (got, want)
    assert calls["prefill"] == 2                                  # (the uncached run and the 9-row prefix: no third prompt pass)
    assert len(calls["extend"]) == 1
    rows, x, before = calls["extend"][0]
    assert before == [9] and x.shape[1] == L - 9 and torch.equal(x, model.model.embed_tokens(conv[:, 9:]))
    assert calls["decode"] - n_dec == len(want) - 1
    # a cache too small for the conversation is refused by name, not grown (the real hook: it checks before it computes anything)
    from metamorph_amd.model.language_model.metamorph_llama import MetaMorphLlamaForCausalLM
    from types import SimpleNamespace
    small = _cache(capacity=12)
    small.kv = SimpleNamespace(lengths=[9], max_len=12, batch=1)
    small.pads = [0]
    with pytest.raises(ValueError, match="HipKVCache capacity 12"):
        MetaMorphLlamaForCausalLM._extend_batch(model, torch.zeros(1, 5, 256), small)


def test_crop_then_extend_lands_on_the_cropped_length():
    model, calls, ids, _ = _model()
    emb = model.model.embed_tokens(ids.repeat(1, 3))[:, :11]
    cache = _cache(capacity=32)
    model(inputs_embeds=emb, past_key_values=cache, use_cache=True)
    assert cache.get_seq_length() == 11
    cache.crop(7)
    model(inputs_embeds=emb[:, 7:10], past_key_values=cache, use_cache=True)
    rows, x, before = calls["extend"][-1]
    assert before == [7] and cache.kv.lengths == [10] and cache.get_seq_length() == 10


def test_extend_symbols_are_declared_and_exported():
    from metamorph_amd import lib
    new = ("mm355_attn_extend", "mm355_attn_extend_f8", "mm355_attn_extend_ws_floats")
    names = lib.exported_symbols()
    for n in new:
        assert n in names, n
    text = open(os.path.join(REPO, "include", "mm355.h")).read()
    assert "past[b] + i" in text and "csrc/attn_extend.hip" in text
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(lib.LIB_PATH)
    for n in new:
        assert hasattr(so, n), n
    L = lib.load()
    assert L.mm355_attn_extend_ws_floats(1, 512, 32, 8, 128, 4608) == 0          # 256 workgroups of row tiles: no key split
    assert L.mm355_attn_extend_ws_floats(1, 1, 32, 8, 128, 4096) > 0             # 8 workgroups: the keys are dealt out
    from metamorph_amd import functional as F, ops
    assert callable(ops.attn_extend) and callable(ops.attn_extend_f8) and callable(F.decoder_extend)
    assert F.VARIANTS["extend_pass"] is True
