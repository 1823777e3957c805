"""The ragged pass on the CPU: its five symbols are declared and exported and refuse bad arguments before any launch, ragged_rows_plan on
hand-written cases, config.mm355_ragged_pass, and which functional pass `_prefill_batch` / `_extend_batch` take under which conditions (the
real methods on the stand-in model of tests/test_hf_generate_plumbing.py, `functional` monkeypatched as tests/test_extend_plumbing.py
does).  The kernels are tested on the GPU: tests/test_attn_extend_ragged_gpu.py, tests/test_rope_kv_append_rows_gpu.py,
tests/test_ragged_pass_gpu.py, tests/test_ragged_generate_gpu.py."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from test_hf_generate_plumbing import _cpu_model

NEW = ("mm355_attn_extend_ragged", "mm355_attn_extend_ragged_f8", "mm355_attn_extend_ragged_ws_floats", "mm355_rope_kv_append_rows",
       "mm355_rope_kv_append_rows_f8")
EINVAL, EUNSUPPORTED = -1, -2                                  # MM355_EINVAL, MM355_EUNSUPPORTED


def _lib():
    from metamorph_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return lib


def test_ragged_symbols_are_declared_and_exported():
    lib = _lib()
    names = lib.exported_symbols()
    text = open(os.path.join(REPO, "include", "mm355.h")).read()
    so = ctypes.CDLL(lib.LIB_PATH)
    for n in NEW:
        assert n in names and hasattr(so, n), n
    assert "row_start[b + 1] - row_start[b]" in text and "metamorph_llama.py:502-597" in text
    L = lib.load()
    assert L.mm355_strerror(EINVAL) and L.mm355_attn_extend(0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 1, 8, 1.0, 0, 0, 0) == EINVAL
    # the plan of the ragged form is the plain form's for n = n_max
    for a in ((1, 512, 32, 8, 128, 4608), (1, 1, 32, 8, 128, 4096), (5, 70, 8, 2, 128, 2570)):
        assert L.mm355_attn_extend_ragged_ws_floats(*a) == L.mm355_attn_extend_ws_floats(*a)
    from metamorph_amd import functional as F, ops
    for f in (ops.attn_extend_ragged, ops.attn_extend_ragged_f8, ops.rope_kv_append_rows_, ops.rope_kv_append_rows_f8_, F.decoder_extend_ragged,
              F.ragged_rows_plan):
        assert callable(f)
    assert F.VARIANTS["ragged_pass_attn"] is True
    assert ops.attn_extend_ragged_supported(32, 8, 128) and ops.attn_extend_ragged_supported(16, 16, 72)
    assert not ops.attn_extend_ragged_supported(12, 4, 128) and not ops.attn_extend_ragged_supported(8, 2, 132)


def test_ragged_entry_points_refuse_before_any_launch():
    """Refusals need no GPU: every pointer below is a made-up aligned address that a refused call never touches."""
    L = _lib().load()
    P = 0x10000                                                   # "a pointer": non-NULL and 16-byte aligned
    B, Hq, Hkv, d, rows = 2, 8, 2, 128, 64

    def ragged(q=P, ld_q=Hq * d, k=P, v=P, ld_kv=Hkv * d, bs=rows * Hkv * d, past=P, row_start=P, n_max=4, q_rows=8, max_kv=rows, o=P, ld_o=Hq * d,
               B=B, Hq=Hq, Hkv=Hkv, d=d, ws=0, ws_floats=0):
        return L.mm355_attn_extend_ragged(q, ld_q, k, v, ld_kv, bs, past, row_start, n_max, q_rows, max_kv, o, ld_o, B, Hq, Hkv, d, 1.0, ws, ws_floats, 0)

    def ragged_f8(fmt=1, ks=P, vs=P, row_start=P, n_max=4, q_rows=8, max_kv=rows):
        return L.mm355_attn_extend_ragged_f8(P, Hq * d, P, P, Hkv * d, rows * Hkv * d, ks, vs, Hkv, rows * Hkv, fmt, P, row_start, n_max, q_rows, max_kv,
                                             P, Hq * d, B, Hq, Hkv, d, 1.0, 0, 0, 0)

    for kw in (dict(row_start=0), dict(n_max=0), dict(n_max=rows + 1), dict(q_rows=0), dict(q=0), dict(past=0), dict(o=0), dict(k=0), dict(B=0),
               dict(Hq=7), dict(q=P + 2), dict(ld_q=Hq * d + 4), dict(ld_kv=Hkv * d - 8), dict(max_kv=0)):
        assert ragged(**kw) == EINVAL, kw
    assert ragged(d=132, ld_q=8 * 132, ld_o=8 * 132, ld_kv=2 * 132) == EUNSUPPORTED and ragged(Hq=6) == EUNSUPPORTED      # d % 8, a group of 3
    # the keys are dealt out at this shape: a workspace that is missing or too small
    n_ws = L.mm355_attn_extend_ragged_ws_floats(B, 4, Hq, Hkv, d, 4096)
    assert n_ws > 0 and ragged(max_kv=4096, bs=4096 * Hkv * d) == EINVAL and ragged(max_kv=4096, bs=4096 * Hkv * d, ws=P, ws_floats=n_ws - 1) == EINVAL
    for kw in (dict(fmt=0), dict(ks=0), dict(vs=0), dict(row_start=0), dict(n_max=0), dict(n_max=rows + 1), dict(q_rows=0)):
        assert ragged_f8(**kw) == EINVAL, kw

    def append(qkv=P, ld=(Hq + 2 * Hkv) * d, R=7, d=d, pos=P, blocks=P, n_blocks=3, rpb=40, k=P, v=P, ld_kv=Hkv * d):
        return L.mm355_rope_kv_append_rows(qkv, ld, R, Hq, Hkv, d, P, P, pos, blocks, n_blocks, rpb, k, v, ld_kv, 40 * Hkv * d, 0)

    def append_f8(fmt=1, R=7, d=d, pos=P, blocks=P, n_blocks=3, rpb=40, ks=P, k=P):
        return L.mm355_rope_kv_append_rows_f8(P, (Hq + 2 * Hkv) * d, R, Hq, Hkv, d, P, P, pos, blocks, n_blocks, rpb, k, P, Hkv * d, 40 * Hkv * d, ks, P,
                                              Hkv, 40 * Hkv, fmt, 0)

    for kw in (dict(n_blocks=0), dict(rpb=0), dict(R=0), dict(pos=0), dict(qkv=0), dict(k=0), dict(d=72), dict(ld=(Hq + 2 * Hkv) * d + 4),
               dict(ld_kv=Hkv * d + 4), dict(blocks=0, n_blocks=6)):      # (no table: block r for row r needs R blocks)
        assert append(**kw) == EINVAL, kw
    for kw in (dict(fmt=0), dict(n_blocks=0), dict(rpb=0), dict(R=0), dict(pos=0), dict(ks=0), dict(d=72), dict(k=P + 4), dict(blocks=0, n_blocks=6)):
        assert append_f8(**kw) == EINVAL, kw
    assert append_f8(d=132) == EUNSUPPORTED


def test_ragged_rows_plan():
    from metamorph_amd.functional import ragged_rows_plan
    p = ragged_rows_plan([3, 1, 2], [0, 5, 7], [0, 1, 2])         # past = 0: a prompt
    assert p.row_start.tolist() == [0, 3, 4, 6] and p.past.tolist() == [0, 5, 7]
    assert p.positions.tolist() == [0, 1, 2, 5, 7, 8] and p.blocks.tolist() == [0, 0, 0, 1, 2, 2]
    assert (p.n_max, p.bound) == (3, 9)
    assert all(a.dtype == np.int32 for a in (p.row_start, p.positions, p.blocks, p.past))
    # permuted, and a subset: the packed rows stand in block order; a block that is not named brings no row
    p = ragged_rows_plan([2, 4], [10, 1], [3, 1])
    assert p.row_start.tolist() == [0, 0, 4, 4, 6] and p.past.tolist() == [0, 1, 0, 10]
    assert p.positions.tolist() == [1, 2, 3, 4, 10, 11] and p.blocks.tolist() == [1, 1, 1, 1, 3, 3]
    assert (p.n_max, p.bound) == (4, 12)
    for bad in (([2, 0], [1, 1], [0, 1]), ([], [], []), ([1, 1], [1, 1], [0, 0]), ([1], [-1], [0]), ([1], [1], [-1]), ([1, 2], [1], [0, 1])):
        with pytest.raises(ValueError, match="ragged_rows_plan"):
            ragged_rows_plan(*bad)


def _model(monkeypatch):
    """the stand-in model with its REAL _prefill_batch / _extend_batch, every functional pass behind them recorded"""
    from metamorph_amd import functional as F, ops
    from metamorph_amd.model.language_model.metamorph_llama import MetaMorphLlamaForCausalLM as M
    model, _ = _cpu_model(np.load(os.path.join(GOLDEN, "hfgen_text.npz")))
    del model._prefill_batch                                      # (the instance attributes of the stand-in: back to the class's methods)
    calls = []

    def new_kv_cache(cache, rows, batch, device):
        cache.kv = SimpleNamespace(lengths=[0] * batch, max_len=rows + 64, batch=batch, shared_len=0)
        cache.meta = model._decode_meta(rows)[1]
        return cache.meta, None, None
    model._new_kv_cache = new_kv_cache

    def record(name, ret):
        def f(*a, **kw):
            calls.append((name, a, kw))
            return ret(*a, **kw)
        monkeypatch.setattr(F, name, f)
    record("decoder_extend_ragged", lambda xs, layers, meta, kv, rows=None: [x.clone() for x in xs])
    record("decoder_prefill", lambda x, layers, meta, kv, row=0: x.clone())
    record("decoder_prefill_chunked", lambda x, layers, meta, kv, chunk, row=0: x.clone())
    record("decoder_extend", lambda x, layers, meta, kv, row=0: x.clone())
    launched = []
    for name in ("attn_extend_ragged", "attn_extend_ragged_f8", "rope_kv_append_rows_", "rope_kv_append_rows_f8_"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: launched.append(_n))
    return model, M, calls, launched


def _cache(**kw):
    from metamorph_amd.model.language_model.metamorph_llama import HipKVCache
    return HipKVCache(**kw)


def _names(calls):
    return [c[0] for c in calls]


def test_config_field_and_routes(monkeypatch):
    from metamorph_amd import functional as F
    model, M, calls, launched = _model(monkeypatch)
    h = 256
    ragged = [torch.zeros(n, h, dtype=torch.bfloat16) for n in (5, 9, 7)]
    equal = [torch.zeros(6, h, dtype=torch.bfloat16) for _ in range(3)]

    def prefill(seqs, **kw):
        del calls[:]
        out = M._prefill_batch(model, seqs, _cache(), stepper=False, **kw)
        assert [tuple(o.shape) for o in out] == [tuple(x.shape) for x in seqs]
        return _names(calls)

    def extend(B, n=4, rows=None):
        del calls[:]
        cache = _cache()
        batch = max(rows) + 1 if rows else B
        cache.kv = SimpleNamespace(lengths=[9, 3, 5][:batch], max_len=64, batch=batch, shared_len=0)
        cache.meta = model._decode_meta(9)[1]
        out = M._extend_batch(model, torch.zeros(B, n, h, dtype=torch.bfloat16), cache, rows=rows)
        assert tuple(out.shape) == (B, n, h)
        return _names(calls)

    # the flag absent, and False: today's calls
    for off in (None, False):
        if off is not None:
            model.config.mm355_ragged_pass = off
        assert not hasattr(model.config, "mm355_ragged_pass") or model.config.mm355_ragged_pass is False
        assert prefill(ragged) == ["decoder_prefill_chunked"] * 3 and prefill(equal) == ["decoder_prefill"]
        assert extend(3) == ["decoder_extend"] * 3 and extend(1) == ["decoder_extend"]
    # on: ragged prompts of B > 1 without a chunk, or within one chunk
    model.config.mm355_ragged_pass = True
    assert prefill(ragged) == ["decoder_extend_ragged"]
    name, a, kw = calls[0]
    assert [tuple(x.shape) for x in a[0]] == [(5, h), (9, h), (7, h)] and a[3].lengths == [0, 0, 0] and "rows" not in kw
    assert prefill(ragged, chunk=9) == ["decoder_extend_ragged"]
    assert prefill(ragged, chunk=8) == ["decoder_prefill_chunked"] * 3          # a chunked ragged prompt: out of scope
    assert prefill(equal) == ["decoder_prefill"] and prefill(ragged[:1]) == ["decoder_prefill_chunked"]
    # a follow-up turn of B > 1: one pass for all sequences, the rows handed on
    assert extend(3) == ["decoder_extend_ragged"] and calls[0][2]["rows"] == [0, 1, 2] and len(calls[0][1][0]) == 3
    assert extend(2, rows=[2, 0]) == ["decoder_extend_ragged"] and calls[0][2]["rows"] == [2, 0]
    assert extend(1) == ["decoder_extend"]
    # the tools' switch, and a head shape without a kernel, fall back to today's calls
    old = F.set_variant("ragged_pass_attn", False)
    try:
        assert prefill(ragged) == ["decoder_prefill_chunked"] * 3 and extend(3) == ["decoder_extend"] * 3
    finally:
        F.set_variant("ragged_pass_attn", old)
    monkeypatch.setattr(F, "ragged_pass_supported", lambda meta: False)
    assert prefill(ragged) == ["decoder_prefill_chunked"] * 3 and extend(3) == ["decoder_extend"] * 3
    # anything but a bool is refused by name
    for bad in (1, "auto", None):
        model.config.mm355_ragged_pass = bad
        with pytest.raises(ValueError, match="mm355_ragged_pass"):
            prefill(ragged)
        with pytest.raises(ValueError, match="mm355_ragged_pass"):
            extend(3)
    assert not launched                                           # and with the flag absent no new kernel anywhere: none of the passes above reaches one
