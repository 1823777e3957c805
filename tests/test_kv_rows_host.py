"""functional.KVRows on the host: the per-layer record a KVCache hands to the passes.  Its tensors are the cache's buffers (no copies, made
once), its one-sequence and prefix views are the slices the passes used to spell out, and every method calls the op of its name in
`ops`, in the cache's format, with the format's tensor group where the C side expects it.  The ops are replaced by recorders: no kernel
runs here (the passes on the device: tests/test_decode_walks_gpu.py and the tests of each pass)."""
import pytest
import torch

FORMATS = ("bf16", "fp8_e4m3")
NL, B, CAP, HQ, HKV, D = 3, 3, 12, 4, 2, 16
LAYER = 1


def new_cache(fmt, batch=B):
    from metamorph_amd import functional as F
    return F.KVCache(NL, CAP, HKV * D, "cpu", Hq=HQ, d=D, batch=batch, fmt=fmt)


def same(a, b):
    return (a.data_ptr(), tuple(a.shape), a.stride(), a.dtype) == (b.data_ptr(), tuple(b.shape), b.stride(), b.dtype)


def names(fmt):
    return ("k", "v", "k_scale", "v_scale") if fmt == "fp8_e4m3" else ("k", "v")


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_record_aliases_the_cache(fmt):
    cache = new_cache(fmt)
    assert len(cache.rows) == NL
    for i, rows in enumerate(cache.rows):
        assert rows.f8 == (fmt == "fp8_e4m3") == (cache.kv8 is not None) and rows.sfx == ("_f8" if rows.f8 else "")
        assert len(rows.kv) == len(names(fmt))
        for t, name in zip(rows.kv, names(fmt)):
            assert t is getattr(rows, name) and same(t, getattr(cache, name)[i]), (i, name)
        if not rows.f8:
            assert rows.k_scale is None and rows.v_scale is None
    assert cache.rows[LAYER] is cache.rows[LAYER]                    # made once: a captured step sees the same tensors every time


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_sequence_and_prefix_views(fmt):
    cache = new_cache(fmt)
    rows = cache.rows[LAYER]
    for b in range(B):
        one = rows.seq(b)
        assert one.f8 == rows.f8
        for t, name in zip(one.kv, names(fmt)):
            assert same(t, getattr(cache, name)[LAYER, b:b + 1]), (b, name)
    for t, name in zip(rows.prefix(), names(fmt)):
        assert same(t, getattr(cache, name)[LAYER, 0]), name


class Recorder:
    """stands in for the names of `ops`: logs (name, args, kwargs), returns a token"""

    def __init__(self, monkeypatch, ops):
        self.log = []
        for name in ("rope_kv_append_", "rope_kv_append_rows_", "attn_decode", "attn_extend", "attn_extend_ragged", "attn_decode_shared",
                     "attn_extend_shared"):
            for n in (name, name[:-1] + "_f8_" if name.endswith("_") else name + "_f8"):
                assert callable(getattr(ops, n)), n
                monkeypatch.setattr(ops, n, lambda *a, _n=n, **k: (self.log.append((_n, a, k)), "ret:" + _n)[1])
        for n in ("kv_quant_f8", "rows_gather"):
            monkeypatch.setattr(ops, n, lambda *a, _n=n, **k: (self.log.append((_n, a, k)), None)[1])

    def one(self):
        assert len(self.log) == 1, self.log
        return self.log.pop()


def is_group(got, want):
    return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_method_calls_the_op_of_its_format(fmt, monkeypatch):
    from metamorph_amd import ops
    cache = new_cache(fmt)
    rows = cache.rows[LAYER]
    f8 = fmt == "fp8_e4m3"
    kv = [getattr(cache, n)[LAYER] for n in names(fmt)]
    pre = [getattr(cache, n)[LAYER, 0] for n in names(fmt)]
    g = len(kv)
    r = Recorder(monkeypatch, ops)

    # RoPE + append: the tensor group is last (qkv, Hq, Hkv, d, cos, sin, positions[, blocks], k, v[, k_scale, v_scale])
    for method, name, head in ((rows.rope_append_, "rope_kv_append_f8_" if f8 else "rope_kv_append_", ("Hq", "Hkv", "d", "cos", "sin", "pos")),
                               (rows.rope_append_rows_, "rope_kv_append_rows_f8_" if f8 else "rope_kv_append_rows_",
                                ("Hq", "Hkv", "d", "cos", "sin", "pos", "blk"))):
        assert method("qkv", *head) == "ret:" + name
        n, a, k = r.one()
        assert n == name and a[:1 + len(head)] == ("qkv",) + head and is_group(a[1 + len(head):], kv) and k == {}

    # attention over the cache: q, the tensor group, then the caller's arguments
    for method, base in ((rows.attn_decode, "attn_decode"), (rows.attn_extend, "attn_extend"), (rows.attn_extend_ragged, "attn_extend_ragged")):
        name = base + ("_f8" if f8 else "")
        assert method("q", "a0", "a1", 7, workspace="ws") == "ret:" + name
        n, a, k = r.one()
        assert n == name and a[0] == "q" and is_group(a[1:1 + g], kv) and a[1 + g:] == ("a0", "a1", 7) and k == {"workspace": "ws"}

    # over a prefix stored once: q, the prefix rows of sequence 0, the tensor group, then the caller's arguments
    for method, base in ((rows.attn_decode_shared, "attn_decode_shared"), (rows.attn_extend_shared, "attn_extend_shared")):
        name = base + ("_f8" if f8 else "")
        assert method("q", "a0", 5, workspace="ws", own_block="tbl") == "ret:" + name
        n, a, k = r.one()
        assert n == name and a[0] == "q" and is_group(a[1:1 + g], pre) and is_group(a[1 + g:1 + 2 * g], kv)
        assert a[1 + 2 * g:] == ("a0", 5) and k == {"workspace": "ws", "own_block": "tbl"}


@pytest.mark.parametrize("fmt", FORMATS)
def test_store_rows(fmt, monkeypatch):
    """fp8_e4m3: kv_quant_f8 for k, then v, into the bytes and scales; bf16: rows_gather twice into the rows of ONE sequence where the
    identity map is given, else a tensor copy into all sequences (no op)."""
    from metamorph_amd import ops
    cache = new_cache(fmt)
    cache.k.zero_(), cache.v.zero_()
    r = Recorder(monkeypatch, ops)
    n, row0, b = 2, 3, 1
    W = HKV * D
    src = torch.arange(B * n * 2 * W, dtype=torch.float32).reshape(B * n, 2 * W).bfloat16()
    ks, vs = src[:, :W], src[:, W:]                                   # column blocks of a wider tensor, as the passes hand them over
    ident = torch.arange(n, dtype=torch.int32)
    one = cache.rows[LAYER].seq(b)
    one.store_rows(ks[:n], vs[:n], HKV, D, row0, n, ident)
    if fmt == "fp8_e4m3":
        for t, sc, s in (("k", "k_scale", ks), ("v", "v_scale", vs)):
            name, a, k = r.log.pop(0)
            assert name == "kv_quant_f8" and same(a[0], s[:n]) and a[1:3] == (HKV, D) and same(a[3], getattr(cache, t)[LAYER, b:b + 1])
            assert same(a[4], getattr(cache, sc)[LAYER, b:b + 1]) and k == {"row0": row0, "rows_per_seq": n}
        assert r.log == []
        cache.rows[LAYER].store_rows(ks, vs, HKV, D, row0, n)
        for t, sc, s in (("k", "k_scale", ks), ("v", "v_scale", vs)):
            name, a, k = r.log.pop(0)
            assert name == "kv_quant_f8" and same(a[0], s) and same(a[3], getattr(cache, t)[LAYER]) and same(a[4], getattr(cache, sc)[LAYER])
            assert k == {"row0": row0, "rows_per_seq": n}
        assert r.log == []
        return
    for t, s in (("k", ks), ("v", vs)):
        name, a, k = r.log.pop(0)
        assert name == "rows_gather" and same(a[0], s[:n]) and a[1] is ident and same(k["out"], getattr(cache, t)[LAYER, b, row0:row0 + n])
    assert r.log == []
    cache.rows[LAYER].store_rows(ks, vs, HKV, D, row0, n)
    assert r.log == []
    assert torch.equal(cache.k[LAYER, :, row0:row0 + n], ks.reshape(B, n, W)) and torch.equal(cache.v[LAYER, :, row0:row0 + n], vs.reshape(B, n, W))
    assert float(cache.k[LAYER, :, :row0].abs().sum()) == 0 and float(cache.k[LAYER, :, row0 + n:].abs().sum()) == 0
    assert float(cache.k[LAYER - 1].abs().sum()) == 0 and float(cache.k[LAYER + 1].abs().sum()) == 0
