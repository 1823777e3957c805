"""The launch sequence of every layer walk of a cached decode, route by route: decoder_prefill (fused), decoder_extend and
decoder_extend_shared (fused and plain) and the decode step of more than 16 sequences (_decode_rows_gemm, fused and unfused); further down
the decode step of up to 16 sequences (with and without a shared prefix), decoder_extend_ragged, decoder_prefill's plain route and
decoder_extend_shared's per-sequence append.  On bf16 and on quantize_decoder_ weights, over a bf16 and an fp8_e4m3 cache.  The callables
of functional.ops (and, for a quantised layer, its record's own GEMMs and its dequantiser) are wrapped to log their names, functional.params_ready logs the layer it is called for, and the log of one
call is compared with a list written out here: tests elsewhere count named ops, this one fixes their order.

The h = 1024 model of tests/test_extend_pass_gpu.py (8 / 2 heads of 128, I = 2048), its first two layers: on the h = 256 model no
projection is split at these row counts, so no fused route would run.  One more model of the same widths with I = 10496 puts the gate|up
projection on the two-row-group GEMV that a step of 17 .. 32 sequences takes on wide weights (ops.gemv_rows32_units)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.ref_model import init_state_dict  # noqa: E402
from test_extend_pass_gpu import FMT, embeds, hip_model, model_meta, model_of, new_cache, tiny_cfg  # noqa: E402

pytestmark = pytest.mark.gpu
NL = 2                                                       # layers walked

# every op of functional.ops that a walk may launch (queries such as gemm_splitk_splits are not launches)
OPS = ("rmsnorm_fwd", "gemm", "gemm_splitk", "gemm_splitk_norm", "gemm_splitk_swiglu", "gemm_splitk_rope_append", "gemm_swiglu", "swiglu_fwd",
       "gemv", "gemv_swiglu", "gemv_rope_append", "gemm_rope", "rope_qk_", "rope_kv_append_", "rope_kv_append_f8_", "kv_quant_f8", "rows_gather",
       "attn_fwd", "attn_extend", "attn_extend_f8", "attn_extend_shared", "attn_extend_shared_f8", "attn_decode", "attn_decode_f8",
       "attn_decode_shared", "attn_decode_shared_f8", "rope_kv_append_rows_", "rope_kv_append_rows_f8_", "attn_extend_ragged",
       "attn_extend_ragged_f8")
RECORD = ("gemm", "gemm_norm", "gemm_swiglu", "gemm_rope_append", "gemv", "gemv_swiglu", "gemv_rope_append", "dequant")
# a quantised layer whose four projections all run on their bytes: the record's op in place of the bf16 one
ON_BYTES = {"gemm_splitk": "w8.gemm", "gemm_splitk_norm": "w8.gemm_norm", "gemm_splitk_swiglu": "w8.gemm_swiglu",
            "gemm_splitk_rope_append": "w8.gemm_rope_append"}
# kernel launches behind an op, as the docstrings of functional count them: a split projection is two (the slices, then the reduce launch
# that carries the epilogue), everything else one
LAUNCHES = {"gemm_splitk": 2, "gemm_splitk_norm": 2, "gemm_splitk_swiglu": 2, "gemm_splitk_rope_append": 2,
            "w8.gemm": 2, "w8.gemm_norm": 2, "w8.gemm_swiglu": 2, "w8.gemm_rope_append": 2}


def launches(names):
    return sum(LAUNCHES.get(n, 1) for n in names if not n.startswith("ready:"))


def logged(monkeypatch, layers, fn):
    """fn() with every op wrapped: the names in call order, "ready:<i>" where params_ready is called for layer i"""
    from metamorph_amd import functional as F
    log = []
    index = {id(layer): i for i, layer in enumerate(layers)}
    with monkeypatch.context() as mp:
        for name in OPS:
            mp.setattr(F.ops, name, lambda *a, _o=getattr(F.ops, name), _n=name, **k: (log.append(_n), _o(*a, **k))[1])
        for name in RECORD:
            mp.setattr(F.W8Layer, name, staticmethod(lambda *a, _o=getattr(F.W8Layer, name), _n="w8." + name, **k: (log.append(_n), _o(*a, **k))[1]))
        mp.setattr(F, "_PARAM_READY_HOOK", lambda key, backward=False: log.append(f"ready:{index.get(id(key))}"))
        with torch.no_grad():
            out = fn()
    torch.cuda.synchronize()
    return log, out


def fused_walk(step, gu, weights):
    """The fused split-K walk of NL layers around its q|k|v + append + attention step and its gate|up ops (written for bf16 weights; on
    a quantised layer the split projections become the record's): the input norm in front of the first layer only, o and down with the
    norm that follows in their reduce launch, the next layer's parameters asked for before its norm weight is read, the plain down last."""
    w = (lambda names: [ON_BYTES.get(n, n) for n in names]) if weights == "w8" else (lambda names: list(names))
    scratch = ["w8.dequant"] if weights == "w8" and "gemm_splitk_swiglu" not in gu else []     # gate|up off its bytes: dequantised first
    gu = list(gu) if scratch else w(gu)
    first = ["ready:0"] + scratch + ["rmsnorm_fwd"] + w(step) + w(["gemm_splitk_norm"]) + gu + ["ready:1"] + w(["gemm_splitk_norm"])
    last = ["ready:1"] + scratch + w(step) + w(["gemm_splitk_norm"]) + gu + w(["gemm_splitk"])
    return [first, last]


def plain_walk(step, weights, on_bytes=False):
    """The plain walk of NL layers: every norm, the rotation and SwiGLU as launches of their own.  A quantised layer is dequantised into the
    scratch first (decoder_extend / decoder_extend_shared) or runs every projection on its bytes (the decode step: on_bytes)."""
    body = ["rmsnorm_fwd", "gemm_splitk"] + list(step) + ["gemm_splitk", "rmsnorm_fwd", "gemm_splitk", "swiglu_fwd", "gemm_splitk"]
    if weights == "w8" and on_bytes:
        body = [ON_BYTES.get(n, n) for n in body]
    scratch = ["w8.dequant"] * 4 if weights == "w8" and not on_bytes else []
    return [[f"ready:{i}"] + scratch + body for i in range(NL)]


def check(log, layers_expected, what):
    flat = [n for layer in layers_expected for n in layer]
    print(f"   {what}: {launches(log)} launches; layer 0: {' '.join(layers_expected[0])}")
    assert log == flat, (what, log, flat)


def all_on_bytes(m, rows, gu_rows=None):
    from metamorph_amd import functional as F
    return all(F.w8_on_gemm(layer, rows, gu_rows) == frozenset(F.W8Layer.NAMES) for layer in m.model.layers[:NL])


def splits(meta, h, rows):
    from metamorph_amd import ops
    return ops.gemm_splitk_splits(rows, (meta.Hq + 2 * meta.Hkv) * meta.d, h)


GU_PROMPT = {21: ["gemm_splitk_swiglu"], 65: ["gemm", "swiglu_fwd"]}       # PROMPT_GU_SPLITK_ROWS = 64: 65 rows take the plain GEMM


@pytest.mark.parametrize("fmt", ["bf16", FMT])
@pytest.mark.parametrize("weights", ["bf16", "w8"])
@pytest.mark.parametrize("L", [21, 65])
def test_fused_prompt_pass(L, weights, fmt, monkeypatch):
    """decoder_prefill of one sequence, fused: q|k|v + RoPE + the K / V rows into the cache in one split projection, attention, then (an
    fp8_e4m3 cache) the quantisation of the two staging buffers."""
    from metamorph_amd import functional as F
    cfg, m, _ = model_of("h1024", weights)
    h, layers = cfg.hidden_size, m.model.layers[:NL]
    x = embeds(1, L, h, seed=3)[0].contiguous()
    cache, meta, cos, sin = new_cache(m, cfg, L + 4, fmt=fmt)
    assert F.PROMPT_GU_SPLITK_ROWS == 64 and F.VARIANTS["prefill_fused"] and F.VARIANTS["prefill_splitk"] and splits(meta, h, L)
    if weights == "w8":
        assert all_on_bytes(m, L, 64) == (L <= 64) and F.w8_on_gemm(layers[0], L, 64) >= {"qkv", "o", "down"}
    log, _ = logged(monkeypatch, layers, lambda: F.decoder_prefill(x, layers, model_meta(m, L, cos, sin), cache))
    step = ["gemm_splitk_rope_append", "attn_fwd"] + (["kv_quant_f8", "kv_quant_f8"] if fmt == FMT else [])
    check(log, fused_walk(step, GU_PROMPT[L], weights), f"prefill {L} rows {weights} {fmt}")
    assert cache.lengths == [L]


def filled(m, cfg, layers, fmt, L0, cap):
    from metamorph_amd import functional as F
    cache, meta, cos, sin = new_cache(m, cfg, cap, fmt=fmt)
    with torch.no_grad():
        F.decoder_prefill(embeds(1, L0, cfg.hidden_size, seed=4)[0].contiguous(), layers, model_meta(m, L0, cos, sin), cache)
    return cache, meta


@pytest.mark.parametrize("fmt", ["bf16", FMT])
@pytest.mark.parametrize("weights", ["bf16", "w8"])
@pytest.mark.parametrize("fused", [True, False])
def test_extend_pass(fused, weights, fmt, monkeypatch):
    """decoder_extend of 19 rows on 21 cached rows.  Fused: the prompt pass's walk with attention over the cache rows (an fp8_e4m3 cache:
    plain projection, rotation, quantising append); plain (prefill_fused off): the rotation and the append as launches of their own."""
    from metamorph_amd import functional as F
    cfg, m, _ = model_of("h1024", weights)
    h, layers, n = cfg.hidden_size, m.model.layers[:NL], 19
    monkeypatch.setitem(F.VARIANTS, "prefill_fused", fused)
    cache, meta = filled(m, cfg, layers, fmt, 21, 48)
    assert F.VARIANTS["prefill_splitk"] and splits(meta, h, n) and (weights == "bf16" or all_on_bytes(m, n, 64))
    x = embeds(1, n, h, seed=5)[0].contiguous()
    log, _ = logged(monkeypatch, layers, lambda: F.decoder_extend(x, layers, meta, cache))
    append = ["kv_quant_f8", "kv_quant_f8"] if fmt == FMT else ["rows_gather", "rows_gather"]
    attn = "attn_extend_f8" if fmt == FMT else "attn_extend"
    if fused:
        step = ["gemm_splitk", "rope_qk_"] + append + [attn] if fmt == FMT else ["gemm_splitk_rope_append", attn]
        check(log, fused_walk(step, ["gemm_splitk_swiglu"], weights), f"extend fused {weights} {fmt}")
    else:
        check(log, plain_walk(["rope_qk_"] + append + [attn], weights), f"extend plain {weights} {fmt}")
    assert cache.lengths == [21 + n]


@pytest.mark.parametrize("fmt", ["bf16", FMT])
@pytest.mark.parametrize("weights", ["bf16", "w8"])
@pytest.mark.parametrize("fused", [True, False])
def test_shared_extend_pass(fused, weights, fmt, monkeypatch):
    """decoder_extend_shared of 5 rows for each of 3 sequences on a 16-row shared prefix (15 rows in the projections): both routes rotate
    and append outside the projection; the bf16 append of sequences that start at one row is a tensor copy, no op of ours."""
    from metamorph_amd import functional as F
    cfg, m, _ = model_of("h1024", weights)
    h, layers, B, n, S = cfg.hidden_size, m.model.layers[:NL], 3, 5, 16
    monkeypatch.setitem(F.VARIANTS, "prefill_fused", fused)
    cache, meta, cos, sin = new_cache(m, cfg, S + n + 4, fmt=fmt, batch=B)
    with torch.no_grad():
        F.decoder_prefill(embeds(1, S, h, seed=6)[0].contiguous(), layers, model_meta(m, S, cos, sin), cache, row=0)
    cache.set_lengths([S] * B)
    cache.set_shared(S)
    assert F.VARIANTS["prefill_splitk"] and splits(meta, h, B * n) and (weights == "bf16" or all_on_bytes(m, B * n, 64))
    x = embeds(B, n, h, seed=7)
    log, _ = logged(monkeypatch, layers, lambda: F.decoder_extend_shared(x, layers, meta, cache))
    step = ["rope_qk_"] + (["kv_quant_f8", "kv_quant_f8", "attn_extend_shared_f8"] if fmt == FMT else ["attn_extend_shared"])
    if fused:
        check(log, fused_walk(["gemm_splitk"] + step, ["gemm_splitk_swiglu"], weights), f"extend_shared fused {weights} {fmt}")
    else:
        check(log, plain_walk(step, weights), f"extend_shared plain {weights} {fmt}")
    assert cache.lengths == [S + n] * B


def decode_step(m, cfg, B, fmt, monkeypatch):
    """one decoder_decode_row of B sequences that hold 5 rows each, logged"""
    from metamorph_amd import functional as F
    h, layers = cfg.hidden_size, m.model.layers[:NL]
    cache, meta, cos, sin = new_cache(m, cfg, 12, fmt=fmt, batch=B)
    mb = model_meta(m, 5, cos, sin)
    mb.B = B
    with torch.no_grad():
        F.decoder_prefill(embeds(B, 5, h, seed=8).reshape(B * 5, h), layers, mb, cache)
    x = embeds(1, B, h, seed=9)[0].contiguous()
    log, _ = logged(monkeypatch, layers, lambda: F.decoder_decode_row(x, layers, meta, cache, cos, sin))
    assert cache.lengths == [6] * B
    return log, meta


@pytest.mark.parametrize("fmt", ["bf16", FMT])
@pytest.mark.parametrize("weights", ["bf16", "w8"])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("B", [17, 33])
def test_wide_decode_step(B, fused, weights, fmt, monkeypatch):
    """_decode_rows_gemm through decoder_decode_row: 17 sequences (the first past the GEMV route) and 33 (the first past the 32-row gate|up
    GEMV, which these narrow gate|up weights do not take at 17 either).  Fused: nine launches per layer (ten on an fp8_e4m3 cache) plus the
    first layer's input norm; unfused: thirteen."""
    from metamorph_amd import functional as F, ops
    cfg, m, _ = model_of("h1024", weights)
    monkeypatch.setitem(F.VARIANTS, "decode_wide_fused", fused)
    log, meta = decode_step(m, cfg, B, fmt, monkeypatch)
    assert splits(meta, cfg.hidden_size, B) and not ops.gemv_rows32_units(meta.I // 2) and (weights == "bf16" or all_on_bytes(m, B))
    step = ["rope_kv_append_f8_", "attn_decode_f8"] if fmt == FMT else ["rope_kv_append_", "attn_decode"]
    if fused:
        step = ["gemm_splitk"] + step if fmt == FMT else ["gemm_splitk_rope_append", "attn_decode"]
        check(log, fused_walk(step, ["gemm_splitk_swiglu"], weights), f"decode {B} fused {weights} {fmt}")
        assert launches(log) == NL * (10 if fmt == FMT else 9) + 1
    else:
        check(log, plain_walk(step, weights, on_bytes=True), f"decode {B} unfused {weights} {fmt}")
        assert launches(log) == NL * 13                        # (the quantising append stands where the bf16 append stood)
    assert "gemv_swiglu" not in log


_WIDE = []


def test_wide_decode_step_gate_up_on_the_gemv(monkeypatch):
    """17 sequences on gate|up weights wide enough for the GEMV's second row group (I = 10496: ops.gemv_rows32_units): the fused step runs
    gate|up + SwiGLU as ONE launch of the GEMV -- eight launches per layer -- and 33 sequences go back to the split projection."""
    from metamorph_amd import functional as F, ops
    if not _WIDE:
        cfg = tiny_cfg(hidden_size=1024, intermediate_size=10496, num_attention_heads=8, num_key_value_heads=2, num_hidden_layers=NL)
        _WIDE.append((cfg, hip_model(cfg, init_state_dict(cfg, seed=31, dtype=torch.bfloat16)).eval()))
    cfg, m = _WIDE[0]
    assert F.VARIANTS["decode_wide_fused"] and F.VARIANTS["decode_wide_gu_gemv"] and ops.gemv_rows32_units(cfg.intermediate_size // 2)
    log, meta = decode_step(m, cfg, 17, "bf16", monkeypatch)
    assert splits(meta, cfg.hidden_size, 17)
    check(log, fused_walk(["gemm_splitk_rope_append", "attn_decode"], ["gemv_swiglu"], "bf16"), "decode 17 fused, gate|up on the GEMV")
    assert launches(log) == NL * 8 + 1
    log, _ = decode_step(m, cfg, 33, "bf16", monkeypatch)
    check(log, fused_walk(["gemm_splitk_rope_append", "attn_decode"], ["gemm_splitk_swiglu"], "bf16"), "decode 33 fused, wide gate|up")
    assert launches(log) == NL * 9 + 1


def rows16_walk(B, fused, weights, fmt, attn):
    """The decode step of up to 16 sequences, NL layers (_decode_rows16): every projection a GEMV (a quantised layer: its record's, and no
    params_ready -- the record holds the bytes).  Fused, bf16 cache: norm + q|k|v + RoPE + append in one GEMV, norm + gate|up + SwiGLU in
    another, the norms as launches of their own beyond decode_fold_rows rows; an fp8_e4m3 cache: norm, plain q|k|v GEMV, quantising append.
    Unfused: nine launches per layer."""
    r = (lambda n: "w8." + n) if weights == "w8" else (lambda n: n)
    append = "rope_kv_append_f8_" if fmt == FMT else "rope_kv_append_"
    norm = [] if B <= 4 else ["rmsnorm_fwd"]
    if not fused:
        body = ["rmsnorm_fwd", r("gemv"), append, attn, r("gemv"), "rmsnorm_fwd", r("gemv"), "swiglu_fwd", r("gemv")]
    elif fmt == FMT:
        body = ["rmsnorm_fwd", r("gemv"), append, attn, r("gemv")] + norm + [r("gemv_swiglu"), r("gemv")]
    else:
        body = norm + [r("gemv_rope_append"), attn, r("gemv")] + norm + [r("gemv_swiglu"), r("gemv")]
    return [([f"ready:{i}"] if weights == "bf16" else []) + body for i in range(NL)]


@pytest.mark.parametrize("fmt", ["bf16", FMT])
@pytest.mark.parametrize("weights", ["bf16", "w8"])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("B", [3, 6])
def test_decode_step_of_up_to_16(B, fused, weights, fmt, monkeypatch):
    """_decode_rows16 through decoder_decode_row: 3 sequences (the norms folded into the GEMVs: five launches per layer, seven on an
    fp8_e4m3 cache) and 6 (past decode_fold_rows: seven and eight); decode_fused off: nine."""
    from metamorph_amd import functional as F
    cfg, m, _ = model_of("h1024", weights)
    assert F.VARIANTS["decode_fold_rows"] == 4
    monkeypatch.setitem(F.VARIANTS, "decode_fused", fused)
    log, _ = decode_step(m, cfg, B, fmt, monkeypatch)
    check(log, rows16_walk(B, fused, weights, fmt, "attn_decode_f8" if fmt == FMT else "attn_decode"), f"decode {B} fused={fused} {weights} {fmt}")
    per_layer = 9 if not fused else (5 if B <= 4 else 7) + (fmt == FMT) * (2 if B <= 4 else 1)
    assert launches(log) == NL * per_layer


def shared_cache(m, cfg, layers, fmt, B, S, cap):
    """B sequences on the S rows of one prompt, stored once in sequence 0"""
    from metamorph_amd import functional as F
    cache, meta, cos, sin = new_cache(m, cfg, cap, fmt=fmt, batch=B)
    with torch.no_grad():
        F.decoder_prefill(embeds(1, S, cfg.hidden_size, seed=6)[0].contiguous(), layers, model_meta(m, S, cos, sin), cache, row=0)
    cache.set_lengths([S] * B)
    return cache, meta, cos, sin


@pytest.mark.parametrize("fmt", ["bf16", FMT])
@pytest.mark.parametrize("weights", ["bf16", "w8"])
@pytest.mark.parametrize("own_rows", [None, 4])
def test_decode_step_on_a_shared_prefix(own_rows, weights, fmt, monkeypatch):
    """The step of 3 sequences on a 16-row shared prefix, without and with a table of own rows (the beams): the launches of the plain step,
    attn_decode_shared(_f8) where attn_decode(_f8) stood."""
    from metamorph_amd import functional as F
    cfg, m, _ = model_of("h1024", weights)
    h, layers, B, S = cfg.hidden_size, m.model.layers[:NL], 3, 16
    cache, meta, cos, sin = shared_cache(m, cfg, layers, fmt, B, S, S + 8)
    cache.set_shared(S, own_rows=own_rows)
    assert (cache.own_block is not None) == (own_rows is not None) and F.VARIANTS["decode_fused"]
    x = embeds(1, B, h, seed=9)[0].contiguous()
    log, _ = logged(monkeypatch, layers, lambda: F.decoder_decode_row(x, layers, meta, cache, cos, sin))
    check(log, rows16_walk(B, True, weights, fmt, "attn_decode_shared_f8" if fmt == FMT else "attn_decode_shared"),
          f"shared decode own_rows={own_rows} {weights} {fmt}")
    assert cache.lengths == [S + 1] * B


@pytest.mark.parametrize("fmt", ["bf16", FMT])
@pytest.mark.parametrize("weights", ["bf16", "w8"])
@pytest.mark.parametrize("fused", [True, False])
def test_ragged_extend_pass(fused, weights, fmt, monkeypatch):
    """decoder_extend_ragged of 5 / 9 / 7 rows on sequences holding 0 / 6 / 11 (21 packed rows): on both routes one
    rope_kv_append_rows_(_f8_) and one attn_extend_ragged(_f8) per layer behind the plain projection."""
    from metamorph_amd import functional as F
    cfg, m, _ = model_of("h1024", weights)
    h, layers, lens, held = cfg.hidden_size, m.model.layers[:NL], [5, 9, 7], [0, 6, 11]
    monkeypatch.setitem(F.VARIANTS, "prefill_fused", fused)
    cache, meta, cos, sin = new_cache(m, cfg, 24, fmt=fmt, batch=3)
    with torch.no_grad():
        for b, L0 in enumerate(held):
            if L0:
                F.decoder_prefill(embeds(1, L0, h, seed=10 + b)[0].contiguous(), layers, model_meta(m, L0, cos, sin), cache, row=b)
    assert cache.lengths == held and F.ragged_pass_supported(meta)
    assert F.VARIANTS["prefill_splitk"] and splits(meta, h, sum(lens)) and (weights == "bf16" or all_on_bytes(m, sum(lens), 64))
    xs = [embeds(1, n, h, seed=20 + j)[0].contiguous() for j, n in enumerate(lens)]
    log, out = logged(monkeypatch, layers, lambda: F.decoder_extend_ragged(xs, layers, meta, cache))
    step = ["rope_kv_append_rows_f8_", "attn_extend_ragged_f8"] if fmt == FMT else ["rope_kv_append_rows_", "attn_extend_ragged"]
    if fused:
        check(log, fused_walk(["gemm_splitk"] + step, ["gemm_splitk_swiglu"], weights), f"ragged fused {weights} {fmt}")
    else:
        check(log, plain_walk(step, weights), f"ragged plain {weights} {fmt}")
    assert cache.lengths == [p + n for p, n in zip(held, lens)] and [int(o.shape[0]) for o in out] == lens


@pytest.mark.parametrize("fmt", ["bf16", FMT])
@pytest.mark.parametrize("weights", ["bf16", "w8"])
@pytest.mark.parametrize("B", [1, 3])
def test_plain_prompt_pass(B, weights, fmt, monkeypatch):
    """decoder_prefill on the training path's layer forward: one sequence of 21 rows with prefill_fused off, and a batch of 3 prompts of
    7 rows (never fused).  The rows enter the cache behind each layer: kv_quant_f8 twice (fp8_e4m3), rows_gather twice (one bf16
    sequence), a tensor copy -- no op of ours -- for the bf16 batch."""
    from metamorph_amd import functional as F, ops
    cfg, m, _ = model_of("h1024", weights)
    h, layers, L = cfg.hidden_size, m.model.layers[:NL], 21 // B
    monkeypatch.setitem(F.VARIANTS, "prefill_fused", False)
    cache, meta, cos, sin = new_cache(m, cfg, L + 4, fmt=fmt, batch=B)
    mb = model_meta(m, L, cos, sin)
    mb.B = B
    x = embeds(B, L, h, seed=8).reshape(B * L, h)
    wqkv = torch.empty(((meta.Hq + 2 * meta.Hkv) * meta.d, h), device=x.device, dtype=x.dtype)
    assert F.VARIANTS["prefill_splitk"] and not ops.gemm_rope_supported(x, wqkv, meta.Hq, meta.Hkv, meta.d, cos)
    assert not ops.gemm_swiglu_supported(x, torch.empty((2 * meta.I, h), device=x.device, dtype=x.dtype), meta.I)
    log, _ = logged(monkeypatch, layers, lambda: F.decoder_prefill(x, layers, mb, cache))
    store = ["kv_quant_f8", "kv_quant_f8"] if fmt == FMT else (["rows_gather", "rows_gather"] if B == 1 else [])
    check(log, [layer + store for layer in plain_walk(["rope_qk_", "attn_fwd"], weights)], f"prefill plain B={B} {weights} {fmt}")
    assert cache.lengths == [L] * B


@pytest.mark.parametrize("fmt", ["bf16", FMT])
@pytest.mark.parametrize("weights", ["bf16", "w8"])
def test_shared_extend_pass_unequal_past(weights, fmt, monkeypatch):
    """decoder_extend_shared of 5 rows for each of 3 sequences that hold 16 / 18 / 17 rows on a 16-row shared prefix: the append goes
    sequence by sequence, rows_gather twice (kv_quant_f8 twice) each, then ONE attention call."""
    from metamorph_amd import functional as F
    cfg, m, _ = model_of("h1024", weights)
    h, layers, B, n, S = cfg.hidden_size, m.model.layers[:NL], 3, 5, 16
    cache, meta, cos, sin = shared_cache(m, cfg, layers, fmt, B, S, S + n + 4)
    cache.set_shared(S)
    past = [S, S + 2, S + 1]
    assert F.VARIANTS["prefill_fused"] and F.VARIANTS["prefill_splitk"] and splits(meta, h, B * n) and (weights == "bf16" or all_on_bytes(m, B * n, 64))
    x = embeds(B, n, h, seed=7)
    log, _ = logged(monkeypatch, layers, lambda: F.decoder_extend_shared(x, layers, meta, cache, past=past))
    append = (["kv_quant_f8", "kv_quant_f8"] if fmt == FMT else ["rows_gather", "rows_gather"]) * B
    attn = "attn_extend_shared_f8" if fmt == FMT else "attn_extend_shared"
    check(log, fused_walk(["gemm_splitk", "rope_qk_"] + append + [attn], ["gemm_splitk_swiglu"], weights), f"extend_shared unequal past {weights} {fmt}")
    assert cache.lengths == [p + n for p in past]
