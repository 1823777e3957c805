"""A batch of prompts over one prefix cache on the device: functional.decoder_extend_shared (n new rows of each of B sequences on a cache
with a shared prefix, one pass over the weights) against full forwards, its cache discipline and its independence of the padding; then
greedy_decode(shared_prefix_rows=S / "auto"): diverging sequences against each prompt alone through the one-sequence host loop, on the
shared and on the fan-out route, what the route launches, the reference-recorded loop, and replay against eager launches.  The tiny and
the h = 1024 decoders of tests/test_extend_pass_gpu.py, on bf16, fp8_e4m3 and mxfp4 weights; the loop on the sparse-lm_head model and the
fixture models of tests/test_greedy_batch_gpu.py."""
import contextlib
import os

import numpy as np
import pytest
import torch

import test_greedy_batch_gpu as G  # noqa: E402  (the fixture models, the sparse-lm_head model, the gap rule)
import test_sample_gpu as SM  # noqa: E402  (the sampler's arguments, eager launches)
from test_extend_pass_gpu import check_logits, embeds, hip_model, model_meta, new_cache, rel, tiny_cfg  # noqa: E402
from oracle.ref_model import init_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
FMT = "fp8_e4m3"
S, OWN = 21, (3, 7, 1, 19)                                        # the pass: 21 shared rows, own rows per sequence

_MODELS = {}


def _build(size):
    cfg = tiny_cfg() if size == "tiny" else tiny_cfg(hidden_size=1024, intermediate_size=2048, num_attention_heads=8,
                                                     num_key_value_heads=2, num_hidden_layers=3)
    return cfg, hip_model(cfg, init_state_dict(cfg, seed=5 if size == "tiny" else 23, dtype=torch.bfloat16)).eval()


def model_of(size, weights):
    """(cfg, model, reference model), built once per module: the decoders of tests/test_extend_pass_gpu.py.  "w8" / "w4": quantised
    (fp8_e4m3 with power-of-two scales / mxfp4); the reference is a bf16 build holding the dequantised weights, exact in bf16."""
    from metamorph_amd import ops
    key = (size, weights)
    if key not in _MODELS:
        cfg, a = _build(size)
        ref = a
        if weights != "bf16":
            _, ref = _build(size)
            if weights == "w8":
                a.quantize_decoder_(pow2_scales=True)
                deq = lambda rec: rec[0].view(torch.float8_e4m3fn).float() * rec[1][:, None]
            else:
                a.quantize_decoder_(fmt="mxfp4")
                deq = lambda rec: ops.dequant_w4_reference(*rec).to(DEV)
            for la, lb in zip(a.model.layers, ref.model.layers):
                for name, params in (("qkv", [lb.self_attn.q_proj, lb.self_attn.k_proj, lb.self_attn.v_proj]), ("o", [lb.self_attn.o_proj]),
                                     ("gu", [lb.mlp.gate_proj, lb.mlp.up_proj]), ("down", [lb.mlp.down_proj])):
                    w, off = deq(getattr(la.w8, name)), 0
                    assert torch.equal(w.bfloat16().float(), w.float())
                    for p in params:
                        p.weight.data.copy_(w[off:off + p.weight.shape[0]].bfloat16())
                        off += p.weight.shape[0]
        _MODELS[key] = (cfg, a, ref)
    return _MODELS[key]


def _rows(h):
    """the shared rows [S, h] and the own rows of every sequence, [n_b, h] each"""
    e = embeds(1 + len(OWN), S + max(OWN), h, seed=3)
    return e[0, :S].contiguous(), [e[1 + b, :n].contiguous() for b, n in enumerate(OWN)]


_FULL = {}


def full_logits(size, weights, b):
    """ONE llm_forward of the reference model over the S + n_b rows of sequence b: made once and left unchanged"""
    key = (size, weights, b)
    if key not in _FULL:
        cfg, _, ref = model_of(size, weights)
        pre, own = _rows(cfg.hidden_size)
        with torch.no_grad():
            _FULL[key] = ref.llm_forward(inputs_embeds=torch.cat([pre, own[b]], 0)[None], return_dict=True).logits[0].clone()
    return _FULL[key]


def meta_of(m, cache):
    return model_meta(m, 1, *m.model.rope_tables(cache.max_len, DEV))


def shared_pass(m, cfg, fmt="bf16", n_max=max(OWN), fill=None, extra=6):
    """prefix once into sequence 0, set_shared, one decoder_extend_shared pass over the own rows right-padded with zero rows to n_max"""
    from metamorph_amd import functional as F
    h, B = cfg.hidden_size, len(OWN)
    pre, own = _rows(h)
    cache, meta, cos, sin = new_cache(m, cfg, S + n_max + extra, fmt=fmt, batch=B, fill=fill)
    F.decoder_prefill(pre, m.model.layers, model_meta(m, S, cos, sin), cache, row=0)
    cache.set_lengths([S] * B)
    cache.set_shared(S)
    x = torch.zeros((B, n_max, h), device=DEV, dtype=BF16)
    for b, rows in enumerate(own):
        x[b, :OWN[b]] = rows
    return cache, F.decoder_extend_shared(x, m.model.layers, meta, cache)


@pytest.mark.parametrize("size,weights,fmt", [("tiny", "bf16", "bf16"), ("h1024", "bf16", "bf16"), ("tiny", "w8", "bf16"), ("h1024", "w8", "bf16"),
                                              ("tiny", "w4", "bf16"), ("h1024", "bf16", FMT)])
def test_one_shared_extend_pass_gives_the_logits_of_full_forwards(size, weights, fmt):
    """S = 21 shared rows, own rows of 3 / 7 / 1 / 19 per sequence in ONE decoder_extend_shared pass: the logits of every valid row against one
    llm_forward over that sequence's S + n_b rows, by the criterion of test_cached_decode_matches_full_forward"""
    cfg, m, _ = model_of(size, weights)
    with torch.no_grad():
        cache, rows = shared_pass(m, cfg, fmt=fmt)
        assert tuple(rows.shape) == (len(OWN), max(OWN), cfg.hidden_size) and cache.fmt == fmt
        assert cache.lengths == [S + max(OWN)] * len(OWN) and cache.shared_len == S
        for b, n in enumerate(OWN):
            check_logits(m._rows_logits(rows[b, :n].contiguous()), full_logits(size, weights, b)[S:S + n], f"{size} {weights} {fmt} sequence {b}")


def test_the_shared_extend_pass_keeps_the_cache_discipline():
    """on a cache pre-filled with 7.0 / -7.0: lengths and device positions in step, rows [0, S) of blocks 1.. and rows >= S + n_max
    untouched, and the layer-0 K / V of every valid own row those of a one-shot prompt pass over that sequence (rel 6e-3, the bar of
    test_one_extend_pass_gives_the_logits_of_a_full_forward)"""
    from metamorph_amd import functional as F
    cfg, m, _ = model_of("tiny", "bf16")
    B, n_max = len(OWN), max(OWN)
    pre, own = _rows(cfg.hidden_size)
    with torch.no_grad():
        cache, _ = shared_pass(m, cfg, fill=7.0)
        L = S + n_max
        assert cache.lengths == [L] * B and cache.pos_dev.tolist() == [L] * B and cache.len_dev.tolist() == [L + 1] * B
        assert bool((cache.k[:, 1:, :S] == 7.0).all()) and bool((cache.v[:, 1:, :S] == -7.0).all())
        assert bool((cache.k[:, :, L:] == 7.0).all()) and bool((cache.v[:, :, L:] == -7.0).all())
        assert not bool((cache.k[:, 0, :S] == 7.0).any()) and not bool((cache.k[:, :, S:L] == 7.0).any())      # (written: prefix, own and padding rows)
        for b, n in enumerate(OWN):
            one, _, cos, sin = new_cache(m, cfg, S + n + 2)
            F.decoder_prefill(torch.cat([pre, own[b]], 0), m.model.layers, model_meta(m, S + n, cos, sin), one)
            for got, want, what in ((cache.k, one.k, "k"), (cache.v, one.v, "v")):
                r = rel(got[0, b, S:S + n], want[0, 0, S:S + n])
                print(f"   sequence {b}: layer-0 {what} rows {S} .. {S + n - 1} against the one-shot prompt pass: rel {r:.2e}")
                assert r < 6e-3, (b, what, r)
        # a ragged past[]: two more rows per sequence at past[b] = S + n_b (the append goes sequence by sequence), the rows in front kept
        cache2, _ = shared_pass(m, cfg, fill=7.0)
        x = torch.zeros((B, 2, cfg.hidden_size), device=DEV, dtype=BF16)
        past = [S + n for n in OWN]
        cache2.set_lengths(past)
        before = cache2.k[:, :, :S + 1].clone()
        F.decoder_extend_shared(x, m.model.layers, meta_of(m, cache2), cache2)
        assert cache2.lengths == [p + 2 for p in past] and cache2.pos_dev.tolist() == [p + 2 for p in past]
        assert torch.equal(cache2.k[:, :, :S + 1], before)


def test_a_sequence_does_not_see_its_padding():
    """the valid rows of every sequence from the pass padded to n_max = 19 and from the pass padded to 26 zero rows more: another row count
    (other split-K cuts), the same rows"""
    cfg, m, _ = model_of("h1024", "bf16")
    with torch.no_grad():
        _, a = shared_pass(m, cfg)
        cache, b = shared_pass(m, cfg, n_max=max(OWN) + 26)
        assert cache.lengths == [S + max(OWN) + 26] * len(OWN)
        for s, n in enumerate(OWN):
            check_logits(m._rows_logits(b[s, :n].contiguous()), m._rows_logits(a[s, :n].contiguous()), f"sequence {s}: n_max 45 against n_max 19")
            assert bool(torch.isfinite(b[s].float()).all())


def test_decoder_extend_shared_refusals_on_the_device():
    from metamorph_amd import functional as F
    cfg, m, _ = model_of("tiny", "bf16")
    with torch.no_grad():
        cache, _ = shared_pass(m, cfg, extra=2)
        x = torch.zeros((len(OWN), 3, cfg.hidden_size), device=DEV, dtype=BF16)
        meta = meta_of(m, cache)
        with pytest.raises(ValueError, match="capacity of 42 rows is too small for 40 cached \\+ 3 new rows"):
            F.decoder_extend_shared(x, m.model.layers, meta, cache)
        with pytest.raises(ValueError, match="on a shared prefix of 21 rows"):
            F.decoder_extend_shared(x, m.model.layers, meta, cache, past=[21, 20, 21, 21])
        assert cache.lengths == [40] * 4
        cache.set_shared(0)
        with pytest.raises(ValueError, match="needs a cache with a shared prefix"):
            F.decoder_extend_shared(x, m.model.layers, meta, cache, past=[21] * 4)


# ------------------------------------------------------------------ the loop: diverging sequences over one prefix
# Five prompts = one common prefix of 16 rows + own rows of 1 / 4 / 7 / 10 / 13, left-padded, 24 new tokens.  One seed per prompt's own
# rows, searched on an MI355X with the alone runs only (3000 seeds per prompt; kept: walks whose every top-two gap is above 8 x the
# differences tests/test_greedy_batch_gpu.py measured, the longest, one with image rows first) so that the alone runs meet the condition
# asserted below: they walk 25 / 9 / 13 / 8 / 7 iterations, prompts 0 and 4 through image mode.
PREFIX_ROWS, OWN_ROWS, MAX_NEW = 16, (1, 4, 7, 10, 13), G.MAX_NEW
LENS = tuple(PREFIX_ROWS + n for n in OWN_ROWS)
PREFIX_SEED = 4242
DIVERGE_SEEDS = (1507, 2797, 2215, 2051, 201)
# Largest |batch logit - alone logit| over the compared steps of these tests (the shared and the fan-out route, S = 16 and "auto"), measured
# on MI355X, per mode as in tests/test_greedy_batch_gpu.py; the gap threshold is twice that.  (The shared route gave 0.0876 / 0.000348, the
# fan-out route 0.0316 / 0.000268: there the prefix rows are sequence 0's bits and only the extend pass differs from the alone run.)
MEASURED_LOGIT_DIFF = {"token": 0.08758, "image": 0.000348}
GAP_THRESHOLD = {k: 2 * v for k, v in MEASURED_LOGIT_DIFF.items()}
_DIV = {}


def _prompt(b, seed):
    cfg, _ = G._diverge_model()
    pre = torch.randn(PREFIX_ROWS, cfg.hidden_size, generator=torch.Generator().manual_seed(PREFIX_SEED)) * 0.5
    own = torch.randn(OWN_ROWS[b], cfg.hidden_size, generator=torch.Generator().manual_seed(1000003 * b + seed)) * 0.5
    return torch.cat([pre, own], 0).bfloat16()


def _inputs(seeds):
    cfg, _ = G._diverge_model()
    n = max(LENS)
    emb = torch.zeros(len(LENS), n, cfg.hidden_size, dtype=BF16)
    mask = torch.zeros(len(LENS), n, dtype=torch.long)
    for b, L in enumerate(LENS):
        emb[b, n - L:] = _prompt(b, seeds[b])
        mask[b, n - L:] = 1
    return emb.to(DEV), mask.to(DEV)


def alone_run(b, seed):
    """prompt b alone through the one-sequence host loop (the parent's code: the yardstick): (ids, pred_z rows, per iteration: argmax id,
    top-two logit gap, fp32 logits, mode)"""
    _, model = G._diverge_model()
    its = []
    inner = model._head_row

    def head(x, in_image_mode):
        out = inner(x, in_image_mode)
        top = torch.topk(out[0][0], 2)
        its.append((int(top.indices[0]), float(top.values[0] - top.values[1]), out[0][0].clone(), bool(in_image_mode)))
        return out
    model._head_row = head
    try:
        ids, z = model.greedy_decode(None, None, _prompt(b, seed)[None].to(DEV), max_new_tokens=MAX_NEW, output_image=True)
    finally:
        del model._head_row
    return ids[0], z, its


@contextlib.contextmanager
def route(shared, min_rows=1):
    """the shared or the fan-out route; "auto" from min_rows common rows on (the default is the measured 512: these prompts share 16)"""
    from metamorph_amd import functional as F
    old = F.set_variant("shared_prefix_attn", shared), F.set_variant("shared_prefix_min_rows", min_rows)
    try:
        yield
    finally:
        F.set_variant("shared_prefix_attn", old[0])
        F.set_variant("shared_prefix_min_rows", old[1])


def batch_run(seeds, rows, shared=True, poll=None, graph=True, **kw):
    from metamorph_amd import functional as F
    _, model = G._diverge_model()
    emb, mask = _inputs(seeds)
    old = F.set_variant("decode_graph", graph)
    if poll is not None:
        model.config.mm355_greedy_poll_steps = poll
    try:
        with route(shared):
            out = model.greedy_decode(None, mask, emb, max_new_tokens=MAX_NEW, output_image=True, shared_prefix_rows=rows, **kw)
    finally:
        F.set_variant("decode_graph", old)
        if poll is not None:
            del model.config.mm355_greedy_poll_steps
    return out, model._greedy_loop


def _alone():
    if "alone" not in _DIV:
        _DIV["alone"] = [alone_run(b, DIVERGE_SEEDS[b]) for b in range(len(LENS))]
    return _DIV["alone"]


def _batch(rows, shared):
    if (rows, shared) not in _DIV:
        _DIV[(rows, shared)] = batch_run(DIVERGE_SEEDS, rows, shared)
    return _DIV[(rows, shared)]


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "fan-out"])
@pytest.mark.parametrize("rows", [PREFIX_ROWS, "auto"])
def test_prompts_over_one_prefix_give_every_sequence_what_it_gets_alone(rows, shared):
    """ids and pred_z rows of every sequence against the same prompt alone through the one-sequence loop, up to the first iteration at which
    the alone run's top-two logit gap is below the GAP_THRESHOLD of its mode; at least 3 of the 5 are compared to their end, with at least 2
    different lengths"""
    alone = _alone()
    (ids, zs), loop = _batch(rows, shared)
    kv = loop.cache
    assert kv.batch == 5 and kv.lengths == [L + loop.steps for L in LENS] and kv.shared_len == (PREFIX_ROWS if shared else 0)
    whole, ends = 0, set()
    for b, (a_ids, a_z, its) in enumerate(alone):
        n_it, n_tok, n_z, to_end = G._cut(its, GAP_THRESHOLD)
        print(f"   sequence {b}: {len(its)} iterations alone, compared {n_it} ({n_tok} ids, {n_z} pred_z rows); alone ids {a_ids.tolist()}")
        assert ids[b][:n_tok].tolist() == a_ids[:n_tok].tolist(), (b, ids[b].tolist(), a_ids.tolist())
        assert zs[b].shape[0] >= n_z and (n_z == 0 or rel(zs[b][:n_z], a_z[:n_z]) <= 2e-2), b
        for r in range(n_z):
            assert rel(zs[b][r], a_z[r]) <= 2e-2, (b, r)
        if to_end:
            assert ids[b].tolist() == a_ids.tolist() and zs[b].shape[0] == n_z
            whole += 1
            ends.add(len(its))
    assert whole >= 3 and len(ends) >= 2, (whole, ends)


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "fan-out"])
def test_the_prefix_runs_once_and_the_own_rows_in_one_pass(monkeypatch, shared):
    from metamorph_amd import functional as F
    seen = dict(prefill=[], extend_shared=[], extend=[])
    prefill, ext_sh, ext = F.decoder_prefill, F.decoder_extend_shared, F.decoder_extend
    monkeypatch.setattr(F, "decoder_prefill", lambda x, *a, **k: seen["prefill"].append(int(x.shape[0])) or prefill(x, *a, **k))
    monkeypatch.setattr(F, "decoder_extend_shared", lambda x, *a, **k: seen["extend_shared"].append(tuple(x.shape[:2])) or ext_sh(x, *a, **k))
    monkeypatch.setattr(F, "decoder_extend", lambda x, *a, **k: seen["extend"].append(int(x.shape[0])) or ext(x, *a, **k))
    (ids, _), loop = batch_run(DIVERGE_SEEDS, PREFIX_ROWS, shared, graph=False)
    kv = loop.cache
    assert seen["prefill"] == [PREFIX_ROWS] and len(ids) == 5                     # the 16 rows once, not five prompts
    assert kv.lengths == [L + loop.steps for L in LENS]
    if shared:
        assert seen["extend_shared"] == [(5, max(OWN_ROWS))] and seen["extend"] == [] and kv.shared_len == PREFIX_ROWS
    else:
        assert seen["extend_shared"] == [] and seen["extend"] == list(OWN_ROWS) and kv.shared_len == 0
    # without the argument: the parent's route, five prompt passes and nothing shared
    for k in seen:
        del seen[k][:]
    _, model = G._diverge_model()
    emb, mask = _inputs(DIVERGE_SEEDS)
    model.greedy_decode(None, mask, emb, max_new_tokens=2, output_image=True)
    assert seen["prefill"] == list(LENS) and seen["extend_shared"] == [] and model._greedy_loop.cache.shared_len == 0
    # a broken promise is refused before any decoder work
    for k in seen:
        del seen[k][:]
    broken = emb.clone()
    broken[3, max(LENS) - LENS[3] + 5, 0] += 1.0
    with pytest.raises(ValueError, match="sequence 3 differs from sequence 0 at row 5"):
        model.greedy_decode(None, mask, broken, max_new_tokens=2, shared_prefix_rows=PREFIX_ROWS)
    with route(True):
        assert model.greedy_decode(None, mask, broken, max_new_tokens=2, shared_prefix_rows="auto") is not None
    assert model._greedy_loop.cache.shared_len == 5 and seen["prefill"] == [5]
    # "auto" below VARIANTS["shared_prefix_min_rows"] (the default, 512 rows) is the ordinary batch
    for k in seen:
        del seen[k][:]
    model.greedy_decode(None, mask, emb, max_new_tokens=2, shared_prefix_rows="auto")
    assert seen["prefill"] == list(LENS) and seen["extend_shared"] == [] and model._greedy_loop.cache.shared_len == 0


def test_three_copies_walk_the_reference_recorded_loop_over_one_prefix():
    g, model = G._fixture_model("image_prompt")
    with route(True):
        out, embs = model.generate(**G._batch_kw(g, 3, max_new_tokens=int(g["max_new_tokens"]), shared_prefix_rows="auto"))
    loop = model._greedy_loop
    L = loop.cache.lengths[0] - loop.steps
    assert loop.cache.batch == 3 and loop.cache.shared_len == L - 1 and L >= int(g["input_ids"].shape[-1])
    for b in range(3):
        assert out[b].dtype == torch.int32 and out[b].tolist() == g["tokens"].tolist(), (b, out[b].tolist())
        G._check_pred_z(g, embs[b], f"shared prefix, sequence {b}")


def test_replay_eager_and_polling_are_one_computation_over_one_prefix():
    (ids, zs), loop = _batch(PREFIX_ROWS, True)
    assert loop.graphs and loop.cache.shared_len == PREFIX_ROWS
    for graph, poll in ((True, 1), (True, 8), (False, 8)):
        (i2, z2), l2 = batch_run(DIVERGE_SEEDS, PREFIX_ROWS, True, poll=poll, graph=graph)
        assert [t.tolist() for t in i2] == [t.tolist() for t in ids] and all(torch.equal(a, b) for a, b in zip(z2, zs)), (graph, poll)
        assert bool(l2.graphs) == graph and l2.poll == poll and l2.cache.shared_len == PREFIX_ROWS


def test_sampler_and_processors_over_w8_weights_and_the_fp8_cache():
    """the sampler and every logits processor on, fp8_e4m3 weights and the fp8_e4m3 cache, three copies of the image prompt over one
    prefix: captured replay equals eager launches bit for bit"""
    from oracle.ref_model import decode_fixture_state_dict
    g = np.load(os.path.join(G.GOLDEN, "n1_decode_image_prompt.npz"))
    cfg = G.tiny_cfg(num_image_tokens=4)
    model = G.hip_model(cfg, decode_fixture_state_dict(g, cfg, torch.bfloat16)).eval()
    model.quantize_decoder_()
    model.config.mm355_kv_cache_format = FMT
    kw = G._batch_kw(g, 3, max_new_tokens=int(g["max_new_tokens"]), shared_prefix_rows="auto", repetition_penalty=1.3, min_new_tokens=3,
                     suppress_tokens=[41], output_logprobs=True, seed=77, **SM.SAMPLE)
    with route(True):
        ids, zs, logps = model.generate(**kw)
        loop = model._greedy_loop
        assert loop.graphs and loop.processors is not None and loop.sampler is not None and loop.cache.fmt == FMT and loop.cache.shared_len > 0
        i2, z2, l2 = SM._eager(lambda: model.generate(**kw))
    assert not model._greedy_loop.graphs and model._greedy_loop.cache.shared_len == loop.cache.shared_len
    for b in range(3):
        assert ids[b].numel() and 41 not in ids[b].tolist() and logps[b].shape == ids[b].shape and bool((logps[b] <= 0).all())
        assert i2[b].tolist() == ids[b].tolist() and torch.equal(z2[b], zs[b]), b
        assert np.array_equal(l2[b].cpu().numpy().view(np.int32), logps[b].cpu().numpy().view(np.int32)), b
