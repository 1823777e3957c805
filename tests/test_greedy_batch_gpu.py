"""Batched greedy text-and-image decoding on the device: mm355_argmax_rows_f32 against torch.argmax, mm355_greedy_advance against its
host model (functional.greedy_advance_host), and greedy_decode / generate of a batch (functional.GreedyLoopGraph) against the
reference-recorded loops of tests/golden/n1_decode_*.npz and against every sequence decoded alone by the one-sequence host loop."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN  # noqa: E402
from oracle.ref_model import OracleConfig, decode_fixture_state_dict, init_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
START, END, EOT = 128256, 128257, 128009


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def tiny_cfg(**kw):
    base = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=128258,
                v_layers=2, v_intermediate=144, v_image=56, num_image_tokens=4, tokenizer_model_max_length=64)
    base.update(kw)
    return OracleConfig(**base)


def hip_model(cfg, sd):
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_hidden_layers,
               num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads, vocab_size=cfg.vocab_size,
               rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta, max_position_embeddings=cfg.max_position_embeddings,
               tie_word_embeddings=cfg.tie_word_embeddings, **({"rope_scaling": dict(cfg.rope_scaling)} if cfg.rope_scaling else {}))
    geo = dict(hidden_size=cfg.v_hidden, intermediate_size=cfg.v_intermediate, num_hidden_layers=cfg.v_layers, num_attention_heads=cfg.v_heads,
               image_size=cfg.v_image, patch_size=cfg.v_patch, layer_norm_eps=cfg.v_ln_eps)
    return build_model(llm, geo, num_image_tokens=cfg.num_image_tokens, use_vision_ar=cfg.use_vision_ar, normalize_vision=cfg.normalize_vision,
                       apply_softmax=cfg.apply_softmax, image_start_id=cfg.image_start_id, mm_projector_type=cfg.mm_projector_type,
                       image_token_reduction=cfg.image_token_reduction, vision_coef=cfg.vision_coef, max_length=cfg.tokenizer_model_max_length,
                       padding_side=cfg.tokenizer_padding_side, state_dict=sd, device=DEV)


# ------------------------------------------------------------------ 5. argmax
@pytest.mark.parametrize("C", [37, 1000, 128258])
@pytest.mark.parametrize("R", [1, 3, 17])
def test_argmax_rows_equals_torch_argmax(R, C):
    from metamorph_amd import ops
    g = torch.Generator().manual_seed(1000 * R + C)
    rnd = lambda: torch.randn(R, C, generator=g)               # noqa: E731
    far = (5, 4096 + 700) if C > 4096 + 700 else None            # two columns of different 4096-column chunks
    near = (5, 700) if C > 700 else (5, 30)                      # ... and of one chunk
    cases, want = {}, {}
    cases["random"] = rnd()
    x = rnd()
    x[0::2, 0] = 50.0
    x[1::2, C - 1] = 50.0
    cases["first and last column"] = x
    want["first and last column"] = [0 if r % 2 == 0 else C - 1 for r in range(R)]
    for name, cols in (("equal maxima, two chunks", far), ("equal maxima, one chunk", near)):
        if cols is not None:
            x = rnd()
            x[:, cols[0]] = 40.0
            x[:, cols[1]] = 40.0
            cases[name], want[name] = x, [cols[0]] * R
    cases["constant"], want["constant"] = torch.full((R, C), -2.5), [0] * R
    x = torch.full((R, C), float("-inf"))
    x[torch.arange(R), (torch.arange(R) * 7919 + C // 2) % C] = -3.0e38
    cases["-inf and one finite entry"], want["-inf and one finite entry"] = x, [(r * 7919 + C // 2) % C for r in range(R)]
    cases["all -inf"], want["all -inf"] = torch.full((R, C), float("-inf")), [0] * R
    x = rnd()
    x[:, 3] = 9.0
    x[:, 10 if C <= 4096 + 700 else 4096 + 10] = float("nan")
    x[:, near[1] if C <= 4096 + 700 else 3 * 4096 + 500] = float("nan")
    cases["two NaNs and a larger number"], want["two NaNs and a larger number"] = x, [10 if C <= 4096 + 700 else 4096 + 10] * R
    ws = ops.argmax_rows_ws(R, C, DEV)
    for name, x in cases.items():
        got = ops.argmax_rows(x.to(DEV).contiguous(), ws=ws).cpu()
        assert got.dtype == torch.int32
        assert got.tolist() == torch.argmax(x, dim=1).tolist(), name
        if name in want:
            assert got.tolist() == want[name], name


def test_rows_select_picks_rows_by_the_device_mask():
    from metamorph_amd import ops
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn(7, 264, generator=g).bfloat16().to(DEV), torch.randn(7, 264, generator=g).bfloat16().to(DEV)
    mask = torch.tensor([1, 0, 0, 5, 0, -1, 0], dtype=torch.int32, device=DEV)
    out = ops.rows_select(mask, a, b)
    assert torch.equal(out, torch.where(mask[:, None] != 0, a, b))


# ------------------------------------------------------------------ 6. the transition kernel against its host model
ADV = dict(start=60, end=61, eos=(62, 63), plain=(3, 4, 5), N=4, rows=64)


def _advance_stream(B, steps, seed=7):
    """argmax ids per step and sequence from a seeded stream over {start, end, an eos id, three plain ids}"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.tensor([ADV["start"], ADV["end"], ADV["eos"][0], *ADV["plain"]])
    p = torch.tensor([0.25, 0.17, 0.04, 0.18, 0.18, 0.18])
    return ids[torch.multinomial(p.repeat(steps * B, 1), 1, generator=g).view(steps, B)]


@pytest.mark.parametrize("caps", [(41, 41), (3, 2)], ids=["roomy logs", "logs of 3 ids and 2 rows"])
def test_greedy_advance_equals_the_host_model(caps):
    from metamorph_amd import functional as F, ops
    B, h, Dz, steps, max_new = 5, 256, 1152, 40, 30
    token_cap, z_cap = caps
    stream = _advance_stream(B, steps)
    g = torch.Generator().manual_seed(11)
    embed = torch.randn(ADV["rows"], h, generator=g).bfloat16().to(DEV)
    fed_t = torch.randn(steps, B, h, generator=g).bfloat16().to(DEV)
    z_t = torch.randn(steps, B, Dz, generator=g).bfloat16().to(DEV)
    state = torch.zeros((6, B), dtype=torch.int32, device=DEV)
    live = torch.full((1,), B, dtype=torch.int32, device=DEV)
    SENT_I, SENT_F = -77, -7.0
    tok_log = torch.full((B + 1, token_cap), SENT_I, dtype=torch.int32, device=DEV)            # (row B: padding the kernel must not reach)
    z_log = torch.full((B + 1, z_cap, Dz), SENT_F, dtype=torch.bfloat16, device=DEV)
    x_in = torch.empty((B, h), dtype=torch.bfloat16, device=DEV)
    hs = [dict.fromkeys(F.GREEDY_STATE, 0) for _ in range(B)]
    want_tok = torch.full((B + 1, token_cap), SENT_I, dtype=torch.int32)
    want_z = torch.full((B + 1, z_cap, Dz), SENT_F, dtype=torch.bfloat16)
    finished_at = [None] * B
    for t in range(steps):
        tok = stream[t].to(torch.int32).to(DEV)
        x_in.fill_(SENT_F)
        ops.greedy_advance(tok, ADV["rows"], state, live, embed, fed_t[t], z_t[t], x_in, tok_log[:B], z_log[:B], ADV["start"], ADV["end"],
                           ADV["N"], max_new, ADV["eos"])
        want_x = torch.full((B, h), SENT_F, dtype=torch.bfloat16)
        for b in range(B):
            s = hs[b]
            n_tok, n_z = s["n_tokens"], s["n_z"]
            log, nxt = F.greedy_advance_host(s, int(stream[t, b]), ADV["start"], ADV["end"], ADV["N"], max_new, set(ADV["eos"]),
                                             token_cap=token_cap, z_cap=z_cap)
            if log == "tok":
                want_tok[b, n_tok] = int(stream[t, b])
                want_x[b] = embed[int(stream[t, b])].cpu()
            elif log == "z":
                want_z[b, n_z] = z_t[t, b].cpu()
                want_x[b] = fed_t[t, b].cpu()
            if s["done"] and finished_at[b] is None:
                finished_at[b] = t
        want_state = torch.tensor([[s[k] for s in hs] for k in F.GREEDY_STATE], dtype=torch.int32)
        assert torch.equal(state.cpu(), want_state), (t, state.cpu().tolist(), want_state.tolist())
        assert int(live.cpu()) == sum(1 for s in hs if not s["done"]), t
        assert torch.equal(x_in.cpu(), want_x), t                  # finished sequences: the sentinel, bit for bit
        assert torch.equal(tok_log.cpu(), want_tok), t
        assert torch.equal(z_log.cpu(), want_z), t
    # the stream exercises what the comparison is for
    assert all(f is not None for f in finished_at) and int(live.cpu()) == 0
    if caps == (41, 41):
        assert len(set(finished_at)) >= 3, finished_at
        assert max(s["n_z"] for s in hs) >= 4 and any(s["total_out"] == max_new + 1 for s in hs) and any(s["total_out"] <= max_new for s in hs)
    else:
        assert all(s["n_tokens"] <= 3 and s["n_z"] <= 2 for s in hs) and any(s["n_tokens"] == 3 for s in hs) and any(s["n_z"] == 2 for s in hs)


# ------------------------------------------------------------------ 7, 8, 11. reference-pinned
_MODELS = {}


def _fixture_model(name):
    if name not in _MODELS:
        g = np.load(os.path.join(GOLDEN, f"n1_decode_{name}.npz"))
        cfg = tiny_cfg(num_image_tokens=4, **(json.loads(str(g["cfg_json"])) if "cfg_json" in g else {}))
        _MODELS[name] = (g, hip_model(cfg, decode_fixture_state_dict(g, cfg, torch.bfloat16)).eval())
    return _MODELS[name]


def _batch_kw(g, B, **kw):
    images = T(g["images"]).to(DEV).bfloat16().repeat(B, 1, 1, 1) if g["images"].size else None
    return dict(inputs=T(g["input_ids"]).to(DEV).repeat(B, 1), images=images, output_image=True, **kw)


def _check_pred_z(g, emb, who):
    want = T(g["pred_z"])
    assert emb.shape == tuple(want.shape), (who, emb.shape)
    e_hip, e_ref = rel(emb, want), rel(T(g["pred_z_bf16"]), want)
    print(f"   [{who}] pred_z rel err vs reference fp32: hip={e_hip:.3e} reference-bf16={e_ref:.3e}")
    assert e_hip <= max(1.5 * e_ref, 1.2e-2), (who, e_hip, e_ref)
    for r in range(emb.shape[0]):
        assert rel(emb[r], want[r]) <= max(3.0 * e_ref, 2e-2), (who, r)


@pytest.mark.parametrize("B", [3, 17])
def test_batched_generate_emits_the_reference_recorded_loop_for_every_sequence(B):
    """B copies of the fixture's prompt and image through generate(): every sequence walks <image_start> -> four pred_z rows -> <image_end>
    -> text -> <|eot_id|> as the reference recorded it (decision margins > 6 logits).  17 sequences: the decode step's route beyond 16."""
    g, model = _fixture_model("image_prompt")
    out, embs = model.generate(**_batch_kw(g, B, max_new_tokens=int(g["max_new_tokens"])))
    assert isinstance(out, list) and isinstance(embs, list) and len(out) == len(embs) == B
    for b in range(B):
        assert out[b].dtype == torch.int32 and out[b].tolist() == g["tokens"].tolist(), (b, out[b].tolist())
        _check_pred_z(g, embs[b], f"B={B} sequence {b}")
    loop = model._greedy_loop
    assert loop.cache.batch == B and loop.steps <= int(g["max_new_tokens"]) and loop.host_reads <= math.ceil(loop.steps / loop.poll) + 1
    if B == 3:
        for mn in (2, 6):
            o_m, e_m = model.generate(**_batch_kw(g, B, max_new_tokens=mn))
            for b in range(B):
                assert o_m[b].tolist() == g[f"tokens_max{mn}"].tolist() and e_m[b].shape[0] == int(g[f"n_pred_z_max{mn}"]), (mn, b)
                assert torch.equal(e_m[b], embs[b][:e_m[b].shape[0]])
        only = model.generate(**{**_batch_kw(g, B, max_new_tokens=2), "output_image": False})
        assert isinstance(only, list) and [o.tolist() for o in only] == [g["tokens_max2"].tolist()] * B


@pytest.mark.parametrize("name", ["text", "image_prompt", "image_prompt_rope31"])
def test_one_sequence_through_the_device_loop_matches_reference_recorded_loop(name):
    from metamorph_amd import functional as F
    g, model = _fixture_model(name)
    old = F.set_variant("greedy_loop_b1", True)
    try:
        model._greedy_loop = None
        out, emb = model.generate(**_batch_kw(g, 1, max_new_tokens=int(g["max_new_tokens"])))
        assert model._greedy_loop is not None, "the variant did not route one sequence through the device loop"
        for mn in (2, 6):
            o_m, e_m = model.generate(**_batch_kw(g, 1, max_new_tokens=mn))
            assert o_m[0].tolist() == g[f"tokens_max{mn}"].tolist() and e_m.shape[0] == int(g[f"n_pred_z_max{mn}"]), (mn, o_m[0].tolist())
    finally:
        F.set_variant("greedy_loop_b1", old)
    assert isinstance(out, list) and len(out) == 1 and out[0].dtype == torch.int32 and out[0].tolist() == g["tokens"].tolist()
    _check_pred_z(g, emb, f"{name} B=1 device loop")


def _walks_one_image(ids, emb):
    ids = ids.tolist()
    return START in ids and END in ids and ids.index(END) == ids.index(START) + 1 and emb.shape[0] == 4


def _complete_image(ids, emb):
    """<image_start>, four pred_z rows, and an <image_end> after it"""
    ids = ids.tolist()
    return START in ids and END in ids[ids.index(START) + 1:] and emb.shape[0] >= 4


def test_batched_loop_on_an_fp8_kv_cache():
    g, model = _fixture_model("image_prompt")
    model.config.mm355_kv_cache_format = "fp8_e4m3"
    try:
        out, embs = model.generate(**_batch_kw(g, 3, max_new_tokens=int(g["max_new_tokens"])))
        assert model._greedy_loop.cache.fmt == "fp8_e4m3"
    finally:
        model.config.mm355_kv_cache_format = "bf16"
    for b in range(3):
        assert out[b].tolist() == g["tokens"].tolist(), (b, out[b].tolist())
        assert embs[b].shape == tuple(g["pred_z"].shape) and bool(torch.isfinite(embs[b].float()).all()) and _walks_one_image(out[b], embs[b])


# ------------------------------------------------------------------ 9, 10. diverging sequences, left padding
# One seed per prompt, chosen on an MI355X so that the alone runs meet the conditions asserted below (each prompt's alone run depends on
# its own seed only, so the five were searched independently).
DIVERGE_SEEDS = (6, 92, 299, 117, 58)
# Largest |batch logit - alone logit| over the compared steps of this test, measured on MI355X; the gap threshold is twice that.  One
# figure per mode: in token mode the lm_head sees a normed hidden row (logits of +-8), in image mode the projector's output row, whose
# norm -- and with it every logit, the top-two gap and the batch-versus-alone difference -- is two orders of magnitude smaller.  A
# decision can flip only where the gap is below twice the difference of the logits it was taken on, so each iteration is held to the
# threshold of its own mode; under the token-mode figure alone no image-mode iteration of any prompt would ever count as decided (none in
# 20 000 searched prompts), and the conditions asserted below could not be met.
MEASURED_LOGIT_DIFF = {"token": 0.04466, "image": 0.000284}
GAP_THRESHOLD = {k: 2 * v for k, v in MEASURED_LOGIT_DIFF.items()}
LENS, MAX_NEW = (9, 12, 15, 18, 21), 24
_DIV = {}


def _diverge_model():
    """the tiny decode model of test_model_gpu.py with a sparse lm_head in the fixtures' style: <image_start>, <image_end>, <|eot_id|> and 13
    plain ids at 8 x their seeded rows, every other row zero"""
    if "model" not in _DIV:
        cfg = tiny_cfg(num_key_value_heads=1)
        sd = init_state_dict(cfg, seed=5)
        rows = [START, END, EOT] + [41 + 9973 * i for i in range(13)]
        W = torch.zeros_like(sd["lm_head.weight"])
        W[rows] = 8.0 * sd["lm_head.weight"][rows]
        sd["lm_head.weight"] = W
        _DIV["model"] = (cfg, hip_model(cfg, sd).eval())
    return _DIV["model"]


def _prompt(b, seed):
    cfg, _ = _diverge_model()
    g = torch.Generator().manual_seed(1000003 * b + seed)
    return (torch.randn(LENS[b], cfg.hidden_size, generator=g) * 0.5).bfloat16()


def _diverge_inputs(seeds):
    cfg, _ = _diverge_model()
    n = max(LENS)
    emb = torch.zeros(len(LENS), n, cfg.hidden_size, dtype=torch.bfloat16)
    mask = torch.zeros(len(LENS), n, dtype=torch.long)
    for b, L in enumerate(LENS):
        emb[b, n - L:] = _prompt(b, seeds[b])
        mask[b, n - L:] = 1
    return emb.to(DEV), mask.to(DEV)


def _alone_run(b, seed):
    """prompt b alone through the one-sequence host loop (the parent's code: the yardstick): (ids, pred_z rows, per iteration: argmax id,
    top-two logit gap, fp32 logits)"""
    _, model = _diverge_model()
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


def _alone_runs(seeds):
    return [_alone_run(b, seeds[b]) for b in range(len(LENS))]


def _cut(its, thr):
    """(iterations, ids, pred_z rows, whole) of an alone run before the first iteration whose top-two gap is below the threshold of its mode
    (thr: {"token": .., "image": ..}); whole: no such iteration"""
    from metamorph_amd import functional as F
    st = dict.fromkeys(F.GREEDY_STATE, 0)
    for i, (tok, gap, _, in_image) in enumerate(its):
        if gap < thr["image" if in_image else "token"]:
            return i, st["n_tokens"], st["n_z"], False
        F.greedy_advance_host(st, tok, START, END, 4, MAX_NEW, {128001, EOT})
    return len(its), st["n_tokens"], st["n_z"], True


def _batch_run(seeds, poll=None, graph=True):
    from metamorph_amd import functional as F
    _, model = _diverge_model()
    emb, mask = _diverge_inputs(seeds)
    old = F.set_variant("decode_graph", graph)
    if poll is not None:
        model.config.mm355_greedy_poll_steps = poll
    try:
        ids, zs = model.greedy_decode(None, mask, emb, max_new_tokens=MAX_NEW, output_image=True)
    finally:
        F.set_variant("decode_graph", old)
        if poll is not None:
            del model.config.mm355_greedy_poll_steps
    return ids, zs, model._greedy_loop


def _diverge_case():
    if "case" not in _DIV:
        _DIV["case"] = (_alone_runs(DIVERGE_SEEDS), _batch_run(DIVERGE_SEEDS))
    return _DIV["case"]


def test_left_padded_batch_gives_every_sequence_what_it_gets_alone():
    """Five prompts of 9 .. 21 rows, left-padded, 24 new tokens: ids and pred_z rows of every sequence against the same prompt alone through
    the one-sequence loop, up to the first iteration at which the alone run's top-two logit gap is below the GAP_THRESHOLD of its mode (a random-init
    model has near-ties; beyond one the two runs may decode different sequences)."""
    alone, (ids, zs, loop) = _diverge_case()
    assert loop.cache.batch == 5 and loop.cache.lengths == [L + loop.steps for L in LENS]        # padding rows were never cached
    whole, images, ends = 0, 0, set()
    for b, (a_ids, a_z, its) in enumerate(alone):
        n_it, n_tok, n_z, to_end = _cut(its, GAP_THRESHOLD)
        print(f"   sequence {b}: {len(its)} iterations alone, compared {n_it} ({n_tok} ids, {n_z} pred_z rows); alone ids {a_ids.tolist()}")
        assert ids[b][:n_tok].tolist() == a_ids[:n_tok].tolist(), (b, ids[b].tolist(), a_ids.tolist())
        assert zs[b].shape[0] >= n_z and (n_z == 0 or rel(zs[b][:n_z], a_z[:n_z]) <= 2e-2), b
        for r in range(n_z):
            assert rel(zs[b][r], a_z[r]) <= 2e-2, (b, r)
        if to_end:
            assert ids[b].tolist() == a_ids.tolist() and zs[b].shape[0] == n_z
            whole += 1
            ends.add(len(its))
            images += _complete_image(a_ids, a_z)
    assert whole >= 3 and images >= 2 and len({len(its) for _, _, its in alone}) >= 2, (whole, images, ends)


def test_replay_eager_and_polling_are_one_computation(monkeypatch):
    from metamorph_amd import functional as F, ops
    _, (ids, zs, loop) = _diverge_case()
    calls = {"greedy_advance": 0, "argmax_rows": 0}
    for name in calls:
        orig = getattr(ops, name)
        monkeypatch.setattr(F.ops, name, lambda *a, _o=orig, _n=name, **k: (calls.__setitem__(_n, calls[_n] + 1), _o(*a, **k))[1])
    for graph in (True, False):
        for poll in (1, 5, 8):
            calls.update(greedy_advance=0, argmax_rows=0)
            i2, z2, l2 = _batch_run(DIVERGE_SEEDS, poll=poll, graph=graph)
            assert [t.tolist() for t in i2] == [t.tolist() for t in ids], (graph, poll)
            assert all(torch.equal(a, b) for a, b in zip(z2, zs)), (graph, poll)
            assert l2.poll == poll and l2.host_reads <= math.ceil(l2.steps / poll) + 1, (poll, l2.steps, l2.host_reads)
            assert l2.steps <= MAX_NEW
            if graph:
                assert l2.graphs and len(l2.graphs) == 1
                # first iteration + warm-up and capture per attention bound: not once per token
                assert calls["greedy_advance"] <= 3 + 2 * len(l2.graphs) and calls["argmax_rows"] <= 3 + 2 * len(l2.graphs), calls
            else:
                assert not l2.graphs and calls["greedy_advance"] == l2.steps + 1 == calls["argmax_rows"], (calls, l2.steps)


def test_batched_loop_on_fp8_weights():
    """quantize_decoder_() (FP8 weights, bf16 storage released): the batch of three walks start -> 4 rows -> end; ids against the one-sequence
    loop on the same quantised model under the gap rule of the diverging-sequences test."""
    g = np.load(os.path.join(GOLDEN, "n1_decode_image_prompt.npz"))
    cfg = tiny_cfg(num_image_tokens=4)
    model = hip_model(cfg, decode_fixture_state_dict(g, cfg, torch.bfloat16)).eval()
    model.quantize_decoder_(keep_bf16=False)
    its = []
    inner = model._head_row

    def head(x, in_image_mode):
        out = inner(x, in_image_mode)
        top = torch.topk(out[0][0], 2)
        its.append((int(top.indices[0]), float(top.values[0] - top.values[1]), None, bool(in_image_mode)))
        return out
    model._head_row = head
    try:
        a_ids, a_z = model.generate(**_batch_kw(g, 1, max_new_tokens=int(g["max_new_tokens"])))
    finally:
        del model._head_row
    out, embs = model.generate(**_batch_kw(g, 3, max_new_tokens=int(g["max_new_tokens"])))
    n_it, n_tok, n_z, to_end = _cut(its, GAP_THRESHOLD)
    print(f"   fp8 weights: alone ids {a_ids[0].tolist()}, smallest top-two gap {min(i[1] for i in its):.3f}; compared {n_it} of {len(its)} iterations")
    assert len(out) == len(embs) == 3
    for b in range(3):
        assert out[b].dtype == torch.int32 and embs[b].dim() == 2 and embs[b].shape[1] == g["pred_z"].shape[1]
        assert _walks_one_image(out[b], embs[b]), (b, out[b].tolist(), embs[b].shape)
        assert out[b][:n_tok].tolist() == a_ids[0][:n_tok].tolist(), (b, out[b].tolist(), a_ids[0].tolist())
        if to_end:
            assert out[b].tolist() == a_ids[0].tolist()
