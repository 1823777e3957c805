"""mm355_attn_decode_shared / mm355_attn_decode_shared_f8 on the device: one query row per sequence over P shared rows (stored once) followed
by the sequence's own rows [P, kv_lens[b]).  Against the fp32 formula on the CPU at close(1e-2, 1e-2) (the bar of test_attn_extend_gpu.py)
with everything the contract says is never read poisoned: rows [0, P) of every own block, shared rows >= P, own rows >= kv_lens[b].  On
sink and cliff scores against fp64 at 2^-7; the e4m3 form bit for bit against the bf16 form on the dequantised bytes; the indexed form over
the identity table bit for bit against the call without a table, in both formats.
Then the loop: n continuations of one prompt through generate(num_return_sequences=n) on the tiny fixture models -- the reference's
recorded walk for every continuation on the shared and on the fan-out route, the draws against the host model, replay against eager
launches, and what the two routes launch."""
import contextlib

import pytest
import torch

import test_greedy_batch_gpu as G  # noqa: E402  (the tiny fixture models)
import test_sample_gpu as S  # noqa: E402  (the sampled loop's recorder and row check)
from test_attn_extend_gpu import close, kv8_cache  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def _ragged(B, lo, hi):
    return tuple(lo + (b * 7 + 3) % (hi - lo + 1) for b in range(B))


#        B  Hq Hkv  d    P   own lengths
CASES = [(1, 8, 2, 128, 1, (1,)),                                 # the smallest case
         (3, 4, 4, 64, 63, (1, 2, 64)),                           # G = 1, ragged tile
         (4, 8, 2, 128, 64, (65,) * 4),                           # exactly one 16-row fragment
         (5, 32, 8, 128, 65, (1, 130, 7, 64, 3)),                 # 20 rows, two waves
         (16, 8, 2, 128, 200, tuple(range(1, 17))),               # a full 64-row tile
         (17, 8, 2, 128, 1100, _ragged(17, 1, 90)),               # two row tiles, key split and merge
         (40, 8, 1, 64, 700, _ragged(40, 1, 70)),                 # G = 8, five row tiles
         (2, 16, 8, 128, 0, (5, 300)),                            # empty prefix
         (3, 8, 2, 128, 513, (0, 0, 1))]                          # no own rows
CASE_IDS = [f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-P{c[4]}" for c in CASES]
PAD = 5                                                           # capacity = longest length + PAD
IDENTITY = (CASES[3], CASES[5])                                   # where the indexed form runs too, over the table that names every row's own block


def _identity(case):
    B, own = case[0], case[5]
    return torch.arange(B, dtype=torch.uint8).view(B, 1).repeat(1, max(own) + 3).to(DEV)


@pytest.fixture(scope="module")
def ops():
    from metamorph_amd import ops as o
    from metamorph_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return o


def formula(q, ksh, vsh, kc, vc, P, lens, Hq, Hkv, d, dtype=torch.float32):
    """q [B, Hq, d], ksh / vsh [>= P, Hkv, d], kc / vc [B, rows, Hkv, d] -> [B, Hq * d]: row b over the shared rows [0, P) followed by its
    own rows [P, lens[b])"""
    B, G = q.shape[0], Hq // Hkv
    out = torch.empty(B, Hq * d, dtype=dtype)
    for b in range(B):
        kk = torch.cat([ksh[:P], kc[b, P:lens[b]]]).to(dtype).transpose(0, 1).repeat_interleave(G, dim=0)       # [Hq, m, d]
        vv = torch.cat([vsh[:P], vc[b, P:lens[b]]]).to(dtype).transpose(0, 1).repeat_interleave(G, dim=0)
        s = (q[b].to(dtype)[:, None, :] @ kk.transpose(1, 2)) * d ** -0.5                                       # [Hq, 1, m]
        out[b] = (torch.softmax(s, dim=-1) @ vv).reshape(Hq * d)
    return out


def poison(ksh, vsh, kc, vc, P, lens, value=float("nan")):
    for t in (ksh, vsh):
        t[P:] = value
    for t in (kc, vc):
        t[:, :P] = value
        for b, m in enumerate(lens):
            t[b, m:] = value


_INPUTS = {}


def inputs(case):
    """(q, ksh, vsh, kc, vc, lens, reference) of a case on the CPU, made once and shared by the tests that need them"""
    if case not in _INPUTS:
        B, Hq, Hkv, d, P, own = case
        lens = [P + x for x in own]
        rows = max(lens) + PAD
        g = torch.Generator().manual_seed(7 + P + sum(own))
        q = (torch.randn(B, Hq, d, generator=g) * 0.7).bfloat16()
        ksh = (torch.randn(P + 3, Hkv, d, generator=g) * 0.7).bfloat16()
        vsh = (torch.randn(P + 3, Hkv, d, generator=g) * 0.7).bfloat16()
        kc = (torch.randn(B, rows, Hkv, d, generator=g) * 0.7).bfloat16()
        vc = (torch.randn(B, rows, Hkv, d, generator=g) * 0.7).bfloat16()
        ref = formula(q, ksh, vsh, kc, vc, P, lens, Hq, Hkv, d)
        poison(ksh, vsh, kc, vc, P, lens)
        _INPUTS[case] = (q, ksh, vsh, kc, vc, lens, ref)
    return _INPUTS[case]


def _ws(ops, B, Hq, Hkv, d, P, bound):
    n = int(ops._L().mm355_attn_decode_shared_ws_floats(B, Hq, Hkv, d, P, bound))
    assert n > 0
    return torch.full((n,), float("nan"), device=DEV, dtype=torch.float32)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_attn_decode_shared_against_the_formula(ops, case):
    B, Hq, Hkv, d, P, own = case
    q, ksh, vsh, kc, vc, lens, ref = inputs(case)
    rows = kc.shape[1]
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    kd, vd = kc.view(B, rows, Hkv * d).to(DEV), vc.view(B, rows, Hkv * d).to(DEV)
    ks, vs = ksh.view(-1, Hkv * d).to(DEV), vsh.view(-1, Hkv * d).to(DEV)
    qd = q.view(B, Hq * d).to(DEV)
    sc = d ** -0.5
    got = ops.attn_decode_shared(qd, ks, vs, kd, vd, ld, P, max(lens), Hq, Hkv, d, sc)
    close(got, ref, 1e-2, 1e-2, f"attn_decode_shared {case}")
    assert torch.equal(ops.attn_decode_shared(qd, ks, vs, kd, vd, ld, P, max(lens), Hq, Hkv, d, sc), got)
    # the capacity as the bound and a workspace sized at that bound, as the token loop does it: the poisoned tails are still never read
    ws = _ws(ops, B, Hq, Hkv, d, P, rows)
    cap = ops.attn_decode_shared(qd, ks, vs, kd, vd, ld, P, rows, Hq, Hkv, d, sc, workspace=ws)
    close(cap, ref, 1e-2, 1e-2, f"attn_decode_shared {case}, bound = capacity")
    assert torch.equal(ops.attn_decode_shared(qd, ks, vs, kd, vd, ld, P, rows, Hq, Hkv, d, sc, workspace=ws), cap)
    if case in IDENTITY:                                          # the indexed form over the identity table: the same bits
        assert torch.equal(ops.attn_decode_shared(qd, ks, vs, kd, vd, ld, P, max(lens), Hq, Hkv, d, sc, own_block=_identity(case)), got)
        assert torch.equal(ops.attn_decode_shared(qd, ks, vs, kd, vd, ld, P, rows, Hq, Hkv, d, sc, own_block=_identity(case)), cap)
    # q and o as column views of a wider tensor (the q block of a fused q|k|v activation; an output block)
    wide_q = torch.full((B, Hq * d + 2 * Hkv * d), float("nan"), device=DEV, dtype=BF16)
    wide_q[:, :Hq * d] = qd
    wide_o = torch.zeros((B, Hq * d + 64), device=DEV, dtype=BF16)
    o_view = wide_o[:, 64:]
    ret = ops.attn_decode_shared(wide_q[:, :Hq * d], ks, vs, kd, vd, ld, P, max(lens), Hq, Hkv, d, sc, out=o_view)
    assert ret.data_ptr() == o_view.data_ptr() and torch.equal(o_view, got) and float(wide_o[:, :64].float().abs().max()) == 0


@pytest.mark.parametrize("kind", ["sink", "own_cliff", "shared_cliff"])
def test_attn_decode_shared_on_hostile_scores(ops, kind):
    """The construction of test_attn_extend_on_hostile_scores against fp64 at 2^-7: a sink at shared key 0 (+40 over a flat rest); a cliff
    where every score sits at -40 except own key kv_lens[b] - 8 at +40, so the own partial and the shared partials differ by about 115 log2
    units at the merge; and the mirror image, the +40 key inside the shared rows with the own rows flat at -40."""
    B, Hq, Hkv, d, P = 6, 32, 8, 128, 2500
    own = [9, 15, 22, 28, 33, 40]
    lens = [P + x for x in own]
    rows = max(lens) + 3
    g = torch.Generator().manual_seed(11)
    q = (torch.randn(B, Hq, d, generator=g) * 0.5).bfloat16()
    ksh = (torch.randn(P + 2, Hkv, d, generator=g) * 0.5).bfloat16()
    kc = (torch.randn(B, rows, Hkv, d, generator=g) * 0.5).bfloat16()
    vsh = torch.randn(P + 2, Hkv, d, generator=g).bfloat16()
    vc = torch.randn(B, rows, Hkv, d, generator=g).bfloat16()
    unit = d ** -0.5 * 8.0
    q[..., 0] = 8.0
    ksh[..., 0] = 0
    kc[..., 0] = 0
    if kind == "sink":
        ksh[0, :, 0] = 40.0 / unit
    else:
        ksh[..., 0] = -40.0 / unit
        kc[..., 0] = -40.0 / unit
        if kind == "own_cliff":
            for b in range(B):
                kc[b, lens[b] - 8, :, 0] = 40.0 / unit
        else:
            ksh[P - 700, :, 0] = 40.0 / unit
    ref = formula(q, ksh, vsh, kc, vc, P, lens, Hq, Hkv, d, dtype=torch.float64)
    poison(ksh, vsh, kc, vc, P, lens)
    got = ops.attn_decode_shared(q.view(B, Hq * d).to(DEV), ksh.view(-1, Hkv * d).to(DEV), vsh.view(-1, Hkv * d).to(DEV),
                                 kc.view(B, rows, Hkv * d).to(DEV), vc.view(B, rows, Hkv * d).to(DEV),
                                 torch.tensor(lens, dtype=torch.int32, device=DEV), P, max(lens), Hq, Hkv, d, d ** -0.5)
    close(got, ref, 2.0 ** -7, 2.0 ** -7, f"attn_decode_shared {kind}")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_attn_decode_shared_f8_equals_the_bf16_form_on_the_dequantised_cache(ops, case):
    B, Hq, Hkv, d, P, own = case
    lens = [P + x for x in own]
    rows = max(lens) + PAD
    k8, ks, v8, vs = kv8_cache(B, rows, Hkv, d, seed=P + d + sum(own))
    s8 = kv8_cache(1, P + 3, Hkv, d, seed=P + d + sum(own) + 1)
    ksh8, kshs, vsh8, vshs = (t[0] for t in s8)
    deq = lambda t8, ts: ops.dequant_kv8(t8, ts, Hkv, d)           # (before anything is poisoned)
    kb, vb, kshb, vshb = deq(k8, ks), deq(v8, vs), deq(ksh8, kshs), deq(vsh8, vshs)
    poison(ksh8, vsh8, k8, v8, P, lens, value=0x7F)                # what is never read: the NaN byte and a NaN scale
    poison(kshs, vshs, ks, vs, P, lens)
    poison(kshb, vshb, kb, vb, P, lens)
    q = (torch.randn(B, Hq * d, generator=torch.Generator().manual_seed(5)) * 0.7).bfloat16().to(DEV)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    D = lambda *ts: [t.to(DEV) for t in ts]
    for bound in (max(lens), rows):
        ref = ops.attn_decode_shared(q, *D(kshb, vshb, kb, vb), ld, P, bound, Hq, Hkv, d, d ** -0.5)
        got = ops.attn_decode_shared_f8(q, *D(ksh8, vsh8, kshs, vshs, k8, v8, ks, vs), ld, P, bound, Hq, Hkv, d, d ** -0.5)
        assert bool(torch.isfinite(got.float()).all()) and torch.equal(got, ref), (case, bound)
        if case in IDENTITY:                                      # the indexed form over the identity table: the same bits
            idx = ops.attn_decode_shared_f8(q, *D(ksh8, vsh8, kshs, vshs, k8, v8, ks, vs), ld, P, bound, Hq, Hkv, d, d ** -0.5,
                                            own_block=_identity(case))
            assert torch.equal(idx, got), (case, bound)


# ------------------------------------------------------------------ the loop: n continuations of one prompt
@contextlib.contextmanager
def route(shared):
    from metamorph_amd import functional as F
    old = F.set_variant("shared_prefix_attn", shared)
    try:
        yield
    finally:
        F.set_variant("shared_prefix_attn", old)


ARGMAX = dict(do_sample=True, temperature=0.7, top_k=1, seed=3)   # top_k = 1 is the argmax; the fixture's decision margins are above 6 logits


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "fan-out"])
@pytest.mark.parametrize("n", [3, 17])
def test_every_continuation_walks_the_reference_recorded_loop(n, shared):
    g, model = G._fixture_model("image_prompt")
    L = int(g["input_ids"].shape[-1])
    with route(shared):
        out, embs = model.generate(**G._batch_kw(g, 1, max_new_tokens=int(g["max_new_tokens"]), num_return_sequences=n, **ARGMAX))
    kv = model._greedy_loop.cache
    assert kv.batch == n and (kv.shared_len > 0) == shared and (not shared or kv.shared_len == kv.lengths[0] - model._greedy_loop.steps >= L)
    assert isinstance(out, list) and isinstance(embs, list) and len(out) == len(embs) == n
    for b in range(n):
        assert out[b].dtype == torch.int32 and out[b].tolist() == g["tokens"].tolist(), (b, out[b].tolist())
        G._check_pred_z(g, embs[b], f"n={n} shared={shared} continuation {b}")
    if n == 3:
        only = model.generate(**{**G._batch_kw(g, 1, max_new_tokens=2, num_return_sequences=n, **ARGMAX), "output_image": False})
        assert isinstance(only, list) and [o.tolist() for o in only] == [g["tokens_max2"].tolist()] * n


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "fan-out"])
def test_continuations_on_an_fp8_kv_cache(shared):
    """held to what test_batched_loop_on_an_fp8_kv_cache asserts"""
    g, model = G._fixture_model("image_prompt")
    model.config.mm355_kv_cache_format = "fp8_e4m3"
    try:
        with route(shared):
            out, embs = model.generate(**G._batch_kw(g, 1, max_new_tokens=int(g["max_new_tokens"]), num_return_sequences=3, **ARGMAX))
        kv = model._greedy_loop.cache
        assert kv.fmt == "fp8_e4m3" and (kv.shared_len > 0) == shared
    finally:
        model.config.mm355_kv_cache_format = "bf16"
    for b in range(3):
        assert out[b].tolist() == g["tokens"].tolist(), (b, out[b].tolist())
        assert embs[b].shape == tuple(g["pred_z"].shape) and bool(torch.isfinite(embs[b].float()).all()) and G._walks_one_image(out[b], embs[b])


def test_every_continuation_draws_from_its_own_stream(monkeypatch):
    """three sampled continuations, eager: every u is philox_uniform_host(seed, stream id, total_out), every id satisfies the host model on
    the logits of its step; stream ids permute the draws; the same seed repeats ids and image rows exactly."""
    from metamorph_amd import functional as F
    g, model = G._fixture_model("image_prompt")
    rec = S._record(monkeypatch, model)
    kw = G._batch_kw(g, 1, max_new_tokens=int(g["max_new_tokens"]), num_return_sequences=3, **S.SAMPLE)
    with route(True):
        ids, embs = S._eager(lambda: model.generate(**kw, seed=1234))
        loop = model._greedy_loop
        assert loop.seed == 1234 and loop.sampler == (1 / 0.7, 50, 0.9) and not loop.graphs and loop.cache.shared_len > 0
        assert len(rec) == loop.steps + 1 and len(ids) == len(embs) == 3
        first = list(rec)
        for step in first:
            for b in range(3):
                assert step["u"][b] == F.philox_uniform_host(1234, b, step["total_out"][b]), (b, step["total_out"])
                S.check_row(step["logits"][b], 0.7, 50, 0.9, step["u"][b], step["tok"][b], step["stats"][b, 0], step["stats"][b, 1], ("shared", b))
        assert len({tuple(s["u"]) for s in first}) == len(first) and len(set(first[0]["u"])) == 3      # (the streams differ)
        del rec[:]
        ids2, embs2 = S._eager(lambda: model.generate(**kw, seed=1234))
        assert [t.tolist() for t in ids2] == [t.tolist() for t in ids] and all(torch.equal(a, b) for a, b in zip(embs2, embs))
        del rec[:]
        kw["max_new_tokens"] = 1                                  # (the first uniforms are all that is compared from here on)
        S._eager(lambda: model.generate(**kw, seed=1234, stream_ids=[2, 0, 1]))
        assert rec[0]["u"] == [first[0]["u"][2], first[0]["u"][0], first[0]["u"][1]]


def _shared_run(poll=None, graph=True, **kw):
    from metamorph_amd import functional as F
    g, model = G._fixture_model("image_prompt")
    old = F.set_variant("decode_graph", graph)
    if poll is not None:
        model.config.mm355_greedy_poll_steps = poll
    try:
        with route(True):
            ids, zs = model.generate(**G._batch_kw(g, 1, max_new_tokens=int(g["max_new_tokens"]), num_return_sequences=5, **kw))
    finally:
        F.set_variant("decode_graph", old)
        if poll is not None:
            del model.config.mm355_greedy_poll_steps
    return [t.tolist() for t in ids], zs, model._greedy_loop


def test_shared_replay_eager_and_polling_are_one_computation():
    kw = dict(S.SAMPLE, seed=99)
    ids, zs, loop = _shared_run(**kw)
    assert loop.graphs and loop.sampler is not None and loop.cache.shared_len > 0
    for graph, poll in ((True, 1), (True, 5), (False, 8)):
        i2, z2, l2 = _shared_run(poll=poll, graph=graph, **kw)
        assert i2 == ids and all(torch.equal(a, b) for a, b in zip(z2, zs)), (graph, poll)
        assert bool(l2.graphs) == graph and l2.poll == poll and l2.cache.shared_len > 0


def _counted(monkeypatch):
    """counting wrappers: rows per decoder_prefill call, and calls of the two attention ops of the step"""
    from metamorph_amd import functional as F
    seen = dict(prefill=[], attn_decode_shared=0, attn_decode=0, attn_decode_shared_f8=0, attn_decode_f8=0)
    prefill = F.decoder_prefill

    def counting_prefill(x, *a, **k):
        seen["prefill"].append(int(x.shape[0]))
        return prefill(x, *a, **k)
    monkeypatch.setattr(F, "decoder_prefill", counting_prefill)
    for name in ("attn_decode_shared", "attn_decode", "attn_decode_shared_f8", "attn_decode_f8"):
        def wrap(*a, _f=getattr(F.ops, name), _n=name, **k):
            seen[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(F.ops, name, wrap)
    return seen


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "fan-out"])
def test_the_prompt_runs_once_and_the_route_picks_the_attention(monkeypatch, shared):
    g, model = G._fixture_model("image_prompt")
    seen = _counted(monkeypatch)
    n, layers = 4, len(model.model.layers)
    with route(shared):
        ids, _ = S._eager(lambda: model.generate(**G._batch_kw(g, 1, max_new_tokens=int(g["max_new_tokens"]), num_return_sequences=n, **ARGMAX)))
    loop = model._greedy_loop
    L = loop.cache.lengths[0] - loop.steps
    assert len(seen["prefill"]) == 1 and seen["prefill"][0] == L and len(ids) == n        # the prompt's L rows once, not n * L
    ran, idle = ("attn_decode_shared", "attn_decode") if shared else ("attn_decode", "attn_decode_shared")
    assert seen[ran] == layers * loop.steps and seen[idle] == 0 and seen["attn_decode_shared_f8"] == seen["attn_decode_f8"] == 0
    assert loop.cache.shared_len == (L if shared else 0) and loop.cache.batch == n


def test_one_return_sequence_is_the_call_without_the_argument(monkeypatch):
    g, model = G._fixture_model("image_prompt")
    seen = _counted(monkeypatch)
    kw = G._batch_kw(g, 1, max_new_tokens=int(g["max_new_tokens"]))
    runs = []
    for extra in ({}, dict(num_return_sequences=None), dict(num_return_sequences=1)):
        model._greedy_loop = None
        out, emb = model.generate(**kw, **extra)
        assert model._greedy_loop is None                         # (one greedy sequence: the host loop, as before)
        assert isinstance(out, list) and len(out) == 1 and out[0].tolist() == g["tokens"].tolist() and torch.is_tensor(emb)
        runs.append((out[0].tolist(), emb))
    assert all(r[0] == runs[0][0] and torch.equal(r[1], runs[0][1]) for r in runs)
    assert seen["attn_decode_shared"] == 0 and len(seen["prefill"]) == 3
    sampled = []
    for extra in ({}, dict(num_return_sequences=1)):              # one sampled sequence: the device loop on a cache of one, nothing shared
        out, emb = model.generate(**kw, **S.SAMPLE, seed=8, **extra)
        assert model._greedy_loop.cache.batch == 1 and model._greedy_loop.cache.shared_len == 0 and torch.is_tensor(emb)
        sampled.append((out[0].tolist(), emb))
    assert sampled[0][0] == sampled[1][0] and torch.equal(sampled[0][1], sampled[1][1]) and seen["attn_decode_shared"] == 0


def test_the_greedy_walk_of_n_copies_through_the_private_argument():
    """_greedy_decode_loop(copies=n, sampler=None): n greedy continuations over the shared cache, all the fixture's recorded walk"""
    g, model = G._fixture_model("image_prompt")
    kw = G._batch_kw(g, 1)
    (_, _, _, _, emb, _, _, _) = model.prepare_inputs_labels_for_multimodal(kw["inputs"], None, None, None, None, kw["images"], image_sizes=None)
    with route(True), torch.no_grad():
        ids, zs = model._greedy_decode_loop(emb, None, G.START, G.END, (128001, G.EOT), int(g["max_new_tokens"]), True, sampler=None, copies=3)
    assert model._greedy_loop.sampler is None and model._greedy_loop.cache.shared_len == emb.shape[1]
    for b in range(3):
        assert ids[b].tolist() == g["tokens"].tolist(), b
        G._check_pred_z(g, zs[b], f"greedy copy {b}")


def test_decoder_extend_refuses_a_shared_cache():
    from metamorph_amd import functional as F
    g, model = G._fixture_model("image_prompt")
    with route(True):
        model.generate(**G._batch_kw(g, 1, max_new_tokens=2, num_return_sequences=3, **ARGMAX))
    kv, meta = model._greedy_loop.cache, model._greedy_loop.args[1]
    assert kv.shared_len > 0
    x = torch.zeros((3, model.config.hidden_size), device=DEV, dtype=BF16)
    with torch.no_grad(), pytest.raises(ValueError, match="shared prefix.*sequences 1.. do not hold the prefix"):
        F.decoder_extend(x, model.model.layers, meta, kv, row=1)
