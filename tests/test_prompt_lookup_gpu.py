"""Prompt-lookup speculative decoding on the device: mm355_ngram_draft_rows and mm355_spec_verify_advance against their host models
(functional.prompt_lookup_host, functional.spec_advance_host), functional.decoder_verify_rows against n decoder_decode_row steps, and
greedy_decode / generate with prompt_lookup_num_tokens (functional.SpecGreedyLoopGraph) against the reference-recorded loops of
tests/golden/n1_decode_*.npz, against the host models' prediction of its step counts, and against the plain device loop on the near-tie
model of tests/test_greedy_batch_gpu.py."""
import pytest
import torch

from test_extend_pass_gpu import check_logits, embeds, model_meta, model_of  # noqa: E402
from test_greedy_batch_gpu import (ADV, DIVERGE_SEEDS, END, EOT, MAX_NEW, START, _advance_stream, _batch_kw, _check_pred_z,  # noqa: E402
                                   _diverge_inputs, _diverge_model, _fixture_model)
from test_prompt_lookup_host import lookup_histories  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
EOS_IDS = {128001, EOT}


def i32(x):
    return torch.as_tensor(x, dtype=torch.int32).to(DEV)


# ------------------------------------------------------------------ 1. the drafter against its host model
HAND = ([5, 6, 7, 8, 9, 5, 6], [1, 2, 3, 4], [1, 2, 9, 1, 2], [1, 2, 10, 7, 1, 2, 11, 7, 1, 2], [2, 20, 1, 2, 30, 1, 2], [1, 2, 7, -200, 8, 1, 2],
        [1, 2, 7, 100, 8, 1, 2], [1, 2, -200, 5, 1, 2, 6, 1, 2], [1, 2, -200, 5, 2, 8, 1, 2], [-200, 4, -200])


@pytest.mark.parametrize("K,N", [(1, 1), (4, 2), (15, 4)])
@pytest.mark.parametrize("B", [1, 3, 17])
def test_drafter_equals_the_host_model(B, K, N):
    """the histories of the host test (the 5000-id ones first: longer than one pass of the workgroup) and its hand cases, B = 17 with
    done and in-image sequences among them: drafts, their count, the input rows, positions and the mode mask"""
    from metamorph_amd import functional as F, ops
    C, rows, h, n = 100, 128, 264, K + 1
    pool = sorted((hh for hh, _ in lookup_histories()), key=len, reverse=True) + [list(x) for x in HAND]
    hists = pool[:B]
    cap = max(len(x) for x in hists) + 3
    hist = torch.ones((B, cap), dtype=torch.int32)               # (behind a history: a valid id, so that a read past its end would show)
    for b, x in enumerate(hists):
        hist[b, :len(x)] = torch.tensor(x, dtype=torch.int32)
    done = [int(B > 3 and b % 5 == 3) for b in range(B)]
    in_image = [int(B > 3 and b % 5 == 4) * (b + 1) for b in range(B)]
    state = torch.zeros((6, B), dtype=torch.int32)
    state[3], state[0] = torch.tensor(done), torch.tensor(in_image)
    pos = torch.tensor([11 + 3 * b for b in range(B)], dtype=torch.int32)
    g = torch.Generator().manual_seed(5)
    embed = torch.randn(rows, h, generator=g).bfloat16().to(DEV)
    SENT = -7
    drafts, n_draft = torch.full((B, K), SENT, dtype=torch.int32, device=DEV), torch.full((B,), SENT, dtype=torch.int32, device=DEV)
    pos_rows, mask_rows = torch.full((B * n,), SENT, dtype=torch.int32, device=DEV), torch.full((B * n,), SENT, dtype=torch.int32, device=DEV)
    x_in = torch.full((B * n, h), float(SENT), dtype=BF16, device=DEV)
    ops.ngram_draft_rows(hist.to(DEV), i32([len(x) for x in hists]), state.to(DEV), pos.to(DEV), K, N, C, embed, drafts, n_draft, x_in,
                         pos_rows, mask_rows)
    drafts, n_draft, pos_rows, mask_rows, x_in, emb = drafts.cpu(), n_draft.cpu(), pos_rows.cpu(), mask_rows.cpu(), x_in.cpu(), embed.cpu()
    some = 0
    for b, x in enumerate(hists):
        if done[b]:                                              # a finished sequence: its rows' positions, nothing else
            assert drafts[b].eq(SENT).all() and n_draft[b] == SENT and pos_rows[b * n:(b + 1) * n].tolist() == [int(pos[b]) + i for i in range(n)]
            assert mask_rows[b * n:(b + 1) * n].eq(SENT).all() and x_in[b * n:(b + 1) * n].eq(SENT).all(), b
            continue
        want = [] if in_image[b] else F.prompt_lookup_host(x, K, N, C)
        some += bool(want)
        assert int(n_draft[b]) == len(want) and drafts[b].tolist() == want + [-1] * (K - len(want)), (b, len(x), drafts[b].tolist(), want)
        assert pos_rows[b * n:(b + 1) * n].tolist() == [int(pos[b]) + i for i in range(n)], b
        assert mask_rows[b * n:(b + 1) * n].tolist() == [in_image[b]] + [0] * K, b
        assert x_in[b * n].eq(SENT).all(), b                     # row 0 is the advance kernel's
        for j in range(K):
            assert torch.equal(x_in[b * n + 1 + j], emb[want[j]] if j < len(want) else torch.zeros(h, dtype=BF16)), (b, j)
    assert some >= min(B, 3)


# ------------------------------------------------------------------ 2. verify-and-advance against its host model
@pytest.mark.parametrize("caps", [(41, 41), (3, 2)], ids=["roomy logs", "logs of 3 ids and 2 rows"])
@pytest.mark.parametrize("K", [1, 3])
def test_spec_verify_advance_equals_the_host_model(K, caps):
    """In the manner of test_greedy_advance_equals_the_host_model: five sequences, seeded streams over {start, end, an eos id, three plain
    ids} in which a row's id equals its draft with probability 0.7.  The first call is the loop's first iteration (count_step=False)."""
    from metamorph_amd import functional as F, ops
    B, h, Dz, steps, max_new, n = 5, 256, 1152, 40, 30, K + 1
    token_cap, z_cap = caps
    R, hist_cap, acc_cap = B * n, 4 + 41, steps
    ids = _advance_stream(R, 2 * steps, seed=7 + K)               # [2 * steps, R]: drafts and ids that are no draft
    g = torch.Generator().manual_seed(11)
    hit = torch.rand(steps, R, generator=g) < 0.7
    nds = torch.randint(0, K + 1, (steps, B), generator=g)
    embed = torch.randn(ADV["rows"], h, generator=g).bfloat16().to(DEV)
    fed_t = torch.randn(steps, R, h, generator=g).bfloat16().to(DEV)
    z_t = torch.randn(steps, R, Dz, generator=g).bfloat16().to(DEV)
    state = torch.zeros((6, B), dtype=torch.int32, device=DEV)
    live = torch.full((1,), B, dtype=torch.int32, device=DEV)
    SENT_I, SENT_F = -77, -7.0
    tok_log = torch.full((B + 1, token_cap), SENT_I, dtype=torch.int32, device=DEV)            # (row B: padding the kernel must not reach)
    z_log = torch.full((B + 1, z_cap, Dz), SENT_F, dtype=BF16, device=DEV)
    hist = torch.full((B + 1, hist_cap), SENT_I, dtype=torch.int32, device=DEV)
    acc = torch.full((B + 1, acc_cap), SENT_I, dtype=torch.int32, device=DEV)
    look = [[3, 4, 5, 60][:b % 5] for b in range(B)]
    for b in range(B):
        hist[b, :len(look[b])] = i32(look[b])
    hist_len, n_steps = i32([len(x) for x in look]), torch.zeros(B, dtype=torch.int32, device=DEV)
    pos, length = i32([10 + b for b in range(B)]), i32([11 + b for b in range(B)])
    x_in = torch.empty((R, h), dtype=BF16, device=DEV)
    hs = [dict.fromkeys(F.GREEDY_STATE, 0) for _ in range(B)]
    w_tok, w_z = torch.full((B + 1, token_cap), SENT_I, dtype=torch.int32), torch.full((B + 1, z_cap, Dz), SENT_F, dtype=BF16)
    w_hist, w_acc, w_pos = [list(x) for x in look], [[] for _ in range(B)], [10 + b for b in range(B)]
    accepted, finished_at = 0, [None] * B
    args = (ADV["start"], ADV["end"], ADV["N"], max_new, ADV["eos"])

    def launch(t, toks, drafts, nd, count):
        x_in.fill_(SENT_F)
        ops.spec_verify_advance(toks, drafts, nd, ADV["rows"], state, live, embed, fed_t[t], z_t[t], x_in, tok_log[:B], z_log[:B], hist[:B],
                                hist_len, pos, length, acc[:B], n_steps, *args, count_step=count)

    for t in range(steps):
        drafts = ids[2 * t].view(B, n)[:, :K].contiguous()
        nd = nds[t] if t else torch.zeros(B, dtype=torch.long)
        toks = ids[2 * t + 1].view(B, n).clone()
        toks[:, :K] = torch.where(hit[t].view(B, n)[:, :K], drafts, toks[:, :K])
        launch(t, i32(toks.reshape(-1)), i32(drafts), i32(nd), count=t > 0)
        want_x = torch.full((R, h), SENT_F, dtype=BF16)
        for b in range(B):
            s = hs[b]
            its = F.spec_advance_host(s, toks[b].tolist(), drafts[b, :int(nd[b])].tolist(), ADV["start"], ADV["end"], ADV["N"], max_new,
                                      set(ADV["eos"]), token_cap=token_cap, z_cap=z_cap)
            n_tok, n_z = s["n_tokens"] - sum(log == "tok" for log, _ in its), s["n_z"] - sum(log == "z" for log, _ in its)
            for i, (log, _) in enumerate(its):
                r = b * n + i
                if log == "tok":
                    w_tok[b, n_tok] = toks[b, i]
                    w_hist[b].append(int(toks[b, i]))
                    want_x[b * n] = embed[int(toks[b, i])].cpu()
                    n_tok += 1
                elif log == "z":
                    w_z[b, n_z] = z_t[t, r].cpu()
                    want_x[b * n] = fed_t[t, r].cpu()
                    n_z += 1
            if its and t > 0:
                w_acc[b].append(len(its))
                w_pos[b] += len(its)
                accepted += len(its) - 1
            if s["done"] and finished_at[b] is None:
                finished_at[b] = t
        want_state = torch.tensor([[s[k] for s in hs] for k in F.GREEDY_STATE], dtype=torch.int32)
        assert torch.equal(state.cpu(), want_state), (t, state.cpu().tolist(), want_state.tolist())
        assert int(live.cpu()) == sum(1 for s in hs if not s["done"]), t
        assert torch.equal(x_in.cpu(), want_x), t                  # rows 1 .. K and finished sequences: the sentinel, bit for bit
        assert torch.equal(tok_log.cpu(), w_tok) and torch.equal(z_log.cpu(), w_z), t
        hl, ns, hc, ac = hist_len.tolist(), n_steps.tolist(), hist.cpu(), acc.cpu()
        assert hl == [len(x) for x in w_hist] and ns == [len(x) for x in w_acc], (t, hl, ns)
        for b in range(B):
            assert hc[b, :hl[b]].tolist() == w_hist[b] and hc[b, hl[b]:].eq(SENT_I).all(), (t, b)
            assert ac[b, :ns[b]].tolist() == w_acc[b] and ac[b, ns[b]:].eq(SENT_I).all(), (t, b)
        assert hc[B].eq(SENT_I).all() and ac[B].eq(SENT_I).all()
        assert pos.tolist() == w_pos and length.tolist() == [p + 1 for p in w_pos], (t, pos.tolist(), w_pos)
    # the stream exercises what the comparison is for
    assert all(f is not None for f in finished_at) and int(live.cpu()) == 0
    if caps == (41, 41):
        assert len(set(finished_at)) >= 3 and max(s["n_z"] for s in hs) >= 4 and (K == 1 or accepted >= 10), (finished_at, accepted)
        assert any(max(a) == n for a in w_acc if a), w_acc        # a step that used every row
    else:
        assert all(s["n_tokens"] <= 3 and s["n_z"] <= 2 for s in hs) and any(s["n_tokens"] == 3 for s in hs)
    # every sequence done: another call writes nothing
    before = [t.clone() for t in (state, live, tok_log, z_log, hist, hist_len, acc, n_steps, pos, length)]
    launch(0, i32(toks.reshape(-1)), i32(drafts), i32(nds[1]), count=True)
    assert x_in.eq(SENT_F).all()
    for a, b in zip(before, (state, live, tok_log, z_log, hist, hist_len, acc, n_steps, pos, length)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 3. the step's decoder pass against n decode steps
@pytest.mark.parametrize("fmt", ["bf16", "fp8_e4m3"])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_verify_rows_equal_n_decode_steps(B, fmt):
    """K = 3: four rows per sequence in ONE decoder_verify_rows against four decoder_decode_row steps on a copy of the cache; B = 5 is 20
    rows, the route beyond 16.  Logits under the rule of test_extend_pass_gpu.py (2e-2 * scale, argmax equal or a near tie), the cache
    rows below pos + n within 2e-2 * their scale, every other cache row untouched, no length moved.
    The fp8_e4m3 cache stores ROUNDED values, and the rule is asserted on them as it stands, with one counted exception.  The two runs
    attend through different kernels, so layer 1 rounds inputs that differ by a bf16 ulp (2^-8 relative; 0.0039 at the rows' scale, what
    the bf16 cache shows); where a rounding boundary lies between two such inputs they become NEIGHBOURING e4m3 codes, 2^-3 .. 2^-4 of the
    value apart (three mantissa bits), which exceeds the rule's 0.0225 for every value above about 0.18.  An element beyond the rule
    must therefore be exactly that: the same head-row scale in both caches and raw bytes one code apart with one sign; and there may be
    few of them: a boundary falls between inputs one ulp apart for at most 2^-8 / 2^-4 = one element in 16, were every element to
    differ by a whole ulp.  Measured on an MI355X with the first form of this test: one element of sequence 0's K rows, 0.03125 = one
    code at 0.25 .. 0.5."""
    from metamorph_amd import functional as F, ops
    cfg, m, _ = model_of("tiny", "bf16")
    h, n, cap = cfg.hidden_size, 4, 40
    lens = [5, 9, 12, 7, 10][:B]
    layers = m.model.layers

    def filled():
        _, meta = m._decode_meta(1)
        cos, sin = m.model.rope_tables(cap, DEV)
        meta.cos, meta.sin = cos, sin
        c = F.KVCache(cfg.num_hidden_layers, cap, meta.Hkv * meta.d, DEV, Hq=meta.Hq, d=meta.d, batch=B, fmt=fmt)
        for t, v in ((c.k, 7), (c.v, 9), (c.k_scale, 3.0), (c.v_scale, 5.0)):
            if t is not None:
                t.fill_(v)
        return c, meta, cos, sin
    with torch.no_grad():
        ca, meta, cos, sin = filled()
        for b, L in enumerate(lens):
            F.decoder_prefill(embeds(1, L, h, seed=20 + b)[0].contiguous(), layers, model_meta(m, L, cos, sin), ca, row=b)
        cb = filled()[0]
        tensors = lambda c: [t for t in (c.k, c.v, c.k_scale, c.v_scale) if t is not None]      # noqa: E731
        untouched = [t.clone() for t in tensors(cb)]
        for s, t in zip(tensors(ca), tensors(cb)):
            t.copy_(s)
        cb.set_lengths(lens)
        x = embeds(1, B * n, h, seed=31)[0].contiguous()
        seq = torch.stack([F.decoder_decode_row(x[i::n].contiguous(), layers, meta, ca, cos, sin).clone() for i in range(n)], 1)
        pos_rows = (cb.pos_dev.view(B, 1) + torch.arange(n, dtype=torch.int32, device=DEV)).reshape(-1).contiguous()
        blocks = (torch.arange(B * n, dtype=torch.int32) // n).to(DEV)
        got = F.decoder_verify_rows(x, layers, meta, cb, n, pos_rows, blocks, cap)
        assert cb.lengths == lens and cb.pos_dev.tolist() == lens and cb.len_dev.tolist() == [L + 1 for L in lens]
        assert ca.lengths == [L + n for L in lens]
        check_logits(m._rows_logits(got), m._rows_logits(seq.reshape(B * n, h)), f"B={B} {fmt} verify rows")
        Hkv, d = meta.Hkv, meta.d
        for name in ("k", "v"):
            a, b_ = getattr(ca, name), getattr(cb, name)
            if fmt != "bf16":
                sa, sb = getattr(ca, name + "_scale"), getattr(cb, name + "_scale")
            for b, L in enumerate(lens):
                if fmt == "bf16":
                    ra, rb = a[:, b, :L + n].float(), b_[:, b, :L + n].float()
                else:
                    ra = ops.dequant_kv8(a[:, b, :L + n], sa[:, b, :L + n], Hkv, d).float()
                    rb = ops.dequant_kv8(b_[:, b, :L + n], sb[:, b, :L + n], Hkv, d).float()
                err, scale = float((ra - rb).abs().max()), float(ra.abs().max())
                over = (ra - rb).abs() > 2e-2 * scale
                print(f"   B={B} {fmt} {name} rows of sequence {b}: max err {err:.4f} against 2e-2 * {scale:.3f}, {int(over.sum())} of "
                      f"{over.numel()} elements beyond it")
                if fmt == "bf16":
                    assert not bool(over.any()), (name, b, err, scale)
                    continue
                qa, qb = a[:, b, :L + n].int(), b_[:, b, :L + n].int()
                same_scale = (sa[:, b, :L + n] == sb[:, b, :L + n]).repeat_interleave(d, dim=-1)
                neighbours = ((qa - qb).abs() == 1) & ((qa ^ qb) < 128)      # one code apart, one sign (e4m3: sign and magnitude)
                assert int(over.sum()) <= over.numel() // 16, (name, b, int(over.sum()), over.numel())
                assert bool((same_scale & neighbours)[over].all()), (name, b, err, scale)
        for t, u in zip(tensors(cb), untouched):
            for b, L in enumerate(lens):
                assert torch.equal(t[:, b, L + n:], u[:, b, L + n:]), (B, fmt, b)


# ------------------------------------------------------------------ 4. end to end
def predict(ids, n_z, lookup, K, N, C, max_new, num_image_tokens=4):
    """(acc_log, emitted) of ONE sequence as the host models give them for the ids it emitted and the ids it looks up in"""
    from metamorph_amd import functional as F
    sc = (START, END, num_image_tokens, max_new, EOS_IDS)
    st, stream, j = dict.fromkeys(F.GREEDY_STATE, 0), [], 0
    while not st["done"]:                                        # the id of every iteration (an image row's id is not used: 0)
        image_row = st["in_image"] and st["n_img"] < num_image_tokens
        stream.append(0 if image_row else int(ids[j]))
        j += not image_row
        F.greedy_advance_host(st, stream[-1], *sc)
    assert j == len(ids) and st["n_z"] == n_z, (ids, n_z, st)
    s, hist, acc, it = dict.fromkeys(F.GREEDY_STATE, 0), [int(t) for t in lookup], [], 0
    drafts = []
    while not s["done"]:
        toks = (stream[it:it + K + 1] + [-1] * (K + 1))[:K + 1]
        its = F.spec_advance_host(s, toks, drafts, *sc)
        hist += [toks[i] for i, (log, _) in enumerate(its) if log == "tok"]
        if it:
            acc.append(len(its))
        it += len(its)
        drafts = [] if s["done"] or s["in_image"] else F.prompt_lookup_host(hist, K, N, C)
    assert it == len(stream)
    return acc, it


def spec_generate(model, kw, K, lookup=None, N=None, poll=1, graph=True, fmt=None):
    from metamorph_amd import functional as F
    old = F.set_variant("decode_graph", graph)
    model.config.mm355_greedy_poll_steps = poll
    if fmt is not None:
        model.config.mm355_kv_cache_format = fmt
    try:
        model._greedy_loop = None
        extra = {} if lookup is None else {"prompt_lookup_ids": lookup}
        out, embs = model.generate(**kw, prompt_lookup_num_tokens=K, max_matching_ngram_size=N, **extra)
    finally:
        F.set_variant("decode_graph", old)
        del model.config.mm355_greedy_poll_steps
        if fmt is not None:
            model.config.mm355_kv_cache_format = "bf16"
    loop = model._greedy_loop
    assert isinstance(loop, F.SpecGreedyLoopGraph)
    return out, embs, loop


def check_counts(loop, outs, n_zs, lookups, K, N, C, max_new):
    """steps (read every step: poll = 1), emitted and acc_log are the host models' prediction, exactly"""
    want = [predict(o.tolist(), nz, lk, K, N, C, max_new) for o, nz, lk in zip(outs, n_zs, lookups)]
    assert loop.acc_log == [w[0] for w in want] and loop.emitted == [w[1] for w in want], (loop.acc_log, loop.emitted, want)
    assert loop.poll != 1 or loop.steps == max(len(w[0]) for w in want), (loop.steps, want)
    assert loop.cache.lengths == [L0 + sum(w[0]) for L0, w in zip(loop.prompt_lengths, want)]


RECORDED = [START, END, 41, 42, EOT]
OVERLAP = [7, END, 41, 42, EOT, 9]
CORRUPT = [7, END, 41, 43, EOT, 9]
NONE = [7, 9, 11]


@pytest.mark.parametrize("name", ["text", "image_prompt", "image_prompt_rope31"])
def test_one_sequence_with_prompt_lookup_emits_the_reference_recorded_loop(name):
    g, model = _fixture_model(name)
    max_new, C = int(g["max_new_tokens"]), 128258
    kw = _batch_kw(g, 1, max_new_tokens=max_new)
    assert g["tokens"].tolist() == RECORDED and g["pred_z"].shape[0] == 4
    for K, lookup, steps in ((3, OVERLAP, 6), (1, OVERLAP, 7), (3, CORRUPT, None), (3, NONE, None), (3, None, None), (15, OVERLAP, 6)):
        out, emb, loop = spec_generate(model, kw, K, lookup)
        assert isinstance(out, list) and len(out) == 1 and out[0].dtype == torch.int32 and out[0].tolist() == RECORDED, (K, lookup, out)
        _check_pred_z(g, emb, f"{name} K={K} lookup={lookup}")
        used = lookup if lookup is not None else g["input_ids"][0].tolist()      # (generate() hands its `inputs` on)
        check_counts(loop, out, [4], [used], K, 2, C, max_new)
        assert steps is None or loop.steps == steps, (K, lookup, loop.steps, loop.acc_log)
        assert loop.host_reads <= loop.steps + 1 and len(loop.graphs) == 1
    assert spec_generate(model, kw, 3, OVERLAP)[2].steps < 8       # (the plain loop: 8 steps)


@pytest.mark.parametrize("how", ["bf16 cache", "fp8 cache"])
def test_batch_with_lookup_ids_per_sequence(how):
    """Three copies of the recorded prompt, each with other lookup ids.  bf16 cache: pred_z under _check_pred_z.  fp8 cache: the e4m3 K / V
    rows themselves move pred_z off the bf16 recording by more than _check_pred_z's bound (rel err 1.58e-2 against max(1.5 * 8.2e-3,
    1.2e-2) for the speculative loop and 1.56e-2 for the plain loop, measured on an MI355X and printed here), so the yardstick there is the plain device loop on the same
    cache format, which the speculative loop has to reproduce: rel err <= 2e-2 for all rows and for each (measured: 6.3e-3), the bound of
    test_left_padded_batch_gives_every_sequence_what_it_gets_alone for two runs of one model."""
    from test_greedy_batch_gpu import T, rel
    g, model = _fixture_model("image_prompt")
    max_new = int(g["max_new_tokens"])
    lookups = [OVERLAP, CORRUPT, NONE]
    out, embs, loop = spec_generate(model, _batch_kw(g, 3, max_new_tokens=max_new), 3, lookups, fmt="fp8_e4m3" if how == "fp8 cache" else None)
    assert loop.cache.fmt == ("fp8_e4m3" if how == "fp8 cache" else "bf16") and loop.cache.batch == 3
    if how == "fp8 cache":
        model.config.mm355_kv_cache_format = "fp8_e4m3"
        try:
            p_out, p_embs = model.generate(**_batch_kw(g, 3, max_new_tokens=max_new))
            assert model._greedy_loop.cache.fmt == "fp8_e4m3"
        finally:
            model.config.mm355_kv_cache_format = "bf16"
    for b in range(3):
        assert out[b].tolist() == RECORDED, (b, out[b].tolist())
        if how == "bf16 cache":
            _check_pred_z(g, embs[b], f"B=3 {how} sequence {b}")
            continue
        assert p_out[b].tolist() == RECORDED and embs[b].shape == p_embs[b].shape == tuple(g["pred_z"].shape)
        print(f"   B=3 fp8 cache sequence {b}: pred_z rel err vs reference fp32: speculative {rel(embs[b], T(g['pred_z'])):.3e}, plain loop "
              f"{rel(p_embs[b], T(g['pred_z'])):.3e}; speculative against plain {rel(embs[b], p_embs[b]):.3e}")
        assert rel(embs[b], p_embs[b]) <= 2e-2 and all(rel(embs[b][r], p_embs[b][r]) <= 2e-2 for r in range(4)), b
    check_counts(loop, out, [4] * 3, lookups, 3, 2, 128258, max_new)
    assert len({len(a) for a in loop.acc_log}) >= 2              # the sequences took different numbers of steps


def test_prompt_lookup_on_fp8_weights():
    """quantize_decoder_() (FP8 weights, bf16 storage released): the recorded ids (their margins exceed 6 logits) and the step counts the
    host models predict, as on bf16 weights.  pred_z: the quantised model is another model than the recorded one -- every weight is
    rounded to three mantissa bits --, so its rows are held to the one-sequence host loop on the SAME quantised weights, rel err <= 2e-2
    for all rows and for each (the bound of test_left_padded_batch_gives_every_sequence_what_it_gets_alone for two runs of one model);
    the distance to the bf16 recording is printed for both loops (measured on an MI355X: 5.3e-2 and 5.4e-2, against 5.4e-3 between them)."""
    import numpy as np
    import os
    from conftest import GOLDEN
    from oracle.ref_model import decode_fixture_state_dict
    from test_greedy_batch_gpu import T, hip_model, rel, tiny_cfg
    g = np.load(os.path.join(GOLDEN, "n1_decode_image_prompt.npz"))
    cfg = tiny_cfg(num_image_tokens=4)
    model = hip_model(cfg, decode_fixture_state_dict(g, cfg, torch.bfloat16)).eval()
    model.quantize_decoder_(keep_bf16=False)
    max_new = int(g["max_new_tokens"])
    a_ids, a_z = model.generate(**_batch_kw(g, 1, max_new_tokens=max_new))      # the one-sequence host loop on the same weights
    lookups = [OVERLAP, CORRUPT, NONE]
    out, embs, loop = spec_generate(model, _batch_kw(g, 3, max_new_tokens=max_new), 3, lookups)
    for b in range(3):
        same = embs[b].shape == a_z.shape == tuple(g["pred_z"].shape)
        print(f"   fp8 weights sequence {b}: ids {out[b].tolist()}, one-sequence loop {a_ids[0].tolist()}, pred_z rel err against it "
              f"{rel(embs[b], a_z) if same else None}; vs reference fp32: speculative {rel(embs[b], T(g['pred_z'])) if same else None}, "
              f"one-sequence loop {rel(a_z, T(g['pred_z'])) if same else None}")
    for b in range(3):
        assert out[b].tolist() == RECORDED, (b, out[b].tolist())
    check_counts(loop, out, [4] * 3, lookups, 3, 2, 128258, max_new)
    assert a_ids[0].tolist() == RECORDED
    for b in range(3):
        assert embs[b].shape == a_z.shape and rel(embs[b], a_z) <= 2e-2 and all(rel(embs[b][r], a_z[r]) <= 2e-2 for r in range(4)), b


# ------------------------------------------------------------------ 5. the near-tie model: against the plain device loop
# The five prompts of test_greedy_batch_gpu.py, left-padded, 24 new tokens, on its seeds DIVERGE_SEEDS = (6, 92, 299, 117, 58): no other
# seeds were needed.  One run on an MI355X that printed the gaps: under 2e-2 * the logit scale (8.07, a threshold of 0.161) the plain
# device loop meets no near tie on any of the five, so all five are compared to their end (3 / 25 / 25 / 25 / 25 iterations), and the
# speculative run with K = 4 accepts 17 drafts inside the compared span (24 steps are launched either way: sequence 3 needs them).
_NEAR = {}
K_NEAR = 4


def _plain_run():
    """the plain device loop, launched eagerly with the head wrapped: ids, image rows and the fp32 logits of every iteration"""
    from metamorph_amd import functional as F
    if "plain" not in _NEAR:
        _, model = _diverge_model()
        emb, mask = _diverge_inputs(DIVERGE_SEEDS)
        rows = []
        inner = model._head_rows_device

        def head(x, in_image, logits_out):
            out = inner(x, in_image, logits_out)
            rows.append(logits_out.clone())
            return out
        model._head_rows_device = head
        old = F.set_variant("decode_graph", False)
        try:
            ids, zs = model.greedy_decode(None, mask, emb, max_new_tokens=MAX_NEW, output_image=True)
        finally:
            F.set_variant("decode_graph", old)
            del model._head_rows_device
        _NEAR["plain"] = (ids, zs, torch.stack(rows, 0).cpu())
    return _NEAR["plain"]


def _lookups(ids):
    """the plain run's ids with every fifth one replaced"""
    out = []
    for t in ids:
        t = t.tolist()
        t[4::5] = [3] * len(t[4::5])
        out.append(t)
    return out


def _near_run(poll=8, graph=True):
    from metamorph_amd import functional as F
    _, model = _diverge_model()
    emb, mask = _diverge_inputs(DIVERGE_SEEDS)
    old = F.set_variant("decode_graph", graph)
    model.config.mm355_greedy_poll_steps = poll
    try:
        ids, zs = model.greedy_decode(None, mask, emb, max_new_tokens=MAX_NEW, output_image=True, prompt_lookup_num_tokens=K_NEAR,
                                      prompt_lookup_ids=_lookups(_plain_run()[0]))
    finally:
        F.set_variant("decode_graph", old)
        del model.config.mm355_greedy_poll_steps
    return ids, zs, model._greedy_loop


def _near_case():
    if "spec" not in _NEAR:
        _NEAR["spec"] = _near_run()
    return _NEAR["spec"]


def test_near_tie_model_matches_the_plain_loop_up_to_its_first_near_tie():
    """Ids against the plain device loop up to the first iteration at which the plain run's top-two gap is below 2e-2 * the logit scale
    (the rule of tests/test_extend_pass_gpu.py; scale: the largest |logit| of the plain run).  Only iterations that log an id count: an
    image row's id is used by nobody.  At least 3 of the 5 sequences are compared to their end and the compared span holds at least 10
    accepted drafts (DIVERGE_SEEDS meet both, measured on an MI355X)."""
    from metamorph_amd import functional as F
    p_ids, p_zs, logits = _plain_run()
    ids, zs, loop = _near_case()
    scale = float(logits.abs().max())
    whole, accepted = 0, 0
    for b in range(5):
        st, n_it, tie = dict.fromkeys(F.GREEDY_STATE, 0), 0, False
        while not st["done"]:
            row = logits[n_it, b]
            image_row = st["in_image"] and st["n_img"] < 4
            top = torch.topk(row, 2)
            if not image_row and float(top.values[0] - top.values[1]) < 2e-2 * scale:
                tie = True
                break
            F.greedy_advance_host(st, int(top.indices[0]), START, END, 4, MAX_NEW, EOS_IDS)
            n_it += 1
        n_tok, n_z = st["n_tokens"], st["n_z"]
        done_its, acc_b = 1, 0
        for a in loop.acc_log[b]:                                # accepted drafts of the steps that lie wholly inside the compared span
            if done_its + a <= n_it:
                acc_b += a - 1
            done_its += a
        print(f"   sequence {b}: plain run {int(p_ids[b].numel())} ids, compared {n_it} iterations ({n_tok} ids, {n_z} rows), near tie: {tie}, "
              f"accepted drafts in the span {acc_b}, acc_log {loop.acc_log[b]}")
        assert ids[b][:n_tok].tolist() == p_ids[b][:n_tok].tolist(), (b, ids[b].tolist(), p_ids[b].tolist())
        assert zs[b].shape[0] >= n_z and (n_z == 0 or float((zs[b][:n_z].float() - p_zs[b][:n_z].float()).norm()
                                                             / p_zs[b][:n_z].float().norm()) <= 2e-2), b
        accepted += acc_b
        if not tie:
            assert ids[b].tolist() == p_ids[b].tolist() and zs[b].shape[0] == p_zs[b].shape[0], b
            want = predict(ids[b].tolist(), zs[b].shape[0], _lookups(p_ids)[b], K_NEAR, 2, 128258, MAX_NEW)
            assert (loop.acc_log[b], loop.emitted[b]) == want, (b, loop.acc_log[b], want)
            whole += 1
    print(f"   scale {scale:.3f}: {whole} sequences compared to their end, {accepted} accepted drafts, {loop.steps} steps against "
          f"{logits.shape[0] - 1} plain")
    assert whole >= 3 and accepted >= 10, (whole, accepted)


def test_replay_eager_and_polling_give_one_result():
    ids, zs, loop = _near_case()
    assert loop.poll == 8 and len(loop.graphs) == 1
    lookups = _lookups(_plain_run()[0])
    for b in range(5):                                           # whatever the ids are, the counts are the host models' for them
        assert (loop.acc_log[b], loop.emitted[b]) == predict(ids[b].tolist(), zs[b].shape[0], lookups[b], K_NEAR, 2, 128258, MAX_NEW), b
    for graph in (True, False):
        for poll in (1, 5, 8):
            i2, z2, l2 = _near_run(poll=poll, graph=graph)
            assert [t.tolist() for t in i2] == [t.tolist() for t in ids], (graph, poll)
            assert all(torch.equal(a, b) for a, b in zip(z2, zs)), (graph, poll)
            assert l2.acc_log == loop.acc_log and l2.emitted == loop.emitted and l2.cache.lengths == loop.cache.lengths, (graph, poll)
            assert l2.poll == poll and l2.host_reads <= -(-l2.steps // poll) + 1 and l2.steps <= MAX_NEW
            assert len(l2.graphs) == (1 if graph else 0), (graph, poll)
            if poll == 1:
                assert l2.steps == max(len(a) for a in l2.acc_log)
