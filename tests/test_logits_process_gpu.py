"""Logits processors and per-token log-probabilities on the device: mm355_logits_process_rows_f32 against functional.logits_process_host
bit for bit, mm355_token_note_rows_f32 against functional.token_note_host (written entries within 1e-4 + 2^-22 |logp|, everything else
untouched), and both inside functional.GreedyLoopGraph: every step of the eager loop against the host models, replay / eager / polling as
one computation (batch, sampler, n continuations on both routes), and the loop as it was when every option is off."""
import collections

import numpy as np
import pytest
import torch

import test_greedy_batch_gpu as G  # noqa: E402  (the tiny fixture models)
import test_sample_gpu as S  # noqa: E402  (the row families, the eager switch)
from test_shared_prefix_gpu import route  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(R, C) for C in (37, 1000) for R in (1, 3, 17)] + [(3, 128258)]
FAMILIES = S.FAMILIES + ("nan row", "+inf row", "-inf only")
BITMAPS = ("empty", "full", "random 30%", "last word's valid bits", "last word's bits beyond C")
EOS = (128001, G.EOT)


def family(name, R, C, g):
    if name in S.FAMILIES:
        return S.family(name, R, C, g)
    x = torch.randn(R, C, generator=g) * 2.0
    if name == "nan row":
        x[:, C // 3] = float("nan")
    elif name == "+inf row":
        x[:, C // 2] = float("inf")
    else:
        x[:] = float("-inf")
    return x


def bitmap(kind, R, C, g):
    """uint32 [R, words]: one word more than the C logits need where the kind does not care, so that the row stride is not ceil(C / 32)"""
    from metamorph_amd import ops
    need = ops.seen_words(C)
    words = need + (kind in ("empty", "random 30%"))
    ids = np.arange(words * 32)
    if kind == "empty":
        on = np.zeros((R, words * 32), dtype=bool)
    elif kind == "full":
        on = np.broadcast_to(ids < C, (R, words * 32)).copy()
    elif kind == "random 30%":
        on = (torch.rand(R, words * 32, generator=g) < 0.3).numpy()
    elif kind == "last word's valid bits":
        on = np.broadcast_to((ids >= (need - 1) * 32) & (ids < C), (R, words * 32)).copy()
    else:
        on = np.broadcast_to(ids >= C, (R, words * 32)).copy()
    return np.packbits(on.reshape(R, words, 32), axis=-1, bitorder="little").view(np.uint32).reshape(R, words)


def dev_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int32)).to(DEV)


def host_bits(t):
    return t.cpu().numpy().view(np.uint32)


def i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def device_process(x, bits, penalty, total_out, min_new, eos, suppress):
    from metamorph_amd import ops
    d = x.to(DEV).contiguous()
    sup = torch.tensor(list(suppress), dtype=torch.int32).to(DEV) if suppress else None
    ops.logits_process_rows(d, penalty, None if bits is None else dev_bits(bits), torch.tensor(total_out, dtype=torch.int32).to(DEV), min_new,
                            eos, sup)
    return d.cpu().numpy()


def lists_for(C):
    """eos ids and suppressed ids with entries outside [0, C) among them"""
    return [C - 1, 5, -1, C, 2 ** 31 - 1], [9, C + 3, -200, C - 2, -2 ** 31, C, 11 % C]


@pytest.mark.parametrize("R,C", SHAPES)
def test_process_kernel_equals_the_host_model_bit_for_bit(R, C):
    from metamorph_amd import functional as F
    g = torch.Generator().manual_seed(7 * R + C)
    eos, suppress = lists_for(C)
    total_out = [r % 5 for r in range(R)] if R > 1 else [2]      # min_new_tokens = 3: both sides of it
    changed = 0
    for k, name in enumerate(FAMILIES):
        x = family(name, R, C, g)
        for j, kind in enumerate(BITMAPS):
            bits = bitmap(kind, R, C, g)
            penalty = (1.3, 0.7, 2.0)[(k + j) % 3]
            tot = total_out if (k + j) % 2 == 0 else [t + 3 for t in total_out]
            sup = suppress if j % 2 == 0 else []
            got = device_process(x, bits, penalty, tot, 3, eos, sup)
            for r in range(R):
                want = F.logits_process_host(x[r].numpy(), bits[r], penalty, tot[r], 3, eos, sup)
                assert np.array_equal(i32(got[r]), i32(want)), (name, kind, penalty, r, np.nonzero(i32(got[r]) != i32(want))[0][:8])
            changed += int(not np.array_equal(i32(got), i32(x.numpy())))
    assert changed >= (len(FAMILIES) - 1) * 3                    # (the comparison is of edited rows; a row of -inf only cannot change)
    # the steps one at a time, and all off
    x = family("peaked", R, C, g)
    bits = bitmap("random 30%", R, C, g)
    for args in ((1.0, 0, [], []), (1.0, 3, eos, []), (1.0, 0, [], suppress), (1.7, 0, [], []), (1.0, 3, [], [])):
        penalty, min_new, e, sup = args
        got = device_process(x, bits if penalty != 1.0 else None, penalty, [1] * R, min_new, e, sup)
        for r in range(R):
            assert np.array_equal(i32(got[r]), i32(F.logits_process_host(x[r].numpy(), bits[r], penalty, 1, min_new, e, sup))), (args, r)


@pytest.mark.parametrize("R,C", SHAPES)
def test_a_penalised_argmax_gives_way(R, C):
    """non-vacuity: each row's argmax id marked, penalty 2.0 -- the processed row's argmax is another id in every row, in the host model
    first and then on the device"""
    from metamorph_amd import functional as F, ops
    g = torch.Generator().manual_seed(31 * R + C)
    x = family("peaked", R, C, g)
    raw = ops.argmax_rows(x.to(DEV).contiguous()).cpu().tolist()
    assert raw == x.argmax(dim=1).tolist()
    bits = np.stack([F.seen_bits_host([raw[r]], C) for r in range(R)])
    host = [int(np.argmax(F.logits_process_host(x[r].numpy(), bits[r], 2.0, 0, 0, [], None))) for r in range(R)]
    assert all(h != a for h, a in zip(host, raw)), (host, raw)
    got = device_process(x, bits, 2.0, [0] * R, 0, [], [])
    dev = ops.argmax_rows(torch.from_numpy(got).to(DEV)).cpu().tolist()
    assert dev == host


# ------------------------------------------------------------------ the note kernel
N_IMG, CAP = 4, 6
#           done in_image n_img     n_tokens  tok
STATES = [(0, 0, 0, 2, "col"),                                   # logs
          (0, 1, N_IMG, 0, "max"),                               # logs: in image mode, but the image is complete
          (1, 0, 0, 1, "col"),                                   # done
          (0, 1, N_IMG - 1, 1, "col"),                           # an image row
          (0, 0, 0, CAP, "col"),                                 # the log is full
          (0, 0, 0, 1, "C"),                                     # an id that is no column
          (0, 0, 0, 1, "-1"),
          (0, 0, 2, CAP - 1, "-inf")]                            # logs into the last entry; on rows that have one, an id at -inf
NOTE_FAMILIES = ("peaked", "flat", "-inf entries", "spike", "magnitude 350", "nan row", "+inf row", "-inf only")
POISON_F, POISON_W = 12345.678, 0x5A5A5A5A


def logp_band(want):
    return 1e-4 + 2.0 ** -22 * abs(want)


def note_case(x, k0, g):
    """the states of STATES (k0 + r) for the rows of x -> (state [6, R] int32, tok list)"""
    R, C = x.shape
    st = torch.zeros(6, R, dtype=torch.int32)
    tok = []
    for r in range(R):
        done, in_image, n_img, n_tokens, kind = STATES[(k0 + r) % len(STATES)]
        st[0, r], st[1, r], st[3, r], st[4, r] = in_image, n_img, done, n_tokens
        st[2, r], st[5, r] = 3, 1
        minus = torch.nonzero(x[r] == float("-inf")).view(-1)
        if kind == "C":
            tok.append(C)
        elif kind == "-1":
            tok.append(-1)
        elif kind == "max":
            tok.append(int(torch.argmax(x[r])))
        elif kind == "-inf" and len(minus):
            tok.append(int(minus[0]))
        else:
            tok.append(int(torch.randint(0, C, (1,), generator=g)))
    return st, tok


def device_note(x, st, tok, seen0, logp0, want_seen=True, want_logp=True):
    from metamorph_amd import ops
    seen = dev_bits(seen0) if want_seen else None
    logp = torch.from_numpy(logp0.copy()).to(DEV) if want_logp else None
    ops.token_note_rows(x.to(DEV).contiguous(), torch.tensor(tok, dtype=torch.int32).to(DEV), st.to(DEV), N_IMG, CAP, seen=seen, logp_log=logp)
    return (host_bits(seen) if want_seen else None), (logp.cpu().numpy() if want_logp else None)


@pytest.mark.parametrize("R,C", SHAPES)
def test_note_kernel_writes_what_the_host_model_says_and_nothing_else(R, C):
    from metamorph_amd import functional as F, ops
    g = torch.Generator().manual_seed(13 * R + C)
    words = ops.seen_words(C) + 1
    worst, tightest, written, nans, minus_inf = 0.0, 0.0, 0, 0, 0
    for name in NOTE_FAMILIES:
        x = torch.randn(R, C, generator=g) * 350.0 if name == "magnitude 350" else family(name, R, C, g)
        for k0 in range(0, len(STATES), R):
            st, tok = note_case(x, k0, g)
            seen0 = np.full((R, words), POISON_W, dtype=np.uint32)
            seen0[:, ::3] = 0
            logp0 = np.full((R, CAP), POISON_F, dtype=np.float32)
            seen, logp = device_note(x, st, tok, seen0, logp0)
            for r in range(R):
                in_image, n_img, _, done, n_tokens, _ = st[:, r].tolist()
                logs, want = F.token_note_host(x[r].double().numpy(), tok[r], done, in_image, n_img, n_tokens, N_IMG, CAP)
                assert logs == (STATES[(k0 + r) % len(STATES)] in (STATES[0], STATES[1], STATES[7])), (name, k0, r)
                exp_seen, exp_logp = seen0[r].copy(), i32(logp0[r]).copy()
                if logs:
                    exp_seen[tok[r] >> 5] |= np.uint32(1 << (tok[r] & 31))
                    got = float(logp[r, n_tokens])
                    if np.isnan(want):
                        assert np.isnan(got), (name, k0, r, got)
                        nans += 1
                    elif want == -np.inf:
                        assert got == -np.inf, (name, k0, r, got)
                        minus_inf += 1
                    else:
                        assert abs(got - want) <= logp_band(want), (name, k0, r, got, want)
                        worst, tightest = max(worst, abs(got - want)), max(tightest, abs(got - want) / logp_band(want))
                    exp_logp[n_tokens] = i32(logp[r])[n_tokens]
                    written += 1
                assert np.array_equal(seen[r], exp_seen), (name, k0, r)
                assert np.array_equal(i32(logp[r]), exp_logp), (name, k0, r)
    print(f"   R={R} C={C}: {written} entries written, {nans} NaN, {minus_inf} -inf, largest |logp - host| {worst:.3e}, "
          f"at most {tightest:.2f} of the band")
    assert written >= 3 * len(NOTE_FAMILIES) and nans >= 9 and minus_inf >= 1
    # one output at a time: the other one may be null
    x = family("peaked", R, C, g)
    st, tok = note_case(x, 0, g)
    seen0, logp0 = np.zeros((R, words), dtype=np.uint32), np.zeros((R, CAP), dtype=np.float32)
    both = device_note(x, st, tok, seen0, logp0)
    assert np.array_equal(device_note(x, st, tok, seen0, logp0, want_logp=False)[0], both[0])
    assert np.array_equal(i32(device_note(x, st, tok, seen0, logp0, want_seen=False)[1]), i32(both[1]))


def test_both_kernels_repeat_their_bits_and_rows_are_independent():
    g = torch.Generator().manual_seed(23)
    for C in (1000, 128258):
        x = family("peaked", 17, C, g)
        bits = bitmap("random 30%", 17, C, g)
        eos, suppress = lists_for(C)
        tot = [r % 5 for r in range(17)]
        a = device_process(x, bits, 1.3, tot, 3, eos, suppress)
        assert np.array_equal(i32(a), i32(device_process(x, bits, 1.3, tot, 3, eos, suppress)))
        st = torch.zeros(6, 17, dtype=torch.int32)
        st[4] = torch.arange(17) % CAP
        tok = torch.randint(0, C, (17,), generator=g).tolist()
        seen0, logp0 = bits.copy(), np.zeros((17, CAP), dtype=np.float32)
        s1, l1 = device_note(x, st, tok, seen0, logp0)
        s2, l2 = device_note(x, st, tok, seen0, logp0)
        assert np.array_equal(s1, s2) and np.array_equal(i32(l1), i32(l2))
        for r in (0, 8, 16):
            one = device_process(x[r:r + 1], bits[r:r + 1], 1.3, tot[r:r + 1], 3, eos, suppress)
            assert np.array_equal(i32(one[0]), i32(a[r])), (C, r)
            s, l = device_note(x[r:r + 1], st[:, r:r + 1].contiguous(), tok[r:r + 1], seen0[r:r + 1], logp0[r:r + 1])
            assert np.array_equal(s[0], s1[r]) and np.array_equal(i32(l[0]), i32(l1[r])), (C, r)


# ------------------------------------------------------------------ the loop
_PLAIN = {}


def _special():
    return {G.START, G.END, *EOS}


def _diverge_call(**kw):
    _, model = G._diverge_model()
    emb, mask = G._diverge_inputs(G.DIVERGE_SEEDS)
    return model, model.greedy_decode(None, mask, emb, max_new_tokens=G.MAX_NEW, output_image=True, **kw)


def _image_call(B=3, **kw):
    g, model = G._fixture_model("image_prompt")
    return model, model.generate(**G._batch_kw(g, B, max_new_tokens=int(g["max_new_tokens"]), **kw))


CALLS = {"diverge": _diverge_call, "image_prompt": _image_call}


def _plain(name):
    """the fixture's run with every option off: (ids as lists, image rows, an id it emits that is no special one: the most frequent)"""
    if name not in _PLAIN:
        _, (ids, zs) = CALLS[name]()
        ids = [t.tolist() for t in ids]
        count = collections.Counter(i for t in ids for i in t if i not in _special())
        assert count, ids
        _PLAIN[name] = (ids, zs, count.most_common(1)[0][0])
    return _PLAIN[name]


def _record(monkeypatch):
    """wrap ops.logits_process_rows and ops.token_note_rows as the loop calls them: per step the raw and the processed logits, the bitmap
    before and after the note, the state both read, the pick, argmax_rows of the processed rows, and the log-probabilities written"""
    from metamorph_amd import functional as F, ops
    rec = []
    process, note = ops.logits_process_rows, ops.token_note_rows

    def process_wrapped(logits, penalty, seen, total_out, min_new, eos, sup):
        step = dict(raw=logits.cpu().numpy(), args=(penalty, min_new, list(eos), [] if sup is None else sup.cpu().tolist()),
                    seen=None if seen is None else host_bits(seen), total_out=total_out.cpu().tolist())
        process(logits, penalty, seen, total_out, min_new, eos, sup)
        step["processed"] = logits.cpu().numpy()
        rec.append(step)

    def note_wrapped(logits, tok, state, num_image_tokens, token_cap, seen=None, logp_log=None):
        step = rec[-1]
        assert "tok" not in step
        step.update(tok=tok.cpu().tolist(), state=state.cpu().numpy().copy(), noted=logits.cpu().numpy(), N=num_image_tokens, cap=token_cap,
                    argmax=ops.argmax_rows(logits).cpu().tolist())
        note(logits, tok, state, num_image_tokens, token_cap, seen=seen, logp_log=logp_log)
        step.update(seen_after=None if seen is None else host_bits(seen), logp=None if logp_log is None else logp_log.cpu().numpy())
    monkeypatch.setattr(F.ops, "logits_process_rows", process_wrapped)
    monkeypatch.setattr(F.ops, "token_note_rows", note_wrapped)
    return rec


@pytest.mark.parametrize("name", ["diverge", "image_prompt"])
def test_every_step_of_the_eager_loop_is_what_the_host_models_say(monkeypatch, name):
    """G._diverge_model() with its five left-padded prompts, and three copies of the image-prompt fixture: repetition_penalty=1.3,
    min_new_tokens=3, one suppressed id (the most frequent id of the plain run that is neither an image marker nor an eos id) and
    output_logprobs=True, eager, every step recorded.  Non-vacuity: at least one logged pick differs from the argmax of its raw row; the
    fixtures as they stand give 14 (diverge) and 9 (image prompt) such picks on an MI355X, no other seed or penalty was needed."""
    from metamorph_amd import functional as F
    plain_ids, _, sup = _plain(name)
    rec = _record(monkeypatch)
    kw = dict(repetition_penalty=1.3, min_new_tokens=3, suppress_tokens=[sup], output_logprobs=True)
    model, (ids, zs, logps) = S._eager(lambda: CALLS[name](**kw))
    loop = model._greedy_loop
    B = len(ids)
    assert not loop.graphs and len(rec) == loop.steps + 1 and len(zs) == len(logps) == B == loop.cache.batch
    C = rec[0]["raw"].shape[1]
    words = rec[0]["seen"].shape[1]
    bitmap_now = np.zeros((B, words), dtype=np.uint32)
    logged = [[] for _ in range(B)]
    moved, worst = 0, 0.0
    for step in rec:
        penalty, min_new, eos, suppressed = step["args"]
        assert (penalty, min_new, sorted(eos), suppressed) == (1.3, 3, sorted(EOS), [sup])
        assert np.array_equal(step["seen"], bitmap_now) and step["total_out"] == step["state"][2].tolist()
        assert np.array_equal(i32(step["noted"]), i32(step["processed"])) and step["tok"] == step["argmax"]
        for b in range(B):
            want = F.logits_process_host(step["raw"][b], step["seen"][b], 1.3, step["total_out"][b], 3, eos, [sup])
            assert np.array_equal(i32(step["processed"][b]), i32(want)), (b, step["total_out"])
            in_image, n_img, total_out, done, n_tokens, _ = step["state"][:, b].tolist()
            tok = step["tok"][b]
            logs, lp = F.token_note_host(step["processed"][b].astype(np.float64), tok, done, in_image, n_img, n_tokens, step["N"], step["cap"])
            if logs:
                bitmap_now[b, tok >> 5] |= np.uint32(1 << (tok & 31))
                got = step["logp"][b, n_tokens]
                assert abs(float(got) - lp) <= logp_band(lp), (b, total_out, got, lp)
                worst = max(worst, abs(float(got) - lp))
                logged[b].append((tok, got))
                assert tok != sup and not (total_out < 3 and tok in EOS), (b, total_out, tok)
                moved += int(np.argmax(step["raw"][b])) != tok
        assert np.array_equal(step["seen_after"], bitmap_now)
    for b in range(B):
        assert ids[b].tolist() == [t for t, _ in logged[b]] and sup not in ids[b].tolist()
        assert logps[b].dtype == torch.float32 and logps[b].shape == ids[b].shape
        assert np.array_equal(i32(logps[b].cpu().numpy()), i32([v for _, v in logged[b]])), b
    print(f"   [{name}] suppressed id {sup}: {moved} picks moved off the raw argmax, largest |logp - host| {worst:.3e}")
    assert moved >= 1
    assert [t.tolist() for t in ids] != plain_ids
    if name == "image_prompt":
        assert all(z.shape[0] == 4 for z in zs)                  # image rows are still emitted


OPTS = dict(repetition_penalty=1.3, min_new_tokens=3, output_logprobs=True)


def _run(name, graph=True, poll=None, shared=True, **kw):
    from metamorph_amd import functional as F
    model = (G._diverge_model() if name == "diverge" else G._fixture_model("image_prompt"))[1]
    old = F.set_variant("decode_graph", graph)
    if poll is not None:
        model.config.mm355_greedy_poll_steps = poll
    try:
        with route(shared):
            _, (ids, zs, logps) = CALLS[name](**OPTS, suppress_tokens=[_plain(name)[2]], **kw)
    finally:
        F.set_variant("decode_graph", old)
        if poll is not None:
            del model.config.mm355_greedy_poll_steps
    return [t.tolist() for t in ids], zs, [i32(t.cpu().numpy()).tolist() for t in logps], model._greedy_loop


@pytest.mark.parametrize("case", ["batch greedy", "batch sampled", "shared", "fan-out"])
def test_replay_eager_and_polling_are_one_computation_with_the_processors(case):
    """captured replay, eager launches and the poll values 1, 5 and 8 give the same ids, image rows and log-probability bits: the five
    left-padded prompts greedy and sampled (fixed seed), and three continuations of the image prompt on the shared and the fan-out route"""
    name, kw = {"batch greedy": ("diverge", {}), "batch sampled": ("diverge", dict(S.SAMPLE, seed=99)),
                "shared": ("image_prompt", dict(S.SAMPLE, seed=99, B=1, num_return_sequences=3, shared=True)),
                "fan-out": ("image_prompt", dict(S.SAMPLE, seed=99, B=1, num_return_sequences=3, shared=False))}[case]
    ids, zs, logps, loop = _run(name, **kw)
    p = loop.processors
    assert loop.graphs and p is not None and p.penalised and p.want_logprobs and (loop.sampler is None) == (case == "batch greedy")
    assert loop.seen.dtype == torch.int32 and loop.logp_log.shape == loop.tok_log.shape
    if "num_return_sequences" in kw:
        assert loop.cache.batch == 3 and (loop.cache.shared_len > 0) == kw["shared"]
    assert [len(t) for t in ids] == [len(t) for t in logps] and any(len(t) > 3 for t in ids)
    for graph, poll in ((True, 1), (True, 5), (False, 8)):
        i2, z2, l2, loop2 = _run(name, graph=graph, poll=poll, **kw)
        assert i2 == ids and l2 == logps and all(torch.equal(a, b) for a, b in zip(z2, zs)), (case, graph, poll)
        assert bool(loop2.graphs) == graph and loop2.poll == poll


def test_nothing_changes_when_every_option_is_off(monkeypatch):
    from metamorph_amd import functional as F, ops
    calls = []
    for fn in ("logits_process_rows", "token_note_rows"):
        monkeypatch.setattr(F.ops, fn, lambda *a, _fn=fn, **k: calls.append(_fn))
    g, _ = G._fixture_model("image_prompt")
    for kw in ({}, dict(repetition_penalty=1.0, min_new_tokens=0, suppress_tokens=[]),
               dict(repetition_penalty=None, min_new_tokens=None, suppress_tokens=None, output_logprobs=False, repetition_penalty_ids=None)):
        for name in CALLS:
            model, out = CALLS[name](**kw)
            assert len(out) == 2
            loop = model._greedy_loop
            assert loop.processors is None and not isinstance(getattr(loop, "seen", None), torch.Tensor)
            assert not isinstance(getattr(loop, "logp_log", None), torch.Tensor)
            assert [t.tolist() for t in out[0]] == _plain(name)[0] and all(torch.equal(a, b) for a, b in zip(out[1], _plain(name)[1]))
            if name == "image_prompt":                           # the reference-recorded loop, as before
                assert [t.tolist() for t in out[0]] == [g["tokens"].tolist()] * 3
    assert calls == [] and ops.logits_process_rows is not None


PENALTY_IDS = 4.0


def test_repetition_penalty_ids_mark_before_the_first_step(monkeypatch):
    """every id the plain run emits marked for every sequence: the first step reads that bitmap, and where a sequence's raw argmax is
    among the marked ids its first pick is another id"""
    from metamorph_amd import functional as F
    plain_ids, _, _ = _plain("diverge")
    marks = sorted({i for t in plain_ids for i in t})
    rec = _record(monkeypatch)
    model, (ids, _) = S._eager(lambda: _diverge_call(repetition_penalty=PENALTY_IDS, repetition_penalty_ids=marks))
    first = rec[0]
    C = first["raw"].shape[1]
    assert np.array_equal(first["seen"], np.stack([F.seen_bits_host(marks, C)] * len(ids)))
    hit = 0
    for b in range(len(ids)):
        raw = int(np.argmax(first["raw"][b]))
        assert raw == plain_ids[b][0]
        if raw in marks:
            assert first["tok"][b] != raw and ids[b][0].item() == first["tok"][b], (b, raw)
            hit += 1
    assert hit >= 1
    # one list per sequence reaches its own row
    del rec[:]
    per_seq = [[plain_ids[b][0]] for b in range(len(ids))]
    S._eager(lambda: _diverge_call(repetition_penalty=PENALTY_IDS, repetition_penalty_ids=per_seq))
    assert np.array_equal(rec[0]["seen"], np.stack([F.seen_bits_host(m, C) for m in per_seq]))


def test_one_sequence_with_an_option_goes_through_the_device_loop():
    g, model = G._fixture_model("text")
    for kw in (dict(repetition_penalty=1.3), dict(min_new_tokens=2), dict(suppress_tokens=[5]), dict(output_logprobs=True)):
        model._greedy_loop = None
        out = model.generate(**G._batch_kw(g, 1, max_new_tokens=6, **kw))
        loop = model._greedy_loop
        assert loop is not None and loop.processors is not None and loop.cache.batch == 1
        ids = out[0]
        assert isinstance(ids, list) and len(ids) == 1 and ids[0].dtype == torch.int32
        if "output_logprobs" in kw:
            assert len(out) == 3 and isinstance(out[2], list) and len(out[2]) == 1 and out[2][0].shape == ids[0].shape
            assert out[2][0].dtype == torch.float32 and bool((out[2][0] <= 0).all())
            only = model.generate(**{**G._batch_kw(g, 1, max_new_tokens=6, **kw), "output_image": False})
            assert len(only) == 2 and only[0][0].tolist() == ids[0].tolist() and torch.equal(only[1][0], out[2][0])
        else:
            assert len(out) == 2


@pytest.mark.parametrize("case", ["fp8 cache", "w8 weights", "w4 weights"])
def test_the_options_ride_on_quantised_weights_and_the_fp8_cache(case):
    """none of these touches the tail: three copies of the image prompt with every option on -- aligned log-probabilities, no suppressed id,
    no eos id first, and captured replay equal to eager launches bit for bit"""
    import os
    from oracle.ref_model import decode_fixture_state_dict
    g, model = G._fixture_model("image_prompt")
    if case != "fp8 cache":
        cfg = G.tiny_cfg(num_image_tokens=4)
        model = G.hip_model(cfg, decode_fixture_state_dict(np.load(os.path.join(G.GOLDEN, "n1_decode_image_prompt.npz")), cfg, torch.bfloat16)).eval()
        model.quantize_decoder_(**({} if case == "w8 weights" else dict(fmt="mxfp4")))
    sup = _plain("image_prompt")[2]
    kw = G._batch_kw(g, 3, max_new_tokens=int(g["max_new_tokens"]), suppress_tokens=[sup], **OPTS)
    if case == "fp8 cache":
        model.config.mm355_kv_cache_format = "fp8_e4m3"
    try:
        ids, zs, logps = model.generate(**kw)
        loop = model._greedy_loop
        assert loop.graphs and loop.processors is not None and (loop.cache.fmt == "fp8_e4m3") == (case == "fp8 cache")
        i2, z2, l2 = S._eager(lambda: model.generate(**kw))
    finally:
        if case == "fp8 cache":
            model.config.mm355_kv_cache_format = "bf16"
    for b in range(3):
        t = ids[b].tolist()
        assert t and sup not in t and t[0] not in EOS, (b, t)    # (later ids may follow image rows, which count as outputs)
        assert logps[b].shape == ids[b].shape and logps[b].dtype == torch.float32 and bool((logps[b] <= 0).all())
        assert i2[b].tolist() == t and torch.equal(z2[b], zs[b]) and np.array_equal(i32(l2[b].cpu().numpy()), i32(logps[b].cpu().numpy())), b
