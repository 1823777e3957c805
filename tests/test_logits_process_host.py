"""Logits processors and per-token log-probabilities in the device token loop, the parts that need no GPU: the C ABI's symbols and
validation, functional.logits_process_host (the specification of mm355_logits_process_rows_f32) against transformers' processors bit for
bit, functional.token_note_host against greedy_advance_host and torch.log_softmax, and greedy_decode's refusals of bad arguments."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mm355_logits_process_rows_f32", "mm355_token_note_rows_f32")


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.int32), np.asarray(b, dtype=np.float32).view(np.int32))


def test_logits_symbols_and_validation_without_a_gpu():
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
    L = lib.load()
    P = 4096                                                     # a non-null stand-in: no kernel is launched on the error path
    eos = (ctypes.c_int32 * 16)(*range(16))
    E = ctypes.addressof(eos)
    assert ops.seen_words(1) == 1 and ops.seen_words(32) == 1 and ops.seen_words(33) == 2 and ops.seen_words(128256) == 4008

    def process(x=P, R=2, C=64, penalty=1.3, seen=P, words=2, total_out=P, min_new=2, eos_ids=E, n_eos=2, sup=P, n_sup=3):
        return L.mm355_logits_process_rows_f32(x, R, C, penalty, seen, words, total_out, min_new, eos_ids, n_eos, sup, n_sup, 0)
    assert process(x=0) == -1
    assert process(R=0) == -1 and process(C=0) == -1 and process(R=65536) == -1 and process(C=2**31 - 1) == -1
    for bad in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert process(penalty=bad) == -1, bad
    assert process(seen=0) == -1                                 # penalty != 1 with a null bitmap
    assert process(words=1) == -1 and process(C=65, words=2) == -1
    assert process(total_out=0) == -1                            # min_new_tokens > 0 with a null state row
    assert process(n_eos=ops.GREEDY_MAX_EOS + 1) == -1 and process(n_eos=-1) == -1 and process(eos_ids=0) == -1
    assert process(sup=0) == -1 and process(n_sup=-1) == -1
    # nothing to edit: fine, and nothing is launched (the pointers are stand-ins)
    assert process(penalty=1.0, seen=0, words=0, total_out=0, min_new=0, eos_ids=0, n_eos=0, sup=0, n_sup=0) == 0

    def note(x=P, R=2, C=64, tok=P, in_image=P, n_img=P, done=P, n_tokens=P, N=4, cap=8, seen=P, words=2, logp=P):
        return L.mm355_token_note_rows_f32(x, R, C, tok, in_image, n_img, done, n_tokens, N, cap, seen, words, logp, 0)
    for null in ("x", "tok", "in_image", "n_img", "done", "n_tokens"):
        assert note(**{null: 0}) == -1, null
    assert note(R=0) == -1 and note(C=0) == -1 and note(R=65536) == -1 and note(C=2**31 - 1) == -1
    assert note(cap=-1) == -1 and note(cap=2**31) == -1
    assert note(seen=0, logp=0) == -1 and note(words=1) == -1 and note(C=65) == -1


# ------------------------------------------------------------------ logits_process_host against transformers
def _hf(row, history, penalty, n_new, min_new, eos, suppress):
    """RepetitionPenalty -> MinNewTokensLength -> SuppressTokens of transformers on one fp32 row; history: the generated ids"""
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                                                        SuppressTokensLogitsProcessor)
    prompt = 3
    ids = torch.tensor([[0] * prompt + list(history)[:n_new] + [0] * max(n_new - len(history), 0)], dtype=torch.long)
    s = torch.from_numpy(np.array(row, dtype=np.float32))[None].clone()
    if penalty != 1.0:
        s = RepetitionPenaltyLogitsProcessor(penalty)(torch.tensor([list(history)], dtype=torch.long), s)
    if min_new > 0:
        s = MinNewTokensLengthLogitsProcessor(prompt, min_new, eos, device="cpu")(ids, s)
    if suppress:
        s = SuppressTokensLogitsProcessor(suppress, device="cpu")(ids, s)
    assert s.dtype == torch.float32
    return s[0].numpy()


@pytest.mark.parametrize("C", [37, 1000])
def test_logits_process_host_equals_the_hf_processors_bit_for_bit(C):
    from metamorph_amd import functional as F
    rng = np.random.default_rng(C)
    eos = [C - 2, 5]
    cases = 0
    for penalty in (0.7, 1.0, 1.3, 2.0):
        for min_new, n_new in ((0, 4), (3, 2), (3, 3), (3, 4), (1, 0)):
            row = (rng.standard_normal(C) * 4.0).astype(np.float32)
            history = rng.integers(0, C, size=max(n_new, 1) + 5).tolist()
            history += [history[0], history[0], 5]                # repeated ids, and an eos id that is also a marked id
            suppress = [int(rng.integers(0, C)), history[1]] if (cases % 2) else []
            want = _hf(row, history, penalty, n_new, min_new, eos, suppress)
            got = F.logits_process_host(row, F.seen_bits_host(history, C), penalty, n_new, min_new, eos, suppress)
            assert got.dtype == np.float32 and bits_equal(got, want), (penalty, min_new, n_new)
            if penalty != 1.0:
                assert not bits_equal(got, row)
            if min_new > n_new:
                assert got[5] == -np.inf and got[C - 2] == -np.inf
            elif penalty != 1.0 and 5 not in suppress:
                assert np.isfinite(got[5]) and got[5] != row[5]
            cases += 1
    assert cases == 20


def test_logits_process_host_edges():
    from metamorph_amd import functional as F
    C = 37
    row = np.linspace(-3, 3, C).astype(np.float32)
    row[0], row[1], row[2], row[3], row[4] = -0.0, np.inf, -np.inf, np.nan, 0.0
    full = np.full(3, 0xFFFFFFFF, dtype=np.uint32)              # every id marked, the last word's bits beyond C set, and a spare word
    got = F.logits_process_host(row, full, 2.0, 0, 0, [], None)
    assert np.signbit(got[0]) and got[0] == 0 and got[1] == np.inf and got[2] == -np.inf and np.isnan(got[3]) and not np.signbit(got[4])
    assert bits_equal(got[5:], np.where(row[5:] < 0, row[5:] * np.float32(2), row[5:] / np.float32(2)))
    want = _hf(row, list(range(C)), 2.0, 0, 0, [], [])
    assert bits_equal(got, want)
    # only bits beyond C set: nothing is marked
    beyond = np.array([0, 0xFFFFFFE0, 0xFFFFFFFF], dtype=np.uint32)
    assert bits_equal(F.logits_process_host(row, beyond, 2.0, 0, 0, [], None), row)
    # penalty 1 and a null bitmap skip the step
    assert bits_equal(F.logits_process_host(row, full, 1.0, 0, 0, [], None), row)
    assert bits_equal(F.logits_process_host(row, None, 2.0, 0, 0, [], None), row)
    # ids outside [0, C) in either list are skipped
    got = F.logits_process_host(row, None, 1.0, 0, 2, [-1, C, 7, 2**31 - 1], [C + 5, -200, 9, -2**31])
    want = row.copy()
    want[[7, 9]] = -np.inf
    assert bits_equal(got, want)
    got = F.logits_process_host(row, None, 1.0, 2, 2, [7], [9])    # total_out has reached min_new_tokens: the eos id stays
    want = row.copy()
    want[9] = -np.inf
    assert bits_equal(got, want)
    with pytest.raises(ValueError):
        F.seen_bits_host([C], C)


# ------------------------------------------------------------------ token_note_host
def test_token_note_host_logs_when_greedy_advance_host_logs_a_token():
    from metamorph_amd import functional as F
    N, cap, C = 4, 3, 16
    row = np.arange(C, dtype=np.float64)
    n = 0
    for done, in_image, n_img, n_tokens, tok in itertools.product((0, 1), (0, 1), (N - 1, N), (cap - 1, cap), (3, 60, 61, 62)):
        st = dict(in_image=in_image, n_img=n_img, total_out=5, done=done, n_tokens=n_tokens, n_z=1)
        t = tok if tok < C else 3
        logs, _ = F.token_note_host(row, t, done, in_image, n_img, n_tokens, N, cap)
        log, _ = F.greedy_advance_host(dict(st), tok, 60, 61, N, 100, {62}, token_cap=cap, z_cap=8)
        assert logs == (log == "tok"), (done, in_image, n_img, n_tokens, tok)
        n += logs
    assert 0 < n < 64
    # an id that is no column logs nothing (mm355_greedy_advance refuses it as well)
    assert F.token_note_host(row, C, 0, 0, 0, 0, N, cap)[0] is False and F.token_note_host(row, -1, 0, 0, 0, 0, N, cap)[0] is False
    assert F.token_note_host(row, 3, 0, 0, 0, 0, N, cap)[0] is True


@pytest.mark.parametrize("C", [37, 1000])
def test_token_note_host_is_log_softmax_in_fp64(C):
    from metamorph_amd import functional as F
    rng = np.random.default_rng(C + 1)
    for scale in (1.0, 4.0, 350.0):
        x = rng.standard_normal(C) * scale
        x[rng.integers(0, C, size=C // 5)] = -np.inf
        x[7] = 0.5
        want = torch.log_softmax(torch.from_numpy(x), dim=-1).numpy()
        for tok in (0, 7, C - 1, int(np.argmax(x))):
            _, lp = F.token_note_host(x, tok, 0, 0, 0, 0, 4, 8)
            if want[tok] == -np.inf:
                assert lp == -np.inf
            else:
                assert abs(lp - want[tok]) <= 1e-12 * max(1.0, abs(want[tok])), (scale, tok, lp, want[tok])
    x = rng.standard_normal(C)
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[3] = bad
        assert np.isnan(F.token_note_host(y, 5, 0, 0, 0, 0, 4, 8)[1])
    assert np.isnan(F.token_note_host(np.full(C, -np.inf), 5, 0, 0, 0, 0, 4, 8)[1])
    y = x.copy()
    y[5] = -np.inf
    assert F.token_note_host(y, 5, 0, 0, 0, 0, 4, 8)[1] == -np.inf


# ------------------------------------------------------------------ refusals
def _tiny_cpu_model():
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
               rms_norm_eps=1e-5, rope_theta=500000.0)
    geo = dict(hidden_size=64, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14)
    return build_model(llm, geo, num_image_tokens=4, max_length=64)


def test_greedy_decode_refuses_bad_processor_arguments_by_name():
    model = _tiny_cpu_model().eval()
    emb = torch.zeros(2, 5, 64, dtype=torch.bfloat16)

    def call(e=emb, **kw):
        return model.greedy_decode(None, None, e, max_new_tokens=4, **kw)
    for bad in (0.0, -1.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="repetition_penalty"):
            call(repetition_penalty=bad)
    for bad in (-1, 2.5, 5, "3", True):
        with pytest.raises(ValueError, match="min_new_tokens"):
            call(min_new_tokens=bad)
    for bad in ([320], [-200], [3, -1]):
        with pytest.raises(ValueError, match="suppress_tokens"):
            call(suppress_tokens=bad)
        with pytest.raises(ValueError, match="repetition_penalty_ids"):
            call(repetition_penalty=1.3, repetition_penalty_ids=bad)
    with pytest.raises(ValueError, match="repetition_penalty_ids"):
        call(repetition_penalty_ids=[3])                           # no active penalty
    with pytest.raises(ValueError, match="repetition_penalty_ids"):
        call(repetition_penalty=1.0, repetition_penalty_ids=[3])
    with pytest.raises(ValueError, match="repetition_penalty_ids"):
        call(repetition_penalty=1.3, repetition_penalty_ids=[[3], [4], [5]])      # three lists for two sequences
    with pytest.raises(ValueError, match="repetition_penalty_ids"):
        call(e=emb[:1], repetition_penalty=1.3, repetition_penalty_ids=[[3], [4]], do_sample=True, temperature=0.7, num_return_sequences=2)
    for kw in (dict(repetition_penalty=1.3), dict(min_new_tokens=2), dict(suppress_tokens=[7]), dict(output_logprobs=True)):
        with pytest.raises(NotImplementedError, match="use_cache=False"):
            call(use_cache=False, **kw)
        with pytest.raises(NotImplementedError, match="use_cache=False"):
            call(e=emb[:1], use_cache=False, **kw)
    # what is off is None: the loop is then built as before
    P = type(model)._processors_of
    assert P(None, None, None, False, None, 4, 320, 2) is None and P(1.0, 0, [], False, None, 4, 320, 2) is None
    assert P(1.3, 4, [9, 7, 9], True, [5, 6], 4, 320, 2) == dict(repetition_penalty=1.3, min_new_tokens=4, suppress=[7, 9], want_logprobs=True,
                                                               marks=[[5, 6], [5, 6]])
    assert P(2, None, None, False, [[1], [2]], 4, 320, 2)["marks"] == [[1], [2]]
    assert P(None, 2.0, None, False, None, 4, 320, 1)["min_new_tokens"] == 2
