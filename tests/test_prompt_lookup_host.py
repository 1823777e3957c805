"""Prompt-lookup speculative decoding in the device token loop, the parts that need no GPU: functional.prompt_lookup_host (the
specification of mm355_ngram_draft_rows) against transformers' PromptLookupCandidateGenerator and on hand cases,
functional.spec_advance_host (the specification of mm355_spec_verify_advance) against greedy_advance_host and a scripted stream, the
C ABI's symbols and validation, and greedy_decode's refusals by name."""
import ctypes
import itertools
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mm355_ngram_draft_rows", "mm355_spec_verify_advance")
START, END, EOS = 60, 61, 62


def lookup_histories():
    """(history, alphabet size) over 3 - 5 valid ids, so that matches are frequent: lengths 0, 1, 2, N + 1 for N in {1, 2, 4}, 50 and 5000
    (shared with tests/test_prompt_lookup_gpu.py)"""
    out = []
    for i, L in enumerate((0, 1, 2, 3, 5, 50, 50, 5000, 5000)):
        A = 3 + i % 3
        g = torch.Generator().manual_seed(100 + i)
        out.append((torch.randint(0, A, (L,), generator=g).tolist(), A))
    return out


def test_prompt_lookup_host_equals_transformers_candidate_generator():
    try:
        from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    except ImportError:
        pytest.skip("transformers has no PromptLookupCandidateGenerator")
    from metamorph_amd import functional as F
    hits = 0
    for (hist, A), K, N in itertools.product(lookup_histories(), (1, 4, 15), (1, 2, 4)):
        gen = PromptLookupCandidateGenerator(eos_token_id=None, num_output_tokens=K, max_matching_ngram_size=N, max_length=10**9)
        ids = torch.tensor([hist], dtype=torch.long)
        cand, _ = gen.get_candidates(ids)
        want = cand[0, len(hist):].tolist()
        got = F.prompt_lookup_host(hist, K, N, A)
        assert got == want, (len(hist), K, N, got, want)
        hits += bool(want)
    assert hits >= 36                                            # not a comparison of empty lists: 50 ids over <= 5 values repeat one


def test_prompt_lookup_host_hand_cases():
    from metamorph_amd import functional as F
    P = F.prompt_lookup_host
    C = 100
    assert P([5, 6, 7, 8, 9, 5, 6], 3, 2, C) == [7, 8, 9]                      # a match at index 0
    assert P([1, 2, 3, 4], 3, 2, C) == [] and P([4, 4], 3, 2, C) == [4]        # only the trailing occurrence; ... and one in front of it
    assert P([3], 3, 2, C) == [] and P([], 3, 2, C) == []
    assert P([1, 2, 9, 1, 2], 5, 2, C) == [9, 1, 2]                            # a continuation cut by the end
    assert P([1, 2, 10, 7, 1, 2, 11, 7, 1, 2], 2, 2, C) == [10, 7]             # several matches: the earliest wins
    assert P([2, 20, 1, 2, 30, 1, 2], 1, 2, C) == [30]                         # the longer n-gram beats an earlier shorter one
    assert P([2, 20, 1, 2, 30, 1, 2], 1, 1, C) == [20]
    assert P([1, 2, 7, -200, 8, 1, 2], 4, 2, C) == [7]                         # a continuation cropped at -200 ...
    assert P([1, 2, 7, 100, 8, 1, 2], 4, 2, C) == [7]                          # ... and at an id >= C
    assert P([1, 2, -200, 5, 1, 2, 6, 1, 2], 3, 2, C) == [6, 1, 2]             # a match whose cropped continuation is empty is skipped
    assert P([1, 2, -200, 5, 2, 8, 1, 2], 3, 2, C) == [8, 1, 2]                # ... down to a shorter n-gram where no other is left
    assert P([-200, 4, -200], 2, 1, C) == [4]                                  # ids outside [0, C) compare as plain integers in a pattern


def _adv(state, tok, **kw):
    from metamorph_amd import functional as F
    return F.greedy_advance_host(state, tok, START, END, 4, kw.pop("max_new", 30), {EOS}, **kw)


def _spec(state, toks, drafts, **kw):
    from metamorph_amd import functional as F
    return F.spec_advance_host(state, toks, drafts, START, END, 4, kw.pop("max_new", 30), {EOS}, **kw)


def test_spec_advance_host_without_drafts_is_greedy_advance_host():
    from metamorph_amd import functional as F
    g = torch.Generator().manual_seed(3)
    stream = torch.tensor([START, END, EOS, 3, 4, 5])[torch.multinomial(torch.tensor([0.25, 0.17, 0.04, 0.18, 0.18, 0.18]), 60, True,
                                                                     generator=g)].tolist()
    for caps in (dict(), dict(token_cap=3, z_cap=2)):
        a, b = dict.fromkeys(F.GREEDY_STATE, 0), dict.fromkeys(F.GREEDY_STATE, 0)
        for t, tok in enumerate(stream):
            was_done = a["done"]
            want = _adv(a, tok, max_new=40, **caps)
            got = _spec(b, [tok, 99, 98], [], max_new=40, **caps)
            assert got == ([] if was_done else [want]) and a == b, (t, got, want)
        assert a["done"]


def test_spec_advance_host_stops_where_the_rules_say():
    """start -> 4 image rows -> end -> text -> eos, the drafts matching across every boundary"""
    from metamorph_amd import functional as F
    s = dict.fromkeys(F.GREEDY_STATE, 0)
    ref = dict.fromkeys(F.GREEDY_STATE, 0)
    # text, then <start>: the walk ends on entering image mode although the next draft matches
    out = _spec(s, [7, 8, START, 9], [7, 8, START])
    assert out == [("tok", "embed")] * 3 and s["in_image"] == 1 and s["n_tokens"] == 3
    for t in (7, 8, START):
        _adv(ref, t)
    assert s == ref
    # image rows: one iteration per step whatever the ids and drafts say (the drafter gives none here; a stale list changes nothing)
    for k in range(4):
        out = _spec(s, [5, 5, 5, 5], [5, 5, 5])
        assert out == [("z", "fed")] and s["n_z"] == k + 1
    assert s["in_image"] == 0 and s["n_img"] == 4
    # <end>, text: accepted through the boundary; the last row has no draft behind it
    out = _spec(s, [END, 41, 42, 43], [END, 41, 42])
    assert out == [("tok", "embed")] * 4 and s["n_img"] == 0 and s["n_tokens"] == 7
    # a miss: the iteration that emits the differing id is the last one
    out = _spec(s, [41, 44, 42, 43], [41, 42, 43])
    assert len(out) == 2 and s["n_tokens"] == 9
    # fewer drafts than rows: i == len(drafts) ends the walk
    assert len(_spec(s, [41, 42, 43, 44], [41])) == 2
    # eos: done, later rows are not run although their drafts match; afterwards nothing runs
    out = _spec(s, [41, EOS, 42, 43], [41, EOS, 42])
    assert len(out) == 2 and s["done"] == 1 and s["n_tokens"] == 13 and s["total_out"] == 17
    assert _spec(s, [41, 42, 43, 44], [41, 42, 43]) == [] and s["total_out"] == 17
    # total_out > max_new_tokens ends it the same way
    s = dict.fromkeys(F.GREEDY_STATE, 0)
    assert len(_spec(s, [1, 2, 3, 4], [1, 2, 3], max_new=1)) == 2 and s["done"] == 1 and s["total_out"] == 2


def test_spec_advance_host_caps():
    from metamorph_amd import functional as F
    s = dict.fromkeys(F.GREEDY_STATE, 0)
    out = _spec(s, [1, 2, 3, 4], [1, 2, 3], token_cap=3, z_cap=2)
    assert out == [("tok", "embed")] * 3 + [(None, None)] and s["done"] == 1 and s["n_tokens"] == 3 and s["total_out"] == 3
    s = dict.fromkeys(F.GREEDY_STATE, 0)
    assert _spec(s, [START, 0], [START], token_cap=3, z_cap=2) == [("tok", "embed")]
    assert _spec(s, [0, 0], [], token_cap=3, z_cap=2) == [("z", "fed")] and _spec(s, [0, 0], [], token_cap=3, z_cap=2) == [("z", "fed")]
    assert _spec(s, [0, 0], [], token_cap=3, z_cap=2) == [(None, None)] and s["done"] == 1 and s["n_z"] == 2


def test_spec_symbols_and_validation_without_a_gpu():
    from metamorph_amd import functional as F, lib, ops
    from metamorph_amd.model.language_model import metamorph_llama as M
    names = lib.exported_symbols()
    header = open(os.path.join(REPO, "include", "mm355.h")).read()
    for n in NEW:
        assert n in names and f"{n}(" in header, n
    assert "#define MM355_SPEC_MAX_DRAFT 15" in header and "#define MM355_SPEC_MAX_NGRAM 8" in header
    assert M.MM355_SPEC_MAX_DRAFT == F.SPEC_MAX_DRAFT == ops.SPEC_MAX_DRAFT == 15 and F.SPEC_MAX_NGRAM == ops.SPEC_MAX_NGRAM == 8
    assert ops.attn_extend_supported(32, 8, 128) and ops.attn_extend_supported(2, 1, 24) and not ops.attn_extend_supported(6, 2, 128)
    assert not ops.attn_extend_supported(2, 1, 256) and not ops.attn_extend_supported(2, 1, 60)
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = lib.load()
    P = 4096                                                     # a non-null, 16-byte aligned stand-in: no kernel is launched on the error path

    def draft(hist=P, hist_cap=64, B=2, K=3, N=2, C=100, embed=P, ld=64, rows=128, x_in=P, h=64, mask=P):
        return L.mm355_ngram_draft_rows(hist, hist_cap, P, P, P, P, B, K, N, C, embed, ld, rows, P, P, x_in, ld, h, P, mask, 0)
    for bad in (dict(hist=0), dict(mask=0), dict(embed=0), dict(x_in=0), dict(B=0), dict(K=0), dict(K=16), dict(N=0), dict(N=9), dict(C=0),
                dict(C=129), dict(hist_cap=0), dict(h=60), dict(ld=56), dict(embed=P + 8)):
        assert draft(**bad) == -1, bad

    def verify(tok=P, B=2, K=3, C=100, rows=128, fed=P, ld=64, h=64, Dz=32, pos=P, acc=P, count=1, n_eos=1, eos=P, hist_cap=64, z_log=P):
        return L.mm355_spec_verify_advance(tok, P, P, B, K, C, P, P, P, P, P, P, P, P, ld, rows, fed, ld, P, Dz, P, ld, h, Dz, P, 8, z_log, 8, P,
                                           hist_cap, P, pos, P, acc, 8, P, count, 60, 61, 4, 30, eos, n_eos, 0)
    for bad in (dict(tok=0), dict(fed=0), dict(B=0), dict(K=0), dict(K=16), dict(C=129), dict(h=60), dict(Dz=36), dict(pos=0), dict(acc=0),
                dict(n_eos=9), dict(n_eos=1, eos=0), dict(hist_cap=0), dict(z_log=P + 4), dict(ld=56)):
        assert verify(**bad) == -1, bad


def _tiny_cpu_model(**llm_kw):
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
               rms_norm_eps=1e-5, rope_theta=500000.0)
    llm.update(llm_kw)
    geo = dict(hidden_size=64, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14)
    return build_model(llm, geo, num_image_tokens=4, max_length=64)


def test_greedy_decode_refuses_bad_prompt_lookup_arguments_by_name():
    model = _tiny_cpu_model().eval()
    emb = torch.zeros(2, 5, 64, dtype=torch.bfloat16)

    def call(e=emb, **kw):
        return model.greedy_decode(None, None, e, max_new_tokens=4, **kw)
    for bad in (-1, 16, 2.0, "3", True):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            call(prompt_lookup_num_tokens=bad)
    for bad in (0, -2, 9, 1.5, "2", False):
        with pytest.raises(ValueError, match="max_matching_ngram_size"):
            call(prompt_lookup_num_tokens=3, max_matching_ngram_size=bad)
    for bad in ([[1], [2], [3]], [[1]], [1.5, 2], torch.zeros(3, 4, dtype=torch.long), torch.zeros(2, 4), [2**31]):
        with pytest.raises(ValueError, match="prompt_lookup_ids"):
            call(prompt_lookup_num_tokens=3, prompt_lookup_ids=bad)
    with pytest.raises(ValueError, match="prompt_lookup_ids"):      # a tensor is read with the attention mask
        model.greedy_decode(None, torch.ones(2, 5, dtype=torch.long), emb, max_new_tokens=4, prompt_lookup_num_tokens=3,
                            prompt_lookup_ids=torch.zeros(2, 4, dtype=torch.long))
    for kw, why in ((dict(do_sample=True, temperature=0.7), "sampler"), (dict(num_return_sequences=2), "num_return_sequences"),
                    (dict(repetition_penalty=1.3), "repetition_penalty"), (dict(min_new_tokens=2), "min_new_tokens"),
                    (dict(suppress_tokens=[7]), "suppress_tokens"), (dict(output_logprobs=True), "output_logprobs"),
                    (dict(shared_prefix_rows=2), "shared_prefix_rows"), (dict(shared_prefix_rows="auto"), "shared_prefix_rows"),
                    (dict(use_cache=False), "use_cache=False"), (dict(num_beams=4), "num_beams")):
        with pytest.raises(ValueError, match=why) as err:
            call(prompt_lookup_num_tokens=3, prompt_lookup_ids=[1, 2, 3], **kw)
        assert "prompt_lookup_num_tokens=3" in str(err.value)
    with pytest.raises(ValueError, match="device_beam_search"):
        model.generate(inputs=torch.zeros(1, 5, dtype=torch.long), prompt_lookup_num_tokens=3, device_beam_search=True, num_beams=2)
    # a head shape the row kernels do not take: d = 24 is no multiple of 16
    odd = _tiny_cpu_model(hidden_size=48).eval()
    with pytest.raises(ValueError, match="no kernel for Hq=2 Hkv=1 d=24"):
        odd.greedy_decode(None, None, torch.zeros(1, 5, 48, dtype=torch.bfloat16), max_new_tokens=4, prompt_lookup_num_tokens=3)
    # what is off is None, and the ids come out as one list per sequence
    A, I = type(model)._prompt_lookup_arg, type(model)._prompt_lookup_ids
    assert A(None, None) is None and A(0, 5) is None and A(None, 3) is None and A(3, None) == (3, 2) and A(15, 8) == (15, 8)
    assert I(None, None, 2) == [[], []] and I([], None, 2) == [[], []] and I([4, -200, 5], None, 2) == [[4, -200, 5]] * 2
    assert I([[1], [2, 3]], None, 2) == [[1], [2, 3]] and I(([1], (2, 3)), None, 2) == [[1], [2, 3]]
    ids, mask = torch.tensor([[0, 0, 7, 8], [1, -200, 3, 4]]), torch.tensor([[0, 0, 1, 1], [1, 1, 1, 1]])
    assert I(ids, mask, 2) == [[7, 8], [1, -200, 3, 4]] and I(ids, None, 2) == ids.tolist()
