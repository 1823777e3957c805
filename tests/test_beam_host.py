"""Beam search in the device token loop, the parts that need no GPU: the host model (functional.beam_step_host / beam_search_host) against
transformers' own GenerationMixin._beam_search bit for bit, the table of own cache rows against a brute-force replay, the refusals of
beam_decode by name, and the C ABI's new symbols and their argument validation by return code."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mm355_attn_decode_shared_idx", "mm355_attn_decode_shared_idx_f8", "mm355_beam_select_rows_ws_bytes", "mm355_beam_select_rows_f32",
       "mm355_beam_advance")


# ------------------------------------------------------------------ the host model against transformers

V, P = 61, 7


@pytest.fixture(scope="module")
def tiny_llama():
    """a random CPU Llama built from a config alone (nothing is downloaded); weights x 4 so that the rows are peaked and hypotheses finish"""
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=V, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                      max_position_embeddings=64, pad_token_id=0)
    model = LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(4.0)
    prompt = torch.randint(1, V, (1, P), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        walk = model.generate(prompt, max_new_tokens=9, do_sample=False, num_beams=1, eos_token_id=None)[0, P:].tolist()
    return model, prompt, walk


def _hf(model, prompt, K, eos, lp, es, new):
    with torch.no_grad():
        out = model.generate(prompt, num_beams=K, num_return_sequences=K, do_sample=False, max_new_tokens=new, eos_token_id=list(eos),
                             length_penalty=lp, early_stopping=es, return_dict_in_generate=True, output_scores=True, pad_token_id=0)
    lens = (out.beam_indices >= 0).sum(1).tolist()
    ids = [out.sequences[i, P:P + lens[i]].tolist() for i in range(K)]
    return ids, out.sequences_scores.numpy(), [s.numpy() for s in out.scores]


def test_host_model_equals_transformers_beam_search_bit_for_bit(tiny_llama):
    from metamorph_amd import functional as F
    model, prompt, walk = tiny_llama
    never = next(i for i in range(1, V) if i not in walk)
    # the first two sets come from the greedy walk so that hypotheses do finish; the third id is only ever reached by a losing beam
    eos_sets = ((walk[2],), (walk[1], walk[4]), (never,))
    cases = list(itertools.product((2, 3, 4), eos_sets, (1.0, 0.0, 2.0, -1.0), (False, True, "never"), (1, 2, 9)))
    assert len(cases) == 324
    early, short = 0, 0
    for K, eos, lp, es, new in cases:
        want_ids, want_scores, rows = _hf(model, prompt, K, eos, lp, es, new)
        ids, scores, flags, steps = F.beam_search_host(lambda t, state: rows[t], K, V, eos, new, lp, es)
        tag = (K, eos, lp, es, new)
        assert steps == len(rows), tag
        assert [i.tolist() for i in ids] == want_ids, tag
        assert scores.tobytes() == want_scores.astype(np.float32).tobytes(), tag
        assert flags.all(), tag
        early += steps < new
        short += len(ids[0]) < new
    # without searches that stop early and best hypotheses that are shorter than the budget the pool and the heuristic are untested
    # (this model and prompt: 17 and 66 of the 324)
    assert early >= 10 and short >= 40, (early, short)


# ------------------------------------------------------------------ the table of own rows

@pytest.mark.parametrize("K,steps,seed", [(2, 5, 0), (3, 17, 1), (8, 40, 2), (4, 1, 3)])
def test_table_update_follows_the_ancestors(K, steps, seed):
    """following own_block from beam b gives exactly the blocks its ancestors appended their rows to"""
    from metamorph_amd import functional as F
    rng = np.random.default_rng(seed)
    Vt, M = 50, 2 * K
    state = F.beam_state_host(K, steps + 1)
    len_pow = F.beam_len_pow(steps + 1, 1.0)
    lineage = [[] for _ in range(K)]                              # per slot: the slot each of its own rows was appended from
    for n in range(steps):
        par = rng.integers(0, K, M)
        val = np.sort(rng.standard_normal(M).astype(np.float32))[::-1] - np.float32(n)
        idx = (par * Vt + rng.permutation(Vt)[:M]).astype(np.int32)
        F.beam_step_host(state, val, idx, Vt, (), steps + 1, len_pow)
        assert state["live"][0] == 1 and state["parent"].tolist() == par[:K].tolist()
        lineage = [lineage[p] + [i] for i, p in enumerate(par[:K])]
        for b in range(K):
            assert state["own_block"][b, :n + 1].tolist() == lineage[b], (n, b)
            # and the back-pointer logs name the same ancestors
            slot, back = b, []
            for u in range(n, -1, -1):
                back.append(slot)
                slot = int(state["parent_log"][u][slot])
            assert back[::-1] == lineage[b]


# ------------------------------------------------------------------ the refusals of beam_decode, and generate()'s routing

def _tiny_cpu_model(**llm_kw):
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
               rms_norm_eps=1e-5, rope_theta=500000.0)
    llm.update(llm_kw)
    geo = dict(hidden_size=64, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14)
    return build_model(llm, geo, num_image_tokens=4, max_length=64)


def test_beam_decode_refuses_by_name_before_any_device_work():
    from metamorph_amd import functional as F
    model = _tiny_cpu_model().eval()
    emb = torch.zeros(1, 5, 64, dtype=torch.bfloat16)

    def call(e=emb, num_beams=3, **kw):
        kw.setdefault("max_new_tokens", 4)
        return model.beam_decode(None, None, e, num_beams, **kw)
    for bad in (1, 0, 9, 2.0, "3", True, None):
        with pytest.raises(ValueError, match=r"num_beams.*integer in \[2, 8\]"):
            call(num_beams=bad)
    with pytest.raises(ValueError, match="one prompt, got 2"):
        call(torch.zeros(2, 5, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="num_return_sequences = 4 exceeds num_beams = 3"):
        call(num_return_sequences=4)
    with pytest.raises(ValueError, match="9 eos ids.*up to 8"):
        call(eos_token_id=tuple(range(9)))
    for bad in (float("inf"), float("nan"), -float("inf"), "x"):
        with pytest.raises(ValueError, match="length_penalty must be a finite number"):
            call(length_penalty=bad)
    for bad in ("always", 1, 0, None, 2):
        with pytest.raises(ValueError, match="early_stopping.*False, True or 'never'"):
            call(early_stopping=bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="max_new_tokens.*integer >= 1"):
            call(max_new_tokens=bad)
    with pytest.raises(NotImplementedError, match="use_cache=False"):
        call(use_cache=False)
    with pytest.raises(NotImplementedError, match="do_sample=True.*beam sampling"):
        call(do_sample=True)
    for kw in (dict(repetition_penalty=1.2), dict(min_new_tokens=2), dict(suppress_tokens=[5]), dict(output_logprobs=True)):
        with pytest.raises(NotImplementedError, match="logits processors are not part of the device beam loop"):
            call(**kw)
    with pytest.raises(NotImplementedError, match="output_image=True.*token-only"):
        call(output_image=True)
    F.set_variant("shared_prefix_attn", False)
    try:
        with pytest.raises(NotImplementedError, match=r"shared_prefix_attn.*no fan-out fallback.*generate\(use_customize_greedy=False, num_beams=K\)"):
            call()
    finally:
        F.set_variant("shared_prefix_attn", True)
    # a GQA group of 16: mm355_attn_decode_shared does not take it
    wide = _tiny_cpu_model(hidden_size=128, num_attention_heads=16, num_key_value_heads=1).eval()
    with pytest.raises(NotImplementedError, match=r"head shape Hq=16 Hkv=1.*no fan-out fallback.*generate\(use_customize_greedy=False, num_beams=K\)"):
        wide.beam_decode(None, None, torch.zeros(1, 5, 128, dtype=torch.bfloat16), 3, max_new_tokens=4)
    # fewer logits than candidates: 8 beams keep 9 * 8 = 72 candidates with 8 eos ids
    small = _tiny_cpu_model(vocab_size=64).eval()
    with pytest.raises(ValueError, match="64 logits are fewer than the 72 candidates"):
        small.beam_decode(None, None, emb, 8, eos_token_id=tuple(range(8)), max_new_tokens=4)


def test_generate_routes_by_the_new_keyword_only(monkeypatch):
    from transformers import GenerationMixin
    model = _tiny_cpu_model().eval()
    seen = []
    monkeypatch.setattr(type(model), "beam_decode", lambda self, **kw: seen.append(("beam", kw)) or "beam")
    monkeypatch.setattr(type(model), "greedy_decode", lambda self, **kw: seen.append(("greedy", kw)) or "greedy")
    monkeypatch.setattr(GenerationMixin, "generate", lambda self, **kw: seen.append(("hf", kw)) or "hf")
    embed = model.get_model().embed_tokens                       # (the embedding gather is a HIP kernel: stand in for it on the CPU)
    monkeypatch.setattr(type(embed), "forward", lambda self, i: torch.zeros(tuple(i.shape) + (64,), dtype=torch.bfloat16))
    ids = torch.tensor([[1, 2, 3]])
    assert model.generate(ids, device_beam_search=True, num_beams=3, max_new_tokens=4, length_penalty=0.5) == "beam"
    kind, kw = seen[-1]
    assert kind == "beam" and kw["num_beams"] == 3 and kw["max_new_tokens"] == 4 and kw["length_penalty"] == 0.5
    assert "device_beam_search" not in kw and tuple(kw["inputs_embeds"].shape) == (1, 3, 64) and kw["output_image"] is False
    # without the keyword: exactly the two routes there were
    assert model.generate(ids, num_beams=3, max_new_tokens=4) == "greedy" and seen[-1][0] == "greedy" and seen[-1][1]["num_beams"] == 3
    assert model.generate(ids, use_customize_greedy=False, num_beams=3, max_new_tokens=4) == "hf"
    kind, kw = seen[-1]
    assert kind == "hf" and kw["num_beams"] == 3 and "device_beam_search" not in kw
    assert model.generate(ids, device_beam_search=False, max_new_tokens=4) == "greedy" and "device_beam_search" not in seen[-1][1]


# ------------------------------------------------------------------ the C ABI

def test_beam_symbols_and_argument_validation_without_a_gpu():
    from metamorph_amd import lib, ops
    names = lib.exported_symbols()
    header = open(os.path.join(REPO, "include", "mm355.h")).read()
    for n in NEW:
        assert n in names and f"{n}(" in header, n
    assert "#define MM355_BEAM_MAX 8" in header and ops.BEAM_MAX == 8
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(lib.LIB_PATH)
    for n in NEW:
        assert hasattr(so, n), n
    assert hasattr(ops, "beam_select_rows") and hasattr(ops, "beam_advance")
    L = lib.load()
    P = 4096                                                     # a non-null, 16-byte aligned stand-in: no kernel is launched on the error path

    # --- the indexed attention: mm355_attn_decode_shared's refusals, and the table's own
    B, Hq, Hkv, d, rows, S = 3, 8, 2, 128, 512, 300
    ld, bs = Hkv * d, rows * Hkv * d
    need = L.mm355_attn_decode_shared_ws_floats(B, Hq, Hkv, d, S, rows)

    def idx(q=P, k=P, lens=P, tbl=P, ldt=8, S_=S, B_=B, Hq_=Hq, d_=d, ws=P, nws=need):
        return L.mm355_attn_decode_shared_idx(q, Hq_ * d, P, P, ld, k, P, ld, bs, lens, tbl, ldt, S_, rows, P, Hq_ * d, B_, Hq_, Hkv, d_, 0.1, ws, nws, 0)

    def idx8(fmt=1, ks=P, tbl=P, ldt=8, B_=B, d_=d, nws=need):
        return L.mm355_attn_decode_shared_idx_f8(P, Hq * d, P, P, ld, P, P, Hkv, P, P, ld, bs, ks, P, Hkv, rows * Hkv, fmt, P, tbl, ldt, S, rows, P,
                                                 Hq * d, B_, Hq, Hkv, d_, 0.1, P, nws, 0)
    for null in ("q", "k", "lens"):
        assert idx(**{null: 0}) == -1, null
    assert idx(ldt=0) == -1 and idx(ldt=-4) == -1                # a table without columns
    big = L.mm355_attn_decode_shared_ws_floats(256, Hq, Hkv, d, S, rows)
    assert idx(B_=256, nws=big) == -1                            # one byte cannot name 256 blocks
    assert idx(S_=-1) == -1 and idx(S_=rows + 1) == -1 and idx(ws=0) == -1 and idx(nws=need - 1) == -1 and idx(q=P + 2) == -1
    assert idx(d_=124) == -2 and idx(Hq_=6) == -2
    assert idx8(fmt=7) == -1 and idx8(ks=0) == -1 and idx8(ldt=0) == -1 and idx8(B_=256, nws=big) == -1 and idx8(nws=need - 1) == -1
    assert idx8(d_=124) == -2

    # --- the selection
    K, V, M = 4, 1000, 8
    wsb = L.mm355_beam_select_rows_ws_bytes(K, V, M)
    assert wsb == K * M * 8 and L.mm355_beam_select_rows_ws_bytes(9, V, 18) == 0 and L.mm355_beam_select_rows_ws_bytes(K, V, 3) == 0

    def sel(x=P, run=P, stats=P, cv=P, ci=P, K_=K, V_=V, M_=M, ws=P, nws=wsb):
        return L.mm355_beam_select_rows_f32(x, K_, V_, run, M_, stats, cv, ci, ws, nws, 0)
    for null in ("x", "run", "stats", "cv", "ci", "ws"):
        assert sel(**{null: 0}) == -1, null
    assert sel(K_=0) == -1 and sel(K_=9, M_=18, nws=1 << 20) == -1                    # K outside [1, MM355_BEAM_MAX]
    assert sel(M_=3) == -1 and sel(M_=37, nws=1 << 20) == -1                          # M outside [K, 9 K]
    assert sel(V_=1, M_=8) == -1 and sel(V_=0) == -1 and sel(V_=2**31 - 1) == -1      # M > K V, V out of argmax_rows_f32's bounds
    assert sel(nws=wsb - 1) == -1 and sel(ws=P + 2) == -1                             # the workspace: short, misaligned

    # --- the bookkeeping
    eos = (ctypes.c_int32 * 8)(*range(8))
    h, cap = 64, 16

    def adv(cv=P, ci=P, run=P, fs=P, ff=P, fe=P, scal=P, live=P, tok=P, par=P, tl=P, pl=P, K_=K, M_=M, V_=V, cap_=cap, tbl=P, ldt=cap, emb=P,
            lde=h, erows=V, xin=P, ldx=h, h_=h, pw=P, new=cap, lp=1.0, es=0, eos_=ctypes.addressof(eos), n_eos=2):
        return L.mm355_beam_advance(cv, ci, K_, M_, V_, run, fs, ff, fe, scal, live, tok, par, tl, pl, cap_, tbl, ldt, emb, lde, erows, xin, ldx,
                                    h_, pw, new, lp, es, eos_, n_eos, 0)
    for null in ("cv", "ci", "run", "fs", "ff", "fe", "scal", "live", "tok", "par", "tl", "pl", "pw"):
        assert adv(**{null: 0}) == -1, null
    assert adv(K_=9) == -1 and adv(M_=3) == -1 and adv(V_=1) == -1
    assert adv(new=0) == -1 and adv(cap_=cap - 1) == -1 and adv(ldt=cap - 1) == -1    # no step, logs or a table shorter than the search
    assert adv(es=3) == -1 and adv(es=-1) == -1 and adv(lp=float("nan")) == -1
    assert adv(n_eos=9) == -1 and adv(n_eos=-1) == -1 and adv(eos_=0) == -1
    assert adv(emb=0) == -1 and adv(xin=0) == -1                                      # the next rows come as a pair
    assert adv(erows=V - 1) == -1 and adv(h_=60) == -1 and adv(lde=h - 8) == -1 and adv(ldx=h + 4) == -1 and adv(xin=P + 8) == -1
