"""Batched greedy text-and-image decoding, the parts that need no GPU: functional.greedy_advance_host (the specification of
mm355_greedy_advance) walked over the reference-recorded argmax streams of tests/golden/n1_decode_*.npz and over hand-written branches,
the C ABI's symbols and validation, and greedy_decode's refusals of a batch."""
import ctypes
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
START, END, EOS = 128256, 128257, (128001, 128009)


def _walk(stream, N, max_new, start=START, end=END, eos=EOS, **caps):
    """the loop of `_greedy_decode_cached` with its branch replaced by greedy_advance_host: (ids, pred_z rows, iterations, state)"""
    from metamorph_amd import functional as F
    st = dict.fromkeys(F.GREEDY_STATE, 0)
    ids, n_z, it = [], 0, 0
    for tok in stream:
        if st["done"]:
            break
        log, nxt = F.greedy_advance_host(st, int(tok), start, end, N, max_new, set(eos), **caps)
        it += 1
        if log == "tok":
            ids.append(int(tok))
            assert nxt == "embed"
        elif log == "z":
            n_z += 1
            assert nxt == "fed"
        assert len(ids) == st["n_tokens"] and n_z == st["n_z"]
    return ids, n_z, it, st


@pytest.mark.parametrize("name", ["text", "image_prompt", "image_prompt_rope31"])
def test_host_model_walks_the_reference_recorded_streams(name):
    g = np.load(os.path.join(GOLDEN, f"n1_decode_{name}.npz"))
    stream = g["step_argmax"].tolist()
    ids, n_z, it, st = _walk(stream, 4, int(g["max_new_tokens"]))
    assert ids == g["tokens"].tolist() and n_z == 4 and it == 9 and st["done"] == 1
    for mn in (2, 6):
        ids, n_z, it, st = _walk(stream, 4, mn)
        assert ids == g[f"tokens_max{mn}"].tolist() and n_z == int(g[f"n_pred_z_max{mn}"]) and it == int(g[f"iterations_max{mn}"])
        assert st["done"] == 1 and st["total_out"] == mn + 1


def test_host_model_unrecorded_branches():
    from metamorph_amd import functional as F
    # an eos id arriving inside image mode: the iteration still logs its pred_z row (the image branch comes first), then the loop ends
    ids, n_z, it, st = _walk([100, 5, 9, 5, 5], 4, 12, start=100, end=101, eos=(9,))
    assert (ids, n_z, it) == ([100], 2, 3)
    assert st == dict(in_image=1, n_img=2, total_out=3, done=1, n_tokens=1, n_z=2)
    # a second <image_start> before <image_end>: n_img stays at N, so the image branch is closed and ids are logged while in_image is 1
    stream = [100, 7, 7, 7, 7, 100, 8, 101, 3]
    ids, n_z, it, st = _walk(stream[:7], 4, 12, start=100, end=101, eos=(9,))
    assert (ids, n_z, it) == ([100, 100, 8], 4, 7)
    assert st == dict(in_image=1, n_img=4, total_out=7, done=0, n_tokens=3, n_z=4)
    ids, n_z, it, st = _walk(stream, 4, 12, start=100, end=101, eos=(9,))
    assert (ids, n_z, it) == ([100, 100, 8, 101, 3], 4, 9)
    assert st == dict(in_image=0, n_img=0, total_out=9, done=0, n_tokens=5, n_z=4)
    # a full token log sets done and writes nothing
    ids, n_z, it, st = _walk([5, 6, 7, 8], 4, 12, start=100, end=101, eos=(9,), token_cap=2, z_cap=8)
    assert (ids, n_z, it) == ([5, 6], 0, 3)
    assert st == dict(in_image=0, n_img=0, total_out=2, done=1, n_tokens=2, n_z=0)
    # ... and so does a full z log
    ids, n_z, it, st = _walk([100, 7, 7, 7], 4, 12, start=100, end=101, eos=(9,), token_cap=8, z_cap=1)
    assert (ids, n_z, it) == ([100], 1, 3)
    assert st == dict(in_image=1, n_img=1, total_out=2, done=1, n_tokens=1, n_z=1)
    # a finished sequence: nothing changes
    keep = dict(st)
    assert F.greedy_advance_host(st, 5, 100, 101, 4, 12, {9}) == (None, None) and st == keep


def _host_loop(stream, N, max_new, start=START, end=END, eos=EOS):
    """functional.greedy_host_loop -- the loop greedy_decode runs for one sequence -- with a head that reads the argmax stream:
    (ids, pred_z rows, head calls).  Call i hands out the rows ("fed", i) and ("z", i); what is logged and fed back is checked here."""
    from metamorph_amd import functional as F
    todo, modes, fed = iter(stream), [], []

    def head(in_image):
        modes.append(in_image)
        return next(todo), ("fed", len(modes) - 1), ("z", len(modes) - 1)
    ids, z_rows = F.greedy_host_loop(head, lambda tok, row: fed.append((tok, row)), start, end, N, max_new, eos)
    assert len(fed) == len(modes) - 1                            # every iteration but the last one feeds the next
    assert all(modes[i] for _, i in z_rows)                      # an image row comes from a head call in image mode
    for i, (tok, row) in enumerate(fed):
        assert tok == stream[i] and row == (("fed", i) if ("z", i) in z_rows else None)
    return ids, len(z_rows), len(modes)


@pytest.mark.parametrize("name", ["text", "image_prompt", "image_prompt_rope31"])
def test_host_loop_walks_the_reference_recorded_streams(name):
    g = np.load(os.path.join(GOLDEN, f"n1_decode_{name}.npz"))
    stream = g["step_argmax"].tolist()
    for mn in (int(g["max_new_tokens"]), 2, 6):
        assert _host_loop(stream, 4, mn) == _walk(stream, 4, mn)[:3]
    assert _host_loop(stream, 4, int(g["max_new_tokens"])) == (g["tokens"].tolist(), 4, 9)
    for mn in (2, 6):
        assert _host_loop(stream, 4, mn) == (g[f"tokens_max{mn}"].tolist(), int(g[f"n_pred_z_max{mn}"]), int(g[f"iterations_max{mn}"]))


def test_host_loop_unrecorded_branches():
    # (the streams of test_host_model_unrecorded_branches that run without log caps; where _walk stops because its stream ends, the
    # budget ends the loop at the same iteration)
    assert _host_loop([100, 5, 9, 5, 5], 4, 12, start=100, end=101, eos=(9,)) == ([100], 2, 3)
    stream = [100, 7, 7, 7, 7, 100, 8, 101, 3]
    assert _walk(stream[:7], 4, 12, start=100, end=101, eos=(9,))[:3] == ([100, 100, 8], 4, 7)
    assert _host_loop(stream[:7], 4, 6, start=100, end=101, eos=(9,)) == ([100, 100, 8], 4, 7)
    assert _walk(stream, 4, 12, start=100, end=101, eos=(9,))[:3] == ([100, 100, 8, 101, 3], 4, 9)
    assert _host_loop(stream, 4, 8, start=100, end=101, eos=(9,)) == ([100, 100, 8, 101, 3], 4, 9)


def test_greedy_symbols_and_validation_without_a_gpu():
    from metamorph_amd import lib
    names = lib.exported_symbols()
    new = ("mm355_argmax_rows_ws_bytes", "mm355_argmax_rows_f32", "mm355_rows_select_bf16", "mm355_greedy_advance")
    for n in new:
        assert n in names, n
    assert "#define MM355_GREEDY_MAX_EOS 8" in open(os.path.join(REPO, "include", "mm355.h")).read()
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(lib.LIB_PATH)
    for n in new:
        assert hasattr(so, n), n
    L = lib.load()
    P = 4096                                                     # a non-null, 16-byte aligned stand-in: no kernel is launched on the error path
    assert L.mm355_argmax_rows_ws_bytes(3, 128258) == 3 * 32 * 8 and L.mm355_argmax_rows_ws_bytes(1, 4096) == 8
    assert L.mm355_argmax_rows_ws_bytes(0, 5) == 0 and L.mm355_argmax_rows_ws_bytes(5, 0) == 0
    #                              x  R  C  out ws bytes stream
    assert L.mm355_argmax_rows_f32(0, 1, 8, P, P, 8, 0) == -1
    assert L.mm355_argmax_rows_f32(P, 1, 8, 0, P, 8, 0) == -1
    assert L.mm355_argmax_rows_f32(P, 1, 8, P, 0, 8, 0) == -1
    assert L.mm355_argmax_rows_f32(P, 1, 0, P, P, 8, 0) == -1        # C = 0
    assert L.mm355_argmax_rows_f32(P, 0, 8, P, P, 8, 0) == -1
    assert L.mm355_argmax_rows_f32(P, 2, 8, P, P, 8, 0) == -1        # a workspace for one row
    #                               a  lda b ldb mask out ldo R  h  stream
    assert L.mm355_rows_select_bf16(0, 64, P, 64, P, P, 64, 2, 64, 0) == -1
    assert L.mm355_rows_select_bf16(P, 64, P, 64, 0, P, 64, 2, 64, 0) == -1
    assert L.mm355_rows_select_bf16(P, 64, P, 64, P, P, 64, 0, 64, 0) == -1
    assert L.mm355_rows_select_bf16(P, 64, P, 64, P, P, 64, 2, 60, 0) == -1       # h % 8
    assert L.mm355_rows_select_bf16(P, 64, P + 8, 64, P, P, 64, 2, 64, 0) == -1   # a misaligned row
    assert L.mm355_rows_select_bf16(P, 64, P, 68, P, P, 64, 2, 64, 0) == -1       # a stride that misaligns the second row
    eos = (ctypes.c_int32 * 9)(*range(1, 10))
    E = ctypes.addressof(eos)

    def advance(tok=P, B=2, C=320, state=P, live=P, embed=P, rows=320, fed=P, ldf=64, z=P, x=P, h=64, Dz=32, tlog=P, zlog=P, n_eos=2):
        return L.mm355_greedy_advance(tok, B, C, state, state, state, state, state, state, live, embed, 64, rows, fed, ldf, z, Dz, x, 64, h, Dz,
                                      tlog, 4, zlog, 4, 300, 301, 4, 12, E, n_eos, 0)
    for null in ("tok", "state", "live", "embed", "fed", "z", "x", "tlog", "zlog"):
        assert advance(**{null: 0}) == -1, null
    assert advance(C=0) == -1 and advance(B=0) == -1
    assert advance(n_eos=9) == -1                                # more than 8 eos ids
    assert advance(C=321) == -1                                  # an argmax id could lie beyond the embedding's rows
    assert advance(x=P + 8) == -1 and advance(ldf=68) == -1 and advance(h=60) == -1       # misaligned rows


def _tiny_cpu_model():
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
               rms_norm_eps=1e-5, rope_theta=500000.0)
    geo = dict(hidden_size=64, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14)
    return build_model(llm, geo, num_image_tokens=4, max_length=64)


def test_greedy_decode_refuses_a_batch_it_cannot_take_by_name():
    model = _tiny_cpu_model().eval()
    emb = torch.zeros(2, 5, 64, dtype=torch.bfloat16)
    right = torch.tensor([[1, 1, 1, 1, 1], [1, 1, 1, 0, 0]])
    with pytest.raises(NotImplementedError, match="LEFT-padded prompts"):
        model.greedy_decode(None, right, emb, max_new_tokens=4)
    with pytest.raises(ValueError, match="does not match the prompt batch"):
        model.greedy_decode(None, right[:, :4], emb, max_new_tokens=4)
    with pytest.raises(NotImplementedError, match=r"use_cache=False\) handles one sequence"):
        model.greedy_decode(None, None, emb, max_new_tokens=4, use_cache=False)
