"""Sampled decoding in the device token loop, the parts that need no GPU: the C ABI's symbols and validation, functional.philox4x32_10
against the published known answers, functional.sample_row_host (the specification of mm355_sample_rows_f32) against transformers'
logits warpers, and greedy_decode's refusals of bad sampling arguments."""
import ctypes
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mm355_philox_uniform_rows", "mm355_sample_rows_ws_bytes", "mm355_sample_rows_f32")


def test_sample_symbols_and_validation_without_a_gpu():
    from metamorph_amd import lib
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
    P = 4096                                                     # a non-null, 16-byte aligned stand-in: no kernel is launched on the error path
    assert L.mm355_sample_rows_ws_bytes(3, 128258) >= 0

    def sample(x=P, R=2, C=64, inv_t=1.0, top_k=0, top_p=1.0, u=P, out=P, stats=0, ws=P, ws_bytes=1 << 30):
        return L.mm355_sample_rows_f32(x, R, C, inv_t, top_k, top_p, u, out, stats, ws, ws_bytes, 0)
    for null in ("x", "u", "out"):
        assert sample(**{null: 0}) == -1, null
    assert sample(R=0) == -1 and sample(C=0) == -1 and sample(R=65536) == -1 and sample(C=2**31 - 1) == -1
    assert sample(ws=P + 2) == -1                                # a misaligned workspace
    assert sample(ws_bytes=L.mm355_sample_rows_ws_bytes(2, 64) - 1) == -1
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert sample(inv_t=bad) == -1, bad
    assert sample(top_k=-1) == -1
    for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert sample(top_p=bad) == -1, bad
    #                                  seed ids ctr u  R  stream
    assert L.mm355_philox_uniform_rows(1, 0, P, P, 2, 0) == -1
    assert L.mm355_philox_uniform_rows(1, P, 0, P, 2, 0) == -1
    assert L.mm355_philox_uniform_rows(1, P, P, 0, 2, 0) == -1
    assert L.mm355_philox_uniform_rows(1, P, P, P, 0, 0) == -1


def test_philox4x32_10_known_answers():
    """the known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10)"""
    from metamorph_amd import functional as F
    f = 0xFFFFFFFF
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((f, f, f, f), (f, f), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert F.philox4x32_10(ctr, key) == want, (ctr, key)
    assert F.philox_uniform_host(0, 0, 0) == (0x6627e8d5 >> 8) * 2.0 ** -24
    seed = 0x299f31d0a4093822                                    # key words = (low, high), counter = (counter, stream id, 0, 0)
    assert F.philox_uniform_host(seed, 7, 3) == (F.philox4x32_10((3, 7, 0, 0), (0xa4093822, 0x299f31d0))[0] >> 8) * 2.0 ** -24
    us = [F.philox_uniform_host(11, s, c) for s in range(4) for c in (0, 1, 2**31 - 1)]
    assert all(0.0 <= u < 1.0 for u in us) and len(set(us)) == len(us)


SETTINGS = [(1.0, 0, 1.0), (0.7, 0, 0.9), (0.7, 50, 1.0), (1.3, 40, 0.95), (0.7, 1, 1.0), (0.7, 5, 0.5)]


@pytest.mark.parametrize("C", [37, 1000])
def test_sample_row_host_keeps_what_the_hf_warpers_keep(C):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    from metamorph_amd import functional as F
    rng = np.random.default_rng(C)
    for scale in (4.0, 1.0):
        for T, top_k, top_p in SETTINGS:
            x = rng.standard_normal(C) * scale
            assert len(np.unique(x)) == C                        # tie-free
            s = torch.from_numpy(x)[None]
            if T != 1.0:
                s = TemperatureLogitsWarper(T)(None, s)
            if top_k:
                s = TopKLogitsWarper(top_k)(None, s)
            if top_p < 1.0:
                s = TopPLogitsWarper(top_p)(None, s)
            want = set(torch.nonzero(torch.isfinite(s[0])).view(-1).tolist())
            u = float(rng.random())
            cand, tau_lo, tau_hi, Z = F.sample_row_host(x, 1.0 / T, top_k, top_p, u)
            assert tau_lo == tau_hi and tau_lo in x
            kept = np.nonzero(x >= tau_lo)[0]
            assert set(kept.tolist()) == want, (scale, T, top_k, top_p)
            w = np.exp((x - x.max()) / T)
            assert abs(Z - w[kept].sum()) <= 1e-12 * Z
            cdf = np.cumsum(w[kept])
            assert cand == [int(kept[int(np.searchsorted(cdf, u * Z, side="right"))])], (scale, T, top_k, top_p, u)
            # the bands hold the exact answer, and at eps = 0 they are the exact answer
            c2, lo2, hi2, Z2 = F.sample_row_host(x, 1.0 / T, top_k, top_p, u, eps=1e-4)
            assert lo2 <= tau_lo <= hi2 and Z2 == Z and cand[0] in c2
            c3, _, _, Z3 = F.sample_row_host(x, 1.0 / T, top_k, top_p, u, tau=float(x.max()))
            assert c3 == [int(np.argmax(x))] and Z3 == 1.0


def test_sample_row_host_edges():
    from metamorph_amd import functional as F
    x = np.array([1.0, 3.0, 3.0, -np.inf, 2.0, 3.0])
    assert F.sample_row_host(x, 1.0, 1, 1.0, 0.5) == ([2], 3.0, 3.0, 3.0)          # ties at the k-th value are all kept
    assert F.sample_row_host(x, 1.0, 1, 1.0, 0.0)[0] == [1] and F.sample_row_host(x, 1.0, 1, 1.0, 1 - 2.0 ** -24)[0] == [5]
    cand, lo, hi, Z = F.sample_row_host(x, 1.0, 0, 1.0, 1 - 2.0 ** -24)
    assert cand == [5] and lo == hi == -np.inf                   # no filter: tau is the row minimum, -inf weighs nothing
    assert F.sample_row_host(x, 1.0, 0, 1.0, 1 - 2.0 ** -24, eps=1e-4)[0] == [5]
    nan = np.array([0.0, np.nan, 5.0, np.nan])
    cand, lo, hi, Z = F.sample_row_host(nan, 1.0, 0, 0.9, 0.3)
    assert cand == [1] and np.isnan(lo) and Z == 0.0
    assert F.sample_row_host(np.array([0.0, np.inf, np.inf]), 1.0, 0, 0.9, 0.3) == ([1], np.inf, np.inf, 0.0)
    assert F.sample_row_host(np.full(4, -np.inf), 1.0, 0, 0.9, 0.3) == ([0], -np.inf, -np.inf, 0.0)


def _tiny_cpu_model():
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=320,
               rms_norm_eps=1e-5, rope_theta=500000.0)
    geo = dict(hidden_size=64, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14)
    return build_model(llm, geo, num_image_tokens=4, max_length=64)


def test_greedy_decode_refuses_bad_sampling_arguments_by_name():
    model = _tiny_cpu_model().eval()
    emb = torch.zeros(2, 5, 64, dtype=torch.bfloat16)

    def call(**kw):
        return model.greedy_decode(None, None, emb, max_new_tokens=4, do_sample=True, **{"temperature": 0.7, **kw})
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="top_p"):
            call(top_p=bad)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="top_k"):
            call(top_k=bad)
    for bad in (-0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            call(temperature=bad)
    with pytest.raises(ValueError, match="num_beams"):
        call(num_beams=4)
    with pytest.raises(ValueError, match="stream_ids"):
        call(stream_ids=[0])
    with pytest.raises(NotImplementedError, match="use_cache=False"):
        call(use_cache=False)
    with pytest.raises(NotImplementedError, match="use_cache=False"):
        model.greedy_decode(None, None, emb[:1], max_new_tokens=4, do_sample=True, temperature=0.7, use_cache=False)
    # the sampler is chosen by (do_sample, temperature) alone
    S = type(model)._sampler_of
    assert S(None, 0.7, 5, 0.9, None, 1, None, 2) is None and S(True, None, 5, 0.9, None, 1, None, 2) is None
    assert S(True, 0.0, 5, 0.9, None, 1, None, 2) is None
    assert S(True, 0.5, None, None, 1, 9, None, 3) == (2.0, 0, 1.0, 9, [0, 1, 2])
    torch.manual_seed(1234)
    a = S(True, 0.5, 50, 0.9, None, None, [4, 5], 2)
    torch.manual_seed(1234)
    b = S(True, 0.5, 50, 0.9, None, None, [4, 5], 2)
    assert a == b and a[4] == [4, 5] and 0 <= a[3] < 2**64 and a[3] != S(True, 0.5, 50, 0.9, None, None, [4, 5], 2)[3]
