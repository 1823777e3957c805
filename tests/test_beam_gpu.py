"""Beam search in the device token loop, on the device: mm355_attn_decode_shared_idx / _idx_f8 against the fp32 formula of
test_shared_prefix_gpu.py extended by the table (everything the contract says is never read poisoned) and bit for bit against
mm355_attn_decode_shared; mm355_beam_select_rows_f32 and mm355_beam_advance bit for bit against their host models
(functional.beam_select_host / beam_step_host); then the loop (functional.BeamLoopGraph, beam_decode) on the tiny decode model of
test_greedy_batch_gpu.py: every step against the host model, replay against eager launches and polling, and against the HF path."""
import contextlib
import math

import numpy as np
import pytest
import torch

import test_greedy_batch_gpu as G  # noqa: E402  (the tiny fixture models)
import test_shared_prefix_gpu as SP  # noqa: E402  (the fp32 formula)
from test_attn_extend_gpu import close, kv8_cache  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from metamorph_amd import ops as o
    from metamorph_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return o


# ------------------------------------------------------------------ 1. indexed own rows in the shared-prefix attention
#             B  Hq Hkv  d    P  own rows
ATTN_CASES = [(2, 8, 2, 128, 1, 1),                                # the smallest case
              (3, 4, 4, 64, 63, 64),                               # G = 1, exactly one tile of own rows
              (8, 32, 8, 128, 65, 130),                            # three tiles: the table is fetched two tiles ahead
              (4, 8, 1, 64, 0, 5),                                 # empty prefix
              (3, 8, 2, 128, 513, 0)]                              # no own rows: no entry is read
ATTN_IDS = [f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-P{c[4]}-own{c[5]}" for c in ATTN_CASES]
PAD = 5


def beam_table(B, own, cols, seed):
    """own_block of B beams after `own` steps of functional.beam_step_host on random parents"""
    from metamorph_amd import functional as F
    rng = np.random.default_rng(seed)
    state = F.beam_state_host(B, cols - 1)
    pw = F.beam_len_pow(cols - 1, 1.0)
    M = 2 * B
    for n in range(own):
        idx = (rng.integers(0, B, M) * 50 + rng.permutation(50)[:M]).astype(np.int32)
        F.beam_step_host(state, np.sort(rng.standard_normal(M).astype(np.float32))[::-1] - np.float32(n), idx, 50, (), cols, pw)
    return torch.from_numpy(state["own_block"][:, :cols].copy())


def tables(case):
    B, _, _, _, P, own = case
    cols = own + 3
    g = torch.Generator().manual_seed(3 + P + own)
    return {"random": torch.randint(0, B, (B, cols), generator=g, dtype=torch.uint8), "beams": beam_table(B, own, cols, seed=P + own)}


def gathered(t, tbl, P, own):
    """t [B, rows, ...] -> the same with own row j of sequence b taken from block tbl[b, j - P]"""
    out = t.clone()
    for b in range(t.shape[0]):
        for j in range(own):
            out[b, P + j] = t[int(tbl[b, j]), P + j]
    return out


def poison_unused(ts, tbl, P, own, value):
    """everything the contract says is never read: rows [0, P) and rows >= P + own of every block, and the own rows no query's table names"""
    B = tbl.shape[0]
    used = torch.zeros(B, ts[0].shape[1], dtype=torch.bool)
    for b in range(B):
        for j in range(own):
            used[int(min(int(tbl[b, j]), B - 1)), P + j] = True
    for t in ts:
        t[~used] = value


_ATTN = {}


def attn_inputs(case):
    """(q, ksh, vsh, kc, vc) of a case on the CPU, unpoisoned; made once"""
    if case not in _ATTN:
        B, Hq, Hkv, d, P, own = case
        rows = P + own + PAD
        g = torch.Generator().manual_seed(11 + P + own)
        mk = lambda *s: (torch.randn(*s, generator=g) * 0.7).bfloat16()      # noqa: E731
        _ATTN[case] = (mk(B, Hq, d), mk(P + 3, Hkv, d), mk(P + 3, Hkv, d), mk(B, rows, Hkv, d), mk(B, rows, Hkv, d))
    return _ATTN[case]


def _dev(case, q, ksh, vsh, kc, vc):
    B, Hq, Hkv, d, P, own = case
    return (q.view(B, Hq * d).to(DEV), ksh.view(-1, Hkv * d).to(DEV), vsh.view(-1, Hkv * d).to(DEV), kc.view(B, -1, Hkv * d).to(DEV),
            vc.view(B, -1, Hkv * d).to(DEV))


@pytest.mark.parametrize("kind", ["random", "beams"])
@pytest.mark.parametrize("case", ATTN_CASES, ids=ATTN_IDS)
def test_indexed_attention_against_the_formula(ops, case, kind):
    B, Hq, Hkv, d, P, own = case
    q, ksh, vsh, kc, vc = attn_inputs(case)
    tbl = tables(case)[kind].clone()
    lens = [P + own] * B
    ref = SP.formula(q, ksh, vsh, gathered(kc, tbl, P, own), gathered(vc, tbl, P, own), P, lens, Hq, Hkv, d)
    ksh, vsh, kc, vc = ksh.clone(), vsh.clone(), kc.clone(), vc.clone()
    ksh[P:], vsh[P:] = float("nan"), float("nan")
    poison_unused((kc, vc), tbl, P, own, float("nan"))
    tbl[:, own:] = 255                                             # entries at or beyond the length: never read
    rows = kc.shape[1]
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    args = _dev(case, q, ksh, vsh, kc, vc)
    for bound in (P + own if P + own else 1, rows):                # the tight bound, and the capacity as the token loop passes it
        got = ops.attn_decode_shared(*args, ld, P, bound, Hq, Hkv, d, d ** -0.5, own_block=tbl.to(DEV))
        close(got, ref, 1e-2, 1e-2, f"attn_decode_shared_idx {case} {kind} bound {bound}")
        assert torch.equal(ops.attn_decode_shared(*args, ld, P, bound, Hq, Hkv, d, d ** -0.5, own_block=tbl.to(DEV)), got)


@pytest.mark.parametrize("case", ATTN_CASES, ids=ATTN_IDS)
def test_null_and_identity_tables_are_the_unindexed_kernel(ops, case):
    B, Hq, Hkv, d, P, own = case
    q, ksh, vsh, kc, vc = attn_inputs(case)
    ld = torch.tensor([P + own] * B, dtype=torch.int32, device=DEV)
    args = _dev(case, q, ksh, vsh, kc, vc)
    ident = torch.arange(B, dtype=torch.uint8).view(B, 1).repeat(1, own + 3).to(DEV)
    L = ops._L()
    for bound in (max(P + own, 1), kc.shape[1]):
        want = ops.attn_decode_shared(*args, ld, P, bound, Hq, Hkv, d, d ** -0.5)
        assert torch.equal(ops.attn_decode_shared(*args, ld, P, bound, Hq, Hkv, d, d ** -0.5, own_block=ident), want), bound
        # the new entry point with a NULL table
        qd, ks, vs, kd, vd = args
        n_ws = int(L.mm355_attn_decode_shared_ws_floats(B, Hq, Hkv, d, P, bound))
        ws = torch.empty(n_ws, device=DEV, dtype=torch.float32)
        out = torch.empty_like(want)
        rc = L.mm355_attn_decode_shared_idx(qd.data_ptr(), qd.stride(0), ks.data_ptr(), vs.data_ptr(), ks.stride(0), kd.data_ptr(), vd.data_ptr(),
                                            kd.stride(1), kd.stride(0), ld.data_ptr(), 0, 0, P, bound, out.data_ptr(), out.stride(0), B, Hq, Hkv, d,
                                            d ** -0.5, ws.data_ptr(), n_ws, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(out, want), bound


@pytest.mark.parametrize("case", ATTN_CASES, ids=ATTN_IDS)
def test_indexed_f8_form_equals_the_bf16_form_on_the_dequantised_cache(ops, case):
    B, Hq, Hkv, d, P, own = case
    rows = P + own + PAD
    tbl = tables(case)["random"].clone()
    k8, ks, v8, vs = kv8_cache(B, rows, Hkv, d, seed=P + d + own)
    ksh8, kshs, vsh8, vshs = (t[0] for t in kv8_cache(1, P + 3, Hkv, d, seed=P + d + own + 1))
    deq = lambda t8, ts: ops.dequant_kv8(t8, ts, Hkv, d)           # noqa: E731  (before anything is poisoned)
    kb, vb, kshb, vshb = deq(k8, ks), deq(v8, vs), deq(ksh8, kshs), deq(vsh8, vshs)
    poison_unused((k8, v8), tbl, P, own, 0x7F)                     # the NaN byte and a NaN scale
    poison_unused((ks, vs, kb, vb), tbl, P, own, float("nan"))
    for t, val in ((ksh8, 0x7F), (vsh8, 0x7F), (kshs, float("nan")), (vshs, float("nan")), (kshb, float("nan")), (vshb, float("nan"))):
        t[P:] = val
    tbl[:, own:] = 255
    q = (torch.randn(B, Hq * d, generator=torch.Generator().manual_seed(5)) * 0.7).bfloat16().to(DEV)
    ld = torch.tensor([P + own] * B, dtype=torch.int32, device=DEV)
    D = lambda *ts: [t.to(DEV) for t in ts]                        # noqa: E731
    for bound in (max(P + own, 1), rows):
        ref = ops.attn_decode_shared(q, *D(kshb, vshb, kb, vb), ld, P, bound, Hq, Hkv, d, d ** -0.5, own_block=tbl.to(DEV))
        got = ops.attn_decode_shared_f8(q, *D(ksh8, vsh8, kshs, vshs, k8, v8, ks, vs), ld, P, bound, Hq, Hkv, d, d ** -0.5, own_block=tbl.to(DEV))
        assert bool(torch.isfinite(got.float()).all()) and torch.equal(got, ref), (case, bound)


def test_out_of_range_table_entries_stay_inside_the_cache(ops):
    """entries >= B are clamped to the last block: the output is that of the clamped table and no poisoned row shows"""
    case = ATTN_CASES[2]
    B, Hq, Hkv, d, P, own = case
    q, ksh, vsh, kc, vc = attn_inputs(case)
    tbl = tables(case)["random"].clone()
    tbl[::2, ::3] = 200
    tbl[1, 5] = 255
    tbl[3, own - 1] = B
    clamped = tbl.clamp(max=B - 1)
    kc, vc = kc.clone(), vc.clone()
    poison_unused((kc, vc), clamped, P, own, float("nan"))
    ld = torch.tensor([P + own] * B, dtype=torch.int32, device=DEV)
    args = _dev(case, q, ksh, vsh, kc, vc)
    got = ops.attn_decode_shared(*args, ld, P, kc.shape[1], Hq, Hkv, d, d ** -0.5, own_block=tbl.to(DEV))
    assert bool(torch.isfinite(got.float()).all())
    assert torch.equal(got, ops.attn_decode_shared(*args, ld, P, kc.shape[1], Hq, Hkv, d, d ** -0.5, own_block=clamped.to(DEV)))


# ------------------------------------------------------------------ 2. candidate selection
def select_rows(K, V, seed):
    """name -> (x [K, V] fp32, running [K] fp32)"""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda s=1.0: torch.randn(K, V, generator=g) * s         # noqa: E731
    run = -torch.rand(K, generator=g) * 5
    step0 = torch.full((K,), -1e9)
    step0[0] = 0
    fam = {"random": (rnd(3.0), run), "peaked": (rnd(350.0), run), "step 0": (rnd(3.0), step0), "peaked, step 0": (rnd(350.0), step0)}
    x = rnd(3.0)
    x[torch.rand(K, V, generator=g) < 0.4] = float("-inf")
    x[:, V // 2] = 1.0                                             # (every row keeps a finite entry)
    fam["-inf entries"] = (x, run)
    x = rnd(3.0)
    x[0] = -2.5                                                    # a row of equal values: the M lowest indices of that row
    fam["a row of equal values"] = (x, torch.zeros(K))
    fam["equal rows and equal scores"] = (torch.full((K, V), 0.75), torch.zeros(K))
    return fam


def _same_floats(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and a[~np.isnan(a)].tobytes() == b[~np.isnan(b)].tobytes()


def _check_select(ops, x, run, M, what, stats_band=True):
    from metamorph_amd import functional as F
    K, V = x.shape
    xd, rd = x.to(DEV).contiguous(), run.to(DEV).contiguous()
    stats, val, idx = ops.beam_select_rows(xd, rd, M)
    stats2, val2, idx2 = ops.beam_select_rows(xd, rd, M)
    stats, val, idx = stats.cpu().numpy(), val.cpu().numpy(), idx.cpu().numpy()
    assert _same_floats(stats, stats2.cpu().numpy()) and _same_floats(val, val2.cpu().numpy()) and np.array_equal(idx, idx2.cpu().numpy()), what
    lp = F.beam_logprob_rows_host(x.numpy(), stats)
    want_val, want_idx = F.beam_select_host(lp, run.numpy(), M)
    assert np.array_equal(idx, want_idx), (what, idx.tolist(), want_idx.tolist())
    assert _same_floats(val, want_val), (what, val.tolist(), want_val.tolist())
    if stats_band:
        # the band token_note_rows_f32 is held to: 1e-4 + 2^-22 |value|
        x64 = x.double()
        m = x64.max(1).values
        lse = torch.log(torch.exp(x64 - m[:, None]).sum(1))
        for got, ref in ((stats[:, 0], m.numpy()), (stats[:, 1], lse.numpy())):
            err = np.abs(got.astype(np.float64) - ref)
            print(f"   {what}: stats err {err.max():.3e}")
            assert (err <= 1e-4 + 2.0 ** -22 * np.abs(ref)).all(), (what, err.max())
    return stats, val, idx


@pytest.mark.parametrize("n_eos", [0, 1, 8])
@pytest.mark.parametrize("K,V", [(K, V) for K in (1, 2, 3, 8) for V in (37, 1000)] + [(4, 128258)])
def test_beam_select_rows_equals_the_host_model(ops, K, V, n_eos):
    from metamorph_amd import functional as F
    M = F.beam_candidates(K, n_eos)
    for name, (x, run) in select_rows(K, V, seed=1000 * K + V + n_eos).items():
        stats, val, idx = _check_select(ops, x, run, M, f"K={K} V={V} M={M} {name}")
        if name == "a row of equal values" and K == 1:
            assert idx.tolist() == list(range(M)), idx.tolist()      # the index tie rule
        if name == "equal rows and equal scores":
            assert idx.tolist() == list(range(M)), idx.tolist()


@pytest.mark.parametrize("K,V", [(3, 1000), (4, 128258)])
def test_beam_select_rows_nan_and_inf_rows_follow_the_documented_rule(ops, K, V):
    """a NaN in a row, a +inf maximum or a row of -inf only: that row's lse and all its scores are NaN, and a NaN sorts after every number"""
    from metamorph_amd import functional as F
    g = torch.Generator().manual_seed(V)
    M = 2 * K
    for bad_row, make in ((0, lambda r: r.__setitem__(V // 3, float("nan"))), (1, lambda r: r.__setitem__(V - 1, float("inf"))),
                          (K - 1, lambda r: r.fill_(float("-inf")))):
        x = torch.randn(K, V, generator=g) * 3
        make(x[bad_row])
        stats, val, idx = _check_select(ops, x, torch.zeros(K), M, f"K={K} V={V} bad row {bad_row}", stats_band=False)
        assert np.isnan(stats[bad_row, 1]) and not np.isnan(np.delete(stats[:, 1], bad_row)).any()
        assert not np.isnan(val).any() and not (idx // V == bad_row).any()      # the other rows hold M numbers
    x = torch.randn(K, V, generator=g)
    x[1:, 5] = float("nan")                                        # one good row of V >= M numbers... and with M > what it holds:
    stats, val, idx = _check_select(ops, x[:, :3].contiguous(), torch.zeros(K), 5, f"K={K} V=3, two NaN rows", stats_band=False)
    x3 = x[:, :3].clone()
    x3[1:, 1] = float("nan")
    stats, val, idx = _check_select(ops, x3.contiguous(), torch.zeros(K), 5, f"K={K} V=3, NaN rows fill the list", stats_band=False)
    assert np.isnan(val[3:]).all() and idx[3:].tolist() == [3, 4] and not np.isnan(val[:3]).any()


# ------------------------------------------------------------------ 3. the bookkeeping
ADV_V, ADV_EOS = 50, (7, 9)


def advance_stream(K, steps, seed, eos_rate, decay):
    """per step the M sorted candidates (values, flat indices): random parents, ids that hit an eos id at `eos_rate`, values that fall by
    about `decay` per step"""
    rng = np.random.default_rng(seed)
    M = 3 * K
    plain = [i for i in range(ADV_V) if i not in ADV_EOS]
    out = []
    for n in range(steps):
        val = np.sort((rng.standard_normal(M) - decay * n).astype(np.float32))[::-1].copy()
        ids = np.where(rng.random(M) < eos_rate, rng.choice(ADV_EOS, M), rng.choice(plain, M))
        out.append((val, (rng.integers(0, K, M) * ADV_V + ids).astype(np.int32)))
    return out


ADV_STREAMS = [dict(K=2, steps=6, seed=0, eos_rate=0.3, decay=1.0), dict(K=3, steps=9, seed=1, eos_rate=0.15, decay=3.0),
               dict(K=4, steps=12, seed=2, eos_rate=0.4, decay=0.2), dict(K=8, steps=7, seed=3, eos_rate=0.1, decay=1.0),
               dict(K=3, steps=5, seed=4, eos_rate=0.0, decay=1.0), dict(K=2, steps=12, seed=5, eos_rate=0.12, decay=2.0)]


def run_advance_host(stream, K, new, lp, es, cover=None):
    """the host model over a stream -> the state after every step (copies)"""
    from metamorph_amd import functional as F
    state = F.beam_state_host(K, new)
    pw = F.beam_len_pow(new, lp)
    snaps = []
    for val, idx in stream:
        if cover is not None and state["live"][0]:
            n, unsat = int(state["scal"][1]), int(state["scal"][0])
            hit = np.isin(idx % ADV_V, ADV_EOS) | (n + 1 >= new)
            cover["eos among the first K"] |= bool(hit[:K].any() and not hit.all())
            cover["eos only beyond the first K"] |= bool(hit[K:].any() and not hit[:K].any())
            cover["last step"] |= bool(n + 1 >= new)
        F.beam_step_host(state, val, idx, ADV_V, ADV_EOS, new, pw, lp, es)
        if cover is not None:
            cover["heuristic turns off"] |= bool(snaps and snaps[-1]["scal"][0] == 1 and state["scal"][0] == 0)
            cover["stops before the last step"] |= bool(not state["live"][0] and state["scal"][1] < new)
        snaps.append({k: v.copy() for k, v in state.items()})
    return snaps


@pytest.mark.parametrize("es", [False, True, "never"], ids=["es-False", "es-True", "es-never"])
@pytest.mark.parametrize("lp", [0.0, 1.0, 2.0, -1.0])
def test_beam_advance_equals_the_host_model(ops, lp, es):
    from metamorph_amd import functional as F
    cover = dict.fromkeys(("eos among the first K", "eos only beyond the first K", "last step", "heuristic turns off",
                           "stops before the last step"), False)
    h = 64
    embed = torch.randn(ADV_V, h, generator=torch.Generator().manual_seed(1)).bfloat16().to(DEV)
    for spec in ADV_STREAMS:
        K, steps = spec["K"], spec["steps"]
        new = steps - 2 if spec["seed"] % 2 else steps             # some streams run past their last step: the launches after it write nothing
        stream = advance_stream(**spec)
        snaps = run_advance_host(stream, K, new, lp, es, cover)
        host = F.beam_state_host(K, new)
        state = {n: torch.from_numpy(host[n]).to(DEV) for n in F.BEAM_STATE}
        pw = torch.from_numpy(F.beam_len_pow(new, lp)).to(DEV)
        x_in = torch.full((K, h), -7.0, dtype=BF16, device=DEV)
        for t, (val, idx) in enumerate(stream):
            was_live = bool(snaps[t - 1]["live"][0]) if t else True
            if not was_live:                                       # poisoned outputs: a finished search writes nothing
                state["tok"].fill_(-77)
                state["parent"].fill_(-77)
                x_in.fill_(-7.0)
            before = {n: v.clone() for n, v in state.items()}
            ops.beam_advance(torch.from_numpy(val).to(DEV), torch.from_numpy(idx).to(DEV), ADV_V, state, pw, new, lp,
                             F.BEAM_EARLY_STOPPING[es], ADV_EOS, embed=embed, x_in=x_in)
            if not was_live:
                assert all(torch.equal(state[n], before[n]) for n in state) and float(x_in.float().min()) == -7.0 == float(x_in.float().max()), t
                continue
            for n in F.BEAM_STATE:
                got, want = state[n].cpu().numpy(), snaps[t][n]
                if n == "own_block":                               # (columns beyond the step are whatever they were)
                    got, want = got[:, :t + 1], want[:, :t + 1]
                if n in ("tok_log", "parent_log"):
                    got, want = got[:t + 1], want[:t + 1]
                same = _same_floats(got, want) if got.dtype == np.float32 else np.array_equal(got, want)
                assert same, (spec, t, n, got.tolist(), want.tolist())
            assert torch.equal(x_in, embed[state["tok"].long()]), (spec, t)
    missing = [k for k, v in cover.items() if not v]
    assert not missing, missing


@pytest.mark.parametrize("es", [False, True, "never"], ids=["es-False", "es-True", "es-never"])
def test_beam_advance_on_a_full_pool(ops, es):
    """A search never reaches a step with a full pool under early_stopping=True (it stops there), so that branch is entered from a crafted
    state: every pool entry finished, the search live.  With early stopping every new hypothesis is pushed below the pool; without, a
    better one replaces the worst entry."""
    from metamorph_amd import functional as F
    K, new, lp = 3, 8, 1.0
    host = F.beam_state_host(K, new)
    host["running"][:] = (-1.0, -1.5, -2.0)
    host["fin_score"][:] = (-0.9, -1.1, -1.3)
    host["fin_flag"][:] = 1
    host["fin_end"][:] = ((0, 0, 7), (1, 1, 9), (1, 2, 7))
    host["scal"][:] = (1, 2)
    state = {n: torch.from_numpy(host[n].copy()).to(DEV) for n in F.BEAM_STATE}
    val = np.array([-2.0, -2.2, -2.4, -2.6, -2.8, -3.0, -3.5, -4.0, -5.0], dtype=np.float32)
    idx = np.array([0 * ADV_V + 7, 1 * ADV_V + 3, 2 * ADV_V + 9, 0 * ADV_V + 4, 1 * ADV_V + 5, 2 * ADV_V + 6, 0 * ADV_V + 8, 7, 9], dtype=np.int32)
    pw = F.beam_len_pow(new, lp)
    F.beam_step_host(host, val, idx, ADV_V, ADV_EOS, new, pw, lp, es)
    ops.beam_advance(torch.from_numpy(val).to(DEV), torch.from_numpy(idx).to(DEV), ADV_V, state, torch.from_numpy(pw).to(DEV), new, lp,
                     F.BEAM_EARLY_STOPPING[es], ADV_EOS)
    for n in F.BEAM_STATE:
        got, want = state[n].cpu().numpy(), host[n]
        if n == "own_block":
            got, want = got[:, :3], want[:, :3]
        if n in ("tok_log", "parent_log"):
            got, want = got[2:3], want[2:3]
        assert _same_floats(got, want) if got.dtype == np.float32 else np.array_equal(got, want), (n, got.tolist(), want.tolist())
    # -2.0 / 3 = -0.667 beats every pool entry: it enters the pool unless early stopping closed it
    assert (host["fin_score"][0] == np.float32(-2.0) / np.float32(3.0)) == (es is not True), host["fin_score"].tolist()
    assert host["live"][0] == (0 if es is True else 1)


# ------------------------------------------------------------------ 4. the loop
# Token prompts for the diverging-sequences test's tiny decode model (test_greedy_batch_gpu._diverge_model: sparse lm_head, peaked rows):
# per number of beams (length, seed) pairs, chosen on an MI355X so that every decision of the search has the margin asserted below.
BEAM_EOS = (G.EOT,)
BEAM_NEW = 8                                                      # where no margin is at stake
BEAM_PROMPTS = {2: ((15, 51), (12, 73)), 4: ((12, 5), (18, 53))}  # the second of each finishes hypotheses early ((12, 73) stops after 2 steps)
HF_NEW = {2: 6, 4: 4}                                             # new tokens in the comparisons whose margins are asserted
# Largest |accumulated score in the device beam loop - accumulated score on the HF path| of one candidate (a sum of log-probabilities), over
# all steps and candidates of these prompts, measured on MI355X: the two routes differ in the attention kernel (the shared-prefix split
# against one pass per sequence), so their logits differ in the last bf16 digits.  2026-10-19: 0.02494 and 0.02354 (two beams), 0.02210
# and 0.02652 (four beams); the margins of the four searches are 0.390, 0.233, 0.137 and 0.075.
MEASURED_SCORE_DIFF = {2: 0.0250, 4: 0.0266}


@contextlib.contextmanager
def variant(name, value):
    from metamorph_amd import functional as F
    old = F.set_variant(name, value)
    try:
        yield
    finally:
        F.set_variant(name, old)


def prompt_ids(length, seed):
    return torch.randint(0, 128256, (1, length), generator=torch.Generator().manual_seed(7919 * length + seed)).to(DEV)


def beam_run(model, ids, K, graph=True, poll=None, record=False, mask=None, **kw):
    """beam_decode(num_return_sequences=K, output_scores=True) of a token prompt -> (ids, scores, loop, trace); trace (record=True): per
    tail the loop's logits, statistics, candidates and state, copied to the host"""
    from metamorph_amd import functional as F
    trace = []

    def on_tail(loop):
        trace.append(dict(logits=loop.logits.cpu().numpy(), stats=loop.stats.cpu().numpy(), val=loop.cand_val.cpu().numpy(),
                          idx=loop.cand_idx.cpu().numpy(), state={n: t.cpu().numpy() for n, t in loop.state.items()}))
    init = F.BeamLoopGraph.__init__

    def patched(self, *a, **k):
        init(self, *a, **k)
        self.on_tail = on_tail if record else None
    F.BeamLoopGraph.__init__ = patched
    if poll is not None:
        model.config.mm355_greedy_poll_steps = poll
    try:
        with variant("decode_graph", graph):
            kw.setdefault("max_new_tokens", BEAM_NEW)
            kw.setdefault("eos_token_id", BEAM_EOS)
            out, scores = model.beam_decode(None, mask, model.get_model().embed_tokens(ids), K, num_return_sequences=K, output_scores=True, **kw)
    finally:
        F.BeamLoopGraph.__init__ = init
        if poll is not None:
            del model.config.mm355_greedy_poll_steps
    assert all(o.dtype == torch.int32 for o in out) and scores.dtype == torch.float32
    return [o.tolist() for o in out], scores.cpu().numpy(), model._beam_loop, trace


def host_search(rows_fn, K, V, eos, new, lp=1.0, es=False, check=None):
    """beam_search_host with its steps laid open: -> (per step (values, indices) of the candidates, the smallest decision margin, the
    final state).  check(n, val, idx, state): called after every step.
    The margin: a search's result is made of set decisions on ACCUMULATED scores -- which K candidates that did not hit run on (the
    K-th of them against the next one), which candidates that hit sit among the first K (entry K - 1 against entry K), which
    finished hypotheses the pool keeps and in which order (neighbours among the first K + 1 finished scores), and whether the best
    running beam can still beat the worst pool entry.  Two routes whose accumulated scores differ by at most D take the same decisions
    wherever these gaps exceed 2 D; the order inside the set of running beams only renumbers the slots."""
    from metamorph_amd import functional as F
    state = F.beam_state_host(K, new)
    pw = F.beam_len_pow(new, lp)
    M = F.beam_candidates(K, len(eos))
    margin, steps = float("inf"), []
    n = 0
    while state["live"][0]:
        val, idx = F.beam_select_host(rows_fn(n, state), state["running"], M)
        hit = np.isin(idx % V, eos) | (n + 1 >= new)
        v64 = val.astype(np.float64)
        gaps = []
        if not hit.all():
            nh = np.flatnonzero(~hit)
            assert len(nh) > K, (n, "every candidate that did not hit runs on: the next one is not in the list")
            gaps.append(v64[nh[K - 1]] - v64[nh[K]])
        if hit[K - 1] or hit[K]:                                  # (which hypothesis finishes: also where both hit, and in the last step)
            gaps.append(v64[K - 1] - v64[K])
        fin = np.concatenate([state["fin_score"][state["fin_flag"] != 0].astype(np.float64), v64[:K][hit[:K]] / float(pw[n])])
        fin = np.sort(fin)[::-1][:K + 1]
        if fin.size > 1:
            gaps.append(float((-np.diff(fin)).min()))
        F.beam_step_host(state, val, idx, V, eos, new, pw, lp, es)
        if state["fin_flag"].all() and not hit.all():             # the heuristic decides: by how much?
            hyp = pw[(new if es == "never" and lp > 0 else n + 1) - 1]
            gaps.append(abs(float(state["running"][0]) / float(hyp) - float(state["fin_score"].min())))
        margin = min([margin] + [float(g) for g in gaps])
        steps.append((val, idx))
        if check is not None:
            check(n, val, idx, state)
        n += 1
    return steps, margin, state


def replay_on_host(trace, K, V, eos, new, lp=1.0, es=False):
    """the host model driven by the loop's own logits, every step of the loop asserted bit for bit -> host_search's result"""
    from metamorph_amd import functional as F

    def check(n, val, idx, state):
        t = trace[n]
        assert np.array_equal(idx, t["idx"]) and _same_floats(val, t["val"]), (n, idx.tolist(), t["idx"].tolist())
        for name in F.BEAM_STATE:
            got, want = t["state"][name], state[name]
            if name == "own_block":
                got, want = got[:, :n + 1], want[:, :n + 1]
            assert _same_floats(got, want) if got.dtype == np.float32 else np.array_equal(got, want), (n, name, got.tolist(), want.tolist())
    return host_search(lambda n, state: F.beam_logprob_rows_host(trace[n]["logits"], trace[n]["stats"]), K, V, eos, new, lp, es, check)


def score_difference(steps_a, steps_b):
    """the largest difference between two routes' accumulated scores of one candidate, over the steps both ran"""
    worst = 0.0
    for (va, ia), (vb, ib) in zip(steps_a, steps_b):
        b = dict(zip(ib.tolist(), vb.tolist()))
        worst = max([worst] + [abs(float(v) - b[i]) for i, v in zip(ia.tolist(), va.tolist()) if i in b and abs(v) < 1e8 and abs(b[i]) < 1e8])
    return worst


@pytest.mark.parametrize("K", [2, 4])
def test_every_step_of_the_eager_loop_equals_the_host_model(K):
    from metamorph_amd import functional as F
    _, model = G._diverge_model()
    V = model.lm_head.weight.shape[0]
    for length, seed in BEAM_PROMPTS[K]:
        ids, scores, loop, trace = beam_run(model, prompt_ids(length, seed), K, graph=False, record=True, max_new_tokens=HF_NEW[K])
        assert not loop.graphs and len(trace) == loop.steps + 1
        _, margin, state = replay_on_host(trace, K, V, BEAM_EOS, HF_NEW[K])
        want_ids, want_scores, flags = F.beam_hypotheses_host(state)
        assert ids == [i.tolist() for i in want_ids] and _same_floats(scores, want_scores) and flags.all()
        print(f"   K={K} prompt {(length, seed)}: {loop.steps + 1} tails, margin {margin:.4f}, ids {ids}, scores {scores.tolist()}")


def test_replay_eager_and_polling_are_one_computation():
    _, model = G._diverge_model()
    K = 4
    p = prompt_ids(*BEAM_PROMPTS[K][0])
    ids, scores, loop, _ = beam_run(model, p, K, graph=True)
    assert loop.graphs and len(loop.graphs) == 1
    for graph in (True, False):
        for poll in (1, 5, 8):
            i2, s2, l2, _ = beam_run(model, p, K, graph=graph, poll=poll)
            assert i2 == ids and s2.tobytes() == scores.tobytes(), (graph, poll)
            assert all(np.array_equal(l2.final[n], loop.final[n]) for n in ("fin_end", "fin_flag", "fin_score", "running")), (graph, poll)
            assert l2.poll == poll and l2.host_reads <= math.ceil(l2.steps / poll) + 1 and l2.steps <= BEAM_NEW - 1
            assert bool(l2.graphs) == graph


def _strip(row):
    """a generated row of the HF path without its padding: up to and including the first eos id"""
    for i, t in enumerate(row):
        if t in BEAM_EOS:
            return row[:i + 1]
    return row


@pytest.mark.parametrize("K", [2, 4])
def test_beam_decode_returns_the_hf_paths_hypotheses(K):
    """generate(device_beam_search=True) against the HF path generate(use_customize_greedy=False, num_beams=K, num_return_sequences=K) on
    the same model: equal ids, scores within twice the measured difference of the two routes' scores.  The margin of every decision
    (host_search) is asserted, not assumed, and no prompt is left out."""
    _, model = G._diverge_model()
    V = model.lm_head.weight.shape[0]
    for length, seed in BEAM_PROMPTS[K]:
        p = prompt_ids(length, seed)
        new = HF_NEW[K]
        ids, scores, loop, trace = beam_run(model, p, K, record=True, max_new_tokens=new)
        steps, margin, _ = replay_on_host(trace, K, V, BEAM_EOS, new)
        kw = dict(inputs=p, num_beams=K, num_return_sequences=K, max_new_tokens=new, eos_token_id=list(BEAM_EOS))
        routed, routed_scores = model.generate(device_beam_search=True, output_scores=True, **kw)
        assert [r.tolist() for r in routed] == ids and routed_scores.cpu().numpy().tobytes() == scores.tobytes()
        hf = model.generate(use_customize_greedy=False, do_sample=False, pad_token_id=128001, return_dict_in_generate=True, output_scores=True, **kw)
        hf_ids = [_strip(row.tolist()) for row in hf.sequences]
        hf_scores = hf.sequences_scores.float().cpu().numpy()
        hf_rows = [r.float().cpu().numpy().reshape(K, V) for r in hf.scores]
        hf_steps, hf_margin, _ = host_search(lambda n, state: hf_rows[n], K, V, BEAM_EOS, new)
        diff = score_difference(steps, hf_steps)
        print(f"   K={K} prompt {(length, seed)}: margin {margin:.4f} (on the HF path's rows {hf_margin:.4f}), largest score difference of the "
              f"routes {diff:.5f} over {len(hf_steps)} steps")
        print(f"      ids {ids} hf {hf_ids}\n      scores {scores.tolist()} hf {hf_scores.tolist()}")
        assert margin > 2 * MEASURED_SCORE_DIFF[K], (length, seed, margin)
        assert ids == hf_ids, (length, seed, ids, hf_ids)
        assert diff <= MEASURED_SCORE_DIFF[K], (length, seed, diff)
        assert len(hf_steps) == len(hf_rows) == len(steps)          # both routes stop at the same step
        assert np.abs(scores - hf_scores).max() <= 2 * MEASURED_SCORE_DIFF[K], (scores.tolist(), hf_scores.tolist())


def _quantised(fmt):
    cfg, _ = G._diverge_model()
    from oracle.ref_model import init_state_dict
    sd = init_state_dict(cfg, seed=5)
    rows = [G.START, G.END, G.EOT] + [41 + 9973 * i for i in range(13)]
    W = torch.zeros_like(sd["lm_head.weight"])
    W[rows] = 8.0 * sd["lm_head.weight"][rows]
    sd["lm_head.weight"] = W
    model = G.hip_model(cfg, sd).eval()
    if fmt is not None:
        model.quantize_decoder_(fmt=fmt)
    return model


@pytest.mark.parametrize("what", ["fp8_e4m3 weights", "mxfp4 weights", "fp8_e4m3 cache"])
def test_replay_equals_eager_on_quantised_weights_and_cache(what):
    K = 3
    p = prompt_ids(14, 2)
    if what.endswith("weights"):
        model = _quantised(what.split()[0])
    else:
        _, model = G._diverge_model()
        model.config.mm355_kv_cache_format = "fp8_e4m3"
    try:
        ids, scores, loop, _ = beam_run(model, p, K, graph=True)
        i2, s2, l2, _ = beam_run(model, p, K, graph=False)
    finally:
        if what.endswith("cache"):
            model.config.mm355_kv_cache_format = "bf16"
    assert loop.graphs and not l2.graphs
    assert loop.cache.fmt == ("fp8_e4m3" if what.endswith("cache") else "bf16") and loop.cache.own_block is not None
    assert ids == i2 and scores.tobytes() == s2.tobytes() and np.isfinite(scores).all(), (ids, i2, scores, s2)
    assert all(np.array_equal(l2.final[n], loop.final[n]) for n in ("fin_end", "fin_flag", "fin_score", "running", "tok_log", "parent_log"))
    assert all(1 <= len(i) <= BEAM_NEW for i in ids)


def test_a_left_padded_prompt_is_the_prompt():
    _, model = G._diverge_model()
    K = 2
    p = prompt_ids(*BEAM_PROMPTS[K][0])
    ids, scores, loop, _ = beam_run(model, p, K)
    pad = 5
    padded = torch.cat([torch.zeros((1, pad), dtype=p.dtype, device=DEV), p], 1)
    mask = torch.cat([torch.zeros((1, pad), dtype=torch.long), torch.ones((1, p.shape[1]), dtype=torch.long)], 1).to(DEV)
    i2, s2, l2, _ = beam_run(model, padded, K, mask=mask)
    assert l2.cache.shared_len == p.shape[1] == loop.cache.shared_len                # the padding rows were never cached
    assert i2 == ids and s2.tobytes() == scores.tobytes()
