"""mm355_attn_extend_shared / mm355_attn_extend_shared_f8 on the device: n new query rows per sequence over S shared rows (stored once)
followed by the sequence's own rows [S, past[b] + i], the new rows already appended.  Against the fp32 formula on the CPU at close(1e-2,
1e-2) (the bar of test_attn_extend_gpu.py and test_shared_prefix_gpu.py), every case with the bound at max(past) + n and again at the
capacity, with everything the contract says is never read poisoned with NaN: rows [0, S) of every own block, shared rows >= S, own rows >=
past[b] + n.  On hostile scores against fp64 at 2^-7; the e4m3 form bit for bit against the bf16 form on the dequantised bytes; the same
launch twice gives equal bits; n == 1 equals mm355_attn_decode_shared and S == 0 follows mm355_attn_extend's formula."""
import pytest
import torch

from test_attn_extend_gpu import close, kv8_cache  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def _ragged(B, lo, hi):
    return tuple(lo + (b * 7 + 3) % (hi - lo + 1) for b in range(B))


#        B   n  Hq Hkv  d    S    past - S
CASES = [(1, 1, 2, 1, 128, 1, (0,)),                              # the smallest case
         (3, 5, 8, 2, 128, 70, (0, 0, 0)),                        # 60 packed rows, ragged shared tile
         (3, 20, 8, 2, 128, 200, (0, 3, 17)),                     # two own row tiles per sequence, ragged last shared row tile
         (2, 7, 4, 4, 64, 63, (5, 0)),                            # G = 1
         (5, 3, 8, 1, 40, 65, _ragged(5, 0, 70)),                 # G = 8, d below the padded width
         (2, 4, 8, 2, 128, 1100, (0, 9)),                         # the shared key split
         (4, 6, 4, 2, 96, 0, (1, 2, 0, 30)),                      # no shared rows
         (17, 2, 8, 2, 128, 130, _ragged(17, 0, 90)),             # more than 16 sequences
         # n == 1, the decode-shared case, on each path of the row map
         (3, 1, 4, 4, 64, 63, (0, 1, 63)),                        # G = 1, ragged shared tile
         (5, 1, 8, 1, 40, 65, _ragged(5, 0, 70)),                 # G = 8, d below the padded width
         (4, 1, 4, 2, 96, 0, (1, 2, 0, 30)),                      # d = 96, no shared rows
         (17, 1, 8, 2, 128, 1100, _ragged(17, 0, 90)),            # the shared key split, two row tiles
         (3, 1, 8, 2, 128, 513, (0, 0, 0))]                       # the own part is the one new row
CASE_IDS = [f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{c[4]}-S{c[5]}" for c in CASES]
PAD = 5                                                           # capacity = longest length + PAD


@pytest.fixture(scope="module")
def ops():
    from metamorph_amd import ops as o
    from metamorph_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return o


def formula(q, ksh, vsh, kc, vc, S, past, n, Hq, Hkv, d, dtype=torch.float32):
    """q [B, n, Hq, d], ksh / vsh [>= S, Hkv, d], kc / vc [B, rows, Hkv, d] -> [B * n, Hq * d]: row (b, i) over the shared rows [0, S)
    followed by rows [S, past[b] + i] of block b"""
    B, G = q.shape[0], Hq // Hkv
    out = torch.empty(B, n, Hq * d, dtype=dtype)
    for b in range(B):
        m = past[b] + n
        kk = torch.cat([ksh[:S], kc[b, S:m]]).to(dtype).transpose(0, 1).repeat_interleave(G, dim=0)       # [Hq, m, d]
        vv = torch.cat([vsh[:S], vc[b, S:m]]).to(dtype).transpose(0, 1).repeat_interleave(G, dim=0)
        s = (q[b].to(dtype).transpose(0, 1) @ kk.transpose(1, 2)) * d ** -0.5                             # [Hq, n, m]
        keys, rows = torch.arange(m)[None, None, :], (past[b] + torch.arange(n))[None, :, None]
        s = s.masked_fill(keys > rows, float("-inf"))
        out[b] = (torch.softmax(s, dim=-1) @ vv).transpose(0, 1).reshape(n, Hq * d)
    return out.view(B * n, Hq * d)


def poison(ksh, vsh, kc, vc, S, ends, value=float("nan")):
    for t in (ksh, vsh):
        t[S:] = value
    for t in (kc, vc):
        t[:, :S] = value
        for b, m in enumerate(ends):
            t[b, m:] = value


_INPUTS = {}


def inputs(case):
    """(q, ksh, vsh, kc, vc, past, reference) of a case on the CPU, made once and shared by the tests that need them"""
    if case not in _INPUTS:
        B, n, Hq, Hkv, d, S, own = case
        past = [S + x for x in own]
        rows = max(past) + n + PAD
        g = torch.Generator().manual_seed(7 + S + sum(own) + n)
        q = (torch.randn(B, n, Hq, d, generator=g) * 0.7).bfloat16()
        ksh = (torch.randn(S + 3, Hkv, d, generator=g) * 0.7).bfloat16()
        vsh = (torch.randn(S + 3, Hkv, d, generator=g) * 0.7).bfloat16()
        kc = (torch.randn(B, rows, Hkv, d, generator=g) * 0.7).bfloat16()
        vc = (torch.randn(B, rows, Hkv, d, generator=g) * 0.7).bfloat16()
        ref = formula(q, ksh, vsh, kc, vc, S, past, n, Hq, Hkv, d)
        poison(ksh, vsh, kc, vc, S, [p + n for p in past])
        _INPUTS[case] = (q, ksh, vsh, kc, vc, past, ref)
    return _INPUTS[case]


def _ws(ops, B, n, Hq, Hkv, d, S, bound):
    m = int(ops._L().mm355_attn_extend_shared_ws_floats(B, n, Hq, Hkv, d, S, bound))
    assert m > 0
    return torch.full((m,), float("nan"), device=DEV, dtype=torch.float32)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_attn_extend_shared_against_the_formula(ops, case):
    B, n, Hq, Hkv, d, S, own = case
    q, ksh, vsh, kc, vc, past, ref = inputs(case)
    rows = kc.shape[1]
    pd = torch.tensor(past, dtype=torch.int32, device=DEV)
    kd, vd = kc.view(B, rows, Hkv * d).to(DEV), vc.view(B, rows, Hkv * d).to(DEV)
    ks, vs = ksh.view(-1, Hkv * d).to(DEV), vsh.view(-1, Hkv * d).to(DEV)
    qd = q.view(B * n, Hq * d).to(DEV)
    sc = d ** -0.5
    tight = max(past) + n
    got = ops.attn_extend_shared(qd, ks, vs, kd, vd, pd, n, S, tight, Hq, Hkv, d, sc)
    close(got, ref, 1e-2, 1e-2, f"attn_extend_shared {case}")
    assert torch.equal(ops.attn_extend_shared(qd, ks, vs, kd, vd, pd, n, S, tight, Hq, Hkv, d, sc), got)        # the same launch twice
    # the capacity as the bound, over a workspace that starts as NaN: the poisoned tails are still never read, the bits are the same
    ws = _ws(ops, B, n, Hq, Hkv, d, S, rows)
    cap = ops.attn_extend_shared(qd, ks, vs, kd, vd, pd, n, S, rows, Hq, Hkv, d, sc, workspace=ws)
    close(cap, ref, 1e-2, 1e-2, f"attn_extend_shared {case}, bound = capacity")
    assert torch.equal(cap, got) and torch.equal(ops.attn_extend_shared(qd, ks, vs, kd, vd, pd, n, S, rows, Hq, Hkv, d, sc, workspace=ws), cap)
    # q and o as column views of a wider tensor (the q block of a fused q|k|v activation; an output block)
    wide_q = torch.full((B * n, Hq * d + 2 * Hkv * d), float("nan"), device=DEV, dtype=BF16)
    wide_q[:, :Hq * d] = qd
    wide_o = torch.zeros((B * n, Hq * d + 64), device=DEV, dtype=BF16)
    o_view = wide_o[:, 64:]
    ret = ops.attn_extend_shared(wide_q[:, :Hq * d], ks, vs, kd, vd, pd, n, S, tight, Hq, Hkv, d, sc, out=o_view)
    assert ret.data_ptr() == o_view.data_ptr() and torch.equal(o_view, got) and float(wide_o[:, :64].float().abs().max()) == 0
    if n == 1:                                                    # the decode-shared case, bit for bit
        lens = torch.tensor([p + 1 for p in past], dtype=torch.int32, device=DEV)
        assert torch.equal(ops.attn_decode_shared(qd, ks, vs, kd, vd, lens, S, tight, Hq, Hkv, d, sc), got)


@pytest.mark.parametrize("kind", ["sink", "own_cliff", "shared_cliff"])
def test_attn_extend_shared_on_hostile_scores(ops, kind):
    """The construction of test_attn_decode_shared_on_hostile_scores against fp64 at 2^-7, with n = 12 rows per sequence: a sink at shared
    key 0 (+40 over a flat rest); a cliff where every score sits at -40 except, for row (b, i), own key past[b] + i - 7 at +40 (the key 7
    before each row's own position; rows whose cliff key would lie before the own rows see a flat -40), so the own partial and the shared
    partials differ by about 115 log2 units at the merge; and the mirror image, the +40 key inside the shared rows."""
    B, n, Hq, Hkv, d, S = 4, 12, 32, 8, 128, 2500
    own = [0, 3, 40, 70]
    past = [S + x for x in own]
    rows = max(past) + n + 3
    g = torch.Generator().manual_seed(11)
    q = (torch.randn(B, n, Hq, d, generator=g) * 0.5).bfloat16()
    ksh = (torch.randn(S + 2, Hkv, d, generator=g) * 0.5).bfloat16()
    kc = (torch.randn(B, rows, Hkv, d, generator=g) * 0.5).bfloat16()
    vsh = torch.randn(S + 2, Hkv, d, generator=g).bfloat16()
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
                for i in range(n):
                    if past[b] + i - 7 >= S:
                        kc[b, past[b] + i - 7, :, 0] = 40.0 / unit
        else:
            ksh[S - 700, :, 0] = 40.0 / unit
    ref = formula(q, ksh, vsh, kc, vc, S, past, n, Hq, Hkv, d, dtype=torch.float64)
    poison(ksh, vsh, kc, vc, S, [p + n for p in past])
    got = ops.attn_extend_shared(q.view(B * n, Hq * d).to(DEV), ksh.view(-1, Hkv * d).to(DEV), vsh.view(-1, Hkv * d).to(DEV),
                                 kc.view(B, rows, Hkv * d).to(DEV), vc.view(B, rows, Hkv * d).to(DEV),
                                 torch.tensor(past, dtype=torch.int32, device=DEV), n, S, max(past) + n, Hq, Hkv, d, d ** -0.5)
    close(got, ref, 2.0 ** -7, 2.0 ** -7, f"attn_extend_shared {kind}")


@pytest.mark.parametrize("case", [CASES[i] for i in (2, 4, 5, 6, 9, 11)], ids=[CASE_IDS[i] for i in (2, 4, 5, 6, 9, 11)])
def test_attn_extend_shared_f8_equals_the_bf16_form_on_the_dequantised_cache(ops, case):
    B, n, Hq, Hkv, d, S, own = case
    past = [S + x for x in own]
    ends = [p + n for p in past]
    rows = max(ends) + PAD
    k8, ks, v8, vs = kv8_cache(B, rows, Hkv, d, seed=S + d + sum(own))
    s8 = kv8_cache(1, S + 3, Hkv, d, seed=S + d + sum(own) + 1)
    ksh8, kshs, vsh8, vshs = (t[0] for t in s8)
    deq = lambda t8, ts: ops.dequant_kv8(t8, ts, Hkv, d)           # (before anything is poisoned)
    kb, vb, kshb, vshb = deq(k8, ks), deq(v8, vs), deq(ksh8, kshs), deq(vsh8, vshs)
    poison(ksh8, vsh8, k8, v8, S, ends, value=0x7F)                # what is never read: the NaN byte and a NaN scale
    poison(kshs, vshs, ks, vs, S, ends)
    poison(kshb, vshb, kb, vb, S, ends)
    q = (torch.randn(B * n, Hq * d, generator=torch.Generator().manual_seed(5)) * 0.7).bfloat16().to(DEV)
    pd = torch.tensor(past, dtype=torch.int32, device=DEV)
    D = lambda *ts: [t.to(DEV) for t in ts]
    for bound in (max(ends), rows):
        ref = ops.attn_extend_shared(q, *D(kshb, vshb, kb, vb), pd, n, S, bound, Hq, Hkv, d, d ** -0.5)
        got = ops.attn_extend_shared_f8(q, *D(ksh8, vsh8, kshs, vshs, k8, v8, ks, vs), pd, n, S, bound, Hq, Hkv, d, d ** -0.5)
        assert bool(torch.isfinite(got.float()).all()) and torch.equal(got, ref), (case, bound)
        assert torch.equal(ops.attn_extend_shared_f8(q, *D(ksh8, vsh8, kshs, vshs, k8, v8, ks, vs), pd, n, S, bound, Hq, Hkv, d, d ** -0.5), got)
        if n == 1:                                                # the decode-shared case on the same bytes, bit for bit
            lens = torch.tensor(ends, dtype=torch.int32, device=DEV)
            assert torch.equal(ops.attn_decode_shared_f8(q, *D(ksh8, vsh8, kshs, vshs, k8, v8, ks, vs), lens, S, bound, Hq, Hkv, d, d ** -0.5), got)


def test_no_shared_rows_is_the_extend_case(ops):
    """shared_len == 0 against mm355_attn_extend on the same cache: the same formula, another key split, so close and not equal"""
    case = CASES[6]
    B, n, Hq, Hkv, d, S, own = case
    q, ksh, vsh, kc, vc, past, ref = inputs(case)
    rows = kc.shape[1]
    pd = torch.tensor(past, dtype=torch.int32, device=DEV)
    kd, vd = kc.view(B, rows, Hkv * d).to(DEV), vc.view(B, rows, Hkv * d).to(DEV)
    qd = q.view(B * n, Hq * d).to(DEV)
    ext = ops.attn_extend(qd, kd, vd, pd, n, max(past) + n, Hq, Hkv, d, d ** -0.5)
    got = ops.attn_extend_shared(qd, ksh.view(-1, Hkv * d).to(DEV), vsh.view(-1, Hkv * d).to(DEV), kd, vd, pd, n, 0, max(past) + n, Hq, Hkv, d,
                                 d ** -0.5)
    close(got, ext.float(), 1e-2, 1e-2, "attn_extend_shared with no shared rows against attn_extend")
