"""The KV-cache kernels at the length the product is built for (LLaMA-3.1: 131072 positions) and on caches laid out beyond 4 GiB.

  1. attn_decode (variants 0, 1, 2) and attn_decode_f8 over a bound of 131072 rows: 128 key groups (variant 1: 512 chunks) folded by the
     last arriver, sequences of 131072, 100003, 700 and 0 rows under that bound;
  2. attn_extend, attn_extend_f8 and attn_extend_ragged with 64 key runs of 32 tiles and the merge over 64 partials;
  3. attn_decode_shared / attn_extend_shared over a shared prefix of 131008 rows;
  4. every reader and writer of the cache on K / V views whose last sequence starts more than 2^31 elements (4 GiB) behind the first;
  5. the RoPE tables up to row 131071.

The inputs, the fp64 formula and the threshold |got - ref| <= 2^-7 |ref| + 2^-20 are those of tests/kv_long_refs.py (why they can tell right
from wrong at this length: tests/test_kv_long_refs_host.py).  Run with -s: every comparison prints its measured largest relative error."""
import os

import numpy as np
import pytest
import torch

import kv_long_refs as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
LONG = 131072


@pytest.fixture(scope="module")
def ops():
    from metamorph_amd import ops as o
    from metamorph_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    yield o
    _INPUTS.clear()
    _FAR.clear()
    torch.cuda.empty_cache()


_INPUTS = {}


def made_once(key, make):
    if key not in _INPUTS:
        _INPUTS[key] = make()
    return _INPUTS[key]


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def quantised(k, v, Hkv, d, lens, seed):
    """the e4m3 cache of k / v (kv_long_refs.quantize_rows_kv8), its dequantised bf16 rows, and the device operands with the rows from
    lens[b] on poisoned (the NaN byte and a NaN scale)"""
    from metamorph_amd import ops
    k8, ks = K.quantize_rows_kv8(k, Hkv, d, seed)
    v8, vs = K.quantize_rows_kv8(v, Hkv, d, seed + 1)
    kb, vb = ops.dequant_kv8(k8, ks, Hkv, d), ops.dequant_kv8(v8, vs, Hkv, d)
    for b, L in enumerate(lens):
        for t8, ts in ((k8, ks), (v8, vs)):
            t8[b, L:] = 0x7F
            ts[b, L:] = float("nan")
    return kb, vb, tuple(t.to(DEV) for t in (k8, v8, ks, vs))


# ------------------------------------------------------------------------------------------------ 1. decode at 131072 rows

DEC_LENS = [LONG, 100003, 700, 0]
#            Hq Hkv  d
DEC_CASES = [(8, 1, 128), (4, 1, 128), (1, 1, 64), (8, 1, 72)]


def decode_case(kind, Hq, Hkv, d):
    """host inputs (rows beyond a sequence poisoned), device caches, and per channel shift (q on the device, fp64 reference)"""
    def make():
        runs = []
        for shift in (range(0, K.NCH, Hq) if kind == "needle" else (0,)):        # fewer than 8 heads: every needle still gets a head
            q, k, v = K.decode_inputs(kind, DEC_LENS, LONG, Hq, Hkv, d, shift=shift)
            runs.append((shift, q.to(DEV), K.decode_ref(q, k, v, DEC_LENS, Hq, Hkv, d)))
        K.poison_(DEC_LENS, k, v)
        return k, v, k.to(DEV), v.to(DEV), runs
    return made_once(("decode", kind, Hq, Hkv, d), make)


@pytest.mark.parametrize("kind", ["flat", "needle"])
@pytest.mark.parametrize("case", DEC_CASES, ids=["-".join(map(str, c)) for c in DEC_CASES])
def test_attn_decode_under_a_bound_of_131072_rows(ops, case, kind):
    """Variants 0, 1 and 2 against fp64 over 128 key groups (variant 1: 512 chunks) per query head: a full cache, 100003 rows (ragged last
    group and chunk), 700 rows (one live group whose workgroup writes the row itself while 127 others leave) and an empty sequence (a zero
    row).  Variant 2 equals variant 0 bit for bit; a second launch on the same workspace gives the same bits and the arrival counters are
    back at zero."""
    Hq, Hkv, d = case
    B = len(DEC_LENS)
    _, _, kd, vd, runs = decode_case(kind, Hq, Hkv, d)
    lens = i32(DEC_LENS)
    n_ws = int(ops._L().mm355_attn_decode_ws_floats(B, Hq, d, LONG))
    assert n_ws == ((B * Hq + 3) & ~3) + B * Hq * (LONG // 256) * (d + 2)         # 512 chunk records (variant 1); 128 group records
    for shift, q, ref in runs:
        outs = {}
        for variant in (0, 1, 2):
            ws = torch.zeros(n_ws, device=DEV, dtype=torch.float32)
            out = ops.attn_decode(q, kd, vd, lens, LONG, Hq, Hkv, d, d ** -0.5, workspace=ws, variant=variant).clone()
            K.accept(out, ref, f"attn_decode v{variant} {kind} Hq={Hq} d={d} shift={shift} at {LONG} keys")
            again = ops.attn_decode(q, kd, vd, lens, LONG, Hq, Hkv, d, d ** -0.5, workspace=ws, variant=variant)
            assert torch.equal(again, out), ("second launch on the same workspace", variant)
            assert int(ws[:B * Hq].view(torch.int32).abs().max()) == 0, ("arrival counters", variant)
            assert float(out[3].float().abs().max()) == 0, ("empty sequence", variant)
            outs[variant] = out
        assert torch.equal(outs[2], outs[0])
        if kind == "needle":
            for b, L in enumerate(DEC_LENS[:3]):
                want = K.decode_needle_keys(L)
                assert [K.spelled(outs[0][b].float().cpu().view(Hq, d)[h], d) for h in range(Hq)] == [want[(h + shift) % K.NCH] for h in range(Hq)]


@pytest.mark.parametrize("kind", ["flat", "needle"])
@pytest.mark.parametrize("case", [DEC_CASES[0], DEC_CASES[3]], ids=["8-1-128", "8-1-72"])
def test_attn_decode_f8_under_a_bound_of_131072_rows(ops, case, kind):
    """The same caches quantised (a power-of-two scale per key and head): bit for bit the bf16 form on the dequantised cache, and fp64 of the
    dequantised values, variants 0 and 2."""
    Hq, Hkv, d = case
    q, k, v = K.decode_inputs(kind, DEC_LENS, LONG, Hq, Hkv, d)
    kb, vb, c8 = quantised(k, v, Hkv, d, DEC_LENS, seed=d)
    ref = K.decode_ref(q, kb, vb, DEC_LENS, Hq, Hkv, d)
    K.poison_(DEC_LENS, kb, vb)
    qd, lens, kbd, vbd = q.to(DEV), i32(DEC_LENS), kb.to(DEV), vb.to(DEV)
    for variant in (0, 2):
        got = ops.attn_decode_f8(qd, *c8, lens, LONG, Hq, Hkv, d, d ** -0.5, variant=variant)
        K.accept(got, ref, f"attn_decode_f8 v{variant} {kind} d={d} at {LONG} keys")
        assert torch.equal(got, ops.attn_decode(qd, kbd, vbd, lens, LONG, Hq, Hkv, d, d ** -0.5, variant=variant)), variant


# ------------------------------------------------------------------------------------------------ 2. extend with 64 key runs

#          B  Hq Hkv  d    past              n   bound
X_CASES = [(1, 4, 1, 128, (LONG - 17,), 17, LONG),
           (2, 4, 1, 128, (100003, 65519), 33, 100003 + 33)]
X_IDS = ["131055+17", "100003_65519+33"]
X_KINDS = ["flat", "needle", "beyond"]


def lib_extend_nsplit(ops, B, n, Hq, Hkv, d, bound):
    """the library's nsplit, from mm355_attn_extend_ws_floats = B Hkv nsplit rpad (DP + 2)"""
    nqt = (n * (Hq // Hkv) + 63) // 64
    ws = int(ops._L().mm355_attn_extend_ws_floats(B, n, Hq, Hkv, d, bound))
    per = B * Hkv * nqt * 64 * (K.pick_dp(d) + 2)
    assert ws % per == 0
    return ws // per if ws else 1


def extend_case(ops, case, kind):
    def make():
        B, Hq, Hkv, d, past, n, bound = case
        nsplit, tps, _ = K.extend_runs(B, n, Hq, Hkv, bound)
        q, k, v = K.extend_inputs(kind, list(past), n, bound + 8, Hq, Hkv, d, (nsplit, tps))
        ref = K.extend_ref(q, k, v, past, n, Hq, Hkv, d)
        return q, k, v, ref
    return made_once(("extend", case, kind), make)


@pytest.mark.parametrize("case", X_CASES, ids=X_IDS)
def test_the_restated_key_runs_are_the_librarys(ops, case):
    """kv_long_refs.key_runs places the needles on the run edges: it must be the library's rule.  131072 keys under two row tiles: the cap of
    64 runs, 32 tiles each."""
    B, Hq, Hkv, d, past, n, bound = case
    nsplit, tps, nqt = K.extend_runs(B, n, Hq, Hkv, bound)
    assert lib_extend_nsplit(ops, B, n, Hq, Hkv, d, bound) == nsplit
    assert (nsplit, tps, nqt) == ((64, 32, 2) if bound == LONG else (43, 37, 3))


@pytest.mark.parametrize("kind", X_KINDS)
@pytest.mark.parametrize("case", X_CASES, ids=X_IDS)
def test_attn_extend_with_long_key_runs(ops, case, kind):
    """attn_extend against fp64 and attn_extend_f8 bit for bit against it on the dequantised cache (and against fp64 of those values); the
    cache rows from past + n on are NaN.  With two sequences the ragged form with a uniform table gives attn_extend's bits."""
    B, Hq, Hkv, d, past, n, bound = case
    q, k, v, ref = extend_case(ops, case, kind)
    lens = [p + n for p in past]
    kp, vp = k.clone(), v.clone()
    K.poison_(lens, kp, vp)
    qd, pd = q.to(DEV), i32(past)
    got = ops.attn_extend(qd, kp.to(DEV), vp.to(DEV), pd, n, bound, Hq, Hkv, d, d ** -0.5)
    K.accept(got, ref, f"attn_extend {kind} past={past} n={n}")
    if kind != "flat":
        out = got.float().cpu().view(B, n, Hq, d)
        for b, p in enumerate(past):                          # rows 1 .. 5 and 7: one visible needle each, at a known key
            want = K.extend_needle_keys(p, n, *K.extend_runs(B, n, Hq, Hkv, bound)[:2]) if kind == "needle" else None
            for i in (1, 2, 3, 4, 5, 7):
                key = want[i] if want else p + i
                if key <= p + i:                              # (a run edge beyond a short sequence was moved to its last row)
                    assert K.spelled(out[b, i, 0], d) == key, (kind, b, i)
    if B > 1:
        rs = i32(range(0, B * n + 1, n))
        assert torch.equal(ops.attn_extend_ragged(qd, kp.to(DEV), vp.to(DEV), pd, rs, n, bound, Hq, Hkv, d, d ** -0.5), got)
    kb, vb, c8 = quantised(k, v, Hkv, d, lens, seed=n)
    ref8 = K.extend_ref(q, kb, vb, past, n, Hq, Hkv, d)
    K.poison_(lens, kb, vb)
    got8 = ops.attn_extend_f8(qd, *c8, pd, n, bound, Hq, Hkv, d, d ** -0.5)
    K.accept(got8, ref8, f"attn_extend_f8 {kind} past={past} n={n}")
    assert torch.equal(got8, ops.attn_extend(qd, kb.to(DEV), vb.to(DEV), pd, n, bound, Hq, Hkv, d, d ** -0.5))


@pytest.mark.parametrize("kind", X_KINDS)
def test_attn_extend_ragged_with_long_key_runs(ops, kind):
    """A ragged table (5 and 33 rows) over the caches of the two-sequence case, against fp64: the launch plan is that of n_max = 33."""
    B, Hq, Hkv, d, past, n, bound = X_CASES[1]
    q, k, v, _ = extend_case(ops, X_CASES[1], kind)
    ns = [5, 33]
    qr = torch.cat([q[:5], q[n:2 * n]])
    ref = K.extend_ref(qr, k, v, past, ns, Hq, Hkv, d)
    kp, vp = k.clone(), v.clone()
    K.poison_([p + m for p, m in zip(past, ns)], kp, vp)
    got = ops.attn_extend_ragged(qr.to(DEV), kp.to(DEV), vp.to(DEV), i32(past), i32([0, 5, 38]), n, bound, Hq, Hkv, d, d ** -0.5)
    K.accept(got, ref, f"attn_extend_ragged {kind} rows={ns}")


# ------------------------------------------------------------------------------------------------ 3. a shared prefix of 131008 rows

S_LEN = LONG - 64
S_OWN = (3, 40, 0)


def shared_case(ops, form, kind):
    """form "decode": one row per sequence, kv_lens = S_LEN + own; "extend": 5 new rows behind S_LEN + own cached ones"""
    def make():
        Hq, n = (8, 1) if form == "decode" else (4, 5)
        B, Hkv, d = len(S_OWN), 1, 128
        past = [S_LEN + o - (1 if form == "decode" else 0) for o in S_OWN]
        nsplit, tps, nqt = K.shared_runs(B, n, Hq, Hkv, S_LEN)
        fn = "mm355_attn_decode_shared_ws_floats" if form == "decode" else "mm355_attn_extend_shared_ws_floats"
        ws = int(getattr(ops._L(), fn)(B, *(() if form == "decode" else (n,)), Hq, Hkv, d, S_LEN, LONG))
        assert ws == Hkv * (nsplit + 1) * nqt * 64 * (K.pick_dp(d) + 2) and (nsplit, tps) == (64, 32)
        q, ksh, vsh, k, v = K.shared_inputs(kind, S_LEN, past, n, LONG, Hq, Hkv, d, (nsplit, tps))
        ref = K.extend_ref(q, k, v, past, n, Hq, Hkv, d, shared=(ksh, vsh, S_LEN))
        K.poison_([p + n for p in past], k, v)
        return Hq, Hkv, d, n, past, q, ref, [t.to(DEV) for t in (q, ksh, vsh, k, v)]
    return made_once(("shared", form, kind), make)


@pytest.mark.parametrize("kind", ["flat", "needle"])
@pytest.mark.parametrize("form", ["decode", "extend"])
def test_shared_prefix_attention_over_a_long_prefix(ops, form, kind):
    """attn_decode_shared and attn_extend_shared against fp64: 64 runs of 32 tiles over the shared rows and the merge over 65 partials;
    own rows of 3, 40 and 0 cached rows; needles on the run edges, on the last shared row, on the first and the last own row."""
    Hq, Hkv, d, n, past, q, ref, (qd, ksh, vsh, k, v) = shared_case(ops, form, kind)
    if form == "decode":
        got = ops.attn_decode_shared(qd, ksh, vsh, k, v, i32([p + 1 for p in past]), S_LEN, LONG, Hq, Hkv, d, d ** -0.5)
    else:
        got = ops.attn_extend_shared(qd, ksh, vsh, k, v, i32(past), n, S_LEN, LONG, Hq, Hkv, d, d ** -0.5)
    K.accept(got, ref, f"attn_{form}_shared {kind} prefix={S_LEN} own={S_OWN}")
    if kind == "needle":
        pos = K.shared_needle_keys(S_LEN, S_LEN - 1, 64, 32)
        out = got.float().cpu().view(len(past) * n, Hq, d)
        for r in range(out.shape[0]):
            b = r // n
            last = past[b] + n - 1
            for h in range(Hq):
                c = (3 * r + h) % K.NCH
                want = pos[c] if c not in (5, 6) else (None if last < S_LEN else (S_LEN if c == 5 else last))
                if want is not None and (c != 6 or r % n == n - 1):              # (the last own row is visible to the last query row only)
                    assert K.spelled(out[r, h], d) == want, (form, r, h, c)


# ------------------------------------------------------------------------------------------------ 4. caches beyond 4 GiB

_FAR = {}
F_HKV, F_D, F_ROWS, GUARD = 2, 128, 1100, 64
F_LD = 2 * F_HKV * F_D                                        # K and V interleaved in one row: V = K + Hkv d columns


def far_alloc(dtype):
    """one allocation of 2^31 + 2^27 elements (bf16: 4.25 GiB) or 2^32 + 2^28 bytes, never initialised as a whole"""
    if dtype not in _FAR:
        n = (1 << 31) + (1 << 27) if dtype == BF16 else (1 << 32) + (1 << 28)
        _FAR[dtype] = torch.empty(n, device=DEV, dtype=dtype)
    return _FAR[dtype]


class FarCache:
    """B sequences of F_ROWS rows as K / V views [B, F_ROWS, Hkv d] of one huge allocation: sequence 0 starts at element 0, the last one
    beyond 2^31 elements (bf16) / 2^32 bytes (e4m3).  Only the rows and a guard band of 64 rows around each sequence are ever touched: the
    guard is NaN / the NaN byte, and `unchanged_outside` holds it (and the first elements of the allocation) to its bits."""

    def __init__(self, B, dtype, fill):
        self.buf, self.B, self.dtype = far_alloc(dtype), B, dtype
        far = ((1 << 31) + (1 << 26)) * (1 if dtype == BF16 else 2)
        self.bs = -(-far // (B - 1) // 16) * 16
        W = F_HKV * F_D
        assert (B - 1) * self.bs > (1 << 31) * (1 if dtype == BF16 else 2) and self.region(B - 1)[1] <= self.buf.numel()
        assert self.region(0)[1] < self.region(1)[0]
        for b in range(B):
            lo, hi = self.region(b)
            self.buf[lo:hi] = float("nan") if dtype == BF16 else 0x7F
        self.k = self.buf.as_strided((B, F_ROWS, W), (self.bs, F_LD, 1))
        self.v = self.buf[W:].as_strided((B, F_ROWS, W), (self.bs, F_LD, 1))
        self.k.copy_(fill[0])
        self.v.copy_(fill[1])
        self.before = [self.buf[slice(*self.region(b))].clone() for b in range(B)]

    def region(self, b):
        """[lo, hi) of the allocation: sequence b's rows and the guard rows around them"""
        return max(0, b * self.bs - GUARD * F_LD), b * self.bs + (F_ROWS + GUARD) * F_LD

    def compact(self):
        return self.k.contiguous(), self.v.contiguous()

    def unchanged_outside(self, kc, vc):
        """every touched byte of the allocation is what it was, except that the K / V rows now equal the compact caches kc / vc (which went
        through the same call)"""
        W = F_HKV * F_D
        for b in range(self.B):
            lo, hi = self.region(b)
            want = self.before[b].clone()
            off = b * self.bs - lo
            want[off:].as_strided((F_ROWS, W), (F_LD, 1)).copy_(kc[b])
            want[off + W:].as_strided((F_ROWS, W), (F_LD, 1)).copy_(vc[b])
            now = self.buf[lo:hi]
            same = now.view(torch.int16) == want.view(torch.int16) if self.dtype == BF16 else now == want
            assert bool(same.all()), (b, int((~same).sum()))


def rnd(*shape, seed, scale=0.7):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).bfloat16()


def far_rows(B, seed=40):
    W = F_HKV * F_D
    return rnd(B, F_ROWS, W, seed=seed).to(DEV), rnd(B, F_ROWS, W, seed=seed + 1).to(DEV)


def test_cache_readers_beyond_4_gib(ops):
    """Every bf16 reader on far views equals itself on a compact copy of the same rows, bit for bit (the launch plan depends on the
    arguments, not on the strides): attn_decode (variant 0 with a bound <= 1024: one group, no records, and > 1024: records and the merge;
    variant 1), attn_extend, attn_extend_ragged, attn_decode_shared with and without an own-block table that names the far block, and
    attn_extend_shared.  The address arithmetic of all of them was read first: every product of a sequence, block or row index with a stride
    is 64-bit (attn_decode.hip, attn_tile.h load_tile / load_tile_idx, attn_extend.hip, attn_extend_shared.hip)."""
    B, Hq, Hkv, d = 2, 8, F_HKV, F_D
    far = FarCache(B, BF16, far_rows(B))
    assert far.k.stride(0) * 2 > 1 << 32 and far.k[1].data_ptr() - far.buf.data_ptr() > 1 << 32
    kc, vc = far.compact()
    sc = d ** -0.5
    q = rnd(B, Hq * d, seed=1).to(DEV)
    for variant, lens, bound in ((0, [700, 1000], 1024), (0, [1100, 1090], F_ROWS), (1, [1100, 1090], F_ROWS), (2, [300, 1100], F_ROWS)):
        a = ops.attn_decode(q, far.k, far.v, i32(lens), bound, Hq, Hkv, d, sc, variant=variant)
        assert torch.equal(a, ops.attn_decode(q, kc, vc, i32(lens), bound, Hq, Hkv, d, sc, variant=variant)), (variant, bound)
        assert bool(torch.isfinite(a.float()).all()) and float(a.float().abs().max()) > 0
    n, past = 40, i32([1000, 1050])
    qx = rnd(B * n, Hq * d, seed=2).to(DEV)
    assert int(ops._L().mm355_attn_extend_ws_floats(B, n, Hq, Hkv, d, F_ROWS)) > 0                 # (the key split and its merge launch)
    a = ops.attn_extend(qx, far.k, far.v, past, n, F_ROWS, Hq, Hkv, d, sc)
    assert torch.equal(a, ops.attn_extend(qx, kc, vc, past, n, F_ROWS, Hq, Hkv, d, sc)) and bool(torch.isfinite(a.float()).all())
    rs = i32([0, 5, 45])
    a = ops.attn_extend_ragged(qx[:45], far.k, far.v, past, rs, n, F_ROWS, Hq, Hkv, d, sc)
    assert torch.equal(a, ops.attn_extend_ragged(qx[:45], kc, vc, past, rs, n, F_ROWS, Hq, Hkv, d, sc)) and bool(torch.isfinite(a.float()).all())
    S = 256
    ksh, vsh = rnd(S, Hkv * d, seed=3).to(DEV), rnd(S, Hkv * d, seed=4).to(DEV)
    lens = i32([700, 1100])
    tbl = torch.ones(B, F_ROWS - S, dtype=torch.uint8)
    tbl[1, ::2] = 0                                           # sequence 0: every own row from the far block; sequence 1: every other one
    for own_block in (None, tbl.to(DEV)):
        a = ops.attn_decode_shared(q, ksh, vsh, far.k, far.v, lens, S, F_ROWS, Hq, Hkv, d, sc, own_block=own_block)
        assert torch.equal(a, ops.attn_decode_shared(q, ksh, vsh, kc, vc, lens, S, F_ROWS, Hq, Hkv, d, sc, own_block=own_block))
        assert bool(torch.isfinite(a.float()).all())
    a = ops.attn_extend_shared(qx, ksh, vsh, far.k, far.v, past, n, S, F_ROWS, Hq, Hkv, d, sc)
    assert torch.equal(a, ops.attn_extend_shared(qx, ksh, vsh, kc, vc, past, n, S, F_ROWS, Hq, Hkv, d, sc)) and bool(torch.isfinite(a.float()).all())
    far.unchanged_outside(kc, vc)


def far_f8(ops, B, seed=50):
    """an e4m3 far cache of B sequences with compact scales [B, F_ROWS, Hkv], and the compact copies"""
    k8, ks = ops.quantize_kv8(rnd(B, F_ROWS, F_HKV * F_D, seed=seed), F_HKV, F_D)
    v8, vs = ops.quantize_kv8(rnd(B, F_ROWS, F_HKV * F_D, seed=seed + 1), F_HKV, F_D)
    return FarCache(B, torch.uint8, (k8.to(DEV), v8.to(DEV))), ks.to(DEV), vs.to(DEV)


def test_f8_cache_readers_beyond_4_gib(ops):
    """attn_decode_f8 (both plans) and attn_extend_f8 on e4m3 views whose last sequence starts beyond 2^32 bytes, scales compact: equal to
    themselves on a compact copy of the bytes."""
    B, Hq, Hkv, d = 2, 8, F_HKV, F_D
    far, ks, vs = far_f8(ops, B)
    assert far.k[1].data_ptr() - far.buf.data_ptr() > 1 << 32
    kc, vc = far.compact()
    sc = d ** -0.5
    q = rnd(B, Hq * d, seed=1).to(DEV)
    for lens, bound in (([700, 1000], 1024), ([1100, 1090], F_ROWS)):
        a = ops.attn_decode_f8(q, far.k, far.v, ks, vs, i32(lens), bound, Hq, Hkv, d, sc)
        assert torch.equal(a, ops.attn_decode_f8(q, kc, vc, ks, vs, i32(lens), bound, Hq, Hkv, d, sc)) and bool(torch.isfinite(a.float()).all())
    n, past = 40, i32([1000, 1050])
    qx = rnd(B * n, Hq * d, seed=2).to(DEV)
    a = ops.attn_extend_f8(qx, far.k, far.v, ks, vs, past, n, F_ROWS, Hq, Hkv, d, sc)
    assert torch.equal(a, ops.attn_extend_f8(qx, kc, vc, ks, vs, past, n, F_ROWS, Hq, Hkv, d, sc)) and bool(torch.isfinite(a.float()).all())
    far.unchanged_outside(kc, vc)


def rope(ops, rows=F_ROWS):
    return made_once(("rope", rows), lambda: ops.rope_table(rows, F_D, 500000.0, DEV))


@pytest.mark.parametrize("writer", ["rope_kv_append_", "rope_kv_append_rows_", "gemv_rope_append", "gemm_splitk_rope_append"])
def test_cache_writers_beyond_4_gib(ops, writer):
    """The bf16 writers on far views: the rows they write equal the rows the same call writes into a compact cache, and every other touched
    element of the allocation (the other rows, the guard bands, the first elements of the allocation) keeps its bits.  Positions include the
    last row of the far block.  Their address arithmetic was read first: b * bs_kv + pos * ld_kv is 64-bit in decode.hip's append kernels,
    decode_gemv.h's fused store and gemm_bf16.hip's split-K reduce."""
    Hq, Hkv, d = 4, F_HKV, F_D
    N, Kd = (Hq + 2 * Hkv) * d, 512
    cos, sin = rope(ops)
    B = {"rope_kv_append_": 2, "rope_kv_append_rows_": 2, "gemv_rope_append": 3, "gemm_splitk_rope_append": 24}[writer]
    fill = far_rows(B)
    far = FarCache(B, BF16, fill)
    kc, vc = far.compact()
    pos = [9 + 37 * b for b in range(B)]
    pos[-1] = F_ROWS - 1

    def call(k, v):
        if writer == "rope_kv_append_":
            return ops.rope_kv_append_(rnd(B, N, seed=5).to(DEV), Hq, Hkv, d, cos, sin, i32(pos), k, v)
        if writer == "rope_kv_append_rows_":
            return ops.rope_kv_append_rows_(rnd(5, N, seed=5).to(DEV), Hq, Hkv, d, cos, sin, i32([9, 700, F_ROWS - 1, 0, 33]), i32([1, 0, 1, 1, 0]), k, v)
        x, w = rnd(B, Kd, seed=6).to(DEV), rnd(N, Kd, seed=7, scale=0.05).to(DEV)
        return getattr(ops, writer)(x, w, Hq, Hkv, d, cos, sin, i32(pos), k, v)

    a, b = call(far.k, far.v), call(kc, vc)
    assert torch.equal(a[:, :Hq * d], b[:, :Hq * d])
    assert bool((kc[-1, F_ROWS - 1] != fill[0][-1, F_ROWS - 1]).any())            # (the last row of the far block was written)
    far.unchanged_outside(kc, vc)


@pytest.mark.parametrize("writer", ["rope_kv_append_f8_", "rope_kv_append_rows_f8_", "kv_quant_f8"])
def test_f8_cache_writers_beyond_4_gib(ops, writer):
    """The e4m3 writers on far byte views with compact scales: bytes and scales equal those of the same call on a compact cache, the guard
    bands keep the NaN byte.  (decode_kv8.hip: seq * bs + row * ld in 64 bits for bytes and scales.)"""
    Hq, Hkv, d = 4, F_HKV, F_D
    N = (Hq + 2 * Hkv) * d
    cos, sin = rope(ops)
    B = 2
    far, ks, vs = far_f8(ops, B)
    kc, vc = far.compact()
    ksc, vsc, k0 = ks.clone(), vs.clone(), kc.clone()

    def call(k, v, s_k, s_v):
        if writer == "rope_kv_append_f8_":
            ops.rope_kv_append_f8_(rnd(B, N, seed=5).to(DEV), Hq, Hkv, d, cos, sin, i32([9, F_ROWS - 1]), k, v, s_k, s_v)
        elif writer == "rope_kv_append_rows_f8_":
            ops.rope_kv_append_rows_f8_(rnd(5, N, seed=5).to(DEV), Hq, Hkv, d, cos, sin, i32([9, 700, F_ROWS - 1, 0, 33]), i32([1, 0, 1, 1, 0]),
                                        k, v, s_k, s_v)
        else:                                                 # 2 sequences x 30 rows at rows 1070 .. 1099, K then V
            ops.kv_quant_f8(rnd(60, Hkv * d, seed=8).to(DEV), Hkv, d, k, s_k, row0=F_ROWS - 30, rows_per_seq=30)
            ops.kv_quant_f8(rnd(60, Hkv * d, seed=9).to(DEV), Hkv, d, v, s_v, row0=F_ROWS - 30, rows_per_seq=30)

    call(far.k, far.v, ks, vs)
    call(kc, vc, ksc, vsc)
    assert torch.equal(ks, ksc) and torch.equal(vs, vsc)
    assert bool((kc[1, F_ROWS - 1] != k0[1, F_ROWS - 1]).any())                   # (the last row of the far block was written)
    far.unchanged_outside(kc, vc)


# ------------------------------------------------------------------------------------------------ 5. RoPE tables to row 131071

def rope_rows():
    g = torch.Generator().manual_seed(17)
    return torch.cat([torch.tensor([0, 4095, 4096, 65535, 65536, LONG - 1]), torch.randint(0, LONG, (2048,), generator=g)])


@pytest.mark.parametrize("name,scaling", [("llama31_8b", 1.0), ("default", 1.0), ("llama31_8b", 0.5)])
def test_rope_table_freq_to_the_end_of_the_context(ops, name, scaling):
    """mm355_rope_table_freq at 131072 rows: at l = 131071 the angle is ~1.3e5 rad, where only a full argument reduction is right.  Against
    HF's arithmetic on the host (the fp32 product l * inv_freq, cos / sin of it in fp64, times the scaling, one rounding to bf16) with the
    bars of test_rope_table_freq_matches_hf_recorded_tables: no entry more than one bf16 step away, >= 99.5 % bit-identical, halves equal."""
    from conftest import GOLDEN
    inv = np.load(os.path.join(GOLDEN, "r6_rope_tables.npz"))[f"{name}::inv_freq"]
    cos, sin = ops.rope_table_freq(LONG, 128, inv, scaling, DEV)
    assert cos.shape == (LONG, 128) and torch.equal(cos[:, :64], cos[:, 64:]) and torch.equal(sin[:, :64], sin[:, 64:])
    rows = rope_rows()
    cr, sr = K.rope_table_ref(rows, inv, scaling)
    for got, want, what in ((cos, cr, "cos"), (sin, sr, "sin")):
        steps = K.bf16_steps(got.cpu()[rows], want)
        same = float((steps == 0).float().mean())
        print(f"   rope_table_freq {name} x{scaling} {what}: {same:.5f} bit-identical, at most {int(steps.max())} bf16 steps away")
        assert int(steps.max()) <= 1 and same >= 0.995, (name, what, int(steps.max()), same)


def test_rope_kv_append_at_the_last_positions(ops):
    """rope_kv_append_ at positions 131071, 65536 and 0 of the LLaMA-3.1 table, bit for bit against HF's rotation of the same table rows"""
    from conftest import GOLDEN
    inv = np.load(os.path.join(GOLDEN, "r6_rope_tables.npz"))["llama31_8b::inv_freq"]
    Hq, Hkv, d, B = 4, 2, 128, 3
    cos, sin = ops.rope_table_freq(LONG, d, inv, 1.0, DEV)
    pos = [LONG - 1, 65536, 0]
    qkv = rnd(B, (Hq + 2 * Hkv) * d, seed=3, scale=1.0)
    kc = torch.zeros(B, LONG, Hkv * d, device=DEV, dtype=BF16)
    vc = torch.zeros_like(kc)
    dev = qkv.to(DEV)
    ops.rope_kv_append_(dev, Hq, Hkv, d, cos, sin, i32(pos), kc, vc)
    p = torch.tensor(pos)
    rot = K.hf_rope_rows(qkv[:, :(Hq + Hkv) * d], cos.cpu()[p], sin.cpu()[p], d)
    assert torch.equal(dev.cpu()[:, :Hq * d], rot[:, :Hq * d])
    for b, pb in enumerate(pos):
        assert torch.equal(kc[b, pb].cpu(), rot[b, Hq * d:]) and torch.equal(vc[b, pb].cpu(), qkv[b, (Hq + Hkv) * d:])
    assert int((kc != 0).any(-1).sum()) == B and int((vc != 0).any(-1).sum()) == B


def test_rope_table_theta_entry_point_far_rows(ops):
    """mm355_rope_table (the theta entry point; the model uses mm355_rope_table_freq) computes inv_freq on the device with powf, which may
    differ from the host's inv_freq by an ulp -- at l = 131071 that is already a bf16 step or more in the fast bands.  It may be trusted for
    what the code guarantees: both halves of a row equal, row 0 exact (cos 1, sin 0), and a table of short contexts (pinned to 4095 by
    test_rope_table_freq_matches_hf_recorded_tables).  Its distance from the freq table at the far rows is measured and printed, not
    asserted."""
    from conftest import GOLDEN
    inv = np.load(os.path.join(GOLDEN, "r6_rope_tables.npz"))["default::inv_freq"]
    ct, st = ops.rope_table(LONG, 128, 500000.0, DEV)
    cf, sf = ops.rope_table_freq(LONG, 128, inv, 1.0, DEV)
    assert torch.equal(ct[:, :64], ct[:, 64:]) and torch.equal(st[:, :64], st[:, 64:])
    assert bool((ct[0].float() == 1).all()) and bool((st[0].float() == 0).all())
    for rows, what in ((slice(0, 4096), "rows < 4096"), (slice(65536, LONG), "rows >= 65536"), (slice(LONG - 1, LONG), "row 131071")):
        dc = (ct[rows].float() - cf[rows].float()).abs()
        steps = K.bf16_steps(ct[rows].cpu(), cf[rows].cpu())
        print(f"   rope_table vs rope_table_freq, {what}: {float((steps != 0).float().mean()):.4f} of the cos entries differ, "
              f"max |diff| {float(dc.max()):.3e}" + (f", at most {int(steps.max())} bf16 steps" if what.startswith("row ") else ""))
