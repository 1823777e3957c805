"""mm355_attn_extend_ragged / mm355_attn_extend_ragged_f8 on the device: sequence b brings n_b = row_start[b + 1] - row_start[b] query rows,
packed without padding rows, against a cache that already holds them.  A uniform table equals mm355_attn_extend bit for bit (the plan is a
function of the launch arguments alone); ragged tables against tests/test_attn_extend_gpu.py's fp32 formula, evaluated per sequence with
that sequence's own n, at that test's close(1e-2, 1e-2), with NaN in everything the contract says is never read (cache rows >= past[b] +
n_b, the whole block of an empty sequence, q rows beyond row_start[B]) and a sentinel in o whose rows beyond row_start[B] must keep their
bits; the e4m3 form bit for bit against the bf16 form on the dequantised cache; the sink and cliff caches of
test_attn_extend_on_hostile_scores against fp64 at that test's 2^-7; the refusals by return code."""
import pytest
import torch

from test_attn_extend_gpu import close, formula, inputs, kv8_cache

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
SENTINEL = -1.75                                                  # (a bf16 value no output row holds in all columns)

#           B  Hq Hkv  d   past               n
UNIFORM = [(3, 4, 4, 64, (1, 63, 64), 5),
           (2, 32, 4, 128, (513, 77), 64),
           (2, 8, 2, 128, (2500, 1030), 70)]                      # the key split and its merge launch
#          Hq Hkv  d   n_b              past
RAGGED = [(8, 2, 128, (1, 0, 17, 70), (0, 5, 63, 130)),           # an empty sequence, a prompt, 16 packed rows per wave, two row tiles
          (32, 8, 128, (129, 3), (0, 2500)),                      # the key split with one short sequence
          (16, 16, 72, (33, 2), (40, 0)),
          (8, 1, 64, (16, 5), (300, 1))]                          # G = 8
TAIL = 3                                                          # q / o rows beyond row_start[B]


@pytest.fixture(scope="module")
def ops():
    from metamorph_amd import ops as o
    from metamorph_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return o


def _ids(cases):
    return ["-".join("_".join(map(str, x)) if isinstance(x, tuple) else str(x) for x in c) for c in cases]


def _i32(xs):
    return torch.tensor(list(xs), dtype=torch.int32, device=DEV)


def _row_start(ns):
    rs = [0]
    for n in ns:
        rs.append(rs[-1] + n)
    return rs


@pytest.mark.parametrize("case", UNIFORM, ids=_ids(UNIFORM))
def test_uniform_table_equals_attn_extend(ops, case):
    B, Hq, Hkv, d, past, n = case
    q, kc, vc, _ = inputs(case)                                   # (the tail of the cache is poisoned)
    rows = kc.shape[1]
    pd, rs = _i32(past), _i32(b * n for b in range(B + 1))
    kd, vd, qd = kc.view(B, rows, Hkv * d).to(DEV), vc.view(B, rows, Hkv * d).to(DEV), q.view(B * n, Hq * d).to(DEV)
    for bound in (max(past) + n, rows):
        ref = ops.attn_extend(qd, kd, vd, pd, n, bound, Hq, Hkv, d, d ** -0.5)
        got = ops.attn_extend_ragged(qd, kd, vd, pd, rs, n, bound, Hq, Hkv, d, d ** -0.5)
        assert bool(torch.isfinite(got.float()).all()) and torch.equal(got, ref), (case, bound)


_RAGGED = {}


def ragged_inputs(case):
    """(q packed + NaN tail, kc, vc poisoned, reference for the packed rows) on the CPU, made once"""
    if case not in _RAGGED:
        Hq, Hkv, d, ns, past = case
        B, R = len(ns), sum(ns)
        rows = max(p + n for p, n in zip(past, ns)) + 5
        g = torch.Generator().manual_seed(3 + sum(past) + R)
        q = (torch.randn(R + TAIL, Hq, d, generator=g) * 0.7).bfloat16()
        kc = (torch.randn(B, rows, Hkv, d, generator=g) * 0.7).bfloat16()
        vc = (torch.randn(B, rows, Hkv, d, generator=g) * 0.7).bfloat16()
        rs = _row_start(ns)
        ref = torch.cat([formula(q[rs[b]:rs[b + 1]][None], kc[b:b + 1], vc[b:b + 1], [past[b]], ns[b], Hq, Hkv, d)
                         for b in range(B) if ns[b]], 0)
        for b in range(B):                                        # never read: rows >= past + n_b, and every row of an empty sequence
            lo = past[b] + ns[b] if ns[b] else 0
            kc[b, lo:] = float("nan")
            vc[b, lo:] = float("nan")
        q[R:] = float("nan")
        _RAGGED[case] = (q, kc, vc, ref)
    return _RAGGED[case]


@pytest.mark.parametrize("case", RAGGED, ids=_ids(RAGGED))
def test_ragged_table_against_the_formula(ops, case):
    Hq, Hkv, d, ns, past = case
    q, kc, vc, ref = ragged_inputs(case)
    B, R, rows = len(ns), sum(ns), kc.shape[1]
    qd = q.view(R + TAIL, Hq * d).to(DEV)
    kd, vd = kc.view(B, rows, Hkv * d).to(DEV), vc.view(B, rows, Hkv * d).to(DEV)
    pd, rs = _i32(past), _i32(_row_start(ns))
    for bound in (max(p + n for p, n in zip(past, ns)), rows):    # the capacity as the bound: another split, the tail still never read
        o = torch.full((R + TAIL, Hq * d), SENTINEL, device=DEV, dtype=BF16)
        ret = ops.attn_extend_ragged(qd, kd, vd, pd, rs, max(ns), bound, Hq, Hkv, d, d ** -0.5, out=o)
        assert ret.data_ptr() == o.data_ptr()
        close(o[:R], ref, 1e-2, 1e-2, f"attn_extend_ragged {case}, bound {bound}")
        assert bool((o[R:] == SENTINEL).all()), "rows that belong to no sequence were written"
    # n_max beyond every n_b (the launch is sized by it; the extra row tiles leave at once), q and o as column views of wider tensors
    wide_q = torch.full((R + TAIL, Hq * d + 2 * Hkv * d), float("nan"), device=DEV, dtype=BF16)
    wide_q[:R, :Hq * d] = qd[:R]
    wide_o = torch.full((R + TAIL, Hq * d + 64), SENTINEL, device=DEV, dtype=BF16)
    ops.attn_extend_ragged(wide_q[:, :Hq * d], kd, vd, pd, rs, min(max(ns) + 70, rows), rows, Hq, Hkv, d, d ** -0.5, out=wide_o[:, 64:])
    close(wide_o[:R, 64:], ref, 1e-2, 1e-2, f"attn_extend_ragged {case}, a larger n_max, views")
    assert bool((wide_o[:, :64] == SENTINEL).all()) and bool((wide_o[R:] == SENTINEL).all())


@pytest.mark.parametrize("case", RAGGED[:2], ids=_ids(RAGGED[:2]))
def test_ragged_f8_equals_the_bf16_form_on_the_dequantised_cache(ops, case):
    Hq, Hkv, d, ns, past = case
    B, R = len(ns), sum(ns)
    rows = max(p + n for p, n in zip(past, ns)) + 5
    k8, ks, v8, vs = kv8_cache(B, rows, Hkv, d, seed=sum(past) + d + R)
    kb, vb = ops.dequant_kv8(k8, ks, Hkv, d), ops.dequant_kv8(v8, vs, Hkv, d)      # (before the tail is poisoned)
    for b in range(B):                                            # never read: the NaN byte and a NaN scale
        lo = past[b] + ns[b] if ns[b] else 0
        for t8, ts in ((k8, ks), (v8, vs)):
            t8[b, lo:] = 0x7F
            ts[b, lo:] = float("nan")
    q = (torch.randn(R, Hq * d, generator=torch.Generator().manual_seed(5)) * 0.7).bfloat16().to(DEV)
    pd, rs = _i32(past), _i32(_row_start(ns))
    for bound in (max(p + n for p, n in zip(past, ns)), rows):
        ref = ops.attn_extend_ragged(q, kb.to(DEV), vb.to(DEV), pd, rs, max(ns), bound, Hq, Hkv, d, d ** -0.5)
        got = ops.attn_extend_ragged_f8(q, k8.to(DEV), v8.to(DEV), ks.to(DEV), vs.to(DEV), pd, rs, max(ns), bound, Hq, Hkv, d, d ** -0.5)
        assert bool(torch.isfinite(got.float()).all()) and torch.equal(got, ref), (case, bound)


@pytest.mark.parametrize("kind", ["sink", "cliff"])
def test_ragged_on_hostile_scores(ops, kind):
    """test_attn_extend_on_hostile_scores' sink and cliff caches with n_b = (40, 9) new rows, against fp64 at that test's 2^-7"""
    B, Hq, Hkv, d, past, ns = 2, 32, 8, 128, [2500, 700], (40, 9)
    rows = max(p + n for p, n in zip(past, ns)) + 3
    g = torch.Generator().manual_seed(11)
    q = (torch.randn(sum(ns), Hq, d, generator=g) * 0.5).bfloat16()
    kc = (torch.randn(B, rows, Hkv, d, generator=g) * 0.5).bfloat16()
    vc = torch.randn(B, rows, Hkv, d, generator=g).bfloat16()
    unit = d ** -0.5 * 8.0
    q[..., 0] = 8.0
    kc[..., 0] = 0
    if kind == "sink":
        kc[:, 0, :, 0] = 40.0 / unit
    else:
        kc[..., 0] = -40.0 / unit
        for b in range(B):
            for i in range(7, ns[b]):
                kc[b, past[b] + i - 7, :, 0] = 40.0 / unit
    rs = _row_start(ns)
    ref = torch.cat([formula(q[rs[b]:rs[b + 1]][None], kc[b:b + 1], vc[b:b + 1], [past[b]], ns[b], Hq, Hkv, d, dtype=torch.float64)
                     for b in range(B)], 0)
    for b in range(B):
        kc[b, past[b] + ns[b]:] = float("nan")
        vc[b, past[b] + ns[b]:] = float("nan")
    got = ops.attn_extend_ragged(q.view(sum(ns), Hq * d).to(DEV), kc.view(B, rows, Hkv * d).to(DEV), vc.view(B, rows, Hkv * d).to(DEV),
                                 _i32(past), _i32(rs), max(ns), max(p + n for p, n in zip(past, ns)), Hq, Hkv, d, d ** -0.5)
    close(got, ref, 2.0 ** -7, 2.0 ** -7, f"attn_extend_ragged {kind}")


def test_ragged_entry_points_check_their_arguments(ops):
    L = ops._L()
    st = torch.cuda.current_stream().cuda_stream
    B, Hq, Hkv, d, rows, R = 2, 4, 2, 128, 16, 6
    q = torch.zeros(R, Hq * d, device=DEV, dtype=BF16)
    o = torch.full((R, Hq * d), SENTINEL, device=DEV, dtype=BF16)
    k = torch.zeros(B, rows, Hkv * d, device=DEV, dtype=BF16)
    k8 = torch.zeros(B, rows, Hkv * d, device=DEV, dtype=torch.uint8)
    sc = torch.ones(B, rows, Hkv, device=DEV, dtype=torch.float32)
    past, rs = _i32([3, 0]), _i32([0, 4, 6])
    P = lambda t: t.data_ptr()
    ld, bs = Hkv * d, rows * Hkv * d

    def bf(q_=None, ldq=Hq * d, k_=None, ldkv=ld, bskv=bs, past_=None, rs_=None, n_max=4, q_rows=R, bound=rows, o_=None, ldo=Hq * d, Hq_=Hq, d_=d):
        return L.mm355_attn_extend_ragged(P(q) if q_ is None else q_, ldq, P(k) if k_ is None else k_, P(k), ldkv, bskv,
                                          P(past) if past_ is None else past_, P(rs) if rs_ is None else rs_, n_max, q_rows, bound,
                                          P(o) if o_ is None else o_, ldo, B, Hq_, Hkv, d_, 0.1, 0, 0, st)

    def f8(fmt=1, ks_=None, vs_=None, k_=None, ldkv=ld, rs_=None, n_max=4, q_rows=R, d_=d, Hq_=Hq):
        return L.mm355_attn_extend_ragged_f8(P(q), Hq_ * d, P(k8) if k_ is None else k_, P(k8), ldkv, bs, P(sc) if ks_ is None else ks_,
                                             P(sc) if vs_ is None else vs_, Hkv, rows * Hkv, fmt, P(past), P(rs) if rs_ is None else rs_, n_max,
                                             q_rows, rows, P(o), Hq_ * d, B, Hq_, Hkv, d_, 0.1, 0, 0, st)
    # every refusal first, on the sentinel output: nothing may have been launched
    assert bf(rs_=0) == -1 and bf(n_max=0) == -1 and bf(n_max=rows + 1) == -1 and bf(q_rows=0) == -1      # the ragged form's own
    assert bf(q_=0) == -1 and bf(past_=0) == -1 and bf(o_=0) == -1 and bf(k_=0) == -1                      # NULL pointers
    assert bf(q_=P(q) + 2) == -1 and bf(o_=P(o) + 8) == -1 and bf(k_=P(k) + 8) == -1                       # misaligned pointers
    assert bf(ldq=Hq * d + 4) == -1 and bf(ldo=Hq * d + 2) == -1 and bf(ldkv=ld + 4) == -1 and bf(bskv=bs + 4) == -1
    assert bf(ldkv=ld - 8) == -1 and bf(Hq_=5) == -1
    assert bf(d_=124) == -2 and bf(d_=136) == -2 and bf(Hq_=6, ldq=6 * d, ldo=6 * d) == -2 and bf(Hq_=32, ldq=32 * d, ldo=32 * d) == -2
    assert f8(fmt=7) == -1 and f8(ks_=0) == -1 and f8(vs_=0) == -1 and f8(rs_=0) == -1 and f8(n_max=0) == -1 and f8(n_max=rows + 1) == -1
    assert f8(q_rows=0) == -1 and f8(k_=P(k8) + 4) == -1 and f8(ldkv=ld + 4) == -1 and f8(ks_=P(sc) + 2) == -1
    assert f8(d_=124) == -2 and f8(Hq_=6) == -2
    # a key split without its workspace: 16 workgroups of row tiles on a bound of 4096 keys
    big = torch.zeros(B, 4096, Hkv * d, device=DEV, dtype=BF16)
    assert L.mm355_attn_extend_ragged_ws_floats(B, 4, Hq, Hkv, d, 4096) > 0
    assert L.mm355_attn_extend_ragged(P(q), Hq * d, P(big), P(big), ld, 4096 * ld, P(past), P(rs), 4, R, 4096, P(o), Hq * d, B, Hq, Hkv, d, 0.1,
                                      0, 0, st) == -1
    torch.cuda.synchronize()
    assert bool((o == SENTINEL).all()), "a refused call wrote its output"
    assert bf() == 0 and f8() == 0                                # the well-formed calls (no key split here: no workspace needed)
    torch.cuda.synchronize()
    assert not bool((o == SENTINEL).any())
