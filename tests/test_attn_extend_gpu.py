"""mm355_attn_extend / mm355_attn_extend_f8 on the device: n new query rows per sequence at positions past .. past + n - 1 against a cache
that already holds them.  Against the fp32 formula on the CPU (as test_attn_decode: softmax(q K^T d^-0.5) V over the keys 0 .. past + i,
close(1e-2, 1e-2)), with every cache row >= past + n poisoned; on the sink and cliff caches of test_attn_decode_on_hostile_scores at that
test's 2^-7 against fp64; the e4m3 form bit for bit against the bf16 form on the dequantised cache; and the argument refusals by return
code.  The cases cover n = 1, an empty prefix, row tiles and key tiles that are no multiple of 64, GQA groups 1 / 2 / 4 / 8, d = 64 / 72 /
128, one workgroup per (sequence, KV head) and the key split with its merge launch (few workgroups on a long prefix)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16

#        B  Hq Hkv  d   past               n
CASES = [(1, 8, 2, 128, (0,), 1),
         (1, 8, 2, 128, (0,), 130),
         (3, 4, 4, 64, (1, 63, 64), 5),
         (2, 32, 4, 128, (513, 77), 64),
         (1, 16, 16, 72, (40,), 33),
         (2, 8, 2, 128, (2500, 1030), 70),
         (1, 4, 2, 64, (4000,), 1),
         (3, 32, 8, 128, (127, 128, 129), 129),
         (1, 8, 1, 128, (300,), 16)]


@pytest.fixture(scope="module")
def ops():
    from metamorph_amd import ops as o
    from metamorph_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return o


def close(got, ref, rtol, atol, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    print(f"   {what}: max abs err {float(err.max()):.3e}, max |ref| {float(ref.abs().max()):.3e}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} off, max abs err {float(err.max())}"


def formula(q, kc, vc, past, n, Hq, Hkv, d, dtype=torch.float32):
    """q [B, n, Hq, d], kc / vc [B, rows, Hkv, d] (any float dtype) -> [B * n, Hq * d]: row (b, i) over the keys 0 .. past[b] + i"""
    B, G = q.shape[0], Hq // Hkv
    out = torch.empty(B, n, Hq * d, dtype=dtype)
    for b in range(B):
        m = past[b] + n
        kk = kc[b, :m].to(dtype).transpose(0, 1).repeat_interleave(G, dim=0)                  # [Hq, m, d]
        vv = vc[b, :m].to(dtype).transpose(0, 1).repeat_interleave(G, dim=0)
        s = (q[b].to(dtype).transpose(0, 1) @ kk.transpose(1, 2)) * d ** -0.5                 # [Hq, n, m]
        keys, rows = torch.arange(m)[None, None, :], (past[b] + torch.arange(n))[None, :, None]
        s = s.masked_fill(keys > rows, float("-inf"))
        out[b] = (torch.softmax(s, dim=-1) @ vv).transpose(0, 1).reshape(n, Hq * d)
    return out.view(B * n, Hq * d)


_INPUTS = {}


def inputs(case):
    """(q, kc, vc, reference) of a case on the CPU, made once and shared by the tests that need them"""
    if case not in _INPUTS:
        B, Hq, Hkv, d, past, n = case
        rows = max(past) + n + 5
        g = torch.Generator().manual_seed(7 + sum(past) + n)
        q = (torch.randn(B, n, Hq, d, generator=g) * 0.7).bfloat16()
        kc = (torch.randn(B, rows, Hkv, d, generator=g) * 0.7).bfloat16()
        vc = (torch.randn(B, rows, Hkv, d, generator=g) * 0.7).bfloat16()
        ref = formula(q, kc, vc, past, n, Hq, Hkv, d)
        for b in range(B):                                        # rows the contract says are never read
            kc[b, past[b] + n:] = float("nan")
            vc[b, past[b] + n:] = float("nan")
        _INPUTS[case] = (q, kc, vc, ref)
    return _INPUTS[case]


CASE_IDS = ["-".join(str(x) for x in (c[0], c[1], c[2], c[3], "_".join(map(str, c[4])), c[5])) for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_attn_extend_against_the_formula(ops, case):
    B, Hq, Hkv, d, past, n = case
    q, kc, vc, ref = inputs(case)
    rows = kc.shape[1]
    pd = torch.tensor(past, dtype=torch.int32, device=DEV)
    kd, vd = kc.view(B, rows, Hkv * d).to(DEV), vc.view(B, rows, Hkv * d).to(DEV)
    qd = q.view(B * n, Hq * d).to(DEV)
    bound = max(past) + n
    got = ops.attn_extend(qd, kd, vd, pd, n, bound, Hq, Hkv, d, d ** -0.5)
    close(got, ref, 1e-2, 1e-2, f"attn_extend {case}")
    # the capacity as the bound (another key split for the same rows): the poisoned tail is still never read
    close(ops.attn_extend(qd, kd, vd, pd, n, rows, Hq, Hkv, d, d ** -0.5), ref, 1e-2, 1e-2, f"attn_extend {case}, bound = capacity")
    # q and o as column views of a wider tensor (the q block of a fused q|k|v activation; an output block)
    wide_q = torch.full((B * n, Hq * d + 2 * Hkv * d), float("nan"), device=DEV, dtype=BF16)
    wide_q[:, :Hq * d] = qd
    wide_o = torch.zeros((B * n, Hq * d + 64), device=DEV, dtype=BF16)
    o_view = wide_o[:, 64:]
    ret = ops.attn_extend(wide_q[:, :Hq * d], kd, vd, pd, n, bound, Hq, Hkv, d, d ** -0.5, out=o_view)
    assert ret.data_ptr() == o_view.data_ptr() and torch.equal(o_view, got) and float(wide_o[:, :64].float().abs().max()) == 0


@pytest.mark.parametrize("kind", ["sink", "cliff"])
def test_attn_extend_on_hostile_scores(ops, kind):
    """The sink (key 0 of the prefix, +40 over everything else) and the cliff (every score at -40 except keys at +40, here the key 7 before
    each query row's own position, inside the chunk: a row's last key tile lifts its maximum by 115 log2 units, and the partials of the key
    split differ by as much when they are merged) of test_attn_decode_on_hostile_scores, against fp64."""
    B, Hq, Hkv, d, past, n = 2, 32, 8, 128, [2500, 700], 40
    rows = max(past) + n + 3
    g = torch.Generator().manual_seed(11)
    q = (torch.randn(B, n, Hq, d, generator=g) * 0.5).bfloat16()
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
            for i in range(7, n):                                 # (rows 0 .. 6: their cliff key would lie in the prefix; they see a flat -40)
                kc[b, past[b] + i - 7, :, 0] = 40.0 / unit
    ref = formula(q, kc, vc, past, n, Hq, Hkv, d, dtype=torch.float64)
    for b in range(B):
        kc[b, past[b] + n:] = float("nan")
        vc[b, past[b] + n:] = float("nan")
    got = ops.attn_extend(q.view(B * n, Hq * d).to(DEV), kc.view(B, rows, Hkv * d).to(DEV), vc.view(B, rows, Hkv * d).to(DEV),
                          torch.tensor(past, dtype=torch.int32, device=DEV), n, max(past) + n, Hq, Hkv, d, d ** -0.5)
    close(got, ref, 2.0 ** -7, 2.0 ** -7, f"attn_extend {kind}")


def kv8_cache(B, rows, Hkv, d, seed):
    """tests/test_kv8_gpu.py's cache: scales drawn per key and head over 2^-6 .. 2^6, the bytes so that the dequantised values stay ~ N(0, 1)"""
    g = torch.Generator().manual_seed(seed)

    def one():
        e = torch.randint(-6, 7, (B, rows, Hkv), generator=g)
        s = torch.ldexp(torch.ones(B, rows, Hkv), e)
        y = (torch.randn(B, rows, Hkv, d, generator=g) / s[..., None]).clamp(-448, 448)
        return y.to(torch.float8_e4m3fn).view(torch.uint8).reshape(B, rows, Hkv * d).contiguous(), s.contiguous()
    return one() + one()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_attn_extend_f8_equals_attn_extend_on_the_dequantised_cache(ops, case):
    B, Hq, Hkv, d, past, n = case
    rows = max(past) + n + 5
    k8, ks, v8, vs = kv8_cache(B, rows, Hkv, d, seed=sum(past) + d + n)
    kb, vb = ops.dequant_kv8(k8, ks, Hkv, d), ops.dequant_kv8(v8, vs, Hkv, d)      # (before the tail is poisoned)
    for b in range(B):                                            # past the end: the NaN byte and a NaN scale
        for t8, ts in ((k8, ks), (v8, vs)):
            t8[b, past[b] + n:] = 0x7F
            ts[b, past[b] + n:] = float("nan")
    q = (torch.randn(B * n, Hq * d, generator=torch.Generator().manual_seed(5)) * 0.7).bfloat16().to(DEV)
    pd = torch.tensor(past, dtype=torch.int32, device=DEV)
    for bound in (max(past) + n, rows):
        ref = ops.attn_extend(q, kb.to(DEV), vb.to(DEV), pd, n, bound, Hq, Hkv, d, d ** -0.5)
        got = ops.attn_extend_f8(q, k8.to(DEV), v8.to(DEV), ks.to(DEV), vs.to(DEV), pd, n, bound, Hq, Hkv, d, d ** -0.5)
        assert bool(torch.isfinite(got.float()).all()) and torch.equal(got, ref), (case, bound)


def test_attn_extend_entry_points_check_their_arguments(ops):
    L = ops._L()
    st = torch.cuda.current_stream().cuda_stream
    B, n, Hq, Hkv, d, rows = 1, 4, 4, 2, 128, 16
    q = torch.zeros(B * n, Hq * d, device=DEV, dtype=BF16)
    o = torch.zeros_like(q)
    k = torch.zeros(B, rows, Hkv * d, device=DEV, dtype=BF16)
    k8 = torch.zeros(B, rows, Hkv * d, device=DEV, dtype=torch.uint8)
    sc = torch.ones(B, rows, Hkv, device=DEV, dtype=torch.float32)
    past = torch.full((B,), 3, device=DEV, dtype=torch.int32)
    P = lambda t: t.data_ptr()
    ld, bs = Hkv * d, rows * Hkv * d

    def bf(q_=None, ldq=Hq * d, k_=None, ldkv=ld, bskv=bs, past_=None, n_=n, bound=rows, o_=None, ldo=Hq * d, Hq_=Hq, Hkv_=Hkv, d_=d):
        return L.mm355_attn_extend(P(q) if q_ is None else q_, ldq, P(k) if k_ is None else k_, P(k), ldkv, bskv, P(past) if past_ is None else past_,
                                   n_, bound, P(o) if o_ is None else o_, ldo, B, Hq_, Hkv_, d_, 0.1, 0, 0, st)

    def f8(fmt=1, ks_=None, vs_=None, k_=None, ldkv=ld, d_=d, Hq_=Hq):
        return L.mm355_attn_extend_f8(P(q), Hq_ * d, P(k8) if k_ is None else k_, P(k8), ldkv, bs, P(sc) if ks_ is None else ks_,
                                      P(sc) if vs_ is None else vs_, Hkv, rows * Hkv, fmt, P(past), n, rows, P(o), Hq_ * d, B, Hq_, Hkv, d_, 0.1, 0, 0, st)
    assert bf() == 0 and f8() == 0                                # the well-formed calls (no key split here: no workspace needed)
    assert bf(q_=0) == -1 and bf(past_=0) == -1 and bf(o_=0) == -1 and bf(k_=0) == -1          # NULL pointers
    assert bf(q_=P(q) + 2) == -1 and bf(o_=P(o) + 8) == -1 and bf(k_=P(k) + 8) == -1           # misaligned pointers
    assert bf(ldq=Hq * d + 4) == -1 and bf(ldo=Hq * d + 2) == -1 and bf(ldkv=ld + 4) == -1 and bf(bskv=bs + 4) == -1   # misaligned strides
    assert bf(ldkv=ld - 8) == -1                                  # a row stride shorter than a row
    assert bf(n_=rows + 1) == -1 and bf(Hq_=5) == -1              # more new rows than the bound; Hq % Hkv
    assert bf(d_=124) == -2 and bf(d_=136) == -2                  # d % 8, d > 128
    assert bf(Hq_=6, ldq=6 * d, ldo=6 * d) == -2 and bf(Hq_=32, ldq=32 * d, ldo=32 * d) == -2  # GQA groups of 3 and 16
    assert f8(fmt=7) == -1 and f8(ks_=0) == -1 and f8(vs_=0) == -1                             # a format that does not exist, NULL scales
    assert f8(k_=P(k8) + 4) == -1 and f8(ldkv=ld + 4) == -1 and f8(ks_=P(sc) + 2) == -1        # 8-byte cache alignment, 4-byte scales
    assert f8(d_=124) == -2 and f8(Hq_=6) == -2
    # a key split without its workspace is refused before any launch: 8 workgroups of row tiles on a bound of 4096 keys
    big = torch.zeros(1, 4096, Hkv * d, device=DEV, dtype=BF16)
    assert L.mm355_attn_extend_ws_floats(1, 1, Hq, Hkv, d, 4096) > 0
    assert L.mm355_attn_extend(P(q), Hq * d, P(big), P(big), ld, 4096 * ld, P(past), 1, 4096, P(o), Hq * d, 1, Hq, Hkv, d, 0.1, 0, 0, st) == -1
    from metamorph_amd.lib import Mm355Error
    with pytest.raises(Mm355Error, match=r"\(-2\)$"):
        ops.attn_extend(torch.zeros(n, 6 * d, device=DEV, dtype=BF16), k, k.clone(), past, n, rows, 6, 2, d, 0.1)
    torch.cuda.synchronize()
