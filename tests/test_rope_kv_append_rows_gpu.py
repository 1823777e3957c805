"""mm355_rope_kv_append_rows / mm355_rope_kv_append_rows_f8 on the device: mm355_rope_kv_append(_f8) with a block and a position per row.
The yardstick is bit identity with the existing kernels: without a table (block r for row r) the same call; with a table every row against
a one-row call of the existing kernel on its block, the caches compared WHOLE so that every row that was not named keeps its sentinel
bits; 70 000 rows (past the old grid bound) on 16 sampled rows; the refusals by return code."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
SHAPES = [(8, 2, 128), (4, 4, 64)]
R, NBLK, LMAX = 7, 3, 40
POS = [0, 39, 17, 5, 39, 21, 8]                                   # scattered, both ends of a block
BLK = [2, 0, 1, 1, 2, 0, 2]                                       # two (three) rows into one block


@pytest.fixture(scope="module")
def ops():
    from metamorph_amd import ops as o
    from metamorph_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return o


def _rows(n, Hq, Hkv, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, (Hq + 2 * Hkv) * d, generator=g) * 2.0).bfloat16()
    x[0, Hq * d:Hq * d + d] = 0                                   # a zero K head-row
    return x.to(DEV)


def _i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device=DEV)


def _bf16_caches(nblk, W):
    return torch.full((nblk, LMAX, W), -3.0, device=DEV, dtype=BF16), torch.full((nblk, LMAX, W), -3.0, device=DEV, dtype=BF16)


def _f8_caches(nblk, Hkv, W):
    k8 = torch.full((nblk, LMAX, W), 0xA5, dtype=torch.uint8, device=DEV)
    ks = torch.full((nblk, LMAX, Hkv), -7.0, dtype=torch.float32, device=DEV)
    return k8, k8.clone(), ks, ks.clone()


@pytest.mark.parametrize("shape", SHAPES)
def test_without_a_table_it_is_rope_kv_append(ops, shape):
    Hq, Hkv, d = shape
    qkv = _rows(R, Hq, Hkv, d, seed=d)
    cos, sin = ops.rope_table(LMAX, d, 10000.0, DEV)
    pos = _i32(POS)
    kr, vr = _bf16_caches(R, Hkv * d)
    ref = ops.rope_kv_append_(qkv.clone(), Hq, Hkv, d, cos, sin, pos, kr, vr)
    kg, vg = _bf16_caches(R, Hkv * d)
    got = ops.rope_kv_append_rows_(qkv.clone(), Hq, Hkv, d, cos, sin, pos, None, kg, vg)
    assert torch.equal(got, ref) and torch.equal(kg, kr) and torch.equal(vg, vr)
    assert not torch.equal(kg, _bf16_caches(R, Hkv * d)[0])
    k8r, v8r, ksr, vsr = _f8_caches(R, Hkv, Hkv * d)
    ref8 = ops.rope_kv_append_f8_(qkv.clone(), Hq, Hkv, d, cos, sin, pos, k8r, v8r, ksr, vsr)
    k8, v8, ks, vs = _f8_caches(R, Hkv, Hkv * d)
    got8 = ops.rope_kv_append_rows_f8_(qkv.clone(), Hq, Hkv, d, cos, sin, pos, None, k8, v8, ks, vs)
    assert torch.equal(got8, ref8) and torch.equal(got8, ref)
    for a, b in ((k8, k8r), (v8, v8r), (ks, ksr), (vs, vsr)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape", SHAPES)
def test_with_a_table_every_row_is_a_one_row_call_on_its_block(ops, shape):
    Hq, Hkv, d = shape
    qkv = _rows(R, Hq, Hkv, d, seed=d + 1)
    cos, sin = ops.rope_table(LMAX, d, 10000.0, DEV)
    pos, blk = _i32(POS), _i32(BLK)
    kr, vr = _bf16_caches(NBLK, Hkv * d)
    k8r, v8r, ksr, vsr = _f8_caches(NBLK, Hkv, Hkv * d)
    ref, ref8 = qkv.clone(), qkv.clone()
    for r in range(R):                                            # the existing kernels, one row into block BLK[r] at a time
        b = BLK[r]
        ops.rope_kv_append_(ref[r:r + 1], Hq, Hkv, d, cos, sin, pos[r:r + 1], kr[b:b + 1], vr[b:b + 1])
        ops.rope_kv_append_f8_(ref8[r:r + 1], Hq, Hkv, d, cos, sin, pos[r:r + 1], k8r[b:b + 1], v8r[b:b + 1], ksr[b:b + 1], vsr[b:b + 1])
    kg, vg = _bf16_caches(NBLK, Hkv * d)
    got = ops.rope_kv_append_rows_(qkv.clone(), Hq, Hkv, d, cos, sin, pos, blk, kg, vg)
    assert torch.equal(got, ref) and torch.equal(got[:, Hq * d:], qkv[:, Hq * d:])
    assert torch.equal(kg, kr) and torch.equal(vg, vr)            # whole: the R named rows, every other row its sentinel
    assert int((kg != -3.0).any(dim=2).sum()) == R and int((vg != -3.0).any(dim=2).sum()) == R
    k8, v8, ks, vs = _f8_caches(NBLK, Hkv, Hkv * d)
    got8 = ops.rope_kv_append_rows_f8_(qkv.clone(), Hq, Hkv, d, cos, sin, pos, blk, k8, v8, ks, vs)
    assert torch.equal(got8, ref8) and torch.equal(got8, ref)
    for a, b in ((k8, k8r), (v8, v8r), (ks, ksr), (vs, vsr)):
        assert torch.equal(a, b)
    assert int((ks != -7.0).any(dim=2).sum()) == R
    # entries out of range are clamped into the cache: block 9 -> the last block, position -4 -> row 0, position 99 -> the last row
    kc, vc = _bf16_caches(NBLK, Hkv * d)
    ops.rope_kv_append_rows_(qkv[:3].clone(), Hq, Hkv, d, cos, sin, _i32([7, -4, 99]), _i32([9, -1, 1]), kc, vc)
    named = (kc != -3.0).any(dim=2).nonzero().tolist()
    assert named == [[0, 0], [1, LMAX - 1], [NBLK - 1, 7]], named


def test_more_rows_than_a_grid_dimension(ops):
    Hq, Hkv, d, n = 2, 1, 16, 70000                               # (the existing kernels take at most 65535 rows)
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(n, (Hq + 2 * Hkv) * d, generator=g).bfloat16().to(DEV)
    cos, sin = ops.rope_table(4, d, 10000.0, DEV)
    pos = torch.randint(0, 2, (n,), generator=g).to(torch.int32).to(DEV)
    kg = torch.full((n, 2, Hkv * d), -3.0, device=DEV, dtype=BF16)
    vg = kg.clone()
    got = ops.rope_kv_append_rows_(qkv.clone(), Hq, Hkv, d, cos, sin, pos, None, kg, vg)
    k8 = torch.full((n, 2, Hkv * d), 0xA5, dtype=torch.uint8, device=DEV)
    v8, ks = k8.clone(), torch.full((n, 2, Hkv), -7.0, dtype=torch.float32, device=DEV)
    vs = ks.clone()
    got8 = ops.rope_kv_append_rows_f8_(qkv.clone(), Hq, Hkv, d, cos, sin, pos, None, k8, v8, ks, vs)
    assert torch.equal(got8, got)
    assert int((kg != -3.0).any(dim=2).sum()) == n and int((ks != -7.0).any(dim=2).sum()) == n
    for r in [0, 1, 65534, 65535, 65536, n - 1] + torch.randint(0, n, (10,), generator=g).tolist():
        k1, v1 = torch.full((1, 2, Hkv * d), -3.0, device=DEV, dtype=BF16), torch.full((1, 2, Hkv * d), -3.0, device=DEV, dtype=BF16)
        q1 = ops.rope_kv_append_(qkv[r:r + 1].clone(), Hq, Hkv, d, cos, sin, pos[r:r + 1], k1, v1)
        assert torch.equal(got[r:r + 1], q1) and torch.equal(kg[r:r + 1], k1) and torch.equal(vg[r:r + 1], v1), r
        a8, b8 = torch.full((1, 2, Hkv * d), 0xA5, dtype=torch.uint8, device=DEV), torch.full((1, 2, Hkv * d), 0xA5, dtype=torch.uint8, device=DEV)
        as_, bs_ = torch.full((1, 2, Hkv), -7.0, device=DEV), torch.full((1, 2, Hkv), -7.0, device=DEV)
        ops.rope_kv_append_f8_(qkv[r:r + 1].clone(), Hq, Hkv, d, cos, sin, pos[r:r + 1], a8, b8, as_, bs_)
        assert torch.equal(k8[r:r + 1], a8) and torch.equal(v8[r:r + 1], b8) and torch.equal(ks[r:r + 1], as_) and torch.equal(vs[r:r + 1], bs_), r


def test_rows_entry_points_check_their_arguments(ops):
    L = ops._L()
    st = torch.cuda.current_stream().cuda_stream
    Hq, Hkv, d = 8, 2, 128
    W, ld = Hkv * d, (Hq + 2 * Hkv) * d
    qkv = _rows(R, Hq, Hkv, d, seed=9)
    keep = qkv.clone()
    cos, sin = ops.rope_table(LMAX, d, 10000.0, DEV)
    pos, blk = _i32(POS), _i32(BLK)
    kc, vc = _bf16_caches(NBLK, W)
    k8, v8, ks, vs = _f8_caches(NBLK, Hkv, W)
    P = lambda t: t.data_ptr()

    def bf(qkv_=None, ld_=ld, R_=R, d_=d, pos_=None, blk_=None, nblk=NBLK, rpb=LMAX, k_=None, ldkv=W, bs=LMAX * W):
        return L.mm355_rope_kv_append_rows(P(qkv) if qkv_ is None else qkv_, ld_, R_, Hq, Hkv, d_, P(cos), P(sin), P(pos) if pos_ is None else pos_,
                                           P(blk) if blk_ is None else blk_, nblk, rpb, P(kc) if k_ is None else k_, P(vc), ldkv, bs, st)

    def f8(fmt=1, R_=R, d_=d, pos_=None, blk_=None, nblk=NBLK, rpb=LMAX, k_=None, ks_=None, ldkv=W):
        return L.mm355_rope_kv_append_rows_f8(P(qkv), ld, R_, Hq, Hkv, d_, P(cos), P(sin), P(pos) if pos_ is None else pos_,
                                              P(blk) if blk_ is None else blk_, nblk, rpb, P(k8) if k_ is None else k_, P(v8), ldkv, LMAX * W,
                                              P(ks) if ks_ is None else ks_, P(vs), Hkv, LMAX * Hkv, fmt, st)
    assert bf(nblk=0) == -1 and bf(rpb=0) == -1 and f8(nblk=0) == -1 and f8(rpb=0) == -1      # the new bounds
    assert bf(blk_=0) == -1 and f8(blk_=0) == -1                 # no table: block r for row r needs R blocks
    assert bf(qkv_=0) == -1 and bf(pos_=0) == -1 and bf(k_=0) == -1 and bf(R_=0) == -1         # the existing kernel's refusals
    assert bf(d_=72) == -1 and bf(ld_=ld + 4) == -1 and bf(ldkv=W + 4) == -1 and bf(bs=LMAX * W + 4) == -1
    assert f8(fmt=7) == -1 and f8(pos_=0) == -1 and f8(ks_=0) == -1 and f8(R_=0) == -1 and f8(k_=P(k8) + 4) == -1 and f8(ldkv=W - 8) == -1
    assert f8(d_=72) == -1 and f8(d_=132) == -2
    torch.cuda.synchronize()
    assert torch.equal(qkv, keep) and bool((kc == -3.0).all()) and bool((k8 == 0xA5).all()) and bool((ks == -7.0).all())
    assert bf() == 0 and f8() == 0                                # the well-formed calls
    torch.cuda.synchronize()
