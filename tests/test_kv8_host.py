"""The host side of the FP8 (e4m3) KV cache: ops.quantize_kv8 / dequant_kv8 against the contract written out by hand (power-of-two scale, the
smallest admissible one; RNE onto the e4m3fn grid by exhaustive search, ties to the even byte; exact dequantisation), and the bytes a
KVCache(fmt="fp8_e4m3") holds.  CPU only."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metamorph_amd import ops  # noqa: E402

BF16 = torch.bfloat16


def e4m3_rne_bytes(y):
    """RNE of fp64 values |y| <= 448 onto e4m3fn by search over the 127 finite magnitudes; a tie goes to the even byte; the sign bit is y's."""
    mags = torch.arange(0, 127, dtype=torch.uint8).view(torch.float8_e4m3fn).double()      # bytes 0x00 .. 0x7e, ascending
    a = y.abs().reshape(-1)
    hi = torch.searchsorted(mags, a).clamp(max=126)
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = a - mags[lo], mags[hi] - a
    pick = torch.where(dlo < dhi, lo, torch.where(dhi < dlo, hi, torch.where(lo % 2 == 0, lo, hi)))
    pick = torch.where(mags[hi] == a, hi, pick)
    sign = torch.signbit(y.reshape(-1)).to(torch.int64) * 128
    return (pick + sign).to(torch.uint8).reshape(y.shape)


def rows(n, Hkv, d, seed, mag=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, Hkv * d, generator=g) * mag).to(BF16)


def bf16_next_up(x):
    return (x.to(BF16).view(torch.int16) + 1).view(BF16)


@pytest.mark.parametrize("mag", [0.01, 1.0, 300.0])
@pytest.mark.parametrize("Hkv_d", [(2, 128), (4, 64), (16, 72)])
def test_quantize_kv8_is_the_contract(Hkv_d, mag):
    Hkv, d = Hkv_d
    x = rows(37, Hkv, d, seed=1, mag=mag)
    x[3] = 0                                                 # zero head-rows
    x[5, :d] = -0.0
    q, s = ops.quantize_kv8(x, Hkv, d)
    assert q.dtype == torch.uint8 and q.shape == x.shape and s.dtype == torch.float32 and s.shape == (37, Hkv)
    xs = x.double().view(37, Hkv, d)
    amax = xs.abs().amax(-1)
    # a power of two, admissible, and half of it is not
    m, _ = torch.frexp(s)
    assert torch.equal(m, torch.full_like(m, 0.5))
    assert bool((amax / s.double() <= 448).all()) and bool(((amax / (s.double() / 2) > 448) | (amax == 0)).all())
    assert torch.equal(s[3], torch.ones(Hkv)) and torch.equal(s[amax == 0], torch.ones(int((amax == 0).sum())))
    assert torch.equal(q.view(37, Hkv, d), e4m3_rne_bytes(xs / s.double()[..., None]))
    assert bool((q[5, :d] == 0x80).all()), "-0 keeps its sign"
    deq = ops.dequant_kv8(q, s, Hkv, d)
    exact = q.view(torch.float8_e4m3fn).double().view(37, Hkv, d) * s.double()[..., None]
    assert torch.equal(deq.double().view(37, Hkv, d), exact), "dequantised values are exactly bf16"
    normal = (xs / s.double()[..., None]).abs() >= 2.0 ** -6
    err = (xs - exact).abs()
    assert bool((err[normal] <= 2.0 ** -4 * xs.abs()[normal]).all())


def test_scale_boundaries_ties_and_subnormals():
    Hkv, d = 1, 16
    for k in (-9, 0, 5):
        on = torch.zeros(1, d, dtype=BF16)
        on[0, 3] = 448.0 * 2.0 ** k                          # amax exactly 448 * 2^k: scale 2^k, byte 0x7e
        on[0, 4] = -0.3 * 2.0 ** k
        q, s = ops.quantize_kv8(on, Hkv, d)
        assert float(s) == 2.0 ** k and int(q[0, 3]) == 0x7e
        up = on.clone()
        up[0, 3] = bf16_next_up(on[0, 3])                    # one bf16 ulp above: the next power of two
        q, s = ops.quantize_kv8(up, Hkv, d)
        assert float(s) == 2.0 ** (k + 1) and int(q[0, 3]) == 0x76   # 450 / 2 = 225 -> 224 = 0x76
    # exact half-way points between e4m3 neighbours, both parities, normals and subnormals (spacing 16 in [128, 256), 2 in [16, 32), 2^-9 below 2^-6)
    t = torch.zeros(1, d, dtype=BF16)
    t[0, 0] = 448.0                                          # pins the scale to 1
    vals = [136.0, 152.0, -168.0, 17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, -5 * 2.0 ** -10, 2.0 ** -11, 2.0 ** -6 + 2.0 ** -10, -0.0]
    for i, v in enumerate(vals):
        t[0, 1 + i] = v
    assert torch.equal(t.double()[0, 1:1 + len(vals)], torch.tensor(vals, dtype=torch.float64)), "the test values are bf16 values"
    q, s = ops.quantize_kv8(t, Hkv, d)
    assert float(s) == 1.0
    want = [0x70, 0x72, 0x80 | 0x72, 0x58, 0x5a, 0x00, 0x02, 0x80 | 0x02, 0x00, 0x08, 0x80]
    # 136 -> 128 (0x70, even), 152 -> 160 (0x72), -168 -> -160; 17 -> 16 (0x58), 19 -> 20 (0x5a); 2^-10 -> 0, 3 * 2^-10 -> 2^-8 (0x02),
    # -5 * 2^-10 -> -2^-8, 2^-11 -> 0, 2^-6 + 2^-10 -> 2^-6 (0x08, even)
    assert q[0, 1:1 + len(vals)].tolist() == want, (q[0, 1:1 + len(vals)].tolist(), want)
    assert torch.equal(q.view(1, 1, d), e4m3_rne_bytes(t.double().view(1, 1, d)))


def test_kvcache_formats():
    from metamorph_amd import functional as F
    for d, Hkv in ((128, 2), (64, 4)):
        a = F.KVCache(3, 40, Hkv * d, "cpu", d=d, batch=2)
        b = F.KVCache(3, 40, Hkv * d, "cpu", d=d, batch=2, fmt="fp8_e4m3")
        assert a.fmt == "bf16" and a.k.dtype == BF16 and a.kv8 is None
        assert b.k.dtype == torch.uint8 and b.k_scale.shape == (3, 2, 40, Hkv) and b.k_scale.dtype == torch.float32
        assert b.nbytes() * 2 * d == a.nbytes() * (d + 4), (a.nbytes(), b.nbytes())
    with pytest.raises(ValueError, match="fp4_e2m1"):
        F.KVCache(1, 8, 128, "cpu", d=128, fmt="fp4_e2m1")
