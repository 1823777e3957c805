"""Inputs and fp64 formulas for the long-context tests of the KV-cache kernels (tests/test_kv_long_context_gpu.py; checked on the CPU by
tests/test_kv_long_refs_host.py).  Pure torch on the CPU.

On random data an attention output over 131072 keys is ~ 0.7 / sqrt(n) ~ 0.002, far below what the suite's usual 1e-2 bounds see, so the
inputs here are built to make a long-context mistake visible:

  * the first NCH = 8 columns of every query / key head are BIAS CHANNELS: a query is 8.0 in ONE of them (query head h of a decode step:
    channel h % 8; query row i of an extend chunk: channel i % 8) and 0 in the others, a key carries bias / (d^-0.5 * 8) there, so the score
    of a key is its bias in the query's channel plus a real dot product over the other columns (N(0, 0.5^2) in bf16);
  * "flat": no bias; V holds segment indicators, v[j, c] = 1 iff j // ceil(kv_len / d) == c: output column c is the softmax mass of one
    contiguous 1 / d of the keys (~ 1 / d), every term non-negative, so the comparison is purely relative;
  * "needle": one key per channel at +40; V holds the key's index in binary, v[j, c] = bit c of j (c < 17) and v[j, d / 2 + c] = 1 - bit c
    (d = 128: column 64 + c), so an output row spells the index of the key that was actually read;
  * "beyond" (extend forms): key past + j, j = 1 .. 7, carries the needle of row j - 1 (channel (j - 1) % 8), which that row must not see
    (row 0 gives the no-needle answer), and of row j, whose own position it is.

The reference is the contract formula in fp64, softmax(q k^T d^-0.5 over the visible keys) v, per (sequence, KV head) on the same bf16 (or
dequantised e4m3) values.  Accepted: |got - ref| <= 2^-7 |ref| + 2^-20.  On the flat inputs all terms are non-negative, so the errors -- one
bf16 rounding of the output (2^-8), the bf16 rounding of P in the MFMA forms (2^-9 per term, not amplified), fp32 scores and exp (~1e-5 at
|s| <= 45) -- do not cancel into something larger; 2^-7 is about twice their sum.  2^-20 lies 2^13 below the flat outputs and only admits
the ~1e-12 leakage onto the zero bits of a needle row."""
import math

import torch

BF16 = torch.bfloat16
NCH = 8                                                      # bias channels: columns 0 .. 7 of a head
NEEDLE = 40.0
REL, ABS = 2.0 ** -7, 2.0 ** -20


# ------------------------------------------------------------------------------------------------ the acceptance threshold

def measure(got, ref):
    """(largest error as a fraction of the bar 2^-7 |ref| + 2^-20, largest relative error over the entries with |ref| >= 2^-12)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf")
    err = (got - ref).abs()
    big = ref.abs() >= 2.0 ** -12
    rel = float((err[big] / ref.abs()[big]).max()) if bool(big.any()) else 0.0
    return float((err / (REL * ref.abs() + ABS)).max()) if err.numel() else 0.0, rel


def accept(got, ref, what):
    """assert the threshold; prints and returns the measured largest relative error"""
    frac, rel = measure(got, ref)
    print(f"   {what}: max rel err {rel:.3e}, {frac:.3f} of the bar")
    assert frac <= 1.0, f"{what}: {frac:.2f} x the bar 2^-7 |ref| + 2^-20 (max rel err {rel:.3e})"
    return rel


# ------------------------------------------------------------------------------------------------ the library's key runs, restated

def key_runs(nwg, ktiles):
    """attn_tile::key_runs: ktiles 64-key tiles dealt to nsplit workgroups in contiguous runs of tps tiles -> (nsplit, tps)"""
    ns = 1
    if nwg < 128:
        ns = min(max(1, ktiles // 4), (256 + nwg - 1) // nwg)
    ns = min(ns, 64)
    tps = -(-ktiles // ns)
    return -(-ktiles // tps), tps


def extend_runs(B, n, Hq, Hkv, bound):
    """mm355_attn_extend's plan -> (nsplit, tps, row tiles)"""
    nqt = (n * (Hq // Hkv) + 63) // 64
    return key_runs(B * Hkv * nqt, (bound + 63) // 64) + (nqt,)


def shared_runs(B, n, Hq, Hkv, shared_len):
    """mm355_attn_extend_shared's plan over the shared rows (n = 1: the decode step) -> (nsplit, tps, row tiles)"""
    nqt = (B * n * (Hq // Hkv) + 63) // 64
    return key_runs(Hkv * nqt, (shared_len + 63) // 64) + (nqt,)


def pick_dp(d):
    return 64 if d <= 64 else (96 if d <= 96 else 128)


# ------------------------------------------------------------------------------------------------ the formula and its mutations

def attend64(q, k, v, limits, scale, mutate=None):
    """q [R, d], k / v [m, d], limits int64 [R]: row r sees the keys j <= limits[r] (-1: none, a zero row) -> fp64 [R, d].
    mutate (name, arg) is one of the mistakes the threshold has to reject (test_kv_long_refs_host.py):
      ("drop_tile", t) / ("double_tile", t)  the keys [64 t, 64 t + 64) left out / counted twice
      ("limit", +-1)                         every key limit off by one
      ("shift_v", +-1)                       key j reads the V row j +- 1
      ("no_rescale", j0)                     the partials of the runs [0, j0) and [j0, m) added without rescaling to a common maximum"""
    q, k, v = q.double(), k.double(), v.double()
    m = k.shape[0]
    name, arg = mutate if mutate else (None, None)
    lim = limits.clone().long()
    if m == 0:
        return torch.zeros(q.shape[0], v.shape[1], dtype=torch.float64)
    s = (q @ k.t()) * scale
    if name == "limit":
        lim = (lim + arg).clamp(max=m - 1)
    elif name == "drop_tile":
        s[:, 64 * arg:64 * arg + 64] = float("-inf")
    elif name == "double_tile":
        s[:, 64 * arg:64 * arg + 64] += math.log(2.0)
    elif name == "shift_v":
        v = torch.roll(v, -arg, 0)
    s.masked_fill_(torch.arange(m)[None, :] > lim[:, None], float("-inf"))
    runs = ((0, arg), (arg, m)) if name == "no_rescale" else ((0, m),)
    o = torch.zeros(q.shape[0], v.shape[1], dtype=torch.float64)
    l = torch.zeros(q.shape[0], 1, dtype=torch.float64)
    common = s.amax(1, keepdim=True)
    for lo, hi in runs:
        if hi <= lo:
            continue
        mx = s[:, lo:hi].amax(1, keepdim=True) if name == "no_rescale" else common
        mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
        p = torch.exp(s[:, lo:hi] - mx)
        o += p @ v[lo:hi]
        l += p.sum(1, keepdim=True)
    return torch.where(l > 0, o / l.clamp(min=1e-300), torch.zeros_like(o))


def emulate_bf16p(q, k, v, limits, scale, mutate=None):
    """The arithmetic of the MFMA forms: fp32 scores, P rounded to bf16 in front of the PV product, fp32 sums (the denominator from the
    unrounded P), one bf16 rounding of the output -> fp64 of that bf16 result"""
    assert mutate is None
    m = k.shape[0]
    if m == 0:
        return torch.zeros(q.shape[0], v.shape[1], dtype=torch.float64)
    s = (q.float() @ k.float().t()) * scale
    s.masked_fill_(torch.arange(m)[None, :] > limits[:, None], float("-inf"))
    mx = s.amax(1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    p = torch.exp(s - mx)
    l = p.sum(1, keepdim=True)
    o = p.bfloat16().float() @ v.float()
    return torch.where(l > 0, o / l.clamp(min=1e-30), torch.zeros_like(o)).bfloat16().double()


def decode_ref(q, k, v, lens, Hq, Hkv, d, fn=attend64, mutate=None):
    """q [B, Hq d], k / v [B, rows, Hkv d], lens[b] cached rows -> fp64 [B, Hq d], per (sequence, KV head).  (Two rows beyond lens[b] are
    handed to fn where the cache has them: only a mutated key limit looks at them.)"""
    B, G = q.shape[0], Hq // Hkv
    out = torch.zeros(B, Hq * d, dtype=torch.float64)
    for b in range(B):
        L = int(lens[b])
        m = min(L + 2, k.shape[1]) if mutate else L
        for hk in range(Hkv):
            qq = q[b].view(Hq, d)[hk * G:(hk + 1) * G]
            r = fn(qq, k[b, :m, hk * d:(hk + 1) * d], v[b, :m, hk * d:(hk + 1) * d], torch.full((G,), L - 1), d ** -0.5, mutate=mutate)
            out[b].view(Hq, d)[hk * G:(hk + 1) * G] = r
    return out


def extend_ref(q, k, v, past, ns, Hq, Hkv, d, fn=attend64, mutate=None, shared=None):
    """Sequence b brings ns[b] rows (an int: the same number each), packed in q [sum ns, Hq d] in order; row (b, i) sees the keys j <= past[b] +
    i of k / v [B, rows, Hkv d] -> fp64 [sum ns, Hq d].  shared = (k_shared, v_shared, S): the keys [0, S) come from those rows [S, Hkv d]
    instead (the shared-prefix forms; with ns = 1 and past = kv_lens - 1 their decode step)."""
    B, G = len(past), Hq // Hkv
    ns = [ns] * B if isinstance(ns, int) else list(ns)
    out = torch.zeros(q.shape[0], Hq * d, dtype=torch.float64)
    r0 = 0
    for b in range(B):
        n, p = ns[b], int(past[b])
        if n == 0:
            continue
        m = min(p + n + (2 if mutate else 0), k.shape[1])
        lim = (p + torch.arange(n)).repeat_interleave(G)
        for hk in range(Hkv):
            cs = slice(hk * d, (hk + 1) * d)
            kk, vv = k[b, :m, cs], v[b, :m, cs]
            if shared is not None:
                ksh, vsh, S = shared
                kk, vv = torch.cat([ksh[:S, cs], kk[S:]]), torch.cat([vsh[:S, cs], vv[S:]])
            qq = q[r0:r0 + n].view(n, Hq, d)[:, hk * G:(hk + 1) * G].reshape(n * G, d)
            r = fn(qq, kk, vv, lim, d ** -0.5, mutate=mutate)
            out[r0:r0 + n].view(n, Hq, d)[:, hk * G:(hk + 1) * G] = r.view(n, G, d)
        r0 += n
    return out


# ------------------------------------------------------------------------------------------------ input builders

_BASE = {}


def base_rows(B, rows, W, seed):
    """N(0, 0.5^2) in bf16, [B, rows, W]; made once per shape and seed and never written to"""
    key = (B, rows, W, seed)
    if key not in _BASE:
        _BASE[key] = (torch.randn(B, rows, W, generator=torch.Generator().manual_seed(seed)) * 0.5).bfloat16()
    return _BASE[key]


def key_unit(d):
    """the key value that is one unit of bias against a query of 8.0"""
    return 1.0 / (d ** -0.5 * 8.0)


def queries(R, Hq, d, channel, seed):
    """[R, Hq d]: N(0, 0.5^2) outside the bias channels; row r, head h is 8.0 in channel channel(r, h) and 0 in the other seven"""
    q = (torch.randn(R, Hq, d, generator=torch.Generator().manual_seed(seed)) * 0.5).bfloat16()
    q[..., :NCH] = 0
    for r in range(R):
        for h in range(Hq):
            q[r, h, channel(r, h) % NCH] = 8.0
    return q.view(R, Hq * d)


def keys_with(base, Hkv, d, needles):
    """a copy of base [B, rows, Hkv d] with the bias channels of every head zero except needles: (b, key, channel) at +NEEDLE"""
    k = base.clone()
    kv = k.view(k.shape[0], k.shape[1], Hkv, d)
    kv[..., :NCH] = 0
    for b, j, c in needles:
        kv[b, j, :, c % NCH] = NEEDLE * key_unit(d)
    return k


def v_segments(lens, rows, Hkv, d):
    """flat: v[b, j, c] = 1 iff j // ceil(lens[b] / d) == c, for every head"""
    v = torch.zeros(len(lens), rows, Hkv, d, dtype=BF16)
    j = torch.arange(rows)
    for b, L in enumerate(lens):
        seg = max(1, -(-int(L) // d))
        v[b] = (j[:, None] // seg == torch.arange(d)[None, :]).to(BF16)[:, None, :]
    return v.view(len(lens), rows, Hkv * d)


def v_bits(B, rows, Hkv, d):
    """needle: v[j, c] = bit c of j for c < 17, v[j, d / 2 + c] = 1 - bit c, the other columns 0, for every sequence and head"""
    assert d // 2 + 17 <= d and d // 2 >= 17
    j = torch.arange(rows)
    bits = ((j[:, None] >> torch.arange(17)[None, :]) & 1).to(BF16)
    v = torch.zeros(rows, d, dtype=BF16)
    v[:, :17] = bits
    v[:, d // 2:d // 2 + 17] = 1 - bits
    return v[None, :, None, :].expand(B, rows, Hkv, d).reshape(B, rows, Hkv * d).contiguous()


def spelled(row, d):
    """the key index an output row of the needle inputs spells (its first 17 columns rounded to bits)"""
    return int(sum(1 << c for c in range(17) if float(row[c]) > 0.5))


def decode_needle_keys(L):
    """0, 255, 256, 1023, 1024, the first key of the last 1024-group, the last key, and the middle one: one per channel, inside [0, L)"""
    return [min(p, L - 1) for p in (0, 255, 256, 1023, 1024, (L - 1) // 1024 * 1024, L - 1, L // 2)]


def decode_inputs(kind, lens, rows, Hq, Hkv, d, shift=0, seed=1):
    """(q [B, Hq d], k, v [B, rows, Hkv d]) of a decode step over lens[b] cached rows; query head h uses channel (h + shift) % 8"""
    B = len(lens)
    base = base_rows(B, rows, Hkv * d, seed)
    q = queries(B, Hq, d, lambda r, h: h + shift, seed + 100)
    if kind == "flat":
        return q, keys_with(base, Hkv, d, []), v_segments(lens, rows, Hkv, d)
    assert kind == "needle"
    needles = [(b, j, c) for b, L in enumerate(lens) if L > 0 for c, j in enumerate(decode_needle_keys(L))]
    return q, keys_with(base, Hkv, d, needles), v_bits(B, rows, Hkv, d)


def extend_needle_keys(past, n, nsplit, tps):
    """63, 64, the last key of run 0, the first key of run 1 and of the last run, and three rows' own positions (of rows 5, 14 and 7: row 6,
    which shares row 14's channel, does not see that one): one per channel, inside [0, past + n)"""
    return [min(p, past + n - 1) for p in (63, 64, tps * 64 - 1, tps * 64, (nsplit - 1) * tps * 64, past + 5, past + 14, past + 7)]


def extend_inputs(kind, past, n, rows, Hq, Hkv, d, runs, seed=2):
    """(q [B n, Hq d], k, v [B, rows, Hkv d]) of n new rows per sequence at past[b] ..; query row i uses channel i % 8; runs = (nsplit, tps)"""
    B = len(past)
    base = base_rows(B, rows, Hkv * d, seed)
    q = queries(B * n, Hq, d, lambda r, h: r % n, seed + 100)
    if kind == "flat":
        return q, keys_with(base, Hkv, d, []), v_segments([p + n for p in past], rows, Hkv, d)
    if kind == "needle":
        needles = [(b, j, c) for b, p in enumerate(past) for c, j in enumerate(extend_needle_keys(p, n, *runs))]
    else:
        assert kind == "beyond" and n >= 9
        needles = [(b, p + j, c) for b, p in enumerate(past) for j in range(1, 8) for c in (j - 1, j)]
    return q, keys_with(base, Hkv, d, needles), v_bits(B, rows, Hkv, d)


def shared_needle_keys(S, last, nsplit, tps):
    """63, the last key of run 0, the first key of run 1 and of the last run, the last shared row, the first own row, the sequence's last
    key and the middle of the prefix: one per channel, inside [0, last]"""
    return [min(p, last) for p in (63, tps * 64 - 1, tps * 64, (nsplit - 1) * tps * 64, S - 1, S, last, S // 2)]


def shared_inputs(kind, S, past, n, rows, Hq, Hkv, d, runs, seed=3):
    """A prefix of S rows stored once and the own rows [S, past[b] + n) of every sequence: (q [B n, Hq d], k_shared, v_shared [S, Hkv d], k, v
    [B, rows, Hkv d] whose rows [0, S) are NaN: they are never read).  Head h of query row r = b n + i uses channel 3 r + h.  The needles of the
    shared part (channels 0 .. 4 and 7) are the same for every sequence; those of the own part (channels 5 and 6) sit at S and at past[b] + n
    - 1 where the sequence has such rows, and a sequence without them gives the no-needle answer there."""
    B = len(past)
    last = [p + n - 1 for p in past]
    sh = base_rows(1, S, Hkv * d, seed)
    own = base_rows(B, rows - S, Hkv * d, seed + 1)
    q = queries(B * n, Hq, d, lambda r, h: 3 * r + h, seed + 100)
    if kind == "flat":
        full_v = v_segments([max(last) + 1], rows, Hkv, d)[0]                     # one segment map, over the longest sequence
        ksh, kown = keys_with(sh, Hkv, d, [])[0], keys_with(own, Hkv, d, [])
    else:
        assert kind == "needle"
        pos = shared_needle_keys(S, S - 1, *runs)
        ksh = keys_with(sh, Hkv, d, [(0, j, c) for c, j in enumerate(pos) if c not in (5, 6)])[0]
        kown = keys_with(own, Hkv, d, [(b, j, c) for b in range(B) if last[b] >= S for j, c in ((0, 5), (last[b] - S, 6))])
        full_v = v_bits(1, rows, Hkv, d)[0]
    vsh, vown = full_v[:S].contiguous(), full_v[S:][None].expand(B, rows - S, Hkv * d).contiguous()
    nan = torch.full((B, S, Hkv * d), float("nan"), dtype=BF16)
    return q, ksh.contiguous(), vsh, torch.cat([nan, kown], 1), torch.cat([nan, vown], 1)


def poison_(lens, *caches):
    """the rows the contract says are never read: NaN from lens[b] on (in place)"""
    for t in caches:
        for b, L in enumerate(lens):
            t[b, L:] = float("nan")


def quantize_rows_kv8(x, Hkv, d, seed):
    """tests/test_kv8_gpu.py's cache recipe on GIVEN rows x [..., Hkv d] bf16: a power-of-two scale per key and head drawn over 2^-6 .. 2^6
    (raised where the head-row's largest value would otherwise exceed 448, so that no needle saturates), the bytes e4m3(x / scale)
    -> (uint8 [..., Hkv d], f32 scales [..., Hkv])"""
    xs = x.float().reshape(*x.shape[:-1], Hkv, d)
    e = torch.randint(-6, 7, xs.shape[:-1], generator=torch.Generator().manual_seed(seed))
    m, ex = torch.frexp(xs.abs().amax(-1))                   # amax = m 2^ex, m < 1: amax / 2^(ex - 8) < 256
    e = torch.maximum(e, (ex - 8).to(e.dtype))
    s = torch.ldexp(torch.ones(e.shape), e)
    y = (xs / s[..., None]).clamp(-448, 448)
    return y.to(torch.float8_e4m3fn).view(torch.uint8).reshape(x.shape).contiguous(), s.contiguous()


# ------------------------------------------------------------------------------------------------ RoPE

def rope_table_ref(rows, inv_freq, scaling):
    """HF's table rows: the fp32 product float32(l) * inv_freq[j] (its 1-term fp32 matmul), cos / sin of it in fp64, times the scaling,
    rounded once to bf16; both halves of a row -> (cos, sin) bf16 [len(rows), 2 len(inv_freq)]"""
    ang = (rows.float()[:, None] * torch.as_tensor(inv_freq, dtype=torch.float32)[None, :]).double()
    c, s = (torch.cos(ang) * scaling).to(BF16), (torch.sin(ang) * scaling).to(BF16)
    return torch.cat([c, c], 1), torch.cat([s, s], 1)


def hf_rope_rows(x, cos, sin, d):
    """HF's x * cos + rotate_half(x) * sin on bf16 tensors (each product rounded to bf16, then the sum): x [M, H d], cos / sin [M, d]"""
    M = x.shape[0]
    xv, c, s = x.view(M, -1, d), cos.view(M, 1, d), sin.view(M, 1, d)
    rot = torch.cat([-xv[..., d // 2:], xv[..., :d // 2]], -1)
    return (xv * c + rot * s).reshape(M, -1)


def bf16_steps(a, b):
    """distance of two bf16 tensors in steps of the bf16 grid (ordered-integer distance)"""
    def ordered(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (ordered(a) - ordered(b)).abs()
