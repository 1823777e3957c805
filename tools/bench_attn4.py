#!/usr/bin/env python3
"""attn4 (one wave per SIMD, hand-placed stream) against attn2 (the generic-d kernels, variant 2) and an fp32 reference:
correctness on the d == 128 cases of tests/test_kernels_gpu.py + full-size shapes, the serialised stream (variant 41) bit for bit
against the placed one (variant 4), then timings.   python tools/bench_attn4.py [--quick]"""
import os
import sys
import math

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from metamorph_amd import ops

DEV = "cuda"
BASE = 2                                                     # the comparison kernels: the generic attn2


def ref_attention(q, k, v, seqlens, causal):
    """q [B, L, Hq, d] etc. (float32 on the device) -> o [B, L, Hq, d], lse [B, Hq, L]"""
    B, L, Hq, d = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    o = torch.zeros_like(q)
    lse = torch.zeros(B, Hq, L, device=q.device)
    for b in range(B):
        n = seqlens[b] if seqlens else L
        for h in range(Hq):
            s = (q[b, :, h] @ k[b, :, h // rep].T) * d ** -0.5
            mask = torch.zeros(L, L, dtype=torch.bool, device=q.device)
            if causal:
                mask |= ~torch.ones(L, L, dtype=torch.bool, device=q.device).tril()
            mask[:, n:] = True
            s = s.masked_fill(mask, float("-inf"))
            lse[b, h] = torch.logsumexp(s, -1)
            o[b, :, h] = torch.softmax(s, -1) @ v[b, :, h // rep]
        o[b, n:] = 0
        lse[b, :, n:] = 0
    return o, lse


def run_case(B, L, Hq, Hkv, causal, seqlens, seed=0, full_ref=True):
    d = 128
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = (torch.randn(B * L, (Hq + 2 * Hkv) * d, generator=g) * 0.7).bfloat16().to(DEV)
    q2, k2, v2 = qkv[:, :Hq * d], qkv[:, Hq * d:(Hq + Hkv) * d], qkv[:, (Hq + Hkv) * d:]
    sl = torch.tensor(seqlens, dtype=torch.int32, device=DEV) if seqlens else None
    o2, l2 = ops.attn_fwd(q2, k2, v2, B, L, Hq, Hkv, d, d ** -0.5, causal, sl, variant=BASE)
    res = {}
    for var in (41, 4):
        o = torch.full((B * L, Hq * d), float("nan"), device=DEV, dtype=torch.bfloat16)
        o4, l4 = ops.attn_fwd(q2, k2, v2, B, L, Hq, Hkv, d, d ** -0.5, causal, sl, out=o, variant=var)
        torch.cuda.synchronize()
        res[var] = (o4.clone(), l4.clone())
    tag = f"B{B} L{L} H{Hq}/{Hkv} causal={int(causal)} seqlens={seqlens}"
    ok = True
    if full_ref:
        ro, rl = ref_attention(q2.float().view(B, L, Hq, d), k2.float().view(B, L, Hkv, d), v2.float().view(B, L, Hkv, d), seqlens, causal)
        ro = ro.reshape(B * L, Hq * d)
    for var, (o4, l4) in res.items():
        fin = bool(torch.isfinite(o4.float()).all()) and bool(torch.isfinite(l4).all())
        e2 = float((o4.float() - o2.float()).abs().max())
        el2 = float((l4 - l2).abs().max())
        msg = f"[{tag}] variant {var}: finite={fin} |o - o_attn2|max={e2:.3e} |lse - lse_attn2|max={el2:.3e}"
        if full_ref:
            er = float((o4.float() - ro).abs().max())
            e2r = float((o2.float() - ro).abs().max())
            elr = float((l4 - rl).abs().max())
            msg += f"  vs fp32: attn4 {er:.3e} (attn2 {e2r:.3e}) lse {elr:.3e}"
            good = fin and er <= max(2.0 * e2r, 1.5e-2) and elr <= 1e-2
        else:
            good = fin and e2 <= 3e-2 and el2 <= 1e-2
        print(msg + ("  OK" if good else "  **MISMATCH**"), flush=True)
        if not good:
            ok = False
            # localise: worst 64-row wave segment / head / column block
            diff = (o4.float() - (ro if full_ref else o2.float())).abs().view(B, L, Hq, d)
            diff = torch.nan_to_num(diff, nan=1e9)
            per_row = diff.amax(dim=(2, 3))                  # [B, L]
            seg = per_row.view(B, -1, min(64, L)) if L % 64 == 0 else None
            if seg is not None:
                print("   per-64-row segment max error (sample 0):", [f"{x:.1e}" for x in seg[0].amax(-1).tolist()][:40])
            per_col = diff.amax(dim=(0, 1, 2)).view(-1, 8).amax(-1)
            print("   per-8-column max error:", [f"{x:.1e}" for x in per_col.tolist()])
            per_head = diff.amax(dim=(0, 1, 3))
            print("   per-head max error:", [f"{x:.1e}" for x in per_head.tolist()])
            rr = int(per_row[0].argmax())
            print(f"   worst row of sample 0: {rr}; row values attn4 {o4.view(B, L, Hq, d)[0, rr, 0, :8].tolist()} ref {(ro if full_ref else o2.float()).view(B, L, Hq, d)[0, rr, 0, :8].tolist()}")
    same = torch.equal(res[4][0], res[41][0]) and torch.equal(res[4][1], res[41][1])
    print(f"[{tag}] placed stream == serialised stream bit for bit: {same}", flush=True)
    return ok and same


def timeit(fn, it=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / it


def bench(B, L, Hq, Hkv, causal=True, variants=(0, 4, 41)):
    d = 128
    qkv = (torch.randn(B * L, (Hq + 2 * Hkv) * d, device=DEV) * 0.5).bfloat16()
    q2, k2, v2 = qkv[:, :Hq * d], qkv[:, Hq * d:(Hq + Hkv) * d], qkv[:, (Hq + Hkv) * d:]
    fl = 4.0 * B * Hq * L * L * d / (2 if causal else 1)
    out = torch.empty((B * L, Hq * d), device=DEV, dtype=torch.bfloat16)
    for var in [BASE if v == 0 else v for v in variants]:
        ms = timeit(lambda: ops.attn_fwd(q2, k2, v2, B, L, Hq, Hkv, d, d ** -0.5, causal, None, out=out, variant=var))
        print(f"[bench B{B} L{L} H{Hq}/{Hkv} causal={int(causal)}] variant {var}: {ms:.3f} ms  {fl / ms / 1e9:.1f} TFLOP/s", flush=True)


if __name__ == "__main__":
    quick = "--quick" in sys.argv
    cases = [  # B, L, Hq, Hkv, causal, seqlens
        (1, 64, 2, 1, True, None),
        (1, 256, 2, 1, True, None),
        (2, 200, 4, 2, True, [200, 137]),
        (2, 333, 8, 2, True, [333, 256]),
        (1, 513, 4, 2, True, None),
        (2, 200, 2, 2, False, [200, 77]),
        (2, 256, 4, 1, True, [1, 256]),
        (1, 300, 6, 3, True, None),
        (2, 384, 12, 4, True, [300, 384]),
        (2, 320, 16, 2, True, [320, 191]),
        (1, 1024, 4, 2, True, None),
        (2, 2048, 8, 2, True, [2048, 1715]),
        (1, 2048, 4, 4, False, None),
    ]
    allok = True
    for c in cases:
        try:
            allok &= run_case(*c)
        except Exception as e:                               # keep going: the later cases localise the defect
            print(f"[{c}] EXCEPTION {type(e).__name__}: {e}", flush=True)
            allok = False
    print("ALL CASES OK" if allok else "SOME CASES FAILED", flush=True)
    # spiked scores: one key per sample far above the rest -> the rare rescale path runs mid-sequence
    torch.manual_seed(5)
    B, L, Hq, Hkv, d = 1, 1024, 4, 2, 128
    qkv = (torch.randn(B * L, (Hq + 2 * Hkv) * d) * 0.5)
    qkv[700, Hq * d:(Hq + Hkv) * d] *= 12.0                  # key 700 of both KV heads
    qkv = qkv.bfloat16().to(DEV)
    q2, k2, v2 = qkv[:, :Hq * d], qkv[:, Hq * d:(Hq + Hkv) * d], qkv[:, (Hq + Hkv) * d:]
    ro, rl = ref_attention(q2.float().view(B, L, Hq, d), k2.float().view(B, L, Hkv, d), v2.float().view(B, L, Hkv, d), None, True)
    for var in (BASE, 41, 4):
        o4, l4 = ops.attn_fwd(q2, k2, v2, B, L, Hq, Hkv, d, d ** -0.5, True, None, variant=var)
        print(f"[spike] variant {var}: |o - fp32|max={float((o4.float() - ro.reshape(B * L, -1)).abs().max()):.3e} lse {float((l4 - rl).abs().max()):.3e}", flush=True)
    if not quick:
        bench(4, 2048, 32, 8)
        bench(16, 2048, 32, 8)
        bench(16, 2048, 32, 8, variants=(0, 4))
        bench(8, 4096, 32, 8, variants=(0, 4))
        bench(16, 2048, 64, 8, causal=False, variants=(0, 4))
