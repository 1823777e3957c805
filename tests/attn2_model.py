"""Test infrastructure for the generic-head-size attention kernels (metamorph_amd/csrc/attn2.hip: every d != 128, and d == 128 as the
fallback of the stream kernels, variant 2):

  * attn2_forward_model -- a CPU model of the ARITHMETIC of attn2::fwd_kernel (what it computes and in which precision, not how it
    schedules it), with the number of deferred-rescale branches it takes per 16-row wave;
  * truth64 -- plain fp64 attention and its autograd, the truth every result is measured against;
  * check_forward / check_backward -- the bars tests/test_attn_generic_gpu.py holds the kernels to (the same as the d == 128 hostile-input
    tests): distance to the truth relative to the distance of the bf16 flash yardstick (attn4_model.flash_bf16_backward), which
    tests/test_attn2_model.py shows are strong enough to reject plausible kernel bugs.

The kernel's arithmetic, per (sample, query head), query block of 64 rows = 4 waves of 16 rows, key tile of 64 keys:
  * raw scores are fp32 sums of exact bf16 x bf16 products of q and k as stored; a masked key (kg >= seqlen, or causal kg > qg) is -inf
  * per row mx = fp32(max raw * c), c = fp32(fp32(scale) * fp32(log2 e)); a wave takes the branch when some row has mx > m + 6 (log2 units)
    or m = -inf < mx; then EVERY row of the wave sets m' = max(m, mx) and scales l and O by alpha = exp2(m - m') (0 when m was -inf)
  * p = exp2(fma(s, c, -m)); l sums the fp32 p, O accumulates bf16(p) V in fp32
  * o = bf16(O * fp32(1 / l)), lse = (m + log2 l) ln 2; both 0 for rows >= seqlen
  * rows >= seqlen inside a block that has valid rows still take part in their wave's decision (only keys are masked); rows >= L read q
    row L - 1; a causal block walks the key tiles below min(seqlen, q0 + 64), a wave skips a tile when kv0 > qw0 + 15.
"""
import torch

from attn4_model import sl2_of

THR = 6.0
WAVE = 16                                                       # query rows per wave (one rescale decision)
BLOCK = 64                                                      # query rows per workgroup
TILE = 64                                                       # keys per tile
LN2 = 0.6931471805599453


def attn2_forward_model(q, k, v, seqlens, causal, scale, rescale_o=True):
    """q [B, L, Hq, d], k / v [B, L, Hkv, d] bf16 (CPU); seqlens list[int] | None.  rescale_o=False: the branch scales l but not O (a
    deliberately broken kernel, for the checker-power tests).
    -> o [B, L, Hq, d] bf16, lse [B, Hq, L] fp32, counts int32 [B, Hq, ceil(L / 64) * 4] = branches taken after a wave's first tile."""
    B, L, Hq, d = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    nblk = (L + BLOCK - 1) // BLOCK
    Lp = nblk * BLOCK
    c = sl2_of(scale)
    c64 = float(c)
    ninf = float("-inf")
    rows = torch.arange(Lp)
    qrows = rows.clamp(max=L - 1)
    q0 = rows // BLOCK * BLOCK
    qw0 = rows // WAVE * WAVE
    o = torch.zeros(B, L, Hq, d, dtype=torch.bfloat16)
    lse = torch.zeros(B, Hq, L)
    counts = torch.zeros(B, Hq, Lp // WAVE, dtype=torch.int32)
    for b in range(B):
        seqlen = L if seqlens is None else min(int(seqlens[b]), L)
        if seqlen == 0:
            continue
        Q = q[b, qrows].float().permute(1, 0, 2)                          # [Hq, Lp, d]
        K = k[b].float().repeat_interleave(rep, 1).permute(1, 0, 2)      # [Hq, L, d]
        V = v[b].float().repeat_interleave(rep, 1).permute(1, 0, 2)
        kv_end = (q0 + BLOCK).clamp(max=seqlen) if causal else torch.full((Lp,), seqlen)
        ntiles = (kv_end + TILE - 1) // TILE                              # per row: the tiles its block walks
        in_block = q0 < seqlen
        m = torch.full((Hq, Lp), ninf)
        l = torch.zeros(Hq, Lp)
        O = torch.zeros(Hq, Lp, d)
        for t in range((seqlen + TILE - 1) // TILE):
            kv0 = t * TILE
            kg = kv0 + torch.arange(TILE)
            kc = kg.clamp(max=L - 1)
            s = Q @ K[:, kc].transpose(1, 2)                              # [Hq, Lp, 64] raw q . k
            vis = kg[None, :] < seqlen
            if causal:
                vis = vis & (kg[None, :] <= rows[:, None])
            s = s.masked_fill(~vis[None], ninf)
            act = in_block & (t < ntiles)                                 # [Lp]
            if causal:
                act = act & (kv0 <= qw0 + WAVE - 1)
            mx = s.max(dim=-1).values * c                                 # fp32 product
            grow = ((mx > m + THR) | (m == ninf)) & (mx > ninf)
            fire = grow.view(Hq, -1, WAVE).any(-1) & act.view(-1, WAVE)[:, 0][None]                   # [Hq, waves]
            if t > 0:
                counts[b] += fire.int()
            fr = fire.repeat_interleave(WAVE, 1)                          # [Hq, Lp]
            mn = torch.maximum(m, mx)
            alpha = torch.where(m == ninf, torch.zeros(()), torch.exp2(m - mn))
            alpha = torch.where(fr, alpha, torch.ones(()))
            l = l * alpha
            if rescale_o:
                O = O * alpha[..., None]
            m = torch.where(fr, mn, m)
            # p = exp2(fma(s, c, -m)): one rounding of the exact s * c - m (fp64 holds the product of two fp32 values exactly)
            arg = (s.double() * c64 - m.double()[..., None]).float()
            p = torch.where((m == ninf)[..., None], torch.zeros(()), torch.exp2(arg))
            l = torch.where(act[None], l + p.sum(-1), l)
            O = torch.where(act[None, :, None], O + p.to(torch.bfloat16).float() @ V[:, kc], O)
        valid = rows < seqlen
        inv = torch.where(valid[None] & (l > 0), 1.0 / l, torch.zeros(()))
        ob = (O * inv[..., None]).to(torch.bfloat16)                      # [Hq, Lp, d]
        o[b] = ob[:, :L].permute(1, 0, 2)
        lw = torch.where(valid[None], (m + torch.log2(l)) * LN2, torch.zeros(()))
        lse[b] = lw[:, :L]
    return o, lse, counts


# ------------------------------------------------------------------------------------------------ fp64 truth

def truth64(q, k, v, do, seqlens, causal, scale, drop_keys=None):
    """Plain fp64 attention over the valid keys of each sample (and its autograd when do is given).  drop_keys = a key range (lo, hi)
    left out of the softmax (the checker-power tests' "kernel that skipped a tile").  Rows / keys beyond a sample's length are 0.
    -> o, lse [B, Hq, L], dq, dk, dv: fp64 in the input layouts (the gradients None without do)."""
    B, L, Hq, d = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    f = torch.float64
    o = torch.zeros(B, L, Hq, d, dtype=f)
    lse = torch.zeros(B, Hq, L, dtype=f)
    grads = None if do is None else [torch.zeros(B, L, Hq, d, dtype=f), torch.zeros(B, L, Hkv, d, dtype=f), torch.zeros(B, L, Hkv, d, dtype=f)]
    for b in range(B):
        n = L if seqlens is None else min(int(seqlens[b]), L)
        if n == 0:
            continue
        Q, K, V = (x[b, :n].to(f).permute(1, 0, 2).requires_grad_(do is not None) for x in (q, k, v))
        with torch.set_grad_enabled(do is not None):
            s = (Q @ K.repeat_interleave(rep, 0).transpose(1, 2)) * scale
            vis = torch.ones(n, n, dtype=torch.bool)
            if causal:
                vis = vis.tril()
            if drop_keys is not None:
                vis[:, drop_keys[0]:drop_keys[1]] = False
            s = s.masked_fill(~vis[None], float("-inf"))
            lz = torch.logsumexp(s, -1)
            ob = torch.exp(s - lz[..., None]).nan_to_num(0.0) @ V.repeat_interleave(rep, 0)   # (a row with every key dropped: 0)
        o[b, :n] = ob.detach().permute(1, 0, 2)
        lse[b, :, :n] = lz.detach()
        if do is not None:
            (ob * do[b, :n].to(f).permute(1, 0, 2)).sum().backward()
            for g, x in zip(grads, (Q, K, V)):
                g[b, :n] = x.grad.permute(1, 0, 2)
    if do is None:
        return o, lse, None, None, None
    return (o, lse, *grads)


# ------------------------------------------------------------------------------------------------ the checkers

def valid_rows(B, L, seqlens):
    if seqlens is None:
        return torch.ones(B, L, dtype=torch.bool)
    return torch.arange(L)[None] < torch.tensor([min(int(n), L) for n in seqlens])[:, None]


def check_forward(o, lse, truth_o, truth_lse, yard_o, model_o, seqlens):
    """o [B, L, Hq, d], lse [B, Hq, L]: a kernel's (or a candidate's) result on the valid rows.  The bars of tests/test_attn_hostile_gpu.py:
      o   max error <= 1.5 x the yardstick's + 2e-3 |o|max, rms error <= 1.5 x the yardstick's + 2e-4 |o|max (against fp64);
      o   against the model of the kernel's own arithmetic <= 2^-6 max(1, |o|max);
      lse |error| <= 1e-4 (1 + |lse|) against fp64.
    -> (failures: list[str], errors: dict)"""
    B, L = o.shape[:2]
    vr = valid_rows(B, L, seqlens)
    if not bool(vr.any()):
        return [], {}
    t = truth_o[vr]
    omax = float(t.abs().max())
    e = o[vr].double() - t
    ey = yard_o[vr].double() - t
    err = dict(max=float(e.abs().max()), rms=float(e.pow(2).mean().sqrt()), y_max=float(ey.abs().max()), y_rms=float(ey.pow(2).mean().sqrt()),
               model=float((o[vr].double() - model_o[vr].double()).abs().max()), omax=omax)
    lv = vr[:, None, :].expand(B, lse.shape[1], L)
    err["lse"] = float(((lse[lv].double() - truth_lse[lv]).abs() / (1.0 + truth_lse[lv].abs())).max())
    bad = []
    if not err["max"] <= 1.5 * err["y_max"] + 2e-3 * omax:
        bad.append("o max error vs fp64")
    if not err["rms"] <= 1.5 * err["y_rms"] + 2e-4 * omax:
        bad.append("o rms error vs fp64")
    if not err["model"] <= 2.0 ** -6 * max(1.0, omax):
        bad.append("o vs the model of its own arithmetic")
    if not err["lse"] <= 1e-4:
        bad.append("lse vs fp64")
    return bad, err


def check_backward(grads, truth, yard):
    """grads / truth / yard = (dq, dk, dv).  Bars: relative-norm error <= 2 x the yardstick's + 3e-3, max error <= 3 x the yardstick's
    + 2^-7 |g|max, both against the fp64 truth.  -> (failures: list[str], errors: dict name -> (rel, rel_yard, max, max_yard, |g|max))"""
    bad, err = [], {}
    for name, x, t, y in zip(("dq", "dk", "dv"), grads, truth, yard):
        t = t.double()
        nrm = max(float(t.norm()), 1e-30)
        ex, ey = x.double() - t, y.double() - t
        rel, rel_y = float(ex.norm()) / nrm, float(ey.norm()) / nrm
        mx, mx_y, gmax = float(ex.abs().max()), float(ey.abs().max()), float(t.abs().max())
        err[name] = (rel, rel_y, mx, mx_y, gmax)
        if not rel <= 2.0 * rel_y + 3e-3:
            bad.append(f"{name} relative-norm error")
        if not mx <= 3.0 * mx_y + 2.0 ** -7 * gmax:
            bad.append(f"{name} max error")
    return bad, err
