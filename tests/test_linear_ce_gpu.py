"""The fused lm_head cross entropy (mm355_linear_ce in metamorph_amd/csrc/linear_ce.hip, reached through ops.linear_ce and
functional.LinearCrossEntropyFn) at the shapes the training step runs it: h = 4096, V = 128 258 (Vp = 128 384), ~28 000 target rows in four
8192-row chunks, fp32 dW accumulated over the chunks.  Needs an MI355X:  pytest -m gpu

  * truth: the same operation on the same bf16 inputs with no intermediate rounding -- fp32 logits, log-softmax, mean NLL,
    dh = dlogits . W and dW = dlogits^T . x -- through torch's fp32 GEMMs on the device (TF32 off; hipBLASLt / rocBLAS, nothing of
    libmm355), chunked.  That truth is anchored to fp64 on the host at ~48 sampled rows (first / last row of every chunk, rows 8191 / 8192):
    their full-width logits, NLL and dh rows, and a few whole dW rows (the last 2-row M tile 128 256 / 128 257 and target rows);
  * yardstick: the reference stack's own arithmetic (metamorph_llama.py:393-413): bf16 nn.Linear logits, `.float()` cross entropy
    averaged over the target rows, its gradient cast back to bf16 by the backward of `.float()`, bf16 GEMMs for dh and dW (one GEMM over
    all n rows, as autograd runs it);
  * bars: for loss, dh and dW the kernel's error against the truth is at most C x the yardstick's error + a floor, per metric: relative
    Frobenius norm, max-abs, and the worst row (dh rows; dW vocabulary rows) relative to its own norm plus 1e-3 of the median row norm
    (rows whose gradient cancels to ~0 -- a target on a dominant logit -- carry only rounding noise).  C and the floors are BARS below:
    1.5 x the largest ratio measured over every geometry here on the first MI355X run, rounded up (this project's convention).  The
    fp32 dW of a multi-chunk call is more accurate than the yardstick's bf16 dW, so its measured ratio sits well below 1;
  * sensitivity: inside the bench-shape test the same bars are applied to corrupted copies of the truth -- dW without the last chunk,
    loss / gradients normalised by 1/8192 instead of 1/n, one dh row of the last chunk zeroed -- and must reject every one of them;
  * contract: outputs pre-filled with NaN and the workspace with 0xFF bytes (a NaN in bf16 and fp32) give the bits of a zero-filled
    workspace (every padding column of W^T, dyT and xT is written before a GEMM reads it), two calls give the same bits, the loss-only
    call gives the training call's loss, and a single-chunk bf16 dW is the fp32 dW rounded to bf16;
  * the autograd function the model calls, with the bench's uploaded plan: an upstream gradient of 0.25, hidden.grad exactly 0 off the
    target rows, weight.grad accumulated into a prior gradient, and a stale NaN `_mm_grad_buf` overwritten rather than added to.
"""
import math
import os
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

DEV = "cuda"
BF16 = torch.bfloat16
CHUNK = 8192
H, V_LLAMA3 = 4096, 128258

# quantity -> metric -> (C, floor); error(kernel) <= C * error(yardstick) + floor.  Every error is relative: the loss error to |loss|,
# "fro" / "row" to the truth's norms, "max" to max |truth|.  Measured kernel / yardstick ratios on the first MI355X run, over every geometry:
#   loss  1.00-1.15 where the yardstick is above 1e-6 (2.6 once, at 1.2e-7 vs 4.7e-8: summation-order noise, inside the floor);
#   dh    1.00 on every metric (the kernel and the yardstick round the same bf16 gradient and the same bf16 GEMM output);
#   dW    1.00 for a one-chunk bf16 dW; 0.09-0.76 (fro), 0.09-0.44 (max), 0.92-1.00 (row) for the fp32 dW accumulated over chunks.
# C = 1.5 x the largest ratio; the floors are 1.5 x the largest error the ratio does not cover (loss) or a decade under the smallest
# yardstick error measured (dh, dW), so they cannot hide a gross error.
BARS = {
    "loss": {"abs": (1.5, 2e-7)},
    "dh": {"fro": (1.5, 1e-4), "max": (1.5, 2e-4), "row": (1.5, 2e-4)},
    "dw": {"fro": (1.5, 1e-4), "max": (1.5, 2e-4), "row": (1.5, 2e-4)},
}


@pytest.fixture(scope="module")
def ops():
    from metamorph_amd import ops as _ops
    from metamorph_amd import lib
    lib.load()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield _ops
    print(f"\n   [linear_ce] file {time.time() - t0:.1f} s, peak device memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ inputs

def _bench_plan():
    """the bench step's batch (bench.make_batch(16, 2048, 256), rank 0, pool slot 0) through the model's own splice plan"""
    import bench
    from metamorph_amd.splice_plan import build_splice_plan
    ids, lab, msk, _ = bench.make_batch(16, 2048, 256, "cpu", seed=1234)
    return build_splice_plan(ids.numpy(), lab.numpy(), msk.numpy(), 16, 256, 4096, "right", vocab_size=V_LLAMA3)


def _weights(V, h, seed, hot=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    W = torch.randn(V, h, device=DEV, generator=g) * 0.02          # logits ~ N(0, 1.3^2) for unit hidden rows at h = 4096
    if hot:
        # trained-head-like: class k of 32 owns hidden coordinate k (set to 8 in its rows, see _hidden); column DOM[k] has weight 7 there
        # (logit ~ +56, one dominant column per row), column ANTI[k] has -3 (logit ~ -24): NLL ~ 0 on DOM, ~ 80 on ANTI
        W[:, :32] = 0.0
        for k in range(32):
            W[_dom(V, k), k], W[_anti(V, k), k] = 7.0, -3.0
    return W.to(BF16)


def _dom(V, k):
    return 1000 + 37 * k


def _anti(V, k):
    return V - 3 - 41 * k


def _hidden(M, h, seed, ldh=None, hot=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    base = torch.randn(M, ldh or h, device=DEV, generator=g)
    if hot:
        base[:, :32] = 0.0
        base[torch.arange(M, device=DEV), torch.arange(M, device=DEV) % 32] = 8.0
    return base.to(BF16)[:, :h]


def _targets(n, V, seed, hot=False, rows=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.randint(0, V, (n,), device=DEV, generator=g)
    t[0], t[-1] = V - 1, V - 2                                       # the last 2-row M tile of the dW GEMM carries target rows
    if hot:
        src = torch.arange(n, device=DEV) if rows is None else rows.long()
        k = src % 32
        third = torch.arange(n, device=DEV) % 3
        dom = torch.tensor([_dom(V, i) for i in range(32)], device=DEV)[k]
        anti = torch.tensor([_anti(V, i) for i in range(32)], device=DEV)[k]
        t = torch.where(third == 0, dom, torch.where(third == 1, anti, t))
    return t.to(torch.int32)


# ------------------------------------------------------------------------------------------------ truth, yardstick, anchor

def _truth(x, W, tgt, sub=4096):
    """fp32 on the device, no intermediate rounding: per-row NLL / lse, loss (fp64 sum), dh [n, h] f32, dW [V, h] f32 and the last
    8192-row chunk's share of dW (for the missing-chunk self-check)"""
    n, h = x.shape
    V = W.shape[0]
    Wf = W.float()
    nll = torch.empty(n, device=DEV, dtype=torch.float32)
    lse = torch.empty(n, device=DEV, dtype=torch.float32)
    dh = torch.empty(n, h, device=DEV, dtype=torch.float32)
    dW = torch.zeros(V, h, device=DEV, dtype=torch.float32)
    dW_last = torch.zeros(V, h, device=DEV, dtype=torch.float32)
    last0 = (n - 1) // CHUNK * CHUNK
    bounds = sorted(set(list(range(0, n, sub)) + [last0, n]))
    for a, b in zip(bounds[:-1], bounds[1:]):
        xf = x[a:b].float()
        t = tgt[a:b].long()
        z = xf @ Wf.t()
        m = z.max(dim=1).values
        l = m + torch.log(torch.exp(z - m[:, None]).sum(dim=1))
        lse[a:b] = l
        zt = z.gather(1, t[:, None])[:, 0]
        nll[a:b] = l - zt
        p = z.sub_(l[:, None]).exp_()
        p.scatter_(1, t[:, None], 0.0)
        # d/dz_t = p_t - 1 = -(sum of the other p): no cancellation on rows whose target dominates
        p.scatter_(1, t[:, None], -p.sum(dim=1, keepdim=True))
        p.mul_(1.0 / n)
        dh[a:b] = p @ Wf
        (dW_last if a >= last0 else dW).addmm_(p.t(), xf)
        del z, p, xf
    dW.add_(dW_last)
    loss = float(nll.double().sum() / n)
    del Wf
    return dict(loss=loss, nll=nll, lse=lse, dh=dh, dw=dW, dw_last=dW_last)


def _yardstick(x, W, tgt, sub=4096):
    """the reference's arithmetic: bf16 logits, .float() CE mean, gradient rounded to bf16, bf16 GEMMs for dh and dW (one GEMM over n)"""
    n, h = x.shape
    V = W.shape[0]
    dl = torch.empty(n, V, device=DEV, dtype=BF16)
    nll = torch.empty(n, device=DEV, dtype=torch.float32)
    for a in range(0, n, sub):
        b = min(n, a + sub)
        lf = torch.nn.functional.linear(x[a:b], W).float()
        t = tgt[a:b].long()
        ls = torch.log_softmax(lf, dim=1)
        nll[a:b] = -ls.gather(1, t[:, None])[:, 0]
        g = ls.exp_()
        g.scatter_add_(1, t[:, None], -torch.ones(b - a, 1, device=DEV))
        dl[a:b] = (g * (1.0 / n)).to(BF16)
        del lf, ls, g
    loss = float(nll.mean())
    dh = dl @ W
    dW = dl.t() @ x
    del dl
    return dict(loss=loss, dh=dh, dw=dW)


def _anchor_rows(n):
    pick = {0, n - 1, n // 2, n // 3}
    for a in range(0, n, CHUNK):
        pick |= {a, min(n, a + CHUNK) - 1}
    if n > CHUNK:
        pick |= {CHUNK - 2, CHUNK - 1, CHUNK, CHUNK + 1}
    g = np.random.default_rng(n)
    while len(pick) < min(48, n):
        pick.add(int(g.integers(0, n)))
    return sorted(pick)


def _anchor(x, W, tgt, tr, vocab_rows, tol=1e-4):
    """fp64 on the host at sampled rows: logits, NLL and dh rows; and whole dW rows at `vocab_rows` (with the truth's lse per row)"""
    n, h = x.shape
    V = W.shape[0]
    rows = _anchor_rows(n)
    ri = torch.tensor(rows, device=DEV)
    xs = x[ri].double().cpu()
    ts = tgt[ri].long().cpu()
    Wh = W.cpu()
    z = torch.empty(len(rows), V, dtype=torch.float64)
    blk = 16384
    for v0 in range(0, V, blk):
        z[:, v0:v0 + blk] = xs @ Wh[v0:v0 + blk].double().t()
    lse = torch.logsumexp(z, dim=1)
    nll = lse - z.gather(1, ts[:, None])[:, 0]
    p = torch.exp(z - lse[:, None])
    p.scatter_(1, ts[:, None], 0.0)
    p.scatter_(1, ts[:, None], -p.sum(dim=1, keepdim=True))
    p /= n
    dh = torch.zeros(len(rows), h, dtype=torch.float64)
    for v0 in range(0, V, blk):
        dh += p[:, v0:v0 + blk] @ Wh[v0:v0 + blk].double()
    assert torch.allclose(tr["nll"][ri].double().cpu(), nll, rtol=0, atol=2e-5 * (1 + float(nll.abs().max()))), "fp32 truth NLL vs fp64"
    e = (tr["dh"][ri].double().cpu() - dh).norm(dim=1) / dh.norm(dim=1).clamp_min(1e-300)
    assert float(e.max()) < tol, ("fp32 truth dh rows vs fp64", float(e.max()))
    assert abs(tr["loss"] - float(tr["nll"].double().mean())) < 1e-9
    # dW rows: dW[v] = sum_r (p_rv - [t_r = v]) / n * x_r, p_rv from the fp64 logit column and the truth's (fp32) lse
    xd = x.double()
    Wv = W[vocab_rows].double()
    zc = xd @ Wv.t()                                                    # [n, k]
    pc = torch.exp(zc - tr["lse"].double()[:, None])
    pc -= (tgt.long()[:, None] == torch.tensor(vocab_rows, device=DEV)[None, :]).double()
    dwr = (pc.t() @ xd) / n
    e = (tr["dw"][vocab_rows].double() - dwr).norm(dim=1) / dwr.norm(dim=1)
    assert float(e.max()) < tol, ("fp32 truth dW rows vs fp64", vocab_rows, e.tolist())
    del xd, zc, pc


# ------------------------------------------------------------------------------------------------ metrics and bars

def _rownorms(a, block=8192):
    """row norms summed in fp64: the gradient rows of columns far below a dominant logit hold values ~1e-29, whose squares underflow fp32"""
    return torch.cat([a[i:i + block].double().norm(dim=1) for i in range(0, a.shape[0], block)])


def _metrics(got, truth):
    """(relative Frobenius, max-abs / max|truth|, worst row relative to its norm + 1e-3 x the median row norm)"""
    d = got.float() - truth
    dn, tn = _rownorms(d), _rownorms(truth)
    row = (dn / (tn + 1e-3 * tn.median())).max()
    return {"fro": float(dn.norm() / tn.norm()), "max": float(d.abs().max() / truth.abs().max()), "row": float(row)}


def _judge(got, yard, tr):
    """{quantity: {metric: (error, yardstick error, bar)}} and the list of metrics over their bars"""
    out, bad = {}, []
    for q in ("loss", "dh", "dw"):
        if got.get(q) is None:
            continue
        if q == "loss":
            e = {"abs": abs(got[q] - tr[q]) / abs(tr[q])}
            y = {"abs": abs(yard[q] - tr[q]) / abs(tr[q])}
        else:
            e, y = _metrics(got[q], tr[q]), _metrics(yard[q], tr[q])
        out[q] = {}
        for k, (c, floor) in BARS[q].items():
            bar = c * y[k] + floor
            out[q][k] = (e[k], y[k], bar)
            if not e[k] <= bar:
                bad.append(f"{q}.{k}: {e[k]:.3e} > {bar:.3e} (yardstick {y[k]:.3e})")
    return out, bad


def _report(name, res):
    parts = []
    for q, d in res.items():
        parts.append(q + " " + " ".join(f"{k} {e:.2e}/{y:.2e} (x{e / y if y > 0 else float('inf'):.2f})" for k, (e, y, _) in d.items()))
    print(f"\n   [{name}] kernel/yardstick: " + " | ".join(parts))


def _dw_rows(V, tgt):
    t = tgt.long().cpu()
    return sorted({V - 2, V - 1, 0, int(t[1]), int(t[len(t) // 2]), V // 2})


# ------------------------------------------------------------------------------------------------ geometries

def _run_case(ops, name, hidden, rows, tgt, W, anchor=False, selfcheck=False, anchor_tol=1e-4):
    n = tgt.numel()
    x = hidden[rows.long()] if rows is not None else hidden[:n]
    x = x.contiguous()
    loss, dh, dw = ops.linear_ce(hidden, rows, tgt, W)
    assert dw.dtype == (torch.float32 if n > CHUNK else BF16)
    got = {"loss": float(loss), "dh": dh, "dw": dw}
    assert math.isfinite(got["loss"]) and bool(torch.isfinite(dh).all()) and bool(torch.isfinite(dw).all())
    tr = _truth(x, W, tgt)
    if anchor:
        _anchor(x, W, tgt, tr, _dw_rows(W.shape[0], tgt), anchor_tol)
    yard = _yardstick(x, W, tgt)
    res, bad = _judge(got, yard, tr)
    _report(name, res)
    # the rows the issue names: the last, 2-row M tile of the dW GEMM and target rows, against the same per-row bar
    vr = _dw_rows(W.shape[0], tgt)
    tn = _rownorms(tr["dw"][vr])
    e = _rownorms(dw[vr].float() - tr["dw"][vr]) / tn
    ey = _rownorms(yard["dw"][vr].float() - tr["dw"][vr]) / tn
    c, floor = BARS["dw"]["row"]
    assert bool((e <= c * ey.max() + floor).all()), ("dW named rows", vr, e.tolist(), ey.tolist())
    assert not bad, (name, bad)
    if selfcheck:
        _selfcheck(tr, yard, n)
    del tr, yard, got, dh, dw, x
    _free()


def _selfcheck(tr, yard, n):
    """the bars must reject a missing chunk, a wrong normaliser and a zeroed row -- built from the truth itself"""
    assert n > CHUNK and n % CHUNK
    no_last = {"loss": tr["loss"], "dh": tr["dh"], "dw": tr["dw"] - tr["dw_last"]}
    assert any(b.startswith("dw.") for b in _judge(no_last, yard, tr)[1]), "bars pass dW without the last chunk"
    s = n / CHUNK
    wrong = {"loss": tr["loss"] * s, "dh": tr["dh"] * s, "dw": tr["dw"] * s}
    bad = _judge(wrong, yard, tr)[1]
    for q in ("loss", "dh", "dw"):
        assert any(b.startswith(q + ".") for b in bad), f"bars pass {q} normalised by 1/8192 instead of 1/n"
    dh0 = tr["dh"].clone()
    dh0[(n - 1) // CHUNK * CHUNK + 7] = 0.0
    assert any(b.startswith("dh.") for b in _judge({"loss": tr["loss"], "dh": dh0}, yard, tr)[1]), "bars pass a zeroed dh row"
    del no_last, wrong, dh0


def test_linear_ce_bench_shape(ops):
    """the bench step's own rows / targets (n = 27 992: chunks 8192 x 3 + 3416, rp = 3456), anchored to fp64, with the self-checks"""
    plan = _bench_plan()
    M = plan.B * plan.L
    assert M == 16 * 2048 and plan.n_valid > 3 * CHUNK
    hidden = _hidden(M, H, seed=11)
    W = _weights(V_LLAMA3, H, seed=12)
    rows = torch.from_numpy(plan.ce_rows.astype(np.int32)).to(DEV)
    tgt = torch.from_numpy(plan.shift_targets[plan.ce_rows].astype(np.int32)).to(DEV)
    _run_case(ops, f"bench n={plan.n_valid}", hidden, rows, tgt, W, anchor=True, selfcheck=True)


# name, last-chunk rows or n, V, h
EDGES = [
    ("last1-rp8", CHUNK + 1, V_LLAMA3, H),
    ("last511-rp512", CHUNK + 511, V_LLAMA3, H),
    ("last512", CHUNK + 512, V_LLAMA3, H),
    ("last513-rp640", CHUNK + 513, V_LLAMA3, H),
    ("one-chunk-bf16dw", CHUNK, V_LLAMA3, H),
    ("three-chunks", 3 * CHUNK, V_LLAMA3, H),
    ("V128256-no-pad", CHUNK + 300, 128256, H),
    ("tinyllama-V32002", 3 * CHUNK + 100, 32002, 2048),
]


@pytest.mark.parametrize("name,n,V,h", EDGES, ids=[e[0] for e in EDGES])
def test_linear_ce_chunk_and_padding_edges(ops, name, n, V, h):
    M = n + n // 7
    hidden = _hidden(M, h, seed=n)
    W = _weights(V, h, seed=V + h)
    g = torch.Generator(device=DEV).manual_seed(n + 1)
    rows = torch.randperm(M, device=DEV, generator=g)[:n].sort().values.to(torch.int32)
    tgt = _targets(n, V, seed=n + 2)
    _run_case(ops, name, hidden, rows, tgt, W)


def test_linear_ce_trained_head_logits(ops):
    """|z| up to ~60-80, one dominant column per row; a third of the targets on it (NLL ~ 0, p - 1 cancels), a third on a column at
    z ~ -24 (NLL ~ 80); two chunks with a 1000-row tail; anchored to fp64"""
    n = CHUNK + 1000
    M = n + 500
    hidden = _hidden(M, H, seed=21, hot=True)
    W = _weights(V_LLAMA3, H, seed=22, hot=True)
    rows = torch.arange(0, M, device=DEV)[torch.randperm(M, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))[:n]]
    rows = rows.sort().values.to(torch.int32)
    tgt = _targets(n, V_LLAMA3, seed=23, hot=True, rows=rows)
    x = hidden[rows.long()].float()
    z = x[:64] @ W.float().t()
    assert float(z.max()) > 40 and float(z.min()) < -15, (float(z.max()), float(z.min()))
    del x, z
    # the fp32 truth's logits carry ~1e-4 absolute error here (an fp32 accumulator at |z| ~ 56 rounds each of the 4096 products at
    # ulp(56)), so its dh / dW rows sit up to ~2e-4 from fp64 (measured 1.8e-4): still ~1000 x closer than the bf16 logits (ulp 0.25)
    _run_case(ops, "trained-head", hidden, rows, tgt, W, anchor=True, anchor_tol=5e-4)


def test_linear_ce_strided_hidden_first_rows(ops):
    """a hidden view with ldh > h and rows=None (the first n rows): no gather, the GEMMs read the strided view directly"""
    n = 2 * CHUNK + 77
    hidden = _hidden(n + 40, H, seed=31, ldh=H + 64)
    assert hidden.stride(0) == H + 64
    W = _weights(V_LLAMA3, H, seed=32)
    tgt = _targets(n, V_LLAMA3, seed=33)
    _run_case(ops, "strided-no-rows", hidden, None, tgt, W)


# ------------------------------------------------------------------------------------------------ contract and bits

def _raw(ops, hidden, rows, tgt, W, need_dh=True, need_dw=True, dw_f32=None, ws_byte=0):
    """mm355_linear_ce with NaN-filled outputs and a workspace filled with `ws_byte`"""
    L = ops._L()
    ph, _, h, ldh = ops._rows2d(hidden)
    pw, V, _, ldw = ops._rows2d(W)
    n = tgt.numel()
    if dw_f32 is None:
        dw_f32 = n > CHUNK
    nan = float("nan")
    loss = torch.full((1,), nan, device=DEV)
    dh = torch.full((n, h), nan, device=DEV, dtype=BF16) if need_dh else None
    dw = torch.full((V, h), nan, device=DEV, dtype=torch.float32 if dw_f32 else BF16) if need_dw else None
    nb = int(L.mm355_linear_ce_ws_bytes(n, V, h, int(rows is not None), int(need_dh), int(need_dw)))
    ws = torch.full((nb,), ws_byte, device=DEV, dtype=torch.uint8)
    rc = L.mm355_linear_ce(ph, ldh, ops._p(rows), tgt.data_ptr(), n, pw, ldw, V, h, loss.data_ptr(), ops._p(dh), ops._p(dw), int(dw_f32),
                           ws.data_ptr(), nb, ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    del ws
    return loss, dh, dw


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("n", [CHUNK + 1, CHUNK + 513, 300], ids=["last1-rp8", "last513-rp640", "single-rp304"])
def test_linear_ce_poisoned_workspace(ops, n):
    """workspace all 0xFF (bf16 / fp32 NaN), outputs NaN: finite results, bit-identical to a zero-filled workspace"""
    M = n + 64
    hidden = _hidden(M, H, seed=41 + n)
    W = _weights(V_LLAMA3, H, seed=42)
    rows = torch.arange(3, 3 + n, device=DEV, dtype=torch.int32)
    tgt = _targets(n, V_LLAMA3, seed=43)
    for r in (rows, None):
        a = _raw(ops, hidden, r, tgt, W, ws_byte=0xFF)
        b = _raw(ops, hidden, r, tgt, W, ws_byte=0)
        for name, u, v in zip(("loss", "dh", "dw"), a, b):
            assert bool(torch.isfinite(u).all()), (name, n, r is None)
            assert _same_bits(u, v), (name, n, r is None)
        la = _raw(ops, hidden, r, tgt, W, need_dh=False, need_dw=False, ws_byte=0xFF)[0]
        assert _same_bits(la, a[0]), ("loss-only call", n)
        del a, b
    _free()


def test_linear_ce_bits_reproducible_and_eval_call(ops):
    """bench shape: two calls give the same loss / dh / dW bits; the loss-only (evaluation) call gives the training call's loss bits"""
    plan = _bench_plan()
    hidden = _hidden(plan.B * plan.L, H, seed=51)
    W = _weights(V_LLAMA3, H, seed=52)
    rows = torch.from_numpy(plan.ce_rows.astype(np.int32)).to(DEV)
    tgt = torch.from_numpy(plan.shift_targets[plan.ce_rows].astype(np.int32)).to(DEV)
    a = ops.linear_ce(hidden, rows, tgt, W)
    b = ops.linear_ce(hidden, rows, tgt, W)
    for name, u, v in zip(("loss", "dh", "dw"), a, b):
        assert _same_bits(u, v), name
    del b
    ev = ops.linear_ce(hidden, rows, tgt, W, need_dh=False, need_dw=False)
    assert ev[1] is None and ev[2] is None
    assert _same_bits(ev[0], a[0])
    del a
    _free()


@pytest.mark.parametrize("n", [CHUNK, 513, 40], ids=["8192", "513-rp640", "40"])
def test_linear_ce_bf16_dw_is_rounded_f32_dw(ops, n):
    """one chunk: the bf16 dW is the fp32 dW rounded to bf16 (same GEMM, only the epilogue's store differs); loss / dh unchanged"""
    hidden = _hidden(n, H, seed=61 + n)
    W = _weights(V_LLAMA3, H, seed=62)
    tgt = _targets(n, V_LLAMA3, seed=63)
    l16, dh16, dw16 = ops.linear_ce(hidden, None, tgt, W, dw_f32=False)
    l32, dh32, dw32 = ops.linear_ce(hidden, None, tgt, W, dw_f32=True)
    assert dw16.dtype == BF16 and dw32.dtype == torch.float32
    assert _same_bits(l16, l32) and _same_bits(dh16, dh32)
    r = dw32.to(BF16)
    diff = int((dw16.view(torch.int16) != r.view(torch.int16)).sum())
    assert diff == 0, f"{diff} of {dw16.numel()} bf16 dW elements differ from the rounded fp32 dW"
    _free()


# ------------------------------------------------------------------------------------------------ the autograd function

def test_linear_ce_autograd_function_bench_plan(ops):
    """functional.LinearCrossEntropyFn with the bench plan through metamorph_arch.upload_plan, an upstream gradient of 0.25:
    hidden.grad is 0.25 x the kernel's dh on ce_rows (a power of two: exact) and exactly 0 elsewhere, and within the bars of the truth;
    weight.grad accumulates onto a prior gradient; a stale NaN `_mm_grad_buf` is overwritten"""
    from metamorph_amd import functional as F
    from metamorph_amd.model.metamorph_arch import upload_plan
    plan = _bench_plan()
    M = plan.B * plan.L
    pd = upload_plan(plan, DEV)
    torch.cuda.synchronize()
    rows, tgt = pd["ce_rows"], pd["ce_targets"]
    n = plan.n_valid
    assert torch.equal(tgt.cpu(), torch.from_numpy(plan.shift_targets[plan.ce_rows].astype(np.int32)))
    hidden = _hidden(M, H, seed=71).clone().requires_grad_(True)
    head = torch.nn.Linear(H, V_LLAMA3, bias=False, device=DEV, dtype=BF16)
    with torch.no_grad():
        head.weight.copy_(_weights(V_LLAMA3, H, seed=72))
    W = head.weight
    ref_loss, ref_dh, ref_dw = ops.linear_ce(hidden.detach(), rows, tgt, W.detach())
    x = hidden.detach()[rows.long()].contiguous()
    tr = _truth(x, W.detach(), tgt)
    yard = _yardstick(x, W.detach(), tgt)
    del x
    c, floor = BARS["dw"]["max"]
    dw_tol = c * _metrics(yard["dw"], tr["dw"])["max"] + floor                     # relative to max |dW|
    dw_max = float(tr["dw"].abs().max())

    # (1) upstream 0.25, weight.grad already present: the accumulate branch of grad_target
    prior = (torch.randn(W.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(73)) * float(tr["dw"].std())).to(BF16)
    W.grad = prior.clone()
    loss = F.LinearCrossEntropyFn.apply(hidden, W, head, pd, n)
    assert _same_bits(loss.reshape(1), ref_loss)
    (0.25 * loss).backward()
    torch.cuda.synchronize()
    g = hidden.grad
    off = torch.ones(M, dtype=torch.bool, device=DEV)
    off[rows.long()] = False
    assert int(off.sum()) == M - n and bool((g[off] == 0).all()) and not bool(torch.signbit(g[off]).any())
    assert _same_bits(g[rows.long()], (ref_dh.float() * 0.25).to(BF16))
    res, bad = _judge({"dh": g[rows.long()].float() * 4.0}, yard, tr)
    assert not bad, bad
    want = prior.float() + 0.25 * tr["dw"]
    err = (W.grad.float() - want).abs()
    assert bool((err <= 0.25 * dw_tol * dw_max + 2.0 ** -8 * want.abs()).all()), float((err - 2.0 ** -8 * want.abs()).max())
    del want, err, prior

    # (2) no .grad, a stale NaN _mm_grad_buf: the buffer becomes .grad and is overwritten
    hidden.grad = None
    W.grad = None
    W._mm_grad_buf = torch.full_like(W.data, float("nan"))
    buf_ptr = W._mm_grad_buf.data_ptr()
    loss = F.LinearCrossEntropyFn.apply(hidden, W, head, pd, n)
    (0.25 * loss).backward()
    torch.cuda.synchronize()
    assert W.grad is not None and W.grad.data_ptr() == buf_ptr
    assert bool(torch.isfinite(W.grad).all())
    assert _same_bits(W.grad, (ref_dw * 0.25).to(BF16)) or bool(
        ((W.grad.float() - 0.25 * tr["dw"]).abs() <= 0.25 * dw_tol * dw_max + 2.0 ** -8 * 0.25 * tr["dw"].abs()).all())
    del tr, yard, ref_dh, ref_dw, hidden, head, W
    _free()
