#!/usr/bin/env python3
"""Weight-only FP8 beyond 16 rows, in ONE process run (LLaMA-3-8B widths, random weights, a cache of 1024 rows): the captured decode step at
17 / 32 / 64 sequences and the one-sequence prompt pass at 128 / 512 / 1024 / 2048 rows, each three ways -- bf16 weights, quantised weights
on the scratch route (VARIANTS["w8_gemm"] off: what the model ran before mm355_gemm_w8*) and quantised weights on the w8 split-K GEMM --
and the per-launch time and weight GB/s of every projection shape at 17 ... 2048 rows, bf16 GEMM against the w8 GEMM against the scratch
route's dequantise + bf16 GEMM (beyond a projection's split limit the w8 kernel runs as one slice: that pair decides
W8_GEMM_UNSPLIT_MAX_ROWS).  REPS repetitions each: median
and spread.  The bf16 figures are taken first, then the same model is quantised in place.  Writes profiles/decode_w8_wide.json; the routing
constants of functional.py (W8_GEMM_MAX_ROWS, W8_GEMM_UNSPLIT_MAX_ROWS) and DESIGN.md section 7.1 are set from that file.
Environment: LAYERS (32), REPS (5), STEPS (24 steps per repetition), PASSES (8 prompt passes per repetition), LAUNCH_ONLY (1: only the
per-launch table), OUT."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from metamorph_amd import functional as F, ops
from metamorph_amd.factory import LLAMA3_8B, build_model

dev = torch.device("cuda:0")
LAYERS, REPS, STEPS, CACHE = int(os.environ.get("LAYERS", 32)), int(os.environ.get("REPS", 5)), int(os.environ.get("STEPS", 24)), 1024
PASSES = int(os.environ.get("PASSES", 8))                     # prompt passes per repetition (host-timed: enough of them to bury the sync)
h, I, V = 4096, 14336, LLAMA3_8B["vocab_size"]
SHAPES = {"qkv": (6144, h), "o": (h, h), "gate_up": (2 * I, h), "down": (h, I), "lm_head": (V, h)}
BATCHES, PROMPTS = (17, 32, 64), (128, 512, 1024, 2048)


def timed(fn, n):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def step_times(model, B):
    _, meta = model._decode_meta(CACHE)
    cap = CACHE + 8
    cos, sin = model.model.rope_tables(cap, dev)
    meta.cos, meta.sin = cos, sin
    kv = F.KVCache(len(model.model.layers), cap, meta.Hkv * meta.d, dev, Hq=meta.Hq, d=meta.d, batch=B)
    kv.k.normal_(0, 0.5); kv.v.normal_(0, 0.5)
    start = [CACHE - STEPS - 4 - 7 * b for b in range(B)]     # every timed step stays inside the 1024-row attention bound
    kv.set_lengths(start)
    st = F.DecodeStepGraph(model.model.layers, meta, kv, cos, sin, h, dev)
    rows = (torch.randn(B, h, device=dev) * 0.02).bfloat16()
    head = lambda x: model._rows_logits(x)
    for _ in range(3):
        head(st.step(rows))
    out = []
    for _ in range(REPS):
        kv.set_lengths(start)                                 # every repetition at the same cache lengths
        out.append(timed(lambda: head(st.step(rows)), STEPS) * 1e3)
    return dict(ms_per_step=statistics.median(out), reps=out, spread=max(out) - min(out), graph=st.graph is not None)


def prompt_ms(model, L):
    _, meta = model._decode_meta(L)
    cos, sin = model.model.rope_tables(L + 8, dev)
    meta.cos, meta.sin = cos, sin
    kv = F.KVCache(len(model.model.layers), L + 8, meta.Hkv * meta.d, dev, Hq=meta.Hq, d=meta.d)
    x = (torch.randn(L, h, device=dev) * 0.02).bfloat16()
    def run():
        kv.set_lengths([0]); F.decoder_prefill(x, model.model.layers, meta, kv)
    run(); run()
    ts = [timed(run, PASSES) * 1e3 for _ in range(REPS)]
    return dict(ms=statistics.median(ts), spread=max(ts) - min(ts))


def launch_times(M):
    """us per launch and GB/s of weight bytes for the plain projection three ways: the bf16 GEMM on bf16 weights (split-K GEMM + reduce where
    it splits, the plain kernel where not; the lm_head: fp32 logits), the w8 GEMM on the bytes, and the scratch route of a quantised model
    (mm355_dequant_w8_bf16 into one buffer, then the bf16 GEMM on it).  Weights rotated through > 600 MB of copies (the 256 MB last-level
    cache holds none of them)."""
    res = {}
    for name, (N, K) in SHAPES.items():
        x = (torch.randn(M, K, device=dev) * 0.05).bfloat16()
        f32 = name == "lm_head"
        out = torch.empty(M, N, device=dev, dtype=torch.float32 if f32 else torch.bfloat16)
        bf16_gemm = (lambda w: ops.gemm(x, w, out=out)) if f32 else (lambda w: ops.gemm_splitk(x, w, out=out))
        res[name] = dict(split=bool(ops.gemm_splitk_splits(M, N, K)))
        for kind in ("bf16", "w8", "w8_scratch"):
            nbytes = N * K * (2 if kind == "bf16" else 1)
            n = max(2, (600 << 20) // nbytes + 1)
            if kind == "bf16":
                ws = [(torch.randn(N, K, device=dev) * 0.02).bfloat16() for _ in range(n)]
                fns = [(lambda w=w: bf16_gemm(w)) for w in ws]
            else:
                ws = [torch.randint(0, 120, (N, K), device=dev, dtype=torch.uint8) for _ in range(n)]
                sc = torch.full((N,), 1e-3, device=dev)
                if kind == "w8":
                    fns = [(lambda w=w: ops.gemm_w8(x, w, sc, out=out)) for w in ws]
                else:
                    buf = torch.empty(N, K, device=dev, dtype=torch.bfloat16)
                    fns = [(lambda w=w: bf16_gemm(ops.dequant_w8(w, sc, out=buf))) for w in ws]
            def rnd():
                for f in fns:
                    f()
            rnd()
            ts = [timed(rnd, 3) / n * 1e6 for _ in range(REPS)]
            us = statistics.median(ts)
            res[name][kind] = dict(us=us, spread_us=max(ts) - min(ts), weight_GBps=nbytes / us / 1e3)
            del ws, fns
        r = res[name]
        r["w8_beats_scratch"] = r["w8_scratch"]["us"] - r["w8"]["us"] > max(r["w8"]["spread_us"], r["w8_scratch"]["spread_us"])
    return res


LAUNCH_ROWS = (17, 32, 64, 512, 1024, 2048)


def main():
    if os.environ.get("LAUNCH_ONLY") == "1":
        with torch.no_grad():
            print(json.dumps({str(M): launch_times(M) for M in LAUNCH_ROWS}, indent=1))
        return
    model = build_model(dict(LLAMA3_8B, num_hidden_layers=LAYERS), dict(num_hidden_layers=1), num_image_tokens=256, max_length=4096,
                        device=dev, init_on_device=True).eval()
    res = dict(layers=LAYERS, cache_rows=CACHE, reps=REPS, steps_per_rep=STEPS, device=torch.cuda.get_device_name(0), step={}, prompt={}, launch={})
    with torch.no_grad():
        for kind in ("bf16", "w8_scratch", "w8_gemm"):
            if kind == "w8_scratch":
                model.quantize_decoder_(lm_head=True)
                torch.cuda.empty_cache()
            old = F.set_variant("w8_gemm", kind != "w8_scratch")
            try:
                res["step"][kind] = {str(B): step_times(model, B) for B in BATCHES}
                res["prompt"][kind] = {str(L): prompt_ms(model, L) for L in PROMPTS}
            finally:
                F.set_variant("w8_gemm", old)
            print(kind, json.dumps(res["step"][kind]), json.dumps(res["prompt"][kind]), flush=True)
        del model
        torch.cuda.empty_cache()
        res["launch"] = {str(M): launch_times(M) for M in LAUNCH_ROWS}

    def verdict(table, key):
        out = {}
        for n in table["bf16"]:
            b, s, g = (table[k][n] for k in ("bf16", "w8_scratch", "w8_gemm"))
            sp = max(b["spread"], s["spread"], g["spread"])
            out[n] = dict(bf16_ms=b[key], w8_scratch_ms=s[key], w8_gemm_ms=g[key], spread_ms=sp,
                          w8_gemm_beats_scratch=s[key] - g[key] > sp, w8_gemm_beats_bf16=b[key] - g[key] > sp)
        return out
    res["verdict"] = dict(step=verdict(res["step"], "ms_per_step"), prompt=verdict(res["prompt"], "ms"))
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "decode_w8_wide.json"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["verdict"], indent=1))
    print(json.dumps(res["launch"], indent=1))


if __name__ == "__main__":
    main()
