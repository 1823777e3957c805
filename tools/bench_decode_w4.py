#!/usr/bin/env python3
"""Cached decode on bf16 weights, weight-only FP8 and weight-only MXFP4 (quantize_decoder_) in ONE process run, LLaMA-3-8B widths, random
weights, a cache of 1024 rows: per-token time of the captured step at batch 1 / 4 / 8 / 16 (REPS repetitions each: median and spread) and
the per-launch times and GB/s of the five GEMV shapes (q|k|v, o, gate|up, down, lm_head) at 1 and 8 rows, three ways.  A fresh model per
format (the lm_head stays bf16 in all three, as "mxfp4" requires).  Writes profiles/decode_w4.json."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from metamorph_amd import functional as F, ops
from metamorph_amd.factory import LLAMA3_8B, build_model

dev = torch.device("cuda:0")
LAYERS, REPS, STEPS, CACHE = int(os.environ.get("LAYERS", 32)), int(os.environ.get("REPS", 5)), int(os.environ.get("STEPS", 48)), 1024
h, I, V = 4096, 14336, LLAMA3_8B["vocab_size"]
SHAPES = {"qkv": (6144, h), "o": (h, h), "gate_up": (2 * I, h), "down": (h, I), "lm_head": (V, h)}


def timed(fn, n):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def step_times(model, B):
    _, meta = model._decode_meta(CACHE)
    cap = CACHE + (REPS + 1) * STEPS + 8
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
    kv.set_lengths(start)
    out = []
    for _ in range(REPS):
        kv.set_lengths(start)                                 # every repetition at the same cache lengths
        out.append(timed(lambda: head(st.step(rows)), STEPS) * 1e3)
    return dict(ms_per_step=statistics.median(out), reps=out, spread=max(out) - min(out), graph=st.graph is not None)


def launch_times(M, kind):
    """us per launch and GB/s of weight bytes, weights rotated through > 600 MB of copies (the 256 MB last-level cache holds none of them)"""
    res = {}
    for name, (N, K) in SHAPES.items():
        nbytes = {"bf16": N * K * 2, "w8": N * K + 4 * N, "w4": N * K // 2 + N * K // 32}[kind]
        n = max(2, (600 << 20) // nbytes + 1)
        x = (torch.randn(M, K, device=dev) * 0.05).bfloat16()
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        if kind == "w4":
            ws = [torch.randint(0, 256, (N, K // 2), device=dev, dtype=torch.uint8) for _ in range(n)]
            sc = torch.randint(115, 122, (N, K // 32), device=dev, dtype=torch.uint8)
            fns = [(lambda w=w: ops.gemv_w4(x, w, sc, out=out)) for w in ws]
        elif kind == "w8":
            ws = [torch.randint(0, 120, (N, K), device=dev, dtype=torch.uint8) for _ in range(n)]
            sc = torch.full((N,), 1e-3, device=dev)
            fns = [(lambda w=w: ops.gemv_w8(x, w, sc, out=out)) for w in ws]
        else:
            ws = [(torch.randn(N, K, device=dev) * 0.02).bfloat16() for _ in range(n)]
            fns = [(lambda w=w: ops.gemv(x, w, out=out)) for w in ws]
        def rnd():
            for f in fns:
                f()
        rnd()
        ts = [timed(rnd, 3) / n * 1e6 for _ in range(REPS)]
        us = statistics.median(ts)
        res[name] = dict(us=us, spread_us=max(ts) - min(ts), weight_GBps=nbytes / us / 1e3)
        del ws, fns
    return res


def main():
    res = dict(layers=LAYERS, cache_rows=CACHE, reps=REPS, steps_per_rep=STEPS, device=torch.cuda.get_device_name(0), step={}, launch={})
    with torch.no_grad():
        for kind, fmt in (("bf16", None), ("w8", "fp8_e4m3"), ("w4", "mxfp4")):
            model = build_model(dict(LLAMA3_8B, num_hidden_layers=LAYERS), dict(num_hidden_layers=1), num_image_tokens=256, max_length=4096,
                                device=dev, init_on_device=True).eval()
            if fmt is not None:
                model.quantize_decoder_(fmt=fmt)
                torch.cuda.empty_cache()
            res["step"][kind] = {str(B): step_times(model, B) for B in (1, 4, 8, 16)}
            del model
            torch.cuda.empty_cache()
            res["launch"][kind] = {str(M): launch_times(M, kind) for M in (1, 8)}
            print(kind, json.dumps(res["step"][kind]), flush=True)
    res["verdict"] = {}
    for B in ("1", "4", "8", "16"):
        st = {k: res["step"][k][B] for k in ("bf16", "w8", "w4")}
        spread = max(st["w8"]["spread"], st["w4"]["spread"])
        res["verdict"][B] = dict(bf16_ms=st["bf16"]["ms_per_step"], w8_ms=st["w8"]["ms_per_step"], w4_ms=st["w4"]["ms_per_step"],
                                 larger_spread_ms=spread, w4_faster_than_w8_by_more_than_the_spread=st["w8"]["ms_per_step"] - st["w4"]["ms_per_step"] > spread)
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "decode_w4.json"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["verdict"], indent=1))
    print(json.dumps(res["launch"], indent=1))


if __name__ == "__main__":
    main()
