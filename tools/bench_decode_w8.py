#!/usr/bin/env python3
"""Cached decode on bf16 weights against weight-only FP8 (quantize_decoder_) in ONE process run, LLaMA-3-8B widths, random weights, a cache
of 1024 rows: per-token time of the captured step at batch 1 / 4 / 8 / 16 (REPS repetitions each: median and spread), the per-launch times
of the five GEMV shapes (q|k|v, o, gate|up, down, lm_head) at 1 and 8 rows, and the prompt pass at 512 rows.  The bf16 figures are taken
first, then the same model is quantised in place.  Writes profiles/decode_w8.json."""
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


def launch_times(M, w8):
    """us per launch and GB/s of weight bytes, weights rotated through > 600 MB of copies (the 256 MB last-level cache holds none of them)"""
    res = {}
    for name, (N, K) in SHAPES.items():
        nbytes = N * K * (1 if w8 else 2)
        n = max(2, (600 << 20) // nbytes + 1)
        x = (torch.randn(M, K, device=dev) * 0.05).bfloat16()
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        if w8:
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


def prompt_ms(model, L=512):
    _, meta = model._decode_meta(L)
    cos, sin = model.model.rope_tables(L + 8, dev)
    meta.cos, meta.sin = cos, sin
    kv = F.KVCache(len(model.model.layers), L + 8, meta.Hkv * meta.d, dev, Hq=meta.Hq, d=meta.d)
    x = (torch.randn(L, h, device=dev) * 0.02).bfloat16()
    def run():
        kv.set_lengths([0]); F.decoder_prefill(x, model.model.layers, meta, kv)
    run(); run()
    ts = [timed(run, 2) * 1e3 for _ in range(REPS)]
    return dict(ms=statistics.median(ts), spread=max(ts) - min(ts))


def main():
    model = build_model(dict(LLAMA3_8B, num_hidden_layers=LAYERS), dict(num_hidden_layers=1), num_image_tokens=256, max_length=4096,
                        device=dev, init_on_device=True).eval()
    res = dict(layers=LAYERS, cache_rows=CACHE, reps=REPS, steps_per_rep=STEPS, device=torch.cuda.get_device_name(0), step={}, launch={}, prompt_512={})
    with torch.no_grad():
        for kind in ("bf16", "w8"):
            if kind == "w8":
                model.quantize_decoder_(lm_head=True)
                torch.cuda.empty_cache()
            res["step"][kind] = {str(B): step_times(model, B) for B in (1, 4, 8, 16)}
            res["prompt_512"][kind] = prompt_ms(model)
            res["launch"][kind] = {str(M): launch_times(M, kind == "w8") for M in (1, 8)}
            print(kind, json.dumps(res["step"][kind]), json.dumps(res["prompt_512"][kind]), flush=True)
    res["verdict"] = {B: dict(bf16_ms=res["step"]["bf16"][B]["ms_per_step"], w8_ms=res["step"]["w8"][B]["ms_per_step"],
                              bf16_spread_ms=res["step"]["bf16"][B]["spread"],
                              w8_faster_by_more_than_the_spread=res["step"]["bf16"][B]["ms_per_step"] - res["step"]["w8"][B]["ms_per_step"]
                              > res["step"]["bf16"][B]["spread"]) for B in ("1", "4", "8", "16")}
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "decode_w8.json"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["verdict"], indent=1))
    print(json.dumps(res["launch"], indent=1))


if __name__ == "__main__":
    main()
