#!/usr/bin/env python3
"""Weight-only MXFP4 beyond 16 rows, in ONE process run (LLaMA-3-8B widths, random weights, a cache of 1024 rows): the captured decode step
at 17 / 32 / 64 sequences and the one-sequence prompt pass at 128 / 512 rows, each four ways -- bf16 weights, "mxfp4" weights on the scratch
route (VARIANTS["w4_gemm"] off: what the model ran before mm355_gemm_w4*), "mxfp4" weights on the w4 split-K GEMM, and "fp8_e4m3" weights on
the w8 split-K GEMM (decoder layers only: the lm_head is bf16 in all four and is left out) -- and the per-launch time and weight GB/s of
the four projection shapes at 17 rows: the bf16 split-K GEMM, the scratch route's dequantise + bf16 GEMM, the w4 GEMM and the w8 GEMM, the
weights rotated through more than 600 MB.  REPS repetitions each: median and spread.  The w4 row caps are forced to 4096 (split) / 0
(unsplit) for the run, whatever functional.py holds, so that the tool measures the routes it names.  Writes profiles/decode_w4_wide.json;
W4_GEMM_MAX_ROWS of functional.py and DESIGN.md section 7.1 are set from that file: an entry stays above 0 only where the GEMM is ahead of
the scratch route of the same run by more than the larger spread.
Environment: LAYERS (8), REPS (5), STEPS (24 steps per repetition), PASSES (8 prompt passes per repetition), LAUNCH_ONLY (1: only the
per-launch table), OUT."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from metamorph_amd import functional as F, ops
from metamorph_amd.factory import LLAMA3_8B, build_model

dev = torch.device("cuda:0")
LAYERS, REPS, STEPS, CACHE = int(os.environ.get("LAYERS", 8)), int(os.environ.get("REPS", 5)), int(os.environ.get("STEPS", 24)), 1024
PASSES = max(8, int(os.environ.get("PASSES", 8)))             # prompt passes per repetition (host-timed: enough of them to bury the sync)
h, I = 4096, 14336
SHAPES = {"qkv": (6144, h), "o": (h, h), "gate_up": (2 * I, h), "down": (h, I)}
BATCHES, PROMPTS, LAUNCH_ROWS = (17, 32, 64), (128, 512), (17,)
KINDS = ("bf16", "w4_scratch", "w4_gemm", "w8_gemm")


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
    for _ in range(3):
        st.step(rows)
    out = []
    for _ in range(REPS):
        kv.set_lengths(start)                                 # every repetition at the same cache lengths
        out.append(timed(lambda: st.step(rows), STEPS) * 1e3)
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
    return dict(ms=statistics.median(ts), reps=ts, spread=max(ts) - min(ts))


def launch_times(M):
    """us per launch and GB/s of weight bytes for the plain projection four ways: the bf16 split-K GEMM on bf16 weights, the scratch route of
    a 4-bit model (mm355_dequant_w4_bf16 into one buffer, then the bf16 split-K GEMM on it), the w4 GEMM on the nibbles and the w8 GEMM on
    e4m3 bytes.  Weights rotated through > 600 MB of copies (the 256 MB last-level cache holds none of them)."""
    res = {}
    for name, (N, K) in SHAPES.items():
        x = (torch.randn(M, K, device=dev) * 0.05).bfloat16()
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        res[name] = dict(split=bool(ops.gemm_splitk_splits(M, N, K)))
        for kind in ("bf16", "w4_scratch", "w4", "w8"):
            nbytes = N * K * 2 if kind == "bf16" else (N * K if kind == "w8" else N * K // 2 + N * K // 32)
            n = max(2, (600 << 20) // nbytes + 1)
            if kind == "bf16":
                ws = [(torch.randn(N, K, device=dev) * 0.02).bfloat16() for _ in range(n)]
                fns = [(lambda w=w: ops.gemm_splitk(x, w, out=out)) for w in ws]
            elif kind == "w8":
                ws = [torch.randint(0, 120, (N, K), device=dev, dtype=torch.uint8) for _ in range(n)]
                sc = torch.full((N,), 1e-3, device=dev)
                fns = [(lambda w=w: ops.gemm_w8(x, w, sc, out=out)) for w in ws]
            else:
                ws = [(torch.randint(0, 256, (N, K // 2), device=dev, dtype=torch.uint8),
                       torch.randint(110, 125, (N, K // 32), device=dev, dtype=torch.uint8)) for _ in range(n)]
                if kind == "w4":
                    fns = [(lambda w=w: ops.gemm_w4(x, *w, out=out)) for w in ws]
                else:
                    buf = torch.empty(N, K, device=dev, dtype=torch.bfloat16)
                    fns = [(lambda w=w: ops.gemm_splitk(x, ops.dequant_w4(*w, out=buf), out=out)) for w in ws]
            def rnd():
                for f in fns:
                    f()
            rnd()
            ts = [timed(rnd, 3) / n * 1e6 for _ in range(REPS)]
            us = statistics.median(ts)
            res[name][kind] = dict(us=us, spread_us=max(ts) - min(ts), weight_GBps=nbytes / us / 1e3)
            del ws, fns
        r = res[name]
        sp = max(r["w4"]["spread_us"], r["w4_scratch"]["spread_us"])
        r["w4_against_scratch"] = position(r["w4_scratch"]["us"] - r["w4"]["us"], sp)
        r["w4_against_w8"] = position(r["w8"]["us"] - r["w4"]["us"], max(r["w4"]["spread_us"], r["w8"]["spread_us"]))
    return res


def position(gain, spread):
    """the w4 GEMM against another column: gain = the other's time minus its own"""
    return "ahead" if gain > spread else ("behind" if -gain > spread else "inside the spread")


def build(fmt):
    model = build_model(dict(LLAMA3_8B, num_hidden_layers=LAYERS), dict(num_hidden_layers=1), num_image_tokens=256, max_length=4096,
                        device=dev, init_on_device=True).eval()
    if fmt is not None:
        model.quantize_decoder_(fmt=fmt)
        torch.cuda.empty_cache()
    return model


def main():
    F.W4_GEMM_MAX_ROWS = {n: 4096 for n in F.W8Layer.NAMES}
    F.W4_GEMM_UNSPLIT_MAX_ROWS = {n: 0 for n in F.W8Layer.NAMES}
    if os.environ.get("LAUNCH_ONLY") == "1":
        with torch.no_grad():
            print(json.dumps({str(M): launch_times(M) for M in LAUNCH_ROWS}, indent=1))
        return
    res = dict(layers=LAYERS, cache_rows=CACHE, reps=REPS, steps_per_rep=STEPS, passes_per_rep=PASSES, device=torch.cuda.get_device_name(0),
               step={}, prompt={}, launch={})
    with torch.no_grad():
        model = None
        for kind in KINDS:
            if kind in ("bf16", "w4_scratch", "w8_gemm"):    # (w4_gemm: the model of w4_scratch)
                del model
                torch.cuda.empty_cache()
                model = build({"bf16": None, "w4_scratch": "mxfp4", "w8_gemm": "fp8_e4m3"}[kind])
            old = F.set_variant("w4_gemm", kind != "w4_scratch")
            try:
                res["step"][kind] = {str(B): step_times(model, B) for B in BATCHES}
                res["prompt"][kind] = {str(L): prompt_ms(model, L) for L in PROMPTS}
            finally:
                F.set_variant("w4_gemm", old)
            print(kind, json.dumps(res["step"][kind]), json.dumps(res["prompt"][kind]), flush=True)
        del model
        torch.cuda.empty_cache()
        res["launch"] = {str(M): launch_times(M) for M in LAUNCH_ROWS}

    def verdict(table, key):
        out = {}
        for n in table["bf16"]:
            t = {k: table[k][n] for k in KINDS}
            row = {f"{k}_ms": t[k][key] for k in KINDS}
            row.update({f"{k}_spread_ms": t[k]["spread"] for k in KINDS})
            g = t["w4_gemm"]
            for other in ("w4_scratch", "bf16", "w8_gemm"):
                row[f"w4_gemm_against_{other}"] = position(t[other][key] - g[key], max(g["spread"], t[other]["spread"]))
            out[n] = row
        return out
    res["verdict"] = dict(step=verdict(res["step"], "ms_per_step"), prompt=verdict(res["prompt"], "ms"))
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "decode_w4_wide.json"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["verdict"], indent=1))
    print(json.dumps(res["launch"], indent=1))


if __name__ == "__main__":
    main()
