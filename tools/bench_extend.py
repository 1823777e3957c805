#!/usr/bin/env python3
"""The extend pass against what it replaces, in ONE process run (LLaMA-3-8B layer shapes, random weights, LAYERS layers scaled to 32):

1. functional.decoder_extend of n in {2, 4, 8, 16, 64, 512} rows on a cache holding 512 and 4096 rows, against n captured decode steps
   (DecodeStepGraph.step once per row: what `_decode_batch` ran for such a call before the extend pass existed), on a bf16 and an
   fp8_e4m3 cache, on bf16 and on quantize_decoder_ weights.  Both arms leave the cache at its start length before every repetition.
2. A 4096-row prompt of one sequence in one pass (decoder_prefill) against slices of 512 rows (decoder_prefill_chunked): time and
   torch.cuda.max_memory_allocated above the resident model and cache, on bf16 and on quantised weights.

REPS repetitions each: median (and min).  Prints markdown tables (profiles/extend_pass.md is this output) and writes OUT (json).
Environment: LAYERS (4), REPS (5), OUT (extend_pass.json in the working directory), ROWS (the n list), PREFIXES."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from metamorph_amd import functional as F
from metamorph_amd.factory import LLAMA3_8B, build_model

dev = torch.device("cuda:0")
LAYERS, REPS = int(os.environ.get("LAYERS", 4)), int(os.environ.get("REPS", 5))
ROWS = [int(x) for x in os.environ.get("ROWS", "2,4,8,16,64,512").split(",")]
PREFIXES = [int(x) for x in os.environ.get("PREFIXES", "512,4096").split(",")]
OUT = os.environ.get("OUT", "extend_pass.json")
h = LLAMA3_8B["hidden_size"]
SCALE = 32 / LAYERS


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def med(fn, reset):
    ts = []
    for _ in range(REPS + 1):
        reset()
        ts.append(timed(fn))
    ts = ts[1:]                                               # (the first repetition warms up: graph capture, workspaces)
    return statistics.median(ts), min(ts)


def extend_table(model, weights, res):
    layers = model.model.layers
    for fmt in ("bf16", "fp8_e4m3"):
        for past in PREFIXES:
            cap = past + max(ROWS) + 8
            _, meta = model._decode_meta(1)
            cos, sin = model.model.rope_tables(cap, dev)
            meta.cos, meta.sin = cos, sin
            kv = F.KVCache(len(layers), cap, meta.Hkv * meta.d, dev, Hq=meta.Hq, d=meta.d, fmt=fmt)
            if fmt == "bf16":
                kv.k.normal_(0, 0.5); kv.v.normal_(0, 0.5)
            else:
                kv.k.random_(0, 120); kv.v.random_(0, 120); kv.k_scale.fill_(2.0 ** -6); kv.v_scale.fill_(2.0 ** -6)
            kv.set_lengths([past])
            st = F.DecodeStepGraph(layers, meta, kv, cos, sin, h, dev)
            for n in ROWS:
                x = (torch.randn(n, h, device=dev) * 0.02).bfloat16()
                reset = lambda: kv.set_lengths([past])
                one = med(lambda: F.decoder_extend(x, layers, meta, kv), reset)
                steps = med(lambda: [st.step(x[t:t + 1]) for t in range(n)], reset)
                r = dict(weights=weights, cache=fmt, past=past, n=n, layers=LAYERS, extend_ms=one[0], extend_min_ms=one[1], steps_ms=steps[0],
                         steps_min_ms=steps[1], extend_ms_32=one[0] * SCALE, steps_ms_32=steps[0] * SCALE, speedup=steps[0] / one[0],
                         graph=st.graph is not None)
                res["extend"].append(r)
                print(f"| {weights} | {fmt} | {past} | {n} | {r['extend_ms_32']:.2f} | {r['steps_ms_32']:.2f} | {r['speedup']:.2f} |", flush=True)
            del st, kv
            torch.cuda.empty_cache()


def prompt_table(model, weights, res, L=4096, chunk=512):
    layers = model.model.layers
    _, meta = model._decode_meta(L)
    cos, sin = model.model.rope_tables(L + 8, dev)
    meta.cos, meta.sin = cos, sin
    kv = F.KVCache(len(layers), L + 8, meta.Hkv * meta.d, dev, Hq=meta.Hq, d=meta.d)
    x = (torch.randn(L, h, device=dev) * 0.02).bfloat16()
    for name, fn in (("one pass", lambda: F.decoder_prefill(x, layers, meta, kv)),
                     (f"slices of {chunk}", lambda: F.decoder_prefill_chunked(x, layers, meta, kv, chunk))):
        reset = lambda: kv.set_lengths([0])
        reset(); fn(); torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t = med(fn, reset)
        peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        r = dict(weights=weights, rows=L, how=name, layers=LAYERS, ms=t[0], min_ms=t[1], ms_32=t[0] * SCALE, peak_mib_above_resident=peak)
        res["prompt"].append(r)
        print(f"| {weights} | {name} | {r['ms_32']:.1f} | {peak:.0f} |", flush=True)


def main():
    res = dict(layers=LAYERS, reps=REPS, device=torch.cuda.get_device_name(0), extend=[], prompt=[])
    model = build_model(dict(LLAMA3_8B, num_hidden_layers=LAYERS), dict(num_hidden_layers=1), num_image_tokens=256, max_length=4096,
                        device=dev, init_on_device=True).eval()
    with torch.no_grad():
        for weights in ("bf16", "w8"):
            if weights == "w8":
                model.quantize_decoder_(lm_head=True)
            print(f"\n### decoder_extend against n decode steps, {weights} weights ({LAYERS} layers measured, ms scaled to 32 layers; median of {REPS})\n")
            print("| weights | cache | cached rows | n | extend pass ms | n steps ms | steps / extend |\n|---|---|---|---|---|---|---|", flush=True)
            extend_table(model, weights, res)
            print(f"\n### 4096-row prompt, {weights} weights (ms scaled to 32 layers; peak MiB above the resident model and cache, {LAYERS} layers)\n")
            print("| weights | how | ms | peak MiB |\n|---|---|---|---|", flush=True)
            prompt_table(model, weights, res)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
