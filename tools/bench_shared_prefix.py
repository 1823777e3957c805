#!/usr/bin/env python3
"""n continuations of one prompt: the shared prompt cache against what it replaces, in ONE process run (LLaMA-3-8B layer shapes, random
weights, LAYERS layers scaled to 32).

1. The decode step of n in {4, 16, 32, 64} sequences on a prompt of {512, 2048, 8192} rows, on a bf16 and an fp8_e4m3 cache, three arms on
   the same cache contents (the prompt's rows in sequence 0, copied to every sequence): "shared" (KVCache.set_shared: mm355_attn_decode_shared
   reads the rows once), "fan-out" (every sequence reads its own copy: mm355_attn_decode) and "repeated" -- the cache a batch of n copies of
   the prompt leaves behind, which runs the launches of the fan-out arm; it is timed on its own as the yardstick and shows the noise between
   two runs of one code path.  Each arm is a captured DecodeStepGraph; a repetition is STEPS steps from the prompt's length, the arms take
   turns within a repetition.  Also the largest absolute difference of the step's hidden rows between the shared and the fan-out arm.
2. The prompt pass: once (decoder_prefill of one sequence) against the batch of n copies (decoder_prefill of n * rows rows), the latter
   only up to BATCH_ROWS rows in all (default 32768).

REPS repetitions each: median (and min).  Prints markdown tables (profiles/shared_prefix.md is this output) and writes OUT (json).
Environment: LAYERS (2), REPS (5), STEPS (8), OUT (shared_prefix.json in the working directory), COPIES, PROMPTS, BATCH_ROWS."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from metamorph_amd import functional as F
from metamorph_amd.factory import LLAMA3_8B, build_model

dev = torch.device("cuda:0")
LAYERS, REPS, STEPS = int(os.environ.get("LAYERS", 2)), int(os.environ.get("REPS", 5)), int(os.environ.get("STEPS", 8))
COPIES = [int(x) for x in os.environ.get("COPIES", "4,16,32,64").split(",")]
PROMPTS = [int(x) for x in os.environ.get("PROMPTS", "512,2048,8192").split(",")]
BATCH_ROWS = int(os.environ.get("BATCH_ROWS", 32768))
OUT = os.environ.get("OUT", "shared_prefix.json")
h = LLAMA3_8B["hidden_size"]
SCALE = 32 / LAYERS


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def fill(kv, L):
    """random prompt rows in sequence 0, copied to every sequence"""
    if kv.fmt == "bf16":
        kv.k[:, 0, :L].normal_(0, 0.5); kv.v[:, 0, :L].normal_(0, 0.5)
    else:
        kv.k[:, 0, :L].random_(0, 120); kv.v[:, 0, :L].random_(0, 120); kv.k_scale.fill_(2.0 ** -6); kv.v_scale.fill_(2.0 ** -6)
    kv.copy_prefix(L)


def step_table(model, res):
    layers = model.model.layers
    for fmt in ("bf16", "fp8_e4m3"):
        for L in PROMPTS:
            for n in COPIES:
                cap = L + STEPS + 8
                _, meta = model._decode_meta(1)
                cos, sin = model.model.rope_tables(cap, dev)
                meta.cos, meta.sin = cos, sin
                x = (torch.randn(n, h, device=dev) * 0.02).bfloat16()
                arms = {}
                for arm in ("shared", "fan-out", "repeated"):
                    kv = F.KVCache(len(layers), cap, meta.Hkv * meta.d, dev, Hq=meta.Hq, d=meta.d, batch=n, fmt=fmt)
                    torch.manual_seed(L + n)
                    fill(kv, L)
                    kv.set_lengths([L] * n)
                    if arm == "shared":
                        kv.set_shared(L)
                    y = F.decoder_decode_row(x, layers, meta, kv, cos, sin).clone()      # eager, once: the hidden rows of the first step
                    kv.set_lengths([L] * n)
                    arms[arm] = (kv, F.DecodeStepGraph(layers, meta, kv, cos, sin, h, dev), y, [])
                diff = float((arms["shared"][2].float() - arms["fan-out"][2].float()).abs().max())
                ref = float(arms["fan-out"][2].float().abs().max())
                for rep in range(REPS + 1):                   # (the first repetition warms up)
                    for arm, (kv, st, _, ts) in arms.items():
                        kv.set_lengths([L] * n)
                        ts.append(timed(lambda: [st.step(x) for _ in range(STEPS)]) / STEPS)
                r = dict(cache=fmt, rows=L, n=n, layers=LAYERS, steps=STEPS, max_abs_diff=diff, max_abs_hidden=ref,
                         graph=all(a[1].graph is not None for a in arms.values()))
                for arm, (_, _, _, ts) in arms.items():
                    key = arm.replace("-", "_")
                    r[key + "_ms"], r[key + "_min_ms"], r[key + "_ms_32"] = statistics.median(ts[1:]), min(ts[1:]), statistics.median(ts[1:]) * SCALE
                r["repeated_over_shared"] = r["repeated_ms"] / r["shared_ms"]
                res["step"].append(r)
                print(f"| {fmt} | {L} | {n} | {r['shared_ms_32']:.2f} | {r['fan_out_ms_32']:.2f} | {r['repeated_ms_32']:.2f} | "
                      f"{r['repeated_over_shared']:.2f} | {diff:.2e} ({ref:.2f}) |", flush=True)
                del arms
                torch.cuda.empty_cache()


def prompt_table(model, res):
    layers = model.model.layers
    for L in PROMPTS:
        for n in COPIES:
            cap = L + 8
            cos, sin = model.model.rope_tables(cap, dev)
            kv = F.KVCache(len(layers), cap, model._decode_meta(1)[1].Hkv * model._decode_meta(1)[1].d, dev, batch=n)
            x = (torch.randn(L, h, device=dev) * 0.02).bfloat16()
            _, m1 = model._decode_meta(L)
            m1.cos, m1.sin = cos, sin
            runs = {"once": lambda: F.decoder_prefill(x, layers, m1, kv, row=0)}
            if n * L <= BATCH_ROWS:
                _, mb = model._decode_meta(L)
                mb.B, mb.cos, mb.sin = n, cos, sin
                xb = x.repeat(n, 1)
                runs["batch"] = lambda: F.decoder_prefill(xb, layers, mb, kv)
            ts = {k: [] for k in runs}
            for rep in range(REPS + 1):
                for k, fn in runs.items():
                    kv.set_lengths([0] * n)
                    ts[k].append(timed(fn))
            r = dict(rows=L, n=n, layers=LAYERS, once_ms=statistics.median(ts["once"][1:]), once_ms_32=statistics.median(ts["once"][1:]) * SCALE)
            if "batch" in ts:
                r["batch_ms"] = statistics.median(ts["batch"][1:])
                r["batch_ms_32"] = r["batch_ms"] * SCALE
            res["prompt"].append(r)
            b = f"{r['batch_ms_32']:.1f} | {r['batch_ms'] / r['once_ms']:.1f}" if "batch_ms" in r else f"not measured (> {BATCH_ROWS} rows) | -"
            print(f"| {L} | {n} | {r['once_ms_32']:.1f} | {b} |", flush=True)
            del kv, runs
            torch.cuda.empty_cache()


def main():
    res = dict(layers=LAYERS, reps=REPS, steps=STEPS, device=torch.cuda.get_device_name(0), step=[], prompt=[])
    model = build_model(dict(LLAMA3_8B, num_hidden_layers=LAYERS), dict(num_hidden_layers=1), num_image_tokens=256, max_length=4096,
                        device=dev, init_on_device=True).eval()
    with torch.no_grad():
        print(f"\n### decode step of n continuations of one prompt, bf16 weights ({LAYERS} layers measured, ms per step scaled to 32 layers; "
              f"median of {REPS} x {STEPS} steps)\n")
        print("| cache | prompt rows | n | shared ms | fan-out ms | repeated ms | repeated / shared | max abs diff of the hidden rows, shared vs "
              "fan-out (max abs) |\n|---|---|---|---|---|---|---|---|", flush=True)
        step_table(model, res)
        print(f"\n### prompt pass (ms scaled to 32 layers; median of {REPS})\n")
        print("| prompt rows | n | once ms | batch of n ms | batch / once |\n|---|---|---|---|---|", flush=True)
        prompt_table(model, res)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
