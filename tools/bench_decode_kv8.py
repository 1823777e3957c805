#!/usr/bin/env python3
"""Decode over an FP8 (e4m3) KV cache against the bf16 cache, in ONE process run (LLaMA-3-8B widths, random weights, 8 layers + lm_head):
  * the captured decode step at 1 / 16 / 64 sequences x caches of 1024 / 4096 rows, bf16 cache against fp8 cache, on bf16 weights and on
    quantize_decoder_ weights -- the two caches alternate inside every repetition;
  * per-launch times of attn_decode against attn_decode_f8 and of rope_kv_append_ against rope_kv_append_f8_ at the same shapes, with the
    achieved GB/s over the bytes of the live cache rows (scales included), the caches rotated through copies larger than the last-level cache;
  * max logit difference and top-1 agreement of the fp8-cache step against the bf16-cache step on seeded weights (teacher-forced rows).
REPS repetitions each: median and spread.  Writes profiles/decode_kv8.json; DESIGN.md section 7.1 quotes that file.
Environment: LAYERS (8), REPS (5), STEPS (16 steps per repetition), OUT."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from metamorph_amd import functional as F, ops
from metamorph_amd.factory import LLAMA3_8B, build_model

dev = torch.device("cuda:0")
LAYERS, REPS, STEPS = int(os.environ.get("LAYERS", 8)), int(os.environ.get("REPS", 5)), int(os.environ.get("STEPS", 16))
h, Hq, Hkv, d = 4096, 32, 8, 128
W = Hkv * d
BATCHES, CACHES = (1, 16, 64), (1024, 4096)
FMTS = ("bf16", "fp8_e4m3")


def timed(fn, n):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def start_lengths(B, rows):
    return [rows - STEPS - 4 - 7 * b for b in range(B)]      # every timed step stays inside `rows` (1024: the one-key-group bound)


def fill(kv):
    if kv.kv8 is None:
        kv.k.normal_(0, 0.5); kv.v.normal_(0, 0.5)
    else:
        kv.k.random_(0, 120); kv.v.random_(0, 120)           # finite e4m3 bytes (|value| <= 240), scales of 2^-9
        kv.k_scale.fill_(2.0 ** -9); kv.v_scale.fill_(2.0 ** -9)


def step_times(model, B, rows):
    _, meta = model._decode_meta(rows)
    cap = rows + 8
    cos, sin = model.model.rope_tables(cap, dev)
    meta.cos, meta.sin = cos, sin
    start = start_lengths(B, rows)
    x = (torch.randn(B, h, device=dev) * 0.02).bfloat16()
    run = {}
    for fmt in FMTS:
        kv = F.KVCache(len(model.model.layers), cap, W, dev, Hq=Hq, d=d, batch=B, fmt=fmt)
        fill(kv)
        kv.set_lengths(start)
        st = F.DecodeStepGraph(model.model.layers, meta, kv, cos, sin, h, dev)
        run[fmt] = (kv, st)
        for _ in range(3):
            model._rows_logits(st.step(x))
    out = {fmt: [] for fmt in FMTS}
    for _ in range(REPS):
        for fmt in FMTS:                                      # the two caches alternate inside a repetition
            kv, st = run[fmt]
            kv.set_lengths(start)
            out[fmt].append(timed(lambda: model._rows_logits(st.step(x)), STEPS) * 1e3)
    res = {fmt: dict(ms_per_step=statistics.median(t), reps=t, spread=max(t) - min(t), graph=run[fmt][1].graph is not None,
                     cache_MB=run[fmt][0].nbytes() / 2 ** 20) for fmt, t in out.items()}
    sp = max(res[f]["spread"] for f in FMTS)
    res["fp8_minus_bf16_ms"] = res["fp8_e4m3"]["ms_per_step"] - res["bf16"]["ms_per_step"]
    res["spread_ms"] = sp
    res["fp8_faster"] = -res["fp8_minus_bf16_ms"] > sp
    res["fp8_slower"] = res["fp8_minus_bf16_ms"] > sp
    return res


def launch_times(B, rows):
    """us per launch of the attention and append kernels of ONE layer, both formats; GB/s over the bytes of the live rows"""
    cap = rows + 8
    lens = [n + 1 for n in start_lengths(B, rows)]
    kvl = torch.tensor(lens, dtype=torch.int32, device=dev)
    pos = torch.tensor([n - 1 for n in lens], dtype=torch.int32, device=dev)
    bound = F.SHORT_KV if rows <= F.SHORT_KV else cap
    cos, sin = ops.rope_table(cap, d, 500000.0, dev)
    qkv = (torch.randn(B, (Hq + 2 * Hkv) * d, device=dev) * 0.5).bfloat16()
    ws = torch.zeros(int(ops._L().mm355_attn_decode_ws_floats(B, Hq, d, cap)), device=dev, dtype=torch.float32)
    res = {}
    for fmt in FMTS:
        per_row = 2 * W * 2 if fmt == "bf16" else 2 * (W + 4 * Hkv)
        live = sum(lens) * per_row
        n = min(max(2, (600 << 20) // (B * cap * per_row) + 1), 128)
        caches = []
        for _ in range(n):
            kv = F.KVCache(1, cap, W, dev, batch=B, d=d, fmt=fmt)
            fill(kv)
            caches.append(kv)
        if fmt == "bf16":
            att = [(lambda c=c: ops.attn_decode(qkv[:, :Hq * d], c.k[0], c.v[0], kvl, bound, Hq, Hkv, d, d ** -0.5, workspace=ws)) for c in caches]
            app = [(lambda c=c: ops.rope_kv_append_(qkv, Hq, Hkv, d, cos, sin, pos, c.k[0], c.v[0])) for c in caches]
        else:
            att = [(lambda c=c: ops.attn_decode_f8(qkv[:, :Hq * d], c.k[0], c.v[0], c.k_scale[0], c.v_scale[0], kvl, bound, Hq, Hkv, d, d ** -0.5,
                                                   workspace=ws)) for c in caches]
            app = [(lambda c=c: ops.rope_kv_append_f8_(qkv, Hq, Hkv, d, cos, sin, pos, c.k[0], c.v[0], c.k_scale[0], c.v_scale[0])) for c in caches]
        res[fmt] = dict(copies=n, live_MB=live / 2 ** 20)
        for name, fns in (("attn", att), ("append", app)):
            def rnd():
                for f in fns:
                    f()
            rnd()
            inner = max(1, 200 // n)
            ts = [timed(rnd, inner) / n * 1e6 for _ in range(REPS)]
            us = statistics.median(ts)
            res[fmt][name] = dict(us=us, spread_us=max(ts) - min(ts))
            if name == "attn":
                res[fmt][name]["GBps"] = live / us / 1e3
        del caches, att, app
        torch.cuda.empty_cache()
    return res


def accuracy(model, B=16, L0=256, steps=8):
    """Teacher-forced: both caches are fed the same prompt and the same rows; per step the fp32 logits of the two"""
    _, meta = model._decode_meta(L0)
    cap = L0 + steps + 2
    cos, sin = model.model.rope_tables(cap, dev)
    g = torch.Generator(device="cpu").manual_seed(17)
    emb = (torch.randn(B, L0 + steps, h, generator=g) * 0.02).bfloat16().to(dev)
    kvs = {}
    for fmt in FMTS:
        kv = F.KVCache(len(model.model.layers), cap, W, dev, Hq=Hq, d=d, batch=B, fmt=fmt)
        for b in range(B):
            _, mb = model._decode_meta(L0)
            mb.cos, mb.sin = cos, sin
            F.decoder_prefill(emb[b, :L0].contiguous(), model.model.layers, mb, kv, row=b)
        kvs[fmt] = kv
    meta.cos, meta.sin = cos, sin
    diff, scale, agree, total = 0.0, 0.0, 0, 0
    for t in range(steps):
        rows = emb[:, L0 + t].contiguous()
        lg = {fmt: model._rows_logits(F.decoder_decode_row(rows, model.model.layers, meta, kvs[fmt], cos, sin)).float() for fmt in FMTS}
        diff = max(diff, float((lg["bf16"] - lg["fp8_e4m3"]).abs().max()))
        scale = max(scale, float(lg["bf16"].abs().max()))
        agree += int((lg["bf16"].argmax(-1) == lg["fp8_e4m3"].argmax(-1)).sum())
        total += B
    return dict(sequences=B, prompt_rows=L0, steps=steps, max_logit_diff=diff, max_abs_logit=scale, top1_agree=agree, top1_total=total)


def main():
    torch.manual_seed(1234)
    model = build_model(dict(LLAMA3_8B, num_hidden_layers=LAYERS), dict(num_hidden_layers=1), num_image_tokens=256, max_length=4096,
                        device=dev, init_on_device=True).eval()
    res = dict(layers=LAYERS, reps=REPS, steps_per_rep=STEPS, device=torch.cuda.get_device_name(0), step={}, launch={}, accuracy={})
    with torch.no_grad():
        for weights in ("bf16", "w8"):
            if weights == "w8":
                model.quantize_decoder_(lm_head=True)
                torch.cuda.empty_cache()
            res["accuracy"][weights] = accuracy(model)
            print(weights, "accuracy", json.dumps(res["accuracy"][weights]), flush=True)
            res["step"][weights] = {}
            for rows in CACHES:
                for B in BATCHES:
                    r = step_times(model, B, rows)
                    res["step"][weights][f"{B}x{rows}"] = r
                    print(weights, f"{B}x{rows}", json.dumps({k: v for k, v in r.items() if k not in FMTS}),
                          {f: round(r[f]["ms_per_step"], 4) for f in FMTS}, flush=True)
                    torch.cuda.empty_cache()
        del model
        torch.cuda.empty_cache()
        for rows in CACHES:
            for B in BATCHES:
                res["launch"][f"{B}x{rows}"] = launch_times(B, rows)
                print("launch", f"{B}x{rows}", json.dumps(res["launch"][f"{B}x{rows}"]), flush=True)
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "decode_kv8.json"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
