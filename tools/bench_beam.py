#!/usr/bin/env python3
"""Beam search: the device beam loop (beam_decode / generate(device_beam_search=True)) against the HF beam path
(generate(use_customize_greedy=False, num_beams=K): HF's host loop, HipKVCache.reorder_cache per token), in ONE process run (LLaMA-3-8B
layer shapes, random weights, LAYERS layers, V = 128 258 logits).

1. ms per step: each arm generates NEW and SHORT new tokens from the same prompt; (t(NEW) - t(SHORT)) / (NEW - SHORT) leaves the prompt
   pass, the capture and the first tail out.  No eos id, so both arms run every step.  K in BEAMS, prompts of PROMPTS rows.
2. The new kernels alone, captured launches replayed: mm355_beam_select_rows_f32 and mm355_beam_advance at K rows of V logits, and the
   attention launch with the table (mm355_attn_decode_shared_idx) against mm355_attn_decode_shared at the same shape; the spread between
   two timings of the same unindexed launch is printed beside them.

REPS repetitions, the arms taking turns: median (and min).  Prints markdown tables (profiles/beam_search.md is this output) and writes OUT
(json).  Environment: LAYERS (2), REPS (5), NEW (64), SHORT (8), BEAMS (2,4,8), PROMPTS (512,2048), OUT (beam_search.json)."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from metamorph_amd import functional as F, ops
from metamorph_amd.factory import LLAMA3_8B, build_model

dev = torch.device("cuda:0")
LAYERS, REPS = int(os.environ.get("LAYERS", 2)), int(os.environ.get("REPS", 5))
NEW, SHORT = int(os.environ.get("NEW", 64)), int(os.environ.get("SHORT", 8))
BEAMS = [int(x) for x in os.environ.get("BEAMS", "2,4,8").split(",")]
PROMPTS = [int(x) for x in os.environ.get("PROMPTS", "512,2048").split(",")]
OUT = os.environ.get("OUT", "beam_search.json")
V = 128258


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def loop_table(model, res):
    for L in PROMPTS:
        ids = torch.randint(0, 128000, (1, L), generator=torch.Generator().manual_seed(L)).to(dev)
        for K in BEAMS:
            kw = dict(inputs=ids, num_beams=K, num_return_sequences=1)
            arms = {"device": lambda n: model.generate(device_beam_search=True, eos_token_id=(), max_new_tokens=n, **kw),
                    "hf": lambda n: model.generate(use_customize_greedy=False, do_sample=False, eos_token_id=None, pad_token_id=0, max_new_tokens=n,
                                                   return_dict_in_generate=True, output_scores=False, **kw)}
            ts = {(a, n): [] for a in arms for n in (NEW, SHORT)}
            for rep in range(REPS + 1):                       # (the first repetition warms up)
                for a, fn in arms.items():
                    for n in (NEW, SHORT):
                        t, out = timed(lambda: fn(n))
                        ts[(a, n)].append(t)
                        got = len(out[0]) if a == "device" else out.sequences.shape[1]
                        assert got == n, (a, n, got)          # every step ran
            r = dict(rows=L, K=K, layers=LAYERS, new=NEW, short=SHORT)
            for a in arms:
                per = [(x - y) / (NEW - SHORT) for x, y in zip(ts[(a, NEW)][1:], ts[(a, SHORT)][1:])]
                r[a + "_ms"], r[a + "_min_ms"], r[a + "_total_ms"] = statistics.median(per), min(per), statistics.median(ts[(a, NEW)][1:])
            r["hf_over_device"] = r["hf_ms"] / r["device_ms"]
            res["loop"].append(r)
            print(f"| {L} | {K} | {r['device_ms']:.3f} ({r['device_min_ms']:.3f}) | {r['hf_ms']:.3f} ({r['hf_min_ms']:.3f}) | {r['hf_over_device']:.2f} | "
                  f"{r['device_total_ms']:.1f} | {r['hf_total_ms']:.1f} |", flush=True)
            torch.cuda.empty_cache()


def graph_us(fn, n=50):
    """fn captured once, the graph of n launches replayed: microseconds per launch"""
    fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay(); torch.cuda.synchronize()
    t, _ = timed(g.replay)
    return t * 1e3 / n


def kernel_table(model, res):
    cfg = model.config
    Hq, Hkv, d = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.hidden_size // cfg.num_attention_heads
    for K in BEAMS:
        M = F.beam_candidates(K, 2)
        x = torch.randn(K, V, device=dev) * 3
        CAP = 8192                                            # (every timed launch is a live step: the logs and the table have room for all of them)
        host = F.beam_state_host(K, CAP)
        host["running"][:] = -torch.rand(K).numpy()
        state = {n: torch.from_numpy(host[n]).to(dev) for n in F.BEAM_STATE}
        pw = torch.from_numpy(F.beam_len_pow(CAP, 1.0)).to(dev)
        stats, val, idx = ops.beam_select_rows(x, state["running"], M)
        ws = ops.beam_select_rows_ws(K, V, M, dev)
        embed = model.model.embed_tokens.weight.data
        x_in = torch.zeros((K, embed.shape[1]), device=dev, dtype=torch.bfloat16)

        running = state["running"].clone()                    # (the selection's input stays what it was while the advance moves the state)

        def advance():
            ops.beam_advance(val, idx, V, state, pw, CAP, 1.0, 0, (128001, 128009), embed=embed, x_in=x_in)
        runs = {"select": lambda: ops.beam_select_rows(x, running, M, stats, val, idx, ws), "advance": advance}
        for L in PROMPTS:
            own = NEW // 2
            rows = L + NEW + 2
            q = (torch.randn(K, Hq * d, device=dev) * 0.5).bfloat16()
            kc = (torch.randn(K, rows, Hkv * d, device=dev) * 0.5).bfloat16()
            vc = (torch.randn(K, rows, Hkv * d, device=dev) * 0.5).bfloat16()
            lens = torch.full((K,), L + own, device=dev, dtype=torch.int32)
            tbl = torch.randint(0, K, (K, NEW + 1), device=dev, dtype=torch.uint8)
            sws = torch.empty(int(ops._L().mm355_attn_decode_shared_ws_floats(K, Hq, Hkv, d, L, rows)), device=dev, dtype=torch.float32)
            out = torch.empty_like(q)
            A = (q, kc[0], vc[0], kc, vc, lens, L, rows, Hq, Hkv, d, d ** -0.5)
            runs[f"attn {L}"] = lambda A=A, out=out, sws=sws: ops.attn_decode_shared(*A, out=out, workspace=sws)
            runs[f"attn {L} again"] = runs[f"attn {L}"]
            runs[f"attn_idx {L}"] = lambda A=A, out=out, sws=sws, tbl=tbl: ops.attn_decode_shared(*A, out=out, workspace=sws, own_block=tbl)
        ts = {k: [] for k in runs}
        for rep in range(REPS + 1):
            for k, fn in runs.items():
                ts[k].append(graph_us(fn))
        assert int(state["live"].item()) == 1 and int(state["scal"][1].item()) < CAP, "the timed advance launches were not all live steps"
        r = dict(K=K, M=M, V=V, **{k.replace(" ", "_") + "_us": statistics.median(t[1:]) for k, t in ts.items()})
        res["kernels"].append(r)
        att = " | ".join(f"{r[f'attn_{L}_us']:.1f} / {r[f'attn_idx_{L}_us']:.1f} (spread {abs(r[f'attn_{L}_us'] - r[f'attn_{L}_again_us']):.1f})" for L in PROMPTS)
        print(f"| {K} | {M} | {r['select_us']:.1f} | {r['advance_us']:.1f} | {att} |", flush=True)


def main():
    res = dict(layers=LAYERS, reps=REPS, new=NEW, short=SHORT, device=torch.cuda.get_device_name(0), loop=[], kernels=[])
    model = build_model(dict(LLAMA3_8B, num_hidden_layers=LAYERS, vocab_size=V), dict(num_hidden_layers=1), num_image_tokens=256, max_length=4096,
                        device=dev, init_on_device=True).eval()
    with torch.no_grad():
        print(f"\n### beam search, ms per step: the device beam loop against the HF beam path ({LAYERS} layers, V = {V}, bf16; "
              f"(t({NEW} tokens) - t({SHORT} tokens)) / {NEW - SHORT}, median (min) of {REPS})\n")
        print(f"| prompt rows | K | device loop ms | HF path ms | HF / device | device, {NEW} tokens in all ms | HF, {NEW} tokens in all ms |\n"
              "|---|---|---|---|---|---|---|", flush=True)
        loop_table(model, res)
        print(f"\n### the new kernels alone (captured launches, microseconds, median of {REPS}; own rows: {NEW // 2})\n")
        print("| K | M | beam_select_rows | beam_advance | " + " | ".join(f"attention, {L} shared rows: unindexed / indexed" for L in PROMPTS)
              + " |\n|---|---|---|---|" + "---|" * len(PROMPTS), flush=True)
        kernel_table(model, res)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
