#!/usr/bin/env python3
"""B prompts that share a prefix of S rows: the shared-prefix batch route against the route it replaces (LLaMA-3-8B layer shapes, random
weights, LAYERS layers scaled to 32).

Arms, on the same prompts (one prefix of S rows + own rows per sequence):
  "parent": the prompts without the argument -- _prefill_batch (prompts of one length as one batch of B * L rows, ragged ones one after
            the other, every sequence caching its own copy of the prefix), then the batch's decode step (mm355_attn_decode);
  "shared": greedy_decode(shared_prefix_rows=S)'s prompt pass -- _prefill_shared_batch (the prefix once, the own rows of all sequences in one
            decoder_extend_shared pass), then the decode step over the shared cache (mm355_attn_decode_shared).
Cells: S in PREFIXES x own rows in OWN ("r": ragged, 64 - 8 .. 64 + 8 rows) x B in BATCHES.  Per cell the prompt pass in ms and the
captured decode step in ms per step (STEPS steps from the prompts' lengths), median of REPS repetitions after one warm-up, the arms
taking turns within a repetition; "spread" is the largest (max - min) / median of the two arms' repetitions.  A cell counts as LOST
where the shared arm is slower than the parent arm by more than that spread.

The driver starts one child process per (S, B) under its own `timeout` (CELL_TIMEOUT seconds) and stops at the first child that fails.
Prints markdown tables (profiles/shared_prefix_batch.md is this output) and writes OUT (json).
Environment: LAYERS (2), REPS (5), STEPS (8), PREFIXES (512,2048), OWN (16,64,256,r), BATCHES (4,16), CELL_TIMEOUT (240), OUT."""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYERS, REPS, STEPS = int(os.environ.get("LAYERS", 2)), int(os.environ.get("REPS", 5)), int(os.environ.get("STEPS", 8))
PREFIXES = [int(x) for x in os.environ.get("PREFIXES", "512,2048").split(",")]
OWN = os.environ.get("OWN", "16,64,256,r").split(",")
BATCHES = [int(x) for x in os.environ.get("BATCHES", "4,16").split(",")]
CELL_TIMEOUT = int(os.environ.get("CELL_TIMEOUT", 240))
OUT = os.environ.get("OUT", "shared_prefix_batch.json")
SCALE = 32 / LAYERS


def own_rows(own, B):
    return [64 - 8 + (b * 5) % 17 for b in range(B)] if own == "r" else [int(own)] * B


def child(S, B):
    import torch
    from metamorph_amd import functional as F
    from metamorph_amd.factory import LLAMA3_8B, build_model
    from metamorph_amd.model.language_model.metamorph_llama import HipKVCache
    dev = torch.device("cuda:0")
    h = LLAMA3_8B["hidden_size"]
    model = build_model(dict(LLAMA3_8B, num_hidden_layers=LAYERS), dict(num_hidden_layers=1), num_image_tokens=256, max_length=4096,
                        device=dev, init_on_device=True).eval()
    layers = model.model.layers

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    rows = []
    with torch.no_grad():
        for own in OWN:
            ns = own_rows(own, B)
            torch.manual_seed(S + B + max(ns))
            pre = (torch.randn(S, h, device=dev) * 0.02).bfloat16()
            seqs = [torch.cat([pre, (torch.randn(n, h, device=dev) * 0.02).bfloat16()], 0) for n in ns]
            cap = S + max(ns) + STEPS + 8
            x = (torch.randn(B, h, device=dev) * 0.02).bfloat16()
            lens = [S + n for n in ns]
            prefill = {"parent": lambda c: model._prefill_batch(seqs, c, stepper=False), "shared": lambda c: model._prefill_shared_batch(seqs, c, S)}
            ts = {a: dict(prompt=[], step=[]) for a in prefill}
            for rep in range(REPS + 1):                       # (the first repetition warms up)
                for arm, fn in prefill.items():
                    cache = HipKVCache(capacity=cap)
                    t, _ = timed(lambda: fn(cache))
                    ts[arm]["prompt"].append(t)
                    kv = cache.kv
                    assert kv.lengths == lens and (kv.shared_len == S) == (arm == "shared"), (arm, kv.lengths, kv.shared_len)
                    st = F.DecodeStepGraph(layers, cache.meta, kv, cache.meta.cos, cache.meta.sin, h, dev)
                    st.step(x)                                # (warm-up and capture)
                    kv.set_lengths(lens)
                    ts[arm]["step"].append(timed(lambda: [st.step(x) for _ in range(STEPS)])[0] / STEPS)
                    del st, kv, cache
            r = dict(S=S, own=own, B=B, layers=LAYERS, steps=STEPS, reps=REPS)
            for what in ("prompt", "step"):
                spread = 0.0
                for arm in prefill:
                    v = ts[arm][what][1:]
                    r[f"{arm}_{what}_ms"], r[f"{arm}_{what}_min_ms"] = statistics.median(v), min(v)
                    spread = max(spread, (max(v) - min(v)) / statistics.median(v))
                r[f"{what}_spread"] = spread
                r[f"{what}_ratio"] = r[f"parent_{what}_ms"] / r[f"shared_{what}_ms"]
                r[f"{what}_lost"] = r[f"shared_{what}_ms"] > r[f"parent_{what}_ms"] * (1 + spread)
            rows.append(r)
            torch.cuda.empty_cache()
    print("CELLS " + json.dumps(rows), flush=True)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--cell":
        return child(int(sys.argv[2]), int(sys.argv[3]))
    res = dict(layers=LAYERS, reps=REPS, steps=STEPS, cells=[])
    print(f"\n### B prompts over one prefix of S rows, bf16 weights and cache ({LAYERS} layers measured, ms scaled to 32 layers; median of "
          f"{REPS}, {STEPS} steps per repetition)\n")
    print("| S | own rows | B | prompt pass: parent ms | shared ms | parent / shared | spread | decode step: parent ms | shared ms | parent / shared "
          "| spread | lost |\n|---|---|---|---|---|---|---|---|---|---|---|---|", flush=True)
    for S in PREFIXES:
        for B in BATCHES:
            p = subprocess.run(["timeout", "-k", "10", str(CELL_TIMEOUT), sys.executable, os.path.abspath(__file__), "--cell", str(S), str(B)],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            line = next((l for l in p.stdout.splitlines() if l.startswith("CELLS ")), None)
            if p.returncode != 0 or line is None:             # a child that failed or hung: nothing more is started on the device
                print(p.stdout[-3000:])
                print(f"child S={S} B={B} ended with status {p.returncode}: stopping", flush=True)
                return 1
            for r in json.loads(line[6:]):
                res["cells"].append(r)
                lost = ", ".join(w for w in ("prompt", "step") if r[f"{w}_lost"]) or "-"
                print(f"| {r['S']} | {'64 +- 8' if r['own'] == 'r' else r['own']} | {r['B']} | {r['parent_prompt_ms'] * SCALE:.1f} | "
                      f"{r['shared_prompt_ms'] * SCALE:.1f} | {r['prompt_ratio']:.2f} | {r['prompt_spread']:.2f} | {r['parent_step_ms'] * SCALE:.2f} | "
                      f"{r['shared_step_ms'] * SCALE:.2f} | {r['step_ratio']:.2f} | {r['step_spread']:.2f} | {lost} |", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
