#!/usr/bin/env python3
"""What the logits processors and the per-token log-probabilities add to the captured step of the device token loop, in ONE process run
(LLaMA-3-8B layer shapes, random weights, LAYERS layers; the decoder part of a step scales with the layers, the tail does not).

1. ms per captured step of greedy_decode at B in BATCHES (1, 16) with every option off and with everything on -- repetition_penalty 1.3,
   min_new_tokens = the run's length (the eos step stays live), two suppressed ids, output_logprobs -- as the difference of two run lengths
   (the prompt pass cancels).  No sequence ever finishes: the "on" arm's only eos id is a suppressed one, which cannot be picked.  The arms
   take turns within a repetition; REPS repetitions: median (and min).  The step is also given scaled to 32 layers (x 32 / LAYERS, which
   overstates the tail; the added time is NOT scaled).
2. The launches alone on the loop's last logits (device events around back-to-back calls, live sequences): mm355_logits_process_rows_f32,
   mm355_token_note_rows_f32, both, and mm355_sample_rows_f32 (temperature 0.7, top-k 50, top-p 0.9) on the same rows as the yardstick.

Prints markdown tables (profiles/logits_process.md is this output) and writes OUT (json).
Environment: LAYERS (2), REPS (5), PROMPT (64), NEW (64), BATCHES (1,16), OUT (logits_process.json in the working directory)."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from metamorph_amd import functional as F, ops
from metamorph_amd.factory import LLAMA3_8B, build_model

dev = torch.device("cuda:0")
LAYERS, REPS = int(os.environ.get("LAYERS", 2)), int(os.environ.get("REPS", 5))
L0, NEW = int(os.environ.get("PROMPT", 64)), int(os.environ.get("NEW", 64))
BATCHES = [int(b) for b in os.environ.get("BATCHES", "1,16").split(",")]
OUT = os.environ.get("OUT", "logits_process.json")
SCALE = 32 / LAYERS
h = LLAMA3_8B["hidden_size"]
SUPPRESS = [7, 128256]
ON = dict(repetition_penalty=1.3, suppress_tokens=SUPPRESS, output_logprobs=True, eos_token_id=(SUPPRESS[0],))


def run_ms(model, emb, n, kw):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    model.greedy_decode(None, None, emb, **{"eos_token_id": (), "max_new_tokens": n, **kw})
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def per_step(model, emb, kw):
    return (run_ms(model, emb, 2 * NEW, kw(2 * NEW)) - run_ms(model, emb, NEW, kw(NEW))) / NEW


def tail_us(call, n=200):
    """microseconds per call of a launch sequence, device events around n back-to-back calls"""
    for _ in range(10):
        call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def main():
    res = dict(layers=LAYERS, reps=REPS, prompt=L0, new=NEW, device=torch.cuda.get_device_name(0), step=[], launches=[])
    model = build_model(dict(LLAMA3_8B, num_hidden_layers=LAYERS), dict(num_hidden_layers=1), num_image_tokens=256, max_length=4096,
                        device=dev, init_on_device=True).eval()
    arms = {"off": lambda n: {}, "on": lambda n: dict(ON, min_new_tokens=n)}
    old = F.set_variant("greedy_loop_b1", True)                  # (one sequence with every option off takes the device loop as well)
    try:
        print(f"\n### captured step of the device token loop, {LAYERS} decoder layers at 8B widths, V = {model.config.vocab_size}, prompts of "
              f"{L0} rows, per step = (run of {2 * NEW} - run of {NEW} tokens) / {NEW}; median (min) of {REPS}, the arms taking turns\n")
        print(f"| B | off ms | on ms | added us (on - off) | off ms x {SCALE:g} (32 layers) | added / that |\n|---|---|---|---|---|---|", flush=True)
        loops = {}
        for B in BATCHES:
            emb = (torch.randn(B, L0, h, device=dev) * 0.02).bfloat16()
            ts = {k: [] for k in arms}
            for rep in range(REPS + 1):                          # (the first repetition warms up)
                for k, kw in arms.items():
                    ts[k].append(per_step(model, emb, kw))
            loops[B] = model._greedy_loop                        # the "on" arm's: its static logits, bitmap and logs
            off, on = statistics.median(ts["off"][1:]), statistics.median(ts["on"][1:])
            r = dict(B=B, off_ms=off, off_min_ms=min(ts["off"][1:]), on_ms=on, on_min_ms=min(ts["on"][1:]), added_us=(on - off) * 1e3,
                     off_ms_32=off * SCALE, steps=loops[B].steps, graph=bool(loops[B].graphs))
            res["step"].append(r)
            print(f"| {B} | {off:.4f} ({r['off_min_ms']:.4f}) | {on:.4f} ({r['on_min_ms']:.4f}) | {r['added_us']:+.1f} | {r['off_ms_32']:.3f} | "
                  f"{(on - off) / r['off_ms_32'] * 100:+.2f} % |", flush=True)
        print("\n### the launches alone on the loop's last logits (us per call, device events around 200 back-to-back calls, live sequences)\n")
        print("| B | logits_process_rows | token_note_rows | both | sample_rows (T 0.7, top-k 50, top-p 0.9) | both / sample_rows |\n|---|---|---|---|---|---|",
              flush=True)
        for B, loop in loops.items():
            p = loop.processors
            assert p is not None and p.penalised and p.want_logprobs
            state = torch.zeros_like(loop.state)                 # live sequences at their first entry
            u = torch.rand(B, device=dev)
            penalty, min_new, sup = loop._process
            eos = loop.scalars[4]
            N, cap = loop.scalars[2], loop.tok_log.shape[1]

            def process():
                ops.logits_process_rows(loop.logits, penalty, loop.seen, state[2], min_new, eos, sup)

            def note():
                ops.token_note_rows(loop.logits, loop.tok, state, N, cap, seen=loop.seen, logp_log=loop.logp_log)

            def both():
                process(); note()
            t = dict(B=B, marked_ids=int(sum(bin(w & 0xFFFFFFFF).count("1") for w in loop.seen[0].cpu().tolist())),
                     process_us=tail_us(process), note_us=tail_us(note), both_us=tail_us(both),
                     sample_us=tail_us(lambda: ops.sample_rows(loop.logits, 1 / 0.7, 50, 0.9, u, out=loop.tok)))
            res["launches"].append(t)
            print(f"| {B} | {t['process_us']:.1f} | {t['note_us']:.1f} | {t['both_us']:.1f} | {t['sample_us']:.1f} | {t['both_us'] / t['sample_us']:.2f} |",
                  flush=True)
        print(f"\n(ids marked in sequence 0's bitmap at the end of the run: {[t['marked_ids'] for t in res['launches']]})")
    finally:
        F.set_variant("greedy_loop_b1", old)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    with torch.no_grad():
        main()
