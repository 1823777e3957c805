#!/usr/bin/env python3
"""ms per prompt pass of a RAGGED batch at LLaMA-3-8B widths, config.mm355_ragged_pass on a model whose functional.VARIANTS["ragged_pass_attn"]
is flipped between the two arms: off = one decoder_prefill per sequence (today's default), on = ONE functional.decoder_extend_ragged pass.
Cells: B in {4, 16} x mean length in {64, 576, 2048} rows with a +-12 % spread (seeded), through the model's _prefill_batch; and one
follow-up-turn cell per B: 64 new rows on caches of 500 - 700 rows through _extend_batch (off: one decoder_extend per sequence).
Both arms run in this process, interleaved (off, on, off, on, ..), after one warm-up run of each; a run is timed with the host clock between
two device synchronises; the table gives the median and the range of REPS runs.  The arms' outputs are compared at every size timed (the
last hidden row of every sequence: max |on - off| / max |off| and ||on - off|| / ||off||).  Set LAYERS=32 for the whole 8B decoder,
CELLS="4x64,16x576,turn4" for a subset."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from metamorph_amd import functional as F
from metamorph_amd.factory import LLAMA3_8B, build_model
from metamorph_amd.model.language_model.metamorph_llama import HipKVCache

dev = torch.device("cuda:0")
layers = int(os.environ.get("LAYERS", 8))
reps = int(os.environ.get("REPS", 5))
model = build_model(dict(LLAMA3_8B, num_hidden_layers=layers), dict(num_hidden_layers=1), num_image_tokens=256, max_length=4096,
                    device=dev, init_on_device=True).eval()
model.config.mm355_ragged_pass = True
h = 4096


def lengths(B, mean, seed):
    """B seeded lengths within +-12 % of `mean`, both ends of the range present"""
    rng = np.random.default_rng(seed)
    ls = np.rint(mean * (1 + 0.12 * rng.uniform(-1, 1, B))).astype(int)
    ls[0], ls[-1] = round(mean * 0.88), round(mean * 1.12)
    return [int(n) for n in ls]


def timed(run):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = run()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def ab(run):
    """run(on) -> last hidden rows; -> ({arm: [seconds]}, (max, L2) relative difference of the arms' outputs)"""
    ts, outs = {False: [], True: []}, {}
    for on in (False, True):                                  # warm-up: code objects, workspaces, the allocator's blocks
        F.set_variant("ragged_pass_attn", on)
        outs[on] = timed(lambda: run(on))[1].float()
    for _ in range(reps):
        for on in (False, True):
            F.set_variant("ragged_pass_attn", on)
            ts[on].append(timed(lambda: run(on))[0])
    F.set_variant("ragged_pass_attn", True)
    d = outs[True] - outs[False]
    return ts, (float(d.abs().max() / outs[False].abs().max()), float(d.norm() / outs[False].norm()))


def row(name, rows, ts, diff):
    off, on = (statistics.median(ts[a]) * 1e3 for a in (False, True))
    rng = lambda a: f"{min(ts[a]) * 1e3:.1f} - {max(ts[a]) * 1e3:.1f}"      # noqa: E731
    print(f"| {name} | {rows} | {off:.1f} ({rng(False)}) | {on:.1f} ({rng(True)}) | {off / on:.2f} x | {diff[0]:.1e} / {diff[1]:.1e} |", flush=True)


def prompt_cell(B, mean):
    lens = lengths(B, mean, seed=B * 10007 + mean)
    seqs = [(torch.randn(n, h, device=dev) * 0.02).bfloat16() for n in lens]

    def run(on):
        with torch.no_grad():
            outs = model._prefill_batch(seqs, HipKVCache(capacity=max(lens) + 8), stepper=False)
        return torch.stack([o[-1] for o in outs], 0)
    ts, diff = ab(run)
    row(f"prompts {B} x {mean} +-12 % ({min(lens)} - {max(lens)})", sum(lens), ts, diff)


def turn_cell(B, new=64):
    past = [int(n) for n in np.random.default_rng(B).integers(500, 701, B)]
    past[0], past[-1] = 500, 700
    cache = HipKVCache(capacity=max(past) + new + 8)
    with torch.no_grad():
        F.set_variant("ragged_pass_attn", False)
        model._prefill_batch([(torch.randn(n, h, device=dev) * 0.02).bfloat16() for n in past], cache, stepper=False)
    x = (torch.randn(B, new, h, device=dev) * 0.02).bfloat16()

    def run(on):
        cache.kv.set_lengths(past)                            # (the turn again on the same cached rows)
        with torch.no_grad():
            return model._extend_batch(x, cache)[:, -1]
    ts, diff = ab(run)
    row(f"turn {B} x {new} new rows on 500 - 700 cached", B * new, ts, diff)


cells = os.environ.get("CELLS", "4x64,16x64,4x576,16x576,4x2048,16x2048,turn4,turn16").split(",")
print(f"{layers} decoder layers at 8B widths, bf16 weights and cache, {reps} interleaved runs per arm after one warm-up each; ms: median (range)")
print("| cell | packed rows | off: per sequence, ms | on: one ragged pass, ms | off / on | outputs: max / L2 rel diff |")
print("|---|---|---|---|---|---|", flush=True)
for c in cells:
    if c.startswith("turn"):
        turn_cell(int(c[4:]))
    else:
        B, mean = (int(v) for v in c.split("x"))
        prompt_cell(B, mean)
