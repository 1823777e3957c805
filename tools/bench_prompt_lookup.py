#!/usr/bin/env python3
"""Prompt-lookup speculative decoding (greedy_decode(prompt_lookup_num_tokens=K), functional.SpecGreedyLoopGraph) at LLaMA-3-8B widths with
random weights: ms per step of the speculative loop for K in {3, 7, 15} and B in {1, 4} next to the plain device loop's step, measured in
one process with the runs alternating, and the break-even acceptance = speculative step / plain step: the mean number of ids a step must
emit for the speculative loop to be as fast as the plain one.  The step's shape is fixed, so its cost does not depend on what is
accepted: it is measured with empty lookup ids (no drafts, one id per step; per-step cost = the difference of two run lengths, the
prompt pass cancels).  Then two runs whose lookup ids hold an earlier run's output: the plain run's, and the speculative loop's own from
a run without lookup ids.  A random-weight model decides on near ties, so the speculative step (another row count, another GEMV /
GEMM route) soon leaves the plain run's ids and the first finds little; the second repeats its own decisions, so every draft the
lookup finds is right.  Reported: steps, the mean of acc_log (ids per step) and ms per emitted id of the loop alone (a run of one
new token subtracted).
LAYERS=8 for a quick look; the default is the whole 32-layer decoder."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from metamorph_amd import functional as F
from metamorph_amd.factory import LLAMA3_8B, build_model

dev = torch.device("cuda:0")
layers = int(os.environ.get("LAYERS", 32))
L0, new = int(os.environ.get("PROMPT", 64)), int(os.environ.get("NEW", 64))
model = build_model(dict(LLAMA3_8B, num_hidden_layers=layers), dict(num_hidden_layers=1), num_image_tokens=256, max_length=4096,
                    device=dev, init_on_device=True).eval()
model.config.mm355_greedy_poll_steps = 8
h = 4096
TEXT = dict(start_image_token_id=-1, end_image_token_id=-2, eos_token_id=())      # text only, and every run takes all its tokens


def timed(emb, n, **kw):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = model.greedy_decode(None, None, emb, max_new_tokens=n, **TEXT, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def per_step(emb, **kw):
    """seconds per step: the difference of a run of 2 * new and one of new tokens"""
    timed(emb, 2, **kw)
    return (timed(emb, 2 * new, **kw)[0] - timed(emb, new, **kw)[0]) / new


old = F.set_variant("greedy_loop_b1", True)                  # one sequence through the device loop in the plain runs too
print(f"{layers} decoder layers at 8B widths, V = {model.config.vocab_size}, prompts of {L0} rows, {new} new tokens, poll 8", flush=True)
try:
    for B in [int(b) for b in os.environ.get("BATCHES", "1,4").split(",")]:
        torch.manual_seed(B)
        emb = (torch.randn(B, L0, h, device=dev) * 0.02).bfloat16()
        per_step(emb)                                        # (the first measurement of a batch size reads low or high: discarded)
        for K in [int(k) for k in os.environ.get("DRAFTS", "3,7,15").split(",")]:
            rows = []
            for rnd in (1, 2):                               # two rounds, plain and speculative alternating
                p = per_step(emb)
                s = per_step(emb, prompt_lookup_num_tokens=K, prompt_lookup_ids=[])
                rows.append((p, s))
                print(f"B={B} K={K:2d} round {rnd}: plain {p*1e3:7.3f} ms/step, speculative ({B * (K + 1):2d} rows) {s*1e3:7.3f} ms/step, "
                      f"break-even {s/p:.2f} ids per step", flush=True)
            t1 = timed(emb, 1)[0]
            tp, ids = timed(emb, new)
            t1s = timed(emb, 1, prompt_lookup_num_tokens=K, prompt_lookup_ids=[])[0]
            own = timed(emb, new, prompt_lookup_num_tokens=K, prompt_lookup_ids=[])[1]
            for what, src in (("the plain run's ids", ids), ("its own ids", own)):
                ts, got = timed(emb, new, prompt_lookup_num_tokens=K, prompt_lookup_ids=[t.tolist() for t in src])
                loop = model._greedy_loop
                acc = [a for log in loop.acc_log for a in log]
                same = sum(int(torch.equal(a, b)) for a, b in zip(src, got))
                print(f"B={B} K={K:2d} lookup ids = {what}: {loop.steps} steps for {new} ids, mean acc_log {sum(acc) / max(len(acc), 1):.2f}, "
                      f"{(ts - t1s) / new * 1e3:7.3f} ms per id and sequence against {(tp - t1) / new * 1e3:7.3f} plain; {same} of {B} "
                      f"sequences emit those ids to the end", flush=True)
finally:
    F.set_variant("greedy_loop_b1", old)
