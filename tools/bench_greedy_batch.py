#!/usr/bin/env python3
"""ms per step of greedy_decode's two loops at LLaMA-3-8B widths: the one-sequence host loop (head, argmax and embedding lookup on the
host side of every token) and the device-resident loop of a batch (functional.GreedyLoopGraph) at B = 1, 4, 8, 16 and at
config.mm355_greedy_poll_steps 1 and 8.  Per-step cost = the difference of two run lengths (the prompt pass cancels)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from metamorph_amd import functional as F
from metamorph_amd.factory import LLAMA3_8B, build_model

dev = torch.device("cuda:0")
layers = int(os.environ.get("LAYERS", 8))
L0, new = int(os.environ.get("PROMPT", 64)), int(os.environ.get("NEW", 64))
model = build_model(dict(LLAMA3_8B, num_hidden_layers=layers), dict(num_hidden_layers=1), num_image_tokens=256, max_length=4096,
                    device=dev, init_on_device=True).eval()
h = 4096


def per_step(B, device_loop, poll=None):
    emb = (torch.randn(B, L0, h, device=dev) * 0.02).bfloat16()
    old = F.set_variant("greedy_loop_b1", device_loop)
    if poll is not None:
        model.config.mm355_greedy_poll_steps = poll
    try:
        run = lambda n: model.greedy_decode(None, None, emb, max_new_tokens=n, eos_token_id=())      # noqa: E731 (no eos: every run takes n steps)
        run(2)
        ts = []
        for n in (new, 2 * new):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            run(n)
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    finally:
        F.set_variant("greedy_loop_b1", old)
        if poll is not None:
            del model.config.mm355_greedy_poll_steps
    return (ts[1] - ts[0]) / new


print(f"{layers} decoder layers at 8B widths, prompts of {L0} rows, {new} new tokens (per step: difference of {new} and {2 * new} tokens)", flush=True)
t = per_step(1, False)
print(f"host loop     B= 1        : {t*1e3:7.3f} ms/step", flush=True)
for B in [int(b) for b in os.environ.get("BATCHES", "1,4,8,16").split(",")]:
    for poll in (1, 8):
        t = per_step(B, True, poll)
        print(f"device loop   B={B:2d} poll={poll} : {t*1e3:7.3f} ms/step = {t/B*1e3:.3f} ms per token and sequence", flush=True)
