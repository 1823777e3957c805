#!/usr/bin/env python3
"""ms per step of greedy_decode's two loops at LLaMA-3-8B widths: the one-sequence host loop (head, argmax and embedding lookup on the
host side of every token) and the device-resident loop of a batch (functional.GreedyLoopGraph) at B = 1, 4, 8, 16 and at
config.mm355_greedy_poll_steps 1 and 8.  Per-step cost = the difference of two run lengths (the prompt pass cancels).
--sample: the device loop's step with and without the sampler (mm355_philox_uniform_rows + mm355_sample_rows_f32 in place of the argmax)
at B = 1 and 16 for no filter, top-p 0.9 and top-k 50 + top-p 0.9, the greedy step re-measured before each of them, twice over, and the tails
alone on the loop's last logits (device events).  Set LAYERS=32 for the whole 8B decoder."""
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


def per_step(B, device_loop, poll=None, **kw):
    emb = (torch.randn(B, L0, h, device=dev) * 0.02).bfloat16()
    old = F.set_variant("greedy_loop_b1", device_loop)
    if poll is not None:
        model.config.mm355_greedy_poll_steps = poll
    try:
        run = lambda n: model.greedy_decode(None, None, emb, max_new_tokens=n, eos_token_id=(), **kw)      # noqa: E731 (no eos: every run takes n steps)
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


def sample_table():
    from metamorph_amd import ops
    settings = (("no filter", dict(top_k=0, top_p=1.0)), ("top-p 0.9", dict(top_k=0, top_p=0.9)), ("top-k 50 + top-p 0.9", dict(top_k=50, top_p=0.9)))
    print(f"{layers} decoder layers at 8B widths, V = {model.config.vocab_size}, prompts of {L0} rows, {new} new tokens, temperature 0.7, poll 8; "
          f"the greedy step is re-measured before every sampled one", flush=True)
    for B in [int(b) for b in os.environ.get("BATCHES", "1,16").split(",")]:
        per_step(B, True, 8)                                 # (the first measurement of a batch size reads low or high: discarded)
        for rnd in (1, 2):                                   # two rounds: the spread of the greedy figures is the noise of the percentages
            for name, kw in settings:
                g = per_step(B, True, 8)
                t = per_step(B, True, 8, do_sample=True, temperature=0.7, seed=1, **kw)
                print(f"B={B:2d} round {rnd} {name:21s}: greedy {g*1e3:7.3f} ms/step, sampled {t*1e3:7.3f} ms/step ({(t/g-1)*100:+.1f} %)", flush=True)
        loop = model._greedy_loop                            # its static logits: the last step's
        ws = ops.argmax_rows_ws(B, loop.C, dev)
        print(f"B={B:2d} tails alone on the last logits: argmax_rows {tail_us(lambda: ops.argmax_rows(loop.logits, out=loop.tok, ws=ws)):6.1f} us, "
              f"philox_uniform_rows {tail_us(lambda: ops.philox_uniform_rows(1, loop.stream_ids, loop.state[2], out=loop.u)):6.1f} us, sample_rows "
              + ", ".join(f"{name} {tail_us(lambda: ops.sample_rows(loop.logits, 1 / 0.7, kw['top_k'], kw['top_p'], loop.u, out=loop.tok)):6.1f} us"
                          for name, kw in settings), flush=True)


if "--sample" in sys.argv[1:]:
    sample_table()
    sys.exit(0)
print(f"{layers} decoder layers at 8B widths, prompts of {L0} rows, {new} new tokens (per step: difference of {new} and {2 * new} tokens)", flush=True)
t = per_step(1, False)
print(f"host loop     B= 1        : {t*1e3:7.3f} ms/step", flush=True)
for B in [int(b) for b in os.environ.get("BATCHES", "1,4,8,16").split(",")]:
    for poll in (1, 8):
        t = per_step(B, True, poll)
        print(f"device loop   B={B:2d} poll={poll} : {t*1e3:7.3f} ms/step = {t/B*1e3:.3f} ms per token and sequence", flush=True)
