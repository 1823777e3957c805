"""The host side of the device token loops without a device: GreedyLoopGraph.run and BeamLoopGraph.run with a stub in place of the step and
of the device's `live` counter.  The loop launches its steps blind and looks at `live` every `poll` steps; these tests fix when it looks
and when it stops, the bound the GPU tests state as host_reads <= ceil(steps / poll) + 1."""
import math

import pytest
import torch

from metamorph_amd import functional as F


class Live:
    """`live` of a loop whose sequences all finish in step `dies_at` (None: never): logs the step count of every read"""

    def __init__(self, loop, dies_at):
        self.loop, self.dies_at, self.reads = loop, dies_at, []

    def _value(self):
        return 0 if self.dies_at is not None and self.loop.steps >= self.dies_at else 1

    def item(self):
        self.reads.append(self.loop.steps)
        return self._value()

    def cpu(self):                                           # (the final read of the results: the whole state, not a poll)
        return torch.tensor([0], dtype=torch.int32)


def stub_loop(kind, n_steps, poll, dies_at):
    """a loop of `kind` that may take n_steps steps, built without a device: run() with _tail and _step stubbed"""
    loop = object.__new__(F.GreedyLoopGraph if kind == "greedy" else F.BeamLoopGraph)
    loop.poll, loop.steps, loop.host_reads, loop.processors, loop.on_tail = poll, 0, 0, None, None
    loop._tail = lambda x: None
    loop._step = lambda: None
    live = Live(loop, dies_at)
    if kind == "greedy":
        B = 2
        loop.max_new_tokens = n_steps
        loop.state = torch.zeros((len(F.GREEDY_STATE), B), dtype=torch.int32)
        loop.state[3] = 1                                    # every sequence done: what the device leaves behind
        loop.tok_log = torch.zeros((B, n_steps + 1), dtype=torch.int32)
        loop.z_log = torch.zeros((B, n_steps + 1, 4))
        loop.live = live
    else:
        loop.max_new_tokens = n_steps + 1                    # (the first tail generates id 1: max_new_tokens - 1 steps)
        loop.state = {n: torch.from_numpy(a) for n, a in F.beam_state_host(2, loop.max_new_tokens).items()}
        loop.state["live"] = live
    return loop, live


@pytest.mark.parametrize("kind", ["greedy", "beam"])
@pytest.mark.parametrize("poll", [1, 3, 8])
def test_live_is_read_every_poll_steps_and_never_after_the_last(kind, poll):
    for n_steps in (0, 1, poll, poll + 1, 2 * poll, 5 * poll + 2):
        loop, live = stub_loop(kind, n_steps, poll, None)
        loop.run(torch.zeros(2, 4))
        assert loop.steps == n_steps
        assert live.reads == [s for s in range(1, n_steps + 1) if s % poll == 0 and s < n_steps], (n_steps, live.reads)
        assert loop.host_reads == len(live.reads) + 1 <= math.ceil(loop.steps / poll) + 1


@pytest.mark.parametrize("kind", ["greedy", "beam"])
@pytest.mark.parametrize("poll", [1, 3, 8])
def test_the_loop_stops_at_the_first_read_of_zero(kind, poll):
    n_steps = 4 * poll + 1
    for dies_at in (1, poll, poll + 1, 3 * poll, n_steps):
        loop, live = stub_loop(kind, n_steps, poll, dies_at)
        loop.run(torch.zeros(2, 4))
        stop = math.ceil(dies_at / poll) * poll              # the first look at or after the step that finished the last sequence
        assert loop.steps == min(stop, n_steps), (dies_at, loop.steps)
        assert live.reads == [s for s in range(poll, loop.steps + 1, poll) if s < n_steps]
        assert loop.host_reads == len(live.reads) + 1 <= math.ceil(loop.steps / poll) + 1


def test_the_beam_loop_calls_on_tail_after_every_tail():
    loop, _ = stub_loop("beam", 5, 3, None)
    seen = []
    loop.on_tail = lambda lp: seen.append(lp.steps)
    loop.run(torch.zeros(2, 4))
    assert seen == [0, 1, 2, 3, 4, 5]
