"""Sampled decoding on the device: mm355_philox_uniform_rows against functional.philox_uniform_host integer for integer,
mm355_sample_rows_f32 against its fp64 host model functional.sample_row_host (bands of eps = 1e-4, see there), and the sampler inside
functional.GreedyLoopGraph: per-step draws in eager mode, replay / eager / polling as one computation, top_k = 1 as the greedy loop."""
import numpy as np
import pytest
import torch

import test_greedy_batch_gpu as G  # noqa: E402  (the tiny fixture models)
from sample_refs import DEV, FAMILIES, SETTINGS, U_MAX, check_row, device_draw, family  # noqa: E402  (shared with the edge tests)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R,C", [(R, C) for C in (37, 1000) for R in (1, 3, 17)] + [(3, 128258)])
def test_sample_rows_against_the_host_model(R, C):
    settings = [SETTINGS[1], SETTINGS[3]] if C == 128258 else SETTINGS
    g = torch.Generator().manual_seed(100003 * R + C)
    single, drawn, widest_flat = 0, 0, 0
    for name in FAMILIES:
        x = family(name, R, C, g)
        rows = x.double().numpy()
        for T, top_k, top_p in settings:
            u_drawn = (torch.randint(0, 2 ** 24, (R,), generator=g).float() * 2.0 ** -24)
            for kind, u in (("drawn", u_drawn), ("0", torch.zeros(R)), ("max", torch.full((R,), U_MAX))):
                out, stats = device_draw(x, T, top_k, top_p, u)
                for r in range(R):
                    n = check_row(rows[r], T, top_k, top_p, float(u[r]), out[r], stats[r, 0], stats[r, 1], (name, T, top_k, top_p, kind, r))
                    if name == "peaked" and kind == "drawn":
                        drawn += 1
                        single += n == 1
                    if name == "flat":
                        widest_flat = max(widest_flat, n)
    print(f"   R={R} C={C}: peaked rows with one candidate {single}/{drawn}, widest flat candidate set {widest_flat}")
    # the set check must not hide a wrong pick
    assert single >= 0.95 * drawn, (single, drawn)
    if C == 128258:
        assert widest_flat <= 32, widest_flat


def test_top_k_1_is_the_argmax_and_nonfinite_maxima_follow_it():
    from metamorph_amd import ops
    g = torch.Generator().manual_seed(5)
    for C in (37, 1000, 128258):
        x = torch.randn(3, C, generator=g) * 3.0
        x[:, 7] = x.max() + 1.0                                  # (a unique maximum also where 128258 fp32 draws repeat a value)
        want = ops.argmax_rows(x.to(DEV).contiguous()).cpu().tolist()
        for u in (0.0, 0.37, U_MAX):
            out, stats = device_draw(x, 0.7, 1, 1.0, torch.full((3,), u))
            assert out == want == [7, 7, 7] and stats[:, 1].tolist() == [1.0] * 3 and stats[:, 0].tolist() == x[:, 7].double().tolist()
        # NaN, +inf and all -inf: the argmax rule, stats = (m, 0)
        y = torch.randn(4, C, generator=g)
        y[0, 5], y[0, C - 2], y[0, 3] = float("nan"), float("nan"), float("inf")
        y[1, C - 1], y[1, 11] = float("inf"), 50.0
        y[2, 9], y[2, 20] = float("inf"), float("inf")
        y[3] = float("-inf")
        want = ops.argmax_rows(y.to(DEV).contiguous()).cpu().tolist()
        assert want == [5, C - 1, 9, 0]
        for T, top_k, top_p in SETTINGS:
            out, stats = device_draw(y, T, top_k, top_p, torch.full((4,), 0.6))
            assert out == want, (C, T, top_k, top_p, out)
            assert np.isnan(stats[0, 0]) and stats[1:, 0].tolist() == [np.inf, np.inf, -np.inf] and stats[:, 1].tolist() == [0.0] * 4


def test_sample_rows_is_reproducible_and_rows_are_independent():
    g = torch.Generator().manual_seed(17)
    for C in (1000, 128258):
        x = torch.randn(17, C, generator=g) * 2.0
        u = torch.rand(17, generator=g)
        for T, top_k, top_p in (SETTINGS[0], SETTINGS[3]):
            out, stats = device_draw(x, T, top_k, top_p, u)
            out2, stats2 = device_draw(x, T, top_k, top_p, u)
            assert out == out2 and np.array_equal(stats, stats2)
            for r in (0, 8, 16):
                o1, s1 = device_draw(x[r:r + 1], T, top_k, top_p, u[r:r + 1])
                assert o1 == [out[r]] and np.array_equal(s1[0], stats[r]), (C, r)


@pytest.mark.parametrize("R", [1, 17])
def test_philox_uniform_rows_equal_the_host(R):
    from metamorph_amd import functional as F, ops
    g = torch.Generator().manual_seed(R)
    for seed in (0, 1, 0x299f31d0a4093822, 2 ** 64 - 1):
        ids = torch.randint(0, 2 ** 31 - 1, (R,), generator=g).to(torch.int32)
        ctr = torch.randint(0, 2 ** 31 - 1, (R,), generator=g).to(torch.int32)
        ctr[0] = 0
        ctr[-1] = 2 ** 31 - 1 if R > 1 else 0
        ids[0] = 0
        for c in (ctr, torch.full((R,), 2 ** 31 - 1, dtype=torch.int32)):
            u = ops.philox_uniform_rows(seed, ids.to(DEV), c.to(DEV)).cpu()
            assert u.dtype == torch.float32 and bool(((u >= 0) & (u < 1)).all())
            want = [F.philox_uniform_host(seed, int(ids[r]), int(c[r])) for r in range(R)]
            assert u.double().tolist() == want, seed                 # (a multiple of 2^-24 below 1: exact in fp32)


# ------------------------------------------------------------------ the loop
SAMPLE = dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9)


def _record(monkeypatch, model):
    """wrap ops.sample_rows as the loop calls it: per call the sequences' total_out, the logits, u, (tau, Z) and the drawn ids"""
    from metamorph_amd import functional as F, ops
    rec = []
    orig = ops.sample_rows

    def wrapped(logits, inv_t, top_k, top_p, u, out=None, ws=None):
        stats = torch.empty((logits.shape[0], 2), device=logits.device)
        total_out = model._greedy_loop.state[2].clone()
        tok = orig(logits, inv_t, top_k, top_p, u, out=out, stats=stats, ws=ws)
        rec.append(dict(total_out=total_out.cpu().tolist(), logits=logits.cpu().double().numpy(), u=u.cpu().double().tolist(),
                        stats=stats.cpu().double().numpy(), tok=tok.cpu().tolist(), args=(inv_t, top_k, top_p)))
        return tok
    monkeypatch.setattr(F.ops, "sample_rows", wrapped)
    return rec


def _eager(fn):
    from metamorph_amd import functional as F
    old = F.set_variant("decode_graph", False)
    try:
        return fn()
    finally:
        F.set_variant("decode_graph", old)


def test_every_step_of_the_eager_loop_draws_what_the_host_model_allows(monkeypatch):
    """(a) and (d): three copies of the image-mode prompt; every u is philox_uniform_host(seed, b, total_out_b), every id satisfies
    sample_row_host on the logits of its step; the same seed repeats the run, another seed draws other uniforms."""
    from metamorph_amd import functional as F
    g, model = G._fixture_model("image_prompt")
    rec = _record(monkeypatch, model)
    kw = G._batch_kw(g, 3, max_new_tokens=int(g["max_new_tokens"]), **SAMPLE)
    ids, embs = _eager(lambda: model.generate(**kw, seed=1234))
    loop = model._greedy_loop
    assert loop.seed == 1234 and loop.sampler == (1 / 0.7, 50, 0.9) and not loop.graphs
    assert len(rec) == loop.steps + 1 and len(ids) == len(embs) == 3
    first = list(rec)
    for step in first:
        assert step["args"] == (1 / 0.7, 50, 0.9)
        for b in range(3):
            assert step["u"][b] == F.philox_uniform_host(1234, b, step["total_out"][b]), (b, step["total_out"])
            check_row(step["logits"][b], 0.7, 50, 0.9, step["u"][b], step["tok"][b], step["stats"][b, 0], step["stats"][b, 1], ("loop", b))
    assert any(e.shape[0] == 4 for e in embs)                    # image rows are emitted under sampling as well
    del rec[:]
    ids2, embs2 = _eager(lambda: model.generate(**kw, seed=1234))
    assert [t.tolist() for t in ids2] == [t.tolist() for t in ids] and all(torch.equal(a, b) for a, b in zip(embs2, embs))
    assert [s["u"] for s in rec] == [s["u"] for s in first]
    del rec[:]
    kw["max_new_tokens"] = 1                                     # (the first uniforms are all that is compared from here on)
    _eager(lambda: model.generate(**kw, seed=1235))
    assert model._greedy_loop.seed == 1235 and rec[0]["u"] != first[0]["u"]
    # the stream id, not the place in the batch, names a sequence's draws
    del rec[:]
    _eager(lambda: model.generate(**kw, seed=1234, stream_ids=[2, 0, 1]))
    assert rec[0]["u"] == [first[0]["u"][2], first[0]["u"][0], first[0]["u"][1]]


def _sampled_run(poll=None, graph=True, **kw):
    from metamorph_amd import functional as F
    _, model = G._diverge_model()
    emb, mask = G._diverge_inputs(G.DIVERGE_SEEDS)
    old = F.set_variant("decode_graph", graph)
    if poll is not None:
        model.config.mm355_greedy_poll_steps = poll
    try:
        ids, zs = model.greedy_decode(None, mask, emb, max_new_tokens=G.MAX_NEW, output_image=True, **kw)
    finally:
        F.set_variant("decode_graph", old)
        if poll is not None:
            del model.config.mm355_greedy_poll_steps
    return [t.tolist() for t in ids], zs, model._greedy_loop


def test_sampled_replay_eager_and_polling_are_one_computation():
    """(b): five left-padded prompts, a fixed seed: captured replay, eager launches and two poll values give the same ids and image rows"""
    kw = dict(SAMPLE, seed=99)
    ids, zs, loop = _sampled_run(**kw)
    assert loop.graphs and loop.sampler is not None and loop.seed == 99
    for graph, poll in ((True, 1), (True, 5), (False, 8)):
        i2, z2, l2 = _sampled_run(poll=poll, graph=graph, **kw)
        assert i2 == ids and all(torch.equal(a, b) for a, b in zip(z2, zs)), (graph, poll)
        assert bool(l2.graphs) == graph and l2.poll == poll
    i3, _, _ = _sampled_run(**dict(kw, seed=100, top_k=0, top_p=1.0, temperature=1.5))
    assert i3 != ids                                             # (the seed and the settings reach the device)


def test_top_k_1_and_temperature_0_are_the_greedy_loop():
    """(c) and (e)"""
    greedy, gz, gl = _sampled_run()
    assert gl.sampler is None and gl.seed is None
    ids, zs, loop = _sampled_run(do_sample=True, temperature=0.7, top_k=1, seed=3)
    assert loop.sampler == (1 / 0.7, 1, 1.0)
    assert ids == greedy and all(torch.equal(a, b) for a, b in zip(zs, gz))
    for kw in (dict(do_sample=True, temperature=0.0, top_k=5, top_p=0.5, seed=3), dict(do_sample=True), dict(do_sample=False, temperature=0.7)):
        ids, zs, loop = _sampled_run(**kw)
        assert loop.sampler is None, kw
        assert ids == greedy and all(torch.equal(a, b) for a, b in zip(zs, gz)), kw


def test_one_sequence_samples_through_the_device_loop():
    g, model = G._fixture_model("text")
    model._greedy_loop = None
    kw = G._batch_kw(g, 1, max_new_tokens=6, **SAMPLE)
    out, emb = model.generate(**kw, seed=8)
    loop = model._greedy_loop
    assert loop is not None and loop.sampler is not None and loop.cache.batch == 1
    assert isinstance(out, list) and len(out) == 1 and out[0].dtype == torch.int32
    out2, _ = model.generate(**kw, seed=8)
    assert out2[0].tolist() == out[0].tolist()
