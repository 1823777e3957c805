"""CPU-only: the builders and the acceptance threshold of tests/kv_long_refs.py can tell right from wrong at the full lengths the GPU cases
use (131072 and 100003 keys):

  (a) the bf16-P emulation (fp32 scores, P rounded to bf16, fp32 sums, one bf16 rounding of the output -- the arithmetic of the MFMA forms)
      stays inside |got - ref| <= 2^-7 |ref| + 2^-20 on every builder;
  (b) each mutation of the formula -- a 64-key tile dropped, a tile counted twice, the key limit off by one in either direction, the needle
      read at j +- 1, the partials of two runs added without rescaling to a common maximum -- exceeds it on at least one builder;
  (c) the restated key-run rule gives the plans the GPU cases assert, and the needles land on the run edges.

Run with -s to see the measured figures."""
import pytest
import torch

import kv_long_refs as K

D = 128
LENS = [131072, 100003, 700, 0]
ROWS = 131072
X_PAST, X_N, X_HQ = [131072 - 17], 17, 4                       # the extend case: 68 packed rows, nsplit 64, tps 32
X_RUNS = K.extend_runs(1, X_N, X_HQ, 1, 131072)[:2]

_CASES = {}


def case(name):
    """(reference kind, arguments of the reference after fn / mutate) of a builder, made once"""
    if name not in _CASES:
        form, kind = name.split("/")
        if form == "decode":
            q, k, v = K.decode_inputs(kind, LENS, ROWS, 8, 1, D)
            _CASES[name] = (K.decode_ref, (q, k, v, LENS, 8, 1, D))
        else:
            q, k, v = K.extend_inputs(kind, X_PAST, X_N, ROWS, X_HQ, 1, D, X_RUNS)
            _CASES[name] = (K.extend_ref, (q, k, v, X_PAST, X_N, X_HQ, 1, D))
    return _CASES[name]


_REFS = {}


def ref(name):
    if name not in _REFS:
        fn, args = case(name)
        _REFS[name] = fn(*args)
    return _REFS[name]


BUILDERS = ["decode/flat", "decode/needle", "extend/flat", "extend/needle", "extend/beyond"]


def test_key_runs_restated():
    assert K.key_runs(2, 2048) == (64, 32) and X_RUNS == (64, 32)                 # 131072 keys, two row tiles: the cap of 64 runs
    assert K.key_runs(1, 63) == (13, 5)                                           # what the suite reached before: 63 tiles in runs of 5
    assert K.key_runs(128, 2048) == (1, 2048) and K.key_runs(6, 1564) == (43, 37)
    assert K.shared_runs(3, 1, 8, 1, 131072 - 64)[:2] == (64, 32)
    pos = K.extend_needle_keys(X_PAST[0], X_N, *X_RUNS)
    assert pos[:5] == [63, 64, 2047, 2048, 63 * 2048] and pos[5:] == [X_PAST[0] + 5, X_PAST[0] + 14, X_PAST[0] + 7]
    assert K.decode_needle_keys(131072) == [0, 255, 256, 1023, 1024, 130048, 131071, 65536]


def test_needle_rows_spell_the_key_that_was_read():
    out = ref("decode/needle")
    for b, L in enumerate(LENS[:3]):
        assert [K.spelled(out[b].view(8, D)[h], D) for h in range(8)] == K.decode_needle_keys(L)
    assert float(out[3].abs().max()) == 0                                         # the empty sequence: a zero row
    out = ref("extend/needle").view(X_N, X_HQ, D)
    pos = K.extend_needle_keys(X_PAST[0], X_N, *X_RUNS)
    for i in range(X_N):
        if i != 6:                                                                # (row 6's needle is row 14's own position: not visible)
            assert K.spelled(out[i, 0], D) == pos[i % 8], i
    assert 0.3 < float(out[6, 0, 0]) < 0.7                                        # no needle: every bit column near one half
    out = ref("extend/beyond").view(X_N, X_HQ, D)
    assert 0.3 < float(out[0, 0, 0]) < 0.7                                        # row 0 must not see its needle at past + 1
    for i in range(1, 8):
        assert K.spelled(out[i, 0], D) == X_PAST[0] + i                           # row i sees the key at its own position


@pytest.mark.parametrize("name", BUILDERS)
def test_emulation_stays_inside_the_threshold(name):
    fn, args = case(name)
    frac, rel = K.measure(fn(*args, fn=K.emulate_bf16p), ref(name))
    print(f"   bf16-P emulation on {name}: max rel err {rel:.3e}, {frac:.3f} of the bar")
    assert frac <= 1.0, (name, frac, rel)


MUTATIONS = [("drop_tile", 1000), ("double_tile", 1000), ("limit", 1), ("limit", -1), ("shift_v", 1), ("shift_v", -1),
             ("no_rescale", 32 * 64)]


@pytest.mark.parametrize("mutation", MUTATIONS, ids=[f"{n}{a:+d}" for n, a in MUTATIONS])
def test_every_mutation_exceeds_the_threshold_somewhere(mutation):
    over = {}
    for name in BUILDERS:
        fn, args = case(name)
        frac, _ = K.measure(fn(*args, mutate=mutation), ref(name))
        over[name] = round(frac, 2)
        if frac > 1.0 and name.startswith("extend"):                              # (the decode builders are cheap: show them all)
            break
    print(f"   {mutation}: error as a multiple of the bar {over}")
    assert max(over.values()) > 1.0, (mutation, over)


def test_a_dropped_tile_is_far_outside_on_flat():
    """the figure the threshold was chosen against: one of 2048 tiles missing moves a flat output several times the bar"""
    for name in ("decode/flat",):
        fn, args = case(name)
        frac, _ = K.measure(fn(*args, mutate=("drop_tile", 1000)), ref(name))
        print(f"   {name} without tile 1000: {frac:.1f} x the bar")
        assert frac > 4.0


def test_quantised_rows_keep_their_needles():
    q, k, v = K.decode_inputs("needle", [700], 704, 8, 1, D)
    k8, ks = K.quantize_rows_kv8(k, 1, D, seed=5)
    kd = (k8.view(torch.float8_e4m3fn).float().view(1, 704, 1, D) * ks[..., None]).view(1, 704, D)
    assert float(kd[0, 255, 1]) * D ** -0.5 * 8 > 38 and bool(torch.isfinite(kd).all())
    assert bool(((ks == torch.ldexp(torch.ones(()), torch.log2(ks).round().int()))).all())
