"""The CPU side of tests/test_sample_edges_gpu.py: which branch of select_key (metamorph_amd/csrc/sample.hip) every row of those
tests takes, by the fp32 mirror sample_refs.round0_occupancy; functional.sample_row_host against the sort-based hf_kept_set (and that
against transformers' warpers); and the cap on the host model's candidate sets under which a wrong pick cannot hide."""
import numpy as np
import pytest
import torch

import sample_refs as S


def _ids(cases):
    return [f"{c[0]}-{c[1]}" for c in cases]


def _selects(C, top_k, top_p):
    return (["count"] if 0 < top_k < C else []) + (["mass"] if top_p < 1.0 else [])


@pytest.mark.parametrize("name,C,R,seed", S.OVERFULL_CASES, ids=_ids(S.OVERFULL_CASES))
def test_every_overfull_row_takes_the_branch_it_is_meant_for(name, C, R, seed):
    x, sets = S.overfull_case(name, C, R, seed)
    assert x.dtype == torch.float32 and tuple(x.shape) == (R, C)
    want = S.BRANCHES[(name, C)]
    seen = {}
    for T, top_k, top_p, _ in sets:
        for r in range(R):
            occ = S.round0_occupancy(x[r].numpy(), S.f32(1.0 / T), top_k, S.f32(top_p))
            assert [o[0] for o in occ] == _selects(C, top_k, top_p), (T, top_k, top_p, occ)
            for i, (kind, b, n) in enumerate(occ):
                after_k = kind == "mass" and i == 1
                if name.startswith("finite_mask"):                   # every unmasked value in the top bin: exact, whatever 256 / span rounds to
                    assert (b, n) == (255, top_k if after_k else C - 7), (T, top_k, top_p, occ)
                if want is None:
                    assert n == (top_k if after_k else S.SMP_LIST + 1)
                elif want[(T, top_k, top_p)][i] == S.REREAD:
                    assert n >= S.REREAD_MIN, (T, top_k, top_p, r, occ)
                else:
                    assert n <= S.SMP_LIST, (T, top_k, top_p, r, occ)
                key = (T, top_k, top_p, kind)
                seen[key] = (min(seen.get(key, (n, n))[0], n), max(seen.get(key, (n, n))[1], n))
    print(f"   {name} C={C}: " + ", ".join(f"{k[3]} at {k[:3]}: n = {lo}" + (f" .. {hi}" if hi != lo else "") for k, (lo, hi) in seen.items()))


def test_the_boundary_pair_is_one_row_with_and_without_its_last_column():
    a, sa = S.overfull_case("finite_mask(-1e9)", 8199, 2, 8199)
    b, sb = S.overfull_case("finite_mask(-1e9)", 8200, 2, 8199)
    assert torch.equal(b[:, :8199], a) and bool((b[:, 8199].abs() < 20).all())
    assert int((a == -1e9).sum()) == int((b == -1e9).sum()) == 2 * 7
    for r in range(2):
        for T, top_k, top_p in S.SETTINGS[1:3]:
            assert [o[2] for o in S.round0_occupancy(a[r].numpy(), S.f32(1.0 / T), top_k, S.f32(top_p))] == [S.SMP_LIST]
            assert [o[2] for o in S.round0_occupancy(b[r].numpy(), S.f32(1.0 / T), top_k, S.f32(top_p))] == [S.SMP_LIST + 1]


def test_the_cases_hold_each_kind_of_reread():
    """a count select alone, a mass select alone, and a mass select after a count select with both on the re-read branch"""
    T, k, p = S.SETTINGS[3]
    assert (T, k, p) == (1.3, 40, 0.95)
    x, _ = S.overfull_case("plateau", 20011, 2, 20011)
    for r in range(2):
        occ = S.round0_occupancy(x[r].numpy(), S.f32(1.0 / T), k, S.f32(p))
        assert [o[0] for o in occ] == ["count", "mass"] and all(o[2] >= S.REREAD_MIN for o in occ), occ
        assert occ[0][1] == occ[1][1]                                # (the plateau's bin both times)
    alone = {kind: [nc for nc, br in S.BRANCHES.items() if br and any(v == [S.REREAD] and _selects(nc[1], s[1], s[2]) == [kind]
                                                                     for s, v in br.items())] for kind in ("count", "mass")}
    assert alone["count"] and alone["mass"], alone


def test_the_key_lo_row_rereads_a_bin_that_holds_values_top_k_refused():
    from metamorph_amd import functional as F
    x, ((T, top_k, top_p, _),) = S.keylo_case()
    C = x.shape[1]
    for r in range(x.shape[0]):
        row = x[r].numpy()
        occ = S.round0_occupancy(row, S.f32(1.0 / T), top_k, S.f32(top_p))
        assert occ == [("count", 255, C - 7), ("mass", 255, top_k)] and top_k >= S.REREAD_MIN and C - 7 - top_k > 0, occ
        _, lo, hi, _ = F.sample_row_host(row.astype(np.float64), S.f32(1.0 / T), top_k, S.f32(top_p), 0.5, eps=0.0)
        hf = S.hf_kept_set(row, S.f32(1.0 / T), top_k, S.f32(top_p))
        assert lo == hi and np.array_equal(row >= lo, hf) and 1000 < int(hf.sum()) < top_k


def test_mirror_on_rows_worked_out_by_hand():
    # m = 8, fmn = -8: scale = 16, the digit of x is 255 - min(floor((8 - x) * 16), 255); -inf -> 0
    row = np.array([8.0, 7.95, 7.0, 0.0, -7.9, -8.0, -np.inf, -np.inf], dtype=np.float32)
    assert S.digit0(row, 8.0, 16.0).tolist() == [255, 255, 239, 127, 1, 0, 0, 0]
    assert S.round0_occupancy(row, 1.0, 0, 1.0) == []
    assert S.round0_occupancy(row, 1.0, 2, 1.0) == [("count", 255, 2)]
    assert S.round0_occupancy(row, 1.0, 3, 1.0) == [("count", 239, 1)]
    assert S.round0_occupancy(row, 1.0, 7, 1.0) == [("count", 0, 3)]                # the 7th largest is -inf: the bin of fmn and -inf
    # weights 1, e^-0.05 = 0.951, e^-1 = 0.368, e^-8, ...: Z = 2.3195, the top bin holds 0.841 of it
    assert S.round0_occupancy(row, 1.0, 0, 0.5) == [("mass", 255, 2)]
    assert S.round0_occupancy(row, 1.0, 0, 0.9) == [("mass", 239, 1)]
    assert S.round0_occupancy(row, 1.0, 7, 0.9) == [("count", 0, 3), ("mass", 239, 1)]
    assert S.round0_occupancy(row, 1.0, 2, 0.9) == [("count", 255, 2), ("mass", 255, 2)]
    assert S.round0_occupancy(row, 1.0, 3, 0.9999) == [("count", 239, 1), ("mass", 239, 1)]
    # no select: all equal, a non-finite maximum
    assert S.round0_occupancy(np.full(9, 1.25, dtype=np.float32), 1.0, 3, 0.9) == []
    assert S.round0_occupancy(np.array([0.0, np.inf], dtype=np.float32), 1.0, 1, 0.9) == []
    assert S.round0_occupancy(np.array([0.0, np.nan], dtype=np.float32), 1.0, 1, 0.9) == []
    assert S.round0_occupancy(np.full(4, -np.inf, dtype=np.float32), 1.0, 1, 0.9) == []
    assert [S.wscale_bits(C) for C in (37, 1 << 22, (1 << 22) + 1, 1 << 30)] == [40, 40, 39, 32]


@pytest.mark.parametrize("C", S.POINT_CS)
def test_point_rows_cover_the_walk_edges_and_their_top_k_select(C):
    span_w, chunk = S.walk_geometry(C)
    assert (span_w, chunk) == ((8192, 512) if C == 128258 else (1024, 64))
    sets = S.point_sets(C)
    assert len(sets) >= 3 and all(len(c) == 5 == len(set(c)) and c == sorted(c) and 0 <= c[0] and c[-1] < C for c in sets)
    edges = S.walk_edges(C)
    assert set(edges) <= set(c for cols in sets for c in cols)
    assert {0, C - 1} <= set(edges) and all(e in edges for e in (63, 64, 511, 512, C - 65, C - 64, span_w) if 0 <= e < C)
    if C == 128258:                                                  # the last wave's span, and two columns of its chunk that C cuts short
        assert 15 * span_w in edges and (C - 1) // chunk * chunk + chunk > C and (C - 64) // chunk == (C - 1) // chunk
    for cols in sets:
        row = S.points(cols)(1, C)[0].numpy()
        assert row.dtype == np.float32 and np.nonzero(row == 0.0)[0].tolist() == cols and int(np.isinf(row).sum()) == C - 5
        assert S.round0_occupancy(row, 1.0, 0, 1.0) == []
        (kind, b, n), = S.round0_occupancy(row, 1.0, 8, 1.0)         # span = 0: scale = 0, every finite value in bin 255, -inf in bin 0
        assert (kind, b, n) == ("count", 0, C - 5)
        assert (n > S.SMP_LIST) == (C >= 8200)


@pytest.mark.parametrize("name", S.TEMP_FAMILIES)
@pytest.mark.parametrize("C", S.TEMP_CS)
def test_temperature_rows_underflow_or_flatten_and_stay_on_the_list(C, name):
    x, sets = S.temperature_case(name, C)
    bits = S.wscale_bits(C)
    for T, top_k, top_p, _ in sets:
        for r in range(S.TEMP_R):
            row = x[r].numpy()
            occ = S.round0_occupancy(row, S.f32(1.0 / T), top_k, S.f32(top_p))
            assert [o[0] for o in occ] == _selects(C, top_k, top_p) and all(o[2] <= S.SMP_LIST for o in occ), occ
            fin = row[row > -np.inf].astype(np.float64)
            fixed = np.floor(np.exp((fin - fin.max()) * S.f32(1.0 / T)) * 2.0 ** bits)
            if T < 1:                                                # most fixed-point weights of the mass select are 0
                assert (fixed == 0).mean() > 0.5, (T, (fixed == 0).mean())
            else:                                                    # nearly flat: the lightest finite column within e^-2.5 of the heaviest
                assert fixed.min() > 0.08 * 2.0 ** bits, (T, fixed.min() * 2.0 ** -bits)


# ------------------------------------------------------------------------------------------------ the host model against HF's order

@pytest.mark.parametrize("C", [37, 1000])
def test_hf_kept_set_is_what_the_transformers_warpers_keep(C):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    rng = np.random.default_rng(C + 1)
    settings = S.SETTINGS + S.TEMP_SETTINGS + [(0.7, 5, 0.5), (1.0, C + 3, 0.9)]
    for masked in (False, True):
        for T, top_k, top_p in settings:
            x = rng.standard_normal(C) * 3.0
            if masked:
                x[rng.random(C) < 0.3] = -np.inf
                x[C // 2] = 0.25
            s = torch.from_numpy(x)[None]
            if T != 1.0:
                s = TemperatureLogitsWarper(T)(None, s)
            if top_k:
                s = TopKLogitsWarper(top_k)(None, s)
            if top_p < 1.0:
                s = TopPLogitsWarper(top_p)(None, s)
            want = torch.isfinite(s[0]).numpy()
            assert np.array_equal(S.hf_kept_set(x, 1.0 / T, top_k, top_p), want), (masked, T, top_k, top_p)


@pytest.mark.parametrize("name,C,R,seed", S.OVERFULL_CASES, ids=_ids(S.OVERFULL_CASES))
def test_host_model_keeps_what_hf_keeps_on_the_overfull_rows(name, C, R, seed):
    """{x >= tau} of sample_row_host (without its -inf entries, which weigh nothing) is hf_kept_set; on the plateau the model keeps the
    whole tie where HF's sort cuts through it, and differs nowhere else"""
    from metamorph_amd import functional as F
    x, sets = S.overfull_case(name, C, R, seed)
    rows = x.double().numpy()
    for T, top_k, top_p, _ in sets:
        for r in range(R):
            _, lo, hi, _ = F.sample_row_host(rows[r], S.f32(1.0 / T), top_k, S.f32(top_p), 0.5, eps=0.0)
            assert lo == hi
            model = (rows[r] >= lo) & (rows[r] > -np.inf)
            hf = S.hf_kept_set(rows[r], S.f32(1.0 / T), top_k, S.f32(top_p))
            if name in S.TIE_FREE:
                assert np.array_equal(model, hf), (T, top_k, top_p, r, int(model.sum()), int(hf.sum()))
            else:
                assert not (hf & ~model).any() and bool((rows[r][model & ~hf] == S.PLATEAU).all()), (T, top_k, top_p, r)
                assert bool(model.any()) and int(model.sum()) in (int(hf.sum()), S.PLATEAU_N + S.PLATEAU_TOP, C)


# ------------------------------------------------------------------------------------------------ the set check must not hide a wrong pick

def test_candidate_sets_of_the_edge_tests_stay_within_the_cap():
    from metamorph_amd import functional as F
    cases = [(n, C, R) + S.overfull_case(n, C, R, seed) for n, C, R, seed in S.OVERFULL_CASES]
    cases += [(n, C, S.TEMP_R) + S.temperature_case(n, C) for n in S.TEMP_FAMILIES for C in S.TEMP_CS]
    cases += [("key_lo row",) + S.KEYLO_CASE[1:3] + S.keylo_case()]
    widest, filtered = {}, {}
    for name, C, R, x, sets in cases:
        rows = x.double().numpy()
        for T, top_k, top_p, u_drawn in sets:
            for kind, u in S.u_kinds(R, u_drawn):
                for r in range(R):
                    n = len(F.sample_row_host(rows[r], S.f32(1.0 / T), top_k, S.f32(top_p), float(u[r]), eps=S.EPS)[0])
                    assert 1 <= n <= S.CAND_CAP, (name, C, T, top_k, top_p, kind, r, n)
                    widest[name] = max(widest.get(name, 0), n)
                    if top_k or top_p < 1.0:
                        filtered[name] = max(filtered.get(name, 0), n)
    print("   widest candidate set (under a filter): " + ", ".join(f"{n} {w} ({filtered[n]})" for n, w in widest.items()))


def test_rows_of_the_first_sampler_test_never_overfill_a_bin():
    """for the record: the generator sequence of test_sample_gpu.test_sample_rows_against_the_host_model, whose fullest chosen bin
    stays on the list branch (which is why the rows above exist)"""
    fullest = (0, None)
    for R, C in [(R, C) for C in (37, 1000) for R in (1, 3, 17)] + [(3, 128258)]:
        settings = [S.SETTINGS[1], S.SETTINGS[3]] if C == 128258 else S.SETTINGS
        g = torch.Generator().manual_seed(100003 * R + C)
        for name in S.FAMILIES:
            x = S.family(name, R, C, g).numpy()
            for T, top_k, top_p in settings:
                S.drawn_u(R, g)                                      # (the test draws its u here)
                for r in range(R):
                    for kind, b, n in S.round0_occupancy(x[r], S.f32(1.0 / T), top_k, S.f32(top_p)):
                        fullest = max(fullest, (n, (name, R, C, T, top_k, top_p, kind, b)))
    print(f"   fullest chosen bin of the existing rows: {fullest[0]} values at {fullest[1]}")
