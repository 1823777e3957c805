"""mm355_sample_rows_f32 where its first tests do not go (the rows and references are tests/sample_refs.py; which branch each row takes
is proved on the CPU by tests/test_sample_refs_host.py):

  * rows whose chosen bin of round 0 holds more than the 8192 keys of the LDS list, so that rounds 1 .. 4 of select_key read the row
    again -- in the count select, in the mass select, and in a mass select after a count select -- next to the row that fills the list
    exactly;
  * the pick walk on rows of five unit weights, whose partial sums are exact, with the picked column on every wave-span, chunk and
    64-column scan boundary and in the chunk that the end of the row cuts short;
  * temperatures at which most weights underflow (T = 0.05) or the row is nearly flat (T = 20).
The specification is functional.sample_row_host, in the bands of check_row."""
import time

import numpy as np
import pytest
import torch

import sample_refs as S

pytestmark = pytest.mark.gpu


def _check_case(tag, x, sets):
    R = x.shape[0]
    rows = x.double().numpy()
    widest, taus = 0, {}
    for T, top_k, top_p, u_drawn in sets:
        for kind, u in S.u_kinds(R, u_drawn):
            out, stats = S.device_draw(x, T, top_k, top_p, u)
            for r in range(R):
                n = S.check_row(rows[r], T, top_k, top_p, float(u[r]), out[r], stats[r, 0], stats[r, 1], (tag, T, top_k, top_p, kind, r))
                widest = max(widest, n)
                taus[(T, top_k, top_p, r)] = stats[r, 0]
    assert widest <= S.CAND_CAP, widest
    return widest, taus


@pytest.mark.parametrize("name,C,R,seed", S.OVERFULL_CASES, ids=[f"{c[0]}-{c[1]}" for c in S.OVERFULL_CASES])
def test_rows_that_overfill_a_bin_of_round_0(name, C, R, seed):
    t0 = time.time()
    x, sets = S.overfull_case(name, C, R, seed)
    widest, taus = _check_case(name, x, sets)
    # top-k alone: the band of check_row is a point, tau is the exact k-th largest value
    T, top_k, top_p = S.SETTINGS[2]
    for r in range(R):
        kth = float(np.sort(x[r].numpy())[C - top_k])
        assert taus[(T, top_k, top_p, r)] == kth, (name, r, taus[(T, top_k, top_p, r)], kth)
        if name == "plateau":
            assert kth == S.PLATEAU
        if name == "allowed_set":
            assert kth == -np.inf
    print(f"   {name} C={C} R={R}: widest candidate set {widest}, {time.time() - t0:.2f} s")


def test_a_mass_select_rereads_only_what_top_k_kept():
    """both selects of one call on the re-read branch, the second with 8004 values in its bin that top_k = 12000 refused"""
    t0 = time.time()
    x, sets = S.keylo_case()
    widest, _ = _check_case("key_lo row", x, sets)
    print(f"   key_lo row: widest candidate set {widest}, {time.time() - t0:.2f} s")


@pytest.mark.parametrize("C", S.POINT_CS)
def test_the_pick_walk_on_rows_of_five_unit_weights(C):
    from metamorph_amd import functional as F
    t0 = time.time()
    sets = S.point_sets(C)
    nu = len(S.POINT_US)
    x = torch.cat([S.points(cols)(nu, C) for cols in sets])          # one row per (column set, u)
    u = torch.tensor(S.POINT_US * len(sets), dtype=torch.float32)
    assert u.double().tolist() == S.POINT_US * len(sets)
    for T, top_k, top_p in S.POINT_FILTERS:
        out, stats = S.device_draw(x, T, top_k, top_p, u)
        for s, cols in enumerate(sets):
            row = x[s * nu].double().numpy()
            for j in range(nu):
                cand, lo, hi, Z = F.sample_row_host(row, S.f32(1.0 / T), top_k, S.f32(top_p), S.POINT_US[j], eps=0.0)
                assert len(cand) == 1 and lo == hi == -np.inf and Z == 5.0
                if j < 5:                                            # u = (j + 0.5) / 5: the prefix 1, 2, .. first exceeds j + 0.5 at cols[j]
                    assert cand == [cols[j]]
                else:                                                # u = fp32(0.2) > 0.2: u Z lies in [1, 2), the interval of cols[1]
                    assert cand == [cols[1]]
                got = (out[s * nu + j], stats[s * nu + j, 0], stats[s * nu + j, 1])
                assert got == (cand[0], lo, 5.0), (C, top_k, cols, S.POINT_US[j], got, cand)
    print(f"   C={C}: {len(sets)} column sets {sets}, {time.time() - t0:.2f} s")


@pytest.mark.parametrize("name", S.TEMP_FAMILIES)
@pytest.mark.parametrize("C", S.TEMP_CS)
def test_temperatures_that_underflow_or_flatten_the_weights(C, name):
    t0 = time.time()
    x, sets = S.temperature_case(name, C)
    widest, _ = _check_case(name, x, sets)
    print(f"   {name} C={C}: widest candidate set {widest}, {time.time() - t0:.2f} s")
