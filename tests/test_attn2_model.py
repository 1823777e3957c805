"""CPU checks of the test infrastructure behind tests/test_attn_generic_gpu.py (tests/attn2_model.py): the model of attn2::fwd_kernel's
arithmetic is as close to fp64 as the bf16 flash yardstick, the hostile inputs provably drive its deferred-rescale branch at generic head
sizes (and the inputs of the older generic-d kernel tests provably do not), the `threshold` inputs sit on the decision's exact fp32
boundary for every head size, the d == 128 inputs are unchanged, and the comparison the GPU test uses rejects plausible kernel bugs."""
import hashlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn2_model as M2  # noqa: E402
import attn4_model as M4  # noqa: E402

KINDS = ("benign", "rising", "one_row", "sink", "cliff", "wide", "threshold")
D_SWEEP = (16, 32, 40, 56, 80, 88, 96, 104, 120)


def _do(B, L, Hq, d, seqlens, seed=5):
    g = torch.Generator().manual_seed(seed)
    do = (torch.randn(B, L, Hq, d, generator=g) * 0.5).to(torch.bfloat16)
    return do * M2.valid_rows(B, L, seqlens)[:, :, None, None]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d,causal,seqlens", [(64, True, [320, 229]), (72, False, None)])
def test_model_against_fp64_and_the_branch_fires(kind, d, causal, seqlens):
    B = 3 if kind == "threshold" else 2
    if kind == "threshold" and seqlens is not None:
        seqlens = seqlens + [320]
    L = 320                                                      # (> 300: the second sink)
    q, k, v = M4.hostile_inputs(kind, B, L, 2, 1, seed=1, d=d)
    scale = d ** -0.5
    o, lse, cnt = M2.attn2_forward_model(q, k, v, seqlens, causal, scale)
    to, tl, *_ = M2.truth64(q, k, v, None, seqlens, causal, scale)
    yo = M4.flash_bf16_forward(q, k, v, seqlens, causal, scale)
    bad, err = M2.check_forward(o, lse, to, tl, yo, o, seqlens)
    assert not bad, (bad, err)
    inval = ~M2.valid_rows(B, L, seqlens)
    assert bool((o[inval] == 0).all()) and bool((lse.transpose(1, 2)[inval] == 0).all()), "padding rows must be zero"
    if kind == "benign":
        assert int(cnt.sum()) == 0
    else:
        assert int(cnt.sum()) > 0, "the deferred-rescale branch never fired: the input is not hostile"
    if kind == "rising":                                         # 8 log2 units per tile: every tile after a wave's first fires
        assert int(cnt.min()) >= 0 and int(cnt.max()) == (L + 63) // 64 - 1
    if kind == "threshold":
        assert int(cnt[0].sum()) == 0 and int(cnt[1].sum()) == 0 and int(cnt[2].sum()) > 0


@pytest.mark.parametrize("d", D_SWEEP + (64, 72))
@pytest.mark.parametrize("causal", [True, False])
def test_threshold_fires_one_step_above_only(d, causal):
    """fp32(s1 * c) one fp32 step below / exactly on / one step above the threshold m + 6: only sample 2 takes the branch, once per wave
    that walks key tile 1."""
    L = 200
    q, k, v = M4.hostile_inputs("threshold", 3, L, 2, 1, seed=3, d=d)
    c = M4.sl2_of(d ** -0.5)
    for b, (s0, s1) in enumerate(M4.threshold_scores(d)):       # the raw scores the kernel's MFMAs form, exactly, in any order
        assert float(q[b, 5, 0].float() @ k[b, 0, 0].float()) == float(s0)
        assert float(q[b, 5, 0].float() @ k[b, 70, 0].float()) == float(s1)
    x = M4.threshold_scores(d)[0][1] * c
    T = [s0 * c + 6.0 for s0, _ in M4.threshold_scores(d)]
    assert bool(x == torch.nextafter(T[0], torch.tensor(0.0))) and bool(x == T[1]) and bool(x == torch.nextafter(T[2], torch.tensor(9.0)))
    _, _, cnt = M2.attn2_forward_model(q, k, v, None, causal, d ** -0.5)
    assert int(cnt[0].sum()) == 0 and int(cnt[1].sum()) == 0
    waves_tile1 = (torch.arange(0, (L + 63) // 64 * 64, 16) >= 64) if causal else torch.ones((L + 63) // 64 * 4, dtype=torch.bool)
    assert torch.equal(cnt[2], waves_tile1.int()[None].expand(2, -1))


# the generic-d rows of tests/test_kernels_gpu.py::ATT_CASES, with that file's input construction (rnd(B * L, ld, seed, scale=0.7))
@pytest.mark.parametrize("case", [(2, 130, 4, 4, 64, True, [130, 5]), (2, 100, 3, 3, 72, False, None), (1, 729, 2, 2, 72, False, None)])
def test_older_generic_cases_never_reach_the_branch(case):
    B, L, Hq, Hkv, d, causal, seqlens = case
    for seed in (0, 3):                                          # test_attn_fwd / test_attn_bwd
        g = torch.Generator().manual_seed(seed)
        qkv = (torch.randn(B * L, (Hq + 2 * Hkv) * d, generator=g) * 0.7).to(torch.bfloat16)
        q = qkv[:, :Hq * d].reshape(B, L, Hq, d)
        k = qkv[:, Hq * d:(Hq + Hkv) * d].reshape(B, L, Hkv, d)
        v = qkv[:, (Hq + Hkv) * d:].reshape(B, L, Hkv, d)
        _, _, cnt = M2.attn2_forward_model(q, k, v, seqlens, causal, d ** -0.5)
        assert int(cnt.sum()) == 0


def test_d128_inputs_unchanged():
    """hostile_inputs(d = 128), the inputs of tests/test_attn_hostile_gpu.py, are bit for bit what they were before the d argument"""
    want = {"benign": "1b34f98d32e3344f", "rising": "0667d9c32752fc5e", "one_row": "ca0f1a07326d2929", "sink": "d8842fd5cee90ce4",
            "cliff": "0ae0861a4aa5d1e5", "wide": "c37f56ccd3b5af73", "threshold": "67a20980fc0748a0"}
    for kind in KINDS:
        h = hashlib.sha256()
        for t in M4.hostile_inputs(kind, 3 if kind == "threshold" else 2, 300, 2, 1, seed=1):
            h.update(t.contiguous().view(torch.int16).numpy().tobytes())
        assert h.hexdigest()[:16] == want[kind], kind


# ------------------------------------------------------------------------------------------------ checker power

POWER_CASES = {  # name: B, L, Hq, Hkv, d, causal, seqlens, dropped key tile, missing query tile
    "tower": (2, 729, 4, 4, 72, False, None, 5, 5),
    "tinyllama": (1, 2048, 8, 1, 64, True, None, 1, 16),
}


@pytest.fixture(scope="module", params=sorted(POWER_CASES))
def power(request):
    B, L, Hq, Hkv, d, causal, seqlens, kt, qt = POWER_CASES[request.param]
    scale = d ** -0.5
    out = {"name": request.param, "geo": POWER_CASES[request.param]}
    for kind in ("benign", "rising"):
        q, k, v = M4.hostile_inputs(kind, B, L, Hq, Hkv, seed=11, d=d)
        do = _do(B, L, Hq, d, seqlens)
        om, lm, _ = M2.attn2_forward_model(q, k, v, seqlens, causal, scale)
        to, tl, tq, tk, tv = M2.truth64(q, k, v, do, seqlens, causal, scale)
        yo, yq, yk, yv = M4.flash_bf16_backward(q, k, v, do, seqlens, causal, scale)
        out[kind] = dict(q=q, k=k, v=v, do=do, om=om, lm=lm, truth=(to, tl, tq, tk, tv), yard=(yo, yq, yk, yv))
    return out


def _fwd_verdict(r, o, lse, seqlens):
    to, tl = r["truth"][:2]
    return M2.check_forward(o, lse, to, tl, r["yard"][0], r["om"], seqlens)


def test_checker_accepts_the_model_and_the_yardstick(power):
    seqlens = power["geo"][6]
    for kind in ("benign", "rising"):
        r = power[kind]
        assert not _fwd_verdict(r, r["om"], r["lm"], seqlens)[0]
        assert not _fwd_verdict(r, r["yard"][0], r["lm"], seqlens)[0]
        bad, err = M2.check_backward(r["yard"][1:], r["truth"][2:], r["yard"][1:])
        assert not bad, err


def test_checker_rejects_a_dropped_key_tile(power):
    B, L, Hq, Hkv, d, causal, seqlens, kt, _ = power["geo"]
    r = power["benign"]
    o_drop = M2.truth64(r["q"], r["k"], r["v"], None, seqlens, causal, d ** -0.5, drop_keys=(64 * kt, 64 * kt + 64))[0].to(torch.bfloat16)
    bad, err = _fwd_verdict(r, o_drop, r["lm"], seqlens)
    print(f"\n   {power['name']}: o without key tile {kt}: {bad} {err}")
    assert bad


def test_checker_rejects_o_not_rescaled(power):
    B, L, Hq, Hkv, d, causal, seqlens, _, _ = power["geo"]
    r = power["rising"]
    o_bad, lse_bad, _ = M2.attn2_forward_model(r["q"], r["k"], r["v"], seqlens, causal, d ** -0.5, rescale_o=False)
    bad, err = _fwd_verdict(r, o_bad, lse_bad, seqlens)
    print(f"\n   {power['name']}: O not rescaled on the branch: {bad} {err}")
    assert bad


@pytest.mark.parametrize("kind", ["benign", "rising"])
def test_checker_rejects_scaled_gradients(power, kind):
    r = power[kind]
    yq, yk, yv = r["yard"][1:]
    for name, g in (("dk x 0.8", (yq, yk * 0.8, yv)), ("dv x 0.8", (yq, yk, yv * 0.8))):
        bad, err = M2.check_backward(g, r["truth"][2:], r["yard"][1:])
        print(f"\n   {power['name']} {kind}: {name}: {bad}")
        assert bad, (name, err)


def _contribution(r, geo, rows=None, head=None):
    """the part of dk / dv that comes from the given query rows / query head (the backward is linear in do)"""
    B, L, Hq, Hkv, d, causal, seqlens = geo[:7]
    do = torch.zeros_like(r["do"])
    if rows is not None:
        do[:, rows[0]:rows[1]] = r["do"][:, rows[0]:rows[1]]
    if head is not None:
        do[:, :, head] = r["do"][:, :, head]
    _, _, _, ck, cv = M2.truth64(r["q"], r["k"], r["v"], do, seqlens, causal, d ** -0.5)
    return ck, cv


def test_checker_rejects_a_missing_query_tile(power):
    geo = power["geo"]
    qt = geo[8]
    r = power["benign"]
    yq, yk, yv = r["yard"][1:]
    ck, cv = _contribution(r, geo, rows=(64 * qt, 64 * qt + 64))
    for name, g in (("dk", (yq, yk - ck, yv)), ("dv", (yq, yk, yv - cv))):
        bad, err = M2.check_backward(g, r["truth"][2:], r["yard"][1:])
        print(f"\n   {power['name']}: {name} without query tile {qt}: {bad}")
        assert bad, (name, err)


@pytest.mark.parametrize("power", ["tinyllama"], indirect=True)     # (the tower has no GQA group)
def test_checker_rejects_a_missing_gqa_head(power):
    geo = power["geo"]
    r = power["benign"]
    yq, yk, yv = r["yard"][1:]
    ck, cv = _contribution(r, geo, head=geo[2] // geo[3] - 1)    # the last query head of KV group 0
    for name, g in (("dk", (yq, yk - ck, yv)), ("dv", (yq, yk, yv - cv))):
        bad, err = M2.check_backward(g, r["truth"][2:], r["yard"][1:])
        print(f"\n   {power['name']}: {name} without one query head of its group: {bad}")
        assert bad, (name, err)
