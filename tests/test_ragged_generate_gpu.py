"""config.mm355_ragged_pass = True through the public interface, against the same calls with the field absent: greedy_decode of the five
left-padded prompts of tests/test_greedy_batch_gpu.py (that file's seeds, lengths, gap rule and caps, its helpers imported), a follow-up
turn of B = 3 through forward(past_key_values=HipKVCache), and HF generate()."""
import pytest
import torch

import test_greedy_batch_gpu as GB
from test_extend_pass_gpu import check_logits, embeds, model_of

pytestmark = pytest.mark.gpu
DEV = "cuda"


class _flag:
    """config.mm355_ragged_pass = True for a block, the passes the model takes counted"""

    def __init__(self, model, monkeypatch, on=True):
        from metamorph_amd import functional as F
        self.model, self.on, self.calls = model, on, {"decoder_extend_ragged": 0, "decoder_extend": 0, "decoder_prefill": 0}
        for name in self.calls:
            orig = getattr(F, name)
            monkeypatch.setattr(F, name, lambda *a, _o=orig, _n=name, **k: (self.calls.__setitem__(_n, self.calls[_n] + 1), _o(*a, **k))[1])

    def __enter__(self):
        if self.on:
            self.model.config.mm355_ragged_pass = True
        return self.calls

    def __exit__(self, *exc):
        if self.on:
            del self.model.config.mm355_ragged_pass


def test_greedy_decode_of_left_padded_prompts_flag_on_against_flag_off(monkeypatch):
    """Ids and pred_z rows of every sequence, flag on against flag off, up to the first iteration at which the alone run's top-two gap is
    below the GAP_THRESHOLD of its mode (test_left_padded_batch_gives_every_sequence_what_it_gets_alone's rule, its 2e-2 and its caps: at
    least 3 of 5 sequences compared to their end, at least 2 complete images).  With the flag on the five prompts are ONE pass."""
    alone, (ids0, zs0, _) = GB._diverge_case()                    # the alone runs (the gaps) and the batch with the field absent
    _, model = GB._diverge_model()
    with _flag(model, monkeypatch) as calls:
        ids1, zs1, loop = GB._batch_run(GB.DIVERGE_SEEDS)
    assert calls == {"decoder_extend_ragged": 1, "decoder_extend": 0, "decoder_prefill": 0}, calls
    assert not hasattr(model.config, "mm355_ragged_pass")
    assert loop.cache.batch == 5 and loop.cache.lengths == [L + loop.steps for L in GB.LENS]
    whole, images = 0, 0
    for b, (a_ids, a_z, its) in enumerate(alone):
        n_it, n_tok, n_z, to_end = GB._cut(its, GB.GAP_THRESHOLD)
        print(f"   sequence {b}: {len(its)} iterations alone, compared {n_it} ({n_tok} ids, {n_z} pred_z rows)")
        assert ids1[b][:n_tok].tolist() == ids0[b][:n_tok].tolist(), (b, ids1[b].tolist(), ids0[b].tolist())
        assert zs1[b].shape[0] >= n_z and (n_z == 0 or GB.rel(zs1[b][:n_z], zs0[b][:n_z]) <= 2e-2), b
        for r in range(n_z):
            assert GB.rel(zs1[b][r], zs0[b][r]) <= 2e-2, (b, r)
        if to_end:
            assert ids1[b].tolist() == ids0[b].tolist() and zs1[b].shape[0] == n_z
            whole += 1
            images += GB._complete_image(a_ids, a_z)
    print(f"   compared to their end: {whole} of 5 sequences, {images} complete images")
    assert whole >= 3 and images >= 2, (whole, images)


def test_follow_up_turn_of_three_sequences_is_one_pass(monkeypatch):
    """forward(past_key_values=cache) twice on B = 3 left-padded prompts: the prompts, then 6 new rows each.  Flag on: one packed pass per
    call (no decoder_prefill, no decoder_extend); the logits of both calls against the flag-off run by test_extend_pass_gpu's criterion,
    the caches' lengths equal."""
    from metamorph_amd.model.language_model.metamorph_llama import HipKVCache
    cfg, m, _ = model_of("tiny", "bf16")
    h, lens, n = cfg.hidden_size, (21, 9, 15), 6
    emb = embeds(3, max(lens) + n, h, seed=29)
    L0 = max(lens)
    prompt, mask = torch.zeros(3, L0, h, dtype=torch.bfloat16, device=DEV), torch.zeros(3, L0, dtype=torch.long, device=DEV)
    for b, L in enumerate(lens):
        prompt[b, L0 - L:], mask[b, L0 - L:] = emb[b, :L], 1
    turn = torch.stack([emb[b, L:L + n] for b, L in enumerate(lens)], 0)
    mask2 = torch.cat([mask, torch.ones(3, n, dtype=torch.long, device=DEV)], 1)
    runs = {}
    for on in (False, True):
        with torch.no_grad(), _flag(m, monkeypatch, on) as calls:
            c = HipKVCache(capacity=L0 + n + 8)
            a = m(inputs_embeds=prompt, attention_mask=mask, past_key_values=c, use_cache=True).logits
            first = dict(calls)
            b = m(inputs_embeds=turn, attention_mask=mask2, past_key_values=c, use_cache=True).logits
            runs[on] = (a.float(), b.float(), list(c.kv.lengths), first, dict(calls))
    assert runs[False][3]["decoder_extend_ragged"] == 0 and runs[False][4] == {"decoder_extend_ragged": 0, "decoder_extend": 3, "decoder_prefill": 3}
    assert runs[True][3] == {"decoder_extend_ragged": 1, "decoder_extend": 0, "decoder_prefill": 0}
    assert runs[True][4] == {"decoder_extend_ragged": 2, "decoder_extend": 0, "decoder_prefill": 0}
    assert runs[True][2] == runs[False][2] == [L + n for L in lens]
    assert tuple(runs[True][1].shape[:2]) == (3, n)
    for b, L in enumerate(lens):
        check_logits(runs[True][0][b, L0 - L:], runs[False][0][b, L0 - L:], f"prompt {b}: flag on against flag off")
        check_logits(runs[True][1][b], runs[False][1][b], f"turn of sequence {b}: flag on against flag off")


def test_hf_generate_returns_sequences_of_the_same_lengths(monkeypatch):
    cfg, m, _ = model_of("tiny", "bf16")
    g = torch.Generator().manual_seed(31)
    lens, L0 = (11, 5, 8), 11
    ids = torch.randint(0, 127000, (3, L0), generator=g)
    mask = torch.zeros(3, L0, dtype=torch.long)
    for b, L in enumerate(lens):
        mask[b, L0 - L:] = 1
    kw = dict(inputs=ids.to(DEV), attention_mask=mask.to(DEV), use_customize_greedy=False, do_sample=False, max_new_tokens=6, eos_token_id=128009,
              pad_token_id=128001)
    off = m.generate(**kw)
    with _flag(m, monkeypatch) as calls:
        on = m.generate(**kw)
    assert calls["decoder_extend_ragged"] == 1 and calls["decoder_prefill"] == 0
    assert tuple(on.shape) == tuple(off.shape) and on[:, :L0].tolist() == off[:, :L0].tolist()
    for b in range(3):
        assert int((on[b] != 128001).sum()) == int((off[b] != 128001).sum()), (b, on[b].tolist(), off[b].tolist())
    m.config.mm355_ragged_pass = "yes"
    try:
        with pytest.raises(ValueError, match="mm355_ragged_pass"):
            m.generate(**kw)
    finally:
        del m.config.mm355_ragged_pass
