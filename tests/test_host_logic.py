"""CPU tier: the product's host-side logic against the golden vectors recorded from the reference, the C-ABI
library's exports, and the rule that the product never touches oracle/ or a CPU fallback."""
import ast
import ctypes
import glob
import json
import os
import re

import numpy as np
from types import SimpleNamespace
import pytest
import torch

from conftest import GOLDEN, REPO


# ------------------------------------------------------------------ A1

def test_tokenizer_image_token_matches_reference():
    from oracle.fake_tokenizer import FakeTokenizer
    from metamorph_amd.mm_utils import tokenizer_image_token
    cases = json.load(open(os.path.join(GOLDEN, "a1_tokenizer.json")))
    for c in cases:
        tok = FakeTokenizer(add_bos=c["add_bos"])
        assert tokenizer_image_token(c["prompt"], tok, c["image_token_index"]) == c["ids"], c["prompt"]
    t = tokenizer_image_token("a <image> b", FakeTokenizer(), return_tensors="pt")
    assert t.dtype == torch.long
    with pytest.raises(ValueError):
        tokenizer_image_token("a", FakeTokenizer(), return_tensors="np")


def test_llama3_template_gives_double_bos():
    """literal <|begin_of_text|> in the prompt + the tokenizer's automatic BOS -> two BOS ids."""
    from oracle.fake_tokenizer import FakeTokenizer
    from metamorph_amd.mm_utils import tokenizer_image_token
    ids = tokenizer_image_token("<|begin_of_text|> hi <image_start><image><image_end>", FakeTokenizer(add_bos=True))
    assert ids[:2] == [128000, 128000] and ids.count(-200) == 1 and ids[ids.index(-200) - 1] == 128256


# ------------------------------------------------------------------ A5

@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "a5_*.npz"))))
def test_splice_plan_matches_reference(path):
    from metamorph_amd.splice_plan import build_splice_plan
    g = np.load(path)
    Timg = int(g["rows_per_image"])
    # a5_wrap_*: the wrapper's None handling (metamorph_arch.py:245-256, 400-412) -- labels / attention_mask not given, position_ids given,
    # no tokenizer_model_max_length in the config
    labels = g["labels"] if ("labels_given" not in g.files or int(g["labels_given"])) else None
    mask = g["attention_mask"] if ("mask_given" not in g.files or int(g["mask_given"])) else None
    max_len = int(g["max_length"]) if int(g["max_length"]) >= 0 else None
    args = (g["input_ids"], labels, mask, int(g["num_images"]), Timg, max_len, "left" if int(g["left"]) else "right")
    if "error" in g.files:                                    # known answer: an image + no max length is `int > None` in the reference (:324)
        with pytest.raises(TypeError):
            build_splice_plan(*args)
        return
    plan = build_splice_plan(*args)
    B, L = g["out_labels"].shape if "out_labels" in g.files else g["out_shape"].tolist()
    assert (plan.B, plan.L) == (B, L)
    assert np.array_equal(plan.src.reshape(B, L), g["out_src"])
    if "out_labels" in g.files:
        assert np.array_equal(plan.labels, g["out_labels"])
    else:
        assert plan.labels is None and int(g["out_labels_is_none"]) == 1
    if "out_attention_mask" in g.files:
        assert np.array_equal(plan.attention_mask, g["out_attention_mask"])
    else:                                                     # no mask in: every row is a token row (pad ids included), None goes back out
        assert int(g["out_mask_is_none"]) == 1 and np.array_equal(plan.attention_mask, g["out_src"] != -1)
    if "out_position_ids" in g.files:                         # given position_ids are replaced by arange over each sample's rows, 0 on padding
        assert np.array_equal(plan.position_ids, g["out_position_ids"])
    assert np.array_equal(plan.image_positions, g["out_image_positions"])
    assert plan.target_keep.tolist() == g["out_target_keep"].tolist()
    if "out_labels" not in g.files:
        return
    # derived index arrays are consistent with the primary ones
    flat = plan.src
    for n, r in enumerate(plan.feat_row.tolist()):
        if r >= 0:
            assert flat[r] == -2 - n
    assert (plan.feat_row >= 0).sum() == (flat <= -2).sum()
    nxt = np.zeros((B, L), dtype=bool)
    nxt[:, :-1] = g["out_image_positions"][:, 1:] == 1
    assert plan.pred_rows.tolist() == np.flatnonzero(nxt.reshape(-1)).tolist()
    st = np.full((B, L), -100)
    st[:, :-1] = g["out_labels"][:, 1:]
    assert np.array_equal(plan.shift_targets, st.reshape(-1))
    assert plan.n_valid == int((st != -100).sum())
    assert plan.seqlens.tolist() == (g["out_attention_mask"] if "out_attention_mask" in g.files else g["out_src"] != -1).sum(1).tolist()
    # embedding-gradient segments cover every token row exactly once, grouped by id
    seen = []
    for s in range(plan.emb_tok.shape[0]):
        rows = plan.emb_pos[plan.emb_seg[s]: plan.emb_seg[s + 1]]
        assert (flat[rows] == plan.emb_tok[s]).all()
        seen.extend(rows.tolist())
    assert sorted(seen) == np.flatnonzero(flat >= 0).tolist()


def test_splice_plan_matches_oracle_on_random_batches():
    from metamorph_amd.splice_plan import build_splice_plan
    from oracle.ref_plan import splice_bookkeeping
    rng = np.random.default_rng(0)
    for trial in range(200):
        B = int(rng.integers(1, 5))
        Timg = int(rng.choice([1, 4, 16]))
        max_len = int(rng.choice([12, 24, 40, 4096]))
        rows, labs = [], []
        for b in range(B):
            n = int(rng.integers(2, 30))
            ids = rng.integers(3, 1000, size=n).tolist()
            lab = [int(x) if rng.random() < 0.5 else -100 for x in ids]
            for _ in range(int(rng.integers(0, 4))):
                p = int(rng.integers(1, len(ids)))
                if ids[p - 1] == -200 or (p < len(ids) and ids[p] == -200):
                    continue
                ids.insert(p, -200)
                lab.insert(p, -200)
                if rng.random() < 0.5:
                    lab[p - 1] = 128256
            rows.append(ids)
            labs.append(lab)
        T_ = max(len(r) for r in rows)
        pad = lambda r, v: r + [v] * (T_ - len(r))
        ids_a = np.array([pad(r, 0) for r in rows])
        lab_a = np.array([pad(r, -100) for r in labs])
        msk_a = np.array([[True] * len(r) + [False] * (T_ - len(r)) for r in rows])
        n_img = sum(max(1, r.count(-200)) for r in rows)
        side = "left" if trial % 5 == 0 else "right"
        ref = splice_bookkeeping(ids_a.tolist(), lab_a.tolist(), msk_a.tolist(), n_img, Timg, max_len, side)
        plan = build_splice_plan(ids_a, lab_a, msk_a, n_img, Timg, max_len, side)
        src = [[-1 if s is None else (-2 - (s[1] * Timg + s[2]) if isinstance(s, tuple) else s) for s in row] for row in ref["src"]]
        assert np.array_equal(plan.src.reshape(plan.B, plan.L), np.array(src))
        assert np.array_equal(plan.labels, np.array(ref["labels"]))
        assert np.array_equal(plan.image_positions, np.array(ref["image_positions"]))
        assert np.array_equal(plan.attention_mask, np.array(ref["attention_mask"]))
        assert np.array_equal(plan.position_ids, np.array(ref["position_ids"]))
        assert plan.target_keep.tolist() == ref["target_keep"]


def test_splice_plan_error_behaviour():
    from metamorph_amd.splice_plan import build_splice_plan
    with pytest.raises(IndexError):                         # sentinel with no token before it (reference :317)
        build_splice_plan(np.array([[-200, 5]]), np.array([[-100, 5]]), None, 1, 4, 64)
    with pytest.raises(IndexError):                         # text-only sample but no dummy image supplied (reference :420)
        build_splice_plan(np.array([[1, 2], [1, -200]]), np.array([[1, 2], [1, -200]]), None, 1, 4, 64)


# ------------------------------------------------------------------ C ABI

def test_library_exports_every_declared_symbol():
    from metamorph_amd import lib
    names = lib.exported_symbols()
    assert len(names) >= 30
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(lib.LIB_PATH)
    for n in names:
        assert hasattr(so, n), n
    L = lib.load()
    assert L.mm355_version() == 100
    assert b"invalid" in L.mm355_strerror(-1)
    # argument validation works without a GPU (no kernel is launched on the error path)
    assert L.mm355_gemm_bf16(0, 8, 0, 8, 0, 8, 16, 16, 16, 0, 0, 0, 0, 0, 0, 0) == -1
    assert L.mm355_rmsnorm_fwd(0, 0, 0, 4, 8, 1e-5, 0) == -1
    assert L.mm355_transpose_bf16(16, 8, 4, 8, 32, 2, 0) == -1         # ld_out < rows: output rows would overlap


def test_header_cites_reference_for_every_family():
    text = open(os.path.join(REPO, "include", "mm355.h")).read()
    for cite in ("metamorph_llama.py", "metamorph_arch.py", "siglip_encoder.py", "multimodal_projector/builder.py", "zero2.json"):
        assert cite in text, cite


# ------------------------------------------------------------------ isolation rules

def _imports(path):
    tree = ast.parse(open(path).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for a in node.names:
                yield a.name
        elif isinstance(node, ast.ImportFrom) and node.module:
            yield ("." * node.level) + node.module


def test_product_never_imports_oracle_or_reference():
    bad = []
    for path in glob.glob(os.path.join(REPO, "metamorph_amd", "**", "*.py"), recursive=True):
        src = open(path).read()
        for mod in _imports(path):
            if mod.split(".")[0] in ("oracle", "metamorph") or "oracle" in mod:
                bad.append((path, mod))
        if "/root/reference" in src:
            bad.append((path, "/root/reference"))
    assert not bad, bad


def test_no_torch_math_fallback_in_ops():
    """ops.py may allocate / zero / view tensors but must not compute with torch."""
    src = open(os.path.join(REPO, "metamorph_amd", "ops.py")).read()
    for banned in ("torch.matmul", "torch.nn.functional", "F.linear", ".softmax(", "torch.einsum", "@ ", ".mm(", "scaled_dot_product"):
        assert banned not in src, banned


def test_cpu_tensor_is_refused_not_emulated():
    from metamorph_amd import ops
    from metamorph_amd.lib import Mm355Unavailable
    a = torch.zeros(16, 16, dtype=torch.bfloat16)
    with pytest.raises(Mm355Unavailable):
        ops.gemm(a, a)
    with pytest.raises(Mm355Unavailable):
        ops.rmsnorm_fwd(a, a[0], 1e-5)


# ------------------------------------------------------------------ model surface

def test_state_dict_keys_and_config():
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
               vocab_size=300, rms_norm_eps=1e-5, rope_theta=500000.0)
    m = build_model(llm, dict(num_hidden_layers=1, intermediate_size=144, image_size=28), num_image_tokens=4)
    keys = set(m.state_dict().keys())
    expect = {"model.embed_tokens.weight", "model.norm.weight", "lm_head.weight", "model.mm_projector.0.weight",
              "model.mm_projector.0.bias", "model.mm_projector.2.weight", "model.mm_projector.2.bias",
              "model.vision_proj.weight", "model.vision_proj.bias", "vision_head.0.weight", "vision_head.0.bias",
              "vision_head.2.weight", "vision_head.2.bias",
              "model.vision_tower.vision_tower.embeddings.patch_embedding.weight",
              "model.vision_tower.vision_tower.embeddings.position_embedding.weight",
              "model.vision_tower.vision_tower.encoder.layers.0.self_attn.out_proj.bias",
              "model.vision_tower.vision_tower.encoder.layers.0.mlp.fc1.weight",
              "model.vision_tower.vision_tower.post_layernorm.weight"}
    for i in range(2):
        for n in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
                  "mlp.down_proj", "input_layernorm", "post_attention_layernorm"):
            expect.add(f"model.layers.{i}.{n}.weight")
    assert expect <= keys, expect - keys
    assert m.config.model_type == "metamorph_llama"
    assert m.vision_head[2].weight.shape == (1152, 64)
    assert np.isnan(m.loss_language) and np.isnan(m.loss_image_ar)
    from metamorph_amd.model import build_vision_projector
    with pytest.raises(ValueError):
        build_vision_projector(type("C", (), dict(mm_projector_type="nope", mm_hidden_size=8, hidden_size=8))())


def test_fused_weight_views_survive_dtype_cast():
    from metamorph_amd import functional as F
    ps = [torch.nn.Parameter(torch.randn(4, 8)), torch.nn.Parameter(torch.randn(2, 8)), torch.nn.Parameter(torch.randn(2, 8))]
    before = [p.detach().clone() for p in ps]
    w = F.fused_weight(ps)
    assert w.shape == (8, 8) and all(torch.equal(p.data, b) for p, b in zip(ps, before))
    assert F._adjacent([p.data for p in ps]) and F.fused_weight(ps).data_ptr() == w.data_ptr()
    w[0, 0] = 42.0
    assert float(ps[0][0, 0]) == 42.0
    fb, acc, bufs = F.fused_grad_target(ps)
    assert acc is False and fb.shape == (8, 8)
    fb.fill_(1.0)
    F.commit_fused_grad(ps, fb, acc, bufs)
    assert all(p.grad is not None and float(p.grad.sum()) == p.numel() for p in ps)
    fb2, acc2, _ = F.fused_grad_target(ps)
    assert acc2 is True and fb2.data_ptr() == fb.data_ptr()


def test_save_and_from_pretrained_round_trip(tmp_path):
    """HF plumbing the reference relies on (train.py:1411-1423 / save_pretrained): same keys, same values back."""
    from metamorph_amd.factory import build_model
    from metamorph_amd.model import MetaMorphLlamaForCausalLM
    llm = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
               vocab_size=300, rms_norm_eps=1e-5, rope_theta=500000.0)
    m = build_model(llm, dict(num_hidden_layers=1, intermediate_size=144, image_size=28), num_image_tokens=4)
    m.save_pretrained(tmp_path)
    m2 = MetaMorphLlamaForCausalLM.from_pretrained(tmp_path, torch_dtype=torch.bfloat16, vision_head="mlp", normalize_vision=True)
    sd1, sd2 = m.state_dict(), m2.state_dict()
    for k, v in sd1.items():
        if "vision_tower" not in k:
            assert torch.equal(v, sd2[k]), k
    assert m2.config.num_image_tokens == 4 and m2.config.model_type == "metamorph_llama"


@pytest.mark.parametrize("world", [1, 2, 8])
def test_deepspeed_zero2_shard_layout_round_trip(tmp_path, world):
    """`checkpoint.read_deepspeed_zero2_checkpoint`: DeepSpeed's per-rank ZeRO-2 resume files (reference train.py:210-213 / 1592-1599; layout
    restated from DeepSpeed 0.15.1's zero_to_fp32.py -- PARITY UNPINNED: DeepSpeed is not in this image, no real file could be recorded) -> the
    world-size-independent optimizer state.  Round trip through a writer of the same layout at world 1 / 2 / 8: two parameter groups, sizes that
    do not divide 2 x world (alignment padding), bf16_ and plain file names; a missing rank and a ZeRO-3 stage are refused."""
    from metamorph_amd.checkpoint import read_deepspeed_zero2_checkpoint, write_deepspeed_zero2_layout
    g = torch.Generator().manual_seed(world)
    shapes = {"model.embed_tokens.weight": (37, 8), "model.layers.0.mlp.gate_proj.weight": (5, 8), "model.norm.weight": (8,), "lm_head.bias": (3,)}
    cons = {"step": 7, "param_groups": [{"lr": 2e-5, "weight_decay": 0.0, "betas": (0.9, 0.999), "eps": 1e-8}, {"lr": 2e-6, "weight_decay": 0.1, "betas": (0.9, 0.999), "eps": 1e-8}],
            "state": {n: {k: torch.randn(*shp, generator=g) for k in ("master", "exp_avg", "exp_avg_sq")} for n, shp in shapes.items()}}
    groups = [["model.embed_tokens.weight", "model.layers.0.mlp.gate_proj.weight"], ["model.norm.weight", "lm_head.bias"]]
    d = str(tmp_path / "checkpoint-7")
    step_dir = write_deepspeed_zero2_layout(cons, groups, d, world, tag="global_step7", bf16=world != 2)
    assert sorted(os.listdir(step_dir)) == sorted(["mp_rank_00_model_states.pt"] + [f"{'bf16_' if world != 2 else ''}zero_pp_rank_{r}_mp_rank_00_optim_states.pt" for r in range(world)])
    back = read_deepspeed_zero2_checkpoint(d)
    assert back["step"] == 7 and set(back["state"]) == set(shapes)
    for n in shapes:
        for k in ("master", "exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][n][k], cons["state"][n][k]), (n, k)
    assert [pg["lr"] for pg in back["param_groups"]] == [2e-5, 2e-6]
    if world > 1:
        os.remove(os.path.join(step_dir, f"{'bf16_' if world != 2 else ''}zero_pp_rank_{world - 1}_mp_rank_00_optim_states.pt"))
        with pytest.raises((FileNotFoundError, ValueError)):
            read_deepspeed_zero2_checkpoint(d)


def test_compact_row_maps_are_inverse_and_tile_aligned():
    """Padding-free rows: c2p / p2c of metamorph_llama.compact_row_maps are inverse on the valid rows, list samples back to back in order, mark
    padding / tail rows -1, and the compact row count is a whole number of 256-row GEMM tiles (>= one tile, also for an all-empty batch)."""
    from metamorph_amd.splice_plan import compact_row_maps
    rng = np.random.default_rng(5)
    for _ in range(50):
        B, L = int(rng.integers(1, 9)), int(rng.integers(1, 900))
        n = rng.integers(0, L + 1, size=B)
        c2p, p2c = compact_row_maps(n, B, L)
        total = int(n.sum())
        assert c2p.shape[0] % 256 == 0 and c2p.shape[0] >= max(total, 256) and c2p.shape[0] - total < 256 + (total == 0) * 256
        assert (c2p[total:] == -1).all() and (c2p[:total] >= 0).all() and (np.diff(c2p[:total]) > 0).all()
        assert p2c.shape == (B * L,) and (p2c[c2p[:total]] == np.arange(total)).all()
        valid = (np.arange(L)[None] < n[:, None]).reshape(-1)
        assert ((p2c >= 0) == valid).all()
        # full = True (what the plan upload carries): one array whose every prefix of >= `rows` entries is a valid map, up to whole tiles of B x L
        cf, pf = compact_row_maps(n, B, L, full=True)
        assert cf.shape[0] == max(c2p.shape[0], (B * L + 255) // 256 * 256) and (cf[:c2p.shape[0]] == c2p).all() and (cf[c2p.shape[0]:] == -1).all()
        assert (pf == p2c).all()


def test_llama31_checkpoint_config_round_trips_and_unsupported_fields_are_refused_by_name(tmp_path):
    """A LLaMA-3.1-shaped config.json (rope_scaling rope_type "llama3" -- the reference README's base model, README.md:178,187 -- plus tied
    embeddings and an explicit head_dim) constructs, saves and loads back: same RoPE frequencies, lm_head still tied, q_proj sized by head_dim.
    dynamic / yarn / longrope RoPE, attention_bias and mlp_bias are refused at construction, by name."""
    from metamorph_amd.factory import build_model
    from metamorph_amd.model import MetaMorphConfig, MetaMorphLlamaForCausalLM
    from metamorph_amd.rope import rope_params
    r31 = dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=8192)
    llm = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=300,
               rms_norm_eps=1e-5, rope_theta=500000.0, max_position_embeddings=131072, rope_scaling=r31, tie_word_embeddings=True, head_dim=16)
    geo = dict(num_hidden_layers=1, intermediate_size=144, image_size=28)
    m = build_model(llm, geo, num_image_tokens=4)
    assert m.model.rope.rope_type == "llama3" and m.model.rope.head_dim == 16
    assert m.lm_head.weight is m.model.embed_tokens.weight
    assert m.model.layers[0].self_attn.q_proj.weight.shape == (32, 64) and m.model.layers[0].self_attn.o_proj.weight.shape == (64, 32)
    assert len([n for n, _ in m.named_parameters() if n == "lm_head.weight"]) == 0       # one Parameter: optimizers / ZeRO buffers see it once
    m.save_pretrained(tmp_path)
    m2 = MetaMorphLlamaForCausalLM.from_pretrained(tmp_path, torch_dtype=torch.bfloat16, vision_head="mlp", normalize_vision=True)
    assert m2.lm_head.weight is m2.model.embed_tokens.weight and torch.equal(m2.lm_head.weight, m.lm_head.weight)
    assert np.array_equal(m2.model.rope.inv_freq, m.model.rope.inv_freq) and m2.model.rope.rope_type == "llama3"
    assert not np.array_equal(m.model.rope.inv_freq, rope_params(MetaMorphConfig(**{k: v for k, v in llm.items() if k != "rope_scaling"})).inv_freq)
    m.resize_token_embeddings(302)
    assert m.lm_head.weight is m.model.embed_tokens.weight and m.lm_head.weight.shape[0] == 302
    base = {k: v for k, v in llm.items() if k not in ("rope_scaling", "tie_word_embeddings", "head_dim")}
    for kind in ("dynamic", "yarn", "longrope"):
        with pytest.raises(NotImplementedError, match=kind):
            rope_params(SimpleNamespace(hidden_size=64, num_attention_heads=2, rope_theta=1e4, rope_scaling={"rope_type": kind, "factor": 2.0}))
    with pytest.raises(NotImplementedError, match="dynamic"):
        build_model(dict(base, rope_scaling={"rope_type": "dynamic", "factor": 2.0}), geo, num_image_tokens=4)
    for field in ("attention_bias", "mlp_bias"):
        with pytest.raises(NotImplementedError, match="bias"):
            MetaMorphLlamaForCausalLM(MetaMorphConfig(**base, **{field: True}))


# ------------------------------------------------------------------ row N2: batch producer vs the reference's own outputs
def _n2():
    with open(os.path.join(GOLDEN, "n2_batch_producer.json")) as f:
        return json.load(f)


def test_preprocess_llama3_matches_reference():
    """preprocess_multimodal + preprocess_llama3 (llama3 template, label masking incl. the mismatch rule) are integer-exact
    against tests/golden/n2_batch_producer.json, recorded from the reference with the fake tokenizer."""
    import copy
    from types import SimpleNamespace
    from metamorph_amd.data import preprocess, preprocess_multimodal
    from oracle.fake_tokenizer import FakeTokenizer
    cases = _n2()["preprocess"]
    assert len(cases) >= 40
    for c in cases:
        tok = FakeTokenizer(add_bos=c["add_bos"], model_max_length=c["model_max_length"])
        src = preprocess_multimodal(copy.deepcopy(c["sources"]), SimpleNamespace(is_multimodal=True, mm_use_im_start_end=c["mm_use_im_start_end"]))
        out = preprocess(src, tok, has_image=c["has_image"])
        tag = (c["name"], c["add_bos"], c["mm_use_im_start_end"], c["model_max_length"])
        assert out["input_ids"].tolist() == c["input_ids"], tag
        assert out["labels"].tolist() == c["labels"], tag
        assert out["input_ids"].dtype == torch.long and out["labels"].dtype == torch.long


def test_collator_matches_reference():
    from metamorph_amd.data import DataCollatorForSupervisedDataset
    from oracle.fake_tokenizer import FakeTokenizer
    for c in _n2()["collate"]:
        tok = FakeTokenizer(model_max_length=c["model_max_length"])
        inst = [dict(input_ids=torch.tensor(d["input_ids"]), labels=torch.tensor(d["labels"]), image=[torch.tensor(im) for im in d["image"]])
                for d in c["instances"]]
        out = DataCollatorForSupervisedDataset(tokenizer=tok)(inst)
        assert out["input_ids"].tolist() == c["out"]["input_ids"] and out["labels"].tolist() == c["out"]["labels"]
        assert out["attention_mask"].tolist() == c["out"]["attention_mask"] and out["attention_mask"].dtype == torch.bool
        assert out["images"].tolist() == c["out"]["images"]


# ------------------------------------------------------------------ row N3: checkpoint layouts of the reference's orchestration
def test_adapter_checkpoint_layout(tmp_path):
    """Stage-1 adapter files land where the reference's trainer puts them (train.py:186-209, metamorph_trainer.py:273-292)
    and carry the parameters selected by name."""
    from metamorph_amd.checkpoint import safe_save_model, save_mm_adapter, save_trainer_adapter_checkpoint
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1,
               vocab_size=300, rms_norm_eps=1e-5, rope_theta=500000.0)
    m = build_model(llm, dict(num_hidden_layers=1, intermediate_size=144, image_size=28), num_image_tokens=4)
    sd = dict(m.named_parameters())
    p1 = save_mm_adapter(m, str(tmp_path / "run" / "checkpoint-30"))
    assert p1 == str(tmp_path / "run" / "mm_projector" / "checkpoint-30.bin") and os.path.exists(p1)
    assert os.path.exists(tmp_path / "run" / "checkpoint-30" / "config.json")
    w = torch.load(p1)
    assert set(w) == {k for k in sd if "mm_projector" in k} and len(w) == 4
    assert all(torch.equal(w[k], sd[k].detach()) for k in w)
    p2 = save_mm_adapter(m, str(tmp_path / "final"), use_im_start_end=True)
    assert p2 == str(tmp_path / "final" / "mm_projector.bin")
    assert "model.embed_tokens.weight" in torch.load(p2)
    p3 = save_trainer_adapter_checkpoint(m, str(tmp_path / "run"), 77)
    assert p3 == str(tmp_path / "run" / "checkpoint-77" / "mm_projector.bin") and os.path.exists(p3)
    assert safe_save_model(m, str(tmp_path / "a"), tune_mm_mlp_adapter=True) == str(tmp_path / "a" / "mm_projector.bin")
    safe_save_model(m, str(tmp_path / "full"))
    assert os.path.exists(tmp_path / "full" / "config.json") and any(f.startswith("model") for f in os.listdir(tmp_path / "full"))
    # the file is what initialize_vision_modules(pretrain_mm_mlp_adapter=...) consumes
    m2 = build_model(llm, dict(num_hidden_layers=1, intermediate_size=144, image_size=28), num_image_tokens=4)
    m2.get_model().mm_projector.load_state_dict({k.split("mm_projector.")[1]: v for k, v in torch.load(p1).items()})
    assert all(torch.equal(a, b) for a, b in zip(m.get_model().mm_projector.state_dict().values(), m2.get_model().mm_projector.state_dict().values()))


def _listing(root):
    files = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            rel = os.path.relpath(os.path.join(d, f), root)
            entry = {"bytes_nonzero": os.path.getsize(os.path.join(d, f)) > 0}
            if f.endswith(".bin"):
                blob = torch.load(os.path.join(d, f), map_location="cpu", weights_only=True)
                entry["keys"] = list(blob.keys())
                entry["dtypes"] = [str(v.dtype) for v in blob.values()]
                entry["shapes"] = [list(v.shape) for v in blob.values()]
                entry["sums"] = [float(v.double().sum()) for v in blob.values()]
            files[rel] = entry
    return dict(sorted(files.items()))


def _n3_model(seed, dtype):
    from metamorph_amd.factory import build_model
    from oracle.ref_model import OracleConfig, init_state_dict
    cfg = OracleConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                       vocab_size=128258, v_layers=2, v_intermediate=144, v_image=56, num_image_tokens=4, tokenizer_model_max_length=64)
    llm = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
               vocab_size=128258, rms_norm_eps=1e-5, rope_theta=500000.0)
    geo = dict(hidden_size=1152, intermediate_size=144, num_hidden_layers=2, num_attention_heads=16, image_size=56, patch_size=14)
    return build_model(llm, geo, num_image_tokens=4, max_length=64, state_dict=init_state_dict(cfg, seed=seed), dtype=dtype)


def test_checkpoint_layouts_match_reference_recorded(tmp_path):
    """Row N3 PINNED: tests/golden/n3_checkpoint_layouts.json records what the reference's own `safe_save_model_for_hf_trainer`
    (train.py:186-222) and `MetaMorphTrainer._save_checkpoint` / `_save` (metamorph_trainer.py:273-298) wrote for a tiny model
    (oracle/gen_golden.py n3): relative paths, key ORDER, dtypes, shapes and a checksum per tensor of every `.bin`.  The same seeded
    weights in this build's model through `checkpoint.py` / `MetaMorphTrainer` must produce the same listing."""
    from types import SimpleNamespace
    from metamorph_amd.checkpoint import safe_save_model, save_trainer_adapter_checkpoint
    from metamorph_amd.trainer import MetaMorphTrainer
    g = json.load(open(os.path.join(GOLDEN, "n3_checkpoint_layouts.json")))
    models = {"bf16": _n3_model(g["seed"], torch.bfloat16), "f32": _n3_model(g["seed"], torch.float32)}
    n = 0
    for i, c in enumerate(g["cases"]):
        m = models[c["dtype"]]
        root = tmp_path / f"case{i}"
        if c["fn"] == "safe_save_model_for_hf_trainer":
            safe_save_model(m, str(root / c["output_dir"]), tune_mm_mlp_adapter=True, use_im_start_end=c["use_im_start_end"])
        elif c["fn"] == "MetaMorphTrainer._save_checkpoint":
            run = str(root / "run")
            args = SimpleNamespace(tune_mm_mlp_adapter=True, use_im_start_end=c["use_im_start_end"], local_rank=-1, should_save=True, output_dir=run)
            stub = SimpleNamespace(args=args, model=m, state=SimpleNamespace(global_step=c["global_step"]), _get_output_dir=lambda trial=None, run=run: run)
            MetaMorphTrainer._save_checkpoint(stub, m, None)
            MetaMorphTrainer._save(stub, os.path.join(run, "ignored"))           # adapter runs: `_save` writes nothing
        else:                                                                    # full model: a CPU state dict under the reference's keys
            sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
            keys = list(sd.keys())
            assert [k for k in keys if "vision_tower" not in k] == c["keys_without_tower"]
            assert sorted({str(v.dtype) for v in sd.values()}) == c["dtypes"]
            n += 1
            continue
        got = _listing(root)
        want = c["files"]
        assert list(got) == list(want), (c, list(got))
        for rel in want:
            for field in ("keys", "dtypes", "shapes"):
                assert got[rel].get(field) == want[rel].get(field), (c["fn"], rel, field)
            if "sums" in want[rel]:
                assert got[rel]["sums"] == pytest.approx(want[rel]["sums"], rel=1e-6, abs=1e-6), (c["fn"], rel)
        n += 1
    assert n == len(g["cases"]) == 14
    # re-load (metamorph_arch.py:91-96): an adapter file written with embed_tokens in it changes the projector only
    from metamorph_amd.checkpoint import get_mm_adapter_state
    donor = _n3_model(48, torch.float32)
    blob = get_mm_adapter_state(donor.named_parameters(), ["mm_projector", "embed_tokens"])
    assert list(blob) == g["reload"]["adapter_keys"]
    path = str(tmp_path / "mm_projector.bin")
    torch.save(blob, path)
    fresh = models["f32"]
    before = {k: v.detach().clone() for k, v in fresh.state_dict().items()}
    margs = SimpleNamespace(vision_tower="siglip/CLIP-ViT-SO400M-14-384", mm_vision_select_layer=-1, mm_vision_select_feature="patch",
                            pretrain_mm_mlp_adapter=path, mm_projector_type="mlp2x_gelu", mm_patch_merge_type="flat",
                            image_token_reduction="interpolation", num_image_tokens=4, freeze_vision=True, normalize_vision=True,
                            apply_softmax=False, vision_coef=1.0)
    fresh.get_model().initialize_vision_modules(margs, fsdp=None)
    after = fresh.state_dict()
    changed = sorted(k for k in before if k in after and not torch.equal(before[k], after[k]))
    from_blob = sorted(k for k in changed if k in blob and torch.equal(after[k], blob[k].to(after[k].dtype)))
    assert from_blob == g["reload"]["changed_to_adapter_values"]
    # the reference also re-creates the dead `vision_proj` Linear with fresh random weights (:86); nothing else may change
    assert set(changed) - set(g["reload"]["changed_keys"]) == set() and set(from_blob) <= set(changed)


# ------------------------------------------------------------------ N2: image pre-processing (caller side, CPU)
def test_process_images_matches_reference_golden():
    """mm_utils.process_images / expand2square + the hub-free SigLIP image processor against outputs recorded from the
    reference's own process_images driving transformers' SiglipImageProcessor (oracle/gen_golden.py images)."""
    from types import SimpleNamespace
    from PIL import Image
    from metamorph_amd.image_processing import SiglipImageProcessor
    from metamorph_amd.mm_utils import expand2square, process_images
    g = np.load(os.path.join(GOLDEN, "n2_process_images.npz"))
    names = [str(n) for n in g["names"]]
    proc = SiglipImageProcessor(size=int(g["size"]))
    pil = {n: Image.fromarray(g["in_" + n]) for n in names}
    bg = tuple(int(x * 255) for x in proc.image_mean)
    for n in ("wide", "tall"):
        assert np.array_equal(np.asarray(expand2square(pil[n], bg)), g["square_of_" + n]), n
    sq = expand2square(pil["square"], bg)
    assert sq.size == pil["square"].size and np.array_equal(np.asarray(sq), g["in_square"])
    pad = process_images([pil[n].convert("RGB") for n in names], proc, SimpleNamespace(image_aspect_ratio="pad"))
    plain = process_images([pil[n] for n in names], proc, SimpleNamespace(image_aspect_ratio=None))
    assert pad.dtype == torch.float32 and tuple(pad.shape) == g["pad"].shape
    assert np.abs(pad.numpy() - g["pad"]).max() <= 1e-6
    assert np.abs(plain.numpy() - g["plain"]).max() <= 1e-6
    # uint8 arrays (HWC / CHW) go the same way as PIL images
    hwc = g["in_wide"]
    a = proc.preprocess(hwc, return_tensors="pt")["pixel_values"]
    b = proc.preprocess(np.ascontiguousarray(hwc.transpose(2, 0, 1)), return_tensors="pt")["pixel_values"]
    c = proc.preprocess(pil["wide"], return_tensors="pt")["pixel_values"]
    assert torch.equal(a, c) and torch.equal(b, c)


def test_tower_carries_an_image_processor_without_the_hub():
    from types import SimpleNamespace
    from metamorph_amd.model.multimodal_encoder.siglip_encoder import SiglipVisionTower
    args = SimpleNamespace(mm_vision_geometry=dict(hidden_size=32, intermediate_size=48, num_hidden_layers=1, num_attention_heads=2,
                                                   image_size=28, patch_size=14, layer_norm_eps=1e-6))
    tower = SiglipVisionTower("siglip/CLIP-ViT-SO400M-14-384", args, delay_load=True)
    assert tower.image_processor is None
    tower.load_model(random_init=True)
    ip = tower.image_processor
    assert ip.crop_size == {"height": 384, "width": 384} and tuple(ip.image_mean) == (0.5, 0.5, 0.5)


def test_conversation_templates_match_reference_prompts():
    """conv_templates[...].copy() / append_message / get_prompt against prompts recorded from the reference's templates."""
    from metamorph_amd import conversation as C
    g = json.load(open(os.path.join(GOLDEN, "n2_conversation.json")))
    assert C.default_conversation.version == g["default"]
    for case in g["cases"]:
        conv = C.conv_templates[case["template"]].copy()
        assert list(conv.roles) == case["roles"] and conv.sep == case["sep"] and conv.system == case["system"]
        assert conv.version == case["version"]
        for r, m in case["turns"]:
            conv.append_message(conv.roles[r], tuple(m) if isinstance(m, list) else m)
        assert conv.get_prompt() == case["prompt"], (case["template"], case["dialog"])
        assert C.conv_templates[case["template"]].messages == []          # copy() does not leak messages into the template
    with pytest.raises(ValueError):
        C.Conversation(system="", roles=("a", "b"), messages=[], sep_style=C.SeparatorStyle.TWO).get_prompt()


def test_splice_plan_refuses_what_the_reference_refuses():
    """one image too few, or a token id outside the vocabulary, is an IndexError in the reference
    (image_features[cur_image_idx] at metamorph_arch.py:277,320; nn.Embedding at :278,298) -- never an out-of-bounds device gather."""
    from metamorph_amd.splice_plan import build_splice_plan
    A, ST, IM, EN = 128000, 128256, -200, 128257
    ids = np.array([[A, 5, ST, IM, EN, 6, ST, IM, EN, 7]])
    lab = np.array([[-100, -100, ST, IM, EN, 6, ST, IM, EN, 7]])
    build_splice_plan(ids, lab, None, 2, 4, 64)                              # two answer images, two supplied: fine
    with pytest.raises(IndexError):
        build_splice_plan(ids, lab, None, 1, 4, 64)                          # ... one supplied
    with pytest.raises(IndexError):                                          # text-only sample needs its dummy image as well
        build_splice_plan(np.array([[A, IM, 7], [A, 8, 9]]), None, None, 1, 4, 64)
    with pytest.raises(IndexError):
        build_splice_plan(np.array([[A, 5, 128258]]), None, None, 1, 4, 64, vocab_size=128258)
    with pytest.raises(IndexError):
        build_splice_plan(np.array([[A, -7, 5]]), None, None, 1, 4, 64, vocab_size=128258)
    build_splice_plan(np.array([[A, 5, 128257]]), None, None, 1, 4, 64, vocab_size=128258)


def test_vision_tower_name_grammar_matches_reference():
    """`extract_res_interp` against outputs recorded from the reference function (siglip_encoder.py:34-59), errors included."""
    from metamorph_amd.model.multimodal_encoder.siglip_encoder import extract_res_interp
    for name, want in json.load(open(os.path.join(GOLDEN, "a10_tower_names.json"))):
        if want == "ValueError":
            with pytest.raises(ValueError):
                extract_res_interp(name)
        else:
            assert list(extract_res_interp(name)) == want, name


# ------------------------------------------------------------------ the rest of the Python surface, reference-recorded
def _surface():
    with open(os.path.join(GOLDEN, "surface.json")) as f:
        return json.load(f)


def test_get_model_name_from_path_matches_reference_recorded():
    from metamorph_amd.mm_utils import get_model_name_from_path
    for path, want in _surface()["model_names"].items():
        if want.endswith("Error"):                                # a bare "checkpoint-N" has no parent folder: the reference raises IndexError
            with pytest.raises(IndexError):
                get_model_name_from_path(path)
        else:
            assert get_model_name_from_path(path) == want, path


def test_keywords_stopping_criteria_matches_reference_recorded():
    """mm_utils.py:226-258 on 107 recorded cases: id-suffix match, decoded-text match over the last min(new tokens, max_keyword_len)
    tokens only (so "the answer is yes no" does NOT stop on "answer is yes"), BOS stripped from keyword ids, every row of a batch must stop."""
    from metamorph_amd.mm_utils import KeywordsStoppingCriteria
    from oracle.fake_tokenizer import VocabTokenizer
    g = _surface()
    prompt = torch.tensor([g["prompt_ids"]])
    enc = lambda text: VocabTokenizer(add_bos=True)(text).input_ids[1:]
    n_stop = 0
    for c in g["stopping"]:
        crit = KeywordsStoppingCriteria(c["keywords"], VocabTokenizer(add_bos=c["add_bos"]), prompt)
        assert (crit.max_keyword_len, crit.start_len) == (c["max_keyword_len"], c["start_len"])
        gens = c["generated"] if isinstance(c["generated"], list) else [c["generated"]]
        ids = torch.cat([prompt.repeat(len(gens), 1), torch.tensor([enc(x) for x in gens], dtype=torch.long)], 1)
        assert bool(crit(ids, None)) == c["stop"], c
        n_stop += c["stop"]
    assert n_stop == 13 and len(g["stopping"]) == 107


def test_initialize_vision_tokenizer_matches_reference_recorded(tmp_path):
    """metamorph_arch.py:427-469 on 16 recorded runs of the reference (fp32 and bf16 weights): tokens added, embedding / lm_head resized with
    the old rows untouched, the start / end rows = the mean of the old rows IN THE WEIGHTS' dtype (or the rows of a stage-1 adapter file of
    either accepted shape; any other shape is the reference's ValueError), and the requires_grad policy of `tune_mm_mlp_adapter`."""
    from types import SimpleNamespace
    from metamorph_amd.factory import build_model
    from oracle.fake_tokenizer import VocabTokenizer
    from oracle.ref_model import OracleConfig, init_state_dict
    g = _surface()
    cfg = OracleConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=512,
                       v_layers=2, v_intermediate=144, v_image=56, num_image_tokens=4, tokenizer_model_max_length=64)
    sd = init_state_dict(cfg, seed=g["seed"])
    rng = np.random.default_rng(52)
    adapters = {}
    for kind, rows in (("full", 514), ("rows", 2), ("bad", 7)):
        w = torch.from_numpy(rng.standard_normal((rows, 64), dtype=np.float32))
        assert float(w.double().sum()) == g["adapter_rows_sum"][kind]
        adapters[kind] = str(tmp_path / f"adapter_{kind}.bin")
        torch.save({"model.embed_tokens.weight": w}, adapters[kind])
    llm = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=512,
               rms_norm_eps=1e-5, rope_theta=500000.0)
    geo = dict(hidden_size=1152, intermediate_size=144, num_hidden_layers=2, num_attention_heads=16, image_size=56, patch_size=14)
    assert len(g["vision_tokenizer"]) == 16
    for c in g["vision_tokenizer"]:
        dt = torch.float32 if c["dtype"] == "f32" else torch.bfloat16
        model = build_model(llm, geo, num_image_tokens=4, max_length=64, state_dict=sd, dtype=dt)
        tk = VocabTokenizer()
        margs = SimpleNamespace(mm_use_im_patch_token=c["mm_use_im_patch_token"], mm_use_im_start_end=c["mm_use_im_start_end"],
                                tune_mm_mlp_adapter=c["tune_mm_mlp_adapter"], pretrain_mm_mlp_adapter=adapters[c["adapter"]] if c["adapter"] else None)
        if c["error"]:
            with pytest.raises(ValueError):
                model.initialize_vision_tokenizer(margs, tk)
        else:
            model.initialize_vision_tokenizer(margs, tk)
        ie, oe = model.get_input_embeddings().weight, model.get_output_embeddings().weight
        assert (len(tk), tk.added) == (c["len_tokenizer"], c["added"]), c
        assert list(ie.shape) == c["embed_shape"] and list(oe.shape) == c["lm_head_shape"] and model.config.vocab_size == c["config_vocab_size"]
        assert [ie.requires_grad, oe.requires_grad] == c["requires_grad"], c
        assert torch.equal(ie.data[:512].float(), sd["model.embed_tokens.weight"].to(dt).float()) and torch.equal(oe.data[:512].float(), sd["lm_head.weight"].to(dt).float())
        if c["new_embed_rows"]:
            assert torch.equal(ie.data[-2:].float(), torch.tensor(c["new_embed_rows"])), c     # bit-exact, bf16 included
            assert torch.equal(oe.data[-2:].float(), torch.tensor(c["new_lm_head_rows"])), c
        elif c["mm_use_im_start_end"] and not c["error"]:         # after a (randomly initialised) patch-token row: the mean includes that row
            assert torch.equal(ie.data[-2:], ie.data[:-2].mean(dim=0, keepdim=True).expand(2, -1))
            assert torch.equal(oe.data[-2:], oe.data[:-2].mean(dim=0, keepdim=True).expand(2, -1))


def test_optimizer_parameter_groups_match_reference_recorded():
    """`MetaMorphTrainer.create_optimizer`'s grouping (reference metamorph_trainer.py:154-245) recorded from the reference on the same tiny
    model, tower frozen and trainable, with `mm_projector_lr` / `vision_lr` (the former wins when both are set): same parameter names in the
    same groups, same per-group lr / weight decay.  Norm weights (RMSNorm included, as under the reference's pinned transformers) and biases
    are not decayed.  Empty groups are dropped here; the attention-pool `head.*` of the HF tower does not exist in this build."""
    from metamorph_amd.factory import build_model
    from metamorph_amd.trainer import optimizer_grouped_parameters
    with open(os.path.join(GOLDEN, "n4_optimizer_groups.json")) as f:
        cases = json.load(f)["cases"]
    llm = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=128258,
               rms_norm_eps=1e-5, rope_theta=500000.0)
    geo = dict(hidden_size=1152, intermediate_size=144, num_hidden_layers=2, num_attention_heads=16, image_size=56, patch_size=14)
    model = build_model(llm, geo, num_image_tokens=4, max_length=64)
    mine = {n for n, _ in model.named_parameters()}
    assert len(cases) == 8
    for c in cases:
        for n, p in model.named_parameters():
            p.requires_grad_(c["train_tower"] or "vision_tower" not in n)
        name_of = {id(p): n for n, p in model.named_parameters()}
        groups = optimizer_grouped_parameters(model, 0.05, c["mm_projector_lr"], c["vision_lr"])
        got = [(g["weight_decay"], g.get("lr", c["base_lr"]), [name_of[id(p)] for p in g["params"]]) for g in groups]
        want = []
        for g in c["groups"]:
            absent = [n for n in g["names"] if n not in mine]
            assert all(".vision_tower.head." in n for n in absent), absent
            names = [n for n in g["names"] if n in mine]
            if names:
                want.append((g["weight_decay"], g["lr"], names))
        assert len(got) == len(want), (c, [len(x[2]) for x in got], [len(x[2]) for x in want])
        for (wd_g, lr_g, n_g), (wd_w, lr_w, n_w) in zip(got, want):
            assert (wd_g, lr_g) == (wd_w, lr_w) and n_g == n_w, (c["train_tower"], c["mm_projector_lr"], c["vision_lr"], set(n_g) ^ set(n_w))


def test_initialize_vision_modules_side_effects_match_reference_recorded():
    """metamorph_arch.py:46-96 as the reference ran it: config fields written, a frozen projector un-frozen, `vision_proj` re-created,
    `temperature_in` 0.1 -> 1, and the ALREADY BUILT tower keeps its own `select_layer` (only the config takes the new value)."""
    from types import SimpleNamespace
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=512,
               rms_norm_eps=1e-5, rope_theta=500000.0)
    geo = dict(hidden_size=1152, intermediate_size=144, num_hidden_layers=2, num_attention_heads=16, image_size=56, patch_size=14)
    for c in _surface()["vision_modules"]:
        model = build_model(llm, geo, num_image_tokens=4, max_length=64)
        inner = model.get_model()
        for p in inner.mm_projector.parameters():
            p.requires_grad_(not c["projector_frozen_before"])
        old_proj = inner.vision_proj
        assert inner.temperature_in == c["temperature_in_before"]
        margs = SimpleNamespace(vision_tower=c["config"]["mm_vision_tower"], mm_vision_select_layer=c["config"]["mm_vision_select_layer"],
                                mm_vision_select_feature=c["config"]["mm_vision_select_feature"], pretrain_mm_mlp_adapter=None,
                                mm_projector_type=c["config"]["mm_projector_type"], mm_patch_merge_type=c["config"]["mm_patch_merge_type"])
        inner.initialize_vision_modules(margs, fsdp=None)
        assert {k: getattr(model.config, k) for k in c["config"]} == c["config"]
        assert inner.temperature_in == c["temperature_in"] and (inner.vision_proj is not old_proj) == c["vision_proj_is_new_object"]
        assert list(inner.vision_proj.weight.shape) == c["vision_proj_shape"]
        assert [p.requires_grad for p in inner.mm_projector.parameters()] == c["projector_requires_grad"]
        assert inner.vision_tower.select_layer == c["tower_select_layer_attr"]


def test_splice_plan_matches_reference_on_120_random_batches():
    """tests/golden/a5rand_reference.npz: what the REFERENCE's prepare_inputs_labels_for_multimodal returned for 120 seeded random ragged batches
    (0-3 images per sample, answer / prompt images, overflow drops, truncation, text-only samples with their dummy image, every fifth case
    left-padded; oracle/gen_golden.py a5rand).  Both the product's plan builder and the oracle's loop restatement must reproduce labels, mask,
    image positions, kept targets and the origin of every spliced row bit for bit."""
    from metamorph_amd.splice_plan import build_splice_plan
    from oracle.gen_inputs import a5_random_batches
    from oracle.ref_plan import splice_bookkeeping
    g = np.load(os.path.join(GOLDEN, "a5rand_reference.npz"))
    cases = a5_random_batches(int(g["n_cases"]), int(g["seed"]))
    stats = dict(left=0, dropped=0, answer=0)
    for ci, (rows, labs, Timg, max_len, side) in enumerate(cases):
        T_ = max(len(r) for r in rows)
        ids_a = np.array([r + [128001] * (T_ - len(r)) for r in rows])
        lab_a = np.array([r + [-100] * (T_ - len(r)) for r in labs])
        msk_a = ids_a != 128001
        n_img = sum(max(1, r.count(-200)) for r in rows)
        B, L = g["out_shape"][ci].tolist()
        want = {k: g[k][ci, :B, :L] for k in ("out_labels", "out_attention_mask", "out_image_positions", "out_src")}
        keep = [int(x) for x in g["out_target_keep"][ci] if x >= 0]
        plan = build_splice_plan(ids_a, lab_a, msk_a, n_img, Timg, max_len, side)
        assert (plan.B, plan.L) == (B, L), ci
        assert np.array_equal(plan.src.reshape(B, L), want["out_src"]), ci
        assert np.array_equal(plan.labels, want["out_labels"]) and np.array_equal(plan.image_positions, want["out_image_positions"]), ci
        assert np.array_equal(plan.attention_mask, want["out_attention_mask"].astype(bool)) and plan.target_keep.tolist() == keep, ci
        ref = splice_bookkeeping(ids_a.tolist(), lab_a.tolist(), msk_a.tolist(), n_img, Timg, max_len, side)
        src = [[-1 if s is None else (-2 - (s[1] * Timg + s[2]) if isinstance(s, tuple) else s) for s in row] for row in ref["src"]]
        assert np.array_equal(np.array(src), want["out_src"]) and np.array_equal(np.array(ref["labels"]), want["out_labels"]), ci
        assert np.array_equal(np.array(ref["image_positions"]), want["out_image_positions"]) and ref["target_keep"] == keep, ci
        stats["left"] += side == "left"
        stats["dropped"] += int(sum(r.count(-200) for r in rows) * Timg > (want["out_src"] <= -2).sum())
        stats["answer"] += len(keep)
    assert stats["left"] == 24 and stats["dropped"] >= 10 and stats["answer"] == 180, stats


def test_preprocess_llama3_matches_reference_on_random_conversations():
    """tests/golden/n2_random.json: 40 seeded random conversations x 5 tokenizer / template settings through the REFERENCE's
    preprocess_multimodal + preprocess_llama3 (1-4 rounds, empty answers, <image> at any place of either role's turn, a leading gpt turn,
    truncation at 24 tokens; the tokenization-mismatch rule that masks a whole sample fires in 91 of the 200 cases)."""
    import copy
    from types import SimpleNamespace
    from metamorph_amd.data import preprocess, preprocess_multimodal
    from oracle.fake_tokenizer import FakeTokenizer
    from oracle.gen_inputs import n2_random_sources
    with open(os.path.join(GOLDEN, "n2_random.json")) as f:
        g = json.load(f)
    sources = n2_random_sources(g["n_sources"], g["seed"])
    assert len(g["cases"]) == 200
    masked = 0
    for c in g["cases"]:
        tok = FakeTokenizer(add_bos=c["add_bos"], model_max_length=c["model_max_length"])
        tag = (c["source"], c["add_bos"], c["mm_use_im_start_end"], c["model_max_length"])
        src = preprocess_multimodal(copy.deepcopy(sources[c["source"]]), SimpleNamespace(is_multimodal=True, mm_use_im_start_end=c["mm_use_im_start_end"]))
        out = preprocess(src, tok, has_image=c["has_image"])
        assert out["input_ids"].tolist() == c["input_ids"], tag
        assert out["labels"].tolist() == c["labels"], tag
        masked += all(x == -100 for x in c["labels"][0])
    assert masked == 91




def test_bench_rccl_log_summary_and_bus_bandwidth(tmp_path):
    """bench.py at N > 1 summarises RCCL's own NCCL_DEBUG=INFO log into the JSON line (the driver's 8-GPU run cannot be observed
    otherwise): version, channel count, algorithm / protocol per collective, transports, the head of the log; bus bandwidth =
    bytes (world - 1) / world / exposed time.  Pure host logic: exercised here on a synthetic log in RCCL's format."""
    import sys
    sys.path.insert(0, REPO)
    import bench
    log = tmp_path / "rccl.log"
    log.write_text("\n".join([
        "host:123:123 [0] NCCL INFO Kernel version: 6.18.51-ant.1",
        "host:123:123 [0] NCCL INFO RCCL version : 2.26.6-HEAD:64f48b6",
        "host:123:140 [0] NCCL INFO comm 0x1 rank 0 nranks 8 cudaDev 0 busId 1000 - Init START",
        "host:123:140 [0] NCCL INFO Channel 00/32 : 0 1 2 3 4 5 6 7",
        "host:123:140 [0] NCCL INFO Channel 00 : 0[0] -> 1[1] via P2P/IPC",
        "host:123:140 [0] NCCL INFO 32 coll channels, 32 collnet channels, 0 nvls channels, 32 p2p channels, 2 p2p channels per peer",
        "host:123:150 [0] NCCL INFO ReduceScatter: opCount 5 sendbuff 0x1 recvbuff 0x2 count 27262976 datatype 9 op 0 root 0 comm 0x1 [nranks=8] stream 0x3",
        "host:123:150 [0] NCCL INFO ReduceScatter: 218103808 Bytes -> Algo RING proto SIMPLE channel{Lo..Hi}={0..31}",
        "host:123:151 [0] NCCL INFO AllGather: 218103808 Bytes -> Algo RING proto LL128 nchannels 16",
        "host:123:151 [0] NCCL INFO AllGather: 218103808 Bytes -> Algo RING proto LL128 nchannels 16",
    ]) + "\n")

    class Opt:
        def comm_bytes_per_step(self):
            return {"reduce_scatter_bytes": 16_000_000_000, "all_gather_bytes": 16_000_000_000}

    out = bench.rccl_summary(str(log), Opt(), steps=4, world=8)
    assert out["version"] == "2.26.6-HEAD:64f48b6" and out["coll_channels"] == 32 and out["log_lines"] == 10 and 6 <= len(out["log_head"]) <= 9 and not any("Kernel version" in ln for ln in out["log_head"])
    seen = out["collectives_seen"]
    assert seen.get("AllGather: algo RING proto LL128 channels 16") == 2 and any(k.startswith("ReduceScatter: algo RING proto SIMPLE") for k in seen)
    assert out["transport_lines"]["p2p_or_xgmi"] >= 1 and out["bytes_per_step"]["all_gather_bytes"] == 16_000_000_000
    bw = bench.bus_bandwidth(out, {"all_gather": 50.0, "reduce_scatter_exposed": 40.0}, world=8, overlap=False)
    assert bw == {"all_gather_gb_s": 280.0, "reduce_scatter_gb_s": 350.0}
    assert bench.bus_bandwidth(out, {"all_gather": 50.0, "reduce_scatter_exposed": 4.0}, world=8, overlap=True) == {"all_gather_gb_s": 280.0}
    assert bench.bus_bandwidth(out, {"all_gather": 50.0}, world=1, overlap=False) is None
    assert bench.rccl_summary(str(tmp_path / "missing.log"), Opt(), 1, 8) == {"log": str(tmp_path / "missing.log")}


@pytest.mark.parametrize("gen,sub", [("gen_attn4", "attn4_gen"), ("gen_attn4_bwd", "attn4_bwd_gen")])
def test_committed_instruction_streams_are_what_the_generators_emit(tmp_path, monkeypatch, gen, sub):
    """The hand-placed streams (csrc/*_gen/*.inc: one asm statement per instruction) are build inputs generated by tools/gen_*.py; the
    committed files must be exactly what the committed generators emit -- no hand edits, no stale files."""
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location(gen, os.path.join(REPO, "tools", gen + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = str(tmp_path / sub)
    monkeypatch.setattr(sys, "argv", [gen + ".py"])
    monkeypatch.setattr(mod, "OUT", out)
    mod.main()
    committed = os.path.join(REPO, "metamorph_amd", "csrc", sub)
    new, old = sorted(os.listdir(out)), sorted(f for f in os.listdir(committed) if f.endswith(".inc"))
    assert new == old, (set(new) ^ set(old))
    for f in new:
        assert open(os.path.join(out, f)).read() == open(os.path.join(committed, f)).read(), f


def test_compiler_stays_out_of_the_attention_streams_registers():
    """tools/audit_attn4.py on the code objects of csrc/attn4.hip and attn4_bwd.hip (compiled here with the build's flags):
    outside the asm statements no instruction may name a VGPR at or above the kernel's amdgpu_num_vgpr limit or any AGPR, and there is no
    scratch traffic and no VGPR spill -- a compiler copy into a register the hand-placed stream owns would be silent corruption."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("audit_attn4", os.path.join(REPO, "tools", "audit_attn4.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name in ("attn4", "attn4_bwd"):
        bad, stats = mod.audit(mod.compile_s(name))
        assert stats and all(v["mfma"] >= 64 and v["asm_lines"] > v["mfma"] for v in stats.values()), (name, stats)
        assert not bad, (name, bad[:5])


def test_batched_gemv_lds_relayout_is_conflict_free():
    """csrc/decode.hip, gemv_mfma_kernel<.., WLDS>: a 256-column block of 16 weight rows is loaded coalesced (instruction u: rows 2u and
    2u + 1, lanes 0..31 / 32..63, 16 B per lane), written to wave-private LDS with rows WROW = 544 bytes apart and read back as MFMA
    fragments (lane fr = lane & 15, fq = lane >> 4: row fr, 16 B at k-step u, quarter fq).  Restated here: every lane of a read gets the
    16 bytes its row / step / quarter were written with, and both the writes and the reads are bank-conflict free in each of the four
    16-lane groups the hardware services together (MI355X_MICROARCH.md, LDS table) -- 16 different 16-byte slots of the 256-byte bank row."""
    WROW = 544
    groups = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
              list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)), list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]
    where = {}                                                   # LDS byte address -> (row of the 16, first column of the 8)
    for u in range(8):
        wr = {lane: (2 * u + (lane >> 5)) * WROW + (lane & 31) * 16 for lane in range(64)}
        for lane, addr in wr.items():
            assert addr not in where
            where[addr] = (2 * u + (lane >> 5), (lane & 31) * 8)
        for g in groups:
            assert len({(wr[l] >> 4) & 15 for l in g}) == 16, ("write", u)
    assert len(where) == 16 * 32 and max(where) + 16 <= 16 * WROW
    for u in range(8):
        rd = {lane: (lane & 15) * WROW + u * 64 + (lane >> 4) * 16 for lane in range(64)}
        for lane, addr in rd.items():
            assert where[addr] == (lane & 15, u * 32 + (lane >> 4) * 8)      # A operand: row fr, k = 32 u + 8 fq .. + 7
        for g in groups:
            assert len({(rd[l] >> 4) & 15 for l in g}) == 16, ("read", u)


def test_decode_gemv_window_addressing():
    """csrc/decode.hip, gemv_deep_kernel: the x rows sit in LDS in windows of WT trips (a trip = 1024 columns = two 512-column chunks, a
    lane takes 8 columns of a chunk).  Restated: for every K the trips of all windows cover every column below K exactly once, the LDS
    column a lane reads for trip j of window `win` is the global column minus the window's first column, lies inside the window row
    (`wk` columns), and the clamp that keeps the reads of a trip BEHIND the end inside the row never moves a valid read."""
    for WT in (4, 16):
        for K in (8, 64, 512, 1032, 1152, 4096, 4104, 5120, 8192, 12288, 14336, 16384, 16392, 16896, 40000):
            ntrip = (K + 1023) // 1024
            nwin = (ntrip + WT - 1) // WT
            wk = min(ntrip, WT) * 1024
            seen = set()
            for win in range(nwin):
                nt = min(WT, ntrip - win * WT)
                for j0 in range(0, nt, 2):                       # the ring holds two trips: pairs, the second may lie behind the end
                    for j in (j0, j0 + 1):
                        t = win * WT + j
                        for ch in range(2):
                            for lane in (0, 1, 31, 63):
                                k = (t * 2 + ch) * 512 + lane * 8
                                col = min((j * 2 + ch) * 512, wk - 512) + lane * 8
                                assert 0 <= col and col + 8 <= wk, (WT, K, win, j, ch, lane)
                                if k < K:
                                    assert col == k - win * WT * 1024, (WT, K, win, j, ch, lane)
                                    if lane == 0:
                                        seen.add(k // 512)
            assert seen == set(range((K + 511) // 512)), (WT, K)


def test_batched_gemv_x_window_protocol():
    """csrc/decode.hip, gemv_mfma_kernel<.., XK>: the x rows of block b live in LDS buffer b & 1.  Program order of every wave, restated:
    store blocks 0, 1; barrier; then per pair (bk, bk + 1): read buffer 0 (block bk); barrier; store block bk + 2 into buffer 0; read
    buffer 1 (block bk + 1); barrier; store block bk + 3 into buffer 1.  Waves run freely between barriers, so within one barrier phase
    any wave's stores may precede or follow any other wave's reads: the protocol is right iff (1) no phase holds a store to and a read
    of the same buffer, and (2) every read finds the block it wants, stored in an EARLIER phase and not overwritten since.  All waves run
    the same number of pairs (nbu) -- a barrier count that depended on the wave's own slice would hang the workgroup."""
    for nbu in range(0, 9):
        phases = [[("store", 0, 0), ("store", 1, 1)], []]        # ops of ONE wave per barrier phase (all waves run the same list); the
        for bk in range(0, nbu, 2):                              # barrier behind the first two stores opens the second phase
            phases[-1].append(("read", 0, bk))                   # ... read buffer 0, then the barrier ends the phase
            phases.append([("store", 0, bk + 2), ("read", 1, bk + 1)])
            phases.append([("store", 1, bk + 3)])
        content = {0: None, 1: None}                             # what a buffer holds once the phase's stores are all done
        for ph in phases:
            stores = {buf: blk for op, buf, blk in ph if op == "store"}
            reads = [(buf, blk) for op, buf, blk in ph if op == "read"]
            for buf, blk in reads:
                assert buf not in stores, (nbu, ph)              # (1): another wave could be on either side of it
                assert content[buf] == blk, (nbu, ph, content)   # (2)
            content.update(stores)
        n_barriers = len(phases) - 1
        assert n_barriers == 1 + 2 * ((nbu + 1) // 2)            # a function of nbu only
    # the uniform pair count: the longest slice's number of complete 8-step blocks, from (K, slices) only
    def nbu_of(K, XK):
        nst = (K + 31) // 32
        complete = nst - 1 if K % 32 else nst
        return max(max(min(nst * (q + 1) // XK, complete) - nst * q // XK, 0) // 8 for q in range(XK))
    assert nbu_of(4096, 1) == 16 and nbu_of(4096, 4) == 4 and nbu_of(14336, 4) == 14 and nbu_of(1032, 4) == 1 and nbu_of(512, 4) == 0


def test_fused_decode_gemv_row_ownership_is_a_partition():
    """csrc/decode_gemv.h, unit_rows<MODE> (every decode GEMV kernel): a wave owns four-row units chosen so that its epilogue finds its partners in its own
    accumulators -- MODE 1 (SwiGLU): gate rows c, c + 1 and up rows I + c, I + c + 1; MODE 2 (RoPE + cache append): the rotation partners
    j, j + 1, j + d/2, j + 1 + d/2 of one q / k head, four neighbours of a v head.  The formulas, restated here, must cover every weight
    row exactly once for the geometries the models use (a row owned twice or never would be a silent wrong answer only for some heads)."""
    def units_swiglu(I):
        return [(c, c + 1, I + c, I + c + 1) for c in range(0, I, 2)]

    def units_rope(Hq, Hkv, d):
        upd, out = d // 4, []
        for unit in range((Hq + 2 * Hkv) * d // 4):
            if unit < (Hq + Hkv) * upd:
                hd, j = unit // upd, (unit % upd) * 2
                r0 = hd * d + j
                out.append((r0, r0 + 1, r0 + d // 2, r0 + d // 2 + 1))
            else:
                b0 = (Hq + Hkv) * d + (unit - (Hq + Hkv) * upd) * 4
                out.append((b0, b0 + 1, b0 + 2, b0 + 3))
        return out

    for I in (64, 1000, 14336, 28672):
        rows = sorted(r for u in units_swiglu(I) for r in u)
        assert rows == list(range(2 * I))
    for Hq, Hkv, d in ((32, 8, 128), (64, 8, 128), (8, 1, 64), (2, 1, 80), (4, 4, 64)):
        us = units_rope(Hq, Hkv, d)
        rows = sorted(r for u in us for r in u)
        assert rows == list(range((Hq + 2 * Hkv) * d)), (Hq, Hkv, d)
        for u in us[:(Hq + Hkv) * d // 4]:                    # partners stay inside one head, d/2 apart
            assert u[0] // d == u[3] // d and u[2] - u[0] == d // 2 and u[0] % d < d // 2


def test_host_mirrors_serve_the_splice_plan_without_a_device_copy():
    """metamorph_amd.hostmirror: the integer batch tensors keep their host originals when they are moved to the device, so that the splice
    plan (host integer work) needs no device -> host copy and no synchronisation.  A mirror dies with its tensor, is invalidated by an
    in-place write, and CPU tensors are their own mirror."""
    import gc
    from metamorph_amd import hostmirror as HM
    ids = torch.arange(12).view(3, 4)
    before = dict(HM.STATS)
    assert HM.host_array(ids) is not None and HM.STATS["cpu"] == before["cpu"] + 1          # a CPU tensor: its own storage, no copy
    assert np.shares_memory(HM.host_array(ids), ids.numpy())
    fake_dev = ids.clone()                                        # stands in for the device copy (same API: object identity + version)
    HM.attach(fake_dev, ids)
    ent = HM._MIRRORS[id(fake_dev)]
    assert ent[0]() is fake_dev and np.array_equal(ent[2], ids.numpy())
    v0 = fake_dev._version
    fake_dev.add_(1)                                              # an in-place write: the mirror no longer describes the tensor
    assert fake_dev._version != v0 and HM._MIRRORS[id(fake_dev)][1] == v0
    with pytest.raises(ValueError):
        HM.attach(fake_dev, ids[:2])
    n = len(HM._MIRRORS)
    del fake_dev
    gc.collect()
    assert len(HM._MIRRORS) == n - 1                              # weak: no tensor is kept alive by its mirror
    assert HM.host_array(None) is None


def test_upload_plan_packs_every_array_with_its_dtype():
    """upload_plan: the index arrays and the [B, L] tensors handed back to the caller travel in ONE buffer (16-byte aligned pieces, own
    dtypes); on the CPU path the views must reproduce the host arrays exactly."""
    from metamorph_amd.model.metamorph_arch import upload_plan
    from metamorph_amd.splice_plan import build_splice_plan
    ids = np.array([[1, 5, 128256, -200, 128257, 7, 9, 0], [1, 4, 6, 8, 3, 0, 0, 0]])
    lab = np.where(ids > 5, ids, -100)
    msk = np.array([[1] * 7 + [0], [1] * 5 + [0] * 3], dtype=bool)
    plan = build_splice_plan(ids, lab, msk, 2, 3, 64, "right", 128256, vocab_size=128258)
    pd = upload_plan(plan, "cpu", extra=dict(labels=plan.labels, mask=plan.attention_mask, image_positions=plan.image_positions,
                                             position_ids=None, keep=np.array([0], dtype=np.int32)))
    assert pd["x_labels"].dtype == torch.int64 and torch.equal(pd["x_labels"], torch.from_numpy(plan.labels))
    assert pd["x_mask"].dtype == torch.bool and torch.equal(pd["x_mask"], torch.from_numpy(plan.attention_mask))
    assert torch.equal(pd["x_image_positions"], torch.from_numpy(plan.image_positions)) and "x_position_ids" not in pd
    assert pd["x_keep"].dtype == torch.int32 and pd["x_keep"].tolist() == [0]
    for k in ("src", "feat_row", "pred_rows", "seqlens", "emb_tok", "emb_seg", "emb_pos", "ce_rows"):
        assert pd[k].dtype == torch.int32 and np.array_equal(pd[k].numpy(), np.asarray(getattr(plan, k), dtype=np.int32)), k
        assert pd[k].data_ptr() % 16 == 0 or pd[k].numel() == 0, k


def test_pre_registered_multi_gpu_prediction_model():
    """bench.predict_step: the expectation for the N-GPU runs this build never sees, written down before the driver's
    scaling run: one rank returns the measured step; more ranks subtract the sharded part of AdamW, add what the links cannot hide; the
    direct (one hop per shard) algorithm is never slower than the ring; everything is finite and the 8-GPU figures are the ones DESIGN quotes."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    seg, tail = 218_112_000 * 2.0, (8.07e9 - 32 * 218_112_000) * 2.0
    assert b.predict_step(1, 1240.0, 39.4, seg, tail) == {"world": 1, "ms_per_step": 1240.0}
    last = None
    for n in (2, 4, 8):
        r = b.predict_step(n, 1240.0, 39.4, seg, tail)
        assert r["direct"]["ms_per_step"] <= r["ring"]["ms_per_step"]
        assert r["ring"]["compute_ms"] == round(1240.0 - 39.4 * (1 - 1 / n), 1)
        assert r["ring"]["all_gather_ms"] > r["direct"]["all_gather_ms"] or n == 2
        last = r
    assert 7.0 <= last["ring"]["scaling_vs_one_rank"] <= 7.7 and 7.8 <= last["direct"]["scaling_vs_one_rank"] <= 8.2, last


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_bench_refuses_zero_timed_steps(monkeypatch):
    b = _bench_module()
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "3", "--warmup", "0", "--dump-outputs", "d"])
    a = b.parse()
    assert a.steps == 3 and a.warmup == 0 and a.dump_outputs == "d"
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        b.parse()


def test_bench_full_is_opt_in(monkeypatch):
    """A plain `bench.py --gpus 1 --steps N --warmup W` leaves out what its line does not need; `--full` asks for it."""
    b = _bench_module()
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = b.parse()
    assert a.full is False and a.no_cpu_baseline is False
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", "--full"])
    assert b.parse().full is True


def test_bench_dump_outputs_is_a_fixed_sample_within_the_size_limit(tmp_path):
    """bench.dump_outputs on stand-in objects: float32 / float64 .npy files, the same positions on every call, parameters and gradients
    sampled at the same positions, small tensors whole, at most 64 MB in all."""
    b = _bench_module()
    g = torch.Generator().manual_seed(5)
    big = torch.nn.Parameter(torch.randn(3000, 7, generator=g).to(torch.bfloat16))
    small = torch.nn.Parameter(torch.randn(10, generator=g).to(torch.bfloat16))
    frozen = torch.nn.Parameter(torch.randn(50, generator=g), requires_grad=False)
    big._mm_grad_buf = big.detach().float() * 2           # a gradient kept outside .grad, as Zero2AdamW keeps it
    small.grad = small.detach() * 4
    model = SimpleNamespace(named_parameters=lambda: [("big", big), ("frozen", frozen), ("small", small)], loss_language=1.5,
                            loss_image_ar=float("nan"))
    opt = SimpleNamespace(master=torch.randn(3 << 20, generator=g), grad_norm_value=lambda: 0.25)
    out = SimpleNamespace(loss=torch.tensor(2.0), hidden_states=torch.randn(2, 600, 1000, generator=g).to(torch.bfloat16))
    shapes = b.dump_outputs(str(tmp_path / "a"), out, model, opt)
    b.dump_outputs(str(tmp_path / "b"), out, model, opt)
    names = {"loss", "loss_language", "loss_image_ar", "grad_norm", "hidden_states", "params", "grads", "master_weights"}
    assert set(shapes) == names and sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in names)
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert x.dtype in (np.float32, np.float64) and list(x.shape) == shapes[n], n
        assert np.array_equal(x, y, equal_nan=True), n
        total += x.nbytes
    assert total <= 64 << 20
    d = tmp_path / "a"
    assert np.load(d / "loss.npy").tolist() == [2.0] and np.load(d / "grad_norm.npy").tolist() == [0.25]
    assert np.load(d / "loss_language.npy").tolist() == [1.5] and np.isnan(np.load(d / "loss_image_ar.npy")).all()
    assert shapes["hidden_states"] == [b.DUMP_FLAT_SAMPLE] and shapes["master_weights"] == [b.DUMP_FLAT_SAMPLE]
    params, grads = np.load(d / "params.npy"), np.load(d / "grads.npy")
    assert params.shape == (b.DUMP_PER_TENSOR + 10,)                  # the frozen parameter is not part of the training step's result
    np.testing.assert_array_equal(params[-10:], small.detach().float().numpy())      # small tensors whole, in order
    np.testing.assert_array_equal(grads, np.concatenate([params[:-10] * 2, params[-10:] * 4]).astype(np.float32))
    assert set(params[:-10].tolist()) <= set(big.detach().float().reshape(-1).tolist())


def test_decode_attention_bound_follows_the_host_known_lengths():
    """mm355_attn_decode sizes its launch by an upper bound on the cached lengths: 1024 (one key group, one workgroup per query head) while
    every sequence INCLUDING the row about to be appended fits, the cache's capacity afterwards; a cache smaller than 1024 rows is its own
    bound.  functional.decode_kv_bound reads the host mirror of the lengths only."""
    import types
    import metamorph_amd.functional as F

    def cache(lengths, cap):
        return types.SimpleNamespace(lengths=list(lengths), length=max(lengths), max_len=cap)
    assert F.decode_kv_bound(cache([5, 700, 1022], 4096)) == 1024
    assert F.decode_kv_bound(cache([5, 700, 1023], 4096)) == 1024          # the appended row makes 1024: still one group
    assert F.decode_kv_bound(cache([5, 700, 1024], 4096)) == 4096
    assert F.decode_kv_bound(cache([3000], 4096)) == 4096
    assert F.decode_kv_bound(cache([10, 20], 644)) == 644                  # capacity below one group: the capacity
    assert F.decode_kv_bound(cache([10, 20], 1024)) == 1024
