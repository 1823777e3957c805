"""MetaMorphLlamaForCausalLM on MI355X kernels -- drop-in for the reference class of the same name
(reference metamorph/model/language_model/metamorph_llama.py:129-738).

Same constructor, same `forward` signature and `CausalLMOutputWithPast` contract, same side-effect attributes
(`loss_language`, `loss_image_ar`), same state-dict keys; the arithmetic is libmm355 (hand-written gfx950
HIP) instead of transformers' LlamaModel + torch ops:

  reference                                         here
  ------------------------------------------------  --------------------------------------------------------
  HF LlamaModel, 32 x LlamaDecoderLayer             functional.DecoderLayerFn (one autograd node per layer:
    (RMSNorm, q/k/v/o Linear, RoPE, SDPA, SwiGLU)      fused qkv / gate-up GEMMs, flash attention, fused
                                                       residual epilogues, hand-written backward)
  lm_head -> fp32 logits [B,L,V] -> CrossEntropy    functional.LinearCrossEntropyFn (chunked, target rows only)
  mask-multiply + boolean index (device sync)       row gather by the host plan (no sync)
  vision_head -> F.normalize -> cosine_similarity   GEMMs + fused cosine loss kernel
  three .item() syncs per step                      device-side combine; floats materialise only when read
"""
from __future__ import annotations


import copy
import math
import operator
import numpy as np
import torch
import torch.nn as nn
from transformers import AutoConfig, AutoModelForCausalLM, GenerationMixin, LlamaConfig, PreTrainedModel
from transformers.cache_utils import DynamicCache
from transformers.modeling_outputs import CausalLMOutputWithPast

from ... import functional as F
from ... import ops
from ...constants import DEFAULT_IMAGE_END_ID, DEFAULT_IMAGE_START_ID, IGNORE_INDEX
from ...splice_plan import SplicePlan, compact_row_maps
from ...hostmirror import host_array
from ...rope import head_dim as _head_dim, rope_params
from ..metamorph_arch import MetaMorphMetaForCausalLM, MetaMorphMetaModel, upload_plan
from ..modules import HipEmbedding, HipGELU, HipLinear, HipRMSNorm

BF16 = torch.bfloat16
MM355_SPEC_MAX_DRAFT = F.SPEC_MAX_DRAFT                      # greedy_decode(prompt_lookup_num_tokens=K): K <= 15 guessed tokens per step


class MetaMorphConfig(LlamaConfig):
    model_type = "metamorph_llama"


def _left_pad_maps(seqlens, B, L):
    """Row maps between the left-padded layout (valid rows [L - n_b, L)) and the right-padded one (valid rows [0, n_b)):
    (to_right [B*L]: source row of every right-layout row, -1 = zero row; to_left: the inverse; off [B] = L - n_b), all int32."""
    to_right = np.full(B * L, -1, dtype=np.int32)
    to_left = np.full(B * L, -1, dtype=np.int32)
    off = (L - np.asarray(seqlens, dtype=np.int64)).astype(np.int32)
    for b in range(B):
        n = int(seqlens[b])
        to_right[b * L:b * L + n] = b * L + off[b] + np.arange(n, dtype=np.int32)
        to_left[b * L + off[b]:(b + 1) * L] = b * L + np.arange(n, dtype=np.int32)
    return to_right, to_left, off


class _Attention(nn.Module):
    def __init__(self, config):
        super().__init__()
        h, d = config.hidden_size, _head_dim(config)
        self.q_proj = HipLinear(h, config.num_attention_heads * d, bias=False)
        self.k_proj = HipLinear(h, config.num_key_value_heads * d, bias=False)
        self.v_proj = HipLinear(h, config.num_key_value_heads * d, bias=False)
        self.o_proj = HipLinear(config.num_attention_heads * d, h, bias=False)


class _MLP(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.gate_proj = HipLinear(config.hidden_size, config.intermediate_size, bias=False)
        self.up_proj = HipLinear(config.hidden_size, config.intermediate_size, bias=False)
        self.down_proj = HipLinear(config.intermediate_size, config.hidden_size, bias=False)


class _DecoderLayer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.self_attn = _Attention(config)
        self.mlp = _MLP(config)
        self.input_layernorm = HipRMSNorm(config.hidden_size, eps=config.rms_norm_eps)
        self.post_attention_layernorm = HipRMSNorm(config.hidden_size, eps=config.rms_norm_eps)


class _SeqView:
    """Read-only view of ONE sequence of a HipKVCache (introspection: tests, debugging): its left-padding and its cached length."""

    def __init__(self, cache, b):
        self._c, self._b = cache, b

    @property
    def pad(self):
        return self._c.pads[self._b]

    @property
    def length(self):
        return self._c.kv.lengths[self._b]


class HipKVCache(DynamicCache):
    """What `past_key_values` is under HF `generate()` (reference metamorph_llama.py:711-717, `use_customize_greedy=False`): a
    `transformers` Cache whose payload is ONE `functional.KVCache` for the whole batch (batch rows / beams) -- post-RoPE keys / values of
    every decoder layer in the layout the decode kernels read ([layers, batch, max_len, Hkv*d] bf16, per-row write positions on the device)
    -- plus the captured hipGraph of the per-token step, which takes all rows through the decoder in ONE pass over the weights (as the
    reference's `forward` does: the batch goes to one HF forward per step).  HF only asks a cache for its length and, under beam search,
    to re-order its batch rows (`reorder_cache`); the tensors never leave the device or change layout."""

    def __init__(self, capacity=None, kv_format=None, prefill_chunk=None, **kw):
        super().__init__(**kw)
        if prefill_chunk is not None and int(prefill_chunk) < 1:
            raise ValueError(f"HipKVCache(prefill_chunk={prefill_chunk}): a prompt is run in slices of at least 1 row (None: in one pass)")
        self.capacity = capacity          # rows to allocate at the first (prompt) pass; None: prompt + 1024 + 2
        # a prompt of more rows runs its first prefill_chunk rows as the prompt pass and every further slice as an extend pass against the
        # rows cached so far (functional.decoder_extend); None: config.mm355_prefill_chunk_rows, whose default None is one pass
        self.prefill_chunk = None if prefill_chunk is None else int(prefill_chunk)
        self.kv_format = kv_format        # "bf16" / "fp8_e4m3" (functional.KVCache); None: config.mm355_kv_cache_format
        self.kv = None                    # functional.KVCache of the whole batch
        self.pads = []                    # left-padding rows of every sequence in the batch HF sees (never cached: kv.lengths count real rows)
        self.stepper = None               # functional.DecodeStepGraph
        self.meta = None

    @property
    def states(self):
        return [] if self.kv is None else [_SeqView(self, b) for b in range(len(self.pads))]

    def get_seq_length(self, layer_idx=0):
        # the length HF counts: padded prompt + generated tokens, the same for every row of a left-padded batch
        return 0 if self.kv is None else int(self.kv.lengths[0]) + self.pads[0]

    def get_max_cache_shape(self, layer_idx=0):
        return -1 if self.kv is None else int(self.kv.max_len)

    def reorder_cache(self, beam_idx):
        """Beam search: row i continues the hypothesis that lived in row beam_idx[i].  ONE gather over the batch dimension of the live
        prefix (every layer, keys and values) through a temporary, written back in place: buffers -- and the captured graph that points
        at them -- stay where they are; a row may be source and target at once."""
        idx = [int(i) for i in beam_idx.reshape(-1).tolist()]
        if len(idx) != len(self.pads):
            raise ValueError(f"reorder_cache: {len(idx)} indices for {len(self.pads)} sequences")
        if all(i == j for i, j in enumerate(idx)):
            return
        kv = self.kv
        n = max(kv.lengths)
        sel = torch.as_tensor(idx, dtype=torch.long, device=kv.k.device)
        kv.k[:, :, :n].copy_(kv.k[:, :, :n].index_select(1, sel))
        kv.v[:, :, :n].copy_(kv.v[:, :, :n].index_select(1, sel))
        if getattr(kv, "k_scale", None) is not None:          # an fp8_e4m3 cache: the scales travel with their bytes
            kv.k_scale[:, :, :n].copy_(kv.k_scale[:, :, :n].index_select(1, sel))
            kv.v_scale[:, :, :n].copy_(kv.v_scale[:, :, :n].index_select(1, sel))
        kv.set_lengths([kv.lengths[j] for j in idx])
        self.pads = [self.pads[j] for j in idx]

    def crop(self, max_length):
        """HF's convention: keep the first `max_length` positions of the PADDED sequence (what get_seq_length counts); negative = drop
        the last -max_length positions.  Every row keeps max_length - pad real rows."""
        if self.kv is None:                                   # nothing cached yet (an empty DynamicCache.crop is a no-op as well)
            return
        max_length = int(max_length)
        if max_length < 0:
            max_length = self.get_seq_length() + max_length
        keep = [min(n, max(max_length - pad, 0)) for n, pad in zip(self.kv.lengths, self.pads)]
        if keep != list(self.kv.lengths):
            self.kv.set_lengths(keep)


class MetaMorphLlamaModel(MetaMorphMetaModel, nn.Module):
    """`model.*` sub-tree: embed_tokens, layers, norm, vision_tower, mm_projector, vision_proj."""
    config_class = MetaMorphConfig

    def __init__(self, config, vision_delay_load=True):
        nn.Module.__init__(self)
        self.config = config
        if getattr(config, "attention_bias", False) or getattr(config, "mlp_bias", False):
            raise NotImplementedError("attention_bias / mlp_bias are not used by LLaMA-3 and have no fused kernel")
        self.embed_tokens = HipEmbedding(config.vocab_size, config.hidden_size)
        self.layers = nn.ModuleList([_DecoderLayer(config) for _ in range(config.num_hidden_layers)])
        self.norm = HipRMSNorm(config.hidden_size, eps=config.rms_norm_eps)
        self._init_vision(config, vision_delay_load=vision_delay_load)
        self.rope = rope_params(config)         # refuses the RoPE variants without a kernel path at construction, by name
        self._rope = None
        # set by PreTrainedModel.gradient_checkpointing_enable() (HF looks for this attribute on the sub-modules): per-layer
        # recompute in DecoderLayerFn / SiglipLayerFn instead of torch.utils.checkpoint
        self.gradient_checkpointing = False
        # MI355X extension of the checkpointing mode (288 GB of HBM rarely needs every layer recomputed): None = every decoder layer
        # (the reference's behaviour), n = only the first n decoder layers keep just their input; the rest keep their activations.
        # Recompute runs the same kernels on the same inputs, so gradients carry the same bits for any n (tests/test_trainer_gpu.py).
        self.checkpoint_layers = None
        # optional fn(layer_index, rows [B*L, h]) called with every decoder layer's output (what the reference's forced
        # `output_hidden_states=True`, metamorph_llama.py:345, would collect); rows of a left-padded batch are in the moved
        # (right-padded) layout.  Used by the full-depth parity test; None costs nothing.
        self.layer_output_hook = None

    def rope_tables(self, L, device):
        """cos / sin [>= L, head_dim] bf16 of the config's RoPE variant (metamorph_amd.rope: default, llama3, linear)."""
        if self._rope is None or self._rope[0][0] < L or self._rope[0][1] != str(device):
            Lc = max(L, 256)
            rp = self.rope
            cos, sin = ops.rope_table_freq(Lc, rp.head_dim, rp.inv_freq, rp.attention_scaling, device)
            self._rope = ((Lc, str(device)), cos, sin)
        return self._rope[1], self._rope[2]


class MetaMorphLlamaForCausalLM(PreTrainedModel, GenerationMixin, MetaMorphMetaForCausalLM):
    config_class = MetaMorphConfig
    base_model_prefix = "model"
    supports_gradient_checkpointing = True      # honoured as per-layer recompute (functional.LayerMeta.recompute)
    accepts_loss_kwargs = False                 # like the reference's forward(): no `num_items_in_batch` normalisation inside the model
    _no_split_modules = ["_DecoderLayer"]
    _keys_to_ignore_on_load_unexpected = [r"model\.vision_tower\.vision_tower\.head\..*", r".*rotary_emb\.inv_freq"]
    # config.tie_word_embeddings (LLaMA-3.2 1B / 3B bases): lm_head.weight IS model.embed_tokens.weight, as in HF's LlamaForCausalLM the
    # reference subclasses (metamorph_llama.py:223); post_init() / from_pretrained tie them through this mapping.  One Parameter, one
    # gradient buffer: the fused CE's weight gradient and the splice's embedding-row sums accumulate into it (functional.grad_target).
    _tied_weights_keys = {"lm_head.weight": "model.embed_tokens.weight"}

    def __init__(self, config, use_vision_ar=True, vision_head="None", vision_coef=1.0, normalize_vision=False,
                 apply_softmax=False, vision_delay_load=True, full_ar=False):
        super().__init__(config)
        self.model = MetaMorphLlamaModel(config, vision_delay_load=vision_delay_load)
        self.pretraining_tp = getattr(config, "pretraining_tp", 1)
        self.vocab_size = config.vocab_size
        self.lm_head = HipLinear(config.hidden_size, config.vocab_size, bias=False)
        self.normalize_vision = bool(normalize_vision) or bool(getattr(config, "normalize_vision", False))
        self.apply_softmax = bool(apply_softmax)
        vision_head = getattr(config, "vision_head_type", vision_head)
        # the reference hard-codes 1152 (metamorph_llama.py:255) = the SO400M feature width; here: the tower's feature width, i.e.
        # mm_hidden_size, or a quarter of it under 'concat_interpolation' (mm_hidden_size = 4 x tower width, siglip_encoder.py:110) --
        # so that reference checkpoints load unchanged in every configuration
        hv = getattr(config, "mm_hidden_size", 1152)
        if getattr(config, "image_token_reduction", "none") == "concat_interpolation":
            hv //= 4
        h = config.hidden_size
        if vision_head == "linear":
            self.vision_head = HipLinear(h, h)
        elif vision_head == "mlp":
            self.vision_head = nn.Sequential(HipLinear(h, h), HipGELU(), HipLinear(h, hv))
        elif vision_head == "mlp2x_gelu":
            self.vision_head = nn.Sequential(HipLinear(h, h), HipGELU(), HipLinear(h, h), HipGELU(), HipLinear(h, hv))
        else:
            self.vision_head = HipLinear(h, hv)
        self._vision_head_out = h if vision_head == "linear" else hv
        self.use_vision_ar = use_vision_ar
        self.vision_coef = vision_coef
        self._loss_language_t = None
        self._loss_image_ar_t = None
        self._mm_plan = None
        self._compact_hwm = {}                      # (B, L) -> compact decoder rows in use (constant across steps: llm_forward)
        self.post_init()

    # ------------------------------------------------------------------ HF plumbing
    def _init_weights(self, module):
        std = getattr(self.config, "initializer_range", 0.02)
        if isinstance(module, HipLinear):
            nn.init.normal_(module.weight, mean=0.0, std=std)
            if module.bias is not None:
                nn.init.zeros_(module.bias)
        elif isinstance(module, HipEmbedding):
            nn.init.normal_(module.weight, mean=0.0, std=std)

    def get_model(self):
        return self.model

    def get_input_embeddings(self):
        return self.model.embed_tokens

    def set_input_embeddings(self, value):
        self.model.embed_tokens = value

    def get_output_embeddings(self):
        return self.lm_head

    def set_output_embeddings(self, value):
        self.lm_head = value

    def resize_token_embeddings(self, new_num_tokens=None, pad_to_multiple_of=None, mean_resizing=True):
        if new_num_tokens is None or new_num_tokens == self.config.vocab_size:
            return self.get_input_embeddings()
        tied = self.lm_head.weight is self.model.embed_tokens.weight
        for mod in (self.model.embed_tokens, self.lm_head):
            if tied and mod is self.lm_head:
                mod.weight = self.model.embed_tokens.weight          # stays ONE parameter
                break
            old = mod.weight.data
            new = torch.empty((new_num_tokens, old.shape[1]), device=old.device, dtype=old.dtype)
            nn.init.normal_(new, std=getattr(self.config, "initializer_range", 0.02))
            n = min(old.shape[0], new_num_tokens)
            new[:n] = old[:n]
            mod.weight = nn.Parameter(new, requires_grad=mod.weight.requires_grad)
        self.model.embed_tokens.num_embeddings = new_num_tokens
        self.lm_head.out_features = new_num_tokens
        self.config.vocab_size = self.vocab_size = new_num_tokens
        return self.get_input_embeddings()

    @property
    def loss_language(self):
        """float, like the reference's attribute (metamorph_llama.py:464); the device->host read happens here,
        when a logger asks, not inside forward."""
        return float("nan") if self._loss_language_t is None else float(self._loss_language_t)

    @property
    def loss_image_ar(self):
        return float("nan") if self._loss_image_ar_t is None else float(self._loss_image_ar_t)

    # ------------------------------------------------------------------ plan handling
    def _plan_for(self, inputs_embeds, attention_mask, labels, image_positions):
        cached = self._mm_plan
        if cached is not None and cached[0] is inputs_embeds:
            self._mm_plan = None
            return cached[1]
        # inputs_embeds supplied by the caller: derive the index arrays from the given tensors (one host copy)
        B, L, _ = inputs_embeds.shape
        msk = np.ones((B, L), dtype=bool) if attention_mask is None else host_array(attention_mask).astype(bool)
        left = getattr(self.config, "tokenizer_padding_side", "right") == "left"
        seqlens = msk.sum(1).astype(np.int32)
        if not all((msk[b, L - seqlens[b]:] if left else msk[b, : seqlens[b]]).all() for b in range(B)):
            raise NotImplementedError("attention_mask must be a contiguous padding mask on the configured tokenizer_padding_side")
        lab = host_array(labels)
        pos = np.zeros((B, L), dtype=np.int64) if image_positions is None else host_array(image_positions)
        nxt = np.zeros((B, L), dtype=bool)
        nxt[:, :-1] = pos[:, 1:] == 1
        st = ce_rows = None
        n_valid = 0
        if lab is not None:
            s = np.full((B, L), IGNORE_INDEX, dtype=np.int64)
            s[:, :-1] = lab[:, 1:]
            st = s.reshape(-1).astype(np.int32)
            ce_rows = np.flatnonzero(st != IGNORE_INDEX).astype(np.int32)
            n_valid = int(ce_rows.shape[0])
        z = np.zeros(0, dtype=np.int32)
        plan = SplicePlan(B=B, L=L, rows_per_image=0, src=z, labels=lab, attention_mask=msk, image_positions=pos,
                          position_ids=np.zeros((B, L), dtype=np.int64), seqlens=seqlens, target_keep=np.zeros(0, dtype=np.int64),
                          feat_row=z, pred_rows=np.flatnonzero(nxt.reshape(-1)).astype(np.int32), shift_targets=st,
                          ce_rows=ce_rows, n_valid=n_valid, emb_tok=z, emb_seg=np.zeros(1, dtype=np.int32), emb_pos=z,
                          images_consumed=0, padding_side="left" if left else "right")
        return upload_plan(plan, inputs_embeds.device)

    # ------------------------------------------------------------------ the hot path
    def llm_forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None,
                    inputs_embeds=None, labels=None, use_cache=None, output_attentions=None, output_hidden_states=None,
                    return_dict=None, cache_position=None, image_positions=None, decoding=False, image_features=None):
        """Reference metamorph_llama.py:285-498."""
        if past_key_values is not None or use_cache:
            # HF `generate()` (reference :711-717 -> GenerationMixin -> forward with a cache): prompt pass / one row per step on the
            # decode-shape kernels
            if labels is not None or decoding:
                raise NotImplementedError("past_key_values / use_cache together with labels or the image-AR head: the cached path is the "
                                          "generation path (no loss)")
            # images handed through prepare_inputs_for_generation arrive spliced, with image_positions / image_features: without labels the
            # reference computes no loss from them either (metamorph_llama.py:420-474 sits under `if labels is not None`), so they are dropped
            return self._cached_forward(input_ids, inputs_embeds, attention_mask, past_key_values, return_dict)
        if output_attentions:
            raise NotImplementedError("output_attentions: attention probabilities are never materialised by the flash kernel")
        if self.w8_format is not None:
            raise NotImplementedError("forward without past_key_values on a decoder quantised with quantize_decoder_: the weight-only "
                                      "quantised weights serve the cached generation path only (greedy_decode, generate() / forward with a HipKVCache)")
        return_dict = True if return_dict is None else return_dict
        cfg = self.config
        F.params_ready(None)
        if inputs_embeds is None:
            inputs_embeds = self.model.embed_tokens(input_ids)
        if inputs_embeds.dtype != BF16:
            raise TypeError(f"inputs_embeds must be bf16, got {inputs_embeds.dtype}")
        B, L, h = inputs_embeds.shape
        pd = self._plan_for(inputs_embeds, attention_mask, labels, image_positions)
        plan = pd["host"]
        dev = inputs_embeds.device
        if position_ids is not None:
            # The kernels rotate row l of a sample by l (+ the sample's left-padding offset); RoPE only sees position DIFFERENCES, so any
            # position_ids that advance by one over a sample's valid rows (what the reference builds, metamorph_arch.py:362-399, and
            # what HF's default arange is) give the same attention.  Anything else (packed sequences, gaps) is refused, not ignored.
            pid = position_ids.detach().cpu().numpy().reshape(B, L)
            for b in range(B):
                rows = np.flatnonzero(plan.attention_mask[b])
                if rows.size > 1 and not (np.diff(pid[b, rows]) == 1).all():
                    raise NotImplementedError("position_ids must advance by one over each sample's valid rows (custom positions are not supported)")
        Hq, Hkv = cfg.num_attention_heads, cfg.num_key_value_heads
        d = _head_dim(cfg)
        # Left padding (tokenizer_padding_side = "left", reference metamorph_arch.py:362-386): the attention kernels take per-sample
        # lengths counted from row 0, so the batch is moved to the right-padded row layout for the decoder and back afterwards; the
        # RoPE position of a moved row stays its ORIGINAL row index (HF: position_ids = arange(L), padding included), which the
        # kernels get as a per-sample offset.  Causal attention over the valid rows is unchanged by the move.
        shift = plan.padding_side == "left" and not plan.attention_mask.all()
        pos_off = None
        if shift:
            to_right, to_left, off = _left_pad_maps(plan.seqlens, B, L)
            moved = torch.from_numpy(np.concatenate([to_right, to_left, off])).to(dev)
            to_right_d, to_left_d, pos_off = moved[:B * L], moved[B * L:2 * B * L], moved[2 * B * L:]
        cos, sin = self.model.rope_tables(2 * L if shift else L, dev)
        # Padding-free rows (reference: batches are right-padded to their longest sample, train.py:1258-1284, and the intended attention is
        # varlen, llama_flash_attn_monkey_patch.py:95-104; tokens/s counts VALID tokens): when enough of the B x L rows are
        # padding, the decoder runs on the sum(len) valid rows only (LayerMeta.c2p / p2c) -- norms, GEMMs and SwiGLU never touch a padding
        # row; q|k|v -> attention -> o visits the padded layout through row gathers.  `mm355_compact_rows`: True / False / "auto" (default:
        # on when at least an eighth of the rows is saved; the gathers + one RoPE pass per layer cost ~2 % of a layer).
        c2p_d = p2c_d = None
        mode = getattr(cfg, "mm355_compact_rows", "auto")
        n_valid_rows = int(plan.seqlens.sum())
        if mode is not False and n_valid_rows > 0:
            # The compact row count is kept CONSTANT across steps of one (B, L) shape: a high-water mark of what the batches seen so far needed,
            # in steps of 1/16 of B x L.  Tensor sizes that change from step to step defeat the caching allocator at the occupancy a
            # training run has (222 of 288 GB at B = 16): every new maximum costs a flush of the cache, and PyTorch-ROCm has no expandable
            # segments -- measured (profiles/r6_ragged_compact_rows.log): per-batch row counts at 5 - 20 % padding ran 1.4 x SLOWER than the
            # padded layout.  With a constant count the shapes are as static as the padded path's and the saving is that of the fullest batch.
            step_rows = max(256, (B * L // 16 + 255) // 256 * 256)
            need = (n_valid_rows + step_rows - 1) // step_rows * step_rows
            hwm = self._compact_hwm.get((B, L), 0)
            rows = min(max(need, hwm), (B * L + 255) // 256 * 256)
            if mode == "exact":                                      # this batch's own count (256-row granule): sizes change from step to step
                rows = min((n_valid_rows + 255) // 256 * 256, (B * L + 255) // 256 * 256)
            if mode is True or mode == "exact" or rows <= 0.875 * B * L:   # "auto": at least an eighth of the rows saved
                if mode != "exact":
                    self._compact_hwm[(B, L)] = rows
                c2p_d, p2c_d = pd["c2p"][:rows], pd["p2c"]            # uploaded with the rest of the plan (one pinned, asynchronous copy)
        self._decoder_rows = (int(c2p_d.shape[0]) if c2p_d is not None else B * L, B * L)     # (rows the decoder ran on, padded rows): introspection
        meta = F.LayerMeta(B, L, Hq, Hkv, d, cfg.intermediate_size, cfg.rms_norm_eps, cos, sin, pd["seqlens"],
                           recompute=bool(self.model.gradient_checkpointing) and self.training, pos_offset=pos_off, c2p=c2p_d, p2c=p2c_d)

        x = inputs_embeds.reshape(B * L, h)
        if not x.is_contiguous():
            x = x.contiguous()
        if shift:
            x = F.RowsPermuteFn.apply(x, to_right_d, to_left_d)
        if c2p_d is not None:
            x = F.RowsPermuteFn.apply(x, c2p_d, p2c_d)                  # [rows_compact, h]; backward gathers with p2c (padding rows: zero)
        tap = self.model.layer_output_hook
        n_ck = self.model.checkpoint_layers
        meta_keep = meta
        if meta.recompute and n_ck is not None:
            meta_keep = copy.copy(meta)
            meta_keep.recompute = False
        for li, layer in enumerate(self.model.layers):
            x = F.decoder_layer(x, layer, meta if (n_ck is None or li < int(n_ck)) else meta_keep)
            if tap is not None:                                         # the reference's output_hidden_states tuple, one entry at a time
                tap(li, x if p2c_d is None else ops.rows_gather(x.detach(), p2c_d))
        if c2p_d is not None:
            x = F.RowsPermuteFn.apply(x, p2c_d, c2p_d)                  # back to [B * L, h] (padding rows: zeros, as the padded path leaves them
        if shift:
            x = F.RowsPermuteFn.apply(x, to_left_d, to_right_d)
        hid = self.model.norm(x)                                       # [B*L, h]
        hidden_states = hid.view(B, L, h)

        pred_z = None
        if decoding:                                                    # metamorph_llama.py:363-377
            with torch.no_grad():
                last = hidden_states[:, -1, :].contiguous()
                pred_z = self.vision_head(last)
                if self.normalize_vision:
                    pred_z = ops.bilinear_l2norm(pred_z.view(B, 1, -1).contiguous(), 1, 1, True).view(B, -1)
                if self.apply_softmax:
                    pred_z = ops.softmax_rows(pred_z.contiguous(), 0.07)
                prediction = self.model.mm_projector(pred_z)
                hidden_states = hidden_states.clone()
                hidden_states[:, -1, :] = prediction
                hid = hidden_states.view(B * L, h)

        loss = None
        logits = None
        tp = int(getattr(cfg, "pretraining_tp", 1) or 1)
        if tp > 1 and self.lm_head.weight.shape[0] % tp:
            # reference :393-396: `weight.split(vocab_size // tp)` yields tp + 1 slices when tp does not divide the vocabulary and the
            # loop over range(tp) silently drops the tail rows (for V = 128258 and tp = 4: <image_start> / <image_end>); not reproduced
            raise NotImplementedError(f"pretraining_tp={tp} does not divide the vocabulary ({self.lm_head.weight.shape[0]} rows)")
        # pretraining_tp > 1 (reference :393-396) computes the logits in `tp` vocabulary slices and concatenates them: every logit is
        # the same K-long dot product either way, and the kernels below tile the vocabulary anyway (the fused CE walks row chunks x
        # 256-column tiles), so the sliced and the unsliced form are one computation here (golden: tests/golden/r3_pretraining_tp2_*)
        if labels is None or getattr(cfg, "mm355_return_logits", False) or not torch.is_grad_enabled():
            # inference / evaluation: the full fp32 logits tensor of the reference (metamorph_llama.py:398-399)
            logits = ops.gemm(hid.detach(), self.lm_head.weight.data, out_f32=True).view(B, L, -1)
        if labels is not None:
            nan = torch.full((), float("nan"), device=dev, dtype=torch.float32)
            if plan.n_valid > 0:
                ce = F.LinearCrossEntropyFn.apply(hid, self.lm_head.weight, self.lm_head, pd, plan.n_valid)
            else:
                ce = nan                                                # mean over no targets (torch CE semantics)
            loss = ce
            if image_positions is not None:
                if image_features is not None:
                    R = int(plan.pred_rows.shape[0])
                    tgt = image_features.reshape(-1, image_features.shape[-1])
                    cosine = self.normalize_vision and not self.apply_softmax
                    Rt = tgt.shape[0]
                    if R == 0 and Rt == 0 and (cosine or self.apply_softmax):
                        l_img = nan          # mean over an empty tensor -- SURVEY A9 (understanding-only / text-only batches)
                    elif cosine and (R != Rt or tgt.shape[1] != self._vision_head_out):
                        # F.cosine_similarity raises on a row-count mismatch -- or, under 'concat_interpolation', on the width mismatch
                        # between the 1152-wide head and the 4 x 1152 targets -- and the reference's try/except (:451-455) substitutes CE
                        l_img = ce
                    elif self.apply_softmax and (R != Rt or R == 0):
                        # soft-CE: `target * log(pred)` with different row counts is a broadcasting error in the reference (:445)
                        raise RuntimeError(f"image-AR head (soft-CE): {R} prediction rows vs {Rt} target rows -- the reference raises here "
                                           f"as well (metamorph_llama.py:445)")
                    elif R == 0 or Rt == 0:
                        # mean-abs (`mse_loss_fn`, :211-219): no target rows -> division by len(z) = 0; no prediction rows -> the Python
                        # float 0.0 has no .item() (:466)
                        raise RuntimeError(f"image-AR head (mean-abs): {R} prediction rows vs {Rt} target rows -- the reference raises here "
                                           f"as well (metamorph_llama.py:211-219,466)")
                    else:
                        pred_in = F.RowsGatherFn.apply(hid, pd["pred_rows"])
                        pred = self.vision_head(pred_in).contiguous()
                        tgt = tgt.to(BF16).contiguous()
                        if self.apply_softmax:                           # soft-CE against softmax(feat / 0.07) targets (:437-447)
                            l_img = F.SoftCELossFn.apply(pred, tgt, self.normalize_vision)
                        elif self.normalize_vision:                      # -mean cos (:449-455)
                            l_img = F.CosineLossFn.apply(pred, tgt, True)
                        else:
                            # mean |t - p| (`mse_loss_fn`, :459) -- the constructor default.  The reference walks zip(target rows,
                            # prediction rows) and divides by len(target): with R != Rt it silently uses the first min(R, Rt) row pairs
                            # and still divides by Rt (:215-217)
                            n = min(R, Rt)
                            if n != R:
                                pred = pred[:n].contiguous()
                            l_img = F.MeanAbsLossFn.apply(pred, tgt[:n].contiguous() if n != Rt else tgt, Rt)
                else:
                    l_img = ce                                          # metamorph_llama.py:461-462
                self._loss_language_t = ce.detach()
                self._loss_image_ar_t = l_img.detach()
                if self.use_vision_ar:
                    # `if loss_image_ar.item() != 0` without the host sync (NaN != 0 is True, so NaN propagates)
                    loss = torch.where(l_img.detach() != 0, ce + self.vision_coef * l_img, ce)

        if not return_dict:
            out = (logits,)
            return (loss,) + out if loss is not None else out
        return CausalLMOutputWithPast(loss=pred_z if decoding else loss, logits=logits, past_key_values=None,
                                      hidden_states=hidden_states, attentions=None)

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                labels=None, use_cache=None, output_attentions=None, output_hidden_states=None, images=None,
                image_sizes=None, return_dict=None, cache_position=None, image_embeds=None):
        """Reference metamorph_llama.py:603-660 (same parameter list: no **kwargs, so HF Trainer keeps dividing the loss by the
        gradient-accumulation steps exactly as it does for the reference class)."""
        image_positions = None
        target = None
        if inputs_embeds is None and past_key_values is not None and (images is None or past_key_values.get_seq_length() > 0):
            # a decode step under HF generate(): token ids only, the prompt (with its images) already sits in the cache -- the
            # reference reaches the same early return in prepare_inputs_labels_for_multimodal (`input_ids.shape[1] == 1`, :187-193)
            pass
        elif inputs_embeds is None:
            (input_ids, position_ids, attention_mask, past_key_values, inputs_embeds, labels, image_positions,
             target) = self.prepare_inputs_labels_for_multimodal(input_ids, position_ids, attention_mask, past_key_values,
                                                                 labels, images, image_sizes, image_embeds)
        return self.llm_forward(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids,
                                past_key_values=past_key_values, inputs_embeds=inputs_embeds, labels=labels,
                                use_cache=use_cache, output_attentions=output_attentions,
                                output_hidden_states=output_hidden_states, return_dict=return_dict,
                                image_positions=image_positions, image_features=target)

    # ------------------------------------------------------------------ decoding (reference :502-597, :665-717)
    @torch.no_grad()
    def greedy_decode(self, position_ids, attention_mask, inputs_embeds, start_image_token_id=DEFAULT_IMAGE_START_ID,
                      end_image_token_id=DEFAULT_IMAGE_END_ID, eos_token_id=(128001, 128009), do_sample=None,
                      temperature=None, top_p=None, num_beams=None, max_new_tokens=1024, use_cache=None, output_image=False,
                      top_k=None, seed=None, stream_ids=None, num_return_sequences=None, repetition_penalty=None, min_new_tokens=None,
                      suppress_tokens=None, output_logprobs=False, repetition_penalty_ids=None, shared_prefix_rows=None,
                      prompt_lookup_num_tokens=None, max_matching_ngram_size=None, prompt_lookup_ids=None):
        """Token mode / continuous 'image mode' greedy loop.  use_cache=False re-runs the prefix every step exactly like
        the reference (which forces use_cache=False, O(L^2)); the default keeps a KV cache and feeds one row per step
        through the decode-shape kernels -- same state machine, same outputs.
        A batch (inputs_embeds [B, L, h], B > 1; attention_mask all-valid or LEFT-padded, padding rows are never computed or cached) runs
        the loop of every sequence at once with the token loop on the device (functional.GreedyLoopGraph): `output` is then a list of B
        int32 id tensors and the image rows a list of B [n_b, Dz] tensors.  functional.set_variant("greedy_loop_b1", True) sends one
        sequence through the same loop (return shapes as for one sequence).
        do_sample truthy AND temperature > 0 samples instead: every id is drawn from softmax(logits / temperature) after top_k (None / 0:
        off) and top_p (None / 1: off) in HF's order, by mm355_sample_rows_f32 inside the same device loop (also for one sequence; image
        rows are emitted as before).  Sequence b draws from the Philox stream (seed, stream_ids[b]) at its own output position, so a
        sequence's ids do not depend on the batch it rides in; seed=None takes 64 bits from torch's CPU generator (torch.manual_seed
        repeats a run), stream_ids defaults to range(B).  Any other do_sample / temperature (None or 0.0, the reference demo's call) is
        the greedy loop, bit for bit.
        num_return_sequences = n > 1 (one prompt, an active sampler): n continuations of the prompt, returned in the batch shapes (a list
        of n id tensors, a list of n image-row tensors); continuation b draws from the stream (seed, stream_ids[b]), stream_ids defaults
        to range(n).  The prompt runs through the decoder ONCE into sequence 0 of a cache of n sequences, and every step reads its rows
        once for all continuations (mm355_attn_decode_shared; functional.set_variant("shared_prefix_attn", False), or a head shape that
        kernel does not take: the prompt's cache rows are copied to every sequence and the step is the batch's).  Refused by name: n > 1
        without an active sampler (n greedy continuations are n copies), with more than one prompt, or with use_cache=False.  None or 1:
        as without the argument.
        Logits processors, applied on the device between the head and the pick in HF's order (mm355_logits_process_rows_f32, inside the
        captured step; any of them sends one sequence through the device loop as well): repetition_penalty (None / 1: off) divides the
        positive and multiplies the negative logits of the ids the sequence has GENERATED so far -- what HF does when it is handed
        inputs_embeds, as generate() hands them; repetition_penalty_ids (one id list, or one list per sequence; one list for all
        continuations of num_return_sequences) marks ids before the first step for callers who want HF's prompt-included behaviour, and
        generate() does not pass it.  min_new_tokens (None / 0: off) keeps the eos ids at -inf while the sequence's count of outputs is
        below it; the count is the loop's total_out, so image rows count as outputs.  suppress_tokens (None / empty: off) keeps its ids
        at -inf throughout (128256, <im_start>, asks for a text-only answer).  output_logprobs=True also returns, aligned with the ids,
        the fp32 log-probability of every emitted id under the PROCESSED logits -- after the three processors, before temperature, top-k
        and top-p; with no processor active the model's own log-softmax (mm355_token_note_rows_f32): (ids, logprobs), or (ids, image rows,
        logprobs) with output_image=True, `logprobs` a list of fp32 tensors in the batch shapes, also for one sequence.  All of it works
        with batches, left padding, the sampler and num_return_sequences.  Refused by name before any device work: a penalty that is not
        finite or <= 0; min_new_tokens negative, non-integer or above max_new_tokens; an id outside [0, vocabulary) in suppress_tokens or
        repetition_penalty_ids (strip the -200 image sentinel first); repetition_penalty_ids without an active penalty or with the
        wrong number of lists; any of the options with use_cache=False (NotImplementedError).
        shared_prefix_rows = S (a batch of B > 1 prompts that begin alike: one image asked B questions, a system prompt in front of B
        items): an int S promises that, once left padding is stripped, rows [0, S) of every sequence are the same rows; "auto" takes the
        longest common prefix of the stripped rows, capped so that every sequence keeps one own row, and is the ordinary batch below
        functional.VARIANTS["shared_prefix_min_rows"] rows.  The promise is checked on the device before any decoder work (one comparison,
        one synchronisation); a break raises ValueError naming the first sequence and row that differ.  The S rows then run through the
        decoder ONCE into sequence 0 of the cache, the B sequences' own rows -- right-padded with zero rows to the longest -- in ONE more
        pass over the weights (functional.decoder_extend_shared, mm355_attn_extend_shared), and every step of the device loop reads the
        prefix once for all sequences (mm355_attn_decode_shared).  functional.set_variant("shared_prefix_attn", False), or a head shape
        the kernels do not take: the prefix still runs once, its cache rows are copied to every sequence, the own rows go through
        decoder_extend one sequence after the other and the step is the batch's.  The sampler, the logits processors, log-probabilities,
        quantised weights and the fp8 cache work as without it.  One prompt: the argument is validated and the call is the one without
        it.  Refused by name before any device work: use_cache=False, num_return_sequences > 1, an S that is negative, no integer and not
        "auto", or above min L_b - 1 (every sequence keeps at least one own row).  None (the default): as without the argument.
        prompt_lookup_num_tokens = K (an integer in [1, MM355_SPEC_MAX_DRAFT = 15]; None / 0: as without the argument): prompt-lookup
        speculative decoding, HF's option of that name, in the device loop (functional.SpecGreedyLoopGraph).  Every step carries a
        sequence's next input and up to K ids guessed from its own text through the decoder in one pass over the weights and emits up
        to K + 1 ids; the guesses are the continuation of the earliest earlier occurrence of the sequence's last max_matching_ngram_size
        = N ids (1 .. 8; None: 2, HF's default), shorter n-grams tried after longer ones (mm355_ngram_draft_rows: HF's
        PromptLookupCandidateGenerator).  prompt_lookup_ids is the text looked up in, with what the sequence emits appended: one id list,
        one list per sequence, or a [B, n] integer tensor read with the attention mask (left-padding entries dropped); it may be empty,
        and ids outside the vocabulary (the -200 image sentinel) stay in: they match nothing emitted and end a draft.  greedy_decode
        receives embeddings, hence the ids as an argument of their own; generate() passes its `inputs`.  Every emitted id is the argmax
        of a row computed on the correct prefix: the ids and image rows are those of the loop without the argument wherever its decision
        is no near tie (another row count takes another GEMV / GEMM route through the same weights).  The return shapes are the device
        loop's; one sequence goes through the device loop too.  Works with batches, left padding, the fp8 KV cache and quantised
        weights.  Refused by name before any device work: K or N out of range or no integer, prompt_lookup_ids with the wrong number of
        lists, K together with an active sampler, num_return_sequences > 1, a logits processor or output_logprobs, shared_prefix_rows,
        use_cache=False or num_beams > 1, and a head shape the row kernels do not take (functional.verify_rows_supported)."""
        cached = use_cache is None or use_cache
        spec = self._prompt_lookup_arg(prompt_lookup_num_tokens, max_matching_ngram_size)
        if spec is not None:
            B0 = inputs_embeds.shape[0]
            lookup = self._prompt_lookup_ids(prompt_lookup_ids, attention_mask, B0)
            copies = self._copies_of(num_return_sequences)
            clash = [what for what, on in (
                ("an active sampler (do_sample=True and temperature > 0): a draft is verified against the argmax, not against a draw",
                 bool(do_sample) and temperature is not None and float(temperature) > 0),
                (f"num_return_sequences={copies}: greedy continuations of one prompt are all the same sequence", copies > 1),
                ("repetition_penalty / min_new_tokens / suppress_tokens / output_logprobs: the processors see one row per sequence and step",
                 self._processors_of(repetition_penalty, min_new_tokens, suppress_tokens, output_logprobs, repetition_penalty_ids,
                                     max_new_tokens, self._vocab_rows, B0) is not None),
                (f"shared_prefix_rows={shared_prefix_rows!r}: the speculative step attends every sequence's own rows only",
                 shared_prefix_rows is not None),
                ("use_cache=False: the drafts are verified against the KV cache (use_cache=True)", not cached),
                (f"num_beams={num_beams}: beam search is not part of the speculative loop", num_beams not in (None, 1)),
            ) if on]
            if clash:
                raise ValueError(f"greedy_decode(prompt_lookup_num_tokens={spec[0]}) does not go with {clash[0]}")
            _, m0 = self._decode_meta(1)
            if not F.verify_rows_supported(m0):
                raise ValueError(f"greedy_decode(prompt_lookup_num_tokens={spec[0]}): no kernel for Hq={m0.Hq} Hkv={m0.Hkv} d={m0.d} "
                                 "(ops.attn_extend_supported with d % 16 == 0)")
            return self._greedy_decode_loop(inputs_embeds, attention_mask, start_image_token_id, end_image_token_id, eos_token_id,
                                            max_new_tokens, output_image, spec=(*spec, lookup))
        copies = self._copies_of(num_return_sequences)
        shared_rows = None
        if shared_prefix_rows is not None:
            want = self._shared_prefix_arg(shared_prefix_rows)
            if not cached:
                raise ValueError(f"greedy_decode(shared_prefix_rows={shared_prefix_rows!r}, use_cache=False): the sequences share the prefix's "
                                 "KV cache rows (use_cache=True)")
            if copies > 1:
                raise ValueError(f"greedy_decode(shared_prefix_rows={shared_prefix_rows!r}, num_return_sequences={copies}): continuations of "
                                 "several prompts over one prefix are not built; repeat the prompts instead")
            B0, n0 = inputs_embeds.shape[:2]
            shared_rows = self._shared_prefix_of(want, inputs_embeds, self._left_pads(attention_mask, B0, n0))
        processors = self._processors_of(repetition_penalty, min_new_tokens, suppress_tokens, output_logprobs, repetition_penalty_ids,
                                         max_new_tokens, self._vocab_rows, inputs_embeds.shape[0])
        if processors is not None and not cached:
            raise NotImplementedError("greedy_decode(repetition_penalty / min_new_tokens / suppress_tokens / output_logprobs, use_cache=False): "
                                      "the logits processors run in the device loop on the KV cache (use_cache=True)")
        if copies > 1:
            if not cached:
                raise ValueError(f"greedy_decode(num_return_sequences={copies}, use_cache=False): the continuations share the prompt's KV "
                                 "cache rows (use_cache=True)")
            if inputs_embeds.shape[0] != 1:
                raise ValueError(f"greedy_decode(num_return_sequences={copies}) takes one prompt, got {inputs_embeds.shape[0]}")
            sampler = self._sampler_of(do_sample, temperature, top_k, top_p, num_beams, seed, stream_ids, copies)
            if sampler is None:
                raise ValueError(f"greedy_decode(num_return_sequences={copies}) needs an active sampler (do_sample=True and temperature > "
                                 "0): greedy continuations of one prompt are all the same sequence")
            return self._greedy_decode_loop(inputs_embeds, attention_mask, start_image_token_id, end_image_token_id, eos_token_id,
                                            max_new_tokens, output_image, sampler=sampler, copies=copies, processors=processors)
        sampler = self._sampler_of(do_sample, temperature, top_k, top_p, num_beams, seed, stream_ids, inputs_embeds.shape[0])
        if sampler is not None and not cached:
            raise NotImplementedError("greedy_decode(do_sample=True, use_cache=False): sampling runs in the device loop on the KV cache "
                                      "(use_cache=True)")
        if cached:
            if inputs_embeds.shape[0] != 1 or F.VARIANTS["greedy_loop_b1"] or sampler is not None or processors is not None:
                return self._greedy_decode_loop(inputs_embeds, attention_mask, start_image_token_id, end_image_token_id, eos_token_id,
                                                max_new_tokens, output_image, sampler=sampler, processors=processors, shared_rows=shared_rows)
            return self._greedy_decode_cached(inputs_embeds, start_image_token_id, end_image_token_id, eos_token_id,
                                              max_new_tokens, output_image)
        if inputs_embeds.shape[0] != 1:
            raise NotImplementedError(f"greedy_decode(use_cache=False) handles one sequence (as the reference's loop does), got "
                                      f"{inputs_embeds.shape[0]}; a batch runs on the KV cache (use_cache=True)")
        dev = inputs_embeds.device

        def head(in_image):                                   # the whole prefix again, as the reference runs it
            out = self.llm_forward(inputs_embeds=inputs_embeds, attention_mask=None, return_dict=True, decoding=in_image)
            return int(torch.argmax(out.logits[:, -1, :], dim=-1)[0]), out.hidden_states[:, -1, :].unsqueeze(0), out.loss

        def feed(tok, row):
            nonlocal inputs_embeds
            if row is None:
                row = self.model.embed_tokens(torch.tensor([[tok]], device=dev))
            inputs_embeds = torch.cat((inputs_embeds, row), dim=1)
        return self._one_sequence(F.greedy_host_loop(head, feed, start_image_token_id, end_image_token_id,
                                                     self.get_model().vision_tower.image_token_len, max_new_tokens, eos_token_id),
                                  dev, output_image)

    # ------------------------------------------------------------------ weight-only FP8 decode (reference builder.py:13-25, load_8bit=True)
    w8_format = None                                         # set by quantize_decoder_
    w8_lm_head = None                                        # (bytes, scales) of a quantised lm_head
    w8_released = False

    @torch.no_grad()
    def quantize_decoder_(self, fmt="fp8_e4m3", lm_head=False, pow2_scales=False, keep_bf16=False):
        """Quantise the fused projections of every decoder layer (q|k|v, o, gate|up, down; on request the lm_head) to weight-only FP8:
        e4m3 bytes + one fp32 scale per output row (ops.quantize_w8).  Decode steps of up to 16 sequences then stream half the bytes
        (mm355_gemv*_w8); larger batches and the prompt pass of one sequence stream the same bytes through the w8 split-K GEMM
        (mm355_gemm_w8*, functional.w8_route) for every projection that the split-K GEMM splits at that row count -- at 8B widths a
        prompt of up to 960 rows (its gate|up up to functional.PROMPT_GU_SPLITK_ROWS), a decode step of up to 192 sequences.  What is left dequantises one projection at a time into a
        shared scratch buffer and runs the bf16 GEMMs (functional.W8Scratch: correct, not fast): projections at row counts where they are not
        split (a one-sequence prompt of more than 960 rows at 8B widths runs wholly there), the prompt pass's gate|up above
        functional.PROMPT_GU_SPLITK_ROWS rows, the batched prompt pass of all sequences at once, passes of more than 4096 rows.  The bf16
        storage of the quantised projections is released unless keep_bf16;
        embed_tokens, norms, vision tower, projector and vision head stay bf16.  The model ends in eval mode: generation only.
        fmt="mxfp4" (the counterpart of the reference's load_4bit=True): OCP MXFP4, e2m1 nibbles + one e8m0 scale per 32 consecutive k
        (ops.quantize_w4), 4.25 bits per weight and coarser than FP8 (relative RMS weight error 0.114 against 0.026 on Gaussian weights;
        on a trained checkpoint: not measured) -- opt-in.  Decode steps of up to 16 sequences run on mm355_gemv*_w4; there is no w4
        split-K GEMM yet, so every other route (more sequences, prompt passes, decoder_extend) takes the scratch route.  Hidden and
        intermediate size must be multiples of 32; lm_head=True is refused (the head is the accuracy-critical matrix and beyond 16 rows
        it would need a temporary of its bf16 size); pow2_scales has no effect (the group scales are powers of two by format)."""
        if fmt not in ops.QUANT_FORMATS:
            raise ValueError(f"quantize_decoder_: unknown format {fmt!r} (supported: {sorted(ops.QUANT_FORMATS)})")
        if self.w8_format is not None:
            raise RuntimeError(f"quantize_decoder_: the decoder is already quantised ({self.w8_format}); a second call would quantise "
                               "quantised weights")
        if lm_head and (getattr(self.config, "tie_word_embeddings", False)
                        or self.lm_head.weight.data_ptr() == self.model.embed_tokens.weight.data_ptr()):
            raise ValueError("quantize_decoder_(lm_head=True) with tied embeddings: lm_head shares its storage with embed_tokens, which "
                             "stays bf16; pass lm_head=False")
        w4 = fmt in ops.W4_FORMATS
        if w4 and lm_head:
            raise ValueError('quantize_decoder_(fmt="mxfp4", lm_head=True): a 4-bit lm_head is not supported (the head is the '
                             "accuracy-critical matrix); pass lm_head=False")
        if w4 and (self.config.hidden_size % 32 or self.config.intermediate_size % 32):
            raise ValueError(f'quantize_decoder_(fmt="mxfp4"): hidden size {self.config.hidden_size} and intermediate size '
                             f"{self.config.intermediate_size} must be multiples of 32 (one scale per 32 consecutive k)")
        scratch = F.W8Scratch()
        for layer in self.model.layers:
            layer.w8 = (F.W4Layer if w4 else F.W8Layer)(layer, scratch, pow2_scales=pow2_scales, keep_bf16=keep_bf16)
        if lm_head:
            w = self.lm_head.weight
            self.w8_lm_head = ops.quantize_w8(w.data, pow2_scales)
            w.w8_quantized = True
            if not keep_bf16:
                w.data = w.data.new_empty((0, w.shape[1]))
                w.requires_grad_(False)
        self.w8_format = fmt
        self.w8_released = not keep_bf16
        self.eval()
        return self

    def state_dict(self, *args, **kwargs):
        if self.w8_format is not None and self.w8_released:
            raise RuntimeError("state_dict of a decoder quantised with quantize_decoder_: the bf16 weights of the quantised projections "
                               "were released (save before quantising, or pass keep_bf16=True)")
        return super().state_dict(*args, **kwargs)

    # ------------------------------------------------------------------ the heads of cached generation
    @property
    def _vocab_rows(self):
        """the width of the logits: the rows of the lm_head, quantised or not"""
        return self.w8_lm_head[0].shape[0] if self.w8_lm_head is not None else self.lm_head.weight.shape[0]

    def _lm_head(self, hid, out=None):
        """fp32 logits of the normed rows `hid` [n, h], into `out` [n, V] if given: the lm_head dispatch of cached generation.  A quantised
        lm_head: up to 16 rows mm355_gemv_w8, more rows mm355_gemm_w8 (one slice, fp32 output); with VARIANTS["w8_gemm"] off or beyond its
        limits (more than 4096 rows, a hidden size that is no multiple of 64) the bf16 GEMM on the dequantised weight, a temporary of the
        lm_head's size.  A bf16 lm_head: up to 32 rows mm355_gemv_bf16 where it takes them (17 .. 32 rows: wide weights only -- the lm_head
        is one), else the GEMM."""
        n = hid.shape[0]
        if out is None:
            out = torch.empty((n, self._vocab_rows), device=hid.device, dtype=torch.float32)
        if self.w8_lm_head is not None:
            q, scale = self.w8_lm_head
            if n <= 16:
                return ops.gemv_w8(hid, q, scale, out=out)
            if F.VARIANTS["w8_gemm"] and ops.gemm_w8_supported(n, hid.shape[1]):
                return ops.gemm_w8(hid, q, scale, out=out)
            return ops.gemm(hid, ops.dequant_w8(q, scale), out=out)
        w = self.lm_head.weight.data
        if n <= 32 and ops.gemv_supported(hid, w):
            return ops.gemv(hid, w, out=out)
        return ops.gemm(hid, w, out=out)

    def _image_head(self, hid):
        """The image head on the normed rows `hid` [n, h] (reference metamorph_llama.py:363-377): vision_head -> L2 normalisation if
        normalize_vision -> softmax(. / 0.07) if apply_softmax -> mm_projector.  Returns (pred_z [n, Dz], the projected rows [n, h])."""
        n = hid.shape[0]
        pred_z = self.vision_head(hid)
        if self.normalize_vision:
            pred_z = ops.bilinear_l2norm(pred_z.view(n, 1, -1).contiguous(), 1, 1, True).view(n, -1)
        if self.apply_softmax:
            pred_z = ops.softmax_rows(pred_z.contiguous(), 0.07)
        return pred_z, self.model.mm_projector(pred_z)

    # ------------------------------------------------------------------ cached decode (row N1)
    def _decode_meta(self, L):
        cfg = self.config
        h, Hq, Hkv = cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads
        return h, F.LayerMeta(1, L, Hq, Hkv, _head_dim(cfg), cfg.intermediate_size, cfg.rms_norm_eps, None, None, None)

    @torch.no_grad()
    def _head_row(self, x, in_image_mode):
        """Final norm + (image mode: _image_head) + fp32 logits of ONE hidden row (reference metamorph_llama.py:363-377, 398-399).
        Returns (logits [1,V] f32, row fed back in image mode, pred_z)."""
        hid = self.model.norm(x)
        pred_z = None
        if in_image_mode:
            pred_z, hid = self._image_head(hid)
        return self._lm_head(hid.contiguous()), hid, pred_z

    @torch.no_grad()
    def _kv_cache_format(self, fmt=None):
        """The KV cache format of cached generation: `fmt` if given, else config.mm355_kv_cache_format ("bf16", the default, or
        "fp8_e4m3": e4m3 bytes plus one fp32 scale per head-row, functional.KVCache)."""
        fmt = getattr(self.config, "mm355_kv_cache_format", "bf16") if fmt is None else fmt
        if fmt not in ops.KV_FORMATS:
            raise ValueError(f"unknown KV cache format {fmt!r}; known: {', '.join(ops.KV_FORMATS)}")
        return fmt

    def _prefill_chunk_rows(self, cache=None):
        """Rows per slice of a chunked prompt pass: the cache's own `prefill_chunk` if it has one, else config.mm355_prefill_chunk_rows
        (None, the default: the prompt in one pass)."""
        n = getattr(cache, "prefill_chunk", None)
        if n is None:
            n = getattr(self.config, "mm355_prefill_chunk_rows", None)
            if n is not None and int(n) < 1:
                raise ValueError(f"config.mm355_prefill_chunk_rows = {n}: a prompt is run in slices of at least 1 row (None: in one pass)")
        return None if n is None else int(n)

    def _ragged_pass(self, meta):
        """Whether a ragged batch of prompts, and a follow-up turn of B > 1 sequences, runs as one packed pass
        (functional.decoder_extend_ragged): config.mm355_ragged_pass (a bool; absent: False), and then functional.VARIANTS["ragged_pass_attn"]
        and a head shape the pass takes."""
        on = getattr(self.config, "mm355_ragged_pass", False)
        if not isinstance(on, bool):
            raise ValueError(f"config.mm355_ragged_pass = {on!r}: True or False (absent: False)")
        return on and F.VARIANTS["ragged_pass_attn"] and F.ragged_pass_supported(meta)

    def _greedy_decode_cached(self, inputs_embeds, start_image_token_id, end_image_token_id, eos_token_id, max_new_tokens,
                              output_image):
        assert inputs_embeds.shape[0] == 1                     # (a batch takes _greedy_decode_loop)
        if inputs_embeds.dtype != BF16:
            raise TypeError(f"inputs_embeds must be bf16, got {inputs_embeds.dtype}")
        dev = inputs_embeds.device
        F.params_ready(None)
        L0 = inputs_embeds.shape[1]
        num_image_tokens = self.get_model().vision_tower.image_token_len
        h, meta = self._decode_meta(L0)
        max_len = L0 + max_new_tokens + 2
        cos, sin = self.model.rope_tables(max_len, dev)
        meta.cos, meta.sin = cos, sin
        cache = F.KVCache(len(self.model.layers), max_len, meta.Hkv * meta.d, dev, Hq=meta.Hq, d=meta.d, fmt=self._kv_cache_format())
        x = F.decoder_prefill_chunked(inputs_embeds.reshape(L0, h).contiguous(), self.model.layers, meta, cache,
                                      self._prefill_chunk_rows())[-1:].contiguous()
        stepper = F.DecodeStepGraph(self.model.layers, meta, cache, cos, sin, h, dev)

        def head(in_image):
            logits, fed_back, pred_z = self._head_row(x, in_image)
            return int(torch.argmax(logits[0], dim=-1)), fed_back, pred_z

        def feed(tok, row):
            nonlocal x
            if row is None:
                row = self.model.embed_tokens(torch.tensor([[tok]], device=dev)).view(1, h)
            x = stepper.step(row)
        return self._one_sequence(F.greedy_host_loop(head, feed, start_image_token_id, end_image_token_id, num_image_tokens, max_new_tokens,
                                                     eos_token_id), dev, output_image)

    @staticmethod
    def _one_sequence(logged, dev, output_image):
        """functional.greedy_host_loop's (ids, pred_z rows) in greedy_decode's return shapes for one sequence"""
        ids, z_rows = logged
        emb = torch.cat(z_rows, dim=0) if z_rows else torch.tensor([], dtype=torch.float32, device=dev)
        output = [torch.tensor(ids, dtype=torch.int32, device=dev)]
        return (output, emb) if output_image else output

    # ------------------------------------------------------------------ the greedy loop of a batch, token loop on the device
    def _head_rows_device(self, x, in_image, logits_out):
        """_head_row for every sequence with the mode on the device: final norm, _image_head for ALL rows, mm355_rows_select_bf16 by
        `in_image` (int32 [B]), fp32 logits into `logits_out`.  The launch sequence does not depend on the modes.  Returns (the rows the
        lm_head saw, pred_z)."""
        hid = self.model.norm(x).contiguous()
        pred_z, projected = self._image_head(hid)
        fed = ops.rows_select(in_image, projected.contiguous(), hid)
        self._lm_head(fed, logits_out)
        return fed, pred_z.contiguous()

    @staticmethod
    def _left_pads(attention_mask, B, n):
        """Padding rows in front of every sequence of a [B, n] prompt batch (None / all-valid: none); right padding is refused."""
        pads = [0] * B
        if attention_mask is not None and not bool(attention_mask.to(torch.bool).all()):
            m = attention_mask.to(torch.bool).cpu()
            if tuple(m.shape) != (B, n):
                raise ValueError(f"attention_mask {tuple(m.shape)} does not match the prompt batch {(B, n)}")
            for b in range(B):
                nb = int(m[b].sum())
                if nb == 0 or not bool(m[b, n - nb:].all()):
                    raise NotImplementedError("cached decoding takes LEFT-padded prompts (valid rows at the end); right padding puts pad rows "
                                              "between the prompt and the generated tokens in the reference as well")
                pads[b] = n - nb
        return pads

    @staticmethod
    def _copies_of(num_return_sequences):
        """greedy_decode's num_return_sequences -> the number of continuations per prompt (None: 1); anything but a positive integer is
        refused by name."""
        if num_return_sequences is None:
            return 1
        try:
            if isinstance(num_return_sequences, bool):
                raise TypeError
            n = operator.index(num_return_sequences)
        except TypeError:
            n = 0
        if n < 1:
            raise ValueError(f"greedy_decode: num_return_sequences = {num_return_sequences!r} must be a positive integer")
        return n

    @staticmethod
    def _prompt_lookup_arg(prompt_lookup_num_tokens, max_matching_ngram_size):
        """greedy_decode's prompt_lookup_num_tokens / max_matching_ngram_size -> (K, N), or None for the call without them (K None or 0);
        anything but integers in [1, MM355_SPEC_MAX_DRAFT] and [1, functional.SPEC_MAX_NGRAM] (N None: 2) is refused by name."""
        def integer(v):
            if isinstance(v, (bool, str)):
                raise TypeError
            return operator.index(v)
        try:
            K = 0 if prompt_lookup_num_tokens is None else integer(prompt_lookup_num_tokens)
        except TypeError:
            K = -1
        if not 0 <= K <= MM355_SPEC_MAX_DRAFT:
            raise ValueError(f"greedy_decode: prompt_lookup_num_tokens = {prompt_lookup_num_tokens!r} must be an integer in [1, "
                             f"{MM355_SPEC_MAX_DRAFT}] (None or 0: off): a step carries the next input and that many guessed tokens")
        try:
            N = 2 if max_matching_ngram_size is None else integer(max_matching_ngram_size)
        except TypeError:
            N = -1
        if not 1 <= N <= F.SPEC_MAX_NGRAM:
            raise ValueError(f"greedy_decode: max_matching_ngram_size = {max_matching_ngram_size!r} must be an integer in [1, "
                             f"{F.SPEC_MAX_NGRAM}] (None: 2)")
        return (K, N) if K else None

    @staticmethod
    def _prompt_lookup_ids(prompt_lookup_ids, attention_mask, B):
        """greedy_decode's prompt_lookup_ids -> one list of ints per sequence: None is B empty lists, one flat list serves every sequence,
        a [B, n] integer tensor is read with the attention mask (entries under a 0 are dropped); anything else is refused by name."""
        ids = prompt_lookup_ids
        if ids is None:
            return [[] for _ in range(B)]
        if torch.is_tensor(ids):
            if ids.dim() != 2 or ids.shape[0] != B or ids.is_floating_point():
                raise ValueError(f"greedy_decode: prompt_lookup_ids {tuple(ids.shape)} {ids.dtype} must be a [{B}, n] integer tensor")
            keep = torch.ones_like(ids, dtype=torch.bool) if attention_mask is None else attention_mask.to(torch.bool)
            if tuple(keep.shape) != tuple(ids.shape):
                raise ValueError(f"greedy_decode: prompt_lookup_ids {tuple(ids.shape)} does not match the attention mask {tuple(keep.shape)}")
            ids = [[t for t, k in zip(row, m) if k] for row, m in zip(ids.cpu().tolist(), keep.cpu().tolist())]
        try:
            lists = list(ids)
            if not (lists and isinstance(lists[0], (list, tuple))):
                lists = [lists] * B
            lists = [[operator.index(t) for t in row] for row in lists]
        except TypeError:
            raise ValueError("greedy_decode: prompt_lookup_ids must be a list of integer ids, one such list per sequence or a [B, n] "
                             "integer tensor") from None
        if len(lists) != B:
            raise ValueError(f"greedy_decode: prompt_lookup_ids holds {len(lists)} lists for {B} sequences (one list for all, or one per "
                             "sequence)")
        if any(not -2**31 <= t < 2**31 for row in lists for t in row):
            raise ValueError("greedy_decode: prompt_lookup_ids holds ids that are no int32")
        return lists

    @staticmethod
    def _shared_prefix_arg(shared_prefix_rows):
        """greedy_decode's shared_prefix_rows -> "auto" or a non-negative int; anything else is refused by name."""
        if isinstance(shared_prefix_rows, str) and shared_prefix_rows == "auto":
            return "auto"
        try:
            if isinstance(shared_prefix_rows, (bool, str)):
                raise TypeError
            S = operator.index(shared_prefix_rows)
        except TypeError:
            S = -1
        if S < 0:
            raise ValueError(f"greedy_decode: shared_prefix_rows = {shared_prefix_rows!r} must be a non-negative integer or \"auto\"")
        return S

    @staticmethod
    def _first_differing_rows(inputs_embeds, pads, rows):
        """For every sequence of a left-padded [B, n, h] batch the first of its stripped rows [0, rows) that is not sequence 0's row, `rows`
        where there is none: one comparison where the batch lives and one copy to the host.  rows <= min(n - pads[b])."""
        B, n, h = inputs_embeds.shape
        if rows <= 0 or B == 1:
            return [max(rows, 0)] * B
        if len(set(pads)) == 1:                                  # (no ragged padding: a view)
            x = inputs_embeds[:, pads[0]:pads[0] + rows]
        else:
            idx = torch.tensor(pads, dtype=torch.int64).view(B, 1) + torch.arange(rows, dtype=torch.int64).view(1, rows)
            x = inputs_embeds.gather(1, idx.to(inputs_embeds.device).view(B, rows, 1).expand(B, rows, h))  # the stripped rows [B, rows, h]
        differs = (x != x[:1]).any(-1)                                                                         # [B, rows]
        first = torch.where(differs.any(1), differs.to(torch.int32).argmax(1), rows)
        return [int(i) for i in first.cpu()]

    @classmethod
    def _shared_prefix_of(cls, want, inputs_embeds, pads):
        """The rows the batch's shared-prefix route shares: `want` is _shared_prefix_arg's value, pads the left padding of every sequence.
        None: the ordinary batch (one prompt, nothing shared, or "auto" below functional.VARIANTS["shared_prefix_min_rows"]).  An int
        above min L_b - 1, or one whose promise does not hold, is refused by name."""
        B, n, _ = inputs_embeds.shape
        cap = n - max(pads) - 1                                 # every sequence keeps at least one own row
        if want == "auto":
            if B == 1:
                return None
            S = min(cls._first_differing_rows(inputs_embeds, pads, cap))
            return S if S >= max(1, int(F.VARIANTS["shared_prefix_min_rows"])) else None
        if want > cap:
            raise ValueError(f"greedy_decode: shared_prefix_rows = {want} leaves a sequence of {cap + 1} rows no row of its own (at most "
                             f"{cap}: the shortest sequence minus one)")
        if B == 1 or want == 0:
            return None
        first = cls._first_differing_rows(inputs_embeds, pads, want)
        bad = [b for b in range(B) if first[b] < want]
        if bad:
            raise ValueError(f"greedy_decode: shared_prefix_rows = {want}, but sequence {bad[0]} differs from sequence 0 at row {first[bad[0]]} "
                             "(rows counted after left padding is stripped)")
        return want

    @staticmethod
    def _sampler_of(do_sample, temperature, top_k, top_p, num_beams, seed, stream_ids, B):
        """greedy_decode's sampling arguments -> GreedyLoopGraph's `sampler` tuple, or None for the greedy loop (do_sample falsy, or
        temperature None / 0).  Refuses bad values by name before any device work."""
        if not do_sample or temperature is None:
            return None
        temperature = float(temperature)
        if not math.isfinite(temperature) or temperature < 0:
            raise ValueError(f"greedy_decode: temperature = {temperature} must be finite and >= 0 (0: greedy)")
        if temperature == 0:
            return None
        top_k = 0 if top_k is None else top_k
        if isinstance(top_k, float) and not top_k.is_integer():
            raise ValueError(f"greedy_decode: top_k = {top_k} must be an integer >= 0 (0: off)")
        if int(top_k) < 0 or int(top_k) > 2**31 - 1:
            raise ValueError(f"greedy_decode: top_k = {top_k} must be an integer >= 0 (0: off)")
        top_p = 1.0 if top_p is None else float(top_p)
        if not (0.0 < top_p <= 1.0):                             # (a NaN fails both comparisons)
            raise ValueError(f"greedy_decode: top_p = {top_p} must lie in (0, 1] (1: off)")
        if num_beams not in (None, 1):
            raise ValueError(f"greedy_decode: num_beams = {num_beams} with do_sample=True: the device loop samples one continuation per "
                             "sequence, beam search is not part of it (repeat the prompt and give each copy its own stream id)")
        inv_t = 1.0 / temperature
        if not math.isfinite(inv_t):
            raise ValueError(f"greedy_decode: temperature = {temperature} is too small to divide by (0: greedy)")
        if seed is None:
            seed = int(torch.randint(-2**63, 2**63 - 1, (1,), dtype=torch.int64).item())
        stream_ids = list(range(B)) if stream_ids is None else [int(i) for i in stream_ids]
        if len(stream_ids) != B or any(i < 0 or i > 2**31 - 1 for i in stream_ids):
            raise ValueError(f"greedy_decode: stream_ids = {stream_ids}: one id in [0, 2^31) per sequence ({B})")
        return (inv_t, int(top_k), top_p, int(seed) & 0xFFFFFFFFFFFFFFFF, stream_ids)

    @staticmethod
    def _processors_of(repetition_penalty, min_new_tokens, suppress_tokens, output_logprobs, repetition_penalty_ids, max_new_tokens, V, B):
        """greedy_decode's logits-processor arguments -> a dict of plain values for functional.LogitsProcessors (the suppressed ids still a
        host list), or None when every option is off.  Refuses bad values by name before any device work.  V: the width of the logits;
        B: the number of prompts."""
        def ids_of(name, ids):
            try:
                out = [operator.index(i) for i in ids]
            except TypeError:
                raise ValueError(f"greedy_decode: {name} = {ids!r} must be a list of integer ids") from None
            bad = [i for i in out if not 0 <= i < V]
            if bad:
                raise ValueError(f"greedy_decode: {name} holds ids outside [0, {V}): {bad[:4]} (strip sentinels such as the image index first)")
            return out
        penalty = 1.0 if repetition_penalty is None else float(repetition_penalty)
        if not (math.isfinite(penalty) and penalty > 0):
            raise ValueError(f"greedy_decode: repetition_penalty = {repetition_penalty} must be finite and > 0 (1: off)")
        min_new = 0 if min_new_tokens is None else min_new_tokens
        try:
            if isinstance(min_new, bool):
                raise TypeError
            min_new = int(min_new) if isinstance(min_new, float) and min_new.is_integer() else operator.index(min_new)
        except TypeError:
            min_new = -1
        if min_new < 0 or min_new > int(max_new_tokens):
            raise ValueError(f"greedy_decode: min_new_tokens = {min_new_tokens!r} must be an integer in [0, max_new_tokens = {max_new_tokens}] "
                             "(0: off)")
        suppress = [] if suppress_tokens is None else ids_of("suppress_tokens", suppress_tokens)
        marks = None
        if repetition_penalty_ids is not None:
            if penalty == 1.0:
                raise ValueError("greedy_decode: repetition_penalty_ids without an active repetition_penalty: nothing would read the marks")
            lists = list(repetition_penalty_ids)
            if lists and isinstance(lists[0], (list, tuple, torch.Tensor)):
                if len(lists) != B:
                    raise ValueError(f"greedy_decode: repetition_penalty_ids holds {len(lists)} lists for {B} sequences (one list for all, "
                                     "or one per sequence)")
                marks = [ids_of("repetition_penalty_ids", [int(i) for i in l]) for l in lists]
            else:
                marks = [ids_of("repetition_penalty_ids", lists)] * B
        if penalty == 1.0 and min_new == 0 and not suppress and not output_logprobs:
            return None
        return dict(repetition_penalty=penalty, min_new_tokens=min_new, suppress=sorted(set(suppress)), want_logprobs=bool(output_logprobs),
                    marks=marks)

    def _greedy_decode_loop(self, inputs_embeds, attention_mask, start_image_token_id, end_image_token_id, eos_token_id, max_new_tokens,
                            output_image, sampler=None, copies=1, processors=None, shared_rows=None, spec=None):
        """greedy_decode of B sequences: the prompt pass of _prefill_batch (same-length prompts as one batch, ragged ones one after the
        other), then functional.GreedyLoopGraph -- one pass over the weights per step for all sequences, head, argmax and the reference's
        mode state machine on the device.  The host reads the live counter every config.mm355_greedy_poll_steps steps (default 8: at most
        7 wasted steps per call against one synchronisation per 8 tokens; a judgement, tools/bench_greedy_batch.py gives the numbers).
        copies > 1 (one prompt): `copies` continuations of it, the prompt pass of _prefill_shared; sampler=None then walks the greedy loop
        `copies` times over (tests).  processors: _processors_of's dict (its marks one list per prompt: a prompt's list marks every one of
        its continuations); with want_logprobs the log-probabilities are returned last.  shared_rows = S (_shared_prefix_of: B > 1 prompts
        whose first S stripped rows are the same rows): the prompt pass of _prefill_shared_batch.  spec = (K, N, lookup ids per sequence):
        prompt-lookup speculation -- functional.SpecGreedyLoopGraph in place of the loop, K more cache rows, nothing else differs."""
        if inputs_embeds.dtype != BF16:
            raise TypeError(f"inputs_embeds must be bf16, got {inputs_embeds.dtype}")
        dev = inputs_embeds.device
        B, n, h = inputs_embeds.shape
        pads = self._left_pads(attention_mask, B, n)
        F.params_ready(None)
        max_new_tokens = int(max_new_tokens)
        seqs = [inputs_embeds[b, pads[b]:].reshape(n - pads[b], h) for b in range(B)]
        cache = HipKVCache(capacity=max(x.shape[0] for x in seqs) + max_new_tokens + 2 + (spec[0] if spec else 0))
        if copies > 1:
            if B != 1:
                raise ValueError(f"{copies} continuations take one prompt, got {B}")
            x0 = self._prefill_shared(seqs[0], cache, copies, chunk=self._prefill_chunk_rows())
        elif shared_rows:
            x0 = self._prefill_shared_batch(seqs, cache, shared_rows, chunk=self._prefill_chunk_rows())
        else:
            outs = self._prefill_batch(seqs, cache, stepper=False, chunk=self._prefill_chunk_rows())
            x0 = torch.stack([o[-1] for o in outs], 0)
        embed = self.model.embed_tokens.weight.data
        proc = None
        if processors is not None:
            sup = processors["suppress"]
            marks = processors["marks"]
            proc = F.LogitsProcessors(processors["repetition_penalty"], processors["min_new_tokens"],
                                      torch.tensor(sup, dtype=torch.int32).to(dev) if sup else None, processors["want_logprobs"],
                                      None if marks is None else [marks[b // copies] for b in range(B * copies)])
        loop_args = (self.model.layers, cache.meta, cache.kv, cache.meta.cos, cache.meta.sin, h, dev, self._head_rows_device, embed,
                     self._vocab_rows, self._vision_head_out, start_image_token_id, end_image_token_id,
                     self.get_model().vision_tower.image_token_len, max_new_tokens, set(eos_token_id))
        poll = self._poll_steps()
        if spec:
            loop = F.SpecGreedyLoopGraph(*loop_args, lookup_ids=spec[2], num_draft=spec[0], max_ngram=spec[1], poll=poll)
        else:
            loop = F.GreedyLoopGraph(*loop_args, poll=poll, sampler=sampler, processors=proc)
        self._greedy_loop = loop                              # (tools / tests: steps, host_reads, the static logits of the last step)
        ids, embs, *logp = loop.run(x0)
        if B == 1 and copies == 1:                            # one sequence: the return shapes of _greedy_decode_cached
            embs = embs[0] if embs[0].shape[0] else torch.tensor([], dtype=torch.float32, device=dev)
        if logp:
            return (ids, embs, logp[0]) if output_image else (ids, logp[0])
        return (ids, embs) if output_image else ids

    # ------------------------------------------------------------------ beam search, token loop on the device
    def _head_text_rows(self, x, logits_out):
        """final norm + lm_head -> fp32 logits into `logits_out`: the text-only head of the beam loop (no image head is run)"""
        self._lm_head(self.model.norm(x).contiguous(), logits_out)

    def _poll_steps(self):
        """steps between two host reads of a device loop's live counter: config.mm355_greedy_poll_steps (absent: 8)"""
        return getattr(self.config, "mm355_greedy_poll_steps", 8)

    @torch.no_grad()
    def beam_decode(self, position_ids, attention_mask, inputs_embeds, num_beams, eos_token_id=(128001, 128009), max_new_tokens=1024,
                    length_penalty=1.0, early_stopping=False, num_return_sequences=None, output_scores=False, do_sample=None,
                    use_cache=None, output_image=False, repetition_penalty=None, min_new_tokens=None, suppress_tokens=None,
                    output_logprobs=False):
        """HF's beam search (GenerationMixin._beam_search with do_sample=False and no logits processors: the hypotheses of
        generate(use_customize_greedy=False, num_beams=K)) for ONE prompt with the token loop on the device (functional.BeamLoopGraph).
        The prompt (inputs_embeds [1, L, h] bf16; an attention_mask may left-pad it) runs through the decoder once and its cache rows are
        stored and read once for all K = num_beams beams (mm355_attn_decode_shared_idx); a beam's own rows are never moved, a table says
        where they live.  Per token: one captured step, one pass over the weights, no host read (config.mm355_greedy_poll_steps as for
        greedy_decode).  Tokens only: <im_start> is an ordinary id.  Returns the num_return_sequences (default 1) best hypotheses, best
        first, as int32 id tensors -- the generated ids up to and including the eos id that ended them, unpadded; with output_scores=True
        (ids, scores), scores the fp32 `sequences_scores` (sum of log-probabilities / length ** length_penalty).  length_penalty and
        early_stopping (False, True or "never") are HF's.  w8 / w4 weights and the FP8 cache work as in greedy_decode.
        Refused by name before any device work -- ValueError: num_beams no integer in [2, 8], more than one prompt, num_return_sequences
        > num_beams, more eos ids than the device loop takes, a length_penalty that is not finite, another early_stopping,
        max_new_tokens < 1, fewer logits than a step keeps candidates; NotImplementedError: use_cache=False, do_sample, any logits
        processor (repetition_penalty, min_new_tokens, suppress_tokens, output_logprobs), output_image=True, and a head shape
        mm355_attn_decode_shared does not take or set_variant("shared_prefix_attn", False) -- there is no fan-out fallback: use the HF
        path, generate(use_customize_greedy=False, num_beams=K)."""
        try:
            K = -1 if isinstance(num_beams, bool) else operator.index(num_beams)
        except TypeError:
            K = -1
        if not 2 <= K <= F.BEAM_MAX:
            raise ValueError(f"beam_decode: num_beams = {num_beams!r} must be an integer in [2, {F.BEAM_MAX}] (1 beam is greedy_decode)")
        if inputs_embeds.shape[0] != 1:
            raise ValueError(f"beam_decode takes one prompt, got {inputs_embeds.shape[0]}")
        n_ret = self._copies_of(num_return_sequences)
        if n_ret > K:
            raise ValueError(f"beam_decode: num_return_sequences = {n_ret} exceeds num_beams = {K}: the pool holds num_beams hypotheses")
        eos = sorted(set(int(e) for e in ([] if eos_token_id is None else
                                          [eos_token_id] if isinstance(eos_token_id, int) else eos_token_id)))
        if len(eos) > ops.GREEDY_MAX_EOS:
            raise ValueError(f"beam_decode: {len(eos)} eos ids: the device loop takes up to {ops.GREEDY_MAX_EOS}")
        try:
            length_penalty = float(length_penalty)
        except (TypeError, ValueError):
            length_penalty = float("nan")
        if not math.isfinite(length_penalty):
            raise ValueError("beam_decode: length_penalty must be a finite number")
        if early_stopping not in (False, True, "never") or (isinstance(early_stopping, (int, float)) and not isinstance(early_stopping, bool)):
            raise ValueError(f"beam_decode: early_stopping = {early_stopping!r} must be False, True or 'never'")
        if isinstance(max_new_tokens, bool) or not isinstance(max_new_tokens, int) or max_new_tokens < 1:
            raise ValueError(f"beam_decode: max_new_tokens = {max_new_tokens!r} must be an integer >= 1")
        V = self._vocab_rows
        M = F.beam_candidates(K, len(eos))
        if V < M:
            raise ValueError(f"beam_decode: {V} logits are fewer than the {M} candidates a step of {K} beams with {len(eos)} eos ids keeps")
        if not (use_cache is None or use_cache):
            raise NotImplementedError("beam_decode(use_cache=False): the beams live in the KV cache (use_cache=True)")
        if do_sample:
            raise NotImplementedError("beam_decode(do_sample=True): beam sampling is not part of the device beam loop")
        if (repetition_penalty not in (None, 1, 1.0) or min_new_tokens not in (None, 0) or (suppress_tokens is not None and len(suppress_tokens))
                or output_logprobs):
            raise NotImplementedError("beam_decode(repetition_penalty / min_new_tokens / suppress_tokens / output_logprobs): logits "
                                      "processors are not part of the device beam loop (HF applies them after the log-softmax)")
        if output_image:
            raise NotImplementedError("beam_decode(output_image=True): the beam loop is token-only, image rows are not generated under beams")
        cfg = self.config
        hf_path = "use the HF path: generate(use_customize_greedy=False, num_beams=K)"
        if not ops.attn_decode_shared_supported(cfg.num_attention_heads, cfg.num_key_value_heads, _head_dim(cfg)):
            raise NotImplementedError(f"beam_decode: mm355_attn_decode_shared does not take the head shape Hq={cfg.num_attention_heads} "
                                      f"Hkv={cfg.num_key_value_heads} d={_head_dim(cfg)} and there is no fan-out fallback; {hf_path}")
        if not F.VARIANTS["shared_prefix_attn"]:
            raise NotImplementedError(f'beam_decode with set_variant("shared_prefix_attn", False): the beams share the prompt\'s cache rows '
                                      f"and there is no fan-out fallback; {hf_path}")
        if inputs_embeds.dtype != BF16:
            raise TypeError(f"inputs_embeds must be bf16, got {inputs_embeds.dtype}")
        dev = inputs_embeds.device
        _, n, h = inputs_embeds.shape
        pads = self._left_pads(attention_mask, 1, n)
        F.params_ready(None)
        x2d = inputs_embeds[0, pads[0]:].reshape(n - pads[0], h)
        cache = HipKVCache(capacity=x2d.shape[0] + max_new_tokens + 2)
        x0 = self._prefill_shared(x2d, cache, K, chunk=self._prefill_chunk_rows(), own_rows=max_new_tokens + 1)
        loop = F.BeamLoopGraph(self.model.layers, cache.meta, cache.kv, cache.meta.cos, cache.meta.sin, h, dev, self._head_text_rows,
                               self.model.embed_tokens.weight.data, V, max_new_tokens, eos, length_penalty, early_stopping,
                               poll=self._poll_steps())
        self._beam_loop = loop                                # (tools / tests: steps, host_reads, the final state)
        ids, scores, _ = loop.run(x0)
        out = [torch.from_numpy(i).to(dev) for i in ids[:n_ret]]
        return (out, torch.from_numpy(scores[:n_ret].copy()).to(dev)) if output_scores else out

    # ------------------------------------------------------------------ HF generate() on the decode kernels (reference :711-738)
    def _new_kv_cache(self, cache, rows, batch, device):
        """`cache.kv`: a fresh functional.KVCache of `batch` sequences for a prompt of `rows` rows (the HipKVCache's own capacity and
        format, else rows + 1024 + 2 and the config's), and `cache.meta`, the geometry of its steps with the RoPE tables of that capacity.
        Returns (meta, cos, sin)."""
        cap = cache.capacity if cache.capacity is not None else rows + 1024 + 2
        if cap < rows + 1:
            raise ValueError(f"HipKVCache capacity {cap} is smaller than the prompt ({rows} rows)")
        cos, sin = self.model.rope_tables(cap, device)
        _, meta = self._decode_meta(rows)
        meta.cos, meta.sin = cos, sin
        cache.kv = F.KVCache(len(self.model.layers), cap, meta.Hkv * meta.d, device, Hq=meta.Hq, d=meta.d, batch=batch,
                             fmt=self._kv_cache_format(cache.kv_format))
        cache.meta = meta
        return meta, cos, sin

    def _prefill_batch(self, seqs, cache, stepper=True, chunk=None):
        """Prompt pass of a batch: seqs = one [L_b, h] tensor of prompt rows per sequence (padding already stripped) -> their hidden rows
        (pre final norm), one [L_b, h] tensor each; allocates and fills `cache.kv` and captures the per-token step.  Prompts of one length
        (the beams of a beam search, an unpadded batch) go through the decoder as ONE batch; ragged prompts one after the other -- or, with
        config.mm355_ragged_pass = True and no chunking, packed into ONE functional.decoder_extend_ragged pass on the fresh cache.
        stepper=False: no DecodeStepGraph is captured (the greedy loop brings its own step); chunk: rows per slice of a chunked prompt pass
        (functional.decoder_prefill_chunked), one sequence after the other."""
        dev = seqs[0].device
        B, h = len(seqs), seqs[0].shape[1]
        lens = [int(x.shape[0]) for x in seqs]
        L0 = max(lens)
        meta, cos, sin = self._new_kv_cache(cache, L0, B, dev)
        ragged = self._ragged_pass(meta)
        if B > 1 and all(n == L0 for n in lens) and (chunk is None or L0 <= chunk):
            _, mb = self._decode_meta(L0)
            mb.B, mb.cos, mb.sin = B, cos, sin
            rows = F.decoder_prefill(torch.cat(seqs, 0), self.model.layers, mb, cache.kv)
            out = list(rows.view(B, L0, h).unbind(0))
        elif ragged and B > 1 and (chunk is None or L0 <= chunk):
            out = F.decoder_extend_ragged([x2d.contiguous() for x2d in seqs], self.model.layers, meta, cache.kv)
        else:
            out = []
            for b, x2d in enumerate(seqs):
                _, mb = self._decode_meta(lens[b])
                mb.cos, mb.sin = cos, sin
                out.append(F.decoder_prefill_chunked(x2d.contiguous(), self.model.layers, mb, cache.kv, chunk, row=b))
        if stepper:
            cache.stepper = F.DecodeStepGraph(self.model.layers, meta, cache.kv, cos, sin, h, dev)
        return out

    def _prefill_shared(self, x2d, cache, n, chunk=None, own_rows=None):
        """Prompt pass of n continuations of ONE prompt x2d [L, h]: the prompt runs once into sequence 0 of a cache of n sequences; returns
        the prompt's last hidden row (pre final norm) n times, [n, h].  Afterwards every sequence holds L rows and, on the shared route
        (functional.VARIANTS["shared_prefix_attn"] and a head shape mm355_attn_decode_shared takes), rows [0, L) of sequence 0 are every
        sequence's first rows (KVCache.set_shared); else they are copied into every sequence's block (KVCache.copy_prefix) and the step
        runs on the batch's attention.  own_rows (beam_decode, which has checked that the shared route applies): the columns of the
        table of own rows, KVCache.set_shared(L, own_rows=...)."""
        L, h = int(x2d.shape[0]), x2d.shape[1]
        meta, cos, sin = self._new_kv_cache(cache, L, n, x2d.device)
        kv = cache.kv
        _, mb = self._decode_meta(L)
        mb.cos, mb.sin = cos, sin
        rows = F.decoder_prefill_chunked(x2d.contiguous(), self.model.layers, mb, kv, chunk, row=0)
        if F.VARIANTS["shared_prefix_attn"] and ops.attn_decode_shared_supported(meta.Hq, meta.Hkv, meta.d):
            kv.set_lengths([L] * n)
            kv.set_shared(L, own_rows=own_rows)
        else:
            assert own_rows is None
            kv.copy_prefix(L)
            kv.set_lengths([L] * n)
        return rows[-1:].expand(n, h).contiguous()

    def _prefill_shared_batch(self, seqs, cache, S, chunk=None):
        """Prompt pass of B prompts whose first S rows are the same rows: seqs = one [L_b, h] tensor per sequence (padding stripped, 1 <= S
        <= min L_b - 1) -> the last hidden row (pre final norm) of every prompt, [B, h].  The S rows run once into sequence 0 of a cache of
        B sequences.  On the shared route (functional.VARIANTS["shared_prefix_attn"] and a head shape mm355_attn_extend_shared takes) they
        become every sequence's first rows (KVCache.set_shared) and the own rows n_b = L_b - S of all sequences run as ONE
        functional.decoder_extend_shared pass on [B, max n_b, h], right-padded with zero rows.  The padding is safe: rows are independent
        outside attention and attention is causal over the own rows, so a valid row never sees a padding row; the padding rows' K / V land
        at own rows >= L_b, which the loop's kv_lens[b] keeps unread until its appends have overwritten them from row L_b on.  Else
        (fan-out) the rows are copied into every sequence's block (KVCache.copy_prefix), the own rows go through decoder_extend one
        sequence after the other and the step runs on the batch's attention.  Afterwards sequence b holds L_b rows."""
        dev = seqs[0].device
        B, h = len(seqs), seqs[0].shape[1]
        lens = [int(x.shape[0]) for x in seqs]
        L0 = max(lens)
        assert B > 1 and 1 <= S <= min(lens) - 1, (B, S, lens)
        meta, cos, sin = self._new_kv_cache(cache, L0, B, dev)
        kv = cache.kv
        _, mb = self._decode_meta(S)
        mb.cos, mb.sin = cos, sin
        F.decoder_prefill_chunked(seqs[0][:S].contiguous(), self.model.layers, mb, kv, chunk, row=0)
        if F.VARIANTS["shared_prefix_attn"] and ops.attn_extend_shared_supported(meta.Hq, meta.Hkv, meta.d):
            kv.set_lengths([S] * B)
            kv.set_shared(S)
            own = torch.zeros((B, L0 - S, h), device=dev, dtype=seqs[0].dtype)
            for b, x2d in enumerate(seqs):
                own[b, :lens[b] - S] = x2d[S:]
            rows = F.decoder_extend_shared(own, self.model.layers, meta, kv)
            kv.set_lengths(lens)
            return torch.stack([rows[b, lens[b] - S - 1] for b in range(B)], 0)
        kv.copy_prefix(S)
        kv.set_lengths([S] * B)
        return torch.stack([F.decoder_extend(x2d[S:].contiguous(), self.model.layers, meta, kv, row=b)[-1] for b, x2d in enumerate(seqs)], 0)

    def _decode_batch(self, x, cache):
        """New rows x [B, n, h] (the hook of n = 1: one row per sequence and step) appended against the batch's cache, every position in ONE
        pass for all B sequences -> their hidden rows [B, n, h] (pre final norm)."""
        outs = [cache.stepper.step(x[:, t].contiguous()).clone() for t in range(x.shape[1])]
        return outs[0].unsqueeze(1) if len(outs) == 1 else torch.stack(outs, 1)

    def _extend_batch(self, x, cache, rows=None):
        """n > 1 new rows per sequence x [B, n, h] on the FILLED cache -> their hidden rows [B, n, h] (pre final norm): one extend pass per
        sequence (functional.decoder_extend: the weights streamed once for its n rows), one sequence after the other as ragged prompts run
        -- or, with config.mm355_ragged_pass = True and B > 1, ONE functional.decoder_extend_ragged pass for all B sequences.
        rows: the sequences of the cache the B row blocks belong to (default: all of them, in order).  functional.set_variant("extend_pass",
        False), or fewer than VARIANTS["extend_min_rows"] rows: the captured decode step once per row (all sequences at once)."""
        B, n, h = x.shape
        kv = cache.kv
        rows = list(range(kv.batch)) if rows is None else [int(b) for b in rows]
        if len(rows) != B:
            raise ValueError(f"{B} row blocks for {len(rows)} sequences")
        need = max(kv.lengths[b] for b in rows) + n
        if need > kv.max_len:
            raise ValueError(f"HipKVCache capacity {kv.max_len} is smaller than the {need} rows this call extends a sequence to "
                             "(size it with HipKVCache(capacity=...); a cache is not grown)")
        if (not F.VARIANTS["extend_pass"] or n < F.VARIANTS["extend_min_rows"]) and rows == list(range(kv.batch)):
            return MetaMorphLlamaForCausalLM._decode_batch(self, x, cache)
        if self._ragged_pass(cache.meta) and B > 1:             # one pass for all B sequences, each at its own cached length
            return torch.stack(F.decoder_extend_ragged(list(x.contiguous().unbind(0)), self.model.layers, cache.meta, kv, rows=rows), 0)
        return torch.stack([F.decoder_extend(x[j].contiguous(), self.model.layers, cache.meta, kv, row=b) for j, b in enumerate(rows)], 0)

    def _rows_logits(self, rows, return_hidden=False):
        """final norm + lm_head -> fp32 logits [n, V] (reference :349-359 final norm, :393-399); return_hidden: (logits, normed rows)."""
        hid = self.model.norm(rows)
        logits = self._lm_head(hid.contiguous())
        return (logits, hid) if return_hidden else logits

    @torch.no_grad()
    def _cached_forward(self, input_ids, inputs_embeds, attention_mask, past_key_values, return_dict):
        F.params_ready(None)
        if inputs_embeds is None:
            inputs_embeds = self.model.embed_tokens(input_ids)
        if inputs_embeds.dtype != BF16:
            raise TypeError(f"inputs_embeds must be bf16, got {inputs_embeds.dtype}")
        cache = past_key_values
        if isinstance(cache, HipKVCache) and cache.kv is not None and attention_mask is not None and inputs_embeds.shape[1] > 1:
            # continuing a conversation: generate(inputs=<whole conversation>, past_key_values=<cache holding a prefix of it>).  The mask
            # covers cached + new positions whatever the installed transformers did with the inputs_embeds of a filled cache, so the rows
            # beyond (mask length - cached length) from the end are the cached prefix: only the rest goes through the decoder
            new = int(attention_mask.shape[1]) - cache.get_seq_length()
            if 0 < new < inputs_embeds.shape[1]:
                inputs_embeds = inputs_embeds[:, -new:]
        B, n, h = inputs_embeds.shape
        if cache is None:
            cache = HipKVCache()
        if not isinstance(cache, HipKVCache):
            if cache.get_seq_length() != 0:
                raise NotImplementedError("past_key_values must be a metamorph_amd HipKVCache (generate() creates one); a foreign, "
                                          "already filled transformers Cache holds tensors in another layout")
            cache = HipKVCache()                              # an empty HF cache object: swap in ours
        first = cache.kv is None
        if first:
            # batch rows / beams are independent sequences of ONE cache.  A batch of prompts of different lengths arrives LEFT-padded with
            # its attention mask (the reference: HF generate derives position_ids = cumsum(mask) - 1 from it, so every row is decoded
            # exactly as it would be alone).  Here the padding rows are never computed or cached: each sequence keeps its own length,
            # `pads` only restores the common length HF counts.
            pads = self._left_pads(attention_mask, B, n)
            cache.pads = pads
            seqs = [inputs_embeds[b, pads[b]:].reshape(n - pads[b], h) for b in range(B)]
            chunk = self._prefill_chunk_rows(cache)
            if chunk is None or max(x.shape[0] for x in seqs) <= chunk:
                outs = self._prefill_batch(seqs, cache)
            else:
                if cache.capacity is None:                    # (the prompt hook sizes the cache from the rows it is given)
                    cache.capacity = max(x.shape[0] for x in seqs) + 1024 + 2
                outs = [[o] for o in self._prefill_batch([x[:chunk] for x in seqs], cache)]
                for r0 in range(chunk, max(x.shape[0] for x in seqs), chunk):
                    live = [b for b in range(B) if seqs[b].shape[0] > r0]
                    if len({min(seqs[b].shape[0], r0 + chunk) for b in live}) == 1:      # one slice length: one call for all of them
                        ys = self._extend_batch(torch.stack([seqs[b][r0:r0 + chunk] for b in live], 0), cache,
                                                **({} if len(live) == B else {"rows": live}))
                        for j, b in enumerate(live):
                            outs[b].append(ys[j])
                    else:
                        for b in live:
                            outs[b].append(self._extend_batch(seqs[b][None, r0:r0 + chunk], cache, rows=[b])[0])
                outs = [torch.cat([t.to(o[0].dtype) for t in o], 0) for o in outs]
            # padding positions: rows nobody reads (HF takes logits[:, -1])
            rows = torch.cat([r if not pads[b] else torch.cat([r.new_zeros((pads[b], h)), r], 0) for b, r in enumerate(outs)], 0)
        else:
            if len(cache.pads) != B:
                raise ValueError(f"cache holds {len(cache.pads)} sequences, the step brings {B}")
            rows = (self._decode_batch if n == 1 else self._extend_batch)(inputs_embeds, cache).reshape(B * n, h)
        logits, hidden = self._rows_logits(rows.contiguous(), return_hidden=True)
        logits, hidden = logits.view(B, n, -1), hidden.view(B, n, h)
        if return_dict is False:
            return (logits, cache)
        return CausalLMOutputWithPast(loss=None, logits=logits, past_key_values=cache, hidden_states=hidden, attentions=None)

    def prepare_inputs_for_generation(self, input_ids, past_key_values=None, inputs_embeds=None, **kwargs):
        """Reference metamorph_llama.py:721-735: the HF default plus `images` / `image_sizes` handed through."""
        images = kwargs.pop("images", None)
        image_sizes = kwargs.pop("image_sizes", None)
        inputs = super().prepare_inputs_for_generation(input_ids, past_key_values=past_key_values, inputs_embeds=inputs_embeds, **kwargs)
        if images is not None:
            inputs["images"] = images
        if image_sizes is not None:
            inputs["image_sizes"] = image_sizes
        return inputs

    @torch.no_grad()
    def generate(self, inputs=None, images=None, image_sizes=None, output_image=False, use_customize_greedy=True,
                 image_embeds=None, **kwargs):
        position_ids = kwargs.pop("position_ids", None)
        attention_mask = kwargs.pop("attention_mask", None)
        device_beam_search = kwargs.pop("device_beam_search", False)
        if kwargs.get("shared_prefix_rows") is None:
            kwargs.pop("shared_prefix_rows", None)               # (None is the call without the argument, on every route)
        elif device_beam_search or not use_customize_greedy:
            # (before the prompt is embedded: the shared-prefix batch is a route of greedy_decode's device loop only)
            raise ValueError(f"generate(shared_prefix_rows={kwargs['shared_prefix_rows']!r}) runs in greedy_decode's device loop: not with "
                             + ("device_beam_search=True (the beams of one prompt share its rows already)" if device_beam_search else
                                "use_customize_greedy=False (HF's generate path drives forward() and knows no shared prefix)"))
        if use_customize_greedy or device_beam_search:
            # prompt-lookup speculation is a route of greedy_decode's device loop, which looks the drafts up in `inputs`; with
            # use_customize_greedy=False the arguments go on to HF untouched, which has the option itself
            if self._prompt_lookup_arg(kwargs.get("prompt_lookup_num_tokens"), kwargs.get("max_matching_ngram_size")) is None:
                for name in ("prompt_lookup_num_tokens", "max_matching_ngram_size", "prompt_lookup_ids"):
                    kwargs.pop(name, None)                       # (None / 0 is the call without the arguments)
            elif device_beam_search:
                raise ValueError(f"generate(prompt_lookup_num_tokens={kwargs['prompt_lookup_num_tokens']!r}) runs in greedy_decode's device "
                                 "loop: not with device_beam_search=True (a draft is verified against the argmax, not against a beam)")
            elif kwargs.get("prompt_lookup_ids") is None and inputs is not None:
                # (read here, with the mask of the ids: the prompt's rows, and with them the mask, grow where an image is spliced in)
                kwargs["prompt_lookup_ids"] = self._prompt_lookup_ids(inputs, attention_mask, inputs.shape[0])
        if images is not None or image_embeds is not None:
            (_, position_ids, attention_mask, _, inputs_embeds, _, _, _) = self.prepare_inputs_labels_for_multimodal(
                inputs, position_ids, attention_mask, None, None, images, image_sizes=image_sizes, image_embeds=image_embeds)
        else:
            inputs_embeds = self.get_model().embed_tokens(inputs)
        if device_beam_search:
            # beam search with the token loop on the device (beam_decode): HF's hypotheses without HF's per-token host loop and cache reorder
            return self.beam_decode(position_ids=position_ids, attention_mask=attention_mask, inputs_embeds=inputs_embeds,
                                    output_image=output_image, **kwargs)
        if not use_customize_greedy:
            # reference :711-717: `super().generate(position_ids=..., attention_mask=..., inputs_embeds=..., **kwargs)` -- HF's sampling
            # / greedy search driving forward() with a cache.  Here the cache is a HipKVCache (decode kernels + hipGraph replay).
            if kwargs.get("past_key_values") is None and kwargs.get("use_cache", True):
                L0 = int(inputs_embeds.shape[1])
                new = kwargs.get("max_new_tokens")
                if new is None and kwargs.get("max_length") is not None:
                    new = max(int(kwargs["max_length"]) - L0, 1)         # HF subtracts the inputs_embeds length from max_length itself
                if new is None:
                    gc = kwargs.get("generation_config") or self.generation_config
                    new = getattr(gc, "max_new_tokens", None)
                    if new is None:                                      # HF's max_length is a TOTAL that includes the inputs_embeds rows
                        new = max(int(getattr(gc, "max_length", None) or 20) - L0, 1)
                kwargs["past_key_values"] = HipKVCache(capacity=L0 + int(new) + 2)
            return GenerationMixin.generate(self, position_ids=position_ids, attention_mask=attention_mask, inputs_embeds=inputs_embeds,
                                            **kwargs)
        return self.greedy_decode(position_ids=position_ids, attention_mask=attention_mask, inputs_embeds=inputs_embeds,
                                  output_image=output_image, **kwargs)


for _reg, _args in ((AutoConfig.register, ("metamorph_llama", MetaMorphConfig)),
                    (AutoModelForCausalLM.register, (MetaMorphConfig, MetaMorphLlamaForCausalLM))):
    try:
        _reg(*_args)
    except ValueError:      # already registered (e.g. the reference package imported in the same process)
        pass
