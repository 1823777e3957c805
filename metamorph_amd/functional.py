"""torch.autograd glue around the libmm355 kernels.

Each Function's forward AND backward are sequences of HIP kernels (metamorph_amd.ops); autograd is used
only to order them and to carry the activation gradients between the coarse blocks.  Weight gradients are
written by the backward kernels straight into persistent gradient buffers (`param.grad` becomes a view of
them) -- the "contiguous_gradients" behaviour of the reference's DeepSpeed ZeRO-2 config
(reference scripts/zero2.json:23) -- so no per-step gradient allocation or extra accumulate pass exists.
"""
from __future__ import annotations

import dataclasses
import math
import os
from collections import namedtuple

import numpy as np
import torch
from torch.autograd import Function

from . import ops

BF16 = torch.bfloat16
# Kernel-composition switches of the decoder layer.  The product runs the defaults (each one measured the winner on MI355X, DESIGN.md
# section 4); tools/ and tests flip them through set_variant() for same-box A/B runs -- there is no environment switch.
#   fuse_swiglu     SwiGLU in the gate|up GEMM's epilogue (same bits, one pass less)
#   fuse_rope       RoPE in the q|k|v GEMM's epilogue / inverse RoPE in the attention backward epilogues (same bits)
#   fuse_swiglu_bwd SwiGLU backward in the down_proj input-gradient GEMM's epilogue (same bits)
#   decode_graph    the per-token decode step is captured once as a hipGraph and replayed
VARIANTS = {"fuse_swiglu": True, "fuse_rope": True, "fuse_swiglu_bwd": True, "decode_graph": True, "decode_fused": True,
            # keep the transposed copies of the decoder weights (the B operands of the input-gradient GEMMs) from one backward call to
            # the next until the optimizer rewrites the parameters: under gradient accumulation the four transposes per layer are made
            # once per optimizer step instead of once per micro-batch (+2 bytes per decoder parameter while a window is open)
            "wt_cache": False,
            "decode_fold_rows": 4,                           # decode step: fold the RMSNorms into the GEMVs' operand reads up to this many rows
            # prompt pass of a cached decode: q|k|v, o and down projections through the split-K GEMM (a few hundred rows: the plain kernels are a
            # latency chain over K there)
            "prefill_splitk": True,
            # decode step of MORE than 16 sequences (one pass over the weights through the split-K GEMM): RoPE + cache append, the two RMSNorms
            # and SwiGLU folded into the reduce launches of the split projections (nine launches per layer instead of thirteen; same bits)
            "decode_wide_fused": True, "decode_wide_gu_gemv": True,
            # the prompt pass of ONE sequence (a few hundred rows): the same reduce launches (RoPE + the K / V rows straight into the cache, both
            # RMSNorms), attention reading K / V from the cache rows -- same bits as the prefill_splitk pass, five launches per layer less
            "prefill_fused": True,
            # quantised layers (quantize_decoder_): projections of the prompt pass and of decode steps of more than 16 sequences on the w8
            # split-K GEMM (mm355_gemm_w8*: the weight bytes streamed once); off: every such projection through the W8Scratch route
            "w8_gemm": True,
            # the same switch for layers in format "mxfp4" (mm355_gemm_w4*), so that the two formats can be compared independently
            "w4_gemm": True,
            # n > 1 new rows on a filled cache (a follow-up turn, a prompt run in chunks): ONE pass over the weights with mm355_attn_extend
            # (decoder_extend); off, or fewer than extend_min_rows rows: one captured decode step per row (two rows: the pass's floor of one
            # split-K stream over the weights is 0.81 - 1.46 x two GEMV steps, profiles/extend_pass.md)
            "extend_pass": True, "extend_min_rows": 3,
            # greedy_decode of ONE sequence through the device-resident loop that batches take (GreedyLoopGraph) instead of the host loop
            "greedy_loop_b1": False,
            # n continuations of one prompt (greedy_decode(num_return_sequences=n)): the prompt's cache rows stored once in sequence 0 and read
            # once per KV head and step by mm355_attn_decode_shared (KVCache.set_shared); off, or where that kernel does not take the shape:
            # the rows are copied into every sequence's block and the step runs on mm355_attn_decode.  The prompt runs once either way.
            "shared_prefix_attn": True,
            # B prompts that begin alike (greedy_decode(shared_prefix_rows="auto")): the smallest common prefix, in rows, that is worth the
            # shared route (the prefix once + one decoder_extend_shared pass); below it the ordinary batch.  512: the smallest measured prefix
            # from which no cell of profiles/shared_prefix_batch.md loses -- at 1 / 16 / 128 shared rows two passes over the weights cost
            # more than the one batched prompt pass of prompts of equal length (0.56 - 0.90 x); an int S is taken at its word
            "shared_prefix_min_rows": 512,
            # a model with config.mm355_ragged_pass = True: ragged prompts, and follow-up turns of B > 1 sequences, as ONE packed pass over the
            # weights with mm355_attn_extend_ragged (decoder_extend_ragged); off: one sequence after the other, as without the config field.
            # The tools' switch for same-process A/B runs (profiles/ragged_pass.md); the config field, default off, is the product's
            "ragged_pass_attn": True}


def set_variant(name, value):
    """Flip one composition switch (tools / tests); returns the previous value."""
    if name not in VARIANTS:
        raise KeyError(f"unknown variant {name!r}: {sorted(VARIANTS)}")
    old, VARIANTS[name] = VARIANTS[name], (int(value) if isinstance(VARIANTS[name], int) and not isinstance(VARIANTS[name], bool) else bool(value))
    return old


_CUS = 256                                                   # MI355X: one 256x256 tile per CU at a time


# ------------------------------------------------------------------------------------------------
# parameter / gradient storage helpers
# ------------------------------------------------------------------------------------------------

def _adjacent(ts):
    """True if the 2-D contiguous tensors `ts` are back-to-back rows of ONE storage object (tensors that merely
    happen to sit next to each other in the caching allocator do not count: a view over them would outgrow the
    first tensor's storage)."""
    t0 = ts[0]
    ptr = t0.data_ptr()
    st = t0.untyped_storage()
    total = sum(t.numel() * t.element_size() for t in ts)
    if ptr - st.data_ptr() + total > st.nbytes():
        return False
    for t in ts:
        if (not t.is_contiguous() or t.data_ptr() != ptr or t.shape[1:] != t0.shape[1:] or t.dtype != t0.dtype
                or t.untyped_storage().data_ptr() != st.data_ptr()):
            return False
        ptr += t.numel() * t.element_size()
    return True


def _view_rows(first, rows):
    """A [rows, cols] tensor aliasing the storage that starts at `first` (a contiguous 2-D tensor)."""
    out = first.new_empty(0)
    out.set_(first.untyped_storage(), first.storage_offset(), (rows, first.shape[1]), (first.shape[1], 1))
    return out


def fused_weight(params):
    """One [sum rows, K] tensor holding `params` back to back; re-points the parameters into it if needed."""
    datas = [p.data for p in params]
    rows = sum(d.shape[0] for d in datas)
    if _adjacent(datas):
        return _view_rows(datas[0], rows)
    buf = torch.empty((rows, datas[0].shape[1]), device=datas[0].device, dtype=datas[0].dtype)
    off = 0
    for p, d in zip(params, datas):
        buf[off:off + d.shape[0]].copy_(d)
        p.data = buf[off:off + d.shape[0]]
        off += d.shape[0]
    return buf


# Bumped by every optimizer step that rewrites parameters through raw pointers (Zero2AdamW / Zero3AdamW: mm355_adamw_shard and
# in-place collectives do not touch torch's per-tensor version counters); derived operand caches key on it.
_PARAM_GENERATION = [0]


def bump_param_generation():
    _PARAM_GENERATION[0] += 1


def param_generation():
    return _PARAM_GENERATION[0]


_LAYER_GRAD_HOOK = None


def set_layer_grad_hook(fn):
    """fn(layer) is called at the end of every DecoderLayerFn.backward (Zero2AdamW starts that layer's gradient
    reduce-scatter there, overlapping it with the backward of the earlier layers); None removes it."""
    global _LAYER_GRAD_HOOK
    _LAYER_GRAD_HOOK = fn


_PARAM_READY_HOOK = None


def set_param_ready_hook(fn):
    """fn(key) is called before a group of trainable parameters is first read in a forward pass -- key = the decoder layer
    module, or None for everything outside the decoder layers.  Zero2AdamW's asynchronous update makes the compute stream
    wait there for that segment's update (and all-gather) instead of at the end of step()."""
    global _PARAM_READY_HOOK
    _PARAM_READY_HOOK = fn


def params_ready(key=None, backward=False):
    """key = the decoder layer module about to be read (None: everything outside the decoder layers); backward=True when the
    reader is that layer's backward pass (Zero3AdamW then also attaches the layer's gradient slot)."""
    if _PARAM_READY_HOOK is not None:
        _PARAM_READY_HOOK(key, backward)


def grad_target(p):
    """(buffer, accumulate) for the gradient of parameter `p`."""
    if p.grad is not None:
        return p.grad, True
    buf = getattr(p, "_mm_grad_buf", None)
    if buf is None or buf.shape != p.shape or buf.device != p.device or buf.dtype != p.dtype:
        buf = torch.empty_like(p.data)
        p._mm_grad_buf = buf
    return buf, False


def commit_grad(p, buf):
    if p.grad is None:
        p.grad = buf


def fused_grad_target(params):
    """(fused buffer [sum rows, K], accumulate) whose row blocks are / become the .grad of `params`."""
    grads = [p.grad for p in params]
    rows = sum(p.shape[0] for p in params)
    if all(g is not None for g in grads) and _adjacent(grads):
        return _view_rows(grads[0], rows), True, None
    if all(g is None for g in grads):
        bufs = []
        for p in params:
            b = getattr(p, "_mm_grad_buf", None)
            bufs.append(b if (b is not None and b.shape == p.shape and b.device == p.device) else None)
        if any(b is None for b in bufs) or not _adjacent(bufs):
            big = torch.empty((rows, params[0].shape[1]), device=params[0].device, dtype=params[0].dtype)
            off = 0
            bufs = []
            for p in params:
                p._mm_grad_buf = big[off:off + p.shape[0]]
                bufs.append(p._mm_grad_buf)
                off += p.shape[0]
        return _view_rows(bufs[0], rows), False, bufs
    # mixed state (some grads set, some not): compute into a scratch buffer, then add per parameter
    return torch.empty((rows, params[0].shape[1]), device=params[0].device, dtype=params[0].dtype), None, None


def commit_fused_grad(params, fused, accumulate, bufs):
    if accumulate is True:
        return
    if accumulate is False:
        for p, b in zip(params, bufs):
            if p.requires_grad:
                p.grad = b
        return
    off = 0
    for p in params:
        blk = fused[off:off + p.shape[0]]
        off += p.shape[0]
        if not p.requires_grad:
            continue
        tgt, acc = grad_target(p)
        ops.axpy_(tgt, blk.contiguous(), None, 1.0, acc)
        commit_grad(p, tgt)


def _padded_rows(R, long_k=False):
    """K dimension a transposed copy of R rows gets: a multiple of 8 (legal GEMM K), or of 128 for a long contraction headed for
    the ping-pong kernel (whole pairs of 64-wide K tiles: keeps a ragged token count off the register-staged fallback kernel)."""
    return (R + 127) // 128 * 128 if (long_k and R >= 512) else (R + 7) // 8 * 8


def transpose_padded(x2d, Rp=None):
    """x [R, C] -> [C, Rp] with zero padding columns (they add nothing to a product contracted over them); Rp defaults to R
    rounded up to 8."""
    R, C = x2d.shape
    Rp = _padded_rows(R) if Rp is None else Rp
    buf = torch.empty((C, Rp), device=x2d.device, dtype=BF16)
    if Rp != R:
        buf[:, R:].zero_()                                    # only the padding columns
    ops.transpose(x2d, out=buf[:, :R])
    return buf


def _dw_operands(dy2d, x2d, dyT=None, xT=None):
    """Contraction-major operands (dy^T [N, Mp], x^T [K, Mp]) of a weight-gradient GEMM in NT form; a copy a producer already
    wrote (dyT / xT) fixes Mp, otherwise long contractions are padded to whole pairs of K tiles."""
    R = (dy2d if dy2d is not None else x2d).shape[0]
    Rp = dyT.shape[1] if dyT is not None else (xT.shape[1] if xT is not None else _padded_rows(R, long_k=True))
    return (transpose_padded(dy2d, Rp) if dyT is None else dyT, transpose_padded(x2d, Rp) if xT is None else xT)


def weight_grad_gemm(dy2d, x2d, out, accumulate, dyT=None, xT=None):
    """out[N,K] (+)= dy[M,N]^T @ x[M,K] as the NT GEMM of the explicitly transposed operands.  dyT / xT: contraction-major
    copies a producer already wrote (the row-major argument may then be None)."""
    a, b = _dw_operands(dy2d, x2d, dyT, xT)
    ops.gemm(a, b, out=out, accumulate=accumulate)


def _pair_saves_a_wave(rows0, cols0, rows1, cols1, contraction):
    """Two weight gradients [rows, cols] over `contraction` token rows: does one paired launch of the 256x256 kernel need fewer
    waves of workgroups than two launches?  (Both must be problems the ping-pong kernel takes on its own: >= 200 tiles.)"""
    t0 = -(-rows0 // 256) * -(-cols0 // 256)
    t1 = -(-rows1 // 256) * -(-cols1 // 256)
    kp = _padded_rows(contraction, long_k=True)
    if min(t0, t1) < 200 or kp % 128:
        return False
    return -(-(t0 + t1) // _CUS) < -(-t0 // _CUS) + -(-t1 // _CUS)


_WT_CACHE = {}                                               # (storage, offset, shape, strides) -> ((generation, source versions...), transposed copy)


def transposed_weight(w, sources=None):
    """w [N, K] -> [K, Np] (transpose_padded).  With VARIANTS["wt_cache"] AND `sources` given the copy is kept until the parameters change:
    same bits, one transpose per optimizer step.  `sources` = the parameters w is (a fused view of); it is passed only at the decoder
    layer's own call sites, whose operands are long-lived parameters or views of the optimizer's flat buffer -- never by the generic
    input_grad_gemm (LinearFn / LinearWBFn also see per-forward temporaries, whose address a later tensor can reuse).  An entry is valid
    for one parameter generation (`bump_param_generation`: every optimizer step / checkpoint load, which write behind torch's back) AND one
    set of torch version counters of the sources (any in-place write through torch -- copy_, load_state_dict, mul_ -- invalidates it
    without anybody having to bump)."""
    if sources is None or not VARIANTS["wt_cache"]:
        return transpose_padded(w)
    key = (w.untyped_storage().data_ptr(), w.storage_offset(), tuple(w.shape), tuple(w.stride()))
    stamp = (param_generation(),) + tuple(p._version for p in sources)
    hit = _WT_CACHE.get(key)
    if hit is not None and hit[0] == stamp:
        return hit[1]
    if _WT_CACHE and next(iter(_WT_CACHE.values()))[0][0] != stamp[0]:
        _WT_CACHE.clear()                                     # a new generation: every cached copy is stale
    wt = transpose_padded(w)
    _WT_CACHE[key] = (stamp, wt)
    return wt


def drop_transposed_weights():
    _WT_CACHE.clear()


def _pairable(a0, b0, a1, b1):
    """Two plain NT problems worth one launch: each big enough for the 256 x 256 kernel on its own (>= 200 tiles), the first a whole
    number of 8 workgroups (the second problem's workgroups then keep their XCD), both eligible for mm355_gemm_pair_bf16."""
    t0 = -(-a0.shape[0] // 256) * -(-b0.shape[0] // 256)
    t1 = -(-a1.shape[0] // 256) * -(-b1.shape[0] // 256)
    return min(t0, t1) >= 200 and t0 % 8 == 0 and ops.gemm_pair_supported(a0, b0, a1, b1)


def input_grad_gemm(dy2d, w, out=None, residual=None):
    """dx[M,K] = dy[M,N] @ w[N,K]  (+ residual), the NT GEMM against the transposed weight"""
    return ops.gemm(dy2d, transposed_weight(w), out=out, residual=residual)


# ------------------------------------------------------------------------------------------------
# LLaMA decoder layer as ONE autograd node
# ------------------------------------------------------------------------------------------------

class LayerMeta:
    """Geometry shared by all decoder layers of one forward pass."""

    def __init__(self, B, L, Hq, Hkv, d, I, eps, cos, sin, seqlens, recompute=False, pos_offset=None, c2p=None, p2c=None):
        self.B, self.L, self.Hq, self.Hkv, self.d, self.I, self.eps = B, L, Hq, Hkv, d, I, eps
        self.cos, self.sin, self.seqlens = cos, sin, seqlens
        self.pos_offset = pos_offset        # int32 [B] or None: RoPE position of row (b, l) = l + pos_offset[b] (left-padded batches)
        # padding-free rows (ragged batches): the decoder's row-wise work (norms, GEMMs, SwiGLU, residuals) runs on the COMPACT layout --
        # the sum(len) valid rows back to back, rounded up to 256 with zero rows -- and only q|k|v -> attention -> o visits the padded
        # [B, L] layout the attention kernels address (per-sample lengths from row b * L).  c2p int32 [rows]: padded row of every compact
        # row (-1: a zero row of the tail); p2c int32 [B * L]: compact row of every padded row (-1: padding).  None: x IS the padded layout.
        self.c2p, self.p2c = c2p, p2c
        # prompt pass of a cached decode (decoder_prefill sets it): a few hundred rows -- the q|k|v, o and down projections take the split-K
        # GEMM (ops.gemm_splitk); inference only
        self.prompt_pass = False
        self.scale = d ** -0.5
        # gradient checkpointing (reference train.py:1443-1449 + `--gradient_checkpointing True` in every launch script): keep only
        # the layer input, re-run the layer's forward kernels at the start of its backward
        self.recompute = recompute


PROMPT_GU_SPLITK_ROWS = 64


def decoder_layer_forward(x, layer, m: LayerMeta):
    """x [B*L, h] -> (y, saved tensors).  HF LlamaDecoderLayer semantics (reference call site
    metamorph_llama.py:349-359)."""
    att, mlp = layer.self_attn, layer.mlp
    wqkv = fused_weight([att.q_proj.weight, att.k_proj.weight, att.v_proj.weight])
    wgu = fused_weight([mlp.gate_proj.weight, mlp.up_proj.weight])
    n1, rstd1 = ops.rmsnorm_fwd(x, layer.input_layernorm.weight, m.eps, want_rstd=True)
    if m.p2c is None and VARIANTS["fuse_rope"] and ops.gemm_rope_supported(n1, wqkv, m.Hq, m.Hkv, m.d, m.cos):
        qkv = ops.gemm_rope(n1, wqkv, m.B, m.L, m.Hq, m.Hkv, m.d, m.cos, m.sin, pos_offset=m.pos_offset)     # rotation in the GEMM epilogue: same bits
        del n1
    else:
        qkv = ops.gemm_splitk(n1, wqkv) if m.prompt_pass else ops.gemm(n1, wqkv)
        del n1
        if m.p2c is not None:                                  # compact rows -> the padded layout attention addresses (padding rows: zeros)
            qkv = ops.rows_gather(qkv, m.p2c)
        ops.rope_qk_(qkv, m.B, m.L, m.Hq, m.Hkv, m.d, m.cos, m.sin, pos_offset=m.pos_offset)
    nq, nk = m.Hq * m.d, m.Hkv * m.d
    o, lse = ops.attn_fwd(qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:], m.B, m.L, m.Hq, m.Hkv, m.d, m.scale, True, m.seqlens)
    if m.c2p is not None:
        o = ops.rows_gather(o, m.c2p)                          # back to compact rows for o_proj and everything after it
    x2 = ops.gemm_splitk(o, att.o_proj.weight, residual=x) if m.prompt_pass else ops.gemm(o, att.o_proj.weight, residual=x)
    n2, rstd2 = ops.rmsnorm_fwd(x2, layer.post_attention_layernorm.weight, m.eps, want_rstd=True)
    if VARIANTS["fuse_swiglu"] and ops.gemm_swiglu_supported(n2, wgu, m.I):
        gu, act = ops.gemm_swiglu(n2, wgu, m.I)                # SiLU(gate) * up formed in the GEMM epilogue: same bits, one pass less
        del n2
    else:
        # (prompt passes of up to 64 rows: gate|up through the split-K GEMM as well -- 5.65 -> 5.25 ms per 64-row pass; from 128 rows on the
        # plain 128 x 128 tiles are faster)
        gu = ops.gemm_splitk(n2, wgu) if (m.prompt_pass and n2.shape[0] <= PROMPT_GU_SPLITK_ROWS) else ops.gemm(n2, wgu)
        del n2
        act = ops.swiglu_fwd(gu, m.I)
    y = ops.gemm_splitk(act, mlp.down_proj.weight, residual=x2) if m.prompt_pass else ops.gemm(act, mlp.down_proj.weight, residual=x2)
    # rstd1 / rstd2 (fp32 [M] each): the backward pass rebuilds the TRANSPOSED norm outputs from them in one pass (rmsnorm_apply_t)
    return y, (qkv, o, lse, x2, gu, rstd1, rstd2)


def _rmsnorm_backward(dn, x, w, eps, dres):
    """dres + d rmsnorm / dx; the weight gradient (if trained) lands in the parameter's gradient buffer in the same launch pair."""
    if not w.requires_grad:
        return ops.rmsnorm_bwd(dn, x, w, eps, dres=dres, dw_f32=None)
    buf, acc = grad_target(w)
    dx = ops.rmsnorm_bwd_wgrad(dn, x, w, eps, buf, acc, dres=dres)
    commit_grad(w, buf)
    return dx


class DecoderLayerFn(Function):
    @staticmethod
    def forward(ctx, x, layer, meta, *weights):
        y, saved = decoder_layer_forward(x, layer, meta)
        ctx.layer, ctx.meta = layer, meta
        if meta.recompute:
            del saved
            ctx.save_for_backward(x)
        else:
            ctx.save_for_backward(x, *saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        layer, m = ctx.layer, ctx.meta
        params_ready(layer, backward=True)                                     # sharded parameters (ZeRO-3): gather before use
        if len(ctx.saved_tensors) == 1:                                        # checkpointed: same kernels, same inputs => same bits
            (x,) = ctx.saved_tensors
            _, (qkv, o, lse, x2, gu, rstd1, rstd2) = decoder_layer_forward(x, layer, m)
        else:
            x, qkv, o, lse, x2, gu, rstd1, rstd2 = ctx.saved_tensors
        att, mlp = layer.self_attn, layer.mlp
        dy = dy.contiguous()
        h = x.shape[1]
        nq, nk = m.Hq * m.d, m.Hkv * m.d
        dev = x.device

        # ---- MLP ----
        gu_params = [mlp.gate_proj.weight, mlp.up_proj.weight]
        # full fine-tune on whole 64-row tiles: SwiGLU backward writes act^T and dgu^T itself (no transpose passes over them)
        fused_t = (dy.shape[0] % 64 == 0 and m.I % 64 == 0 and mlp.down_proj.weight.requires_grad
                   and all(p.requires_grad for p in gu_params))
        wdT = wdT_made = None
        if fused_t and VARIANTS["fuse_swiglu_bwd"]:
            wdT = wdT_made = transposed_weight(mlp.down_proj.weight, sources=(mlp.down_proj.weight,))
            if not ops.gemm_swiglu_bwd_supported(dy, wdT, gu, m.I):
                wdT = None
        if wdT is not None:
            # d act = dy Wd formed, rounded and consumed in the GEMM's epilogue: same bits as the two launches, no d act round trip
            dgu, actT, dguT = ops.gemm_swiglu_bwd(dy, wdT, gu, m.I)
            act = None
            del wdT
        else:
            dact = ops.gemm(dy, wdT_made) if wdT_made is not None else input_grad_gemm(dy, mlp.down_proj.weight)   # [M, I]
            if fused_t:
                dgu, actT, dguT = ops.swiglu_bwd_t(gu, dact, m.I)
                act = None
            else:
                dgu, act = ops.swiglu_bwd(gu, dact, m.I, want_act=mlp.down_proj.weight.requires_grad)
                actT = dguT = None
            del dact
        qkv_params = [att.q_proj.weight, att.k_proj.weight, att.v_proj.weight]
        held = None                      # down_proj's weight-gradient problem, kept back to share a launch with qkv's
        if mlp.down_proj.weight.requires_grad:
            wd = mlp.down_proj.weight
            buf, acc = grad_target(wd)
            if (all(p.requires_grad for p in qkv_params)
                    and _pair_saves_a_wave(wd.shape[0], wd.shape[1], sum(p.shape[0] for p in qkv_params), h, dy.shape[0])):
                held = _dw_operands(dy, act, xT=actT) + (buf, acc)
            else:
                weight_grad_gemm(dy, act, buf, acc, xT=actT)
            commit_grad(wd, buf)
        del act, actT
        wgu = fused_weight(gu_params)
        dn2 = None
        if any(p.requires_grad for p in gu_params):
            fb, acc, bufs = fused_grad_target(gu_params)
            rp = dguT.shape[1] if dguT is not None else _padded_rows(x2.shape[0], long_k=True)
            n2T = ops.rmsnorm_apply_t(x2, layer.post_attention_layernorm.weight, rstd2, rp)   # norm output, contraction-major, from the saved rstd
            a0, b0 = _dw_operands(dgu, None, dyT=dguT, xT=n2T)
            wguT = transposed_weight(wgu, sources=gu_params)
            if _pairable(a0, b0, dgu, wguT):
                dn2 = torch.empty((dgu.shape[0], wguT.shape[0]), device=dev, dtype=BF16)
                ops.gemm_pair(a0, b0, fb, bool(acc), dgu, wguT, dn2, False)   # the weight gradient's long-K tiles first
            else:
                dn2 = ops.gemm(dgu, wguT)
                ops.gemm(a0, b0, out=fb, accumulate=bool(acc))
            del n2T, a0, b0, wguT
            commit_fused_grad(gu_params, fb, acc, bufs)
        if dn2 is None:
            dn2 = input_grad_gemm(dgu, wgu)                                     # [M, h]
        del dgu, dguT
        dx2 = _rmsnorm_backward(dn2, x2, layer.post_attention_layernorm.weight, m.eps, dy)     # dy + d rmsnorm
        del dn2

        # ---- attention ----
        do = None
        if att.o_proj.weight.requires_grad:
            buf, acc = grad_target(att.o_proj.weight)
            a0, b0 = _dw_operands(dx2, o)
            woT = transposed_weight(att.o_proj.weight, sources=(att.o_proj.weight,))
            if _pairable(a0, b0, dx2, woT):
                do = torch.empty((dx2.shape[0], woT.shape[0]), device=dev, dtype=BF16)
                ops.gemm_pair(a0, b0, buf, acc, dx2, woT, do, False)
            else:
                do = ops.gemm(dx2, woT)
                ops.gemm(a0, b0, out=buf, accumulate=acc)
            del a0, b0, woT
            commit_grad(att.o_proj.weight, buf)
        if do is None:
            do = input_grad_gemm(dx2, att.o_proj.weight)                        # [M, Hq*d]
        dqkv = torch.empty_like(qkv)
        fuse_rope = VARIANTS["fuse_rope"] and ops.attn_bwd_rope_supported(m.d)      # inverse RoPE of dq / dk in the attention kernels' epilogues
        o_att = o
        if m.p2c is not None:                                  # padding-free rows: o / d o to the padded layout (qkv was saved in it)
            o_att, do = ops.rows_gather(o, m.p2c), ops.rows_gather(do, m.p2c)
        ops.attn_bwd(qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:], o_att, do, lse, m.B, m.L, m.Hq, m.Hkv, m.d,
                     m.scale, True, m.seqlens, dqkv[:, :nq], dqkv[:, nq:nq + nk], dqkv[:, nq + nk:],
                     rope=(m.cos, m.sin, m.pos_offset) if fuse_rope else None)
        del do, o_att
        if not fuse_rope:
            ops.rope_qk_(dqkv, m.B, m.L, m.Hq, m.Hkv, m.d, m.cos, m.sin, inverse=True, pos_offset=m.pos_offset)
        if m.c2p is not None:
            dqkv = ops.rows_gather(dqkv, m.c2p)                # gradients of the compact q|k|v rows (tail rows: zeros)
        wqkv = fused_weight(qkv_params)
        dn1 = ops.gemm(dqkv, transposed_weight(wqkv, sources=qkv_params))
        if any(p.requires_grad for p in qkv_params):
            fb, acc, bufs = fused_grad_target(qkv_params)
            n1T = ops.rmsnorm_apply_t(x, layer.input_layernorm.weight, rstd1, _padded_rows(x.shape[0], long_k=True))
            if held is not None:
                a1, b1 = _dw_operands(dqkv, None, xT=n1T)
                if ops.gemm_pair_supported(held[0], held[1], a1, b1):
                    ops.gemm_pair(held[0], held[1], held[2], held[3], a1, b1, fb, bool(acc))
                else:                                                          # e.g. an operand beyond 2 GiB
                    ops.gemm(held[0], held[1], out=held[2], accumulate=held[3])
                    ops.gemm(a1, b1, out=fb, accumulate=bool(acc))
                held = None
                del a1, b1
            else:
                weight_grad_gemm(dqkv, None, fb, bool(acc), xT=n1T)
            commit_fused_grad(qkv_params, fb, acc, bufs)
            del n1T
        del dqkv
        dx = _rmsnorm_backward(dn1, x, layer.input_layernorm.weight, m.eps, dx2)
        if _LAYER_GRAD_HOOK is not None:                                       # every gradient of this layer is final now
            _LAYER_GRAD_HOOK(layer)
        return (dx, None, None) + (None,) * (len(ctx.needs_input_grad) - 3)


def decoder_layer(x, layer, meta):
    params_ready(layer)
    ws = [p for p in layer.parameters()]
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in ws)):
        return DecoderLayerFn.apply(x, layer, meta, *ws)
    return decoder_layer_forward(x, layer, meta)[0]


# ------------------------------------------------------------------------------------------------
# small composable nodes: RMSNorm, Linear(+bias), GELU, row gather, cosine loss
# ------------------------------------------------------------------------------------------------

class RmsNormFn(Function):
    @staticmethod
    def forward(ctx, x, w, eps):
        ctx.save_for_backward(x, w)
        ctx.eps = eps
        return ops.rmsnorm_fwd(x, w.data if isinstance(w, torch.nn.Parameter) else w, eps)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dw = torch.zeros(x.shape[-1], device=x.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        dx = ops.rmsnorm_bwd(dy.contiguous(), x, w, ctx.eps, dres=None, dw_f32=dw)
        dwb = None
        if dw is not None:
            dwb = torch.empty_like(w)
            ops.axpy_(dwb, dw, None, 1.0, False)
        return dx, dwb, None


class LinearFn(Function):
    """y = x W^T (+ b); weight / bias gradients go straight to the parameters' gradient buffers."""

    @staticmethod
    def forward(ctx, x, weight, bias, module):
        ctx.module = module
        ctx.save_for_backward(x)
        return ops.gemm(x, weight, bias=bias)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        mod = ctx.module
        dy = dy.contiguous()
        w, b = mod.weight, mod.bias
        dx = input_grad_gemm(dy, w) if ctx.needs_input_grad[0] else None
        if w.requires_grad:
            buf, acc = grad_target(w)
            weight_grad_gemm(dy, x, buf, acc)
            commit_grad(w, buf)
        if b is not None and b.requires_grad:
            s = torch.zeros(b.shape[0], device=dy.device, dtype=torch.float32)
            ops.colsum_f32(dy, s)
            buf, acc = grad_target(b)
            ops.axpy_(buf, s, None, 1.0, acc)
            commit_grad(b, buf)
        return dx, None, None, None


def _param_grad_f32(p, s_f32):
    """p.grad (+)= s_f32 (an fp32 reduction result such as a bias / norm-weight gradient), into the parameter's gradient buffer."""
    buf, acc = grad_target(p)
    ops.axpy_(buf.view(-1), s_f32.view(-1), None, 1.0, acc)
    commit_grad(p, buf)


def _linear_grads(mod, dy2d, x2d):
    """Weight and bias gradients of y = x W^T + b from dy (may be a strided column block) and the saved input."""
    if mod.weight.requires_grad:
        buf, acc = grad_target(mod.weight)
        weight_grad_gemm(dy2d, x2d, buf, acc)
        commit_grad(mod.weight, buf)
    if mod.bias is not None and mod.bias.requires_grad:
        s = torch.zeros(mod.bias.shape[0], device=dy2d.device, dtype=torch.float32)
        ops.colsum_f32(dy2d, s)
        _param_grad_f32(mod.bias, s)


# ------------------------------------------------------------------------------------------------
# SigLIP encoder with a backward pass (freeze_vision=False, reference siglip_encoder.py:138-141 running HF
# SiglipEncoderLayer under grad).  Coarse nodes like DecoderLayerFn: forward keeps (x, qkv, o, lse, x2, fc1 pre-activation),
# backward recomputes the two LayerNorms and the GELU, parameter gradients go straight to their gradient buffers.
# ------------------------------------------------------------------------------------------------

class SiglipGeo:
    def __init__(self, N, P, heads, d, eps, recompute=False):
        self.N, self.P, self.heads, self.d, self.eps = N, P, heads, d, eps
        self.scale = d ** -0.5
        self.recompute = recompute


def _siglip_qkv(h1, att, hv):
    qkv = torch.empty((h1.shape[0], 3 * hv), device=h1.device, dtype=BF16)
    for i, proj in enumerate((att.q_proj, att.k_proj, att.v_proj)):     # HF stores k, v, q, out separately (with biases)
        ops.gemm(h1, proj.weight.data, out=qkv[:, i * hv:(i + 1) * hv], bias=proj.bias.data)
    return qkv


def siglip_layer_forward(x, layer, g):
    att, mlp = layer.self_attn, layer.mlp
    hv = x.shape[1]
    ln1, ln2 = layer.layer_norm1, layer.layer_norm2
    h1 = ops.layernorm_fwd(x, ln1.weight.data, ln1.bias.data, g.eps)
    qkv = _siglip_qkv(h1, att, hv)
    del h1
    o, lse = ops.attn_fwd(qkv[:, :hv], qkv[:, hv:2 * hv], qkv[:, 2 * hv:], g.N, g.P, g.heads, g.heads, g.d, g.scale, False, None)
    x2 = ops.gemm(o, att.out_proj.weight.data, bias=att.out_proj.bias.data, residual=x)
    h2 = ops.layernorm_fwd(x2, ln2.weight.data, ln2.bias.data, g.eps)
    f_pre = ops.gemm(h2, mlp.fc1.weight.data, bias=mlp.fc1.bias.data)
    del h2
    f = ops.gelu_fwd(f_pre, ops.GELU_TANH)
    y = ops.gemm(f, mlp.fc2.weight.data, bias=mlp.fc2.bias.data, residual=x2)
    return y, (qkv, o, lse, x2, f_pre)


class SiglipLayerFn(Function):
    @staticmethod
    def forward(ctx, x, layer, g, *params):
        y, saved = siglip_layer_forward(x, layer, g)
        ctx.layer, ctx.g = layer, g
        if g.recompute:
            del saved
            ctx.save_for_backward(x)
        else:
            ctx.save_for_backward(x, *saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        layer, g = ctx.layer, ctx.g
        if len(ctx.saved_tensors) == 1:
            (x,) = ctx.saved_tensors
            _, (qkv, o, lse, x2, f_pre) = siglip_layer_forward(x, layer, g)
        else:
            x, qkv, o, lse, x2, f_pre = ctx.saved_tensors
        att, mlp = layer.self_attn, layer.mlp
        ln1, ln2 = layer.layer_norm1, layer.layer_norm2
        hv = x.shape[1]
        dev = x.device
        dy = dy.contiguous()
        # ---- MLP
        f = ops.gelu_fwd(f_pre, ops.GELU_TANH)
        df = input_grad_gemm(dy, mlp.fc2.weight)
        _linear_grads(mlp.fc2, dy, f)
        del f
        dfp = ops.gelu_bwd(f_pre, df, ops.GELU_TANH)
        del df
        h2 = ops.layernorm_fwd(x2, ln2.weight.data, ln2.bias.data, g.eps)
        dh2 = input_grad_gemm(dfp, mlp.fc1.weight)
        _linear_grads(mlp.fc1, dfp, h2)
        del h2, dfp
        dw, db = torch.zeros(hv, device=dev, dtype=torch.float32), torch.zeros(hv, device=dev, dtype=torch.float32)
        dx2 = ops.layernorm_bwd(dh2, x2, ln2.weight.data, g.eps, dw, db, dres=dy)       # dy + d LayerNorm2
        del dh2
        if ln2.weight.requires_grad:
            _param_grad_f32(ln2.weight, dw)
            _param_grad_f32(ln2.bias, db)
        # ---- attention
        do = input_grad_gemm(dx2, att.out_proj.weight)
        _linear_grads(att.out_proj, dx2, o)
        dqkv = torch.empty_like(qkv)
        ops.attn_bwd(qkv[:, :hv], qkv[:, hv:2 * hv], qkv[:, 2 * hv:], o, do, lse, g.N, g.P, g.heads, g.heads, g.d, g.scale, False, None,
                     dqkv[:, :hv], dqkv[:, hv:2 * hv], dqkv[:, 2 * hv:])
        del do
        h1 = ops.layernorm_fwd(x, ln1.weight.data, ln1.bias.data, g.eps)
        dh1 = None
        for i, proj in enumerate((att.q_proj, att.k_proj, att.v_proj)):
            blk = dqkv[:, i * hv:(i + 1) * hv]
            dh1 = input_grad_gemm(blk, proj.weight, residual=dh1)
            _linear_grads(proj, blk, h1)
        del h1, dqkv
        dw, db = torch.zeros(hv, device=dev, dtype=torch.float32), torch.zeros(hv, device=dev, dtype=torch.float32)
        dx = ops.layernorm_bwd(dh1, x, ln1.weight.data, g.eps, dw, db, dres=dx2)
        if ln1.weight.requires_grad:
            _param_grad_f32(ln1.weight, dw)
            _param_grad_f32(ln1.bias, db)
        return (dx, None, None) + (None,) * (len(ctx.needs_input_grad) - 3)


class PatchEmbedFn(Function):
    """Conv2d(kernel = stride = patch) + bias + position embedding as im2col + GEMM; gradients of the three parameters."""

    @staticmethod
    def forward(ctx, images, emb, *params):
        w = emb.patch_embedding.weight
        k = w.shape[1] * w.shape[2] * w.shape[3]
        kp = (k + 7) // 8 * 8
        wpe = torch.zeros((w.shape[0], kp), device=w.device, dtype=BF16)
        wpe[:, :k].copy_(w.data.reshape(w.shape[0], k))
        p = w.shape[2]
        N, _, H, W = images.shape
        P = (H // p) * (W // p)
        cols = ops.im2col_patch(images, p, kp)
        x = ops.gemm(cols, wpe, bias=emb.patch_embedding.bias.data, residual=emb.position_embedding.weight.data, res_row_mod=P)
        ctx.emb, ctx.k, ctx.N, ctx.P = emb, k, N, P
        ctx.save_for_backward(cols)
        return x

    @staticmethod
    def backward(ctx, dy):
        (cols,) = ctx.saved_tensors
        emb, k, N, P = ctx.emb, ctx.k, ctx.N, ctx.P
        dy = dy.contiguous()
        w, b, pos = emb.patch_embedding.weight, emb.patch_embedding.bias, emb.position_embedding.weight
        hv = w.shape[0]
        if w.requires_grad:
            dwp = torch.empty((hv, cols.shape[1]), device=dy.device, dtype=BF16)
            weight_grad_gemm(dy, cols, dwp, False)
            buf, acc = grad_target(w)
            ops.axpy_(buf.view(hv, k), dwp[:, :k].contiguous(), None, 1.0, acc)
            commit_grad(w, buf)
        if b.requires_grad:
            s = torch.zeros(hv, device=dy.device, dtype=torch.float32)
            ops.colsum_f32(dy, s)
            _param_grad_f32(b, s)
        if pos.requires_grad:                                   # every image adds the same table: sum over the images
            s = torch.zeros(P * hv, device=dy.device, dtype=torch.float32)
            ops.colsum_f32(dy.view(N, P * hv), s)
            _param_grad_f32(pos, s)
        return (None, None) + (None,) * (len(ctx.needs_input_grad) - 2)


class BilinearL2NormFn(Function):
    @staticmethod
    def forward(ctx, x, side_in, side_out, normalize):
        ctx.args = (side_in, side_out, normalize)
        ctx.save_for_backward(x)
        return ops.bilinear_l2norm(x, side_in, side_out, normalize)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        side_in, side_out, normalize = ctx.args
        return ops.bilinear_l2norm_bwd(x, dy.contiguous(), side_in, side_out, normalize), None, None, None


def linear(x2d, module):
    if (x2d.shape[0] <= 32 and not (torch.is_grad_enabled() and (x2d.requires_grad or module.weight.requires_grad))
            and ops.gemv_supported(x2d, module.weight.data)):
        # decode shape: a handful of rows, inference only -> stream the weight once (mm355_gemv_bf16)
        return ops.gemv(x2d, module.weight.data, bias=None if module.bias is None else module.bias.data)
    return LinearFn.apply(x2d, module.weight, module.bias, module)


class KVRows:
    """The cached rows of ONE layer, in the cache's format: k / v [sequences, max_len, width] and, fp8_e4m3, their scales [sequences,
    max_len, Hkv] (bf16: None).  The one place that knows the format: every method is the cache operation of that name in `ops`, in the
    format's form (rope_kv_append_ / rope_kv_append_f8_, ...) with the format's tensor group at its place among the arguments; the passes
    hand over everything else.  The op is looked up by name when it is called: tests and tools wrap the names of `ops`."""

    def __init__(self, k, v, k_scale=None, v_scale=None):
        self.k, self.v, self.k_scale, self.v_scale = k, v, k_scale, v_scale
        self.f8 = k_scale is not None
        self.sfx = "_f8" if self.f8 else ""
        self.kv = (k, v, k_scale, v_scale) if self.f8 else (k, v)

    def seq(self, row):
        """the same record narrowed to sequence `row` (the batch dimension stays)"""
        return KVRows(*(t[row:row + 1] for t in self.kv))

    def prefix(self):
        """the rows of sequence 0, [max_len, width] each: where a prefix is stored once (KVCache.set_shared)"""
        return tuple(t[0] for t in self.kv)

    def rope_append_(self, qkv, *args):
        return getattr(ops, f"rope_kv_append{self.sfx}_")(qkv, *args, *self.kv)

    def rope_append_rows_(self, qkv, *args):
        return getattr(ops, f"rope_kv_append_rows{self.sfx}_")(qkv, *args, *self.kv)

    def attn_decode(self, q, *args, **kw):
        return getattr(ops, "attn_decode" + self.sfx)(q, *self.kv, *args, **kw)

    def attn_extend(self, q, *args, **kw):
        return getattr(ops, "attn_extend" + self.sfx)(q, *self.kv, *args, **kw)

    def attn_extend_ragged(self, q, *args, **kw):
        return getattr(ops, "attn_extend_ragged" + self.sfx)(q, *self.kv, *args, **kw)

    def attn_decode_shared(self, q, *args, **kw):
        return getattr(ops, "attn_decode_shared" + self.sfx)(q, *self.prefix(), *self.kv, *args, **kw)

    def attn_extend_shared(self, q, *args, **kw):
        return getattr(ops, "attn_extend_shared" + self.sfx)(q, *self.prefix(), *self.kv, *args, **kw)

    def store_rows(self, k_rows, v_rows, Hkv, d, row0, n, ident=None):
        """Already rotated k / v rows [sequences * n, width] (may be column blocks of a wider tensor) -> rows row0 .. row0 + n - 1 of every
        sequence.  fp8_e4m3: quantised on the way, one launch each.  bf16: ONE sequence with ident = arange(n) int32 as a strided row copy
        with 16-byte vectors (mm355_rows_gather with the identity map: ~3 us; ATen's strided bf16 copy took 28 us per call, 1.3 of the
        10.8 ms of a 512-row prompt pass), ident None: a tensor copy into all sequences."""
        if self.f8:
            ops.kv_quant_f8(k_rows, Hkv, d, self.k, self.k_scale, row0=row0, rows_per_seq=n)
            ops.kv_quant_f8(v_rows, Hkv, d, self.v, self.v_scale, row0=row0, rows_per_seq=n)
        elif ident is not None:
            ops.rows_gather(k_rows, ident, out=self.k[0, row0:row0 + n])
            ops.rows_gather(v_rows, ident, out=self.v[0, row0:row0 + n])
        else:
            self.k[:, row0:row0 + n].copy_(k_rows.view(-1, n, k_rows.shape[1]))
            self.v[:, row0:row0 + n].copy_(v_rows.view(-1, n, v_rows.shape[1]))


class KVCache:
    """Post-RoPE keys and values of every decoder layer for a BATCH of sequences: [layers, batch, max_len, Hkv*d] bf16 each (one sequence:
    batch = 1).  Every row of the batch has its own length; the write positions live on the device as well (pos_dev / len_dev, int32
    [batch]) so that a decode step -- ONE pass over the weights for all rows -- is replayable as a hipGraph.  `rows[i]` is layer i as the
    passes use it (KVRows, made once: the buffers never move)."""

    def __init__(self, n_layers, max_len, width, device, Hq=None, d=None, batch=1, fmt="bf16"):
        if fmt not in ops.KV_FORMATS:
            raise ValueError(f"unknown KV cache format {fmt!r}; known: {', '.join(ops.KV_FORMATS)}")
        self.batch = batch
        self.fmt = fmt
        self.k_scale = self.v_scale = None
        if fmt == "fp8_e4m3":
            # one e4m3 byte per value plus one fp32 scale per head-row (ops.quantize_kv8): (d + 4) / 2d of the bf16 bytes
            if d is None or width % d:
                raise ValueError("an fp8_e4m3 KV cache needs the head size d (its scales are per head-row)")
            self.k = torch.empty((n_layers, batch, max_len, width), device=device, dtype=torch.uint8)
            self.v = torch.empty((n_layers, batch, max_len, width), device=device, dtype=torch.uint8)
            self.k_scale = torch.empty((n_layers, batch, max_len, width // d), device=device, dtype=torch.float32)
            self.v_scale = torch.empty((n_layers, batch, max_len, width // d), device=device, dtype=torch.float32)
        else:
            self.k = torch.empty((n_layers, batch, max_len, width), device=device, dtype=BF16)
            self.v = torch.empty((n_layers, batch, max_len, width), device=device, dtype=BF16)
        self.rows = [KVRows(*(t[i] for t in (self.k, self.v, self.k_scale, self.v_scale) if t is not None)) for i in range(n_layers)]
        self.max_len = max_len
        self.lengths = [0] * batch                                               # host mirror of pos_dev
        self.pos_dev = torch.zeros(batch, device=device, dtype=torch.int32)      # row the next token of sequence b is written to
        self.len_dev = torch.ones(batch, device=device, dtype=torch.int32)       # = pos + 1: rows visible to that token
        self.Hq, self.d = Hq, d
        self.shared_len = 0                                                      # > 0: rows [0, shared_len) of sequence 0 are every sequence's first rows
        self.shared_ws = None
        self.own_block = None                                                    # uint8 [batch, own rows]: the block each own row lives in (beams)
        self.ws = None
        if Hq is not None:                                                       # (sized for the whole batch: beyond 16 rows one attention launch serves all of them)
            self.ws = torch.zeros(int(ops._L().mm355_attn_decode_ws_floats(batch, Hq, d, max_len)), device=device,
                                  dtype=torch.float32)                           # arrival counters start at 0

    @property
    def kv8(self):
        """(k_scale, v_scale) of an fp8_e4m3 cache, None for a bf16 one"""
        return None if self.k_scale is None else (self.k_scale, self.v_scale)

    @property
    def shared(self):
        """(shared_len, workspace of mm355_attn_decode_shared) while the first rows are shared, else None; with a table of own rows
        (set_shared(n, own_rows=...)) it rides along as a third entry"""
        if self.shared_len <= 0:
            return None
        return (self.shared_len, self.shared_ws) if self.own_block is None else (self.shared_len, self.shared_ws, self.own_block)

    def set_shared(self, n, own_rows=None):
        """Declare rows [0, n) of sequence 0 the first n rows of EVERY sequence (n continuations of one prompt: the prompt's rows are stored
        and read once; rows [0, n) of the other sequences' blocks are never read again).  Every sequence must hold at least n rows
        (set_lengths first); n = 0 ends the sharing.  The decode step then attends through mm355_attn_decode_shared.
        own_rows = r (the beams of a beam search): also allocates own_block, uint8 [batch, r], the block in which own row t of sequence b
        lives -- the identity at the start; the step then attends through mm355_attn_decode_shared_idx and whoever permutes the
        sequences (mm355_beam_advance) rewrites the table instead of moving rows."""
        n = int(n)
        self.own_block = None
        if own_rows is not None:
            if n <= 0 or int(own_rows) < 1 or self.batch > 255:
                raise ValueError(f"a table of own rows needs a shared prefix (got {n} rows), at least one column (got {own_rows}) and at "
                                 f"most 255 sequences (got {self.batch}): one byte names a block")
        if n < 0 or n > min(self.lengths):
            raise ValueError(f"shared prefix of {n} rows on sequences of {self.lengths} rows: every sequence must hold the shared rows")
        if n > 0:
            if self.Hq is None or self.d is None:
                raise ValueError("a shared prefix needs a cache built with Hq and d (they size the attention workspace)")
            Hkv = self.k.shape[-1] // self.d
            n_ws = int(ops._L().mm355_attn_decode_shared_ws_floats(self.batch, self.Hq, Hkv, self.d, n, self.max_len))
            if n_ws <= 0:
                raise ValueError(f"mm355_attn_decode_shared has no workspace for batch={self.batch} Hq={self.Hq} Hkv={Hkv} d={self.d}")
            self.shared_ws = torch.empty(n_ws, device=self.k.device, dtype=torch.float32)
            if own_rows is not None:
                self.own_block = torch.arange(self.batch, dtype=torch.uint8).view(-1, 1).repeat(1, int(own_rows)).to(self.k.device)
        else:
            self.shared_ws = None
        self.shared_len = n

    def copy_prefix(self, n):
        """rows [0, n) of sequence 0 (scales included) into every other sequence's block: the fan-out of one prompt to the batch"""
        for t in (self.k, self.v, self.k_scale, self.v_scale):
            if t is not None and self.batch > 1:
                t[:, 1:, :n].copy_(t[:, :1, :n].expand(-1, self.batch - 1, -1, -1))

    def nbytes(self):
        """bytes of the cached rows (and their scales)"""
        return sum(t.numel() * t.element_size() for t in (self.k, self.v, self.k_scale, self.v_scale) if t is not None)

    @property
    def length(self):
        """rows of the longest sequence (= THE length when batch == 1)"""
        return max(self.lengths)

    @length.setter
    def length(self, n):
        self.lengths = [n] * self.batch

    def set_length(self, n, row=None):
        if row is None:
            self.set_lengths([n] * self.batch)
        else:
            ls = list(self.lengths)
            ls[row] = n
            self.set_lengths(ls)

    def set_lengths(self, lengths):
        assert len(lengths) == self.batch
        self.lengths = [int(n) for n in lengths]
        pos = torch.tensor(self.lengths, dtype=torch.int32)
        self.pos_dev.copy_(pos)
        self.len_dev.copy_(pos + 1)


def decoder_prefill(x, layers, meta, cache, row=0):
    """Prompt pass of a cached decode: the training-path layer forward, keeping each layer's post-RoPE k / v rows.
    x [meta.B * L, h] -> hidden rows (pre final norm).  meta.B == 1: the prompt of sequence `row`; meta.B == cache.batch: all sequences
    at once (prompts of ONE length -- the beams of a beam search, a batch without padding)."""
    B = meta.B
    L = x.shape[0] // B
    assert B == 1 or (B == cache.batch and row == 0)
    meta.prompt_pass = VARIANTS["prefill_splitk"] and not torch.is_grad_enabled() and x.shape[0] <= 4096
    ident = torch.arange(L, device=x.device, dtype=torch.int32) if B == 1 else None
    if (B == 1 and meta.prompt_pass and VARIANTS["prefill_fused"] and meta.d % 16 == 0 and meta.pos_offset is None and meta.p2c is None
            and ops.gemm_splitk_splits(L, (meta.Hq + 2 * meta.Hkv) * meta.d, x.shape[1])):
        x = _prefill_layers_fused(x, layers, meta, cache, row, ident)
        cache.set_length(L, row)
        return x
    for i, layer in enumerate(layers):
        params_ready(layer)
        w8_materialize(layer)                                 # (a quantised layer: ALL four projections dequantised into the shared scratch, see W8Scratch -- a one-sequence prompt gets here once q|k|v is no longer split, 960 rows at 8B widths)
        x, saved = decoder_layer_forward(x, layer, meta)
        _store_kv(cache.rows[i].seq(row) if B == 1 else cache.rows[i], saved[0], meta, 0, ident)
        del saved
    if B == 1:
        cache.set_length(L, row)
    else:
        cache.set_length(L)
    return x


def _seq_rows(t, n):
    """Cache rows t [max_len, width] of ONE sequence as the [n, max_len, width] cache operand of a call with n rows: a batch stride of 0,
    every row of the call belongs to this sequence."""
    return t.as_strided((n, t.shape[0], t.shape[1]), (0, t.stride(0), 1))


def _store_kv(rows, qkv, meta, row0, ident=None):
    """the rotated k and the v columns of the new q|k|v rows -> cache rows row0 .. of every sequence of `rows` (KVRows.store_rows)"""
    nq, nk = meta.Hq * meta.d, meta.Hkv * meta.d
    rows.store_rows(qkv[:, nq:nq + nk], qkv[:, nq + nk:], meta.Hkv, meta.d, row0, qkv.shape[0] // rows.k.shape[0], ident)


def _gate_up(on8, rec, mlp, n2, meta, prompt):
    """gate|up + SwiGLU of a fused walk: on the record's bytes where w8_route put it there (a decode step of 17 - 32 rows too: the w8 GEMV has
    no second row group), else the split-K form with SwiGLU in its reduce launch -- but for a prompt-side pass (prefill, extend,
    extend_shared) the ping-pong GEMM with the SwiGLU epilogue where it takes the shape and two launches beyond PROMPT_GU_SPLITK_ROWS rows,
    and for a decode step of up to 32 rows on wide weights the weight stream of the 16-row GEMV, a second x row group on its fragments."""
    if "gu" in on8:
        return rec.gemm_swiglu(n2, *rec.gu, meta.I)
    wgu = fused_weight([mlp.gate_proj.weight, mlp.up_proj.weight])
    if prompt:
        if VARIANTS["fuse_swiglu"] and ops.gemm_swiglu_supported(n2, wgu, meta.I):
            return ops.gemm_swiglu(n2, wgu, meta.I)[1]
        if n2.shape[0] > PROMPT_GU_SPLITK_ROWS:
            return ops.swiglu_fwd(ops.gemm(n2, wgu), meta.I)
    elif VARIANTS["decode_wide_gu_gemv"] and n2.shape[0] <= 32 and meta.I % 2 == 0 and ops.gemv_rows32_units(meta.I // 2):
        return ops.gemv_swiglu(n2, wgu, meta.I)
    return ops.gemm_splitk_swiglu(n2, wgu, meta.I)


def _fused_walk(x, layers, meta, attend, prompt):
    """x [rows, h] through every layer with what follows a split projection in its reduce launch: the input norm as a launch of its own
    for the first layer only, o / down + residual + the RMSNorm that follows (mm355_gemm_splitk_norm_bf16; the last down: the plain split
    projection).  The one step that differs between the passes is the caller's: attend(qkv, i) -> o, where qkv(w8_op, bf16_op, *args) is
    layer i's q|k|v projection of the normed rows (_proj: the plain split projection or the one with RoPE + cache append) and what follows
    it -- rotation, append, attention -- is up to the caller.  prompt: the prompt passes' gate|up rule and row limit, else the decode
    step's.  A quantised layer: w8_route per layer, these projections on the w8 GEMM, the rest dequantised."""
    n1 = None
    for i, layer in enumerate(layers):
        params_ready(layer)
        rec = getattr(layer, "w8", None)
        on8 = w8_route(layer, x.shape[0], PROMPT_GU_SPLITK_ROWS if prompt else None)
        att, mlp = layer.self_attn, layer.mlp
        if n1 is None:
            n1 = ops.rmsnorm_fwd(x, layer.input_layernorm.weight, meta.eps)
        o = attend(lambda w8_op, bf16_op, *args: _proj(on8, rec, "qkv", (att.q_proj.weight, att.k_proj.weight, att.v_proj.weight),
                                                       w8_op, bf16_op, n1, *args), i)
        x2, n2 = _proj(on8, rec, "o", (att.o_proj.weight,), "gemm_norm", ops.gemm_splitk_norm, o,
                       layer.post_attention_layernorm.weight, meta.eps, residual=x)
        act = _gate_up(on8, rec, mlp, n2, meta, prompt)
        if i + 1 < len(layers):
            params_ready(layers[i + 1])                       # (its input norm weight is read by this layer's last launch)
            x, n1 = _proj(on8, rec, "down", (mlp.down_proj.weight,), "gemm_norm", ops.gemm_splitk_norm, act,
                          layers[i + 1].input_layernorm.weight, meta.eps, residual=x2)
        else:
            x = _proj(on8, rec, "down", (mlp.down_proj.weight,), "gemm", ops.gemm_splitk, act, residual=x2)
    return x


def _plain_walk(x, layers, meta, splitk, append_attend):
    """x [rows, h] through every layer on the plain route of decoder_extend / decoder_extend_shared: every norm, the rotation and SwiGLU
    as launches of their own, the projections on the split-K GEMM (`splitk`) or the plain one; a quantised layer on the scratch route, as
    decoder_prefill's plain pass.  append_attend(qkv, i) -> o is the caller's: rotation, append and attention of layer i."""
    mm = ops.gemm_splitk if splitk else ops.gemm
    for i, layer in enumerate(layers):
        params_ready(layer)
        w8_materialize(layer)
        att, mlp = layer.self_attn, layer.mlp
        wqkv = fused_weight([att.q_proj.weight, att.k_proj.weight, att.v_proj.weight])
        wgu = fused_weight([mlp.gate_proj.weight, mlp.up_proj.weight])
        o = append_attend(mm(ops.rmsnorm_fwd(x, layer.input_layernorm.weight, meta.eps), wqkv), i)
        x2 = mm(o, att.o_proj.weight, residual=x)
        n2 = ops.rmsnorm_fwd(x2, layer.post_attention_layernorm.weight, meta.eps)
        if VARIANTS["fuse_swiglu"] and ops.gemm_swiglu_supported(n2, wgu, meta.I):
            _, act = ops.gemm_swiglu(n2, wgu, meta.I)
        else:
            gu = ops.gemm_splitk(n2, wgu) if (splitk and x.shape[0] <= PROMPT_GU_SPLITK_ROWS) else ops.gemm(n2, wgu)
            act = ops.swiglu_fwd(gu, meta.I)
        x = mm(act, mlp.down_proj.weight, residual=x2)
    return x


def _extend_walk(x, layers, meta, append_attend, attend=None):
    """The route of a pass that extends a cache by the rows x [R, h], chosen on R: _fused_walk where the prompt pass's fused walk applies (up
    to 4096 rows, q|k|v split, d % 16 == 0), else _plain_walk.  append_attend(qkv, i) -> o: rotation, append and attention of layer i on
    the projected rows; attend: the fused walk's step where the pass has one of its own (a fused q|k|v form), else the plain split
    projection in front of append_attend."""
    R, h = x.shape
    splitk = VARIANTS["prefill_splitk"] and R <= 4096
    if splitk and VARIANTS["prefill_fused"] and meta.d % 16 == 0 and ops.gemm_splitk_splits(R, (meta.Hq + 2 * meta.Hkv) * meta.d, h):
        return _fused_walk(x, layers, meta, attend or (lambda qkv, i: append_attend(qkv("gemm", ops.gemm_splitk), i)), prompt=True)
    return _plain_walk(x, layers, meta, splitk, append_attend)


def _prefill_layers_fused(x, layers, meta, cache, row, ident):
    """decoder_prefill for one sequence of a few hundred rows on _fused_walk: q|k|v -> RoPE at the row's position -> rotated k and v
    straight into the cache rows (mm355_gemm_splitk_rope_append_bf16 on _seq_rows), attention reads K / V from the cache rows.  The bits of
    decoder_layer_forward's prompt pass (rope_qk_ and rope_kv_append share their arithmetic)."""
    L = x.shape[0]
    nq = meta.Hq * meta.d
    stage = None
    if cache.kv8 is not None:
        # fp8_e4m3 cache: the reduce launch writes the rotated k and the v rows into ONE pair of bf16 staging buffers shared by all layers,
        # attention runs on them (the bits of the bf16-cache pass), then they are quantised into the cache rows
        stage = torch.empty((2, L, meta.Hkv * meta.d), device=x.device, dtype=BF16)

    def attend(qkv, i):
        rows = cache.rows[i].seq(row)
        kc, vc = (stage[0], stage[1]) if stage is not None else (rows.k[0], rows.v[0])   # [max_len, width]
        q = qkv("gemm_rope_append", ops.gemm_splitk_rope_append, meta.Hq, meta.Hkv, meta.d, meta.cos, meta.sin, ident,
                _seq_rows(kc, L), _seq_rows(vc, L))
        o, _ = ops.attn_fwd(q[:, :nq], kc[:L], vc[:L], 1, L, meta.Hq, meta.Hkv, meta.d, meta.scale, True, meta.seqlens)
        if stage is not None:
            rows.store_rows(stage[0], stage[1], meta.Hkv, meta.d, 0, L)
        return o

    return _fused_walk(x, layers, meta, attend, prompt=True)


def decoder_extend(x, layers, meta, cache, row=0):
    """n new rows of sequence `row` on its FILLED cache in one pass over the weights: x [n, h] -> hidden rows [n, h] (pre final norm); the rows
    sit at positions past .. past + n - 1 (past = cache.lengths[row] >= 1) and afterwards cache.lengths[row] == past + n.  A follow-up turn
    of a conversation, a slice of a prompt run in chunks, candidate tokens scored against a cache (then KVCache.set_length back).
    _prefill_layers_fused's walk (_fused_walk) with three differences in its attention step: the positions are past + arange(n), attention
    is mm355_attn_extend over the cache rows (the append comes first), and an fp8_e4m3 cache is read back quantised -- the new rows are
    rotated in the q|k|v activation, quantised into the cache at row past and attended from there: the semantics of n decode steps (every
    row sees the quantised form of all rows, its own included), not of the first prompt pass.  The projections take the prompt pass's
    routes (w8_route, W8Scratch, the split-K limits); where the fused walk does not apply (more than 4096 rows, q|k|v not split,
    d % 16 != 0) the plain route (_plain_walk) with mm355_rope_qk_pos and a row copy into the cache (_extend_walk)."""
    n = x.shape[0]
    if cache.shared_len > 0:
        raise ValueError(f"decoder_extend on a cache with a shared prefix of {cache.shared_len} rows: sequences 1.. do not hold the prefix "
                         "(only sequence 0 stores it), so their rows cannot be extended in place")
    past = int(cache.lengths[row])
    if past < 1:
        raise ValueError(f"decoder_extend needs a filled cache, sequence {row} holds no rows: the first rows of a sequence go through decoder_prefill")
    if past + n > cache.max_len:
        raise ValueError(f"KV cache capacity of {cache.max_len} rows is too small for {past} cached + {n} new rows")
    if torch.is_grad_enabled():
        raise RuntimeError("decoder_extend is an inference pass (torch.no_grad())")
    H = (meta.Hq, meta.Hkv, meta.d)
    nq = meta.Hq * meta.d
    bound = past + n
    ident = torch.arange(n, device=x.device, dtype=torch.int32)
    pos = ident + past
    past_dev = pos[:1]

    def append_attend(qkv, i):                                # rotation in place, (quantising) append, attention over the cache rows
        rows = cache.rows[i].seq(row)
        ops.rope_qk_(qkv, 1, n, *H, meta.cos, meta.sin, pos_offset=past_dev)
        _store_kv(rows, qkv, meta, past, ident)
        return rows.attn_extend(qkv[:, :nq], past_dev, n, bound, *H, meta.scale)

    def attend(qkv, i):
        if cache.kv8 is not None:                             # plain split projection, then as the plain route (no fused f8 form)
            return append_attend(qkv("gemm", ops.gemm_splitk), i)
        rows = cache.rows[i].seq(row)
        q = qkv("gemm_rope_append", ops.gemm_splitk_rope_append, *H, meta.cos, meta.sin, pos, _seq_rows(rows.k[0], n), _seq_rows(rows.v[0], n))
        return rows.attn_extend(q[:, :nq], past_dev, n, bound, *H, meta.scale)

    x = _extend_walk(x, layers, meta, append_attend, attend)
    cache.set_length(past + n, row)
    return x


def decoder_extend_shared(x, layers, meta, cache, past=None):
    """n new rows of EACH of the B = cache.batch sequences of a cache with a shared prefix (KVCache.set_shared) in ONE pass over the weights:
    x [B, n, h] -> hidden rows [B, n, h] (pre final norm).  Row (b, i) sits at position past[b] + i (past: a list of B ints, default
    cache.lengths; past[b] >= cache.shared_len) and attends the shared rows and then rows [shared_len, past[b] + i] of block b; afterwards
    cache.lengths[b] == past[b] + n.  B different questions over one context: the pass between the prefix and the decode loop.
    decoder_extend's two routes and its projection routing (w8_route, W8Scratch, the split-K limits, on the row count B * n) with three
    differences: the positions are per row (mm355_rope_qk_pos with B sequences of n rows); the append goes into block b per sequence (one
    launch per tensor where all sequences start at the same row, else sequence by sequence), so q|k|v is always the plain split
    projection + rotation + append that decoder_extend takes on an fp8_e4m3 cache (the fused reduce launch cannot name a block per row);
    attention is mm355_attn_extend_shared.  An fp8_e4m3 cache is read back quantised, as decoder_extend reads it.
    Sequences of unequal length: right-pad x with zero rows to the longest and set_lengths afterwards.  Rows are independent outside
    attention and attention is causal over the own rows, so a valid row never sees a padding row; the padding rows' K / V land at own rows
    beyond the sequence's length, where no kernel reads them before a later append overwrites them."""
    if x.dim() != 3 or x.shape[0] != cache.batch:
        raise ValueError(f"decoder_extend_shared takes x [batch, n, h] with batch = {cache.batch} sequences, got {tuple(x.shape)}")
    B, n, h = x.shape
    S = cache.shared_len
    if S <= 0:
        raise ValueError("decoder_extend_shared needs a cache with a shared prefix (KVCache.set_shared); without one the pass is decoder_extend")
    past = [int(p) for p in (cache.lengths if past is None else past)]
    if len(past) != B or min(past) < S:
        raise ValueError(f"decoder_extend_shared: new rows at {past} on a shared prefix of {S} rows: every sequence's own rows begin at or "
                         "after the shared rows")
    if max(past) + n > cache.max_len:
        raise ValueError(f"KV cache capacity of {cache.max_len} rows is too small for {max(past)} cached + {n} new rows")
    if torch.is_grad_enabled():
        raise RuntimeError("decoder_extend_shared is an inference pass (torch.no_grad())")
    x = x.reshape(B * n, h)
    H = (meta.Hq, meta.Hkv, meta.d)
    nq = meta.Hq * meta.d
    bound = max(past) + n
    ident = torch.arange(n, device=x.device, dtype=torch.int32)
    past_dev = torch.tensor(past, dtype=torch.int32).to(x.device)
    n_ws = int(ops._L().mm355_attn_extend_shared_ws_floats(B, n, *H, S, bound))
    ws = torch.empty(max(n_ws, 4), device=x.device, dtype=torch.float32)

    def append_attend(qkv, i):
        rows = cache.rows[i]
        ops.rope_qk_(qkv, B, n, *H, meta.cos, meta.sin, pos_offset=past_dev)
        if len(set(past)) > 1:
            for b in range(B):
                _store_kv(rows.seq(b), qkv[b * n:(b + 1) * n], meta, past[b], ident)
        else:
            _store_kv(rows, qkv, meta, past[0])
        return rows.attn_extend_shared(qkv[:, :nq], past_dev, n, S, bound, *H, meta.scale, workspace=ws)

    x = _extend_walk(x, layers, meta, append_attend)
    cache.set_lengths([p + n for p in past])
    return x.view(B, n, h)


RaggedRowsPlan = namedtuple("RaggedRowsPlan", "row_start positions blocks past n_max bound")


def ragged_rows_plan(lens, past, rows):
    """The tables of one packed pass (host, numpy): sequence rows[j] of a cache holds past[j] rows and brings lens[j] >= 1 new ones.  The
    packed rows stand in BLOCK order (the sequences sorted by rows[j]), as mm355_attn_extend_ragged's non-decreasing table needs them.
    With B = max(rows) + 1 blocks and R = sum(lens) rows -> row_start int32 [B + 1] (a block that is not named brings no row), past int32 [B]
    (0 for such a block), positions int32 [R] (past + i of the row's sequence: its RoPE position and its cache row), blocks int32 [R] (its
    block), n_max = max(lens) and bound = max(past[j] + lens[j]), the two host bounds of the launch."""
    lens, past, rows = [int(n) for n in lens], [int(p) for p in past], [int(b) for b in rows]
    if not lens or len(past) != len(lens) or len(rows) != len(lens):
        raise ValueError(f"ragged_rows_plan: {len(lens)} row counts, {len(past)} cached lengths and {len(rows)} sequences: one of each per entry, at least one entry")
    if min(lens) < 1:
        raise ValueError(f"ragged_rows_plan: an entry without new rows ({lens}): leave the sequence out instead")
    if min(past) < 0 or min(rows) < 0 or len(set(rows)) != len(rows):
        raise ValueError(f"ragged_rows_plan: sequences {rows} holding {past} rows: distinct sequences, no negative index or length")
    B = max(rows) + 1
    n_b, past_b = np.zeros(B, np.int64), np.zeros(B, np.int32)
    n_b[rows], past_b[rows] = lens, past
    row_start = np.zeros(B + 1, np.int64)
    np.cumsum(n_b, out=row_start[1:])
    blocks = np.repeat(np.arange(B, dtype=np.int32), n_b)
    positions = (np.arange(row_start[-1]) - row_start[blocks] + past_b[blocks]).astype(np.int32)
    return RaggedRowsPlan(row_start.astype(np.int32), positions, blocks, past_b, max(lens), max(p + n for p, n in zip(past, lens)))


def ragged_pass_supported(meta):
    """the head shapes decoder_extend_ragged takes: those of mm355_attn_extend_ragged with d % 16 == 0 (mm355_rope_kv_append_rows)"""
    return ops.attn_extend_ragged_supported(meta.Hq, meta.Hkv, meta.d) and meta.d % 16 == 0


def decoder_extend_ragged(xs, layers, meta, cache, rows=None):
    """New rows of SEVERAL sequences of one cache, a different number each, in ONE pass over the weights: xs = a list of [n_j, h] bf16
    tensors, n_j >= 1, the new rows of the distinct sequences rows[j] (default: all sequences, in order) -> their hidden rows (pre final
    norm), one [n_j, h] tensor each.  Sequence rows[j] holds past_j = cache.lengths[rows[j]] rows -- 0 is allowed: a prompt -- and
    afterwards past_j + n_j.  A ragged batch of prompts, or the follow-up turns of a batch.
    The sum(n_j) rows run packed, without padding rows (ragged_rows_plan), through decoder_extend_shared's two routes, chosen and routed
    (w8_route, W8Scratch, the split-K limits) on the packed row count; the attention step is the plain split projection, ONE
    mm355_rope_kv_append_rows launch (RoPE at the row's position, k and v into its row of its block) and ONE mm355_attn_extend_ragged call
    over the cache, which then holds the new rows; the workspace is made once per pass.  An fp8_e4m3 cache is read back quantised, as
    decoder_extend reads it: every row sees the quantised form of all rows, its own included.  A PROMPT on this route therefore has the
    semantics of the later slices of decoder_prefill_chunked, not of decoder_prefill, whose rows attend the unquantised K / V of the
    pass; on a bf16 cache the two agree up to the order of the sums."""
    xs = list(xs)
    rows = list(range(cache.batch)) if rows is None else [int(b) for b in rows]
    if cache.shared_len > 0:
        raise ValueError(f"decoder_extend_ragged on a cache with a shared prefix of {cache.shared_len} rows: sequences 1.. do not hold the "
                         "prefix; their own rows go through decoder_extend_shared")
    if not xs or len(xs) != len(rows):
        raise ValueError(f"decoder_extend_ragged: {len(xs)} row blocks for {len(rows)} sequences")
    if len(set(rows)) != len(rows) or min(rows) < 0 or max(rows) >= cache.batch:
        raise ValueError(f"decoder_extend_ragged: sequences {rows} of a cache of {cache.batch}: distinct sequences of the cache")
    h = xs[0].shape[-1]
    if any(x.dim() != 2 or x.shape[0] < 1 or x.shape[1] != h or x.dtype != BF16 for x in xs):
        raise ValueError(f"decoder_extend_ragged takes [n_j, {h}] bf16 tensors with n_j >= 1, got {[(tuple(x.shape), x.dtype) for x in xs]}")
    if not ragged_pass_supported(meta):
        raise ValueError(f"decoder_extend_ragged: no kernel for Hq={meta.Hq} Hkv={meta.Hkv} d={meta.d} (ops.attn_extend_ragged_supported, "
                         "d % 16 == 0)")
    lens = [int(x.shape[0]) for x in xs]
    plan = ragged_rows_plan(lens, [cache.lengths[b] for b in rows], rows)
    if plan.bound > cache.max_len:
        raise ValueError(f"KV cache capacity of {cache.max_len} rows is too small for {plan.bound} rows (cached + new) of one sequence")
    if torch.is_grad_enabled():
        raise RuntimeError("decoder_extend_ragged is an inference pass (torch.no_grad())")
    dev = xs[0].device
    x = torch.cat([xs[j] for j in sorted(range(len(rows)), key=rows.__getitem__)], 0)      # block order
    R = x.shape[0]
    B = plan.past.shape[0]
    tables = torch.from_numpy(np.concatenate([plan.row_start, plan.past, plan.positions, plan.blocks])).to(dev)      # one copy
    row_start, past_dev, pos, blk = tables[:B + 1], tables[B + 1:2 * B + 1], tables[2 * B + 1:2 * B + 1 + R], tables[2 * B + 1 + R:]
    H = (meta.Hq, meta.Hkv, meta.d)
    nq = meta.Hq * meta.d
    n_ws = int(ops._L().mm355_attn_extend_ragged_ws_floats(B, plan.n_max, *H, plan.bound))
    ws = torch.empty(max(n_ws, 4), device=dev, dtype=torch.float32)

    def append_attend(qkv, i):                                # rotation + (quantising) append per row, attention over the cache rows
        cache.rows[i].rope_append_rows_(qkv, *H, meta.cos, meta.sin, pos, blk)
        return cache.rows[i].attn_extend_ragged(qkv[:, :nq], past_dev, row_start, plan.n_max, plan.bound, *H, meta.scale, workspace=ws)

    x = _extend_walk(x, layers, meta, append_attend)
    new = list(cache.lengths)
    for b, n in zip(rows, lens):
        new[b] += n
    cache.set_lengths(new)
    return [x[int(plan.row_start[b]):int(plan.row_start[b]) + n] for b, n in zip(rows, lens)]


def decoder_prefill_chunked(x, layers, meta, cache, chunk, row=0):
    """decoder_prefill of one sequence in slices of `chunk` rows: the first through decoder_prefill, every further one (the last may be short)
    through decoder_extend against the rows cached so far.  Bounds the live activations by the slice, and keeps a quantised decoder on the w8
    split-K GEMM where the whole prompt would leave it (W8Scratch).  An fp8_e4m3 cache: the slices after the first read the cache quantised.
    chunk None: not chunked, decoder_prefill as it is."""
    if chunk is None:
        return decoder_prefill(x, layers, meta, cache, row)
    L = x.shape[0]
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"prefill chunk of {chunk} rows: need at least 1")
    if L <= chunk:
        return decoder_prefill(x, layers, meta, cache, row)
    assert meta.B == 1
    head = LayerMeta(1, chunk, meta.Hq, meta.Hkv, meta.d, meta.I, meta.eps, meta.cos, meta.sin, None)
    outs = [decoder_prefill(x[:chunk].contiguous(), layers, head, cache, row)]
    for r0 in range(chunk, L, chunk):
        outs.append(decoder_extend(x[r0:min(L, r0 + chunk)].contiguous(), layers, meta, cache, row))
    return torch.cat(outs, 0)


class W8Scratch:
    """ONE layer's fused projections as bf16, shared by every quantised layer of a model (W8Layer and W4Layer alike): a projection whose
    route has no kernel on the quantised bytes is dequantised into it (one mm355_dequant_w8_bf16 / mm355_dequant_w4_bf16 launch, a write +
    read of its bf16 weights on top of the GEMM) and takes the existing bf16 GEMM from there.  Correct and not fast.  Since mm355_gemm_w8*
    and mm355_gemm_w4* that is: the batched prompt pass of all sequences at once
    (decoder_layer_forward), passes of more than 4096 rows, the prompt pass's gate|up above PROMPT_GU_SPLITK_ROWS rows (the ping-pong
    gemm_swiglu), every projection at a row count where the split-K GEMM does not split it (W8_GEMM_UNSPLIT_MAX_ROWS / W4_GEMM_UNSPLIT_MAX_ROWS: at 8B widths a
    one-sequence prompt's q|k|v beyond 960 rows -- decoder_prefill then runs the WHOLE pass on this route; any projection too narrow
    to be split), and everything while the format's switch (VARIANTS["w8_gemm"], VARIANTS["w4_gemm"]) is off.  A buffer is allocated when
    its projection first takes this route: `bufs` stays None on a model whose steps all run on the bytes."""

    def __init__(self):
        self.bufs = None

    def view(self, rec, name):
        if self.bufs is None:
            self.bufs = {}
        shape = rec.shape(name)
        buf = self.bufs.get(name)
        if buf is None or tuple(buf.shape) != shape:
            buf = self.bufs[name] = torch.empty(shape, device=rec.qkv[0].device, dtype=BF16)
        return buf


class W8Layer:
    """The quantised fused weights of one decoder layer (format "fp8_e4m3": ops.quantize_w8): q|k|v, o, gate|up, down, each as
    (bytes uint8 [N, K], scale f32 [N]) -- the FUSED matrices, as fused_weight concatenates them.  `released`: the layer's bf16 projection
    parameters no longer hold storage of their own (they alias the model's W8Scratch while a scratch route runs)."""
    NAMES = ("qkv", "o", "gu", "down")
    ON_GEMM = True                                           # the format has a split-K GEMM on its bytes (mm355_gemm_w8*)
    GEMM_SWITCH = "w8_gemm"                                  # the VARIANTS switch of that GEMM; its row caps: gemm_caps()
    gemv, gemv_swiglu, gemv_rope_append, dequant = (staticmethod(f) for f in (ops.gemv_w8, ops.gemv_swiglu_w8, ops.gemv_rope_append_w8,
                                                                                ops.dequant_w8))
    gemm, gemm_norm, gemm_swiglu, gemm_rope_append, gemm_supported = (staticmethod(f) for f in (
        ops.gemm_w8, ops.gemm_w8_norm, ops.gemm_w8_swiglu, ops.gemm_w8_rope_append, ops.gemm_w8_supported))

    @staticmethod
    def gemm_caps():
        """(split, unsplit) row-cap tables of the format's GEMM, read when asked: tools and tests patch the module's tables."""
        return W8_GEMM_MAX_ROWS, W8_GEMM_UNSPLIT_MAX_ROWS

    @staticmethod
    def quantize(w, pow2_scales):
        return ops.quantize_w8(w, pow2_scales)

    def __init__(self, layer, scratch, pow2_scales=False, keep_bf16=False):
        att, mlp = layer.self_attn, layer.mlp
        self.params = {"qkv": [att.q_proj.weight, att.k_proj.weight, att.v_proj.weight], "o": [att.o_proj.weight],
                       "gu": [mlp.gate_proj.weight, mlp.up_proj.weight], "down": [mlp.down_proj.weight]}
        self.rows = {n: [p.shape[0] for p in ps] for n, ps in self.params.items()}
        for n in self.NAMES:
            setattr(self, n, self.quantize(torch.cat([p.data for p in self.params[n]], 0), pow2_scales))
        self.scratch = scratch
        self.released = not keep_bf16
        for ps in self.params.values():
            for p in ps:
                p.w8_quantized = True
        if self.released:
            for ps in self.params.values():
                for p in ps:
                    p.data = p.data.new_empty((0, p.shape[1]))
                    p.requires_grad_(False)

    def shape(self, name):
        """(N, K) of the fused weight `name`."""
        return (sum(self.rows[name]), self.params[name][0].shape[1])

    def materialize(self, names=NAMES):
        """The projections `names` of this layer as bf16 for a route without w8 kernels (see W8Scratch), one matrix at a time: a projection
        that runs on its bytes is not dequantised.  A layer that kept its bf16 parameters runs on them."""
        if not self.released:
            return
        for n in names:
            buf = self.scratch.view(self, n)
            self.dequant(*getattr(self, n), out=buf)
            off = 0
            for p, rows in zip(self.params[n], self.rows[n]):
                p.data = buf[off:off + rows]
                off += rows


class W4Layer(W8Layer):
    """W8Layer in format "mxfp4" (ops.quantize_w4): each fused matrix as (nibbles uint8 [N, K/2], e8m0 group scales uint8 [N, K/32]).
    Decode steps of up to 16 rows run on the mm355_gemv*_w4 kernels; wider steps, one-sequence prompt passes and decoder_extend run the
    projections that the split-K GEMM splits on mm355_gemm_w4* (the nibbles streamed once; the bits of the bf16 split-K GEMM on the
    dequantised weight, so switching VARIANTS["w4_gemm"] changes no result) up to the row caps W4_GEMM_MAX_ROWS /
    W4_GEMM_UNSPLIT_MAX_ROWS -- 0 until measured, see there.  What the caps leave out dequantises into the W8Scratch
    (mm355_dequant_w4_bf16, exact) and runs the bf16 GEMMs."""
    ON_GEMM = True                                           # mm355_gemm_w4*
    GEMM_SWITCH = "w4_gemm"
    gemv, gemv_swiglu, gemv_rope_append, dequant = (staticmethod(f) for f in (ops.gemv_w4, ops.gemv_swiglu_w4, ops.gemv_rope_append_w4,
                                                                                ops.dequant_w4))
    gemm, gemm_norm, gemm_swiglu, gemm_rope_append, gemm_supported = (staticmethod(f) for f in (
        ops.gemm_w4, ops.gemm_w4_norm, ops.gemm_w4_swiglu, ops.gemm_w4_rope_append, ops.gemm_w4_supported))

    @staticmethod
    def gemm_caps():
        return W4_GEMM_MAX_ROWS, W4_GEMM_UNSPLIT_MAX_ROWS

    @staticmethod
    def quantize(w, pow2_scales):                            # (the group scales are powers of two by format: pow2_scales has no effect)
        return ops.quantize_w4(w)


def refuse_w8_params(params, who):
    """Parameters of a decoder quantised with quantize_decoder_ cannot be trained or sharded: refused by name."""
    flat = [p for g in params for p in (g["params"] if isinstance(g, dict) else [g])]
    if any(getattr(p, "w8_quantized", False) for p in flat):
        raise RuntimeError(f"{who}: the decoder was quantised with quantize_decoder_ (weight-only FP8 / MXFP4 are inference formats); "
                           "ZeRO wrapping and training of quantised weights are not supported")


def w8_materialize(layer):
    rec = getattr(layer, "w8", None)
    if rec is not None:
        rec.materialize()


# Which projection of a quantised layer takes the w8 GEMM up to how many rows (the rest: W8Scratch), from profiles/decode_w8_wide.json
# (tools/bench_wide_w8.py).  "split": row counts at which the split-K GEMM cuts the projection into K slices -- the
# captured step of 17 / 32 / 64 sequences runs 2.3 - 2.6 x faster than on the scratch route and every split launch is ahead of
# dequantise + bf16 GEMM, so these go to the w8 GEMM up to its limit of 4096 rows.  "unsplit": row counts at which it does not (at 8B widths
# q|k|v beyond ~960 rows, o and down beyond ~1500, gate|up beyond ~200; any small projection) -- the w8 kernel then runs as one slice of
# 64 x 128 tiles against the large-tile bf16 kernels on the dequantised weight: that pair is in the
# tool's per-launch table (w8 against dequantise + bf16 GEMM at 512 / 1024 / 2048 rows), but no MI355X run of it is recorded with this change
# (measured: not yet), so unsplit projections stay on the scratch route (0 rows).  decoder_prefill leaves the per-projection loop once q|k|v is
# no longer split: a one-sequence prompt of 8B widths runs q|k|v, o and down on their bytes up to 960 rows (gate|up up to
# PROMPT_GU_SPLITK_ROWS) and WHOLLY on the scratch route beyond 960 rows.
W8_GEMM_MAX_ROWS = {"qkv": 4096, "o": 4096, "gu": 4096, "down": 4096}
W8_GEMM_UNSPLIT_MAX_ROWS = {"qkv": 0, "o": 0, "gu": 0, "down": 0}

# The same two tables for format "mxfp4" (mm355_gemm_w4*; tools/bench_wide_w4.py writes profiles/decode_w4_wide.json).
# An entry stays above 0 only where the w4 GEMM is ahead of the scratch route of the same run by more than the larger spread.  No MI355X
# run of the tool is recorded with this change (measured: not yet) -- the captured-step comparison at 17 sequences was not taken -- so by
# the rule for unmeasured shapes the split caps are 0 as well: a w4 model keeps the scratch route until the tool has run, and the caps then
# go to 4096 for every projection it shows ahead.  tests/test_w4_gemm_gpu.py runs the routes with the caps patched to 4096 / 0.
W4_GEMM_MAX_ROWS = {"qkv": 0, "o": 0, "gu": 0, "down": 0}
W4_GEMM_UNSPLIT_MAX_ROWS = {"qkv": 0, "o": 0, "gu": 0, "down": 0}


def w8_on_gemm(layer, rows, gu_rows=None):
    """The projections of `layer` that run on their quantised bytes at `rows` rows (W8Layer: mm355_gemm_w8*, W4Layer: mm355_gemm_w4*), as a
    set of W8Layer.NAMES, by the switch and the row caps of the record's own format.  gu_rows: the caller's own row limit for gate|up on a
    GEMM of 64 x 128 tiles (the prompt pass: PROMPT_GU_SPLITK_ROWS).  Empty for a layer that is not quantised."""
    rec = getattr(layer, "w8", None)
    on8 = set()
    if rec is not None and rec.ON_GEMM and VARIANTS[rec.GEMM_SWITCH]:
        split, unsplit = rec.gemm_caps()
        for n in W8Layer.NAMES:
            N, K = rec.shape(n)
            cap = (split if ops.gemm_splitk_splits(rows, N, K) else unsplit)[n]
            if n == "gu" and gu_rows is not None:
                cap = min(cap, gu_rows)
            if rows <= cap and rec.gemm_supported(rows, K):
                on8.add(n)
    return frozenset(on8)


def w8_route(layer, rows, gu_rows=None):
    """w8_on_gemm(), and the other projections of a quantised layer dequantised into the scratch buffer here."""
    on8 = w8_on_gemm(layer, rows, gu_rows)
    rec = getattr(layer, "w8", None)
    if rec is not None:
        rec.materialize([n for n in W8Layer.NAMES if n not in on8])
    return on8


def _proj(on8, rec, name, weights, w8_op, bf16_op, x, *args, **kw):
    """One projection of a layer through the record's own GEMM op `w8_op` ("gemm", "gemm_norm", "gemm_rope_append": W8Layer on its e4m3
    bytes, W4Layer on its nibbles) where w8_route put it there, else through the bf16 op on the (fused) bf16 weight: the two ops of a pair
    take the same arguments after the weight."""
    if name in on8:
        return getattr(rec, w8_op)(x, *getattr(rec, name), *args, **kw)
    return bf16_op(x, weights[0] if len(weights) == 1 else fused_weight(weights), *args, **kw)


def _attend_decode(q, rows, meta, cache, kv_bound):
    """Attention of the step's new rows (one per sequence, already appended) over `rows`, one layer of the cache: every sequence over its own
    rows (mm355_attn_decode), or, on a cache whose first rows are shared (KVCache.set_shared), over rows [0, shared_len) of sequence 0 and
    then its own rows (mm355_attn_decode_shared); with the cache's table own_block, which says in which block each own row lives,
    mm355_attn_decode_shared_idx."""
    H = (meta.Hq, meta.Hkv, meta.d, meta.scale)
    if cache.shared_len > 0:
        tbl = {} if cache.own_block is None else {"own_block": cache.own_block}
        return rows.attn_decode_shared(q, cache.len_dev, cache.shared_len, kv_bound, *H, workspace=cache.shared_ws, **tbl)
    return rows.attn_decode(q, cache.len_dev, kv_bound, *H, workspace=cache.ws)


def _append_attend(qkv, rows, meta, cache, cos, sin, kv_bound):
    """The step's new q|k|v rows against `rows`: RoPE + (quantising) append, then attention over the cache -- the row just appended
    included.  Two launches; the projection in front is the plain one."""
    rows.rope_append_(qkv, meta.Hq, meta.Hkv, meta.d, cos, sin, cache.pos_dev)
    return _attend_decode(qkv[:, :meta.Hq * meta.d], rows, meta, cache, kv_bound)


_Rows16 = namedtuple("_Rows16", "gemv gemv_swiglu gemv_rope_append qkv o gu down")


def _bf16_rows16(layer):
    """A bf16 layer in the shape of a W8Layer record, as _decode_rows16 reads one: the GEMVs and each fused projection as the operands
    behind x (here the weight alone).  Built per layer and step: fused_weight and the parameters are asked for when the layer runs
    (parameter generations, the ZeRO hooks), and the ops are read from `ops` then (tests and tools wrap them there)."""
    att, mlp = layer.self_attn, layer.mlp
    return _Rows16(ops.gemv, ops.gemv_swiglu, ops.gemv_rope_append,
                   (fused_weight([att.q_proj.weight, att.k_proj.weight, att.v_proj.weight]),), (att.o_proj.weight,),
                   (fused_weight([mlp.gate_proj.weight, mlp.up_proj.weight]),), (mlp.down_proj.weight,))


def _decode_rows16(x, layers, meta, cache, cos, sin, kv_bound):
    """<= 16 new rows (one per sequence) through every decoder layer against their cache rows (cache.rows[i]):
    every weight is streamed ONCE for all rows (mm355_gemv* take M <= 16: up to four rows on the vector ALU, 5 .. 16 on MFMA), attention per
    row at its own length.  One launch sequence for every weight format: a quantised layer runs it on its record's own kernels (W8Layer:
    mm355_gemv*_w8, W4Layer: mm355_gemv*_w4), a bf16 layer on mm355_gemv*_bf16 through _bf16_rows16."""
    nq = meta.Hq * meta.d
    fused = VARIANTS["decode_fused"] and meta.I % 2 == 0 and meta.d % 4 == 0
    for i, layer in enumerate(layers):
        rows = cache.rows[i]
        rec = getattr(layer, "w8", None)
        if rec is None:
            params_ready(layer)
            rec = _bf16_rows16(layer)
        if fused:
            # five launches per layer: RMSNorm folded into the q|k|v and gate|up GEMVs' operand reads, RoPE + cache append and SwiGLU into
            # their epilogues, the flash-decoding merge into the chunk that finishes last (same bits as the nine-launch sequence below).
            # Five rows and more (the MFMA GEMVs): the norm runs as its own launch -- folded in, every workgroup would normalise ALL rows again
            # (measured, cached step of 32 layers: four rows 3.50 -> 3.38 ms with the norms folded, eight rows slower) -- seven launches, same bits.
            fold = x.shape[0] <= VARIANTS["decode_fold_rows"]
            if cache.kv8 is not None:
                # fp8_e4m3 cache: the norm and the plain projection as launches of their own (no fused *_rope_append_f8 form), then the
                # quantising append and attention over the bytes: seven launches per layer up to the fold limit, eight beyond
                qkv = rec.gemv(ops.rmsnorm_fwd(x, layer.input_layernorm.weight, meta.eps), *rec.qkv)
                o = _append_attend(qkv, rows, meta, cache, cos, sin, kv_bound)
            else:
                n1 = x if fold else ops.rmsnorm_fwd(x, layer.input_layernorm.weight, meta.eps)
                qkv = rec.gemv_rope_append(n1, *rec.qkv, meta.Hq, meta.Hkv, meta.d, cos, sin, cache.pos_dev, rows.k, rows.v,
                                           norm_w=layer.input_layernorm.weight if fold else None, eps=meta.eps)
                o = _attend_decode(qkv[:, :nq], rows, meta, cache, kv_bound)
            x2 = rec.gemv(o, *rec.o, residual=x)
            n2 = x2 if fold else ops.rmsnorm_fwd(x2, layer.post_attention_layernorm.weight, meta.eps)
            act = rec.gemv_swiglu(n2, *rec.gu, meta.I, norm_w=layer.post_attention_layernorm.weight if fold else None, eps=meta.eps)
            x = rec.gemv(act, *rec.down, residual=x2)
            continue
        x = _rows16_unfused(x, layer, rec, meta, lambda qkv: _append_attend(qkv, rows, meta, cache, cos, sin, kv_bound))
    return x


def _rows16_unfused(x, layer, rec, meta, append_attend):
    """One layer of the 16-row GEMV route with every norm, the attention step and SwiGLU as launches of their own (nine and more per
    layer); rec: the layer's W8Layer record or _bf16_rows16(layer); append_attend(qkv) -> o is the caller's attention step."""
    n1 = ops.rmsnorm_fwd(x, layer.input_layernorm.weight, meta.eps)
    o = append_attend(rec.gemv(n1, *rec.qkv))
    x2 = rec.gemv(o, *rec.o, residual=x)
    n2 = ops.rmsnorm_fwd(x2, layer.post_attention_layernorm.weight, meta.eps)
    act = ops.swiglu_fwd(rec.gemv(n2, *rec.gu), meta.I)
    return rec.gemv(act, *rec.down, residual=x2)


def verify_rows_supported(meta):
    """the head shapes decoder_verify_rows takes: those of mm355_attn_extend with d % 16 == 0 (mm355_rope_kv_append_rows)"""
    return ops.attn_extend_supported(meta.Hq, meta.Hkv, meta.d) and meta.d % 16 == 0


def decoder_verify_rows(x, layers, meta, cache, n, pos_rows, blocks, kv_bound):
    """n rows PER SEQUENCE against the cache in one pass over the weights, positions read from the device: x [B * n, h], row (b, i) at b * n
    + i -> hidden rows [B * n, h] (pre final norm).  Row (b, i) is rotated at pos_rows[b * n + i] and appended there in block blocks[b * n +
    i] (int32 device tables; the caller keeps pos_rows[b * n + i] = cache.pos_dev[b] + i and blocks = r // n), then attends the keys j <=
    cache.pos_dev[b] + i of its sequence: the attention step of a layer is the plain q|k|v projection, ONE mm355_rope_kv_append_rows launch
    and ONE mm355_attn_extend call with past = cache.pos_dev, on a bf16 or an fp8_e4m3 cache alike (read back quantised, as n decode steps
    read it).  Row (b, i) therefore gets what decoder_decode_row would give it as the i-th of n successive steps -- the step of prompt-lookup
    speculation (SpecGreedyLoopGraph): rows 1.. are guesses, and whoever verifies them decides how many rows count.  The function changes
    NO length (cache.pos_dev / len_dev / lengths): rows above a sequence's length are not visible to a later step and are overwritten.
    kv_bound: the host bound of the attention launch, every pos + n <= kv_bound <= cache.max_len.  Up to 16 rows: the GEMV route of
    _decode_rows16 in its unfused form (a quantised layer on its bytes); more: _fused_walk with the decode step's gate|up rule.  No host
    value enters a launch but the shapes: capturable once."""
    R = x.shape[0]
    if R != cache.batch * n or n < 1:
        raise ValueError(f"decoder_verify_rows: {R} rows for {cache.batch} sequences of n = {n} rows")
    if cache.shared_len > 0:
        raise ValueError(f"decoder_verify_rows on a cache with a shared prefix of {cache.shared_len} rows is not built")
    if not verify_rows_supported(meta):
        raise ValueError(f"decoder_verify_rows: no kernel for Hq={meta.Hq} Hkv={meta.Hkv} d={meta.d} (ops.attn_extend_supported, d % 16 == 0)")
    if not n <= kv_bound <= cache.max_len:
        raise ValueError(f"decoder_verify_rows: attention bound {kv_bound} for n = {n} rows on a cache of {cache.max_len} rows")
    H = (meta.Hq, meta.Hkv, meta.d)
    nq = meta.Hq * meta.d
    n_ws = int(ops._L().mm355_attn_extend_ws_floats(cache.batch, n, *H, kv_bound))
    ws = torch.empty(max(n_ws, 4), device=x.device, dtype=torch.float32)

    def append_attend(qkv, i):
        rows = cache.rows[i]
        rows.rope_append_rows_(qkv, *H, meta.cos, meta.sin, pos_rows, blocks)
        return rows.attn_extend(qkv[:, :nq], cache.pos_dev, n, kv_bound, *H, meta.scale, workspace=ws)

    if R > 16:
        return _fused_walk(x, layers, meta, lambda qkv, i: append_attend(qkv("gemm", ops.gemm_splitk), i), prompt=False)
    for i, layer in enumerate(layers):
        rec = getattr(layer, "w8", None)
        if rec is None:
            params_ready(layer)
            rec = _bf16_rows16(layer)
        x = _rows16_unfused(x, layer, rec, meta, lambda qkv: append_attend(qkv, i))
    return x


def _decode_rows_gemm(x, layers, meta, cache, cos, sin, kv_bound):
    """17 new rows and more (one per sequence) through every decoder layer in ONE pass over the weights (round 6; rounds 5: chunks of 16 rows,
    i.e. the 15 GB read once per chunk).  The GEMV kernels hold one 16-row MFMA operand; beyond it the projections take the split-K GEMM of
    the prompt pass (mm355_gemm_splitk_bf16: 64 x 128 tiles x K slices -- at 32 rows a weight-streaming problem with ~3 workgroups per CU),
    attention per row at its own length; RoPE + cache append, the two RMSNorms and SwiGLU ride in the reduce launches of the split projections
    (VARIANTS["decode_wide_fused"]; as launches of their own -- thirteen per layer instead of nine -- when off: same bits).  A quantised layer
    takes the same launches on mm355_gemm_w8* (w8_route: per projection; the bytes are streamed once, nothing is dequantised)."""
    nq = meta.Hq * meta.d
    if VARIANTS["decode_wide_fused"] and meta.d % 16 == 0:
        # what follows a split projection rides in its reduce launch (mm355_gemm_splitk_{rope_append,norm,swiglu}_bf16): 9 launches per layer
        def attend(qkv, i):
            rows = cache.rows[i]
            if cache.kv8 is not None:                        # fp8_e4m3 cache: the plain split projection, then the quantising append (ten launches per layer)
                return _append_attend(qkv("gemm", ops.gemm_splitk), rows, meta, cache, cos, sin, kv_bound)
            q = qkv("gemm_rope_append", ops.gemm_splitk_rope_append, meta.Hq, meta.Hkv, meta.d, cos, sin, cache.pos_dev, rows.k, rows.v)
            return _attend_decode(q[:, :nq], rows, meta, cache, kv_bound)

        return _fused_walk(x, layers, meta, attend, prompt=False)
    for i, layer in enumerate(layers):
        params_ready(layer)
        rec = getattr(layer, "w8", None)
        on8 = w8_route(layer, x.shape[0])
        att, mlp = layer.self_attn, layer.mlp
        n1 = ops.rmsnorm_fwd(x, layer.input_layernorm.weight, meta.eps)
        qkv = _proj(on8, rec, "qkv", (att.q_proj.weight, att.k_proj.weight, att.v_proj.weight), "gemm", ops.gemm_splitk, n1)
        o = _append_attend(qkv, cache.rows[i], meta, cache, cos, sin, kv_bound)
        x2 = _proj(on8, rec, "o", (att.o_proj.weight,), "gemm", ops.gemm_splitk, o, residual=x)
        n2 = ops.rmsnorm_fwd(x2, layer.post_attention_layernorm.weight, meta.eps)
        gu = _proj(on8, rec, "gu", (mlp.gate_proj.weight, mlp.up_proj.weight), "gemm", ops.gemm_splitk, n2)
        act = ops.swiglu_fwd(gu, meta.I)
        x = _proj(on8, rec, "down", (mlp.down_proj.weight,), "gemm", ops.gemm_splitk, act, residual=x2)
    return x


SHORT_KV = 1024                                              # mm355_attn_decode: a bound of <= 1024 rows is one key group (no merge, more workgroups)


def decode_kv_bound(cache):
    """The static upper bound on the cached lengths handed to mm355_attn_decode for the NEXT step: 1024 while every sequence (incl. the row
    being appended) still fits one key group -- the kernel then runs its single-group form --, the cache's capacity afterwards.  The host
    knows the lengths (cache.lengths); the bound is a launch parameter, so a captured step exists once per bound (DecodeStepGraph)."""
    return SHORT_KV if (cache.length + 1 <= SHORT_KV and cache.max_len >= SHORT_KV) else cache.max_len


def decoder_decode_row(x, layers, meta, cache, cos, sin, kv_bound=None):
    """One new row PER SEQUENCE against the cache (reference semantics: HF LlamaDecoderLayer with past_key_values, the whole batch in one
    forward per step -- metamorph_llama.py:711-717; the reference's own greedy loop recomputes the prefix instead, :502-597).
    x [batch, h] -> [batch, h]; row b is appended at cache.lengths[b].  The batch goes through the layers in ONE pass (16 rows at a time):
    the 15 GB of LLaMA-3-8B weights are read once per step, not once per sequence.  Every position-dependent input is read from device
    memory (cache.pos_dev / len_dev): the launch sequence is identical for every token, i.e. capturable once and replayable
    (DecodeStepGraph)."""
    if cache.length >= cache.max_len:
        raise ValueError(f"KV cache full ({cache.max_len} rows)")
    B = x.shape[0]
    if B != cache.batch:
        raise ValueError(f"{B} rows for a cache of {cache.batch} sequences")
    bound = decode_kv_bound(cache) if kv_bound is None else kv_bound
    if cache.length + 1 > bound:
        # the bound is a launch parameter (number of key groups): a sequence longer than it would silently attend to its first `bound` keys
        raise ValueError(f"decode bound {bound} is below the longest sequence + 1 ({cache.length + 1}); lengths change only through set_lengths")
    y = (_decode_rows16 if B <= 16 else _decode_rows_gemm)(x, layers, meta, cache, cos, sin, bound)
    cache.pos_dev.add_(1)
    cache.len_dev.add_(1)
    cache.lengths = [n + 1 for n in cache.lengths]
    return y


class _CapturedStep:
    """One decode step over `cache` as a hipGraph per attention bound (decode_kv_bound: the short, single-key-group form while every
    sequence holds <= 1024 rows, the general one afterwards), captured when the bound is first needed and replayed per token; eager
    launches if capture is not possible (functional.set_variant("decode_graph", False) forces that).  A subclass owns the static input
    rows `x_in` and supplies what follows decoder_decode_row in a step (_tail), the `label` of the warning and, where the warm-up must
    leave no trace in its own state, _quiet().  The loops' run() share _poll_loop."""
    label = "decode"

    def __init__(self, layers, meta, cache, cos, sin):
        self.args = (layers, meta, cache, cos, sin)
        self.cache = cache
        self.graphs = {}                                     # kv bound -> (graph, what _launches returned under capture)
        self.capture_ok = VARIANTS["decode_graph"]

    def _launches(self, bound=None):
        """one step on the rows in `x_in`, eager: decoder_decode_row, then the subclass's tail on its hidden rows"""
        return self._tail(decoder_decode_row(self.x_in, *self.args, kv_bound=bound))

    def _tail(self, x):
        return x

    def _quiet(self):
        """(tensor, value) or None: the warm-up launches run for real, so the tensor is filled with the value around warm-up and capture
        (a state in which the step logs and feeds nothing) and restored afterwards"""
        return None

    def _capture(self, bound):
        cache = self.cache
        keep = list(cache.lengths)
        quiet = self._quiet()
        saved = None if quiet is None else quiet[0].clone()
        try:
            if quiet is not None:
                quiet[0].fill_(quiet[1])
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                       # warm-up outside capture (writes a scratch cache row, overwritten by the next real step)
                self._launches(bound)
            torch.cuda.current_stream().wait_stream(side)
            cache.set_lengths(keep)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = self._launches(bound)
            cache.lengths = keep                                 # capture records, it does not run: host mirror unchanged
            self.graphs[bound] = (g, out)
        except Exception as e:                                   # pragma: no cover - depends on the runtime
            import warnings
            warnings.warn(f"hipGraph capture of the {self.label} step failed ({e!r}); using eager launches")
            self.capture_ok = False
            self.graphs = {}
            cache.set_lengths(keep)
        if quiet is not None:
            quiet[0].copy_(saved)

    def _captured(self):
        """The (graph, output) of the next step's bound, captured now if the bound is new; None: eager launches.  Refuses a full cache."""
        if self.capture_ok:
            bound = decode_kv_bound(self.cache)
            if bound not in self.graphs:
                self._capture(bound)
        if not self.capture_ok:
            return None
        if self.cache.length >= self.cache.max_len:
            raise ValueError(f"KV cache full ({self.cache.max_len} rows)")
        return self.graphs[bound]

    def _replay(self, entry):
        entry[0].replay()
        self.cache.lengths = [n + 1 for n in self.cache.lengths]
        return entry[1]

    def _step(self):
        entry = self._captured()
        return self._launches() if entry is None else self._replay(entry)

    def _poll_loop(self, n_steps, after_step=None):
        """Up to n_steps steps, launched blind; the device's count of live sequences is read every `poll` steps -- never after the last
        step, the results are read then anyway -- and the first 0 ends the loop.  `host_reads` counts the reads, the final one included."""
        for s in range(n_steps):
            self._step()
            self.steps += 1
            if after_step is not None:
                after_step(self)
            if self.steps % self.poll == 0 and s + 1 < n_steps:
                self.host_reads += 1
                if int(self.live.item()) == 0:
                    break
        self.host_reads += 1


class DecodeStepGraph(_CapturedStep):
    """decoder_decode_row captured as a hipGraph (5 - 7 launches x layers per step collapse into one graph launch; the per-token step is
    launch-bound otherwise) and replayed per token: copy the new rows (one per sequence) into `x_in`, replay, read `x_out`.  One capture
    per attention bound (_CapturedStep), the first one made here."""

    def __init__(self, layers, meta, cache, cos, sin, h, device):
        super().__init__(layers, meta, cache, cos, sin)
        self.x_in = torch.zeros((cache.batch, h), device=device, dtype=BF16)
        if self.capture_ok:
            self._capture(decode_kv_bound(cache))

    @property
    def graph(self):                                         # (tools / tests: "is the step a graph?")
        return next(iter(self.graphs.values()))[0] if self.graphs else None

    def step(self, rows):
        """rows [batch, h] (one new row per sequence) -> their hidden rows [batch, h] (pre final norm; overwritten by the next step)"""
        entry = self._captured()
        if entry is None:
            return decoder_decode_row(rows.contiguous().view(self.cache.batch, -1), *self.args)
        self.x_in.copy_(rows.view(self.cache.batch, -1))
        return self._replay(entry)


GREEDY_STATE = ("in_image", "n_img", "total_out", "done", "n_tokens", "n_z")     # rows of GreedyLoopGraph.state, arguments of mm355_greedy_advance


def greedy_advance_host(state, tok, start_id, end_id, num_image_tokens, max_new_tokens, eos_ids, token_cap=None, z_cap=None):
    """One iteration of the reference's greedy loop (metamorph_llama.py:569-589) for ONE sequence on plain ints: the specification of
    mm355_greedy_advance.  state: dict over GREEDY_STATE, updated in place; tok: the argmax of this iteration's logits.  Returns
    (log, next_row): log "tok" (the id goes to the token log), "z" (the image head's pred_z row goes to the z log) or None; next_row "embed"
    (embed_tokens[tok]), "fed" (the row the lm_head saw: the projector output) or None.  A finished sequence changes nothing and returns
    (None, None); so does one whose log is full (token_cap / z_cap rows), which is set done instead of written."""
    s = state
    if s["done"]:
        return None, None
    image_row = bool(s["in_image"]) and s["n_img"] < num_image_tokens
    if (z_cap is not None and s["n_z"] >= z_cap) if image_row else (token_cap is not None and s["n_tokens"] >= token_cap):
        s["done"] = 1
        return None, None
    if not s["in_image"] and tok == start_id:
        s["in_image"] = 1
    elif image_row:
        s["n_img"] += 1
        s["n_z"] += 1
        if s["n_img"] == num_image_tokens:
            s["in_image"] = 0
    elif tok == end_id:
        s["in_image"] = 0
        s["n_img"] = 0
    if not image_row:
        s["n_tokens"] += 1
    s["total_out"] += 1
    if tok in eos_ids or s["total_out"] > max_new_tokens:
        s["done"] = 1
    return ("z", "fed") if image_row else ("tok", "embed")


def greedy_host_loop(head, feed, start_id, end_id, num_image_tokens, max_new_tokens, eos_ids):
    """The reference's greedy loop (metamorph_llama.py:502-597) of ONE sequence, token loop on the host: greedy_advance_host per iteration.
    head(in_image) -> (tok, fed_row, pred_z): the argmax id of the current row's logits, the row the lm_head saw, the image head's row;
    feed(tok, row): the next input, `row` the fed row after an image row, None for embed_tokens[tok].  Returns (ids, pred_z rows) as logged."""
    state, eos, logs = dict.fromkeys(GREEDY_STATE, 0), set(eos_ids), {"tok": [], "z": []}
    while True:
        tok, fed_row, pred_z = head(bool(state["in_image"]))
        log, next_row = greedy_advance_host(state, tok, start_id, end_id, num_image_tokens, max_new_tokens, eos)
        logs[log].append(tok if log == "tok" else pred_z)      # (no log caps: every iteration of a live sequence logs)
        if state["done"]:
            return logs["tok"], logs["z"]
        feed(tok, fed_row if next_row == "fed" else None)


BEAM_MAX = 8                                                 # MM355_BEAM_MAX
BEAM_EARLY_STOPPING = {False: 0, True: 1, "never": 2}        # mm355_beam_advance's early_stopping


def beam_candidates(num_beams, n_eos):
    """M: the candidates HF's beam search keeps per step (`beams_to_keep`), max(2, 1 + eos ids) * K"""
    return max(2, 1 + int(n_eos)) * int(num_beams)


def beam_len_pow(max_new_tokens, length_penalty):
    """float32(t ** length_penalty), t = 1 .. max_new_tokens: the divisors of HF's length penalty as it forms them (a Python int to a
    Python power, rounded to fp32 where it meets the fp32 scores).  The device reads this table and calls no pow."""
    import numpy as np
    out = np.empty(int(max_new_tokens), dtype=np.float32)
    with np.errstate(over="ignore"):
        for t in range(1, int(max_new_tokens) + 1):
            try:
                out[t - 1] = np.float32(t ** length_penalty)
            except OverflowError:
                out[t - 1] = np.float32(np.inf)
    return out


def _beam_order(vals):
    """indices of `vals` in the candidates' order: value descending, a NaN after every number, among equals the lower index first
    (torch.topk leaves ties open; this is the rule of cand_beats in csrc/beam.hip)"""
    import numpy as np
    v = np.asarray(vals, dtype=np.float32)
    nan = np.isnan(v)
    return np.lexsort((np.arange(v.shape[0]), np.where(nan, np.float32(0), -v), nan))


def beam_logprob_rows_host(x, stats):
    """(x[b, i] - m_b) - lse_b in fp32, in that order: the log-probabilities mm355_beam_select_rows_f32 forms from its own statistics
    stats [K, 2] = (m, lse); a row whose lse is NaN (a NaN in the row, m = +-inf) is NaN throughout."""
    import numpy as np
    x = np.asarray(x, dtype=np.float32)
    st = np.asarray(stats, dtype=np.float32)
    with np.errstate(all="ignore"):
        lp = (x - st[:, :1]) - st[:, 1:2]
    lp[np.isnan(st[:, 1])] = np.float32("nan")
    return lp


def beam_select_host(lp, running, M):
    """Step 1 of HF's beam step: the M best of acc[b * V + i] = lp[b, i] + running[b] (fp32) -> (values [M] fp32, flat indices [M] int32),
    sorted in _beam_order.  The specification of the candidate list of mm355_beam_select_rows_f32 (given beam_logprob_rows_host of its
    statistics)."""
    import numpy as np
    lp = np.asarray(lp, dtype=np.float32)
    with np.errstate(all="ignore"):
        acc = (lp + np.asarray(running, dtype=np.float32)[:, None]).reshape(-1)
    order = _beam_order(acc)[:int(M)]
    return acc[order], order.astype(np.int32)


def beam_state_host(num_beams, max_new_tokens):
    """The state of a beam search before its first step (HF _beam_search, section 3): a dict of NumPy arrays, the layout of the device
    state of BeamLoopGraph.  own_block is the table of mm355_attn_decode_shared_idx, the identity at the start."""
    import numpy as np
    K, cap = int(num_beams), int(max_new_tokens) + 1
    running = np.full(K, -1e9, dtype=np.float32)
    running[0] = 0
    return dict(running=running, fin_score=np.full(K, -1e9, dtype=np.float32), fin_flag=np.zeros(K, dtype=np.int32),
                fin_end=np.full((K, 3), -1, dtype=np.int32), scal=np.array([1, 0], dtype=np.int32), live=np.array([1], dtype=np.int32),
                tok=np.zeros(K, dtype=np.int32), parent=np.zeros(K, dtype=np.int32), tok_log=np.zeros((cap, K), dtype=np.int32),
                parent_log=np.zeros((cap, K), dtype=np.int32), own_block=np.repeat(np.arange(K, dtype=np.uint8)[:, None], cap, 1))


def beam_step_host(state, cand_val, cand_idx, V, eos_ids, max_new_tokens, len_pow, length_penalty=1.0, early_stopping=False):
    """Steps 2 - 6 of one iteration of HF's GenerationMixin._beam_search (transformers 5.15, generation/utils.py: stopping criteria,
    _get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic, _beam_search_has_unfinished_sequences)
    for ONE prompt on the M sorted candidates of step 1, in fp32 with HF's literal -1e9: the specification of mm355_beam_advance.
    state: beam_state_host's dict, updated in place (a search whose live flag is 0 changes nothing); len_pow: beam_len_pow.
    Besides HF's state it keeps what the device keeps instead of id sequences: row n of the back-pointer logs tok_log / parent_log, for
    every pool entry where its hypothesis ended (fin_end: step, the parent's slot, id), and the table own_block: after the step whose
    generated length was n, own rows [0, n) of slot i are those of its parent and row n is the row slot i appends next, in block i."""
    import numpy as np
    s = state
    if not s["live"][0]:
        return
    f32, NEG = np.float32, np.float32(-1e9)
    K, M = s["running"].shape[0], len(cand_val)
    unsat, n = int(s["scal"][0]), int(s["scal"][1])
    if not 0 <= n < int(max_new_tokens):
        s["live"][0] = 0
        return
    val = np.asarray(cand_val, dtype=np.float32)
    idx = np.clip(np.asarray(cand_idx, dtype=np.int64), 0, K * int(V) - 1)
    par, ids = (idx // V).astype(np.int32), (idx % V).astype(np.int32)
    eos = set(int(e) for e in eos_ids)
    hit = np.array([int(i) in eos or n + 1 >= max_new_tokens for i in ids])
    with np.errstate(all="ignore"):
        # 3. running beams
        run = val + hit.astype(np.float32) * NEG
        pick = _beam_order(run)[:K]
        s["running"][:] = run[pick]
        s["tok"][:], s["parent"][:] = ids[pick], par[pick]
        s["tok_log"][n], s["parent_log"][n] = ids[pick], par[pick]
        # 4. finished pool
        full = bool(s["fin_flag"].all())
        fin_now = hit & (np.arange(M) < K)
        fin = val / f32(len_pow[n])
        fin = fin + f32(full and early_stopping is True) * NEG
        fin = fin + f32(not unsat) * NEG
        fin = fin + (~fin_now).astype(np.float32) * NEG
        scores = np.concatenate([s["fin_score"], fin.astype(np.float32)])
        flags = np.concatenate([s["fin_flag"], fin_now.astype(np.int32)])
        ends = np.concatenate([s["fin_end"], np.stack([np.full(M, n, dtype=np.int32), par, ids], 1)])
        keep = _beam_order(scores)[:K]
        s["fin_score"][:], s["fin_flag"][:], s["fin_end"][:] = scores[keep], flags[keep], ends[keep]
        # 5. the heuristic
        n1 = n + 1
        fixed = early_stopping == "never" and length_penalty > 0.0
        best = s["running"][0] / f32(len_pow[(int(max_new_tokens) if fixed else n1) - 1])
        worst = np.where(s["fin_flag"] != 0, np.min(s["fin_score"]), NEG)
        unsat = int(bool(unsat) and bool(np.any(best > worst)))
    s["scal"][:] = (unsat, n1)
    # 6. go on?
    if not (unsat and not (bool(s["fin_flag"].all()) and early_stopping is True) and not bool(hit.all())):
        s["live"][0] = 0
    # the table of own rows
    tbl = s["own_block"]
    tbl[:, :n] = tbl[s["parent"], :n]
    tbl[:, n] = np.arange(K, dtype=np.uint8)


def beam_hypotheses_host(state):
    """The pool of a finished search -> (ids, scores, flags): per pool entry, best first, its generated ids (int32; rebuilt from the
    back-pointer logs: the entry ended at step t with `id` on the beam that sat in slot p after step t - 1), its fp32 score and whether
    it is a finished hypothesis (an unfinished entry has no ids and HF's -1e9)."""
    import numpy as np
    out = []
    for (t, p, tok), flag in zip(state["fin_end"].tolist(), state["fin_flag"].tolist()):
        ids = []
        if flag:
            ids = [tok]
            for u in range(t - 1, -1, -1):
                ids.append(int(state["tok_log"][u][p]))
                p = int(state["parent_log"][u][p])
        out.append(np.array(ids[::-1], dtype=np.int32))
    return out, np.array(state["fin_score"], dtype=np.float32), np.array(state["fin_flag"], dtype=np.int32)


def beam_search_host(logprob_rows_fn, num_beams, V, eos_ids, max_new_tokens, length_penalty=1.0, early_stopping=False):
    """HF's beam search for one prompt, driven by logprob_rows_fn(t, state) -> the [K, V] fp32 log-probability rows of the running beams
    at step t (state["tok"] / state["parent"] say which beams those are).  Returns (ids, scores, flags, steps): beam_hypotheses_host of
    the final pool and the number of steps run."""
    import numpy as np
    if early_stopping not in (False, True, "never") or isinstance(early_stopping, (int, float)) and not isinstance(early_stopping, bool):
        raise ValueError(f"early_stopping = {early_stopping!r}: one of False, True, 'never'")
    state = beam_state_host(num_beams, max_new_tokens)
    len_pow = beam_len_pow(max_new_tokens, length_penalty)
    M = beam_candidates(num_beams, len(set(eos_ids)))
    t = 0
    while state["live"][0]:
        val, idx = beam_select_host(np.asarray(logprob_rows_fn(t, state), dtype=np.float32), state["running"], M)
        beam_step_host(state, val, idx, V, eos_ids, max_new_tokens, len_pow, length_penalty, early_stopping)
        t += 1
    return (*beam_hypotheses_host(state), t)


def philox4x32_10(counter4, key2):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) on plain ints: four 32-bit counter
    words and two key words -> four output words.  The specification of the generator in mm355_philox_uniform_rows."""
    c = [int(v) & 0xFFFFFFFF for v in counter4]
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key2)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return tuple(c)


def philox_uniform_host(seed, stream_id, counter):
    """The uniform in [0, 1) of (seed, stream id, counter): key = the seed's low and high 32 bits, counter = (counter, stream id, 0, 0),
    the top 24 bits of output word 0 times 2^-24 (exact in fp32).  What mm355_philox_uniform_rows writes for one row."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return (philox4x32_10((counter, stream_id, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))[0] >> 8) * 2.0 ** -24


def sample_row_host(x, inv_t, top_k, top_p, u, eps=0.0, tau=None):
    """One row of mm355_sample_rows_f32 in fp64: the specification of the sampler, as greedy_advance_host is of the transition.  x: the row
    (any float sequence), u in [0, 1).  Returns (candidates, tau_lo, tau_hi, Z).
    Weights w_i = exp((x_i - m) * inv_t), m the maximum.  top-k keeps i iff #{x_j > x_i} < top_k (0 or >= C: off); of those, top-p keeps
    i iff the weight above x_i is < top_p * Zk, Zk the weight top-k kept (>= 1: off): the kept set is {x_i >= tau}.
    eps = 0: tau_lo = tau_hi = tau, Z the kept weight and candidates the one index whose interval [P_(i-1), P_i) of the kept weights'
    running sum in index order holds u * Z.  eps > 0 gives the bands an fp32 implementation is held to: the top-p comparison is taken at
    (top_p -+ eps) * Zk -- tau_hi is the tau of the smaller threshold, tau_lo that of the larger one, both values of the row, the top-k
    part exact -- and candidates are the kept indices of positive weight whose interval meets [(u - eps) Z, (u + eps) Z], plus the last
    kept index where (u + eps) Z reaches Z (rounding may leave no index).  tau: evaluate Z and the candidates for the kept set
    {x_i >= tau} (an implementation's own tau out of the band) instead of the eps = 0 one.
    A maximum that is NaN or infinite: ([torch.argmax's index], m, m, 0.0)."""
    import numpy as np
    x = np.asarray(x, dtype=np.float64)
    C = x.shape[0]
    nan = np.isnan(x)
    m = float("nan") if nan.any() else float(x.max())
    if not math.isfinite(m):
        return [int(np.argmax(nan)) if nan.any() else int(np.argmax(x))], m, m, 0.0
    w = np.exp((x - m) * float(inv_t))
    vals, inv, counts = np.unique(x, return_inverse=True, return_counts=True)       # ascending distinct values
    mass = np.bincount(inv.reshape(-1), weights=w, minlength=len(vals))
    n_above = counts[::-1].cumsum()[::-1] - counts
    m_above = np.concatenate((mass[::-1].cumsum()[::-1][1:], [0.0]))                # (summed from the top: no cancellation)
    k_on = 0 < int(top_k) < C
    kept_k = n_above < int(top_k) if k_on else np.ones(len(vals), dtype=bool)
    j_k = int(np.argmax(kept_k))                                                    # kept_k is a suffix of the ascending values
    Zk = m_above[j_k] + mass[j_k]

    def tau_of(p):
        if float(top_p) >= 1.0:
            return float(vals[j_k])
        kept = kept_k & (m_above < p * Zk)
        kept[-1] = True
        return float(vals[int(np.argmax(kept))])
    tau_lo, tau_hi = tau_of(float(top_p) + eps), tau_of(float(top_p) - eps)
    t = tau_of(float(top_p)) if tau is None else float(tau)
    idx = np.nonzero(x >= t)[0]
    P = np.cumsum(w[idx])
    Z = math.fsum(w[idx])
    lo, hi = (u - eps) * Z, (u + eps) * Z
    prev = np.concatenate(([0.0], P[:-1]))
    cand = idx[(w[idx] > 0) & (P > lo) & (prev <= hi)].tolist()
    if hi >= Z and int(idx[-1]) not in cand:
        cand.append(int(idx[-1]))
    return [int(c) for c in cand], tau_lo, tau_hi, Z


def seen_bits_host(ids, C, words=None):
    """The bitmap of mm355_logits_process_rows_f32 / mm355_token_note_rows_f32 for one sequence: uint32 [words >= ceil(C / 32)], bit
    (i & 31) of word (i >> 5) set for every id i of `ids` (each in [0, C))."""
    import numpy as np
    bits = np.zeros(ops.seen_words(C) if words is None else int(words), dtype=np.uint32)
    for i in ids:
        i = int(i)
        if not 0 <= i < C:
            raise ValueError(f"id {i} outside [0, {C})")
        bits[i >> 5] |= np.uint32(1 << (i & 31))
    return bits


def logits_process_host(row_f32, seen_bits, penalty, total_out, min_new_tokens, eos_ids, suppress_ids):
    """One row of mm355_logits_process_rows_f32 in numpy.float32: its specification, which the kernel equals bit for bit.  row_f32: the C
    logits; seen_bits: the sequence's uint32 bitmap (seen_bits_host) or None; total_out: the loop's count of outputs of the sequence.
    HF's order: every marked i < C becomes x_i * penalty where x_i < 0, x_i / penalty otherwise (skipped for penalty 1 or no bitmap; bits
    at positions >= C are ignored); then, while total_out < min_new_tokens (> 0), every eos id becomes -inf; then every suppressed id
    does.  Ids outside [0, C) in either list are skipped.  Returns a new float32 array."""
    import numpy as np
    x = np.array(row_f32, dtype=np.float32, copy=True)
    C = x.shape[0]
    p = np.float32(penalty)
    if seen_bits is not None and p != np.float32(1.0):
        words = np.asarray(seen_bits, dtype=np.uint32)
        marked = ((words[np.arange(C) >> 5] >> (np.arange(C) & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)
        with np.errstate(all="ignore"):
            x[marked] = np.where(x[marked] < 0, x[marked] * p, x[marked] / p)
    if int(min_new_tokens) > 0 and int(total_out) < int(min_new_tokens):
        for e in eos_ids:
            if 0 <= int(e) < C:
                x[int(e)] = -np.inf
    for s in ([] if suppress_ids is None else suppress_ids):
        if 0 <= int(s) < C:
            x[int(s)] = -np.inf
    return x


def token_note_host(row, tok, done, in_image, n_img, n_tokens, num_image_tokens, token_cap):
    """One row of mm355_token_note_rows_f32: (logs, logp).  logs: the row logs an id -- not done, no image row (in_image and n_img <
    num_image_tokens), n_tokens < token_cap and 0 <= tok < C -- which is when greedy_advance_host returns the log "tok".  logp (float64,
    NaN where tok is no column): row[tok] - m - ln(sum_i exp(row_i - m)) in fp64, m the maximum; a NaN in the row, m = +inf or a row of
    -inf only give NaN, row[tok] = -inf under a finite m gives -inf.  The kernel's fp32 value is held to it within 1e-4 + 2^-22 |logp|."""
    import numpy as np
    x = np.asarray(row, dtype=np.float64)
    C, tok = x.shape[0], int(tok)
    logs = (not done) and not (in_image and n_img < num_image_tokens) and 0 <= n_tokens < token_cap and 0 <= tok < C
    if not 0 <= tok < C:
        return logs, float("nan")
    m = float("nan") if np.isnan(x).any() else float(x.max())
    if not math.isfinite(m):
        return logs, float("nan")
    with np.errstate(all="ignore"):
        return logs, float(x[tok] - m - math.log(math.fsum(np.exp(x - m))))


@dataclasses.dataclass
class LogitsProcessors:
    """What GreedyLoopGraph(processors=...) applies to the logits between the head and the pick, and what it notes after the pick.
    repetition_penalty (1: off), min_new_tokens (0: off; counts the loop's total_out, so image rows count) and suppress_ids (an int32
    DEVICE tensor, or None: off) are the arguments of mm355_logits_process_rows_f32; want_logprobs logs the log-probability of every
    emitted id (of the processed row, before temperature / top-k / top-p: mm355_token_note_rows_f32); marks: ids marked as seen before
    the first step -- one list for every sequence or one list per sequence (None: a sequence's bitmap starts empty, HF's behaviour when
    it is handed inputs_embeds)."""
    repetition_penalty: float = 1.0
    min_new_tokens: int = 0
    suppress_ids: object = None
    want_logprobs: bool = False
    marks: object = None

    @property
    def penalised(self):
        return float(self.repetition_penalty) != 1.0

    @property
    def edits(self):
        return self.penalised or int(self.min_new_tokens) > 0 or (self.suppress_ids is not None and self.suppress_ids.numel() > 0)

    @property
    def active(self):
        return self.edits or bool(self.want_logprobs)


def _refuse_loop_args(n_eos, C, embed, poll, an_id="an argmax id", beams=None):
    """what every device token loop refuses before it allocates anything, in this order (`beams`: the beam loop's count of them)"""
    if n_eos > ops.GREEDY_MAX_EOS:
        raise ValueError(f"{n_eos} eos ids: the device loop takes up to {ops.GREEDY_MAX_EOS}")
    if beams is not None and not 1 <= beams <= BEAM_MAX:
        raise ValueError(f"{beams} beams: the device beam loop takes 1 .. {BEAM_MAX}")
    if C > embed.shape[0]:
        raise ValueError(f"{C} logits over an embedding of {embed.shape[0]} rows: {an_id} would be no row of it")
    if int(poll) < 1:
        raise ValueError(f"mm355_greedy_poll_steps = {poll}: the live counter is read every poll >= 1 steps")


class _GreedyLoopBase(_CapturedStep):
    """What the greedy device loops share: the refusals, the scalars, the static buffers of a step of `rows` rows per sequence (`x_in`,
    `logits`, `tok`), `state` (GREEDY_STATE) and `live`, the logs `tok_log` / `z_log` of max_new_tokens + 1 iterations, `steps` / `host_reads`
    and the read-out after the last step.  A subclass supplies _tail and, allocated between `tok` and the logs, what its pick needs."""

    def __init__(self, layers, meta, cache, cos, sin, h, device, head, embed, C, Dz, start_id, end_id, num_image_tokens, max_new_tokens,
                 eos_ids, poll, rows=1):
        _refuse_loop_args(len(eos_ids), C, embed, poll)
        super().__init__(layers, meta, cache, cos, sin)
        B, R = cache.batch, cache.batch * rows
        self.head, self.embed, self.C, self.max_new_tokens, self.poll = head, embed, int(C), int(max_new_tokens), int(poll)
        self.scalars = (int(start_id), int(end_id), int(num_image_tokens), self.max_new_tokens, sorted(int(e) for e in eos_ids))
        cap = self.max_new_tokens + 1                        # iterations of the loop: total_out > max_new_tokens ends it
        self.x_in = torch.zeros((R, h), device=device, dtype=BF16)
        self.state = torch.zeros((len(GREEDY_STATE), B), device=device, dtype=torch.int32)
        self.live = torch.full((1,), B, device=device, dtype=torch.int32)
        self.logits = torch.empty((R, self.C), device=device, dtype=torch.float32)
        self.tok = torch.zeros(R, device=device, dtype=torch.int32)
        self._alloc_pick(R, device)
        self.tok_log = torch.zeros((B, cap), device=device, dtype=torch.int32)
        self.z_log = torch.zeros((B, cap, Dz), device=device, dtype=BF16)
        self.host_reads, self.steps = 0, 0

    def _alloc_pick(self, R, device):
        self.arg_ws = ops.argmax_rows_ws(R, self.C, device)

    def _quiet(self):
        return self.state[3], 1                              # with every sequence done the kernels log, feed and write no state

    def _results(self):
        """(state on the host, per sequence its int32 ids, per sequence its [n_b, Dz] bf16 image rows) once every sequence is done"""
        st = self.state.cpu()
        if not bool(st[3].all()):                               # pragma: no cover - max_new_tokens steps finish every sequence by construction
            raise RuntimeError(f"{self.label} loop: sequences still live after {self.steps} steps (state {st.tolist()})")
        n_tok, n_z = st[4].tolist(), st[5].tolist()
        return st, [self.tok_log[b, :n].clone() for b, n in enumerate(n_tok)], [self.z_log[b, :n].clone() for b, n in enumerate(n_z)]


class GreedyLoopGraph(_GreedyLoopBase):
    """The greedy text-and-image loop (reference metamorph_llama.py:502-597) of a batch with the token loop on the device.  One step is
    decoder_decode_row (all rows, whatever route the batch size takes) -> `head` (the model's final norm, image head for ALL rows, row select
    by the device-resident mode, lm_head into the static fp32 `logits`) -> mm355_argmax_rows_f32 -> mm355_greedy_advance, which runs the
    reference's branch per sequence (greedy_advance_host) and writes the next input rows into `x_in`: the step reads no host value, so it is
    captured as ONE hipGraph on one stream per attention bound (decode_kv_bound) and replayed per token; set_variant("decode_graph", False)
    runs the same launches eagerly.  The host replays at most max_new_tokens steps and reads the device's count of live sequences every
    `poll` steps -- the only device -> host read of the loop (`host_reads` counts them, the final read of the results included).  A finished
    sequence keeps riding along: mm355_greedy_advance writes nothing for it, its cache rows grow and nobody reads them (the cache's
    max(L_b) + max_new_tokens + 2 rows cover max_new_tokens steps for every sequence), so the results do not depend on `poll`.
    head(x [B, h], in_image int32 [B], logits_out f32 [B, C]) -> (fed [B, h], pred_z [B, Dz]).
    sampler = (inv_temperature, top_k, top_p, seed, stream_ids): the id is drawn instead of taken as the argmax -- mm355_philox_uniform_rows
    (seed, stream_ids[b], the sequence's total_out) -> mm355_sample_rows_f32 (sample_row_host) in place of the argmax, everything else as
    it is.  The uniforms are stateless, so the warm-up launch and the capture consume no draw and a sequence's draws depend on (seed, its
    stream id, its total_out) only; an image row ignores the id as before, its draw is unused.  `seed` records the seed.
    processors = a LogitsProcessors with anything active: the tail becomes head -> mm355_logits_process_rows_f32 (only where a processor
    edits: penalty, min_new_tokens, suppress_ids) -> the pick as above, on the processed row -> mm355_token_note_rows_f32 (only where the
    penalty needs the ids marked or the log-probabilities are wanted) -> mm355_greedy_advance, all inside the same captured graph (and in
    the first, uncaptured tail).  `seen` [B, seen_words(C)] holds the bitmap of the ids each sequence has logged (int32 storage of the
    uint32 words, ~16 KB per sequence at 128 256 logits), `logp_log` [B, cap] fp32 the log-probability of every logged id under the
    PROCESSED logits (before temperature, top-k and top-p; with no processor editing, the model's own log-softmax); run() then returns them
    as a third list.  processors None (or nothing active in it): none of this is allocated or launched."""
    label = "greedy"

    def __init__(self, layers, meta, cache, cos, sin, h, device, head, embed, C, Dz, start_id, end_id, num_image_tokens, max_new_tokens,
                 eos_ids, poll=8, sampler=None, processors=None):
        self.sampler, self.seed, self._draw = None, None, sampler
        super().__init__(layers, meta, cache, cos, sin, h, device, head, embed, C, Dz, start_id, end_id, num_image_tokens, max_new_tokens,
                         eos_ids, poll)
        self.processors = processors if processors is not None and processors.active else None
        if self.processors is not None:
            self._init_processors(cache.batch, self.max_new_tokens + 1, device)

    def _alloc_pick(self, B, device):
        if self._draw is None:
            return super()._alloc_pick(B, device)
        inv_t, top_k, top_p, seed, stream_ids = self._draw
        if len(stream_ids) != B:
            raise ValueError(f"{len(stream_ids)} stream ids for {B} sequences")
        self.sampler, self.seed = (float(inv_t), int(top_k), float(top_p)), int(seed) & 0xFFFFFFFFFFFFFFFF
        self.stream_ids = torch.tensor([int(i) for i in stream_ids], dtype=torch.int32).to(device)
        self.u = torch.zeros(B, device=device, dtype=torch.float32)
        self.smp_ws = ops.sample_rows_ws(B, self.C, device)

    def _init_processors(self, B, cap, device):
        p = self.processors
        penalty, min_new = float(p.repetition_penalty), int(p.min_new_tokens)
        if not (math.isfinite(penalty) and penalty > 0):
            raise ValueError(f"repetition_penalty = {penalty} must be finite and > 0 (1: off)")
        if min_new < 0:
            raise ValueError(f"min_new_tokens = {min_new} must be >= 0 (0: off)")
        sup = p.suppress_ids
        if sup is not None and (sup.dtype != torch.int32 or sup.dim() != 1 or not sup.is_cuda):
            raise ValueError("suppress_ids: a 1-D int32 device tensor")
        if p.marks is not None and not p.penalised:
            raise ValueError("initial marks without an active repetition penalty: nothing would read them")
        self._process = (penalty, min_new, sup.contiguous() if sup is not None and sup.numel() else None) if p.edits else None
        if p.penalised:
            words = ops.seen_words(self.C)
            bits = np.zeros((B, words), dtype=np.uint32)
            if p.marks is not None:
                marks = list(p.marks)
                per_row = marks if marks and isinstance(marks[0], (list, tuple)) else [marks] * B
                if len(per_row) != B:
                    raise ValueError(f"{len(per_row)} lists of marked ids for {B} sequences")
                for b in range(B):
                    bits[b] = seen_bits_host(per_row[b], self.C, words)
            self.seen = torch.from_numpy(bits.view(np.int32)).to(device)
        if p.want_logprobs:
            self.logp_log = torch.zeros((B, cap), device=device, dtype=torch.float32)

    def _tail(self, x):
        fed, pred_z = self.head(x, self.state[0], self.logits)
        p = self.processors
        if p is not None and self._process is not None:
            penalty, min_new, sup = self._process
            ops.logits_process_rows(self.logits, penalty, self.seen if p.penalised else None, self.state[2], min_new, self.scalars[4], sup)
        if self.sampler is None:
            ops.argmax_rows(self.logits, out=self.tok, ws=self.arg_ws)
        else:
            ops.philox_uniform_rows(self.seed, self.stream_ids, self.state[2], out=self.u)
            ops.sample_rows(self.logits, *self.sampler, self.u, out=self.tok, ws=self.smp_ws)
        if p is not None and (p.penalised or p.want_logprobs):
            ops.token_note_rows(self.logits, self.tok, self.state, self.scalars[2], self.tok_log.shape[1],
                                seen=self.seen if p.penalised else None, logp_log=self.logp_log if p.want_logprobs else None)
        ops.greedy_advance(self.tok, self.C, self.state, self.live, self.embed, fed, pred_z, self.x_in, self.tok_log, self.z_log,
                           *self.scalars)

    def run(self, x0):
        """x0 [B, h]: the prompt pass's last hidden row of every sequence (pre final norm).  The first iteration's head and advance run on
        it without a decoder step; then up to max_new_tokens steps.  Returns (ids, pred_z): per sequence its int32 ids and its [n_b, Dz]
        bf16 image rows; with processors.want_logprobs (ids, pred_z, logprobs): per sequence the fp32 log-probabilities of its ids."""
        self._tail(x0.contiguous())
        self._poll_loop(self.max_new_tokens)
        st, *out = self._results()
        if self.processors is not None and self.processors.want_logprobs:
            out.append([self.logp_log[b, :n].clone() for b, n in enumerate(st[4].tolist())])
        return tuple(out)


SPEC_MAX_DRAFT, SPEC_MAX_NGRAM = ops.SPEC_MAX_DRAFT, ops.SPEC_MAX_NGRAM      # MM355_SPEC_MAX_DRAFT, MM355_SPEC_MAX_NGRAM


def prompt_lookup_host(hist, K, N, C):
    """The drafts of ONE sequence on plain ints: the specification of mm355_ngram_draft_rows, equal to HF's
    PromptLookupCandidateGenerator.get_candidates (num_output_tokens = K, max_matching_ngram_size = N, no eos ids, no logits processor,
    unbounded max_length) wherever every id lies in [0, C).  hist: the lookup ids followed by the ids logged so far.  For m = min(N, len -
    1) down to 1 the last m ids are the pattern; the LOWEST index where it occurs and whose continuation hist[idx + m : idx + m + K],
    cropped at the first id outside [0, C), is not empty gives the drafts (the trailing occurrence has no continuation; a match whose
    continuation starts with such an id is skipped).  Returns the list of drafts, [] if no m has a match."""
    hist = [int(t) for t in hist]
    L = len(hist)
    for m in range(min(int(N), L - 1), 0, -1):
        pat = hist[L - m:]
        for idx in range(L - m):
            if hist[idx] == pat[0] and hist[idx:idx + m] == pat:
                out = []
                for t in hist[idx + m:idx + m + int(K)]:
                    if not 0 <= t < C:
                        break
                    out.append(t)
                if out:
                    return out
    return []


def spec_advance_host(state, toks, drafts, start_id, end_id, num_image_tokens, max_new_tokens, eos_ids, token_cap=None, z_cap=None):
    """One step of prompt-lookup speculation for ONE sequence on plain ints: the specification of mm355_spec_verify_advance, a loop over
    greedy_advance_host.  toks: the argmax of the step's rows (row 0: the real next input, row i: the input drafts[i - 1]), at least
    len(drafts) + 1 of them.  Iteration i runs greedy_advance_host with toks[i]; the walk ends after the first iteration that logged
    nothing (a full log), finished the sequence, was an image row (the next input is a fed row), left the sequence in image mode (the next
    row's head mask differs), was the last row with a draft behind it (i == len(drafts)) or whose id is not the draft the next row was fed
    (toks[i] != drafts[i]).  state is updated in place.  Returns the iterations run as greedy_advance_host's (log, next_row) pairs -- []
    for a sequence that was done on entry; their number is what the cache's length advances by."""
    out = []
    if state["done"]:
        return out
    for i, tok in enumerate(toks):
        log, nxt = greedy_advance_host(state, int(tok), start_id, end_id, num_image_tokens, max_new_tokens, eos_ids, token_cap=token_cap,
                                       z_cap=z_cap)
        out.append((log, nxt))
        if log is None or state["done"] or log == "z" or state["in_image"] or i >= len(drafts) or int(tok) != int(drafts[i]):
            break
    return out


class SpecGreedyLoopGraph(_GreedyLoopBase):
    """GreedyLoopGraph with prompt-lookup speculation (HF's prompt_lookup_num_tokens; no second model): a step carries n = K + 1 rows per
    sequence -- its real next input and up to K ids guessed from its own text -- and emits up to n ids.  One step is decoder_verify_rows
    (B * n rows, one pass over the weights) -> `head` on all rows with the per-row mode mask -> mm355_argmax_rows_f32 over B * n rows ->
    mm355_spec_verify_advance (the reference's branch, greedy_advance_host, over the rows of a sequence while its guesses hold; advances
    the cache's pos_dev / len_dev by the iterations run) -> mm355_ngram_draft_rows (the next step's guesses and input rows): the step reads
    no host value and its shape is fixed, so it is ONE hipGraph on one stream, captured for one attention bound, the cache's capacity.
    Every emitted id is the argmax of a row computed on the correct prefix -- the loop is the sequential greedy loop run on a subset of the
    step's rows; rejected and dummy rows land above a sequence's length, are never read and are overwritten by the next step.  A finished
    sequence advances by 0 (the kernels write no state for it; its rows keep landing at its length, where nobody reads them), so max(L_b) + max_new_tokens + 2 + K cache rows suffice; the host keeps an
    upper bound of the lengths, refuses a cache that cannot hold another n rows, and sets cache.lengths from len_dev after the run.
    lookup_ids: one id list per sequence, the text its drafts are looked up in (with what it emits appended); ids outside [0, C) are kept:
    they match nothing the loop emits and end a draft.  head(x [B * n, h], mask int32 [B * n], logits_out f32 [B * n, C]) -> (fed, pred_z).
    After run(): `steps`, `host_reads`, `emitted` (loop iterations per sequence) and `acc_log` (per sequence the iterations each of its
    steps advanced, the first iteration -- run on the prompt's last row without a step -- not among them)."""
    label = "speculative greedy"

    def __init__(self, layers, meta, cache, cos, sin, h, device, head, embed, C, Dz, start_id, end_id, num_image_tokens, max_new_tokens,
                 eos_ids, lookup_ids, num_draft, max_ngram=2, poll=8):
        K, N = int(num_draft), int(max_ngram)
        if not 1 <= K <= SPEC_MAX_DRAFT or not 1 <= N <= SPEC_MAX_NGRAM:
            raise ValueError(f"speculative loop: {K} drafts (1 .. {SPEC_MAX_DRAFT}) from n-grams of up to {N} ids (1 .. {SPEC_MAX_NGRAM})")
        _refuse_loop_args(len(eos_ids), C, embed, poll)       # (the shared refusals come before the loop's own)
        B = cache.batch
        if len(lookup_ids) != B:
            raise ValueError(f"{len(lookup_ids)} lists of lookup ids for {B} sequences")
        if not verify_rows_supported(meta):
            raise ValueError(f"speculative loop: no kernel for Hq={meta.Hq} Hkv={meta.Hkv} d={meta.d} (ops.attn_extend_supported, d % 16 == 0)")
        if meta.cos is not cos or meta.sin is not sin:
            raise ValueError("speculative loop: meta.cos / meta.sin must be the RoPE tables cos / sin (decoder_verify_rows reads them from meta)")
        super().__init__(layers, meta, cache, cos, sin, h, device, head, embed, C, Dz, start_id, end_id, num_image_tokens, max_new_tokens,
                         eos_ids, poll, rows=K + 1)
        self.K, self.N, self.n = K, N, K + 1
        n, R, cap = self.n, B * (K + 1), self.max_new_tokens + 1
        i32 = dict(device=device, dtype=torch.int32)
        look = [[int(t) for t in ids] for ids in lookup_ids]
        hist = np.zeros((B, max(len(ids) for ids in look) + cap), dtype=np.int32)
        for b, ids in enumerate(look):
            hist[b, :len(ids)] = ids
        self.hist = torch.from_numpy(hist).to(device)
        self.hist_len = torch.tensor([len(ids) for ids in look], dtype=torch.int32).to(device)
        self.drafts = torch.full((B, K), -1, **i32)
        self.n_draft = torch.zeros(B, **i32)
        self.pos_rows = torch.zeros(R, **i32)
        self.mask_rows = torch.zeros(R, **i32)
        self.blocks = (torch.arange(R, dtype=torch.int32) // n).to(device)
        self.acc = torch.zeros((B, cap), **i32)
        self.n_steps = torch.zeros(B, **i32)
        self.prompt_lengths = list(cache.lengths)
        self._len_cap = max(cache.lengths) + cap             # no sequence grows beyond it: it is done after `cap` iterations
        self._upper = max(cache.lengths)                     # upper bound of the device-resident lengths
        self.emitted, self.acc_log = None, None

    def _launches(self, bound=None):
        layers, meta, cache, _, _ = self.args
        return self._tail(decoder_verify_rows(self.x_in, layers, meta, cache, self.n, self.pos_rows, self.blocks,
                                              cache.max_len if bound is None else bound))

    def _tail(self, x, count_step=True):
        fed, pred_z = self.head(x, self.mask_rows, self.logits)
        ops.argmax_rows(self.logits, out=self.tok, ws=self.arg_ws)
        cache = self.cache
        ops.spec_verify_advance(self.tok, self.drafts, self.n_draft, self.C, self.state, self.live, self.embed, fed, pred_z, self.x_in,
                                self.tok_log, self.z_log, self.hist, self.hist_len, cache.pos_dev, cache.len_dev, self.acc, self.n_steps,
                                *self.scalars, count_step=count_step)
        ops.ngram_draft_rows(self.hist, self.hist_len, self.state, cache.pos_dev, self.K, self.N, self.C, self.embed, self.drafts,
                             self.n_draft, self.x_in, self.pos_rows, self.mask_rows)

    def _captured(self):
        """the one (graph, output), captured at the first step -- the device lengths still equal the host's then, which _capture restores
        around its warm-up --; None: eager launches.  Refuses a cache that cannot hold another n rows of the longest possible sequence."""
        cache = self.cache
        if self._upper + self.n > cache.max_len:
            raise ValueError(f"KV cache of {cache.max_len} rows cannot hold another {self.n} rows behind up to {self._upper}")
        if self.capture_ok and cache.max_len not in self.graphs:
            self._capture(cache.max_len)
        return self.graphs[cache.max_len] if self.capture_ok else None

    def _replay(self, entry):
        entry[0].replay()                                    # (the lengths move on the device alone)
        return entry[1]

    def _step(self):
        super()._step()
        self._upper = min(self._upper + self.n, self._len_cap)

    def run(self, x0):
        """x0 [B, h]: the prompt pass's last hidden row of every sequence (pre final norm).  The first iteration runs the step's tail on
        them, placed in rows (b, 0) with no drafts and without a decoder step; then up to max_new_tokens steps.  Returns (ids, pred_z) as
        GreedyLoopGraph.run does."""
        B, n = self.cache.batch, self.n
        x = torch.zeros_like(self.x_in)
        x[0::n] = x0
        self._tail(x, count_step=False)
        self._poll_loop(self.max_new_tokens)
        st, ids, pred_z = self._results()
        n_steps, acc = self.n_steps.tolist(), self.acc.cpu()
        self.cache.lengths = [m - 1 for m in self.cache.len_dev.tolist()]
        self.emitted, self.acc_log = st[2].tolist(), [acc[b, :n_steps[b]].tolist() for b in range(B)]
        return ids, pred_z


BEAM_STATE = ("running", "fin_score", "fin_flag", "fin_end", "scal", "live", "tok", "parent", "tok_log", "parent_log", "own_block")


class BeamLoopGraph(_CapturedStep):
    """HF's beam search (GenerationMixin._beam_search: one prompt, do_sample=False, no logits processors, tokens only) with the token loop
    on the device: GreedyLoopGraph's sibling.  The K beams are the K sequences of a cache whose prompt rows are stored once
    (KVCache.set_shared(L, own_rows=max_new_tokens + 1)); a beam's own rows stay where they were appended and the cache's table own_block
    says in which block each one lives, so no cache row is ever reordered.  One step is decoder_decode_row (attention through
    mm355_attn_decode_shared_idx) -> `head` (final norm and lm_head into the static fp32 `logits`; no image head) ->
    mm355_beam_select_rows_f32 (log-softmax statistics and the M best of the K * V accumulated scores) -> mm355_beam_advance (HF's
    bookkeeping, the back-pointer logs, the new table and the next input rows: beam_step_host).  The step reads no host value: ONE hipGraph
    per attention bound, replayed per token; set_variant("decode_graph", False) runs the same launches eagerly.  The host replays at most
    max_new_tokens - 1 steps and reads `live` every `poll` steps (`host_reads` counts them, the final read of the results included).  A
    finished search rides along: mm355_beam_advance writes nothing for it, so the result does not depend on `poll`.
    head(x [K, h], logits_out f32 [K, C]).  run(x0) returns beam_hypotheses_host of the final pool."""
    label = "beam"

    def __init__(self, layers, meta, cache, cos, sin, h, device, head, embed, C, max_new_tokens, eos_ids, length_penalty=1.0,
                 early_stopping=False, poll=8):
        eos = sorted(set(int(e) for e in eos_ids))
        K = cache.batch
        _refuse_loop_args(len(eos), C, embed, poll, an_id="a candidate id", beams=K)
        if early_stopping not in BEAM_EARLY_STOPPING or (isinstance(early_stopping, (int, float)) and not isinstance(early_stopping, bool)):
            raise ValueError(f"early_stopping = {early_stopping!r}: one of False, True, 'never'")
        self.max_new_tokens, self.poll, self.C = int(max_new_tokens), int(poll), int(C)
        self.M = beam_candidates(K, len(eos))
        if self.max_new_tokens < 1 or self.M > K * self.C:
            raise ValueError(f"max_new_tokens = {max_new_tokens} must be >= 1 and {K} x {C} logits must hold the {self.M} candidates of a step")
        if cache.own_block is None or cache.own_block.shape[1] < self.max_new_tokens:
            raise ValueError("the beam loop runs on a cache with a table of own rows: KVCache.set_shared(L, own_rows=max_new_tokens + 1)")
        super().__init__(layers, meta, cache, cos, sin)
        self.head, self.embed = head, embed
        self.eos, self.length_penalty, self.early_stopping = eos, float(length_penalty), BEAM_EARLY_STOPPING[early_stopping]
        host = beam_state_host(K, self.max_new_tokens)
        self.state = {n: (cache.own_block if n == "own_block" else torch.from_numpy(host[n]).to(device)) for n in BEAM_STATE}
        self.len_pow = torch.from_numpy(beam_len_pow(self.max_new_tokens, float(length_penalty))).to(device)
        self.x_in = torch.zeros((K, h), device=device, dtype=BF16)
        self.logits = torch.empty((K, self.C), device=device, dtype=torch.float32)
        self.stats = torch.zeros((K, 2), device=device, dtype=torch.float32)
        self.cand_val = torch.zeros(self.M, device=device, dtype=torch.float32)
        self.cand_idx = torch.zeros(self.M, device=device, dtype=torch.int32)
        self.sel_ws = ops.beam_select_rows_ws(K, self.C, self.M, device)
        self.host_reads = 0
        self.steps = 0
        self.on_tail = None                                  # (tests: called after every tail with the loop)

    @property
    def live(self):
        return self.state["live"]

    def _tail(self, x):
        self.head(x, self.logits)
        ops.beam_select_rows(self.logits, self.state["running"], self.M, self.stats, self.cand_val, self.cand_idx, self.sel_ws)
        ops.beam_advance(self.cand_val, self.cand_idx, self.C, self.state, self.len_pow, self.max_new_tokens, self.length_penalty,
                         self.early_stopping, self.eos, embed=self.embed, x_in=self.x_in)

    def _quiet(self):
        return self.live, 0                                  # a search that is not live logs and feeds nothing

    def run(self, x0):
        """x0 [K, h]: the prompt pass's last hidden row, K times (pre final norm): HF's step 0, whose running scores (0, -1e9, ...) let
        only the first beam through.  Then up to max_new_tokens - 1 steps.  Returns (ids, scores, flags): per pool entry, best first,
        its generated int32 ids (NumPy), and the fp32 scores and finished flags of the pool."""
        self._tail(x0.contiguous())
        if self.on_tail is not None:
            self.on_tail(self)
        self._poll_loop(self.max_new_tokens - 1, self.on_tail)
        host = {n: t.cpu().numpy() for n, t in self.state.items()}
        if host["live"][0]:                                      # pragma: no cover - the step that generates id max_new_tokens ends every search
            raise RuntimeError(f"beam loop: the search is still live after {self.steps} steps (scal {host['scal'].tolist()})")
        self.final = host
        return beam_hypotheses_host(host)


class GeluFn(Function):
    @staticmethod
    def forward(ctx, x, kind):
        ctx.save_for_backward(x)
        ctx.kind = kind
        return ops.gelu_fwd(x, kind)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return ops.gelu_bwd(x, dy.contiguous(), ctx.kind), None


class TransposeFn(Function):
    """x [R, C] -> x^T [C, Rp] (zero-padded columns when Rp > R); backward transposes the live part back."""

    @staticmethod
    def forward(ctx, x, Rp):
        ctx.R = x.shape[0]
        return transpose_padded(x, Rp) if Rp is not None else _transpose_exact(x)

    @staticmethod
    def backward(ctx, dy):
        return _transpose_exact(dy[:, :ctx.R]), None


def _transpose_exact(x2d):
    R, C = x2d.shape
    out = torch.empty((C, R), device=x2d.device, dtype=BF16)
    ops.transpose(x2d, out=out)
    return out


class PadFn(Function):
    """t [N, K] (or [N]) -> zero-padded [Np, Kp] (or [Np]): legal GEMM operand shapes for odd widths; backward slices."""

    @staticmethod
    def forward(ctx, t, Np, Kp):
        ctx.shape = tuple(t.shape)
        src = t.data if isinstance(t, torch.nn.Parameter) else t
        if t.dim() == 1:
            out = torch.zeros((Np,), device=t.device, dtype=t.dtype)
            out[:t.shape[0]].copy_(src)
        else:
            out = torch.zeros((Np, Kp), device=t.device, dtype=t.dtype)
            out[:t.shape[0], :t.shape[1]].copy_(src)
        return out

    @staticmethod
    def backward(ctx, dy):
        sl = dy[:ctx.shape[0]] if len(ctx.shape) == 1 else dy[:ctx.shape[0], :ctx.shape[1]]
        return sl.contiguous(), None, None


class LinearWBFn(Function):
    """y = x W^T + b with weight / bias passed as TENSORS (gradients returned through autograd, e.g. to PadColsFn)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return ops.gemm(x, weight, bias=bias)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = input_grad_gemm(dy, w) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w)
            weight_grad_gemm(dy, x, dw, False)
        db = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            s = torch.zeros(dy.shape[1], device=dy.device, dtype=torch.float32)
            ops.colsum_f32(dy, s)
            db = torch.empty(dy.shape[1], device=dy.device, dtype=BF16)
            ops.axpy_(db, s, None, 1.0, False)
        return dx, dw, db


class RowsPermuteFn(Function):
    """out[r] = x[fwd[r]] (fwd[r] = -1 -> zero row); backward gathers with the inverse map.  Moves a left-padded batch to the
    right-padded row layout the attention kernels take (per-sample lengths from row 0) and back."""

    @staticmethod
    def forward(ctx, x, fwd_i32, inv_i32):
        ctx.save_for_backward(inv_i32)
        return ops.rows_gather(x, fwd_i32)

    @staticmethod
    def backward(ctx, dy):
        (inv,) = ctx.saved_tensors
        return ops.rows_gather(dy.contiguous(), inv), None, None


class RowsGatherFn(Function):
    """out[r] = x[idx[r]] (idx unique, >= 0); backward scatters into a zero tensor."""

    @staticmethod
    def forward(ctx, x, idx_i32):
        ctx.save_for_backward(idx_i32)
        ctx.shape = x.shape
        return ops.rows_gather(x, idx_i32)

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        dx = torch.zeros(ctx.shape, device=dy.device, dtype=BF16)
        ops.rows_scatter_add_(dx, dy.contiguous(), idx)
        return dx, None


class CosineLossFn(Function):
    """-mean_r cos(target_r, normalize(pred_r))  (metamorph_llama.py:433-435,449-455)."""

    @staticmethod
    def forward(ctx, pred_raw, target, normalize):
        cos_sum, dpred = ops.cosine_loss(pred_raw, target, normalize, want_grad=True)
        ctx.save_for_backward(dpred)
        R = pred_raw.shape[0]
        # scalar plumbing on a 1-element tensor
        return (cos_sum * (-1.0 / R)).reshape(())

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return _scaled_copy(dpred, g), None, None


def _scaled_copy(saved, g):
    """saved * g into a FRESH tensor (a second backward through the same graph must not see a pre-scaled gradient)."""
    out = torch.empty_like(saved)
    ops.axpy_(out, saved, g.reshape(1).float().contiguous(), 1.0, False)
    return out


class MeanAbsLossFn(Function):
    """mean |target - pred|: the reference's `mse_loss_fn` (metamorph_llama.py:211-219, reached at :459 when neither
    normalize_vision nor apply_softmax is set -- the constructor default)."""

    @staticmethod
    def forward(ctx, pred, target, denom_rows=None):
        """denom_rows: the row count the reference divides by (len(target), :217) when it differs from the rows compared."""
        abs_sum, dpred = ops.mean_abs_loss(pred, target, want_grad=True)
        ctx.save_for_backward(dpred)
        R = pred.shape[0]
        ctx.scale = 1.0 if denom_rows in (None, R) else R / float(denom_rows)       # the kernel's gradient carries 1 / (R C)
        return (abs_sum * (ctx.scale / pred.numel())).reshape(())

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return _scaled_copy(dpred, g * ctx.scale if ctx.scale != 1.0 else g), None, None


class SoftCELossFn(Function):
    """-(target * log(softmax(u / 0.07) + 1e-10)).sum(1).mean(), u = F.normalize(pred) when normalize_vision
    (metamorph_llama.py:434-447)."""

    @staticmethod
    def forward(ctx, pred_raw, target, normalize):
        loss_sum, dpred = ops.soft_ce_loss(pred_raw, target, normalize, 0.07, want_grad=True)
        ctx.save_for_backward(dpred)
        return (loss_sum * (1.0 / pred_raw.shape[0])).reshape(())

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return _scaled_copy(dpred, g), None, None


class SoftmaxRowsFn(Function):
    """softmax(x / 0.07) over the feature dimension (tower side, siglip_encoder.py:210-211)."""

    @staticmethod
    def forward(ctx, x2d, temperature):
        y = ops.softmax_rows(x2d, temperature)
        ctx.save_for_backward(y)
        ctx.temperature = temperature
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return ops.softmax_rows_bwd(y, dy.contiguous(), ctx.temperature), None


# ------------------------------------------------------------------------------------------------
# splice (K6): embedding gather + image rows + zero padding
# ------------------------------------------------------------------------------------------------

class SpliceFn(Function):
    @staticmethod
    def forward(ctx, embed_weight, proj2d, embed_module, plan_dev):
        ctx.embed_module, ctx.plan = embed_module, plan_dev
        ctx.proj_shape = None if proj2d is None else proj2d.shape
        h = embed_weight.shape[1]
        return ops.splice_gather(embed_weight, proj2d, plan_dev["src"], h)

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous()
        plan, emb = ctx.plan, ctx.embed_module
        dproj = None
        if ctx.proj_shape is not None and ctx.needs_input_grad[1]:
            dproj = ops.rows_gather(dout, plan["feat_row"][: ctx.proj_shape[0]])
        w = emb.weight
        if w.requires_grad and plan["emb_tok"].numel() > 0:
            buf, acc = grad_target(w)
            if not acc:
                buf.zero_()                       # rows of tokens that do not occur keep a zero gradient
            ops.embed_grad_(buf, dout, plan["emb_tok"], plan["emb_seg"], plan["emb_pos"], True)
            commit_grad(w, buf)
        return None, dproj, None, None


class EmbeddingFn(Function):
    """Plain `embed_tokens(ids)` WITH a gradient: the text-only training path (forward(images=None): the reference's splice returns early,
    metamorph_arch.py:184-191, and HF's LlamaModel embeds the ids itself).  Backward = the splice's deterministic segmented row sum
    (`mm355_embed_grad`: rows sorted by token id on the host, from the ids' host mirror if their mover registered one -- hostmirror.py --,
    else one D2H copy; this is not the hot path)."""

    @staticmethod
    def forward(ctx, embed_weight, embed_module, ids):
        ctx.embed_module = embed_module
        ctx.ids = ids
        flat = ids.reshape(-1).to(torch.int32)
        out = ops.splice_gather(embed_weight, None, flat, embed_weight.shape[1])
        return out.view(*ids.shape, embed_weight.shape[1])

    @staticmethod
    def backward(ctx, dout):
        w = ctx.embed_module.weight
        if w.requires_grad:
            from .hostmirror import host_array
            flat = host_array(ctx.ids).reshape(-1).astype(np.int64)
            order = np.argsort(flat, kind="stable")
            sorted_tok = flat[order]
            starts = np.flatnonzero(np.concatenate(([True], sorted_tok[1:] != sorted_tok[:-1])))
            dev = dout.device
            tok = torch.from_numpy(sorted_tok[starts].astype(np.int32)).to(dev)
            seg = torch.from_numpy(np.concatenate((starts, [sorted_tok.size])).astype(np.int32)).to(dev)
            pos = torch.from_numpy(order.astype(np.int32)).to(dev)
            buf, acc = grad_target(w)
            if not acc:
                buf.zero_()
            ops.embed_grad_(buf, dout.reshape(-1, dout.shape[-1]).contiguous(), tok, seg, pos, True)
            commit_grad(w, buf)
        return None, None, None


# ------------------------------------------------------------------------------------------------
# lm_head + shifted cross entropy without materialising [M, V] logits (K13)
# ------------------------------------------------------------------------------------------------

CE_CHUNK = 8192


class LinearCrossEntropyFn(Function):
    """loss = mean over rows with a target of CE(hidden_r @ W^T, target_r) -- ONE library call (mm355_linear_ce, include/mm355.h).

    Rows without a target were already dropped by the host plan (`ce_rows`), so no flop is spent on
    ignored positions.  Inside the library, per chunk of 8192 rows: logits GEMM (bf16) -> fp32 softmax / NLL kernel that overwrites
    the logits with d loss / d logits -> the two gradient GEMMs; the per-row NLL values are summed in a fixed order (bit-reproducible
    loss).  The [M,V] fp32 logits tensor of the reference (metamorph_llama.py:398-399) never exists.
    """

    @staticmethod
    def forward(ctx, hidden, weight, head_module, plan_dev, n_valid):
        loss, dhc, dw = ops.linear_ce(hidden, plan_dev["ce_rows"], plan_dev["ce_targets"], weight, need_dh=hidden.requires_grad,
                                      need_dw=weight.requires_grad, dw_f32=n_valid > CE_CHUNK)
        ctx.head_module, ctx.plan, ctx.hidden_shape = head_module, plan_dev, hidden.shape
        ctx.save_for_backward(dhc, dw)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        dhc, dw = ctx.saved_tensors
        gs = g.reshape(1).float().contiguous()
        dh = None
        if dhc is not None:
            dh = ops.rows_gather(dhc, ctx.plan["ce_inv"])   # scatter back to [M, h] (zero rows elsewhere)
            ops.scale_(dh, gs, 1.0)
        w = ctx.head_module.weight
        if dw is not None and w.requires_grad:
            buf, acc = grad_target(w)
            ops.axpy_(buf, dw, gs, 1.0, acc)
            commit_grad(w, buf)
        return dh, None, None, None, None
