"""The heads of cached generation without a GPU: which ops `_rows_logits`, `_head_text_rows`, `_head_row` and `_head_rows_device` launch, on
which operand shapes and into which output dtype, for every row count at which the lm_head dispatch changes its route, the bf16 and the
quantised lm_head, VARIANTS["w8_gemm"] on and off, and the image head with normalize_vision / apply_softmax on and off.  The ops are
replaced by recorders that return tensors of the right shape and dtype; the expected sequences are literals."""
import pytest
import torch

BF16 = torch.bfloat16
H, HV, V = 64, 32, 320                                       # hidden size, image-feature width, vocabulary of the tiny model
ROWS = (1, 4, 16, 17, 32, 33)
NAMES = {torch.bfloat16: "bf16", torch.float32: "f32", torch.uint8: "u8", torch.int32: "i32"}

# the lm_head's launches per (lm_head, rows); {n}: the row count
GEMV = ("gemv ({n},64),(320,64) -> f32({n},320)",)
GEMM = ("gemm ({n},64),(320,64) -> f32({n},320)",)
GEMV_W8 = ("gemv_w8 ({n},64),(320,64),(320) -> f32({n},320)",)
GEMM_W8 = ("gemm_w8 ({n},64),(320,64),(320) -> f32({n},320)",)
DEQUANT = ("dequant_w8 (320,64),(320) -> bf16(320,64)", "gemm ({n},64),(320,64) -> f32({n},320)")
LM_HEAD = {
    # a bf16 lm_head too narrow for the 17 .. 32 row GEMV (ops.gemv_rows32_units), and one wide enough (the real one is)
    "bf16": {1: GEMV, 4: GEMV, 16: GEMV, 17: GEMM, 32: GEMM, 33: GEMM},
    "bf16_wide": {1: GEMV, 4: GEMV, 16: GEMV, 17: GEMV, 32: GEMV, 33: GEMM},
    # a quantised lm_head with VARIANTS["w8_gemm"] on, off, and on where ops.gemm_w8_supported says no
    "w8": {1: GEMV_W8, 4: GEMV_W8, 16: GEMV_W8, 17: GEMM_W8, 32: GEMM_W8, 33: GEMM_W8},
    "w8_gemm_off": {1: GEMV_W8, 4: GEMV_W8, 16: GEMV_W8, 17: DEQUANT, 32: DEQUANT, 33: DEQUANT},
    "w8_unsupported": {16: GEMV_W8, 17: DEQUANT},
}
CASES = [(fmt, n) for fmt, table in LM_HEAD.items() for n in table]

NORM = ("rmsnorm_fwd ({n},64),(64) -> bf16({n},64)",)
# the image head; {lin}: F.linear's route, gemv up to 16 rows (these weights are narrow) and the GEMM beyond
VISION_HEAD = ("{lin} ({n},64),(32,64)+bias -> bf16({n},32)",)
NORMALIZE = ("bilinear_l2norm ({n},1,32) 1 1 True -> bf16({n},1,32)",)
SOFTMAX = ("softmax_rows ({n},32) 0.07 -> bf16({n},32)",)
PROJECTOR = ("{lin} ({n},32),(64,32)+bias -> bf16({n},64)", "gelu_fwd ({n},64) -> bf16({n},64)", "{lin} ({n},64),(64,64)+bias -> bf16({n},64)")
SELECT = ("rows_select ({n}),({n},64),({n},64) -> bf16({n},64)",)


def _image_head(normalize, softmax):
    return VISION_HEAD + (NORMALIZE if normalize else ()) + (SOFTMAX if softmax else ()) + PROJECTOR


def _lines(templates, n):
    return [t.format(n=n, lin="gemv" if n <= 16 else "gemm") for t in templates]


@pytest.fixture(scope="module")
def model():
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=H, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=V,
               rms_norm_eps=1e-5, rope_theta=500000.0)
    geo = dict(hidden_size=HV, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14)
    return build_model(llm, geo, num_image_tokens=4, max_length=64, vision_head="None").eval()


class _Recorder:
    """stands in for the ops the heads reach: every call is logged as 'name operand shapes -> dtype(shape)' and returns an empty tensor"""

    def __init__(self, monkeypatch, wide_head, w8_supported):
        from metamorph_amd import ops
        self.log, self.last = [], None
        self.wide_head, self.w8_supported = wide_head, w8_supported
        for name in ("rmsnorm_fwd", "gemm", "gemv", "gemv_w8", "gemm_w8", "dequant_w8", "gelu_fwd", "bilinear_l2norm", "softmax_rows",
                     "rows_select", "gemv_supported", "gemm_w8_supported"):
            monkeypatch.setattr(ops, name, getattr(self, name))

    def _note(self, name, operands, out, extra=""):
        shapes = ",".join("(" + ",".join(str(s) for s in t.shape) + ")" for t in operands)
        self.log.append(f"{name} {shapes}{extra} -> {NAMES[out.dtype]}({','.join(str(s) for s in out.shape)})")
        self.last = out
        return out

    def _matmul(self, name, operands, rows, cols, out, f32, bias=None):
        if out is None:
            out = torch.empty((rows, cols), dtype=torch.float32 if f32 else BF16)
        assert tuple(out.shape) == (rows, cols)
        return self._note(name, operands, out, "+bias" if bias is not None else "")

    # (the predicates decide, they launch nothing: not logged)
    def gemv_supported(self, x, w):
        return x.shape[0] <= 16 or (x.shape[0] <= 32 and self.wide_head and w.shape[0] == V)

    def gemm_w8_supported(self, M, K):
        return self.w8_supported

    def rmsnorm_fwd(self, x, w, eps):
        return self._note("rmsnorm_fwd", (x, w), torch.empty_like(x))

    def gemm(self, a, b, out=None, *, bias=None, out_f32=False):
        assert a.dtype == BF16 and b.dtype == BF16
        return self._matmul("gemm", (a, b), a.shape[0], b.shape[0], out, out_f32, bias)

    def gemv(self, x, w, out=None, bias=None):
        assert x.dtype == BF16 and w.dtype == BF16 and x.shape[0] <= 32
        return self._matmul("gemv", (x, w), x.shape[0], w.shape[0], out, False, bias)

    def gemv_w8(self, x, q, scale, out=None):
        assert x.shape[0] <= 16
        return self._matmul("gemv_w8", (x, q, scale), x.shape[0], q.shape[0], out, False)

    def gemm_w8(self, x, q, scale, residual=None, out=None, out_f32=False):
        assert residual is None
        return self._matmul("gemm_w8", (x, q, scale), x.shape[0], q.shape[0], out, out_f32)

    def dequant_w8(self, q, scale, out=None):
        assert out is None and q.dtype == torch.uint8
        return self._note("dequant_w8", (q, scale), torch.empty(q.shape, dtype=BF16))

    def gelu_fwd(self, x, kind):
        return self._note("gelu_fwd", (x,), torch.empty_like(x))

    def bilinear_l2norm(self, feat, side_in, side_out, normalize):
        assert feat.is_contiguous()
        return self._note("bilinear_l2norm", (feat,), torch.empty_like(feat), f" {side_in} {side_out} {normalize}")

    def softmax_rows(self, x, temperature=0.07):
        assert x.is_contiguous()
        return self._note("softmax_rows", (x,), torch.empty_like(x), f" {temperature}")

    def rows_select(self, mask, a, b, out=None):
        assert out is None and mask.dtype == torch.int32
        return self._note("rows_select", (mask, a, b), torch.empty_like(a))


@pytest.fixture
def record(model, monkeypatch):
    """record(fmt) -> the recorder, with the model's lm_head and VARIANTS["w8_gemm"] set up for the LM_HEAD table's row `fmt`"""
    from metamorph_amd import functional as F

    def start(fmt):
        if fmt.startswith("w8"):
            monkeypatch.setattr(model, "w8_lm_head", (torch.zeros((V, H), dtype=torch.uint8), torch.ones(V)), raising=False)
        monkeypatch.setitem(F.VARIANTS, "w8_gemm", fmt != "w8_gemm_off")
        return _Recorder(monkeypatch, wide_head=fmt == "bf16_wide", w8_supported=fmt != "w8_unsupported")
    return start


@pytest.mark.parametrize("fmt,n", CASES)
def test_rows_logits_and_the_text_head(model, record, fmt, n):
    rec = record(fmt)
    rows = torch.zeros((n, H), dtype=BF16)
    with torch.no_grad():
        logits = model._rows_logits(rows)
        assert rec.log == _lines(NORM + LM_HEAD[fmt][n], n)
        assert logits is rec.last and logits.dtype == torch.float32 and tuple(logits.shape) == (n, V)
        del rec.log[:]
        logits, hid = model._rows_logits(rows, return_hidden=True)
        assert rec.log == _lines(NORM + LM_HEAD[fmt][n], n)
        assert logits is rec.last and hid.dtype == BF16 and tuple(hid.shape) == (n, H)
        del rec.log[:]
        out = torch.empty((n, V), dtype=torch.float32)
        assert model._head_text_rows(rows, out) is None
        assert rec.log == _lines(NORM + LM_HEAD[fmt][n], n) and rec.last is out


@pytest.mark.parametrize("fmt,n", CASES + [("bf16", 3), ("w8", 3)])
def test_head_rows_device(model, record, fmt, n):
    rec = record(fmt)
    x, mask, out = torch.zeros((n, H), dtype=BF16), torch.zeros(n, dtype=torch.int32), torch.empty((n, V), dtype=torch.float32)
    lm_head = LM_HEAD[fmt][n] if n != 3 else LM_HEAD[fmt][4]
    for normalize, softmax in ((False, False), (True, False), (False, True), (True, True)):
        model.normalize_vision, model.apply_softmax = normalize, softmax
        del rec.log[:]
        with torch.no_grad():
            fed, pred_z = model._head_rows_device(x, mask, out)
        assert rec.log == _lines(NORM + _image_head(normalize, softmax) + SELECT + lm_head, n), (normalize, softmax)
        assert rec.last is out and fed.dtype == BF16 and tuple(fed.shape) == (n, H)
        assert pred_z.dtype == BF16 and tuple(pred_z.shape) == (n, HV)


@pytest.mark.parametrize("fmt", ["bf16", "bf16_wide", "w8", "w8_gemm_off"])
def test_head_row_in_both_modes(model, record, fmt):
    rec = record(fmt)
    x = torch.zeros((1, H), dtype=BF16)
    logits, hid, pred_z = model._head_row(x, False)
    assert rec.log == _lines(NORM + LM_HEAD[fmt][1], 1)
    assert logits is rec.last and tuple(logits.shape) == (1, V) and tuple(hid.shape) == (1, H) and pred_z is None
    for normalize, softmax in ((False, False), (True, False), (False, True), (True, True)):
        model.normalize_vision, model.apply_softmax = normalize, softmax
        del rec.log[:]
        logits, hid, pred_z = model._head_row(x, True)
        assert rec.log == _lines(NORM + _image_head(normalize, softmax) + LM_HEAD[fmt][1], 1), (normalize, softmax)
        assert logits is rec.last and logits.dtype == torch.float32 and tuple(logits.shape) == (1, V)
        assert tuple(hid.shape) == (1, H) and pred_z.dtype == BF16 and tuple(pred_z.shape) == (1, HV)


def test_the_hooks_are_looked_up_on_the_instance(model, record, monkeypatch):
    """tests and tools replace the heads on a model instance: whoever calls them finds them through `self` at call time"""
    rec = record("bf16")
    seen = []
    monkeypatch.setattr(model, "_rows_logits", lambda rows, return_hidden=False: seen.append("rows") or (rows, rows), raising=False)
    monkeypatch.setattr(model, "_decode_batch", lambda x, cache: x, raising=False)
    from metamorph_amd.model.language_model.metamorph_llama import HipKVCache
    cache = HipKVCache()
    cache.kv, cache.pads = object(), [0]                         # (a filled cache of one sequence: the step of HF generate())
    model._cached_forward(None, torch.zeros((1, 1, H), dtype=BF16), None, cache, False)
    assert seen == ["rows"] and rec.log == []
