"""Test infrastructure for the kernels that write contraction-major ("transposed") copies: mm355_transpose_bf16, mm355_rmsnorm_apply_t,
mm355_swiglu_bwd_t and mm355_gemm_swiglu_bwd_bf16.  Plain torch, runs on whichever device it is asked for; nothing here is derived from a
kernel's output.  tests/test_transposed_refs_host.py asserts every construction below on the CPU.

  framed            an output view inside a flat sentinel-filled buffer, with a check that nothing outside the view was written
  random_bits       uniformly random 16-bit patterns as bf16 (NaN payloads, +-0, subnormals, infinities): the transposes copy bits
  apply_t_inputs    x, w and an ARBITRARY positive fp32 rstd for rmsnorm_apply_t
  apply_t_ref       its bit-exact torch reference
  swb_*             the cases, the probe channels and the operands of the fused SwiGLU-backward GEMM
"""
import torch

import helper_refs as H

BF16 = torch.bfloat16
GUARD = 4096                         # sentinel elements before and after every framed view
SENTINELS = (0x5A5B, 0xC3A7)         # two finite bf16 patterns: a call is run once over each and the reference's bits are required both
#                                      times, so an element the kernel never wrote shows as a sentinel in at least one of the two runs


def ceil8(n):
    return (n + 7) // 8 * 8


def ragged_ld(n):
    """the smallest leading dimension >= n that is not a multiple of 8 (the scalar-store branches)"""
    return n if n % 8 else n + 1


def _i16(pattern):
    return pattern - 65536 if pattern >= 32768 else pattern


class Framed:
    """A [rows, cols] bf16 view with leading dimension ld inside one flat buffer filled with `sentinel`: at least GUARD elements before
    and after it, its first element `misalign` elements past a 16-byte boundary (0: aligned)."""

    def __init__(self, shape, ld, sentinel, device="cpu", misalign=0):
        rows, cols = shape
        assert ld >= cols and rows > 0 and cols > 0 and 0 <= misalign < 8
        self.rows, self.cols, self.ld, self.sentinel = rows, cols, ld, sentinel
        n = GUARD + 8 + rows * ld + GUARD
        self.bits = torch.full((n,), _i16(sentinel), dtype=torch.int16, device=device)
        self.buf = self.bits.view(BF16)
        base = self.buf.data_ptr()
        assert base % 2 == 0
        self.start = GUARD + (-(base // 2 + GUARD)) % 8 + misalign
        self.view = self.buf.as_strided((rows, cols), (ld, 1), self.start)
        assert (self.view.data_ptr() - 2 * misalign) % 16 == 0 and self.view.data_ptr() == base + 2 * self.start

    def outside(self):
        """bool mask over the flat buffer: True at every element that is not an element of the view (both guards and the ld - cols gap
        behind every row, the last included)"""
        m = torch.ones(self.bits.numel(), dtype=torch.bool, device=self.bits.device)
        m.as_strided((self.rows, self.cols), (self.ld, 1), self.start).fill_(False)
        return m

    def check_untouched(self, what=""):
        """every element outside the view is still the sentinel.  Looks at the two guards and the gaps as three views (no mask of the size
        of the buffer: the 2 GiB case); the message, built on a failure only, says where."""
        s, end = _i16(self.sentinel), self.start + self.rows * self.ld
        ok = (self.bits[:self.start] == s).all() & (self.bits[end:] == s).all()
        if self.ld > self.cols:
            ok = ok & (self.bits.as_strided((self.rows, self.ld - self.cols), (self.ld, 1), self.start + self.cols) == s).all()
        if bool(ok):
            return
        bad = self.outside() & (self.bits != s)
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            rel = i - self.start
            raise AssertionError(f"{what}: {int(bad.sum())} elements outside the [{self.rows}, {self.cols}] view (ld {self.ld}) were written; first at "
                                 f"flat offset {rel} from the view's start (row {rel // self.ld}, column {rel % self.ld}): "
                                 f"{int(self.bits[i]) & 0xFFFF:#06x}, sentinel {self.sentinel:#06x}")

    def check_all_sentinel(self, what=""):
        bad = self.bits != _i16(self.sentinel)
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements written by a call that was refused"


def framed(shape, ld, sentinel, device="cpu", misalign=0):
    return Framed(shape, ld, sentinel, device, misalign)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def within(got, ref, bound, what):
    """|got - ref| <= bound on every element, in fp64 (the check of tests/test_helpers_gpu.py)"""
    got, ref = got.to(H.F64), ref.to(H.F64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= bound)                                       # a NaN anywhere is bad
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        b = bound if bound.dim() == 0 else bound.expand_as(err)[i]
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} outside the bound; first at {i}: got {float(got[i]):.9g} "
                             f"ref {float(ref[i]):.9g} bound {float(b):.3g}")


# ------------------------------------------------------------------------------------------------ A. transposes

def random_bits(rows, cols, ld=None, seed=0, device="cpu"):
    """[rows, cols] view (leading dimension ld) of uniformly random 16-bit patterns seen as bf16; the columns [cols, ld) hold random
    patterns too and must never be copied.  Up to 2^24 elements are drawn on the host (the same on every device, so the host test speaks
    about what the GPU test runs); the 2 GiB case is drawn on the device it is asked for."""
    ld = cols if ld is None else ld
    gen_dev = "cpu" if rows * ld <= 2 ** 24 else device
    g = torch.Generator(device=gen_dev).manual_seed(seed)
    flat = torch.randint(-32768, 32768, (rows * ld,), generator=g, dtype=torch.int16, device=gen_dev).to(device)
    return flat.view(BF16).as_strided((rows, cols), (ld, 1), 0)


TRANSPOSE_ROWS = (1, 7, 8, 9, 63, 64, 65, 130)
TRANSPOSE_COLS = (1, 7, 8, 9, 63, 64, 65, 203)


def transpose_grid():
    """(rows, cols, ld_in, ld_out) of the small cases: cols % 8 != 0 is the scalar-load branch, a ragged ld_out the scalar-store branch"""
    for rows in TRANSPOSE_ROWS:
        for cols in TRANSPOSE_COLS:
            for ld_in in (ceil8(cols), ceil8(cols) + 8):
                for ld_out in (ceil8(rows), ceil8(rows) + 8, ragged_ld(rows)):
                    yield rows, cols, ld_in, ld_out


# ------------------------------------------------------------------------------------------------ B. rmsnorm_apply_t

APPLY_T_M = (1, 8, 63, 65, 300)
APPLY_T_H = (8, 64, 72, 1160)


def apply_t_inputs(M, h, device="cpu"):
    """x [M, h] ~ 1.5 N(0, 1), w [h] ~ 1 + 0.1 N(0, 1) (bf16) and rstd [M]: fp32 values log-uniform in [1/8, 8) with all 24 significand
    bits in use -- NOT the rstd of x: the kernel is handed the numbers and has to use row r's for row r."""
    g = torch.Generator().manual_seed(1000 * M + h)
    x = (torch.randn(M, h, generator=g) * 1.5).to(BF16)
    w = (1.0 + 0.1 * torch.randn(h, generator=g)).to(BF16)
    rstd = torch.exp2(torch.rand(M, generator=g, dtype=torch.float64) * 6.0 - 3.0).to(torch.float32)
    return x.to(device), w.to(device), rstd.to(device)


def apply_t_ref(x, w, rstd):
    """(w * bf16(x * rstd))^T, [h, M]: two fp32 multiplications of bf16 / fp32 operands, each followed by RNE to bf16.  An IEEE
    multiplication has one correctly rounded result and nothing can be contracted across the rounding between them, so these are the
    kernel's bits."""
    return (w.float() * (x.float() * rstd[:, None]).bfloat16().float()).bfloat16().t()


def apply_t_ref64(x, w, rstd):
    """the same in fp64 with helper_refs.round_bf at the two rounding points; the first product (8 x 24 significand bits) is exact in fp64
    and is rounded to fp32 first, as the one fp32 multiplication rounds it.  Returns (y^T, x * rstd in fp32, its bf16 rounding)."""
    t32 = (x.to(H.F64) * rstd.to(H.F64)[:, None]).to(torch.float32).to(H.F64)
    t = H.round_bf(t32)
    return H.round_bf(w.to(H.F64) * t).t(), t32, t


# ------------------------------------------------------------------------------------------------ D. fused SwiGLU-backward GEMM

# (M, I, K, ld_gu - 2 I, ld_dgu - 2 I, ldT - M)
SWB_CASES = [
    (8, 64, 128, 0, 0, 0),          # 1: one live 8-row vector, one live wave column
    (264, 64, 128, 0, 0, 0),        # 2: second row tile with 8 live rows
    (200, 192, 256, 8, 16, 56),     # 3: M % 64 != 0, wave column 3 outside I, every leading dimension padded
    (392, 320, 128, 0, 0, 0),       # 4: 2 x 2 tiles (total & 7 == 4); in the last row tile wm = 1 has 8 live rows
    (520, 576, 384, 0, 0, 120),     # 5: 3 x 3 tiles (total & 7 == 1, one raster group shorter than gm), three K-tile pairs
    (1288, 704, 128, 0, 0, 0),      # 6: ntm = 6: raster groups of 4 and 2
    (1800, 256, 128, 0, 0, 0),      # 7: ntm = 8, ntn = 1, last tile 8 rows
    (2624, 4672, 128, 0, 0, 0),     # 8: the smallest problem gemm_swiglu_bwd_supported admits, 11 x 19 = 209 tiles
]
PROBE_GATE = 1.28125                 # silu = 1.00279: rounds to bf16 1.0, 1.1e-3 away from the tie at 1 + 2^-8
EXACT_MAX = 256                      # integers up to here are bf16 values


def probe_channels(I, device="cpu"):
    return torch.arange(5, I, 16, device=device)


def swb_gu(M, I, ld_gu, seed, device="cpu"):
    """gu [M, 2 I] (leading dimension ld_gu, NaN in the gap) ~ 1.5 N(0, 1) with the gate of every channel c % 16 == 5 set to PROBE_GATE:
    there the kernel's bf16 silu is exactly 1, so the up half of dgu is the bf16 d act the epilogue formed and actT[c] is u[:, c]"""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((M, ld_gu), float("nan"), dtype=BF16)
    buf[:, :2 * I] = (torch.randn(M, 2 * I, generator=g) * 1.5).to(BF16)
    buf[:, probe_channels(I)] = PROBE_GATE
    return buf.to(device)[:, :2 * I]


def swb_operands(M, I, K, seed, exact, device="cpu"):
    """dy [M, K], wdT [I, K].  exact: entries from {-1, 0, 1}, so that every d act is an integer which every summation order gives
    exactly; else N(0, 1) (the scales of test_gemm_fp32_output_tight)."""
    g = torch.Generator().manual_seed(seed)
    if exact:
        dy = torch.randint(-1, 2, (M, K), generator=g).to(BF16)
        wdT = torch.randint(-1, 2, (I, K), generator=g).to(BF16)
    else:
        dy = torch.randn(M, K, generator=g).to(BF16)
        wdT = torch.randn(I, K, generator=g).to(BF16)
    return dy.to(device), wdT.to(device)


def swb_seed(case_index, exact):
    return 100 * (case_index + 1) + (7 if exact else 3)


def dact64(dy, wdT):
    return dy.to(H.F64) @ wdT.to(H.F64).t()
