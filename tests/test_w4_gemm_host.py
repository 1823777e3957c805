"""The weight-only MXFP4 split-K GEMM (mm355_gemm_w4*), the parts that need no GPU: the exported symbols and their signatures, the validation
the C ABI does before any launch, the workspace sizes against the bf16 split-K forms, the LDS layout of the nibble B tile with the path of
the scale bytes, and the routing switch and row caps of the two quantised formats."""
import ctypes
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

I64, PTR, U32, F32, INT = ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float, ctypes.c_int
X = [PTR, I64, PTR, I64, PTR, I64, INT]                          # x, ldx, Wq, ldw_bytes, S, lds_bytes, fmt
SIGNATURES = {
    "mm355_gemm_w4_ws_floats": (I64, [I64, I64, I64]),
    "mm355_gemm_w4": (INT, X + [PTR, I64, I64, I64, I64, PTR, I64, U32, PTR, I64, PTR]),
    "mm355_gemm_w4_norm": (INT, X + [PTR, I64, I64, I64, PTR, I64, PTR, F32, PTR, PTR, I64, PTR]),
    "mm355_gemm_w4_swiglu_ws_floats": (I64, [I64, I64, I64]),
    "mm355_gemm_w4_swiglu": (INT, X + [PTR, I64, I64, I64, I64, PTR, I64, PTR]),
    "mm355_gemm_w4_rope_append": (INT, X + [PTR, I64, I64, I64, I64, I64, I64, PTR, PTR, PTR, PTR, PTR, I64, I64, PTR, I64, PTR]),
}
# (N, K) of tests/test_w4_gemm_gpu.py, with what the split-K rule makes of them at 17 .. 100 rows
GPU_SHAPES = ((136, 512), (136, 1024), (264, 1088), (520, 2048))
GPU_ROWS = (17, 32, 33, 64, 100)


def _load():
    from metamorph_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return lib, lib.load()


def test_gemm_w4_symbols_and_signatures():
    lib, L = _load()
    names = lib.exported_symbols()
    so = ctypes.CDLL(lib.LIB_PATH)
    for n, (ret, args) in SIGNATURES.items():
        assert n in names, n
        assert hasattr(so, n), n
        fn = getattr(L, n)
        assert fn.restype is ret, (n, fn.restype)
        assert len(fn.argtypes) == len(args), (n, len(fn.argtypes), len(args))
        for i, (got, want) in enumerate(zip(fn.argtypes, args)):
            assert got is want, (n, i, got, want)


def test_gemm_w4_validation_without_a_gpu():
    _, L = _load()
    P = 4096                                                     # a non-null, 16-byte aligned stand-in: no kernel is launched on the error path
    EINVAL, EUNSUPPORTED = -1, -2

    def gemm(x=P, ldx=64, wq=P, ldw=32, s=P, lds=2, fmt=2, c=P, ldc=8, M=17, N=8, K=64, res=0, ldr=0, flags=0, ws=P, nws=1 << 20):
        return L.mm355_gemm_w4(x, ldx, wq, ldw, s, lds, fmt, c, ldc, M, N, K, res, ldr, flags, ws, nws, 0)
    assert gemm(fmt=1) == EINVAL                                 # the FP8 format: not this kernel's
    assert gemm(fmt=7) == EINVAL                                 # a format that does not exist
    assert gemm(K=96, ldx=96, ldw=48, lds=3) == EINVAL           # K % 64 (a whole number of scale groups is not enough)
    assert gemm(K=32, ldx=32, ldw=16, lds=1) == EINVAL
    assert gemm(ldw=40) == EINVAL                                # ldw_bytes % 16
    assert gemm(ldw=16) == EINVAL                                # ldw_bytes < K / 2
    assert gemm(lds=1) == EINVAL                                 # lds_bytes < K / 32
    assert gemm(ldx=68) == EINVAL                                # ldx % 8
    assert gemm(s=0) == EINVAL                                   # no scale bytes
    assert gemm(wq=P + 8) == EINVAL                              # misaligned nibbles
    assert gemm(x=P + 2) == EINVAL
    assert gemm(c=P + 4) == EINVAL
    assert gemm(flags=8, res=0) == EINVAL                        # RESIDUAL without a residual
    assert gemm(flags=8, res=P + 2) == EINVAL                    # ... with a misaligned one
    assert gemm(flags=1) == EINVAL                               # a flag the w4 GEMM does not take (BIAS)
    assert gemm(M=4097) == EUNSUPPORTED                          # larger passes stay on the scratch route
    # a problem that IS split, with a workspace that is too small / missing / misaligned
    M, N, K = 20, 1024, 4096
    need = L.mm355_gemm_w4_ws_floats(M, N, K)
    assert need > 0
    big = dict(M=M, N=N, K=K, ldx=K, ldw=K // 2, lds=K // 32, ldc=N)
    assert gemm(**big, nws=need - 1) == EINVAL
    assert gemm(**big, ws=0) == EINVAL
    assert gemm(**big, ws=P + 4) == EINVAL
    W, S = K // 2, K // 32

    #                                                         C  M   N     K    res ldr norm eps Y  ws nws stream
    assert L.mm355_gemm_w4_norm(P, K, P, W, P, S, 1, P, M, N, K, 0, 0, P, 1e-5, P, P, need, 0) == EINVAL          # fmt
    assert L.mm355_gemm_w4_norm(P, K, P, W, 0, S, 2, P, M, N, K, 0, 0, P, 1e-5, P, P, need, 0) == EINVAL          # NULL S
    assert L.mm355_gemm_w4_norm(P, K, P, W, P, S - 1, 2, P, M, N, K, 0, 0, P, 1e-5, P, P, need, 0) == EINVAL      # lds_bytes < K / 32
    assert L.mm355_gemm_w4_norm(P, K, P, W, P, S, 2, P, M, N, K, 0, 0, P, 1e-5, P, P, need - 1, 0) == EINVAL
    assert L.mm355_gemm_w4_norm(P, K, P, W, P, S, 2, P, 5000, N, K, 0, 0, P, 1e-5, P, P, 1 << 40, 0) == EUNSUPPORTED
    #                                                           act ld  M  I    K    ws nws stream
    need_s = L.mm355_gemm_w4_swiglu_ws_floats(M, 512, K)
    assert L.mm355_gemm_w4_swiglu(P, K, P, W, P, S, 3, P, 512, M, 512, K, P, need_s, 0) == EINVAL
    assert L.mm355_gemm_w4_swiglu(P, K, P, W + 8, P, S, 2, P, 512, M, 512, K, P, need_s, 0) == EINVAL            # ldw_bytes % 16
    assert L.mm355_gemm_w4_swiglu(P, K, P, W - 16, P, S, 2, P, 512, M, 512, K, P, need_s, 0) == EINVAL           # ldw_bytes < K / 2
    assert L.mm355_gemm_w4_swiglu(P, K, P, W, P, S, 2, P, 512, M, 512, K, P, need_s - 1, 0) == EINVAL
    assert L.mm355_gemm_w4_swiglu(P, K, P, W, P, S, 2, P, 510, M, 510, K, P, 1 << 30, 0) == EINVAL                # I % 4 (2 I must be splittable)
    assert L.mm355_gemm_w4_swiglu(P, K, P, W, P, S, 2, P, 500, M, 512, K, P, need_s, 0) == EINVAL                 # ld_act < I
    assert L.mm355_gemm_w4_swiglu(P, K, P, W, P, S, 2, P, 512, 4097, 512, K, P, 1 << 40, 0) == EUNSUPPORTED
    #                                                                qkv ld   M  Hq Hkv d   K  cos sin pos kc vc ldkv bs  ws nws stream
    assert L.mm355_gemm_w4_rope_append(P, K, P, W, P, S, 0, P, 1024, M, 4, 2, 128, K, P, P, P, P, P, 256, 4096, P, need, 0) == EINVAL
    assert L.mm355_gemm_w4_rope_append(P, K + 32, P, W + 16, P, S + 1, 2, P, 1024, M, 4, 2, 128, K + 32, P, P, P, P, P, 256, 4096, P, need, 0) == EINVAL
    assert L.mm355_gemm_w4_rope_append(P, K + 4, P, W, P, S, 2, P, 1024, M, 4, 2, 128, K, P, P, P, P, P, 256, 4096, P, need, 0) == EINVAL   # ldx % 8
    assert L.mm355_gemm_w4_rope_append(P, K, P, W, P, S, 2, P, 1024, M, 4, 2, 128, K, P, P, P, P, P, 256, 4096, P, need - 1, 0) == EINVAL
    assert L.mm355_gemm_w4_rope_append(P, K, P, W, P, S, 2, P, 1024, 4097, 4, 2, 128, K, P, P, P, P, P, 256, 4096, P, 1 << 40, 0) == EUNSUPPORTED
    # the 16-row GEMV keeps its own limit
    assert L.mm355_gemv_w4(P, 64, P, 32, P, 2, 2, P, 64, 17, 8, 64, 0, 0, 0, 0, 0) == EUNSUPPORTED


def test_gemm_w4_workspaces_equal_the_bf16_split_k_forms():
    _, L = _load()
    split = 0
    shapes = ((6144, 4096), (4096, 4096), (4096, 14336), (28672, 4096), (128256, 4096), (1536, 1024), (1024, 2048), (4096, 1024)) + GPU_SHAPES
    for M in (1, 17, 20, 32, 33, 64, 100, 512, 1024, 2048, 4096):
        for (N, K) in shapes:
            ref = L.mm355_gemm_splitk_ws_floats(M, N, K)
            assert L.mm355_gemm_w4_ws_floats(M, N, K) == ref, (M, N, K)
            split += ref > 0
            if N % 2 == 0:
                assert L.mm355_gemm_w4_swiglu_ws_floats(M, N // 2, K) == L.mm355_gemm_splitk_swiglu_ws_floats(M, N // 2, K), (M, N, K)
    assert split > 20
    for M in GPU_ROWS:                                           # what the GPU tests claim of their shapes: S * M * N floats
        assert [L.mm355_gemm_w4_ws_floats(M, N, K) // (M * N) for (N, K) in GPU_SHAPES] == [0, 2, 2, 4], M
        for I in (68, 260):
            assert L.mm355_gemm_w4_swiglu_ws_floats(M, I, 1024) == 2 * M * 2 * I, (M, I)


@pytest.mark.parametrize("BM", [32, 64])
def test_b_tile_layout_is_conflict_free_and_complete(BM):
    """The nibble B tile of gemm_wq_kernel<W4, BM> (W4::Lane, csrc/gemm_w4.hip) in LDS: 128 weight rows x 32 bytes behind the x tile, written by LDS-DMA in
    1-KiB pieces (one per wave: lane L -> piece byte 16 L, row L >> 1, slot L & 1, source chunk (L & 1) ^ ((row >> 3) & 1)), read by one
    ds_read_b64 per lane and fragment, of which the lane keeps dword fq & 1.  ds_read_b64 is served per 32-lane half with
    bank = (byte / 4) % 64 and lanes that read the same address are served together: in every half of every fragment read the DISTINCT
    addresses must touch each bank at most once, and a lane must find the nibbles k = kk*32 + fq*8 .. +7 of weight row wn*32 + j*16 + fr in
    the dword it keeps.  The scale byte it widens them with must be S[n][k0/32 + kk] of that row.

    A Python MODEL of the address formulae, not a run of the kernel: it needs no GPU.  What ties it to the kernel is the source check below
    -- the expressions the model restates must still be the ones in the file -- and tests/test_w4_gemm_gpu.py, where a nibble or a scale
    byte taken from anywhere else breaks the bit-for-bit and every-code tests."""
    src = open(os.path.join(REPO, "metamorph_amd", "csrc", "gemm_w4.hip")).read()
    for expr in ("const int rb = lane >> 1;", "const int cb = (lane & 1) ^ ((rb >> 3) & 1);", "const int bx = (fr >> 3) & 1;",
                 "A_BYTES + (wn * TN + fr) * 32 + (fq >> 1) * 8", "int b_off1 = b_off + 512;", "const int bsw0 = bx << 4;",
                 "const int bsw1 = (1 ^ bx) << 4;", "B_BYTES = BN * 32", "const bool odd = (fq & 1) != 0;", "odd ? q.y : q.x",
                 "srcB = Wb + (int64_t)min(n0 + wave_s * 32 + rb, N - 1) * w.ldw + cb * 16;", "(lptr_t)(sb + A_BYTES), 16, 0, 0);",
                 "srcS[j] = Sb + (int64_t)min(n0 + wn * TN + j * 16 + fr, N - 1) * w.lds;", "__builtin_memcpy(&v, srcS[j] + 2 * kt, 2);",
                 "e8m0_to_f32(kk ? sc[j] >> 8 : sc[j] & 0xffu)", "unsigned char* sb = smem + buf * STAGE + wave_s * 1024;"):
        assert expr in src, expr
    A_BYTES = BM * 128
    image = {}                                                   # LDS byte (relative to the stage) -> (row, byte of the row's 32 in this K tile)
    for wave in range(4):                                        # gdma: the piece of wave w at stage + A_BYTES + w * 1024, rows w*32 ..
        for lane in range(64):
            rb = lane >> 1
            cb = (lane & 1) ^ ((rb >> 3) & 1)
            for b in range(16):
                image[A_BYTES + wave * 1024 + lane * 16 + b] = (wave * 32 + rb, cb * 16 + b)
    assert len(image) == 128 * 32 and len(set(image.values())) == 128 * 32
    assert min(image) == A_BYTES and max(image) == A_BYTES + 128 * 32 - 1
    seen = set()
    for wn in range(4):
        for j in range(2):
            for kk in range(2):
                for half in range(2):
                    addrs = set()
                    for lane in range(half * 32, half * 32 + 32):
                        fr, fq = lane & 15, lane >> 4
                        bx = (fr >> 3) & 1
                        addr = A_BYTES + (wn * 32 + fr) * 32 + (fq >> 1) * 8 + j * 512 + ((kk ^ bx) << 4)
                        assert addr % 8 == 0
                        keep = addr + 4 * (fq & 1)               # odd ? q.y : q.x
                        row = wn * 32 + j * 16 + fr
                        for b in range(4):                       # byte b of the dword: k = kk*32 + fq*8 + 2b (low nibble), + 1 (high nibble)
                            assert image[keep + b] == (row, (kk * 32 + fq * 8) // 2 + b), (wn, j, kk, lane, b)
                            seen.add((row, kk * 32 + fq * 8 + 2 * b))
                            seen.add((row, kk * 32 + fq * 8 + 2 * b + 1))
                        addrs.add(addr)
                    assert len(addrs) == 16                      # lanes fq and fq ^ 1 of a row: one address
                    banks = [b for a in addrs for b in ((a // 4) % 64, (a // 4 + 1) % 64)]
                    assert len(banks) == len(set(banks)) == 32, (wn, j, kk, half, sorted(banks))
    assert len(seen) == 128 * 64                                 # every (row, k) nibble of the tile is fetched by some lane
    # the scale bytes: little-endian 16-bit word at S[n] + (slice offset + k0) / 32, byte kk of it for k-step kk
    for kslice, sl, kt in ((0, 0, 0), (0, 0, 5), (576, 1, 0), (576, 1, 7), (1024, 3, 15)):
        k0 = sl * kslice + kt * 64                               # first k of the tile in the whole row
        word_at = ((sl * kslice) >> 5) + 2 * kt
        for kk in range(2):
            assert word_at + kk == k0 // 32 + kk


def _cpu_model(fmt):
    from metamorph_amd.factory import build_model
    llm = dict(hidden_size=1024, intermediate_size=2048, num_hidden_layers=1, num_attention_heads=8, num_key_value_heads=2, vocab_size=320,
               rms_norm_eps=1e-5, rope_theta=500000.0)
    geo = dict(hidden_size=64, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14)
    model = build_model(llm, geo, num_image_tokens=4, max_length=64)
    model.quantize_decoder_(fmt=fmt)
    return model.model.layers[0]


def test_routing_switch_and_caps_belong_to_the_format(monkeypatch):
    from metamorph_amd import functional as F, ops
    assert F.VARIANTS["w4_gemm"] is True and F.W4Layer.ON_GEMM is True
    assert F.W4_GEMM_UNSPLIT_MAX_ROWS == {"qkv": 0, "o": 0, "gu": 0, "down": 0}            # unmeasured shapes stay on the scratch route
    assert set(F.W4_GEMM_MAX_ROWS) == set(F.W8Layer.NAMES) and all(v in (0, 4096) or 0 < v < 4096 for v in F.W4_GEMM_MAX_ROWS.values())
    w4, w8 = _cpu_model("mxfp4"), _cpu_model("fp8_e4m3")
    assert isinstance(w4.w8, F.W4Layer) and not isinstance(w8.w8, F.W4Layer)
    for (N, K) in ((1536, 1024), (1024, 1024), (4096, 1024), (1024, 2048)):
        assert ops.gemm_splitk_splits(20, N, K), (N, K)
    every = frozenset(F.W8Layer.NAMES)
    monkeypatch.setattr(F, "W4_GEMM_MAX_ROWS", {n: 4096 for n in every})
    monkeypatch.setattr(F, "W4_GEMM_UNSPLIT_MAX_ROWS", {n: 0 for n in every})
    monkeypatch.setattr(F, "W8_GEMM_MAX_ROWS", {n: 4096 for n in every})
    monkeypatch.setattr(F, "W8_GEMM_UNSPLIT_MAX_ROWS", {n: 0 for n in every})
    for v4 in (True, False):
        for v8 in (True, False):
            monkeypatch.setitem(F.VARIANTS, "w4_gemm", v4)
            monkeypatch.setitem(F.VARIANTS, "w8_gemm", v8)
            assert F.w8_on_gemm(w4, 20) == (every if v4 else frozenset()), (v4, v8)
            assert F.w8_on_gemm(w8, 20) == (every if v8 else frozenset()), (v4, v8)
    monkeypatch.setitem(F.VARIANTS, "w4_gemm", True)
    monkeypatch.setitem(F.VARIANTS, "w8_gemm", True)
    assert F.w8_on_gemm(w4, 4097) == frozenset()                 # beyond the kernel's rows
    assert F.w8_on_gemm(w4, 100, gu_rows=64) == every - {"gu"}   # the prompt pass's own limit for gate|up
    # each format reads ITS table
    monkeypatch.setattr(F, "W4_GEMM_MAX_ROWS", {"qkv": 4096, "o": 0, "gu": 4096, "down": 4096})
    assert F.w8_on_gemm(w4, 20) == every - {"o"} and F.w8_on_gemm(w8, 20) == every
    monkeypatch.setattr(F, "W8_GEMM_MAX_ROWS", {"qkv": 0, "o": 4096, "gu": 4096, "down": 4096})
    assert F.w8_on_gemm(w4, 20) == every - {"o"} and F.w8_on_gemm(w8, 20) == every - {"qkv"}
    # the records carry their own GEMM ops
    assert F.W4Layer.gemm is ops.gemm_w4 and F.W4Layer.gemm_norm is ops.gemm_w4_norm and F.W4Layer.gemm_swiglu is ops.gemm_w4_swiglu
    assert F.W4Layer.gemm_rope_append is ops.gemm_w4_rope_append and F.W4Layer.gemm_supported is ops.gemm_w4_supported
    assert F.W8Layer.gemm is ops.gemm_w8 and F.W8Layer.gemm_norm is ops.gemm_w8_norm and F.W8Layer.gemm_swiglu is ops.gemm_w8_swiglu
    assert F.W8Layer.gemm_rope_append is ops.gemm_w8_rope_append and F.W8Layer.gemm_supported is ops.gemm_w8_supported
