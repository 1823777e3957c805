"""The weight-only FP8 split-K GEMM (mm355_gemm_w8*), the parts that need no GPU: the exported symbols and their signatures, the validation
the C ABI does before any launch, the workspace sizes against the bf16 split-K forms, and the LDS layout of the byte B tile."""
import ctypes
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

I64, PTR, U32, F32, INT = ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float, ctypes.c_int
X = [PTR, I64, PTR, I64, PTR, INT]                                # x, ldx, Wq, ldw_bytes, scale, fmt
SIGNATURES = {
    "mm355_gemm_w8_ws_floats": (I64, [I64, I64, I64]),
    "mm355_gemm_w8": (INT, X + [PTR, I64, I64, I64, I64, PTR, I64, U32, PTR, I64, PTR]),
    "mm355_gemm_w8_norm": (INT, X + [PTR, I64, I64, I64, PTR, I64, PTR, F32, PTR, PTR, I64, PTR]),
    "mm355_gemm_w8_swiglu_ws_floats": (I64, [I64, I64, I64]),
    "mm355_gemm_w8_swiglu": (INT, X + [PTR, I64, I64, I64, I64, PTR, I64, PTR]),
    "mm355_gemm_w8_rope_append": (INT, X + [PTR, I64, I64, I64, I64, I64, I64, PTR, PTR, PTR, PTR, PTR, I64, I64, PTR, I64, PTR]),
}


def _load():
    from metamorph_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return lib, lib.load()


def test_gemm_w8_symbols_and_signatures():
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
    # (a check of the header's TEXT only: where the scale is applied is part of the documented contract.  That the kernels apply it there is
    # what tests/test_w8_gemm_gpu.py checks, bit for bit)
    text = open(os.path.join(REPO, "include", "mm355.h")).read()
    assert "sum_s scale[n] * P_s" in text


def test_gemm_w8_validation_without_a_gpu():
    _, L = _load()
    P = 4096                                                     # a non-null, 16-byte aligned stand-in: no kernel is launched on the error path
    EINVAL, EUNSUPPORTED = -1, -2

    def gemm(x=P, ldx=64, wq=P, ldw=64, scale=P, fmt=1, c=P, ldc=8, M=17, N=8, K=64, res=0, ldr=0, flags=0, ws=P, nws=1 << 20):
        return L.mm355_gemm_w8(x, ldx, wq, ldw, scale, fmt, c, ldc, M, N, K, res, ldr, flags, ws, nws, 0)
    assert gemm(fmt=2) == EINVAL                                 # the MXFP4 format: not this kernel's
    assert gemm(fmt=7) == EINVAL                                 # a format that does not exist
    assert gemm(K=48, ldx=48, ldw=48) == EINVAL                  # K % 64
    assert gemm(K=32, ldx=32, ldw=32) == EINVAL
    assert gemm(ldw=72) == EINVAL                                # ldw_bytes % 16
    assert gemm(ldw=48) == EINVAL                                # ldw_bytes < K
    assert gemm(ldx=68) == EINVAL                                # ldx % 8
    assert gemm(scale=0) == EINVAL                               # no scales
    assert gemm(scale=P + 2) == EINVAL                           # ... or misaligned ones
    assert gemm(wq=P + 8) == EINVAL                              # misaligned weight bytes
    assert gemm(x=P + 2) == EINVAL
    assert gemm(c=P + 4) == EINVAL
    assert gemm(flags=8, res=0) == EINVAL                        # RESIDUAL without a residual
    assert gemm(flags=8, res=P + 2) == EINVAL                    # ... with a misaligned one
    assert gemm(flags=1) == EINVAL                               # a flag the w8 GEMM does not take (BIAS)
    assert gemm(M=4097) == EUNSUPPORTED                          # larger passes stay on the scratch route
    # a problem that IS split, with a workspace that is too small / missing
    M, N, K = 20, 1024, 4096
    need = L.mm355_gemm_w8_ws_floats(M, N, K)
    assert need > 0
    assert gemm(M=M, N=N, K=K, ldx=K, ldw=K, ldc=N, nws=need - 1) == EINVAL
    assert gemm(M=M, N=N, K=K, ldx=K, ldw=K, ldc=N, ws=0) == EINVAL
    assert gemm(M=M, N=N, K=K, ldx=K, ldw=K, ldc=N, ws=P + 4) == EINVAL

    #                                                    C  M   N     K    res ldr norm eps Y  ws nws stream
    assert L.mm355_gemm_w8_norm(P, K, P, K, P, 2, P, M, N, K, 0, 0, P, 1e-5, P, P, need, 0) == EINVAL
    assert L.mm355_gemm_w8_norm(P, K, P, K, 0, 1, P, M, N, K, 0, 0, P, 1e-5, P, P, need, 0) == EINVAL
    assert L.mm355_gemm_w8_norm(P, K, P, K, P, 1, P, M, N, K, 0, 0, P, 1e-5, P, P, need - 1, 0) == EINVAL
    assert L.mm355_gemm_w8_norm(P, K, P, K, P, 1, P, 5000, N, K, 0, 0, P, 1e-5, P, P, 1 << 40, 0) == EUNSUPPORTED
    #                                                      act ld  M  I    K    ws nws stream
    need_s = L.mm355_gemm_w8_swiglu_ws_floats(M, 512, K)
    assert L.mm355_gemm_w8_swiglu(P, K, P, K, P, 3, P, 512, M, 512, K, P, need_s, 0) == EINVAL
    assert L.mm355_gemm_w8_swiglu(P, K, P, K + 8, P, 1, P, 512, M, 512, K, P, need_s, 0) == EINVAL     # ldw_bytes % 16
    assert L.mm355_gemm_w8_swiglu(P, K, P, K, P, 1, P, 512, M, 512, K, P, need_s - 1, 0) == EINVAL
    assert L.mm355_gemm_w8_swiglu(P, K, P, K, P, 1, P, 510, M, 510, K, P, 1 << 30, 0) == EINVAL           # I % 4 (2 I must be splittable)
    assert L.mm355_gemm_w8_swiglu(P, K, P, K, P, 1, P, 500, M, 512, K, P, need_s, 0) == EINVAL            # ld_act < I
    assert L.mm355_gemm_w8_swiglu(P, K, P, K, P, 1, P, 512, 4097, 512, K, P, 1 << 40, 0) == EUNSUPPORTED
    #                                                           qkv ld   M  Hq Hkv d   K  cos sin pos kc vc ldkv bs  ws nws stream
    assert L.mm355_gemm_w8_rope_append(P, K, P, K, P, 0, P, 1024, M, 4, 2, 128, K, P, P, P, P, P, 256, 4096, P, need, 0) == EINVAL
    assert L.mm355_gemm_w8_rope_append(P, K, P, K, P, 1, P, 1024, M, 4, 2, 128, K + 32, P, P, P, P, P, 256, 4096, P, need, 0) == EINVAL
    assert L.mm355_gemm_w8_rope_append(P, K + 4, P, K, P, 1, P, 1024, M, 4, 2, 128, K, P, P, P, P, P, 256, 4096, P, need, 0) == EINVAL   # ldx % 8
    assert L.mm355_gemm_w8_rope_append(P, K, P, K, P, 1, P, 1024, M, 4, 2, 128, K, P, P, P, P, P, 256, 4096, P, need - 1, 0) == EINVAL
    assert L.mm355_gemm_w8_rope_append(P, K, P, K, P, 1, P, 1024, 4097, 4, 2, 128, K, P, P, P, P, P, 256, 4096, P, 1 << 40, 0) == EUNSUPPORTED
    # the 16-row GEMV keeps its own limit
    assert L.mm355_gemv_w8(P, 64, P, 64, P, 1, P, 64, 17, 8, 64, 0, 0, 0, 0, 0) == EUNSUPPORTED


def test_gemm_w8_workspaces_equal_the_bf16_split_k_forms():
    _, L = _load()
    split = 0
    for M in (1, 17, 20, 32, 33, 64, 100, 512, 1024, 2048, 4096):
        for (N, K) in ((6144, 4096), (4096, 4096), (4096, 14336), (28672, 4096), (136, 512), (128256, 4096), (1536, 1024), (1024, 2048)):
            ref = L.mm355_gemm_splitk_ws_floats(M, N, K)
            if ref > 0:
                split += 1
                assert L.mm355_gemm_w8_ws_floats(M, N, K) == ref, (M, N, K)
            if N % 2 == 0:
                assert L.mm355_gemm_w8_swiglu_ws_floats(M, N // 2, K) == L.mm355_gemm_splitk_swiglu_ws_floats(M, N // 2, K), (M, N, K)
    assert split > 20


def test_b_tile_layout_is_conflict_free_and_complete():
    """The byte B tile of gemm_wq_kernel<W8, BM> (W8::Lane, csrc/gemm_w8.hip) in LDS: 128 weight rows x 64 bytes, written by LDS-DMA in 1-KiB pieces (lane L ->
    piece byte 16 L, row L >> 2, slot L & 3, source chunk (L & 3) ^ ((row >> 2) & 3)), read by one ds_read_b64 per lane and fragment.
    ds_read_b64 is served per 32-lane half with bank = (byte / 4) % 64: every half of every fragment read must touch each of the 64 banks
    exactly once, and a lane must find bytes k = kk*32 + fq*8 .. +7 of weight row wn*32 + j*16 + fr at the address it reads.

    This is the enumeration the kernel's comment refers to, kept as a record of how the layout was checked: a Python MODEL of the address
    formulae, not a run of the kernel.  It needs no GPU and passes without gemm_w8.hip being compiled.  What ties it to the kernel is the
    source check below -- the swizzle expressions the model restates must still be the ones in the file, so a changed swizzle fails here
    until the model is brought along -- and tests/test_w8_gemm_gpu.py, where a (row, k) byte that lands anywhere else breaks the
    bit-for-bit and every-byte tests."""
    src = open(os.path.join(REPO, "metamorph_amd", "csrc", "gemm_w8.hip")).read()
    for expr in ("const int rb = lane >> 2;", "const int cb = (lane & 3) ^ ((rb >> 2) & 3);", "const int bx = (fr >> 2) & 3;",
                 "A_BYTES + (wn * TN + fr) * 64 + (fq & 1) * 8", "int b_off1 = b_off + 1024;", "const int bsw0 = (((fq >> 1)) ^ bx) << 4;",
                 "const int bsw1 = ((2 + (fq >> 1)) ^ bx) << 4;", "B_BYTES = BN * 64"):
        assert expr in src, expr
    image = {}                                                   # LDS byte (relative to the B tile) -> (row, k)
    for piece in range(8):
        for lane in range(64):
            row = lane >> 2
            chunk = (lane & 3) ^ ((row >> 2) & 3)
            for b in range(16):
                image[piece * 1024 + lane * 16 + b] = (piece * 16 + row, chunk * 16 + b)
    assert len(image) == 128 * 64 and len(set(image.values())) == 128 * 64
    for wn in range(4):
        for j in range(2):
            for kk in range(2):
                for half in range(2):
                    banks = []
                    for lane in range(half * 32, half * 32 + 32):
                        fr, fq = lane & 15, lane >> 4
                        addr = (wn * 32 + fr) * 64 + (fq & 1) * 8 + j * 1024 + (((kk * 2 + (fq >> 1)) ^ ((fr >> 2) & 3)) << 4)
                        assert addr % 8 == 0
                        for b in range(8):
                            assert image[addr + b] == (wn * 32 + j * 16 + fr, kk * 32 + fq * 8 + b), (wn, j, kk, lane, b)
                        banks += [(addr // 4) % 64, (addr // 4 + 1) % 64]
                    assert sorted(banks) == list(range(64)), (wn, j, kk, half)
