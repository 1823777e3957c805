// Weight-only MXFP4 GEMM for gfx950: C[M,N] = epilogue(x[M,K] . Wd[N,K]^T), Wd[n][k] = e2m1(nibble) * 2^(S[n][k/32] - 127): OCP e2m1 nibbles
// Wq[N][K/2] plus one e8m0 scale byte per 32 consecutive k, S[N][K/32] (the format of decode_w4.hip).  The prompt pass and decode steps of
// more than 16 sequences on a 4-bit model: the weight is streamed as NIBBLES, 0.27 x the traffic of the bf16 GEMM, instead of being
// dequantised into a scratch buffer first.
//
// The kernel is the twin of gemm_w8_kernel<32|64> (gemm_w8.hip) and through it of gemm_nt_kernel<32|64, 128, 1, 4, true, 0> as splitk_partials
// (gemm_bf16.hip) launches it, and keeps its summation order exactly: the same slices (mm_splitk_slices), the same kslice, 64-wide K tiles,
// per tile and fragment the two v_mfma_f32_16x16x32_bf16 in the same order with the same k in every operand slot (lane group fq holds
// k = kk*32 + fq*8 .. +7).  Every Wd is exactly a bf16 value and the group scale sits INSIDE the widening conversion, so the B fragments are
// bit for bit those the bf16 kernel reads from the dequantised weight and so are all results, for any scales: nothing is multiplied in the
// epilogue and the partials of a split problem are plain P_s (tests/test_w4_gemm_gpu.py rests on this).
//   * A (x) tiles: LDS-DMA into [rows][64 bf16] with the 16-B chunk index XOR-ed with (row & 7), as in gemm_bf16.hip / gemm_w8.hip.
//   * B (weight) tiles: LDS-DMA of nibbles.  A B row of a K tile is 32 bytes = two 16-B chunks (chunk kk = the k-step kk = ONE scale group),
//     a DMA piece (64 lanes x 16 B, lane-linear in LDS) is 32 rows x 2 chunks, the 128 rows of a tile are one piece per wave.  Lane L lands
//     in (row L >> 1, slot L & 1) and fetches source chunk (L & 1) ^ ((row >> 3) & 1).  A lane's fragment (8 consecutive k) is the dword fq
//     of chunk kk of row fr.  It is read with ONE ds_read_b64 per lane of the 8-byte half (fq >> 1) of that chunk, at byte
//     row*32 + ((kk ^ ((fr >> 3) & 1)) << 4) + (fq >> 1)*8, and the lane keeps dword fq & 1 of it (one v_cndmask).  Why not ds_read_b32:
//     its banks are (byte / 4) % 32, and the 16 rows x 2 dwords of a 32-lane half then need 16 distinct 8-byte slots in a 128-byte bank
//     period out of 16-byte DMA units that offer one such slot each (the half (fq >> 1) is one value per 32-lane half): 2-way at best.
//     ds_read_b64 is served per 32-lane half with bank = (byte / 4) % 64: a half (fq in {0,1} or {2,3}, all fr) reads 16 distinct 8-byte
//     addresses (lanes fq and fq ^ 1 of a row share one: a broadcast), row fr sits 32 bytes after row fr - 1, so rows fr and fr + 8 share a
//     256-byte bank period position and the XOR with (fr >> 3) puts them on its two chunks: 16 addresses on 16 distinct bank pairs.
//     Checked by enumeration in tests/test_w4_gemm_host.py::test_b_tile_layout_is_conflict_free_and_complete, which also checks that the DMA
//     image and the fragment reads agree on where every (row, k) nibble lives.
//   * scale bytes: per K tile a lane needs S[n][k0/32 + kk] of its two fragment rows n, kk = 0, 1: two adjacent bytes per row.  They travel
//     as per-lane global loads, one tile AHEAD of their use, issued in FRONT of the LDS-DMA of the same tile: the vector-memory counter
//     retires in order, so a load behind a DMA would hold its consumer until the DMA has landed, and a load whose first use sits in the span
//     where a DMA is in flight makes hipcc drain the DMA there (vmcnt(0)).  Here the first use is one iteration later, behind the barrier
//     that has drained the counter anyway, and the loaded word is handed to its consumers behind that barrier: no wait is added (checked
//     in the ISA: no s_waitcnt vmcnt between the DMA issue and the one in front of the barrier).
//     Not a DMA piece: 2 bytes per row is below every DMA width that keeps rows apart, and S rows need no alignment (lds_bytes is free).
//     One 16-bit load per fragment row and K tile; the four lanes fq of a row read the same two bytes (one request per 16 lanes).
//   * widening: e2m1x8_to_bf16 (four v_cvt_scalef32_pk_bf16_fp4 per fragment, exact), k order kept.  64 x 128 tile: 16 conversions per
//     thread and K tile and no permutes, beside 16 MFMAs per wave.
#include "gemm_common.h"
#include "splitk.h"

namespace {

struct GemmW4Args {
    GemmArgs g;                                              // A = x, C / res / flags / kslice as the bf16 kernel; B and ldb unused
    const uint8_t* Wq; int64_t ldw;                          // bytes
    const uint8_t* S; int64_t lds;                           // bytes
};

template <int BM>
__global__ __launch_bounds__(256) void gemm_w4_kernel(GemmW4Args w) {
    constexpr int BN = 128, NW = 4;
    constexpr int TM = BM, TN = BN / NW, FM = TM / 16, FN = TN / 16;
    constexpr int A_BYTES = BM * 128, B_BYTES = BN * 32, STAGE = A_BYTES + B_BYTES;
    constexpr int AI = BM / 8 / NW;                          // 1-KiB DMA pieces per wave: 8 x rows of 128 B; ONE piece of 32 weight rows of 32 B
    constexpr int GM = 8;
    static_assert(AI >= 1 && FN == 2 && B_BYTES == NW * 1024, "tile shape");
    const GemmArgs& a = w.g;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    // ---- workgroup -> tile: gemm_nt_kernel's map
    const int total = a.ntm * a.ntn;
    const int bid = blockIdx.x;
    const int q8 = total >> 3, r8 = total & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
    const int gsize = GM * a.ntn;
    const int grp = logical / gsize;
    const int first_m = grp * GM;
    const int gm = min(a.ntm - first_m, GM);
    const int in_g = logical - grp * gsize;
    const int tm = first_m + in_g % gm;
    const int tn = in_g / gm;
    const int m0 = tm * BM, n0 = tn * BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave;
    const int fr = lane & 15, fq = lane >> 4;
    const int sl = a.kslice ? (int)blockIdx.y : 0;
    const uint16_t* Ab = a.A + (int64_t)sl * a.kslice;
    const uint8_t* Wb = w.Wq + (((int64_t)sl * a.kslice) >> 1);
    const uint8_t* Sb = w.S + (((int64_t)sl * a.kslice) >> 5);
    const int M = a.M, N = a.N, K = a.kslice ? min(a.kslice, a.K - sl * a.kslice) : a.K;
    const int nk = K >> 6;                                   // (host: K % 64 == 0, kslice % 64 == 0)

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int sw0 = ((fq) ^ (fr & 7)) << 4;
    const int sw1 = ((4 + fq) ^ (fr & 7)) << 4;
    const int a_off = fr * 128;
    const int bx = (fr >> 3) & 1;
    const int b_off = A_BYTES + (wn * TN + fr) * 32 + (fq >> 1) * 8;
    // the second fragment's rows sit 512 B further on; the offset is kept opaque so that the two reads stay two ds_read_b64 (gemm_w8.hip:
    // the ds_read2 forms are banked (byte / 4) % 32, the layout above is conflict-free for the 64-bank form only)
    int b_off1 = b_off + 512;
    asm volatile("" : "+v"(b_off1));
    const int bsw0 = bx << 4;
    const int bsw1 = (1 ^ bx) << 4;
    const bool odd = (fq & 1) != 0;                          // which dword of the 8 bytes read is this lane's fragment

    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const uint16_t* srcA[AI];
    const uint8_t* srcB;
    const uint8_t* srcS[FN];
    {
        const int rin = lane >> 3;                           // row inside the 8-row x piece
        const int c = (lane & 7) ^ rin;                      // source chunk that belongs in LDS slot (lane & 7)
#pragma unroll
        for (int i = 0; i < AI; ++i)
            srcA[i] = Ab + (int64_t)min(m0 + (i * NW + wave_s) * 8 + rin, M - 1) * a.lda + c * 8;
        const int rb = lane >> 1;                            // row inside the 32-row weight piece
        const int cb = (lane & 1) ^ ((rb >> 3) & 1);         // source chunk that belongs in LDS slot (lane & 1)
        srcB = Wb + (int64_t)min(n0 + wave_s * 32 + rb, N - 1) * w.ldw + cb * 16;
#pragma unroll
        for (int j = 0; j < FN; ++j) srcS[j] = Sb + (int64_t)min(n0 + wn * TN + j * 16 + fr, N - 1) * w.lds;
    }
    auto gdma = [&](int kt, int buf) {
        const int64_t k0 = kt << 6;
        unsigned char* sb = smem + buf * STAGE + wave_s * 1024;
#pragma unroll
        for (int i = 0; i < AI; ++i)
            __builtin_amdgcn_global_load_lds((gptr_t)(srcA[i] + k0), (lptr_t)(sb + i * NW * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gptr_t)(srcB + (k0 >> 1)), (lptr_t)(sb + A_BYTES), 16, 0, 0);
    };
    // the scale bytes of K tile kt, two per fragment row as ONE 16-bit word: byte kk = S[n_j][k0/32 + kk] (S rows need no alignment: the
    // copy leaves the form of the load to hipcc, which takes a single global_load_ushort)
    auto gscale = [&](int kt, uint32_t (&s)[FN]) {
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            uint16_t v;
            __builtin_memcpy(&v, srcS[j] + 2 * kt, 2);
            s[j] = v;
        }
    };

    // ---- main loop: gemm_nt_kernel's two-stage schedule (next tile in flight during the MFMAs); the scale bytes one tile ahead, in front
    //      of the DMA.  The loaded words are handed over BEHIND the barrier through an opaque move: without it hipcc unpacks them right
    //      behind the load, i.e. waits vmcnt(0) between the DMA pieces.
    uint32_t sc[FN], scn[FN];
    gscale(0, scn);
    gdma(0, 0);
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            sc[j] = scn[j];
            asm volatile("" : "+v"(sc[j]));
        }
        if (kt + 1 < nk) {
            gscale(kt + 1, scn);
            gdma(kt + 1, cur ^ 1);
        }
        const unsigned char* sb = smem + cur * STAGE;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 af[FM], bf[FN];
#pragma unroll
            for (int i = 0; i < FM; ++i) af[i] = *(const bf16x8*)(sb + a_off + i * 2048 + (kk ? sw1 : sw0));
#pragma unroll
            for (int j = 0; j < FN; ++j) {
                const u32x2 q = *(const u32x2*)(sb + (j ? b_off1 : b_off) + (kk ? bsw1 : bsw0));
                uint32_t p[4];
                e2m1x8_to_bf16(odd ? q.y : q.x, e8m0_to_f32(kk ? sc[j] >> 8 : sc[j] & 0xffu), p);
                bf[j] = __builtin_bit_cast(bf16x8, u32x4{p[0], p[1], p[2], p[3]});
            }
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        cur ^= 1;
    }

    // ---- epilogue: gemm_nt_kernel's store (accumulator element r of fragment j is column j*16 + fr of the wave's 32); no scale here
    GemmArgs e = a;
    if (a.kslice) e.C = (float*)a.C + (int64_t)sl * a.M * a.ldc;     // this slice's partial tile, plain fp32
    gemm_epilogue<TM, TN, FM, FN>(acc, e, smem, m0, n0, 0, wn, wave, lane);
}

// x rows, weight nibbles and scale bytes in the form the kernel addresses them (64-bit addresses: no limit on N * ldw_bytes); everything a
// launch depends on, before any launch
int w4_gemm_check(const void* x, int64_t ldx, const void* Wq, int64_t ldw, const void* S, int64_t lds, int fmt, int64_t M, int64_t N, int64_t K) {
    if (!x || !Wq || !S || M <= 0 || N <= 0 || K <= 0) return MM355_EINVAL;
    if (fmt != MM355_W4_MXFP4) return MM355_EINVAL;
    if ((K & 63) || (ldx & 7) || ldx < K || (ldw & 15) || ldw < K / 2 || lds < K / 32 || !mm_aligned16(x) || !mm_aligned16(Wq)) return MM355_EINVAL;
    if (N > 0x7fffffff || K > 0x7fffffff) return MM355_EINVAL;
    if (M > 4096) return MM355_EUNSUPPORTED;                 // larger passes: mm355_dequant_w4_bf16 + the bf16 GEMMs
    return MM355_OK;
}

// x . Wd^T: S > 1 -> fp32 partials workspace[slice][M][N] (`slices` written; the caller reduces them), S == 1 -> one slice with
// gemm_nt_kernel's epilogue straight into C (flags: RESIDUAL | OUT_F32)
int w4_gemm_launch(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw, const uint8_t* Sc, int64_t lds, int64_t M, int64_t N, int64_t K,
                   int S, float* workspace, void* C, int64_t ldc, const mm355_bf16* residual, int64_t ldr, uint32_t flags, hipStream_t stream,
                   int& slices) {
    GemmW4Args w = {};
    GemmArgs& a = w.g;
    a.A = x; a.lda = ldx; a.M = (int)M; a.N = (int)N; a.K = (int)K;
    w.Wq = Wq; w.ldw = ldw; w.S = Sc; w.lds = lds;
    if (S > 1) {
        a.C = workspace; a.ldc = N; a.flags = MM355_GEMM_OUT_F32;
        const int64_t nk = K / 64;
        a.kslice = (int)((nk + S - 1) / S) * 64;
        slices = (int)((K + a.kslice - 1) / a.kslice);
    } else {
        a.C = C; a.ldc = ldc; a.res = residual; a.ldr = ldr; a.flags = flags; a.kslice = 0;
        slices = 1;
    }
    a.ntn = (int)((N + 127) / 128);
    // tiles as splitk_partials: 64 x 128 (four waves side by side), up to 32 rows 32 x 128; the same bits under either
    if (M <= 32) {
        a.ntm = 1;
        hipLaunchKernelGGL(gemm_w4_kernel<32>, dim3((unsigned)a.ntn, (unsigned)slices), dim3(256), 2 * (32 * 128 + 128 * 32), stream, w);
    } else {
        a.ntm = (int)((M + 63) / 64);
        const int64_t total = (int64_t)a.ntm * a.ntn;
        if (total > 0x7fffffff) return MM355_EINVAL;
        hipLaunchKernelGGL(gemm_w4_kernel<64>, dim3((unsigned)total, (unsigned)slices), dim3(256), 2 * (64 * 128 + 128 * 32), stream, w);
    }
    return mm_launch_status();
}

}  // namespace

extern "C" int64_t mm355_gemm_w4_ws_floats(int64_t M, int64_t N, int64_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const int S = mm_splitk_slices(M, N, K);
    return S > 1 ? (int64_t)S * M * N : 0;
}

extern "C" int mm355_gemm_w4(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes, int fmt,
                             void* C, int64_t ldc, int64_t M, int64_t N, int64_t K, const mm355_bf16* residual, int64_t ldr, uint32_t flags,
                             float* workspace, int64_t workspace_floats, void* stream) {
    (void)hipGetLastError();
    if (!C) return MM355_EINVAL;
    if (flags & ~(MM355_GEMM_RESIDUAL | MM355_GEMM_OUT_F32)) return MM355_EINVAL;
    if ((flags & MM355_GEMM_RESIDUAL) && (!residual || !mm_aligned16(residual))) return MM355_EINVAL;
    if (!(flags & MM355_GEMM_RESIDUAL)) residual = nullptr;
    const int rc = w4_gemm_check(x, ldx, Wq, ldw_bytes, S, lds_bytes, fmt, M, N, K);
    if (rc != MM355_OK) return rc;
    if (!mm_aligned16(C) || ldc < N) return MM355_EINVAL;
    const int Sk = mm_splitk_slices(M, N, K);
    const bool f32 = (flags & MM355_GEMM_OUT_F32) != 0;
    int slices = 0;
    if (Sk <= 1 || f32) {                                    // one slice, stored straight into C (fp32 output is never split: the reduce launches write bf16)
        return w4_gemm_launch(x, ldx, Wq, ldw_bytes, S, lds_bytes, M, N, K, 1, nullptr, C, ldc, residual, ldr, flags, (hipStream_t)stream, slices);
    }
    if ((ldc & 7) || (residual && (ldr & 7)) || !workspace || !mm_aligned16(workspace) || workspace_floats < (int64_t)Sk * M * N) return MM355_EINVAL;
    const int rl = w4_gemm_launch(x, ldx, Wq, ldw_bytes, S, lds_bytes, M, N, K, Sk, workspace, nullptr, 0, nullptr, 0, 0u, (hipStream_t)stream, slices);
    if (rl != MM355_OK) return rl;
    return mm_splitk_reduce(workspace, slices, M, N, residual, ldr, (mm355_bf16*)C, ldc, (hipStream_t)stream);
}

extern "C" int mm355_gemm_w4_norm(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes,
                                  int fmt, mm355_bf16* C, int64_t M, int64_t N, int64_t K, const mm355_bf16* residual, int64_t ldr,
                                  const mm355_bf16* norm_w, float eps, mm355_bf16* Y, float* workspace, int64_t workspace_floats, void* stream) {
    (void)hipGetLastError();
    if (!C || !Y || !norm_w || N <= 0 || (N & 7)) return MM355_EINVAL;
    if (!mm_aligned16(C) || !mm_aligned16(Y) || !mm_aligned16(norm_w) || (residual && ((ldr & 7) || !mm_aligned16(residual)))) return MM355_EINVAL;
    const int rc = w4_gemm_check(x, ldx, Wq, ldw_bytes, S, lds_bytes, fmt, M, N, K);
    if (rc != MM355_OK) return rc;
    const int Sk = mm_splitk_slices(M, N, K);
    int slices = 0;
    if (Sk <= 1) {                                           // not split: the launch sequence, as the bf16 twin
        const int rl = w4_gemm_launch(x, ldx, Wq, ldw_bytes, S, lds_bytes, M, N, K, 1, nullptr, C, N, residual, ldr,
                                      residual ? MM355_GEMM_RESIDUAL : 0u, (hipStream_t)stream, slices);
        return rl != MM355_OK ? rl : mm355_rmsnorm_fwd(C, norm_w, Y, M, N, eps, stream);
    }
    if ((N >> 3) > 8 * 256) return MM355_EUNSUPPORTED;      // (the row lives in registers: mm355_rmsnorm_fwd's own limit)
    if (!workspace || !mm_aligned16(workspace) || workspace_floats < (int64_t)Sk * M * N) return MM355_EINVAL;
    const int rl = w4_gemm_launch(x, ldx, Wq, ldw_bytes, S, lds_bytes, M, N, K, Sk, workspace, nullptr, 0, nullptr, 0, 0u, (hipStream_t)stream, slices);
    if (rl != MM355_OK) return rl;
    return mm_splitk_reduce_norm(workspace, slices, M, N, residual, ldr, C, norm_w, eps, Y, (hipStream_t)stream);
}

extern "C" int64_t mm355_gemm_w4_swiglu_ws_floats(int64_t M, int64_t I, int64_t K) {
    if (M <= 0 || I <= 0 || K <= 0) return 0;
    const int S = mm_splitk_slices(M, 2 * I, K);
    return S > 1 ? (int64_t)S * M * 2 * I : M * I;          // not split: the bf16 [M][2 I] gate | up rows of the plain sequence
}

extern "C" int mm355_gemm_w4_swiglu(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes,
                                    int fmt, mm355_bf16* act, int64_t ld_act, int64_t M, int64_t I, int64_t K, float* workspace,
                                    int64_t workspace_floats, void* stream) {
    (void)hipGetLastError();
    if (!act || !workspace || I <= 0 || (I & 3) || I > 0x3fffffff || ld_act < I || !mm_aligned16(workspace)) return MM355_EINVAL;
    const int64_t N = 2 * I;
    const int rc = w4_gemm_check(x, ldx, Wq, ldw_bytes, S, lds_bytes, fmt, M, N, K);
    if (rc != MM355_OK) return rc;
    if (workspace_floats < mm355_gemm_w4_swiglu_ws_floats(M, I, K)) return MM355_EINVAL;
    const int Sk = mm_splitk_slices(M, N, K);
    int slices = 0;
    if (Sk <= 1) {
        if ((I & 7) || !mm_aligned16(act)) return MM355_EINVAL;  // (mm355_swiglu_fwd's own limits)
        if (ld_act != I) return MM355_EUNSUPPORTED;
        mm355_bf16* gu = (mm355_bf16*)workspace;
        const int rl = w4_gemm_launch(x, ldx, Wq, ldw_bytes, S, lds_bytes, M, N, K, 1, nullptr, gu, N, nullptr, 0, 0u, (hipStream_t)stream, slices);
        return rl != MM355_OK ? rl : mm355_swiglu_fwd(gu, act, M, I, stream);
    }
    const int rl = w4_gemm_launch(x, ldx, Wq, ldw_bytes, S, lds_bytes, M, N, K, Sk, workspace, nullptr, 0, nullptr, 0, 0u, (hipStream_t)stream, slices);
    if (rl != MM355_OK) return rl;
    return mm_splitk_reduce_swiglu(workspace, slices, M, I, act, ld_act, (hipStream_t)stream);
}

extern "C" int mm355_gemm_w4_rope_append(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S,
                                         int64_t lds_bytes, int fmt, mm355_bf16* qkv, int64_t ld_qkv, int64_t M, int64_t Hq, int64_t Hkv,
                                         int64_t d, int64_t K, const mm355_bf16* cos_t, const mm355_bf16* sin_t, const int32_t* positions,
                                         mm355_bf16* k_cache, mm355_bf16* v_cache, int64_t ld_kv, int64_t batch_stride_kv, float* workspace,
                                         int64_t workspace_floats, void* stream) {
    (void)hipGetLastError();
    if (!qkv || !cos_t || !sin_t || !positions || !k_cache || !v_cache || Hq <= 0 || Hkv <= 0 || d <= 0 || (d & 15) || (ld_qkv & 7) || (ld_kv & 7) ||
        (batch_stride_kv & 7) || !mm_aligned16(qkv) || !mm_aligned16(k_cache) || !mm_aligned16(v_cache) || !mm_aligned16(cos_t) ||
        !mm_aligned16(sin_t))
        return MM355_EINVAL;
    const int64_t N = (Hq + 2 * Hkv) * d;
    if (ld_qkv < N) return MM355_EINVAL;
    const int rc = w4_gemm_check(x, ldx, Wq, ldw_bytes, S, lds_bytes, fmt, M, N, K);
    if (rc != MM355_OK) return rc;
    const int Sk = mm_splitk_slices(M, N, K);
    int slices = 0;
    if (Sk <= 1) {
        const int rl = w4_gemm_launch(x, ldx, Wq, ldw_bytes, S, lds_bytes, M, N, K, 1, nullptr, qkv, ld_qkv, nullptr, 0, 0u, (hipStream_t)stream, slices);
        return rl != MM355_OK ? rl
                              : mm355_rope_kv_append(qkv, ld_qkv, M, Hq, Hkv, d, cos_t, sin_t, positions, k_cache, v_cache, ld_kv, batch_stride_kv, stream);
    }
    if (!workspace || !mm_aligned16(workspace) || workspace_floats < (int64_t)Sk * M * N) return MM355_EINVAL;
    const int rl = w4_gemm_launch(x, ldx, Wq, ldw_bytes, S, lds_bytes, M, N, K, Sk, workspace, nullptr, 0, nullptr, 0, 0u, (hipStream_t)stream, slices);
    if (rl != MM355_OK) return rl;
    return mm_splitk_reduce_rope_append(workspace, slices, M, Hq, Hkv, d, qkv, ld_qkv, cos_t, sin_t, positions, k_cache, v_cache, ld_kv,
                                        batch_stride_kv, (hipStream_t)stream);
}
