// What the split-K GEMMs over quantised weights share (gemm_w8.hip: e4m3 bytes + a scale per row; gemm_w4.hip: MXFP4 nibbles + a scale
// byte per 32 columns): the kernel skeleton and the host driver behind the extern "C" entry points.  The skeleton is
// gemm_nt_kernel<32|64, 128, 1, 4, true, 0> as splitk_partials (gemm_bf16.hip) launches it -- the same tile map, slices, kslice, 64-wide K
// tiles, per tile and fragment the two v_mfma_f32_16x16x32_bf16 in the same order with the same k in every operand slot (lane group fq
// holds k = kk*32 + fq*8 .. +7), the same epilogue -- with the B side handed to a format policy W.  A format supplies:
//   * Args (GemmArgs g in front: A = x, C / res / flags / kslice as the bf16 kernel, B and ldb unused; then its weight operands), FMT
//     and operands_ok() for the host;
//   * Lane<BM>, one lane's B side of a BM x 128 tile, with the sizes of a stage (A_BYTES, B_BYTES, STAGE: the x tile, then the format's B
//     image) and these members:
//   * init(): its per-lane B fragment offsets and B (and scale) source pointers;
//   * ahead() + dma(): the B part of one tile's LDS-DMA and what travels beside the tile, issued in FRONT of the tile's DMA; take(): the
//     hand-over of what ahead() loaded, behind the barrier;
//   * frag(): one B fragment as bf16x8 from LDS for (fragment j, k-step kk);
//   * finish(): what happens to the accumulators in front of the epilogue.
// The skeleton never asks which format it runs; the LDS image of the B tile and the reasons for it are described in the format's file.
#pragma once
#include "gemm_common.h"
#include "splitk.h"

namespace {

template <class W, int BM>
__global__ __launch_bounds__(256) void gemm_wq_kernel(typename W::Args w) {
    constexpr int BN = 128, NW = 4;
    constexpr int TM = BM, TN = BN / NW, FM = TM / 16, FN = TN / 16;
    using Lane = typename W::template Lane<BM>;
    constexpr int STAGE = Lane::STAGE;
    constexpr int AI = BM / 8 / NW;                          // 1-KiB DMA pieces of x per wave: 8 rows of 128 B
    static_assert(AI >= 1 && FN == 2 && Lane::A_BYTES == BM * 128 && Lane::B_BYTES % (NW * 1024) == 0 && Lane::TN == TN, "tile shape");
    const GemmArgs& a = w.g;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    int tm, tn;
    gemm_tile_map(a.ntm, a.ntn, 8, blockIdx.x, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave;
    const int fr = lane & 15, fq = lane >> 4;
    const int sl = a.kslice ? (int)blockIdx.y : 0;
    const uint16_t* Ab = a.A + (int64_t)sl * a.kslice;
    const int M = a.M, K = a.kslice ? min(a.kslice, a.K - sl * a.kslice) : a.K;
    const int nk = K >> 6;                                   // (host: K % 64 == 0, kslice % 64 == 0)

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // A (x) tiles: LDS-DMA into [rows][64 bf16] with the 16-B chunk index XOR-ed with (row & 7), as in gemm_bf16.hip
    const int sw0 = ((fq) ^ (fr & 7)) << 4;
    const int sw1 = ((4 + fq) ^ (fr & 7)) << 4;
    const int a_off = fr * 128;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    Lane b;
    b.init(w, (int64_t)sl * a.kslice, n0, wn, wave_s, lane);
    const uint16_t* srcA[AI];
    {
        const int rin = lane >> 3;                           // row inside the 8-row x piece
        const int c = (lane & 7) ^ rin;                      // source chunk that belongs in LDS slot (lane & 7)
#pragma unroll
        for (int i = 0; i < AI; ++i)
            srcA[i] = Ab + (int64_t)min(m0 + (i * NW + wave_s) * 8 + rin, M - 1) * a.lda + c * 8;
    }
    auto gdma = [&](int kt, int buf) {
        const int64_t k0 = kt << 6;
        unsigned char* sb = smem + buf * STAGE + wave_s * 1024;
#pragma unroll
        for (int i = 0; i < AI; ++i)
            __builtin_amdgcn_global_load_lds((gptr_t)(srcA[i] + k0), (lptr_t)(sb + i * NW * 1024), 16, 0, 0);
        b.dma(kt, smem, buf);
    };

    // ---- main loop: gemm_nt_kernel's two-stage schedule (next tile in flight during the MFMAs); what a format loads beside the tile goes
    //      out in front of the tile's DMA and is taken over behind the barrier (gemm_w4.hip says why)
    b.ahead(0);
    gdma(0, 0);
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        b.take();
        if (kt + 1 < nk) {
            b.ahead(kt + 1);
            gdma(kt + 1, cur ^ 1);
        }
        const unsigned char* sb = smem + cur * STAGE;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 af[FM], bf[FN];
#pragma unroll
            for (int i = 0; i < FM; ++i) af[i] = *(const bf16x8*)(sb + a_off + i * 2048 + (kk ? sw1 : sw0));
#pragma unroll
            for (int j = 0; j < FN; ++j) bf[j] = b.frag(sb, j, kk);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        cur ^= 1;
    }

    // ---- epilogue: the format's step, then gemm_nt_kernel's store (accumulator element r of fragment j is column j*16 + fr of the wave's 32)
    b.finish(acc, w, n0 + wn * TN + fr);
    GemmArgs e = a;
    if (a.kslice) e.C = (float*)a.C + (int64_t)sl * a.M * a.ldc;     // this slice's partial tile, plain fp32
    gemm_epilogue<TM, TN, FM, FN>(acc, e, smem, m0, n0, 0, wn, wave, lane);
}

// ---- host driver.  `w` carries the format's weight operands (w.g is filled here); every form checks everything a launch depends on
// before any launch.

// x rows and the weight operands in the form the kernel addresses them (64-bit addresses: no limit on N * ldw)
template <class W>
int wq_check(const typename W::Args& w, int fmt, const void* x, int64_t ldx, int64_t M, int64_t N, int64_t K) {
    if (!x || M <= 0 || N <= 0 || K <= 0 || fmt != W::FMT || !W::operands_ok(w, K)) return MM355_EINVAL;
    if ((K & 63) || (ldx & 7) || ldx < K || !mm_aligned16(x)) return MM355_EINVAL;
    if (N > 0x7fffffff || K > 0x7fffffff) return MM355_EINVAL;
    if (M > 4096) return MM355_EUNSUPPORTED;                 // larger passes: the format's dequantise launch + the bf16 GEMMs
    return MM355_OK;
}

// x . Wd^T (Wd: the weight as the format defines it): S > 1 -> fp32 partials workspace[slice][M][N] (`slices` written; the caller reduces
// them), S == 1 -> one slice with gemm_nt_kernel's epilogue straight into C (flags: RESIDUAL | OUT_F32)
template <class W>
int wq_launch(typename W::Args w, const mm355_bf16* x, int64_t ldx, int64_t M, int64_t N, int64_t K, int S, float* workspace, void* C, int64_t ldc,
              const mm355_bf16* residual, int64_t ldr, uint32_t flags, hipStream_t stream, int& slices) {
    GemmArgs& a = w.g;
    a = {};
    a.A = x; a.lda = ldx; a.M = (int)M; a.N = (int)N; a.K = (int)K;
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
        hipLaunchKernelGGL((gemm_wq_kernel<W, 32>), dim3((unsigned)a.ntn, (unsigned)slices), dim3(256), 2 * W::template Lane<32>::STAGE, stream, w);
    } else {
        a.ntm = (int)((M + 63) / 64);
        const int64_t total = (int64_t)a.ntm * a.ntn;
        if (total > 0x7fffffff) return MM355_EINVAL;
        hipLaunchKernelGGL((gemm_wq_kernel<W, 64>), dim3((unsigned)total, (unsigned)slices), dim3(256), 2 * W::template Lane<64>::STAGE, stream, w);
    }
    return mm_launch_status();
}

// the first launch of a split form: the S slices as partials in the caller's workspace
template <class W>
int wq_partials(const typename W::Args& w, const mm355_bf16* x, int64_t ldx, int64_t M, int64_t N, int64_t K, int S, float* workspace,
                int64_t workspace_floats, hipStream_t stream, int& slices) {
    if (!workspace || !mm_aligned16(workspace) || workspace_floats < (int64_t)S * M * N) return MM355_EINVAL;
    return wq_launch<W>(w, x, ldx, M, N, K, S, workspace, nullptr, 0, nullptr, 0, 0u, stream, slices);
}

// C = x . Wd^T (+ residual), bf16 or fp32
template <class W>
int wq_gemm(const typename W::Args& w, int fmt, const mm355_bf16* x, int64_t ldx, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
            const mm355_bf16* residual, int64_t ldr, uint32_t flags, float* workspace, int64_t workspace_floats, hipStream_t stream) {
    (void)hipGetLastError();
    if (!C) return MM355_EINVAL;
    if (flags & ~(MM355_GEMM_RESIDUAL | MM355_GEMM_OUT_F32)) return MM355_EINVAL;
    if ((flags & MM355_GEMM_RESIDUAL) && (!residual || !mm_aligned16(residual))) return MM355_EINVAL;
    if (!(flags & MM355_GEMM_RESIDUAL)) residual = nullptr;
    const int rc = wq_check<W>(w, fmt, x, ldx, M, N, K);
    if (rc != MM355_OK) return rc;
    if (!mm_aligned16(C) || ldc < N) return MM355_EINVAL;
    const int S = mm_splitk_slices(M, N, K);
    int slices = 0;
    if (S <= 1 || (flags & MM355_GEMM_OUT_F32))              // one slice, stored straight into C (fp32 output is never split: the reduce launches write bf16)
        return wq_launch<W>(w, x, ldx, M, N, K, 1, nullptr, C, ldc, residual, ldr, flags, stream, slices);
    if ((ldc & 7) || (residual && (ldr & 7))) return MM355_EINVAL;
    const int rl = wq_partials<W>(w, x, ldx, M, N, K, S, workspace, workspace_floats, stream, slices);
    if (rl != MM355_OK) return rl;
    return mm_splitk_reduce(workspace, slices, M, N, residual, ldr, (mm355_bf16*)C, ldc, stream);
}

// ... and Y = RMSNorm(C; norm_w, eps)
template <class W>
int wq_gemm_norm(const typename W::Args& w, int fmt, const mm355_bf16* x, int64_t ldx, mm355_bf16* C, int64_t M, int64_t N, int64_t K,
                 const mm355_bf16* residual, int64_t ldr, const mm355_bf16* norm_w, float eps, mm355_bf16* Y, float* workspace,
                 int64_t workspace_floats, hipStream_t stream) {
    (void)hipGetLastError();
    if (!C || !Y || !norm_w || N <= 0 || (N & 7)) return MM355_EINVAL;
    if (!mm_aligned16(C) || !mm_aligned16(Y) || !mm_aligned16(norm_w) || (residual && ((ldr & 7) || !mm_aligned16(residual)))) return MM355_EINVAL;
    const int rc = wq_check<W>(w, fmt, x, ldx, M, N, K);
    if (rc != MM355_OK) return rc;
    const int S = mm_splitk_slices(M, N, K);
    int slices = 0;
    if (S <= 1) {                                            // not split: the launch sequence, as the bf16 form
        const int rl = wq_launch<W>(w, x, ldx, M, N, K, 1, nullptr, C, N, residual, ldr, residual ? MM355_GEMM_RESIDUAL : 0u, stream, slices);
        return rl != MM355_OK ? rl : mm355_rmsnorm_fwd(C, norm_w, Y, M, N, eps, stream);
    }
    if ((N >> 3) > 8 * 256) return MM355_EUNSUPPORTED;      // (the row lives in registers: mm355_rmsnorm_fwd's own limit)
    const int rl = wq_partials<W>(w, x, ldx, M, N, K, S, workspace, workspace_floats, stream, slices);
    if (rl != MM355_OK) return rl;
    return mm_splitk_reduce_norm(workspace, slices, M, N, residual, ldr, C, norm_w, eps, Y, stream);
}

// act = SiLU(g) * u, [g | u] = x . Wd^T, N = 2 I
template <class W>
int wq_gemm_swiglu(const typename W::Args& w, int fmt, const mm355_bf16* x, int64_t ldx, mm355_bf16* act, int64_t ld_act, int64_t M, int64_t I,
                   int64_t K, float* workspace, int64_t workspace_floats, hipStream_t stream) {
    (void)hipGetLastError();
    if (!act || !workspace || I <= 0 || (I & 3) || I > 0x3fffffff || ld_act < I || !mm_aligned16(workspace)) return MM355_EINVAL;
    const int64_t N = 2 * I;
    const int rc = wq_check<W>(w, fmt, x, ldx, M, N, K);
    if (rc != MM355_OK) return rc;
    if (workspace_floats < mm_splitk_swiglu_ws_floats(M, I, K)) return MM355_EINVAL;
    const int S = mm_splitk_slices(M, N, K);
    int slices = 0;
    if (S <= 1) {
        if ((I & 7) || !mm_aligned16(act)) return MM355_EINVAL;  // (mm355_swiglu_fwd's own limits)
        if (ld_act != I) return MM355_EUNSUPPORTED;
        mm355_bf16* gu = (mm355_bf16*)workspace;
        const int rl = wq_launch<W>(w, x, ldx, M, N, K, 1, nullptr, gu, N, nullptr, 0, 0u, stream, slices);
        return rl != MM355_OK ? rl : mm355_swiglu_fwd(gu, act, M, I, stream);
    }
    const int rl = wq_partials<W>(w, x, ldx, M, N, K, S, workspace, workspace_floats, stream, slices);
    if (rl != MM355_OK) return rl;
    return mm_splitk_reduce_swiglu(workspace, slices, M, I, act, ld_act, stream);
}

// q rotated -> qkv, rotated k and v -> the cache rows positions[m]; N = (Hq + 2 Hkv) d
template <class W>
int wq_gemm_rope_append(const typename W::Args& w, int fmt, const mm355_bf16* x, int64_t ldx, mm355_bf16* qkv, int64_t ld_qkv, int64_t M, int64_t Hq,
                        int64_t Hkv, int64_t d, int64_t K, const mm355_bf16* cos_t, const mm355_bf16* sin_t, const int32_t* positions,
                        mm355_bf16* k_cache, mm355_bf16* v_cache, int64_t ld_kv, int64_t batch_stride_kv, float* workspace, int64_t workspace_floats,
                        hipStream_t stream) {
    (void)hipGetLastError();
    if (!qkv || !cos_t || !sin_t || !positions || !k_cache || !v_cache || Hq <= 0 || Hkv <= 0 || d <= 0 || (d & 15) || (ld_qkv & 7) || (ld_kv & 7) ||
        (batch_stride_kv & 7) || !mm_aligned16(qkv) || !mm_aligned16(k_cache) || !mm_aligned16(v_cache) || !mm_aligned16(cos_t) ||
        !mm_aligned16(sin_t))
        return MM355_EINVAL;
    const int64_t N = (Hq + 2 * Hkv) * d;
    if (ld_qkv < N) return MM355_EINVAL;
    const int rc = wq_check<W>(w, fmt, x, ldx, M, N, K);    // (M <= 4096: the reduce launch's grid.y)
    if (rc != MM355_OK) return rc;
    const int S = mm_splitk_slices(M, N, K);
    int slices = 0;
    if (S <= 1) {
        const int rl = wq_launch<W>(w, x, ldx, M, N, K, 1, nullptr, qkv, ld_qkv, nullptr, 0, 0u, stream, slices);
        return rl != MM355_OK ? rl
                              : mm355_rope_kv_append(qkv, ld_qkv, M, Hq, Hkv, d, cos_t, sin_t, positions, k_cache, v_cache, ld_kv, batch_stride_kv, stream);
    }
    const int rl = wq_partials<W>(w, x, ldx, M, N, K, S, workspace, workspace_floats, stream, slices);
    if (rl != MM355_OK) return rl;
    return mm_splitk_reduce_rope_append(workspace, slices, M, Hq, Hkv, d, qkv, ld_qkv, cos_t, sin_t, positions, k_cache, v_cache, ld_kv,
                                        batch_stride_kv, stream);
}

}  // namespace
