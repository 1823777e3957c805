// Weight-only FP8 GEMM for gfx950: C[M,N] = epilogue(scale[n] * x[M,K] . fp32(Wq[N,K])^T), Wq = OCP e4m3fn bytes, one fp32 scale per output
// row (the format of decode_w8.hip).  The prompt pass and decode steps of more than 16 sequences on a quantised model: the weight is streamed
// as BYTES, half the traffic of the bf16 GEMM, instead of being dequantised into a scratch buffer first.
//
// The kernel is the twin of gemm_nt_kernel<32|64, 128, 1, 4, true, 0> as splitk_partials (gemm_bf16.hip) launches it, and keeps its
// summation order exactly: the same slices (mm_splitk_slices), the same kslice, 64-wide K tiles, per tile and fragment the two
// v_mfma_f32_16x16x32_bf16 in the same order with the same k in every operand slot (lane group fq holds k = kk*32 + fq*8 .. +7).  Every
// product bf16 x e4m3 is exact in fp32, so with power-of-two scales the results equal those of the bf16 kernel on the dequantised weight
// bit for bit (tests/test_w8_gemm_gpu.py rests on this).
//   * A (x) tiles: LDS-DMA into [rows][64 bf16] with the 16-B chunk index XOR-ed with (row & 7), as in gemm_bf16.hip.
//   * B (weight) tiles: LDS-DMA of bytes.  A B row of a K tile is 64 bytes, a DMA piece (64 lanes x 16 B, lane-linear in LDS) is 16 rows x
//     four 16-B chunks; lane L lands in (row L >> 2, slot L & 3) and fetches source chunk (L & 3) ^ ((row >> 2) & 3).  A fragment read is
//     one ds_read_b64 per lane: row fr, k-step kk, lane group fq -> chunk c = kk*2 + (fq >> 1), half fq & 1, at byte
//     row*64 + ((c ^ ((fr >> 2) & 3)) << 4) + (fq & 1)*8.  ds_read_b64 is served per 32-lane half, bank = (byte / 4) % 64: within a half
//     (fq in {0,1} or {2,3}, all fr) c is one value, rows fr and fr + 4 share a 64-B bank group and (fr >> 2) spreads them over its four
//     chunks, fr & 3 picks the bank group, fq & 1 the 8-B half: 32 lanes on 32 distinct 8-B bank pairs.  Checked by enumerating
//     (byte / 4) % 64 over both halves, both k-steps and both fragments of every wave: each of the 64 banks is hit exactly once per half
//     (the check is tests/test_w8_gemm_host.py::test_b_tile_layout_is_conflict_free_and_complete, which also checks that the DMA image and
//     the fragment reads agree on where every (row, k) byte lives).
//   * widening: the 8 bytes of a fragment -> 8 bf16 in registers with e4m3x4_to_bf16 (v_cvt_pk_f32_fp8 + v_perm_b32, exact), k order kept.
//     64 x 128 tile: 16 conversions + 16 permutes per thread and K tile beside 16 MFMAs per wave.
//   * scale: every fp32 accumulator is multiplied by scale[n] where the kernel stores it -- a split problem stores scale[n] * P_s per slice
//     and the unchanged reduce kernels of gemm_bf16.hip add the slices: sum_s scale * P_s instead of scale * sum_s P_s (identical for
//     power-of-two scales, otherwise one fp32 rounding per slice).  An unsplit problem (one slice) stores epilogue(scale[n] * P) straight
//     into C (residual / fp32 output as mm355_gemm_bf16).
#include "gemm_common.h"
#include "splitk.h"

namespace {

struct GemmW8Args {
    GemmArgs g;                                              // A = x, C / res / flags / kslice as the bf16 kernel; B and ldb unused
    const uint8_t* Wq; int64_t ldw;                          // bytes
    const float* scale;
};

template <int BM>
__global__ __launch_bounds__(256) void gemm_w8_kernel(GemmW8Args w) {
    constexpr int BN = 128, NW = 4;
    constexpr int TM = BM, TN = BN / NW, FM = TM / 16, FN = TN / 16;
    constexpr int A_BYTES = BM * 128, B_BYTES = BN * 64, STAGE = A_BYTES + B_BYTES;
    constexpr int AI = BM / 8 / NW, BI = BN / 16 / NW;       // 1-KiB DMA pieces per wave: 8 x rows of 128 B, 16 weight rows of 64 B
    constexpr int GM = 8;
    static_assert(AI >= 1 && BI >= 1 && FN == 2, "tile shape");
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
    const uint8_t* Wb = w.Wq + (int64_t)sl * a.kslice;
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
    const int bx = (fr >> 2) & 3;
    const int b_off = A_BYTES + (wn * TN + fr) * 64 + (fq & 1) * 8;
    // the second fragment's rows sit 1 KiB further on; the offset is kept opaque so that the two reads stay two ds_read_b64: with both
    // offsets visible hipcc merges them into one ds_read2st64_b64, and the ds_read2 forms are banked (byte / 4) % 32 and documented at
    // 16 bytes per lane in 16 LDS cycles against 2 x 2 cycles for two ds_read_b64 -- the layout above is conflict-free for the 64-bank form
    // only.  Reasoned from those documented rates; the merged form was NOT timed against this one on the device.
    int b_off1 = b_off + 1024;
    asm volatile("" : "+v"(b_off1));
    const int bsw0 = (((fq >> 1)) ^ bx) << 4;
    const int bsw1 = ((2 + (fq >> 1)) ^ bx) << 4;

    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const uint16_t* srcA[AI];
    const uint8_t* srcB[BI];
    {
        const int rin = lane >> 3;                           // row inside the 8-row x piece
        const int c = (lane & 7) ^ rin;                      // source chunk that belongs in LDS slot (lane & 7)
#pragma unroll
        for (int i = 0; i < AI; ++i)
            srcA[i] = Ab + (int64_t)min(m0 + (i * NW + wave_s) * 8 + rin, M - 1) * a.lda + c * 8;
        const int rb = lane >> 2;                            // row inside the 16-row weight piece
        const int cb = (lane & 3) ^ ((rb >> 2) & 3);         // source chunk that belongs in LDS slot (lane & 3)
#pragma unroll
        for (int i = 0; i < BI; ++i)
            srcB[i] = Wb + (int64_t)min(n0 + (i * NW + wave_s) * 16 + rb, N - 1) * w.ldw + cb * 16;
    }
    auto gdma = [&](int kt, int buf) {
        const int64_t k0 = kt << 6;
        unsigned char* sb = smem + buf * STAGE + wave_s * 1024;
#pragma unroll
        for (int i = 0; i < AI; ++i)
            __builtin_amdgcn_global_load_lds((gptr_t)(srcA[i] + k0), (lptr_t)(sb + i * NW * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < BI; ++i)
            __builtin_amdgcn_global_load_lds((gptr_t)(srcB[i] + k0), (lptr_t)(sb + A_BYTES + i * NW * 1024), 16, 0, 0);
    };

    // ---- main loop: gemm_nt_kernel's two-stage schedule (next tile in flight during the MFMAs)
    gdma(0, 0);
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) gdma(kt + 1, cur ^ 1);
        const unsigned char* sb = smem + cur * STAGE;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 af[FM], bf[FN];
#pragma unroll
            for (int i = 0; i < FM; ++i) af[i] = *(const bf16x8*)(sb + a_off + i * 2048 + (kk ? sw1 : sw0));
#pragma unroll
            for (int j = 0; j < FN; ++j) {
                const u32x2 q = *(const u32x2*)(sb + (j ? b_off1 : b_off) + (kk ? bsw1 : bsw0));
                u32x4 p;
                uint32_t lo, hi;
                e4m3x4_to_bf16(q.x, lo, hi); p.x = lo; p.y = hi;
                e4m3x4_to_bf16(q.y, lo, hi); p.z = lo; p.w = hi;
                bf[j] = __builtin_bit_cast(bf16x8, p);
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

    // ---- epilogue: the scale, then gemm_nt_kernel's store (accumulator element r of fragment j is column j*16 + fr of the wave's 32)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const float s = w.scale[min(n0 + wn * TN + j * 16 + fr, N - 1)];
#pragma unroll
        for (int i = 0; i < FM; ++i) acc[i][j] *= s;
    }
    GemmArgs e = a;
    if (a.kslice) e.C = (float*)a.C + (int64_t)sl * a.M * a.ldc;     // this slice's partial tile, plain fp32
    gemm_epilogue<TM, TN, FM, FN>(acc, e, smem, m0, n0, 0, wn, wave, lane);
}

// x rows, weight bytes and scales in the form the kernel addresses them; everything a launch depends on, before any launch
int w8_gemm_check(const void* x, int64_t ldx, const void* Wq, int64_t ldw, const float* scale, int fmt, int64_t M, int64_t N, int64_t K) {
    if (!x || !Wq || !scale || M <= 0 || N <= 0 || K <= 0) return MM355_EINVAL;
    if (fmt != MM355_W8_E4M3) return MM355_EINVAL;
    if ((K & 63) || (ldx & 7) || ldx < K || (ldw & 15) || ldw < K || !mm_aligned16(x) || !mm_aligned16(Wq) || (((uintptr_t)scale) & 3u)) return MM355_EINVAL;
    if (N > 0x7fffffff || K > 0x7fffffff) return MM355_EINVAL;
    if (M > 4096) return MM355_EUNSUPPORTED;                 // larger passes: mm355_dequant_w8_bf16 + the bf16 GEMMs
    return MM355_OK;
}

// scale[n] * (x . Wq^T): S > 1 -> fp32 partials workspace[slice][M][N] (`slices` written; the caller reduces them), S == 1 -> one slice
// with gemm_nt_kernel's epilogue straight into C (flags: RESIDUAL | OUT_F32)
int w8_gemm_launch(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw, const float* scale, int64_t M, int64_t N, int64_t K, int S,
                   float* workspace, void* C, int64_t ldc, const mm355_bf16* residual, int64_t ldr, uint32_t flags, hipStream_t stream, int& slices) {
    GemmW8Args w = {};
    GemmArgs& a = w.g;
    a.A = x; a.lda = ldx; a.M = (int)M; a.N = (int)N; a.K = (int)K;
    w.Wq = Wq; w.ldw = ldw; w.scale = scale;
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
        hipLaunchKernelGGL(gemm_w8_kernel<32>, dim3((unsigned)a.ntn, (unsigned)slices), dim3(256), 2 * (32 * 128 + 128 * 64), stream, w);
    } else {
        a.ntm = (int)((M + 63) / 64);
        const int64_t total = (int64_t)a.ntm * a.ntn;
        if (total > 0x7fffffff) return MM355_EINVAL;
        hipLaunchKernelGGL(gemm_w8_kernel<64>, dim3((unsigned)total, (unsigned)slices), dim3(256), 2 * (64 * 128 + 128 * 64), stream, w);
    }
    return mm_launch_status();
}

}  // namespace

extern "C" int64_t mm355_gemm_w8_ws_floats(int64_t M, int64_t N, int64_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const int S = mm_splitk_slices(M, N, K);
    return S > 1 ? (int64_t)S * M * N : 0;
}

extern "C" int mm355_gemm_w8(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt, void* C,
                             int64_t ldc, int64_t M, int64_t N, int64_t K, const mm355_bf16* residual, int64_t ldr, uint32_t flags,
                             float* workspace, int64_t workspace_floats, void* stream) {
    (void)hipGetLastError();
    if (!C) return MM355_EINVAL;
    if (flags & ~(MM355_GEMM_RESIDUAL | MM355_GEMM_OUT_F32)) return MM355_EINVAL;
    if ((flags & MM355_GEMM_RESIDUAL) && (!residual || !mm_aligned16(residual))) return MM355_EINVAL;
    if (!(flags & MM355_GEMM_RESIDUAL)) residual = nullptr;
    const int rc = w8_gemm_check(x, ldx, Wq, ldw_bytes, scale, fmt, M, N, K);
    if (rc != MM355_OK) return rc;
    if (!mm_aligned16(C) || ldc < N) return MM355_EINVAL;
    const int S = mm_splitk_slices(M, N, K);
    const bool f32 = (flags & MM355_GEMM_OUT_F32) != 0;
    int slices = 0;
    if (S <= 1 || f32) {                                     // one slice, stored straight into C (fp32 output is never split: the reduce launches write bf16)
        return w8_gemm_launch(x, ldx, Wq, ldw_bytes, scale, M, N, K, 1, nullptr, C, ldc, residual, ldr, flags, (hipStream_t)stream, slices);
    }
    if ((ldc & 7) || (residual && (ldr & 7)) || !workspace || !mm_aligned16(workspace) || workspace_floats < (int64_t)S * M * N) return MM355_EINVAL;
    const int rl = w8_gemm_launch(x, ldx, Wq, ldw_bytes, scale, M, N, K, S, workspace, nullptr, 0, nullptr, 0, 0u, (hipStream_t)stream, slices);
    if (rl != MM355_OK) return rl;
    return mm_splitk_reduce(workspace, slices, M, N, residual, ldr, (mm355_bf16*)C, ldc, (hipStream_t)stream);
}

extern "C" int mm355_gemm_w8_norm(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt,
                                  mm355_bf16* C, int64_t M, int64_t N, int64_t K, const mm355_bf16* residual, int64_t ldr,
                                  const mm355_bf16* norm_w, float eps, mm355_bf16* Y, float* workspace, int64_t workspace_floats, void* stream) {
    (void)hipGetLastError();
    if (!C || !Y || !norm_w || N <= 0 || (N & 7)) return MM355_EINVAL;
    if (!mm_aligned16(C) || !mm_aligned16(Y) || !mm_aligned16(norm_w) || (residual && ((ldr & 7) || !mm_aligned16(residual)))) return MM355_EINVAL;
    const int rc = w8_gemm_check(x, ldx, Wq, ldw_bytes, scale, fmt, M, N, K);
    if (rc != MM355_OK) return rc;
    const int S = mm_splitk_slices(M, N, K);
    int slices = 0;
    if (S <= 1) {                                            // not split: the launch sequence, as the bf16 twin
        const int rl = w8_gemm_launch(x, ldx, Wq, ldw_bytes, scale, M, N, K, 1, nullptr, C, N, residual, ldr, residual ? MM355_GEMM_RESIDUAL : 0u,
                                      (hipStream_t)stream, slices);
        return rl != MM355_OK ? rl : mm355_rmsnorm_fwd(C, norm_w, Y, M, N, eps, stream);
    }
    if ((N >> 3) > 8 * 256) return MM355_EUNSUPPORTED;      // (the row lives in registers: mm355_rmsnorm_fwd's own limit)
    if (!workspace || !mm_aligned16(workspace) || workspace_floats < (int64_t)S * M * N) return MM355_EINVAL;
    const int rl = w8_gemm_launch(x, ldx, Wq, ldw_bytes, scale, M, N, K, S, workspace, nullptr, 0, nullptr, 0, 0u, (hipStream_t)stream, slices);
    if (rl != MM355_OK) return rl;
    return mm_splitk_reduce_norm(workspace, slices, M, N, residual, ldr, C, norm_w, eps, Y, (hipStream_t)stream);
}

extern "C" int64_t mm355_gemm_w8_swiglu_ws_floats(int64_t M, int64_t I, int64_t K) {
    if (M <= 0 || I <= 0 || K <= 0) return 0;
    const int S = mm_splitk_slices(M, 2 * I, K);
    return S > 1 ? (int64_t)S * M * 2 * I : M * I;          // not split: the bf16 [M][2 I] gate | up rows of the plain sequence
}

extern "C" int mm355_gemm_w8_swiglu(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt,
                                    mm355_bf16* act, int64_t ld_act, int64_t M, int64_t I, int64_t K, float* workspace, int64_t workspace_floats,
                                    void* stream) {
    (void)hipGetLastError();
    if (!act || !workspace || I <= 0 || (I & 3) || I > 0x3fffffff || ld_act < I || !mm_aligned16(workspace)) return MM355_EINVAL;
    const int64_t N = 2 * I;
    const int rc = w8_gemm_check(x, ldx, Wq, ldw_bytes, scale, fmt, M, N, K);
    if (rc != MM355_OK) return rc;
    if (workspace_floats < mm355_gemm_w8_swiglu_ws_floats(M, I, K)) return MM355_EINVAL;
    const int S = mm_splitk_slices(M, N, K);
    int slices = 0;
    if (S <= 1) {
        if ((I & 7) || !mm_aligned16(act)) return MM355_EINVAL;  // (mm355_swiglu_fwd's own limits)
        if (ld_act != I) return MM355_EUNSUPPORTED;
        mm355_bf16* gu = (mm355_bf16*)workspace;
        const int rl = w8_gemm_launch(x, ldx, Wq, ldw_bytes, scale, M, N, K, 1, nullptr, gu, N, nullptr, 0, 0u, (hipStream_t)stream, slices);
        return rl != MM355_OK ? rl : mm355_swiglu_fwd(gu, act, M, I, stream);
    }
    const int rl = w8_gemm_launch(x, ldx, Wq, ldw_bytes, scale, M, N, K, S, workspace, nullptr, 0, nullptr, 0, 0u, (hipStream_t)stream, slices);
    if (rl != MM355_OK) return rl;
    return mm_splitk_reduce_swiglu(workspace, slices, M, I, act, ld_act, (hipStream_t)stream);
}

extern "C" int mm355_gemm_w8_rope_append(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt,
                                         mm355_bf16* qkv, int64_t ld_qkv, int64_t M, int64_t Hq, int64_t Hkv, int64_t d, int64_t K,
                                         const mm355_bf16* cos_t, const mm355_bf16* sin_t, const int32_t* positions, mm355_bf16* k_cache,
                                         mm355_bf16* v_cache, int64_t ld_kv, int64_t batch_stride_kv, float* workspace, int64_t workspace_floats,
                                         void* stream) {
    (void)hipGetLastError();
    if (!qkv || !cos_t || !sin_t || !positions || !k_cache || !v_cache || Hq <= 0 || Hkv <= 0 || d <= 0 || (d & 15) || (ld_qkv & 7) || (ld_kv & 7) ||
        (batch_stride_kv & 7) || !mm_aligned16(qkv) || !mm_aligned16(k_cache) || !mm_aligned16(v_cache) || !mm_aligned16(cos_t) ||
        !mm_aligned16(sin_t))
        return MM355_EINVAL;
    const int64_t N = (Hq + 2 * Hkv) * d;
    if (ld_qkv < N) return MM355_EINVAL;
    const int rc = w8_gemm_check(x, ldx, Wq, ldw_bytes, scale, fmt, M, N, K);
    if (rc != MM355_OK) return rc;
    const int S = mm_splitk_slices(M, N, K);
    int slices = 0;
    if (S <= 1) {
        const int rl = w8_gemm_launch(x, ldx, Wq, ldw_bytes, scale, M, N, K, 1, nullptr, qkv, ld_qkv, nullptr, 0, 0u, (hipStream_t)stream, slices);
        return rl != MM355_OK ? rl
                              : mm355_rope_kv_append(qkv, ld_qkv, M, Hq, Hkv, d, cos_t, sin_t, positions, k_cache, v_cache, ld_kv, batch_stride_kv, stream);
    }
    if (!workspace || !mm_aligned16(workspace) || workspace_floats < (int64_t)S * M * N) return MM355_EINVAL;
    const int rl = w8_gemm_launch(x, ldx, Wq, ldw_bytes, scale, M, N, K, S, workspace, nullptr, 0, nullptr, 0, 0u, (hipStream_t)stream, slices);
    if (rl != MM355_OK) return rl;
    return mm_splitk_reduce_rope_append(workspace, slices, M, Hq, Hkv, d, qkv, ld_qkv, cos_t, sin_t, positions, k_cache, v_cache, ld_kv,
                                        batch_stride_kv, (hipStream_t)stream);
}
