// Weight-only FP8 GEMM for gfx950: C[M,N] = epilogue(scale[n] * x[M,K] . fp32(Wq[N,K])^T), Wq = OCP e4m3fn bytes, one fp32 scale per output
// row (the format of decode_w8.hip).  The prompt pass and decode steps of more than 16 sequences on a quantised model: the weight is streamed
// as BYTES, half the traffic of the bf16 GEMM, instead of being dequantised into a scratch buffer first.
//
// The kernel is gemm_wq_kernel<W8, 32|64> (gemm_wq.h: the skeleton of gemm_nt_kernel<32|64, 128, 1, 4, true, 0> as splitk_partials of
// gemm_bf16.hip launches it, summation order kept exactly) with the policy W8 below; the host side is that header's driver.  Every product
// bf16 x e4m3 is exact in fp32, so with power-of-two scales the results equal those of the bf16 kernel on the dequantised weight bit for
// bit (tests/test_w8_gemm_gpu.py rests on this).
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
#include "gemm_wq.h"

namespace {

struct W8 {
    struct Args {
        GemmArgs g;
        const uint8_t* Wq; int64_t ldw;                      // bytes
        const float* scale;
    };
    static constexpr int FMT = MM355_W8_E4M3;

    static bool operands_ok(const Args& w, int64_t K) {
        return w.Wq && w.scale && !(w.ldw & 15) && w.ldw >= K && mm_aligned16(w.Wq) && !(((uintptr_t)w.scale) & 3u);
    }

    template <int BM>
    struct Lane {
        static constexpr int BN = 128, NW = 4, TN = BN / NW;
        static constexpr int A_BYTES = BM * 128, B_BYTES = BN * 64, STAGE = A_BYTES + B_BYTES;
        static constexpr int BI = BN / 16 / NW;              // 1-KiB DMA pieces per wave: 16 weight rows of 64 B

        int off[2], sw[2];                                   // fragment j at sb + off[j] + sw[kk]
        int wave_s;
        const uint8_t* srcB[BI];

        MM_DEV void init(const Args& w, int64_t k_first, int n0, int wn, int wave, int lane) {
            const int fr = lane & 15, fq = lane >> 4;
            const int bx = (fr >> 2) & 3;
            const int b_off = A_BYTES + (wn * TN + fr) * 64 + (fq & 1) * 8;
            // the second fragment's rows sit 1 KiB further on; the offset is kept opaque so that the two reads stay two ds_read_b64: with
            // both offsets visible hipcc merges them into one ds_read2st64_b64, and the ds_read2 forms are banked (byte / 4) % 32 and
            // documented at 16 bytes per lane in 16 LDS cycles against 2 x 2 cycles for two ds_read_b64 -- the layout above is conflict-free
            // for the 64-bank form only.  Reasoned from those documented rates; the merged form was NOT timed against this one on the device.
            int b_off1 = b_off + 1024;
            asm volatile("" : "+v"(b_off1));
            const int bsw0 = (((fq >> 1)) ^ bx) << 4;
            const int bsw1 = ((2 + (fq >> 1)) ^ bx) << 4;
            off[0] = b_off; off[1] = b_off1; sw[0] = bsw0; sw[1] = bsw1;
            wave_s = wave;
            const uint8_t* Wb = w.Wq + k_first;
            const int N = w.g.N;
            const int rb = lane >> 2;                        // row inside the 16-row weight piece
            const int cb = (lane & 3) ^ ((rb >> 2) & 3);     // source chunk that belongs in LDS slot (lane & 3)
#pragma unroll
            for (int i = 0; i < BI; ++i)
                srcB[i] = Wb + (int64_t)min(n0 + (i * NW + wave_s) * 16 + rb, N - 1) * w.ldw + cb * 16;
        }
        MM_DEV void ahead(int) {}                            // nothing travels beside the tile
        MM_DEV void take() {}
        MM_DEV void dma(int kt, unsigned char* smem, int buf) const {
            const int64_t k0 = kt << 6;
            unsigned char* sb = smem + buf * STAGE + wave_s * 1024;
#pragma unroll
            for (int i = 0; i < BI; ++i)
                __builtin_amdgcn_global_load_lds((gptr_t)(srcB[i] + k0), (lptr_t)(sb + A_BYTES + i * NW * 1024), 16, 0, 0);
        }
        MM_DEV bf16x8 frag(const unsigned char* sb, int j, int kk) const {
            const u32x2 q = *(const u32x2*)(sb + off[j] + sw[kk]);
            u32x4 p;
            uint32_t lo, hi;
            e4m3x4_to_bf16(q.x, lo, hi); p.x = lo; p.y = hi;
            e4m3x4_to_bf16(q.y, lo, hi); p.z = lo; p.w = hi;
            return __builtin_bit_cast(bf16x8, p);
        }
        // the scale of this lane's two columns (col, col + 16) on every accumulator
        template <int FM>
        MM_DEV void finish(f32x4 (&acc)[FM][2], const Args& w, int col) const {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float s = w.scale[min(col + j * 16, w.g.N - 1)];
#pragma unroll
                for (int i = 0; i < FM; ++i) acc[i][j] *= s;
            }
        }
    };
};

W8::Args w8_weight(const uint8_t* Wq, int64_t ldw_bytes, const float* scale) {
    W8::Args w = {};
    w.Wq = Wq; w.ldw = ldw_bytes; w.scale = scale;
    return w;
}

}  // namespace

extern "C" int64_t mm355_gemm_w8_ws_floats(int64_t M, int64_t N, int64_t K) { return mm_splitk_ws_floats(M, N, K); }

extern "C" int mm355_gemm_w8(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt, void* C,
                             int64_t ldc, int64_t M, int64_t N, int64_t K, const mm355_bf16* residual, int64_t ldr, uint32_t flags,
                             float* workspace, int64_t workspace_floats, void* stream) {
    return wq_gemm<W8>(w8_weight(Wq, ldw_bytes, scale), fmt, x, ldx, C, ldc, M, N, K, residual, ldr, flags, workspace, workspace_floats,
                       (hipStream_t)stream);
}

extern "C" int mm355_gemm_w8_norm(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt,
                                  mm355_bf16* C, int64_t M, int64_t N, int64_t K, const mm355_bf16* residual, int64_t ldr,
                                  const mm355_bf16* norm_w, float eps, mm355_bf16* Y, float* workspace, int64_t workspace_floats, void* stream) {
    return wq_gemm_norm<W8>(w8_weight(Wq, ldw_bytes, scale), fmt, x, ldx, C, M, N, K, residual, ldr, norm_w, eps, Y, workspace, workspace_floats,
                            (hipStream_t)stream);
}

extern "C" int64_t mm355_gemm_w8_swiglu_ws_floats(int64_t M, int64_t I, int64_t K) { return mm_splitk_swiglu_ws_floats(M, I, K); }

extern "C" int mm355_gemm_w8_swiglu(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt,
                                    mm355_bf16* act, int64_t ld_act, int64_t M, int64_t I, int64_t K, float* workspace, int64_t workspace_floats,
                                    void* stream) {
    return wq_gemm_swiglu<W8>(w8_weight(Wq, ldw_bytes, scale), fmt, x, ldx, act, ld_act, M, I, K, workspace, workspace_floats, (hipStream_t)stream);
}

extern "C" int mm355_gemm_w8_rope_append(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt,
                                         mm355_bf16* qkv, int64_t ld_qkv, int64_t M, int64_t Hq, int64_t Hkv, int64_t d, int64_t K,
                                         const mm355_bf16* cos_t, const mm355_bf16* sin_t, const int32_t* positions, mm355_bf16* k_cache,
                                         mm355_bf16* v_cache, int64_t ld_kv, int64_t batch_stride_kv, float* workspace, int64_t workspace_floats,
                                         void* stream) {
    return wq_gemm_rope_append<W8>(w8_weight(Wq, ldw_bytes, scale), fmt, x, ldx, qkv, ld_qkv, M, Hq, Hkv, d, K, cos_t, sin_t, positions, k_cache,
                                   v_cache, ld_kv, batch_stride_kv, workspace, workspace_floats, (hipStream_t)stream);
}
