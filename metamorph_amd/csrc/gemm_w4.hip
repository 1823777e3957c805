// Weight-only MXFP4 GEMM for gfx950: C[M,N] = epilogue(x[M,K] . Wd[N,K]^T), Wd[n][k] = e2m1(nibble) * 2^(S[n][k/32] - 127): OCP e2m1 nibbles
// Wq[N][K/2] plus one e8m0 scale byte per 32 consecutive k, S[N][K/32] (the format of decode_w4.hip).  The prompt pass and decode steps of
// more than 16 sequences on a 4-bit model: the weight is streamed as NIBBLES, 0.27 x the traffic of the bf16 GEMM, instead of being
// dequantised into a scratch buffer first.
//
// The kernel is gemm_wq_kernel<W4, 32|64> (gemm_wq.h: the skeleton of gemm_nt_kernel<32|64, 128, 1, 4, true, 0> as splitk_partials of
// gemm_bf16.hip launches it, summation order kept exactly) with the policy W4 below; the host side is that header's driver.  Every Wd is
// exactly a bf16 value and the group scale sits INSIDE the widening conversion, so the B fragments are bit for bit those the bf16 kernel
// reads from the dequantised weight and so are all results, for any scales: nothing is multiplied in the epilogue and the partials of a
// split problem are plain P_s (tests/test_w4_gemm_gpu.py rests on this).
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
#include "gemm_wq.h"

namespace {

struct W4 {
    struct Args {
        GemmArgs g;
        const uint8_t* Wq; int64_t ldw;                      // bytes
        const uint8_t* S; int64_t lds;                       // bytes
    };
    static constexpr int FMT = MM355_W4_MXFP4;

    static bool operands_ok(const Args& w, int64_t K) {
        return w.Wq && w.S && !(w.ldw & 15) && w.ldw >= K / 2 && w.lds >= K / 32 && mm_aligned16(w.Wq);
    }

    template <int BM>
    struct Lane {
        static constexpr int BN = 128, NW = 4, TN = BN / NW, FN = TN / 16;
        static constexpr int A_BYTES = BM * 128, B_BYTES = BN * 32, STAGE = A_BYTES + B_BYTES;
        static_assert(B_BYTES == NW * 1024, "ONE 1-KiB DMA piece of 32 weight rows of 32 B per wave");

        int off[2], sw[2];                                   // fragment j: the 8 bytes at sb + off[j] + sw[kk] ...
        bool odd;                                            // ... of which this lane's fragment is this dword
        int wave_s;
        const uint8_t* srcB;
        const uint8_t* srcS[FN];
        uint32_t sc[FN], scn[FN];                            // the scale words of the tile in use / of the tile in flight

        MM_DEV void init(const Args& w, int64_t k_first, int n0, int wn, int wave, int lane) {
            const int fr = lane & 15, fq = lane >> 4;
            const int bx = (fr >> 3) & 1;
            const int b_off = A_BYTES + (wn * TN + fr) * 32 + (fq >> 1) * 8;
            // the second fragment's rows sit 512 B further on; the offset is kept opaque so that the two reads stay two ds_read_b64
            // (gemm_w8.hip: the ds_read2 forms are banked (byte / 4) % 32, the layout above is conflict-free for the 64-bank form only)
            int b_off1 = b_off + 512;
            asm volatile("" : "+v"(b_off1));
            const int bsw0 = bx << 4;
            const int bsw1 = (1 ^ bx) << 4;
            const bool odd = (fq & 1) != 0;                  // which dword of the 8 bytes read is this lane's fragment
            off[0] = b_off; off[1] = b_off1; sw[0] = bsw0; sw[1] = bsw1; this->odd = odd;
            wave_s = wave;
            const uint8_t* Wb = w.Wq + (k_first >> 1);
            const uint8_t* Sb = w.S + (k_first >> 5);
            const int N = w.g.N;
            const int rb = lane >> 1;                        // row inside the 32-row weight piece
            const int cb = (lane & 1) ^ ((rb >> 3) & 1);     // source chunk that belongs in LDS slot (lane & 1)
            srcB = Wb + (int64_t)min(n0 + wave_s * 32 + rb, N - 1) * w.ldw + cb * 16;
#pragma unroll
            for (int j = 0; j < FN; ++j) srcS[j] = Sb + (int64_t)min(n0 + wn * TN + j * 16 + fr, N - 1) * w.lds;
        }
        // the scale bytes of K tile kt, two per fragment row as ONE 16-bit word: byte kk = S[n_j][k0/32 + kk] (S rows need no alignment:
        // the copy leaves the form of the load to hipcc, which takes a single global_load_ushort).  One tile ahead, in front of the DMA.
        MM_DEV void ahead(int kt) {
#pragma unroll
            for (int j = 0; j < FN; ++j) {
                uint16_t v;
                __builtin_memcpy(&v, srcS[j] + 2 * kt, 2);
                scn[j] = v;
            }
        }
        // The loaded words are handed over BEHIND the barrier through an opaque move: without it hipcc unpacks them right behind the load,
        // i.e. waits vmcnt(0) between the DMA pieces.
        MM_DEV void take() {
#pragma unroll
            for (int j = 0; j < FN; ++j) {
                sc[j] = scn[j];
                asm volatile("" : "+v"(sc[j]));
            }
        }
        MM_DEV void dma(int kt, unsigned char* smem, int buf) const {
            const int64_t k0 = kt << 6;
            unsigned char* sb = smem + buf * STAGE + wave_s * 1024;
            __builtin_amdgcn_global_load_lds((gptr_t)(srcB + (k0 >> 1)), (lptr_t)(sb + A_BYTES), 16, 0, 0);
        }
        MM_DEV bf16x8 frag(const unsigned char* sb, int j, int kk) const {
            const u32x2 q = *(const u32x2*)(sb + off[j] + sw[kk]);
            uint32_t p[4];
            e2m1x8_to_bf16(odd ? q.y : q.x, e8m0_to_f32(kk ? sc[j] >> 8 : sc[j] & 0xffu), p);
            return __builtin_bit_cast(bf16x8, u32x4{p[0], p[1], p[2], p[3]});
        }
        template <int FM>
        MM_DEV void finish(f32x4 (&)[FM][2], const Args&, int) const {}   // no scale here: it sat inside the widening
    };
};

W4::Args w4_weight(const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes) {
    W4::Args w = {};
    w.Wq = Wq; w.ldw = ldw_bytes; w.S = S; w.lds = lds_bytes;
    return w;
}

}  // namespace

extern "C" int64_t mm355_gemm_w4_ws_floats(int64_t M, int64_t N, int64_t K) { return mm_splitk_ws_floats(M, N, K); }

extern "C" int mm355_gemm_w4(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes, int fmt,
                             void* C, int64_t ldc, int64_t M, int64_t N, int64_t K, const mm355_bf16* residual, int64_t ldr, uint32_t flags,
                             float* workspace, int64_t workspace_floats, void* stream) {
    return wq_gemm<W4>(w4_weight(Wq, ldw_bytes, S, lds_bytes), fmt, x, ldx, C, ldc, M, N, K, residual, ldr, flags, workspace, workspace_floats,
                       (hipStream_t)stream);
}

extern "C" int mm355_gemm_w4_norm(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes,
                                  int fmt, mm355_bf16* C, int64_t M, int64_t N, int64_t K, const mm355_bf16* residual, int64_t ldr,
                                  const mm355_bf16* norm_w, float eps, mm355_bf16* Y, float* workspace, int64_t workspace_floats, void* stream) {
    return wq_gemm_norm<W4>(w4_weight(Wq, ldw_bytes, S, lds_bytes), fmt, x, ldx, C, M, N, K, residual, ldr, norm_w, eps, Y, workspace,
                            workspace_floats, (hipStream_t)stream);
}

extern "C" int64_t mm355_gemm_w4_swiglu_ws_floats(int64_t M, int64_t I, int64_t K) { return mm_splitk_swiglu_ws_floats(M, I, K); }

extern "C" int mm355_gemm_w4_swiglu(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes,
                                    int fmt, mm355_bf16* act, int64_t ld_act, int64_t M, int64_t I, int64_t K, float* workspace,
                                    int64_t workspace_floats, void* stream) {
    return wq_gemm_swiglu<W4>(w4_weight(Wq, ldw_bytes, S, lds_bytes), fmt, x, ldx, act, ld_act, M, I, K, workspace, workspace_floats,
                              (hipStream_t)stream);
}

extern "C" int mm355_gemm_w4_rope_append(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S,
                                         int64_t lds_bytes, int fmt, mm355_bf16* qkv, int64_t ld_qkv, int64_t M, int64_t Hq, int64_t Hkv,
                                         int64_t d, int64_t K, const mm355_bf16* cos_t, const mm355_bf16* sin_t, const int32_t* positions,
                                         mm355_bf16* k_cache, mm355_bf16* v_cache, int64_t ld_kv, int64_t batch_stride_kv, float* workspace,
                                         int64_t workspace_floats, void* stream) {
    return wq_gemm_rope_append<W4>(w4_weight(Wq, ldw_bytes, S, lds_bytes), fmt, x, ldx, qkv, ld_qkv, M, Hq, Hkv, d, K, cos_t, sin_t, positions,
                                   k_cache, v_cache, ld_kv, batch_stride_kv, workspace, workspace_floats, (hipStream_t)stream);
}
