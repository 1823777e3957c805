// Decode GEMVs over weight-only MXFP4 (gfx950): W[N][K] stored as OCP e2m1 nibbles Wq[N][K/2] (byte j of a row: k = 2j in bits 3:0,
// k = 2j+1 in bits 7:4) plus one e8m0 scale byte per 32 consecutive k, S[N][K/32]; dequantised value e2m1(nibble) * 2^(S - 127).  A quarter
// of the bf16 bytes (4.25 bits per weight); the counterpart of the reference's load_4bit=True (metamorph/model/builder.py:13-25).
//   y[m][n] = epilogue(sum_k fp32(Wd[n][k]) * fp32(x[m][k]))       x bf16, fp32 accumulation, the group scale INSIDE the conversion
// Every Wd is exactly a bf16 value and every product exact in fp32, so only the summation order separates these kernels from an exact
// evaluation.  The structure is that of decode_w8.hip, with 32 weights = ONE scale group per 16-byte load:
//   * the x rows (PRENORM: bf16(w * bf16(x * rstd)), rmsnorm_fwd_kernel's arithmetic and reduction order) are parked in LDS windows, so
//     that once the stream runs only weight and scale loads sit in the in-order vector-memory queue;
//   * a register ring of trips, each load with its scale byte (the 64 lanes of a wave read 64 contiguous scale bytes of a row); lanes
//     behind the end of a row carry the out-of-range mark of the buffer descriptors (zeros, no memory access);
//   * v_cvt_scalef32_pk_bf16_fp4 turns one byte (two e2m1 values) and the group scale (an fp32 whose exponent field is S) into the packed
//     bf16 pair that v_dot2c_f32_bf16 (up to four rows) and v_mfma_f32_16x16x32_bf16 (5 .. 16 rows) take: ONE widening instruction per
//     two weights, nothing is multiplied after the sum.  x stays bf16.
//   * the epilogues (bias / GELU / residual; SiLU(g) u; RoPE + cache append) are decode_gemv.h's, shared with decode_w8.hip; a fused form
//     and the launch sequence it replaces run the same stream in the same order: the same bits.
#include "decode_gemv.h"

namespace {

// (the widening helpers e2m1x8_to_bf16 / e8m0_to_f32 live in mm355_common.h: shared with gemm_w4.hip)

// ------------------------------------------------------------------------------------------------ up to four rows: the vector ALU
// A wave owns one unit (four weight rows) over the whole K.  A trip = 2048 columns x 4 rows = four 16-byte loads and four scale bytes per
// lane (lane l: columns 32 l .. 32 l + 31 of the trip, one scale group); NB trips ride in the register ring.  The x rows pass through LDS in
// windows of WK columns (two buffers when a row is longer than one window).  A lane reads its 64 bytes of an x row as four 16-byte
// vectors; vector v of a row sits at slot v ^ (((v >> 2) ^ (v >> 4)) & 3), which spreads the 16 lanes of a ds_read_b128 group over all
// 64 banks.  Every weight dword is widened once (four conversions) and feeds MR dot2 chains.
template <int MR, int MODE, bool PRENORM>
__global__ __launch_bounds__(NT) void gemv_w4_valu_kernel(WqArgs a) {
    constexpr int R = 4, NB = 4;
    constexpr int WK = MR == 4 ? 4096 : 8192;                // columns per x window
    constexpr int WT = WK / 2048;                            // trips per window
    constexpr int XV = WK / 8 / NT;                          // 16-byte x vectors per thread, row and window
    extern __shared__ __attribute__((aligned(16))) unsigned char xs[];          // [1 or 2 windows][MR][wk] bf16
    __shared__ float red[MR][NT / 64];
    __shared__ float rstd_s[MR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int unit = blockIdx.x * (NT / 64) + wave;
    const int K = a.K, M = a.M;
    const int ntrip = (K + 2047) >> 11, nwin = (ntrip + WT - 1) / WT, nv = K >> 3;
    const int wk = min(ntrip, WT) << 11;                     // elements per window row in LDS
    int rows[R];
    unit_rows<MODE>(a, unit, rows);
    const bool live = unit_live<MODE>(a, rows);
    const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)a.W, 0, (uint32_t)((uint64_t)(a.N - 1) * a.ldw + (uint64_t)(K >> 1)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsS = __builtin_amdgcn_make_buffer_rsrc((void*)a.S, 0, (uint32_t)((uint64_t)(a.N - 1) * a.lds + (uint64_t)(K >> 5)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (uint32_t)((uint64_t)(M - 1) * a.ldx * 2 + (uint64_t)K * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsN = __builtin_amdgcn_make_buffer_rsrc((void*)(PRENORM ? a.norm_w : a.x), 0, (uint32_t)K * 2u, 0x00020000);
    uint32_t wo[R], so[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        wo[r] = (uint32_t)min(rows[r], a.N - 1) * (uint32_t)a.ldw;
        so[r] = (uint32_t)min(rows[r], a.N - 1) * (uint32_t)a.lds;
    }
    u32x4 xr[MR][XV], nr[XV];
    auto stage_load = [&](int w) {                           // this thread's vectors v = t + 256 i of window w; beyond K: zeros, no access
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            const int v = w * (WK / 8) + threadIdx.x + NT * i;
            const uint32_t sk = v < nv ? 0u : OOB;
#pragma unroll
            for (int m = 0; m < MR; ++m)
                xr[m][i] = __builtin_amdgcn_raw_buffer_load_b128(rsX, ((uint32_t)min(m, M - 1) * (uint32_t)a.ldx * 2u + (uint32_t)v * 16u) | sk, 0, 0);
            if constexpr (PRENORM) nr[i] = __builtin_amdgcn_raw_buffer_load_b128(rsN, ((uint32_t)v * 16u) | sk, 0, 0);
        }
    };
    auto stage_store = [&](int w) {                          // -> LDS window buffer w & 1
        unsigned char* dst = xs + (size_t)(w & 1) * MR * wk * 2;
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            const int v = threadIdx.x + NT * i;
            if (v * 8 < wk) {
                const int slot = v ^ (((v >> 2) ^ (v >> 4)) & 3);
#pragma unroll
                for (int m = 0; m < MR; ++m) {
                    u32x4 out = xr[m][i];
                    if constexpr (PRENORM) {
                        float xv[8], nw[8];
                        unpack8(xr[m][i], xv);
                        unpack8(nr[i], nw);
                        const float rs = rstd_s[m];
#pragma unroll
                        for (int e = 0; e < 8; ++e) xv[e] = nw[e] * round_bf(xv[e] * rs);
                        out = pack8(xv);
                    }
                    *(u32x4*)(dst + ((size_t)m * wk + slot * 8) * 2) = out;
                }
            }
        }
    };
    auto issue = [&](u32x4 (&w)[R], uint32_t (&s)[R], int t) {
        const int k = t * 2048 + lane * 32;
        const uint32_t sk = (live && k < K) ? 0u : OOB;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            w[r] = __builtin_amdgcn_raw_buffer_load_b128(rsW, (wo[r] + (uint32_t)(k >> 1)) | sk, 0, 2);
            s[r] = __builtin_amdgcn_raw_buffer_load_b8(rsS, (so[r] + (uint32_t)(k >> 5)) | sk, 0, 2);
        }
    };
    // rmsnorm_fwd_kernel's reduction (thread t sums elements 8 (t + 256 i) .. + 7 in order, block_sum<256>), all rows in one pass
    auto finish_norm = [&](float (&ss)[MR]) {
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            const float w = wave_sum(ss[m]);
            if (lane == 0) red[m][wave] = w;
        }
        __syncthreads();
        if (threadIdx.x < MR) {
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < NT / 64; ++i) t += red[threadIdx.x][i];
            rstd_s[threadIdx.x] = rsqrtf(t / (float)K + a.eps);
        }
        __syncthreads();
    };
    // ---- the first NB trips of the weight stream, then the x rows behind them (they are needed together)
    u32x4 wb[NB][R];
    uint32_t sb[NB][R];
#pragma unroll
    for (int j = 0; j < NB; ++j) issue(wb[j], sb[j], j);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PRENORM) {
        if (nwin > 1) {                                      // rows longer than a window: their sums of squares first (x from L2, read again below)
            float ss[MR];
#pragma unroll
            for (int m = 0; m < MR; ++m) ss[m] = 0.f;
            for (int v = threadIdx.x; v < nv; v += NT) {
#pragma unroll
                for (int m = 0; m < MR; ++m) {
                    float xv[8];
                    unpack8(*(const u32x4*)(a.x + (int64_t)min(m, M - 1) * a.ldx + v * 8), xv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) ss[m] += xv[e] * xv[e];
                }
            }
            finish_norm(ss);
        }
    }
    stage_load(0);
    if constexpr (PRENORM) {
        if (nwin == 1) {
            float ss[MR];
#pragma unroll
            for (int m = 0; m < MR; ++m) {
                ss[m] = 0.f;
#pragma unroll
                for (int i = 0; i < XV; ++i) {
                    float xv[8];
                    unpack8(xr[m][i], xv);                   // (beyond K: zeros)
#pragma unroll
                    for (int e = 0; e < 8; ++e) ss[m] += xv[e] * xv[e];
                }
            }
            finish_norm(ss);
        }
    }
    stage_store(0);
    __syncthreads();
    // ---- the stream
    float acc[MR][R];
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[m][r] = 0.f;
    const int sw = (lane ^ (lane >> 2)) & 3;                 // this lane's x vector j sits at slot 4 (lane + 64 trip) + (j ^ sw)
    auto consume = [&](const u32x4 (&w)[R], const uint32_t (&s)[R], int t) {
        const int j = t % WT;                                // trip j of window t / WT
        const unsigned char* src = xs + (size_t)((t / WT) & 1) * MR * wk * 2
                                   + (size_t)(min(j * 2048, wk - 2048) + lane * 32) * 2;   // (a trip behind the end is all zeros: any staged x will do)
        uint32_t xv[MR][16];
#pragma unroll
        for (int m = 0; m < MR; ++m) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const u32x4 x4 = *(const u32x4*)(src + (size_t)m * wk * 2 + ((e ^ sw) << 4));
                xv[m][4 * e] = x4.x; xv[m][4 * e + 1] = x4.y; xv[m][4 * e + 2] = x4.z; xv[m][4 * e + 3] = x4.w;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t wq[4] = {w[r].x, w[r].y, w[r].z, w[r].w};
            const float sc = e8m0_to_f32(s[r]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                uint32_t p[4];
                e2m1x8_to_bf16(wq[e], sc, p);
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int m = 0; m < MR; ++m)
                        acc[m][r] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(mm_bf16x2, p[b]), __builtin_bit_cast(mm_bf16x2, xv[m][4 * e + b]), acc[m][r], false);
            }
        }
    };
    for (int t0 = 0; t0 < ntrip; t0 += NB) {
#pragma unroll
        for (int jj = 0; jj < NB; ++jj) {
            const int t = t0 + jj;                           // (uniform over the workgroup: every wave runs the same trips)
            if (t < ntrip) {
                const int win = t / WT;
                if (t % WT == 0 && win + 1 < nwin) {         // the NEXT window lands while this one is consumed
                    stage_load(win + 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
                consume(wb[jj], sb[jj], t);
                // (keeps "consume trip t, then refill its registers": without the pin the sums sink below the loads and the ring is renamed)
#pragma unroll
                for (int m = 0; m < MR; ++m) asm volatile("" : "+v"(acc[m][0]), "+v"(acc[m][1]), "+v"(acc[m][2]), "+v"(acc[m][3]) : : "memory");
                __builtin_amdgcn_sched_barrier(0);
                issue(wb[jj], sb[jj], t + NB);
                __builtin_amdgcn_sched_barrier(0);
                if (t % WT == WT - 1 && win + 1 < nwin) {    // into the OTHER buffer: everyone left it at the barrier before this window
                    stage_store(win + 1);
                    __syncthreads();
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[m][r] = wave_sum(acc[m][r]);
    if (!live) return;
    if constexpr (MODE == 0) {                               // lane (m * R + r) finishes output (m, rows[r])
        if (lane < MR * R) {
            const int m = lane / R, r = lane % R, n = rows[0] + r;
            if (m < M && n < a.N) {
                float v = 0.f;
#pragma unroll
                for (int mm = 0; mm < MR; ++mm)
#pragma unroll
                    for (int rr = 0; rr < R; ++rr)
                        if (mm == m && rr == r) v = acc[mm][rr];
                plain_store(a, m, n, v);
            }
        }
    } else {
        if (lane >= M) return;                               // lane m finishes the unit's outputs of row m
        float v4[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float t = 0.f;
#pragma unroll
            for (int mm = 0; mm < MR; ++mm)
                if (mm == lane) t = acc[mm][r];
            v4[r] = round_bf(t);                             // what the unfused GEMV stores
        }
        fused_store<MODE>(a, rows, lane, v4);
    }
}

// ------------------------------------------------------------------------------------------------ 5 .. 16 rows: MFMA
// As gemv_w8_mfma_kernel: a wave owns four units = 16 weight rows as the A operand of v_mfma_f32_16x16x32_bf16 (lane fr = lane & 15 holds
// row fr), the x rows are the B operand (row m = fr).  A lane's 16-byte load is row fr, columns k + 32 fq .. + 31 (fq = lane >> 4), one scale
// group: widened it is the A fragment of FOUR MFMAs, whose B fragments are the 64 bytes of x row m at the same columns in LDS -- which 32
// columns an MFMA sums is free as long as A and B agree, so no re-layout is needed.  A step = 128 columns, a trip = two steps (128
// contiguous bytes per weight row), NB trips in the ring.  The x rows pass through two LDS windows of 1024 columns = four trips (rows 2064
// bytes apart).  ks = 4 (few weight rows): the four waves of a workgroup share one group of 16 rows, each takes a quarter of every window,
// the partial tiles meet in LDS in a fixed order; ks depends on the number of units only, so a fused kernel and the sequence it replaces
// see the same sums.  D: lane (m = fr, unit fq) ends with the four outputs of one unit for one x row.
constexpr int WKM = 1024;
constexpr int XROW = WKM * 2 + 16;

template <int MRT, int MODE, bool PRENORM>
__global__ __launch_bounds__(NT) void gemv_w4_mfma_kernel(WqArgs a) {
    constexpr int NB = 4;
    constexpr int XV = MRT / 2;                              // 16-byte x vectors per thread and window: MRT rows x 128 vectors over 256 threads
    extern __shared__ __attribute__((aligned(16))) unsigned char xs[];          // [2][M][XROW]
    __shared__ f32x4 part[NT / 64][64];
    __shared__ float red[MRT][NT / 64];
    __shared__ float rstd_s[MRT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int ks = a.ks;
    const int group = blockIdx.x * ((NT / 64) / ks) + wave / ks, kslice = wave % ks;
    const int K = a.K, M = a.M;
    const int nwin = (K + WKM - 1) / WKM, nv = K >> 3;
    const int tpw = 4 / ks;                                  // trips of this wave per window (8 / ks steps)
    const int ntrip = nwin * tpw;
    int rows[4];
    unit_rows<MODE>(a, group * 4 + (fr >> 2), rows);
    const bool alive = unit_live<MODE>(a, rows) && rows[fr & 3] < a.N;
    const uint32_t wo = (uint32_t)min(rows[fr & 3], a.N - 1) * (uint32_t)a.ldw;
    const uint32_t so = (uint32_t)min(rows[fr & 3], a.N - 1) * (uint32_t)a.lds;
    const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)a.W, 0, (uint32_t)((uint64_t)(a.N - 1) * a.ldw + (uint64_t)(K >> 1)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsS = __builtin_amdgcn_make_buffer_rsrc((void*)a.S, 0, (uint32_t)((uint64_t)(a.N - 1) * a.lds + (uint64_t)(K >> 5)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (uint32_t)((uint64_t)(M - 1) * a.ldx * 2 + (uint64_t)K * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsN = __builtin_amdgcn_make_buffer_rsrc((void*)(PRENORM ? a.norm_w : a.x), 0, (uint32_t)K * 2u, 0x00020000);
    const int sm = threadIdx.x >> 7, sv = threadIdx.x & 127;   // staging: vector sv of window row sm + 2 i
    u32x4 xr[XV], nr;
    auto stage_load = [&](int w) {
        const int v = w * (WKM / 8) + sv;
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            const int m = sm + 2 * i;
            const uint32_t sk = (m < M && v < nv) ? 0u : OOB;
            xr[i] = __builtin_amdgcn_raw_buffer_load_b128(rsX, ((uint32_t)min(m, M - 1) * (uint32_t)a.ldx * 2u + (uint32_t)v * 16u) | sk, 0, 0);
        }
        if constexpr (PRENORM) nr = __builtin_amdgcn_raw_buffer_load_b128(rsN, ((uint32_t)v * 16u) | (v < nv ? 0u : OOB), 0, 0);
    };
    auto stage_store = [&](int w) {
        unsigned char* dst = xs + (size_t)(w & 1) * M * XROW + sv * 16;
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            const int m = sm + 2 * i;
            if (m < M) {
                u32x4 out = xr[i];
                if constexpr (PRENORM) {
                    float xv[8], nw[8];
                    unpack8(xr[i], xv);
                    unpack8(nr, nw);
                    const float rs = rstd_s[m];
#pragma unroll
                    for (int e = 0; e < 8; ++e) xv[e] = nw[e] * round_bf(xv[e] * rs);
                    out = pack8(xv);
                }
                *(u32x4*)(dst + (size_t)m * XROW) = out;
            }
        }
    };
    auto issue = [&](u32x4 (&w)[2], uint32_t (&s)[2], int t) {   // trip t of this wave: window t / tpw, steps 2 (kslice * tpw + t % tpw) + i
        const int k0 = (t / tpw) * WKM + (kslice * tpw + (t % tpw)) * 256 + fq * 32;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int k = k0 + i * 128;
            const uint32_t sk = (alive && t < ntrip && k < K) ? 0u : OOB;
            w[i] = __builtin_amdgcn_raw_buffer_load_b128(rsW, (wo + (uint32_t)(k >> 1)) | sk, 0, 2);
            s[i] = __builtin_amdgcn_raw_buffer_load_b8(rsS, (so + (uint32_t)(k >> 5)) | sk, 0, 2);
        }
    };
    u32x4 wb[NB][2];
    uint32_t sb[NB][2];
#pragma unroll
    for (int j = 0; j < NB; ++j) issue(wb[j], sb[j], j);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PRENORM) {                                 // rmsnorm_fwd_kernel's sums of squares (thread t: vectors t + 256 i in order; block_sum<256>), x from L2
        float ss[MRT];
#pragma unroll
        for (int m = 0; m < MRT; ++m) ss[m] = 0.f;
        for (int v = threadIdx.x; v < nv; v += NT) {
#pragma unroll
            for (int m = 0; m < MRT; ++m) {
                if (m < M) {
                    float xv[8];
                    unpack8(*(const u32x4*)(a.x + (int64_t)m * a.ldx + v * 8), xv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) ss[m] += xv[e] * xv[e];
                }
            }
        }
#pragma unroll
        for (int m = 0; m < MRT; ++m) {
            const float w = wave_sum(ss[m]);
            if (lane == 0) red[m][wave] = w;
        }
        __syncthreads();
        if (threadIdx.x < MRT) {
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < NT / 64; ++i) t += red[threadIdx.x][i];
            rstd_s[threadIdx.x] = rsqrtf(t / (float)K + a.eps);
        }
        __syncthreads();
    }
    stage_load(0);
    stage_store(0);
    __syncthreads();
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const int xm = min(fr, M - 1);                           // (columns of D beyond M are never read)
    auto consume = [&](const u32x4 (&w)[2], const uint32_t (&s)[2], int t) {
        const unsigned char* src = xs + (size_t)((t / tpw) & 1) * M * XROW + (size_t)xm * XROW
                                   + ((kslice * tpw + (t % tpw)) * 256 + fq * 32) * 2;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint32_t wq[4] = {w[i].x, w[i].y, w[i].z, w[i].w};
            const float sc = e8m0_to_f32(s[i]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const u32x4 xf = *(const u32x4*)(src + i * 256 + e * 16);
                uint32_t p[4];
                e2m1x8_to_bf16(wq[e], sc, p);
                const u32x4 af = {p[0], p[1], p[2], p[3]};
                if (e & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af), __builtin_bit_cast(bf16x8, xf), acc1, 0, 0, 0);
                else acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af), __builtin_bit_cast(bf16x8, xf), acc0, 0, 0, 0);
            }
        }
    };
    for (int t0 = 0; t0 < ntrip; t0 += NB) {
#pragma unroll
        for (int jj = 0; jj < NB; ++jj) {
            const int t = t0 + jj;                           // (uniform over the workgroup: every wave runs the same trips)
            if (t < ntrip) {
                const int win = t / tpw;
                if (t % tpw == 0 && win + 1 < nwin) {        // the NEXT window lands while this one is consumed
                    stage_load(win + 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
                consume(wb[jj], sb[jj], t);
                asm volatile("" : "+v"(acc0), "+v"(acc1) : : "memory");
                __builtin_amdgcn_sched_barrier(0);
                issue(wb[jj], sb[jj], t + NB);
                __builtin_amdgcn_sched_barrier(0);
                if (t % tpw == tpw - 1 && win + 1 < nwin) {  // into the OTHER buffer: everyone left it at the barrier before this window
                    stage_store(win + 1);
                    __syncthreads();
                }
            }
        }
    }
    f32x4 acc = acc0 + acc1;
    if (ks > 1) {
        part[wave][lane] = acc;
        __syncthreads();
        if (kslice != 0) return;
        acc = part[wave][lane];
        for (int q = 1; q < ks; ++q) acc += part[wave + q][lane];
    }
    // lane (m = fr, unit fq of the group): the four outputs of that unit for x row m
    const int m = fr;
    int ro[4];
    unit_rows<MODE>(a, group * 4 + fq, ro);
    if (m >= M || !unit_live<MODE>(a, ro)) return;
    if constexpr (MODE == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = ro[0] + r;
            if (n < a.N) plain_store(a, m, n, acc[r]);
        }
    } else {
        float v4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v4[r] = round_bf(acc[r]);
        fused_store<MODE>(a, ro, m, v4);
    }
}

// ------------------------------------------------------------------------------------------------ Wq, S -> bf16 (every route without a w4 kernel)
// a thread: 16 bytes of Wq and their scale byte -> 64 bytes of bf16, exact (no rounding: every Wd is a bf16 value)
__global__ __launch_bounds__(NT) void dequant_w4_kernel(const uint8_t* __restrict__ q, int64_t ldq, const uint8_t* __restrict__ S, int64_t lds,
                                                        uint16_t* __restrict__ out, int64_t ldo, int64_t N, int kg) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= N * kg) return;
    const int64_t n = idx / kg;
    const int c = (int)(idx % kg);
    const u32x4 w = *(const u32x4*)(q + n * ldq + (int64_t)c * 16);
    const float sc = e8m0_to_f32(S[n * lds + c]);
    const uint32_t wq[4] = {w.x, w.y, w.z, w.w};
    uint16_t* dst = out + n * ldo + (int64_t)c * 32;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint32_t p[4];
        e2m1x8_to_bf16(wq[e], sc, p);
        *(u32x4*)(dst + 8 * e) = u32x4{p[0], p[1], p[2], p[3]};
    }
}

constexpr int LDS_OPT_IN = 80 * 1024;                        // both forms hold at most 66 KiB of x windows next to a few KiB of static LDS

template <int MODE>
int launch_w4(WqArgs& a, int64_t units, bool prenorm, hipStream_t s) {
#define W4_LAUNCH(KERNEL, GRID, LDS) do { static std::atomic<uint64_t> ok{0};                                                      \
        if (mm_ensure_dynamic_lds((const void*)KERNEL, LDS_OPT_IN, ok) != MM355_OK) return MM355_ELAUNCH;                            \
        hipLaunchKernelGGL(KERNEL, dim3(GRID), dim3(NT), LDS, s, a); } while (0)
    if (a.M <= 4) {
        const unsigned grid = (unsigned)((units + NT / 64 - 1) / (NT / 64));
        const int mr = a.M == 1 ? 1 : (a.M == 2 ? 2 : 4);
        const int wt = mr == 4 ? 2 : 4, ntrip = (a.K + 2047) >> 11;
        const int lds = (ntrip > wt ? 2 : 1) * mr * (ntrip < wt ? ntrip : wt) * 2048 * 2;        // <= 64 KiB
#define W4_V(MR) do { if (prenorm) { if constexpr (MODE != 0) W4_LAUNCH((gemv_w4_valu_kernel<MR, MODE, true>), grid, lds); }         \
                      else W4_LAUNCH((gemv_w4_valu_kernel<MR, MODE, false>), grid, lds); } while (0)
        if (mr == 1) W4_V(1);
        else if (mr == 2) W4_V(2);
        else W4_V(4);
#undef W4_V
        return mm_launch_status();
    }
    const int64_t groups = (units + 3) / 4;                  // 16 weight rows each
    a.ks = groups < 1024 ? 4 : 1;
    const unsigned grid = (unsigned)((groups + (NT / 64) / a.ks - 1) / ((NT / 64) / a.ks));
    const int lds = 2 * a.M * XROW;
#define W4_M(MRT) do { if (prenorm) { if constexpr (MODE != 0) W4_LAUNCH((gemv_w4_mfma_kernel<MRT, MODE, true>), grid, lds); }      \
                       else W4_LAUNCH((gemv_w4_mfma_kernel<MRT, MODE, false>), grid, lds); } while (0)
    if (a.M <= 8) W4_M(8);
    else W4_M(16);
#undef W4_M
#undef W4_LAUNCH
    return mm_launch_status();
}

// x rows, weight bytes, scale bytes and every fused operand in the form the kernels address them (32-bit byte offsets through buffer
// descriptors)
int w4_check(const void* x, int64_t ldx, const void* Wq, int64_t ldw, const void* S, int64_t lds, int fmt, int64_t M, int64_t N, int64_t K) {
    if (!x || !Wq || !S || M <= 0 || N <= 0 || K <= 0) return MM355_EINVAL;
    if (fmt != MM355_W4_MXFP4) return MM355_EINVAL;
    if ((K & 31) || (ldx & 7) || (ldw & 15) || ldw < K / 2 || lds < K / 32 || !mm_aligned16(x) || !mm_aligned16(Wq)) return MM355_EINVAL;
    if (N > 0x7fffffff || K > 0x7fffffff) return MM355_EINVAL;
    if (M > 16) return MM355_EUNSUPPORTED;                   // more rows: mm355_dequant_w4_bf16 + mm355_gemm_bf16
    if ((uint64_t)N * ldw >= 0xf0000000ull || (uint64_t)N * lds >= 0xf0000000ull || (uint64_t)(M - 1) * ldx * 2 + K * 2 >= 0xf0000000ull)
        return MM355_EUNSUPPORTED;
    return MM355_OK;
}

}  // namespace

extern "C" int mm355_gemv_w4(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes, int fmt,
                             void* y, int64_t ldy, int64_t M, int64_t N, int64_t K, const mm355_bf16* bias, const mm355_bf16* residual,
                             int64_t ldr, uint32_t flags, void* stream) {
    (void)hipGetLastError();   // drop any stale, unrelated runtime status before we launch
    if (!y) return MM355_EINVAL;
    if ((flags & MM355_GEMM_BIAS) && !bias) return MM355_EINVAL;
    if ((flags & MM355_GEMM_RESIDUAL) && !residual) return MM355_EINVAL;
    if ((flags & MM355_GEMM_GELU_ERF) && (flags & MM355_GEMM_GELU_TANH)) return MM355_EINVAL;
    const int rc = w4_check(x, ldx, Wq, ldw_bytes, S, lds_bytes, fmt, M, N, K);
    if (rc != MM355_OK) return rc;
    if (flags & MM355_GEMM_ACCUMULATE) return MM355_EUNSUPPORTED;
    WqArgs a = {};
    a.x = x; a.ldx = ldx; a.W = Wq; a.ldw = ldw_bytes; a.S = S; a.lds = lds_bytes; a.M = (int)M; a.N = (int)N; a.K = (int)K;
    a.y = y; a.ldy = ldy; a.bias = bias; a.res = residual; a.ldr = ldr; a.flags = flags;
    return launch_w4<0>(a, (N + 3) / 4, false, (hipStream_t)stream);
}

extern "C" int mm355_gemv_swiglu_w4(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes,
                                    int fmt, mm355_bf16* act, int64_t ld_act, int64_t M, int64_t I, int64_t K, const mm355_bf16* norm_w,
                                    float eps, void* stream) {
    (void)hipGetLastError();
    if (!act || I <= 0) return MM355_EINVAL;
    if (I > 0x3fffffff) return MM355_EINVAL;
    const int rc = w4_check(x, ldx, Wq, ldw_bytes, S, lds_bytes, fmt, M, 2 * I, K);
    if (rc != MM355_OK) return rc;
    if (I & 1) return MM355_EUNSUPPORTED;
    if ((ld_act & 1) || (((uintptr_t)act) & 3u)) return MM355_EINVAL;
    if (norm_w && !mm_aligned16(norm_w)) return MM355_EINVAL;
    if (norm_w && M > 4 && M * (((K + 31) & ~(int64_t)31) + 8) * 2 > 140 * 1024) return MM355_EUNSUPPORTED;   // as the bf16 form documents
    WqArgs a = {};
    a.x = x; a.ldx = ldx; a.W = Wq; a.ldw = ldw_bytes; a.S = S; a.lds = lds_bytes; a.M = (int)M; a.N = (int)(2 * I); a.K = (int)K;
    a.norm_w = norm_w; a.eps = eps; a.out = act; a.ld_out = ld_act; a.I = (int)I;
    return launch_w4<1>(a, I / 2, norm_w != nullptr, (hipStream_t)stream);
}

extern "C" int mm355_gemv_rope_append_w4(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S,
                                         int64_t lds_bytes, int fmt, mm355_bf16* qkv, int64_t ld_qkv, int64_t M, int64_t Hq, int64_t Hkv,
                                         int64_t d, int64_t K, const mm355_bf16* norm_w, float eps, const mm355_bf16* cos_t,
                                         const mm355_bf16* sin_t, const int32_t* positions, mm355_bf16* k_cache, mm355_bf16* v_cache,
                                         int64_t ld_kv, int64_t batch_stride_kv, void* stream) {
    (void)hipGetLastError();
    if (!qkv || !cos_t || !sin_t || !positions || !k_cache || !v_cache || Hq <= 0 || Hkv <= 0 || d <= 0) return MM355_EINVAL;
    const int64_t N = (Hq + 2 * Hkv) * d;
    const int rc = w4_check(x, ldx, Wq, ldw_bytes, S, lds_bytes, fmt, M, N, K);
    if (rc != MM355_OK) return rc;
    if (d & 3) return MM355_EUNSUPPORTED;                    // rotation partners in pairs: d / 2 even
    if ((ld_qkv & 1) || (ld_kv & 3) || (batch_stride_kv & 3) || (((uintptr_t)qkv) & 3u) || (((uintptr_t)k_cache) & 7u) || (((uintptr_t)v_cache) & 7u))
        return MM355_EINVAL;
    if (norm_w && !mm_aligned16(norm_w)) return MM355_EINVAL;
    if (norm_w && M > 4 && M * (((K + 31) & ~(int64_t)31) + 8) * 2 > 140 * 1024) return MM355_EUNSUPPORTED;
    WqArgs a = {};
    a.x = x; a.ldx = ldx; a.W = Wq; a.ldw = ldw_bytes; a.S = S; a.lds = lds_bytes; a.M = (int)M; a.N = (int)N; a.K = (int)K;
    a.norm_w = norm_w; a.eps = eps; a.out = qkv; a.ld_out = ld_qkv; a.Hq = (int)Hq; a.Hkv = (int)Hkv; a.d = (int)d;
    a.cos_t = cos_t; a.sin_t = sin_t; a.positions = positions; a.kc = k_cache; a.vc = v_cache; a.ld_kv = ld_kv; a.bs_kv = batch_stride_kv;
    return launch_w4<2>(a, N / 4, norm_w != nullptr, (hipStream_t)stream);
}

extern "C" int mm355_dequant_w4_bf16(const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes, int fmt, mm355_bf16* out,
                                     int64_t ld_out, int64_t N, int64_t K, void* stream) {
    (void)hipGetLastError();
    if (!Wq || !S || !out || N <= 0 || K <= 0) return MM355_EINVAL;
    if (fmt != MM355_W4_MXFP4) return MM355_EINVAL;
    if ((K & 31) || (ldw_bytes & 15) || ldw_bytes < K / 2 || lds_bytes < K / 32 || (ld_out & 7) || ld_out < K || !mm_aligned16(Wq) || !mm_aligned16(out))
        return MM355_EINVAL;
    const int64_t kg = K / 32, total = N * kg;
    if (K > 0x7fffffff || (total + NT - 1) / NT > 0x7fffffff) return MM355_EINVAL;
    hipLaunchKernelGGL(dequant_w4_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, Wq, ldw_bytes, S, lds_bytes,
                       out, ld_out, N, (int)kg);
    return mm_launch_status();
}
