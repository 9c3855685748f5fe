// The 8-wave backward-weight kernels: pw_wgrad_bf16_kernel, pw_wgrad_bf16_fast_kernel, pw_wgrad_bf16_wide_kernel.
#pragma once
#include "pointwise_bf16_common.h"

// Backward-weight, bf16: contraction index is t; both operands are read as 8 consecutive t
// (two float4), transformed, rounded and written as one 16-byte chunk of a [row][t] image.
template <int GM_, int XM_, bool TV>
__global__ __launch_bounds__(256) void pw_wgrad_bf16_kernel(WgParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char As[2][128 * 128];   // [m][t] bf16
    __shared__ __attribute__((aligned(16))) unsigned char Bs[2][128 * 128];   // [k][t] bf16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int s, mt, ktile;
    wg_work(p, s, mt, ktile);
    const int m0 = mt * PW_BM, n0 = ktile * PW_BN;
    const int M = p.M, K = p.K, T = p.T;
    const int g_mode = PW_MODE(GM_, p.g_mode), x_mode = PW_MODE(XM_, p.x_mode);

    // 128 rows x 8 chunks per operand = 1024 pieces, 4 per thread: piece = tid + 256*i (row = piece>>3, chunk = piece&7)
    float ga[4], gb[4], gc[4], xa[4], xb[4];
    bool mv[4], kv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (tid + 256 * i) >> 3;
        const int m = m0 + row, k = n0 + row;
        mv[i] = m < M; kv[i] = k < K;
        ga[i] = (g_mode != PW_X_NONE) ? ldc(p.ga, m, mv[i], 1.f) : 1.f;
        gb[i] = (g_mode != PW_X_NONE) ? ldc(p.gb, m, mv[i], 0.f) : 0.f;
        gc[i] = (g_mode == PW_X_AFFINE2) ? ldc(p.gc, m, mv[i], 0.f) : 0.f;
        xa[i] = (x_mode != PW_X_NONE) ? ldc(p.xa, k, kv[i], 1.f) : 1.f;
        xb[i] = (x_mode != PW_X_NONE) ? ldc(p.xb, k, kv[i], 0.f) : 0.f;
    }

    f32x4 ra[4][2], ra2[4][2], rb[4][2];
    auto load_tiles = [&](int b, int t0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = tid + 256 * i;
            const int row = piece >> 3, ch = piece & 7;
            const int m = m0 + row, k = n0 + row, t = t0 + ch * 8;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                ra[i][h] = ld4<TV>(p.G, ((size_t)b * M + m) * T, t + 4 * h, T, mv[i]);
                if (g_mode == PW_X_AFFINE2) ra2[i][h] = ld4<TV>(p.G2, ((size_t)b * M + m) * T, t + 4 * h, T, mv[i]);
                rb[i][h] = ld4<TV>(p.X, ((size_t)b * K + k) * T, t + 4 * h, T, kv[i]);
            }
        }
    };
    auto store_tiles = [&](int buf, int t0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = tid + 256 * i;
            const int row = piece >> 3, ch = piece & 7;
            const int t = t0 + ch * 8;
            float va[8], vb[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool tv = t + e < T;
                va[e] = (mv[i] && tv) ? pw_x_transform(g_mode, ra[i][e >> 2][e & 3], ra2[i][e >> 2][e & 3], ga[i], gb[i], gc[i]) : 0.f;
                vb[e] = (kv[i] && tv) ? pw_x_transform(x_mode, rb[i][e >> 2][e & 3], 0.f, xa[i], xb[i], 0.f) : 0.f;
            }
            uint4 oa, ob;
            oa.x = pack_bf16(va[0], va[1]); oa.y = pack_bf16(va[2], va[3]); oa.z = pack_bf16(va[4], va[5]); oa.w = pack_bf16(va[6], va[7]);
            ob.x = pack_bf16(vb[0], vb[1]); ob.y = pack_bf16(vb[2], vb[3]); ob.z = pack_bf16(vb[4], vb[5]); ob.w = pack_bf16(vb[6], vb[7]);
            *reinterpret_cast<uint4*>(&As[buf][bf_off(row, ch)]) = oa;
            *reinterpret_cast<uint4*>(&Bs[buf][bf_off(row, ch)]) = ob;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nt = (T + BF_BK - 1) / BF_BK;
    const WgSpan sp = wg_span(p, s, nt);
    const int nsteps = sp.nb * sp.ntl, b_lo = sp.b_lo;
    const int lr = lane & 31, lh = lane >> 5;
    if (nsteps > 0) {
        load_tiles(b_lo, sp.t_first * BF_BK);
        store_tiles(0, sp.t_first * BF_BK);
    }
    __syncthreads();
    for (int st = 0; st < nsteps; ++st) {
        const int cur = st & 1;
        const int nxt = st + 1;
        const int nb = b_lo + nxt / sp.ntl, ntt = (sp.t_first + nxt % sp.ntl) * BF_BK;
        if (nxt < nsteps) load_tiles(nb, ntt);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < BF_BK / 16; ++ks) {
            const int ch = ks * 2 + lh;
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(&As[cur][bf_off(wm * 64 + lr, ch)]);
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(&As[cur][bf_off(wm * 64 + 32 + lr, ch)]);
            const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(&Bs[cur][bf_off(wn * 64 + lr, ch)]);
            const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(&Bs[cur][bf_off(wn * 64 + 32 + lr, ch)]);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
        }
        // ... and first USED after it: without this fence hipcc hoists the staging arithmetic (and the
        // vmcnt wait it needs) above the MFMAs, which exposes the whole memory latency every k-step.
        asm volatile("" : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[1][0]), "+a"(acc[1][1]));   // accumulators stay in AGPRs
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            asm volatile("" : "+v"(ra[i][0]), "+v"(ra[i][1]), "+v"(rb[i][0]), "+v"(rb[i][1]));
            if (g_mode == PW_X_AFFINE2) asm volatile("" : "+v"(ra2[i][0]), "+v"(ra2[i][1]));
        }
        __builtin_amdgcn_sched_barrier(0);
        if (nxt < nsteps) store_tiles(cur ^ 1, ntt);
        __syncthreads();
    }
    const int col = lane & 31, half = lane >> 5;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const int k = n0 + wn * 64 + j * 32 + col;
                if (m < M && k < K) p.partial[((size_t)s * M + m) * K + k] = acc[i][j][r];
            }
}


// Fast path of the backward-weight kernel for T % 64 == 0: buffer loads with per-batch descriptors
// (rows past M / K read as zero in hardware), per-lane offsets computed once.
template <int GM, int XM, bool TAIL, bool TAPS = false, int IO = 0>
__global__ __launch_bounds__(256) void pw_wgrad_bf16_fast_kernel(WgParams p) {
    static_assert(!TAPS || (GM == PW_X_NONE && XM == PW_X_NONE), "tap-addressed X has no prologues");
    static_assert(!(IO != 0 && TAPS), "16-bit activation storage: plain operands only");
    // operands stored as bf16 [B][rows][pw_pitch16(T, p.B)]: the 8 consecutive t of a piece are ONE 16-byte load
    constexpr bool GB = (IO & WG_IO_G) != 0, G2B = (IO & WG_IO_G2) != 0, XB = (IO & WG_IO_X) != 0;
    __shared__ __attribute__((aligned(16))) unsigned char As[2][128 * 128];   // [m][t] bf16
    __shared__ __attribute__((aligned(16))) unsigned char Bs[2][128 * 128];   // [k][t] bf16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int s, mt, ktile;
    wg_work(p, s, mt, ktile);
    const int m0 = mt * PW_BM, n0 = ktile * PW_BN;
    const int M = p.M, K = p.K, T = p.T;

    float ga[4], gb[4], gc[4], xa[4], xb[4];
    int voG[4], voX[4], ldsO[4], voG16[4], voX16[4];
    const int P16 = pw_pitch16(T, p.B);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int piece = tid + 256 * i;
        const int row = piece >> 3, ch = piece & 7;
        const int m = m0 + row, k = n0 + row;
        const bool mv = m < M, kv = k < K;
        voG16[i] = (m * P16 + ch * 8) * 2;
        voX16[i] = (k * P16 + ch * 8) * 2;
        ga[i] = (GM != PW_X_NONE) ? p.ga[mv ? m : 0] : 1.f;
        gb[i] = (GM != PW_X_NONE) ? p.gb[mv ? m : 0] : 0.f;
        gc[i] = (GM == PW_X_AFFINE2) ? p.gc[mv ? m : 0] : 0.f;
        xa[i] = (XM != PW_X_NONE) ? p.xa[kv ? k : 0] : 1.f;
        xb[i] = (XM != PW_X_NONE) ? p.xb[kv ? k : 0] : 0.f;
        voG[i] = (m * T + ch * 8) * 4;
        voX[i] = (k * T + ch * 8) * 4;
        if constexpr (TAPS) {                  // column k of dW = tap * cx + c: row c of the padded X, shifted (see WgParams)
            const int tap = kv ? k / p.cx : 0;
            voG[i] = (m * p.Tg + p.g_off + ch * 8) * 4;
            voX[i] = kv ? ((k - tap * p.cx) * p.Tx + pw_tap_shift(p.shifts, tap) + ch * 8) * 4 : 0x7fffff00;   // past the descriptor: zero
        }
        ldsO[i] = bf_off(row, ch);
    }
    const int Tg = TAPS ? p.Tg : T, Kx = TAPS ? p.cx : K, Tx = TAPS ? p.Tx : T;

    u32x4 ra[4][GB ? 1 : 2], ra2[4][G2B ? 1 : 2], rb[4][XB ? 1 : 2];
    auto load_tiles = [&](int b, int t0) {
        const __amdgpu_buffer_rsrc_t rG = GB ? make_rsrc(reinterpret_cast<const u16*>(p.G) + (size_t)b * M * P16, (unsigned)M * P16 * 2u)
                                             : make_rsrc(p.G + (size_t)b * M * Tg, (unsigned)M * Tg * 4u);
        const float* g2p = GM == PW_X_AFFINE2 ? p.G2 : p.G;
        const __amdgpu_buffer_rsrc_t rG2 = (GM == PW_X_AFFINE2 ? G2B : GB)
                                               ? make_rsrc(reinterpret_cast<const u16*>(g2p) + (size_t)b * M * P16, (unsigned)M * P16 * 2u)
                                               : make_rsrc(g2p + (size_t)b * M * Tg, (unsigned)M * Tg * 4u);
        const __amdgpu_buffer_rsrc_t rX = XB ? make_rsrc(reinterpret_cast<const u16*>(p.X) + (size_t)b * Kx * P16, (unsigned)Kx * P16 * 2u)
                                             : make_rsrc(p.X + (size_t)b * Kx * Tx, (unsigned)Kx * Tx * 4u);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (GB) ra[i][0] = __builtin_amdgcn_raw_buffer_load_b128(rG, voG16[i], t0 * 2, 0);
            if constexpr (GM == PW_X_AFFINE2 && G2B) ra2[i][0] = __builtin_amdgcn_raw_buffer_load_b128(rG2, voG16[i], t0 * 2, 0);
            if constexpr (XB) rb[i][0] = __builtin_amdgcn_raw_buffer_load_b128(rX, voX16[i], t0 * 2, 0);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if constexpr (!GB) ra[i][h] = __builtin_amdgcn_raw_buffer_load_b128(rG, voG[i] + 16 * h, t0 * 4, 0);
                if constexpr (GM == PW_X_AFFINE2 && !G2B) ra2[i][h] = __builtin_amdgcn_raw_buffer_load_b128(rG2, voG[i] + 16 * h, t0 * 4, 0);
                if constexpr (!XB) rb[i][h] = __builtin_amdgcn_raw_buffer_load_b128(rX, voX[i] + 16 * h, t0 * 4, 0);
            }
        }
    };
    auto store_tiles = [&](int buf, int t0) {
        const bool tail = TAIL && (t0 + BF_BK > T);        // contraction index past T must contribute zero
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float va[8], vb[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float gv;
                    if constexpr (GB) gv = pw_bf16_at(ra[i][0], 4 * h + e);
                    else gv = __builtin_bit_cast(f32x4, ra[i][h])[e];
                    if constexpr (GM == PW_X_AFFINE2) {
                        float g2;
                        if constexpr (G2B) g2 = pw_bf16_at(ra2[i][0], 4 * h + e);
                        else g2 = __builtin_bit_cast(f32x4, ra2[i][h])[e];
                        gv = fmaf(gv, ga[i], fmaf(g2, gb[i], gc[i]));
                    } else if constexpr (GM == PW_X_AFFINE_RELU6) gv = relu6f(fmaf(gv, ga[i], gb[i]));
                    float xv;
                    if constexpr (XB) xv = pw_bf16_at(rb[i][0], 4 * h + e);
                    else xv = __builtin_bit_cast(f32x4, rb[i][h])[e];
                    if constexpr (XM == PW_X_AFFINE_RELU6) xv = relu6f(fmaf(xv, xa[i], xb[i]));
                    va[4 * h + e] = gv;
                    vb[4 * h + e] = xv;
                }
            }
            // rows past M / K were read as zero, but an affine transform of zero is not zero: kill them
            if constexpr (GM != PW_X_NONE) { if (voG[i] >= M * T * 4) {
#pragma unroll
                for (int e = 0; e < 8; ++e) va[e] = 0.f; } }
            if constexpr (XM != PW_X_NONE) { if (voX[i] >= K * T * 4) {
#pragma unroll
                for (int e = 0; e < 8; ++e) vb[e] = 0.f; } }
            if constexpr (TAIL) if (tail) {
                const int tb = t0 + (((tid + 256 * i) & 7) << 3);
#pragma unroll
                for (int e = 0; e < 8; ++e) { if (tb + e >= T) { va[e] = 0.f; vb[e] = 0.f; } }
            }
            u32x4 oa, ob;
            oa[0] = pack_bf16(va[0], va[1]); oa[1] = pack_bf16(va[2], va[3]); oa[2] = pack_bf16(va[4], va[5]); oa[3] = pack_bf16(va[6], va[7]);
            ob[0] = pack_bf16(vb[0], vb[1]); ob[1] = pack_bf16(vb[2], vb[3]); ob[2] = pack_bf16(vb[4], vb[5]); ob[3] = pack_bf16(vb[6], vb[7]);
            *reinterpret_cast<u32x4*>(&As[buf][ldsO[i]]) = oa;
            *reinterpret_cast<u32x4*>(&Bs[buf][ldsO[i]]) = ob;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nt = (T + BF_BK - 1) / BF_BK;
    const WgSpan sp = wg_span(p, s, nt);
    const int nsteps = sp.nb * sp.ntl, b_lo = sp.b_lo;
    const int lr = lane & 31, lh = lane >> 5;
    const int sw = (lr >> 1) & 7;
    const int rdA0 = (wm * 64 + lr) * 128, rdB0 = (wn * 64 + lr) * 128;
    if (nsteps > 0) {
        load_tiles(b_lo, sp.t_first * BF_BK);
        store_tiles(0, sp.t_first * BF_BK);
    }
    __syncthreads();
    for (int st = 0; st < nsteps; ++st) {
        const int cur = st & 1;
        const int nxt = st + 1;
        if (nxt < nsteps) load_tiles(b_lo + nxt / sp.ntl, (sp.t_first + nxt % sp.ntl) * BF_BK);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < BF_BK / 16; ++ks) {
            const int co = ((ks * 2 + lh) ^ sw) << 4;
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(&As[cur][rdA0 + co]);
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(&As[cur][rdA0 + 32 * 128 + co]);
            const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(&Bs[cur][rdB0 + co]);
            const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(&Bs[cur][rdB0 + 32 * 128 + co]);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
        }
        asm volatile("" : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[1][0]), "+a"(acc[1][1]));   // accumulators stay in AGPRs
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            asm volatile("" : "+v"(ra[i][0]), "+v"(rb[i][0]));
            if constexpr (!GB) asm volatile("" : "+v"(ra[i][1]));
            if constexpr (!XB) asm volatile("" : "+v"(rb[i][1]));
            if constexpr (GM == PW_X_AFFINE2) {
                asm volatile("" : "+v"(ra2[i][0]));
                if constexpr (!G2B) asm volatile("" : "+v"(ra2[i][1]));
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (nxt < nsteps) store_tiles(cur ^ 1, (sp.t_first + nxt % sp.ntl) * BF_BK);
        __syncthreads();
    }
    const int col = lane & 31, half = lane >> 5;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const int k = n0 + wn * 64 + j * 32 + col;
                if (m < M && k < K) p.partial[((size_t)s * M + m) * K + k] = acc[i][j][r];
            }
}

// ---------------------------------------------------------------------------------------------
// Backward-weight with a 256-row tile on the PLAIN operand (act16 training combinations).  In the 128 x 128 kernel above every
// thread transforms 8 + 8 elements per piece of both operands -- BatchNorm-backward affine of two bf16 tensors on G, or
// BatchNorm + ReLU6 on X -- and each operand tile is transformed again by every workgroup along the other tile axis (4x at
// 512 channels): a timing-only build without transform / LDS stores (profiles/r02j_gemm_ablation.txt) takes the project gradient from 62 to 41 us, so the kernel is
// bound by VALU issue of the staging, not by the matrix pipe or memory.  Here the block tile is GR x XR = 128 x 256 or 256 x 128
// with the 128 rows on the TRANSFORMED operand: half the redundant transforms per MFMA, and a plain bf16 operand is copied to
// LDS as loaded (no unpack / repack).  8 waves of 64 x 64, one workgroup per CU, same LDS images and fragment reads.
template <int GM, int XM, bool TAIL, int IO, int GR, int XR, int NST>
__global__ __launch_bounds__(512) void pw_wgrad_bf16_wide_kernel(WgParams p) {
    static_assert(GR % 64 == 0 && XR % 64 == 0 && (GR / 64) * (XR / 64) == 8, "8 waves of 64 x 64");
    constexpr bool GB = (IO & WG_IO_G) != 0, G2B = (IO & WG_IO_G2) != 0, XB = (IO & WG_IO_X) != 0;
    constexpr int NG = GR / 64, NX = XR / 64;               // 16-byte LDS pieces per thread and operand
    constexpr bool GCOPY = GB && GM == PW_X_NONE, XCOPY = XB && XM == PW_X_NONE;    // stored as loaded
    __shared__ __attribute__((aligned(16))) unsigned char As[2][GR * 128];   // [m][t] bf16
    __shared__ __attribute__((aligned(16))) unsigned char Bs[2][XR * 128];   // [k][t] bf16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / NX, wn = wave % NX;
    int s, mt, ktile;
    wg_work(p, s, mt, ktile);
    const int m0 = mt * GR, n0 = ktile * XR;
    const int M = p.M, K = p.K, T = p.T;
    const int P16 = pw_pitch16(T, p.B);

    float ga[NG], gb[NG], gc[NG], xa[NX], xb[NX];
    int voG[NG], voX[NX], ldsG[NG], ldsX[NX];
    bool gv_[NG], xv_[NX];
#pragma unroll
    for (int i = 0; i < NG; ++i) {
        const int piece = tid + 512 * i;
        const int row = piece >> 3, ch = piece & 7;
        const int m = m0 + row;
        gv_[i] = m < M;
        voG[i] = GB ? (m * P16 + ch * 8) * 2 : (m * T + ch * 8) * 4;
        ga[i] = (GM != PW_X_NONE) ? p.ga[gv_[i] ? m : 0] : 1.f;
        gb[i] = (GM != PW_X_NONE) ? p.gb[gv_[i] ? m : 0] : 0.f;
        gc[i] = (GM == PW_X_AFFINE2) ? p.gc[gv_[i] ? m : 0] : 0.f;
        ldsG[i] = bf_off(row, ch);
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        const int piece = tid + 512 * i;
        const int row = piece >> 3, ch = piece & 7;
        const int k = n0 + row;
        xv_[i] = k < K;
        voX[i] = XB ? (k * P16 + ch * 8) * 2 : (k * T + ch * 8) * 4;
        xa[i] = (XM != PW_X_NONE) ? p.xa[xv_[i] ? k : 0] : 1.f;
        xb[i] = (XM != PW_X_NONE) ? p.xb[xv_[i] ? k : 0] : 0.f;
        ldsX[i] = bf_off(row, ch);
    }
    // a second G tensor (affine2) may have a different storage type than the first
    int voG2[GM == PW_X_AFFINE2 ? NG : 1];
    if constexpr (GM == PW_X_AFFINE2) {
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            const int piece = tid + 512 * i;
            const int m = m0 + (piece >> 3), ch = piece & 7;
            voG2[i] = G2B ? (m * P16 + ch * 8) * 2 : (m * T + ch * 8) * 4;
        }
    }

    // NST = 2 register stages: the tile of step st + 2 is requested before the MFMAs of step st and first used after the MFMAs
    // of step st + 1 (with one stage a step lasts about one memory latency: 8 waves per CU, nothing else to run meanwhile).
    // Measured: the project gradient 57 -> 53.5 us; the expand gradient, whose fp32 X pieces make a stage 48 registers, spills
    // with two stages (69 -> 82 us) and keeps one.
    // NST = 3: two stages for G, ONE for X -- for the expand gradient: its X (the block input, fp32, 33 MB re-read by all 16 row
    // tiles: L2 hits) is requested one step ahead, its G streams (dz1 and a1 from HBM) two steps ahead; 64 staging registers.
    constexpr int NSG = NST >= 2 ? 2 : 1, NSX = NST == 2 ? 2 : 1;
    u32x4 ra[NSG][NG][GB ? 1 : 2], ra2[NSG][GM == PW_X_AFFINE2 ? NG : 1][G2B ? 1 : 2], rb[NSX][NX][XB ? 1 : 2];
    auto load_x = [&](auto stg, int b, int t0) {
        constexpr int SX = NSX == 2 ? decltype(stg)::value : 0;
        const __amdgpu_buffer_rsrc_t rX = XB ? make_rsrc(reinterpret_cast<const u16*>(p.X) + (size_t)b * K * P16, (unsigned)K * P16 * 2u)
                                             : make_rsrc(p.X + (size_t)b * K * T, (unsigned)K * T * 4u);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
#pragma unroll
            for (int h = 0; h < (XB ? 1 : 2); ++h) rb[SX][i][h] = __builtin_amdgcn_raw_buffer_load_b128(rX, voX[i] + 16 * h, t0 * (XB ? 2 : 4), 0);
        }
    };
    auto load_tiles = [&](auto stg, int b, int t0) {
        constexpr int SG = decltype(stg)::value;
        const __amdgpu_buffer_rsrc_t rG = GB ? make_rsrc(reinterpret_cast<const u16*>(p.G) + (size_t)b * M * P16, (unsigned)M * P16 * 2u)
                                             : make_rsrc(p.G + (size_t)b * M * T, (unsigned)M * T * 4u);
        const float* g2p = GM == PW_X_AFFINE2 ? p.G2 : p.G;
        const __amdgpu_buffer_rsrc_t rG2 = G2B ? make_rsrc(reinterpret_cast<const u16*>(g2p) + (size_t)b * M * P16, (unsigned)M * P16 * 2u)
                                               : make_rsrc(g2p + (size_t)b * M * T, (unsigned)M * T * 4u);
#pragma unroll
        for (int i = 0; i < NG; ++i) {
#pragma unroll
            for (int h = 0; h < (GB ? 1 : 2); ++h) ra[SG][i][h] = __builtin_amdgcn_raw_buffer_load_b128(rG, voG[i] + 16 * h, t0 * (GB ? 2 : 4), 0);
            if constexpr (GM == PW_X_AFFINE2) {
#pragma unroll
                for (int h = 0; h < (G2B ? 1 : 2); ++h)
                    ra2[SG][i][h] = __builtin_amdgcn_raw_buffer_load_b128(rG2, voG2[i] + 16 * h, t0 * (G2B ? 2 : 4), 0);
            }
        }
        if constexpr (NST != 3) load_x(stg, b, t0);        // NST 3: X is requested separately, one step ahead
    };
    auto store_tiles = [&](auto stg, int buf, int t0) {
        constexpr int SG = decltype(stg)::value;
        constexpr int SX = NSX == 2 ? SG : 0;
        const bool tail = TAIL && (t0 + BF_BK > T);        // contraction index past T must contribute zero
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            u32x4 oa;
            if (GCOPY && !tail) {
                oa = ra[SG][i][0];
            } else {
                float va[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float gv;
                    if constexpr (GB) gv = pw_bf16_at(ra[SG][i][0], e);
                    else gv = __builtin_bit_cast(f32x4, ra[SG][i][e >> 2])[e & 3];
                    if constexpr (GM == PW_X_AFFINE2) {
                        float g2;
                        if constexpr (G2B) g2 = pw_bf16_at(ra2[SG][i][0], e);
                        else g2 = __builtin_bit_cast(f32x4, ra2[SG][i][e >> 2])[e & 3];
                        gv = fmaf(gv, ga[i], fmaf(g2, gb[i], gc[i]));
                    } else if constexpr (GM == PW_X_AFFINE_RELU6) gv = relu6f(fmaf(gv, ga[i], gb[i]));
                    va[e] = gv;
                }
                // rows past M were read as zero, but an affine transform of zero is not zero: kill them
                if constexpr (GM != PW_X_NONE) { if (!gv_[i]) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) va[e] = 0.f; } }
                if constexpr (TAIL) if (tail) {
                    const int tb = t0 + (((tid + 512 * i) & 7) << 3);
#pragma unroll
                    for (int e = 0; e < 8; ++e) { if (tb + e >= T) va[e] = 0.f; }
                }
                oa[0] = pack_bf16(va[0], va[1]); oa[1] = pack_bf16(va[2], va[3]); oa[2] = pack_bf16(va[4], va[5]); oa[3] = pack_bf16(va[6], va[7]);
            }
            *reinterpret_cast<u32x4*>(&As[buf][ldsG[i]]) = oa;
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            u32x4 ob;
            if (XCOPY && !tail) {
                ob = rb[SX][i][0];
            } else {
                float vb[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float xv;
                    if constexpr (XB) xv = pw_bf16_at(rb[SX][i][0], e);
                    else xv = __builtin_bit_cast(f32x4, rb[SX][i][e >> 2])[e & 3];
                    if constexpr (XM == PW_X_AFFINE_RELU6) xv = relu6f(fmaf(xv, xa[i], xb[i]));
                    vb[e] = xv;
                }
                if constexpr (XM != PW_X_NONE) { if (!xv_[i]) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) vb[e] = 0.f; } }
                if constexpr (TAIL) if (tail) {
                    const int tb = t0 + (((tid + 512 * i) & 7) << 3);
#pragma unroll
                    for (int e = 0; e < 8; ++e) { if (tb + e >= T) vb[e] = 0.f; }
                }
                ob[0] = pack_bf16(vb[0], vb[1]); ob[1] = pack_bf16(vb[2], vb[3]); ob[2] = pack_bf16(vb[4], vb[5]); ob[3] = pack_bf16(vb[6], vb[7]);
            }
            *reinterpret_cast<u32x4*>(&Bs[buf][ldsX[i]]) = ob;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nt = (T + BF_BK - 1) / BF_BK;
    const WgSpan sp = wg_span(p, s, nt);
    const int nsteps = sp.nb * sp.ntl, b_lo = sp.b_lo;
    const int lr = lane & 31, lh = lane >> 5;
    const int sw = (lr >> 1) & 7;
    const int rdA0 = (wm * 64 + lr) * 128, rdB0 = (wn * 64 + lr) * 128;
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, NSG - 1>;
    // step -> (batch element, t offset); indices past the end are clamped to the last step (an unconditional, redundant load:
    // a conditional one would make hipcc wait for the YOUNGER stage at the join)
    auto issue = [&](auto stg, int step) {
        const int q = min(step, nsteps - 1);
        load_tiles(stg, b_lo + q / sp.ntl, (sp.t_first + q % sp.ntl) * BF_BK);
    };
    auto issue_x = [&](int step) {
        const int q = min(step, nsteps - 1);
        load_x(S0{}, b_lo + q / sp.ntl, (sp.t_first + q % sp.ntl) * BF_BK);
    };
    auto mfma_block = [&](int cur) {
#pragma unroll
        for (int ks = 0; ks < BF_BK / 16; ++ks) {
            const int co = ((ks * 2 + lh) ^ sw) << 4;
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(&As[cur][rdA0 + co]);
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(&As[cur][rdA0 + 32 * 128 + co]);
            const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(&Bs[cur][rdB0 + co]);
            const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(&Bs[cur][rdB0 + 32 * 128 + co]);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
        }
        // (accumulators pinned as VGPRs, not AGPRs: with any AGPR use hipcc splits the 256 registers of a 512-thread block
        // 128 / 128 and the two staging stages spill)
        asm volatile("" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[1][0]), "+v"(acc[1][1]));
    };
    // the registers of stage SG are first USED after this point (a macro: clang rejects captured arrays as asm operands in a generic lambda)
#define WG_PIN(SG)                                                                                  \
    do {                                                                                            \
        _Pragma("unroll") for (int i_ = 0; i_ < NG; ++i_) {                                         \
            asm volatile("" : "+v"(ra[SG][i_][0]));                                                 \
            if constexpr (!GB) asm volatile("" : "+v"(ra[SG][i_][1]));                              \
            if constexpr (GM == PW_X_AFFINE2) {                                                     \
                asm volatile("" : "+v"(ra2[SG][i_][0]));                                            \
                if constexpr (!G2B) asm volatile("" : "+v"(ra2[SG][i_][1]));                        \
            }                                                                                       \
        }                                                                                           \
        _Pragma("unroll") for (int i_ = 0; i_ < NX; ++i_) {                                         \
            asm volatile("" : "+v"(rb[NSX == 2 ? SG : 0][i_][0]));                                  \
            if constexpr (!XB) asm volatile("" : "+v"(rb[NSX == 2 ? SG : 0][i_][1]));               \
        }                                                                                           \
    } while (0)
    if constexpr (NST == 1) {
        if (nsteps > 0) {
            issue(S0{}, 0);
            store_tiles(S0{}, 0, sp.t_first * BF_BK);
        }
        __syncthreads();
        for (int st = 0; st < nsteps; ++st) {
            issue(S0{}, st + 1);
            __builtin_amdgcn_sched_barrier(0);
            mfma_block(st & 1);
            WG_PIN(0);
            __builtin_amdgcn_sched_barrier(0);
            if (st + 1 < nsteps) store_tiles(S0{}, (st + 1) & 1, (sp.t_first + (st + 1) % sp.ntl) * BF_BK);
            __syncthreads();
        }
    } else {
    if (nsteps > 0) {
        issue(S0{}, 0);
        if constexpr (NST == 3) issue_x(0);
        issue(S1{}, 1);
        store_tiles(S0{}, 0, sp.t_first * BF_BK);
    }
    __syncthreads();
    for (int st = 0; st < nsteps; st += 2) {
        // even step st: LDS 0; stage 1 holds step st + 1; stage 0 is free -> step st + 2
        if constexpr (NST == 3) issue_x(st + 1);           // X first: it is needed a step sooner than the G tiles requested below
        issue(S0{}, st + 2);
        __builtin_amdgcn_sched_barrier(0);
        mfma_block(0);
        WG_PIN(1);
        __builtin_amdgcn_sched_barrier(0);
        if (st + 1 < nsteps) store_tiles(S1{}, 1, (sp.t_first + (st + 1) % sp.ntl) * BF_BK);
        __syncthreads();
        if (st + 1 >= nsteps) break;
        // odd step st + 1: LDS 1; stage 0 holds step st + 2; stage 1 is free -> step st + 3
        if constexpr (NST == 3) issue_x(st + 2);
        issue(S1{}, st + 3);
        __builtin_amdgcn_sched_barrier(0);
        mfma_block(1);
        WG_PIN(0);
        __builtin_amdgcn_sched_barrier(0);
        if (st + 2 < nsteps) store_tiles(S0{}, 0, (sp.t_first + (st + 2) % sp.ntl) * BF_BK);
        __syncthreads();
    }
    }
#undef WG_PIN
    const int col = lane & 31, half = lane >> 5;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const int k = n0 + wn * 64 + j * 32 + col;
                if (m < M && k < K) p.partial[((size_t)s * M + m) * K + k] = acc[i][j][r];
            }
}
