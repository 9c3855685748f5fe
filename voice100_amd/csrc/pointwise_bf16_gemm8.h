// The 8-wave NN GEMM kernels: pw_gemm_bf16_kernel (any shape) and pw_gemm_bf16_fast_kernel (buffer-addressed).
#pragma once
#include "pointwise_bf16_common.h"

// 8 consecutive bf16 of A[m][k..k+7], RAW (address clamped when out of range; mask8bf at the use)
template <bool KV>
__device__ __forceinline__ uint4 ld8bf(const u16* __restrict__ base, size_t row_off, int k, int K, bool row_ok) {
    uint4 v;
    if constexpr (KV) {
        const bool ok = row_ok && k < K;
        v = *reinterpret_cast<const uint4*>(base + (ok ? row_off + k : 0));
    } else {
        unsigned t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool ok = row_ok && (k + e) < K;
            t[e] = base[ok ? row_off + k + e : 0];
        }
        v.x = t[0] | (t[1] << 16); v.y = t[2] | (t[3] << 16); v.z = t[4] | (t[5] << 16); v.w = t[6] | (t[7] << 16);
    }
    return v;
}

__device__ __forceinline__ uint4 mask8bf(uint4 v, int k, int K, bool row_ok) {
    unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned lo = (row_ok && (k + 2 * e) < K) ? 0xffffu : 0u;
        const unsigned hi = (row_ok && (k + 2 * e + 1) < K) ? 0xffff0000u : 0u;
        w[e] &= (lo | hi);
    }
    return uint4{w[0], w[1], w[2], w[3]};
}

template <int XM_, int EPI_, bool TV, bool KV, bool F16 = false>
__global__ __launch_bounds__(256) void pw_gemm_bf16_kernel(PwParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char As[2][128 * 128];   // [m][k] bf16, 16 KB per buffer
    __shared__ __attribute__((aligned(16))) unsigned char Bs[2][128 * 128];   // [t][k] bf16
    __shared__ float red[2][2][64][2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int b, tt, mt;
    pw_work(p, b, tt, mt);
    const int m0 = mt * PW_BM, t0 = tt * PW_BN;
    const int M = p.M, K = p.K, T = p.T;
    const int x_mode = PW_MODE(XM_, p.x_mode);
    const size_t xoff = (size_t)b * K * T;

    // A tile: 128 rows x 8 chunks(8 bf16) = 1024 16-byte pieces, 4 per thread
    // B tile: 64 k x 128 t fp32; thread owns 8 consecutive k (one chunk) x 4 consecutive t
    const int b_tq = (tid & 31) * 4;       // t offset in tile
    const int b_kc = tid >> 5;             // chunk 0..7  -> k = 8*b_kc .. +7

    uint4 ra[4];
    f32x4 rb[8], rb2[8];
    float ca[8], cb[8], cc[8];
    auto load_tiles = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = tid + 256 * i;
            const int row = piece >> 3, ch = piece & 7;
            ra[i] = ld8bf<KV>(p.Abf, (size_t)(m0 + row) * K, k0 + ch * 8, K, (m0 + row) < M);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + b_kc * 8 + e;
            const bool kv = k < K;
            rb[e] = ld4<TV>(p.X, xoff + (size_t)k * T, t0 + b_tq, T, kv);
            if (x_mode == PW_X_AFFINE2) rb2[e] = ld4<TV>(p.X2, xoff + (size_t)k * T, t0 + b_tq, T, kv);
            if (x_mode != PW_X_NONE) { ca[e] = ldc(p.xa, k, kv, 1.f); cb[e] = ldc(p.xb, k, kv, 0.f); }
            if (x_mode == PW_X_AFFINE2) cc[e] = ldc(p.xc, k, kv, 0.f);
        }
    };
    auto store_tiles = [&](int buf, int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = tid + 256 * i;
            const int row = piece >> 3, ch = piece & 7;
            *reinterpret_cast<uint4*>(&As[buf][bf_off(row, ch)]) = mask8bf(ra[i], k0 + ch * 8, K, (m0 + row) < M);
        }
        float v[8][4];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + b_kc * 8 + e;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v[e][q] = (k < K && t0 + b_tq + q < T) ? pw_x_transform(x_mode, rb[e][q], rb2[e][q], ca[e], cb[e], cc[e]) : 0.f;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint4 o;
            o.x = pack16<F16>(v[0][q], v[1][q]); o.y = pack16<F16>(v[2][q], v[3][q]);
            o.z = pack16<F16>(v[4][q], v[5][q]); o.w = pack16<F16>(v[6][q], v[7][q]);
            *reinterpret_cast<uint4*>(&Bs[buf][bf_off(b_tq + q, b_kc)]) = o;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = (K + BF_BK - 1) / BF_BK;
    load_tiles(0);
    store_tiles(0, 0);
    __syncthreads();
    const int lr = lane & 31, lh = lane >> 5;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) load_tiles((kt + 1) * BF_BK);
        __builtin_amdgcn_sched_barrier(0);      // loads are issued before the MFMA block ...
#pragma unroll
        for (int ks = 0; ks < BF_BK / 16; ++ks) {          // 16 k per MFMA: lane half lh holds k = 16*ks + 8*lh .. +7
            const int ch = ks * 2 + lh;
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(&As[cur][bf_off(wm * 64 + lr, ch)]);
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(&As[cur][bf_off(wm * 64 + 32 + lr, ch)]);
            const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(&Bs[cur][bf_off(wn * 64 + lr, ch)]);
            const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(&Bs[cur][bf_off(wn * 64 + 32 + lr, ch)]);
            acc[0][0] = mfma16<F16>(a0, b0, acc[0][0]);
            acc[0][1] = mfma16<F16>(a0, b1, acc[0][1]);
            acc[1][0] = mfma16<F16>(a1, b0, acc[1][0]);
            acc[1][1] = mfma16<F16>(a1, b1, acc[1][1]);
        }
        // ... and first USED after it: without this fence hipcc hoists the staging arithmetic (and the
        // vmcnt wait it needs) above the MFMAs, which exposes the whole memory latency every k-step.
        asm volatile("" : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[1][0]), "+a"(acc[1][1]));   // accumulators stay in AGPRs
        asm volatile("" : "+v"(rb[0]), "+v"(rb[1]), "+v"(rb[2]), "+v"(rb[3]), "+v"(rb[4]), "+v"(rb[5]), "+v"(rb[6]), "+v"(rb[7]));
        if (x_mode == PW_X_AFFINE2)
            asm volatile("" : "+v"(rb2[0]), "+v"(rb2[1]), "+v"(rb2[2]), "+v"(rb2[3]), "+v"(rb2[4]), "+v"(rb2[5]), "+v"(rb2[6]), "+v"(rb2[7]));
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < nk) store_tiles(cur ^ 1, (kt + 1) * BF_BK);
        __syncthreads();
    }
    pw_epilogue<EPI_>(p, acc, b, m0, t0, tt, wm, wn, lane, red);
}

// ---------------------------------------------------------------------------------------------
// Fast path of the NN kernel for full tiles (K % 64 == 0, T % 128 == 0 -- every layer of the
// reference networks at the benchmark shapes).  Same tiling and LDS images as above, but every
// global access is a buffer load: the descriptors are wave-uniform, the per-lane byte offsets are
// computed once, the k-step advance is a scalar offset, and rows past M fall outside the
// descriptor and read as zero in hardware -- no per-load address arithmetic, no masks.
template <int XM, int EPI, int BM, bool F16 = false, bool TAPS = false, int IO = 0, bool PERSIST = false>
__global__ __launch_bounds__(BM * 2) void pw_gemm_bf16_fast_kernel(PwParams p) {
    static_assert(!TAPS || XM == PW_X_NONE, "tap-addressed X has no prologue");
    static_assert(!(IO != 0 && TAPS), "16-bit activation storage: no tap-addressed form");
    static_assert(((IO & PW_IO_F16) != 0) == (F16 && IO != 0), "fp16-stored tensors go with fp16 operands (PW_IO_F16), bf16-stored ones with bf16");
    static_assert(!(F16 && IO != 0 && XM != PW_X_NONE), "fp16 storage: plain X operand only (inference)");
    // PERSIST: the grid is a divisor of the tile count and a workgroup walks tiles v = blockIdx.x, + gridDim.x, ...; the first two
    // k-tiles of the NEXT tile are requested into the (idle) staging registers before the epilogue of the current one, so a
    // tile's start does not wait a memory latency (2.5 us of the ~15 us a 256 x 128 x 512 tile takes) and the epilogue's
    // stores overlap the next tile's loads.  For the short-K GEMMs (several tiles per CU); XM == NONE only (register budget).
    static_assert(!PERSIST || (XM == PW_X_NONE && !TAPS), "persistent form: plain X operand");
    constexpr bool XB = (IO & PW_IO_X) != 0, X2B = (IO & PW_IO_X2) != 0;    // operand tensors stored as bf16 (pitched rows)
    using XReg = std::conditional_t<XB, u32x2, u32x4>;
    using X2Reg = std::conditional_t<X2B, u32x2, u32x4>;
    // BM x 128 block tile, BM/64 x 2 waves of 64x64.  BM = 256 (8 waves, one block per CU) halves the L2 traffic of
    // the X operand, which is what bounds these GEMMs (each X tile is re-read by every M-tile); BM = 128 for M <= 128.
    constexpr int NT = BM * 2;                      // threads
    constexpr int KPT = 2048 / NT;                  // k rows per thread in the X patch: 8 (256 threads) or 4 (512)
    constexpr int A_BYTES = BM * 128;               // one A stage: [BM][64] bf16
    constexpr int SMEM = (BM * 128 * 4 > 2 * A_BYTES + 2 * 128 * 128) ? BM * 128 * 4 : 2 * A_BYTES + 2 * 128 * 128;
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];      // stages, reused by the epilogue as [BM][128] fp32
    unsigned char* As = smem;                       // [2][BM][64] bf16
    unsigned char* Bs = smem + 2 * A_BYTES;         // [2][128][64] bf16

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int b, tt, mt;
    int vtile = blockIdx.x;
    const int ntiles_all = PERSIST ? p.n_mtiles * p.n_ttiles * p.B : 0;
    if constexpr (PERSIST) pw_work_v(p, vtile, ntiles_all, b, tt, mt);
    else pw_work(p, b, tt, mt);
    int m0 = mt * BM, t0 = tt * PW_BN;
    const int M = p.M, K = p.K, T = p.T;
    // tap-addressed X: physical rows are the cx channels of the padded tensor, row pitch Tx (see PwParams)
    const int Tx = TAPS ? p.Tx : T;
    const int Kx = TAPS ? p.cx : K;
    const int P16 = pw_pitch16(T, p.B);                  // row pitch of the bf16-stored tensors
    const int TxX = XB ? P16 : Tx, TxX2 = X2B ? P16 : Tx;
    constexpr int EX = XB ? 2 : 4, EX2 = X2B ? 2 : 4;      // bytes per element

    const __amdgpu_buffer_rsrc_t rA = make_rsrc(p.Abf, (unsigned)M * K * 2u);
    __amdgpu_buffer_rsrc_t rX = make_rsrc(reinterpret_cast<const char*>(p.X) + (size_t)b * Kx * TxX * EX,
                                          (unsigned)Kx * TxX * EX);
    const __amdgpu_buffer_rsrc_t rX2 = make_rsrc(reinterpret_cast<const char*>(XM == PW_X_AFFINE2 ? p.X2 : p.X) +
                                                     (size_t)b * Kx * (XM == PW_X_AFFINE2 ? TxX2 * EX2 : TxX * EX),
                                                 (unsigned)Kx * (XM == PW_X_AFFINE2 ? TxX2 * EX2 : TxX * EX));
    const __amdgpu_buffer_rsrc_t rCa = make_rsrc(XM != PW_X_NONE ? p.xa : p.X, (unsigned)K * 4u);
    const __amdgpu_buffer_rsrc_t rCb = make_rsrc(XM != PW_X_NONE ? p.xb : p.X, (unsigned)K * 4u);
    const __amdgpu_buffer_rsrc_t rCc = make_rsrc(XM == PW_X_AFFINE2 ? p.xc : p.X, (unsigned)K * 4u);

    const int b_tq = (tid & 31) * 4;               // t offset in tile
    const int b_kg = tid >> 5;                     // k group: rows KPT*b_kg .. +KPT-1
    int voA[4], ldsA[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int piece = tid + NT * i;
        const int row = piece >> 3, ch = piece & 7;
        voA[i] = ((m0 + row) * K + ch * 8) * 2;
        ldsA[i] = bf_off(row, ch);
    }
    int voX[KPT], voX2[XM == PW_X_AFFINE2 ? KPT : 1];
#pragma unroll
    for (int e = 0; e < KPT; ++e) {
        voX[e] = ((KPT * b_kg + e) * TxX + t0 + b_tq) * EX;
        if constexpr (XM == PW_X_AFFINE2) voX2[e] = ((KPT * b_kg + e) * TxX2 + t0 + b_tq) * EX2;
    }
    const int voC = KPT * b_kg * 4;
    int ldsB[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) ldsB[q] = bf_off(b_tq + q, (KPT * b_kg) >> 3) + ((KPT * b_kg) & 7) * 2;
    // PERSIST: re-aim the X descriptor and the per-lane offsets at tile v
    auto retarget = [&](int v) {
        pw_work_v(p, v, ntiles_all, b, tt, mt);
        m0 = mt * BM; t0 = tt * PW_BN;
        rX = make_rsrc(reinterpret_cast<const char*>(p.X) + (size_t)b * Kx * TxX * EX, (unsigned)Kx * TxX * EX);
#pragma unroll
        for (int i = 0; i < 4; ++i) voA[i] = ((m0 + ((tid + NT * i) >> 3)) * K + ((tid + NT * i) & 7) * 8) * 2;
#pragma unroll
        for (int e = 0; e < KPT; ++e) voX[e] = ((KPT * b_kg + e) * TxX + t0 + b_tq) * EX;
    };

    // NST register stages of global loads in flight: with two, the loads of tile k+2 are issued
    // before the MFMA block of tile k and first used during the MFMA block of tile k+1.  The two-tensor prologue
    // (XM == AFFINE2) keeps one stage at BM = 128 (register budget); at BM = 256 its patch is half as large.
    constexpr int NST = (XM == PW_X_AFFINE2 && KPT == 8) ? 1 : 2;
    constexpr int NC = KPT / 4;                     // float4 coefficient loads per array
    u32x4 ra[NST][4], rca[NC], rcb[NC], rcc[XM == PW_X_AFFINE2 ? NC : 1];
    XReg rb[NST][KPT];
    X2Reg rb2[NST][XM == PW_X_AFFINE2 ? KPT : 1];
    auto load_tiles = [&](int k0, auto stg) {
        constexpr int SG = decltype(stg)::value;
#pragma unroll
        for (int i = 0; i < 4; ++i) ra[SG][i] = __builtin_amdgcn_raw_buffer_load_b128(rA, voA[i], k0 * 2, 0);
        int so = k0 * TxX * EX;
        if constexpr (TAPS) {                  // a k-tile never straddles two taps (cx % 64 == 0, checked by the launcher)
            const int tap = k0 / p.cx;
            so = ((k0 - tap * p.cx) * Tx + pw_tap_shift(p.shifts, tap)) * 4;
        }
#pragma unroll
        for (int e = 0; e < KPT; ++e) {
            if constexpr (XB) rb[SG][e] = __builtin_amdgcn_raw_buffer_load_b64(rX, voX[e], so, 0);
            else rb[SG][e] = __builtin_amdgcn_raw_buffer_load_b128(rX, voX[e], so, 0);
            if constexpr (XM == PW_X_AFFINE2) {
                if constexpr (X2B) rb2[SG][e] = __builtin_amdgcn_raw_buffer_load_b64(rX2, voX2[e], k0 * TxX2 * EX2, 0);
                else rb2[SG][e] = __builtin_amdgcn_raw_buffer_load_b128(rX2, voX2[e], k0 * TxX2 * EX2, 0);
            }
        }
    };
    // BN coefficients of the tile that is about to be STORED: tiny, L2-resident, single register stage
    auto load_coefs = [&](int k0) {
        if constexpr (XM != PW_X_NONE) {
#pragma unroll
            for (int h = 0; h < NC; ++h) {
                rca[h] = __builtin_amdgcn_raw_buffer_load_b128(rCa, voC + 16 * h, k0 * 4, 0);
                rcb[h] = __builtin_amdgcn_raw_buffer_load_b128(rCb, voC + 16 * h, k0 * 4, 0);
                if constexpr (XM == PW_X_AFFINE2) rcc[h] = __builtin_amdgcn_raw_buffer_load_b128(rCc, voC + 16 * h, k0 * 4, 0);
            }
        }
    };
    // one quarter of a tile store: A piece `q` and t-column `q` of this thread's X patch
    auto store_slice = [&](int buf, auto stg, auto slc) {
        constexpr int SG = decltype(stg)::value;
        constexpr int q = decltype(slc)::value;
        *reinterpret_cast<u32x4*>(As + buf * A_BYTES + ldsA[q]) = ra[SG][q];
        if constexpr (XM == PW_X_NONE && XB) {
            // plain 16-bit X (bf16, or fp16 under F16: the stored format IS the operand format): the [k][t] -> [t][k] transposition is a byte shuffle of the loaded words (column q of rows 2j, 2j + 1
            // -> word j), one v_perm_b32 per two elements instead of unpack + unpack + v_cvt_pk
            constexpr unsigned sel = (q & 1) ? 0x07060302u : 0x05040100u;
            unsigned char* dst = Bs + buf * (128 * 128) + ldsB[q];
            if constexpr (KPT == 8) {
                u32x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_perm(rb[SG][2 * j + 1][q >> 1], rb[SG][2 * j][q >> 1], sel);
                *reinterpret_cast<u32x4*>(dst) = o;
            } else {
                uint2 o;
                o.x = __builtin_amdgcn_perm(rb[SG][1][q >> 1], rb[SG][0][q >> 1], sel);
                o.y = __builtin_amdgcn_perm(rb[SG][3][q >> 1], rb[SG][2][q >> 1], sel);
                *reinterpret_cast<uint2*>(dst) = o;
            }
            return;
        }
        float v[KPT];
#pragma unroll
        for (int e = 0; e < KPT; ++e) {
            float x;
            if constexpr (XB) x = pw_bf16_at(rb[SG][e], q);
            else x = __builtin_bit_cast(f32x4, rb[SG][e])[q];
            if constexpr (XM == PW_X_NONE) v[e] = x;
            else {
                const float ca = __builtin_bit_cast(f32x4, rca[e >> 2])[e & 3];
                const float cb = __builtin_bit_cast(f32x4, rcb[e >> 2])[e & 3];
                if constexpr (XM == PW_X_AFFINE_RELU6) v[e] = relu6f(fmaf(x, ca, cb));
                else {
                    float x2;
                    if constexpr (X2B) x2 = pw_bf16_at(rb2[SG][e], q);
                    else x2 = __builtin_bit_cast(f32x4, rb2[SG][e])[q];
                    v[e] = fmaf(x, ca, fmaf(x2, cb, __builtin_bit_cast(f32x4, rcc[e >> 2])[e & 3]));
                }
            }
        }
        unsigned char* dst = Bs + buf * (128 * 128) + ldsB[q];
        if constexpr (KPT == 8) {
            u32x4 o;
            o[0] = pack16<F16>(v[0], v[1]); o[1] = pack16<F16>(v[2], v[3]); o[2] = pack16<F16>(v[4], v[5]); o[3] = pack16<F16>(v[6], v[7]);
            *reinterpret_cast<u32x4*>(dst) = o;
        } else {
            uint2 o;
            o.x = pack16<F16>(v[0], v[1]); o.y = pack16<F16>(v[2], v[3]);
            *reinterpret_cast<uint2*>(dst) = o;
        }
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, NST - 1>;
    using Q0 = std::integral_constant<int, 0>; using Q1 = std::integral_constant<int, 1>;
    using Q2 = std::integral_constant<int, 2>; using Q3 = std::integral_constant<int, 3>;
    auto store_tiles = [&](int buf, auto stg) {
        store_slice(buf, stg, Q0{}); store_slice(buf, stg, Q1{}); store_slice(buf, stg, Q2{}); store_slice(buf, stg, Q3{});
    };

    f32x16 acc[2][2];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    };
    zero_acc();

    const int nk = (K + BF_BK - 1) / BF_BK;
    const int lr = lane & 31, lh = lane >> 5;
    const int sw = (lr >> 1) & 7;                       // fragment rows are lr (+32, +64..): same swizzle key
    const int rdA0 = (wm * 64 + lr) * 128, rdB0 = (wn * 64 + lr) * 128;
    auto mfma_step = [&](int cur, int ks) {
        const int co = ((ks * 2 + lh) ^ sw) << 4;
        const unsigned char* Ab = As + cur * A_BYTES;
        const unsigned char* Bb = Bs + cur * (128 * 128);
        const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(Ab + rdA0 + co);
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(Ab + rdA0 + 32 * 128 + co);
        const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(Bb + rdB0 + co);
        const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(Bb + rdB0 + 32 * 128 + co);
        acc[0][0] = mfma16<F16>(a0, b0, acc[0][0]);
        acc[0][1] = mfma16<F16>(a0, b1, acc[0][1]);
        acc[1][0] = mfma16<F16>(a1, b0, acc[1][0]);
        acc[1][1] = mfma16<F16>(a1, b1, acc[1][1]);
    };
    auto mfma_block = [&](int cur) {
#pragma unroll
        for (int ks = 0; ks < BF_BK / 16; ++ks) mfma_step(cur, ks);
    };
    // pin: the registers of stage SG are first USED after this point.
    // (a macro, not a lambda: clang rejects captured arrays as inline-asm operands inside a generic lambda)
#define PW_PIN(SG)                                                                                            \
    do {                                                                                                      \
        _Pragma("unroll") for (int e_ = 0; e_ < KPT; ++e_) {                                                  \
            asm volatile("" : "+v"(rb[SG][e_]));                                                              \
            if constexpr (XM == PW_X_AFFINE2) asm volatile("" : "+v"(rb2[SG][e_]));                           \
        }                                                                                                     \
        asm volatile("" : "+v"(ra[SG][0]), "+v"(ra[SG][1]), "+v"(ra[SG][2]), "+v"(ra[SG][3]));                \
    } while (0)
    if constexpr (PERSIST) {               // first tile: k-tiles 0 and 1 (later tiles: requested before the previous epilogue)
        load_tiles(0, S0{});
        if (nk > 1) load_tiles(BF_BK, S1{});
    }
    for (;;) {
    if constexpr (NST == 1) {
        load_tiles(0, S0{});
        load_coefs(0);
        store_tiles(0, S0{});
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int cur = kt & 1;
            if (kt + 1 < nk) { load_tiles((kt + 1) * BF_BK, S0{}); load_coefs((kt + 1) * BF_BK); }
            __builtin_amdgcn_sched_barrier(0);      // loads are issued before the MFMA block ...
            mfma_block(cur);
            // ... and first USED after it: without the fence hipcc hoists the staging arithmetic (and the vmcnt wait it
            // needs) above the MFMAs, which exposes the whole memory latency every k-step
            asm volatile("" : "+a"(acc[0][0]), "+a"(acc[0][1]), "+a"(acc[1][0]), "+a"(acc[1][1]));
            PW_PIN(0);
            __builtin_amdgcn_sched_barrier(0);
            if (kt + 1 < nk) store_tiles(cur ^ 1, S0{});
            __syncthreads();
        }
    } else {
        // tile t lives in register stage t&1 and LDS buffer t&1
        if constexpr (!PERSIST) {
            load_tiles(0, S0{});
            load_coefs(0);
            if (nk > 1) load_tiles(BF_BK, S1{});
        }
        store_tiles(0, S0{});
        __syncthreads();
        // Steady state: the tile to be stored was loaded a whole iteration ago, so its transform + LDS writes are
        // interleaved with the MFMAs of the current tile (matrix pipe and VALU/LDS overlap inside one wave).
        int kt = 0;
        // Main loop: both prefetches are unconditional.  (A conditional load makes hipcc's waitcnt insertion assume
        // the not-taken count at the join, so the wait for the OLDER stage degenerates into a wait for the prefetch
        // just issued -- the whole point of the second register stage.)
        for (; kt + 3 < nk; kt += 2) {
            // even tile kt: compute LDS 0; stage 1 holds tile kt+1; stage 0 is free -> tile kt+2.
            // vmcnt retires in order: the coefficient loads needed first are issued BEFORE the tile prefetch
            load_coefs((kt + 1) * BF_BK);
            __builtin_amdgcn_sched_barrier(0);
            load_tiles((kt + 2) * BF_BK, S0{});
            __builtin_amdgcn_sched_barrier(0);
            mfma_step(0, 0); mfma_step(0, 1);
            __builtin_amdgcn_sched_barrier(0);
            PW_PIN(NST - 1);
            store_slice(1, S1{}, Q0{}); mfma_step(0, 2);
            store_slice(1, S1{}, Q1{}); mfma_step(0, 3);
            store_slice(1, S1{}, Q2{}); store_slice(1, S1{}, Q3{});
            __syncthreads();
            // odd tile kt+1: compute LDS 1; stage 0 holds tile kt+2; stage 1 is free -> tile kt+3
            load_coefs((kt + 2) * BF_BK);
            __builtin_amdgcn_sched_barrier(0);
            load_tiles((kt + 3) * BF_BK, S1{});
            __builtin_amdgcn_sched_barrier(0);
            mfma_step(1, 0); mfma_step(1, 1);
            __builtin_amdgcn_sched_barrier(0);
            PW_PIN(0);
            store_slice(0, S0{}, Q0{}); mfma_step(1, 2);
            store_slice(0, S0{}, Q1{}); mfma_step(1, 3);
            store_slice(0, S0{}, Q2{}); store_slice(0, S0{}, Q3{});
            __syncthreads();
        }
        // Tail: the last two or three tiles (at most one pass), prefetches guarded
        for (; kt + 1 < nk; kt += 2) {
            const bool more = kt + 2 < nk;          // wave-uniform; MFMAs stay outside the branches (one accumulator chain)
            load_coefs((kt + 1) * BF_BK);
            __builtin_amdgcn_sched_barrier(0);
            if (more) load_tiles((kt + 2) * BF_BK, S0{});
            __builtin_amdgcn_sched_barrier(0);
            PW_PIN(NST - 1);
            mfma_step(0, 0); mfma_step(0, 1);
            store_slice(1, S1{}, Q0{}); mfma_step(0, 2);
            store_slice(1, S1{}, Q1{}); mfma_step(0, 3);
            store_slice(1, S1{}, Q2{}); store_slice(1, S1{}, Q3{});
            __syncthreads();
            if (more) load_coefs((kt + 2) * BF_BK);
            __builtin_amdgcn_sched_barrier(0);
            if (more) PW_PIN(0);
            mfma_step(1, 0); mfma_step(1, 1);
            if (more) store_slice(0, S0{}, Q0{});
            mfma_step(1, 2);
            if (more) store_slice(0, S0{}, Q1{});
            mfma_step(1, 3);
            if (more) { store_slice(0, S0{}, Q2{}); store_slice(0, S0{}, Q3{}); }
            __syncthreads();
        }
        if (kt < nk) {                         // odd tile count: the last tile already sits in LDS 0
            mfma_block(0);
            __syncthreads();                   // the epilogue reuses the stage buffers: every wave must be done reading
        }
    }
#undef PW_PIN
    if constexpr (PERSIST) {
        const int eb_ = b, em0 = m0, et0 = t0, ett = tt;
        const int vnext = vtile + (int)gridDim.x;
        const bool more_tiles = vnext < ntiles_all;               // block-uniform
        // this tile's R / coefficient loads first, the next tile's first k-tiles queued behind them, then the epilogue proper
        const bool lean = pw_tile_is_full(p, BM, em0, et0);
        PwEpilogueFull<EPI, BM, IO> ef;
        if (lean) ef.issue(p, eb_, em0, et0, tid);
        if (more_tiles) {
            retarget(vnext);
            load_tiles(0, S0{});
            if (nk > 1) load_tiles(BF_BK, S1{});
        }
        if (lean) ef.finish(p, acc, reinterpret_cast<float*>(smem), eb_, ett, wm, wn, tid);
        else pw_epilogue_lds<EPI, BM, IO>(p, acc, reinterpret_cast<float*>(smem), eb_, em0, et0, ett, wm, wn, tid);
        if (more_tiles) {
            vtile = vnext;
            zero_acc();
            __syncthreads();               // the epilogue's reads of the parked tile are done: the stage buffers are free again
            continue;
        }
    } else {
        pw_epilogue_lds<EPI, BM, IO>(p, acc, reinterpret_cast<float*>(smem), b, m0, t0, tt, wm, wn, tid);
    }
    break;
    }
}
