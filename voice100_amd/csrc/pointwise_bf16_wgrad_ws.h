// pw_wgrad_bf16_ws_kernel: the wave-specialised backward-weight kernel.
#pragma once
#include "pointwise_bf16_common.h"

// Wave-specialised backward-weight (round 3): pw_gemm_bf16_ws_kernel's division of labour on pw_wgrad_bf16_wide_kernel's tile.
// Twelve waves: waves 0-7 (64 x 64 each of the GR x XR tile) copy the PLAIN operand's 256 x 64 bf16 tile to LDS as loaded (4 pieces
// per lane, two register stages, one ds_write_b128 + the request two steps ahead behind each k-step's MFMAs) and run the MFMAs;
// waves 8-11 stage the TRANSFORMED operand's 128 x 64 tile (BatchNorm-backward affine of two bf16 tensors, or BatchNorm + ReLU6):
// NSQ register stages of loads, transform, bf16 pack, 4 ds_write_b128 per lane and step.  One barrier per step.  Full tiles only
// (M % GR == 0, K % XR == 0); TAIL: T % 64 != 0, contraction indices past T are zeroed in BOTH operands (masks on the plain one).
// GRP (pointwise_bf16_wgrad_group.h): the workgroup walks the WHOLE contraction of its tile in the order of the p.S splits and sums
// the splits' partial tiles itself, in slab order from 0.f (pw_slab_reduce4_kernel's sum, bit for bit); p.partial is then the
// finished [M][K] gradient.  The running sum's fragments live in registers, the last RL of the four in LDS (runs: one f32x4 per
// matrix lane and register quad, [RL * 4][512]).
template <int GM, int XM, bool TAIL, int IO, int GR, int XR, int NSW, bool GRP = false, int RL = 0>
__device__ __forceinline__ void pw_wgrad_bf16_ws_body(const WgParams& p, const int s, const int mt, const int ktile, unsigned char* const As0,
                                                      unsigned char* const Bs0, f32x4* const runs) {
    // (both plain -- G = the finished gradient da1, round 5 --: G takes the 128-row side and its "transform" is a copy)
    static_assert(!(GM != PW_X_NONE && XM != PW_X_NONE), "at most one transformed operand (128 rows); the other one plain (256 rows)");
    static_assert((IO & WG_IO_G) && (IO & WG_IO_X) && (GM != PW_X_AFFINE2 || (IO & WG_IO_G2)), "bf16-stored operands only");
    constexpr bool PG = GM == PW_X_NONE && XM != PW_X_NONE; // the plain 256-row operand is G
    static_assert((PG ? GR : XR) == 256 && (PG ? XR : GR) == 128, "tile shape");
    constexpr int QM = PG ? XM : GM;                        // the transform
    constexpr int NX = XR / 64;
    static_assert(NSW == 4 || NSW == 8, "staging waves: one or two per SIMD");
    constexpr int NSQ = (QM == PW_X_AFFINE2 && NSW == 4) ? 3 : 4;    // register stages of the transformed operand
    constexpr int NQP = 16 / NSW;                           // 16-byte pieces per staging lane and step
    constexpr int QRS = 8 * NSW;                            // rows between a lane's pieces
    unsigned char (*As)[GR * 128] = reinterpret_cast<unsigned char (*)[GR * 128]>(As0);   // [2][m][t] bf16
    unsigned char (*Bs)[XR * 128] = reinterpret_cast<unsigned char (*)[XR * 128]>(Bs0);   // [2][k][t] bf16
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = mt * GR, n0 = ktile * XR;
    const int M = p.M, K = p.K, T = p.T;
    const int P16 = pw_pitch16(T, p.B);
    const int nt = (T + BF_BK - 1) / BF_BK;
    const WgSpan sp = GRP ? WgSpan{0, p.B, 0, nt} : wg_span(p, s, nt);       // GRP: the splits' utterance runs, one behind the other
    const int nsteps = sp.nb * sp.ntl, b_lo = sp.b_lo;
    // step -> (batch element, t offset); steps past the end are clamped to the last (an unconditional, redundant load: a
    // conditional one would make hipcc wait for the YOUNGER stage at the join)
    auto step_bt = [&](int step, int& b, int& t0) {
        const int q = min(step, nsteps - 1);
        (void)q;
        const int bi = q / sp.ntl;
        b = b_lo + bi;
        t0 = (sp.t_first + q - bi * sp.ntl) * BF_BK;
    };
    // contraction indices t0 + 8 ch + e >= T of a 16-byte piece -> zero
    auto tail_mask = [&](u32x4 v, int tb) {
        const int nv = T - tb;                              // (one live value, constants compared against it: registers are short in GRP)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] &= nv > 2 * j + 1 ? 0xffffffffu : (nv > 2 * j ? 0xffffu : 0u);
        return v;
    };
    if (!GRP && nsteps == 0) {                              // (no work for this split: the partial tile is zeros)
        if (wave < 8) {
            const int wm = wave / NX, wn = wave % NX, col = lane & 31, half = lane >> 5;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, k = n0 + wn * 64 + j * 32 + col;
                        p.partial[((size_t)s * M + m) * K + k] = 0.f;
                    }
        }
        return;
    }

    if (wave >= 8) {
        // ------------------------------------------------ staging waves: the transformed operand ------------------------------------------------
        const int pt = tid - 512;
        const int qrow = pt >> 3, ch = pt & 7;              // piece i: row qrow + QRS i (same swizzle key), chunk ch
        const int row0 = PG ? n0 : m0, rows = PG ? K : M;
        const float* q1 = PG ? p.X : p.G;
        const float* q2 = PG ? p.X : p.G2;
        const float* pa = PG ? p.xa : p.ga;
        const float* pb = PG ? p.xb : p.gb;
        unsigned char (*Qs)[128 * 128] = PG ? reinterpret_cast<unsigned char (*)[128 * 128]>(Bs) : reinterpret_cast<unsigned char (*)[128 * 128]>(As);
        float ca[NQP], cb[NQP], cc[NQP];
#pragma unroll
        for (int i = 0; i < NQP; ++i) {
            const int r = row0 + qrow + QRS * i;
            ca[i] = QM != PW_X_NONE ? pa[r] : 1.f; cb[i] = QM != PW_X_NONE ? pb[r] : 0.f;
            cc[i] = QM == PW_X_AFFINE2 ? p.gc[r] : 0.f;
        }
        const int voQ = ((row0 + qrow) * P16 + ch * 8) * 2;
        const int stepQ = QRS * P16 * 2;
        const int ldsQ = bf_off(qrow, ch);
        u32x4 rq[NSQ][NQP], rq2[NSQ][QM == PW_X_AFFINE2 ? NQP : 1];
#define WS_SB() __builtin_amdgcn_sched_barrier(0)
        auto load_q = [&](int step, auto stg, int i) {
            constexpr int SG = decltype(stg)::value;
            int b, t0;
            step_bt(step, b, t0);
            const __amdgpu_buffer_rsrc_t r1 = make_rsrc(reinterpret_cast<const u16*>(q1) + (size_t)b * rows * P16, (unsigned)rows * P16 * 2u);
            rq[SG][i] = __builtin_amdgcn_raw_buffer_load_b128(r1, voQ, t0 * 2 + i * stepQ, 0);
            if constexpr (QM == PW_X_AFFINE2) {
                const __amdgpu_buffer_rsrc_t r2 = make_rsrc(reinterpret_cast<const u16*>(q2) + (size_t)b * rows * P16, (unsigned)rows * P16 * 2u);
                rq2[SG][i] = __builtin_amdgcn_raw_buffer_load_b128(r2, voQ, t0 * 2 + i * stepQ, 0);
            }
        };
        // step st (registers of stage SG) -> LDS slot st & 1; step st + NSQ requested into the same registers
        auto stage = [&](int st, auto stg) {
            constexpr int SG = decltype(stg)::value;
            unsigned char* Qd = Qs[st & 1] + ldsQ;
            int tb = 0;
            bool tail = false;
            if constexpr (TAIL) {
                int b, t0;
                step_bt(st, b, t0);
                tail = t0 + BF_BK > T;
                tb = t0 + ch * 8;
            }
            u32x4 o[NQP];
#pragma unroll
            for (int i = 0; i < NQP; ++i) {
                if constexpr (QM == PW_X_NONE) {            // plain operand on the staged side: copied as loaded
                    o[i] = rq[SG][i];
                    if constexpr (TAIL) { if (tail) o[i] = tail_mask(o[i], tb); }
                    continue;
                }
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float x = pw_bf16_at(rq[SG][i], e);
                    if constexpr (QM == PW_X_AFFINE2) v[e] = fmaf(x, ca[i], fmaf(pw_bf16_at(rq2[SG][i], e), cb[i], cc[i]));
                    else v[e] = relu6f(fmaf(x, ca[i], cb[i]));
                }
                o[i][0] = pack_bf16(v[0], v[1]); o[i][1] = pack_bf16(v[2], v[3]); o[i][2] = pack_bf16(v[4], v[5]); o[i][3] = pack_bf16(v[6], v[7]);
                if constexpr (TAIL) { if (tail) o[i] = tail_mask(o[i], tb); }
            }
            WS_SB();
#pragma unroll
            for (int i = 0; i < NQP; ++i) {                 // stores and the next requests interleaved
                *reinterpret_cast<u32x4*>(Qd + i * (QRS * 128)) = o[i];
                load_q(st + NSQ, stg, i);
                WS_SB();
            }
        };
        using S0 = std::integral_constant<int, 0>; using S1 = std::integral_constant<int, 1>;
        using S2 = std::integral_constant<int, 2>; using S3 = std::integral_constant<int, 3>;
#pragma unroll
        for (int i = 0; i < NQP; ++i) load_q(0, S0{}, i);
        WS_SB();
#pragma unroll
        for (int i = 0; i < NQP; ++i) load_q(1, S1{}, i);
        WS_SB();
#pragma unroll
        for (int i = 0; i < NQP; ++i) load_q(2, S2{}, i);
        WS_SB();
        if constexpr (NSQ == 4) {
#pragma unroll
            for (int i = 0; i < NQP; ++i) load_q(3, S3{}, i);
            WS_SB();
        }
        stage(0, S0{});
        __syncthreads();                                   // step 0 is in LDS
        // NSQ steps per trip with EXITS, not skipped bodies (pw_gemm_bf16_ws_kernel); the stores are unconditional (a step past the
        // last re-stages the last tile into the slot nobody reads)
        // (Round 5: whole trips WITHOUT exits, then the last nsteps % NSQ steps straight-line -- with an exit behind every step the first
        //  step of every trip waited vmcnt(0): see the staging waves of pw_gemm_bf16_ws_kernel)
        int st = 0;
        for (; st + NSQ <= nsteps; st += NSQ) {
            stage(st + 1, S1{});
            __syncthreads();
            stage(st + 2, S2{});
            __syncthreads();
            if constexpr (NSQ == 4) {
                stage(st + 3, S3{});
                __syncthreads();
            }
            stage(st + NSQ, S0{});
            __syncthreads();
        }
        if (st < nsteps) {
            stage(st + 1, S1{});
            __syncthreads();
            if (st + 1 < nsteps) {
                stage(st + 2, S2{});
                __syncthreads();
                if constexpr (NSQ == 4) {
                    if (st + 2 < nsteps) {
                        stage(st + 3, S3{});
                        __syncthreads();
                    }
                }
            }
        }
#undef WS_SB
        return;
    }

    // ---------------------------------------------------- matrix waves: the plain operand + MFMA ----------------------------------------------------
    const int wm = wave / NX, wn = wave % NX;
    const int prow = tid >> 3, pch = tid & 7;               // piece i: row prow + 64 i (same swizzle key), chunk pch
    const int prow0 = PG ? m0 : n0, prows = PG ? M : K;
    const float* pp = PG ? p.G : p.X;
    unsigned char (*Ps)[256 * 128] = PG ? reinterpret_cast<unsigned char (*)[256 * 128]>(As) : reinterpret_cast<unsigned char (*)[256 * 128]>(Bs);
    const int voP = ((prow0 + prow) * P16 + pch * 8) * 2;
    const int stepP = 64 * P16 * 2;
    const int ldsP = bf_off(prow, pch);
    u32x4 rp[2][4];
    auto load_p = [&](int step, auto stg, int i) {
        constexpr int SG = decltype(stg)::value;
        int b, t0;
        step_bt(step, b, t0);
        const __amdgpu_buffer_rsrc_t r = make_rsrc(reinterpret_cast<const u16*>(pp) + (size_t)b * prows * P16, (unsigned)prows * P16 * 2u);
        rp[SG][i] = __builtin_amdgcn_raw_buffer_load_b128(r, voP, t0 * 2 + i * stepP, 0);
    };
    auto piece_out = [&](int step, u32x4 v) {
        if constexpr (TAIL) {
            int b, t0;
            step_bt(step, b, t0);
            if (t0 + BF_BK > T) v = tail_mask(v, t0 + pch * 8);
        }
        return v;
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int lr = lane & 31, lh = lane >> 5;
    const int sw = (lr >> 1) & 7;
    const int rdA0 = (wm * 64 + lr) * 128, rdB0 = (wn * 64 + lr) * 128;
    // step st: fragments from slot st & 1; the plain tile of step st + 1 (registers of stage SG) -> slot (st + 1) & 1, step st + 3 requested
    auto block = [&](int st, auto stg) {
        constexpr int SG = decltype(stg)::value;
        const unsigned char* Ab = As[st & 1];
        const unsigned char* Bb = Bs[st & 1];
        unsigned char* Pd = Ps[(st + 1) & 1] + ldsP;
#pragma unroll
        for (int ks = 0; ks < BF_BK / 16; ++ks) {
            const int co = ((ks * 2 + lh) ^ sw) << 4;
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(Ab + rdA0 + co);
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(Ab + rdA0 + 32 * 128 + co);
            const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(Bb + rdB0 + co);
            const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(Bb + rdB0 + 32 * 128 + co);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            *reinterpret_cast<u32x4*>(Pd + ks * 8192) = piece_out(st + 1, rp[SG][ks]);
            load_p(st + 3, stg, ks);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    using S0 = std::integral_constant<int, 0>; using S1 = std::integral_constant<int, 1>;
#pragma unroll
    for (int i = 0; i < 4; ++i) load_p(0, S0{}, i);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) load_p(1, S1{}, i);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) { *reinterpret_cast<u32x4*>(Ps[0] + ldsP + i * 8192) = piece_out(0, rp[0][i]); load_p(2, S0{}, i); }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();                                       // step 0 is in LDS
    // GRP: behind the last step of a split the partial tile joins the running sum and the accumulators restart from zero.  The
    // splits of wg_span, one behind the other, ARE the walk b-major, t-minor: S <= B ends one every ceil(B / S) utterances (the last
    // may be short, later ones empty), S = B * TS at the ends hi(c) = (c + 1) nt / TS of every utterance's chunks (some empty when
    // nt < TS).  An empty split's slab is zeros and changes no sum.
    constexpr int NRR = GRP ? 4 - RL : 1;                  // running-sum fragments in registers
    f32x16 run[NRR];
    const int per = ((p.B + p.S - 1) / p.S) * sp.ntl, TS = p.S > p.B ? p.S / p.B : 0;
    auto next_fold = [&](int cur) {                        // the first split end behind step cur (wave-uniform)
        if (TS == 0) return min(cur + per, nsteps);
        const int b = cur / sp.ntl, w = cur - b * sp.ntl;
        int c = 0;
        while ((int)((long)(c + 1) * sp.ntl / TS) <= w) ++c;
        return b * sp.ntl + (int)((long)(c + 1) * sp.ntl / TS);
    };
    int fold_at = GRP ? next_fold(0) : 0;
    if constexpr (GRP) {
#pragma unroll
        for (int f = 0; f < NRR; ++f)
#pragma unroll
            for (int r = 0; r < 16; ++r) run[f][r] = 0.f;
#pragma unroll
        for (int f = 0; f < RL * 4; ++f) runs[f * 512 + tid] = f32x4{0.f, 0.f, 0.f, 0.f};    // (a lane's own slots: no barrier)
    }
    auto fold = [&](int done) {
        if constexpr (GRP) {
            if (done != fold_at) return;
            fold_at = next_fold(done);
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                f32x16& a = acc[f >> 1][f & 1];
                if (f < NRR) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) run[f < NRR ? f : 0][r] += a[r];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        f32x4& d = runs[((f - NRR) * 4 + q) * 512 + tid];
                        d += f32x4{a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]};
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) a[r] = 0.f;
            }
        }
    };
    int st = 0;
    for (; st + 1 < nsteps; st += 2) {                     // pairs, then the odd step
        block(st, S1{});
        fold(st + 1);
        __syncthreads();
        block(st + 1, S0{});
        fold(st + 2);
        __syncthreads();
    }
    if (st < nsteps) {
        block(st, S1{});
        fold(st + 1);
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
                float v = acc[i][j][r];
                if constexpr (GRP) {
                    const int f = i * 2 + j;
                    v = f < NRR ? run[f < NRR ? f : 0][r] : runs[((f - NRR) * 4 + (r >> 2)) * 512 + tid][r & 3];
                }
                p.partial[((size_t)s * M + m) * K + k] = v;      // (full tiles only: no bounds tests, no exec-mask branches)
            }
}

template <int GM, int XM, bool TAIL, int IO, int GR, int XR, int NSW>
__global__ __launch_bounds__(512 + 64 * NSW) void pw_wgrad_bf16_ws_kernel(WgParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char As[2][GR * 128];   // [m][t] bf16
    __shared__ __attribute__((aligned(16))) unsigned char Bs[2][XR * 128];   // [k][t] bf16
    int s, mt, ktile;
    wg_work(p, s, mt, ktile);
    pw_wgrad_bf16_ws_body<GM, XM, TAIL, IO, GR, XR, NSW>(p, s, mt, ktile, &As[0][0], &Bs[0][0], nullptr);
}
