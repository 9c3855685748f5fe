// pw_wgrad_group_small_kernel: the grouped backward-weight launch (pointwise_bf16_wgrad_group.h) on a 128 x 128 tile, for weight
// gradients with too few 256 x 128 tiles to give every CU one (the narrow blocks' 256 x 1024: 8 of those, 16 of these).
#pragma once
#include <utility>
#include "pointwise_bf16_wgrad_group.h"

// One workgroup of eight waves (two per SIMD, 64 x 32 of the tile each) carries its tile through the WHOLE contraction in the order
// of the problem's S splits, exactly as pw_wgrad_bf16_ws_body<..., GRP> does: the same v_mfma_f32_32x32x16_bf16 over the same 64-deep
// steps (utterance-major), each split's partial tile accumulated from 0.f and added to a running sum in slab order from 0.f, the
// project gradient's X through the same relu6(xa x + xb) and bf16 rounding, tail columns zeroed in both operands.  An output
// element sees the instruction sequence it sees there, so dW is bit-identical to v100_pw_wgrad_io's.
// No staging waves: every lane copies two 16-byte pieces of each operand per step (rows 64 apart: one swizzle key) through NSTG
// register stages, the pieces of step st + 1 stored and those of step st + 1 + NSTG requested behind the first two k-sub-steps'
// MFMAs.  Accumulators and the running sum both live in registers (32 + 32 of a wave's 256).  LDS: two slots of 2 x 16 KB.
// (Four waves of 64 x 64 were measured too: one wave per SIMD cannot issue a step's ~260 instructions in the time of its 16
// MFMAs -- 237 us for the bench's eight problems against 190 us on eight waves; profiles/wgrad_group2_ab.txt.)
template <class F, int... I>
__device__ __forceinline__ void wgs_static_for(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }

template <int XM, bool TAIL, int NSTG>
__device__ __forceinline__ void pw_wgrad_small_body(const WgGroupProblem& q, const int mt, const int ktile, unsigned char* const smem) {
    unsigned char (*As)[128 * 128] = reinterpret_cast<unsigned char (*)[128 * 128]>(smem);           // [2][m][t] bf16
    unsigned char (*Bs)[128 * 128] = reinterpret_cast<unsigned char (*)[128 * 128]>(smem + 32768);   // [2][k][t] bf16
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;              // 64 x 32 of the tile
    const int m0 = mt * 128, n0 = ktile * 128;
    const int M = q.M, K = q.K, T = q.T, B = q.B, S = q.S;
    const int P16 = pw_pitch16(T, B);
    const int nt = (T + BF_BK - 1) / BF_BK;
    const int nsteps = B * nt;                              // the splits' utterance runs, one behind the other
    // (utterance, t offset) of the next step; the last step repeats (an unconditional, redundant load and store into the slot
    // nobody reads)
    auto advance = [&](int& b, int& t0) {
        if (t0 + BF_BK < nt * BF_BK) t0 += BF_BK;
        else if (b + 1 < B) { ++b; t0 = 0; }
    };
    // contraction indices tb + e >= T of a 16-byte piece -> zero
    auto tail_mask = [&](u32x4 v, int tb) {
        const int nv = T - tb;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] &= nv > 2 * j + 1 ? 0xffffffffu : (nv > 2 * j ? 0xffffu : 0u);
        return v;
    };
    const int prow = tid >> 3, pch = tid & 7;               // piece i: row prow + 64 i, chunk pch
    const int voG = ((m0 + prow) * P16 + pch * 8) * 2, voX = ((n0 + prow) * P16 + pch * 8) * 2;
    const int stepR = 64 * P16 * 2;
    const int ldsP = bf_off(prow, pch);
    float ca[2], cb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        ca[i] = XM != PW_X_NONE ? q.xa[n0 + prow + 64 * i] : 1.f;
        cb[i] = XM != PW_X_NONE ? q.xb[n0 + prow + 64 * i] : 0.f;
    }
    u32x4 rg[NSTG][2], rx[NSTG][2];
    auto load = [&](auto stg, int i, int b, int t0) {
        constexpr int SG = decltype(stg)::value;
        const __amdgpu_buffer_rsrc_t r1 = make_rsrc(reinterpret_cast<const u16*>(q.G) + (size_t)b * M * P16, (unsigned)M * P16 * 2u);
        const __amdgpu_buffer_rsrc_t r2 = make_rsrc(reinterpret_cast<const u16*>(q.X) + (size_t)b * K * P16, (unsigned)K * P16 * 2u);
        rg[SG][i] = __builtin_amdgcn_raw_buffer_load_b128(r1, voG, t0 * 2 + i * stepR, 0);
        rx[SG][i] = __builtin_amdgcn_raw_buffer_load_b128(r2, voX, t0 * 2 + i * stepR, 0);
    };
    // piece i of the step at t0 (registers of stage SG) -> LDS slot
    auto store = [&](auto stg, int i, int slot, int t0) {
        constexpr int SG = decltype(stg)::value;
        u32x4 g = rg[SG][i], o = rx[SG][i];
        if constexpr (XM != PW_X_NONE) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = relu6f(fmaf(pw_bf16_at(o, e), ca[i], cb[i]));
            o[0] = pack_bf16(v[0], v[1]); o[1] = pack_bf16(v[2], v[3]); o[2] = pack_bf16(v[4], v[5]); o[3] = pack_bf16(v[6], v[7]);
        }
        if constexpr (TAIL) {
            if (t0 + BF_BK > T) { g = tail_mask(g, t0 + pch * 8); o = tail_mask(o, t0 + pch * 8); }
        }
        *reinterpret_cast<u32x4*>(As[slot] + ldsP + i * 8192) = g;
        *reinterpret_cast<u32x4*>(Bs[slot] + ldsP + i * 8192) = o;
    };
    f32x16 acc[2], run[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = run[i][r] = 0.f;
    const int lr = lane & 31, lh = lane >> 5;
    const int sw = (lr >> 1) & 7;
    const int rdA0 = (wm * 64 + lr) * 128, rdB0 = (wn * 32 + lr) * 128;
    int lb = 0, lt = 0;                                     // the step the next loads request
    int wb = 0, wt = 0;                                     // the step the next stores write
    // step st: fragments from slot st & 1 (those of k-sub-step ks + 1 requested ahead of the MFMAs of ks); the tile of step st + 1
    // (registers of stage SG) -> slot (st + 1) & 1, step st + 1 + NSTG requested
    auto block = [&](int st, auto stg) {
        const unsigned char* Ab = As[st & 1] + rdA0;
        const unsigned char* Bb = Bs[st & 1] + rdB0;
        bf16x8 a[2][2], b[2];
        auto frags = [&](int ks, int f) {
            const int co = ((ks * 2 + lh) ^ sw) << 4;
            a[f][0] = *reinterpret_cast<const bf16x8*>(Ab + co);
            a[f][1] = *reinterpret_cast<const bf16x8*>(Ab + 32 * 128 + co);
            b[f] = *reinterpret_cast<const bf16x8*>(Bb + co);
        };
        frags(0, 0);
#pragma unroll
        for (int ks = 0; ks < BF_BK / 16; ++ks) {
            const int f = ks & 1;
            if (ks + 1 < BF_BK / 16) frags(ks + 1, f ^ 1);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[f][0], b[f], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[f][1], b[f], acc[1], 0, 0, 0);
            if (ks < 2) {
                store(stg, ks, (st + 1) & 1, wt);
                load(stg, ks, lb, lt);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        advance(lb, lt);
        advance(wb, wt);
    };
    using S0 = std::integral_constant<int, 0>;
    const auto stages = std::make_integer_sequence<int, NSTG>{};
    wgs_static_for([&](auto sg) {                          // steps 0 .. NSTG - 1 requested
#pragma unroll
        for (int i = 0; i < 2; ++i) load(sg, i, lb, lt);
        advance(lb, lt);
        __builtin_amdgcn_sched_barrier(0);
    }, stages);
#pragma unroll
    for (int i = 0; i < 2; ++i) { store(S0{}, i, 0, wt); load(S0{}, i, lb, lt); }
    advance(lb, lt);
    advance(wb, wt);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();                                       // step 0 is in LDS
    // Behind the last step of a split the partial tile joins the running sum and the accumulators restart from zero
    // (pw_wgrad_bf16_ws_body: S <= B ends a split every ceil(B / S) utterances, S = B * TS at the ends (c + 1) nt / TS of every
    // utterance's chunks; an empty split's slab is zeros and changes no sum).
    const int per = ((B + S - 1) / S) * nt, TS = S > B ? S / B : 0;
    auto next_fold = [&](int cur) {                        // the first split end behind step cur (wave-uniform)
        if (TS == 0) return min(cur + per, nsteps);
        const int b = cur / nt, w = cur - b * nt;
        int c = 0;
        while ((int)((long)(c + 1) * nt / TS) <= w) ++c;
        return b * nt + (int)((long)(c + 1) * nt / TS);
    };
    int fold_at = next_fold(0);
    auto fold = [&](int done) {
        if (done != fold_at) return;
        fold_at = next_fold(done);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) { run[i][r] += acc[i][r]; acc[i][r] = 0.f; }
    };
    int st = 0;
    for (; st + NSTG <= nsteps; st += NSTG)                // NSTG steps a trip (the stages are named at compile time), then the rest
        wgs_static_for([&](auto i) {
            block(st + i, std::integral_constant<int, (i + 1) % NSTG>{});
            fold(st + i + 1);
            __syncthreads();
        }, stages);
    wgs_static_for([&](auto i) {
        if (st + i < nsteps) {
            block(st + i, std::integral_constant<int, (i + 1) % NSTG>{});
            fold(st + i + 1);
            __syncthreads();
        }
    }, stages);
    const int col = lane & 31, half = lane >> 5;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const int k = n0 + wn * 32 + col;
            q.dW[(size_t)m * K + k] = run[i][r];           // (full tiles only: no bounds tests)
        }
}

// Workgroup 8 j + x is slot j of XCD x, as in pw_wgrad_group_kernel: the tiles of one problem sit on one XCD and share its L2.
#define WG_SMALL_STAGES 4         // register stages of the operand copies (measured: 2 / 4 / 6 within 2 % of each other at 8 waves)
template <bool TAIL>
__global__ __launch_bounds__(512) void pw_wgrad_group_small_kernel(WgGroupParams g) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[65536];
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
    int pi = -1;
    for (int i = 0; i < g.n; ++i)
        if (g.pr[i].xcd == x && j >= g.pr[i].slot0 && j < g.pr[i].slot0 + g.pr[i].ntiles) pi = i;
    if (pi < 0) return;
    const WgGroupProblem& q = g.pr[pi];
    const int t = j - q.slot0, nkt = q.K / 128;
    if (q.x_mode == PW_X_AFFINE_RELU6) pw_wgrad_small_body<PW_X_AFFINE_RELU6, TAIL, WG_SMALL_STAGES>(q, t / nkt, t % nkt, smem);
    else pw_wgrad_small_body<PW_X_NONE, TAIL, WG_SMALL_STAGES>(q, t / nkt, t % nkt, smem);
}
