// K15: the recurrence of a (bidirectional) LSTM layer -- nn.LSTM over packed, ragged sequences (_asr_v2.py:32-34, 46).
//
// The input projection x W_ih^T + b_ih and the weight / data gradients of W_ih and W_hh are K1 GEMMs (v100_pw_gemm /
// v100_pw_wgrad); this file is only the sequential part.  Layouts (fp32 unless stated):
//   xproj  [ndir][B][4H][T]   x W_ih^T + b_ih, gate order i, f, g, o (nn.LSTM's)
//   y      [B][ndir H][T]     the layer output, 0 at t >= len_b (pad_packed_sequence)
//   h_n/c_n, dh_n/dc_n        [ndir][B][H]
//   act    [ndir][T][B][4H]   training only: i, f, g, o after their nonlinearities, indexed by STEP s
//   cs     [ndir][T][B][H]    training only: the cell state after step s
//   hprev  [ndir][B][H][T]    training only: the h that step t read (0 at a sequence's first step): the X of the dW_hh GEMM
//   dgates [ndir][B][4H][T]   backward output: d(pre-activation gates), 0 at t >= len_b
// Step s of direction 0 is t = s, of direction 1 t = len_b - 1 - s; a sequence is active at steps s < len_b.
//
// Work split.  A group = (direction, 16-sequence batch slice); it has G = H / U workgroups, each owning U hidden
// units -- all four gate rows of them in the forward, so the cell update is local.  Per step a workgroup computes
// D[M][16] = A[M][K] * B[16][K]^T on the matrix cores, A its slice of W_hh (forward: the 4U gate rows, K = H; backward: W_hh^T's U rows,
// K = 4H) staged ONCE into LDS, B the previous step's h (forward) or dgates (backward) of the whole group, read from a two-slot
// exchange ring in global memory.  Two slots suffice: a workgroup writes slot s&1 (last read as step s-2's output) only after every
// workgroup of its group has published step s-1, and each publishes step s-1 only after its own reads of step s-2's output.
//
// Two launch forms of ONE kernel body, steps [s0, s1):
//   step form        s1 = s0 + 1, one launch per step; the launch boundary orders the steps (no polling at all);
//   persistent form  all steps in one launch; workgroups hand the ring slot to each other with the counter form of the agent-scope
//                    release / acquire recipe (cdna_hip_programming Guideline 16): payload plain-stored, every wave drains, barrier,
//                    one lane: release fence, drain, relaxed agent fetch_add on the group's counter; the consumer polls that word
//                    relaxed (bounded), one acquire fence, drain, barrier, then every wave loads.  Every spin is bounded by a time limit
//                    and a give-up word in device memory (sync[0] = step + 1) that the host checks after the call.
// The arithmetic of a step does not depend on the form or on placement, so the two forms are bit-identical.
#include "common.h"
#include "voice100_hip.h"

namespace {

constexpr int LS_THREADS = 256;
constexpr int LS_NB = 16;                    // sequences per group: the MFMA's N
constexpr int LS_LDS_CAP = 160 * 1024;
constexpr int LS_MAX_GRID = 128;             // the persistent form stays well below the 256 CUs of the chip
constexpr unsigned long long LS_GIVEUP_TICKS = 200ull * 1000 * 1000;   // 2 s of the 100 MHz s_memrealtime clock per wait
constexpr int LS_SYNC_HEAD = 4;              // sync[0] give-up word, sync[4 + group] the groups' counters

typedef __attribute__((address_space(1))) unsigned gu32;
typedef _Float16 ls_f16x8 __attribute__((ext_vector_type(8)));

struct Geo {
    int U, G, M, K, pitch, elt, TW, KW, wbytes, lds, wlds;
};

// U in {32, 16}: the largest whose W_hh slice and partial-sum buffer fit the LDS; if neither does (fp32 at H > 512), U = 16 with the
// A operand read from global memory (step form only).
static Geo ls_geometry(int H, int fmt, int backward) {
    Geo g{};
    g.elt = fmt ? 2 : 4;
    for (int U : {32, 16}) {
        if (H % U) continue;
        g.U = U;
        g.G = H / U;
        g.M = backward ? U : 4 * U;
        g.K = backward ? 4 * H : H;
        const int ch = fmt ? 32 : 16;
        const int kp = (g.K + ch - 1) / ch * ch;
        g.pitch = kp + 16 / g.elt;                            // one 16-byte slot of padding per row (LDS banks)
        g.TW = g.M / 16 < 4 ? g.M / 16 : 4;
        g.KW = 4 / g.TW;
        g.wbytes = g.M * g.pitch * g.elt;
        const int red = g.KW * g.M * LS_NB * 4;
        g.lds = g.wbytes + red + 16;
        g.wlds = 1;
        if (g.lds <= LS_LDS_CAP) return g;
    }
    g.U = 16; g.G = H / 16; g.M = backward ? 16 : 64; g.K = backward ? 4 * H : H;
    const int ch = fmt ? 32 : 16;
    g.pitch = (g.K + ch - 1) / ch * ch + 16 / g.elt;
    g.TW = g.M / 16 < 4 ? g.M / 16 : 4;
    g.KW = 4 / g.TW;
    g.wbytes = g.M * g.pitch * g.elt;
    g.lds = g.KW * g.M * LS_NB * 4 + 16;
    g.wlds = 0;
    return g;
}

struct LsParams {
    const float* xin;        // forward: xproj; backward: dy
    const void* w;           // prepared W_hh slices [ndir][G][M][pitch]
    const float* b0;         // forward: b_hh of direction 0 / 1 (may be NULL); backward: dh_n / dc_n (may be NULL)
    const float* b1;
    const int* lens;
    float* out;              // forward: y; backward: dgates
    float* hn;
    float* cn;
    float* act;
    float* cs;
    float* hprev;
    float* xch;              // exchange ring [ndir][2][B][XK]
    float* st;               // per-(unit, sequence) carried state [ndir][B][H] (c forward, dc backward)
    unsigned* sync;
    int B, T, H, ndir, U, G, M, K, pitch, TW, KW, wbytes, nslices, s0, s1, persistent;
};

__device__ __forceinline__ float ls_sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }
__device__ __forceinline__ float ls_tanh(float x) { return 2.0f / (1.0f + __expf(-2.0f * x)) - 1.0f; }

// D[M][16] partial products: wave w takes row tiles tw, tw + TW and K chunks kw, kw + KW, ...; red[kw][row][16] then holds its part.
// The reduction over kw is done by the caller in fixed order, so every output sums its products in one order whatever the form.
template <int FMT, bool WLDS>
__device__ __forceinline__ void ls_product(const LsParams& p, const char* A, const float* Bsrc, int nvalid, float* red,
                                           int wave, int lane) {
    const int nt = p.M / 16, tw = wave % p.TW, kw = wave / p.TW;
    const int r = lane & 15, q = lane >> 4;
    const bool bval = r < nvalid;
    const float* brow = Bsrc + (size_t)(bval ? r : 0) * p.K;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if constexpr (FMT != 0) {
        const int nc = (p.K + 31) / 32;
        for (int c = kw; c < nc; c += p.KW) {
            const int k = c * 32 + 8 * q;
            f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
            if (bval && k < p.K) { v0 = *(const f32x4*)(brow + k); v1 = *(const f32x4*)(brow + k + 4); }
            const unsigned u0 = pack16<FMT == 2>(v0[0], v0[1]), u1 = pack16<FMT == 2>(v0[2], v0[3]);
            const unsigned u2 = pack16<FMT == 2>(v1[0], v1[1]), u3 = pack16<FMT == 2>(v1[2], v1[3]);
            typedef unsigned ls_u32x4 __attribute__((ext_vector_type(4)));
            const ls_u32x4 bu = {u0, u1, u2, u3};
            const bf16x8 bb = __builtin_bit_cast(bf16x8, bu);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int tile = tw + i * p.TW;
                if (tile < nt) {
                    const bf16x8 a = *(const bf16x8*)(A + ((size_t)(tile * 16 + r) * p.pitch + k) * 2);
                    if constexpr (FMT == 2)
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(ls_f16x8, a), __builtin_bit_cast(ls_f16x8, bb), acc[i], 0, 0, 0);
                    else
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb, acc[i], 0, 0, 0);
                }
            }
        }
    } else {
        const int nc = p.K / 16;
        for (int c = kw; c < nc; c += p.KW) {
            const int k = c * 16 + 4 * q;                   // lane (r, q) supplies k + 0..3 to the chunk's four MFMAs
            f32x4 b = {0.f, 0.f, 0.f, 0.f};
            if (bval) b = *(const f32x4*)(brow + k);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int tile = tw + i * p.TW;
                if (tile < nt) {
                    const f32x4 a = *(const f32x4*)(A + ((size_t)(tile * 16 + r) * p.pitch + k) * 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc[i], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int tile = tw + i * p.TW;
        if (tile < nt) {
#pragma unroll
            for (int j = 0; j < 4; ++j) red[((size_t)kw * p.M + tile * 16 + 4 * q + j) * LS_NB + r] = acc[i][j];
        }
    }
}

__device__ __forceinline__ float ls_red_sum(const LsParams& p, const float* red, int row, int n) {
    float v = red[row * LS_NB + n];
    for (int k = 1; k < p.KW; ++k) v += red[((size_t)k * p.M + row) * LS_NB + n];
    return v;
}

// Publish this workgroup's part of step s: every wave drains its stores, barrier, one lane releases and counts.
__device__ __forceinline__ void ls_publish(unsigned* cnt, int tid) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add((gu32*)cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Wait until the group's counter reaches `target`; false (for the whole workgroup) if the wait gave up.
__device__ __forceinline__ bool ls_wait(unsigned* cnt, unsigned target, unsigned* giveup, unsigned code, int tid, int* flag) {
    if (tid == 0) {
        int ok = 1;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load((gu32*)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            if (__hip_atomic_load((gu32*)giveup, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) { ok = 0; break; }
            if (__builtin_amdgcn_s_memrealtime() - t0 > LS_GIVEUP_TICKS) {
                unsigned zero = 0u;
                __hip_atomic_compare_exchange_strong((gu32*)giveup, &zero, code, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
                ok = 0;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        if (ok) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *flag = ok;
    }
    __syncthreads();
    return *flag != 0;
}

struct LsPlace { int dir, n0, g, grp; };

__device__ __forceinline__ LsPlace ls_place(const LsParams& p) {
    int wg = blockIdx.x;
    const int n = gridDim.x;
    if ((n & 7) == 0) wg = (wg & 7) * (n >> 3) + (wg >> 3);      // a group's workgroups share blockIdx % 8 (one XCD): speed only
    LsPlace pl;
    pl.grp = wg / p.G;
    pl.g = wg % p.G;
    pl.dir = pl.grp / p.nslices;
    pl.n0 = (pl.grp % p.nslices) * LS_NB;
    return pl;
}

template <bool WLDS>
__device__ __forceinline__ const char* ls_stage_w(const LsParams& p, const LsPlace& pl, char* lds, int tid) {
    const char* src = (const char*)p.w + (size_t)(pl.dir * p.G + pl.g) * p.wbytes;
    if constexpr (!WLDS) return src;
    for (int i = tid; i < p.wbytes / 16; i += LS_THREADS) ((f32x4*)lds)[i] = ((const f32x4*)src)[i];
    __syncthreads();
    return lds;
}

template <int FMT, bool WLDS>
__global__ __launch_bounds__(LS_THREADS, 1) void lstm_fwd_kernel(LsParams p) {
    extern __shared__ __attribute__((aligned(16))) char ls_smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const LsPlace pl = ls_place(p);
    const int H = p.H, B = p.B, T = p.T, U = p.U, H4 = 4 * H;
    float* red = (float*)(ls_smem + (WLDS ? p.wbytes : 0));
    int* flag = (int*)(ls_smem + (WLDS ? p.wbytes : 0) + p.KW * p.M * LS_NB * 4);
    const char* A = ls_stage_w<WLDS>(p, pl, ls_smem, tid);
    const int nvalid = B - pl.n0 < LS_NB ? B - pl.n0 : LS_NB;
    const int nitem = U * LS_NB / LS_THREADS;                        // 1 (U = 16) or 2 (U = 32) (unit, sequence) items per thread
    int len[2], bq[2];
    float bias[2][4];
    for (int it = 0; it < 2; ++it) {
        const int e = tid + it * LS_THREADS, j = e % U, n = e / U, b = pl.n0 + n;
        bq[it] = (it < nitem && b < B) ? b : -1;
        len[it] = bq[it] >= 0 ? min(max(p.lens[b], 0), T) : 0;          // lengths outside [0, T] cannot address past the tensors
        const float* bh = pl.dir ? p.b1 : p.b0;
        for (int q = 0; q < 4; ++q) bias[it][q] = (bh && bq[it] >= 0) ? bh[q * H + pl.g * U + j] : 0.f;
    }
    unsigned* cnt = p.sync + LS_SYNC_HEAD + pl.grp;
    for (int s = p.s0; s < p.s1; ++s) {
        float xp[2][4];
        for (int it = 0; it < 2; ++it) {                              // the input projection does not depend on the recurrence: load first
            const int b = bq[it], j = (tid + it * LS_THREADS) % U, u = pl.g * U + j;
            if (b >= 0 && s < len[it]) {
                const int t = pl.dir ? len[it] - 1 - s : s;
                const float* xr = p.xin + ((size_t)(pl.dir * B + b) * H4 + u) * T + t;
                for (int q = 0; q < 4; ++q) xp[it][q] = xr[(size_t)q * H * T];
            } else {
                for (int q = 0; q < 4; ++q) xp[it][q] = 0.f;
            }
        }
        if (s > 0) {
            if (p.persistent && s > p.s0 && !ls_wait(cnt, (unsigned)(p.G * s), p.sync, (unsigned)s + 1u, tid, flag)) return;
            const float* hsrc = p.xch + ((size_t)(pl.dir * 2 + ((s - 1) & 1)) * B + pl.n0) * H;
            ls_product<FMT, WLDS>(p, A, hsrc, nvalid, red, wave, lane);
            __syncthreads();
        }
        for (int it = 0; it < 2; ++it) {
            const int b = bq[it];
            if (b < 0) continue;
            const int e = tid + it * LS_THREADS, j = e % U, n = e / U, u = pl.g * U + j;
            float* hx = p.xch + ((size_t)(pl.dir * 2 + (s & 1)) * B + b) * H + u;
            const size_t sidx = (size_t)(pl.dir * B + b) * H + u;
            if (s < len[it]) {
                const int t = pl.dir ? len[it] - 1 - s : s;
                float z[4];
                for (int q = 0; q < 4; ++q) z[q] = xp[it][q] + bias[it][q] + (s > 0 ? ls_red_sum(p, red, q * U + j, n) : 0.f);
                const float gi = ls_sigmoid(z[0]), gf = ls_sigmoid(z[1]), gg = ls_tanh(z[2]), go = ls_sigmoid(z[3]);
                const float cp = s > 0 ? p.st[sidx] : 0.f;
                const float c = gf * cp + gi * gg;
                const float h = go * ls_tanh(c);
                const float hp = s > 0 ? p.xch[((size_t)(pl.dir * 2 + ((s - 1) & 1)) * B + b) * H + u] : 0.f;
                *hx = h;
                p.st[sidx] = c;
                p.out[((size_t)(b * p.ndir + pl.dir) * H + u) * T + t] = h;
                if (p.act) {
                    float* a = p.act + ((size_t)(pl.dir * T + s) * B + b) * H4 + u;
                    a[0] = gi; a[H] = gf; a[2 * H] = gg; a[3 * H] = go;
                    p.cs[((size_t)(pl.dir * T + s) * B + b) * H + u] = c;
                    p.hprev[sidx * T + t] = hp;
                }
                if (s == len[it] - 1) { p.hn[sidx] = h; p.cn[sidx] = c; }
            } else {
                *hx = 0.f;
                p.out[((size_t)(b * p.ndir + pl.dir) * H + u) * T + s] = 0.f;
                if (p.act) p.hprev[sidx * T + s] = 0.f;
            }
        }
        if (p.persistent && s + 1 < p.s1) ls_publish(cnt, tid);
        else __syncthreads();
    }
}

template <int FMT, bool WLDS>
__global__ __launch_bounds__(LS_THREADS, 1) void lstm_bwd_kernel(LsParams p) {
    extern __shared__ __attribute__((aligned(16))) char ls_smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const LsPlace pl = ls_place(p);
    const int H = p.H, B = p.B, T = p.T, U = p.U, H4 = 4 * H;
    float* red = (float*)(ls_smem + (WLDS ? p.wbytes : 0));
    int* flag = (int*)(ls_smem + (WLDS ? p.wbytes : 0) + p.KW * p.M * LS_NB * 4);
    const char* A = ls_stage_w<WLDS>(p, pl, ls_smem, tid);
    const int nvalid = B - pl.n0 < LS_NB ? B - pl.n0 : LS_NB;
    const int nitem = U * LS_NB / LS_THREADS;
    int len[2], bq[2];
    for (int it = 0; it < 2; ++it) {
        const int e = tid + it * LS_THREADS, n = e / U, b = pl.n0 + n;
        bq[it] = (it < nitem && b < B) ? b : -1;
        len[it] = bq[it] >= 0 ? min(max(p.lens[b], 0), T) : 0;          // lengths outside [0, T] cannot address past the tensors
    }
    unsigned* cnt = p.sync + LS_SYNC_HEAD + pl.grp;
    for (int s = p.s1 - 1; s >= p.s0; --s) {
        float dyv[2];
        for (int it = 0; it < 2; ++it) {
            const int b = bq[it], u = pl.g * U + (tid + it * LS_THREADS) % U;
            dyv[it] = 0.f;
            if (b >= 0 && s < len[it]) {
                const int t = pl.dir ? len[it] - 1 - s : s;
                dyv[it] = p.xin[((size_t)(b * p.ndir + pl.dir) * H + u) * T + t];
            }
        }
        if (s + 1 < T) {
            if (p.persistent && s + 1 < p.s1 &&
                !ls_wait(cnt, (unsigned)(p.G * (p.s1 - 1 - s)), p.sync, (unsigned)s + 1u, tid, flag)) return;
            const float* gsrc = p.xch + ((size_t)(pl.dir * 2 + ((s + 1) & 1)) * B + pl.n0) * H4;
            ls_product<FMT, WLDS>(p, A, gsrc, nvalid, red, wave, lane);
            __syncthreads();
        }
        for (int it = 0; it < 2; ++it) {
            const int b = bq[it];
            if (b < 0) continue;
            const int e = tid + it * LS_THREADS, j = e % U, n = e / U, u = pl.g * U + j;
            float* gx = p.xch + ((size_t)(pl.dir * 2 + (s & 1)) * B + b) * H4 + u;
            float* dg = p.out + ((size_t)(pl.dir * B + b) * H4 + u) * T;
            const size_t sidx = (size_t)(pl.dir * B + b) * H + u;
            if (s < len[it]) {
                const int t = pl.dir ? len[it] - 1 - s : s;
                const bool last = s == len[it] - 1;
                const float dhr = last ? (p.b0 ? p.b0[sidx] : 0.f) : ls_red_sum(p, red, j, n);
                const float dcr = last ? (p.b1 ? p.b1[sidx] : 0.f) : p.st[sidx];
                const float dh = dyv[it] + dhr;
                const float* a = p.act + ((size_t)(pl.dir * T + s) * B + b) * H4 + u;
                const float gi = a[0], gf = a[H], gg = a[2 * H], go = a[3 * H];
                const float c = p.cs[((size_t)(pl.dir * T + s) * B + b) * H + u];
                const float cp = s > 0 ? p.cs[((size_t)(pl.dir * T + s - 1) * B + b) * H + u] : 0.f;
                const float tc = ls_tanh(c);
                const float dc = dcr + dh * go * (1.f - tc * tc);
                float z[4];
                z[0] = dc * gg * gi * (1.f - gi);
                z[1] = dc * cp * gf * (1.f - gf);
                z[2] = dc * gi * (1.f - gg * gg);
                z[3] = dh * tc * go * (1.f - go);
                p.st[sidx] = dc * gf;
                for (int q = 0; q < 4; ++q) { gx[q * H] = z[q]; dg[(size_t)q * H * T + t] = z[q]; }
            } else {
                for (int q = 0; q < 4; ++q) { gx[q * H] = 0.f; dg[(size_t)q * H * T + s] = 0.f; }
            }
        }
        if (p.persistent && s > p.s0) ls_publish(cnt, tid);
        else __syncthreads();
    }
}

// prepared W_hh: forward [dir][g][4U rows: gate q, unit j][pitch] = W_hh[q H + g U + j][k]; backward [dir][g][U rows][pitch] =
// W_hh[k][g U + j] (W_hh^T); zero beyond K; fp32, bf16 or fp16 elements
template <int FMT>
__global__ void lstm_prep_kernel(const float* w0, const float* w1, int H, int U, int G, int M, int K, int pitch, int backward,
                                 void* out, long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i % pitch);
        const long long rowid = i / pitch;
        const int row = (int)(rowid % M);
        const int g = (int)((rowid / M) % G);
        const int dir = (int)(rowid / ((long long)M * G));
        const float* w = dir ? w1 : w0;
        float v = 0.f;
        if (k < K) {
            if (backward) v = w[(size_t)k * H + g * U + row];
            else v = w[(size_t)((row / U) * H + g * U + row % U) * H + k];
        }
        if constexpr (FMT == 0) ((float*)out)[i] = v;
        else if constexpr (FMT == 1) ((u16*)out)[i] = f2bf(v);
        else ((u16*)out)[i] = f2h(v);
    }
}

static int ls_shape_ok(int B, int T, int H, int ndir) {
    return B >= 1 && T >= 1 && H >= 16 && H <= 1024 && H % 16 == 0 && (ndir == 1 || ndir == 2);
}

static int ls_nslices(int B) { return (B + LS_NB - 1) / LS_NB; }

template <typename K>
static bool ls_resident(K kernel, int grid, int lds) {
    if (grid > LS_MAX_GRID) return false;
    int dev = 0, cus = 0;                                              // the CURRENT device's CU count, on every call
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return false;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, LS_THREADS, lds) != hipSuccess) return false;
    return per_cu >= 1 && grid <= per_cu * cus;
}

template <typename K>
static int ls_launch(K kernel, LsParams p, const Geo& g, int persistent, bool backward, hipStream_t st) {
    const int grid = p.ndir * p.nslices * g.G;
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, g.lds) != hipSuccess) return V100_ERR_LAUNCH;
    const int nwords = LS_SYNC_HEAD + p.ndir * p.nslices;
    const size_t sync_bytes = (size_t)(nwords + 3) / 4 * 16;
    if (hipMemsetAsync(p.sync, 0, sync_bytes, st) != hipSuccess) return V100_ERR_LAUNCH;
    if (persistent && g.wlds && ls_resident(kernel, grid, g.lds)) {
        p.persistent = 1;
        p.s0 = 0;
        p.s1 = p.T;
        V100_GGL(kernel, dim3(grid), dim3(LS_THREADS), g.lds, st, p);
        return v100_launch_status();
    }
    p.persistent = 0;
    for (int i = 0; i < p.T; ++i) {
        const int s = backward ? p.T - 1 - i : i;
        p.s0 = s;
        p.s1 = s + 1;
        V100_GGL(kernel, dim3(grid), dim3(LS_THREADS), g.lds, st, p);
        if (hipPeekAtLastError() != hipSuccess) return v100_launch_status();
    }
    return v100_launch_status();
}

static LsParams ls_params(const Geo& g, int B, int T, int H, int ndir) {
    LsParams p{};
    p.B = B; p.T = T; p.H = H; p.ndir = ndir;
    p.U = g.U; p.G = g.G; p.M = g.M; p.K = g.K; p.pitch = g.pitch; p.TW = g.TW; p.KW = g.KW; p.wbytes = g.wbytes;
    p.nslices = ls_nslices(B);
    return p;
}

}  // namespace

extern "C" long long v100_lstm_weight_bytes(int H, int ndir, int use_bf16, int backward) {
    if (H < 16 || H > 1024 || H % 16 || ndir < 1 || ndir > 2) return 0;
    const Geo g = ls_geometry(H, use_bf16, backward);
    return (long long)ndir * g.G * g.wbytes;
}

extern "C" int v100_lstm_geometry(int H, int use_bf16, int backward, int* out) {
    if (!out) return V100_ERR_NULL;
    if (H < 16 || H > 1024 || H % 16 || use_bf16 < 0 || use_bf16 > 2 || (backward && use_bf16 == 2)) return V100_ERR_SHAPE;
    const Geo g = ls_geometry(H, use_bf16, backward ? 1 : 0);
    out[0] = g.U; out[1] = g.G; out[2] = g.wlds; out[3] = g.lds;
    return V100_OK;
}

extern "C" long long v100_lstm_ws_bytes(int B, int H, int ndir, int backward) {
    if (B < 1 || H < 16 || ndir < 1 || ndir > 2) return 0;
    const long long xk = backward ? 4LL * H : H;
    return ((long long)ndir * 2 * B * xk + (long long)ndir * B * H) * 4;
}

extern "C" int v100_lstm_sync_words(int B, int ndir) {
    const int n = LS_SYNC_HEAD + ndir * ls_nslices(B);
    return (n + 3) / 4 * 4;
}

extern "C" int v100_lstm_persistent_ok(int B, int H, int ndir, int use_bf16, int backward) {
    if (!ls_shape_ok(B, 1, H, ndir) || use_bf16 < 0 || use_bf16 > 2) return 0;
    const Geo g = ls_geometry(H, use_bf16, backward);
    if (!g.wlds) return 0;
    const int grid = ndir * ls_nslices(B) * g.G;
    const void* k = nullptr;
    if (backward) k = use_bf16 ? (const void*)lstm_bwd_kernel<1, true> : (const void*)lstm_bwd_kernel<0, true>;
    else k = use_bf16 == 2 ? (const void*)lstm_fwd_kernel<2, true> : use_bf16 ? (const void*)lstm_fwd_kernel<1, true>
                                                                               : (const void*)lstm_fwd_kernel<0, true>;
    if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, g.lds) != hipSuccess) return 0;
    return ls_resident(k, grid, g.lds) ? 1 : 0;
}

extern "C" int v100_lstm_weight_prep(const float* w_hh0, const float* w_hh1, int H, int ndir, int use_bf16, int backward,
                                     void* out, void* stream) {
    if (!w_hh0 || !out || (ndir == 2 && !w_hh1)) return V100_ERR_NULL;
    if (H < 16 || H > 1024 || H % 16 || ndir < 1 || ndir > 2 || use_bf16 < 0 || use_bf16 > 2 || (backward && use_bf16 == 2))
        return V100_ERR_SHAPE;
    const Geo g = ls_geometry(H, use_bf16, backward);
    const long long total = (long long)ndir * g.G * g.M * g.pitch;
    const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipStream_t st = (hipStream_t)stream;
    if (use_bf16 == 0) V100_GGL(lstm_prep_kernel<0>, dim3(grid), dim3(256), 0, st, w_hh0, w_hh1, H, g.U, g.G, g.M, g.K, g.pitch, backward, out, total);
    else if (use_bf16 == 1) V100_GGL(lstm_prep_kernel<1>, dim3(grid), dim3(256), 0, st, w_hh0, w_hh1, H, g.U, g.G, g.M, g.K, g.pitch, backward, out, total);
    else V100_GGL(lstm_prep_kernel<2>, dim3(grid), dim3(256), 0, st, w_hh0, w_hh1, H, g.U, g.G, g.M, g.K, g.pitch, backward, out, total);
    return v100_launch_status();
}

extern "C" int v100_lstm_fwd(const float* xproj, const void* w_prep, const float* b_hh0, const float* b_hh1, const int* lens,
                             float* y, float* h_n, float* c_n, float* act, float* cs, float* hprev, void* ws, unsigned* sync,
                             int B, int T, int H, int ndir, int use_bf16, int persistent, void* stream) {
    if (!xproj || !w_prep || !lens || !y || !h_n || !c_n || !ws || !sync) return V100_ERR_NULL;
    if (!ls_shape_ok(B, T, H, ndir) || use_bf16 < 0 || use_bf16 > 2) return V100_ERR_SHAPE;
    const int saved = (act != nullptr) + (cs != nullptr) + (hprev != nullptr);
    if (saved != 0 && saved != 3) return V100_ERR_SHAPE;
    if (saved && use_bf16 == 2) return V100_ERR_SHAPE;             // fp16 is an inference precision
    const Geo g = ls_geometry(H, use_bf16, 0);
    LsParams p = ls_params(g, B, T, H, ndir);
    p.xin = xproj; p.w = w_prep; p.b0 = b_hh0; p.b1 = b_hh1; p.lens = lens; p.out = y; p.hn = h_n; p.cn = c_n;
    p.act = act; p.cs = cs; p.hprev = hprev; p.sync = sync;
    p.xch = (float*)ws;
    p.st = p.xch + (size_t)ndir * 2 * B * H;
    hipStream_t st = (hipStream_t)stream;
    if (g.wlds) {
        if (use_bf16 == 0) return ls_launch(lstm_fwd_kernel<0, true>, p, g, persistent, false, st);
        if (use_bf16 == 1) return ls_launch(lstm_fwd_kernel<1, true>, p, g, persistent, false, st);
        return ls_launch(lstm_fwd_kernel<2, true>, p, g, persistent, false, st);
    }
    if (use_bf16 == 0) return ls_launch(lstm_fwd_kernel<0, false>, p, g, 0, false, st);
    if (use_bf16 == 1) return ls_launch(lstm_fwd_kernel<1, false>, p, g, 0, false, st);
    return ls_launch(lstm_fwd_kernel<2, false>, p, g, 0, false, st);
}

extern "C" int v100_lstm_bwd(const float* dy, const float* dh_n, const float* dc_n, const void* w_prep, const int* lens,
                             const float* act, const float* cs, float* dgates, void* ws, unsigned* sync,
                             int B, int T, int H, int ndir, int use_bf16, int persistent, void* stream) {
    if (!dy || !w_prep || !lens || !act || !cs || !dgates || !ws || !sync) return V100_ERR_NULL;
    if (!ls_shape_ok(B, T, H, ndir) || use_bf16 < 0 || use_bf16 > 1) return V100_ERR_SHAPE;
    const Geo g = ls_geometry(H, use_bf16, 1);
    LsParams p = ls_params(g, B, T, H, ndir);
    p.xin = dy; p.w = w_prep; p.b0 = dh_n; p.b1 = dc_n; p.lens = lens; p.out = dgates;
    p.act = (float*)act; p.cs = (float*)cs; p.sync = sync;
    p.xch = (float*)ws;
    p.st = p.xch + (size_t)ndir * 2 * B * 4 * H;
    hipStream_t st = (hipStream_t)stream;
    if (g.wlds) {
        if (use_bf16 == 0) return ls_launch(lstm_bwd_kernel<0, true>, p, g, persistent, true, st);
        return ls_launch(lstm_bwd_kernel<1, true>, p, g, persistent, true, st);
    }
    if (use_bf16 == 0) return ls_launch(lstm_bwd_kernel<0, false>, p, g, 0, true, st);
    return ls_launch(lstm_bwd_kernel<1, false>, p, g, 0, true, st);
}
