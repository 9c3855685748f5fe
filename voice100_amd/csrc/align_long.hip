// K29: forced alignment of chapter-length recordings in one launch -- a banded Viterbi over the CTC topology.
//
//   ctc_align_long   T up to 2^20 frames against up to 2^19 labels.  K20 (align.hip) keeps a score for every extended position in
//                    LDS and a move byte per frame and position; neither survives a two-hour recording.  Here only a window of W
//                    ("band") consecutive positions [lo, lo + W) is live, everything outside it is -inf, and every LA_BLK frames
//                    the window is re-centred on the best position and the scores are renormalised (their maximum goes into an
//                    fp64 offset: an fp32 running score over 10^5 frames would drop emission differences below its ulp).
//
// The recurrence is the standard CTC one (stay, advance by one, skip a blank between two different labels; ctc_segment's topology,
// not K20's max_move rule), first maximum wins, one fp32 add after the max, no transcendentals: tests/_align_long_ref.py mirrors it
// bit for bit in numpy.
//
// One workgroup of 512 threads per recording; a thread owns groups of four consecutive window slots.  As in align.hip:
//   * emissions: the log-probability rows of LA_BLK frames (and the free-end column, if any) are staged in LDS one block ahead of
//     the recurrence and held in registers across it; rows too wide for the buffer are gathered from global memory (STAGED = false);
//   * the per-frame barrier waits for LDS only: the move stores and the prefetch stay in flight across it;
//   * moves are two bits per slot, four slots to the byte, W / 4 bytes per frame in global memory, slot-indexed; the window's lo of
//     every block of LA_BLK frames is recorded next to them;
//   * traceback: LA_TB frames of moves at a time are staged back into LDS by all threads -- the position falls by at most 2 per
//     frame, so LA_TB frames need 2 (LA_TB - 1) + 1 positions below the current one -- and one thread walks them there; once the
//     position is 0 it stays 0 (nothing lies below state 0), so the rest is filled;
//   * the path leaves through LDS in coalesced rows; durations are the walker's own run lengths (one store per run into a zeroed
//     row: no atomics, nothing is read back).
#include "common.h"
#include <math.h>

#define LA_THREADS 512
#define LA_WAVES (LA_THREADS / 64)
#define LA_BLK 16                                       // frames per staged block of emissions = the re-centring period R
#define LA_NR 8                                         // staged floats per thread and block
#define LA_BUF (LA_NR * LA_THREADS)                     // floats per staging buffer: LA_BLK rows of V, then LA_BLK free-end values
#define LA_VSTAGE (LA_BUF / LA_BLK - 1)                 // widest row that is staged: 255
#define LA_TB 64                                        // frames per traceback block
#define LA_WB 36                                        // staged move bytes per traceback row: (2 (LA_TB - 1) + 3) / 4 + 1 = 33, padded
#define LA_WMIN 64
#define LA_WMAX 8192
#define LA_TMAX (1 << 20)
#define LA_LMAX (1 << 19)
#define LA_HDR 128                                      // bytes: [0] traceback position, [1] feasible; [8..15], [16..23], [24..31] per-wave maxima
#define LA_SKIP (1 << 30)                               // meta: v - 2 is a candidate
#define LA_FREE (1 << 29)                               // meta: the state emits the free-end column
#define LA_DEAD (int)(1u << 31)                         // meta: v >= n
#define LA_COL (LA_FREE - 1)
// LDS-only barrier: LDS traffic of every wave has landed; global loads and stores stay in flight
#define LA_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

static inline long long la_blocks(int T) { return ((long long)T + LA_BLK - 1) / LA_BLK; }
static inline long long la_moves_bytes(int T, int W) { return (long long)T * (W / 4); }           // per recording; W / 4 is a multiple of 16
static inline bool la_supported(int B, int T, int Lmax, int W) {
    return B > 0 && T > 0 && T <= LA_TMAX && Lmax >= 0 && Lmax <= LA_LMAX && W >= LA_WMIN && W <= LA_WMAX && W % 64 == 0;
}

// what this workgroup stored earlier in the launch is read past the vector L1
__device__ __forceinline__ int la_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned char la_ld(const unsigned char* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <bool STAGED>
__global__ __launch_bounds__(LA_THREADS) void ctc_align_long_kernel(const float* __restrict__ logp, const long long* __restrict__ labels,
                                                                    const int* __restrict__ in_len, const int* __restrict__ lab_len,
                                                                    const float* __restrict__ free_logp, unsigned char* moves, int* lo_ws,
                                                                    double* __restrict__ score, int* __restrict__ ok, int* path, int* align,
                                                                    int T, int V, int Lmax, int W, int blank, int NB) {
    extern __shared__ __attribute__((aligned(16))) unsigned char la_smem[];
    const int WS = W + 4;                               // floats per score buffer: four -inf in front of slot 0 (the states below lo)
    const int G = W >> 2;                               // groups of four slots = move bytes per frame
    int* hdr = (int*)la_smem;
    float* rm = (float*)(hdr + 8);
    int* ra = hdr + 16;
    float* rc = (float*)(hdr + 24);
    float* sc = (float*)(la_smem + LA_HDR);             // [2][WS]
    int* meta = (int*)(sc + 2 * WS);                    // [W] emission column and flags of the state in each slot
    unsigned char* win = (unsigned char*)(meta + W);    // [LA_TB][LA_WB] staged moves
    int* rowbase = (int*)(win + LA_TB * LA_WB);         // [LA_TB] state of the first staged move of each row
    int* pl = rowbase + LA_TB;                          // [LA_TB] path of one traceback block
    float* em = (float*)(pl + LA_TB);                   // [2][LA_BUF] staged emissions (STAGED only)

    const int b = blockIdx.x, tid = threadIdx.x;
    int Tb = in_len ? in_len[b] : T;
    if (Tb > T) Tb = T;
    int L = lab_len ? lab_len[b] : Lmax;
    if (L > Lmax) L = Lmax;
    if (L < 0) L = 0;
    const int n = 2 * L + 1;
    const int Sout = 2 * Lmax + 1;
    const long long* lab = labels + (size_t)b * Lmax;
    const float* lp = logp + (size_t)b * T * V;
    const float* fr = free_logp ? free_logp + (size_t)b * T : nullptr;
    unsigned char* bk = moves + (size_t)b * T * G;
    int* lo_b = lo_ws + (size_t)b * NB;
    int* path_b = path + (size_t)b * T;
    int* align_b = align + (size_t)b * Sout;

    auto infeasible = [&]() {                           // nothing to align, or the band lost the path
        for (int t = tid; t < T; t += LA_THREADS) path_b[t] = 0;
        for (int s = tid; s < Sout; s += LA_THREADS) align_b[s] = 0;
        if (tid == 0) { score[b] = -INFINITY; ok[b] = 0; }
    };
    if (Tb < 1) { infeasible(); return; }

    auto mk = [&](int v) -> int {                       // column (clamped into the row) and flags of state v
        if (v >= n) return LA_DEAD;
        long long e = blank;
        int flags = 0;
        if (v & 1) {
            e = lab[v >> 1];
            if (e != blank && v >= 3 && e != lab[(v >> 1) - 1]) flags = LA_SKIP;
        }
        if (fr && (v == 0 || v == n - 1)) flags |= LA_FREE;
        const int c = (int)(e < 0 ? 0 : (e > V - 1 ? V - 1 : e));
        return c | flags;
    };
    const int nblk = (Tb + LA_BLK - 1) / LA_BLK;
    // what block kb's frames read: its rows of logp, flat, then its free-end values at LA_BLK * V
    auto fetch = [&](int kb, int idx) -> float {
        const int f0 = kb * LA_BLK;
        const int rows = min(Tb, f0 + LA_BLK) - f0;
        if (idx < rows * V) return lp[(size_t)f0 * V + idx];
        const int q = idx - LA_BLK * V;
        return (fr && q >= 0 && q < rows) ? fr[f0 + q] : 0.0f;
    };
    for (int s = tid; s < W; s += LA_THREADS) meta[s] = mk(s);
    if (tid < 8) sc[(tid & 3) + (tid >> 2) * WS] = -INFINITY;
    if (STAGED) {
#pragma unroll
        for (int q = 0; q < LA_NR; ++q) em[tid + q * LA_THREADS] = fetch(0, tid + q * LA_THREADS);
    }
    __syncthreads();
    auto emit = [&](int mt, int t, int f, const float* emk) -> float {
        const int c = mt & LA_COL;
        if (STAGED) return emk[(mt & LA_FREE) ? LA_BLK * V + f : f * V + c];
        return (mt & LA_FREE) ? fr[t] : lp[(size_t)t * V + c];
    };
    // frame 0: positions 0 and 1 are live
    for (int s = tid; s < W; s += LA_THREADS) sc[4 + s] = (s < 2 && s < n) ? emit(meta[s], 0, 0, em) : -INFINITY;
    __syncthreads();

    int p = 0;                                          // the score buffer that holds the newest frame
    int lo = 0;
    double offset = 0.0;
    for (int k = 0; k < nblk; ++k) {
        if (k > 0) {
            // re-centre and renormalise: the window's maximum and the first slot that attains it
            const float* cur = sc + p * WS + 4;
            // m: the maximum of all the window's scores (what is subtracted); c, a: the maximum over the states that do not emit the
            // free-end column and the first slot that attains it (where the window goes).  A free end state emits every frame's best
            // log-probability, so no other state ever beats it: taken into the argmax it would pin the window to state 0.
            float m = -INFINITY, c = -INFINITY;
            int a = 0x7fffffff;
            for (int g = tid; g < G; g += LA_THREADS) {
                const f32x4 s4 = *(const f32x4*)(cur + 4 * g);
                const int4 mt = *(const int4*)(meta + 4 * g);
                m = fmaxf(fmaxf(m, fmaxf(s4.x, s4.y)), fmaxf(s4.z, s4.w));
                if (!(mt.x & LA_FREE) && s4.x > c) { c = s4.x; a = 4 * g; }
                if (!(mt.y & LA_FREE) && s4.y > c) { c = s4.y; a = 4 * g + 1; }
                if (!(mt.z & LA_FREE) && s4.z > c) { c = s4.z; a = 4 * g + 2; }
                if (!(mt.w & LA_FREE) && s4.w > c) { c = s4.w; a = 4 * g + 3; }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                m = fmaxf(m, __shfl_xor(m, off, 64));
                const float oc = __shfl_xor(c, off, 64);
                const int oa = __shfl_xor(a, off, 64);
                if (oc > c || (oc == c && oa < a)) { c = oc; a = oa; }
            }
            if ((tid & 63) == 0) { rm[tid >> 6] = m; rc[tid >> 6] = c; ra[tid >> 6] = a; }
            LA_BARRIER();
            m = rm[0];
            c = rc[0];
            a = ra[0];
#pragma unroll
            for (int w = 1; w < LA_WAVES; ++w) {
                m = fmaxf(m, rm[w]);
                const float oc = rc[w];
                const int oa = ra[w];
                if (oc > c || (oc == c && oa < a)) { c = oc; a = oa; }
            }
            if (m > -INFINITY) {                        // the same in every thread
                offset += (double)m;
                const int nlo = c > -INFINITY ? min(max(lo, lo + a - W / 2), max(n - W, 0)) : lo;
                const int shift = nlo - lo;             // >= 0: lo never exceeds max(n - W, 0), and < W / 2
                float* nxt = sc + (p ^ 1) * WS + 4;
                for (int g = tid; g < G; g += LA_THREADS) {
                    f32x4 o;
                    const int s = 4 * g + shift;
                    o.x = s < W ? cur[s] - m : -INFINITY;                    // states that enter the window enter as -inf
                    o.y = s + 1 < W ? cur[s + 1] - m : -INFINITY;
                    o.z = s + 2 < W ? cur[s + 2] - m : -INFINITY;
                    o.w = s + 3 < W ? cur[s + 3] - m : -INFINITY;
                    *(f32x4*)(nxt + 4 * g) = o;
                    if (shift > 0) {                    // meta[s] is read by the thread that writes it
                        int4 mt;
                        mt.x = mk(nlo + 4 * g);
                        mt.y = mk(nlo + 4 * g + 1);
                        mt.z = mk(nlo + 4 * g + 2);
                        mt.w = mk(nlo + 4 * g + 3);
                        *(int4*)(meta + 4 * g) = mt;
                    }
                }
                lo = nlo;
                p ^= 1;
                LA_BARRIER();
            }
        }
        if (tid == 0) lo_b[k] = lo;
        float r[LA_NR];
        if (STAGED && k + 1 < nblk) {                   // the next block's rows: issued here, written to LDS after this block's frames
#pragma unroll
            for (int q = 0; q < LA_NR; ++q) r[q] = fetch(k + 1, tid + q * LA_THREADS);
        }
        const float* emk = em + (k & 1) * LA_BUF;
        const int i1 = min(Tb, (k + 1) * LA_BLK);
        for (int i = max(1, k * LA_BLK); i < i1; ++i) {
            const float* cur = sc + p * WS + 4;
            float* nxt = sc + (p ^ 1) * WS + 4;
            const int f = i - k * LA_BLK;
            unsigned char* bki = bk + (size_t)i * G;
            for (int g = tid; g < G; g += LA_THREADS) {
                const f32x4 c = *(const f32x4*)(cur + 4 * g);
                const float q1 = cur[4 * g - 1], q2 = cur[4 * g - 2];        // slots -1 and -2 hold -inf
                const int4 mt = *(const int4*)(meta + 4 * g);
                const float e0 = emit(mt.x, i, f, emk), e1 = emit(mt.y, i, f, emk), e2 = emit(mt.z, i, f, emk), e3 = emit(mt.w, i, f, emk);
                unsigned mv = 0;
                auto step = [&](float s0, float s1, float s2, int m_, float e, int sh) -> float {
                    float best = s0;
                    unsigned d = 0;
                    if (s1 > best) { best = s1; d = 1; }
                    if ((m_ & LA_SKIP) && s2 > best) { best = s2; d = 2; }
                    mv |= d << sh;
                    return m_ < 0 ? -INFINITY : best + e;
                };
                f32x4 o;
                o.x = step(c.x, q1, q2, mt.x, e0, 0);
                o.y = step(c.y, c.x, q1, mt.y, e1, 2);
                o.z = step(c.z, c.y, c.x, mt.z, e2, 4);
                o.w = step(c.w, c.z, c.y, mt.w, e3, 6);
                *(f32x4*)(nxt + 4 * g) = o;
                bki[g] = (unsigned char)mv;
            }
            p ^= 1;
            LA_BARRIER();
        }
        if (STAGED && k + 1 < nblk) {
            float* dst = em + ((k + 1) & 1) * LA_BUF;   // last read in block k-1, whose frames all ended in a barrier
#pragma unroll
            for (int q = 0; q < LA_NR; ++q) dst[tid + q * LA_THREADS] = r[q];
            LA_BARRIER();
        }
    }
    __syncthreads();                                    // every move store has landed
    if (tid == 0) {
        const float* fin = sc + p * WS + 4;
        auto get = [&](int v) -> float { return (v >= lo && v < lo + W) ? fin[v - lo] : -INFINITY; };
        int j = 0;
        if (n >= 2) j = get(n - 1) > get(n - 2) ? n - 1 : n - 2;
        const float sj = get(j);
        const int feasible = sj > -INFINITY;
        hdr[0] = j;
        hdr[1] = feasible;
        if (feasible) { score[b] = offset + (double)sj; ok[b] = 1; }
    }
    __syncthreads();
    if (!hdr[1]) { infeasible(); return; }
    for (int t = Tb + tid; t < T; t += LA_THREADS) path_b[t] = 0;
    for (int s = tid; s < Sout; s += LA_THREADS) align_b[s] = 0;
    __syncthreads();                                    // the zeros have landed before the walker's run lengths go on top

    // traceback: the moves of frames t_hi .. t_lo+1 give the positions at t_hi .. t_lo+1 and leave the one at t_lo for the next block
    const int wave = tid >> 6, lane = tid & 63;
    int t_hi = Tb - 1;
    int run_end = Tb;                                   // thread 0: one past the last frame of the run the walker is in
    while (t_hi > 0) {
        const int jh = hdr[0];
        if (jh == 0) break;                             // state 0 stays at state 0: every earlier frame is 0
        const int t_lo = max(0, t_hi - LA_TB);
        const int rows = t_hi - t_lo;
        const int wlo = max(jh - 2 * (rows - 1), 0);    // the lowest position any of these frames can be at
        for (int rr = wave; rr < rows; rr += LA_WAVES) {
            const int t = t_hi - rr;
            const int lo_t = la_ld(lo_b + t / LA_BLK);
            const int f = max(wlo - lo_t, 0) & ~3;      // first staged slot of the row
            if (lane == 0) rowbase[rr] = lo_t + f;
            const int c = (f >> 2) + lane;
            if (lane < LA_WB && c < G) win[rr * LA_WB + lane] = la_ld(bk + (size_t)t * G + c);
        }
        __syncthreads();
        if (tid == 0) {
            int j = jh;
            for (int rr = 0; rr < rows; ++rr) {
                pl[rr] = j;
                const int idx = j - rowbase[rr];
                const int mv = (win[rr * LA_WB + (idx >> 2)] >> (2 * (idx & 3))) & 3;
                if (mv) {
                    align_b[j] = run_end - (t_hi - rr);
                    run_end = t_hi - rr;
                    j -= mv;
                }
            }
            hdr[0] = j;
        }
        __syncthreads();
        for (int rr = tid; rr < rows; rr += LA_THREADS) path_b[t_hi - rr] = pl[rr];
        t_hi = t_lo;
    }
    const int j = hdr[0];                               // the position at frame t_hi and, when it is 0, at every frame before
    for (int t = tid; t <= t_hi; t += LA_THREADS) path_b[t] = j;
    if (tid == 0) align_b[j] = run_end;
}

extern "C" int v100_ctc_align_long_block(void) { return LA_BLK; }

extern "C" long long v100_ctc_align_long_workspace_bytes(int B, int T, int Lmax, int band) {
    if (!la_supported(B, T, Lmax, band)) return 0;
    return (long long)B * (la_moves_bytes(T, band) + ((la_blocks(T) * 4 + 15) & ~15LL));
}

template <bool STAGED>
static int la_launch(size_t shmem, hipStream_t st, int B, const float* logp, const long long* labels, const int* in_len, const int* lab_len,
                     const float* free_logp, unsigned char* moves, int* lo_ws, double* score, int* ok, int* path, int* align, int T, int V,
                     int Lmax, int W, int blank, int NB) {
    if (shmem > 64 * 1024 &&
        hipFuncSetAttribute((const void*)ctc_align_long_kernel<STAGED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem) != hipSuccess)
        return V100_ERR_LAUNCH;
    V100_GGL((ctc_align_long_kernel<STAGED>), dim3(B), dim3(LA_THREADS), shmem, st, logp, labels, in_len, lab_len, free_logp, moves, lo_ws,
             score, ok, path, align, T, V, Lmax, W, blank, NB);
    return v100_launch_status();
}

extern "C" int v100_ctc_align_long(const float* logp, const long long* labels, const int* in_len, const int* lab_len, const float* free_logp,
                                   void* ws, double* score, int* ok, int* path, int* align, int B, int T, int V, int Lmax, int band,
                                   int blank, void* stream) {
    if (!logp || !labels || !ws || !score || !ok || !path || !align) return V100_ERR_NULL;
    if (!la_supported(B, T, Lmax, band) || V < 2 || V > LA_COL) return V100_ERR_SHAPE;
    const bool staged = V <= LA_VSTAGE;
    const size_t shmem = LA_HDR + 2 * (size_t)(band + 4) * 4 + (size_t)band * 4 + LA_TB * LA_WB + 2 * LA_TB * 4 +
                         (staged ? 2 * LA_BUF * sizeof(float) : 0);
    const int NB = (int)la_blocks(T);
    unsigned char* mv = (unsigned char*)ws;
    int* lo_ws = (int*)(mv + (size_t)B * la_moves_bytes(T, band));
    hipStream_t st = (hipStream_t)stream;
    if (staged) return la_launch<true>(shmem, st, B, logp, labels, in_len, lab_len, free_logp, mv, lo_ws, score, ok, path, align, T, V, Lmax, band, blank, NB);
    return la_launch<false>(shmem, st, B, logp, labels, in_len, lab_len, free_logp, mv, lo_ws, score, ok, path, align, T, V, Lmax, band, blank, NB);
}
