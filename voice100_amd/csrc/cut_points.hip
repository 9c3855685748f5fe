// K31: where to cut a chapter-length recording for transcription -- the CTC pause cutter (decode.ctc_cut_points).
//
// The rule is tests/_cut_points_ref.py; every decision below is an integer comparison or a comparison of margins that come from one
// fp32 subtraction, so the tables equal the numpy mirror exactly.
//
//   cut_points_frames_kernel   streams the logits once: G = 32 or 64 lanes across V, 64 consecutive frames per wave.  Writes the
//                              margin d[t] = logit[blank] - max of the others (a NaN anywhere in the frame, or inf - inf, is stored
//                              as -inf: not silent, and last in the forced cut's argmax) and one 64-bit word of silent bits per wave.
//   cut_points_walk_kernel     one workgroup of CP_THREADS per recording, four steps, all of them over the bit words and the tables
//                              they give (nothing touches the logits again):
//                                1. trim: the first and the last non-silent frame (a block-wide max over the words);
//                                2. the run table: starts and ends of the maximal silent runs inside the trimmed recording, from the
//                                   0->1 and 1->0 edges of the words, compacted in order with a block scan per pass of CP_PASS frames;
//                                3. stage A: the runs of min_gap frames or more, compacted the same way -- core c lies between cut
//                                   run c - 1 and cut run c;
//                                4. the piece table: CP_THREADS cores at a time, every core that fits is one piece, written by its
//                                   own thread; an oversized core is walked by the whole workgroup (stage B): the candidates of a step
//                                   are a contiguous slice of the run table (at most C / 2 + 1 runs), the forced cut is an argmax over
//                                   at most C / 2 + 1 margins, both one block-wide max of a 64-bit key.
//   cut_points_table_kernel    after the caller has read n_seg (the one read-back): pads the pieces into the silence around them and
//                              writes the [B][S] tables, zeros beyond n_seg.
//
// Every loop runs to a bound computed from n, C and min_frames, never to a condition on the data alone.
// CUT_POINTS_HOST_EMU compiles the walk and the table bodies as plain C++ (a thread per lane, a std::barrier for the workgroup's)
// for tools/cut_points_host.cpp; the library build never defines it.
#ifdef CUT_POINTS_HOST_EMU
#include <stdint.h>
#define CP_DEV static inline
#else
#include "common.h"
#define CP_DEV __device__ __forceinline__
#endif

#define CP_THREADS 512
#define CP_WAVES (CP_THREADS / 64)
#define CP_SPAN 64                                      // frames per thread and pass: one word of silent bits
#define CP_PASS (CP_THREADS * CP_SPAN)                  // frames per pass of the run scan
#define CP_FT 256                                       // threads of the frame pass: four waves of 64 frames
#define CP_TMAX (1 << 20)
#define CP_VMAX 128
#define CP_FMAX 4096
#define CP_FORCED (1u << 31)                            // piece table: the piece begins at a forced cut (starts are below 2^20)

typedef unsigned long long cp_u64;

// per recording: header {n, first, last + 1, pieces}, margins [T], words [(T + 63) / 64], run starts / ends and cut-run indices
// [T / 2 + 2] each (runs alternate with non-silent frames), piece starts / ends [T] each (pieces are disjoint and non-empty)
struct CpLayout { long long hdr, d, mask, rs, re, cut, ps, pe, row; int words, runs; };
static inline long long cp_al(long long x) { return (x + 15) & ~15LL; }
static inline CpLayout cp_layout(int T) {
    CpLayout l;
    l.words = (T + 63) / 64;
    l.runs = T / 2 + 2;
    l.hdr = 0;
    l.d = 16;
    l.mask = l.d + cp_al(4LL * T);
    l.rs = l.mask + cp_al(8LL * l.words);
    l.re = l.rs + cp_al(4LL * l.runs);
    l.cut = l.re + cp_al(4LL * l.runs);
    l.ps = l.cut + cp_al(4LL * l.runs);
    l.pe = l.ps + cp_al(4LL * T);
    l.row = l.pe + cp_al(4LL * T);
    return l;
}
static inline bool cp_supported(int B, int T, int V, int blank, int max_frames, int min_gap, int pad, int min_frames) {
    if (!(B >= 1 && B <= 65535 && T >= 1 && T <= CP_TMAX && V >= 2 && V <= CP_VMAX && blank >= 0 && blank < V)) return false;
    if (!(max_frames >= 2 && max_frames <= CP_FMAX && pad >= 0 && pad <= CP_FMAX && min_frames >= 1 && min_frames <= CP_FMAX)) return false;
    return min_gap >= 0 && max_frames - 2 * pad >= 2 * min_frames;            // min_gap 0: no stage A
}

struct CpArgs { int T, C, min_gap, min_frames; };
struct CpShared { cp_u64 red[CP_WAVES]; cp_u64 bc; int tot[CP_WAVES]; int next; };

#ifdef CUT_POINTS_HOST_EMU
// the host program supplies cp_sync(), cp_block_max(S, tid, v) and cp_block_scan(S, tid, v, &total) over its own threads
static inline int cp_ld(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
static inline cp_u64 cp_ld(const cp_u64* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
static inline void cp_min_shared(int* p, int v) { int o = __atomic_load_n(p, __ATOMIC_RELAXED); while (v < o && !__atomic_compare_exchange_n(p, &o, v, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {} }
static inline int cp_popc(cp_u64 x) { return __builtin_popcountll(x); }
static inline int cp_ctz(cp_u64 x) { return __builtin_ctzll(x); }
static inline int cp_clz(cp_u64 x) { return __builtin_clzll(x); }
void cp_sync();
cp_u64 cp_block_max(CpShared& S, int tid, cp_u64 v);
int cp_block_scan(CpShared& S, int tid, int v, int* total);
#else
// what this workgroup stored earlier in the launch is read past the vector L1
CP_DEV int cp_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
CP_DEV cp_u64 cp_ld(const cp_u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
CP_DEV void cp_min_shared(int* p, int v) { atomicMin(p, v); }
CP_DEV int cp_popc(cp_u64 x) { return __popcll(x); }
CP_DEV int cp_ctz(cp_u64 x) { return __builtin_ctzll(x); }
CP_DEV int cp_clz(cp_u64 x) { return __builtin_clzll(x); }
// workgroup barrier that also orders the tables' global stores before the loads that follow it
CP_DEV void cp_sync() { __threadfence(); __syncthreads(); }

// the largest v of the workgroup, in every thread
CP_DEV cp_u64 cp_block_max(CpShared& S, int tid, cp_u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const cp_u64 o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    __syncthreads();                                                        // the previous reduction's readers are done
    if ((tid & 63) == 0) S.red[tid >> 6] = v;
    __syncthreads();
    cp_u64 m = S.red[0];
#pragma unroll
    for (int w = 1; w < CP_WAVES; ++w) m = S.red[w] > m ? S.red[w] : m;
    return m;
}

// exclusive prefix sum of v over the workgroup's threads in order, and its total
CP_DEV int cp_block_scan(CpShared& S, int tid, int v, int* total) {
    const int lane = tid & 63;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    __syncthreads();
    if (lane == 63) S.tot[tid >> 6] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < CP_WAVES; ++w) {
        const int t = S.tot[w];
        if (w < (tid >> 6)) before += t;
        all += t;
    }
    *total = all;
    return before + inc - v;
}
#endif

// fp32 bits in an order that unsigned comparison follows; -0 counts as +0 (the mirror's argmax compares values)
CP_DEV unsigned cp_ordered(float d) {
    if (d == 0.0f) d = 0.0f;
    unsigned u;
    __builtin_memcpy(&u, &d, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the word of silent bits w with the bit of frame 64 w - 1 shifted in below it
CP_DEV cp_u64 cp_prev_word(const cp_u64* mask, int w, cp_u64 x) { return (x << 1) | (w > 0 ? mask[w - 1] >> 63 : 0ull); }
// bits of word w whose frames t satisfy lo < t < hi
CP_DEV cp_u64 cp_open_range(int w, int lo, int hi) {
    const long long base = 64LL * w;
    const long long a = lo + 1 - base, b = hi - base;                       // bits [a, b)
    if (b <= 0 || a >= 64 || a >= b) return 0ull;
    const cp_u64 below_b = b >= 64 ? ~0ull : ((1ull << b) - 1);
    const cp_u64 below_a = a <= 0 ? 0ull : ((1ull << a) - 1);
    return below_b & ~below_a;
}

// first index in [lo, hi) of the ascending table tab with tab[i] >= key (hi if none); at most 21 halvings of a range below 2^20
CP_DEV int cp_lower_bound(const int* tab, int lo, int hi, int key) {
    for (int it = 0; it < 21 && lo < hi; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cp_ld(tab + mid) < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

CP_DEV void cp_emit(int* ps, int* pe, int idx, int cap, int start, int end, int forced) {
    if (idx >= 0 && idx < cap) { ps[idx] = start | (forced ? (int)CP_FORCED : 0); pe[idx] = end; }
}

// Stage B on the core [a, b) whose runs are rs / re [j0, j1): pieces go to ps / pe from index `out` on; returns their number.
// Every thread of the workgroup calls it with the same arguments and gets the same result.
CP_DEV int cp_split_core(CpShared& S, int tid, const CpArgs& A, const float* d, const int* rs, const int* re, int* ps, int* pe,
                         int a, int b, int j0, int j1, int out) {
    const int C = A.C, mf = A.min_frames;
    const int max_steps = (b - a) / mf + 1;                                 // every step emits at least min_frames frames
    const int max_it = (C / 2 + 1) / CP_THREADS + 2;                        // runs that begin in [a, a + C]: every run ends on a non-silent frame
    int cnt = 0, forced = 0, jcur = j0;
    for (int step = 0; step < max_steps && b - a > C; ++step) {
        cp_u64 best = 0;
        for (int it = 0, j = jcur + tid; it < max_it && j < j1; ++it, j += CP_THREADS) {
            const int r0 = cp_ld(rs + j);
            if (r0 - a > C) break;
            const int r1 = cp_ld(re + j);
            if (r0 - a >= mf && b - r1 >= mf) {
                const cp_u64 key = ((cp_u64)(unsigned)(r1 - r0) << 32) | (unsigned)j;       // the longest, ties to the latest
                best = key > best ? key : best;
            }
        }
        best = cp_block_max(S, tid, best);
        int cut_end, next_a;
        if (best != 0) {
            const int j = (int)(unsigned)(best & 0xFFFFFFFFull);
            cut_end = cp_ld(rs + j);
            next_a = cp_ld(re + j);
            jcur = j + 1;
        } else {
            const int lo = a + (C / 2 > mf ? C / 2 : mf), hi = (a + C < b - mf) ? a + C : b - mf;
            cp_u64 k = 0;
            const int max_jt = (C + 1) / CP_THREADS + 2;
            for (int it = 0, t = lo + tid; it < max_jt && t <= hi; ++it, t += CP_THREADS) {
                const cp_u64 key = ((cp_u64)cp_ordered(d[t]) << 32) | (unsigned)(0x7FFFFFFF - t);   // the largest, ties to the first
                k = key > k ? key : k;
            }
            k = cp_block_max(S, tid, k);
            int t = 0x7FFFFFFF - (int)(unsigned)(k & 0xFFFFFFFFull);
            t = t < lo ? lo : (t > hi ? hi : t);                            // (k is never 0: lo <= hi)
            cut_end = next_a = t;
            jcur = cp_lower_bound(rs, jcur, j1, t);
        }
        if (tid == 0) cp_emit(ps, pe, out + cnt, A.T, a, cut_end, forced);
        forced = best == 0;
        a = next_a;
        ++cnt;
    }
    if (tid == 0) cp_emit(ps, pe, out + cnt, A.T, a, b, forced);
    return cnt + 1;
}

// The walk of one recording (steps 1-4 above).  n frames, words of silent bits in mask, margins in d; writes hdr and the tables.
CP_DEV void cp_walk(CpShared& S, int tid, const CpArgs& A, int n, const float* d, const cp_u64* mask, int* hdr, int* rs, int* re, int* cut,
                    int* ps, int* pe, int run_cap, int* n_seg) {
    const int words = (n + 63) / 64;
    // 1. trim
    cp_u64 lo_key = 0, hi_key = 0;
    for (int w = tid; w < words; w += CP_THREADS) {
        const cp_u64 valid = n - 64 * w >= 64 ? ~0ull : ((1ull << (n - 64 * w)) - 1);
        const cp_u64 loud = ~mask[w] & valid;
        if (loud) {
            const cp_u64 first = (cp_u64)(CP_TMAX - (64 * w + cp_ctz(loud))), last = (cp_u64)(64 * w + 63 - cp_clz(loud) + 1);
            lo_key = first > lo_key ? first : lo_key;
            hi_key = last > hi_key ? last : hi_key;
        }
    }
    lo_key = cp_block_max(S, tid, lo_key);
    hi_key = cp_block_max(S, tid, hi_key);
    if (hi_key == 0) {                                                      // no non-silent frame
        if (tid == 0) { hdr[0] = n; hdr[1] = 0; hdr[2] = 0; hdr[3] = 0; *n_seg = 0; }
        return;
    }
    const int a0 = CP_TMAX - (int)lo_key, b0 = (int)hi_key;
    // 2. the run table: a run begins where a silent frame follows a non-silent one and ends where the opposite happens, both strictly
    //    inside (a0, b0); the two edge counts are equal, and a pass scans them packed in one int (at most 32 of each per word)
    int nruns = 0, nends = 0;
    for (int base = 0; base < words; base += CP_THREADS) {
        const int w = base + tid;
        cp_u64 sb = 0, eb = 0;
        if (w < words) {
            const cp_u64 x = mask[w], p = cp_prev_word(mask, w, x), in = cp_open_range(w, a0, b0);
            sb = x & ~p & in;
            eb = ~x & p & in;
        }
        int total;
        const int packed = cp_block_scan(S, tid, cp_popc(sb) | (cp_popc(eb) << 16), &total);
        int is = nruns + (packed & 0xFFFF), ie = nends + (packed >> 16);
        for (int k = 0; k < 32 && sb; ++k, ++is) {
            if (is < run_cap) rs[is] = 64 * w + cp_ctz(sb);
            sb &= sb - 1;
        }
        for (int k = 0; k < 32 && eb; ++k, ++ie) {
            if (ie < run_cap) re[ie] = 64 * w + cp_ctz(eb);
            eb &= eb - 1;
        }
        nruns += total & 0xFFFF;
        nends += total >> 16;
    }
    nruns = nruns < run_cap ? nruns : run_cap;
    nruns = nruns < nends ? nruns : nends;                                  // (equal by construction)
    cp_sync();
    // 3. stage A: the indices of the runs of min_gap frames or more
    int ncuts = 0;
    if (A.min_gap > 0) {
        for (int base = 0; base < nruns; base += CP_THREADS) {
            const int j = base + tid;
            const int flag = j < nruns && cp_ld(re + j) - cp_ld(rs + j) >= A.min_gap;
            int total;
            const int at = cp_block_scan(S, tid, flag, &total);
            if (flag) cut[ncuts + at] = j;                                  // ncuts + at <= j < run_cap
            ncuts += total;
        }
        cp_sync();
    }
    // 4. the pieces, CP_THREADS cores at a time; `extra` = pieces that stage B has added before the core at hand
    const int ncores = ncuts + 1;
    int extra = 0;
    for (int base = 0; base < ncores; base += CP_THREADS) {
        const int c = base + tid;
        int a = 0, b = 0, j0 = 0, j1 = 0;
        if (c < ncores) {
            const int jl = c > 0 ? cp_ld(cut + c - 1) : -1, jr = c < ncuts ? cp_ld(cut + c) : nruns;
            a = c > 0 ? cp_ld(re + jl) : a0;
            b = c < ncuts ? cp_ld(rs + jr) : b0;
            j0 = jl + 1;
            j1 = jr;
        }
        const int over = c < ncores && b - a > A.C;
        int cur = 0;
        for (int it = 0; it <= CP_THREADS; ++it) {
            if (tid == 0) S.next = CP_THREADS;
            cp_sync();
            if (over && tid >= cur) cp_min_shared(&S.next, tid);
            cp_sync();
            const int nx = S.next;                                          // the next oversized core of this batch, or CP_THREADS
            if (c < ncores && tid >= cur && tid < nx) cp_emit(ps, pe, c + extra, A.T, a, b, 0);
            if (nx >= CP_THREADS) break;
            if (tid == nx) S.bc = ((cp_u64)(unsigned)a << 32) | (unsigned)b;
            cp_sync();
            const int ca = (int)(S.bc >> 32), cb = (int)(S.bc & 0xFFFFFFFFull);
            cp_sync();
            if (tid == nx) S.bc = ((cp_u64)(unsigned)j0 << 32) | (unsigned)j1;
            cp_sync();
            const int cj0 = (int)(S.bc >> 32), cj1 = (int)(S.bc & 0xFFFFFFFFull);
            const int made = cp_split_core(S, tid, A, d, rs, re, ps, pe, ca, cb, cj0, cj1, base + nx + extra);
            extra += made - 1;
            cur = nx + 1;
            cp_sync();
        }
        cp_sync();
    }
    int total = ncores + extra;
    total = total < A.T ? total : A.T;
    if (tid == 0) { hdr[0] = n; hdr[1] = a0; hdr[2] = b0; hdr[3] = total; *n_seg = total; }
}

// Entry k of one recording's padded table: pieces from ps / pe, n and the count from hdr.
CP_DEV void cp_table_entry(const int* hdr, const int* ps, const int* pe, int k, int pad, int* start, int* end, int* forced) {
    const int n = hdr[0], cnt = hdr[3];
    if (k >= cnt) { *start = 0; *end = 0; *forced = 0; return; }
    const unsigned raw = (unsigned)ps[k];
    int s = (int)(raw & ~CP_FORCED), e = pe[k];
    const int f = (raw & CP_FORCED) != 0;
    if (k == 0) s -= pad < s ? pad : s;
    else if (!f) { const int half = (s - pe[k - 1]) / 2; s -= pad < half ? pad : half; }
    if (k == cnt - 1) e += pad < n - e ? pad : n - e;
    else {
        const unsigned nraw = (unsigned)ps[k + 1];
        if (!(nraw & CP_FORCED)) { const int half = ((int)(nraw & ~CP_FORCED) - e) / 2; e += pad < half ? pad : half; }
    }
    *start = s; *end = e; *forced = f;
}

#ifndef CUT_POINTS_HOST_EMU
template <int G>
__global__ __launch_bounds__(CP_FT) void cut_points_frames_kernel(const float* __restrict__ logits, const int* __restrict__ lens,
                                                                  unsigned char* __restrict__ ws, long long row_bytes, long long d_off,
                                                                  long long mask_off, int T, int V, int blank, float margin) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, sub = lane & (G - 1), grp = lane / G;
    int n = lens ? lens[b] : T;
    n = n < 0 ? 0 : (n > T ? T : n);
    const int word = blockIdx.x * (CP_FT / 64) + (threadIdx.x >> 6), base = word * 64;
    if (base >= n) return;                                                  // wave-uniform; nothing beyond a row's length is read
    float* d = (float*)(ws + (size_t)b * row_bytes + d_off);
    cp_u64* mask = (cp_u64*)(ws + (size_t)b * row_bytes + mask_off);
    constexpr int FPI = 64 / G;                                             // frames per iteration
    const int owner = grp * G + (blank & (G - 1));                          // the lane that loads the blank's logit
    cp_u64 bits = 0;
#pragma unroll 4
    for (int it = 0; it < G; ++it) {
        const int f = base + it * FPI + grp;
        const bool valid = f < n;
        float m = -INFINITY, lb = 0.0f;
        int bad = 0;
        if (valid) {
            const float* row = logits + ((size_t)b * T + f) * V;
            for (int v = sub; v < V; v += G) {
                const float x = row[v];
                if (v == blank) lb = x;
                else if (x != x) bad = 1;
                else m = x > m ? x : m;
            }
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {
            m = fmaxf(m, __shfl_xor(m, off, 64));
            bad |= __shfl_xor(bad, off, 64);
        }
        lb = __shfl(lb, owner, 64);
        float dd = lb - m;                                                  // the one fp32 subtraction
        if (bad || dd != dd) dd = -INFINITY;
        const bool silent = valid && dd > margin;
        if (valid && sub == 0) d[f] = dd;
        const cp_u64 bal = __ballot(silent && sub == 0);
        if constexpr (G == 64) bits |= (bal & 1ull) << it;
        else bits |= ((bal & 1ull) | (((bal >> 32) & 1ull) << 1)) << (2 * it);
    }
    if (lane == 0) mask[word] = bits;
}

__global__ __launch_bounds__(CP_THREADS) void cut_points_walk_kernel(const int* __restrict__ lens, unsigned char* ws, CpLayout L, CpArgs A,
                                                                     int* __restrict__ n_seg) {
    __shared__ CpShared S;
    const int b = blockIdx.x, tid = threadIdx.x;
    int n = lens ? lens[b] : A.T;
    n = n < 0 ? 0 : (n > A.T ? A.T : n);
    unsigned char* row = ws + (size_t)b * L.row;
    cp_walk(S, tid, A, n, (const float*)(row + L.d), (const cp_u64*)(row + L.mask), (int*)(row + L.hdr), (int*)(row + L.rs),
            (int*)(row + L.re), (int*)(row + L.cut), (int*)(row + L.ps), (int*)(row + L.pe), L.runs, n_seg + b);
}

__global__ __launch_bounds__(256) void cut_points_table_kernel(const unsigned char* __restrict__ ws, CpLayout L, int pad, int S,
                                                               int* __restrict__ start, int* __restrict__ end, int* __restrict__ forced) {
    const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= S) return;
    const unsigned char* row = ws + (size_t)b * L.row;
    int s, e, f;
    cp_table_entry((const int*)(row + L.hdr), (const int*)(row + L.ps), (const int*)(row + L.pe), k, pad, &s, &e, &f);
    start[(size_t)b * S + k] = s;
    end[(size_t)b * S + k] = e;
    forced[(size_t)b * S + k] = f;
}

extern "C" int v100_ctc_cut_points_span(void) { return CP_SPAN; }
extern "C" int v100_ctc_cut_points_pass(void) { return CP_PASS; }

extern "C" long long v100_ctc_cut_points_workspace_bytes(int B, int T) {
    if (B < 1 || T < 1 || T > CP_TMAX) return 0;
    return (long long)B * cp_layout(T).row;
}

extern "C" int v100_ctc_cut_points(const float* logits, const int* lengths, void* ws, int* n_seg, int B, int T, int V, int blank,
                                   int max_frames, int min_gap, float margin, int pad, int min_frames, void* stream) {
    if (!logits || !ws || !n_seg) return V100_ERR_NULL;
    if (!cp_supported(B, T, V, blank, max_frames, min_gap, pad, min_frames) || margin != margin) return V100_ERR_SHAPE;
    const CpLayout L = cp_layout(T);
    const CpArgs A = {T, max_frames - 2 * pad, min_gap, min_frames};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((L.words + CP_FT / 64 - 1) / (CP_FT / 64)), (unsigned)B);
    if (V <= 32) V100_GGL(cut_points_frames_kernel<32>, grid, dim3(CP_FT), 0, st, logits, lengths, (unsigned char*)ws, L.row, L.d, L.mask, T, V, blank, margin);
    else V100_GGL(cut_points_frames_kernel<64>, grid, dim3(CP_FT), 0, st, logits, lengths, (unsigned char*)ws, L.row, L.d, L.mask, T, V, blank, margin);
    V100_GGL(cut_points_walk_kernel, dim3((unsigned)B), dim3(CP_THREADS), 0, st, lengths, (unsigned char*)ws, L, A, n_seg);
    return v100_launch_status();
}

extern "C" int v100_ctc_cut_points_table(const void* ws, int* start, int* end, int* forced, int B, int T, int S, int pad, void* stream) {
    if (!ws || !start || !end || !forced) return V100_ERR_NULL;
    if (B < 1 || T < 1 || T > CP_TMAX || S < 1 || S > T || pad < 0 || pad > CP_FMAX) return V100_ERR_SHAPE;
    const CpLayout L = cp_layout(T);
    V100_GGL(cut_points_table_kernel, dim3((unsigned)((S + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
             (const unsigned char*)ws, L, pad, S, start, end, forced);
    return v100_launch_status();
}
#endif
