// K33: K26's CTC forward-backward (ctc_segment.hip: time boundaries, expected durations and confidences of every label and word of a
// GIVEN transcript) for chapter-length recordings: the same lattice restricted to a corridor of W ("band") states around a path.
//
//   Frames come in blocks of SL_FB = 16; lo[k] is the first live state of block k = t >> 4; state s is live at t iff
//   lo[t >> 4] <= s < lo[t >> 4] + W and s < n = 2 L + 1.  alpha_t(s), beta_t(s) and the enter / leave terms are zero at every dead
//   state; p, gamma, the onset and last-frame distributions, medians, durations and confidences follow as in K26.  So every output
//   is the posterior over the alignments that stay inside the corridor; lo = 0 and W >= n is K26's quantity.
//   tests/_ctc_segment_long_ref.py is the definition in float64.
//
// One workgroup of 256 threads per recording, forward and backward in one launch; a second small launch sums the words.
//
// Ownership: a ring.  H = W / 2 pairs (blank 2 i, label 2 i + 1) are live at a time, pair i sits in ring slot i mod H, slot q belongs
// to thread q mod 256 (one or two slots a thread).  lo is even, so a window holds whole pairs, the H pairs of any window have distinct
// slots, and a label's six register accumulators (duration, sum gamma log2 y, the two tails, the two median candidates) never move
// when the window does: at a block boundary the slots whose pair changes are set to zero in the row (what enters starts from
// nothing; the one pair next to the new window whose slot is taken but which was live a frame ago is carried in registers for
// that one frame: a step between two live states counts), everything else stays where it is.  Descending in t the pairs above
// the new window are final: their labels are stored there and then; what is live at t = 0 is flushed at the end.  A pair reads its
// neighbours round the ring, and the two reads that would cross the window's edge (the lowest pair's s - 1 / s - 2, the highest
// pair's s + 1 / s + 2) are zeroed.  (Re-centring by shifted copies, K29's way, was not built: it moves the accumulators of every
// label at every move.)
//
// Numbers: K26's pairs (m, e) = m 2^e, m in [1/2, 1) or 0 -- an fp32 for an emission and for alpha in the workspace, an fp64 in the
// rows and the per-label sums (a label that holds 1,000 of 3,000 frames needs gamma to 1e-7 for the medians' margin: the fp32
// recursion gave 6e-7 at 300 frames) -- but e is an int32 RELATIVE TO ITS BLOCK: once per block the
// row's largest exponent goes into an int64 offset (one for alpha, stored per block beside the workspace; one for beta, carried
// downwards) and is taken off the row.  Inside a block an exponent falls by at most 16 x 2^22 (an emission below 2^-(2^22) counts as
// zero) and zero is 2^-(2^28), so nothing wraps.  gamma's exponent is alpha.e + beta.e + (alpha offset + beta offset - p's exponent),
// the bracket clamped once per block.  log_prob leaves as fp64.  No exp or log in the recursion, no float atomics: two calls give
// equal bits.
//
// Memory safety does not rest on the caller's lo: the forward pass clamps each value to [0, hi], hi = (max(n - W, 0) + 1) & ~1,
// clears bit 0, takes the running maximum and stores that for the backward pass.  Every index is formed from the slot, the frame
// and that sanitised value; none depends on a float.
//
// Workspace, per recording: (alpha.m, alpha.e) and the entering share f per frame and ring slot, 12 T H bytes, read back by the
// thread that wrote them, past the vector L1; the alpha offset and the sanitised lo per block; sum gamma log2 y per label for the
// word launch.
#include "common.h"
#include <math.h>

#define SL_FB 16                                        // frames per block: staged emissions, window moves, renormalisation
#define SL_VMAX 128
#define SL_TMAX (1 << 20)
#define SL_LMAX (1 << 19)
#define SL_WMIN 64
#define SL_WMAX 1024
#define SL_THREADS 256
#define SL_PF (SL_FB * SL_VMAX / SL_THREADS)            // prefetch registers a thread
#define SL_LOG2E 1.44269504089f
#define SL_LOG2E_LO 1.92596299e-8f                      // log2(e) less its fp32
#define SL_LN2 0.69314718056
#define SL_EZERO (-(1 << 28))                           // the exponent of zero: below every live exponent of a block
#define SL_EMIN (-(1 << 22))                            // the lowest exponent of an emission
#define SL_DMAX (1 << 29)                               // clamp of the per-block part of gamma's exponent

#define SL_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

struct SlP { float m; int e; };                                               // m 2^e: an emission
struct SlD { double m; int e; };                                              // ... a state of the lattice
struct __attribute__((aligned(16))) SlPP { double bm, lm; int be, le; };      // a pair of states: blank 2 i, label 2 i + 1

__device__ __forceinline__ SlP sl_zero() { return SlP{0.0f, SL_EZERO}; }
__device__ __forceinline__ SlD sl_dzero() { return SlD{0.0, SL_EZERO}; }
__device__ __forceinline__ SlD sl_d(SlP v) { return SlD{(double)v.m, v.e}; }
__device__ __forceinline__ SlPP sl_pp(SlD b, SlD l) { return SlPP{b.m, l.m, b.e, l.e}; }
__device__ __forceinline__ float sl_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float sl_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ int sl_wave_imax(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}
// v 2^e, v >= 0 finite or NaN -> (m, e') with m in [1/2, 1); zero keeps the exponent of zero.  fp32: an emission; fp64: a state
__device__ __forceinline__ SlP sl_norm(float v, int e) {
    const float m = __builtin_amdgcn_frexp_mantf(v);
    return SlP{m, v > 0.0f ? max(e + __builtin_amdgcn_frexp_expf(v), SL_EZERO) : SL_EZERO};
}
// m 2^d, d the exponent less the sum's largest; below -200 the term is nothing
__device__ __forceinline__ double sl_align(double m, int d) { return ldexp(m, min(max(d, -200), 200)); }
__device__ __forceinline__ SlD sl_norm(double v, int e) {
    const double m = __builtin_amdgcn_frexp_mant(v);
    return SlD{m, v > 0.0 ? max(e + __builtin_amdgcn_frexp_exp(v), SL_EZERO) : SL_EZERO};
}
// what this workgroup stored earlier in the launch is read past the vector L1
__device__ __forceinline__ unsigned long long sl_ld(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ long long sl_ld(const long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float sl_ld(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int sl_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct SlOut {
    double* log_prob; int* ok; int* start; int* end; float* duration; float* log_conf;
    int* word_first; int* word_count; int* word_start; int* word_end; float* word_log_conf; int* n_words;
};
struct SlWs { unsigned long long* a; float* f; long long* aoff; int* lo; float* num; };

static inline long long sl_blocks(int T) { return ((long long)T + SL_FB - 1) / SL_FB; }
static inline bool sl_supported(int B, int T, int Lmax, int W) {
    return B >= 1 && T >= 1 && T <= SL_TMAX && Lmax >= 0 && Lmax <= SL_LMAX && W >= SL_WMIN && W <= SL_WMAX && W % 64 == 0;
}

template <int NL>
__global__ __launch_bounds__(SL_THREADS) void ctc_segment_long_kernel(const float* __restrict__ logits, const int* __restrict__ in_len,
                                                                      const long long* __restrict__ labels, const int* __restrict__ lab_len,
                                                                      const int* __restrict__ lo_in, SlWs ws, SlOut out, int T, int V, int Lmax,
                                                                      int W, int blank, int NB) {
    __shared__ SlPP row[2][SL_WMAX / 2];                // the ring, two frames
    __shared__ SlP stage[SL_FB * SL_VMAX];              // the emissions of the staged frames
    __shared__ int red[SL_THREADS / 64];
    constexpr int nthr = SL_THREADS, nwave = SL_THREADS / 64;
    const int H = W >> 1;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int Tb = in_len ? in_len[b] : T;
    Tb = __builtin_amdgcn_readfirstlane(min(max(Tb, 0), T));
    int L = lab_len ? lab_len[b] : Lmax;
    L = __builtin_amdgcn_readfirstlane(min(max(L, 0), Lmax));
    const int n = 2 * L + 1;
    const int hi = (max(n - W, 0) + 1) & ~1;
    const float* x = logits + (size_t)b * T * V;
    const long long* lab = labels + (size_t)b * Lmax;
    const int* lo_b = lo_in + (size_t)b * NB;
    unsigned long long* wa = ws.a + (size_t)b * T * H;
    float* wf = ws.f + (size_t)b * T * H;
    long long* aoff_b = ws.aoff + (size_t)b * NB;
    int* los_b = ws.lo + (size_t)b * NB;
    float* num_b = ws.num + (size_t)b * Lmax;
    int* o_st = out.start + (size_t)b * Lmax;
    int* o_en = out.end + (size_t)b * Lmax;
    float* o_du = out.duration + (size_t)b * Lmax;
    float* o_lc = out.log_conf + (size_t)b * Lmax;

    // the pair that slot q holds while the window starts at pair `base`
    auto pair_of = [&](int q, int base) { const int r = base % H; return base + (q >= r ? q - r : q - r + H); };
    int pi[NL], cls[NL];                                // per owned slot: its pair, the class of its label (-1: probability zero)
    unsigned skipin = 0u, skipout = 0u;                 // bit k: label i may be entered from label i - 1 / may skip to label i + 1
    auto describe = [&](int k, int i) {                 // slot k now holds pair i
        pi[k] = i;
        cls[k] = -1;
        skipin &= ~(1u << k);
        skipout &= ~(1u << k);
        if (i < L) {
            const long long c = lab[i];
            if (c >= 0 && c < V && c != blank) cls[k] = (int)c;
            if (i >= 1 && lab[i - 1] != c) skipin |= 1u << k;
            if (i + 1 < L && lab[i + 1] != c) skipout |= 1u << k;
        }
    };
    auto sane = [&](int v, int cur) { return max(cur, min(max(v, 0), hi) & ~1); };

    float pf[SL_PF];
    auto prefetch = [&](int c) {                        // raw logits of block c into registers
        const int c0 = c * SL_FB, cnt = min(SL_FB, Tb - c0) * V;
        const float* src = x + (size_t)c0 * V;
#pragma unroll
        for (int j = 0; j < SL_PF; ++j) {
            const int idx = tid + j * nthr;
            pf[j] = idx < cnt ? src[idx] : 0.0f;
        }
    };
    auto commit = [&](int c) {                          // ... into the stage, then the softmax in place, a wave per frame
        const int c0 = c * SL_FB, cn = min(SL_FB, Tb - c0), cnt = cn * V;
#pragma unroll
        for (int j = 0; j < SL_PF; ++j) {
            const int idx = tid + j * nthr;
            if (idx < cnt) stage[idx].m = pf[j];
        }
        SL_BARRIER();
        for (int fr = wave; fr < cn; fr += nwave) {
            SlP* r = stage + fr * V;
            const float v0 = lane < V ? r[lane].m : -INFINITY, v1 = lane + 64 < V ? r[lane + 64].m : -INFINITY;
            const float mx = sl_wave_max(fmaxf(v0, v1));
            auto pair = [&](float v, float lse) {       // log2 y = (v - mx) log2(e) - lse as integer + fraction, y = exp2(fraction) 2^integer
                const float d = v - mx, bb = d - v, dl = (v - (d - bb)) + (-mx - bb);        // v - mx = d + dl exactly (6,000 nats under the
                const float h = d * SL_LOG2E;                                                   // best class d alone is off by 2.4e-4)
                const float l = fmaf(d, SL_LOG2E_LO, fmaf(d, SL_LOG2E, -h)) + dl * SL_LOG2E;
                const float e = fmaxf(floorf(h - lse), (float)SL_EMIN);      // (below SL_EMIN the fraction is so low that y is 0)
                const float y = __builtin_amdgcn_exp2f(((h - e) - lse) + l);
                return y > 0.0f || !(y == y) ? sl_norm(y, (int)e) : sl_zero();
            };
            const float d0 = (v0 - mx) * SL_LOG2E, d1 = (v1 - mx) * SL_LOG2E;
            const float total = sl_wave_sum((lane < V ? __builtin_amdgcn_exp2f(d0) : 0.0f) + (lane + 64 < V ? __builtin_amdgcn_exp2f(d1) : 0.0f));
            const float lse = __builtin_amdgcn_logf(total);
            if (lane < V) r[lane] = v0 > -INFINITY ? pair(v0, lse) : sl_zero();
            if (lane + 64 < V) r[lane + 64] = v1 > -INFINITY ? pair(v1, lse) : sl_zero();
        }
        SL_BARRIER();
    };
    // the largest exponent of the row, over the whole workgroup (SL_EZERO: the row is all zero); one barrier
    auto row_max = [&](const SlPP* R) {
        int m = SL_EZERO;
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            const int q = tid + nthr * k;
            if (q < H) m = max(m, max(R[q].be, R[q].le));
        }
        m = sl_wave_imax(m);
        if (lane == 0) red[wave] = m;
        SL_BARRIER();
        m = red[0];
#pragma unroll
        for (int w = 1; w < nwave; ++w) m = max(m, red[w]);
        return __builtin_amdgcn_readfirstlane(m);
    };

    const int nblk = (Tb + SL_FB - 1) / SL_FB;
    const SlPP zz{0.0, 0.0, SL_EZERO, SL_EZERO};
    for (int i = tid; i < 2 * (SL_WMAX / 2); i += nthr) (&row[0][0])[i] = zz;
    bool feasible = false;
    SlD p = sl_dzero();
    long long pE = 0;                                   // p = p.m 2^pE
    double dur[NL], num[NL], tail_on[NL], tail_la[NL];   // sums of up to 2^20 terms of which one label may hold most: fp64
    int st[NL], en[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) { dur[k] = num[k] = tail_on[k] = tail_la[k] = 0.0; st[k] = en[k] = 0; }
    auto flush = [&](int k) {                           // the finished label of slot k leaves
        const int i = pi[k];
        if (tid + nthr * k < H && i < L) {
            o_st[i] = min(max(st[k], 0), T);
            o_en[i] = min(max(en[k], 0), T);
            o_du[i] = (float)dur[k];
            o_lc[i] = (float)(SL_LN2 * num[k] / dur[k]);
            num_b[i] = (float)num[k];
        }
        dur[k] = num[k] = tail_on[k] = tail_la[k] = 0.0;
        st[k] = en[k] = 0;
    };

    if (Tb > 0) {
        int lo = sane(lo_b[0], 0);
        lo = __builtin_amdgcn_readfirstlane(lo);
        int base = lo >> 1;
#pragma unroll
        for (int k = 0; k < NL; ++k) describe(k, pair_of(tid + nthr * k, base));
        long long aoff = 0;
        if (tid == 0) { los_b[0] = lo; aoff_b[0] = 0; }
        __syncthreads();

        // ---- forward: alpha rows in the ring, (alpha, f) of the label states to the workspace
        prefetch(0);
        commit(0);
        for (int c = 0; c < nblk; ++c) {
            const int c0 = c * SL_FB, cn = min(SL_FB, Tb - c0);
            SlD edge = sl_dzero();                       // label base - 1 at the frame before the block: dead from here on, but what leaves it counts
            if (c > 0) {                                // the block boundary: renormalise, move the window
                SlPP* R = row[(c0 - 1) & 1];
                const int base_old = base;
                lo = __builtin_amdgcn_readfirstlane(sane(lo_b[c], lo));
                base = lo >> 1;
                if (base > base_old && base - 1 < base_old + H) {            // (read before row_max's barrier: the slot is reused after it)
                    const SlPP v = R[(base - 1) % H];
                    edge = SlD{v.lm, v.le};
                }
                const int M = row_max(R);
                const int sub = M > SL_EZERO ? M : 0;
                aoff += sub;
                edge.e = edge.m > 0.0f || !(edge.m == edge.m) ? max(edge.e - sub, SL_EZERO) : SL_EZERO;
#pragma unroll
                for (int k = 0; k < NL; ++k) {
                    const int q = tid + nthr * k;
                    if (q < H) {
                        const int i = pair_of(q, base);
                        SlPP v = R[q];
                        if (i != pi[k]) {
                            describe(k, i);
                            v = zz;
                        } else {
                            v.be = v.bm > 0.0f || !(v.bm == v.bm) ? max(v.be - sub, SL_EZERO) : SL_EZERO;
                            v.le = v.lm > 0.0f || !(v.lm == v.lm) ? max(v.le - sub, SL_EZERO) : SL_EZERO;
                        }
                        R[q] = v;
                    }
                }
                if (tid == 0) { los_b[c] = lo; aoff_b[c] = aoff; }
                SL_BARRIER();
            }
            if (c + 1 < nblk) prefetch(c + 1);
            for (int tl = 0; tl < cn; ++tl) {
                const int t = c0 + tl, cur = t & 1, prv = cur ^ 1;
                const SlP* y = stage + tl * V;
                const SlP yb = y[blank];
#pragma unroll
                for (int k = 0; k < NL; ++k) {
                    const int q = tid + nthr * k;
                    if (q < H) {
                        const int i = pi[k];
                        SlD nb = sl_dzero(), nl = sl_dzero();
                        float f = 0.0f;
                        if (i <= L) {
                            SlP yl = sl_zero();
                            if (cls[k] >= 0) yl = y[cls[k]];
                            if (t == 0) {
                                nb = i == 0 ? sl_d(yb) : sl_dzero();
                                nl = i == 0 ? sl_d(yl) : sl_dzero();
                                f = 1.0f;
                            } else {
                                const SlPP own = row[prv][q];
                                const SlPP low = row[prv][q == 0 ? H - 1 : q - 1];
                                SlD pm1 = tl == 0 ? edge : sl_dzero();        // label i - 1: dead below the window
                                if (i > base) pm1 = SlD{low.lm, low.le};
                                {                       // blank 2 i: stay, or from label i - 1
                                    const int em = max(own.be, pm1.e);
                                    nb = sl_norm((sl_align(own.bm, own.be - em) + sl_align(pm1.m, pm1.e - em)) * (double)yb.m, em + yb.e);
                                }
                                {                       // label 2 i + 1: stay, from its blank, or from label i - 1 where that is allowed
                                    SlD sk = sl_dzero();
                                    if ((skipin >> k) & 1u) sk = pm1;
                                    const int em = max(max(own.le, own.be), sk.e);
                                    const double stay = sl_align(own.lm, own.le - em);
                                    const double ent = sl_align(own.bm, own.be - em) + sl_align(sk.m, sk.e - em);
                                    const double sum = stay + ent;
                                    nl = sl_norm(sum * (double)yl.m, em + yl.e);
                                    f = sum > 0.0 ? (float)(ent / sum) : 0.0f;
                                }
                            }
                        }
                        row[cur][q] = sl_pp(nb, nl);
                        if (i < L) {
                            const size_t o = (size_t)t * H + q;
                            wa[o] = ((unsigned long long)(unsigned)nl.e << 32) | (unsigned long long)__float_as_uint((float)nl.m);
                            wf[o] = f;
                        }
                    }
                }
                SL_BARRIER();
            }
            if (c + 1 < nblk) commit(c + 1);
        }
        {
            const SlPP* last = row[(Tb - 1) & 1];
            SlD a1 = sl_dzero(), a2 = sl_dzero();         // states n - 1 = blank of pair L, n - 2 = label of pair L - 1, where live
            if (L >= base && L < base + H) { const SlPP v = last[L % H]; a1 = SlD{v.bm, v.be}; }
            if (L >= 1 && L - 1 >= base && L - 1 < base + H) { const SlPP v = last[(L - 1) % H]; a2 = SlD{v.lm, v.le}; }
            const int em = max(a1.e, a2.e);
            p = sl_norm(sl_align(a1.m, a1.e - em) + sl_align(a2.m, a2.e - em), em);
            pE = aoff + p.e;
        }
        feasible = p.m > 0.0f && p.m < INFINITY;
        __threadfence();
        __syncthreads();                                // the row was read; the block table has landed

        // ---- backward: y beta rows in the ring, the posteriors of the label states into registers.  The last block is still staged.
        if (feasible && L > 0) {
            const double rp = 1.0 / p.m;
            long long boff = 0;
            unsigned long long al[NL], aln[NL];
            float fe[NL], fen[NL];
            auto load_af = [&](int t, unsigned long long* a, float* f) {
#pragma unroll
                for (int k = 0; k < NL; ++k) {
                    const int q = tid + nthr * k;
                    a[k] = 0ull;
                    f[k] = 0.0f;
                    if (q < H) { a[k] = sl_ld(wa + (size_t)t * H + q); f[k] = sl_ld(wf + (size_t)t * H + q); }
                }
            };
            load_af(Tb - 1, al, fe);
            for (int c = nblk - 1; c >= 0; --c) {
                const int c0 = c * SL_FB, cn = min(SL_FB, Tb - c0);
                SlPP edge = zz;                         // pair base + H at the frame after the block: where it is live there, what enters it counts
                if (c < nblk - 1) {                     // the block boundary, downwards
                    SlPP* R = row[(c0 + SL_FB) & 1];
                    const int base_old = base;
                    lo = __builtin_amdgcn_readfirstlane(min(max(sl_ld(los_b + c), 0), hi) & ~1);
                    aoff = sl_ld(aoff_b + c);
                    base = lo >> 1;
                    if (base < base_old && base + H >= base_old) edge = R[base % H];      // (before row_max's barrier, as above)
                    const int M = row_max(R);
                    const int sub = M > SL_EZERO ? M : 0;
                    boff += sub;
                    edge.be = edge.bm > 0.0f || !(edge.bm == edge.bm) ? max(edge.be - sub, SL_EZERO) : SL_EZERO;
                    edge.le = edge.lm > 0.0f || !(edge.lm == edge.lm) ? max(edge.le - sub, SL_EZERO) : SL_EZERO;
#pragma unroll
                    for (int k = 0; k < NL; ++k) {
                        const int q = tid + nthr * k;
                        if (q < H) {
                            const int i = pair_of(q, base);
                            SlPP v = R[q];
                            if (i != pi[k]) {
                                flush(k);
                                describe(k, i);
                                v = zz;
                            } else {
                                v.be = v.bm > 0.0f || !(v.bm == v.bm) ? max(v.be - sub, SL_EZERO) : SL_EZERO;
                                v.le = v.lm > 0.0f || !(v.lm == v.lm) ? max(v.le - sub, SL_EZERO) : SL_EZERO;
                            }
                            R[q] = v;
                        }
                    }
                    SL_BARRIER();
                }
                const long long dd = aoff + boff - pE;
                const int D = (int)(dd < -SL_DMAX ? -SL_DMAX : dd > SL_DMAX ? SL_DMAX : dd);
                if (c > 0) prefetch(c - 1);
                for (int tl = cn - 1; tl >= 0; --tl) {
                    const int t = c0 + tl, cur = t & 1, prv = cur ^ 1;
                    const bool first = t == Tb - 1;
                    if (t > 0) load_af(t - 1, aln, fen);
                    const SlP* y = stage + tl * V;
                    const SlP yb = y[blank];
#pragma unroll
                    for (int k = 0; k < NL; ++k) {
                        const int q = tid + nthr * k;
                        if (q < H) {
                            const int i = pi[k];
                            SlD nb = sl_dzero(), nl = sl_dzero();
                            if (i <= L) {
                                SlP yl = sl_zero();
                                if (cls[k] >= 0) yl = y[cls[k]];
                                const double am = (double)__uint_as_float((unsigned)al[k]) * rp;
                                const int ae = min(max((int)(unsigned)(al[k] >> 32), SL_EZERO), -SL_EZERO);       // (what a dead slot holds is anything)
                                double gam, la;
                                if (first) {
                                    nb = i == L ? sl_d(yb) : sl_dzero();
                                    nl = i == L - 1 ? sl_d(yl) : sl_dzero();
                                    gam = la = i == L - 1 ? sl_align(am, ae + D) : 0.0;
                                } else {
                                    const SlPP own = row[prv][q];
                                    SlPP up = row[prv][q == H - 1 ? 0 : q + 1];          // pair i + 1: dead above the window
                                    if (i == base + H - 1) up = tl == cn - 1 ? edge : zz;
                                    {                   // blank 2 i: stay, or on to its label
                                        const int em = max(own.be, own.le);
                                        nb = sl_norm((sl_align(own.bm, own.be - em) + sl_align(own.lm, own.le - em)) * (double)yb.m, em + yb.e);
                                    }
                                    {                   // label 2 i + 1: stay, on to the next blank, or to label i + 1 where that is allowed
                                        SlD sk = sl_dzero();
                                        if ((skipout >> k) & 1u) sk = SlD{up.lm, up.le};
                                        const int em = max(max(own.le, up.be), sk.e);
                                        const double stay = sl_align(own.lm, own.le - em);
                                        const double ou = sl_align(up.bm, up.be - em) + sl_align(sk.m, sk.e - em);
                                        const double sum = stay + ou;                    // beta_t = sum 2^em
                                        nl = sl_norm(sum * (double)yl.m, em + yl.e);
                                        const double g = sl_align(am, ae + em + D);
                                        gam = g * sum;
                                        la = g * ou;
                                    }
                                }
                                if (i < L) {            // the tails hold P(onset >= t + 1) and P(last >= t + 1) here
                                    if (tail_on[k] <= 0.5) st[k] = t;
                                    if (tail_la[k] <= 0.5) en[k] = t + 1;
                                    tail_on[k] += gam * (double)fe[k];
                                    tail_la[k] += la;
                                    dur[k] += gam;
                                    num[k] += gam > 0.0 ? gam * ((double)yl.e + (double)__builtin_amdgcn_logf(yl.m)) : 0.0;
                                }
                            }
                            row[cur][q] = sl_pp(nb, nl);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < NL; ++k) { al[k] = aln[k]; fe[k] = fen[k]; }
                    SL_BARRIER();
                }
                if (c > 0) commit(c - 1);
            }
#pragma unroll
            for (int k = 0; k < NL; ++k) flush(k);     // what is live at t = 0
        }
    } else {
        feasible = L == 0;
    }

    if (tid == 0) {
        double lp = L == 0 ? 0.0 : -INFINITY;           // no frame
        if (Tb > 0) lp = feasible ? ((double)pE + log2((double)p.m)) * SL_LN2 : -INFINITY;
        out.log_prob[b] = lp;
        out.ok[b] = feasible ? 1 : 0;
    }
    // a feasible row has stored every label (each is live somewhere, or p would be zero); the others, and what lies beyond L
    for (int i = tid; i < Lmax; i += nthr) {
        const bool in = i < L;
        if (in && feasible) continue;
        o_st[i] = 0;
        o_en[i] = 0;
        o_du[i] = 0.0f;
        o_lc[i] = in ? -INFINITY : 0.0f;
        num_b[i] = 0.0f;
    }
}

// the words of a row, from what the first launch left: every word is summed by the thread whose chunk holds its first label, in
// label order (K26's rule and K26's conventions for an infeasible row)
__global__ __launch_bounds__(SL_THREADS) void ctc_segment_long_words_kernel(const long long* __restrict__ labels, const int* __restrict__ lab_len,
                                                                            const float* __restrict__ num, SlOut out, int Lmax, long long sep) {
    __shared__ int s_cnt[SL_THREADS];
    constexpr int nthr = SL_THREADS;
    const int b = blockIdx.x, tid = threadIdx.x;
    int L = lab_len ? lab_len[b] : Lmax;
    L = min(max(L, 0), Lmax);
    const int NW = (Lmax + 1) / 2;
    const long long* lab = labels + (size_t)b * Lmax;
    const float* a_dur = out.duration + (size_t)b * Lmax;
    const float* a_num = num + (size_t)b * Lmax;
    const int* a_st = out.start + (size_t)b * Lmax;
    const int* a_en = out.end + (size_t)b * Lmax;
    const bool feasible = out.ok[b] != 0;
    const int chunk = (L + nthr - 1) / nthr;
    const int c0 = min(tid * chunk, L), c1 = min(c0 + chunk, L);
    auto is_start = [&](int i) { return lab[i] != sep && (i == 0 || lab[i - 1] == sep); };
    int mine = 0;
    for (int i = c0; i < c1; ++i) mine += is_start(i);
    s_cnt[tid] = mine;
    __syncthreads();
    int w = 0, total = 0;
    for (int j = 0; j < nthr; ++j) {
        const int c = s_cnt[j];
        if (j < tid) w += c;
        total += c;
    }
    total = min(total, NW);
    for (int i = c0; i < c1; ++i) {
        if (!is_start(i)) continue;
        int j = i;
        double sd = 0.0, sn = 0.0;
        while (j < L && lab[j] != sep) { sd += a_dur[j]; sn += a_num[j]; ++j; }
        if (w < NW) {
            const size_t o = (size_t)b * NW + w;
            out.word_first[o] = i;
            out.word_count[o] = j - i;
            out.word_start[o] = a_st[i];
            out.word_end[o] = a_en[j - 1];
            out.word_log_conf[o] = feasible ? (float)(SL_LN2 * sn / sd) : -INFINITY;
        }
        ++w;
    }
    for (int q = total + tid; q < NW; q += nthr) {
        const size_t o = (size_t)b * NW + q;
        out.word_first[o] = 0; out.word_count[o] = 0; out.word_start[o] = 0; out.word_end[o] = 0; out.word_log_conf[o] = 0.0f;
    }
    if (tid == 0) out.n_words[b] = total;
}

extern "C" int v100_ctc_segment_long_block(void) { return SL_FB; }

static inline long long sl_up16(long long v) { return (v + 15) & ~15LL; }
// per recording: alpha as (m, e) and the entering share f per frame and ring slot; per block the alpha offset and the sanitised lo;
// per label sum gamma log2 y
extern "C" long long v100_ctc_segment_long_workspace_bytes(int B, int T, int Lmax, int band) {
    if (!sl_supported(B, T, Lmax, band)) return 0;
    const long long H = band / 2, NB = sl_blocks(T);
    return (long long)B * T * H * 12 + sl_up16((long long)B * NB * 8) + sl_up16((long long)B * NB * 4) + sl_up16((long long)B * Lmax * 4);
}

extern "C" int v100_ctc_segment_long(const float* logits, const int* in_len, const long long* labels, const int* lab_len, const int* lo,
                                     void* ws, double* log_prob, int* ok, int* start, int* end, float* duration, float* log_conf,
                                     int* word_first, int* word_count, int* word_start, int* word_end, float* word_log_conf, int* n_words,
                                     int B, int T, int V, int Lmax, int band, int blank, long long sep, void* stream) {
    if (!logits || !labels || !lo || !ws || !log_prob || !ok || !start || !end || !duration || !log_conf) return V100_ERR_NULL;
    const int nword = (word_first != nullptr) + (word_count != nullptr) + (word_start != nullptr) + (word_end != nullptr) +
                      (word_log_conf != nullptr) + (n_words != nullptr);
    if (nword != 0 && nword != 6) return V100_ERR_NULL;             // the word level: all six or none
    if (!sl_supported(B, T, Lmax, band) || V < 2 || V > SL_VMAX || blank < 0 || blank >= V) return V100_ERR_SHAPE;
    const SlOut out{log_prob, ok, start, end, duration, log_conf, word_first, word_count, word_start, word_end, word_log_conf, n_words};
    const long long H = band / 2, NB = sl_blocks(T);
    char* base = (char*)ws;
    SlWs w;
    w.a = (unsigned long long*)base;
    base += (long long)B * T * H * 8;
    w.f = (float*)base;
    base += (long long)B * T * H * 4;
    w.aoff = (long long*)base;
    base += sl_up16((long long)B * NB * 8);
    w.lo = (int*)base;
    base += sl_up16((long long)B * NB * 4);
    w.num = (float*)base;
    hipStream_t st = (hipStream_t)stream;
    if (H <= SL_THREADS)
        V100_GGL(ctc_segment_long_kernel<1>, dim3(B), dim3(SL_THREADS), 0, st, logits, in_len, labels, lab_len, lo, w, out, T, V, Lmax, band,
                 blank, (int)NB);
    else
        V100_GGL(ctc_segment_long_kernel<2>, dim3(B), dim3(SL_THREADS), 0, st, logits, in_len, labels, lab_len, lo, w, out, T, V, Lmax, band,
                 blank, (int)NB);
    int rc = v100_launch_status();
    if (rc != V100_OK || nword == 0) return rc;
    V100_GGL(ctc_segment_long_words_kernel, dim3(B), dim3(SL_THREADS), 0, st, labels, lab_len, w.num, out, Lmax, sep);
    return v100_launch_status();
}
