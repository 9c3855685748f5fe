// K26: CTC forward-backward over the alignments of a GIVEN transcript, reduced per label and per word: time boundaries, expected
// durations and the occupancy-weighted mean log posterior of every label over its soft span, one launch.
//
//   z = blank-extended transcript, S = 2 L + 1 states, label i in state 2 i + 1; y_t = softmax(x[t]) (taken by the kernel);
//   alpha_t(s) = sum over path prefixes that end in s at t (emission at t included), p = alpha_{T-1}(S-1) + alpha_{T-1}(S-2);
//   beta_t(s)  = probability of completing from (t, s), emission at t NOT included; gamma_t(s) = alpha_t(s) beta_t(s) / p;
//   duration[i] = sum_t gamma_t(s_i), log_confidence[i] = sum_t gamma_t(s_i) log y_t(l_i) / duration[i];
//   P(onset_i = t) = gamma_t(s_i) f_t(s_i), f = the share of alpha_t(s_i) that ENTERED s_i at t (not the stay);
//   P(last_i = t)  = alpha_t(s_i) o_t(s_i) / p, o = beta_t without the stay term; start / end = the medians of the two.
//
// One workgroup of 256 threads per utterance.  A thread owns PAIRS of states: pair i = (blank 2 i, label 2 i + 1), i = tid + 256 k,
// k < NL; pair L is the last blank and a phantom label of probability zero.  (Ownership by s mod 256 would put every label state,
// and with it every accumulator, on the odd threads.)
//
// Numbers.  A probability is a pair (m, e) = m 2^e: m an fp32 in [1/2, 1) (or 0), e an integer held in an fp32 (exact to 2^24; a
// whole utterance needs < 2^20).  A sum aligns its terms to the largest exponent (v_ldexp), adds, and renormalises (v_frexp); a
// product multiplies the m and adds the e.  Every step has the RELATIVE error of one fp32 operation whatever the magnitude, the
// exponents never round, and the recursion holds no exp or log.  (The first build kept fp32 logs less the row's maximum: where the
// posterior sits hundreds of nats below the row's best state -- logits of scale 10, many more frames than labels -- the stored log
// itself rounds at 3e-5 a frame and the durations were off by up to 1e-2; see DESIGN.md.)  So gamma = (A.m B.m / p.m) 2^(A.e + B.e
// - p.e) needs no offsets carried beside the rows.  The emissions are staged as such pairs: the log2-softmax with the product
// d log2(e) carried in two floats, split into integer and fraction, exp2 of the fraction.
//
// A frame's row lives in LDS (two rows of float2, guard cells of zero); the emissions of 16 frames are staged in LDS -- raw logits
// prefetched into registers a block ahead, the softmax taken in place by a wave per frame; the one barrier per frame waits for LDS
// only, so the lattice stores and the prefetches stay in flight across it.  Forward: writes, per label state, alpha and f to the
// workspace.  Backward: keeps the rows y_t(z_s) beta_t(s) in LDS, reads (alpha, f) back a frame ahead (the same thread wrote them),
// and accumulates per owned label in registers: duration, sum gamma log2 y, and the tail sums P(onset >= t + 1), P(last >= t + 1).
// Descending in t the tails grow monotonically: while a tail is <= 1/2 the frame is a candidate, the last such frame is the median --
// one compare per frame and label.  No cross-state scan, no float atomics: two runs give equal bits.  Words (maximal runs of labels
// != sep) are summed at the end through LDS, every word by one thread in label order.
//
// Every loop is bounded by T, L, V or the thread count and no index depends on a float, so a row of NaNs ends like any other.
#include "common.h"
#include <math.h>

#define SG_FB 16                                        // frames per staged block of emissions
#define SG_VMAX 128
#define SG_TMAX 4096
#define SG_LMAX 2047
#define SG_THREADS 256
#define SG_PF (SG_FB * SG_VMAX / SG_THREADS)            // prefetch registers a thread
#define SG_LOG2E 1.44269504089f
#define SG_LOG2E_LO 1.92596299e-8f                      // log2(e) less its fp32
#define SG_LN2 0.69314718056
#define SG_EZERO (-1.0e9f)                              // the exponent of zero: below every sum's largest term
#define SG_ZERO make_float2(0.0f, SG_EZERO)

// LDS-only barrier: the LDS traffic of every wave has landed; global loads and the lattice stores stay in flight
#define SG_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

#define SG_DPP(old, v, ctrl, rows, fill) __builtin_amdgcn_update_dpp(old, v, ctrl, rows, 0xf, fill)
__device__ __forceinline__ float sg_wave_max(float v) {
    const int ninf = __builtin_bit_cast(int, -INFINITY);
#define SG_MAXSTEP(ctrl, rows) v = fmaxf(v, __builtin_bit_cast(float, SG_DPP(ninf, __builtin_bit_cast(int, v), ctrl, rows, false)))
    SG_MAXSTEP(0x111, 0xf); SG_MAXSTEP(0x112, 0xf); SG_MAXSTEP(0x114, 0xf); SG_MAXSTEP(0x118, 0xf);
    SG_MAXSTEP(0x142, 0xa); SG_MAXSTEP(0x143, 0xc);
#undef SG_MAXSTEP
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));      // lane 63 has seen every lane
}
__device__ __forceinline__ float sg_wave_total(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wave_sum_dpp_hi(v)), 63));
}

// m 2^e with the exponent difference d = e - (the sum's largest e) <= 0; below -200 the term is nothing (and NaN counts as that)
__device__ __forceinline__ float sg_align(float m, float d) { return ldexpf(m, (int)fminf(fmaxf(d, -200.0f), 200.0f)); }
// v 2^e, v >= 0 finite or NaN -> (m, e') with m in [1/2, 1); zero keeps the exponent of zero
__device__ __forceinline__ float2 sg_norm(float v, float e) {
    const float m = __builtin_amdgcn_frexp_mantf(v);
    return make_float2(m, v > 0.0f ? e + (float)__builtin_amdgcn_frexp_expf(v) : SG_EZERO);
}

struct SgOut {
    float* log_prob; int* start; int* end; float* duration; float* log_conf;
    int* word_first; int* word_count; int* word_start; int* word_end; float* word_log_conf; int* n_words;
};

template <int NL>
__global__ __launch_bounds__(SG_THREADS) void ctc_segment_kernel(const float* __restrict__ logits, const int* __restrict__ in_len,
                                                                 const long long* __restrict__ labels, const int* __restrict__ lab_len,
                                                                 float2* ws_a, float* ws_f, SgOut out, int T, int V, int Lmax,
                                                                 int blank, long long sep) {
    extern __shared__ __attribute__((aligned(16))) float2 sg_smem[];
    __shared__ int s_cnt[SG_THREADS];
    constexpr int RS = 512 * NL + 8;                    // a row: 2 guard cells, <= 512 NL states, guard cells
    constexpr int nthr = SG_THREADS, nwave = SG_THREADS / 64;
    float2* row = sg_smem;                              // [2][RS] (m, e); state s at index 2 + s
    float2* stage = row + 2 * RS;                       // [SG_FB][V] the emissions of the staged frames as (m, e)

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int Tb = in_len ? in_len[b] : T;
    Tb = __builtin_amdgcn_readfirstlane(min(max(Tb, 0), T));
    int L = lab_len ? lab_len[b] : Lmax;
    L = __builtin_amdgcn_readfirstlane(min(max(L, 0), Lmax));
    const float* x = logits + (size_t)b * T * V;
    const long long* lab = labels + (size_t)b * Lmax;
    float2* wa = ws_a + (size_t)b * T * Lmax;
    float* wf = ws_f + (size_t)b * T * Lmax;
    const bool words = out.word_first != nullptr;
    const int NW = (Lmax + 1) / 2;

    for (int i = tid; i < 2 * RS; i += nthr) row[i] = SG_ZERO;

    // the class of each owned label (-1: none, blank or out of range: probability zero) and the two skip permissions
    int cls[NL];
    unsigned skipin = 0u, skipout = 0u;                 // bit k: label i may be entered from label i - 1 / may skip to label i + 1
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        const int i = tid + nthr * k;
        cls[k] = -1;
        if (i < L) {
            const long long c = lab[i];
            if (c >= 0 && c < V && c != blank) cls[k] = (int)c;
            if (i >= 1 && lab[i - 1] != c) skipin |= 1u << k;
            if (i + 1 < L && lab[i + 1] != c) skipout |= 1u << k;
        }
    }

    float pf[SG_PF];
    auto prefetch = [&](int c) {                        // raw logits of block c into registers
        const int c0 = c * SG_FB, cnt = min(SG_FB, Tb - c0) * V;
        const float* src = x + (size_t)c0 * V;
#pragma unroll
        for (int j = 0; j < SG_PF; ++j) {
            const int idx = tid + j * nthr;
            pf[j] = idx < cnt ? src[idx] : 0.0f;
        }
    };
    auto commit = [&](int c) {                          // ... into the stage, then the softmax in place; every wave is past the last
        const int c0 = c * SG_FB, cn = min(SG_FB, Tb - c0), cnt = cn * V;       // read of the stage (the frame's barrier)
#pragma unroll
        for (int j = 0; j < SG_PF; ++j) {
            const int idx = tid + j * nthr;
            if (idx < cnt) stage[idx].x = pf[j];
        }
        SG_BARRIER();
        for (int fr = wave; fr < cn; fr += nwave) {
            float2* r = stage + fr * V;
            const float v0 = lane < V ? r[lane].x : -INFINITY, v1 = lane + 64 < V ? r[lane + 64].x : -INFINITY;
            const float mx = sg_wave_max(fmaxf(v0, v1));
            auto pair = [&](float v, float lse) {       // log2 y = (v - mx) log2(e) - lse as integer + fraction, y = exp2(fraction) 2^integer
                const float d = v - mx, hi = d * SG_LOG2E;
                const float lo = fmaf(d, SG_LOG2E_LO, fmaf(d, SG_LOG2E, -hi));
                const float e = floorf(hi - lse);
                const float y = __builtin_amdgcn_exp2f(((hi - e) - lse) + lo);          // the fraction is in about [0, 1]
                return y > 0.0f || !(y == y) ? sg_norm(y, e) : SG_ZERO;
            };
            const float d0 = (v0 - mx) * SG_LOG2E, d1 = (v1 - mx) * SG_LOG2E;
            const float total = sg_wave_total((lane < V ? __builtin_amdgcn_exp2f(d0) : 0.0f) +
                                              (lane + 64 < V ? __builtin_amdgcn_exp2f(d1) : 0.0f));
            const float lse = __builtin_amdgcn_logf(total);
            if (lane < V) r[lane] = v0 > -INFINITY ? pair(v0, lse) : SG_ZERO;
            if (lane + 64 < V) r[lane + 64] = v1 > -INFINITY ? pair(v1, lse) : SG_ZERO;
        }
        SG_BARRIER();
    };

    const int nblk = (Tb + SG_FB - 1) / SG_FB;
    bool feasible = false;
    float2 p = SG_ZERO;
    float dur[NL], num[NL], tail_on[NL], tail_la[NL];
    int st[NL], en[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) { dur[k] = num[k] = tail_on[k] = tail_la[k] = 0.0f; st[k] = en[k] = 0; }
    __syncthreads();

    if (Tb > 0) {
        // ---- forward: alpha rows in LDS, (alpha, f) of the label states to the workspace
        prefetch(0);
        commit(0);
        for (int c = 0; c < nblk; ++c) {
            const int c0 = c * SG_FB, cn = min(SG_FB, Tb - c0);
            if (c + 1 < nblk) prefetch(c + 1);
            for (int tl = 0; tl < cn; ++tl) {
                const int t = c0 + tl, cur = t & 1, prv = cur ^ 1;
                const float2* y = stage + tl * V;
                const float2 yb = y[blank];
#pragma unroll
                for (int k = 0; k < NL; ++k) {
                    const int i = tid + nthr * k;
                    if (i <= L) {
                        float2 yl = SG_ZERO;
                        if (cls[k] >= 0) yl = y[cls[k]];
                        float2 nb, nl;
                        float f;
                        if (t == 0) {
                            nb = i == 0 ? yb : SG_ZERO;
                            nl = i == 0 ? yl : SG_ZERO;
                            f = 1.0f;
                        } else {
                            const float2* P = row + prv * RS + 2 + 2 * i;
                            const float2 pm1 = P[-1];
                            const float4 p01 = *(const float4*)P;            // blank 2 i (x, y), label 2 i + 1 (z, w)
                            {                           // blank 2 i: stay, or from label i - 1
                                const float em = fmaxf(p01.y, pm1.y);
                                nb = sg_norm((sg_align(p01.x, p01.y - em) + sg_align(pm1.x, pm1.y - em)) * yb.x, em + yb.y);
                            }
                            {                           // label 2 i + 1: stay, from its blank, or from label i - 1 where that is allowed
                                float2 sk = SG_ZERO;
                                if ((skipin >> k) & 1u) sk = pm1;
                                const float em = fmaxf(fmaxf(p01.w, p01.y), sk.y);
                                const float stay = sg_align(p01.z, p01.w - em);
                                const float ent = sg_align(p01.x, p01.y - em) + sg_align(sk.x, sk.y - em);
                                const float sum = stay + ent;
                                nl = sg_norm(sum * yl.x, em + yl.y);
                                f = sum > 0.0f ? ent / sum : 0.0f;
                            }
                        }
                        *(float4*)(row + cur * RS + 2 + 2 * i) = make_float4(nb.x, nb.y, nl.x, nl.y);
                        if (i < L) {
                            wa[(size_t)t * Lmax + i] = nl;
                            wf[(size_t)t * Lmax + i] = f;
                        }
                    }
                }
                SG_BARRIER();
            }
            if (c + 1 < nblk) commit(c + 1);
        }
        {
            const float2* last = row + ((Tb - 1) & 1) * RS + 2;
            const float2 a1 = last[2 * L], a2 = last[2 * L - 1];     // L = 0: the guard cell
            const float em = fmaxf(a1.y, a2.y);
            p = sg_norm(sg_align(a1.x, a1.y - em) + sg_align(a2.x, a2.y - em), em);
        }
        feasible = p.x > 0.0f && p.x < INFINITY;
        SG_BARRIER();                                   // the backward pass writes the row that was just read

        // ---- backward: y beta rows in LDS, the posteriors of the label states into registers.  The last block is still staged.
        if (feasible && L > 0) {
            const float rp = 1.0f / p.x;
            float2 al[NL], aln[NL];
            float fe[NL], fen[NL];
            auto load_af = [&](int t, float2* a, float* f) {
#pragma unroll
                for (int k = 0; k < NL; ++k) {
                    const int i = tid + nthr * k;
                    a[k] = SG_ZERO;
                    f[k] = 0.0f;
                    if (i < L) { a[k] = wa[(size_t)t * Lmax + i]; f[k] = wf[(size_t)t * Lmax + i]; }
                }
            };
            load_af(Tb - 1, al, fe);
            for (int c = nblk - 1; c >= 0; --c) {
                const int c0 = c * SG_FB, cn = min(SG_FB, Tb - c0);
                if (c > 0) prefetch(c - 1);
                for (int tl = cn - 1; tl >= 0; --tl) {
                    const int t = c0 + tl, cur = t & 1, prv = cur ^ 1;
                    const bool first = t == Tb - 1;
                    if (t > 0) load_af(t - 1, aln, fen);
                    const float2* y = stage + tl * V;
                    const float2 yb = y[blank];
#pragma unroll
                    for (int k = 0; k < NL; ++k) {
                        const int i = tid + nthr * k;
                        if (i <= L) {
                            float2 yl = SG_ZERO;
                        if (cls[k] >= 0) yl = y[cls[k]];
                            float2 nb, nl;
                            float gam, la;
                            if (first) {
                                nb = i == L ? yb : SG_ZERO;
                                nl = i == L - 1 ? yl : SG_ZERO;
                                gam = la = i == L - 1 ? sg_align(al[k].x * rp, al[k].y - p.y) : 0.0f;
                            } else {
                                const float4* Q = (const float4*)(row + prv * RS + 2 + 2 * i);
                                const float4 q01 = Q[0], q23 = Q[1];         // blank 2 i, label 2 i + 1; the next pair's
                                {                       // blank 2 i: stay, or on to its label
                                    const float em = fmaxf(q01.y, q01.w);
                                    nb = sg_norm((sg_align(q01.x, q01.y - em) + sg_align(q01.z, q01.w - em)) * yb.x, em + yb.y);
                                }
                                {                       // label 2 i + 1: stay, on to the next blank, or to label i + 1 where that is allowed
                                    float2 sk = SG_ZERO;
                                    if ((skipout >> k) & 1u) sk = make_float2(q23.z, q23.w);
                                    const float em = fmaxf(fmaxf(q01.w, q23.y), sk.y);
                                    const float stay = sg_align(q01.z, q01.w - em);
                                    const float ou = sg_align(q23.x, q23.y - em) + sg_align(sk.x, sk.y - em);
                                    const float sum = stay + ou;                 // beta_t = sum 2^em
                                    nl = sg_norm(sum * yl.x, em + yl.y);
                                    const float g = sg_align(al[k].x * rp, al[k].y + em - p.y);
                                    gam = g * sum;
                                    la = g * ou;
                                }
                            }
                            *(float4*)(row + cur * RS + 2 + 2 * i) = make_float4(nb.x, nb.y, nl.x, nl.y);
                            if (i < L) {                // the tails hold P(onset >= t + 1) and P(last >= t + 1) here
                                if (tail_on[k] <= 0.5f) st[k] = t;
                                if (tail_la[k] <= 0.5f) en[k] = t + 1;
                                tail_on[k] += gam * fe[k];
                                tail_la[k] += la;
                                dur[k] += gam;
                                num[k] += gam > 0.0f ? gam * (yl.y + __builtin_amdgcn_logf(yl.x)) : 0.0f;
                            }
                        }
                    }
#pragma unroll
                    for (int k = 0; k < NL; ++k) { al[k] = aln[k]; fe[k] = fen[k]; }
                    SG_BARRIER();
                }
                if (c > 0) commit(c - 1);
            }
        }
    } else {
        feasible = L == 0;
    }
    __syncthreads();

    // ---- per label, and through LDS (the rows' space) for the words
    if (tid == 0) {
        float lp = L == 0 ? 0.0f : -INFINITY;           // no frame
        if (Tb > 0) lp = feasible ? (float)(((double)p.y + log2((double)p.x)) * SG_LN2) : -INFINITY;
        out.log_prob[b] = lp;
    }
    float* a_dur = (float*)row;                         // [256 NL] each
    float* a_num = a_dur + 256 * NL;
    int* a_st = (int*)(a_num + 256 * NL);
    int* a_en = a_st + 256 * NL;
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        const int i = tid + nthr * k;
        if (i < L) {
            a_dur[i] = feasible ? dur[k] : 0.0f;
            a_num[i] = feasible ? num[k] : 0.0f;
            a_st[i] = feasible ? min(max(st[k], 0), T) : 0;
            a_en[i] = feasible ? min(max(en[k], 0), T) : 0;
        }
    }
    __syncthreads();
    for (int i = tid; i < Lmax; i += nthr) {
        const size_t o = (size_t)b * Lmax + i;
        const bool in = i < L;
        out.start[o] = in ? a_st[i] : 0;
        out.end[o] = in ? a_en[i] : 0;
        out.duration[o] = in ? a_dur[i] : 0.0f;
        out.log_conf[o] = in ? (feasible ? (float)SG_LN2 * a_num[i] / a_dur[i] : -INFINITY) : 0.0f;
    }
    if (!words) return;
    // a word = a maximal run of labels != sep inside the row's length; every word is summed by the thread whose chunk holds its first
    // label, in label order
    const int chunk = (L + nthr - 1) / nthr;
    const int c0 = min(tid * chunk, L), c1 = min(c0 + chunk, L);
    auto is_start = [&](int i) { return lab[i] != sep && (i == 0 || lab[i - 1] == sep); };
    int mine = 0;
    for (int i = c0; i < c1; ++i) mine += is_start(i);
    s_cnt[tid] = mine;
    __syncthreads();
    int w = 0, total = 0;
    for (int j = 0; j < nthr; ++j) {
        const int n = s_cnt[j];
        if (j < tid) w += n;
        total += n;
    }
    total = min(total, NW);
    for (int i = c0; i < c1; ++i) {
        if (!is_start(i)) continue;
        int j = i;
        float sd = 0.0f, sn = 0.0f;
        while (j < L && lab[j] != sep) { sd += a_dur[j]; sn += a_num[j]; ++j; }
        if (w < NW) {
            const size_t o = (size_t)b * NW + w;
            out.word_first[o] = i;
            out.word_count[o] = j - i;
            out.word_start[o] = a_st[i];
            out.word_end[o] = a_en[j - 1];
            out.word_log_conf[o] = feasible ? (float)SG_LN2 * sn / sd : -INFINITY;
        }
        ++w;
    }
    for (int q = total + tid; q < NW; q += nthr) {
        const size_t o = (size_t)b * NW + q;
        out.word_first[o] = 0; out.word_count[o] = 0; out.word_start[o] = 0; out.word_end[o] = 0; out.word_log_conf[o] = 0.0f;
    }
    if (tid == 0) out.n_words[b] = total;
}

static inline bool sg_shape_ok(int B, int T, int Lmax) {
    return B >= 1 && T >= 1 && T <= SG_TMAX && Lmax >= 1 && Lmax <= SG_LMAX;
}

extern "C" int v100_ctc_segment_block(void) { return SG_FB; }

// per utterance, frame and label: alpha as (m, e) and the entering share f
extern "C" long long v100_ctc_segment_workspace_bytes(int B, int T, int Lmax) {
    if (!sg_shape_ok(B, T, Lmax)) return -1;
    return (long long)B * T * Lmax * (long long)(sizeof(float2) + sizeof(float));
}

template <int NL>
static int sg_launch(size_t shmem, hipStream_t st, const float* logits, const int* in_len, const long long* labels,
                     const int* lab_len, void* ws, const SgOut& out, int B, int T, int V, int Lmax, int blank, long long sep) {
    if (shmem > 65536 &&
        hipFuncSetAttribute((const void*)ctc_segment_kernel<NL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem) != hipSuccess)
        return V100_ERR_LAUNCH;
    float2* ws_a = (float2*)ws;
    float* ws_f = (float*)(ws_a + (size_t)B * T * Lmax);
    V100_GGL(ctc_segment_kernel<NL>, dim3(B), dim3(SG_THREADS), shmem, st, logits, in_len, labels, lab_len, ws_a, ws_f, out, T, V, Lmax,
             blank, sep);
    return v100_launch_status();
}

extern "C" int v100_ctc_segment(const float* logits, const int* in_len, const long long* labels, const int* lab_len, void* ws,
                                float* log_prob, int* start, int* end, float* duration, float* log_conf, int* word_first,
                                int* word_count, int* word_start, int* word_end, float* word_log_conf, int* n_words, int B, int T, int V,
                                int Lmax, int blank, long long sep, void* stream) {
    if (!logits || !labels || !ws || !log_prob || !start || !end || !duration || !log_conf) return V100_ERR_NULL;
    const int nword = (word_first != nullptr) + (word_count != nullptr) + (word_start != nullptr) + (word_end != nullptr) +
                      (word_log_conf != nullptr) + (n_words != nullptr);
    if (nword != 0 && nword != 6) return V100_ERR_NULL;             // the word level: all six or none
    if (!sg_shape_ok(B, T, Lmax) || V < 2 || V > SG_VMAX || blank < 0 || blank >= V) return V100_ERR_SHAPE;
    const SgOut out{log_prob, start, end, duration, log_conf, word_first, word_count, word_start, word_end, word_log_conf, n_words};
    const int pairs = Lmax + 1;                         // <= 2048
    const int NL = pairs <= 256 ? 1 : pairs <= 512 ? 2 : pairs <= 1024 ? 4 : 8;
    const size_t shmem = (size_t)(2 * (512 * NL + 8) + SG_FB * V) * sizeof(float2);                // 8 states a thread: up to 80.1 KiB
    hipStream_t st = (hipStream_t)stream;
#define SG_LAUNCH(NL_) sg_launch<NL_>(shmem, st, logits, in_len, labels, lab_len, ws, out, B, T, V, Lmax, blank, sep)
    if (NL == 1) return SG_LAUNCH(1);
    if (NL == 2) return SG_LAUNCH(2);
    if (NL == 4) return SG_LAUNCH(4);
    return SG_LAUNCH(8);
#undef SG_LAUNCH
}
