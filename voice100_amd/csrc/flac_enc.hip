// K30: FLAC encoded on the device, a batch of utterances (or segments of one long row) per call, four launches.
//
//   a. flac_enc_analyze_kernel  one workgroup per (frame, signal): mono has one signal, stereo four (L, R, M = (L+R)>>1, S = L-R).
//                               Samples are quantised (floats: clamp(rint(x 2^(bps-1))), ties to even) or taken as int32 PCM, wasted
//                               bits are removed, and every candidate is COSTED EXACTLY: constant, verbatim, fixed orders 0-4, LPC
//                               orders 1..max_lpc_order, each over Rice parameters 0-14 and partition orders 0..max_partition_order.
//                               The winner's choices go to a plan record; residuals are not kept.
//   b. flac_enc_layout_kernel   one workgroup: per frame the cheapest of independent, left/side, side/right and mid/side, the exact
//                               frame size in bytes, and an exclusive scan of those sizes = every frame's byte offset.
//   c. flac_enc_pack_kernel     one workgroup per frame: residuals are recomputed from the plan; every lane owns chunks of 32 samples
//                               whose bit ranges are known from a scan of their exact bit counts, and writes them MSB-first into the
//                               zeroed output.  Neighbouring ranges meet only in boundary words, which are OR-ed atomically.
//   d. flac_enc_crc_kernel      one wave per frame: CRC-16 of the frame, 64 slices combined by multiplication with x^(8 len) mod P.
//
// Candidate order (ties go to the FIRST): constant, verbatim, fixed 0, 1, 2, 3, 4, LPC 1, 2, ...; within a candidate the smallest
// partition order, within a partition the smallest Rice parameter; stereo: independent, left/side, side/right, mid/side.
// A candidate is dropped when its order >= the frame's length or a residual leaves (-2^31, 2^31); partition order p > 0 needs
// 2^p | length and length >> p > order.  Cost of a partition = sum(u >> k) + (1 + k) n + 4 with u the zig-zag residual: additive, so
// the finest partitioning's sums give every coarser one.  Hence no subframe is larger than verbatim or than the best fixed predictor.
//
// LPC analysis, bit-reproducible by tests/_flac_enc_ref.py: autocorrelation in exact int64 of (x >> max(0, width - 16)) times an
// integer Welch window 256 (D^2 - d^2) / D^2, d = 2i - (n - 1), D = n + 1; Levinson-Durbin in fp64 with + - x / only and contraction
// off; shift from the exponent bits of the largest coefficient; floor(v + 0.5) with error feedback, clamped to the precision (by
// block size: 7 bits up to 192 samples ... 12 bits up to 4608); shift clamped to 15, a negative shift drops the candidate.
// Prediction sums run in 32 bits where width + precision + ceil(log2 order) <= 32 and in 64 bits elsewhere.
//
// Every phase below is "for every thread t: body; barrier", and all state that crosses a barrier lives in the shared struct, so
// FLAC_ENC_HOST_EMU compiles the same bodies as plain C++ (a loop over t per phase) for host-side checking under a sanitizer; the
// library build never defines it.
#ifdef FLAC_ENC_HOST_EMU
#include <stdint.h>
#include <string.h>
#include <math.h>
#define FD static inline
#define FE_PAR(T, ...) { for (int t = 0; t < (T); ++t) { __VA_ARGS__ } }
#define FE_ADD64(p, v) (*(p) += (v))
#define FE_OR(p, v) (*(p) |= (v))
#define FE_XOR(p, v) (*(p) ^= (v))
#define FE_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#else
#include "common.h"
#define FD __device__ __forceinline__
#define FE_PAR(T, ...) { { const int t = threadIdx.x; __VA_ARGS__ } __syncthreads(); }
#define FE_ADD64(p, v) atomicAdd((p), (v))
#define FE_OR(p, v) atomicOr((p), (v))
#define FE_XOR(p, v) atomicXor((p), (v))
#define FE_MAX(p, v) atomicMax((p), (v))
#endif

#define FE_T 256             // threads of the analyze and pack workgroups
#define FE_LT 1024           // threads of the layout workgroup
#define FE_MAXBS 4608        // FLAC's subset limit at <= 48 kHz; two channels of it fit the LDS
#define FE_MAXPO 6
#define FE_MAXP (1 << FE_MAXPO)
#define FE_MAXORD 12
#define FE_NK 15             // Rice parameters 0 .. 14 (15 is the escape code)
#define FE_NCAND (5 + FE_MAXORD)
#define FE_CHUNK 32          // samples per packing unit
#define FE_PLAN 36           // ints per plan record
#define FE_FTAB 8            // ints per frame-table row
enum { FF_ROW, FF_START, FF_N, FF_NUM, FF_ITEM };
enum { PL_TYPE, PL_ORDER, PL_WASTED, PL_PORDER, PL_PREC, PL_SHIFT, PL_BITS, PL_WIDTH, PL_COEF = 8, PL_PARAM = 20 };
enum { PT_CONSTANT, PT_VERBATIM, PT_FIXED, PT_LPC };
enum { FR_ASSIGN, FR_HLEN, FR_BYTES, FR_BITS };
// per-item status [B][2]: code, then 0x7FFFFFFF - (the smallest sample index within the item)
enum { FES_OK, FES_NONFINITE, FES_RANGE, FES_INTERNAL, FES_TABLE };

struct FeArgs {
    const float* xf;         // [R][C][N] or NULL
    const int* xi;           // [R][C][N] or NULL
    long long N;
    int R, C, bps, block_size, max_lpc, max_po, B, F, rate_code, rate_extra;
};

FD int fe_sample(const FeArgs& a, int row, int ch, long long pos, int* st, int idx) {
    const int hi = (1 << (a.bps - 1)) - 1, lo = -hi - 1;
    const long long at = ((long long)row * a.C + ch) * a.N + pos;
    int q = 0, code = 0;
    if (a.xf) {
        const float v = a.xf[at];
        unsigned u;
        __builtin_memcpy(&u, &v, 4);
        if ((u & 0x7F800000u) == 0x7F800000u) code = FES_NONFINITE;
        else {
            float s = v * (float)(1 << (a.bps - 1));                   // exact: a power of two
            s = s < (float)lo ? (float)lo : s > (float)hi ? (float)hi : s;
            q = (int)__builtin_rintf(s);                                // ties to even
        }
    } else {
        q = a.xi[at];
        if (q < lo || q > hi) { code = FES_RANGE; q = q < lo ? lo : hi; }
    }
    if (code) { FE_MAX(&st[0], code); FE_MAX(&st[1], 0x7FFFFFFF - idx); }
    return q;
}

// signal s of a frame at sample i: 0 L (or mono), 1 R, 2 M, 3 S
FD int fe_signal(const FeArgs& a, const int* __restrict__ fr, int s, int i, int* status) {
    const long long pos = (long long)fr[FF_START] + i;
    int* st = status + 2 * fr[FF_ITEM];
    const int idx = fr[FF_NUM] * a.block_size + i;
    if (s == 0) return fe_sample(a, fr[FF_ROW], 0, pos, st, idx);
    if (s == 1) return fe_sample(a, fr[FF_ROW], 1, pos, st, idx);
    const int l = fe_sample(a, fr[FF_ROW], 0, pos, st, idx), r = fe_sample(a, fr[FF_ROW], 1, pos, st, idx);
    return s == 2 ? (l + r) >> 1 : l - r;
}

FD bool fe_frame_ok(const FeArgs& a, const int* __restrict__ fr) {
    return fr[FF_ROW] >= 0 && fr[FF_ROW] < a.R && fr[FF_START] >= 0 && fr[FF_N] >= 1 && fr[FF_N] <= a.block_size &&
           (long long)fr[FF_START] + fr[FF_N] <= a.N && fr[FF_ITEM] >= 0 && fr[FF_ITEM] < a.B && fr[FF_NUM] >= 0 &&
           (long long)fr[FF_NUM] * a.block_size + fr[FF_N] < (1ll << 31);
}

FD int fe_precision(int block_size) {
    return block_size <= 192 ? 7 : block_size <= 384 ? 8 : block_size <= 576 ? 9 : block_size <= 1152 ? 10 : block_size <= 2304 ? 11 : 12;
}
FD int fe_ctz(unsigned v) { return v ? __builtin_ctz(v) : 32; }
FD int fe_fixed_coef(int order, int j) {
    const unsigned wd = order == 1 ? 0x00000001u : order == 2 ? 0x0000FF02u : order == 3 ? 0x0001FD03u : 0xFF04FA04u;
    return (j < order && j < 4) ? (int)(signed char)(wd >> (8 * j)) : 0;
}
FD int fe_window(int i, int n) {                                        // 0 .. 256, integer arithmetic only
    const long long d = 2ll * i - (n - 1), D = (long long)n + 1;
    return (int)((256 * (D * D - d * d)) / (D * D));
}

// ---- a. analyze ---------------------------------------------------------------------------------------------------------------
struct FeAnalyze {
    int xs[FE_MAXBS];                                   // the signal, wasted bits removed
    int xw[FE_MAXBS];                                   // (xs >> down) x window
    unsigned long long psum[FE_MAXP * FE_NK];           // [finest partition][k] = sum(u >> k); merged in place level by level
    unsigned long long ltot[FE_MAXPO + 1];              // bits of the residual section at each partition order
    unsigned long long ac[FE_MAXORD + 1];               // autocorrelation (two's complement int64)
    double lpc[FE_MAXORD];
    unsigned char lparam[FE_MAXPO + 1][FE_MAXP];
    unsigned char bparam[FE_MAXP];
    int ccoef[FE_NCAND][FE_MAXORD], corder[FE_NCAND], cshift[FE_NCAND], cok[FE_NCAND];
    int bcoef[FE_MAXORD];
    int best[8];
    unsigned orall;
    int cbad[FE_NCAND], ctake[FE_NCAND];                // per candidate, so that no flag is reset while a wave still reads it
    int diff, take_p;
};

// thread 0: Levinson-Durbin on S.ac, and the quantised predictor of every order 1 .. maxo into candidates 5 ..
FD void fe_levinson(FeAnalyze& S, int maxo, int prec) {
#pragma clang fp contract(off)
    for (int m = 0; m < FE_MAXORD; ++m) S.cok[5 + m] = 0;
    if ((long long)S.ac[0] <= 0) return;
    double err = (double)(long long)S.ac[0];
    for (int m = 0; m < maxo; ++m) {
        double acc = (double)(long long)S.ac[m + 1];
        for (int j = 0; j < m; ++j) acc = acc - S.lpc[j] * (double)(long long)S.ac[m - j];
        const double k = acc / err;
        S.lpc[m] = k;
        for (int j = 0; j < (m >> 1); ++j) {
            const double a = S.lpc[j], b = S.lpc[m - 1 - j];
            S.lpc[j] = a - k * b;
            S.lpc[m - 1 - j] = b - k * a;
        }
        if (m & 1) S.lpc[m >> 1] = S.lpc[m >> 1] - S.lpc[m >> 1] * k;
        err = err * (1.0 - k * k);
        // quantise the order m + 1 predictor
        double cmax = 0.0;
        for (int j = 0; j <= m; ++j) {
            const double v = S.lpc[j] < 0.0 ? 0.0 - S.lpc[j] : S.lpc[j];
            if (v > cmax) cmax = v;
        }
        unsigned long long cb;
        __builtin_memcpy(&cb, &cmax, 8);
        const int ef = (int)((cb >> 52) & 0x7FF);
        int shift = prec - (ef - 1023) - 2;
        if (ef != 0 && ef != 0x7FF && shift >= 0) {
            if (shift > 15) shift = 15;
            const double scale = (double)(1 << shift), lo = 0.0 - (double)(1 << (prec - 1)), hi = (double)((1 << (prec - 1)) - 1);
            double e = 0.0;
            for (int j = 0; j <= m; ++j) {
                e = e + S.lpc[j] * scale;
                double q = __builtin_floor(e + 0.5);
                q = q < lo ? lo : q > hi ? hi : q;
                e = e - q;
                S.ccoef[5 + m][j] = (int)q;
            }
            S.corder[5 + m] = m + 1;
            S.cshift[5 + m] = shift;
            S.cok[5 + m] = 1;
        }
        if (!(err > 0.0)) return;
    }
}

template <typename ACC>
FD void fe_partition_sums(FeAnalyze& S, int t, int n, int pmax, int order, int shift, const int* coef, int* badflag) {
    const int P = 1 << pmax, plen = n >> pmax;
    const int G = (FE_T / P) < 64 ? (FE_T / P) : 64;
    const int g = t / G, l = t - g * G;
    if (g >= P) return;
    int lo = g * plen;
    const int hi = lo + plen;
    if (lo < order) lo = order;
    unsigned long long s[FE_NK];
#pragma unroll
    for (int k = 0; k < FE_NK; ++k) s[k] = 0;
    int bad = 0;
    for (int i = lo + l; i < hi; i += G) {
        ACC pred = 0;
        for (int j = 0; j < order; ++j) pred += (ACC)coef[j] * (ACC)S.xs[i - 1 - j];
        const long long r = (long long)S.xs[i] - (long long)(pred >> shift);
        if (r <= -(1ll << 31) || r >= (1ll << 31)) bad = 1;
        const unsigned u = ((unsigned)r << 1) ^ (unsigned)((int)r >> 31);
#pragma unroll
        for (int k = 0; k < FE_NK; ++k) s[k] += u >> k;
    }
    if (lo + l < hi) {
#pragma unroll
        for (int k = 0; k < FE_NK; ++k) FE_ADD64(&S.psum[g * FE_NK + k], s[k]);
    }
    if (bad) FE_OR(badflag, 1);
}

FD void fe_analyze(FeAnalyze& S, const FeArgs& a, const int* __restrict__ fr, int sig, int* status, int* __restrict__ plan) {
    const int n = fr[FF_N];
    const int width0 = a.bps + (sig == 3 ? 1 : 0);
    FE_PAR(FE_T,
        if (t == 0) { S.orall = 0; S.diff = 0; }
        if (t < FE_NCAND) { S.cbad[t] = 0; S.ctake[t] = 0; }
        if (t <= FE_MAXORD) S.ac[t] = 0;
    )
    FE_PAR(FE_T,
        unsigned o = 0;
        for (int i = t; i < n; i += FE_T) {
            const int v = fe_signal(a, fr, sig, i, status);
            S.xs[i] = v;
            o |= (unsigned)v;
        }
        if (o) FE_OR(&S.orall, o);
    )
    const int wasted = S.orall ? fe_ctz(S.orall) : 0;
    const int w = width0 - wasted;
    const int down = w > 16 ? w - 16 : 0;
    int maxo = a.max_lpc < n - 1 ? a.max_lpc : n - 1;
    FE_PAR(FE_T,
        for (int i = t; i < n; i += FE_T) {
            const int v = S.xs[i] >> wasted;
            S.xs[i] = v;
            S.xw[i] = (v >> down) * fe_window(i, n);
        }
    )
    FE_PAR(FE_T,
        int d = 0;
        const int x0 = S.xs[0];
        long long acc[FE_MAXORD + 1];
        _Pragma("unroll")
        for (int l = 0; l <= FE_MAXORD; ++l) acc[l] = 0;
        for (int i = t; i < n; i += FE_T) {
            d |= S.xs[i] != x0;
            if (maxo > 0) {
                const long long v = S.xw[i];
        _Pragma("unroll")
                for (int l = 0; l <= FE_MAXORD; ++l)
                    if (l <= maxo && l <= i) acc[l] += v * (long long)S.xw[i - l];
            }
        }
        if (d) FE_OR(&S.diff, 1);
        if (maxo > 0 && t < n) {
        _Pragma("unroll")
            for (int l = 0; l <= FE_MAXORD; ++l)
                if (l <= maxo) FE_ADD64(&S.ac[l], (unsigned long long)acc[l]);
        }
    )
    const int prec = fe_precision(a.block_size);
    FE_PAR(FE_T,
        if (t == 0) {
            // the first two candidates: constant (when it applies), then verbatim -- constant is never the larger
            S.best[PL_TYPE] = S.diff ? PT_VERBATIM : PT_CONSTANT;
            S.best[PL_BITS] = 8 + wasted + (S.diff ? w * n : w);
            S.best[PL_ORDER] = 0; S.best[PL_PORDER] = 0; S.best[PL_PREC] = 0; S.best[PL_SHIFT] = 0;
            for (int c = 0; c < 5; ++c) {
                S.corder[c] = c; S.cshift[c] = 0; S.cok[c] = c < n;
                for (int j = 0; j < FE_MAXORD; ++j) S.ccoef[c][j] = fe_fixed_coef(c, j);
            }
            fe_levinson(S, maxo, prec);
        }
        if (t < FE_MAXP) S.bparam[t] = 0;
        if (t < FE_MAXORD) S.bcoef[t] = 0;
    )
    int pmax = fe_ctz((unsigned)n);
    if (pmax > a.max_po) pmax = a.max_po;
    const int P = 1 << pmax;
    for (int c = 0; c < 5 + maxo; ++c) {
        if (!S.cok[c]) continue;                                         // uniform: read after a barrier
        const int order = S.corder[c], shift = S.cshift[c];
        FE_PAR(FE_T,
            for (int e = t; e < P * FE_NK; e += FE_T) S.psum[e] = 0;
            if (t <= FE_MAXPO) S.ltot[t] = 0;
        )
        int lg = 0;
        while ((1 << lg) < order) ++lg;
        const bool wide = c >= 5 && w + prec + lg > 32;
        FE_PAR(FE_T,
            if (wide) fe_partition_sums<long long>(S, t, n, pmax, order, shift, S.ccoef[c], &S.cbad[c]);
            else fe_partition_sums<int>(S, t, n, pmax, order, shift, S.ccoef[c], &S.cbad[c]);
        )
        if (S.cbad[c]) continue;
        for (int p = pmax; p >= 0; --p) {
            FE_PAR(FE_T,
                if (t < (1 << p)) {
                    const int stride = 1 << (pmax - p);
                    unsigned long long* e = S.psum + (size_t)t * stride * FE_NK;
                    const unsigned long long cnt = (unsigned long long)((n >> p) - (t == 0 ? order : 0));
                    unsigned long long bestc = 0;
                    int bestk = 0;
        _Pragma("unroll")
                    for (int k = 0; k < FE_NK; ++k) {
                        unsigned long long v = e[k];
                        if (p < pmax) { v += e[(stride >> 1) * FE_NK + k]; e[k] = v; }
                        const unsigned long long cost = v + (unsigned long long)(1 + k) * cnt;
                        if (k == 0 || cost < bestc) { bestc = cost; bestk = k; }
                    }
                    S.lparam[p][t] = (unsigned char)bestk;
                    FE_ADD64(&S.ltot[p], bestc + 4);
                }
            )
        }
        FE_PAR(FE_T,
            if (t == 0) {
                int bp = -1;
                unsigned long long bt = 0;
                for (int p = 0; p <= pmax; ++p)
                    if (p == 0 || (n >> p) > order)
                        if (bp < 0 || S.ltot[p] < bt) { bp = p; bt = S.ltot[p]; }
                const unsigned long long bits = 8ull + wasted + (unsigned long long)order * w + (c >= 5 ? 9ull + (unsigned long long)order * prec : 0ull) + 6ull + bt;
                if (bits < (unsigned long long)S.best[PL_BITS]) {
                    S.best[PL_TYPE] = c >= 5 ? PT_LPC : PT_FIXED;
                    S.best[PL_ORDER] = order; S.best[PL_PORDER] = bp; S.best[PL_PREC] = c >= 5 ? prec : 0; S.best[PL_SHIFT] = shift;
                    S.best[PL_BITS] = (int)bits;
                    S.ctake[c] = 1; S.take_p = bp;
                }
            }
        )
        if (S.ctake[c]) {
            FE_PAR(FE_T,
                if (t < FE_MAXP) S.bparam[t] = t < (1 << S.take_p) ? S.lparam[S.take_p][t] : 0;
                if (t < FE_MAXORD) S.bcoef[t] = t < order ? S.ccoef[c][t] : 0;
            )
        }
    }
    FE_PAR(FE_T,
        if (t == 0) {
            plan[PL_TYPE] = S.best[PL_TYPE]; plan[PL_ORDER] = S.best[PL_ORDER]; plan[PL_WASTED] = wasted; plan[PL_PORDER] = S.best[PL_PORDER];
            plan[PL_PREC] = S.best[PL_PREC]; plan[PL_SHIFT] = S.best[PL_SHIFT]; plan[PL_BITS] = S.best[PL_BITS]; plan[PL_WIDTH] = w;
        }
        if (t < FE_MAXORD) plan[PL_COEF + t] = S.bcoef[t];
        if (t < FE_MAXP / 4) {
            unsigned v = 0;
            for (int k = 0; k < 4; ++k) v |= (unsigned)S.bparam[4 * t + k] << (8 * k);
            plan[PL_PARAM + t] = (int)v;
        }
    )
}

// ---- b. layout ----------------------------------------------------------------------------------------------------------------
FD int fe_utf8_len(unsigned v) { return v < 0x80 ? 1 : v < 0x800 ? 2 : v < 0x10000 ? 3 : v < 0x200000 ? 4 : v < 0x4000000 ? 5 : 6; }
FD int fe_bs_code(int bs) {
    if (bs == 192) return 1;
    for (int k = 0; k < 4; ++k) if (bs == 576 << k) return 2 + k;
    for (int k = 0; k < 8; ++k) if (bs == 256 << k) return 8 + k;
    return bs <= 256 ? 6 : 7;
}
struct FeLayout { long long part[FE_LT]; };

FD void fe_layout_frame(const FeArgs& a, const int* __restrict__ fr, const int* __restrict__ plans, int* frec) {
    int assign = 0, bits;
    if (a.C == 1) bits = plans[PL_BITS];
    else {
        const int l = plans[PL_BITS], r = plans[FE_PLAN + PL_BITS], m = plans[2 * FE_PLAN + PL_BITS], s = plans[3 * FE_PLAN + PL_BITS];
        assign = 1; bits = l + r;
        if (l + s < bits) { assign = 8; bits = l + s; }
        if (s + r < bits) { assign = 9; bits = s + r; }
        if (m + s < bits) { assign = 10; bits = m + s; }
    }
    const int bsc = fe_bs_code(fr[FF_N]);
    const int hlen = 4 + fe_utf8_len((unsigned)fr[FF_NUM]) + (bsc == 6 ? 1 : bsc == 7 ? 2 : 0) + (a.rate_code == 12 ? 1 : a.rate_code >= 13 ? 2 : 0) + 1;
    frec[FR_ASSIGN] = assign;
    frec[FR_HLEN] = hlen;
    frec[FR_BYTES] = hlen + ((bits + 7) >> 3) + 2;
    frec[FR_BITS] = bits;
}

FD void fe_layout(FeLayout& S, const FeArgs& a, const int* __restrict__ ftab, const int* __restrict__ plan, int* frec, long long* foff, int* report) {
    const int nsig = a.C == 1 ? 1 : 4;
    const int per = (a.F + FE_LT - 1) / FE_LT;
    FE_PAR(FE_LT,
        long long sum = 0;
        for (int f = t * per; f < (t + 1) * per && f < a.F; ++f) {
            const int* fr = ftab + (size_t)f * FE_FTAB;
            int* rc = frec + (size_t)f * 4;
            if (fe_frame_ok(a, fr)) fe_layout_frame(a, fr, plan + (size_t)f * nsig * FE_PLAN, rc);
            else { rc[FR_ASSIGN] = 0; rc[FR_HLEN] = 0; rc[FR_BYTES] = 0; rc[FR_BITS] = 0; }
            report[f] = rc[FR_BYTES];
            sum += rc[FR_BYTES];
        }
        S.part[t] = sum;
    )
    FE_PAR(FE_LT,
        if (t == 0) {
            long long at = 0;
            for (int k = 0; k < FE_LT; ++k) { const long long v = S.part[k]; S.part[k] = at; at += v; }
        }
    )
    FE_PAR(FE_LT,
        long long at = S.part[t];
        for (int f = t * per; f < (t + 1) * per && f < a.F; ++f) { foff[f] = at; at += frec[(size_t)f * 4 + FR_BYTES]; }
    )
}

// ---- c. pack ------------------------------------------------------------------------------------------------------------------
// A lane's writer: bits go MSB-first into big-endian bytes = byte-swapped dwords.  The first and the last dword of a lane's range may
// be shared with a neighbour and are OR-ed atomically; the dwords between are the lane's alone and are stored (zero ones not at all:
// the output is zeroed).  Nothing is written at or beyond `end` (a bit position) or beyond `words`.
struct FeW {
    unsigned* out;
    long long words, bit, end;
    unsigned acc;
    int first, over;
};
FD void fe_w_flush(FeW& w, long long word, int shared) {
    if (w.acc && word >= 0 && word < w.words) {
        const unsigned v = __builtin_bswap32(w.acc);
        if (shared || w.first) FE_OR(&w.out[word], v);
        else w.out[word] = v;
    }
    w.first = 0;
    w.acc = 0;
}
FD void fe_w_put(FeW& w, unsigned v, int n) {                            // 0 <= n <= 32
    if (w.over || w.bit + n > w.end) { w.over = 1; return; }
    while (n > 0) {
        const int o = (int)(w.bit & 31);
        const int take = n < 32 - o ? n : 32 - o;
        const unsigned chunk = (v >> (n - take)) & (take == 32 ? 0xFFFFFFFFu : (1u << take) - 1u);
        w.acc |= chunk << (32 - o - take);
        w.bit += take;
        n -= take;
        if ((w.bit & 31) == 0) fe_w_flush(w, (w.bit >> 5) - 1, 0);
    }
}
FD void fe_w_zeros(FeW& w, unsigned q) {
    if (w.over || w.bit + q > w.end) { w.over = 1; return; }
    if ((w.bit & 31) + q >= 32) fe_w_flush(w, w.bit >> 5, 0);
    w.bit += q;
}
FD void fe_w_finish(FeW& w) {
    if (w.bit & 31) fe_w_flush(w, w.bit >> 5, 1);
}

struct FePack {
    int xs[2][FE_MAXBS];
    int cbits[2 * (FE_MAXBS / FE_CHUNK)];
    int pl[2][FE_PLAN];
    int total, over;
};

FD unsigned fe_crc8(unsigned crc, unsigned b) {
    crc ^= b;
    for (int k = 0; k < 8; ++k) crc = (crc & 0x80) ? ((crc << 1) ^ 0x07) & 0xFF : (crc << 1) & 0xFF;
    return crc;
}

// chunk c of channel ch: count its bits, and with WR write them
template <bool WR>
FD int fe_chunk(const FePack& S, int ch, int c, int n, FeW& w) {
    const int* pl = S.pl[ch];
    const int* x = S.xs[ch];
    const int type = pl[PL_TYPE], order = pl[PL_ORDER], width = pl[PL_WIDTH], wasted = pl[PL_WASTED], shift = pl[PL_SHIFT];
    int bits = 0;
    if (c == 0) {
        const unsigned tcode = type == PT_CONSTANT ? 0u : type == PT_VERBATIM ? 1u : type == PT_FIXED ? 8u + order : 32u + order - 1;
        bits += 8 + wasted;
        if (WR) {
            fe_w_put(w, (tcode << 1) | (wasted ? 1u : 0u), 8);
            if (wasted) { fe_w_zeros(w, (unsigned)wasted - 1); fe_w_put(w, 1, 1); }
        }
        if (type == PT_CONSTANT) {
            bits += width;
            if (WR) fe_w_put(w, (unsigned)x[0], width);
        } else if (type != PT_VERBATIM) {
            bits += order * width + 6;
            if (WR)
                for (int i = 0; i < order; ++i) fe_w_put(w, (unsigned)x[i], width);
            if (type == PT_LPC) {
                bits += 9 + order * pl[PL_PREC];
                if (WR) {
                    fe_w_put(w, (unsigned)(pl[PL_PREC] - 1), 4);
                    fe_w_put(w, (unsigned)shift, 5);
                    for (int j = 0; j < order; ++j) fe_w_put(w, (unsigned)pl[PL_COEF + j], pl[PL_PREC]);
                }
            }
            if (WR) fe_w_put(w, (unsigned)pl[PL_PORDER], 6);             // method 0 in the two bits above
        }
    }
    if (type == PT_CONSTANT) return bits;
    int lo = c * FE_CHUNK, hi = lo + FE_CHUNK;
    if (hi > n) hi = n;
    if (type == PT_VERBATIM) {
        bits += (hi - lo) * width;
        if (WR)
            for (int i = lo; i < hi; ++i) fe_w_put(w, (unsigned)x[i], width);
        return bits;
    }
    if (lo < order) lo = order;
    if (lo >= hi) return bits;
    const int plen = n >> pl[PL_PORDER];
    int q = lo / plen;
    int next = q == 0 && lo == order ? lo : (q + 1) * plen;                // the next sample that opens a partition
    if (q > 0 && lo == q * plen) next = lo;
    int k = (pl[PL_PARAM + (q >> 2)] >> (8 * (q & 3))) & 15;
    for (int i = lo; i < hi; ++i) {
        if (i == next) {
            q = i / plen;
            k = (pl[PL_PARAM + (q >> 2)] >> (8 * (q & 3))) & 15;
            bits += 4;
            if (WR) fe_w_put(w, (unsigned)k, 4);
            next = (q + 1) * plen;
        }
        long long pred = 0;
        for (int j = 0; j < order; ++j) pred += (long long)pl[PL_COEF + j] * (long long)x[i - 1 - j];
        const long long r = (long long)x[i] - (pred >> shift);
        const unsigned u = ((unsigned)r << 1) ^ (unsigned)((int)r >> 31);
        const unsigned hiq = u >> k;
        bits += (int)hiq + 1 + k;
        if (WR) { fe_w_zeros(w, hiq); fe_w_put(w, (1u << k) | (u & ((1u << k) - 1u)), k + 1); }
    }
    return bits;
}

FD void fe_hb(FeW& w, unsigned& crc, unsigned b) { fe_w_put(w, b & 0xFF, 8); crc = fe_crc8(crc, b & 0xFF); }

FD void fe_pack(FePack& S, const FeArgs& a, const int* __restrict__ fr, const int* __restrict__ plans, const int* __restrict__ frec,
                long long off, unsigned char* out, long long out_bytes, int* status) {
    const int n = fr[FF_N], assign = frec[FR_ASSIGN];
    const int s0 = assign == 9 ? 3 : assign == 10 ? 2 : 0, s1 = assign == 8 || assign == 10 ? 3 : 1;
    const int nu = (n + FE_CHUNK - 1) / FE_CHUNK;
    FE_PAR(FE_T,
        if (t < FE_PLAN) {
            S.pl[0][t] = plans[s0 * FE_PLAN + t];
            if (a.C == 2) S.pl[1][t] = plans[s1 * FE_PLAN + t];
        }
        if (t == 0) S.over = 0;
    )
    FE_PAR(FE_T,
        for (int ch = 0; ch < a.C; ++ch) {
            const int sg = ch ? s1 : s0, wasted = S.pl[ch][PL_WASTED];
            for (int i = t; i < n; i += FE_T) S.xs[ch][i] = fe_signal(a, fr, sg, i, status) >> wasted;
        }
    )
    FE_PAR(FE_T,
        for (int u = t; u < a.C * nu; u += FE_T) {
            const int ch = u >= nu;
            FeW none;
            none.over = 0;
            S.cbits[u] = fe_chunk<false>(S, ch, u - ch * nu, n, none);
        }
    )
    FE_PAR(FE_T,
        if (t == 0) {
            int at = 0;
            for (int u = 0; u < a.C * nu; ++u) { const int v = S.cbits[u]; S.cbits[u] = at; at += v; }
            S.total = at;
        }
    )
    const bool ok = S.total == frec[FR_BITS] && off >= 0 && off + frec[FR_BYTES] <= out_bytes;
    FE_PAR(FE_T,
        FeW w;
        w.out = (unsigned*)out; w.words = out_bytes >> 2; w.acc = 0; w.over = 0;
        w.end = (off + frec[FR_BYTES] - 2) * 8;
        const long long body = (off + frec[FR_HLEN]) * 8;
        if (ok && t == 0) {
            w.bit = off * 8; w.first = 1;
            const int bsc = fe_bs_code(n);
            const int ssc = a.bps == 8 ? 1 : a.bps == 16 ? 4 : 6;
            unsigned crc = 0;
            fe_hb(w, crc, 0xFF); fe_hb(w, crc, 0xF8);
            fe_hb(w, crc, ((unsigned)bsc << 4) | (unsigned)a.rate_code);
            fe_hb(w, crc, ((unsigned)assign << 4) | ((unsigned)ssc << 1));
            const unsigned num = (unsigned)fr[FF_NUM];
            const int ul = fe_utf8_len(num);
            if (ul == 1) fe_hb(w, crc, num);
            else {
                fe_hb(w, crc, ((0xFFu << (8 - ul)) & 0xFF) | (num >> (6 * (ul - 1))));
                for (int k = ul - 2; k >= 0; --k) fe_hb(w, crc, 0x80 | ((num >> (6 * k)) & 0x3F));
            }
            if (bsc == 6) fe_hb(w, crc, (unsigned)(n - 1));
            else if (bsc == 7) { fe_hb(w, crc, (unsigned)(n - 1) >> 8); fe_hb(w, crc, (unsigned)(n - 1)); }
            if (a.rate_code == 12) fe_hb(w, crc, (unsigned)a.rate_extra);
            else if (a.rate_code >= 13) { fe_hb(w, crc, (unsigned)a.rate_extra >> 8); fe_hb(w, crc, (unsigned)a.rate_extra); }
            fe_hb(w, crc, crc);
            fe_w_finish(w);
            if (w.over) FE_OR(&S.over, 1);
        }
        if (ok)
            for (int u = t; u < a.C * nu; u += FE_T) {
                const int ch = u >= nu;
                w.bit = body + S.cbits[u]; w.first = 1; w.acc = 0;
                fe_chunk<true>(S, ch, u - ch * nu, n, w);
                fe_w_finish(w);
                if (w.over) FE_OR(&S.over, 1);
            }
    )
    FE_PAR(FE_T,
        if (t == 0 && (!ok || S.over)) { FE_MAX(&status[2 * fr[FF_ITEM]], (int)FES_INTERNAL); }
    )
}

// ---- d. CRC-16 ----------------------------------------------------------------------------------------------------------------
// CRC-16 (0x8005, initial value 0, MSB first): crc(A || B) = crc(A) x^(8 |B|) mod P  xor  crc(B)
FD unsigned fe_crc16_byte(const unsigned short* __restrict__ ct, unsigned crc, unsigned b) { return ((crc << 8) & 0xFFFF) ^ ct[((crc >> 8) ^ b) & 0xFF]; }
FD void fe_crc16_table(unsigned short* ct, int t, int nt) {
    for (int x = t; x < 256; x += nt) {
        unsigned c = (unsigned)x << 8;
        for (int k = 0; k < 8; ++k) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xFFFF : (c << 1) & 0xFFFF;
        ct[x] = (unsigned short)c;
    }
}
FD unsigned fe_mulmod(unsigned a, unsigned b) {                          // polynomials of degree < 16 over GF(2), mod x^16 + x^15 + x^2 + 1
    unsigned r = 0;
    for (int i = 15; i >= 0; --i) {
        r = (r & 0x8000) ? ((r << 1) ^ 0x8005) & 0xFFFF : (r << 1) & 0xFFFF;
        if ((b >> i) & 1) r ^= a;
    }
    return r;
}
FD unsigned fe_xpow(unsigned long long e) {                              // x^e mod P; at most 64 squarings
    unsigned r = 1, base = 2;
    for (int k = 0; k < 64 && e; ++k, e >>= 1) {
        if (e & 1) r = fe_mulmod(r, base);
        base = fe_mulmod(base, base);
    }
    return r;
}
struct FeCrc { unsigned short ct[256]; unsigned crc; };
#define FE_CT 64
FD void fe_crc(FeCrc& S, const int* __restrict__ frec, long long off, unsigned char* out, long long out_bytes) {
    const long long len = (long long)frec[FR_BYTES] - 2;
    const bool ok = frec[FR_BYTES] > 2 && off >= 0 && off + frec[FR_BYTES] <= out_bytes;
    FE_PAR(FE_CT,
        fe_crc16_table(S.ct, t, FE_CT);
        if (t == 0) S.crc = 0;
    )
    FE_PAR(FE_CT,
        if (ok) {
            const long long per = (len + FE_CT - 1) / FE_CT;
            long long lo = t * per, hi = lo + per;
            if (hi > len) hi = len;
            if (lo < hi) {
                unsigned c = 0;
                for (long long i = lo; i < hi; ++i) c = fe_crc16_byte(S.ct, c, out[off + i]);
                c = fe_mulmod(c, fe_xpow((unsigned long long)(len - hi) * 8));
                FE_XOR(&S.crc, c);
            }
        }
    )
    FE_PAR(FE_CT,
        if (ok && t == 0) { out[off + len] = (unsigned char)(S.crc >> 8); out[off + len + 1] = (unsigned char)S.crc; }
    )
}

// workspace: plan [F][nsig][FE_PLAN] ints | frec [F][4] ints | foff [F] int64
struct FeWs { long long plan, frec, foff, bytes; };
static inline bool fe_ws_layout(int F, int C, FeWs* w) {
    if (F < 1 || F > (1 << 24) || C < 1 || C > 2) return false;
    const long long nsig = C == 1 ? 1 : 4;
    w->plan = 0;
    w->frec = ((long long)F * nsig * FE_PLAN * 4 + 255) / 256 * 256;
    w->foff = w->frec + ((long long)F * 16 + 255) / 256 * 256;
    w->bytes = w->foff + (long long)F * 8;
    return true;
}
static inline bool fe_args_ok(const FeArgs& a) {
    return a.B >= 1 && a.B <= a.F && a.R >= 1 && a.N >= 1 && a.N < (1ll << 31) && (a.bps == 8 || a.bps == 16 || a.bps == 24) &&
           a.block_size >= 16 && a.block_size <= FE_MAXBS && a.max_lpc >= 0 && a.max_lpc <= FE_MAXORD && a.max_po >= 0 &&
           a.max_po <= FE_MAXPO && a.rate_code >= 0 && a.rate_code <= 14 && a.rate_code != 12 && a.rate_extra >= 0 && a.rate_extra < 65536 &&
           (a.xf != 0) != (a.xi != 0);
}

#ifndef FLAC_ENC_HOST_EMU
__global__ __launch_bounds__(FE_T) void flac_enc_analyze_kernel(FeArgs a, const int* __restrict__ ftab, int* __restrict__ plan, int* status) {
    __shared__ FeAnalyze S;
    const int f = blockIdx.x, sig = blockIdx.y, nsig = gridDim.y;
    const int* fr = ftab + (size_t)f * FE_FTAB;
    if (!fe_frame_ok(a, fr)) return;                                    // uniform; the layout kernel reports it
    fe_analyze(S, a, fr, sig, status, plan + ((size_t)f * nsig + sig) * FE_PLAN);
}

__global__ __launch_bounds__(FE_LT) void flac_enc_layout_kernel(FeArgs a, const int* __restrict__ ftab, const int* __restrict__ plan, int* frec,
                                                                long long* foff, int* report) {
    __shared__ FeLayout S;
    fe_layout(S, a, ftab, plan, frec, foff, report);
}

__global__ __launch_bounds__(FE_T) void flac_enc_pack_kernel(FeArgs a, const int* __restrict__ ftab, const int* __restrict__ plan,
                                                             const int* __restrict__ frec, const long long* __restrict__ foff,
                                                             unsigned char* out, long long out_bytes, int* status) {
    __shared__ FePack S;
    const int f = blockIdx.x, nsig = a.C == 1 ? 1 : 4;
    const int* fr = ftab + (size_t)f * FE_FTAB;
    if (!fe_frame_ok(a, fr)) {
        if (threadIdx.x == 0 && fr[FF_ITEM] >= 0 && fr[FF_ITEM] < a.B) atomicMax(&status[2 * fr[FF_ITEM]], (int)FES_TABLE);
        return;
    }
    fe_pack(S, a, fr, plan + (size_t)f * nsig * FE_PLAN, frec + (size_t)f * 4, foff[f], out, out_bytes, status);
}

__global__ __launch_bounds__(FE_CT) void flac_enc_crc_kernel(const int* __restrict__ frec, const long long* __restrict__ foff, unsigned char* out,
                                                             long long out_bytes) {
    __shared__ FeCrc S;
    const int f = blockIdx.x;
    fe_crc(S, frec + (size_t)f * 4, foff[f], out, out_bytes);
}

extern "C" long long v100_flac_encode_workspace_bytes(int F, int C) {
    FeWs w;
    return fe_ws_layout(F, C, &w) ? w.bytes : -1;
}

extern "C" int v100_flac_encode(const float* wave, const int* pcm, const int* ftab, void* ws, unsigned char* out, int* report, int* status,
                                int B, int F, int R, int C, long long N, int bits_per_sample, int block_size, int max_lpc_order,
                                int max_partition_order, int rate_code, int rate_extra, long long out_bytes, void* stream) {
    if ((!wave && !pcm) || !ftab || !ws || !out || !report || !status) return V100_ERR_NULL;
    FeArgs a;
    a.xf = wave; a.xi = wave ? (const int*)0 : pcm; a.N = N; a.R = R; a.C = C; a.bps = bits_per_sample; a.block_size = block_size;
    a.max_lpc = max_lpc_order; a.max_po = max_partition_order; a.B = B; a.F = F; a.rate_code = rate_code; a.rate_extra = rate_extra;
    FeWs w;
    if (!fe_ws_layout(F, C, &w) || !fe_args_ok(a) || out_bytes < 16 || (out_bytes & 3) || out_bytes >= (1ll << 40)) return V100_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* base = (unsigned char*)ws;
    int* plan = (int*)(base + w.plan);
    int* frec = (int*)(base + w.frec);
    long long* foff = (long long*)(base + w.foff);
    if (hipMemsetAsync(out, 0, (size_t)out_bytes, st) != hipSuccess) return V100_ERR_LAUNCH;
    if (hipMemsetAsync(status, 0, (size_t)B * 2 * sizeof(int), st) != hipSuccess) return V100_ERR_LAUNCH;
    if (hipMemsetAsync(base, 0, (size_t)w.frec, st) != hipSuccess) return V100_ERR_LAUNCH;
    V100_GGL(flac_enc_analyze_kernel, dim3(F, C == 1 ? 1 : 4), dim3(FE_T), 0, st, a, ftab, plan, status);
    V100_GGL(flac_enc_layout_kernel, dim3(1), dim3(FE_LT), 0, st, a, ftab, plan, frec, foff, report);
    V100_GGL(flac_enc_pack_kernel, dim3(F), dim3(FE_T), 0, st, a, ftab, plan, frec, foff, out, out_bytes, status);
    V100_GGL(flac_enc_crc_kernel, dim3(F), dim3(FE_CT), 0, st, frec, foff, out, out_bytes);
    return v100_launch_status();
}
#endif
