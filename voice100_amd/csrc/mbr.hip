// K35: minimum-Bayes-risk selection over the n best transcripts of each utterance, and the list's distances to a reference: three
// launches on the caller's stream, no read-back.
//
//   a. mbr_tokenise_kernel, one workgroup of 16 waves per utterance: the N hypotheses (and the reference row, where there is one) are
//      segmented once each (word level: K23's ballot segmentation, a wave per row) and every token -- an id, or a word -- gets a
//      canonical int32 through ONE open-addressing table per utterance, so that equal tokens of different rows get equal numbers.  The
//      table lives in the workspace in global memory (up to 65 x 4096 tokens do not fit LDS), is initialised by the kernel itself, is
//      probed for at most one lap, and a slot's owner is taken as a token's class only after its length and every id have been
//      compared: the hash only finds candidates.  Which token of a class claimed the slot does not matter to any distance.
//   b. mbr_pairs_kernel, one wave per (utterance, pair): the N (N - 1) / 2 unordered pairs and, with a reference, the N pairs (i, ref).
//      The common prefix p and then the common suffix s (clamped to min(n, m) - p, so the two never overlap: aaa / aa) of the two
//      canonical rows are stripped 64 tokens a ballot -- the Levenshtein distance is unchanged by both -- and K23's systolic recurrence
//      runs on the middles, the shorter one as the columns, so that the strip width S is the smallest that fits.  A pair with an absent
//      member writes -1 and leaves, wave-uniformly.
//   c. mbr_finalise_kernel, one workgroup per utterance: posterior p = exp(scale (s - s_max)) / sum over the present hypotheses, in
//      fp64 from the fp32 scores, summed in index order; risk_i = sum_j p_j dist[i][j] in fp64 in the order j = 0 .. N - 1 (no fused
//      multiply-add, so that a host restatement gives the same bits), stored as fp32; THE STORED fp32 RISK IS THE RANKING KEY, smaller
//      first, equal keys in the given order, absent hypotheses (score -inf or NaN) behind in the given order; ranks by counting, as in
//      rescore.hip; the small outputs are written by rank and the id rows move whole.
//
// ed_from_left / ed_segment / ed_systolic are K23's, shared through edit_distance_common.h (edit_distance_kernel's disassembly is
// unchanged by the move: profiles/mbr_isa_identity.txt).  Nothing beyond a row's length is read, lengths and the counts read back from the
// workspace are clamped, ids and canonical tokens are hashed and compared and never used as an index, and every loop is bounded by a
// shape argument.
//
// MBR_HOST_EMU compiles the hash, the posterior's exponent, the ranking rule and the workspace layout as plain C++ for
// tools/mbr_host.cpp (which restates the waves' part); the library build never defines it.
#ifdef MBR_HOST_EMU
#include <math.h>
#include <stdint.h>
#include <string.h>
#define MB_HD static inline
typedef unsigned short u16;
#else
#include "edit_distance_common.h"
#define MB_HD __host__ __device__ __forceinline__
#endif

#define MB_TMAX 4096
#define MB_NBEST_MAX 64
#define MB_ROWS_MAX (MB_NBEST_MAX + 1)                   // the hypotheses and the reference
#define MB_EMPTY 0xffffffffu

typedef unsigned long long mb_u64;

// the hash of the token x[0 .. len): K23's, over all 64 bits of every id
MB_HD mb_u64 mb_hash(const long long* x, int len) {
    mb_u64 h = (mb_u64)len * 0xD6E8FEB86659FD93ull;
    for (int i = 0; i < len; ++i) {
        h = (h ^ (mb_u64)x[i]) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
    }
    return h;
}
MB_HD unsigned mb_fold(mb_u64 h) { return (unsigned)(h ^ (h >> 32)); }

MB_HD int mb_present(float s) { return s > -INFINITY ? 1 : 0; }             // -inf: no hypothesis; NaN: none either

// the posterior's exponent for a present hypothesis of score f, s_max the greatest present score: never NaN (inf - inf, 0 * inf)
MB_HD double mb_arg(double scale, float f, float s_max) {
    if (f == s_max || scale == 0.0) return 0.0;
    return scale * ((double)f - (double)s_max);
}

// is hypothesis i ahead of hypothesis j (i != j)?  the key is the stored fp32 risk; an absent hypothesis is behind every present one
MB_HD bool mb_ahead(float risk_i, int present_i, int i, float risk_j, int present_j, int j) {
    if (present_i != present_j) return present_i > present_j;
    if (present_i && risk_i != risk_j) return risk_i < risk_j;
    return i < j;
}

// Tr = 0: no reference
MB_HD bool mb_shape_ok(int B, int nbest, int T, int Tr) {
    return B >= 1 && nbest >= 1 && nbest <= MB_NBEST_MAX && T >= 1 && T <= MB_TMAX && Tr >= 0 && Tr <= MB_TMAX;
}
MB_HD int mb_rows(int nbest, int Tr) { return nbest + (Tr > 0 ? 1 : 0); }
MB_HD int mb_width(int T, int Tr) { return T > Tr ? T : Tr; }
MB_HD int mb_slots(int rows, int width) {               // load <= 1/2 at the id level, <= 1/4 at the word level
    int P = 128;
    while (P < 2 * rows * width) P <<= 1;                // <= 2^20
    return P;
}
// one utterance's part of the workspace: [R W] int32 canonical tokens, [P] table, [MB_ROWS_MAX + 3] token counts, [R W] [R W] u16 bounds
MB_HD size_t mb_ws_per(int rows, int width) {
    const size_t rw = (size_t)rows * width;
    return (4 * rw + 4 * (size_t)mb_slots(rows, width) + 4 * (MB_ROWS_MAX + 3) + 4 * rw + 15) & ~(size_t)15;
}

#ifndef MBR_HOST_EMU
struct MbWs {
    int* tok;
    unsigned* tab;
    int* cnt;
    u16 *st, *en;
};
__device__ __forceinline__ MbWs mb_ws(unsigned char* ws, int b, int R, int W, int P) {
    unsigned char* base = ws + (size_t)b * mb_ws_per(R, W);
    MbWs w;
    w.tok = (int*)base;
    w.tab = (unsigned*)(w.tok + (size_t)R * W);
    w.cnt = (int*)(w.tab + P);
    w.st = (u16*)(w.cnt + MB_ROWS_MAX + 3);
    w.en = w.st + (size_t)R * W;
    return w;
}

#define MB_TOK_WAVES 16

__global__ __launch_bounds__(64 * MB_TOK_WAVES) void mbr_tokenise_kernel(
        const long long* __restrict__ ids, const int* __restrict__ lens, const float* __restrict__ scores, const long long* __restrict__ ref,
        const int* __restrict__ ref_len, unsigned char* ws, int N, int T, int Tr, int words, long long sep, int P) {
    __shared__ int s_len[MB_ROWS_MAX], s_off[MB_ROWS_MAX + 1];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = mb_rows(N, Tr), W = mb_width(T, Tr);
    const MbWs w = mb_ws(ws, b, R, W, P);
    auto row_ptr = [&](int r) { return r < N ? ids + ((size_t)b * N + r) * T : ref + (size_t)b * Tr; };

    for (int i = tid; i < P; i += 64 * MB_TOK_WAVES) w.tab[i] = MB_EMPTY;
    for (int r = wave; r < R; r += MB_TOK_WAVES) {       // r, and all that is read under it by every lane alike, is wave-uniform
        int n = 0;
        if (r == N) n = min(max(ref_len[b], 0), Tr);
        else if (mb_present(scores[(size_t)b * N + r])) n = min(max(lens[(size_t)b * N + r], 0), T);
        n = __builtin_amdgcn_readfirstlane(n);
        int cnt = n;
        if (words) cnt = __builtin_amdgcn_readfirstlane(ed_segment(row_ptr(r), n, sep, w.st + (size_t)r * W, w.en + (size_t)r * W, lane));
        if (lane == 0) {
            s_len[r] = n;
            s_off[r + 1] = cnt;
            w.cnt[r] = cnt;
        }
    }
    __threadfence();                                     // the table's initial state is in L2, where the atomics below meet it
    __syncthreads();                                     // the table, the word bounds and the counts are visible to the workgroup
    if (tid == 0) {
        s_off[0] = 0;
        for (int r = 0; r < R; ++r) s_off[r + 1] += s_off[r];
    }
    __syncthreads();

    auto token = [&](int r, int k, const long long*& p, int& len) {      // r < R, k < the row's count (so its length is >= 1)
        const int n = s_len[r];
        int s0 = k;
        len = 1;
        if (words) {
            s0 = min((int)w.st[(size_t)r * W + k], n - 1);
            len = min(max((int)w.en[(size_t)r * W + k] - s0 + 1, 1), n - s0);
        }
        p = row_ptr(r) + s0;
    };
    const int total = s_off[R];
    const unsigned mask = (unsigned)P - 1u;
    for (int g = tid; g < total; g += 64 * MB_TOK_WAVES) {
        int lo = 0, hi = R - 1;                          // the row of token g: the last r with s_off[r] <= g
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_off[mid] <= g) lo = mid;
            else hi = mid - 1;
        }
        const int r = lo, k = g - s_off[r];
        const long long* p;
        int len;
        token(r, k, p, len);
        const unsigned self = (unsigned)(r * W + k);
        unsigned slot = mb_fold(mb_hash(p, len)) & mask;
        int id = (int)self;                              // (a whole lap without a home cannot happen at load <= 1/2; then the token stands alone)
        for (int probe = 0; probe < P; ++probe) {
            const unsigned cur = atomicCAS(&w.tab[slot], MB_EMPTY, self);
            if (cur == MB_EMPTY) break;                  // first of its class
            const int r2 = (int)(cur / (unsigned)W), k2 = (int)(cur % (unsigned)W);
            if (r2 < R && k2 < s_off[r2 + 1] - s_off[r2]) {
                const long long* q;
                int qlen;
                token(r2, k2, q, qlen);
                bool same = qlen == len;
                for (int i = 0; same && i < len; ++i) same = q[i] == p[i];
                if (same) { id = (int)cur; break; }
            }
            slot = (slot + 1) & mask;
        }
        w.tok[(size_t)r * W + k] = id;
    }
}

__global__ __launch_bounds__(64) void mbr_pairs_kernel(const float* __restrict__ scores, unsigned char* ws, int* __restrict__ dist,
                                                       int* __restrict__ ref_dist, int N, int T, int Tr, int P) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int R = mb_rows(N, Tr), W = mb_width(T, Tr);
    const MbWs w = mb_ws(ws, b, R, W, P);
    int q = blockIdx.y, i, j;
    const int NP = N * (N - 1) / 2;
    if (q < NP) {                                        // the q-th pair i < j in the order (0, 1), (0, 2), ... (N - 2, N - 1)
        i = 0;
        while (q >= N - 1 - i) {
            q -= N - 1 - i;
            ++i;
        }
        j = i + 1 + q;
    } else {
        i = q - NP;
        j = N;                                           // the reference
    }
    int* d_ij = j < N ? dist + ((size_t)b * N + i) * N + j : ref_dist + (size_t)b * N + i;
    int* d_ji = j < N ? dist + ((size_t)b * N + j) * N + i : d_ij;
    int both = mb_present(scores[(size_t)b * N + i]);
    if (j < N) both &= mb_present(scores[(size_t)b * N + j]);
    if (!__builtin_amdgcn_readfirstlane(both)) {
        if (lane == 0) *d_ij = *d_ji = -1;
        return;
    }
    const int n = __builtin_amdgcn_readfirstlane(min(max(w.cnt[i], 0), W));
    const int m = __builtin_amdgcn_readfirstlane(min(max(w.cnt[j], 0), W));
    const int* a = w.tok + (size_t)i * W;
    const int* c = w.tok + (size_t)j * W;
    const int mn = min(n, m);
    int p = mn;                                          // the common prefix
    for (int p0 = 0; p0 < mn; p0 += 64) {
        const int k = p0 + lane;
        const unsigned long long ne = __ballot(k < mn && a[k] != c[k]);
        if (ne) {
            p = p0 + __ffsll(ne) - 1;
            break;
        }
    }
    const int lim = mn - p;                              // the suffix may not reach into the prefix
    int s = lim;
    for (int s0 = 0; s0 < lim; s0 += 64) {
        const int k = s0 + lane;
        const unsigned long long ne = __ballot(k < lim && a[n - 1 - k] != c[m - 1 - k]);
        if (ne) {
            s = s0 + __ffsll(ne) - 1;
            break;
        }
    }
    p = __builtin_amdgcn_readfirstlane(p);
    s = __builtin_amdgcn_readfirstlane(s);
    const int na = n - p - s, nc = m - p - s;            // the middles
    const bool swap = na < nc;                           // the shorter middle is the columns
    const int* cols = (swap ? a : c) + p;
    const int* rows = (swap ? c : a) + p;
    const int mc = swap ? na : nc, nr = swap ? nc : na;
    int dd;
    if (mc == 0) dd = nr;
    else if (mc <= 64) dd = ed_systolic<1>(cols, rows, mc, nr, lane);
    else if (mc <= 128) dd = ed_systolic<2>(cols, rows, mc, nr, lane);
    else if (mc <= 256) dd = ed_systolic<4>(cols, rows, mc, nr, lane);
    else if (mc <= 512) dd = ed_systolic<8>(cols, rows, mc, nr, lane);
    else if (mc <= 1024) dd = ed_systolic<16>(cols, rows, mc, nr, lane);
    else if (mc <= 2048) dd = ed_systolic<32>(cols, rows, mc, nr, lane);
    else dd = ed_systolic<64>(cols, rows, mc, nr, lane);
    if (lane == 0) *d_ij = *d_ji = dd;
}

#define MB_FIN_THREADS 256

__global__ __launch_bounds__(MB_FIN_THREADS) void mbr_finalise_kernel(
        const long long* __restrict__ ids, const int* __restrict__ lens, const float* __restrict__ scores, unsigned char* ws,
        int* __restrict__ dist, long long* __restrict__ out_ids, int* __restrict__ out_lens, float* __restrict__ out_scores,
        float* __restrict__ out_risk, float* __restrict__ out_post, int* __restrict__ out_ntok, int* __restrict__ out_order,
        int* __restrict__ ref_n, float* __restrict__ expected_len, int N, int T, int Tr, int P, double scale) {
    __shared__ double s_e[MB_NBEST_MAX], s_p[MB_NBEST_MAX];
    __shared__ float s_f[MB_NBEST_MAX], s_risk[MB_NBEST_MAX];
    __shared__ int s_present[MB_NBEST_MAX], s_nt[MB_NBEST_MAX], s_rank[MB_NBEST_MAX];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = mb_rows(N, Tr), W = mb_width(T, Tr);
    const MbWs w = mb_ws(ws, b, R, W, P);
    const size_t row0 = (size_t)b * N;
    if (tid < N) {
        const float f = scores[row0 + tid];
        s_f[tid] = f;
        s_present[tid] = mb_present(f);
        s_nt[tid] = mb_present(f) ? min(max(w.cnt[tid], 0), W) : 0;
    }
    __syncthreads();
    if (tid < N) {
        float s_max = -INFINITY;
        for (int j = 0; j < N; ++j)
            if (s_present[j]) s_max = fmaxf(s_max, s_f[j]);
        s_e[tid] = s_present[tid] ? exp(mb_arg(scale, s_f[tid], s_max)) : 0.0;
    }
    __syncthreads();
    if (tid < N) {
        double z = 0.0;
        for (int j = 0; j < N; ++j) z += s_e[j];         // index order, the same sum in every thread
        s_p[tid] = z > 0.0 ? s_e[tid] / z : 0.0;
    }
    __syncthreads();
    if (tid < N) {
        const int i = tid;
        double risk = 0.0;
        for (int j = 0; j < N; ++j)
            if (j != i && s_present[j]) risk = __dadd_rn(risk, __dmul_rn(s_p[j], (double)dist[(row0 + i) * N + j]));
        s_risk[i] = s_present[i] ? (float)risk : INFINITY;
        dist[(row0 + i) * N + i] = s_present[i] ? 0 : -1;
        if (i == 0) {
            double el = 0.0;
            for (int j = 0; j < N; ++j) el = __dadd_rn(el, __dmul_rn(s_p[j], (double)s_nt[j]));
            expected_len[b] = (float)el;
            if (Tr > 0) ref_n[b] = min(max(w.cnt[N], 0), W);
        }
    }
    __syncthreads();
    if (tid < N) {
        const int j = tid;
        int rank = 0;
        for (int i = 0; i < N; ++i)
            if (i != j && mb_ahead(s_risk[i], s_present[i], i, s_risk[j], s_present[j], j)) ++rank;
        s_rank[j] = rank;                                // a strict total order: the ranks are a permutation of 0 .. N - 1
        const size_t o = row0 + rank;
        out_order[o] = j;
        out_lens[o] = lens[row0 + j];
        out_scores[o] = s_f[j];
        out_risk[o] = s_risk[j];
        out_post[o] = (float)s_p[j];
        out_ntok[o] = s_nt[j];
    }
    __syncthreads();
    for (int j = wave; j < N; j += MB_FIN_THREADS / 64) {  // the id rows move whole, padding included
        const long long* src = ids + (row0 + j) * (size_t)T;
        long long* dst = out_ids + (row0 + s_rank[j]) * (size_t)T;
        for (int p = lane; p < T; p += 64) dst[p] = src[p];
    }
}

extern "C" long long v100_nbest_mbr_workspace_bytes(int B, int nbest, int T, int Tr) {
    if (!mb_shape_ok(B, nbest, T, Tr)) return -1;
    return (long long)B * (long long)mb_ws_per(mb_rows(nbest, Tr), mb_width(T, Tr));
}

extern "C" int v100_nbest_mbr(const long long* ids, const int* lens, const float* scores, const long long* ref, const int* ref_len, void* ws,
                              long long* out_ids, int* out_lens, float* out_scores, float* out_risk, float* out_post, int* out_ntok,
                              int* out_order, int* dist, int* ref_dist, int* ref_n, float* expected_len, int B, int nbest, int T, int Tr,
                              int words, long long sep, double scale, void* stream) {
    if (!ids || !lens || !scores || !ws || !out_ids || !out_lens || !out_scores || !out_risk || !out_post || !out_ntok || !out_order ||
        !dist || !expected_len)
        return V100_ERR_NULL;
    const bool has_ref = ref || ref_len;
    if (has_ref && (!ref || !ref_len || !ref_dist || !ref_n)) return V100_ERR_NULL;
    if (!mb_shape_ok(B, nbest, T, Tr) || (has_ref ? Tr < 1 : Tr != 0) || !(scale - scale == 0.0) || scale < 0.0)
        return V100_ERR_SHAPE;
    const int R = mb_rows(nbest, Tr), P = mb_slots(R, mb_width(T, Tr));
    hipStream_t st = (hipStream_t)stream;
    V100_GGL(mbr_tokenise_kernel, dim3(B), dim3(64 * MB_TOK_WAVES), 0, st, ids, lens, scores, ref, ref_len, (unsigned char*)ws, nbest, T, Tr,
             words != 0, sep, P);
    const int pairs = nbest * (nbest - 1) / 2 + (has_ref ? nbest : 0);
    if (pairs > 0)
        V100_GGL(mbr_pairs_kernel, dim3(B, pairs), dim3(64), 0, st, scores, (unsigned char*)ws, dist, ref_dist, nbest, T, Tr, P);
    V100_GGL(mbr_finalise_kernel, dim3(B), dim3(MB_FIN_THREADS), 0, st, ids, lens, scores, (unsigned char*)ws, dist, out_ids, out_lens,
             out_scores, out_risk, out_post, out_ntok, out_order, ref_n, expected_len, nbest, T, Tr, P, scale);
    return v100_launch_status();
}
#endif
