// K34: re-rank the n best transcripts of each utterance with a word-level back-off n-gram model (lm.WordNGramLM), one launch, no read-back.
//
// One workgroup per utterance, min(nbest, 16) waves; wave w takes hypotheses w, w + waves, ...  Per hypothesis, one wave:
//   1. segmentation: a word is a maximal run of ids != sep inside the hypothesis' length.  64 positions at a time, a ballot of the run
//      starts and one of the run ends; the k-th start and the k-th end are word k (prefix popcounts, no atomics) -- K23's ed_segment,
//      restated here so that edit_distance.hip's code object stays what it is;
//   2. word ids: lane k hashes word k over all 64 bits of its ids, probes the model's open-addressing word table and takes a slot's word
//      id only after the length and every id have been compared with the spelling in the id pool -- the hash only finds candidates.
//      An empty slot, or a whole lap of the table, makes the word <unk>;
//   3. scoring: with every word id known the sentence is parallel over positions.  Lane k walks the back-off for word k on its own
//      context (the at most order - 1 words before it, <s> in front where the model lists it):
//          the longest context first: the (m + 1)-gram listed -> its log p ends the walk; else add the m-gram's back-off weight where
//          the context is listed, drop the oldest word and go on; an unlisted unigram is -inf (compile() lists <unk>, so no word is);
//      every n-gram is found in the open-addressing table of its order, keyed on the n word ids and verified on them;
//   4. the </s> term, where use_eos is set and the model lists </s>;
//   5. the terms are added in fp64 in one fixed order: each lane its words k = lane, lane + 64, ... in turn, the 64 partial sums in a
//      butterfly, then </s>.  Two calls give equal bits.
// After the workgroup's barrier: key = first + lm_weight * lm + word_bonus * n_words in fp64 from the fp32 first-pass score; the rank of
// a hypothesis is the number of hypotheses ahead of it (a greater key, or an equal key and a lower first-pass index; one whose
// first-pass score is -inf or NaN is absent and stays behind every present one, in its first-pass order); the small outputs are written
// by rank and the id rows are copied whole to their new places.
//
// Word bounds and word ids of the hypothesis in flight: 8 bytes a word, 2048 words at 4096 labels = 16 KiB a wave, 256 KiB for 16 waves:
// more than the CU's 160 KiB of LDS, so they live in a global scratch that the same wave writes and reads (as K23's do), between
// workgroup-scope fences.  LDS holds the 64 keys and counts only.
//
// Nothing the tables or the ids hold can move an access outside a buffer or keep a loop running: every probe loop runs at most its
// table's capacity, a slot's pool offset is used only where offset + length lies inside the pool, word ids coming out of a table are
// only ever hashed and compared (never an index), and the per-order offsets and capacities are checked on the host against the table's
// size before the launch.  Workgroups do not communicate.
//
// RESCORE_HOST_EMU compiles the table lookups, the back-off walk and the ranking rule as plain C++ for tools/rescore_host.cpp (which
// restates the wave's part: the ballots and the order of the sum); the library build never defines it.
#ifdef RESCORE_HOST_EMU
#include <math.h>
#include <stdint.h>
#include <string.h>
#define RS_DEV static inline
#else
#include "common.h"
#define RS_DEV __device__ __forceinline__
#endif

#define RS_TMAX 4096
#define RS_NBEST_MAX 64
#define RS_WAVES_MAX 16
#define RS_MAX_ORDER 8
#define RS_UNK 0                                         // word ids: <unk>, <s>, </s>, then the vocabulary in the pool's order
#define RS_BOS 1
#define RS_EOS 2

typedef unsigned long long rs_u64;

// what the kernel knows about the tables, checked by the launcher: ng_off / ng_cap of order n at index n - 1
struct RsModel {
    int order, has_bos, has_eos;
    int pool_len;                                        // int64 elements of the id pool
    int wcap;                                            // slots of the word table, a power of two; a slot is {word id or -1, pool offset, length, 0}
    int ng_off[RS_MAX_ORDER];                            // first int32 of the order's table inside ng
    int ng_cap[RS_MAX_ORDER];                            // its slots, a power of two; a slot is n word ids (the first -1: empty), log p, back-off
};

RS_DEV rs_u64 rs_mix(rs_u64 h, rs_u64 v) {
    h = (h ^ v) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}
RS_DEV unsigned rs_fold(rs_u64 h) { return (unsigned)(h ^ (h >> 32)); }
RS_DEV float rs_as_float(int v) {
    float f;
    memcpy(&f, &v, 4);
    return f;
}

// the id of the word x[0 .. len): a vocabulary word's, or RS_UNK
RS_DEV int rs_word_id(const RsModel& M, const long long* pool, const int* wtab, const long long* x, int len) {
    rs_u64 h = (rs_u64)len * 0xD6E8FEB86659FD93ull;
    for (int i = 0; i < len; ++i) h = rs_mix(h, (rs_u64)x[i]);
    const unsigned mask = (unsigned)M.wcap - 1u;
    unsigned slot = rs_fold(h) & mask;
    for (int probe = 0; probe < M.wcap; ++probe) {       // at most one lap, whatever the table holds
        const int* e = wtab + 4 * (size_t)slot;
        const int wid = e[0], off = e[1], wl = e[2];
        if (wid < 0) return RS_UNK;                      // an empty slot ends the chain
        if (wl == len && off >= 0 && off <= M.pool_len - len) {             // a spelling that leaves the pool is no candidate
            bool same = true;
            for (int i = 0; same && i < len; ++i) same = pool[off + i] == x[i];
            if (same) return wid;
        }
        slot = (slot + 1) & mask;
    }
    return RS_UNK;
}

// token i of the n-gram made of the m words before position k and then `tok`; position -1 is <s>
RS_DEV int rs_key(const int* wid, int k, int m, int tok, int i) {
    if (i >= m) return tok;
    const int p = k - m + i;
    return p < 0 ? RS_BOS : wid[p];
}

// the n-gram of rs_key(.., i), i < n (n = m: the context alone, n = m + 1: with tok); its slot's two floats
RS_DEV bool rs_ngram(const RsModel& M, const int* ng, const int* wid, int k, int m, int tok, int n, float* lp, float* bow) {
    rs_u64 h = (rs_u64)n * 0xD6E8FEB86659FD93ull;
    for (int i = 0; i < n; ++i) h = rs_mix(h, (rs_u64)(unsigned)rs_key(wid, k, m, tok, i));
    const int cap = M.ng_cap[n - 1], stride = n + 2;
    const int* base = ng + M.ng_off[n - 1];
    const unsigned mask = (unsigned)cap - 1u;
    unsigned slot = rs_fold(h) & mask;
    for (int probe = 0; probe < cap; ++probe) {
        const int* e = base + (size_t)slot * stride;
        if (e[0] < 0) return false;
        bool same = true;
        for (int i = 0; same && i < n; ++i) same = e[i] == rs_key(wid, k, m, tok, i);
        if (same) {
            *lp = rs_as_float(e[n]);
            *bow = rs_as_float(e[n + 1]);
            return true;
        }
        slot = (slot + 1) & mask;
    }
    return false;
}

// log p(tok | the words before position k), the back-off walk in fp64 over the float32 table values
RS_DEV double rs_term(const RsModel& M, const int* ng, const int* wid, int k, int tok) {
    const int avail = k + (M.has_bos ? 1 : 0);
    double acc = 0.0;
    float lp, bow;
    for (int m = avail < M.order - 1 ? avail : M.order - 1; m >= 0; --m) {
        if (rs_ngram(M, ng, wid, k, m, tok, m + 1, &lp, &bow)) return acc + (double)lp;
        if (m > 0 && rs_ngram(M, ng, wid, k, m, tok, m, &lp, &bow)) acc += (double)bow;
    }
    return -INFINITY;
}

// is hypothesis i ahead of hypothesis j (i != j)?  keys are never NaN; an absent hypothesis is behind every present one
RS_DEV bool rs_ahead(double key_i, int present_i, int i, double key_j, int present_j, int j) {
    if (present_i != present_j) return present_i > present_j;
    if (present_i && key_i != key_j) return key_i > key_j;
    return i < j;
}

RS_DEV double rs_sort_key(float first, double alpha, double lm, double beta, int n_words) {
    const double key = (double)first + alpha * lm + beta * (double)n_words;
    return key != key ? -INFINITY : key;                 // (a weight of 0 on an infinite term)
}

static inline bool rs_shape_ok(int B, int nbest, int T) { return B >= 1 && nbest >= 1 && nbest <= RS_NBEST_MAX && T >= 1 && T <= RS_TMAX; }
static inline int rs_waves(int nbest) { return nbest < RS_WAVES_MAX ? nbest : RS_WAVES_MAX; }
static inline int rs_words_max(int T) { return (T + 1) / 2; }

// order, the word table and the per-order tables against the sizes of the buffers that hold them
static inline bool rs_model_ok(const RsModel& M, long long wtab_len, long long ng_len) {
    if (M.order < 1 || M.order > RS_MAX_ORDER || M.pool_len < 0) return false;
    if (M.wcap < 1 || (M.wcap & (M.wcap - 1)) || 4ll * M.wcap > wtab_len || wtab_len > 0x7fffffffll || ng_len > 0x7fffffffll) return false;
    for (int n = 1; n <= M.order; ++n) {
        const long long off = M.ng_off[n - 1], cap = M.ng_cap[n - 1];
        if (off < 0 || cap < 1 || (cap & (cap - 1)) || off + cap * (n + 2) > ng_len) return false;
    }
    return true;
}

#ifndef RESCORE_HOST_EMU
// word bounds of one row: st[k] / en[k] = first / last position of word k; returns the number of words (<= (n + 1) / 2)
__device__ __forceinline__ int rs_segment(const long long* __restrict__ x, int n, long long sep, u16* st, u16* en, int lane) {
    int ns = 0, ne = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int p0 = 0; p0 < n; p0 += 64) {                 // n is wave-uniform: every lane takes part in the ballots
        const int p = p0 + lane;
        const bool in = p < n;
        const long long c = in ? x[p] : sep;
        const long long pv = (in && p > 0) ? x[p - 1] : sep;
        const long long nx = (p + 1 < n) ? x[p + 1] : sep;
        const bool tk = in && c != sep;
        const bool s = tk && pv == sep, e = tk && nx == sep;
        const unsigned long long ms = __ballot(s), me = __ballot(e);
        if (s) st[ns + __popcll(ms & below)] = (u16)p;
        if (e) en[ne + __popcll(me & below)] = (u16)p;
        ns += __popcll(ms);
        ne += __popcll(me);
    }
    return ns;
}

__global__ __launch_bounds__(64 * RS_WAVES_MAX) void nbest_rescore_kernel(
        const long long* __restrict__ ids, const int* __restrict__ lens, const float* __restrict__ first, const long long* __restrict__ pool,
        const int* __restrict__ wtab, const int* __restrict__ ng, const RsModel M, unsigned char* ws, long long* __restrict__ out_ids,
        int* __restrict__ out_lens, float* __restrict__ out_scores, float* __restrict__ out_first, float* __restrict__ out_lm,
        int* __restrict__ out_nw, int* __restrict__ out_oov, int* __restrict__ out_order, int nbest, int T, long long sep, double alpha,
        double beta, int use_eos) {
    __shared__ double s_key[RS_NBEST_MAX], s_lm[RS_NBEST_MAX];
    __shared__ int s_nw[RS_NBEST_MAX], s_oov[RS_NBEST_MAX], s_present[RS_NBEST_MAX], s_rank[RS_NBEST_MAX];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
    const int WM = (T + 1) / 2;
    unsigned char* mine = ws + ((size_t)b * waves + wave) * 8 * (size_t)WM;
    int* wid = (int*)mine;                               // [WM] word ids, then [WM] [WM] word bounds
    u16* st = (u16*)(wid + WM);
    u16* en = st + WM;
    const size_t row0 = (size_t)b * nbest;

    for (int j = wave; j < nbest; j += waves) {          // j, and all that is read under it by every lane alike, is wave-uniform
        const float f = first[row0 + j];
        const int present = f > -INFINITY ? 1 : 0;       // -inf: no hypothesis; NaN: none either
        double lm = 0.0;
        int nw = 0, oov = 0;
        if (present) {
            const int n = __builtin_amdgcn_readfirstlane(min(max(lens[row0 + j], 0), T));
            const long long* x = ids + (row0 + j) * (size_t)T;
            nw = __builtin_amdgcn_readfirstlane(rs_segment(x, n, sep, st, en, lane));
            __threadfence_block();                       // the bounds, written by other lanes of this wave, are read below
            for (int k = lane; k < nw; k += 64) {
                const int s0 = min((int)st[k], n - 1);
                const int len = min(max((int)en[k] - s0 + 1, 1), n - s0);
                const int id = rs_word_id(M, pool, wtab, x + s0, len);
                wid[k] = id;
                oov += id == RS_UNK ? 1 : 0;
            }
            __threadfence_block();                       // and so are the word ids
            for (int k = lane; k < nw; k += 64) lm += rs_term(M, ng, wid, k, wid[k]);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                lm += __shfl_xor(lm, off, 64);
                oov += __shfl_xor(oov, off, 64);
            }
            if (use_eos && M.has_eos) lm += rs_term(M, ng, wid, nw, RS_EOS);
            __threadfence_block();                       // the next hypothesis reuses the scratch
        }
        if (lane == 0) {
            s_lm[j] = lm;
            s_nw[j] = nw;
            s_oov[j] = oov;
            s_present[j] = present;
            s_key[j] = present ? rs_sort_key(f, alpha, lm, beta, nw) : -INFINITY;
        }
    }
    __syncthreads();

    if (tid < nbest) {
        const int j = tid;
        const double key = s_key[j];
        const int present = s_present[j];
        int rank = 0;
        for (int i = 0; i < nbest; ++i)
            if (i != j && rs_ahead(s_key[i], s_present[i], i, key, present, j)) ++rank;
        s_rank[j] = rank;                                // a strict total order: the ranks are a permutation of 0 .. nbest - 1
        const size_t o = row0 + rank;
        out_order[o] = j;
        out_lens[o] = lens[row0 + j];
        out_first[o] = first[row0 + j];
        out_scores[o] = present ? (float)key : -INFINITY;
        out_lm[o] = (float)s_lm[j];
        out_nw[o] = s_nw[j];
        out_oov[o] = s_oov[j];
    }
    __syncthreads();

    for (int j = wave; j < nbest; j += waves) {          // the id rows move whole, padding included
        const long long* src = ids + (row0 + j) * (size_t)T;
        long long* dst = out_ids + (row0 + s_rank[j]) * (size_t)T;
        for (int p = lane; p < T; p += 64) dst[p] = src[p];
    }
}

extern "C" long long v100_nbest_rescore_workspace_bytes(int B, int nbest, int T) {
    if (!rs_shape_ok(B, nbest, T)) return -1;
    return (long long)B * rs_waves(nbest) * 8 * rs_words_max(T);
}

extern "C" int v100_nbest_rescore(const long long* ids, const int* lens, const float* first, const long long* pool, long long pool_len,
                                  const int* wtab, long long wtab_len, const int* ng, long long ng_len, const long long* meta, int order,
                                  int has_bos, int has_eos, void* ws, long long* out_ids, int* out_lens, float* out_scores,
                                  float* out_first, float* out_lm, int* out_nw, int* out_oov, int* out_order, int B, int nbest, int T,
                                  long long sep, double lm_weight, double word_bonus, int use_eos, void* stream) {
    if (!ids || !lens || !first || !pool || !wtab || !ng || !meta || !ws || !out_ids || !out_lens || !out_scores || !out_first || !out_lm ||
        !out_nw || !out_oov || !out_order)
        return V100_ERR_NULL;
    if (!rs_shape_ok(B, nbest, T) || order < 1 || order > RS_MAX_ORDER || pool_len < 0 || pool_len > 0x7fffffffll || wtab_len < 4 ||
        wtab_len > 0x7fffffffll || !(lm_weight - lm_weight == 0.0) || !(word_bonus - word_bonus == 0.0))       // (finite weights)
        return V100_ERR_SHAPE;
    RsModel M = {};
    M.order = order;
    M.has_bos = has_bos != 0;
    M.has_eos = has_eos != 0;
    M.pool_len = (int)pool_len;
    M.wcap = (int)(wtab_len / 4);
    for (int n = 0; n < order; ++n) {                    // meta is host memory: [order] offsets, then [order] capacities
        if (meta[n] < 0 || meta[n] > 0x7fffffffll || meta[order + n] < 1 || meta[order + n] > 0x7fffffffll) return V100_ERR_SHAPE;
        M.ng_off[n] = (int)meta[n];
        M.ng_cap[n] = (int)meta[order + n];
    }
    if (!rs_model_ok(M, wtab_len, ng_len)) return V100_ERR_SHAPE;
    V100_GGL(nbest_rescore_kernel, dim3(B), dim3(64 * rs_waves(nbest)), 0, (hipStream_t)stream, ids, lens, first, pool, wtab, ng, M,
             (unsigned char*)ws, out_ids, out_lens, out_scores, out_first, out_lm, out_nw, out_oov, out_order, nbest, T, sep, lm_weight,
             word_bonus, use_eos);
    return v100_launch_status();
}
#endif
