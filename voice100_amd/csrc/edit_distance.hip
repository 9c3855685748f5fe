// K23: batched edit distance (Levenshtein, unit costs) between two zero-padded id batches, at the id level and at the word level.
//
//   D[0][j] = j, D[i][0] = i, D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + (hyp token i != ref token j)); dist = D[n][m].
//
// One wave of 64 lanes per (pair, level); both levels of a batch are the two grid rows of ONE launch.  Three phases, one wave each:
//   1. segmentation (word level only): a token is a maximal run of ids != sep inside the row's length.  64 positions at a time, a
//      ballot of the run starts and one of the run ends; the k-th start and the k-th end are word k (prefix popcounts, no atomics);
//   2. canonical tokens: every token (an id, or a word) is hashed over all 64 bits of its ids and inserted into an open-addressing
//      table in LDS (atomicCAS on the slot, linear probing, load <= 1/2).  A slot holds the index of the first token that claimed
//      it; a later token takes that index as its own only after its length and every id have been compared, otherwise it probes
//      on -- the hash only finds candidates, equality is decided on the ids.  From here on a token is one int32, and two tokens
//      of a pair are equal iff their int32s are (which token of a class claimed the slot does not matter to the distance);
//   3. the recurrence as a systolic array: lane l owns the strip of S reference columns l*S+1 .. l*S+S (row D[i-1][.] of the strip
//      and its tokens in registers, S a compile-time 1, 2, 4, ... 64: the smallest with 64 S >= m), at step s it computes row
//      i = s - l + 1, and takes D[i][l*S] -- lane l-1's last cell of the step before -- and the row's token from its left
//      neighbour by a DPP wave shift (a VALU move, no LDS round trip, no barrier).  A pair costs n + (m-1)/S steps.
// Nothing beyond a row's length is read.  Scratch: the canonical tokens and the word bounds, 8 bytes per id and level, in global
// memory (written and read by the same wave, across a workgroup barrier), so that LDS holds the table only (<= 64 KiB).
#include "edit_distance_common.h"

#define ED_TMAX 4096
#define ED_EMPTY 0xffffffffu

__global__ __launch_bounds__(64) void edit_distance_kernel(const long long* __restrict__ hyp, const int* __restrict__ hyp_len,
                                                           const long long* __restrict__ ref, const int* __restrict__ ref_len,
                                                           unsigned char* ws, int* __restrict__ dist, int* __restrict__ hyp_n,
                                                           int* __restrict__ ref_n, unsigned long long* totals, int B, int Th, int Tr,
                                                           int levels, long long sep, int P) {
    extern __shared__ unsigned ed_tab[];                 // [P] open-addressing table: index of the token that owns the slot
    const int b = blockIdx.x, lev = blockIdx.y, lane = threadIdx.x;
    const bool words = levels == 2 || lev == 1;
    const long long* hb = hyp + (size_t)b * Th;
    const long long* rb = ref + (size_t)b * Tr;
    int nh = __builtin_amdgcn_readfirstlane(min(max(hyp_len[b], 0), Th));
    int nr = __builtin_amdgcn_readfirstlane(min(max(ref_len[b], 0), Tr));

    unsigned char* base = ws + ((size_t)lev * B + b) * 8 * (size_t)(Th + Tr);
    int* tok = (int*)base;                               // [Tr + Th] canonical tokens: the reference's, then the hypothesis'
    u16* st_r = (u16*)(tok + Th + Tr);                   // [Tr] [Tr] [Th] [Th] word bounds
    u16* en_r = st_r + Tr;
    u16* st_h = en_r + Tr;
    u16* en_h = st_h + Th;

    for (int i = lane; i < P; i += 64) ed_tab[i] = ED_EMPTY;
    int n = nh, m = nr;                                  // tokens of the hypothesis (rows) and of the reference (columns)
    if (words) {
        m = __builtin_amdgcn_readfirstlane(ed_segment(rb, nr, sep, st_r, en_r, lane));
        n = __builtin_amdgcn_readfirstlane(ed_segment(hb, nh, sep, st_h, en_h, lane));
    }
    __syncthreads();                                     // the table and the word bounds are visible to every lane

    auto token = [&](int g, const long long*& p, int& len) {
        const bool is_ref = g < m;
        const int w = is_ref ? g : g - m;
        const long long* row = is_ref ? rb : hb;
        int s0 = w;
        len = 1;
        if (words) {
            s0 = is_ref ? st_r[w] : st_h[w];
            len = (is_ref ? en_r[w] : en_h[w]) - s0 + 1;
        }
        p = row + s0;
    };
    for (int g = lane; g < m + n; g += 64) {
        const long long* p;
        int len;
        token(g, p, len);
        unsigned long long h = (unsigned long long)len * 0xD6E8FEB86659FD93ull;
        for (int i = 0; i < len; ++i) {
            h = (h ^ (unsigned long long)p[i]) * 0x9E3779B97F4A7C15ull;
            h ^= h >> 29;
        }
        unsigned slot = (unsigned)(h ^ (h >> 32)) & (unsigned)(P - 1);
        int id;
        for (;;) {
            const unsigned cur = atomicCAS(&ed_tab[slot], ED_EMPTY, (unsigned)g);
            if (cur == ED_EMPTY) { id = g; break; }      // first of its class
            const long long* q;
            int qlen;
            token((int)cur, q, qlen);
            bool same = qlen == len;
            for (int i = 0; same && i < len; ++i) same = q[i] == p[i];
            if (same) { id = (int)cur; break; }
            slot = (slot + 1) & (unsigned)(P - 1);       // another token's slot: at most (m + n) <= P / 2 slots are ever taken
        }
        tok[g] = id;
    }
    __syncthreads();                                     // the tokens are visible to every lane

    int dd;
    if (n == 0 || m == 0) dd = max(n, m);
    else if (m <= 64) dd = ed_systolic<1>(tok, tok + m, m, n, lane);
    else if (m <= 128) dd = ed_systolic<2>(tok, tok + m, m, n, lane);
    else if (m <= 256) dd = ed_systolic<4>(tok, tok + m, m, n, lane);
    else if (m <= 512) dd = ed_systolic<8>(tok, tok + m, m, n, lane);
    else if (m <= 1024) dd = ed_systolic<16>(tok, tok + m, m, n, lane);
    else if (m <= 2048) dd = ed_systolic<32>(tok, tok + m, m, n, lane);
    else dd = ed_systolic<64>(tok, tok + m, m, n, lane);

    if (lane == 0) {
        if (dist) {
            dist[(size_t)lev * B + b] = dd;
            hyp_n[(size_t)lev * B + b] = n;
            ref_n[(size_t)lev * B + b] = m;
        }
        if (totals) {                                    // integer adds: the sums do not depend on the order
            atomicAdd(totals + 3 * lev + 0, (unsigned long long)dd);
            atomicAdd(totals + 3 * lev + 1, (unsigned long long)n);
            atomicAdd(totals + 3 * lev + 2, (unsigned long long)m);
        }
    }
}

static inline bool ed_shape_ok(int B, int Th, int Tr) { return B >= 1 && Th >= 1 && Th <= ED_TMAX && Tr >= 1 && Tr <= ED_TMAX; }

extern "C" long long v100_edit_distance_workspace_bytes(int B, int Th, int Tr) {
    if (!ed_shape_ok(B, Th, Tr)) return -1;
    return 2ll * B * 8 * (Th + Tr);                      // both levels
}

extern "C" int v100_edit_distance(const long long* hyp, const int* hyp_len, const long long* ref, const int* ref_len, void* ws, int* dist,
                                  int* hyp_n, int* ref_n, long long* totals, int B, int Th, int Tr, int levels, long long sep, void* stream) {
    if (!hyp || !hyp_len || !ref || !ref_len || !ws) return V100_ERR_NULL;
    const bool rows = dist && hyp_n && ref_n;
    if ((!rows && (dist || hyp_n || ref_n)) || (!rows && !totals)) return V100_ERR_NULL;     // the three per-row outputs together, or the totals
    if (!ed_shape_ok(B, Th, Tr) || levels < 1 || levels > 3) return V100_ERR_SHAPE;
    int P = 128;
    while (P < 2 * (Th + Tr)) P <<= 1;                   // <= 16384 slots = 64 KiB
    V100_GGL(edit_distance_kernel, dim3(B, levels == 3 ? 2 : 1), dim3(64), (size_t)P * sizeof(unsigned), (hipStream_t)stream, hyp, hyp_len,
             ref, ref_len, (unsigned char*)ws, dist, hyp_n, ref_n, (unsigned long long*)totals, B, Th, Tr, levels, sep, P);
    return v100_launch_status();
}
