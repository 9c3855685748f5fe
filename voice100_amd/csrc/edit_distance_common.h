// The wave-level routines of the edit-distance kernels, shared by K23 (edit_distance.hip) and K35 (mbr.hip): the DPP neighbour shift,
// the ballot segmentation into words, and the systolic Levenshtein recurrence.  Moving them here left edit_distance_kernel's
// disassembly unchanged line for line (profiles/mbr_isa_identity.txt).
#pragma once
#include "common.h"

// lane l takes v of lane l-1; lane 0 takes `first` (DPP wave_shr:1 with bound_ctrl off keeps `old` where there is no source lane)
__device__ __forceinline__ int ed_from_left(int v, int first) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false); }

// word bounds of one row: st[k] / en[k] = first / last position of word k; returns the number of words
__device__ __forceinline__ int ed_segment(const long long* __restrict__ x, int n, long long sep, u16* st, u16* en, int lane) {
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

// rows 1 .. n against the m <= 64 S reference tokens; returns D[n][m] (n, m >= 1, wave-uniform)
template <int S>
__device__ __forceinline__ int ed_systolic(const int* __restrict__ tok_r, const int* __restrict__ tok_h, int m, int n, int lane) {
    int r[S], d[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const int c = lane * S + k;
        r[k] = c < m ? tok_r[c] : -2;                    // columns past m: computed, never read by a column <= m
        d[k] = c + 1;                                    // D[0][c + 1]
    }
    const int lm = (m - 1) / S, km = (m - 1) % S;        // the lane and register that hold column m
    int out = d[S - 1];                                  // this lane's last cell of the row it computed last
    int diag = lane * S;                                 // D[i-1][l S] of the row it computes next
    int hb = -1, h = -1;
    const int steps = n + lm;                            // lane lm computes row n at step n + lm - 1
    for (int s = 0; s < steps; ++s) {
        if ((s & 63) == 0) hb = (s + lane < n) ? tok_h[s + lane] : -1;       // the next 64 rows' tokens, one per lane
        h = ed_from_left(h, __builtin_amdgcn_readlane(hb, s & 63));          // lane 0 starts row s + 1, the others inherit
        const int left = ed_from_left(out, s + 1);                           // D[i][l S]; lane 0: D[i][0] = i
        const int i = s - lane + 1;
        if (i >= 1 && i <= n) {
            int t[S];
            int dg = diag;
#pragma unroll
            for (int k = 0; k < S; ++k) {                // the two candidates from the row above: independent of one another
                t[k] = min(d[k] + 1, dg + (r[k] != h ? 1 : 0));
                dg = d[k];
            }
            int cur = left;
#pragma unroll
            for (int k = 0; k < S; ++k) {                // the candidate from the left: the dependent chain, two VALU ops a cell
                cur = min(t[k], cur + 1);
                d[k] = cur;
            }
            diag = left;
            out = cur;
        }
    }
    int res = 0;
#pragma unroll
    for (int k = 0; k < S; ++k)
        if (k == km) res = d[k];
    return __builtin_amdgcn_readlane(res, lm);
}
