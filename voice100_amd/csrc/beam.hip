// K24: CTC prefix beam search, n best transcripts with their total log probabilities, one launch.
//
//   beam = at most W distinct label prefixes, each with (pb, pnb) = log probability of all alignments of the frames so far that
//   collapse to the prefix and end in blank / in a label.  Per frame, lp = log_softmax(x[t]), tot = pb (+) pnb, (+) = logaddexp:
//     stay    p:      pb' (+)= tot + lp[blank];  pnb' (+)= pnb + lp[e]            (e = last label of p, if any)
//     extend  p + c:  pnb' (+)= (c == e ? pb : tot) + lp[c]                       (every c != blank)
//   contributions to the same prefix merge; the W candidates of highest pb' (+) pnb' are the next beam; probability zero is dropped.
//
// One workgroup of 256 threads per utterance, no traffic between workgroups.  Per frame:
//   * identity: a prefix is a node of a trie, node = child(parent node, label), found or created through an open-addressing table
//     keyed by (parent, label) in the workgroup's own workspace region (64-bit slots {key, node}, one atomicCAS claims a slot or
//     returns its owner; load <= 1/2).  Node numbers are unique per prefix for the whole utterance, so a prefix that left the beam and
//     comes back as an extension gets its old node, and "candidate (p, c) is beam entry q" is q.parent == p.node && q.last == c;
//   * candidates: index k V + c is the extension of beam entry k by c; the slot c == blank holds the stay of k.  Each beam entry q
//     looks for its parent among the entries (<= W compares): if it is there, the extension (parent, q.last) goes into q's stay and
//     its own slot becomes -inf.  Scores in LDS, <= 64 x 128 floats;
//   * selection: radix select (8 bits a pass, one LDS histogram per pass) on the order-preserving integer image of the score finds
//     the key of rank W.  Every wave scans the histogram for itself (four bins a lane, a DPP scan, a ballot finds the lane that holds
//     the digit), so a pass costs one barrier; it stops as soon as a bin is taken whole.  Everything above the key is taken, and of
//     the keys equal to it the lowest candidate indices (an ordered compaction: a contiguous chunk of candidates per lane and a
//     scan; one wave's work up to 16 candidates a lane, all four waves' beyond).  No float compare decides a tie: two runs give
//     equal bits;
//   * new beam (one wave, one lane per entry): node lookup for the extensions, then every score is lowered by the frame's best total,
//     which goes into an fp64 offset.
// The log-softmax of frame t + 1 is taken by a second wave beside frame t's stays, from a row loaded a frame before that.  The
// barriers inside the frame loop wait for LDS only, so that row, the node stores and the table's atomics stay in flight across them.
// What a frame waits for: 3 barriers, 1 more per radix pass after the first, 2 more where all waves compact (each an LDS round trip
// plus the phase's own work), the dependent chain of the one wave that takes the stays and builds the beam, and, in a frame that
// selects an extension, one atomicCAS round trip to L2.  At the end the beam is ranked by total (ties: beam order) and the first
// nbest prefixes are read back through the parent pointers.
//
// Error: the beam's scores stay in (-inf, 0] with the best at 0, so one frame adds a few ulp of numbers of magnitude <= ~30 (the
// log-softmax, one or two logaddexp, one subtraction; exp and log are the hardware's exp2 / log2 at 1 ulp, the exponent's product
// carried in two floats): ~1e-6 absolute per frame whatever T is, against a total that falls by ~1 nat or more per frame; the offset
// is summed in fp64.  Every loop is bounded by T, W, V, 256 or the table size; scores that are NaN or -inf are no candidates, so a
// row of NaNs empties its beam and runs to the end like any other.
//
// K25: the fused form, ctc_beam_kernel<true>, ranks by key = tot + alpha lm + beta len with an n-gram language model given as a
// deterministic automaton (logp [S][V], next [S][V], final [S]).  An entry also carries its state and its LM sum; an extension by c
// adds logp[state][c] and 1 to the length and moves to next[state][c], a stay keeps all three; lm is a function of the prefix, so a
// returning prefix gets the same value from its parent and nothing is stored per node.  The candidate array holds the key (selection
// and compaction are unchanged); the wave that builds the beam takes the CTC total of a selected stay from s_stot and recomputes an
// extension's as the same sum.  The LM part is rescaled like the scores: lm is kept less that of the entry with the highest key,
// the amount goes into an fp64 offset, and the length enters as a difference from that entry's.  The CTC recurrences never see the
// LM.  ctc_beam_kernel<false> is K24, instruction for instruction.
//
// K32: the resumable form, ctc_beam_kernel<LM, true>.  Everything a frame needs from the past is the beam (in LDS), the two fp64
// offsets and the trie, so a launch that loads the first two from a per-row state in global memory, runs a chunk of frames and
// stores them again does the floating-point operations of the one-call form in its order: any split of a recording into chunks
// gives the one call's bits.  What differs: the trie is the caller's for the life of the stream, zeroed once and sized for a
// capacity in frames (the table's size enters the hash, so every launch uses all of it); a fresh node's number comes from the
// row's absolute frame index; a row without frames in a chunk stores nothing.  Reading the n best is a mode of the same kernel,
// without frames and without a store; the walk through the parent pointers is one dependent load per label of each hypothesis.
// Every index and count that comes out of the state is clamped where it is loaded, so a damaged state gives wrong text and stays
// inside the row's buffers.  ctc_beam_kernel<LM, false> is K24 / K25, instruction for instruction (the ISA of both was compared
// with the parent's: the symbol's second template argument and an unread trailing kernel argument are the difference).
#include "common.h"
#include <math.h>

#define BM_THREADS 256
#define BM_WMAX 64
#define BM_VMAX 128
#define BM_TMAX 4096
#define BM_MINSLOTS 64
#define BM_SOLO 16                                      // candidates per lane up to which one wave compacts the selection

// LDS-only barrier: the LDS traffic of every wave has landed; global loads, stores and atomics stay in flight
#define BM_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// Wave-wide scan and maximum on the DPP path: VALU moves, no LDS round trip per step (a __shfl is a ds_bpermute)
#define BM_DPP(old, v, ctrl, rows, fill) __builtin_amdgcn_update_dpp(old, v, ctrl, rows, 0xf, fill)
// inclusive prefix sum: lane l gets the sum of lanes 0 .. l
__device__ __forceinline__ int bm_wave_scan(int v) {
    v += BM_DPP(0, v, 0x111, 0xf, true);                // row_shr:1, 2, 4, 8: a scan inside each row of 16
    v += BM_DPP(0, v, 0x112, 0xf, true);
    v += BM_DPP(0, v, 0x114, 0xf, true);
    v += BM_DPP(0, v, 0x118, 0xf, true);
    v += BM_DPP(0, v, 0x142, 0xa, true);                // row_bcast:15 into rows 1 and 3
    v += BM_DPP(0, v, 0x143, 0xc, true);                // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ float bm_wave_max(float v) {
    const int ninf = __builtin_bit_cast(int, -INFINITY);
#define BM_MAXSTEP(ctrl, rows) v = fmaxf(v, __builtin_bit_cast(float, BM_DPP(ninf, __builtin_bit_cast(int, v), ctrl, rows, false)))
    BM_MAXSTEP(0x111, 0xf); BM_MAXSTEP(0x112, 0xf); BM_MAXSTEP(0x114, 0xf); BM_MAXSTEP(0x118, 0xf);
    BM_MAXSTEP(0x142, 0xa); BM_MAXSTEP(0x143, 0xc);
#undef BM_MAXSTEP
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));      // lane 63 has seen every lane
}
__device__ __forceinline__ float bm_wave_total(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wave_sum_dpp_hi(v)), 63));
}

// exp(d) for d <= 0 and log(u) for u in [1, 128] on the hardware's exp2 / log2 (1 ulp each); the product d log2(e) is carried in two
// floats so that the error of the exponent does not grow with |d|.  A handful of instructions each: they sit in one wave's
// dependent chain in every frame.
__device__ __forceinline__ float bm_exp(float d) {
    if (d < -87.0f) return 0.0f;
    const float t = d * 1.44269504089f;
    float r = fmaf(d, 1.44269504089f, -t);
    r = fmaf(d, 1.92596299e-8f, r);
    return __builtin_amdgcn_exp2f(t) * fmaf(r, 0.69314718056f, 1.0f);
}
__device__ __forceinline__ float bm_log(float u) { return __builtin_amdgcn_logf(u) * 0.69314718056f; }

__device__ __forceinline__ float bm_lae(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + bm_log(1.0f + bm_exp(fminf(a, b) - m));
}

// order-preserving image of a score; 0 = not a candidate (probability zero, or NaN).  Every finite score maps above 0x007fffff.
__device__ __forceinline__ unsigned bm_key(float s) {
    if (!(s > -INFINITY)) return 0u;
    const unsigned u = __float_as_uint(s);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

// K25: what the fused form (LM = true) takes beside K24's arguments; the plain form never reads it
struct BmLm {
    const float* logp;                                  // [S][V] natural log, back-off resolved
    const int* next;                                    // [S][V] the state after (state, label)
    const float* fin;                                   // [S] log p(</s> | state)
    float* ctc_scores;                                  // [B][nbest]
    float* lm_scores;                                   // [B][nbest]
    int S, start, use_eos;
    float alpha, beta;
};

// K32: what the resumable form (STREAM = true) takes beside that; the one-call forms never read it.  The beam of row b lives in
// state + b * stride between two launches (bm_state_bytes): {started, nbeam, frames, 0} int32, {offset, lmoff} fp64, then per entry,
// in beam order, pb, pnb, tot fp32, node, par, last, len, state int32, lm, bias fp32, W of each.
struct BmStream {
    unsigned char* state;
    long long stride;                                   // bytes per row
    int cap;                                            // the capacity in frames that the workspace was sized for
    int width;                                          // read: the width of an ids row
    int read;                                           // 0: run the frames and store the beam; 1: report the n best, store nothing
};
#define BM_STATE_HEAD 32
#define BM_STATE_FIELDS 10

template <bool LM, bool STREAM>
__global__ __launch_bounds__(BM_THREADS) void ctc_beam_kernel(const float* __restrict__ logits, const int* __restrict__ lens,
                                                              unsigned char* ws, long long* __restrict__ ids, int* __restrict__ ids_len,
                                                              float* __restrict__ scores, int T, int V, int W, int nbest, int blank,
                                                              long long region, int P, unsigned vmagic, BmLm lm, BmStream st) {
    __shared__ float s_score[BM_WMAX * BM_VMAX];        // candidate k V + c: total log probability
    __shared__ float s_lp[2][BM_VMAX];                  // frame t in s_lp[t & 1]: written one frame ahead
    __shared__ unsigned s_hist[4][256];                 // one histogram per radix pass
    __shared__ int s_sel[BM_WMAX];                      // the selected candidates, in index order
    __shared__ float s_pb[2][BM_WMAX], s_pnb[2][BM_WMAX], s_tot[2][BM_WMAX];     // the beam, double buffered
    __shared__ int s_node[2][BM_WMAX], s_par[2][BM_WMAX], s_last[2][BM_WMAX], s_len[2][BM_WMAX];
    __shared__ float s_spb[BM_WMAX], s_spnb[BM_WMAX];   // the stay of each entry
    __shared__ int s_wsum[BM_THREADS / 64];
    __shared__ int s_nbeam;                             // entries in the beam
    __shared__ int s_olen[BM_WMAX], s_onode[BM_WMAX];
    // K25 (LM only; the plain form does not touch them and they take no LDS there): per entry the automaton state, the LM log
    // probability less lmoff, the rank key's LM part bias = alpha lm + beta (len - the reference entry's), and the stay's CTC total
    __shared__ int s_state[2][BM_WMAX];
    __shared__ float s_lm[2][BM_WMAX], s_bias[2][BM_WMAX], s_stot[BM_WMAX];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = lens ? lens[b] : T;
    n = __builtin_amdgcn_readfirstlane(min(max(n, 0), T));
    // K32: the row's stored beam.  Everything read from it is clamped before it is used as an index or a count.
    unsigned char* mine_st = nullptr;
    int started = 0, t0 = 0;                            // t0: this row's frames before this launch
    if constexpr (STREAM) {
        mine_st = st.state + (size_t)b * st.stride;
        const int* head = (const int*)mine_st;
        started = __builtin_amdgcn_readfirstlane(head[0]) != 0;
        t0 = started ? __builtin_amdgcn_readfirstlane(min(max(head[2], 0), st.cap)) : 0;
        n = st.read ? 0 : min(n, st.cap - t0);          // no node number beyond the workspace, whatever the caller counted
    }
    const int cap = STREAM ? st.cap : T;                // the frames that the trie holds
    const int OT = STREAM ? st.width : T;               // the width of an ids row
    const float* x = logits + (size_t)b * T * V;
    unsigned long long* table = (unsigned long long*)(ws + (size_t)b * region);          // [P] {key << 32 | node}, 0 = free
    unsigned* nodes = (unsigned*)(table + P);                                            // [1 + W T] parent << 7 | label
    const int maxnode = W * cap;                                                         // the largest node number
    int Pb = BM_MINSLOTS;                               // this row's table: 2 W n slots, of the P = 2 W T that the region holds
    if constexpr (STREAM) Pb = P;                       // K32: all of them, in every launch: the size enters the hash
    else while (Pb < 2 * W * n) Pb <<= 1;
    const int shift = 32 - __builtin_ctz(Pb);

    if constexpr (!STREAM) {
        uint4* tz = (uint4*)table;
        for (int i = tid; i < Pb / 2; i += BM_THREADS) tz[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    if constexpr (STREAM) {
        if (started && wave == 0) {                     // the beam as the last launch left it, in its order
            const int nb0 = min(max(((const int*)mine_st)[1], 0), W);
            if (lane < nb0) {
                const float* f = (const float*)(mine_st + BM_STATE_HEAD);
                const int* q = (const int*)f;
                s_pb[0][lane] = f[lane]; s_pnb[0][lane] = f[W + lane]; s_tot[0][lane] = f[2 * W + lane];
                s_node[0][lane] = min(max(q[3 * W + lane], 0), maxnode);
                s_par[0][lane] = min(max(q[4 * W + lane], -1), maxnode);
                s_last[0][lane] = min(max(q[5 * W + lane], -1), V - 1);
                s_len[0][lane] = q[6 * W + lane];       // clamped where it is reported
                if constexpr (LM) {
                    s_state[0][lane] = min(max(q[7 * W + lane], 0), lm.S - 1);
                    s_lm[0][lane] = f[8 * W + lane]; s_bias[0][lane] = f[9 * W + lane];
                }
            }
            if (lane == 0) s_nbeam = nb0;
        }
    }
    if (tid == 0 && !started) {
        nodes[0] = 0u;
        s_pb[0][0] = 0.0f; s_pnb[0][0] = -INFINITY; s_tot[0][0] = 0.0f;
        s_node[0][0] = 0; s_par[0][0] = -1; s_last[0][0] = -1; s_len[0][0] = 0;
        s_nbeam = 1;
        if constexpr (LM) { s_state[0][0] = lm.start; s_lm[0][0] = 0.0f; s_bias[0][0] = 0.0f; }
    }
    float r0 = -INFINITY, r1 = -INFINITY;               // wave 1: a frame's logits, two per lane
    auto load_row = [&](int t) {
        const float* xt = x + (size_t)t * V;
        if (lane < V) r0 = xt[lane];
        if (lane + 64 < V) r1 = xt[lane + 64];
    };
    auto log_softmax_row = [&](float* dst) {
        const float m = bm_wave_max(fmaxf(r0, r1));
        const float e = (lane < V ? bm_exp(r0 - m) : 0.0f) + (lane + 64 < V ? bm_exp(r1 - m) : 0.0f);
        const float lse = m + bm_log(bm_wave_total(e));
        if (lane < V) dst[lane] = r0 - lse;
        if (lane + 64 < V) dst[lane + 64] = r1 - lse;
    };
    if (wave == 1 && n > 0) {
        load_row(0);
        log_softmax_row(s_lp[0]);
        if (n > 1) load_row(1);
    }
    __threadfence();                                    // the zeroed table is in L2, where the atomics execute
    __syncthreads();

    double offset = 0.0;                                // wave 0: what the rescaling has taken out of the scores so far
    double lmoff = 0.0;                                 // K25, wave 0: what it has taken out of the LM log probabilities
    if constexpr (STREAM) {
        if (started) { offset = ((const double*)mine_st)[2]; lmoff = ((const double*)mine_st)[3]; }
    }
    int cur = 0;
    for (int t = 0; t < n; ++t) {
        const int nb = __builtin_amdgcn_readfirstlane(s_nbeam);
        const int N = nb * V;
        const float* lp = s_lp[t & 1];
#pragma unroll
        for (int i = 0; i < 4; ++i) s_hist[i][tid] = 0u;    // every wave is past the last frame's scans
        if (wave == 1 && t + 1 < n) {                   // the next frame's log-softmax, beside this frame's stays; its buffer was last
            log_softmax_row(s_lp[(t + 1) & 1]);         // read in frame t - 1
            if (t + 2 < n) load_row(t + 2);             // in flight across a whole frame
        }

        // stays (one thread per entry) and extensions (all threads)
        float stot = -INFINITY;
        int kill = -1;
        if (wave == 0) {
            const bool live = lane < nb;
            const int e = live ? s_last[cur][lane] : -1, pq = live ? s_par[cur][lane] : -2, mine = live ? s_node[cur][lane] : -3;
            int k = -1;                                 // the entry that is this prefix' parent, if it is in the beam
            for (int i = 0; i < nb; ++i)
                if (__builtin_amdgcn_readlane(mine, i) == pq) k = i;
            if (live) {
                const float spb = s_tot[cur][lane] + lp[blank];
                float spnb = e >= 0 ? s_pnb[cur][lane] + lp[e] : -INFINITY;
                if (k >= 0 && e >= 0) {                 // the parent's extension by e is this prefix
                    const float base = s_last[cur][k] == e ? s_pb[cur][k] : s_tot[cur][k];
                    spnb = bm_lae(spnb, base + lp[e]);
                    kill = k * V + e;
                }
                s_spb[lane] = spb;
                s_spnb[lane] = spnb;
                stot = bm_lae(spb, spnb);
                if constexpr (LM) s_stot[lane] = stot;
            }
        }
        for (int idx = tid; idx < N; idx += BM_THREADS) {
            const int k = (int)__umulhi((unsigned)idx, vmagic), c = idx - k * V;
            const float base = s_last[cur][k] == c ? s_pb[cur][k] : s_tot[cur][k];
            if constexpr (LM) {                         // the rank key; a CTC total of -inf or NaN stays "no candidate"
                const float ctc = base + lp[c];
                const float l = lm.logp[(size_t)s_state[cur][k] * V + c];       // the states are inside [0, S): clamped where they are set
                s_score[idx] = ctc > -INFINITY ? ctc + (s_bias[cur][k] + (lm.alpha * l + lm.beta)) : -INFINITY;
            } else {
                s_score[idx] = base + lp[c];
            }
        }
        BM_BARRIER();
        if (tid < nb) {
            if constexpr (LM) s_score[tid * V + blank] = stot > -INFINITY ? stot + s_bias[cur][tid] : -INFINITY;
            else s_score[tid * V + blank] = stot;
            if (kill >= 0) s_score[kill] = -INFINITY;
        }
        BM_BARRIER();

        // selection: the key of rank W by radix select, most significant byte first.  Every wave scans the histogram for itself
        // (four bins a lane, a DPP scan, the lane that holds the digit found by a ballot), so a pass costs one barrier.
        const int chunk = (N + BM_THREADS - 1) / BM_THREADS;
        const int lo = min(tid * chunk, N), hi = min(lo + chunk, N);
        for (int idx = lo; idx < hi; ++idx) {
            const unsigned key = bm_key(s_score[idx]);
            if (key) atomicAdd(&s_hist[3][key >> 24], 1u);
        }
        BM_BARRIER();
        unsigned prefix = 0u, mask = 0u;
        int nvalid = 0, remaining = 0;
        for (int pass = 3; pass >= 0; --pass) {
            if (pass < 3) {
                for (int idx = lo; idx < hi; ++idx) {
                    const unsigned key = bm_key(s_score[idx]);
                    if (key && (key & mask) == prefix) atomicAdd(&s_hist[pass][(key >> (8 * pass)) & 255u], 1u);
                }
                BM_BARRIER();
            }
            int h[4], sum = 0;                          // lane l holds digits 255 - 4 l - j: the scan over the lanes counts from the top
#pragma unroll
            for (int j = 0; j < 4; ++j) { h[j] = (int)s_hist[pass][255 - 4 * lane - j]; sum += h[j]; }
            const int S = bm_wave_scan(sum);
            if (pass == 3) {
                nvalid = __builtin_amdgcn_readlane(S, 63);               // every candidate of probability > 0
                remaining = min(W, nvalid);
                if (nvalid <= W) break;                 // fewer candidates than places: all of them (mask 0: every key "equals" the prefix)
            }
            int acc = S - sum, digit = 0, rem = 0, exact = 0;
            const bool hit = S >= remaining && acc < remaining;          // exactly one lane
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (hit && acc < remaining && acc + h[j] >= remaining) {
                    digit = 255 - 4 * lane - j;
                    rem = remaining - acc;
                    exact = h[j] == rem;
                }
                acc += h[j];
            }
            const unsigned long long who = __ballot(hit);
            const int src = who ? __builtin_ctzll(who) : 0;
            prefix |= (unsigned)__builtin_amdgcn_readlane(digit, src) << (8 * pass);
            mask |= 0xffu << (8 * pass);
            remaining = __builtin_amdgcn_readlane(rem, src);
            if (__builtin_amdgcn_readlane(exact, src)) break;            // every key under this prefix is taken: the lower bytes decide nothing
        }

        // ordered compaction: above the prefix, then the first `remaining` of those equal to it.  Up to 16 candidates a lane it is
        // wave 0's alone (its own LDS traffic is in order: no barrier before it reads the list back); beyond, all four waves' with
        // one exchange of the waves' counts.
        auto compact = [&](int c0, int c1, int base) {
            int gb = base & 0xffff, eb = base >> 16;
            for (int idx = c0; idx < c1; ++idx) {
                const unsigned key = bm_key(s_score[idx]);
                if (!key) continue;
                int pos = -1;
                if ((key & mask) > prefix) { pos = gb + min(eb, remaining); ++gb; }
                else if ((key & mask) == prefix) { if (eb < remaining) pos = gb + eb; ++eb; }
                if (pos >= 0 && pos < BM_WMAX) s_sel[pos] = idx;
            }
        };
        auto count = [&](int c0, int c1) {
            int g = 0, e = 0;
            for (int idx = c0; idx < c1; ++idx) {
                const unsigned key = bm_key(s_score[idx]);
                if (key) {
                    g += (key & mask) > prefix;
                    e += (key & mask) == prefix;
                }
            }
            return g | (e << 16);                       // both counts <= 8192
        };
        if (N <= 64 * BM_SOLO) {
            if (wave == 0) {
                const int ch = (N + 63) / 64, c0 = min(lane * ch, N), c1 = min(c0 + ch, N);
                const int packed = count(c0, c1);
                compact(c0, c1, bm_wave_scan(packed) - packed);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        } else {
            const int packed = count(lo, hi);
            const int incl = bm_wave_scan(packed);
            if (lane == 63) s_wsum[wave] = incl;
            BM_BARRIER();
            int excl = incl - packed;
            for (int w = 0; w < wave; ++w) excl += s_wsum[w];
            compact(lo, hi, excl);
            BM_BARRIER();
        }

        // the next beam (wave 0)
        const int nsel = min(W, nvalid);
        const int nx = cur ^ 1;
        if (wave == 0) {
            float pb = -INFINITY, pnb = -INFINITY, tot = -INFINITY;
            int node = 0, par = -1, last = -1, len = 0;
            float key = -INFINITY, lmv = 0.0f;          // K25: the rank key, the LM log probability and the state of the new entry
            int state = 0;
            if (lane < nsel) {
                const int idx = s_sel[lane];
                const int k = (int)__umulhi((unsigned)idx, vmagic), c = idx - k * V;
                tot = s_score[idx];
                if constexpr (LM) {                     // s_score holds the key: the CTC total is the stay's, or the same sum again
                    key = tot;
                    state = s_state[cur][k];
                    lmv = s_lm[cur][k];
                    if (c == blank) {
                        tot = s_stot[k];
                    } else {
                        const size_t at = (size_t)state * V + c;    // both loads are under way while the table is asked
                        const float l = lm.logp[at];
                        const int to = lm.next[at];
                        tot = (s_last[cur][k] == c ? s_pb[cur][k] : s_tot[cur][k]) + lp[c];
                        lmv += l;
                        state = min(max(to, 0), lm.S - 1);
                    }
                }
                if (c == blank) {
                    pb = s_spb[k]; pnb = s_spnb[k];
                    node = s_node[cur][k]; par = s_par[cur][k]; last = s_last[cur][k]; len = s_len[cur][k];
                } else {
                    pnb = tot;
                    last = c; len = s_len[cur][k] + 1; par = s_node[cur][k];
                    const unsigned fresh = 1u + (unsigned)(t0 + t) * (unsigned)W + (unsigned)lane;       // <= W T (K32: W cap)
                    const unsigned key = (unsigned)par * 128u + (unsigned)c + 1u;                // < 2^27
                    const unsigned long long mine = ((unsigned long long)key << 32) | fresh;
                    unsigned slot = (key * 0x9E3779B1u) >> shift;
                    node = (int)fresh;
                    for (int probe = 0; probe < Pb; ++probe) {
                        const unsigned long long old = atomicCAS(&table[slot], 0ull, mine);
                        if (old == 0ull) { nodes[fresh] = ((unsigned)par << 7) | (unsigned)c; break; }       // a new prefix
                        if ((unsigned)(old >> 32) == key) { node = (int)(unsigned)(old & 0xffffffffull); break; }
                        slot = (slot + 1u) & (unsigned)(Pb - 1);                                 // another prefix' slot
                    }
                }
            }
            const float best = bm_wave_max(tot);
            if (lane < nsel) {
                s_pb[nx][lane] = pb - best; s_pnb[nx][lane] = pnb - best; s_tot[nx][lane] = tot - best;
                s_node[nx][lane] = node; s_par[nx][lane] = par; s_last[nx][lane] = last; s_len[nx][lane] = len;
            }
            if constexpr (LM) {                         // the LM part is kept relative to the entry of the highest key (ties: the first)
                const float top = bm_wave_max(key);
                const unsigned long long who = __ballot(lane < nsel && key == top);
                const int src = who ? __builtin_ctzll(who) : 0;
                const float lmref = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, lmv), src));
                const int lenref = __builtin_amdgcn_readlane(len, src);
                if (lane < nsel) {
                    const float rel = lmv - lmref;
                    s_state[nx][lane] = state; s_lm[nx][lane] = rel;
                    s_bias[nx][lane] = lm.alpha * rel + lm.beta * (float)(len - lenref);
                }
                if (nsel > 0) lmoff += (double)lmref;
            }
            if (nsel > 0) offset += (double)best;
            if (lane == 0) s_nbeam = nsel;
        }
        cur = nx;
        BM_BARRIER();
    }

    if constexpr (STREAM) {
        if (!st.read) {                                 // K32: store the beam; a row without frames keeps what it had, bit for bit
            if (wave == 0 && n > 0) {
                const int nbs = s_nbeam;
                float* f = (float*)(mine_st + BM_STATE_HEAD);
                int* q = (int*)f;
                if (lane < nbs) {
                    f[lane] = s_pb[cur][lane]; f[W + lane] = s_pnb[cur][lane]; f[2 * W + lane] = s_tot[cur][lane];
                    q[3 * W + lane] = s_node[cur][lane]; q[4 * W + lane] = s_par[cur][lane];
                    q[5 * W + lane] = s_last[cur][lane]; q[6 * W + lane] = s_len[cur][lane];
                    if constexpr (LM) {
                        q[7 * W + lane] = s_state[cur][lane]; f[8 * W + lane] = s_lm[cur][lane]; f[9 * W + lane] = s_bias[cur][lane];
                    }
                }
                if (lane == 0) {
                    int* head = (int*)mine_st;
                    head[0] = 1; head[1] = nbs; head[2] = t0 + n; head[3] = 0;
                    ((double*)mine_st)[2] = offset; ((double*)mine_st)[3] = lmoff;
                }
            }
            return;
        }
    }

    // rank the beam by total (ties: beam order), report the first nbest
    const int nb = s_nbeam;
    if (wave == 0) {
        float tot = lane < nb ? s_tot[cur][lane] : -INFINITY;
        if constexpr (LM) {                             // rank by the key, with alpha log p(</s> | state) where the caller wants it
            if (lane < nb) {
                const float fin = lm.use_eos ? lm.fin[min(max(s_state[cur][lane], 0), lm.S - 1)] : 0.0f;
                const float all = s_lm[cur][lane] + fin;
                s_lm[cur][lane] = all;
                tot = tot > -INFINITY ? tot + (s_bias[cur][lane] + lm.alpha * fin) : -INFINITY;
                if (!(tot == tot)) tot = -INFINITY;
            }
            s_spb[lane] = tot;
        }
        int rank = 0;
        for (int i = 0; i < nb; ++i) {
            const float ti = LM ? s_spb[i] : s_tot[cur][i];
            rank += (ti > tot) || (ti == tot && i < lane);
        }
        if (lane < nb) s_sel[rank] = lane;
    }
    __syncthreads();
    if (wave == 0 && lane < nbest) {
        int len = 0, node = 0;
        float sc = -INFINITY;
        double lmsum = 0.0, ctc64 = 0.0;
        if (lane < nb) {
            const int j = min(max(s_sel[lane], 0), BM_WMAX - 1);
            len = min(max(s_len[cur][j], 0), STREAM ? min(t0, OT) : n);       // K32: the frames so far, not this launch's
            node = s_node[cur][j];
            ctc64 = (double)s_tot[cur][j] + offset;
            sc = (float)ctc64;
            if constexpr (LM) lmsum = (double)s_lm[cur][j] + lmoff;
        }
        if constexpr (LM) {                             // the key in fp64 from its three parts; -inf, -inf, 0 where there is no hypothesis
            lm.ctc_scores[(size_t)b * nbest + lane] = sc;
            lm.lm_scores[(size_t)b * nbest + lane] = (float)lmsum;
            if (lane < nb) sc = (float)(ctc64 + (double)lm.alpha * lmsum + (double)lm.beta * (double)len);
        }
        scores[(size_t)b * nbest + lane] = sc;
        ids_len[(size_t)b * nbest + lane] = len;
        s_olen[lane] = len;
        s_onode[lane] = node;
    }
    __syncthreads();
    long long* out = ids + (size_t)b * nbest * OT;
    for (int r = 0; r < nbest; ++r)
        for (int i = s_olen[r] + tid; i < OT; i += BM_THREADS) out[(size_t)r * OT + i] = 0;
    if (tid < nbest) {                                  // the labels, last to first, through the parent pointers: one dependent
        int p = s_onode[tid];                           // load per label
        for (int i = s_olen[tid] - 1; i >= 0; --i) {
            const unsigned v = nodes[min(max(p, 0), maxnode)];
            out[(size_t)tid * OT + i] = (long long)(v & 127u);
            p = (int)(v >> 7);
        }
    }
}

static inline bool bm_shape_ok(int B, int T, int V, int W) {
    return B >= 1 && T >= 1 && T <= BM_TMAX && V >= 2 && V <= BM_VMAX && W >= 1 && W <= BM_WMAX;
}
static inline int bm_slots(int T, int W) {
    int P = BM_MINSLOTS;
    while (P < 2 * W * T) P <<= 1;                       // <= 2^19
    return P;
}
static inline long long bm_region(int T, int W) { return 8ll * bm_slots(T, W) + 4ll * ((1 + W * T + 3) & ~3); }

extern "C" long long v100_ctc_beam_workspace_bytes(int B, int T, int V, int W) {
    if (!bm_shape_ok(B, T, V, W)) return -1;
    return (long long)B * bm_region(T, W);
}

extern "C" int v100_ctc_beam_search(const float* logits, const int* lens, void* ws, long long* ids, int* ids_len, float* scores, int B,
                                    int T, int V, int W, int nbest, int blank, void* stream) {
    if (!logits || !ws || !ids || !ids_len || !scores) return V100_ERR_NULL;
    if (!bm_shape_ok(B, T, V, W) || nbest < 1 || nbest > W || blank < 0 || blank >= V) return V100_ERR_SHAPE;
    const unsigned vmagic = (unsigned)((1ull << 32) / (unsigned)V) + 1u;     // idx / V == umulhi(idx, vmagic) for idx < 2^13, V <= 128
    V100_GGL((ctc_beam_kernel<false, false>), dim3(B), dim3(BM_THREADS), 0, (hipStream_t)stream, logits, lens, (unsigned char*)ws, ids,
             ids_len, scores, T, V, W, nbest, blank, bm_region(T, W), bm_slots(T, W), vmagic, BmLm{}, BmStream{});
    return v100_launch_status();
}

// K25: the same search ranked by log p_ctc + alpha log p_lm + beta length (see the header); the workspace is K24's
extern "C" int v100_ctc_beam_search_lm(const float* logits, const int* lens, void* ws, long long* ids, int* ids_len, float* scores,
                                       const float* lm_logp, const int* lm_next, const float* lm_final, int S, int start_state,
                                       float alpha, float beta, int use_eos, float* ctc_scores, float* lm_scores, int B, int T, int V,
                                       int W, int nbest, int blank, void* stream) {
    if (!logits || !ws || !ids || !ids_len || !scores || !lm_logp || !lm_next || !lm_final || !ctc_scores || !lm_scores)
        return V100_ERR_NULL;
    if (!bm_shape_ok(B, T, V, W) || nbest < 1 || nbest > W || blank < 0 || blank >= V) return V100_ERR_SHAPE;
    if (S < 1 || (long long)S * V > (1ll << 28) || start_state < 0 || start_state >= S || !(alpha == alpha) || !(beta == beta) ||
        fabsf(alpha) == INFINITY || fabsf(beta) == INFINITY)
        return V100_ERR_SHAPE;
    const unsigned vmagic = (unsigned)((1ull << 32) / (unsigned)V) + 1u;
    const BmLm lm{lm_logp, lm_next, lm_final, ctc_scores, lm_scores, S, start_state, use_eos != 0, alpha, beta};
    V100_GGL((ctc_beam_kernel<true, false>), dim3(B), dim3(BM_THREADS), 0, (hipStream_t)stream, logits, lens, (unsigned char*)ws, ids,
             ids_len, scores, T, V, W, nbest, blank, bm_region(T, W), bm_slots(T, W), vmagic, lm, BmStream{});
    return v100_launch_status();
}

// K32: the resumable form.  The caller owns two buffers, both zeroed once when the stream is created: the workspace (per row the child
// table and the nodes, sized for max_frames frames) and the state (per row the beam between two launches).
static inline bool bm_stream_ok(int B, int F, int V, int W) {
    return B >= 1 && F >= 1 && V >= 2 && V <= BM_VMAX && W >= 1 && W <= BM_WMAX && (long long)W * F < (1ll << 25);
}
static inline long long bm_state_bytes(int W) { return (BM_STATE_HEAD + 4ll * BM_STATE_FIELDS * W + 15) & ~15ll; }

extern "C" long long v100_ctc_beam_stream_workspace_bytes(int B, int max_frames, int V, int W) {
    if (!bm_stream_ok(B, max_frames, V, W)) return -1;
    return (long long)B * bm_region(max_frames, W);
}

extern "C" long long v100_ctc_beam_stream_state_bytes(int B, int W) {
    if (B < 1 || W < 1 || W > BM_WMAX) return -1;
    return (long long)B * bm_state_bytes(W);
}

template <bool LM>
static int bm_stream_launch(const float* logits, const int* lens, void* ws, void* state, long long* ids, int* ids_len, float* scores,
                            const BmLm& lm, int B, int T, int F, int V, int W, int nbest, int blank, int width, int read, void* stream) {
    const unsigned vmagic = (unsigned)((1ull << 32) / (unsigned)V) + 1u;
    const BmStream st{(unsigned char*)state, bm_state_bytes(W), F, width, read};
    V100_GGL((ctc_beam_kernel<LM, true>), dim3(B), dim3(BM_THREADS), 0, (hipStream_t)stream, logits, lens, (unsigned char*)ws, ids,
             ids_len, scores, T, V, W, nbest, blank, bm_region(F, W), bm_slots(F, W), vmagic, lm, st);
    return v100_launch_status();
}
static inline bool bm_lm_ok(int S, int V, int start_state, float alpha, float beta) {
    return S >= 1 && (long long)S * V <= (1ll << 28) && start_state >= 0 && start_state < S && alpha == alpha && beta == beta &&
           fabsf(alpha) != INFINITY && fabsf(beta) != INFINITY;
}

extern "C" int v100_ctc_beam_stream_push(const float* logits, const int* lens, void* ws, void* state, int B, int T, int max_frames, int V,
                                         int W, int blank, void* stream) {
    if (!logits || !ws || !state) return V100_ERR_NULL;
    if (!bm_stream_ok(B, max_frames, V, W) || T < 1 || T > BM_TMAX || blank < 0 || blank >= V) return V100_ERR_SHAPE;
    return bm_stream_launch<false>(logits, lens, ws, state, nullptr, nullptr, nullptr, BmLm{}, B, T, max_frames, V, W, 1, blank, 1, 0,
                                   stream);
}

extern "C" int v100_ctc_beam_stream_push_lm(const float* logits, const int* lens, void* ws, void* state, const float* lm_logp,
                                            const int* lm_next, const float* lm_final, int S, int start_state, float alpha, float beta,
                                            int B, int T, int max_frames, int V, int W, int blank, void* stream) {
    if (!logits || !ws || !state || !lm_logp || !lm_next || !lm_final) return V100_ERR_NULL;
    if (!bm_stream_ok(B, max_frames, V, W) || T < 1 || T > BM_TMAX || blank < 0 || blank >= V) return V100_ERR_SHAPE;
    if (!bm_lm_ok(S, V, start_state, alpha, beta)) return V100_ERR_SHAPE;
    const BmLm lm{lm_logp, lm_next, lm_final, nullptr, nullptr, S, start_state, 0, alpha, beta};
    return bm_stream_launch<true>(logits, lens, ws, state, nullptr, nullptr, nullptr, lm, B, T, max_frames, V, W, 1, blank, 1, 0, stream);
}

extern "C" int v100_ctc_beam_stream_read(const void* ws, const void* state, long long* ids, int* ids_len, float* scores, int B,
                                         int max_frames, int V, int W, int nbest, int width, void* stream) {
    if (!ws || !state || !ids || !ids_len || !scores) return V100_ERR_NULL;
    if (!bm_stream_ok(B, max_frames, V, W) || nbest < 1 || nbest > W || width < 1) return V100_ERR_SHAPE;
    return bm_stream_launch<false>(nullptr, nullptr, (void*)ws, (void*)state, ids, ids_len, scores, BmLm{}, B, 1, max_frames, V, W, nbest, 0,
                                   width, 1, stream);
}

extern "C" int v100_ctc_beam_stream_read_lm(const void* ws, const void* state, long long* ids, int* ids_len, float* scores,
                                            const float* lm_final, int S, int start_state, float alpha, float beta, int final,
                                            float* ctc_scores, float* lm_scores, int B, int max_frames, int V, int W, int nbest, int width,
                                            void* stream) {
    if (!ws || !state || !ids || !ids_len || !scores || !lm_final || !ctc_scores || !lm_scores) return V100_ERR_NULL;
    if (!bm_stream_ok(B, max_frames, V, W) || nbest < 1 || nbest > W || width < 1) return V100_ERR_SHAPE;
    if (!bm_lm_ok(S, V, start_state, alpha, beta)) return V100_ERR_SHAPE;
    const BmLm lm{nullptr, nullptr, lm_final, ctc_scores, lm_scores, S, start_state, final != 0, alpha, beta};
    return bm_stream_launch<true>(nullptr, nullptr, (void*)ws, (void*)state, ids, ids_len, scores, lm, B, 1, max_frames, V, W, nbest, 0,
                                  width, 1, stream);
}
