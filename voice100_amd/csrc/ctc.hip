// K10: log_softmax + CTC loss + its gradient w.r.t. the logits, fused (asr.py:148-152:
// F.log_softmax(dim=-1) then nn.CTCLoss(blank=0, reduction='mean', zero_infinity=True)).
//
// The stock PyTorch-ROCm CTC kernels cost ~1.6 ms per step at the benchmark shape (T'=512, B=32, L=100),
// almost all of it latency of a 512-step serial recursion.  Here one workgroup owns one (utterance,
// direction): the alpha (forward) and beta (backward) lattices run concurrently, log-probabilities are
// staged through LDS 64 frames at a time, one __syncthreads per frame.  The gradient
//   dL/dlogit[t][c] = softmax[t][c] - exp(logsumexp_{s: ext[s]=c}(alpha+beta)[t] + nll - logprob[t][c])
// (log_softmax's backward is the identity here because that expression sums to zero over c) is formed by one
// wave per frame with LDS float atomics into the <= 128 class bins.
#include "common.h"
#include <math.h>
#include <type_traits>

#define CTC_CHUNK 64
#define CTC_MAXV 128
#define NEG_INF (-INFINITY)

// The recursion is a 512-step serial chain, so the two helpers use the hardware exp2 / log2 (v_exp_f32 / v_log_f32,
// ~1 ulp): an absolute error of ~1e-7 per step in the log domain, against per-utterance losses of O(100).
__device__ __forceinline__ float lse2(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == NEG_INF) return NEG_INF;
    return m + __logf(__expf(a - m) + __expf(b - m));
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
    const float m = fmaxf(fmaxf(a, b), c);
    if (m == NEG_INF) return NEG_INF;
    return m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
}

// lse[b][t] = logsumexp_c logits[b][t][c]
__global__ void ctc_lse_kernel(const float* __restrict__ logits, float* __restrict__ lse, long rows, int V, int* __restrict__ stall, int B) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < B) stall[r] = 0;               // sticky "a pipeline wait ran into its bound" flags of the lattice kernel (read by grad / mean)
    if (r >= rows) return;
    const float* p = logits + r * V;
    float m = NEG_INF;
    for (int c = 0; c < V; ++c) m = fmaxf(m, p[c]);
    float s = 0.f;
    for (int c = 0; c < V; ++c) s += expf(p[c] - m);
    lse[r] = m + logf(s);
}

// grid (B, 2): y = 0 alpha, y = 1 beta.  lattice[b][t][s] written for t < in_len[b], s < 2*tgt_len[b]+1.
// NS = lattice states per thread: 256 * NS >= 2 * Lmax + 1 (8 / 16 cover transcripts of up to 1023 / 2047 tokens -- nn.CTCLoss itself
// has no limit, asr.py:105; up to 1024 states, i.e. 511 tokens, take ctc_lattice_skew_kernel below).
template <int NS>
__global__ __launch_bounds__(256) void ctc_lattice_kernel(const float* __restrict__ logits, const float* __restrict__ lse,
                                                          const long long* __restrict__ targets, const int* __restrict__ in_len,
                                                          const int* __restrict__ tgt_len, float* __restrict__ alpha,
                                                          float* __restrict__ beta, float* __restrict__ nll, int T, int V, int Lmax,
                                                          int Smax, int blank) {
    extern __shared__ float sm[];
    float* lp = sm;                                  // [CTC_CHUNK][V] log-probs of the current chunk
    float* row = sm + CTC_CHUNK * V;                 // [2][Smax + 4] previous / current lattice row (with guard cells)
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    int Tb = in_len[b];
    if (Tb > T) Tb = T;
    int L = tgt_len[b];
    if (L > Lmax) L = Lmax;
    const int S = 2 * L + 1;
    float* lat = (dir == 0 ? alpha : beta) + (size_t)b * T * Smax;
    const long long* tg = targets + (size_t)b * Lmax;
    const int rs = Smax + 4;
    // guard cells (index 0,1 and S+2,S+3 of the padded row) stay -inf
    for (int i = tid; i < 2 * rs; i += 256) row[i] = NEG_INF;
    __syncthreads();
    // no frame: only an empty transcript has an alignment (the empty one, probability 1), as in nn.CTCLoss
    if (Tb <= 0) { if (dir == 0 && tid == 0) nll[b] = L <= 0 ? 0.f : INFINITY; return; }

    // states handled by this thread: s = tid, tid + 256, ... ; class and skip permission per state
    int cls[NS]; bool skip[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int s = tid + 256 * k;
        cls[k] = blank; skip[k] = false;
        if (s < S && (s & 1)) {
            cls[k] = (int)tg[s >> 1];
            if (dir == 0) skip[k] = s >= 2 && tg[s >> 1] != tg[(s >> 1) - 1];
            else skip[k] = s + 2 < S && tg[s >> 1] != tg[(s >> 1) + 1];
        }
        if (cls[k] < 0 || cls[k] >= V) cls[k] = blank;
    }

    const int nchunks = (Tb + CTC_CHUNK - 1) / CTC_CHUNK;
    for (int ci = 0; ci < nchunks; ++ci) {
        const int c0 = dir == 0 ? ci * CTC_CHUNK : (nchunks - 1 - ci) * CTC_CHUNK;     // first frame of the chunk
        const int cn = min(CTC_CHUNK, Tb - c0);
        __syncthreads();
        for (int i = tid; i < cn * V; i += 256) {
            const int tt = i / V, c = i - tt * V;
            lp[i] = logits[((size_t)b * T + c0 + tt) * V + c] - lse[(size_t)b * T + c0 + tt];
        }
        __syncthreads();
        for (int j = 0; j < cn; ++j) {
            const int tl = dir == 0 ? j : cn - 1 - j;
            const int t = c0 + tl;
            const bool first = dir == 0 ? (t == 0) : (t == Tb - 1);
            const int cur = t & 1, prv = cur ^ 1;
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const int s = tid + 256 * k;
                if (s < S) {
                    const float e = lp[tl * V + cls[k]];
                    float v;
                    if (first) {
                        const bool start = dir == 0 ? (s <= 1) : (s >= S - 2);
                        v = start ? e : NEG_INF;
                    } else if (dir == 0) {
                        const float* pr = row + prv * rs + 2 + s;
                        v = e + lse3(pr[0], pr[-1], skip[k] ? pr[-2] : NEG_INF);
                    } else {
                        const float* pr = row + prv * rs + 2 + s;
                        v = e + lse3(pr[0], pr[1], skip[k] ? pr[2] : NEG_INF);
                    }
                    row[cur * rs + 2 + s] = v;
                    lat[(size_t)t * Smax + s] = v;
                }
            }
            __syncthreads();
        }
    }
    if (dir == 0 && tid == 0) {
        const float* last = row + ((Tb - 1) & 1) * rs + 2;
        const float ll = S >= 2 ? lse2(last[S - 1], last[S - 2]) : last[S - 1];
        nll[b] = -ll;
    }
}

// ---------------------------------------------------------------------------------------------
// The same lattice as a WAVE PIPELINE (2 * Lmax + 1 <= 1024 states).  The kernel above pays, on every one of the T dependent
// frames, an LDS write -> barrier -> LDS read round trip of the whole row across 4 waves (~0.33 us per frame: 170 us at
// T' = 512).  Here a lane owns ONE state in direction order (u = s for alpha, u = S-1-s for beta, so both recursions read
// u, u-1, u-2), keeps it in a register and gets its neighbours by DPP (wave_shr:1); only the state at a wave's upper edge
// goes through LDS, into a ring slot per frame, and the waves run SKEWED: wave w may start frame q as soon as wave w-1 has
// published frame q-1 (a progress word per wave; no workgroup barrier in the recursion).  Emission log-probabilities are
// gathered straight from global memory eight frames ahead.
// (Round 5, measured at B = 32, T' = 512, 100-token targets, whole head 134 us: timing-only ablations put 62 us on the
//  handshake, 37 us on the four transcendentals per frame, 10-12 us each on the lattice store and the emission gathers; the same
//  pipeline in LOCKSTEP -- fixed skew of two frames, one s_barrier per frame, no progress words -- was built and measured SLOWER,
//  143 us: a four-wave s_barrier costs more per frame (~75 ns) than the polling it replaces.  DESIGN.md section 8.)
// log2-domain log-sum-exp of three terms on the raw v_exp_f32 / v_log_f32 (no range scaling: the sum lies in [1, 3] or is exactly
// 0), branch-free: an all -inf input gives mm + log2(0) = -inf, never inf - inf
__device__ __forceinline__ float ctc_lse3_log2(float a, float b, float c) {
    const float mm = fmaxf(fmaxf(fmaxf(a, b), c), -1e30f);
    const float sum = __builtin_amdgcn_exp2f(a - mm) + __builtin_amdgcn_exp2f(b - mm) + __builtin_amdgcn_exp2f(c - mm);
    return mm + __builtin_amdgcn_logf(sum);
}
#define CTC_RING 32
#define CTC_SPIN_MAX (1 << 20)      /* a wave never waits forever on a neighbour (all waves of a workgroup are resident: this bound is never reached) */
#define CTC_PF 8
// GROUPED hand-over (G > 0 below).  The handshake above is paid on every frame: a progress test, a speculative progress load and edge
// load, a one-lane store and a one-lane publish under two exec masks, a back-pressure test -- more instructions on the per-frame
// chain than the recursion itself (two DPP moves, one ctc_lse3_log2, a select, a store).  In the grouped form the unit of exchange
// between neighbouring waves is a group of G frames, the group in which emissions are prefetched: per group a wave waits ONCE for
// its upstream wave's group, reads the G edge values with wide LDS reads, runs G frames of pure recursion (no LDS traffic, no
// polling, no exec-mask change) and hands its own G edge values down with one store and one publish.  Wave w then runs one GROUP
// behind wave w-1: the pipeline fills in (waves - 1) * G frames instead of (waves - 1), which short inputs on many waves do not earn
// back -- ctc_lattice_grouped() below is the host's rule.  Every state of every frame sees the same DPP neighbours, the same
// ctc_lse3_log2, the same emission and the same store in both forms: they agree bit for bit (tests/test_gpu_ctc_group.py).
// Only ONE edge value crosses a wave boundary in either form: lane 0 of a wave (u = 64 w, even) holds a blank in both directions, a
// blank has no skip transition, so its u-2 neighbour is never consumed; lane 1's u-2 is lane 0's u-1, which the first DPP delivers.
#ifndef CTC_GROUP
#define CTC_GROUP 16                /* 4 and 8 were built and measured: DESIGN_rejected.md, profiles/ctc_group_ab.txt */
#endif
#define CTC_GRING 8                 /* groups per ring */
static_assert(CTC_GROUP % 4 == 0 && CTC_GROUP >= 4 && CTC_GROUP <= 16, "the group's edge values travel as float4");
typedef float ctc_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float ctc_wave_shr1(float fill, float v) {       // lane l gets v of lane l-1; lane 0 gets `fill`
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}

// G = 0: the per-frame hand-over, emissions prefetched CTC_PF frames ahead; G > 0: the grouped hand-over, groups (and prefetch) of G frames
template <int G>
__global__ __launch_bounds__(1024) void ctc_lattice_skew_kernel(const float* __restrict__ logits, const float* __restrict__ lse,
                                                                const long long* __restrict__ targets, const int* __restrict__ in_len,
                                                                const int* __restrict__ tgt_len, float* __restrict__ alpha,
                                                                float* __restrict__ beta, float* __restrict__ nll, int T, int V, int Lmax,
                                                                int Smax, int blank, int* __restrict__ stall) {
    constexpr int PF = G > 0 ? G : CTC_PF;                                  // frames per prefetch group
    // per upstream wave a ring of the top state's values: one slot per frame, or one slot of G frames per group
    __shared__ __attribute__((aligned(16))) float bnd[16][G > 0 ? CTC_GRING * G : CTC_RING];
    __shared__ int progress[16];
    __shared__ float fin[2];
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, NW = blockDim.x >> 6;
    int Tb = in_len[b];
    if (Tb > T) Tb = T;
    int L = tgt_len[b];
    if (L > Lmax) L = Lmax;
    const int S = 2 * L + 1;
    float* lat = (dir == 0 ? alpha : beta) + (size_t)b * T * Smax;
    const long long* tg = targets + (size_t)b * Lmax;
    if (lane == 0) progress[w] = -1;
    if (tid < 2) fin[tid] = NEG_INF;
    __syncthreads();
    // no frame: only an empty transcript has an alignment (the empty one, probability 1), as in nn.CTCLoss
    if (Tb <= 0) { if (dir == 0 && tid == 0) nll[b] = L <= 0 ? 0.f : INFINITY; return; }

    const int u = tid;                                   // state in direction order
    const int sidx = dir == 0 ? u : S - 1 - u;           // lattice state
    const bool active = u < S;
    int cls = blank;
    bool skip = false;
    if (active && (sidx & 1)) {
        cls = (int)tg[sidx >> 1];
        if (dir == 0) skip = sidx >= 2 && tg[sidx >> 1] != tg[(sidx >> 1) - 1];
        else skip = sidx + 2 < S && tg[sidx >> 1] != tg[(sidx >> 1) + 1];
    }
    if (cls < 0 || cls >= V) cls = blank;

    // frame q of the recursion is time t = q (alpha) / Tb-1-q (beta); emissions of frames q0+8 .. q0+15 are in flight while q0 .. q0+7 compute
    const float* lg = logits + (size_t)b * T * V + cls;
    const float* ls = lse + (size_t)b * T;
    auto emission = [&](int q) -> float {
        const int qq = q < Tb ? q : Tb - 1;
        const int t = dir == 0 ? qq : Tb - 1 - qq;
        return (lg[(size_t)t * V] - ls[t]) * 1.44269504088896340736f;       // log2 units: the recursion runs on exp2 / log2 directly
    };
    // a group's emissions become opaque where the group starts to use them (not where they are loaded: that would wait for the
    // loads on the spot): a rounded product in every frame of both forms, never contracted into the frame's add
    auto settle = [](float (&e)[PF]) {
#pragma unroll
        for (int j = 0; j < PF; ++j) asm volatile("" : "+v"(e[j]));
    };
    float cur[PF], nxt[PF];
#pragma unroll
    for (int j = 0; j < PF; ++j) cur[j] = emission(j);
    settle(cur);

    // relaxed workgroup-scope atomics: plain ds_read / ds_write that the compiler neither caches nor fences (a `volatile` access
    // is bracketed by vmcnt(0) waits, i.e. by the acknowledgement of the previous frame's lattice store: 240 us instead of 170).
    // LDS executes one wave's operations in order, so "edge values, then progress word" needs no fence -- only program order.
    auto prog_load = [&](int i) { return __hip_atomic_load(&progress[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    float a_prev = NEG_INF;
    // lattice row pointer of frame q, advanced by one row per frame (alpha walks up, beta down)
    float* lrow = lat + (size_t)(dir == 0 ? 0 : Tb - 1) * Smax + sidx;
    const long lstep = dir == 0 ? (long)Smax : -(long)Smax;
    // the recursion of one frame (not the first); edge: the upstream wave's top state of the previous frame (lane 0's u-1)
    auto step = [&](float edge, float e) {
        const float sm1 = ctc_wave_shr1(edge, a_prev);
        const float sm2 = ctc_wave_shr1(NEG_INF, sm1);      // lane 0's u-2 is never consumed: see above
        const float v = e + ctc_lse3_log2(a_prev, sm1, skip ? sm2 : NEG_INF);
        return active ? v : NEG_INF;
    };
    int pnext = -2;
    float n63 = NEG_INF;
    // PER-FRAME form, one frame; UP: there is an upstream wave (w > 0), DOWN: a downstream wave (w < NW - 1), FIRST: q == 0.  The roles
    // are fixed per wave, so the loop below is instantiated per role instead of testing them on every frame.
    auto frame = [&](auto up_t, auto down_t, auto first_t, int q, float e) {
        constexpr bool UP = decltype(up_t)::value, DOWN = decltype(down_t)::value, FIRST = decltype(first_t)::value;
        float v63 = NEG_INF;
        if constexpr (UP) {
            if constexpr (!FIRST) {
                // (the progress word travels as an opaque VGPR until here: as a plain uniform value hipcc moves it to an SGPR --
                //  and waits for the LDS read -- right where it was issued, which puts the read's latency back on the chain)
                asm volatile("" : "+v"(pnext));
                if (__builtin_amdgcn_readfirstlane(pnext) >= q - 1) {    // the copy fetched during the previous frame is valid
                    v63 = n63;
                } else {
                    // wait until the upstream wave is TWO frames ahead (or done): with a skew of one, the speculative fetch
                    // below would find frame q unpublished on every frame and this slow path would run each time
                    const int need = min(q + 1, Tb - 1);
                    int guard = 0;
                    for (; prog_load(w - 1) < need && guard < CTC_SPIN_MAX; ++guard) __builtin_amdgcn_s_sleep(1);
                    if (guard >= CTC_SPIN_MAX && lane == 0) stall[b] = 1;      // never reached by design; if it is, poison the result (no silent wrong loss)
                    asm volatile("" ::: "memory");
                    v63 = bnd[w - 1][(q - 1) & (CTC_RING - 1)];
                }
            }
            // speculative fetch for frame q + 1 (edge value of frame q): progress word FIRST -- if it already says >= q, the slot
            // read after it (LDS keeps a wave's operations in order) is complete; used next frame, so its latency hides here
            pnext = prog_load(w - 1);
            asm volatile("" ::: "memory");
            n63 = bnd[w - 1][q & (CTC_RING - 1)];
        }
        float v;
        if constexpr (FIRST) v = (active && u <= 1) ? e : NEG_INF;
        else v = step(v63, e);
        if constexpr (DOWN) {
            // back-pressure, once per half ring: frames q .. q + RING/2 - 1 reuse the slots of frames q - RING .. q - RING/2 - 1, which
            // wave w+1 has read once it has published frame q - RING/2
            if ((q & (CTC_RING / 2 - 1)) == 0 && q >= CTC_RING / 2) {
                int guard = 0;
                for (; prog_load(w + 1) < q - CTC_RING / 2 && guard < CTC_SPIN_MAX; ++guard) __builtin_amdgcn_s_sleep(1);
                if (guard >= CTC_SPIN_MAX && lane == 0) stall[b] = 1;
            }
            asm volatile("" ::: "memory");
            if (lane == 63) bnd[w][q & (CTC_RING - 1)] = v;
        }
        asm volatile("" ::: "memory");       // program order only: LDS performs one wave's writes in the order they were issued
        if (lane == 0) __hip_atomic_store(&progress[w], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        a_prev = v;
        if (active) *lrow = v * 0.69314718055994530942f;      // the lattice is stored in natural-log units
        lrow += lstep;
    };
    // GROUPED form, one group of G frames starting at q0 = g * G (n of them exist; FULL: n == G and g > 0).  progress[w] is the last
    // GROUP wave w has published (-1: none).  Slot g & (GRING - 1) of wave w's ring holds what wave w+1 needs for ITS group g: wave
    // w's top state of frames q0 - 1 .. q0 + G - 2, i.e. the value it carried into the group and its first G - 1 results (the last
    // result rides in the next group's slot; frame 0 reads no neighbour, so slot 0's first value is never used).
    auto group = [&](auto up_t, auto down_t, auto full_t, int g, int n) {
        constexpr bool UP = decltype(up_t)::value, DOWN = decltype(down_t)::value, FULL = decltype(full_t)::value;
        constexpr int G4 = G / 4;
        ctc_f4 edge[G4 > 0 ? G4 : 1];
        for (int i = 0; i < G4; ++i) edge[i] = ctc_f4{NEG_INF, NEG_INF, NEG_INF, NEG_INF};
        if constexpr (UP) {
            // progress word FIRST, the slot right behind it: if the word already says >= g the slot read after it (LDS keeps a wave's
            // operations in order) is complete, and the wait cost one LDS round trip per group; else spin, then read the slot again
            const ctc_f4* slot = reinterpret_cast<const ctc_f4*>(&bnd[w - 1][(g & (CTC_GRING - 1)) * G]);
            const int p = prog_load(w - 1);
            asm volatile("" ::: "memory");
#pragma unroll
            for (int i = 0; i < G4; ++i) edge[i] = slot[i];
#pragma unroll
            for (int i = 0; i < G4; ++i) asm volatile("" : "+v"(edge[i]));      // issued here, ahead of the test: hipcc otherwise sinks the reads behind it
            if (__builtin_amdgcn_readfirstlane(p) < g) {
                int guard = 0;
                for (; prog_load(w - 1) < g && guard < CTC_SPIN_MAX; ++guard) __builtin_amdgcn_s_sleep(1);
                if (guard >= CTC_SPIN_MAX && lane == 0) stall[b] = 1;      // never reached by design; if it is, poison the result (no silent wrong loss)
                asm volatile("" ::: "memory");
#pragma unroll
                for (int i = 0; i < G4; ++i) edge[i] = slot[i];
            }
        }
        const float* ev = reinterpret_cast<const float*>(edge);
        // G frames of pure recursion: no LDS traffic, no polling, no exec-mask change
        float val[G > 0 ? G : 1];
        const float carried = a_prev;
#pragma unroll
        for (int j = 0; j < G; ++j) {
            val[j] = a_prev;                                   // (a frame past the end repeats the last value: never stored, never consumed)
            if (FULL || j < n) {
                if (!FULL && g == 0 && j == 0) val[j] = (active && u <= 1) ? cur[0] : NEG_INF;
                else val[j] = step(ev[j], cur[j]);
            }
            asm volatile("" : "+v"(val[j]));                   // the frame is computed here, by all lanes: not sunk under the stores' exec mask
            a_prev = val[j];
        }
        if constexpr (DOWN) {
            // back-pressure, once per half ring: groups g .. g + GRING/2 - 1 reuse the slots of groups g - GRING .. g - GRING/2 - 1, which
            // wave w+1 has read (at the start of each of them) once it has published group g - GRING/2
            if ((g & (CTC_GRING / 2 - 1)) == 0 && g >= CTC_GRING / 2) {
                int guard = 0;
                for (; prog_load(w + 1) < g - CTC_GRING / 2 && guard < CTC_SPIN_MAX; ++guard) __builtin_amdgcn_s_sleep(1);
                if (guard >= CTC_SPIN_MAX && lane == 0) stall[b] = 1;
            }
            asm volatile("" ::: "memory");
            if (lane == 63) {
                ctc_f4* slot = reinterpret_cast<ctc_f4*>(&bnd[w][(g & (CTC_GRING - 1)) * G]);
#pragma unroll
                for (int i = 0; i < G4; ++i)
                    slot[i] = ctc_f4{i == 0 ? carried : val[4 * i - 1], val[4 * i], val[4 * i + 1], val[4 * i + 2]};
            }
        }
        if constexpr (UP || DOWN) {
            asm volatile("" ::: "memory");   // program order only: LDS performs one wave's writes in the order they were issued
            if (lane == 0) __hip_atomic_store(&progress[w], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (active) {
#pragma unroll
            for (int j = 0; j < G; ++j)
                if (FULL || j < n) lrow[j * lstep] = val[j] * 0.69314718055994530942f;      // the lattice is stored in natural-log units
        }
        lrow += G * lstep;
    };
    auto run = [&](auto up_t, auto down_t) {
        for (int q0 = 0; q0 < Tb; q0 += PF) {
#pragma unroll
            for (int j = 0; j < PF; ++j) nxt[j] = emission(q0 + PF + j);
            if constexpr (G > 0) {
                if (q0 > 0 && q0 + G <= Tb) group(up_t, down_t, std::true_type{}, q0 / G, G);
                else group(up_t, down_t, std::false_type{}, q0 / G, min(G, Tb - q0));
            } else if (q0 == 0) {
                frame(up_t, down_t, std::true_type{}, 0, cur[0]);
#pragma unroll
                for (int j = 1; j < PF; ++j)
                    if (j < Tb) frame(up_t, down_t, std::false_type{}, j, cur[j]);
            } else if (q0 + PF <= Tb) {
#pragma unroll
                for (int j = 0; j < PF; ++j) frame(up_t, down_t, std::false_type{}, q0 + j, cur[j]);
            } else {
#pragma unroll
                for (int j = 0; j < PF; ++j)
                    if (q0 + j < Tb) frame(up_t, down_t, std::false_type{}, q0 + j, cur[j]);
            }
#pragma unroll
            for (int j = 0; j < PF; ++j) cur[j] = nxt[j];
            settle(cur);
        }
    };
    const bool has_up = w > 0, has_down = w < NW - 1;
    if (has_up && has_down) run(std::true_type{}, std::true_type{});
    else if (has_up) run(std::true_type{}, std::false_type{});
    else if (has_down) run(std::false_type{}, std::true_type{});
    else run(std::false_type{}, std::false_type{});
    if (dir == 0) {
        if (u == S - 1) fin[0] = a_prev;
        if (S >= 2 && u == S - 2) fin[1] = a_prev;
        __syncthreads();
        if (tid == 0) nll[b] = -(S >= 2 ? lse2(fin[0] * 0.69314718055994530942f, fin[1] * 0.69314718055994530942f) : fin[0] * 0.69314718055994530942f);
    }
}

// one wave per (b, t): grad[b][t][c] = softmax - exp(lcab + nll - logprob); zero for padded frames / infeasible utterances
// BVT: the gradient goes out as [B, V, T] -- the layout of the tensor the logits were transposed FROM (asr.py:114), so that transpose's
// backward is a view instead of a launch.  A wave's 29 values are then T floats apart: written by the wave itself they were 4-byte
// stores into lines that seven other XCDs' workgroups fill at the same time (24.6 -> 31.5 us); so a workgroup is NW = 16 consecutive
// frames, the values meet in LDS and each class's 16 frames leave as one 64-byte run.
template <int NW, bool BVT>
__global__ __launch_bounds__(64 * NW) void ctc_grad_kernel(const float* __restrict__ logits, const float* __restrict__ lse,
                                                           const long long* __restrict__ targets, const int* __restrict__ in_len,
                                                           const int* __restrict__ tgt_len, const float* __restrict__ alpha,
                                                           const float* __restrict__ beta, float* nll,
                                                           float* __restrict__ grad, int B, int T, int V, int Lmax, int Smax, int blank,
                                                           int mean_scale, const int* __restrict__ stall, float* __restrict__ loss) {
    __shared__ float bins[2 * NW][CTC_MAXV];       // [0, NW): per-wave class sums; [NW, 2 NW): per-wave class references (as unsigned)
    __shared__ float stage[BVT ? NW : 1][BVT ? CTC_MAXV : 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * NW + wave;
    if (loss && blockIdx.x == 0 && wave == 0) {
        // loss = mean_b( finite(nll_b) ? nll_b / max(len_b, 1) : 0 )   (reduction='mean', zero_infinity=True: only +-inf is zeroed,
        // a NaN -- or a lattice whose pipeline wait hit its bound -- stays visible)
        float s = 0.f;
        for (int bb = lane; bb < B; bb += 64) {
            const float v = stall[bb] ? __builtin_nanf("") : nll[bb];
            if (!(v == INFINITY || v == -INFINITY)) s += v / (float)max(tgt_len[bb], 1);
        }
        s = wave_sum(s);
        if (lane == 0) loss[0] = s / (float)B;
    }
    const auto frame = [&]() {
    const int b = (int)(w / T), t = (int)(w % T);
    float* g = BVT ? &stage[wave][0] : grad + ((size_t)b * T + t) * V;
    if (stall[b]) {                                   // see ctc_lattice_skew_kernel: poison instead of a silently wrong result
        for (int c = lane; c < V; c += 64) g[c] = __builtin_nanf("");
        if (t == 0 && lane == 0) nll[b] = __builtin_nanf("");
        return;
    }
    const float n = nll[b];
    int Tb = in_len[b];
    if (Tb > T) Tb = T;
    if (t >= Tb || !(n < INFINITY)) {                 // padded frame, or zero_infinity
        for (int c = lane; c < V; c += 64) g[c] = 0.f;
        return;
    }
    int L = tgt_len[b];
    if (L > Lmax) L = Lmax;
    const int S = 2 * L + 1;
    const float* al = alpha + ((size_t)b * T + t) * Smax;
    const float* be = beta + ((size_t)b * T + t) * Smax;
    const long long* tg = targets + (size_t)b * Lmax;
    // Per-CLASS normalisation (round 6).  The sums of exp(alpha + beta) were taken relative to the frame's largest alpha + beta over
    // ALL states; a class whose log-probability sits more than ~87 nats below the frame's best class then underflowed to an occupancy
    // of exactly 0 although the lattice forces it (found with a transcript whose label has logit -400: the loss was right, that label's
    // gradient 100 % wrong; a diverged model -- the benchmark's own after ~40 steps on noise -- is in that regime at every frame).
    // Now each class has its own reference: dmin[c] = min over its states of (m - (alpha + beta)) (non-negative floats order like their
    // bit patterns: an LDS atomicMin on unsigned), the sums are relative to it, and it goes back into the exponent.
    unsigned* dmin = reinterpret_cast<unsigned*>(&bins[NW + wave][0]);
    for (int c = lane; c < V; c += 64) { bins[wave][c] = 0.f; dmin[c] = 0x7f800000u; }
    float m = NEG_INF;
    for (int s = lane; s < S; s += 64) m = fmaxf(m, al[s] + be[s]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");       // wave-local LDS hand-off between lanes: keep program order for the compiler too
    if (m > NEG_INF) {
        for (int s = lane; s < S; s += 64) {
            int c = (s & 1) ? (int)tg[s >> 1] : blank;
            if (c < 0 || c >= V) c = blank;
            const float d = m - (al[s] + be[s]);                 // >= 0 (+inf for an unreachable state; NaN is left out: it reaches the sum below)
            if (d >= 0.f) atomicMin(&dmin[c], __builtin_bit_cast(unsigned, d));
        }
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
        for (int s = lane; s < S; s += 64) {
            int c = (s & 1) ? (int)tg[s >> 1] : blank;
            if (c < 0 || c >= V) c = blank;
            const float dm = __builtin_bit_cast(float, dmin[c]);
            const float x = al[s] + be[s];
            if (dm < INFINITY || x != x) atomicAdd(&bins[wave][c], expf((x - m) + dm));      // exp(x - (m - dm)) <= 1
        }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");       // wave-local LDS hand-off between lanes: keep program order for the compiler too
    const float z = lse[(size_t)b * T + t];
    const float* lg = logits + ((size_t)b * T + t) * V;
    // mean_scale: gradient of CTCLoss(reduction='mean') = mean_b(nll_b / max(len_b, 1)) instead of nll_b
    const float gs = mean_scale ? 1.f / ((float)max(tgt_len[b], 1) * (float)B) : 1.f;
    for (int c = lane; c < V; c += 64) {
        const float lpc = lg[c] - z;
        const float acc = bins[wave][c];
        const float dm = __builtin_bit_cast(float, dmin[c]);
        // log occupancy = (m - dm) + log(acc) + n - lpc, summed so that the two large terms (m - dm ~ -n + lpc) meet first
        const float occ = (acc > 0.f) ? expf(((m - dm) + n - lpc) + logf(acc)) : (acc != acc ? acc : 0.f);
        g[c] = (expf(lpc) - occ) * gs;
    }
    };
    if (w < (long)B * T) frame();
    if constexpr (BVT) {
        __syncthreads();
        const long w0 = (long)blockIdx.x * NW;
        for (int i = threadIdx.x; i < V * NW; i += 64 * NW) {
            const int c = i / NW, j = i % NW;               // frame fastest: NW consecutive lanes write NW consecutive t of one class
            const long wj = w0 + j;
            if (wj < (long)B * T) grad[((size_t)(wj / T) * V + c) * T + (wj % T)] = stage[j][c];
        }
    }
}

extern "C" int v100_ctc_workspace_floats(int B, int T, int Lmax) {      // alpha + beta + lse + stall flags
    const long n = 2L * B * T * (2 * Lmax + 1) + (long)B * T + B;
    return n > 0x7fffffffL ? -1 : (int)n;
}

// Which hand-over the wave pipeline runs (host rule).  The grouped form saves time on every frame and pays a longer pipeline fill, a
// group instead of a frame per downstream wave, so it runs from a padded length T on that grows with the wave count nw:
// T >= 32 + 4 nw.  Measured, not derived: tools/micro/ctc_group_sweep.py times both forms over T x waves (profiles/
// ctc_group_ab.txt: with groups of 16 the grouped form wins from T = 32 / 32 / 32 / 48 / 96 on 1 / 2 / 4 / 8 / 16 waves, the rule
// asks for 36 / 40 / 48 / 64 / 96; around those lengths the two are within 1 - 2 us of each other, further down the per-frame form
// wins by up to 9 us).  Rows whose in_len is shorter than T finish early in either form.
static int ctc_lattice_form = -1;       // test hook: -1 the rule, 0 per frame, 1 grouped
static bool ctc_lattice_rule(int T, int nw) { return T >= 32 + 4 * nw; }
static bool ctc_lattice_grouped(int T, int nw) { return ctc_lattice_form >= 0 ? ctc_lattice_form != 0 : ctc_lattice_rule(T, nw); }

// Test hook: force the wave pipeline's hand-over process-wide: 0 per frame, 1 grouped, -1 back to the rule.
extern "C" int v100_ctc_lattice_form(int form) {
    if (form < -1 || form > 1) return V100_ERR_SHAPE;
    ctc_lattice_form = form;
    return V100_OK;
}

// Host only (no GPU call): what ctc_run launches for the lattice at this shape, whatever the hook says: -1 the barrier kernels
// (more than 1024 states), 0 the pipeline with the per-frame hand-over, else the pipeline with groups of that many frames.
extern "C" int v100_ctc_lattice_plan(int T, int Lmax) {
    const int Smax = 2 * Lmax + 1;
    if (T <= 0 || Lmax < 0 || Smax > 1024) return -1;
    return ctc_lattice_rule(T, (Smax + 63) / 64) ? CTC_GROUP : 0;
}

// Frames a wave of the grouped pipeline can run ahead of its downstream wave: the ring's capacity.
extern "C" int v100_ctc_lattice_ring_frames(void) { return CTC_GRING * CTC_GROUP; }

static int ctc_run(const float* logits, const long long* targets, const int* in_len, const int* tgt_len, float* workspace, float* nll,
                   float* loss, float* grad, int grad_bvt, int B, int T, int V, int Lmax, int blank, void* stream);

extern "C" int v100_ctc_loss(const float* logits, const long long* targets, const int* in_len, const int* tgt_len, float* workspace,
                             float* nll, float* grad, int B, int T, int V, int Lmax, int blank, void* stream) {
    return ctc_run(logits, targets, in_len, tgt_len, workspace, nll, nullptr, grad, 0, B, T, V, Lmax, blank, stream);
}

// The same plus the reduction of nn.CTCLoss(reduction='mean', zero_infinity=True): loss[0] = mean_b(nll_b / max(len_b, 1)) over
// the feasible utterances, grad = d loss / d logits (asr.py:105, 152) -- no host-side elementwise kernels around the call.
extern "C" int v100_ctc_loss_mean(const float* logits, const long long* targets, const int* in_len, const int* tgt_len, float* workspace,
                                  float* nll, float* loss, float* grad, int B, int T, int V, int Lmax, int blank, void* stream) {
    if (!loss) return V100_ERR_NULL;
    return ctc_run(logits, targets, in_len, tgt_len, workspace, nll, loss, grad, 0, B, T, V, Lmax, blank, stream);
}

// ... with the gradient written as [B, V, T] when grad_bvt != 0 (logits stay [B, T, V]): for a caller whose logits are the transpose of
// a [B, V, T] tensor (asr.py:114) the backward of that transpose is then a view of this buffer.
extern "C" int v100_ctc_loss_mean_t(const float* logits, const long long* targets, const int* in_len, const int* tgt_len,
                                    float* workspace, float* nll, float* loss, float* grad, int grad_bvt, int B, int T, int V, int Lmax,
                                    int blank, void* stream) {
    if (!loss) return V100_ERR_NULL;
    return ctc_run(logits, targets, in_len, tgt_len, workspace, nll, loss, grad, grad_bvt ? 1 : 0, B, T, V, Lmax, blank, stream);
}

static int ctc_run(const float* logits, const long long* targets, const int* in_len, const int* tgt_len, float* workspace, float* nll,
                   float* loss, float* grad, int grad_bvt, int B, int T, int V, int Lmax, int blank, void* stream) {
    if (!logits || !targets || !in_len || !tgt_len || !workspace || !nll || !grad) return V100_ERR_NULL;
    if (B <= 0 || T <= 0 || V <= 0 || V > CTC_MAXV || Lmax < 0 || 2 * Lmax + 1 > 4096 || blank < 0 || blank >= V) return V100_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int Smax = 2 * Lmax + 1;
    float* alpha = workspace;
    float* beta = alpha + (size_t)B * T * Smax;
    float* lse = beta + (size_t)B * T * Smax;
    const long rows = (long)B * T;
    int* stall = (int*)(lse + (size_t)B * T);
    const size_t shmem = (size_t)(CTC_CHUNK * V + 2 * (Smax + 4)) * sizeof(float);
    // above 64 KiB of dynamic LDS (V = 128 with Lmax 2046 / 2047 only) the launch has to be granted first; a device that refuses
    // ends the call here, before anything is launched, instead of failing the lattice launch and running the gradient on garbage
    if (Smax > 2048 && shmem > 65536 &&
        hipFuncSetAttribute((const void*)ctc_lattice_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem) != hipSuccess) {
        (void)hipGetLastError();
        return V100_ERR_LAUNCH;
    }
    V100_GGL(ctc_lse_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, logits, lse, rows, V, stall, B);
#define CTC_LATTICE(NS_)                                                                                                          \
    V100_GGL(ctc_lattice_kernel<NS_>, dim3(B, 2), dim3(256), shmem, st, logits, lse, targets, in_len, tgt_len, alpha, beta, \
                       nll, T, V, Lmax, Smax, blank)
    if (Smax <= 1024) {
        const int nw = (Smax + 63) / 64;
        if (ctc_lattice_grouped(T, nw))
            V100_GGL(ctc_lattice_skew_kernel<CTC_GROUP>, dim3(B, 2), dim3(64 * nw), 0, st, logits, lse, targets, in_len, tgt_len, alpha,
                     beta, nll, T, V, Lmax, Smax, blank, stall);
        else
            V100_GGL(ctc_lattice_skew_kernel<0>, dim3(B, 2), dim3(64 * nw), 0, st, logits, lse, targets, in_len, tgt_len, alpha, beta,
                     nll, T, V, Lmax, Smax, blank, stall);
    } else if (Smax <= 2048) { CTC_LATTICE(8); }
    else { CTC_LATTICE(16); }
#undef CTC_LATTICE
    if (grad_bvt) V100_GGL((ctc_grad_kernel<16, true>), dim3((unsigned)((rows + 15) / 16)), dim3(1024), 0, st, logits, lse, targets, in_len, tgt_len,
                           alpha, beta, nll, grad, B, T, V, Lmax, Smax, blank, loss ? 1 : 0, stall, loss);
    else V100_GGL((ctc_grad_kernel<4, false>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, logits, lse, targets, in_len, tgt_len,
                  alpha, beta, nll, grad, B, T, V, Lmax, Smax, blank, loss ? 1 : 0, stall, loss);     // (the 'mean' reduction rides in block 0)
    return v100_launch_status();
}
