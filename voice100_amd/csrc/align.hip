// K20: forced alignment in one launch (voice100/align_text.py:39-56 on top of voice100/models/align.py:18-66).
//
//   ctc_align   the banded Viterbi of ctc_best_path_kernel (decode.hip) with everything the alignment file needs as outputs:
//               the path, the labels on it, the per-position durations and the score.  Same band growth, same "no blank -> blank
//               double step" rule, first maximum wins, the same fp32 additions in the same order, the same end rule and clamps:
//               path and score are bit-identical to ctc_best_path_kernel.
//
// One workgroup of 256 threads per utterance.  What differs from decode.hip is where each frame's dependent chain waits:
//   * emissions: the log-probability rows of AL_BLK frames are staged in LDS (coalesced loads of whole rows, issued one block
//     ahead of the recurrence and held in registers across it), so a frame reads logp[t][ext(s)] from LDS instead of waiting on a
//     global gather.  Rows wider than AL_VSTAGE are not staged: those shapes keep the global gather (STAGED = false);
//   * the per-frame barrier waits for LDS only (the move stores and the prefetch stay in flight across it);
//   * back pointers are one byte per state: the move j = v - arg (0 .. max_move-1), or AL_JUMP0 where the reference's argmax over
//     an all -inf column leaves the pointer at 0 (np.argmax of equal values: the first row, whose beam entry is 0);
//   * traceback: AL_TB frames of moves at a time are staged back into LDS by all threads -- the position falls by at most
//     max_move-1 per frame, so AL_TB frames need a window of (max_move-1)*(AL_TB-1)+1 columns below the current position -- and
//     one thread walks them there; once the position is 0 it stays 0 (the pointer of state 0 is 0), so the rest is filled;
//   * the path stays in LDS (16 bit); durations are run lengths of the non-decreasing path (first/last frame of each run, no
//     atomics), labels and the zero padding are written by all threads.
#include "common.h"
#include <math.h>

#define AL_THREADS 256
#define AL_BLK 16                                       // frames per staged block of emissions
#define AL_NR 8                                         // staged floats per thread and block
#define AL_BUF (AL_NR * AL_THREADS)                     // floats per staging buffer
#define AL_VSTAGE (AL_BUF / AL_BLK)                     // widest row that is staged: 128
#define AL_TB 64                                        // frames per traceback block
#define AL_JUMP0 255                                    // move byte: the pointer is 0, not v - j
#define AL_TMAX 12000
#define AL_SMAX 4096
// LDS-only barrier: LDS traffic of every wave has landed; global loads and stores stay in flight
#define AL_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

static inline int al_pitch(int Smax) { return (Smax + 15) & ~15; }                     // bytes per frame of the move workspace
static inline int al_window_bytes(int max_move) { return AL_TB * ((max_move - 1) * (AL_TB - 1) + 1); }

// MM: max_move as a compile-time constant (3, the reference's default), or 0 = read it from the argument
template <bool STAGED, int MM>
__global__ __launch_bounds__(AL_THREADS) void ctc_align_kernel(const float* __restrict__ logp, const long long* __restrict__ labels,
                                                               const int* __restrict__ in_len, const int* __restrict__ lab_len,
                                                               unsigned char* moves, int* __restrict__ path,
                                                               long long* __restrict__ best_labels, int* __restrict__ align,
                                                               float* __restrict__ score, int T, int V, int Lmax, int SP, int TP, int P,
                                                               int max_move_arg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char al_smem[];
    int* hdr = (int*)al_smem;                           // [4]: the traceback's current position
    int* ext = hdr + 4;                                 // [SP] blank-extended labels
    float* sc = (float*)(ext + SP);                     // [2][SP] scores; later first/end frame of each run
    u16* pl = (u16*)(sc + 2 * SP);                      // [TP] path
    unsigned char* region = (unsigned char*)(pl + TP);  // staged emissions [2][AL_BUF] fp32, later the traceback window
    float* em = (float*)region;
    unsigned char* win = region;

    const int max_move = MM ? MM : max_move_arg;
    const int b = blockIdx.x, tid = threadIdx.x;
    int Tb = in_len ? in_len[b] : T;
    if (Tb > T) Tb = T;
    int L = lab_len ? lab_len[b] : Lmax;
    if (L > Lmax) L = Lmax;
    if (L < 0) L = 0;
    const int n = 2 * L + 1;
    const int Sout = 2 * Lmax + 1;
    const long long* lab = labels + (size_t)b * Lmax;
    const float* lp = logp + (size_t)b * T * V;
    unsigned char* bk = moves + (size_t)b * T * P;
    int* path_b = path + (size_t)b * T;
    long long* best_b = best_labels + (size_t)b * T;
    int* align_b = align + (size_t)b * Sout;

    if (Tb < 1) {                                       // no frame: nothing to align (ctc_best_path_kernel reads uninitialised scores here)
        for (int t = tid; t < T; t += AL_THREADS) { path_b[t] = 0; best_b[t] = 0; }
        for (int s = tid; s < Sout; s += AL_THREADS) align_b[s] = 0;
        if (tid == 0) score[b] = -INFINITY;
        return;
    }

    auto extg = [&](int v) -> int { return (v < n && (v & 1)) ? (int)lab[v >> 1] : 0; };
    auto col = [&](int e) -> int { return min(max(e, 0), V - 1); };      // a label outside the vocabulary must not index outside the row
    for (int v = tid; v < SP; v += AL_THREADS) ext[v] = extg(v);
    const int e0 = extg(tid), e1 = extg(tid + AL_THREADS);               // the labels of this thread's first two states stay in registers
    const int nblk = (Tb + AL_BLK - 1) / AL_BLK;
    if (STAGED) {
        const int cnt = min(AL_BLK, Tb) * V;
        for (int idx = tid; idx < cnt; idx += AL_THREADS) em[idx] = lp[idx];
    }
    __syncthreads();
    // frame 0: positions 0 and 1 are live (align.py:30)
    int width = n < 2 ? n : 2;
    for (int v = tid; v < SP; v += AL_THREADS) sc[v] = (v < width) ? (STAGED ? em[col(ext[v])] : lp[col(ext[v])]) : -INFINITY;
    __syncthreads();

    for (int k = 0; k < nblk; ++k) {
        float r[AL_NR];
        int cntn = 0;
        if (STAGED && k + 1 < nblk) {                   // the next block's rows: issued here, written to LDS after this block's frames
            const int f0 = (k + 1) * AL_BLK;
            cntn = (min(Tb, f0 + AL_BLK) - f0) * V;
            const float* src = lp + (size_t)f0 * V;
#pragma unroll
            for (int q = 0; q < AL_NR; ++q) {
                const int idx = tid + q * AL_THREADS;
                r[q] = idx < cntn ? src[idx] : 0.0f;
            }
        }
        const float* emk = em + (k & 1) * AL_BUF;
        const int i1 = min(Tb, (k + 1) * AL_BLK);
        for (int i = max(1, k * AL_BLK); i < i1; ++i) {
            const float* cur = sc + ((i - 1) & 1) * SP;
            float* nxt = sc + (i & 1) * SP;
            const int nwidth = min(width + max_move - 1, n);
            const float* emi = STAGED ? emk + (i - k * AL_BLK) * V : lp + (size_t)i * V;
            unsigned char* bki = bk + (size_t)i * P;
            auto step = [&](int v, int e) {
                const float emit = emi[col(e)];
                float best = -INFINITY;
                int arg = 0;
                bool first = true;
#pragma unroll
                for (int j = 0; j < max_move; ++j) {
                    const int kk = v - j;
                    const float c = cur[max(kk, 0)];                     // unconditional: the max_move reads are independent
                    float cand = -INFINITY;
                    int src = 0;
                    if (kk >= 0 && kk < width) {
                        cand = c + emit;
                        if (j > 0 && (j & 1) == 0 && e == 0) cand = -INFINITY;          // no blank -> blank jump
                        src = kk;
                    }
                    if (first || cand > best) { best = cand; arg = src; first = false; }   // np.argmax: first maximum
                }
                nxt[v] = best;
                const int d = v - arg;
                bki[v] = (unsigned char)(d < max_move ? d : AL_JUMP0);
            };
            if constexpr (MM > 0) {
                // the thread's first two states together: every LDS read of both is issued before either is used (indices clamped
                // into the score row, results discarded where the candidate is not live), so a frame costs one LDS round trip
                float ca[MM], cb[MM];
                const int va = tid, vb = tid + AL_THREADS;
                const float ema = emi[col(e0)], emb = emi[col(e1)];
#pragma unroll
                for (int j = 0; j < MM; ++j) {
                    ca[j] = cur[min(max(va - j, 0), SP - 1)];
                    cb[j] = cur[min(max(vb - j, 0), SP - 1)];
                }
                auto pick = [&](int v, int e, float emit, const float* c) {
                    float best = -INFINITY;
                    int arg = 0;
                    bool first = true;
#pragma unroll
                    for (int j = 0; j < MM; ++j) {
                        const int kk = v - j;
                        const bool live = kk >= 0 && kk < width;
                        float cand = live ? c[j] + emit : -INFINITY;
                        if (live && j > 0 && (j & 1) == 0 && e == 0) cand = -INFINITY;      // no blank -> blank jump
                        const int src = live ? kk : 0;
                        if (first || cand > best) { best = cand; arg = src; first = false; }   // np.argmax: first maximum
                    }
                    if (v < nwidth) {
                        nxt[v] = best;
                        const int d = v - arg;
                        bki[v] = (unsigned char)(d < MM ? d : AL_JUMP0);
                    }
                };
                pick(va, e0, ema, ca);
                pick(vb, e1, emb, cb);
            } else {
                if (tid < nwidth) step(tid, e0);
                if (tid + AL_THREADS < nwidth) step(tid + AL_THREADS, e1);
            }
            for (int v = tid + 2 * AL_THREADS; v < nwidth; v += AL_THREADS) step(v, ext[v]);
            AL_BARRIER();
            width = nwidth;
        }
        if (STAGED && k + 1 < nblk) {
            float* dst = em + ((k + 1) & 1) * AL_BUF;   // last read in block k-1, whose frames all ended in a barrier
#pragma unroll
            for (int q = 0; q < AL_NR; ++q) {
                const int idx = tid + q * AL_THREADS;
                if (idx < cntn) dst[idx] = r[q];
            }
            AL_BARRIER();
        }
    }
    __syncthreads();                                    // every move store has landed
    if (tid == 0) {
        const float* fin = sc + ((Tb - 1) & 1) * SP;
        int j = (width >= 2 && fin[width - 1] > fin[width - 2]) ? n - 1 : n - 2;     // align.py:58 (uses the last two live scores)
        if (j < 0) j = 0;
        if (j >= width) j = width - 1;
        score[b] = fin[j];
        hdr[0] = j;
    }
    __syncthreads();

    // traceback: frames t_hi .. t_lo+1 of one block give the positions at t_hi .. t_lo+1 and leave the one at t_lo for the next
    const int wave = tid >> 6, lane = tid & 63;
    int t_hi = Tb - 1;
    while (t_hi > 0) {
        const int jh = hdr[0];
        if (jh == 0) break;                             // state 0 points at state 0: every earlier frame is 0
        const int t_lo = max(0, t_hi - AL_TB);
        const int rows = t_hi - t_lo;
        const int lo = max(0, jh - (max_move - 1) * (rows - 1));
        const int W = jh - lo + 1;
        for (int rr = wave; rr < rows; rr += AL_THREADS / 64) {
            const unsigned char* src = bk + (size_t)(t_hi - rr) * P + lo;
            for (int c = lane; c < W; c += 64) win[rr * W + c] = src[c];
        }
        __syncthreads();
        if (tid == 0) {
            int j = jh;
            for (int rr = 0; rr < rows; ++rr) {
                pl[t_hi - rr] = (u16)j;
                const int mv = win[rr * W + max(j - lo, 0)];
                j = (j == 0 || mv == AL_JUMP0) ? 0 : j - mv;
            }
            hdr[0] = j;
        }
        __syncthreads();
        t_hi = t_lo;
    }
    {
        const int j = hdr[0];                           // the position at frame t_hi and, when it is 0, at every frame before
        for (int t = tid; t <= t_hi; t += AL_THREADS) pl[t] = (u16)j;
    }
    int* st = (int*)sc;                                 // first frame of the run at each position
    int* en = st + SP;                                  // one past its last frame
    for (int s = tid; s < SP; s += AL_THREADS) { st[s] = 0; en[s] = 0; }
    __syncthreads();
    for (int t = tid; t < T; t += AL_THREADS) {
        int p = 0;
        long long lb = 0;
        if (t < Tb) {
            p = pl[t];
            lb = (p & 1) ? lab[p >> 1] : 0;
            if (t == 0 || pl[t - 1] != p) st[p] = t;                     // the path never decreases: one run per position
            if (t == Tb - 1 || pl[t + 1] != p) en[p] = t + 1;
        }
        path_b[t] = p;
        best_b[t] = lb;
    }
    __syncthreads();
    for (int s = tid; s < Sout; s += AL_THREADS) align_b[s] = (s < n) ? en[s] - st[s] : 0;
}

extern "C" int v100_ctc_align_block(void) { return AL_BLK; }

extern "C" long long v100_ctc_align_workspace_bytes(int B, int T, int Lmax) {
    if (B <= 0 || T <= 0 || T > AL_TMAX || Lmax < 0 || 2 * Lmax + 1 > AL_SMAX) return 0;
    return (long long)B * T * al_pitch(2 * Lmax + 1);
}

template <bool STAGED, int MM>
static int al_launch(size_t shmem, hipStream_t st, int B, const float* logp, const long long* labels, const int* in_len, const int* lab_len,
                     unsigned char* moves, int* path, long long* best_labels, int* align, float* score, int T, int V, int Lmax, int SP, int TP,
                     int P, int max_move) {
    if (shmem > 64 * 1024 &&
        hipFuncSetAttribute((const void*)ctc_align_kernel<STAGED, MM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem) != hipSuccess)
        return V100_ERR_LAUNCH;
    V100_GGL((ctc_align_kernel<STAGED, MM>), dim3(B), dim3(AL_THREADS), shmem, st, logp, labels, in_len, lab_len, moves, path, best_labels,
             align, score, T, V, Lmax, SP, TP, P, max_move);
    return v100_launch_status();
}

extern "C" int v100_ctc_align(const float* logp, const long long* labels, const int* in_len, const int* lab_len, void* moves_ws, int* path,
                              long long* best_labels, int* align, float* score, int B, int T, int V, int Lmax, int max_move, void* stream) {
    if (!logp || !labels || !moves_ws || !path || !best_labels || !align || !score) return V100_ERR_NULL;
    const int Smax = 2 * Lmax + 1;
    if (B <= 0 || T <= 0 || T > AL_TMAX || V <= 0 || Lmax < 0 || Smax > AL_SMAX || max_move < 1 || max_move > 8) return V100_ERR_SHAPE;
    const int SP = (Smax + 3) & ~3, TP = (T + 7) & ~7, P = al_pitch(Smax);
    const bool staged = V <= AL_VSTAGE;
    size_t reg = (size_t)al_window_bytes(max_move);
    if (staged && reg < 2 * AL_BUF * sizeof(float)) reg = 2 * AL_BUF * sizeof(float);
    reg = (reg + 15) & ~(size_t)15;
    const size_t shmem = 16 + (size_t)SP * 4 + (size_t)SP * 8 + (size_t)TP * 2 + reg;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* mv = (unsigned char*)moves_ws;
#define AL_GO(S_, M_) al_launch<S_, M_>(shmem, st, B, logp, labels, in_len, lab_len, mv, path, best_labels, align, score, T, V, Lmax, SP, TP, P, max_move)
    if (staged) return max_move == 3 ? AL_GO(true, 3) : AL_GO(true, 0);
    return max_move == 3 ? AL_GO(false, 3) : AL_GO(false, 0);
#undef AL_GO
}
