// K19: one accumulation step of the WORLD feature statistics (voice100/calc_stat.py:40-56), the masked first and second moments
// of f0 [B][T], logspc [B][T][S] and codeap [B][T][A] that become audio_stat.pt.  Frame (b, t) is valid iff t < min(f0_len[b], T).
//
//   moments (float64, 4 + 2S + 2A; layout in include/voice100_hip.h) += the batch's sums,
//
// every product and sum in float64 (an fp32 x fp32 product is exact there), both thresholds compared in fp32 (f0 > 30.0f,
// codeap < -0.2f, as torch compares an fp32 tensor with a Python scalar), and an invalid frame never loaded: the loops END at the
// utterance's last valid element, so NaN or Inf in the padding cannot reach a sum.
//
// Launch 1, world_stat_part_kernel: one workgroup of 1024 threads per (utterance b, chunk of F frames), F and the chunk count C
// from (B, T, S) alone (world_stat_plan).  The valid frames of a chunk are ONE contiguous run of frames x S floats whose first
// element is in column 0, so element i of the run is in column i % S.  A thread walks the run with a stride P = m S, a whole
// number of rows: its column never changes and it needs one (sum, sum of squares) pair, whatever S is.  Positions p < P are dealt
// to threads as p = tid, tid + 1024: with S = 25, P = 81 x 25 = 2025 keeps 2025 of 2048 slots busy, S = 257 takes 7 rows (1799),
// S = 513 three (1539), S = 1024 two; m is the row count with the fullest slots, P <= 2048.  Consecutive threads read consecutive
// floats, eight strides in flight.  codeap is the same walk with S = A and the fp32 test on every element, f0 the same with
// S = 1, a test and a count (P <= 512 for both: they are 1 / S of the bytes).  The m slots that share a column are then added in
// LDS by halving: slot row r += row r + ceil(m / 2), then m = ceil(m / 2), until one row is left -- an order fixed by (m, S).
// The workgroup writes its row of 4 + 2S + 2A doubles to partial[b C + chunk]; a chunk with no valid frame writes zeros.
//
// Launch 2, world_stat_sum_kernel: moments[i] += the sum of partial[.][i].  64 threads per entry: thread g adds rows
// [g R, (g + 1) R) in index order, the 64 sums are halved together in LDS as above, one thread adds the total to moments[i].
//
// No floating-point atomics anywhere, and no order that depends on timing: the same inputs give the same bits.  The kernel only
// reads (the partial rows are ~4 / F of the input bytes): its floor is bytes / HBM rate.
#include "common.h"
#include "../../include/voice100_hip.h"

namespace {
constexpr int kThreads = 1024;
constexpr int kSlots = 2048;                // logspc positions per stride (two per thread)
constexpr int kSmallSlots = 512;            // f0 / codeap positions per stride
constexpr int kMaxS = 1024, kMaxA = 8;
constexpr int kMaxParts = 1024;             // chunks wanted per launch while B allows it (4 workgroups per CU)
constexpr int kSumCols = 16, kSumGroups = 64;

struct StatPlan { int F, C, m_ls, m_ca, m_f0; };

// F frames per chunk and C chunks per utterance from (B, T, S) only.  F is at least 32 (a partial row is 16 S bytes against
// 4 F S bytes read: at most an eighth) and at least 8192 / S (eight elements per thread), and otherwise the smallest that keeps
// B C <= kMaxParts.
inline bool world_stat_plan(int B, int T, int S, int A, StatPlan* pl) {
    if (B < 1 || T < 1 || S < 1 || S > kMaxS || A < 1 || A > kMaxA) return false;
    const int per_b = kMaxParts / B;                                   // 0 when B > kMaxParts: one chunk per utterance
    long long F = per_b > 0 ? ((long long)T + per_b - 1) / per_b : T;
    const long long fmin = (8192 + S - 1) / S > 32 ? (8192 + S - 1) / S : 32;
    if (F < fmin) F = fmin;
    if (F > T) F = T;
    pl->F = (int)F;
    pl->C = (int)(((long long)T + F - 1) / F);
    // rows per stride: the m <= min(kSlots / S, F) that fills the most of its ceil(m S / 1024) x 1024 slots (first such m)
    const int mmax = kSlots / S < pl->F ? kSlots / S : pl->F;
    int best = 1;
    long long best_num = 0, best_den = 1;
    for (int m = 1; m <= mmax; ++m) {
        const long long num = (long long)m * S, den = ((num + kThreads - 1) / kThreads) * kThreads;
        if (num * best_den > best_num * den) { best = m; best_num = num; best_den = den; }
    }
    pl->m_ls = best;
    pl->m_ca = kSmallSlots / A < pl->F ? kSmallSlots / A : pl->F;
    pl->m_f0 = kSmallSlots < pl->F ? kSmallSlots : pl->F;
    return true;
}

struct StatParams {
    const float* f0; const int* f0_len; const float* logspc; const float* codeap; double* partial;
    int B, T, S, A, F, C, m_ls, m_ca, m_f0;
};

// MODE 0: every element (logspc).  1: f0 > 30.0f, counted.  2: codeap < -0.2f.  A NaN fails both tests and propagates in mode 0.
template <int MODE>
__device__ __forceinline__ void stat_add(float v, double& s, double& q, double& c) {
    bool take = true;
    if (MODE == 1) take = v > 30.0f;
    if (MODE == 2) take = v < -0.2f;
    if (take) {
        const double d = (double)v;
        s += d;
        q = fma(d, d, q);
        if (MODE == 1) c += 1.0;
    }
}

// x[0, n) is a run of whole rows of S floats, P = m S.  Slot p < P gets the moments of x[p], x[p + P], ... (all in column p % S),
// added in that order.
template <int MODE>
__device__ __forceinline__ void stat_walk(const float* __restrict__ x, long long n, int P, double* ls, double* lq, double* lc) {
    for (int p = threadIdx.x; p < P; p += kThreads) {
        double s = 0.0, q = 0.0, c = 0.0;
        long long i = p;
        for (; i + 7LL * P < n; i += 8LL * P) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = x[i + (long long)u * P];
#pragma unroll
            for (int u = 0; u < 8; ++u) stat_add<MODE>(v[u], s, q, c);
        }
        for (; i < n; i += P) stat_add<MODE>(x[i], s, q, c);
        ls[p] = s;
        lq[p] = q;
        if (MODE == 1) lc[p] = c;
    }
}

// one halving step over m rows of S slots: row r += row r + ceil(m / 2) for r < floor(m / 2); S (m - half) <= P / 2 <= 1024 threads
__device__ __forceinline__ int stat_halve(double* a, double* b, double* c, int S, int m) {
    if (m > 1) {
        const int half = (m + 1) >> 1, tid = threadIdx.x;
        if (tid < S * (m - half)) {
            a[tid] += a[tid + half * S];
            b[tid] += b[tid + half * S];
            if (c) c[tid] += c[tid + half * S];
        }
        return half;
    }
    return m;
}

__global__ __launch_bounds__(kThreads) void world_stat_part_kernel(StatParams p) {
    __shared__ double ls_s[kSlots], ls_q[kSlots];
    __shared__ double ca_s[kSmallSlots], ca_q[kSmallSlots];
    __shared__ double f0_s[kSmallSlots], f0_q[kSmallSlots], f0_c[kSmallSlots];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.C, chunk = blockIdx.x - b * p.C;
    const int S = p.S, A = p.A, W = 4 + 2 * S + 2 * A;
    double* out = p.partial + (size_t)blockIdx.x * W;

    int len = p.f0_len[b];
    len = min(max(len, 0), p.T);
    const long long t0 = (long long)chunk * p.F;
    const int nf = (int)min(max((long long)len - t0, 0LL), (long long)p.F);       // valid frames of this chunk
    if (nf == 0) {
        for (int i = tid; i < W; i += kThreads) out[i] = 0.0;
        return;
    }
    const size_t frame0 = (size_t)b * p.T + (size_t)t0;
    stat_walk<0>(p.logspc + frame0 * S, (long long)nf * S, p.m_ls * S, ls_s, ls_q, nullptr);
    stat_walk<2>(p.codeap + frame0 * A, (long long)nf * A, p.m_ca * A, ca_s, ca_q, nullptr);
    stat_walk<1>(p.f0 + frame0, nf, p.m_f0, f0_s, f0_q, f0_c);
    __syncthreads();
    int m_ls = p.m_ls, m_ca = p.m_ca, m_f0 = p.m_f0;
    while (m_ls > 1 || m_ca > 1 || m_f0 > 1) {                  // the same trip count in every thread
        m_ls = stat_halve(ls_s, ls_q, nullptr, S, m_ls);
        m_ca = stat_halve(ca_s, ca_q, nullptr, A, m_ca);
        m_f0 = stat_halve(f0_s, f0_q, f0_c, 1, m_f0);
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = f0_s[0];
        out[1] = f0_q[0];
        out[2] = f0_c[0];
        out[3] = (double)nf;
    }
    if (tid < S) {
        out[4 + tid] = ls_s[tid];
        out[4 + S + tid] = ls_q[tid];
    }
    if (tid < A) {
        out[4 + 2 * S + tid] = ca_s[tid];
        out[4 + 2 * S + A + tid] = ca_q[tid];
    }
}

__global__ __launch_bounds__(kSumCols * kSumGroups) void world_stat_sum_kernel(const double* __restrict__ partial, double* moments,
                                                                               int parts, int W) {
    __shared__ double acc[kSumGroups][kSumCols];
    const int c = threadIdx.x % kSumCols, g = threadIdx.x / kSumCols;
    const int i = blockIdx.x * kSumCols + c;
    const int R = (parts + kSumGroups - 1) / kSumGroups;
    double s = 0.0;
    if (i < W) {
        const long long r1 = min((long long)parts, (long long)(g + 1) * R);
        long long r = (long long)g * R;
        for (; r + 16 <= r1; r += 16) {                         // sixteen loads in flight, added in index order all the same
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = partial[(size_t)(r + u) * W + i];
#pragma unroll
            for (int u = 0; u < 16; ++u) s += v[u];
        }
        for (; r < r1; ++r) s += partial[(size_t)r * W + i];
    }
    acc[g][c] = s;
    __syncthreads();
    for (int h = kSumGroups / 2; h >= 1; h >>= 1) {
        if (g < h) acc[g][c] += acc[g + h][c];
        __syncthreads();
    }
    if (g == 0 && i < W) moments[i] += acc[0][c];
}
}  // namespace

extern "C" int v100_world_stat_parts(int B, int T, int S) {
    StatPlan pl;
    if (!world_stat_plan(B, T, S, 1, &pl)) return -1;
    const long long parts = (long long)B * pl.C;
    return parts > 0x7fffffffLL ? -1 : (int)parts;
}

extern "C" int v100_world_stat_accum(const float* f0, const int* f0_len, const float* logspc, const float* codeap, double* partial,
                                     double* moments, int B, int T, int S, int A, void* stream) {
    if (!f0 || !f0_len || !logspc || !codeap || !partial || !moments) return V100_ERR_NULL;
    StatPlan pl;
    if (!world_stat_plan(B, T, S, A, &pl)) return V100_ERR_SHAPE;
    const long long parts = (long long)B * pl.C;
    if (parts > 0x7fffffffLL) return V100_ERR_SHAPE;
    const int W = 4 + 2 * S + 2 * A;
    StatParams p{f0, f0_len, logspc, codeap, partial, B, T, S, A, pl.F, pl.C, pl.m_ls, pl.m_ca, pl.m_f0};
    V100_GGL(world_stat_part_kernel, dim3((unsigned)parts), dim3(kThreads), 0, (hipStream_t)stream, p);
    V100_GGL(world_stat_sum_kernel, dim3((unsigned)((W + kSumCols - 1) / kSumCols)), dim3(kSumCols * kSumGroups), 0,
             (hipStream_t)stream, partial, moments, (int)parts, W);
    return v100_launch_status();
}
