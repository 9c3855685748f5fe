// K27: score a batch of synthesised feature tracks against recordings: dynamic time warping (DTW) between x [B][Tx][D] (the
// hypothesis) and y [B][Ty][D] (the reference), and the sums along the warping path from which mel-cepstral distortion, F0 RMSE
// and the voiced/unvoiced error rate follow.
//
//   d(i,j) = sqrt(sum_{k >= skip} (x[i][k] - y[j][k])^2)
//   C(0,0) = d(0,0),  C(i,j) = d(i,j) + min(C(i-1,j-1), C(i-1,j), C(i,j-1))   (absent predecessors left out; a tie goes to the
//   first of the three in that order),  cost = C(n-1,m-1),  path = the backtrace from (n-1,m-1), reported forwards.
//
// Two launches per call:
//   1. dtw_dist_kernel, over the whole chip: 64 x 64 tiles of d in fp32, from DIFFERENCES (sub, fma; never |x|^2 + |y|^2 - 2xy),
//      the root taken in fp64 and rounded once, so that a perfect square gives its exact root.  Only cells inside both lengths are
//      computed, and nothing beyond a row's length is read.
//   2. dtw_path_kernel, one wave of 64 lanes per pair, three phases:
//      a. the recurrence as a systolic array (the scheme of K23's ed_systolic): lane l owns the strip of S reference columns
//         l*S .. l*S+S-1 (row C(i-1,.) of the strip in fp64 registers, S a compile-time 1, 2, 4, ... 64: the smallest with
//         64 S >= m), at step s it computes row i = s - l and takes C(i, l*S-1) from its left neighbour by a DPP wave shift.  The
//         strip's distances of the NEXT step are loaded while this one computes.  Every cell writes a 2-bit backpointer (0 =
//         diagonal, 1 = up, 2 = left), min(S, 16) cells to a 32-bit word, rows of 64 * max(S/16, 1) words;
//      b. the backtrace, wave-uniform: the wave holds a tile of 64 rows x 4 backpointer words in registers (lane r: row ti - r) and
//         walks inside it by v_readlane; a new tile is loaded only when the walk leaves the old one, so the dependent global loads
//         are one per some tens of steps and not one per step.  The loop runs at most n + m trips whatever the backpointers hold,
//         and row 0 / column 0 force the move, so a non-finite input can neither hang it nor index out of bounds;
//      c. every 64 path cells the lanes take one cell each: the F0 terms in fp64 and, when the path is wanted, the cell into the
//         reversed-path workspace, which the wave copies forwards at the end.
// mode 1 (identity) pairs frame i with frame i for i < min(n, m): no matrix, no recurrence.
// The cumulative cost and the F0 sums are fp64 throughout.  Plain C++ and vector memory instructions only.
#include "common.h"

#define DTW_TMAX 4096
#define DTW_DUMAX 64
#define DTW_TILE 64

__device__ __forceinline__ int dtw_len(const int* len, int b, int width) {
    return len ? min(max(len[b], 0), width) : width;
}

__global__ __launch_bounds__(256) void dtw_dist_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        const int* __restrict__ x_len, const int* __restrict__ y_len,
                                                        float* __restrict__ dm, int Tx, int Ty, int D, int skip, int pitch) {
    __shared__ float xs[DTW_TILE * (DTW_DUMAX + 1)], ys[DTW_TILE * (DTW_DUMAX + 1)];
    const int b = blockIdx.x, j0 = blockIdx.y * DTW_TILE, i0 = blockIdx.z * DTW_TILE, tid = threadIdx.x;
    const int n = dtw_len(x_len, b, Tx), m = dtw_len(y_len, b, Ty);
    if (i0 >= n || j0 >= m) return;                      // block-uniform
    const int Du = D - skip, P = Du | 1;                 // odd pitch: the 16 rows a wave reads fall into different banks
    for (int e = tid; e < DTW_TILE * Du; e += 256) {
        const int r = e / Du, k = e - r * Du;
        xs[r * P + k] = (i0 + r < n) ? x[((size_t)b * Tx + i0 + r) * D + skip + k] : 0.0f;
        ys[r * P + k] = (j0 + r < m) ? y[((size_t)b * Ty + j0 + r) * D + skip + k] : 0.0f;
    }
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0.0f;
    for (int k = 0; k < Du; ++k) {
        float xv[4], yv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            xv[a] = xs[(ty + 16 * a) * P + k];
            yv[a] = ys[(tx + 16 * a) * P + k];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float df = xv[a] - yv[c];
                acc[a][c] = __builtin_fmaf(df, df, acc[a][c]);
            }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = i0 + ty + 16 * a;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + tx + 16 * c;
            if (i < n && j < m) dm[((size_t)b * Tx + i) * pitch + j] = (float)sqrt((double)acc[a][c]);
        }
    }
}

// lane l takes v of lane l-1; lane 0 takes `first` (DPP wave_shr:1 with bound_ctrl off keeps `old` where there is no source lane)
__device__ __forceinline__ double dtw_from_left(double v, double first) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(first), __double2loint(v), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(first), __double2hiint(v), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double dtw_readlane(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

__device__ __forceinline__ double dtw_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ int dtw_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// rows 0 .. n-1 against the m <= 64 S reference columns (n, m >= 1, wave-uniform); dm: the pair's distances, `pitch` floats a row
// (a multiple of 4); bp: the pair's backpointer rows.  Returns C(n-1, m-1).
template <int S>
__device__ __forceinline__ double dtw_systolic(const float* __restrict__ dm, int pitch, int n, int m, unsigned* __restrict__ bp, int lane) {
    constexpr int Q = S < 16 ? S : 16, W = S / Q, V = S < 4 ? S : 4;
    typedef float fvec __attribute__((ext_vector_type(V < 2 ? 2 : V)));
    typedef unsigned uvec __attribute__((ext_vector_type(W < 2 ? 2 : W)));
    const double inf = __builtin_huge_val();
    const int col0 = lane * S;
    double c[S];
#pragma unroll
    for (int k = 0; k < S; ++k) c[k] = inf;              // row -1: absent
    double diag = inf, out = inf;
    float dn[S];
    // the strip of row i: S floats from one row, V at a time; a group is loaded iff its first column is below m (the pitch is a
    // multiple of 4 >= m, so the group then ends inside the row).  Columns >= m feed only columns >= m.
    auto load = [&](int i) {
#pragma unroll
        for (int k = 0; k < S; ++k) dn[k] = 0.0f;
        if (i >= 0 && i < n) {
            const float* row = dm + (size_t)i * pitch + col0;
#pragma unroll
            for (int k = 0; k < S; k += V)
                if (col0 + k < m) {
                    if constexpr (V == 1) {
                        dn[k] = row[k];
                    } else {
                        const fvec v = *(const fvec*)(row + k);
#pragma unroll
                        for (int q = 0; q < V; ++q) dn[k + q] = v[q];
                    }
                }
        }
    };
    const int lm = (m - 1) / S, km = (m - 1) % S;        // the lane and register that hold column m - 1
    const int steps = n + lm;                            // lane lm computes row n - 1 at step n - 1 + lm
    load(-lane);
    for (int s = 0; s < steps; ++s) {
        float dc[S];
#pragma unroll
        for (int k = 0; k < S; ++k) dc[k] = dn[k];
        load(s + 1 - lane);                              // the next step's distances: in flight while this step computes
        const int i = s - lane;
        // C(i, l S - 1); lane 0 has no left neighbour: absent, but for cell (0,0), whose predecessor is a virtual 0
        const double left = dtw_from_left(out, s == 0 ? 0.0 : inf);
        if (i >= 0 && i < n) {
            unsigned w[W];
#pragma unroll
            for (int q = 0; q < W; ++q) w[q] = 0u;
            double dg = diag, cur = left;
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const double up = c[k];
                const double m2 = __builtin_fmin(dg, up);             // the two candidates from the row above: off the chain
                const unsigned b2 = up < dg ? 1u : 0u;                // a tie keeps the diagonal
                dg = up;
                const unsigned mv = cur < m2 ? 2u : b2;               // the left one wins only when strictly smaller
                cur = __builtin_fmin(cur, m2) + (double)dc[k];        // the dependent chain: one min, one add a cell
                c[k] = cur;
                w[k / Q] |= mv << (2 * (k % Q));
            }
            diag = lane == 0 ? inf : left;               // C(i, l S - 1) is the next row's diagonal; column -1 stays absent
            out = cur;
            unsigned* dst = bp + ((size_t)i * 64 + lane) * W;
            if constexpr (W == 1) {
                dst[0] = w[0];
            } else {
                uvec wv;
#pragma unroll
                for (int q = 0; q < W; ++q) wv[q] = w[q];
                *(uvec*)dst = wv;
            }
        }
    }
    double res = 0.0;
#pragma unroll
    for (int k = 0; k < S; ++k)
        if (k == km) res = c[k];
    return dtw_readlane(res, lm);
}

struct DtwSums {
    int voiced, vuv;
    double cents, hz;
};

// one path cell per lane: the F0 terms of the pair (frame i of x, frame j of y)
__device__ __forceinline__ void dtw_f0_terms(DtwSums& a, const float* __restrict__ f0x, const float* __restrict__ f0y, int i, int j,
                                             float f0_floor) {
    const float fx = f0x[i], fy = f0y[j];
    const bool vx = fx >= f0_floor, vy = fy >= f0_floor; // a NaN is unvoiced
    if (vx && vy) {
        const double ct = 1200.0 * log2((double)fx / (double)fy), hz = (double)fx - (double)fy;
        a.voiced += 1;
        a.cents += ct * ct;
        a.hz += hz * hz;
    } else if (vx != vy) {
        a.vuv += 1;
    }
}

__global__ __launch_bounds__(64) void dtw_path_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       const int* __restrict__ x_len, const int* __restrict__ y_len,
                                                       const float* __restrict__ f0x, const float* __restrict__ f0y,
                                                       const float* __restrict__ dm, unsigned* __restrict__ bpw, int* __restrict__ rev,
                                                       double* __restrict__ cost, int* __restrict__ path_len, int* __restrict__ voiced,
                                                       int* __restrict__ vuv_errors, double* __restrict__ f0_sq_cents,
                                                       double* __restrict__ f0_sq_hz, int* __restrict__ path, double* totals, int Tx, int Ty,
                                                       int D, int skip, float f0_floor, int mode, int pitch, long long bp_words_per_pair) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = __builtin_amdgcn_readfirstlane(dtw_len(x_len, b, Tx));
    const int m = __builtin_amdgcn_readfirstlane(dtw_len(y_len, b, Ty));
    const int Lp = Tx + Ty - 1;
    if (f0x) {
        f0x += (size_t)b * Tx;
        f0y += (size_t)b * Ty;
    }
    int2* pout = path ? (int2*)path + (size_t)b * Lp : nullptr;
    DtwSums sums = {0, 0, 0.0, 0.0};
    double total = 0.0;
    int P = 0;

    if (n == 0 || m == 0) {
        // an empty side: zeros everywhere
    } else if (mode == 1) {
        P = min(n, m);
        const float* xb = x + (size_t)b * Tx * D;
        const float* yb = y + (size_t)b * Ty * D;
        for (int i = lane; i < P; i += 64) {
            float acc = 0.0f;
            for (int k = skip; k < D; ++k) {
                const float df = xb[(size_t)i * D + k] - yb[(size_t)i * D + k];
                acc = __builtin_fmaf(df, df, acc);
            }
            total += (double)(float)sqrt((double)acc);
            if (f0x) dtw_f0_terms(sums, f0x, f0y, i, i, f0_floor);
            if (pout) pout[i] = make_int2(i, i);
        }
        total = dtw_wave_sum(total);
    } else {
        const float* dmb = dm + (size_t)b * Tx * pitch;
        unsigned* bp = bpw + (size_t)b * bp_words_per_pair;
        int lq;                                          // log2 of the cells per backpointer word; rw: words per row
        if (m <= 64) { total = dtw_systolic<1>(dmb, pitch, n, m, bp, lane); lq = 0; }
        else if (m <= 128) { total = dtw_systolic<2>(dmb, pitch, n, m, bp, lane); lq = 1; }
        else if (m <= 256) { total = dtw_systolic<4>(dmb, pitch, n, m, bp, lane); lq = 2; }
        else if (m <= 512) { total = dtw_systolic<8>(dmb, pitch, n, m, bp, lane); lq = 3; }
        else if (m <= 1024) { total = dtw_systolic<16>(dmb, pitch, n, m, bp, lane); lq = 4; }
        else if (m <= 2048) { total = dtw_systolic<32>(dmb, pitch, n, m, bp, lane); lq = 4; }
        else { total = dtw_systolic<64>(dmb, pitch, n, m, bp, lane); lq = 4; }
        const int rw = m <= 1024 ? 64 : (m <= 2048 ? 128 : 256);
        __threadfence_block();
        __syncthreads();                                 // the backpointers are visible to every lane

        int2* rv = rev ? (int2*)rev + (size_t)b * Lp : nullptr;
        int i = n - 1, j = m - 1, p = 0;
        int ti = -1, tw = 0;                             // the tile: rows ti - 63 .. ti (lane r: row ti - r), words tw - 3 .. tw
        unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        int ei = 0, ej = 0;                              // the path cell this lane holds until the next flush
        auto flush = [&](int base, int cnt) {
            if (lane < cnt) {
                if (rv) rv[base + lane] = make_int2(ei, ej);
                if (f0x) dtw_f0_terms(sums, f0x, f0y, ei, ej, f0_floor);
            }
        };
        for (int trip = 0; trip < n + m; ++trip) {       // a path has at most n + m - 1 cells: bounded whatever bp holds
            if (lane == (p & 63)) {
                ei = i;
                ej = j;
            }
            ++p;
            if ((p & 63) == 0) flush(p - 64, 64);
            if (i == 0 && j == 0) break;
            unsigned mv;
            if (i == 0) mv = 2u;
            else if (j == 0) mv = 1u;
            else {
                const int wj = j >> lq;
                int r = ti - i, k = wj - (tw - 3);
                if (ti < 0 || r < 0 || r > 63 || k < 0 || k > 3) {
                    ti = i;
                    tw = wj;
                    r = 0;
                    k = 3;
                    w0 = w1 = w2 = w3 = 0u;
                    const int ri = i - lane;
                    if (ri >= 0) {
                        const unsigned* row = bp + (size_t)ri * rw;
                        if (tw >= 3) w0 = row[tw - 3];
                        if (tw >= 2) w1 = row[tw - 2];
                        if (tw >= 1) w2 = row[tw - 1];
                        w3 = row[tw];
                    }
                }
                const int ru = __builtin_amdgcn_readfirstlane(r);
                const unsigned a0 = __builtin_amdgcn_readlane(w0, ru), a1 = __builtin_amdgcn_readlane(w1, ru);
                const unsigned a2 = __builtin_amdgcn_readlane(w2, ru), a3 = __builtin_amdgcn_readlane(w3, ru);
                const unsigned word = k == 0 ? a0 : (k == 1 ? a1 : (k == 2 ? a2 : a3));
                mv = (word >> (2 * (j & ((1 << lq) - 1)))) & 3u;
            }
            if (mv != 2u) --i;                           // here i > 0 unless mv == 2, and j > 0 unless mv == 1
            if (mv != 1u) --j;
        }
        P = p;
        flush(p & ~63, p & 63);
        if (pout) {
            __threadfence_block();
            __syncthreads();                             // the reversed path is visible to every lane
            for (int q = lane; q < P; q += 64) pout[q] = rv[P - 1 - q];
        }
    }
    if (pout)
        for (int q = P + lane; q < Lp; q += 64) pout[q] = make_int2(0, 0);

    sums.voiced = dtw_wave_sum(sums.voiced);
    sums.vuv = dtw_wave_sum(sums.vuv);
    sums.cents = dtw_wave_sum(sums.cents);
    sums.hz = dtw_wave_sum(sums.hz);
    if (lane == 0) {
        if (cost) {
            cost[b] = total;
            path_len[b] = P;
            voiced[b] = sums.voiced;
            vuv_errors[b] = sums.vuv;
            f0_sq_cents[b] = sums.cents;
            f0_sq_hz[b] = sums.hz;
        }
        if (totals && P > 0) {                           // the counts are integers below 2^53: exact in any order
            atomicAdd(totals + 0, (double)P);
            atomicAdd(totals + 1, total);
            if (f0x) {
                atomicAdd(totals + 2, (double)sums.voiced);
                atomicAdd(totals + 3, (double)sums.vuv);
                atomicAdd(totals + 4, sums.cents);
                atomicAdd(totals + 5, sums.hz);
            }
        }
    }
}

static inline bool dtw_shape_ok(int B, int Tx, int Ty, int D, int skip) {
    return B >= 1 && Tx >= 1 && Tx <= DTW_TMAX && Ty >= 1 && Ty <= DTW_TMAX && skip >= 0 && skip < D && D - skip <= DTW_DUMAX;
}
static inline int dtw_pitch(int Ty) { return (Ty + 3) & ~3; }
static inline long long dtw_bp_words(int Tx, int Ty) { return (long long)Tx * (Ty <= 1024 ? 64 : (Ty <= 2048 ? 128 : 256)); }

extern "C" long long v100_dtw_workspace_bytes(int B, int Tx, int Ty, int D, int want_path) {
    if (B < 1 || Tx < 1 || Tx > DTW_TMAX || Ty < 1 || Ty > DTW_TMAX || D < 1) return -1;
    long long bytes = 4ll * B * Tx * dtw_pitch(Ty) + 4ll * B * dtw_bp_words(Tx, Ty);
    if (want_path) bytes += 8ll * B * (Tx + Ty - 1);
    return bytes;
}

extern "C" int v100_dtw_score(const float* x, const int* x_len, const float* y, const int* y_len, const float* f0x, const float* f0y,
                              void* ws, double* cost, int* path_len, int* voiced, int* vuv_errors, double* f0_sq_cents, double* f0_sq_hz,
                              int* path, double* totals, int B, int Tx, int Ty, int D, int skip, float f0_floor, int mode, void* stream) {
    if (!x || !y || !ws) return V100_ERR_NULL;
    if ((f0x == nullptr) != (f0y == nullptr)) return V100_ERR_NULL;                          // the two F0 tracks go together
    const bool rows = cost && path_len && voiced && vuv_errors && f0_sq_cents && f0_sq_hz;
    if (!rows && (cost || path_len || voiced || vuv_errors || f0_sq_cents || f0_sq_hz || path)) return V100_ERR_NULL;
    if (!rows && !totals) return V100_ERR_NULL;                                              // the per-row outputs together, or the totals
    if (!dtw_shape_ok(B, Tx, Ty, D, skip) || mode < 0 || mode > 1) return V100_ERR_SHAPE;
    const int pitch = dtw_pitch(Ty);
    float* dm = (float*)ws;
    unsigned* bp = (unsigned*)(dm + (size_t)B * Tx * pitch);
    int* rev = path ? (int*)(bp + (size_t)B * dtw_bp_words(Tx, Ty)) : nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (mode == 0)
        V100_GGL(dtw_dist_kernel, dim3(B, ceil_div(Ty, DTW_TILE), ceil_div(Tx, DTW_TILE)), dim3(256), 0, st, x, y, x_len, y_len, dm, Tx,
                 Ty, D, skip, pitch);
    V100_GGL(dtw_path_kernel, dim3(B), dim3(64), 0, st, x, y, x_len, y_len, f0x, f0y, (const float*)dm, bp, rev, cost, path_len, voiced,
             vuv_errors, f0_sq_cents, f0_sq_hz, path, totals, Tx, Ty, D, skip, f0_floor, mode, pitch, dtw_bp_words(Tx, Ty));
    return v100_launch_status();
}
