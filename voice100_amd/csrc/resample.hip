// Sample-rate conversion on the device: torchaudio.functional.resample's default method (windowed-sinc polyphase bank, Hann window),
// the step between a decoded audio file and every feature this library computes (voice100/data_modules.py:288-289).
//
//   y[q n + p] = sum_j K[p][j] x[q o + j - width],   x zero outside [0, len),   ceil(n len / o) outputs,
//
// for a rate pair reduced to o / n.  Phase p's taps are non-zero only where |j - width - p o / n| < width, so the host hands the bank
// over in compact form: starts[p] = floor(p o / n) and L = 2 width + 2 taps from there.  Output m = q n + p then reads the L inputs
// from floor(m o / n) - width on: the first input of consecutive outputs never moves backwards, and TILE consecutive outputs need
// one contiguous span of about TILE o / n + L inputs.
//
// One workgroup per (utterance, TILE consecutive outputs).  It stages that span in LDS once, with the zero padding applied while
// staging -- a sample outside [0, len) is never read from memory, so a ragged batch may hold anything beyond a row's length -- and,
// when it fits beside the span, the whole compact bank (pitch L + 1 floats, odd: the 64 lanes of a wave read 64 consecutive phases
// at one tap index, and an odd pitch spreads them over all banks).  A bank too large for LDS is read through the cache instead.
// Each thread then owns outputs tile + tid, + 256, ...: L fused multiply-adds in tap order, fp32.  An output whose window is not
// inside the staged span (a span longer than the LDS budget -- rate pairs with a huge o / n -- or a `starts` table that is not the
// one described above) takes the same L steps on bounds-checked global reads: slower, same bits, never out of bounds.
// The kernel also writes the zeros from an utterance's last output to Mmax, and out_lens[b].
//
// HBM-bound by a wide margin (16 x 10 s at 44.1 kHz: 28 MB in, 10 MB out, ~36 FMAs per output), so it is written for the edges.
#include "common.h"
#include "../../include/voice100_hip.h"

namespace {
constexpr int kThreads = 256;
constexpr int kTile = 1024;                 // outputs per workgroup
constexpr int kLdsFloats = 16384;           // 64 KiB: the span and (when it fits) the bank
constexpr int kSpanMax = 12288;             // longest staged span; outputs beyond it read global memory

struct ResampleParams {
    const float* x; const int* lens; const float* taps; const int* starts; float* y; int* out_lens;
    int Nmax, Mmax, o, n, width, L;
    int pitch;          // LDS row pitch of the bank (odd)
    int span_cap;       // floats of LDS reserved for the input span
};

__host__ __device__ inline long long resample_out_len(long long len, int o, int n) {
    return (len / o) * n + ((len % o) * n + o - 1) / o;           // ceil(n len / o) without forming n len
}

template <bool BANK_IN_LDS>
__global__ __launch_bounds__(kThreads) void resample_sinc_kernel(ResampleParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* xs = lds;                         // [span_cap]
    float* bank = lds + p.span_cap;          // [n][pitch] when BANK_IN_LDS
    const int tid = threadIdx.x, b = blockIdx.y;
    const int o = p.o, n = p.n, L = p.L;

    int len = p.lens ? p.lens[b] : p.Nmax;
    len = min(max(len, 0), p.Nmax);
    const int M = (int)min(resample_out_len(len, o, n), (long long)p.Mmax);       // this row's outputs
    if (blockIdx.x == 0 && tid == 0 && p.out_lens) p.out_lens[b] = M;

    const float* xrow = p.x + (size_t)b * p.Nmax;
    float* yrow = p.y + (size_t)b * p.Mmax;
    const long long m0 = (long long)blockIdx.x * kTile;
    const int mend = (int)min(m0 + kTile, (long long)p.Mmax);
    if (m0 >= M) {                           // a tile beyond the utterance: zeros only
        for (long long m = m0 + tid; m < mend; m += kThreads) yrow[m] = 0.0f;
        return;
    }

    // the span of inputs the tile's live outputs [m0, mlast] read: [lo, lo + span)
    const int mlast = min(mend, M) - 1;
    const int q0 = (int)m0 / n, q1 = mlast / n;
    const long long lo = (long long)q0 * o + p.starts[(int)m0 - q0 * n] - p.width;
    const long long hi = (long long)q1 * o + p.starts[mlast - q1 * n] - p.width + L;
    const int span = (int)min(max(hi - lo, 0LL), (long long)p.span_cap);
    for (int i = tid; i < span; i += kThreads) {
        const long long g = lo + i;
        xs[i] = (g >= 0 && g < len) ? xrow[g] : 0.0f;
    }
    if (BANK_IN_LDS) {
        for (int i = tid; i < n * L; i += kThreads) {
            const int r = i / L;
            bank[r * p.pitch + (i - r * L)] = p.taps[i];
        }
    }
    __syncthreads();

    for (long long mm = m0 + tid; mm < mend; mm += kThreads) {          // 64-bit: the last tile may end at 2^31 - 1
        const int m = (int)mm;
        float acc = 0.0f;
        if (m < M) {
            const int q = m / n, ph = m - q * n;
            const long long g0 = (long long)q * o + p.starts[ph] - p.width;       // first input of this output's window
            const float* k = BANK_IN_LDS ? bank + ph * p.pitch : p.taps + (size_t)ph * L;
            const long long rel = g0 - lo;
            if (rel >= 0 && rel + L <= span) {
                const float* xw = xs + rel;
                for (int j = 0; j < L; ++j) acc = fmaf(k[j], xw[j], acc);
            } else {
                for (int j = 0; j < L; ++j) {
                    const long long g = g0 + j;
                    const float xv = (g >= 0 && g < len) ? xrow[g] : 0.0f;
                    acc = fmaf(k[j], xv, acc);
                }
            }
        }
        yrow[m] = acc;
    }
}
}  // namespace

extern "C" long long v100_resample_out_len(long long len, int o, int n) {
    if (len < 0 || o < 1 || n < 1) return -1;
    return resample_out_len(len, o, n);
}

extern "C" int v100_resample_tile(void) { return kTile; }

extern "C" int v100_resample_sinc(const float* x, const int* lens, const float* taps, const int* starts, float* y, int* out_lens,
                                  int B, int Nmax, int Mmax, int o, int n, int width, int L, void* stream) {
    if (!x || !taps || !starts || !y) return V100_ERR_NULL;
    if (B < 1 || B > 65535 || Nmax < 1 || Mmax < 1 || o < 1 || n < 1 || width < 1 || L < 1) return V100_ERR_SHAPE;
    ResampleParams p{x, lens, taps, starts, y, out_lens, Nmax, Mmax, o, n, width, L, L | 1, 0};
    // inputs between the first windows of a tile's first and last output, plus one window (and one for the floor)
    const long long need = ((long long)(kTile - 1) * o + n - 1) / n + L + 1;
    p.span_cap = (int)((need < kSpanMax ? need : kSpanMax) + 3) & ~3;
    const long long bank = (long long)n * p.pitch;
    const bool bank_in_lds = p.span_cap + bank <= kLdsFloats;
    const size_t shmem = sizeof(float) * (size_t)(p.span_cap + (bank_in_lds ? bank : 0));
    const dim3 grid((unsigned)((Mmax - 1) / kTile + 1), (unsigned)B);
    if (bank_in_lds) V100_GGL(resample_sinc_kernel<true>, grid, dim3(kThreads), shmem, (hipStream_t)stream, p);
    else V100_GGL(resample_sinc_kernel<false>, grid, dim3(kThreads), shmem, (hipStream_t)stream, p);
    return v100_launch_status();
}
