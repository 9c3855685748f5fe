// K22: the phone head's masked cross-entropy of AlignTextToAudioMultiTaskModel (voice100/models/tts.py:328-331), value and
// gradient in one pass, on the logits as the 1x1 head writes them -- channel first, [B][V][L]:
//
//   ce   = CrossEntropyLoss(reduction='none')(logits [B, V, L], target [B, L])
//   mask = arange(L)[None, :] < target_len[:, None]
//   loss = sum(ce * mask) / sum(mask)
//
// The reference spends about a dozen launches per direction on this (log_softmax, nll, the mask, two sums, a division).  Here a
// workgroup owns 64 consecutive columns l of one utterance b: the lanes of a wave run along l, so every row v of the [V][L] plane is
// read and written as one coalesced 256-byte segment, and the four waves split the rows (wave w takes v = w, w + 4, ...).  Three
// sweeps over V -- the maximum, sum exp(x - max), then unit = (softmax - onehot) * mask / sum(mask) -- of which the second and third
// hit L2 (64 columns x 71 rows are 18 KB); the waves combine their maxima and sums through LDS in a fixed order.  Per-workgroup
// partial sums go to a slab that one small kernel adds in block order: deterministic, no atomics, identical bits from call to call.
//
// torch's semantics: sum(mask) = sum_b clamp(target_len[b], 0, L); target == -100 (the default ignore_index) gives 0 and a zero
// gradient but still counts in sum(mask) when inside the length; every length 0 gives 0 / 0 = NaN.  Any other target outside [0, V)
// (torch raises there) is never used as an index: that element's loss is NaN, so a run shows it.  A masked column is never loaded.
#include "common.h"
#include "loss_common.h"
#include <math.h>

#define MCE_IGNORE (-100LL)

__global__ __launch_bounds__(256) void masked_ce_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                                        const int* __restrict__ target_len, float* __restrict__ partial,
                                                        float* __restrict__ unit, int B, int V, int L, int nlb) {
    __shared__ float red[2][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x / nlb, l = (blockIdx.x % nlb) * 64 + lane;
    const bool inside = l < L;
    const bool valid = inside && l < target_len[b];
    const float ms = wl_mask_sum(target_len, B, L, lane);               // by every lane, before the lanes part ways
    const size_t col = (size_t)b * V * L + (size_t)(inside ? l : 0);     // + v * L: row v of this column
    const float* x = logits + col;
    float* u = unit + col;

    float m = -INFINITY;
    if (valid)
        for (int v = wave; v < V; v += 4) m = fmaxf(m, x[(size_t)v * L]);
    red[0][wave][lane] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0][0][lane], red[0][1][lane]), fmaxf(red[0][2][lane], red[0][3][lane]));

    float s = 0.f;
    if (valid)
        for (int v = wave; v < V; v += 4) s += expf(x[(size_t)v * L] - m);
    red[1][wave][lane] = s;
    __syncthreads();
    s = (red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane]);

    const long long t = valid ? target[(size_t)b * L + l] : MCE_IGNORE;
    const bool counted = valid && t != MCE_IGNORE;                    // ignore_index: no loss, no gradient
    const bool in_range = t >= 0 && t < (long long)V;
    if (inside) {
        // (wave-uniform loop bounds; a masked or ignored column writes zeros and loads nothing)
        const float scale = counted ? 1.f / (s * ms) : 0.f;
        for (int v = wave; v < V; v += 4) {
            float g = 0.f;
            if (counted) g = (expf(x[(size_t)v * L] - m) - ((long long)v == t ? s : 0.f)) * scale;
            u[(size_t)v * L] = g;
        }
    }

    if (wave == 0) {
        float ce = 0.f;
        if (counted) ce = in_range ? logf(s) + (m - x[(size_t)t * L]) : NAN;
        ce = wave_sum(ce);
        if (lane == 0) partial[blockIdx.x] = ce;
    }
}

// loss = (the partials in block order, pairwise inside the block of 256 threads) / sum(mask)
__global__ __launch_bounds__(256) void masked_ce_finalize_kernel(const float* __restrict__ partial, int nparts, const int* __restrict__ target_len,
                                                                 int B, int L, float* __restrict__ loss) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s += partial[i];
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    const float ms = wl_mask_sum(target_len, B, L, lane);
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = ((red[0] + red[1]) + (red[2] + red[3])) / ms;
}

extern "C" int v100_masked_ce_parts(int B, int L) {
    if (B <= 0 || L <= 0) return -1;
    const long n = (long)B * ((L + 63) / 64);
    return n > 0x7fffffffL ? -1 : (int)n;
}

extern "C" int v100_masked_ce(const float* logits, const long long* target, const int* target_len, float* partial, float* loss,
                              float* unit, int B, int V, int L, void* stream) {
    if (!logits || !target || !target_len || !partial || !loss || !unit) return V100_ERR_NULL;
    if (B <= 0 || V <= 0 || L <= 0) return V100_ERR_SHAPE;
    const int nparts = v100_masked_ce_parts(B, L);
    if (nparts < 0) return V100_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    V100_GGL(masked_ce_kernel, dim3(nparts), dim3(256), 0, st, logits, target, target_len, partial, unit, B, V, L, (L + 63) / 64);
    V100_GGL(masked_ce_finalize_kernel, dim3(1), dim3(256), 0, st, partial, nparts, target_len, B, L, loss);
    return v100_launch_status();
}

extern "C" int v100_masked_ce_bwd(const float* unit, const float* gout, float* dlogits, int B, int V, int L, void* stream) {
    if (!unit || !gout || !dlogits) return V100_ERR_NULL;
    if (B <= 0 || V <= 0 || L <= 0) return V100_ERR_SHAPE;
    const long total = (long)B * V * L;
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    V100_GGL(scale_by_scalar_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, unit, gout, dlogits, total);
    return v100_launch_status();
}
