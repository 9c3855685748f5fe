// K12: WORLDLoss (voice100/models/_layers_v1.py:37-93) with the target preparation of
// AlignTextToAudioModel._calc_batch_loss (voice100/models/tts.py:203-206) in one pass, value and gradient.
//
// The reference runs ~25 elementwise / reduction kernels over [B, T, 2+S+Cap] tensors per step: hasf0 = f0 >= 30,
// WORLDNorm.normalize of the three targets, adjust_size, the padding mask, BCE-with-logits, three squared (or absolute)
// errors with the mel-slope weights, four masked sums, the mask sum, four divisions -- and as many again in backward.
// Here one wave owns one frame (b, t) of the decoder output pred [B][Tp][A], A = 1 + 1 + S + Cap, reads the frame and its
// targets once, forms the four loss terms, and writes the frame's gradient for unit upstream gradients straight away;
// per-block partial sums go to a slab that one small kernel reduces in a fixed order (deterministic, no atomics).
#include "common.h"
#include "loss_common.h"
#include <math.h>

struct WorldLossParams {
    const float* pred;      // [B][Tp][A]
    const float* f0;        // [B][Tt]       raw (norm given) or normalised
    const float* hasf0;     // [B][Tt] or null (then hasf0 = raw f0 >= 30, needs norm)
    const float* logspc;    // [B][Tt][S]
    const float* codeap;    // [B][Tt][Cap]
    const int* length;      // [B]
    const float* f0_mean; const float* f0_std; const float* ls_mean; const float* ls_std; const float* ca_mean; const float* ca_std;
    const float* w;         // [S] or null
    float* partial;         // [nblocks][4]
    float* unit;            // [B][Tp][A]
    int B, Tp, Tt, S, Cap, l1;
};

__device__ __forceinline__ void wl_el(bool l1, float d, float& v, float& g) {
    if (l1) { v = fabsf(d); g = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
    else { v = d * d; g = 2.f * d; }
}

__global__ __launch_bounds__(256) void world_loss_kernel(WorldLossParams p) {
    __shared__ float red[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int A = 2 + p.S + p.Cap;
    const int n = min(p.Tp, p.Tt);
    const long fi = (long)blockIdx.x * 4 + wave;
    float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
    if (fi < (long)p.B * p.Tp) {
        const int b = (int)(fi / p.Tp), t = (int)(fi % p.Tp);
        const float* pr = p.pred + fi * A;
        float* un = p.unit + fi * A;
        const bool valid = t < n && t < p.length[b];                 // wave-uniform
        if (!valid) {
            for (int a = lane; a < A; a += 64) un[a] = 0.f;
        } else {
            const float inv_ms = 1.f / wl_mask_sum(p.length, p.B, n, lane);
            const bool l1 = p.l1 != 0;
            const bool norm = p.f0_mean != nullptr;
            const size_t ti = (size_t)b * p.Tt + t;
            const float f0raw = p.f0[ti];
            const float z = p.hasf0 ? p.hasf0[ti] : (f0raw >= 30.0f ? 1.f : 0.f);
            const float f0t = norm ? (f0raw - p.f0_mean[0]) / p.f0_std[0] : f0raw;
            if (lane == 0) {
                const float x = pr[0];
                // binary_cross_entropy_with_logits: max(x, 0) - x*z + log(1 + exp(-|x|))
                t0 = fmaxf(x, 0.f) - x * z + log1pf(expf(-fabsf(x)));
                un[0] = (1.f / (1.f + expf(-x)) - z) * inv_ms;
                float v, g;
                wl_el(l1, pr[1] - f0t, v, g);
                t1 = v * z;
                un[1] = g * z * inv_ms;
            }
            const float wmean = 1.f / (float)p.S;
            for (int s = lane; s < p.S; s += 64) {
                float tg = p.logspc[ti * p.S + s];
                if (norm) tg = (tg - p.ls_mean[s]) / p.ls_std[s];
                const float ws = p.w ? p.w[s] : wmean;
                float v, g;
                wl_el(l1, pr[2 + s] - tg, v, g);
                t2 = fmaf(v, ws, t2);
                un[2 + s] = g * ws * inv_ms;
            }
            const float cmean = 1.f / (float)p.Cap;
            for (int s = lane; s < p.Cap; s += 64) {
                float tg = p.codeap[ti * p.Cap + s];
                if (norm) tg = (tg - p.ca_mean[s]) / p.ca_std[s];
                float v, g;
                wl_el(l1, pr[2 + p.S + s] - tg, v, g);
                t3 = fmaf(v, cmean, t3);
                un[2 + p.S + s] = g * cmean * inv_ms;
            }
        }
    }
    t0 = wave_sum(t0); t1 = wave_sum(t1); t2 = wave_sum(t2); t3 = wave_sum(t3);
    if (lane == 0) { red[wave][0] = t0; red[wave][1] = t1; red[wave][2] = t2; red[wave][3] = t3; }
    __syncthreads();
    if (threadIdx.x < 4)
        p.partial[(size_t)blockIdx.x * 4 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// loss[k] = (sum of the partials in block order, pairwise inside the block of 256 threads) / sum(mask)
__global__ __launch_bounds__(256) void world_loss_finalize_kernel(const float* __restrict__ partial, int nparts, const int* __restrict__ length,
                                                                 int B, int n, float* __restrict__ loss) {
    __shared__ float red[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < nparts; i += 256)
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += partial[(size_t)i * 4 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = wave_sum(s[k]);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) red[wave][k] = s[k];
    const float ms = wl_mask_sum(length, B, n, lane);
    __syncthreads();
    if (threadIdx.x < 4) loss[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x])) / ms;
}

// dpred[b][t][a] = unit[b][t][a] * gout[term(a)]
__global__ void world_loss_bwd_kernel(const float* __restrict__ unit, const float* __restrict__ gout, float* __restrict__ dpred, int S, int Cap,
                                      long total) {
    const int A = 2 + S + Cap;
    const float g0 = gout[0], g1 = gout[1], g2 = gout[2], g3 = gout[3];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int a = (int)(i % A);
        const float g = a == 0 ? g0 : (a == 1 ? g1 : (a < 2 + S ? g2 : g3));
        dpred[i] = unit[i] * g;
    }
}

extern "C" int v100_world_loss_parts(int B, int Tp) { return (int)(((long)B * Tp + 3) / 4); }

extern "C" int v100_world_loss(const float* pred, const float* f0, const float* hasf0, const float* logspc, const float* codeap,
                               const int* length, const float* f0_mean, const float* f0_std, const float* ls_mean, const float* ls_std,
                               const float* ca_mean, const float* ca_std, const float* w, float* partial, float* loss, float* unit,
                               int B, int Tp, int Tt, int S, int Cap, int l1, void* stream) {
    if (!pred || !f0 || !logspc || !codeap || !length || !partial || !loss || !unit) return V100_ERR_NULL;
    if (B <= 0 || Tp <= 0 || Tt <= 0 || S <= 0 || Cap <= 0) return V100_ERR_SHAPE;
    const bool norm = f0_mean != nullptr;
    if (norm && (!f0_std || !ls_mean || !ls_std || !ca_mean || !ca_std)) return V100_ERR_NULL;
    if (!norm && (f0_std || ls_mean || ls_std || ca_mean || ca_std)) return V100_ERR_SHAPE;     // all six or none
    if (!norm && !hasf0) return V100_ERR_NULL;       // hasf0 can only be derived from the RAW f0
    hipStream_t st = (hipStream_t)stream;
    WorldLossParams p{pred, f0, hasf0, logspc, codeap, length, f0_mean, f0_std, ls_mean, ls_std, ca_mean, ca_std, w, partial, unit,
                      B, Tp, Tt, S, Cap, l1};
    const int nparts = v100_world_loss_parts(B, Tp);
    V100_GGL(world_loss_kernel, dim3(nparts), dim3(256), 0, st, p);
    V100_GGL(world_loss_finalize_kernel, dim3(1), dim3(256), 0, st, partial, nparts, length, B, Tp < Tt ? Tp : Tt, loss);
    return v100_launch_status();
}

extern "C" int v100_world_loss_bwd(const float* unit, const float* gout, float* dpred, int B, int Tp, int S, int Cap, void* stream) {
    if (!unit || !gout || !dpred) return V100_ERR_NULL;
    if (B <= 0 || Tp <= 0 || S <= 0 || Cap <= 0) return V100_ERR_SHAPE;
    const long total = (long)B * Tp * (2 + S + Cap);
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    V100_GGL(world_loss_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, unit, gout, dpred, S, Cap, total);
    return v100_launch_status();
}

// ---- K16: the v2 WORLDLoss (voice100/models/_layers_v2.py:116-163) with the target preparation of
// AlignTextToAudio._calc_batch_loss (_tts_v2.py:98-101), value and gradient in one pass.
//
// Five terms instead of K12's four: the per-frame layout is A = 2 + S + 2 Cap (hasf0 logit, f0_hat, logspc_hat[S],
// hascodeap logits[Cap], codeap_hat[Cap]); hascodeap = raw codeap < -0.2 is a second BCE target and gates the codeap error;
// logspc and the two codeap terms are plain means over their features (no mel-slope weights).  Targets are always the RAW
// WORLD features: hasf0 / hascodeap are formed before WORLDNorm.normalize, in the kernel.  Same shape as K12: one wave per
// frame, per-block partials [nblocks][5], a one-block finalize that adds them in block order (deterministic, no atomics).
struct WorldLossV2Params {
    const float* pred;      // [B][Tp][A]
    const float* f0;        // [B][Tt]       raw
    const float* logspc;    // [B][Tt][S]    raw
    const float* codeap;    // [B][Tt][Cap]  raw
    const int* length;      // [B]
    const float* f0_mean; const float* f0_std; const float* ls_mean; const float* ls_std; const float* ca_mean; const float* ca_std;
    float* partial;         // [nblocks][5]
    float* unit;            // [B][Tp][A]
    int B, Tp, Tt, S, Cap, l1;
};

// binary_cross_entropy_with_logits(x, z) and its derivative in x
__device__ __forceinline__ void wl_bce(float x, float z, float& v, float& g) {
    v = fmaxf(x, 0.f) - x * z + log1pf(expf(-fabsf(x)));
    g = 1.f / (1.f + expf(-x)) - z;
}

__global__ __launch_bounds__(256) void world_loss_v2_kernel(WorldLossV2Params p) {
    __shared__ float red[4][5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = p.S, Cap = p.Cap;
    const int A = 2 + S + 2 * Cap;
    const int n = min(p.Tp, p.Tt);
    const long fi = (long)blockIdx.x * 4 + wave;
    float t[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (fi < (long)p.B * p.Tp) {
        const int b = (int)(fi / p.Tp), tt = (int)(fi % p.Tp);
        const float* pr = p.pred + fi * A;
        float* un = p.unit + fi * A;
        const bool valid = tt < n && tt < p.length[b];               // wave-uniform
        if (!valid) {
            for (int a = lane; a < A; a += 64) un[a] = 0.f;
        } else {
            const float inv_ms = 1.f / wl_mask_sum(p.length, p.B, n, lane);
            const bool l1 = p.l1 != 0;
            const size_t ti = (size_t)b * p.Tt + tt;
            if (lane == 0) {
                const float f0raw = p.f0[ti];
                const float z = f0raw >= 30.0f ? 1.f : 0.f;
                const float f0t = (f0raw - p.f0_mean[0]) / p.f0_std[0];
                float v, g;
                wl_bce(pr[0], z, v, g);
                t[0] = v;
                un[0] = g * inv_ms;
                wl_el(l1, pr[1] - f0t, v, g);
                t[1] = v * z;
                un[1] = g * z * inv_ms;
            }
            const float smean = 1.f / (float)S;
            for (int s = lane; s < S; s += 64) {
                const float tg = (p.logspc[ti * S + s] - p.ls_mean[s]) / p.ls_std[s];
                float v, g;
                wl_el(l1, pr[2 + s] - tg, v, g);
                t[2] = fmaf(v, smean, t[2]);
                un[2 + s] = g * smean * inv_ms;
            }
            const float cmean = 1.f / (float)Cap;
            for (int s = lane; s < Cap; s += 64) {
                const float raw = p.codeap[ti * Cap + s];
                const float z = raw < -0.2f ? 1.f : 0.f;
                const float tg = (raw - p.ca_mean[s]) / p.ca_std[s];
                float v, g;
                wl_bce(pr[2 + S + s], z, v, g);
                t[3] = fmaf(v, cmean, t[3]);
                un[2 + S + s] = g * cmean * inv_ms;
                wl_el(l1, pr[2 + S + Cap + s] - tg, v, g);
                t[4] = fmaf(v * z, cmean, t[4]);
                un[2 + S + Cap + s] = g * z * cmean * inv_ms;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) t[k] = wave_sum(t[k]);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 5; ++k) red[wave][k] = t[k];
    __syncthreads();
    if (threadIdx.x < 5)
        p.partial[(size_t)blockIdx.x * 5 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// loss[k] = (sum of the partials in block order, pairwise inside the block of 256 threads) / sum(mask), k < 5
__global__ __launch_bounds__(256) void world_loss_v2_finalize_kernel(const float* __restrict__ partial, int nparts, const int* __restrict__ length,
                                                                    int B, int n, float* __restrict__ loss) {
    __shared__ float red[4][5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < nparts; i += 256)
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] += partial[(size_t)i * 5 + k];
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k] = wave_sum(s[k]);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 5; ++k) red[wave][k] = s[k];
    const float ms = wl_mask_sum(length, B, n, lane);
    __syncthreads();
    if (threadIdx.x < 5) loss[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x])) / ms;
}

// dpred[b][t][a] = unit[b][t][a] * gout[term(a)], terms 0..4 in the v2 layout
__global__ void world_loss_v2_bwd_kernel(const float* __restrict__ unit, const float* __restrict__ gout, float* __restrict__ dpred, int S,
                                         int Cap, long total) {
    const int A = 2 + S + 2 * Cap;
    const float g0 = gout[0], g1 = gout[1], g2 = gout[2], g3 = gout[3], g4 = gout[4];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int a = (int)(i % A);
        const float g = a == 0 ? g0 : (a == 1 ? g1 : (a < 2 + S ? g2 : (a < 2 + S + Cap ? g3 : g4)));
        dpred[i] = unit[i] * g;
    }
}

extern "C" int v100_world_loss_v2(const float* pred, const float* f0, const float* logspc, const float* codeap, const int* length,
                                  const float* f0_mean, const float* f0_std, const float* ls_mean, const float* ls_std,
                                  const float* ca_mean, const float* ca_std, float* partial, float* loss, float* unit,
                                  int B, int Tp, int Tt, int S, int Cap, int l1, void* stream) {
    if (!pred || !f0 || !logspc || !codeap || !length || !partial || !loss || !unit) return V100_ERR_NULL;
    if (!f0_mean || !f0_std || !ls_mean || !ls_std || !ca_mean || !ca_std) return V100_ERR_NULL;
    if (B <= 0 || Tp <= 0 || Tt <= 0 || S <= 0 || Cap <= 0) return V100_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    WorldLossV2Params p{pred, f0, logspc, codeap, length, f0_mean, f0_std, ls_mean, ls_std, ca_mean, ca_std, partial, unit,
                        B, Tp, Tt, S, Cap, l1};
    const int nparts = v100_world_loss_parts(B, Tp);
    V100_GGL(world_loss_v2_kernel, dim3(nparts), dim3(256), 0, st, p);
    V100_GGL(world_loss_v2_finalize_kernel, dim3(1), dim3(256), 0, st, partial, nparts, length, B, Tp < Tt ? Tp : Tt, loss);
    return v100_launch_status();
}

extern "C" int v100_world_loss_v2_bwd(const float* unit, const float* gout, float* dpred, int B, int Tp, int S, int Cap, void* stream) {
    if (!unit || !gout || !dpred) return V100_ERR_NULL;
    if (B <= 0 || Tp <= 0 || S <= 0 || Cap <= 0) return V100_ERR_SHAPE;
    const long total = (long)B * Tp * (2 + S + 2 * Cap);
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    V100_GGL(world_loss_v2_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, unit, gout, dpred, S, Cap, total);
    return v100_launch_status();
}

// ---- K17: TextToAlignText's masked L1 loss (_align_v2.py:80-88), value and gradient in one pass.
// pred [B][L][2] fp32, align [B][W] int64 with W >= 2L + 1 (its first 2L entries are the (gap, len) pairs), text_len [B]:
//   loss = sum_{b, i < text_len[b]} mean_k |log(align[b][2i+k] + 1) - pred[b][i][k]| / sum_b min(text_len[b], L)
// One thread per row (b, i), per-block partials, a one-block finalize in block order; unit = d loss / d pred.
__global__ __launch_bounds__(256) void align_loss_kernel(const float* __restrict__ pred, const long long* __restrict__ align,
                                                         const int* __restrict__ text_len, float* __restrict__ partial,
                                                         float* __restrict__ unit, int B, int L, int W) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    const float inv = 0.5f / wl_mask_sum(text_len, B, L, lane);     // every wave forms the same mask sum (B / 64 loads per lane)
    float v = 0.f;
    if (r < (long)B * L) {
        const int b = (int)(r / L), i = (int)(r % L);
        float g0 = 0.f, g1 = 0.f;
        if (i < text_len[b]) {
            const long long* al = align + (size_t)b * W + 2 * i;
            const float d0 = pred[r * 2] - logf((float)(al[0] + 1));
            const float d1 = pred[r * 2 + 1] - logf((float)(al[1] + 1));
            v = 0.5f * (fabsf(d0) + fabsf(d1));
            g0 = (d0 > 0.f ? 1.f : (d0 < 0.f ? -1.f : 0.f)) * inv;
            g1 = (d1 > 0.f ? 1.f : (d1 < 0.f ? -1.f : 0.f)) * inv;
        }
        unit[r * 2] = g0;
        unit[r * 2 + 1] = g1;
    }
    v = wave_sum(v);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void align_loss_finalize_kernel(const float* __restrict__ partial, int nparts, const int* __restrict__ text_len,
                                                                  int B, int L, float* __restrict__ loss) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s += partial[i];
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    const float ms = wl_mask_sum(text_len, B, L, lane);
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = ((red[0] + red[1]) + (red[2] + red[3])) / ms;
}

extern "C" int v100_align_loss_parts(int B, int L) { return (int)(((long)B * L + 255) / 256); }

extern "C" int v100_align_loss(const float* pred, const long long* align, const int* text_len, float* partial, float* loss, float* unit,
                               int B, int L, int W, void* stream) {
    if (!pred || !align || !text_len || !partial || !loss || !unit) return V100_ERR_NULL;
    if (B <= 0 || L <= 0 || W < 2 * L) return V100_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int nparts = v100_align_loss_parts(B, L);
    V100_GGL(align_loss_kernel, dim3(nparts), dim3(256), 0, st, pred, align, text_len, partial, unit, B, L, W);
    V100_GGL(align_loss_finalize_kernel, dim3(1), dim3(256), 0, st, partial, nparts, text_len, B, L, loss);
    return v100_launch_status();
}

extern "C" int v100_align_loss_bwd(const float* unit, const float* gout, float* dpred, int B, int L, void* stream) {
    if (!unit || !gout || !dpred) return V100_ERR_NULL;
    if (B <= 0 || L <= 0) return V100_ERR_SHAPE;
    const long total = (long)B * L * 2;
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    V100_GGL(scale_by_scalar_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, unit, gout, dpred, total);
    return v100_launch_status();
}
