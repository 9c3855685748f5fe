// Adam step of the whole model in ONE launch (torch.optim.Adam as the reference configures it: asr.py:169-176, tts.py:132-135,
// 239-241 -- L2-style weight_decay added to the gradient, bias correction, no amsgrad).  PyTorch's fused multi-tensor Adam
// takes 3 launches and ~145 us for the 11.6 M parameters of asr_en_base (its tensor lists travel in 4 KB kernel-argument
// chunks); here the (parameter, moment) pointers and the chunk list live in device tables that are built once, and only
// the gradient pointers -- autograd hands out fresh gradient tensors every step -- are uploaded per step (8 bytes per tensor).
#include "common.h"
#include <math.h>

struct AdamChunk { int tensor; int count; long long offset; };     // `count` elements of tensor `tensor` starting at `offset`

__device__ __forceinline__ void adam_update(float& pv, float gv, float& mv, float& vv, float lr_over_bc1, float omb1, float beta2,
                                            float omb2, float eps, float weight_decay, float inv_sqrt_bc2) {
    gv = fmaf(weight_decay, pv, gv);
    // omb1 / omb2 = 1 - beta formed in double on the host, as torch does (1.f - 0.999f is off by 1.3e-5 relative)
    mv = fmaf(omb1, gv - mv, mv);                              // exp_avg.lerp_(grad, 1 - beta1)
    vv = fmaf(omb2, gv * gv, beta2 * vv);                      // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    pv -= lr_over_bc1 * mv / (sqrtf(vv) * inv_sqrt_bc2 + eps);
}

__global__ __launch_bounds__(256) void adam_step_kernel(const AdamChunk* __restrict__ chunks, float* const* __restrict__ params,
                                                        const float* const* __restrict__ grads, float* const* __restrict__ exp_avg,
                                                        float* const* __restrict__ exp_avg_sq, float lr_over_bc1, float omb1,
                                                        float beta2, float omb2, float eps, float weight_decay, float inv_sqrt_bc2) {
    const AdamChunk ch = chunks[blockIdx.x];
    float* __restrict__ p = params[ch.tensor] + ch.offset;
    const float* __restrict__ g = grads[ch.tensor] + ch.offset;
    float* __restrict__ m = exp_avg[ch.tensor] + ch.offset;
    float* __restrict__ v = exp_avg_sq[ch.tensor] + ch.offset;
    auto upd = [&](float& pv, float gv, float& mv, float& vv) {
        adam_update(pv, gv, mv, vv, lr_over_bc1, omb1, beta2, omb2, eps, weight_decay, inv_sqrt_bc2);
    };
    const bool vec = ((((size_t)p | (size_t)g | (size_t)m | (size_t)v) & 15) == 0);
    if (vec) {
        const int n4 = ch.count >> 2;
        for (int i = threadIdx.x; i < n4; i += 256) {
            f32x4 pv = reinterpret_cast<f32x4*>(p)[i], mv = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
            const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = pv[e], b = mv[e], c = vv[e];
                upd(a, gv[e], b, c);
                pv[e] = a; mv[e] = b; vv[e] = c;
            }
            reinterpret_cast<f32x4*>(p)[i] = pv; reinterpret_cast<f32x4*>(m)[i] = mv; reinterpret_cast<f32x4*>(v)[i] = vv;
        }
        for (int i = (n4 << 2) + threadIdx.x; i < ch.count; i += 256) upd(p[i], g[i], m[i], v[i]);
    } else {
        for (int i = threadIdx.x; i < ch.count; i += 256) upd(p[i], g[i], m[i], v[i]);
    }
}

extern "C" int v100_adam_chunk_elems() { return 16384; }

// chunks: device array of nchunks {int tensor, int count, long long offset}; params / grads / exp_avg / exp_avg_sq: device arrays of
// float pointers indexed by tensor.  step >= 1 is the number of this update (bias corrections 1 - beta^step).
extern "C" int v100_adam_step(const void* chunks, int nchunks, const void* params, const void* grads, const void* exp_avg,
                              const void* exp_avg_sq, double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                              void* stream) {
    if (!chunks || !params || !grads || !exp_avg || !exp_avg_sq) return V100_ERR_NULL;
    if (nchunks <= 0 || step < 1) return V100_ERR_SHAPE;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    V100_GGL(adam_step_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, (const AdamChunk*)chunks,
                       (float* const*)params, (const float* const*)grads, (float* const*)exp_avg, (float* const*)exp_avg_sq,
                       (float)(lr / bc1), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay,
                       (float)(1.0 / sqrt(bc2)));
    return v100_launch_status();
}

// ---- gradient clipping (torch.nn.utils.clip_grad_norm_ / clip_grad_value_, what Lightning's gradient_clip_val runs between
// backward and optimizer.step()).  Norm clipping is two launches: grad_norm_partials_kernel writes one partial per chunk (sum of
// squares, or max |g| for the infinity norm), then every workgroup of the consuming launch -- the clipped Adam step or the stand-alone
// scale -- reduces ALL the partials itself, in one fixed order, to the total norm and the coefficient.  The workgroups read the same
// values and add them in the same order, so they agree bit for bit without talking to each other inside a launch, and the result is
// the same from run to run (no atomics anywhere on the path).  ~750 partials x 8 bytes per workgroup is L2-resident.
#define V100_NORM_L2 2
#define V100_NORM_INF (-1)
#define V100_CLIP_NORM 1
#define V100_CLIP_VALUE 2

// max that keeps a NaN (torch.amax / linalg.vector_norm(inf) do; fmax drops it)
__device__ __forceinline__ float nan_maxf(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

// sum (or NaN-propagating max) over the 256 threads of the workgroup, in a fixed order; the result in every thread.  lds: 4 doubles.
template <bool MAX>
__device__ __forceinline__ double block_reduce256(double v, double* lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        v = MAX ? nan_max(v, o) : v + o;                       // a + b == b + a: both lanes of a pair hold the same bits
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = lds[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) r = MAX ? nan_max(r, lds[w]) : r + lds[w];
    return r;
}

// total norm from the partials and torch's clip_coef_clamped = clamp(max_norm / (total + 1e-6), max=1) in fp32 -- the division as
// torch evaluates `float / tensor` (reciprocal, then the product), and a clamp that keeps a NaN coefficient a NaN.  Uniform across the
// workgroup, and bit-identical in every workgroup that reads the same partials.  Workgroup 0 stores the total when total_out is set.
__device__ __forceinline__ float clip_coef(const double* __restrict__ partials, int npartials, bool inf, float max_norm,
                                           float* __restrict__ total_out, double* lds) {
    double a = 0.0;
    for (int i = threadIdx.x; i < npartials; i += 256) a = inf ? nan_max(a, partials[i]) : a + partials[i];
    a = inf ? block_reduce256<true>(a, lds) : block_reduce256<false>(a, lds);
    const float total = inf ? (float)a : (float)sqrt(a);
    if (total_out && blockIdx.x == 0 && threadIdx.x == 0) *total_out = total;
    const float coef = (1.0f / (total + 1e-6f)) * max_norm;
    return coef > 1.f ? 1.f : coef;
}

// clip_grad_value_: clamp_min_(-c) then clamp_max_(c), NaN kept
__device__ __forceinline__ float clamp_value(float x, float c) {
    x = x < -c ? -c : x;
    return x > c ? c : x;
}

template <bool INF>
__global__ __launch_bounds__(256) void grad_norm_partials_kernel(const AdamChunk* __restrict__ chunks, const float* const* __restrict__ grads,
                                                                 double* __restrict__ partials) {
    __shared__ double lds[4];
    const AdamChunk ch = chunks[blockIdx.x];
    const float* __restrict__ g = grads[ch.tensor] + ch.offset;
    float acc = 0.f;                                           // fp32 within a lane (64 elements of a 16384-element chunk)
    auto add = [&](float x) { acc = INF ? nan_maxf(acc, fabsf(x)) : fmaf(x, x, acc); };
    int i0 = 0;
    if (((size_t)g & 15) == 0) {
        const int n4 = ch.count >> 2;
        for (int i = threadIdx.x; i < n4; i += 256) {
            const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) add(gv[e]);
        }
        i0 = n4 << 2;
    }
    for (int i = i0 + threadIdx.x; i < ch.count; i += 256) add(g[i]);
    const double r = block_reduce256<INF>((double)acc, lds);  // fp64 across lanes and, in clip_coef, across chunks
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// the Adam step of adam_step_kernel on the clipped gradient, which is also written back to grads (p.grad after torch's in-place clip)
template <int MODE>
__global__ __launch_bounds__(256) void adam_step_clip_kernel(const AdamChunk* __restrict__ chunks, float* const* __restrict__ params,
                                                             float* const* __restrict__ grads, float* const* __restrict__ exp_avg,
                                                             float* const* __restrict__ exp_avg_sq, float lr_over_bc1, float omb1,
                                                             float beta2, float omb2, float eps, float weight_decay, float inv_sqrt_bc2,
                                                             float clip, const double* __restrict__ partials, int npartials, int inf,
                                                             float* __restrict__ total_out) {
    __shared__ double lds[4];
    const float coef = MODE == V100_CLIP_NORM ? clip_coef(partials, npartials, inf != 0, clip, total_out, lds) : 1.f;
    const bool write_g = MODE == V100_CLIP_VALUE || coef != 1.f;     // uniform: a coefficient of exactly 1 leaves every bit as it is
    const AdamChunk ch = chunks[blockIdx.x];
    float* __restrict__ p = params[ch.tensor] + ch.offset;
    float* __restrict__ g = grads[ch.tensor] + ch.offset;
    float* __restrict__ m = exp_avg[ch.tensor] + ch.offset;
    float* __restrict__ v = exp_avg_sq[ch.tensor] + ch.offset;
    auto cl = [&](float x) { return MODE == V100_CLIP_NORM ? x * coef : clamp_value(x, clip); };
    auto upd = [&](float& pv, float gv, float& mv, float& vv) {
        adam_update(pv, gv, mv, vv, lr_over_bc1, omb1, beta2, omb2, eps, weight_decay, inv_sqrt_bc2);
    };
    int i0 = 0;
    if (((((size_t)p | (size_t)g | (size_t)m | (size_t)v) & 15) == 0)) {
        const int n4 = ch.count >> 2;
        for (int i = threadIdx.x; i < n4; i += 256) {
            f32x4 pv = reinterpret_cast<f32x4*>(p)[i], mv = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
            f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                gv[e] = cl(gv[e]);
                float a = pv[e], b = mv[e], c = vv[e];
                upd(a, gv[e], b, c);
                pv[e] = a; mv[e] = b; vv[e] = c;
            }
            if (write_g) reinterpret_cast<f32x4*>(g)[i] = gv;
            reinterpret_cast<f32x4*>(p)[i] = pv; reinterpret_cast<f32x4*>(m)[i] = mv; reinterpret_cast<f32x4*>(v)[i] = vv;
        }
        i0 = n4 << 2;
    }
    for (int i = i0 + threadIdx.x; i < ch.count; i += 256) {
        const float gv = cl(g[i]);
        if (write_g) g[i] = gv;
        upd(p[i], gv, m[i], v[i]);
    }
}

// stand-alone clip of a gradient list (optim.clip_grad_norm_ / clip_grad_value_): scale by the coefficient, or clamp, in place
template <int MODE>
__global__ __launch_bounds__(256) void grad_clip_kernel(const AdamChunk* __restrict__ chunks, float* const* __restrict__ grads, float clip,
                                                        const double* __restrict__ partials, int npartials, int inf,
                                                        float* __restrict__ total_out) {
    __shared__ double lds[4];
    const float coef = MODE == V100_CLIP_NORM ? clip_coef(partials, npartials, inf != 0, clip, total_out, lds) : 1.f;
    if (MODE == V100_CLIP_NORM && coef == 1.f) return;        // uniform
    const AdamChunk ch = chunks[blockIdx.x];
    float* __restrict__ g = grads[ch.tensor] + ch.offset;
    auto cl = [&](float x) { return MODE == V100_CLIP_NORM ? x * coef : clamp_value(x, clip); };
    int i0 = 0;
    if (((size_t)g & 15) == 0) {
        const int n4 = ch.count >> 2;
        for (int i = threadIdx.x; i < n4; i += 256) {
            f32x4 gv = reinterpret_cast<f32x4*>(g)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) gv[e] = cl(gv[e]);
            reinterpret_cast<f32x4*>(g)[i] = gv;
        }
        i0 = n4 << 2;
    }
    for (int i = i0 + threadIdx.x; i < ch.count; i += 256) g[i] = cl(g[i]);
}

extern "C" int v100_grad_norm_partials(const void* chunks, int nchunks, const void* grads, void* partials, int norm_type, void* stream) {
    if (!chunks || !grads || !partials) return V100_ERR_NULL;
    if (nchunks <= 0 || (norm_type != V100_NORM_L2 && norm_type != V100_NORM_INF)) return V100_ERR_SHAPE;
    if (norm_type == V100_NORM_INF)
        V100_GGL(grad_norm_partials_kernel<true>, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, (const AdamChunk*)chunks,
                 (const float* const*)grads, (double*)partials);
    else
        V100_GGL(grad_norm_partials_kernel<false>, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, (const AdamChunk*)chunks,
                 (const float* const*)grads, (double*)partials);
    return v100_launch_status();
}

static int check_clip(int clip_mode, double clip, const void* partials, int npartials, int norm_type) {
    if (clip_mode == V100_CLIP_NORM) {
        if (!partials) return V100_ERR_NULL;
        if (npartials <= 0 || (norm_type != V100_NORM_L2 && norm_type != V100_NORM_INF)) return V100_ERR_SHAPE;
        return V100_OK;
    }
    return clip_mode == V100_CLIP_VALUE ? V100_OK : V100_ERR_SHAPE;
}

extern "C" int v100_adam_step_clip(const void* chunks, int nchunks, const void* params, const void* grads, const void* exp_avg,
                                   const void* exp_avg_sq, double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                                   int clip_mode, double clip, const void* partials, int npartials, int norm_type, void* total_norm,
                                   void* stream) {
    if (!chunks || !params || !grads || !exp_avg || !exp_avg_sq) return V100_ERR_NULL;
    if (nchunks <= 0 || step < 1) return V100_ERR_SHAPE;
    if (int rc = check_clip(clip_mode, clip, partials, npartials, norm_type)) return rc;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const int inf = norm_type == V100_NORM_INF;
#define V100_ADAM_CLIP_LAUNCH(MODE)                                                                                                       \
    V100_GGL(adam_step_clip_kernel<MODE>, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, (const AdamChunk*)chunks,         \
             (float* const*)params, (float* const*)grads, (float* const*)exp_avg, (float* const*)exp_avg_sq, (float)(lr / bc1),           \
             (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay, (float)(1.0 / sqrt(bc2)),         \
             (float)clip, (const double*)partials, npartials, inf, (float*)total_norm)
    if (clip_mode == V100_CLIP_NORM) V100_ADAM_CLIP_LAUNCH(V100_CLIP_NORM);
    else V100_ADAM_CLIP_LAUNCH(V100_CLIP_VALUE);
#undef V100_ADAM_CLIP_LAUNCH
    return v100_launch_status();
}

extern "C" int v100_grad_clip(const void* chunks, int nchunks, const void* grads, int clip_mode, double clip, const void* partials,
                              int npartials, int norm_type, void* total_norm, void* stream) {
    if (!chunks || !grads) return V100_ERR_NULL;
    if (nchunks <= 0) return V100_ERR_SHAPE;
    if (int rc = check_clip(clip_mode, clip, partials, npartials, norm_type)) return rc;
    const int inf = norm_type == V100_NORM_INF;
    if (clip_mode == V100_CLIP_NORM)
        V100_GGL(grad_clip_kernel<V100_CLIP_NORM>, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, (const AdamChunk*)chunks,
                 (float* const*)grads, (float)clip, (const double*)partials, npartials, inf, (float*)total_norm);
    else
        V100_GGL(grad_clip_kernel<V100_CLIP_VALUE>, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, (const AdamChunk*)chunks,
                 (float* const*)grads, (float)clip, (const double*)partials, npartials, inf, (float*)total_norm);
    return v100_launch_status();
}
