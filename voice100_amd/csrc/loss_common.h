// Pieces the masked-loss kernels share (world_loss.hip: K12, K16, K17; phone_loss.hip: K22).
#pragma once
#include "common.h"

// sum over b of clamp(length[b], 0, n): the number of unmasked frames (torch.sum(mask), _layers_v1.py:80,88-92)
__device__ __forceinline__ float wl_mask_sum(const int* __restrict__ length, int B, int n, int lane) {
    float s = 0.f;
    for (int b = lane; b < B; b += 64) s += (float)min(max(length[b], 0), n);
    return wave_sum(s);
}

// dpred = unit * gout[0]: the backward of a scalar loss whose gradient for a unit upstream gradient was saved by its forward
static __global__ void scale_by_scalar_kernel(const float* __restrict__ unit, const float* __restrict__ gout, float* __restrict__ dpred, long total) {
    const float g = gout[0];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) dpred[i] = unit[i] * g;
}
