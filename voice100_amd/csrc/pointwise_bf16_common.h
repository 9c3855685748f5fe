// Shared by the bf16-operand 1x1 GEMM kernels (pointwise_bf16.hip and the pointwise_bf16_*.h kernel headers).
#pragma once
#include <type_traits>
#include "pointwise_common.h"

// =============================================================================================
// bf16 path: operands rounded to bf16 while staging, fp32 accumulate (v_mfma_f32_32x32x16_bf16).
// LDS images are [row][k] with k contiguous (64 bf16 = 128 B per row) and a 16-byte-chunk XOR
// swizzle chunk ^= (row >> 1) & 7 so the fragment ds_read_b128 of 32 consecutive rows is
// conflict-free (bank rule (a/4) % 64; the hardware's four 16-lane groups each see every slot of both row
// parities once).  (Also spreading the X-patch STORES, whose lanes hold rows 4 apart, with an extra
// ^ ((row >> 4) & 1) and a lane remap was measured: no gain, so the simpler form stays.)
// =============================================================================================
#define BF_BK 64

__device__ __forceinline__ int bf_off(int row, int chunk) {          // byte offset inside a [128][64] bf16 tile
    return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
