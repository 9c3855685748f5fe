// The grouped backward-weight launch as host code sees it: the problem record, the two tiers and the launcher
// (pointwise_bf16_group.hip).  No device code: the stack executor (block.hip) includes this, the kernels' headers include it too.
#pragma once
#include <hip/hip_runtime.h>

// One problem of a grouped launch: dW[M][K] = sum_{b,t} G[b][m][t] * x'[b][k][t], both operands bf16-stored (WG_IO_G | WG_IO_X),
// G plain, X plain (x_mode 0: the expand gradient on da1) or relu6(xa x + xb) (x_mode 1: the project gradient).
// S: the split count whose summation order the workgroup reproduces (v100_pw_wgrad_splits).
struct WgGroupProblem {
    const void* G; const void* X; const float* xa; const float* xb; float* dW;
    int B, M, K, T, S, x_mode;
    int xcd, slot0, ntiles;      // placement (launcher): tile i of the problem runs as workgroup 8 * (slot0 + i) + xcd
};
#define WG_GROUP_MAX 16          // problems of one launch
#define WG_GROUP_CHIP_TILES 256  // one tile per CU: the most a tier-1 launch is planned for

// A tier is a tile shape with its kernel.  WG_TIER_WIDE: the wave-specialised 256 x 128 (project) / 128 x 256 (expand) tile, for the
// wide blocks; WG_TIER_SMALL: 128 x 128 in both modes, for gradients with too few wide tiles to fill the chip.
enum WgTier { WG_TIER_WIDE = 0, WG_TIER_SMALL = 1 };

// 1 when the problem (shape fields) can join a launch of the tier: whole tiles, a split count v100_pw_wgrad_io takes
int pw_wgrad_group_supported(WgTier tier, const WgGroupProblem& q);
// tiles of an M x K gradient (0: not whole tiles)
int pw_wgrad_group_tiles(WgTier tier, int M, int K, int x_mode);
// n <= WG_GROUP_MAX problems with operands and shape fields filled in -> one launch; the placement is filled in here
int pw_wgrad_group_launch(WgTier tier, int n, const WgGroupProblem* problems, hipStream_t stream);
