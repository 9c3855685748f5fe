// pw_wgrad_group_kernel: several backward-weight problems of the wave-specialised tile in ONE launch, each workgroup carrying
// its tile through the whole contraction (no split-K slabs, no reduce launch).
#pragma once
#include "pointwise_bf16_wgrad_ws.h"
#include "wgrad_group.h"

// The problem record, WG_GROUP_MAX and the tiers: wgrad_group.h.  Here x_mode 1 runs on a 256 x 128 tile, x_mode 0 on 128 x 256.
#define WG_GROUP_RL 2
struct WgGroupParams { WgGroupProblem pr[WG_GROUP_MAX]; int n; };

// Workgroup 8 j + x is slot j of XCD x (workgroups go round the eight XCDs): the tiles of one problem sit on one XCD and share its
// L2; a slot no problem owns exits.  RL: running-sum fragments kept in LDS (pw_wgrad_bf16_ws_body).
template <bool TAIL, int RL>
__global__ __launch_bounds__(768) void pw_wgrad_group_kernel(WgGroupParams g) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[98304 + RL * 32768];
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
    int pi = -1;
    for (int i = 0; i < g.n; ++i)
        if (g.pr[i].xcd == x && j >= g.pr[i].slot0 && j < g.pr[i].slot0 + g.pr[i].ntiles) pi = i;
    if (pi < 0) return;
    const WgGroupProblem& q = g.pr[pi];
    const int t = j - q.slot0;
    WgParams p{(const float*)q.G, nullptr, nullptr, nullptr, nullptr, (const float*)q.X, q.xa, q.xb, q.dW, q.B, q.M, q.K, q.T, q.S, 0, q.x_mode,
               0, 0, 0, 0, 0, 0, 0, 0u, WG_IO_G | WG_IO_X};
    f32x4* const runs = reinterpret_cast<f32x4*>(smem + 98304);
    if (q.x_mode == PW_X_AFFINE_RELU6) {
        const int nkt = q.K / 128;
        pw_wgrad_bf16_ws_body<0, 1, TAIL, WG_IO_G | WG_IO_X, 256, 128, 4, true, RL>(p, 0, t / nkt, t % nkt, smem, smem + 65536, runs);
    } else {
        const int nkt = q.K / 256;
        pw_wgrad_bf16_ws_body<0, 0, TAIL, WG_IO_G | WG_IO_X, 128, 256, 4, true, RL>(p, 0, t / nkt, t % nkt, smem, smem + 32768, runs);
    }
}
