// The grouped backward-weight launch (pointwise_bf16_wgrad_group.h): eligibility, placement and the C entry point.
#include "pointwise_bf16_wgrad_small.h"
#include "timing.h"

// 1 when a weight gradient with these operands can join a grouped launch: the finished-gradient forms of the wave-specialised
// kernel (G plain; x_mode 1 = project, 256 x 128 tile; x_mode 0 = expand on da1, 128 x 256 tile), every operand bf16-stored, whole
// tiles, a split count v100_pw_wgrad_io takes
extern "C" int v100_pw_wgrad_group_supported(int B, int M, int K, int T, int S, int g_mode, int x_mode, int io16) {
    if (B <= 0 || M <= 0 || K <= 0 || T <= 0 || S <= 0 || (S > B && (S % B != 0 || S / B > 64))) return 0;
    if (g_mode != PW_X_NONE || (x_mode != PW_X_NONE && x_mode != PW_X_AFFINE_RELU6) || io16 != (WG_IO_G | WG_IO_X)) return 0;
    const int GR = x_mode ? 256 : 128, XR = x_mode ? 128 : 256;
    if (M % GR || K % XR) return 0;
    const int P = pw_pitch16(T, B);
    return ((long)(M + 256) * P * 4 < 0x7fffffffL && (long)(K + 256) * P * 4 < 0x7fffffffL) ? 1 : 0;
}

// tiles of problem i of a grouped launch (0: not eligible)
extern "C" int v100_pw_wgrad_group_tiles(int M, int K, int x_mode) {
    const int GR = x_mode ? 256 : 128, XR = x_mode ? 128 : 256;
    return (M > 0 && K > 0 && M % GR == 0 && K % XR == 0) ? (M / GR) * (K / XR) : 0;
}

// ptrs (HOST, 5 per problem): G X xa xb dW; dims (HOST, 8 per problem): B M K T S g_mode x_mode io16
extern "C" int v100_pw_wgrad_group(int n, const void* const* ptrs, const int* dims, void* stream) {
    if (!ptrs || !dims) return V100_ERR_NULL;
    if (n <= 0 || n > WG_GROUP_MAX) return V100_ERR_SHAPE;
    WgGroupParams g;
    g.n = n;
    int fill[8] = {0, 0, 0, 0, 0, 0, 0, 0};            // slots taken on each XCD
    bool tail = false;
    for (int i = 0; i < n; ++i) {
        const void* const* P = ptrs + 5 * i;
        const int* d = dims + 8 * i;
        if (!P[0] || !P[1] || !P[4] || (d[6] != PW_X_NONE && (!P[2] || !P[3]))) return V100_ERR_NULL;
        if (!v100_pw_wgrad_group_supported(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7])) return V100_ERR_SHAPE;
        WgGroupProblem& q = g.pr[i];
        q.G = P[0]; q.X = P[1]; q.xa = (const float*)P[2]; q.xb = (const float*)P[3]; q.dW = (float*)P[4];
        q.B = d[0]; q.M = d[1]; q.K = d[2]; q.T = d[3]; q.S = d[4]; q.x_mode = d[6];
        q.ntiles = v100_pw_wgrad_group_tiles(q.M, q.K, q.x_mode);
        int x = 0;                                      // the emptiest XCD so far (the first of equals)
        for (int c = 1; c < 8; ++c) if (fill[c] < fill[x]) x = c;
        q.xcd = x; q.slot0 = fill[x];
        fill[x] += q.ntiles;
        tail = tail || q.T % BF_BK != 0;
    }
    int slots = 0;
    for (int c = 0; c < 8; ++c) if (fill[c] > slots) slots = fill[c];
    hipStream_t st = (hipStream_t)stream;
    V100TimedRegion timed(V100_T_PW_WGRAD, st);
    // (the tail form is right for whole steps too: its masks then never apply)
    if (tail) V100_GGL((pw_wgrad_group_kernel<true, WG_GROUP_RL>), dim3((unsigned)(8 * slots)), dim3(768), 0, st, g);
    else V100_GGL((pw_wgrad_group_kernel<false, WG_GROUP_RL>), dim3((unsigned)(8 * slots)), dim3(768), 0, st, g);
    return v100_launch_status();
}

// ---- the same launch on 128 x 128 tiles (pointwise_bf16_wgrad_small.h), for gradients with too few 256 x 128 tiles ----

// as v100_pw_wgrad_group_supported, whole 128 x 128 tiles in both modes
extern "C" int v100_pw_wgrad_group_small_supported(int B, int M, int K, int T, int S, int g_mode, int x_mode, int io16) {
    if (B <= 0 || M <= 0 || K <= 0 || T <= 0 || S <= 0 || (S > B && (S % B != 0 || S / B > 64))) return 0;
    if (g_mode != PW_X_NONE || (x_mode != PW_X_NONE && x_mode != PW_X_AFFINE_RELU6) || io16 != (WG_IO_G | WG_IO_X)) return 0;
    if (M % 128 || K % 128) return 0;
    const int P = pw_pitch16(T, B);
    return ((long)(M + 256) * P * 4 < 0x7fffffffL && (long)(K + 256) * P * 4 < 0x7fffffffL) ? 1 : 0;
}

extern "C" int v100_pw_wgrad_group_small_tiles(int M, int K, int x_mode) {
    (void)x_mode;
    return (M > 0 && K > 0 && M % 128 == 0 && K % 128 == 0) ? (M / 128) * (K / 128) : 0;
}

// tables as v100_pw_wgrad_group's
extern "C" int v100_pw_wgrad_group_small(int n, const void* const* ptrs, const int* dims, void* stream) {
    if (!ptrs || !dims) return V100_ERR_NULL;
    if (n <= 0 || n > WG_GROUP_MAX) return V100_ERR_SHAPE;
    WgGroupParams g;
    g.n = n;
    int fill[8] = {0, 0, 0, 0, 0, 0, 0, 0};            // slots taken on each XCD
    bool tail = false;
    for (int i = 0; i < n; ++i) {
        const void* const* P = ptrs + 5 * i;
        const int* d = dims + 8 * i;
        if (!P[0] || !P[1] || !P[4] || (d[6] != PW_X_NONE && (!P[2] || !P[3]))) return V100_ERR_NULL;
        if (!v100_pw_wgrad_group_small_supported(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7])) return V100_ERR_SHAPE;
        WgGroupProblem& q = g.pr[i];
        q.G = P[0]; q.X = P[1]; q.xa = (const float*)P[2]; q.xb = (const float*)P[3]; q.dW = (float*)P[4];
        q.B = d[0]; q.M = d[1]; q.K = d[2]; q.T = d[3]; q.S = d[4]; q.x_mode = d[6];
        q.ntiles = v100_pw_wgrad_group_small_tiles(q.M, q.K, q.x_mode);
        int x = 0;                                      // the emptiest XCD so far (the first of equals)
        for (int c = 1; c < 8; ++c) if (fill[c] < fill[x]) x = c;
        q.xcd = x; q.slot0 = fill[x];
        fill[x] += q.ntiles;
        tail = tail || q.T % BF_BK != 0;
    }
    int slots = 0;
    for (int c = 0; c < 8; ++c) if (fill[c] > slots) slots = fill[c];
    hipStream_t st = (hipStream_t)stream;
    V100TimedRegion timed(V100_T_PW_WGRAD, st);
    if (tail) V100_GGL((pw_wgrad_group_small_kernel<true>), dim3((unsigned)(8 * slots)), dim3(512), 0, st, g);
    else V100_GGL((pw_wgrad_group_small_kernel<false>), dim3((unsigned)(8 * slots)), dim3(512), 0, st, g);
    return v100_launch_status();
}
