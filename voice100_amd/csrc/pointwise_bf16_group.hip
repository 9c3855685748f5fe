// The grouped backward-weight launch (wgrad_group.h): the two tiers, eligibility, placement, the launch and the C entry points.
#include "pointwise_bf16_wgrad_small.h"
#include "timing.h"

// A tier: tile rows of G and of X per x_mode, threads per workgroup, the kernel without / with the tail masks
struct WgTierDesc { int gr[2], xr[2]; unsigned threads; void (*kernel[2])(WgGroupParams); };
static const WgTierDesc kTiers[2] = {
    {{128, 256}, {256, 128}, 768, {pw_wgrad_group_kernel<false, WG_GROUP_RL>, pw_wgrad_group_kernel<true, WG_GROUP_RL>}},
    {{128, 128}, {128, 128}, 512, {pw_wgrad_group_small_kernel<false>, pw_wgrad_group_small_kernel<true>}}};

int pw_wgrad_group_tiles(WgTier tier, int M, int K, int x_mode) {
    const int GR = kTiers[tier].gr[x_mode ? 1 : 0], XR = kTiers[tier].xr[x_mode ? 1 : 0];
    return (M > 0 && K > 0 && M % GR == 0 && K % XR == 0) ? (M / GR) * (K / XR) : 0;
}

// the finished-gradient forms (G plain; X plain or relu6(xa x + xb)), whole tiles, a split count v100_pw_wgrad_io takes
int pw_wgrad_group_supported(WgTier tier, const WgGroupProblem& q) {
    const int B = q.B, M = q.M, K = q.K, T = q.T, S = q.S;
    if (B <= 0 || M <= 0 || K <= 0 || T <= 0 || S <= 0 || (S > B && (S % B != 0 || S / B > 64))) return 0;
    if (q.x_mode != PW_X_NONE && q.x_mode != PW_X_AFFINE_RELU6) return 0;
    if (!pw_wgrad_group_tiles(tier, M, K, q.x_mode)) return 0;
    const int P = pw_pitch16(T, B);
    return ((long)(M + 256) * P * 4 < 0x7fffffffL && (long)(K + 256) * P * 4 < 0x7fffffffL) ? 1 : 0;
}

// a problem's status in a list: a NULL operand comes before an unsupported shape (g_mode, io16: of the table form; every operand bf16-stored)
static int wg_check(WgTier tier, const WgGroupProblem& q, int g_mode, int io16) {
    if (!q.G || !q.X || !q.dW || (q.x_mode != PW_X_NONE && (!q.xa || !q.xb))) return V100_ERR_NULL;
    return g_mode == PW_X_NONE && io16 == (WG_IO_G | WG_IO_X) && pw_wgrad_group_supported(tier, q) ? V100_OK : V100_ERR_SHAPE;
}

// Placement and launch of g's checked problems: each goes to the emptiest XCD so far (the first of equals), its tiles in consecutive slots
static int wg_place_launch(WgTier tier, WgGroupParams& g, hipStream_t st) {
    int fill[8] = {0, 0, 0, 0, 0, 0, 0, 0};            // slots taken on each XCD
    bool tail = false;
    for (int i = 0; i < g.n; ++i) {
        WgGroupProblem& q = g.pr[i];
        q.ntiles = pw_wgrad_group_tiles(tier, q.M, q.K, q.x_mode);
        int x = 0;
        for (int c = 1; c < 8; ++c) if (fill[c] < fill[x]) x = c;
        q.xcd = x; q.slot0 = fill[x];
        fill[x] += q.ntiles;
        tail = tail || q.T % BF_BK != 0;
    }
    int slots = 0;
    for (int c = 0; c < 8; ++c) if (fill[c] > slots) slots = fill[c];
    V100TimedRegion timed(V100_T_PW_WGRAD, st);
    // (the tail form is right for whole steps too: its masks then never apply)
    V100_GGL(kTiers[tier].kernel[tail ? 1 : 0], dim3((unsigned)(8 * slots)), dim3(kTiers[tier].threads), 0, st, g);
    return v100_launch_status();
}

int pw_wgrad_group_launch(WgTier tier, int n, const WgGroupProblem* problems, hipStream_t stream) {
    if (!problems) return V100_ERR_NULL;
    if (n <= 0 || n > WG_GROUP_MAX) return V100_ERR_SHAPE;
    WgGroupParams g;
    g.n = n;
    for (int i = 0; i < n; ++i) {
        g.pr[i] = problems[i];
        if (int rc = wg_check(tier, g.pr[i], PW_X_NONE, WG_IO_G | WG_IO_X)) return rc;
    }
    return wg_place_launch(tier, g, stream);
}

// the table form of both C launchers.  ptrs (HOST, 5 per problem): G X xa xb dW; dims (HOST, 8 per problem): B M K T S g_mode x_mode io16
static int wg_table_launch(WgTier tier, int n, const void* const* ptrs, const int* dims, void* stream) {
    if (!ptrs || !dims) return V100_ERR_NULL;
    if (n <= 0 || n > WG_GROUP_MAX) return V100_ERR_SHAPE;
    WgGroupParams g;
    g.n = n;
    for (int i = 0; i < n; ++i) {
        const void* const* P = ptrs + 5 * i;
        const int* d = dims + 8 * i;
        g.pr[i] = WgGroupProblem{P[0], P[1], (const float*)P[2], (const float*)P[3], (float*)const_cast<void*>(P[4]), d[0], d[1], d[2], d[3], d[4], d[6], 0, 0, 0};
        if (int rc = wg_check(tier, g.pr[i], d[5], d[7])) return rc;
    }
    return wg_place_launch(tier, g, (hipStream_t)stream);
}
static int wg_supported(WgTier tier, int B, int M, int K, int T, int S, int g_mode, int x_mode, int io16) {
    const WgGroupProblem q{nullptr, nullptr, nullptr, nullptr, nullptr, B, M, K, T, S, x_mode, 0, 0, 0};
    return g_mode == PW_X_NONE && io16 == (WG_IO_G | WG_IO_X) && pw_wgrad_group_supported(tier, q);
}

// ---- the C entry points (include/voice100_hip.h): the wide tier, then the same three on 128 x 128 tiles ----
extern "C" int v100_pw_wgrad_group_supported(int B, int M, int K, int T, int S, int g_mode, int x_mode, int io16) {
    return wg_supported(WG_TIER_WIDE, B, M, K, T, S, g_mode, x_mode, io16);
}
extern "C" int v100_pw_wgrad_group_tiles(int M, int K, int x_mode) { return pw_wgrad_group_tiles(WG_TIER_WIDE, M, K, x_mode); }
extern "C" int v100_pw_wgrad_group(int n, const void* const* ptrs, const int* dims, void* stream) {
    return wg_table_launch(WG_TIER_WIDE, n, ptrs, dims, stream);
}
extern "C" int v100_pw_wgrad_group_small_supported(int B, int M, int K, int T, int S, int g_mode, int x_mode, int io16) {
    return wg_supported(WG_TIER_SMALL, B, M, K, T, S, g_mode, x_mode, io16);
}
extern "C" int v100_pw_wgrad_group_small_tiles(int M, int K, int x_mode) { return pw_wgrad_group_tiles(WG_TIER_SMALL, M, K, x_mode); }
extern "C" int v100_pw_wgrad_group_small(int n, const void* const* ptrs, const int* dims, void* stream) {
    return wg_table_launch(WG_TIER_SMALL, n, ptrs, dims, stream);
}
