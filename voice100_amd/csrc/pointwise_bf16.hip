// bf16-operand instantiations of the pointwise GEMM kernels (see pointwise_common.h / pointwise.hip).
#include "pointwise_bf16_common.h"
#include "pointwise_bf16_gemm8.h"
#include "pointwise_bf16_ws.h"
#include "pointwise_bf16_wgrad.h"
#include "pointwise_bf16_ov.h"
#include "pointwise_bf16_sl.h"
#include "pointwise_bf16_wgrad_ws.h"
#include "pointwise_bf16_lat.h"

// ---------------------------------------------------------------------------------------------
// Dispatch: fast kernels (modes fixed at compile time, aligned K) for the combinations the networks
// use; everything else goes to the generic instantiation (run-time modes, scalar-safe loads).
#define PW_NN_COMBOS(X) X(0, 0) X(0, 1) X(1, 1) X(0, 2) X(0, 3) X(0, 4) X(2, 0) X(2, 5)
#define PW_WG_COMBOS(X) X(0, 0) X(0, 1) X(2, 0)

// fp16 operands (inference): the forward combinations only -- plain / bias (heads, ConvTranspose, dense conv), folded
// BN+ReLU6, folded BN(+residual).  false = this combination has no fp16 instantiation.
bool pw_launch_gemm_f16(const PwParams& p, dim3 grid, hipStream_t st) {
    if (p.x_mode != PW_X_NONE) return false;
    const bool tv = (p.T & 3) == 0, kv = (p.K & 7) == 0;
    const bool full = (p.K & 1) == 0 && (long)(p.K + 64) * p.T * 4 < 0x7fffffffL && (long)(p.M + 128) * p.K * 2 < 0x7fffffffL &&
                      (long)p.B * p.M * p.T * 4 < 0x7fffff00L;
    const bool big = full && p.M >= 256;
    PwParams pb = p;
    pb.n_mtiles = (p.M + 255) / 256;
    const dim3 gridb((unsigned)((long)pb.n_mtiles * p.n_ttiles * p.B));
#define X(EP)                                                                                                           \
    if (p.epi_mode == EP) {                                                                                             \
        if (big) V100_GGL((pw_gemm_bf16_fast_kernel<0, EP, 256, true>), gridb, dim3(512), 0, st, pb);        \
        else if (full) V100_GGL((pw_gemm_bf16_fast_kernel<0, EP, 128, true>), grid, dim3(256), 0, st, p);     \
        else if (tv && kv) V100_GGL((pw_gemm_bf16_kernel<0, EP, true, true, true>), grid, dim3(256), 0, st, p); \
        else V100_GGL((pw_gemm_bf16_kernel<0, EP, false, false, true>), grid, dim3(256), 0, st, p);           \
        return true;                                                                                                    \
    }
    X(0) X(2) X(3)
#undef X
    return false;
}

void pw_launch_gemm_bf16(const PwParams& p_in, dim3 grid_in, hipStream_t st) {
    const PwParams& p = p_in;
    const dim3 grid = grid_in;
    const bool tv = (p.T & 3) == 0, kv = (p.K & 7) == 0;
    // Any M, K, T: rows / columns past the tensor fall outside the buffer descriptors and read as zero; columns
    // t >= T inside a row read the next row's (finite) values, which only reach output columns that are never
    // stored; k >= K rows of X are zero, so whatever A holds there is multiplied by zero.
    const bool full = (p.K & 1) == 0 && (long)(p.K + 64) * p.T * 4 < 0x7fffffffL && (long)(p.M + 128) * p.K * 2 < 0x7fffffffL &&
                      (long)p.B * p.M * p.T * 4 < 0x7fffff00L;
    // 256-row block tile: half the X staging per flop.  (A/B in one process, tools/step_time.py: 128-row tiles everywhere cost
    // +0.2 ms of GEMM time per step; 128-row tiles only for the K <= 512 GEMMs -- two workgroups per CU, epilogue of one
    // over the main loop of the other -- measured equal, so one rule.)
    const bool big = full && p.M >= 256;
    if (full) {
        PwParams pb = p;                       // the 256-row tiling has its own m-tile count / grid
        pb.n_mtiles = (p.M + 255) / 256;
        const dim3 gridb((unsigned)((long)pb.n_mtiles * p.n_ttiles * p.B));
#define X(XM, EP)                                                                                                   \
        if (p.x_mode == XM && p.epi_mode == EP) {                                                                   \
            if (big) V100_GGL((pw_gemm_bf16_fast_kernel<XM, EP, 256>), gridb, dim3(512), 0, st, pb);     \
            else V100_GGL((pw_gemm_bf16_fast_kernel<XM, EP, 128>), grid, dim3(256), 0, st, p);            \
            return;                                                                                                 \
        }
        PW_NN_COMBOS(X)
#undef X
    }
    if (kv) {
#define X(XM, EP)                                                                                                   \
        if (p.x_mode == XM && p.epi_mode == EP) {                                                                   \
            if (tv) V100_GGL((pw_gemm_bf16_kernel<XM, EP, true, true>), grid, dim3(256), 0, st, p);          \
            else V100_GGL((pw_gemm_bf16_kernel<XM, EP, false, true>), grid, dim3(256), 0, st, p);            \
            return;                                                                                                 \
        }
        PW_NN_COMBOS(X)
#undef X
    }
    if (tv && kv) V100_GGL((pw_gemm_bf16_kernel<-1, -1, true, true>), grid, dim3(256), 0, st, p);
    else V100_GGL((pw_gemm_bf16_kernel<-1, -1, false, false>), grid, dim3(256), 0, st, p);
}

void pw_launch_wgrad_bf16(const WgParams& p, dim3 grid, hipStream_t st) {
    const bool tv = (p.T & 3) == 0;
    const bool full = (long)(p.M + 128) * p.T * 4 < 0x7fffffffL && (long)(p.K + 128) * p.T * 4 < 0x7fffffffL;
    if (full) {
#define X(GM, XM)                                                                                                   \
        if (p.g_mode == GM && p.x_mode == XM) {                                                                     \
            if (p.T % BF_BK == 0) V100_GGL((pw_wgrad_bf16_fast_kernel<GM, XM, false>), grid, dim3(256), 0, st, p); \
            else V100_GGL((pw_wgrad_bf16_fast_kernel<GM, XM, true>), grid, dim3(256), 0, st, p);          \
            return;                                                                                                 \
        }
        PW_WG_COMBOS(X)
#undef X
    }
#define X(GM, XM)                                                                                                   \
    if (p.g_mode == GM && p.x_mode == XM) {                                                                         \
        if (tv) V100_GGL((pw_wgrad_bf16_kernel<GM, XM, true>), grid, dim3(256), 0, st, p);                   \
        else V100_GGL((pw_wgrad_bf16_kernel<GM, XM, false>), grid, dim3(256), 0, st, p);                     \
        return;                                                                                                     \
    }
    PW_WG_COMBOS(X)
#undef X
    if (tv) V100_GGL((pw_wgrad_bf16_kernel<-1, -1, true>), grid, dim3(256), 0, st, p);
    else V100_GGL((pw_wgrad_bf16_kernel<-1, -1, false>), grid, dim3(256), 0, st, p);
}


static bool pw_launch_gemm_lat(const PwParams& p, hipStream_t st) {
    if (p.B != 1 || p.x_mode != 0 || p.bias || (p.M & 63) || (p.K & 63) || (p.T & 7) || p.K < 64) return false;
    if ((long)p.K * p.T * 4 >= 0x7fffffffL || (long)p.M * p.T * 4 >= 0x7fffffffL || (long)p.M * p.K * 2 >= 0x7fffffffL) return false;
    const long big_tiles = (long)((p.M + 255) / 256) * ((p.T + PW_BN - 1) / PW_BN);
    if (big_tiles > PW_LAT_MAXTILES) return false;
    const dim3 grid((unsigned)((p.M >> 6) * ((p.T + 63) >> 6)));
    const int f16 = p.io16 & PW_IO_F16, io = p.io16 & ~PW_IO_F16;
    if ((p.fmt == 2) != (f16 != 0)) return false;
    if (p.epi_mode == PW_EPI_AFFINE_RELU6 && io == PW_IO_Y) {
        if (f16) V100_GGL((pw_gemm_lat_kernel<PW_EPI_AFFINE_RELU6, true>), grid, dim3(256), 0, st, p);
        else V100_GGL((pw_gemm_lat_kernel<PW_EPI_AFFINE_RELU6, false>), grid, dim3(256), 0, st, p);
        return true;
    }
    if (p.epi_mode == PW_EPI_AFFINE_RES && io == PW_IO_X) {
        if (f16) V100_GGL((pw_gemm_lat_kernel<PW_EPI_AFFINE_RES, true>), grid, dim3(256), 0, st, p);
        else V100_GGL((pw_gemm_lat_kernel<PW_EPI_AFFINE_RES, false>), grid, dim3(256), 0, st, p);
        return true;
    }
    return false;
}

// 16-bit activation storage (PwParams::io16 / WgParams::io16): the combinations the block executor issues in "act16" mode.
// false = no instantiation for this (modes, mask) or the shape does not fit the buffer-addressed kernels.
bool pw_launch_gemm_bf16_io(const PwParams& p, hipStream_t st) {
    const int P = pw_pitch16(p.T, p.B);
    if (pw_launch_gemm_lat(p, st)) return true;
    if (p.io16 & PW_IO_F16) {
        // inference at precision "fp16" with fp16-stored hidden tensors: the two eval-mode GEMMs of a block (256-row tiles; 128 for M < 256)
        if (!((p.K & 1) == 0 && (long)(p.K + 64) * P * 4 < 0x7fffffffL && (long)(p.M + 128) * p.K * 2 < 0x7fffffffL &&
              (long)p.B * p.M * P * 4 < 0x7fffff00L && p.x_mode == 0)) return false;
        const bool big16 = p.M >= 256;
        PwParams pb = p;
        pb.n_mtiles = (p.M + (big16 ? 255 : 127)) / (big16 ? 256 : 128);
        const dim3 grid((unsigned)((long)pb.n_mtiles * p.n_ttiles * p.B));
#define XF(EP, IOV)                                                                                                                  \
        if (p.epi_mode == EP && p.io16 == (IOV)) {                                                                                  \
            if (big16) V100_GGL((pw_gemm_bf16_fast_kernel<0, EP, 256, true, false, (IOV)>), grid, dim3(512), 0, st, pb);            \
            else V100_GGL((pw_gemm_bf16_fast_kernel<0, EP, 128, true, false, (IOV)>), grid, dim3(256), 0, st, pb);                  \
            return true;                                                                                                            \
        }
        // the eval-mode project GEMM (fp16-stored h2 in, fp32 block output): the wave-specialised kernel, as at precision "bf16"
        if (big16 && p.epi_mode == 3 && p.io16 == (PW_IO_X | PW_IO_F16) && (p.K & 63) == 0 && p.K >= PW_WS_MINK && p.K <= WS_MAXK && (p.M & 255) == 0) {
            V100_GGL((pw_gemm_bf16_ws_kernel<0, 3, (PW_IO_X | PW_IO_F16)>), grid, dim3(768), 0, st, pb);
            return true;
        }
        XF(2, PW_IO_Y | PW_IO_F16) XF(3, PW_IO_X | PW_IO_F16)
#undef XF
        return false;
    }
    const bool big = p.M >= 256;
    PwParams pb = p;
    pb.n_mtiles = (p.M + (big ? 255 : 127)) / (big ? 256 : 128);
    const dim3 grid((unsigned)((long)pb.n_mtiles * p.n_ttiles * p.B));
#define X(XM, EP, IOV)                                                                                                          \
    if (p.x_mode == XM && p.epi_mode == EP && p.io16 == (IOV)) {                                                                \
        if (big) V100_GGL((pw_gemm_bf16_fast_kernel<XM, EP, 256, false, false, (IOV)>), grid, dim3(512), 0, st, pb);  \
        else V100_GGL((pw_gemm_bf16_fast_kernel<XM, EP, 128, false, false, (IOV)>), grid, dim3(256), 0, st, pb);      \
        return true;                                                                                                            \
    }
    // epilogue under the next tile's main loop: plain bf16 X, bf16 Y, whole 256-row tiles, K = 256 / 512, >= 2 tiles per workgroup
    if (big && p.x_mode == 0 && (p.K == 256 || p.K == 512) && (p.M & 255) == 0 && !p.bias && (long)p.B * p.K * P * 2 < 0x7fffffffL &&
        (long)p.B * p.M * P * 2 < 0x7ffffff0L) {
        const long nt_ = (long)pb.n_mtiles * p.n_ttiles * p.B;
        const unsigned gridp = 256;                    // one workgroup per CU walks tiles v = blockIdx.x, + 256, ... (any count)
        if (nt_ >= gridp) {
            // split-role kernel: only the mask epilogue (project backward-data) at K = 512; the other short-K shapes fall through
            if (p.epi_mode == 4 && p.io16 == (PW_IO_X | PW_IO_R | PW_IO_Y) && p.K == 512) {
                V100_GGL((pw_gemm_bf16_sl_kernel<4, 8>), dim3(gridp), dim3(768), 0, st, pb);
                return true;
            }
        }
        if (nt_ >= 2 * gridp) {
            if (p.epi_mode == 1 && p.io16 == (PW_IO_X | PW_IO_Y)) {
                if (p.K == 512) V100_GGL((pw_gemm_bf16_ov_kernel<1, (PW_IO_X | PW_IO_Y), 8>), dim3(gridp), dim3(512), 0, st, pb);
                else V100_GGL((pw_gemm_bf16_ov_kernel<1, (PW_IO_X | PW_IO_Y), 4>), dim3(gridp), dim3(512), 0, st, pb);
                return true;
            }
            if (p.epi_mode == 4 && p.io16 == (PW_IO_X | PW_IO_R | PW_IO_Y)) {
                if (p.K == 512) V100_GGL((pw_gemm_bf16_ov_kernel<4, (PW_IO_X | PW_IO_R | PW_IO_Y), 8>), dim3(gridp), dim3(512), 0, st, pb);
                else V100_GGL((pw_gemm_bf16_ov_kernel<4, (PW_IO_X | PW_IO_R | PW_IO_Y), 4>), dim3(gridp), dim3(512), 0, st, pb);
                return true;
            }
        }
    }
    // wave-specialised kernel: bf16-stored X operands, 256-row tiles, whole tiles in M (rows past M are handled by the epilogue)
#define XS(XM, EP, IOV)                                                                                                         \
    if (big && p.x_mode == XM && p.epi_mode == EP && p.io16 == (IOV) && (p.K & 63) == 0 && p.K >= PW_WS_MINK && p.K <= WS_MAXK && (p.M & 255) == 0) { \
        V100_GGL((pw_gemm_bf16_ws_kernel<XM, EP, (IOV)>), grid, dim3(768), 0, st, pb);                                           \
        return true;                                                                                                            \
    }
    XS(1, 1, PW_IO_X) XS(1, 1, PW_IO_X | PW_IO_Y)                       // project forward
    XS(2, 5, PW_IO_X | PW_IO_X2) XS(2, 0, PW_IO_X | PW_IO_X2)           // expand backward-data
    XS(0, 4, PW_IO_X | PW_IO_R | PW_IO_Y)                               // project backward-data
    XS(0, 1, PW_IO_X | PW_IO_Y)                                         // expand forward on the bf16 shadow
    XS(0, 3, PW_IO_X)                                                   // eval-mode project (K = the hidden width): y = bn3(W3 h2) (+ x)
    XS(0, 5, PW_IO_X) XS(0, 0, PW_IO_X)                                 // expand backward-data on the finished gradient da1 (round 5): plain bf16 X, fp32 dx (+ dy)
    XS(0, 5, PW_IO_X | PW_IO_R | PW_IO_Y) XS(0, 5, PW_IO_X | PW_IO_Y) XS(0, 5, PW_IO_X | PW_IO_R) XS(0, 0, PW_IO_X | PW_IO_Y)     // ... with the gradient stream between blocks in bf16 (round 6): dy in and / or dx out
#undef XS
    // short-K GEMMs with several tiles per CU: persistent workgroups (grid = tiles / 2 or / 4 when that divides evenly)
#define XP(XM, EP, IOV)                                                                                                         \
    if (big && p.x_mode == XM && p.epi_mode == EP && p.io16 == (IOV) && p.K <= 512) {                                           \
        const long nt_ = (long)pb.n_mtiles * p.n_ttiles * p.B;                                                                  \
        const long per = (nt_ % 1024 == 0 && nt_ >= 1024) ? 4 : ((nt_ % 512 == 0 && nt_ >= 512) ? 2 : 1);                       \
        if (per > 1) {                                                                                                          \
            V100_GGL((pw_gemm_bf16_fast_kernel<XM, EP, 256, false, false, (IOV), true>), dim3((unsigned)(nt_ / per)),  \
                               dim3(512), 0, st, pb);                                                                           \
            return true;                                                                                                        \
        }                                                                                                                       \
    }
    XP(0, 1, PW_IO_Y)          // expand forward: 61 -> 56.5 us at 2048 x 512 x (32 x 512)
    XP(0, 1, PW_IO_X | PW_IO_Y)    // ... reading the bf16 shadow of the block input (act16 level 4)
    // (the project backward-data GEMM, same shape, does not fit: its mask epilogue keeps 96 registers of R / coefficient /
    //  statistics values beside the two staging stages -- 59 VGPRs spilled, 69 -> 118 us)
#undef XP
    // project backward-data at K <= 256 (4 k-tiles per block tile: prologue and epilogue are most of a tile's time): 128-row tiles,
    // two workgroups per CU, so one's epilogue runs under the other's main loop (30.7 -> 27.5 us at 1024 x 256 x (32 x 512); the
    // expand forward GEMM of that shape loses, 23 -> 30 us: its fp32 X operand is then staged twice as often)
    if (p.x_mode == 0 && p.epi_mode == 4 && p.io16 == (PW_IO_X | PW_IO_R | PW_IO_Y) && p.K <= 256 && big) {
        PwParams ps = p;
        ps.n_mtiles = (p.M + 127) / 128;
        V100_GGL((pw_gemm_bf16_fast_kernel<0, 4, 128, false, false, (PW_IO_X | PW_IO_R | PW_IO_Y)>),
                           dim3((unsigned)((long)ps.n_mtiles * p.n_ttiles * p.B)), dim3(256), 0, st, ps);
        return true;
    }
    X(0, 1, PW_IO_Y)                      // expand forward: a1 out
    X(0, 1, PW_IO_X | PW_IO_Y)            // ... X = bf16 shadow of the block input
    X(1, 1, PW_IO_X)                      // project forward: a2 in (BN2 + ReLU6 on load)
    X(0, 4, PW_IO_R)                      // project backward-data: ReLU6 mask / BN2-backward sums from a2
    X(2, 5, PW_IO_X2) X(2, 0, PW_IO_X2)   // expand backward-data: BN1-backward affine of (dz1, a1)
    X(0, 4, PW_IO_R | PW_IO_Y)            // ... with the hidden gradients stored as bf16 too
    X(2, 5, PW_IO_X | PW_IO_X2) X(2, 0, PW_IO_X | PW_IO_X2)
    X(1, 1, PW_IO_X | PW_IO_Y)            // ... and the project output a3 / its gradient da3
    X(0, 4, PW_IO_X | PW_IO_R | PW_IO_Y)
    X(0, 2, PW_IO_Y)                      // eval-mode expand: h1 = relu6(bn1(W1 x)) stored as bf16 (inference, block executor)
    X(0, 3, PW_IO_X)                      // eval-mode project: y = bn3(W3 h2) (+ x), h2 bf16 in
    X(0, 5, PW_IO_X) X(0, 0, PW_IO_X)     // expand backward-data on da1 (plain bf16 X), fp32 out (+ residual gradient)
    X(0, 5, PW_IO_X | PW_IO_R | PW_IO_Y) X(0, 5, PW_IO_X | PW_IO_Y) X(0, 5, PW_IO_X | PW_IO_R) X(0, 0, PW_IO_X | PW_IO_Y)     // ... bf16 residual gradient in / bf16 dx out (the stack's 16-bit gradient stream)
#undef X
    return false;
}

bool pw_launch_wgrad_bf16_io(const WgParams& p, dim3 grid, hipStream_t st) {
    const int P = pw_pitch16(p.T, p.B);
    if (!((long)(p.M + 256) * P * 4 < 0x7fffffffL && (long)(p.K + 256) * P * 4 < 0x7fffffffL)) return false;
    // 256-row tile on the plain operand, 128 rows on the transformed one (pw_wgrad_bf16_wide_kernel)
#define XW(GM, XM, IOV, GR, XR, NS)                                                                                                    \
    if (p.g_mode == GM && p.x_mode == XM && p.io16 == (IOV) && p.M >= GR && p.K >= XR) {                                            \
        WgParams pw = p;                                                                                                            \
        pw.n_mtiles = (p.M + GR - 1) / GR;                                                                                          \
        pw.n_ktiles = (p.K + XR - 1) / XR;                                                                                          \
        const dim3 gw((unsigned)(pw.n_mtiles * pw.n_ktiles * p.S));                                                                 \
        if (p.T % BF_BK == 0) V100_GGL((pw_wgrad_bf16_wide_kernel<GM, XM, false, (IOV), GR, XR, NS>), gw, dim3(512), 0, st, pw); \
        else V100_GGL((pw_wgrad_bf16_wide_kernel<GM, XM, true, (IOV), GR, XR, NS>), gw, dim3(512), 0, st, pw);                \
        return true;                                                                                                                \
    }
    // wave-specialised form: full tiles, every operand bf16-stored
#define XS(GM, XM, IOV, GR, XR, NSW)                                                                                                  \
    if (p.g_mode == GM && p.x_mode == XM && p.io16 == (IOV) && p.M % GR == 0 && p.K % XR == 0) {                                    \
        WgParams pw = p;                                                                                                            \
        pw.n_mtiles = p.M / GR;                                                                                                     \
        pw.n_ktiles = p.K / XR;                                                                                                     \
        const dim3 gw((unsigned)(pw.n_mtiles * pw.n_ktiles * p.S));                                                                 \
        if (p.T % BF_BK == 0) V100_GGL((pw_wgrad_bf16_ws_kernel<GM, XM, false, (IOV), GR, XR, NSW>), gw, dim3(512 + 64 * NSW), 0, st, pw); \
        else V100_GGL((pw_wgrad_bf16_ws_kernel<GM, XM, true, (IOV), GR, XR, NSW>), gw, dim3(512 + 64 * NSW), 0, st, pw);        \
        return true;                                                                                                                \
    }
    // (measured, profiles/r03_ws_gemm.txt: the project gradient -13 % at 512 channels, the expand gradient -12 %; eight staging
    //  waves instead of four: slower)
    XS(2, 0, WG_IO_G | WG_IO_G2 | WG_IO_X, 128, 256, 4)      // expand gradient
    XS(0, 1, WG_IO_G | WG_IO_X, 256, 128, 4)                 // project gradient
    XS(0, 0, WG_IO_G | WG_IO_X, 128, 256, 4)                 // expand gradient on the finished gradient da1 (round 5)
#undef XS
    XW(2, 0, WG_IO_G | WG_IO_G2 | WG_IO_X, 128, 256, 2)      // ... X = bf16 shadow of the block input: copied as loaded, 32 registers a stage
    // (register staging 3: two stages for G + one for X; 1 = one stage, 2 = two for both: spills)
    XW(2, 0, WG_IO_G | WG_IO_G2, 128, 256, 3)      // expand: G = affine2(dz1, a1), X = block input (plain fp32)
    XW(0, 1, WG_IO_G | WG_IO_X, 256, 128, 2)       // project: G = da3 (plain bf16, copied), X = relu6(bn2(a2))
    XW(0, 0, WG_IO_G | WG_IO_X, 128, 256, 2)       // expand on da1: both operands plain bf16, copied as loaded
    XW(0, 0, WG_IO_G, 128, 256, 1)                 // ... X = the block input in fp32 (no shadow)
#undef XW
#define X(GM, XM, IOV)                                                                                                              \
    if (p.g_mode == GM && p.x_mode == XM && p.io16 == (IOV)) {                                                                      \
        if (p.T % BF_BK == 0) V100_GGL((pw_wgrad_bf16_fast_kernel<GM, XM, false, false, (IOV)>), grid, dim3(256), 0, st, p); \
        else V100_GGL((pw_wgrad_bf16_fast_kernel<GM, XM, true, false, (IOV)>), grid, dim3(256), 0, st, p);                \
        return true;                                                                                                                \
    }
    X(2, 0, WG_IO_G2)                     // expand backward-weight: G = BN1-backward affine of (dz1, a1), X = block input
    X(0, 1, WG_IO_X)                      // project backward-weight: X = relu6(bn2(a2))
    X(2, 0, WG_IO_G | WG_IO_G2)           // ... with dz1 stored as bf16
    X(2, 0, WG_IO_G | WG_IO_G2 | WG_IO_X) // ... and X = bf16 shadow of the block input
    X(0, 1, WG_IO_G | WG_IO_X)            // ... with da3 stored as bf16
    X(0, 0, WG_IO_G | WG_IO_X) X(0, 0, WG_IO_G)      // expand gradient on the finished gradient da1 (bf16), X = bf16 shadow / fp32
#undef X
    return false;
}

// Tap-addressed X operand (PwParams / WgParams): plain store (+bias) or +R epilogue, no prologues.  false = the shape
// does not fit the buffer-addressed kernels (the caller falls back to an explicit im2col copy).
bool pw_taps_fit_bf16(int B, int M, int cx, int ntap, int T, int Tx) {
    const long K = (long)ntap * cx;
    return cx % BF_BK == 0 && ntap >= 1 && ntap <= 8 && (long)(cx + 64) * Tx * 4 < 0x7fffff00L && (M + 128L) * K * 2 < 0x7fffffffL &&
           (long)B * M * T * 4 < 0x7fffff00L && (M + 128L) * Tx * 4 < 0x7fffff00L;
}

bool pw_launch_gemm_taps_bf16(const PwParams& p, dim3 grid, hipStream_t st) {
    if (!pw_taps_fit_bf16(p.B, p.M, p.cx, p.ntap, p.T, p.Tx)) return false;
    const bool big = p.M >= 256;
    PwParams pb = p;
    pb.n_mtiles = (p.M + 255) / 256;
    const dim3 gridb((unsigned)((long)pb.n_mtiles * p.n_ttiles * p.B));
#define X(EP, F16)                                                                                                      \
    if (p.epi_mode == EP && (p.fmt == 2) == F16) {                                                                      \
        if (big) V100_GGL((pw_gemm_bf16_fast_kernel<0, EP, 256, F16, true>), gridb, dim3(512), 0, st, pb);   \
        else V100_GGL((pw_gemm_bf16_fast_kernel<0, EP, 128, F16, true>), grid, dim3(256), 0, st, p);          \
        return true;                                                                                                    \
    }
    X(0, false) X(5, false) X(0, true)
#undef X
    return false;
}

bool pw_launch_wgrad_taps_bf16(const WgParams& p, dim3 grid, hipStream_t st) {
    if (!((p.M + 128L) * p.Tg * 4 < 0x7fffff00L && (p.cx + 128L) * p.Tx * 4 < 0x7fffff00L && p.ntap >= 1 && p.ntap <= 8)) return false;
    if (p.T % BF_BK == 0) V100_GGL((pw_wgrad_bf16_fast_kernel<0, 0, false, true>), grid, dim3(256), 0, st, p);
    else V100_GGL((pw_wgrad_bf16_fast_kernel<0, 0, true, true>), grid, dim3(256), 0, st, p);
    return true;
}
