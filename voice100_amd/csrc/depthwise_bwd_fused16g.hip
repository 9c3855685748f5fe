// Fused depthwise backward, every hidden tensor stored as bf16: dz2 and a2 in, a1 for the mask / xin, dz1 out.
#include "depthwise_common.h"
#include "depthwise_stream16.h"

// the kept-rows form of the streaming kernel (DA1, depthwise_stream16.h): one group, a wave's rows fit its 8 register slots
bool dw_bwd_da1_supported(int B, int C, int T, int K, int G) {
    static const bool on = [] { const char* e = getenv("V100_IR_DA1"); return !(e && e[0] == '0'); }();     // A/B switch
    // rows of 513 .. 768 outputs (time-stretched steps) cannot keep their rows (12 registers a row: the file is full): they keep dz1 + the
    // consumers' transform on load (DESIGN_rejected.md, "round 6 -- finished gradient da1 for time-stretched rows")
    if (!on || G != 1 || B > 32 || T > 512 || T < 1 || C < 1) return false;
#define X(KK) if (K == KK) return true;
    V100_DW_SPECIALISED(X)
#undef X
    return false;
}

bool dw_launch_bwd_fused16g(const DwParams& p, hipStream_t st, const V100TimedLaunch& tl) {
    // rows of up to 768 outputs: the streaming kernel
    if (p.stride == 1 && p.upsample == 1 && p.flip && p.Tin == p.Tout && p.Tin <= 768 &&
        p.pad == p.K - 1 - (p.K - 1) / 2) {
        const DwPathConfig cfg = dw_path_config();
        dim3 grid(p.C, p.G);
#define GO(KK, NTT)                                                                                                               \
    do {                                                                                                                          \
        if (p.da1) {                                                                                                              \
            if (p.fin.mode != 2 || p.G != 1 || p.B > 32 || p.Tin > 512) return false;                                             \
            V100_LAUNCH(tl, (dwconv_bwd16_stream_kernel<KK, NTT, DWS_KEEP_DEPTH, DWS_CP, 2, true>), grid, dim3(256), 0, st, p);   \
        } else if (p.Tin <= 512) V100_LAUNCH(tl, (dwconv_bwd16_stream_kernel<KK, NTT, DWS_DEPTH, DWS_CP, 2>), grid, dim3(256), 0, st, p);  \
        else V100_LAUNCH(tl, (dwconv_bwd16_stream_kernel<KK, NTT, DWS_DEPTH, DWS_CP, 3>), grid, dim3(256), 0, st, p);             \
    } while (0)
#define X(KK)                                                                                                                     \
    if (p.K == KK) {                                                                                                              \
        if (cfg.digits3) GO(KK, 3); else GO(KK, DW_DIGITS16);                                                                               \
        return true;                                                                                                              \
    }
        V100_DW_SPECIALISED(X)
#undef X
#undef GO
    }
    if (p.cm || p.da1) return false;      // the general kernel addresses [B][C][P] only (and has no kept-rows form)
    return dw_launch_specialised<DW_IN_AFFINE2, DW_OUT_MASK_STATS, true, DW_IO_X | DW_IO_X2 | DW_IO_AUX | DW_IO_Y>(p, st, tl);
}
