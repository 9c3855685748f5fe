// The block executor's shape array and prepared-weights buffer: what block.hip (the executors) and pointwise.hip (the batched weight
// preparation) both need to know about an InvertedResidual block.  Host code only.
#pragma once
#include "common.h"
#include "../../include/voice100_hip.h"

// shape = {B, Cin, hid, Cout, T, K, stride, residual, bf16, flags ("prepped"), act16}
// act16 (bf16 operands only): 0 = every activation fp32; 1 = the two hidden tensors saved for backward, a1 and a2, are
// stored as bf16 [B][hid][pitch16(T)] (the caller allocates them so); 2 = also the hidden gradients dz2 / dz1 inside the
// backward workspace; 3 = also the project output a3 (saved for backward; the caller allocates it bf16 [B][cout][pitch16(T)])
// and its BatchNorm-backward gradient da3 (workspace).  Statistics and every accumulation stay fp32; only the stored copies are rounded.
enum { IR_B, IR_CIN, IR_HID, IR_COUT, IR_T, IR_K, IR_STRIDE, IR_RES, IR_BF16, IR_PREPPED, IR_ACT16, IR_NSHAPE };
// flag bits of shape[IR_PREPPED] that only the stack executor sets (the public three: V100_IR_*, voice100_hip.h)
enum { IR_F_NO_Y32 = 4, IR_F_DY16 = 16, IR_F_DX16 = 32, IR_F_DEFER = 64 };

// The EVAL entry points (v100_ir_eval_prep / v100_ir_fwd_eval / v100_ir_stack_fwd_eval) parse the nine leading ints only (IrShape::act16, the training
// level, stays 0) and read shape[IR_ACT16] as the storage of the two hidden tensors: fp32 rows, bf16 [B][hid][pitch16(T)] rows, or channel-major
enum IrEvalLayout { IR_EVAL_F32 = 0, IR_EVAL_ROWS16 = 1, IR_EVAL_CM = 2 };
inline IrEvalLayout ir_eval_layout(const int* sh) { return sh[IR_ACT16] == IR_EVAL_CM ? IR_EVAL_CM : sh[IR_ACT16] ? IR_EVAL_ROWS16 : IR_EVAL_F32; }
// A shape array parsed once.  ir_shape and ir_shape_ints are the only code that knows the flag bits.
struct IrShape {
    int B, cin, hid, cout, T, K, S, res, bf;     // bf: operand format, 0 fp32 / 1 bf16 (/ 2 fp16: inference only)
    int T2, pad, mc;                             // output length, depthwise padding, stride of the coefficient vectors
    int act16;
    bool prepped, shadows;      // the prepared weights are filled already; the pointer tables have the bf16-shadow slots x16 / y16
    bool frozen;                // BatchNorm on its running statistics (a block in eval() that takes part in autograd), fp32 storage only
    // set by the stack executor only: no_y32 = an interior block at level 5, nothing reads its fp32 output, only the shadow is written;
    // backward: dy arrives / dx leaves as bf16 [B][C][pitch16(T)]; defer = the two 1x1 weight gradients wait for its grouped launch
    bool no_y32, dy16, dx16, defer;
};
// flags = false: only the nine leading ints are read (the size helpers, whose callers may pass no more)
inline IrShape ir_shape(const int* sh, bool flags = true) {
    IrShape s{sh[IR_B], sh[IR_CIN], sh[IR_HID], sh[IR_COUT], sh[IR_T], sh[IR_K], sh[IR_STRIDE], sh[IR_RES], sh[IR_BF16]};
    s.pad = (s.K - 1) / 2; s.mc = s.hid > s.cout ? s.hid : s.cout;
    s.T2 = s.S ? (s.T + 2 * s.pad - s.K) / s.S + 1 : 0;          // (a stride of 0 is no valid shape; it must not divide here)
    if (!flags) return s;
    const int f = sh[IR_PREPPED];
    s.act16 = sh[IR_ACT16];
    s.prepped = f & V100_IR_PREPPED; s.shadows = f & V100_IR_SHADOW_SLOTS; s.frozen = f & V100_IR_FROZEN;
    s.no_y32 = f & IR_F_NO_Y32; s.dy16 = f & IR_F_DY16; s.dx16 = f & IR_F_DX16; s.defer = f & IR_F_DEFER;
    return s;
}
inline void ir_shape_ints(const IrShape& s, int* sh) {
    const int f = (s.prepped ? V100_IR_PREPPED : 0) | (s.shadows ? V100_IR_SHADOW_SLOTS : 0) | (s.frozen ? V100_IR_FROZEN : 0) |
                  (s.no_y32 ? IR_F_NO_Y32 : 0) | (s.dy16 ? IR_F_DY16 : 0) | (s.dx16 ? IR_F_DX16 : 0) | (s.defer ? IR_F_DEFER : 0);
    const int v[IR_NSHAPE] = {s.B, s.cin, s.hid, s.cout, s.T, s.K, s.S, s.res, s.bf, f, s.act16};
    for (int i = 0; i < IR_NSHAPE; ++i) sh[i] = v[i];
}

// a caller-owned blob handed out in 256-byte aligned pieces (base NULL: only the size is wanted)
struct Carver {
    char* p; size_t used;
    explicit Carver(void* base) : p((char*)base), used(0) {}
    template <class T> T* take(size_t n) {
        used = (used + 255) & ~size_t(255);
        T* r = p ? (T*)(p + used) : nullptr;
        used += n * sizeof(T);
        return r;
    }
};

// Prepared weights, written once by forward and reused by backward (caller-owned, saved with the block):
// bf16 mode: w1_bf [hid][cin], w1t_bf [cin][hid], w3_bf [cout][hid], w3t_bf [hid][cout];  fp32 mode: w1t, w3t (fp32).
struct IrPrep { void *w1bf, *w1tbf, *w3bf, *w3tbf; float *w1t, *w3t; };
inline size_t ir_prep_carve(const IrShape& s, void* base, IrPrep& w) {
    const size_t n1 = (size_t)s.hid * s.cin, n3 = (size_t)s.cout * s.hid;
    Carver c(base);
    w = IrPrep{};
    if (s.bf) { w.w1bf = c.take<u16>(n1); w.w1tbf = c.take<u16>(n1); w.w3bf = c.take<u16>(n3); w.w3tbf = c.take<u16>(n3); }
    else { w.w1t = c.take<float>(n1); w.w3t = c.take<float>(n3); }
    return c.used + 256;
}
