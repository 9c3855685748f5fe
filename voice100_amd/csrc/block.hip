// Block executor: one host call runs the whole kernel chain of an InvertedResidual block (voice100/models/asr.py:40-59) forward
// (training mode) or backward on the given stream, or (the stack executor, at the end of the file) of a run of consecutive blocks:
// ~12 (forward) / ~20 (backward) Python->C crossings per block become one.  Host code only, no kernel: it sequences the kernel entry
// points of this library (no allocation: the caller passes the outputs, the tensors saved for backward and ONE workspace blob that
// is carved here).  The extern "C" entry points only unpack their shape array (block_shape.h) and pointer table into IrShape and an
// argument struct; ir_fwd_train / ir_bwd / ir_eval_prep / ir_fwd_eval sequence the launches, and the stack executors call those themselves.
#include "common.h"
#include "../../include/voice100_hip.h"
#include "depthwise_common.h"   // DwFin / DwPre: BatchNorm finalisation inside the producing / the consuming kernel
#include "block_shape.h"
#include "wgrad_group.h"
#include <algorithm>
// With one depthwise group the depthwise kernels finalise the BatchNorms on both of their sides (forward BatchNorm 1 from the expand
// GEMM's slab, backward BatchNorm-2 backward from the project backward-data GEMM's slab): bit-identical results, 16 launches fewer,
// 3.30 -> 3.24 ms/step although the depthwise kernels themselves get slower (A/B on one box: profiles/r06_dw_ab.txt).

static inline size_t al256(size_t v) { return (v + 255) & ~size_t(255); }
static const float kMom = 0.1f, kEps = 1e-5f;
#define CK(call) do { rc = (call); if (rc) return rc; } while (0)

static inline int pitch16(int T, int B) { return v100_pitch16(T, B); }      // THE rule: common.h
// the row pitch (elements) of a 16-bit-stored [B][C][P] activation, for host code that allocates such tensors (functional.pitch16)
extern "C" int v100_row_pitch16(int T, int B) { return v100_pitch16(T, B); }
enum { PW_IO_X = 1, PW_IO_X2 = 2, PW_IO_Y = 4, PW_IO_R = 8, PW_IO_F16 = 16, WG_IO_G = 1, WG_IO_G2 = 2, WG_IO_X = 4 };   // DW_IO_*: depthwise_common.h

// A BatchNorm's five tensors (the running statistics are written in training mode), the four coefficient vectors forward leaves
// for backward, and the coefficient blob: 12 vectors, mc floats apart, s1 t1 mean1 rstd1 s2 t2 mean2 rstd2 s3 t3 mean3 rstd3
struct IrBn { const float *gamma, *beta; float *rm, *rv; long long* nbt; };
struct IrBnCoef { float *s, *t, *m, *r; };
struct IrCoef { IrBnCoef bn1, bn2, bn3; };
static IrCoef ir_coef(const float* coef, int mc) {
    float* c = const_cast<float*>(coef);          // (backward only reads it)
    return {{c, c + mc, c + 2 * mc, c + 3 * mc}, {c + 4 * mc, c + 5 * mc, c + 6 * mc, c + 7 * mc}, {c + 8 * mc, c + 9 * mc, c + 10 * mc, c + 11 * mc}};
}
// the 18 parameter / buffer slots of a block, as they stand in both public tables: w1 g1 b1 rm1 rv1 nbt1 | wd .. | w3 ..
struct IrParams { const float* w1; IrBn bn1; const float* wd; IrBn bn2; const float* w3; IrBn bn3; };
static IrParams ir_params(const void* const* t) {
    auto bn = [&](int j) { return IrBn{(const float*)t[j], (const float*)t[j + 1], (float*)t[j + 2], (float*)t[j + 3], (long long*)t[j + 4]}; };
    return {(const float*)t[0], bn(1), (const float*)t[6], bn(7), (const float*)t[12], bn(13)};
}
// The operands of one block, in the order of the public pointer tables.  a1 / a2 / a3 are bf16 where the act16 level says so;
// x16 / y16 are NULL unless the shape has the shadow slots, defer_region unless its weight gradients are deferred.
struct IrFwdArgs { const float* x; IrParams p; float *a1, *a2, *a3, *y, *coef; void *ws, *prep; const void* x16; void* y16; };
struct IrGrads { float *dW1, *dg1, *db1, *dWd, *dg2, *db2, *dW3, *dg3, *db3; };
struct IrBwdArgs {
    const float *x, *a1, *a2, *a3, *w1, *wd, *w3, *g1, *g2, *g3, *coef, *dy; float* dx; IrGrads g; void *ws, *prep; const void* x16; void* defer_region;
};
// THE order of a block's nine gradients in a flat buffer (v100_ir_stack_bwd's `grads`): views into g (NULL: sizes only), total floats
static size_t ir_grads_carve(const IrShape& s, float* g, IrGrads& o) {
    size_t off = 0, hid = s.hid, cout = s.cout, n[9] = {hid * s.cin, hid, hid, hid * s.K, hid, hid, cout * hid, cout, cout};
    float** const m[9] = {&o.dW1, &o.dg1, &o.db1, &o.dWd, &o.dg2, &o.db2, &o.dW3, &o.dg3, &o.db3};
    for (int j = 0; j < 9; ++j) { *m[j] = g ? g + off : nullptr; off += n[j]; }
    return off;
}
// The DwFin of a training-mode BatchNorm (forward: statistics -> scale / shift, saved mean / rstd, running statistics) and of a
// BatchNorm backward (sums -> p, q, r and dgamma, dbeta, from gamma and the saved mean / rstd)
static DwFin fin_train(double count, const IrBn& bn, const IrBnCoef& k) {
    return {1, count, bn.gamma, bn.beta, nullptr, k.s, k.t, nullptr, k.m, k.r, bn.rm, bn.rv, bn.nbt, kMom, kEps};
}
static DwFin fin_bwd(double count, const float* gamma, const IrBnCoef& k, float* p, float* q, float* r, float* dgamma, float* dbeta) {
    return {2, count, gamma, k.m, k.r, p, q, r, dgamma, dbeta, nullptr, nullptr, nullptr, 0.f, 0.f};
}

// 1 when a block of this shape can run with act16 != 0 (stride 1, a depthwise kernel size with an MFMA kernel, bf16 operands,
// tensors addressable by the buffer-descriptor kernels)
static int ir_act16_supported(const IrShape& s) {
    if (s.bf != 1 || s.S != 1 || !v100_dw_mfma_supported(s.K, s.S)) return 0;
    const long B = s.B, hid = s.hid, cin = s.cin, cout = s.cout, P = pitch16(s.T, s.B);
    if (hid % 2 || cin % 2 || cout % 2) return 0;
    if (B * hid * P * 4 >= 0x7fffff00L || (hid + 128) * P * 4 >= 0x7fffff00L || (hid + 128) * (cin > cout ? cin : cout) * 2 >= 0x7fffff00L) return 0;
    return 1;
}
extern "C" int v100_ir_act16_supported(const int* sh) { return sh ? ir_act16_supported(ir_shape(sh, false)) : 0; }

extern "C" long long v100_ir_prep_bytes(const int* shape) { IrPrep w; return (long long)ir_prep_carve(ir_shape(shape, false), nullptr, w); }
static size_t ir_fwd_carve(const IrShape& s, void* base, float** stats) {
    Carver c(base);         // one slab of per-channel partial sums, sized for the largest of the three BatchNorms
    *stats = c.take<float>(std::max({(size_t)v100_pw_num_parts(s.B, s.T) * s.hid * 2, (size_t)v100_dw_num_groups(s.B, s.hid) * s.hid * 2,
                                     (size_t)v100_pw_num_parts(s.B, s.T2) * s.cout * 2}));
    return c.used + 256;
}
extern "C" long long v100_ir_fwd_workspace_bytes(const int* shape) { float* s; return (long long)ir_fwd_carve(ir_shape(shape, false), nullptr, &s); }

static int ir_fwd_train(const IrShape& s, const IrFwdArgs& a, hipStream_t stream) {
    const int B = s.B, cin = s.cin, hid = s.hid, cout = s.cout, T = s.T, K = s.K, S = s.S, res = s.res, bf = s.bf, pad = s.pad, T2 = s.T2;
    if (bf != 0 && bf != 1) return V100_ERR_SHAPE;            // training: fp32 or bf16 operands (fp16 = inference only)
    const float *x = a.x, *w1 = a.p.w1, *wd = a.p.wd, *w3 = a.p.w3;
    float *a1 = a.a1, *a2 = a.a2, *a3 = a.a3, *y = a.y;
    const IrCoef c = ir_coef(a.coef, s.mc);
    float* st;
    IrPrep pw;
    ir_fwd_carve(s, a.ws, &st); ir_prep_carve(s, a.prep, pw);
    void *w1bf = pw.w1bf, *w3bf = pw.w3bf;
    int rc;
    // both orientations in one pass per weight: forward uses w*_bf, backward the transposed copies (skipped when the caller has
    // already filled `prep` for these weights, e.g. for every block of a stack in one v100_ir_prep_batched launch)
    if (!s.prepped) {
        CK(v100_weight_prep(w1, hid, cin, pw.w1bf, pw.w1t, pw.w1tbf, stream));
        CK(v100_weight_prep(w3, cout, hid, pw.w3bf, pw.w3t, pw.w3tbf, stream));
    }
    const int parts1 = v100_pw_num_parts(B, T), parts3 = v100_pw_num_parts(B, T2), G = v100_dw_num_groups(B, hid);
    // frozen: the same kernels with the running statistics in place of the batch's; fp32 storage only (no fused finaliser knows the mode)
    if (s.frozen && s.act16) return V100_ERR_SHAPE;
    auto finalize = [&](const float* stats, int parts, long long count, const IrBn& bn, const IrBnCoef& k, int C) -> int {
        if (s.frozen) return v100_bn_frozen_coeffs(bn.gamma, bn.beta, bn.rm, bn.rv, kEps, k.s, k.t, k.m, k.r, C, stream);
        return v100_bn_finalize_train(stats, parts, count, bn.gamma, bn.beta, bn.rm, bn.rv, bn.nbt, kMom, kEps, k.s, k.t, k.m, k.r, C, stream);
    };
    // BatchNorm 3 finalised by the block-output pass itself (one workgroup per channel)
    const DwPre pre3{fin_train((double)B * T2, a.p.bn3, c.bn3), st, parts3};
    if (s.act16) {
        if (!ir_act16_supported(s)) return V100_ERR_SHAPE;
        const void* x16 = (s.act16 >= 4 && s.shadows) ? a.x16 : nullptr;
        void* y16 = (s.act16 >= 4 && s.shadows) ? a.y16 : nullptr;
        if (x16) CK(v100_pw_gemm_io(w1bf, x16, nullptr, nullptr, nullptr, nullptr, 0, a1, nullptr, nullptr, nullptr, 1, st, B, hid, cin, T, PW_IO_X | PW_IO_Y, stream));
        else CK(v100_pw_gemm_io(w1bf, x, nullptr, nullptr, nullptr, nullptr, 0, a1, nullptr, nullptr, nullptr, 1, st, B, hid, cin, T, PW_IO_Y, stream));
        if (G == 1) {          // the depthwise kernel finalises BatchNorm 2 itself (its workgroup owns the channel's sums) ...
            const DwFin fin = fin_train((double)B * T2, a.p.bn2, c.bn2);
            // ... and BatchNorm 1 too, from the expand GEMM's slab, before its first row
            const DwPre pre{fin_train((double)B * T, a.p.bn1, c.bn1), st, parts1};
            CK(dw_fwd_train_io_fin(a1, wd, c.bn1.s, c.bn1.t, a2, st, G, B, hid, T, K, DW_IO_X | DW_IO_Y, fin, pre, stream));
        } else {
            CK(finalize(st, parts1, (long long)B * T, a.p.bn1, c.bn1, hid));
            CK(v100_dwconv_fwd_train_io(a1, wd, c.bn1.s, c.bn1.t, a2, st, G, B, hid, T, K, DW_IO_X | DW_IO_Y, stream));
            CK(finalize(st, G, (long long)B * T2, a.p.bn2, c.bn2, hid));
        }
        const bool a316 = s.act16 >= 3;          // the project output (saved for backward) as bf16 too
        CK(v100_pw_gemm_io(w3bf, a2, nullptr, c.bn2.s, c.bn2.t, nullptr, 1, a3, nullptr, nullptr, nullptr, 1, st, B, cout, hid, T2, PW_IO_X | (a316 ? PW_IO_Y : 0), stream));
        // level 5: the residual comes from the bf16 shadow of x (what the expand GEMM above read), and an interior block of a stack
        // (no_y32: nothing reads its fp32 output) writes only the shadow of its own output
        const bool r16 = s.act16 >= 5 && x16 && a316;            // (the previous block may not have written its fp32 output at all)
        const bool noy = s.act16 >= 5 && y16 && a316 && s.no_y32;
        CK(chan_affine2_fin(a3, res ? (r16 ? x16 : (const void*)x) : nullptr, noy ? nullptr : y, y16, B, cout, T2, a316 ? 1 : 0, pre3, stream, r16 ? 1 : 0));
        return V100_OK;
    }
    CK(v100_pw_gemm(w1, w1bf, x, nullptr, nullptr, nullptr, nullptr, 0, a1, nullptr, nullptr, nullptr, nullptr, 1, st, B, hid, cin, T, bf, stream));
    CK(finalize(st, parts1, (long long)B * T, a.p.bn1, c.bn1, hid));
    CK(v100_dwconv(a1, nullptr, wd, c.bn1.s, c.bn1.t, nullptr, 1, a2, nullptr, nullptr, nullptr, 0, st, G, B, hid, T, T2, K, S, pad, 0, 1, 0, stream));
    CK(finalize(st, G, (long long)B * T2, a.p.bn2, c.bn2, hid));
    CK(v100_pw_gemm(w3, w3bf, a2, nullptr, c.bn2.s, c.bn2.t, nullptr, 1, a3, nullptr, nullptr, nullptr, nullptr, 1, st, B, cout, hid, T2, bf, stream));
    // a block that itself keeps fp32 storage (the stride-2 first layer) still emits the shadow its successor reads: the caller
    // passes y16 only in bf16 precision at act16 level 4 (x16 / y16 are not read otherwise) -- and, like the 16-bit blocks, lets that
    // pass finalise BatchNorm 3 itself (one launch fewer per step)
    void* y16 = (bf == 1 && s.shadows) ? a.y16 : nullptr;
    if (!s.frozen && y16) {
        CK(chan_affine2_fin(a3, res ? x : nullptr, y, y16, B, cout, T2, 0, pre3, stream, 0));
        return V100_OK;
    }
    CK(finalize(st, parts3, (long long)B * T2, a.p.bn3, c.bn3, cout));
    if (y16) CK(v100_chan_affine2_shadow(a3, res ? x : nullptr, c.bn3.s, c.bn3.t, y, y16, B, cout, T2, 0, stream));
    else CK(v100_chan_affine2(a3, res ? x : nullptr, c.bn3.s, nullptr, c.bn3.t, y, B, cout, T2, stream));
    return V100_OK;
}
// ptrs: 0 x | 1 w1 2 g1 3 b1 4 rm1 5 rv1 6 nbt1 | 7 wd 8 g2 9 b2 10 rm2 11 rv2 12 nbt2 | 13 w3 14 g3 15 b3 16 rm3 17 rv3 18 nbt3 |
//       19 a1 20 a2 21 a3 22 y 23 coef 24 workspace 25 prepared-weights buffer (v100_ir_prep_bytes) | 26 x16 27 y16 (only in a table
//       with the shadow slots; each may be NULL): bf16 shadow [B][C][pitch16(T, B)] of x (by the previous block) / of y (for the next)
extern "C" int v100_ir_fwd_train(const int* sh, const void* const* P, void* stream) {
    if (!sh || !P) return V100_ERR_NULL;
    const IrShape s = ir_shape(sh);
    const IrFwdArgs a{(const float*)P[0], ir_params(P + 1), (float*)P[19], (float*)P[20], (float*)P[21], (float*)P[22], (float*)P[23],
                      const_cast<void*>(P[24]), const_cast<void*>(P[25]), s.shadows ? P[26] : nullptr, s.shadows ? const_cast<void*>(P[27]) : nullptr};
    return ir_fwd_train(s, a, (hipStream_t)stream);
}

struct IrBwdWs { float *part, *da3, *dz2, *dz1, *slab, *pqr; };
static size_t ir_bwd_carve(const IrShape& s, void* base, IrBwdWs& w) {
    const int B = s.B, cin = s.cin, hid = s.hid, cout = s.cout, T = s.T, K = s.K, T2 = s.T2;
    Carver c(base);
    w.part = c.take<float>(std::max({(size_t)v100_dw_num_groups(B, cout) * cout * 2, (size_t)v100_pw_num_parts(B, T2) * hid * 2,
                                     (size_t)v100_dw_num_groups(B, hid) * hid * 2}));
    w.da3 = s.act16 >= 3 ? (float*)c.take<u16>((size_t)B * cout * pitch16(T2, B)) : c.take<float>((size_t)B * cout * T2);
    // act16 == 2: the two hidden gradients are bf16 with pitched rows (half the bytes; the fp32 size is an upper bound
    // only when pitch16(T) <= 2*T, i.e. always)
    if (s.act16 >= 2) {
        w.dz2 = (float*)c.take<u16>((size_t)B * hid * pitch16(T2, B));
        w.dz1 = (float*)c.take<u16>((size_t)B * hid * pitch16(T, B));
    } else {
        w.dz2 = c.take<float>((size_t)B * hid * T2);
        w.dz1 = c.take<float>((size_t)B * hid * T);
    }
    w.slab = c.take<float>(std::max({(size_t)v100_pw_wgrad_splits(B, cout, hid) * cout * hid, (size_t)v100_pw_wgrad_splits(B, hid, cin) * hid * cin,
                                     (size_t)v100_dw_num_groups(B, hid) * hid * K}));
    w.pqr = c.take<float>((size_t)6 * s.mc);       // two coefficient sets (see fin_bwd in ir_bwd)
    return c.used + 256;
}

// ---- deferred weight gradients (stack executor).  A block on the finished-gradient path whose two 1x1 weight gradients are both
// grouped-launch problems of at least min_tiles tiles can leave them to a later grouped launch: their operands are then da3 and
// da1 (kept in a per-block region of the backward workspace), a2 and the block input's shadow (activation blob) and s2 / t2 (the
// block's coefficient blob) -- nothing the rest of the backward walk overwrites.
static size_t ir_defer_da3_bytes(const IrShape& s) { return al256((size_t)s.B * s.cout * pitch16(s.T2, s.B) * 2); }
static size_t ir_defer_bytes(const IrShape& s) { return ir_defer_da3_bytes(s) + al256((size_t)s.B * s.hid * pitch16(s.T, s.B) * 2); }
// (what decides that ir_bwd has finished da3 / da1 to park: everything but the gradients' tiles)
static bool ir_wgrad_defer_path(const IrShape& s, bool have_x16) {
    const int B = s.B, hid = s.hid, T = s.T, K = s.K;
    if (s.act16 < 4 || !s.shadows || s.frozen || !have_x16 || s.S != 1) return false;
    return ir_act16_supported(s) && v100_dw_num_groups(B, hid) == 1 && dw_bwd_da1_supported(B, hid, T, K, 1);
}
// THE two problems of a deferring block: q[0] the project gradient dW3 = da3 x relu6(s2 a2 + t2), q[1] the expand gradient
// dW1 = da1 x (shadow of the block input).  a NULL: the shapes alone (eligibility, tile counts)
static void ir_wgrad_problems(const IrShape& s, const IrBwdArgs* a, WgGroupProblem q[2]) {
    q[0] = WgGroupProblem{nullptr, nullptr, nullptr, nullptr, nullptr, s.B, s.cout, s.hid, s.T, v100_pw_wgrad_splits(s.B, s.cout, s.hid), 1, 0, 0, 0};
    q[1] = WgGroupProblem{nullptr, nullptr, nullptr, nullptr, nullptr, s.B, s.hid, s.cin, s.T, v100_pw_wgrad_splits(s.B, s.hid, s.cin), 0, 0, 0, 0};
    if (!a) return;
    const IrBnCoef bn2 = ir_coef(a->coef, s.mc).bn2;
    q[0].G = a->defer_region; q[0].X = a->a2; q[0].xa = bn2.s; q[0].xb = bn2.t; q[0].dW = a->g.dW3;
    q[1].G = (char*)a->defer_region + ir_defer_da3_bytes(s); q[1].X = a->x16; q[1].dW = a->g.dW1;
}
static int ir_wgrad_defer_tiles(const IrShape& s, WgTier tier) {      // of both gradients
    WgGroupProblem q[2];
    ir_wgrad_problems(s, nullptr, q);
    return pw_wgrad_group_tiles(tier, q[0].M, q[0].K, q[0].x_mode) + pw_wgrad_group_tiles(tier, q[1].M, q[1].K, q[1].x_mode);
}
// both gradients are problems of the tier's launch, of at least min_tiles tiles each (tier 2 has no minimum: it takes what is
// below tier 1's)
static bool ir_wgrad_defer_ok(const IrShape& s, bool have_x16, WgTier tier, int min_tiles) {
    if (!ir_wgrad_defer_path(s, have_x16)) return false;
    WgGroupProblem q[2];
    ir_wgrad_problems(s, nullptr, q);
    for (const WgGroupProblem& p : q)
        if (!pw_wgrad_group_supported(tier, p) || pw_wgrad_group_tiles(tier, p.M, p.K, p.x_mode) < min_tiles) return false;
    return true;
}

extern "C" long long v100_ir_bwd_workspace_bytes(const int* shape) {
    IrBwdWs w;
    IrShape s = ir_shape(shape, false);      // (+ the one field behind the nine that the carve reads)
    s.act16 = shape[IR_ACT16];
    return (long long)ir_bwd_carve(s, nullptr, w);
}

static int ir_bwd(const IrShape& s, const IrBwdArgs& a, hipStream_t stream) {
    const int B = s.B, cin = s.cin, hid = s.hid, cout = s.cout, T = s.T, K = s.K, S = s.S, res = s.res, bf = s.bf, pad = s.pad, T2 = s.T2, mc = s.mc;
    const float *x = a.x, *a1 = a.a1, *a2 = a.a2, *a3 = a.a3, *wd = a.wd, *g1 = a.g1, *g2 = a.g2, *g3 = a.g3, *dy = a.dy;
    const IrCoef c = ir_coef(a.coef, mc);
    const float *s1 = c.bn1.s, *t1 = c.bn1.t, *s2 = c.bn2.s, *t2 = c.bn2.t;
    float* dx = a.dx;
    // the gradient stream between the blocks of a stack in the 16-bit form its forward stream has at level 5 (grad16_ok)
    const int dy16 = s.dy16 ? 1 : 0, dx16 = s.dx16 ? 1 : 0;
    IrBwdWs w;
    ir_bwd_carve(s, a.ws, w);
    // defer (ir_wgrad_defer_ok): the two 1x1 weight gradients are NOT launched here -- the stack executor runs them later, grouped with
    // other blocks' -- so their G operands da3 and da1 go to the block's own region (da3, then da1 at ir_defer_da3_bytes), which outlives this call
    const bool defer = s.defer;
    if (defer) {
        if (!a.defer_region) return V100_ERR_NULL;
        if (s.act16 < 4) return V100_ERR_SHAPE;
        w.da3 = (float*)a.defer_region;
        w.dz1 = (float*)((char*)a.defer_region + ir_defer_da3_bytes(s));
    }
    float *pp = w.pqr, *qq = w.pqr + mc, *rr = w.pqr + 2 * mc;
    int rc;
    IrPrep pw;
    ir_prep_carve(s, a.prep, pw);
    const bool frozen = s.frozen;     // frozen BatchNorm statistics (see ir_fwd_train): q = r = 0 in every coefficient set
    if (frozen && s.act16) return V100_ERR_SHAPE;
    auto bwd_finalize = frozen ? v100_bn_bwd_finalize_frozen : v100_bn_bwd_finalize;
    // BN3 backward
    const int Gr = v100_dw_num_groups(B, cout);
    const bool a316 = s.act16 >= 3;              // a3 (saved) and da3 (workspace) stored as bf16
    bool da3_done = false;
    if (a316) {     // one workgroup per channel sums (dy, dy * a3) and finalises BatchNorm 3's backward itself ...
        const DwFin fin = fin_bwd((double)B * T2, g3, c.bn3, pp, qq, rr, a.g.dg3, a.g.db3);
        // ... and, when the channel's samples fit its registers, applies the affine to them in the same launch
        if (chan_bn3_bwd(dy, a3, w.part, w.da3, B, cout, T2, fin, stream, dy16)) {
            if ((rc = v100_launch_status()) != V100_OK) return rc;
            da3_done = true;
        } else if (dy16) return V100_ERR_SHAPE;           // (the stack executor asks for a 16-bit dy only where the one-pass kernel applies)
        else CK(chan_reduce2_io_fin(dy, a3, w.part, B, cout, T2, fin, stream));
    } else {
        if (dy16) return V100_ERR_SHAPE;
        CK(v100_chan_reduce2(dy, a3, w.part, Gr, B, cout, T2, stream));
        CK(bwd_finalize(w.part, Gr, (long long)B * T2, g3, c.bn3.m, c.bn3.r, pp, qq, rr, a.g.dg3, a.g.db3, cout, stream));
    }
    if (da3_done) {}
    else if (a316) CK(v100_chan_affine2_io(dy, a3, pp, qq, rr, w.da3, B, cout, T2, 6, stream));
    else CK(v100_chan_affine2(dy, a3, pp, qq, rr, w.da3, B, cout, T2, stream));
    if (s.act16) {
        if (!ir_act16_supported(s)) return V100_ERR_SHAPE;
        const bool g16 = s.act16 >= 2;
        if (!defer)
            CK(v100_pw_wgrad_io(w.da3, nullptr, nullptr, nullptr, nullptr, 0, a2, s2, t2, 1, w.slab, a.g.dW3, v100_pw_wgrad_splits(B, cout, hid),
                                B, cout, hid, T2, WG_IO_X | (a316 ? WG_IO_G : 0), stream));
        const int parts16 = v100_pw_num_parts(B, T2);
        CK(v100_pw_gemm_io(pw.w3tbf, w.da3, nullptr, nullptr, nullptr, nullptr, 0, w.dz2, s2, t2, a2, 4, w.part, B, hid, cout, T2,
                           PW_IO_R | (g16 ? PW_IO_Y : 0) | (a316 ? PW_IO_X : 0), stream));
        const int G16 = v100_dw_num_groups(B, hid);
        bool da1 = false;
        if (G16 == 1) {        // BatchNorm-1 backward coefficients by the depthwise backward kernel itself
            // p / q / r are INPUTS of this kernel (BatchNorm-2 backward) and outputs of its finalisation (BatchNorm-1 backward):
            // the outputs go to the second coefficient set
            float *pp2 = w.pqr + 3 * mc, *qq2 = w.pqr + 4 * mc, *rr2 = w.pqr + 5 * mc;
            const DwFin fin = fin_bwd((double)B * T, g1, c.bn1, pp2, qq2, rr2, a.g.dg1, a.g.db1);
            // (BatchNorm-2 backward coefficients: from the GEMM's slab, by the depthwise kernel too)
            const DwPre pre{fin_bwd((double)B * T2, g2, c.bn2, pp, qq, rr, a.g.dg2, a.g.db2), w.part, parts16};
            // Round 5: where the streaming kernel can keep a wave's rows in registers (one group, B <= 32, every hidden tensor bf16) it
            // writes the FINISHED gradient da1 = p dz1 + q a1 + r (into the dz1 buffer) and the two consumers below read ONE plain
            // bf16 tensor -- bit for bit the operand their on-load transform of (dz1, a1) produced.
            da1 = g16 && !frozen && dw_bwd_da1_supported(B, hid, T, K, G16);
            CK(dw_bwd_io_fin(w.dz2, a2, wd, pp, qq, rr, a1, s1, t1, w.dz1, w.part, w.slab, a.g.dWd, G16, B, hid, T, K,
                             g16 ? (DW_IO_X | DW_IO_X2 | DW_IO_AUX | DW_IO_Y) : (DW_IO_X2 | DW_IO_AUX), fin, pre, stream, da1 ? 1 : 0));
            pp = pp2; qq = qq2; rr = rr2;
        } else {
            CK(v100_bn_bwd_finalize(w.part, parts16, (long long)B * T2, g2, c.bn2.m, c.bn2.r, pp, qq, rr, a.g.dg2, a.g.db2, hid, stream));
            CK(v100_dwconv_bwd_io(w.dz2, a2, wd, pp, qq, rr, a1, s1, t1, w.dz1, w.part, w.slab, a.g.dWd, G16, B, hid, T, K,
                                  g16 ? (DW_IO_X | DW_IO_X2 | DW_IO_AUX | DW_IO_Y) : (DW_IO_X2 | DW_IO_AUX), stream));
            CK(v100_bn_bwd_finalize(w.part, G16, (long long)B * T, g1, c.bn1.m, c.bn1.r, pp, qq, rr, a.g.dg1, a.g.db1, hid, stream));
        }
        const void* x16 = (s.act16 >= 4 && s.shadows) ? a.x16 : nullptr;
        if (defer && !(da1 && x16)) return V100_ERR_SHAPE;   // (cannot happen: ir_wgrad_defer_ok tests what decides this path)
        if (da1) {
            if (!defer)
                CK(v100_pw_wgrad_io(w.dz1, nullptr, nullptr, nullptr, nullptr, 0, x16 ? x16 : (const void*)x, nullptr, nullptr, 0, w.slab, a.g.dW1,
                                    v100_pw_wgrad_splits(B, hid, cin), B, hid, cin, T, WG_IO_G | (x16 ? WG_IO_X : 0), stream));
            if (dx)
                CK(v100_pw_gemm_io(pw.w1tbf, w.dz1, nullptr, nullptr, nullptr, nullptr, 0, dx, nullptr, nullptr, res ? dy : nullptr, res ? 5 : 0, nullptr,
                                   B, cin, hid, T, PW_IO_X | ((dy16 && res) ? PW_IO_R : 0) | (dx16 ? PW_IO_Y : 0), stream));
            return V100_OK;
        }
        if (dy16 || dx16) return V100_ERR_SHAPE;
        CK(v100_pw_wgrad_io(w.dz1, a1, pp, qq, rr, 2, x16 ? x16 : (const void*)x, nullptr, nullptr, 0, w.slab, a.g.dW1, v100_pw_wgrad_splits(B, hid, cin),
                            B, hid, cin, T, WG_IO_G2 | (g16 ? WG_IO_G : 0) | (x16 ? WG_IO_X : 0), stream));
        if (dx)
            CK(v100_pw_gemm_io(pw.w1tbf, w.dz1, a1, pp, qq, rr, 2, dx, nullptr, nullptr, res ? dy : nullptr, res ? 5 : 0, nullptr,
                               B, cin, hid, T, PW_IO_X2 | (g16 ? PW_IO_X : 0), stream));
        return V100_OK;
    }
    if (dy16 || dx16) return V100_ERR_SHAPE;
    // pw-linear: weight grad, then data grad through ReLU6 with BN2-backward sums
    CK(v100_pw_wgrad(w.da3, nullptr, nullptr, nullptr, nullptr, 0, a2, s2, t2, 1, w.slab, a.g.dW3, v100_pw_wgrad_splits(B, cout, hid),
                     B, cout, hid, T2, bf, stream));
    const int parts = v100_pw_num_parts(B, T2);
    CK(v100_pw_gemm(pw.w3t, pw.w3tbf, w.da3, nullptr, nullptr, nullptr, nullptr, 0, w.dz2, nullptr, s2, t2, a2, 4, w.part, B, hid, cout, T2, bf, stream));
    CK(bwd_finalize(w.part, parts, (long long)B * T2, g2, c.bn2.m, c.bn2.r, pp, qq, rr, a.g.dg2, a.g.db2, hid, stream));
    // depthwise: weight grad, then data grad through ReLU6 with BN1-backward sums
    const int G = v100_dw_num_groups(B, hid);
    CK(v100_dwconv_bwd(w.dz2, a2, wd, pp, qq, rr, a1, s1, t1, w.dz1, w.part, w.slab, a.g.dWd, G, B, hid, T, T2, K, S, pad, 0, stream));
    CK(bwd_finalize(w.part, G, (long long)B * T, g1, c.bn1.m, c.bn1.r, pp, qq, rr, a.g.dg1, a.g.db1, hid, stream));
    // pw: weight grad, data grad (+ residual)
    CK(v100_pw_wgrad(w.dz1, a1, pp, qq, rr, 2, x, nullptr, nullptr, 0, w.slab, a.g.dW1, v100_pw_wgrad_splits(B, hid, cin),
                     B, hid, cin, T, bf, stream));
    if (dx)
        CK(v100_pw_gemm(pw.w1t, pw.w1tbf, w.dz1, a1, pp, qq, rr, 2, dx, nullptr, nullptr, nullptr, res ? dy : nullptr, res ? 5 : 0, nullptr,
                        B, cin, hid, T, bf, stream));
    return V100_OK;
}
// ptrs: 0 x 1 a1 2 a2 3 a3 | 4 w1 5 wd 6 w3 | 7 g1 8 g2 9 g3 | 10 coef | 11 dy | 12 dx (may be NULL) |
//       13 dW1 14 dg1 15 db1 16 dWd 17 dg2 18 db2 19 dW3 20 dg3 21 db3 | 22 workspace | 23 prepared weights (from forward)
//       24 x16 (only in a table with the shadow slots; may be NULL): the shadow of x the forward read | 25 (only with defer) da3 / da1 region
extern "C" int v100_ir_bwd(const int* sh, const void* const* P, void* stream) {
    if (!sh || !P) return V100_ERR_NULL;
    const IrShape s = ir_shape(sh);
    auto f = [&](int j) { return (float*)P[j]; };
    const IrBwdArgs a{f(0), f(1), f(2), f(3), f(4), f(5), f(6), f(7), f(8), f(9), f(10), f(11), f(12),
                      {f(13), f(14), f(15), f(16), f(17), f(18), f(19), f(20), f(21)}, const_cast<void*>(P[22]), const_cast<void*>(P[23]),
                      s.shadows ? P[24] : nullptr, s.defer ? const_cast<void*>(P[25]) : nullptr};
    return ir_bwd(s, a, (hipStream_t)stream);
}

// ---- eval mode: BatchNorm folded to per-channel scale/shift inside three kernels (pw+BN+ReLU6, dw+BN+ReLU6, pw+BN(+x)).
// The folded coefficients and the bf16 weight copies only change when the parameters do, so they live in a caller-owned
// cache filled by v100_ir_eval_prep; a forward is then 3 launches from one call.  (shape[IR_ACT16] here: IrEvalLayout, block_shape.h)
struct IrEvalCache { void *w1bf, *w3bf; float *s1, *t1, *s2, *t2, *s3, *t3; };
static size_t ir_eval_carve(const IrShape& s, void* base, IrEvalCache& w) {
    Carver c(base);
    w.w1bf = w.w3bf = nullptr;
    if (s.bf) { w.w1bf = c.take<u16>((size_t)s.hid * s.cin); w.w3bf = c.take<u16>((size_t)s.cout * s.hid); }
    w.s1 = c.take<float>(s.hid); w.t1 = c.take<float>(s.hid); w.s2 = c.take<float>(s.hid); w.t2 = c.take<float>(s.hid);
    w.s3 = c.take<float>(s.cout); w.t3 = c.take<float>(s.cout);
    return c.used + 256;
}
extern "C" long long v100_ir_eval_cache_bytes(const int* shape) { IrEvalCache w; return (long long)ir_eval_carve(ir_shape(shape, false), nullptr, w); }
// v100_ir_eval_prep's table (15): w1 | g1 b1 rm1 rv1 | g2 b2 rm2 rv2 | w3 | g3 b3 rm3 rv3 | cache
struct IrEvalBn { const float *gamma, *beta, *rm, *rv; };
struct IrEvalParams { const float* w1; IrEvalBn bn1, bn2; const float* w3; IrEvalBn bn3; };
static IrEvalParams ir_eval_params(const void* const* t) {
    auto bn = [&](int j) { return IrEvalBn{(const float*)t[j], (const float*)t[j + 1], (const float*)t[j + 2], (const float*)t[j + 3]}; };
    return {(const float*)t[0], bn(1), bn(5), (const float*)t[9], bn(10)};
}
// v100_ir_fwd_eval's table (8): x | w1 wd w3 | cache | h1 [B,hid,T] h2 [B,hid,T2] y [B,cout,T2] (the 16-bit layouts of h1 / h2: ir_fwd_eval)
struct IrEvalArgs { const float *x, *w1, *wd, *w3; void* cache; float *h1, *h2, *y; };
static IrEvalArgs ir_eval_args(const void* const* t) {
    return {(const float*)t[0], (const float*)t[1], (const float*)t[2], (const float*)t[3], const_cast<void*>(t[4]), (float*)t[5], (float*)t[6], (float*)t[7]};
}
static int ir_eval_prep(const IrShape& s, const IrEvalParams& p, void* cache, hipStream_t stream) {
    IrEvalCache c; ir_eval_carve(s, cache, c);
    int rc;
    if (s.bf == 2) {                                   // fp16 operands
        CK(v100_weight_prep_f16(p.w1, s.hid, s.cin, c.w1bf, stream));
        CK(v100_weight_prep_f16(p.w3, s.cout, s.hid, c.w3bf, stream));
    } else if (s.bf) {
        CK(v100_weight_prep(p.w1, s.hid, s.cin, c.w1bf, nullptr, nullptr, stream));
        CK(v100_weight_prep(p.w3, s.cout, s.hid, c.w3bf, nullptr, nullptr, stream));
    }
    CK(v100_bn_eval_coeffs(p.bn1.gamma, p.bn1.beta, p.bn1.rm, p.bn1.rv, kEps, c.s1, c.t1, s.hid, stream));
    CK(v100_bn_eval_coeffs(p.bn2.gamma, p.bn2.beta, p.bn2.rm, p.bn2.rv, kEps, c.s2, c.t2, s.hid, stream));
    CK(v100_bn_eval_coeffs(p.bn3.gamma, p.bn3.beta, p.bn3.rm, p.bn3.rv, kEps, c.s3, c.t3, s.cout, stream));
    return V100_OK;
}
extern "C" int v100_ir_eval_prep(const int* sh, const void* const* P, void* stream) {
    if (!sh || !P) return V100_ERR_NULL;
    return ir_eval_prep(ir_shape(sh, false), ir_eval_params(P), const_cast<void*>(P[14]), (hipStream_t)stream);
}
static int ir_fwd_eval(const IrShape& s, IrEvalLayout layout, const IrEvalArgs& a, hipStream_t stream) {
    const int B = s.B, cin = s.cin, hid = s.hid, cout = s.cout, T = s.T, K = s.K, S = s.S, bf = s.bf, T2 = s.T2;
    const float *x = a.x, *r = s.res ? a.x : nullptr;
    IrEvalCache c; ir_eval_carve(s, a.cache, c);
    int rc;
    if (layout != IR_EVAL_F32) {
        // 16-BIT ROWS (precision "bf16"): the two hidden tensors (each 4x the block's width, already BatchNorm'ed and clamped to [0, 6])
        // are stored as bf16 [B][hid][pitch16(T)] -- half the bytes of the three kernels' big streams; the GEMMs round them to bf16 as
        // operands anyway.  Same three launches.
        // CHANNEL-MAJOR (round 4): x [cin][B P] fp32, h1 / h2 [hid][B P] 16-bit, y [cout][B P] fp32, P = pitch16(T) -- every
        // utterance of the batch back to back in ONE [C x (B P)] matrix.  The two 1x1 convolutions are then ONE GEMM over all B P columns
        // (1-second chunks, T' = 51: 128-column tiles are full instead of 40 % full), a channel's rows are contiguous for the depthwise
        // kernel (the order it walks them in), short rows are packed several to a wave item.  The columns T .. P-1 of an utterance are
        // padding: finite garbage that no valid column ever reads (GEMM columns are independent; the depthwise kernel masks them).
        // Hidden tensors in the GEMMs' operand format: bf16, or fp16 at precision "fp16" (held to the shape rules of its bf16 twin).
        const bool cm = layout == IR_EVAL_CM;
        IrShape twin = s; twin.bf = 1;
        if ((cm ? (bf != 1 && bf != 2) || S != 1 || T > 768 : bf != 1) || !ir_act16_supported(twin)) return V100_ERR_SHAPE;
        const long long N = (long long)B * pitch16(T, B);
        if (cm && N > 0x7fffff00LL) return V100_ERR_SHAPE;
        const int nb = cm ? 1 : B, n1 = cm ? (int)N : T, n2 = cm ? (int)N : T2, f16 = bf == 2 ? PW_IO_F16 : 0;     // (rows: bf == 1)
        CK(v100_pw_gemm_io(c.w1bf, x, nullptr, nullptr, nullptr, nullptr, 0, a.h1, c.s1, c.t1, nullptr, 2, nullptr, nb, hid, cin, n1, PW_IO_Y | f16, stream));
        CK(dw_fwd_eval_io(a.h1, a.wd, c.s2, c.t2, a.h2, B, hid, T, K, stream, cm, bf == 2));
        CK(v100_pw_gemm_io(c.w3bf, a.h2, nullptr, nullptr, nullptr, nullptr, 0, a.y, c.s3, c.t3, r, 3, nullptr, nb, cout, hid, n2, PW_IO_X | f16, stream));
        return V100_OK;
    }
    CK(v100_pw_gemm(a.w1, c.w1bf, x, nullptr, nullptr, nullptr, nullptr, 0, a.h1, nullptr, c.s1, c.t1, nullptr, 2, nullptr, B, hid, cin, T, bf, stream));
    CK(v100_dwconv(a.h1, nullptr, a.wd, nullptr, nullptr, nullptr, 0, a.h2, nullptr, c.s2, c.t2, 1, nullptr, v100_dw_num_groups(B, hid),
                   B, hid, T, T2, K, S, s.pad, 0, 1, 0, stream));
    CK(v100_pw_gemm(a.w3, c.w3bf, a.h2, nullptr, nullptr, nullptr, nullptr, 0, a.y, nullptr, c.s3, c.t3, r, 3, nullptr, B, cout, hid, T2, bf, stream));
    return V100_OK;
}
extern "C" int v100_ir_fwd_eval(const int* sh, const void* const* P, void* stream) {
    if (!sh || !P) return V100_ERR_NULL;
    return ir_fwd_eval(ir_shape(sh, false), ir_eval_layout(sh), ir_eval_args(P), (hipStream_t)stream);
}
extern "C" int v100_ir_stack_fwd_eval(int n, const int* shapes, const void* const* ptrs, void* stream) {
    if (!shapes || !ptrs) return V100_ERR_NULL;
    if (n < 0) return V100_ERR_SHAPE;
    int rc;
    for (int i = 0; i < n; ++i, shapes += IR_NSHAPE, ptrs += 8)
        CK(ir_fwd_eval(ir_shape(shapes, false), ir_eval_layout(shapes), ir_eval_args(ptrs), (hipStream_t)stream));
    return V100_OK;
}

// =====================================================================================================================
// Stack executor: ONE host call per direction for a run of consecutive InvertedResidual blocks (the encoder's nine, a decoder
// segment's three or four): the per-block Python -> autograd -> ctypes crossings were 2/3 of the 3 ms a step took to ENQUEUE.
// All activations the run keeps for backward live in ONE caller-allocated blob laid out by v100_ir_stack_plan; backward walks the
// blocks in reverse with one shared workspace and two ping-pong gradient buffers.  Pure sequencing of ir_fwd_train / ir_bwd
// (same kernels, same order, bit-identical results) -- except that backward runs the wide blocks' 1x1 weight gradients later, several
// blocks' in one grouped launch (stack_wgrad_plan; the same sums in the same order, bit-identical too), and the narrow blocks below
// them in a second one on smaller tiles (tier 2 of the same plan).
// desc, plan and params: include/voice100_hip.h; the plan ends with {blob_bytes, bwd_ws_bytes, grad_floats, fwd_ws_offset, 0, 0}
enum { ST_N, ST_B, ST_T, ST_BF16, ST_LEVEL, ST_SHADOW, ST_HDR };
namespace {
struct StackBlock { IrShape s; long long a1, a2, a3, y, y16, coef, prep; int Tout; size_t grad_floats; long long defer_off; };
// bwd_ws = the shared workspace (wsmax: the largest block's), two ping-pong gradient buffers (dxmax each), then the deferring blocks' regions
struct StackTotals { size_t blob_bytes, bwd_ws, grad_floats, fwd_ws_off, wsmax, dxmax; };
// the least tiles of a weight gradient that defers to a grouped launch (one XCD's 32 CUs: 8 such problems fill the chip), of a
// grouped flush (3/4 of the chip; below, split-K launches per problem are faster) and the least workgroups of a tier-2 flush that go
// in one small-tile launch (0: tier 2 off); v100_ir_stack_wgrad_group_thresholds, v100_ir_stack_wgrad_group2_threshold
struct WgThresholds { int min_problem_tiles, min_flush_tiles, min_flush_small; };
WgThresholds wg_thresholds = {32, 192, 96};
// fills blocks[0..n) and the totals; returns 0 on a bad descriptor
int stack_layout(const int* desc, StackBlock* blk, StackTotals& t, int min_tiles = wg_thresholds.min_problem_tiles) {
    t = StackTotals{};
    const int n = desc[ST_N], B = desc[ST_B], bf = desc[ST_BF16], level = desc[ST_LEVEL];
    if (n <= 0 || n > 32 || B <= 0 || desc[ST_T] <= 0 || (bf != 0 && bf != 1)) return 0;
    int T = desc[ST_T];
    size_t off = 0, fwd_ws = 0;
    const bool shadows = bf == 1 && level >= 4;
    for (int i = 0; i < n; ++i) {
        const int* d = desc + ST_HDR + 6 * i;
        StackBlock& b = blk[i];
        const int cin = d[0], hid = d[1], cout = d[2], k = d[3], st = d[4], res = d[5];
        if (cin <= 0 || hid <= 0 || cout <= 0 || k <= 0 || st <= 0) return 0;
        const int dims[9] = {B, cin, hid, cout, T, k, st, res, bf};
        IrShape& s = b.s = ir_shape(dims, false);
        s.prepped = true; s.shadows = shadows;
        if (bf == 1 && level && ir_act16_supported(s)) s.act16 = level;
        const int T2 = b.Tout = s.T2, lv = s.act16;
        if (T2 <= 0) return 0;
        const size_t P = pitch16(T, B), P2 = pitch16(T2, B);
        b.a1 = (long long)off; off = al256(off + (lv ? (size_t)B * hid * P * 2 : (size_t)B * hid * T * 4));
        b.a2 = (long long)off; off = al256(off + (lv ? (size_t)B * hid * P * 2 : (size_t)B * hid * T2 * 4));   // (act16: stride 1, T2 == T)
        b.a3 = (long long)off; off = al256(off + (lv >= 3 ? (size_t)B * cout * P * 2 : (size_t)B * cout * T2 * 4));
        b.y = (long long)off; off = al256(off + (size_t)B * cout * T2 * 4);
        b.y16 = -1;
        if (shadows && (i + 1 < n || desc[ST_SHADOW])) { b.y16 = (long long)off; off = al256(off + (size_t)B * cout * P2 * 2); }
        // level 5: block i - 1 need not write its fp32 output when this block (its only reader inside the stack) takes x from the shadow
        if (i > 0 && lv >= 5 && shadows && blk[i - 1].y16 >= 0 && blk[i - 1].s.act16 >= 5) blk[i - 1].s.no_y32 = true;
        b.coef = (long long)off; off = al256(off + (size_t)12 * s.mc * 4);
        IrPrep pw; float* stats; IrBwdWs bws; IrGrads g;
        b.prep = (long long)off; off = al256(off + ir_prep_carve(s, nullptr, pw));
        fwd_ws = std::max(fwd_ws, ir_fwd_carve(s, nullptr, &stats));
        t.wsmax = std::max(t.wsmax, ir_bwd_carve(s, nullptr, bws));
        t.dxmax = std::max(t.dxmax, (size_t)B * cin * T * 4);
        t.grad_floats += b.grad_floats = ir_grads_carve(s, nullptr, g);
        T = T2;
    }
    t.fwd_ws_off = off;
    t.blob_bytes = al256(off + fwd_ws) + 256;
    t.bwd_ws = al256(t.wsmax) + 2 * al256(t.dxmax) + 256;
    // blocks whose weight gradients backward defers to a grouped launch: da3 / da1 in a region of their own behind the shared part
    // (block 0 is sized for a caller that passes x16; without it the block stays on the per-block path and its region unused)
    for (int i = 0; i < n; ++i) {
        blk[i].defer_off = -1;
        if (ir_wgrad_defer_ok(blk[i].s, i == 0 || blk[i - 1].y16 >= 0, WG_TIER_WIDE, min_tiles)) {
            blk[i].defer_off = (long long)t.bwd_ws;
            t.bwd_ws += ir_defer_bytes(blk[i].s);
        }
    }
    return 1;
}

// What the backward walk (blocks n-1 .. 0) does with block i's two 1x1 weight gradients.  tier: whose launch they wait for (-1:
// none, the block launches them itself); off: byte offset in the backward workspace of the region that keeps da3 / da1 until then
// (-1: none).  flush / flush2: tiles of tier 1 / workgroups of tier 2 flushed right after block i's backward, > 0: one grouped
// launch, < 0: too few to fill the chip, the ordinary per-problem launches (0: no flush).
struct WgBlockPlan { int tier; long long off; int flush, flush2; };
// Tier 1 (wide blocks, regions of their own: stack_layout): a flush falls where the pending problems hold >= min_flush_tiles tiles
// and the next block would not fit into the same launch (it does not defer, or would take the launch past one tile per CU or
// WG_GROUP_MAX problems), and where the walk leaves the stack.
// Tier 2 (narrow blocks): once a tier-1 flush is enqueued, the flushed blocks' regions are dead, and a later block of the walk
// whose gradients are problems of the 128 x 128 launch parks ITS da3 / da1 there (first fit, 256-aligned; same stream, so the
// flush has read a region before the block writes it): no regions of its own, no new bytes.  A tier-2 flush falls where the next
// block cannot join, at WG_GROUP_MAX problems, and where the walk ends; it returns what tier 2 borrowed.
void stack_wgrad_plan(const StackBlock* blk, int n, bool have_x16, const WgThresholds& th, WgBlockPlan* plan) {
    int tiles = 0, count = 0;
    for (int i = n - 1; i >= 0; --i) {
        const bool defer = blk[i].defer_off >= 0 && (i > 0 || have_x16);
        plan[i] = WgBlockPlan{defer ? WG_TIER_WIDE : -1, defer ? blk[i].defer_off : -1, 0, 0};
        if (defer) { tiles += ir_wgrad_defer_tiles(blk[i].s, WG_TIER_WIDE); count += 2; }
        if (!count) continue;
        const bool next = i > 0 && blk[i - 1].defer_off >= 0 && (i > 1 || have_x16);
        const bool fits = next && count + 2 <= WG_GROUP_MAX && tiles + ir_wgrad_defer_tiles(blk[i - 1].s, WG_TIER_WIDE) <= WG_GROUP_CHIP_TILES;
        if (i == 0 || count + 2 > WG_GROUP_MAX || (tiles >= th.min_flush_tiles && !fits)) {
            plan[i].flush = tiles >= th.min_flush_tiles ? tiles : -tiles;
            tiles = count = 0;
        }
    }
    struct Span { long long off; size_t bytes; };
    Span dead[32], avail[32];                              // regions of flushed tier-1 blocks; what is left of them
    int ndead = 0, wait1[32], nwait1 = 0;                  // tier-1 blocks not flushed yet
    int wgs = 0;
    count = 0;
    auto end2 = [&](int at) {
        plan[at].flush2 = wgs >= th.min_flush_small ? wgs : -wgs;
        wgs = count = 0;
        for (int j = 0; j < ndead; ++j) avail[j] = dead[j];
    };
    for (int i = n - 1; i >= 0; --i) {
        const size_t need = ir_defer_bytes(blk[i].s);
        const bool can = th.min_flush_small > 0 && plan[i].tier < 0 &&
                         ir_wgrad_defer_ok(blk[i].s, i > 0 ? blk[i - 1].y16 >= 0 : have_x16, WG_TIER_SMALL, 0);
        auto first_fit = [&]() {
            for (int j = 0; can && j < ndead; ++j)
                if (avail[j].bytes >= need) return j;
            return -1;
        };
        int slot = first_fit();
        if (slot < 0 && count) {                           // (count > 0: block i + 1 joined, so i + 1 < n)
            end2(i + 1);
            slot = first_fit();                            // (the regions were full: a new list starts here)
        }
        if (slot >= 0) {
            plan[i].tier = WG_TIER_SMALL;
            plan[i].off = avail[slot].off;
            avail[slot].off += (long long)need; avail[slot].bytes -= need;      // (ir_defer_bytes is a multiple of 256)
            wgs += ir_wgrad_defer_tiles(blk[i].s, WG_TIER_SMALL);
            count += 2;
            if (i == 0 || count + 2 > WG_GROUP_MAX) end2(i);
        }
        if (plan[i].tier == WG_TIER_WIDE) wait1[nwait1++] = i;
        if (plan[i].flush) {
            for (int j = 0; j < nwait1; ++j) dead[ndead] = avail[ndead] = Span{blk[wait1[j]].defer_off, ir_defer_bytes(blk[wait1[j]].s)}, ++ndead;
            nwait1 = 0;
        }
    }
}

// the body of v100_ir_stack_wgrad_plan (tier 1) and v100_ir_stack_wgrad_plan2 (tier 2): the plan's columns of one tier
int stack_wgrad_plan_table(const int* desc, int have_x16, const WgThresholds& th, int tier, long long* out) {
    if (!desc || !out) return V100_ERR_NULL;
    if (th.min_problem_tiles < 1 || th.min_flush_tiles < 1 || th.min_flush_small < 0) return V100_ERR_SHAPE;
    StackBlock blk[32];
    StackTotals t;
    if (!stack_layout(desc, blk, t, th.min_problem_tiles)) return V100_ERR_SHAPE;
    const int n = desc[ST_N];
    WgBlockPlan plan[32];
    stack_wgrad_plan(blk, n, have_x16 != 0, th, plan);
    size_t shared = t.bwd_ws;
    for (int i = 0; i < n; ++i) {
        out[3 * i] = plan[i].tier == tier;
        out[3 * i + 1] = tier == WG_TIER_WIDE ? blk[i].defer_off : plan[i].tier == tier ? plan[i].off : -1;
        out[3 * i + 2] = tier == WG_TIER_WIDE ? plan[i].flush : plan[i].flush2;
        if (blk[i].defer_off >= 0 && (size_t)blk[i].defer_off < shared) shared = (size_t)blk[i].defer_off;
    }
    out[3 * n] = (long long)t.bwd_ws; out[3 * n + 1] = (long long)shared;
    return V100_OK;
}
}   // namespace

// Test hook: the least tiles of a gradient that defers (32) and of a grouped flush (192).  The defaults are what fills the chip;
// tests lower them to reach the grouped path at small shapes.  Changes v100_ir_stack_plan's bwd_ws_bytes: set before planning.
extern "C" int v100_ir_stack_wgrad_group_thresholds(int min_problem_tiles, int min_flush_tiles) {
    if (min_problem_tiles < 1 || min_flush_tiles < 1) return V100_ERR_SHAPE;
    wg_thresholds.min_problem_tiles = min_problem_tiles;
    wg_thresholds.min_flush_tiles = min_flush_tiles;
    return V100_OK;
}

// The least workgroups of a tier-2 (small-tile) flush that go in one launch (stack_wgrad_plan); 0 turns tier 2 off.
extern "C" int v100_ir_stack_wgrad_group2_threshold(int min_flush_small) {
    if (min_flush_small < 0) return V100_ERR_SHAPE;
    wg_thresholds.min_flush_small = min_flush_small;
    return V100_OK;
}

// Host only (no GPU call): what v100_ir_stack_bwd does with the weight gradients of this descriptor at these thresholds.
// out (HOST long longs, 3 per block + 2): {defers, byte offset of the block's region in the backward workspace (-1: none),
// flush (see WgBlockPlan)}; then {bwd_ws_bytes, bytes of the shared part in front of the regions}.
extern "C" int v100_ir_stack_wgrad_plan(const int* desc, int have_x16, int min_problem_tiles, int min_flush_tiles, long long* out) {
    return stack_wgrad_plan_table(desc, have_x16, WgThresholds{min_problem_tiles, min_flush_tiles, 0}, WG_TIER_WIDE, out);
}

// As v100_ir_stack_wgrad_plan, for tier 2: out = 3 per block {defers to the small-tile launch, byte offset of the region it borrows
// (-1: none), flush2}; then the same two totals (tier 2 adds no bytes).
extern "C" int v100_ir_stack_wgrad_plan2(const int* desc, int have_x16, int min_problem_tiles, int min_flush_tiles, int min_flush_small,
                                         long long* out) {
    return stack_wgrad_plan_table(desc, have_x16, WgThresholds{min_problem_tiles, min_flush_tiles, min_flush_small}, WG_TIER_SMALL, out);
}

extern "C" long long v100_ir_stack_plan(const int* desc, long long* plan) {
    if (!desc || !plan) return -1;
    StackBlock blk[32];
    StackTotals t;
    if (!stack_layout(desc, blk, t)) return -1;
    const int n = desc[ST_N];
    for (int i = 0; i < n; ++i) {
        long long* o = plan + 8 * i;
        o[0] = blk[i].a1; o[1] = blk[i].a2; o[2] = blk[i].a3; o[3] = blk[i].y; o[4] = blk[i].y16; o[5] = blk[i].coef; o[6] = blk[i].prep;
        o[7] = blk[i].Tout;
    }
    const long long tot[6] = {(long long)t.blob_bytes, (long long)t.bwd_ws, (long long)t.grad_floats, (long long)t.fwd_ws_off, 0, 0};
    for (int j = 0; j < 6; ++j) plan[8 * n + j] = tot[j];
    return (long long)t.blob_bytes;
}

// x16: bf16 shadow of x written by whatever produced x (NULL: the first expand GEMM reads the fp32 x)
extern "C" int v100_ir_stack_fwd_train(const int* desc, const void* const* params, const void* x, const void* x16, void* blob,
                                       void* stream) {
    if (!desc || !params || !x || !blob) return V100_ERR_NULL;
    StackBlock blk[32];
    StackTotals t;
    if (!stack_layout(desc, blk, t)) return V100_ERR_SHAPE;
    const int n = desc[ST_N];
    char* base = (char*)blob;
    auto at = [&](long long off) { return (float*)(base + off); };
    int rc;
    {   // bf16 / transposed weight copies of every block: one launch
        int shapes[32 * IR_NSHAPE];
        const void* w1s[32]; const void* w3s[32]; void* preps[32];
        for (int i = 0; i < n; ++i) {
            ir_shape_ints(blk[i].s, shapes + i * IR_NSHAPE);
            const IrParams p = ir_params(params + 18 * i);
            w1s[i] = p.w1; w3s[i] = p.w3; preps[i] = base + blk[i].prep;
        }
        CK(v100_ir_prep_batched(shapes, w1s, w3s, preps, n, stream));
    }
    const void *xin = x, *xin16 = x16;
    for (int i = 0; i < n; ++i) {
        const StackBlock& b = blk[i];
        void* y16 = b.y16 >= 0 ? base + b.y16 : nullptr;
        const IrFwdArgs a{(const float*)xin, ir_params(params + 18 * i), at(b.a1), at(b.a2), at(b.a3), at(b.y), at(b.coef), base + t.fwd_ws_off,
                          base + b.prep, xin16, y16};
        CK(ir_fwd_train(b.s, a, (hipStream_t)stream));
        xin = base + b.y;
        xin16 = y16;
    }
    return V100_OK;
}

// dy: gradient of the last block's output; dx: gradient of x (NULL = not needed); grads: grad_floats floats, per block
// in ir_grads_carve's order; ws: bwd_ws_bytes (plan)
extern "C" int v100_ir_stack_bwd(const int* desc, const void* const* params, const void* x, const void* x16, const void* blob,
                                 const void* dy, void* dx, void* grads, void* ws, void* stream) {
    if (!desc || !params || !x || !blob || !dy || !grads || !ws) return V100_ERR_NULL;
    StackBlock blk[32];
    StackTotals t;
    if (!stack_layout(desc, blk, t)) return V100_ERR_SHAPE;
    const int n = desc[ST_N];
    const char* base = (const char*)blob;
    auto at = [&](long long off) { return (const float*)(base + off); };
    char* w0 = (char*)ws;
    char* pp[2] = {w0 + al256(t.wsmax), w0 + al256(t.wsmax) + al256(t.dxmax)};
    size_t goff = t.grad_floats;
    const void* dyi = dy;
    int rc;
    // Round 6: at level 5 the GRADIENT stream between two blocks is bf16 too (what autograd hands back for a bf16 residual stream under
    // the reference's autocast) wherever both sides can take it: the producer a block on the finished-gradient path (its expand
    // backward-data GEMM adds dy, if it has a residual, and stores dx through the 16-bit epilogue), the consumer a block whose one-pass
    // BatchNorm-3 backward covers the shape.  Half the bytes of the three passes that touch it (dx store, dy in BatchNorm-3 backward, dy as the
    // residual gradient).  V100_IR_GRAD16=0: the fp32 stream (A/B).
    static const bool grad16_on = [] { const char* e = getenv("V100_IR_GRAD16"); return !(e && e[0] == '0'); }();
    auto grad16_ok = [&](int i) {                          // block i can consume a 16-bit dy AND produce a 16-bit dx
        const IrShape& s = blk[i].s;
        return grad16_on && desc[ST_LEVEL] >= 5 && s.act16 >= 3 && s.S == 1 && s.T >= 8 && chan_bn3_bwd_fits(s.B, s.T) && ir_act16_supported(s) &&
               dw_bwd_da1_supported(s.B, s.hid, s.T, s.K, v100_dw_num_groups(s.B, s.hid));
    };
    // Deferred weight gradients (stack_wgrad_plan): the wide blocks' 1x1 weight gradients wait for one grouped launch, one tile per
    // CU through the whole contraction, instead of a split-K launch + slab reduction each.  Same sums in the same order.  Tier 2:
    // the narrow blocks' wait in the regions a tier-1 flush has left dead, for one small-tile launch.
    WgBlockPlan plan[32];
    stack_wgrad_plan(blk, n, x16 != nullptr, wg_thresholds, plan);
    // pending problems of the two tiers, their blocks
    struct Pending { WgGroupProblem pr[WG_GROUP_MAX]; int blk[WG_GROUP_MAX]; int n; } pend[2];
    pend[0].n = pend[1].n = 0;
    auto flush_pending = [&](WgTier tier, bool grouped) -> int {
        Pending& q = pend[tier];
        int rc = V100_OK;
        if (grouped) rc = pw_wgrad_group_launch(tier, q.n, q.pr, (hipStream_t)stream);
        else
            for (int j = 0; j < q.n && rc == V100_OK; ++j) {               // too few tiles: split-K per problem, slabs in the shared workspace
                IrBwdWs w;
                ir_bwd_carve(blk[q.blk[j]].s, w0, w);
                const WgGroupProblem& p = q.pr[j];
                rc = v100_pw_wgrad_io(p.G, nullptr, nullptr, nullptr, nullptr, 0, p.X, p.xa, p.xb, p.x_mode, w.slab, p.dW, p.S, p.B, p.M, p.K, p.T,
                                      WG_IO_G | WG_IO_X, stream);
            }
        q.n = 0;
        return rc;
    };
    bool dy_is16 = false;
    for (int i = n - 1; i >= 0; --i) {
        const StackBlock& b = blk[i];
        IrShape s = b.s;
        const int tier = plan[i].tier;                           // whose launch the block's two 1x1 weight gradients wait for
        s.defer = tier >= 0;
        // dx of block i is dy of block i - 1: 16-bit when both are capable blocks (with or without a residual)
        const bool dx_is16 = i > 0 && grad16_ok(i) && grad16_ok(i - 1);
        if (dy_is16 && !grad16_ok(i)) return V100_ERR_SHAPE;      // (cannot happen: dy_is16 was decided with this block's capability)
        s.dy16 = dy_is16; s.dx16 = dx_is16;
        goff -= b.grad_floats;
        void* dxi = i > 0 ? (void*)pp[i & 1] : dx;
        const IrParams p = ir_params(params + 18 * i);
        const void* x16i = i > 0 ? (blk[i - 1].y16 >= 0 ? (const void*)(base + blk[i - 1].y16) : nullptr) : x16;
        IrBwdArgs a{i > 0 ? at(blk[i - 1].y) : (const float*)x, at(b.a1), at(b.a2), at(b.a3), p.w1, p.wd, p.w3, p.bn1.gamma, p.bn2.gamma, p.bn3.gamma,
                    at(b.coef), (const float*)dyi, (float*)dxi, {}, w0, (void*)(base + b.prep), x16i, tier >= 0 ? w0 + plan[i].off : nullptr};
        ir_grads_carve(s, (float*)grads + goff, a.g);
        CK(ir_bwd(s, a, (hipStream_t)stream));
        if (tier >= 0) {
            Pending& q = pend[tier];
            ir_wgrad_problems(s, &a, q.pr + q.n);
            q.blk[q.n] = q.blk[q.n + 1] = i;
            q.n += 2;
        }
        if (plan[i].flush) CK(flush_pending(WG_TIER_WIDE, plan[i].flush > 0));
        if (plan[i].flush2) CK(flush_pending(WG_TIER_SMALL, plan[i].flush2 > 0));
        dyi = dxi;
        dy_is16 = dx_is16;
    }
    return V100_OK;
}
