"""The eval-mode depthwise stage on 16-bit hidden tensors -- what inference at precision "bf16" / "fp16" runs between the two 1x1 GEMMs
of every stride-1 block (csrc/depthwise.hip dw_fwd_eval_io -> dwconv_fwd16_stream_kernel<..., EV[, F16]>, rows of more than 768 outputs
the general MFMA kernel) -- on its own, through v100_dwconv_fwd_eval_io, ELEMENTWISE against float64 on the operands as the kernel
defines them (style and helpers of tests/test_gpu_io_oracle.py):

  * h1 is the stored bf16 / fp16 value, its pitch padding [T, P) NaN: the kernel loads the run that straddles T and must clear it;
  * a tap is the fp32 tap rounded ONCE to the storage format (dwm_split_taps<DW_DIGITS16 = 1>; the fp16 kernel is instantiated with
    the same NT = 1 and keeps only the first digit of dwm_split_f16, i.e. fp16(w) -- not fp16(w) + fp16(w - fp16(w)));
  * products are exact, accumulation fp32 (reference: float64), then relu6f(fmaf(acc, out_a, out_b)) and one rounding to 16 bits.

Bar, the family's own: |got - ref| - |ref| * ulp <= 2e-4 * max(1, max |ref|) per tensor, ref the result BEFORE its rounding to 16 bits
(as `close(..., out16=True)`), ulp = 2^-8 (bf16) / 2^-10 (fp16); every element counts.  Run with -s for the worst error over its bar.

Regimes (dw_fwd_eval_io's formulas restated in `geom`, in every test id): T <= 512: NS = 2, `segn` utterances of one group share a wave
item `ss` positions apart; 513 .. 768: NS = 3; longer: the general kernel, bf16 batch-major only.  Packing needs more than one utterance
per GROUP and there are G = min(B, ceil(2048 / C)) groups (one from C = 1024), so the packed families run either C = 1024 with the small
batches themselves or a small C with B > 2048 / C; the unpacked ones keep C at 4."""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_io_oracle import col, fma32

pytestmark = pytest.mark.gpu

CM, F16 = 1, 2                       # flags of v100_dwconv_fwd_eval_io
SPECIALISED = (5, 7, 11, 17, 19, 27, 29, 33, 35, 51, 59, 65, 67, 75, 83)      # V100_DW_SPECIALISED
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -10}
TOL = 2e-4
SENTINEL = -7.0                      # exact in both formats and never a result (results lie in [0, 6])
PLANNED_SEGN = {1, 2, 3, 4, 5, 6, 8, 16}


def _native():
    from voice100_amd import _native as N
    N.load()
    return N


def pitch_rule(T, B):                # csrc/common.h v100_pitch16 (checked against v100_row_pitch16 in every case)
    return (T + 63) & ~63 if (B > 1 and T >= 256) else (T + 7) & ~7


def groups_rule(B, C):               # csrc/depthwise.hip v100_dw_num_groups (checked against the helper in every case)
    G = 1 if C >= 1024 else -(-2048 // C)
    return max(1, min(G, B))


def geom(B, C, T, K):
    """dw_fwd_eval_io / dw_launch_fwd_eval16 restated: pitch, segment stride, utterances per item, sub-tiles (0 = general kernel)"""
    P, pad = pitch_rule(T, B), (K - 1) // 2
    ss = (P + pad + 15) & ~15
    room = 512 if T <= 512 else 768
    segn = (room - P) // ss + 1 if T <= 512 else 1
    if segn > 1 and (segn - 1) * ss + P > room:
        segn -= 1
    G = groups_rule(B, C)
    return dict(P=P, pad=pad, ss=ss, segn=segn, ns=2 if T <= 512 else 3 if T <= 768 else 0, G=G, bper=-(-B // G))


def largest_T(K, n):
    """the longest row of which dw_fwd_eval_io still packs n to an item (B > 1)"""
    return max(T for T in range(1, 513) if geom(2, 1024, T, K)["segn"] >= n)


Shape = collections.namedtuple("Shape", "family B C T K signed")
SHAPES = []


def add(family, B, C, T, K, signed=False):
    SHAPES.append(Shape(family, B, C, T, K, signed))


# heavy packing, ONE group (C = 1024): the one-second-chunk row and twice that; B = 1, 2, segn - 1, segn, segn + 1 and 4 segn + 2 (five
# items, i.e. a second item for the first wave, the last one short)
for T_, K_ in ((51, 19), (101, 83)):
    s_ = geom(2, 1024, T_, K_)["segn"]
    for B_ in sorted({1, 2, s_ - 1, s_, s_ + 1, 4 * s_ + 2}):
        add("pack", B_, 1024, T_, K_)
for T_, K_ in ((51, 5), (51, 51), (51, 83), (101, 19)):           # the other segment counts of those rows: 8, 5, 5, 4
    add("pack", geom(2, 1024, T_, K_)["segn"] + 1, 1024, T_, K_)
# rows of a few samples (T = 5 < pad; 7, 8, 9 around the 8-sample run): sixteen to an item at K = 19, eight at K = 83
for T_ in (1, 5, 7, 8, 9):
    add("tiny", 17, 1024, T_, 19)
add("tiny", 9, 1024, 5, 83)
# the edge of the segment count: the longest row that still packs two, that plus 8 (alone), the longest that packs three
for K_ in (83, 19):
    add("edge2", 3, 1024, largest_T(K_, 2), K_)
    add("edge1", 3, 1024, largest_T(K_, 2) + 8, K_)
    add("edge3", 4, 1024, largest_T(K_, 3), K_)
# one row per item: around 256 (the pitch rule changes: 300 -> 320 for B > 1, 304 alone), the ends of NS = 2 and NS = 3
for T_, K_ in ((255, 19), (256, 83), (257, 19), (300, 51), (509, 83), (512, 83), (513, 83), (520, 19), (563, 51), (763, 83), (768, 83)):
    add("stream", 2 + T_ % 2, 4, T_, K_)
add("stream", 1, 4, 300, 19)
add("stream", 1, 4, 563, 83)
add("stream-rows", 6, 1024, 300, 19)           # six rows in one group: the first two waves run a second row
add("stream-rows", 5, 1024, 520, 51)
# the general kernel (bf16 batch-major; refused in the other three forms)
for T_, K_ in ((769, 19), (776, 83), (1100, 51)):
    add("general", 2, 4, T_, K_)
add("general-rows", 5, 1024, 776, 83)
# several groups whose ceil(B / G) utterances are no multiple of segn = 6: a short last item in every group (C = 512: channels permuted
# as well; C = 64: not), and B = 33 on 32 groups: two utterances each, one in the 17th, none in the rest
add("groups", 31, 512, 51, 19)
add("groups", 253, 64, 51, 19)
add("groups-empty", 33, 64, 51, 19)
# v100_chan_of_block<16> is not the identity (C % 128 == 0); taps and coefficients differ per channel in every case
add("perm", 2, 128, 51, 51)
add("perm", 1, 256, 520, 35)
# signed input (the kernel does not assume the producer's range)
add("signed", 7, 1024, 51, 19, True)
add("signed", 2, 4, 520, 83, True)


def shape_id(s):
    g = geom(s.B, s.C, s.T, s.K)
    regime = f"NS{g['ns']}" if g["ns"] else "general"
    return f"{s.family}-B{s.B}-C{s.C}-T{s.T}-K{s.K}-P{g['P']}-ss{g['ss']}-segn{g['segn']}-{regime}-G{g['G']}{'-signed' if s.signed else ''}"


Case = collections.namedtuple("Case", "x16 w a b ref")


@functools.lru_cache(maxsize=4)
def make_case(cuda, fmt, s):
    """operands and the float64 reference of one (format, shape): computed once, shared by the tests that need it, never modified"""
    B, C, T, K = s.B, s.C, s.T, s.K
    pad = (K - 1) // 2
    g = torch.Generator(device=cuda).manual_seed(1000003 * B + 7919 * C + 31 * T + K + (17 if s.signed else 0))
    rnd = lambda *sh: torch.randn(*sh, generator=g, device=cuda)
    uni = lambda *sh: torch.rand(*sh, generator=g, device=cuda)
    # what the expand GEMM's ReLU6 epilogue emits: [0, 6] with exact zeros and sixes
    x = rnd(B, C, T) * 2 if s.signed else torch.clamp(rnd(B, C, T) * 3 + 2.5, 0, 6)
    # the head of every utterance large and distinct per utterance, its tail from another set: whatever leaks across a segment gap
    # moves the outputs next to it by tap * (4 .. 6), far above the bar
    n = min(pad, T // 3)
    if n:
        bi = (torch.arange(B, device=cuda) % 16).float()[:, None, None]
        x[:, :, :n] = 4 + bi / 8
        x[:, :, T - n:] = 0.25 + bi / 16
    x16 = x.to(DT[fmt])
    xs = x16.double()
    if not s.signed:
        assert bool((xs == 0).any()) and bool((xs == 6).any()) and float(xs.min()) >= 0 and float(xs.max()) <= 6
    w = rnd(C, K) * 0.2
    wq = w.to(DT[fmt]).double()                     # the taps as the kernel forms them: ONE rounding to the storage format
    xp = F.pad(xs, (pad, pad))
    acc = torch.zeros_like(xs)
    for j in range(K):                              # F.conv1d(xs, wq[:, None, :], padding=pad, groups=C), written out
        acc += xp[:, :, j:j + T] * wq[:, j][None, :, None]
    # folded BatchNorm 2: both signs of the scale; the shift centres each channel's pre-activation on -3, 3 or 9 with a spread of
    # 2 .. 6, so that all three branches of the clamp occur
    flat = acc.transpose(0, 1).reshape(C, -1)
    med, sd = flat.median(1).values, flat.std(1, unbiased=False).clamp_min(1.0)
    sign = torch.where(uni(C) < 0.5, -1.0, 1.0).double()
    sign[0], sign[1] = 1.0, -1.0
    a = (sign * (0.5 + uni(C).double()) * 4 / sd).float()
    b = (3.0 + ((torch.arange(C, device=cuda) % 3) - 1) * 6.0 - a.double() * med).float()
    ref = torch.clamp(fma32(acc, col(a), col(b)), 0, 6)             # relu6f(fmaf(acc, out_a, out_b)), before its rounding to 16 bits
    assert bool((ref == 0).any()) and bool((ref == 6).any()) and bool(((ref > 0) & (ref < 6)).any())
    assert bool((a > 0).any()) and bool((a < 0).any())
    return Case(x16, w, a, b, ref)


def lay_out(t16, T, P, cm, fill):
    """[B, C, T] -> the tensor as the kernel addresses it: [B][C][P], or [C][B][P] when channel-major, the padding = fill"""
    B, C, _ = t16.shape
    buf = torch.full((B, C, P), fill, dtype=t16.dtype, device=t16.device)
    buf[:, :, :T] = t16
    return buf.transpose(0, 1).contiguous() if cm else buf


def rows(buf, cm):
    return buf.transpose(0, 1) if cm else buf       # [B, C, P] view


def bits(t):
    return t.contiguous().view(torch.int16)


def run(fmt, cm, x16, c, T, K):
    """one call on x16 [B, C, T] -> the output tensor in its layout, pre-filled with SENTINEL"""
    N = _native()
    B, C, _ = x16.shape
    h1 = lay_out(x16, T, pitch_rule(T, B), cm, float("nan"))         # NaN padding: read (the run that straddles T), never used
    h2 = torch.full_like(h1, SENTINEL)
    N.call("v100_dwconv_fwd_eval_io", h1, c.w, c.a, c.b, h2, B, C, T, K, (CM if cm else 0) | (F16 if fmt == "fp16" else 0))
    return h2


def check(got, ref, fmt, what):
    got = got.double()
    assert torch.isfinite(got).all(), what
    bound = TOL * max(1.0, float(ref.abs().max()))
    err = (got - ref).abs() - ref.abs() * ULP[fmt]                  # one rounding of the stored value (half an ulp; the ulp covers ties)
    worst = float(err.max())
    # (for the reader only: how many stored values are not the reference rounded to 16 bits -- fp32 accumulation against float64
    #  decides a rounding the other way now and then; the ulp term of the bar is there for exactly these)
    other = int((got != ref.to(DT[fmt]).double()).sum())
    print(f"[eval-dw-oracle] {what}: worst/bar = {worst / bound:.4f} (worst {worst:.3e}, bar {bound:.3e}; "
          f"{other} of {got.numel()} not round16(ref), max |got - ref| {float((got - ref).abs().max()):.3e})")
    if worst > bound:
        bad = err > bound
        b_, c_, t_ = (int(v) for v in torch.unravel_index(err.argmax(), err.shape))
        raise AssertionError(f"{what}: max err {worst:.3e} > {bound:.3e} at (b, c, t) = ({b_}, {c_}, {t_}): got {float(got[b_, c_, t_])!r}, "
                             f"ref {float(ref[b_, c_, t_])!r}; {int(bad.sum())} of {bad.numel()} elements over the bar, "
                             f"utterances {sorted(set(bad.nonzero()[:, 0].tolist()))[:12]}")


def check_geometry(s):
    """the regime each family is meant to reach, from the formulas; pitch and group count against the library's own helpers"""
    N = _native()
    g = geom(s.B, s.C, s.T, s.K)
    assert N.helper("v100_row_pitch16", s.T, s.B) == g["P"] and N.helper("v100_dw_num_groups", s.B, s.C) == g["G"], (s, g)
    assert N.helper("v100_dw_mfma_supported", s.K, 1) == 1 and s.K in SPECIALISED
    fam = s.family
    if fam in ("pack", "tiny", "groups", "groups-empty", "edge2", "edge3"):
        assert g["ns"] == 2 and g["segn"] >= 2 and (g["segn"] - 1) * g["ss"] + g["P"] <= 512 and g["ss"] % 16 == 0, (s, g)
        assert g["ss"] - s.T >= g["pad"], (s, g)                    # the zero gap two neighbours share
    if fam == "edge2":
        assert g["segn"] == 2 and g["bper"] == 3 and geom(s.B, s.C, s.T + 8, s.K)["segn"] == 1, (s, g)
    if fam == "edge3":
        assert g["segn"] == 3 and g["bper"] == 4 and geom(s.B, s.C, s.T + 8, s.K)["segn"] == 2, (s, g)
    if fam == "edge1":
        assert g["segn"] == 1 and g["ns"] == 2 and geom(s.B, s.C, s.T - 8, s.K)["segn"] == 2, (s, g)
    if fam in ("stream", "stream-rows"):
        assert g["segn"] == 1 and g["ns"] == (2 if s.T <= 512 else 3), (s, g)
    if fam == "stream-rows" or fam == "general-rows":
        assert g["G"] == 1 and s.B > 4, (s, g)
    if fam in ("general", "general-rows"):
        assert g["ns"] == 0 and s.T > 768, (s, g)
    if fam == "groups":
        assert g["G"] > 1 and g["bper"] > g["segn"] and g["bper"] % g["segn"] != 0, (s, g)
        assert all((min(s.B, (i + 1) * g["bper"]) - i * g["bper"]) % g["segn"] != 0 for i in range(g["G"])), (s, g)     # EVERY group
    if fam == "groups-empty":
        assert g["G"] > 1 and (g["G"] - 1) * g["bper"] > s.B, (s, g)                   # the last groups start past the batch
    if fam == "perm":
        assert s.C % 128 == 0, s
    return g


CASES = [(fmt, cm, s) for s in SHAPES for fmt in ("bf16", "fp16") for cm in (0, 1)]
CASE_IDS = [f"{fmt}-{'cm' if cm else 'bm'}-{shape_id(s)}" for fmt, cm, s in CASES]


def test_case_list_covers_every_regime():
    segn = {geom(s.B, s.C, s.T, s.K)["segn"] for s in SHAPES}
    assert segn == PLANNED_SEGN, segn
    assert {geom(s.B, s.C, s.T, s.K)["ns"] for s in SHAPES} == {0, 2, 3}
    assert {5, 19, 51, 83} <= {s.K for s in SHAPES} and min(SPECIALISED) == 5 and max(SPECIALISED) == 83
    packed = [s for s in SHAPES if s.family == "pack" and s.T in (51, 101) and s.K in (19, 83)]
    for T in (51, 101):
        sn = geom(2, 1024, T, 19 if T == 51 else 83)["segn"]
        assert {1, 2, sn - 1, sn, sn + 1, 4 * sn + 2} <= {s.B for s in packed if s.T == T}
    for s in SHAPES:
        check_geometry(s)


@pytest.mark.parametrize("fmt,cm,s", CASES, ids=CASE_IDS)
def test_eval_dw_vs_float64(cuda, fmt, cm, s):
    """Every valid output against float64; the padding of the output rows as include/voice100_hip.h states it: [T, (T + 3) & ~3) is
    overwritten with finite values in [0, 6] that are not part of the result, the rest of [T, P) keeps the caller's bits.  The general
    kernel exists for bf16 batch-major only: the other three forms of a row of more than 768 outputs are refused and nothing is written."""
    g = check_geometry(s)
    B, C, T, K, P = s.B, s.C, s.T, s.K, g["P"]
    what = f"{fmt} {'channel-major' if cm else 'batch-major'} {shape_id(s)}"
    if g["ns"] == 0 and (cm or fmt == "fp16"):
        N = _native()
        h1 = torch.zeros((C, B, P) if cm else (B, C, P), dtype=DT[fmt], device=cuda)
        h2 = torch.full_like(h1, SENTINEL)
        w, ab = torch.zeros(C, K, device=cuda), torch.ones(C, device=cuda)
        with pytest.raises(RuntimeError):
            N.call("v100_dwconv_fwd_eval_io", h1, w, ab, ab, h2, B, C, T, K, (CM if cm else 0) | (F16 if fmt == "fp16" else 0))
        torch.cuda.synchronize()
        assert bool((h2 == SENTINEL).all()), what
        return
    c = make_case(cuda, fmt, s)
    out = rows(run(fmt, cm, c.x16, c, T, K), cm)
    check(out[:, :, :T], c.ref, fmt, what)
    T4 = (T + 3) & ~3
    tail = out[:, :, T:T4].float()
    assert bool(((tail >= 0) & (tail <= 6)).all()), what + ": [T, (T + 3) & ~3)"
    assert bool((out[:, :, T4:] == SENTINEL).all()), what + ": [(T + 3) & ~3, P) was written"


STREAMING = [s for s in SHAPES if s.T <= 768]


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("s", STREAMING, ids=[shape_id(s) for s in STREAMING])
def test_channel_major_equals_batch_major(cuda, fmt, s):
    """the same kernel on the same values in the other storage order: every valid element bit for bit"""
    c = make_case(cuda, fmt, s)
    bm = run(fmt, 0, c.x16, c, s.T, s.K)[:, :, :s.T]
    cm = rows(run(fmt, 1, c.x16, c, s.T, s.K), 1)[:, :, :s.T]
    assert torch.equal(bits(bm), bits(cm)), (fmt, shape_id(s), int((bits(bm) != bits(cm)).sum()))


PACKED = [s for s in SHAPES if geom(s.B, s.C, s.T, s.K)["segn"] >= 2 and geom(s.B, s.C, s.T, s.K)["bper"] >= 2 and s.B <= 33]


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("s", PACKED, ids=[shape_id(s) for s in PACKED])
def test_packed_equals_one_row_alone(cuda, fmt, s):
    """dw_fwd_eval_io: "the packed form sums exactly what the one-row form sums" -- utterance b out of the packed batch equals, bit for
    bit, the same utterance run alone (B = 1: one utterance in its item, no neighbour to bring in).  Valid elements only."""
    c = make_case(cuda, fmt, s)
    packed = run(fmt, 0, c.x16, c, s.T, s.K)[:, :, :s.T]
    for b in range(s.B):
        alone = run(fmt, 0, c.x16[b:b + 1], c, s.T, s.K)[:, :, :s.T]
        assert torch.equal(bits(alone), bits(packed[b:b + 1])), (fmt, shape_id(s), b, int((bits(alone) != bits(packed[b:b + 1])).sum()))


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("cm", [0, 1])
def test_kernel_sizes_without_a_kernel_are_refused(cuda, fmt, cm):
    """dw_fwd_eval_io refuses an even K before anything else, and an odd K outside V100_DW_SPECIALISED finds no kernel in either the
    streaming or the general launcher (16-bit storage exists on the MFMA kernels only): an error, no fallback, nothing written."""
    N = _native()
    flags = (CM if cm else 0) | (F16 if fmt == "fp16" else 0)
    for B, C, T, K in ((2, 4, 51, 18), (2, 4, 51, 84), (2, 4, 51, 3), (2, 4, 51, 21), (2, 4, 600, 21), (2, 4, 900, 21), (2, 4, 900, 18), (2, 4, 51, 85)):
        assert K % 2 == 0 or (K not in SPECIALISED and N.helper("v100_dw_mfma_supported", K, 1) == 0)
        P = pitch_rule(T, B)
        h1 = torch.zeros((C, B, P) if cm else (B, C, P), dtype=DT[fmt], device=cuda)
        h2 = torch.full_like(h1, SENTINEL)
        w, ab = torch.zeros(C, K, device=cuda), torch.ones(C, device=cuda)
        with pytest.raises(RuntimeError):
            N.call("v100_dwconv_fwd_eval_io", h1, w, ab, ab, h2, B, C, T, K, flags)
        with pytest.raises(RuntimeError):
            N.call("v100_dwconv_fwd_eval_io", h1, None, ab, ab, h2, B, C, T, 19, flags)            # a NULL operand
        torch.cuda.synchronize()
        assert bool((h2 == SENTINEL).all()), (fmt, cm, B, C, T, K)
