"""Cases, restated dispatch and float64 references for the fp32-STORAGE depthwise kernels (K2: csrc/depthwise.hip,
csrc/depthwise_common.h, csrc/depthwise_mfma.h): no GPU, no HIP.  tests/test_gpu_dw_f32_oracle.py runs GEOS on the device and
holds every element to the bars below; tests/test_dw_f32_cases_cpu.py checks that the tables reach what they claim to reach, that the
reference is the plain F.conv1d + hardtanh + autograd composition, and that fp32 torch on the CPU sits inside every bar.

Operands as the fp32 kernels define them: an on-load transform is formed in fp32 with the kernel's own fused operations --
relu6f(fmaf(x, a, b)) or fmaf(x, a, fmaf(x2, b, c)) (dw_in_transform) -- and nothing else is rounded; the convolution and its adjoints
run in float64 through F.conv1d and autograd; the ReLU6 mask is (pre > 0) & (pre < 6) on the fp32 pre.  Next to every result the
reference returns A, the same sum over absolute values (A_t = sum_j |w_j| |xin_{t s - pad + j}|, and likewise for the gradients).

Bars, u = 2^-24, every element:
  output          |got - ref| <= c u A + u |ref|,  c = K + 4 for an fmaf chain (K fused multiply-adds: <= ~K u A; 4: the transform's
                  roundings), c = 6 K + 8 for the three-digit MFMA kernel (six digit-pair passes of K terms each into the fp32
                  accumulator; the three dropped digit products are <= ~2 u per product)
  slab sums       the sum of the element bars of what is summed + n u sum|terms|, n the number of terms; sums with aux: the same
                  form on |y aux|
  weight gradient the same rule: n = B Tout products per tap, so c(n) u A_dw + u |ref| with c(n) = n + 4 | 6 n + 8
Both c are worst-case and derived, not fitted."""
from typing import NamedTuple, Tuple

import torch
import torch.nn.functional as F

U = 2.0 ** -24
SPECIALISED = (5, 7, 11, 17, 19, 27, 29, 33, 35, 47, 51, 59, 65, 67, 75, 83)       # V100_DW_SPECIALISED
IN_NONE, IN_AFFINE_RELU6, IN_AFFINE2 = 0, 1, 2                                      # DW_IN_*
OUT_RAW_STATS, OUT_AFFINE_RELU6, OUT_MASK_STATS = 0, 1, 2                           # DW_OUT_*
DWCONV_REGIMES = ("mfma", "s2_r4", "s2_r8", "up2", "generic")
WGRAD_REGIMES = ("spec", "s2", "generic")
BWD_REGIMES = ("fused_g1", "fused_slab", "split")
FAMILIES = ("benign", "spread", "kinks", "sparse")


# ------------------------------------------------------------------------------------------------------------------------------
# a. the dispatch, restated
# ------------------------------------------------------------------------------------------------------------------------------
def regime_dwconv(in_mode, out_mode, K, stride, upsample, flip, pad, Tout, force_generic):
    """v100_dwconv (csrc/depthwise.hip:367-380) and dw_launch_specialised (csrc/depthwise_common.h:565-602), for tensors under the
    2 GiB descriptor limit.  The three (in, out) mode pairs with a launcher: train forward (1, 0), eval forward (0, 1), backward-data
    (2, 2) -- depthwise.hip:369-373.  Stride 1 with a specialised K: the Toeplitz-MFMA kernel, whatever pad (common.h:570-583).
    K = 11 at stride 2: dwconv_kernel<11, 2, R>, R = 8 from Tout > 256 (common.h:588-598).  Zero-stuffed by 2, flipped, K = 11,
    pad = 5, backward-data modes: dwconv_up2_bwd_kernel (depthwise.hip:375-379).  Everything else: dwconv_generic_kernel (:380)."""
    pair = (in_mode, out_mode) in ((IN_AFFINE_RELU6, OUT_RAW_STATS), (IN_NONE, OUT_AFFINE_RELU6), (IN_AFFINE2, OUT_MASK_STATS))
    if not force_generic and upsample == 1 and pair:
        if stride == 1 and K in SPECIALISED:
            return "mfma"
        if K == 11 and stride == 2:
            return "s2_r8" if Tout > 256 else "s2_r4"
    if (not force_generic and upsample == 2 and stride == 1 and flip and K == 11 and pad == (K - 1) // 2
            and in_mode == IN_AFFINE2 and out_mode == OUT_MASK_STATS):
        return "up2"
    return "generic"


def regime_wgrad(g_mode, x_mode, K, stride, force_generic):
    """v100_dwconv_wgrad (csrc/depthwise.hip:397-404): dwconv_wgrad_kernel<K, 1, 8> for the training combination (g' the BN-backward
    affine of two tensors, x' = relu6(bn(a1))) at a specialised K and stride 1, <11, 2, 8> for the opener, else the generic kernel."""
    if not force_generic and g_mode == IN_AFFINE2 and x_mode == IN_AFFINE_RELU6:
        if stride == 1 and K in SPECIALISED:
            return "spec"
        if K == 11 and stride == 2:
            return "s2"
    return "generic"


def regime_bwd(K, stride, force_split, G):
    """v100_dwconv_bwd (csrc/depthwise.hip:540-558): stride 1 with a specialised K runs dw_launch_bwd_fused (the WG form of the MFMA
    kernel, csrc/depthwise_bwd_fused.hip); with one group the kernel's partial IS dw (:545), with more a slab_reduce follows (:549).
    Anything else, or force_split: v100_dwconv_wgrad + v100_dwconv."""
    if not force_split and stride == 1 and K in SPECIALISED:
        return "fused_g1" if G == 1 else "fused_slab"
    return "split"


def launches_bwd(regime):
    """kernel launches one v100_dwconv_bwd issues (the one observable of its route): fused 1 (+ slab_reduce when G > 1); split:
    wgrad kernel + slab_reduce + the data kernel"""
    return {"fused_g1": 1, "fused_slab": 2, "split": 3}[regime]


def c_of(regime, K):
    """the c of the output bar: 6 K + 8 on the MFMA kernels, K + 4 on every fmaf chain"""
    return 6 * K + 8 if regime in ("mfma", "fused_g1", "fused_slab") else K + 4


def cn_of(regime, n):
    """the same rule for a sum of n products (weight gradient): the fused backward's E tiles are MFMA digit passes"""
    return 6 * n + 8 if regime in ("fused_g1", "fused_slab") else n + 4


# ------------------------------------------------------------------------------------------------------------------------------
# c. the case tables.  A Geo is one geometry (forward K / stride / pad, shape (B, G, C, T), T the forward INPUT length); its rows are
# the calls made on it: (op, force, tag).  op: fwd_train | fwd_eval | bwd_data (v100_dwconv), wgrad | wgrad00 (v100_dwconv_wgrad,
# wgrad00 = g_mode 0 / x_mode 0), bwd (v100_dwconv_bwd).  force: force_generic / force_split.  tag: the regime the row is there for.
# ------------------------------------------------------------------------------------------------------------------------------
class Geo(NamedTuple):
    name: str
    K: int
    stride: int
    pad: int
    B: int
    G: int
    C: int
    T: int
    rows: Tuple[Tuple[str, int, str], ...]
    fams: Tuple[str, ...] = ("benign", "spread")

    @property
    def Tout(self):
        return (self.T + 2 * self.pad - self.K) // self.stride + 1


def _spec_rows(G):
    fused = "fused_g1" if G == 1 else "fused_slab"
    return (("fwd_train", 0, "mfma"), ("fwd_train", 1, "generic"), ("fwd_eval", 0, "mfma"), ("fwd_eval", 1, "generic"),
            ("bwd_data", 0, "mfma"), ("bwd_data", 1, "generic"), ("bwd", 0, fused), ("bwd", 1, "split"),
            ("wgrad", 0, "spec"), ("wgrad", 1, "generic"))


ALL_FAMS = FAMILIES
GEOS = []
# a. specialised stride-1 kernels: every K once -- all four (-pad) & 3 and STEPS = 1 ... 4
for _K in SPECIALISED:
    GEOS.append(Geo(f"spec_k{_K}", _K, 1, (_K - 1) // 2, 3, 2, 3, 130, _spec_rows(2), ALL_FAMS if _K == 47 else ("benign", "spread")))
# the 4-output lane group, the 16 x 16 block, the 256-output sub-tile, the 512-output item; rows shorter than K and than the pad
SPEC_T = (1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1025)
for _K in (5, 47, 83):
    for _T in SPEC_T:
        GEOS.append(Geo(f"spec_k{_K}_t{_T}", _K, 1, (_K - 1) // 2, 2, 1, 2, _T, _spec_rows(1),
                        ALL_FAMS if (_K, _T) == (5, 257) else ("benign", "spread")))
    GEOS.append(Geo(f"spec_k{_K}_emptygroup", _K, 1, (_K - 1) // 2, 5, 4, 2, 40, _spec_rows(4)))     # bper = 2: group 3 owns no row
    GEOS.append(Geo(f"spec_k{_K}_ninerows", _K, 1, (_K - 1) // 2, 9, 1, 2, 70, _spec_rows(1)))       # waves take 3, 2, 2, 2 rows
    GEOS.append(Geo(f"spec_k{_K}_onerow", _K, 1, (_K - 1) // 2, 4, 4, 1, 33, _spec_rows(4)))         # one row per group, C = 1
# pad is free at the entry point and the MFMA launcher does not look at it: "valid" (pad 0) and "full" (pad K - 1) through v100_dwconv
_DWCONV_ONLY = (("fwd_train", 0, "mfma"), ("fwd_train", 1, "generic"), ("fwd_eval", 0, "mfma"), ("fwd_eval", 1, "generic"),
                ("bwd_data", 0, "mfma"), ("bwd_data", 1, "generic"))
for _K in (17, 29):
    GEOS.append(Geo(f"valid_k{_K}", _K, 1, 0, 3, 2, 3, 130, _DWCONV_ONLY))
    GEOS.append(Geo(f"full_k{_K}", _K, 1, _K - 1, 3, 2, 3, 130, _DWCONV_ONLY))

# b. the opener's kernels: K = 11, stride 2, pad 5.  Tout = (Tin - 1) // 2 + 1; 512 -> 256 is the last R = 4 row, 513 -> 257 the first
# R = 8 row; 1023 / 1025 the 512-output tile edges of the up2 and the R = 8 kernels; both parities
OPENER_FWD_TAG = {1: "s2_r4", 2: "s2_r4", 3: "s2_r4", 10: "s2_r4", 11: "s2_r4", 12: "s2_r4", 61: "s2_r4", 511: "s2_r4", 512: "s2_r4",
                  513: "s2_r8", 514: "s2_r8", 1023: "s2_r8", 1024: "s2_r8", 1025: "s2_r8", 77: "s2_r4"}


def _opener_rows(Tin):
    f = OPENER_FWD_TAG[Tin]
    return (("fwd_train", 0, f), ("fwd_train", 1, "generic"), ("fwd_eval", 0, f), ("fwd_eval", 1, "generic"),
            ("bwd_data", 0, "up2"), ("bwd_data", 1, "generic"), ("wgrad", 0, "s2"), ("wgrad", 1, "generic"),
            ("bwd", 0, "split"), ("bwd", 1, "split"))


for _T in (1, 2, 3, 10, 11, 12, 61, 511, 512, 513, 514, 1023, 1024, 1025):
    GEOS.append(Geo(f"opener_t{_T}", 11, 2, 5, 3, 2, 2, _T, _opener_rows(_T), ALL_FAMS if _T in (61, 513) else ("benign", "spread")))
GEOS.append(Geo("opener_emptygroup", 11, 2, 5, 5, 4, 2, 77, _opener_rows(77)))
GEOS.append(Geo("opener_ninerows", 11, 2, 5, 9, 1, 2, 77, _opener_rows(77)))

# c. the generic regime: sizes without a specialisation, and the (g_mode 0, x_mode 0) weight gradient that no specialised kernel takes
_GENERIC_ROWS = (("fwd_train", 0, "generic"), ("fwd_eval", 0, "generic"), ("bwd_data", 0, "generic"), ("wgrad", 0, "generic"),
                 ("wgrad00", 0, "generic"), ("bwd", 0, "split"))
for _K, _S in ((9, 1), (13, 1), (9, 2)):
    for _T in (1, 40, 257):
        GEOS.append(Geo(f"generic_k{_K}_s{_S}_t{_T}", _K, _S, (_K - 1) // 2, 3, 2, 3, _T, _GENERIC_ROWS,
                        ALL_FAMS if (_K, _T) == (9, 40) else ("benign", "spread")))
GEOS.append(Geo("wgrad00_k19", 19, 1, 9, 3, 2, 3, 130, (("wgrad00", 0, "generic"),)))
BY_NAME = {g.name: g for g in GEOS}


def row_regime(geo, op, force):
    """what the restated dispatch returns for one row: (entry point, regime)"""
    K, S, pad = geo.K, geo.stride, geo.pad
    if op == "fwd_train":
        return "dwconv", regime_dwconv(IN_AFFINE_RELU6, OUT_RAW_STATS, K, S, 1, 0, pad, geo.Tout, force)
    if op == "fwd_eval":
        return "dwconv", regime_dwconv(IN_NONE, OUT_AFFINE_RELU6, K, S, 1, 0, pad, geo.Tout, force)
    if op == "bwd_data":       # the conv runs over the upstream gradient (length Tout), zero-stuffed by the stride, taps flipped
        return "dwconv", regime_dwconv(IN_AFFINE2, OUT_MASK_STATS, K, 1, S, 1, K - 1 - pad, geo.T, force)
    if op == "wgrad":
        return "wgrad", regime_wgrad(IN_AFFINE2, IN_AFFINE_RELU6, K, S, force)
    if op == "wgrad00":
        return "wgrad", regime_wgrad(IN_NONE, IN_NONE, K, S, force)
    if op == "bwd":
        return "bwd", regime_bwd(K, S, force, geo.G)
    raise ValueError(op)


def groups(geo):
    """[(b0, b1)] per group: bper = ceil(B / G) rows each, as every kernel splits the batch; b0 == b1 for a group without rows"""
    bper = -(-geo.B // geo.G)
    return [(min(geo.B, g * bper), min(geo.B, (g + 1) * bper)) for g in range(geo.G)]


# ------------------------------------------------------------------------------------------------------------------------------
# input families (seeded; on whatever device is asked for)
# ------------------------------------------------------------------------------------------------------------------------------
def _one_hot(B, C, L, device):
    """a single 1.0 per row, at position 0, L - 1, L // 2 in turn"""
    t = torch.zeros(B, C, L, device=device)
    for r in range(B * C):
        t[r // C, r % C, (0, L - 1, L // 2)[r % 3]] = 1.0
    return t


def make_inputs(geo, family, device="cpu"):
    """fp32 tensors of one (geometry, family).  x_fwd: the forward calls' input; a1: the pre-activation tensor of the backward calls
    (ReLU6 mask, weight-gradient operand) -- the same tensor except in `sparse`; dz2 / a2 with (ga, gb, gc): the two streams of the
    incoming gradient g' = ga dz2 + gb a2 + gc; (s1, t1): the on-load affine; (oa, ob): the eval epilogue.
      benign  what tests/test_gpu_kernels.py draws
      spread  per-channel magnitude 10^(-3 .. 3) on the data streams and (in reverse channel order) on the taps
      kinks   s1 = 1, t1 = 0 on every second channel; a quarter of a1 exactly 0.0, a quarter exactly 6.0: pre sits on both kinks
      sparse  one non-zero sample per row against taps 1, 2, ..., K; affines the identity; a1 small integers inside (0, 6): every
              output is one tap's value (or one sample's), all arithmetic exact"""
    B, C, T, K, Tout = geo.B, geo.C, geo.T, geo.K, geo.Tout
    g = torch.Generator(device=device).manual_seed(1000 * K + 7 * T + 13 * B + FAMILIES.index(family))
    rn = lambda *s: torch.randn(*s, generator=g, device=device)        # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=g, device=device)         # noqa: E731
    a1, w = rn(B, C, T) * 2, rn(C, K) * 0.2
    s1, t1 = ru(C) + 0.5, rn(C)
    dz2, a2 = rn(B, C, Tout), rn(B, C, Tout)
    ga, gb, gc = ru(C) + 0.5, rn(C) * 0.3, rn(C) * 0.1
    oa, ob = ru(C) + 0.5, rn(C)
    x_fwd = a1
    if family == "spread":
        e = torch.linspace(-3, 3, C, device=device) if C > 1 else torch.tensor([-3.0], device=device)
        mag = (10.0 ** e)[None, :, None]
        a1, dz2, a2 = a1 * mag, dz2 * mag, a2 * mag
        w = w * (10.0 ** e.flip(0))[:, None]
        x_fwd = a1
    elif family == "kinks":
        sel = torch.arange(C, device=device) % 2 == 0
        s1 = torch.where(sel, torch.ones_like(s1), s1)
        t1 = torch.where(sel, torch.zeros_like(t1), t1)
        r = ru(B, C, T)
        a1 = torch.where(r < 0.25, torch.zeros_like(a1), torch.where(r < 0.5, torch.full_like(a1, 6.0), a1))
        x_fwd = a1
    elif family == "sparse":
        w = torch.arange(1, K + 1, device=device, dtype=torch.float32).repeat(C, 1)
        s1, t1, oa, ob = torch.ones_like(s1), torch.zeros_like(t1), torch.ones_like(oa), torch.zeros_like(ob)
        ga, gb, gc = torch.ones_like(ga), torch.zeros_like(gb), torch.zeros_like(gc)
        x_fwd = _one_hot(B, C, T, device)
        dz2 = _one_hot(B, C, Tout, device)
        a1 = torch.randint(1, 6, (B, C, T), generator=g, device=device).float()
    elif family != "benign":
        raise ValueError(family)
    return dict(x_fwd=x_fwd.contiguous(), a1=a1.contiguous(), w=w.contiguous(), s1=s1, t1=t1, dz2=dz2.contiguous(), a2=a2.contiguous(),
                ga=ga, gb=gb, gc=gc, oa=oa, ob=ob)


# ------------------------------------------------------------------------------------------------------------------------------
# b. the float64 references
# ------------------------------------------------------------------------------------------------------------------------------
def col(v):
    return v.double()[None, :, None]


def fma32(a, b, c):
    """fmaf(a, b, c) of fp32-valued float64 tensors: the product is exact in float64, one rounding of the sum to fp32"""
    return (a * b + c).float().double()


def pre_of(x, a, b):              # fmaf(x, a, b): the fp32 pre-activation both the clamp and the mask see
    return fma32(x.double(), col(a), col(b))


def affine2(x, x2, a, b, c):      # fmaf(x, a, fmaf(x2, b, c))
    return fma32(x.double(), col(a), fma32(x2.double(), col(b), col(c)))


def conv(x, w, stride, pad):
    return F.conv1d(x, w[:, None, :], stride=stride, padding=pad, groups=x.shape[1])


def adjoints(xin, w, gp, stride, pad):
    """autograd of sum(conv(xin, w) * gp): (d / d xin, d / d w)"""
    xv, wv = xin.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    (conv(xv, wv, stride, pad) * gp).sum().backward()
    return xv.grad, wv.grad


class Reference(NamedTuple):
    xin: torch.Tensor        # relu6f(fmaf(x_fwd, s1, t1)), float64 (fp32-valued)
    y: torch.Tensor          # train forward: conv(xin)                                      [B, C, Tout]
    A_y: torch.Tensor
    ye: torch.Tensor         # eval forward: clamp(conv(x_fwd) oa + ob, 0, 6)
    A_ye: torch.Tensor       # |oa| conv(|x|, |w|) + |ob|
    gp: torch.Tensor         # fmaf(dz2, ga, fmaf(a2, gb, gc))
    xb: torch.Tensor         # relu6f(fmaf(a1, s1, t1)): the weight gradient's operand
    mask: torch.Tensor       # (pre > 0) & (pre < 6) on the fp32 pre of a1, as float64
    dx: torch.Tensor         # mask * d/dxin                                                 [B, C, T]
    A_dx: torch.Tensor
    dw: torch.Tensor         # [C, K]
    A_dw: torch.Tensor
    dw00: torch.Tensor       # sum dz2 * a1 windows (g_mode 0, x_mode 0)
    A_dw00: torch.Tensor


def reference(geo, inp):
    S, pad = geo.stride, geo.pad
    w = inp["w"].double()
    xin = pre_of(inp["x_fwd"], inp["s1"], inp["t1"]).clamp(0, 6)
    y, A_y = conv(xin, w, S, pad), conv(xin.abs(), w.abs(), S, pad)
    x0 = inp["x_fwd"].double()
    ye = (conv(x0, w, S, pad) * col(inp["oa"]) + col(inp["ob"])).clamp(0, 6)
    A_ye = conv(x0.abs(), w.abs(), S, pad) * col(inp["oa"]).abs() + col(inp["ob"]).abs()
    gp = affine2(inp["dz2"], inp["a2"], inp["ga"], inp["gb"], inp["gc"])
    pre = pre_of(inp["a1"], inp["s1"], inp["t1"])
    xb = pre.clamp(0, 6)
    mask = ((pre > 0) & (pre < 6)).double()
    dxin, dw = adjoints(xb, w, gp, S, pad)
    A_dxin, A_dw = adjoints(xb.abs(), w.abs(), gp.abs(), S, pad)
    dw00 = adjoints(inp["a1"].double(), w, inp["dz2"].double(), S, pad)[1]
    A_dw00 = adjoints(inp["a1"].double().abs(), w.abs(), inp["dz2"].double().abs(), S, pad)[1]
    return Reference(xin, y, A_y, ye, A_ye, gp, xb, mask, dxin * mask, A_dxin * mask, dw, A_dw, dw00, A_dw00)


def plain_reference(geo, inp):
    """the same quantities composed the plain way, all in float64: affine, F.hardtanh, F.conv1d, autograd (the gradient with respect
    to a1 divided by s1 is the gradient at the pre-activation, which is what the kernels store)"""
    S, pad = geo.stride, geo.pad
    w = inp["w"].double()
    y = conv(F.hardtanh(inp["x_fwd"].double() * col(inp["s1"]) + col(inp["t1"]), 0.0, 6.0), w, S, pad)
    ye = F.hardtanh(conv(inp["x_fwd"].double(), w, S, pad) * col(inp["oa"]) + col(inp["ob"]), 0.0, 6.0)
    gp = col(inp["ga"]) * inp["dz2"].double() + col(inp["gb"]) * inp["a2"].double() + col(inp["gc"])
    a1 = inp["a1"].double().clone().requires_grad_(True)
    wv = w.clone().requires_grad_(True)
    (conv(F.hardtanh(a1 * col(inp["s1"]) + col(inp["t1"]), 0.0, 6.0), wv, S, pad) * gp).sum().backward()
    return dict(y=y, ye=ye, dx=a1.grad / col(inp["s1"]), dw=wv.grad)


# ------------------------------------------------------------------------------------------------------------------------------
# bars
# ------------------------------------------------------------------------------------------------------------------------------
def bar_out(c, A, ref):
    return c * U * A + U * ref.abs()


def slab_bars(geo, y, bar_y, second, kind):
    """per group [(b0, b1)]: reference and bar of (sum y, sum y * second) over the group's rows.  kind "sq": second = y itself (the
    product carries twice y's error); kind "aux": second is an exact input.  -> ref [G, C, 2], bar [G, C, 2]"""
    refs, bars = [], []
    for b0, b1 in groups(geo):
        yy, bb, ss = y[b0:b1], bar_y[b0:b1], second[b0:b1]
        n = (b1 - b0) * y.shape[2]
        prod = yy * ss
        eb = (2 * yy.abs() * bb + bb * bb if kind == "sq" else ss.abs() * bb) + U * prod.abs()
        r0, r1 = yy.sum((0, 2)), prod.sum((0, 2))
        q0 = bb.sum((0, 2)) + n * U * yy.abs().sum((0, 2))
        q1 = eb.sum((0, 2)) + n * U * prod.abs().sum((0, 2))
        refs.append(torch.stack((r0, r1), -1))
        bars.append(torch.stack((q0, q1), -1))
    return torch.stack(refs), torch.stack(bars)


def bar_dw(regime, geo, A_dw, dw):
    return cn_of(regime, geo.B * geo.Tout) * U * A_dw + U * dw.abs()


def ratio(got, ref, bar):
    """worst |got - ref| / bar over all elements; an element whose bar is 0 (reference and A both 0: a masked output, an empty
    group's sums) must be met exactly -- then inf.  NaN / inf in `got` -> inf."""
    got, ref, bar = got.double(), ref.double(), bar.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    r = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0
