"""The tables of tests/_dw_f32_cases.py reach what tests/test_gpu_dw_f32_oracle.py relies on them to reach, the float64 reference is
the plain F.conv1d + hardtanh + autograd composition, and fp32 torch on the CPU sits inside every bar the kernels are held to -- so
the bars are reachable by a correct fp32 implementation before any kernel is judged by them.  No GPU: torch on the CPU only.

V100_DW_ORACLE_JSON=<path> makes the last test write its worst error / bar per quantity there (profiles/dw_f32_oracle_errors.json)."""
import json
import os

import pytest
import torch

import _dw_f32_cases as D

PAIRS = [(g.name, f) for g in D.GEOS for f in g.fams]
FP32_TORCH = {}


def test_names_are_unique_and_shapes_fit():
    assert len(D.BY_NAME) == len(D.GEOS)
    for g in D.GEOS:
        assert 1 <= g.G <= g.B and g.Tout >= 1 and g.K % 2 == 1, g.name
        assert set(g.fams) <= set(D.FAMILIES) and {"benign", "spread"} <= set(g.fams), g.name


def test_every_regime_is_hit_and_every_tag_is_the_dispatch():
    hit = {"dwconv": set(), "wgrad": set(), "bwd": set()}
    for g in D.GEOS:
        for op, force, tag in g.rows:
            entry, regime = D.row_regime(g, op, force)
            assert regime == tag, (g.name, op, force, tag, regime)
            hit[entry].add(regime)
    assert hit["dwconv"] == set(D.DWCONV_REGIMES) and hit["wgrad"] == set(D.WGRAD_REGIMES) and hit["bwd"] == set(D.BWD_REGIMES)
    # kinks and sparse run at one geometry of every regime
    for fam in ("kinks", "sparse"):
        seen = {D.row_regime(g, op, force) for g in D.GEOS if fam in g.fams for op, force, _ in g.rows}
        assert seen == {(e, r) for e in hit for r in hit[e]}, fam


def test_the_tables_hold_what_the_kernels_can_get_wrong():
    mfma = [g for g in D.GEOS if any(t == "mfma" for _, _, t in g.rows)]
    assert {g.K for g in mfma} == set(D.SPECIALISED)
    # (-pad) & 3 and the contraction steps of DwMfmaGeom<K, 3> (csrc/depthwise_mfma.h:90): all four offsets, STEPS 1 ... 4
    assert {(-g.pad) & 3 for g in mfma} == {0, 1, 2, 3}
    assert {(g.K + 15 + 3 + 31) // 32 for g in mfma} == {1, 2, 3, 4}
    for K in (5, 47, 83):
        ts = {g.T for g in mfma if g.K == K}
        assert set(D.SPEC_T) <= ts and min(ts) < (K - 1) // 2 < K
    # an empty group, a group of nine rows (the b + 4 prefetch runs off the end), one row per group
    for fam in ("spec", "opener"):
        gs = [g for g in D.GEOS if g.name.startswith(fam)]
        assert any(b0 == b1 for g in gs for b0, b1 in D.groups(g))
        assert any(b1 - b0 == 9 for g in gs for b0, b1 in D.groups(g))
    assert D.groups(D.BY_NAME["spec_k5_emptygroup"]) == [(0, 2), (2, 4), (4, 5), (5, 5)]
    # the R = 4 | 8 switch of the opener's forward from both sides, and the 512-output tile edges
    op = {g.T: g for g in D.GEOS if g.name.startswith("opener_t")}
    assert op[512].Tout == 256 and op[513].Tout == 257 and op[1023].Tout == 512 and op[1025].Tout == 513
    assert {t % 2 for t in op} == {0, 1} and min(op) < 11
    # pad that is not (K - 1) / 2 through the MFMA kernel
    assert {(g.pad, g.Tout) for g in mfma if g.K == 17 and g.name[:4] in ("vali", "full")} == {(0, 130 - 16), (16, 130 + 16)}


@pytest.mark.parametrize("name,family", PAIRS)
def test_reference_is_the_plain_composition(name, family):
    """the reference differs from the all-float64 composition by the fp32 rounding of the on-load transforms only: at most 4 u times
    the same sums over the magnitudes those roundings are relative to (|x s| + |t|, |ga dz2| + |gb a2| + |gc|)"""
    geo = D.BY_NAME[name]
    inp = D.make_inputs(geo, family)
    ref, plain = D.reference(geo, inp), D.plain_reference(geo, inp)
    S, pad = geo.stride, geo.pad
    w = inp["w"].double().abs()
    xmag = (inp["x_fwd"].double() * D.col(inp["s1"])).abs() + D.col(inp["t1"]).abs()
    amag = (inp["a1"].double() * D.col(inp["s1"])).abs() + D.col(inp["t1"]).abs()
    gmag = (D.col(inp["ga"]) * inp["dz2"].double()).abs() + (D.col(inp["gb"]) * inp["a2"].double()).abs() + D.col(inp["gc"]).abs()
    tol = lambda A: 4 * D.U * A + 1e-13 * A          # noqa: E731
    assert bool(((ref.y - plain["y"]).abs() <= tol(D.conv(xmag, w, S, pad))).all())
    assert torch.equal(ref.ye, plain["ye"])
    Ax, Aw = D.adjoints(amag, w, gmag, S, pad)
    pre64 = inp["a1"].double() * D.col(inp["s1"]) + D.col(inp["t1"])
    same = ((pre64 > 0) & (pre64 < 6)).double() == ref.mask          # an fp32 pre within one rounding of a kink may fall the other way
    assert int((~same).sum()) <= 2
    assert bool((((ref.dx - plain["dx"]).abs() <= tol(Ax)) | ~same).all())
    if bool(same.all()):
        assert bool(((ref.dw - plain["dw"]).abs() <= tol(Aw)).all())
    if family == "kinks":           # pre is exact on every second channel and sits on both kinks: clamped forward, zero gradient
        a1 = inp["a1"][:, 0::2]
        on = (a1 == 0) | (a1 == 6)
        assert 0.4 < float(on.float().mean()) < 0.6
        assert bool((ref.mask[:, 0::2][on] == 0).all()) and bool((ref.dx[:, 0::2][on] == 0).all())
    if family == "sparse":          # every forward output is one tap's value
        vals = set(ref.y.unique().tolist())
        assert vals <= set(range(0, geo.K + 1)) and len(vals) > 1


def _note(key, r):
    FP32_TORCH[key] = max(FP32_TORCH.get(key, 0.0), r)
    assert r <= 1.0, (key, r)


@pytest.mark.parametrize("name,family", PAIRS)
def test_fp32_torch_is_inside_every_bar(name, family):
    """fp32 torch (F.conv1d and its autograd, tensor sums) on the operands as the kernels define them, against the float64 reference
    under the TIGHTER of the two bars (c = K + 4, c(n) = n + 4)."""
    geo = D.BY_NAME[name]
    inp = D.make_inputs(geo, family)
    ref = D.reference(geo, inp)
    S, pad, K = geo.stride, geo.pad, geo.K
    w32 = inp["w"]
    c = D.c_of("generic", K)
    y32 = D.conv(ref.xin.float(), w32, S, pad)
    bar_y = D.bar_out(c, ref.A_y, ref.y)
    _note("fwd_train y", D.ratio(y32, ref.y, bar_y))
    sref, sbar = D.slab_bars(geo, ref.y, bar_y, ref.y, "sq")
    s32 = torch.stack([torch.stack((y32[b0:b1].sum((0, 2)), (y32[b0:b1] * y32[b0:b1]).sum((0, 2))), -1) for b0, b1 in D.groups(geo)])
    _note("fwd_train stats", D.ratio(s32, sref, sbar))
    ye32 = (D.conv(inp["x_fwd"], w32, S, pad) * inp["oa"][None, :, None] + inp["ob"][None, :, None]).clamp(0, 6)
    _note("fwd_eval y", D.ratio(ye32, ref.ye, D.bar_out(c, ref.A_ye, ref.ye)))
    dx32, dw32 = D.adjoints(ref.xb.float(), w32, ref.gp.float(), S, pad)
    dx32 = dx32 * ref.mask.float()
    bar_dx = D.bar_out(c, ref.A_dx, ref.dx)
    _note("bwd dx", D.ratio(dx32, ref.dx, bar_dx))
    a1 = inp["a1"]
    sref, sbar = D.slab_bars(geo, ref.dx, bar_dx, a1.double(), "aux")
    s32 = torch.stack([torch.stack((dx32[b0:b1].sum((0, 2)), (dx32[b0:b1] * a1[b0:b1]).sum((0, 2))), -1) for b0, b1 in D.groups(geo)])
    _note("bwd stats", D.ratio(s32, sref, sbar))
    _note("bwd dw", D.ratio(dw32, ref.dw, D.bar_dw("generic", geo, ref.A_dw, ref.dw)))
    dw0032 = D.adjoints(inp["a1"], w32, inp["dz2"], S, pad)[1]
    _note("wgrad00 dw", D.ratio(dw0032, ref.dw00, D.bar_dw("generic", geo, ref.A_dw00, ref.dw00)))


def test_write_fp32_torch_figures():
    """after the table above: the worst error / bar of fp32 torch per quantity (all <= 1, asserted row by row)"""
    assert FP32_TORCH and max(FP32_TORCH.values()) <= 1.0
    print("[dw-f32-cases] fp32 torch on the CPU, worst/bar:", {k: round(v, 4) for k, v in FP32_TORCH.items()})
    path = os.environ.get("V100_DW_ORACLE_JSON")
    if path:
        with open(path, "w") as f:
            json.dump({k: round(v, 4) for k, v in sorted(FP32_TORCH.items())}, f, indent=1)
