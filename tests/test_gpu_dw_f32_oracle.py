"""The fp32-STORAGE depthwise entry points -- v100_dwconv, v100_dwconv_wgrad, v100_dwconv_bwd: the stride-2 opening block of every
step, every block at precision fp32, every shape the `_io` entry points refuse -- checked ELEMENT BY ELEMENT against float64 on the
operands as the kernels define them, in every launch regime (tests/_dw_f32_cases.py: the restated dispatch, the references, the
tables; tests/test_dw_f32_cases_cpu.py shows fp32 torch inside the same bars).

Bars (u = 2^-24; derived, not fitted): output |got - ref| <= c u A + u |ref| with A the same sum over absolute values, c = K + 4 on
the fmaf-chain kernels (dwconv_kernel, up2, generic) and 6 K + 8 on the three-digit MFMA kernel; slab sums and weight gradients: the
sum of the element bars of what is summed + n u sum|terms|.  An element whose bar is 0 -- a masked gradient, an empty group's sums --
must be met exactly.

Harness, every call: inputs sit inside NaN-filled flat buffers with the tensor's last row directly in front of the NaN slack (a read
past the end poisons an output); outputs, stats, partial and dw are NaN-filled with NaN slack on both sides, which must still be NaN
afterwards; every slab row must be finite (an empty group writes zeros); the regime of the restated dispatch is asserted first (for
v100_dwconv_bwd against the number of launches, the one observable of its route); where two routes exist (force_generic,
force_split) both run and each is held to the oracle.  Run with -s for worst / bar of every comparison.

Measured on an MI355X (profiles/dw_f32_oracle_errors.json), worst error / bar over all 206 cases -- no kernel bug found:
  v100_dwconv        mfma: y 0.159, eval y 0.088, dx 0.114, sums 0.036;  s2_r4: y 0.134, eval y 0.155, sums 0.057;
                     s2_r8: y 0.185, eval y 0.158, sums 0.004;  up2: dx 0.173, sums 0.072;  generic: y 0.230, eval y 0.215, dx 0.232, sums 0.077
  v100_dwconv_wgrad  spec 0.127, s2 0.113, generic 0.127 (modes 0, 0: 0.104)
  v100_dwconv_bwd    fused_g1: dx 0.114, dw 0.126, sums 0.023;  fused_slab: dx 0.090, dw 0.003, sums 0.009;  split: dx 0.190, dw 0.127, sums 0.072
fp32 torch on the CPU under the tighter bar: y 0.238, eval y 0.242, dx 0.261, dw 0.160, sums 0.103.  So the three-digit MFMA kernel's
"fp32 accuracy" holds per element: against 6 K + 8 it sits at 0.16, which is 0.16 * (6 K + 8) / (K + 4) < 1 of the fmaf-chain bar too."""
import json
import os

import pytest
import torch

import _dw_f32_cases as D

pytestmark = pytest.mark.gpu

SLACK = 64                    # floats of NaN in front of and behind every tensor (64 * 4 bytes keeps the 16-byte alignment)
NAN = float("nan")
WORST = {}
PAIRS = [(g.name, f) for g in D.GEOS for f in g.fams]


def _native():
    from voice100_amd import _native as N
    N.load()
    return N


class Buf:
    """a tensor inside a NaN-filled flat buffer: `t` is the view handed to the kernel"""

    def __init__(self, shape, device, src=None, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.flat = torch.full((SLACK + n + SLACK,), NAN, device=device, dtype=dtype)
        self.t = self.flat[SLACK:SLACK + n].view(*shape)
        if src is not None:
            self.t.copy_(src)

    def slack_intact(self):
        return bool(torch.isnan(self.flat[:SLACK]).all()) and bool(torch.isnan(self.flat[SLACK + self.n:]).all())


def judge(what, key, got, ref, bar):
    r = D.ratio(got, ref, bar)
    WORST[key] = max(WORST.get(key, 0.0), r)
    print(f"[dw-f32-oracle] {what} {key}: worst/bar = {r:.4f}")
    assert r <= 1.0, f"{what} {key}: worst error / bar = {r:.4f}"


def check_slabs(what, key, geo, slab, ref, bar):
    """[G, C, n] slab: every row finite, a group without rows all zero, each group's sums inside the bar"""
    assert bool(torch.isfinite(slab).all()), f"{what} {key}: a slab row was not written"
    for g, (b0, b1) in enumerate(D.groups(geo)):
        if b0 == b1:
            assert bool((slab[g] == 0).all()), f"{what} {key}: the empty group {g} did not write zeros"
    if ref is not None:
        judge(what, key, slab, ref, bar)


@pytest.fixture(scope="module", autouse=True)
def _dump_worst():
    yield
    path = os.environ.get("V100_DW_ORACLE_JSON")
    if path and WORST:
        with open(path, "w") as f:
            json.dump({k: round(v, 4) for k, v in sorted(WORST.items())}, f, indent=1)


@pytest.mark.parametrize("name,family", PAIRS)
def test_dw_f32_vs_float64(cuda, name, family):
    N = _native()
    geo = D.BY_NAME[name]
    B, G, C, T, K, S, pad, Tout = geo.B, geo.G, geo.C, geo.T, geo.K, geo.stride, geo.pad, geo.Tout
    inp = D.make_inputs(geo, family, cuda)
    ref = D.reference(geo, inp)
    dev = {k: Buf(tuple(v.shape), cuda, v) for k, v in inp.items()}
    i = {k: b.t for k, b in dev.items()}
    a1d = inp["a1"].double()

    def done(what, *outs):
        torch.cuda.synchronize()
        for b in list(dev.values()) + list(outs):
            assert b.slack_intact(), f"{what}: the NaN slack around a tensor was written"

    for op, force, tag in geo.rows:
        entry, regime = D.row_regime(geo, op, force)
        assert regime == tag, (name, op, force, tag, regime)
        what = f"{name} {family} {op}{' forced' if force else ''}"
        key = f"{entry}:{regime}"
        c = D.c_of(regime, K)
        if op == "fwd_train":
            y, st = Buf((B, C, Tout), cuda), Buf((G, C, 2), cuda)
            N.call("v100_dwconv", i["x_fwd"], None, i["w"], i["s1"], i["t1"], None, 1, y.t, None, None, None, 0, st.t, G, B, C, T, Tout,
                   K, S, pad, 0, 1, force)
            done(what, y, st)
            bar_y = D.bar_out(c, ref.A_y, ref.y)
            judge(what, key + " y", y.t, ref.y, bar_y)
            check_slabs(what, key + " stats", geo, st.t, *D.slab_bars(geo, ref.y, bar_y, ref.y, "sq"))
        elif op == "fwd_eval":
            y = Buf((B, C, Tout), cuda)
            N.call("v100_dwconv", i["x_fwd"], None, i["w"], None, None, None, 0, y.t, None, i["oa"], i["ob"], 1, None, G, B, C, T, Tout,
                   K, S, pad, 0, 1, force)
            done(what, y)
            judge(what, key + " eval y", y.t, ref.ye, D.bar_out(c, ref.A_ye, ref.ye))
        elif op == "bwd_data":
            dx, st = Buf((B, C, T), cuda), Buf((G, C, 2), cuda)
            N.call("v100_dwconv", i["dz2"], i["a2"], i["w"], i["ga"], i["gb"], i["gc"], 2, dx.t, i["a1"], i["s1"], i["t1"], 2, st.t, G,
                   B, C, Tout, T, K, 1, K - 1 - pad, 1, S, force)
            done(what, dx, st)
            bar_dx = D.bar_out(c, ref.A_dx, ref.dx)
            judge(what, key + " dx", dx.t, ref.dx, bar_dx)
            check_slabs(what, key + " stats", geo, st.t, *D.slab_bars(geo, ref.dx, bar_dx, a1d, "aux"))
        elif op in ("wgrad", "wgrad00"):
            part, dw = Buf((G, C, K), cuda), Buf((C, K), cuda)
            if op == "wgrad":
                N.call("v100_dwconv_wgrad", i["dz2"], i["a2"], i["ga"], i["gb"], i["gc"], 2, i["a1"], i["s1"], i["t1"], 1, part.t, dw.t,
                       G, B, C, T, Tout, K, S, pad, force)
                want, A = ref.dw, ref.A_dw
            else:
                N.call("v100_dwconv_wgrad", i["dz2"], None, None, None, None, 0, i["a1"], None, None, 0, part.t, dw.t,
                       G, B, C, T, Tout, K, S, pad, force)
                want, A = ref.dw00, ref.A_dw00
            done(what, part, dw)
            check_slabs(what, key + " partial", geo, part.t, None, None)
            judge(what, key + (" dw" if op == "wgrad" else " dw (modes 0, 0)"), dw.t, want, D.bar_dw(regime, geo, A, want))
            acc = part.t[0].clone()
            for g in range(1, G):
                acc = acc + part.t[g]
            assert torch.equal(acc, dw.t), f"{what}: dw is not the sum of its slabs"
        elif op == "bwd":
            dx, st, part, dw = Buf((B, C, T), cuda), Buf((G, C, 2), cuda), Buf((G, C, K), cuda), Buf((C, K), cuda)
            n0 = N.launch_count()
            N.call("v100_dwconv_bwd", i["dz2"], i["a2"], i["w"], i["ga"], i["gb"], i["gc"], i["a1"], i["s1"], i["t1"], dx.t, st.t, part.t,
                   dw.t, G, B, C, T, Tout, K, S, pad, force)
            assert N.launch_count() - n0 == D.launches_bwd(regime), (what, regime, N.launch_count() - n0)
            done(what, dx, st, part, dw)
            # the data half of the split route is whatever v100_dwconv takes for this geometry
            cd = c if regime != "split" else D.c_of(D.row_regime(geo, "bwd_data", 0)[1], K)
            bar_dx = D.bar_out(cd, ref.A_dx, ref.dx)
            judge(what, key + " dx", dx.t, ref.dx, bar_dx)
            check_slabs(what, key + " stats", geo, st.t, *D.slab_bars(geo, ref.dx, bar_dx, a1d, "aux"))
            if regime != "fused_g1":          # one group: the fused kernel's partial IS dw, the workspace stays untouched
                check_slabs(what, key + " partial", geo, part.t, None, None)
            judge(what, key + " dw", dw.t, ref.dw, D.bar_dw(regime, geo, ref.A_dw, ref.dw))
        else:
            raise ValueError(op)
