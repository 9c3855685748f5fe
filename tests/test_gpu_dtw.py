"""GPU checks of the synthesis scores (K27, csrc/dtw.hip, voice100_amd/metrics.py) against the float64 oracle of tests/_dtw_ref.py.

The kernel's seams, which the length pairs below straddle:
  * the distance pass works in 64 x 64 tiles: lengths 63 / 64 / 65 and 127 / 128 / 129 on either side;
  * the recurrence gives each of the 64 lanes a strip of S reference columns, S the smallest of 1, 2, 4, ... 64 with 64 S >= m: S
    changes between m = 64 | 65, 128 | 129, 256 | 257 (and 512 | 513, inside 1000), 1024 | 1025 (between 1000 and 1100), 2048 | 2049
    (the pair (70, 2100), beyond the issue's list, is the only one on S = 64); a backpointer word holds min(S, 16) cells;
  * the backtrace walks in tiles of 64 rows x 4 backpointer words and hands the path out 64 cells at a time: paths shorter and
    longer than 64 cells, paths that leave a tile through its top (n >> m) and through its left edge (m >> n);
  * the limits: (4096, 300) has Tx at the limit; (1, 1), (1, n), (n, 1) have one row or one column only; lengths 0 give zeros."""
import numpy as np
import pytest
import torch

from _dtw_ref import rates_of, score_batch, totals_of
from conftest import load_golden

pytestmark = pytest.mark.gpu

F0_VALUES = np.array([0.0, 28.0, 29.0, 30.0, 31.0, 32.0, 60.0, 120.0, 240.0], np.float32)  # integers around the floor of 30


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _warp(rng, n, m):
    """m indices into 0 .. n-1, non-decreasing: a smooth random time warp."""
    t = np.linspace(0.0, 1.0, m)
    t = t + 0.12 * np.sin(2 * np.pi * (t * rng.uniform(0.5, 1.5) + rng.rand())) * t * (1 - t) * 4
    return np.clip(np.round(np.maximum.accumulate(t) * (n - 1)), 0, n - 1).astype(np.int64)


def _exact_batch(rng, pairs, Du, skip, Tx=None, Ty=None):
    """Rows constant across the used dimensions, small integers in [0, 8): d = sqrt(Du) |a - b| with Du a perfect square, so every
    distance, every cumulative cost and every f0_sq_hz is exact in fp32 and in fp64, and ties are everywhere.  The skipped leading
    dimensions hold other numbers, which must not count.  y follows a warp of x with a few changed frames."""
    B, D = len(pairs), Du + skip
    Tx = Tx or max(1, max(n for n, _ in pairs))
    Ty = Ty or max(1, max(m for _, m in pairs))
    x, y = np.zeros((B, Tx, D), np.float32), np.zeros((B, Ty, D), np.float32)
    f0x, f0y = np.zeros((B, Tx), np.float32), np.zeros((B, Ty), np.float32)
    for b, (n, m) in enumerate(pairs):
        a = rng.randint(0, 8, max(n, 1))
        w = _warp(rng, max(n, 1), max(m, 1))
        c = np.where(rng.rand(max(m, 1)) < 0.2, rng.randint(0, 8, max(m, 1)), a[w])
        fa = F0_VALUES[rng.randint(0, len(F0_VALUES), max(n, 1))]
        fc = np.where(rng.rand(max(m, 1)) < 0.3, F0_VALUES[rng.randint(0, len(F0_VALUES), max(m, 1))], fa[w])
        x[b, :n, skip:], y[b, :m, skip:] = a[:n, None], c[:m, None]
        x[b, :n, :skip], y[b, :m, :skip] = rng.randn(n, skip), 50 + rng.randn(m, skip)
        f0x[b, :n], f0y[b, :m] = fa[:n], fc[:m]
    xl, yl = np.array([n for n, _ in pairs], np.int32), np.array([m for _, m in pairs], np.int32)
    return x, xl, y, yl, f0x, f0y


def _check(got, ref, Tx, Ty, exact, Du=None, decided=None, what=""):
    """got: a DTWScore with path; ref: the oracle's rows.  exact: every output equals the oracle's (f0_sq_cents, which goes through
    log2, to 1e-9).  Otherwise the cost within (Du + 4) 2^-24 relative, and the path-dependent outputs on the decided rows."""
    cost, plen, voiced, vuv = got.cost.cpu().numpy(), got.path_len.cpu().numpy(), got.voiced.cpu().numpy(), got.vuv_errors.cpu().numpy()
    cents, hz, path = got.f0_sq_cents.cpu().numpy(), got.f0_sq_hz.cpu().numpy(), got.path.cpu().numpy()
    assert path.shape == (len(ref), Tx + Ty - 1, 2) and cost.dtype == np.float64 and plen.dtype == np.int32
    for b, r in enumerate(ref):
        tag = f"{what} row {b}"
        if exact:
            assert cost[b] == r["cost"], tag
        else:
            print(f"{tag}: cost {cost[b]!r} oracle {r['cost']!r} rel {abs(cost[b] - r['cost']) / r['cost']:.3e} "
                  f"bound {(Du + 4) * 2.0 ** -24:.3e} margin {r['margin']:.3e}")
            assert abs(cost[b] - r["cost"]) <= (Du + 4) * 2.0 ** -24 * r["cost"], tag
            if not decided[b]:
                continue
        P = r["path_len"]
        assert plen[b] == P and voiced[b] == r["voiced"] and vuv[b] == r["vuv_errors"], tag
        assert path[b, :P].tolist() == [list(p) for p in r["path"]], tag
        assert not path[b, P:].any(), tag
        assert abs(cents[b] - r["f0_sq_cents"]) <= 1e-9 * r["f0_sq_cents"], tag
        if exact:
            assert hz[b] == r["f0_sq_hz"], tag
        else:
            assert abs(hz[b] - r["f0_sq_hz"]) <= 1e-9 * r["f0_sq_hz"], tag


def _run(cuda, data, skip, dtw=True, **kw):
    from voice100_amd.metrics import dtw_score
    x, xl, y, yl, f0x, f0y = (_dev(a, cuda) for a in data)
    return dtw_score(x, xl, y, yl, f0x, f0y, skip=skip, f0_floor=30.0, dtw=dtw, return_path=True, **kw)


SMALL = [(1, 1), (1, 2), (2, 1), (1, 129), (129, 1), (2, 2), (63, 64), (64, 63), (64, 64), (65, 63), (63, 65), (65, 129), (127, 128),
         (128, 127), (129, 65), (128, 128), (129, 129), (2, 127), (127, 2)]


@pytest.mark.parametrize("Du,skip", [(1, 0), (4, 1), (16, 2), (25, 1)])
def test_exact_small_lengths_and_identity(cuda, Du, skip):
    """Lengths around the 64-wide seams, at every perfect-square Du; then the same batch in identity mode (unequal lengths: the path
    is (i, i) up to the shorter side)."""
    data = _exact_batch(np.random.RandomState(Du), SMALL, Du, skip)
    for dtw in (True, False):
        ref = score_batch(*data, skip=skip, f0_floor=30.0, dtw=dtw)
        _check(_run(cuda, data, skip, dtw), ref, 129, 129, True, what=f"Du {Du} dtw {dtw}")
    assert any(r["vuv_errors"] > 0 for r in ref) and any(r["voiced"] > 0 for r in ref)
    assert sum(r["margin"] == 0.0 for r in score_batch(*data, skip=skip)) > len(SMALL) // 2      # ties on the paths themselves


@pytest.mark.parametrize("pairs,Du", [([(255, 256), (256, 257), (257, 255), (256, 256), (257, 63), (64, 257)], 4),
                                      ([(1000, 1100), (1100, 1000), (1000, 1), (1, 1100), (0, 1100), (1100, 0), (0, 0), (1, 1)], 25),
                                      ([(4096, 300)], 16), ([(70, 2100), (2, 2049)], 1)])
def test_exact_long_lengths(cuda, pairs, Du):
    """The wider strips (S = 4 ... 64), Tx at the limit, and a batch mixing lengths 0, 1 and full."""
    data = _exact_batch(np.random.RandomState(len(pairs)), pairs, Du, 1)
    ref = score_batch(*data, skip=1, f0_floor=30.0)
    _check(_run(cuda, data, 1), ref, data[0].shape[1], data[2].shape[1], True, what=f"{pairs[0]}")
    for r, (n, m) in zip(ref, pairs):
        assert (r["path_len"] == 0) == (n == 0 or m == 0) and (r["path_len"] == 0 or max(n, m) <= r["path_len"] <= n + m - 1)


def test_nan_padding_is_never_read(cuda):
    """Beyond the lengths the features and the f0 tracks hold NaN: the results are those of zero padding, bit for bit."""
    pairs = [(63, 129), (100, 40), (0, 77), (1, 1), (129, 128)]
    data = _exact_batch(np.random.RandomState(7), pairs, 16, 1, Tx=140, Ty=150)
    nan = [a.copy() for a in data]
    for b, (n, m) in enumerate(pairs):
        nan[0][b, n:], nan[2][b, m:], nan[4][b, n:], nan[5][b, m:] = np.nan, np.nan, np.nan, np.nan
    zero, got = _run(cuda, data, 1), _run(cuda, nan, 1)
    for a, c in zip(zero, got):
        assert torch.equal(a, c)
    _check(got, score_batch(*data, skip=1, f0_floor=30.0), 140, 150, True, what="nan padding")
    ident0, ident = _run(cuda, data, 1, dtw=False), _run(cuda, nan, 1, dtw=False)
    for a, c in zip(ident0, ident):
        assert torch.equal(a, c)
    full = _run(cuda, (data[0], None, data[2], None, data[4], data[5]), 1)          # no lengths: the full widths
    _check(full, score_batch(data[0], None, data[2], None, data[4], data[5], skip=1, f0_floor=30.0), 140, 150, True, what="full width")


def _float_batch(rng, B, nmax, mmax, Du, skip):
    """y is a warped, noisy copy of x; f0 tracks with voiced and unvoiced stretches."""
    D = Du + skip
    x, y = np.zeros((B, nmax, D), np.float32), np.zeros((B, mmax, D), np.float32)
    f0x, f0y = np.zeros((B, nmax), np.float32), np.zeros((B, mmax), np.float32)
    xl, yl = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        n, m = (nmax, mmax) if b == 0 else (rng.randint(nmax // 2, nmax + 1), rng.randint(mmax // 2, mmax + 1))
        t = np.arange(n)[:, None] / 9.0
        a = np.sin(t * rng.uniform(0.5, 2.0, D) + rng.rand(D) * 6) + 0.3 * rng.randn(n, D)
        f = np.where(np.sin(np.arange(n) / 11.0 + rng.rand() * 6) > 0.2, 0.0, 120 + 40 * np.sin(np.arange(n) / 17.0) + 3 * rng.randn(n))
        w = _warp(rng, n, m)
        x[b, :n], y[b, :m] = a, a[w] + 0.1 * rng.randn(m, D)
        f0x[b, :n], f0y[b, :m] = f, np.where(rng.rand(m) < 0.05, 0.0, f[w] * (1 + 0.02 * rng.randn(m)))
        xl[b], yl[b] = n, m
    return x, xl, y, yl, f0x, f0y


@pytest.mark.parametrize("Du,skip,nmax,mmax", [(8, 1, 200, 170), (24, 1, 200, 170), (60, 2, 97, 130)])
def test_random_floats_within_the_derived_bound(cuda, Du, skip, nmax, mmax):
    """cost within (Du + 4) 2^-24 relative of the oracle's: each fp32 distance is within (Du/2 + 2) 2^-24 of the exact one (Du
    squares summed in fp32, one root), the minimum over paths inherits that, and the fp64 accumulation adds nothing visible.  A case
    whose decision margin exceeds twice that bound is DECIDED: the device's path must then be the oracle's, and path, path_len and
    the four sums are compared on those.  At most 10 % of the cases may be undecided, asserted on the oracle alone."""
    B = 20
    data = _float_batch(np.random.RandomState(100 + Du), B, nmax, mmax, Du, skip)
    ref = score_batch(*data, skip=skip, f0_floor=30.0)
    decided = [r["margin"] > 2 * (Du + 4) * 2.0 ** -24 for r in ref]
    print(f"Du {Du}: {B - sum(decided)} of {B} cases undecided")
    assert B - sum(decided) <= B // 10
    _check(_run(cuda, data, skip), ref, nmax, mmax, False, Du=Du, decided=decided, what=f"Du {Du}")


def test_totals_and_meter(cuda):
    """Two updates add; the count entries are exact; per_row=False returns None and still adds; compute() gives the oracle's rates."""
    from voice100_amd.metrics import SynthesisScore, dtw_score
    rng = np.random.RandomState(5)
    batches = [_float_batch(rng, 5, 90, 70, 24, 1), _float_batch(rng, 3, 40, 66, 24, 1)]
    rows = [r for d in batches for r in score_batch(*d, skip=1, f0_floor=30.0)]
    want = totals_of(rows)
    meter = SynthesisScore()
    for d in batches:
        x, xl, y, yl, f0x, f0y = (_dev(a, cuda) for a in d)
        assert meter.update(f0x, x, xl, f0y, y, yl) is None
    got = meter.totals.cpu().tolist()
    assert got[0] == want[0] and got[2] == want[2] and got[3] == want[3]              # pairs, voiced, vuv_errors: exact
    assert abs(got[1] - want[1]) <= 28 * 2.0 ** -24 * want[1]
    assert abs(got[4] - want[4]) <= 1e-9 * want[4] and abs(got[5] - want[5]) <= 1e-9 * want[5]
    out, exp = meter.compute(), rates_of(want, 8)
    assert out.keys() == exp.keys() and out["frames"] == exp["frames"] and out["voiced_frames"] == exp["voiced_frames"] and out["utterances"] == 8
    assert abs(out["mcd"] - exp["mcd"]) <= 28 * 2.0 ** -24 * exp["mcd"] and out["vuv_error"] == exp["vuv_error"]
    assert abs(out["f0_rmse_cents"] - exp["f0_rmse_cents"]) <= 1e-9 * exp["f0_rmse_cents"]
    assert abs(out["f0_rmse_hz"] - exp["f0_rmse_hz"]) <= 1e-9 * exp["f0_rmse_hz"]
    # dtw_score itself: totals beside the per-row outputs, which sum to what was added; without f0 only pairs and cost move
    x, xl, y, yl, f0x, f0y = (_dev(a, cuda) for a in batches[1])
    tot = torch.zeros(6, dtype=torch.float64, device=cuda)
    s = dtw_score(x, xl, y, yl, f0x, f0y, skip=1, totals=tot)
    assert s.path is None and tot[0] == s.path_len.sum() and tot[2] == s.voiced.sum() and tot[3] == s.vuv_errors.sum()
    assert abs(float(tot[1]) - float(s.cost.sum())) <= 1e-12 * float(tot[1])
    assert dtw_score(x, xl, y, yl, skip=1, totals=tot, per_row=False) is None
    assert tot[0] == 2 * s.path_len.sum() and tot[2] == s.voiced.sum()
    plain = dtw_score(x, xl, y, yl, skip=1)
    assert plain.voiced is None and plain.f0_sq_hz is None and torch.equal(plain.cost, s.cost) and torch.equal(plain.path_len, s.path_len)
    meter.reset()
    assert meter.compute()["frames"] == 0
    with pytest.raises(RuntimeError):
        dtw_score(x, xl, y, yl, totals=torch.zeros(6, device=cuda))                   # float32 totals
    with pytest.raises(RuntimeError):
        dtw_score(x, xl, y[:, :, :5], yl)                                              # the two D differ
    with pytest.raises(RuntimeError):
        dtw_score(x, xl, y, yl, skip=25)


# ---- the pipelines --------------------------------------------------------------------------------------------------------------

DECODER = [[32, False, 5, 1, 2, False], [32, True, 5, 2, 2, False], [32, False, 5, 1, 2, False]]


def _v2_chain(cuda, S):
    from voice100_amd.infer import TTSPipelineV2
    from voice100_amd.tts_v2 import AlignTextToAudio, TextToAlignText
    from voice100_amd.vocoder import WORLDVocoder
    g = load_golden("tts_v2_tiny.npz")
    ga = g if S == 25 else load_golden("tts_v2_tiny_s257.npz")
    params = lambda d, prefix: {k[len(prefix):]: torch.from_numpy(v) for k, v in d.items() if k.startswith(prefix)}  # noqa: E731
    am = TextToAlignText(29, 2, 32, 2, 1e-3)
    am.load_state_dict(params(g, "align/param/"), strict=True)
    au = AlignTextToAudio(vocab_size=29, logspc_size=S, codeap_size=1, encoder_num_layers=2, encoder_hidden_size=32,
                          decoder_settings=DECODER)
    au.load_state_dict(params(ga, f"audio{S}/param/"), strict=True)
    au = au.to(cuda).eval()
    with torch.no_grad():                                # plausible WORLD statistics: voiced and unvoiced frames both occur
        au.norm.f0_mean.fill_(120.0)
        au.norm.f0_std.fill_(60.0)
        au.norm.logspc_std.fill_(0.2)
    chain = TTSPipelineV2(am.to(cuda).eval(), au, WORLDVocoder(use_mcep=(S == 25)).to(cuda), synthesize=False)
    text, text_len = torch.from_numpy(g["align/text"]).to(cuda), torch.from_numpy(g["align/text_len"]).to(cuda)
    predict = lambda out: au.predict(out["aligntext"], out["aligntext_len"])  # noqa: E731
    return chain, text, text_len, predict


def _v1_chain(cuda):
    from voice100_amd.infer import TTSPipeline
    from voice100_amd.tts import AlignTextToAudioModel, TextToAlignTextModel
    from voice100_amd.vocoder import WORLDVocoder
    torch.manual_seed(4)
    al = TextToAlignTextModel(vocab_size=29, hidden_size=64).to(cuda).eval()
    with torch.no_grad():
        al.layers[4].bias.copy_(torch.tensor([0.6931, 1.3863], device=cuda))
    au = AlignTextToAudioModel(vocab_size=29, hidden_size=64, use_mcep=True).to(cuda).eval()
    with torch.no_grad():
        au.norm.f0_mean.fill_(150.0)
        au.norm.f0_std.fill_(90.0)
    chain = TTSPipeline(al, au, WORLDVocoder(use_mcep=True).to(cuda), synthesize=False)
    text = torch.randint(1, 29, (3, 20), device=cuda)
    predict = lambda out: au.predict(out["aligntext"])[:3]  # noqa: E731
    return chain, text, torch.tensor([20, 11, 16], device=cuda), predict


def _edited_reference(f0, feat, frames):
    """The pipeline's own output with some frames repeated and one dropped, per row: (ref_f0, ref_feat, ref_frames)."""
    B, T = f0.shape
    n = frames.cpu().tolist()
    idx = []
    for b in range(B):
        keep = [i for i in range(n[b]) if i != n[b] // 2] if n[b] > 2 else list(range(n[b]))
        idx.append(sorted(keep + [i for i in keep if i % 7 == 3]))
    Tr = max(1, max(len(r) for r in idx))
    ref_f0, ref_feat = f0.new_zeros((B, Tr)), feat.new_zeros((B, Tr, feat.shape[2]))
    for b, r in enumerate(idx):
        r = torch.tensor(r, dtype=torch.int64, device=f0.device)
        ref_f0[b, :len(r)], ref_feat[b, :len(r)] = f0[b, r], feat[b, r]
    return ref_f0, ref_feat, torch.tensor([len(r) for r in idx], dtype=torch.int32, device=f0.device)


@pytest.mark.parametrize("which", ["v1_mcep", "v2_mcep", "v2_logspc"])
def test_pipeline_score(cuda, which):
    """score() equals dtw_score by hand on the same tensors (on the mel-cepstra of the documented sp2mc conversion for the
    log-spectrum model); an output scored against itself has mcd 0, no voicing error and one pair per frame; evaluate() is the
    loop over score() with one read-back; __call__ gives what it gave."""
    from voice100_amd.metrics import SynthesisScore, dtw_score, mcd_db
    from voice100_amd.vocoder import WORLDVocoder, create_sp2mc_matrix
    chain, text, text_len, predict = _v1_chain(cuda) if which == "v1_mcep" else _v2_chain(cuda, 25 if which == "v2_mcep" else 257)
    with torch.no_grad():
        out = chain(text, text_len)
        f0, feat, _ = predict(out)
    frames = out["frames"]
    assert "wave" not in out and torch.equal(f0, out["f0"])
    if which == "v2_logspc":
        assert feat.shape[2] == 257 and torch.equal(feat, out["logspc"])
        mc = WORLDVocoder(use_mcep=True).to(cuda)
        to_mcep = lambda t: mc.logspc_to_mcep(t.reshape(-1, 257)).reshape(t.shape[0], t.shape[1], 25)  # noqa: E731
        m64 = feat.double().cpu().numpy() @ create_sp2mc_matrix(512, 24, 0.410)
        assert np.abs(to_mcep(feat).double().cpu().numpy() - m64).max() <= 1e-5 * np.abs(m64).max()
    else:
        assert feat.shape[2] == 25
        to_mcep = lambda t: t  # noqa: E731
    ref_f0, ref_feat, ref_frames = _edited_reference(f0, feat, frames)
    meter = SynthesisScore(chain.vocoder)
    res = chain.score(text, text_len, ref_f0, ref_feat, ref_frames, meter=meter)
    hand = dtw_score(to_mcep(feat), frames, to_mcep(ref_feat), ref_frames, f0, ref_f0, skip=1)
    for a, c in zip(res["score"][:6], hand[:6]):
        assert torch.equal(a, c)
    assert torch.equal(res["mcd"], mcd_db(hand.cost, hand.path_len)) and torch.equal(res["frames"], frames)
    assert (hand.path_len >= torch.maximum(frames, ref_frames)).all() and float(hand.cost.sum()) >= 0.0
    want = [float(hand.path_len.sum()), float(hand.cost.sum()), float(hand.voiced.sum()), float(hand.vuv_errors.sum())]
    got = meter.totals.cpu().tolist()
    assert got[0] == want[0] and got[2] == want[2] and got[3] == want[3] and abs(got[1] - want[1]) <= 1e-12 * max(want[1], 1.0)
    own = chain.score(text, text_len, f0, feat, frames)
    assert torch.equal(own["score"].path_len, frames.to(torch.int32)) and float(own["score"].cost.abs().sum()) == 0.0
    assert float(own["mcd"][frames > 0].abs().sum()) == 0.0 and int(own["score"].vuv_errors.sum()) == 0
    rates = chain.evaluate([(text, text_len, ref_f0, ref_feat, ref_frames)] * 2)
    assert rates["frames"] == 2 * int(want[0]) and rates["utterances"] == 2 * text.shape[0]
    assert abs(rates["mcd"] - meter.compute()["mcd"]) <= 1e-12 * max(rates["mcd"], 1.0)
