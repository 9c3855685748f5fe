"""decode.ctc_segment (K26, csrc/ctc_segment.hip) and ASRPipeline.segments / transcribe_timed against the float64 oracle of
tests/_ctc_segment_ref.py (itself checked in tests/test_ctc_segment_cpu.py).

Tolerances: the largest errors measured over the parity cases below (tools/bench_ctc_segment.py, profiles/ctc_segment_bench.json:
log_prob 1.05e-5 relative to max(1, |log_prob|) -- on the planted alignments, whose frame probabilities lie within 1e-7 of 1, where
fp32 cannot hold them closer; 4.7e-7 on every other case --, duration 1.8e-5 and log_confidence 5.8e-5 absolute) times 8, rounded up
to one digit.  A boundary (start,
end, word_start, word_end) is compared where the oracle's margin |cdf - 1/2| exceeds MARGIN = 8 x the duration error rounded up
(2e-4, under the cap of 1e-3); every test asserts that it skipped at most 2 % of its boundaries."""
import math
import wave

import numpy as np
import pytest
import torch

import _ctc_segment_ref as R
from voice100_amd import _native as N
from voice100_amd.asr import AudioToTextCTC
from voice100_amd.decode import CTCSegments, ctc_beam_search, ctc_segment
from voice100_amd.infer import ASRPipeline
from voice100_amd.mel import MelSpectrogramAudioTransform

pytestmark = pytest.mark.gpu

LOGP_REL, DUR_ABS, CONF_ABS, MARGIN = 9e-5, 2e-4, 5e-4, 2e-4
UNDECIDED_CAP = 0.02
FIELDS = CTCSegments._fields


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def run(dev, x, lengths, labels, label_lengths, blank=0, sep=1):
    """Two calls (one launch each, equal bits); the fields as numpy arrays."""
    xt, lt = torch.from_numpy(np.asarray(x)).to(dev), torch.from_numpy(np.asarray(labels)).to(dev)
    il = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    ll = None if label_lengths is None else torch.tensor(label_lengths, dtype=torch.int32, device=dev)
    before = N.launch_count()
    out = ctc_segment(xt, il, lt, ll, blank=blank, sep=sep)
    assert N.launch_count() - before == 1
    again = ctc_segment(xt, il, lt, ll, blank=blank, sep=sep)
    for k, a, c in zip(FIELDS, out, again):
        assert (a is None and c is None) or torch.equal(bits(a), bits(c)), k
    return {k: v.cpu().numpy() for k, v in out._asdict().items() if v is not None}


def check(got, ref, cap=UNDECIDED_CAP):
    """Device fields against segment_batch's: integers equal on the decided boundaries, floats within the tolerances, padding zero,
    infeasible rows as the contract says.  Returns the comparison's figures."""
    c = R.compare(got, ref, MARGIN)
    print(c)
    assert c["wrong"] == 0, c
    assert c["undecided"] <= cap * max(c["boundaries"], 1), c
    assert c["log_prob_rel"] <= LOGP_REL and c["duration_abs"] <= DUR_ABS and c["log_confidence_abs"] <= CONF_ABS, c
    feas = ref["feasible"]
    live = np.isfinite(ref["start_margin"])              # inside the row's labels
    assert np.all(got["log_prob"][~feas] == -np.inf) or np.all(np.isnan(ref["log_prob"][~feas]))
    for k in ("start", "end", "duration", "log_confidence"):
        assert not got[k][~live].any(), k                # padding
    bad = live & ~feas[:, None]
    assert not got["start"][bad].any() and not got["end"][bad].any() and not got["duration"][bad].any()
    assert np.all(got["log_confidence"][bad] == -np.inf)
    if "word_first" in ref:
        assert np.array_equal(got["n_words"], ref["n_words"])
        assert np.array_equal(got["word_first"], ref["word_first"]) and np.array_equal(got["word_count"], ref["word_count"])
        wl = np.isfinite(ref["word_start_margin"])
        for k in ("word_start", "word_end", "word_log_confidence"):
            assert not got[k][~wl].any(), k
        wb = wl & ~feas[:, None]
        assert not got["word_start"][wb].any() and not got["word_end"][wb].any() and np.all(got["word_log_confidence"][wb] == -np.inf)
    ok = live & feas[:, None]                            # what holds for every feasible label, decided or not
    assert np.all(got["start"][ok] < got["end"][ok]) and np.all(got["duration"][ok] >= 1 - DUR_ABS)
    assert np.all(got["log_confidence"][ok] <= 0)
    return c


_ORACLE = {}


def parity(T, L, V):
    if (T, L, V) not in _ORACLE:                         # the reference is computed once and shared
        x, labels = R.parity_case(T, L, V)
        _ORACLE[(T, L, V)] = (x, labels, R.segment_batch(x, None, labels, None))
    return _ORACLE[(T, L, V)]


@pytest.mark.parametrize("T,L", R.BASE_GRID + R.SEAMS)
def test_parity_with_the_oracle(cuda, T, L):
    """The base grid at V in {2, 29, 71, 128} and the seams (S = 255 / 257, 1023 / 1025 states; 256 / 257, 512 / 513, 1024 / 1025 pairs of
    states, where a thread takes one pair more) at V = 29; each batch holds
    the logit scales 0.1, 3 and 10.  The share of undecided boundaries is asserted over the (T, L) group."""
    tally = {"boundaries": 0, "undecided": 0}
    for V in (R.CLASSES if (T, L) in R.BASE_GRID else (29,)):
        x, labels, ref = parity(T, L, V)
        c = check(run(cuda, x, None, labels, None), ref, cap=1.0)
        for k in tally:
            tally[k] += c[k]
    assert tally["undecided"] <= UNDECIDED_CAP * max(tally["boundaries"], 1), tally


def test_frame_block_seams(cuda):
    """Lengths around the emission staging block and its multiples, as rows of one batch and as the tensor's own T."""
    FB = N.load().v100_ctc_segment_block()
    assert FB == 16
    lens = [FB - 1, FB, FB + 1, 2 * FB - 1, 2 * FB, 2 * FB + 1, 3 * FB, 3 * FB + 1, 1, 2]
    rng = np.random.default_rng(21)
    T, V, L = 3 * FB + 1, 29, 6
    x = (rng.standard_normal((len(lens), T, V)) * 3).astype(np.float32)
    labels = rng.integers(1, V, (len(lens), L))
    ll = [min(L, (n + 1) // 2) for n in lens]
    check(run(cuda, x, lens, labels, ll), R.segment_batch(x, lens, labels, ll))
    for n in (FB - 1, FB, FB + 1, 2 * FB + 1):
        check(run(cuda, x[:3, :n], None, labels[:3], None), R.segment_batch(x[:3, :n], None, labels[:3], None), cap=0.1)


def test_widest_variant_on_short_rows(cuda):
    """Eight pairs a thread and 128 classes (the largest LDS footprint, above 64 KiB) on a label tensor 1100 wide whose rows are short."""
    rng = np.random.default_rng(29)
    T, V, Lmax = 70, 128, 1100
    x = (rng.standard_normal((3, T, V)) * 3).astype(np.float32)
    labels = rng.integers(1, V, (3, Lmax))
    lens, ll = [70, 33, 17], [30, 0, 9]
    check(run(cuda, x, lens, labels, ll), R.segment_batch(x, lens, labels, ll), cap=0.1)


def test_ragged_batches(cuda):
    rng = np.random.default_rng(22)
    T, V, L = 40, 29, 12
    x = (rng.standard_normal((7, T, V)) * 3).astype(np.float32)
    labels = rng.integers(1, V, (7, L))
    lens = [40, 0, 55, 17, 40, -3, 33]                   # a zero-length row, lengths above T and below 0
    ll = [12, 5, 30, 0, 0, 0, -2]                        # L = 0 with and without frames, above Lmax, below 0
    check(run(cuda, x, lens, labels, ll), R.segment_batch(x, lens, labels, ll))
    check(run(cuda, x, None, labels, ll), R.segment_batch(x, None, labels, ll))
    check(run(cuda, x, lens, labels, None), R.segment_batch(x, lens, labels, None))
    got = run(cuda, x, lens, labels, ll)
    assert got["log_prob"][1] == -np.inf and got["log_prob"][5] == 0.0               # no frame: labels / none
    lp = R.log_softmax(x[3, :17])
    assert abs(got["log_prob"][3] - lp[:, 0].sum()) <= LOGP_REL * abs(lp[:, 0].sum())
    ns = run(cuda, x, lens, labels, ll, sep=None)        # no word level: the label level is the same bits
    assert "word_first" not in ns and all(np.array_equal(ns[k], got[k]) for k in FIELDS[:5])
    dev_x, dev_l = torch.from_numpy(x).to(cuda), torch.from_numpy(labels).to(cuda)
    empty = ctc_segment(dev_x, None, dev_l[:, :0], None)                            # a zero-width labels tensor: every row is empty
    assert empty.start.shape == (7, 0) and empty.word_first.shape == (7, 0) and not empty.n_words.any()
    want = torch.log_softmax(dev_x.double(), -1)[:, :, 0].sum(1)
    assert torch.allclose(empty.log_prob.double(), want, rtol=LOGP_REL, atol=0)
    for bad in (dict(blank=29), dict(blank=-1)):
        with pytest.raises(RuntimeError, match="limits"):
            ctc_segment(dev_x, None, dev_l, None, **bad)
    with pytest.raises(RuntimeError, match="limits"):
        ctc_segment(dev_x[:, :, :1], None, dev_l, None)
    with pytest.raises(RuntimeError):
        ctc_segment(dev_x, None, dev_l[:3], None)


def test_label_patterns(cuda):
    rng = np.random.default_rng(23)
    T, V = 12, 5
    x = (rng.standard_normal((8, T, V)) * 3).astype(np.float32)
    rows = [[1, 1, 2, 2, 2, 3],                          # repeated labels
            [1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4],        # L = T without repeats: exactly one alignment
            [1, 2, 3, 4, 1, 2, 3, 3, 1, 2, 3, 4],        # L = T with a repeat: infeasible
            [1, 2, 5, 3],                                # a label outside [0, V)
            [1, -1, 3],
            [1, 0, 3],                                   # a label equal to blank
            [2, 2, 2, 2, 2, 2, 2],                       # 7 + 6 frames needed
            [3, 1, 4, 1]]
    ll = [len(r) for r in rows]
    labels = np.zeros((8, 12), np.int64)
    for b, r in enumerate(rows):
        labels[b, :len(r)] = r
    ref = R.segment_batch(x, None, labels, ll)
    assert ref["feasible"].tolist() == [True, True, False, False, False, False, False, True]
    got = run(cuda, x, None, labels, ll)
    check(got, ref)
    assert got["start"][1].tolist() == list(range(12)) and got["end"][1].tolist() == list(range(1, 13))
    ref1 = R.segment_batch(x, None, labels, ll, blank=1, sep=3)                  # another blank and separator
    check(run(cuda, x, None, labels, ll, blank=1, sep=3), ref1)


def test_planted_alignments_have_no_undecided_boundary(cuda):
    for L, V in R.PLANTED:
        x, labels, starts, ends = R.planted_case(L, V)
        ref = R.segment_batch(x, None, labels, None)
        got = run(cuda, x, None, labels, None)
        c = check(got, ref, cap=0.0)
        assert c["undecided"] == 0 and got["start"][0].tolist() == starts and got["end"][0].tolist() == ends
        assert np.exp(got["log_confidence"][0]).min() > 0.99


def test_logit_patterns(cuda):
    rng = np.random.default_rng(25)
    T, V, L = 50, 29, 10
    x = (rng.standard_normal((4, T, V)) * 3).astype(np.float32)
    labels = rng.integers(1, V - 1, (4, L))
    x[0, :, V - 1] = -np.inf                             # a class of probability zero that no label needs
    x[1, :, int(labels[1, 4])] = -np.inf                 # ... and one that a label needs: infeasible
    x[2, ::2] *= 30.0                                    # frames of very peaked and of flat posteriors
    ref = R.segment_batch(x, None, labels, None)
    assert ref["feasible"].tolist() == [True, False, True, True]
    check(run(cuda, x, None, labels, None), ref, cap=0.1)
    y = x.copy()
    y[3, 7] = np.nan                                     # a NaN frame: the row ends like any other, the others do not notice
    got, base = run(cuda, y, None, labels, None), run(cuda, x, None, labels, None)
    for k in FIELDS:
        assert np.array_equal(got[k][:3], base[k][:3], equal_nan=True), k
    assert np.all((got["start"][3] >= 0) & (got["start"][3] <= T)) and np.all((got["end"][3] >= 0) & (got["end"][3] <= T))


def test_bounds_canaries_and_padding(cuda):
    """The library called on views inside larger buffers: the canaries around every output stay, and NaN logits / garbage labels
    beyond the rows' lengths change no bit."""
    rng = np.random.default_rng(26)
    B, T, V, Lmax, PAD = 5, 37, 29, 11, 64
    NW = (Lmax + 1) // 2
    lens, ll = [37, 20, 0, 33, 16], [11, 7, 4, 0, 8]
    x = (rng.standard_normal((B, T, V)) * 3).astype(np.float32)
    labels = rng.integers(1, V, (B, Lmax)).astype(np.int64)
    x2, labels2 = x.copy(), labels.copy()
    for b in range(B):
        x2[b, lens[b]:] = np.nan
        labels2[b, ll[b]:] = rng.integers(-2 ** 62, 2 ** 62, Lmax - ll[b])
    il, lt = torch.tensor(lens, dtype=torch.int32, device=cuda), torch.tensor(ll, dtype=torch.int32, device=cuda)
    sizes = [("log_prob", B, torch.float32), ("start", B * Lmax, torch.int32), ("end", B * Lmax, torch.int32),
             ("duration", B * Lmax, torch.float32), ("log_confidence", B * Lmax, torch.float32), ("word_first", B * NW, torch.int32),
             ("word_count", B * NW, torch.int32), ("word_start", B * NW, torch.int32), ("word_end", B * NW, torch.int32),
             ("word_log_confidence", B * NW, torch.float32), ("n_words", B, torch.int32)]

    def call(xa, la):
        nbytes = N.helper("v100_ctc_segment_workspace_bytes", B, T, Lmax)
        ws = torch.full((nbytes + 2 * PAD,), 0x5A, dtype=torch.uint8, device=cuda)
        bufs = [torch.full((n + 2 * PAD,), -77, dtype=dt, device=cuda) for _, n, dt in sizes]
        views = [buf[PAD:PAD + n] for buf, (_, n, _) in zip(bufs, sizes)]
        N.call("v100_ctc_segment", torch.from_numpy(xa).to(cuda), il, torch.from_numpy(la).to(cuda), lt, ws[PAD:PAD + nbytes], *views,
               B, T, V, Lmax, 0, 1)
        torch.cuda.synchronize()
        for (name, n, _), buf in zip(sizes, bufs):
            assert bool((buf[:PAD] == -77).all()) and bool((buf[PAD + n:] == -77).all()), name
        assert bool((ws[:PAD] == 0x5A).all()) and bool((ws[PAD + nbytes:] == 0x5A).all())
        return {name: v.clone() for (name, _, _), v in zip(sizes, views)}

    clean, dirty = call(x, labels), call(x2, labels2)
    for name, _, _ in sizes:
        assert torch.equal(bits(clean[name]), bits(dirty[name])), name
    got = {k: v.cpu().numpy().reshape(B, -1) if v.numel() != B else v.cpu().numpy() for k, v in clean.items()}
    check(got, R.segment_batch(x, lens, labels, ll), cap=0.1)


def test_log_prob_agrees_with_the_ctc_loss_kernel(cuda):
    rng = np.random.default_rng(27)
    B, T, V, L = 6, 80, 29, 20
    x = torch.from_numpy((rng.standard_normal((B, T, V)) * 3).astype(np.float32)).to(cuda)
    labels = torch.from_numpy(rng.integers(1, V, (B, L))).to(cuda)
    il = torch.tensor([80, 64, 33, 80, 10, 50], dtype=torch.int32, device=cuda)
    ll = torch.tensor([20, 12, 16, 1, 15, 0], dtype=torch.int32, device=cuda)        # row 4 has too few frames
    ws = torch.empty((N.helper("v100_ctc_workspace_floats", B, T, L),), dtype=torch.float32, device=cuda)
    nll, grad = torch.empty((B,), dtype=torch.float32, device=cuda), torch.empty_like(x)
    N.call("v100_ctc_loss", x, labels, il, ll, ws, nll, grad, B, T, V, L, 0)
    seg = ctc_segment(x, il, labels, ll)
    a, c = seg.log_prob.cpu().double(), -nll.cpu().double()
    print(a, c)
    assert torch.isinf(a[4]) and torch.isinf(c[4])
    keep = torch.isfinite(c)
    assert torch.all((a[keep] - c[keep]).abs() <= 1e-5 * c[keep].abs().clamp_min(1.0))          # K10 keeps raw fp32 logs: its own error


def test_log_prob_agrees_with_the_exhaustive_beam_search(cuda):
    """V = 3 and T <= 5: at most 63 prefixes, so a beam of 64 holds every transcript; each score is that transcript's log_prob."""
    rng = np.random.default_rng(28)
    for T in (1, 3, 5):
        x = torch.from_numpy((rng.standard_normal((4, T, 3)) * 2).astype(np.float32)).to(cuda)
        ids, lens, scores = ctc_beam_search(x, None, beam_size=64, nbest=64)
        for r in range(64):
            n = lens[:, r]
            if int(n.max()) == 0 and r > 0:
                continue
            seg = ctc_segment(x, None, ids[:, r, :max(int(n.max()), 1)], n)
            s, a = scores[:, r].cpu().double(), seg.log_prob.cpu().double()
            keep = torch.isfinite(s)
            assert torch.all((a[keep] - s[keep]).abs() <= 1e-5 * s[keep].abs().clamp_min(1.0)), (T, r, a, s)


@pytest.fixture(scope="module")
def model(cuda):
    torch.manual_seed(5)
    return AudioToTextCTC(64, 32, 29, 32).to(cuda).eval()


@pytest.mark.parametrize("beam", [None, 4])
def test_pipeline_segments(cuda, model, beam):
    gen = torch.Generator().manual_seed(6)
    feats = (torch.randn(3, 90, 64, generator=gen) * 2 - 4).to(cuda)
    lens = torch.tensor([90, 61, 32], dtype=torch.int32, device=cuda)
    pipe = ASRPipeline(model, beam_size=beam, frame_seconds=0.02)
    for lengths in (None, lens):
        ids, n = pipe(feats, lengths)
        out = pipe.segments(feats, lengths)
        assert torch.equal(out["ids"], ids) and torch.equal(out["ids_len"], n) and out["frame_seconds"] == 0.02
        with torch.no_grad():
            logits = model(feats)
        L = max(int(n.max()), 1)
        want = ctc_segment(logits, None if lengths is None else model.output_length(lens), ids[:, :L], n)
        for k in FIELDS:
            assert torch.equal(bits(out[k]), bits(getattr(want, k))), k
        assert out["start"].shape == (3, L)
        assert pipe.segments(feats, lengths, sep=None)["word_first"] is None
    with pytest.raises(RuntimeError, match="frame_seconds"):
        ASRPipeline(model).segments(feats)


def test_transcribe_timed(cuda, model, tmp_path):
    alphabet = "_ abcdefghijklmnopqrstuvwxyz'"
    decode = lambda ids: "".join(alphabet[int(i)] for i in ids)  # noqa: E731
    rng = np.random.default_rng(7)
    paths, seconds = [], [0.803, 0.45]
    for k, s in enumerate(seconds):
        pcm = (rng.standard_normal(round(16000 * s)) * 3000).astype("<i2")
        paths.append(str(tmp_path / f"utt{k}.wav"))
        with wave.open(paths[-1], "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(pcm.tobytes())
    mel = MelSpectrogramAudioTransform().to(cuda)
    pipe = ASRPipeline(model, mel)
    assert pipe._frame_seconds("segments") == 160 / 16000 * 2
    from voice100_amd.audio_io import load_batch
    out = pipe.segments(*load_batch(paths, 16000, cuda))
    got = pipe.transcribe_timed(paths, decode)
    assert pipe.transcribe(paths, decode) == [g["text"] for g in got]
    fs = out["frame_seconds"]
    for b, g in enumerate(got):
        n = int(out["ids_len"][b])
        assert g["text"] == decode(out["ids"][b, :n].cpu()) and g["log_prob"] == float(out["log_prob"][b])
        assert len(g["words"]) == int(out["n_words"][b]) == len(g["text"].split())
        assert [w["word"] for w in g["words"]] == g["text"].split()
        for w, word in enumerate(g["words"]):
            assert word["start"] == int(out["word_start"][b, w]) * fs
            assert word["end"] == min(int(out["word_end"][b, w]) * fs, round(16000 * seconds[b]) / 16000)
            assert word["confidence"] == pytest.approx(math.exp(float(out["word_log_confidence"][b, w])), rel=1e-6)
            assert 0 <= word["start"] < word["end"] <= seconds[b] and 0 < word["confidence"] <= 1
    assert ASRPipeline(model, mel, frame_seconds=0.5).segments(*load_batch(paths, 16000, cuda))["frame_seconds"] == 0.5
