"""decode.ctc_align_long (K29, csrc/align_long.hip) on the GPU: exact parity with the numpy fp32 mirror (tests/_align_long_ref.py) at
the smallest shapes that exercise each mechanism, LongAlignPipeline against planted truth, and windowed_logits against the whole
forward and the CPU oracle."""
import numpy as np
import pytest
import torch

import _align_long_ref as R

pytestmark = pytest.mark.gpu


def _check(cuda, lp, labels, in_len=None, lab_len=None, band=64, blank=0, free_ends=False):
    """The launch on lp [B, T, V] / labels [B, L] (numpy) against the mirror: every output equal, no exception."""
    from voice100_amd.decode import ctc_align_long
    dev = lambda a, dt: None if a is None else torch.as_tensor(np.asarray(a), dtype=dt).to(cuda)      # noqa: E731
    got = ctc_align_long(torch.from_numpy(lp).to(cuda), torch.from_numpy(labels).to(cuda), dev(in_len, torch.int32), dev(lab_len, torch.int32),
                         band=band, blank=blank, free_ends=free_ends)
    score, ok, path, align = R.mirror_batch(lp, labels, in_len, lab_len, band, blank, free_ends)
    assert got.score.dtype == torch.float64 and got.ok.dtype == torch.int32 and got.path.dtype == torch.int32 and got.align.dtype == torch.int32
    assert np.array_equal(got.ok.cpu().numpy(), ok)
    assert np.array_equal(got.path.cpu().numpy(), path)
    assert np.array_equal(got.align.cpu().numpy(), align[:, :got.align.shape[1]])
    assert np.array_equal(got.score.cpu().numpy(), score), (got.score.cpu().numpy() - score)
    return score, ok, path, align


def _noisy(seed, T, L, V, nats=3.0, **kw):
    """Weakly planted logits: the path is not obvious, so ties in the max, -inf regions and the band all matter."""
    logits, labels, planted = R.planted(seed, max(T, 2 * L + 1), L, V, nats=nats, **kw)
    return R.log_softmax32(logits[:T]), labels


@pytest.mark.parametrize("T", [1, 15, 16, 17, 400])
@pytest.mark.parametrize("L", [0, 1, 100])
def test_parity_with_the_mirror_over_lengths(cuda, T, L):
    """T around the re-centring period and L from nothing to a band that binds (band 64, n = 201: the window shifts ~25 times over
    400 frames); T < L rows are infeasible in both."""
    lp, labels = _noisy(100 * T + L, T, L, 29)
    score, ok, path, align = _check(cuda, lp[None], labels[None], band=64)
    if L <= 1:
        assert ok[0] == 1
    if T == 400 and L == 100:
        assert ok[0] == 1 and path[0].max() == 200
        _check(cuda, lp[None], labels[None], band=256)            # band >= n
    if T < L:
        assert ok[0] == 0 and score[0] == -np.inf and not path.any() and not align.any()


@pytest.mark.parametrize("V", [2, 29, 200, 300])
def test_parity_over_vocabulary_sizes(cuda, V):
    """V = 300 is past the widest row that is staged in LDS (255): the emissions then come from global memory."""
    lp, labels = _noisy(V, 130, 30, V)
    _check(cuda, lp[None], labels[None], band=64)
    _check(cuda, lp[None], labels[None], band=64, blank=V - 1)
    _check(cuda, lp[None], labels[None], band=64, free_ends=True)


def test_parity_repeated_labels_and_clamped_labels(cuda):
    lp, _ = _noisy(7, 60, 3, 29)
    aab = np.array([[5, 5, 9]], np.int64)                         # no skip over the blank between the two 5s
    score, ok, path, align = _check(cuda, lp[None], aab)
    assert ok[0] == 1 and align[0, 2] >= 1
    _check(cuda, lp[None], np.array([[5, 29, -3, 1000, 5, 5]], np.int64))     # labels outside [0, V) read the nearest column
    lp, labels = _noisy(8, 300, 100, 29, repeats=True)
    _check(cuda, lp[None], labels[None], band=64)
    _check(cuda, lp[None], labels[None], band=128)


def test_parity_per_row_lengths(cuda):
    """B = 3 with lengths shorter than the tensors, one row without frames, lengths beyond the tensors (clamped)."""
    rows = [_noisy(20 + b, 200, 40, 29) for b in range(3)]
    lp = np.stack([r[0] for r in rows])
    labels = np.stack([r[1] for r in rows])
    _check(cuda, lp, labels, in_len=[200, 130, 77], lab_len=[40, 17, 0])
    _check(cuda, lp, labels, in_len=[0, 500, 33], lab_len=[40, 90, 40])
    _check(cuda, lp, labels, in_len=[16, 32, 48], lab_len=[-2, 10, 20], free_ends=True)


def test_parity_free_ends_with_garbage_at_both_ends(cuda):
    logits, labels, planted = R.planted(31, 400, 100, 29)
    rng = np.random.default_rng(32)
    garbage = lambda: R.planted(int(rng.integers(1 << 30)), 50, 20, 29)[0]      # noqa: E731
    lp = R.log_softmax32(np.concatenate([garbage(), logits, garbage()]))
    for band in (64, 256):
        score, ok, path, align = _check(cuda, lp[None], labels[None], band=band, free_ends=True)
        inner = (planted >= 2) & (planted <= 198)
        assert ok[0] == 1 and np.array_equal(path[0, 50:450][inner], planted[inner])
        assert not path[0, :50].any() and (path[0, 450:] == 200).all()


def test_parity_long_sum(cuda):
    """T = 20000, L = 6000, band 512: 1250 renormalisations; the score is an fp64 offset plus an fp32 remainder in both."""
    logits, labels, planted = R.planted(3, 20000, 6000, 29, nats=6.0)
    lp = R.log_softmax32(logits)
    score, ok, path, align = _check(cuda, lp[None], labels[None], band=512)
    assert ok[0] == 1 and abs(score[0]) > 1000.0


def test_band_that_loses_the_path_reports_it(cuda):
    """A recording that is all blank: the maximum stays in state 0, the window never moves, and the end of the text is not in it.
    The wider band holds all 201 states and finds the (poor) path."""
    rng = np.random.default_rng(41)
    logits = rng.standard_normal((300, 29)).astype(np.float32)
    logits[:, 0] += 20.0
    lp = R.log_softmax32(logits)
    labels = rng.integers(1, 29, size=(1, 100)).astype(np.int64)
    score, ok, path, align = _check(cuda, lp[None], labels, band=64)
    assert ok[0] == 0 and score[0] == -np.inf and not path.any() and not align.any()
    score, ok, path, align = _check(cuda, lp[None], labels, band=256)
    assert ok[0] == 1 and path[0, -1] >= 199


class _Identity(torch.nn.Module):
    """Stand-in acoustic model: the features ARE the logits (one frame in, one frame out, no context)."""

    def receptive_field(self):
        return 1, 0, 1

    def forward(self, x):
        return x


def _eight_utterances(seed, noise_utt=None):
    rng = np.random.default_rng(seed)
    parts, labels, cuts, paths, off = [], [], [], [], 0
    for u in range(8):
        L = int(rng.integers(5, 12))
        T = int(rng.integers(3 * L, 5 * L)) + 40
        lg, lb, pa = R.planted(seed * 10 + u, T, L, 29)
        if u == noise_utt:
            lg = rng.standard_normal(lg.shape).astype(np.float32)
        parts.append(lg); cuts.append(len(labels)); labels.extend(lb.tolist()); paths.append(pa + 2 * off)
        off += L
    # joining two planted paths: the last blank of one and the first of the next are the same extended position
    return np.concatenate(parts), np.array(labels, np.int64), cuts, np.concatenate(paths)


def test_long_align_pipeline_finds_the_planted_cuts(cuda):
    from voice100_amd.infer import LongAlignPipeline, utterance_cuts
    logits, labels, cuts, path = _eight_utterances(5)
    truth = utterance_cuts(torch.from_numpy(path), torch.zeros(len(path)), cuts, len(labels), 30, free_ends=False)
    pipe = LongAlignPipeline(_Identity().eval(), None, band=64, keep=100, free_ends=False, frame_seconds=0.02)
    out = pipe.align(None, labels, cuts, feats=torch.from_numpy(logits).to(cuda))
    assert out["ok"] and len(out["utterances"]) == 8 and out["frame_seconds"] == 0.02
    assert [u["start_s"] for u in out["utterances"]] == [float(s) * 0.02 for s in truth[:, 0]]
    assert [u["end_s"] for u in out["utterances"]] == [float(e) * 0.02 for e in truth[:, 1]]
    assert [u["frames"] for u in out["utterances"]] == [int(f) for f in truth[:, 2]]
    assert out["utterances"][0]["start_s"] == 0.0 and out["utterances"][-1]["frames"] > 0
    assert all(u["min_window_logp"] <= u["mean_logp"] + 1e-12 <= 1e-12 for u in out["utterances"])
    # one utterance replaced by noise: the text still has to pass through it, and its confidence is the lowest of the eight
    logits, labels, cuts, path = _eight_utterances(5, noise_utt=3)
    out = LongAlignPipeline(_Identity().eval(), None, band=64, keep=100, frame_seconds=0.02).align(
        None, labels, cuts, feats=torch.from_numpy(logits).to(cuda))
    conf = [u["min_window_logp"] for u in out["utterances"]]
    assert out["ok"] and int(np.argmin(conf)) == 3


def test_windowed_logits_against_the_whole_forward_and_the_oracle(cuda):
    """A small AudioToTextCTC in eval mode, M = 4000 mel frames, keep = 400: five windows (the first and the last of their own
    shapes, the three between them one batch).  Both the stitched logits and the single whole forward are held to the CPU oracle forward at the tolerance
    tests/test_gpu_models.py applies to this model's eval logits (rel_err < 1e-4: max |a - b| / max |b|), and the per-frame argmax
    of the two must agree wherever the oracle's top-two margin exceeds twice that tolerance."""
    from conftest import load_golden, sub, rel_err
    from oracle import cnn
    from voice100_amd.asr import AudioToTextCTC
    from voice100_amd.infer import windowed_logits, window_plan
    TOL = 1e-4                                                    # test_gpu_models.py::test_asr_tiny_golden, eval logits
    g = load_golden("asr_tiny.npz")
    m = AudioToTextCTC(audio_size=64, vocab_size=29, embed_size=32, hidden_size=32)
    m.load_state_dict(sub(g, "state/"), strict=True)
    m = m.to(cuda).eval()
    torch.manual_seed(4)
    feats = torch.randn(4000, 64) * 2 - 4
    state = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref = cnn.audio_to_text_ctc_forward(feats[None], state, training=False)[0]
        whole = m(feats[None].to(cuda))[0]
        stitched = windowed_logits(m, feats.to(cuda), keep=400)
    assert len(window_plan(4000, 400, 413, 2)) == 5 and stitched.shape == whole.shape == ref.shape == (2000, 29)
    print("rel_err whole", rel_err(whole, ref), "stitched", rel_err(stitched, ref))
    assert rel_err(whole, ref) < TOL and rel_err(stitched, ref) < TOL
    top2 = ref.topk(2, dim=-1).values
    clear = (top2[:, 0] - top2[:, 1]) > 2 * TOL * float(ref.abs().max())
    left_out = int((~clear).sum())
    print("frames left out of the argmax comparison:", left_out, "of", clear.numel())
    assert left_out < 0.01 * clear.numel()                        # seed 4: 0 of 2000 on the reference run
    a, b = whole.argmax(-1).cpu(), stitched.argmax(-1).cpu()
    assert torch.equal(a[clear], b[clear]) and torch.equal(a[clear], ref.argmax(-1)[clear])
