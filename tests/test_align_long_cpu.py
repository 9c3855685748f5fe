"""CPU-side checks of the long-recording aligner (K29): the two references against each other, the host helper's sizes and limits,
the refusal of CPU tensors, the encoder's receptive field, the window plan of windowed_logits and the utterance reductions."""
import time

import numpy as np
import pytest
import torch

import _align_long_ref as R


@pytest.fixture(scope="module")
def lib():
    from voice100_amd import _native as N
    return N.load()


CASES = [(seed, T, L, V, rep) for seed, (T, L, V, rep) in enumerate([
    (1, 0, 2, False), (3, 1, 2, False), (15, 3, 29, False), (16, 7, 29, True), (17, 8, 29, False), (400, 100, 29, False),
    (400, 100, 29, True), (301, 150, 5, True), (250, 40, 200, False)])]


@pytest.mark.parametrize("seed,T,L,V,rep", CASES)
def test_mirror_equals_float64_viterbi_when_the_band_does_not_bind(seed, T, L, V, rep):
    """band >= n: the fp32 mirror (with its renormalisation every 16 frames) must find the float64 Viterbi's path, and both the
    planted one, on one-hot logits at 20 nats."""
    logits, labels, planted = R.planted(seed, T, L, V, repeats=rep)
    lp = R.log_softmax32(logits)
    band = max(64, -(-(2 * L + 1) // 64) * 64)
    s32, ok32, p32, a32 = R.mirror(lp, labels, band)
    s64, ok64, p64, a64 = R.viterbi_f64(lp, labels)
    assert ok32 == 1 and ok64 == 1
    assert np.array_equal(p32, p64) and np.array_equal(a32, a64)
    assert np.array_equal(p32, planted)
    assert np.array_equal(a32, np.bincount(planted, minlength=2 * L + 1))
    assert abs(s32 - s64) <= 1e-6 * T * np.abs(lp).max()          # T fp32 additions of values below |lp|max, ulp 6e-8 each


def test_mirror_band_binds_free_ends_and_infeasible_rows():
    logits, labels, planted = R.planted(11, 400, 100, 29)
    lp = R.log_softmax32(logits)
    s, ok, p, a = R.mirror(lp, labels, 64)                        # n = 201: the window shifts about 25 times
    assert ok == 1 and np.array_equal(p, planted)
    s, ok, p, a = R.mirror(lp[:90], labels, 256)                  # fewer frames than labels
    assert ok == 0 and s == float("-inf") and not p.any() and not a.any()
    s, ok, p, a = R.mirror(lp[:0], labels, 256)
    assert ok == 0 and p.shape == (0,)
    # free ends: 50 frames of another text on both sides sit in the first and the last blank
    rng = np.random.default_rng(5)
    garbage = lambda: R.planted(int(rng.integers(1 << 30)), 50, 20, 29)[0]  # noqa: E731
    full = R.log_softmax32(np.concatenate([garbage(), logits, garbage()]))
    s, ok, p, a = R.mirror(full, labels, 256, free_logp=full.max(-1))
    # (an end state emits the frame's best symbol, which on the first and the last label's own frames ties with the label: those
    # two runs may be shared with the end states, everything between them is the planted path)
    inner = (planted >= 2) & (planted <= 198)
    assert ok == 1 and np.array_equal(p[50:450][inner], planted[inner]) and not p[:50].any() and (p[450:] == 200).all()
    s0, ok0, p0, _ = R.mirror(full, labels, 256)
    assert s0 < s - 50 * 10                                       # without them the garbage is paid for as blanks


def test_mirror_long_case_is_fast_enough_for_the_gpu_suite():
    """T = 20000, L = 6000, band 512: the case that covers the renormalisation over a long sum must cost the GPU suite under a second."""
    logits, labels, planted = R.planted(3, 20000, 6000, 29)
    lp = R.log_softmax32(logits)
    t0 = time.perf_counter()
    s, ok, p, a = R.mirror(lp, labels, 512)
    dt = time.perf_counter() - t0
    if dt >= 1.0:                                                 # a busy host: the better of two runs
        t0 = time.perf_counter()
        R.mirror(lp, labels, 512)
        dt = min(dt, time.perf_counter() - t0)
    assert ok == 1 and np.array_equal(p, planted)
    assert dt < 1.0, dt


def test_workspace_helper_sizes_and_limits(lib):
    ws = lib.v100_ctc_align_long_workspace_bytes
    blk = lib.v100_ctc_align_long_block()
    assert blk == R.R == 16
    rows = lambda T: (-(-T // blk) * 4 + 15) // 16 * 16           # noqa: E731  the window's start per block, 16-byte rows
    assert ws(1, 1, 0, 64) == 16 + rows(1)
    assert ws(3, 400, 100, 64) == 3 * (400 * 16 + rows(400))
    assert ws(4, 90000, 25000, 2048) == 4 * (90000 * 512 + rows(90000))
    big = ws(2, 1 << 20, 1 << 19, 8192)                           # 64-bit: 4 GiB of moves
    assert big == 2 * ((1 << 20) * 2048 + rows(1 << 20)) and big > 1 << 32
    for bad in ((0, 10, 5, 64), (1, 0, 5, 64), (1, (1 << 20) + 1, 5, 64), (1, 10, -1, 64), (1, 10, (1 << 19) + 1, 64), (1, 10, 5, 0),
                (1, 10, 5, 32), (1, 10, 5, 96), (1, 10, 5, 8192 + 64), (1, 10, 5, -64)):
        assert ws(*bad) == 0, bad
    one = 16
    assert lib.v100_ctc_align_long(None, one, None, None, None, one, one, one, one, one, 1, 10, 29, 5, 64, 0, None) == 3
    assert lib.v100_ctc_align_long(one, one, None, None, None, one, one, one, one, one, 1, 10, 1, 5, 64, 0, None) == 1      # V < 2
    assert lib.v100_ctc_align_long(one, one, None, None, None, one, one, one, one, one, 1, 10, 29, 5, 100, 0, None) == 1    # band


def test_cpu_tensors_are_refused():
    from voice100_amd.decode import ctc_align_long
    from voice100_amd.infer import windowed_logits
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        ctc_align_long(torch.zeros(1, 8, 29), torch.ones(1, 2, dtype=torch.int64))
    from voice100_amd.asr import AudioToTextCTC
    m = AudioToTextCTC(64, 32, 29, 32).eval()
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        windowed_logits(m, torch.zeros(100, 64))
    with pytest.raises(RuntimeError, match="training mode"):
        windowed_logits(m.train(), torch.zeros(100, 64))


def test_receptive_field_is_derived_from_the_layers():
    from voice100_amd.asr import AudioToTextCTC, ConvVoiceEncoder
    enc = ConvVoiceEncoder(64, 32, 32)
    ks = [(int(b.kernel_size), int(b.stride)) for b in enc.layers]
    assert ks == [(11, 2), (19, 1), (27, 1), (35, 1), (51, 1), (59, 1), (67, 1), (75, 1), (83, 1)]
    field, jump = 1, 1
    for k, s in ks:
        field += (k - 1) * jump
        jump *= s
    assert enc.receptive_field() == (field, (field - 1) // 2, jump) == (827, 413, 2)
    assert AudioToTextCTC(64, 32, 29, 32).receptive_field() == (827, 413, 2)
    # probed: a one-layer stack of a different kernel follows its own list, not a constant
    enc.layers = torch.nn.Sequential(enc.layers[0], enc.layers[2])
    assert enc.receptive_field() == (1 + 10 + 2 * 26, 5 + 26, 2)


@pytest.mark.parametrize("M", [1, 2, 799, 800, 801, 802, 1213, 1214, 1215, 4000, 12345])
@pytest.mark.parametrize("keep", [400, 1500])
def test_window_plan_covers_every_output_frame_once(M, keep):
    from voice100_amd.infer import window_plan
    halo, stride = 413, 2
    plan = window_plan(M, keep, halo, stride)
    n_out = (M + 1) // 2
    covered = []
    for i0, i1, skip, count in plan:
        assert i0 % 2 == 0 and 0 <= i0 < i1 <= M and count >= 1
        local_out = (i1 - i0 + 1) // 2
        assert skip + count <= local_out
        g0 = i0 // 2 + skip                                       # the global output frame of the first kept one
        covered.extend(range(g0, g0 + count))
        # every kept frame sees its whole field, or the recording's own edge
        assert i0 == 0 or 2 * g0 - halo >= i0
        assert i1 == M or 2 * (g0 + count - 1) + halo < i1
    assert covered == list(range(n_out))
    assert plan[0][0] == 0 and plan[-1][1] == M
    inner = {i1 - i0 for i0, i1, _, _ in plan[1:-1] if i0 > 0 and i1 < M}
    assert len(inner) <= 1                                        # the windows in between share one shape


def test_utterance_reductions_on_a_hand_made_path():
    from voice100_amd.infer import utterance_cuts
    # 3 labels, utterances [0, 1] and [2]:   frame 0 1 2 3 4 5 6 7 8 9 10 11
    path = torch.tensor([0, 0, 1, 1, 2, 3, 4, 4, 4, 5, 5, 6], dtype=torch.int32)
    lp = -torch.arange(12, dtype=torch.float32)
    out = utterance_cuts(path, lp, [0, 2], 3, conf_window=2, free_ends=True)
    # the last label of the first utterance ends at frame 6 (exclusive), the next begins at 9: the cut is (6 + 9) // 2 = 7
    assert out[:, 0].tolist() == [2.0, 7.0] and out[:, 1].tolist() == [7.0, 11.0] and out[:, 2].tolist() == [5.0, 4.0]
    assert out[0, 3].item() == pytest.approx(-(2 + 3 + 4 + 5 + 6) / 5) and out[1, 3].item() == pytest.approx(-(7 + 8 + 9 + 10) / 4)
    assert out[0, 4].item() == pytest.approx(-(5 + 6) / 2) and out[1, 4].item() == pytest.approx(-(9 + 10) / 2)
    out = utterance_cuts(path, lp, [0, 2], 3, conf_window=30, free_ends=False)
    assert out[:, 0].tolist() == [0.0, 7.0] and out[:, 1].tolist() == [7.0, 12.0]
    assert out[0, 4].item() == pytest.approx(out[0, 3].item()) == pytest.approx(-21 / 7)     # shorter than the window: one window
    for bad in ([], [1], [0, 0], [0, 3], [0, 2, 1]):
        with pytest.raises(ValueError):
            utterance_cuts(path, lp, bad, 3)


def test_align_long_records_lines():
    from voice100_amd.infer import align_long_records
    out = {"utterances": [{"start_s": 0.04, "end_s": 1.5, "min_window_logp": -0.25}, {"start_s": 1.5, "end_s": 2.0, "min_window_logp": -3.0}]}
    lines = align_long_records(out, [3, 4, 5], [0, 2], lambda ids: "".join(chr(96 + int(i)) for i in ids))
    assert lines == ["0.040|1.500|-0.2500|cd", "1.500|2.000|-3.0000|e"]
