"""Integer decode / alignment steps on the GPU, bit-exact with the reference:
greedy CTC decoding (argmax + merge_repeated, voice100/text.py:99-104), ctc_best_path forced alignment
(voice100/models/align.py:18-66) and the one-launch forced alignment built on it (ctc_align: path, labels, durations and
score, voice100/align_text.py:39-56), TextToAlignTextModel.align (voice100/models/tts.py:89-110) and the v2
TextToAlignText.align (voice100/models/_align_v2.py:48-73).  edit_distance (K23) has no counterpart in the reference: it scores decoded
ids against reference ids (character / phone and word error counts) without leaving the device.  Neither has ctc_beam_search (K24):
the CTC prefix beam search, n best transcripts with their total log probabilities, where the reference decodes greedily, nor its
fused form (K25): the same search with an lm.NGramLM voting inside every frame's selection, nor ctc_segment (K26): the CTC
forward-backward over the alignments of a given transcript, reduced to time boundaries, durations and confidences per label and word,
nor ctc_align_long (K29): the banded Viterbi that aligns a chapter-length recording to its text, nor ctc_cut_points (K31): where to
cut a recording of any length, at its pauses, into pieces that the beam search and ctc_segment take, nor CTCBeamStream and
ctc_beam_search_long (K32): the beam search kept between calls, so that logits can be pushed chunk by chunk and a recording of any
length is decoded as one utterance, bit for bit what one call over all its frames would give, nor ctc_segment_long and
ctc_corridor (K33): ctc_segment inside a corridor round a path, for recordings of up to 2^20 frames, nor rescore_nbest (K34): the
n-best list of the beam search re-ranked by a word-level n-gram model (lm.WordNGramLM), the second pass."""
import math
from typing import NamedTuple, Optional

import torch

from . import _native as N


def ctc_greedy_decode(logits: torch.Tensor, lengths: torch.Tensor = None, blank: int = 0):
    """logits [B, T, V] fp32 -> (ids [B, T] int64 zero-padded, lens [B] int32)."""
    if not logits.is_cuda:
        raise RuntimeError("ctc_greedy_decode: GPU tensors only")
    logits = logits.contiguous().float()
    B, T, V = logits.shape
    lens = lengths.to(device=logits.device, dtype=torch.int32).contiguous() if lengths is not None else None
    out = torch.empty((B, T), dtype=torch.int64, device=logits.device)
    out_len = torch.empty((B,), dtype=torch.int32, device=logits.device)
    N.call("v100_ctc_greedy_decode", logits, lens, out, out_len, B, T, V, int(blank))
    return out, out_len


def ctc_best_path(log_probs: torch.Tensor, labels: torch.Tensor, input_lengths=None, label_lengths=None, max_move: int = 3):
    """log_probs [B, T, V] fp32, labels [B, L] int64 -> (score [B], path [B, T] int32, best_labels [B, T] int64)."""
    if not log_probs.is_cuda:
        raise RuntimeError("ctc_best_path: GPU tensors only")
    lp = log_probs.contiguous().float()
    B, T, V = lp.shape
    labels = labels.to(device=lp.device, dtype=torch.int64).contiguous()
    L = labels.shape[1]
    il = input_lengths.to(device=lp.device, dtype=torch.int32).contiguous() if input_lengths is not None else None
    ll = label_lengths.to(device=lp.device, dtype=torch.int32).contiguous() if label_lengths is not None else None
    back = torch.empty((B, T, 2 * L + 1), dtype=torch.int16, device=lp.device)
    path = torch.empty((B, T), dtype=torch.int32, device=lp.device)
    score = torch.empty((B,), dtype=torch.float32, device=lp.device)
    N.call("v100_ctc_best_path", lp, labels, il, ll, back, path, score, B, T, V, L, int(max_move))
    ext = torch.zeros((B, 2 * L + 1), dtype=torch.int64, device=lp.device)
    ext[:, 1::2] = labels
    return score, path, torch.gather(ext, 1, path.long())


def ctc_align(log_probs: torch.Tensor, labels: torch.Tensor, input_lengths=None, label_lengths=None, max_move: int = 3):
    """Forced alignment in one launch (K20, csrc/align.hip): log_probs [B, T, V] fp32, labels [B, L] int64 ->
    (score [B], path [B, T] int32, best_labels [B, T] int64, align [B, 2L+1] int32).

    score and path are bit-identical to ctc_best_path; best_labels are the blank-extended labels on the path; align[b, s] is the
    number of frames utterance b spends at extended position s -- the row voice100/align_text.py:49-51 writes.  path and
    best_labels are 0 beyond each input length, align beyond 2 * label_length + 1."""
    if not log_probs.is_cuda:
        raise RuntimeError("ctc_align: GPU tensors only")
    lp = log_probs.contiguous().float()
    B, T, V = lp.shape
    labels = labels.to(device=lp.device, dtype=torch.int64).contiguous()
    L = labels.shape[1]
    il = input_lengths.to(device=lp.device, dtype=torch.int32).contiguous() if input_lengths is not None else None
    ll = label_lengths.to(device=lp.device, dtype=torch.int32).contiguous() if label_lengths is not None else None
    nbytes = N.helper("v100_ctc_align_workspace_bytes", B, T, L)
    if nbytes <= 0:
        raise RuntimeError(f"ctc_align: unsupported shape (T = {T} <= 12000 and 2 L + 1 = {2 * L + 1} <= 4096 are the limits)")
    moves = torch.empty((nbytes,), dtype=torch.uint8, device=lp.device)
    path = torch.empty((B, T), dtype=torch.int32, device=lp.device)
    best = torch.empty((B, T), dtype=torch.int64, device=lp.device)
    align = torch.empty((B, 2 * L + 1), dtype=torch.int32, device=lp.device)
    score = torch.empty((B,), dtype=torch.float32, device=lp.device)
    N.call("v100_ctc_align", lp, labels, il, ll, moves, path, best, align, score, B, T, V, L, int(max_move))
    return score, path, best, align


class CTCLongAlign(NamedTuple):
    """What ctc_align_long returns."""
    score: torch.Tensor                                  # [B] fp64: the best path's log-probability (-inf where ok is 0)
    ok: torch.Tensor                                     # [B] int32: 1 where the end position was live in the last window
    path: torch.Tensor                                   # [B, T] int32: extended positions, 0 beyond each input length
    align: torch.Tensor                                  # [B, 2 L + 1] int32: frames per extended position, 0 beyond 2 * label_length + 1


def ctc_align_long(log_probs: torch.Tensor, labels: torch.Tensor, input_lengths=None, label_lengths=None, band: int = 2048,
                   blank: int = 0, free_ends: bool = False) -> CTCLongAlign:
    """Forced alignment of long recordings in one launch (K29, csrc/align_long.hip): log_probs [B, T, V] fp32 (log_softmax of the
    logits: the kernel holds no transcendentals), labels [B, L] int64 -> CTCLongAlign(score, ok, path, align) of device tensors.

    A banded Viterbi over the standard CTC topology (stay, advance by one, skip the blank between two different labels; ctc_segment's
    topology, not ctc_align's max_move rule).  Only `band` consecutive extended positions are live at a time; every 16 frames the
    window is re-centred on its best position -- it never moves back -- and the scores are renormalised into an fp64 offset, so T
    may be 2^20 frames and L 2^19 labels where ctc_align stops at 12000 frames and 2047 labels.  The band is a heuristic: a wrong
    early maximum can drag the window off the true path, which then ends with ok = 0 (score -inf, path and align zero); widen `band`.
    ok is also 0 where there are fewer frames than labels need, or no frame.  band >= 2 L + 1 is the exact Viterbi.
    free_ends: the first and the last extended position (the blanks around the text) emit log_probs.amax(-1) instead of the blank's
    log-probability, so a spoken preamble or outro that is not in the text can sit there.  (No path can beat a state that emits every
    frame's best symbol, so those two positions are left out when the window looks for its best position.)
    Lengths are clamped to [.., T] / [0, L] on the device; labels outside [0, V) read the nearest column.  Two calls give equal bits.
    Limits: 1 <= T <= 2^20, L <= 2^19, V >= 2, 0 <= blank < V, band a multiple of 64 with 64 <= band <= 8192."""
    given = [t for t in (log_probs, labels, input_lengths, label_lengths) if t is not None]
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in given) or log_probs is None or labels is None:
        raise RuntimeError("ctc_align_long: GPU tensors only")
    if log_probs.dim() != 3 or labels.dim() != 2 or labels.shape[0] != log_probs.shape[0]:
        raise RuntimeError(f"ctc_align_long: log_probs [B, T, V] and labels [B, L] with the same B, got {list(log_probs.shape)} and "
                           f"{list(labels.shape)}")
    lp = log_probs.contiguous().float()
    dev = lp.device
    B, T, V = lp.shape
    band, blank = int(band), int(blank)
    labels = labels.to(device=dev, dtype=torch.int64).contiguous()
    il = input_lengths.to(device=dev, dtype=torch.int32).contiguous() if input_lengths is not None else None
    ll = label_lengths.to(device=dev, dtype=torch.int32).contiguous() if label_lengths is not None else None
    if (il is not None and il.numel() != B) or (ll is not None and ll.numel() != B):
        raise RuntimeError(f"ctc_align_long: input_lengths and label_lengths must have {B} elements")
    width = labels.shape[1]
    if width == 0:                                       # no column: every row is empty
        labels, ll = labels.new_zeros((B, 1)), torch.zeros((B,), dtype=torch.int32, device=dev)
    L = labels.shape[1]
    nbytes = N.helper("v100_ctc_align_long_workspace_bytes", B, T, L, band) if B >= 1 else 0
    if nbytes <= 0 or V < 2 or not 0 <= blank < V:
        raise RuntimeError(f"ctc_align_long: unsupported shape or argument (B = {B} >= 1, 1 <= T = {T} <= 2^20, L = {width} <= 2^19, "
                           f"V = {V} >= 2, 0 <= blank = {blank} < V and band = {band}, a multiple of 64 in [64, 8192], are the limits)")
    free = lp.amax(-1).contiguous() if free_ends else None
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    score = torch.empty((B,), dtype=torch.float64, device=dev)
    ok = torch.empty((B,), dtype=torch.int32, device=dev)
    path = torch.empty((B, T), dtype=torch.int32, device=dev)
    align = torch.empty((B, 2 * L + 1), dtype=torch.int32, device=dev)
    N.call("v100_ctc_align_long", lp, labels, il, ll, free, ws, score, ok, path, align, B, T, V, L, band, blank)
    if width == 0:
        align = align[:, :1]
    return CTCLongAlign(score, ok, path, align)


class CutPoints(NamedTuple):
    """What ctc_cut_points returns: S is the largest number of segments over the batch."""
    start: torch.Tensor                                  # [B, S] int32: first frame of each segment, ascending, 0 beyond n_seg
    end: torch.Tensor                                    # [B, S] int32: one past its last frame
    forced: torch.Tensor                                 # [B, S] int32: 1 where the segment begins at a forced cut (no pause there)
    n_seg: torch.Tensor                                  # [B] int32


def ctc_cut_points(logits: torch.Tensor, lengths: torch.Tensor = None, blank: int = 0, max_frames: int = 3000, min_gap=25,
                   margin: float = 0.0, pad: int = 5, min_frames: int = 50) -> CutPoints:
    """Where to cut long recordings into pieces that fit ctc_beam_search and ctc_segment (K31, csrc/cut_points.hip): logits [B, T, V]
    fp32 (the model's output), lengths [B] or None -> CutPoints(start, end, forced, n_seg) of device tensors.  One read-back, of
    n_seg.max(), sizes S.

    A frame is silent where logits[blank] - max of the others (one fp32 subtraction; NaN is not silent) exceeds `margin`; with
    margin >= 0 its argmax is the blank, and CTC never merges labels across a blank, so the greedy decode of the pieces, concatenated,
    is the greedy decode of the recording wherever no cut is forced.  The recording is trimmed to its non-silent frames (none:
    n_seg = 0); every silent run of min_gap frames or more is a cut (min_gap=None: none, only the splitting below); what lies between
    two cuts and is longer than C = max_frames - 2 pad is split left to right at its longest silent run that leaves min_frames
    frames on both sides and at most C on the left (ties to the latest) or, where there is none, at the first maximum of the margin
    over [a + max(C // 2, min_frames), min(a + C, b - min_frames)]: a forced cut, forced = 1 on the segment that begins there.
    Segments are then widened into the silence around them: by min(pad, half of what they share with a neighbour), by
    min(pad, what is there) at the recording's two ends, not at all on a forced side.  So segments are ascending, disjoint,
    non-empty, at most max_frames long, inside each row's length, and every non-silent frame lies in exactly one.
    tests/_cut_points_ref.py is the rule in numpy; the device equals it exactly, and two calls give equal bits.
    Limits: 1 <= T <= 2^20, 2 <= V <= 128, 0 <= blank < V, 2 <= max_frames <= 4096, pad >= 0, min_frames >= 1,
    max_frames - 2 pad >= 2 min_frames, min_gap >= 1 or None.  Lengths are clamped to [0, T]; nothing beyond a row's length is read."""
    given = [t for t in (logits, lengths) if t is not None]
    if not all(isinstance(t, torch.Tensor) for t in given) or logits is None:
        raise RuntimeError("ctc_cut_points: GPU tensors only")
    if logits.dim() != 3:
        raise RuntimeError(f"ctc_cut_points: logits must be [B, T, V], got {list(logits.shape)}")
    B, T, V = logits.shape                               # (the limits need no device: they are checked first)
    blank, max_frames, pad, min_frames, margin = int(blank), int(max_frames), int(pad), int(min_frames), float(margin)
    gap = 0 if min_gap is None else int(min_gap)
    nbytes = N.helper("v100_ctc_cut_points_workspace_bytes", B, T) if B >= 1 else 0
    if (nbytes <= 0 or not 2 <= V <= 128 or not 0 <= blank < V or not 2 <= max_frames <= 4096 or pad < 0 or min_frames < 1
            or max_frames - 2 * pad < 2 * min_frames or (min_gap is not None and gap < 1) or math.isnan(margin)):
        raise RuntimeError(f"ctc_cut_points: unsupported shape or argument (B = {B} >= 1, 1 <= T = {T} <= 2^20, 2 <= V = {V} <= 128, "
                           f"0 <= blank = {blank} < V, 2 <= max_frames = {max_frames} <= 4096, pad = {pad} >= 0, min_frames = {min_frames} "
                           f">= 1, max_frames - 2 pad >= 2 min_frames, min_gap = {min_gap} >= 1 or None and a margin that is not NaN are "
                           "the limits)")
    if lengths is not None and lengths.numel() != B:
        raise RuntimeError(f"ctc_cut_points: lengths must have {B} elements")
    if not all(t.is_cuda for t in given):
        raise RuntimeError("ctc_cut_points: GPU tensors only")
    logits = logits.contiguous().float()
    dev = logits.device
    lens = lengths.to(device=dev, dtype=torch.int32).contiguous() if lengths is not None else None
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    n_seg = torch.empty((B,), dtype=torch.int32, device=dev)
    N.call("v100_ctc_cut_points", logits, lens, ws, n_seg, B, T, V, blank, max_frames, gap, margin, pad, min_frames)
    S = int(n_seg.max())                                 # the one read-back: the tables are exactly that wide
    start, end, forced = (torch.empty((B, S), dtype=torch.int32, device=dev) for _ in range(3))
    if S > 0:
        N.call("v100_ctc_cut_points_table", ws, start, end, forced, B, T, S, pad)
    return CutPoints(start, end, forced, n_seg)


def align_expand(text: torch.Tensor, align: torch.Tensor, text_len=None, head: int = 5, tail: int = 5):
    """text [B, L] int64, align [B, L, 2] (gap, length) -> (aligntext [B, Tmax] int64 zero-padded, lens [B] int32)."""
    if not text.is_cuda:
        raise RuntimeError("align_expand: GPU tensors only")
    text = text.to(torch.int64).contiguous()
    al = align.to(device=text.device, dtype=torch.float64).contiguous()
    B, L = text.shape
    tl = text_len.to(device=text.device, dtype=torch.int32).contiguous() if text_len is not None else None
    out_len = torch.empty((B,), dtype=torch.int32, device=text.device)
    # pass 1: the lengths only (the output's width depends on the data: ONE read-back), pass 2: the expansion, exactly that wide
    # (pad_sequence semantics: the longest utterance ends at the tensor's edge)
    N.call("v100_align_expand", text, al, tl, None, out_len, B, L, 0, int(head), int(tail))
    tmax = max(int(out_len.max()), 1)
    out = torch.empty((B, tmax), dtype=torch.int64, device=text.device)
    N.call("v100_align_expand", text, al, tl, out, out_len, B, L, tmax, int(head), int(tail))
    return out, out_len


def align_expand_v2(text: torch.Tensor, align: torch.Tensor, text_len=None, head: int = 5, tail: int = 5):
    """TextToAlignText.align (_align_v2.py:48-73) batched: text [B, L] int64, align [B, L, 2] (gap, length) ->
    (aligntext [B, Tmax] int64 zero-padded, lens [B] int32), Tmax = max(lens) (pad_sequence semantics).  See v100_align_expand_v2
    for the integer rules and the one departure (a last span past the length lengthens the row instead of raising)."""
    if not text.is_cuda:
        raise RuntimeError("align_expand_v2: GPU tensors only")
    text = text.to(torch.int64).contiguous()
    al = align.to(device=text.device, dtype=torch.float64).contiguous()
    B, L = text.shape
    if al.shape != (B, L, 2):
        raise RuntimeError(f"align_expand_v2: align must be [{B}, {L}, 2], got {list(al.shape)}")
    tl = text_len.to(device=text.device, dtype=torch.int32).contiguous() if text_len is not None else None
    out_len = torch.empty((B,), dtype=torch.int32, device=text.device)
    # pass 1: the lengths only (ONE read-back sizes the output), pass 2: the expansion, exactly that wide
    N.call("v100_align_expand_v2", text, al, tl, None, out_len, B, L, 0, int(head), int(tail))
    tmax = max(int(out_len.max()), 1)
    out = torch.empty((B, tmax), dtype=torch.int64, device=text.device)
    N.call("v100_align_expand_v2", text, al, tl, out, out_len, B, L, tmax, int(head), int(tail))
    return out, out_len


def _edit_distance_launch(name, hyp, hyp_len, ref, ref_len, levels, sep, totals, per_row):
    if not (hyp.is_cuda and ref.is_cuda and hyp_len.is_cuda and ref_len.is_cuda) or (totals is not None and not totals.is_cuda):
        raise RuntimeError(f"{name}: GPU tensors only")
    if hyp.dim() != 2 or ref.dim() != 2 or hyp.shape[0] != ref.shape[0] or hyp.shape[0] < 1:
        raise RuntimeError(f"{name}: hyp [B, Th] and ref [B, Tr] with the same B >= 1, got {list(hyp.shape)} and {list(ref.shape)}")
    dev = hyp.device
    B = hyp.shape[0]
    nl = 2 if levels == 3 else 1
    if not per_row and totals is None:
        raise RuntimeError(f"{name}: nothing to compute (per_row=False and no totals)")
    if totals is not None and (totals.dtype != torch.int64 or totals.numel() != 3 * nl or not totals.is_contiguous()):
        raise RuntimeError(f"{name}: totals must be a contiguous int64 tensor of {3 * nl} elements")
    hyp, ref = hyp.to(torch.int64).contiguous(), ref.to(device=dev, dtype=torch.int64).contiguous()
    hl, rl = hyp_len.to(device=dev, dtype=torch.int32).contiguous(), ref_len.to(device=dev, dtype=torch.int32).contiguous()
    if hl.numel() != B or rl.numel() != B:
        raise RuntimeError(f"{name}: hyp_len and ref_len must have {B} elements")
    if hyp.shape[1] == 0:                                # no column: every row is empty
        hyp, hl = hyp.new_zeros((B, 1)), torch.zeros_like(hl)
    if ref.shape[1] == 0:
        ref, rl = ref.new_zeros((B, 1)), torch.zeros_like(rl)
    Th, Tr = hyp.shape[1], ref.shape[1]
    nbytes = N.helper("v100_edit_distance_workspace_bytes", B, Th, Tr)
    if nbytes <= 0:
        raise RuntimeError(f"{name}: unsupported shape (Th = {Th} <= 4096 and Tr = {Tr} <= 4096 are the limits)")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    out = tuple(torch.empty((nl, B), dtype=torch.int32, device=dev) for _ in range(3)) if per_row else (None, None, None)
    N.call("v100_edit_distance", hyp, hl, ref, rl, ws, out[0], out[1], out[2], totals, B, Th, Tr, int(levels), int(sep))
    return out if per_row else None


def edit_distance(hyp: torch.Tensor, hyp_len: torch.Tensor, ref: torch.Tensor, ref_len: torch.Tensor, sep=None, totals=None,
                  per_row: bool = True):
    """Batched Levenshtein distance in one launch (K23, csrc/edit_distance.hip): hyp [B, Th] int64 with hyp_len [B], ref [B, Tr] int64
    with ref_len [B] -> (dist, hyp_n, ref_n), each [B] int32.  Unit costs; lengths are clamped to [0, width] on the device and
    nothing beyond a row's length is read; ids compare on all 64 bits; Th, Tr <= 4096.

    sep=None: a token is one id (hyp_n / ref_n are the lengths).  sep=<id>: a token is a maximal run of ids != sep inside the row's
    length -- str.split() on the decoded text -- and two words are equal iff they have the same length and the same ids.
    totals: an int64 GPU tensor of 3 elements INTO which the launch adds the batch sums of (dist, hyp_n, ref_n); no read-back.
    per_row=False (with totals): only the totals are computed, and None is returned."""
    out = _edit_distance_launch("edit_distance", hyp, hyp_len, ref, ref_len, 1 if sep is None else 2, 0 if sep is None else sep,
                                totals, per_row)
    return None if out is None else (out[0][0], out[1][0], out[2][0])


def edit_distance_both(hyp: torch.Tensor, hyp_len: torch.Tensor, ref: torch.Tensor, ref_len: torch.Tensor, sep: int = 1, totals=None,
                       per_row: bool = True):
    """edit_distance at both levels from ONE launch: (dist, hyp_n, ref_n), each [2, B] int32 -- row 0 the id level (characters,
    the separator counted like any other id), row 1 the word level with separator `sep`.  totals: int64 [2, 3], added into."""
    out = _edit_distance_launch("edit_distance_both", hyp, hyp_len, ref, ref_len, 3, sep, totals, per_row)
    return out


def _beam_lm_tables(who, lm, device, V, blank, lm_weight, length_bonus):
    """The checks that ctc_beam_search and CTCBeamStream make on a language model and its weights; (logp, next, final, S, alpha, beta)
    as the kernel takes them."""
    tables = (getattr(lm, "logp", None), getattr(lm, "next", None), getattr(lm, "final", None))
    if any(t is None for t in tables):
        raise RuntimeError(f"{who}: the language model is not compiled (NGramLM.compile().to(device) first)")
    logp, nxt, fin = tables
    if logp.dim() != 2 or logp.shape[0] < 1 or nxt.shape != logp.shape or fin.shape != logp.shape[:1]:
        raise RuntimeError(f"{who}: the language model is empty or malformed (logp {list(logp.shape)}, next "
                           f"{list(nxt.shape)}, final {list(fin.shape)}; [S, V], [S, V], [S] with S >= 1 expected)")
    if any(t.device != device for t in tables):
        raise RuntimeError(f"{who}: the language model is on {logp.device}, the logits on {device} (lm.to(device))")
    S = logp.shape[0]
    if logp.shape[1] != V or S * V > 1 << 28 or not 0 <= int(lm.start) < S or blank != int(lm.blank):
        raise RuntimeError(f"{who}: the language model has V = {logp.shape[1]}, blank = {lm.blank}, S = {S} and start state "
                           f"{lm.start}; V = {V}, blank = {blank}, S V <= 2^28 and 0 <= start < S are required")
    alpha, beta = float(lm_weight), float(length_bonus)
    if not (math.isfinite(alpha) and math.isfinite(beta)):
        raise RuntimeError(f"{who}: lm_weight = {alpha} and length_bonus = {beta} must be finite")
    return logp.contiguous().float(), nxt.contiguous().to(torch.int32), fin.contiguous().float(), S, alpha, beta


def ctc_beam_search(logits: torch.Tensor, lengths: torch.Tensor = None, beam_size: int = 16, nbest: int = 1, blank: int = 0, lm=None,
                    lm_weight: float = 0.5, length_bonus: float = 0.0, use_eos: bool = True):
    """CTC prefix beam search in one launch (K24, csrc/beam.hip): logits [B, T, V] fp32 (the model's output, as ctc_greedy_decode takes
    it; the kernel normalises) -> (ids [B, nbest, T] int64 zero-padded, lens [B, nbest] int32, scores [B, nbest] fp32), best first.

    A score is the total log probability of the transcript (the sum over all its alignments, not the best one).  Where the beam holds
    fewer than nbest hypotheses the score is -inf and the length 0; a row of length 0 gives the empty hypothesis with score 0.
    lengths are clamped to [0, T] on the device and nothing beyond a row's length is read.  Ties break on the candidate index, so two
    calls give equal bits.  Limits: 1 <= beam_size <= 64, 2 <= V <= 128, 1 <= nbest <= beam_size, 0 <= blank < V, 1 <= T <= 4096.

    lm: a compiled lm.NGramLM on the logits' device (K25, shallow fusion inside the launch).  The beam is then ranked, in every frame,
    by score = log p_ctc + lm_weight * log p_lm + length_bonus * length, with use_eos the LM's end-of-sentence probability enters
    before the final ranking, and the call returns (ids, lens, scores, ctc_scores, lm_scores): ctc_scores is what the call without an
    LM reports for the same transcript, lm_scores the LM's log probability of it; -inf, -inf, 0 where there is no hypothesis."""
    if not logits.is_cuda or (lengths is not None and not lengths.is_cuda):
        raise RuntimeError("ctc_beam_search: GPU tensors only")
    if logits.dim() != 3:
        raise RuntimeError(f"ctc_beam_search: logits must be [B, T, V], got {list(logits.shape)}")
    logits = logits.contiguous().float()
    B, T, V = logits.shape
    W, nbest, blank = int(beam_size), int(nbest), int(blank)
    nbytes = N.helper("v100_ctc_beam_workspace_bytes", B, T, V, W) if B >= 1 else -1
    if nbytes <= 0 or not 1 <= nbest <= W or not 0 <= blank < V:
        raise RuntimeError(f"ctc_beam_search: unsupported shape or argument (B = {B} >= 1, 1 <= T = {T} <= 4096, 2 <= V = {V} <= 128, "
                           f"1 <= beam_size = {W} <= 64, 1 <= nbest = {nbest} <= beam_size and 0 <= blank = {blank} < V are the limits)")
    lens = lengths.to(device=logits.device, dtype=torch.int32).contiguous() if lengths is not None else None
    if lens is not None and lens.numel() != B:
        raise RuntimeError(f"ctc_beam_search: lengths must have {B} elements")
    if lm is not None:
        logp, nxt, fin, S, alpha, beta = _beam_lm_tables("ctc_beam_search", lm, logits.device, V, blank, lm_weight, length_bonus)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=logits.device)
    ids = torch.empty((B, nbest, T), dtype=torch.int64, device=logits.device)
    ids_len = torch.empty((B, nbest), dtype=torch.int32, device=logits.device)
    scores = torch.empty((B, nbest), dtype=torch.float32, device=logits.device)
    if lm is None:
        N.call("v100_ctc_beam_search", logits, lens, ws, ids, ids_len, scores, B, T, V, W, nbest, blank)
        return ids, ids_len, scores
    ctc_scores, lm_scores = torch.empty_like(scores), torch.empty_like(scores)
    N.call("v100_ctc_beam_search_lm", logits, lens, ws, ids, ids_len, scores, logp, nxt, fin, S, int(lm.start), alpha, beta,
           int(bool(use_eos)), ctc_scores, lm_scores, B, T, V, W, nbest, blank)
    return ids, ids_len, scores, ctc_scores, lm_scores


class CTCBeamStream:
    """ctc_beam_search without a frame limit (K32, the resumable form of csrc/beam.hip): the beam survives between calls, so logits
    can be pushed as they arrive, and any split of a recording into pushes gives ctc_beam_search's result on all the frames bit for
    bit -- the beam is not restarted, the language model keeps one context, no word is split.

        s = CTCBeamStream(batch, vocab, beam_size, lm=lm, max_frames=90000)
        s.push(logits [B, T, V], lengths)      any 1 <= T <= 4096 per call; row b runs clamp(lengths[b], 0, T) more frames
        s.hypotheses(nbest)                    the n best so far, ctc_beam_search's tuple (five tensors with an LM)
        s.finish(nbest)                        the same with the LM's end-of-sentence term (use_eos), and the stream is closed

    hypotheses() runs no frame and stores nothing: it may be called at any time, and twice.  Its ids are [B, nbest, frames pushed],
    zero padded; without final=True the end-of-sentence term is left out, whatever use_eos says.  Reading the labels back is one
    dependent load per label of each hypothesis, so reading after every short push of a long recording costs more than the pushes.
    A row whose length is 0 in a push keeps its state untouched.

    Memory: the prefix trie must persist (the beam's common prefix does not grow: old hypotheses with one early deletion are never
    displaced), and its table's size enters the hash, so the capacity max_frames is fixed here: per row 4 (1 + W max_frames) bytes of
    nodes and 8 bytes per slot of the power of two >= 2 W max_frames, 20 to 36 bytes x beam_size x max_frames -- 30 to 50 MB for
    a 30-minute recording (90000 frames) at beam 16.  Every push counts its T frames against max_frames, whatever the lengths say,
    and a push beyond it raises before anything is launched.  beam_size x max_frames < 2^25 (524k frames at beam 64, 2M at 16).
    The other limits, and the checks on the arguments, are ctc_beam_search's."""

    def __init__(self, batch: int, vocab: int, beam_size: int = 16, blank: int = 0, lm=None, lm_weight: float = 0.5,
                 length_bonus: float = 0.0, use_eos: bool = True, max_frames: int = 65536, device=None):
        if device is None:
            device = lm.logp.device if getattr(lm, "logp", None) is not None else "cuda"
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("CTCBeamStream: GPU tensors only")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        B, V, W, F, blank = int(batch), int(vocab), int(beam_size), int(max_frames), int(blank)
        nbytes = N.helper("v100_ctc_beam_stream_workspace_bytes", B, F, V, W)
        if nbytes <= 0 or not 0 <= blank < V:
            raise RuntimeError(f"CTCBeamStream: unsupported shape or argument (batch = {B} >= 1, 2 <= vocab = {V} <= 128, 1 <= beam_size "
                               f"= {W} <= 64, max_frames = {F} >= 1 with beam_size * max_frames < 2^25 and 0 <= blank = {blank} < "
                               "vocab are the limits)")
        self.lm = None
        if lm is not None:
            self.lm = _beam_lm_tables("CTCBeamStream", lm, device, V, blank, lm_weight, length_bonus) + (int(lm.start),)
        self.batch, self.vocab, self.beam_size, self.blank, self.max_frames, self.device = B, V, W, blank, F, device
        self.use_eos, self.frames, self.closed = bool(use_eos), 0, False
        self._ws = torch.zeros((nbytes,), dtype=torch.uint8, device=device)
        self._state = torch.zeros((N.helper("v100_ctc_beam_stream_state_bytes", B, W),), dtype=torch.uint8, device=device)

    def push(self, logits: torch.Tensor, lengths: torch.Tensor = None) -> None:
        if self.closed:
            raise RuntimeError("CTCBeamStream.push: the stream is finished")
        if not logits.is_cuda or (lengths is not None and not lengths.is_cuda):
            raise RuntimeError("CTCBeamStream.push: GPU tensors only")
        B, V = self.batch, self.vocab
        if logits.dim() != 3 or logits.shape[0] != B or logits.shape[2] != V or not 1 <= logits.shape[1] <= 4096:
            raise RuntimeError(f"CTCBeamStream.push: logits must be [{B}, T, {V}] with 1 <= T <= 4096, got {list(logits.shape)}")
        if logits.device != self.device:
            raise RuntimeError(f"CTCBeamStream.push: the logits are on {logits.device}, the stream on {self.device}")
        T = logits.shape[1]
        if self.frames + T > self.max_frames:
            raise RuntimeError(f"CTCBeamStream.push: {self.frames} frames pushed and {T} more exceed max_frames = {self.max_frames}")
        logits = logits.contiguous().float()
        lens = lengths.to(device=self.device, dtype=torch.int32).contiguous() if lengths is not None else None
        if lens is not None and lens.numel() != B:
            raise RuntimeError(f"CTCBeamStream.push: lengths must have {B} elements")
        if self.lm is None:
            N.call("v100_ctc_beam_stream_push", logits, lens, self._ws, self._state, B, T, self.max_frames, V, self.beam_size, self.blank)
        else:
            logp, nxt, fin, S, alpha, beta, start = self.lm
            N.call("v100_ctc_beam_stream_push_lm", logits, lens, self._ws, self._state, logp, nxt, fin, S, start, alpha, beta, B, T,
                   self.max_frames, V, self.beam_size, self.blank)
        self.frames += T

    def hypotheses(self, nbest: int = 1, final: bool = False):
        if self._ws is None:
            raise RuntimeError("CTCBeamStream.hypotheses: the stream is finished")
        B, W, nbest = self.batch, self.beam_size, int(nbest)
        if not 1 <= nbest <= W:
            raise RuntimeError(f"CTCBeamStream.hypotheses: 1 <= nbest = {nbest} <= beam_size = {W} is required")
        width = max(self.frames, 1)                      # before the first push the ids are [B, nbest, 0]: a view of one column
        ids = torch.empty((B, nbest, width), dtype=torch.int64, device=self.device)
        ids_len = torch.empty((B, nbest), dtype=torch.int32, device=self.device)
        scores = torch.empty((B, nbest), dtype=torch.float32, device=self.device)
        if self.lm is None:
            N.call("v100_ctc_beam_stream_read", self._ws, self._state, ids, ids_len, scores, B, self.max_frames, self.vocab, W, nbest, width)
            return ids[:, :, :self.frames], ids_len, scores
        _, _, fin, S, alpha, beta, start = self.lm
        ctc_scores, lm_scores = torch.empty_like(scores), torch.empty_like(scores)
        N.call("v100_ctc_beam_stream_read_lm", self._ws, self._state, ids, ids_len, scores, fin, S, start, alpha, beta,
               int(bool(final) and self.use_eos), ctc_scores, lm_scores, B, self.max_frames, self.vocab, W, nbest, width)
        return ids[:, :, :self.frames], ids_len, scores, ctc_scores, lm_scores

    def finish(self, nbest: int = 1):
        """hypotheses(nbest, final=True); the stream is closed and its buffers are released."""
        out = self.hypotheses(nbest, final=True)
        self.closed, self._ws, self._state = True, None, None
        return out


def beam_chunk_plan(T: int, chunk: int):
    """How ctc_beam_search_long cuts T frames: [(start, frames)], `chunk` frames each but the last, every frame exactly once."""
    if T < 1 or not 1 <= chunk <= 4096:
        raise ValueError("beam_chunk_plan: T >= 1 and 1 <= chunk <= 4096 are required")
    return [(start, min(chunk, T - start)) for start in range(0, T, chunk)]


def beam_chunk_lengths(lengths: torch.Tensor, start: int, frames: int) -> torch.Tensor:
    """The rows' lengths inside the chunk [start, start + frames): clamp(length - start, 0, frames)."""
    return (lengths - start).clamp(0, frames)


def ctc_beam_search_long(logits: torch.Tensor, lengths: torch.Tensor = None, beam_size: int = 16, nbest: int = 1, blank: int = 0,
                         lm=None, lm_weight: float = 0.5, length_bonus: float = 0.0, use_eos: bool = True, chunk: int = 4096):
    """ctc_beam_search on any number of frames: a CTCBeamStream sized for T, one push per `chunk` frames (beam_chunk_plan; row b has
    clamp(length_b - start, 0, frames) frames in a chunk), then finish(nbest).  Arguments, return values and their shapes are
    ctc_beam_search's, and so are the bits, whatever `chunk` is: at T <= 4096 the two calls agree exactly.  One workgroup per row
    walks its frames one after the other (K24's 3 to 11 us a frame), so a long recording is decoded serially: much slower than
    LongASRPipeline.segments' batch of pieces, and exact, with one language-model context.
    Limits: ctc_beam_search's on B, V, beam_size, nbest and blank; T >= 1 with beam_size * T < 2^25; 1 <= chunk <= 4096.
    Memory: see CTCBeamStream (20 to 36 bytes x beam_size x T per row)."""
    if not logits.is_cuda or (lengths is not None and not lengths.is_cuda):
        raise RuntimeError("ctc_beam_search_long: GPU tensors only")
    if logits.dim() != 3:
        raise RuntimeError(f"ctc_beam_search_long: logits must be [B, T, V], got {list(logits.shape)}")
    B, T, V = logits.shape
    W, nbest, blank, chunk = int(beam_size), int(nbest), int(blank), int(chunk)
    if B < 1 or T < 1 or not 1 <= nbest <= W or not 1 <= chunk <= 4096:
        raise RuntimeError(f"ctc_beam_search_long: unsupported shape or argument (B = {B} >= 1, T = {T} >= 1, 1 <= nbest = {nbest} <= "
                           f"beam_size = {W} and 1 <= chunk = {chunk} <= 4096 are the limits)")
    lens = lengths.to(device=logits.device, dtype=torch.int32).contiguous() if lengths is not None else None
    if lens is not None and lens.numel() != B:
        raise RuntimeError(f"ctc_beam_search_long: lengths must have {B} elements")
    stream = CTCBeamStream(B, V, W, blank, lm, lm_weight, length_bonus, use_eos, max_frames=T, device=logits.device)
    for start, frames in beam_chunk_plan(T, chunk):
        stream.push(logits[:, start:start + frames], None if lens is None else beam_chunk_lengths(lens.reshape(-1), start, frames))
    return stream.finish(nbest)


class Rescored(NamedTuple):
    """What rescore_nbest returns, best first after the second pass."""
    ids: torch.Tensor                                    # [B, nbest, T] int64: the hypotheses' rows as given, re-ordered
    lens: torch.Tensor                                   # [B, nbest] int32
    scores: torch.Tensor                                 # [B, nbest] fp32: first + lm_weight * word LM + word_bonus * words; -inf: none
    first_scores: torch.Tensor                           # [B, nbest] fp32: the first-pass scores as given, re-ordered
    word_lm_scores: torch.Tensor                         # [B, nbest] fp32: the word model's log probability; 0 where there is no hypothesis
    n_words: torch.Tensor                                # [B, nbest] int32
    n_oov: torch.Tensor                                  # [B, nbest] int32: words that are not in the model's vocabulary
    order: torch.Tensor                                  # [B, nbest] int32: order[b, r] = the first-pass rank of the hypothesis now at rank r


def _rescore_launch(ids, lens, scores, word_lm, lm_weight, word_bonus, sep, use_eos, ws=None) -> Rescored:
    """rescore_nbest's checks and its one launch; ws: a workspace of the caller's (tests), at least
    v100_nbest_rescore_workspace_bytes(B, nbest, T) bytes."""
    who = "rescore_nbest"
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in (ids, lens, scores)):
        raise RuntimeError(f"{who}: GPU tensors only")
    if ids.dim() != 3 or lens.shape != ids.shape[:2] or scores.shape != ids.shape[:2]:
        raise RuntimeError(f"{who}: ids [B, nbest, T], lens [B, nbest] and scores [B, nbest] as ctc_beam_search returns them, got "
                           f"{list(ids.shape)}, {list(lens.shape)} and {list(scores.shape)}")
    tables = (getattr(word_lm, "pool", None), getattr(word_lm, "word_table", None), getattr(word_lm, "ngram_table", None))
    if any(t is None for t in tables) or getattr(word_lm, "meta", None) is None:
        raise RuntimeError(f"{who}: the word model is not compiled (WordNGramLM.compile().to(device) first)")
    dev = ids.device
    if any(t.device != dev for t in tables):
        raise RuntimeError(f"{who}: the word model is on {tables[0].device}, the hypotheses on {dev} (word_lm.to(device))")
    B, nbest, width = ids.shape
    alpha, beta = float(lm_weight), float(word_bonus)
    if not (math.isfinite(alpha) and math.isfinite(beta)):
        raise RuntimeError(f"{who}: lm_weight = {alpha} and word_bonus = {beta} must be finite")
    ids = ids.to(torch.int64).contiguous()
    lens, scores = lens.to(torch.int32).contiguous(), scores.float().contiguous()
    if width == 0:                                       # no column: every hypothesis is empty
        ids, lens = ids.new_zeros((B, nbest, 1)), torch.zeros_like(lens)
    T = ids.shape[2]
    nbytes = N.helper("v100_nbest_rescore_workspace_bytes", B, nbest, T)
    order = int(word_lm.order)
    pool, wtab, ng = (t.contiguous() for t in tables)
    meta = word_lm.meta
    if (nbytes <= 0 or not 1 <= order <= 8 or pool.dtype != torch.int64 or wtab.dtype != torch.int32 or ng.dtype != torch.int32
            or meta.dtype != "int64" or meta.size != 2 * order or not meta.flags["C_CONTIGUOUS"]
            or max(pool.numel(), wtab.numel(), ng.numel()) >= 1 << 31 or not 0 <= int(word_lm.pool_len) <= pool.numel()):
        raise RuntimeError(f"{who}: unsupported shape or model (B = {B} >= 1, 1 <= nbest = {nbest} <= 64, hypotheses of T = {width} <= 4096 "
                           f"labels, 1 <= order = {order} <= 8 and tables of fewer than 2^31 elements are the limits)")
    if ws is None:
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    elif not ws.is_cuda or ws.dtype != torch.uint8 or ws.numel() < nbytes:
        raise RuntimeError(f"{who}: the workspace must be a uint8 GPU tensor of at least {nbytes} bytes")
    i32 = lambda: torch.empty((B, nbest), dtype=torch.int32, device=dev)      # noqa: E731
    f32 = lambda: torch.empty((B, nbest), dtype=torch.float32, device=dev)    # noqa: E731
    out_ids, out_lens, out_scores, out_first, out_lm, n_words, n_oov, rank = torch.empty_like(ids), i32(), f32(), f32(), f32(), i32(), i32(), i32()
    try:
        N.call("v100_nbest_rescore", ids, lens, scores, pool, int(word_lm.pool_len), wtab, wtab.numel(), ng, ng.numel(), meta.ctypes.data,
               order, int(bool(word_lm.has_bos)), int(bool(word_lm.has_eos)), ws, out_ids, out_lens, out_scores, out_first, out_lm, n_words,
               n_oov, rank, B, nbest, T, int(sep), alpha, beta, int(bool(use_eos)))
    except RuntimeError as e:
        if "status 1" not in str(e):
            raise
        raise RuntimeError(f"{who}: the word model's tables do not fit their sizes (meta {meta.tolist()}, word table of {wtab.numel()} "
                           f"and n-gram table of {ng.numel()} int32: capacities must be powers of two inside the tables)") from None
    if width == 0:
        out_ids = out_ids[:, :, :0]
    return Rescored(out_ids, out_lens, out_scores, out_first, out_lm, n_words, n_oov, rank)


def rescore_nbest(ids: torch.Tensor, lens: torch.Tensor, scores: torch.Tensor, word_lm, lm_weight: float = 0.5, word_bonus: float = 0.0,
                  sep: int = 1, use_eos: bool = True) -> Rescored:
    """The second pass over an n-best list in one launch (K34, csrc/rescore.hip): ids [B, nbest, T] int64, lens [B, nbest] int32 and
    scores [B, nbest] fp32 exactly as ctc_beam_search returns them (its first three outputs; with a fused character LM `scores` is the
    fused score -- pass ctc_scores instead to rank on the acoustic score alone: the caller decides what the first pass is), word_lm
    a compiled lm.WordNGramLM on the same device -> Rescored, best first.  No read-back inside the call.

    A word is a maximal run of ids != sep inside a hypothesis' length (edit_distance's rule); a word outside the model's vocabulary
    is <unk>.  Every hypothesis gets word_lm_scores = sum over its words of log p(word | the order - 1 words before it, <s> in front
    where the model lists it), plus log p(</s> | ...) with use_eos where the model lists </s>, summed in fp64 over the tables' fp32
    values, and is ranked by scores = first + lm_weight * word_lm_scores + word_bonus * n_words (fp64, stored as fp32): a greater one
    is ahead, equal ones keep their first-pass order.  A hypothesis that the first pass does not have (score -inf, length 0) stays
    behind all the others with score -inf, word_lm_scores 0 and no words.  Dtypes and padding are ctc_beam_search's: ids are the given
    rows, moved whole.  lens are clamped to [0, T] on the device and nothing beyond a hypothesis' length is read; ids may be any
    int64 (they are hashed and compared, never used as an index).  Two calls give equal bits.
    Limits: 1 <= nbest <= 64, hypotheses of 0 to 4096 labels (T <= 4096, so up to 2048 words), model order <= 8, tables of fewer
    than 2^31 elements."""
    return _rescore_launch(ids, lens, scores, word_lm, lm_weight, word_bonus, sep, use_eos)


class MBR(NamedTuple):
    """What mbr_nbest returns: the list by rank (least expected error first), the pairwise distances in the given order."""
    ids: torch.Tensor                                    # [B, nbest, T] int64: the hypotheses' rows as given, re-ordered
    lens: torch.Tensor                                   # [B, nbest] int32
    scores: torch.Tensor                                 # [B, nbest] fp32: the scores as given, re-ordered
    risk: torch.Tensor                                   # [B, nbest] fp32: the expected number of token errors; +inf: no hypothesis
    posterior: torch.Tensor                              # [B, nbest] fp32: the list's posterior; 0: no hypothesis
    n_tokens: torch.Tensor                               # [B, nbest] int32: words (or ids with sep=None)
    order: torch.Tensor                                  # [B, nbest] int32: order[b, r] = the given index of the hypothesis now at rank r
    dist: torch.Tensor                                   # [B, nbest, nbest] int32, GIVEN order: pairwise distances; -1: one is absent
    expected_len: torch.Tensor                           # [B] fp32: the posterior mean of the token count
    ref_dist: Optional[torch.Tensor]                     # [B, nbest] int32, GIVEN order: distances to the reference; None without one
    ref_n: Optional[torch.Tensor]                        # [B] int32: the reference's tokens; None without one


def _mbr_launch(ids, lens, scores, sep, scale, ref, ref_len, ws=None) -> MBR:
    """mbr_nbest's checks and its three launches; ws: a workspace of the caller's (tests), at least
    v100_nbest_mbr_workspace_bytes(B, nbest, T, Tr) bytes."""
    who = "mbr_nbest"
    given = (ids, lens, scores) + (() if ref is None and ref_len is None else (ref, ref_len))
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in given):
        raise RuntimeError(f"{who}: GPU tensors only")
    if ids.dim() != 3 or lens.shape != ids.shape[:2] or scores.shape != ids.shape[:2]:
        raise RuntimeError(f"{who}: ids [B, nbest, T], lens [B, nbest] and scores [B, nbest] as ctc_beam_search returns them, got "
                           f"{list(ids.shape)}, {list(lens.shape)} and {list(scores.shape)}")
    dev = ids.device
    B, nbest, width = ids.shape
    has_ref = ref is not None
    if has_ref and (ref.dim() != 2 or ref.shape[0] != B or ref_len.numel() != B):
        raise RuntimeError(f"{who}: ref [B, Tr] and ref_len [B] with B = {B}, got {list(ref.shape)} and {list(ref_len.shape)}")
    scale = float(scale)
    if not (math.isfinite(scale) and scale >= 0.0):
        raise RuntimeError(f"{who}: scale = {scale} must be finite and not negative")
    ids = ids.to(torch.int64).contiguous()
    lens, scores = lens.to(torch.int32).contiguous(), scores.float().contiguous()
    if width == 0:                                       # no column: every hypothesis is empty
        ids, lens = ids.new_zeros((B, nbest, 1)), torch.zeros_like(lens)
    T, Tr, rl = ids.shape[2], 0, None
    if has_ref:
        ref = ref.to(device=dev, dtype=torch.int64).contiguous()
        rl = ref_len.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if ref.shape[1] == 0:
            ref, rl = ref.new_zeros((B, 1)), torch.zeros_like(rl)
        Tr = ref.shape[1]
    nbytes = N.helper("v100_nbest_mbr_workspace_bytes", B, nbest, T, Tr) if B >= 1 else -1
    if nbytes <= 0:
        raise RuntimeError(f"{who}: unsupported shape (B = {B} >= 1, 1 <= nbest = {nbest} <= 64, hypotheses of T = {width} <= 4096 labels "
                           f"and a reference of Tr = {Tr} <= 4096 labels are the limits)")
    if ws is None:
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    elif not ws.is_cuda or ws.dtype != torch.uint8 or ws.numel() < nbytes:
        raise RuntimeError(f"{who}: the workspace must be a uint8 GPU tensor of at least {nbytes} bytes")
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)          # noqa: E731
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)        # noqa: E731
    out_ids, out_lens, out_scores, risk, post, ntok, order = torch.empty_like(ids), i32(B, nbest), f32(B, nbest), f32(B, nbest), \
        f32(B, nbest), i32(B, nbest), i32(B, nbest)
    dist, elen = i32(B, nbest, nbest), f32(B)
    ref_dist, ref_n = (i32(B, nbest), i32(B)) if has_ref else (None, None)
    N.call("v100_nbest_mbr", ids, lens, scores, ref if has_ref else None, rl, ws, out_ids, out_lens, out_scores, risk, post, ntok, order,
           dist, ref_dist, ref_n, elen, B, nbest, T, Tr, 0 if sep is None else 1, 0 if sep is None else int(sep), scale)
    if width == 0:
        out_ids = out_ids[:, :, :0]
    return MBR(out_ids, out_lens, out_scores, risk, post, ntok, order, dist, elen, ref_dist, ref_n)


def mbr_nbest(ids: torch.Tensor, lens: torch.Tensor, scores: torch.Tensor, sep=1, scale: float = 1.0, ref: torch.Tensor = None,
              ref_len: torch.Tensor = None) -> MBR:
    """Minimum-Bayes-risk selection over an n-best list (K35, csrc/mbr.hip; three launches, no read-back): ids [B, nbest, T] int64,
    lens [B, nbest] int32 and scores [B, nbest] fp32 exactly as ctc_beam_search or rescore_nbest return them -> MBR, the hypothesis
    with the least expected number of token errors under the list's posterior first.

    A hypothesis is absent when its score is -inf or NaN; one of length 0 with a finite score is present and empty.  sep=<id>: a token
    is a word, a maximal run of ids != sep inside the hypothesis' length, and two words are equal iff they have the same length and
    the same ids; sep=None: a token is one id (edit_distance's convention at both levels).
      dist[b, i, j]    the Levenshtein distance (unit costs) between the token sequences of hypotheses i and j, in the GIVEN order:
                       symmetric, 0 on the diagonal, -1 where either is absent;
      posterior[b, i]  exp(scale (s_i - s_max)) / the sum over the present hypotheses, in fp64 from the fp32 scores; 0 for an absent one;
      risk[b, i]       sum_j posterior_j dist[i, j] (fp64, stored as fp32): the expected number of token errors of i; +inf for an absent one;
      expected_len[b]  sum_j posterior_j n_tokens_j, so risk / expected_len is the expected error rate: a quality estimate per utterance
                       that needs no reference;
      order            by the stored fp32 risk, smaller first; equal risks keep the given order; absent hypotheses follow in the given
                       order.  ids (rows moved whole), lens, scores, risk, posterior and n_tokens are in that order.
    ref [B, Tr] int64 with ref_len [B]: ref_dist[b, i] = the distance of hypothesis i (GIVEN order) to the reference, -1 for an absent
    one, and ref_n[b] = the reference's tokens -- the list's oracle error is ref_dist's minimum over the present ones.

    What the numbers are not: the posterior is over the LIST, not over all transcripts, so risk underestimates the true expected error
    when the list is short, and scale is not calibrated here (1.0 takes the scores as log probabilities).
    lens and ref_len are clamped to [0, width] on the device and nothing beyond a row's length is read; ids may be any int64 (hashed
    and compared, never an index).  Two calls give equal bits.  Limits: 1 <= nbest <= 64, T and Tr <= 4096, finite scale >= 0."""
    return _mbr_launch(ids, lens, scores, sep, scale, ref, ref_len)


class CTCSegments(NamedTuple):
    """What ctc_segment returns; the word fields are None with sep=None."""
    log_prob: torch.Tensor                               # [B] fp32: log p(labels | logits), summed over all alignments
    start: torch.Tensor                                  # [B, L] int32: the median first frame of each label
    end: torch.Tensor                                    # [B, L] int32: one past the median last frame
    duration: torch.Tensor                               # [B, L] fp32: the expected number of frames
    log_confidence: torch.Tensor                         # [B, L] fp32: occupancy-weighted mean log posterior of the label
    word_first: Optional[torch.Tensor]                   # [B, (L + 1) // 2] int32: index of the word's first label
    word_count: Optional[torch.Tensor]                   # ... its number of labels
    word_start: Optional[torch.Tensor]                   # ... start of its first label
    word_end: Optional[torch.Tensor]                     # ... end of its last label
    word_log_confidence: Optional[torch.Tensor]          # ... fp32: the same mean over all the word's labels
    n_words: Optional[torch.Tensor]                      # [B] int32


def ctc_segment(logits: torch.Tensor, lengths: torch.Tensor, labels: torch.Tensor, label_lengths: torch.Tensor, blank: int = 0,
                sep=1) -> CTCSegments:
    """Time boundaries, expected durations and confidences of every label and word of a GIVEN transcript, from the CTC
    forward-backward over all its alignments in one launch (K26, csrc/ctc_segment.hip): logits [B, T, V] fp32 (the model's output; the
    kernel normalises), lengths [B] or None, labels [B, L] int64 (any hypothesis: a reference text, a decode), label_lengths [B] or
    None -> CTCSegments of device tensors.  No read-back inside the call.

    This is the posterior of the ALIGNMENTS given the transcript -- when each label was spoken if the transcript is right, and how
    well the frames it claims support it -- not a posterior of the transcript being right.  With gamma_t(i) the posterior probability
    that frame t is spent in label i: duration = sum_t gamma_t(i), log_confidence = sum_t gamma_t(i) log_softmax(logits[t])[l_i] /
    duration (exp of it is the confidence), start / end = the medians of the label's first frame and of one past its last frame, so
    start < end <= the next label's start.  A word is a maximal run of labels != sep (edit_distance's rule); sep=None: no word level.
    Lengths are clamped to [0, T] / [0, L] on the device and nothing beyond them is read; outputs beyond them are 0.  A row whose
    labels cannot be aligned (too few frames, a label equal to blank or outside [0, V)) gets log_prob -inf, start = end = 0,
    duration 0 and log_confidence -inf.  Two calls give equal bits.  Limits: 1 <= T <= 4096, 2 <= V <= 128, L <= 2047; beyond them
    ctc_segment_long computes the same inside a corridor round a path."""
    given = [t for t in (logits, lengths, labels, label_lengths) if t is not None]
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in given) or logits is None or labels is None:
        raise RuntimeError("ctc_segment: GPU tensors only")
    if logits.dim() != 3 or labels.dim() != 2 or labels.shape[0] != logits.shape[0]:
        raise RuntimeError(f"ctc_segment: logits [B, T, V] and labels [B, L] with the same B, got {list(logits.shape)} and "
                           f"{list(labels.shape)}")
    dev = logits.device
    logits = logits.contiguous().float()
    B, T, V = logits.shape
    blank = int(blank)
    labels = labels.to(device=dev, dtype=torch.int64).contiguous()
    il = lengths.to(device=dev, dtype=torch.int32).contiguous() if lengths is not None else None
    ll = label_lengths.to(device=dev, dtype=torch.int32).contiguous() if label_lengths is not None else None
    if (il is not None and il.numel() != B) or (ll is not None and ll.numel() != B):
        raise RuntimeError(f"ctc_segment: lengths and label_lengths must have {B} elements")
    width = labels.shape[1]
    if width == 0:                                       # no column: every row is empty
        labels, ll = labels.new_zeros((B, 1)), torch.zeros((B,), dtype=torch.int32, device=dev)
    Lmax = labels.shape[1]
    nbytes = N.helper("v100_ctc_segment_workspace_bytes", B, T, Lmax) if B >= 1 else -1
    if nbytes <= 0 or not 2 <= V <= 128 or not 0 <= blank < V:
        raise RuntimeError(f"ctc_segment: unsupported shape or argument (B = {B} >= 1, 1 <= T = {T} <= 4096, 2 <= V = {V} <= 128, "
                           f"L = {width} <= 2047 and 0 <= blank = {blank} < V are the limits)")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)    # noqa: E731
    log_prob, start, end, duration, log_conf = f32(B), i32(B, Lmax), i32(B, Lmax), f32(B, Lmax), f32(B, Lmax)
    NW = (Lmax + 1) // 2
    word = (i32(B, NW), i32(B, NW), i32(B, NW), i32(B, NW), f32(B, NW), i32(B)) if sep is not None else (None,) * 6
    N.call("v100_ctc_segment", logits, il, labels, ll, ws, log_prob, start, end, duration, log_conf, *word, B, T, V, Lmax, blank,
           0 if sep is None else int(sep))
    if width == 0:
        start, end, duration, log_conf = (t[:, :0] for t in (start, end, duration, log_conf))
        word = tuple(t[:, :0] for t in word[:5]) + (word[5],) if sep is not None else word
    return CTCSegments(log_prob, start, end, duration, log_conf, *word)


class CTCLongSegments(NamedTuple):
    """What ctc_segment_long returns: CTCSegments' fields, log_prob in fp64, and ok; the word fields are None with sep=None."""
    log_prob: torch.Tensor                               # [B] fp64: log p(labels | logits) over the alignments inside the corridor
    ok: torch.Tensor                                     # [B] int32: 1 where that probability is not zero
    start: torch.Tensor                                  # [B, L] int32
    end: torch.Tensor                                    # [B, L] int32
    duration: torch.Tensor                               # [B, L] fp32
    log_confidence: torch.Tensor                         # [B, L] fp32
    word_first: Optional[torch.Tensor]                   # [B, (L + 1) // 2] int32
    word_count: Optional[torch.Tensor]
    word_start: Optional[torch.Tensor]
    word_end: Optional[torch.Tensor]
    word_log_confidence: Optional[torch.Tensor]
    n_words: Optional[torch.Tensor]                      # [B] int32


def ctc_corridor(path: torch.Tensor, lengths, label_lengths, band: int = 256) -> torch.Tensor:
    """The corridor that ctc_segment_long walks, from a CTC path: path [B, T] int32 (extended positions, as ctc_align_long returns
    them), lengths [B] or None, label_lengths [B] (or one int for every row) -> lo [B, ceil(T / 16)] int32, the first live state of
    every block of 16 frames.  With c_k = path[16 k], hi = (max(2 L + 1 - band, 0) + 1) & ~1:
    lo_k = clamp((c_k + 16 - band / 2) & ~1, 0, hi), then a running maximum over k; blocks beyond a row's length repeat its last value.
    A CTC path advances by at most 2 states a frame, so it stays inside [lo_k, lo_k + band) at any band >= 64.  Stock torch ops, no
    read-back."""
    if not isinstance(path, torch.Tensor) or path.dim() != 2 or path.shape[1] < 1:
        raise RuntimeError("ctc_corridor: path must be a tensor [B, T] with T >= 1")
    W = int(band)
    if W < 64 or W > 1024 or W % 64:
        raise RuntimeError(f"ctc_corridor: band = {W} must be a multiple of 64 in [64, 1024]")
    B, T = path.shape
    dev = path.device
    NB = (T + 15) // 16
    idx = (torch.arange(NB, device=dev) * 16)[None].expand(B, NB)
    if lengths is not None:
        last = (lengths.to(device=dev, dtype=torch.int64).reshape(B).clamp(0, T) - 1).clamp_min(0)
        idx = torch.minimum(idx, (last // 16 * 16)[:, None])
    ll = torch.as_tensor(label_lengths, device=dev).to(torch.int64).reshape(-1).expand(B)
    hi = torch.bitwise_and((2 * ll + 1 - W).clamp_min(0) + 1, -2)
    c = path.gather(1, idx).to(torch.int64)
    lo = torch.minimum(torch.bitwise_and(c + (16 - W // 2), -2).clamp_min(0), hi[:, None])
    return torch.cummax(lo, dim=1).values.to(torch.int32).contiguous()


def ctc_segment_long(logits: torch.Tensor, lengths: torch.Tensor, labels: torch.Tensor, label_lengths: torch.Tensor, path=None, lo=None,
                     band: int = 256, blank: int = 0, sep=1, align_band: int = 2048, path_ok=None) -> CTCLongSegments:
    """ctc_segment for chapter-length recordings (K33, csrc/ctc_segment_long.hip): the same time boundaries, expected durations and
    confidences of every label and word of a GIVEN transcript, from the CTC forward-backward over the alignments that stay inside a
    CORRIDOR of `band` states around a path.  logits [B, T, V] fp32 (the model's output; the kernel normalises), lengths [B] or None,
    labels [B, L] int64, label_lengths [B] or None -> CTCLongSegments of device tensors.  No read-back inside the call.

    The corridor: frames come in blocks of 16, lo[b, k] is the first live state of block k (of the 2 L + 1 states: label i is state
    2 i + 1), and a state is live where lo <= s < lo + band.  Alignments that leave the corridor count for nothing: every output is
    the posterior over those that stay inside, and log_prob is at most ctc_segment's.  Where the frames pin the path down (a trained
    model on its own transcript) nothing measurable is lost at band 64 already; on diffuse logits mass is cut -- widen band.
    lo=: a corridor of the caller's, [B, ceil(T / 16)] int32; the device clamps it to [0, hi], clears bit 0 and takes the running
    maximum before it trusts it.  path=: a CTC path [B, T] int32 (ctc_align_long's), from which ctc_corridor builds lo; with it
    path_ok=: [B], the aligner's ok -- a row where it is 0 has a path of zeros, and comes back with ok = 0 and the outputs of a row
    without an alignment, whatever the corridor of zeros would give.  Neither:
    ctc_align_long runs on the log_softmax of the same logits at band `align_band`; a row that the aligner lost comes back with ok = 0.
    lo = 0 everywhere with band >= 2 L + 1 is ctc_segment's quantity exactly.
    A row whose corridor holds no alignment (it misses the end, too few frames, a label equal to blank or outside [0, V)) gets ok = 0,
    log_prob -inf, start = end = 0, duration 0 and log_confidence -inf; its words are still delimited.  Lengths are clamped on the
    device, nothing beyond them is read, outputs beyond them are 0.  Two calls give equal bits.  Memory: 12 T band / 2 bytes a row
    (138 MB for 30 minutes at band 256).  Limits: 1 <= T <= 2^20, L <= 2^19, 2 <= V <= 128, band a multiple of 64 in [64, 1024]."""
    given = [t for t in (logits, lengths, labels, label_lengths, path, lo, path_ok) if t is not None]
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in given) or logits is None or labels is None:
        raise RuntimeError("ctc_segment_long: GPU tensors only")
    if logits.dim() != 3 or labels.dim() != 2 or labels.shape[0] != logits.shape[0]:
        raise RuntimeError(f"ctc_segment_long: logits [B, T, V] and labels [B, L] with the same B, got {list(logits.shape)} and "
                           f"{list(labels.shape)}")
    if path is not None and lo is not None:
        raise RuntimeError("ctc_segment_long: give a path or a corridor, not both")
    if path_ok is not None and (path is None or path_ok.numel() != logits.shape[0]):
        raise RuntimeError(f"ctc_segment_long: path_ok goes with path= and has {logits.shape[0]} elements")
    dev = logits.device
    logits = logits.contiguous().float()
    B, T, V = logits.shape
    blank, band = int(blank), int(band)
    labels = labels.to(device=dev, dtype=torch.int64).contiguous()
    il = lengths.to(device=dev, dtype=torch.int32).contiguous() if lengths is not None else None
    ll = label_lengths.to(device=dev, dtype=torch.int32).contiguous() if label_lengths is not None else None
    if (il is not None and il.numel() != B) or (ll is not None and ll.numel() != B):
        raise RuntimeError(f"ctc_segment_long: lengths and label_lengths must have {B} elements")
    width = labels.shape[1]
    if width == 0:                                       # no column: every row is empty
        labels, ll = labels.new_zeros((B, 1)), torch.zeros((B,), dtype=torch.int32, device=dev)
    Lmax = labels.shape[1]
    nbytes = N.helper("v100_ctc_segment_long_workspace_bytes", B, T, Lmax, band) if B >= 1 else 0
    if nbytes <= 0 or not 2 <= V <= 128 or not 0 <= blank < V:
        raise RuntimeError(f"ctc_segment_long: unsupported shape or argument (B = {B} >= 1, 1 <= T = {T} <= 2^20, 2 <= V = {V} <= 128, "
                           f"L = {width} <= 2^19, 0 <= blank = {blank} < V and band = {band}, a multiple of 64 in [64, 1024], are the "
                           "limits)")
    NB = (T + 15) // 16
    lost = path_ok.reshape(B) == 0 if path_ok is not None else None
    if lo is None:
        lens_l = ll.clamp(0, Lmax) if ll is not None else Lmax
        if path is None:
            al = ctc_align_long(torch.log_softmax(logits, dim=-1), labels, il, ll, band=align_band, blank=blank)
            path, lost = al.path, al.ok == 0
        if path.shape != (B, T):
            raise RuntimeError(f"ctc_segment_long: path must be [{B}, {T}], got {list(path.shape)}")
        lo = ctc_corridor(path.to(torch.int32), il, lens_l, band)
    if lo.shape != (B, NB):
        raise RuntimeError(f"ctc_segment_long: lo must be [{B}, {NB}] (one value per block of 16 frames), got {list(lo.shape)}")
    lo = lo.to(torch.int32).contiguous()
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)    # noqa: E731
    log_prob, ok = torch.empty((B,), dtype=torch.float64, device=dev), i32(B)
    start, end, duration, log_conf = i32(B, Lmax), i32(B, Lmax), f32(B, Lmax), f32(B, Lmax)
    NW = (Lmax + 1) // 2
    word = (i32(B, NW), i32(B, NW), i32(B, NW), i32(B, NW), f32(B, NW), i32(B)) if sep is not None else (None,) * 6
    N.call("v100_ctc_segment_long", logits, il, labels, ll, lo, ws, log_prob, ok, start, end, duration, log_conf, *word, B, T, V, Lmax,
           band, blank, 0 if sep is None else int(sep))
    if lost is not None:                                 # the aligner's lost rows: the infeasible outputs, whatever the corridor of zeros gave
        row = lost[:, None]
        inside = torch.arange(Lmax, device=dev)[None] < (ll[:, None] if ll is not None else Lmax)
        ninf = torch.full((), float("-inf"), dtype=torch.float32, device=dev)
        log_prob = torch.where(lost, ninf.double(), log_prob)
        ok = torch.where(lost, torch.zeros_like(ok), ok)
        start, end = torch.where(row, torch.zeros_like(start), start), torch.where(row, torch.zeros_like(end), end)
        duration = torch.where(row, torch.zeros_like(duration), duration)
        log_conf = torch.where(row & inside, ninf, log_conf)
        if sep is not None:
            wf, wc, wst, wen, wlc, nw = word
            inw = torch.arange(NW, device=dev)[None] < nw[:, None]
            word = (wf, wc, torch.where(row, torch.zeros_like(wst), wst), torch.where(row, torch.zeros_like(wen), wen),
                    torch.where(row & inw, ninf, wlc), nw)
    if width == 0:
        start, end, duration, log_conf = (t[:, :0] for t in (start, end, duration, log_conf))
        word = tuple(t[:, :0] for t in word[:5]) + (word[5],) if sep is not None else word
    return CTCLongSegments(log_prob, ok, start, end, duration, log_conf, *word)
