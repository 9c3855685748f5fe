"""Inference side of the hot path: the configs[2] TTS chain on the device, and the pure data-parallel scatter of
inference requests over the GPUs of a node (SURVEY.md 8e "Inference": replicas only, no collective on the data path).

Reference call sites this serves:
  * voice100/update_samples.py:30-90 -- text -> align model -> align() -> audio model predict -> vocoder glue, one batch
    of sample sentences (here: `TTSPipeline`, every step INCLUDING the pyworld synthesis on the GPU: it ends in a waveform);
  * voice100/models/asr.py:110-116 -- AudioToTextCTC.forward over independent utterances / 1-second chunks
    (here: `ASRPipeline`, log-mel -> encoder -> logits -> greedy CTC ids);
  * BASELINE.json configs[4]: "streaming 1-second chunks at 16 kHz, 8 x MI355X" -- chunks are independent, so rank r of
    `world` takes every world-th chunk (`shard_indices(..., "round_robin")`) or a contiguous slice of a request batch,
    runs its replica, and only the small results (token ids, WORLD features) are gathered on rank 0 (`scatter_run`).

Nothing here computes on the CPU: the pipelines call the HIP-backed modules; `scatter_run` is plumbing over
torch.distributed ("nccl" = RCCL on the GPU box, "gloo" in the CPU tests, where a stock-op stand-in model is used).
"""
import math
from typing import Callable, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

__all__ = ["shard_indices", "scatter_run", "TTSPipeline", "TTSPipelineV2", "ASRPipeline", "AlignPipeline", "align_records",
           "ErrorRate", "GraphedForward", "window_plan", "windowed_logits", "utterance_cuts", "LongAlignPipeline", "align_long_records",
           "cut_utterances", "batch_plan", "join_ids", "LongASRPipeline", "long_transcript_records"]


def shard_indices(n_items: int, rank: int, world: int, mode: str = "contiguous") -> torch.Tensor:
    """Indices (int64, ascending) of the items rank `rank` of `world` processes.
    "contiguous": one slice per rank, ceil(n / world) items each (a request batch);
    "round_robin": items rank, rank + world, ... (a stream of chunks: every rank stays equally loaded as chunks arrive)."""
    if not 0 <= rank < world:
        raise ValueError("rank must be in [0, world)")
    if mode == "contiguous":
        per = (n_items + world - 1) // world
        lo = min(n_items, rank * per)
        return torch.arange(lo, min(n_items, lo + per), dtype=torch.int64)
    if mode == "round_robin":
        return torch.arange(rank, max(n_items, rank), world, dtype=torch.int64)
    raise ValueError("mode must be 'contiguous' or 'round_robin'")


def _world(group=None) -> Tuple[int, int]:
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def scatter_run(fn: Callable[..., Sequence[torch.Tensor]], inputs: Sequence[torch.Tensor], mode: str = "contiguous",
                group=None, pad_value=0, out_specs=None) -> Optional[List[torch.Tensor]]:
    """Run `fn` data-parallel over dim 0 of `inputs` and gather its outputs on rank 0.

    Every rank holds (or can index) the full `inputs`; rank r calls fn(*[x[idx_r] for x in inputs]) on its shard -- no
    collective touches the data path -- and gets back a sequence of tensors whose dim 0 is the shard.  Outputs may be
    ragged in dim 1 across ranks (aligned-text / WORLD-frame counts differ): they are padded with `pad_value` to the
    global maximum before the gather.  Returns the outputs in the ORIGINAL item order on the group's rank 0 (whatever its
    global rank is) and None elsewhere.  With no process group (or a group of one) it is just fn(*inputs).
    `out_specs` = [(trailing shape, dtype), ...] per output when the caller knows them (fixed-size outputs: token-id
    matrices, per-chunk features): the shapes then need no agreement round, i.e. no object all-gather and no host
    synchronisation per call -- what a timed streaming loop wants."""
    rank, world = _world(group)
    n = inputs[0].shape[0]
    if any(x.shape[0] != n for x in inputs):
        raise ValueError("scatter_run: inputs must share dim 0")
    if world == 1:
        return [o for o in fn(*inputs)]
    idx = shard_indices(n, rank, world, mode)
    per = (n + world - 1) // world                       # every rank pads its shard to `per` items so gathers are regular
    if idx.numel():
        outs = [o for o in fn(*[x[idx.to(x.device)] for x in inputs])]
    else:
        outs = None
    # Shapes and dtypes are agreed through rank 0's view of a rank that has work; ranks without items (n < world) build
    # zero-sized placeholders after learning the trailing shapes.
    if out_specs is not None:
        specs = [(tuple(sh), str(dt)) for sh, dt in out_specs]
        if outs is not None and any(tuple(o.shape[1:]) != sp[0] or str(o.dtype) != sp[1] for o, sp in zip(outs, specs)):
            raise ValueError("scatter_run: fn's outputs do not match out_specs")
        meta = [specs] * world
    else:
        meta = [None] * world
        dist.all_gather_object(meta, None if outs is None else [(tuple(o.shape[1:]), str(o.dtype)) for o in outs], group=group)
    ref = next((m for m in meta if m is not None), None)
    if ref is None:
        return [] if rank == 0 else None
    # dist.gather's dst is a GLOBAL rank: the group's rank 0 may be any process of the job
    dst = dist.get_global_rank(group, 0) if group is not None else 0
    dev = outs[0].device if outs is not None else inputs[0].device
    result = []
    for k, (_, dtname) in enumerate(ref):
        dt = getattr(torch, dtname.replace("torch.", ""))
        trailing = [m[k][0] for m in meta if m is not None]
        nd = len(trailing[0])
        full = tuple(max(t[d] for t in trailing) for d in range(nd))           # pad every ragged trailing dim to its maximum
        buf = torch.full((per,) + full, pad_value, dtype=dt, device=dev)
        if outs is not None:
            o = outs[k]
            buf[(slice(0, o.shape[0]),) + tuple(slice(0, s) for s in o.shape[1:])] = o
        gathered = [torch.empty_like(buf) for _ in range(world)] if rank == 0 else None
        dist.gather(buf, gathered, dst=dst, group=group)
        if rank == 0:
            merged = torch.full((n,) + full, pad_value, dtype=dt, device=dev)
            for r in range(world):
                ir = shard_indices(n, r, world, mode)
                if ir.numel():
                    merged[ir.to(dev)] = gathered[r][:ir.numel()]
            result.append(merged)
    return result if rank == 0 else None


@torch.no_grad()
def _tts_score(self, text: torch.Tensor, text_len: torch.Tensor, ref_f0: torch.Tensor, ref_feat: torch.Tensor, ref_frames: torch.Tensor,
               meter=None):
    """Objective scores of the pipeline's output against a recording's WORLD features (metrics.dtw_score, K27): the chain of
    __call__ with the synthesis off, then the DTW of its f0 / features / frames with ref_f0 [B, Tr] Hz, ref_feat [B, Tr, C] and
    ref_frames [B].  The distance is taken on mel-cepstra without c0: the audio model's own output where it predicts mel-cepstra,
    its log-spectrum through sp2mc otherwise (SynthesisScore.to_mcep; the same for ref_feat).  Returns {"score": the per-utterance
    metrics.DTWScore, "mcd" [B] float64 dB (nan for an empty pair), "frames" [B]}; no read-back.  meter: a metrics.SynthesisScore
    that also takes the batch's sums."""
    from .metrics import SynthesisScore, mcd_db
    out, feat = self._run(text, text_len, False)
    dev = feat.device
    m = meter if meter is not None else SynthesisScore(self.vocoder)
    sc = m.update(out["f0"], feat, out["frames"], ref_f0.to(dev), ref_feat.to(dev), ref_frames.to(dev), per_row=True)
    return {"score": sc, "mcd": mcd_db(sc.cost, sc.path_len), "frames": out["frames"]}


def _tts_evaluate(self, batches, meter=None):
    """Scores over an iterable of (text, text_len, ref_f0, ref_feat, ref_frames): score() per batch into one meter, and ONE
    device-to-host synchronisation at the end.  Returns SynthesisScore.compute()."""
    from .metrics import SynthesisScore
    meter = meter if meter is not None else SynthesisScore(self.vocoder)
    for text, text_len, ref_f0, ref_feat, ref_frames in batches:
        self.score(text, text_len, ref_f0, ref_feat, ref_frames, meter)
    return meter.compute()


def _tts_save(self, out, paths, bits_per_sample: int = 16, **enc):
    """Write the synthesis of __call__ to files: out["wave"][b, :out["wave_len"][b]] at the vocoder's sample rate to paths[b] (.wav or
    .flac, `audio_io.save_batch`: one FLAC encoding pass on the device, one copy for the WAV files).  ValueError when `out` holds no
    "wave" (a pipeline built with synthesize=False or without a vocoder)."""
    from .audio_io import save_batch
    if "wave" not in out or "wave_len" not in out:
        raise ValueError(f"{type(self).__name__}.save: the result holds no \"wave\" (synthesize=False, or no vocoder): nothing to write")
    save_batch(paths, out["wave"], out["wave_len"], int(self.vocoder.sample_rate), bits_per_sample, **enc)


class TTSPipeline:
    """BASELINE configs[2] end to end on the device (update_samples.py:46-84, the pyworld synthesis included):

        text [B, L] int64, text_len [B]
          -> TextToAlignTextModel.forward                 [B, L, 2]  log(gap + 1), log(len + 1)        (tts.py:79-87)
          -> align = max(exp(pred) - 1, 0)                (_align_v2.py:39-46; v1 has no predict(): it trains on log(align + 1),
                                                           tts.py:126.  Negative values are clamped: the reference's Python loop
                                                           would index from the END of the tensor for a negative start)
          -> align() per utterance, on the device         aligntext [B, La] int64, lens                (tts.py:89-110, bit-exact)
          -> AlignTextToAudioModel.predict                f0 [B, 2La-1], logspc|mcep, codeap           (tts.py:192-201)
          -> (use_mcep) logspc = mcep @ mc2sp             one fp32 MFMA GEMM over all B x T frames      (vocoder.py:95)
          -> spc = max(exp(logspc) - 1e-15, 0)                                                         (vocoder.py:99)
          -> ap = decode_aperiodicity(codeap); waveform = synthesize(f0, spc, ap)                      (vocoder.py:100-101; round 4,
                                                           csrc/world.hip -- parity unpinned, see voice100_amd/vocoder.py)

    configs[2] therefore ends in a waveform [B, samples] on the device ("wave", zero beyond each utterance's "wave_len").
    An audio model whose predict returns a fourth value (AlignTextToAudioMultiTaskModel: the phone logits [B, Vt, La], tts.py:308-317)
    gets it back as "phone_logits"; every other entry is what the three-value models give."""

    def __init__(self, align_model, audio_model, vocoder=None, head: int = 5, tail: int = 5, synthesize: bool = True,
                 f0_ceil: float = 1000.0):
        self.align_model, self.audio_model, self.vocoder = align_model, audio_model, vocoder
        self.head, self.tail = head, tail
        self.synthesize, self.f0_ceil = synthesize, f0_ceil

    @torch.no_grad()
    def __call__(self, text: torch.Tensor, text_len: torch.Tensor):
        return self._run(text, text_len, self.synthesize)[0]

    score, evaluate, save = _tts_score, _tts_evaluate, _tts_save

    def _run(self, text: torch.Tensor, text_len: torch.Tensor, synthesize: bool):
        """The chain of __call__: its result, and the audio model's own features (mel-cepstra with a use_mcep vocoder)."""
        from .decode import align_expand
        pred = self.align_model(text)                                        # [B, L, 2]
        align = torch.clamp_min(torch.exp(pred) - 1.0, 0.0)
        aligntext, at_len = align_expand(text, align, text_len, self.head, self.tail)
        # (align_expand sizes the batch exactly as wide as its longest utterance -- pad_sequence semantics, update_samples.py:66 --
        # so that one ends at the convolutions' zero padding, not at extra blank tokens)
        # 2 * La - 1 frames; AlignTextToAudioMultiTaskModel.predict adds the phone logits [B, Vt, La] as a fourth value (tts.py:308-317)
        f0, feat, codeap, *extra = self.audio_model.predict(aligntext)
        if len(extra) > 1:
            raise RuntimeError(f"TTSPipeline: audio_model.predict returned {3 + len(extra)} values; three or four expected")
        v = self.vocoder
        if v is not None and v.use_mcep:
            B, T, C = feat.shape
            logspc = v.mcep_to_logspc(feat.reshape(B * T, C)).reshape(B, T, -1)
        else:
            logspc = feat
        spc = v.logspc_to_spc(logspc) if v is not None else None
        # valid WORLD frames per utterance: 2 * len - 1 (update_samples.py:81 slices 2 * len, which yields the same)
        frames = torch.clamp_min(2 * at_len - 1, 0)
        out = {"align": align, "aligntext": aligntext, "aligntext_len": at_len, "f0": f0, "logspc": logspc, "spc": spc,
               "codeap": codeap, "frames": frames}
        if extra:
            out["phone_logits"] = extra[0]
        if v is not None and synthesize and v.n_fft == 512 and f0.shape[1] >= 2:
            wave, npulses = v.synthesize(f0, spc, frames=frames, f0_ceil=self.f0_ceil, codeap=codeap)
            out["wave"], out["n_pulses"] = wave, npulses
            out["wave_len"] = (frames.to(torch.float64) * v.frame_period * v.sample_rate / 1000).to(torch.int64)
        return out, feat


class TTSPipelineV2:
    """The v2 sample chain (update_samples.py:50-80) on the device:

        text [B, L] int64, text_len [B]
          -> TextToAlignText.predict                       align [B, max(text_len), 2] = exp(pred) - 1, unclamped  (_align_v2.py:39-46)
          -> align() batched, on the device                aligntext [B, max n] int64 zero padded (pad_sequence width), n [B]
                                                           (_align_v2.py:48-73, v100_align_expand_v2)
          -> AlignTextToAudio.predict                      f0 [B, 2 max(n) - 1], logspc|mcep, codeap, gated   (_tts_v2.py:80-94)
          -> (use_mcep) logspc = mcep @ mc2sp              one fp32 MFMA GEMM over all B x T frames           (vocoder.py:95)
          -> optionally synthesize, frames = min(2 n, 2 max(n) - 1) per utterance   (update_samples.py:80-84 slices [:2 n])

    The existing TTSPipeline (the v1 models) is unchanged."""

    def __init__(self, align_model, audio_model, vocoder=None, head: int = 5, tail: int = 5, synthesize: bool = True,
                 f0_ceil: float = 1000.0):
        self.align_model, self.audio_model, self.vocoder = align_model, audio_model, vocoder
        self.head, self.tail = head, tail
        self.synthesize, self.f0_ceil = synthesize, f0_ceil

    @torch.no_grad()
    def __call__(self, text: torch.Tensor, text_len: torch.Tensor):
        return self._run(text, text_len, self.synthesize)[0]

    score, evaluate, save = _tts_score, _tts_evaluate, _tts_save

    def _run(self, text: torch.Tensor, text_len: torch.Tensor, synthesize: bool):
        """The chain of __call__: its result, and the audio model's own features (mel-cepstra with a use_mcep vocoder)."""
        from .decode import align_expand_v2
        align, align_len = self.align_model.predict(text, text_len)         # [B, max(text_len), 2]
        L = align.shape[1]
        aligntext, at_len = align_expand_v2(text[:, :L], align, align_len, self.head, self.tail)
        f0, feat, codeap = self.audio_model.predict(aligntext, at_len)       # 2 * max(n) - 1 frames
        v = self.vocoder
        if v is not None and v.use_mcep:
            B, T, C = feat.shape
            logspc = v.mcep_to_logspc(feat.reshape(B * T, C)).reshape(B, T, -1)
        else:
            logspc = feat
        spc = v.logspc_to_spc(logspc) if v is not None else None
        frames = torch.clamp_max(2 * at_len, f0.shape[1])
        out = {"align": align, "aligntext": aligntext, "aligntext_len": at_len, "f0": f0, "logspc": logspc, "spc": spc,
               "codeap": codeap, "frames": frames}
        if v is not None and synthesize and v.n_fft == 512 and f0.shape[1] >= 2:
            wave, npulses = v.synthesize(f0, spc, frames=frames, f0_ceil=self.f0_ceil, codeap=codeap)
            out["wave"], out["n_pulses"] = wave, npulses
            out["wave_len"] = (frames.to(torch.float64) * v.frame_period * v.sample_rate / 1000).to(torch.int64)
        return out, feat


class ASRPipeline:
    """BASELINE configs[4] per replica: waveform chunks [B, N] fp32 (16 kHz) -> log-mel [B, T, 64] -> AudioToTextCTC logits
    -> greedy CTC ids [B, T'] int64 (zero padded) + lengths (data_modules.py:276-291, asr.py:110-116, text.py:99-104).
    beam_size=W decodes with the CTC prefix beam search instead (K24; no counterpart in the reference): the call returns its best
    hypothesis in the same form, so transcribe, score and evaluate work unchanged, and nbest() returns the `nbest` best with scores.
    lm=<a compiled lm.NGramLM on the model's device> fuses it into that search (K25): hypotheses are ranked by
    log p_ctc + lm_weight * log p_lm + length_bonus * length, and nbest() returns (ids, lens, scores, ctc_scores, lm_scores).
    word_lm=<a compiled lm.WordNGramLM on the model's device> adds the second pass (K34, decode.rescore_nbest): the search returns its
    rescore_size best (default: beam_size), they are re-ranked by score + word_lm_weight * log p_word_lm + word_bonus * words (score:
    the search's own, the fused one with lm=), the call and everything built on it take the top hypothesis after that, and nbest()
    returns decode.Rescored, cut to `nbest` ranks.  It needs a beam_size; without it every path is what it was.
    mbr="word" or "id" adds minimum-Bayes-risk selection (K35, decode.mbr_nbest) as the last stage: the search returns its mbr_size best
    (default: rescore_size with a word model, else beam_size; with a word model the second pass re-ranks that same list), and the call
    and everything built on it take the hypothesis with the least expected number of word (sep) or id errors under the posterior
    exp(mbr_scale * score) of the last stage's scores, which is not always the one with the best score.  nbest() returns decode.MBR,
    its rank-ordered fields cut to `nbest` ranks (dist, in the given order, and expected_len stay whole).  It needs a beam_size;
    with mbr=None every path executes exactly the calls it executes without the argument.

    With `lengths` the rows are utterances of their own lengths: samples per row when the pipeline has a `mel` (the features
    and their frame counts then come from one ragged launch, mel.transform(wav, lengths)), frames per row when it has none
    (wav_or_mel is the padded feature batch); the decode stops at model.output_length(frames) of each row."""

    def __init__(self, model, mel=None, beam_size=None, nbest=1, lm=None, lm_weight=0.5, length_bonus=0.0, frame_seconds=None,
                 word_lm=None, word_lm_weight=0.5, word_bonus=0.0, rescore_size=None, sep=1, mbr=None, mbr_scale=1.0, mbr_size=None):
        if (lm is not None or word_lm is not None) and beam_size is None:
            raise RuntimeError("ASRPipeline: a language model needs a beam_size (the greedy decode has nothing to rank)")
        if mbr is not None:
            if mbr not in ("word", "id"):
                raise RuntimeError(f"ASRPipeline: mbr = {mbr!r} must be None, \"word\" or \"id\"")
            if beam_size is None:
                raise RuntimeError("ASRPipeline: mbr needs a beam_size (the greedy decode has one hypothesis)")
            if not (math.isfinite(float(mbr_scale)) and float(mbr_scale) >= 0.0):
                raise RuntimeError(f"ASRPipeline: mbr_scale = {mbr_scale} must be finite and not negative")
        if word_lm is not None:
            rescore_size = int(beam_size if rescore_size is None else rescore_size)
            if not 1 <= rescore_size <= beam_size or rescore_size < nbest:
                raise RuntimeError(f"ASRPipeline: nbest = {nbest} <= rescore_size = {rescore_size} <= beam_size = {beam_size} is required")
        self.word_lm, self.word_lm_weight, self.word_bonus, self.rescore_size, self.sep = word_lm, word_lm_weight, word_bonus, rescore_size, sep
        if mbr is not None:
            mbr_size = int((rescore_size if word_lm is not None else beam_size) if mbr_size is None else mbr_size)
            if not nbest <= mbr_size <= beam_size or mbr_size < 1:
                raise RuntimeError(f"ASRPipeline: nbest = {nbest} <= mbr_size = {mbr_size} <= beam_size = {beam_size} is required")
        self.mbr, self.mbr_scale, self.mbr_size = mbr, float(mbr_scale), mbr_size
        self.model, self.mel = model, mel
        self.frame_seconds = frame_seconds                     # seconds per output frame (segments, transcribe_timed); None: from the mel
        self.beam_size, self.nbest_size = beam_size, nbest     # beam_size=None: the greedy decode
        self.lm, self.lm_weight, self.length_bonus = lm, lm_weight, length_bonus

    def _beam(self, logits, out_len, nbest):
        from .decode import ctc_beam_search
        if self.lm is None:
            return ctc_beam_search(logits, out_len, self.beam_size, nbest)
        return ctc_beam_search(logits, out_len, self.beam_size, nbest, lm=self.lm, lm_weight=self.lm_weight,
                               length_bonus=self.length_bonus)

    def _rescore(self, hyps):
        """decode.rescore_nbest of a beam search's tuple with the pipeline's word model."""
        from .decode import rescore_nbest
        return rescore_nbest(hyps[0], hyps[1], hyps[2], self.word_lm, self.word_lm_weight, self.word_bonus, self.sep)

    def _mbr(self, hyps):
        """decode.mbr_nbest of the first three tensors of a beam search's or a second pass' tuple, at the pipeline's level and scale."""
        from .decode import mbr_nbest
        return mbr_nbest(hyps[0], hyps[1], hyps[2], sep=self.sep if self.mbr == "word" else None, scale=self.mbr_scale)

    def _mbr_list(self, logits, out_len):
        """beam -> (word rescoring, if configured, over the same list) -> mbr_nbest on the scores of the last stage."""
        hyps = self._beam(logits, out_len, self.mbr_size)
        return self._mbr(hyps if self.word_lm is None else self._rescore(hyps))

    def _top(self, logits, out_len):
        """(ids [B, T'], lens [B], score [B]) of the best hypothesis: the beam search's, with a word model the second pass', with mbr
        the one of least expected error."""
        if self.mbr is not None:
            ids, n, score = self._mbr_list(logits, out_len)[:3]
        elif self.word_lm is None:
            ids, n, score = self._beam(logits, out_len, 1)[:3]
        else:
            ids, n, score = self._rescore(self._beam(logits, out_len, self.rescore_size))[:3]
        return ids[:, 0], n[:, 0], score[:, 0]

    def _logits(self, wav_or_mel: torch.Tensor, lengths=None):
        """The model's logits and, with `lengths`, the output frames of each row (else None)."""
        if lengths is None:
            feats = self.mel(wav_or_mel) if self.mel is not None else wav_or_mel
            return self.model(feats), None
        if self.mel is not None:
            feats, audio_len = self.mel.transform(wav_or_mel, lengths)
        else:
            feats, audio_len = wav_or_mel, torch.as_tensor(lengths).to(wav_or_mel.device)
        return self.model(feats), self.model.output_length(audio_len)

    @torch.no_grad()
    def __call__(self, wav_or_mel: torch.Tensor, lengths=None):
        """(ids [B, T'] int64 zero padded, lens [B] int32): the greedy decode, or with a beam_size the best hypothesis of the prefix
        beam search (decode.ctc_beam_search, K24)."""
        logits, out_len = self._logits(wav_or_mel, lengths)
        return self._best(logits, out_len)

    def _best(self, logits, out_len):
        """The decode of __call__ on logits that are already there."""
        from .decode import ctc_greedy_decode
        if self.beam_size is None:
            return ctc_greedy_decode(logits) if out_len is None else ctc_greedy_decode(logits, out_len)
        return self._top(logits, out_len)[:2]

    @torch.no_grad()
    def nbest(self, wav_or_mel: torch.Tensor, lengths=None):
        """The nbest hypotheses of the beam search, best first: (ids [B, nbest, T'] int64 zero padded, lens [B, nbest] int32,
        scores [B, nbest] fp32 = total log probability; -inf with length 0 where there are fewer hypotheses), and with a language model
        also ctc_scores and lm_scores [B, nbest] fp32 (scores is then the fused score).  With a word model: decode.Rescored, the
        `nbest` best of the rescore_size hypotheses after the second pass.  With mbr: decode.MBR, ids, lens, scores, risk, posterior,
        n_tokens and order cut to `nbest` ranks; dist (given order, [B, mbr_size, mbr_size]) and expected_len whole.  Needs a beam_size."""
        if self.beam_size is None:
            raise RuntimeError("ASRPipeline.nbest: the pipeline was built without a beam_size (the greedy decode has one hypothesis)")
        logits, out_len = self._logits(wav_or_mel, lengths)
        if self.mbr is not None:
            m = self._mbr_list(logits, out_len)
            return type(m)(*(t[:, :self.nbest_size] for t in m[:7]), *m[7:])
        if self.word_lm is None:
            return self._beam(logits, out_len, self.nbest_size)
        from .decode import Rescored
        return Rescored(*(t[:, :self.nbest_size] for t in self._rescore(self._beam(logits, out_len, self.rescore_size))))

    def transcribe(self, paths, decode: Callable[[torch.Tensor], str]) -> List[str]:
        """WAV or FLAC files -> their transcripts: audio_io.load_batch, the ragged pipeline, then `decode` (the caller's tokenizer.decode,
        ids tensor -> str, as in align_records) on each row's ids; one device-to-host copy per tensor.  Needs a `mel`."""
        from .audio_io import load_batch
        if self.mel is None:
            raise RuntimeError("ASRPipeline.transcribe: the pipeline has no mel transform to turn waveforms into features")
        wave, wave_len = load_batch(paths, self.mel.sample_rate, self.mel.dft_basis.device)
        ids, n = self(wave, wave_len)
        ids, n = ids.cpu(), n.cpu()
        return [decode(ids[i, :int(n[i])]) for i in range(ids.shape[0])]

    def _frame_seconds(self, who: str) -> float:
        """Seconds per output frame: the constructor's frame_seconds, else the mel's hop times the model's frame reduction."""
        if self.frame_seconds is not None:
            return float(self.frame_seconds)
        if self.mel is None:
            raise RuntimeError(f"ASRPipeline.{who}: the pipeline has no mel transform to take the frame period from "
                               "(pass frame_seconds= to the constructor)")
        frames = int(self.model.output_length(torch.tensor([4096])))
        return self.mel.hop_length / self.mel.sample_rate * 4096 / frames

    @torch.no_grad()
    def segments(self, wav_or_mel: torch.Tensor, lengths=None, sep=1):
        """One forward, the decode of __call__ (greedy, beam, or beam with the LM, as configured), then decode.ctc_segment (K26) of that
        hypothesis on the same logits.  Returns a dict of device tensors: "ids" [B, T'] int64 and "ids_len" [B] as __call__ returns
        them, the fields of decode.CTCSegments ("log_prob" [B]; "start", "end", "duration", "log_confidence" [B, L], L = the longest
        hypothesis; "word_first", "word_count", "word_start", "word_end", "word_log_confidence" [B, (L + 1) // 2] and "n_words" [B],
        None with sep=None) in output frames, and "frame_seconds" (a float: multiply a frame index by it).  One read-back, of
        ids_len.max(), sizes L.  The numbers are posteriors of the alignment GIVEN the hypothesis, not of the hypothesis being right."""
        from .decode import ctc_segment
        frame_seconds = self._frame_seconds("segments")
        logits, out_len = self._logits(wav_or_mel, lengths)
        ids, n = self._best(logits, out_len)
        L = max(int(n.max()), 1)                               # the one read-back: the label tensors are exactly that wide
        seg = ctc_segment(logits, out_len, ids[:, :L], n, sep=sep)
        out = {"ids": ids, "ids_len": n}
        out.update(seg._asdict())
        out["frame_seconds"] = frame_seconds
        return out

    def transcribe_timed(self, paths, decode: Callable[[torch.Tensor], str], sep=1):
        """WAV files -> one entry per file: {"text", "log_prob", "words"}, words a list of {"word", "start", "end", "confidence"} with
        times in seconds and confidence = exp(word_log_confidence); audio_io.load_batch, segments, then `decode` (the caller's
        tokenizer.decode, ids tensor -> str) on each row's ids and on each word's; one device-to-host copy per tensor.  A time is a
        frame index times frame_seconds; the last frame reaches past the last sample (the mel frames are centred), so an end is cut
        at the file's own duration.  Needs a `mel`."""
        from .audio_io import load_batch
        if self.mel is None:
            raise RuntimeError("ASRPipeline.transcribe_timed: the pipeline has no mel transform to turn waveforms into features")
        if sep is None:
            raise RuntimeError("ASRPipeline.transcribe_timed: words need a separator id (segments(sep=None) gives the label level)")
        wave, wave_len = load_batch(paths, self.mel.sample_rate, self.mel.dft_basis.device)
        out = self.segments(wave, wave_len, sep)
        fs = out["frame_seconds"]
        keys = ("ids", "ids_len", "log_prob", "word_first", "word_count", "word_start", "word_end", "word_log_confidence", "n_words")
        ids, n, log_prob, first, count, start, end, conf, nw = (out[k].cpu() for k in keys)
        conf, seconds = torch.exp(conf), wave_len.cpu().double() / self.mel.sample_rate
        result = []
        for i in range(ids.shape[0]):
            words = [{"word": decode(ids[i, int(first[i, w]):int(first[i, w]) + int(count[i, w])]), "start": int(start[i, w]) * fs,
                      "end": min(int(end[i, w]) * fs, float(seconds[i])), "confidence": float(conf[i, w])} for w in range(int(nw[i]))]
            result.append({"text": decode(ids[i, :int(n[i])]), "log_prob": float(log_prob[i]), "words": words})
        return result


    @torch.no_grad()
    def score(self, wav_or_mel: torch.Tensor, lengths, text: torch.Tensor, text_len: torch.Tensor, sep: int = 1):
        """The ragged call, then decode.edit_distance_both of the decoded ids against text [B, L] int64 / text_len [B] (one launch,
        no read-back).  Returns {"ids" [B, T'] int64, "ids_len" [B] int32, and per utterance, int32 [B]: "char_errors", "hyp_chars",
        "chars" (the id level: distance, decoded ids, reference ids), "word_errors", "hyp_words", "words" (words split at `sep`)}."""
        from .decode import edit_distance_both
        ids, n = self(wav_or_mel, lengths)
        dist, hyp_n, ref_n = edit_distance_both(ids, n, text.to(ids.device), text_len.to(ids.device), sep)
        return {"ids": ids, "ids_len": n, "char_errors": dist[0], "hyp_chars": hyp_n[0], "chars": ref_n[0],
                "word_errors": dist[1], "hyp_words": hyp_n[1], "words": ref_n[1]}

    @torch.no_grad()
    def evaluate(self, batches, sep: int = 1):
        """Error rates over an iterable of (wav_or_mel, lengths, text, text_len): the ragged call and ErrorRate.update per batch, and
        ONE device-to-host synchronisation at the end.  Returns ErrorRate.compute()."""
        meter = ErrorRate(sep)
        for wav_or_mel, lengths, text, text_len in batches:
            ids, n = self(wav_or_mel, lengths)
            meter.update(ids, n, text.to(ids.device), text_len.to(ids.device))
        return meter.compute()


class ErrorRate:
    """Running character (or phone) and word error rates of a validation loop, counted on the device (decode.edit_distance_both, K23).

    update(hyp, hyp_len, ref, ref_len) scores one batch of zero-padded int64 id rows at both levels in one launch and adds the
    batch sums into an int64 device tensor: no device-to-host synchronisation.  compute() does the one read-back and returns
    {"cer", "wer", "char_errors", "chars", "word_errors", "words", "utterances"}: the rates are errors / reference tokens, Python
    floats taken from the integer totals, nan when the reference count is 0.  reset() zeroes the counters.

    sep is the id that separates words; the default 1 is the space of the reference's 29-symbol character vocabulary
    (voice100/text.py: "_ abc...z'", blank 0, space 1).  sep=None (phone vocabularies: no word level) leaves "wer", "word_errors"
    and "words" out; "cer" is then the phone error rate."""

    def __init__(self, sep=1):
        self.sep = sep
        self.totals = None                               # int64 [levels, 3]: errors, hypothesis tokens, reference tokens
        self.utterances = 0

    def reset(self):
        if self.totals is not None:
            self.totals.zero_()
        self.utterances = 0

    @torch.no_grad()
    def update(self, hyp: torch.Tensor, hyp_len: torch.Tensor, ref: torch.Tensor, ref_len: torch.Tensor):
        from .decode import edit_distance, edit_distance_both
        if not hyp.is_cuda:
            raise RuntimeError("ErrorRate.update: GPU tensors only")
        if self.totals is None:
            self.totals = torch.zeros((1 if self.sep is None else 2, 3), dtype=torch.int64, device=hyp.device)
        elif self.totals.device != hyp.device:
            raise RuntimeError("ErrorRate.update: the counters live on another device")
        if self.sep is None:
            edit_distance(hyp, hyp_len, ref, ref_len, None, self.totals, per_row=False)
        else:
            edit_distance_both(hyp, hyp_len, ref, ref_len, self.sep, self.totals, per_row=False)
        self.utterances += hyp.shape[0]

    def compute(self):
        rows = self.totals.cpu().tolist() if self.totals is not None else [[0, 0, 0]] * (1 if self.sep is None else 2)
        rate = lambda e, n: e / n if n > 0 else float("nan")  # noqa: E731
        out = {"cer": rate(rows[0][0], rows[0][2]), "char_errors": rows[0][0], "chars": rows[0][2], "utterances": self.utterances}
        if self.sep is not None:
            out.update({"wer": rate(rows[1][0], rows[1][2]), "word_errors": rows[1][0], "words": rows[1][2]})
        return out


class AlignPipeline:
    """The loop body of voice100/align_text.py:39-56 for one batch, on the device:

        audio [B, T, audio_size], audio_len [B], text [B, Lmax] int64, text_len [B]
          -> model._forward_btv                            logits [B, T_out, V], logits_len      (AudioAlignCTC or AudioToAlignText)
          -> torch.log_softmax                             a stock op: the kernel's additions stay those of the reference
          -> decode.ctc_align, one launch                  Viterbi over min(logits_len, text_len) labels (align.py:147), path,
                                                           labels on the path, durations, scores    (K20, csrc/align.hip)

    Returns {"score" [B] fp32: the per-utterance best-path scores (the reference's ctc_best_path drops them, align.py:161),
    "hist" [B, T_out] int32: positions in the blank-extended text, "path" [B, T_out] int64: the labels there, "path_len" [B],
    "align" [B, 2 Lmax + 1] int32: frames per extended position, laid out for the ORIGINAL text_len and 0 beyond}.
    The module must be in eval mode: dropout would randomise the alignments."""

    def __init__(self, model, max_move: int = 3):
        self.model, self.max_move = model, int(max_move)

    @torch.no_grad()
    def __call__(self, audio: torch.Tensor, audio_len: torch.Tensor, text: torch.Tensor, text_len: torch.Tensor):
        from .decode import ctc_align
        if self.model.training:
            raise RuntimeError("AlignPipeline: the model is in training mode (call model.eval(): dropout would randomise the alignment)")
        if not audio.is_cuda:
            raise RuntimeError("AlignPipeline: GPU tensors only")
        logits, logits_len = self.model._forward_btv(audio, audio_len)
        lp = torch.log_softmax(logits, dim=-1)
        dev = lp.device
        logits_len = logits_len.to(dev)
        lab_len = torch.minimum(logits_len, text_len.to(dev))            # for very short audio (align.py:147)
        score, hist, path, align = ctc_align(lp, text.to(dev), logits_len, lab_len, self.max_move)
        return {"score": score, "hist": hist, "path": path, "path_len": logits_len, "align": align}


def align_records(out, text: torch.Tensor, text_len: torch.Tensor, decode: Callable[[torch.Tensor], str]) -> List[str]:
    """The lines `raw_text|raw_align_text|align` of voice100/align_text.py:48-56 for one AlignPipeline result (no newline).
    `decode` is the caller's tokenizer.decode (ids tensor -> str); one device-to-host copy per tensor, then CPU string work."""
    path, path_len, align = out["path"].cpu(), out["path_len"].cpu(), out["align"].cpu()
    text, text_len = text.cpu(), text_len.cpu()
    lines = []
    for i in range(path.shape[0]):
        n = int(text_len[i])
        durations = " ".join(str(int(x)) for x in align[i, :2 * n + 1])
        lines.append(decode(text[i, :n]) + "|" + decode(path[i, :int(path_len[i])]) + "|" + durations)
    return lines


def window_plan(n_frames: int, keep: int, halo: int, stride: int):
    """How windowed_logits cuts a recording of n_frames input frames: a list of (in_start, in_end, out_skip, out_count) -- the
    forward of input frames [in_start, in_end) gives the recording's output frames from local index out_skip on, out_count of
    them, and the windows in order cover every output frame ((n_frames - 1) // stride + 1 of them) exactly once.  A window is `keep`
    output frames plus `halo` input frames (rounded up to a multiple of `stride`, so that every start is one) on each side; what
    would begin before frame 0 begins there, what would end beyond the end ends there, so those edges see the padding of the whole
    forward."""
    if n_frames < 1 or keep < 1 or halo < 0 or stride < 1:
        raise ValueError("window_plan: n_frames >= 1, keep >= 1, halo >= 0 and stride >= 1 are required")
    n_out = (n_frames - 1) // stride + 1
    h = -(-halo // stride)                               # the halo in output frames
    plan = []
    for o0 in range(0, n_out, keep):
        o1 = min(o0 + keep, n_out)
        w0 = max(o0 - h, 0)
        plan.append((w0 * stride, min((o0 + keep + h) * stride, n_frames), o0 - w0, o1 - o0))
    return plan


@torch.no_grad()
def windowed_logits(model, feats: torch.Tensor, keep: int = 1500, halo=None, max_batch: int = 32) -> torch.Tensor:
    """The logits [T', V] of ONE recording of any length, feats [M, audio_size], as batched forwards over equal windows (window_plan):
    `keep` output frames each plus the encoder's halo on both sides, so a two-hour recording runs at the batch shapes the kernels
    are tuned for and no activation grows with M.  The halo comes from model.receptive_field() (ConvVoiceEncoder derives it from
    its layer list); with it every kept frame sees exactly the inputs the whole forward gives it, and the first and the last window
    end where the recording does, so the result is the whole forward's up to the rounding of differently tiled kernels.  Windows
    of equal shape go `max_batch` at a time; what cannot share a shape (the first and the last windows, typically) runs as its own
    call.  A model without receptive_field() (the LSTM models: their state spans the recording) needs halo= in input frames, and
    the result is then APPROXIMATE: frames near a window's edge miss the context beyond it.  Eval mode only, like AlignPipeline."""
    if model.training:
        raise RuntimeError("windowed_logits: the model is in training mode (call model.eval(): dropout would randomise the logits)")
    if not feats.is_cuda:
        raise RuntimeError("windowed_logits: GPU tensors only")
    if feats.dim() != 2 or feats.shape[0] < 1:
        raise RuntimeError(f"windowed_logits: feats must be [M, audio_size] with M >= 1, got {list(feats.shape)}")
    rf = getattr(model, "receptive_field", None)
    if halo is None:
        if rf is None:
            raise RuntimeError("windowed_logits: the model has no receptive_field() to take the halo from (pass halo= in input "
                               "frames; the result is then approximate)")
        _, halo, stride = rf()
    elif rf is not None:
        stride = rf()[2]
    else:
        stride = 4096 // int(model.output_length(torch.tensor([4096])))
    plan = window_plan(feats.shape[0], int(keep), int(halo), int(stride))
    groups = {}                                          # (input frames, out_skip, out_count) -> window indices
    for w, (i0, i1, skip, count) in enumerate(plan):
        groups.setdefault((i1 - i0, skip, count), []).append(w)
    pieces = [None] * len(plan)
    for (_, skip, count), ws in groups.items():
        for c in range(0, len(ws), max_batch):
            chunk = ws[c:c + max_batch]
            x = torch.stack([feats[plan[w][0]:plan[w][1]] for w in chunk])
            y = model(x)
            for k, w in enumerate(chunk):
                pieces[w] = y[k, skip:skip + count]
    return torch.cat(pieces, dim=0)


def utterance_cuts(path: torch.Tensor, frame_logp: torch.Tensor, cuts, n_labels: int, conf_window: int = 30, free_ends: bool = True):
    """The reductions of LongAlignPipeline on one aligned recording, stock ops on whatever device the tensors are on: path [T]
    (extended positions, non-decreasing, every label visited), frame_logp [T] (the log-probability of the path's symbol at each
    frame), cuts = the label indices where utterances begin (ascending, the first 0) -> a float64 tensor [U, 5] of (start, end,
    frames, mean_logp, min_window_logp) in frames.  The boundary between two utterances is the midpoint of the frames between the
    last label of one and the first label of the next; the first utterance starts at frame 0 and the last ends at T, or with
    free_ends at the first frame of the first label and one past the last frame of the last (what lies outside is the preamble
    and the outro).  min_window_logp is the lowest mean of frame_logp over any conf_window consecutive frames inside the utterance
    (the whole utterance where it is shorter): the CTC-segmentation confidence."""
    dev = path.device
    T = path.shape[0]
    cuts_l = [int(c) for c in cuts]
    U = len(cuts_l)
    if U < 1 or cuts_l[0] != 0 or any(b <= a for a, b in zip(cuts_l, cuts_l[1:])) or cuts_l[-1] >= n_labels:
        raise ValueError("utterance_cuts: cuts must be ascending label indices that begin with 0 and stay below the number of labels")
    cuts_t = torch.tensor(cuts_l, dtype=torch.int64, device=dev)
    p = path.to(torch.int64).contiguous()
    first = torch.searchsorted(p, 2 * cuts_t + 1)                                      # first frame of each utterance's first label
    last_lab = torch.cat([cuts_t[1:] - 1, torch.tensor([n_labels - 1], dtype=torch.int64, device=dev)])
    last = torch.searchsorted(p, 2 * last_lab + 1, right=True)                         # one past the last frame of its last label
    mid = torch.div(last[:-1] + first[1:], 2, rounding_mode="floor")
    lo_edge = first[:1] if free_ends else torch.zeros(1, dtype=torch.int64, device=dev)
    hi_edge = last[-1:] if free_ends else torch.full((1,), T, dtype=torch.int64, device=dev)
    start, end = torch.cat([lo_edge, mid]), torch.cat([mid, hi_edge])
    frames = end - start
    cs = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), torch.cumsum(frame_logp.to(torch.float64), 0)])
    nz = frames.clamp_min(1).to(torch.float64)
    mean = (cs[end] - cs[start]) / nz
    cw = torch.minimum(frames, torch.full_like(frames, int(conf_window))).clamp_min(1)  # a short utterance is one window
    t = torch.arange(T, dtype=torch.int64, device=dev)
    uid = (torch.searchsorted(start, t, right=True) - 1).clamp_min(0)                   # the utterance a window starting at t belongs to
    w_end = t + cw[uid]
    inside = (t >= start[uid]) & (w_end <= end[uid])
    wmean = (cs[w_end.clamp_max(T)] - cs[t]) / cw[uid].to(torch.float64)
    wmean = torch.where(inside, wmean, torch.full_like(wmean, float("inf")))
    wmin = torch.full((U,), float("inf"), dtype=torch.float64, device=dev).scatter_reduce(0, uid, wmean, "amin")
    wmin = torch.where(frames > 0, wmin, mean)
    return torch.stack([start.double(), end.double(), frames.double(), mean, wmin], dim=1)


class LongAlignPipeline:
    """A chapter-length recording and its text -> utterance cut points with confidences, on the device:

        path or waveform
          -> audio_io.load_batch (load_audio + resample)   the recording at the mel's sample rate
          -> mel                                           feats [M, audio_size]
          -> windowed_logits                               logits [T', V] from batched forwards over equal windows
          -> torch.log_softmax                             a stock op: the kernel holds no transcendentals
          -> decode.ctc_align_long, one launch             the banded Viterbi path over all T' frames        (K29, csrc/align_long.hip)
          -> utterance_cuts                                gather, an fp64 cumsum, and ONE read-back

    align() returns {"ok": bool, "score": float (the path's log-probability), "frame_seconds": float, "utterances": a list, one
    entry per element of `cuts`, of {"start_s", "end_s", "frames", "mean_logp", "min_window_logp"}}.  ok False (the band lost the path
    or the text does not fit the frames: widen `band`) comes with an empty list.  Seconds follow ASRPipeline's frame-period rule."""

    def __init__(self, model, mel=None, band: int = 2048, keep: int = 1500, free_ends: bool = True, conf_window: int = 30,
                 frame_seconds=None, blank: int = 0):
        self.model, self.mel = model, mel
        self.band, self.keep, self.free_ends, self.conf_window, self.blank = int(band), int(keep), bool(free_ends), int(conf_window), int(blank)
        self.frame_seconds = frame_seconds

    def _feats(self, path_or_wave):
        if self.mel is None:
            raise RuntimeError("LongAlignPipeline.align: the pipeline has no mel transform to turn a waveform into features (pass feats=)")
        if isinstance(path_or_wave, torch.Tensor):
            wave = path_or_wave.to(self.mel.dft_basis.device)
        else:
            from .audio_io import load_batch
            wave = load_batch([path_or_wave], self.mel.sample_rate, self.mel.dft_basis.device)[0][0]
        return self.mel(wave.reshape(1, -1))[0]

    @torch.no_grad()
    def align(self, path_or_wave, text_ids, cuts, feats: torch.Tensor = None):
        """path_or_wave: a WAV / FLAC file, or a waveform [N] at the mel's sample rate; or feats [M, audio_size] directly.
        text_ids: the whole text's label ids ([L], a tensor or a sequence); cuts: the label indices where utterances begin."""
        from .decode import ctc_align_long
        frame_seconds = ASRPipeline(self.model, self.mel, frame_seconds=self.frame_seconds)._frame_seconds("align")
        if feats is None:
            feats = self._feats(path_or_wave)
        logits = windowed_logits(self.model, feats, self.keep)
        lp = torch.log_softmax(logits.float(), dim=-1)
        dev = lp.device
        text = torch.as_tensor(text_ids, dtype=torch.int64).to(dev).reshape(1, -1)
        L = text.shape[1]
        res = ctc_align_long(lp[None], text, band=self.band, blank=self.blank, free_ends=self.free_ends)
        ext = torch.full((2 * L + 1,), self.blank, dtype=torch.int64, device=dev)
        ext[1::2] = text[0]
        pos = res.path[0].long()
        frame_logp = lp.gather(1, ext[pos].clamp(0, lp.shape[1] - 1)[:, None])[:, 0]
        if self.free_ends:                               # the two end states emitted the best symbol's log-probability
            frame_logp = torch.where((pos == 0) | (pos == 2 * L), lp.amax(-1), frame_logp)
        table = utterance_cuts(res.path[0], frame_logp, cuts, L, self.conf_window, self.free_ends)
        head = torch.stack([res.score[0], res.ok[0].double()])
        flat = torch.cat([head, table.reshape(-1)]).cpu()                    # the one read-back
        ok = bool(flat[1] != 0)
        rows = flat[2:].reshape(-1, 5).tolist() if ok else []
        utts = [{"start_s": r[0] * frame_seconds, "end_s": r[1] * frame_seconds, "frames": int(r[2]), "mean_logp": r[3],
                 "min_window_logp": r[4]} for r in rows]
        return {"ok": ok, "score": float(flat[0]), "frame_seconds": frame_seconds, "utterances": utts}


def cut_utterances(wave: torch.Tensor, sample_rate: int, out, paths, pad_s: float = 0.0, bits_per_sample: int = 16, **enc):
    """Turn a `LongAlignPipeline.align` result into files: utterance u's samples [floor((start_s - pad_s) rate), ceil((end_s + pad_s) rate)),
    clamped to the recording, go to paths[u] (.flac: all of them in ONE `encode_flac` call that reads the segments in place through
    rows / starts; .wav: one copy of the recording to the host).  wave: the recording [samples] or [channels, samples] on the device.
    Returns the sample ranges [(begin, end)].  Raises, and writes nothing, when the alignment failed (`ok` False), when the number
    of paths differs from the number of utterances, or when an utterance is empty."""
    import math
    from . import audio_io as A
    if not out.get("ok", False):
        raise ValueError("cut_utterances: the alignment failed (ok is False): nothing is written")
    utts, paths = out["utterances"], list(paths)
    if len(paths) != len(utts):
        raise ValueError(f"cut_utterances: {len(paths)} paths for {len(utts)} utterances")
    if wave.dim() not in (1, 2):
        raise ValueError(f"cut_utterances: the recording must be [samples] or [channels, samples] (got {tuple(wave.shape)})")
    kinds = [A._audio_kind(p, "cut_utterances") for p in paths]
    total = wave.shape[-1]
    ranges = []
    for u, ut in enumerate(utts):
        a = min(max(math.floor((ut["start_s"] - pad_s) * sample_rate), 0), total)
        e = min(max(math.ceil((ut["end_s"] + pad_s) * sample_rate), 0), total)
        if e <= a:
            raise ValueError(f"cut_utterances: utterance {u} ({ut['start_s']:.3f} s .. {ut['end_s']:.3f} s) holds no samples")
        ranges.append((a, e))
    fl = [u for u, k in enumerate(kinds) if k == "flac"]
    if fl:
        rec = wave[None] if wave.dim() == 2 else wave[None, None]
        files = A.encode_flac(rec, [ranges[u][1] - ranges[u][0] for u in fl], sample_rate, bits_per_sample, rows=[0] * len(fl),
                              starts=[ranges[u][0] for u in fl], **enc)
    host = wave.cpu() if len(fl) < len(paths) else None
    if host is not None:
        A._pcm_bytes(host, bits_per_sample, "cut_utterances")          # refuses a non-finite sample before anything is written
    for u, data in zip(fl, files if fl else []):
        with open(paths[u], "wb") as f:
            f.write(data)
    for u, k in enumerate(kinds):
        if k == "wav":
            A.save_wav(paths[u], host[..., ranges[u][0]:ranges[u][1]], sample_rate, bits_per_sample)
    return ranges


def align_long_records(out, text_ids, cuts, decode: Callable[[torch.Tensor], str]) -> List[str]:
    """The lines `start|end|confidence|text` for one LongAlignPipeline.align result (no newline): seconds with three decimals, the
    confidence = min_window_logp (a log-probability per frame: nearer 0 is better), and `decode` (the caller's tokenizer.decode, ids
    tensor -> str, as in align_records) on each utterance's labels."""
    text = torch.as_tensor(text_ids, dtype=torch.int64).cpu().reshape(-1)
    edges = list(cuts) + [text.numel()]
    return [f"{u['start_s']:.3f}|{u['end_s']:.3f}|{u['min_window_logp']:.4f}|" + decode(text[edges[i]:edges[i + 1]])
            for i, u in enumerate(out["utterances"])]


def batch_plan(n_segments: int, max_batch: int):
    """How LongASRPipeline packs its segments, sorted by length (longest first), into decode calls: [(lo, hi)] over the sorted order,
    at most max_batch rows each, every segment exactly once.  The first row of a call is its longest: the call is padded to it."""
    if n_segments < 0 or max_batch < 1:
        raise ValueError("batch_plan: n_segments >= 0 and max_batch >= 1 are required")
    return [(lo, min(lo + max_batch, n_segments)) for lo in range(0, n_segments, max_batch)]


def join_ids(rows, sep):
    """The ids of a whole transcript from its utterances' (lists of ints): the utterances in order, with the separator id between two
    of them wherever neither supplies one (the one before does not end with it and the one after does not begin with it); empty
    utterances are left out.  sep=None: plain concatenation."""
    out = []
    for row in rows:
        row = [int(i) for i in row]
        if not row:
            continue
        if out and sep is not None and out[-1] != sep and row[0] != sep:
            out.append(int(sep))
        out.extend(row)
    return out


class LongASRPipeline:
    """A chapter-length recording -> its transcript as utterances with times, on the device:

        path or waveform
          -> audio_io.load_batch, mel                      feats [M, audio_size]
          -> windowed_logits                               logits [T', V] from batched forwards over equal windows
          -> decode.ctc_cut_points                         where to cut: at the pauses, pieces of at most max_frames frames  (K31)
          -> gather                                        the segments sorted by length, at most max_batch rows per call, each call
                                                           padded to its longest (stock indexing ops)
          -> the decode of an ASRPipeline                  greedy, the prefix beam search, or the beam search with the LM   (K24, K25)
          -> decode.ctc_segment (timed, or greedy)         times and confidences of the labels and words of each segment     (K26)
          -> offsets                                       every frame index moves by its segment's start

    The one-call beam search and ctc_segment stop at 4096 frames and run one workgroup per row, so a recording is decoded as a batch
    of its pieces (their long forms, K32's ctc_beam_search_long and K33's ctc_segment_long, serve whole()).  Cutting inside a run of
    blank frames costs the greedy decode nothing (CTC never merges labels across a blank: the pieces' decodes, concatenated, are the
    recording's); the beam search loses only what it would have carried across the pause,
    and THE LANGUAGE MODEL'S CONTEXT RESTARTS AT EVERY CUT: each segment is scored as a sentence of its own.  A forced cut (a
    stretch of max_frames frames without an admissible pause) may split a word; its segment says so in "forced".  whole() (K32) has
    none of the three: it decodes the recording as one utterance with a resumable beam, one frame after the other, at many times
    the cost; with confidences=True decode.ctc_segment_long (K33) adds the soft times and the confidences of its labels and words.
    An ASRPipeline is held and called for the decode; blank must be 0, as there.  Eval mode only, like windowed_logits.
    Device-to-host copies: the number of segments S, one copy of the calls' widths, and the longest hypothesis of each call."""

    def __init__(self, model, mel=None, beam_size=None, lm=None, lm_weight=0.5, length_bonus=0.0, keep=1500, max_frames=3000, min_gap=25,
                 margin=0.0, pad=5, min_frames=50, max_batch=32, blank=0, sep=1, frame_seconds=None, band=2048, seg_band=256,
                 word_lm=None, word_lm_weight=0.5, word_bonus=0.0, rescore_size=None, mbr=None, mbr_scale=1.0, mbr_size=None):
        if int(blank) != 0:
            raise RuntimeError(f"LongASRPipeline: blank = {blank}; the decode of ASRPipeline takes the blank at id 0")
        if int(max_batch) < 1:
            raise RuntimeError(f"LongASRPipeline: max_batch = {max_batch} must be at least 1")
        self.asr = ASRPipeline(model, mel, beam_size=beam_size, nbest=1, lm=lm, lm_weight=lm_weight, length_bonus=length_bonus,
                               frame_seconds=frame_seconds, word_lm=word_lm, word_lm_weight=word_lm_weight, word_bonus=word_bonus,
                               rescore_size=rescore_size, sep=sep, mbr=mbr, mbr_scale=mbr_scale, mbr_size=mbr_size)
        self.model, self.mel = model, mel
        self.keep, self.max_batch, self.blank, self.sep = int(keep), int(max_batch), int(blank), sep
        self.band = int(band)                                # whole(): ctc_align_long's band
        self.seg_band = int(seg_band)                        # whole(confidences=True): ctc_segment_long's band
        self.cut = dict(max_frames=int(max_frames), min_gap=min_gap, margin=float(margin), pad=int(pad), min_frames=int(min_frames))

    def _wave(self, path_or_wave, who):
        if self.mel is None:
            raise RuntimeError(f"LongASRPipeline.{who}: the pipeline has no mel transform to turn a waveform into features (pass feats= "
                               "or logits=)")
        if isinstance(path_or_wave, torch.Tensor):
            return path_or_wave.to(self.mel.dft_basis.device).reshape(-1)
        from .audio_io import load_batch
        return load_batch([path_or_wave], self.mel.sample_rate, self.mel.dft_basis.device)[0][0]

    def _frame_seconds(self):
        if self.asr.frame_seconds is None and self.mel is None:
            return None
        return self.asr._frame_seconds("segments")

    @torch.no_grad()
    def segments(self, path_or_wave=None, feats: torch.Tensor = None, logits: torch.Tensor = None, timed: bool = True):
        """path_or_wave: a WAV / FLAC file or a waveform [N] at the mel's sample rate; or feats [M, audio_size]; or logits [T', V]
        that are already there.  Returns a dict of device tensors, segments in the recording's order: "seg_start", "seg_end", "forced" [S]
        int32 (decode.ctc_cut_points); "ids" [S, L] int64 zero padded and "ids_len" [S] int32, L the longest hypothesis; "score" [S]
        fp32: the beam search's score (the fused one with a language model), or for the greedy decode ctc_segment's log_prob; with
        timed=True (or the greedy decode) the fields of decode.CTCSegments, [S, ...], whose frame fields ("start", "end",
        "word_start", "word_end") are moved by seg_start inside each row's labels / words, so they count the recording's frames;
        and "frame_seconds" (a float, or None where the pipeline has neither a mel nor frame_seconds)."""
        from .decode import ctc_cut_points, ctc_segment
        if logits is None:
            if feats is None:
                feats = self.mel(self._wave(path_or_wave, "segments").reshape(1, -1))[0]
            logits = windowed_logits(self.model, feats, self.keep)
        if not logits.is_cuda:
            raise RuntimeError("LongASRPipeline.segments: GPU tensors only")
        if logits.dim() != 2:
            raise RuntimeError(f"LongASRPipeline.segments: logits must be [T', V], got {list(logits.shape)}")
        logits = logits.contiguous().float()
        dev = logits.device
        T = logits.shape[0]
        cp = ctc_cut_points(logits[None], None, self.blank, **self.cut)
        seg_start, seg_end, forced = cp.start[0], cp.end[0], cp.forced[0]
        S = seg_start.shape[0]                               # (ctc_cut_points read it back)
        out = {"seg_start": seg_start, "seg_end": seg_end, "forced": forced}
        greedy = self.asr.beam_size is None
        with_seg = timed or greedy
        seg_len = seg_end - seg_start
        order = torch.argsort(seg_len, descending=True, stable=True)
        plan = batch_plan(S, self.max_batch)
        widths = seg_len[order][::self.max_batch].cpu().tolist() if S else []       # the longest of each call, one copy
        parts = []
        for (lo, hi), width in zip(plan, widths):
            rows = order[lo:hi]
            st, ln = seg_start[rows].long(), seg_len[rows].contiguous()
            idx = (st[:, None] + torch.arange(width, device=dev)[None]).clamp_max(T - 1)
            x = logits[idx]                                   # [rows, width, V]; what lies beyond a row's length is never read
            if greedy:
                ids, n = self.asr._best(x, ln)
                score = None
            else:
                ids, n, score = self.asr._top(x, ln)
                n = n.contiguous()
            L = max(int(n.max()), 1)
            ids = ids[:, :L].contiguous()
            seg = ctc_segment(x, ln, ids, n, blank=self.blank, sep=self.sep) if with_seg else None
            parts.append((rows, st, ids, n, score if score is not None else seg.log_prob, seg, L))
        L = max([p[6] for p in parts], default=1)
        ids_all = torch.zeros((S, L), dtype=torch.int64, device=dev)
        n_all = torch.zeros((S,), dtype=torch.int32, device=dev)
        score_all = torch.zeros((S,), dtype=torch.float32, device=dev)
        fields = {}
        if with_seg:
            NW = (L + 1) // 2
            wide = {"start": torch.int32, "end": torch.int32, "duration": torch.float32, "log_confidence": torch.float32}
            words = {"word_first": torch.int32, "word_count": torch.int32, "word_start": torch.int32, "word_end": torch.int32,
                     "word_log_confidence": torch.float32} if self.sep is not None else {}
            fields = {k: torch.zeros((S, L), dtype=dt, device=dev) for k, dt in wide.items()}
            fields.update({k: torch.zeros((S, NW), dtype=dt, device=dev) for k, dt in words.items()})
            fields["log_prob"] = torch.zeros((S,), dtype=torch.float32, device=dev)
            fields["n_words"] = torch.zeros((S,), dtype=torch.int32, device=dev) if self.sep is not None else None
            for k in ("word_first", "word_count", "word_start", "word_end", "word_log_confidence"):
                fields.setdefault(k, None)
        for rows, st, ids, n, score, seg, Lc in parts:
            ids_all[rows, :Lc] = ids
            n_all[rows] = n
            score_all[rows] = score
            if seg is None:
                continue
            shift = st.int()[:, None]
            in_labels = torch.arange(Lc, device=dev)[None] < n[:, None]
            for k, v in seg._asdict().items():
                if v is None:
                    continue
                if k in ("start", "end"):
                    v = torch.where(in_labels, v + shift, v)
                elif k in ("word_start", "word_end"):
                    v = torch.where(torch.arange(v.shape[1], device=dev)[None] < seg.n_words[:, None], v + shift, v)
                if v.dim() == 1:
                    fields[k][rows] = v
                else:
                    fields[k][rows, :v.shape[1]] = v
        out.update({"ids": ids_all, "ids_len": n_all, "score": score_all})
        out.update(fields)
        out["frame_seconds"] = self._frame_seconds()
        return out

    def transcribe(self, path, decode: Callable[[torch.Tensor], str]):
        """A WAV / FLAC file -> {"text", "utterances": [{"start_s", "end_s", "text", "score", "forced", "words": [{"word", "start",
        "end", "confidence"}]}], "frame_seconds"}, following ASRPipeline.transcribe_timed: times in seconds, an end cut at the file's
        own duration, confidence = exp(word_log_confidence), `decode` the caller's tokenizer.decode (ids tensor -> str).  "text" is
        the decode of all utterances' ids, joined by the separator id wherever neither neighbour supplies one (join_ids).  Needs a
        `mel` and a separator id; one device-to-host copy per tensor."""
        if self.sep is None:
            raise RuntimeError("LongASRPipeline.transcribe: words need a separator id (segments() gives the label level)")
        wave = self._wave(path, "transcribe")
        out = self.segments(wave)
        fs = out["frame_seconds"]
        seconds = wave.shape[0] / self.mel.sample_rate
        keys = ("seg_start", "seg_end", "forced", "ids", "ids_len", "score", "word_first", "word_count", "word_start", "word_end",
                "word_log_confidence", "n_words")
        s0, s1, forced, ids, n, score, first, count, start, end, conf, nw = (out[k].cpu() for k in keys)
        conf = torch.exp(conf)
        utts = []
        for i in range(ids.shape[0]):
            words = [{"word": decode(ids[i, int(first[i, w]):int(first[i, w]) + int(count[i, w])]), "start": int(start[i, w]) * fs,
                      "end": min(int(end[i, w]) * fs, seconds), "confidence": float(conf[i, w])} for w in range(int(nw[i]))]
            utts.append({"start_s": int(s0[i]) * fs, "end_s": min(int(s1[i]) * fs, seconds), "text": decode(ids[i, :int(n[i])]),
                         "score": float(score[i]), "forced": bool(forced[i]), "words": words})
        whole = join_ids([ids[i, :int(n[i])].tolist() for i in range(ids.shape[0])], self.sep)
        return {"text": decode(torch.tensor(whole, dtype=torch.int64)), "utterances": utts, "frame_seconds": fs}

    @torch.no_grad()
    def whole(self, path_or_wave=None, feats: torch.Tensor = None, logits: torch.Tensor = None, timed: bool = True, chunk: int = 4096,
              confidences: bool = False):
        """The recording decoded as ONE utterance (K32): windowed_logits, then decode.ctc_beam_search_long over all its frames -- the
        beam is never restarted, the language model keeps one context, no cut can split a word -- and with timed=True
        decode.ctc_align_long of the best transcript on the log-softmax of the same logits (band = the constructor's).  The inputs
        are segments()'.  Needs a beam_size: the greedy decode of the pieces already concatenates to the recording's.  One workgroup
        walks the frames one after the other, so this is much slower than segments() (see decode.ctc_beam_search_long), and its
        memory grows with the recording.  Returns a dict of device tensors: "ids" [L] int64 and "ids_len", "score" (0-dim; the fused
        score with a language model, then also "ctc_score" and "lm_score"); with timed "start", "end" [L] int32 = each label's first
        frame and one past its last on the best path (the cumulative sum of the aligner's frames per position) and "ok" (0-dim
        int32; 0: the band lost the path, start = end = 0 -- widen band); and "frame_seconds".  confidences=True (it needs timed) adds
        what decode.ctc_segment_long (K33) computes inside the corridor of seg_band states (the constructor's) round that path -- ctc_segment
        itself stops at 4096 frames: "log_prob" (0-dim fp64), "soft_start", "soft_end" [L] int32 (the posterior medians, where
        "start" / "end" are the best path's), "duration", "log_confidence" [L] fp32, the word fields "word_first", "word_count",
        "word_start", "word_end", "word_log_confidence" and "n_words" (None without a separator id), and "seg_ok" (0-dim int32; 0:
        no alignment inside the corridor, or the aligner lost the path: then the new keys hold what a row without an alignment gets,
        log_prob -inf, times and durations 0, confidences -inf).  The other keys are what they are without it, bit for bit.
        One read-back, of ids_len, sizes L.  With a word model (K34) the search returns its rescore_size best, decode.rescore_nbest re-ranks
        them (one more read-back, of the longest hypothesis), every key above describes the top one after that, and "first_score" and
        "word_lm_score" (0-dim) are added.  With mbr (K35) the search returns its mbr_size best, the second pass (if any) re-ranks them,
        decode.mbr_nbest picks the one of least expected error, every key describes that one, and "risk" and "expected_len" are added."""
        from .decode import ctc_align_long, ctc_beam_search_long, ctc_segment_long
        a = self.asr
        if a.beam_size is None:
            raise RuntimeError("LongASRPipeline.whole: the pipeline decodes greedily, and the greedy decodes of segments()' pieces "
                               "already concatenate to the recording's exactly (pass beam_size=)")
        if logits is None:
            if feats is None:
                feats = self.mel(self._wave(path_or_wave, "whole").reshape(1, -1))[0]
            logits = windowed_logits(self.model, feats, self.keep)
        if not logits.is_cuda:
            raise RuntimeError("LongASRPipeline.whole: GPU tensors only")
        if logits.dim() != 2:
            raise RuntimeError(f"LongASRPipeline.whole: logits must be [T', V], got {list(logits.shape)}")
        logits = logits.contiguous().float()
        size = a.mbr_size if a.mbr is not None else 1 if a.word_lm is None else a.rescore_size
        res = ctc_beam_search_long(logits[None], None, a.beam_size, size, self.blank, a.lm, a.lm_weight, a.length_bonus, chunk=chunk)
        extra = {}
        if a.mbr is not None:                                # K35 as the last stage, after the second pass where there is one
            width = max(int(res[1].max()), 1)                # a second read-back: the rows are as wide as the frames, the labels far fewer
            if width > 4096:
                raise RuntimeError(f"LongASRPipeline.whole: mbr takes hypotheses of up to 4096 labels, and one has {width} "
                                   "(segments() selects piece by piece)")
            hyps = (res[0][:, :, :width].contiguous(),) + tuple(res[1:3])
            rs = None if a.word_lm is None else a._rescore(hyps)
            m = a._mbr(hyps if rs is None else rs)
            top = m.order[0, 0].long()                       # its index in the list that mbr_nbest was given
            extra = {"risk": m.risk[0, 0], "expected_len": m.expected_len[0]}
            if rs is not None:
                extra.update({"first_score": rs.first_scores[0, top], "word_lm_score": rs.word_lm_scores[0, top]})
                top = rs.order[0, top].long()
            res = (m.ids, m.lens, m.scores) + tuple(t[:, top][:, None] for t in res[3:])
        elif a.word_lm is not None:                          # the second pass (K34): the top of the rescore_size best, re-ranked
            width = max(int(res[1].max()), 1)                # a second read-back: the rows are as wide as the frames, the labels far fewer
            if width > 4096:
                raise RuntimeError(f"LongASRPipeline.whole: the word model rescores hypotheses of up to 4096 labels, and one has {width} "
                                   "(segments() rescores piece by piece)")
            rs = a._rescore((res[0][:, :, :width].contiguous(),) + tuple(res[1:]))
            top = rs.order[0, 0].long()
            extra = {"first_score": rs.first_scores[0, 0], "word_lm_score": rs.word_lm_scores[0, 0]}
            res = (rs.ids, rs.lens, rs.scores) + tuple(t[:, top][:, None] for t in res[3:])
        n = res[1][0, 0]
        L = max(int(n), 1)                                   # the one read-back
        ids = res[0][0, 0, :L].contiguous()
        out = {"ids": ids, "ids_len": n, "score": res[2][0, 0]}
        if a.lm is not None:
            out.update({"ctc_score": res[3][0, 0], "lm_score": res[4][0, 0]})
        out.update(extra)
        if timed:
            al = ctc_align_long(torch.log_softmax(logits, dim=-1)[None], ids[None], None, n.reshape(1), band=self.band, blank=self.blank)
            ends = torch.cumsum(al.align[0], 0, dtype=torch.int32)[1:2 * L:2]        # label i sits at extended position 2 i + 1
            out.update({"start": ends - al.align[0, 1:2 * L:2], "end": ends, "ok": al.ok[0]})
            if confidences:
                seg = ctc_segment_long(logits[None], None, ids[None], n.reshape(1), path=al.path, path_ok=al.ok, band=self.seg_band,
                                       blank=self.blank, sep=self.sep)
                first = lambda t: None if t is None else t[0]                    # noqa: E731
                out.update({"log_prob": seg.log_prob[0], "soft_start": seg.start[0], "soft_end": seg.end[0], "duration": seg.duration[0],
                            "log_confidence": seg.log_confidence[0], "word_first": first(seg.word_first),
                            "word_count": first(seg.word_count), "word_start": first(seg.word_start), "word_end": first(seg.word_end),
                            "word_log_confidence": first(seg.word_log_confidence), "n_words": first(seg.n_words),
                            "seg_ok": seg.ok[0]})
        elif confidences:
            raise RuntimeError("LongASRPipeline.whole: confidences=True needs timed=True (the corridor is built round the aligner's path)")
        out["frame_seconds"] = self._frame_seconds()
        return out

    def transcribe_whole(self, path, decode: Callable[[torch.Tensor], str], confidences: bool = False):
        """A WAV / FLAC file -> {"text", "words": [{"word", "start", "end"}], "score", "frame_seconds"} from whole(): times in seconds,
        an end cut at the file's own duration, a word a maximal run of labels other than the separator, `decode` the caller's
        tokenizer.decode (ids tensor -> str).  confidences=True: whole(confidences=True), and every word also carries "confidence" =
        exp(word_log_confidence), as ASRPipeline.transcribe_timed's do (0 where seg_ok is 0).  Needs a `mel` and a separator id."""
        if self.sep is None:
            raise RuntimeError("LongASRPipeline.transcribe_whole: words need a separator id (whole() gives the label level)")
        wave = self._wave(path, "transcribe_whole")
        out = self.whole(wave, confidences=confidences)
        fs = out["frame_seconds"]
        seconds = wave.shape[0] / self.mel.sample_rate
        n = int(out["ids_len"])
        ids, start, end = (out[k].cpu()[:n] for k in ("ids", "start", "end"))
        words, first = [], None
        for i in range(n + 1):
            if i < n and int(ids[i]) != self.sep:
                first = i if first is None else first
            elif first is not None:
                words.append({"word": decode(ids[first:i]), "start": int(start[first]) * fs, "end": min(int(end[i - 1]) * fs, seconds)})
                first = None
        if confidences:                                      # the word level of ctc_segment_long delimits words by the same rule
            conf = torch.exp(out["word_log_confidence"]).cpu()
            for w, word in enumerate(words):
                word["confidence"] = float(conf[w])
        return {"text": decode(ids), "words": words, "score": float(out["score"]), "frame_seconds": fs}


def long_transcript_records(result) -> List[str]:
    """The lines `start|end|score|text` for one LongASRPipeline.transcribe result (no newline): seconds with three decimals and the
    utterance's score (a log-probability) with four, like align_long_records."""
    return [f"{u['start_s']:.3f}|{u['end_s']:.3f}|{u['score']:.4f}|{u['text']}" for u in result["utterances"]]


class GraphedForward:
    """One eval-mode forward recorded as a HIP graph (torch.cuda.CUDAGraph) and replayed per call.

    The small shapes are launch-bound, not GPU-bound: configs[0] (AudioToTextCTC on 2 x 256 frames) is ~30 launches of a few microseconds
    each, so the host's per-launch cost IS the latency; a graph submits them as one unit.  Large batches gain nothing (the GPU is the
    bottleneck there) and the training step is not capturable (its augmentation draws upload fresh host data every iteration).

    fn: a callable of CUDA tensors whose shapes never change (a model in eval mode, `model.predict`, a pipeline without host read-backs);
    example inputs fix the shapes.  Calls copy their arguments into the graph's static inputs and return the graph's static outputs --
    OVERWRITTEN by the next call (clone what must survive).  Weights are read in place: an optimizer step or load_state_dict between calls
    is seen by the next replay only if no derived copy is involved -- re-record after changing weights."""

    def __init__(self, fn, *example: torch.Tensor, warmup: int = 3):
        if not example or not all(isinstance(e, torch.Tensor) and e.is_cuda for e in example):
            raise RuntimeError("GraphedForward: example inputs must be CUDA tensors")
        self.static_in = [e.clone() for e in example]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(max(1, warmup)):            # one-time work (derived weight copies, plans, table uploads) happens here, not in the graph
                fn(*self.static_in)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.static_out = fn(*self.static_in)

    def __call__(self, *args: torch.Tensor):
        if len(args) != len(self.static_in):
            raise TypeError(f"GraphedForward: expected {len(self.static_in)} inputs")
        for dst, a in zip(self.static_in, args):
            if a.shape != dst.shape or a.dtype != dst.dtype:
                raise RuntimeError(f"GraphedForward: recorded for {tuple(dst.shape)} {dst.dtype}, got {tuple(a.shape)} {a.dtype} (record another graph)")
            dst.copy_(a, non_blocking=True)
        self.graph.replay()
        return self.static_out
