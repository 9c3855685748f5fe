"""From WAV files to ids on ragged batches: audio_io.load_batch, data.AudioTextCollate and the length-aware infer.ASRPipeline,
each against the same thing built by hand, one utterance at a time (load_wav + resample + transform per file, then pad_sequence:
what the reference's dataset and collate do, data_modules.py:287-292 and 446-455).  Equality is exact throughout: the batched
calls run the same arithmetic on the same samples."""
import math
import wave

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pad_sequence

from voice100_amd.asr import AudioToTextCTC
from voice100_amd.audio_io import load_batch, load_wav, resample
from voice100_amd.data import BLANK_AUDIO, BLANK_IDX, AudioTextCollate
from voice100_amd.decode import ctc_greedy_decode
from voice100_amd.infer import ASRPipeline
from voice100_amd.mel import MelSpectrogramAudioTransform
from voice100_amd.trainer import TrainStep

pytestmark = pytest.mark.gpu

SR = 16000
FILES = [(16000, 0.5, 1), (16000, 1.2, 2), (8000, 0.3, 1), (22050, 0.75, 1), (16000, 0.31, 1)]   # (rate, seconds, channels)
ALPHABET = "_abcdefghijklmnopqrstuvwxyz' "


def decode(ids):
    return "".join(ALPHABET[int(i)] for i in ids)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory, cuda):
    """Five 16-bit PCM files (three rates, one stereo) and, per file, what the per-utterance path gives."""
    root = tmp_path_factory.mktemp("ragged_wavs")
    rng = np.random.default_rng(0)
    tr = MelSpectrogramAudioTransform().to(cuda)
    paths, waves, feats = [], [], []
    for k, (rate, seconds, channels) in enumerate(FILES):
        pcm = (rng.standard_normal((round(rate * seconds), channels)) * 3000).astype("<i2")
        path = str(root / f"utt{k}.wav")
        with wave.open(path, "wb") as f:
            f.setnchannels(channels)
            f.setsampwidth(2)
            f.setframerate(rate)
            f.writeframes(pcm.tobytes())
        waveform, sr = load_wav(path)
        assert sr == rate and waveform.shape == (channels, pcm.shape[0])
        w = resample(waveform[0].to(cuda), sr, SR)
        paths.append(path)
        waves.append(w)
        feats.append(tr.transform(w))
    gen = torch.Generator().manual_seed(1)
    texts = [torch.randint(1, 29, (n,), generator=gen) for n in (7, 12, 3, 9, 5)]
    audio = pad_sequence(feats, batch_first=True, padding_value=BLANK_AUDIO)
    audio_len = torch.tensor([f.shape[0] for f in feats], dtype=torch.int32, device=cuda)
    return {"tr": tr, "paths": paths, "waves": waves, "feats": feats, "texts": texts, "audio": audio, "audio_len": audio_len}


def test_load_batch_matches_the_per_file_path_in_the_order_of_paths(corpus, cuda):
    wave_, wave_len = load_batch(corpus["paths"], SR, cuda)
    waves = corpus["waves"]
    assert wave_.dtype == torch.float32 and wave_len.dtype == torch.int32 and wave_.is_cuda and wave_len.is_cuda
    assert wave_.shape == (5, max(w.shape[0] for w in waves))
    assert wave_len.tolist() == [w.shape[0] for w in waves]
    for b, w in enumerate(waves):
        assert torch.equal(wave_[b, :w.shape[0]], w), b
        assert not wave_[b, w.shape[0]:].any(), b
    # another order of the same files: the rows follow it
    order = [3, 0, 2, 4, 1]
    again, again_len = load_batch([corpus["paths"][i] for i in order], SR)
    assert torch.equal(again, wave_[order]) and torch.equal(again_len, wave_len[order])
    # one rate only, already the target's: copied through
    same, same_len = load_batch([corpus["paths"][4], corpus["paths"][0]], SR, cuda)
    assert same.shape == (2, 8000) and same_len.tolist() == [4960, 8000]
    assert torch.equal(same[1], waves[0]) and torch.equal(same[0, :4960], waves[4]) and not same[0, 4960:].any()


def test_collate_equals_the_hand_built_batch_and_trains(corpus, cuda):
    tr, paths, texts = corpus["tr"], corpus["paths"], corpus["texts"]
    collate = AudioTextCollate(tr)
    batch = collate(list(zip(paths, texts)))
    (audio, audio_len), (text, text_len) = batch
    assert (audio.dtype, audio_len.dtype, text.dtype, text_len.dtype) == (torch.float32, torch.int32, torch.int64, torch.int32)
    assert all(t.device == audio.device for t in (audio_len, text, text_len)) and audio.is_cuda
    assert torch.equal(audio, corpus["audio"]) and torch.equal(audio_len, corpus["audio_len"])
    assert torch.equal(text.cpu(), pad_sequence(texts, batch_first=True, padding_value=BLANK_IDX))
    assert text_len.tolist() == [len(t) for t in texts]
    # the module called on the list of paths is the audio half of the collate
    fa, fl = tr(paths)
    assert torch.equal(fa, audio) and torch.equal(fl, audio_len)
    # waveform tensors (host, device) and paths mixed: the same batch
    for items in ([w.cpu() for w in corpus["waves"]], corpus["waves"],
                  [paths[0], corpus["waves"][1].cpu(), paths[2], corpus["waves"][3], paths[4]]):
        (a2, l2), (t2, tl2) = collate(list(zip(items, texts)))
        assert torch.equal(a2, audio) and torch.equal(l2, audio_len) and torch.equal(t2, text) and torch.equal(tl2, text_len)
    torch.manual_seed(0)
    step = TrainStep(AudioToTextCTC(64, 32, 29, 64).to(cuda))
    loss = step(batch)
    assert loss.dim() == 0 and math.isfinite(float(loss))


def test_pipeline_with_lengths_transcribe_and_the_unchanged_chunk_call(corpus, cuda):
    tr, paths = corpus["tr"], corpus["paths"]
    torch.manual_seed(3)
    model = AudioToTextCTC(64, 32, 29, 64).to(cuda).eval()
    pipe = ASRPipeline(model, tr)
    wave_, wave_len = load_batch(paths, SR, cuda)
    with torch.no_grad():
        want_ids, want_n = ctc_greedy_decode(model(corpus["audio"]), model.output_length(corpus["audio_len"]))
    ids, n = pipe(wave_, wave_len)
    assert torch.equal(ids, want_ids) and torch.equal(n, want_n)
    assert all(int(k) <= (int(l) + 1) // 2 for k, l in zip(want_n, corpus["audio_len"]))
    # frame counts with a feature batch and no transform
    ids2, n2 = ASRPipeline(model)(corpus["audio"], corpus["audio_len"])
    assert torch.equal(ids2, want_ids) and torch.equal(n2, want_n)
    assert pipe.transcribe(paths, decode) == [decode(want_ids[b, :int(want_n[b])].cpu()) for b in range(5)]
    with pytest.raises(RuntimeError):
        ASRPipeline(model).transcribe(paths, decode)
    # equal-length chunks, no lengths: the call as it was
    gen = torch.Generator().manual_seed(4)
    chunks = (torch.randn(3, SR, generator=gen) * 0.1).to(cuda)
    with torch.no_grad():
        old_ids, old_n = ctc_greedy_decode(model(tr(chunks)))
    got_ids, got_n = pipe(chunks)
    assert torch.equal(got_ids, old_ids) and torch.equal(got_n, old_n)
