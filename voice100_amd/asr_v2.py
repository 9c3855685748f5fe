"""AudioToAlignText: the v2 ASR model (voice100/models/_asr_v2.py:18-86; config/asr_en_base.yaml), drop-in.

Same constructor, state_dict keys (`encoder.*`, `lstm.*`, `dense.*`), forward() contract and LightningModule hooks.  The v2 conv
front-end is layers_v2 (K1 GEMMs + the fused LayerNorm / GELU), the 2-layer bidirectional LSTM is voice100_amd.lstm.LSTM (K15),
`dense` is a K1 GEMM, and the loss is the fused log_softmax + CTC kernel (zero_infinity semantics).  The packed-sequence round
trip of the reference (pack_padded_sequence -> nn.LSTM -> pad_packed_sequence) is the LSTM's padded form with lengths: the same
numbers, padded positions exactly 0 before `dense`.
"""
from typing import List, Tuple

import torch
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from . import functional as F_
from ._base import Voice100ModelBase, tracing
from .audio import BatchSpectrogramAugumentation
from .layers_v2 import get_conv_layers
from .lstm import LSTM

__all__ = ["AudioToAlignText"]


class AudioToAlignText(Voice100ModelBase):
    """audio [B, T, audio_size] fp32, audio_len [B] -> (logits [T_out, B, vocab_size], lengths [B]), T_out = max((audio_len + 1) // 2)."""

    def __init__(self, audio_size: int, encoder_settings: List[List], decoder_num_layers: int, decoder_hidden_size: int,
                 vocab_size: int, learning_rate: float = 0.001) -> None:
        super().__init__()
        self.save_hyperparameters()
        self.encoder = get_conv_layers(audio_size, encoder_settings)
        self.lstm = LSTM(input_size=decoder_hidden_size, hidden_size=decoder_hidden_size, num_layers=decoder_num_layers,
                         dropout=0.2, bidirectional=True)
        self.dense = nn.Linear(decoder_hidden_size * 2, vocab_size)
        self.criterion = nn.CTCLoss(zero_infinity=True)      # kept for API parity; the step uses functional.ctc_loss
        self.batch_augment = BatchSpectrogramAugumentation()

    def _forward_btv(self, audio: torch.Tensor, audio_len: torch.Tensor):
        x = self.encoder(F_.transpose_last2(audio))                      # [B, C, T']
        x_len = torch.div(audio_len + 1, 2, rounding_mode="trunc")
        t_out = int(x_len.max())                                         # what pad_packed_sequence returns: one host sync
        if t_out < x.shape[2]:
            x = x[:, :, :t_out].contiguous()
        y, _, _ = self.lstm.forward_bct(x, x_len)                        # [B, 2H, T_out], 0 beyond each length
        logits = F_.pointwise_conv1d(y, self.dense.weight, self.dense.bias)
        return F_.transpose_last2(logits), x_len                         # [B, T_out, V]

    def forward(self, audio: torch.Tensor, audio_len: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if tracing():
            x = self.encoder(torch.transpose(audio, -2, -1))
            x_len = torch.div(audio_len + 1, 2, rounding_mode="trunc")
            packed = pack_padded_sequence(torch.transpose(x, -2, -1), x_len.cpu(), batch_first=True, enforce_sorted=False)
            out, _ = self.lstm(packed)
            out, out_len = pad_packed_sequence(out, batch_first=False)
            return self.dense(out), out_len
        logits, x_len = self._forward_btv(audio, audio_len)
        return logits.transpose(0, 1), x_len

    def _calc_batch_loss(self, batch):
        (audio, audio_len), (text, text_len) = batch
        if self.training:
            audio, audio_len = self.batch_augment(audio, audio_len)
        logits, logits_len = self._forward_btv(audio, audio_len)
        # log_softmax + CTCLoss(blank=0, mean, zero_infinity=True) in the fused lattice kernels (K10)
        return F_.ctc_loss(logits, text, logits_len, text_len, blank=0)

    def training_step(self, batch, batch_idx=0):
        loss = self._calc_batch_loss(batch)
        self.log_dict({"train_loss": loss})
        return loss

    def validation_step(self, batch, batch_idx=0):
        metrics = {"val_loss": self._calc_batch_loss(batch)}
        self.log_dict(metrics)
        return metrics

    def test_step(self, batch, batch_idx=0):
        metrics = {"test_loss": self._calc_batch_loss(batch)}
        self.log_dict(metrics)
        return metrics

    def configure_optimizers(self):
        """Plain Adam (_asr_v2.py:75-79): one fused launch for the whole model on the GPU (csrc/adam.hip)."""
        params = list(self.parameters())
        if all(p.is_cuda for p in params):
            from .optim import FusedAdam
            return FusedAdam(params, lr=self.hparams.learning_rate)
        return torch.optim.Adam(params, lr=self.hparams.learning_rate)

    @torch.no_grad()
    def ctc_best_path(self, audio: torch.Tensor = None, audio_len: torch.Tensor = None, text: torch.Tensor = None,
                      text_len: torch.Tensor = None, logits: torch.Tensor = None):
        """_asr_v2.py:81-116 on the device best-path kernel: (score, hist, path, logits_len), or the argmax [T, B] without text.
        hist [B, T_out] int32 are the best path's positions in the blank-extended label sequence, path [B, T_out] the labels there,
        both zero beyond each utterance.  `score` keeps the reference's quirk (_asr_v2.py:116): it is NOT the scores but the last
        utterance's label path as float32 -- kept for drop-in compatibility; the per-utterance scores are not returned."""
        from .decode import ctc_best_path as _best_path
        if logits is None:
            logits, logits_len = self.forward(audio, audio_len)
            logits = torch.log_softmax(logits, dim=-1)
        else:
            logits_len = audio_len
        if text is None:
            return logits.argmax(axis=-1)
        dev = logits.device
        logits_len = logits_len.to(dev)
        text_len = torch.minimum(logits_len, text_len.to(dev))
        lp = logits.transpose(0, 1).contiguous()                         # [B, T, V]
        _, pos, labels = _best_path(lp, text.to(dev), logits_len, text_len)
        t_out = int(logits_len.max())
        valid = torch.arange(lp.shape[1], device=dev)[None, :] < logits_len[:, None].long()
        hist = torch.where(valid, pos, torch.zeros_like(pos))[:, :t_out]
        path = torch.where(valid, labels, torch.zeros_like(labels))[:, :t_out]
        last = int(logits_len[-1])
        score = path[-1, :last].to(torch.float32)
        return score, hist, path, logits_len
