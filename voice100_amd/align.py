"""AudioAlignCTC: the v1 aligner (voice100/models/align.py:69-180; export_onnx_v1.export_onnx_align), drop-in.

Same constructor, state_dict keys (`conv.*`, `lstm.*`, `dense.*`), forward() contract and LightningModule hooks.  `conv` is an
nn.Conv1d holder (k = 3, stride 2, padding 1) run through functional.conv1d_dense (im2col + the K1 GEMM), the 2-layer
bidirectional LSTM is voice100_amd.lstm.LSTM (K15), `dense` is a K1 GEMM, the loss is the fused log_softmax + CTC kernel
(zero_infinity semantics) and ctc_best_path runs on the one-launch alignment kernel (K20, decode.ctc_align).  The packed-sequence
round trip of the reference is the LSTM's padded form with lengths: the same numbers, padded positions exactly 0 before `dense`.
fp32 and bf16 train (trainer.TrainStep); fp16 is an eval precision.  GPU only: on the CPU the first kernel call raises
RuntimeError; while a graph is traced (torch.jit.trace / torch.onnx.export) the forward is the stock-op restatement.
"""
from typing import Tuple

import torch
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from . import functional as F_
from ._base import Voice100ModelBase, tracing
from .audio import BatchSpectrogramAugumentation
from .lstm import LSTM

__all__ = ["AudioAlignCTC"]


class AudioAlignCTC(Voice100ModelBase):
    """audio [B, T, audio_size] fp32, audio_len [B] -> (logits [T_out, B, vocab_size], lengths [B]), T_out = max((audio_len + 1) // 2)."""

    def __init__(self, audio_size, vocab_size, hidden_size, num_layers, learning_rate):
        super().__init__()
        self.save_hyperparameters()
        self.conv = nn.Conv1d(audio_size, hidden_size, kernel_size=3, stride=2, padding=1)     # parameter holder: conv1d_dense runs it
        self.relu = nn.ReLU()
        self.lstm = LSTM(input_size=hidden_size, hidden_size=hidden_size, num_layers=num_layers, dropout=0.2, bidirectional=True)
        self.dense = nn.Linear(hidden_size * 2, vocab_size)
        self.criterion = nn.CTCLoss(zero_infinity=True)      # kept for API parity; the step uses functional.ctc_loss
        self.batch_augment = BatchSpectrogramAugumentation()

    def _forward_btv(self, audio: torch.Tensor, audio_len: torch.Tensor):
        x = F_.conv1d_dense(F_.transpose_last2(audio), self.conv.weight, self.conv.bias, stride=2, padding=1)      # [B, H, (T + 1) // 2]
        x = torch.relu(x)
        x_len = torch.div(audio_len + 1, 2, rounding_mode="trunc")
        t_out = int(x_len.max())                                         # what pad_packed_sequence returns: one host sync
        if t_out < x.shape[2]:
            x = x[:, :, :t_out].contiguous()
        y, _, _ = self.lstm.forward_bct(x, x_len)                        # [B, 2H, T_out], 0 beyond each length
        logits = F_.pointwise_conv1d(y, self.dense.weight, self.dense.bias)
        return F_.transpose_last2(logits), x_len                         # [B, T_out, V]

    def forward(self, audio: torch.Tensor, audio_len: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if tracing():
            x = self.relu(self.conv(torch.transpose(audio, 1, 2)))
            x_len = torch.div(audio_len + 1, 2, rounding_mode="trunc")
            packed = pack_padded_sequence(torch.transpose(x, 1, 2), x_len.cpu(), batch_first=True, enforce_sorted=False)
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
        """Plain Adam (align.py:127-131): one fused launch for the whole model on the GPU (csrc/adam.hip)."""
        params = list(self.parameters())
        if all(p.is_cuda for p in params):
            from .optim import FusedAdam
            return FusedAdam(params, lr=self.hparams.learning_rate)
        return torch.optim.Adam(params, lr=self.hparams.learning_rate)

    @torch.no_grad()
    def ctc_best_path(self, audio: torch.Tensor = None, audio_len: torch.Tensor = None, text: torch.Tensor = None,
                      text_len: torch.Tensor = None, logits: torch.Tensor = None):
        """align.py:133-164 on the one-launch alignment kernel: (score, hist, path, logits_len), or the argmax [T, B] without text.
        hist [B, T_out] int32 are the best path's positions in the blank-extended label sequence, path [B, T_out] the labels there,
        both zero beyond each utterance.  `score` keeps the reference's quirk (align.py:161): it is NOT the scores but the last
        utterance's label path as float32 -- kept for drop-in compatibility; infer.AlignPipeline returns the per-utterance scores."""
        from .decode import ctc_align
        if logits is None:
            logits, logits_len = self.forward(audio, audio_len)
            logits = torch.log_softmax(logits, dim=-1)
        else:
            logits_len = audio_len
        if text is None:
            return logits.argmax(axis=-1)
        dev = logits.device
        logits_len = logits_len.to(dev)
        text_len = torch.minimum(logits_len, text_len.to(dev))           # for very short audio
        lp = logits.transpose(0, 1).contiguous()                         # [B, T, V]
        _, hist, path, _ = ctc_align(lp, text.to(dev), logits_len, text_len)
        t_out = int(logits_len.max())
        hist, path = hist[:, :t_out], path[:, :t_out]
        last = int(logits_len[-1])
        score = path[-1, :last].to(torch.float32)
        return score, hist, path, logits_len

    @staticmethod
    def add_model_specific_args(parent_parser):
        parser = parent_parser.add_argument_group("voice100.models.align.AudioAlignCTC")
        parser.add_argument('--hidden_size', type=int, default=128)
        parser.add_argument('--num_layers', type=int, default=2)
        parser.add_argument('--learning_rate', type=float, default=0.001)
        return parent_parser

    @staticmethod
    def from_argparse_args(args, **kwargs):
        return AudioAlignCTC(hidden_size=args.hidden_size, num_layers=args.num_layers, learning_rate=args.learning_rate, **kwargs)
