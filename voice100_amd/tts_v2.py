"""TextToAlignText and AlignTextToAudio: the v2 TTS models (voice100/models/_align_v2.py, _tts_v2.py; config/align_*_base.yaml,
config/tts_*_base.yaml), drop-in.

Same constructors, state_dict keys (`embedding.*`, `lstm.*`, `dense.*` / `decoder.*`, `projection.*`, `norm.*`), forward() /
predict() contracts and LightningModule hooks.  The embedding is functional.embedding_bct, the 2-layer bidirectional LSTM is
voice100_amd.lstm.LSTM (K15) in its channel-major form, the TTS decoder is layers_v2 (K1 GEMMs + the fused LayerNorm / GELU),
`dense` / `projection` are K1 GEMMs, and the losses are one HIP pass each with their gradient: the v2 WORLDLoss (K16) and the
align model's masked L1 loss (K17).  predict's epilogue is v100_world_unnormalize_v2 and align() is v100_align_expand_v2.  The
packed-sequence round trip of the reference is the LSTM's padded form with lengths: the same numbers, padded positions exactly
0, which is what the reference's decoder sees after pad_packed_sequence.  While a graph is traced the modules run stock ops.
"""
from argparse import ArgumentParser
from typing import List, Optional, Tuple

import torch
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from . import _stock
from . import functional as F_
from ._base import Voice100ModelBase, tracing
from .layers_v2 import get_conv_layers
from .lstm import LSTM
from .tts import WORLDNorm

__all__ = ["TextToAlignText", "AlignTextToAudio", "WORLDLoss", "WORLDNorm", "align_v2"]


def align_v2(text: torch.Tensor, align: torch.Tensor, head: int = 5, tail: int = 5) -> torch.Tensor:
    """The v2 expansion of one utterance (_align_v2.py:48-73) on the host: text [L], align [L, 2] -> aligntext [n] (text's dtype).
    Same integer rules as v100_align_expand_v2, whose fp64 index-order sum it also uses; a last span that ends past the length
    lengthens the row (the reference raises IndexError there)."""
    text, al = text.cpu(), align.detach().cpu().to(torch.float64).tolist()
    total = 0.0
    for g, n in al:
        total += g
        total += n
    if al:
        total -= al[0][0]
    spans, t, u = [], float(head), 0
    for i, (g, n) in enumerate(al):
        if i > 0:
            t += g
        s = max(int(t), u)
        u = s + 1
        t += n
        e = max(int(t), u)
        u = e
        spans.append((s, e))
    out = torch.zeros(max(head + int(total) + tail, u), dtype=text.dtype)
    for i, (s, e) in enumerate(spans):
        out[s:e] = text[i]
    return out


class TextToAlignText(Voice100ModelBase):
    """text [B, L] int64, text_len [B] -> (pred [B, max(text_len), 2] = log(gap + 1), log(len + 1), lengths)."""

    def __init__(self, vocab_size, num_layers, hidden_size, num_outputs, learning_rate) -> None:
        super().__init__()
        self.save_hyperparameters()
        assert num_outputs == 2
        self.embedding = nn.Embedding(vocab_size, hidden_size)
        self.lstm = LSTM(input_size=hidden_size, hidden_size=hidden_size, num_layers=num_layers, dropout=0.2, bidirectional=True,
                         batch_first=True)
        self.dense = nn.Linear(hidden_size * 2, num_outputs)

    def _forward_btc(self, text: torch.Tensor, text_len: torch.Tensor):
        t_out = int(text_len.max())                                      # what pad_packed_sequence returns: one host read
        if t_out < text.shape[1]:
            text = text[:, :t_out]
        x = F_.embedding_bct(text.contiguous(), self.embedding.weight)  # [B, H, T]
        y, _, _ = self.lstm.forward_bct(x, text_len)                     # [B, 2H, T], 0 beyond each length
        return F_.transpose_last2(F_.pointwise_conv1d(y, self.dense.weight, self.dense.bias))   # [B, T, 2]

    def forward(self, text: torch.Tensor, text_len: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if tracing():
            embed = torch.nn.functional.embedding(text, self.embedding.weight)
            packed = pack_padded_sequence(embed, text_len.cpu(), batch_first=True, enforce_sorted=False)
            out, _ = self.lstm(packed)
            out, out_len = pad_packed_sequence(out, batch_first=True)
            return self.dense(out), out_len
        return self._forward_btc(text, text_len), text_len

    def predict(self, text: torch.Tensor, text_len: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(exp(pred) - 1, lengths): the predicted (gap, length) per token, unclamped (a gap can be in (-1, 0))."""
        align, align_len = self.forward(text, text_len)
        return torch.exp(align) - 1, align_len

    def align(self, text: torch.Tensor, align: torch.Tensor, head=5, tail=5) -> torch.Tensor:
        """One utterance: text [L], align [L, 2] -> aligntext [n] (_align_v2.py:48-73); on the device for CUDA tensors."""
        assert text.dim() == 1
        assert align.dim() == 2
        if text.is_cuda:
            out, _ = self.align_batch(text[None], align[None], None, head, tail)
            return out[0].to(text.dtype)
        return align_v2(text, align, head, tail)

    @staticmethod
    def align_batch(text: torch.Tensor, align: torch.Tensor, text_len: Optional[torch.Tensor] = None, head=5, tail=5):
        """align() for a batch on the device: text [B, L], align [B, L, 2], text_len [B] -> (aligntext [B, max n] int64 zero padded,
        n [B] int32), what align() per utterance followed by pad_sequence(batch_first=True) gives (update_samples.py:58-67)."""
        from .decode import align_expand_v2
        return align_expand_v2(text, align, text_len, head, tail)

    def _calc_batch_loss(self, batch) -> torch.Tensor:
        (text, text_len), (align, align_len) = batch
        pred = self._forward_btc(text, text_len)
        # align[:, :-1].reshape(B, -1, 2), log(align + 1), |.-pred| averaged over the pair, masked mean over text_len: one kernel (K17)
        return F_.align_loss(pred, align, text_len)

    def training_step(self, batch, batch_idx=0):
        loss = self._calc_batch_loss(batch)
        self.log("train_loss", loss)
        return loss

    def validation_step(self, batch, batch_idx=0):
        loss = self._calc_batch_loss(batch)
        self.log("val_loss", loss)
        return {"val_loss": loss}

    def test_step(self, batch, batch_idx=0):
        loss = self._calc_batch_loss(batch)
        self.log("test_loss", loss)
        return {"test_loss": loss}

    def configure_optimizers(self):
        """Plain Adam (_align_v2.py:90-93): one fused launch for the whole model on the GPU (csrc/adam.hip)."""
        params = list(self.parameters())
        if all(p.is_cuda for p in params):
            from .optim import FusedAdam
            return FusedAdam(params, lr=self.hparams.learning_rate)
        return torch.optim.Adam(params, lr=self.hparams.learning_rate)

    @staticmethod
    def add_model_specific_args(parent_parser):
        parser = ArgumentParser(parents=[parent_parser], add_help=False)
        parser.add_argument("--num_layers", type=int, default=2)
        parser.add_argument("--hidden_size", type=int, default=512)
        parser.add_argument("--num_outputs", type=int, default=2)
        parser.add_argument("--learning_rate", type=float, default=1e-3)
        return parser

    @staticmethod
    def from_argparse_args(args, **kwargs):
        return TextToAlignText(hidden_size=args.hidden_size, learning_rate=args.learning_rate, **kwargs)


class WORLDLoss(nn.Module):
    """The v2 WORLDLoss (_layers_v2.py:116-163) fused with AlignTextToAudio's target preparation (_tts_v2.py:98-101) in K16.

    forward(length, pred, f0, logspc, codeap, norm) takes the projection output pred [B, Tp, 2+S+2Cap] and the RAW targets
    f0 [B, Tt], logspc [B, Tt, S], codeap [B, Tt, Cap] with the WORLDNorm module, and returns the five terms as a [5] tensor
    (hasf0, f0, logspc, hascodeap, codeap).  No parameters, as in the reference."""

    def __init__(self, loss: str = "mse") -> None:
        super().__init__()
        if loss not in ("l1", "mse"):
            raise ValueError("Unknown loss type")
        self.loss = loss

    def forward(self, length, pred, f0, logspc, codeap, norm) -> torch.Tensor:
        nv = (norm.f0_mean, norm.f0_std, norm.logspc_mean, norm.logspc_std, norm.codeap_mean, norm.codeap_std)
        return F_.world_loss_v2(pred, length, f0, logspc, codeap, nv, self.loss)


class AlignTextToAudio(Voice100ModelBase):
    """aligntext [B, L] int64, aligntext_len [B] -> (hasf0_logits [B, T], f0_hat [B, T], logspc_hat [B, T, S],
    hascodeap_logits [B, T, Cap], codeap_hat [B, T, Cap]), T = 2 max(aligntext_len) - 1."""

    def __init__(self, vocab_size: int, logspc_size: int, codeap_size: int, encoder_num_layers: int, encoder_hidden_size: int,
                 decoder_settings: List[List], logspc_weight: float = 5.0, learning_rate: float = 1e-3, f0_size: int = 1,
                 audio_stat: Optional[str] = None) -> None:
        super().__init__()
        self.save_hyperparameters()
        if f0_size != 1:
            raise NotImplementedError("AlignTextToAudio: f0_size = 1 only (the reference's recipes)")
        self.encoder_hidden_size = encoder_hidden_size
        self.vocab_size = vocab_size
        self.f0_size = f0_size
        self.logspc_size = logspc_size
        self.codeap_size = codeap_size
        self.audio_size = 2 * self.f0_size + self.logspc_size + 2 * self.codeap_size
        self.embedding = nn.Embedding(vocab_size, encoder_hidden_size)
        self.lstm = LSTM(input_size=encoder_hidden_size, hidden_size=encoder_hidden_size, num_layers=encoder_num_layers, dropout=0.2,
                         bidirectional=True)
        self.decoder = get_conv_layers(2 * encoder_hidden_size, decoder_settings)
        self.projection = nn.Linear(decoder_settings[-1][0], self.audio_size)
        self.norm = WORLDNorm(self.logspc_size, self.codeap_size)
        self.criterion = WORLDLoss()
        self.logspc_weight = logspc_weight
        # the total's weights over the five terms, kept on the model's device (not part of the state_dict)
        self.register_buffer("_term_weights", torch.tensor([1.0, 1.0, float(logspc_weight), 1.0, 1.0]), persistent=False)
        if audio_stat is not None:
            self.norm.load_state_dict(torch.load(audio_stat))

    def _sizes(self):
        return [self.f0_size, self.f0_size, self.logspc_size, self.codeap_size, self.codeap_size]

    def _project(self, aligntext: torch.Tensor, aligntext_len: torch.Tensor) -> torch.Tensor:
        """The projection output [B, 2T - 1, 2+S+2Cap], T = max(aligntext_len)."""
        if tracing():
            x = _stock.embedding_bct(aligntext, self.embedding.weight)
            packed = pack_padded_sequence(torch.transpose(x, 1, 2), aligntext_len.cpu(), batch_first=True, enforce_sorted=False)
            out, _ = self.lstm(packed)
            out, _ = pad_packed_sequence(out, batch_first=True)
            x = torch.transpose(self.decoder(torch.transpose(out, -2, -1)), -2, -1)
            return self.projection(x)
        t_out = int(aligntext_len.max())                                 # what pad_packed_sequence returns: one host read
        if t_out < aligntext.shape[1]:
            aligntext = aligntext[:, :t_out]
        x = F_.embedding_bct(aligntext.contiguous(), self.embedding.weight)   # [B, H, T]
        y, _, _ = self.lstm.forward_bct(x, aligntext_len)                # [B, 2H, T], 0 beyond each length
        y = self.decoder(y)                                              # [B, C, 2T - 1]
        return F_.transpose_last2(F_.pointwise_conv1d(y, self.projection.weight, self.projection.bias))

    def forward(self, aligntext: torch.Tensor, aligntext_len: torch.Tensor
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        x = self._project(aligntext, aligntext_len)
        hasf0_logits, f0_hat, logspc_hat, hascodeap_logits, codeap_hat = torch.split(x, self._sizes(), dim=2)
        return hasf0_logits[:, :, 0], f0_hat[:, :, 0], logspc_hat, hascodeap_logits, codeap_hat

    def predict(self, aligntext: torch.Tensor, aligntext_len: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(f0, logspc, codeap) un-normalised; f0 is 0 where the hasf0 logit < 0, codeap where its hascodeap logit < 0."""
        x = self._project(aligntext, aligntext_len)
        n = self.norm
        if tracing():
            hasf0, f0, logspc, hascodeap, codeap = torch.split(x, self._sizes(), dim=2)
            hasf0, f0 = hasf0[:, :, 0], f0[:, :, 0]
            f0, logspc, codeap = n.unnormalize(f0, logspc, codeap)
            f0 = torch.where(hasf0 < 0, torch.zeros(size=(1,), dtype=f0.dtype, device=f0.device), f0)
            codeap = torch.where(hascodeap < 0, torch.zeros(size=(1, 1), dtype=codeap.dtype, device=codeap.device), codeap)
            return f0, logspc, codeap
        return F_.world_unnormalize_gate_v2(x, n.f0_mean, n.f0_std, n.logspc_mean, n.logspc_std, n.codeap_mean, n.codeap_std)

    def _loss_terms(self, batch) -> torch.Tensor:
        (f0, f0_len, logspc, codeap), (aligntext, aligntext_len) = batch
        # hasf0 = f0 >= 30, hascodeap = codeap < -0.2, WORLDNorm.normalize, adjust_size, the mask, the five terms and d/dpred:
        # everything after the projection is one kernel (K16)
        return self.criterion(f0_len, self._project(aligntext, aligntext_len), f0, logspc, codeap, self.norm)

    def _calc_batch_loss(self, batch) -> Tuple[torch.Tensor, ...]:
        return tuple(self._loss_terms(batch).unbind(0))

    def _step(self, task: str, batch) -> torch.Tensor:
        terms = self._loss_terms(batch)
        loss = torch.dot(terms, self._term_weights)   # hasf0 + f0 + logspc_weight * logspc + hascodeap + codeap
        self.log(f"{task}_loss", loss)
        for name, v in zip(("hasf0", "f0", "logspc", "hascodeap", "codeap"), terms.detach().unbind(0)):
            self.log(f"{task}_{name}_loss", v)
        return loss

    def training_step(self, batch, batch_idx=0) -> torch.Tensor:
        return self._step("train", batch)

    def validation_step(self, batch, batch_idx=0):
        return {"val_loss": self._step("val", batch)}

    def test_step(self, batch, batch_idx=0):
        return {"test_loss": self._step("test", batch)}

    def configure_optimizers(self):
        """Plain Adam (_tts_v2.py:137-140) over the trained parameters: one fused launch on the GPU (csrc/adam.hip)."""
        params = [p for p in self.parameters() if p.requires_grad]
        if all(p.is_cuda for p in params):
            from .optim import FusedAdam
            return FusedAdam(params, lr=self.hparams.learning_rate)
        return torch.optim.Adam(params, lr=self.hparams.learning_rate)

    @staticmethod
    def add_model_specific_args(parent_parser):
        parser = ArgumentParser(parents=[parent_parser], add_help=False)
        parser.add_argument("--model_size", choices=["base"], default="base")
        parser.add_argument("--audio_stat", type=str)
        parser.add_argument("--learning_rate", type=float, default=1e-3)
        return parser

    @staticmethod
    def from_argparse_args(args, **kwargs):
        if args.model_size == "base":
            # out_channels, transpose, kernel_size, stride, padding, bias (config/tts_en_base.yaml:20-23)
            decoder_settings = [[512, False, 5, 1, 2, False], [512, True, 5, 2, 2, False], [512, False, 5, 1, 2, False]]
            encoder_num_layers, encoder_hidden_size = 2, 512
        else:
            raise ValueError("Unknown model_size")
        use_mcep = args.vocoder == "world_mcep"
        model = AlignTextToAudio(encoder_num_layers=encoder_num_layers, encoder_hidden_size=encoder_hidden_size,
                                 decoder_settings=decoder_settings, logspc_size=25 if use_mcep else 257, codeap_size=1,
                                 learning_rate=args.learning_rate, **kwargs)
        if not args.resume_from_checkpoint:
            if args.audio_stat is None:
                args.audio_stat = f"./data/{args.dataset}-stat.pt"
            model.norm.load_state_dict(torch.load(args.audio_stat))
        return model
