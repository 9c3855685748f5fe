"""`LSTM`: a drop-in for torch.nn.LSTM as the reference's v2 models use it (_asr_v2.py:32-34, 46), on the HIP recurrence (K15).

Parameter names, shapes, registration order and initialisation are nn.LSTM's (`weight_ih_l{k}[_reverse]`, `weight_hh_...`,
`bias_ih_...`, `bias_hh_...`; uniform(-1/sqrt(H), 1/sqrt(H)) in registration order), so a reference checkpoint loads with
strict=True and the same seed draws the same weights.  Each layer is one functional.LSTMLayerFn; dropout between layers runs
in training mode through functional.dropout.  The precision is functional.get_matmul_precision(): fp32, or bf16 operands with
fp32 accumulate and fp32 cell state; fp16 is inference only.  GPU only: on the CPU the first kernel call raises RuntimeError.
While a graph is being traced (torch.jit.trace / torch.onnx.export) the forward is the stock aten LSTM (_stock.lstm).
"""
import math
from typing import Optional

import torch
from torch import nn
from torch.nn.utils.rnn import PackedSequence, pack_padded_sequence, pad_packed_sequence

from . import _stock
from . import functional as F_
from ._base import tracing

__all__ = ["LSTM"]


class LSTM(nn.Module):
    """nn.LSTM(input_size, hidden_size, num_layers, bias, batch_first, dropout, bidirectional) without proj_size or a given (h0, c0).

    forward(PackedSequence)                -> (PackedSequence, (h_n, c_n)) as nn.LSTM returns them;
    forward(padded, lengths=...)           -> (padded output, zero beyond each length, (h_n, c_n)); padded is [T, B, C]
                                              ([B, T, C] with batch_first), lengths [B] (CPU or device);
    forward_bct(x [B, C, T], lengths)      -> (y [B, D H, T], h_n, c_n): the channel-major form the v2 models chain into their
                                              convolutions without a transpose."""

    def __init__(self, input_size: int, hidden_size: int, num_layers: int = 1, bias: bool = True, batch_first: bool = False,
                 dropout: float = 0.0, bidirectional: bool = False, proj_size: int = 0, device=None, dtype=None):
        super().__init__()
        if proj_size:
            raise NotImplementedError("LSTM: proj_size is not supported")
        if dtype not in (None, torch.float32):
            raise NotImplementedError("LSTM: float32 parameters only")
        if not 0.0 <= float(dropout) <= 1.0:
            raise ValueError("dropout should be a number in range [0, 1]")
        if hidden_size % 16 or not 16 <= hidden_size <= 1024:
            raise NotImplementedError("LSTM: hidden_size must be a multiple of 16 in [16, 1024]")
        self.input_size, self.hidden_size, self.num_layers = int(input_size), int(hidden_size), int(num_layers)
        self.bias, self.batch_first, self.dropout, self.bidirectional = bool(bias), bool(batch_first), float(dropout), bool(bidirectional)
        self.proj_size = 0
        ndir = 2 if bidirectional else 1
        H = self.hidden_size
        for layer in range(self.num_layers):
            cin = self.input_size if layer == 0 else H * ndir
            for d in range(ndir):
                sfx = f"_l{layer}" + ("_reverse" if d else "")
                self.register_parameter("weight_ih" + sfx, nn.Parameter(torch.empty(4 * H, cin, device=device)))
                self.register_parameter("weight_hh" + sfx, nn.Parameter(torch.empty(4 * H, H, device=device)))
                if self.bias:
                    self.register_parameter("bias_ih" + sfx, nn.Parameter(torch.empty(4 * H, device=device)))
                    self.register_parameter("bias_hh" + sfx, nn.Parameter(torch.empty(4 * H, device=device)))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        stdv = 1.0 / math.sqrt(self.hidden_size)
        for w in self.parameters():
            nn.init.uniform_(w, -stdv, stdv)

    def extra_repr(self) -> str:
        return (f"{self.input_size}, {self.hidden_size}, num_layers={self.num_layers}, bias={self.bias}, "
                f"batch_first={self.batch_first}, dropout={self.dropout}, bidirectional={self.bidirectional}")

    def layer_params(self, layer: int):
        out = []
        for d in range(2 if self.bidirectional else 1):
            sfx = f"_l{layer}" + ("_reverse" if d else "")
            out += [getattr(self, "weight_ih" + sfx), getattr(self, "weight_hh" + sfx),
                    getattr(self, "bias_ih" + sfx, None), getattr(self, "bias_hh" + sfx, None)]
        return out

    def forward_bct(self, x: torch.Tensor, lengths: torch.Tensor):
        lens = lengths.to(device=x.device, dtype=torch.int32).contiguous()
        hs, cs = [], []
        for layer in range(self.num_layers):
            if layer:
                x = F_.dropout(x, self.dropout, self.training)
            x, h, c = F_.lstm_layer(x, lens, self.layer_params(layer), layer=layer)
            hs.append(h)
            cs.append(c)
        return x, torch.cat(hs, 0), torch.cat(cs, 0)

    def forward(self, input, hx=None, lengths: Optional[torch.Tensor] = None):
        if hx is not None:
            raise NotImplementedError("LSTM: a given (h0, c0) is not supported; the state starts at zero")
        if tracing():
            return _stock.lstm(self, input, lengths)
        if isinstance(input, PackedSequence):
            padded, lens = pad_packed_sequence(input, batch_first=True)           # original batch order, CPU lengths
            y, h, c = self.forward_bct(F_.transpose_last2(padded.contiguous()), lens)
            out = pack_padded_sequence(F_.transpose_last2(y), lens, batch_first=True, enforce_sorted=False)
            return out, (h, c)
        if lengths is None:
            raise NotImplementedError("LSTM: give a PackedSequence or a padded tensor with lengths=")
        x = input if self.batch_first else input.transpose(0, 1)                  # [B, T, C]
        T = x.shape[1]
        if not lengths.is_cuda and (int(lengths.min()) < 1 or int(lengths.max()) > T):
            raise ValueError(f"LSTM: lengths must lie in [1, {T}]")
        y, h, c = self.forward_bct(F_.transpose_last2(x.contiguous()), lengths)
        out = F_.transpose_last2(y)                                               # [B, T, D H]
        return (out if self.batch_first else out.transpose(0, 1)), (h, c)
