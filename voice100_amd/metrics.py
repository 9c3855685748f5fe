"""Objective scores of synthesised WORLD features, counted on the device (K27, csrc/dtw.hip).

The standard measures for a WORLD-feature synthesiser -- mel-cepstral distortion (MCD), F0 RMSE and the voiced/unvoiced error
rate -- compare a predicted track with a recording's frame by frame, after a time alignment: the align model predicts its own
durations, so the two never have the same number of frames.  The alignment is dynamic time warping on the mel-cepstral distance.

  dtw_score       one call: the DTW of every pair of a batch, and the sums along each warping path
  mcd_db          (10 / ln 10) sqrt(2) cost / pairs: the mean distance per path pair in dB
  SynthesisScore  a running meter shaped like infer.ErrorRate: update() adds a batch into a device tensor without a read-back
"""
import math
from typing import NamedTuple, Optional

import torch

from . import _native as N

__all__ = ["DTWScore", "dtw_score", "mcd_db", "SynthesisScore"]

T_MAX, DU_MAX = 4096, 64


class DTWScore(NamedTuple):
    cost: torch.Tensor                       # [B] float64: the cumulative distance along the path
    path_len: torch.Tensor                   # [B] int32: pairs on the path
    voiced: Optional[torch.Tensor]           # [B] int32: pairs with both frames voiced (None without f0 inputs, like the next three)
    vuv_errors: Optional[torch.Tensor]       # [B] int32: pairs with exactly one frame voiced
    f0_sq_cents: Optional[torch.Tensor]      # [B] float64: sum of (1200 log2(f0x / f0y))^2 over the voiced pairs
    f0_sq_hz: Optional[torch.Tensor]         # [B] float64: sum of (f0x - f0y)^2 over the voiced pairs
    path: Optional[torch.Tensor]             # [B, Tx + Ty - 1, 2] int32 (frame of x, frame of y), zero beyond path_len; None unless asked


def dtw_score(x: torch.Tensor, x_len, y: torch.Tensor, y_len, f0x=None, f0y=None, skip: int = 0, f0_floor: float = 30.0,
              dtw: bool = True, totals=None, per_row: bool = True, return_path: bool = False):
    """Time-align every hypothesis x [B, Tx, D] with its reference y [B, Ty, D] and sum along the path (K27, csrc/dtw.hip).

    x_len / y_len: [B] frames per row, or None for the full width; clamped to [0, width] on the device, and nothing beyond a row's
    length is read.  The local distance is the Euclidean distance over the dimensions skip .. D-1 (MCD leaves out c0: skip=1).
    dtw=True: C(i,j) = d(i,j) + min(C(i-1,j-1), C(i-1,j), C(i,j-1)), a tie to the first of the three; the path is the backtrace.
    dtw=False: frame i against frame i, for i < min(n, m).  A pair with an empty side gives zeros.
    f0x [B, Tx] / f0y [B, Ty] in Hz go together; a frame is voiced iff f0 >= f0_floor (30.0 is the reference's own hasf0 rule).
    totals: a float64 GPU tensor of 6 elements INTO which the call adds the batch sums {pairs, cost, voiced, vuv_errors, f0_sq_cents,
    f0_sq_hz}; no read-back.  per_row=False (with totals): only the totals are computed, and None is returned.
    Distances are fp32 from differences; the cumulative cost and the f0 sums are fp64.
    Limits: B >= 1, 1 <= Tx, Ty <= 4096, 0 <= skip < D, D - skip <= 64.  Returns a DTWScore."""
    name = "dtw_score"
    tensors = [t for t in (x, x_len, y, y_len, f0x, f0y, totals) if t is not None]
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
        raise RuntimeError(f"{name}: GPU tensors only")
    if x.dim() != 3 or y.dim() != 3 or x.shape[0] != y.shape[0] or x.shape[2] != y.shape[2] or x.shape[0] < 1:
        raise RuntimeError(f"{name}: x [B, Tx, D] and y [B, Ty, D] with the same B >= 1 and D, got {list(x.shape)} and {list(y.shape)}")
    if (f0x is None) != (f0y is None):
        raise RuntimeError(f"{name}: f0x and f0y go together")
    if not per_row and totals is None:
        raise RuntimeError(f"{name}: nothing to compute (per_row=False and no totals)")
    if not per_row and return_path:
        raise RuntimeError(f"{name}: return_path needs per_row=True")
    if totals is not None and (totals.dtype != torch.float64 or totals.numel() != 6 or not totals.is_contiguous()):
        raise RuntimeError(f"{name}: totals must be a contiguous float64 tensor of 6 elements")
    dev = x.device
    B, Tx, D = x.shape
    Ty, skip = y.shape[1], int(skip)
    nbytes = N.helper("v100_dtw_workspace_bytes", B, Tx, Ty, D, int(bool(return_path))) if Tx >= 1 and Ty >= 1 and D >= 1 else -1
    if nbytes <= 0 or not 0 <= skip < D or D - skip > DU_MAX:
        raise RuntimeError(f"{name}: unsupported shape (1 <= Tx = {Tx} <= {T_MAX}, 1 <= Ty = {Ty} <= {T_MAX}, 0 <= skip = {skip} < D = {D} "
                           f"and D - skip <= {DU_MAX} are the limits)")
    x, y = x.to(torch.float32).contiguous(), y.to(device=dev, dtype=torch.float32).contiguous()

    def lens(t):
        if t is None:
            return None
        t = t.to(device=dev, dtype=torch.int32).contiguous()
        if t.numel() != B:
            raise RuntimeError(f"{name}: x_len and y_len must have {B} elements")
        return t
    xl, yl = lens(x_len), lens(y_len)
    if f0x is not None:
        if tuple(f0x.shape) != (B, Tx) or tuple(f0y.shape) != (B, Ty):
            raise RuntimeError(f"{name}: f0x must be [{B}, {Tx}] and f0y [{B}, {Ty}], got {list(f0x.shape)} and {list(f0y.shape)}")
        f0x, f0y = f0x.to(torch.float32).contiguous(), f0y.to(device=dev, dtype=torch.float32).contiguous()
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    if per_row:
        Bp = (B + 3) & ~3                                                    # every row of the two blocks starts 16-byte aligned
        f64 = torch.empty((3, Bp), dtype=torch.float64, device=dev)          # cost, f0_sq_cents, f0_sq_hz
        i32 = torch.empty((3, Bp), dtype=torch.int32, device=dev)            # path_len, voiced, vuv_errors
        out = [f64[0, :B], i32[0, :B], i32[1, :B], i32[2, :B], f64[1, :B], f64[2, :B]]
    else:
        out = [None] * 6
    path = torch.empty((B, Tx + Ty - 1, 2), dtype=torch.int32, device=dev) if return_path else None
    N.call("v100_dtw_score", x, xl, y, yl, f0x, f0y, ws, *out, path, totals, B, Tx, Ty, D, skip, float(f0_floor), 0 if dtw else 1)
    if not per_row:
        return None
    if f0x is None:
        out[2:] = [None] * 4
    return DTWScore(out[0], out[1], out[2], out[3], out[4], out[5], path)


def mcd_db(cost, pairs):
    """Mel-cepstral distortion in dB from a path's cumulative distance and its number of pairs: (10 / ln 10) sqrt(2) cost / pairs;
    nan at pairs == 0.  Tensors in, a float64 tensor out; numbers in, a float out."""
    k = 10.0 / math.log(10.0) * math.sqrt(2.0)
    if isinstance(cost, torch.Tensor) or isinstance(pairs, torch.Tensor):
        cost = torch.as_tensor(cost).to(torch.float64)
        pairs = torch.as_tensor(pairs, device=cost.device).to(torch.float64)
        return torch.where(pairs > 0, k * cost / pairs, torch.full_like(cost, float("nan")))
    return k * cost / pairs if pairs > 0 else float("nan")


class SynthesisScore:
    """Running MCD, F0 RMSE and voiced/unvoiced error rate of an evaluation loop, summed on the device (dtw_score, K27).

    update(f0, feat, frames, ref_f0, ref_feat, ref_frames) scores one batch -- f0 [B, T] Hz, feat [B, T, mcep_dim + 1] mel-cepstra,
    frames [B] valid frames per row, and the same for the reference -- and adds the batch sums into a float64 device tensor: no
    device-to-host synchronisation.  Features that arrive as a log-spectrum [B, T, n_fft/2 + 1] are first taken to mel-cepstra with
    create_sp2mc_matrix(n_fft, mcep_dim, alpha) of the vocoder's rate, on the exact-fp32 GEMM path; that needs a `vocoder`, whose own
    use_mcep setting does not matter.  c0 is left out of the distance (skip=1).
    compute() does the one read-back and returns {"mcd" (dB), "f0_rmse_cents", "f0_rmse_hz", "vuv_error", "frames" (path pairs),
    "voiced_frames", "utterances"}; a rate is nan where its denominator is 0.  reset() zeroes the totals.
    dtw=False pairs frame i with frame i instead of warping."""

    def __init__(self, vocoder=None, f0_floor: float = 30.0, dtw: bool = True):
        self.vocoder, self.f0_floor, self.dtw = vocoder, float(f0_floor), bool(dtw)
        self.totals = None                               # float64 [6]: pairs, cost, voiced, vuv_errors, f0_sq_cents, f0_sq_hz
        self.utterances = 0
        self._sp2mc_t = None

    def reset(self):
        if self.totals is not None:
            self.totals.zero_()
        self.utterances = 0

    def to_mcep(self, feat: torch.Tensor) -> torch.Tensor:
        """feat [B, T, C]: mel-cepstra as they are; a log-spectrum of the vocoder's n_fft/2 + 1 bins through sp2mc."""
        v = self.vocoder
        if feat.dim() != 3:
            raise RuntimeError(f"SynthesisScore: features must be [B, T, C], got {list(feat.shape)}")
        if v is None or feat.shape[2] != v.n_fft // 2 + 1:
            if feat.shape[2] - 1 > DU_MAX:
                raise RuntimeError(f"SynthesisScore: {feat.shape[2]} feature dimensions are no mel-cepstrum (at most {DU_MAX + 1}); "
                                   "a log-spectrum needs the vocoder whose n_fft/2 + 1 bins it has")
            return feat
        if self._sp2mc_t is None or self._sp2mc_t.device != feat.device:
            import numpy as np
            from .vocoder import create_sp2mc_matrix
            m = create_sp2mc_matrix(v.n_fft, v.mcep_dim, v.mcep_alpha)
            self._sp2mc_t = torch.from_numpy(np.ascontiguousarray(m.T).astype(np.float32)).to(feat.device)
        B, T, C = feat.shape
        return v._frames_matmul(feat.reshape(B * T, C).float(), self._sp2mc_t).reshape(B, T, -1)

    @torch.no_grad()
    def update(self, f0, feat, frames, ref_f0, ref_feat, ref_frames, per_row: bool = False, return_path: bool = False):
        if not (feat.is_cuda and ref_feat.is_cuda):
            raise RuntimeError("SynthesisScore.update: GPU tensors only")
        if self.totals is None:
            self.totals = torch.zeros(6, dtype=torch.float64, device=feat.device)
        elif self.totals.device != feat.device:
            raise RuntimeError("SynthesisScore.update: the totals live on another device")
        out = dtw_score(self.to_mcep(feat), frames, self.to_mcep(ref_feat), ref_frames, f0, ref_f0, skip=1, f0_floor=self.f0_floor,
                        dtw=self.dtw, totals=self.totals, per_row=per_row, return_path=return_path)
        self.utterances += feat.shape[0]
        return out

    def compute(self):
        t = self.totals.cpu().tolist() if self.totals is not None else [0.0] * 6
        pairs, cost, voiced, vuv, cents, hz = t
        nan = float("nan")
        return {"mcd": mcd_db(cost, pairs), "f0_rmse_cents": math.sqrt(cents / voiced) if voiced > 0 else nan,
                "f0_rmse_hz": math.sqrt(hz / voiced) if voiced > 0 else nan, "vuv_error": vuv / pairs if pairs > 0 else nan,
                "frames": int(pairs), "voiced_frames": int(voiced), "utterances": self.utterances}
