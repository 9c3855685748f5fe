"""The WORLD feature statistics of a data set -- the `audio_stat.pt` that `--audio_stat` / `audio_stat=` loads into `WORLDNorm` --
accumulated on the GPU (csrc/world_stat.hip).

The reference's `voice100/calc_stat.py` masks by multiplication and rounds every product and per-batch sum to fp32 before its
double accumulator.  Here one `update` is two launches that add a padded batch's exact products, in float64, into the raw
moments; frames beyond an utterance's length are never read; the spectral and aperiodicity widths are general.  The state
dict has the reference's six keys, dtypes, shapes and formulae (codeap divided by the FRAME count, as there).
"""
import torch

from . import _native as N

__all__ = ["WORLDStat", "calc_stat"]

MAX_LOGSPC_SIZE, MAX_CODEAP_SIZE = 1024, 8


class WORLDStat:
    """Running raw moments of (f0, logspc or mcep, codeap) batches.

    `moments` is a float64 tensor of 4 + 2S + 2A entries on `device`, zero at first:
    [0] sum f0, [1] sum f0^2, [2] count, over valid frames with f0 > 30;  [3] valid frames;  [4:4+S] sum logspc and
    [4+S:4+2S] sum logspc^2 per column over valid frames;  then A sums of codeap and A of codeap^2 per band over valid
    elements with codeap < -0.2.  Raw moments of shards add: `a.moments += b.moments`, or an all-reduce of `moments`."""

    def __init__(self, logspc_size: int, codeap_size: int = 1, device=None) -> None:
        if not 1 <= int(logspc_size) <= MAX_LOGSPC_SIZE or not 1 <= int(codeap_size) <= MAX_CODEAP_SIZE:
            raise ValueError(f"WORLDStat: logspc_size must be in [1, {MAX_LOGSPC_SIZE}] and codeap_size in [1, {MAX_CODEAP_SIZE}] "
                             f"(got {logspc_size}, {codeap_size})")
        self.logspc_size, self.codeap_size = int(logspc_size), int(codeap_size)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        self.moments = torch.zeros(4 + 2 * self.logspc_size + 2 * self.codeap_size, dtype=torch.float64, device=self.device)
        self._partial = {}

    def _arg(self, x, name, shape):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise ValueError(f"WORLDStat.update: {name} must be a float32 tensor")
        if tuple(x.shape) != shape:
            raise ValueError(f"WORLDStat.update: {name} must be {list(shape)}, got {list(x.shape)}")
        return x

    @torch.no_grad()
    def update(self, f0, f0_len, logspc, codeap) -> None:
        """Add one padded batch: f0 [B, T], f0_len [B] (any integer dtype), logspc [B, T, S], codeap [B, T, A]; frame (b, t)
        counts iff t < f0_len[b].  Two launches, no host synchronisation.  CPU tensors are moved to the device; lengths given
        on the CPU must lie in [0, T] (ValueError), lengths on the device are clamped to it by the kernel."""
        if not isinstance(f0, torch.Tensor) or f0.dim() != 2:
            raise ValueError("WORLDStat.update: f0 must be [B, T]")
        B, T = f0.shape
        S, A = self.logspc_size, self.codeap_size
        f0 = self._arg(f0, "f0", (B, T))
        logspc = self._arg(logspc, "logspc", (B, T, S))
        codeap = self._arg(codeap, "codeap", (B, T, A))
        lens = torch.as_tensor(f0_len)
        if tuple(lens.shape) != (B,) or lens.dtype.is_floating_point or lens.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise ValueError(f"WORLDStat.update: f0_len must be [{B}] integers, got {list(lens.shape)} {lens.dtype}")
        if not lens.is_cuda and B and (int(lens.min()) < 0 or int(lens.max()) > T):
            raise ValueError(f"WORLDStat.update: f0_len must lie in [0, {T}]")
        if self.device.type != "cuda":                           # after the argument checks, which need no device
            raise RuntimeError("WORLDStat.update runs on the GPU only (no CPU fallback)")
        if B == 0 or T == 0:
            return
        f0, logspc, codeap = (x.to(self.device).contiguous() for x in (f0, logspc, codeap))
        if lens.is_cuda and lens.dtype != torch.int32:
            lens = lens.clamp(0, T)                              # before narrowing: an int64 beyond 2^31 must not wrap
        lens = lens.to(self.device, torch.int32).contiguous()
        partial = self._partial.get((B, T))
        if partial is None:
            parts = N.helper("v100_world_stat_parts", B, T, S)
            partial = self._partial[(B, T)] = torch.empty(parts * self.moments.numel(), dtype=torch.float64, device=self.device)
        if not self.moments.is_contiguous() or self.moments.device != self.device or self.moments.dtype != torch.float64:
            raise RuntimeError("WORLDStat.moments must stay a contiguous float64 tensor on the stat's device")
        with torch.cuda.device(self.device):
            N.call("v100_world_stat_accum", f0, lens, logspc, codeap, partial, self.moments, B, T, S, A)

    def state_dict(self):
        """The six tensors `voice100/calc_stat.py` saves: float64 on the CPU, f0_* [1], logspc_* [S], codeap_* [A];
        mean = sum / count, std = sqrt(sqrsum / count - mean^2).  codeap is divided by the number of valid FRAMES, not of
        its own elements (the reference's `codeap_count = logspc_count`).  A zero count gives NaN."""
        S, A = self.logspc_size, self.codeap_size
        m = self.moments.detach().to("cpu", torch.float64)
        f0_count, frames = m[2:3], m[3:4]
        out = {}
        for name, s, q, n in (("f0", m[0:1], m[1:2], f0_count), ("logspc", m[4:4 + S], m[4 + S:4 + 2 * S], frames),
                              ("codeap", m[4 + 2 * S:4 + 2 * S + A], m[4 + 2 * S + A:4 + 2 * S + 2 * A], frames)):
            mean = s / n
            out[name + "_mean"] = mean
            out[name + "_std"] = torch.sqrt(q / n - mean ** 2)
        return out


def calc_stat(data, output_path):
    """`voice100.calc_stat.calc_stat`: the statistics of every batch of `data.predict_dataloader()` -- batches
    ((f0, f0_len, logspc, codeap), (text, text_len)) -- saved to `output_path` with torch.save and returned.  The feature
    widths come from `data.audio_transform.vocoder.output_dims`."""
    f0_dim, logspc_size, codeap_size = data.audio_transform.vocoder.output_dims
    if f0_dim != 1:
        raise ValueError(f"calc_stat: the vocoder's f0 width must be 1 (got {f0_dim})")
    stat = WORLDStat(logspc_size, codeap_size)
    for batch in data.predict_dataloader():
        (f0, f0_len, logspc, codeap), _ = batch
        stat.update(f0, f0_len, logspc, codeap)
    state_dict = stat.state_dict()
    torch.save(state_dict, output_path)
    return state_dict
