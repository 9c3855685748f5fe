"""Float64 restatement of the WORLD statistics step (include/voice100_hip.h, K19) in CPU torch, written from the layout table and
the arithmetic rules, not from the kernel: frames are SELECTED by the length (nothing beyond it is read into a sum), products and
sums are float64, and the two thresholds are compared in float32.

moments_ref(batches, S, A) -> (moments, mag, terms), three float64 vectors of 4 + 2S + 2A entries: the raw moments of all the
batches, sum |term| per entry, and the number of terms per entry.  Two float64 summations of the same n terms in different
orders differ by at most 2 (n - 1) u sum |term| to first order (each is within (n - 1) u sum |term| of the exact sum, u = 2^-53),
which `bound` rounds up to 2 n u sum |term|.
"""
import numpy as np
import torch

U = 2.0 ** -53


def moments_ref(batches, S, A):
    W = 4 + 2 * S + 2 * A
    mom = torch.zeros(W, dtype=torch.float64)
    mag = torch.zeros(W, dtype=torch.float64)
    terms = torch.zeros(W, dtype=torch.float64)

    def put(at, cols, values):
        """values: float64 [n, cols], one row per selected element of a column (cols > 1: every column selects all rows)"""
        mom[at:at + cols] += values.sum(0)
        mag[at:at + cols] += values.abs().sum(0)
        terms[at:at + cols] += values.shape[0]

    for f0, f0_len, logspc, codeap in batches:
        f0, logspc, codeap = (torch.as_tensor(x).detach().cpu() for x in (f0, logspc, codeap))
        assert f0.dtype == logspc.dtype == codeap.dtype == torch.float32
        B, T = f0.shape
        assert logspc.shape == (B, T, S) and codeap.shape == (B, T, A)
        for b in range(B):
            n = min(max(int(f0_len[b]), 0), T)
            if n == 0:
                continue
            f = f0[b, :n]
            f = f[f > 30.0].double()                              # fp32 tensor against a Python scalar: compared in fp32
            put(0, 1, f[:, None])
            put(1, 1, (f * f)[:, None])
            mom[2] += f.numel()
            mom[3] += n
            ls = logspc[b, :n].double()
            put(4, S, ls)
            put(4 + S, S, ls * ls)
            for a in range(A):
                c = codeap[b, :n, a]
                c = c[c < -0.2].double()
                put(4 + 2 * S + a, 1, c[:, None])
                put(4 + 2 * S + A + a, 1, (c * c)[:, None])
    return mom, mag, terms


def bound(mag, terms):
    return 2.0 * terms * U * mag


def stats_ref(mom, S, A):
    """The six tensors of the state dict from raw moments, float64 (codeap over the FRAME count)."""
    m = mom.double()
    out = {}
    for name, s, q, n in (("f0", m[0:1], m[1:2], m[2]), ("logspc", m[4:4 + S], m[4 + S:4 + 2 * S], m[3]),
                          ("codeap", m[4 + 2 * S:4 + 2 * S + A], m[4 + 2 * S + A:], m[3])):
        out[name + "_mean"] = s / n
        out[name + "_std"] = torch.sqrt(q / n - (s / n) ** 2)
    return out


def spread(mom, S, A):
    """E[x^2] / var per statistic (the factor by which a relative error of the raw moments grows in a std), largest per key"""
    m = mom.double()
    out = {}
    for name, s, q, n in (("f0", m[0:1], m[1:2], m[2]), ("logspc", m[4:4 + S], m[4 + S:4 + 2 * S], m[3]),
                          ("codeap", m[4 + 2 * S:4 + 2 * S + A], m[4 + 2 * S + A:], m[3])):
        ex2 = q / n
        out[name] = float((ex2 / (ex2 - (s / n) ** 2)).max())
    return out


def make_batch(B, T, S, A, seed, lens=None):
    """A seeded batch in the shape of real features: f0 zero on ~40 % of frames, else 80-280; logspc ~ N(-8, 2); codeap either
    below -0.2 or about zero; zero padding beyond the lengths (one row full)."""
    g = torch.Generator().manual_seed(seed)
    if lens is None:
        lens = torch.randint(1, T + 1, (B,), generator=g)
        lens[int(torch.randint(0, B, (1,), generator=g))] = T
    lens = torch.as_tensor(lens, dtype=torch.int64)
    voiced = torch.rand(B, T, generator=g) >= 0.4
    f0 = torch.where(voiced, 80.0 + 200.0 * torch.rand(B, T, generator=g), torch.zeros(())).float()
    logspc = (torch.randn(B, T, S, generator=g) * 2.0 - 8.0).float()
    low = torch.rand(B, T, A, generator=g) < 0.6
    codeap = torch.where(low, -0.3 - 20.0 * torch.rand(B, T, A, generator=g), -1e-3 * torch.rand(B, T, A, generator=g)).float()
    mask = torch.arange(T)[None, :] < lens[:, None]
    return f0 * mask, lens, logspc * mask[:, :, None], codeap * mask[:, :, None]


def as_numpy(d):
    return {k: np.asarray(v) for k, v in d.items()}
