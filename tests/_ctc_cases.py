"""Cases and float64 reference for the CTC head (K10, csrc/ctc.hip): no GPU, no HIP.

CASES is the list of tests/test_gpu_ctc_oracle.py; test_ctc_cases_cpu.py checks that it reaches what it claims to reach and that the
reference meets closed forms.  Every case is built from a fixed seed: logits = randn * scale, labels by `mode`:
  rand   uniform over the non-blank labels
  norep  no two neighbours equal (every skip transition allowed)
  same   one label repeated (no skip transition allowed)

reference(case) is torch.nn.functional.ctc_loss on the CPU in float64 through log_softmax, per utterance; e32 is the same call's
float32 error against it -- the yardstick of the gradient bar, which therefore never depends on the kernel under test.
regime(case) restates ctc_run's dispatch."""
import functools
from typing import NamedTuple, Tuple

import torch
import torch.nn.functional as F

CTC_CHUNK = 64          # frames of log-probabilities the barrier kernels stage in LDS
LDS_STATIC_MAX = 65536  # above it the launch needs hipFuncAttributeMaxDynamicSharedMemorySize


class Case(NamedTuple):
    name: str
    B: int
    T: int
    V: int
    Lmax: int
    mode: str
    tgt_len: Tuple[int, ...]
    in_len: Tuple[int, ...]
    infeasible: Tuple[int, ...] = ()      # rows declared to have no alignment
    blank: int = 0
    scale: float = 2.0
    seed: int = 0


def _case(seed, name, B, T, V, Lmax, mode, tgt_len, in_len, **kw):
    assert len(tgt_len) == B and len(in_len) == B and max(tgt_len) <= Lmax and max(in_len) <= T
    return Case(name, B, T, V, Lmax, mode, tuple(tgt_len), tuple(in_len), seed=seed, **kw)


CASES = [
    # all 16 waves of the skew kernel live (S = 1023, 961); lengths 1 : 511 in one batch
    _case(1, "skew16_full", 4, 640, 29, 511, "rand", (511, 480, 1, 0), (640, 600, 640, 37)),
    # 15 idle waves; in_len 1 and 8: shorter than one prefetch group
    _case(2, "skew16_idle", 4, 40, 29, 511, "rand", (1, 3, 20, 0), (1, 8, 40, 1)),
    _case(3, "edge_31", 2, 100, 29, 31, "norep", (31, 30), (100, 64)),                      # Smax 63: one wave
    # Smax 65: wave 1 holds one state; in_len round the 16 / 32-frame ring marks; row 0 (in_len = L) has a single alignment
    _case(4, "edge_32_ring", 8, 64, 29, 32, "norep", (32,) * 8, (32, 33, 40, 47, 48, 49, 63, 64)),
    _case(5, "edge_512", 2, 700, 29, 512, "rand", (512, 300), (700, 560)),                  # Smax 1025: <8>, one state in slot 4
    _case(6, "edge_1023", 2, 1200, 71, 1023, "rand", (1023, 513), (1200, 1100)),            # <8> full
    _case(7, "edge_1024", 2, 1200, 29, 1024, "rand", (1024, 2), (1200, 1111)),              # Smax 2049: <16>; lengths 1 : 512
    _case(8, "max_2047_v128", 1, 2100, 128, 2047, "norep", (2047,), (2100,)),               # <16> full; LDS above 64 KiB
    _case(9, "max_2046_v128", 2, 2100, 128, 2046, "rand", (2046, 1500), (2100, 2000)),      # the other Smax above 64 KiB
    _case(10, "max_2047_v29", 1, 2100, 29, 2047, "norep", (2047,), (2100,)),                # the same kernel under 64 KiB
    # no skip transition anywhere; row 0 (in_len = 2 L - 1) has a single alignment
    _case(11, "same_label", 3, 120, 5, 40, "same", (40, 40, 17), (79, 120, 120)),
    _case(12, "two_classes", 2, 90, 2, 30, "same", (30, 11), (59, 90)),
    _case(13, "blank_last", 3, 70, 29, 12, "rand", (12, 7, 0), (70, 33, 5), blank=28),
    _case(14, "peaky", 3, 300, 29, 100, "rand", (100, 64, 5), (300, 250, 299), scale=10.0),
    _case(15, "flat", 3, 300, 29, 100, "rand", (100, 64, 5), (300, 250, 299), scale=0.1),
    # row 1 has fewer frames than labels: no alignment.  Row 2 has no frame and no label: the empty alignment, probability 1,
    # nll 0 (torch's answer, and decode.ctc_segment's log_prob 0 for such a row).  Row 4: an empty target over 64 frames.
    _case(16, "infeasible_mix", 5, 64, 29, 20, "rand", (20, 20, 0, 5, 0), (64, 19, 0, 64, 64), infeasible=(1,)),
]
BY_NAME = {c.name: c for c in CASES}
# rows whose lattice has exactly one path: (case, row)
SINGLE_ALIGNMENT = (("edge_32_ring", 0), ("same_label", 0))


@functools.lru_cache(maxsize=None)
def inputs(case):
    """logits [B, T, V] float32 and labels [B, Lmax] int64 (valid labels in the padding too)."""
    g = torch.Generator().manual_seed(4100 + case.seed)
    logits = torch.randn(case.B, case.T, case.V, generator=g) * case.scale
    n = case.V - 1                                                   # non-blank labels, as ranks 0 .. n-1
    if case.mode == "rand":
        rank = torch.randint(0, n, (case.B, case.Lmax), generator=g)
    elif case.mode == "norep":
        step = torch.randint(1, n, (case.B, case.Lmax), generator=g)  # 1 .. n-1: never back onto the neighbour
        rank = torch.cumsum(step, 1) % n
    elif case.mode == "same":
        rank = torch.randint(0, n, (case.B, 1), generator=g).expand(case.B, case.Lmax).contiguous()
    else:
        raise ValueError(case.mode)
    labels = rank + (rank >= case.blank).long()                      # skip over the blank
    assert int(labels.min()) >= 0 and int(labels.max()) < case.V and not bool((labels == case.blank).any())
    return logits, labels


class Reference(NamedTuple):
    nll64: torch.Tensor       # [B] float64, inf where infeasible
    G64: torch.Tensor         # [B, T, V] float64: d nll_b / d logits[b]; zero on infeasible rows and padded frames
    mean64: float             # reduction='mean', zero_infinity=True
    e32: torch.Tensor         # [B] float64: max |G32[b] - G64[b]|, G32 the same call in float32


def _unscaled_gradient(case, dtype):
    """d nll_b / d logits[b] for every b at once: the utterances do not interact, so it is the gradient of sum_b nll_b
    (zero_infinity: an infeasible row contributes a zero loss and a zero gradient)."""
    logits, labels = inputs(case)
    x = logits.to(dtype, copy=True).requires_grad_(True)
    F.ctc_loss(F.log_softmax(x.transpose(0, 1), dim=-1), labels, torch.tensor(case.in_len), torch.tensor(case.tgt_len),
               blank=case.blank, reduction="none", zero_infinity=True).sum().backward()
    return x.grad


@functools.lru_cache(maxsize=None)
def reference(case):
    logits, labels = inputs(case)
    il, tl = torch.tensor(case.in_len), torch.tensor(case.tgt_len)
    with torch.no_grad():
        lp = F.log_softmax(logits.double().transpose(0, 1), dim=-1)
        nll64 = F.ctc_loss(lp, labels, il, tl, blank=case.blank, reduction="none", zero_infinity=False)
        mean64 = float(F.ctc_loss(lp, labels, il, tl, blank=case.blank, reduction="mean", zero_infinity=True))
    G64 = _unscaled_gradient(case, torch.float64)
    e32 = (_unscaled_gradient(case, torch.float32).double() - G64).abs().flatten(1).amax(1)
    return Reference(nll64, G64, mean64, e32)


def random_walk_term(case, ref):
    """sqrt(in_len) * max(1, |nll|) * 2^-24: in_len roundings of values of size |nll|, as a random walk."""
    nll = torch.where(torch.isfinite(ref.nll64), ref.nll64.abs(), torch.zeros_like(ref.nll64)).clamp_min(1.0)
    return torch.tensor(case.in_len, dtype=torch.float64).sqrt() * nll * 2.0 ** -24


def grad_bar(case, ref):
    """Per utterance: max(2e-4, 2 e32, random-walk term).  The entries of G lie in [-1, 1]."""
    return torch.maximum(torch.full_like(ref.e32, 2e-4), torch.maximum(2 * ref.e32, random_walk_term(case, ref)))


def regime(case):
    """ctc_run's dispatch: which lattice kernel runs, how wide, and per utterance the highest wave (skew kernel: 64 states a wave) or
    slot (barrier kernels: state s sits in slot s // 256) that carries a state; None for a row without frames."""
    Smax = 2 * case.Lmax + 1
    S = [2 * L + 1 for L in case.tgt_len]
    if Smax <= 1024:
        out = {"kernel": "skew", "waves": (Smax + 63) // 64, "lds_bytes": None, "unit": 64}
    else:
        out = {"kernel": "lattice8" if Smax <= 2048 else "lattice16", "waves": 4,
               "lds_bytes": (CTC_CHUNK * case.V + 2 * (Smax + 4)) * 4, "unit": 256}
    out["Smax"] = Smax
    out["live"] = [(s - 1) // out["unit"] if n > 0 else None for s, n in zip(S, case.in_len)]
    out["lds_attribute"] = out["lds_bytes"] is not None and out["lds_bytes"] > LDS_STATIC_MAX
    return out


def single_alignment_path(case, row):
    """The only path of a SINGLE_ALIGNMENT row: the labels themselves (in_len = L, no repeats) or labels with a blank between
    each pair (in_len = 2 L - 1, all labels equal)."""
    _, labels = inputs(case)
    L, n = case.tgt_len[row], case.in_len[row]
    lab = labels[row, :L].tolist()
    if n == L:
        assert all(a != b for a, b in zip(lab, lab[1:]))
        return lab
    assert n == 2 * L - 1 and all(a == b for a, b in zip(lab, lab[1:]))
    path = [case.blank] * n
    path[0::2] = lab
    return path


def workspace_floats(case):
    """alpha + beta + lse + stall flags (v100_ctc_workspace_floats); the largest is max_2046_v128's, 138 MB."""
    return 2 * case.B * case.T * (2 * case.Lmax + 1) + case.B * case.T + case.B
