"""Inputs shared by the resumable beam search's tests (K32): tests/test_beam_stream_cpu.py and tests/test_gpu_beam_stream.py.

planted() gives logits with a clear best path -- runs of 1 to 3 frames of one label, then 1 to 5 frames of blank, each raised by `peak`
over unit noise -- so that the forking oracles of tests/_beam_ref.py and tests/_beam_lm_ref.py decide a case of thousands of frames
with one leaf.  LONG is the case past ctc_beam_search's 4096 frames: both rows are the same planted logits, of lengths 4200 and 4097;
the plain oracle ends both with one leaf, whose best scores are LONG_SCORES (tests/test_beam_stream_cpu.py pins them, so the fixture
cannot drift).  peak 6 rather than 12 keeps |score| large enough that accept()'s tolerance of 1e-4 |score| stays above the kernel's
documented ~1e-6 per frame.  LM_CASE is the fused oracle's: 700 frames at peak 12 with the order-3 fit model at (0.5, 0.3) are decided
with one leaf (at 4200 frames the LM oracle forks into more than 32 leaves: its relative near-tie window grows with |key|)."""
import functools

import numpy as np

from _beam_ref import SHAPES, beam_search_fork, seeded_logits

LONG = dict(T=4200, V=8, seed=1, peak=6.0, W=4, lengths=(4200, 4097))
LONG_SCORES = (-178.06, -173.56)
LM_CASE = dict(T=700, V=8, seed=1, peak=12.0, W=4, alpha=0.5, beta=0.3, chunk=256)
# the shapes of the chunked-equals-one-call tests, out of _beam_ref.SHAPES
CHUNK_SHAPES = [(24, 8, 4), (33, 29, 8), (64, 29, 16), (16, 128, 64), (12, 3, 64), (40, 2, 8), (1, 29, 8), (2, 29, 8), (300, 8, 4)]


def planted(T, V, seed, peak):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, V)).astype(np.float32)
    t = 0
    while t < T:
        c = int(rng.integers(1, V)); d = int(rng.integers(1, 4)); g = int(rng.integers(1, 6))
        x[t:t+d, c] += peak; x[t+d:t+d+g, 0] += peak
        t += d + g
    return x


def shape_logits(T, V, W):
    """_beam_ref's seeded logits [cases, T, V] of one of its shapes, and ragged lengths that include 0 and T."""
    scale, _, cases = next(s[3:] for s in SHAPES if s[:3] == (T, V, W))
    x = seeded_logits(T, V, W, scale, cases)
    rng = np.random.default_rng(T + V + W)
    lengths = rng.integers(0, T + 1, cases)
    lengths[0], lengths[-1] = T, 0                       # (one case: 0)
    return x, [int(n) for n in lengths]


def chunks_of(T):
    """The chunk sizes of the chunked-equals-one-call tests: {1, 7, T - 1, T, 4096}, those that are a chunk size at all."""
    return sorted({c for c in (1, 7, T - 1, T, 4096) if c >= 1})


@functools.lru_cache(maxsize=None)
def long_leaves():
    """The plain forking oracle on LONG's two rows: [leaves of row 0, leaves of row 1]."""
    x = planted(LONG["T"], LONG["V"], LONG["seed"], LONG["peak"])
    return [beam_search_fork(x[:n], LONG["W"]) for n in LONG["lengths"]]
