"""The case list of the FLAC encoder's tests (K30), shared by the CPU and the GPU test: integer PCM, built with numpy only.

    cases() -> [Case(name, pcm [C, N] int32, bits, rate, block_size, max_lpc_order, max_partition_order)]

Every item is at most three frames long."""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np

Case = namedtuple("Case", "name pcm bits rate block_size max_lpc_order max_partition_order")


@lru_cache(maxsize=None)
def _resonance(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 0.3, n)
    at = int(rng.integers(0, 80))
    while at < n:
        x[at] += 8.0
        at += int(rng.integers(80, 161))
    y = x.tolist()
    for f, bw in ((500.0, 80.0), (1500.0, 120.0), (2500.0, 160.0)):
        r = math.exp(-math.pi * bw / 16000.0)
        a1, a2 = 2.0 * r * math.cos(2.0 * math.pi * f / 16000.0), -r * r
        y1 = y2 = 0.0
        for i in range(n):
            v = y[i] + a1 * y1 + a2 * y2
            y2, y1 = y1, v
            y[i] = v
    y = np.asarray(y)
    return np.rint(y * (12000.0 / np.abs(y).max())).astype(np.int32)


def resonance(n, seed=0):
    """The resonance fixture: seeded noise of sigma 0.3 plus pulses of 8.0 every 80-160 samples through three two-pole resonators in
    series at 16 kHz (500 Hz / 80 Hz bandwidth, 1500 / 120, 2500 / 160), scaled to a peak of 12,000 and rounded.  [n] int32."""
    return _resonance(n, seed).copy()


def _mono(name, x, bits=16, rate=16000, bs=4096, lpc=8, po=6):
    return Case(name, np.asarray(x, np.int32)[None], bits, rate, bs, lpc, po)


@lru_cache(maxsize=None)
def _cases():
    rng = np.random.default_rng(30)
    out = []
    res = resonance(8193, 0)
    for n in (1, 2, 15, 16, 17, 4095, 4096, 4097, 8193):
        out.append(_mono(f"len{n}", res[100:100 + n] if n < 4000 else res[:n]))
    for bs, n in ((16, 40), (192, 500), (1152, 2500), (4096, 4100)):
        out.append(_mono(f"bs{bs}", res[:n], bs=bs))
    n = 4200
    t = np.arange(n)
    out.append(_mono("zeros", np.zeros(n)))
    out.append(_mono("constant", np.full(n, -1234)))
    out.append(_mono("ramp", (t * 7 - 12000) % 30000 - 15000))
    out.append(_mono("square", np.where((t // 37) % 2, 32767, -32768)))
    out.append(_mono("noise", rng.integers(-32768, 32768, n)))
    out.append(_mono("shifted3", rng.integers(-3000, 3000, n) << 3))
    out.append(_mono("sine", np.rint(20000 * np.sin(t * 0.0371))))
    spike = np.zeros(n)
    spike[3001] = 29999
    out.append(_mono("spike", spike))
    out.append(_mono("resonance", resonance(4200, 1)))
    out.append(_mono("rate44100", res[:300], rate=44100, bs=192))
    out.append(_mono("rate12345", res[:300], rate=12345, bs=256))
    out.append(_mono("rate655350", res[:300], rate=655350, bs=256))
    out.append(_mono("rate100001", res[:300], rate=100001, bs=256))
    out.append(_mono("lpc0", res[:1000], lpc=0, bs=576))
    out.append(_mono("po0", res[:1000], po=0, bs=512))
    a, b = resonance(4200, 2), resonance(4200, 3)
    for name, l, r in (("identical", a, a), ("inverted", a, -a), ("independent", a, b), ("one_silent", a, np.zeros_like(a)),
                       ("near", a, a + rng.integers(-3, 4, 4200))):
        out.append(Case("stereo_" + name, np.stack([l, r]).astype(np.int32), 16, 16000, 4096, 8, 6))
    out.append(Case("stereo_bs192", np.stack([a[:450], b[:450]]).astype(np.int32), 16, 22050, 192, 8, 6))
    n = 1300
    out.append(_mono("w8_noise", rng.integers(-128, 128, n), bits=8, bs=1152))
    out.append(_mono("w8_resonance", res[:n] // 100, bits=8, bs=1152))
    out.append(Case("w8_stereo", np.stack([res[:n] // 100, res[7:n + 7] // 110]).astype(np.int32), 8, 8000, 1152, 8, 6))
    out.append(_mono("w24_noise", rng.integers(-(1 << 23), 1 << 23, n), bits=24, bs=1152, lpc=12))
    big = res[:4200].astype(np.int64) * 690 + rng.integers(-40, 41, 4200)
    out.append(_mono("w24_resonance", big, bits=24, lpc=12))
    out.append(Case("w24_stereo", np.stack([big[:n], -big[:n] + 5]).astype(np.int32), 24, 48000, 1152, 12, 6))
    out.append(_mono("w24_extremes", np.where(t[:n] & 1, (1 << 23) - 1, -(1 << 23)), bits=24, bs=1152, lpc=12))
    return tuple(out)


def cases():
    return list(_cases())
