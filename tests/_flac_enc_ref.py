"""Test-side mirror of the FLAC encoder's search (K30), in numpy and Python floats, sharing no code with voice100_amd.  It makes every
choice the device makes -- wasted bits, constant / verbatim / fixed 0-4 / LPC 1..max order, partition order, Rice parameters, stereo
assignment -- by the same exact bit counts and the same tie rules, and hands the choices to tests/_flac_ref.py as Sub / Frame objects,
so the bits themselves are packed by the independent encoder already in the tree.

    encode(pcm [C, N] int, rate, bps, ...) -> Encoded(data, header_len, frames, frame_bytes, bits, fixed_bits, verbatim_bits)

bits / fixed_bits / verbatim_bits: per frame, the subframe bits of the mirror's choice, of the best choice without LPC, and of plain
verbatim subframes.  LPC analysis: exact int64 autocorrelation of (x >> max(0, width - 16)) times the integer Welch window
256 (D^2 - d^2) // D^2 (d = 2 i - (n - 1), D = n + 1); Levinson-Durbin in Python floats (IEEE double, one rounding per operation, the
device's order of operations); shift from the exponent field of the largest coefficient; floor(v + 0.5) with error feedback."""
import math
import struct
from collections import namedtuple

import numpy as np

import _flac_ref as R

Encoded = namedtuple("Encoded", "data header_len frames frame_bytes bits fixed_bits verbatim_bits")
NK = 15


def quantise(wave, bps):
    """clamp(rint(x 2^(bps-1))), ties to even, in float32 as the device computes it; x float32."""
    x = np.asarray(wave, np.float32) * np.float32(1 << (bps - 1))
    return np.clip(np.rint(x), -(1 << (bps - 1)), (1 << (bps - 1)) - 1).astype(np.int64)


def precision(block_size):
    for limit, p in ((192, 7), (384, 8), (576, 9), (1152, 10), (2304, 11)):
        if block_size <= limit:
            return p
    return 12


def _ctz(v):
    return (v & -v).bit_length() - 1


def window(n):
    i = np.arange(n, dtype=np.int64)
    d, D = 2 * i - (n - 1), n + 1
    return (256 * (D * D - d * d)) // (D * D)


def lpc_candidates(xs, w, n, max_order, prec):
    """[(order, coefs, shift)] for orders 1 .. min(max_order, n - 1), skipping what the device drops."""
    maxo = min(max_order, n - 1)
    if maxo < 1:
        return []
    xw = (xs >> max(0, w - 16)) * window(n)
    ac = [int(np.dot(xw[l:], xw[:n - l])) for l in range(maxo + 1)]
    if ac[0] <= 0:
        return []
    out, lpc, err = [], [0.0] * maxo, float(ac[0])
    for m in range(maxo):
        acc = float(ac[m + 1])
        for j in range(m):
            acc = acc - lpc[j] * float(ac[m - j])
        k = acc / err
        lpc[m] = k
        for j in range(m >> 1):
            a, b = lpc[j], lpc[m - 1 - j]
            lpc[j] = a - k * b
            lpc[m - 1 - j] = b - k * a
        if m & 1:
            lpc[m >> 1] = lpc[m >> 1] - lpc[m >> 1] * k
        err = err * (1.0 - k * k)
        cmax = max(abs(v) for v in lpc[:m + 1])
        ef = (struct.unpack("<Q", struct.pack("<d", cmax))[0] >> 52) & 0x7FF
        shift = prec - (ef - 1023) - 2
        if ef not in (0, 0x7FF) and shift >= 0:
            shift = min(shift, 15)
            scale, lo, hi = float(1 << shift), -float(1 << (prec - 1)), float((1 << (prec - 1)) - 1)
            e, q = 0.0, []
            for j in range(m + 1):
                e = e + lpc[j] * scale
                v = min(max(float(math.floor(e + 0.5)), lo), hi)
                e = e - v
                q.append(int(v))
            out.append((m + 1, q, shift))
        if not err > 0.0:
            break
    return out


def _residual_cost(xs, n, order, coefs, shift, pmax):
    """(bits of the residual section, partition order, parameters) or None when a residual leaves (-2^31, 2^31)."""
    pred = np.zeros(n - order, np.int64)
    for j in range(order):
        pred += int(coefs[j]) * xs[order - 1 - j:n - 1 - j]
    res = xs[order:] - (pred >> shift)
    if np.any(res <= -(1 << 31)) or np.any(res >= (1 << 31)):
        return None
    u = np.zeros(n, np.int64)
    u[order:] = (res << 1) ^ (res >> 63)
    sums = np.stack([(u >> k).reshape(1 << pmax, -1).sum(axis=1) for k in range(NK)], axis=1)      # [P, NK]
    best = None
    levels = {}
    for p in range(pmax, -1, -1):
        if p < pmax:
            sums = sums[0::2] + sums[1::2]
        cnt = np.full(1 << p, n >> p, np.int64)
        cnt[0] -= order
        cost = sums + (1 + np.arange(NK, dtype=np.int64))[None, :] * cnt[:, None]
        ks = np.argmin(cost, axis=1)                                  # the first minimum
        levels[p] = (int(cost[np.arange(1 << p), ks].sum()) + 4 * (1 << p), [int(k) for k in ks])
    for p in range(pmax + 1):
        if p == 0 or (n >> p) > order:
            if best is None or levels[p][0] < best[0]:
                best = (levels[p][0], p, levels[p][1])
    return best


def search(x, width, block_size, max_lpc_order, max_partition_order):
    """One signal of one frame -> (bits, Sub, bits without LPC)."""
    x = np.asarray(x, np.int64)
    n = len(x)
    orall = int(np.bitwise_or.reduce(x))
    wasted = _ctz(orall) if orall else 0
    xs, w = x >> wasted, width - wasted
    if np.all(xs == xs[0]):
        best = (8 + wasted + w, R.Sub("constant", wasted=wasted))
    else:
        best = (8 + wasted + w * n, R.Sub("verbatim", wasted=wasted))
    pmax = min(_ctz(n), max_partition_order)
    prec = precision(block_size)
    cands = [("fixed", o, R.FIXED[o], 0) for o in range(5) if o < n]
    fixed_best = None
    cands += [("lpc", o, c, s) for o, c, s in lpc_candidates(xs, w, n, max_lpc_order, prec)]
    for kind, order, coefs, shift in cands:
        if kind == "lpc" and fixed_best is None:
            fixed_best = best[0]
        rc = _residual_cost(xs, n, order, coefs, shift, pmax)
        if rc is None:
            continue
        bits = 8 + wasted + order * w + (9 + order * prec if kind == "lpc" else 0) + 6 + rc[0]
        if bits < best[0]:
            best = (bits, R.Sub(kind, order=order, coefs=list(coefs) if kind == "lpc" else None, precision=prec if kind == "lpc" else None,
                                shift=shift, wasted=wasted, method=0, porder=rc[1], params=rc[2]))
    return best[0], best[1], best[0] if fixed_best is None else fixed_best


def rate_form(rate):
    if rate in R.RATE_CODES:
        return "code"
    if rate < 65536:
        return "hz16"
    if rate % 10 == 0 and rate // 10 < 65536:
        return "tenhz16"
    return "info"


def plan_frame(pcm, bps, block_size, max_lpc_order, max_partition_order):
    """pcm [C, n] -> (Frame, bits, bits without LPC, plain verbatim bits)."""
    pcm = np.asarray(pcm, np.int64)
    C, n = pcm.shape
    if C == 1:
        sigs, widths = [pcm[0]], [bps]
    else:
        sigs, widths = [pcm[0], pcm[1], (pcm[0] + pcm[1]) >> 1, pcm[0] - pcm[1]], [bps, bps, bps, bps + 1]
    found = [search(s, w, block_size, max_lpc_order, max_partition_order) for s, w in zip(sigs, widths)]
    verbatim = C * (8 + bps * n)

    def pick(col):
        if C == 1:
            return None, found[0][col], [0]
        options = [(1, (0, 1)), (8, (0, 3)), (9, (3, 1)), (10, (2, 3))]
        best = None
        for assign, (a, b) in options:
            bits = found[a][col] + found[b][col]
            if best is None or bits < best[1]:
                best = (assign, bits, [a, b])
        return best
    assign, bits, which = pick(0)
    _, fixed_bits, _ = pick(2)
    fr = R.Frame(n, [found[k][1] for k in which], assign=assign, bs_form=None, rate_form="code", size_form="code")
    return fr, bits, fixed_bits, verbatim


def encode(pcm, rate, bps, block_size=4096, max_lpc_order=8, max_partition_order=6, md5=False) -> Encoded:
    pcm = np.asarray(pcm, np.int64)
    if pcm.ndim == 1:
        pcm = pcm[None]
    C, N = pcm.shape
    frames, out, bits, fixed_bits, verbatim_bits = [], [], [], [], []
    for k, at in enumerate(range(0, N, block_size)):
        seg = pcm[:, at:at + block_size]
        fr, b, fb, vb = plan_frame(seg, bps, block_size, max_lpc_order, max_partition_order)
        fr.rate_form = rate_form(rate)
        frames.append(fr)
        bits.append(b)
        fixed_bits.append(fb)
        verbatim_bits.append(vb)
        out.append(R.encode_frame(seg, k, rate, bps, fr))
    sizes = [len(o) for o in out]
    info = R.streaminfo(rate, C, bps, N, block_size, block_size, R.pcm_md5(pcm, bps) if md5 else bytes(16), min(sizes), max(sizes))
    data = R.container(info, b"".join(out))
    return Encoded(data, len(data) - sum(sizes), frames, sizes, bits, fixed_bits, verbatim_bits)


def describe(sub):
    """A subframe's predictor fields on one line, for a mismatch report."""
    return (f"{sub.kind} order={sub.order} wasted={sub.wasted} precision={sub.precision} shift={sub.shift} coefs={sub.coefs} "
            f"porder={sub.porder} params={sub.params}")
