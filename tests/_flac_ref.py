"""Test-side FLAC oracle, written from the format description and sharing no code with voice100_amd.audio_io: a reference decoder in
plain Python, and an encoder that takes every choice explicitly (it searches for nothing) and computes the residuals from the PCM so
that decoding returns the PCM exactly.  Bits are packed with numpy.

    decode(data) -> Decoded(pcm [C, N] int32, sample_rate, bits_per_sample, md5_ok)
    encode(pcm, rate, bps, frames, ...) -> bytes          frames: a list of Frame, each with one Sub per channel
"""
import hashlib
from collections import namedtuple

import numpy as np

Decoded = namedtuple("Decoded", "pcm sample_rate bits_per_sample md5_ok")

BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
SIZE_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}
FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


# ---- checksums ----------------------------------------------------------------------------------------------------------------
def _crc_table(poly, width):
    top, mask = 1 << (width - 1), (1 << width) - 1
    tab = []
    for x in range(256):
        c = x << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        tab.append(c)
    return tab


_T8, _T16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def crc8(data) -> int:
    c = 0
    for b in data:
        c = _T8[c ^ b]
    return c


def _crc16_slow(data, c=0) -> int:
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


_BLK = 64
_POS = None          # [_BLK][256]: the CRC of byte x followed by k zero bytes
_ADV = None          # the CRC register advanced by _BLK zero bytes, as two byte tables


def _crc16_tables():
    global _POS, _ADV
    pos = np.zeros((_BLK, 256), np.uint16)
    pos[0] = _T16
    t16 = np.array(_T16, np.uint16)
    for k in range(1, _BLK):
        pos[k] = (pos[k - 1] << 8) ^ t16[pos[k - 1] >> 8]
    hi = np.array([_crc16_slow(bytes(_BLK), x << 8) for x in range(256)], np.uint16)
    lo = np.array([_crc16_slow(bytes(_BLK), x) for x in range(256)], np.uint16)
    _POS, _ADV = pos, (hi, lo)


def crc16(data) -> int:
    """CRC-16 (0x8005, initial value 0): by blocks of 64 bytes in numpy -- leading zero bytes do not change a CRC that starts at 0."""
    if len(data) < 4 * _BLK:
        return _crc16_slow(data)
    if _POS is None:
        _crc16_tables()
    a = np.frombuffer(bytes(data), np.uint8)
    pad = -len(a) % _BLK
    a = np.concatenate([np.zeros(pad, np.uint8), a]).reshape(-1, _BLK)
    blk = np.bitwise_xor.reduce(_POS[np.arange(_BLK - 1, -1, -1)[None, :], a], axis=1)
    hi, lo = _ADV
    c = 0
    for b in blk.tolist():
        c = int(hi[c >> 8]) ^ int(lo[c & 0xFF]) ^ b
    return c


def pcm_md5(pcm, bps) -> bytes:
    """MD5 of the interleaved little-endian samples at whole bytes per sample."""
    nb = (bps + 7) // 8
    inter = np.ascontiguousarray(np.asarray(pcm, np.int64).T).reshape(-1)
    raw = np.zeros((inter.size, nb), np.uint8)
    for k in range(nb):
        raw[:, k] = (inter >> (8 * k)) & 0xFF
    return hashlib.md5(raw.tobytes()).digest()


# ---- the reference decoder ----------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, data, pos=0):
        self.d, self.p = data, pos * 8

    def read(self, n):
        if n == 0:
            return 0
        a, e = self.p >> 3, (self.p + n + 7) >> 3
        if e > len(self.d):
            raise ValueError("ran off the end of the stream")
        v = int.from_bytes(self.d[a:e], "big")
        v = (v >> (e * 8 - self.p - n)) & ((1 << n) - 1)
        self.p += n
        return v

    def signed(self, n):
        v = self.read(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self):
        q = 0
        while True:
            a = self.p >> 3
            chunk = self.d[a:a + 8]
            if not chunk:
                raise ValueError("ran off the end of the stream")
            nbits = len(chunk) * 8 - (self.p & 7)
            v = int.from_bytes(chunk, "big") & ((1 << nbits) - 1)
            if v:
                z = nbits - v.bit_length()
                self.p += z + 1
                return q + z
            q += nbits
            self.p += nbits


def parse_streaminfo(data):
    if data[:4] != b"fLaC":
        raise ValueError("not FLAC")
    pos, info = 4, None
    while True:
        last, typ, ln = data[pos] >> 7, data[pos] & 0x7F, int.from_bytes(data[pos + 1:pos + 4], "big")
        if typ == 0:
            b = data[pos + 4:pos + 38]
            x = int.from_bytes(b[10:18], "big")
            info = dict(min_bs=int.from_bytes(b[0:2], "big"), max_bs=int.from_bytes(b[2:4], "big"), rate=x >> 44, channels=((x >> 41) & 7) + 1,
                        bps=((x >> 36) & 31) + 1, total=x & ((1 << 36) - 1), md5=bytes(b[18:34]))
        pos += 4 + ln
        if last:
            return info, pos


def _decode_subframe(br, n, width):
    if br.read(1):
        raise ValueError("subframe padding bit set")
    typ = br.read(6)
    wasted = br.unary() + 1 if br.read(1) else 0
    width -= wasted
    if typ == 0:
        out = [br.signed(width)] * n
    elif typ == 1:
        out = [br.signed(width) for _ in range(n)]
    else:
        if 8 <= typ <= 12:
            order = typ - 8
            out = [br.signed(width) for _ in range(order)]
            coefs, shift = FIXED[order], 0
        elif typ >= 32:
            order = (typ & 31) + 1
            out = [br.signed(width) for _ in range(order)]
            prec = br.read(4) + 1
            shift = br.signed(5)
            if prec == 16 or shift < 0:
                raise ValueError("reserved LPC precision or negative shift")
            coefs = [br.signed(prec) for _ in range(order)]
        else:
            raise ValueError(f"reserved subframe type {typ}")
        method = br.read(2)
        if method > 1:
            raise ValueError("reserved residual coding method")
        pbits = 5 if method else 4
        porder = br.read(4)
        res = []
        for p in range(1 << porder):
            cnt = (n >> porder) - (order if p == 0 else 0)
            k = br.read(pbits)
            if k == (1 << pbits) - 1:
                w = br.read(5)
                res.extend(br.signed(w) for _ in range(cnt))
            else:
                for _ in range(cnt):
                    u = (br.unary() << k) | br.read(k)
                    res.append((u >> 1) ^ -(u & 1))
        if len(res) != n - order:
            raise ValueError("partition sizes do not add up")
        for r in res:
            acc = 0
            for j in range(order):
                acc += coefs[j] * out[-1 - j]
            out.append(r + (acc >> shift))
    return [s << wasted for s in out] if wasted else out


def decode_frame(data, pos, info):
    """One frame at byte `pos` -> (channels [C, bs], sample position, end offset).  Under fixed blocking the position is the frame
    number times the block size of the stream's FIRST frame (the second RFC example has STREAMINFO block sizes of 4096 and frames of
    16 and 3 samples: the minimum block size of STREAMINFO is not the stride)."""
    h = data[pos:pos + 4]
    if h[0] != 0xFF or (h[1] & 0xFE) != 0xF8:
        raise ValueError(f"no sync code at byte {pos}")
    variable = h[1] & 1
    bsc, src, assign, ssc = h[2] >> 4, h[2] & 15, h[3] >> 4, (h[3] >> 1) & 7
    if bsc == 0 or src == 15 or assign > 10 or ssc in (3, 7) or h[3] & 1:
        raise ValueError("reserved code in a frame header")
    p = pos + 4
    lead = data[p]
    n = 0
    while lead & (0x80 >> n):
        n += 1
    num = lead & (0x7F >> n) if n else lead
    for k in range(1, n):
        num = (num << 6) | (data[p + k] & 0x3F)
    p += max(n, 1)
    if bsc == 1:
        bs = 192
    elif bsc <= 5:
        bs = 576 << (bsc - 2)
    elif bsc == 6:
        bs, p = data[p] + 1, p + 1
    elif bsc == 7:
        bs, p = int.from_bytes(data[p:p + 2], "big") + 1, p + 2
    else:
        bs = 256 << (bsc - 8)
    p += {12: 1, 13: 2, 14: 2}.get(src, 0)
    if crc8(data[pos:p]) != data[p]:
        raise ValueError(f"CRC-8 mismatch at byte {pos}")
    bps = {0: info["bps"], 1: 8, 2: 12, 4: 16, 5: 20, 6: 24}[ssc]
    nch = assign + 1 if assign < 8 else 2
    br = _Bits(data, p + 1)
    chans = []
    for ch in range(nch):
        side = (assign == 8 and ch == 1) or (assign == 9 and ch == 0) or (assign == 10 and ch == 1)
        chans.append(_decode_subframe(br, bs, bps + (1 if side else 0)))
    end = (br.p + 7) >> 3
    if crc16(data[pos:end]) != int.from_bytes(data[end:end + 2], "big"):
        raise ValueError(f"CRC-16 mismatch in the frame at byte {pos}")
    a = np.array(chans, dtype=np.int64)
    if assign == 8:
        a[1] = a[0] - a[1]
    elif assign == 9:
        a[0] = a[0] + a[1]
    elif assign == 10:
        m = (a[0] << 1) | (a[1] & 1)
        a = np.stack([(m + a[1]) >> 1, (m - a[1]) >> 1])
    return a, (num if variable else num * info.setdefault("first_bs", bs)), end + 2


def decode(data) -> Decoded:
    data = bytes(data)
    info, pos = parse_streaminfo(data)
    out = np.zeros((info["channels"], info["total"]), np.int64)
    at = 0
    while pos < len(data):
        a, where, pos = decode_frame(data, pos, info)
        if where != at:
            raise ValueError(f"frame at sample {where}, expected {at}")
        out[:, at:at + a.shape[1]] = a
        at += a.shape[1]
    if at != info["total"]:
        raise ValueError(f"{at} samples decoded, STREAMINFO says {info['total']}")
    md5_ok = None if info["md5"] == bytes(16) else pcm_md5(out, info["bps"]) == info["md5"]
    return Decoded(out.astype(np.int32), info["rate"], info["bps"], md5_ok)


# ---- the encoder --------------------------------------------------------------------------------------------------------------
class Sub:
    """One subframe's choices.  kind: 'constant', 'verbatim', 'fixed', 'lpc'.  params: one entry per partition (2^porder of them), an int
    Rice parameter or ('esc', raw width)."""

    def __init__(self, kind="verbatim", order=0, coefs=None, precision=None, shift=0, wasted=0, method=0, porder=0, params=(0,)):
        self.kind, self.order, self.coefs, self.precision, self.shift = kind, order, coefs, precision, shift
        self.wasted, self.method, self.porder, self.params = wasted, method, porder, list(params)


class Frame:
    """One frame's choices.  assign: 0..7 = that many + 1 independent channels, 8 left/side, 9 side/right, 10 mid/side.  bs_form: 'code' (a
    table entry), 8 or 16 (trailing bits); rate_form: 'info', 'code', 'khz8', 'hz16', 'tenhz16'; size_form: 'info' or 'code'."""

    def __init__(self, bs, subs, assign=None, bs_form=None, rate_form="info", size_form="code"):
        self.bs, self.subs, self.assign, self.bs_form, self.rate_form, self.size_form = bs, list(subs), assign, bs_form, rate_form, size_form


def _bits(v, n):
    """n bits of v (two's complement for negative v), most significant first, as a uint8 array of 0/1."""
    v = np.asarray(v, np.int64).reshape(-1, 1)
    sh = np.arange(n - 1, -1, -1, dtype=np.int64)[None, :]
    return ((v >> sh) & 1).astype(np.uint8).reshape(-1) if n else np.zeros(0, np.uint8)


def _rice_bits(res, k):
    res = np.asarray(res, np.int64)
    u = (res << 1) ^ (res >> 63)
    q = u >> k
    ln = q + 1 + k
    start = np.concatenate([[0], np.cumsum(ln)[:-1]]) if len(res) else np.zeros(0, np.int64)
    out = np.zeros(int(ln.sum()), np.uint8)
    out[start + q] = 1
    for b in range(k):
        out[start + q + 1 + b] = (u >> (k - 1 - b)) & 1
    return out


def _utf8(v):
    if v < 0x80:
        return bytes([v])
    n = 2
    while v >= 1 << (5 * n + 1):
        n += 1
    out = [((0xFF << (8 - n)) & 0xFF) | (v >> (6 * (n - 1)))]
    for k in range(n - 2, -1, -1):
        out.append(0x80 | ((v >> (6 * k)) & 0x3F))
    return bytes(out)


def _subframe_bits(x, width, s: Sub):
    """x: the channel's samples (int64) as the subframe must reproduce them; width: its sample width before wasted bits."""
    n = len(x)
    if s.wasted:
        assert not np.any(x & ((1 << s.wasted) - 1)), "wasted bits are not zero in the signal"
        x = x >> s.wasted
    w = width - s.wasted
    assert w >= 1 and np.all(x >= -(1 << (w - 1))) and np.all(x < (1 << (w - 1))), "samples do not fit the subframe's width"
    typ = {"constant": 0, "verbatim": 1}.get(s.kind)
    if s.kind == "fixed":
        typ = 8 + s.order
    elif s.kind == "lpc":
        typ = 32 + s.order - 1
    parts = [_bits(0, 1), _bits(typ, 6), _bits(1 if s.wasted else 0, 1)]
    if s.wasted:
        parts.append(_bits(1, s.wasted))
    if s.kind == "constant":
        assert np.all(x == x[0])
        parts.append(_bits(x[0], w))
        return np.concatenate(parts)
    if s.kind == "verbatim":
        parts.append(_bits(x, w))
        return np.concatenate(parts)
    order = s.order
    coefs = np.array(FIXED[order] if s.kind == "fixed" else s.coefs, np.int64)
    shift = 0 if s.kind == "fixed" else s.shift
    assert len(coefs) == order and order <= n
    parts.append(_bits(x[:order], w))
    if s.kind == "lpc":
        assert 1 <= s.precision <= 15 and 0 <= shift <= 15
        assert np.all(coefs >= -(1 << (s.precision - 1))) and np.all(coefs < (1 << (s.precision - 1)))
        parts += [_bits(s.precision - 1, 4), _bits(shift, 5), _bits(coefs, s.precision)]
    pred = np.zeros(n - order, np.int64)
    for j in range(order):
        pred += coefs[j] * x[order - 1 - j:n - 1 - j]
    res = x[order:] - (pred >> shift)
    assert np.all(np.abs(res) < (1 << 31)), "a residual does not fit 32 bits"
    parts += [_bits(s.method, 2), _bits(s.porder, 4)]
    npart = 1 << s.porder
    assert len(s.params) == npart and (s.porder == 0 or n % npart == 0) and (n >> s.porder) >= order
    at = 0
    pbits = 5 if s.method else 4
    for p, par in enumerate(s.params):
        cnt = (n >> s.porder) - (order if p == 0 else 0)
        r = res[at:at + cnt]
        at += cnt
        if isinstance(par, tuple):
            rw = par[1]
            assert 0 <= rw <= 31 and (cnt == 0 or (rw == 0 and not np.any(r)) or (rw and np.all(r >= -(1 << (rw - 1))) and np.all(r < (1 << (rw - 1)))))
            parts += [_bits((1 << pbits) - 1, pbits), _bits(rw, 5), _bits(r, rw)]
        else:
            assert 0 <= par < (1 << pbits) - 1
            parts += [_bits(par, pbits), _rice_bits(r, par)]
    return np.concatenate(parts)


def encode_frame(pcm, number, rate, bps, fr: Frame, variable=False) -> bytes:
    """pcm [C, bs] -> one frame; number: the frame number, or the first sample's number under variable blocking."""
    pcm = np.asarray(pcm, np.int64)
    C, bs = pcm.shape
    assert bs == fr.bs and len(fr.subs) == C
    assign = C - 1 if fr.assign is None else fr.assign
    widths = [bps] * C
    if assign == 8:
        chans, widths = [pcm[0], pcm[0] - pcm[1]], [bps, bps + 1]
    elif assign == 9:
        chans, widths = [pcm[0] - pcm[1], pcm[1]], [bps + 1, bps]
    elif assign == 10:
        chans, widths = [(pcm[0] + pcm[1]) >> 1, pcm[0] - pcm[1]], [bps, bps + 1]
    else:
        chans = list(pcm)
    form = fr.bs_form
    if form is None:
        form = "code" if bs in BS_CODES else (8 if bs <= 256 else 16)
    bsc = BS_CODES[bs] if form == "code" else (6 if form == 8 else 7)
    src = {"info": 0, "code": RATE_CODES.get(rate), "khz8": 12, "hz16": 13, "tenhz16": 14}[fr.rate_form]
    ssc = 0 if fr.size_form == "info" else SIZE_CODES[bps]
    head = bytes([0xFF, 0xF8 | (1 if variable else 0), (bsc << 4) | src, (assign << 4) | (ssc << 1)]) + _utf8(number)
    if bsc == 6:
        head += bytes([bs - 1])
    elif bsc == 7:
        head += (bs - 1).to_bytes(2, "big")
    if src == 12:
        head += bytes([rate // 1000])
    elif src == 13:
        head += rate.to_bytes(2, "big")
    elif src == 14:
        head += (rate // 10).to_bytes(2, "big")
    head += bytes([crc8(head)])
    body = np.concatenate([_subframe_bits(np.asarray(c, np.int64), w, s) for c, w, s in zip(chans, widths, fr.subs)])
    frame = head + np.packbits(body).tobytes()
    return frame + crc16(frame).to_bytes(2, "big")


def streaminfo(rate, channels, bps, total, min_bs, max_bs, md5=bytes(16), min_frame=0, max_frame=0) -> bytes:
    x = (rate << 44) | ((channels - 1) << 41) | ((bps - 1) << 36) | total
    return (min_bs.to_bytes(2, "big") + max_bs.to_bytes(2, "big") + min_frame.to_bytes(3, "big") + max_frame.to_bytes(3, "big")
            + x.to_bytes(8, "big") + md5)


def container(info: bytes, frames: bytes, extra_blocks=()) -> bytes:
    """fLaC + STREAMINFO + extra metadata blocks ((type, payload) pairs) + the frames."""
    blocks = [(0, info)] + list(extra_blocks)
    out = b"fLaC"
    for k, (typ, body) in enumerate(blocks):
        out += bytes([(0x80 if k == len(blocks) - 1 else 0) | typ]) + len(body).to_bytes(3, "big") + body
    return out + frames


def encode(pcm, rate, bps, frames, variable=False, extra_blocks=(), md5=True, split=False):
    """pcm [C, N] int -> a FLAC file of the given frames (their block sizes must add up to N).  split: also return the header length
    and the frames' byte lengths."""
    pcm = np.asarray(pcm, np.int64)
    C, N = pcm.shape
    assert sum(f.bs for f in frames) == N
    at, out = 0, []
    sizes = [f.bs for f in frames]
    min_bs = min(sizes[:-1]) if len(sizes) > 1 else sizes[0]
    if not variable:
        assert all(s == sizes[0] for s in sizes[:-1]) and sizes[-1] <= sizes[0]
        min_bs = sizes[0]
    for k, f in enumerate(frames):
        out.append(encode_frame(pcm[:, at:at + f.bs], at if variable else k, rate, bps, f, variable))
        at += f.bs
    info = streaminfo(rate, C, bps, N, min_bs, max(sizes), pcm_md5(pcm, bps) if md5 else bytes(16))
    data = container(info, b"".join(out), extra_blocks)
    if split:
        return data, len(data) - sum(len(o) for o in out), [len(o) for o in out]
    return data


def rice_params(pcm_channel, sub: Sub, n_bs):
    """Fill sub.params with the best Rice parameter per partition for this channel (the one search the benchmark's encoder does:
    'parameters picked per partition'); the predictor itself stays as given."""
    x = np.asarray(pcm_channel, np.int64) >> sub.wasted
    coefs = np.array(FIXED[sub.order] if sub.kind == "fixed" else sub.coefs, np.int64)
    shift = 0 if sub.kind == "fixed" else sub.shift
    pred = np.zeros(n_bs - sub.order, np.int64)
    for j in range(sub.order):
        pred += coefs[j] * x[sub.order - 1 - j:n_bs - 1 - j]
    res = x[sub.order:] - (pred >> shift)
    u = (res << 1) ^ (res >> 63)
    at, params = 0, []
    for p in range(1 << sub.porder):
        cnt = (n_bs >> sub.porder) - (sub.order if p == 0 else 0)
        part = u[at:at + cnt]
        at += cnt
        best = min(range(15 if sub.method == 0 else 31), key=lambda k: int((part >> k).sum()) + (1 + k) * cnt)
        params.append(best)
    sub.params = params
    return sub
