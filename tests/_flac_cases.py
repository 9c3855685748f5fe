"""The FLAC test set, built once per process by the explicit encoder of _flac_ref: every case is (name, file bytes, pcm [C, N] int32,
rate, bits).  test_flac_cpu.py decodes each with the reference decoder; test_gpu_flac.py decodes all of them on the device."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import _flac_ref as R
from _flac_ref import Frame, Sub

Case = namedtuple("Case", "name data pcm rate bits")

# the worked examples of the format's RFC (libFLAC 1.3.3)
VECTORS = (
    ("rfc_1", "664c6143800000221000100000000f00000f0ac442f0000000013e84b41807dc690307586a3dad1a2e0f"
              "fff869180000bf0358fd03128baa9a", [[25588], [10416]], 44100, 16),
    ("rfc_2", "664c614300000022100010000000170000440ac442f000000013d5b0564975e98b8d8b930422757b8103"
              "03000012000000000000000000000000000000001000"
              "0400003a200000007265666572656e6365206c6962464c414320312e332e33203230313930383034"
              "010000000e0000005449544c453dd7a9d79cd795d79d"
              "81000006000000000000"
              "fff86998000f9912086701623d1442998f5df70d6fe00c17caeb21000ee7a77a24a1590c1217b603097b784faa9a33d285e070ad5b1b4851b4010d99d2cd1a68f1e6b810"
              "fff869180102a402c382c40bc14a03ee48dd03b67c1330",
     [[10372, 18041, 14942, 17876, 15627, 17899, 16242, 18077, 16824, 18263, 17295, -14418, -15201, -14508, -15195, -14818, -15486, -15349, -16054],
      [6070, 10545, 8743, 10449, 9143, 10463, 9502, 10569, 9840, 10680, 10113, -8428, -8895, -8476, -8896, -8653, -9072, -8958, -9410]],
     44100, 16),
    ("rfc_3", "664c6143800000221000100000001f00001f07d0007000000018f8f9e396f5cbcfc6dc807f9977906b32"
              "fff868020017e944004f6f313d1047d227cb6d090831452bdc2822228057a3",
     [[0, 79, 111, 78, 8, -61, -90, -68, -13, 42, 67, 53, 13, -27, -46, -38, -12, 14, 24, 19, 6, -4, -5, 0]], 32000, 8),
)
RFC_1_FRAME = bytes.fromhex("fff869180000bf0358fd03128baa9a")


def _noise(rng, C, N, bits, amp=None):
    """Uniform noise over the whole range (or +-amp), with both extremes present."""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    if amp is not None:
        lo, hi = max(lo, -amp), min(hi, amp)
    x = rng.integers(lo, hi + 1, size=(C, N), dtype=np.int64)
    x[:, 0], x[:, -1] = lo, hi
    return x


def _auto(sub, x, n):
    return R.rice_params(x, sub, n)


def _case(name, pcm, rate, bits, frames, **kw):
    pcm = np.asarray(pcm, np.int64)
    return Case(name, R.encode(pcm, rate, bits, frames, **kw), pcm.astype(np.int32), rate, bits)


def _types(rng):
    """constant, verbatim, fixed 0..4: one frame each, 16 bits, mono, blocks of 192; the last frame holds one sample."""
    bs = 192
    x = _noise(rng, 1, 7 * bs + 1, 16)
    x[0, :bs] = -12345
    subs = [Sub("constant"), Sub("verbatim")] + [Sub("fixed", order=o, method=1) for o in range(5)]
    frames = []
    for k, s in enumerate(subs):
        if s.kind == "fixed":
            _auto(s, x[0, k * bs:(k + 1) * bs], bs)
        frames.append(Frame(bs, [s]))
    frames.append(Frame(1, [Sub("verbatim")]))
    return _case("types16", x, 16000, 16, frames)


def _lpc_cross(rng):
    """LPC orders 1, 2, 8, 12, 32 x precision 1, 5, 12, 15 x shift 0, 14, coefficients alternating between the two ends of their range;
    16 bits, mono, blocks of 64.  The amplitude is bounded so that the residual fits 31 bits."""
    bs, frames, chunks = 64, [], []
    for order in (1, 2, 8, 12, 32):
        for prec in (1, 5, 12, 15):
            for shift in (0, 14):
                lo, hi = -(1 << (prec - 1)), (1 << (prec - 1)) - 1
                coefs = [lo if j % 2 == 0 else hi for j in range(order)]
                amp = min(32767, (1 << (29 + shift)) // (order * (1 << (prec - 1))))
                x = _noise(rng, 1, bs, 16, amp)
                s = _auto(Sub("lpc", order=order, coefs=coefs, precision=prec, shift=shift, method=1), x[0], bs)
                frames.append(Frame(bs, [s], bs_form=8))
                chunks.append(x)
    return _case("lpc_cross", np.concatenate(chunks, axis=1), 22050, 16, frames)


def _lpc_wide(rng):
    """24 bits, order 32, precision 15, shift 14, full-scale samples whose signs line up with the coefficients': the sum passes 2^42 and
    needs the 64-bit accumulator; the residual takes the 5-bit Rice form with parameter 30.  Second channel: the same through a side
    channel of 25 bits (left/side), verbatim."""
    bs, F = 64, (1 << 23) - 1
    left = np.array([F if n % 2 == 0 else -F for n in range(bs)], np.int64)
    coefs = [-16384 if j % 2 == 0 else 16383 for j in range(32)]
    right = -left - 1                                                  # side = left - right = +-2^24 - ...: 25 bits
    x = np.stack([left, right])
    fr = Frame(bs, [Sub("lpc", order=32, coefs=coefs, precision=15, shift=14, method=1, params=[30]), Sub("verbatim")], assign=8, bs_form=8)
    return _case("lpc_wide24", x, 96000, 24, [fr])


def _bits_cases(rng):
    out = []
    for bits in (8, 12, 16, 20, 24):
        for form in ("code", "info"):
            x = _noise(rng, 1, 33, bits)
            f0 = Frame(17, [Sub("verbatim")], size_form=form, bs_form=8)
            f1 = Frame(16, [_auto(Sub("fixed", order=2, method=1), x[0, 17:], 16)], size_form=form, bs_form=8)
            out.append(_case(f"bits{bits}_{form}", x, 8000, bits, [f0, f1], variable=True))
    return out


def _residual_forms(rng):
    """24 bits, mono, blocks of 256, fixed predictors of order 0 and 1 so that the residual is under the test's control."""
    bs, frames, chunks = 256, [], []

    def add(x, sub):
        chunks.append(np.asarray(x, np.int64)[None, :])
        frames.append(Frame(bs, [sub]))

    x = rng.integers(-2, 3, bs)
    x[100] = 100                                                       # Rice parameter 0: a unary run of 200 zeros
    x[200] = -300                                                      # and one of 599
    add(x, Sub("fixed", order=0, method=0, params=[0]))
    add(_noise(rng, 1, bs, 16)[0], Sub("fixed", order=0, method=0, params=[14]))
    add(_noise(rng, 1, bs, 18)[0], Sub("fixed", order=0, method=1, params=[16]))
    add(_noise(rng, 1, bs, 24)[0], Sub("fixed", order=0, method=1, params=[30]))
    add(np.zeros(bs), Sub("fixed", order=0, method=0, params=[("esc", 0)]))
    add(rng.integers(-1, 1, bs), Sub("fixed", order=0, method=1, params=[("esc", 1)]))
    add(_noise(rng, 1, bs, 17)[0], Sub("fixed", order=0, method=0, params=[("esc", 17)]))
    for porder in range(9):                                            # partition orders 0 .. 8; at 8 the first partition of the order-1
        npart = 1 << porder                                            # predictor holds no residual at all
        params = [(("esc", 13) if p % 3 == 2 else 9 + p % 3) for p in range(npart)]
        add(np.cumsum(rng.integers(-1500, 1501, bs)), Sub("fixed", order=1, method=p_method(porder), porder=porder, params=params))
    return _case("residual_forms", np.concatenate(chunks, axis=1), 48000, 24, frames)


def p_method(porder):
    return porder & 1


def _wasted(rng):
    """Wasted bits 1 and 7 on plain and on side channels (16 bits, stereo, blocks of 32)."""
    bs = 32
    a = _noise(rng, 2, bs, 16)
    a[0] &= ~1
    a[1] &= ~127
    b = _noise(rng, 2, bs, 15)
    b[1] = b[0] - 2 * rng.integers(-3000, 3000, bs)                    # left/side: the side channel has one wasted bit
    c = _noise(rng, 2, bs, 15)
    c[1] = c[0] - 128 * rng.integers(-100, 100, bs)                    # mid/side: seven
    d = _noise(rng, 2, bs, 15)
    d[0] = d[1] + 128 * rng.integers(-100, 100, bs)                    # side/right: seven
    frames = [Frame(bs, [Sub("verbatim", wasted=1), Sub("verbatim", wasted=7)], assign=1, bs_form=8),
              Frame(bs, [Sub("verbatim"), Sub("verbatim", wasted=1)], assign=8, bs_form=8),
              Frame(bs, [Sub("verbatim"), Sub("verbatim", wasted=7)], assign=10, bs_form=8),
              Frame(bs, [Sub("verbatim", wasted=7), Sub("verbatim")], assign=9, bs_form=8)]
    return _case("wasted", np.concatenate([a, b, c, d], axis=1), 44100, 16, frames)


def _channels(rng):
    out = []
    bs = 48
    x = _noise(rng, 2, 4 * bs, 16)                                     # random parities: odd mid + side sums among them
    frames = []
    for k, assign in enumerate((1, 8, 9, 10)):
        subs = [_auto(Sub("fixed", order=1, method=1), ch, bs) for ch in _stereo(x[:, k * bs:(k + 1) * bs], assign)]
        frames.append(Frame(bs, subs, assign=assign, bs_form=8))
    out.append(_case("stereo", x, 44100, 16, frames))
    for C in (3, 8):
        x = _noise(rng, C, 40, 12)
        out.append(_case(f"channels{C}", x, 48000, 12, [Frame(24, [Sub("verbatim")] * C, bs_form=8), Frame(16, [Sub("verbatim")] * C, bs_form=8)]))
    return out


def _stereo(x, assign):
    if assign == 8:
        return [x[0], x[0] - x[1]]
    if assign == 9:
        return [x[0] - x[1], x[1]]
    if assign == 10:
        return [(x[0] + x[1]) >> 1, x[0] - x[1]]
    return [x[0], x[1]]


def _block_sizes(rng):
    out = []
    for bs in (16, 17, 192, 576, 4096, 4608, 65535):
        x = _noise(rng, 1, bs + 1, 8)
        f0 = Frame(bs, [Sub("fixed", order=0, method=0, params=[6])])
        out.append(_case(f"block{bs}", x, 16000, 8, [f0, Frame(1, [Sub("verbatim")])]))      # a last frame of one sample
    # every block-size code in one variable-blocking stream (sample numbers of 1 to 3 bytes)
    sizes = [192, 576, 1152, 2304, 4608, 100, 1000, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768]
    forms = ["code"] * 5 + [8, 16] + ["code"] * 8
    x = _noise(rng, 1, sum(sizes), 8)
    x[0, 192:192 + 576] = 7
    frames = [Frame(s, [Sub("constant") if k == 1 else Sub("verbatim")], bs_form=f) for k, (s, f) in enumerate(zip(sizes, forms))]
    out.append(_case("block_codes_variable", x, 16000, 8, frames, variable=True))
    return out


def _rates(rng):
    out = []
    for rate in R.RATE_CODES:
        x = _noise(rng, 1, 16, 16)
        out.append(_case(f"rate{rate}", x, rate, 16, [Frame(16, [Sub("verbatim")], rate_form="code", bs_form=8)]))
    x = _noise(rng, 1, 5 * 16, 16)
    frames = [Frame(16, [Sub("verbatim")], rate_form=f, bs_form=8) for f in ("info", "code", "khz8", "hz16", "tenhz16")]
    out.append(_case("rate_forms", x, 16000, 16, frames))
    return out


def _many_frames(rng):
    """More than 2,048 frames under fixed blocking at 16 samples: frame numbers of 1, 2 and 3 bytes."""
    n = 2100
    x = _noise(rng, 1, 16 * n, 8)
    return _case("frames2100", x, 8000, 8, [Frame(16, [Sub("verbatim")], bs_form=8)] * n)


def _false_candidates(rng):
    """Verbatim payloads that spell a frame header with a correct CRC-8, and the whole of the RFC's first frame with its CRC-16."""
    out = []
    # 8 bits, mono, fixed blocks of 64: the spelled header claims frame 1 of the stream, with a 16-bit block size
    head = bytes([0xFF, 0xF8, 0x70, 0x02, 0x01, 0x00, 0x3F])
    head += bytes([R.crc8(head)])
    x = _noise(rng, 1, 3 * 64, 8)
    spell = np.frombuffer(head, np.int8).astype(np.int64)
    x[0, 10:10 + len(spell)] = spell
    x[0, 64 + 20:64 + 20 + len(spell)] = spell
    out.append(_case("false_header", x, 16000, 8, [Frame(64, [Sub("verbatim")], bs_form=8)] * 3))
    # 16 bits, stereo: the RFC's whole first frame (one sample, frame number 0) as eight big-endian samples of channel 0
    x = _noise(rng, 2, 40, 16)
    raw = RFC_1_FRAME + b"\x00"
    x[0, 5:13] = np.frombuffer(raw, ">i2").astype(np.int64)
    out.append(_case("false_frame", x, 44100, 16, [Frame(24, [Sub("verbatim")] * 2, bs_form=8), Frame(16, [Sub("verbatim")] * 2, bs_form=8)]))
    return out


@lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20280)
    out = [Case(name, bytes.fromhex(hx), np.array(pcm, np.int32), rate, bits) for name, hx, pcm, rate, bits in VECTORS]
    out += [_types(rng), _lpc_cross(rng), _lpc_wide(rng)] + _bits_cases(rng) + [_residual_forms(rng), _wasted(rng)]
    out += _channels(rng) + _block_sizes(rng) + _rates(rng) + [_many_frames(rng)] + _false_candidates(rng)
    return tuple(out)


@lru_cache(maxsize=None)
def refusal_base():
    """Four frames of 192 samples (16 bits, mono): (file bytes, header length, frame byte lengths, pcm)."""
    rng = np.random.default_rng(7)
    x = _noise(rng, 1, 4 * 192, 16)
    frames = [Frame(192, [_auto(Sub("fixed", order=2, method=0), x[0, k * 192:(k + 1) * 192], 192)]) for k in range(4)]
    data, head, sizes = R.encode(x, 16000, 16, frames, split=True)
    return data, head, sizes, x.astype(np.int32)


def refusals():
    """(name, damaged file bytes, the frame the error must name, a word of the reason)."""
    data, head, sizes, _ = refusal_base()
    starts = [head + sum(sizes[:k]) for k in range(4)]
    flipped = bytearray(data)
    flipped[starts[2] + sizes[2] // 2] ^= 0x10
    cut = data[:starts[3] + sizes[3] // 2]
    removed = data[:starts[1]] + data[starts[2]:]
    total = bytearray(data)
    x = int.from_bytes(total[8 + 10:8 + 18], "big") + 1                # STREAMINFO's total_samples, one too large
    total[8 + 10:8 + 18] = x.to_bytes(8, "big")
    return (("flipped_bit", bytes(flipped), 2, "CRC-16"), ("cut", cut, 3, "past the end"), ("removed", removed, 1, "sample position"),
            ("total_plus_one", bytes(total), 4, "short of"))
