#!/usr/bin/env python3
"""Time the device FLAC decoder (csrc/flac.hip, audio_io.decode_flac) on a LibriSpeech-shaped batch.

32 utterances of 10 to 16 s at 16 kHz, mono, 16 bits: a seeded harmonic-plus-noise signal with a moving pitch and a syllable envelope,
encoded ONCE outside every timed region by the explicit encoder of tests/_flac_ref.py with settings typical of the corpus (block size
4096, LPC order 8 from the windowed autocorrelation, 12-bit coefficients, the best partition order up to 5, the best Rice parameter per
partition).  Arms, alternating in rounds after a warm-up; each reports the median round and the spread (max - min) / median:
  a   decode_flac(list of bytes): parse, one host-to-device copy, the launches, the status read-back.  Host clock; the read-back
      synchronises.
  a'  v100_flac_decode alone, bytes and table resident on the device, outputs preallocated.  Device events around --iters calls.
  b   the same PCM as 16-bit WAV files through load_batch at the files' own rate: a copy and a convert -- the floor.  Host clock + synchronise.
  c   the reference decoder (tests/_flac_ref.py, plain Python) over the same batch.  Host clock.
The bar, in the project's form: c / a - 1 > max(3 %, 3 x the larger spread) -- the device path beats the only other FLAC decoder this
tree has.  No absolute time is a pass criterion.  Not measured here: the kernels under a profiler, real LibriSpeech files, libFLAC.
    python tools/bench_flac.py [--rounds 5] [--iters 10] [--ref-rounds 2] [--out profiles/flac_bench.json]
"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _flac_ref as R  # noqa: E402

RATE, BS, ORDER, PRECISION, MAX_PORDER = 16000, 4096, 8, 12, 5
README_STEP_MS = 3.02          # README.md: asr_en_base training step, B = 32 x 1024 frames, on one MI355X


def speechlike(rng, n):
    """Harmonics of a wandering pitch under a two-formant envelope, gated by a syllable-rate envelope, plus noise; int16."""
    t = np.arange(n) / RATE
    f0 = 120.0 + 40.0 * np.sin(2 * np.pi * 0.31 * t + rng.uniform(0, 6)) + 15.0 * np.sin(2 * np.pi * 1.7 * t + rng.uniform(0, 6))
    phase = 2 * np.pi * np.cumsum(f0) / RATE
    x = np.zeros(n)
    for h in range(1, 31):
        fh = h * 140.0
        gain = np.exp(-((fh - 600.0) / 400.0) ** 2) + 0.5 * np.exp(-((fh - 1900.0) / 600.0) ** 2) + 0.03
        x += gain / h ** 0.5 * np.sin(h * phase + rng.uniform(0, 6))
    env = np.clip(np.sin(2 * np.pi * 3.1 * t + rng.uniform(0, 6)) + 0.4, 0.0, None) ** 2
    x = x * env + 0.02 * rng.standard_normal(n) * (0.3 + env)
    x = x / np.abs(x).max() * 9000.0 + 12.0 * rng.standard_normal(n)
    return np.clip(np.round(x), -32768, 32767).astype(np.int64)


def lpc_sub(x):
    """The subframe choices for one block: order-8 LPC (Levinson-Durbin on the Hann-windowed autocorrelation), coefficients in 12 bits,
    the partition order up to 5 and per-partition Rice parameters that cost the fewest bits."""
    n = len(x)
    if n <= ORDER:
        return R.Sub("verbatim")
    w = x * np.hanning(n)
    r = np.array([float(np.dot(w[:n - k], w[k:])) for k in range(ORDER + 1)])
    r[0] = r[0] * (1 + 1e-9) + 1e-9
    a, err = np.zeros(ORDER), r[0]
    for i in range(ORDER):
        k = (r[i + 1] - np.dot(a[:i], r[i:0:-1])) / err
        a[:i + 1] = np.concatenate([a[:i] - k * a[:i][::-1], [k]])
        err *= 1.0 - k * k
    top = max(float(np.abs(a).max()), 1e-9)
    shift = int(min(15, max(0, PRECISION - 2 - int(np.floor(np.log2(top))))))
    coefs = np.clip(np.round(a * (1 << shift)), -(1 << (PRECISION - 1)), (1 << (PRECISION - 1)) - 1).astype(np.int64)
    pred = np.zeros(n - ORDER, np.int64)
    for j in range(ORDER):
        pred += coefs[j] * x[ORDER - 1 - j:n - 1 - j]
    res = x[ORDER:] - (pred >> shift)
    u = (res << 1) ^ (res >> 63)
    ks = np.arange(15)[:, None]
    best = None
    for porder in range(MAX_PORDER + 1):
        if n % (1 << porder) or (n >> porder) <= ORDER:
            break
        at, params, bits = 0, [], 6
        for p in range(1 << porder):
            cnt = (n >> porder) - (ORDER if p == 0 else 0)
            cost = (u[None, at:at + cnt] >> ks).sum(axis=1) + (1 + ks[:, 0]) * cnt
            at += cnt
            k = int(cost.argmin())
            params.append(k)
            bits += 4 + int(cost[k])
        if best is None or bits < best[0]:
            best = (bits, porder, params)
    return R.Sub("lpc", order=ORDER, coefs=[int(c) for c in coefs], precision=PRECISION, shift=shift, method=0, porder=best[1], params=best[2])


def encode_utterance(x):
    frames = [R.Frame(min(BS, len(x) - at), [lpc_sub(x[at:at + BS])]) for at in range(0, len(x), BS)]
    return R.encode(x[None, :], RATE, 16, frames)


def make_batch(utterances, lo, hi, seed=2028):
    rng = np.random.default_rng(seed)
    pcm = [speechlike(rng, int(rng.integers(int(lo * RATE), int(hi * RATE) + 1))) for _ in range(utterances)]
    return pcm, [encode_utterance(x) for x in pcm]


def med_spread(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m


def kernel_resources():
    """Registers, LDS and scratch of each kernel as the compiler reports them (compile only; 'not measured' without hipcc)."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return "not measured (no hipcc)"
    csrc = os.path.join(ROOT, "voice100_amd", "csrc")
    cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-Wno-unused-result",
           "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "flac.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: _Z\d+(flac_\w+_kernel)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out or "not measured (no remarks in the compiler's output)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--ref-rounds", type=int, default=2)
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--seconds", type=float, nargs=2, default=(10.0, 16.0))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flac_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_flac.py needs a GPU (a timing taken anywhere else says nothing)")
    from voice100_amd import _native as N
    from voice100_amd import audio_io as A
    dev = torch.device("cuda:0")

    t0 = time.perf_counter()
    pcm, files = make_batch(args.utterances, *args.seconds)
    encode_s = time.perf_counter() - t0
    samples = sum(len(x) for x in pcm)
    flac_bytes = sum(len(f) for f in files)
    frames = sum(-(-len(x) // BS) for x in pcm)
    tmp = tempfile.mkdtemp(prefix="flac_bench_")
    wavs = []
    for k, x in enumerate(pcm):
        wavs.append(os.path.join(tmp, f"u{k}.wav"))
        with wave.open(wavs[-1], "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(RATE)
            f.writeframes(x.astype("<i2").tobytes())

    # exactness first, at the size that is timed: the device's PCM is the encoder's input, and the WAV path gives the same floats
    wave_a, len_a, _, pcm_a = A.decode_flac(files, dev, return_pcm=True, verify_md5=True)
    wave_b, len_b = A.load_batch(wavs, RATE, dev)
    for b, x in enumerate(pcm):
        assert torch.equal(pcm_a[b, 0, :len(x)].cpu(), torch.from_numpy(x.astype(np.int32)))
    assert torch.equal(wave_a, wave_b) and torch.equal(len_a, len_b)

    # a': resident inputs and preallocated outputs
    names = [str(k) for k in range(len(files))]
    infos = [A.flac_info(f) for f in files]
    buf, table, S, H, stage_ints, longest = A._flac_plan(files, infos, names)
    B, Nmax = len(files), max(i.total_samples for i in infos)
    d_buf, d_table = torch.from_numpy(buf).to(dev), torch.from_numpy(table).to(dev)
    ws = torch.empty((int(N.helper("v100_flac_workspace_bytes", B, S, H, stage_ints)),), dtype=torch.uint8, device=dev)
    out = torch.zeros((B, Nmax), dtype=torch.float32, device=dev)
    lengths = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B, 2), dtype=torch.int32, device=dev)

    def arm_a():
        t = time.perf_counter()
        A.decode_flac(files, dev)
        return (time.perf_counter() - t) * 1e3

    def arm_a_launches():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            N.call("v100_flac_decode", d_buf, int(buf.size), d_table, ws, out, None, lengths, status, B, S, H, stage_ints, longest, 1, 1, Nmax)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    def arm_b():
        t = time.perf_counter()
        A.load_batch(wavs, RATE, dev)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for _ in range(3):
        arm_a(), arm_a_launches(), arm_b()
    assert int(status[:, 0].abs().max()) == 0 and torch.equal(out, wave_a)
    ta, tl, tb = [], [], []
    for _ in range(args.rounds):
        ta.append(arm_a())
        tl.append(arm_a_launches())
        tb.append(arm_b())
    tc = []
    for _ in range(args.ref_rounds):
        t = time.perf_counter()
        got = [R.decode(f).pcm for f in files]
        tc.append((time.perf_counter() - t) * 1e3)
    for x, g in zip(pcm, got):
        assert np.array_equal(g[0], x)
    shutil.rmtree(tmp, ignore_errors=True)

    (a, sa), (l, sl), (b, sb), (c, sc) = med_spread(ta), med_spread(tl), med_spread(tb), med_spread(tc)
    audio_s = samples / RATE
    margin, need = c / a - 1.0, max(0.03, 3.0 * max(sa, sc))

    def arm(ms, spread, rounds, clock):
        return {"median_ms": round(ms, 4), "spread": round(spread, 4), "rounds_ms": [round(v, 4) for v in rounds], "clock": clock,
                "flac_MB_in_per_s": round(flac_bytes / ms / 1e3, 2), "Msamples_out_per_s": round(samples / ms / 1e3, 3),
                "audio_seconds_per_second": round(audio_s / (ms / 1e3), 1)}
    result = {
        "tool": "tools/bench_flac.py", "device": torch.cuda.get_device_name(0),
        "batch": {"utterances": B, "seconds_each": list(args.seconds), "rate": RATE, "bits": 16, "channels": 1, "samples": samples,
                  "audio_seconds": round(audio_s, 2), "flac_bytes": flac_bytes, "wav_bytes": 2 * samples, "compression": round(flac_bytes / (2 * samples), 4),
                  "frames": frames, "frame_slots": S, "workspace_MB": round(ws.numel() / 1e6, 1),
                  "encoder": f"block {BS}, LPC order {ORDER}, precision {PRECISION}, partition order <= {MAX_PORDER}, Rice parameter per partition",
                  "encode_seconds_outside_the_timed_region": round(encode_s, 2)},
        "a_decode_flac_from_host_bytes": arm(a, sa, ta, "host clock, ends in the status read-back"),
        "a_prime_launches_only_resident_bytes": arm(l, sl, tl, f"device events around {args.iters} calls"),
        "b_load_batch_on_wav_files_floor": arm(b, sb, tb, "host clock + synchronise"),
        "c_reference_decoder_on_the_host": arm(c, sc, tc, "host clock"),
        "a_over_training_step": {"readme_step_ms": README_STEP_MS, "fraction": round(a / README_STEP_MS, 3),
                                 "note": "README.md: asr_en_base training step, B = 32 x 1024 frames (10.24 s of audio per row)"},
        "a_prime_over_training_step": round(l / README_STEP_MS, 3),
        "bar": {"c_over_a_minus_1": round(margin, 2), "needed": round(need, 4), "met": bool(margin > need)},
        "kernel_resources": kernel_resources(),
        "exact": "int32 PCM equals the encoder's input; float rows equal load_batch on 16-bit WAV files of the same PCM (torch.equal), MD5s verified",
        "not_measured": ["the kernels under a profiler (per-kernel times, LDS conflicts)", "real LibriSpeech files", "a comparison with libFLAC",
                         "the strided staging store (-DFLAC_STRIDED_STAGE) inside this run: it was timed in a process of its own, DESIGN.md K28"],
    }
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not result["bar"]["met"]:
        raise SystemExit("the bar is not met")


if __name__ == "__main__":
    main()
