#!/usr/bin/env python3
"""Time the device FLAC encoder (csrc/flac_enc.hip, audio_io.encode_flac) on the batch tools/bench_flac.py decodes: 32 utterances of
10 to 16 s at 16 kHz, mono, 16 bits (the same seeded speech-like signal), as float32 rows on the device.

Arms, alternating in rounds after a warm-up; each reports the median round and the spread (max - min) / median:
  a   encode_flac(device tensor, lengths) -> a list of bytes on the host: the frame table, the launches, both read-backs.  Host clock.
      Run at max_lpc_order 0, 8 (the default) and 12.
  b   v100_flac_encode alone, everything resident and preallocated.  Device events around --iters calls.  Same three settings.
  c   what one could do before: wave.cpu(), to int16, stdlib `wave` into memory -- no compression at all.  Host clock.
  d   the explicit encoder of tests/_flac_ref.py with a fixed order-2 predictor and the best Rice parameter per partition (partition
      order 3), timed over --ref-utterances utterances and scaled to the batch by samples.  Host clock.
  e   decode_flac of arm a's files in this same run, beside the 4.36 ms the decoder's own bench recorded for its batch.
Sizes: the files of each setting against the WAV bytes, and LPC against the fixed-only optimum (max_lpc_order 0: the search is exact,
so that is the optimum over constant / verbatim / fixed 0-4).  No time or ratio is a pass criterion; two arms differ only beyond
max(3 %, 3 x the larger spread).  Not measured: the kernels under a profiler, real recordings, libFLAC's sizes.
    python tools/bench_flac_enc.py [--rounds 5] [--iters 10] [--out profiles/flac_enc_bench.json]
"""
import argparse
import io
import json
import os
import re
import shutil
import subprocess
import sys
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _flac_ref as R  # noqa: E402
from bench_flac import RATE, med_spread, speechlike  # noqa: E402

DECODER_BENCH_MS = 4.36        # profiles/flac_bench.json of the parent commit: decode_flac from host bytes, its own batch


def kernel_resources():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return "not measured (no hipcc)"
    csrc = os.path.join(ROOT, "voice100_amd", "csrc")
    cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-Wno-unused-result",
           "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "flac_enc.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: _Z\d+(flac_enc_\w+_kernel)", line)
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
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--ref-utterances", type=int, default=1)
    ap.add_argument("--seconds", type=float, nargs=2, default=(10.0, 16.0))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flac_enc_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_flac_enc.py needs a GPU (a timing taken anywhere else says nothing)")
    from voice100_amd import _native as N
    from voice100_amd import audio_io as A
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2028)
    lo, hi = args.seconds
    pcm = [speechlike(rng, int(rng.integers(int(lo * RATE), int(hi * RATE) + 1))) for _ in range(args.utterances)]
    lens = [len(x) for x in pcm]
    samples, B, Nmax = sum(lens), len(pcm), max(lens)
    host = np.zeros((B, Nmax), np.float32)
    for b, x in enumerate(pcm):
        host[b, :len(x)] = x.astype(np.float32) / 32768.0
    wave_d = torch.from_numpy(host).to(dev)

    # exactness first, at the size that is timed
    files = {lpc: A.encode_flac(wave_d, lens, RATE, max_lpc_order=lpc, md5=True) for lpc in (0, 8, 12)}
    for lpc, fl in files.items():
        _, _, _, got = A.decode_flac(fl, dev, return_pcm=True, verify_md5=True)
        for b, x in enumerate(pcm):
            assert torch.equal(got[b, 0, :len(x)].cpu(), torch.from_numpy(x.astype(np.int32))), (lpc, b)
    assert np.array_equal(R.decode(files[8][0]).pcm[0], pcm[0])

    # b: resident inputs, preallocated outputs
    ftab, first, out_bytes = A._flac_enc_plan(lens, list(range(B)), [0] * B, B, Nmax, 1, 16, 4096)
    F = ftab.shape[0]
    d_ftab = torch.from_numpy(ftab).to(dev)
    ws = torch.empty((int(N.helper("v100_flac_encode_workspace_bytes", F, 1)),), dtype=torch.uint8, device=dev)
    out = torch.empty((out_bytes,), dtype=torch.uint8, device=dev)
    report = torch.empty((F,), dtype=torch.int32, device=dev)
    status = torch.empty((B, 2), dtype=torch.int32, device=dev)

    def arm_a(lpc):
        t = time.perf_counter()
        A.encode_flac(wave_d, lens, RATE, max_lpc_order=lpc)
        return (time.perf_counter() - t) * 1e3

    def arm_b(lpc):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            N.call("v100_flac_encode", wave_d, None, d_ftab, ws, out, report, status, B, F, B, 1, Nmax, 16, 4096, lpc, 6, 5, 0, out_bytes)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    def arm_c():
        t = time.perf_counter()
        q = (wave_d * 32768.0).round().clamp(-32768, 32767).to(torch.int16).cpu().numpy()
        blobs = []
        for b, n in enumerate(lens):
            buf = io.BytesIO()
            with wave.open(buf, "wb") as f:
                f.setnchannels(1)
                f.setsampwidth(2)
                f.setframerate(RATE)
                f.writeframes(q[b, :n].astype("<i2").tobytes())
            blobs.append(buf.getvalue())
        return (time.perf_counter() - t) * 1e3

    def arm_e():
        t = time.perf_counter()
        A.decode_flac(files[8], dev)
        return (time.perf_counter() - t) * 1e3

    for _ in range(3):
        for lpc in (0, 8, 12):
            arm_a(lpc), arm_b(lpc)
        arm_c(), arm_e()
    assert int(status[:, 0].abs().max()) == 0
    ta, tb, tc, te = {0: [], 8: [], 12: []}, {0: [], 8: [], 12: []}, [], []
    for _ in range(args.rounds):
        for lpc in (0, 8, 12):
            ta[lpc].append(arm_a(lpc))
            tb[lpc].append(arm_b(lpc))
        tc.append(arm_c())
        te.append(arm_e())
    # d: the host encoder this tree had, over a slice
    td, ref_samples = [], sum(lens[:args.ref_utterances])
    for _ in range(2):
        t = time.perf_counter()
        for x in pcm[:args.ref_utterances]:
            frames = []
            for at in range(0, len(x), 4096):
                seg = x[at:at + 4096]
                porder = 3 if len(seg) % 8 == 0 and len(seg) // 8 > 2 else 0
                sub = R.Sub("fixed", order=2, porder=porder, params=[0] * (1 << porder)) if len(seg) > 2 else R.Sub("verbatim")
                frames.append(R.Frame(len(seg), [R.rice_params(seg, sub, len(seg)) if sub.kind == "fixed" else sub]))
            R.encode(x[None], RATE, 16, frames)
        td.append((time.perf_counter() - t) * 1e3 * samples / ref_samples)

    audio_s = samples / RATE

    def arm(v, clock):
        m, s = med_spread(v)
        return {"median_ms": round(m, 4), "spread": round(s, 4), "rounds_ms": [round(x, 4) for x in v], "clock": clock,
                "audio_seconds_per_second": round(audio_s / (m / 1e3), 1), "Msamples_per_s": round(samples / m / 1e3, 3)}

    def differ(x, y):
        (mx, sx), (my, sy) = med_spread(x), med_spread(y)
        return {"ratio": round(mx / my, 3), "needed": round(max(0.03, 3 * max(sx, sy)), 4), "different": bool(abs(mx / my - 1) > max(0.03, 3 * max(sx, sy)))}
    sizes = {lpc: sum(len(f) for f in fl) for lpc, fl in files.items()}
    result = {
        "tool": "tools/bench_flac_enc.py", "device": torch.cuda.get_device_name(0),
        "batch": {"utterances": B, "seconds_each": list(args.seconds), "rate": RATE, "bits": 16, "channels": 1, "samples": samples,
                  "audio_seconds": round(audio_s, 2), "frames": F, "block_size": 4096, "max_partition_order": 6,
                  "workspace_MB": round(ws.numel() / 1e6, 2), "output_buffer_MB": round(out_bytes / 1e6, 2)},
        "a_encode_flac_to_host_bytes": {f"max_lpc_order_{lpc}": arm(ta[lpc], "host clock, ends in the second read-back") for lpc in (0, 8, 12)},
        "b_launches_only_resident": {f"max_lpc_order_{lpc}": arm(tb[lpc], f"device events around {args.iters} calls") for lpc in (0, 8, 12)},
        "c_cpu_int16_stdlib_wave_in_memory": arm(tc, "host clock"),
        "d_reference_encoder_fixed2_scaled": dict(arm(td, "host clock, scaled by samples"), utterances_timed=args.ref_utterances),
        "e_decode_flac_of_arm_a_files": dict(arm(te, "host clock, ends in the status read-back"), parent_commit_own_batch_ms=DECODER_BENCH_MS),
        "comparisons": {"a8_over_c": differ(ta[8], tc), "a8_over_a0": differ(ta[8], ta[0]), "a12_over_a8": differ(ta[12], ta[8]),
                        "b8_over_b0": differ(tb[8], tb[0]), "b12_over_b8": differ(tb[12], tb[8]), "d_over_a8": differ(td, ta[8])},
        "bytes": {"wav": 2 * samples + 44 * B, **{f"flac_max_lpc_order_{lpc}": s for lpc, s in sizes.items()},
                  "flac8_over_wav": round(sizes[8] / (2 * samples + 44 * B), 4), "flac8_over_fixed_only_optimum": round(sizes[8] / sizes[0], 4),
                  "flac12_over_fixed_only_optimum": round(sizes[12] / sizes[0], 4)},
        "kernel_resources": kernel_resources(),
        "exact": "every file of every setting decodes on the device to the encoder's input with its MD5 verified; file 0 also through tests/_flac_ref.py",
        "not_measured": ["the kernels under a profiler (per-kernel times)", "real recordings", "libFLAC's sizes and speed"],
    }
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
