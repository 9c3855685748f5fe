#!/usr/bin/env python3
"""Time the long-recording aligner (decode.ctc_align_long, csrc/align_long.hip, K29) and the windowed forward that feeds it.

Workload: B = 4 recordings of T = 90 000 frames (30 min at 50 frames/s) with 25 000 labels each, V = 29, band 2048; seeded planted
alignments (6 nats on the planted symbol) over N(0, 1) noise, log_softmax on the device.  Arms, in one process:
  (a) ctc_align_long: one library launch (plus the allocation of its outputs and workspace);
  (b) the same banded recurrence (moves, re-centring and renormalisation every 16 frames) in stock torch ops on the device, all four
      recordings batched.  It is TIMED OVER A SLICE of --slice frames and SCALED to T (a frame costs the same wherever it is: the
      window is always `band` wide); its traceback is not run, so the scaled figure flatters it;
  (c) the numpy fp32 mirror (tests/_align_long_ref.py) on the host, ONE recording, once, host clock -- and its score, ok, path and
      align are compared with the launch's for equality at the timed shape;
  (d) infer.windowed_logits of AudioToTextCTC(64, 512, 29, 512) over the same 30 minutes (180 000 mel frames, keep 1500) beside one
      plain forward of 32 x 1024 frames, in frames per second of audio.
(a), (b) and the two halves of (d) alternate over --rounds rounds; each timing is a window of back-to-back calls between two device
events, ended by a device synchronise.  Reported per arm: every round, the median and the spread (max - min) / median; a difference
between two arms counts only beyond the project's bar, max(3 %, 3 x the larger spread).
    python tools/bench_align_long.py [--rounds 5] [--slice 512] [--out profiles/align_long_bench.json]
    python tools/bench_align_long.py --resources-only      # no GPU: the compiler's resource report of the kernel, into the same file
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, T, L, V, BAND, R = 4, 90000, 25000, 29, 2048, 16


def resource_report():
    """VGPRs, SGPRs, scratch and static LDS of the two instantiations, from hipcc's -Rpass-analysis=kernel-resource-usage."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "voice100_amd", "csrc", "align_long.hip")
    cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(src),
           "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = "staged" if "ILb1E" in m.group(1) else "global_gather"
            out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                         ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"), ("static_lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"),
                         ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    lds = lambda band, staged: 128 + 2 * (band + 4) * 4 + band * 4 + 64 * 36 + 2 * 64 * 4 + (2 * 4096 * 4 if staged else 0)   # noqa: E731
    out["dynamic_lds_bytes"] = {"band_2048_staged": lds(2048, True), "band_8192_staged": lds(8192, True), "band_64_staged": lds(64, True)}
    out["threads_per_workgroup"] = 512
    return out


def window(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters                                 # ms per call


def summary(times):
    med = statistics.median(times)
    return {"rounds_ms": [round(t, 4) for t in times], "median_ms": round(med, 4), "spread": round((max(times) - min(times)) / med, 4)}


def stock_banded(lp, labels, frames, band=BAND, blank=0):
    """The recurrence of K29 in stock torch ops, batched over the recordings, for the first `frames` frames: scores, moves,
    re-centring and renormalisation; no traceback.  One read-back per re-centring would serialise it further; there is none."""
    import torch
    dev = lp.device
    nb, _, v = lp.shape
    n = 2 * labels.shape[1] + 1
    ext = torch.full((nb, n + band), blank, dtype=torch.int64, device=dev)
    ext[:, 1:n:2] = labels
    skip = torch.zeros((nb, n + band), dtype=torch.bool, device=dev)
    skip[:, 2:n] = (ext[:, 2:n] != blank) & (ext[:, 2:n] != ext[:, :n - 2])
    dead = (torch.arange(n + band, device=dev)[None, :] >= n).expand(nb, -1)
    neg = torch.tensor(float("-inf"), device=dev)
    sp = torch.full((nb, band + 2), float("-inf"), device=dev)
    sp[:, 2:4] = lp[:, 0].gather(1, ext[:, :2])
    lo = torch.zeros((nb, 1), dtype=torch.int64, device=dev)
    offset = torch.zeros((nb,), dtype=torch.float64, device=dev)
    moves = torch.empty((frames, nb, band), dtype=torch.uint8, device=dev)
    slots = torch.arange(band, device=dev)[None, :]
    hi = max(n - band, 0)
    for t0 in range(0, frames, R):
        if t0 > 0:
            s = sp[:, 2:]
            m, a = s.max(dim=1, keepdim=True)
            offset += m[:, 0].double()
            nlo = torch.clamp(torch.maximum(lo, lo + a - band // 2), max=hi)
            src = slots + (nlo - lo)
            sp[:, 2:] = torch.where(src < band, s.gather(1, src.clamp_max(band - 1)) - m, neg)
            lo = nlo
        idx = lo + slots
        c, sk, dd = ext.gather(1, idx), skip.gather(1, idx), dead.gather(1, idx)
        t1 = min(frames, t0 + R)
        emis = lp[:, t0:t1].gather(2, c[:, None, :].expand(nb, t1 - t0, band))
        for t in range(max(t0, 1), t1):
            s0, s1, s2 = sp[:, 2:], sp[:, 1:-1], sp[:, :-2]
            m1 = s1 > s0
            best = torch.where(m1, s1, s0)
            m2 = sk & (s2 > best)
            best = torch.where(m2, s2, best)
            moves[t] = m1.to(torch.uint8) + m2.to(torch.uint8) * (2 - m1.to(torch.uint8))
            sp[:, 2:] = torch.where(dd, neg, best + emis[:, t - t0])
    return sp, lo, offset, moves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slice", type=int, default=512, help="frames the stock-op arm is timed over")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_long_bench.json"))
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()
    prior = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            prior = json.load(f)
    if args.resources_only:
        prior["compiler_resource_report"] = resource_report()
        with open(args.out, "w") as f:
            f.write(json.dumps(prior, indent=1) + "\n")
        print(json.dumps(prior["compiler_resource_report"], indent=1))
        return
    import numpy as np
    import torch
    import _align_long_ref as ref
    from voice100_amd.asr import AudioToTextCTC
    from voice100_amd.decode import ctc_align_long
    from voice100_amd.infer import windowed_logits
    if not torch.cuda.is_available():
        raise SystemExit("bench_align_long.py needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    rows = [ref.planted(100 + b, T, L, V, nats=6.0) for b in range(B)]
    lp = torch.log_softmax(torch.from_numpy(np.stack([r[0] for r in rows])).to(dev), -1)
    labels = torch.from_numpy(np.stack([r[1] for r in rows])).to(dev)
    planted = np.stack([r[2] for r in rows])

    got = ctc_align_long(lp, labels, band=BAND)
    on_planted = float((got.path.cpu().numpy() == planted).mean())
    t0 = time.perf_counter()
    m_score, m_ok, m_path, m_align = ref.mirror(lp[0].cpu().numpy(), labels[0].cpu().numpy(), BAND)
    mirror_s = time.perf_counter() - t0
    equal = {"score": bool(float(got.score[0]) == m_score), "ok": bool(int(got.ok[0]) == m_ok),
             "path": bool(np.array_equal(got.path[0].cpu().numpy(), m_path)), "align": bool(np.array_equal(got.align[0].cpu().numpy(), m_align))}
    if not all(equal.values()):
        raise SystemExit(f"bench_align_long.py: the launch and the mirror disagree at the timed shape: {equal}")

    torch.manual_seed(0)
    model = AudioToTextCTC(64, 512, V, 512).to(dev).eval()
    feats = torch.randn(2 * T, 64, device=dev) * 2 - 4
    batch = torch.randn(32, 1024, 64, device=dev) * 2 - 4
    with torch.no_grad():
        arms = {"ctc_align_long": (lambda: ctc_align_long(lp, labels, band=BAND), 4),
                "stock_ops_slice": (lambda: stock_banded(lp, labels, args.slice), 1),
                "windowed_logits_30min": (lambda: windowed_logits(model, feats, keep=1500), 1),
                "plain_forward_32x1024": (lambda: model(batch), 4)}
        for fn, _ in arms.values():
            window(fn, 1)
        times = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, (fn, iters) in arms.items():
                times[k].append(window(fn, iters))
    res = {k: dict(summary(v), calls_per_window=arms[k][1]) for k, v in times.items()}
    stock_scaled = res["stock_ops_slice"]["median_ms"] * T / args.slice
    res["stock_ops_slice"].update(slice_frames=args.slice, scaled_to_T_ms=round(stock_scaled, 1),
                                  note="timed over the slice and scaled by T / slice; no traceback")
    res["numpy_mirror_host"] = {"seconds_one_recording": round(mirror_s, 2), "scaled_to_B_ms": round(mirror_s * B * 1e3, 0),
                                "note": "host clock, one run of one recording, scaled by B"}
    res["windowed_logits_30min"]["mel_frames_per_s"] = round(2 * T / res["windowed_logits_30min"]["median_ms"] * 1e3)
    res["plain_forward_32x1024"]["mel_frames_per_s"] = round(32 * 1024 / res["plain_forward_32x1024"]["median_ms"] * 1e3)
    a_ms = res["ctc_align_long"]["median_ms"]
    noise = max(res["ctc_align_long"]["spread"], res["stock_ops_slice"]["spread"])
    noise_d = max(res["windowed_logits_30min"]["spread"], res["plain_forward_32x1024"]["spread"])
    out = {"tool": "tools/bench_align_long.py", "device": torch.cuda.get_device_name(0),
           "shape": {"B": B, "T": T, "L": L, "V": V, "band": BAND, "workspace_bytes": B * (T * (BAND // 4) + (-(-T // R) * 4 + 15) // 16 * 16)},
           "method": f"windows of back-to-back calls between device events, {args.rounds} alternating rounds, one warm-up call per arm",
           "outputs_equal_mirror_at_timed_shape": equal, "fraction_of_frames_on_the_planted_path": round(on_planted, 6),
           "all_rows_ok": bool(int(got.ok.min()) == 1), "arms": res,
           "launch_ns_per_frame": round(a_ms * 1e6 / T, 1),          # the recordings run side by side, one workgroup each
           "stock_ops_scaled_over_launch": round(stock_scaled / a_ms, 1),
           "numpy_mirror_scaled_over_launch": round(mirror_s * B * 1e3 / a_ms, 1),
           "bar_align": round(max(0.03, 3 * noise), 4),
           "windowed_over_plain_throughput": round(res["windowed_logits_30min"]["mel_frames_per_s"] / res["plain_forward_32x1024"]["mel_frames_per_s"], 3),
           "bar_forward": round(max(0.03, 3 * noise_d), 4)}
    if "compiler_resource_report" in prior:
        out["compiler_resource_report"] = prior["compiler_resource_report"]
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
