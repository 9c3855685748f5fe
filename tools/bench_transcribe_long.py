#!/usr/bin/env python3
"""Time the CTC pause cutter (decode.ctc_cut_points, csrc/cut_points.hip, K31) and the long-form transcription built on it.

Workload: planted logits, V = 29: one-hot at 20 nats over N(0, 1) noise (as tools/bench_beam_lm.py), utterances of 100-300 frames
(2-6 s at 50 frames/s) separated by pauses of 30-80 blank frames; recordings of T = 90 000 frames (30 min).  Arms, in one process:
  (a) ctc_cut_points on 4 x 90 000 frames: two launches, the read-back of n_seg.max(), one launch for the tables;
  (b) the same tables from stock torch ops on the device (margins, run edges by nonzero -- which synchronises --, the cut flags), one
      read-back of the cores, then stage B and the pads on the host (the numpy mirror's own routines);
  (c) logits.cpu() plus the numpy mirror (tests/_cut_points_ref.py), host clock, once;
  (d) LongASRPipeline.segments(logits=) of ONE recording at max_batch 32: greedy, beam 16, beam 16 with an order-3 NGramLM.fit model;
  (e) the same three with max_batch 1: the same decode issued one segment per call;
and, for scale, infer.windowed_logits of AudioToTextCTC(64, 512, 29, 512) over one recording's 180 000 mel frames beside
ctc_cut_points of that one recording.  The tables of (a), (b) and (c) must be equal before anything is timed.  The device arms
alternate over --rounds rounds; each timing is a window of back-to-back calls between two device events, ended by a device synchronise.
Reported per arm: every round, the median and the spread (max - min) / median; a ratio counts only beyond the project's bar,
max(3 %, 3 x the larger spread).
    python tools/bench_transcribe_long.py [--rounds 5] [--out profiles/transcribe_long_bench.json]
    python tools/bench_transcribe_long.py --resources-only      # no GPU: the compiler's resource report of the kernels, into the same file
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

B, T, V = 4, 90000, 29
CUT = dict(max_frames=3000, min_gap=25, margin=0.0, pad=5, min_frames=50)


def resource_report():
    """VGPRs, SGPRs, scratch and static LDS of the kernels, from hipcc's -Rpass-analysis=kernel-resource-usage."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "voice100_amd", "csrc", "cut_points.hip")
    cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(src),
           "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            fn = m.group(1)
            name = ("frames_32_lanes" if "frames_kernelILi32" in fn else "frames_64_lanes" if "frames_kernelILi64" in fn
                    else "walk" if "walk_kernel" in fn else "table" if "table_kernel" in fn else fn)
            out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                         ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"), ("static_lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"),
                         ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    out["threads_per_workgroup"] = {"frames": 256, "walk": 512, "table": 256}
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


def stock_tables(logits, blank=0, **cut):
    """Arm (b): margins, silent runs, stage A and the cores in stock torch ops on the device; one read-back of the cores (and, only
    where a core is oversized, of the row's margins); stage B and the pads on the host."""
    import numpy as np
    import torch
    import _cut_points_ref as ref
    nb, t, v = logits.shape
    C, gap = cut["max_frames"] - 2 * cut["pad"], cut["min_gap"]
    keep = torch.arange(v, device=logits.device) != blank
    d = logits[:, :, blank] - logits[:, :, keep].amax(-1)
    silent = d > cut["margin"]
    packs = []
    for b in range(nb):
        loud = torch.nonzero(~silent[b])[:, 0]
        if loud.numel() == 0:
            packs.append(None)
            continue
        a0, b0 = loud[:1], loud[-1:] + 1
        s = silent[b].to(torch.int8)
        edge = s[1:] - s[:-1]
        rs, re = torch.nonzero(edge == 1)[:, 0] + 1, torch.nonzero(edge == -1)[:, 0] + 1
        inside = (rs > a0) & (rs < b0)
        rs = rs[inside]
        re = re[(re > a0) & (re <= b0)][:rs.numel()]
        cutf = (re - rs) >= gap
        packs.append((torch.cat([a0, re[cutf]]), torch.cat([rs[cutf], b0])))
    flat = torch.cat([torch.cat([torch.tensor([p[0].numel()], device=logits.device), p[0], p[1]]) if p is not None
                      else torch.zeros(1, dtype=torch.int64, device=logits.device) for p in packs]).cpu().numpy()       # the read-back
    rows, at = [], 0
    for b in range(nb):
        k = int(flat[at])
        starts, ends = flat[at + 1:at + 1 + k], flat[at + 1 + k:at + 1 + 2 * k]
        at += 1 + 2 * k
        if k and int((ends - starts).max()) > C:                    # stage B on the host: the mirror's routine on the row's margins
            pieces = ref.pieces_of_row(d[b].cpu().numpy(), **cut)
        else:
            pieces = [(int(a), int(e), 0) for a, e in zip(starts, ends)]
        rows.append(ref.pad_pieces(pieces, t, cut["pad"]))
    S = max(len(r[0]) for r in rows)
    out = np.zeros((3, nb, S), dtype=np.int32)
    for b, r in enumerate(rows):
        for k in range(3):
            out[k, b, :len(r[k])] = r[k]
    return out[0], out[1], out[2], np.array([len(r[0]) for r in rows], dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcribe_long_bench.json"))
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()
    prior = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            prior = json.load(f)
    if args.resources_only:
        prior["compiler_resource_report"] = resource_report()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(prior, indent=1) + "\n")
        print(json.dumps(prior["compiler_resource_report"], indent=1))
        return
    import numpy as np
    import torch
    import _cut_points_ref as ref
    from voice100_amd import _native as N
    from voice100_amd.asr import AudioToTextCTC
    from voice100_amd.decode import ctc_cut_points
    from voice100_amd.infer import LongASRPipeline, windowed_logits
    from voice100_amd.lm import NGramLM
    if not torch.cuda.is_available():
        raise SystemExit("bench_transcribe_long.py needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    rows = [ref.planted(200 + b, T, V, speech=(100, 300), amp=20.0) for b in range(B)]
    host = np.stack([r[0] for r in rows])
    logits = torch.from_numpy(host).to(dev)
    one = logits[0].contiguous()

    got = ctc_cut_points(logits, None, **CUT)
    dev_tab = [t.cpu().numpy() for t in got]
    stock_tab = stock_tables(logits, **CUT)
    t0 = time.perf_counter()
    mirror_tab = ref.mirror(logits.cpu().numpy(), None, **CUT)
    mirror_s = time.perf_counter() - t0
    equal = {"stock_ops": all(np.array_equal(a, b) for a, b in zip(dev_tab, stock_tab)),
             "numpy_mirror": all(np.array_equal(a, b) for a, b in zip(dev_tab, mirror_tab))}
    if not all(equal.values()):
        raise SystemExit(f"bench_transcribe_long.py: the tables of the three arms differ at the timed shape: {equal}")

    texts = []
    for s, e in zip(mirror_tab[0][0], mirror_tab[1][0]):
        seq = rows[0][1][s:e]
        seq = seq[np.concatenate([[True], seq[1:] != seq[:-1]])]
        texts.append([int(v) for v in seq if v != 0])
    lm = NGramLM.fit(texts, V, 3).compile().to(dev)
    decodes = {"greedy": {}, "beam16": dict(beam_size=16), "beam16_lm": dict(beam_size=16, lm=lm)}
    pipes = {(k, mb): LongASRPipeline(None, frame_seconds=0.02, max_batch=mb, **kw, **CUT) for k, kw in decodes.items() for mb in (32, 1)}
    ref_out = {k: pipes[(k, 32)].segments(logits=one) for k in decodes}
    for k in decodes:                                                 # the two ways of issuing the decode must agree, too
        alone = pipes[(k, 1)].segments(logits=one)
        if not all(torch.equal(alone[f], ref_out[k][f]) for f in ("seg_start", "ids", "ids_len")):
            raise SystemExit(f"bench_transcribe_long.py: {k}: one segment per call gives other ids than the batched decode")
    seg_len = (ref_out["greedy"]["seg_end"] - ref_out["greedy"]["seg_start"]).cpu().numpy()
    order = np.sort(seg_len)[::-1]
    padded = sum(int(order[lo]) * len(order[lo:lo + 32]) for lo in range(0, len(order), 32))

    torch.manual_seed(0)
    model = AudioToTextCTC(64, 512, V, 512).to(dev).eval()
    feats = torch.randn(2 * T, 64, device=dev) * 2 - 4
    with torch.no_grad():
        arms = {"ctc_cut_points_4x90000": (lambda: ctc_cut_points(logits, None, **CUT), 8),
                "stock_ops_4x90000": (lambda: stock_tables(logits, **CUT), 2),
                "ctc_cut_points_1x90000": (lambda: ctc_cut_points(one[None], None, **CUT), 8),
                "windowed_logits_30min": (lambda: windowed_logits(model, feats, keep=1500), 1)}
        for k in decodes:
            arms[f"segments_{k}_batched"] = ((lambda p=pipes[(k, 32)]: p.segments(logits=one)), 2)
            arms[f"segments_{k}_one_per_call"] = ((lambda p=pipes[(k, 1)]: p.segments(logits=one)), 1)
        for fn, _ in arms.values():
            window(fn, 1)
        times = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, (fn, iters) in arms.items():
                times[k].append(window(fn, iters))
    res = {k: dict(summary(v), calls_per_window=arms[k][1]) for k, v in times.items()}
    res["numpy_mirror_host_4x90000"] = {"seconds": round(mirror_s, 3), "note": "host clock, logits.cpu() included, one run"}
    a_ms = res["ctc_cut_points_4x90000"]["median_ms"]
    ratios = {}
    for k in decodes:
        b_, o_ = res[f"segments_{k}_batched"], res[f"segments_{k}_one_per_call"]
        ratios[k] = {"one_per_call_over_batched": round(o_["median_ms"] / b_["median_ms"], 2),
                     "bar": round(max(0.03, 3 * max(b_["spread"], o_["spread"])), 4)}
    out = {"tool": "tools/bench_transcribe_long.py", "device": torch.cuda.get_device_name(0),
           "shape": {"B": B, "T": T, "V": V, **{k: v for k, v in CUT.items()}, "workspace_bytes": int(N.helper("v100_ctc_cut_points_workspace_bytes", B, T)),
                     "logits_bytes": B * T * V * 4},
           "method": f"windows of back-to-back calls between device events, {args.rounds} alternating rounds, one warm-up call per arm",
           "tables_equal_at_timed_shape": equal, "segments_per_recording": [int(v) for v in dev_tab[3]],
           "forced_cuts": int(dev_tab[2].sum()), "arms": res,
           "stock_ops_over_launch": round(res["stock_ops_4x90000"]["median_ms"] / a_ms, 1),
           "numpy_mirror_over_launch": round(mirror_s * 1e3 / a_ms, 1),
           "bar_cutter": round(max(0.03, 3 * max(res["ctc_cut_points_4x90000"]["spread"], res["stock_ops_4x90000"]["spread"])), 4),
           "cutter_share_of_windowed_forward": round(res["ctc_cut_points_1x90000"]["median_ms"] / res["windowed_logits_30min"]["median_ms"], 5),
           "segments_of_the_decoded_recording": int(len(seg_len)),
           "padded_frame_fraction_at_max_batch_32": round(1.0 - float(seg_len.sum()) / padded, 4),
           "decode": ratios,
           "not_measured": ["a profiler run (counters, achieved bandwidth of the frame pass)", "a trained model", "real recordings",
                            "other vocabularies, max_frames or min_gap", "recordings with forced cuts at this length"]}
    if "compiler_resource_report" in prior:
        out["compiler_resource_report"] = prior["compiler_resource_report"]
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
