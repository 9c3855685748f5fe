#!/usr/bin/env python3
"""Measure minimum-Bayes-risk selection (decode.mbr_nbest, csrc/mbr.hip, K35): what it costs beside what the package could do before it
and beside the beam search that feeds it, how far its outputs are from the float64 oracle, and what it does to the word error rate of
tools/bench_rescore.py's synthetic task.

Without --step the tool is a driver: every GPU step is a child process of its own under `timeout` (--limit seconds each), the steps
run one after the other, and the first that fails, faults or runs out of time ends the run -- nothing more is started on the device.
    cases   tests/_mbr_ref.py's case list on the device against the oracle: every integer equal, and the largest observed ratio of an
            error to its derived bound per output -> profiles/mbr_errors.json (also: --cases alone)
    timing  K34's headline shape: 32 utterances x 512 frames, V = 29, logits from the tests' generator, beam 16, nbest 16; the
            hypotheses are the beam search's own; word and id level.  And one long list: B = 1, N = 16, about 4000 labels, each row a
            copy of a base row with at most 8 scattered edits (what LongASRPipeline.whole() produces).  Arms:
              (a) mbr_nbest, the whole call (workspace and outputs allocated: it is the call a user makes);
              (b) what the package could do before, on the device: the rows expanded to B N^2 pairs with stock indexing, ONE
                  edit_distance launch over them, torch.softmax / bmm / a stable sort / gathers; its outputs equal (a)'s;
              (c) .cpu() of the three tensors, then the float64 oracle, on the host clock (word level and the long list);
              (d) ctc_beam_search of the same run, for proportion.
            (a), (b), (d): windows of at least --window seconds of back-to-back calls between device events, --rounds alternating
            rounds, median and spread (max - min) / median.  The bar: (b) / (a) - 1 > max(3 %, 3 x the larger spread).
            For both shapes: the share of the DP cells that the trimming of common prefixes and suffixes leaves, counted on the host.
    task    bench_rescore.py's learnable task with its seeds and noise: WER / CER of beam, beam -> MBR (word level, scales 0.25, 0.5,
            1, 2), beam -> word rescoring -> MBR, and the same after the character LM; beside each the PREDICTED WER sum risk_0 / sum
            expected_len, and the list's floor from ref_dist, which must equal what bench_rescore.py's sixteen-call loop gives.
            No threshold: the table is a property of this task.
Not measured: a trained acoustic model, real recordings, the kernels alone under a profiler.
    python tools/bench_mbr.py [--window 0.3] [--rounds 5] [--noise 5.0] [--limit 240] [--out profiles/mbr_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mbr_ref as R  # noqa: E402
import _rescore_ref as RS  # noqa: E402
from _beam_ref import seeded_logits  # noqa: E402
from voice100_amd.decode import ctc_beam_search, edit_distance, mbr_nbest, rescore_nbest  # noqa: E402
from voice100_amd.infer import ErrorRate  # noqa: E402
from voice100_amd.lm import NGramLM, WordNGramLM  # noqa: E402

B, T, V, W, NBEST = 32, 512, 29, 16, 16
STEPS = ("cases", "timing", "task")


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters                                     # ms per call


def summary(times):
    med = statistics.median(times)
    return {"rounds_ms": [round(t, 5) for t in times], "median_ms": round(med, 5), "spread": round((max(times) - min(times)) / med, 4)}


def device_model(lm, dev):
    twin = WordNGramLM(lm.order, lm.ngrams, lm.sep, lm.blank, lm.symbols, lm.unk_logp)
    twin.pool, twin.pool_len, twin.word_table, twin.ngram_table, twin.meta = lm.pool, lm.pool_len, lm.word_table, lm.ngram_table, lm.meta
    return twin.to(dev)


def step_cases(dev, args):
    worst = {"posterior": 0.0, "risk": 0.0, "expected_len": 0.0}
    cases = R.case_list()
    hyps = 0
    for name, ids, lens, scores, kw in cases:
        ref = R.oracle(ids, lens, scores, **kw)
        dkw = {k: torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
        out = mbr_nbest(*(torch.from_numpy(a).to(dev) for a in (ids, lens, scores)), **dkw)
        bad, w = R.check(name, {k: None if v is None else v.cpu().numpy() for k, v in zip(out._fields, out)}, ref, ids, lens, scores)
        if bad:
            raise SystemExit("bench_mbr.py: " + "; ".join(bad))
        hyps += int(np.isfinite(ref["risk"]).sum())
        worst = {k: max(v, w[k]) for k, v in worst.items()}
    return {"cases": len(cases), "hypotheses": hyps, "bound": "2^-23 |value| + 2^-149, tests/_mbr_ref.py",
            "largest_error_over_bound": {k: round(v, 4) for k, v in worst.items()},
            "integers": "dist, ref_dist, ref_n, n_tokens and order equal to the oracle's in every case"}


def emulate(ids, lens, scores, sep, scale):
    """arm (b): the same outputs from K23's edit_distance over every ordered pair and stock tensor ops"""
    Bn, n, width = ids.shape
    hyp, hl = ids[:, :, None].expand(Bn, n, n, width).reshape(-1, width), lens[:, :, None].expand(Bn, n, n).reshape(-1)
    oth, ol = ids[:, None].expand(Bn, n, n, width).reshape(-1, width), lens[:, None].expand(Bn, n, n).reshape(-1)
    d, hn, _ = edit_distance(hyp.contiguous(), hl.contiguous(), oth.contiguous(), ol.contiguous(), sep=sep)
    here = scores > -math.inf
    both = here[:, :, None] & here[:, None]
    dist = torch.where(both, d.reshape(Bn, n, n), torch.full_like(d, -1).reshape(Bn, n, n))
    post = torch.nan_to_num(torch.softmax(torch.where(here, scores.double() * scale, torch.full_like(scores, -math.inf).double()), dim=1))
    risk = torch.bmm(dist.clamp(min=0).double(), post[:, :, None])[:, :, 0].float()
    risk = torch.where(here, risk, torch.full_like(risk, math.inf))
    ntok = torch.where(here, hn.reshape(Bn, n, n)[:, :, 0], torch.zeros_like(lens))
    elen = (post * ntok.double()).sum(1).float()
    order = torch.argsort(risk, dim=1, stable=True)
    g = lambda t: torch.gather(t, 1, order)                                # noqa: E731
    out_ids = torch.gather(ids, 1, order[:, :, None].expand(Bn, n, width))
    return out_ids, g(lens), g(scores), g(risk), g(post.float()), g(ntok), order.to(torch.int32), dist, elen


def cells_left(ids, lens, scores, sep):
    """the share of the N (N - 1) / 2 pairs' DP cells that remains once common prefixes and suffixes are stripped"""
    full = left = 0
    for b in range(ids.shape[0]):
        rows = [R.split_tokens(ids[b, i], int(lens[b, i]), sep) for i in range(ids.shape[1]) if R.present(scores[b, i])]
        for i in range(len(rows)):
            for j in range(i + 1, len(rows)):
                a, c = rows[i], rows[j]
                mn = min(len(a), len(c))
                p = 0
                while p < mn and a[p] == c[p]:
                    p += 1
                s = 0
                while s < mn - p and a[len(a) - 1 - s] == c[len(c) - 1 - s]:
                    s += 1
                full += len(a) * len(c)
                left += (len(a) - p - s) * (len(c) - p - s)
    return round(left / max(full, 1), 5)


def long_list(rng, n=16, labels=4000):
    base = rng.integers(2, V, size=labels)
    base[rng.random(labels) < 0.18] = 1                                  # words of a few labels
    rows = []
    for k in range(n):
        row = base.tolist()
        for _ in range(int(rng.integers(1, 9)) if k else 0):
            at, what = int(rng.integers(0, len(row))), int(rng.integers(0, 3))
            if what == 0:
                row[at] = int(rng.integers(2, V))
            elif what == 1:
                del row[at]
            else:
                row.insert(at, int(rng.integers(2, V)))
        rows.append(row)
    ids, lens = R.pack([rows])
    scores = np.sort(rng.uniform(-40.0, -30.0, size=(1, n)))[:, ::-1].astype(np.float32).copy()
    return ids, lens, scores


def time_arms(arms, args):
    iters = {}
    for k, fn in arms.items():
        per_call = max(window(fn, 3), 1e-4)
        iters[k] = max(3, int(args.window * 1e3 / per_call) + 1)
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            times[k].append(window(fn, iters[k]))
    return {k: dict(summary(v), calls_per_window=iters[k]) for k, v in times.items()}


def agree(a, b):
    """arm (b) against arm (a): the integers equal, the floats within a few fp32 roundings (torch's softmax and bmm sum in their own order)"""
    ok = torch.equal(a.dist, b[7]) and torch.equal(a.n_tokens, b[5]) and torch.equal(a.order, b[6]) and torch.equal(a.ids, b[0])
    fin = torch.isfinite(a.risk)
    return bool(ok and torch.allclose(a.risk[fin], b[3][fin], rtol=1e-5, atol=1e-30) and torch.allclose(a.posterior, b[4], rtol=1e-5, atol=1e-30))


def step_timing(dev, args):
    x = torch.from_numpy(seeded_logits(T, V, W, 3, B)).to(dev)
    first = ctc_beam_search(x, None, W, NBEST)
    host = tuple(t.cpu().numpy() for t in first)
    out = {"method": f"windows of >= {args.window} s of back-to-back calls between device events, {args.rounds} alternating rounds; host "
                     "arm: one call on the host clock", "shapes": {}}
    shapes = [("headline, word level", first, 1, True), ("headline, id level", first, None, False)]
    li, ll, ls = long_list(np.random.default_rng(2035))
    long = tuple(torch.from_numpy(a).to(dev) for a in (li, ll, ls))
    shapes += [("long list, word level", long, 1, True), ("long list, id level", long, None, False)]
    for name, hyp, sep, with_host in shapes:
        h = host if hyp is first else (li, ll, ls)
        arms = {"mbr_nbest": lambda: mbr_nbest(*hyp, sep=sep), "edit_distance_and_stock_ops": lambda: emulate(*hyp, sep, 1.0)}
        if hyp is first:
            arms["beam_search"] = lambda: ctc_beam_search(x, None, W, NBEST)
        same = agree(mbr_nbest(*hyp, sep=sep), emulate(*hyp, sep, 1.0))
        res = time_arms(arms, args)
        spread = max(v["spread"] for v in res.values())
        bar = max(0.03, 3 * spread)
        a, b_ = res["mbr_nbest"]["median_ms"], res["edit_distance_and_stock_ops"]["median_ms"]
        entry = {"shape": {"B": int(h[0].shape[0]), "nbest": int(h[0].shape[1]), "T": int(h[0].shape[2]),
                           "mean_labels": round(float(h[1].mean()), 1), "sep": sep, "scale": 1.0},
                 "arm_b_outputs_equal_arm_a": same, "dp_cells_left_after_trimming": cells_left(*h, sep), "arms": res,
                 "largest_spread": spread, "bar": round(bar, 4),
                 "summary": {"mbr_nbest_ms": a, "edit_distance_and_stock_ops_ms": b_, "b_over_a": round(b_ / a, 3),
                             "b_over_a_minus_1_clears_the_bar": bool(b_ / a - 1 > bar)}}
        if hyp is first:
            entry["summary"]["beam_search_ms"] = res["beam_search"]["median_ms"]
            entry["summary"]["mbr_share_of_beam_search"] = round(a / res["beam_search"]["median_ms"], 4)
        if with_host:                                                    # arm (c)
            t0 = time.perf_counter()
            R.oracle(*(t.cpu().numpy() for t in hyp), sep=sep)
            entry["host_arm"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "clock": "host perf_counter, .cpu() copies included, one call"}
            entry["summary"]["host_over_mbr_nbest"] = round(entry["host_arm"]["ms"] / a, 1)
        out["shapes"][name] = entry
    return out


def make_task(dev, args, count=128, words_each=6, size=200):
    """tools/bench_rescore.py's task, draw for draw: the same generator, seeds and order of draws"""
    rng = np.random.default_rng(2027)
    lex = RS.lexicon(rng, size, longest=6)
    init, trans = rng.dirichlet(np.full(size, 0.5)), rng.dirichlet(np.full(size, 0.05), size=size)

    def draw(n):
        out = []
        for _ in range(n):
            s = [int(rng.choice(size, p=init))]
            for _ in range(words_each - 1):
                s.append(int(rng.choice(size, p=trans[s[-1]])))
            out.append(RS.join([lex[i] for i in s]))
        return out

    train, refs = draw(4000), draw(count)
    wlm = device_model(WordNGramLM.fit(train, 1, 2, unk_logp=-math.log(100.0 * size)).compile(), dev)
    clm = NGramLM.fit(train, V, 5).compile().to(dev)
    L = max(len(r) for r in refs)
    x = rng.standard_normal((count, 2 * L, V)) * args.noise
    flen = np.zeros(count, dtype=np.int32)
    for b, ref in enumerate(refs):
        x[b, np.arange(0, 2 * len(ref), 2), ref] += 20.0
        x[b, 1:2 * len(ref):2, 0] += 20.0
        flen[b] = 2 * len(ref)
    ref = torch.zeros((count, L), dtype=torch.int64, device=dev)
    for b, r in enumerate(refs):
        ref[b, :len(r)] = torch.tensor(r)
    ref_len = torch.tensor([len(r) for r in refs], dtype=torch.int32, device=dev)
    return torch.from_numpy(x.astype(np.float32)).to(dev), torch.from_numpy(flen).to(dev), ref, ref_len, wlm, clm


def step_task(dev, args):
    x, flen, ref, ref_len, wlm, clm = make_task(dev, args)

    def rates(ids, lens):
        meter = ErrorRate(sep=1)
        meter.update(ids.contiguous(), lens.contiguous(), ref, ref_len)
        r = meter.compute()
        return {"wer": round(r["wer"], 5), "cer": round(r["cer"], 5)}

    def mbr_grid(hyp):
        grid = {}
        for scale in (0.25, 0.5, 1.0, 2.0):
            m = mbr_nbest(hyp[0], hyp[1], hyp[2], scale=scale)
            grid[f"scale_{scale}"] = dict(rates(m.ids[:, 0], m.lens[:, 0]), top_changed=int((m.order[:, 0] != 0).sum()),
                                          predicted_wer=round(float(m.risk[:, 0].double().sum() / m.expected_len.double().sum()), 5))
        return grid

    out = {"utterances": int(x.shape[0]), "noise": args.noise, "beam_size": W, "nbest": NBEST, "level": "word",
           "task": "tools/bench_rescore.py's: its seeds, its noise, its word model (order 2) and character model (order 5)"}
    plain = ctc_beam_search(x, flen, W, NBEST)
    fused = ctc_beam_search(x, flen, W, NBEST, lm=clm, lm_weight=1.0, length_bonus=1.0)
    floors = {}
    for key, hyp in (("beam", plain), ("beam_char_lm", fused)):
        out[key] = rates(hyp[0][:, 0], hyp[1][:, 0])
        out[key + "_then_mbr"] = mbr_grid(hyp)
        rs = rescore_nbest(hyp[0], hyp[1], hyp[2], wlm, lm_weight=0.5)
        out[key + "_then_rescore"] = dict(rates(rs.ids[:, 0], rs.lens[:, 0]), word_lm_weight=0.5)
        out[key + "_then_rescore_then_mbr"] = mbr_grid(rs)
        m = mbr_nbest(hyp[0], hyp[1], hyp[2], ref=ref, ref_len=ref_len)
        big = torch.full_like(m.ref_dist, 1 << 20)
        floor = float(torch.where(m.ref_dist >= 0, m.ref_dist, big).amin(1).sum()) / float(m.ref_n.sum())
        errs = []
        for r in range(NBEST):                                           # bench_rescore.py's sixteen-call loop
            d, _, n = edit_distance(hyp[0][:, r].contiguous(), hyp[1][:, r].contiguous(), ref, ref_len, sep=1)
            errs.append(torch.where(hyp[2][:, r] > -float("inf"), d, torch.full_like(d, 1 << 20)))
        loop = float(torch.stack(errs).amin(0).sum()) / float(n.sum())
        if floor != loop:
            raise SystemExit(f"bench_mbr.py: the floor from ref_dist, {floor}, is not the sixteen-call loop's, {loop}")
        floors[key] = round(floor, 5)
    out["nbest_floor_wer"] = dict(floors, equals_the_sixteen_call_loop=True)
    out["not_measured"] = "a trained model, real recordings; scale is not calibrated on held-out data"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="least seconds per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--noise", type=float, default=5.0)
    ap.add_argument("--limit", type=int, default=240, help="seconds each GPU step may take")
    ap.add_argument("--cases", action="store_true", help="only the cases step")
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step in this process and print its JSON (the driver's children)")
    ap.add_argument("--part", default=None, help="where a child writes its JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mbr_bench.json"))
    ap.add_argument("--errors-out", default=os.path.join(ROOT, "profiles", "mbr_errors.json"))
    args = ap.parse_args()
    if args.step is not None:
        if not torch.cuda.is_available():
            raise SystemExit("bench_mbr.py needs a GPU (a timing taken anywhere else says nothing)")
        dev = torch.device("cuda:0")
        res = {"cases": step_cases, "timing": step_timing, "task": step_task}[args.step](dev, args)
        res["device"] = torch.cuda.get_device_name(0)
        with open(args.part, "w") as f:
            json.dump(res, f)
        return 0
    tmp = tempfile.mkdtemp(prefix="bench_mbr_")
    parts = {}
    for step in (("cases",) if args.cases else STEPS):
        part = os.path.join(tmp, step + ".json")
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--part", part,
               "--window", str(args.window), "--rounds", str(args.rounds), "--noise", str(args.noise)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"bench_mbr.py: step {step} ended with status {rc}; nothing more is started", file=sys.stderr)
            return rc
        parts[step] = json.load(open(part))
    os.makedirs(os.path.dirname(os.path.abspath(args.errors_out)), exist_ok=True)
    errors = dict({"tool": "tools/bench_mbr.py --cases"}, **parts["cases"])
    with open(args.errors_out, "w") as f:
        f.write(json.dumps(errors, indent=1) + "\n")
    print(json.dumps(errors, indent=1))
    if args.cases:
        return 0
    out = {"tool": "tools/bench_mbr.py", "device": parts["timing"].pop("device")}
    out.update(parts["timing"])
    parts["task"].pop("device")
    out["learnable_task"] = parts["task"]
    out["not_measured"] = ("a trained model, real recordings; the kernels alone under a profiler, so no per-launch split (figures are whole "
                           "calls with their allocations)")
    text = json.dumps(out, indent=1)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
