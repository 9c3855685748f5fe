#!/usr/bin/env python3
"""Measure the second pass (decode.rescore_nbest, csrc/rescore.hip, K34): what it costs beside the host loop it replaces and beside the
beam search that feeds it, how far its scores are from the float64 oracle, and what it does to the word error rate of a synthetic task.

Without --step the tool is a driver: every GPU step is a child process of its own under `timeout` (--limit seconds each), the steps
run one after the other, and the first that fails, faults or runs out of time ends the run -- nothing more is started on the device.
    cases   tests/_rescore_ref.py's case list and the planted flip on the device against the oracle: counts and ranks equal, and the
            largest observed ratio of a score's error to its derived bound -> profiles/rescore_errors.json (also: --cases alone)
    timing  K24's headline shape: 32 utterances x 512 frames, V = 29, logits from the tests' generator, beam 16, nbest 16; the
            hypotheses are the beam search's own.  The model: WordNGramLM.fit of order 3 on sentences over a few thousand words -- the
            words of every third hypothesis and random ones.  Arms:
              (a) rescore_nbest, the whole call (workspace and outputs allocated: it is the call a user makes);
              (b) what a user does without it: .cpu() of the three tensors, then the float64 oracle per utterance, on the host clock;
              (c) ctc_beam_search of the same run, for proportion.
            (a) and (c): windows of at least --window seconds of back-to-back calls between device events, --rounds alternating rounds,
            median and spread (max - min) / median.  The bar: (b) / (a) - 1 > max(3 %, 3 x the larger spread); (a) / (c) has no bar.
    task    a learnable task in the manner of tools/bench_beam_lm.py: sentences of 6 words from a first-order chain over a lexicon of
            200 words; logits are the one-hot reference (each label one frame, a blank frame after it) at 20 nats plus
            standard_normal * --noise; the word model (order 2) and the character model (order 5) are fitted on a disjoint draw.
            WER and CER through ErrorRate for greedy, beam, beam + character LM, and the last two followed by the second pass over a
            small grid of word_lm_weight.  No threshold: the table is a property of this task.
Not measured: a trained acoustic model, a real language model, the kernel alone under a profiler.
    python tools/bench_rescore.py [--window 0.3] [--rounds 5] [--noise 5.0] [--limit 240] [--out profiles/rescore_bench.json]
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
import _rescore_ref as R  # noqa: E402
from _beam_ref import seeded_logits  # noqa: E402
from voice100_amd.decode import ctc_beam_search, ctc_greedy_decode, edit_distance, rescore_nbest  # noqa: E402
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
    lm, packed = R.flip_case()
    worst = {"scores": 0.0, "word_lm_scores": 0.0}
    cases = R.case_list() + [("the planted flip", lm, packed[0], packed[1], packed[2], {})]
    hyps = 0
    for name, lm, ids, lens, scores, kw in cases:
        ref = R.oracle(lm, ids, lens, scores, **kw)
        out = rescore_nbest(*(torch.from_numpy(a).to(dev) for a in (ids, lens, scores)), device_model(lm, dev), **kw)
        for k in ("order", "n_words", "n_oov"):
            if not np.array_equal(getattr(out, k).cpu().numpy(), ref[k]):
                raise SystemExit(f"bench_rescore.py: {name}: {k} differs from the oracle")
        for k, b in (("scores", "bound_score"), ("word_lm_scores", "bound_lm")):
            got = getattr(out, k).cpu().numpy().astype(np.float64)
            there = np.isfinite(ref[k])
            hyps += int(there.sum()) if k == "scores" else 0
            worst[k] = max(worst[k], float(np.max(np.abs(got[there] - ref[k][there]) / np.maximum(ref[b][there], 1e-300), initial=0.0)))
    return {"cases": len(cases), "hypotheses": hyps, "bound": "2^-23 (A + |value|), tests/_rescore_ref.py",
            "largest_error_over_bound": {k: round(v, 4) for k, v in worst.items()}, "counts_and_ranks": "equal to the oracle's in every case"}


def step_timing(dev, args):
    x = torch.from_numpy(seeded_logits(T, V, W, 3, B)).to(dev)
    first = ctc_beam_search(x, None, W, NBEST)
    ids, lens, scores = (t.cpu().numpy() for t in first)
    rng = np.random.default_rng(2026)
    seen = [R.split_words(ids[b, r], int(lens[b, r]), 1) for b in range(B) for r in range(0, NBEST, 3)]
    lex = sorted({w for s in seen for w in s} | set(R.lexicon(rng, 2000, longest=8)))
    train = [R.join(s) for s in seen if s] + [R.join(s) for s in R.sentences(rng, lex, 3000, longest=12)]
    t0 = time.perf_counter()
    host = WordNGramLM.fit(train, 1, 3, unk_logp=-math.log(10.0 * len(lex))).compile()
    built = time.perf_counter() - t0
    lm = device_model(host, dev)
    out = rescore_nbest(*first, lm)
    ref = R.oracle(host, ids, lens, scores)
    agree = int((out.order.cpu().numpy() == ref["order"]).all(axis=1).sum())
    t = []
    for _ in range(args.host_rounds):                                    # arm (b)
        t0 = time.perf_counter()
        h = tuple(a.cpu().numpy() for a in first)
        R.oracle(host, *h)
        t.append((time.perf_counter() - t0) * 1e3)
    host_arm = dict(summary(t), clock="host perf_counter, .cpu() copies included")
    arms = {"rescore": lambda: rescore_nbest(*first, lm), "beam_search": lambda: ctc_beam_search(x, None, W, NBEST)}
    iters = {}
    for k, fn in arms.items():
        per_call = max(window(fn, 3), 1e-4)
        iters[k] = max(3, int(args.window * 1e3 / per_call) + 1)
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            times[k].append(window(fn, iters[k]))
    res = {k: dict(summary(v), calls_per_window=iters[k]) for k, v in times.items()}
    spread = max(v["spread"] for v in res.values())
    bar = max(0.03, 3 * spread)
    a, c, b_ = res["rescore"]["median_ms"], res["beam_search"]["median_ms"], host_arm["median_ms"]
    nw = out.n_words.cpu().numpy()
    return {"shape": {"B": B, "T": T, "V": V, "beam_size": W, "nbest": NBEST, "lm_weight": 0.5, "word_bonus": 0.0, "use_eos": True},
            "method": f"windows of >= {args.window} s of back-to-back calls between device events, {args.rounds} alternating rounds; host "
                      f"arm: {args.host_rounds} call(s) on the host clock",
            "model": {"order": 3, "vocabulary": len(lex), "ngrams": [len(t_) for t_ in host.ngrams], "fit_and_compile_s": round(built, 2),
                      "table_bytes": int(host.pool.numel() * 8 + host.word_table.numel() * 4 + host.ngram_table.numel() * 4)},
            "hypotheses": {"mean_labels": round(float(lens.mean()), 1), "mean_words": round(float(nw.mean()), 1),
                           "unknown_word_share": round(float(out.n_oov.sum()) / max(int(nw.sum()), 1), 3),
                           "utterances_whose_ranking_equals_the_oracle": agree,
                           "utterances_whose_top_changed": int((out.order[:, 0] != 0).sum())},
            "arms": res, "host_arm": host_arm, "largest_spread": spread, "bar": round(bar, 4),
            "summary": {"rescore_ms": a, "host_ms": b_, "beam_search_ms": c, "host_over_rescore": round(b_ / a, 1),
                        "clears_the_bar": bool(b_ / a - 1 > bar), "rescore_share_of_beam_search": round(a / c, 4)}}


def step_task(dev, args, count=128, words_each=6, size=200):
    rng = np.random.default_rng(2027)
    lex = R.lexicon(rng, size, longest=6)
    init, trans = rng.dirichlet(np.full(size, 0.5)), rng.dirichlet(np.full(size, 0.05), size=size)

    def draw(n):
        out = []
        for _ in range(n):
            s = [int(rng.choice(size, p=init))]
            for _ in range(words_each - 1):
                s.append(int(rng.choice(size, p=trans[s[-1]])))
            out.append(R.join([lex[i] for i in s]))
        return out

    train, refs = draw(4000), draw(count)
    wlm = device_model(WordNGramLM.fit(train, 1, 2, unk_logp=-math.log(100.0 * size)).compile(), dev)
    clm = NGramLM.fit(train, V, 5).compile().to(dev)
    L = max(len(r) for r in refs)
    frames = 2 * L
    x = rng.standard_normal((count, frames, V)) * args.noise
    flen = np.zeros(count, dtype=np.int32)
    for b, ref in enumerate(refs):
        x[b, np.arange(0, 2 * len(ref), 2), ref] += 20.0
        x[b, 1:2 * len(ref):2, 0] += 20.0
        flen[b] = 2 * len(ref)
    x = torch.from_numpy(x.astype(np.float32)).to(dev)
    flen = torch.from_numpy(flen).to(dev)
    ref = torch.zeros((count, L), dtype=torch.int64, device=dev)
    for b, r in enumerate(refs):
        ref[b, :len(r)] = torch.tensor(r)
    ref_len = torch.tensor([len(r) for r in refs], dtype=torch.int32, device=dev)

    def rates(ids, lens):
        meter = ErrorRate(sep=1)
        meter.update(ids.contiguous(), lens.contiguous(), ref, ref_len)
        r = meter.compute()
        return {"wer": round(r["wer"], 5), "cer": round(r["cer"], 5)}

    out = {"utterances": count, "words_each": words_each, "lexicon": size, "noise": args.noise, "beam_size": W, "nbest": NBEST,
           "word_model": "WordNGramLM.fit, order 2, 4000 sentences of a disjoint draw", "character_model": "NGramLM.fit, order 5, the same text",
           "greedy": rates(*ctc_greedy_decode(x, flen))}
    plain = ctc_beam_search(x, flen, W, NBEST)
    fused = ctc_beam_search(x, flen, W, NBEST, lm=clm, lm_weight=1.0, length_bonus=1.0)
    out["beam"] = rates(plain[0][:, 0], plain[1][:, 0])
    out["beam_char_lm"] = dict(rates(fused[0][:, 0], fused[1][:, 0]), lm_weight=1.0, length_bonus=1.0)
    for key, hyp in (("beam_then_rescore", plain), ("beam_char_lm_then_rescore", fused)):
        grid = {}
        for weight in (0.25, 0.5, 1.0, 2.0):
            rs = rescore_nbest(hyp[0], hyp[1], hyp[2], wlm, lm_weight=weight)
            grid[f"word_lm_weight_{weight}"] = dict(rates(rs.ids[:, 0], rs.lens[:, 0]), top_changed=int((rs.order[:, 0] != 0).sum()))
        out[key] = grid
        out[key + "_best_wer"] = min(v["wer"] for v in grid.values())
    oracle_wer = []
    for hyp in (plain, fused):                           # the best the second pass could do: the n-best list's lowest error per utterance
        errs = []
        for r in range(NBEST):
            d, _, n = edit_distance(hyp[0][:, r].contiguous(), hyp[1][:, r].contiguous(), ref, ref_len, sep=1)
            errs.append(torch.where(hyp[2][:, r] > -float("inf"), d, torch.full_like(d, 1 << 20)))
        oracle_wer.append(round(float(torch.stack(errs).amin(0).sum()) / float(n.sum()), 5))
    out["nbest_oracle_wer"] = {"beam": oracle_wer[0], "beam_char_lm": oracle_wer[1]}
    out["not_measured"] = "a trained model, a real LM"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="least seconds per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=1)
    ap.add_argument("--noise", type=float, default=5.0)
    ap.add_argument("--limit", type=int, default=240, help="seconds each GPU step may take")
    ap.add_argument("--cases", action="store_true", help="only the cases step")
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step in this process and print its JSON (the driver's children)")
    ap.add_argument("--part", default=None, help="where a child writes its JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescore_bench.json"))
    ap.add_argument("--errors-out", default=os.path.join(ROOT, "profiles", "rescore_errors.json"))
    args = ap.parse_args()
    if args.step is not None:
        if not torch.cuda.is_available():
            raise SystemExit("bench_rescore.py needs a GPU (a timing taken anywhere else says nothing)")
        dev = torch.device("cuda:0")
        res = {"cases": step_cases, "timing": step_timing, "task": step_task}[args.step](dev, args)
        res["device"] = torch.cuda.get_device_name(0)
        with open(args.part, "w") as f:
            json.dump(res, f)
        return 0
    tmp = tempfile.mkdtemp(prefix="bench_rescore_")
    parts = {}
    for step in (("cases",) if args.cases else STEPS):
        part = os.path.join(tmp, step + ".json")
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--part", part,
               "--window", str(args.window), "--rounds", str(args.rounds), "--host-rounds", str(args.host_rounds), "--noise", str(args.noise)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"bench_rescore.py: step {step} ended with status {rc}; nothing more is started", file=sys.stderr)
            return rc
        parts[step] = json.load(open(part))
    os.makedirs(os.path.dirname(os.path.abspath(args.errors_out)), exist_ok=True)
    errors = dict({"tool": "tools/bench_rescore.py --cases"}, **parts["cases"])
    with open(args.errors_out, "w") as f:
        f.write(json.dumps(errors, indent=1) + "\n")
    print(json.dumps(errors, indent=1))
    if args.cases:
        return 0
    out = {"tool": "tools/bench_rescore.py", "device": parts["timing"].pop("device")}
    out.update(parts["timing"])
    parts["task"].pop("device")
    out["learnable_task"] = parts["task"]
    out["not_measured"] = "a trained model, a real LM; the kernel alone under a profiler (figures are whole calls with their allocations)"
    text = json.dumps(out, indent=1)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
