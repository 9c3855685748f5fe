"""Accuracy of the CTC head (K10) against float64.
  (no option)  relative L2 over a batch, next to torch's float32 CPU lattice, at three training shapes
  --cases      per utterance over the cases of tests/_ctc_cases.py: the kernel's max-abs gradient error, torch's float32 error e32, the
               random-walk term, the bar of tests/test_gpu_ctc_oracle.py and err / bar; written to profiles/ctc_oracle_errors.json"""
import argparse, json, os, sys, torch, torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from voice100_amd import functional as F_
dev = torch.device("cuda")


def batch_l2():
    for (B, T, V, L) in ((3, 700, 29, 300), (2, 1100, 29, 505), (32, 512, 29, 100)):
        g = torch.Generator().manual_seed(B * 100 + T)
        logits = torch.randn(B, T, V, generator=g) * 2
        targets = torch.randint(1, V, (B, L), generator=g)
        in_len = torch.randint(min(2 * L + 1, T), T + 1, (B,), generator=g).to(torch.int32)
        tgt_len = torch.randint(1, L + 1, (B,), generator=g).to(torch.int32)
        res = {}
        for name, dt in (("f64", torch.float64), ("f32cpu", torch.float32)):
            x = logits.to(dt).clone().requires_grad_(True)
            l = F.ctc_loss(F.log_softmax(x.transpose(0, 1), dim=-1), targets, in_len, tgt_len, blank=0, reduction="mean", zero_infinity=True)
            l.backward(); res[name] = (float(l), x.grad.double())
        x = logits.to(dev).requires_grad_(True)
        l = F_.ctc_loss(x, targets.to(dev), in_len.to(dev), tgt_len.to(dev)); l.backward()
        res["hip"] = (float(l), x.grad.cpu().double())
        ref = res["f64"]
        for k in ("f32cpu", "hip"):
            d = (res[k][1] - ref[1]).norm() / ref[1].norm()
            print(f"B{B} T{T} L{L} {k:7s}: loss err {abs(res[k][0]-ref[0])/abs(ref[0]):.2e}  grad rel-L2 err vs f64 {float(d):.2e}")


def per_utterance(out_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _ctc_cases as C
    from voice100_amd import _native as N
    rows, worst = [], {}
    for case in C.CASES:
        ref, reg = C.reference(case), C.regime(case)
        logits, labels = C.inputs(case)
        B, T, V, L = case.B, case.T, case.V, case.Lmax
        ws = torch.empty(int(N.helper("v100_ctc_workspace_floats", B, T, L)), device=dev)
        nll, grad = torch.empty(B, device=dev), torch.empty(B, T, V, device=dev)
        N.call("v100_ctc_loss", logits.to(dev), labels.to(dev), torch.tensor(case.in_len, dtype=torch.int32, device=dev),
               torch.tensor(case.tgt_len, dtype=torch.int32, device=dev), ws, nll, grad, B, T, V, L, case.blank)
        nll, G = nll.cpu().double(), grad.cpu().double()
        bar, rw = C.grad_bar(case, ref), C.random_walk_term(case, ref)
        kernel = reg["kernel"] + (f"/{reg['waves']}w" if reg["kernel"] == "skew" else "")
        for b in range(B):
            err = float((G[b] - ref.G64[b]).abs().max())
            want = float(ref.nll64[b])
            nll_rel = None if want == float("inf") else abs(float(nll[b]) - want) / max(1.0, abs(want))
            rows.append({"case": case.name, "utterance": b, "kernel": kernel, "live": reg["live"][b], "in_len": case.in_len[b],
                         "tgt_len": case.tgt_len[b], "nll64": want if nll_rel is not None else "inf", "nll_rel_err": nll_rel,
                         "grad_max_abs_err": err, "e32": float(ref.e32[b]), "random_walk": float(rw[b]), "bar": float(bar[b]),
                         "ratio": err / float(bar[b]), "err_over_e32": err / float(ref.e32[b]) if float(ref.e32[b]) > 0 else None})
            r = rows[-1]
            print(f"{case.name:15s}[{b}] {kernel:9s} live {str(r['live']):4s} nll_rel {0.0 if nll_rel is None else nll_rel:.1e} err {err:.2e} "
                  f"e32 {r['e32']:.2e} rw {r['random_walk']:.2e} bar {r['bar']:.2e} ratio {r['ratio']:.3f}")
            if r["ratio"] > worst.get(reg["kernel"], {"ratio": -1.0})["ratio"]:
                worst[reg["kernel"]] = {"ratio": r["ratio"], "case": case.name, "utterance": b}
    print("largest err / bar per regime:", worst)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"note": "max-abs gradient error per utterance of v100_ctc_loss against float64 (tests/_ctc_cases.py); "
                           "bar = max(2e-4, 2 e32, random_walk); e32 = torch's float32 CPU lattice against the same reference; "
                           "the max-abs ratio per utterance had not been measured before this record (relative L2 over a batch had)",
                   "device": torch.cuda.get_device_name(0), "largest_ratio_per_regime": worst, "utterances": rows}, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_oracle_errors.json"))
    a = ap.parse_args()
    per_utterance(a.out) if a.cases else batch_l2()
