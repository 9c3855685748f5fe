"""The case list of tests/_ctc_cases.py reaches what tests/test_gpu_ctc_oracle.py relies on it to reach, and its float64 reference
meets the closed forms that exist.  No GPU: everything here is torch on the CPU."""
import pytest
import torch

import _ctc_cases as C

CLOSED_FORM = 1e-12


def _regimes(kernel):
    return [(c, C.regime(c)) for c in C.CASES if C.regime(c)["kernel"] == kernel]


def test_names_are_unique_and_lengths_fit():
    assert len(C.BY_NAME) == len(C.CASES)
    for c in C.CASES:
        logits, labels = C.inputs(c)
        assert logits.shape == (c.B, c.T, c.V) and labels.shape == (c.B, c.Lmax) and logits.dtype == torch.float32
        assert max(c.tgt_len) == c.Lmax or c.name == "skew16_idle"        # (that case is about a wide launch over short rows)
        assert 0 <= c.blank < c.V and c.Lmax <= 2047 and c.V <= 128


def test_label_modes():
    for c in C.CASES:
        _, labels = C.inputs(c)
        eq = labels[:, 1:] == labels[:, :-1]
        if c.mode == "norep":
            assert not bool(eq.any()), c.name
        if c.mode == "same":
            assert bool(eq.all()), c.name


def test_every_wave_and_slot_carries_a_state_somewhere():
    skew, l8, l16 = _regimes("skew"), _regimes("lattice8"), _regimes("lattice16")
    live = lambda group: {v for _, r in group for v in r["live"] if v is not None}      # noqa: E731
    assert 15 in live(skew) and 7 in live(l8) and 15 in live(l16)
    assert {1, 2, 16} <= {r["waves"] for _, r in skew}
    # a full launch holds a feasible row: enough frames for every state to be reachable
    for group, top in ((skew, 15), (l8, 7), (l16, 15)):
        assert any(v == top and n >= c.tgt_len[b] for c, r in group for b, (v, n) in enumerate(zip(r["live"], c.in_len)) if v is not None)
    # the regime edges: Smax 63 / 65, 1023 / 1025, 2047 / 2049 and the kernel's limit 4095
    assert {63, 65, 1023, 1025, 2047, 2049, 4095} <= {C.regime(c)["Smax"] for c in C.CASES}
    assert C.regime(C.BY_NAME["edge_512"])["live"][0] == 4 and C.regime(C.BY_NAME["edge_1024"])["live"][0] == 8


def test_both_launches_above_64_kib_and_one_below():
    l16 = _regimes("lattice16")
    big = {r["Smax"] for c, r in l16 if r["lds_attribute"]}
    assert big == {4093, 4095}
    assert all(c.V == 128 for c, r in l16 if r["lds_attribute"])
    assert any(not r["lds_attribute"] and r["Smax"] == 4095 for _, r in l16)
    assert all(not r["lds_attribute"] for _, r in _regimes("lattice8"))
    # no other (V, Lmax) within the kernel's limits needs the attribute
    need = {(V, L) for V in range(1, 129) for L in range(512, 2048) if (C.CTC_CHUNK * V + 2 * (2 * L + 1 + 4)) * 4 > C.LDS_STATIC_MAX}
    assert need == {(128, 2046), (128, 2047)}


def test_layout_route_sees_ragged_blocks_and_the_class_limit():
    """The [B, V, T] gradient kernel takes 16 frames a workgroup."""
    rows = {c.name: c.B * c.T for c in C.CASES}
    assert rows["skew16_idle"] == 160 and rows["blank_last"] == 210 and rows["edge_31"] == 200
    assert sum(1 for n in rows.values() if n % 16) >= 3 and any(c.V == 128 for c in C.CASES)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_feasibility_and_yardstick(case):
    ref = C.reference(case)
    for b in range(case.B):
        if b in case.infeasible:
            assert ref.nll64[b] == float("inf"), b
            assert not bool(ref.G64[b].any())
        else:
            assert bool(torch.isfinite(ref.nll64[b])), b
    assert bool(torch.isfinite(ref.e32).all()) and bool(torch.isfinite(ref.G64).all())
    assert float(ref.G64.abs().max()) <= 1.0 + 1e-12
    for b, n in enumerate(case.in_len):
        assert not bool(ref.G64[b, n:].any()), b                           # padded frames
    bar = C.grad_bar(case, ref)
    assert bool((bar >= 2e-4).all()) and bool((bar >= C.random_walk_term(case, ref)).all()) and float(bar.max()) < 4e-2
    # 'mean' is the per-utterance losses over max(len, 1), infeasible rows as zero
    tl = torch.tensor(case.tgt_len, dtype=torch.float64).clamp_min(1)
    want = float((torch.where(torch.isfinite(ref.nll64), ref.nll64, torch.zeros_like(ref.nll64)) / tl).mean())
    assert abs(ref.mean64 - want) <= CLOSED_FORM * max(1.0, abs(want))


def test_bars_stay_far_below_a_structural_error():
    """A mishandled wave edge, slot or chunk makes errors of 0.1 to 1 in a gradient whose entries lie in [-1, 1]: the bars are 2e-4 to
    4e-4 on every case of at most 120 frames and stay under 4e-2 at the kernel's limit (Lmax 2047, nll 1.3e4)."""
    for c in C.CASES:
        bar = C.grad_bar(c, C.reference(c))
        assert float(bar.max()) <= (4e-4 if c.T <= 120 else 4e-2), c.name


@pytest.mark.parametrize("name,row", C.SINGLE_ALIGNMENT)
def test_single_alignment_rows(name, row):
    case = C.BY_NAME[name]
    ref = C.reference(case)
    logits, _ = C.inputs(case)
    n = case.in_len[row]
    path = torch.tensor(C.single_alignment_path(case, row))
    lp = torch.log_softmax(logits[row, :n].double(), -1)
    nll = -float(lp[torch.arange(n), path].sum())
    assert abs(float(ref.nll64[row]) - nll) <= CLOSED_FORM * abs(nll)
    G = lp.exp()
    G[torch.arange(n), path] -= 1.0
    assert float((ref.G64[row, :n] - G).abs().max()) <= CLOSED_FORM
    assert not bool(ref.G64[row, n:].any())


def test_empty_targets():
    seen = 0
    for case in C.CASES:
        ref = C.reference(case)
        logits, _ = C.inputs(case)
        for b, (L, n) in enumerate(zip(case.tgt_len, case.in_len)):
            if L:
                continue
            seen += 1
            lp = torch.log_softmax(logits[b, :n].double(), -1)
            nll = -float(lp[:, case.blank].sum())
            assert abs(float(ref.nll64[b]) - nll) <= CLOSED_FORM * max(1.0, abs(nll)), (case.name, b)
            G = lp.exp()
            G[:, case.blank] -= 1.0
            assert n == 0 or float((ref.G64[b, :n] - G).abs().max()) <= CLOSED_FORM, (case.name, b)
            assert not bool(ref.G64[b, n:].any())
    assert seen >= 5
    mix = C.BY_NAME["infeasible_mix"]
    assert mix.in_len[2] == 0 and mix.tgt_len[2] == 0 and float(C.reference(mix).nll64[2]) == 0.0      # no frame, no label: nll 0
