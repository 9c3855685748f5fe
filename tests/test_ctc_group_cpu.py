"""The host rule that picks the hand-over form of the CTC wave pipeline (csrc/ctc.hip, ctc_lattice_grouped), restated in
tests/_ctc_group_cases.py and held against the library's own answer (v100_ctc_lattice_plan: host only), and what the cases of
tests/test_gpu_ctc_group.py reach.  No GPU."""
import torch

import _ctc_cases as C
import _ctc_group_cases as G
from voice100_amd import _native as N


def _plan(T, Lmax):
    return int(N.load().v100_ctc_lattice_plan(T, Lmax))


def test_the_rule_is_the_librarys():
    assert int(N.load().v100_ctc_lattice_ring_frames()) == G.RING_FRAMES and G.RING_FRAMES % G.GROUP == 0
    for Lmax in (0, 1, 31, 32, 63, 64, 100, 255, 256, 511):
        nw = (2 * Lmax + 1 + 63) // 64
        for T in list(range(1, 100)) + [512, 640, 4096]:
            assert _plan(T, Lmax) == (G.GROUP if G.rule(T, nw) else 0), (T, Lmax)
    assert [min(T for T in range(1, 100) if G.rule(T, nw)) for nw in (1, 2, 4, 8, 16)] == [36, 40, 48, 64, 96]
    assert _plan(512, 512) == -1 and _plan(512, 2047) == -1            # more than 1024 states: the barrier kernels
    assert _plan(0, 10) == -1 and _plan(8, -1) == -1
    assert _plan(512, 100) == G.GROUP                                   # the benchmark's shape: 4 waves over 512 frames


def test_the_hook_takes_three_values_and_leaves_the_plan_alone():
    lib = N.load()
    assert lib.v100_ctc_lattice_form(2) == 1 and lib.v100_ctc_lattice_form(-2) == 1
    try:
        for form in (0, 1):
            assert lib.v100_ctc_lattice_form(form) == 0
            assert _plan(40, 511) == 0 and _plan(640, 511) == G.GROUP   # the plan is the rule, whatever is forced
    finally:
        assert lib.v100_ctc_lattice_form(-1) == 0


def test_both_forms_are_reached_by_the_rule():
    chosen = {c.name: G.rule(c.T, G.waves(c)) for c in G.CASES}
    assert all(_plan(c.T, c.Lmax) == (G.GROUP if chosen[c.name] else 0) for c in G.CASES)
    assert chosen["skew16_full"] and not chosen["skew16_idle"]          # 16 waves: long rows grouped, 40 frames per frame
    assert chosen["group_L31"] and chosen["group_L32"] and not chosen["group_L100"] and not chosen["group_L511"]
    assert chosen["group2_L100"] and chosen["group_ring_wrap"]
    assert {G.waves(c) for c in G.CASES if chosen[c.name]} >= {1, 2, 4, 16}
    assert {G.waves(c) for c in G.CASES if not chosen[c.name]} >= {4, 16}


def test_what_the_cases_reach():
    assert {c.name for c in G.PIPELINE} == {c.name for c in C.CASES if C.regime(c)["kernel"] == "skew"} and len(G.PIPELINE) >= 10
    assert len({c.name for c in G.CASES}) == len(G.CASES)
    # the boundary batch: one frame, one under / at / one over 8 and one group, the whole length; 1, 2, 4 and 16 waves
    assert G.BOUNDARY_IN_LEN == (1, 7, 8, 9, G.GROUP - 1, G.GROUP, G.GROUP + 1, 40)
    assert {k * G.GROUP + d for k in (2, 3) for d in (-1, 0, 1)} | {4 * G.GROUP} <= set(G.BOUNDARY2_IN_LEN)
    assert [G.waves(c) for c in G.BOUNDARY] == [1, 2, 4, 16, 4]
    for c in G.BOUNDARY:
        ref = C.reference(c)
        for b in range(c.B):
            assert (float(ref.nll64[b]) == float("inf")) == (b in c.infeasible), (c.name, b)
    for c in G.BOUNDARY[:4]:
        assert (c.B, c.T, c.V) == (8, 40, 29) and c.in_len == G.BOUNDARY_IN_LEN and c.tgt_len[7] == c.Lmax
    assert 2 * G.BOUNDARY[1].Lmax + 1 == 65                             # a last wave with a single state
    # rows without a frame, and rows shorter than a group on 16 waves, come with the pipeline cases
    assert any(n == 0 for c in G.PIPELINE for n in c.in_len)
    assert {1, 8, 37} <= {n for c in G.PIPELINE if G.waves(c) == 16 for n in c.in_len}
    assert any(n % G.GROUP for c in G.CASES for n in c.in_len)
    # ring wrap: two waves, both holding states of a feasible row, at least twice the ring's capacity in frames
    w = G.RING_WRAP
    assert G.waves(w) == 2 and min(w.in_len) >= 2 * G.RING_FRAMES and 2 * w.tgt_len[0] + 1 > 64
    assert bool(torch.isfinite(C.reference(w).nll64).all())
