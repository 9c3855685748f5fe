"""Cases for the two hand-over forms of the CTC wave pipeline (csrc/ctc.hip: per frame / per group of frames): no GPU, no HIP.

CASES is the list of tests/test_gpu_ctc_group.py: every pipeline case of tests/_ctc_cases.py (at most 1024 lattice states), the
group's boundary lengths on 1, 2, 4 and 16 waves, and one case long enough to wrap the grouped form's ring more than twice.
rule() restates ctc_run's host rule; test_ctc_group_cpu.py holds it against the library and checks what the cases reach."""
import _ctc_cases as C

GROUP = 16           # frames per group (CTC_GROUP)
RING_FRAMES = 128    # the grouped ring: 8 groups (CTC_GRING)

# in_len of a single frame, around 8 (the per-frame form's prefetch group) and 16 (the group), and the whole padded length: one batch
BOUNDARY_IN_LEN = (1, 7, 8, 9, 15, 16, 17, 40)
# ... and around two, three and four groups
BOUNDARY2_IN_LEN = (15, 31, 32, 33, 47, 48, 49, 64)


def _boundary(seed, Lmax):
    """No label repeats its neighbour, so L labels fit L frames: row 5 (16 labels, 16 frames) has a single alignment.  Row 7 carries
    Lmax labels: every wave of the launch holds states; with more labels than its 40 frames it has no alignment (nll inf, zero
    gradient) while both lattices still run through their reachable states."""
    return C._case(seed, f"group_L{Lmax}", 8, 40, 29, Lmax, "norep", (1, 3, 4, 4, 7, 16, 8, Lmax), BOUNDARY_IN_LEN,
                   infeasible=(7,) if Lmax > 40 else ())


BOUNDARY = [
    _boundary(41, 31),       # Smax 63: one wave, no hand-over
    _boundary(42, 32),       # Smax 65: two waves, wave 1 holds a single state (row 7)
    _boundary(43, 100),      # Smax 201: four waves
    _boundary(44, 511),      # Smax 1023: 16 waves
]
# the second batch on four waves: rows 3 - 7 are feasible and reach into wave 1 or 2, row 7 (64 labels, 64 frames) has a single alignment
BOUNDARY.append(C._case(46, "group2_L100", 8, 64, 29, 100, "norep", (7, 100, 16, 33, 40, 48, 20, 64), BOUNDARY2_IN_LEN, infeasible=(1,)))
# two waves, both full of live states on row 0, T = 2.25 rings: slots are reused twice, back-pressure tests at every half ring
RING_WRAP = C._case(45, "group_ring_wrap", 2, 288, 29, 60, "norep", (60, 33), (288, 261))
PIPELINE = [c for c in C.CASES if 2 * c.Lmax + 1 <= 1024]
CASES = PIPELINE + BOUNDARY + [RING_WRAP]


def waves(case):
    return (2 * case.Lmax + 1 + 63) // 64


def rule(T, nw):
    """ctc_run's choice for the pipeline: True = grouped.  The grouped form pays a longer fill per downstream wave."""
    return T >= 32 + 4 * nw
