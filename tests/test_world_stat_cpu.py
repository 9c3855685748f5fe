"""CPU-side checks of the WORLD statistics (voice100_amd/calc_stat.py, csrc/world_stat.hip): the float64 restatement against the
reference's own output (tests/golden/world_stat.npz, written by make_golden_stat.py), WORLDStat.state_dict against the
restatement, what update refuses, and the host-side half of the two C entry points.  Nothing here launches a kernel.

Tolerance towards the fixture: 4 x gap per key, gap being the largest relative difference the generator measured between the
reference's output and the restatement -- the reference's own fp32 rounding of products and per-batch sums (3e-8 ... 3e-6, the
largest on logspc_std: fp32's 6e-8 amplified by E[x^2] / var); the factor 4 is for another torch build's reduction order.
"""
import ctypes
import os

import pytest
import torch

import _world_stat_ref as R
from conftest import load_golden

KEYS = ("f0_mean", "f0_std", "logspc_mean", "logspc_std", "codeap_mean", "codeap_std")


@pytest.fixture(scope="module")
def golden():
    return load_golden("world_stat.npz")


def fixture_batches(g, S):
    return [tuple(torch.from_numpy(g[f"in/{S}/{i}/{k}"]) for k in ("f0", "f0_len", "logspc", "codeap")) for i in range(2)]


@pytest.fixture(scope="module")
def lib():
    from voice100_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return N.load()


@pytest.mark.parametrize("S", [257, 25])
def test_restatement_matches_the_reference_output(golden, S):
    batches = fixture_batches(golden, S)
    assert [tuple(b[0].shape) for b in batches] == [(2, 17), (3, 9)]
    for f0, f0_len, _, _ in batches:
        assert int(f0_len.min()) >= 1 and int(f0_len.max()) == f0.shape[1]
    mom, _, _ = R.moments_ref(batches, S, 1)
    got = R.stats_ref(mom, S, 1)
    for k in KEYS:
        want = torch.from_numpy(golden[f"expect/{S}/{k}"])
        gap = float(golden[f"gap/{S}/{k}"])
        assert want.dtype == torch.float64 and got[k].shape == want.shape
        err = float(((got[k] - want).abs() / got[k].abs()).max())
        print(f"S={S} {k}: restatement vs reference {err:.3e}, gap {gap:.3e}")
        assert 0.0 < gap < 1e-5, k                               # fp32 rounding, not a disagreement about the formula
        assert err <= 4.0 * gap, (k, err, gap)


@pytest.mark.parametrize("S,A", [(257, 1), (25, 1), (513, 2)])
def test_state_dict_from_cpu_moments(S, A):
    from voice100_amd.calc_stat import WORLDStat
    from voice100_amd import tts, tts_v2
    batches = [R.make_batch(3, 11, S, A, 5 + S), R.make_batch(2, 7, S, A, 6 + S)]
    mom, _, _ = R.moments_ref(batches, S, A)
    stat = WORLDStat(S, A, device="cpu")
    assert stat.moments.dtype == torch.float64 and tuple(stat.moments.shape) == (4 + 2 * S + 2 * A,) and not stat.moments.any()
    stat.moments += mom
    sd = stat.state_dict()
    want = R.stats_ref(mom, S, A)
    assert tuple(sd) == KEYS
    for k, shape in zip(KEYS, ((1,), (1,), (S,), (S,), (A,), (A,))):
        assert sd[k].dtype == torch.float64 and sd[k].device.type == "cpu" and tuple(sd[k].shape) == shape, k
        assert bool(torch.isfinite(sd[k]).all())
        assert float(((sd[k] - want[k]).abs() / want[k].abs()).max()) <= 1e-12, k
    # codeap over the FRAME count, not over its own elements
    assert torch.equal(sd["codeap_mean"], mom[4 + 2 * S:4 + 2 * S + A] / mom[3])
    for norm_cls in (tts.WORLDNorm, tts_v2.WORLDNorm):
        norm = norm_cls(S, A)
        norm.load_state_dict(sd, strict=True)
        assert torch.equal(norm.logspc_std, sd["logspc_std"].float())
    # shards add
    a, b = WORLDStat(S, A, device="cpu"), WORLDStat(S, A, device="cpu")
    a.moments += R.moments_ref(batches[:1], S, A)[0]
    b.moments += R.moments_ref(batches[1:], S, A)[0]
    a.moments += b.moments
    _, mag, terms = R.moments_ref(batches, S, A)
    assert bool(((a.moments - mom).abs() <= R.bound(mag, terms)).all())       # another association of the same float64 terms


def test_zero_counts_give_nan():
    from voice100_amd.calc_stat import WORLDStat
    sd = WORLDStat(25, 1, device="cpu").state_dict()
    assert all(bool(torch.isnan(v).all()) for v in sd.values()) and tuple(sd) == KEYS
    stat = WORLDStat(3, 2, device="cpu")                         # frames, but no voiced one: only f0 is NaN
    stat.moments[3] = 4.0
    stat.moments[4:7] = torch.tensor([4.0, 8.0, -4.0])
    stat.moments[7:10] = torch.tensor([8.0, 32.0, 8.0])
    sd = stat.state_dict()
    assert bool(torch.isnan(sd["f0_mean"]).all()) and bool(torch.isnan(sd["f0_std"]).all())
    assert sd["logspc_mean"].tolist() == [1.0, 2.0, -1.0] and sd["logspc_std"].tolist() == [1.0, 2.0, 1.0]
    assert sd["codeap_mean"].tolist() == [0.0, 0.0] and sd["codeap_std"].tolist() == [0.0, 0.0]


def test_update_has_no_cpu_fallback_and_checks_its_arguments():
    from voice100_amd.calc_stat import WORLDStat, calc_stat  # noqa: F401
    S, A = 25, 2
    stat = WORLDStat(S, A, device="cpu")
    f0, lens, logspc, codeap = R.make_batch(2, 6, S, A, 3)
    with pytest.raises(RuntimeError):
        stat.update(f0, lens, logspc, codeap)
    assert not stat.moments.any()
    for bad in ([7, 1], [-1, 6], torch.tensor([6, 9])):
        with pytest.raises(ValueError):
            stat.update(f0, bad, logspc, codeap)
    with pytest.raises(ValueError):
        stat.update(f0, [6, 6, 6], logspc, codeap)               # [B] lengths
    with pytest.raises(ValueError):
        stat.update(f0, lens, logspc[:, :, :24], codeap)         # logspc.shape[2] != logspc_size
    with pytest.raises(ValueError):
        stat.update(f0, lens, logspc, codeap[:, :, :1])
    with pytest.raises(ValueError):
        stat.update(f0, lens, logspc[:, :5], codeap)
    with pytest.raises(ValueError):
        stat.update(f0.double(), lens, logspc, codeap)
    for S_, A_ in ((0, 1), (1025, 1), (25, 0), (25, 9)):
        with pytest.raises(ValueError):
            WORLDStat(S_, A_, device="cpu")


def test_entry_points_host_side(lib):
    parts = lib.v100_world_stat_parts
    for B, T, S in ((1, 1, 257), (16, 1000, 257), (16, 1000, 25), (256, 1000, 257), (3, 40, 513), (2, 19, 1024), (2, 33, 1), (5000, 7, 25)):
        n = parts(B, T, S)
        assert n >= B and n % B == 0 and n // B <= T, (B, T, S, n)           # whole chunks per utterance, none empty by construction
        assert n <= max(B, 1024)
    assert parts(16, 1000, 257) > 16                               # an utterance is split while the batch is small
    for bad in ((0, 10, 25), (2, 0, 25), (2, 10, 0), (2, 10, 1025), (-1, 10, 25)):
        assert parts(*bad) == -1
    one = ctypes.c_void_p(16)
    accum = lib.v100_world_stat_accum
    ok = (one, one, one, one, one, one)
    for i in range(6):                                             # every pointer is required
        args = list(ok)
        args[i] = None
        assert accum(*args, 2, 10, 25, 1, None) == 3
    for B, T, S, A in ((0, 10, 25, 1), (2, 0, 25, 1), (2, 10, 0, 1), (2, 10, 1025, 1), (2, 10, 25, 0), (2, 10, 25, 9), (-2, 10, 25, 1)):
        assert accum(*ok, B, T, S, A, None) == 1
    assert accum(None, one, one, one, one, one, 2, 10, 1025, 1, None) == 3
