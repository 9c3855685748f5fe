"""The WORLD statistics kernel (csrc/world_stat.hip, K19) and voice100_amd.calc_stat on the device, against the float64
restatement in tests/_world_stat_ref.py and the reference's own output (tests/golden/world_stat.npz).

Bound on every raw sum: |device - restatement| <= 2 n 2^-53 sum |term|, n the number of terms and sum |term| taken from the
restatement: both add the same exact float64 terms (an fp32 x fp32 product is exact in float64), each in an order of its own,
and each is within (n - 1) 2^-53 sum |term| of the exact sum to first order.  n <= 16000 gives <= 3.6e-12 relative to sum |term|.
Counts are exact.  Means and stds: 1e-9 relative -- that bound times E[x^2] / var <= 32 (asserted on the inputs) is 1.2e-10.
"""
import numpy as np
import pytest
import torch

import _world_stat_ref as R
from conftest import load_golden
from voice100_amd import _native as N
from voice100_amd.calc_stat import WORLDStat, calc_stat

pytestmark = pytest.mark.gpu

KEYS = ("f0_mean", "f0_std", "logspc_mean", "logspc_std", "codeap_mean", "codeap_std")
SHAPES = [(1, 1, 257, 1), (3, 40, 257, 1), (2, 57, 25, 1), (5, 129, 25, 1), (2, 33, 1, 1), (3, 40, 513, 2), (2, 19, 1024, 8),
          (16, 1000, 257, 1)]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def assert_moments(got, batches, S, A, what):
    mom, mag, terms = R.moments_ref(batches, S, A)
    got = got.detach().cpu()
    assert got.dtype == torch.float64 and got.shape == mom.shape
    assert got[2] == mom[2] and got[3] == mom[3], f"{what}: counts {got[2:4].tolist()} vs {mom[2:4].tolist()}"
    err, bnd = (got - mom).abs(), R.bound(mag, terms)
    ratio = float((err / bnd.clamp_min(1e-300)).max())
    print(f"{what}: largest error / bound {ratio:.3f} (largest bound / sum|term| {float((bnd / mag.clamp_min(1e-300)).max()):.2e})")
    worst = int(torch.argmax(err - bnd))
    assert bool((err <= bnd).all()), f"{what}: moment {worst}: got {got[worst]!r}, float64 {mom[worst]!r}, bound {bnd[worst]:.3e}"
    return mom


def to_dev(batch, dev):
    f0, lens, logspc, codeap = batch
    return f0.to(dev), lens.to(dev), logspc.to(dev), codeap.to(dev)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_raw_moments_against_the_restatement(cuda, shape):
    B, T, S, A = shape
    batch = R.make_batch(B, T, S, A, 1000 + B + T + S + A)
    stat = WORLDStat(S, A, device=cuda)
    assert stat.moments.is_cuda and not stat.moments.any()
    stat.update(*to_dev(batch, cuda))
    assert_moments(stat.moments, [batch], S, A, f"{shape}")


class _FakeData:
    def __init__(self, batches, S, A):
        import types
        self.audio_transform = types.SimpleNamespace(vocoder=types.SimpleNamespace(output_dims=(1, S, A)))
        self._batches = batches

    def predict_dataloader(self):
        return [((f0, lens, logspc, codeap), (None, None)) for f0, lens, logspc, codeap in self._batches]


@pytest.mark.parametrize("S", [257, 25])
def test_fixture_end_to_end_through_calc_stat(cuda, tmp_path, S):
    g = load_golden("world_stat.npz")
    batches = [tuple(torch.from_numpy(g[f"in/{S}/{i}/{k}"]) for k in ("f0", "f0_len", "logspc", "codeap")) for i in range(2)]
    mom, _, _ = R.moments_ref(batches, S, 1)
    spread = R.spread(mom, S, 1)
    assert max(spread.values()) <= 32.0, spread                  # what the 1e-9 below presupposes
    want = R.stats_ref(mom, S, 1)
    path = tmp_path / "audio_stat.pt"
    returned = calc_stat(_FakeData(batches, S, 1), str(path))        # CPU batches, as a data loader yields them
    saved = torch.load(str(path))
    assert tuple(saved) == KEYS == tuple(returned)
    for k in KEYS:
        v = saved[k]
        assert v.dtype == torch.float64 and v.device.type == "cpu" and v.shape == want[k].shape and torch.equal(v, returned[k])
        rel = float(((v - want[k]).abs() / want[k].abs()).max())
        fix = torch.from_numpy(g[f"expect/{S}/{k}"])
        gap = float(g[f"gap/{S}/{k}"])
        rel_fix = float(((v - fix).abs() / want[k].abs()).max())
        print(f"S={S} {k}: vs restatement {rel:.3e}, vs reference {rel_fix:.3e} (gap {gap:.3e})")
        assert rel <= 1e-9, (k, rel)
        assert rel_fix <= 4.0 * gap, (k, rel_fix, gap)


@pytest.mark.parametrize("shape", [(4, 40, 257, 1), (4, 57, 25, 2), (3, 1100, 25, 1)], ids=lambda s: "x".join(map(str, s)))
def test_padding_is_never_read(cuda, shape):
    B, T, S, A = shape
    lens = [T, 0, T // 3, 1][:B]
    f0, lens, logspc, codeap = R.make_batch(B, T, S, A, 77 + S, lens=lens)
    clean = WORLDStat(S, A, device=cuda)
    clean.update(*to_dev((f0, lens, logspc, codeap), cuda))
    assert_moments(clean.moments, [(f0, lens, logspc, codeap)], S, A, f"zero padded {shape}")
    pad = torch.arange(T)[None, :] >= lens[:, None]
    junk = torch.tensor([float("nan"), float("inf"), -float("inf")])
    f0n, lsn, can = f0.clone(), logspc.clone(), codeap.clone()
    f0n[pad] = junk[torch.arange(int(pad.sum())) % 3]
    lsn[pad] = junk[(torch.arange(int(pad.sum()) * S) % 3)].reshape(-1, S)
    can[pad] = junk[(torch.arange(int(pad.sum()) * A) % 3)].reshape(-1, A)
    dirty = WORLDStat(S, A, device=cuda)
    dirty.update(*to_dev((f0n, lens, lsn, can), cuda))
    assert torch.equal(bits(dirty.moments), bits(clean.moments))
    assert bool(torch.isfinite(dirty.moments).all())
    # device lengths beyond T are clamped by the kernel (CPU lengths like these are a ValueError); only full rows are comparable
    full = lens == T
    over = torch.where(full, torch.tensor(T + 1000), lens).to(torch.int32)
    over[int(torch.nonzero(full)[0])] = 2 ** 31 - 1
    clamped = WORLDStat(S, A, device=cuda)
    clamped.update(f0n.to(cuda), over.to(cuda), lsn.to(cuda), can.to(cuda))
    assert torch.equal(bits(clamped.moments), bits(clean.moments))
    negative = WORLDStat(S, A, device=cuda)                       # and below zero: an empty utterance
    negative.update(f0n.to(cuda), torch.where(lens == 0, torch.tensor(-5), lens).to(torch.int32).to(cuda), lsn.to(cuda), can.to(cuda))
    assert torch.equal(bits(negative.moments), bits(clean.moments))
    with pytest.raises(ValueError):
        clean.update(f0.to(cuda), over, logspc.to(cuda), codeap.to(cuda))


def test_nan_in_a_valid_frame(cuda):
    """NaN in a valid frame: propagates for logspc (that column only), fails both threshold tests for f0 and codeap."""
    B, T, S, A = 2, 23, 25, 2
    f0, lens, logspc, codeap = R.make_batch(B, T, S, A, 9, lens=[T, 11])
    f0[0, 3] = codeap[0, 4, 1] = logspc[1, 2, 7] = float("nan")
    stat = WORLDStat(S, A, device=cuda)
    stat.update(*to_dev((f0, lens, logspc, codeap), cuda))
    got = stat.moments.cpu()
    mom, mag, terms = R.moments_ref([(f0, lens, logspc, codeap)], S, A)
    nan = torch.isnan(got)
    assert torch.nonzero(nan).flatten().tolist() == [4 + 7, 4 + S + 7] and torch.equal(nan, torch.isnan(mom))
    assert got[2] == mom[2] and got[3] == mom[3] == T + 11
    assert bool(((got - mom).abs()[~nan] <= R.bound(mag, terms)[~nan]).all())


def test_thresholds_are_compared_in_fp32(cuda):
    lo = np.float32(-0.2)                                        # -0.2 rounded to fp32 lies BELOW the double -0.2:
    assert float(lo) < -0.2                                      # a comparison in double would count it
    ca_vals = [lo, np.nextafter(lo, np.float32(-1.0))]
    f0_vals = [np.float32(30.0), np.nextafter(np.float32(30.0), np.float32(100.0))]
    S = 3
    f0 = torch.tensor([f0_vals], dtype=torch.float32)
    codeap = torch.tensor([ca_vals], dtype=torch.float32)[:, :, None]
    logspc = torch.zeros(1, 2, S)
    stat = WORLDStat(S, 1, device=cuda)
    stat.update(f0.to(cuda), torch.tensor([2], device=cuda), logspc.to(cuda), codeap.to(cuda))
    m = stat.moments.cpu()
    assert m[2] == 1.0 and m[3] == 2.0
    assert m[0] == float(f0_vals[1]) and m[1] == float(f0_vals[1]) ** 2
    assert m[4 + 2 * S] == float(ca_vals[1]) and m[4 + 2 * S + 1] == float(ca_vals[1]) ** 2
    # torch's own comparison agrees (the restatement is built on it)
    assert (f0 > 30.0).tolist() == [[False, True]] and (codeap[:, :, 0] < -0.2).tolist() == [[False, True]]


def test_determinism_accumulation_and_launch_count(cuda):
    S, A = 257, 1
    batches = [R.make_batch(B, T, S, A, 40 + i) for i, (B, T) in enumerate(((3, 40), (2, 57), (4, 129)))]
    dev = [to_dev(b, cuda) for b in batches]
    runs = []
    for _ in range(2):
        stat = WORLDStat(S, A, device=cuda)
        for i, b in enumerate(dev):
            before = N.launch_count()
            stat.update(*b)
            assert N.launch_count() - before == 2, f"update {i}"
        runs.append(stat.moments.clone())
    assert torch.equal(bits(runs[0]), bits(runs[1]))
    mom = assert_moments(runs[0], batches, S, A, "three batches, one stat")
    total = torch.zeros_like(runs[0])
    for b in dev:
        one = WORLDStat(S, A, device=cuda)
        one.update(*b)
        total += one.moments
    _, mag, terms = R.moments_ref(batches, S, A)
    assert bool(((total.cpu() - runs[0].cpu()).abs() <= R.bound(mag, terms)).all())
    assert total[2].item() == mom[2].item() and total[3].item() == mom[3].item()
    # the same shape again reuses the cached partial buffer: still two launches, and the sums double
    again = WORLDStat(S, A, device=cuda)
    again.update(*dev[0])
    first = again.moments.clone()
    before = N.launch_count()
    again.update(*dev[0])
    assert N.launch_count() - before == 2 and len(again._partial) == 1
    assert torch.equal(bits(again.moments), bits(first + first))


def test_from_the_vocoder(cuda):
    from voice100_amd.vocoder import WORLDVocoder
    voc = WORLDVocoder(16000)
    rng = np.random.default_rng(5)
    lens = [4800, 3300]                                          # 0.3 s and 0.21 s
    x = np.zeros((2, lens[0]), dtype=np.float32)
    for b, (n, hz) in enumerate(zip(lens, (140.0, 210.0))):
        t = np.arange(n) / 16000.0
        x[b, :n] = 0.4 * np.sin(2 * np.pi * hz * t) + 0.2 * np.sin(4 * np.pi * hz * t) + 0.02 * rng.standard_normal(n)
    f0, feat, codeap = voc.encode_batch(torch.from_numpy(x).to(cuda), torch.tensor(lens, device=cuda))
    frames = torch.tensor([voc.frames(n) for n in lens])
    _, S, A = voc.output_dims
    assert f0.dtype == feat.dtype == codeap.dtype == torch.float32 and tuple(feat.shape) == (2, int(frames.max()), S)
    stat = WORLDStat(S, A, device=cuda)
    stat.update(f0, frames, feat, codeap)
    mom = assert_moments(stat.moments, [(f0.cpu(), frames, feat.cpu(), codeap.cpu())], S, A, "vocoder features")
    assert mom[3] == int(frames.sum())
    print(f"vocoder features: {int(mom[2])} voiced of {int(mom[3])} frames")
