#!/usr/bin/env python3
"""Generate tests/golden/world_stat.npz by CALLING the reference's calc_stat (voice100/calc_stat.py) on seeded batches.

Run in the build container only (needs the reference checkout; see make_golden.py for the stubs):

    python tests/golden/make_golden_stat.py

calc_stat.py imports voice100.data_modules only to annotate its argument; a placeholder module stands in for it (the real one
pulls in torchaudio and the text pipeline).  The `data` object is hand-made: `audio_transform.vocoder.output_dims` and a
`predict_dataloader()` that returns two padded batches, (2, 17) and (3, 9) frames, lengths in [1, T] with one full row, zero
padding -- once with S = 257 (log spectrum) and once with S = 25 (mel-cepstrum), A = 1, the two widths the reference accepts.
Written: the inputs, the six tensors the reference saved per S (expect/<S>/<key>), and gap/<S>/<key>, the largest relative
difference between those and the float64 restatement in tests/_world_stat_ref.py -- the size of the reference's own fp32
rounding, which the tests use as their tolerance towards the fixture.  Only data is written -- no reference source.
"""
import contextlib
import io
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, _install_stubs  # noqa: E402
import _world_stat_ref as R  # noqa: E402

SHAPES = ((2, 17), (3, 9))
# With ~45 frames the sample variance of one of 257 columns can fall well below the nominal 4, and the end-to-end test's bound
# presupposes E[x^2] / var <= 32 for every statistic: 20261028 is the first seed from 20261018 on whose batches satisfy that
# (asserted below).  A property of the inputs only; no output of the code under test went into the choice.
SEED = 20261028
KEYS = ("f0_mean", "f0_std", "logspc_mean", "logspc_std", "codeap_mean", "codeap_std")


def main():
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    _install_stubs()
    dm = types.ModuleType("voice100.data_modules")
    dm.AudioTextDataModule = object
    sys.modules["voice100.data_modules"] = dm
    from voice100.calc_stat import calc_stat
    torch.set_num_threads(1)

    out = {}
    for S in (257, 25):
        batches = [R.make_batch(B, T, S, 1, SEED + 100 * S + i) for i, (B, T) in enumerate(SHAPES)]
        for i, (f0, f0_len, logspc, codeap) in enumerate(batches):
            out.update({f"in/{S}/{i}/f0": f0.numpy(), f"in/{S}/{i}/f0_len": f0_len.numpy(),
                        f"in/{S}/{i}/logspc": logspc.numpy(), f"in/{S}/{i}/codeap": codeap.numpy()})
        data = types.SimpleNamespace(
            audio_transform=types.SimpleNamespace(vocoder=types.SimpleNamespace(output_dims=(1, S, 1))),
            predict_dataloader=lambda batches=batches: [((f0, l, ls, ca), (None, None)) for f0, l, ls, ca in batches])
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "audio_stat.pt")
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                calc_stat(data, path)
            saved = torch.load(path)
        assert tuple(saved) == KEYS
        mom, _, _ = R.moments_ref(batches, S, 1)
        want = R.stats_ref(mom, S, 1)
        for k in KEYS:
            v = saved[k]
            assert v.dtype == torch.float64 and tuple(v.shape) == tuple(want[k].shape)
            out[f"expect/{S}/{k}"] = v.numpy()
            out[f"gap/{S}/{k}"] = np.float64(((v - want[k]).abs() / want[k].abs()).max())
            print(S, k, tuple(v.shape), f"gap {out[f'gap/{S}/{k}']:.3e}")
        print(S, "E[x^2]/var", R.spread(mom, S, 1))
        assert max(R.spread(mom, S, 1).values()) <= 32.0
    path = os.path.join(HERE, "world_stat.npz")
    np.savez_compressed(path, **out)
    print("world_stat.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
