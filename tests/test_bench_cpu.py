"""bench.py's host-side pieces that need no GPU: the option surface of a plain / --full
run and the --dump-outputs writer (float32 files, a fixed seeded sample when an array
is over its share of the size limit)."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def test_options_of_a_plain_and_a_full_run():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True,
                         check=True).stdout
    for opt in ('--gpus', '--steps', '--warmup', '--dump-outputs', '--full'):
        assert opt in out, opt


def test_dump_outputs_writes_float32_and_samples_reproducibly(tmp_path, monkeypatch):
    bench = _bench()
    g = torch.Generator().manual_seed(7)
    model = types.SimpleNamespace(flat_grad=torch.randn(5000, generator=g), flat_params=torch.randn(5000, generator=g))
    nll = torch.randn(28, generator=g, dtype=torch.float64)

    bench.dump_outputs(str(tmp_path / 'a'), nll, model)
    assert sorted(os.listdir(tmp_path / 'a')) == ['grad.npy', 'nll.npy']
    for name, t in (('nll', nll), ('grad', model.flat_grad)):
        a = np.load(tmp_path / 'a' / f'{name}.npy')
        assert a.dtype == np.float32 and a.shape == (t.numel(),)
        np.testing.assert_array_equal(a, t.to(torch.float32).numpy())

    # two files within 64 KiB of headers + 2 * 1000 floats: the 5000-element array is sampled
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', (1 << 16) + 2 * 4 * 1000)
    bench.dump_outputs(str(tmp_path / 'b'), nll, model)
    bench.dump_outputs(str(tmp_path / 'c'), nll, model)
    total = 0
    for name in ('nll', 'grad'):
        b, c = np.load(tmp_path / 'b' / f'{name}.npy'), np.load(tmp_path / 'c' / f'{name}.npy')
        np.testing.assert_array_equal(b, c)
        total += os.path.getsize(tmp_path / 'b' / f'{name}.npy')
    assert total <= bench.DUMP_MAX_BYTES
    b = np.load(tmp_path / 'b' / 'grad.npy')
    assert b.shape == (1000,) and np.isin(b, model.flat_grad.numpy()).all()
    np.testing.assert_array_equal(np.load(tmp_path / 'b' / 'nll.npy'), nll.to(torch.float32).numpy())
