"""bench.py's command line (host only): a plain run measures the main line alone, --full switches the extra lines
and the CPU baseline on, and --dump-outputs writes float32 arrays — whole, or the same seeded sample every time."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bench


def test_plain_run_measures_the_main_line_only():
    opt = bench.parse_args(['--gpus', '1', '--steps', '7', '--warmup', '2'])
    assert (opt.steps, opt.warmup) == (7, 2)
    assert not opt.full and not opt.extra and opt.no_cpu_baseline and opt.dump_outputs is None


def test_full_turns_the_extras_and_the_cpu_baseline_on():
    opt = bench.parse_args(['--full'])
    assert opt.full and opt.extra and opt.c4_extra and opt.c5_extra and not opt.no_cpu_baseline
    opt = bench.parse_args(['--full', '--no-extra', '--no-cpu-baseline'])
    assert opt.full and not opt.extra and opt.no_cpu_baseline
    # the older switches alone do not bring anything back
    opt = bench.parse_args(['--no-cpu-baseline'])
    assert not opt.extra and opt.no_cpu_baseline


def test_dump_outputs_is_refused_for_the_kernel_roofline_run():
    with pytest.raises(SystemExit):
        bench.parse_args(['--config', 'c5', '--dump-outputs', 'x'])


def _flat(n):
    g = torch.Generator().manual_seed(1)
    return SimpleNamespace(numel=n, direct=True, param=torch.randn(n, generator=g),
                           accum=torch.randn(n, generator=g).double())


def test_dump_outputs_writes_float32_arrays(tmp_path):
    flat = _flat(1000)
    losses = (torch.tensor(3.5), torch.tensor(2.25, dtype=torch.float64), torch.tensor(1.25))
    bench.dump_outputs(str(tmp_path / 'o'), losses, flat)
    got = {p.name: np.load(p) for p in (tmp_path / 'o').iterdir()}
    assert sorted(got) == ['grad.npy', 'loss.npy', 'loss_mi.npy', 'loss_rec.npy', 'params.npy']
    assert all(a.dtype == np.float32 for a in got.values())
    assert [float(got[f'{k}.npy'][0]) for k in ('loss', 'loss_rec', 'loss_mi')] == [3.5, 2.25, 1.25]
    np.testing.assert_array_equal(got['params.npy'], flat.param.numpy())  # small stores are written whole
    np.testing.assert_array_equal(got['grad.npy'], flat.accum.float().numpy())


def test_dump_outputs_samples_a_large_store_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_SAMPLE', 64)
    flat = _flat(5000)
    losses = (torch.tensor(1.0),) * 3
    bench.dump_outputs(str(tmp_path / 'a'), losses, flat)
    bench.dump_outputs(str(tmp_path / 'b'), losses, flat)
    a, b = np.load(tmp_path / 'a' / 'params.npy'), np.load(tmp_path / 'b' / 'params.npy')
    assert a.shape == (64,)
    np.testing.assert_array_equal(a, b)
    idx = np.sort(np.random.default_rng(3407).integers(0, 5000, 64))
    np.testing.assert_array_equal(a, flat.param.numpy()[idx])
    np.testing.assert_array_equal(np.load(tmp_path / 'a' / 'grad.npy'), flat.accum.float().numpy()[idx])
    # without a whole accumulation (data parallel) only the parameters are written
    flat.direct = False
    bench.dump_outputs(str(tmp_path / 'c'), losses, flat)
    assert not (tmp_path / 'c' / 'grad.npy').exists() and (tmp_path / 'c' / 'params.npy').exists()
