"""bench.py's timed path on the GPU at its tiny configuration: --steps sets the number of timed steps, the line
carries ms_per_step, and --dump-outputs writes what the last timed step computed — the same from run to run, since
the inputs are pinned and every kernel of the step sums in a fixed order."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bench

pytestmark = pytest.mark.gpu


def test_dump_outputs_repeat_bit_for_bit(tmp_path):
    opt = SimpleNamespace(steps=3, warmup=1, zero1=False, dp_split=False, gnn_shard=False)
    cfg = dict(bench.CONFIGS['tiny'])
    wl = bench.workload(cfg, 'tiny')
    dev = torch.device('cuda', 0)
    lines = [bench.run_train(opt, cfg, 'tiny', 'fp32', wl, 1, 0, dev, dump=str(tmp_path / d)) for d in 'ab']
    for line in lines:
        assert line['steps'] == 3 and line['warmup'] == 1 and line['dtype'] == 'f32'
        assert line['ms_per_step'] > 0
        # value is the sequences of the timed steps over their time
        assert line['value'] == pytest.approx(cfg['B'] / (line['ms_per_step'] * 1e-3), rel=1e-3)
    names = sorted(p.name for p in (tmp_path / 'a').iterdir())
    assert names == ['grad.npy', 'loss.npy', 'loss_mi.npy', 'loss_rec.npy', 'params.npy']
    total = 0
    for n in names:
        a, b = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
        np.testing.assert_array_equal(a, b, err_msg=n)
        total += a.nbytes
    assert total <= 64 << 20
    assert float(np.load(tmp_path / 'a' / 'loss.npy')[0]) == pytest.approx(lines[0]['loss'], abs=1e-5)
    n_params = lines[0]['n_params']
    assert np.load(tmp_path / 'a' / 'params.npy').shape == (min(n_params, bench.DUMP_SAMPLE),)
    assert np.abs(np.load(tmp_path / 'a' / 'grad.npy')).max() > 0
