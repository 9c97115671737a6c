"""f2: the native data pipeline (c2dsr_amd/libc2dsr_prep.so, include/c2dsr_prep.h) is bit-exact with
the reference's processing — against the reference's own lists (tests/golden/data_*.npz), the
Food-Kitchen val file checksums (tests/golden/fk_data.npz, made by importing the reference) and the
Python restatement on synthetic files — and leaves Python's global `random` exactly where the
reference's draws would (so a following Python draw is the same)."""
import hashlib
import os
import random

import numpy as np
import pytest

from c2dsr_amd import dataloader as DL
from c2dsr_amd import graph as GR
from c2dsr_amd import prep, synth
from tests import goldens as G


def _raw(tmp_path, name='base'):
    d = G.load(f'data_{name}.npz')
    for mode in ('train', 'val', 'test'):
        (tmp_path / f'{mode}_new.txt').write_bytes(d[f'raw_{mode}'].tobytes())
    return d


def _eval_fields(seqs, last, neg):
    return [seqs[:, j] for j in range(6)] + [last[:, j:j + 1] for j in range(4)] + [neg]


def test_library_exports_every_declared_symbol():
    import ctypes
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                            'c2dsr_prep.h')).read()
    names = re.findall(r'\b(c2dsr_prep_\w+)\s*\(', hdr)
    L = ctypes.CDLL(prep.LIB_PATH)
    assert len(names) >= 7
    for n in names:
        assert hasattr(L, n), n


def test_native_lists_equal_reference_fixture(tmp_path):
    d = _raw(tmp_path)
    c = G.CONFIGS['base']
    random.seed(3407)  # main.py:91, then train / val / test datasets in this order
    tr = prep.RawFile(str(tmp_path / 'train_new.txt')).train_rows(c['n_a'], c['n_b'], c['len_max'])
    va = prep.RawFile(str(tmp_path / 'val_new.txt')).eval_rows(c['n_a'], c['n_b'], c['len_max'], G.N_NEG)
    te = prep.RawFile(str(tmp_path / 'test_new.txt')).eval_rows(c['n_a'], c['n_b'], c['len_max'], G.N_NEG)
    assert tr.shape[0] == int(d['n_train'])
    for j in range(14):
        np.testing.assert_array_equal(tr[:, j], d[f'train_{j}'], err_msg=f'train field {j}')
    for mode, r in (('val', va), ('test', te)):
        for j, f in enumerate(_eval_fields(*r)):
            np.testing.assert_array_equal(f, d[f'{mode}_{j}'], err_msg=f'{mode} field {j}')


@pytest.mark.parametrize('seed,n_a,n_b,L,n_neg', [(1, 40, 60, 8, 10), (2, 300, 500, 20, 99), (3, 5000, 9000, 15, 999),
                                                  (4, 9000, 5000, 30, 999), (5, 30, 35, 50, 12)])
def test_native_matches_python_restatement(tmp_path, seed, n_a, n_b, L, n_neg):
    """Both sample paths (pool for small populations, set rejection for 999 of ≥4117), ties in the
    timestamps, n_b < n_a (Q14's range(n_b - n_a) edge), dropped sequences, the RNG state after."""
    synth.make_dataset(str(tmp_path), n_a, n_b, L, 300, 200, seed=seed, ties=True, n_min=2)
    for mode in ('train', 'val'):
        fn = str(tmp_path / f'{mode}_new.txt')
        py_seqs = GR.read_sequences(fn)
        rf = prep.RawFile(fn)
        off, items = rf.sequences()
        assert [list(items[off[i]:off[i + 1]]) for i in range(rf.n_seq)] == py_seqs
        if mode == 'val' and n_b - n_a < n_neg + 1:
            continue  # the reference's sample would raise for domain-B rows (population too small)
        random.seed(1000 + seed)
        if mode == 'train':
            ref = DL.to_arrays(DL.preprocess_train(py_seqs, n_a, n_b, L))
        else:
            ref = DL.to_arrays(DL.preprocess_evaluate(py_seqs, n_a, n_b, L, n_neg))
        after_py = random.random()
        random.seed(1000 + seed)
        got = rf.train_rows(n_a, n_b, L) if mode == 'train' else rf.eval_rows(n_a, n_b, L, n_neg)
        after_native = random.random()
        fields = [got[:, j] for j in range(14)] if mode == 'train' else _eval_fields(*got)
        for j, (x, y) in enumerate(zip(fields, ref)):
            np.testing.assert_array_equal(x, y, err_msg=f'{mode} field {j}')
        assert after_native == after_py


def test_native_edges_match_python(tmp_path):
    synth.make_dataset(str(tmp_path), 700, 900, 30, 500, 10, seed=9, ties=True, n_min=2)
    fn = str(tmp_path / 'train_new.txt')
    s1, p1 = GR.transition_edges(GR.read_sequences(fn), 700)
    s2, p2 = prep.RawFile(fn).edges(700)
    np.testing.assert_array_equal(s1, s2)
    np.testing.assert_array_equal(p1, p2)


def test_native_food_kitchen_checksums(tmp_path):
    """tests/golden/fk_data.npz: the reference's processing of the real FK val file (as train and as
    eval data) and its graph; checked by sha256 like tests/test_dataprep.py.  The file's bytes are
    tests/golden/fk_val_new.npz."""
    fk = G.load('fk_data.npz')
    (tmp_path / 'val_new.txt').write_bytes(G.load('fk_val_new.npz')['val_new_txt'].tobytes())
    rf = prep.RawFile(str(tmp_path / 'val_new.txt'))
    random.seed(3407)
    tr = rf.train_rows(29207, 34886, 15)
    arr = np.stack([tr[:, j] for j in range(14)], axis=1)
    assert tuple(arr.shape) == tuple(fk['trainlike_shape'])
    assert hashlib.sha256(np.ascontiguousarray(arr).tobytes()).digest() == fk['trainlike_sha256'].tobytes()
    seqs, last, neg = rf.eval_rows(29207, 34886, 15, 999)
    flat = np.concatenate([np.concatenate([seqs[i].reshape(-1), last[i], neg[i]]) for i in range(len(neg))])
    assert hashlib.sha256(flat.tobytes()).digest() == fk['evallike_sha256'].tobytes()


def test_native_errors_are_reported(tmp_path):
    p = tmp_path / 'bad_new.txt'
    p.write_text('u1\t1\t3|5\tnot-a-field\n')
    with pytest.raises(ValueError, match='line 1'):
        prep.RawFile(str(p))
    with pytest.raises(FileNotFoundError):
        prep.RawFile(str(tmp_path / 'missing.txt'))
    q = tmp_path / 'long_new.txt'
    q.write_text('u1\t1\t' + '\t'.join(f'{i}|{i}' for i in range(12)) + '\n')
    with pytest.raises(ValueError, match='longer than len_max'):
        prep.RawFile(str(q)).train_rows(5, 20, 8)
