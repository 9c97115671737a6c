"""Full-catalogue top-K recommendation and full-ranking evaluation (csrc/topk.hip, ops.full_topk / ops.eval_query,
Trainer.full_ranks / evaluate_full / recommend) against int64 / float64 computations on the CPU.

Exact-integer data (every value and partial sum exact in hi/lo bf16 and fp32) is checked with torch.equal, ties
ordered by ascending id; float data with the band 5e-5 · max_j |s64(i, j)| per row (the split-bf16 tolerance TOL of
tests/test_gpu_ce3.py)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BAND = 5e-5


def _run(q, W, b, k, **kw):
    from c2dsr_amd import ops
    kw = {key: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for key, v in kw.items()}
    ids, scores, rank = ops.full_topk(q.to(DEV), W.to(DEV), b.to(DEV), k, **kw)
    return ids.cpu(), scores.cpu(), None if rank is None else rank.cpu()


def _int_data(M, n, d, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-3, 4, (M, d), generator=g)
    W = torch.randint(-3, 4, (n, d), generator=g)
    b = torch.randint(-5, 6, (n,), generator=g)
    t = torch.randint(0, n, (M,), generator=g)
    return q, W, b, t


def _int_expect(q, W, b, k, t=None, exclude=None):
    """int64 scores → (ids, scores fp32, rank): score descending, id ascending among equal scores (stable sort)."""
    s = q.long() @ W.long().T + b.long()[None, :]
    rank = None
    if t is not None:
        rank = (1 + (s > s.gather(1, (t % s.shape[1])[:, None])).sum(1)).int()
    low = s.min() - 1
    sel = s.clone()
    if exclude is not None:
        n = s.shape[1]
        for i in range(s.shape[0]):
            e = exclude[i]
            sel[i, e[(e >= 0) & (e < n)]] = low
    val, idx = torch.sort(sel, dim=1, descending=True, stable=True)
    val, idx = val[:, :k], idx[:, :k].clone()
    out = val.float()
    gone = val == low
    idx[gone] = -1
    out[gone] = float('-inf')
    return idx, out, rank


# ---------------------------------------------------------------- 1. exact integers
@pytest.mark.parametrize('M,n,d,k,n_split', [(1, 129, 16, 1, 1), (33, 1000, 30, 5, 2), (130, 4099, 64, 20, 3),
                                             (300, 5000, 256, 128, 4), (64, 128, 128, 128, 1)])
def test_exact_integers(M, n, d, k, n_split):
    q, W, b, t = _int_data(M, n, d, seed=M + n + d + k)
    ids, scores, rank = _run(q.float(), W.float(), b.float(), k, target=t, n_split=n_split)
    eids, escores, erank = _int_expect(q, W, b, k, t)
    assert torch.equal(rank, erank)
    assert torch.equal(scores, escores)
    assert torch.equal(ids, eids)


# ---------------------------------------------------------------- 2. adversarial order
@pytest.mark.parametrize('n_split', [1, 3])
@pytest.mark.parametrize('k', [1, 20, 128])
def test_adversarial_order(k, n_split):
    n, d, M = 5000, 64, 3
    q = torch.zeros(M, d)
    q[:, 0] = 1
    b = torch.zeros(n)
    t = torch.tensor([0, n // 2, n - 1])
    j = torch.arange(n)
    for col in (j, n - j, torch.full((n,), 7)):  # ascending (every column beats the threshold), descending, equal
        W = torch.zeros(n, d)
        W[:, 0] = col.float()
        W[:, 1] = 2.0  # multiplied by q's zero
        ids, scores, rank = _run(q, W, b, k, target=t, n_split=n_split)
        eids, escores, erank = _int_expect(q.long(), W.long(), b.long(), k, t)
        assert torch.equal(ids, eids) and torch.equal(scores, escores) and torch.equal(rank, erank)
    # every W row the same random float vector: all n columns, the targets' pre-pass included, must give one bit
    # pattern per row — ids 0..k-1, no column above any target
    g = torch.Generator().manual_seed(k + n_split)
    q = torch.randn(M, d, generator=g)
    W = torch.randn(1, d, generator=g).expand(n, d).contiguous()
    b = torch.full((n,), 0.37)
    ids, scores, rank = _run(q, W, b, k, target=t, n_split=n_split)
    assert torch.equal(ids, torch.arange(k).expand(M, k))
    assert torch.equal(rank, torch.ones(M, dtype=torch.int32))
    assert bool((scores == scores[:, :1]).all())


# ---------------------------------------------------------------- 3. float data vs float64
FLOAT_SHAPES = [(300, 5000, 256, 20), (33, 1000, 64, 128), (130, 4099, 128, 5), (64, 777, 30, 20)]


@functools.lru_cache(maxsize=None)
def _float_case(M, n, d):
    """Inputs scaled as in tests/test_gpu_eval.py::test_eval_rank_kernel_large, and their float64 scores."""
    g = torch.Generator().manual_seed(M + n + d)
    q = torch.randn(M, d, generator=g) + torch.randn(M, d, generator=g)
    W = torch.randn(n, d, generator=g) * 0.1
    b = torch.randn(n, generator=g)
    t = (torch.rand(M, generator=g) * n).long()
    s64 = q.double() @ W.double().T + b.double()[None, :]
    return q, W, b, t, s64


def _check_band(ids, scores, rank, s64, t, k):
    M, n = s64.shape
    band = BAND * s64.abs().max(1).values  # [M]
    assert bool(((ids >= 0) & (ids < n)).all())
    srt = torch.sort(ids, dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), 'ids not distinct'
    assert bool((scores[:, 1:] <= scores[:, :-1]).all()), 'scores not non-increasing'
    got64 = s64.gather(1, ids)
    err = (scores.double() - got64).abs()
    print('worst score error / band:', float((err / band[:, None]).max()))
    assert bool((err <= band[:, None]).all())
    kth = torch.sort(s64, dim=1, descending=True).values[:, k - 1]
    assert bool((got64 >= (kth - band)[:, None]).all()), 'an id below the k-th boundary band'
    must = s64 > (kth + band)[:, None]
    have = torch.zeros(M, n, dtype=torch.bool)
    have.scatter_(1, ids, True)
    assert bool((have | ~must).all()), 'an item above the k-th boundary band is missing'
    if rank is not None:
        sg = s64.gather(1, t[:, None])
        lo = 1 + (s64 > sg + band[:, None]).sum(1)
        notme = torch.ones(M, n, dtype=torch.bool)
        notme.scatter_(1, t[:, None], False)
        hi = 1 + ((s64 > sg - band[:, None]) & notme).sum(1)
        assert bool(((lo <= rank) & (rank <= hi)).all()), (rank, lo, hi)


@pytest.mark.parametrize('M,n,d,k', FLOAT_SHAPES)
def test_float_vs_float64(M, n, d, k):
    q, W, b, t, s64 = _float_case(M, n, d)
    ids, scores, rank = _run(q, W, b, k, target=t)
    _check_band(ids, scores, rank, s64, t, k)


# ---------------------------------------------------------------- 4. determinism
def test_bitwise_independent_of_split_and_run():
    M, n, d, k = FLOAT_SHAPES[0]
    q, W, b, t, _ = _float_case(M, n, d)
    ref = _run(q, W, b, k, target=t, n_split=1)
    for ns in (2, 5, 5):
        got = _run(q, W, b, k, target=t, n_split=ns)
        for a, e in zip(got, ref):
            assert torch.equal(a, e), ns
        assert torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32)), ns


# ---------------------------------------------------------------- 5. exclusion and row filter
def test_exclusion():
    M, n, d, k, E = 130, 300, 64, 20, 50
    q, W, b, t = _int_data(M, n, d, seed=5)
    g = torch.Generator().manual_seed(55)
    ex = torch.randint(-20, n + 20, (M, E), generator=g)  # entries outside [0, n) are padding
    ex[:, 0] = _int_expect(q, W, b, 1)[0][:, 0]  # each row's best item is excluded
    ex[::7, 1] = t[::7]  # excluding the target does not change its rank
    ids, scores, rank = _run(q.float(), W.float(), b.float(), k, target=t, exclude=ex, n_split=2)
    eids, escores, erank = _int_expect(q, W, b, k, t, exclude=ex)
    assert torch.equal(ids, eids) and torch.equal(scores, escores)
    assert torch.equal(rank, erank)
    assert not bool((ids[:, :, None] == ex[:, None, :]).any())
    assert torch.equal(rank, _run(q.float(), W.float(), b.float(), k, target=t, n_split=2)[2])
    # fewer than k items left: the tail is (-1, -inf)
    n2 = 60
    W2, b2 = W[:n2], b[:n2]
    ex2 = torch.stack([torch.randperm(n2, generator=g)[:E] for _ in range(M)])
    ids, scores, _ = _run(q.float(), W2.float(), b2.float(), k, exclude=ex2)
    eids, escores, _ = _int_expect(q, W2, b2, k, exclude=ex2)
    assert torch.equal(ids, eids) and torch.equal(scores, escores)
    assert bool((ids[:, n2 - E:] == -1).all()) and bool((scores[:, n2 - E:] == float('-inf')).all())
    assert bool((ids[:, :n2 - E] >= 0).all())


def test_row_filter():
    M, n, d, k = 130, 300, 64, 20
    q, W, b, t = _int_data(M, n, d, seed=6)
    g = torch.Generator().manual_seed(66)
    dom = torch.randint(0, 2, (M,), generator=g) * 3  # any nonzero value names domain b
    dom[128:] = 3  # the second row block holds no row of domain a
    eids, escores, erank = _int_expect(q, W, b, k, t)

    def fresh():
        return (torch.full((M, k), -7, dtype=torch.int64, device=DEV),
                torch.full((M, k), 123.0, dtype=torch.float32, device=DEV),
                torch.full((M,), -9, dtype=torch.int32, device=DEV))

    for which in (0, 1):
        out = fresh()
        _run(q.float(), W.float(), b.float(), k, target=t, dom=dom, which=which, out=out, n_split=2)
        ids, scores, rank = (x.cpu() for x in out)
        mine = (dom != 0) == (which != 0)
        assert torch.equal(ids[mine], eids[mine]) and torch.equal(scores[mine], escores[mine])
        assert torch.equal(rank[mine], erank[mine])
        assert bool((ids[~mine] == -7).all()) and bool((scores[~mine] == 123.0).all()) and bool((rank[~mine] == -9).all())
    # both heads into shared buffers cover every row
    out = fresh()
    for which in (0, 1):
        _run(q.float(), W.float(), b.float(), k, target=t, dom=dom, which=which, out=out)
    assert torch.equal(out[0].cpu(), eids) and torch.equal(out[2].cpu(), erank)
    # no matching row anywhere: nothing is written
    out = fresh()
    _run(q.float(), W.float(), b.float(), k, target=t, dom=torch.zeros(M, dtype=torch.int64), which=1, out=out)
    assert bool((out[0] == -7).all()) and bool((out[1] == 123.0).all()) and bool((out[2] == -9).all())


# ---------------------------------------------------------------- 6. bad target
def test_bad_and_negative_targets():
    M, n, d, k = 33, 1000, 64, 5
    q, W, b, t = _int_data(M, n, d, seed=7)
    eids, escores, erank = _int_expect(q, W, b, k, t)
    t2 = t.clone()
    t2[1::2] -= n  # torch-style wrap
    t2[0], t2[4], t2[8] = n, -n - 1, 10 ** 12
    ids, scores, rank = _run(q.float(), W.float(), b.float(), k, target=t2)
    erank = erank.clone()
    erank[[0, 4, 8]] = -1
    assert torch.equal(rank, erank)
    assert torch.equal(ids, eids) and torch.equal(scores, escores)


# ---------------------------------------------------------------- 7. trainer level (golden config `base`)
@functools.lru_cache(maxsize=None)
def _trainer_case():
    from tests.test_gpu_eval import _eval_batch, _eval_trainer
    tr, _ = _eval_trainer('base')
    batch = _eval_batch('base', 'val')
    tr.model.eval()
    with torch.no_grad():
        tr.model.convolve_graph()
        dv = [x.to(DEV) for x in batch]
        h_share, hx, hy = (h.detach().cpu() for h in tr.model(*dv[:6]))
    m = tr.model
    B, L = batch[1].shape
    xory = batch[8].reshape(-1)
    il_a, il_b, gt = batch[6].reshape(-1), batch[7].reshape(-1), batch[9].reshape(-1)
    rows = []
    for i in range(B):
        a = int(xory[i]) == 0
        il = int((il_a if a else il_b)[i])
        qi = (h_share[i, -1] + (hx if a else hy)[i, il]).double()  # the fp32 add of the query, then float64
        head = m.classifier_a if a else m.classifier_b
        rows.append(head.weight.detach().cpu().double() @ qi + head.bias.detach().cpu().double())
    return tr, batch, rows, xory, gt


def _check_rows(ids, scores, rank, rows, gt, k, exclude=None):
    for i, s in enumerate(rows):
        s = s.clone()
        t = gt[i:i + 1] % len(s)
        if exclude is not None:
            e = exclude[i]
            e = e[(e >= 0) & (e < len(s))]
            assert not bool((ids[i][:, None] == e[None, :]).any())
            keep = torch.ones(len(s), dtype=torch.bool)
            keep[e] = False
            back = torch.nonzero(keep)[:, 0]
            pos = torch.full((len(s),), -1, dtype=torch.int64)
            pos[back] = torch.arange(len(back))
            assert bool((pos[ids[i]] >= 0).all())
            _check_band(pos[ids[i]][None], scores[i][None], None, s[back][None], None, k)
        else:
            _check_band(ids[i][None], scores[i][None], None if rank is None else rank[i][None], s[None], t, k)


def test_trainer_full_ranks_and_recommend():
    tr, batch, rows, xory, gt = _trainer_case()
    with torch.no_grad():
        rank, flag = tr.full_ranks(batch)
        ids, scores = tr.recommend(batch[:9], k=5, exclude_seen=False)
        ids_x, scores_x = tr.recommend(batch[:9], k=5, exclude_seen=True)
    assert rank.dtype == torch.int32 and torch.equal(flag.cpu(), xory)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (len(rows), 5) and scores.dtype == torch.float32
    _check_rows(ids.cpu(), scores.cpu(), rank.cpu(), rows, gt, 5)
    n_a = tr.n_item_a
    seen = torch.where(xory[:, None] == 0, batch[1], batch[2] - n_a)  # the row's in-domain history, domain-local
    _check_rows(ids_x.cpu(), scores_x.cpu(), None, rows, gt, 5, exclude=seen)


def test_trainer_evaluate_full_and_bad_index():
    from c2dsr_amd.metrics import RankMetrics
    tr, batch, _, _, _ = _trainer_case()
    with torch.no_grad():
        rank, flag = tr.full_ranks(batch)
    whole = RankMetrics(DEV)
    whole.add(rank, flag)
    half = batch[0].shape[0] // 2
    parts = [tuple(x[:half] for x in batch), tuple(x[half:] for x in batch)]
    got = tr.evaluate_full(parts)
    for a, e in zip(got.values(), whole.values()):
        assert a == pytest.approx(e, rel=1e-12)
    bad = list(batch)
    bad[6], bad[7] = bad[6].clone(), bad[7].clone()
    bad[6][0], bad[7][0] = 10 ** 6, 10 ** 6
    with pytest.raises(IndexError):
        tr.recommend(tuple(bad[:9]), k=5)
    with pytest.raises(IndexError):
        tr.evaluate_full([tuple(bad)]).values()
