"""Per-kernel numerics of the loss head (csrc/loss.hip), the row utilities and the row-subset embedding on the
MI355X: every entry point through the C ABI against a plain float64 CPU computation of the same op on the same
fp32 inputs.

Tolerances (u = 2^-24, the fp32 unit roundoff):
* copies, index work, integer counts, a single fp32 add: bit-equal;
* an fp32 sum of n products: the a-priori bound (n + 2)·u·Σ|terms|, evaluated per element in float64;
* one or two fused multiply-adds per element: 4·u·Σ|operands of the sum| (the compiler may contract a·b + c);
* kernels built on __expf / logf: the suite's fp32 convention, rel < 1e-5 of max |reference|.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope='module', autouse=True)
def _lib():
    from c2dsr_amd._lib import lib
    assert torch.cuda.is_available()
    lib.load()
    yield


def dv(t):
    return None if t is None else t.to(DEV)


def f32(x):
    """A Python float as the kernel receives it (a float argument of the C ABI), in double."""
    return float(np.float32(x))


def assert_within(got, ref, bound, what=''):
    """|got - ref| <= bound element-wise (ref, bound float64 on the CPU); on failure: how many miss, the largest
    error, the smallest bound among them."""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), (what, int(bad.sum()), float(err[bad].max()), float(bound[bad].min()))


def assert_bits_equal(a, b):
    """Bit equality of two fp32 tensors (NaN patterns included)."""
    assert torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


# ----------------------------------------------------------------------------- 1. pooling
POOL_SHAPES = [(1, 7, 4), (6, 17, 12), (5, 50, 256), (3, 100, 64), (2, 128, 512)]


def _masks(B, L, g, first_kind):
    """int64 [B, L] masks, no row all-zero; row b is of kind (first_kind + b) % 4: 0 = a single nonzero, 1 = all ones,
    2 = values in {0, 1, 2, 3}, 3 = 0/1 at density 0.3."""
    gm = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        kind = (first_kind + b) % 4
        if kind == 0:
            gm[b, int(torch.randint(0, L, (1,), generator=g))] = 1
        elif kind == 1:
            gm[b] = 1
        elif kind == 2:
            gm[b] = torch.randint(0, 4, (L,), generator=g)
        else:
            gm[b] = (torch.rand(L, generator=g) < 0.3).long()
        if int(gm[b].sum()) == 0:
            gm[b, int(torch.randint(0, L, (1,), generator=g))] = 1
    return gm


def _pool_case(B, L, d, empty=None):
    """Masks, their fp32 mean-pooling weights (computed on the CPU, as Trainer.cal_mask), h and output gradients.
    B = 2 starts at kind 1 so that its two rows are the all-ones and the {0..3} rows at L = 128."""
    g = torch.Generator().manual_seed(B * 1000 + L * 10 + d)
    first = 1 if B == 2 else 0
    gma, gmb = _masks(B, L, g, first), _masks(B, L, g, first + 2)
    if empty is not None:
        gma[empty] = 0
        gmb[empty] = 0
    wa = gma.float() / gma.float().sum(-1, keepdim=True)  # 0 / 0 = NaN for an empty mask
    wb = gmb.float() / gmb.float().sum(-1, keepdim=True)
    h = torch.randn(B * L, d, generator=g)
    d1, d2 = torch.randn(B, d, generator=g), torch.randn(B, d, generator=g)
    return g, gma, gmb, wa, wb, h, d1, d2


def _pool_ref(h, w, B, L, d):
    """float64 Σ_l h[b,l,:]·w[b,l] and its n-term fp32 bound."""
    terms = h.double().reshape(B, L, d) * w.double().reshape(B, L, 1)
    return terms.sum(1), (L + 2) * U * terms.abs().sum(1)


def _compact(need, g):
    """The rows of ``need`` (bool [M]) in a random permuted order: (row list int32, inverse map int32 with -1
    elsewhere)."""
    rows = torch.nonzero(need).reshape(-1)
    rows = rows[torch.randperm(rows.numel(), generator=g)]
    inv = torch.full((need.numel(),), -1, dtype=torch.int32)
    inv[rows] = torch.arange(rows.numel(), dtype=torch.int32)
    return rows.to(torch.int32), inv


def _compact_h(h, rows, guard_value):
    """h's rows ``rows`` behind one leading guard row inside the same tensor: compact row 0 starts one row in, so a
    kernel that follows a -1 map entry reads the guard row (and stays inside the tensor)."""
    buf = torch.empty(rows.numel() + 1, h.shape[1])
    buf[0] = guard_value
    buf[1:] = h[rows.long()]
    return dv(buf)


@pytest.mark.parametrize('B,L,d', POOL_SHAPES)
def test_pool_weights(B, L, d):
    from c2dsr_amd._lib import lib, stream
    _, gma, gmb, _, _, _, _, _ = _pool_case(B, L, d)
    for gm in (gma, gmb):
        w = torch.full((B, L), float('nan'), device=DEV)
        lib('c2dsr_pool_weights', dv(gm), B, L, w, stream())
        ref = gm.double() / gm.double().sum(-1, keepdim=True)
        assert_within(w, ref, 4 * U * ref.abs(), 'pool_weights')  # 4·u·|ref| <= 4 ulp
        assert torch.equal(w.cpu() == 0, gm == 0)


@pytest.mark.parametrize('mapped', [False, True])
@pytest.mark.parametrize('dual', [False, True])
@pytest.mark.parametrize('B,L,d', POOL_SHAPES)
def test_pool2_fwd(B, L, d, dual, mapped):
    from c2dsr_amd._lib import lib, stream
    g, gma, gmb, wa, wb, h, _, _ = _pool_case(B, L, d)
    hd, hmap = dv(h), None
    if mapped:  # compact h: exactly the rows with a nonzero weight, permuted, behind a NaN guard row
        need = (gma != 0) | (gmb != 0) if dual else gma != 0
        rows, inv = _compact(need.reshape(-1), g)
        hd, hmap = _compact_h(h, rows, float('nan'))[1:], dv(inv)
    o1 = torch.full((B, d), float('nan'), device=DEV)
    o2 = torch.full((B, d), float('nan'), device=DEV) if dual else None
    lib('c2dsr_pool2_fwd', hd, hmap, dv(wa), dv(wb) if dual else None, B, L, d, o1, o2, stream())
    assert_within(o1, *_pool_ref(h, wa, B, L, d), 'out1')
    if dual:
        assert_within(o2, *_pool_ref(h, wb, B, L, d), 'out2')


def test_pool2_fwd_refuses_w2_without_out2():
    from c2dsr_amd._lib import HipLibError, lib, stream
    B, L, d = 2, 5, 8
    w = torch.rand(B, L, device=DEV)
    with pytest.raises(HipLibError, match='hipError 1'):
        lib('c2dsr_pool2_fwd', torch.randn(B * L, d, device=DEV), None, w, w, B, L, d,
            torch.empty(B, d, device=DEV), None, stream())


@pytest.mark.parametrize('B,L,d', POOL_SHAPES)
def test_pool_fwd_bwd(B, L, d):
    """c2dsr_pool_fwd / c2dsr_pool_bwd (single weight, full rows; bwd accumulates into dh)."""
    from c2dsr_amd._lib import lib, stream
    g, _, _, wa, _, h, d1, _ = _pool_case(B, L, d)
    out = torch.full((B, d), float('nan'), device=DEV)
    lib('c2dsr_pool_fwd', dv(h), dv(wa), B, L, d, out, stream())
    assert_within(out, *_pool_ref(h, wa, B, L, d), 'pool_fwd')
    dh0 = torch.randn(B * L, d, generator=g)
    dh = dv(dh0)
    lib('c2dsr_pool_bwd', dv(d1), dv(wa), B, L, d, dh, stream())
    t = d1.double().repeat_interleave(L, 0) * wa.double().reshape(-1, 1)
    assert_within(dh, dh0.double() + t, 4 * U * (dh0.double().abs() + t.abs()), 'pool_bwd')


@pytest.mark.parametrize('compact', [False, True])
@pytest.mark.parametrize('dual', [False, True])
@pytest.mark.parametrize('B,L,d', POOL_SHAPES)
def test_pool2_bwd(B, L, d, dual, compact):
    from c2dsr_amd._lib import lib, stream
    g, gma, gmb, wa, wb, _, d1, d2 = _pool_case(B, L, d)
    t = d1.double().repeat_interleave(L, 0) * wa.double().reshape(-1, 1)
    mag = t.abs()
    if dual:
        t2 = d2.double().repeat_interleave(L, 0) * wb.double().reshape(-1, 1)
        t, mag = t + t2, mag + t2.abs()
    idx, n_rows = None, 0
    if compact:
        need = (gma != 0) | (gmb != 0) if dual else gma != 0
        rows, _ = _compact(need.reshape(-1), g)
        assert rows.numel() < B * L
        idx, n_rows = dv(rows), rows.numel()
        t, mag = t[rows.long()], mag[rows.long()]
    n = n_rows if compact else B * L
    args = (dv(d1), dv(wa), dv(d2) if dual else None, dv(wb) if dual else None, B, L, d, idx, n_rows)
    dh = torch.full((n, d), float('nan'), device=DEV)  # accumulate 0: overwritten
    lib('c2dsr_pool2_bwd', *args, 0, dh, stream())
    assert_within(dh, t, 4 * U * mag, 'overwrite')
    dh0 = torch.randn(n, d, generator=g)
    dh = dv(dh0)
    lib('c2dsr_pool2_bwd', *args, 1, dh, stream())
    assert_within(dh, dh0.double() + t, 4 * U * (dh0.double().abs() + mag), 'accumulate')


@pytest.mark.parametrize('mapped', [False, True])
@pytest.mark.parametrize('B,L,d', [(6, 17, 12), (3, 100, 64)])
def test_pool2_empty_mask_sequence(B, L, d, mapped):
    """A sequence whose mask is empty has NaN weights (0 / 0, as the reference's cal_mask): its pooled outputs and
    its rows of dh are NaN, every other sequence is unaffected — and with a row map, whose entries for that
    sequence are -1, no row of h is read for it (a -1 row contributes a zero vector).  The compact h sits behind a
    finite guard row, so every access stays inside the tensor either way."""
    from c2dsr_amd._lib import lib, stream
    e = 1
    g, gma, gmb, wa, wb, h, d1, d2 = _pool_case(B, L, d, empty=e)
    assert torch.isnan(wa[e]).all() and torch.isnan(wb[e]).all()
    w = torch.full((B, L), 7.0, device=DEV)
    lib('c2dsr_pool_weights', dv(gma), B, L, w, stream())
    assert torch.isnan(w[e]).all() and torch.equal(torch.isnan(w).cpu(), torch.isnan(wa))
    hd, hmap = dv(h), None
    need = ((gma != 0) | (gmb != 0)).reshape(-1)
    rows, inv = _compact(need, g)
    if mapped:
        hd, hmap = _compact_h(h, rows, 0.5)[1:], dv(inv)
        assert int(inv[e * L:(e + 1) * L].max()) == -1
    o1 = torch.zeros(B, d, device=DEV)
    o2 = torch.zeros(B, d, device=DEV)
    lib('c2dsr_pool2_fwd', hd, hmap, dv(wa), dv(wb), B, L, d, o1, o2, stream())
    ok = torch.arange(B) != e
    for o, wt in ((o1, wa), (o2, wb)):
        assert torch.isnan(o[e]).all()
        ref, bound = _pool_ref(h, torch.nan_to_num(wt), B, L, d)
        assert_within(o[dv(ok)], ref[ok], bound[ok], 'other sequences')
    # backward: the full layout gives the empty sequence's rows NaN; the compact layout does not hold them
    t = (d1.double().repeat_interleave(L, 0) * wa.double().reshape(-1, 1)
         + d2.double().repeat_interleave(L, 0) * wb.double().reshape(-1, 1))
    mag = (d1.double().repeat_interleave(L, 0) * wa.double().reshape(-1, 1)).abs() + \
        (d2.double().repeat_interleave(L, 0) * wb.double().reshape(-1, 1)).abs()
    if mapped:
        dh = torch.full((rows.numel(), d), float('nan'), device=DEV)
        lib('c2dsr_pool2_bwd', dv(d1), dv(wa), dv(d2), dv(wb), B, L, d, dv(rows), rows.numel(), 0, dh, stream())
        assert_within(dh, t[rows.long()], 4 * U * mag[rows.long()], 'compact bwd')
    else:
        dh = torch.zeros(B * L, d, device=DEV)
        lib('c2dsr_pool2_bwd', dv(d1), dv(wa), dv(d2), dv(wb), B, L, d, None, 0, 0, dh, stream())
        rows_ok = ok.repeat_interleave(L)
        assert torch.isnan(dh.reshape(B, L, d)[e]).all()
        assert_within(dh[dv(rows_ok)], t[rows_ok], 4 * U * mag[rows_ok], 'full bwd')


def test_pool2_bwd_unmapped_compact_row():
    """A compact row whose idx entry is -1 belongs to no (b, l): no weight is read for it and it receives a zero
    vector (accumulate 0) or keeps its value (accumulate 1).  The weights sit one element inside a larger tensor,
    so element -1 of them is inside it too."""
    from c2dsr_amd._lib import lib, stream
    B, L, d = 3, 9, 8
    g = torch.Generator().manual_seed(4)
    wbuf = torch.rand(B * L + 1, generator=g)
    wbuf[0] = 1e30
    wd = dv(wbuf)[1:]
    w = wbuf[1:]
    d1 = torch.randn(B, d, generator=g)
    idx = torch.tensor([5, -1, 26, 0, -1, 13], dtype=torch.int32)
    live = idx >= 0
    t = torch.zeros(idx.numel(), d, dtype=torch.float64)
    t[live] = d1.double()[idx[live].long() // L] * w.double()[idx[live].long()].reshape(-1, 1)
    dh = torch.full((idx.numel(), d), float('nan'), device=DEV)
    lib('c2dsr_pool2_bwd', dv(d1), wd, None, None, B, L, d, dv(idx), idx.numel(), 0, dh, stream())
    assert_within(dh, t, 4 * U * t.abs(), 'overwrite')
    assert torch.equal(dh.cpu()[~live], torch.zeros(int((~live).sum()), d))
    dh0 = torch.randn(idx.numel(), d, generator=g)
    dh = dv(dh0)
    lib('c2dsr_pool2_bwd', dv(d1), wd, None, None, B, L, d, dv(idx), idx.numel(), 1, dh, stream())
    assert_within(dh, dh0.double() + t, 4 * U * (dh0.double().abs() + t.abs()), 'accumulate')
    assert torch.equal(dh.cpu()[~live], dh0[~live])


# ----------------------------------------------------------------------------- 2. discriminator scores, MI loss
@pytest.mark.parametrize('ldo', [1, 4])
@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('d', [4, 16, 100, 256, 512])
@pytest.mark.parametrize('M', [1, 5, 777])
def test_rowdot(M, d, bias, ldo):
    from c2dsr_amd._lib import lib, stream
    g = torch.Generator().manual_seed(M * 1000 + d)
    xb = torch.randn(M, d + 4, generator=g)  # ldx = d + 4: the last 4 columns are not part of the rows
    xb[:, d:] = float('nan')
    y = torch.randn(M, d, generator=g)
    bv = torch.randn(1, generator=g) if bias else None
    O0 = torch.randn(M, ldo, generator=g)
    O = dv(O0)
    col = ldo // 2
    lib('c2dsr_rowdot', dv(xb), d + 4, dv(y), d, M, d, dv(bv), O[:, col], ldo, stream())
    terms = xb[:, :d].double() * y.double()
    ref, mag, n = terms.sum(1), terms.abs().sum(1), d
    if bias:
        ref, mag, n = ref + bv.double(), mag + bv.double().abs(), d + 1
    assert_within(O[:, col], ref, (n + 2) * U * mag, 'rowdot')
    keep = torch.arange(ldo) != col
    assert torch.equal(O.cpu()[:, keep], O0[:, keep])  # the other columns of the larger tensor: untouched


@pytest.mark.parametrize('norm_mult', [1, 4])
@pytest.mark.parametrize('B', [1, 63, 1000, 1025, 2500])
def test_mi_loss(B, norm_mult):
    from c2dsr_amd._lib import lib, stream
    g = torch.Generator().manual_seed(B)
    s = torch.randn(4, B, generator=g) * 3
    planted = [0.0, 30.0, -30.0, 90.0, -90.0]
    for k in range(4):  # every planted value in every row (as many as B holds), at rotating positions
        for j in range(min(B, 5)):
            s[k, (j * 211) % B if B >= 5 else j] = planted[(j + k) % 5]
    Bn = norm_mult * B  # the global batch under data parallelism
    outs = []
    for _ in range(2):
        loss = torch.full((1,), float('nan'), device=DEV)
        ds = torch.full((4, B), float('nan'), device=DEV)
        lib('c2dsr_mi_loss', dv(s), B, Bn, loss, ds, stream())
        outs.append((loss.cpu(), ds.cpu()))
    x = s.double()
    yl = torch.tensor([1.0, 0.0, 1.0, 0.0], dtype=torch.float64)[:, None]
    bce = x.clamp_min(0) - x * yl + torch.log1p(torch.exp(-x.abs()))  # BCEWithLogits, float64
    ref_loss = bce.sum() / Bn
    ref_ds = (torch.sigmoid(x) - yl) / Bn
    loss, ds = outs[0]
    assert torch.isfinite(loss).all() and torch.isfinite(ds).all()
    assert abs(float(loss) - float(ref_loss)) < 1e-5 * abs(float(ref_loss))
    assert rel(ds, ref_ds) < 1e-5
    assert_bits_equal(outs[0][0], outs[1][0])
    assert_bits_equal(outs[0][1], outs[1][1])


# ----------------------------------------------------------------------------- 3. classifier-head operands
REC_SHAPES = [(1, 7, 4, 3), (5, 20, 12, 5), (37, 50, 256, 10), (3, 128, 64, 128)]


def _rec_case(B, L, d, R, mapped, seed=0):
    """hs / hx [B·L, d] and, mapped, permuted compact subsets of their rows holding at least the last R positions:
    (device tensor, device map or None, row list or None) for each."""
    g = torch.Generator().manual_seed(B * 100 + L + d + R + seed)
    M = B * L
    hs, hx = torch.randn(M, d, generator=g), torch.randn(M, d, generator=g)
    tail = (torch.arange(M) % L) >= L - R
    out = []
    for h in (hs, hx):
        if mapped:
            need = tail | (torch.rand(M, generator=g) < 0.3)
            rows, inv = _compact(need, g)
            out.append((dv(h[rows.long()].contiguous()), dv(inv), rows.long()))
        else:
            out.append((dv(h), None, None))
    b = torch.arange(B).repeat_interleave(R)
    bl = b * L + (L - R) + torch.arange(R).repeat(B)  # the (b, L-R+k) rows, stacked row r = b·R + k
    return g, hs, hx, out, bl


@pytest.mark.parametrize('mapped', [False, True])
@pytest.mark.parametrize('B,L,d,R', REC_SHAPES)
def test_rec_gather_and_targets(B, L, d, R, mapped):
    from c2dsr_amd._lib import lib, stream
    g, hs, hx, ((hsd, hsm, _), (hxd, hxm, _)), bl = _rec_case(B, L, d, R, mapped)
    BR = B * R
    Hcat = torch.full((2 * BR, d), float('nan'), device=DEV)
    Hpad = torch.full((2 * BR, d), float('nan'), device=DEV)
    lib('c2dsr_rec_gather', hsd, hsm, hxd, hxm, B, L, d, R, Hcat, Hpad, stream())
    assert torch.equal(Hcat.cpu(), torch.cat([hs[bl], hs[bl] + hx[bl]]))  # second half: one fp32 add
    assert torch.equal(Hpad.cpu(), torch.cat([hs[bl], hx[bl]]))
    ts, tx = torch.randint(0, 1000, (B, L), generator=g), torch.randint(0, 1000, (B, L), generator=g)
    tcat = torch.full((2 * BR,), -1, dtype=torch.int64, device=DEV)
    lib('c2dsr_rec_targets', dv(ts), dv(tx), B, L, R, tcat, stream())
    assert torch.equal(tcat.cpu(), torch.cat([ts.reshape(-1)[bl], tx.reshape(-1)[bl]]))


@pytest.mark.parametrize('mapped', [False, True])
@pytest.mark.parametrize('B,L,d,R', REC_SHAPES)
def test_rec_scatter(B, L, d, R, mapped):
    from c2dsr_amd._lib import lib, stream
    g, hs0, hx0, ((hsd, hsm, hsr), (hxd, hxm, hxr)), bl = _rec_case(B, L, d, R, mapped, seed=1)  # prefilled dhs / dhx
    BR, n = B * R, 5
    dHcat = torch.randn(2 * BR, d, generator=g)
    dl = torch.randn(2 * BR, n + 1, generator=g)  # the pad column of dlogits: strided, pad_ld = n + 1
    wpad = torch.randn(d, generator=g)
    dld = dv(dl)
    lib('c2dsr_rec_scatter', dv(dHcat), dld[:, n], n + 1, dv(wpad), B, L, d, R, hsd, hsm, hxd, hxm, stream())
    g1, g2 = dHcat[:BR].double(), dHcat[BR:].double()
    p1 = dl[:BR, n].double()[:, None] * wpad.double()
    p2 = dl[BR:, n].double()[:, None] * wpad.double()
    for got, rows, h0, add, mag in ((hsd, hsr, hs0, g1 + g2 + p1, g1.abs() + g2.abs() + p1.abs()),
                                    (hxd, hxr, hx0, g2 + p2, g2.abs() + p2.abs())):
        ref = h0.double().clone()
        bound = torch.zeros_like(ref)  # rows outside the last R positions: bit-unchanged
        ref[bl] += add
        bound[bl] = 4 * U * (h0.double()[bl].abs() + mag)
        if rows is not None:
            ref, bound = ref[rows], bound[rows]
        assert_within(got, ref, bound, 'rec_scatter')


@pytest.mark.parametrize('split', [0, 1])
@pytest.mark.parametrize('mapped', [False, True])
@pytest.mark.parametrize('B,L,d,R', REC_SHAPES)
def test_rec_gather_compact(B, L, d, R, mapped, split):
    from c2dsr_amd._lib import lib, stream
    g, hs, hx, ((hsd, hsm, _), (hxd, hxm, _)), bl = _rec_case(B, L, d, R, mapped, seed=2)
    BR = B * R
    Hcat = torch.cat([hs[bl], hs[bl] + hx[bl]])
    Hpad_ref = torch.cat([hs[bl], hx[bl]])
    keep = torch.rand(2 * BR, generator=g) < 0.6
    keep[int(torch.randint(0, 2 * BR, (1,), generator=g))] = True
    for idx in (torch.nonzero(keep).reshape(-1).to(torch.int32), None):  # an ascending 60 % subset; Mv = 0
        Mv = 0 if idx is None else idx.numel()
        M_pad = -(-Mv // 64) * 64
        cols = 2 * d if split else d
        Hpad = torch.full((2 * BR, d), float('nan'), device=DEV)
        Hc = torch.full((max(Mv, 1), d), float('nan'), device=DEV)
        img = torch.full((max(M_pad, 1), cols), float('nan'), device=DEV, dtype=torch.bfloat16)
        lib('c2dsr_rec_gather_compact', hsd, hsm, hxd, hxm, B, L, d, R, dv(idx), Mv, M_pad, split, Hpad, Hc, img,
            stream())
        assert torch.equal(Hpad.cpu(), Hpad_ref)
        if Mv == 0:
            continue
        Hc_ref = Hcat[idx.long()]
        assert torch.equal(Hc.cpu(), Hc_ref)
        # the image: what the conversion kernels make of the reference rows (the kernel comment's claim)
        want = torch.full((M_pad, cols), float('nan'), device=DEV, dtype=torch.bfloat16)
        if split:
            lib('c2dsr_f32_split_bf16', dv(Hc_ref), Mv, d, M_pad, want, stream())
        else:
            want[Mv:] = 0
            lib('c2dsr_f32_to_bf16', dv(Hc_ref), Mv * d, want, stream())
        assert torch.equal(img.view(torch.int16), want.view(torch.int16))
        assert torch.equal(img[Mv:].view(torch.int16), torch.zeros(M_pad - Mv, cols, dtype=torch.int16, device=DEV))
        # and independently of them: hi = RNE bf16 of the value, lo = RNE bf16 of the remainder
        hi = Hc_ref.to(torch.bfloat16)
        assert torch.equal(img[:Mv, :d].cpu(), hi)
        if split:
            assert torch.equal(img[:Mv, d:].cpu(), (Hc_ref - hi.float()).to(torch.bfloat16))


# ----------------------------------------------------------------------------- 4. materialised-logit CE, scalars
CE_SHAPES = [(1, 1, 2), (5, 62, 64), (130, 256, 260), (64, 1000, 1001)]
# the per-row loss lse - l[t] is a difference of two fp32 values: where the target holds all of the mass it cancels.
# Measured at (M 1, n 1, ld 2), scale 25 (logits 14.1612, -13.7317, target 0): the same formula in fp32 torch on the
# CPU gives 0 where float64 gives 7.69e-13 (fp32 lse rounds to the target logit), rel 1.0 of max |ref|; 4x that.
# Every case is also held to 1e-5 of max |lse| (the scale of the two values subtracted).
CE_ROW_TOL = {(1, 1, 25.0, 'mixed'): 4.0}


@pytest.mark.parametrize('scale,tmode', [(1.0, 'mixed'), (25.0, 'mixed'), (1.0, 'valid'), (25.0, 'ignored')])
@pytest.mark.parametrize('M,n,ld', CE_SHAPES)
def test_ce_fwd_bwd(M, n, ld, scale, tmode):
    """c2dsr_ce_fwd / c2dsr_ce_bwd over ncol = n + 1 logits of rows of stride ld (the width every d that
    c2dsr_ce_supported refuses runs): lse and the per-row loss against float64 logsumexp, the in-place gradient
    against (exp(l - lse) - onehot)·w_r; the columns from ncol up to ld hold NaN and are neither read nor
    written."""
    from c2dsr_amd._lib import lib, stream
    g = torch.Generator().manual_seed(M + n + int(scale))
    ncol, ignore = n + 1, n
    lg = torch.full((M, ld), float('nan'))
    lg[:, :ncol] = torch.randn(M, ncol, generator=g) * scale
    if M >= 3:
        lg[1, int(torch.randint(0, ncol, (1,), generator=g))] += 80.0  # one +80 outlier
        lg[2, :ncol] = 3.0                                             # all-equal values
    t = torch.randint(0, n, (M,), generator=g)
    if tmode == 'mixed':
        t[torch.rand(M, generator=g) < 0.3] = ignore
    elif tmode == 'ignored':
        t[:] = ignore
    valid = t != ignore
    lgd = dv(lg)
    lse = torch.full((M,), float('nan'), device=DEV)
    rows = torch.full((M,), float('nan'), device=DEV)
    lib('c2dsr_ce_fwd', lgd, ld, M, ncol, dv(t), ignore, lse, rows, stream())
    x = lg[:, :ncol].double()
    lse_r = torch.logsumexp(x, 1)
    rows_r = torch.where(valid, lse_r - x.gather(1, t[:, None])[:, 0], torch.zeros(M, dtype=torch.float64))
    assert rel(lse, lse_r) < 1e-5
    assert rel(rows, rows_r) < CE_ROW_TOL.get((M, n, scale, tmode), 1e-5)
    assert float((rows.double().cpu() - rows_r).abs().max()) < 1e-5 * float(lse_r.abs().max())
    assert torch.equal(rows.cpu()[~valid], torch.zeros(int((~valid).sum())))  # ignored rows: exactly 0
    # backward in place, lse given (the fp32 rounding of the float64 value: an input of the kernel)
    split, lam = M // 2, 0.7
    coef, gs = torch.tensor([0.37, 1.9]), torch.tensor([0.5])
    lse_in = lse_r.float()
    lib('c2dsr_ce_bwd', lgd, ld, M, ncol, dv(t), ignore, dv(lse_in), dv(coef), split, dv(gs), lam, stream())
    w_r = torch.where(valid, gs.double() * f32(lam) * coef.double()[(torch.arange(M) >= split).long()],
                      torch.zeros(M, dtype=torch.float64))
    oh = torch.zeros(M, ncol, dtype=torch.float64)
    oh[torch.arange(M), t] = 1.0
    ref = (torch.exp(x - lse_in.double()[:, None]) - oh) * w_r[:, None]
    got = lgd.cpu()
    assert torch.isfinite(got[:, :ncol]).all()
    assert rel(got[:, :ncol], ref) < 1e-5
    assert_bits_equal(got[:, ncol:], lg[:, ncol:])  # columns ncol..ld: bit-unchanged


def test_outer_add_strided():
    from c2dsr_amd._lib import lib, stream
    g = torch.Generator().manual_seed(1)
    M, d, ldo, sa = 77, 37, 41, 6
    A, v = torch.randn(M, sa, generator=g), torch.randn(d, generator=g)
    out0 = torch.randn(M, ldo, generator=g)
    out, Ad = dv(out0), dv(A)
    lib('c2dsr_outer_add', Ad[:, 4], sa, dv(v), M, d, out, ldo, stream())
    p = A[:, 4].double()[:, None] * v.double()
    assert_within(out[:, :d], out0[:, :d].double() + p, 4 * U * (out0[:, :d].double().abs() + p.abs()), 'outer_add')
    assert torch.equal(out.cpu()[:, d:], out0[:, d:])


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('M,d', [(1, 4), (123, 7), (37, 100)])  # n = M·d: no multiple of 256
def test_rowscale(M, d, accumulate):
    from c2dsr_amd._lib import lib, stream
    g = torch.Generator().manual_seed(M + d)
    x, s, out0 = torch.randn(M, d, generator=g), torch.randn(M, generator=g), torch.randn(M, d, generator=g)
    out = dv(out0) if accumulate else torch.full((M, d), float('nan'), device=DEV)
    lib('c2dsr_rowscale', dv(x), dv(s), M * d, d, out, accumulate, stream())
    p = x.double() * s.double()[:, None]
    base = out0.double() if accumulate else torch.zeros_like(p)
    assert_within(out, base + p, 4 * U * (base.abs() + p.abs()), 'rowscale')


def test_scale_ds_and_loss_accumulate():
    from c2dsr_amd._lib import lib, stream
    g = torch.Generator().manual_seed(2)
    n, f = 4 * 333, 0.3
    ds0, gs = torch.randn(n, generator=g), torch.tensor([1.7])
    ds = dv(ds0)
    lib('c2dsr_scale_ds', ds, n, dv(gs), f, stream())
    ref = ds0.double() * gs.double() * f32(f)
    assert_within(ds, ref, 4 * U * ref.abs(), 'scale_ds')
    a, b, c = (torch.randn(1, generator=g) for _ in range(3))
    acc0, w = torch.randn(3, generator=g), 37.0
    acc = dv(acc0)
    lib('c2dsr_loss_accumulate', dv(a), dv(b), dv(c), w, acc, stream())
    p = w * torch.cat([a, b, c]).double()
    assert_within(acc, acc0.double() + p, 4 * U * (acc0.double().abs() + p.abs()), 'loss_accumulate')


@pytest.mark.parametrize('BR', [1, 100, 128, 1100, 5000])
def test_loss_partials(BR):
    from c2dsr_amd._lib import lib, stream
    g = torch.Generator().manual_seed(BR)
    n_a, n_b = 50, 70
    tA, tB = torch.randint(0, n_a, (2 * BR,), generator=g), torch.randint(0, n_b, (2 * BR,), generator=g)
    tA[torch.rand(2 * BR, generator=g) < 0.3] = n_a
    tB[torch.rand(2 * BR, generator=g) < 0.3] = n_b
    rA, rB = torch.rand(2 * BR, generator=g) * 10, torch.rand(2 * BR, generator=g) * 10
    rA[tA == n_a] = 777.0  # rows of ignored targets are not part of any sum
    rB[tB == n_b] = 777.0
    ws_n = int(lib.raw('c2dsr_loss_partials_workspace')(BR))
    half = (torch.arange(2 * BR) >= BR).long()
    cnt = torch.zeros(8, dtype=torch.float64)
    sums, mags, terms = torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), [0] * 4
    for q, (r, t, ig) in enumerate(((rA, tA, n_a), (rB, tB, n_b))):
        for h in (0, 1):
            sel = (t != ig) & (half == h)
            cnt[4 + 2 * q + h] = int(sel.sum())
            sums[2 * q + h] = r.double()[sel].sum()
            mags[2 * q + h] = r.double()[sel].abs().sum()
            terms[2 * q + h] = int(sel.sum())
    outs = []
    for _ in range(2):
        vec = torch.full((8,), float('nan'), device=DEV)
        ws = torch.full((ws_n,), float('nan'), device=DEV)
        lib('c2dsr_loss_partials', dv(rA), dv(tA), n_a, dv(rB), dv(tB), n_b, BR, vec, ws, stream())
        outs.append(vec.cpu())
    vec = outs[0]
    assert torch.equal(vec[4:].double(), cnt[4:])  # integers below 2^24: exact
    bound = torch.tensor([(terms[k] + 2) * U * float(mags[k]) for k in range(4)], dtype=torch.float64)
    assert_within(vec[:4], sums, bound, 'sums')
    assert_bits_equal(outs[0], outs[1])
    # counts only
    vec0 = torch.full((8,), float('nan'), device=DEV)
    ws = torch.full((ws_n,), float('nan'), device=DEV)
    lib('c2dsr_loss_partials', None, dv(tA), n_a, None, dv(tB), n_b, BR, vec0, ws, stream())
    assert torch.equal(vec0.cpu().double(), cnt)


@pytest.mark.parametrize('with_cnt', [False, True])
def test_loss_finalize(with_cnt):
    """The scalar combination of the reference's train_batch (its cross-entropy means, the count-weighted shared
    loss over len_rec·n_batch rows, loss_rec, the lambda mix) in float64, and the per-row gradient weights."""
    from c2dsr_amd._lib import lib, stream
    lam, BR_global = 0.7, 5000
    sums = torch.tensor([812.5, 1290.25, 640.75, 1511.0])
    counts = torch.tensor([301.0, 412.0, 256.0, 399.0])  # != BR_global
    lmi = 2.6183
    vec = torch.cat([sums, torch.tensor([11.0, 13.0, 17.0, 19.0]) if with_cnt else counts, torch.tensor([lmi])])
    cnt = torch.cat([torch.full((4,), float('nan')), counts]) if with_cnt else None
    out3, cA, cB = (torch.full((k,), float('nan'), device=DEV) for k in (3, 2, 2))
    lib('c2dsr_loss_finalize', dv(vec), dv(cnt), BR_global, lam, out3, cA, cB, stream())
    s, c, lm, RB = sums.double(), counts.double(), float(np.float32(lmi)), float(BR_global)
    ce = s / c  # F.cross_entropy(ignore_index): the mean over the valid rows
    loss_share = ce[0] * c[0] / RB + ce[2] * c[2] / RB
    loss_rec = loss_share + ce[1] + ce[3]
    loss = f32(lam) * loss_rec + (1 - f32(lam)) * lm
    for got, want in ((out3, [loss, loss_rec, lm]), (cA, [1 / RB, 1 / c[1]]), (cB, [1 / RB, 1 / c[3]])):
        want = torch.tensor([float(v) for v in want], dtype=torch.float64)
        assert float(((got.double().cpu() - want).abs() / want.abs()).max()) < 1e-6


# ----------------------------------------------------------------------------- 5. row utilities
@pytest.mark.parametrize('d,ld', [(8, 12), (6, 6), (8, 10)])  # float4 path; scalar (d); scalar (ld)
def test_gather_rows(d, ld):
    from c2dsr_amd._lib import lib, stream
    g = torch.Generator().manual_seed(d + ld)
    N, n = 301, 517
    src = torch.randn(N, ld, generator=g)
    idx = torch.randint(0, N, (n,), generator=g).to(torch.int32)
    dst = torch.full((n, d), float('nan'), device=DEV)
    lib('c2dsr_gather_rows', dv(src), ld, dv(idx), n, d, dst, stream())
    assert torch.equal(dst.cpu(), src[idx.long(), :d])


@pytest.mark.parametrize('d', [8, 6])
def test_expand_rows(d):
    from c2dsr_amd._lib import lib, stream
    g = torch.Generator().manual_seed(d)
    M = 515
    keep = torch.rand(M, generator=g) < 0.6
    rows = torch.nonzero(keep).reshape(-1)
    rows = rows[torch.randperm(rows.numel(), generator=g)]
    inv = torch.full((M,), -1, dtype=torch.int32)
    inv[rows] = torch.arange(rows.numel(), dtype=torch.int32)
    src = torch.randn(rows.numel(), d, generator=g)
    dst = torch.full((M, d), float('nan'), device=DEV)
    lib('c2dsr_expand_rows', dv(src), dv(inv), M, d, dst, stream())
    want = torch.zeros(M, d)
    want[rows] = src
    assert torch.equal(dst.cpu(), want)


# ----------------------------------------------------------------------------- 7. row-subset embedding
@pytest.mark.parametrize('d,p,nk0', [(64, 0.0, False), (64, 0.2, True), (256, 0.2, False), (256, 0.0, True)])
def test_embed_fwd_rows_equals_indexed_full(d, p, nk0):
    """c2dsr_embed_fwd_rows writes the rows q_idx ‖ k_idx of what c2dsr_embed_fwd writes for all rows (itself
    checked against float64 in test_gpu_kernels.test_embed_fwd_bwd_deterministic), bit for bit: the dropout
    element index is the input row's."""
    from c2dsr_amd._lib import lib, stream
    g = torch.Generator().manual_seed(d + int(p * 10))
    n_items, L, n_rows, base = 90, 10, 430, 77
    seq = torch.randint(0, n_items, (n_rows,), generator=g)
    pos = torch.randint(0, L, (n_rows,), generator=g)
    H, E, P = (dv(torch.randn(n_items, d, generator=g)), dv(torch.randn(n_items, d, generator=g)),
               dv(torch.randn(L, d, generator=g)))
    scale = float(d) ** 0.5
    full = torch.empty(n_rows, d, device=DEV)
    lib('c2dsr_embed_fwd', dv(seq), dv(pos), n_rows, d, H, E, None, P, scale, 11, 22, p, base, full, n_items, L, None,
        stream())
    qi = torch.nonzero(torch.rand(n_rows, generator=g) < 0.4).reshape(-1).to(torch.int32)
    ki = torch.nonzero(torch.rand(n_rows, generator=g) < 0.5).reshape(-1).to(torch.int32)
    assert len(set(qi.tolist()) & set(ki.tolist())) > 0  # overlapping
    if nk0:
        ki = ki[:0]
    nq, nk = qi.numel(), ki.numel()
    X = torch.full((nq + nk, d), float('nan'), device=DEV)
    lib('c2dsr_embed_fwd_rows', dv(seq), dv(pos), n_rows, d, H, E, P, scale, 11, 22, p, base, dv(qi), nq,
        dv(ki) if nk else None, nk, X, n_items, L, None, stream())
    assert torch.equal(X, full[dv(torch.cat([qi, ki]).long())])


@pytest.mark.parametrize('d,p', [(64, 0.0), (256, 0.2), (12, 0.3)])
def test_embed_fwd_given_rows(d, p):
    """c2dsr_embed_fwd with Xin (the lookup done elsewhere): X = (Xin + P[pos])·mask."""
    from c2dsr_amd._lib import lib, stream
    from oracle.c2dsr_oracle import keep_mask
    g = torch.Generator().manual_seed(d)
    L, n_rows, base, keys = 10, 433, 77, (11, 22)
    pos = torch.randint(0, L, (n_rows,), generator=g)
    Xin, P = torch.randn(n_rows, d, generator=g), torch.randn(L, d, generator=g)
    X = torch.full((n_rows, d), float('nan'), device=DEV)
    lib('c2dsr_embed_fwd', None, dv(pos), n_rows, d, None, None, dv(Xin), dv(P), 1.0, keys[0], keys[1], p, base, X, 0,
        L, None, stream())
    idx = (np.arange(n_rows)[:, None] + base) * d + np.arange(d)[None, :]
    mk = torch.from_numpy(keep_mask(idx, keys, p).astype(np.float64)) / (1 - f32(p))
    assert rel(X, (Xin.double() + P.double()[pos]) * mk) < 1e-6
