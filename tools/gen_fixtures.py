"""Generate golden vectors from the REFERENCE implementation (runs only in the
build container, where /root/reference exists; the GPU box never runs this).

The reference is imported read-only via sys.path; nothing of its source is
copied.  Outputs are plain arrays (npz, no pickles) under tests/golden/:

  data_<cfg>.npz   processed train/val/test lists from CDSRDataset
                   (dataloader.py:60-228, random.seed(3407) like main.py:91)
  graph_<cfg>.npz  COO of adj_share/adj_specific (utils/graph.py:33-96)
  model_<cfg>.npz  initial params, per-step intermediates, grads and params
                   for two train_batch steps (trainer.py:91-160), dropout 0
  eval_<cfg>.npz   evaluate_batch ranks after the two steps (trainer.py:162-181)
  metrics.npz      cal_metrics / cal_score (utils/metrics.py)
  fk_data.npz      checksums + head of the Food-Kitchen val/test processing
  fk_val_new.npz   the Food-Kitchen val_new.txt those checksums were made from, as bytes
  traj_<cfg>.npz   main.py's epoch loop driven through the reference Trainer(args, noter) for
                   N_EPOCH epochs (seeded like main.py:90-95, dropout 0, num_workers 0): per-epoch
                   train losses, the shuffled batch order, val/test ranks and cal_score
  processed_<cfg>/ the {train,val,test}.pkl + graph.pkl the reference writes with --use_raw
                   --save_processed (dataloader.py:26-29, utils/graph.py:101-103) and the item lists,
                   for the use_raw=False read path (c2dsr_amd/processed.py)

Usage:  python tools/gen_fixtures.py   (PYTHONDONTWRITEBYTECODE=1 is set here)
"""
import argparse
import hashlib
import os
import random
import sys
import tempfile
from types import SimpleNamespace

os.environ['PYTHONDONTWRITEBYTECODE'] = '1'
sys.dont_write_bytecode = True

import numpy as np
import torch

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, 'tests', 'golden')
sys.path.insert(0, REPO)
from c2dsr_amd import synth  # noqa: E402

CONFIGS = {
    # name: (n_a, n_b, L, R, d, n_train, n_eval, model flags)
    'base': dict(n_a=40, n_b=60, len_max=8, len_rec=4, d_latent=16, n_train=40, n_eval=12,
                 n_gnn=1, n_attn=1, n_head=1, norm_first=False, d_bias=False, shared_item_embed=False),
    'var': dict(n_a=40, n_b=60, len_max=8, len_rec=4, d_latent=16, n_train=40, n_eval=12,
                n_gnn=2, n_attn=2, n_head=2, norm_first=True, d_bias=True, shared_item_embed=False),
    'shared': dict(n_a=40, n_b=60, len_max=8, len_rec=4, d_latent=16, n_train=40, n_eval=12,
                   n_gnn=1, n_attn=1, n_head=1, norm_first=False, d_bias=False, shared_item_embed=True),
}
N_NEG = 10
BATCH = 16


def ref_import():
    sys.path.insert(0, REF)
    import dataloader as ref_dl  # noqa
    import models.C2DSR as ref_model  # noqa
    import trainer as ref_trainer  # noqa
    import utils.graph as ref_graph  # noqa
    import utils.metrics as ref_metrics  # noqa
    return ref_dl, ref_model, ref_trainer, ref_graph, ref_metrics


def make_args(cfg, path_raw, path_data):
    a = SimpleNamespace()
    a.dataset = 'Synthetic'
    a.path_raw = path_raw
    a.path_data = path_data
    a.use_raw = True
    a.save_processed = False
    a.device = torch.device('cpu')
    a.batch_size = BATCH
    a.batch_size_eval = 64
    a.num_workers = 0
    a.n_neg_sample = N_NEG
    a.len_max = cfg['len_max']
    a.len_rec = cfg['len_rec']
    a.d_latent = cfg['d_latent']
    a.n_gnn = cfg['n_gnn']
    a.n_attn = cfg['n_attn']
    a.n_head = cfg['n_head']
    a.norm_first = cfg['norm_first']
    a.d_bias = cfg['d_bias']
    a.shared_item_embed = cfg['shared_item_embed']
    a.dropout_gnn = 0.0
    a.dropout_attn = 0.0
    a.lr = 1e-3
    a.l2 = 5e-4
    a.lr_step = 10
    a.lr_gamma = 0.5
    a.lambda_loss = 0.7
    a.n_item_a = cfg['n_a']
    a.n_item_b = cfg['n_b']
    a.n_item = cfg['n_a'] + cfg['n_b'] + 1
    a.idx_pad = a.n_item - 1
    return a


def lists_to_arrays(rows, prefix):
    out = {}
    if not rows:
        return out
    k = len(rows[0])
    for j in range(k):
        col = [r[j] for r in rows]
        out[f'{prefix}_{j}'] = np.asarray(col, dtype=np.int64)
    return out


def gen_config(name, cfg, ref):
    ref_dl, ref_model, ref_trainer, ref_graph, ref_metrics = ref
    tmp = tempfile.mkdtemp(prefix=f'c2dsr_fx_{name}_')
    path_raw = os.path.join(tmp, 'raw')
    path_data = os.path.join(tmp, 'data')
    os.makedirs(path_data)
    synth.make_dataset(path_raw, cfg['n_a'], cfg['n_b'], cfg['len_max'], cfg['n_train'], cfg['n_eval'],
                       seed=11, ties=True, n_min=2)
    args = make_args(cfg, path_raw, path_data)

    # ---- a1: processed lists (main.py seeds random with 3407 before Trainer) ----
    random.seed(3407)
    torch.manual_seed(3407)
    np.random.seed(3407)
    ds_tr = ref_dl.CDSRDataset(args, 'train')
    ds_va = ref_dl.CDSRDataset(args, 'val')
    ds_te = ref_dl.CDSRDataset(args, 'test')
    data = {}
    data.update(lists_to_arrays(ds_tr.data, 'train'))
    data.update(lists_to_arrays(ds_va.data, 'val'))
    data.update(lists_to_arrays(ds_te.data, 'test'))
    data['n_train'] = np.int64(len(ds_tr.data))
    data['n_val'] = np.int64(len(ds_va.data))
    data['n_test'] = np.int64(len(ds_te.data))
    for mode in ('train', 'val', 'test'):
        with open(os.path.join(path_raw, f'{mode}_new.txt'), encoding='utf-8') as f:
            data[f'raw_{mode}'] = np.frombuffer(f.read().encode('utf-8'), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT, f'data_{name}.npz'), **data)

    # ---- a2: graphs ----
    adj_s, adj_p = ref_graph.preprocess_graph(args, os.path.join(path_raw, 'train_new.txt'))
    g = {}
    for k, adj in (('share', adj_s), ('specific', adj_p)):
        idx = adj._indices().numpy()
        g[f'{k}_row'] = idx[0].astype(np.int64)
        g[f'{k}_col'] = idx[1].astype(np.int64)
        g[f'{k}_val'] = adj._values().numpy().astype(np.float32)
    g['n'] = np.int64(args.n_item)
    np.savez_compressed(os.path.join(OUT, f'graph_{name}.npz'), **g)

    # ---- model: two train_batch steps, dropout 0, fixed batch order ----
    torch.manual_seed(1234)
    model = ref_model.C2DSR(args, adj_s, adj_p)
    tr = ref_trainer.Trainer.__new__(ref_trainer.Trainer)
    tr.model = model
    tr.optimizer = torch.optim.AdamW(filter(lambda x: x.requires_grad, model.parameters()), lr=args.lr,
                                     weight_decay=args.l2, amsgrad=True)
    tr.scheduler = torch.optim.lr_scheduler.StepLR(tr.optimizer, step_size=args.lr_step, gamma=args.lr_gamma)
    tr.device = args.device
    tr.d_latent = args.d_latent
    tr.n_item_a = args.n_item_a
    tr.n_item_b = args.n_item_b
    tr.len_rec = args.len_rec
    tr.lambda_loss = args.lambda_loss
    tr.label_pos = torch.ones(args.batch_size, 1)
    tr.label_neg = torch.zeros(args.batch_size, 1)

    m = {}
    for k, v in model.state_dict().items():
        m[f'init/{k}'] = v.detach().numpy().copy()
    m['param_names'] = np.array([n for n, p in model.named_parameters()])

    cap = {}

    def hook(name):
        def f(mod, inp, out):
            cap.setdefault(name, []).append(out.detach().numpy().copy())
        return f

    hooks = []
    for nm in ('gnn_share', 'gnn_a', 'gnn_b', 'attn_share', 'attn_a', 'attn_b', 'D_a', 'D_b'):
        hooks.append(getattr(model, nm).register_forward_hook(hook(nm)))

    real_step = tr.optimizer.step
    grads_snap = {}

    def step_wrapper(*a, **kw):
        grads_snap['g'] = {n: (p.grad.detach().numpy().copy() if p.grad is not None else None)
                           for n, p in model.named_parameters()}
        return real_step(*a, **kw)

    tr.optimizer.step = step_wrapper

    tensors = [torch.LongTensor(np.stack([np.asarray(r[j]) for r in ds_tr.data])) for j in range(14)]
    n_tr = tensors[0].shape[0]
    batches = [tuple(t[i:i + BATCH] for t in tensors) for i in range(0, n_tr, BATCH)]
    n_steps = min(3, len(batches))  # includes a short last batch when n_tr % BATCH != 0
    model.train()
    tr.optimizer.zero_grad()
    for s in range(n_steps):
        cap.clear()
        model.convolve_graph()
        loss, loss_rec, loss_mi = tr.train_batch(batches[s])
        m[f's{s}/loss'] = np.float32(loss.item())
        m[f's{s}/loss_rec'] = np.float32(loss_rec.item())
        m[f's{s}/loss_mi'] = np.float32(loss_mi.item())
        m[f's{s}/hi_share'] = cap['gnn_share'][0]
        m[f's{s}/hi_a'] = cap['gnn_a'][0]
        m[f's{s}/hi_b'] = cap['gnn_b'][0]
        m[f's{s}/h_share'] = cap['attn_share'][0]
        m[f's{s}/h_neg_a'] = cap['attn_share'][1]
        m[f's{s}/h_neg_b'] = cap['attn_share'][2]
        m[f's{s}/hx'] = cap['attn_a'][0]
        m[f's{s}/hy'] = cap['attn_b'][0]
        m[f's{s}/sim_a'] = np.stack(cap['D_a'])
        m[f's{s}/sim_b'] = np.stack(cap['D_b'])
        for n, gv in grads_snap['g'].items():
            if gv is not None:
                m[f's{s}/grad/{n}'] = gv
        for n, p in model.named_parameters():
            m[f's{s}/param/{n}'] = p.detach().numpy().copy()
        m[f's{s}/batch_lo'] = np.int64(s * BATCH)
        m[f's{s}/batch_n'] = np.int64(batches[s][0].shape[0])
    m['n_steps'] = np.int64(n_steps)
    for h in hooks:
        h.remove()
    np.savez_compressed(os.path.join(OUT, f'model_{name}.npz'), **m)

    # ---- eval ranks after the steps (model.eval(), one convolve_graph) ----
    model.eval()
    ev = {}
    with torch.no_grad():
        model.convolve_graph()
        for mode, ds in (('val', ds_va), ('test', ds_te)):
            t = [torch.LongTensor(np.stack([np.asarray(r[j]) for r in ds.data])) for j in range(11)]
            ra, rb = tr.evaluate_batch(tuple(t))
            ev[f'{mode}_rank_a'] = np.asarray(ra, dtype=np.int64)
            ev[f'{mode}_rank_b'] = np.asarray(rb, dtype=np.int64)
            h_s, hx, hy = model(*t[:6])
            ev[f'{mode}_h_share'] = h_s.numpy()
            ev[f'{mode}_hx'] = hx.numpy()
            ev[f'{mode}_hy'] = hy.numpy()
    for n, p in model.named_parameters():
        ev[f'param/{n}'] = p.detach().numpy().copy()
    np.savez_compressed(os.path.join(OUT, f'eval_{name}.npz'), **ev)
    print(f'[{name}] train={len(ds_tr.data)} val={len(ds_va.data)} test={len(ds_te.data)} '
          f'E_share={len(g["share_val"])} E_spec={len(g["specific_val"])} steps={n_steps}')


N_EPOCH = 3


class _Noter:
    def __init__(self):
        self.train = []

    def log_train(self, *a):
        self.train.append(a[:3])

    def __getattr__(self, name):
        return lambda *a, **k: None


def gen_trajectory(name, cfg, ref):
    """main.py:88-148 through the reference's own Trainer (trainer.py:13-83), dropout 0."""
    import shutil
    ref_dl, ref_model, ref_trainer, ref_graph, ref_metrics = ref
    tmp = tempfile.mkdtemp(prefix=f'c2dsr_traj_{name}_')
    path_raw = os.path.join(tmp, 'raw')
    path_data = os.path.join(tmp, 'data')
    os.makedirs(path_data)
    synth.make_dataset(path_raw, cfg['n_a'], cfg['n_b'], cfg['len_max'], cfg['n_train'], cfg['n_eval'],
                       seed=11, ties=True, n_min=2)
    args = make_args(cfg, path_raw, path_data)
    args.save_processed = True
    bench = [0.1124, 0.0865, 0.0574, 0.0416]
    random.seed(3407)
    torch.manual_seed(3407)
    np.random.seed(3407)
    noter = _Noter()
    tr = ref_trainer.Trainer(args, noter)
    sched = torch.optim.lr_scheduler.StepLR(tr.optimizer, step_size=args.lr_step, gamma=args.lr_gamma)
    out = {'n_epoch': np.int64(N_EPOCH)}
    for k, v in tr.model.state_dict().items():
        out[f'init/{k}'] = v.detach().numpy().copy()
    loader = tr.trainloader

    class _Rec:  # records the shuffled batch order; iteration itself is the DataLoader's
        def __init__(self, order):
            self.order = order
            self.dataset = loader.dataset

        def __iter__(self):
            for b in loader:
                self.order.append(b[0].numpy().copy())
                yield b

    for e in range(N_EPOCH):
        order = []
        tr.trainloader = _Rec(order)
        va, vb = tr.run_epoch()
        sched.step()
        ta, tb = tr.run_test()
        out[f'e{e}/order_seq_share'] = np.concatenate(order)
        out[f'e{e}/loss'] = np.asarray(noter.train[-1], dtype=np.float64)
        out[f'e{e}/val_a'] = np.asarray(va, dtype=np.int64)
        out[f'e{e}/val_b'] = np.asarray(vb, dtype=np.int64)
        out[f'e{e}/test_a'] = np.asarray(ta, dtype=np.int64)
        out[f'e{e}/test_b'] = np.asarray(tb, dtype=np.int64)
        out[f'e{e}/val_score'] = np.asarray(ref_metrics.cal_score(va, vb, bench), dtype=np.float64)
        out[f'e{e}/test_score'] = np.asarray(ref_metrics.cal_score(ta, tb, bench), dtype=np.float64)
    for n, p in tr.model.named_parameters():
        out[f'final/{n}'] = p.detach().numpy().copy()
    np.savez_compressed(os.path.join(OUT, f'traj_{name}.npz'), **out)
    dst = os.path.join(OUT, f'processed_{name}')
    os.makedirs(dst, exist_ok=True)
    for f in ('train.pkl', 'val.pkl', 'test.pkl', 'graph.pkl'):
        shutil.copy(os.path.join(path_data, f), os.path.join(dst, f))
    for f in ('items_a.txt', 'items_b.txt'):
        shutil.copy(os.path.join(path_raw, f), os.path.join(dst, f))
    print(f'[traj {name}] epochs={N_EPOCH} losses={[tuple(out[f"e{e}/loss"]) for e in range(N_EPOCH)]}')


def gen_metrics(ref):
    ref_metrics = ref[4]
    rng = np.random.default_rng(5)
    ra = rng.integers(1, 60, size=97).tolist()
    rb = rng.integers(1, 40, size=53).tolist()
    out = {'ranks_a': np.asarray(ra), 'ranks_b': np.asarray(rb)}
    for k, bm in (('fk', [0.1124, 0.0865, 0.0574, 0.0416]), ('mb', [0.0647, 0.0476, 0.0284, 0.0217])):
        out[f'score_{k}'] = np.asarray(ref_metrics.cal_score(ra, rb, bm), dtype=np.float64)
    out['metrics_a'] = np.asarray(ref_metrics.cal_metrics(ra), dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, 'metrics.npz'), **out)


def gen_fk(ref):
    """Food-Kitchen val/test processing (the only real raw files present)."""
    ref_dl = ref[0]
    a = SimpleNamespace(path_raw=os.path.join(REF, 'data/raw/Food-Kitchen'), path_data=tempfile.mkdtemp(),
                        device='cpu', batch_size=128, dataset='Food-Kitchen', n_neg_sample=999, len_max=15,
                        use_raw=True)
    a.n_item_a = 29207
    a.n_item_b = 34886
    a.n_item = a.n_item_a + a.n_item_b + 1
    a.idx_pad = a.n_item - 1
    out = {}
    random.seed(3407)
    # 'train' mode on the val file = the stand-in train set
    ds = ref_dl.CDSRDataset.__new__(ref_dl.CDSRDataset)
    ds.__dict__.update(mode='val', path_raw=a.path_raw, device='cpu', batch_size=128, dataset=a.dataset,
                       idx_pad=a.idx_pad, n_item_a=a.n_item_a, n_item_b=a.n_item_b, n_neg_sample=999, len_max=15)
    tr = ds.preprocess_train()
    arr = np.asarray(tr, dtype=np.int64)
    out['trainlike_sha256'] = np.frombuffer(hashlib.sha256(arr.tobytes()).digest(), dtype=np.uint8)
    out['trainlike_shape'] = np.asarray(arr.shape)
    out['trainlike_head'] = arr[:64]
    ev = ds.preprocess_evaluate()
    # rows are ragged only in the [1]-lists; flatten row-wise with fixed layout
    flat = np.concatenate([np.concatenate([np.asarray(x, dtype=np.int64) for x in r]) for r in ev])
    out['evallike_sha256'] = np.frombuffer(hashlib.sha256(flat.tobytes()).digest(), dtype=np.uint8)
    out['evallike_n'] = np.int64(len(ev))
    out['evallike_head'] = np.stack([np.concatenate([np.asarray(x, dtype=np.int64) for x in r]) for r in ev[:16]])
    # graph built on the val file as stand-in train file
    adj_s, adj_p = ref[3].preprocess_graph(a, os.path.join(a.path_raw, 'val_new.txt'))
    for k, adj in (('share', adj_s), ('specific', adj_p)):
        idx = adj._indices().numpy().astype(np.int64)
        val = adj._values().numpy().astype(np.float32)
        out[f'{k}_nnz'] = np.int64(val.size)
        out[f'{k}_idx_sha256'] = np.frombuffer(hashlib.sha256(idx.tobytes()).digest(), dtype=np.uint8)
        out[f'{k}_val_sha256'] = np.frombuffer(hashlib.sha256(val.tobytes()).digest(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT, 'fk_data.npz'), **out)
    # the processed file itself, as bytes, for the tests that process it again
    with open(os.path.join(a.path_raw, 'val_new.txt'), 'rb') as f:
        np.savez_compressed(os.path.join(OUT, 'fk_val_new.npz'), val_new_txt=np.frombuffer(f.read(), dtype=np.uint8))
    print(f'[fk] trainlike={arr.shape} eval={len(ev)} nnz={out["share_nnz"]}/{out["specific_nnz"]}')


D256 = dict(n_a=300, n_b=400, len_max=50, len_rec=10, d_latent=256, n_train=40, n_eval=8,
            n_gnn=1, n_attn=1, n_head=1, norm_first=False, d_bias=False, shared_item_embed=False)


def sample_idx(n):
    """the elements of a flattened tensor a d=256 fixture keeps (≤ ~4k, evenly strided)"""
    return np.arange(0, n, max(1, n // 4096), dtype=np.int64)


def gen_d256(ref):
    """The benchmarked shape (d=256, L=50, R=10) pinned by the reference itself at small
    item counts: one train_batch (dropout 0) of the reference Trainer on a synthetic raw set.  The model's
    initial parameters are not stored — torch.manual_seed(1234) before C2DSR(...) reproduces them bit for
    bit in c2dsr_amd (checked for the d=16 configs, tests/test_model_surface.py) — and the large tensors are
    kept on an even sample of their elements (sample_idx) with their full max-abs, so the fixture stays small.
    Writes tests/golden/model_d256.npz (+ the processed train lists and the graph COO)."""
    ref_dl, ref_model, ref_trainer, ref_graph, ref_metrics = ref
    cfg = D256
    tmp = tempfile.mkdtemp(prefix='c2dsr_fx_d256_')
    path_raw = os.path.join(tmp, 'raw')
    path_data = os.path.join(tmp, 'data')
    os.makedirs(path_data)
    synth.make_dataset(path_raw, cfg['n_a'], cfg['n_b'], cfg['len_max'], cfg['n_train'], cfg['n_eval'],
                       seed=17, ties=True, n_min=20)
    args = make_args(cfg, path_raw, path_data)
    random.seed(3407)
    torch.manual_seed(3407)
    np.random.seed(3407)
    ds_tr = ref_dl.CDSRDataset(args, 'train')
    out = lists_to_arrays(ds_tr.data, 'train')
    adj_s, adj_p = ref_graph.preprocess_graph(args, os.path.join(path_raw, 'train_new.txt'))
    for k, adj in (('share', adj_s), ('specific', adj_p)):
        idx = adj._indices().numpy()
        out[f'{k}_row'] = idx[0].astype(np.int64)
        out[f'{k}_col'] = idx[1].astype(np.int64)
        out[f'{k}_val'] = adj._values().numpy().astype(np.float32)
    torch.manual_seed(1234)
    model = ref_model.C2DSR(args, adj_s, adj_p)
    tr = ref_trainer.Trainer.__new__(ref_trainer.Trainer)
    tr.model = model
    tr.optimizer = torch.optim.AdamW(filter(lambda x: x.requires_grad, model.parameters()), lr=args.lr,
                                     weight_decay=args.l2, amsgrad=True)
    tr.device, tr.d_latent, tr.n_item_a, tr.n_item_b = args.device, args.d_latent, args.n_item_a, args.n_item_b
    tr.len_rec, tr.lambda_loss = args.len_rec, args.lambda_loss
    tr.label_pos = torch.ones(args.batch_size, 1)
    tr.label_neg = torch.zeros(args.batch_size, 1)
    cap = {}
    hooks = [getattr(model, nm).register_forward_hook(
        (lambda nm: lambda mod, inp, o: cap.setdefault(nm, []).append(o.detach().numpy().copy()))(nm))
        for nm in ('gnn_share', 'gnn_a', 'gnn_b', 'attn_share', 'attn_a', 'attn_b')]
    snap = {}
    real_step = tr.optimizer.step

    def step_wrapper(*a, **kw):
        snap.update({n: p.grad.detach().numpy().copy() for n, p in model.named_parameters() if p.grad is not None})
        return real_step(*a, **kw)

    tr.optimizer.step = step_wrapper
    tensors = [torch.LongTensor(np.stack([np.asarray(r[j]) for r in ds_tr.data])) for j in range(14)]
    model.train()
    tr.optimizer.zero_grad()
    model.convolve_graph()
    loss, loss_rec, loss_mi = tr.train_batch(tuple(t[:BATCH] for t in tensors))
    for h in hooks:
        h.remove()
    out.update({'s0/loss': np.float64(loss.item()), 's0/loss_rec': np.float64(loss_rec.item()),
                's0/loss_mi': np.float64(loss_mi.item()), 'batch_n': np.int64(BATCH)})
    named = {'hi_share': cap['gnn_share'][0], 'hi_a': cap['gnn_a'][0], 'hi_b': cap['gnn_b'][0],
             'h_share': cap['attn_share'][0], 'h_neg_a': cap['attn_share'][1], 'h_neg_b': cap['attn_share'][2],
             'hx': cap['attn_a'][0], 'hy': cap['attn_b'][0]}
    named.update({f'grad/{n}': g for n, g in snap.items()})
    for k, v in named.items():
        flat = v.reshape(-1).astype(np.float32)
        out[f's0/{k}'] = flat[sample_idx(flat.size)]
        out[f's0/{k}:maxabs'] = np.float64(np.abs(flat).max())
        out[f's0/{k}:numel'] = np.int64(flat.size)
    np.savez_compressed(os.path.join(OUT, 'model_d256.npz'), **out)
    print(f'[d256] train={len(ds_tr.data)} loss={loss.item():.6f} tensors={len(named)}')


# BASELINE configs[1] (C2) at its own shape: Food-Kitchen item counts, d=256, L=50, R=10, B=1024 (VERDICT r03
# next #1).  The inputs are NOT stored: they are the synthetic sequences the full-size GPU tests build
# (synth.make_sequences(2·B, seed=1, n_min=6)), written in the raw format for the reference to process; the fixture
# pins their processed form by sha256 so a test that rebuilds them through c2dsr_amd proves it fed the same batch.
C2 = dict(n_a=29207, n_b=34886, len_max=50, len_rec=10, d_latent=256, n_gnn=1, n_attn=1, n_head=1,
          norm_first=False, d_bias=False, shared_item_embed=False)
C2_BATCH = 1024


def _sha(arrs):
    h = hashlib.sha256()
    for a in arrs:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


# BASELINE configs[2] (C3) at Movie-Book item counts: 36,845 + 63,937 items, d=256, L=50,
# R=10; B=1024 — the reference's CPU step at B=2048 materialises ~33 GB of logits / log-softmax / their gradients
# per step on top of the model, more than this container's 64 GB leaves room for.  Same synthetic generator as C2.
C3 = dict(C2, n_a=36845, n_b=63937)
C3_BATCH = 1024


def gen_c2(ref, cfg=C2, B=C2_BATCH, tag='c2'):
    """One reference train_batch (dropout 0) at C2's (or, tag 'c3', C3's) full shape, stored like model_d256.npz
    (an even sample of every tensor's elements with the full max-abs) plus, for the sparse embedding-table
    gradients, a sample of their nonzero elements.  Writes tests/golden/model_<tag>.npz."""
    ref_dl, ref_model, ref_trainer, ref_graph, ref_metrics = ref
    tmp = tempfile.mkdtemp(prefix=f'c2dsr_fx_{tag}_')
    path_raw = os.path.join(tmp, 'raw')
    path_data = os.path.join(tmp, 'data')
    os.makedirs(path_data)
    seqs = synth.make_sequences(2 * B, cfg['n_a'], cfg['n_b'], cfg['len_max'], seed=1, n_min=6)
    synth.write_items(path_raw, cfg['n_a'], cfg['n_b'])
    synth.write_raw(path_raw, 'train', seqs, ties=False)
    args = make_args(cfg, path_raw, path_data)
    args.batch_size = B
    random.seed(3407)
    torch.manual_seed(3407)
    np.random.seed(3407)
    ds_tr = ref_dl.CDSRDataset(args, 'train')
    lists = [np.asarray([r[j] for r in ds_tr.data[:B]], dtype=np.int64) for j in range(14)]
    out = {'batch_n': np.int64(B), 'n_users': np.int64(2 * B), 'n_train': np.int64(len(ds_tr.data)),
           'batch_sha256': np.str_(_sha(lists))}
    adj_s, adj_p = ref_graph.preprocess_graph(args, os.path.join(path_raw, 'train_new.txt'))
    for k, adj in (('share', adj_s), ('specific', adj_p)):
        a = adj.coalesce()
        idx = a.indices().numpy()
        out[f'{k}_sha256'] = np.str_(_sha([idx[0].astype(np.int64), idx[1].astype(np.int64),
                                           a.values().numpy().astype(np.float32)]))
        out[f'{k}_nnz'] = np.int64(idx.shape[1])
    torch.manual_seed(1234)
    model = ref_model.C2DSR(args, adj_s, adj_p)
    tr = ref_trainer.Trainer.__new__(ref_trainer.Trainer)
    tr.model = model
    tr.optimizer = torch.optim.AdamW(filter(lambda x: x.requires_grad, model.parameters()), lr=args.lr,
                                     weight_decay=args.l2, amsgrad=True)
    tr.device, tr.d_latent, tr.n_item_a, tr.n_item_b = args.device, args.d_latent, args.n_item_a, args.n_item_b
    tr.len_rec, tr.lambda_loss = args.len_rec, args.lambda_loss
    tr.label_pos = torch.ones(B, 1)
    tr.label_neg = torch.zeros(B, 1)
    cap = {}
    hooks = [getattr(model, nm).register_forward_hook(
        (lambda nm: lambda mod, inp, o: cap.setdefault(nm, []).append(o.detach().numpy().copy()))(nm))
        for nm in ('gnn_share', 'gnn_a', 'gnn_b', 'attn_share', 'attn_a', 'attn_b')]
    snap = {}
    real_step = tr.optimizer.step

    def step_wrapper(*a, **kw):
        snap.update({n: p.grad.detach().numpy().copy() for n, p in model.named_parameters() if p.grad is not None})
        return real_step(*a, **kw)

    tr.optimizer.step = step_wrapper
    model.train()
    tr.optimizer.zero_grad()
    model.convolve_graph()
    loss, loss_rec, loss_mi = tr.train_batch(tuple(torch.from_numpy(x) for x in lists))
    for h in hooks:
        h.remove()
    out.update({'s0/loss': np.float64(loss.item()), 's0/loss_rec': np.float64(loss_rec.item()),
                's0/loss_mi': np.float64(loss_mi.item())})
    named = {'hi_share': cap['gnn_share'][0], 'hi_a': cap['gnn_a'][0], 'hi_b': cap['gnn_b'][0],
             'h_share': cap['attn_share'][0], 'h_neg_a': cap['attn_share'][1], 'h_neg_b': cap['attn_share'][2],
             'hx': cap['attn_a'][0], 'hy': cap['attn_b'][0]}
    named.update({f'grad/{n}': g for n, g in snap.items()})
    for k, v in named.items():
        flat = v.reshape(-1).astype(np.float32)
        out[f's0/{k}'] = flat[sample_idx(flat.size)]
        out[f's0/{k}:maxabs'] = np.float64(np.abs(flat).max())
        out[f's0/{k}:numel'] = np.int64(flat.size)
        nz = np.flatnonzero(flat)
        if k.startswith('grad/') and nz.size < flat.size // 2:  # sparse (embedding tables): sample the nonzeros
            sel = nz[sample_idx(nz.size)]
            out[f's0/{k}:nz_idx'] = sel.astype(np.int64)
            out[f's0/{k}:nz_val'] = flat[sel]
    np.savez_compressed(os.path.join(OUT, f'model_{tag}.npz'), **out)
    print(f'[{tag}] train={len(ds_tr.data)} loss={loss.item():.6f} tensors={len(named)}')


FK_EPOCHS = 2


def gen_fk_trajectory(ref):
    """north_star's metric reproduction on Food-Kitchen: main.py's loop (main.py:88-148)
    through the reference's own Trainer on the FK stand-in — the only FK interaction files present are
    data/raw/Food-Kitchen/val.txt and test_new.txt (train_new.txt is a missing blob), so
    train := val.txt and val := test := test_new.txt — at BASELINE configs[0] (C1: d=64, L=15 as main.py
    forces for FK, B=128, R=10, 999 sampled negatives), dropout 0, num_workers 0, FK_EPOCHS epochs.
    Writes tests/golden/fk_raw_{train,eval,items}.npz (the four raw input files as bytes, in three files to keep
    each small) and traj_fk.npz: per-step losses,
    per-epoch train losses, the shuffled batch order, val/test ranks, cal_metrics and cal_score."""
    ref_dl, ref_model, ref_trainer, ref_graph, ref_metrics = ref
    src = os.path.join(REF, 'data/raw/Food-Kitchen')
    tmp = tempfile.mkdtemp(prefix='c2dsr_fktraj_')
    path_raw = os.path.join(tmp, 'raw')
    path_data = os.path.join(tmp, 'data')
    os.makedirs(path_raw)
    os.makedirs(path_data)
    files = {'train_new.txt': 'val.txt', 'val_new.txt': 'test_new.txt', 'test_new.txt': 'test_new.txt',
             'items_a.txt': 'items_a.txt', 'items_b.txt': 'items_b.txt'}
    raw = {}
    for dst, f in files.items():
        data = open(os.path.join(src, f), 'rb').read()
        open(os.path.join(path_raw, dst), 'wb').write(data)
        raw[f] = np.frombuffer(data, dtype=np.uint8)
    raw = {k.replace('.', '_'): v for k, v in raw.items()}
    for part, keys in (('train', ['val_txt']), ('eval', ['test_new_txt']), ('items', ['items_a_txt', 'items_b_txt'])):
        np.savez_compressed(os.path.join(OUT, f'fk_raw_{part}.npz'), **{k: raw[k] for k in keys})
    cfg = dict(n_a=29207, n_b=34886, len_max=15, len_rec=10, d_latent=64, n_gnn=1, n_attn=1, n_head=1,
               norm_first=False, d_bias=False, shared_item_embed=False)
    args = make_args(cfg, path_raw, path_data)
    args.dataset = 'Food-Kitchen'
    args.batch_size = 128
    args.batch_size_eval = 2048
    args.n_neg_sample = 999
    bench = [0.1124, 0.0865, 0.0574, 0.0416]  # utils/constant.py:14
    random.seed(3407)
    torch.manual_seed(3407)
    np.random.seed(3407)
    noter = _Noter()
    tr = ref_trainer.Trainer(args, noter)
    sched = torch.optim.lr_scheduler.StepLR(tr.optimizer, step_size=args.lr_step, gamma=args.lr_gamma)
    out = {'n_epoch': np.int64(FK_EPOCHS)}
    steps = []
    tb_orig = tr.train_batch

    def tb(batch):
        r = tb_orig(batch)
        steps.append([float(x) for x in r])
        return r

    tr.train_batch = tb
    loader = tr.trainloader

    class _Rec:
        def __init__(self, order):
            self.order = order
            self.dataset = loader.dataset

        def __iter__(self):
            for b in loader:
                self.order.append(b[0].numpy().copy())
                yield b

    for e in range(FK_EPOCHS):
        order = []
        tr.trainloader = _Rec(order)
        va, vb = tr.run_epoch()
        sched.step()
        ta, tb_ = tr.run_test()
        out[f'e{e}/order_seq_share'] = np.concatenate(order)
        out[f'e{e}/loss'] = np.asarray(noter.train[-1], dtype=np.float64)
        out[f'e{e}/step_losses'] = np.asarray(steps, dtype=np.float64)
        steps.clear()
        for k, v in (('val_a', va), ('val_b', vb), ('test_a', ta), ('test_b', tb_)):
            out[f'e{e}/{k}'] = np.asarray(v, dtype=np.int64)
            out[f'e{e}/{k}_metrics'] = np.asarray(ref_metrics.cal_metrics(v), dtype=np.float64)
        out[f'e{e}/val_score'] = np.asarray(ref_metrics.cal_score(va, vb, bench), dtype=np.float64)
        out[f'e{e}/test_score'] = np.asarray(ref_metrics.cal_score(ta, tb_, bench), dtype=np.float64)
        print(f'[fk traj] epoch {e}: loss {out[f"e{e}/loss"]} test score {out[f"e{e}/test_score"]}', flush=True)
    np.savez_compressed(os.path.join(OUT, 'traj_fk.npz'), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='')
    ap.add_argument('--traj', action='store_true', help='only the epoch trajectories')
    ap.add_argument('--fk-traj', action='store_true', help='only the Food-Kitchen metric trajectory')
    ap.add_argument('--d256', action='store_true', help='only the d=256 / L=50 / R=10 golden step')
    ap.add_argument('--c2', action='store_true', help='only the C2-shape (FK items, d=256, L=50, B=1024) golden step')
    ap.add_argument('--c3', action='store_true', help='only the C3-shape (MB items, d=256, L=50, B=1024) golden step')
    opt = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(4)
    ref = ref_import()
    if opt.d256:
        gen_d256(ref)
        return
    if opt.c2:
        torch.set_num_threads(8)
        gen_c2(ref)
        return
    if opt.c3:
        torch.set_num_threads(8)
        gen_c2(ref, C3, C3_BATCH, 'c3')
        return
    if opt.fk_traj:
        torch.set_num_threads(8)
        gen_fk_trajectory(ref)
        return
    if opt.traj:
        for name in ('base', 'var'):
            gen_trajectory(name, CONFIGS[name], ref)
        return
    for name, cfg in CONFIGS.items():
        if opt.only and name != opt.only:
            continue
        gen_config(name, cfg, ref)
    if not opt.only:
        gen_metrics(ref)
        gen_fk(ref)


if __name__ == '__main__':
    main()
