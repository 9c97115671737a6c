"""Micro-benchmark of the full-catalogue top-K / full-rank sweep (csrc/topk.hip through ops.full_topk, with target,
k = 20, fp32 inputs) at the benchmark configurations' head shapes, next to the materialising path a user would write
today on the same device: torch.addmm in fp32 ([B, n] scores), torch.topk and a `>`-count.

Per shape: HIP-event times (warm-up, then the median of REPS timed runs of ITERS calls each, clocks as found), the
sweep's achieved TFLOP/s (executed: 3 MFMA products, 6·B·n·d flops; credited: 2·B·n·d), the score-matrix bytes the
materialising path allocates and the workspace bytes of the fused one.  Writes profiles/topk_micro.json.
usage: python tools/topk_micro.py [out.json]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from c2dsr_amd import ops  # noqa: E402
from c2dsr_amd._lib import lib  # noqa: E402

SHAPES = [  # bench.py CONFIGS: (label, B, n, d)
    ('Movie-Book head b', 2048, 63937, 256),
    ('Food-Kitchen head a', 1024, 29207, 256),
    ('Food-Kitchen head b', 1024, 34886, 256),
]
K, WARMUP, REPS, ITERS = 20, 3, 7, 5


def timed(fn):
    """median over REPS of the mean time (µs) of ITERS back-to-back calls"""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / ITERS * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'topk_micro.json')
    dev = torch.device('cuda')
    torch.manual_seed(0)
    rows = []
    for label, B, n, d in SHAPES:
        q = torch.randn(B, d, device=dev) + torch.randn(B, d, device=dev)
        W = torch.randn(n, d, device=dev) * 0.1
        b = torch.randn(n, device=dev)
        t = torch.randint(0, n, (B,), device=dev)
        ns = int(lib.raw('c2dsr_full_topk_splits')(B, n))

        def fused():
            return ops.full_topk(q, W, b, K, target=t)

        def materialised():
            s = torch.addmm(b, q, W.t())
            v, i = torch.topk(s, K, dim=1)
            r = 1 + (s > s.gather(1, t[:, None])).sum(1)
            return i, v, r

        ids, sc, rk = fused()
        i2, v2, r2 = materialised()
        agree = float((ids == i2).float().mean())  # the two paths round differently: a sanity figure, not a check
        rank_agree = float((rk.long() == r2).float().mean())
        tf, tf_lo, tf_hi = timed(fused)
        tm, tm_lo, tm_hi = timed(materialised)
        flops = 2.0 * B * n * d
        rows.append(dict(
            shape=label, B=B, n=n, d=d, k=K, n_split=ns,
            fused_us=round(tf, 1), fused_us_min_max=[round(tf_lo, 1), round(tf_hi, 1)],
            materialised_us=round(tm, 1), materialised_us_min_max=[round(tm_lo, 1), round(tm_hi, 1)],
            fused_tflops_executed=round(3 * flops / tf / 1e6, 1), fused_tflops_credited=round(flops / tf / 1e6, 1),
            fused_includes='q image, cached W image, sweep, merge',
            materialised_score_bytes=4 * B * n,
            fused_workspace_bytes=int(lib.raw('c2dsr_full_topk_workspace')(B, n, K, ns)),
            topk_id_agreement=round(agree, 5), rank_agreement=round(rank_agree, 5)))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(tool='tools/topk_micro.py', device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS,
               iters_per_rep=ITERS, statistic='median of reps (min, max alongside); clocks as found', rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
