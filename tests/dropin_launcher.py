"""A launcher in the manner of the reference's main.py, for tests/test_dropin_main.py (copied there as ``main.py``
into a directory that holds the dropin/ files): it knows nothing of process groups, gives every process the same
``args.device``, imports ``Trainer`` from the ``trainer`` module beside it and builds ``Trainer(args, noter)`` — the
process group and the rank's device are the drop-in Trainer's business.  The options and the Namespace fields are
those main.py hands to the Trainer; the processed data is read from data/<dataset>/ under the
working directory."""
import argparse
import os
import random

import numpy as np
import torch

from trainer import Trainer


class Noter:
    def log_msg(self, msg):
        print(msg, flush=True)

    def log_train(self, *a):
        print('train', *a, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cuda', default='0')
    ap.add_argument('--seed', type=int, default=3407)
    ap.add_argument('--n_epoch', type=int, default=200)
    ap.add_argument('--batch_size', type=int, default=512)
    ap.add_argument('--batch_size_eval', type=int, default=2048)
    ap.add_argument('--num_workers', type=int, default=1)
    ap.add_argument('--use_raw', action='store_true')
    ap.add_argument('--n_neg_sample', type=int, default=999)
    ap.add_argument('--len_rec', type=int, default=10)
    ap.add_argument('--d_latent', type=int, default=128)
    ap.add_argument('--shared_item_embed', action='store_true')
    ap.add_argument('--d_bias', action='store_true')
    ap.add_argument('--n_gnn', type=int, default=1)
    ap.add_argument('--dropout_gnn', type=float, default=0.2)
    ap.add_argument('--n_attn', type=int, default=1)
    ap.add_argument('--n_head', type=int, default=1)
    ap.add_argument('--dropout_attn', type=float, default=0.2)
    ap.add_argument('--norm_first', action='store_true')
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--l2', type=float, default=5e-4)
    ap.add_argument('--lr_gamma', type=float, default=0.5)
    ap.add_argument('--lr_step', type=int, default=10)
    ap.add_argument('--lambda_loss', type=float, default=0.7)
    args = ap.parse_args()
    args.dataset, args.len_max = 'Food-Kitchen', 15
    args.device = torch.device('cpu' if args.cuda == 'cpu' else 'cuda:' + args.cuda)
    args.path_data = os.path.join(os.getcwd(), 'data', args.dataset)
    args.path_raw = os.path.join(os.getcwd(), 'data', 'raw', args.dataset)

    random.seed(args.seed)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)

    noter = Noter()
    trainer = Trainer(args, noter)
    scheduler = torch.optim.lr_scheduler.StepLR(trainer.optimizer, step_size=args.lr_step, gamma=args.lr_gamma)
    for epoch in range(1, args.n_epoch + 1):
        noter.log_msg(f'\n[Epoch {epoch}]')
        trainer.run_epoch()
        scheduler.step()


if __name__ == '__main__':
    main()
