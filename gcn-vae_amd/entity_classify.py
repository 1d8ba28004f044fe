"""R-GCN entity classification (kgvae/entity_classify.py, byte-identical to baselines/rgcn/entity_classify.py) on gfx950.

    python -m gcn_vae_amd.entity_classify -d aifb-synthetic --testing --gpu 0
    python -m gcn_vae_amd.entity_classify -d am-synthetic --n-bases 40 --n-hidden 10 --l2norm 5e-4 --testing --gpu 0

``EntityClassify`` keeps the reference's classes, layer order, initialisers and state_dict keys: integer-id input layer
``RelGraphConv(num_nodes, h, R, "basis", nb, relu, self_loop, dropout)``, ``n_layers - 2`` hidden basis layers, and an output
layer ``RelGraphConv(h, C, R, "basis", nb, softmax(dim=1), self_loop)`` whose softmax probabilities ``forward`` returns.  The
reference trains ``F.cross_entropy`` on those probabilities -- a second softmax -- and that is kept: its published accuracies
come from it.  Differences:

* with ``num_bases < num_rels`` the input layer builds each edge's row from the basis planes (``fused_basis_select``) instead
  of the (R, num_nodes, h) weight; ``--materialise-basis`` selects the materialised path;
* the softmax, both losses and both accuracies come from one head launch (``loss_and_metrics``), Adam with ``--l2norm`` is
  ``optim.FlatAdam(weight_decay=...)``;
* ``--gpu`` must name a ROCm device: there is no CPU path.  Datasets: ``data.load_entity_data``.
"""
import argparse
import time
from functools import partial

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .data import load_entity_data
from .encoders import BaseRGCN
from .graph import KGraph
from .layers import RelGraphConv
from .optim import FlatAdam


class EntityClassify(BaseRGCN):
    def __init__(self, num_nodes, h_dim, out_dim, num_rels, num_bases=-1, num_hidden_layers=1, dropout=0, use_self_loop=False,
                 use_cuda=False, materialise_basis=False):
        super().__init__(num_nodes, h_dim, out_dim, num_rels, num_bases, num_hidden_layers=num_hidden_layers, dropout=dropout,
                         use_self_loop=use_self_loop, use_cuda=use_cuda)
        self.layers[0].fused_basis_select = not materialise_basis

    def create_features(self):
        features = torch.arange(self.num_nodes)
        if self.use_cuda:
            features = features.cuda()
        return features

    def build_input_layer(self):
        return RelGraphConv(self.num_nodes, self.h_dim, self.num_rels, "basis", self.num_bases, activation=F.relu,
                            self_loop=self.use_self_loop, dropout=self.dropout)

    def build_hidden_layer(self, idx):
        return RelGraphConv(self.h_dim, self.h_dim, self.num_rels, "basis", self.num_bases, activation=F.relu,
                            self_loop=self.use_self_loop, dropout=self.dropout)

    def build_output_layer(self):
        return RelGraphConv(self.h_dim, self.out_dim, self.num_rels, "basis", self.num_bases,
                            activation=partial(F.softmax, dim=1), self_loop=self.use_self_loop)

    def logits(self, g, h, r, norm):
        """The output layer's rows before its softmax."""
        for layer in self.layers[:-1]:
            h = layer(g, h, r, norm)
        out = self.layers[-1]
        act, out.activation = out.activation, None
        try:
            return out(g, h, r, norm)
        finally:
            out.activation = act

    def forward(self, g, h, r, norm):
        return ops.softmax_rows(self.logits(g, h, r, norm))

    def loss_and_metrics(self, g, h, r, norm, labels, train_idx, val_idx=None, test_idx=None):
        """(p, losses, counts): the probabilities of every row, F.cross_entropy(p[idx], labels[idx]) for each of up to three
        disjoint index sets (losses[0] is the training loss; differentiable) and the rows whose argmax is the label (int32)."""
        return ops.ec_head(self.logits(g, h, r, norm), labels, train_idx, val_idx, test_idx)


def head_rule(h, labels, sets, glosses=None, grad_p=None):
    """The rule of ``ops.ec_head`` (gv_ec_head_fwd / _bwd) in plain torch, any device and dtype, with the backward written out:
        p = softmax(h);  losses[s] = mean over i in set s of logsumexp(p_i) - p_i[y_i]   (F.cross_entropy on p; NaN if empty)
        counts[s] = #{i in s : argmax(p_i) == y_i}, ties to the lowest column
        dh = p * (dp - <dp, p>),  dp = grad_p + sum_s [i in s] glosses[s] / |s| * (softmax(p_i) - onehot(y_i))
    Returns (p, losses (3,), counts (3,) int64, dh); dh is None when neither glosses nor grad_p is given."""
    sets = list(sets) + [None] * (3 - len(sets))
    p = torch.softmax(h, dim=1)
    losses, counts = [], []
    dp = None if grad_p is None else grad_p.to(h.dtype).clone()
    if glosses is not None and dp is None:
        dp = torch.zeros_like(h)
    for s, idx in enumerate(sets):
        if idx is None or idx.numel() == 0:
            losses.append(float('nan'))
            counts.append(0)
            continue
        ps, y = p[idx], labels[idx]
        losses.append((torch.logsumexp(ps, 1) - ps.gather(1, y.view(-1, 1)).squeeze(1)).mean())
        counts.append(int((ps.argmax(1) == y).sum()))
        if glosses is not None:
            dp[idx] += glosses[s] / idx.numel() * (torch.softmax(ps, 1) - F.one_hot(y, h.shape[1]).to(h.dtype))
    losses = torch.stack([torch.as_tensor(v, dtype=h.dtype, device=h.device) for v in losses])
    dh = None if dp is None else p * (dp - (dp * p).sum(1, keepdim=True))
    return p, losses, torch.tensor(counts, dtype=torch.int64), dh


def main(args):
    if args.gpu < 0 or not torch.cuda.is_available():
        raise RuntimeError('gcn_vae_amd runs on a ROCm device only (pass --gpu N on an MI355X box); there is no CPU path')
    torch.cuda.set_device(args.gpu)
    dev = torch.device('cuda', args.gpu)
    data = load_entity_data(args.dataset, bfs_level=args.bfs_level, relabel=args.relabel)
    num_nodes, num_rels, num_classes = data.num_nodes, data.num_rels, data.num_classes
    train_idx, test_idx = data.train_idx, data.test_idx

    # the reference's split: the first fifth of train_idx validates; --testing validates on the training set itself
    if args.validation:
        val_idx = train_idx[:len(train_idx) // 5]
        train_idx = train_idx[len(train_idx) // 5:]
    else:
        val_idx = train_idx
    same_val = val_idx is train_idx

    feats = torch.arange(num_nodes, device=dev)
    edge_type = torch.from_numpy(data.edge_type).to(dev)
    edge_norm = torch.from_numpy(data.edge_norm).unsqueeze(1).to(dev)
    labels = torch.from_numpy(data.labels).view(-1).to(dev)
    train_t = torch.from_numpy(np.asarray(train_idx, dtype=np.int64)).to(dev)
    val_t = None if same_val else torch.from_numpy(np.asarray(val_idx, dtype=np.int64)).to(dev)
    test_t = torch.from_numpy(np.asarray(test_idx, dtype=np.int64)).to(dev)

    g = KGraph()
    g.add_nodes(num_nodes)
    g.add_edges(data.edge_src, data.edge_dst)

    if args.seed is not None:
        torch.manual_seed(args.seed)
    model = EntityClassify(len(g), args.n_hidden, num_classes, num_rels, num_bases=args.n_bases,
                           num_hidden_layers=args.n_layers - 2, dropout=args.dropout, use_self_loop=args.use_self_loop,
                           use_cuda=True, materialise_basis=args.materialise_basis).to(dev)
    optimizer = FlatAdam(model.parameters(), lr=args.lr, weight_decay=args.l2norm)

    print("start training...")
    forward_time, backward_time = [], []
    model.train()
    for epoch in range(args.n_epochs):
        optimizer.zero_grad()
        torch.cuda.synchronize()
        t0 = time.time()
        _, losses, counts = model.loss_and_metrics(g, feats, edge_type, edge_norm, labels, train_t, val_t)
        loss = losses[0]
        torch.cuda.synchronize()
        t1 = time.time()
        loss.backward()
        optimizer.step()
        torch.cuda.synchronize()
        t2 = time.time()
        forward_time.append(t1 - t0)
        backward_time.append(t2 - t1)
        print("Epoch {:05d} | Train Forward Time(s) {:.4f} | Backward Time(s) {:.4f}".
              format(epoch, forward_time[-1], backward_time[-1]))
        lv, cv = losses.detach().cpu(), counts.cpu()
        train_acc = cv[0].item() / len(train_idx)
        val_loss, val_acc = (lv[0].item(), train_acc) if same_val else (lv[1].item(), cv[1].item() / len(val_idx))
        print("Train Accuracy: {:.4f} | Train Loss: {:.4f} | Validation Accuracy: {:.4f} | Validation loss: {:.4f}".
              format(train_acc, lv[0].item(), val_acc, val_loss))
    print()

    model.eval()
    with torch.no_grad():
        _, losses, counts = model.loss_and_metrics(g, feats, edge_type, edge_norm, labels, test_t)
    test_acc = counts[0].item() / len(test_idx)
    print("Test Accuracy: {:.4f} | Test loss: {:.4f}".format(test_acc, losses[0].item()))
    print()

    print("Mean forward time: {:4f}".format(np.mean(forward_time[len(forward_time) // 4:])))
    print("Mean backward time: {:4f}".format(np.mean(backward_time[len(backward_time) // 4:])))
    return test_acc


def build_parser():
    parser = argparse.ArgumentParser(description='RGCN')
    parser.add_argument("--dropout", type=float, default=0, help="dropout probability")
    parser.add_argument("--n-hidden", type=int, default=16, help="number of hidden units")
    parser.add_argument("--gpu", type=int, default=-1, help="gpu")
    parser.add_argument("--lr", type=float, default=1e-2, help="learning rate")
    parser.add_argument("--n-bases", type=int, default=-1, help="number of filter weight matrices, default: -1 [use all]")
    parser.add_argument("--n-layers", type=int, default=2, help="number of propagation rounds")
    parser.add_argument("-e", "--n-epochs", type=int, default=50, help="number of training epochs")
    parser.add_argument("-d", "--dataset", type=str, required=True, help="dataset to use")
    parser.add_argument("--l2norm", type=float, default=0, help="l2 norm coef")
    parser.add_argument("--relabel", default=False, action='store_true', help="remove untouched nodes and relabel")
    parser.add_argument("--use-self-loop", default=False, action='store_true',
                        help="include self feature as a special relation")
    fp = parser.add_mutually_exclusive_group(required=False)
    fp.add_argument('--validation', dest='validation', action='store_true')
    fp.add_argument('--testing', dest='validation', action='store_false')
    parser.set_defaults(validation=True)
    parser.add_argument("--materialise-basis", default=False, action='store_true',
                        help="input layer through the full (R, num_nodes, h) weight instead of the fused basis rows "
                             "(for comparison; refused past 2^31 weight elements); not a reference flag")
    parser.add_argument("--seed", type=int, default=None,
                        help="seed torch's generator before the model is built (reproducible runs); default: unseeded, as "
                             "the reference; not a reference flag")
    return parser


if __name__ == '__main__':
    cli = build_parser().parse_args()
    print(cli)
    cli.bfs_level = cli.n_layers + 1     # pruning used nodes for memory
    main(cli)
