#!/usr/bin/env python3
"""Entity-classification epoch time (forward + head + backward + Adam) on the four synthetic RDF-sized datasets with the
hyperparameters of the reference's baselines/rgcn/README.md, fused basis input layer against the materialised (R, N, h) weight,
with peak device memory, and the fused kernels' algorithmic bytes against 8 TB/s.  Each (dataset, input layer) runs in a child
process of its own under a time limit, so a run that does not fit or takes too long is recorded as such.

    python tools/ec_bench.py [--datasets aifb,mutag,bgs,am] [--epochs 10] [--warmup 3] [--limit 900] [--cpu-epochs 5]

Epoch time: device events around each epoch, median over --epochs after --warmup.  CPU baseline: the torch oracle
(oracle.rgcn op sequence + F.cross_entropy + torch.optim.Adam) on aifb-synthetic."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

README = {     # baselines/rgcn/README.md: n_bases, n_hidden, l2norm, relabel (n_layers 2, --testing)
    'aifb': dict(nb=-1, h=16, l2=0.0, relabel=False),
    'mutag': dict(nb=30, h=16, l2=5e-4, relabel=False),
    'bgs': dict(nb=40, h=16, l2=5e-4, relabel=True),
    'am': dict(nb=40, h=10, l2=5e-4, relabel=False),
}
HBM = 8e12


def one(ds, mode, epochs, warmup):
    from gcn_vae_amd import lib
    from gcn_vae_amd.data import load_entity_data
    from gcn_vae_amd.entity_classify import EntityClassify
    from gcn_vae_amd.graph import KGraph
    from gcn_vae_amd.optim import FlatAdam
    cfg = README[ds]
    t0 = time.time()
    d = load_entity_data(ds + '-synthetic', bfs_level=3, relabel=cfg['relabel'])
    load_s = time.time() - t0
    dev = torch.device('cuda', 0)
    g = KGraph()
    g.add_nodes(d.num_nodes)
    g.add_edges(d.edge_src, d.edge_dst)
    feats = torch.arange(d.num_nodes, device=dev)
    et = torch.from_numpy(d.edge_type).to(dev)
    en = torch.from_numpy(d.edge_norm).unsqueeze(1).to(dev)
    labels = torch.from_numpy(d.labels).to(dev)
    tr = torch.from_numpy(d.train_idx).to(dev)
    torch.manual_seed(0)
    model = EntityClassify(d.num_nodes, cfg['h'], d.num_classes, d.num_rels, num_bases=cfg['nb'], num_hidden_layers=0,
                           use_self_loop=False, use_cuda=True, materialise_basis=(mode == 'materialised')).to(dev)
    opt = FlatAdam(model.parameters(), lr=1e-2, weight_decay=cfg['l2'])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()

    def epoch():
        opt.zero_grad()
        _, losses, _ = model.loss_and_metrics(g, feats, et, en, labels, tr)
        losses[0].backward()
        opt.step()
        return losses

    t0 = time.time()
    epoch()                   # first epoch: index and plan building
    torch.cuda.synchronize()
    first_s = time.time() - t0
    for _ in range(warmup):
        epoch()
    times = []
    for _ in range(epochs):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        losses = epoch()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    out = dict(dataset=ds, mode=mode, nodes=d.num_nodes, rels=d.num_rels, edges=int(len(d.edge_src)), nb=model.layers[0].num_bases,
               h=cfg['h'], epoch_ms_median=float(np.median(times)), epoch_ms_min=float(np.min(times)), epochs=epochs,
               peak_gib=torch.cuda.max_memory_allocated() / 2 ** 30, first_epoch_s=first_s, load_s=load_s,
               loss=float(losses[0]))
    layer = model.layers[0]
    if mode == 'fused' and layer.num_bases < layer.num_rels:
        lib.TIMER = lib.KernelTimer()
        for _ in range(3):
            epoch()
        res = lib.TIMER.results_ms()
        lib.TIMER = None
        plan = _plan_of(g, et, layer, feats)
        nr, ng, nb, h, r = plan['n_runs'], plan['n_groups'], layer.num_bases, layer.out_feat, layer.num_rels
        fwd_bytes = 4 * (ng * nb * h + r * nb + 2 * nr + nr * h)
        bwd_bytes = 4 * (nr * h + 2 * nr + 2 * ng + 2 * ng * nb * h) + 4 * (ng * nb * h + nr * h + 2 * nr + nr * nb) + 4 * nr * nb
        for tag, nbytes in (('ec_basis_fwd', fwd_bytes), ('ec_basis_bwd', bwd_bytes)):
            ms = float(np.median(res[tag]))
            out[tag] = dict(ms=ms, bytes=nbytes, tb_s=nbytes / ms / 1e9, share_of_8tbs=nbytes / ms / 1e9 / (HBM / 1e12))
        out.update(runs=nr, id_groups=ng)
    print('RESULT ' + json.dumps(out), flush=True)


def _plan_of(g, et, layer, feats):
    from gcn_vae_amd.graph import graph_index_of
    gidx = graph_index_of(g, feats.device)
    ridx = gidx.relation_index(et, layer.num_rels)
    return next(iter(ridx.__dict__['_basis_select'].values()))


def cpu_baseline(epochs):
    from gcn_vae_amd.data import load_entity_data
    from oracle import rgcn as orgcn
    d = load_entity_data('aifb-synthetic', bfs_level=3)
    cfg = README['aifb']
    src, dst = torch.from_numpy(d.edge_src), torch.from_numpy(d.edge_dst)
    et, en = torch.from_numpy(d.edge_type), torch.from_numpy(d.edge_norm).view(-1, 1)
    labels, tr = torch.from_numpy(d.labels), torch.from_numpy(d.train_idx)
    torch.manual_seed(0)
    p1 = {k: torch.nn.Parameter(v) for k, v in orgcn.init_params(d.num_nodes, cfg['h'], d.num_rels, 'basis', None).items()}
    p2 = {k: torch.nn.Parameter(v) for k, v in orgcn.init_params(cfg['h'], d.num_classes, d.num_rels, 'basis', None).items()}
    opt = torch.optim.Adam(list(p1.values()) + list(p2.values()), lr=1e-2, weight_decay=cfg['l2'])
    feats = torch.arange(d.num_nodes)
    times = []
    for i in range(epochs + 1):
        t0 = time.perf_counter()
        opt.zero_grad()
        h = orgcn.rel_graph_conv(feats, src, dst, et, en, p1, 'basis', None, torch.relu)
        p = F.softmax(orgcn.rel_graph_conv(h, src, dst, et, en, p2, 'basis', None), dim=1)
        F.cross_entropy(p[tr], labels[tr]).backward()
        opt.step()
        if i:
            times.append((time.perf_counter() - t0) * 1e3)
    return dict(dataset='aifb', mode='cpu-oracle', threads=torch.get_num_threads(), epoch_ms_median=float(np.median(times)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--datasets', default='aifb,mutag,bgs,am')
    ap.add_argument('--epochs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--limit', type=int, default=900, help='seconds per child run')
    ap.add_argument('--cpu-epochs', type=int, default=5)
    ap.add_argument('--one', nargs=2, metavar=('DATASET', 'MODE'), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(args.one[0], args.one[1], args.epochs, args.warmup)
    rows = []
    for ds in args.datasets.split(','):
        modes = ['fused', 'materialised'] if README[ds]['nb'] > 0 else ['materialised']     # nb = R: no basis to fuse
        for mode in modes:
            cmd = ['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--one', ds, mode,
                   '--epochs', str(args.epochs), '--warmup', str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = [x for x in r.stdout.splitlines() if x.startswith('RESULT ')]
            if r.returncode == 0 and line:
                row = json.loads(line[-1][7:])
            else:
                tail = (r.stderr or r.stdout).strip().splitlines()[-1:] or ['']
                row = dict(dataset=ds, mode=mode, failed=r.returncode, reason=tail[0][-300:])
            rows.append(row)
            print(json.dumps(row), flush=True)
            # a run that does not fit ends with a Python exception (status 1) naming torch.OutOfMemoryError, or with the layer's
            # ValueError for a weight past 2^31 elements; anything else (a fault, an abort, a time limit) ends the bench here
            refused = r.returncode == 1 and ('OutOfMemoryError' in r.stderr or 'materialised basis weight' in r.stderr)
            if r.returncode != 0 and not refused:
                print(json.dumps(dict(stopped=f'{ds}/{mode} ended with status {r.returncode}; no further GPU runs')), flush=True)
                return 1
    if args.cpu_epochs:
        row = cpu_baseline(args.cpu_epochs)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
