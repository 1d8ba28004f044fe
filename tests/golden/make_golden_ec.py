#!/usr/bin/env python3
"""Generate tests/golden/entity_classify.npz and entity_classify_cli.json by IMPORTING THE REFERENCE's entity classifier.

Runs only where the reference tree is present (the GPU box never runs this).  ``kgvae/entity_classify.py`` is imported from
where it lies under the ``dgl`` stand-in of ``oracle/dgl_shim.py``, as make_golden.py does; only inputs and outputs are
written.  The stand-in has no ``load_data(name, bfs_level=, relabel=)``: the graph comes from this package's own loader
(``synthetic-ec``, host numpy) and is stored with the fixture.

    python tests/golden/make_golden_ec.py

entity_classify.npz, per configuration tag L2 / L3 (2 and 3 layers; num_bases < num_rels, self-loops, dropout 0):
  <tag>.init.<key>   the seeded model's initial state dict          <tag>.probs   forward probabilities (N, C)
  <tag>.loss         F.cross_entropy(probs[train_idx], labels[...])  <tag>.grad.<key>  every parameter gradient
  <tag>.adam3.<key>  parameters after 3 steps of Adam(lr, weight_decay=5e-4)
  graph.*            edge_src / edge_dst / edge_type / edge_norm / labels / train_idx, num_nodes, num_rels, num_classes
entity_classify_cli.json: the reference parser's options, defaults and types, and the defaults it parses to.
"""
import json
import os
import runpy
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import argparse  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import dgl_shim  # noqa: E402

REF = '/root/reference/kgvae'
dgl_shim.install()
sys.path.insert(0, REF)
import entity_classify as ref_ec  # noqa: E402

torch.autograd.set_detect_anomaly(False)   # the reference switches it on at import (model.py:10)

DATASET = 'synthetic-ec:160:5:900:3:40:11'     # 160 nodes, 10 relations with inverses, 3 classes
CONFIGS = {'L2': dict(n_layers=2, h=8, nb=3, seed=5), 'L3': dict(n_layers=3, h=6, nb=4, seed=6)}
LR, WD = 1e-2, 5e-4


def npy(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def build(data, cfg):
    torch.manual_seed(cfg['seed'])
    return ref_ec.EntityClassify(data.num_nodes, cfg['h'], data.num_classes, data.num_rels, num_bases=cfg['nb'],
                                 num_hidden_layers=cfg['n_layers'] - 2, dropout=0.0, use_self_loop=True, use_cuda=False)


def gen_model():
    from gcn_vae_amd.data import load_entity_data
    data = load_entity_data(DATASET, bfs_level=None)
    out = {'graph.edge_src': data.edge_src, 'graph.edge_dst': data.edge_dst, 'graph.edge_type': data.edge_type,
           'graph.edge_norm': data.edge_norm, 'graph.labels': data.labels, 'graph.train_idx': data.train_idx,
           'graph.num_nodes': np.int64(data.num_nodes), 'graph.num_rels': np.int64(data.num_rels),
           'graph.num_classes': np.int64(data.num_classes)}
    g = dgl_shim.graphs.SimpleGraph()
    g.add_nodes(data.num_nodes)
    g.add_edges(data.edge_src, data.edge_dst)
    feats = torch.arange(data.num_nodes)
    et = torch.from_numpy(data.edge_type)
    en = torch.from_numpy(data.edge_norm).unsqueeze(1)
    labels = torch.from_numpy(data.labels)
    tr = torch.from_numpy(data.train_idx)
    for tag, cfg in CONFIGS.items():
        model = build(data, cfg)
        for k, v in model.state_dict().items():
            out[f'{tag}.init.{k}'] = v
        logits = model(g, feats, et, en)
        loss = F.cross_entropy(logits[tr], labels[tr])
        loss.backward()
        out[f'{tag}.probs'] = logits
        out[f'{tag}.loss'] = loss
        for k, p in model.named_parameters():
            out[f'{tag}.grad.{k}'] = p.grad
        model = build(data, cfg)
        opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=WD)
        for _ in range(3):
            opt.zero_grad()
            logits = model(g, feats, et, en)
            F.cross_entropy(logits[tr], labels[tr]).backward()
            opt.step()
        for k, p in model.named_parameters():
            out[f'{tag}.adam3.{k}'] = p
        print(f'{tag}: loss {float(loss):.6f}, keys {sorted(model.state_dict())}')
    path = os.path.join(HERE, 'entity_classify.npz')
    np.savez_compressed(path, **{k: npy(v) for k, v in out.items()})
    print(f'wrote entity_classify.npz: {os.path.getsize(path) / 1024:.1f} kB')


class _Captured(Exception):
    pass


def gen_cli():
    """Run the reference script's __main__ block up to parse_args and keep its parser."""
    box = {}
    orig = argparse.ArgumentParser.parse_args

    def grab(self, *a, **k):
        box['parser'] = self
        raise _Captured()

    argparse.ArgumentParser.parse_args = grab
    try:
        runpy.run_path(os.path.join(REF, 'entity_classify.py'), run_name='__main__')
    except _Captured:
        pass
    finally:
        argparse.ArgumentParser.parse_args = orig
    parser = box['parser']
    options = []
    for a in parser._actions:
        if isinstance(a, argparse._HelpAction):
            continue
        options.append(dict(option_strings=list(a.option_strings), dest=a.dest, default=a.default,
                            type=None if a.type is None else a.type.__name__, action=type(a).__name__,
                            const=a.const, required=bool(a.required)))
    groups = [sorted(x.dest for x in g._group_actions) for g in parser._mutually_exclusive_groups]
    parsed = vars(parser.parse_args(['-d', 'x']))
    manifest = dict(options=options, mutually_exclusive=groups, defaults=parsed)
    with open(os.path.join(HERE, 'entity_classify_cli.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'wrote entity_classify_cli.json: {len(options)} options')


if __name__ == '__main__':
    gen_model()
    gen_cli()
