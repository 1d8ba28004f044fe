"""Knowledge-graph datasets.

``load_data(name)`` returns an object with ``num_nodes, num_rels, train, valid, test`` ((n,3) int64
arrays of (subject, relation, object)) as ``dgl.contrib.data.load_data`` did for the reference
(kgvae/link_predict.py:105-110).  Files are read from ``$GCNVAE_DATA`` or ``~/.dgl/<name>/`` in the
DGL-0.4 layout the reference's own code assumes (kgvae/utils.py:249-256): ``entities.dict`` /
``relations.dict`` with ``id<TAB>name`` lines and ``train.txt`` / ``valid.txt`` / ``test.txt`` with
``subject<TAB>relation<TAB>object`` names.  No dataset ships with this repo and there is no network
here, so ``name`` may also be ``synthetic:<entities>:<relations>:<train>[:<valid>:<test>[:<seed>]]``
(Zipf(0.8) endpoints -- the hub skew of FB15k-237 -- and uniform relations).

``load_entity_data(name, bfs_level=3, relabel=False)`` is the entity-classification counterpart (the RDF datasets of
kgvae/entity_classify.py:46-67).  It returns an object with ``num_nodes, num_rels, num_classes, labels, train_idx, test_idx,
edge_src, edge_dst, edge_type, edge_norm`` (numpy) and ``old_ids`` (the original id of every node kept).  Names:

* ``aifb-synthetic``, ``mutag-synthetic``, ``bgs-synthetic``, ``am-synthetic``: seeded graphs at the published R-GCN sizes
  (entities / relations / triples / classes / labelled nodes, ``EC_SIZES``);
* ``synthetic-ec:<nodes>:<rels>:<triples>:<classes>:<labelled>[:<seed>]``;
* a directory ``$GCNVAE_DATA/<name>/`` (or ``~/.dgl/<name>/``) holding ``graph.npz`` with arrays ``src``, ``dst``, ``etype``
  (one entry per triple (s, r, o), relation ids in [0, num_rels)) and scalars ``num_nodes``, ``num_rels``, plus ``labels.npy``
  (int64, one per node; -1 where unlabelled), ``train_idx.npy`` and ``test_idx.npy`` (int64 node ids).  ``save_entity_dir``
  writes this layout.

Rules, the same for every source:

* inverse edges -- triple (s, r, o) gives the edges s -> o of type r and o -> s of type r + R, so ``num_rels`` is 2R;
* ``edge_norm`` = 1 / (number of edges of the same type into the same destination), c_{i,r} of the R-GCN paper, computed
  before any pruning; edges are ordered by (destination, source, type);
* pruning, ``bfs_level`` = n_layers + 1 as the reference passes it: an edge is kept iff its destination lies within
  n_layers - 1 reverse hops of a labelled node -- exactly the edges an n_layers-deep model's labelled outputs depend on;
* ``relabel``: nodes that are neither labelled nor an endpoint of a kept edge are dropped, the rest renumbered in increasing
  old-id order.

Synthetic labels are planted so that structure decides them: the first C * k relations (k = min(2, R // C)) are reserved,
class c owning relations c*k .. c*k + k - 1; every labelled node of class c receives three extra in-edges (triples (s, r, v)
from Zipf-drawn sources s) of its class's relations, and the ordinary triples use only the other relations.  A model that can
tell the relation types arriving at a node can therefore learn the classes; nothing else carries them.  The labelled nodes are
drawn uniformly, classes uniformly, and split 80 / 20 into train and test in a seeded random order.
"""
import os

import numpy as np

FB15K237 = dict(num_nodes=14541, num_rels=237, n_train=272115, n_valid=17535, n_test=20466)
WN18RR = dict(num_nodes=40943, num_rels=11, n_train=86835, n_valid=3034, n_test=3134)


class KGDataset:
    def __init__(self, name, num_nodes, num_rels, train, valid, test):
        self.name, self.num_nodes, self.num_rels = name, int(num_nodes), int(num_rels)
        self.train, self.valid, self.test = train, valid, test


def synthetic_kg(num_nodes, num_rels, n_train, n_valid=0, n_test=0, seed=0, zipf=0.8, name='synthetic'):
    rs = np.random.RandomState(seed)
    p = (np.arange(num_nodes) + 1.0) ** (-zipf)
    p /= p.sum()

    def draw(n):
        s = rs.choice(num_nodes, size=n, p=p)
        o = rs.choice(num_nodes, size=n, p=p)
        r = rs.randint(0, num_rels, size=n)
        return np.stack([s, r, o], axis=1).astype(np.int64)

    return KGDataset(name, num_nodes, num_rels, draw(n_train), draw(n_valid), draw(n_test))


def _read_dict(path):
    out = {}
    with open(path) as f:
        for line in f:
            line = line.rstrip('\n')
            if line:
                idx, name = line.split('\t')
                out[name] = int(idx)
    return out


def _read_triplets(path, ent, rel):
    rows = []
    with open(path) as f:
        for line in f:
            parts = line.rstrip('\n').split('\t')
            if len(parts) == 3:
                rows.append((ent[parts[0]], rel[parts[1]], ent[parts[2]]))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)


def load_data(name):
    if name.startswith('synthetic:'):
        f = [int(x) for x in name.split(':')[1:]]
        f += [0] * (6 - len(f))
        return synthetic_kg(f[0], f[1], f[2], f[3], f[4], seed=f[5], name=name)
    if name in ('FB15k-237-synthetic', 'WN18RR-synthetic'):
        cfg = FB15K237 if name.startswith('FB') else WN18RR
        return synthetic_kg(cfg['num_nodes'], cfg['num_rels'], cfg['n_train'], cfg['n_valid'], cfg['n_test'], name=name)
    root = os.environ.get('GCNVAE_DATA', os.path.join(os.path.expanduser('~'), '.dgl'))
    d = os.path.join(root, name)
    if not os.path.isdir(d):
        raise FileNotFoundError(f'dataset directory {d} not found (expected entities.dict, relations.dict, '
                                f'train/valid/test.txt); use "{name}-synthetic" or "synthetic:..." without files')
    ent = _read_dict(os.path.join(d, 'entities.dict'))
    rel = _read_dict(os.path.join(d, 'relations.dict'))
    return KGDataset(name, len(ent), len(rel), *(_read_triplets(os.path.join(d, s + '.txt'), ent, rel)
                                                 for s in ('train', 'valid', 'test')))


# ------------------------------------------------------------------------------------------------
# entity classification (kgvae/entity_classify.py)
EC_SIZES = {      # entities, relations, triples, classes, labelled (Schlichtkrull et al., Table 1)
    'aifb': (8285, 45, 29043, 4, 176),
    'mutag': (23644, 23, 74227, 2, 340),
    'bgs': (333845, 103, 916199, 2, 146),
    'am': (1666764, 133, 5988321, 11, 1000),
}
EC_PLANTED_EDGES = 3


class EntityDataset:
    def __init__(self, name, num_nodes, num_rels, num_classes, labels, train_idx, test_idx, edge_src, edge_dst, edge_type,
                 edge_norm, old_ids):
        self.name, self.num_nodes, self.num_rels, self.num_classes = name, int(num_nodes), int(num_rels), int(num_classes)
        self.labels, self.train_idx, self.test_idx = labels, train_idx, test_idx
        self.edge_src, self.edge_dst, self.edge_type, self.edge_norm = edge_src, edge_dst, edge_type, edge_norm
        self.old_ids = old_ids


def synthetic_entity_triples(num_nodes, num_rels, n_triples, num_classes, n_labelled, seed=0, zipf=0.8):
    """(triples (T, 3) int64, labels (N,) int64 with -1 where unlabelled, train_idx, test_idx) with planted labels (module docstring)."""
    if num_classes < 1 or num_rels < num_classes:
        raise ValueError(f'need 1 <= classes <= relations, got {num_classes} classes for {num_rels} relations')
    if not 0 < n_labelled <= num_nodes or n_labelled * EC_PLANTED_EDGES > n_triples:
        raise ValueError(f'{n_labelled} labelled nodes do not fit {num_nodes} nodes / {n_triples} triples')
    rs = np.random.RandomState(seed)
    p = (np.arange(num_nodes) + 1.0) ** (-zipf)
    p /= p.sum()
    k = min(2, num_rels // num_classes)
    reserved = num_classes * k
    labelled = rs.choice(num_nodes, size=n_labelled, replace=False)
    y = rs.randint(0, num_classes, size=n_labelled)
    y[:min(num_classes, n_labelled)] = np.arange(min(num_classes, n_labelled))    # every class occurs
    rs.shuffle(y)
    n_plant = n_labelled * EC_PLANTED_EDGES
    n_base = n_triples - n_plant
    lo = reserved if reserved < num_rels else 0
    base = np.stack([rs.choice(num_nodes, size=n_base, p=p), rs.randint(lo, num_rels, size=n_base),
                     rs.choice(num_nodes, size=n_base, p=p)], axis=1)
    obj = np.repeat(labelled, EC_PLANTED_EDGES)
    rel = np.repeat(y, EC_PLANTED_EDGES) * k + rs.randint(0, k, size=n_plant)
    plant = np.stack([rs.choice(num_nodes, size=n_plant, p=p), rel, obj], axis=1)
    triples = np.concatenate([base, plant]).astype(np.int64)
    labels = np.full(num_nodes, -1, dtype=np.int64)
    labels[labelled] = y
    order = rs.permutation(n_labelled)
    n_train = int(round(0.8 * n_labelled))
    return triples, labels, labelled[order[:n_train]].astype(np.int64), labelled[order[n_train:]].astype(np.int64)


def entity_graph(triples, num_nodes, num_rels):
    """Edges with inverses, (dst, src, type)-ordered, and c_{i,r} norms: (src, dst, etype, norm)."""
    s, r, o = triples[:, 0], triples[:, 1], triples[:, 2]
    src = np.concatenate([s, o]).astype(np.int64)
    dst = np.concatenate([o, s]).astype(np.int64)
    et = np.concatenate([r, r + num_rels]).astype(np.int64)
    order = np.lexsort((et, src, dst))
    src, dst, et = src[order], dst[order], et[order]
    key = dst * (2 * num_rels) + et
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    norm = (1.0 / cnt[inv.reshape(-1)]).astype(np.float32)
    return src, dst, et, norm


def prune_edges(src, dst, num_nodes, labelled, n_layers):
    """Mask of the edges whose destination lies within n_layers - 1 reverse hops of a labelled node."""
    reach = np.zeros(num_nodes, dtype=bool)
    reach[labelled] = True
    for _ in range(max(n_layers - 1, 0)):
        nxt = reach.copy()
        nxt[src[reach[dst]]] = True
        if (nxt == reach).all():
            break
        reach = nxt
    return reach[dst]


def _ec_finish(name, num_nodes, num_rels, num_classes, triples, labels, train_idx, test_idx, bfs_level, relabel):
    src, dst, et, norm = entity_graph(triples, num_nodes, num_rels)
    labelled = np.concatenate([train_idx, test_idx])
    if bfs_level is not None:
        keep = prune_edges(src, dst, num_nodes, labelled, int(bfs_level) - 1)
        src, dst, et, norm = src[keep], dst[keep], et[keep], norm[keep]
    old_ids = np.arange(num_nodes, dtype=np.int64)
    if relabel:
        used = np.zeros(num_nodes, dtype=bool)
        used[labelled] = True
        used[src] = True
        used[dst] = True
        old_ids = np.nonzero(used)[0].astype(np.int64)
        new_of = np.full(num_nodes, -1, dtype=np.int64)
        new_of[old_ids] = np.arange(old_ids.size)
        src, dst = new_of[src], new_of[dst]
        labels, train_idx, test_idx = labels[old_ids], new_of[train_idx], new_of[test_idx]
        num_nodes = old_ids.size
    return EntityDataset(name, num_nodes, 2 * num_rels, num_classes, labels, train_idx, test_idx, src, dst, et, norm, old_ids)


def save_entity_dir(path, triples, num_nodes, num_rels, labels, train_idx, test_idx):
    """Write the directory layout ``load_entity_data`` reads (module docstring)."""
    os.makedirs(path, exist_ok=True)
    triples = np.asarray(triples, dtype=np.int64)
    np.savez(os.path.join(path, 'graph.npz'), src=triples[:, 0], etype=triples[:, 1], dst=triples[:, 2],
             num_nodes=np.int64(num_nodes), num_rels=np.int64(num_rels))
    for f, a in (('labels', labels), ('train_idx', train_idx), ('test_idx', test_idx)):
        np.save(os.path.join(path, f + '.npy'), np.asarray(a, dtype=np.int64))


def load_entity_data(name, bfs_level=3, relabel=False):
    """The dataset of kgvae/entity_classify.py:46 (``load_data(args.dataset, bfs_level=args.bfs_level, relabel=args.relabel)``);
    bfs_level None: no pruning."""
    if name.startswith('synthetic-ec:'):
        f = [int(x) for x in name.split(':')[1:]]
        if len(f) not in (5, 6):
            raise ValueError('synthetic-ec:<nodes>:<rels>:<triples>:<classes>:<labelled>[:<seed>]')
        n, r, t, c, lab = f[:5]
        triples, labels, tr, te = synthetic_entity_triples(n, r, t, c, lab, seed=f[5] if len(f) == 6 else 0)
        return _ec_finish(name, n, r, c, triples, labels, tr, te, bfs_level, relabel)
    base = name[:-len('-synthetic')] if name.endswith('-synthetic') else None
    if base in EC_SIZES:
        n, r, t, c, lab = EC_SIZES[base]
        triples, labels, tr, te = synthetic_entity_triples(n, r, t, c, lab, seed=0)
        return _ec_finish(name, n, r, c, triples, labels, tr, te, bfs_level, relabel)
    root = os.environ.get('GCNVAE_DATA', os.path.join(os.path.expanduser('~'), '.dgl'))
    d = os.path.join(root, name)
    if not os.path.isfile(os.path.join(d, 'graph.npz')):
        raise FileNotFoundError(f'entity dataset {d}/graph.npz not found (layout: gcn_vae_amd.data docstring); use '
                                f'"{name}-synthetic" or "synthetic-ec:..." without files')
    z = np.load(os.path.join(d, 'graph.npz'))
    n, r = int(z['num_nodes']), int(z['num_rels'])
    triples = np.stack([z['src'], z['etype'], z['dst']], axis=1).astype(np.int64)
    labels = np.load(os.path.join(d, 'labels.npy')).astype(np.int64)
    tr = np.load(os.path.join(d, 'train_idx.npy')).astype(np.int64)
    te = np.load(os.path.join(d, 'test_idx.npy')).astype(np.int64)
    lab = labels[np.concatenate([tr, te])]
    c = int(lab.max()) + 1 if lab.size else 0
    return _ec_finish(name, n, r, c, triples, labels, tr, te, bfs_level, relabel)
