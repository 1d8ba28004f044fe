"""Entity classification on the host: the dataset loader's rules, pruning against the CPU oracle, the CLI against the reference
parser (a manifest made by tests/golden/make_golden_ec.py), and the head's rule (entity_classify.head_rule) under autograd.   pytest -m "not gpu" """
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import rgcn as orgcn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_published_sizes_and_inverse_edges():
    from gcn_vae_amd.data import EC_SIZES, load_entity_data, synthetic_entity_triples
    d = load_entity_data('aifb-synthetic', bfs_level=None)
    n, r, t, c, lab = EC_SIZES['aifb']
    assert (d.num_nodes, d.num_rels, d.num_classes) == (n, 2 * r, c)
    assert len(d.edge_src) == 2 * t
    assert len(d.train_idx) + len(d.test_idx) == lab and len(d.train_idx) == round(0.8 * lab)
    assert not set(d.train_idx.tolist()) & set(d.test_idx.tolist())
    assert (d.labels[d.train_idx] >= 0).all() and (d.labels[d.test_idx] >= 0).all()
    assert (d.labels >= 0).sum() == lab and set(d.labels[d.labels >= 0].tolist()) == set(range(c))
    # every triple (s, r, o) is the edge s -> o of type r and the edge o -> s of type r + R
    triples, _, _, _ = synthetic_entity_triples(n, r, t, c, lab, seed=0)
    fwd = {(int(s), int(o), int(k)) for s, k, o in triples}
    fwd_m = sorted((s, o, k) for s, k, o in triples.tolist())
    inv_m = sorted((o, s, k + r) for s, k, o in triples.tolist())
    got = sorted(zip(d.edge_src.tolist(), d.edge_dst.tolist(), d.edge_type.tolist()))
    assert got == sorted(fwd_m + inv_m)
    assert len(fwd) > 0
    # (dst, src, type) order
    key = np.stack([d.edge_dst, d.edge_src, d.edge_type], 1)
    assert (np.lexsort(key.T[::-1]) == np.arange(len(key))).all()


def test_edge_norm_is_one_over_typed_in_degree():
    from gcn_vae_amd.data import load_entity_data
    d = load_entity_data('synthetic-ec:300:7:2000:3:50:4', bfs_level=None)
    cnt = {}
    for v, k in zip(d.edge_dst.tolist(), d.edge_type.tolist()):
        cnt[(v, k)] = cnt.get((v, k), 0) + 1
    want = np.array([1.0 / cnt[(v, k)] for v, k in zip(d.edge_dst.tolist(), d.edge_type.tolist())], dtype=np.float32)
    np.testing.assert_array_equal(d.edge_norm, want)
    # pruning keeps the norm computed on the whole graph
    p = load_entity_data('synthetic-ec:300:7:2000:3:50:4', bfs_level=3)
    full = {(s, t, k): w for s, t, k, w in zip(d.edge_src.tolist(), d.edge_dst.tolist(), d.edge_type.tolist(), d.edge_norm.tolist())}
    assert 0 < len(p.edge_src) < len(d.edge_src)
    for s, t, k, w in zip(p.edge_src.tolist(), p.edge_dst.tolist(), p.edge_type.tolist(), p.edge_norm.tolist()):
        assert full[(s, t, k)] == w


def test_directory_layout_round_trip(tmp_path, monkeypatch):
    from gcn_vae_amd.data import load_entity_data, save_entity_dir, synthetic_entity_triples
    triples, labels, tr, te = synthetic_entity_triples(120, 5, 700, 2, 30, seed=3)
    save_entity_dir(str(tmp_path / 'toy'), triples, 120, 5, labels, tr, te)
    monkeypatch.setenv('GCNVAE_DATA', str(tmp_path))
    a = load_entity_data('toy', bfs_level=3, relabel=True)
    b = load_entity_data('synthetic-ec:120:5:700:2:30:3', bfs_level=3, relabel=True)
    for k in ('num_nodes', 'num_rels', 'num_classes'):
        assert getattr(a, k) == getattr(b, k)
    for k in ('labels', 'train_idx', 'test_idx', 'edge_src', 'edge_dst', 'edge_type', 'edge_norm', 'old_ids'):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    with pytest.raises(FileNotFoundError):
        load_entity_data('missing')


def _oracle_model(data, params, n_layers, nb):
    src, dst = torch.from_numpy(data.edge_src), torch.from_numpy(data.edge_dst)
    et, norm = torch.from_numpy(data.edge_type), torch.from_numpy(data.edge_norm).view(-1, 1)
    h = torch.arange(data.num_nodes)
    for i, p in enumerate(params):
        act = torch.relu if i < n_layers - 1 else None
        h = orgcn.rel_graph_conv(h, src, dst, et, norm, p, 'basis', nb, act)
    return h


def _params(num_nodes, num_rels, h, c, n_layers, nb, seed):
    gen = torch.Generator().manual_seed(seed)
    dims = [num_nodes] + [h] * (n_layers - 1) + [c]
    out = []
    for i in range(n_layers):
        p = orgcn.init_params(dims[i], dims[i + 1], num_rels, 'basis', nb, True, True, generator=gen, dtype=torch.float64)
        p['h_bias'] = torch.randn(dims[i + 1], generator=gen, dtype=torch.float64) * 0.1
        out.append(p)
    return out


@pytest.mark.parametrize('n_layers', [2, 3])
def test_pruning_keeps_the_labelled_outputs(n_layers):
    """bfs_level = n_layers + 1: the labelled rows' outputs of an n_layers-deep model are what the whole graph gives, with and
    without relabelling (the input layer's V and loop-weight rows follow the kept nodes)."""
    from gcn_vae_amd.data import load_entity_data
    name, nb = 'synthetic-ec:400:6:2500:3:40:9', 4
    full = load_entity_data(name, bfs_level=None)
    params = _params(full.num_nodes, full.num_rels, 5, full.num_classes, n_layers, nb, seed=2)
    ref = _oracle_model(full, [{k: v.float() for k, v in p.items()} for p in params], n_layers, nb)
    lab = np.concatenate([full.train_idx, full.test_idx])
    for relabel in (False, True):
        pr = load_entity_data(name, bfs_level=n_layers + 1, relabel=relabel)
        assert len(pr.edge_src) < len(full.edge_src)
        ps = [{k: v.float() for k, v in p.items()} for p in params]
        if relabel:
            assert pr.num_nodes < full.num_nodes
            old = torch.from_numpy(pr.old_ids)
            ps[0] = dict(ps[0], weight=ps[0]['weight'][:, old].contiguous(), loop_weight=ps[0]['loop_weight'][old].contiguous())
        out = _oracle_model(pr, ps, n_layers, nb)
        new_lab = np.concatenate([pr.train_idx, pr.test_idx])
        np.testing.assert_array_equal(pr.old_ids[new_lab], lab)
        torch.testing.assert_close(out[torch.from_numpy(new_lab)], ref[torch.from_numpy(lab)], rtol=1e-5, atol=1e-6)
        np.testing.assert_array_equal(pr.labels[new_lab], full.labels[lab])


def test_cli_flags_and_defaults_equal_the_reference_parser():
    from gcn_vae_amd.entity_classify import build_parser
    man = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'entity_classify_cli.json')))
    parser = build_parser()
    ours = {a.dest if a.option_strings else a.dest: a for a in parser._actions}
    by_opts = {tuple(a.option_strings): a for a in parser._actions}
    for o in man['options']:
        a = by_opts.get(tuple(o['option_strings']))
        assert a is not None, o['option_strings']
        assert a.dest == o['dest'] and a.default == o['default'] and a.const == o['const']
        assert (None if a.type is None else a.type.__name__) == o['type'], o['dest']
        assert type(a).__name__ == o['action'] and bool(a.required) == o['required'], o['dest']
    extra = {tuple(a.option_strings) for a in parser._actions if a.option_strings} - \
        {tuple(o['option_strings']) for o in man['options']} - {('-h', '--help')}
    assert extra == {('--materialise-basis',), ('--seed',)}
    got = vars(parser.parse_args(['-d', 'x']))
    assert got.pop('materialise_basis') is False and got.pop('seed') is None
    assert got == man['defaults']
    assert [sorted(a.dest for a in g._group_actions) for g in parser._mutually_exclusive_groups] == man['mutually_exclusive']
    assert vars(parser.parse_args(['-d', 'x', '--testing']))['validation'] is False
    assert 'materialise_basis' in ours


def test_head_rule_equals_cross_entropy_of_softmax_under_autograd():
    """entity_classify.head_rule -- the rule gv_ec_head_* implement, backward written out -- against
    F.cross_entropy(F.softmax(h)) and torch.argmax under autograd, in float64, over three disjoint sets (one empty)."""
    from gcn_vae_amd.entity_classify import head_rule
    gen = torch.Generator().manual_seed(0)
    for c in (2, 4, 11, 64):
        h = torch.randn(30, c, generator=gen, dtype=torch.float64) * 3
        h[:3] = 0.0                                          # ties: argmax to column 0
        y = torch.randint(0, c, (30,), generator=gen)
        perm = torch.randperm(30, generator=gen)
        sets = (perm[:17], perm[17:17], perm[17:25])
        gl = torch.tensor([0.7, 0.4, -0.2], dtype=torch.float64)
        gp = torch.randn(30, c, generator=gen, dtype=torch.float64)
        ht = h.clone().requires_grad_(True)
        pt = F.softmax(ht, dim=1)
        l0 = F.cross_entropy(pt[sets[0]], y[sets[0]])
        l2 = F.cross_entropy(pt[sets[2]], y[sets[2]])
        (gl[0] * l0 + gl[2] * l2 + (pt * gp).sum()).backward()
        p, losses, counts, dh = head_rule(h, y, sets, gl, gp)
        torch.testing.assert_close(p, pt.detach())
        torch.testing.assert_close(losses[0], l0.detach())
        assert torch.isnan(losses[1])
        torch.testing.assert_close(losses[2], l2.detach())
        want = [int((pt[s].argmax(1) == y[s]).sum()) for s in sets]
        assert counts.tolist() == want
        torch.testing.assert_close(dh, ht.grad)
        assert head_rule(h, y, sets)[3] is None
