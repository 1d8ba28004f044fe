"""Per-entity completion for the TransE baseline, host side (no GPU): the rule of transe.complete_entities_from_distances against a
brute-force Python sort, the refusals of gv_transe_entity_topk before any launch, its workspace size, and the --profile-topk /
--profile-entities / --profile-out flags of ``python -m gcn_vae_amd.transe``."""
import ctypes
import os
import re
import struct

import pytest
import torch

NAN, INF = float('nan'), float('inf')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'gv_transe_entity_topk'


def _bits(x):
    return struct.unpack('<I', struct.pack('<f', x))[0]


def _brute(dist, entities, k, listed, exclude_self):
    """The rule, one candidate at a time: distance ascending, then relation, then entity; NaN after every number (+inf included)."""
    m, num_rels, n = dist.shape
    rows = []
    for i, a in enumerate(entities):
        cands = []
        for r in range(num_rels):
            hidden = set((listed or {}).get((a, r), ()))
            for x in range(n):
                if (exclude_self and x == a) or x in hidden:
                    continue
                v = float(dist[i, r, x])
                nan = v != v
                v = 0.0 if v == 0.0 else v                                  # -0 ties with, and is reported as, +0
                cands.append((1 if nan else 0, 0.0 if nan else v, r, x, 0x7fc00000 if nan else _bits(v)))
        cands.sort(key=lambda c: c[:4])
        rows.append(cands[:k] + [(0, 0.0, -1, -1, _bits(INF))] * max(0, k - len(cands)))
    return ([[c[2] for c in row] for row in rows], [[c[3] for c in row] for row in rows], [[c[4] for c in row] for row in rows])


def _dense_filter(listed, n, num_rels):
    """(lo, hi, ent) with one range per key a * R + r, as ranking._mine_filter hands them on."""
    lo, hi, ent = [], [], []
    for a in range(n):
        for r in range(num_rels):
            lo.append(len(ent))
            ent.extend(sorted(set(listed.get((a, r), ()))))
            hi.append(len(ent))
    return torch.tensor(lo), torch.tensor(hi), torch.tensor(ent, dtype=torch.int64)


def _check(dist, entities, k, listed, exclude_self):
    from gcn_vae_amd import transe
    m, num_rels, n = dist.shape
    filt = dict(zip(('filt_lo', 'filt_hi', 'filt_ent'), _dense_filter(listed, n, num_rels))) if listed else {}
    rel, other, out = transe.complete_entities_from_distances(dist, torch.tensor(entities), k, exclude_self=exclude_self, **filt)
    assert rel.dtype == torch.int64 and other.dtype == torch.int64 and out.dtype == torch.float32
    assert rel.shape == other.shape == out.shape == (m, k)
    want_rel, want_other, want_bits = _brute(dist, entities, k, listed, exclude_self)
    assert rel.tolist() == want_rel
    assert other.tolist() == want_other
    assert [[b & 0xffffffff for b in row] for row in out.view(torch.int32).tolist()] == want_bits
    return rel, other, out


def test_from_distances_equals_a_python_sort_on_a_hand_made_tensor():
    # (3, 2, 5), rows for entities 1, 4, 1.  Equal distances inside a relation (0.5 twice in [0, 0]) and across relations (2.0 in
    # [0, 0] and [0, 1]); a NaN, a +inf, a -0; (1, 0) lists entity 3, the best of its relation; the loops are (r, 1) and (r, 4).
    dist = torch.tensor([[[0.5, 0.1, 0.5, 0.05, 2.0], [2.0, 0.0, NAN, 0.75, INF]],
                         [[3.0, 1.0, -0.0, 1.0, 0.0], [1.0, 4.0, 0.25, NAN, 0.5]],
                         [[0.5, 0.1, 0.5, 0.05, 2.0], [2.0, 0.0, NAN, 0.75, INF]]])
    listed = {(1, 0): [3], (4, 1): [0, 1]}
    rel, other, out = _check(dist, [1, 4, 1], 12, listed, True)
    # entity 1: 8 candidates less the listed (0, 3) = 7, then padding; the tie 0.5 goes by entity, the tie 2.0 by relation
    assert list(zip(rel[0].tolist(), other[0].tolist()))[:7] == [(0, 0), (0, 2), (1, 3), (0, 4), (1, 0), (1, 4), (1, 2)]
    assert out[0, 5].item() == INF and out[0, 6].item() != out[0, 6].item()           # +inf is a candidate, ahead of the NaN
    assert (rel[0, 7:] == -1).all() and (other[0, 7:] == -1).all() and (out[0, 7:] == INF).all()
    assert (rel[0] == rel[2]).all() and (other[0] == other[2]).all()                  # a repeated entity repeats its row
    # entity 4: -0 comes out as +0 and first, its loop's 0.0 is no candidate, relation 1 has lost entities 0 and 1
    assert (rel[1, 0].item(), other[1, 0].item()) == (0, 2) and _bits(out[1, 0].item()) == 0
    assert list(zip(rel[1].tolist(), other[1].tolist()))[1:5] == [(1, 2), (0, 1), (0, 3), (0, 0)]
    assert (1, 0) not in list(zip(rel[1].tolist(), other[1].tolist()))
    for k in (1, 3, 8):
        for excl in (True, False):
            _check(dist, [1, 4, 1], k, listed, excl)
            _check(dist, [1, 4, 1], k, None, excl)
    # with the loops kept, the zero of (0, 1, 1) -- reported as +0 -- leads entity 1's list
    rel, other, out = _check(dist, [1, 4, 1], 10, None, False)
    assert (rel[0, 0].item(), other[0, 0].item()) == (1, 1) and _bits(out[0, 0].item()) == 0
    assert (rel[0, 9].item(), other[0, 9].item()) == (1, 2) and _bits(out[0, 9].item()) == 0x7fc00000


def test_symbols_are_declared_and_bound():
    from gcn_vae_amd import lib
    header = open(os.path.join(ROOT, 'include', 'gcnvae.h')).read()
    for name, n_args in ((ENTRY, 22), (ENTRY + '_workspace_bytes', 5)):
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == n_args
        assert re.search(r'\b%s\s*\(' % name, header)
    assert lib.SIGNATURES[ENTRY + '_workspace_bytes'][0] is lib._L and lib.SIGNATURES[ENTRY][1][20] is lib._L


def test_c_entry_refuses_bad_arguments_before_any_launch():
    from gcn_vae_amd import lib
    l = lib.load()
    fn = getattr(l, ENTRY)
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)

    def call(ents=p, m=4, en=p, rn=p, n=10, num_rels=3, dim=8, head=0, p_norm=1, lo=None, hi=None, ent=None, n_ent=0, k=5, span=0,
             rel=p, other=p, dist=p, ws=p, ws_bytes=1 << 20):
        return fn(ents, m, en, rn, n, num_rels, dim, head, p_norm, lo, hi, ent, n_ent, 1, k, span, rel, other, dist, ws, ws_bytes, None)

    def refused(code, text, **kw):
        rc = call(**kw)
        err = lib.last_error()
        assert rc == code, (kw, rc, err)
        assert err.startswith(ENTRY + ':') and text in err, (kw, err)

    SHAPE, NULL = -2, -1
    assert call(m=0, k=0) == SHAPE                                          # sizes are looked at even without queries
    refused(SHAPE, 'k=0', k=0)
    refused(SHAPE, 'k=129', k=129)
    refused(SHAPE, 'dim=0', dim=0)
    refused(SHAPE, 'dim=513', dim=513)
    assert call(dim=512, ws_bytes=0) == SHAPE and 'workspace' in lib.last_error()      # 512 itself passes the size check
    refused(SHAPE, 'p_norm=3', p_norm=3)
    refused(SHAPE, 'p_norm=0', p_norm=0)
    refused(SHAPE, 'num_rels=0', num_rels=0)
    refused(SHAPE, 'n=0', n=0)
    refused(SHAPE, 'm=-1', m=-1)
    refused(SHAPE, 'n_filt_ent=-1', n_ent=-1, lo=p, hi=p, ent=p)
    refused(SHAPE, '31 bits', n=1 << 16, num_rels=1 << 15)
    refused(SHAPE, 'span_tiles=-1', span=-1)
    for given in (dict(lo=p), dict(hi=p), dict(ent=p), dict(lo=p, hi=p), dict(lo=p, ent=p), dict(hi=p, ent=p)):
        refused(NULL, 'all given or all NULL', n_ent=1, **given)
    refused(SHAPE, 'workspace of 159 bytes, 160 needed', ws_bytes=4 * 5 * 8 - 1)       # one span of three tiles: m * k keys
    refused(SHAPE, 'workspace of 479 bytes, 480 needed', span=1, ws_bytes=3 * 4 * 5 * 8 - 1)
    for missing in ('ents', 'en', 'rn', 'rel', 'other', 'dist', 'ws'):
        refused(NULL, 'NULL pointer', **{missing: None})
    # m == 0 returns before the pointers are looked at
    assert call(ents=None, m=0, en=None, rn=None, rel=None, other=None, dist=None, ws=None, ws_bytes=0) == 0


def test_workspace_bytes():
    from gcn_vae_amd import lib
    ws = getattr(lib.load(), ENTRY + '_workspace_bytes')
    for bad in ((0, 10, 3, 5, 0), (-1, 10, 3, 5, 0), (4, 0, 3, 5, 0), (4, 10, 0, 5, 0), (4, 10, 3, 0, 0), (4, 10, 3, 129, 0),
                (4, 10, 3, 5, -1), (4, 1 << 16, 1 << 15, 5, 0)):
        assert ws(*bad) == 0, bad
    # a given span_tiles: m * ceil(R * ceil(N / 64) / span_tiles) * k * 8, span_tiles capped at the number of tiles
    for m, n, num_rels, k, span in ((4, 10, 3, 5, 1), (4, 10, 3, 5, 2), (4, 10, 3, 5, 100), (65, 130, 5, 128, 4), (1, 14541, 237, 10, 7),
                                    (3, 64, 2, 1, 1), (3, 65, 2, 1, 1)):
        tiles = num_rels * ((n + 63) // 64)
        per = min(span, tiles)
        assert ws(m, n, num_rels, k, span) == m * ((tiles + per - 1) // per) * k * 8, (m, n, num_rels, k, span)
    # the library's rule (k_topk.h, topk_spans_of with at most 256 spans): about 1024 workgroups, spans of at least 8 tiles
    def rule(m, n, num_rels):
        tiles, row_tiles = num_rels * ((n + 63) // 64), (m + 63) // 64
        s = max(1, min((1024 + row_tiles - 1) // row_tiles, max(1, tiles // 8), 256))
        per = (tiles + s - 1) // s
        return (tiles + per - 1) // per

    assert ws(4, 10, 3, 5, 0) == 4 * 5 * 8
    for m, n, num_rels, k in ((1, 14541, 237, 100), (14541, 14541, 237, 100), (40943, 40943, 11, 128), (65, 130, 5, 10), (1, 600, 2, 3)):
        assert ws(m, n, num_rels, k, 0) == m * rule(m, n, num_rels) * k * 8, (m, n, num_rels, k)
    assert rule(1, 14541, 237) > 200                                         # a single entity is spread over the chip


def _cli(*extra):
    from gcn_vae_amd import transe
    return transe.build_parser().parse_args(['-d', 'x', *extra])


def test_cli_flags_and_refusals(tmp_path):
    from gcn_vae_amd import train, transe
    base = _cli()
    assert base.profile_topk == 0 and base.profile_entities is None and base.profile_out == 'transe_profiles.tsv'
    transe.check_args(base)
    on = _cli('--profile-topk', '128', '--profile-entities', '3,1,3', '--profile-out', 'p.tsv', '--test-mode')
    assert on.profile_topk == 128 and on.profile_entities == '3,1,3' and on.profile_out == 'p.tsv'
    transe.check_args(on)
    for bad in ('129', '-1'):
        with pytest.raises(ValueError, match='--profile-topk'):
            transe.check_args(_cli('--profile-topk', bad))
    # one parser of --profile-entities for both CLIs: an id equal to N is outside [0, N)
    assert transe.profile_entities_arg is train.profile_entities_arg
    assert transe.profile_entities_arg('3,59,3,0', 60) == [3, 59, 3, 0]
    with pytest.raises(ValueError, match=r'entity 60 lies outside \[0, 60\)'):
        transe.profile_entities_arg('3,60', 60)
    listing = tmp_path / 'ids.txt'
    listing.write_text('2\n\n4\n')
    with pytest.raises(ValueError, match='outside'):
        transe.profile_entities_arg(str(listing), 4)


def test_side_and_k_are_checked_before_any_device_is_touched():
    from gcn_vae_amd import transe
    tables = (torch.zeros(10, 8), torch.zeros(3, 8), 1, True)
    ents = torch.tensor([4, 1, 4])
    for route in (transe.complete_entities, transe.complete_entities_unfused):
        with pytest.raises(ValueError, match='side'):
            route(tables, ents, 5, side='x')
        for k in (0, 129):
            with pytest.raises(ValueError, match='k must lie'):
                route(tables, ents, k)
        with pytest.raises(RuntimeError, match='no CPU fallback'):           # valid arguments: the device check, no launch
            route(tables, ents, 5, side='o')
    with pytest.raises(ValueError, match='31 bits'):
        transe.complete_entities((torch.zeros(1 << 16, 1), torch.zeros(1 << 15, 1), 1, True), ents, 5)
