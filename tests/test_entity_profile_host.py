"""Per-entity completion, host side (no GPU): the rule of ranking.complete_entities_from_scores against a brute-force Python loop on
random and on dyadic (m, R, N) tensors, the argument checks of ranking.complete_entities / ops.entity_topk_scores /
gv_entity_topk_scores before any launch, and the --profile-topk / --profile-entities / --profile-out flags."""
import ctypes
import struct

import pytest
import torch

NAN, INF = float('nan'), float('inf')


def _bits(x):
    return struct.unpack('<I', struct.pack('<f', x))[0]


def _brute(score, entities, k, listed=None, exclude_self=True):
    """The rule, one candidate at a time: ``listed`` maps (entity, relation) to the ids that are no candidates there."""
    m, num_rels, n = score.shape
    rel, other, bits = [], [], []
    for i, a in enumerate(entities):
        cands = []
        for r in range(num_rels):
            hidden = set((listed or {}).get((a, r), ()))
            for x in range(n):
                if (exclude_self and x == a) or x in hidden:
                    continue
                v = float(score[i, r, x])
                nan = v != v
                v = 0.0 if v == 0.0 else v                                  # -0 ties with, and is reported as, +0
                cands.append((1 if nan else 0, 0.0 if nan else -v, r, x, 0x7fc00000 if nan else _bits(v)))
        cands.sort(key=lambda c: c[:4])
        cands = cands[:k] + [(0, 0.0, -1, -1, _bits(-INF))] * max(0, k - len(cands))
        rel.append([c[2] for c in cands])
        other.append([c[3] for c in cands])
        bits.append([c[4] for c in cands])
    return rel, other, bits


def _dense_filter(listed, n, num_rels):
    """(lo, hi, ent) with one range per key a * R + r, as ranking._mine_filter hands them on."""
    lo, hi, ent = [], [], []
    for a in range(n):
        for r in range(num_rels):
            ids = sorted(set(listed.get((a, r), ())))
            lo.append(len(ent))
            ent.extend(ids)
            hi.append(len(ent))
    return torch.tensor(lo), torch.tensor(hi), torch.tensor(ent, dtype=torch.int64)


def _check(score, entities, k, listed=None, exclude_self=True):
    from gcn_vae_amd import ranking
    m, num_rels, n = score.shape
    filt = dict(zip(('filt_lo', 'filt_hi', 'filt_ent'), _dense_filter(listed, n, num_rels))) if listed is not None else {}
    rel, other, logits = ranking.complete_entities_from_scores(score, torch.tensor(entities), k, exclude_self=exclude_self, **filt)
    assert rel.dtype == torch.int64 and other.dtype == torch.int64 and logits.dtype == torch.float32
    assert rel.shape == other.shape == logits.shape == (m, k)
    want_rel, want_other, want_bits = _brute(score, entities, k, listed, exclude_self)
    assert rel.tolist() == want_rel
    assert other.tolist() == want_other
    assert [[b & 0xffffffff for b in row] for row in logits.view(torch.int32).tolist()] == want_bits
    return rel, other, logits


def _random_listed(gen, n, num_rels, share):
    listed = {}
    for a in range(n):
        for r in range(num_rels):
            ids = torch.nonzero(torch.rand(n, generator=gen) < share).flatten().tolist()
            if ids:
                listed[(a, r)] = ids
    return listed


@pytest.mark.parametrize('m, num_rels, n, k', [(5, 3, 17, 7), (9, 1, 33, 40), (4, 6, 8, 128), (1, 2, 70, 1)])
def test_from_scores_equals_the_loop_on_random_tensors(m, num_rels, n, k):
    gen = torch.Generator().manual_seed(m * 1000 + n)
    score = torch.randn(m, num_rels, n, generator=gen)
    entities = torch.randint(0, n, (m,), generator=gen).tolist()            # unsorted, repeats likely
    listed = _random_listed(gen, n, num_rels, 0.2)
    for excl in (True, False):
        _check(score, entities, k, None, excl)
        _check(score, entities, k, listed, excl)


def _dyadic(gen, m, num_rels, n):
    """Multiples of 1/4 from a range of nine values: ties everywhere, inside a relation and across relations."""
    return torch.randint(-4, 5, (m, num_rels, n), generator=gen).float() * 0.25


def test_from_scores_equals_the_loop_on_dyadic_tensors_with_specials():
    gen = torch.Generator().manual_seed(7)
    m, num_rels, n = 6, 4, 19
    score = _dyadic(gen, m, num_rels, n)
    score[0, 1, 3], score[0, 2, 3], score[1, 0, 0] = NAN, NAN, NAN
    score[2, 3, 5], score[2, 0, 6], score[3, 1, 1] = INF, -INF, -INF
    score[score == 0.0] = -0.0                                              # every zero a negative one, next to ...
    score[4, 0, 2], score[4, 1, 2] = 0.0, 0.0                               # ... two positive ones
    entities = [7, 2, 7, 0, 18, 2]                                          # duplicates, not sorted
    listed = _random_listed(gen, n, num_rels, 0.3)
    for k in (1, 5, 60, 128):                                               # 128 > 4 * 18 candidates: padding
        for excl in (True, False):
            _check(score, entities, k, None, excl)
            _check(score, entities, k, listed, excl)


def test_ties_go_by_relation_then_entity_and_specials_come_out_canonical():
    score = torch.tensor([[[1.0, 2.0, 2.0, 0.5], [2.0, 2.0, -0.0, NAN], [3.0, 0.0, -INF, 2.0]]])      # (1, 3, 4), entity 0
    rel, other, logits = _check(score, [0], 12, None, False)
    assert list(zip(rel[0].tolist(), other[0].tolist())) == [(2, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 3), (0, 0), (0, 3), (1, 2),
                                                            (2, 1), (2, 2), (1, 3)]
    got = logits[0].tolist()
    assert [str(x) for x in got[8:10]] == ['0.0', '0.0'] and got[10] == -INF and got[11] != got[11]
    rel, other, logits = _check(score, [0], 12, None, True)                 # without the loops (r, 0): 9 candidates, 3 pads
    assert (rel[0, 9:] == -1).all() and (other[0, 9:] == -1).all() and (logits[0, 9:] == -INF).all()
    assert 0 not in other[0, :9].tolist()


def test_filter_hides_the_best_candidate_of_its_relation_only():
    score = torch.tensor([[[9.0, 1.0, 2.0], [9.0, 3.0, 4.0]], [[5.0, 6.0, 7.0], [8.0, 5.0, 5.0]]])     # entities 1 and 2
    rel, other, _ = _check(score, [1, 2], 2, {(1, 0): [0], (2, 1): [0, 1, 2]}, True)
    assert list(zip(rel[0].tolist(), other[0].tolist())) == [(1, 0), (1, 2)]          # (0, 0) hidden, (1, 0) is not
    assert list(zip(rel[1].tolist(), other[1].tolist())) == [(0, 1), (0, 0)]          # relation 1 lists everybody
    rel, other, _ = _check(score[[1, 0, 1]], [2, 1, 2], 7, {(1, 0): [0], (2, 1): [0, 1, 2]}, False)
    assert (rel[0] == rel[2]).all() and (other[0] == other[2]).all()                  # a repeated entity repeats its row


def test_argument_checks_raise_before_any_device_is_touched():
    from gcn_vae_amd import ops, ranking
    emb, w, ents = torch.zeros(10, 8), torch.zeros(3, 8), torch.tensor([4, 1, 4])
    for route in (ranking.complete_entities, ranking.complete_entities_unfused):
        with pytest.raises(ValueError, match='side'):
            route(emb, w, ents, 5, side='x')
        for k in (0, 129):
            with pytest.raises(ValueError, match='k must lie'):
                route(emb, w, ents, k)
        with pytest.raises(TypeError):
            route(emb, w, ents, 5, type_constraint=None)                     # not accepted yet
    with pytest.raises(ValueError, match='width'):
        ranking.complete_entities(emb, torch.zeros(3, 7), ents, 5)
    with pytest.raises(ValueError, match='31 bits'):                          # 2^16 entities x 2^15 relations, width 1
        ranking.complete_entities(torch.zeros(1 << 16, 1), torch.zeros(1 << 15, 1), ents, 5)
    with pytest.raises(ValueError, match='31 bits'):
        ops.entity_topk_scores(ents, torch.zeros(1 << 16, 1), torch.zeros(1 << 15, 1), 5)
    assert ops._entity_topk_operands(ents, torch.zeros((1 << 16) - 1, 1), torch.zeros(1 << 15, 1)) == (3, 65535, 32768, 1)
    with pytest.raises(ValueError, match=r'\[0, 10\)'):
        ops.entity_topk_scores(torch.tensor([4, 10]), emb, w, 5)
    with pytest.raises(ValueError, match=r'\[0, 10\)'):
        ops.entity_topk_scores(torch.tensor([-1, 4]), emb, w, 5)
    with pytest.raises(TypeError, match='ents'):
        ops.entity_topk_scores(torch.tensor([1.0]), emb, w, 5)
    with pytest.raises(ValueError, match='span'):
        ops.entity_topk_scores(ents, emb, w, 5, span=0)
    lo, hi, ent = torch.zeros(30, dtype=torch.long), torch.ones(30, dtype=torch.long), torch.tensor([3])
    with pytest.raises(ValueError, match='together'):
        ops.entity_topk_scores(ents, emb, w, 5, None, lo, hi, None)
    with pytest.raises(ValueError, match='one filter range'):                 # one range per key a * R + r: 30 of them
        ops.entity_topk_scores(ents, emb, w, 5, None, lo[:10], hi[:10], ent)
    with pytest.raises(ValueError, match='filt_lo <= filt_hi'):
        ops.entity_topk_scores(ents, emb, w, 5, None, hi, lo, ent)
    with pytest.raises(ValueError, match=r'\[0, 10\)'):
        ops.entity_topk_scores(ents, emb, w, 5, None, lo, hi, ent + 7)
    with pytest.raises(RuntimeError, match='no CPU fallback'):                # valid arguments: the device check, still no launch
        ops.entity_topk_scores(ents, emb, w, 5, None, lo, hi, ent)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ranking.complete_entities(emb, w, ents, 5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ranking.complete_entities(emb, w, ents, 5, side='o', filter_index=ranking.FilterIndex(10, 3, [[1, 2, 3], [4, 0, 4]]))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ranking.complete_entities_unfused(emb, w, ents, 5)


def test_c_entry_validates_arguments_before_any_launch():
    from gcn_vae_amd import lib
    l = lib.load()
    fn = l.gv_entity_topk_scores
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)

    def call(ents=p, m=4, e=p, ld_e=8, w=p, ld_w=8, lo=None, hi=None, ent=None, n_ent=0, k=5, span=0, rel=p, other=p, logits=p,
             ws=p, ws_bytes=1 << 20, n=10, num_rels=3, h=8):
        return fn(ents, m, e, ld_e, w, ld_w, None, lo, hi, ent, n_ent, 1, k, span, rel, other, logits, ws, ws_bytes, n, num_rels, h, None)

    assert call(ents=None, m=0, e=None, w=None, rel=None, other=None, logits=None, ws=None, ws_bytes=0) == 0          # m == 0
    assert call(k=0) != 0 and 'k=0' in lib.last_error()
    assert call(k=129) != 0 and 'k=129' in lib.last_error()
    assert call(m=-1) != 0 and 'm=-1' in lib.last_error()
    assert call(n=0) != 0 and 'n=0' in lib.last_error()
    assert call(num_rels=0) != 0 and 'num_rels=0' in lib.last_error()
    assert call(h=0) != 0 and 'h=0' in lib.last_error()
    assert call(n_ent=-1, lo=p, hi=p, ent=p) != 0 and 'n_filt_ent=-1' in lib.last_error()
    assert call(n=1 << 16, num_rels=1 << 15) != 0 and '31 bits' in lib.last_error()
    assert call(span=-1) != 0 and 'span_tiles=-1' in lib.last_error()
    assert call(ld_e=7) != 0 and 'leading dimension' in lib.last_error()
    assert call(ld_w=7) != 0 and 'leading dimension' in lib.last_error()
    assert call(lo=p, ent=p, n_ent=1) != 0 and 'NULL' in lib.last_error()
    assert call(ent=p, n_ent=1) != 0 and 'NULL' in lib.last_error()
    for missing in ('ents', 'e', 'w', 'rel', 'other', 'logits', 'ws'):
        assert call(**{missing: None}) != 0 and 'NULL' in lib.last_error(), missing
    assert call(ws_bytes=4 * 5 * 8 - 1) != 0 and 'workspace' in lib.last_error()       # one span of three tiles: m * k keys
    assert call(span=1, ws_bytes=3 * 4 * 5 * 8 - 1) != 0 and 'workspace' in lib.last_error()
    ws = l.gv_entity_topk_scores_workspace_bytes
    assert ws(0, 10, 3, 5) == 0 and ws(4, 10, 3, 0) == 0 and ws(4, 10, 3, 129) == 0 and ws(4, 1 << 16, 1 << 15, 5) == 0
    assert ws(4, 10, 3, 5) == 4 * 5 * 8
    big = ws(14541, 14541, 237, 100)
    assert big >= 14541 * 100 * 8 and big % (14541 * 100 * 8) == 0
    one = ws(1, 14541, 237, 100)                                            # a single entity is spread over many spans
    assert one >= 64 * 100 * 8 and one % (100 * 8) == 0


def test_parser_has_the_profile_flags_and_keeps_every_other_default(tmp_path):
    from gcn_vae_amd import train
    p = train.build_parser()
    base = p.parse_args(['-d', 'FB15k-237-synthetic'])
    assert base.profile_topk == 0 and base.profile_entities is None and base.profile_out == 'profiles.tsv'
    assert base.generate is False and base.predict_topk == 0 and base.complete_topk == 0
    on = p.parse_args(['-d', 'x', '--test-mode', 'True', '--profile-topk', '10', '--profile-entities', '3,1,3', '--profile-out', 'p.tsv'])
    assert on.profile_topk == 10 and on.profile_entities == '3,1,3' and on.profile_out == 'p.tsv' and on.test_mode is True
    train.check_args(on)
    with pytest.raises(ValueError, match='--profile-topk'):                  # decodes a trained checkpoint
        train.check_args(p.parse_args(['-d', 'x', '--profile-topk', '10']))
    with pytest.raises(ValueError, match='--profile-topk'):
        train.check_args(p.parse_args(['-d', 'x', '--test-mode', 'True', '--profile-topk', '129']))
    assert train.profile_entities_arg(None, 4) == [0, 1, 2, 3]
    assert train.profile_entities_arg('3, 1,3', 4) == [3, 1, 3]
    listing = tmp_path / 'ids.txt'
    listing.write_text('2\n\n0\n2\n')
    assert train.profile_entities_arg(str(listing), 4) == [2, 0, 2]
    with pytest.raises(ValueError, match='outside'):
        train.profile_entities_arg('1,4', 4)
    with pytest.raises(ValueError, match='--profile-entities'):
        train.profile_entities_arg('1,x', 4)
