"""Per-relation completion on the GPU (gv_mine_scores_by_relation / gv_mine_scores_typed_by_relation, ops.relation_topk_scores[_typed],
ranking.complete_relations) against the rule stated on logits materialised on the device by the expression that defines them
(ops.mul + ops.gemm per relation), selected by ranking.complete_relations_from_scores.  Every comparison is exact: ids equal, logits
equal as bit patterns, per-relation counts equal.  pytest -m gpu."""
import numpy as np
import pytest
import torch

from mine_cases import _lists
from mine_typed_cases import member_lists, member_masks
from relation_profile_cases import same_rows

pytestmark = pytest.mark.gpu

SHAPES = [(50, 3, 8),          # one partial tile
          (130, 7, 200),       # 3 x 3 tile pairs, a last tile of 2 rows, resident tiles
          (130, 3, 244),       # chunked staging, the last chunk 4 wide
          (70, 2, 500),        # chunked staging, three chunks
          (700, 20, 16),       # 121 tile pairs: rel_span 3, a workgroup flushes several relations' histograms
          (64, 1, 64)]


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


def _materialise(ops, emb, w, bias=None):
    """score[r, s, o], by the expression that defines the logit."""
    emb = emb.contiguous()
    out = torch.stack([ops.gemm(ops.mul(emb, w[r].expand_as(emb).contiguous()), emb, trans_b=True, precision='f32')
                       for r in range(w.shape[0])])
    return out if bias is None else out + bias


def _tables(n, num_rels, h, seed, scaled=True):
    """Entity and relation tables; ``scaled``: w rows scaled by 2^-10 .. 2^10, so that every relation's K-th logit sits in its own
    first-level histogram bin -- the case ONE threshold for the whole graph gets wrong."""
    gen = torch.Generator().manual_seed(seed)
    emb, w = torch.randn(n, h, generator=gen) * 0.5, torch.randn(num_rels, h, generator=gen)
    if scaled:
        w *= (2.0 ** torch.linspace(-10, 10, num_rels)).view(-1, 1) if num_rels > 1 else 1.0
    return emb.cuda(), w.cuda(), gen


def _ks(n, m):
    """(k, max_results): 1, 10, 1 000 and more than any relation's candidates."""
    return [(1, 1 << 22), (10, 1 << 22), (1000, 1 << 22), (n * n + 5, m * (n * n + 5))]


@pytest.mark.parametrize('n,num_rels,h', SHAPES)
def test_every_relations_list_equals_the_definition(ops, n, num_rels, h):
    from gcn_vae_amd import ranking
    emb, w, gen = _tables(n, num_rels, h, 3 * n + num_rels + h)
    bias = torch.tensor(0.375, device='cuda') if h == 200 else None
    score = _materialise(ops, emb, w, bias)
    lo, hi, ent = _lists(n * num_rels, n, gen, dense=n <= 70)
    for filt, exclude_self in (({}, True), (dict(filt_lo=lo, filt_hi=hi, filt_ent=ent), True), (dict(filt_lo=lo, filt_hi=hi, filt_ent=ent), False)):
        for k, cap in _ks(n, num_rels):
            kw = dict(exclude_self=exclude_self, max_results=cap, **filt)
            got = ops.relation_topk_scores(emb, w, k, bias=bias, **kw)
            assert got[0].dtype == got[1].dtype == torch.int64 and got[2].dtype == torch.float32
            assert got[0].shape == got[1].shape == got[2].shape == (num_rels, k) and got[3]['count'].shape == (num_rels,)
            assert same_rows(got, ranking.complete_relations_from_scores(score, k, **kw)), (k, exclude_self, bool(filt))
            assert 2 <= got[3]['passes'] <= len(ops.MINE_RELATION_LEVELS) + 1
    if num_rels > 1:                                 # the global miner's one threshold: the top-500 of the graph leave relations out
        trip = ops.mine_scores(emb, w, k=500, bias=bias)[0]
        assert len(set(trip[:, 1].tolist())) < num_rels


def test_negative_nan_and_tied_relations(ops):
    """A relation with only negative logits, one whose w row is NaN (an empty list), duplicated rows of E (exact ties at the K-th
    value inside and across tile pairs), -0 and +0."""
    from gcn_vae_amd import ranking
    n, num_rels, h = 130, 7, 200
    emb, w, gen = _tables(n, num_rels, h, 17)
    emb = emb.abs()
    for j in (7, 63, 64, 70, 128, 129):
        emb[j] = emb[3]
    emb[20] = 0.0
    emb[21] = -0.0
    w[3] = -w[3].abs()                               # every logit of relation 3 is negative (or -0)
    w[4] = float('nan')
    w[1] = 1.0                                       # symmetric: (s, o) ties with (o, s)
    score = _materialise(ops, emb, w)
    assert float(score[3][~torch.isnan(score[3])].max()) <= 0.0
    for k in (1, 4, 10, 1000, n * n):
        got = ops.relation_topk_scores(emb, w, k, max_results=num_rels * n * n)
        assert same_rows(got, ranking.complete_relations_from_scores(score, k, max_results=num_rels * n * n)), k
        assert got[0][4].tolist() == [-1] * k and bool(torch.isinf(got[2][4]).all()) and int(got[3]['count'][4]) == 0
        assert not bool(torch.isnan(got[2]).any())
    zero = got[2] == 0
    assert int(zero.sum()) > 0 and not bool(torch.signbit(got[2][zero]).any())          # -0 is reported as +0


def test_a_subset_in_any_order_equals_the_rows_of_the_whole(ops):
    from gcn_vae_amd import ranking
    n, num_rels, h = 130, 7, 200
    emb, w, gen = _tables(n, num_rels, h, 23)
    lo, hi, ent = _lists(n * num_rels, n, gen, dense=False)
    kw = dict(filt_lo=lo, filt_hi=hi, filt_ent=ent)
    whole = ops.relation_topk_scores(emb, w, 50, **kw)
    for rels in ([5, 0, 2], torch.tensor([6]), torch.tensor([2, 5, 0], device='cuda', dtype=torch.int32)):
        part = ops.relation_topk_scores(emb, w, 50, relations=rels, **kw)
        rows = torch.as_tensor(rels).cpu().long()
        assert part[0].shape == (len(rows), 50) and same_rows(part, whole, None, rows)
    score = _materialise(ops, emb, w)
    assert same_rows(ops.relation_topk_scores(emb, w, 50, relations=[5, 0, 2], **kw),
                     ranking.complete_relations_from_scores(score, 50, relations=[5, 0, 2], **kw))


def test_the_routes_agree_with_each_other(ops):
    """complete_relations = complete_relations_unfused = per relation mine_scores(E, w[r:r+1], k=K) with that relation's filter."""
    from gcn_vae_amd import ranking
    n, num_rels, h, k = 130, 7, 200, 40
    emb, w, gen = _tables(n, num_rels, h, 29)
    trip = torch.stack([torch.randint(0, n, (900,), generator=gen), torch.randint(0, num_rels, (900,), generator=gen),
                        torch.randint(0, n, (900,), generator=gen)], 1)
    fi = ranking.FilterIndex(n, num_rels, trip.numpy(), device='cuda')
    got = ranking.complete_relations(emb, w, k, filter_index=fi, flow_log_prob=torch.tensor(-0.5))
    assert same_rows(got, ranking.complete_relations_unfused(emb, w, k, filter_index=fi, flow_log_prob=torch.tensor(-0.5)))
    lo, hi, ent = ranking._mine_filter(fi, n, num_rels, emb.device)
    bias = torch.tensor(-0.5, device='cuda')
    for r in range(num_rels):
        t, logits, info = ops.mine_scores(emb, w[r:r + 1], k=k, bias=bias, filt_lo=lo[r::num_rels], filt_hi=hi[r::num_rels], filt_ent=ent)
        assert torch.equal(t[:, 0], got[0][r]) and torch.equal(t[:, 2], got[1][r]) and bool((t[:, 1] == 0).all())
        assert torch.equal(logits.view(torch.int32), got[2][r].view(torch.int32)) and info['count'] == int(got[3]['count'][r])
    known = {tuple(x) for x in trip.tolist()}
    assert not any((int(s), r, int(o)) in known for r in range(num_rels) for s, o in zip(got[0][r].tolist(), got[1][r].tolist()))


def test_a_tie_above_the_share_is_an_overflow_naming_the_relation(ops):
    ones, w1 = torch.ones(100, 8, device='cuda'), torch.ones(2, 8, device='cuda')
    with pytest.raises(ops.MineOverflow) as err:
        ops.relation_topk_scores(ones, w1, 300, max_results=2 * 9899)
    assert err.value.count == 9900 and 'relation 0' in str(err.value) and '9900' in str(err.value)
    subj, obj, logits, info = ops.relation_topk_scores(ones, w1, 300, max_results=2 * 9900)
    want = [(s, o) for s in range(100) for o in range(100) if s != o][:300]
    for r in range(2):
        assert list(zip(subj[r].tolist(), obj[r].tolist())) == want and bool((logits[r] == 8).all())
    assert info['count'].tolist() == [9900, 9900]
    with pytest.raises(ops.MineOverflow) as err:                 # only the tied relation is named
        w2 = torch.ones(2, 8, device='cuda')
        w2[0, 0] = float('nan')
        ops.relation_topk_scores(ones, w2, 300, max_results=2 * 9899)
    assert 'relation 1' in str(err.value)


# ---- among type-correct pairs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,num_rels,h', [(50, 3, 8), (130, 7, 200), (70, 6, 500), (300, 12, 16)])
def test_typed_lists_equal_the_definition_on_masked_scores(ops, n, num_rels, h):
    """mine_typed_cases' member lists: both sets full, 63 / 65, 64 / 1, an EMPTY subject set, 65 / 63, 1 / full."""
    from gcn_vae_amd import ranking
    emb, w, gen = _tables(n, num_rels, h, 5 * n + num_rels + h)
    cs, co = member_masks(n, num_rels, gen)
    set_ptr, set_ids = member_lists(cs, co)
    score = _materialise(ops, emb, w)
    lo, hi, ent = _lists(n * num_rels, n, gen, dense=n <= 70)
    masks = dict(cand_subj=cs.cuda(), cand_obj=co.cuda())
    for filt, exclude_self in (({}, True), (dict(filt_lo=lo, filt_hi=hi, filt_ent=ent), False)):
        for k, cap in _ks(n, num_rels):
            kw = dict(exclude_self=exclude_self, max_results=cap, **filt)
            got = ops.relation_topk_scores_typed(emb, w, k, set_ptr, set_ids, **kw)
            assert same_rows(got, ranking.complete_relations_from_scores(score, k, **masks, **kw)), (k, exclude_self, bool(filt))
            assert got[3]['passes'] <= len(ops.MINE_RELATION_TYPED_LEVELS) + 1
            if num_rels > 3:                         # relation 3 has no subject
                assert got[0][3].tolist() == [-1] * k and int(got[3]['count'][3]) == 0
    # a surviving fact's logit is the untyped call's, bit for bit
    k = n * n
    typed = ops.relation_topk_scores_typed(emb, w, k, set_ptr, set_ids, max_results=num_rels * k)
    plain = ops.relation_topk_scores(emb, w, k, max_results=num_rels * k)
    for r in range(num_rels):
        bits = torch.full((n, n), -1, dtype=torch.int64, device='cuda')
        live = plain[0][r] >= 0
        bits[plain[0][r][live], plain[1][r][live]] = plain[2][r][live].view(torch.int32).long()
        live = typed[0][r] >= 0
        assert torch.equal(bits[typed[0][r][live], typed[1][r][live]], typed[2][r][live].view(torch.int32).long())
    # a subset, and the spans: the result does not depend on them
    part = ops.relation_topk_scores_typed(emb, w, 10, set_ptr, set_ids, relations=[2, 0])
    whole = ops.relation_topk_scores_typed(emb, w, 10, set_ptr, set_ids)
    assert same_rows(part, whole, None, torch.tensor([2, 0]))
    for span in (1, 1000):
        assert same_rows(ops.relation_topk_scores_typed(emb, w, 10, set_ptr, set_ids, span=span), whole)


def test_typed_through_a_type_constraint_and_its_cross_check(ops):
    from gcn_vae_amd import ranking
    n, num_rels, h, k = 130, 7, 200, 25
    emb, w, gen = _tables(n, num_rels, h, 31)
    trip = torch.stack([torch.randint(0, n, (600,), generator=gen), torch.randint(0, num_rels - 1, (600,), generator=gen),
                        torch.randint(0, n, (600,), generator=gen)], 1).numpy()      # relation 6 is never seen: empty sets
    fi, tc = ranking.FilterIndex(n, num_rels, trip, device='cuda'), ranking.TypeConstraint(n, num_rels, trip, device='cuda')
    got = ranking.complete_relations(emb, w, k, relations=[6, 1, 4], filter_index=fi, type_constraint=tc)
    assert same_rows(got, ranking.complete_relations_unfused(emb, w, k, relations=[6, 1, 4], filter_index=fi, type_constraint=tc))
    assert got[0][0].tolist() == [-1] * k
    mined = ranking.mine_triplets(emb, w, threshold=float('-inf'), filter_index=fi, type_constraint=tc, max_results=2 ** 31 - 1)
    for i, r in enumerate([6, 1, 4]):                # mine_triplets(type_constraint=)'s rule, on the same member lists
        of_r = mined[0][:, 1] == r
        assert torch.equal(mined[0][of_r][:k, 0], got[0][i][got[0][i] >= 0]) and torch.equal(mined[0][of_r][:k, 2], got[1][i][got[1][i] >= 0])
        assert torch.equal(mined[1][of_r][:k].view(torch.int32), got[2][i][got[0][i] >= 0].view(torch.int32))


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_relation_profiles(tmp_path):
    from gcn_vae_amd import train
    from gcn_vae_amd.encoders import KGVAE
    spec = 'synthetic:60:4:400:40:40'
    kg = __import__('gcn_vae_amd.data', fromlist=['load_data']).load_data(spec)
    torch.manual_seed(0)
    net = train.LinkPredict(KGVAE, kg.num_nodes, 16, kg.num_rels, num_bases=4, num_hidden_layers=1, dropout=0.0,
                            use_cuda=True, reg_param=0.01, kl_param=1e-3, mmd_param=0.0, k=4, n_flows=2).cuda()
    ckpt = str(tmp_path / 'm.pth')
    torch.save({'state_dict': train.host_state_dict(net), 'epoch': 0}, ckpt)
    known = {tuple(x) for x in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    seen_s = {r: {t[0] for t in known if t[1] == r} for r in range(kg.num_rels)}
    seen_o = {r: {t[2] for t in known if t[1] == r} for r in range(kg.num_rels)}
    which, k = [kg.num_rels - 1, 0, 2], 7
    base = ['-d', spec, '--gpu', '0', '--n-hidden', '16', '--n-bases', '4', '--n-layers', '1', '--mog-k', '4', '--n-flows', '2',
            '--test-mode', 'True', '--model-state-file', ckpt, '--relation-profile-topk', str(k)]
    for typed in (False, True):
        out = str(tmp_path / f'relations_{typed}.tsv')
        train.main(train.build_parser().parse_args(base + ['--relation-profile-ids', ','.join(map(str, which)), '--relation-profile-out', out]
                                                   + (['--relation-profile-typed'] if typed else [])))
        rows = [line.rstrip('\n').split('\t') for line in open(out)]
        assert all(len(row) == 5 for row in rows) and 0 < len(rows) <= len(which) * k
        groups = [int(row[1]) for row in rows]
        assert [r for i, r in enumerate(groups) if i == 0 or groups[i - 1] != r] == [r for r in which if r in groups]      # the order asked
        for r in set(groups):
            mine = [row for row in rows if int(row[1]) == r]
            assert [int(row[3]) for row in mine] == list(range(1, len(mine) + 1))                                          # rank from 1
            logits = [float(row[4]) for row in mine]
            assert logits == sorted(logits, reverse=True) and (typed or len(mine) == k)
            for s, _, o, _, _ in mine:
                assert (int(s), r, int(o)) not in known and s != o
                assert not typed or (int(s) in seen_s[r] and int(o) in seen_o[r])
    everything = str(tmp_path / 'all.tsv')
    train.main(train.build_parser().parse_args(base + ['--relation-profile-out', everything]))
    rows = [line.split('\t') for line in open(everything)]
    assert len(rows) == kg.num_rels * k and [int(row[1]) for row in rows] == [r for r in range(kg.num_rels) for _ in range(k)]
