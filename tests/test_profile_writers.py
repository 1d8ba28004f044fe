"""The per-entity profile TSVs (train.write_entity_profiles, train.write_mc_entity_profiles, transe.write_entity_profiles): the
formatter on hand-made results and the three writers over a stubbed route, both against the text written out here (no GPU); and,
on the GPU, the writers' loop over sides and chunks against one un-chunked call of the route per side."""
import functools

import pytest
import torch

NAN, INF = float('nan'), float('inf')
ENTS = [7, 2, 7]                                                     # m = 3 with a repeat, k = 3
# per side: three facts, an all-padding row, a single fact -- values 1/3 (nine digits), 0.0, -0.0 and a NaN among them
REL = {'s': [[1, 0, 2], [-1, -1, -1], [4, -1, -1]], 'o': [[3, -1, -1], [-1, -1, -1], [0, 2, 2]]}
OTHER = {'s': [[5, 3, 9], [-1, -1, -1], [0, -1, -1]], 'o': [[8, -1, -1], [-1, -1, -1], [6, 1, 4]]}
FIRST = {'s': [[1 / 3, 0.0, -0.0], [-INF, -INF, -INF], [NAN, -INF, -INF]], 'o': [[2.5, -INF, -INF], [-INF, -INF, -INF], [0.1, 0.0, NAN]]}
SECOND = {'s': [[0.75, 0.5, -0.0], [0.0, 0.0, 0.0], [NAN, 0.0, 0.0]], 'o': [[1 / 3, 0.0, 0.0], [0.0, 0.0, 0.0], [0.25, NAN, 0.0]]}

LOGIT_PROB = ('7\ts\t1\t5\t1\t0.333333343\t0.582570195\n7\ts\t0\t3\t2\t0\t0.5\n7\ts\t2\t9\t3\t-0\t0.5\n7\ts\t4\t0\t1\tnan\tnan\n'
              '7\to\t3\t8\t1\t2.5\t0.924141824\n7\to\t0\t6\t1\t0.100000001\t0.524979174\n7\to\t2\t1\t2\t0\t0.5\n7\to\t2\t4\t3\tnan\tnan\n')
MEAN_STD = ('7\ts\t1\t5\t1\t0.333333343\t0.75\n7\ts\t0\t3\t2\t0\t0.5\n7\ts\t2\t9\t3\t-0\t-0\n7\ts\t4\t0\t1\tnan\tnan\n'
            '7\to\t3\t8\t1\t2.5\t0.333333343\n7\to\t0\t6\t1\t0.100000001\t0.25\n7\to\t2\t1\t2\t0\tnan\n7\to\t2\t4\t3\tnan\t0\n')
DISTANCE = ('7\ts\t1\t5\t1\t0.333333343\n7\ts\t0\t3\t2\t0\n7\ts\t2\t9\t3\t-0\n7\ts\t4\t0\t1\tnan\n'
            '7\to\t3\t8\t1\t2.5\n7\to\t0\t6\t1\t0.100000001\n7\to\t2\t1\t2\t0\n7\to\t2\t4\t3\tnan\n')


def _results(side, n_values):
    return (torch.tensor(REL[side]), torch.tensor(OTHER[side]), torch.tensor(FIRST[side]), torch.tensor(SECOND[side]))[:2 + n_values]


def test_formatter_counts_from_one_drops_padding_and_writes_nine_digits():
    from gcn_vae_amd import train
    for n_values, text in ((2, MEAN_STD), (1, DISTANCE)):
        lines = [line for side in ('s', 'o') for line in train.profile_lines(side, ENTS, *_results(side, n_values))]
        assert ''.join(lines) == text and all(line.endswith('\n') for line in lines)
    rel, other, logits = _results('s', 1)
    assert ''.join(train.profile_lines('s', torch.tensor(ENTS), rel, other, logits, torch.sigmoid(logits))) == LOGIT_PROB[:LOGIT_PROB.index('7\to')]
    assert train.profile_lines('o', [], *(t[:0] for t in _results('o', 2))) == []


def test_writers_write_s_lines_then_o_lines_of_their_route(tmp_path, monkeypatch):
    """Every writer over a stubbed route that answers with the tables above: the file's text, and the count returned."""
    from gcn_vae_amd import ranking, train, transe

    def route(n_values):
        def complete(*args, side, **kw):
            assert args[-2].tolist() == ENTS and args[-1] == 3
            return _results(side, n_values)
        return complete

    monkeypatch.setattr(ranking, 'complete_entities', route(1))
    monkeypatch.setattr(ranking, 'complete_entities_mc', route(2))
    monkeypatch.setattr(transe, 'complete_entities', route(1))
    emb, w, path = torch.zeros(10, 4), torch.zeros(5, 4), str(tmp_path / 'p.tsv')
    for text, write in ((LOGIT_PROB, lambda: train.write_entity_profiles(path, emb, w, ENTS, 3, None)),
                        (MEAN_STD, lambda: train.write_mc_entity_profiles(path, emb.unsqueeze(0), w, ENTS, 3, None)),
                        (DISTANCE, lambda: transe.write_entity_profiles(path, (emb, w, 1, True), ENTS, 3, None))):
        assert write() == 8
        with open(path) as f:
            assert f.read() == text


@pytest.mark.gpu
def test_writers_loop_over_sides_and_chunks_equals_one_call_per_side(tmp_path, monkeypatch):
    """n = 70 (two 64-column tiles, the second partial), R = 3, h = 8, k = 5, entities [69, 0, 69] two per chunk: a repeat, and a
    chunk boundary inside the three.  A filter lists a few facts of the query entities on either side."""
    from gcn_vae_amd import ranking, train, transe
    n, num_rels, h, k, ents = 70, 3, 8, 5, [69, 0, 69]
    gen = torch.Generator().manual_seed(70 * 3 + 8)
    emb, w = (torch.randn(n, h, generator=gen) * 0.5).cuda(), torch.randn(num_rels, h, generator=gen).cuda()
    z = (emb.cpu().unsqueeze(0) + 0.2 * torch.randn(2, n, h, generator=gen)).cuda()
    flps = torch.tensor([0.3, -0.2]).cuda()
    fi = ranking.FilterIndex(n, num_rels, [[69, 0, 1], [69, 2, 64], [0, 1, 69], [5, 1, 0], [69, 1, 0], [33, 2, 69]], device='cuda')
    tables = (emb, w, 1, True)
    small = functools.partial(train.write_profile_lines, rows=2)
    monkeypatch.setattr(train, 'write_profile_lines', small)
    monkeypatch.setattr(transe, 'write_profile_lines', small)
    part, path = torch.tensor(ents).cuda(), str(tmp_path / 'p.tsv')

    def logit_prob(side):
        rel, other, logits = ranking.complete_entities(emb, w, part, k, side=side, filter_index=fi, flow_log_prob=0.25)
        return rel, other, logits, torch.sigmoid(logits)

    for write, route in ((lambda: train.write_entity_profiles(path, emb, w, ents, k, fi, flow_log_prob=0.25), logit_prob),
                         (lambda: train.write_mc_entity_profiles(path, z, w, ents, k, fi, flow_log_probs=flps),
                          lambda side: ranking.complete_entities_mc(z, w, part, k, side=side, filter_index=fi, flow_log_probs=flps)),
                         (lambda: transe.write_entity_profiles(path, tables, ents, k, fi),
                          lambda side: transe.complete_entities(tables, part, k, side=side, filter_index=fi))):
        want = [line for side in ('s', 'o') for line in train.profile_lines(side, ents, *route(side))]
        assert len(want) == 2 * 3 * k                                 # 70 * 3 candidates a row less a few: no padding here
        assert write() == len(want)
        with open(path) as f:
            assert f.readlines() == want
