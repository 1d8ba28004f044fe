#!/usr/bin/env python3
"""TransE at FB15k-237-synthetic size with baselines/transe/main.py's hyperparameters (dim 200, L1, norm_flag, margin 5,
nbatches 100, neg_ent 25, bern, filter, SGD alpha 1): µs per training step eager and graph-replayed, an epoch of 100 steps,
raw + filtered evaluation of the test split, and the same for the plain-torch formulation of the reference on the same GPU
(autograd + torch.optim.SGD on the fused sampler's batches; materialised distances + sort_and_rank).  Each case runs in a child
process under a time limit and stops the bench at its first failure.

    python tools/transe_bench.py [--steps 200] [--warmup 20] [--limit 600]
    python tools/transe_bench.py --topk [--out profiles/transe_topk/bench.json]
    python tools/transe_bench.py --mine [--out profiles/transe_mine/bench.json]
    python tools/transe_bench.py --profile [--profile-shapes fb,wn18rr,fb-dim500] [--out profiles/transe_profile/bench.json]
    python tools/transe_bench.py --relation-profile [--relation-profile-shapes fb,wn18rr,fb-dim500,wn18rr-dim500]

--topk runs the link-prediction leg alone: both directions of the test split (40 932 queries), filter = train + valid + test,
L1 and L2, k = 10 and 100; per configuration predict_topk (fused), predict_topk_unfused (materialised distances + sort) and
rank_transe on the same queries (the bare distance sweep with a counting epilogue).  Each is warmed up once and timed over
--topk-repeats synchronised runs; the median and the minimum are reported, in ms.

--mine runs the completion leg alone: the 100 000 nearest new triplets of ALL 14 541 x 237 x 14 541, train + valid + test
filtered, dim 200 with L1 and L2 and dim 500 with L1 and L2: mine_triplets (fused) against mine_triplets_unfused (per-relation
materialised distances + torch selection) in the same process, each warmed up once, medians of --mine-repeats (unfused: half as
many) synchronised runs; the two results are asserted bit-equal.  At dim 200 predict_topk(k = 128) over all N x R queries is timed
once as well -- it answers another question (the best 128 per query, not the global K).

--profile runs the per-entity completion leg alone: an entity's k nearest new facts over all relations (side 's', train + valid +
test filtered, loops kept as predict_topk keeps them), FB15k-237 and WN18RR sizes, dim 200, L1 and L2, k = 10 and 100, for every
entity and for a single one: complete_entities (fused) against predict_topk over all m x R queries + a torch merge, and against
complete_entities_unfused -- on the all-entities set measured on 256 entities and scaled, which the JSON says.  All three in one
process, each warmed up once, medians of --profile-repeats synchronised runs; the answers are asserted bit-equal.

--relation-profile runs the per-relation completion leg alone: each relation's own K nearest new facts (train + valid + test filtered,
loops left out), FB15k-237 and WN18RR sizes, dim 200 and 500, L1 and L2, typed and untyped, K = 10 and 1 000, for every relation
and for three: complete_relations (fused) against one transe_mine(k = K) call per relation on that relation's row and filter
slice, and against complete_relations_unfused.  All three in one process, each warmed up once, medians of
--relation-profile-repeats synchronised runs; the answers are asserted bit-equal.  It also reports how many relations the graph's
100 000 nearest new triplets (mine_triplets) touch.  Output: profiles/transe_relation_profile/bench.json.

--opt runs the optimiser leg alone (python tools/transe_bench.py --opt [--out profiles/transe_opt/bench.json]): the whole step at
the workload above with SGD, Adagrad, Adadelta and Adam, eager and captured, the four interleaved over --opt-rounds rounds of
--steps steps in one process (medians and minima in µs, and each method over SGD); then the update alone on one batch's
occurrence rows: ops.transe_apply_opt against transe.apply_unfused (index_add_ + torch.optim on the same device and rows) and
against plain SGD's ops.transe_apply.  Its bytes are an upper estimate: the occurrence rows read once, plus every table and state
array read and written once (all rows for Adadelta / Adam, the touched rows otherwise), against 8 TB/s.

Step bytes: algorithmic, counting the gathered rows (3 per positive + 1 per negative), the occurrence gradients written and read,
and the touched table rows read and written once, against 8 TB/s.  Scorer: |a - b| terms at ~1.5 VALU instructions each against
the 157 TFLOP/s fp32 vector rate (an estimate of the floor; the fraction reported is floor / measured)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM, VALU = 8e12, 157e12


def setup():
    from gcn_vae_amd import transe
    from gcn_vae_amd.data import load_data
    data = load_data('FB15k-237-synthetic')
    torch.manual_seed(0)
    model = transe.TransE(data.num_nodes, data.num_rels, dim=200, p_norm=1, norm_flag=True).cuda()
    return data, model


def timed(fn, n, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3      # us


def case_step(steps, warmup):
    from gcn_vae_amd import transe
    data, model = setup()
    tr = transe.DeviceTrainer(model, data.train, 100, 25, True, True, 5.0, 1.0)
    eager = timed(tr.step, steps, warmup)
    tr.capture()
    graph = timed(tr.step, steps, warmup)
    t0 = time.time()
    loss = tr.epoch()
    epoch_ms = (time.time() - t0) * 1e3
    B, K, dim = tr.batch, 25, 200
    rows = B * (3 + K)                                    # gathered rows
    occ = (2 + K) * B + B                                 # gradient rows written, then read
    touched = min(data.num_nodes, (2 + K) * B) + min(data.num_rels, B)
    nbytes = 4 * dim * (rows + 2 * occ + 2 * touched)
    return dict(step_eager_us=eager, step_graph_us=graph, epoch_ms=epoch_ms, epoch_loss=loss, batch=B,
                step_bytes=nbytes, step_hbm_floor_us=nbytes / HBM * 1e6, hbm_fraction_graph=nbytes / HBM * 1e6 / graph)


def case_eval(steps, warmup):
    from gcn_vae_amd import transe
    from gcn_vae_amd.ranking import FilterIndex
    data, model = setup()
    fi = FilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device='cuda')
    test = torch.as_tensor(np.asarray(data.test), dtype=torch.long)
    ent, rel = model.ent_embeddings.weight.data, model.rel_embeddings.weight.data
    fn = lambda: transe.rank_transe(ent, rel, test, 1, True, fi)  # noqa: E731
    us = timed(fn, 3, 1)
    terms = 2 * len(test) * data.num_nodes * 200
    floor_us = terms * 1.5 / VALU * 1e6
    out = transe.evaluate(model, test, fi, verbose=False)
    return dict(eval_ms=us / 1e3, terms=terms, valu_floor_ms_estimate=floor_us / 1e3, valu_fraction=floor_us / us,
                mrr_raw=out['mrr_raw'], mrr_filtered=out['mrr_filtered'])


def case_torch_step(steps, warmup):
    from gcn_vae_amd import transe
    data, model = setup()
    tr = transe.DeviceTrainer(model, data.train, 100, 25, True, True, 5.0, 1.0)
    ns = transe.NegativeSampling(model, transe.MarginLoss(margin=5.0), batch_size=tr.batch).cuda()
    opt = torch.optim.SGD(ns.parameters(), lr=1.0)
    from gcn_vae_amd import ops

    def step():
        tr.rng.tick()
        ops.transe_sample(tr.rng.state, tr.stream_id, tr.train, model.ent_tot, tr.batch, 25, tr.p_head, tr.filt, tr.bh, tr.br, tr.bt)
        opt.zero_grad()
        loss = ns({'batch_h': tr.bh.long(), 'batch_t': tr.bt.long(), 'batch_r': tr.br.long(), 'mode': 'normal'})
        loss.backward()
        opt.step()
    return dict(torch_step_us=timed(step, min(steps, 100), warmup))


def case_torch_eval(steps, warmup):
    from gcn_vae_amd import transe
    from gcn_vae_amd.ranking import FilterIndex
    data, model = setup()
    fi = FilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device='cuda')
    test = torch.as_tensor(np.asarray(data.test), dtype=torch.long)
    ent, rel = model.ent_embeddings.weight.data, model.rel_embeddings.weight.data
    us = timed(lambda: transe.rank_transe_unfused(ent, rel, test, 1, True, fi), 1, 0)
    return dict(torch_eval_ms=us / 1e3)


def _repeat_ms(fn, repeats):
    fn()                                                  # warm-up: library load, allocator, LDS attribute
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e))
    return dict(median_ms=float(np.median(out)), min_ms=float(min(out)), runs=[round(x, 3) for x in out])


def case_topk(steps, warmup, repeats=5):
    from gcn_vae_amd import transe
    from gcn_vae_amd.ranking import FilterIndex
    data, model = setup()
    fi = FilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device='cuda')
    test = torch.as_tensor(np.asarray(data.test), dtype=torch.long).cuda()
    ent, rel = model.ent_embeddings.weight.data, model.rel_embeddings.weight.data
    s, r, o = test[:, 0], test[:, 1], test[:, 2]
    res = dict(queries=2 * len(test), entities=data.num_nodes, dim=200, repeats=repeats)
    for p in (1, 2):
        tables = (ent, rel, p, True)

        def both(fn, k):
            fn(tables, s, r, k, direction='o', filter_index=fi)
            fn(tables, o, r, k, direction='s', filter_index=fi)
        res[f'rank_p{p}'] = _repeat_ms(lambda: transe.rank_transe(ent, rel, test, p, True, fi), repeats)
        for k in (10, 100):
            fused = _repeat_ms(lambda: both(transe.predict_topk, k), repeats)
            unfused = _repeat_ms(lambda: both(transe.predict_topk_unfused, k), max(2, repeats // 2))
            res[f'p{p}_k{k}'] = dict(fused=fused, unfused=unfused, unfused_over_fused=unfused['median_ms'] / fused['median_ms'],
                                     fused_over_rank=fused['median_ms'] / res[f'rank_p{p}']['median_ms'])
    return res


def case_mine(steps, warmup, repeats=3):
    from gcn_vae_amd import transe
    from gcn_vae_amd.data import load_data
    from gcn_vae_amd.ranking import FilterIndex
    data = load_data('FB15k-237-synthetic')
    fi = FilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device='cuda')
    n, num_rels, k = data.num_nodes, data.num_rels, 100000
    res = dict(entities=n, relations=num_rels, k=k, repeats=repeats)

    def say(*a):
        print(*a, file=sys.stderr, flush=True)
    for dim in (200, 500):
        torch.manual_seed(0)
        model = transe.TransE(n, num_rels, dim=dim, p_norm=1, norm_flag=True).cuda()
        ent, rel = model.ent_embeddings.weight.data, model.rel_embeddings.weight.data
        for p in (1, 2):
            tables = (ent, rel, p, True)
            got = transe.mine_triplets(tables, k=k, filter_index=fi)
            want = transe.mine_triplets_unfused(tables, k=k, filter_index=fi)
            assert got[0].shape == (k, 3) and torch.equal(got[0], want[0]) and got[2]['count'] == want[2]['count']
            assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
            fused = _repeat_ms(lambda: transe.mine_triplets(tables, k=k, filter_index=fi), repeats)
            unfused = _repeat_ms(lambda: transe.mine_triplets_unfused(tables, k=k, filter_index=fi), max(1, repeats // 2))
            # the distance sweep alone: n * R * n pairs of dim terms, two vector operations each, per pass
            floor_ms = 2.0 * n * num_rels * n * dim / (VALU / 2) * 1e3
            out = dict(fused=fused, unfused=unfused, unfused_over_fused=unfused['median_ms'] / fused['median_ms'],
                       passes=got[2]['passes'], count=got[2]['count'], bit_equal=True, farthest=float(got[1][-1]),
                       pass_floor_ms=floor_ms, floor_over_fused_pass=floor_ms * got[2]['passes'] / fused['median_ms'])
            say(f'dim {dim} p {p}', json.dumps(out))
            if dim == 200:
                a = torch.arange(n, device='cuda').repeat_interleave(num_rels)
                r = torch.arange(num_rels, device='cuda').repeat(n)
                torch.cuda.synchronize()
                t0 = time.time()
                transe.predict_topk(tables, a, r, 128, direction='o', filter_index=fi)
                torch.cuda.synchronize()
                out['predict_topk_128_all_queries_ms'] = (time.time() - t0) * 1e3
                say(f'dim {dim} p {p} predict_topk over {a.numel()} queries: {out["predict_topk_128_all_queries_ms"]:.0f} ms')
            res[f'dim{dim}_p{p}'] = out
    return res


PROFILE_SHAPES = {'fb': ('FB15k-237-synthetic', 200), 'wn18rr': ('WN18RR-synthetic', 200), 'fb-dim500': ('FB15k-237-synthetic', 500)}


def case_profile(steps, warmup, repeats=3, shapes='fb,wn18rr', chunk=2048, unfused_entities=256):
    """The per-entity completion leg: transe.complete_entities (fused) against (a) transe.predict_topk over all m * R queries of the
    entities, ``chunk`` entities at a time, + a torch merge over each entity's R x k answers, and (b) transe.complete_entities_unfused
    -- on the all-entities set measured on the first ``unfused_entities`` entities and scaled by m / that (both recorded)."""
    from gcn_vae_amd import transe
    from gcn_vae_amd.data import load_data
    from gcn_vae_amd.ranking import FilterIndex
    from entity_bench_common import merge_all_queries, same

    def say(*a):
        print(*a, file=sys.stderr, flush=True)

    res = dict(unit='ms; each route warmed up once, then the median of synchronised timed runs, all in one process', repeats=repeats,
               side='s', exclude_self=False, shapes={})
    for shape in shapes.split(','):
        name, dim = PROFILE_SHAPES[shape]
        data = load_data(name)
        n, num_rels = data.num_nodes, data.num_rels
        fi = FilterIndex(n, num_rels, data.train, data.valid, data.test, device='cuda')
        torch.manual_seed(0)
        model = transe.TransE(n, num_rels, dim=dim, p_norm=1, norm_flag=True).cuda()
        ent, rel = model.ent_embeddings.weight.data, model.rel_embeddings.weight.data
        rels = torch.arange(num_rels, device='cuda')
        cases = []
        for p in (1, 2):
            tables = (ent, rel, p, True)
            for query, ents in (('all', torch.arange(n, device='cuda')), ('single', torch.tensor([n // 2], device='cuda'))):
                m = ents.numel()
                sample = ents[:min(m, unfused_entities)]
                for k in (10, 100):
                    kw = dict(side='s', filter_index=fi, exclude_self=False)         # predict_topk keeps the loops

                    def fused():
                        return transe.complete_entities(tables, ents, k, **kw)

                    def per_query():
                        out = []
                        for at in range(0, m, chunk):
                            part = ents[at:at + chunk]
                            ids, dist = transe.predict_topk(tables, part.repeat_interleave(num_rels), rels.repeat(part.numel()), k,
                                                            direction='o', filter_index=fi)
                            out.append(merge_all_queries(ids, dist, part.numel(), n, num_rels, k, True))
                        return tuple(torch.cat(t) for t in zip(*out))

                    def unfused():
                        return transe.complete_entities_unfused(tables, sample, k, **kw)

                    got = fused()
                    eq_q, eq_u = same(got, per_query()), same(tuple(t[:sample.numel()] for t in got), unfused())
                    t_f = _repeat_ms(fused, repeats)
                    t_q = _repeat_ms(per_query, max(1, repeats - 1) if query == 'all' else repeats)
                    t_u = _repeat_ms(unfused, max(1, repeats - 1))
                    scale = m / sample.numel()
                    case = dict(p_norm=p, query=query, entities=m, k=k, fused=t_f, per_query=t_q,
                                per_query_over_fused=t_q['median_ms'] / t_f['median_ms'], unfused_entities=sample.numel(),
                                unfused_measured=t_u, unfused_ms_scaled=t_u['median_ms'] * scale,
                                unfused_over_fused=t_u['median_ms'] * scale / t_f['median_ms'], equal_per_query=eq_q,
                                equal_unfused=eq_u)
                    say(f"{shape} L{p} {query:6s} k={k:3d}: fused {t_f['median_ms']:9.2f} ms | predict_topk + merge "
                        f"{t_q['median_ms']:9.2f} ms ({case['per_query_over_fused']:.2f}x) | unfused {case['unfused_ms_scaled']:10.2f} ms "
                        f"({case['unfused_over_fused']:.2f}x, measured on {sample.numel()} entities) | equal: {eq_q} {eq_u}")
                    if not (eq_q and eq_u):
                        raise SystemExit('the fused route differs from a cross-check route')
                    cases.append(case)
        res['shapes'][shape] = dict(dataset=name, entities=n, relations=num_rels, dim=dim, filter_triplets=int(fi.ent['o'].numel()),
                                    cases=cases)
    return res


RELATION_SHAPES = dict(PROFILE_SHAPES, **{'wn18rr-dim500': ('WN18RR-synthetic', 500)})


def case_relation_profile(steps, warmup, repeats=3, shapes='fb,wn18rr,fb-dim500,wn18rr-dim500', cover_k=100000):
    """The per-relation completion leg: transe.complete_relations (fused: every relation's own threshold from the same few sweeps)
    against (a) one ops.transe_mine[_typed](k=K) call per relation on that relation's row of the normalised table and its slice of
    the filter (and its two member lists), and (b) transe.complete_relations_unfused; L1 and L2, typed and untyped, K = 10 and
    1 000, every relation and three relations.  The three answers are asserted bit-equal.  Per shape and norm it also counts the
    relations that the graph's ``cover_k`` nearest new triplets (mine_triplets) touch."""
    from gcn_vae_amd import ops, transe
    from gcn_vae_amd.data import load_data
    from gcn_vae_amd.ranking import FilterIndex, TypeConstraint, _mine_filter

    def say(*a):
        print(*a, file=sys.stderr, flush=True)

    def same(a, b):
        return (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
                and torch.equal(a[3]['count'], b[3]['count']))

    res = dict(unit='ms; each route warmed up once, then the median of synchronised timed runs, all in one process', repeats=repeats,
               exclude_self=True, shapes={})
    for shape in shapes.split(','):
        name, dim = RELATION_SHAPES[shape]
        data = load_data(name)
        n, num_rels = data.num_nodes, data.num_rels
        fi = FilterIndex(n, num_rels, data.train, data.valid, data.test, device='cuda')
        tc = TypeConstraint(n, num_rels, data.train, data.valid, data.test, device='cuda')
        set_ptr, set_ids = tc.members(torch.device('cuda'))
        lo, hi, f_ent = _mine_filter(fi, n, num_rels, torch.device('cuda'))
        torch.manual_seed(0)
        model = transe.TransE(n, num_rels, dim=dim, p_norm=1, norm_flag=True).cuda()
        ent, rel = model.ent_embeddings.weight.data, model.rel_embeddings.weight.data
        en, rn = ops.transe_queries(ent, norm_flag=True), ops.transe_queries(rel, norm_flag=True)
        cases, covered = [], {}
        for p in (1, 2):
            tables = (ent, rel, p, True)
            trip = transe.mine_triplets(tables, k=cover_k, filter_index=fi)[0]
            covered[f'p{p}'] = int(torch.unique(trip[:, 1]).numel())
            say(f'{shape} L{p}: the graph\'s {cover_k} nearest new triplets touch {covered[f"p{p}"]} of {num_rels} relations')
            for typed in (False, True):
                constrained = dict(type_constraint=tc) if typed else {}
                for which, rels in (('all', list(range(num_rels))), ('three', [num_rels - 1, 0, num_rels // 2])):
                    for k in (10, 1000):
                        def fused():
                            return transe.complete_relations(tables, k, relations=rels, filter_index=fi, **constrained)

                        def per_relation():
                            rows = []
                            for r in rels:
                                f = dict(filt_lo=lo[r::num_rels], filt_hi=hi[r::num_rels], filt_ent=f_ent)
                                if typed:
                                    o_ids = set_ids[set_ptr[r]:set_ptr[r + 1]]
                                    s_ids = set_ids[set_ptr[num_rels + r]:set_ptr[num_rels + r + 1]]
                                    ptr_r = torch.tensor([0, o_ids.numel(), o_ids.numel() + s_ids.numel()], device='cuda')
                                    rows.append(ops.transe_mine_typed(en, rn[r:r + 1], p, ptr_r, torch.cat([o_ids, s_ids]), k=k, **f))
                                else:
                                    rows.append(ops.transe_mine(en, rn[r:r + 1], p, k=k, **f))
                            return rows

                        def unfused():
                            return transe.complete_relations_unfused(tables, k, relations=rels, filter_index=fi, **constrained)

                        got = fused()
                        eq_u = same(got, unfused())
                        eq_r = all(torch.equal(t[:, 0], got[0][i][:t.shape[0]]) and torch.equal(t[:, 2], got[1][i][:t.shape[0]])
                                   and torch.equal(d.view(torch.int32), got[2][i][:t.shape[0]].view(torch.int32))
                                   and info['count'] == int(got[3]['count'][i]) and bool((got[0][i][t.shape[0]:] < 0).all())
                                   for i, (t, d, info) in enumerate(per_relation()))
                        t_f = _repeat_ms(fused, repeats)
                        t_r = _repeat_ms(per_relation, max(1, repeats - 1))
                        t_u = _repeat_ms(unfused, max(1, repeats - 1))
                        case = dict(p_norm=p, typed=typed, relations=which, m=len(rels), k=k, passes=got[3]['passes'], fused=t_f,
                                    per_relation_miner=t_r, per_relation_miner_over_fused=t_r['median_ms'] / t_f['median_ms'],
                                    unfused=t_u, unfused_over_fused=t_u['median_ms'] / t_f['median_ms'], equal_per_relation=eq_r,
                                    equal_unfused=eq_u)
                        say(f"{shape} L{p} {'typed  ' if typed else 'untyped'} {which:5s} k={k:4d}: fused {t_f['median_ms']:9.2f} ms "
                            f"({got[3]['passes']} sweeps) | miner per relation {t_r['median_ms']:9.2f} ms "
                            f"({case['per_relation_miner_over_fused']:.2f}x) | unfused {t_u['median_ms']:9.2f} ms "
                            f"({case['unfused_over_fused']:.2f}x) | equal: {eq_r} {eq_u}")
                        if not (eq_r and eq_u):
                            raise SystemExit('the fused route differs from a cross-check route')
                        cases.append(case)
        res['shapes'][shape] = dict(dataset=name, entities=n, relations=num_rels, dim=dim, filter_triplets=int(fi.ent['o'].numel()),
                                    cover_k=cover_k, relations_covered_by_mine_triplets=covered, cases=cases)
    return res


OPT_ALPHA = {'sgd': 1.0, 'adagrad': 0.1, 'adadelta': 1.0, 'adam': 1e-3}


def _rounds(fns, n, warmup, rounds):
    """{name: {median_us, min_us, runs}} of ``timed`` over ``rounds`` interleaved rounds (every function once per round)."""
    out = {k: [] for k in fns}
    for r in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, n, warmup if r == 0 else 3))
    return {k: dict(median_us=float(np.median(v)), min_us=float(min(v)), runs=[round(x, 2) for x in v]) for k, v in out.items()}


def case_opt(steps, warmup, rounds=5):
    """The optimiser leg: the whole training step per method (eager, then captured), the methods interleaved round by round in
    one process next to plain SGD; then the update alone on one batch's occurrence rows -- ops.transe_apply_opt against
    transe.apply_unfused (index_add_ + torch.optim, same device, same rows) and against plain SGD's ops.transe_apply."""
    from gcn_vae_amd import ops, transe
    data, _ = setup()
    methods = ('sgd', 'adagrad', 'adadelta', 'adam')
    trainers = {}
    for m in methods:
        torch.manual_seed(0)
        model = transe.TransE(data.num_nodes, data.num_rels, dim=200, p_norm=1, norm_flag=True).cuda()
        trainers[m] = transe.DeviceTrainer(model, data.train, 100, 25, True, True, 5.0, OPT_ALPHA[m], opt_method=m)
    tr = trainers['sgd']
    B, K, dim = tr.batch, 25, 200
    rows = data.num_nodes + data.num_rels
    res = dict(batch=B, neg_ent=K, dim=dim, table_rows=rows, steps=steps, rounds=rounds, alpha=OPT_ALPHA,
               step_eager=_rounds({m: t.step for m, t in trainers.items()}, steps, warmup, rounds))
    for t in trainers.values():
        t.capture()
    res['step_graph'] = _rounds({m: t.step for m, t in trainers.items()}, steps, warmup, rounds)
    for kind in ('step_eager', 'step_graph'):
        for m in methods:
            res[kind][m]['over_sgd'] = res[kind][m]['median_us'] / res[kind]['sgd']['median_us']
    # the update alone, on the occurrence rows the SGD trainer's last step left in its buffers
    torch.cuda.synchronize()
    g_ent, g_rel, part = tr.grads
    parts = tr.order.parts
    occ_e, occ_r = tr.occ_ent.long(), tr.br[:B].long()
    loss = torch.zeros(1, device='cuda')
    fns = {}
    keep = []
    for m in methods:
        ent, rel = tr.ent.clone(), tr.rel.clone()
        state = ops.TransEOptState(ent.shape[0], rel.shape[0], dim, ent.device)
        fns[m + '_fused'] = (lambda m=m, ent=ent, rel=rel, state=state:
                             ops.transe_apply_opt(ent, rel, g_ent, g_rel, parts, m, OPT_ALPHA[m], part, 5.0, loss, state=state))
        ent2, rel2 = tr.ent.clone(), tr.rel.clone()
        opt = transe.make_optimizer([ent2, rel2], m, OPT_ALPHA[m])
        fns[m + '_unfused'] = (lambda ent2=ent2, rel2=rel2, opt=opt: transe.apply_unfused(ent2, rel2, g_ent, occ_e, g_rel, occ_r, opt))
        keep.append((ent, rel, state, ent2, rel2, opt))
    ent0, rel0 = tr.ent.clone(), tr.rel.clone()
    fns['sgd_transe_apply'] = lambda: ops.transe_apply(ent0, rel0, g_ent, g_rel, parts, 1.0, part, 5.0, loss)
    res['apply'] = _rounds(fns, steps, warmup, rounds)
    for m in methods:
        f, u = res['apply'][m + '_fused'], res['apply'][m + '_unfused']
        arrays = {'sgd': 0, 'adagrad': 4, 'adadelta': 6, 'adam': 6}[m]       # table + state arrays, each read and written
        dense = m in ('adadelta', 'adam')
        nbytes = 4 * dim * ((2 + K) * B + B) + (4 * dim * rows * arrays if dense else
                                                 4 * dim * (min(data.num_nodes, (2 + K) * B) + min(data.num_rels, B)) * max(arrays, 2))
        res['apply'][m] = dict(unfused_over_fused=u['median_us'] / f['median_us'], bytes_upper=nbytes,
                               hbm_floor_us=nbytes / HBM * 1e6, hbm_fraction=nbytes / HBM * 1e6 / f['median_us'])
    return res


def case_mine_trace(steps, warmup):
    """What ``rocprofv3 --kernel-trace --stats -- python tools/transe_bench.py --case mine_trace`` profiles: the fused top-K route
    alone, dim 200, L1 then L2, a warm-up and two runs each."""
    from gcn_vae_amd import transe
    from gcn_vae_amd.data import load_data
    from gcn_vae_amd.ranking import FilterIndex
    data = load_data('FB15k-237-synthetic')
    fi = FilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device='cuda')
    torch.manual_seed(0)
    model = transe.TransE(data.num_nodes, data.num_rels, dim=200, p_norm=1, norm_flag=True).cuda()
    ent, rel = model.ent_embeddings.weight.data, model.rel_embeddings.weight.data
    passes = {}
    for p in (1, 2):
        for _ in range(3):
            passes[f'p{p}'] = transe.mine_triplets((ent, rel, p, True), k=100000, filter_index=fi)[2]['passes']
    torch.cuda.synchronize()
    return dict(runs_per_norm=3, passes=passes)


CASES = {'mine_trace': case_mine_trace, 'step': case_step, 'eval': case_eval, 'torch_step': case_torch_step, 'torch_eval': case_torch_eval}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--limit', type=int, default=600)
    ap.add_argument('--case', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--topk', action='store_true', help='run the link-prediction leg alone')
    ap.add_argument('--topk-repeats', type=int, default=5)
    ap.add_argument('--mine', action='store_true', help='run the completion leg alone')
    ap.add_argument('--mine-repeats', type=int, default=3)
    ap.add_argument('--opt', action='store_true', help='run the optimiser leg alone')
    ap.add_argument('--opt-rounds', type=int, default=5)
    ap.add_argument('--profile', action='store_true', help='run the per-entity completion leg alone')
    ap.add_argument('--profile-repeats', type=int, default=3)
    ap.add_argument('--profile-shapes', default='fb,wn18rr', help=f'comma list of {sorted(PROFILE_SHAPES)}')
    ap.add_argument('--relation-profile', action='store_true', help='run the per-relation completion leg alone')
    ap.add_argument('--relation-profile-repeats', type=int, default=3)
    ap.add_argument('--relation-profile-shapes', default='fb,wn18rr,fb-dim500,wn18rr-dim500', help=f'comma list of {sorted(RELATION_SHAPES)}')
    ap.add_argument('--out', default=None, help='with --topk / --mine / --opt / --profile / --relation-profile: also write the JSON '
                                                'result to this file (--profile: profiles/transe_profile/bench.json, '
                                                '--relation-profile: profiles/transe_relation_profile/bench.json unless given)')
    a = ap.parse_args()
    if a.case == 'mine':
        print('RESULT ' + json.dumps(case_mine(a.steps, a.warmup, a.mine_repeats)))
        return
    if a.case == 'topk':
        print('RESULT ' + json.dumps(case_topk(a.steps, a.warmup, a.topk_repeats)))
        return
    if a.case == 'opt':
        print('RESULT ' + json.dumps(case_opt(a.steps, a.warmup, a.opt_rounds)))
        return
    if a.case == 'profile':
        print('RESULT ' + json.dumps(case_profile(a.steps, a.warmup, a.profile_repeats, a.profile_shapes)))
        return
    if a.case == 'relation_profile':
        print('RESULT ' + json.dumps(case_relation_profile(a.steps, a.warmup, a.relation_profile_repeats, a.relation_profile_shapes)))
        return
    if a.profile and a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'transe_profile', 'bench.json')
    if a.relation_profile and a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'transe_relation_profile', 'bench.json')
    if a.topk or a.mine or a.opt or a.profile or a.relation_profile:
        leg = ['--case', 'topk', '--topk-repeats', str(a.topk_repeats)] if a.topk else ['--case', 'mine', '--mine-repeats',
                                                                                           str(a.mine_repeats)]
        if a.opt:
            leg = ['--case', 'opt', '--opt-rounds', str(a.opt_rounds), '--steps', str(a.steps), '--warmup', str(a.warmup)]
        if a.profile:
            leg = ['--case', 'profile', '--profile-repeats', str(a.profile_repeats), '--profile-shapes', a.profile_shapes]
        if a.relation_profile:
            leg = ['--case', 'relation_profile', '--relation-profile-repeats', str(a.relation_profile_repeats),
                   '--relation-profile-shapes', a.relation_profile_shapes]
        # the mining and the profile legs report each configuration on stderr as it finishes
        r = subprocess.run(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__)] + leg,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE if a.topk else None, text=True, cwd=ROOT)
        line = [x for x in r.stdout.splitlines() if x.startswith('RESULT ')]
        if r.returncode != 0 or not line:
            print(json.dumps(dict(failed=r.returncode, tail=(r.stdout + (r.stderr or ''))[-1500:])), file=sys.stderr)
            sys.exit(1)
        text = json.dumps(json.loads(line[0][7:]), indent=1)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write(text + '\n')
        return
    if a.case:
        print('RESULT ' + json.dumps(CASES[a.case](a.steps, a.warmup)))
        return
    res = {}
    for name in ('step', 'eval', 'torch_step', 'torch_eval'):
        r = subprocess.run(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--case', name,
                            '--steps', str(a.steps), '--warmup', str(a.warmup)], capture_output=True, text=True, cwd=ROOT)
        line = [x for x in r.stdout.splitlines() if x.startswith('RESULT ')]
        if r.returncode != 0 or not line:
            res[name] = dict(failed=r.returncode, tail=(r.stdout + r.stderr)[-1500:])
            print(json.dumps(res[name]), file=sys.stderr)
            break
        res[name] = json.loads(line[0][7:])
        print(name, json.dumps(res[name]), flush=True)
    print(json.dumps(res))
    sys.exit(1 if any('failed' in v for v in res.values()) else 0)


if __name__ == '__main__':
    main()
