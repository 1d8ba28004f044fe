#!/usr/bin/env python3
"""Per-relation completion (ranking.complete_relations: gv_mine_scores_by_relation / gv_mine_scores_typed_by_relation) against the
routes it has to be judged by, alternated in one process, on FB15k-237- and WN18RR-synthetic at h = 200 and 500, k = 100 and
10 000, for all relations and for 3 of them, typed and untyped:
  fused        ranking.complete_relations: every relation's threshold from the same three to five sweeps
  per_relation (a) one whole-graph miner call per relation with a one-row w and that relation's filter (ops.mine_scores; typed:
               ops.mine_scores_typed with that relation's two member lists) -- what the tree offered before
  gemm_topk    (b) ranking.complete_relations_unfused: per relation the materialised GEMM, then torch.topk and the rule
and, once per dataset and width:
  hist_sweep   one HIST sweep of gv_mine_scores_by_relation against gv_mine_scores' at the same size, unfiltered, the counting
               level (every candidate lands in a bin: the price of the per-relation histogram) and a refining level
  coverage     how many relations the global top-100 000 (ranking.mine_triplets) holds, on the random tables and on tables whose
               w rows carry a log-normal scale (sigma = 1), as trained relation rows differ in norm
    python tools/relation_profile_bench.py                       # writes profiles/relation_profile/bench.json
    python tools/relation_profile_bench.py --datasets fb --widths 200 --reps 3
Timing: device events around each call on the current stream -- end to end, so the filter, the member lists and the unit plan are
rebuilt per call, and the host's read-backs between sweeps are inside -- the median of --reps after one warm-up of every route,
the routes taken in turn within a repetition.  --slow-reps bounds the repeats of a route whose warm-up took more than
--slow-ms.  fused and gemm_topk must agree exactly or the run fails."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gcn_vae_amd import data, lib, ops, ranking   # noqa: E402
from gcn_vae_amd.lib import ptr                   # noqa: E402

DATASETS = {'fb': 'FB15k-237-synthetic', 'wn18rr': 'WN18RR-synthetic'}


def same(a, b):
    return (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
            and torch.equal(a[3]['count'], b[3]['count']))


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return out, s.elapsed_time(e)


def bench(routes, reps, slow_ms, slow_reps):
    """{name: fn} -> ({name: result of the warm-up call}, {name: {'median_ms', 'min_ms', 'ms'}})"""
    results, warm = {}, {}
    for name, fn in routes.items():
        results[name], warm[name] = timed(fn)
    times = {name: [] for name in routes}
    for rep in range(reps):
        for name, fn in routes.items():
            if rep < (slow_reps if warm[name] > slow_ms else reps):
                times[name].append(timed(fn)[1])
    return results, {name: {'median_ms': round(statistics.median(t), 3), 'min_ms': round(min(t), 3), 'ms': [round(x, 3) for x in t]}
                     for name, t in times.items()}


def per_relation_route(emb, w, k, rels, filt, members):
    """(a): one miner call per relation with a one-row w, its filter rows and (typed) its two member lists."""
    lo, hi, ent = filt
    num_rels = w.shape[0]
    rows = []
    for r in rels:
        kw = dict(k=k, filt_lo=lo[r::num_rels], filt_hi=hi[r::num_rels], filt_ent=ent)
        if members is None:
            rows.append(ops.mine_scores(emb, w[r:r + 1], **kw))
        else:
            set_ptr, set_ids = members
            obj, subj = set_ids[set_ptr[r]:set_ptr[r + 1]], set_ids[set_ptr[num_rels + r]:set_ptr[num_rels + r + 1]]
            one_ptr = torch.tensor([0, obj.numel(), obj.numel() + subj.numel()], dtype=torch.int64, device=emb.device)
            rows.append(ops.mine_scores_typed(emb, w[r:r + 1], one_ptr, torch.cat([obj, subj]), **kw))
    return rows


def hist_sweeps(emb, w, k, reps):
    """One unfiltered HIST sweep of each kernel, timed with events: the counting level (prefix_bits 0) and one refining level at the
    prefix the walk for K = ``k`` takes there."""
    n, h, num_rels, dev = emb.shape[0], emb.shape[1], w.shape[0], emb.device
    rels = torch.arange(num_rels, dtype=torch.int32, device=dev)
    out = {}

    def glob(prefix_bits, prefix, bin_bits, words):
        lib.call('gv_mine_scores', ptr(emb), h, ptr(w), h, None, None, None, None, 0, 1, 1, 0, prefix_bits, prefix, bin_bits, None, 0,
                 ptr(words), ptr(words), None, 0, n, num_rels, h, lib.stream())

    def slots(prefix_bits, prefix, bin_bits, words):
        lib.call('gv_mine_scores_by_relation', ptr(emb), h, ptr(w), h, None, None, None, None, 0, 1, 1, ptr(rels), num_rels, None,
                 prefix_bits, ptr(prefix), bin_bits, None, 0, None, ptr(words), ptr(words), None, 0, n, num_rels, h, lib.stream())

    def median(fn):
        fn()
        return round(statistics.median(timed(fn)[1] for _ in range(reps)), 3)

    g0, g_words = ops.MINE_LEVELS[0][1], torch.zeros(1 << ops.MINE_LEVELS[0][1], dtype=torch.int64, device=dev)
    s0, s_words = ops.MINE_RELATION_LEVELS[0][1], torch.zeros(num_rels << ops.MINE_RELATION_LEVELS[0][1], dtype=torch.int64, device=dev)
    zero = torch.zeros(num_rels, dtype=torch.int32, device=dev)
    out['global_count_ms'] = median(lambda: glob(0, 0, g0, g_words))
    out['by_relation_count_ms'] = median(lambda: slots(0, zero, s0, s_words))
    # the bins the walks take next
    tail = torch.flip(torch.cumsum(torch.flip(g_words, [0]), 0), [0])
    g_prefix = int(torch.nonzero(tail >= k).max())
    tails = torch.flip(torch.cumsum(torch.flip(s_words.view(num_rels, -1), [1]), 1), [1])
    s_prefix = ((tails >= k).long() * torch.arange(1 << s0, device=dev)).max(1).values.to(torch.int32)
    g1, s1 = ops.MINE_LEVELS[1], ops.MINE_RELATION_LEVELS[1]
    out['global_refine_ms'] = median(lambda: glob(g1[0], g_prefix, g1[1], g_words))
    out['by_relation_refine_ms'] = median(lambda: slots(s1[0], s_prefix, s1[1], s_words))
    out['count_ratio'] = round(out['by_relation_count_ms'] / out['global_count_ms'], 3)
    out['refine_ratio'] = round(out['by_relation_refine_ms'] / out['global_refine_ms'], 3)
    return out


def coverage(emb, w, fi, gen):
    """Relations present in the global top-100 000, on the tables as they are and with log-normal row scales on w."""
    out = {}
    scale = torch.exp(torch.randn(w.shape[0], 1, generator=gen)).to(w.device)
    for name, table in (('random_w', w), ('lognormal_row_scale_w', w * scale)):
        trip = ranking.mine_triplets(emb, table, k=100000, filter_index=fi)[0]
        per = torch.bincount(trip[:, 1], minlength=w.shape[0])
        out[name] = {'relations_in_global_top_100000': int((per > 0).sum()), 'of': int(w.shape[0]),
                     'largest_share': round(float(per.max()) / max(int(per.sum()), 1), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--datasets', type=str, default='fb,wn18rr')
    ap.add_argument('--widths', type=str, default='200,500')
    ap.add_argument('--ks', type=str, default='100,10000')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--slow-ms', type=float, default=2000.0)
    ap.add_argument('--slow-reps', type=int, default=1)
    ap.add_argument('--skip-typed', action='store_true')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'relation_profile', 'bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('relation_profile_bench.py measures on an MI355X; no device found')
    dev = torch.device('cuda')
    report = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'slow_ms': args.slow_ms, 'slow_reps': args.slow_reps,
              'timing': 'device events around each call (end to end: filter, lists and plan rebuilt per call, host read-backs '
                        'inside), median after one warm-up of every route, routes alternated', 'runs': [], 'hist_sweep': [], 'coverage': []}
    if os.path.exists(args.out):                     # a run over part of the cells extends the file
        with open(args.out) as fh:
            old = json.load(fh)
        for key in ('runs', 'hist_sweep', 'coverage'):
            report[key] = old.get(key, [])

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(report, fh, indent=1)

    for key in args.datasets.split(','):
        kg = data.load_data(DATASETS[key])
        n, num_rels = kg.num_nodes, kg.num_rels
        fi = ranking.FilterIndex(n, num_rels, kg.train, kg.valid, kg.test, device=dev)
        tc = ranking.TypeConstraint(n, num_rels, kg.train, kg.valid, kg.test, device=dev)
        three = [num_rels - 1, 0, num_rels // 2]
        for width in (int(x) for x in args.widths.split(',')):
            gen = torch.Generator().manual_seed(0)
            emb = (torch.randn(n, width, generator=gen) * 0.3).to(dev)
            w = torch.randn(num_rels, width, generator=gen).to(dev)
            head = {'dataset': DATASETS[key], 'entities': n, 'relations': num_rels, 'width': width}
            sweeps = dict(head, **hist_sweeps(emb, w, 100, max(args.reps, 3)))
            report['hist_sweep'].append(sweeps)
            print(f"{DATASETS[key]:>20} h={width}: HIST sweep by relation / global, counting {sweeps['by_relation_count_ms']} / "
                  f"{sweeps['global_count_ms']} ms ({sweeps['count_ratio']}x), refining {sweeps['by_relation_refine_ms']} / "
                  f"{sweeps['global_refine_ms']} ms ({sweeps['refine_ratio']}x)", flush=True)
            cov = dict(head, **coverage(emb, w, fi, gen))
            report['coverage'].append(cov)
            print(f"{DATASETS[key]:>20} h={width}: global top-100000 holds {cov['random_w']['relations_in_global_top_100000']} of "
                  f"{num_rels} relations (log-normal row scales: {cov['lognormal_row_scale_w']['relations_in_global_top_100000']})", flush=True)
            save()
            for typed in ((False,) if args.skip_typed else (False, True)):
                for k in (int(x) for x in args.ks.split(',')):
                    for which, rels in (('all', None), ('3', three)):
                        constraint = {'type_constraint': tc} if typed else {}
                        ids = list(range(num_rels)) if rels is None else rels

                        def one_by_one():
                            filt = ranking._mine_filter(fi, n, num_rels, dev)
                            return per_relation_route(emb, w, k, ids, filt, tc.members(dev) if typed else None)

                        routes = {'fused': lambda: ranking.complete_relations(emb, w, k, relations=rels, filter_index=fi, **constraint),
                                  'per_relation': one_by_one,
                                  'gemm_topk': lambda: ranking.complete_relations_unfused(emb, w, k, relations=rels, filter_index=fi,
                                                                                          **constraint)}
                        results, times = bench(routes, args.reps, args.slow_ms, args.slow_reps)
                        if not same(results['fused'], results['gemm_topk']):
                            raise SystemExit(f'{key} h={width} k={k} {which} typed={typed}: the fused and the materialised routes disagree')
                        f, a, b = (times[r]['median_ms'] for r in ('fused', 'per_relation', 'gemm_topk'))
                        report['runs'].append(dict(head, typed=typed, k=k, relations_asked=len(ids), passes=results['fused'][3]['passes'],
                                                   returned=int((results['fused'][0] >= 0).sum()), fused_equals_gemm_topk=True,
                                                   times=times, per_relation_over_fused=round(a / f, 3),
                                                   gemm_topk_over_fused=round(b / f, 3)))
                        print(f"{DATASETS[key]:>20} h={width} {'typed' if typed else 'all pairs':>9} k={k:<6} {which:>3} relations: fused "
                              f"{f:9.2f} ms ({results['fused'][3]['passes']} sweeps) | per relation {a:9.2f} ms ({a / f:6.2f}x) | "
                              f"gemm + topk {b:9.2f} ms ({b / f:6.2f}x)", flush=True)
                        save()
    print('wrote', args.out)


if __name__ == '__main__':
    main()
