#!/usr/bin/env python3
"""Type-correct completion on the Monte-Carlo posterior predictive (ranking.mine_triplets_mc: gv_mine_scores_typed_mc) against
the routes it has to be judged by, alternated in one process, for S = 1, 4 and 16 posterior samples:
  fused           ranking.mine_triplets_mc: one sweep per pass whose key is pbar, then the spread of the returned triplets
  fused_sweep     the same without the spread (members + filter + ops.mine_scores_typed_mc): what compares with the floor below
  unfused         ranking.mine_triplets_mc_unfused: per relation and sample, index_select + mul + GEMM + torch sigmoid, a running
                  mean, torch selection -- the real competitor
  single_x_S      S calls of ranking.mine_triplets(..., type_constraint=) on the single samples (gv_mine_scores_typed).  NOT the
                  same answer (S lists, no mean): the cost floor the single-sample sweep already offers
on FB15k-237- and WN18RR-synthetic, h = 200: K = 100 000 and one threshold run (the threshold is the K-th pbar of the top-K run;
the single-sample calls take its logit).
    python tools/mine_typed_mc_bench.py                       # writes profiles/mine_typed_mc/bench.json
    python tools/mine_typed_mc_bench.py --datasets fb --samples 1,4 --reps 3
Each figure is the median of --reps synchronised timed regions after --warmup untimed rounds of every route, the routes taken
in turn within a repetition; end to end, so every route pays for TypeConstraint.members, the filter's ranges and the unit plan
every call.  Sets and filter are the dataset's train + valid + test triplets.  fused and unfused must return the same triplets
wherever the K-th value leaves no doubt, at probabilities within 1e-5, or the run fails."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gcn_vae_amd import data, ops, ranking   # noqa: E402

DATASETS = {'fb': 'FB15k-237-synthetic', 'wn18rr': 'WN18RR-synthetic'}
TOL = 1e-5


def agree(a, b, n, num_rels, edge):
    """the triplets above ``edge`` + TOL of either route are in the other, common triplets' probabilities within TOL"""
    def lin(t):
        return (t[:, 0] * num_rels + t[:, 1]) * n + t[:, 2]
    la, lb = lin(a[0]), lin(b[0])
    if not (bool(torch.isin(la[a[1] > edge + TOL], lb).all()) and bool(torch.isin(lb[b[1] > edge + TOL], la).all())):
        return False
    oa, ob = torch.argsort(la), torch.argsort(lb)
    ia, ib = oa[torch.isin(la[oa], lb)], ob[torch.isin(lb[ob], la)]
    return bool(((a[1][ia] - b[1][ib]).abs() <= TOL).all())


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def bench(routes, reps, warmup):
    results = {}
    for _ in range(warmup):
        results = {name: fn() for name, fn in routes.items()}
    times = {name: [] for name in routes}
    for _ in range(reps):
        for name, fn in routes.items():
            times[name].append(timed(fn)[1] * 1e3)
    return results, {name: {'median_ms': round(statistics.median(t), 3), 'min_ms': round(min(t), 3), 'ms': [round(x, 3) for x in t]}
                     for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--datasets', type=str, default='fb,wn18rr')
    ap.add_argument('--samples', type=str, default='1,4,16')
    ap.add_argument('--width', type=int, default=200)
    ap.add_argument('--k', type=int, default=100000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'mine_typed_mc', 'bench.json'))
    args = ap.parse_args()
    dev = torch.device('cuda')
    report = {'device': torch.cuda.get_device_name(0), 'width': args.width, 'k': args.k, 'reps': args.reps, 'warmup': args.warmup,
              'timing': 'median of synchronised wall-clock regions after the untimed rounds of every route, routes alternated; '
                        'end to end (members, filter ranges and unit plan rebuilt every call)', 'runs': []}
    for key in args.datasets.split(','):
        kg = data.load_data(DATASETS[key])
        n, num_rels = kg.num_nodes, kg.num_rels
        fi = ranking.FilterIndex(n, num_rels, kg.train, kg.valid, kg.test, device=dev)
        tc = ranking.TypeConstraint(n, num_rels, kg.train, kg.valid, kg.test, device=dev)
        for n_samples in (int(x) for x in args.samples.split(',')):
            gen = torch.Generator().manual_seed(0)
            base = torch.randn(n, args.width, generator=gen) * 0.3
            z = (base.unsqueeze(0) + 0.1 * torch.randn(n_samples, n, args.width, generator=gen)).to(dev)
            w = torch.randn(num_rels, args.width, generator=gen).to(dev)
            flps = (0.1 * torch.randn(n_samples, generator=gen)).to(dev)
            sel, last = {'k': args.k}, None
            for kind in ('topk', 'threshold'):
                if kind == 'threshold':                 # the K-th pbar of the top-K run just made
                    p = float(last['fused'][1][-1])
                    sel = {'threshold': p}
                    one = {'threshold': math.inf if p >= 1.0 else -math.inf if p <= 0.0 else math.log(p / (1.0 - p))}
                else:
                    one = dict(sel)

                def sweep(s=sel):
                    lo, hi, ent = ranking._mine_filter(fi, n, num_rels, dev)
                    set_ptr, set_ids = ranking._mine_members(tc, n, num_rels, dev)
                    return ops.mine_scores_typed_mc(z, w, set_ptr, set_ids, bias=flps, filt_lo=lo, filt_hi=hi, filt_ent=ent, **s)

                routes = {'fused': lambda s=sel: ranking.mine_triplets_mc(z, w, filter_index=fi, type_constraint=tc, flow_log_probs=flps, **s),
                          'fused_sweep': sweep,
                          'unfused': lambda s=sel: ranking.mine_triplets_mc_unfused(z, w, filter_index=fi, type_constraint=tc,
                                                                                    flow_log_probs=flps, **s),
                          'single_x_S': lambda s=one: [ranking.mine_triplets(z[i], w, filter_index=fi, type_constraint=tc,
                                                                             flow_log_prob=flps[i], **s) for i in range(n_samples)]}
                results, times = bench(routes, args.reps, args.warmup)
                fused, unfused = results['fused'], results['unfused']
                edge = sel['threshold'] if kind == 'threshold' else min(float(fused[1].min()), float(unfused[1].min()))
                if not agree(fused, unfused, n, num_rels, edge):
                    raise SystemExit(f'{key} S={n_samples} {kind}: the fused and the unfused route disagree')
                last = results
                f, fs, u, o = (times[r]['median_ms'] for r in ('fused', 'fused_sweep', 'unfused', 'single_x_S'))
                run = {'dataset': DATASETS[key], 'entities': n, 'relations': num_rels, 'samples': n_samples, 'query': kind,
                       'selection': dict(sel), 'returned': int(fused[0].shape[0]), 'count': fused[3]['count'],
                       'passes': fused[3]['passes'], 'fused_agrees_with_unfused': True, 'times': times,
                       'unfused_over_fused': round(u / f, 3), 'single_x_S_over_fused_sweep': round(o / fs, 3),
                       'fused_sweep_ms_per_sample': round(fs / n_samples, 3), 'single_ms_per_sample': round(o / n_samples, 3)}
                report['runs'].append(run)
                print(f"{DATASETS[key]:>20} S={n_samples:<2} {kind:>9}: fused {f:9.2f} ms (sweep alone {fs:9.2f}) | unfused {u:9.2f} ms "
                      f"({u / f:6.2f}x) | {n_samples} single-sample calls {o:9.2f} ms ({o / fs:6.2f}x the sweep)", flush=True)
                os.makedirs(os.path.dirname(args.out), exist_ok=True)
                with open(args.out, 'w') as fh:
                    json.dump(report, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
