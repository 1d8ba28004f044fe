"""Cost of the type-constrained protocol on the Monte-Carlo posterior predictive on an MI355X against its three alternatives, on the
same queries in the same process.

    python tools/mc_type_constraint_bench.py [--repeats 5] [--samples 1 4 16] [--out profiles/mc_type_constraint/bench.json]

Queries: both directions of the FB15k-237-sized synthetic test split (2 x 20 466 queries, 14 541 entities), h = 200, filter and
type sets from train + valid + test (the sets have the synthetic graph's own density), S samples of the entity table (a shared
base plus per-sample noise) with one flow bias each.  Per S and per leg -- the ranks (raw + filtered, and for the constrained
routes the two constrained kinds on top), top-k at k = 10 with the spread -- four routes:
  fused          ranking.perturb_and_get_rank_mc_constrained / predict_topk_mc(type_constraint=...): one launch pair per 4 096
                 queries, pbar never stored
  unconstrained  ranking.perturb_and_get_rank_mc / predict_topk_mc on the same queries: what the constraint costs
  unfused        the materialised twin: S GEMMs, sigmoids and a running sum per 1 024 queries, then count / select under the mask
  separate       S calls of the single-sample constrained ranker / top-k, one per sample: a cost reference (it yields S
                 rankings, not the posterior-predictive one)
The routes of a leg alternate inside every repeat after two untimed rounds of all four; every figure is the median of --repeats
synchronised runs timed with device events, in ms (the minimum is kept too).  The drivers are timed as the CLI calls them,
host-side argument checks and filter / set look-ups included, alike on all sides.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


WARMUP = 2
ROUTES = ('fused', 'unconstrained', 'unfused', 'separate')


def _ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def _stat(out):
    return dict(median_ms=float(np.median(out)), min_ms=float(min(out)), runs=[round(x, 3) for x in out])


def _leg(routes, repeats):
    """The routes alternate inside every repeat (A B C D, A B C D, ...), after WARMUP untimed rounds of all."""
    for _ in range(WARMUP):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fn in routes.items():
            times[name].append(_ms(fn))
    res = {name: _stat(t) for name, t in times.items()}
    for other in ROUTES[1:]:
        res['fused_over_' + other] = res['fused']['median_ms'] / res[other]['median_ms']
    return res


def run(repeats, samples):
    from gcn_vae_amd import ranking
    from gcn_vae_amd.data import load_data
    data = load_data('FB15k-237-synthetic')
    fi = ranking.FilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device='cuda')
    tc = ranking.TypeConstraint(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device='cuda')
    test = torch.as_tensor(np.asarray(data.test), dtype=torch.long).cuda()
    s, r, o = test[:, 0], test[:, 1], test[:, 2]
    n, h = len(test), 200
    sizes = tc.sizes.float()
    res = dict(queries=2 * n, entities=data.num_nodes, width=h, repeats=repeats, warmup=WARMUP, k=10,
               mean_set_share=float((sizes[torch.cat([r, r + data.num_rels])] / data.num_nodes).mean()))
    gen = torch.Generator().manual_seed(0)
    base = torch.randn(data.num_nodes, h, generator=gen) * 0.3
    w = torch.randn(data.num_rels, h, generator=gen).cuda()
    for n_s in samples:
        z = (base[None] + 0.15 * torch.randn(n_s, data.num_nodes, h, generator=gen)).cuda()
        flps = (0.3 + 0.1 * torch.randn(n_s, generator=gen)).cuda()

        def rank(route):
            for a, b, d in ((o, s, 's'), (s, o, 'o')):
                if route == 'fused':
                    ranking.perturb_and_get_rank_mc_constrained(z, w, a, r, b, n, fi, tc, d, flow_log_probs=flps)
                elif route == 'unconstrained':
                    ranking.perturb_and_get_rank_mc(z, w, a, r, b, n, fi, d, flow_log_probs=flps)
                elif route == 'unfused':
                    ranking.perturb_and_get_rank_mc_constrained_unfused(z, w, a, r, b, n, fi, tc, d, flow_log_probs=flps)
                else:
                    for i in range(n_s):
                        ranking.perturb_and_get_rank_constrained(z[i], w, a, r, b, n, fi, tc, d, flow_log_prob=flps[i])

        def topk(route):
            for a, d in ((s, 'o'), (o, 's')):
                if route == 'fused':
                    ranking.predict_topk_mc(z, w, a, r, 10, d, fi, flps, type_constraint=tc)
                elif route == 'unconstrained':
                    ranking.predict_topk_mc(z, w, a, r, 10, d, fi, flps)
                elif route == 'unfused':
                    ranking.predict_topk_mc_unfused(z, w, a, r, 10, d, fi, flps, type_constraint=tc)
                else:
                    for i in range(n_s):
                        ranking.predict_topk(z[i], w, a, r, 10, direction=d, filter_index=fi, flow_log_prob=flps[i],
                                             type_constraint=tc)
        res[f'S{n_s}'] = dict(rank_four_way=_leg({x: (lambda x=x: rank(x)) for x in ROUTES}, repeats),
                              topk_k10=_leg({x: (lambda x=x: topk(x)) for x in ROUTES}, repeats))
        del z
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--samples', type=int, nargs='+', default=[1, 4, 16])
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    a = ap.parse_args()
    res = run(a.repeats, a.samples)
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    for name, legs in res.items():
        if isinstance(legs, dict):
            for leg, v in legs.items():
                print('{:4s} {:14s} '.format(name, leg) + '  '.join('{} {:9.3f} ms'.format(x, v[x]['median_ms']) for x in ROUTES)
                      + '  ' + '  '.join('fused/{} {:.3f}'.format(x, v['fused_over_' + x]) for x in ROUTES[1:]))
    print('RESULT ' + json.dumps(res))


if __name__ == '__main__':
    main()
