"""Cost of the Monte-Carlo posterior-predictive ranker and top-k on an MI355X against its two alternatives, on the same queries in
the same process.

    python tools/mc_bench.py [--repeats 5] [--samples 1 4 16] [--out profiles/mc/bench.json]

Queries: both directions of the FB15k-237-sized synthetic test split (2 x 20 466 queries, 14 541 entities), h = 200, the filter
from train + valid + test, S samples of the entity table (a shared base plus per-sample noise) with one flow bias each.  Per S
and per leg -- rank raw, rank raw + filtered, top-k at k = 10 (with the spread) -- three routes:
  fused      ranking.perturb_and_get_rank_mc / predict_topk_mc: one launch pair per 4 096 queries, pbar never stored
  separate   (a) S calls of the existing single-sample ranker / top-k, one per sample: the price of S separate evaluations (it
             yields S rankings, not the posterior-predictive one)
  unfused    (b) the materialised route: S GEMMs, sigmoids and a running sum per 1 024 queries, then compare / select
The routes of a leg alternate inside every repeat after two untimed rounds of all three; every figure is the median of --repeats
synchronised runs timed with device events, in ms (the minimum is kept too).  The drivers are timed as the CLI calls them, host-side
argument checks and filter look-ups included, alike on all sides.
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
    """The routes alternate inside every repeat (A B C, A B C, ...), after WARMUP untimed rounds of all."""
    for _ in range(WARMUP):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fn in routes.items():
            times[name].append(_ms(fn))
    res = {name: _stat(t) for name, t in times.items()}
    res['fused_over_separate'] = res['fused']['median_ms'] / res['separate']['median_ms']
    res['fused_over_unfused'] = res['fused']['median_ms'] / res['unfused']['median_ms']
    return res


def run(repeats, samples):
    from gcn_vae_amd import ranking
    from gcn_vae_amd.data import load_data
    data = load_data('FB15k-237-synthetic')
    fi = ranking.FilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device='cuda')
    test = torch.as_tensor(np.asarray(data.test), dtype=torch.long).cuda()
    s, r, o = test[:, 0], test[:, 1], test[:, 2]
    n, h = len(test), 200
    res = dict(queries=2 * n, entities=data.num_nodes, width=h, repeats=repeats, warmup=WARMUP, k=10)
    gen = torch.Generator().manual_seed(0)
    base = torch.randn(data.num_nodes, h, generator=gen) * 0.3
    w = torch.randn(data.num_rels, h, generator=gen).cuda()
    for n_s in samples:
        z = (base[None] + 0.15 * torch.randn(n_s, data.num_nodes, h, generator=gen)).cuda()
        flps = (0.3 + 0.1 * torch.randn(n_s, generator=gen)).cuda()

        def rank(route, filt):
            f = fi if filt else None
            for a, b, d in ((o, s, 's'), (s, o, 'o')):
                if route == 'fused':
                    ranking.perturb_and_get_rank_mc(z, w, a, r, b, n, f, d, flow_log_probs=flps)
                elif route == 'unfused':
                    ranking.perturb_and_get_rank_mc_unfused(z, w, a, r, b, n, f, d, flow_log_probs=flps)
                else:
                    for i in range(n_s):
                        if filt:
                            ranking.perturb_and_get_rank_filtered(z[i], w, a, r, b, n, fi, d, flow_log_prob=flps[i])
                        else:
                            ranking.perturb_and_get_rank(z[i], w, a, r, b, n, flow_log_prob=flps[i])

        def topk(route):
            for a, d in ((s, 'o'), (o, 's')):
                if route == 'fused':
                    ranking.predict_topk_mc(z, w, a, r, 10, d, fi, flps)
                elif route == 'unfused':
                    ranking.predict_topk_mc_unfused(z, w, a, r, 10, d, fi, flps)
                else:
                    for i in range(n_s):
                        ranking.predict_topk(z[i], w, a, r, 10, direction=d, filter_index=fi, flow_log_prob=flps[i])
        routes = ('fused', 'separate', 'unfused')
        res[f'S{n_s}'] = dict(
            rank_raw=_leg({x: (lambda x=x: rank(x, False)) for x in routes}, repeats),
            rank_raw_filtered=_leg({x: (lambda x=x: rank(x, True)) for x in routes}, repeats),
            topk_k10=_leg({x: (lambda x=x: topk(x)) for x in routes}, repeats))
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
                print('{:4s} {:18s} fused {:9.3f} ms  separate {:9.3f} ms  unfused {:9.3f} ms  fused/separate {:.3f}  '
                      'fused/unfused {:.3f}'.format(name, leg, v['fused']['median_ms'], v['separate']['median_ms'],
                                                    v['unfused']['median_ms'], v['fused_over_separate'], v['fused_over_unfused']))
    print('RESULT ' + json.dumps(res))


if __name__ == '__main__':
    main()
