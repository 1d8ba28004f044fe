#!/usr/bin/env python3
"""Whole-graph triplet mining: the fused all-relation sweep (ranking.mine_triplets / gv_mine_scores) against the two routes that
exist without it, alternated in one process:
  unfused    ranking.mine_triplets_unfused: one GEMM per relation + torch selection under a running K-th logit
  per-query  ranking.predict_topk (k = 128) over all N x R queries (s, r, ?) in chunks -- a per-row top-k, NOT the global answer
    python tools/mine_bench.py                        # FB15k-237 size (14 541 x 237, h = 200), K = 100 000 + one threshold run
    python tools/mine_bench.py --shape wn18rr         # 40 943 x 11, h = 200
    python tools/mine_bench.py --shape fb-h500        # FB15k-237 size with h = 500: the k-chunked staging
    python tools/mine_bench.py --trace-leg            # only the fused top-K, for `rocprofv3 --kernel-trace --stats -- ...`
    python tools/mine_bench.py --stats-csv kernel_stats.csv      # share of the 155 TF f32 MFMA peak from such a run's table
Each figure is the median of --reps synchronised timed regions after one warm-up of every route.  The filter is the synthetic
dataset's train + valid + test triplets."""
import argparse
import csv
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcn_vae_amd import data, ranking   # noqa: E402

SHAPES = {'fb': ('FB15k-237-synthetic', 200), 'wn18rr': ('WN18RR-synthetic', 200), 'fb-h500': ('FB15k-237-synthetic', 500)}
PEAK_F32_MFMA = 155e12


def pass_flop(n, num_rels, h):
    return 2.0 * n * num_rels * n * h


def stats_leg(path, shape):
    kg = data.load_data(SHAPES[shape][0])
    flop = pass_flop(kg.num_nodes, kg.num_rels, SHAPES[shape][1])
    for row in csv.DictReader(open(path)):
        if 'k_mine<' in row['Name']:
            avg = float(row['AverageNs']) * 1e-9
            print(f"{row['Name']}: {row['Calls']} passes, {avg * 1e3:.2f} ms each, {flop / avg / 1e12:.1f} TFLOP/s = "
                  f"{flop / avg / PEAK_F32_MFMA:.2f} of the f32 MFMA peak ({flop:.3e} flop per pass)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=sorted(SHAPES), default='fb')
    ap.add_argument('--k', type=int, default=100000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--trace-leg', action='store_true')
    ap.add_argument('--stats-csv', type=str, default=None)
    ap.add_argument('--skip', type=str, default='', help='comma list of routes to leave out: unfused, per-query')
    args = ap.parse_args()
    if args.stats_csv:
        return stats_leg(args.stats_csv, args.shape)
    name, h = SHAPES[args.shape]
    kg = data.load_data(name)
    dev = torch.device('cuda')
    n, num_rels = kg.num_nodes, kg.num_rels
    fi = ranking.FilterIndex(n, num_rels, kg.train, kg.valid, kg.test, device=dev)
    gen = torch.Generator().manual_seed(0)
    emb = (torch.randn(n, h, generator=gen) * 0.3).to(dev)
    w = torch.randn(num_rels, h, generator=gen).to(dev)
    flp = torch.tensor(0.3, device=dev)
    kw = dict(filter_index=fi, flow_log_prob=flp)

    def fused_k():
        return ranking.mine_triplets(emb, w, k=args.k, **kw)

    if args.trace_leg:
        for _ in range(3):
            out = fused_k()
        torch.cuda.synchronize()
        print(f'{args.shape}: 3 fused top-{args.k} runs of {out[2]["passes"]} passes each, {pass_flop(n, num_rels, h):.3e} flop per pass')
        return
    t_cut = float(fused_k()[1][-1])

    def fused_t():
        return ranking.mine_triplets(emb, w, threshold=t_cut, **kw)

    def unfused():
        return ranking.mine_triplets_unfused(emb, w, k=args.k, **kw)

    def per_query():
        a = torch.arange(n, device=dev).repeat_interleave(num_rels)
        r = torch.arange(num_rels, device=dev).repeat(n)
        return ranking.predict_topk(emb, w, a, r, 128, direction='o', filter_index=fi, flow_log_prob=flp)

    skip = set(args.skip.split(','))
    routes = [('fused top-K', fused_k), ('fused threshold', fused_t)]
    routes += [(nm, fn) for nm, fn in (('unfused', unfused), ('per-query', per_query)) if nm not in skip]
    times, outs = {nm: [] for nm, _ in routes}, {}
    for nm, fn in routes:                       # warm-up of every route
        outs[nm] = fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):                  # alternated
        for nm, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[nm].append(time.perf_counter() - t0)
    med = {nm: statistics.median(v) for nm, v in times.items()}
    fk = outs['fused top-K']
    passes, flop = fk[2]['passes'], pass_flop(n, num_rels, h)
    print(f'{args.shape}: {n} x {num_rels} x {n} = {n * num_rels * n:.3e} triplets, h = {h}, K = {args.k}, filter {fi.ent["o"].numel()} '
          f'triplets; median of {args.reps}')
    print(f'fused top-K     : {med["fused top-K"] * 1e3:9.2f} ms  ({passes} product passes: {flop * passes / med["fused top-K"] / 1e12:.1f} '
          f'TFLOP/s of wall time, {flop * passes / med["fused top-K"] / PEAK_F32_MFMA:.2f} of the f32 MFMA peak)')
    ft = outs['fused threshold']
    print(f'fused threshold : {med["fused threshold"] * 1e3:9.2f} ms  (logit >= {t_cut:.6g}: {ft[2]["count"]} triplets, 1 pass, '
          f'{flop / med["fused threshold"] / 1e12:.1f} TFLOP/s)')
    if 'unfused' in med:
        u = outs['unfused']
        same = torch.equal(fk[0], u[0]) and torch.equal(fk[1].view(torch.int32), u[1].view(torch.int32))
        print(f'unfused         : {med["unfused"] * 1e3:9.2f} ms  ({med["unfused"] / med["fused top-K"]:.2f}x fused top-K; equal: {same})')
        if not same:
            raise SystemExit('fused mining differs from the unfused path')
    if 'per-query' in med:
        print(f'per-query route : {med["per-query"] * 1e3:9.2f} ms  ({med["per-query"] / med["fused top-K"]:.2f}x fused top-K; '
              f'{n * num_rels} queries, top-128 per query, no global selection)')


if __name__ == '__main__':
    main()
