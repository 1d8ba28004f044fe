#!/usr/bin/env python3
"""Raw-MRR evaluation throughput: the whole FB15k-237 test split in both directions
(2 x 20 466 queries against 14 541 entities, h = 200) through the fused rank-count scorer (gv_rank_scores) and through the
materialised form (one GEMM per 100-query batch + torch sigmoid / gather / compare / sum -- what ranking.py did before).
    python tools/eval_bench.py [--cpu-rows 200]     # --cpu-rows: also time the reference's (h, Eb, V) formulation on the host
    python tools/eval_bench.py --filtered           # filtered ranks: raw only, raw + filtered in one launch pair, materialised torch
    python tools/eval_bench.py --topk 10            # top-k link prediction: fused (filtered / unfiltered), materialised, raw ranker
--filtered and --topk take the test split and the filter (train + valid + test) of the FB15k-237-synthetic dataset (Zipf-skewed
lists)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcn_vae_amd import ranking   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cpu-rows', type=int, default=0)
    ap.add_argument('--filtered', action='store_true')
    ap.add_argument('--topk', type=int, default=0)
    args = ap.parse_args()
    if args.filtered:
        return filtered_leg()
    if args.topk:
        return topk_leg(args.topk)
    gen = torch.Generator().manual_seed(0)
    v, h, n, n_rel = 14541, 200, 20466, 237
    emb = (torch.randn(v, h, generator=gen) * 0.3).cuda()
    w = torch.randn(n_rel, h, generator=gen).cuda()
    trip = torch.stack([torch.randint(0, v, (n,), generator=gen), torch.randint(0, n_rel, (n,), generator=gen),
                        torch.randint(0, v, (n,), generator=gen)], 1).cuda()

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps, out

    t_f, mrr_f = timed(lambda: ranking.calc_mrr(emb, w, trip, hits=[1, 3, 10], eval_bz=100, verbose=False), 5)
    fused = ranking.perturb_and_get_rank
    ranking.perturb_and_get_rank = ranking.perturb_and_get_rank_unfused
    try:
        t_u, mrr_u = timed(lambda: ranking.calc_mrr(emb, w, trip, hits=[1, 3, 10], eval_bz=100, verbose=False), 2)
    finally:
        ranking.perturb_and_get_rank = fused
    flop = 2 * 2.0 * n * v * h * 2          # two directions, two passes (target probability, count)
    print(f'fused    : {t_f * 1e3:8.2f} ms per full evaluation ({2 * n} queries)  MRR {mrr_f:.6f}  '
          f'{flop / t_f / 1e12:.1f} TFLOP/s f32 MFMA (two passes)')
    print(f'unfused  : {t_u * 1e3:8.2f} ms (410 batches of 100: GEMM + sigmoid + gather + compare + sum)  MRR {mrr_u:.6f}')
    if args.cpu_rows:
        e, ww = emb.cpu(), w.cpu()
        s, r, o = (trip[:args.cpu_rows, i].cpu() for i in range(3))
        t0 = time.perf_counter()
        emb_ar = (e[s] * ww[r]).transpose(0, 1).unsqueeze(2)            # (h, Eb, 1)   kgvae/utils.py:195-203
        emb_c = e.transpose(0, 1).unsqueeze(1)                          # (h, 1, V)
        score = torch.sigmoid(torch.sum(torch.bmm(emb_ar, emb_c), dim=0))
        _, idx = torch.sort(score, dim=1, descending=True)
        ranks = torch.nonzero(idx == o.view(-1, 1))[:, 1]
        dt = time.perf_counter() - t0
        print(f'host, reference formulation: {dt * 1e3:.1f} ms for {args.cpu_rows} queries -> '
              f'{dt / args.cpu_rows * 2 * n:.1f} s per full evaluation ({torch.get_num_threads()} threads)')


def filtered_leg(chunk=4096, reps=5):
    from gcn_vae_amd import data, ops
    kg = data.load_data('FB15k-237-synthetic')
    dev = torch.device('cuda')
    t0 = time.perf_counter()
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device=dev)
    torch.cuda.synchronize()
    t_index = time.perf_counter() - t0
    gen = torch.Generator().manual_seed(0)
    v, h = kg.num_nodes, 200
    emb = (torch.randn(v, h, generator=gen) * 0.3).to(dev)
    w = torch.randn(kg.num_rels, h, generator=gen).to(dev)
    trip = torch.from_numpy(kg.test).to(dev)
    s, r, o = trip[:, 0], trip[:, 1], trip[:, 2]
    n = trip.shape[0]
    dirs = ((o, s, 's'), (s, o, 'o'))

    def raw_only():
        return [ranking.perturb_and_get_rank(emb, w, a, r, b, n) for a, b, _ in dirs]

    def raw_and_filtered():
        return [ranking.perturb_and_get_rank_filtered(emb, w, a, r, b, n, fi, d) for a, b, d in dirs]

    def materialised():          # one GEMM per chunk of queries, the filter as a dense (chunk, V) mask, torch compare + sum
        out = []
        for a, b, d in dirs:
            lo_all, hi_all = fi.lookup(a, r, d)
            ent = fi.entities(d).long()
            for c in range(0, n, chunk):
                sl = slice(c, min(n, c + chunk))
                q = ops.mul(emb[a[sl]].contiguous(), w[r[sl]].contiguous())
                score = ops.gemm(q, emb, trans_b=True)
                m = score.shape[0]
                lo, hi = lo_all[sl], hi_all[sl]
                lens = hi - lo
                total = int(lens.sum())
                keep = torch.ones_like(score, dtype=torch.bool)
                if total:
                    rows = torch.repeat_interleave(torch.arange(m, device=dev), lens)
                    first = torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)
                    idx = torch.repeat_interleave(lo, lens) + torch.arange(total, device=dev) - first
                    keep[rows, ent[idx]] = False
                t = b[sl].view(-1, 1)
                keep.scatter_(1, t, False)
                tgt = score.gather(1, t)
                out.append(((~(score <= tgt)) & keep).sum(1).float() + 0.5 * ((score == tgt) & keep).sum(1).float())
        return out

    def timed(fn, k):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k, out

    t_raw, _ = timed(raw_only, reps)
    t_both, both = timed(raw_and_filtered, reps)
    t_mat, mat = timed(materialised, 2)
    filt = torch.cat([f for _, f in both])
    assert torch.equal(filt, torch.cat(mat)), 'fused filtered ranks differ from the materialised ones'
    lens = torch.cat([torch.unique_consecutive(fi.keys[d], return_counts=True)[1] for d in 'so'])
    print(f'filter index : {t_index * 1e3:8.2f} ms once ({fi.ent["o"].numel()} distinct triplets; list length mean '
          f'{lens.float().mean():.2f}, max {int(lens.max())})')
    print(f'raw only     : {t_raw * 1e3:8.2f} ms per full evaluation ({2 * n} queries x {v} entities, h = {h})')
    print(f'raw+filtered : {t_both * 1e3:8.2f} ms  ({t_both / t_raw:.2f}x raw only)   filtered MRR '
          f'{(1.0 / (filt + 1)).mean().item():.6f}')
    print(f'materialised : {t_mat * 1e3:8.2f} ms (filtered only: GEMM + dense filter mask + torch compare / sum, '
          f'{chunk}-query chunks)')


def topk_leg(k, reps=5):
    """Top-k link prediction for both directions of the test split: fused with the filter, fused without, the materialised
    path (ranking.predict_topk_unfused: GEMM + dense mask + two stable sorts) and, for scale, the raw-only fused ranker."""
    from gcn_vae_amd import data
    kg = data.load_data('FB15k-237-synthetic')
    dev = torch.device('cuda')
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device=dev)
    gen = torch.Generator().manual_seed(0)
    v, h = kg.num_nodes, 200
    emb = (torch.randn(v, h, generator=gen) * 0.3).to(dev)
    w = torch.randn(kg.num_rels, h, generator=gen).to(dev)
    trip = torch.from_numpy(kg.test).to(dev)
    s, r, o = trip[:, 0], trip[:, 1], trip[:, 2]
    n = trip.shape[0]
    dirs = ((s, o, 'o'), (o, s, 's'))

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps, out

    def fused(filt):
        return [ranking.predict_topk(emb, w, a, r, k, d, fi if filt else None) for a, _, d in dirs]

    def unfused(filt):
        return [ranking.predict_topk_unfused(emb, w, a, r, k, d, fi if filt else None) for a, _, d in dirs]

    t_ff, ff = timed(lambda: fused(True), reps)
    t_fu, fu = timed(lambda: fused(False), reps)
    t_uf, uf = timed(lambda: unfused(True), 2)
    t_raw, _ = timed(lambda: [ranking.perturb_and_get_rank(emb, w, a, r, b, n) for a, b, _ in dirs], reps)
    same_f = all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(ff, uf))
    same_u = all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(fu, unfused(False)))
    flop = 2.0 * (2 * n) * v * h            # one MFMA pass over every (query, entity) pair
    print(f'top-{k}: {2 * n} queries x {v} entities, h = {h}; fused == unfused: filtered {same_f}, unfiltered {same_u}')
    print(f'fused, filtered     : {t_ff * 1e3:8.2f} ms  ({flop / t_ff / 1e12:.1f} TFLOP/s of the score pass)')
    print(f'fused, unfiltered   : {t_fu * 1e3:8.2f} ms  ({flop / t_fu / 1e12:.1f} TFLOP/s)')
    print(f'unfused, filtered   : {t_uf * 1e3:8.2f} ms  (GEMM + dense mask + two stable sorts; {t_uf / t_ff:.1f}x fused)')
    print(f'raw ranker (fused)  : {t_raw * 1e3:8.2f} ms  (two MFMA passes; fused filtered top-{k} is {t_ff / t_raw:.2f}x this)')
    if not (same_f and same_u):
        raise SystemExit('fused top-k differs from the unfused path')


if __name__ == '__main__':
    main()
