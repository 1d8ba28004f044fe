#!/usr/bin/env python3
"""Per-entity completion on the KG-VAE posterior predictive end to end: the fused route (ranking.complete_entities_mc:
gv_entity_topk_scores_mc / gv_entity_topk_scores_typed_mc, then the spread) against what exists without it, alternated in one
process:
  fused_mean     the fused sweep alone (ops.entity_topk_scores{,_typed}_mc behind the same filter / member lists): no spread.
  (a) per-query  predict_topk_mc over the entity's (a, r) queries (typed: the queries with a on the query side of r only),
                 --chunk entities at a time, then a torch merge over each entity's relations.  Same means; it computes the
                 spread of every per-query proposal, so it is compared with the fused route WITH the spread.
  (b) single     S calls of the single-sample complete_entities, one per sample.  S lists, NOT the same answer: the cost
                 yardstick per sample (selection runs S times, the fused sweep selects once per tile).
  (c) unfused    complete_entities_mc_unfused: per sample and relation a GEMM, torch's sigmoid, the materialised (rows, R, N)
                 probabilities; on the all-entities set it runs on the first --unfused-entities entities only and the figure is
                 scaled (both are recorded).
    python tools/entity_profile_mc_bench.py                              # FB15k-237 and WN18RR sizes, width 200
    python tools/entity_profile_mc_bench.py --shapes wn18rr --samples 4 --k 10
Query sets: every entity, and a single one; S in --samples; k in --k; typed and untyped; side 's'; filter and constraint from the
synthetic dataset's train + valid + test; exclude_self off in all routes (predict_topk_mc keeps the loops).  Each figure is the
median of --reps synchronised timed regions after one warm-up of every route, in milliseconds.  A cell whose fused sweep is
expected to run longer than --max-seconds (from the cells measured so far) keeps reps = 1 and drops routes (a) and (c) on the
all-entities set: they are written as "not measured".  Writes profiles/entity_profile_mc/bench.json under --out-dir."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gcn_vae_amd import data, ops, ranking   # noqa: E402
from entity_bench_common import SHAPES, merge_member_queries, same, time_routes   # noqa: E402

NOT_MEASURED = 'not measured'


def bench_shape(shape, samples, ks, reps, chunk, unfused_entities, max_seconds, queries):
    name, h = SHAPES[shape]
    kg = data.load_data(name)
    dev = torch.device('cuda')
    n, num_rels = kg.num_nodes, kg.num_rels
    fi = ranking.FilterIndex(n, num_rels, kg.train, kg.valid, kg.test, device=dev)
    tc = ranking.TypeConstraint(n, num_rels, kg.train, kg.valid, kg.test, device=dev)
    on_query_side = ranking.complete_masks(tc, 's', dev)[0]                  # (R, N): a is a subject of r
    every_side = torch.ones_like(on_query_side)
    gen = torch.Generator().manual_seed(0)
    base = torch.randn(n, h, generator=gen) * 0.3
    w = torch.randn(num_rels, h, generator=gen).to(dev)
    cases = []
    for s in samples:
        z = (base.unsqueeze(0) + 0.1 * torch.randn(s, n, h, generator=gen)).to(dev)
        flps = (0.3 + 0.1 * torch.randn(s, generator=gen)).to(dev)
        for typed in (True, False):
            constraint = dict(type_constraint=tc) if typed else {}
            kw = dict(side='s', filter_index=fi, exclude_self=False)
            lo, hi, ent = ranking._mine_filter(fi, n, num_rels, dev)
            for query in queries:
                ents = torch.arange(n, device=dev) if query == 'all' else torch.tensor([n // 2], device=dev)
                m = ents.numel()
                sample = ents[:min(m, unfused_entities)]
                for k in ks:
                    def fused():
                        return ranking.complete_entities_mc(z, w, ents, k, flow_log_probs=flps, **kw, **constraint)

                    def fused_mean():
                        if typed:
                            return ops.entity_topk_scores_typed_mc(ents, z, w, k, *tc.members(dev), 's', flps, lo, hi, ent, False)
                        return ops.entity_topk_scores_mc(ents, z, w, k, flps, lo, hi, ent, False)

                    def per_query():
                        member = on_query_side if typed else every_side
                        out = []
                        for at in range(0, m, chunk):
                            part = ents[at:at + chunk]
                            rows, rels = torch.nonzero(member[:, part].t(), as_tuple=True)          # row-major, relations ascending
                            if rows.numel():
                                ids, mean, _ = ranking.predict_topk_mc(z, w, part[rows], rels, k, direction='o', filter_index=fi,
                                                                       flow_log_probs=flps, **constraint)
                            else:
                                ids = torch.zeros(0, k, dtype=torch.long, device=dev)
                                mean = torch.zeros(0, k, device=dev)
                            out.append(merge_member_queries(rows, rels, ids, mean, part.numel(), n, num_rels, k, False))
                        return tuple(torch.cat(t) for t in zip(*out))

                    def single():
                        return [ranking.complete_entities(z[i], w, ents, k, flow_log_prob=flps[i], **kw, **constraint) for i in range(s)]

                    def unfused():
                        return ranking.complete_entities_mc_unfused(z, w, sample, k, flow_log_probs=flps, **kw, **constraint)

                    # what the sweep is expected to take, from the single-sample kernel's measured cost per sample so far
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ranking.complete_entities(z[0], w, ents, k, flow_log_prob=flps[0], **kw, **constraint)
                    torch.cuda.synchronize()
                    long = (time.perf_counter() - t0) * s > max_seconds
                    routes = [('fused', fused), ('fused_mean', fused_mean), ('single', single)]
                    if not long or query != 'all':
                        routes += [('per_query', per_query), ('unfused', unfused)]
                    outs, med = time_routes(routes, 1 if long else reps)
                    scale = m / sample.numel()
                    case = dict(samples=s, typed=typed, query=query, entities=m, k=k, reps=1 if long else reps, fused_ms=med['fused'],
                                fused_mean_only_ms=med['fused_mean'], single_sample_x_S_ms=med['single'],
                                single_sample_per_call_ms=med['single'] / s, fused_mean_per_sample_ms=med['fused_mean'] / s,
                                single_over_fused_mean=med['single'] / med['fused_mean'])
                    if 'per_query' in med:
                        equal = same(outs['fused'], outs['per_query'])
                        case.update(per_query_ms=med['per_query'], per_query_over_fused=med['per_query'] / med['fused'],
                                    equal_per_query=equal, unfused_entities=sample.numel(), unfused_ms_measured=med['unfused'],
                                    unfused_ms_scaled=med['unfused'] * scale, unfused_over_fused=med['unfused'] * scale / med['fused'])
                        if not equal:
                            raise SystemExit('the fused route differs from predict_topk_mc + merge')
                    else:
                        case.update(per_query_ms=NOT_MEASURED, unfused_ms_scaled=NOT_MEASURED)
                    fmt = lambda v: f'{v:9.2f}' if isinstance(v, float) else f'{v:>9s}'      # noqa: E731
                    print(f"{shape} S={s:2d} {'typed  ' if typed else 'untyped'} {query:6s} k={k:3d}: fused {fmt(case['fused_ms'])} ms "
                          f"(mean only {fmt(case['fused_mean_only_ms'])}) | S x single-sample {fmt(case['single_sample_x_S_ms'])} ms "
                          f"({case['single_over_fused_mean']:.2f}x of mean only) | predict_topk_mc + merge {fmt(case['per_query_ms'])} ms | "
                          f"unfused {fmt(case['unfused_ms_scaled'])} ms", flush=True)
                    cases.append(case)
    return dict(dataset=name, entities=n, relations=num_rels, width=h, cases=cases)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', type=str, default='fb,wn18rr', help=f'comma list of {sorted(SHAPES)}')
    ap.add_argument('--samples', type=str, default='1,4,16')
    ap.add_argument('--k', type=str, default='10,100')
    ap.add_argument('--queries', type=str, default='all,single')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--chunk', type=int, default=512, help='entities per predict_topk_mc + merge chunk of the per-query route')
    ap.add_argument('--unfused-entities', type=int, default=256)
    ap.add_argument('--max-seconds', type=float, default=1.0,
                    help='a cell whose sweep is expected to run longer is timed once, without the per-query and unfused routes')
    ap.add_argument('--out-dir', type=str, default=os.path.join(ROOT, 'profiles'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('entity_profile_mc_bench measures on the GPU: no device found')
    samples, ks = [int(x) for x in args.samples.split(',')], [int(x) for x in args.k.split(',')]
    out = os.path.join(args.out_dir, 'entity_profile_mc', 'bench.json')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    result = {}
    for s in args.shapes.split(','):                                         # (written after every shape: a long run keeps what it has)
        result[s] = bench_shape(s, samples, ks, args.reps, args.chunk, args.unfused_entities, args.max_seconds, args.queries.split(','))
        with open(out, 'w') as f:
            json.dump(dict(unit='ms, median of timed regions ending in a device synchronise', reps=args.reps, side='s',
                           exclude_self=False, shapes=result), f, indent=1)
            f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main()
