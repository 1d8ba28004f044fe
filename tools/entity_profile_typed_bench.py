#!/usr/bin/env python3
"""Per-entity completion among type-correct facts end to end, both models: the fused typed route (complete_entities(type_constraint=):
gv_entity_topk_scores_typed / gv_transe_entity_topk_typed) against the routes that exist without it, alternated in one process:
  (a) per-query  predict_topk(type_constraint=) over the (a, r) queries with a on the query side of r, --chunk entities at a time,
                 then a torch merge over each entity's relations.  Same answer.
  (b) unfused    complete_entities_unfused(type_constraint=): the materialised (rows, R, N) values under the constraint's masks; on
                 the all-entities set it runs on the first --unfused-entities entities only and the figure is scaled (both are
                 recorded).  Same answer.
  (c) untyped    the untyped fused complete_entities.  A DIFFERENT answer: what the constraint saves or costs.
    python tools/entity_profile_typed_bench.py                          # both models, FB15k-237 and WN18RR sizes, width 200
    python tools/entity_profile_typed_bench.py --models distmult --shapes fb
Query sets: every entity, and a single one; k = 10 and 100; side 's'; filter and constraint from the synthetic dataset's train +
valid + test; L1 and L2 for TransE.  End to end: the member lists, the tile prefix and the per-key filter ranges are rebuilt every
call.  Each figure is the median of --reps synchronised timed regions after one warm-up of every route, in milliseconds; the
answers of (a) and (b) are asserted bit-equal to the fused one (exclude_self is off in all: predict_topk keeps the loops).  Also
records the column tiles the typed sweep walks against the untyped R * ceil(N / 64).  Writes
profiles/entity_profile_typed/bench.json (DistMult) and profiles/transe_profile_typed/bench.json (TransE) under --out-dir."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gcn_vae_amd import data, ops, ranking, transe   # noqa: E402
from entity_bench_common import SHAPES, merge_member_queries, same, time_routes   # noqa: E402

OUT = {'distmult': os.path.join('entity_profile_typed', 'bench.json'), 'transe': os.path.join('transe_profile_typed', 'bench.json')}


def bench_shape(model, shape, ks, reps, chunk, unfused_entities):
    name, h = SHAPES[shape]
    kg = data.load_data(name)
    dev = torch.device('cuda')
    n, num_rels = kg.num_nodes, kg.num_rels
    fi = ranking.FilterIndex(n, num_rels, kg.train, kg.valid, kg.test, device=dev)
    tc = ranking.TypeConstraint(n, num_rels, kg.train, kg.valid, kg.test, device=dev)
    set_ptr, _ = tc.members(dev)
    tiles = ops.entity_typed_plan(set_ptr, num_rels, 's')[1]
    on_query_side = ranking.complete_masks(tc, 's', dev)[0]                  # (R, N): a is a subject of r
    sizes = (set_ptr[1:] - set_ptr[:-1]).float()
    geometry = dict(typed_tiles=tiles, untyped_tiles=num_rels * ((n + 63) // 64),
                    mean_object_share=float(sizes[:num_rels].mean()) / n, mean_subject_share=float(sizes[num_rels:].mean()) / n,
                    member_queries=int(on_query_side.sum()), all_queries=n * num_rels)
    gen = torch.Generator().manual_seed(0)
    if model == 'distmult':
        emb = (torch.randn(n, h, generator=gen) * 0.3).to(dev)
        w = torch.randn(num_rels, h, generator=gen).to(dev)
        variants = [(None, dict(flow_log_prob=torch.tensor(0.3, device=dev)))]
    else:
        torch.manual_seed(0)
        net = transe.TransE(n, num_rels, dim=h, p_norm=1, norm_flag=True).cuda()
        ent, rel = net.ent_embeddings.weight.data, net.rel_embeddings.weight.data
        variants = [(1, {}), (2, {})]
    cases = []
    for p, extra in variants:
        kw = dict(side='s', filter_index=fi, exclude_self=False, **extra)
        if model == 'distmult':
            def complete(route, ents, k, **more):
                return route(emb, w, ents, k, **kw, **more)

            def topk(a, r, k):
                return ranking.predict_topk(emb, w, a, r, k, direction='o', filter_index=fi, type_constraint=tc, **extra)
            mod = ranking
        else:
            tables = (ent, rel, p, True)

            def complete(route, ents, k, **more):
                return route(tables, ents, k, **kw, **more)

            def topk(a, r, k):
                return transe.predict_topk(tables, a, r, k, direction='o', filter_index=fi, type_constraint=tc)
            mod = transe
        for query, ents in (('all', torch.arange(n, device=dev)), ('single', torch.tensor([n // 2], device=dev))):
            m = ents.numel()
            sample = ents[:min(m, unfused_entities)]
            for k in ks:
                def fused():
                    return complete(mod.complete_entities, ents, k, type_constraint=tc)

                def per_query():
                    out = []
                    for at in range(0, m, chunk):
                        part = ents[at:at + chunk]
                        rows, rels = torch.nonzero(on_query_side[:, part].t(), as_tuple=True)      # row-major, relations ascending
                        if rows.numel():
                            ids, values = topk(part[rows], rels, k)
                        else:
                            ids = torch.zeros(0, k, dtype=torch.long, device=dev)
                            values = torch.zeros(0, k, device=dev)
                        out.append(merge_member_queries(rows, rels, ids, values, part.numel(), n, num_rels, k, model == 'transe'))
                    return tuple(torch.cat(t) for t in zip(*out))

                def unfused():
                    return complete(mod.complete_entities_unfused, sample, k, type_constraint=tc)

                def untyped():
                    return complete(mod.complete_entities, ents, k)

                outs, med = time_routes([('fused', fused), ('per_query', per_query), ('unfused', unfused), ('untyped', untyped)], reps)
                scale = m / sample.numel()
                case = dict(query=query, entities=m, k=k, fused_ms=med['fused'], per_query_ms=med['per_query'],
                            per_query_over_fused=med['per_query'] / med['fused'], unfused_entities=sample.numel(),
                            unfused_ms_measured=med['unfused'], unfused_ms_scaled=med['unfused'] * scale,
                            unfused_over_fused=med['unfused'] * scale / med['fused'], untyped_fused_ms=med['untyped'],
                            untyped_over_fused=med['untyped'] / med['fused'],
                            rows_with_a_candidate=int((outs['fused'][0][:, 0] >= 0).sum()),
                            equal_per_query=same(outs['fused'], outs['per_query']),
                            equal_unfused=same(tuple(t[:sample.numel()] for t in outs['fused']), outs['unfused']))
                if p is not None:
                    case = dict(p_norm=p, **case)
                print(f"{model} {shape} {'' if p is None else 'L%d ' % p}{query:6s} k={k:3d}: fused typed {case['fused_ms']:8.2f} ms | "
                      f"predict_topk + merge {case['per_query_ms']:8.2f} ms ({case['per_query_over_fused']:.2f}x) | unfused "
                      f"{case['unfused_ms_scaled']:9.2f} ms ({case['unfused_over_fused']:.2f}x, measured on {sample.numel()}) | untyped "
                      f"fused {case['untyped_fused_ms']:8.2f} ms ({case['untyped_over_fused']:.2f}x) | equal: {case['equal_per_query']} "
                      f"{case['equal_unfused']}", flush=True)
                if not (case['equal_per_query'] and case['equal_unfused']):
                    raise SystemExit('the fused typed route differs from a cross-check route')
                cases.append(case)
    return dict(dataset=name, entities=n, relations=num_rels, width=h, filter_triplets=int(fi.ent['o'].numel()), **geometry, cases=cases)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', type=str, default='distmult,transe')
    ap.add_argument('--shapes', type=str, default='fb,wn18rr', help=f'comma list of {sorted(SHAPES)}')
    ap.add_argument('--k', type=str, default='10,100')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--chunk', type=int, default=2048, help='entities per predict_topk + merge chunk of the per-query route')
    ap.add_argument('--unfused-entities', type=int, default=256)
    ap.add_argument('--out-dir', type=str, default=os.path.join(ROOT, 'profiles'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('entity_profile_typed_bench measures on the GPU: no device found')
    ks = [int(x) for x in args.k.split(',')]
    for model in args.models.split(','):
        result = {s: bench_shape(model, s, ks, args.reps, args.chunk, args.unfused_entities) for s in args.shapes.split(',')}
        out = os.path.join(args.out_dir, OUT[model])
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            json.dump(dict(unit='ms, median of timed regions ending in a device synchronise', reps=args.reps, side='s',
                           exclude_self=False, shapes=result), f, indent=1)
            f.write('\n')
        print('wrote', out)


if __name__ == '__main__':
    main()
