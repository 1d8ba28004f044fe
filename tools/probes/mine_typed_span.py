"""ops-level time of the type-constrained sweeps by span (ops.mine_scores_typed / ops.transe_mine_typed with the member lists and
the filter ranges prepared once), FB15k-237-synthetic, width 200, K = 100 000 and the threshold of that K-th logit; median of 7
synchronised regions.  Prints JSON (profiles/mine_typed/span_probe.json is one run's output)."""
import json, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gcn_vae_amd import data, ops, ranking
kg = data.load_data('FB15k-237-synthetic')
dev = torch.device('cuda')
n, R = kg.num_nodes, kg.num_rels
fi = ranking.FilterIndex(n, R, kg.train, kg.valid, kg.test, device=dev)
tc = ranking.TypeConstraint(n, R, kg.train, kg.valid, kg.test, device=dev)
lo, hi, ent = ranking._mine_filter(fi, n, R, dev)
gen = torch.Generator().manual_seed(0)
emb = (torch.randn(n, 200, generator=gen) * 0.3).to(dev)
w = torch.randn(R, 200, generator=gen).to(dev)
rel = (torch.randn(R, 200, generator=gen) * 0.3).to(dev)
en, rn = ops.transe_queries(emb, norm_flag=True), ops.transe_queries(rel, norm_flag=True)
def t(fn, reps=7):
    fn(); out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); out.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(out), 3)
res = {'members_ms': t(lambda: tc.members(dev)), 'filter_ranges_ms': t(lambda: ranking._mine_filter(fi, n, R, dev))}
ptr, ids = tc.members(dev)
res['plan_ms'] = t(lambda: ops.mine_typed_plan(ptr, R))
res['tile_pairs'] = int(ops.mine_typed_plan(ptr, R, 1).shape[0])
f = dict(filt_lo=lo, filt_hi=hi, filt_ent=ent)
thr = float(ops.mine_scores_typed(emb, w, ptr, ids, k=100000, **f)[1][-1])
for span in (1, 2, 4, 8, 16, 32):
    res[f'distmult_k_span{span}'] = t(lambda: ops.mine_scores_typed(emb, w, ptr, ids, k=100000, span=span, **f))
    res[f'distmult_thr_span{span}'] = t(lambda: ops.mine_scores_typed(emb, w, ptr, ids, threshold=thr, span=span, **f))
for span in (4, 8, 16, 32):
    for p in (1, 2):
        res[f'transe_l{p}_k_span{span}'] = t(lambda: ops.transe_mine_typed(en, rn, p, ptr, ids, k=100000, span=span, **f))
res['distmult_thr_count'] = ops.mine_scores_typed(emb, w, ptr, ids, threshold=thr, **f)[2]['count']
print(json.dumps(res, indent=1))
