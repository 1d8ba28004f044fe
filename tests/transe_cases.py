"""Constructed TransE training-step cases for the float64 tests (test_transe_cases_host.py without a GPU,
test_gpu_transe_f64.py on the device), and their two plain-torch references: ``transe.step_unfused`` on doubles and on the
float32 CPU tables.

``make_case`` lays a batch out as gv_transe_step reads it (OpenKE: B positives, then K blocks of B negatives; every negative keeps
the positive's relation and exactly one of its entities) and plants, in every case,
  * entity 0: an all-zero row (head of positive 0, and the head-corrupted negative 0 of positive 3 when there is one);
  * entity 1: a row of L2 norm 5e-13, below F.normalize's eps (tail of positive 1);
  * entity 2: a row of L2 norm 2e-12, above it (head of positive 2);
  * entity 3: the hot entity, on the free side of positives 0..2 and head or tail of every positive up to ceil(B / 2): a long
    occurrence run for gv_transe_apply;
  * entity V - 1: never drawn, so its row has no occurrence;
  * negative j of positive b corrupts the head when b + j is odd and the tail otherwise: both kinds within one positive once
    K >= 2;
  * the last negative of the last positive is the positive itself (tail "corrupted" to the same id: ns == ps, d = 0).

Scaling.  Under norm_flag the tables are N(0, 1): the scores do not depend on the scale, and the regulariser (which reads the raw
rows) stays visible next to the hinge.  Without it the entries are N(0, s^2) with s chosen for a typical score of 8
(s = 8 / (1.38 dim) for p = 1, 8 / (1.73 sqrt(dim)) for p = 2): at unit scale and dim 200 the scores reach several hundred and
the self-adversarial softmax exp(-ns T) is ill-conditioned in any float32 evaluation.

Margin.  Chosen from the float64 scores: the midpoint of the widest gap between neighbouring values of ns - ps that leaves
between 20 % and 80 % of the (positive, negative) pairs active (ps - ns > -margin), rounded to float32 (MarginLoss holds a
float32 margin).  Learning rate: the power of two nearest to a tenth of (median row max of the table) / (median row max of the
ordinary rows' float64 gradient), so that three steps move an ordinary row by a sizeable share of itself -- a table bound relative
to the row's own size could not see an update much smaller than that.

Ambiguity is a precondition.  Two branches of the step are discontinuous: the sign of z = (h + r) - t for p = 1 and the hinge at
d = -margin.  A float32 evaluation may take the other branch when the float64 value lies within float32 rounding of the edge:
  * element: |z64| < 16 * 2^-23 * (|h| + |r| + |t|), on the normalised operands under norm_flag (p = 1 only: the p = 2 gradient
    z / ||z|| is continuous); an exact zero that the float32 evaluation also makes exactly zero (dim 1 under norm_flag:
    0 + 1 - 1) is no ambiguity, both precisions take sign(0) = 0;
  * pair: |d64 + margin| < 2 * dim * 2^-23 * (|ps| + |ns|).
``make_case`` tries seed, seed + 1, ... (at most 8) and returns the first one whose float64 reference has no such element or pair
in any of the three steps the tests take (the later steps start from tables that moved, so their edges are screened too).  Nothing
is ever left out of a comparison.

Conditioning is a precondition as well (``cancelled_rows``): the bound is relative to a row's summed gradient, so a seed in which
a row's uses cancel to less than 2^-7 of their size is passed over too.  It happens at dim 1 under norm_flag, where every
normalised entry is 0, +-0.5 or +-1: the +-0.2 / 1e-12 uses of a near-zero row can cancel down to the regulariser's 1e-15, which
no float32 summation order but the reference's own keeps.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from gcn_vae_amd import transe

STEPS = 3
MAX_SEEDS = 8
ULP = 2.0 ** -23

# (V, R, dim, B, K) and what each reaches in k_transe_step / k_transe_apply (one wave per positive, 8 register slots of 64 columns)
SHAPES = [
    (50, 5, 1, 5, 1),          # dim 1, one live lane; last block with one live wave
    (97, 7, 63, 5, 2),         # guard inside slot 0
    (97, 7, 64, 4, 3),         # slot 0 exactly full
    (97, 7, 65, 7, 3),         # slot 1 with one lane; B % 4 = 3
    (211, 2, 200, 130, 2),     # the workload's width (slots 0..3, guard in slot 3), 33 blocks, loss sum over B > 64, runs > 64
    (64, 3, 500, 9, 4),        # guard inside the last slot
    (64, 3, 512, 9, 4),        # every slot full
    (30, 2, 128, 257, 1),      # K = 1, B = 257: 65 blocks, the last with one wave, very long runs on 30 entities
]
# (p, norm_flag, adv, regul): every shape sees adv None / 1.0 and regul 0 / 0.01, alone, together and neither
COMBOS = [(1, True, None, 0.01), (1, False, 1.0, 0.0), (2, True, 1.0, 0.01), (2, False, None, 0.0)]
PARAMS = [(s, c) for s in SHAPES for c in COMBOS]


def param_id(param):
    (v, r, dim, b, k), (p, nf, adv, regul) = param
    return f'V{v}-R{r}-dim{dim}-B{b}-K{k}-p{p}-{"norm" if nf else "raw"}-adv{adv or 0:g}-regul{regul:g}'


ZERO, TINY_BELOW, TINY_ABOVE, HOT = 0, 1, 2, 3


def special_tables(V, R, dim, scale, rs):
    """float32 tables N(0, scale^2) with the zero row and the two rows on either side of F.normalize's eps."""
    ent = (rs.standard_normal((V, dim)) * scale).astype(np.float32)
    rel = (rs.standard_normal((R, dim)) * scale).astype(np.float32)
    ent[ZERO] = 0.0
    for row, norm in ((TINY_BELOW, 5e-13), (TINY_ABOVE, 2e-12)):
        x = rs.standard_normal(dim)
        ent[row] = (x * (norm / np.sqrt((x * x).sum()))).astype(np.float32)
    return torch.from_numpy(ent), torch.from_numpy(rel)


def raw_scale(dim, p):
    return 8.0 / (1.38 * dim) if p == 1 else 8.0 / (1.73 * math.sqrt(dim))


def make_batch(V, R, B, K, rs):
    """(bh, br, bt) int64 of B * (1 + K) rows with the planted structure of the module docstring."""
    assert V >= 8 and B >= 4 and K >= 1
    draw = lambda n: rs.randint(0, V - 1, n)          # noqa: E731  entity V - 1 is never drawn
    h, t, r = draw(B), draw(B), rs.randint(0, R, B)
    for b in range(3, (B + 1) // 2):                   # the hot run: head and tail in turn
        if b % 2:
            h[b] = HOT
        else:
            t[b] = HOT
    h[0], t[0] = ZERO, HOT
    h[1], t[1] = HOT, TINY_BELOW
    h[2], t[2] = TINY_ABOVE, HOT
    h[3] = HOT
    bh, br, bt = [h], [r], [t]
    for j in range(K):
        nh, nt = h.copy(), t.copy()
        for b in range(B):
            side, keep = (nh, h[b]) if (b + j) % 2 else (nt, t[b])
            side[b] = (keep + 1 + rs.randint(0, V - 2)) % (V - 1)        # any drawn entity but the one replaced
        if j == 0:
            nh[3] = ZERO                               # b + j odd: a head-corrupted negative on the zero row
        if j == K - 1:
            nh[B - 1], nt[B - 1] = h[B - 1], t[B - 1]  # the negative identical to its positive
        bh.append(nh)
        br.append(r.copy())
        bt.append(nt)
    return [torch.from_numpy(np.concatenate(x).astype(np.int64)) for x in (bh, br, bt)]


def corrupted_ids(c):
    """(K, B) entity id of each negative's corrupted side as the kernel picks it: the head when it differs from the positive's,
    the tail otherwise."""
    B, K = c['B'], c['K']
    nh, nt = c['bh'][B:].view(K, B), c['bt'][B:].view(K, B)
    return torch.where(nh != c['bh'][:B], nh, nt)


def occurrence_ids(c):
    """The entity id of every g_ent row: [h of b | t of b | corrupted side of (j, b)]."""
    B = c['B']
    return torch.cat([c['bh'][:B], c['bt'][:B], corrupted_ids(c).reshape(-1)])


def operands(ent, rel, bh, br, bt, norm_flag):
    h, r, t = ent[bh], rel[br], ent[bt]
    if norm_flag:
        h, r, t = F.normalize(h, 2, -1), F.normalize(r, 2, -1), F.normalize(t, 2, -1)
    return h, r, t


def ambiguity(ent64, rel64, ent32, rel32, bh, br, bt, B, dim, p, norm_flag, margin):
    """(rows (N,) bool with an ambiguous element, pairs (K, B) bool) of one step from these tables, by the two rules of the
    module docstring.  ``ent32`` / ``rel32`` are the float32 tables of the same step (for the exact-zero exemption)."""
    h, r, t = operands(ent64, rel64, bh, br, bt, norm_flag)
    z = (h + r) - t
    if p == 1:
        h32, r32, t32 = operands(ent32, rel32, bh, br, bt, norm_flag)
        exact_zero = (z == 0) & (((h32 + r32) - t32) == 0)
        rows = ((z.abs() < 16 * ULP * (h.abs() + r.abs() + t.abs())) & ~exact_zero).any(1)
    else:
        rows = torch.zeros(z.shape[0], dtype=torch.bool)
    score = torch.norm(z, p, -1)
    ps, ns = score[:B].view(1, B), score[B:].view(-1, B)
    pairs = ((ps - ns) + margin).abs() < 2 * dim * ULP * (ps.abs() + ns.abs())
    return rows, pairs


def cancelled_rows(c):
    """How many table rows' first-step float64 gradient is what is left of a cancellation among the row's uses: row max of the
    summed gradient below 2^-7 of the sum of the uses' row maxima (a use: one gathered h, t or r row of the batch, its gradient
    taken by autograd on the gathered copies).  The bound grants 1e-5 of the SUMMED row's size, while every use is rounded to
    2^-24 of its OWN size in float32, in whatever order an implementation adds them: below 2^-24 / 1e-5 ~ 2^-7 the sum is not
    determined to the bound by float32 arithmetic at all (dim 1 under norm_flag: uses of +-0.2 / 1e-12 on a near-zero row that
    cancel to the regulariser's 1e-15).  A row that is exactly zero in the float64 AND the float32 reference is no such row: equal
    and opposite uses (a positive and the negative identical to it) cancel exactly in any precision."""
    bh, br, bt, B = c['bh'], c['br'], c['bt'], c['B']
    h, r, t = (x.double().clone().requires_grad_(True) for x in (c['ent'][bh], c['rel'][br], c['ent'][bt]))
    score = transe.score_rule(h, r, t, c['p'], c['nf'])
    loss = transe.MarginLoss(c['adv'], c['margin'])(score[:B].view(-1, B).permute(1, 0), score[B:].view(-1, B).permute(1, 0))
    if c['regul'] != 0:
        loss = loss + c['regul'] * ((torch.mean(h ** 2) + torch.mean(t ** 2) + torch.mean(r ** 2)) / 3)
    loss.backward()
    uses_e = torch.zeros(c['V'], dtype=torch.float64).index_add_(0, bh, h.grad.abs().amax(1)).index_add_(0, bt, t.grad.abs().amax(1))
    uses_r = torch.zeros(c['R'], dtype=torch.float64).index_add_(0, br, r.grad.abs().amax(1))
    n = 0
    for g64, g32, uses in ((c['out64'][0][2], c['out32'][0][2], uses_e), (c['out64'][0][3], c['out32'][0][3], uses_r)):
        exact_zero = (g64 == 0).all(1) & (g32 == 0).all(1)
        n += int(((g64.abs().amax(1) * 128 < uses) & ~exact_zero).sum())
    return n


def choose_margin(ps, ns):
    """The float32 margin in the widest gap of ns - ps that leaves 20..80 % of the pairs active, or None."""
    v = torch.sort((ns - ps).reshape(-1)).values
    n = v.numel()
    best = None
    for active in range(math.ceil(0.2 * n), math.floor(0.8 * n) + 1):        # pairs with ns - ps < margin
        if not 0 < active < n:
            continue
        lo, hi = float(v[active - 1]), float(v[active])
        m = float(np.float32(0.5 * (lo + hi)))
        if m > 0 and lo < m < hi and (best is None or hi - lo > best[0]):
            best = (hi - lo, m)
    return None if best is None else best[1]


def run_steps(c, dtype, steps=STEPS):
    """``steps`` plain-torch SGD steps on the case's batch: [(score, loss, g_ent, g_rel)] per step and the (steps + 1) table pairs."""
    ent, rel = c['ent'].to(dtype), c['rel'].to(dtype)
    outs, tables = [], [(ent, rel)]
    for _ in range(steps):
        out = transe.step_unfused(ent, rel, c['bh'], c['br'], c['bt'], c['B'], c['p'], c['nf'], c['margin'], c['adv'], c['regul'])
        ent, rel = ent - c['lr'] * out[2], rel - c['lr'] * out[3]
        outs.append(out)
        tables.append((ent, rel))
    return outs, tables


def build(V, R, dim, B, K, p, norm_flag, adv, regul, seed):
    """One seed's case with its references and its ambiguity counts, or None when no margin leaves 20..80 % of the pairs active."""
    rs = np.random.RandomState(seed)
    ent, rel = special_tables(V, R, dim, 1.0 if norm_flag else raw_scale(dim, p), rs)
    bh, br, bt = make_batch(V, R, B, K, rs)
    c = dict(ent=ent, rel=rel, bh=bh, br=br, bt=bt, V=V, R=R, dim=dim, B=B, K=K, p=p, nf=norm_flag, adv=adv, regul=regul, seed=seed)
    h, r, t = operands(ent.double(), rel.double(), bh, br, bt, norm_flag)
    score = torch.norm((h + r) - t, p, -1)
    ps, ns = score[:B].view(1, B), score[B:].view(-1, B)
    c['margin'] = choose_margin(ps, ns)
    if c['margin'] is None:
        return None
    c['active_share'] = float(((ps - ns) > -c['margin']).double().mean())
    c['lr'] = 1.0
    g = run_steps(c, torch.float64, 1)[0][0][2]
    touched = torch.zeros(V, dtype=torch.bool)
    touched[occurrence_ids(c)] = True
    touched[:HOT] = False                             # the ~1e11 gradients of the zero and tiny rows do not set the step size
    gmax = float(g[touched].abs().amax(1).median())
    xmax = float(ent[HOT:].abs().amax(1).median())
    c['lr'] = 2.0 ** round(math.log2(0.1 * xmax / gmax)) if gmax > 0 else 1.0
    c['out64'], c['tab64'] = run_steps(c, torch.float64)
    c['out32'], c['tab32'] = run_steps(c, torch.float32)
    c['cancelled'] = cancelled_rows(c)
    c['amb_rows'] = c['amb_pairs'] = 0
    for (e64, r64), (e32, r32) in zip(c['tab64'][:STEPS], c['tab32'][:STEPS]):
        rows, pairs = ambiguity(e64, r64, e32, r32, bh, br, bt, B, dim, p, norm_flag, c['margin'])
        c['amb_rows'] += int(rows.sum())
        c['amb_pairs'] += int(pairs.sum())
    return c


@functools.lru_cache(maxsize=None)
def make_case(V, R, dim, B, K, p, norm_flag, adv, regul, seed=0):
    """The first of seeds ``seed`` .. ``seed + 7`` whose case has a margin and no ambiguous element or pair; raises when none has.
    Cached: every test of a process shares one case and its references, and none changes them."""
    tried = []
    for s in range(seed, seed + MAX_SEEDS):
        c = build(V, R, dim, B, K, p, norm_flag, adv, regul, s)
        if c is not None and c['amb_rows'] == 0 and c['amb_pairs'] == 0 and c['cancelled'] == 0:
            return c
        tried.append((s, None if c is None else (c['amb_rows'], c['amb_pairs'], c['cancelled'])))
    raise AssertionError(f'no usable seed among (seed, (ambiguous rows, pairs, cancelled rows) or None without a margin): {tried}')


def case_of(param):
    return make_case(*param[0], *param[1])


def worst_ratio(got, fix, bound):
    """max |got - fix| / bound: how much of the bound the device used."""
    got, fix = got.detach().cpu().double(), torch.as_tensor(np.asarray(fix)).double()
    return float(((got - fix).abs() / bound).max())
