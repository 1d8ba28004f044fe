"""TEST INFRASTRUCTURE ONLY -- float64 reference of the block-diagonal R-GCN aggregation family (K1: gv_rgcn_bdd_aggregate,
gv_rgcn_bdd_aggregate_phases, gv_rgcn_bdd_aggregate_lds, gv_rgcn_bdd_grad_weight) with an element-wise error bound.

Aggregation, row i, block b, output column q (W[r] block b is P x Q, stored Q x P when transposed):

    out_iq = keep_scale * keep_iq * act(sum_{e -> i} c_e sum_p x[s_e, bP+p] W[r_e]_b[p, q] + addend_iq)

    |got - ref| <= keep_scale * ((n_i + 1) u S_iq + 3 u |addend_iq|) + TINY,      S_iq = sum_e |c_e| sum_p |x W|,  u = 2**-24

n_i counts the roundings a term passes through in the kernels' order of operations:
  * per-row and phase kernels: the block product is an fma chain over P (P), the coefficient is applied by the fma that adds
    the product into the item's accumulator (1), the item's accumulator takes at most d_i such adds, and the fix-up of a row
    split into m items sums the m partial slots in order (m).  n_i = P + 1 + d_i + m_i;
  * LDS-resident kernel: the inputs are scaled by the coefficient first (1), a lane accumulates IPL inputs of every edge
    (IPL d_i), the five input groups of a block are summed by three shifts (3), then the slot sum (m).  n_i = 4 + IPL d_i + m_i.
    With bf16 operands the reference takes the ROUNDED operands: bf16(fp32(c x)) and bf16(W), whose products are exact in fp32.
Then one rounding for the addend and one for the keep scale (the + 1 and the 3 u |addend|); ReLU is 1-Lipschitz.

Weight gradient, relation r (accumulate: + the old value):

    gW[r]_b[p, q] = sum_{e in r} c_e x[s_e, bP+p] g[d_e, bQ+q]
    |got - ref| <= (d_r + m_r + 3) u sum_e |c_e x g| + u |old| + TINY

(x c rounded once, one fma per edge into the item's accumulator, the ordered slot sum of the m_r items, the old value.)
Rows without edges are exact: act(addend) * keep * scale (0 without addend); relations without edges: 0 (or the old rows).
"""
import torch

U = 2.0 ** -24 * (1 + 2.0 ** -20)       # one rounding, second-order terms included
TINY = 2.0 ** -126


def round_bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def chunks_of(deg, chunk):
    """Items of a row of ``deg`` edges cut into <= chunk-edge items; the fix-up sums them only when there are two or more."""
    if chunk is None:
        return torch.zeros_like(deg)
    m = (deg + chunk - 1) // chunk
    return torch.where(m > 1, m, torch.zeros_like(m))


def _blocks(weight, nb, p, q, trans):
    """W as [R, nb, P, Q] (the gathered width first) in float32."""
    w = weight.float().reshape(weight.shape[0], nb, q, p).transpose(2, 3) if trans else weight.float().reshape(-1, nb, p, q)
    return w


def edge_terms(feat, weight, nbrs, etypes, coef, nb, p, q, trans=False, bf16=False):
    """Per-edge contributions c_e x[s_e] W[r_e] and their absolute sums, float64 [E, nb*Q] each."""
    e = nbrs.numel()
    x = feat.float()[nbrs.long()].reshape(e, nb, p)
    c = torch.ones(e) if coef is None else coef.float().reshape(-1)
    w = _blocks(weight, nb, p, q, trans)
    if bf16:
        x = round_bf16(x * c.view(-1, 1, 1))
        w = round_bf16(w)
        c = torch.ones(e)
    x64, c64 = x.double(), c.double().view(-1, 1)
    val = torch.zeros(e, nb * q, dtype=torch.float64)
    mag = torch.zeros(e, nb * q, dtype=torch.float64)
    et = etypes.long()
    for r in torch.unique(et).tolist():
        sel = torch.nonzero(et == r).flatten()
        w64 = w[r].double()
        val[sel] = torch.einsum('ebp,bpq->ebq', x64[sel], w64).reshape(-1, nb * q)
        mag[sel] = torch.einsum('ebp,bpq->ebq', x64[sel].abs(), w64.abs()).reshape(-1, nb * q)
    return val * c64, mag * c64.abs()


def aggregate(feat, weight, rows, nbrs, etypes, coef, n_rows, nb, p, q, trans=False, addend=None, act=0, keep=None,
              keep_scale=1.0, chunk=None, lds_ipl=None, bf16=False, terms=None):
    """(want, bound, degree) of one K1 launch; ``rows`` is the output row of every edge, ``nbrs`` its gathered row.
    ``lds_ipl``: the LDS-resident kernel's inputs per lane (its order of operations), None: the per-row / phase kernels'."""
    val, mag = edge_terms(feat, weight, nbrs, etypes, coef, nb, p, q, trans, bf16) if terms is None else terms
    ri = rows.long()
    s = torch.zeros(n_rows, nb * q, dtype=torch.float64).index_add_(0, ri, val)
    sabs = torch.zeros(n_rows, nb * q, dtype=torch.float64).index_add_(0, ri, mag)
    deg = torch.bincount(ri, minlength=n_rows)
    m = chunks_of(deg, chunk)
    n = (4 + lds_ipl * deg + m) if lds_ipl else (p + 1 + deg + m)
    bnd = (n + 1).double().view(-1, 1) * U * sabs
    want = s
    if addend is not None:
        a64 = addend.double()
        want = want + a64
        bnd = bnd + 3 * U * a64.abs()
    if act:
        want = torch.relu(want)
    if keep is not None:
        k = keep.bool()
        want = torch.where(k, want * keep_scale, torch.zeros((), dtype=torch.float64))
        bnd = torch.where(k, bnd * keep_scale, torch.zeros((), dtype=torch.float64))
    return want, bnd + TINY, deg


def edgeless_rows(n_rows, out_dim, addend=None, act=0, keep=None, keep_scale=1.0):
    """What a row without edges holds, in float32 exactly as the epilogue computes it."""
    v = torch.zeros(n_rows, out_dim) if addend is None else addend.float().clone()
    if act:
        v = torch.relu(v)
    if keep is not None:
        v = torch.where(keep.bool(), v * torch.tensor(keep_scale, dtype=torch.float32), torch.zeros(()))
    return v


def grad_weight(x, g, src, dst, etypes, coef, num_rels, nb, p, q, chunk=None, old=None):
    """(want, bound, edges per relation) of gv_rgcn_bdd_grad_weight; float64 [num_rels, nb*P*Q]."""
    e = src.numel()
    xs = x.double()[src.long()].reshape(e, nb, p)
    gd = g.double()[dst.long()].reshape(e, nb, q)
    c = torch.ones(e, dtype=torch.float64) if coef is None else coef.double().reshape(-1)
    t = torch.einsum('ebp,ebq->ebpq', xs * c.view(-1, 1, 1), gd).reshape(e, -1)
    ta = torch.einsum('ebp,ebq->ebpq', (xs * c.view(-1, 1, 1)).abs(), gd.abs()).reshape(e, -1)
    et = etypes.long()
    want = torch.zeros(num_rels, nb * p * q, dtype=torch.float64).index_add_(0, et, t)
    sabs = torch.zeros(num_rels, nb * p * q, dtype=torch.float64).index_add_(0, et, ta)
    deg = torch.bincount(et, minlength=num_rels)
    n = deg + chunks_of(deg, chunk) + 3
    bnd = n.double().view(-1, 1) * U * sabs
    if old is not None:
        want = want + old.double()
        bnd = bnd + U * old.double().abs()
    return want, bnd + TINY, deg


def max_ratio(got, want, bnd):
    """Worst |got - want| / bound (inf where got is not finite but want is); <= 1: every element inside its bound."""
    got = got.detach().to('cpu', torch.float64)
    err = (got - want).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err)
    return float((err / bnd).max()) if err.numel() else 0.0


def row_gap(want_a, want_b, bnd, rows):
    """Negative control: the smallest, over ``rows``, of the row's largest |want_a - want_b| / bound (> 1: a kernel that
    computed want_b instead of want_a would leave the bound in every one of these rows)."""
    worst = float('inf')
    for i in rows:
        worst = min(worst, float(((want_a[i] - want_b[i]).abs() / bnd[i]).max()))
    return worst
