"""TEST INFRASTRUCTURE ONLY -- float64 reference of the dense product family (include/gcnvae.h: gv_gemm_f32, gv_gemm_f32_live_rows,
gv_gemm_f32_sparse, gv_gemm_bf16) with an element-wise error bound:

    out = act(op(A') @ op(B) + bias) (+ c_old)        A' = (mask > 0 ? A : 0), applied before any rounding

    |got - ref|_ij <= (k + 2) u (|op(A')| @ |op(B)|)_ij + 2 u |bias_j| + u |c_old_ij| + TINY,        u = 2**-24

The product is a fp32 fma chain (or, split-K, a few of them summed in fp32): k + 2 roundings of at most u relative to
sum_k |a_ik b_kj| each, one for the bias add, one for the accumulate.  ReLU is 1-Lipschitz, so the bound holds after it.
bf16 operands: the bound is taken on the ROUNDED operands (round to nearest even, oracle/bf16.py), whose products are
exact in fp32.  A NaN mask value is not positive: the entry is dropped, as is any NaN or inf in A under it.
"""
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126


def round_bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def masked(a, mask):
    """A as the kernels read it under a ReLU mask: an entry survives only where the mask is > 0 (NaN, -0.0, +0.0 drop it)."""
    return a if mask is None else torch.where(mask > 0, a, torch.zeros((), dtype=a.dtype))


def products(a, b, mask=None, bf16=False):
    """(op(A') @ op(B), |op(A')| @ |op(B)|) in float64 from the fp32 operands the kernel consumes; a is op(A) (m, k), b is op(B) (k, n)."""
    a = masked(a.float(), mask)
    b = b.float()
    if bf16:
        a, b = round_bf16(a), round_bf16(b)
    a64, b64 = a.double(), b.double()
    return a64 @ b64, a64.abs() @ b64.abs()


def epilogue(s, sabs, k, bias=None, act=0, c_old=None):
    """The expected value and the element-wise bound of act(s + bias) (+ c_old), from products()."""
    want, bnd = s, (k + 2) * U * sabs
    if bias is not None:
        bias64 = bias.double().view(1, -1)
        want = want + bias64
        bnd = bnd + 2 * U * bias64.abs()
    if act:
        want = torch.relu(want)
    if c_old is not None:
        old = c_old.double()
        want = old + want
        bnd = bnd + U * old.abs()
    return want, bnd + TINY


def max_ratio(got, want, bnd):
    """Worst |got - want| / bound (inf where got is not finite but want is); <= 1 means every element is inside its bound."""
    got = got.detach().to('cpu', torch.float64)
    err = (got - want).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err)
    return float((err / bnd).max()) if err.numel() else 0.0


def dropped_term_violates(a, b, bnd, rows, cols, mask=None, bf16=False):
    """Negative control: for each (i, j), the reference with its largest single term a_ik b_kj removed lies outside the bound
    (so the tolerance would catch a dropped k-step there).  Returns the smallest term / bound ratio over the elements."""
    a = masked(a.float(), mask)
    b = b.float()
    if bf16:
        a, b = round_bf16(a), round_bf16(b)
    worst = float('inf')
    for i, j in zip(rows, cols):
        terms = (a[i].double() * b[:, j].double()).abs()
        worst = min(worst, float(terms.max()) / float(bnd[i, j]))
    return worst
