"""The dense product family (csrc/k_gemm.hip: gv_gemm_f32, gv_gemm_f32_live_rows, gv_gemm_f32_sparse, gv_gemm_bf16 -- all through
gemm_any(), i.e. ops.gemm) and the R-GCN output side (gv_rgcn_epilogue_fwd / _bwd, gv_colsum) against a float64 reference of the
same operation, element by element, inside the rigorous bound of oracle/gemm.py:

    |got - ref| <= (k + 2) u (|op(A')| @ |op(B)|)_ij + 2 u |bias_j| + u |c_old_ij| + TINY,      u = 2**-24

Exact zeros are asserted exactly: masked-out terms, skipped tiles, padding rows under ops.live_rows, columns outside the window
of a strided ``out``.  The host-only tests (no GPU) show that the bound would catch a dropped k-step at every shape used, and
that each shape reaches the tile configuration it claims to cover.

Tile configurations (gemm_any): 64 x 64 blocks (MT = 1) unless 128-row blocks still give >= 1024 blocks (MT = 2); BK = 16 for
a row-major A, 32 for A stored [K, M]; GV_GEMM_NT / GV_GEMM_BK / GV_GEMM_MT are read once per process, so the knob-only
configurations run in child processes (tests/workers/gemm_knob_worker.py).

Set GV_GEMM_RATIOS=<file> to have the worst |got - ref| / bound per kernel written there as JSON."""
import json
import os
import subprocess
import sys

import pytest
import torch

from oracle import gemm as og

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
# (bias, act, accumulate): none, each alone, all three together
EPILOGUES = [(False, 0, False), (True, 0, False), (False, 1, False), (False, 0, True), (True, 1, True)]
SPLITS = (1, 2, 7, 64)          # 7 and 64 are rounded down by k_chunk_for wherever k / split < 32
# ragged shapes (MT = 1 at every split); the MT = 2 shapes: 33 x 33 = 1089 blocks of 128 x 64, m % 128 = 4 -- the second
# 64-row half of the last block row lies outside m; and a weight-gradient product (A stored [K, M]) over K = 8192
SMALL = [(37, 19, 53), (5, 3, 2), (68, 132, 100), (260, 500, 1000), (200, 400, 3000), (64, 64, 40), (4, 4, 4)]
BIG = [(4100, 2050, 72, LAYOUTS, (1, 2, 7)), (1000, 1000, 8192, [(True, False), (True, True)], (8, 64))]


# ---- mirror of gemm_any's tile choice ----------------------------------------------------------------------------------------
def k_chunk_for(k, split):
    per = -(-k // split)
    return -(-per // 32) * 32


def effective_split(k, split):
    return 1 if (k == 0 or split <= 1) else -(-k // k_chunk_for(k, split))


def picked_mt(m, n, k, split, nt=1):
    blocks128 = -(-n // (64 * nt)) * -(-m // 128) * effective_split(k, split)
    return 2 if blocks128 >= 1024 else 1


def operands(m, n, k, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(m, k, generator=gen), torch.randn(k, n, generator=gen), torch.randn(n, generator=gen),
            torch.randn(m, n, generator=gen))


def stored(t, trans):
    """op(X) as the kernel stores X: transposed layouts hold X^T row-major."""
    return t.t().contiguous() if trans else t.contiguous()


RATIOS = {}


def check(key, got, want, bnd):
    r = og.max_ratio(got, want, bnd)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    assert r <= 1.0, f'{key}: |got - ref| / bound = {r:.3g}'
    return r


@pytest.fixture(scope='module', autouse=True)
def _report_ratios():
    yield
    path = os.environ.get('GV_GEMM_RATIOS')
    if path and RATIOS:
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        for k, v in RATIOS.items():
            old[k] = max(old.get(k, 0.0), v)
        with open(path, 'w') as f:
            json.dump(old, f, indent=1, sort_keys=True)


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


def run_grid(ops, m, n, k, layouts, splits, seed, key, precision='f32', epilogues=EPILOGUES, mask=None):
    """Every layout x epilogue x split of one shape against one float64 reference; returns the number of products checked."""
    a, b, bias, c0 = operands(m, n, k, seed)
    bf16 = precision == 'bf16'
    s, sabs = og.products(a, b, mask=mask, bf16=bf16)
    dev = {'bias': bias.cuda()}
    count = 0
    for ta, tb in layouts:
        a_d, b_d = stored(a, ta).cuda(), stored(b, tb).cuda()
        m_d = stored(mask, ta).cuda() if mask is not None else None
        for split in splits:
            for use_bias, act, acc in epilogues:
                want, bnd = og.epilogue(s, sabs, k, bias if use_bias else None, act, c0 if acc else None)
                out = c0.cuda() if acc else None
                got = ops.gemm(a_d, b_d, trans_a=ta, trans_b=tb, bias=dev['bias'] if use_bias else None, act=act, out=out,
                               accumulate=acc, split_k=split, a_relu_mask=m_d, precision=precision)
                check(key, got, want, bnd)
                count += 1
    return count


# ---- host-only: the tolerance catches a dropped k-step, the shapes reach their paths ------------------------------------
def _sample_elements(m, n, count=24, seed=0):
    gen = torch.Generator().manual_seed(seed)
    rows = [0, m - 1, m - 1, 0] + torch.randint(0, m, (count,), generator=gen).tolist()
    cols = [0, n - 1, 0, n - 1] + torch.randint(0, n, (count,), generator=gen).tolist()
    return rows, cols


@pytest.mark.parametrize('shape', [s[:3] for s in BIG] + SMALL, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_bound_catches_a_dropped_term(shape, bf16):
    """Negative control: at the corners and at random elements of every shape, removing the largest single term a_ik b_kj from
    the reference leaves it outside the bound -- a kernel that dropped one k-step there would fail."""
    m, n, k = shape
    a, b, _, _ = operands(m, n, k, seed=m + n + k)
    _, sabs = og.products(a, b, bf16=bf16)
    _, bnd = og.epilogue(sabs, sabs, k)
    rows, cols = _sample_elements(m, n)
    assert og.dropped_term_violates(a, b, bnd, rows, cols, bf16=bf16) > 1.0


def test_bound_catches_a_dropped_term_under_a_relu_mask():
    m, n, k = 68, 132, 100
    a, b, _, _ = operands(m, n, k, seed=1)
    mask = _relu_mask(m, k, seed=1)
    _, sabs = og.products(a, b, mask=mask)
    _, bnd = og.epilogue(sabs, sabs, k)
    rows, cols = _sample_elements(m, n)
    assert og.dropped_term_violates(a, b, bnd, rows, cols, mask=mask) > 1.0


def test_shapes_reach_the_tile_configurations_they_claim():
    """The tile choice of gemm_any, restated: a shape that no longer reaches the path its test covers fails here."""
    for m, n, k in SMALL:
        for split in SPLITS:
            assert picked_mt(m, n, k, split) == 1, (m, n, k, split)
    for m, n, k, _, splits in BIG:
        for split in splits:
            assert picked_mt(m, n, k, split) == 2, (m, n, k, split)
    # the requests that k_chunk_for rounds down (chunks are whole multiples of 32)
    assert effective_split(53, 7) == 2 and effective_split(1000, 64) == 32 and effective_split(72, 7) == 3
    assert effective_split(8192, 8) == 8 and effective_split(8192, 64) == 64
    assert picked_mt(1000, 1000, 8192, 1) == 1 and picked_mt(4100, 2050, 72, 1, nt=2) == 1


# ---- the product grid ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_gemm_small_shapes_all_layouts_epilogues_splits(ops, shape, precision):
    m, n, k = shape
    run_grid(ops, m, n, k, LAYOUTS, SPLITS, m + n + k, f'gv_gemm_{precision} MT=1', precision)


@gpu
@pytest.mark.parametrize('big', BIG, ids=lambda s: 'x'.join(map(str, s[:3])))
def test_gemm_mt2_shapes_all_layouts_epilogues_splits(ops, big):
    m, n, k, layouts, splits = big
    for split in splits:
        assert picked_mt(m, n, k, split) == 2
    run_grid(ops, m, n, k, layouts, splits, m + n + k, 'gv_gemm_f32 MT=2')


@gpu
def test_gemm_bf16_mt2_sized_shape(ops):
    """gv_gemm_bf16 has one tile shape (64 x 64 x 32); the big shape still covers its ragged last block row / column."""
    run_grid(ops, 4100, 2050, 72, LAYOUTS, (1, 7), 7, 'gv_gemm_bf16 big', 'bf16', epilogues=[EPILOGUES[0], EPILOGUES[-1]])


@gpu
def test_gemm_bf16_really_rounds_its_operands(ops):
    """The bf16 result lies inside the bound of the ROUNDED operands and far outside the fp32 bound of the unrounded ones."""
    m, n, k = 260, 500, 1000
    a, b, _, _ = operands(m, n, k, 3)
    got = ops.gemm(a.cuda(), b.cuda(), precision='bf16')
    want, bnd = og.epilogue(*og.products(a, b, bf16=True), k)
    check('gv_gemm_bf16 MT=1', got, want, bnd)
    want32, bnd32 = og.epilogue(*og.products(a, b), k)
    outside = ((got.cpu().double() - want32).abs() > bnd32).double().mean()
    assert float(outside) > 0.4          # ~60 % of the elements at this shape
    with ops.gemm_precision('bf16'):          # the global switch takes the same entry
        assert torch.equal(ops.gemm(a.cuda(), b.cuda()), got)


# ---- a_relu_mask ---------------------------------------------------------------------------------------------------------
def _relu_mask(m, k, seed):
    """Positive, negative, -0.0, +0.0 and NaN mask values."""
    gen = torch.Generator().manual_seed(seed + 1000)
    mask = torch.randn(m, k, generator=gen)
    pick = torch.randint(0, 8, (m, k), generator=gen)
    mask[pick == 0] = -0.0
    mask[pick == 1] = 0.0
    mask[pick == 2] = float('nan')
    return mask


def _poison_masked_out(a, mask, seed):
    """NaN / +inf / -inf in A wherever the mask drops the entry: each must contribute an exact 0."""
    gen = torch.Generator().manual_seed(seed + 2000)
    a = a.clone()
    dead = ~(mask > 0)
    pick = torch.randint(0, 4, a.shape, generator=gen)
    a[dead & (pick == 0)] = float('nan')
    a[dead & (pick == 1)] = float('inf')
    a[dead & (pick == 2)] = float('-inf')
    return a


@gpu
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
@pytest.mark.parametrize('shape', [(37, 19, 53), (68, 132, 100), (260, 500, 1000), (4100, 2050, 72)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_gemm_a_relu_mask(ops, precision, shape):
    """A is read as (mask > 0 ? A : 0): a NaN mask value is not > 0, so it drops its entry like -0.0, +0.0 and negative values do;
    NaN and +-inf in A under those entries never reach the sum."""
    m, n, k = shape
    a, b, bias, c0 = operands(m, n, k, 11)
    mask = _relu_mask(m, k, 11)
    a = _poison_masked_out(a, mask, 11)
    s, sabs = og.products(a, b, mask=mask, bf16=precision == 'bf16')
    assert torch.isfinite(s).all()
    key = f'gv_gemm_{precision} a_relu_mask'
    splits = (1, 3) if m < 1000 else (1,)
    for ta, tb in LAYOUTS:
        a_d, b_d, m_d = stored(a, ta).cuda(), stored(b, tb).cuda(), stored(mask, ta).cuda()
        for split in splits:
            for use_bias, act, acc in (EPILOGUES[0], EPILOGUES[-1]):
                want, bnd = og.epilogue(s, sabs, k, bias if use_bias else None, act, c0 if acc else None)
                got = ops.gemm(a_d, b_d, trans_a=ta, trans_b=tb, bias=bias.cuda() if use_bias else None, act=act,
                               out=c0.cuda() if acc else None, accumulate=acc, split_k=split, a_relu_mask=m_d, precision=precision)
                check(key, got, want, bnd)
    # a row of A whose mask is nowhere positive contributes nothing at all: that row of the product is an exact 0
    mask2 = mask.clone()
    mask2[m // 2] = -0.0
    mask2[m - 1] = float('nan')
    got = ops.gemm(a.cuda(), b.cuda(), a_relu_mask=mask2.cuda(), precision=precision).cpu()
    assert torch.equal(got[[m // 2, m - 1]], torch.zeros(2, n))


# ---- operand and output geometry -------------------------------------------------------------------------------------------
SENTINEL = 1234.5


def _embed(t, offset_rows, offset_cols, ld, fill=None, gen=None):
    """t as a (rows, cols) window of a larger row-major tensor of leading dimension ld (returns window, host copy of the whole)."""
    rows, cols = t.shape
    big = (torch.full((rows + offset_rows + 2, ld), fill) if fill is not None
           else torch.randn(rows + offset_rows + 2, ld, generator=gen))
    big[offset_rows:offset_rows + rows, offset_cols:offset_cols + cols] = t
    big = big.cuda()
    return big[offset_rows:offset_rows + rows, offset_cols:offset_cols + cols], big


def _ld(cols):
    return -(-(cols + 1) // 4) * 4 + 4          # a multiple of 4, > cols + 1: room for a 1-float offset


@gpu
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
@pytest.mark.parametrize('placement', ['row_slice_ld', 'offset_1_float'])
@pytest.mark.parametrize('shape', [(37, 19, 53), (68, 132, 100), (130, 70, 45)], ids=lambda s: 'x'.join(map(str, s)))
def test_gemm_sliced_operands_and_strided_out(ops, precision, shape, placement):
    """Operands that are windows of larger tensors (ld > width; with a 1-float offset the rows are not 16-B aligned although
    ld % 4 == 0, so the vector loads are off) and ``out`` as a column window of a sentinel-filled tensor (ldc > n): the result
    matches the reference and every sentinel outside the m x n window is unchanged, on the direct and the split-K paths."""
    m, n, k = shape
    a, b, bias, c0 = operands(m, n, k, 21)
    mask = _relu_mask(m, k, 21)
    gen = torch.Generator().manual_seed(5)
    col_off = 1 if placement == 'offset_1_float' else 0
    key = f'gv_gemm_{precision} strided'
    for ta, tb in LAYOUTS:
        sa, sb, sm = stored(a, ta), stored(b, tb), stored(mask, ta)
        a_d, _ = _embed(sa, 3, col_off, _ld(sa.shape[1]), gen=gen)
        m_d, _ = _embed(sm, 3, col_off, _ld(sa.shape[1]), gen=gen)
        b_d, _ = _embed(sb, 2, col_off, _ld(sb.shape[1]), gen=gen)
        assert a_d.stride(0) % 4 == 0 and (a_d.data_ptr() % 16 != 0) == (col_off == 1)
        for split in (1, 3):
            for use_mask in (False, True):
                for use_bias, act, acc in (EPILOGUES[0], EPILOGUES[-1]):
                    s, sabs = og.products(a, b, mask=mask if use_mask else None, bf16=precision == 'bf16')
                    want, bnd = og.epilogue(s, sabs, k, bias if use_bias else None, act, c0 if acc else None)
                    out, big = _embed(c0 if acc else torch.full((m, n), SENTINEL), 1, 2, n + 7, fill=SENTINEL)
                    ops.gemm(a_d, b_d, trans_a=ta, trans_b=tb, bias=bias.cuda() if use_bias else None, act=act, out=out,
                             accumulate=acc, split_k=split, a_relu_mask=m_d if use_mask else None, precision=precision)
                    check(key, out, want, bnd)
                    big = big.cpu()
                    big[1:1 + m, 2:2 + n] = SENTINEL
                    assert torch.equal(big, torch.full_like(big, SENTINEL)), 'a write outside the m x n window of out'


@gpu
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_gemm_empty_reduction_and_empty_output(ops, precision):
    """k == 0: out = act(bias) (+ the old values); m == 0 or n == 0: nothing is launched and out is untouched."""
    m, n = 70, 130
    _, _, bias, c0 = operands(m, n, 1, 31)
    bias[::3] = -bias[::3].abs()
    for ta, tb in LAYOUTS:
        a = torch.empty((0, m) if ta else (m, 0)).cuda()
        b = torch.empty((n, 0) if tb else (0, n)).cuda()
        for split in (1, 4):
            got = ops.gemm(a, b, trans_a=ta, trans_b=tb, bias=bias.cuda(), act=ops.ACT_RELU, split_k=split, precision=precision)
            assert torch.equal(got.cpu(), torch.relu(bias).expand(m, n))
            out = c0.cuda()
            ops.gemm(a, b, trans_a=ta, trans_b=tb, bias=bias.cuda(), out=out, accumulate=True, split_k=split, precision=precision)
            assert torch.equal(out.cpu(), c0 + bias)
            assert torch.equal(ops.gemm(a, b, trans_a=ta, trans_b=tb, split_k=split, precision=precision).cpu(), torch.zeros(m, n))
    big = torch.full((9, 9), SENTINEL).cuda()
    for mm, nn, kk in ((0, 5, 7), (5, 0, 7), (0, 0, 3)):
        a, b = torch.randn(mm, kk).cuda(), torch.randn(kk, nn).cuda()
        for split in (1, 3):
            out = big[:mm, :nn]
            got = ops.gemm(a, b, out=out, accumulate=True, split_k=split, precision=precision)
            assert tuple(got.shape) == (mm, nn)
            assert tuple(ops.gemm(a, b, split_k=split, precision=precision).shape) == (mm, nn)
    torch.cuda.synchronize()
    assert torch.equal(big.cpu(), torch.full((9, 9), SENTINEL))


@gpu
def test_gemm_refuses_a_bad_out_before_launching(ops):
    """ops.gemm writes ``out`` through its pointer and row stride only: a wrong shape, type, device or layout is refused."""
    a, b = torch.randn(40, 30).cuda(), torch.randn(30, 20).cuda()
    sentinel = torch.full((64, 64), SENTINEL).cuda()
    bad = [
        (ValueError, sentinel[:40, :21]),                  # one column too many
        (ValueError, sentinel[:41, :20]),                  # one row too many
        (ValueError, sentinel[:20, :40].t()),              # right shape, inner stride 64
        (ValueError, sentinel[:40, :40][:, ::2]),          # right shape, inner stride 2
        (TypeError, sentinel.view(-1)[:800]),              # 1-D
        (TypeError, sentinel[:40, :20].double()),
        (TypeError, sentinel[:40, :20].to(torch.bfloat16)),
        (TypeError, [[0.0] * 20] * 40),
        (ValueError, torch.zeros(40, 20)),                 # host memory
    ]
    for exc, out in bad:
        for split in (1, 3):
            for precision in ('f32', 'bf16'):
                with pytest.raises(exc):
                    ops.gemm(a, b, out=out, split_k=split, precision=precision)
    with pytest.raises(ValueError):
        ops.gemm(a, b, bias=sentinel[0, :21].contiguous())
    with pytest.raises(RuntimeError):
        ops.gemm(a, b, bias=torch.zeros(20))             # host memory
    torch.cuda.synchronize()
    assert torch.equal(sentinel.cpu(), torch.full((64, 64), SENTINEL))
    ok = sentinel[:40, 3:23]          # a strided window of the right shape is accepted
    ops.gemm(a, b, out=ok)
    want, bnd = og.epilogue(*og.products(a.cpu(), b.cpu()), 30)
    check('gv_gemm_f32 MT=1', ok, want, bnd)


# ---- c_tiles and live_rows at a 128-row-block shape -------------------------------------------------------------------------
def _tile_mask(m, n):
    """Block-triangular: tile (i, j) wanted iff j <= (i + 1) // 2.  Tile rows 2I and 2I + 1 (one 128-row block) differ in column
    I + 1, so some blocks hold a wanted and an unwanted 64 x 64 tile."""
    ti = torch.arange(m) // 64
    tj = torch.arange(n) // 64
    return (tj[None, :] <= (ti[:, None] + 1) // 2).float()


@gpu
@pytest.mark.parametrize('split', [1, 3])
def test_gemm_c_tiles_at_a_128_row_block_shape(ops, split):
    """gv_gemm_f32_sparse with tile words: the wanted tiles match the reference, every unwanted 64 x 64 tile is stored as exact
    zeros (the old values when accumulating) -- also inside a 128-row block that holds a wanted tile -- and the window's
    sentinels are kept.  Split-K with the wanted-tile count walks MT = 1 blocks of the wanted tiles only, without it the MT = 2
    grid of the dense product."""
    m, n, k = 4100, 2050, 72
    assert picked_mt(m, n, k, split) == 2
    a, b, _, c0 = operands(m, n, k, 41)
    tiles = _tile_mask(m, n)
    words = ops.block_words(tiles.cuda(), 'tiles')
    assert words._gv_wanted > 0
    unwanted = tiles == 0
    s, sabs = og.products(a, b)
    a_d, b_d = stored(a, True).cuda(), b.cuda()           # a weight gradient: A stored [K, M]
    variants = [('counted', words)] + ([('uncounted', words.clone())] if split > 1 else [])
    for name, w in variants:
        for acc in (False, True):
            want, bnd = og.epilogue(s, sabs, k, c_old=c0 if acc else None)
            out, big = _embed(c0 if acc else torch.full((m, n), SENTINEL), 1, 2, n + 6, fill=SENTINEL)
            ops.gemm(a_d, b_d, trans_a=True, out=out, accumulate=acc, split_k=split, c_tiles=w)
            got = out.cpu()
            assert torch.equal(got[unwanted], c0[unwanted] if acc else torch.zeros(int(unwanted.sum()))), \
                f'{name}: an unwanted tile holds something else than {"its old values" if acc else "zeros"}'
            keep = ~unwanted
            check('gv_gemm_f32_sparse c_tiles', got[keep].view(1, -1), want[keep].view(1, -1), bnd[keep].view(1, -1))
            big = big.cpu()
            big[1:1 + m, 2:2 + n] = SENTINEL
            assert torch.equal(big, torch.full_like(big, SENTINEL))


@gpu
@pytest.mark.parametrize('live', [3000, 3008])
@pytest.mark.parametrize('split', [1, 3])
def test_gemm_live_rows_row_major_a_at_a_128_row_block_shape(ops, live, split):
    """ops.live_rows with a row-major A of ``cap`` rows (gv_gemm_f32_live_rows): rows below the device count match the reference
    although the padding rows of A hold NaN-free garbage; without split-K the 128-row blocks that start at or past the count store
    zeros (keep the old values when accumulating) -- live = 3008 lies on the 64-row boundary inside block 23, so rows 3008..3071
    are computed under MT = 2 and zeroed under MT = 1: the test sees which tiles ran."""
    m, n, k = 4100, 2050, 72
    assert picked_mt(m, n, k, split) == 2
    a, b, bias, c0 = operands(m, n, k, 51)
    a[live:] *= 1e3                                       # padding rows: finite, far from the live ones
    s, sabs = og.products(a, b)
    rows_dev = torch.tensor([live], dtype=torch.int32, device='cuda')
    bm = 128
    skipped_from = -(-live // bm) * bm if split == 1 else m
    for tb in (False, True):
        a_d, b_d = a.cuda(), stored(b, tb).cuda()
        for use_bias, act, acc in (EPILOGUES[0], EPILOGUES[-1]):
            want, bnd = og.epilogue(s, sabs, k, bias if use_bias else None, act, c0 if acc else None)
            out, big = _embed(c0 if acc else torch.full((m, n), SENTINEL), 1, 2, n + 6, fill=SENTINEL)
            with ops.live_rows(rows_dev, m):
                ops.gemm(a_d, b_d, trans_b=tb, bias=bias.cuda() if use_bias else None, act=act, out=out, accumulate=acc,
                         split_k=split)
            got = out.cpu()
            check('gv_gemm_f32_live_rows', got[:skipped_from], want[:skipped_from], bnd[:skipped_from])
            assert torch.equal(got[skipped_from:], c0[skipped_from:] if acc else torch.zeros(m - skipped_from, n))
            big = big.cpu()
            big[1:1 + m, 2:2 + n] = SENTINEL
            assert torch.equal(big, torch.full_like(big, SENTINEL))


@gpu
@pytest.mark.parametrize('live', [5000, 5120])
@pytest.mark.parametrize('split', [1, 8])
def test_gemm_live_rows_weight_gradient_at_a_128_row_block_shape(ops, live, split):
    """ops.live_rows with A stored [K, M] (a weight gradient over ``cap`` node rows): the reduction ends at the device count --
    NaN in the padding rows of both operands never reaches the result.  5120 is the end of a split-K chunk, 5000 lies inside one."""
    m, n, k = 1000, 1000, 8192
    a, b, bias, c0 = operands(m, n, k, 61)
    s, sabs = og.products(a[:, :live], b[:live])
    a[:, live:] = float('nan')
    b[live:] = float('nan')
    rows_dev = torch.tensor([live], dtype=torch.int32, device='cuda')
    a_d = stored(a, True).cuda()
    for tb in (False, True):
        b_d = stored(b, tb).cuda()
        for use_bias, act, acc in (EPILOGUES[0], EPILOGUES[-1]):
            want, bnd = og.epilogue(s, sabs, live, bias if use_bias else None, act, c0 if acc else None)
            with ops.live_rows(rows_dev, k):
                got = ops.gemm(a_d, b_d, trans_a=True, trans_b=tb, bias=bias.cuda() if use_bias else None, act=act,
                               out=c0.cuda() if acc else None, accumulate=acc, split_k=split)
            check('gv_gemm_f32_live_rows', got, want, bnd)


# ---- knob-only tile shapes, one child process per setting -----------------------------------------------------------------
KNOBS = [{'GV_GEMM_NT': '2'}, {'GV_GEMM_BK': '32'}, {'GV_GEMM_BK': '16'}, {'GV_GEMM_MT': '2', 'GV_GEMM_NT': '2'}]


@gpu
def test_gemm_knob_only_tile_shapes_in_child_processes():
    """GV_GEMM_NT=2 (128-column blocks), GV_GEMM_BK forced to the other depth of each layout (32 for a row-major A, 16 for A
    stored [K, M]) and MT = NT = 2 at the small shapes: the settings are read once per process, so each runs in a child of its
    own (tests/workers/gemm_knob_worker.py), one at a time; the first failing child stops the test."""
    worker = os.path.join(ROOT, 'tests', 'workers', 'gemm_knob_worker.py')
    for knob in KNOBS:
        env = dict(os.environ, **knob)
        for name in ('GV_GEMM_NT', 'GV_GEMM_BK', 'GV_GEMM_MT'):
            if name not in knob:
                env.pop(name, None)
        out = subprocess.run([sys.executable, worker], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, f'{knob}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-3000:]}'
        assert 'products checked' in out.stdout, out.stdout[-2000:]
        line = [l for l in out.stdout.splitlines() if l.startswith('{')][-1]
        for key, r in json.loads(line).items():
            RATIOS[f'{key} {knob}'] = r


# ---- column sums and the R-GCN epilogue -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('m', [0, 1, 63, 64, 65, 100003])
def test_colsum(ops, m):
    """gv_colsum over 64 row slices: m < 64 leaves slices empty.  With and without relu_mask (the entry counts where mask > 0:
    NaN, -0.0 and +0.0 drop it) and accumulate, contiguous and with a leading dimension > n."""
    gen = torch.Generator().manual_seed(m)
    for n in (1, 63, 64, 200, 1100):
        if m == 100003 and n == 1100:
            continue                           # 110 M floats: the large-n case runs at m = 65
        clean = torch.randn(m, n, generator=gen)
        mask = _relu_mask(m, n, m + n)
        poisoned = _poison_masked_out(clean, mask, n)       # summed under the mask only
        old = torch.randn(n, generator=gen)
        for strided in (False, True):
            place = (lambda t: _embed(t, 1, 3, n + 5, gen=gen)[0]) if strided else (lambda t: t.cuda())
            m_d = place(mask)
            for use_mask in (False, True):
                x_d = place(poisoned if use_mask else clean)
                x64 = (og.masked(poisoned, mask) if use_mask else clean).double()
                for acc in (False, True):
                    want = x64.sum(0) + (old.double() if acc else 0)
                    bnd = (m + 2) * og.U * x64.abs().sum(0) + (og.U * old.double().abs() if acc else 0) + og.TINY
                    got = ops.colsum(x_d, out=old.cuda() if acc else None, accumulate=acc, relu_mask=m_d if use_mask else None)
                    check('gv_colsum', got.view(1, -1), want.view(1, -1), bnd.view(1, -1))


@gpu
@pytest.mark.parametrize('m', [0, 1, 3001])
@pytest.mark.parametrize('n', [200, 1024, 38, 1100])
def test_rgcn_epilogue_fwd_bwd(ops, m, n):
    """gv_rgcn_epilogue_fwd / _bwd against the float64 formula, with and without addend, ReLU and a keep mask (scale 1.25); the
    bias gradient from the fused column sums (n % 4 == 0, n <= 1024: 200, 1024) and from the fallback gv_colsum (38, 1100)."""
    gen = torch.Generator().manual_seed(m * 7 + n)
    agg, addend, gout = (torch.randn(m, n, generator=gen) for _ in range(3))
    agg[:, ::5] = -addend[:, ::5]                          # exact zeros before the ReLU
    keep = (torch.rand(m, n, generator=gen) > 0.3).to(torch.uint8)
    old = torch.randn(n, generator=gen)
    scale = 1.25
    u = og.U * (1 + 2 ** -20)                             # one rounding per operation (+ second-order terms)
    for use_add in (False, True):
        for act in (ops.ACT_NONE, ops.ACT_RELU):
            for use_keep in (False, True):
                sc = scale if use_keep else 1.0
                v = agg.double() + (addend.double() if use_add else 0)
                vb = u * (agg.double().abs() + (addend.double().abs() if use_add else 0))
                if act:
                    v = torch.relu(v)
                if use_keep:
                    v = torch.where(keep.bool(), v * sc, torch.zeros((), dtype=torch.float64))
                    vb = torch.where(keep.bool(), vb * sc + u * v.abs(), torch.zeros((), dtype=torch.float64))
                out = ops.epilogue_fwd(agg.cuda(), addend.cuda() if use_add else None, act, keep.cuda() if use_keep else None, sc)
                check('gv_rgcn_epilogue_fwd', out, v, vb + og.TINY)
                fout = out.cpu()
                if use_keep:
                    assert torch.equal(fout[keep == 0], torch.zeros(int((keep == 0).sum())))
                g_ref = gout.double() * sc
                if use_keep:
                    g_ref = torch.where(keep.bool(), g_ref, torch.zeros((), dtype=torch.float64))
                if act:
                    g_ref = torch.where(fout > 0, g_ref, torch.zeros((), dtype=torch.float64))
                g_bnd = u * g_ref.abs() + og.TINY
                dead = g_ref == 0
                for acc in (False, True):
                    cs = old.cuda() if acc else torch.full((n,), SENTINEL).cuda()
                    g = ops.epilogue_bwd(out, gout.cuda(), act, keep.cuda() if use_keep else None, sc, colsum_out=cs,
                                         colsum_accumulate=acc)
                    check('gv_rgcn_epilogue_bwd', g, g_ref, g_bnd)
                    assert torch.equal(g.cpu()[dead], torch.zeros(int(dead.sum())))
                    want = g_ref.sum(0) + (old.double() if acc else 0)
                    bnd = (m + 3) * u * g_ref.abs().sum(0) + (u * old.double().abs() if acc else 0) + og.TINY
                    fused = n % 4 == 0 and n <= 1024
                    check(f'epilogue_bwd colsum ({"fused" if fused else "gv_colsum"})', cs.view(1, -1), want.view(1, -1),
                          bnd.view(1, -1))
                    g2 = ops.epilogue_bwd(out, gout.cuda(), act, keep.cuda() if use_keep else None, sc)
                    assert torch.equal(g2, g)
