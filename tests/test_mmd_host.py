"""The MMD and prior-sampler tests' own footing (no GPU): the hand references of mmd_cases are the float64 oracle's; a float32
restatement of the kernels stays under HALF the bound of test_gpu_mmd.py at every shape it uses, so the inputs leave room for a
correct kernel; every rule that is wrong in one detail exceeds the bound wherever it can differ at all (the pairs where it
cannot are listed, and shown to be the same numbers); an all-zero gradient -- what the checks of tests/test_gpu_ops.py accept at
the widths the project ships -- exceeds it on at least 99 % of the elements; and the shape list reaches all seven kernel
instantiations by gv_mmd_fwd's / gv_mmd_bwd's own dispatch rule."""
import pytest
import torch

import mmd_cases as mc
from oracle import kgvae as okg
from oracle import prob as oprob

FORM_CASES = [(sx, sy, h, s) for sx, sy, h in mc.FORM_SHAPES for s in mc.SCALES]
INDEX_CASES = [(sx, h, s) for sx, h in mc.INDEX_SHAPES for s in mc.SCALES]
GROUPS = {'fwd': ('partials',), 'bwd': ('gx', 'gy')}


def ident(c):
    return '-'.join(str(v) for v in c)


# ---- the shape list against the dispatch rule ---------------------------------------------------------------------------------
def test_shape_list_reaches_all_seven_instantiations():
    reached = {}
    for sx, sy, h in mc.FORM_SHAPES:
        for name in mc.dispatch(h):
            reached.setdefault(name, []).append((sx, sy, h))
    assert set(reached) == set(mc.INSTANCES), sorted(set(mc.INSTANCES) - set(reached))
    widths = {name: sorted({s[2] for s in shapes}) for name, shapes in reached.items()}
    assert widths == {'k_mmd_fwd_g<4>': [4, 200, 256], 'k_mmd_bwd_g<4>': [4, 200, 256], 'k_mmd_fwd_g<8>': [260, 512],
                      'k_mmd_fwd<4>': [6, 30], 'k_mmd_bwd<4>': [6, 30], 'k_mmd_fwd<16>': [258, 516, 1024],
                      'k_mmd_bwd<16>': [258, 260, 512, 516, 1024]}
    # the row counts that the loops' strides make interesting, on both sides and once swapped
    rows16 = {n for name in ('k_mmd_fwd_g<4>', 'k_mmd_fwd_g<8>') for s in reached[name] for n in s[:2]}
    lanes = {n for name in ('k_mmd_fwd<4>', 'k_mmd_fwd<16>') for s in reached[name] for n in s[:2]}
    assert rows16 >= {1, 63, 65, 129, 130} and lanes >= {1, 17, 33, 49, 65}
    assert (65, 129, 200) in mc.FORM_SHAPES and (129, 65, 200) in mc.FORM_SHAPES
    assert (17, 33, 30) in mc.FORM_SHAPES and (33, 17, 30) in mc.FORM_SHAPES
    assert all(sx != sy or (sx, sy) == (1, 1) for sx, sy, _ in mc.FORM_SHAPES) and max(max(s[:2]) for s in mc.FORM_SHAPES) <= 130
    # GV_MMD_ROWS16=0 and an unaligned base send the aligned widths to the lane-per-column forms
    for h in (4, 200, 256):
        assert mc.dispatch(h, rows16=False) == mc.dispatch(h, aligned=False) == ('k_mmd_fwd<4>', 'k_mmd_bwd<4>')
    for h in (260, 512):
        assert mc.dispatch(h, rows16=False) == ('k_mmd_fwd<16>', 'k_mmd_bwd<16>')
    assert [mc.dispatch(h) for _, h in mc.INDEX_SHAPES] == [('k_mmd_fwd_g<4>', 'k_mmd_bwd_g<4>'), ('k_mmd_fwd<16>', 'k_mmd_bwd<16>')]


def test_inputs_are_what_the_docstring_says():
    for sx, sy, h in mc.FORM_SHAPES:
        if sx == sy == 1:
            continue
        for scale in mc.SCALES:
            exx, eyy, exy = mc.case_references(sx, sy, h, scale)['exponents']
            off = torch.cat([exx[~torch.eye(sx, dtype=torch.bool)], eyy[~torch.eye(sy, dtype=torch.bool)], exy.reshape(-1)])
            if scale == 'n':
                # about 2 / h: the mean over the pairs is (2, 1.5 + 0.01 and 0.98 of 1 / h for xx, xy, yy)
                assert 0.9 / h < float(off.mean()) < 2.1 / h, (sx, sy, h, float(off.mean()))
            else:
                # spans roughly 0.2 to 1.6: narrower at large h, wider at h = 4 and 6, K far from 1 throughout
                assert float(off.min()) < 0.65 and float(off.max()) > 1.1, (sx, sy, h, float(off.min()), float(off.max()))
                assert 0.2 < float(torch.exp(-off).median()) < 0.7
    for sx, h in mc.INDEX_SHAPES:
        pick = mc.make_index_case(sx, h)[2]
        counts = torch.bincount(pick, minlength=mc.INDEX_ROWS)
        assert pick.numel() == mc.INDEX_PICKS and pick.dtype == torch.int64 and int(pick.max()) < mc.INDEX_ROWS - 1
        assert int(counts[5]) == 3 and int(counts[11]) == 2 and int(pick[0]) == 11 and int(pick[-1]) == 11
        assert int((counts == 2).sum()) == 30 and int((counts == 1).sum()) == 7 and int((counts == 0).sum()) == mc.INDEX_ROWS - 38
    for k, h, repeat in mc.SAMPLER_SHAPES:
        raw0 = mc.sampler_case(k, h, repeat)[0][k]
        assert raw0[:min(h, 6)].tolist() == [float(torch.tensor(v)) for v in mc.PLANT[:min(h, 6)]]
    assert set(mc.PLANT) == {-30.0, -5.0, 0.0, 19.99, 20.01, 50.0}


# ---- the hand references are the oracle's ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', FORM_CASES, ids=ident)
def test_float64_references_equal_the_oracle(case):
    """Value and both gradients against torch autograd in float64 on oracle.kgvae.rbf_kernel's three means, to 1e-12: of the value
    for the value, of sum_j |t_j| for a gradient element (the terms cancel; 1e-12 of the sum itself would ask more of float64 than
    it has)."""
    sx, sy, h, scale = case
    x, y = mc.make_case(sx, sy, h, scale)
    ref = mc.case_references(sx, sy, h, scale)
    xo, yo = x.double().requires_grad_(True), y.double().requires_grad_(True)
    mo = okg.rbf_kernel(xo, xo).mean() + okg.rbf_kernel(yo, yo).mean() - 2 * okg.rbf_kernel(xo, yo).mean()
    (mo * mc.grad_scale(*mc.GRAD_ARGS[scale])).backward()
    assert abs(float(ref['mmd'] - mo.detach())) <= 1e-12 * float(ref['partials'].abs().sum())
    for name, got in (('gx', xo.grad), ('gy', yo.grad)):
        assert ref[name].dtype == torch.float64
        assert bool(((ref[name] - got).abs() <= 1e-12 * ref[name + '_abs'] + 1e-300).all()), name
    assert float(ref['gx'].abs().max()) > 0 and float(ref['gy'].abs().max()) > 0


@pytest.mark.parametrize('case', INDEX_CASES, ids=ident)
def test_indexed_reference_equals_autograd_through_the_gather(case):
    sx, h, scale = case
    x, y, pick, prefill = mc.make_index_case(sx, h, scale)
    ref = mc.index_case_references(sx, h, scale)
    xo, yo = x.double().requires_grad_(True), y.double().requires_grad_(True)
    ys = yo[pick]
    mo = okg.rbf_kernel(xo, xo).mean() + okg.rbf_kernel(ys, ys).mean() - 2 * okg.rbf_kernel(xo, ys).mean()
    (mo * mc.grad_scale(0.37, 1.3)).backward()
    want = prefill.double() + yo.grad
    mass = prefill.double().abs().index_add_(0, pick, ref['dense']['gy_abs'])
    assert bool(((ref['gy'] - want).abs() <= 1e-12 * mass).all())
    assert bool(((ref['dense']['gx'] - xo.grad).abs() <= 1e-12 * ref['dense']['gx_abs']).all())
    assert torch.equal(ref['gy'][~ref['picked']], prefill.double()[~ref['picked']]) and int(ref['picked'].sum()) == 38


@pytest.mark.parametrize('shape', mc.SAMPLER_SHAPES, ids=ident)
def test_sampler_reference_equals_the_oracle(shape):
    k, h, repeat = shape
    z_pre, eps, g, _ = mc.sampler_case(k, h, repeat)
    ref = mc.sampler_reference(z_pre, eps, g)
    zo = z_pre.double().requires_grad_(True)
    if repeat > 1:
        m_mix, v_mix = oprob.gaussian_parameters(zo.unsqueeze(0), dim=1)
    else:
        m_mix, v_mix = oprob.gaussian_parameters(zo, dim=0)
    out = oprob.sample_gaussian(m_mix, v_mix, eps.double(), repeat=repeat)
    out.backward(g.double())
    assert out.shape == ref['out'].shape
    assert bool(((ref['out'] - out.detach()).abs() <= 1e-12 * (ref['out'].abs() + 1e-300)).all())
    assert bool(((ref['gz'] - zo.grad).abs() <= 1e-12 * ref['gz_abs'] + 1e-300).all())


# ---- room for a correct kernel ------------------------------------------------------------------------------------------------------
def ratios(got, ref):
    out = {name: mc.worst_ratio(got[name], ref[name], ref[name + '_bound']) for name in ('partials', 'gx', 'gy')}
    vref, vbound = mc.value_reference(got['partials'])
    out['mmd'] = mc.worst_ratio(got['mmd'], vref, vbound)
    return out


@pytest.mark.parametrize('case', FORM_CASES, ids=ident)
def test_restatement_leaves_half_the_bound(case):
    sx, sy, h, scale = case
    got = mc.restate(*mc.make_case(sx, sy, h, scale), None, None, *mc.GRAD_ARGS[scale])
    for what, r in ratios(got, mc.case_references(sx, sy, h, scale)).items():
        print(f'RATIO restatement {ident(case)} {what} {r:.3f}')
        assert r < 0.5, f'{what}: {r:.3f} of the bound'


def index_ratios(got, ref):
    out = ratios(dict(got, gy=got['gx']), dict(ref['dense'], gy=ref['dense']['gx'], gy_bound=ref['dense']['gx_bound']))
    out['gy'] = mc.worst_ratio(got['gy'], ref['gy'], ref['gy_bound'])
    return out


@pytest.mark.parametrize('case', INDEX_CASES, ids=ident)
@pytest.mark.parametrize('prefilled', [False, True])
def test_indexed_restatement_leaves_half_the_bound(case, prefilled):
    """Into an all-zero gy the adds of the contributions are all there is, and they leave half.  Into the randn prefill one
    correctly rounded add of |prefill| ~ 1 and |contribution| ~ 1e-6 errs by up to u |result|, and m u (|prefill| + sum
    |contribution|) at m = 1 IS that statement: nothing stays under half of it on 60 000 elements, and nothing correct exceeds
    it.  There the restatement is held to the bound itself, and to half of what is left once the adds have their roundings."""
    sx, h, scale = case
    x, y, pick, prefill = mc.make_index_case(sx, h, scale)
    if prefilled:
        ref = mc.index_case_references(sx, h, scale)
    else:
        prefill = torch.zeros_like(prefill)
        ref = mc.indexed_reference(x, y, pick, prefill, 0.37, 1.3)
    got = mc.restate(x, y, pick, prefill, 0.37, 1.3)
    for what, r in index_ratios(got, ref).items():
        print(f'RATIO restatement indexed {ident(case)} prefilled={prefilled} {what} {r:.3f}')
        assert r < (1.0 if (prefilled and what == 'gy') else 0.5), f'{what}: {r:.3f} of the bound'
    rest = mc.worst_ratio_after_adds(got['gy'], ref['gy'], ref['gy_bound'], ref['gy_adds'])
    print(f'RATIO restatement indexed {ident(case)} prefilled={prefilled} gy after its adds {rest:.3f}')
    assert rest < 0.5
    assert torch.equal(got['gy'][~ref['picked']], prefill[~ref['picked']])


@pytest.mark.parametrize('shape', mc.SAMPLER_SHAPES, ids=ident)
@pytest.mark.parametrize('accumulate', [False, True])
def test_sampler_restatement_leaves_half_the_bound(shape, accumulate):
    """The forward's last add (mu + eps sd, where eps sd may be 1e-4 of mu) and the accumulating backward's (prefill + value)
    are single roundings held to u |result|, as above: the whole error stays inside the bound, and what is left of it once
    that one rounding is granted stays under half of what is left of the bound."""
    z_pre, eps, g, prefill = mc.sampler_case(*shape)
    prefill = prefill if accumulate else None
    ref = mc.sampler_reference(z_pre, eps, g, prefill)
    got = dict(zip(('out', 'gz'), mc.sampler_restate(z_pre, eps, g, prefill)))
    for what in ('out', 'gz'):
        r = mc.worst_ratio(got[what], ref[what], ref[what + '_bound'])
        rest = mc.worst_ratio_after_adds(got[what], ref[what], ref[what + '_bound'], ref[what + '_adds'])
        print(f'RATIO restatement sampler {ident(shape)} acc={accumulate} {what} {r:.3f}, after its last add {rest:.3f}')
        assert r < 1.0 and rest < 0.5, f'{what}: {r:.3f} of the bound, {rest:.3f} after the last add'
        if what == 'gz' and not accumulate:
            assert r < 0.5


# ---- the bound rejects what is wrong ---------------------------------------------------------------------------------------------
def exempt(rule, group, single_row, indexed, gscale):
    """Where a wrong rule CANNOT differ from the right one (it must then give the same numbers, which the tests assert)."""
    if rule in ('index_off_by_one', 'store_not_add') and not indexed:
        return 'there is no index'
    if rule == 'store_not_add' and group == 'fwd':
        return 'the forward writes one slot a block'
    if rule == 'gscale_dropped' and (group == 'fwd' or gscale == 1.0):
        return 'the forward takes no gscale; gscale = 1 is dropped without trace'
    if single_row and rule == 'cross_weight':
        return '1 / n_same^2 = 1 / (sx sy) = 1'
    if single_row and rule == 'drop_last_same' and group == 'bwd':
        return "the only same-set row is the block's own: K = 1, a - a = 0, no gradient term (the forward loses its K = 1)"
    return None


@pytest.mark.parametrize('case', FORM_CASES, ids=ident)
def test_bound_rejects_the_wrong_rules(case):
    sx, sy, h, scale = case
    x, y = mc.make_case(sx, sy, h, scale)
    gscale, gmmd = mc.GRAD_ARGS[scale]
    ref, right = mc.case_references(sx, sy, h, scale), mc.restate(x, y, None, None, gscale, gmmd)
    for rule in mc.WRONG:
        bad = mc.restate(x, y, None, None, gscale, gmmd, wrong=rule)
        r = ratios(bad, ref)
        for group, names in GROUPS.items():
            if exempt(rule, group, sx == sy == 1, False, gscale):
                assert all(torch.equal(bad[n], right[n]) for n in names), (rule, group)
            else:
                worst = max(r[n] for n in names)
                print(f'RATIO wrong {rule} {ident(case)} {group} {worst:.1f}')
                assert worst > 1.0, f'{rule} {group}: only {worst:.3f} of the bound'


@pytest.mark.parametrize('case', INDEX_CASES, ids=ident)
def test_bound_rejects_the_wrong_rules_on_the_indexed_path(case):
    sx, h, scale = case
    args = mc.make_index_case(sx, h, scale)
    ref, right = mc.index_case_references(sx, h, scale), mc.restate(*args, 0.37, 1.3)
    for rule in mc.WRONG:
        bad = mc.restate(*args, 0.37, 1.3, wrong=rule)
        r = index_ratios(bad, ref)
        for group, names in GROUPS.items():
            if exempt(rule, group, False, True, 0.37):
                assert all(torch.equal(bad[n], right[n]) for n in names), (rule, group)
            else:
                worst = max(r[n] for n in names)
                print(f'RATIO wrong indexed {rule} {ident(case)} {group} {worst:.1f}')
                assert worst > 1.0, f'{rule} {group}: only {worst:.3f} of the bound'
    # the two index rules are visible in gy ALONE (gx may or may not move): that is the output they are about
    for rule in ('index_off_by_one', 'store_not_add'):
        bad = mc.restate(*args, 0.37, 1.3, wrong=rule)
        assert mc.worst_ratio(bad['gy'], ref['gy'], ref['gy_bound']) > 1.0, rule


def sampler_exempt(rule, what, repeat):
    if rule == 'no_threshold':
        return 'float32 sigmoid(raw) is exactly 1 above 16.7: the threshold at 20 is not visible in the factor'
    if rule == 'stride_k_wrong' and repeat == 1:
        return 's = k: row j is the only row of component j at either stride'
    if rule == 'sigmoid_dropped' and what == 'out':
        return 'the forward has no sigmoid'
    return None


@pytest.mark.parametrize('shape', mc.SAMPLER_SHAPES, ids=ident)
def test_bound_rejects_the_wrong_sampler_rules(shape):
    z_pre, eps, g, prefill = mc.sampler_case(*shape)
    ref = mc.sampler_reference(z_pre, eps, g, prefill)
    right = dict(zip(('out', 'gz'), mc.sampler_restate(z_pre, eps, g, prefill)))
    for rule in mc.SAMPLER_WRONG:
        bad = dict(zip(('out', 'gz'), mc.sampler_restate(z_pre, eps, g, prefill, wrong=rule)))
        for what in ('out', 'gz'):
            if sampler_exempt(rule, what, shape[2]):
                assert torch.equal(bad[what], right[what]), (rule, what)
            else:
                worst = mc.worst_ratio(bad[what], ref[what], ref[what + '_bound'])
                print(f'RATIO wrong sampler {rule} {ident(shape)} {what} {worst:.1f}')
                assert worst > 1.0, f'{rule} {what}: only {worst:.3f} of the bound'


# ---- zeros are rejected ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', FORM_CASES, ids=ident)
def test_an_all_zero_gradient_exceeds_the_bound_almost_everywhere(case):
    ref = mc.case_references(*case)
    for name in ('gx', 'gy'):
        share = mc.share_above(ref[name], ref[name + '_bound'])
        print(f'SHARE zeros rejected {ident(case)} {name} {share:.4f}')
        assert share >= 0.99, f'{name}: zeros pass on {1 - share:.2%} of the elements'
    assert mc.share_above(ref['partials'], ref['partials_bound']) == 1.0


@pytest.mark.parametrize('case', INDEX_CASES, ids=ident)
def test_a_backward_that_never_adds_exceeds_the_indexed_bound(case):
    """Into zeros (the loss head's own case) an untouched gy is an all-zero gradient: rejected on 99 % of the picked rows'
    elements.  Into the randn prefill one rounding of the prefill, u |prefill| ~ 6e-8, is of the size of the contributions
    themselves (4 |a| / (h^2 n) ~ 1e-7 .. 1e-6), so an untouched element is told apart only where the contribution is the larger:
    on more than half of them, which fails the comparison just as surely.  test_gpu_mmd.py runs both prefills."""
    sx, h, scale = case
    x, y, pick, prefill = mc.make_index_case(sx, h, scale)
    ref = mc.index_case_references(sx, h, scale)
    picked = ref['picked']
    assert mc.share_above(ref['dense']['gx'], ref['dense']['gx_bound']) >= 0.99
    assert mc.share_above((ref['gy'] - prefill.double())[picked], ref['gy_bound'][picked]) > 0.5
    zero = mc.indexed_reference(x, y, pick, torch.zeros_like(prefill), 0.37, 1.3)
    assert mc.share_above(zero['gy'][picked], zero['gy_bound'][picked]) >= 0.99


@pytest.mark.parametrize('shape', mc.SAMPLER_SHAPES, ids=ident)
def test_a_zero_sampler_gradient_exceeds_the_bound(shape):
    z_pre, eps, g, _ = mc.sampler_case(*shape)
    ref = mc.sampler_reference(z_pre, eps, g)
    assert mc.share_above(ref['gz'], ref['gz_bound']) >= 0.99
