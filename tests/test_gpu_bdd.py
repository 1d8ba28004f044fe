"""The block-diagonal R-GCN aggregation family (K1) against the float64 reference of oracle/bdd.py, element by element:

    per-row kernels (csrc/k_bdd.hip: k_agg_fast / _packed / _split / _generic, k_gradw_fast / _split / _generic, the fix-ups),
    relation phases (csrc/k_phase.hip: k_agg_phase; csrc/k_stream.hip: k_agg_stream), LDS-resident weights (csrc/k_lds.hip).

The host-only tests restate the dispatch (lane_plan, pack_plan, phase_plan, lds_plan and the GV_*_CASE tables, parsed out of
csrc/), check the restatement against the library's exported plan entries, and assert that the shapes below reach every
instantiation the tables list -- a new instantiation without a test fails here.  They also show that the bound would catch a
dropped edge, a wrong relation and a dropped split-row item at every shape used.

GV_K1_U, GV_K1_BPL1 and GV_K1_LDS_U are read once per process: those runs go to child processes (tests/workers/bdd_knob_worker.py).
Set GV_BDD_RATIOS=<file> to have the worst |got - ref| / bound per kernel family written there as JSON."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import bdd as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gcn-vae_amd', 'csrc')
gpu = pytest.mark.gpu


# ---- the dispatch tables, parsed ----------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _calls(text, macro):
    """Argument tuples of every use of ``macro(...)`` outside its #define, in source order."""
    out = []
    for m in re.finditer(r'(?<![\w#])' + macro + r'\(([^()]*)\)', text):
        line_start = text.rfind('\n', 0, m.start()) + 1
        if text[line_start:m.start()].lstrip().startswith('#define'):
            continue
        args = [a.strip() for a in m.group(1).split(',')]
        if any(re.search(r'_$', a) for a in args):        # a macro's own parameter list (P_, Q_, ...)
            continue
        out.append(tuple(True if a == 'true' else False if a == 'false' else int(a) for a in args))
    return out


def tables():
    bdd, phase, stream, lds = _src('k_bdd.hip'), _src('k_phase.hip'), _src('k_stream.hip'), _src('k_lds.hip')
    gw_at = bdd.index('extern "C" int gv_rgcn_bdd_grad_weight(')
    agg, gw = bdd[:gw_at], bdd[gw_at:]
    return {
        'PK': _calls(agg, 'GV_PK_CASE'), 'PK_U': _calls(agg, 'GV_PK_U'), 'SPLIT': _calls(agg, 'GV_SPLIT_CASE'),
        'AGG': _calls(agg, 'GV_AGG_CASE'), 'AGG_U': _calls(agg, 'GV_AGG_U'),
        'GW_SPLIT': _calls(gw, 'GV_GW_SPLIT'), 'GW': _calls(gw, 'GV_GW_CASE'),
        'PHASE': [c + (False,) for c in _calls(phase, 'GV_PHASE_CASE')] + _calls(phase, 'GV_PHASE_CASE_L'),
        'STREAM': _calls(stream, 'GV_STREAM_CASE'), 'LDS': _calls(lds, 'GV_LDS_CASE'),
    }


T = tables()
KNOB_U = (2, 4, 8)


def parsed_kernels():
    """Every kernel template instance the tables can launch (the per-process knobs included)."""
    ks = set()
    ks |= {('k_agg_packed',) + c for c in T['PK']}
    ks |= {('k_agg_packed',) + c + (u,) for c in T['PK_U'] for u in KNOB_U}
    ks |= {('k_agg_split',) + c[:5] for c in T['SPLIT']}
    ks |= {('k_agg_fast',) + c for c in T['AGG']}
    ks |= {('k_agg_fast',) + c + (u,) for c in T['AGG_U'] for u in KNOB_U}
    ks |= {('k_agg_generic', False), ('k_agg_generic', True), ('k_agg_fixup',)}
    ks |= {('k_gradw_split',) + c[:4] for c in T['GW_SPLIT']}
    ks |= {('k_gradw_fast',) + c for c in T['GW']}
    ks |= {('k_gradw_generic',), ('k_gradw_fixup4',), ('k_gradw_fixup',)}
    ks |= {('k_agg_phase',) + c for c in T['PHASE']}
    ks |= {('k_agg_stream',) + c + (lc,) for c in T['STREAM'] for lc in (50, 0)}
    ks |= {('k_agg_lds',) + c for c in T['LDS']}
    return ks


# ---- the plans, restated ------------------------------------------------------------------------------------------------
def lane_plan(nb, p, aggregate=False, bpl1=1):
    cands = {1: (4, 2), 2: (2, 4, 1), 4: (1, 2), 8: (1,), 10: (1,)}.get(p)
    if p == 5:
        cands = (1, 2) if (bpl1 and aggregate) else (2,)
    if cands is None:
        return None
    for bpl in cands:
        if nb % bpl:
            continue
        lanes = nb // bpl
        for parts in range(1, 17):
            if lanes % parts:
                continue
            per = lanes // parts
            if per <= 64 and (per >= 16 or parts == 1):
                return bpl, parts
    return None


def pack_plan(nb, p, q, trans):
    if p < 4:
        bpl = 4 // p
        if nb % bpl or nb // bpl > 64:
            return None
    else:
        bpl = next((b for b in (1, 2) if nb % b == 0 and nb // b <= 64), 0)
        if not bpl:
            return None
    if (bpl * p * q) % 4:
        return None
    ok = (((p == 2 and q in (2, 4)) or (p == 4 and q in (4, 8))) if not trans else
          ((p == 2 and q == 2) or (p == 4 and q in (2, 4)) or (p == 8 and q == 4)))
    return (bpl, 1 if p < 4 else 0) if ok else None


def agg_kernel(nb, p, q, trans, vec_ok=True, packed=False, u=0, bpl1=1):
    """The kernel gv_rgcn_bdd_aggregate launches (its selection order)."""
    if packed:
        pl = pack_plan(nb, p, q, trans)
        assert pl is not None and vec_ok
        if u:
            for c in T['PK_U']:
                if c == (p, q, trans) + pl:
                    return ('k_agg_packed',) + c + (u,)
        for c in T['PK']:
            if c[:5] == (p, q, trans) + pl:
                return ('k_agg_packed',) + c
    for pi, qo, t, qs, uu, parts in T['SPLIT']:
        if vec_ok and (pi, qo, t) == (p, q, trans) and nb % parts == 0 and (nb // parts) * (qo // qs) <= 64 and nb <= 32:
            return ('k_agg_split', pi, qo, t, qs, uu)
    lp = lane_plan(nb, p, True, bpl1)
    bpl = lp[0] if lp else 0
    if u and vec_ok and (p, q, trans, bpl) in T['AGG_U']:
        return ('k_agg_fast', p, q, trans, bpl, u)
    for c in T['AGG']:
        if vec_ok and c[:4] == (p, q, trans, bpl):
            return ('k_agg_fast',) + c
    return ('k_agg_generic', trans)


def gradw_kernel(nb, p, q, vec_ok=True, bpl1=1):
    for pp, qq, qs, uu, parts in T['GW_SPLIT']:
        if vec_ok and (pp, qq) == (p, q) and nb % parts == 0 and nb <= 32 and (nb // parts) * (qq // qs) <= 64:
            return ('k_gradw_split', pp, qq, qs, uu)
    lp = lane_plan(nb, p, p == 5 and q >= 10, bpl1)
    bpl = lp[0] if lp else 0
    for c in T['GW']:
        if vec_ok and c[:3] == (p, q, bpl):
            return ('k_gradw_fast',) + c
    return ('k_gradw_generic',)


PHASE_SHAPES = {(2, 2, False): (2, 8, 8, 0), (2, 4, False): (2, 8, 8, 0), (5, 5, False): (1, 6, 8, 0), (5, 10, False): (1, 2, 4, 1),
                (2, 2, True): (2, 8, 8, 0), (4, 2, True): (2, 4, 8, 0), (5, 5, True): (1, 6, 8, 0), (10, 5, True): (1, 2, 8, 0)}


def phase_plan(nb, p, q, trans, k_req=0):
    """(bpl, parts, lanes, k, qmajor) of k_phase.hip's phase_plan, or None."""
    if (p, q, trans) not in PHASE_SHAPES:
        return None
    bpl, u, k, qm = PHASE_SHAPES[(p, q, trans)]
    if nb % bpl:
        return None
    if k_req and k_req != k:
        if trans and (p, q) == (10, 5) and k_req == 3:
            k = 3
        elif k_req != 4 or k < 4:
            return None
        else:
            k = k_req
    slots = nb // bpl
    parts = next((c for c in range(1, 17) if slots % c == 0 and slots // c <= 64), 0)
    if not parts:
        return None
    return bpl, parts, slots // parts, k, qm


def phase_kernel(nb, p, q, trans, k_req=0, stream=True, dsel=0):
    pl = phase_plan(nb, p, q, trans, k_req)
    assert pl is not None
    bpl, parts, lanes, k, qm = pl
    if stream:
        seen = False
        for pas in (0, 1):
            for c in T['STREAM']:
                if c[:5] == (p, q, trans, bpl, k) and c[6] == bool(qm):
                    if pas == 0 and dsel and dsel != c[5]:
                        seen = True
                        continue
                    return ('k_agg_stream',) + c + (50 if lanes == 50 else 0,)
            if not seen:
                break
    for c in T['PHASE']:
        if c[:5] == (p, q, trans, bpl, k):
            return ('k_agg_phase',) + c
    return None


LDS_SHAPES = {(10, 10, False): (2, 1, 10, 4, 8), (10, 20, False): (2, 2, 5, 4, 8), (20, 10, False): (4, 2, 5, 4, 8),
              (10, 10, True): (2, 1, 10, 4, 8), (10, 20, True): (2, 1, 10, 3, 5), (20, 10, True): (4, 1, 10, 4, 8)}


def lds_plan(nb, p, q, num_rels, bf, u_env=0):
    """(ipl, oh, bpp, u, kb, parts) of k_lds.hip's lds_plan, or None."""
    if (p, q, bf) not in LDS_SHAPES:
        return None
    ipl, oh, bpp, u, kb = LDS_SHAPES[(p, q, bf)]
    if u_env == 6 and bpp * q == 100:
        u, kb = 6, 10
    if nb % bpp:
        return None
    slots = bpp * oh
    cl = 16 * ((slots - 1) // 3) + 5 * ((slots - 1) % 3) + p // ipl
    opl = q // oh
    nw = (ipl // 2) * opl if bf else ipl * opl
    nq, po = (nw + 3) // 4, bpp * q
    tq = num_rels * nq * cl
    if ((tq + 63) & ~63) * 16 + 16 * kb * po * 4 + 16 > 160 * 1024:
        return None
    return ipl, oh, bpp, u, kb, nb // bpp


def lds_kernel(nb, p, q, num_rels, bf, u_env=0):
    ipl, oh, bpp, u, kb, _ = lds_plan(nb, p, q, num_rels, bf, u_env)
    for c in T['LDS']:
        if c == (p, q, ipl, oh, bpp, u, kb, bf):
            return ('k_agg_lds',) + c
    return None


# ---- the test shapes: (num_bases, blk_in, blk_out, transpose) ---------------------------------------------------------------
# per-row aggregation, f32 weights (forward: transpose False; backward-x: True)
AGG_SHAPES = [
    (40, 1, 1, False), (40, 1, 2, False), (40, 1, 1, True), (40, 2, 1, True),
    (100, 2, 2, False), (100, 2, 4, False), (100, 2, 2, True), (100, 4, 2, True),
    (4, 4, 4, False), (4, 4, 8, False), (4, 4, 2, True), (4, 4, 4, True), (3, 8, 4, True),
    (666, 4, 4, False), (666, 4, 8, False), (666, 4, 2, True), (666, 4, 4, True),      # two blocks per lane: 333 lanes in 9 parts of 37
    (100, 5, 5, False), (100, 5, 10, False), (100, 5, 5, True), (50, 10, 5, True),
    (666, 5, 5, False), (666, 5, 10, False), (666, 5, 5, True),
    (40, 10, 10, False), (40, 10, 10, True),
    (20, 10, 10, False), (20, 10, 10, True), (20, 10, 20, False), (20, 20, 10, True),    # column-split kernels
    (6, 5, 5, False), (6, 5, 10, False), (3, 8, 4, False), (6, 5, 10, True),           # a single part; no case: generic
]
# lane-packed weights (ops.pack_weight): one block per lane (<= 64 bases) and two (66..128)
PACK_SHAPES = [(100, 2, 2, False), (100, 2, 4, False), (100, 2, 2, True), (40, 4, 2, True), (100, 4, 2, True),
               (16, 4, 4, False), (100, 4, 4, False), (16, 4, 8, False), (100, 4, 8, False), (16, 4, 4, True), (100, 4, 4, True),
               (16, 8, 4, True), (100, 8, 4, True)]
GW_SHAPES = [(40, 1, 1), (40, 1, 2), (100, 2, 2), (100, 2, 4), (16, 4, 4), (16, 4, 8), (666, 4, 4), (666, 4, 8),
             (100, 5, 5), (100, 5, 10), (666, 5, 10), (40, 10, 10), (20, 10, 10), (20, 10, 20), (6, 5, 5)]
# relation phases: (num_bases, blk_in, blk_out, transpose, rows per wave requested)
PHASE_RUNS = [(100, 2, 2, False, 0), (100, 2, 2, False, 4), (100, 2, 4, False, 0), (100, 2, 4, False, 4),
              (100, 2, 2, True, 0), (100, 2, 2, True, 4), (100, 4, 2, True, 0), (100, 4, 2, True, 4), (40, 4, 2, True, 0), (40, 4, 2, True, 4),
              (100, 5, 5, False, 0), (100, 5, 5, False, 4), (60, 5, 5, False, 0), (60, 5, 5, False, 4), (100, 5, 5, True, 0), (100, 5, 5, True, 4),
              (12, 5, 5, True, 0), (12, 5, 5, True, 4), (100, 5, 10, False, 0), (6, 5, 10, False, 0), (50, 10, 5, True, 0), (50, 10, 5, True, 4),
              (50, 10, 5, True, 3), (8, 10, 5, True, 0), (8, 10, 5, True, 4)]
# LDS-resident weights: (num_bases, blk_in, blk_out, num_rels, bf16)
LDS_RUNS = [(20, 10, 10, 22, False), (20, 10, 20, 22, False), (20, 20, 10, 22, False),
            (20, 10, 10, 22, True), (20, 10, 20, 22, True), (20, 20, 10, 22, True)]
# knob runs (child processes): GV_K1_U on the shapes its variants cover, GV_K1_BPL1=0 on the 5-wide blocks, GV_K1_LDS_U=6
U_SHAPES = [(100, 2, 2, False), (100, 2, 4, False), (100, 2, 2, True), (666, 4, 2, True)]
U_PACK_SHAPES = [(100, 2, 2, False), (100, 2, 4, False), (100, 2, 2, True), (100, 4, 2, True)]
BPL1_SHAPES = [(100, 5, 5, False), (100, 5, 10, False), (100, 5, 5, True)]
KNOBS = [{'GV_K1_U': str(u)} for u in KNOB_U] + [{'GV_K1_BPL1': '0'}, {'GV_K1_LDS_U': '6'}]
# the ring depth and XCD knobs are read per call (monkeypatch.setenv): D = 6 for the 5x10 blocks, the first listed otherwise
STREAM_D = {(5, 10, False): (2, 6), (10, 5, True): (2, 3)}

# instantiations no test shape can reach, with the reason
UNREACHABLE = {}


def knob_of(env):
    return {'u': int(env.get('GV_K1_U', 0)), 'bpl1': int(env.get('GV_K1_BPL1', 1)), 'lds_u': int(env.get('GV_K1_LDS_U', 0))}


def reached_kernels():
    ks = set()
    runs = [({}, True)] + [(k, False) for k in KNOBS]
    for env, base in runs:
        kn = knob_of(env)
        agg = AGG_SHAPES if base else (U_SHAPES if kn['u'] else BPL1_SHAPES if kn['bpl1'] == 0 else [])
        pack = PACK_SHAPES if base else (U_PACK_SHAPES if kn['u'] else [])
        for nb, p, q, t in agg:
            ks.add(agg_kernel(nb, p, q, t, u=kn['u'], bpl1=kn['bpl1']))
        for nb, p, q, t in pack:
            ks.add(agg_kernel(nb, p, q, t, packed=True, u=kn['u'], bpl1=kn['bpl1']))
        lds_runs = LDS_RUNS if (base or kn['lds_u']) else []
        for nb, p, q, r, bf in lds_runs:
            ks.add(lds_kernel(nb, p, q, r, bf, kn['lds_u']))
    for t in (False, True):                       # the unaligned base of test_bdd_aggregate_strided_and_unaligned
        ks.add(agg_kernel(4, 4, 4, t, vec_ok=False))
    ks.add(('k_agg_fixup',))
    for nb, p, q in GW_SHAPES:
        ks.add(gradw_kernel(nb, p, q))
    ks |= {('k_gradw_generic',), ('k_gradw_fixup4',), ('k_gradw_fixup',)}     # unaligned grad-W (fix-up without 16-B rows)
    for nb, p, q, t, k in PHASE_RUNS:
        ks.add(phase_kernel(nb, p, q, t, k))
        ks.add(phase_kernel(nb, p, q, t, k, stream=False))
        for d in STREAM_D.get((p, q, t), ()):
            ks.add(phase_kernel(nb, p, q, t, k, dsel=d))
    return ks


# ---- host-only: the restated plans agree with the library; every instantiation is reached -----------------------------------
def test_tables_parse():
    for name, n in (('PK', 13), ('PK_U', 4), ('SPLIT', 4), ('AGG', 25), ('AGG_U', 4), ('GW_SPLIT', 2), ('GW', 12), ('PHASE', 16),
                    ('STREAM', 10), ('LDS', 10)):
        assert len(T[name]) == n, (name, T[name])


def test_mirror_matches_the_exported_plans():
    """pack_plan vs gv_rgcn_bdd_pack_supported, phase_plan vs gv_rgcn_bdd_phase_plan, lds_plan vs gv_rgcn_bdd_lds_plan."""
    import ctypes
    from gcn_vae_amd import lib
    L = lib.load()
    blocks = [(1, 1), (1, 2), (2, 1), (2, 2), (2, 4), (4, 2), (4, 4), (4, 8), (8, 4), (5, 5), (5, 10), (10, 5), (10, 10),
              (10, 20), (20, 10), (3, 3)]
    bases = [1, 2, 3, 4, 6, 8, 12, 16, 20, 40, 50, 60, 64, 66, 100, 128, 130, 256, 666, 1000]
    plan = (ctypes.c_int32 * 7)()
    for p, q in blocks:
        for t in (False, True):
            for nb in bases:
                assert bool(L.gv_rgcn_bdd_pack_supported(nb, p, q, int(t))) == (pack_plan(nb, p, q, t) is not None), (nb, p, q, t)
                for k in (0, 3, 4, 8):
                    for thr in (0, 64, 256):
                        ok = L.gv_rgcn_bdd_phase_plan(nb, p, q, int(t), 120, 160 * 1024, 1, k, thr, ctypes.addressof(plan))
                        mine = phase_plan(nb, p, q, t, k)
                        assert bool(ok) == (mine is not None), (nb, p, q, t, k)
                        if ok:
                            assert (plan[0], plan[1], plan[2], plan[6]) == (mine[0], mine[1], mine[3], thr or 1024)
            for bf in (False, True):
                for nb in bases:
                    for r in (1, 22, 60, 200):
                        ok = L.gv_rgcn_bdd_lds_plan(nb, p, q, r, int(bf), ctypes.addressof(plan))
                        mine = lds_plan(nb, p, q, r, bf)
                        assert bool(ok) == (mine is not None), (nb, p, q, r, bf)
                        if ok:
                            assert plan[0] == mine[5]


def test_every_instantiation_is_reached():
    """The shapes and knob runs of this file, through the restated dispatch, reach exactly the parsed instantiations."""
    reached = reached_kernels()
    assert None not in reached
    parsed = parsed_kernels()
    missing = parsed - reached - set(UNREACHABLE)
    assert not missing, f'instantiations no test reaches: {sorted(missing, key=str)}'
    assert not (reached - parsed), f'the mirror names kernels the tables do not list: {sorted(reached - parsed, key=str)}'


def test_shapes_reach_the_kernels_they_claim():
    """Spot checks of the restated plans at the shapes named in the comments above."""
    assert lane_plan(666, 5, True) == (2, 9) and lane_plan(666, 4, True) == (2, 9)
    assert agg_kernel(666, 5, 10, False) == ('k_agg_fast', 5, 10, False, 2, 1)
    assert agg_kernel(100, 5, 5, False, bpl1=0) == ('k_agg_fast', 5, 5, False, 2, 2)
    assert agg_kernel(100, 5, 5, False) == ('k_agg_fast', 5, 5, False, 1, 2)
    assert agg_kernel(20, 10, 20, False) == ('k_agg_split', 10, 20, False, 4, 2)
    assert agg_kernel(6, 5, 5, False) == ('k_agg_fast', 5, 5, False, 1, 2)
    assert agg_kernel(3, 8, 4, False) == ('k_agg_generic', False)
    assert gradw_kernel(666, 5, 10) == ('k_gradw_fast', 5, 10, 2, 1)
    assert phase_kernel(50, 10, 5, True, 3) == ('k_agg_phase', 10, 5, True, 1, 3, 3, False)
    assert phase_kernel(100, 5, 10, False, dsel=6) == ('k_agg_stream', 5, 10, False, 1, 4, 6, True, 2, 50)
    assert phase_kernel(60, 5, 5, False) == ('k_agg_stream', 5, 5, False, 1, 8, 6, False, 1, 0)
    assert phase_plan(100, 5, 5, False)[1] == 2 and phase_plan(100, 5, 10, False)[1] == 2
    assert lds_kernel(20, 20, 10, 22, True, 6) == ('k_agg_lds', 20, 10, 4, 1, 10, 6, 10, True)


# ---- graphs -------------------------------------------------------------------------------------------------------------
def make_graph(degs, num_rels, seed, n_src=None, rels=None):
    """Edges into row i = degs[i], sources uniform, relations uniform over ``rels`` (default all); rows in order."""
    rs = np.random.RandomState(seed)
    n = len(degs)
    n_src = n if n_src is None else n_src
    dst = np.repeat(np.arange(n), degs)
    src = rs.randint(0, n_src, size=dst.size)
    pool = np.arange(num_rels) if rels is None else np.asarray(rels)
    et = pool[rs.randint(0, pool.size, size=dst.size)] if dst.size else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(src.astype(np.int64)), torch.from_numpy(dst.astype(np.int64)), torch.from_numpy(et.astype(np.int64))


def hub_degrees(n, chunk, seed):
    """Rows with no edge, one, the chunk exactly, one more, multiples of it and one more, the rest 0..12."""
    rs = np.random.RandomState(seed)
    d = rs.randint(0, 13, size=n)
    special = [0, 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 5 * chunk, 0, 1]
    d[:len(special)] = special
    d[n - 1] = 3 * chunk + 1
    d[n - 2] = 0
    return d


def operands(n, nb, p, q, num_rels, seed, n_src=None):
    gen = torch.Generator().manual_seed(seed)
    n_src = n if n_src is None else n_src
    feat = torch.randn(n_src, nb * p, generator=gen)
    weight = torch.randn(num_rels, nb * p * q, generator=gen)
    addend = torch.randn(n, nb * q, generator=gen)
    keep = (torch.rand(n, nb * q, generator=gen) > 0.25).to(torch.uint8)
    return feat, weight, addend, keep


# ---- host-only: negative controls ---------------------------------------------------------------------------------------
def _sample_rows(deg, count=12):
    rows = torch.nonzero(deg > 0).flatten().tolist()
    return rows[:count] + rows[-count:]


@pytest.mark.parametrize('shape', sorted(set(s[:4] for s in AGG_SHAPES)), ids=lambda s: 'x'.join(map(str, s)))
def test_bound_catches_a_wrong_edge(shape):
    """At sampled rows of every aggregation shape: the reference with one edge dropped, or with one edge given its neighbour's
    relation, or without one item of a split row, lies outside the bound."""
    nb, p, q, t = shape
    chunk, R = 8, 6
    n = 40 if nb * p * q < 20000 else 14
    degs = hub_degrees(n, chunk, nb + p + q)
    src, dst, et = make_graph(degs, R, nb * 3 + q)
    feat, weight, _, _ = operands(n, nb, p, q, R, nb + q)
    coef = torch.rand(src.numel()) + 0.5
    val, mag = ob.edge_terms(feat, weight, src, et, coef, nb, p, q, t)
    want, bnd, deg = ob.aggregate(feat, weight, dst, src, et, coef, n, nb, p, q, t, chunk=chunk, terms=(val, mag))
    rows = _sample_rows(deg)
    first = {i: int(torch.nonzero(dst == i).flatten()[0]) for i in rows}
    # one edge dropped: the first edge of the row
    assert min(float((val[first[i]].abs() / bnd[i]).max()) for i in rows) > 1.0
    # one edge given its neighbour's relation (the next relation id where the neighbour has the same one)
    for i in rows:
        e = first[i]
        et2 = et.clone()
        et2[e] = (et[e] + 1) % R
        v2, _ = ob.edge_terms(feat, weight, src[e:e + 1], et2[e:e + 1], coef[e:e + 1], nb, p, q, t)
        assert float(((val[e] - v2[0]).abs() / bnd[i]).max()) > 1.0, i
    # one item of a split row dropped
    split = [i for i in range(n) if degs[i] > chunk]
    for i in split:
        es = torch.nonzero(dst == i).flatten()
        item = val[es[chunk:2 * chunk]].sum(0)
        assert float((item.abs() / bnd[i]).max()) > 1.0, i


@pytest.mark.parametrize('shape', GW_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_grad_weight_bound_catches_a_wrong_edge(shape):
    nb, p, q = shape
    R, chunk = 5, 8
    n = 30
    src, dst, et = make_graph(np.full(n, 3), R, nb + q, rels=[0, 2, 3, 4])
    gen = torch.Generator().manual_seed(q)
    x, g = torch.randn(n, nb * p, generator=gen), torch.randn(n, nb * q, generator=gen)
    coef = torch.rand(src.numel(), generator=gen) + 0.5
    want, bnd, deg = ob.grad_weight(x, g, src, dst, et, coef, R, nb, p, q, chunk)
    for r in (0, 2, 4):
        es = torch.nonzero(et == r).flatten()
        e = int(es[0])
        term = coef[e].double() * torch.einsum('bp,bq->bpq', x[src[e]].double().view(nb, p), g[dst[e]].double().view(nb, q))
        assert float((term.reshape(-1).abs() / bnd[r]).max()) > 1.0
        item = sum(coef[int(k)].double() * torch.einsum('bp,bq->bpq', x[src[k]].double().view(nb, p),
                                                         g[dst[k]].double().view(nb, q)) for k in es[chunk:2 * chunk])
        assert float((item.reshape(-1).abs() / bnd[r]).max()) > 1.0
    assert torch.equal(want[1], torch.zeros_like(want[1]))


# ---- GPU ----------------------------------------------------------------------------------------------------------------
RATIOS = {}


def check(key, got, want, bnd):
    r = ob.max_ratio(got, want, bnd)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    assert r <= 1.0, f'{key}: |got - ref| / bound = {r:.3g}'
    return r


@pytest.fixture(scope='module', autouse=True)
def _report_ratios():
    yield
    path = os.environ.get('GV_BDD_RATIOS')
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


POISON = 1234.5
# (act, addend, keep, coef)
EPILOGUES = [(0, False, False, False), (1, True, True, True), (1, False, False, True), (0, True, False, True)]


def run_agg(ops, nb, p, q, t, seed, packed=False, chunk=8, n=None, epilogues=EPILOGUES, key=None):
    """Every epilogue of one shape on a hub-row graph; returns the outputs (for bit comparisons)."""
    R = 7
    n = n or (60 if nb * max(p, q) < 3000 else 24)
    degs = hub_degrees(n, chunk, seed)
    src, dst, et = make_graph(degs, R, seed, rels=[0, 1, 2, 4, 6])          # relations 3 and 5 have no edges
    feat, weight, addend, keep = operands(n, nb, p, q, R, seed)
    coef = torch.rand(src.numel(), generator=torch.Generator().manual_seed(seed)) + 0.25
    gi = ops.GraphIndex(src.cuda(), dst.cuda(), n, chunk=chunk)
    ri = ops.RelationIndex(gi, et.cuda(), R)
    assert gi.by_dst.seg.n_fix > 0
    terms = ob.edge_terms(feat, weight, src, et, coef, nb, p, q, t)
    terms1 = ob.edge_terms(feat, weight, src, et, None, nb, p, q, t)
    w_d = ops.pack_weight(weight.cuda(), nb, p, q, t) if packed else weight.cuda()
    key = key or str(agg_kernel(nb, p, q, t, packed=packed))
    outs = []
    for act, use_add, use_keep, use_coef in epilogues:
        want, bnd, deg = ob.aggregate(feat, weight, dst, src, et, coef if use_coef else None, n, nb, p, q, t,
                                      addend if use_add else None, act, keep if use_keep else None, 1.25, chunk=chunk,
                                      terms=terms if use_coef else terms1)
        got = ops.bdd_aggregate(gi.by_dst.seg, gi.nbr_by_dst, ri.et_by_dst, coef.cuda() if use_coef else None, gi.by_dst.perm,
                                feat.cuda(), w_d, nb, p, q, t, addend.cuda() if use_add else None, act,
                                keep.cuda() if use_keep else None, 1.25, packed=packed)
        check(key, got, want, bnd)
        empty = deg == 0
        exact = ob.edgeless_rows(n, nb * q, addend if use_add else None, act, keep if use_keep else None, 1.25)
        assert torch.equal(got.cpu()[empty], exact[empty])
        outs.append(got.cpu())
    return outs


@gpu
@pytest.mark.parametrize('shape', AGG_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bdd_aggregate_per_row(ops, shape):
    nb, p, q, t = shape
    run_agg(ops, nb, p, q, t, seed=nb + 3 * p + 7 * q + t)


@gpu
@pytest.mark.parametrize('shape', PACK_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bdd_aggregate_lane_packed(ops, shape):
    nb, p, q, t = shape
    run_agg(ops, nb, p, q, t, seed=nb + p + q, packed=True, epilogues=EPILOGUES[:2])


@gpu
def test_bdd_aggregate_edge_cases(ops):
    """An empty graph, a single node and one relation: rows without edges are exactly the epilogue of the addend."""
    for n, degs, R in ((5, [0] * 5, 1), (1, [3], 1), (1, [0], 2), (64, [1] * 64, 1)):
        nb, p, q = 4, 4, 4
        src, dst, et = make_graph(np.asarray(degs), R, n)
        feat, weight, addend, keep = operands(n, nb, p, q, R, n)
        gi = ops.GraphIndex(src.cuda(), dst.cuda(), n, chunk=2)
        ri = ops.RelationIndex(gi, et.cuda(), R)
        for use_add in (False, True):
            want, bnd, _ = ob.aggregate(feat, weight, dst, src, et, None, n, nb, p, q, False, addend if use_add else None, 1,
                                        keep, 1.25, chunk=2)
            got = ops.bdd_aggregate(gi.by_dst.seg, gi.nbr_by_dst, ri.et_by_dst, None, gi.by_dst.perm, feat.cuda(), weight.cuda(),
                                    nb, p, q, False, addend.cuda() if use_add else None, 1, keep.cuda(), 1.25)
            check(str(agg_kernel(nb, p, q, False)), got, want, bnd)


@gpu
@pytest.mark.parametrize('trans', [False, True])
def test_bdd_aggregate_strided_and_unaligned(ops, trans):
    """feat and out as windows of wider poison-filled tensors: ld > row (the vector kernels) and a base 1 float off 16 B (the
    generic kernels); every column outside the row keeps its poison."""
    nb, p, q, R, n, chunk = 4, 4, 4, 5, 50, 8
    degs = hub_degrees(n, chunk, 5)
    src, dst, et = make_graph(degs, R, 5)
    feat, weight, addend, keep = operands(n, nb, p, q, R, 5)
    coef = torch.rand(src.numel()) + 0.5
    gi = ops.GraphIndex(src.cuda(), dst.cuda(), n, chunk=chunk)
    ri = ops.RelationIndex(gi, et.cuda(), R)
    want, bnd, _ = ob.aggregate(feat, weight, dst, src, et, coef, n, nb, p, q, trans, addend, 1, keep, 1.25, chunk=chunk)
    for off in (0, 1):
        fbig = torch.full((n, nb * p + 12), POISON)
        fbig[:, off:off + nb * p] = feat
        fbig = fbig.cuda()
        obig = torch.full((n, nb * q + 12), POISON).cuda()
        out = obig[:, off:off + nb * q]
        ops.bdd_aggregate(gi.by_dst.seg, gi.nbr_by_dst, ri.et_by_dst, coef.cuda(), gi.by_dst.perm, fbig[:, off:off + nb * p],
                          weight.cuda(), nb, p, q, trans, addend.cuda(), 1, keep.cuda(), 1.25, out=out)
        check(str(agg_kernel(nb, p, q, trans, vec_ok=off == 0)), out, want, bnd)
        ob_ = obig.cpu()
        ob_[:, off:off + nb * q] = POISON
        assert torch.equal(ob_, torch.full_like(ob_, POISON)), 'a write outside the row'


def run_gradw(ops, nb, p, q, seed, aligned=True, chunk=8):
    R, n = 7, 40
    degs = np.random.RandomState(seed).randint(0, 6, size=n)
    src, dst, et = make_graph(degs, R, seed, rels=[0, 1, 2, 4, 6])
    gen = torch.Generator().manual_seed(seed)
    x, g = torch.randn(n, nb * p, generator=gen), torch.randn(n, nb * q, generator=gen)
    old = torch.randn(R, nb * p * q, generator=gen)
    coef = torch.rand(src.numel(), generator=gen) + 0.25
    gi = ops.GraphIndex(src.cuda(), dst.cuda(), n)
    ri = ops.RelationIndex(gi, et.cuda(), R, chunk=chunk)
    assert ri.by_rel.seg.n_fix > 0
    key = str(gradw_kernel(nb, p, q, vec_ok=aligned))
    for acc in (False, True):
        want, bnd, deg = ob.grad_weight(x, g, src, dst, et, coef, R, nb, p, q, chunk, old if acc else None)
        if aligned:
            out = old.cuda() if acc else None
            got = ops.bdd_grad_weight(ri.by_rel.seg, ri.src_by_rel, ri.dst_by_rel, coef.cuda(), ri.by_rel.perm, x.cuda(), g.cuda(),
                                      nb, p, q, out=out, accumulate=acc)
        else:
            big = torch.full((R * nb * p * q + 1,), POISON).cuda()
            out = big[1:].view(R, nb * p * q)
            if acc:
                out.copy_(old.cuda())
            xb = torch.zeros(n, nb * p + 1).cuda()
            xb[:, 1:] = x.cuda()
            got = ops.bdd_grad_weight(ri.by_rel.seg, ri.src_by_rel, ri.dst_by_rel, coef.cuda(), ri.by_rel.perm, xb[:, 1:], g.cuda(),
                                      nb, p, q, out=out, accumulate=acc)
            assert float(big[0].cpu()) == POISON
        check(key, got, want, bnd)
        none = deg == 0
        assert torch.equal(got.cpu()[none], (old if acc else torch.zeros_like(old))[none])


@gpu
@pytest.mark.parametrize('shape', GW_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bdd_grad_weight(ops, shape):
    nb, p, q = shape
    run_gradw(ops, nb, p, q, seed=nb + p + q)


@gpu
def test_bdd_grad_weight_unaligned(ops):
    """x and grad_w 1 float off 16 B: the generic kernel and the 4-B fix-up."""
    run_gradw(ops, 4, 4, 4, seed=3, aligned=False)


# ---- relation phases --------------------------------------------------------------------------------------------------------
def phase_run(ops, monkeypatch, nb, p, q, t, rows, threads, lds, src, dst, et, R, n, chunk, seed, epilogues=EPILOGUES[:2]):
    monkeypatch.setattr(ops.indices, 'PHASE_LDS_BYTES', lds)
    monkeypatch.setattr(ops.indices, 'PHASE_THREADS', threads)
    monkeypatch.setattr(ops.indices, 'PHASE_ROWS', rows)
    feat, weight, addend, keep = operands(n, nb, p, q, R, seed)
    # transposed (backward-x) launches gather along the forward edges' destinations into their sources
    rows_of, nbr_of = (src, dst) if t else (dst, src)
    coef = torch.rand(src.numel(), generator=torch.Generator().manual_seed(seed)) + 0.25
    gi = ops.GraphIndex(src.cuda(), dst.cuda(), n, chunk=chunk)
    ri = ops.RelationIndex(gi, et.cuda(), R)
    ph = ri.phase_order(gi, 'src' if t else 'dst', nb, p, q)
    assert ph is not None
    w_p = ops.pack_weight_phase(ph, weight.cuda(), nb, p, q)
    terms = ob.edge_terms(feat, weight, nbr_of, et, coef, nb, p, q, t)
    outs = []
    for act, use_add, use_keep, _ in epilogues:
        want, bnd, deg = ob.aggregate(feat, weight, rows_of, nbr_of, et, coef, n, nb, p, q, t, addend if use_add else None, act,
                                      keep if use_keep else None, 1.25, chunk=chunk, terms=terms)
        got = ops.bdd_aggregate_phases(ph, ph.coef(coef.cuda()), feat.cuda(), w_p, R, nb, p, q, addend.cuda() if use_add else None,
                                       act, keep.cuda() if use_keep else None, 1.25)
        check('phase ' + str(phase_kernel(nb, p, q, t, rows, stream=ops.indices.phase_stream_on())), got, want, bnd)
        exact = ob.edgeless_rows(n, nb * q, addend if use_add else None, act, keep if use_keep else None, 1.25)
        assert torch.equal(got.cpu()[deg == 0], exact[deg == 0])
        outs.append(got.cpu())
    return outs, ph


@gpu
@pytest.mark.parametrize('run', PHASE_RUNS, ids=lambda s: 'x'.join(map(str, s)))
def test_phase_kernels_streamed_and_batch_per_list(ops, monkeypatch, run):
    """Streamed and batch-per-list kernels (GV_PHASE_STREAM=0) against the reference and against each other (same bits), at
    64- and 256-thread workgroups with a short LDS budget (many phases, a short last one, relations without edges), hub rows
    split into 8-edge items; every ring depth GV_PHASE_STREAM_D names and the (tile, part) grid (GV_PHASE_XCD=0) give the
    same bits."""
    nb, p, q, t, rows = run
    R, n, chunk = 13, 70, 8
    degs = hub_degrees(n, chunk, nb + q)
    src, dst, et = make_graph(degs, R, nb + p, rels=[r for r in range(R) if r not in (4, 5, 11)])
    if t:
        src, dst = dst, src                     # the hub rows on the gathered-into side
        order = torch.sort(dst, stable=True)[1]
        src, dst, et = src[order], dst[order], et[order]
    res = {}
    for threads, lds in ((64, 12288), (256, 24576), (1024, 160 * 1024)):
        for stream in ('1', '0'):
            monkeypatch.setenv('GV_PHASE_STREAM', stream)
            outs, ph = phase_run(ops, monkeypatch, nb, p, q, t, rows, threads, lds, src, dst, et, R, n, chunk, nb + q)
            res[(threads, stream)] = outs
        assert all(torch.equal(a, b) for a, b in zip(res[(threads, '1')], res[(threads, '0')])), 'streamed vs batch-per-list'
    assert ph.n_fix > 0
    monkeypatch.setenv('GV_PHASE_STREAM', '1')
    pl = phase_plan(nb, p, q, t, rows)
    for d in STREAM_D.get((p, q, t), ()):
        monkeypatch.setenv('GV_PHASE_STREAM_D', str(d))
        outs, _ = phase_run(ops, monkeypatch, nb, p, q, t, rows, 256, 24576, src, dst, et, R, n, chunk, nb + q)
        assert all(torch.equal(a, b) for a, b in zip(outs, res[(256, '1')])), f'ring depth {d}'
    monkeypatch.delenv('GV_PHASE_STREAM_D', raising=False)
    if pl[1] == 2:
        monkeypatch.setenv('GV_PHASE_XCD', '0')
        outs, ph0 = phase_run(ops, monkeypatch, nb, p, q, t, rows, 128, 24576, src, dst, et, R, n, chunk, nb + q)
        monkeypatch.setenv('GV_PHASE_XCD', '1')
        outs1, ph1 = phase_run(ops, monkeypatch, nb, p, q, t, rows, 128, 24576, src, dst, et, R, n, chunk, nb + q)
        assert ph1.n_tiles % 4 != 0 or ph1.n_tiles < 4, ph1.n_tiles
        assert all(torch.equal(a, b) for a, b in zip(outs, outs1)), 'XCD grid vs (tile, part) grid'


STREAM_LENGTHS = [1, 5, 6, 7, 63, 64, 65, 127, 128, 129, 191, 193]


@gpu
@pytest.mark.parametrize('shape', [(100, 5, 5, False), (60, 5, 5, True), (100, 5, 10, False), (50, 10, 5, True)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_stream_lengths_around_the_ring_and_the_metadata_batches(ops, monkeypatch, shape):
    """One 64-thread workgroup: the wave's stream is exactly L positions long (the K rows of its tile hold L edges), for L
    around the ring depth D and the 64-position metadata batches; the batch-per-list kernel gives the same bits."""
    nb, p, q, t = shape
    K = phase_plan(nb, p, q, t)[3]
    R = 9
    for L in STREAM_LENGTHS:
        degs = np.full(K, L // K)
        degs[:L % K] += 1
        src, dst, et = make_graph(degs, R, L, rels=[0, 3, 4, 8])
        if t:
            src, dst = dst, src
            order = torch.sort(dst, stable=True)[1]
            src, dst, et = src[order], dst[order], et[order]
        res = []
        for stream in ('1', '0'):
            monkeypatch.setenv('GV_PHASE_STREAM', stream)
            outs, ph = phase_run(ops, monkeypatch, nb, p, q, t, 0, 64, 12288, src, dst, et, R, K, 256, L,
                                 epilogues=EPILOGUES[1:2])
            assert ph.n_tiles == 1 and int(ph.off[-1]) == L
            res.append(outs[0])
        assert torch.equal(res[0], res[1]), f'L = {L}'


@gpu
@pytest.mark.parametrize('run', LDS_RUNS, ids=lambda s: 'x'.join(map(str, s)))
def test_lds_resident_kernels(ops, run):
    run_lds(ops, *run)


def run_lds(ops, nb, p, q, R, bf, u_env=0):
    from gcn_vae_amd import indices
    n, chunk = 90, 64
    degs = hub_degrees(n, chunk, nb + q)
    src, dst, et = make_graph(degs, R, nb + p, rels=[r for r in range(R) if r % 5])
    feat, weight, addend, keep = operands(n, nb, p, q, R, nb + p + q)
    coef = torch.rand(src.numel(), generator=torch.Generator().manual_seed(2)) + 0.25
    gi = ops.GraphIndex(src.cuda(), dst.cuda(), n)
    ri = ops.RelationIndex(gi, et.cuda(), R)
    pl = indices.lds_plan(R, nb, p, q, bf=bf)
    assert pl is not None
    order = gi.lds_order('dst', pl[2])
    assert order.n_fix > 0 and order.n_empty > 0
    key = str(lds_kernel(nb, p, q, R, bf, u_env))
    outs = []
    for trans in (False, True):
        w_p = indices.pack_weight_lds(weight.cuda(), nb, p, q, trans, pl)
        terms = ob.edge_terms(feat, weight, src, et, coef, nb, p, q, trans, bf16=bf)
        for act, use_add, use_keep, _ in EPILOGUES[:2]:
            want, bnd, deg = ob.aggregate(feat, weight, dst, src, et, coef, n, nb, p, q, trans, addend if use_add else None, act,
                                          keep if use_keep else None, 1.25, chunk=pl[2], lds_ipl=LDS_SHAPES[(p, q, bf)][0],
                                          bf16=bf, terms=terms)
            got = indices.bdd_aggregate_lds(order, gi.nbr_by_dst, ri.et_by_dst, coef.cuda(), gi.by_dst.perm, feat.cuda(), w_p, R, nb,
                                            p, q, trans, addend.cuda() if use_add else None, act,
                                            keep.cuda() if use_keep else None, 1.25, plan=pl)
            check(key, got, want, bnd)
            exact = ob.edgeless_rows(n, nb * q, addend if use_add else None, act, keep if use_keep else None, 1.25)
            assert torch.equal(got.cpu()[deg == 0], exact[deg == 0])
            outs.append(got.cpu())
    return outs


# ---- the Python dispatch: one pass per family through ops.rel_graph_conv_bdd -------------------------------------------------
@gpu
@pytest.mark.parametrize('family', ['per_row', 'phases', 'lds'])
def test_rel_graph_conv_bdd_dispatch(ops, monkeypatch, family):
    """Forward output of the layer (self-loop addend through the dense product) within the K1 bound plus the product's own."""
    from gcn_vae_amd import indices
    if family == 'phases':
        nb, fin, fout, R = 100, 500, 500, 13
        monkeypatch.setattr(indices, 'K1_PHASES', '1')
        monkeypatch.setattr(indices, 'PHASE_LDS_BYTES', 24576)
        monkeypatch.setattr(indices, 'PHASE_THREADS', 256)
    elif family == 'lds':
        nb, fin, fout, R = 20, 200, 200, 22
    else:
        nb, fin, fout, R = 100, 200, 400, 13
        monkeypatch.setattr(indices, 'K1_LDS', '0')
    n, chunk = 80, 8
    degs = hub_degrees(n, chunk, 1)
    src, dst, et = make_graph(degs, R, 2)
    p, q = fin // nb, fout // nb
    feat, weight, _, keep = operands(n, nb, p, q, R, 3)
    loop = torch.randn(fin, fout, generator=torch.Generator().manual_seed(4)) * 0.1
    bias = torch.randn(fout, generator=torch.Generator().manual_seed(5))
    norm = torch.rand(src.numel(), 1) + 0.25
    gi = ops.GraphIndex(src.cuda(), dst.cuda(), n, chunk=chunk)
    ri = ops.RelationIndex(gi, et.cuda(), R)
    got = ops.rel_graph_conv_bdd(feat.cuda(), weight.cuda(), bias.cuda(), loop.cuda(), norm.cuda(), gi, ri, nb, 1, keep.cuda(), 1.25)
    addend = feat.double() @ loop.double() + bias.double()
    want, bnd, _ = ob.aggregate(feat, weight, dst, src, et, norm, n, nb, p, q, False, addend, 1, keep, 1.25,
                                chunk=64 if family == 'lds' else chunk, lds_ipl=2 if family == 'lds' else None)
    # the self-loop product's own rounding (fp32 fma chain over fin): (fin + 2) u (|x| @ |W| + |b|), scaled with the keep mask
    dense = (fin + 2) * ob.U * (feat.double().abs() @ loop.double().abs() + bias.double().abs())
    bnd = bnd + torch.where(keep.bool(), 1.25 * dense, torch.zeros((), dtype=torch.float64))
    check(f'rel_graph_conv_bdd {family}', got, want, bnd)


# ---- the per-process knobs, one child process each ----------------------------------------------------------------------------
@gpu
def test_static_knobs_in_child_processes(ops, tmp_path):
    """GV_K1_U = 2 / 4 / 8, GV_K1_BPL1=0 and GV_K1_LDS_U=6 are read once per process: each runs in a child of its own
    (tests/workers/bdd_knob_worker.py), one at a time; the first failing child stops the test.  GV_K1_BPL1=0 must give the bits
    of the default lane plan (k_bdd.hip: "bit-identical results")."""
    worker = os.path.join(ROOT, 'tests', 'workers', 'bdd_knob_worker.py')
    base = {}
    for nb, p, q, t in BPL1_SHAPES:
        base[f'{nb}x{p}x{q}x{int(t)}'] = run_agg(ops, nb, p, q, t, seed=nb + 3 * p + 7 * q + t)
    for knob in KNOBS:
        env = dict(os.environ, **knob)
        for name in ('GV_K1_U', 'GV_K1_BPL1', 'GV_K1_LDS_U'):
            if name not in knob:
                env.pop(name, None)
        dump = str(tmp_path / f'bdd_knob_{"_".join(f"{k}{v}" for k, v in knob.items())}.pt')
        out = subprocess.run([sys.executable, worker, dump], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, f'{knob}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-3000:]}'
        assert 'launches checked' in out.stdout, out.stdout[-2000:]
        line = [l for l in out.stdout.splitlines() if l.startswith('{')][-1]
        for key, r in json.loads(line).items():
            RATIOS[f'{key} {knob}'] = r
        if knob.get('GV_K1_BPL1') == '0':
            got = torch.load(dump)
            for name, outs in base.items():
                assert all(torch.equal(a, b) for a, b in zip(got[name], outs)), f'GV_K1_BPL1=0 changed the bits of {name}'
