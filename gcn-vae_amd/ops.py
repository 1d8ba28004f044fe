"""Tensor-level wrappers over the C ABI: index builders, raw ops, and torch.autograd Functions.

Every function here requires CUDA (ROCm) float32 tensors and the built HIP library; nothing
falls back to torch CPU math.  torch is used for device memory, the current stream and autograd
bookkeeping only (plus sort/cumsum when an index is built, outside the hot step).
"""
import contextlib
import ctypes as _ct
import itertools as _it
import os as _os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import lib
from .lib import ptr

ACT_NONE, ACT_RELU = 0, 1

# Direct gradient targets: parameter storage address -> the gradient buffer its gradient should be ADDED
# into (registered by optim.FlatAdam, whose arena is zeroed once per step).  A backward that finds its
# parameter here accumulates in place and returns None for it, so autograd launches no zero-fill and no
# AccumulateGrad add for that parameter.  Empty registry = ordinary autograd behaviour.
DIRECT_GRAD = {}
# Gradient buffers (keyed by address) that are known to be all-zero right now: the optimiser adds its arena slices after
# zero_grad() / step(); the first backward kernel that writes one removes it.  Only a buffer listed here may be
# OVERWRITTEN by a backward kernel (the identity-embedding path below); anything else is accumulated into.
GRAD_FRESH = set()
# Bumped whenever the registry changes (an optimiser is built or dropped).  A Function that resolved a direct target in its
# forward stamps the value on its ctx; its backward refuses to run if the registry changed in between (it would add into an
# arena that is no longer the parameters' -- INTEGRATION.md, "The optimiser contract").
DIRECT_EPOCH = [0]


def _stamp_direct(ctx):
    ctx._gv_direct_epoch = DIRECT_EPOCH[0]


def _verify_direct(ctx):
    if getattr(ctx, '_gv_direct_epoch', DIRECT_EPOCH[0]) != DIRECT_EPOCH[0]:
        raise RuntimeError('the optimiser gradient arena (ops.DIRECT_GRAD) changed between this forward and its backward: '
                           'build / drop FlatAdam outside a forward-backward pair')


def _direct(t):
    tgt = DIRECT_GRAD.get(t.data_ptr()) if t is not None else None
    return tgt if (tgt is not None and tgt.shape == t.shape) else None


def _direct_flat(t):
    """Direct target of a contiguous VIEW of a parameter that starts at its storage (e.g. z_pre.squeeze(0))."""
    tgt = DIRECT_GRAD.get(t.data_ptr()) if t is not None else None
    return tgt.view(t.shape) if (tgt is not None and tgt.numel() == t.numel() and tgt.is_contiguous()) else None
EPILOGUE_COLSUM_SLICES = 1024  # = GV_EPILOGUE_COLSUM_SLICES (include/gcnvae.h)
DEFAULT_CHUNK = 256        # max edges per work item of the dst/src-sorted aggregations
DEFAULT_CHUNK_REL = 128    # max edges per work item of the by-relation weight gradient


CHUNK_DIV = int(_os.environ.get('GV_CHUNK_DIV', '4096'))


def chunk_for(n_entries: int, most: int = DEFAULT_CHUNK) -> int:
    """Edges per work item for a list of ``n_entries``.  One wave walks an item's edges in order (four in flight), so on a SMALL
    graph the longest item, not the edge count, sets a launch's duration: a sampled batch of 20 000 edges whose hub rows were
    cut into 256-edge items spent 40-80 us per aggregation on 64 serial steps of one wave.  Items shrink with the list: a power of
    two, n / 4096 rounded down, between 16 and ``most`` (measured over n / 2048, 4096, 8192: FB15k-237-sized graphs -- 0.54 M
    edges -- run best on 128-edge items: 1.049 vs 1.058 ms at h = 200, 3.46 vs 3.56 ms at h = 500; lists of >= 1 M entries keep 256)."""
    env = _os.environ.get('GV_CHUNK')
    if env:
        return max(1, int(env))
    # by-relation lists (most = DEFAULT_CHUNK_REL) keep larger items: few, long segments -- 22 relations of 7 900 edges at WN18RR
    # size -- pay for every extra partial slot in the fix-up (weight-gradient launches 58 / 68 us with 128-edge items, 67 / 92 with 32)
    div = CHUNK_DIV // 4 if most == DEFAULT_CHUNK_REL else CHUNK_DIV
    c = 16
    while c * 2 <= most and c * 2 * div <= int(n_entries):
        c *= 2
    return c
DIST_FWD_CHUNKS = 2        # destination-row blocks whose all-reduce overlaps the next block's aggregation


# ------------------------------------------------------------------------------------------------
# fork / join on side streams: independent groups of small, latency-bound launches (KL, MMD, scalar
# reductions, weight-gradient GEMMs) run beside the bandwidth-bound kernels instead of behind them.
# Under hipGraph capture the event edges become parallel graph branches.  Buffers a branch writes are
# allocated by the caller BEFORE the fork (torch's allocator is per stream).  Opt in with GV_CONCURRENCY=1.
CONCURRENCY = _os.environ.get('GV_CONCURRENCY', '0') == '1'   # measured null on MI355X (1.49 vs 1.49 ms/step): off by default
_side_streams = {}


def _side(i):
    key = (torch.cuda.current_device(), i)
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream()
    return _side_streams[key]


@contextlib.contextmanager
def fork(i):
    """Run the enclosed launches on side stream ``i`` (after everything already enqueued on the current
    stream); pair with ``join(i)`` before their results are consumed."""
    if not CONCURRENCY:
        yield
        return
    s = _side(i)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        yield


def join(*ids):
    if CONCURRENCY:
        cur = torch.cuda.current_stream()
        for i in ids:
            cur.wait_stream(_side(i))


# Parameter gradients BESIDE the backward pass.  A launch whose only consumer is the optimiser (a weight gradient written straight
# into the gradient arena) need not hold up the kernels that feed autograd: it goes to one side stream -- a parallel branch of a
# captured graph -- and that stream is joined once, when the engine has run the whole backward pass (the optimiser step comes after).
# What such launches read is kept from the allocator until the join (autograd frees a node's saved tensors as soon as the node ran).
# Off when a process group exists: the gradients then feed all-reduces started inside the backward pass, and a captured step is a
# chain of graph segments cut at the collectives (a stream forked in one segment cannot be joined in another).
# Used by the MADE backward (weight-gradient products that need one workgroup per CU, beside backward chains whose second round
# of workgroups leaves half of the CUs idle: -0.13 ms at WN18RR size) and, since round 4, by the R-GCN layers' weight gradients
# where the layer is large (RGCN_BWD_SIDE below; in round 3, with the gradients going through AccumulateGrad and other kernels,
# the same cost more than it hid: FB15k-237 1.047 -> 1.089 ms per step, the mini-batch step 0.98 -> 1.11).  Not by the decoder's.
BWD_SIDE = _os.environ.get('GV_BWD_SIDE', '1') == '1'
_bwd_side_held = []
# ... the R-GCN layers' weight gradients too (round 4, with the arena targets): 'auto' = where the layer is large and the side stream
# carries nothing else in this backward pass -- measured per step: h = 500 3.41 -> 3.28 ms, 1 M nodes / 50 M edges 81.4 -> 78.9,
# FB15k-237 size 1.026 -> 1.020; NOT the mini-batch graph (20 000 edges: 0.967 -> 1.006) and not behind IAF blocks, whose weight-gradient
# products already run there (WN18RR + 3 IAF 4.98 -> 5.19, mini-batch + 3 IAF fp32 5.03 -> 5.15).  '0' / '1': never / wherever possible.
# (The decoder's relation-side gradient the same way: 1.020 -> 1.048 ms -- a 24-us launch does not carry its fork and join.)
RGCN_BWD_SIDE = _os.environ.get('GV_RGCN_BWD_SIDE', 'auto')
RGCN_BWD_SIDE_MIN_WORK = 10 ** 8       # edges x widest side of the layer


_bwd_side_others = [False]     # something other than an R-GCN layer put work on the side stream in this backward pass


def rgcn_bwd_side(num_edges, width):
    layout = launch_layout()
    if not layout.bwd_side or layout.process_group:      # (under a process group the arena feeds collectives started inside the pass)
        return False
    if RGCN_BWD_SIDE == 'auto':
        return not _bwd_side_others[0] and num_edges * width >= RGCN_BWD_SIDE_MIN_WORK
    return RGCN_BWD_SIDE == '1'


@dataclass(frozen=True)
class LaunchLayout:
    """How a step may spread its launches over streams -- decided in ONE place (``launch_layout()``) from the process state, read by
    ``backward_side``, ``made.made_prepare`` and ``made._by_row_blocks``."""
    timed: bool             # a lib.KernelTimer is installed (bench.py's per-kernel figures): every launch runs alone, in order
    process_group: bool     # a torch.distributed group exists: the step carries collectives, a captured step is a chain of segments
    bwd_side: bool          # a MADE's weight-gradient products beside the rest of the backward pass (side stream 'bwd')
    bwd_side_join_at_collective: bool   # ... joined in front of the next collective (a fork must not outlive its graph segment)
    made_prepare: bool      # the flows' parameter-only work beside the encoder's layers (side stream 'made_prep')
    row_blocks: bool        # a MADE's passes over independent row blocks on their own streams (forked and joined inside the node)


def launch_layout():
    from . import made as _made          # (made imports ops: resolved at call time)
    timed, pg = lib.TIMER is not None, _process_group()
    return LaunchLayout(
        timed=timed, process_group=pg,
        # the side stream is joined when the backward pass has run -- or, with collectives on the step, in front of the first
        # collective after the fork (distributed.start_collective -> backward_side_finish): the products then still run beside the
        # remaining backward chains of the flow stack, which is where they were hidden anyway
        bwd_side=BWD_SIDE and not timed, bwd_side_join_at_collective=pg,
        # forked at the START of the forward pass, in front of the encoder's collectives: not under a process group
        made_prepare=_made.MADE_PREPARE and not timed and not pg,
        row_blocks=not timed)


def _process_group():
    """A torch.distributed process group exists (even of one rank): the step then carries collectives, a captured step is a chain
    of graph SEGMENTS cut at them, and a stream forked in one segment may not be joined in another -- no deferred side streams."""
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized()


@contextlib.contextmanager
def backward_side(enabled, *held, rgcn=False):
    """Inside an autograd backward: run the enclosed launches on the side stream (after everything already enqueued); ``held``:
    the tensors they touch.  Yields whether the side stream is in use."""
    if not (enabled and launch_layout().bwd_side):      # (timed launches run alone: bench.py's per-kernel lines)
        # A node that stays on the main stream while an EARLIER node of this backward pass left work on the side stream: the two
        # may write the same slices of the gradient arena (one MADE's parameters behind two nodes -- the posterior pass and a
        # separate MMD prior pass; the first stores on the side stream, the second accumulates, or hands its gradient to
        # AccumulateGrad, on this one).  Order them: this stream waits for the side stream first.
        if _bwd_side_held:
            torch.cuda.current_stream().wait_stream(_side('bwd'))
        yield False
        return
    side, main = _side('bwd'), torch.cuda.current_stream()
    side.wait_stream(main)
    with torch.cuda.stream(side):
        yield True
    first = not _bwd_side_held
    _bwd_side_held.append(held)
    if not rgcn:
        _bwd_side_others[0] = True
    if first:
        def _join():
            if not _bwd_side_held:      # joined already (in front of a collective: backward_side_finish)
                return
            # the stream the pass was started under AND the one current now (backward() may be called under another stream than
            # the node's launches ran on; the optimiser reads the arena on the caller's)
            main.wait_stream(side)
            cur = torch.cuda.current_stream()
            if cur != main:
                cur.wait_stream(side)
            _bwd_side_held.clear()
            _bwd_side_others[0] = False
        torch.autograd.Variable._execution_engine.queue_callback(_join)


def backward_side_finish():
    """Join the side stream if a backward pass left work on it without reaching its end (an exception inside the pass): called
    by the optimiser before it reads or clears the gradient arena."""
    if _bwd_side_held:
        torch.cuda.current_stream().wait_stream(_side('bwd'))
        _bwd_side_held.clear()
    # unconditionally: a pass that raised (or ran without the engine's end-of-pass callback) after a MADE node had set the flag would
    # otherwise keep rgcn_bwd_side('auto') off for the rest of the process
    _bwd_side_others[0] = False


class StayOnDevice:
    """Mixin of the HIP modules: once their parameters live on a ROCm device, ``module.cpu()`` / ``.to('cpu')`` leaves them
    there.  The reference moves its model to the host for validation (kgvae/link_predict.py:239-242, "full graph is too
    large") and back; there is no CPU path here to move to -- the compute stays on the GPU and ``to_module_device`` brings
    whatever the caller hands in (node ids, relation types, norms on the host) to the parameters.  Not a fallback."""
    _gv_warned = False

    def _apply(self, fn, *args, **kwargs):
        dev = next((t.device for t in list(self.parameters()) + list(self.buffers()) if t.is_cuda), None)
        if dev is not None:
            try:
                moved = fn(torch.zeros(1, device=dev))
            except Exception:          # a fn that does not take a plain tensor: not a device move
                moved = None
            if moved is not None and moved.device.type == 'cpu':
                if not StayOnDevice._gv_warned:
                    StayOnDevice._gv_warned = True
                    import sys
                    print('[gcn_vae_amd] .cpu() on a HIP module is a no-op: parameters stay on %s, inputs are copied to them'
                          % dev, file=sys.stderr)
                return self
        return super()._apply(fn, *args, **kwargs)


def to_module_device(param, *tensors):
    """The caller's tensors on the device of ``param`` (a host -> device copy when they are elsewhere; None passes through)."""
    dev = param.device
    out = tuple(t if (t is None or not isinstance(t, torch.Tensor) or t.device == dev) else t.to(dev) for t in tensors)
    return out if len(out) != 1 else out[0]


def _chk(t, dtype=torch.float32, name='tensor'):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f'{name}: the gfx950 path needs a CUDA/ROCm tensor (got '
                           f'{type(t).__name__} on {getattr(t, "device", "?")}); there is no CPU fallback')
    if t.dtype != dtype:
        raise TypeError(f'{name}: expected {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{name}: must be contiguous')
    return t


def _row_major(t, name='matrix'):
    """2-D fp32 CUDA tensor with unit inner stride; returns (tensor, leading dimension)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f'{name}: the gfx950 path needs a CUDA/ROCm tensor; there is no CPU fallback')
    if t.dtype != torch.float32 or t.dim() != 2:
        raise TypeError(f'{name}: expected 2-D float32, got {t.dtype} {tuple(t.shape)}')
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


# ------------------------------------------------------------------------------------------------
# work-item lists, graph / relation / triplet indices, the phase and LDS-resident K1 launch forms: indices.py (same namespace
# for the callers: ops.GraphIndex, ops.bdd_aggregate_phases, ...)
# ------------------------------------------------------------------------------------------------
from .indices import *                                           # noqa: E402,F401,F403
from .indices import _carve_i32, _index_caps, _index_workspace, _rowptr_from_sorted      # noqa: E402,F401
from . import indices                                            # noqa: E402,F401  (ops.indices.<KNOB>: where that file's knobs live)
from . import batch_index                                        # noqa: E402,F401
from .batch_index import build_batch_indices                      # noqa: E402,F401


# ------------------------------------------------------------------------------------------------
# raw ops
RGCN_SIDE_GRADW_FIRST = _os.environ.get('GV_RGCN_SIDE_GRADW_FIRST', 'auto')


def rgcn_side_gradw_first(num_edges, width):
    """Order of the layer's two weight gradients on the backward side stream.  The main stream runs the self-loop's dL/dx product
    (MFMA-bound) and then the K1^T aggregation (cache-bandwidth-bound); with the relation-weight gradient (cache-bandwidth-bound)
    FIRST on the side stream and the self-loop's weight-gradient product (MFMA-bound) behind it, the launches that run beside each
    other want different things.  Measured: FB15k-237 size, h = 200: 1.005 -> 0.986 ms; h = 500: 2.993 -> 2.999; 1 M nodes / 50 M
    edges: 75.0 -> 75.2; WN18RR + 3 IAF: the same.  'auto': cache-resident graphs at input widths up to 256; '0' / '1' force."""
    if RGCN_SIDE_GRADW_FIRST in ('0', '1'):
        return RGCN_SIDE_GRADW_FIRST == '1'
    return num_edges <= 4_000_000 and width <= 256


def _k1_items(gidx, seg):
    """The work-item list a single-GPU K1 launch over a static graph walks: long items first where that is switched on."""
    if indices.K1_ITEMS_LARGEST_FIRST and not gidx.sync_free:
        return indices.largest_first(seg)
    return seg


def pack_supported(num_bases, blk_in, blk_out, transpose_w=False):
    return bool(lib.load().gv_rgcn_bdd_pack_supported(num_bases, blk_in, blk_out, 1 if transpose_w else 0))


def pack_weight(weight, num_bases, blk_in, blk_out, transpose_w=False):
    """Lane-packed copy of a bdd relation-weight matrix for one K1 launch kind (see include/gcnvae.h)."""
    weight = _chk(weight, name='weight')
    packed = torch.empty_like(weight)
    lib.call('gv_rgcn_bdd_pack_weight', ptr(weight), weight.shape[0], num_bases, blk_in, blk_out,
             1 if transpose_w else 0, ptr(packed), lib.stream())
    return packed


def _check_items(seg: SegmentItems):
    """The kernels index these lists by launch geometry: refuse a handle whose counts exceed its buffers."""
    if seg.n_items < 0 or seg.n_fix < 0 or seg.items.numel() < 4 * seg.n_items or seg.fix.numel() < 4 * seg.n_fix:
        raise ValueError(f'inconsistent work-item lists: n_items={seg.n_items} (buffer {seg.items.numel() // 4}), '
                         f'n_fix={seg.n_fix} (buffer {seg.fix.numel() // 4})')
    if seg.n_items > 0 and seg.items.data_ptr() == 0:
        raise ValueError('work-item list has no storage')


def bdd_aggregate(seg: SegmentItems, nbr, etype, coef, coef_idx, feat, weight, num_bases, blk_in, blk_out,
                  transpose_w=False, addend=None, act=ACT_NONE, keep=None, keep_scale=1.0, out=None, packed=False):
    feat, ld_feat = _row_major(feat, 'feat')
    weight = _chk(weight, name='weight')
    n_seg = seg.rowptr.numel() - 1
    out_dim = num_bases * blk_out
    if feat.shape[1] != num_bases * blk_in:
        raise ValueError(f'feat has {feat.shape[1]} columns, expected num_bases*blk_in = {num_bases * blk_in}')
    num_rels = weight.shape[0]
    if weight.numel() != num_rels * num_bases * blk_in * blk_out:
        raise ValueError('weight shape does not match (R, num_bases*blk_in*blk_out)')
    if out is None:
        out = torch.empty(n_seg, out_dim, dtype=torch.float32, device=feat.device)
    ld_add = 0
    if addend is not None:
        addend, ld_add = _row_major(addend, 'addend')
        if tuple(addend.shape) != (n_seg, out_dim):
            raise ValueError('addend shape mismatch')
    if keep is not None:
        _chk(keep, torch.uint8, 'keep')
        if tuple(keep.shape) != (n_seg, out_dim):
            raise ValueError('keep shape mismatch')
    if coef is not None:
        coef = _chk(coef.reshape(-1), name='coef')
    _check_items(seg)
    partial = None
    if seg.n_fix > 0:
        partial = torch.empty(seg.n_slots, out_dim, dtype=torch.float32, device=feat.device)
    ld_out = out.stride(0) if n_seg > 1 else out_dim
    tag = f'agg_{"T" if transpose_w else "N"}_{blk_in}x{blk_out}_nb{num_bases}'
    # (per-kernel timing, bench.py: the aggregation kernel is timed alone, the split rows' fix-up launched behind it)
    timed = lib.TIMER is not None
    lib.call('gv_rgcn_bdd_aggregate', ptr(seg.items), seg.n_items, ptr(seg.fix), 0 if timed else seg.n_fix, ptr(nbr),
             ptr(etype), ptr(coef), ptr(coef_idx), ptr(feat), ld_feat, ptr(weight), num_rels, num_bases, blk_in,
             blk_out, 1 if transpose_w else 0, 1 if packed else 0, ptr(addend), ld_add, act, ptr(keep),
             float(keep_scale), ptr(out), ld_out, ptr(partial), lib.stream(), tag=tag)
    if timed and seg.n_fix > 0:      # the aggregation kernel was timed alone; finish the split rows
        lib.call('gv_rgcn_bdd_fixup', ptr(seg.fix), seg.n_fix, ptr(partial), out_dim, ptr(addend), ld_add, act,
                 ptr(keep), float(keep_scale), ptr(out), ld_out, lib.stream())
    return out


def bdd_grad_weight(seg: SegmentItems, src, dst, coef, coef_idx, x, g, num_bases, blk_in, blk_out, out=None,
                    accumulate=False):
    x, ld_x = _row_major(x, 'x')
    g, ld_g = _row_major(g, 'g')
    n_seg = seg.rowptr.numel() - 1
    w_row = num_bases * blk_in * blk_out
    if out is None:
        out = torch.empty(n_seg, w_row, dtype=torch.float32, device=x.device)
        accumulate = False
    if coef is not None:
        coef = _chk(coef.reshape(-1), name='coef')
    partial = None
    if seg.n_fix > 0:
        partial = torch.empty(seg.n_slots, w_row, dtype=torch.float32, device=x.device)
    lib.call('gv_rgcn_bdd_grad_weight', ptr(seg.items), seg.n_items, ptr(seg.fix), seg.n_fix, ptr(src), ptr(dst),
             ptr(coef), ptr(coef_idx), ptr(x), ld_x, ptr(g), ld_g, num_bases, blk_in, blk_out, ptr(out), ptr(partial),
             1 if accumulate else 0, lib.stream(), tag=f'gradw_{blk_in}x{blk_out}_nb{num_bases}')
    return out


GEMM_PRECISION = 'f32'      # 'f32': exact fp32 MFMA; 'bf16': bf16 operands, fp32 accumulation (BASELINE configs[2])


def set_gemm_precision(precision):
    """Precision of every dense product on the path (MaskedLinear, self-loop term, evaluation scorer)."""
    global GEMM_PRECISION
    if precision not in ('f32', 'bf16'):
        raise ValueError("precision must be 'f32' or 'bf16'")
    GEMM_PRECISION = precision


@contextlib.contextmanager
def gemm_precision(precision):
    old = GEMM_PRECISION
    set_gemm_precision(precision)
    try:
        yield
    finally:
        set_gemm_precision(old)


LIVE_ROWS = None        # (device int32 (1,), cap): inside a static-shape batch step, node arrays of cap rows hold *rows_dev real rows


class live_rows:
    """``with ops.live_rows(rows_dev, cap):`` -- the fp32 products over node arrays of exactly ``cap`` rows skip the padding rows
    (gv_gemm_f32_live_rows: zero rows out, a shorter reduction for the weight gradients; gv_made_chain_f32: workgroups that hold
    only padding rows).  graph_step.GraphedMiniBatchStep wraps the step in it: ~30 % of a sampled batch's 14 541 padded rows are
    padding.
    CONTRACT: inside the context EVERY fp32 operand of exactly ``cap`` rows is taken for a padded node array -- the match is by
    row count, nothing marks the arrays.  The caller must not run products over other (cap, k) operands inside it (the captured
    mini-batch step does not: its only other row counts are cap + 200 and 200).  The VALUES of padding rows behind the first
    ``*rows_dev`` are unspecified (zeros from skipped tiles / workgroups, act(bias) from tiles that straddle the boundary); they
    take no part in any sum, mean or gradient."""

    def __init__(self, rows_dev, cap):
        self.val = (rows_dev, int(cap)) if rows_dev is not None else None

    def __enter__(self):
        global LIVE_ROWS
        self.saved, LIVE_ROWS = LIVE_ROWS, self.val
        return self

    def __exit__(self, *exc):
        global LIVE_ROWS
        LIVE_ROWS = self.saved
        return False


# Riders (csrc/k_riders.h, gv_gemm_f32_riders): the forward head's small launches whose inputs do not depend on a layer's self-loop
# product -- the forward's random draws, layer 2's lane-packed weights, the KL mixture table -- run as extra workgroups of that
# product's launch.  GV_GEMM_RIDERS=0: every one of them stand-alone, where it stood before.
# The finisher kinds: the prior sampler of get_mmd on layer 2's forward product ('prior'); in the backward, on a layer's
# dL/dx = g @ loop_weight^T, the KL backward's finishing launch ('klfin', layer 2) and the bias column sums of an epilogue
# backward ('colsum', layer 1) -- their inputs are complete before that product and nothing reads their outputs (arena slices,
# leaf gradients) before the optimiser.
GEMM_RIDERS = _os.environ.get('GV_GEMM_RIDERS', '1') == '1'
RIDER_KINDS_ALL = ('rng', 'pack', 'mix', 'prior', 'klfin', 'colsum')
GEMM_RIDER_KINDS = set(_os.environ.get('GV_GEMM_RIDER_KINDS', ','.join(RIDER_KINDS_ALL)).split(','))      # measurement: which kinds may ride


def rider_kind(kind):
    """Whether jobs of ``kind`` are handed to a RiderBox at all (off: the launch stays where it stood, nothing is deferred)."""
    return GEMM_RIDERS and kind in GEMM_RIDER_KINDS


def _dist_active():
    return torch.distributed.is_available() and torch.distributed.is_initialized()


class _Riders(_ct.Structure):
    """ctypes mirror of gv_riders (include/gcnvae.h)."""
    _fields_ = [('rng_state', _ct.c_void_p), ('rng_ptr', _ct.c_void_p * 8), ('rng_count', _ct.c_int64 * 8),
                ('rng_kind', _ct.c_int32 * 8), ('rng_drop_p', _ct.c_float * 8), ('rng_stream', _ct.c_uint32 * 8),
                ('rng_jobs', _ct.c_int32), ('pack_rels', _ct.c_int32), ('pack_bases', _ct.c_int32), ('pack_blk_in', _ct.c_int32),
                ('pack_blk_out', _ct.c_int32), ('pack_transpose', _ct.c_int32), ('pack_weight', _ct.c_void_p),
                ('packed', _ct.c_void_p), ('packed_pair', _ct.c_void_p), ('mix_z_pre', _ct.c_void_p), ('mix', _ct.c_void_p),
                ('mix_k', _ct.c_int32), ('mix_h', _ct.c_int32)]


class _RidersFin(_ct.Structure):
    """ctypes mirror of gv_riders_fin (include/gcnvae.h)."""
    _fields_ = [('prior_z_pre', _ct.c_void_p), ('prior_eps', _ct.c_void_p), ('prior_out', _ct.c_void_p), ('kl_part', _ct.c_void_p),
                ('kl_z_pre', _ct.c_void_p), ('kl_gkl', _ct.c_void_p), ('kl_g_zpre', _ct.c_void_p), ('kl_g_bias', _ct.c_void_p),
                ('cs_part', _ct.c_void_p), ('cs_out', _ct.c_void_p), ('kl_n', _ct.c_int64), ('kl_gscale', _ct.c_float),
                ('prior_s', _ct.c_int32), ('prior_k', _ct.c_int32), ('prior_h', _ct.c_int32), ('kl_slices', _ct.c_int32),
                ('kl_h', _ct.c_int32), ('kl_k', _ct.c_int32), ('kl_accumulate', _ct.c_int32), ('kl_accumulate_bias', _ct.c_int32),
                ('cs_n', _ct.c_int32), ('cs_slices', _ct.c_int32), ('cs_accumulate', _ct.c_int32)]


class RiderBox:
    """Explicit hand-off of independent small jobs to the NEXT self-loop product of one layer call (KGVAE.forward ->
    RelGraphConv.forward -> _RelGraphConvBdd.forward -> _gemm_addend -> gemm(..., riders=box)): whoever holds the box either
    launches its jobs as riders of that product (``ride``) or, where the combined launch does not apply, stand-alone on the
    spot (``flush``) -- in both cases on the caller's stream and before anything reads what they write.  ``done`` says that
    one of the two happened; the encoder checks it after the layer call, so a box cannot be dropped silently.
      rng  : (DeviceRNG, [(tensor, kind, drop_p, stream)]) -- already claimed (DeviceRNG.claim), at most 8 jobs ride
      pack : (weight, num_bases, blk_in, blk_out, transpose_w, packed, packed_pair or None)
      mix  : (z_pre (2k, h) contiguous, KL workspace) -- the table at the head of the workspace
      prior : (z_pre, eps (s, h), out) -- gv_prior_sample_fwd
      klfin : (KL workspace, z_pre, gkl, gscale, g_zpre, accumulate, g_bias or None, accumulate_bias, n, h, k) -- the finisher of
              gv_reparam_kl_bwd_fold_sweep's slice sums
      colsum: (part, n, slices, out, accumulate) -- gv_colsum_finish
    A box made in a backward pass (the last two kinds) is launched by the layer backward that made or received it."""
    __slots__ = ('rng', 'pack', 'mix', 'prior', 'klfin', 'colsum', 'done', 'rode')

    def __init__(self):
        self.rng = self.pack = self.mix = self.prior = self.klfin = self.colsum = None
        self.done = False
        self.rode = ()          # the kinds that went out as riders (tests, profiles)

    def empty(self):
        return all(getattr(self, k) is None for k in RIDER_KINDS_ALL)

    def _kl_part(self):
        ws, h, k = self.klfin[0], self.klfin[9], self.klfin[10]
        l = lib.load()
        return ws.data_ptr() + 4 * int(l.gv_kl_bwd_part_offset(h, k)), int(l.gv_kl_bwd_slices())

    def _launch_alone(self, kinds):
        if 'rng' in kinds and self.rng is not None:
            self.rng[0].launch(self.rng[1])
        if 'pack' in kinds and self.pack is not None:
            w, nb, bi, bo, trans, packed, pair = self.pack
            if pair is not None:
                lib.call('gv_rgcn_bdd_pack_weight_pair', ptr(w), w.shape[0], nb, bi, bo, ptr(packed), ptr(pair), lib.stream())
            else:
                lib.call('gv_rgcn_bdd_pack_weight', ptr(w), w.shape[0], nb, bi, bo, 1 if trans else 0, ptr(packed), lib.stream())
        if 'mix' in kinds and self.mix is not None:
            z_pre, ws = self.mix
            lib.call('gv_kl_mix', ptr(z_pre), z_pre.shape[0] // 2, z_pre.shape[1], ptr(ws), lib.stream())
        if 'prior' in kinds and self.prior is not None:
            z_pre, eps, out = self.prior
            lib.call('gv_prior_sample_fwd', ptr(z_pre), ptr(eps), ptr(out), eps.shape[0], z_pre.shape[0] // 2, z_pre.shape[1],
                     lib.stream())
        if 'klfin' in kinds and self.klfin is not None:
            _, z_pre, gkl, gscale, gzp, acc, g_bias, acc_b, n, h, k = self.klfin
            part, slices = self._kl_part()
            lib.call('gv_kl_bwd_mix_final', part, slices, ptr(z_pre), ptr(gkl), float(gscale), ptr(gzp), 1 if acc else 0, ptr(g_bias),
                     1 if acc_b else 0, n, h, k, lib.stream())
        if 'colsum' in kinds and self.colsum is not None:
            part, n, slices, out, acc = self.colsum
            lib.call('gv_colsum_finish', ptr(part), n, slices, ptr(out), 1 if acc else 0, lib.stream())

    def flush(self):
        """Every job stand-alone, here and now."""
        if self.done:
            raise RuntimeError('RiderBox: its jobs were already launched')
        self._launch_alone(RIDER_KINDS_ALL)
        self.done = True

    def ride(self, gemm_args):
        """Launch the product ``gemm_args`` (gv_gemm_f32's arguments without the stream) with the jobs as its riders."""
        if self.done:
            raise RuntimeError('RiderBox: its jobs were already launched')
        ride = {k for k in RIDER_KINDS_ALL if getattr(self, k) is not None and k in GEMM_RIDER_KINDS}
        if 'rng' in ride and len(self.rng[1]) > 8:
            ride.discard('rng')
        self._launch_alone(set(RIDER_KINDS_ALL) - ride)
        d = _Riders()
        if 'rng' in ride:
            rng, jobs = self.rng
            d.rng_state, d.rng_jobs = rng.state.data_ptr(), len(jobs)
            for i, (t, kind, p, st) in enumerate(jobs):
                d.rng_ptr[i], d.rng_count[i], d.rng_kind[i], d.rng_drop_p[i], d.rng_stream[i] = t.data_ptr(), t.numel(), kind, float(p), st
        if 'pack' in ride:
            w, nb, bi, bo, trans, packed, pair = self.pack
            d.pack_weight, d.packed, d.packed_pair = w.data_ptr(), packed.data_ptr(), (pair.data_ptr() if pair is not None else None)
            d.pack_rels, d.pack_bases, d.pack_blk_in, d.pack_blk_out, d.pack_transpose = w.shape[0], nb, bi, bo, 1 if trans else 0
        if 'mix' in ride:
            z_pre, ws = self.mix
            d.mix_z_pre, d.mix, d.mix_k, d.mix_h = z_pre.data_ptr(), ws.data_ptr(), z_pre.shape[0] // 2, z_pre.shape[1]
        if gemm_args[1] or ride & {'prior', 'klfin', 'colsum'}:     # A @ B^T, or a finisher kind: the entry that knows them
            f = _RidersFin()
            if 'prior' in ride:
                z_pre, eps, out = self.prior
                f.prior_z_pre, f.prior_eps, f.prior_out = z_pre.data_ptr(), eps.data_ptr(), out.data_ptr()
                f.prior_s, f.prior_k, f.prior_h = eps.shape[0], z_pre.shape[0] // 2, z_pre.shape[1]
            if 'klfin' in ride:
                _, z_pre, gkl, gscale, gzp, acc, g_bias, acc_b, n, h, k = self.klfin
                f.kl_part, f.kl_slices = self._kl_part()
                f.kl_z_pre, f.kl_gkl, f.kl_g_zpre, f.kl_g_bias = z_pre.data_ptr(), ptr(gkl), gzp.data_ptr(), ptr(g_bias)
                f.kl_gscale, f.kl_n, f.kl_h, f.kl_k = float(gscale), n, h, k
                f.kl_accumulate, f.kl_accumulate_bias = 1 if acc else 0, 1 if acc_b else 0
            if 'colsum' in ride:
                part, n, slices, out, acc = self.colsum
                f.cs_part, f.cs_out, f.cs_n, f.cs_slices, f.cs_accumulate = part.data_ptr(), out.data_ptr(), n, slices, 1 if acc else 0
            lib.call('gv_gemm_f32_riders_fin', *gemm_args, _ct.addressof(d), _ct.addressof(f), lib.stream())
        else:
            lib.call('gv_gemm_f32_riders', *gemm_args, _ct.addressof(d), lib.stream())
        self.rode = tuple(sorted(ride))
        self.done = True


def gemm(a, b, trans_a=False, trans_b=False, bias=None, act=ACT_NONE, out=None, accumulate=False, split_k=1,
         a_relu_mask=None, precision=None, b_k_chunks=None, c_tiles=None, riders=None):
    """out = act(op(a') @ op(b) + bias) (+ out);  a' = a * [a_relu_mask > 0] when a mask (same layout as a) is given.
    precision None = the global GEMM_PRECISION.  b_k_chunks / c_tiles (int64 device words, ops.block_words): blocks of op(b) / tiles
    of the result known to be zero are skipped (gv_gemm_f32_sparse; fp32 only).  ``riders`` (RiderBox): its jobs ride on this
    launch where that form exists (plain fp32 A @ B or A @ B^T, no split-K, no zero-block words, no live-row count) and are launched
    stand-alone in front of it everywhere else."""
    a, lda = _row_major(a, 'a')
    b, ldb = _row_major(b, 'b')
    m, k = (a.shape[1], a.shape[0]) if trans_a else a.shape
    kb, n = (b.shape[1], b.shape[0]) if trans_b else b.shape
    if k != kb:
        raise ValueError(f'gemm inner dimensions differ: {k} vs {kb}')
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=a.device)
        accumulate = False
    else:       # written through (pointer, out.stride(0)) only: a wrong shape, type or layout would be written out of bounds
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.dim() != 2:
            raise TypeError(f'out: expected a 2-D float32 tensor, got {getattr(out, "dtype", type(out).__name__)} '
                            f'{tuple(getattr(out, "shape", ()))}')
        if out.device != a.device or b.device != a.device:
            raise ValueError(f'out / b must be on the device of a ({a.device}), got {out.device} / {b.device}')
        if tuple(out.shape) != (m, n):
            raise ValueError(f'out: expected shape {(m, n)}, got {tuple(out.shape)}')
        if m * n and ((n > 1 and out.stride(1) != 1) or (m > 1 and out.stride(0) < n)):
            raise ValueError(f'out: needs unit inner stride and a leading dimension >= {n}, got strides {out.stride()}')
    if bias is not None:
        _chk(bias, name='bias')
        if bias.numel() != n or bias.device != a.device:
            raise ValueError(f'bias: expected {n} values on {a.device}, got {bias.numel()} on {bias.device}')
    ws, ws_bytes = None, 0
    if split_k > 1:
        ws_bytes = int(lib.load().gv_gemm_workspace_bytes(m, n, k, split_k))
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=a.device)
    if a_relu_mask is not None:
        a_relu_mask, ld_mask = _row_major(a_relu_mask, 'a_relu_mask')
        if tuple(a_relu_mask.shape) != tuple(a.shape) or ld_mask != lda:
            raise ValueError('a_relu_mask must have the shape and leading dimension of a')
    entry = 'gv_gemm_bf16' if (precision or GEMM_PRECISION) == 'bf16' else 'gv_gemm_f32'
    live = LIVE_ROWS
    if riders is not None:
        plain = (entry == 'gv_gemm_f32' and b_k_chunks is None and c_tiles is None and not trans_a and split_k <= 1
                 and m > 0 and n > 0 and not (live is not None and a.shape[0] == live[1] and a.device == live[0].device))
        if GEMM_RIDERS and plain and not riders.empty():
            riders.ride((0, 1 if trans_b else 0, m, n, k, ptr(a), lda, ptr(b), ldb, ptr(out), out.stride(0) if m > 1 else n, ptr(bias), act,
                         1 if accumulate else 0, 1, ptr(a_relu_mask), None, 0))
            return out
        riders.flush()
    if (b_k_chunks is not None or c_tiles is not None) and entry == 'gv_gemm_f32':
        if b_k_chunks is not None and (b_k_chunks.dtype != torch.int64 or b_k_chunks.numel() < (n + 63) // 64 or k > 1024 or split_k != 1):
            raise ValueError('b_k_chunks: one int64 word per 64-column tile, k <= 1024, no split-K')
        if c_tiles is not None and (c_tiles.dtype != torch.int64 or c_tiles.numel() * 64 < ((m + 63) // 64) * ((n + 63) // 64)):
            raise ValueError('c_tiles: one bit per 64 x 64 tile of the result')
        rows = live[0] if (live is not None and a.shape[0] == live[1] and a.device == live[0].device) else None
        lib.call('gv_gemm_f32_sparse', 1 if trans_a else 0, 1 if trans_b else 0, m, n, k, ptr(a), lda, ptr(b), ldb, ptr(out),
                 out.stride(0) if m > 1 else n, ptr(bias), act, 1 if accumulate else 0, split_k, ptr(a_relu_mask), ptr(ws),
                 ws_bytes, ptr(rows), ptr(b_k_chunks), ptr(c_tiles), int(getattr(c_tiles, '_gv_wanted', 0)) if c_tiles is not None else 0,
                 lib.stream())
        return out
    if live is not None and entry == 'gv_gemm_f32' and a.shape[0] == live[1] and a.device == live[0].device:
        lib.call('gv_gemm_f32_live_rows', 1 if trans_a else 0, 1 if trans_b else 0, m, n, k, ptr(a), lda, ptr(b), ldb, ptr(out),
                 out.stride(0) if m > 1 else n, ptr(bias), act, 1 if accumulate else 0, split_k, ptr(a_relu_mask), ptr(ws),
                 ws_bytes, ptr(live[0]), lib.stream())
        return out
    lib.call(entry, 1 if trans_a else 0, 1 if trans_b else 0, m, n, k, ptr(a), lda, ptr(b), ldb, ptr(out),
             out.stride(0) if m > 1 else n, ptr(bias), act, 1 if accumulate else 0, split_k, ptr(a_relu_mask), ptr(ws),
             ws_bytes, lib.stream())
    return out


def block_words(mask, kind):
    """Which blocks of a 0/1 matrix hold a non-zero entry, as the int64 words gv_gemm_f32_sparse takes (host-side: one read-back of the
    mask -- build them once per static mask).  ``mask`` (out, in), as a MaskedLinear stores it.
      'fwd'   y = x @ (W * mask)^T : per 64 outputs one word, bit c = inputs 16 c .. 16 c + 15 reach any of them
      'bwd'   g_x = g @ (W * mask) : per 64 inputs one word, bit c = outputs 16 c .. 16 c + 15 depend on any of them
      'tiles' dW = g^T @ x         : bit (i * ceil(in / 64) + j) = the 64 x 64 tile (i, j) of the (out, in) gradient is wanted"""
    import numpy as np
    m = (mask.detach().to('cpu').numpy() != 0)
    o, i = m.shape

    def pad(x, r, c):
        y = np.zeros((-(-x.shape[0] // r) * r, -(-x.shape[1] // c) * c), dtype=bool)
        y[:x.shape[0], :x.shape[1]] = x
        return y
    if kind in ('fwd', 'bwd'):
        mm = m if kind == 'fwd' else m.T                       # rows = the product's columns n, columns = its k
        if mm.shape[1] > 1024:
            return None
        y = pad(mm, 64, 16)
        blk = y.reshape(y.shape[0] // 64, 64, y.shape[1] // 16, 16).any(axis=(1, 3))       # (n tiles, k chunks)
        words = np.zeros(blk.shape[0], dtype=np.uint64)
        for c in range(blk.shape[1]):
            words |= blk[:, c].astype(np.uint64) << np.uint64(c)
    elif kind == 'tiles':
        y = pad(m, 64, 64)
        blk = y.reshape(y.shape[0] // 64, 64, y.shape[1] // 64, 64).any(axis=(1, 3)).reshape(-1)
        words = np.zeros((blk.size + 63) // 64, dtype=np.uint64)
        for b in np.nonzero(blk)[0]:
            words[b >> 6] |= np.uint64(1) << np.uint64(b & 63)
    else:
        raise ValueError(kind)
    out = torch.from_numpy(words.view(np.int64).copy()).to(mask.device)
    if kind == 'tiles':
        out._gv_wanted = int(blk.sum())          # how many tiles are wanted: lets the split-K product launch blocks for those only
    return out


def rank_scores(q, entities, target, bias=None):
    """Raw ranks (0-based, float: x.5 under ties) of ``target[i]`` among all entities under score = q @ entities^T + bias:
    the number of OTHER entities with a strictly larger logit plus HALF the number that tie with it (gv_rank_scores:
    MFMA tiles with a rank-count epilogue; the (m, V) score matrix is never stored).  Logits, not sigmoid outputs: same
    order, no saturation ties.  A NaN target score ranks last."""
    return _rank_scores('gv_rank_scores', q, entities, target, bias, None)[0][0]


def _rank_scores(entry, q, entities, target, bias, filt, cand=None, mc=False):
    """The five ``rank_scores*`` wrappers: the operands' checks, the target, the filter (``filt``: (filt_lo, filt_hi, filt_ent), each
    possibly None; None: the entry takes no filter), the candidate sets (``cand``: (cand, cand_set) or None), the bias, the buffers
    and the call.  ``mc``: q / entities are sample stacks (``_mc_operands``).  Returns (one rank tensor per count the entry takes --
    raw, filtered, raw_constrained, filtered_constrained; None for a filtered one without a filter --, the targets' own values).
    The counts are not cleared here: the entry zeroes every count array it is given, and a row it is not given comes back as None."""
    if mc:
        q, entities, s, m, v, h = _mc_operands(q, entities)
        operands = (ptr(q), h, m * h, ptr(entities), h, v * h, s)
    else:
        q, ld_q, entities, ld_e = _score_operands(q, entities)
        (m, h), v = q.shape, entities.shape[0]
        operands = (ptr(q), ld_q, ptr(entities), ld_e)
    dev = q.device
    # (a wrong number of targets is reported ahead of a missing filter, a target out of range after it)
    if entry == 'gv_rank_scores_filtered' and target.numel() == m and any(t is None for t in filt):
        raise ValueError('rank_scores_filtered needs filt_lo, filt_hi and filt_ent')
    tgt32 = _target_args(target, m, v, dev)
    lo32, hi32, ent32, n_ent = _filter_args(*(filt or (None, None, None)), m, v, dev)
    sets = () if cand is None else _cand_args(*cand, m, v, dev)
    bias = _mc_bias_arg(bias, s, dev) if mc else _bias_arg(bias)
    tgt = torch.empty(max(m, 1), dtype=torch.float32, device=dev)
    counts = torch.empty((1 if filt is None else 2) * (1 if cand is None else 2), max(m, 1), dtype=torch.int32, device=dev)
    given = lo32 is not None
    if m == 0 and mc and cand is not None:      # (an empty stack has no sample stride to give)
        return _ranks(counts, 0, given), tgt[:0]
    filter_args = () if filt is None else (ptr(lo32), ptr(hi32), ptr(ent32), n_ent)
    set_args = () if cand is None else (ptr(sets[0]), sets[1], sets[2], ptr(sets[3]))
    count_args = [ptr(c) if given or i % 2 == 0 else None for i, c in enumerate(counts)]
    lib.call(entry, *operands, ptr(tgt32), ptr(bias), *filter_args, *set_args, ptr(tgt), *count_args, m, v, h, lib.stream())
    return _ranks(counts, m, given), tgt[:m]


def _score_operands(q, entities):
    """The two operands of a DistMult ranking query, row-major and of one width: (q, ld_q, entities, ld_e)."""
    q, ld_q = _row_major(q, 'q')
    entities, ld_e = _row_major(entities, 'entities')
    if q.shape[1] != entities.shape[1]:
        raise ValueError('q / entities width mismatch')
    return q, ld_q, entities, ld_e


def _target_args(target, m, v, device):
    """One target entity per query row, inside [0, v): int32 on the queries' device."""
    target = target.reshape(-1)
    if target.numel() != m:
        raise ValueError('one target per query row')
    if m and (int(target.min()) < 0 or int(target.max()) >= v):
        raise ValueError(f'targets must lie in [0, {v})')
    return target.to(device=device, dtype=torch.int32).contiguous()


def _topk_arg(k):
    k = int(k)
    if not 1 <= k <= TOPK_MAX:
        raise ValueError(f'k must lie in [1, {TOPK_MAX}], got {k}')
    return k


def _bias_arg(bias):
    """The scorers' optional scalar bias as the one-element float32 tensor the entries read."""
    return None if bias is None else _chk(bias.reshape(1).to(torch.float32).contiguous(), name='bias')


def _ranks(counts, m, filt=True):
    """Ranks from a (1, 2 or 4, >= m) buffer of counts 2 #better + #equal: one float tensor per row of the buffer.  The odd rows
    are the filtered counts, which the entries leave unwritten when no filter was given (``filt`` False): None for those."""
    r = counts[:, :m].to(torch.float32) * 0.5
    return tuple(r[i] if filt or i % 2 == 0 else None for i in range(r.shape[0]))


def _filter_args(filt_lo, filt_hi, filt_ent, m, v, device, what='entity', last='filt_ent'):
    """The checks of ``rank_scores_filtered`` on an optional filter: (lo32, hi32, ent32, n_ent), all None / 0 without one.
    ``what`` / ``last``: what the listed ids are and how the caller names their array (the pair queries list relations)."""
    given = [t is not None for t in (filt_lo, filt_hi, filt_ent)]
    if any(given) and not all(given):
        raise ValueError(f'filt_lo, filt_hi and {last} are given together or not at all')
    if not all(given):
        return None, None, None, 0
    filt_lo, filt_hi, filt_ent = filt_lo.reshape(-1), filt_hi.reshape(-1), filt_ent.reshape(-1)
    if filt_lo.numel() != m or filt_hi.numel() != m:
        raise ValueError('one filter range (filt_lo, filt_hi) per query row')
    n_ent = filt_ent.numel()
    if n_ent >= 2 ** 31:
        raise ValueError(f'{last}: more than 2**31 - 1 entries')
    if m and (int(filt_lo.min()) < 0 or int(filt_hi.max()) > n_ent or bool((filt_hi < filt_lo).any())):
        raise ValueError(f'filter ranges must satisfy 0 <= filt_lo <= filt_hi <= {n_ent}')
    if n_ent and (int(filt_ent.min()) < 0 or int(filt_ent.max()) >= v):
        raise ValueError(f'filtered {what} ids must lie in [0, {v})')
    i32 = dict(device=device, dtype=torch.int32)
    ent32 = filt_ent.to(**i32).contiguous() if n_ent else torch.zeros(1, **i32)
    return filt_lo.to(**i32).contiguous(), filt_hi.to(**i32).contiguous(), ent32, n_ent


def rank_scores_filtered(q, entities, target, filt_lo, filt_hi, filt_ent, bias=None):
    """(raw, filtered) ranks of ``target[i]``, both as ``rank_scores`` returns them (0-based floats, x.5 under ties), from one
    launch pair (gv_rank_scores_filtered).  The filtered rank leaves out the candidates ``filt_ent[filt_lo[i]:filt_hi[i]]`` --
    entity ids sorted ascending and unique inside each range (ranking.FilterIndex builds them) -- whatever their score; ranges
    may be empty, may hold the target and may be shared.  The raw rank equals ``rank_scores`` bit for bit."""
    return _rank_scores('gv_rank_scores_filtered', q, entities, target, bias, (filt_lo, filt_hi, filt_ent))[0]


TOPK_MAX = 128      # largest k gv_topk_scores takes


def _topk_operands(q, entities):
    """The shape checks of ``topk_scores`` on its two operands, ahead of any look at their device: (m, v, h)."""
    for name, t in (('q', q), ('entities', entities)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise TypeError(f'{name}: expected a 2-D tensor')
    if q.shape[1] != entities.shape[1]:
        raise ValueError('q / entities width mismatch')
    m, v, h = q.shape[0], entities.shape[0], q.shape[1]
    if v < 1 or h < 1:
        raise ValueError(f'need at least one entity and width >= 1 (v={v}, h={h})')
    return m, v, h


def topk_scores(q, entities, k, bias=None, filt_lo=None, filt_hi=None, filt_ent=None):
    """The ``k`` best entities per query row under ``logit[i, j] = q[i] . entities[j] (+ bias)`` -- the logits ``rank_scores``
    compares, bit for bit -- from one fused launch pair (gv_topk_scores) that never stores the score matrix.  With a filter
    (``filt_lo``, ``filt_hi``, ``filt_ent`` as ``rank_scores_filtered`` takes them) the ids ``filt_ent[filt_lo[i]:filt_hi[i]]``
    are no candidates of row i.  Order: logit descending, equal logits (-0 and +0 alike) by lower id, NaN after everything.
    Returns ``(ids int64 (m, k), logits float32 (m, k))``; rows with fewer than k candidates are padded with id -1, logit -inf.
    Logits are reported with -0 as +0 and every NaN as the one quiet NaN (``ranking.topk_from_scores`` does the same)."""
    return _topk_scores('gv_topk_scores', q, entities, k, bias, (filt_lo, filt_hi, filt_ent))


def _topk_scores(entry, q, entities, k, bias, filt, cand=None, mc=False):
    """The four ``topk_scores*`` wrappers, with ``_rank_scores``' arguments: the checks, the outputs, the workspace and the call.
    Returns (ids int64 (m, k), values float32 (m, k))."""
    if mc:
        q, entities, s, m, v, h = _mc_operands(q, entities)
    else:
        m, v, h = _topk_operands(q, entities)
    k = _topk_arg(k)
    if cand is None:                            # topk_scores reports a bad filter ahead of a CPU tensor, the constrained form after it
        lo32, hi32, ent32, n_ent = _filter_args(*filt, m, v, q.device)
    if mc:
        operands = (ptr(q), h, m * h, ptr(entities), h, v * h, s)
    else:
        q, ld_q = _row_major(q, 'q')
        entities, ld_e = _row_major(entities, 'entities')
        operands = (ptr(q), ld_q, ptr(entities), ld_e)
    dev = q.device
    if cand is not None:
        lo32, hi32, ent32, n_ent = _filter_args(*filt, m, v, dev)
        words, ld_cand, n_sets, set32 = _cand_args(*cand, m, v, dev)
    ids = torch.empty(m, k, dtype=torch.int32, device=dev)
    values = torch.empty(m, k, dtype=torch.float32, device=dev)
    if m == 0:
        return ids.long(), values
    bias = _mc_bias_arg(bias, s, dev) if mc else _bias_arg(bias)
    ws = torch.empty(int(lib.load().gv_topk_scores_workspace_bytes(m, v, k)), dtype=torch.uint8, device=dev)
    set_args = () if cand is None else (ptr(words), ld_cand, n_sets, ptr(set32))
    lib.call(entry, *operands, ptr(bias), ptr(lo32), ptr(hi32), ptr(ent32), n_ent, *set_args, k, ptr(ids), ptr(values), ptr(ws), m, v, h,
             lib.stream())
    return ids.long(), values


def _cand_args(cand, cand_set, m, v, device):
    """A candidate bitmask (``ranking.TypeConstraint.words``: (n_sets, >= ceil(v / 32)) int32 or uint32, entity j = bit j & 31
    of word j >> 5; a view with a longer row stride is taken as it is) and one set id per query row: (words, ld_cand, n_sets,
    set32).  Set ids are NOT range-checked: an id outside [0, n_sets) is the empty set, on the device too."""
    if not isinstance(cand, torch.Tensor) or not cand.is_cuda or cand.device != device:
        raise RuntimeError('cand: the gfx950 path needs a CUDA/ROCm tensor on the queries\' device; there is no CPU fallback')
    if cand.dtype not in (torch.int32, torch.uint32) or cand.dim() != 2:
        raise TypeError(f'cand: expected a 2-D int32 / uint32 bitmask, got {cand.dtype} {tuple(cand.shape)}')
    n_sets, w = cand.shape
    if n_sets < 1 or w < (v + 31) // 32:
        raise ValueError(f'cand: need at least one set and ceil({v} / 32) = {(v + 31) // 32} words per set, got {tuple(cand.shape)}')
    if cand.stride(1) != 1 or (n_sets > 1 and cand.stride(0) < w):
        cand = cand.contiguous()
    cand_set = cand_set.reshape(-1)
    if cand_set.numel() != m:
        raise ValueError('one candidate set id per query row')
    return cand, (cand.stride(0) if n_sets > 1 else w), n_sets, cand_set.to(device=device, dtype=torch.int32).contiguous()


def rank_scores_constrained(q, entities, target, cand, cand_set, filt_lo=None, filt_hi=None, filt_ent=None, bias=None):
    """(raw, filtered, raw_constrained, filtered_constrained) ranks of ``target[i]``, as ``rank_scores_filtered`` returns them,
    from one launch pair (gv_rank_scores_constrained).  The constrained ranks count only the candidates whose bit is set in
    row ``cand_set[i]`` of the bitmask ``cand`` (see ``_cand_args``); the target itself is never counted, member or not, and an
    empty or out-of-range set gives rank 0.  The first two equal ``rank_scores_filtered`` bit for bit.  Without a filter the two
    filtered ranks are None."""
    return _rank_scores('gv_rank_scores_constrained', q, entities, target, bias, (filt_lo, filt_hi, filt_ent), (cand, cand_set))[0]


def topk_scores_constrained(q, entities, k, cand, cand_set, bias=None, filt_lo=None, filt_hi=None, filt_ent=None):
    """``topk_scores`` among the members of a per-query candidate set only (gv_topk_scores_constrained): the candidates of row i
    are the entities whose bit is set in row ``cand_set[i]`` of the bitmask ``cand`` (see ``_cand_args``), less the filter-listed
    ids.  Order, ties, NaN and padding are ``topk_scores``'; a set with fewer than k members pads, an out-of-range set id gives
    an all-padding row."""
    return _topk_scores('gv_topk_scores_constrained', q, entities, k, bias, (filt_lo, filt_hi, filt_ent), (cand, cand_set))


def _entity_topk_operands(ents, emb, w):
    """The shape checks of ``entity_topk_scores`` on its operands, ahead of any look at their device: (m, n, num_rels, h)."""
    for name, t in (('emb', emb), ('w', w)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise TypeError(f'{name}: expected a 2-D tensor')
    if not isinstance(ents, torch.Tensor) or ents.dim() != 1 or ents.is_floating_point() or ents.dtype == torch.bool:
        raise TypeError('ents: expected a 1-D integer tensor of entity ids')
    if emb.shape[1] != w.shape[1]:
        raise ValueError('emb / w width mismatch')
    n, num_rels, h = emb.shape[0], w.shape[0], emb.shape[1]
    if n < 1 or num_rels < 1 or h < 1:
        raise ValueError(f'need at least one entity, one relation and width >= 1 (n={n}, num_rels={num_rels}, h={h})')
    if n * num_rels >= 2 ** 31:
        raise ValueError(f'n * num_rels = {n * num_rels} does not fit 31 bits: a candidate (r, x) is the id r * n + x')
    return ents.numel(), n, num_rels, h


def _entity_topk_args(ents, span, tile, filt, m, n, num_rels, k, id_dtype, device):
    """What the per-entity wrappers do once the operands' shapes and k stand: the checks of ``span`` (``tile``: how the wrapper
    calls a tile), of the query entities' range and of the filter over the N * R keys, then the outputs.  Returns (``_filter_args``'
    tuple, (rel, ent, values), ents32)."""
    if span is not None and int(span) < 1:
        raise ValueError(f'span counts (relation, {tile} tile) pairs per workgroup: at least 1, got {span}')
    if m and (int(ents.min()) < 0 or int(ents.max()) >= n):
        raise ValueError(f'query entities must lie in [0, {n})')
    filt32 = _filter_args(*filt, n * num_rels, n, device)
    outs = tuple(torch.empty(m, k, dtype=t, device=device) for t in (id_dtype, id_dtype, torch.float32))
    return filt32, outs, ents.to(device=device, dtype=torch.int32).contiguous()


def _entity_span_tiles(span, n_tiles):
    """The ``span_tiles`` an entry is handed: 0 is the library's rule, else ``span`` (checked: >= 1) held to the row's tiles."""
    return 0 if span is None else max(1, min(int(span), n_tiles))


def _entity_topk(entry, ents, table, w, k, bias, filt, exclude_self, span, typed=None, mc=False):
    """The four ``entity_topk_scores*`` wrappers, in the style of ``_topk_scores``: the checks in their one order, the outputs, the
    workspace and the call.  ``filt``: (filt_lo, filt_hi, filt_ent); ``typed``: (set_ptr, set_ids, side) for the sweeps over the
    member lists, else None; ``mc``: ``table`` is the (S, N, h) sample stack and ``bias`` holds one value per sample.  Returns (rel
    int64 (m, k), ent int64 (m, k), values float32 (m, k))."""
    if mc:
        s, m, n, num_rels, h = _entity_topk_mc_operands(ents, table, w)
    else:
        m, n, num_rels, h = _entity_topk_operands(ents, table, w)
    k = _topk_arg(k)
    (lo32, hi32, ent32, n_ent), (rel, ent, values), ents32 = _entity_topk_args(
        ents, span, 'column' if typed is None else 'member', filt, m, n, num_rels, k, torch.int32, table.device)
    if mc:
        table, ld_e, e_stride = _mine_sample_stack(table, 'z')
        tables = (ptr(table), ld_e, e_stride, s)
    else:
        table, ld_e = _row_major(table, 'emb')
        tables = (ptr(table), ld_e)
    w, ld_w = _row_major(w, 'w')
    dev = table.device
    if typed is None:
        n_tiles, lists = num_rels * ((n + 63) // 64), ()
        span_tiles = _entity_span_tiles(span, n_tiles)
    else:
        ptr64, ids32, tile_ptr, n_tiles, cand_base, span_tiles = _entity_topk_typed_args(*typed, span, n, num_rels, dev)
        lists = (ptr(ptr64), ptr(ids32), ptr(tile_ptr), n_tiles, cand_base)
    if m == 0:
        return rel.long(), ent.long(), values
    bias = _mc_bias_arg(bias, s, dev) if mc else _bias_arg(bias)
    if typed is not None:
        ws_bytes = int(lib.load().gv_entity_topk_scores_typed_workspace_bytes(m, n_tiles, k, span_tiles))
    elif span_tiles:    # gv_entity_topk_scores_workspace_bytes takes no span_tiles (the ABI stays): a given span's lists are sized here
        ws_bytes = m * ((n_tiles + span_tiles - 1) // span_tiles) * k * 8
    else:
        ws_bytes = int(lib.load().gv_entity_topk_scores_workspace_bytes(m, n, num_rels, k))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    lib.call(entry, ptr(ents32), m, *tables, ptr(w), ld_w, ptr(bias), ptr(lo32), ptr(hi32), ptr(ent32), n_ent, *lists,
             int(bool(exclude_self)), k, span_tiles, ptr(rel), ptr(ent), ptr(values), ptr(ws), ws_bytes, n, num_rels, h, lib.stream())
    return rel.long(), ent.long(), values


def entity_topk_scores(ents, emb, w, k, bias=None, filt_lo=None, filt_hi=None, filt_ent=None, exclude_self=True, span=None):
    """Per-entity completion: for every query entity ``a = ents[i]`` the ``k`` best pairs (r, x) over ALL relations under
    ``logit[i, r, x] = (emb[a] * w[r]) . emb[x] (+ bias)`` -- bit for bit ``gemm(mul(emb[a], w[r]), emb^T, precision='f32') + bias``,
    the logits ``topk_scores`` and ``mine_scores`` select on -- from one fused launch pair (gv_entity_topk_scores) that keeps one
    sorted list per entity while the relations are walked: no (entity x relation) query matrix, no per-relation results.  With
    a filter (one range per key ``a * R + r``, N * R of them: ``ranking._mine_filter`` builds it) the ids
    ``filt_ent[filt_lo[a * R + r]:filt_hi[a * R + r]]`` are no candidates under relation r, nor is ``x == a`` with
    ``exclude_self``.  Order: logit descending (-0 and +0 alike), then relation, then entity ascending; NaN after everything.
    ``ents`` may repeat and need not be sorted.  ``span``: (relation, 64-column tile) pairs per workgroup instead of the library's
    rule -- the result does not depend on it.  Returns ``(rel int64 (m, k), ent int64 (m, k), logits float32 (m, k))``, padded
    with -1 / -1 / -inf past a row's last candidate; -0 is reported as +0 and every NaN as the one quiet NaN."""
    return _entity_topk('gv_entity_topk_scores', ents, emb, w, k, bias, (filt_lo, filt_hi, filt_ent), exclude_self, span)


def _pair_args(table, rels, names, s, o, target, k, filt, p_norm=None, ids_checked=False):
    """What the two pair queries check ahead of any look at a device, in their one order: the operands' shapes, the pairs, k
    (0: no top-k), that something is asked for, the pairs' range, [the norm and the width,] the targets and the filter over the
    relations.  ``ids_checked``: the caller vouches for every id's range (``pair_ids_check``), so the device-to-host reads behind
    those checks are not made; the shapes are still checked.  Returns (m, n, num_rels, h, k, tgt32 or None, ``_filter_args``' tuple)."""
    tname, rname = names
    for name, t in ((tname, table), (rname, rels)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise TypeError(f'{name}: expected a 2-D tensor')
    for name, t in (('s', s), ('o', o)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.is_floating_point() or t.dtype == torch.bool:
            raise TypeError(f'{name}: expected a 1-D integer tensor of entity ids')
    if table.shape[1] != rels.shape[1]:
        raise ValueError(f'{tname} / {rname} width mismatch')
    n, num_rels, h = table.shape[0], rels.shape[0], table.shape[1]
    if n < 1 or num_rels < 1 or h < 1:
        raise ValueError(f'need at least one entity, one relation and width >= 1 (n={n}, num_rels={num_rels}, h={h})')
    m = s.numel()
    if o.numel() != m:
        raise ValueError('one object per subject: s and o are the two columns of the pairs')
    k = int(k)
    if not 0 <= k <= TOPK_MAX:
        raise ValueError(f'k must lie in [0, {TOPK_MAX}] (0: no top-k), got {k}')
    if target is None and k == 0:
        raise ValueError('nothing asked for: give target (ranks), k >= 1 (top-k) or both')
    if m and not ids_checked:
        lo, hi = torch.aminmax(torch.stack((s.long(), o.to(s.device).long())))
        lo, hi = torch.stack((lo, hi)).tolist()                     # (one host round trip for both columns)
        if lo < 0 or hi >= n:
            raise ValueError(f'pair entities must lie in [0, {n})')
    if p_norm is not None:
        _p_norm(p_norm)
        if h > TRANSE_MAX_DIM:
            raise ValueError(f'{tname} / {rname}: width {h} above {TRANSE_MAX_DIM}')
    dev = table.device
    if ids_checked:
        return m, n, num_rels, h, k, _pair_target_unread(target, m, dev), _pair_filter_unread(*filt, m, dev)
    tgt32 = None if target is None else _target_args(target, m, num_rels, dev)
    return m, n, num_rels, h, k, tgt32, _filter_args(*filt, m, num_rels, dev, 'relation', 'filt_rel')


def _pair_target_unread(target, m, device):
    """``_target_args`` without its look at the values."""
    if target is None:
        return None
    target = target.reshape(-1)
    if target.numel() != m:
        raise ValueError('one target per query row')
    return target.to(device=device, dtype=torch.int32).contiguous()


def _pair_filter_unread(filt_lo, filt_hi, filt_rel, m, device):
    """``_filter_args`` without its looks at the values (the kernels clamp every range into the list on their own)."""
    given = [t is not None for t in (filt_lo, filt_hi, filt_rel)]
    if any(given) and not all(given):
        raise ValueError('filt_lo, filt_hi and filt_rel are given together or not at all')
    if not all(given):
        return None, None, None, 0
    filt_lo, filt_hi, filt_rel = filt_lo.reshape(-1), filt_hi.reshape(-1), filt_rel.reshape(-1)
    if filt_lo.numel() != m or filt_hi.numel() != m:
        raise ValueError('one filter range (filt_lo, filt_hi) per query row')
    n_rel = filt_rel.numel()
    if n_rel >= 2 ** 31:
        raise ValueError('filt_rel: more than 2**31 - 1 entries')
    i32 = dict(device=device, dtype=torch.int32)
    rel32 = filt_rel.to(**i32).contiguous() if n_rel else torch.zeros(1, **i32)
    return filt_lo.to(**i32).contiguous(), filt_hi.to(**i32).contiguous(), rel32, n_rel


def pair_ids_check(s, o, target, n, num_rels):
    """The range checks of the pair queries on a whole query set, in ONE device-to-host read: every entity of ``s`` / ``o`` in
    [0, n), every target (when given) in [0, num_rels).  A chunked driver makes it once and passes ``ids_checked=True`` with each
    chunk; a filter built by ``ranking.PairFilterIndex`` for the same sizes is in range by construction."""
    if not s.numel():
        return
    ends = [torch.aminmax(torch.stack((s.long(), o.to(s.device).long())))]
    if target is not None:
        ends.append(torch.aminmax(target.to(s.device).long()))
    ends = torch.stack([x for pair in ends for x in pair]).tolist()
    if ends[0] < 0 or ends[1] >= n:
        raise ValueError(f'pair entities must lie in [0, {n})')
    if target is not None and (ends[2] < 0 or ends[3] >= num_rels):
        raise ValueError(f'targets must lie in [0, {num_rels})')


def _pair_buffers(m, k, ranked, id_dtype, dev, n_counts=2):
    """The outputs of a pair query: (tgt, counts (2, m) -- (4, m) for a constrained one -- or None, ids (m, k), values (m, k))."""
    tgt = torch.empty(max(m, 1), dtype=torch.float32, device=dev) if ranked else None
    counts = torch.empty(n_counts, max(m, 1), dtype=torch.int32, device=dev) if ranked else None
    return tgt, counts, torch.empty(m, k, dtype=id_dtype, device=dev), torch.empty(m, k, dtype=torch.float32, device=dev)


def _pair_cand_args(cand, n, num_rels, device):
    """The relation bitmask of a constrained pair query (``ranking.TypeConstraint.relation_words``: row e the relations entity e
    was subject of, row n + e those it was object of) through ``_cand_args``' type, shape and device checks with v = num_rels;
    the pairs index 2 n rows.  Returns the entries' (cand, ld_cand, n_sets)."""
    words, ld_cand, n_sets, _ = _cand_args(cand, torch.zeros(0, dtype=torch.int32), 0, num_rels, device)
    if n_sets < 2 * n:
        raise ValueError(f'cand: need 2 n = {2 * n} rows (entity e as subject, then as object), got {n_sets}')
    return words, ld_cand, n_sets


def _pair_count_ptrs(counts, given):
    """The count arguments of a pair entry from the (2 or 4, m) buffer: the filtered ones only with a filter and targets."""
    if counts is None:
        return (None,) * 4
    return tuple(ptr(counts[i]) if i < counts.shape[0] and (given or i % 2 == 0) else None for i in range(4))


def _pair_result(counts, m, given, k, ids, values):
    """(ranks, topk): ``(raw, filtered or None)`` as ``rank_scores_filtered`` returns them, or None without targets; ``(ids int64
    (m, k), values float32 (m, k))``, or None with k == 0."""
    return (None if counts is None else _ranks(counts, m, given)), (None if k == 0 else (ids.long(), values))


def pair_relation_scores(emb, w, s, o, *, target=None, k=0, bias=None, filt_lo=None, filt_hi=None, filt_rel=None, cand=None,
                         ids_checked=False):
    """Relation prediction: for every entity pair ``(s[i], o[i])`` the relations under ``logit[i, r] = (emb[s_i] * emb[o_i]) . w[r]
    (+ bias)`` -- bit for bit ``gemm(mul(emb[s], emb[o]), w^T, precision='f32') + bias`` -- from ONE launch without a workspace
    (gv_pair_rel_scores): a workgroup owns 64 pairs and walks every 64-relation tile itself, and the (m, h) product matrix is
    never stored.  With ``target`` (one relation per pair): the 0-based mid-ranks of the target among all relations, raw and --
    with a filter -- with the relations ``filt_rel[filt_lo[i]:filt_hi[i]]`` left out of the count (sorted ascending and unique
    inside each range, ``ranking.PairFilterIndex`` builds them; a listed target is allowed), by the definition, tie rule and NaN
    rule of ``rank_scores_filtered``.  With ``k >= 1``: the k best relations in ``topk_scores``' order (logit descending, equal
    logits by lower id, NaN last), the listed ones left out, padded with id -1 / logit -inf; -0 is reported as +0 and every NaN
    as the one quiet NaN.  Returns ``(ranks, topk)``: ``(raw, filtered or None)`` or None without ``target``; ``(ids int64 (m, k),
    logits float32 (m, k))`` or None with ``k == 0``.  Pair ids outside the table are refused here: the kernel trusts them.
    ``ids_checked=True`` skips the reads behind the range checks of pairs, targets and filter for a caller that has made them
    (``pair_ids_check``: the chunked drivers check a whole query set once).
    ``cand`` (gv_pair_rel_scores_constrained): the relation bitmask ``ranking.TypeConstraint.relation_words`` -- (>= 2 n, >=
    ceil(R / 32)) int32, see ``_pair_cand_args`` -- whose rows ``s[i]`` and ``n + o[i]`` AND to the pair's TYPE-CORRECT relations.
    The ranks become ``(raw, filtered, raw_constrained, filtered_constrained)`` by ``rank_scores_constrained``'s rules (the
    constrained counts take type-correct relations only, the target is never counted, none besides the target gives 0; the first
    two are the unconstrained call's bit for bit) and the list's candidates the type-correct relations less the listed ones.
    Bits at columns >= R are ignored."""
    m, n, num_rels, h, k, tgt32, (lo32, hi32, rel32, n_rel) = _pair_args(emb, w, ('emb', 'w'), s, o, target, k, (filt_lo, filt_hi, filt_rel),
                                                                         ids_checked=ids_checked)
    emb, ld_e = _row_major(emb, 'emb')
    w, ld_w = _row_major(w, 'w')
    dev = emb.device
    if w.device != dev:
        raise ValueError(f'emb on {dev}, w on {w.device}')
    sets = () if cand is None else _pair_cand_args(cand, n, num_rels, dev)
    tgt, counts, ids, values = _pair_buffers(m, k, tgt32 is not None, torch.int32, dev, 2 if cand is None else 4)
    given = lo32 is not None
    if m:
        s32, o32 = (t.to(device=dev, dtype=torch.int32).contiguous() for t in (s, o))
        c = _pair_count_ptrs(counts, given)
        lib.call('gv_pair_rel_scores' if cand is None else 'gv_pair_rel_scores_constrained', ptr(emb), ld_e, n, ptr(w), ld_w, num_rels,
                 ptr(s32), ptr(o32), ptr(tgt32), ptr(_bias_arg(bias)), ptr(lo32), ptr(hi32), ptr(rel32), n_rel,
                 *((ptr(sets[0]),) + sets[1:] if sets else ()), k, ptr(tgt), *c[:4 if sets else 2], ptr(ids), ptr(values), m, h,
                 lib.stream())
    return _pair_result(counts, m, given, k, ids, values)


def pair_relation_scores_mc(z, w, s, o, *, target=None, k=0, bias=None, filt_lo=None, filt_hi=None, filt_rel=None, cand=None,
                            ids_checked=False):
    """``pair_relation_scores`` on the Monte-Carlo posterior predictive of S samples (gv_pair_rel_scores_mc{,_constrained}): ``z``
    (S, N, h) holds one entity table per sample (``KGVAE.posterior_samples``; unit inner stride, row and sample strides are kept
    when they span their rows / table), ``w`` the one relation table, ``bias`` (S,) optionally each draw's flow_log_prob (None: no
    bias).  The value is ``pbar[i, r] = mean_s sigmoid((z_s[s_i] * z_s[o_i]) . w[r] + bias[s])``, summed in ascending sample order
    in registers and ranked / selected once per 64-relation tile: bit for bit what ``rank_scores_mc`` / ``topk_scores_mc`` give
    for ``q = mul(z[:, s], z[:, o])`` against ``w`` repeated per sample.  Ranks are mid-ranks -- pbar saturates, so ties are real
    -- and NaN is never optimistic; the list is padded with -1 / -inf.  ``cand``, the filter and ``ids_checked`` are
    ``pair_relation_scores``'.  Returns ``(ranks, topk, tgt)``: ``tgt`` (m,) the target's own pbar, None without ``target``."""
    if not isinstance(z, torch.Tensor) or z.dim() != 3 or z.shape[0] < 1:
        raise TypeError('z: expected a 3-D (samples, entities, width) tensor with at least one sample')
    n_samples = z.shape[0]
    m, n, num_rels, h, k, tgt32, (lo32, hi32, rel32, n_rel) = _pair_args(z[0], w, ('z', 'w'), s, o, target, k, (filt_lo, filt_hi, filt_rel),
                                                                         ids_checked=ids_checked)
    z, ld_e, e_stride = _mine_sample_stack(z, 'z')
    w, ld_w = _row_major(w, 'w')
    dev = z.device
    if w.device != dev:
        raise ValueError(f'z on {dev}, w on {w.device}')
    sets = () if cand is None else _pair_cand_args(cand, n, num_rels, dev)
    tgt, counts, ids, values = _pair_buffers(m, k, tgt32 is not None, torch.int32, dev, 2 if cand is None else 4)
    given = lo32 is not None
    if m:
        s32, o32 = (t.to(device=dev, dtype=torch.int32).contiguous() for t in (s, o))
        c = _pair_count_ptrs(counts, given)
        lib.call('gv_pair_rel_scores_mc' if cand is None else 'gv_pair_rel_scores_mc_constrained', ptr(z), ld_e, e_stride, n_samples, n,
                 ptr(w), ld_w, num_rels, ptr(s32), ptr(o32), ptr(tgt32), ptr(_mc_bias_arg(bias, n_samples, dev)), ptr(lo32), ptr(hi32),
                 ptr(rel32), n_rel, *((ptr(sets[0]),) + sets[1:] if sets else ()), k, ptr(tgt), *c[:4 if sets else 2], ptr(ids),
                 ptr(values), m, h, lib.stream())
    return _pair_result(counts, m, given, k, ids, values) + (None if tgt is None else tgt[:m],)


def entity_typed_plan(set_ptr, num_rels, side='s'):
    """The columns of the type-constrained per-entity sweeps from the member lists' sizes, with torch ops on ``set_ptr``'s device
    (a CPU tensor works): ``(tile_ptr int32 [R + 1], n_tiles, cand_base)``.  ``side='s'`` (facts (a, r, x)): the candidates of
    relation r are its objects, set ``cand_base + r`` with ``cand_base = 0``; ``side='o'`` (facts (x, r, a)): its subjects,
    ``cand_base = R``.  ``tile_ptr`` is the prefix of ``ceil(|candidates of r| / 64)`` -- a row's columns are the r-major sequence
    of (relation, 64-member tile) pairs -- and ``n_tiles = tile_ptr[R]``, read back with one sync.  2**31 tiles or more:
    ValueError."""
    if side not in ('s', 'o'):
        raise ValueError("side is 's' (the entity as subject: the candidates are objects) or 'o' (as object: subjects)")
    cand_base = 0 if side == 's' else num_rels
    sizes = (set_ptr[1:] - set_ptr[:-1]).to(torch.int64)[cand_base:cand_base + num_rels]
    tile_ptr = torch.zeros(num_rels + 1, dtype=torch.int64, device=set_ptr.device)
    tile_ptr[1:] = torch.cumsum((sizes + 63) // 64, 0)
    n_tiles = int(tile_ptr[-1])
    if n_tiles >= 2 ** 31:
        raise ValueError(f'the candidate lists have {n_tiles} tiles of 64 members, more than 2**31 - 1')
    return tile_ptr.to(torch.int32).contiguous(), n_tiles, cand_base


def _entity_topk_typed_args(set_ptr, set_ids, side, span, n, num_rels, device):
    """What the two typed per-entity wrappers add to ``_entity_topk_args``: the member lists checked (``_mine_typed_members``) and
    on the tables' device, the plan, and ``span`` held to the number of tiles.  Returns (ptr64, ids32, tile_ptr, n_tiles, cand_base,
    span_tiles)."""
    for name, t in (('set_ptr', set_ptr), ('set_ids', set_ids)):
        if not isinstance(t, torch.Tensor) or t.device != device:
            raise RuntimeError(f'{name}: the gfx950 path needs a CUDA/ROCm tensor on the tables\' device; there is no CPU fallback')
    ptr64, ids32 = _mine_typed_members(set_ptr, set_ids, n, num_rels)
    tile_ptr, n_tiles, cand_base = entity_typed_plan(ptr64, num_rels, side)
    if not ids32.numel():
        ids32 = torch.zeros(1, dtype=torch.int32, device=device)
    return ptr64, ids32, tile_ptr, n_tiles, cand_base, _entity_span_tiles(span, n_tiles)


def entity_topk_scores_typed(ents, emb, w, k, set_ptr, set_ids, side='s', bias=None, filt_lo=None, filt_hi=None, filt_ent=None,
                             exclude_self=True, span=None):
    """``entity_topk_scores`` among the TYPE-CORRECT facts only (gv_entity_topk_scores_typed).  The sets are given as lists
    (``set_ptr`` int64 [2 R + 1], ``set_ids``: ``ranking.TypeConstraint.members``, set r = the objects of r, set R + r its
    subjects).  ``side='s'``: the facts (a, r, x) with a among r's subjects and x among its objects -- the filter is the object
    queries'; ``side='o'``: the facts (x, r, a) with a among r's objects and x among its subjects -- the filter is the subject
    queries'.  The logit is ``entity_topk_scores``' either way (the query entity's row carries w[r]), bit for bit, and so are
    order, ties, NaN, -0, padding and the outputs; the filter is independent of the sets.  One fused launch pair walks the
    relations' candidate lists, 64 members a tile, rows gathered through the ids: ``sum_r ceil(|C_r| / 64)`` column tiles per
    64-entity row tile instead of ``R * ceil(N / 64)``.  An entity on the query side of no relation gets an all-padding row.
    ``span``: (relation, 64-member tile) pairs per workgroup instead of the library's rule -- the result does not depend on it."""
    return _entity_topk('gv_entity_topk_scores_typed', ents, emb, w, k, bias, (filt_lo, filt_hi, filt_ent), exclude_self, span,
                        (set_ptr, set_ids, side))


def _mc_operands(q, entities):
    """The two sample stacks of a Monte-Carlo query -- q (S, m, h), entities (S, v, h) -- checked for shape ahead of any look at
    their device, then as contiguous float32: (q, entities, S, m, v, h)."""
    for name, t in (('q', q), ('entities', entities)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise TypeError(f'{name}: expected a 3-D (samples, rows, width) tensor')
    if q.shape[0] != entities.shape[0] or q.shape[0] < 1:
        raise ValueError(f'q / entities need the same number of samples, at least one ({q.shape[0]} vs {entities.shape[0]})')
    if q.shape[2] != entities.shape[2]:
        raise ValueError('q / entities width mismatch')
    (s, m, h), v = q.shape, entities.shape[1]
    if v < 1 or h < 1:
        raise ValueError(f'need at least one entity and width >= 1 (v={v}, h={h})')
    q, entities = _chk(q.contiguous(), name='q'), _chk(entities.contiguous(), name='entities')
    if entities.device != q.device:
        raise ValueError(f'entities must be on the device of q ({q.device}), got {entities.device}')
    return q, entities, s, m, v, h


def _mc_bias_arg(bias, s, device):
    """The MC scorers' optional per-sample bias (each draw's flow_log_prob): float32 (S,) on the queries' device."""
    if bias is None:
        return None
    bias = bias.reshape(-1)
    if bias.numel() != s:
        raise ValueError(f'bias: one value per sample ({s}), got {bias.numel()}')
    return _chk(bias.to(device=device, dtype=torch.float32).contiguous(), name='bias')


def rank_scores_mc(q, entities, target, bias=None, filt_lo=None, filt_hi=None, filt_ent=None):
    """Posterior-predictive ranks from S samples (gv_rank_scores_mc): ``q`` (S, m, h) and ``entities`` (S, v, h) hold one query
    matrix and one entity table per sample, ``bias`` (S,) optionally each draw's flow_log_prob.  The value ranked is
    ``pbar[i, j] = mean_s sigmoid(q[s, i] . entities[s, j] + bias[s])``, never stored; ranks follow ``rank_scores_filtered``'s
    rules (0-based floats, x.5 under ties -- pbar saturates, so ties are real --, NaN never optimistic).  Returns ``(raw,
    filtered, tgt)``: ``filtered`` is None without a filter, ``tgt`` (m,) is the target's own pbar."""
    (raw, filtered), tgt = _rank_scores('gv_rank_scores_mc', q, entities, target, bias, (filt_lo, filt_hi, filt_ent), mc=True)
    return raw, filtered, tgt


def topk_scores_mc(q, entities, k, bias=None, filt_lo=None, filt_hi=None, filt_ent=None):
    """The ``k`` most probable entities per query row under ``rank_scores_mc``'s pbar -- the very values it ranks, bit for bit --
    from one fused launch pair (gv_topk_scores_mc).  Filter, order (pbar descending, ties by lower id, NaN last) and padding (id
    -1, value -inf) are ``topk_scores``'.  Returns ``(ids int64 (m, k), prob_mean float32 (m, k))``."""
    return _topk_scores('gv_topk_scores_mc', q, entities, k, bias, (filt_lo, filt_hi, filt_ent), mc=True)


def rank_scores_mc_constrained(q, entities, target, cand, cand_set, bias=None, filt_lo=None, filt_hi=None, filt_ent=None):
    """The type-constrained protocol on ``rank_scores_mc``'s pbar (gv_rank_scores_mc_constrained): returns ``(raw, filtered,
    raw_constrained, filtered_constrained, tgt)``.  ``raw``, ``filtered`` and ``tgt`` equal ``rank_scores_mc``'s bit for bit; the
    constrained ranks count, on the same pbar, only the members of row ``cand_set[i]`` of the bitmask ``cand`` (see
    ``_cand_args``): the target is never counted, member or not, and an empty or out-of-range set gives rank 0.  Without a filter
    the two filtered ranks are None."""
    ranks, tgt = _rank_scores('gv_rank_scores_mc_constrained', q, entities, target, bias, (filt_lo, filt_hi, filt_ent), (cand, cand_set),
                              mc=True)
    return ranks + (tgt,)


def topk_scores_mc_constrained(q, entities, k, cand, cand_set, bias=None, filt_lo=None, filt_hi=None, filt_ent=None):
    """``topk_scores_mc`` among the members of a per-query candidate set only (gv_topk_scores_mc_constrained): the candidates of
    row i are the entities whose bit is set in row ``cand_set[i]`` of the bitmask ``cand`` (see ``_cand_args``), less the
    filter-listed ids; the values are ``rank_scores_mc_constrained``'s pbar, bit for bit.  A set with fewer than k members pads
    (id -1, value -inf), an out-of-range set id gives an all-padding row.  Returns ``(ids int64 (m, k), prob_mean float32 (m, k))``."""
    return _topk_scores('gv_topk_scores_mc_constrained', q, entities, k, bias, (filt_lo, filt_hi, filt_ent), (cand, cand_set), mc=True)


def _entity_topk_mc_operands(ents, z, w):
    """The shape checks of the Monte-Carlo per-entity wrappers, ahead of any look at the tensors' device: ``z`` an (S, N, h) stack
    with at least one sample, then ``_entity_topk_operands`` on a sample.  Returns (S, m, n, num_rels, h)."""
    if not isinstance(z, torch.Tensor) or z.dim() != 3 or z.shape[0] < 1:
        raise TypeError('z: expected a 3-D (samples, entities, width) tensor with at least one sample')
    return (z.shape[0],) + _entity_topk_operands(ents, z[0], w)


def entity_topk_scores_mc(ents, z, w, k, bias=None, filt_lo=None, filt_hi=None, filt_ent=None, exclude_self=True, span=None):
    """``entity_topk_scores`` on the Monte-Carlo posterior predictive of S samples (gv_entity_topk_scores_mc): ``z`` (S, N, h) holds
    one entity table per sample (unit inner stride; row and sample strides are kept when they span their rows / table), ``w`` the
    one relation table, ``bias`` (S,) optionally each draw's flow_log_prob.  The value selected is
    ``pbar[i, r, x] = mean_s sigmoid((z_s[a] * w[r]) . z_s[x] + bias[s])``, summed in ascending sample order in registers and
    selected once per (relation, column tile): bit for bit the ``prob_mean`` ``topk_scores_mc`` returns for the query
    ``mul(z_s[a], w[r])`` at entity x.  Filter, ``exclude_self``, ``span`` and padding (-1 / -1 / -inf) are ``entity_topk_scores``';
    order: pbar descending, then relation, then entity ascending -- pbar saturates, so candidates whose every sample rounds to
    1.0f are a real tie, broken by (r, x); a NaN in any sample gives NaN, after everything.  Returns ``(rel int64 (m, k), ent int64
    (m, k), prob_mean float32 (m, k))``."""
    return _entity_topk('gv_entity_topk_scores_mc', ents, z, w, k, bias, (filt_lo, filt_hi, filt_ent), exclude_self, span, mc=True)


def entity_topk_scores_typed_mc(ents, z, w, k, set_ptr, set_ids, side='s', bias=None, filt_lo=None, filt_hi=None, filt_ent=None,
                                exclude_self=True, span=None):
    """``entity_topk_scores_mc`` among the TYPE-CORRECT facts only (gv_entity_topk_scores_typed_mc): the member lists, ``side`` and
    ``span`` of ``entity_topk_scores_typed``, the samples, ``bias`` (S,), pbar, order, ties, NaN and padding of
    ``entity_topk_scores_mc`` -- a candidate's pbar is the untyped sweep's, bit for bit.  Returns ``(rel int64 (m, k), ent int64
    (m, k), prob_mean float32 (m, k))``."""
    return _entity_topk('gv_entity_topk_scores_typed_mc', ents, z, w, k, bias, (filt_lo, filt_hi, filt_ent), exclude_self, span,
                        (set_ptr, set_ids, side), mc=True)


def pair_prob_std_mc(q, entities, ids, bias=None):
    """Population standard deviation over the samples of ``sigmoid(q[s, i] . entities[s, ids[i, c]] + bias[s])`` for every
    selected pair (gv_pair_prob_std_mc; two-pass in fp32, the dot a plain fmaf chain): float32 (m, k).  Padding ids (-1) give
    0, one sample gives exactly 0."""
    q, entities, s, m, v, h = _mc_operands(q, entities)
    if not isinstance(ids, torch.Tensor) or ids.dim() != 2 or ids.shape[0] != m or ids.shape[1] < 1:
        raise ValueError(f'ids: expected ({m}, k >= 1) entity ids, one row per query')
    if ids.numel() and int(ids.max()) >= v:
        raise ValueError(f'ids must lie below {v} (negative: padding)')
    k = ids.shape[1]
    std = torch.empty(m, k, dtype=torch.float32, device=q.device)
    if m == 0:
        return std
    bias = _mc_bias_arg(bias, s, q.device)
    ids32 = ids.to(device=q.device, dtype=torch.int32).contiguous()
    lib.call('gv_pair_prob_std_mc', ptr(q), h, m * h, ptr(entities), h, v * h, s, ptr(bias), ptr(ids32), k, ptr(std), m, v, h,
             lib.stream())
    return std


MINE_MAX_RESULTS = 1 << 22     # default cap on the triplets one mining call may return (64 MiB of records)
MINE_LEVELS = ((0, 12), (12, 10), (22, 10))      # (prefix bits, bin bits) of the histogram passes: 12 + 10 + 10 = the whole key


class MineOverflow(RuntimeError):
    """A mining run found more triplets than ``max_results`` allows; ``count`` is how many (nothing is truncated silently)."""

    def __init__(self, count, max_results, what):
        self.count, self.max_results = int(count), int(max_results)
        super().__init__(f'{what}: {self.count} triplets, more than max_results={self.max_results}; raise the threshold or the cap')


def mine_key(x):
    """The ordered 32-bit key of a logit (host mirror of the kernels' sign-flip map): larger key = larger logit, -0 as +0,
    NaN -> 0 (never a candidate)."""
    import struct
    x = float(x)
    if x != x:
        return 0
    u = struct.unpack('<I', struct.pack('<f', x))[0]
    if u == 0x80000000:
        u = 0
    return (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)


def mine_order(triplets, logits, num_nodes, num_rels, ascending=False):
    """Sort mined (triplets int64 (n, 3), logits (n,)) into the rule's total order: logit descending (-0 as +0), then (s, r, o)
    ascending.  ``ascending``: the values are distances, smallest first (gv_transe_mine's order).  Any device."""
    logits = logits.to(torch.float32) + 0.0
    lin = (triplets[:, 0] * num_rels + triplets[:, 1]) * max(num_nodes, 1) + triplets[:, 2]
    order = torch.argsort(lin, stable=True)
    order = order[torch.argsort(logits[order], descending=not ascending, stable=True)]
    return triplets[order], logits[order]


def mine_select(triplets, logits, k, max_results, num_nodes, num_rels, ascending=False):
    """The top-K end of every mining route: from candidates that include everything at or above the K-th logit, the first K in
    the total order and the number at or above the K-th logit's exact value (more than ``max_results`` of those: MineOverflow).
    ``ascending``: distances, the K smallest and the number at or below the K-th."""
    triplets, logits = mine_order(triplets, logits, num_nodes, num_rels, ascending)
    n = logits.numel()
    count = n if n <= k else int((logits <= logits[k - 1]).sum() if ascending else (logits >= logits[k - 1]).sum())
    if count > max_results:
        what = 'at or below the K-th distance' if ascending else 'at or above the K-th logit'
        raise MineOverflow(count, max_results, f'top-{k}: the candidates {what}')
    return triplets[:k], logits[:k], count


def _mine_args(k, threshold, max_results):
    """(k, threshold, max_results) of a mining call, checked: exactly one of k >= 1 and a threshold that is not NaN."""
    if (k is None) == (threshold is None):
        raise ValueError('give exactly one of k and threshold')
    max_results = int(max_results)
    if not 1 <= max_results < 2 ** 31:
        raise ValueError(f'max_results must lie in [1, 2**31), got {max_results}')
    if k is not None:
        k = int(k)
        if k < 1:
            raise ValueError(f'k must be >= 1, got {k}')
    else:
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError('threshold is NaN')
    return k, threshold, max_results


def _mine_tables(a, name_a, b, name_b, prepare=None):
    """The two tables of a mining call, checked: 2-D tensors, each through ``prepare(t, name)`` when the wrapper vets its tables this
    early, of one width."""
    for name, t in ((name_a, a), (name_b, b)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise TypeError(f'{name}: expected a 2-D tensor')
    if prepare is not None:
        a, b = prepare(a, name_a), prepare(b, name_b)
    if a.shape[1] != b.shape[1]:
        raise ValueError(f'{name_a} / {name_b} width mismatch')
    return a, b


def _mine_sizes(n, num_rels, filt_lo, filt_hi, filt_ent, args=None):
    """``N * R`` below 2**31 and the filter given whole or not at all; between the two, where ``mine_scores`` has always made them,
    the checks of ``args`` = (k, threshold, max_results), which are returned checked."""
    if n * num_rels >= 2 ** 31:
        raise ValueError(f'N * R = {n * num_rels} reaches 2**31')
    if args is not None:
        args = _mine_args(*args)
    given = [t is not None for t in (filt_lo, filt_hi, filt_ent)]
    if any(given) and not all(given):
        raise ValueError('filt_lo, filt_hi and filt_ent are given together or not at all')
    return args


def _mine_device(a, name_a, b, name_b):
    """(the device both tables are on, the empty result when there is no entity or else None)"""
    dev = a.device
    if b.device != dev:
        raise ValueError(f'{name_b} must be on the device of {name_a} ({dev})')
    return dev, (None if a.shape[0] else _mine_empty(dev))


def _mine_empty(dev):
    return (torch.zeros(0, 3, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.float32, device=dev),
            {'count': 0, 'passes': 0})


def _mine_filter_args(filt_lo, filt_hi, filt_ent, n, num_rels, dev, workspace_bytes):
    """The filter of a mining call as the kernels take it: (lo32, hi32, ent32, n_ent, workspace, workspace bytes), all None / 0
    without one.  ``workspace_bytes``: the entry point that sizes the re-bucketed filter."""
    if filt_lo is None:
        return None, None, None, 0, None, 0
    filt_lo, filt_hi, filt_ent = filt_lo.reshape(-1), filt_hi.reshape(-1), filt_ent.reshape(-1)
    if filt_lo.numel() != n * num_rels or filt_hi.numel() != n * num_rels:
        raise ValueError('one filter range (filt_lo, filt_hi) per key s * R + r')
    n_ent = filt_ent.numel()
    if n_ent >= 2 ** 31:
        raise ValueError('filt_ent: more than 2**31 - 1 entries')
    if int(filt_lo.min()) < 0 or int(filt_hi.max()) > n_ent or bool((filt_hi < filt_lo).any()):
        raise ValueError(f'filter ranges must satisfy 0 <= filt_lo <= filt_hi <= {n_ent}')
    if n_ent and (int(filt_ent.min()) < 0 or int(filt_ent.max()) >= n):
        raise ValueError(f'filtered entity ids must lie in [0, {n})')
    i32 = dict(device=dev, dtype=torch.int32)
    lo32, hi32 = filt_lo.to(**i32).contiguous(), filt_hi.to(**i32).contiguous()
    ent32 = filt_ent.to(**i32).contiguous() if n_ent else torch.zeros(1, **i32)
    ws_bytes = int(workspace_bytes(n, num_rels, n_ent))
    return lo32, hi32, ent32, n_ent, torch.empty(ws_bytes, dtype=torch.uint8, device=dev), ws_bytes


def _mine_drive(launch, dev, n, num_rels, k, threshold, threshold_key, max_results, ascending, name):
    """What both miners do around their kernel: a threshold run is one emission at ``threshold_key``; top-K walks the histogram
    levels (12 + 10 + 10 key bits) to the key of the K-th best candidate, then emits once.  ``launch(mode, key_min, prefix_bits,
    prefix, bin_bits, out, capacity, words)`` is one pass of the kernel, ``words`` its counter / histogram; a record's fourth
    word is the value (the logit, or the distance when ``ascending``).  Returns ``(triplets, values, info)`` in the rule's order."""
    edge_of = 'at or below the K-th distance' if ascending else 'at or above the K-th logit'
    info = {'count': 0, 'passes': 0}
    words = torch.zeros(1 << MINE_LEVELS[0][1], dtype=torch.int64, device=dev)      # the counter / the histogram
    empty = (torch.zeros(0, 3, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.float32, device=dev))

    def run(mode, key_min=0, prefix_bits=0, prefix=0, bin_bits=1, out=None, capacity=0):
        launch(mode, key_min, prefix_bits, prefix, bin_bits, out, capacity, words)
        info['passes'] += 1

    def emit(key_min, capacity):
        out = torch.empty(max(capacity, 1), 4, dtype=torch.int32, device=dev)
        run(0, key_min=key_min, out=out, capacity=capacity)
        count = int(words[0])
        rec = out[:min(count, capacity)]
        return count, rec[:, :3].long(), rec[:, 3].contiguous().view(torch.float32)

    if k is None:
        count, trip, logits = emit(threshold_key, min(max_results, n * num_rels * n))
        info['count'] = count
        if count > max_results:
            raise MineOverflow(count, max_results, f'threshold {threshold}')
        return mine_order(trip, logits, n, num_rels, ascending) + (info,)

    above, key_min = 0, None          # candidates strictly above the range being narrowed; the emission threshold once known
    prefix = 0
    for prefix_bits, bin_bits in MINE_LEVELS:
        run(1, prefix_bits=prefix_bits, prefix=prefix, bin_bits=bin_bits)
        hist = words[:1 << bin_bits].cpu().numpy()
        total = int(hist.sum())
        if prefix_bits == 0 and total <= k:           # fewer candidates than asked for: all of them
            if total > max_results:
                raise MineOverflow(total, max_results, f'top-{k}: all candidates')
            if total == 0:
                return empty + (info,)
            key_min, edge = 1, total
            break
        tail = hist[::-1].cumsum()[::-1]              # tail[b] = candidates of this range in bins >= b
        b = int((tail >= k - above).nonzero()[0].max())
        prefix = (prefix << bin_bits) | b
        above += int(tail[b]) - int(hist[b])
        edge = above + int(hist[b])                   # what an emission at this bin's lower edge returns
        shift = 32 - prefix_bits - bin_bits
        if edge <= max_results or shift == 0:
            key_min = prefix << shift
            break
    if edge > max_results:            # one exact value holds more candidates than may be returned
        raise MineOverflow(edge, max_results, f'top-{k}: the candidates {edge_of}')
    count, trip, logits = emit(key_min, edge)
    if count != edge:
        raise RuntimeError(f'{name}: the emission pass found {count} candidates where the histograms counted {edge}')
    trip, logits, info['count'] = mine_select(trip, logits, k, max_results, n, num_rels, ascending)
    return trip, logits, info


def mine_scores(emb, w, *, threshold=None, k=None, bias=None, filt_lo=None, filt_hi=None, filt_ent=None, exclude_self=True,
                max_results=MINE_MAX_RESULTS):
    """Mine ALL triplets of a DistMult decoder: ``logit[s, r, o] = (emb[s] * w[r]) . emb[o] (+ bias)``, bit for bit
    ``gemm(mul(emb, w[r]), emb^T, precision='f32') + bias``, over every (s, r, o) -- less the triplets of the filter (key
    ``s * R + r`` -> ``filt_ent[filt_lo[key]:filt_hi[key]]``), less s == o when ``exclude_self``, less NaN logits -- without
    storing a score (gv_mine_scores: a workgroup keeps a subject and an object tile of ``emb`` in LDS and walks the relations).
    ``threshold=t``: every candidate with logit >= t; ``k=K``: the K best.  Order: logit descending (-0 as +0), then (s, r, o).
    Returns ``(triplets int64 (n, 3), logits float32 (n,), info)``; ``info['count']`` is the number of candidates at or above
    the threshold (top-K: at or above the K-th logit), ``info['passes']`` the passes over the N x R x N product.  More than
    ``max_results`` such candidates raise ``MineOverflow`` with the count.  Top-K finds its threshold with up to three
    histogram passes over the ordered key's bits (12 + 10 + 10), then emits once."""
    if (k is None) == (threshold is None):
        raise ValueError('give exactly one of k and threshold')
    return _mine_scores('gv_mine_scores', emb, w, None, threshold, k, bias, filt_lo, filt_hi, filt_ent, exclude_self, max_results)


def _mine_lists(members, multiple, filt, n, num_rels, dev, workspace_bytes):
    """What a sweep's entry point takes besides its tables and the selection, as ``(lists, workspace, held)`` in the C order:
    ``lists`` = ``[set_ptr, set_ids, units, n_units,] filt_lo, filt_hi, filt_ent, n_filt_ent`` (the bracketed four for a typed
    sweep: the checked ``members`` = (set_ptr, set_ids, span) moved to ``dev`` and their unit plan; ``filt`` = (lo, hi, ent)),
    ``workspace`` = ``workspace, workspace_bytes`` for a whole-graph sweep's re-bucketed filter (sized by ``workspace_bytes``),
    () for a typed one.  Both hold raw addresses: ``held`` is the tensors behind them, which the caller keeps until its last
    launch.  None: the typed plan is empty."""
    if members is None:
        lo32, hi32, ent32, n_ent, ws, ws_bytes = _mine_filter_args(*filt, n, num_rels, dev, workspace_bytes)
        held, sets, after = (ws,), (), (ptr(ws), ws_bytes)
    else:
        set_ptr, set_ids = members[0].to(dev), members[1].to(dev)
        units = mine_typed_plan(set_ptr, num_rels, members[2], multiple=multiple)
        if units.shape[0] == 0:
            return None
        lo32, hi32, ent32, n_ent = _mine_typed_filter_args(*filt, n, num_rels, dev)
        held, sets, after = (set_ptr, set_ids, units), (ptr(set_ptr), ptr(set_ids), ptr(units), units.shape[0]), ()
    return sets + (ptr(lo32), ptr(hi32), ptr(ent32), n_ent), after, held + (lo32, hi32, ent32)


def _mine_sample_stack(z, name):
    """The (S, N, h) sample stack of a Monte-Carlo mining call as the kernel reads it: float32 on the GPU with unit inner stride,
    rows ``ld >= h`` apart and samples a stride apart that spans a whole table (kept as given when it already is, else made
    contiguous).  Returns (tensor, ld, sample stride in elements -- 0 for one sample)."""
    if not z.is_cuda:
        raise RuntimeError(f'{name}: the gfx950 path needs a CUDA/ROCm tensor; there is no CPU fallback')
    if z.dtype != torch.float32:
        raise TypeError(f'{name}: expected float32, got {z.dtype}')
    s, n, h = z.shape
    ld = z.stride(1) if n > 1 else h
    if (h > 1 and z.stride(2) != 1) or ld < h or (s > 1 and z.stride(0) < (n - 1) * ld + h):
        z, ld = z.contiguous(), h
    return z, ld, (z.stride(0) if s > 1 else 0)


def _mine_scores(entry, emb, w, members, threshold, k, bias, filt_lo, filt_hi, filt_ent, exclude_self, max_results, mc=False):
    """``mine_scores`` (``members`` None), ``mine_scores_typed`` (``members`` = (set_ptr, set_ids, span)) and, with ``mc``,
    ``mine_scores_typed_mc`` (``emb`` the (S, N, h) sample stack, ``bias`` one value per sample, the threshold a probability):
    one set of checks, one launch; the typed sweeps add their member lists and unit list and read the filter as given, the
    whole-graph one re-buckets it into a workspace."""
    n_samples = None
    if mc:
        if not isinstance(emb, torch.Tensor) or emb.dim() != 3 or emb.shape[0] < 1:
            raise TypeError('z: expected a 3-D (samples, entities, width) tensor with at least one sample')
        n_samples = emb.shape[0]
    _mine_tables(emb[0] if mc else emb, 'z[s]' if mc else 'emb', w, 'w')
    n, num_rels, h = emb.shape[-2], w.shape[0], emb.shape[-1]
    if num_rels < 1 or h < 1:
        raise ValueError(f'need at least one relation and width >= 1 (R={num_rels}, h={h})')
    k, threshold, max_results = _mine_sizes(n, num_rels, filt_lo, filt_hi, filt_ent, args=(k, threshold, max_results))
    if members is not None:
        members = _mine_typed_members(members[0], members[1], n, num_rels) + (members[2],)
    if n_samples is None:
        emb, ld_e = _row_major(emb, 'emb')
        tables = (ld_e,)
    else:
        emb, ld_e, e_stride = _mine_sample_stack(emb, 'z')
        tables = (ld_e, e_stride, n_samples)
    w, ld_w = _row_major(w, 'w')
    dev, nothing = _mine_device(emb if n_samples is None else emb[0], 'emb', w, 'w')
    if nothing is not None:
        return nothing
    lists = _mine_lists(members, 1, (filt_lo, filt_hi, filt_ent), n, num_rels, dev, lib.load().gv_mine_scores_workspace_bytes)
    if lists is None:
        return _mine_empty(dev)
    lists, workspace, _held = lists      # _held: the tensors behind the addresses, alive until this frame returns
    if bias is not None and n_samples is not None:
        bias = _mc_bias_arg(torch.as_tensor(bias).detach(), n_samples, dev)
    elif bias is not None:
        bias = torch.as_tensor(bias, dtype=torch.float32, device=dev) if not isinstance(bias, torch.Tensor) else bias
        bias = _chk(bias.detach().reshape(1).to(torch.float32).contiguous(), name='bias')

    def launch(mode, key_min, prefix_bits, prefix, bin_bits, out, capacity, words):
        lib.call(entry, ptr(emb), *tables, ptr(w), ld_w, ptr(bias), *lists, 1 if exclude_self else 0, mode, key_min, prefix_bits,
                 prefix, bin_bits, ptr(out), capacity, ptr(words), ptr(words), *workspace, n, num_rels, h, lib.stream())

    return _mine_drive(launch, dev, n, num_rels, k, threshold, None if k is not None else mine_key(threshold), max_results, False,
                       entry)


MINE_TYPED_SPAN = 8            # object tiles a unit of the typed sweeps takes at most against one staged subject tile
MINE_TYPED_FILL = 1024         # units wanted before tiles are grouped at all: four workgroups for each of the MI355X's 256 CUs


def mine_typed_plan(ptr, num_rels, span=None, multiple=1):
    """The unit list of the type-constrained sweeps from the member lists' sizes, with torch ops on ``ptr``'s device (a CPU tensor
    works): int32 (U, 4) rows ``(r, subject tile, first object tile, end object tile)`` over 64-member tiles of relation r's
    subject list (set ``num_rels + r``) and object list (set ``r``), every tile pair in exactly one unit.  ``span`` object tiles a
    unit (the last of a row of units fewer); None: ``MINE_TYPED_SPAN`` when that still leaves ``MINE_TYPED_FILL`` units, else as
    many as do, at least ``multiple`` and a multiple of it (the TransE kernel takes four object tiles at a time).  The result of a
    sweep does not depend on it.  More than 2**31 - 1 units: ValueError."""
    sizes = (ptr[1:] - ptr[:-1]).to(torch.int64)
    n_o, n_s = sizes[:num_rels], sizes[num_rels:]
    s_tiles, o_tiles = (n_s + 63) // 64, (n_o + 63) // 64
    if span is None:
        pairs = int((s_tiles * o_tiles).sum())
        span = min(MINE_TYPED_SPAN, max(1, pairs // MINE_TYPED_FILL))
        span = max(multiple, span // multiple * multiple)
    span = int(span)
    if span < 1:
        raise ValueError(f'span must be >= 1, got {span}')
    groups = (o_tiles + span - 1) // span
    per_r = s_tiles * groups
    total = int(per_r.sum())
    if total > 2 ** 31 - 1:
        raise ValueError(f'the type-constrained sweep has {total} units, more than 2**31 - 1')
    rel = torch.repeat_interleave(torch.arange(num_rels, device=ptr.device), per_r)
    local = torch.arange(total, device=ptr.device) - (torch.cumsum(per_r, 0) - per_r)[rel]
    g = groups[rel].clamp(min=1)
    first = (local % g) * span
    units = torch.stack([rel, local // g, first, torch.minimum(first + span, o_tiles[rel])], 1)
    return units.to(torch.int32).contiguous()


def _mine_typed_members(ptr, ids, n, num_rels):
    """The member lists of a typed mining call, checked with torch ops where they are (a bad id would be an out-of-bounds gather, so
    none reaches a launch): ``ptr`` int64 [2 R + 1] from 0, non-decreasing, ending at ``ids.numel()``; every id in [0, n); every
    set strictly ascending (a tile's object ids are searched by bisection).  ValueError otherwise."""
    for name, t in (('ptr', ptr), ('ids', ids)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype not in (torch.int32, torch.int64):
            raise TypeError(f'{name}: expected a 1-D int32 / int64 tensor')
    if ptr.numel() != 2 * num_rels + 1:
        raise ValueError(f'ptr: expected {2 * num_rels + 1} entries (2 R + 1), got {ptr.numel()}')
    if ids.device != ptr.device:
        raise ValueError('ptr and ids must be on one device')
    ptr = ptr.to(torch.int64)
    if int(ptr[0]) != 0 or bool((ptr[1:] < ptr[:-1]).any()) or int(ptr[-1]) != ids.numel():
        raise ValueError(f'ptr must start at 0, be non-decreasing and end at ids.numel() = {ids.numel()}')
    if ids.numel() >= 2 ** 31:
        raise ValueError('ids: more than 2**31 - 1 members')
    if ids.numel():
        if int(ids.min()) < 0 or int(ids.max()) >= n:
            raise ValueError(f'member ids must lie in [0, {n})')
        starts = torch.zeros(ids.numel() + 1, dtype=torch.bool, device=ids.device)
        starts[ptr] = True
        if bool(((ids[1:] <= ids[:-1]) & ~starts[1:-1]).any()):
            raise ValueError('the members of every set must be strictly ascending')
    return ptr.contiguous(), ids.to(torch.int32).contiguous()


def _mine_typed_filter_args(filt_lo, filt_hi, filt_ent, n, num_rels, dev):
    """``_mine_filter_args`` for the typed sweeps, which read the ranges as given and need each key's listed objects ascending."""
    lo32, hi32, ent32, n_ent, _, _ = _mine_filter_args(filt_lo, filt_hi, filt_ent, n, num_rels, dev, lambda *a: 0)
    if n_ent > 1:
        starts = torch.zeros(n_ent + 1, dtype=torch.bool, device=dev)
        starts[lo32.long()] = True
        if bool(((ent32[1:] < ent32[:-1]) & ~starts[1:-1]).any()):
            raise ValueError('the listed objects of every key must be ascending')
    return lo32, hi32, ent32, n_ent


def mine_scores_typed(emb, w, set_ptr, set_ids, *, threshold=None, k=None, bias=None, filt_lo=None, filt_hi=None, filt_ent=None,
                      exclude_self=True, max_results=MINE_MAX_RESULTS, span=None):
    """``mine_scores`` among the TYPE-CORRECT triplets only: ``s`` a member of set ``R + r``, ``o`` a member of set ``r``, the sets
    given as lists (``set_ptr`` int64 [2 R + 1], ``set_ids``: ``ranking.TypeConstraint.members``).  Everything else -- logits bit for bit,
    filter, ``exclude_self``, NaN, order, ``info``, ``MineOverflow`` -- is ``mine_scores``'.  gv_mine_scores_typed walks the
    transposed order: a workgroup takes a relation, a 64-member tile of its subject list and ``span`` tiles of its object list
    (``mine_typed_plan``; the result does not depend on ``span``), rows gathered through the ids.  An empty plan returns the
    empty result without a launch."""
    return _mine_scores('gv_mine_scores_typed', emb, w, (set_ptr, set_ids, span), threshold, k, bias, filt_lo, filt_hi, filt_ent,
                        exclude_self, max_results)


def mine_scores_typed_mc(z, w, set_ptr, set_ids, *, threshold=None, k=None, bias=None, filt_lo=None, filt_hi=None, filt_ent=None,
                         exclude_self=True, max_results=MINE_MAX_RESULTS, span=None):
    """``mine_scores_typed`` on the Monte-Carlo posterior predictive of S samples: ``z`` (S, N, h) holds one entity table per
    sample (unit inner stride; row and sample strides are kept), ``w`` the one relation table, ``bias`` (S,) optionally each
    draw's flow_log_prob.  The value selected is ``pbar[s, r, o] = mean_s sigmoid((z_s[s] * w[r]) . z_s[o] + bias[s])``, summed in
    ascending sample order and never stored: bit for bit the ``prob_mean`` ``topk_scores_mc`` returns for the query
    ``mul(z_s[s], w[r])`` at entity o (gv_mine_scores_typed_mc: the sample loop runs outside a unit's object tiles, one pbar
    accumulator per tile in registers).  ``threshold`` is a PROBABILITY compared with pbar; order: pbar descending, then
    (s, r, o) ascending; a NaN in any sample makes the triplet no candidate.  Member lists, filter, ``exclude_self``, ``span``,
    ``info`` and ``MineOverflow`` are ``mine_scores_typed``'.  pbar saturates: candidates whose every sample rounds to 1.0f
    tie, and when the tie at the K-th value holds more than ``max_results`` candidates the call raises ``MineOverflow`` with the
    count, as the rule says for any tie.  Returns ``(triplets int64 (n, 3), probs float32 (n,), info)``."""
    return _mine_scores('gv_mine_scores_typed_mc', z, w, (set_ptr, set_ids, span), threshold, k, bias, filt_lo, filt_hi, filt_ent,
                        exclude_self, max_results, mc=True)


# ---- per-relation completion: every relation's own K best ---------------------------------------------------------------------------
# (prefix bits, bin bits) of the histogram passes of the two by-relation sweeps.  The whole-graph form flushes its LDS histogram
# after EVERY relation, so it keeps 256 bins (one LDS read per thread and flush: DESIGN.md 4d-3); a typed unit owns one relation and
# keeps the miners' 12 + 10 + 10.
MINE_RELATION_LEVELS = ((0, 8), (8, 8), (16, 8), (24, 8))
MINE_RELATION_TYPED_LEVELS = MINE_LEVELS
MINE_RELATION_HIST_WORDS = 1 << 24      # = MINE_SLOT_HIST_WORDS (csrc/k_mine.h): m << bin_bits histogram words at most


def relation_ids_check(relations, num_rels, device=None):
    """The ``relations`` of a per-relation query as int64 [m] on ``device`` (default: where they are): a 1-D integer list of unique
    ids in [0, num_rels), any order; None: every relation.  Checked with ONE device-to-host read, as ``pair_ids_check``; a repeated
    or out-of-range id is a ValueError, an empty list too."""
    if relations is None:
        return torch.arange(num_rels, dtype=torch.int64, device=device)
    rels = torch.as_tensor(relations, device=device)
    if not rels.numel():
        raise ValueError('relations: expected at least one relation id')
    if rels.dim() != 1 or rels.dtype not in (torch.int32, torch.int64):
        raise TypeError('relations: expected a 1-D int32 / int64 list of relation ids')
    rels = rels.long()
    ordered = torch.sort(rels).values
    lo, hi, repeated = torch.stack((ordered[0], ordered[-1], (ordered[1:] == ordered[:-1]).any().long())).tolist()
    if lo < 0 or hi >= num_rels:
        raise ValueError(f'relation ids must lie in [0, {num_rels})')
    if repeated:
        raise ValueError('relations: a relation id is repeated')
    return rels


def _relation_args(k, m, max_results):
    """(k, max_results, the share of ``max_results`` one relation may return) of a per-relation call: k >= 1, m * k <= max_results."""
    k, max_results = int(k), int(max_results)
    if k < 1:
        raise ValueError(f'k must be >= 1, got {k}')
    if not 1 <= max_results < 2 ** 31:
        raise ValueError(f'max_results must lie in [1, 2**31), got {max_results}')
    if m * k > max_results:
        raise ValueError(f'm * k = {m} * {k} = {m * k} results, more than max_results={max_results}')
    return k, max_results, max_results // m


def _relation_overflow(rel, count, share, m, k, ascending=False):
    edge_of = 'at or below the K-th distance' if ascending else 'at or above the K-th logit'
    return MineOverflow(count, share, f'relation {rel} (one of {m}, each with an equal share of max_results), top-{k}: the candidates '
                                      f'{edge_of}')


def relation_select(slot, s, o, logits, rels, k, n, share, ascending=False):
    """The top-K end of every per-relation route: from candidates ``(slot, s, o, logit)`` that include, for every slot i < m (the
    relation ``rels[i]``), everything at or above its K-th logit, the first K of each slot in ``mine_order``'s order restricted to
    it -- logit descending (-0 as +0), then (s, o) ascending -- as ``(subj int64 (m, k), obj int64 (m, k), logits float32 (m, k),
    count int64 [m])``, short rows padded with -1 / -1 / -inf; ``count[i]`` is the number of slot i's candidates at or above its
    K-th logit's exact value (all of them when it has fewer than K).  A count above ``share`` raises ``MineOverflow`` naming the
    relation.  ``ascending``: the values are distances (the TransE routes) -- smallest first, then (s, o); padding -1 / -1 / +inf;
    ``count[i]`` the candidates at or below the K-th distance's exact value, and the overflow says so.  Any device."""
    m, dev = rels.numel(), logits.device
    logits = logits.to(torch.float32) + 0.0
    order = torch.argsort(s * max(n, 1) + o, stable=True)
    order = order[torch.argsort(logits[order], descending=not ascending, stable=True)]
    order = order[torch.argsort(slot[order], stable=True)]
    slot, s, o, logits = slot[order], s[order], o[order], logits[order]
    sizes = torch.bincount(slot, minlength=m)
    start = torch.cumsum(sizes, 0) - sizes
    rank = torch.arange(slot.numel(), device=dev) - start[slot]
    subj = torch.full((m, k), -1, dtype=torch.int64, device=dev)
    obj = torch.full((m, k), -1, dtype=torch.int64, device=dev)
    best = torch.full((m, k), float('inf' if ascending else '-inf'), dtype=torch.float32, device=dev)
    keep = rank < k
    subj[slot[keep], rank[keep]], obj[slot[keep], rank[keep]], best[slot[keep], rank[keep]] = s[keep], o[keep], logits[keep]
    kth = best[:, k - 1]                                 # the padding value where the slot has fewer than K: everything counts
    within = logits <= kth[slot] if ascending else logits >= kth[slot]
    count = torch.zeros(m, dtype=torch.int64, device=dev).index_add_(0, slot, within.long())
    over = torch.nonzero(count > share).reshape(-1)
    if over.numel():
        i = int(over[0])
        raise _relation_overflow(int(rels[i]), int(count[i]), share, m, k, ascending)
    return subj, obj, best, count


def _mine_drive_by_relation(launch, dev, n, rels, k, share, levels, name, ascending=False):
    """``_mine_drive``'s top-K walk for ALL relations of ``rels`` (int64 [m], unique) at once: each has its own K-th key, found on
    its own histogram.  ``launch(mode, rels32, key_min, prefix_bits, prefix, bin_bits, out, capacity, out_base, words)`` is one
    sweep of the kernel over m slots -- int32 [m] relation ids (-1: the slot sits this pass out), per-slot ``key_min`` / ``prefix``
    (uint32 bit patterns in int32 [m]), ``words`` the counters int64 [m] or the histograms int64 [m << bin_bits], ``out_base`` int64
    [m + 1] the slots' segments of ``out`` (capacity, 4).  After each HIST sweep the (m, bins) histogram is read ONCE; every
    unresolved slot takes the bin that holds its K-th candidate and extends its prefix; a slot is resolved once what an emission
    at that bin's lower edge returns fits its ``share`` of the results (or the key is spent) and sits out the later sweeps.  One
    EMIT sweep follows, the segments an exclusive scan of the edges, each counter checked against its edge; then
    ``relation_select``.  ``levels``: the (prefix bits, bin bits) of the passes.  ``ascending``: a record's fourth word is a distance
    and the keys are those of -d (the TransE sweeps), so the walk is the same and only ``relation_select``'s order, padding and
    count turn round.  Returns (subj, obj, logits, info)."""
    m = rels.numel()
    rel_host = rels.cpu().numpy().astype(np.int64)
    above, prefix = np.zeros(m, np.int64), np.zeros(m, np.int64)
    key_min, edge = np.zeros(m, np.int64), np.zeros(m, np.int64)
    live = np.ones(m, bool)
    info = {'count': torch.zeros(m, dtype=torch.int64, device=dev), 'passes': 0}

    def i32(a, fill=None):                               # uint32 values / ids as the int32 [m] the kernel reads
        a = a if fill is None else np.where(fill, a, -1)
        return torch.from_numpy(a.astype(np.uint32).view(np.int32) if fill is None else a.astype(np.int32)).to(dev)

    for prefix_bits, bin_bits in levels:
        if not live.any():
            break
        bins, shift = 1 << bin_bits, 32 - prefix_bits - bin_bits
        words = torch.zeros(m * bins, dtype=torch.int64, device=dev)
        launch(1, i32(rel_host, live), None, prefix_bits, i32(prefix), bin_bits, None, 0, None, words)
        info['passes'] += 1
        hist = words.view(m, bins).cpu().numpy()
        tail = hist[:, ::-1].cumsum(1)[:, ::-1]          # tail[i, b] = slot i's candidates of its range in bins >= b
        few = live & (tail[:, 0] <= k) if prefix_bits == 0 else np.zeros(m, bool)      # fewer candidates than asked for: all
        edge[few], key_min[few] = tail[few, 0], (tail[few, 0] > 0).astype(np.int64)
        walk = np.nonzero(live & ~few)[0]
        holds = tail[walk] >= (k - above[walk])[:, None]
        if not holds[:, 0].all():
            i = walk[np.argmin(holds[:, 0])]
            raise RuntimeError(f'{name}: relation {rel_host[i]}: a refining pass counted fewer candidates than the level above it')
        b = bins - 1 - np.argmax(holds[:, ::-1], axis=1)                                 # the last bin that still holds the K-th
        prefix[walk] = (prefix[walk] << bin_bits) | b
        above[walk] += tail[walk, b] - hist[walk, b]
        edge[walk] = above[walk] + hist[walk, b]         # what an emission at this bin's lower edge returns
        done = walk[(edge[walk] <= share) | (shift == 0)]
        key_min[done] = prefix[done] << shift
        live[few] = False
        live[done] = False
    over = np.nonzero(edge > share)[0]
    if over.size:                     # one exact value of a relation holds more candidates than it may return
        raise _relation_overflow(rel_host[over[0]], edge[over[0]], share, m, k, ascending)
    out_base = np.concatenate([[0], np.cumsum(edge)])
    total = int(out_base[-1])
    if total == 0:
        empty = torch.zeros(0, dtype=torch.int64, device=dev)
        subj, obj, best, _ = relation_select(empty, empty, empty, torch.zeros(0, device=dev), rels, k, n, share, ascending)
        return subj, obj, best, info
    out = torch.empty(total, 4, dtype=torch.int32, device=dev)
    counters = torch.zeros(m, dtype=torch.int64, device=dev)
    launch(0, i32(rel_host, edge > 0), i32(key_min), 0, None, 1, out, total, torch.from_numpy(out_base).to(dev), counters)
    info['passes'] += 1
    found = counters.cpu().numpy()
    if (found != edge).any():
        i = int(np.nonzero(found != edge)[0][0])
        raise RuntimeError(f'{name}: relation {rel_host[i]}: the emission pass found {found[i]} candidates where the histograms '
                           f'counted {edge[i]}')
    slot = torch.repeat_interleave(torch.arange(m, device=dev), torch.from_numpy(edge).to(dev))
    subj, obj, best, info['count'] = relation_select(slot, out[:, 0].long(), out[:, 2].long(), out[:, 3].contiguous().view(torch.float32),
                                                     rels, k, n, share, ascending)
    return subj, obj, best, info


def _relation_topk(entry, levels, emb, w, k, relations, members, bias, filt_lo, filt_hi, filt_ent, exclude_self, max_results):
    """``relation_topk_scores`` (``members`` None) and ``relation_topk_scores_typed`` (``members`` = (set_ptr, set_ids, span)):
    ``_mine_scores``' checks and operands, the slots, one launch closure, ``_mine_drive_by_relation``."""
    _mine_tables(emb, 'emb', w, 'w')
    n, num_rels, h = emb.shape[0], w.shape[0], emb.shape[1]
    if num_rels < 1 or h < 1:
        raise ValueError(f'need at least one relation and width >= 1 (R={num_rels}, h={h})')
    _mine_sizes(n, num_rels, filt_lo, filt_hi, filt_ent)
    rels = relation_ids_check(relations, num_rels)
    m = rels.numel()
    k, max_results, share = _relation_args(k, m, max_results)
    if (m << max(b for _, b in levels)) > MINE_RELATION_HIST_WORDS:
        raise ValueError(f'{m} relations: more than {MINE_RELATION_HIST_WORDS} histogram words; ask for them in several calls')
    if members is not None:
        members = _mine_typed_members(members[0], members[1], n, num_rels) + (members[2],)
    emb, ld_e = _row_major(emb, 'emb')
    w, ld_w = _row_major(w, 'w')
    dev, nothing = _mine_device(emb, 'emb', w, 'w')
    rels = rels.to(dev)
    info = {'count': torch.zeros(m, dtype=torch.int64, device=dev), 'passes': 0}
    padding = (torch.full((m, k), -1, dtype=torch.int64, device=dev), torch.full((m, k), -1, dtype=torch.int64, device=dev),
               torch.full((m, k), float('-inf'), dtype=torch.float32, device=dev), info)
    if nothing is not None:
        return padding
    if members is None:
        lo32, hi32, ent32, n_ent, ws, ws_bytes = _mine_filter_args(filt_lo, filt_hi, filt_ent, n, num_rels, dev,
                                                                   lib.load().gv_mine_scores_workspace_bytes)
        sets, after = (), (ptr(ws), ws_bytes)
    else:
        set_ptr, set_ids = members[0].to(dev), members[1].to(dev)
        units = relation_typed_plan(set_ptr, num_rels, rels, members[2])
        if units.shape[0] == 0:
            return padding
        lo32, hi32, ent32, n_ent = _mine_typed_filter_args(filt_lo, filt_hi, filt_ent, n, num_rels, dev)
        sets, after = (ptr(set_ptr), ptr(set_ids), ptr(units), units.shape[0]), ()
    if bias is not None:
        bias = torch.as_tensor(bias, dtype=torch.float32, device=dev) if not isinstance(bias, torch.Tensor) else bias
        bias = _chk(bias.detach().reshape(1).to(torch.float32).contiguous(), name='bias')

    def launch(mode, rels32, key_min, prefix_bits, prefix, bin_bits, out, capacity, out_base, words):
        lib.call(entry, ptr(emb), ld_e, ptr(w), ld_w, ptr(bias), *sets, ptr(lo32), ptr(hi32), ptr(ent32), n_ent,
                 1 if exclude_self else 0, mode, ptr(rels32), m, ptr(key_min), prefix_bits, ptr(prefix), bin_bits, ptr(out), capacity,
                 ptr(out_base), ptr(words), ptr(words), *after, n, num_rels, h, lib.stream())

    return _mine_drive_by_relation(launch, dev, n, rels, k, share, levels, entry)


def relation_topk_scores(emb, w, k, *, relations=None, bias=None, filt_lo=None, filt_hi=None, filt_ent=None, exclude_self=True,
                         max_results=MINE_MAX_RESULTS):
    """Every relation's OWN ``k`` best triplets of a DistMult decoder: for each relation r of ``relations`` (unique ids, any order;
    None: all) the k candidates (s, o) of largest ``logit[s, r, o]``, ``mine_scores``' logit bit for bit and its candidates -- all
    (s, o) less the filter's triplets of r, less s == o under ``exclude_self``, less NaN.  ``mine_scores`` walks to ONE key for
    the whole graph, which compares relations by the scale of their ``w`` rows; here the thresholds, prefixes, histograms,
    counters and output segments are per relation (gv_mine_scores_by_relation: the miner's loop order over the chosen relations
    only, a 256-bin histogram flushed per relation), so all lists come out of the same three to five sweeps and a few relations
    cost their share of a sweep.  Returns ``(subj int64 (m, k), obj int64 (m, k), logits float32 (m, k), info)``, row i for
    ``relations[i]`` in ``relation_select``'s order, short rows padded with -1 / -1 / -inf; ``info['count']`` int64 [m] is each
    relation's candidates at or above its K-th logit, ``info['passes']`` the sweeps.  ``m * k <= max_results``; a relation may
    return ``max_results // m`` records, and one whose candidates at or above its K-th logit are more raises ``MineOverflow``
    naming it."""
    return _relation_topk('gv_mine_scores_by_relation', MINE_RELATION_LEVELS, emb, w, k, relations, None, bias, filt_lo, filt_hi,
                          filt_ent, exclude_self, max_results)


def relation_typed_plan(set_ptr, num_rels, rels, span=None, multiple=1):
    """``mine_typed_plan`` for the relations ``rels`` (int64 [m], unique) only, a unit's first word being the SLOT (the index into
    ``rels``) as gv_mine_scores_typed_by_relation reads it; the default span is chosen from the chosen relations' tile pairs, a
    multiple of ``multiple`` (4 for gv_transe_mine_typed_by_relation, which takes four object tiles at a time)."""
    sizes = (set_ptr[1:] - set_ptr[:-1]).to(torch.int64)
    chosen = torch.zeros(num_rels, dtype=torch.bool, device=set_ptr.device)
    chosen[rels.to(set_ptr.device)] = True
    sizes = sizes * torch.cat([chosen, chosen])
    units = mine_typed_plan(torch.cat([sizes.new_zeros(1), torch.cumsum(sizes, 0)]), num_rels, span, multiple=multiple)
    slot_of = torch.full((num_rels,), -1, dtype=torch.int32, device=set_ptr.device)
    slot_of[rels.to(set_ptr.device)] = torch.arange(rels.numel(), dtype=torch.int32, device=set_ptr.device)
    units[:, 0] = slot_of[units[:, 0].long()]
    return units.contiguous()


def relation_topk_scores_typed(emb, w, k, set_ptr, set_ids, *, relations=None, bias=None, filt_lo=None, filt_hi=None, filt_ent=None,
                               exclude_self=True, max_results=MINE_MAX_RESULTS, span=None):
    """``relation_topk_scores`` among the TYPE-CORRECT pairs only: s a member of set ``R + r``, o a member of set ``r``
    (``mine_scores_typed``'s member lists and rule, the same logits bit for bit).  gv_mine_scores_typed_by_relation walks
    ``relation_typed_plan``'s units -- the chosen relations' tiles only; the result does not depend on ``span`` -- and keeps the typed
    miner's 12 + 10 + 10 histogram levels, a unit's workgroup owning one relation.  A relation with an empty subject or object
    list returns an all-padding row."""
    return _relation_topk('gv_mine_scores_typed_by_relation', MINE_RELATION_TYPED_LEVELS, emb, w, k, relations,
                          (set_ptr, set_ids, span), bias, filt_lo, filt_hi, filt_ent, exclude_self, max_results)


def pick_split_k(m_out, n_out, k):
    """Reduction-heavy shapes (weight gradients: small output, K = nodes) need split-K to fill 256 CUs."""
    tiles = ((m_out + 63) // 64) * ((n_out + 63) // 64)
    if tiles >= 256 or k < 2048:
        return 1
    if k >= 65536:      # a MADE's passes stacked: 500 x 500 over 131 k rows 676 us with 16 splits, 635 with 64 (1000 x 500: 1 348 -> 1 221)
        return 64
    return max(1, min(64, 1024 // tiles, k // 256))


def colsum(x, out=None, accumulate=False, relu_mask=None):
    x, ld = _row_major(x, 'x')
    if relu_mask is not None:
        relu_mask, ldm = _row_major(relu_mask, 'relu_mask')
        if tuple(relu_mask.shape) != tuple(x.shape) or ldm != ld:
            raise ValueError('relu_mask must have the shape and leading dimension of x')
    m, n = x.shape
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=x.device)
        accumulate = False
    ws = torch.empty(64 * n, dtype=torch.float32, device=x.device)
    lib.call('gv_colsum', ptr(x), ptr(relu_mask), m, n, ld, ptr(out), ptr(ws), 1 if accumulate else 0, lib.stream())
    return out


def epilogue_fwd(agg, addend, act, keep, keep_scale):
    agg = _chk(agg, name='agg')
    out = torch.empty_like(agg)
    if addend is not None:
        addend = _chk(addend, name='addend')
    lib.call('gv_rgcn_epilogue_fwd', ptr(agg), ptr(addend), act, ptr(keep), float(keep_scale), ptr(out),
             agg.shape[0], agg.shape[1], lib.stream())
    return out


def epilogue_bwd(out, grad_out, act, keep, keep_scale, colsum_out=None, colsum_accumulate=False, riders=None):
    """g = d(act/dropout epilogue); with ``colsum_out`` the same pass also yields the column sums of g (bias grad).
    ``riders`` (RiderBox): the finishing launch of the fused column sums is left in the box (the caller launches it)."""
    grad_out = _chk(grad_out.contiguous(), name='grad_out')
    g = torch.empty_like(grad_out)
    m, n = grad_out.shape
    fused = colsum_out is not None and n % 4 == 0 and n <= 1024
    part = torch.empty(EPILOGUE_COLSUM_SLICES * n, dtype=torch.float32, device=g.device) if fused else None
    lib.call('gv_rgcn_epilogue_bwd', ptr(out), ptr(grad_out), act, ptr(keep), float(keep_scale), ptr(g), m, n, ptr(part),
             lib.stream())
    if fused and riders is not None:
        riders.colsum = (part, n, EPILOGUE_COLSUM_SLICES, colsum_out, bool(colsum_accumulate))
    elif fused:
        lib.call('gv_colsum_finish', ptr(part), n, EPILOGUE_COLSUM_SLICES, ptr(colsum_out), 1 if colsum_accumulate else 0,
                 lib.stream())
    elif colsum_out is not None:
        colsum(g, out=colsum_out, accumulate=colsum_accumulate)
    return g


def axpby(alpha, x, beta=0.0, y=None, a=None):
    x = _chk(x.contiguous(), name='x')
    if y is None:
        y = torch.empty_like(x)
        beta = 0.0
    lib.call('gv_axpby', x.numel(), ptr(a), float(alpha), ptr(x), float(beta), ptr(y), lib.stream())
    return y


def copy_into(dst, src):
    """dst <- src (contiguous fp32, same size) as an ordinary KERNEL.  torch's copy_ / clone / cat of contiguous tensors go through
    hipMemcpyAsync, which a hipGraph records as a memcpy NODE -- and on this stack such a node can replay with stale parameters
    after any other runtime work between two replays ('Memory access fault by GPU'; DESIGN.md, hipGraph hazards).  Nothing on
    a capturable path may copy that way."""
    src = _chk(src.contiguous(), name='src')
    if dst.numel() != src.numel() or not dst.is_contiguous():
        raise ValueError('copy_into: same size, contiguous destination')
    lib.call('gv_axpby', src.numel(), None, 1.0, ptr(src), 0.0, ptr(dst), lib.stream())
    return dst


def copy_of(x):
    return copy_into(torch.empty_like(x, memory_format=torch.contiguous_format), x)


class _CatRows(torch.autograd.Function):
    """torch.cat([a, b], dim=0) of two (rows, d) matrices with kernel copies (see copy_into)."""

    @staticmethod
    def forward(ctx, a, b):
        out = torch.empty(a.shape[0] + b.shape[0], a.shape[1], dtype=torch.float32, device=a.device)
        copy_into(out[:a.shape[0]], a)
        copy_into(out[a.shape[0]:], b)
        ctx.na = a.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        return g[:ctx.na], g[ctx.na:]


def cat_rows(a, b):
    return _CatRows.apply(a, b)


class _SplitRows(torch.autograd.Function):
    """(x[:n], x[n:]) whose backward assembles the gradient with kernel copies: autograd's own SliceBackward is zeros + copy_,
    i.e. a memcpy node in a captured step (see copy_into)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n, ctx.shape = int(n), tuple(x.shape)
        ctx.set_materialize_grads(False)
        return x[:n], x[n:]

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None and gb is None:
            return None, None
        ref = ga if ga is not None else gb
        out = torch.empty(ctx.shape, dtype=ref.dtype, device=ref.device)
        for part, g in ((out[:ctx.n], ga), (out[ctx.n:], gb)):
            if part.numel() == 0:
                continue
            if g is None:
                part.zero_()
            else:
                copy_into(part, g)
        return out, None


def split_rows(x, n):
    """The first ``n`` rows of ``x`` and the rest (differentiable; capturable)."""
    return _SplitRows.apply(x, n)


def mul(a, b):
    a, b = _chk(a.contiguous(), name='a'), _chk(b.contiguous(), name='b')
    out = torch.empty_like(a)
    lib.call('gv_mul', a.numel(), ptr(a), ptr(b), ptr(out), lib.stream())
    return out


def mul_multi(as_, bs, outs=None):
    """[a * b for a, b in zip(as_, bs)] in ONE launch (at most 8 pairs; gv_mul_multi).  ``outs``: per pair a contiguous
    tensor to write into, or None for a new one."""
    as_ = [_chk(a.contiguous(), name='a') for a in as_]
    bs = [_chk(b.contiguous(), name='b') for b in bs]
    outs = [torch.empty_like(a) if (outs is None or outs[i] is None) else outs[i] for i, a in enumerate(as_)]
    k = len(as_)
    tab = lambda ts: (_ct.c_void_p * k)(*[ptr(t) for t in ts])
    ta, tb, to = tab(as_), tab(bs), tab(outs)
    tn = (_ct.c_int64 * k)(*[a.numel() for a in as_])
    lib.call('gv_mul_multi', k, _ct.addressof(ta), _ct.addressof(tb), _ct.addressof(to), _ct.addressof(tn), lib.stream())
    return outs


# ------------------------------------------------------------------------------------------------
# autograd Functions
# ------------------------------------------------------------------------------------------------
# Device RNG: every random draw of a forward pass (dropout keep masks, reparameterisation noise, prior
# noise) comes from ONE launch of a counter-based generator (Philox4x32-10, gv_rng_fill) keyed by
# {seed, tick} held on the device.  The tick advances on the device (folded into the embedding lookup, or
# gv_rng_tick), so a captured hipGraph draws fresh numbers at every replay -- and none of torch's graph-safe
# RNG bookkeeping kernels (seed/offset fills, one generator launch per tensor) are on the path.
RNG_KEEP_MASK, RNG_NORMAL = 0, 1
_rng_streams = _it.count(1)
_rngs = {}


def new_rng_stream():
    """A process-unique stream id; modules take one per random draw site at construction."""
    return next(_rng_streams) & 0xFFFFFFFF


class DeviceRNG:
    def __init__(self, device):
        self.device = torch.device(device)
        self._seed = None
        self.state = torch.zeros(2, dtype=torch.int64, device=self.device)     # {seed, tick}
        self._used = set()          # streams drawn since the last tick
        self._sync_seed()

    def _sync_seed(self):
        seed = torch.initial_seed() & 0x7FFFFFFFFFFFFFFF     # follows torch.manual_seed
        if seed != self._seed:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('torch.manual_seed changed during hipGraph capture')
            self._seed = seed
            self.state.copy_(torch.tensor([seed, 0], dtype=torch.int64))
            self._used.clear()

    def tick(self):
        self._sync_seed()
        lib.call('gv_rng_tick', ptr(self.state), lib.stream())
        self._used.clear()

    def folded_tick(self):
        """The state pointer for a kernel that advances the tick as a side effect (gv_gather_rows_rng_tick)."""
        self._sync_seed()
        self._used.clear()
        return self.state

    def claim(self, jobs):
        """The host side of a fill whose launch comes later on this stream (a rider of the next self-loop product, ops.RiderBox):
        the seed, the "same stream twice within one tick" rule and the buffer checks, at the place where fill would have run."""
        self._sync_seed()
        if any(j[3] in self._used for j in jobs):     # same stream twice within one tick would repeat its numbers
            self.tick()
        for t, kind, _, _ in jobs:
            want = torch.uint8 if kind == RNG_KEEP_MASK else torch.float32
            if t.dtype != want or not t.is_contiguous() or t.device != self.device:
                raise TypeError('rng fill: buffers must be contiguous uint8 (mask) / float32 (normal) on the RNG device')
        self._used.update(j[3] for j in jobs)

    def fill(self, jobs):
        """jobs: [(tensor, kind, drop_p, stream)] -- uint8 tensors for RNG_KEEP_MASK, float32 for RNG_NORMAL."""
        self.claim(jobs)
        self.launch(jobs)

    def launch(self, jobs):
        """The launches of claimed jobs, stand-alone."""
        for i in range(0, len(jobs), 8):
            part = jobs[i:i + 8]
            n = len(part)
            ptrs = (_ct.c_void_p * n)(*[t.data_ptr() for t, _, _, _ in part])
            counts = (_ct.c_int64 * n)(*[t.numel() for t, _, _, _ in part])
            kinds = (_ct.c_int32 * n)(*[k for _, k, _, _ in part])
            ps = (_ct.c_float * n)(*[float(p) for _, _, p, _ in part])
            streams = (_ct.c_uint32 * n)(*[s for _, _, _, s in part])
            lib.call('gv_rng_fill', ptr(self.state), n, ptrs, counts, kinds, ps, streams, lib.stream())


def device_rng(device):
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('the device RNG lives on a ROCm device (no CPU fallback)')
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _rngs:
        _rngs[key] = DeviceRNG(torch.device('cuda', key))
    return _rngs[key]


class _Embedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, ids, tick_rng=None):
        table = _chk(table, name='embedding table')
        ids = _chk(ids.reshape(-1), torch.int64, 'node ids')
        out = torch.empty(ids.numel(), table.shape[1], dtype=torch.float32, device=table.device)
        if tick_rng is not None and ids.numel() > 0:      # the start-of-forward RNG tick rides on this launch
            lib.call('gv_gather_rows_rng_tick', ptr(table), ptr(ids), ptr(out), ids.numel(), table.shape[1],
                     ptr(tick_rng.folded_tick()), lib.stream())
        else:
            lib.call('gv_gather_rows', ptr(table), ptr(ids), ptr(out), ids.numel(), table.shape[1], lib.stream())
        ctx.save_for_backward(ids)
        ctx.shape = tuple(table.shape)
        ctx.direct = _direct(table)
        _stamp_direct(ctx)
        return out

    @staticmethod
    def backward(ctx, g):
        (ids,) = ctx.saved_tensors
        g = _chk(g.contiguous(), name='grad')
        _verify_direct(ctx)
        tgt = ctx.direct
        gt = tgt if tgt is not None else torch.zeros(ctx.shape, dtype=torch.float32, device=g.device)
        lib.call('gv_scatter_add_rows', ptr(g), ptr(ids), ptr(gt), ids.numel(), ctx.shape[1], lib.stream())
        if tgt is not None:
            GRAD_FRESH.discard(tgt.data_ptr())
        return (None if tgt is not None else gt), None, None


class _EmbeddingIdentity(torch.autograd.Function):
    """The lookup when ids == arange(num_rows) (full-graph training, kgvae/link_predict.py:141-147): no gathered copy --
    the output aliases the table -- and no scatter-add in backward: the consuming layer writes the gradient rows straight
    into the table's gradient (``_gv_grad_target`` on the output tells it where), or, failing that, one add."""

    @staticmethod
    def forward(ctx, table, tick_rng):
        ctx.set_materialize_grads(False)
        if tick_rng is not None:
            tick_rng.tick()
        ctx.direct = _direct(table)
        _stamp_direct(ctx)
        return table.detach().view(table.shape)

    @staticmethod
    def backward(ctx, g):
        if g is None:                  # the layer already wrote the rows into the gradient arena
            return None, None
        g = _chk(g.contiguous(), name='grad')
        _verify_direct(ctx)
        tgt = ctx.direct
        if tgt is None:
            return g, None
        lib.call('gv_axpby', g.numel(), None, 1.0, ptr(g), 1.0, ptr(tgt), lib.stream())
        GRAD_FRESH.discard(tgt.data_ptr())
        return None, None


_identity_ids = {}


def _ids_are_identity(table, ids):
    """ids == arange(table rows)?  Decided once per ids tensor (one host synchronisation), cached on identity + version."""
    if ids.numel() != table.shape[0]:
        return False
    key = (ids.data_ptr(), ids._version, ids.numel())
    hit = _identity_ids.get(key)
    if hit is None:
        if len(_identity_ids) > 64:
            _identity_ids.clear()
        # the entry holds the ids tensor: its address cannot be handed to another tensor while the verdict is cached
        hit = _identity_ids[key] = (bool((ids.reshape(-1) == torch.arange(ids.numel(), device=ids.device)).all()), ids)
    return hit[0]


def embedding(table, ids, tick_rng=None, sole_consumer=False):
    """table[ids].  ``sole_consumer``: the caller guarantees that ONE R-GCN layer consumes the result (the encoders' input
    layer): with an identity lookup that layer may then write dL/dx straight into the table's gradient rows."""
    identity = False
    if table.is_cuda and isinstance(ids, torch.Tensor) and ids.is_cuda and ids.dtype == torch.int64:
        if torch.cuda.is_current_stream_capturing():      # no host synchronisation under capture: only a cached verdict counts
            hit = _identity_ids.get((ids.data_ptr(), ids._version, ids.numel()))
            identity = bool(hit and hit[0]) and ids.numel() == table.shape[0]
        else:
            identity = _ids_are_identity(table, ids)
    if identity and sole_consumer:      # the output ALIASES the table: only for the fused layer, which never writes its input
        out = _EmbeddingIdentity.apply(table, tick_rng)
        out._gv_grad_target = _direct(table)
        return out
    return _Embedding.apply(table, ids, tick_rng)      # a real copy, as nn.Embedding returns


# ---- the R-GCN layers' shared pieces: epilogue gradient, self-loop + bias addend, loop-weight and relation-weight gradients,
# the edge norm in a launch's order, the packed bdd weights and the K1 choice of _RelGraphConvBdd
def _epilogue_grad(out, grad_out, act, keep, keep_scale, want_bias, d_b, riders=None):
    """(g, grad_bias): g = dL/d(pre-epilogue rows); with ``want_bias`` the same pass yields the bias gradient (the column sums of
    g), added into the optimiser's arena when the bias has a direct target ``d_b`` (grad_bias is then None)."""
    if not want_bias:
        return epilogue_bwd(out, grad_out, act, keep, keep_scale), None
    grad_bias = d_b if d_b is not None else torch.empty(grad_out.shape[1], dtype=torch.float32, device=grad_out.device)
    g = epilogue_bwd(out, grad_out, act, keep, keep_scale, colsum_out=grad_bias, colsum_accumulate=d_b is not None, riders=riders)
    return g, (None if d_b is not None else grad_bias)


def _gemm_addend(x, loop_weight, h_bias, out_feat, loop_bf=None, riders=None):
    """The forward epilogue's addend: x @ loop_weight + h_bias (on the bf16 dense forms ``loop_bf`` when the caller has them),
    h_bias broadcast to x's rows without a self loop, or None.  ``riders`` (RiderBox): its jobs ride on the fp32 product, and
    are launched stand-alone here on every other branch."""
    if riders is not None and (loop_weight is None or loop_bf is not None):
        riders.flush()
        riders = None
    if loop_weight is not None and loop_bf is not None:
        return dense_bf16(x, loop_bf[0], loop_weight.shape[1], loop_weight.shape[0], bias=h_bias)
    if loop_weight is not None:
        return gemm(x, loop_weight, bias=h_bias, riders=riders)
    if h_bias is not None:
        return h_bias.unsqueeze(0).expand(x.shape[0], out_feat).contiguous()
    return None


def _row_addend(h_bias, loop_rows, n, out_feat):
    """The addend of the integer-id layers: h_bias broadcast to n rows plus the gathered self-loop rows, or either alone, or None."""
    if h_bias is None:
        return loop_rows
    addend = h_bias.unsqueeze(0).expand(n, out_feat).contiguous()
    if loop_rows is not None:
        lib.call('gv_axpby', addend.numel(), None, 1.0, ptr(loop_rows), 1.0, ptr(addend), lib.stream())
    return addend


def _loop_grads(x, g, loop_weight, d_l, want_loop, want_x, loop_bf=None, riders=None):
    """(grad_loop, gx_loop) of the self-loop term x @ loop_weight: the loop weight's gradient x^T g (added into its direct target
    ``d_l`` when there is one, grad_loop then None) and g @ loop_weight^T (on the bf16 form of ``loop_bf`` when given).
    ``riders`` (RiderBox): the backward's finishers ride on the fp32 dL/dx product; without one they are launched here, alone."""
    if riders is not None and (loop_weight is None or not want_x or loop_bf is not None):
        riders.flush()
        riders = None
    if loop_weight is None:
        return None, None
    grad_loop = gx_loop = None
    if want_loop:
        grad_loop = gemm(x, g, trans_a=True, split_k=pick_split_k(x.shape[1], g.shape[1], x.shape[0]), out=d_l,
                         accumulate=d_l is not None)
        if d_l is not None:
            grad_loop = None
    if want_x:
        if loop_bf is not None:
            gx_loop = dense_bf16(g, loop_bf[1], loop_weight.shape[0], loop_weight.shape[1])
        else:
            gx_loop = gemm(g, loop_weight, trans_b=True, riders=riders)
    return grad_loop, gx_loop


def _coef_order(gidx, ridx, coef, side):
    """(coef, coef_idx) of a launch over the by-source ('src') or by-relation ('rel') edge order: on static graphs the edge norm
    cached in that order, read directly; on graphs indexed sync-free (rebuilt per batch) the norm read through the permutation."""
    if gidx.sync_free or coef is None:
        return coef, (gidx.by_src.perm if side == 'src' else ridx.by_rel.perm)
    return (gidx.coef_in_src_order(coef) if side == 'src' else ridx.coef_in_rel_order(coef)), None


def _relation_weight_grad(gidx, ridx, coef, x, g, nb, si, so, d_w):
    """dL/dW of the bdd relation weights (added into the direct target ``d_w`` when there is one: None is returned then)."""
    coef_r, idx_r = _coef_order(gidx, ridx, coef, 'rel')
    grad_w = bdd_grad_weight(ridx.by_rel.seg, ridx.src_by_rel, ridx.dst_by_rel, coef_r, idx_r, x, g, nb, si, so, out=d_w,
                             accumulate=d_w is not None)
    return None if d_w is not None else grad_w


def _bdd_weight_fwd(ctx, weight, nb, si, so, pk, pk_bwd, riders=None):
    """The forward K1 launch's weight operand (lane-packed with ``pk``).  When the backward-x launch packs too (``pk_bwd``) one
    launch writes both layouts and the backward's copy is kept on ctx for _bdd_weight_bwd.  ``riders`` (RiderBox): the packing
    is left in the box -- the layer's self-loop product, launched in front of the K1 launch, carries it."""
    ctx.w_bwd_packed = None
    ctx.w_version = weight._version
    if pk and riders is not None:
        w_fwd = torch.empty_like(weight)
        if pk_bwd:
            ctx.w_bwd_packed = torch.empty_like(weight)
        riders.pack = (weight, nb, si, so, False, w_fwd, ctx.w_bwd_packed)
        return w_fwd
    if pk and pk_bwd:
        w_fwd, ctx.w_bwd_packed = torch.empty_like(weight), torch.empty_like(weight)
        lib.call('gv_rgcn_bdd_pack_weight_pair', ptr(weight), weight.shape[0], nb, si, so, ptr(w_fwd), ptr(ctx.w_bwd_packed),
                 lib.stream())
        return w_fwd
    return pack_weight(weight, nb, si, so, False) if pk else weight


def _bdd_weight_bwd(ctx, weight, nb, so, si):
    """(weight operand, packed) of the backward-x per-row launch: the forward's copy while the weight is unchanged, else packed here."""
    pk = si * so >= 8 and pack_supported(nb, so, si, True)
    if ctx.w_bwd_packed is not None and weight._version == ctx.w_version:
        return ctx.w_bwd_packed, pk
    return (pack_weight(weight, nb, so, si, True) if pk else weight), pk


def _bdd_k1(ctx, side, tl, gidx, ridx, coef, feat, weight, nb, bi, bo, plain_weight, addend, act=ACT_NONE, keep=None,
            keep_scale=1.0, out=None, sharded=False):
    """The K1 launch of _RelGraphConvBdd over one ordering: 'dst' = the forward (``bi`` x ``bo`` = si x so blocks), 'src' = the
    backward w.r.t. x (so x si, transposed).  Precedence: relation phases (``tl``, the caller's PhaseOrder or None) > relation
    groups (decided in the forward: ctx.grouped) > LDS-resident > relation runs > plain.  ``sharded``: the edge-sharded backward,
    which takes the plain kernel (the forward's chunk loop stays with the forward).  ``plain_weight()`` gives the per-row kernels'
    (weight, packed); ``addend()`` is called after any weight packing, in front of the launch.  The forward records the LDS
    launch's operand precision on ctx.k1_bf for its backward."""
    trans, r = side == 'src', weight.shape[0]
    if tl is not None:
        return bdd_aggregate_phases(tl, None if coef is None else tl.coef(coef), feat, pack_weight_phase(tl, weight, nb, bi, bo),
                                    r, nb, bi, bo, addend(), act, keep, keep_scale, out=out)
    seg = gidx.by_src.seg if trans else gidx.by_dst.seg
    nbr, ety = (gidx.nbr_by_src, ridx.et_by_src) if trans else (gidx.nbr_by_dst, ridx.et_by_dst)

    def coef_operands():
        # the LDS and plain launches read the norm differently by direction: the forward in the caller's edge order through
        # by_dst.perm; the backward, on static graphs, from the copy cached in by-source order
        return _coef_order(gidx, ridx, coef, 'src') if trans else (coef, gidx.by_dst.perm)
    # relation groups are decided once, in the forward (ctx.grouped), and the backward follows that decision; the backward asks
    # for the LDS plan at the operand precision its forward chose (ctx.k1_bf), not at the current GEMM precision
    lp = None if (ctx.grouped or sharded) else lds_plan(r, nb, bi, bo, bf=ctx.k1_bf if trans else None)
    if lp is not None and lds_graph(gidx, side, lp[2]):       # few relation types: the whole table resident in LDS (csrc/k_lds.hip)
        if not trans:
            ctx.k1_bf = bool(lp[3])
            if not torch.cuda.is_current_stream_capturing():
                # the backward-x launch's list too, while a host read-back is still allowed: a step captured after this eager forward
                # (a no-grad evaluation pass in front of the training capture) must not find it missing
                lp_b = lds_plan(r, nb, bo, bi, bf=ctx.k1_bf)
                if lp_b is not None:
                    gidx.lds_order('src', lp_b[2])
        c, c_idx = coef_operands()
        return bdd_aggregate_lds(gidx.lds_order(side, lp[2]), nbr, ety, c, c_idx, feat,
                                 pack_weight_lds(weight, nb, bi, bo, trans, lp), r, nb, bi, bo, trans, addend(), act, keep,
                                 keep_scale, out=out, plan=lp)
    w, pk = plain_weight()
    if ctx.grouped:
        seg_g, nbr_g, ety_g, perm = ridx.grouped_order(gidx, side)
        coef_g = None if coef is None else ridx.grouped_coef(coef, side, perm)
        return bdd_aggregate(seg_g, nbr_g, ety_g, coef_g, None, feat, w, nb, bi, bo, trans, addend(), act, keep, keep_scale,
                             out=out, packed=pk)
    if K1_REL_RUNS and not gidx.sync_free and not sharded:
        nbr_r, et_r, _, coef_r = ridx.rel_sorted(gidx, side, coef)      # rows sorted by relation: weight reuse along runs
        return bdd_aggregate(_k1_items(gidx, seg), nbr_r, et_r, coef_r, None, feat, w, nb, bi, bo, trans, addend(), act, keep,
                             keep_scale, out=out, packed=pk)
    c, c_idx = coef_operands()
    return bdd_aggregate(_k1_items(gidx, seg), nbr, ety, c, c_idx, feat, w, nb, bi, bo, trans, addend(), act, keep, keep_scale,
                         out=out, packed=pk)


class _RelGraphConvBdd(torch.autograd.Function):
    """out = keep*scale*act( sum_e norm_e * blockdiag(W_{r_e}) x[src_e]  + x@loop_weight + h_bias ).

    ``reduce_hook`` (multi-GPU edge sharding): a callable that STARTS an in-place sum of a tensor over the
    ranks and returns a handle with ``wait()`` (distributed.make_reduce_hook).  With a hook the raw aggregate
    is kept separate from the epilogue so that it can be all-reduced in between, overlapped with the layer's
    self-loop GEMM; backward all-reduces the gradient of the aggregate the same way, overlapped with the bias /
    loop-weight gradients and the loop GEMM.
    """

    @staticmethod
    def forward(ctx, x, weight, h_bias, loop_weight, norm, gidx, ridx, num_bases, act, keep, keep_scale,
                reduce_hook, link_box=None, riders=None):
        x, _ = _row_major(x, 'x')
        n, in_feat = x.shape
        # a caller that hands over a box runs the one-GPU dynamic-shape step: the backward's finishers may ride as well
        ctx.bwd_riders = riders is not None and reduce_hook is None and not _dist_active()
        if riders is not None and (reduce_hook is not None or loop_weight is None):
            riders.flush()          # edge-sharded: the aggregation precedes the self-loop product; no self loop: no product
            riders = None
        si = in_feat // num_bases
        so = weight.shape[1] // (num_bases * si)
        out_feat = num_bases * so
        coef = None if norm is None else norm.reshape(-1)
        # relation phases (weights staged through LDS once per tile, csrc/k_phase.hip): static single-GPU graphs
        tl = None
        if reduce_hook is None and use_phases(gidx, si, so, False, x.shape[0], in_feat):
            tl = ridx.phase_order(gidx, 'dst', num_bases, si, so)
        # lane-packed weights pay off once a block's weights span >= 32 B (measured: 2x4 / 4x2 blocks -24 % / -19 %,
        # 2x2 blocks +-0): pack per launch kind, a ~1.5 MB pass per layer
        pk = tl is None and si * so >= 8 and pack_supported(num_bases, si, so, False)
        bwd_phases = reduce_hook is None and use_phases(gidx, so, si, True, n, out_feat)
        pk_bwd = not bwd_phases and si * so >= 8 and pack_supported(num_bases, so, si, True)
        w_fwd = _bdd_weight_fwd(ctx, weight, num_bases, si, so, pk, pk_bwd and ctx.needs_input_grad[0], riders)
        ctx.loop_bf = dense_bf16_forms(loop_weight) if (loop_weight is not None and x.shape[0] >= 4096) else None

        def addend():       # (every K1 route calls it once, after its own weight packing and in front of its launch)
            return _gemm_addend(x, loop_weight, h_bias, out_feat, ctx.loop_bf, riders)

        ctx.grouped = tl is None and reduce_hook is None and use_relation_groups(weight, gidx)
        ctx.k1_bf = False
        if reduce_hook is None:
            out = _bdd_k1(ctx, 'dst', tl, gidx, ridx, coef, x, weight, num_bases, si, so, lambda: (w_fwd, pk), addend, act, keep,
                          keep_scale)
        else:
            # edge-sharded: aggregate the destination rows in DIST_FWD_CHUNKS blocks; the all-reduce of block c runs
            # on RCCL's stream while block c+1 is aggregated and, at the end, under the self-loop GEMM
            agg = torch.empty(n, out_feat, dtype=torch.float32, device=x.device)
            pending = []
            for r0, r1, sub in gidx.dst_chunks(DIST_FWD_CHUNKS):
                bdd_aggregate(sub, gidx.nbr_by_dst, ridx.et_by_dst, coef, gidx.by_dst.perm, x, w_fwd, num_bases, si, so,
                              packed=pk, out=agg)
                pending.append(reduce_hook(agg[r0:r1]))
            add = addend()
            for h in pending:
                h.wait()
            out = epilogue_fwd(agg, add, act, keep, keep_scale)
        ctx.save_for_backward(x, weight, loop_weight, coef, out if act == ACT_RELU else None, keep)
        ctx.meta = (gidx, ridx, num_bases, si, so, act, keep_scale, h_bias is not None, reduce_hook)
        ctx.direct = (_direct(weight), _direct(h_bias), _direct(loop_weight))
        _stamp_direct(ctx)
        # x is the embedding table itself (identity lookup) and this layer is its only consumer: dL/dx rows go straight
        # into the table's gradient (zero at this point of the step: the optimiser cleared it, nothing else adds to it)
        tgt = getattr(x, '_gv_grad_target', None)
        ctx.x_grad_target = tgt if (tgt is not None and reduce_hook is None and tuple(tgt.shape) == tuple(x.shape)) else None
        # a caller that knows the output's one consumer asks for the epilogue hand-off (EpilogueLink): no activation, one GPU
        ctx.epi_link = None
        if link_box is not None and act == ACT_NONE and reduce_hook is None:
            ctx.epi_link = link_box[0] = EpilogueLink(keep, keep_scale, h_bias is not None and ctx.needs_input_grad[2],
                                                      ctx.direct[1], out_feat)
            ctx.epi_link.carries_fin = ctx.bwd_riders
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, loop_weight, coef, out, keep = ctx.saved_tensors
        gidx, ridx, nb, si, so, act, keep_scale, has_bias, reduce_hook = ctx.meta
        _verify_direct(ctx)
        d_w, d_b, d_l = ctx.direct
        folded = ctx.epi_link.take(grad_out) if ctx.epi_link is not None else None
        # the finishers that this layer's dL/dx product carries (ops.RiderBox): the KL backward's, left on the link by the
        # reparameterisation's backward, or this layer's own bias column sums; launched in this call either way
        fin_box = ctx.epi_link.take_fin() if ctx.epi_link is not None else None
        if folded is not None:          # the consumer's backward wrote these rows masked and summed the bias gradient
            g, grad_bias = folded
        else:
            if fin_box is None and ctx.bwd_riders and rider_kind('colsum') and LIVE_ROWS is None and d_b is not None:
                fin_box = RiderBox()      # (d_b: an arena slice; a buffer returned to autograd could be read before the product)
            g, grad_bias = _epilogue_grad(out, grad_out, act, keep, keep_scale, has_bias and ctx.needs_input_grad[2], d_b, fin_box)
        if fin_box is not None and fin_box.empty():
            fin_box = None
        ctx.fin_box = fin_box           # (kept for inspection)
        pending = None
        g_agg = g
        if reduce_hook is not None:      # gradient of this rank's partial aggregate = sum over ranks; overlapped below
            g_agg = copy_of(g)
            pending = reduce_hook(g_agg)
        # the layer's two weight gradients (stored straight into the optimiser's arena: nothing in this backward pass reads them)
        # on the side stream, beside the dL/dx path -- where that pays (RGCN_BWD_SIDE)
        side_w = reduce_hook is None and d_l is not None and d_w is not None and loop_weight is not None \
            and ctx.needs_input_grad[3] and ctx.needs_input_grad[1] and rgcn_bwd_side(gidx.num_edges, max(x.shape[1], g.shape[1]))
        if side_w:
            with backward_side(True, x, g, g_agg, weight, coef, rgcn=True):
                gw_first = rgcn_side_gradw_first(gidx.num_edges, x.shape[1])
                if not gw_first:
                    _loop_grads(x, g, loop_weight, d_l, True, False)
                _relation_weight_grad(gidx, ridx, coef, x, g_agg, nb, si, so, d_w)
                if gw_first:
                    _loop_grads(x, g, loop_weight, d_l, True, False)
        # (the loop weight's gradient on this stream, NOT ordered behind the side stream: d_l / d_w are this layer's own arena
        # slices, which no other node of the pass writes -- a wait here serialises the flows' weight-gradient products with the
        # R-GCN backward: WN18RR + 3 IAF 4.9 -> 5.2 ms when it was tried)
        grad_loop, gx_loop = _loop_grads(x, g, loop_weight, d_l, ctx.needs_input_grad[3] and not side_w, ctx.needs_input_grad[0],
                                         ctx.loop_bf, fin_box)
        if fin_box is not None and not fin_box.done:
            raise RuntimeError('_RelGraphConvBdd.backward: the finishers\' RiderBox was dropped (a gradient was never finished)')
        if pending is not None:
            pending.wait()
        grad_x = None
        if ctx.needs_input_grad[0]:
            # dL/dx rows may be stored straight into the embedding table's gradient (identity lookup) -- but only while that
            # buffer is known to be zero (fresh from zero_grad / step); a second backward before the next step, or another
            # lookup of the table whose gradient landed first, must be added to, not erased
            x_tgt = x_add = ctx.x_grad_target
            if x_tgt is not None:
                if x_tgt.data_ptr() in GRAD_FRESH:
                    GRAD_FRESH.discard(x_tgt.data_ptr())
                    x_add = None
                else:
                    x_tgt = None
            tl = None
            if reduce_hook is None and use_phases(gidx, so, si, True, g_agg.shape[0], g_agg.shape[1]):
                tl = ridx.phase_order(gidx, 'src', nb, so, si)
            grad_x = _bdd_k1(ctx, 'src', tl, gidx, ridx, coef, g_agg, weight, nb, so, si,
                             lambda: _bdd_weight_bwd(ctx, weight, nb, so, si), lambda: gx_loop, out=x_tgt,
                             sharded=reduce_hook is not None)
            if x_tgt is not None:
                grad_x = None                                  # written in place
            elif x_add is not None:     # the table's gradient already holds something: add
                lib.call('gv_axpby', grad_x.numel(), None, 1.0, ptr(grad_x), 1.0, ptr(x_add), lib.stream())
                grad_x = None
        grad_w = None
        if ctx.needs_input_grad[1] and not side_w:
            grad_w = _relation_weight_grad(gidx, ridx, coef, x, g_agg, nb, si, so, d_w)
        return grad_x, grad_w, grad_bias, grad_loop, None, None, None, None, None, None, None, None, None, None


K1_REL_RUNS = _os.environ.get('GV_K1_REL_RUNS', '1') == '1'     # static graphs: rows sorted by relation (weight reuse along runs)
REL_GROUPS = _os.environ.get('GV_REL_GROUPS', '0')         # '0' (default: off) | 'auto' | '1'
L2_WEIGHT_BUDGET = 3 << 20                                  # bytes of relation weights one XCD's 4 MiB L2 can keep hot


def use_relation_groups(weight, gidx):
    """Group a row's edges by relation range (RelationIndex.grouped_order) when the weight table overflows an XCD's L2:
    static graphs only (the grouped index is built with host-side sizes).  Opt-in: measured at h = 500 it takes 19 % off
    the 5x10 aggregation launch but is step-neutral, because every row then goes through the fix-up pass."""
    if REL_GROUPS == '0' or gidx.sync_free or gidx.num_edges == 0:
        return False
    return REL_GROUPS == '1' or weight.numel() * 4 > L2_WEIGHT_BUDGET


def rel_graph_conv_bdd(x, weight, h_bias, loop_weight, norm, gidx, ridx, num_bases, act=ACT_NONE, keep=None,
                       keep_scale=1.0, reduce_hook=None, sole_consumer=False, riders=None):
    """``sole_consumer``: the caller hands the output to exactly one node that accepts an EpilogueLink (ops.reparam); the output
    then carries the hand-off (``out._gv_epi_link``) when the layer can offer one.  ``riders``: a RiderBox for the layer's
    self-loop product (launched in this call either way)."""
    if not (sole_consumer and KL_SEAM_FOLD):
        return _RelGraphConvBdd.apply(x, weight, h_bias, loop_weight, norm, gidx, ridx, num_bases, act, keep,
                                      float(keep_scale), reduce_hook, None, riders)
    box = [None]
    out = _RelGraphConvBdd.apply(x, weight, h_bias, loop_weight, norm, gidx, ridx, num_bases, act, keep, float(keep_scale),
                                 reduce_hook, box, riders)
    out._gv_epi_link = box[0]
    return out


def rel_rows_gemm(feat, rows, w3, transpose_w, tiles, n_tiles, n_edges):
    """msg[p] = feat[rows[p]] @ W_r (or W_r^T) for the edges in by-relation order; w3 is (R, in, out)."""
    feat, ld = _row_major(feat, 'feat')
    w3 = _chk(w3, name='dense relation weights')
    r, fin, fout = w3.shape
    msg = torch.empty(n_edges, fin if transpose_w else fout, dtype=torch.float32, device=feat.device)
    lib.call('gv_rel_rows_gemm', ptr(feat), ld, ptr(rows), ptr(w3), r, fin, fout, 1 if transpose_w else 0, ptr(tiles), n_tiles,
             ptr(msg), lib.stream())
    return msg


class _RelGraphConvDense(torch.autograd.Function):
    """RelGraphConv with a full (in x out) matrix per relation -- the `basis` regulariser after W_r = sum_b w_comp[r,b] V_b
    (DGL's basis_message_func).  Messages are relation-grouped f32 MFMA GEMMs with gathered rows
    (gv_rel_rows_gemm, edges in by-relation order); their per-destination sum, x norm, + self loop + bias, activation and
    dropout is the K1 aggregation with 1x1 blocks over the message rows.  Backward: the same two steps transposed for
    dL/dx, one relation-grouped (in x E_r) @ (E_r x out) product per relation for dL/dW."""

    @staticmethod
    def forward(ctx, x, w3, h_bias, loop_weight, norm, gidx, ridx, act, keep, keep_scale):
        x, _ = _row_major(x, 'x')
        fin = x.shape[1]
        r, fin_w, fout = w3.shape
        if fin_w != fin:
            raise ValueError(f'dense relation weights are {tuple(w3.shape)}, x has {fin} columns')
        coef = None if norm is None else norm.reshape(-1)
        tiles, n_tiles, pos_d, pos_s, zeros = ridx.dense_plan(gidx)
        addend = _gemm_addend(x, loop_weight, h_bias, fout)
        msg = rel_rows_gemm(x, ridx.src_by_rel, w3, False, tiles, n_tiles, gidx.num_edges)
        ones = torch.ones(1, fout, dtype=torch.float32, device=x.device)
        out = bdd_aggregate(gidx.by_dst.seg, pos_d, zeros, coef, gidx.by_dst.perm, msg, ones, fout, 1, 1, False, addend, act,
                            keep, keep_scale)
        ctx.save_for_backward(x, w3, loop_weight, coef, out if act == ACT_RELU else None, keep)
        ctx.meta = (gidx, ridx, act, keep_scale, h_bias is not None)
        ctx.direct = (_direct(h_bias), _direct(loop_weight))
        _stamp_direct(ctx)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, w3, loop_weight, coef, out, keep = ctx.saved_tensors
        gidx, ridx, act, keep_scale, has_bias = ctx.meta
        _verify_direct(ctx)
        d_b, d_l = ctx.direct
        r, fin, fout = w3.shape
        tiles, n_tiles, pos_d, pos_s, zeros = ridx.dense_plan(gidx)
        grad_x = grad_w = None
        g, grad_bias = _epilogue_grad(out, grad_out, act, keep, keep_scale, has_bias and ctx.needs_input_grad[2], d_b)
        grad_loop, gx_loop = _loop_grads(x, g, loop_weight, d_l, ctx.needs_input_grad[3], ctx.needs_input_grad[0])
        if ctx.needs_input_grad[0]:
            msg2 = rel_rows_gemm(g, ridx.dst_by_rel, w3, True, tiles, n_tiles, gidx.num_edges)
            ones = torch.ones(1, fin, dtype=torch.float32, device=x.device)
            coef_s, idx_s = (gidx.coef_in_src_order(coef), None) if coef is not None else (None, None)
            grad_x = bdd_aggregate(gidx.by_src.seg, pos_s, zeros, coef_s, idx_s, msg2, ones, fin, 1, 1, False, gx_loop)
        if ctx.needs_input_grad[1]:
            g2, ld_g = _row_major(g, 'g')
            grad_w = torch.empty_like(w3)
            scale = ridx.coef_in_rel_order(coef) if coef is not None else None
            lib.call('gv_rel_gradw_gemm', ptr(x), x.stride(0), ptr(ridx.src_by_rel), ptr(g2), ld_g, ptr(ridx.dst_by_rel),
                     ptr(scale), ptr(ridx.by_rel.seg.rowptr), r, fin, fout, ptr(grad_w), lib.stream())
        return grad_x, grad_w, grad_bias, grad_loop, None, None, None, None, None, None


class _RelGraphConvSelect(torch.autograd.Function):
    """RelGraphConv('basis') on INTEGER-ID node features (the one-hot input layer of kgvae/entity_classify.py:25-34, :63;
    DGL utils.bmm_maybe_select): a message is ROW (etype, id[src]) of the relation's (in x out) matrix, no product --

        out[v] = keep*scale*act( sum_{e: dst=v} norm_e * W[etype_e * in + id[src_e], :]  +  loop_rows[v] + h_bias )

    Forward = the K1 aggregation with 1x1 blocks gathering rows of W (R*in, out) through a per-edge row index; backward
    w.r.t. W = the same aggregation over the transposed incidence (destination = W row, source = node row of dL/dh), a
    rectangular graph index built once per (graph, ids); ``loop_rows`` = loop_weight[id] comes in through ops.embedding,
    whose backward scatter-adds its gradient."""

    @staticmethod
    def forward(ctx, wflat, loop_rows, h_bias, norm, gidx, plan, act, keep, keep_scale):
        wflat, _ = _row_major(wflat, 'relation rows')
        n, fout = gidx.num_nodes, wflat.shape[1]
        coef = None if norm is None else norm.reshape(-1)
        addend = _row_addend(h_bias, None if loop_rows is None else _chk(loop_rows.contiguous(), name='loop rows'), n, fout)
        ones = torch.ones(1, fout, dtype=torch.float32, device=wflat.device)
        out = bdd_aggregate(gidx.by_dst.seg, plan['row_by_dst'], plan['zeros'], coef, gidx.by_dst.perm, wflat, ones, fout, 1, 1,
                            False, addend, act, keep, keep_scale)
        ctx.save_for_backward(coef, out if act == ACT_RELU else None, keep)
        ctx.meta = (plan, act, keep_scale, h_bias is not None, loop_rows is not None, tuple(wflat.shape))
        ctx.direct_b = _direct(h_bias)
        _stamp_direct(ctx)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        coef, out, keep = ctx.saved_tensors
        plan, act, keep_scale, has_bias, has_loop, wshape = ctx.meta
        _verify_direct(ctx)
        g, grad_bias = _epilogue_grad(out, grad_out, act, keep, keep_scale, has_bias and ctx.needs_input_grad[2], ctx.direct_b)
        grad_w = None
        if ctx.needs_input_grad[0]:
            gi = plan['by_row']                      # destinations = rows of W, sources = node rows of g
            ones = torch.ones(1, wshape[1], dtype=torch.float32, device=g.device)
            coef_r = None if coef is None else coef[plan['edge_of_by_row']].contiguous()
            grad_w = bdd_aggregate(gi.by_dst.seg, gi.nbr_by_dst, plan['zeros'], coef_r, None, g, ones, wshape[1], 1, 1)
        return grad_w, (g if has_loop else None), grad_bias, None, None, None, None, None, None


def select_plan(gidx, ridx, ids, in_feat):
    """Index of the row-select layer, once per (graph, relation types, ids): the W row of every edge in by-destination
    order, and the rectangular graph (W row <- destination node) of its weight gradient."""
    cache = ridx.__dict__.setdefault('_select', {})
    key = (ids.data_ptr(), ids._version, ids.numel(), int(in_feat))
    hit = cache.get(key)
    if hit is None:
        ids = ids.reshape(-1)
        if ids.numel() != gidx.num_src_nodes:
            raise ValueError(f'{ids.numel()} node ids for a graph of {gidx.num_src_nodes} nodes')
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= in_feat):
            raise ValueError(f'integer node features must lie in [0, in_feat = {in_feat})')
        et = ridx.keepalive.reshape(-1).to(torch.int64)
        row = et * in_feat + ids[gidx.src32.long()]                         # caller's edge order
        if int(ridx.num_rels) * int(in_feat) >= 2 ** 31:
            raise ValueError('num_rels * in_feat must fit int32')
        perm_d = gidx.by_dst.perm
        row_by_dst = (row if perm_d is None else row[perm_d.long()]).to(torch.int32).contiguous()
        # weight gradient: a graph whose destinations are W rows and whose sources are the edges' destination NODES
        by_row = GraphIndex(gidx.dst32.long(), row, int(ridx.num_rels) * int(in_feat), num_src_nodes=gidx.num_nodes)
        edge_of = torch.arange(gidx.num_edges, device=gidx.device) if by_row.by_dst.perm is None else by_row.by_dst.perm.long()
        hit = cache[key] = dict(row_by_dst=row_by_dst, by_row=by_row, edge_of_by_row=edge_of,
                                zeros=torch.zeros(max(gidx.num_edges, 1), dtype=torch.int32, device=gidx.device), keep=ids)
    return hit


def check_select_weight_size(num_rels, in_feat, out_feat):
    """The materialised integer-id path (W of num_rels x in_feat x out_feat elements, its gradient the same) is held to
    2^31 elements: past that it was measured to train a different model (NOTES.md, entity classification at the AM size).
    A basis layer with num_bases < num_rels takes the fused path instead (RelGraphConv.fused_basis_select)."""
    if int(num_rels) * int(in_feat) * int(out_feat) >= 2 ** 31:
        raise ValueError(f'the materialised basis weight would have {num_rels} x {in_feat} x {out_feat} >= 2^31 elements; '
                         'use the fused basis select layer (RelGraphConv.fused_basis_select, num_bases < num_rels)')


def rel_graph_conv_select(ids, w3, h_bias, loop_weight, norm, gidx, ridx, act=ACT_NONE, keep=None, keep_scale=1.0):
    """RelGraphConv('basis') with integer-id features: w3 is (R, in, out), ids int64 (N,)."""
    r, fin, fout = w3.shape
    check_select_weight_size(r, fin, fout)
    plan = select_plan(gidx, ridx, ids, fin)
    loop_rows = embedding(loop_weight, ids.reshape(-1)) if loop_weight is not None else None
    return _RelGraphConvSelect.apply(w3.reshape(r * fin, fout), loop_rows, h_bias, norm, gidx, plan, act, keep, float(keep_scale))


def rel_graph_conv_dense(x, w3, h_bias, loop_weight, norm, gidx, ridx, act=ACT_NONE, keep=None, keep_scale=1.0):
    return _RelGraphConvDense.apply(x, w3, h_bias, loop_weight, norm, gidx, ridx, act, keep, float(keep_scale))


# ------------------------------------------------------------------------------------------------
# entity classification (kgvae/entity_classify.py): the basis integer-id input layer without W, and the softmax / CE head
class _RelGraphConvBasisSelect(torch.autograd.Function):
    """RelGraphConv('basis', num_bases < num_rels) on INTEGER-ID node features without forming W = w_comp @ V, which is
    (R, rows, out) -- 17.7 GB at the AM dataset's size.  An edge's message is row id[src] of W_etype; the edges that share an
    (id, relation) pair -- a run -- share that row, so gv_ec_basis_rows_fwd makes it once per run from the nb basis planes and the
    1x1-block K1 aggregation sums the runs' rows into the destinations (x norm, + loop row + bias, activation, dropout), as
    _RelGraphConvSelect does over the rows of a materialised W.  Backward: S = the same aggregation over the run <- destination
    incidence, then gv_ec_basis_rows_bwd gives dV (only the ids that occur), and dcomp by relation in a fixed order; the
    self-loop rows loop_weight[id] come back through the same aggregation over the id <- node incidence (not the embedding's
    scatter-add: repeated ids would add in arrival order).  Every gradient has the same bits on every run."""

    @staticmethod
    def forward(ctx, v, comp, loop_weight, h_bias, norm, gidx, plan, act, keep, keep_scale):
        v, comp = _chk(v, name='basis weight'), _chk(comp, name='w_comp')
        nb, rows, fout = v.shape
        r = comp.shape[0]
        if comp.shape[1] != nb or r != plan['num_rels']:
            raise ValueError(f'w_comp is {tuple(comp.shape)}, expected ({plan["num_rels"]}, {nb})')
        n = gidx.num_nodes
        coef = None if norm is None else norm.reshape(-1)
        n_runs = plan['n_runs']
        msg = torch.empty(max(n_runs, 1), fout, dtype=torch.float32, device=v.device)
        lib.call('gv_ec_basis_rows_fwd', ptr(v), ptr(comp), ptr(plan['run_id']), ptr(plan['run_rel']), n_runs, fout, nb, r, rows,
                 ptr(msg), lib.stream(), tag='ec_basis_fwd')
        loop_rows = None
        if loop_weight is not None:
            loop_weight = _chk(loop_weight, name='loop_weight')
            if tuple(loop_weight.shape) != (rows, fout):
                raise ValueError(f'loop_weight is {tuple(loop_weight.shape)}, expected ({rows}, {fout})')
            loop_rows = torch.empty(n, fout, dtype=torch.float32, device=v.device)
            lib.call('gv_gather_rows', ptr(loop_weight), ptr(plan['ids']), ptr(loop_rows), n, fout, lib.stream())
        addend = _row_addend(h_bias, loop_rows, n, fout)
        ones = torch.ones(1, fout, dtype=torch.float32, device=v.device)
        out = bdd_aggregate(gidx.by_dst.seg, plan['run_by_dst'], plan['zeros'], coef, gidx.by_dst.perm, msg, ones, fout, 1, 1,
                            False, addend, act, keep, keep_scale)
        ctx.save_for_backward(v, comp, coef, out if act == ACT_RELU else None, keep)
        ctx.meta = (plan, act, keep_scale, h_bias is not None, loop_weight is not None)
        ctx.direct = (_direct(v), _direct(comp), _direct(h_bias), _direct(loop_weight))
        _stamp_direct(ctx)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        v, comp, coef, out, keep = ctx.saved_tensors
        plan, act, keep_scale, has_bias, has_loop = ctx.meta
        _verify_direct(ctx)
        d_v, d_c, d_b, d_l = ctx.direct
        nb, rows, fout = v.shape
        r = comp.shape[0]
        grad_v = grad_c = None
        g, grad_bias = _epilogue_grad(out, grad_out, act, keep, keep_scale, has_bias and ctx.needs_input_grad[3], d_b)
        want_v, want_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (want_v or want_c) and plan['n_runs'] > 0:
            gi = plan['by_run']                      # destinations = runs, sources = node rows of g
            ones = torch.ones(1, fout, dtype=torch.float32, device=g.device)
            s = bdd_aggregate(gi.by_dst.seg, gi.nbr_by_dst, plan['zeros'], _coef_by_run(plan, coef), None, g, ones, fout, 1, 1)
        else:
            s = None
        dv = dc = None
        if want_v:
            dv = d_v if d_v is not None else torch.zeros_like(v)
        if want_c:
            dc = d_c if d_c is not None else torch.zeros_like(comp)
        if s is not None:
            # a direct target is accumulated into (the arena is zeroed per step); a fresh zeros tensor is as well -- the kernel
            # writes only the rows of ids that occur, so one accumulate flag serves both
            q = torch.empty(plan['n_runs'] * nb if want_c else 0, dtype=torch.float32, device=g.device)
            lib.call('gv_ec_basis_rows_bwd', ptr(v), ptr(comp), ptr(s), ptr(plan['run_id']), ptr(plan['run_rel']),
                     ptr(plan['run_ptr']), plan['n_groups'], ptr(plan['q_pos']), ptr(plan['rel_ptr']), plan['n_runs'], fout, nb, r,
                     rows, ptr(dv), ptr(q), ptr(dc), 1, lib.stream(), tag='ec_basis_bwd')
        if want_v:
            grad_v = None if d_v is not None else dv
        if want_c:
            grad_c = None if d_c is not None else dc
        grad_loop = None
        if has_loop and ctx.needs_input_grad[2]:
            gi = plan['by_id']                       # destinations = loop_weight rows, sources = node rows of g
            ones = torch.ones(1, fout, dtype=torch.float32, device=g.device)
            grad_loop = bdd_aggregate(gi.by_dst.seg, gi.nbr_by_dst, plan['zeros_n'], None, None, g, ones, fout, 1, 1)
            if d_l is not None:
                lib.call('gv_axpby', grad_loop.numel(), None, 1.0, ptr(grad_loop), 1.0, ptr(d_l), lib.stream())
                grad_loop = None
        return grad_v, grad_c, grad_loop, grad_bias, None, None, None, None, None, None


def _coef_by_run(plan, coef):
    """The edge norms in the run <- destination graph's order; cached on the tensor's identity and version (the norm of a graph
    is the same every epoch)."""
    if coef is None:
        return None
    key = (coef.data_ptr(), coef._version, coef.numel())
    hit = plan.get('coef_by_run')
    if hit is None or hit[0] != key:          # the entry holds the tensor: its address cannot be recycled while cached
        hit = plan['coef_by_run'] = (key, coef[plan['edge_of_by_run']].contiguous(), coef)
    return hit[1]


def basis_select_plan(gidx, ridx, ids, in_feat):
    """Index of the fused basis row-select layer, once per (graph, relation types, ids): the distinct (id, relation) pairs of
    the edges (runs, sorted by id then relation), each edge's run in by-destination order, the run <- destination graph of the
    backward, the runs' id groups and their relation order.  No num_rels * in_feat < 2^31 limit: nothing is indexed by W row."""
    cache = ridx.__dict__.setdefault('_basis_select', {})
    key = (ids.data_ptr(), ids._version, ids.numel(), int(in_feat))
    hit = cache.get(key)
    if hit is None:
        ids = ids.reshape(-1)
        if ids.numel() != gidx.num_src_nodes:
            raise ValueError(f'{ids.numel()} node ids for a graph of {gidx.num_src_nodes} nodes')
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= in_feat):
            raise ValueError(f'integer node features must lie in [0, in_feat = {in_feat})')
        if gidx.num_edges >= 2 ** 31:
            raise ValueError('the fused basis select layer indexes edges with int32')
        num_rels = int(ridx.num_rels)
        dev = gidx.device
        et = ridx.keepalive.reshape(-1).to(torch.int64)
        pair = ids[gidx.src32.long()] * num_rels + et                    # caller's edge order
        uniq, run_of = torch.unique(pair, sorted=True, return_inverse=True)
        n_runs = int(uniq.numel())
        run_id = torch.div(uniq, num_rels, rounding_mode='floor')
        run_rel = (uniq - run_id * num_rels).to(torch.int32).contiguous()
        starts = torch.ones(n_runs, dtype=torch.bool, device=dev)
        if n_runs > 1:
            starts[1:] = run_id[1:] != run_id[:-1]
        run_ptr = torch.cat([torch.nonzero(starts).reshape(-1), torch.tensor([n_runs], device=dev)]).to(torch.int64).contiguous()
        order_rel = torch.sort(run_rel, stable=True)[1]
        q_pos = torch.empty(n_runs, dtype=torch.int64, device=dev)
        q_pos[order_rel] = torch.arange(n_runs, device=dev)
        rel_ptr = torch.zeros(num_rels + 1, dtype=torch.int64, device=dev)
        rel_ptr[1:] = torch.cumsum(torch.bincount(run_rel.long(), minlength=num_rels), 0)
        perm_d = gidx.by_dst.perm
        run_by_dst = (run_of if perm_d is None else run_of[perm_d.long()]).to(torch.int32).contiguous()
        by_run = GraphIndex(gidx.dst32.long(), run_of, max(n_runs, 1), num_src_nodes=gidx.num_nodes)
        edge_of = torch.arange(gidx.num_edges, device=dev) if by_run.by_dst.perm is None else by_run.by_dst.perm.long()
        nodes = torch.arange(ids.numel(), device=dev)
        by_id = GraphIndex(nodes, ids, int(in_feat), num_src_nodes=ids.numel())      # loop_weight row <- node
        hit = cache[key] = dict(num_rels=num_rels, n_runs=n_runs, n_groups=int(run_ptr.numel()) - 1,
                                run_id=run_id.to(torch.int32).contiguous(), run_rel=run_rel, run_ptr=run_ptr, q_pos=q_pos,
                                rel_ptr=rel_ptr, run_by_dst=run_by_dst, by_run=by_run, edge_of_by_run=edge_of,
                                zeros=torch.zeros(max(gidx.num_edges, 1), dtype=torch.int32, device=dev), by_id=by_id,
                                zeros_n=torch.zeros(max(ids.numel(), 1), dtype=torch.int32, device=dev),
                                ids=ids.contiguous(), keep=ids)
    return hit


def rel_graph_conv_basis_select(ids, v, comp, h_bias, loop_weight, norm, gidx, ridx, act=ACT_NONE, keep=None, keep_scale=1.0):
    """RelGraphConv('basis', nb < R) with integer-id features, W never formed: v is (nb, in, out), comp (R, nb), ids int64 (N,)."""
    nb, fin, fout = v.shape
    plan = basis_select_plan(gidx, ridx, ids, fin)
    return _RelGraphConvBasisSelect.apply(v, comp, loop_weight, h_bias, norm, gidx, plan, act, keep, float(keep_scale))


EC_HEAD_MAX_CLASSES = 64    # = GV_EC_HEAD_MAX_CLASSES (include/gcnvae.h)


def _head_rows(h):
    h = _chk(h, name='head rows')
    if h.dim() != 2 or not 1 <= h.shape[1] <= EC_HEAD_MAX_CLASSES:
        raise ValueError(f'head rows must be (N, C) with 1 <= C <= {EC_HEAD_MAX_CLASSES}, got {tuple(h.shape)}')
    return h


_head_plans = {}


def head_plan(n, c, labels, sets, device=None):
    """Row -> slot map of up to three DISJOINT index sets (train / validation / test) for gv_ec_head_*, validated once and cached
    on the tensors' identity and version: int64 CUDA 1-D indices in [0, n), no index twice, labels int64 (n,) in [0, C) on the
    indexed rows."""
    if labels is None or not isinstance(labels, torch.Tensor) or not labels.is_cuda:
        raise RuntimeError('labels: the gfx950 head needs a CUDA/ROCm int64 tensor')
    if device is not None and labels.device != device:
        raise RuntimeError(f'labels are on {labels.device}, the head rows on {device}')
    if labels.dtype != torch.int64 or labels.dim() != 1 or labels.shape[0] != n:
        raise ValueError(f'labels must be int64 of shape ({n},), got {labels.dtype} {tuple(labels.shape)}')
    sets = list(sets) + [None] * (3 - len(sets))
    if len(sets) != 3:
        raise ValueError('at most three index sets (train, validation, test)')
    key = (n, c, labels.data_ptr(), labels._version) + tuple(
        (None if s is None else (s.data_ptr(), s._version, s.numel(), s.device)) for s in sets)
    hit = _head_plans.get(key)
    if hit is not None:
        return hit
    parts = []
    for i, s in enumerate(sets):
        if s is None:
            s = torch.zeros(0, dtype=torch.int64, device=labels.device)
        if not isinstance(s, torch.Tensor) or s.device != labels.device:
            raise RuntimeError(f'index set {i}: must be a tensor on {labels.device}')
        if s.dtype != torch.int64 or s.dim() != 1:
            raise ValueError(f'index set {i}: expected 1-D int64, got {s.dtype} {tuple(s.shape)}')
        if s.numel() and (int(s.min()) < 0 or int(s.max()) >= n):
            raise ValueError(f'index set {i}: indices must lie in [0, {n})')
        if s.numel() and (int(labels[s].min()) < 0 or int(labels[s].max()) >= c):
            raise ValueError(f'index set {i}: labels must lie in [0, {c}) on the indexed rows')
        parts.append(s)
    cat = torch.cat(parts)
    if torch.unique(cat).numel() != cat.numel():
        raise ValueError('index sets must be free of duplicates and pairwise disjoint')
    row_pos = torch.full((n,), -1, dtype=torch.int32, device=labels.device)
    row_pos[cat] = torch.arange(cat.numel(), dtype=torch.int32, device=labels.device)
    sizes = [p.numel() for p in parts]
    off = torch.tensor([0, sizes[0], sizes[0] + sizes[1], sum(sizes)], dtype=torch.int64, device=labels.device)
    if len(_head_plans) > 16:
        _head_plans.clear()
    hit = _head_plans[key] = dict(row_pos=row_pos, off=off, sizes=sizes, total=sum(sizes), keep=(labels, parts))
    return hit


class _ECHead(torch.autograd.Function):
    """p = softmax(h) by rows and, over up to three index sets, the mean of F.cross_entropy(p, y) -- a second softmax, as the
    reference trains (kgvae/entity_classify.py:104) -- and the number of rows whose argmax is the label: ONE row launch plus a
    fixed-order finishing pass.  Backward: one row launch, each row's loss term through both softmaxes, plus grad_p."""

    @staticmethod
    def forward(ctx, h, labels, plan):
        n, c = h.shape
        p = torch.empty_like(h)
        losses = torch.empty(3, dtype=torch.float32, device=h.device)
        counts = torch.empty(3, dtype=torch.int32, device=h.device)
        work = torch.empty(max(plan['total'], 1), dtype=torch.float32, device=h.device)
        correct = torch.empty(max(plan['total'], 1), dtype=torch.int32, device=h.device)
        lib.call('gv_ec_head_fwd', ptr(h), ptr(labels), ptr(plan['row_pos']), ptr(plan['off']), n, c, ptr(p), ptr(work),
                 ptr(correct), ptr(losses), ptr(counts), lib.stream())
        ctx.mark_non_differentiable(counts)
        ctx.save_for_backward(p, labels)
        ctx.plan = plan
        return p, losses, counts

    @staticmethod
    def backward(ctx, gp, glosses, _gcounts):
        p, labels = ctx.saved_tensors
        plan = ctx.plan
        n, c = p.shape
        gp = None if gp is None else _chk(gp.contiguous(), name='grad p')
        gl = None if glosses is None else _chk(glosses.contiguous(), name='grad losses')
        dh = torch.empty_like(p)
        lib.call('gv_ec_head_bwd', ptr(p), ptr(labels), ptr(plan['row_pos']), ptr(plan['off']), ptr(gl), ptr(gp), n, c, ptr(dh),
                 lib.stream())
        return dh, None, None


class _SoftmaxRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h):
        n, c = h.shape
        p = torch.empty_like(h)
        lib.call('gv_ec_head_fwd', ptr(h), None, None, None, n, c, ptr(p), None, None, None, None, lib.stream())
        ctx.save_for_backward(p)
        return p

    @staticmethod
    def backward(ctx, gp):
        (p,) = ctx.saved_tensors
        n, c = p.shape
        dh = torch.empty_like(p)
        lib.call('gv_ec_head_bwd', ptr(p), None, None, None, None, ptr(_chk(gp.contiguous(), name='grad p')), n, c, ptr(dh),
                 lib.stream())
        return dh


def softmax_rows(h):
    """softmax(h, dim=1) of (N, C <= 64) rows on the head kernel."""
    return _SoftmaxRows.apply(_head_rows(h))


def ec_head(h, labels, train_idx, val_idx=None, test_idx=None):
    """The entity-classification head on the output layer's pre-softmax rows h (N, C <= 64):
    returns (p, losses, counts) -- p = softmax(h) for every row; losses (3,) = F.cross_entropy(p[idx], labels[idx]) per set
    (NaN for an empty set), differentiable; counts (3,) int32 = rows with argmax(p) == label.  Sets are int64 and disjoint."""
    h = _head_rows(h)
    plan = head_plan(h.shape[0], h.shape[1], labels, (train_idx, val_idx, test_idx), h.device)
    return _ECHead.apply(h, labels, plan)


class _RelGraphConvRows(torch.autograd.Function):
    """The same layer for the multi-GPU DESTINATION-ROW partition ("cheaper alternative"): this rank owns
    ``part.own_rows`` rows of the node table and every edge that ends in them, so it computes FINAL output rows -- no
    reduction of partial aggregates.  ``gidx`` is rectangular: destinations are local row ids, sources index the whole
    table (``part.total_rows`` rows = world x slot rows; a rank's real rows come first in its slot, the tail is zero).

      gather_input   x is this rank's slot (slot_rows, in): ALL-GATHER it into the full table, under the self-loop
                     GEMM of the rank's own rows and the weight packing; backward REDUCE-SCATTERs the partial gradient
                     of the full table (K1^T over the rank's edges), under the loop-weight products and grad-W
      otherwise      x already is the full table (replicated embedding lookup); backward returns this rank's partial
                     gradient of all its rows (summed later by the parameter-gradient all-reduce)
      pad_output     return a (slot_rows, out) tensor with a zero tail, ready to be gathered by the next layer
      gather_output  PIPELINED exchange (part.chunks > 1): the layer itself gathers its output -- its rows are aggregated in
                     part.chunks blocks of slot rows and block k's all-gather runs under block k + 1's aggregation -- and returns
                     the FULL table (total_rows, out).  The gradient that comes back for it is the consumer's reduce-scattered
                     partial sums, valid in this rank's slot rows only (see x_gathered)
      x_gathered     x is such a gathered table: no gather here; backward computes K1^T block by block (the same slot-row range
                     of every rank per block), reduce-scatters block k under block k + 1 and returns a full-size tensor whose
                     rows of THIS rank's slot hold the summed gradient (the others are never read)
    """

    @staticmethod
    def forward(ctx, x, weight, h_bias, loop_weight, norm, gidx, ridx, num_bases, act, keep, keep_scale, part,
                gather_input, pad_output, gather_output=False, x_gathered=False):
        x, _ = _row_major(x, 'x')
        c, slot, row0, total = part.own_rows, part.slot_rows, part.row0, part.total_rows
        in_feat = x.shape[1]
        si = in_feat // num_bases
        so = weight.shape[1] // (num_bases * si)
        out_feat = num_bases * so
        if gidx.num_nodes != c or gidx.num_src_nodes != total:
            raise ValueError(f'row-partition graph index is {gidx.num_nodes} x {gidx.num_src_nodes}, expected {c} x {total}')
        if x_gathered and gather_input:
            raise ValueError('x_gathered: the table arrives gathered, gather_input must be False')
        if x.shape[0] != (slot if gather_input else total):
            raise ValueError(f'x has {x.shape[0]} rows, expected {slot if gather_input else total}')
        coef = None if norm is None else norm.reshape(-1)
        pending = None
        if gather_input:
            x_full = torch.empty(total, in_feat, dtype=torch.float32, device=x.device)
            pending = part.all_gather(x_full, x)
            x_own = x[:c]
        else:
            x_full, x_own = x, x[row0:row0 + c]
        pk = si * so >= 8 and pack_supported(num_bases, si, so, False)
        pk_bwd = si * so >= 8 and pack_supported(num_bases, so, si, True)
        w_fwd = _bdd_weight_fwd(ctx, weight, num_bases, si, so, pk, pk_bwd)
        addend = _gemm_addend(x_own, loop_weight, h_bias, out_feat) if c > 0 else None
        pad_output = pad_output or gather_output
        buf = torch.empty(slot if pad_output else c, out_feat, dtype=torch.float32, device=x.device)
        if pad_output and c < slot:
            buf[c:].zero_()
        if pending is not None:
            pending.wait()
        out = buf[:c]
        result = buf
        if gather_output:
            # block k of the rank's rows is final (aggregate + epilogue in one launch) -> its gather starts; block k + 1 follows
            result = torch.empty(total, out_feat, dtype=torch.float32, device=x.device)
            bounds = part.chunk_bounds()
            subs = gidx.row_blocks('dst', [[(min(a, c), min(b, c))] for a, b in bounds])
            waits = []
            for (a, b), sub in zip(bounds, subs):
                if c > 0 and sub.n_items > 0:
                    bdd_aggregate(sub, gidx.nbr_by_dst, ridx.et_by_dst, coef, gidx.by_dst.perm, x_full, w_fwd, num_bases,
                                  si, so, False, addend, act, keep, keep_scale, out=out, packed=pk)
                waits.append(part.gather_rows(result, buf, a, b))
            for wt in waits:
                wt.wait()
        elif c > 0:
            bdd_aggregate(gidx.by_dst.seg, gidx.nbr_by_dst, ridx.et_by_dst, coef, gidx.by_dst.perm, x_full, w_fwd, num_bases,
                          si, so, False, addend, act, keep, keep_scale, out=out, packed=pk)
        ctx.save_for_backward(x_full, weight, loop_weight, coef, out if act == ACT_RELU else None, keep)
        ctx.meta = (gidx, ridx, num_bases, si, so, act, keep_scale, h_bias is not None, part, gather_input)
        ctx.pipe = (bool(gather_output), bool(x_gathered))
        ctx.direct = (_direct(weight), _direct(h_bias), _direct(loop_weight))
        _stamp_direct(ctx)
        return result

    @staticmethod
    def backward(ctx, grad_out):
        x_full, weight, loop_weight, coef, out, keep = ctx.saved_tensors
        gidx, ridx, nb, si, so, act, keep_scale, has_bias, part, gather_input = ctx.meta
        gather_output, x_gathered = ctx.pipe
        c, slot, row0, total = part.own_rows, part.slot_rows, part.row0, part.total_rows
        _verify_direct(ctx)
        d_w, d_b, d_l = ctx.direct
        dev, in_feat = x_full.device, x_full.shape[1]
        # (a gathered output's gradient is the consumer's reduce-scattered sums, valid in this rank's slot rows)
        grad_out = grad_out[row0:row0 + c] if gather_output else grad_out[:c]
        x_own = x_full[row0:row0 + c]
        if c == 0:           # a rank without rows: contributes zeros to the exchange
            gfull = torch.zeros(total, in_feat, dtype=torch.float32, device=dev)
            if gather_input or x_gathered:
                own = torch.empty(slot, in_feat, dtype=torch.float32, device=dev)
                if x_gathered:
                    for a, b in part.chunk_bounds():
                        part.reduce_scatter_rows(own, gfull, a, b).wait()
                    gfull[row0:row0 + slot].copy_(own)
                    return (gfull,) + (None,) * 15
                part.reduce_scatter(own, gfull).wait()
                return (own,) + (None,) * 15
            return (gfull,) + (None,) * 15
        g, grad_bias = _epilogue_grad(out, grad_out, act, keep, keep_scale, has_bias and ctx.needs_input_grad[2], d_b)
        # K1^T first: its exchange then runs under the loop-weight products and the relation-weight gradient
        grad_x = pending = None
        if ctx.needs_input_grad[0]:
            w_bwd, pk = _bdd_weight_bwd(ctx, weight, nb, so, si)
            coef_s, idx_s = _coef_order(gidx, ridx, coef, 'src')
            own_sum = waits = None
            if x_gathered:
                # block k = the same slot-row range of EVERY rank's slot: its partial sums are complete after its own launch and
                # leave (reduce-scatter) while block k + 1 is computed
                bounds = part.chunk_bounds()
                subs = gidx.row_blocks('src', [[(r * slot + a, r * slot + b) for r in range(part.world)] for a, b in bounds])
                gfull = torch.empty(total, in_feat, dtype=torch.float32, device=dev)
                own_sum = torch.empty(slot, in_feat, dtype=torch.float32, device=dev)
                waits = []
                for (a, b), sub in zip(bounds, subs):
                    bdd_aggregate(sub, gidx.nbr_by_src, ridx.et_by_src, coef_s, idx_s, g, w_bwd, nb, so, si, True, None,
                                  packed=pk, out=gfull)
                    waits.append(part.reduce_scatter_rows(own_sum, gfull, a, b))
            else:
                gfull = bdd_aggregate(gidx.by_src.seg, gidx.nbr_by_src, ridx.et_by_src, coef_s, idx_s, g, w_bwd, nb, so, si,
                                      True, None, packed=pk)                      # (total, in): this rank's partial sums
            if gather_input:
                grad_x = torch.empty(slot, in_feat, dtype=torch.float32, device=dev)
                pending = part.reduce_scatter(grad_x, gfull)
            else:
                grad_x = gfull
        grad_loop, gx_loop = _loop_grads(x_own, g, loop_weight, d_l, ctx.needs_input_grad[3], ctx.needs_input_grad[0])
        grad_w = None
        if ctx.needs_input_grad[1]:
            grad_w = _relation_weight_grad(gidx, ridx, coef, x_full, g, nb, si, so, d_w)
        if pending is not None:
            pending.wait()
        if x_gathered and ctx.needs_input_grad[0]:
            for wt in waits:
                wt.wait()
            grad_x[row0:row0 + slot].copy_(own_sum)      # the summed gradient in this rank's slot rows; the other rows are never read
        if gx_loop is not None:       # the self-loop term only touches the rank's own rows
            own = grad_x[:c] if gather_input else grad_x[row0:row0 + c]
            lib.call('gv_axpby', own.numel(), None, 1.0, ptr(gx_loop), 1.0, ptr(own), lib.stream())
        return (grad_x, grad_w, grad_bias, grad_loop) + (None,) * 12


def rel_graph_conv_rows(x, weight, h_bias, loop_weight, norm, gidx, ridx, num_bases, part, act=ACT_NONE, keep=None,
                        keep_scale=1.0, gather_input=True, pad_output=False, gather_output=False, x_gathered=False):
    return _RelGraphConvRows.apply(x, weight, h_bias, loop_weight, norm, gidx, ridx, num_bases, act, keep,
                                   float(keep_scale), part, bool(gather_input), bool(pad_output), bool(gather_output),
                                   bool(x_gathered))


class _PadRows(torch.autograd.Function):
    """(c, h) -> (rows, h) with a zero tail (a rank's slot of the row partition); backward returns the first c rows."""

    @staticmethod
    def forward(ctx, x, rows):
        ctx.c = x.shape[0]
        out = torch.empty(rows, x.shape[1], dtype=x.dtype, device=x.device)
        out[:ctx.c].copy_(x)
        if rows > ctx.c:
            out[ctx.c:].zero_()
        return out

    @staticmethod
    def backward(ctx, g):
        return g[:ctx.c], None


def pad_rows(x, rows):
    return x if x.shape[0] == rows else _PadRows.apply(x, rows)


class _LinComb2(torch.autograd.Function):
    """wa*a + wb*b on device scalars (b may be None): the rank-local share of the loss in the row partition."""

    @staticmethod
    def forward(ctx, a, wa, b, wb):
        ctx.w = (float(wa), float(wb), b is not None)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        lib.call('gv_lincomb4', ptr(a), float(wa), ptr(b), float(wb), None, 0.0, None, 0.0, ptr(out), lib.stream())
        return out

    @staticmethod
    def backward(ctx, g):
        wa, wb, has_b = ctx.w
        g = _chk(g.reshape(1).contiguous(), name='g')
        ga = torch.empty((), dtype=torch.float32, device=g.device)
        lib.call('gv_lincomb4', ptr(g), wa, None, 0.0, None, 0.0, None, 0.0, ptr(ga), lib.stream())
        gb = None
        if has_b:
            gb = torch.empty((), dtype=torch.float32, device=g.device)
            lib.call('gv_lincomb4', ptr(g), wb, None, 0.0, None, 0.0, None, 0.0, ptr(gb), lib.stream())
        return ga, None, gb, None


def lincomb2(a, wa, b=None, wb=0.0):
    return _LinComb2.apply(a, wa, b, wb)


class _Linear(torch.autograd.Function):
    """y = act(x @ W^T + b) with W (out, in) -- torch's F.linear layout (MaskedLinear, flow_network.py:14-15)."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        x, _ = _row_major(x, 'x')
        y = gemm(x, w, trans_b=True, bias=b, act=act)
        ctx.save_for_backward(x, w, y if act == ACT_RELU else None)
        ctx.act, ctx.has_bias = act, b is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        g = epilogue_bwd(y, gy, ctx.act, None, 1.0) if ctx.act == ACT_RELU else _chk(gy.contiguous(), name='gy')
        gx = gemm(g, w) if ctx.needs_input_grad[0] else None
        gw = None
        if ctx.needs_input_grad[1]:
            gw = gemm(g, x, trans_a=True, split_k=pick_split_k(g.shape[1], x.shape[1], x.shape[0]))
        gb = colsum(g) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return gx, gw, gb, None


def linear(x, w, b=None, act=ACT_NONE):
    return _Linear.apply(x, w, b, act)


class _Mul(torch.autograd.Function):
    """mask * weight (MaskedLinear); the mask is a constant buffer."""

    @staticmethod
    def forward(ctx, mask, w):
        ctx.save_for_backward(mask)
        ctx.direct = _direct(w)
        _stamp_direct(ctx)
        return mul(mask, w)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        _verify_direct(ctx)
        tgt = ctx.direct
        if tgt is not None and tgt.data_ptr() in GRAD_FRESH and tgt.is_contiguous():
            # the weight's slice of the optimiser arena is still all-zero: the masked gradient is written straight into it
            # (no temporary, no AccumulateGrad add)
            g = _chk(g.contiguous(), name='grad')
            lib.call('gv_mul', g.numel(), ptr(mask), ptr(g), ptr(tgt), lib.stream())
            GRAD_FRESH.discard(tgt.data_ptr())
            return None, None
        return None, mul(mask, g)


def masked_weight(mask, w):
    return _Mul.apply(mask, w)


class KLLink:
    """Hand-off between the reparameterisation node and the loss head when K3 and K6 are fused (gv_reparam_kl_fwd / _bwd):
    the forward leaves the KL pass's responsibilities and workspace here for the loss head; the loss head's backward leaves
    the upstream scalar and its two scales here and lets the reparameterisation's backward do KL's node gradients."""
    __slots__ = ('resp', 'ws', 'z_pre_ptr', 'z_pre_version', 'gkl', 'gscale', 'z_extra', 'claimed')

    def __init__(self, resp, ws, z_pre):
        self.resp, self.ws = resp, ws
        self.z_pre_ptr, self.z_pre_version = z_pre.data_ptr(), z_pre._version
        self.gkl = None
        self.gscale = self.z_extra = 0.0
        self.claimed = False          # ONE loss head may take the hand-off; a second one on the same z runs its own KL passes

    def matches(self, z_pre):
        return z_pre is not None and z_pre.data_ptr() == self.z_pre_ptr and z_pre._version == self.z_pre_version


FUSE_REPARAM_KL = _os.environ.get('GV_FUSE_REPARAM_KL', '1') == '1'
# The seam between the encoder's last layer and the loss head, on the hand-off route above: sum z^2 from the KL forward sweep
# (no gv_mean_sq2 launch) and that layer's epilogue gradient + bias sums from the KL backward sweep (no gv_rgcn_epilogue_bwd /
# gv_colsum_finish launches).  GV_KL_SEAM_FOLD=0: the three separate launches.
KL_SEAM_FOLD = _os.environ.get('GV_KL_SEAM_FOLD', '1') == '1'
LOSS_COMBINE_WREL_MAX = 65536      # = GV_LOSS_COMBINE_WREL_MAX (include/gcnvae.h): the combine block sums a relation table up to this size
KL_BWD_COLS4_KMAX = 10             # components the float4-column KL backward holds in registers (csrc/k_loss.hip, kl_bwd_cols4)


class EpilogueLink:
    """Hand-off between an R-GCN layer WITHOUT activation and the reparameterisation node that is the ONLY consumer of its output
    h2 (KGVAE.forward knows that): the layer's forward leaves its keep mask, keep scale and bias-gradient target here; the
    reparameterisation's backward may then write dL/dh2 already masked and sum the bias gradient in the same sweep
    (gv_reparam_kl_bwd_fold).  It records the buffer it returned in ``buf``; the layer's backward skips its own epilogue
    gradient only for that very buffer."""
    __slots__ = ('keep', 'keep_scale', 'want_bias', 'bias_target', 'n_bias', '_gv_direct_epoch', 'buf', 'buf_version', 'grad_bias',
                 'carries_fin', 'fin')

    def __init__(self, keep, keep_scale, want_bias, bias_target, n_bias):
        self.keep, self.keep_scale = keep, float(keep_scale)
        self.want_bias, self.bias_target, self.n_bias = bool(want_bias), bias_target, int(n_bias)
        _stamp_direct(self)               # bias_target is a slice of the optimiser arena as it stood in the layer's forward
        self.buf = self.grad_bias = None
        self.buf_version = 0
        # carries_fin: the layer promises that its backward launches a RiderBox left in ``fin`` (the KL backward's finisher)
        self.carries_fin, self.fin = False, None

    def take_fin(self):
        box, self.fin = self.fin, None
        return box

    def record(self, buf, grad_bias):
        self.buf, self.buf_version, self.grad_bias = buf, buf._version, grad_bias

    def take(self, grad_out):
        """The layer's backward: None when nothing was folded; (g, grad_bias) when ``grad_out`` is the folded buffer, untouched;
        raises when the fold happened but another gradient was added to h2's (the mask cannot be undone)."""
        buf, version, grad_bias = self.buf, self.buf_version, self.grad_bias
        self.buf = self.grad_bias = None
        if buf is None:
            return None
        if (grad_out is None or grad_out.data_ptr() != buf.data_ptr() or tuple(grad_out.shape) != tuple(buf.shape)
                or grad_out.dtype != buf.dtype or not grad_out.is_contiguous() or grad_out._version != version):
            raise RuntimeError('the layer-2 epilogue gradient was folded into the KL backward (ops.EpilogueLink), but the gradient '
                               'arriving at the layer is not that buffer: something else consumed the layer output as well and '
                               'its gradient was added unmasked.  Only hand an EpilogueLink to ops.reparam when it is the sole '
                               'consumer (GV_KL_SEAM_FOLD=0 turns the fold off)')
        return grad_out, grad_bias


def kl_seam_fold_ok(epi, gm, gv, h, k, tensors=()):
    """THE rule of the KL backward's epilogue fold (decided in _Reparam.backward, at run time): a link from the layer, no other
    consumer of z_mean / z_sigma (their gradients would be added to dL/dh2 after the mask), and the float4-column backward's own
    conditions -- h % 4 == 0, h <= 1024, k <= 10 components (their mixture table then fits the LDS), 16-B aligned operands (the
    keep mask 4-B) -- because the lane-per-column form does not carry the fold."""
    if epi is None or not KL_SEAM_FOLD or gm is not None or gv is not None:
        return False
    if _os.environ.get('GV_KL_BWD_V4', '1') == '0' or h % 4 != 0 or h > 1024 or not 1 <= k <= KL_BWD_COLS4_KMAX:
        return False
    if epi.keep is not None and (epi.keep.data_ptr() % 4 != 0 or not epi.keep.is_contiguous()
                                 or tuple(epi.keep.shape)[-1] != 2 * h or epi.keep.dtype != torch.uint8):
        return False
    if epi.want_bias and epi.n_bias != 2 * h:
        return False
    return all(t is None or t.data_ptr() % 16 == 0 for t in tensors)


class _Reparam(torch.autograd.Function):
    """(z, m, v) = reparameterise(h2, eps): m = h2[:, :h], v = softplus(h2[:, h:]) + 1e-8, z = m + eps*sqrt(v).
    With ``z_pre`` (the mixture prior's parameters, (2k, h)) the KL forward pass over the same rows rides along."""

    @staticmethod
    def forward(ctx, h2, eps, z_pre, link_box, epi_link=None, kl_ws=None):
        ctx.set_materialize_grads(False)
        h2 = _chk(h2.contiguous(), name='h2')
        n, h = h2.shape[0], h2.shape[1] // 2
        eps = _chk(eps.contiguous(), name='eps')
        z = torch.empty(n, h, dtype=torch.float32, device=h2.device)
        v = torch.empty_like(z)
        m = torch.empty_like(z)
        ctx.link = None
        ctx.epi_link = epi_link if z_pre is not None else None
        if z_pre is not None:
            z_pre = _chk(z_pre.contiguous(), name='z_pre')
            k = z_pre.shape[0] // 2
            resp = torch.empty(n, k, dtype=torch.float32, device=h2.device)
            if kl_ws is not None and kl_ws.matches(z_pre, n, h, k):     # the mixture table is already at the head of the workspace
                ws = kl_ws.ws
                lib.call('gv_reparam_kl_fwd_mix', ptr(h2), ptr(eps), ptr(z_pre), ptr(z), ptr(v), ptr(m), ptr(resp), ptr(ws), 1, n, h,
                         k, lib.stream())
            else:
                ws = torch.empty(kl_workspace_floats(n, h, k), dtype=torch.float32, device=h2.device)
                lib.call('gv_reparam_kl_fwd', ptr(h2), ptr(eps), ptr(z_pre), ptr(z), ptr(v), ptr(m), ptr(resp), ptr(ws), n, h, k,
                         lib.stream())
            ctx.link = link_box[0] = KLLink(resp, ws, z_pre)
            ctx.save_for_backward(h2, eps, v, z, z_pre)
        else:
            lib.call('gv_reparam_fwd', ptr(h2), ptr(eps), ptr(z), ptr(v), ptr(m), n, h, lib.stream())
            ctx.save_for_backward(h2, eps, v)
        return z, m, v

    @staticmethod
    def backward(ctx, gz, gm, gv):
        link, epi = ctx.link, ctx.epi_link
        if epi is not None:
            epi.buf = epi.grad_bias = None                 # nothing folded yet in this backward pass
        if link is not None and link.gkl is not None:      # the loss head left KL's backward to this node
            h2, eps, v, z, z_pre = ctx.saved_tensors
            n, h = v.shape
            k = z_pre.shape[0] // 2
            gz = None if gz is None else _chk(gz.contiguous(), name='gz')
            d_zp = _direct_flat(z_pre)
            gzp = d_zp if d_zp is not None else torch.empty_like(z_pre)
            gh2 = torch.empty_like(h2)
            if kl_seam_fold_ok(epi, gm, gv, h, k, (z, h2, v, eps, link.resp, link.ws, gz, gh2)):
                # the producing layer's epilogue gradient rides along: gh2 leaves masked, its column sums are the bias gradient
                g_bias = d_b = None
                if epi.want_bias:
                    d_b = epi.bias_target
                    if d_b is not None:
                        _verify_direct(epi)                # the arena slice resolved in the LAYER's forward
                    g_bias = d_b if d_b is not None else torch.empty(2 * h, dtype=torch.float32, device=h2.device)
                # the finishing launch (z_pre's gradient, the bias sums) rides on the layer's dL/dx product, which is next on this
                # stream -- when its outputs are arena slices, which nothing reads before the optimiser (a buffer returned to
                # autograd may be added to another gradient of z_pre at once)
                if (epi.carries_fin and epi.fin is None and rider_kind('klfin') and LIVE_ROWS is None and d_zp is not None
                        and (g_bias is None or d_b is not None)):
                    lib.call('gv_reparam_kl_bwd_fold_sweep', ptr(z), ptr(h2), ptr(v), ptr(eps), ptr(z_pre), ptr(link.resp),
                             ptr(link.gkl), float(link.gscale), float(link.z_extra), ptr(gz), ptr(gh2), ptr(gzp), ptr(epi.keep),
                             epi.keep_scale, ptr(g_bias), ptr(link.ws), n, h, k, lib.stream())
                    epi.fin = RiderBox()
                    epi.fin.klfin = (link.ws, z_pre, link.gkl, float(link.gscale), gzp, d_zp is not None, g_bias, d_b is not None,
                                     n, h, k)
                else:
                    lib.call('gv_reparam_kl_bwd_fold', ptr(z), ptr(h2), ptr(v), ptr(eps), ptr(z_pre), ptr(link.resp), ptr(link.gkl),
                             float(link.gscale), float(link.z_extra), ptr(gz), ptr(gh2), ptr(gzp), 1 if d_zp is not None else 0,
                             ptr(epi.keep), epi.keep_scale, ptr(g_bias), 1 if d_b is not None else 0, ptr(link.ws), n, h, k,
                             lib.stream())
                link.gkl = None
                epi.record(gh2, None if d_b is not None else g_bias)
                return gh2, None, (None if d_zp is not None else gzp), None, None, None
            lib.call('gv_reparam_kl_bwd', ptr(z), ptr(h2), ptr(v), ptr(eps), ptr(z_pre), ptr(link.resp), ptr(link.gkl),
                     float(link.gscale), float(link.z_extra), ptr(gz), ptr(gh2), ptr(gzp), 1 if d_zp is not None else 0,
                     ptr(link.ws), n, h, k, lib.stream())
            link.gkl = None
            if gm is not None or gv is not None:       # z_mean / z_sigma have another consumer (a second loss head, a user's own term)
                extra = torch.empty_like(h2)
                gm = None if gm is None else _chk(gm.contiguous(), name='gm')
                gv = None if gv is None else _chk(gv.contiguous(), name='gv')
                lib.call('gv_reparam_bwd', ptr(h2), ptr(eps), ptr(v), None, ptr(gm), ptr(gv), ptr(extra), n, h, lib.stream())
                gh2 += extra
            return gh2, None, (None if d_zp is not None else gzp), None, None, None
        h2, eps, v = ctx.saved_tensors[:3]
        n, h = v.shape
        gz = None if gz is None else _chk(gz.contiguous(), name='gz')
        gm = None if gm is None else _chk(gm.contiguous(), name='gm')
        gv = None if gv is None else _chk(gv.contiguous(), name='gv')
        gh2 = torch.empty_like(h2)
        lib.call('gv_reparam_bwd', ptr(h2), ptr(eps), ptr(v), ptr(gz), ptr(gm), ptr(gv), ptr(gh2), n, h, lib.stream())
        return gh2, None, None, None, None, None


def kl_workspace_floats(n, h, k):
    return int(lib.load().gv_kl_workspace_bytes(n, h, k)) // 4


class KLWorkspace:
    """A KL workspace allocated AHEAD of ops.reparam, so that its mixture table can be made early (the mix job of a RiderBox):
    ``ws`` for (n, h, k) and the z_pre (address, version) the table is made from.  ops.reparam takes it only for that z_pre."""
    __slots__ = ('ws', 'z_pre', 'key')

    def __init__(self, z_pre, n):
        z_pre = _chk(z_pre.detach().contiguous(), name='z_pre')
        k, h = z_pre.shape[0] // 2, z_pre.shape[1]
        self.z_pre = z_pre
        self.ws = torch.empty(kl_workspace_floats(n, h, k), dtype=torch.float32, device=z_pre.device)
        self.key = (z_pre.data_ptr(), z_pre._version, int(n), h, k)

    def matches(self, z_pre, n, h, k):
        return (z_pre.data_ptr(), z_pre._version, int(n), h, k) == self.key


def reparam(h2, eps, z_pre=None, epi_link=None, kl_ws=None):
    """``z_pre``: when the caller knows that the loss head will evaluate KL(z) against this mixture with no flow in between,
    the KL forward pass is done in the same sweep; the returned z then carries the hand-off (``z._gv_kl_link``).
    ``epi_link``: the EpilogueLink of the layer that made ``h2``, from a caller that knows this node is h2's ONLY consumer.
    ``kl_ws``: a KLWorkspace whose mixture table has been made from this z_pre (on this stream, before this call)."""
    if z_pre is None or not FUSE_REPARAM_KL:
        return _Reparam.apply(h2, eps, None, None, None, None)
    box = [None]
    z, m, v = _Reparam.apply(h2, eps, z_pre, box, epi_link if KL_SEAM_FOLD else None, kl_ws)
    z._gv_kl_link = box[0]
    return z, m, v


# The DistMult head's forward in by-relation order, summing the relation gradient on the way (gv_distmult_bce_fwd_grad), and the
# backward's one finishing launch (gv_distmult_grad_finish) in place of gv_bce_grad + the 1x1 grad-W launches + the regulariser's
# axpby.  GV_DISTMULT_FUSED=0: the separate sweeps.
DISTMULT_FUSED = _os.environ.get('GV_DISTMULT_FUSED', '1') == '1'


def distmult_fused_ok(embed, ld_e, w_rel, ld_w):
    """THE shape rule of the fused DistMult sweep: a triplet's 16 lanes hold up to four float4 columns each (h <= 256, h % 4 == 0,
    16-B aligned rows).  Everything else (h = 500 of BASELINE configs[3] among it) keeps the three separate sweeps."""
    h = embed.shape[1]
    return (DISTMULT_FUSED and h % 4 == 0 and h <= 256 and ld_e % 4 == 0 and ld_w % 4 == 0
            and embed.data_ptr() % 16 == 0 and w_rel.data_ptr() % 16 == 0)


def _distmult_fused_fwd(embed, ld_e, w_rel, ld_w, labels, bias, tidx, score, ws, mmd=None):
    """Launch the fused forward; returns what the finishing launch needs: (delta, u, partial).  ``ws``: 2048 floats.
    ``mmd`` = (z_pri, z, pick, part, gx_u, gy_u): the MMD sweep's row workgroups ride in the same launch."""
    seg, T, h = tidx.rel, tidx.T, embed.shape[1]
    _check_items(seg)
    f32 = dict(dtype=torch.float32, device=embed.device)
    delta = torch.empty(2 * T if tidx.pos3 is not None else T, **f32)
    u = torch.empty(w_rel.shape[0], h, **f32)
    partial = torch.empty(seg.n_slots, h, **f32) if seg.n_fix > 0 else None
    args = (ptr(seg.items), seg.n_items, ptr(tidx.rel_s), ptr(tidx.rel_o), ptr(tidx.rel_tid), ptr(embed), ld_e, ptr(w_rel), ld_w,
            ptr(labels), ptr(bias), ptr(tidx.pos3), ptr(score), ptr(delta), ptr(u), ptr(partial), ptr(ws), T, h)
    if mmd is None:
        lib.call('gv_distmult_bce_fwd_grad', *args, lib.stream())
    else:
        x, y, pick, part, gx_u, gy_u = mmd
        lib.call('gv_distmult_bce_fwd_grad_mmd', *args, ptr(x), ptr(y), ptr(pick), x.shape[0], pick.numel(), x.shape[1],
                 ptr(part), ptr(gx_u), ptr(gy_u), lib.stream())
    return delta, u, partial


def _distmult_fused_finish(fused, gloss, tidx, w_rel, ld_w, reg_scale, g_w, accumulate, ws, dbias):
    """g_w (+)= (g/T) * relation row sums + g * reg_scale * w_rel, *dbias, and the returned coefficients (g/T) * delta (a fresh
    buffer: a second backward over a retained graph scales the forward's delta again, not its own output)."""
    delta, u, partial = fused
    seg = tidx.rel
    d_out = torch.empty_like(delta)
    lib.call('gv_distmult_grad_finish', ptr(gloss), ptr(u), ptr(partial), ptr(seg.fix), seg.n_fix, ptr(seg.rowptr), seg.chunk,
             w_rel.shape[0], w_rel.shape[1], ptr(w_rel), ld_w, float(reg_scale), ptr(g_w), g_w.stride(0), 1 if accumulate else 0,
             ptr(delta), ptr(d_out), delta.numel(), ptr(ws), ptr(dbias), tidx.T, lib.stream())
    return d_out


class _DistMultBCE(torch.autograd.Function):
    """(loss, score) of the DistMult scorer with BCE-with-logits (mean); ``bias`` = flow_log_prob or None.
    ``gscore`` handed to backward (from users of ``score``) is added to the BCE gradient."""

    @staticmethod
    def forward(ctx, embed, w_rel, bias, labels, tidx, grad_mode=True):
        ctx.set_materialize_grads(False)
        embed, ld_e = _row_major(embed, 'embed')
        w_rel, ld_w = _row_major(w_rel, 'w_relation')
        labels = _chk(labels.reshape(-1), name='labels')
        T, h = tidx.T, embed.shape[1]
        if labels.numel() != T:
            raise ValueError('labels / triplets length mismatch')
        score = torch.empty(T, dtype=torch.float32, device=embed.device)
        loss = torch.empty((), dtype=torch.float32, device=embed.device)
        ws = torch.empty(2048, dtype=torch.float32, device=embed.device)
        ctx.fused = None
        # (grad_mode: the caller's torch.is_grad_enabled() -- inside forward it is always off)
        if grad_mode and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]) and distmult_fused_ok(embed, ld_e, w_rel, ld_w):
            ctx.fused = _distmult_fused_fwd(embed, ld_e, w_rel, ld_w, labels, bias, tidx, score, ws)
            lib.call('gv_loss_combine', ptr(ws), T, None, 0, 0, None, 0, h, 0, None, 0, 0, 0.0, 0.0, 0.0, None, ptr(loss), None,
                     lib.stream())
        else:
            lib.call('gv_distmult_bce_fwd', ptr(embed), ld_e, ptr(w_rel), ld_w, ptr(tidx.trip32), ptr(tidx.fwd_order),
                     ptr(labels), ptr(bias), ptr(score), ptr(loss), ptr(ws), T, h, lib.stream())
        ctx.save_for_backward(embed, w_rel, labels, score)
        ctx.tidx, ctx.has_bias, ctx.ws, ctx.ld_w = tidx, bias is not None, ws, ld_w
        ctx.mark_non_differentiable(score)
        return loss, score

    @staticmethod
    def backward(ctx, gloss, _gscore):
        if gloss is None:
            return None, None, None, None, None, None
        embed, w_rel, labels, score = ctx.saved_tensors
        tidx = ctx.tidx
        T, h = tidx.T, embed.shape[1]
        dev = embed.device
        gloss = _chk(gloss.reshape(1).contiguous(), name='gloss')
        dbias = torch.empty((), dtype=torch.float32, device=dev) if ctx.has_bias else None
        if ctx.fused is not None:
            g_w = torch.empty_like(w_rel)
            d_inc = _distmult_fused_finish(ctx.fused, gloss, tidx, w_rel, ctx.ld_w, 0.0, g_w, False, ctx.ws, dbias)
            g_embed = None
            if ctx.needs_input_grad[0]:
                g_embed = bdd_aggregate(tidx.inc, tidx.inc_other, tidx.inc_rel, d_inc,
                                        None if tidx.pos3 is not None else tidx.inc_tid, embed, w_rel, h, 1, 1)
            return g_embed, (g_w if ctx.needs_input_grad[1] else None), dbias, None, None, None
        dscore = torch.empty(T, dtype=torch.float32, device=dev)
        ws = torch.empty(1024, dtype=torch.float32, device=dev)
        lib.call('gv_bce_grad', ptr(score), ptr(labels), ptr(gloss), ptr(dscore), None, None, None, ptr(dbias), ptr(ws), T,
                 lib.stream())
        g_embed = g_w = None
        if ctx.needs_input_grad[0]:
            g_embed = bdd_aggregate(tidx.inc, tidx.inc_other, tidx.inc_rel, dscore, tidx.inc_tid, embed, w_rel,
                                    h, 1, 1)
        if ctx.needs_input_grad[1]:
            g_w = bdd_grad_weight(tidx.rel, tidx.rel_s, tidx.rel_o, dscore, tidx.rel_tid, embed, embed, h, 1, 1)
        return g_embed, g_w, dbias, None, None, None


def distmult_bce(embed, w_rel, bias, labels, tidx):
    return _DistMultBCE.apply(embed, w_rel, bias, labels, tidx, torch.is_grad_enabled())


class _DistMultScore(torch.autograd.Function):
    """score_t = sum_d e[s,d] w[r,d] e[o,d]  (LinkPredict.calc_score) with a general backward."""

    @staticmethod
    def forward(ctx, embed, w_rel, tidx):
        embed, ld_e = _row_major(embed, 'embed')
        w_rel, ld_w = _row_major(w_rel, 'w_relation')
        T, h = tidx.T, embed.shape[1]
        score = torch.empty(T, dtype=torch.float32, device=embed.device)
        loss = torch.empty((), dtype=torch.float32, device=embed.device)
        ws = torch.empty(1024, dtype=torch.float32, device=embed.device)
        zeros = torch.zeros(T, dtype=torch.float32, device=embed.device)
        lib.call('gv_distmult_bce_fwd', ptr(embed), ld_e, ptr(w_rel), ld_w, ptr(tidx.trip32), ptr(tidx.fwd_order), ptr(zeros),
                 None, ptr(score), ptr(loss), ptr(ws), T, h, lib.stream())
        ctx.save_for_backward(embed, w_rel)
        ctx.tidx = tidx
        return score

    @staticmethod
    def backward(ctx, gscore):
        embed, w_rel = ctx.saved_tensors
        tidx, h = ctx.tidx, embed.shape[1]
        gscore = _chk(gscore.contiguous(), name='gscore')
        g_embed = g_w = None
        if ctx.needs_input_grad[0]:
            g_embed = bdd_aggregate(tidx.inc, tidx.inc_other, tidx.inc_rel, gscore, tidx.inc_tid, embed, w_rel,
                                    h, 1, 1)
        if ctx.needs_input_grad[1]:
            g_w = bdd_grad_weight(tidx.rel, tidx.rel_s, tidx.rel_o, gscore, tidx.rel_tid, embed, embed, h, 1, 1)
        return g_embed, g_w, None


def distmult_score(embed, w_rel, tidx):
    return _DistMultScore.apply(embed, w_rel, tidx)


class _MeanSq(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _chk(x.contiguous(), name='x')
        out = torch.empty((), dtype=torch.float32, device=x.device)
        ws = torch.empty(1024, dtype=torch.float32, device=x.device)
        lib.call('gv_mean_sq', ptr(x), x.numel(), 1.0 / x.numel(), ptr(out), ptr(ws), 0, lib.stream())
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return axpby(2.0 / x.numel(), x, a=_chk(g.reshape(1).contiguous(), name='g'))


def mean_sq(x):
    return _MeanSq.apply(x)


class _KL(torch.autograd.Function):
    """KGVAE.get_kl: mean_n[ logN(z; m, v) + flp - log mean_j N(z; m_j, v_j) ]; z_pre is (2k, h)."""

    @staticmethod
    def forward(ctx, z, m, v, z_pre, flp):
        z, m, v = (_chk(t.contiguous(), name=nm) for t, nm in ((z, 'z'), (m, 'z_mean'), (v, 'z_sigma')))
        z_pre = _chk(z_pre.contiguous(), name='z_pre')
        n, h = z.shape
        k = z_pre.shape[0] // 2
        ws = torch.empty(int(lib.load().gv_kl_workspace_bytes(n, h, k)) // 4, dtype=torch.float32, device=z.device)
        resp = torch.empty(n, k, dtype=torch.float32, device=z.device)
        kl = torch.empty((), dtype=torch.float32, device=z.device)
        lib.call('gv_kl_fwd', ptr(z), ptr(m), h, ptr(v), ptr(z_pre), ptr(flp), ptr(resp), ptr(kl), ptr(ws), n, h, k,
                 None, lib.stream())
        ctx.save_for_backward(z, m, v, z_pre, resp, ws)
        ctx.has_flp = flp is not None
        ctx.zp_version = z_pre._version
        return kl

    @staticmethod
    def backward(ctx, gkl):
        z, m, v, z_pre, resp, ws = ctx.saved_tensors       # ws still holds the forward's mixture table
        n, h = z.shape
        k = z_pre.shape[0] // 2
        gkl = _chk(gkl.reshape(1).contiguous(), name='gkl')
        gz, gm, gv = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
        d_zp = _direct_flat(z_pre)
        gzp = d_zp if d_zp is not None else torch.empty_like(z_pre)
        lib.call('gv_kl_bwd', ptr(z), ptr(m), h, ptr(v), ptr(z_pre), ptr(resp), ptr(gkl), 1.0, 0.0, ptr(gz), ptr(gm), ptr(gv),
                 ptr(gzp), 1 if d_zp is not None else 0, ptr(ws), 1, n, h, k, None, lib.stream())
        return gz, gm, gv, (None if d_zp is not None else gzp), (copy_of(gkl.reshape(1)).reshape(()) if ctx.has_flp else None)


def kl_to_mixture(z, m, v, z_pre, flp=None):
    return _KL.apply(z, m, v, z_pre, flp)


class _IAFUpdate(torch.autograd.Function):
    """x_new[:, c] = z*exp(alpha+mu) where colcount[c] > 0 else x_old; net = [mu | alpha]."""

    @staticmethod
    def forward(ctx, z, net, x_old, colcount):
        z, net, x_old = (_chk(t.contiguous(), name=nm) for t, nm in ((z, 'z'), (net, 'net'), (x_old, 'x_old')))
        n, d = z.shape
        x_new = torch.empty_like(z)
        lib.call('gv_iaf_update_fwd', ptr(z), ptr(net), 2 * d, ptr(x_old), ptr(colcount), ptr(x_new), n, d, lib.stream())
        ctx.save_for_backward(z, net, colcount)
        return x_new

    @staticmethod
    def backward(ctx, gx):
        z, net, colcount = ctx.saved_tensors
        n, d = z.shape
        gx = _chk(gx.contiguous(), name='gx')
        gz, gnet, gold = torch.empty_like(z), torch.empty_like(net), torch.empty_like(z)
        lib.call('gv_iaf_update_bwd', ptr(z), ptr(net), 2 * d, ptr(colcount), ptr(gx), None, ptr(gz), ptr(gnet), ptr(gold),
                 n, d, lib.stream())
        return gz, gnet, gold, None


MADE_ROW0_BWD = _os.environ.get('GV_MADE_ROW0_BWD', '1') == '1'


def iaf_bwd_row0(z, net_row, colcount0, g_cur, gld, g_z):
    """Pass 0 of a MADE backward (the update was fed one broadcast [mu | alpha] row): g_z += the pass's share, returns the
    gradient w.r.t. that row (1, 2d) -- gv_iaf_update_bwd_row0, or the generic update backward + column sums + axpby."""
    n, d = z.shape
    st = lib.stream()
    if MADE_ROW0_BWD and d % 4 == 0 and d <= 1024 and net_row.is_contiguous():
        ws = torch.empty(int(lib.load().gv_iaf_update_bwd_row0_workspace_floats(d)), dtype=torch.float32, device=z.device)
        g_row = torch.empty(1, 2 * d, dtype=torch.float32, device=z.device)
        lib.call('gv_iaf_update_bwd_row0', ptr(z), ptr(net_row), ptr(colcount0), ptr(g_cur), ptr(gld), ptr(g_z), ptr(g_row), ptr(ws),
                 n, d, st)
        return g_row
    gz_p = torch.empty(n, d, dtype=torch.float32, device=z.device)
    g_net0 = torch.empty(n, 2 * d, dtype=torch.float32, device=z.device)
    g_dump = torch.empty(n, d, dtype=torch.float32, device=z.device)
    lib.call('gv_iaf_update_bwd', ptr(z), ptr(net_row), 0, ptr(colcount0), ptr(g_cur), ptr(gld), ptr(gz_p), ptr(g_net0), ptr(g_dump),
             n, d, st)
    lib.call('gv_axpby', n * d, None, 1.0, ptr(gz_p), 1.0, ptr(g_z), st)
    return colsum(g_net0).view(1, -1)


def iaf_update(z, net, x_old, colcount):
    return _IAFUpdate.apply(z, net, x_old, colcount)


class _RowSumCols(torch.autograd.Function):
    """sum over columns [col0, col0+ncols) of each row (log_det = sum_d alpha)."""

    @staticmethod
    def forward(ctx, x, col0, ncols):
        x = _chk(x.contiguous(), name='x')
        out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        lib.call('gv_rowsum', ptr(x), x.shape[1], col0, ncols, ptr(out), x.shape[0], lib.stream())
        ctx.meta = (tuple(x.shape), col0, ncols)
        return out

    @staticmethod
    def backward(ctx, g):
        shape, col0, ncols = ctx.meta
        gx = torch.zeros(shape, dtype=torch.float32, device=g.device)
        gx[:, col0:col0 + ncols] = g.unsqueeze(1)
        return gx, None, None


def rowsum_cols(x, col0, ncols):
    return _RowSumCols.apply(x, col0, ncols)


class _MeanRowsMulti(torch.autograd.Function):
    """mean over the rows that exist of the sum of up to 8 per-row vectors: KGVAE.flow_log_prob (kgvae/model.py:116-123) in one
    launch instead of adds + mask + sum + divide through torch; backward: one launch, the same gradient vector for every input.
    Only the first ``n`` entries of the vectors take part (rows riding along behind them -- get_mmd's prior rows -- get zero)."""

    @staticmethod
    def forward(ctx, rows_dev, n, *xs):
        xs = [_chk(x.contiguous().reshape(-1), name='log_det') for x in xs]
        length = xs[0].numel()
        if any(x.numel() != length for x in xs) or not 0 < n <= length:
            raise ValueError('mean_rows_multi: vectors of one length >= n')
        out = torch.empty((), dtype=torch.float32, device=xs[0].device)
        tab = (_ct.c_void_p * len(xs))(*[ptr(x) for x in xs])
        ws = torch.empty(64, dtype=torch.float32, device=xs[0].device)
        lib.call('gv_mean_rows_multi', len(xs), _ct.addressof(tab), n, ptr(rows_dev), ptr(out), ptr(ws), lib.stream())
        ctx.rows_dev, ctx.n, ctx.len, ctx.k = rows_dev, n, length, len(xs)
        return out

    @staticmethod
    def backward(ctx, g):
        g = _chk(g.contiguous().reshape(()), name='g')
        gx = torch.empty(ctx.len, dtype=torch.float32, device=g.device)
        lib.call('gv_mean_rows_bwd', ptr(g), ctx.len, ctx.n, ptr(ctx.rows_dev), ptr(gx), lib.stream())
        return (None, None) + (gx,) * ctx.k


def mean_rows_multi(xs, n=None, rows_dev=None):
    """mean_r sum_i xs[i][r] over the first n rows (None: all) that exist (rows_dev: device int32 count, None = all n)."""
    xs = list(xs)
    if not 1 <= len(xs) <= 8:
        raise ValueError('mean_rows_multi: 1..8 vectors')
    return _MeanRowsMulti.apply(rows_dev, int(xs[0].numel() if n is None else n), *xs)


class _ReverseCols(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _chk(x.contiguous(), name='x')
        out = torch.empty_like(x)
        lib.call('gv_reverse_cols', ptr(x), ptr(out), x.shape[0], x.shape[1], lib.stream())
        return out

    @staticmethod
    def backward(ctx, g):
        g = _chk(g.contiguous(), name='g')
        out = torch.empty_like(g)
        lib.call('gv_reverse_cols', ptr(g), ptr(out), g.shape[0], g.shape[1], lib.stream())
        return out


def reverse_cols(x):
    return _ReverseCols.apply(x)


class _MatMul(torch.autograd.Function):
    """Plain differentiable a @ b on the f32 MFMA GEMM (basis combination W = w_comp @ V)."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return gemm(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = _chk(g.contiguous(), name='g')
        ga = gemm(g, b, trans_b=True) if ctx.needs_input_grad[0] else None
        gb = gemm(a, g, trans_a=True, split_k=pick_split_k(a.shape[1], g.shape[1], a.shape[0])) \
            if ctx.needs_input_grad[1] else None
        return ga, gb


def matmul(a, b):
    return _MatMul.apply(a, b)


class _MMD(torch.autograd.Function):
    """KGVAE.get_mmd's three RBF-kernel means on x (sx, h) and y (sy, h), fused forward / backward."""

    @staticmethod
    def forward(ctx, x, y):
        x, y = _chk(x.contiguous(), name='z_pri'), _chk(y.contiguous(), name='z_post')
        out = torch.empty((), dtype=torch.float32, device=x.device)
        ws = torch.empty(x.shape[0] + y.shape[0], dtype=torch.float32, device=x.device)
        lib.call('gv_mmd_fwd', ptr(x), ptr(y), None, x.shape[0], y.shape[0], x.shape[1], ptr(out), ptr(ws), lib.stream())
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        g = _chk(g.reshape(1).contiguous(), name='g')
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        lib.call('gv_mmd_bwd', ptr(x), ptr(y), None, x.shape[0], y.shape[0], x.shape[1], ptr(g), 1.0, ptr(gx), ptr(gy),
                 lib.stream())
        return gx, gy


def mmd(x, y):
    return _MMD.apply(x, y)


# The MMD term's value and gradients in one sweep, riding in the fused DistMult forward launch (gv_distmult_bce_fwd_grad_mmd), and
# ONE finishing launch in the backward (gv_mmd_grad_finish) in place of gv_mmd_fwd + gv_mmd_bwd + gv_prior_sample_bwd.
# GV_MMD_FUSED=0: the separate launches.
MMD_FUSED = _os.environ.get('GV_MMD_FUSED', '1') == '1'


def mmd_sweep_ok(z_pri, z, h_max=256):
    """THE shape rule of the one-sweep MMD inside the DistMult launch: a partner row's 16 lanes hold up to four float4 columns each
    (h <= 256, h % 4 == 0, 16-B aligned rows) and a workgroup per row leaves one of gv_loss_combine's 1024 partial slots."""
    h = z_pri.shape[1]
    return (MMD_FUSED and h % 4 == 0 and h <= h_max and z.shape[1] == h and z_pri.data_ptr() % 16 == 0
            and z.data_ptr() % 16 == 0)


class PriorLink:
    """Hand-off between the prior sampler's node and the loss head that takes its output as z_pri: the sampler's forward leaves
    z_pre and eps here; a loss head on the one-sweep MMD route claims the link (once) and its backward's finishing launch
    (gv_mmd_grad_finish) produces z_pre's gradient from the unscaled MMD rows itself.  It records the z_pri gradient buffer it
    returned in ``buf``; the sampler's backward skips its own launch only for that very buffer."""
    __slots__ = ('z_pre', 'eps', 'out_ptr', 'out_version', 'out_shape', 'claimed', 'buf', 'buf_version', 'gz')

    def __init__(self, z_pre, eps, out):
        self.z_pre, self.eps = z_pre, eps
        self.out_ptr, self.out_version, self.out_shape = out.data_ptr(), out._version, tuple(out.shape)
        self.claimed = False          # ONE loss head may take the hand-off; a second one on the same z_pri runs the separate launches
        self.buf = self.gz = None
        self.buf_version = 0

    def matches(self, z_pri):
        return (z_pri is not None and z_pri.data_ptr() == self.out_ptr and z_pri._version == self.out_version
                and tuple(z_pri.shape) == self.out_shape and z_pri.is_contiguous())

    def record(self, buf, gz):
        self.buf, self.buf_version, self.gz = buf, buf._version, gz

    def take(self, grad_out):
        """The sampler's backward: None when nothing was folded; (gz,) -- gz None when z_pre's gradient went straight into its
        direct target -- when ``grad_out`` is the buffer the loss head returned, untouched; raises when the fold happened but
        another gradient was added to z_pri's (z_pre's share of it would be lost)."""
        buf, version, gz = self.buf, self.buf_version, self.gz
        self.buf = self.gz = None
        if buf is None:
            return None
        if (grad_out is None or grad_out.data_ptr() != buf.data_ptr() or tuple(grad_out.shape) != tuple(buf.shape)
                or grad_out.dtype != buf.dtype or not grad_out.is_contiguous() or grad_out._version != version):
            raise RuntimeError('the prior sampler\'s backward was folded into the loss head\'s MMD finishing launch (ops.PriorLink), '
                               'but the gradient arriving at the sampler is not that buffer: something else consumed z_pri as well.  '
                               'Only hand a linked z_pri to ops.loss_head when the head is its sole consumer (GV_MMD_FUSED=0 turns '
                               'the fold off)')
        return (gz,)


class _PriorSample(torch.autograd.Function):
    """z_pri = cat([m]*repeat) + eps * cat([sqrt(softplus(raw)+1e-8)]*repeat) for z_pre = [m; raw] (2k, h)."""

    @staticmethod
    def forward(ctx, z_pre, eps, link_box=None, riders=None):
        z_pre, eps = _chk(z_pre.contiguous(), name='z_pre'), _chk(eps.contiguous(), name='eps')
        k, h = z_pre.shape[0] // 2, z_pre.shape[1]
        out = torch.empty_like(eps)
        ctx.set_materialize_grads(False)
        if riders is not None and riders.prior is None and not riders.done and rider_kind('prior'):
            riders.prior = (z_pre, eps, out)          # the box's product carries the launch (eps is complete on this stream)
        else:
            lib.call('gv_prior_sample_fwd', ptr(z_pre), ptr(eps), ptr(out), eps.shape[0], k, h, lib.stream())
        ctx.save_for_backward(z_pre, eps)
        ctx.link = None
        if link_box is not None and eps.shape[0] % k == 0:
            ctx.link = link_box[0] = PriorLink(z_pre, eps, out)
        return out

    @staticmethod
    def backward(ctx, g):
        z_pre, eps = ctx.saved_tensors
        link = ctx.link
        if link is not None and link.claimed:
            folded = link.take(g)
            if folded is not None:
                return folded[0], None, None, None
        if g is None:
            return None, None, None, None
        g = _chk(g.contiguous(), name='g')
        d_zp = _direct_flat(z_pre)
        gz = d_zp if d_zp is not None else torch.empty_like(z_pre)
        lib.call('gv_prior_sample_bwd', ptr(z_pre), ptr(eps), ptr(g), ptr(gz), 1 if d_zp is not None else 0, eps.shape[0],
                 z_pre.shape[0] // 2, z_pre.shape[1], lib.stream())
        return (None if d_zp is not None else gz), None, None, None


def prior_sample(z_pre, eps, riders=None):
    """The returned z_pri carries the hand-off to a loss head on the one-sweep MMD route (``z_pri._gv_prior_link``).
    ``riders`` (RiderBox): a box whose product is launched later on this stream and before anything reads z_pri carries the launch."""
    if not MMD_FUSED:
        return _PriorSample.apply(z_pre, eps, None, riders)
    box = [None]
    out = _PriorSample.apply(z_pre, eps, box, riders)
    out._gv_prior_link = box[0]
    return out


class _LossHead(torch.autograd.Function):
    """LinkPredict.get_loss as ONE autograd node (kgvae/link_predict.py:71-92):

        loss = BCE(DistMult(z, w_rel, triplets) + flp) + reg*(mean z^2 + mean w_rel^2) + kl_w*KL + mmd_w*MMD

    with KL = KGVAE.get_kl(z) and MMD = KGVAE.get_mmd's kernel means on (z_pri, z[pick]).  Forward is the
    K5/K6 kernels plus one scalar combine; backward produces a single gradient for z: KL's gz, the regulariser
    and the MMD rows are accumulated into one buffer that the DistMult gather-aggregate (K1, 1x1 blocks)
    takes as its fused addend -- no multi-use gradient adds, no scalar glue kernels.  The KL and MMD kernel
    groups (small, latency-bound) run on side streams beside the bandwidth-bound DistMult kernels.
    Returns (loss, predict_loss, kl, mmd); only ``loss`` is differentiable.
    """

    @staticmethod
    def forward(ctx, z, z_mean, z_sigma, w_rel, z_pre, flp, z_pri, pick, labels, tidx, reg_w, kl_w, mmd_w, score_bias,
                embed_rows=None, rows_dev=None, kl_link=None, grad_mode=True, prior_link=None):
        z, ld_z = _row_major(z, 'embed')
        if rows_dev is not None:          # static-shape batch: rows [*rows_dev, n) of z are padding (include/gcnvae.h, rows_dev)
            rows_dev = _chk(rows_dev.reshape(-1), torch.int32, 'rows_dev')
            if kl_w <= 0 or embed_rows is not None:
                raise NotImplementedError('rows_dev needs kl_w > 0 (the padding rows are masked in the KL pass) and no embed_rows')
        w_rel, ld_w = _row_major(w_rel, 'w_relation')
        labels = _chk(labels.reshape(-1), name='labels')
        dev, (n, h), T = z.device, z.shape, tidx.T
        if labels.numel() != T:
            raise ValueError('labels / triplets length mismatch')
        f32 = dict(dtype=torch.float32, device=dev)
        ctx.set_materialize_grads(False)
        scal = torch.empty(4, **f32)                 # pred, reg, kl, mmd (each written before it is read)
        pred, reg, kl, mmd = scal[0:1], scal[1:2], scal[2:3], scal[3:4]
        ws, ws2 = torch.empty(2048, **f32), torch.empty(1024, **f32)
        score = torch.empty(T, **f32)
        loss = torch.empty((), **f32)
        bias = flp if (score_bias and flp is not None) else None
        resp = wsk = z_post = wsm = None
        link = kl_link if (kl_link is not None and not kl_link.claimed and kl_w > 0 and flp is None and rows_dev is None
                           and embed_rows is None and kl_link.matches(z_pre) and kl_link.resp.shape[0] == n) else None
        if link is not None:
            link.claimed = True
        if kl_w > 0:
            z_mean, z_sigma = _chk(z_mean.contiguous(), name='z_mean'), _chk(z_sigma.contiguous(), name='z_sigma')
            z_pre = _chk(z_pre.contiguous(), name='z_pre')
            k = z_pre.shape[0] // 2
            if link is None:
                wsk = torch.empty(int(lib.load().gv_kl_workspace_bytes(n, h, k)) // 4, **f32)
                resp = torch.empty(n, k, **f32)
        if mmd_w > 0:
            z_pri = _chk(z_pri.contiguous(), name='z_pri')
            pick = _chk(pick.reshape(-1), torch.int64, 'pick')
            wsm = torch.empty(z_pri.shape[0] + pick.numel(), **f32)
        if ld_z != h or ld_w != h:
            raise ValueError('loss_head needs contiguous embeddings and relation table')
        # (grad_mode: the caller's torch.is_grad_enabled() -- inside forward it is always off)
        dm_fused = grad_mode and (ctx.needs_input_grad[0] or ctx.needs_input_grad[3]) and distmult_fused_ok(z, ld_z, w_rel, ld_w)
        # the MMD sweep rides in the fused DistMult launch when the sampler that made z_pri left its hand-off (its backward is
        # then this node's finishing launch) and the shapes fit
        plink = prior_link if (mmd_w > 0 and dm_fused and prior_link is not None and not prior_link.claimed
                               and prior_link.matches(z_pri) and mmd_sweep_ok(z_pri, z)
                               and z_pri.shape[0] + pick.numel() <= 1024) else None
        if plink is not None:
            plink.claimed = True
        ctx.prior_link = plink
        st = lib.stream()
        # every term leaves its per-block partial sums in its workspace; ONE combine launch finishes the four sums
        if link is not None:
            resp, wsk = link.resp, link.ws                 # the KL pass already ran with the reparameterisation
        elif kl_w > 0:
            lib.call('gv_kl_fwd', ptr(z), ptr(z_mean), h, ptr(z_sigma), ptr(z_pre), ptr(flp), ptr(resp), None, ptr(wsk),
                     n, h, k, ptr(rows_dev), st)
        if mmd_w > 0 and plink is None:      # the posterior sample set is rows `pick` of z, read in place
            lib.call('gv_mmd_fwd', ptr(z_pri), ptr(z), ptr(pick), z_pri.shape[0], pick.numel(), h, None, ptr(wsm), st)
        # embed_rows: the regulariser's mean runs over that many rows (the rest of z are all-zero padding rows of the
        # multi-GPU row partition)
        z_count = z.numel() if embed_rows is None else int(embed_rows) * h
        # on the hand-off route the KL sweep that made z left sum z^2 in its workspace, and the combine launch sums w_rel^2 itself
        reg_fold = (link is not None and KL_SEAM_FOLD and w_rel.numel() <= LOSS_COMBINE_WREL_MAX and w_rel.numel() % 4 == 0
                    and w_rel.data_ptr() % 16 == 0)
        if not reg_fold:
            lib.call('gv_mean_sq2', ptr(z), z.numel(), 1.0 / z_count, ptr(w_rel), w_rel.numel(), 1.0 / w_rel.numel(), None,
                     ptr(ws2), ptr(rows_dev), n, st)
        # DistMult scorer + BCE (three 800-B row gathers per triplet: the bandwidth-bound part)
        # (with a backward to come and a width the fused sweep covers: in by-relation order, the relation gradient's sums with it)
        ctx.fused = ctx.mmd_u = None
        if dm_fused:
            if plink is not None:      # value partials and the gradient rows at upstream 1, for the backward's finishing launch
                ctx.mmd_u = (torch.empty_like(z_pri), torch.empty(pick.numel(), h, **f32))
            ctx.fused = _distmult_fused_fwd(z, ld_z, w_rel, ld_w, labels, bias, tidx, score, ws,
                                            None if plink is None else (z_pri, z, pick, wsm) + ctx.mmd_u)
            ctx.ws = ws
        else:
            lib.call('gv_distmult_bce_fwd', ptr(z), ld_z, ptr(w_rel), ld_w, ptr(tidx.trip32), ptr(tidx.fwd_order), ptr(labels),
                     ptr(bias), ptr(score), None, ptr(ws), T, h, st)
        if reg_fold:
            lib.call('gv_loss_combine_fold', ptr(ws), T, ptr(w_rel), z.numel(), w_rel.numel(), ptr(wsk), n, h, z_pre.shape[0] // 2,
                     ptr(wsm) if mmd_w > 0 else None, z_pri.shape[0] if mmd_w > 0 else 0, pick.numel() if mmd_w > 0 else 0,
                     float(reg_w), float(kl_w), float(mmd_w), ptr(scal), ptr(loss), st)
        else:
            lib.call('gv_loss_combine', ptr(ws), T, ptr(ws2), z.numel(), w_rel.numel(), ptr(wsk) if kl_w > 0 else None, n, h,
                     (z_pre.shape[0] // 2) if kl_w > 0 else 0, ptr(wsm) if mmd_w > 0 else None,
                     z_pri.shape[0] if mmd_w > 0 else 0, pick.numel() if mmd_w > 0 else 0, float(reg_w), float(kl_w),
                     float(mmd_w), ptr(scal), ptr(loss), ptr(rows_dev), st)
        ctx.save_for_backward(z, z_mean if kl_w > 0 else None, z_sigma if kl_w > 0 else None, w_rel,
                              z_pre if kl_w > 0 else None, resp, z_pri if mmd_w > 0 else None, z_post,
                              pick if mmd_w > 0 else None, labels, score, wsk, rows_dev)
        ctx.meta = (tidx, float(reg_w), float(kl_w), float(mmd_w), bias is not None, flp is not None and kl_w > 0)
        ctx.z_count = z_count
        ctx.kl_link = link
        ctx.direct_w = _direct(w_rel) if ld_w == h else None
        _stamp_direct(ctx)
        out_pred, out_kl, out_mmd = pred.reshape(()), kl.reshape(1), mmd.reshape(())
        ctx.mark_non_differentiable(out_pred, out_kl, out_mmd)
        return loss, out_pred, out_kl, out_mmd

    @staticmethod
    def backward(ctx, g, _gp, _gk, _gm):
        if g is None:
            return (None,) * 19
        z, z_mean, z_sigma, w_rel, z_pre, resp, z_pri, z_post, pick, labels, score, wsk, rows_dev = ctx.saved_tensors
        z_count = ctx.z_count
        tidx, reg_w, kl_w, mmd_w, has_bias, flp_in_kl = ctx.meta
        dev, (n, h), T = z.device, z.shape, tidx.T
        f32 = dict(dtype=torch.float32, device=dev)
        g = _chk(g.reshape(1).contiguous(), name='gloss')
        # every buffer a side branch writes is allocated here, before the forks
        fused = ctx.fused
        dscore = torch.empty(T, **f32) if fused is None else None
        dbias = torch.empty((), **f32) if has_bias else None      # (written by an ordered final sum: no fill)
        ws = torch.empty(1024, **f32) if fused is None else None
        link = ctx.kl_link
        gz = torch.empty_like(z) if link is None else None
        gm = gv = gzp = d_zp = g_pri = g_post = None
        if link is not None:
            # KL's node gradients and the regulariser's are chained through the reparameterisation by ITS backward
            # (gv_reparam_kl_bwd): here only the scalar and the two scales are handed over
            link.gkl, link.gscale, link.z_extra = g, kl_w, 2.0 * reg_w / z_count
            d_zp = True          # z_pre's gradient is produced there too
        elif kl_w > 0:
            k = z_pre.shape[0] // 2                       # wsk: the forward's workspace, mixture table still valid
            d_zp = _direct_flat(z_pre)
            gm, gv = torch.empty_like(z), torch.empty_like(z)
            gzp = d_zp if d_zp is not None else torch.empty_like(z_pre)
        plink, gzs, d_zs = ctx.prior_link, None, None
        if mmd_w > 0:
            g_pri = torch.empty_like(z_pri)
        if plink is not None:      # the sampler's z_pre gradient is produced by the finishing launch
            d_zs = _direct_flat(plink.z_pre)
            gzs = d_zs if d_zs is not None else torch.empty_like(plink.z_pre)
        _verify_direct(ctx)
        d_w = ctx.direct_w
        g_w = d_w if d_w is not None else torch.empty_like(w_rel)
        g_flp = torch.empty((), **f32) if (has_bias or flp_in_kl) else None
        st = lib.stream()

        def mmd_backward(target, stream):
            """The MMD rows ADDED into rows `pick` of ``target``, z_pri's gradient into g_pri (and, on the one-sweep route, the
            sampler's z_pre gradient)."""
            if plink is None:
                lib.call('gv_mmd_bwd', ptr(z_pri), ptr(z), ptr(pick), z_pri.shape[0], pick.numel(), h, ptr(g), mmd_w,
                         ptr(g_pri), ptr(target), stream)
                return
            gx_u, gy_u = ctx.mmd_u
            lib.call('gv_mmd_grad_finish', ptr(gx_u), ptr(gy_u), ptr(pick), z_pri.shape[0], pick.numel(), h, ptr(g), mmd_w,
                     ptr(target), ptr(g_pri), ptr(plink.z_pre), ptr(plink.eps), ptr(gzs), 1 if d_zs is not None else 0,
                     plink.z_pre.shape[0] // 2, stream)
            plink.record(g_pri, None if d_zs is not None else gzs)
        # branch 1: KL backward (writes gz, gm, gv, gzp), then the regulariser folded into gz
        with fork(1):
            s1 = lib.stream()
            if link is not None:
                pass
            elif kl_w > 0:
                # the embedding regulariser's gradient g * (2 reg_w / numel) * z rides on the same pass over z
                lib.call('gv_kl_bwd', ptr(z), ptr(z_mean), h, ptr(z_sigma), ptr(z_pre), ptr(resp), ptr(g), kl_w,
                         2.0 * reg_w / z_count, ptr(gz), ptr(gm), ptr(gv), ptr(gzp), 1 if d_zp is not None else 0, ptr(wsk),
                         1, n, h, k, ptr(rows_dev), s1)
            else:
                lib.call('gv_axpby', z.numel(), ptr(g), 2.0 * reg_w / z_count, ptr(z), 0.0, ptr(gz), s1)
            if mmd_w > 0 and link is None:      # MMD backward: prior rows -> g_pri, posterior rows ADDED into rows `pick` of gz (now complete)
                mmd_backward(gz, s1)
        # main: dL/dscore, then the relation-side gradient (does not need gz)
        if fused is not None:          # the forward summed the relation rows: scale them, add the regulariser, scale delta
            d_inc = _distmult_fused_finish(fused, g, tidx, w_rel, h, 2.0 * reg_w / w_rel.numel(), g_w, d_w is not None, ctx.ws,
                                           dbias)
            idx_inc = None if tidx.pos3 is not None else tidx.inc_tid
        else:
            if tidx.pos3 is not None:      # dL/dscore also lands in the two launches' own orders
                d_inc, d_rel, idx_inc, idx_rel = torch.empty(2 * T, **f32), torch.empty(T, **f32), None, None
            else:
                d_inc, d_rel, idx_inc, idx_rel = dscore, dscore, tidx.inc_tid, tidx.rel_tid
            lib.call('gv_bce_grad', ptr(score), ptr(labels), ptr(g), ptr(dscore), ptr(tidx.pos3),
                     ptr(d_inc) if tidx.pos3 is not None else None, ptr(d_rel) if tidx.pos3 is not None else None,
                     ptr(dbias), ptr(ws), T, st)
            bdd_grad_weight(tidx.rel, tidx.rel_s, tidx.rel_o, d_rel, idx_rel, z, z, h, 1, 1, out=g_w,
                            accumulate=d_w is not None)
            lib.call('gv_axpby', w_rel.numel(), ptr(g), 2.0 * reg_w / w_rel.numel(), ptr(w_rel), 1.0, ptr(g_w), st)
        join(1)
        g_z = bdd_aggregate(indices.largest_first(tidx.inc) if indices.K1_ITEMS_LARGEST_FIRST else tidx.inc, tidx.inc_other, tidx.inc_rel,
                            d_inc, idx_inc, z, w_rel, h, 1, 1, addend=gz)
        if link is not None and mmd_w > 0:       # no KL buffer to ride on: the MMD rows are added to the decoder's gradient
            mmd_backward(g_z, st)
        if g_flp is not None:
            lib.call('gv_lincomb4', ptr(dbias) if has_bias else None, 1.0, ptr(g) if flp_in_kl else None, kl_w, None, 0.0,
                     None, 0.0, ptr(g_flp), st)
        return (g_z, gm, gv, (None if d_w is not None else g_w), (None if d_zp is not None else gzp), g_flp, g_pri, None,
                None, None, None, None, None, None, None, None, None, None, None)


def loss_head(z, z_mean, z_sigma, w_rel, z_pre, flp, z_pri, pick, labels, tidx, reg_w, kl_w, mmd_w, score_bias,
              embed_rows=None, rows_dev=None):
    return _LossHead.apply(z, z_mean, z_sigma, w_rel, z_pre, flp, z_pri, pick, labels, tidx, float(reg_w), float(kl_w),
                           float(mmd_w), bool(score_bias), embed_rows, rows_dev, getattr(z, '_gv_kl_link', None),
                           torch.is_grad_enabled(), getattr(z_pri, '_gv_prior_link', None))


# ------------------------------------------------------------------------------------------------
# K4, the masked MLP of the IAF blocks (MADE): made.py -- same namespace for the callers (ops.made_forward, ops.made_chain, ...)
# ------------------------------------------------------------------------------------------------
from .made import *                                              # noqa: E402,F401,F403
from .made import _ChainLayer, _RowLayer, _MADEForward, _MADEForwardBF16      # noqa: E402,F401
from . import made                                               # noqa: E402,F401  (ops.made.<KNOB>)


# ------------------------------------------------------------------------------------------------
# TransE (transe.py): sampler, fused step, ordered SGD, queries, distances and the filtered ranker (k_transe.hip)
# ------------------------------------------------------------------------------------------------
TRANSE_MAX_DIM = 512      # = GV_TRANSE_MAX_DIM (include/gcnvae.h)


def _i32(t, name, n=None):
    t = _chk(t, torch.int32, name)
    if not t.is_contiguous() or (n is not None and t.numel() != n):
        raise ValueError(f'{name}: expected a contiguous int32 tensor of {n} entries')
    return t


def _table(t, name):
    t = _chk(t, name=name)
    if t.dim() != 2 or not t.is_contiguous() or not 1 <= t.shape[1] <= TRANSE_MAX_DIM:
        raise ValueError(f'{name}: expected a contiguous (rows, dim) float32 table with 1 <= dim <= {TRANSE_MAX_DIM}')
    return t


def _p_norm(p):
    if p not in (1, 2):
        raise ValueError(f'p_norm must be 1 or 2, got {p}')
    return int(p)


def transe_sample(rng_state, stream_id, train, n_ent, batch, neg_ent, p_head=None, filt=None, bh=None, br=None, bt=None,
                  draws=None, check=True):
    """(bh, br, bt) int32 of batch * (1 + neg_ent) rows in OpenKE's layout (gv_transe_sample).  ``train`` int32 (n, 3) on the device;
    ``p_head`` float32 [num_rels] or None; ``filt`` = (f_lo, f_hi, f_ent_o, f_ent_s) as ``transe.TrainFilter`` holds them, or None.
    ``check`` reads the triples and filter ranges back to validate them before the launch (pass False under capture, once the
    same arrays have been checked)."""
    train = _i32(train, 'train')
    if train.dim() != 2 or train.shape[1] != 3 or train.shape[0] < 1:
        raise ValueError('train: expected (n >= 1, 3) int32 triples')
    batch, neg_ent, n_ent = int(batch), int(neg_ent), int(n_ent)
    if batch < 1 or neg_ent < 0 or n_ent < 1:
        raise ValueError(f'batch={batch} neg_ent={neg_ent} n_ent={n_ent}')
    n = batch * (1 + neg_ent)
    dev = train.device
    bh = torch.empty(n, dtype=torch.int32, device=dev) if bh is None else _i32(bh, 'bh', n)
    br = torch.empty(n, dtype=torch.int32, device=dev) if br is None else _i32(br, 'br', n)
    bt = torch.empty(n, dtype=torch.int32, device=dev) if bt is None else _i32(bt, 'bt', n)
    if p_head is not None:
        p_head = _chk(p_head, name='p_head')
    if check:        # reads the triples back (once per training set in DeviceTrainer; callers under capture pass check=False)
        if int(train[:, [0, 2]].min()) < 0 or int(train[:, [0, 2]].max()) >= n_ent or int(train[:, 1].min()) < 0:
            raise ValueError(f'train: entity ids must lie in [0, {n_ent}) and relation ids be >= 0')
        if p_head is not None and int(train[:, 1].max()) >= p_head.numel():
            raise ValueError(f'p_head: {p_head.numel()} entries, relation ids up to {int(train[:, 1].max())}')
    f = [None] * 4
    if filt is not None:
        f = [_i32(filt[0], 'f_lo', 2 * train.shape[0]), _i32(filt[1], 'f_hi', 2 * train.shape[0]),
             _i32(filt[2], 'f_ent_o'), _i32(filt[3], 'f_ent_s')]
        if check and (int(f[0].min()) < 0 or bool((f[1] < f[0]).any())
                      or int(f[1][0::2].max()) > f[2].numel() or int(f[1][1::2].max()) > f[3].numel()):
            raise ValueError('filt: ranges must satisfy 0 <= f_lo <= f_hi <= len(f_ent_o / f_ent_s)')
    rng_state = _chk(rng_state, torch.int64, 'rng_state')
    if rng_state.numel() < 2 or rng_state.device != train.device:
        raise ValueError('rng_state: the {seed, tick} int64 pair on the triples\' device')
    if draws is not None:
        draws = _chk(draws, torch.int32, 'draws')
        if draws.numel() != batch * (neg_ent + 2):
            raise ValueError('draws: batch * (neg_ent + 2) int32 entries')
    lib.call('gv_transe_sample', ptr(rng_state), int(stream_id) & 0xFFFFFFFF, ptr(train), train.shape[0], n_ent, ptr(p_head),
             *[ptr(x) for x in f], batch, neg_ent, ptr(bh), ptr(br), ptr(bt), ptr(draws), lib.stream())
    return bh, br, bt


def transe_step(ent, rel, bh, br, bt, batch, neg_ent, p_norm, norm_flag, margin, adv_temperature=None, regul_rate=0.0,
                out=None, score=None, occ_ent=None, check=True):
    """Forward, loss and backward of one batch in one launch (gv_transe_step).  Returns (g_ent (2 + neg_ent) * batch x dim,
    g_rel batch x dim, loss_part [batch]): one gradient row per occurrence, the loss = loss_part.sum() + margin.  ``occ_ent``
    (int32 [(2 + neg_ent) * batch], optional) receives the entity id of each g_ent row.  Every negative shares the positive's
    relation and one of its entities (the sampler's layout): the side whose id differs from the positive's is the corrupted one."""
    ent, rel = _table(ent, 'ent'), _table(rel, 'rel')
    if ent.shape[1] != rel.shape[1]:
        raise ValueError('ent / rel width mismatch')
    batch, neg_ent = int(batch), int(neg_ent)
    if batch < 1 or neg_ent < 1:
        raise ValueError(f'batch={batch} neg_ent={neg_ent}: need at least one positive and one negative each')
    n, dim = batch * (1 + neg_ent), ent.shape[1]
    bh, br, bt = _i32(bh, 'bh', n), _i32(br, 'br', n), _i32(bt, 'bt', n)
    if check:        # reads the ids back: callers under hipGraph capture pass check=False for ids made in range on the device
        for name, t, hi in (('bh', bh, ent.shape[0]), ('bt', bt, ent.shape[0]), ('br', br, rel.shape[0])):
            if int(t.min()) < 0 or int(t.max()) >= hi:
                raise ValueError(f'{name}: ids must lie in [0, {hi})')
    p_norm = _p_norm(p_norm)
    if adv_temperature is not None and not adv_temperature > 0:
        raise ValueError('adv_temperature must be > 0 (or None)')
    if out is None:
        out = (torch.empty((2 + neg_ent) * batch, dim, device=ent.device), torch.empty(batch, dim, device=ent.device),
               torch.empty(batch, device=ent.device))
    elif (tuple(_chk(out[0], name='g_ent').shape) != ((2 + neg_ent) * batch, dim) or tuple(_chk(out[1], name='g_rel').shape) != (batch, dim)
          or _chk(out[2], name='loss_part').numel() != batch):
        raise ValueError('out: (g_ent ((2 + neg_ent) batch, dim), g_rel (batch, dim), loss_part [batch])')
    if score is not None:
        score = _chk(score, name='score')
        if score.numel() != n:
            raise ValueError('score: batch * (1 + neg_ent) entries')
    if occ_ent is not None:
        occ_ent = _i32(occ_ent, 'occ_ent', (2 + neg_ent) * batch)
    lib.call('gv_transe_step', ptr(ent), ptr(rel), ptr(bh), ptr(br), ptr(bt), batch, neg_ent, dim, p_norm, int(bool(norm_flag)),
             float(margin), float(adv_temperature or 0.0), float(regul_rate), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(score),
             ptr(occ_ent), lib.stream())
    return out


class TransEOrder:
    """Buffers of the two occurrence orderings (entities, relations) gv_build_csr makes for the SGD launch, sized once (work
    items and fix-ups are 4 int32 each, as indices.KGraph carves them)."""

    def __init__(self, n_occ_e, n_ent, n_occ_r, n_rel, device, chunk=256):
        from .indices import _index_caps, _index_workspace
        self.parts = []
        for n_occ, n_seg in ((n_occ_e, n_ent), (n_occ_r, n_rel)):
            items_cap, fix_cap, _ = _index_caps(n_occ, n_seg, chunk)
            i32 = dict(dtype=torch.int32, device=device)
            self.parts.append(dict(n=n_occ, n_seg=n_seg, perm=torch.empty(n_occ, **i32), rowptr=torch.empty(n_seg + 1, **i32),
                                   items=torch.empty(4 * items_cap, **i32), items_cap=items_cap, fix=torch.empty(4 * fix_cap, **i32),
                                   fix_cap=fix_cap))
        self.ws, self.ws_bytes = _index_workspace(device, max(n_occ_e, n_occ_r), max(n_ent, n_rel))
        self.chunk = chunk

    def build(self, keys_e, keys_r):
        for p, keys in zip(self.parts, (keys_e, keys_r)):
            lib.call('gv_build_csr', ptr(keys), p['n'], p['n_seg'], self.chunk, ptr(p['perm']), ptr(p['rowptr']), ptr(p['items']),
                     p['items_cap'], ptr(p['fix']), p['fix_cap'], ptr(self.ws), self.ws_bytes, lib.stream())
        return self.parts


def transe_apply(ent, rel, g_ent, g_rel, order, lr, loss_part, margin, loss_out, epoch_acc=None):
    """p += -lr * g on the touched rows of both tables, occurrences summed in order (gv_transe_apply); ``order`` = the two
    ``TransEOrder`` parts after ``build``.  Writes loss_out[0] = loss_part.sum() + margin and adds it to epoch_acc (float64)."""
    ent, rel = _table(ent, 'ent'), _table(rel, 'rel')
    dim = ent.shape[1]
    if rel.shape[1] != dim or ent.device != rel.device:
        raise ValueError('ent / rel: same width and device')
    pe, pr = order
    g_ent, g_rel = _chk(g_ent, name='g_ent'), _chk(g_rel, name='g_rel')
    if pe['n_seg'] != ent.shape[0] or pr['n_seg'] != rel.shape[0]:
        raise ValueError(f'the orderings cover {pe["n_seg"]} entities / {pr["n_seg"]} relations, the tables hold '
                         f'{ent.shape[0]} / {rel.shape[0]} rows')
    if tuple(g_ent.shape) != (pe['n'], dim) or tuple(g_rel.shape) != (pr['n'], dim):
        raise ValueError(f'g_ent {tuple(g_ent.shape)} / g_rel {tuple(g_rel.shape)}: expected ({pe["n"]}, {dim}) / ({pr["n"]}, {dim}), '
                         'one row per ordered occurrence')
    loss_part, loss_out = _chk(loss_part, name='loss_part'), _chk(loss_out, name='loss_out')
    if loss_part.numel() < 1 or loss_out.numel() < 1:
        raise ValueError('loss_part and loss_out need at least one entry')
    for name, t in (('g_ent', g_ent), ('g_rel', g_rel), ('loss_part', loss_part), ('loss_out', loss_out)):
        if t.device != ent.device:
            raise ValueError(f'{name}: on {t.device}, the tables on {ent.device}')
    if epoch_acc is not None:
        epoch_acc = _chk(epoch_acc, torch.float64, 'epoch_acc')
        if epoch_acc.numel() < 1 or epoch_acc.device != ent.device:
            raise ValueError('epoch_acc: one float64 entry on the tables\' device')
    lib.call('gv_transe_apply', ptr(ent), ent.shape[0], ptr(g_ent), ptr(pe['perm']), ptr(pe['rowptr']), ptr(rel), rel.shape[0],
             ptr(g_rel), ptr(pr['perm']), ptr(pr['rowptr']), ent.shape[1], float(lr), ptr(loss_part), loss_part.numel(),
             float(margin), ptr(loss_out), ptr(epoch_acc), lib.stream())


TRANSE_OPT_METHODS = {'sgd': 0, 'adagrad': 1, 'adadelta': 2, 'adam': 3}      # = GV_TRANSE_OPT_* (include/gcnvae.h)


class TransEOptState:
    """What ``transe_apply_opt`` keeps between steps: two float32 arrays per table, shaped like the table (``ent`` / ``rel``:
    pairs (s1, s2) -- Adagrad: s1 = sum; Adadelta: square_avg, acc_delta; Adam: exp_avg, exp_avg_sq; SGD: unused), and ``t``, the
    number of steps taken, int64 [1] on the device."""

    def __init__(self, n_ent, n_rel, dim, device):
        self.ent = (torch.zeros(n_ent, dim, device=device), torch.zeros(n_ent, dim, device=device))
        self.rel = (torch.zeros(n_rel, dim, device=device), torch.zeros(n_rel, dim, device=device))
        self.t = torch.zeros(1, dtype=torch.int64, device=device)

    def tensors(self):
        return (*self.ent, *self.rel, self.t)

    def zero_(self):
        for x in self.tensors():
            x.zero_()
        return self

    def snapshot(self):
        """Copies of the four arrays and the step number (device tensors): what ``restore`` puts back."""
        return tuple(x.clone() for x in self.tensors())

    def restore(self, snap):
        """Put a ``snapshot`` back IN PLACE (every address stays what a captured step recorded)."""
        for x, s in zip(self.tensors(), snap):
            x.copy_(s)
        return self


def transe_apply_opt(ent, rel, g_ent, g_rel, order, method, lr, loss_part, margin, loss_out, epoch_acc=None, *, state,
                     weight_decay=0.0, lr_decay=0.0):
    """One optimiser step on both tables from the occurrence gradients, summed in order as ``transe_apply`` sums them
    (gv_transe_apply_opt): ``method`` 'sgd' | 'adagrad' | 'adadelta' | 'adam' (case-insensitive) is the rule of torch.optim at
    torch's defaults with the coupled ``weight_decay``; ``lr_decay`` is Adagrad's.  ``state`` (a ``TransEOptState``) is updated in
    place: its step number ``t`` is advanced by one on the stream first (a captured replay advances it too), then one launch
    reads it.  Under Adadelta, Adam or a non-zero weight_decay every row of both tables is updated (torch's dense semantics);
    otherwise rows without occurrences are not written.  Writes loss_out / epoch_acc as ``transe_apply`` does."""
    code = TRANSE_OPT_METHODS.get(method.lower()) if isinstance(method, str) else None
    if code is None:
        raise ValueError(f'method {method!r}: expected one of {sorted(TRANSE_OPT_METHODS)}')
    lr, weight_decay, lr_decay = float(lr), float(weight_decay), float(lr_decay)
    for name, x in (('lr', lr), ('weight_decay', weight_decay), ('lr_decay', lr_decay)):
        if not x >= 0.0:
            raise ValueError(f'{name} must be >= 0, got {x}')
    if lr_decay != 0.0 and code != TRANSE_OPT_METHODS['adagrad']:
        raise ValueError('lr_decay is Adagrad\'s: pass 0 with any other method')
    if not isinstance(state, TransEOptState):
        raise TypeError('state: a TransEOptState')
    for name, pair, table in (('state.ent', state.ent, ent), ('state.rel', state.rel, rel)):
        for i, x in enumerate(pair):
            if tuple(x.shape) != tuple(table.shape):
                raise ValueError(f'{name}[{i}]: shape {tuple(x.shape)}, the table {tuple(table.shape)}')
    ent, rel = _table(ent, 'ent'), _table(rel, 'rel')
    dim = ent.shape[1]
    if rel.shape[1] != dim or ent.device != rel.device:
        raise ValueError('ent / rel: same width and device')
    pe, pr = order
    g_ent, g_rel = _chk(g_ent, name='g_ent'), _chk(g_rel, name='g_rel')
    if pe['n_seg'] != ent.shape[0] or pr['n_seg'] != rel.shape[0]:
        raise ValueError(f'the orderings cover {pe["n_seg"]} entities / {pr["n_seg"]} relations, the tables hold '
                         f'{ent.shape[0]} / {rel.shape[0]} rows')
    if tuple(g_ent.shape) != (pe['n'], dim) or tuple(g_rel.shape) != (pr['n'], dim):
        raise ValueError(f'g_ent {tuple(g_ent.shape)} / g_rel {tuple(g_rel.shape)}: expected ({pe["n"]}, {dim}) / ({pr["n"]}, {dim}), '
                         'one row per ordered occurrence')
    loss_part, loss_out = _chk(loss_part, name='loss_part'), _chk(loss_out, name='loss_out')
    if loss_part.numel() < 1 or loss_out.numel() < 1:
        raise ValueError('loss_part and loss_out need at least one entry')
    for name, pair in (('state.ent', state.ent), ('state.rel', state.rel)):
        for i, x in enumerate(pair):
            _chk(x, name=f'{name}[{i}]')
    t = _chk(state.t, torch.int64, 'state.t')
    if t.numel() != 1:
        raise ValueError('state.t: one int64 entry')
    for name, x in (('g_ent', g_ent), ('g_rel', g_rel), ('loss_part', loss_part), ('loss_out', loss_out), ('state.ent', state.ent[0]),
                    ('state.ent', state.ent[1]), ('state.rel', state.rel[0]), ('state.rel', state.rel[1]), ('state.t', t)):
        if x.device != ent.device:
            raise ValueError(f'{name}: on {x.device}, the tables on {ent.device}')
    if epoch_acc is not None:
        epoch_acc = _chk(epoch_acc, torch.float64, 'epoch_acc')
        if epoch_acc.numel() < 1 or epoch_acc.device != ent.device:
            raise ValueError('epoch_acc: one float64 entry on the tables\' device')
    t.add_(1)         # on the stream, ahead of the launch that reads it: part of a captured step
    lib.call('gv_transe_apply_opt', ptr(ent), ent.shape[0], ptr(g_ent), ptr(pe['perm']), ptr(pe['rowptr']), ptr(rel), rel.shape[0],
             ptr(g_rel), ptr(pr['perm']), ptr(pr['rowptr']), dim, code, lr, weight_decay, lr_decay, ptr(state.ent[0]),
             ptr(state.ent[1]), ptr(state.rel[0]), ptr(state.rel[1]), ptr(t), ptr(loss_part), loss_part.numel(), float(margin),
             ptr(loss_out), ptr(epoch_acc), lib.stream())


def transe_queries(ent, rel=None, a=None, r=None, head=False, norm_flag=True):
    """q[i] = n(ent[a[i]]) + n(rel[r[i]]) (tail queries), n(ent[a[i]]) - n(rel[r[i]]) (head queries); without ``rel`` the
    normalised table n(ent) (gv_transe_queries)."""
    ent = _table(ent, 'ent')
    dim = ent.shape[1]
    if rel is None:
        m = ent.shape[0]
    else:
        rel = _table(rel, 'rel')
        if rel.shape[1] != dim:
            raise ValueError('ent / rel width mismatch')
        a = a.to(device=ent.device, dtype=torch.int32).contiguous()
        r = r.to(device=ent.device, dtype=torch.int32).contiguous()
        m = a.numel()
        if r.numel() != m:
            raise ValueError('one relation per query')
        if m and (int(a.min()) < 0 or int(a.max()) >= ent.shape[0] or int(r.min()) < 0 or int(r.max()) >= rel.shape[0]):
            raise ValueError('query ids out of range')
    q = torch.empty(m, dim, dtype=torch.float32, device=ent.device)
    lib.call('gv_transe_queries', ptr(ent), ptr(rel), ptr(a), ptr(r), m, dim, int(bool(head)), int(bool(norm_flag)), ptr(q),
             lib.stream())
    return q


def transe_distances(q, en, p_norm):
    """(m, v) = ||q[i] - en[j]||_p, materialised (gv_transe_distances): the fused ranker's distances, bit for bit."""
    q, en = _table(q, 'q'), _table(en, 'entities')
    if q.shape[1] != en.shape[1]:
        raise ValueError('q / entities width mismatch')
    p_norm = _p_norm(p_norm)
    out = torch.empty(q.shape[0], en.shape[0], dtype=torch.float32, device=q.device)
    lib.call('gv_transe_distances', ptr(q), q.shape[0], ptr(en), en.shape[0], q.shape[1], p_norm, ptr(out), lib.stream())
    return out


def _transe_operands(q, en):
    """The two tables of a TransE query, of one width."""
    q, en = _table(q, 'q'), _table(en, 'entities')
    if q.shape[1] != en.shape[1]:
        raise ValueError('q / entities width mismatch')
    return q, en


def transe_rank_filtered(q, en, target, p_norm, filt_lo=None, filt_hi=None, filt_ent=None):
    """(raw, filtered) 0-based mid-ranks of ``target[i]`` under score = -||q[i] - en[j]||_p -- ``ranking.sort_and_rank`` on
    ``transe_distances`` bit for bit -- without the distance matrix (gv_transe_rank_filtered).  The filter ranges are
    ``rank_scores_filtered``'s; without them the filtered rank equals the raw one."""
    return _transe_rank('gv_transe_rank_filtered', q, en, target, p_norm, (filt_lo, filt_hi, filt_ent))


def _transe_rank(entry, q, en, target, p_norm, filt, cand=None):
    """The two ``transe_rank_*`` wrappers, with ``_rank_scores``' ``filt`` and ``cand``: the checks, the counts and the call.  One
    rank tensor per count the entry takes; the constrained entry leaves the filtered ones unwritten without a filter (None)."""
    q, en = _transe_operands(q, en)
    p_norm = _p_norm(p_norm)
    m, v = q.shape[0], en.shape[0]
    tgt32 = _target_args(target, m, v, q.device)
    lo32, hi32, ent32, _ = _filter_args(*filt, m, v, q.device)
    sets = () if cand is None else _cand_args(*cand, m, v, q.device)
    counts = torch.zeros(2 if cand is None else 4, max(m, 1), dtype=torch.int32, device=q.device)
    given = cand is None or lo32 is not None
    set_args = () if cand is None else (ptr(sets[0]), sets[1], sets[2], ptr(sets[3]))
    count_args = [ptr(c) if given or i % 2 == 0 else None for i, c in enumerate(counts)]
    lib.call(entry, ptr(q), m, ptr(en), v, q.shape[1], p_norm, ptr(tgt32), ptr(lo32), ptr(hi32), ptr(ent32), *set_args, *count_args,
             lib.stream())
    return _ranks(counts, m, given)


def transe_topk(q, en, k, p_norm, filt_lo=None, filt_hi=None, filt_ent=None):
    """The ``k`` nearest entities of every query row under ``||q[i] - en[j]||_p`` -- ``transe_distances``' distances bit for bit
    -- from one fused launch pair (gv_transe_topk) that never stores the distance matrix.  With a filter (as
    ``transe_rank_filtered`` takes it) the ids ``filt_ent[filt_lo[i]:filt_hi[i]]`` are no candidates of row i.  Order: distance
    ascending, equal distances by lower id, NaN after everything (+inf included).  Returns ``(ids int64 (m, k), dist float32
    (m, k))``; rows with fewer than k candidates are padded with id -1, distance +inf.  A zero distance is reported as +0 and
    every NaN as the one quiet NaN (``transe.topk_from_distances`` does the same)."""
    return _transe_topk('gv_transe_topk', q, en, k, p_norm, (filt_lo, filt_hi, filt_ent))


def _transe_topk(entry, q, en, k, p_norm, filt, cand=None):
    """The two ``transe_topk*`` wrappers, with ``_transe_rank``'s arguments: the checks, the outputs, the workspace and the call.
    Returns (ids int64 (m, k), dist float32 (m, k))."""
    q, en = _transe_operands(q, en)
    if q.device != en.device:
        raise ValueError(f'q on {q.device}, entities on {en.device}')
    p_norm = _p_norm(p_norm)
    k = _topk_arg(k)
    m, v = q.shape[0], en.shape[0]
    if v < 1:
        raise ValueError('need at least one entity')
    lo32, hi32, ent32, n_ent = _filter_args(*filt, m, v, q.device)
    sets = () if cand is None else _cand_args(*cand, m, v, q.device)
    ids = torch.empty(m, k, dtype=torch.int64, device=q.device)
    dist = torch.empty(m, k, dtype=torch.float32, device=q.device)
    if m == 0:
        return ids, dist
    ws = torch.empty(int(lib.load().gv_transe_topk_workspace_bytes(m, v, k)), dtype=torch.uint8, device=q.device)
    set_args = () if cand is None else (ptr(sets[0]), sets[1], sets[2], ptr(sets[3]))
    lib.call(entry, ptr(q), m, ptr(en), v, q.shape[1], p_norm, ptr(lo32), ptr(hi32), ptr(ent32), n_ent, *set_args, k, ptr(ids),
             ptr(dist), ptr(ws), lib.stream())
    return ids, dist


def transe_rank_constrained(q, en, target, p_norm, cand, cand_set, filt_lo=None, filt_hi=None, filt_ent=None):
    """(raw, filtered, raw_constrained, filtered_constrained) 0-based mid-ranks of ``target[i]`` under score =
    -||q[i] - en[j]||_p (gv_transe_rank_constrained): ``transe_rank_filtered``'s two, bit for bit, and the same over the members
    of row ``cand_set[i]`` of the bitmask ``cand`` (as ``rank_scores_constrained`` takes it).  Without a filter the two filtered
    ranks are None."""
    return _transe_rank('gv_transe_rank_constrained', q, en, target, p_norm, (filt_lo, filt_hi, filt_ent), (cand, cand_set))


def transe_topk_constrained(q, en, k, p_norm, cand, cand_set, filt_lo=None, filt_hi=None, filt_ent=None):
    """``transe_topk`` among the members of a per-query candidate set only (gv_transe_topk_constrained): the candidates of row i
    are the entities whose bit is set in row ``cand_set[i]`` of the bitmask ``cand`` (as ``rank_scores_constrained`` takes it),
    less the filter-listed ids.  Order and padding are ``transe_topk``'s."""
    return _transe_topk('gv_transe_topk_constrained', q, en, k, p_norm, (filt_lo, filt_hi, filt_ent), (cand, cand_set))


def transe_entity_topk(ents, en, rn, k, p_norm, head=False, filt_lo=None, filt_hi=None, filt_ent=None, exclude_self=True, span=None):
    """Per-entity completion for TransE: for every query entity ``a = ents[i]`` the ``k`` nearest pairs (r, x) over ALL relations
    under ``d[i, r, x] = ||(en[a] + rn[r]) - en[x]||_p`` (``head``: ``en[a] - rn[r]``, the facts (x, r, a)) -- bit for bit
    ``transe_distances(transe_queries(ent, rel, a, r, head), en, p_norm)``, the distances ``transe_topk`` selects on -- from one
    fused launch pair (gv_transe_entity_topk) that keeps one sorted list per entity while the relations are walked: no (entity x
    relation) query matrix, no per-relation results.  ``en`` / ``rn`` are the normalised tables (``transe_queries(table,
    norm_flag=...)``).  With a filter (one range per key ``a * R + r``, N * R of them: ``ranking._mine_filter`` builds it) the ids
    ``filt_ent[filt_lo[a * R + r]:filt_hi[a * R + r]]`` are no candidates under relation r, nor is ``x == a`` with
    ``exclude_self``.  Order: distance ascending, then relation, then entity ascending; NaN after everything (+inf included).
    ``ents`` may repeat and need not be sorted.  ``span``: (relation, 64-entity tile) pairs per workgroup instead of the library's
    rule -- the result does not depend on it.  Returns ``(rel int64 (m, k), other int64 (m, k), dist float32 (m, k))``, padded
    with -1 / -1 / +inf past a row's last candidate; a zero distance is reported as +0 and every NaN as the one quiet NaN."""
    return _transe_entity_topk('gv_transe_entity_topk', ents, en, rn, k, p_norm, head, (filt_lo, filt_hi, filt_ent), exclude_self, span)


def transe_entity_topk_typed(ents, en, rn, k, p_norm, set_ptr, set_ids, head=False, filt_lo=None, filt_hi=None, filt_ent=None,
                             exclude_self=True, span=None):
    """``transe_entity_topk`` among the TYPE-CORRECT facts only (gv_transe_entity_topk_typed), with the member lists of
    ``entity_topk_scores_typed``.  ``head=False``: the facts (a, r, x) at ``||en[a] + rn[r] - en[x]||_p``, a among r's subjects
    and x among its objects; ``head=True``: the facts (x, r, a) at ``||en[a] - rn[r] - en[x]||_p``, a among r's objects and x
    among its subjects.  The distances bit for bit, order, ties, NaN, padding and the outputs are ``transe_entity_topk``'s; the
    filter is independent of the sets.  One fused launch pair walks the relations' candidate lists, 64 members a tile.  An entity
    on the query side of no relation gets an all-padding row.  ``span``: (relation, 64-member tile) pairs per workgroup -- the
    result does not depend on it."""
    return _transe_entity_topk('gv_transe_entity_topk_typed', ents, en, rn, k, p_norm, head, (filt_lo, filt_hi, filt_ent), exclude_self,
                               span, (set_ptr, set_ids, 'o' if head else 's'))


def _transe_entity_topk(entry, ents, en, rn, k, p_norm, head, filt, exclude_self, span, typed=None):
    """The two ``transe_entity_topk*`` wrappers, with ``_entity_topk``'s ``filt`` and ``typed``: the checks in their one order, the
    outputs, the workspace and the call.  Returns (rel int64 (m, k), other int64 (m, k), dist float32 (m, k))."""
    m, n, num_rels, dim = _entity_topk_operands(ents, en, rn)
    k = _topk_arg(k)
    p_norm = _p_norm(p_norm)
    if dim > TRANSE_MAX_DIM:
        raise ValueError(f'en / rn: width {dim} above {TRANSE_MAX_DIM}')
    (lo32, hi32, ent32, n_ent), (rel, other, dist), ents32 = _entity_topk_args(
        ents, span, 'entity' if typed is None else 'member', filt, m, n, num_rels, k, torch.int64, en.device)
    en, rn = _table(en.contiguous(), 'en'), _table(rn.contiguous(), 'rn')
    dev = en.device
    if rn.device != dev:
        raise ValueError(f'en on {dev}, rn on {rn.device}')
    if typed is None:
        span_tiles, lists = _entity_span_tiles(span, num_rels * ((n + 63) // 64)), ()
    else:
        ptr64, ids32, tile_ptr, n_tiles, cand_base, span_tiles = _entity_topk_typed_args(*typed, span, n, num_rels, dev)
        lists = (ptr(ptr64), ptr(ids32), ptr(tile_ptr), n_tiles, cand_base)
    if m == 0:
        return rel, other, dist
    if typed is None:
        ws_bytes = int(lib.load().gv_transe_entity_topk_workspace_bytes(m, n, num_rels, k, span_tiles))
    else:
        ws_bytes = int(lib.load().gv_transe_entity_topk_typed_workspace_bytes(m, n_tiles, k, span_tiles))
    ws =torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    lib.call(entry, ptr(ents32), m, ptr(en), ptr(rn), n, num_rels, dim, int(bool(head)), p_norm, ptr(lo32), ptr(hi32), ptr(ent32), n_ent,
             *lists, int(bool(exclude_self)), k, span_tiles, ptr(rel), ptr(other), ptr(dist), ptr(ws), ws_bytes, lib.stream())
    return rel, other, dist


def transe_pair_relations(en, rn, s, o, p_norm, *, target=None, k=0, filt_lo=None, filt_hi=None, filt_rel=None, cand=None,
                          ids_checked=False):
    """Relation prediction for TransE: ``pair_relation_scores`` on distances, smaller is better (gv_transe_pair_rel, one launch, no
    workspace).  ``d[i, r] = ||(en[o_i] - en[s_i]) - rn[r]||_p`` on the dense tables ``transe_entity_topk`` takes -- bit for bit
    ``transe_distances(en[o] - en[s], rn, p_norm)``; in exact arithmetic the triplet's ``||n(s) + n(r) - n(o)||``, but NOT the bit
    pattern ``transe_topk`` reports for the same triplet, which associates the operands the other way.  Ranks follow
    ``transe_rank_filtered``'s rule, the top-k ``transe_topk``'s order (distance ascending, equal distances by lower id, NaN after
    +inf), padded with id -1 / distance +inf.  ``ids_checked``, ``cand`` (gv_transe_pair_rel_constrained: the type-correct
    relations of each pair, four ranks, the narrowed list) and the returned ``(ranks, topk)`` are ``pair_relation_scores``'."""
    m, n, num_rels, dim, k, tgt32, (lo32, hi32, rel32, n_rel) = _pair_args(en, rn, ('en', 'rn'), s, o, target, k,
                                                                           (filt_lo, filt_hi, filt_rel), p_norm, ids_checked)
    en, rn = _table(en.contiguous(), 'en'), _table(rn.contiguous(), 'rn')
    dev = en.device
    if rn.device != dev:
        raise ValueError(f'en on {dev}, rn on {rn.device}')
    sets = () if cand is None else _pair_cand_args(cand, n, num_rels, dev)
    tgt, counts, ids, dist = _pair_buffers(m, k, tgt32 is not None, torch.int64, dev, 2 if cand is None else 4)
    given = lo32 is not None
    if m:
        s32, o32 = (t.to(device=dev, dtype=torch.int32).contiguous() for t in (s, o))
        c = _pair_count_ptrs(counts, given)
        lib.call('gv_transe_pair_rel' if cand is None else 'gv_transe_pair_rel_constrained', ptr(en), ptr(rn), n, num_rels, dim, int(p_norm),
                 ptr(s32), ptr(o32), ptr(tgt32), ptr(lo32), ptr(hi32), ptr(rel32), n_rel, *((ptr(sets[0]),) + sets[1:] if sets else ()), k,
                 ptr(tgt), *c[:4 if sets else 2], ptr(ids), ptr(dist), m, lib.stream())
    return _pair_result(counts, m, given, k, ids, dist)


def transe_mine(en, rn, p_norm, *, k=None, threshold=None, filt_lo=None, filt_hi=None, filt_ent=None, exclude_self=True,
                max_results=MINE_MAX_RESULTS):
    """Mine ALL triplets of a TransE model: ``d[s, r, o] = ||(en[s] + rn[r]) - en[o]||_p`` over every (s, r, o), bit for bit
    ``transe_distances`` on the tail queries ``transe_queries`` makes of (s, r); ``en`` / ``rn`` are the normalised tables
    (``transe_queries(table, norm_flag=...)``).  Candidates: every triplet, less the filter's (key ``s * R + r`` ->
    ``filt_ent[filt_lo[key]:filt_hi[key]]``), less s == o when ``exclude_self``, less NaN distances (+inf is one) -- without storing
    a distance (gv_transe_mine: a workgroup keeps a subject and an object tile of ``en`` in LDS and walks the relations).
    ``threshold=t``: every candidate with d <= t (a negative t: none); ``k=K``: the K nearest.  Order: distance ascending, then
    (s, r, o).  Returns ``(triplets int64 (n, 3), distances float32 (n,), info)``; ``info['count']``, ``info['passes']`` and
    ``MineOverflow`` as in ``mine_scores``, with "at or below the distance" for "at or above the logit"."""
    return _transe_mine('gv_transe_mine', en, rn, p_norm, None, k, threshold, filt_lo, filt_hi, filt_ent, exclude_self, max_results)


def _transe_mine_tables(en, rn, p_norm, members, filt_lo, filt_hi, filt_ent):
    """What every TransE mining wrapper checks and prepares of its tables: the member lists (checked before the tables are made
    contiguous), the two tables of one width, the norm, at least one relation, the sizes and the filter's shape.  Returns ``(en, rn,
    p_norm, members, device, the empty mining result when there is no entity or else None)``."""
    if members is not None:
        for name, t in (('en', en), ('rn', rn)):
            if not isinstance(t, torch.Tensor) or t.dim() != 2:
                raise TypeError(f'{name}: expected a 2-D tensor')
        members = _mine_typed_members(members[0], members[1], en.shape[0], rn.shape[0]) + (members[2],)
    en, rn = _mine_tables(en, 'en', rn, 'rn', prepare=lambda t, name: _table(t.contiguous(), name))
    p_norm = _p_norm(p_norm)
    if rn.shape[0] < 1:
        raise ValueError('need at least one relation')
    _mine_sizes(en.shape[0], rn.shape[0], filt_lo, filt_hi, filt_ent)
    dev, nothing = _mine_device(en, 'en', rn, 'rn')
    return en, rn, p_norm, members, dev, nothing


def _transe_mine(entry, en, rn, p_norm, members, k, threshold, filt_lo, filt_hi, filt_ent, exclude_self, max_results):
    """``transe_mine`` (``members`` None) and ``transe_mine_typed`` (``members`` = (set_ptr, set_ids, span)), as ``_mine_scores`` is
    both DistMult miners; the member lists are checked before the tables are made contiguous."""
    k, threshold, max_results = _mine_args(k, threshold, max_results)
    en, rn, p_norm, members, dev, nothing = _transe_mine_tables(en, rn, p_norm, members, filt_lo, filt_hi, filt_ent)
    n, num_rels, dim = en.shape[0], rn.shape[0], en.shape[1]
    if nothing is not None:
        return nothing
    lists = _mine_lists(members, 4, (filt_lo, filt_hi, filt_ent), n, num_rels, dev, lib.load().gv_transe_mine_workspace_bytes)
    if lists is None:
        return _mine_empty(dev)
    lists, workspace, _held = lists      # _held: the tensors behind the addresses, alive until this frame returns

    def launch(mode, key_min, prefix_bits, prefix, bin_bits, out, capacity, words):
        lib.call(entry, ptr(en), ptr(rn), n, num_rels, dim, p_norm, *lists, 1 if exclude_self else 0, mode, key_min, prefix_bits,
                 prefix, bin_bits, ptr(out), capacity, ptr(words), ptr(words), *workspace, lib.stream())

    # d <= t is key(-d) >= key(-t); t = -0 keys as +0, the key of every zero distance
    return _mine_drive(launch, dev, n, num_rels, k, threshold, None if k is not None else mine_key(-threshold), max_results, True,
                       entry)


def transe_mine_typed(en, rn, p_norm, set_ptr, set_ids, *, k=None, threshold=None, filt_lo=None, filt_hi=None, filt_ent=None,
                      exclude_self=True, max_results=MINE_MAX_RESULTS, span=None):
    """``transe_mine`` among the TYPE-CORRECT triplets only: ``s`` a member of set ``R + r``, ``o`` a member of set ``r``, the sets
    given as lists (``set_ptr`` int64 [2 R + 1], ``set_ids``: ``ranking.TypeConstraint.members``), checked as ``mine_scores_typed``
    checks them.  Distances bit for bit, filter, ``exclude_self``, NaN, order, ``info`` and ``MineOverflow`` are ``transe_mine``'s.
    gv_transe_mine_typed: a workgroup takes a relation, a 64-member tile of its subject list and ``span`` tiles of its object list,
    four at a time (``mine_typed_plan``; the result does not depend on ``span``).  An empty plan returns the empty result without
    a launch."""
    return _transe_mine('gv_transe_mine_typed', en, rn, p_norm, (set_ptr, set_ids, span), k, threshold, filt_lo, filt_hi, filt_ent,
                        exclude_self, max_results)


# ---- per-relation completion for TransE: every relation's own K nearest -------------------------------------------------------------
def _transe_relation_topk(entry, levels, en, rn, k, p_norm, relations, members, filt_lo, filt_hi, filt_ent, exclude_self, max_results):
    """``transe_relation_topk`` (``members`` None) and ``transe_relation_topk_typed`` (``members`` = (set_ptr, set_ids, span)), as
    ``_relation_topk`` is the DistMult pair: ``_transe_mine``'s checks and tables, the slots, one launch closure,
    ``_mine_drive_by_relation`` on the keys of -d."""
    _mine_tables(en, 'en', rn, 'rn')
    if rn.shape[0] < 1:
        raise ValueError('need at least one relation')
    rels = relation_ids_check(relations, rn.shape[0])
    m = rels.numel()
    k, max_results, share = _relation_args(k, m, max_results)
    if (m << max(b for _, b in levels)) > MINE_RELATION_HIST_WORDS:
        raise ValueError(f'{m} relations: more than {MINE_RELATION_HIST_WORDS} histogram words; ask for them in several calls')
    en, rn, p_norm, members, dev, nothing = _transe_mine_tables(en, rn, p_norm, members, filt_lo, filt_hi, filt_ent)
    n, num_rels, dim = en.shape[0], rn.shape[0], en.shape[1]
    rels = rels.to(dev)
    info = {'count': torch.zeros(m, dtype=torch.int64, device=dev), 'passes': 0}
    padding = (torch.full((m, k), -1, dtype=torch.int64, device=dev), torch.full((m, k), -1, dtype=torch.int64, device=dev),
               torch.full((m, k), float('inf'), dtype=torch.float32, device=dev), info)
    if nothing is not None:
        return padding
    if members is None:
        lo32, hi32, ent32, n_ent, ws, ws_bytes = _mine_filter_args(filt_lo, filt_hi, filt_ent, n, num_rels, dev,
                                                                   lib.load().gv_transe_mine_workspace_bytes)
        sets, after = (), (ptr(ws), ws_bytes)
    else:
        set_ptr, set_ids = members[0].to(dev), members[1].to(dev)
        units = relation_typed_plan(set_ptr, num_rels, rels, members[2], multiple=4)
        if units.shape[0] == 0:
            return padding
        lo32, hi32, ent32, n_ent = _mine_typed_filter_args(filt_lo, filt_hi, filt_ent, n, num_rels, dev)
        sets, after = (ptr(set_ptr), ptr(set_ids), ptr(units), units.shape[0]), ()

    def launch(mode, rels32, key_min, prefix_bits, prefix, bin_bits, out, capacity, out_base, words):
        lib.call(entry, ptr(en), ptr(rn), n, num_rels, dim, p_norm, *sets, ptr(lo32), ptr(hi32), ptr(ent32), n_ent,
                 1 if exclude_self else 0, mode, ptr(rels32), m, ptr(key_min), prefix_bits, ptr(prefix), bin_bits, ptr(out), capacity,
                 ptr(out_base), ptr(words), ptr(words), *after, lib.stream())

    return _mine_drive_by_relation(launch, dev, n, rels, k, share, levels, entry, ascending=True)


def transe_relation_topk(en, rn, k, p_norm, *, relations=None, filt_lo=None, filt_hi=None, filt_ent=None, exclude_self=True,
                         max_results=MINE_MAX_RESULTS):
    """Every relation's OWN ``k`` nearest triplets of a TransE model: for each relation r of ``relations`` (unique ids, any order;
    None: all) the k candidates (s, o) of smallest ``d[s, r, o] = ||(en[s] + rn[r]) - en[o]||_p``, ``transe_mine``'s distance bit
    for bit and its candidates -- all (s, o) less the filter's triplets of r, less s == o under ``exclude_self``, less NaN (+inf is
    a candidate); ``en`` / ``rn`` are the normalised tables.  ``transe_mine`` walks to ONE distance for the whole graph, which the
    relations with short translation vectors fill; here thresholds, prefixes, histograms, counters and output segments are per
    relation (gv_transe_mine_by_relation: the miner's loop order over the chosen relations only, four slots in flight, each with
    its own early-exit bound and 256-bin histogram), so all lists come out of the same two to five sweeps and a few relations cost
    their share of a sweep.  Returns ``(subj int64 (m, k), obj int64 (m, k), dist float32 (m, k), info)``, row i for
    ``relations[i]`` in ``relation_select(ascending=True)``'s order -- distance ascending, then (s, o) --, short rows padded with
    -1 / -1 / +inf; ``info['count']`` int64 [m] is each relation's candidates at or below its K-th distance, ``info['passes']`` the
    sweeps.  ``m * k <= max_results``; a relation may return ``max_results // m`` records, and one whose candidates at or below its
    K-th distance are more raises ``MineOverflow`` naming it."""
    return _transe_relation_topk('gv_transe_mine_by_relation', MINE_RELATION_LEVELS, en, rn, k, p_norm, relations, None, filt_lo,
                                 filt_hi, filt_ent, exclude_self, max_results)


def transe_relation_topk_typed(en, rn, k, p_norm, set_ptr, set_ids, *, relations=None, filt_lo=None, filt_hi=None, filt_ent=None,
                               exclude_self=True, max_results=MINE_MAX_RESULTS, span=None):
    """``transe_relation_topk`` among the TYPE-CORRECT pairs only: s a member of set ``R + r``, o a member of set ``r``
    (``transe_mine_typed``'s member lists and rule, the same distances bit for bit).  gv_transe_mine_typed_by_relation walks
    ``relation_typed_plan``'s units -- the chosen relations' tiles only, four object tiles at a time; the result does not depend on
    ``span`` -- and keeps the typed miner's 12 + 10 + 10 histogram levels, a unit's workgroup owning one relation.  A relation with
    an empty subject or object list returns an all-padding row."""
    return _transe_relation_topk('gv_transe_mine_typed_by_relation', MINE_RELATION_TYPED_LEVELS, en, rn, k, p_norm, relations,
                                 (set_ptr, set_ids, span), filt_lo, filt_hi, filt_ent, exclude_self, max_results)
