"""The host-side decisions of the layer-2 / loss-head seam fold (ops.EpilogueLink, ops.kl_seam_fold_ok), with CPU tensors standing
in for the device buffers: no kernel runs.  The fold is requested only when the float4-column KL backward would take it and
nothing else feeds dL/dh2; the layer skips its own epilogue gradient only for the very buffer the fold wrote, and raises when
another gradient reached it."""
import pytest
import torch


@pytest.fixture()
def ops(monkeypatch):
    from gcn_vae_amd import ops as _ops
    monkeypatch.setattr(_ops, 'KL_SEAM_FOLD', True)
    monkeypatch.delenv('GV_KL_BWD_V4', raising=False)
    return _ops


def link(ops, n=8, h=8, keep=True, bias_target=None):
    mask = torch.ones(n, 2 * h, dtype=torch.uint8) if keep else None
    return ops.EpilogueLink(mask, 1.25 if keep else 1.0, True, bias_target, 2 * h)


def test_fold_is_requested_only_where_the_column_backward_takes_it(ops, monkeypatch):
    some = torch.zeros(4)
    assert ops.kl_seam_fold_ok(link(ops), None, None, 8, 10)
    assert ops.kl_seam_fold_ok(link(ops, keep=False), None, None, 8, 1)            # dropout off is a folded case
    assert ops.kl_seam_fold_ok(link(ops, h=200), None, None, 200, 10) and ops.kl_seam_fold_ok(link(ops, h=500), None, None, 500, 10)
    assert not ops.kl_seam_fold_ok(None, None, None, 8, 10)                        # nobody offered a link
    assert not ops.kl_seam_fold_ok(link(ops), some, None, 8, 10)                   # z_mean has another consumer
    assert not ops.kl_seam_fold_ok(link(ops), None, some, 8, 10)                   # z_sigma has another consumer
    assert not ops.kl_seam_fold_ok(link(ops), None, None, 8, 12)                   # k > 10: the lane-per-column form runs
    assert not ops.kl_seam_fold_ok(link(ops), None, None, 8, 11)
    assert not ops.kl_seam_fold_ok(link(ops, h=6), None, None, 6, 10)              # h % 4 != 0
    assert not ops.kl_seam_fold_ok(link(ops, h=1028), None, None, 1028, 2)         # wider than the column form covers
    assert not ops.kl_seam_fold_ok(link(ops, h=16), None, None, 8, 10)             # a mask of another width
    buf = torch.zeros(64)
    off = buf[1:9]
    assert off.data_ptr() % 16 != 0 and not ops.kl_seam_fold_ok(link(ops), None, None, 8, 10, (buf, None, off))
    assert ops.kl_seam_fold_ok(link(ops), None, None, 8, 10, (buf, None))
    odd = link(ops)
    odd.keep = torch.ones(8 * 16 + 1, dtype=torch.uint8)[1:].view(8, 16)          # a mask that is not 4-byte aligned
    assert not ops.kl_seam_fold_ok(odd, None, None, 8, 10)
    monkeypatch.setenv('GV_KL_BWD_V4', '0')                                        # the column form switched off
    assert not ops.kl_seam_fold_ok(link(ops), None, None, 8, 10)
    monkeypatch.delenv('GV_KL_BWD_V4')
    monkeypatch.setattr(ops, 'KL_SEAM_FOLD', False)                                # the switch
    assert not ops.kl_seam_fold_ok(link(ops), None, None, 8, 10)


def test_layer_takes_only_the_folded_buffer(ops):
    ln = link(ops)
    assert ln.take(torch.zeros(8, 16)) is None                                     # nothing folded: the layer runs its own pass
    buf, bias = torch.randn(8, 16), torch.randn(16)
    ln.record(buf, bias)
    g, gb = ln.take(buf)
    assert g is buf and gb is bias and ln.buf is None and ln.take(buf) is None     # consumed once
    ln.record(buf, None)
    with pytest.raises(RuntimeError, match='not that buffer'):
        ln.take(buf + 0.0)                                                         # another tensor (a sum of two gradients)
    ln.record(buf, None)
    with pytest.raises(RuntimeError, match='not that buffer'):
        ln.take(buf.view(16, 8))                                                   # same storage, another shape
    ln.record(buf, None)
    buf.add_(1.0)                                                                  # same storage, added to in place
    with pytest.raises(RuntimeError, match='not that buffer'):
        ln.take(buf)
    ln.record(buf, None)
    with pytest.raises(RuntimeError, match='not that buffer'):
        ln.take(None)


def test_autograd_hands_the_recorded_buffer_to_the_sole_producer(ops):
    """A stand-in producer / consumer pair under autograd: with one consumer the producer's backward receives the consumer's very
    buffer; with a second consumer of the same output autograd adds the two gradients and the producer refuses."""
    class Producer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, ln):
            ctx.ln = ln
            return x * 2.0

        @staticmethod
        def backward(ctx, grad_out):
            taken = ctx.ln.take(grad_out)
            seen.append(taken is not None)
            return (grad_out if taken is None else taken[0]) * 2.0, None

    class Consumer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, h2, ln):
            ctx.ln, ctx.shape = ln, h2.shape
            return h2.sum()

        @staticmethod
        def backward(ctx, g):
            buf = torch.full(ctx.shape, float(g))
            ctx.ln.record(buf, None)
            return buf, None

    seen = []
    x = torch.randn(8, 16, requires_grad=True)
    ln = link(ops)
    Consumer.apply(Producer.apply(x, ln), ln).backward()
    assert seen == [True] and torch.equal(x.grad, torch.full((8, 16), 2.0))
    ln = link(ops)
    h2 = Producer.apply(x, ln)
    with pytest.raises(RuntimeError, match='not that buffer'):
        (Consumer.apply(h2, ln) + (h2 * 3.0).sum()).backward()


def test_link_carries_the_direct_target_stamp(ops):
    """The bias gradient may go straight into an optimiser arena slice resolved in the layer's forward: like every direct target it
    is refused once the registry changed."""
    ln = link(ops, bias_target=torch.zeros(16))
    ops._verify_direct(ln)
    ops.DIRECT_EPOCH[0] += 1
    try:
        with pytest.raises(RuntimeError, match='gradient arena'):
            ops._verify_direct(ln)
    finally:
        ops.DIRECT_EPOCH[0] -= 1
