#!/usr/bin/env python3
"""Generate tests/golden/transe.npz by IMPORTING THE REFERENCE's TransE baseline (baselines/transe: model, loss,
negative_sampling; not tester / trainer, which need OpenKE's Base.so and tqdm).  Runs only where the reference tree is present;
its root is the first argument or $GCNVAE_REFERENCE.  Only inputs and outputs are written.

    python tests/golden/make_golden_transe.py /path/to/reference

transe.npz, per case tag (p1_norm, p1_raw, p2_norm, p2_raw: p_norm x norm_flag, margin 5; adv: self-adversarial T = 1;
regul: regul_rate 0.5; tie: dyadic tables, no normalisation, a hinge tie p - n == -margin and a zero difference):
  <tag>.ent / .rel        initial tables              <tag>.bh / .br / .bt   batch (B positives, then neg_ent blocks of B)
  <tag>.cfg               [B, neg_ent, p_norm, norm_flag, margin, adv_temperature (0: none), regul_rate, lr]
  <tag>.score / .loss     NegativeSampling's scores and loss      <tag>.g_ent / .g_rel   table gradients
  <tag>.ent3 / .rel3      tables after 3 SGD steps (lr, the same batch)
  seed.ent / seed.rel     TransE(V, R, dim) initial tables under torch.manual_seed(0); state_keys: the state-dict keys
Entity 0 is an all-zero row and the head of positive 0 in every case.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('GCNVAE_REFERENCE')
if not REF or not os.path.isdir(os.path.join(REF, 'baselines', 'transe')):
    sys.exit('usage: make_golden_transe.py <reference root> (the directory holding baselines/transe)')
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
from baselines.transe.loss import MarginLoss  # noqa: E402
from baselines.transe.model import TransE  # noqa: E402
from baselines.transe.negative_sampling import NegativeSampling  # noqa: E402

V, R, DIM, B, K = 12, 4, 16, 4, 3


def batch(rs, head_first):
    """B positives (positive 0 has head 0, the zero row), K negatives each; one side replaced by a different entity."""
    h = rs.randint(1, V, B)
    h[0] = 0
    r, t = rs.randint(0, R, B), rs.randint(1, V, B)
    bh, br, bt = [h], [r], [t]
    for j in range(K):
        nh, nt = h.copy(), t.copy()
        for b in range(B):
            if (b + j + head_first) % 2:
                nh[b] = (h[b] + 1 + rs.randint(0, V - 1)) % V
            else:
                nt[b] = (t[b] + 1 + rs.randint(0, V - 1)) % V
        bh.append(nh); br.append(r.copy()); bt.append(nt)
    return [np.concatenate(x).astype(np.int64) for x in (bh, br, bt)]


def run(ent, rel, bh, br, bt, p_norm, norm_flag, margin, adv, regul, lr, steps):
    model = TransE(V, R, dim=DIM, p_norm=p_norm, norm_flag=norm_flag)
    with torch.no_grad():
        model.ent_embeddings.weight.copy_(torch.from_numpy(ent))
        model.rel_embeddings.weight.copy_(torch.from_numpy(rel))
    ns = NegativeSampling(model=model, loss=MarginLoss(adv_temperature=adv, margin=margin), batch_size=B, regul_rate=regul)
    opt = torch.optim.SGD(ns.parameters(), lr=lr)
    data = {'batch_h': torch.from_numpy(bh), 'batch_r': torch.from_numpy(br), 'batch_t': torch.from_numpy(bt), 'mode': 'normal'}
    out = {}
    for s in range(steps):
        opt.zero_grad()
        score = model(data)
        loss = ns(data)
        loss.backward()
        if s == 0:
            out['score'] = score.detach().numpy().copy()
            out['loss'] = np.float32(loss.item())
            out['g_ent'] = model.ent_embeddings.weight.grad.numpy().copy()
            out['g_rel'] = model.rel_embeddings.weight.grad.numpy().copy()
        opt.step()
    out['ent3'] = model.ent_embeddings.weight.detach().numpy().copy()
    out['rel3'] = model.rel_embeddings.weight.detach().numpy().copy()
    return out


def main():
    arrays = {}
    torch.manual_seed(0)
    seeded = TransE(V, R, dim=DIM, p_norm=1, norm_flag=True)
    sd = seeded.state_dict()
    arrays['seed.ent'] = sd['ent_embeddings.weight'].numpy().copy()
    arrays['seed.rel'] = sd['rel_embeddings.weight'].numpy().copy()
    arrays['state_keys'] = np.array(list(sd.keys()))
    cases = {'p1_norm': (1, True, 5.0, None, 0.0), 'p1_raw': (1, False, 5.0, None, 0.0), 'p2_norm': (2, True, 5.0, None, 0.0),
             'p2_raw': (2, False, 5.0, None, 0.0), 'adv': (1, True, 5.0, 1.0, 0.0), 'regul': (1, True, 5.0, None, 0.5),
             'tie': (1, False, None, None, 0.0)}
    for i, (tag, (p, nf, margin, adv, regul)) in enumerate(cases.items()):
        rs = np.random.RandomState(100 + i)
        torch.manual_seed(100 + i)
        m = TransE(V, R, dim=DIM, p_norm=p, norm_flag=nf)
        ent = m.ent_embeddings.weight.detach().numpy().copy()
        rel = m.rel_embeddings.weight.detach().numpy().copy()
        bh, br, bt = batch(rs, i)
        lr = 1.0 if nf else 0.1
        if tag == 'tie':
            # dyadic entries: every sum is exact in float32 in any order.  Positive 1 has t = h + r (a zero difference);
            # negative 0 of positive 0 is chosen with a larger distance, and the margin makes that pair an exact hinge tie.
            ent = (rs.randint(-8, 9, (V, DIM)) / 8.0).astype(np.float32)
            rel = (rs.randint(-8, 9, (R, DIM)) / 8.0).astype(np.float32)
            if bt[1] != bh[1]:
                ent[bt[1]] = ent[bh[1]] + rel[br[1]]
            ent[0] = 0.0
            d = lambda o: np.abs((ent[bh[o]] + rel[br[o]]) - ent[bt[o]]).sum(dtype=np.float32)  # noqa: E731
            head = bh[B] != bh[0]
            for cand in range(1, V):
                if head:
                    bh[B] = cand
                elif cand != bt[0]:
                    bt[B] = cand
                if d(B) > d(0):
                    break
            margin = float(d(B) - d(0))
            lr = 0.125
        ent[0] = 0.0
        res = run(ent, rel, bh, br, bt, p, nf, margin, adv, regul, lr, 3)
        arrays[f'{tag}.ent'], arrays[f'{tag}.rel'] = ent, rel
        arrays[f'{tag}.bh'], arrays[f'{tag}.br'], arrays[f'{tag}.bt'] = bh, br, bt
        arrays[f'{tag}.cfg'] = np.array([B, K, p, int(nf), margin, adv or 0.0, regul, lr], dtype=np.float64)
        for k, v in res.items():
            arrays[f'{tag}.{k}'] = v
    np.savez_compressed(os.path.join(HERE, 'transe.npz'), **arrays)
    print('wrote', os.path.join(HERE, 'transe.npz'), len(arrays), 'arrays')


if __name__ == '__main__':
    main()
