"""Launched by tests/test_gpu_bdd.py, once per K1 knob setting (GV_K1_U, GV_K1_BPL1, GV_K1_LDS_U in the environment: the library
reads them once per process).  Runs the shapes whose kernels that knob changes against the float64 reference and its bound;
saves the outputs to the file named by argv[1] (for the parent's bit comparisons) and prints the worst |got - ref| / bound as
one JSON line.  Any miss raises (non-zero exit)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch                                   # noqa: E402

import test_gpu_bdd as T                       # noqa: E402
from gcn_vae_amd import ops                    # noqa: E402


def main():
    assert torch.cuda.is_available()
    kn = T.knob_of(os.environ)
    saved, count = {}, 0
    if kn['u']:
        for nb, p, q, t in T.U_SHAPES:
            key = str(T.agg_kernel(nb, p, q, t, u=kn['u']))
            saved[f'{nb}x{p}x{q}x{int(t)}'] = T.run_agg(ops, nb, p, q, t, seed=nb + 3 * p + 7 * q + t, key=key)
            count += len(T.EPILOGUES)
        for nb, p, q, t in T.U_PACK_SHAPES:
            key = str(T.agg_kernel(nb, p, q, t, packed=True, u=kn['u']))
            T.run_agg(ops, nb, p, q, t, seed=nb + p + q, packed=True, epilogues=T.EPILOGUES[:2], key=key)
            count += 2
    if kn['bpl1'] == 0:
        for nb, p, q, t in T.BPL1_SHAPES:
            key = str(T.agg_kernel(nb, p, q, t, bpl1=0))
            saved[f'{nb}x{p}x{q}x{int(t)}'] = T.run_agg(ops, nb, p, q, t, seed=nb + 3 * p + 7 * q + t, key=key)
            count += len(T.EPILOGUES)
    if kn['lds_u']:
        for nb, p, q, r, bf in T.LDS_RUNS:
            T.run_lds(ops, nb, p, q, r, bf, kn['lds_u'])
            count += 4
    torch.save(saved, sys.argv[1])
    print(f'{ {k: v for k, v in os.environ.items() if k in ("GV_K1_U", "GV_K1_BPL1", "GV_K1_LDS_U")} }: {count} launches checked')
    print(json.dumps(T.RATIOS))


if __name__ == '__main__':
    main()
