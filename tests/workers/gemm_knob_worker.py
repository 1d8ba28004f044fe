"""Launched by tests/test_gpu_gemm.py, once per tile knob setting (GV_GEMM_NT / GV_GEMM_BK / GV_GEMM_MT in the environment: the
library reads them once per process).  Runs the small-shape grid of that file -- every layout x epilogue x split, with and
without a ReLU mask -- against the float64 reference and its bound; prints the worst |got - ref| / bound as one JSON line.
Any miss raises (non-zero exit)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch                                   # noqa: E402

import test_gpu_gemm as T                      # noqa: E402
from gcn_vae_amd import ops                    # noqa: E402


def main():
    assert torch.cuda.is_available()
    count = 0
    for m, n, k in T.SMALL:
        count += T.run_grid(ops, m, n, k, T.LAYOUTS, T.SPLITS, m + n + k, 'gv_gemm_f32 knob')
        mask = T._relu_mask(m, k, m + n + k)
        count += T.run_grid(ops, m, n, k, T.LAYOUTS, (1, 7), m + n + k, 'gv_gemm_f32 knob a_relu_mask',
                            epilogues=[T.EPILOGUES[0], T.EPILOGUES[-1]], mask=mask)
    knobs = {name: os.environ[name] for name in ('GV_GEMM_NT', 'GV_GEMM_BK', 'GV_GEMM_MT') if name in os.environ}
    print(f'{knobs}: {count} products checked')
    print(json.dumps(T.RATIOS))


if __name__ == '__main__':
    main()
