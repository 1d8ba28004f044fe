"""Launched once by tests/test_gpu_mmd.py with GV_MMD_ROWS16=0 in the environment (the library reads it once per process): runs
the aligned-width shapes of mmd_cases.FORM_SHAPES, which the default dispatch gives to the row-of-16 kernels, and one indexed
case on the lane-per-column kernels, against the same float64 references and bounds.  Any miss raises (non-zero exit); the worst
|got - ref| / bound of every comparison is printed as one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch                                   # noqa: E402

import mmd_cases as mc                         # noqa: E402
import test_gpu_mmd as T                       # noqa: E402
from gcn_vae_amd import ops                    # noqa: E402


def main():
    assert torch.cuda.is_available()
    assert os.environ.get(T.KNOB) == '0', f'{T.KNOB} must be 0 in this process'
    count = 0
    for sx, sy, h, scale in T.ALIGNED_WIDTH_CASES:
        fwd, bwd = mc.dispatch(h, rows16=False)
        assert 'g<' not in fwd and 'g<' not in bwd
        T.check_dense(ops, f'{fwd} {bwd} {sx}x{sy}x{h} {scale}', sx, sy, h, scale)
        count += 1
    fwd, bwd = mc.dispatch(200, rows16=False)
    T.check_indexed(ops, f'indexed {fwd} {bwd} 40x{mc.INDEX_PICKS}x200 n', 40, 200, 'n', True, 1.3)
    count += 1
    print(f'{T.KNOB}=0: {count} cases checked')
    print(json.dumps(T.RATIOS))


if __name__ == '__main__':
    main()
