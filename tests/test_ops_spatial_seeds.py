"""CPU: the seed of the fused-final cases of tests/test_gpu_ops_spatial.py.  The fp64 oracle on the fp32-rounded inputs and the same oracle evaluated in fp32 on the
CPU have to disagree on fewer derivative sides (BN outputs of the last block, sign of x_hat - x) than the cap the GPU test holds the device to (1e-5 x
pre-activations + 8): a device within the same round-off can then meet it too.  No GPU work, all four cases."""
import numpy as np
import pytest

from tests.test_gpu_ops_spatial import FIN_CASES, fin_forward, fin_inputs


@pytest.mark.parametrize('name', list(FIN_CASES))
def test_fused_final_seed_stays_under_the_flip_cap(name):
    t = fin_inputs(name)
    _, bn64, _, xh64 = fin_forward(t)
    _, bn32, _, xh32 = fin_forward(t, np.float32)
    flips = int(((bn64 > 0) != (bn32 > 0)).sum()) + int((np.sign(xh64 - t['x']) != np.sign(xh32 - t['x'].astype(np.float32))).sum())
    print(f'{name}: {flips} sides differ between fp64 and fp32 on the CPU (cap {1e-5 * bn64.size + 8:.0f})')
    assert flips <= 1e-5 * bn64.size + 8, flips
