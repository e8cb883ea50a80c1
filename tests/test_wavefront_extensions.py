"""Oracle side of tests/test_wavefront_extensions_gpu.py (no GPU): every seeded batch of tests/wv_ext_cases.py solves with
adaptive rho in the CPU oracle, and in each batch at least one problem changes rho -- so the GPU test of the adaptive
wavefront kernel cannot pass without a rho update, a park and a resume, and a later change of penalty_qp that took the
updates away would show here."""
import numpy as np
import pytest

import wv_ext_cases as wx


@pytest.mark.parametrize("shape,seed", wx.BATCHES, ids=wx.IDS)
def test_every_batch_solves_and_changes_rho_in_the_oracle(shape, seed):
    ref = wx.oracle_adaptive(shape, seed)
    assert np.all(ref[:, 0] == 1), ref
    assert (ref[:, 2] >= 1).any(), ref
    assert (ref[:, 2] == 0).any(), ref             # and one that keeps the initial rho: both paths of the update point


def test_the_batches_reach_four_instantiations_of_the_kernel():
    """<8,1,1,4>, <8,2,2,8>, <7,4,3,10> with run-time lanes per block (four) and <7,4,3,10,3> with three."""
    from test_wavefront_edges import wv_plan
    plans = []
    for shape, seed in wx.BATCHES:
        P, q, A, l, u = wx.build(shape, seed)[0][0]
        info = wv_plan(P, A)
        assert info[0] == 1, (shape, info)
        plans.append((info[4], info[5], info[6], info[7], 3 if info[3] == 3 and info[5] == 4 else 0))      # <BS, NS, NV, NSTEP, LPB>
    assert plans == [(8, 1, 1, 4, 0), (8, 2, 2, 8, 0), (7, 4, 3, 10, 0), (7, 4, 3, 10, 3)], plans
