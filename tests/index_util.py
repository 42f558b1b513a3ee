"""What the GPU tests of the four index classes share (test_index_gpu.py, test_ivf_gpu.py, test_pq_gpu.py, test_ivfpq_gpu.py)."""
import numpy as np
import torch

from topk_ref import bits


def cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def same(got, want, what=''):
    """two (idx, vals) pairs, tensors or ndarrays: equal ids, equal value bits"""
    got = tuple(t.cpu().numpy() if torch.is_tensor(t) else t for t in got)
    want = tuple(t.cpu().numpy() if torch.is_tensor(t) else t for t in want)
    assert (got[0] == want[0]).all(), (what, np.argwhere(got[0] != want[0])[:5])
    assert (bits(got[1]) == bits(want[1])).all(), (what, np.argwhere(bits(got[1]) != bits(want[1]))[:5])
