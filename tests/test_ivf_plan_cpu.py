"""The device planner of the inverted files, host side (no GPU): the numpy restatement (tests/ivf_plan_ref.py) against
loops over the definition, the library's new entries and the checks they make before anything is launched, and the host
bound of the scan's grid against the true workgroup count."""
import ctypes
import os
import re

import numpy as np
import pytest

import ivf_plan_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('col_off', 'pair_off', 'pair_q', 'pair_col', 'item_off', 'counts')


def _random_table(r, Q, nprobe, nlist, empty=0.0, distinct=True):
    """list_off with zero-length, one-row and several-tile lists; probe with distinct lists per query (as a search makes
    them) or any, a share `empty` of the slots -1"""
    lens = r.choice([0, 1, 31, 255, 256, 257, 700, 3000], nlist)
    list_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    if distinct:
        probe = np.stack([r.permutation(nlist)[:nprobe] for _ in range(Q)]).astype(np.int32).reshape(Q, nprobe)
    else:
        probe = r.randint(0, nlist, (Q, nprobe)).astype(np.int32)
    probe[r.rand(Q, nprobe) < empty] = -1
    return probe, list_off


@pytest.mark.parametrize('seed', range(12))
def test_restatement_is_the_definition(seed):
    r = np.random.RandomState(400 + seed)
    Q, nlist = r.randint(1, 40), r.randint(1, 12)
    nprobe = r.randint(1, nlist + 1)
    probe, list_off = _random_table(r, Q, nprobe, nlist, empty=(0.0, 0.2, 0.6)[seed % 3], distinct=seed % 2 == 0)
    if seed == 5:
        probe[0, 0] = nlist + 3           # outside [0, nlist): empty, as -1 is
    got, want = ivf_plan_ref.plan(probe, list_off), ivf_plan_ref.plan_brute(probe, list_off)
    for key in KEYS:
        assert got[key].dtype == np.int32 and got[key].shape == want[key].shape, key
        assert (got[key] == want[key]).all(), (key, got[key], want[key])


def test_restatement_small_cases_by_hand():
    """Two queries at two of three lists of 300, 0 and 40 rows, one slot empty."""
    t = ivf_plan_ref.plan(np.array([[2, 0], [0, -1]]), np.array([0, 300, 300, 340]))
    assert t['col_off'].tolist() == [[0, 40], [0, 300]]
    assert t['pair_off'].tolist() == [0, 2, 2, 3]                 # list 0: flat 1 and 2; list 2: flat 0; flat 3 is empty
    assert t['pair_q'].tolist() == [0, 1, 0, 1] and t['pair_col'].tolist() == [40, 0, 0, 300]
    assert t['item_off'].tolist() == [0, 2, 2, 3] and t['counts'].tolist() == [3, 340]
    t = ivf_plan_ref.plan(np.zeros((0, 4), np.int32), np.array([0, 5]))
    assert t['counts'].tolist() == [0, 0] and t['pair_off'].tolist() == [0, 0] and t['pair_q'].shape == (0,)


def test_library_exports_the_planner():
    from dirtorch_amd import _lib, ops
    lib = _lib.load()
    for name, nargs in (('dir_ivf_plan', 12), ('dir_ivf_plan_max_pairs', 0)):
        assert hasattr(lib, name), 'missing export ' + name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert lib.dir_ivf_plan_max_pairs() == ops.ivf_plan_max_pairs() >= 4096
    assert ops.ivf_plan_max_pairs() & (ops.ivf_plan_max_pairs() - 1) == 0       # the flat index takes whole bits of a key
    assert (65535 << 14 | ops.ivf_plan_max_pairs() - 1) < 1 << 31 and ops.ivf_plan_max_pairs() <= 1 << 14
    assert ops.ivf_scan_max_items() == lib.dir_launch_max_threads() // 768
    header = open(os.path.join(ROOT, 'include', 'dir_engine.h')).read()
    m = re.search(r'\nint dir_ivf_plan\((.*?)\);', header, re.S)
    assert m and len(m.group(1).split(',')) == 12
    assert 'int dir_ivf_plan_max_pairs(void);' in header
    assert '`items` may be ANY upper bound of item_off[nlist]' in header


def test_argument_errors_need_no_gpu():
    """DIR_ERR_INVALID (-1) before anything is launched: the pointers below are host memory no kernel may touch."""
    from dirtorch_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.dir_last_error
    limit = lib.dir_ivf_plan_max_pairs()

    def plan(probe=p, Q=3, nprobe=4, list_off=p, nlist=8, col_off=p, pair_off=p, pair_q=p, pair_col=p, item_off=p, counts=p):
        return lib.dir_ivf_plan(probe, Q, nprobe, list_off, nlist, col_off, pair_off, pair_q, pair_col, item_off, counts, None)

    for name in ('Q', 'nprobe', 'nlist'):
        assert plan(**{name: -1}) == -1 and err().startswith(b'ivf_plan:') and b'negative' in err(), name
    assert plan(nlist=65536) == -1 and b'65535' in err()
    assert plan(Q=limit + 1, nprobe=1) == -1 and b'dir_ivf_plan_max_pairs' in err()
    assert plan(Q=limit // 32 + 1, nprobe=32) == -1 and b'dir_ivf_plan_max_pairs' in err()
    assert plan(Q=1 << 20, nprobe=1 << 20) == -1 and b'dir_ivf_plan_max_pairs' in err()     # the product in 64 bits
    assert plan(nlist=0) == -1 and b'without a list' in err()
    for name in ('probe', 'list_off', 'col_off', 'pair_off', 'pair_q', 'pair_col', 'item_off', 'counts'):
        assert plan(**{name: None}) == -1 and b'null' in err(), name
    assert plan(Q=0) == 0 and plan(Q=0, probe=None, counts=None) == 0           # nothing to do: DIR_OK, nothing launched
    assert buf.raw == bytes(256)


def test_ops_argument_errors():
    """ops.ivf_plan's own checks come before the device is touched: host tensors, dtypes, shapes and the three limits."""
    import torch
    from dirtorch_amd import ops
    off, probe = torch.zeros(5, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match='device tensor'):
        ops.ivf_plan(off, probe, 1)


@pytest.mark.parametrize('seed', range(10))
def test_host_bound_of_the_grid_holds(seed):
    """item_off[nlist] <= the bound the scan is launched with <= rows * (the tiles of the nprobe longest lists), for tables
    as a search makes them: distinct lists per query, any lengths - also when every query probes the same lists (one group
    serves 32 of them) and when some slots are empty."""
    r = np.random.RandomState(500 + seed)
    Q, nlist = r.randint(1, 80), r.randint(1, 40)
    nprobe = r.randint(1, nlist + 1)
    probe, list_off = _random_table(r, Q, nprobe, nlist, empty=0.1 * (seed % 3))
    if seed % 4 == 3:
        probe[:] = probe[0]
    lens = np.diff(list_off)
    bound, plain = ivf_plan_ref.items_bound(lens, Q, nprobe), ivf_plan_ref.plain_bound(lens, Q, nprobe)
    items = int(ivf_plan_ref.plan(probe, list_off)['counts'][0])
    print('Q %d nprobe %d nlist %d: items %d, bound %d, plain bound %d' % (Q, nprobe, nlist, items, bound, plain))
    assert items <= bound <= plain
    # the bound index.py computes is this one
    from dirtorch_amd import index
    holder = index._InvertedLists()
    holder._lens = lens.astype(np.int64)
    assert holder._plan_items(Q, nprobe) == bound


def test_host_bound_is_reached():
    """One query at the nprobe longest lists, and 33 queries that all probe them (a second group of one pair on every
    tile): the bound is the count."""
    list_off = np.concatenate([[0], np.cumsum([10, 700, 256, 0, 257])]).astype(np.int32)
    probe = np.array([[1, 4, 2]], np.int32)
    assert ivf_plan_ref.items_bound(np.diff(list_off), 1, 3) == int(ivf_plan_ref.plan(probe, list_off)['counts'][0]) == 3 + 2 + 1
    probe = np.repeat(probe, 33, axis=0)
    assert ivf_plan_ref.items_bound(np.diff(list_off), 33, 3) == int(ivf_plan_ref.plan(probe, list_off)['counts'][0]) == 12
