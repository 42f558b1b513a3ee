"""alpha-QE / DBA from neighbour lists, the checks that need no GPU: the numpy restatement (tests/expand_ref.py) against the
reference's recorded outputs, the new symbol through header, ctypes table and ops, dir_expand_lists' argument errors
(they are raised before anything is launched) and the --expand flag of the two command lines."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from expand_ref import expand_lists_ref, lane_sums
from test_oracle_golden import QE_CASES, qe_inputs
from topk_ref import topk_ref_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exact_lists(q, db, k, same_set):
    """the stable-argsort lists of the fp32 scores (topk_ref restates np.argsort(row, kind='stable')[::-1][:k])"""
    scores = np.asarray(q, np.float32) @ np.asarray(db, np.float32).T
    return topk_ref_rows(scores, k, exclude=np.arange(len(q)) if same_set else None)


@pytest.mark.parametrize('k,alpha', QE_CASES)
def test_restatement_reproduces_the_reference_goldens(k, alpha, qe_goldens):
    """expand_lists_ref on exact lists against the reference's expand_descriptors outputs (tests/golden/qe_goldens.npz:
    five cases, the db form and the self-set) at the atol of tests/test_ranking_gpu.py.  Every self-set row of these
    inputs has k other rows scoring above 0, so the reference's zeroed diagonal is never picked (asserted)."""
    q, db = qe_inputs()
    idx, vals = exact_lists(q, db, k, False)
    np.testing.assert_allclose(expand_lists_ref(q, db, idx, vals, alpha), qe_goldens['qe.db.k%d.a%d' % (k, alpha)],
                               rtol=0, atol=2e-6)
    idx, vals = exact_lists(db, db, k, True)
    assert (idx != np.arange(len(db))[:, None]).all() and (vals > 0).all()
    np.testing.assert_allclose(expand_lists_ref(db, db, idx, vals, alpha), qe_goldens['qe.self.k%d.a%d' % (k, alpha)],
                               rtol=0, atol=2e-6)


def test_restatement_rules():
    """The parts of the definition the goldens do not reach: an empty slot adds nothing and its vals entry is not read,
    the mean divides by k + 1 whatever the number of empty slots, k = 0 normalises, a NaN weight stays in its row, and
    the lane a column belongs to."""
    r = np.random.RandomState(5)
    x, db = r.standard_normal((6, 12)).astype(np.float32), r.standard_normal((9, 12)).astype(np.float32)
    idx = np.array([[3, -1, 5]] * 6, np.int32)
    vals = np.array([[0.5, np.nan, 0.25]] * 6, np.float32)
    got = expand_lists_ref(x, db, idx, vals, 1)
    acc = (x + db[3] * np.float32(0.5) + db[5] * np.float32(0.25)) * (np.float32(1) / np.float32(4))
    np.testing.assert_allclose(got, acc / np.linalg.norm(acc, axis=1, keepdims=True), rtol=0, atol=1e-6)
    none = expand_lists_ref(x, db, np.zeros((6, 0), np.int32), np.zeros((6, 0), np.float32), 3)
    np.testing.assert_allclose(none, x / np.linalg.norm(x, axis=1, keepdims=True), rtol=0, atol=1e-6)
    vals[2, 0] = np.nan
    bad = expand_lists_ref(x, db, idx, vals, 1)
    assert np.isnan(bad[2]).all() and np.array_equal(np.delete(bad, 2, 0), np.delete(got, 2, 0))
    one = np.zeros((1, 2052), np.float32)
    one[0, [0, 3, 4, 1023, 1024, 1027, 2051]] = [1, 2, 3, 4, 5, 6, 7]
    p = lane_sums(one)[0]
    assert p[0] == 1 + 4 + 25 + 36 + 49 and p[1] == 9 and p[255] == 16 and p.sum() == 140


def test_header_ctypes_and_ops_agree_on_the_new_symbol():
    from dirtorch_amd import _lib, ops, ranking
    src = open(os.path.join(ROOT, 'include', 'dir_engine.h')).read()
    m = re.search(r'int dir_expand_lists\(([^)]*)\);', src)
    assert m, 'include/dir_engine.h does not declare dir_expand_lists'
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    assert [p.split()[-1].lstrip('*') for p in params] == ['descs', 'ldd', 'n', 'db', 'ldb', 'm', 'D', 'idx', 'vals', 'ldl',
                                                           'k', 'alpha', 'out', 'ldo', 'stream']
    want = [ctypes.c_void_p if '*' in p else {'int': ctypes.c_int, 'float': ctypes.c_float}[p.split()[0]] for p in params]
    res, args = _lib.SIGNATURES['dir_expand_lists']
    assert res is ctypes.c_int and args == want
    fn = _lib.load().dir_expand_lists
    assert fn.argtypes == want
    assert list(inspect.signature(ops.expand_lists).parameters) == ['descs', 'db', 'idx', 'vals', 'alpha']
    sig = inspect.signature(ranking.expand_device).parameters
    assert list(sig)[:6] == ['descs', 'db', 'alpha', 'k', 'index', 'scratch_bytes']
    assert sig['db'].default is None and sig['alpha'].default == 0 and sig['k'].default == 0 and sig['index'].default is None
    assert os.path.isfile(os.path.join(ROOT, 'deep-image-retrieval_amd', 'csrc', 'expand_lists.hip'))
    assert 'expand_lists' in open(os.path.join(ROOT, 'deep-image-retrieval_amd', 'csrc', 'build.sh')).read()


def test_expand_lists_argument_errors_need_no_gpu():
    """Every DIR_ERR_INVALID case of the header, with a non-null host address for the pointers: nothing is launched."""
    from dirtorch_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.dir_last_error

    def call(descs=p, ldd=8, n=3, db=p, ldb=8, m=5, D=8, idx=p, vals=p, ldl=4, k=4, alpha=1.0, out=p, ldo=8):
        return lib.dir_expand_lists(descs, ldd, n, db, ldb, m, D, idx, vals, ldl, k, alpha, out, ldo, None)

    assert call(D=0) == -1 and b'D < 1' in err()
    assert call(n=-1) == -1 and call(m=-1) == -1 and call(k=-1, ldl=0) == -1 and b'negative' in err()
    assert call(ldd=7) == -1 and call(ldb=7) == -1 and call(ldo=7) == -1 and b'ld' in err()
    assert call(ldl=3) == -1 and b'ldl' in err()
    assert call(alpha=-0.5) == -1 and b'alpha' in err()
    assert call(alpha=float('nan')) == -1 and b'alpha' in err()
    for name in ('descs', 'db', 'idx', 'vals', 'out'):
        assert call(**{name: None}) == -1 and b'null' in err(), name
    assert call(n=0) == 0 and call(n=0, descs=None, db=None, idx=None, vals=None, out=None) == 0


def test_expand_device_argument_errors_need_no_gpu():
    from dirtorch_amd import ranking
    x = np.zeros((4, 8), np.float32)
    assert ranking.expand_device(x, db=x, alpha=3, k=0) is x      # the reference's contract
    with pytest.raises(ValueError):
        ranking.expand_device(x, k=-1)
    with pytest.raises(ValueError):
        ranking.expand_device(x, k=2, alpha=-1)


@pytest.mark.parametrize('module', ['retrieve', 'eval_dir'])
def test_command_lines_reject_a_bad_expand_value_before_anything_is_loaded(module, capsys):
    """--expand takes matrix or lists; anything else ends in argparse's exit 2 - with a dataset and a checkpoint that do
    not exist, so nothing was opened on the way."""
    import importlib
    mod = importlib.import_module('dirtorch_amd.' + module)
    argv = ['--dataset', 'ImageList("/nonexistent/db.txt")', '--checkpoint', '/nonexistent/ck.pt', '--expand', 'rows']
    if module == 'retrieve':
        argv += ['--output', '/nonexistent/out.npz']
    with pytest.raises(SystemExit) as e:
        mod.main(argv)
    assert e.value.code == 2
    assert '--expand' in capsys.readouterr().err


def test_descriptors_rejects_a_bad_route_before_anything_is_loaded():
    from dirtorch_amd import eval_dir
    with pytest.raises(ValueError):
        eval_dir.descriptors(None, None, None, expand='rows')
    with pytest.raises(ValueError):
        eval_dir.descriptors(None, None, None, expand='matrix', expand_index=lambda rows: None)
    with pytest.raises(ValueError):
        eval_dir.eval_model(None, None, None, expand='rows')
