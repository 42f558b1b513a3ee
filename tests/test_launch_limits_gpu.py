"""Launches at the extent limit on the device: dir_gather_scores across its cut into several launches, at the largest single
launch, and Int8Index.search(rerank=R) end to end at the smallest Q * R that needs two launches.

The shapes are set by the limit, not by the workload: P = dir_launch_max_threads() / 256 * 4 pairs (one wave a pair, four
a workgroup; 67 108 860) is what one launch takes, so every case has about 2^26 pairs and buffers of 0.27 GB; D and N are
as small as the two load paths allow.  Operands are integers in [-3, 3]: every dot product is exact (|sum| <= 36) and
the comparison is bit for bit against an int64 reference.

No case runs a `refuse` row of tests/launch_limits.py at its largest admissible size: that takes buffers of several GB to
show what the small shapes of the other suites already cover; the refusals themselves are in test_launch_limits_cpu.py.

The tests bite (each mutant built once, run once; 1 and 2 on the device - they write too few or the wrong pairs, nothing out
of bounds - 3 without one):
  mutant                                                   fails
  1  every launch of the cut starts at pair 0 (item0       test_gather_scores_across_the_cut, all four cases: "pair 67108860
     dropped)                                              (P +0, row 1048575 column 60): -12345.0, exactly -2 expected";
                                                           test_int8_search_rerank_past_the_limit: row 32768 differs.  The two
                                                           single-launch cases pass, as they must.
  2  the cut without its last launch                       the same five tests with the same messages; the two single-launch
                                                           cases pass
  3  l2norm_rows without its guard (no GPU)                test_launch_limits_cpu.py::test_refusal_needs_no_gpu[pointwise-
                                                           l2norm_rows_kernel-x]: -5, "no ROCm-capable device is detected"
The library of the commit before the cut (one launch of ceil(Q * R / 4) workgroups) fails the first case too: no error, 192
of 67 109 056 pairs written (profiles/launch_limits.txt)."""
import numpy as np
import pytest
import torch

import index_ref
from index_util import cuda as _cuda, same as _same
from topk_ref import bits, topk_ref_rows

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.0)
N_ROWS = 5


def pairs_per_launch():
    from dirtorch_amd import _lib
    return int(_lib.load().dir_launch_max_threads()) // 256 * 4


def gather_case(Q, R, D, seed=0):
    """dir_gather_scores on Q x R pairs with a score pitch of R + 2 -> (scores [Q, R + 2] on the device, cand, the int64
    reference [Q, R] on the device: the exact dot product, 0 where cand is -1)."""
    from dirtorch_amd.ops import call, ptr, stream_ptr
    r = np.random.RandomState(1000 * D + R + seed)
    q = r.randint(-3, 4, (Q, D))
    b = r.randint(-3, 4, (N_ROWS, D))
    gen = torch.Generator(device='cuda').manual_seed(R + D + seed)
    cand = torch.randint(0, N_ROWS, (Q, R), dtype=torch.int32, device='cuda', generator=gen)
    cand[torch.rand(Q, R, device='cuda', generator=gen) < 0.1] = -1          # about one in ten
    scores = torch.full((Q, R + 2), float(SENTINEL), dtype=torch.float32, device='cuda')
    qd, bd = _cuda(q), _cuda(b)
    call('dir_gather_scores', ptr(qd), D, Q, ptr(bd), D, N_ROWS, D, ptr(cand), R, R, ptr(scores), R + 2, stream_ptr())
    torch.cuda.synchronize()
    table = torch.from_numpy(q.astype(np.int64) @ b.astype(np.int64).T).cuda()             # [Q, 5], exact
    want = torch.gather(table, 1, cand.clamp(min=0).long())
    return scores, cand, want


def check_gather(scores, cand, want, P):
    Q, R = cand.shape
    got = scores[:, :R]
    empty = cand < 0
    # by name first: the four pairs on each side of pair P (the first of a second launch) and the last pair
    for item in sorted({i for i in list(range(P - 4, P + 4)) + [Q * R - 1] if 0 <= i < Q * R}):
        qi, ri = divmod(item, R)
        g, c, w = float(got[qi, ri]), int(cand[qi, ri]), int(want[qi, ri])
        if c < 0:
            assert np.isnan(g), 'pair %d (P %+d, row %d column %d): %r where the candidate is -1' % (item, item - P, qi, ri, g)
        else:
            assert g == w, 'pair %d (P %+d, row %d column %d): %r, exactly %d expected' % (item, item - P, qi, ri, g, w)
    # every element, zero tolerance: NaN exactly at -1, the stored bits of the exact sum elsewhere, the pitch untouched
    assert torch.equal(torch.isnan(got), empty)
    want_bits = torch.where(empty, got.view(torch.int32), want.to(torch.float32).view(torch.int32))
    wrong = got.view(torch.int32) != want_bits
    assert not bool(wrong.any()), 'first wrong pairs (row, column): %s' % wrong.nonzero()[:5].tolist()
    pad = scores[:, R:]
    assert bool((pad == float(SENTINEL)).all()), 'the pitch columns were written'


@pytest.mark.parametrize('R,D', [(64, 3), (64, 4), (37, 3), (37, 4)])
def test_gather_scores_across_the_cut(R, D):
    """Q * R >= P + 192 pairs, the first such Q: two launches, the second of a few hundred pairs.  P is a multiple of neither
    R, so a query's candidates straddle the cut in the middle of a row (column 60 of 64, 36 of 37).  D = 3: the scalar loads;
    D = 4: the 16-byte ones."""
    P = pairs_per_launch()
    Q = -(-(P + 192) // R)
    assert P % R != 0 and P + 192 <= Q * R < P + 192 + R
    check_gather(*gather_case(Q, R, D), P)


@pytest.mark.parametrize('D', [3, 4])
def test_gather_scores_at_the_largest_single_launch(D):
    """Exactly P pairs (P = 60 * 1 118 481): one launch of the largest admissible size."""
    P = pairs_per_launch()
    R = 60
    assert P % R == 0
    check_gather(*gather_case(P // R, R, D), P)


def test_int8_search_rerank_past_the_limit():
    """Int8Index.search(rerank = R) where the re-score takes two launches, at the smallest shape that reaches it: R = N =
    dir_topk_max_k() = 2048 and Q = P // R + 16 = 32 783 rows (the last eight rows apart from the eight past the cut).  Integer descriptors, so the re-scored values are exact: lists
    and value bits equal the reference (index_ref, topk_ref_rows), as in test_index_gpu.py's
    test_search_rerank_exact_on_small_integers - checked on the first and last eight rows and the eight on each side of
    row P // R, whose candidates the cut divides (rows are independent)."""
    from dirtorch_amd import ops
    from dirtorch_amd.index import Int8Index
    P = pairs_per_launch()
    N = R = ops.topk_max_k()
    D, k = 8, 10
    cut = P // R
    Q = cut + 16
    assert cut * R < P < (cut + 1) * R and (Q - 16) * R < P
    r = np.random.RandomState(141)
    x = r.randint(-3, 4, (N, D)).astype(np.float32)
    q = r.randint(-3, 4, (Q, D)).astype(np.float32)
    index = Int8Index(D).add(x)
    idx, vals = index.search(_cuda(q), k, rerank=R, source=_cuda(x))
    assert tuple(idx.shape) == (Q, k) and tuple(vals.shape) == (Q, k)
    rows = np.r_[0:8, cut - 8:cut + 8, Q - 8:Q]
    quant = index_ref.score(*index_ref.quantize(q[rows]), *index_ref.quantize(x))
    exact = (q[rows].astype(np.float64) @ x.astype(np.float64).T).astype(np.float32)
    cand = topk_ref_rows(quant, R)[0]
    want = topk_ref_rows(np.take_along_axis(exact, cand.astype(np.int64), axis=1), k, ids=cand)
    sel = torch.from_numpy(rows).cuda()
    _same((idx[sel], vals[sel]), want, 'rows %s' % rows.tolist())
    assert not bool(torch.isnan(vals).any()) and bool((idx >= 0).all())
    assert (bits(vals[cut].cpu().numpy()) == bits(want[1][8 + 8])).all()        # (row P // R by name)
