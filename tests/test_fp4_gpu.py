"""The fp4 descriptor index on the device (dir_quantize_rows_fp4, dir_similarity_fp4, index.Fp4Index, python -m
dirtorch_amd.retrieve --index fp4) against the numpy restatement of tests/fp4_ref.py.  Every partial sum of a score is a
multiple of 1/64 below 2^24 / 64, exact in fp32 in any order, so codes, block bytes, scales, scores and the lists of a
scan are compared bit for bit; test_accumulation_is_exact_up_to_the_bound carries the one supposition about the
hardware: the matrix core adds exactly representable fp32 sums exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fp4_ref
from index_util import cuda as _cuda, same as _same
from topk_ref import bits, topk_ref_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QB, ROWS = 96, 256      # csrc/index_fp4.hip: query rows per block, database rows per workgroup


def _bits_equal(got, want):
    """the same stored bits, a NaN matching any NaN (which NaN a multiply returns is not part of the definition)"""
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def _u8(a):
    return _cuda(a, np.uint8)


# ---- quantize_rows_fp4 -------------------------------------------------------------------------------------------------
def _quantize(x, pitch=0):
    """(codes, exps, scales) ndarrays of ops.quantize_rows_fp4; the output buffers are likely to reuse a block full of
    0x55, so a padding byte the kernel does not write shows."""
    from dirtorch_amd import ops
    N, D = x.shape
    dev = _cuda(x)
    if pitch:
        wide = torch.full((N, D + pitch), float('nan'), dtype=torch.float32, device='cuda')
        wide[:, :D] = dev
        dev = wide[:, :D]
    ldc, lde = fp4_ref.widths(D)
    junk = [torch.full((N, w), 0x55, dtype=torch.uint8, device='cuda') for w in (ldc, lde)]
    del junk
    codes, exps, scales = ops.quantize_rows_fp4(dev)
    assert codes.dtype == exps.dtype == torch.uint8 and scales.dtype == torch.float32
    assert tuple(codes.shape) == (N, ldc) and tuple(exps.shape) == (N, lde) and tuple(scales.shape) == (N,)
    return codes.cpu().numpy(), exps.cpu().numpy(), scales.cpu().numpy()


def _check_quantize(x, pitch=0, what=''):
    codes, exps, scales = _quantize(x, pitch)
    wc, we, ws = fp4_ref.quantize(x)
    assert (codes == wc).all(), (what, np.argwhere(codes != wc)[:5])
    assert (exps == we).all(), (what, np.argwhere(exps != we)[:5])
    assert (bits(scales) == bits(ws)).all(), (what, np.argwhere(bits(scales) != bits(ws))[:5])
    return codes, exps, scales


@pytest.mark.parametrize('D', [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2048, 2500])
def test_quantize_rows_matches_the_restatement(D):
    """One wave per row, four rows per workgroup, eight lanes per block of 32; 2048 values is what a wave keeps in
    registers (2500: the two-pass form); pitched inputs take the scalar loads."""
    r = np.random.RandomState(180 + D)
    for N in (1, 257):
        x = (r.standard_normal((N, D)) * np.exp(r.uniform(-12, 12, (N, 1)))).astype(np.float32)
        _check_quantize(x, what='%d x %d' % (N, D))
    x = (r.standard_normal((41, D)) * np.exp(r.uniform(-3, 3, (41, (D + 31) // 32)).repeat(32, axis=1)[:, :D])).astype(np.float32)
    _check_quantize(x, pitch=3, what='pitch D + 3, blocks of many levels')
    _check_quantize(x, pitch=4, what='pitch D + 4')


@pytest.mark.parametrize('D', [33, 257, 2048, 2500])
def test_quantize_rows_degenerate_tie_and_clamped_rows(D):
    r = np.random.RandomState(190)
    nb = (D + 31) // 32
    x = r.standard_normal((40, D)).astype(np.float32)
    x[0] = 0
    x[1] = np.float32(1e-40) * r.randint(-3, 4, D)                # subnormals
    x[2] = np.float32(2.0 ** -61) * r.choice([-1, 1], D)          # normal, below 2^-60
    x[3, D // 2] = np.nan
    x[4, D - 1] = np.inf
    x[5, 0] = -np.inf
    x[6] = -0.0
    x[7] = 0
    x[7, D - 1] = -3                                              # a single non-zero, in the last (partial) block
    x[8] = 0
    x[8, 0] = np.float32(2.0 ** -60)                              # the smallest row that is kept
    mid = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5, 4, 6, 7], np.float32)
    for row, E in ((9, 0), (10, -40), (11, 100)):                 # every value a tie (or on the grid), blocks of three levels
        level = E - r.randint(0, 3, nb).repeat(32)[:D]
        level[:32] = E
        x[row] = mid[r.randint(0, 10, D)] * r.choice([-1, 1], D) * np.float32(2.0) ** level.astype(np.float32)
        x[row, 0] = 4 * np.float32(2.0) ** np.float32(E)
    for row in range(12, 20):                                     # blocks falling away binade by binade: the clamp
        fall = -(np.arange(nb) % (row - 8)).repeat(32)[:D]
        x[row] = r.uniform(-1, 1, D) * np.float32(2.0) ** fall.astype(np.float32)
    codes, exps, scales = _check_quantize(x, what='D = %d' % D)
    assert not codes[:7].any() and (exps[:7] == 127).all()
    assert (bits(scales[[0, 1, 2, 6]]) == 0).all() and np.isnan(scales[3:6]).all()
    assert np.count_nonzero(codes[7]) == 1 and np.count_nonzero(codes[8]) == 1
    assert (exps[12:20, :nb] == 125).any() or nb < 3


# ---- similarity_fp4 ----------------------------------------------------------------------------------------------------
def _coded(r, n, D, junk=False):
    """random stored rows (codes [n, ldc], exps [n, lde]): every nibble, -0 included, and the three block levels; junk: the
    codes past D hold noise, the block bytes past D anything but 255 and those past D rounded up to 64 anything"""
    ldc, lde = fp4_ref.widths(D)
    nib = np.zeros((n, 2 * ldc), np.uint8)
    if junk:
        nib[:] = r.randint(0, 16, nib.shape)
    nib[:, :D] = r.randint(0, 16, (n, D))
    exps = np.full((n, lde), 127, np.uint8)
    if junk:
        exps[:] = r.randint(0, 255, exps.shape)
        exps[:, (D + 63) // 64 * 2:] = 255
    exps[:, :(D + 31) // 32] = r.randint(125, 128, (n, (D + 31) // 32))
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8), exps


def _clean(codes, exps, D):
    """the stored rows as the definition reads them: nothing past D"""
    codes, exps = codes.copy(), exps.copy()
    codes[:, (D + 1) // 2:] = 0
    if D % 2:
        codes[:, D // 2] &= 0x0f
    exps[:, (D + 31) // 32:] = 127
    return codes, exps


@pytest.mark.parametrize('D', [33, 257, 320])
def test_scan_layout_one_hot_pairs(D):
    """Query row i holds one non-zero, at k_q(i); database row j one, at k_b(j) = k_q(j mod Q): a cell is non-zero iff
    the two k agree, and then it is the product of the two stored values - code and block level are functions of (row,
    k), different ones on the two sides.  The shifts walk every row through every block, so every block of a slab, both
    lane halves, the partial last slab (D = 320: two chunks of eight; 33, 257: one real block and a padding one), the
    three accumulator blocks, the four row groups and all eight consumer waves see a non-zero at every nibble position.
    A wrong lane, nibble or scale-byte map moves or rescales a cell."""
    from dirtorch_amd import ops
    ldc, lde = fp4_ref.widths(D)
    nb = (D + 31) // 32
    one = torch.ones(257, dtype=torch.float32, device='cuda')

    def rows(n, k, code, sign, level, other):
        nib = np.zeros((n, 2 * ldc), np.uint8)
        nib[np.arange(n), k] = code | (sign << 3)
        exps = np.full((n, lde), 127, np.uint8)
        exps[:, :nb] = other
        exps[np.arange(n), k // 32] = level
        value = fp4_ref.GRID[code].astype(np.float64) * np.where(sign, -1, 1) * 2.0 ** (level.astype(np.float64) - 127)
        return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8), exps, value

    seen = set()
    for Q in (1, 97):
        for N in (1, 257):
            i, j = np.arange(Q), np.arange(N)
            for shift in range(0, nb * 32, 32):
                kq = (3 * i + shift) % D
                kb = (3 * (j % Q) + shift) % D
                cq, eq, vq = rows(Q, kq, 1 + (i + kq) % 7, (i * kq + i) & 1, 125 + (i + 2 * kq) % 3,
                                  (125 + (i[:, None] + np.arange(nb)[None, :]) % 3))
                cb, eb, vb = rows(N, kb, 1 + (3 * j + 2 * kb) % 7, (j + kb) & 1, 125 + (2 * j + kb // 32) % 3,
                                  (125 + (2 * j[:, None] + np.arange(nb)[None, :] + 1) % 3))
                got = ops.similarity_fp4(_u8(cq), _u8(eq), one[:Q], _u8(cb), _u8(eb), one[:N], D).cpu().numpy()
                hit = kq[:, None] == kb[None, :]
                want = np.where(hit, vq[:, None] * vb[None, :], 0).astype(np.float32)
                assert ((got != 0) == hit).all(), (Q, N, shift, np.argwhere((got != 0) != hit)[:5])
                assert (bits(got) == bits(want)).all(), (Q, N, shift, np.argwhere(bits(got) != bits(want))[:5])
                assert (bits(got) == bits(fp4_ref.score(cq, eq, np.ones(Q), cb, eb, np.ones(N), D))).all()
                if Q == 97 and N == 257:
                    qi, bj = np.nonzero(hit)
                    seen |= set(zip((kq[qi] // 32).tolist(), (qi // 32).tolist(), (qi % 32 // 8).tolist(), (bj // 32).tolist()))
    # (block of the row, accumulator block, row group, consumer wave): every block with every accumulator block and row
    # group, every wave (and the row of the second tile).  A last block of one value (D = 33, 257) is met by few rows: it
    # is seen with every accumulator block
    full = range(nb if D % 32 == 0 else nb - 1)
    assert {(b, a, g) for b, a, g, w in seen} >= {(b, a, g) for b in full for a in range(4) for g in range(4) if a < 3 or g == 0}
    assert {(b, a) for b, a, g, w in seen} >= {(nb - 1, a) for a in range(3)}
    assert {w for b, a, g, w in seen} == set(range(9))


@pytest.mark.parametrize('D', [1, 64, 65, 129, 255, 256, 257, 448, 2048])
def test_similarity_fp4_is_the_restatement(D):
    """One launch form: grid = (database tiles of 256 rows, query blocks of 96 rows), K slabs of 256 over D rounded up to
    64.  Q = 1 / 96 | 97 / 200: a partial block, a full one, one block plus a row, three blocks; N on both sides of a
    tile and three tiles; D = 64, 65 .. 129: the last slab is a quarter or a half, 255, 256: one whole slab, 257: a slab
    and a quarter, 448: two slabs, the last three quarters, 2048: eight slabs (the three-stage ring goes round).  The
    database rows carry noise past D in their codes and block bytes (it must not count), and a NaN and a zero scale."""
    from dirtorch_amd import ops
    r = np.random.RandomState(200 + D)
    cq, eq = _coded(r, 200, D)
    cb, eb = _coded(r, 600, D, junk=True)
    sq = np.exp2(r.randint(-20, 5, 200)).astype(np.float32)
    sb = np.exp2(r.randint(-20, 5, 600)).astype(np.float32)
    sb[5], sb[7], sq[3] = np.nan, 0, 0
    want = fp4_ref.score(cq, eq, sq, *_clean(cb, eb, D), sb, D)
    dq, de, ds, db, dbe, dbs = _u8(cq), _u8(eq), _cuda(sq), _u8(cb), _u8(eb), _cuda(sb)
    for Q in (1, QB, QB + 1, 200):
        for N in (1, ROWS - 1, ROWS, ROWS + 1, 600):
            got = ops.similarity_fp4(dq[:Q], de[:Q], ds[:Q], db[:N], dbe[:N], dbs[:N], D)
            assert got.dtype == torch.float32 and tuple(got.shape) == (Q, N)
            g = got.cpu().numpy()
            assert _bits_equal(g, want[:Q, :N]).all(), (Q, N, np.argwhere(~_bits_equal(g, want[:Q, :N]))[:5])
    # a score pitch lds > N: the columns past N stay as they were; database rows from a row offset
    out = torch.full((97, 300), -7.0, dtype=torch.float32, device='cuda')
    got = ops.similarity_fp4(dq[:97], de[:97], ds[:97], db[3:260], dbe[3:260], dbs[3:260], D, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (97, 257)
    assert _bits_equal(got.cpu().numpy(), want[:97, 3:260]).all() and (out[:, 257:] == -7).all()
    # rows at a pitch wider than their width, noise in between
    ldc, lde = fp4_ref.widths(D)
    wc = torch.full((600, ldc + 48), 0xff, dtype=torch.uint8, device='cuda')
    we = torch.full((600, lde + 16), 0xff, dtype=torch.uint8, device='cuda')
    wc[:, :ldc], we[:, :lde] = db, dbe
    got = ops.similarity_fp4(dq, de, ds, wc[:, :ldc], we[:, :lde], dbs, D)
    assert _bits_equal(got.cpu().numpy(), want).all()


def test_accumulation_is_exact_up_to_the_bound():
    """D = 7281, the widest row.  Every code +-6 at the top level: the score is the integer bound 36 * 7281 itself, whose
    partial sums run through every multiple of 36 up to 2^24 / 64 - exact only if the matrix core adds exactly
    representable fp32 sums exactly, in whatever order it takes the 64 products of a step and the slabs of a row (every
    tile starts at another slab).  Alternating signs cancel to 0 or to the odd one out; rows of all three block levels and
    all codes are compared with the restatement's integer sums."""
    from dirtorch_amd import ops
    D = fp4_ref.MAX_DIM
    ldc, lde = fp4_ref.widths(D)
    r = np.random.RandomState(210)
    Q, N = 5, 600
    nq, nbn = np.full((Q, 2 * ldc), 7, np.uint8), np.full((N, 2 * ldc), 7, np.uint8)
    nq[:, D:], nbn[:, D:] = 0, 0
    eq, eb = np.full((Q, lde), 127, np.uint8), np.full((N, lde), 127, np.uint8)
    nq[1, 1:D:2] = 15                                             # query 1: + - + - ...
    nbn[1, 0:D:2] = 15                                            # row 1: - + - + ...
    nbn[2, :D] = 7 | (r.randint(0, 2, D) << 3).astype(np.uint8)   # row 2: random signs
    nq[2:, :D] = r.randint(0, 16, (Q - 2, D))                     # queries 2 ..: every code, every level
    eq[2:, :(D + 31) // 32] = r.randint(125, 128, (Q - 2, (D + 31) // 32))
    nbn[3:300, :D] = r.randint(0, 16, (297, D))
    eb[3:300, :(D + 31) // 32] = r.randint(125, 128, (297, (D + 31) // 32))
    for n in range(300, N):                                       # +-6 at the top level, a growing share flipped
        nbn[n, r.choice(D, (n - 300) * D // 600, replace=False)] = 15
    cq, cb = (nq[:, 0::2] | (nq[:, 1::2] << 4)).astype(np.uint8), (nbn[:, 0::2] | (nbn[:, 1::2] << 4)).astype(np.uint8)
    acc = fp4_ref.acc(cq, eq, cb, eb, D)
    assert acc[0, 0] == 36 * D == 262116 and acc[0, 0] * 64 == 2 ** 24 - 1792
    assert acc[0, 1] == -36 and acc[1, 0] == 36 and acc[1, 1] == -36 * D and acc[1, 300] == 36
    assert (np.abs(acc) * 64 > 2 ** 23).sum() > 100               # sums that need all 24 bits
    one = np.ones(max(Q, N), np.float32)
    got = ops.similarity_fp4(_u8(cq), _u8(eq), _cuda(one[:Q]), _u8(cb), _u8(eb), _cuda(one[:N]), D).cpu().numpy()
    assert (bits(got) == bits(acc)).all(), np.argwhere(bits(got) != bits(acc))[:5]
    sq, sb = np.exp2(r.randint(-30, 30, Q)).astype(np.float32), np.exp2(r.randint(-30, 30, N)).astype(np.float32)
    got = ops.similarity_fp4(_u8(cq), _u8(eq), _cuda(sq), _u8(cb), _u8(eb), _cuda(sb), D).cpu().numpy()
    assert (bits(got) == bits(fp4_ref.score(cq, eq, sq, cb, eb, sb, D))).all()


# ---- Fp4Index ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sets():
    """The inputs tests/test_fp4_cpu.py checks the re-rank condition on, their quantised and exact scores."""
    q, b = fp4_ref.rerank_sets()
    quant = fp4_ref.score(*fp4_ref.quantize(q), *fp4_ref.quantize(b), 200)
    exact64 = q.astype(np.float64) @ b.astype(np.float64).T
    mass = np.abs(q.astype(np.float64)) @ np.abs(b.astype(np.float64)).T            # sum_k |q_k b_k|
    return dict(q=q, b=b, quant=quant, exact64=exact64, exact=exact64.astype(np.float32), mass=mass)


def _index(b):
    from dirtorch_amd.index import Fp4Index
    return Fp4Index(b.shape[1]).add(b)


def test_search_is_the_restatement_however_the_work_is_cut(sets):
    """The lists are fp4_ref.search's, value bits included, whether the database is scanned whole, in db_rows chunks or
    with a small scratch, and whether it was added in one call or in three."""
    from dirtorch_amd.index import Fp4Index
    q, b = sets['q'], sets['b']
    one = _index(b)
    three = Fp4Index(200)
    three.add(b[:1000])                                           # an ndarray,
    three.add(torch.from_numpy(b[1000:1001]))                     # a CPU tensor,
    three.add(torch.from_numpy(b[1001:]).cuda())                  # a CUDA tensor
    assert len(one) == len(three) == 3000
    assert torch.equal(one.codes, three.codes) and torch.equal(one.exps, three.exps) and torch.equal(one.scales, three.scales)
    wc, we, ws = fp4_ref.quantize(b)
    assert (one.codes.cpu().numpy() == wc).all() and (one.exps.cpu().numpy() == we).all()
    assert (bits(one.scales.cpu().numpy()) == bits(ws)).all()
    assert one.nbytes() == 3000 * (128 + 8 + 4)
    for k in (10, 100):
        want = fp4_ref.search(q, b, k)
        _same(want, topk_ref_rows(sets['quant'], k))
        for index in (one, three):
            for kw in ({}, dict(scratch_bytes=4 * 3000 * 10), dict(db_rows=701), dict(db_rows=701, scratch_bytes=4 * 701 * 10)):
                idx, vals = index.search(q, k, **kw)
                assert idx.dtype == torch.int32 and vals.dtype == torch.float32 and idx.is_cuda and vals.is_cuda
                _same((idx, vals), want, '%r, k = %d' % (kw, k))


def test_search_same_set_and_short_rows(sets):
    b = sets['b'][:600]
    index = _index(b)
    own = np.arange(600, dtype=np.int32)
    for k, kw in ((20, {}), (20, dict(db_rows=177, scratch_bytes=4 * 177 * 250)), (600, {})):
        idx, vals = index.search(b, k, same_set=True, **kw)
        _same((idx, vals), fp4_ref.search(b, b, k, exclude=own), 'k = %d' % k)
        assert (idx.cpu().numpy() != own[:, None]).all()
    assert (idx[:, -1] == -1).all() and torch.isnan(vals[:, -1]).all()        # k = N: a row has N - 1 neighbours
    idx, vals = index.search(b, 600, rerank=600, source=_cuda(b), same_set=True)
    assert (idx[:, -1] == -1).all() and torch.isnan(vals[:, -1]).all() and (idx[:, :-1] >= 0).all()


def test_search_rerank_gives_retrieve_devices_lists(sets):
    """(k, R) = (10, 40) and (100, 400).  The precondition - the restatement's shortlist of R holds the exact top k of
    every query (tests/test_fp4_cpu.py) - is asserted first; then the index's lists are retrieve_device's, and the values
    are within gather_scores' bound of the fp64 scores."""
    from dirtorch_amd import ranking
    q, b = sets['q'], sets['b']
    index = _index(b)
    rows = np.arange(33)[:, None]
    for k, R in ((10, 40), (100, 400)):
        want = topk_ref_rows(sets['exact'], k)[0]
        short = topk_ref_rows(sets['quant'], R)[0]
        assert all(set(want[i]) <= set(short[i]) for i in range(33))
        idx, vals = index.search(q, k, rerank=R, source=_cuda(b))
        got = idx.cpu().numpy()
        assert (got == want).all()
        assert (got == ranking.retrieve_device(q, b, k)[0].cpu().numpy()).all()
        err = np.abs(vals.cpu().numpy().astype(np.float64) - sets['exact64'][rows, got])
        assert (err <= 202 * 2.0 ** -24 * sets['mass'][rows, got]).all()
        idx2, vals2 = index.search(q, k, rerank=R, source=b, db_rows=701)
        assert torch.equal(idx2, idx) and torch.equal(vals2.view(torch.int32), vals.view(torch.int32))


def test_save_load_round_trip_and_argument_errors(sets, tmp_path):
    from dirtorch_amd import ops
    from dirtorch_amd.index import Fp4Index
    q, b = sets['q'], sets['b']
    index = _index(b)
    path = str(tmp_path / 'index.npz')
    index.save(path)
    with np.load(path) as f:
        assert sorted(f.files) == ['D', 'codes', 'exps', 'scales']
        assert f['codes'].shape == (3000, 100) and f['codes'].dtype == np.uint8 and f['exps'].shape == (3000, 7)
    back = Fp4Index.load(path)
    assert back.D == 200 and len(back) == 3000 and back.nbytes() == index.nbytes()
    assert torch.equal(back.codes, index.codes) and torch.equal(back.exps, index.exps)
    assert torch.equal(back.scales.view(torch.int32), index.scales.view(torch.int32))
    for kw in (dict(), dict(rerank=40, source=_cuda(b))):
        a, c = index.search(q, 10, **kw), back.search(q, 10, **kw)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1].view(torch.int32), c[1].view(torch.int32))
    with pytest.raises(ValueError):
        Fp4Index(ops.index_fp4_max_dim() + 1)
    with pytest.raises(ValueError):
        Fp4Index(0)
    with pytest.raises(ValueError):
        index.search(q, 10, rerank=40)                           # no source
    with pytest.raises(ValueError):
        index.search(q, 10, rerank=9, source=b)                  # R < k
    with pytest.raises(ValueError):
        index.search(q, 3001)
    with pytest.raises(ValueError):
        index.search(q, 10, same_set=True)
    with pytest.raises(ValueError):
        index.add(np.zeros((3, 199), np.float32))
    with pytest.raises(ValueError):
        ops.quantize_rows_fp4(torch.zeros(2, ops.index_fp4_max_dim() + 1, device='cuda'))
    c, e, s = ops.quantize_rows_fp4(_cuda(q))
    with pytest.raises(ValueError):
        ops.similarity_fp4(c, e, s, index.codes, index.exps, index.scales, 257)     # codes too narrow for that D
    with pytest.raises(TypeError):
        ops.similarity_fp4(c.to(torch.int8), e, s, index.codes, index.exps, index.scales, 200)


# ---- python -m dirtorch_amd.retrieve --index fp4, ranking.expand_device(index=Fp4Index) --------------------------------
def test_retrieve_cli_with_an_fp4_index(tmp_path):
    """The CLI in fresh processes on the synthetic descriptors of test_retrieve_cli_with_an_int8_index (--load-feats):
    with --index fp4 [--rerank 28] the .npz holds what Fp4Index.search gives for the same descriptors."""
    import dir_oracle as O
    r = np.random.RandomState(69)
    N, D, k = 120, 32, 7
    x = np.round(r.standard_normal((N, D)) * 4).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    np.save(str(tmp_path / 'feats.bdescs.npy'), x)
    (tmp_path / 'db.txt').write_text(''.join('img%d.jpg c%d\n' % (i, i % 9) for i in range(N)))
    sd = O.synth_state_dict('resnet18', seed=7, gemp=3.0, out_dim=D)
    torch.save({'model_options': dict(arch='resnet18_rmac', out_dim=D, pooling='gem', gemp=3),
                'state_dict': {'module.' + key: v for key, v in sd.items()}}, str(tmp_path / 'ck.pt'))
    pkg = os.path.join(ROOT, 'deep-image-retrieval_amd')
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get('PYTHONPATH', ''))
    runs = {'rerank': ['--index', 'fp4', '--rerank', '28'], 'raw': ['--index', 'fp4']}
    outs = {name: str(tmp_path / (name + '.npz')) for name in runs}
    procs = [subprocess.Popen([sys.executable, '-m', 'dirtorch_amd.retrieve', '--dataset',
                               'ImageListLabels("%s", root="%s")' % (tmp_path / 'db.txt', tmp_path), '--checkpoint',
                               str(tmp_path / 'ck.pt'), '--whiten', '', '--load-feats', str(tmp_path), '--gpu', '0',
                               '--topk', str(k), '--output', outs[name]] + flags, env=env) for name, flags in runs.items()]
    assert [p.wait(timeout=300) for p in procs] == [0, 0]
    index = _index(x)
    for name, kw in (('rerank', dict(rerank=28, source=x)), ('raw', {})):
        npz = np.load(outs[name])
        assert sorted(npz.files) == ['idx', 'scores'] and npz['idx'].dtype == np.int32 and npz['scores'].dtype == np.float32
        _same((npz['idx'], npz['scores']), tuple(t.cpu().numpy() for t in index.search(x, k, same_set=True, **kw)), name)
        assert (npz['idx'] != np.arange(N)[:, None]).all()
    npz = np.load(outs['raw'])
    _same((npz['idx'], npz['scores']), fp4_ref.search(x, x, k, exclude=np.arange(N)), 'raw lists')


def test_expand_device_takes_an_fp4_index(sets):
    """ranking.expand_device(index=Fp4Index) needs no change: its lists are the index's own."""
    from dirtorch_amd import ops, ranking
    b = sets['b'][:600]
    index = _index(b)
    for kw in ({}, dict(rerank=32)):
        got = ranking.expand_device(b, alpha=2, k=8, index=index, **kw)
        idx, vals = index.search(b, 8, same_set=True, **(dict(kw, source=_cuda(b)) if kw else {}))
        want = ops.expand_lists(_cuda(b), _cuda(b), idx, vals, 2.0)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    q = sets['q']
    got = ranking.expand_device(q, db=b, alpha=1, k=5, index=index)
    want = ops.expand_lists(_cuda(q), _cuda(b), *index.search(q, 5), 1.0)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
