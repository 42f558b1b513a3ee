"""What the three flat code scans have alike (the frame of a scan workgroup and the scaled store of csrc/flat_scan.h; the
two-pass row walk that each quantiser kernel keeps for itself), met directly at the smallest shapes at which it can go
wrong, once per format.  The expected values are those of tests/index_ref.py, fp4_ref.py and bin_ref.py, compared bit for
bit (a NaN matching any NaN)."""
import numpy as np
import pytest
import torch

import bin_ref
import fp4_ref
import index_ref
from index_util import cuda as _cuda
from topk_ref import bits

pytestmark = pytest.mark.gpu

FORMATS = ('i8', 'fp4', 'bin')
SENTINEL = -7.0


def _bits_equal(got, want):
    """the same stored bits, a NaN matching any NaN (which NaN a multiply returns is not part of the definition)"""
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def _i8_codes(r, n, D):
    """int8 codes [n, D rounded up to 64] over -127 .. 127 in every column (at D = 64 and 320 a row has no padding of its own:
    the int8 database's noise is the columns _embedded puts behind every row; as query codes of the bit scan, where ldq > D is
    allowed, the columns past D are noise)"""
    return r.randint(-127, 128, (n, index_ref.pad64(D))).astype(np.int8)


def _fp4_rows(r, n, D, junk):
    """stored fp4 rows (codes [n, ldc], block bytes [n, lde]): every nibble and the three block levels; junk: noise past D
    (a block byte between D and D rounded up to 64 anything but 255, as tests/test_fp4_gpu.py has it)"""
    ldc, lde = fp4_ref.widths(D)
    nb = (D + 31) // 32
    nib = r.randint(0, 16, (n, 2 * ldc)).astype(np.uint8)
    exps = r.randint(0, 255, (n, lde)).astype(np.uint8)
    exps[:, (D + 63) // 64 * 2:] = 255
    if not junk:
        nib[:, D:] = 0
        exps[:] = 127
    exps[:, :nb] = r.randint(125, 128, (n, nb))
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8), exps


def _fp4_clean(codes, exps, D):
    """the stored rows as the definition reads them: nothing past D"""
    codes, exps = codes.copy(), exps.copy()
    codes[:, (D + 1) // 2:] = 0
    if D % 2:
        codes[:, D // 2] &= 0x0f
    exps[:, (D + 31) // 32:] = 127
    return codes, exps


def _sides(fmt, r, Q, N, D):
    """(query tensors, database tensors, the scores [Q, N] the definition gives) without the scales, as numpy arrays: the
    query side as its quantiser leaves it, the database side with noise wherever the definition does not look"""
    if fmt == 'i8':
        cq, cb = _i8_codes(r, Q, D), _i8_codes(r, N, D)
        cq[:, D:] = 0
        return (cq,), (cb,), lambda sq, sb: index_ref.score(cq[:, :D], sq, cb[:, :D], sb)
    if fmt == 'fp4':
        q, b = _fp4_rows(r, Q, D, junk=False), _fp4_rows(r, N, D, junk=True)
        return q, b, lambda sq, sb: fp4_ref.score(*q, sq, *_fp4_clean(*b, D), sb, D)
    cq = _i8_codes(r, Q, D)                                        # (the image is zero past D: the noise must not count)
    rows = r.randint(0, 256, (N, bin_ref.width(D))).astype(np.uint8)
    return (cq,), (rows,), lambda sq, sb: bin_ref.score(cq, sq, rows, sb, D)


def _similarity(fmt):
    from dirtorch_amd import ops
    return {'i8': ops.similarity_i8, 'fp4': ops.similarity_fp4, 'bin': ops.similarity_bin}[fmt]


def _embedded(r, a, extra):
    """the rows of `a` as a slice of a larger noisy array on the device: from row 3 on, `extra` columns of noise behind
    every row (a multiple of the alignment the scan asks of the operand, so the slice stays admissible as it lies)"""
    big = r.randint(0, 256, (a.shape[0] + 6, a.shape[1] + extra)).astype(np.uint8).view(a.dtype)
    big[3:3 + a.shape[0], :a.shape[1]] = a
    return _cuda(big, a.dtype)[3:3 + a.shape[0], :a.shape[1]]


@pytest.mark.parametrize('fmt', FORMATS)
def test_frame_and_scaled_store(fmt):
    """D = 64: one slab (a quarter slab of fp4 codes, one chunk of bits); D = 320: three int8 slabs with the last half cut, two
    fp4 slabs with two of eight chunks in the last, one bit slab of three chunks.  N = 1, 33, 255, 257, 289: one row, a wave
    and a row, a tile less a row, a tile and a row, and a second tile with wave 0 full and one row in wave 1 - the descriptor
    extent (rows - 1) * ldp + Kb and the n < NP guard at each.  Q = 1, 97, 193: a row, a block and a row, two blocks and a
    row.  The database is a slice of a larger array with noise behind every row; one NaN and one zero row scale, one zero
    query scale; the scores go to an out= of row pitch N + 9 whose nine columns past N must keep what they held."""
    similarity = _similarity(fmt)
    Qmax, Nmax = 193, 289
    for D in (64, 320):
        r = np.random.RandomState(700 + D)
        qside, bside, score = _sides(fmt, r, Qmax, Nmax, D)
        sq = np.exp(r.uniform(-8, 2, Qmax)).astype(np.float32)
        sb = np.exp(r.uniform(-8, 2, Nmax)).astype(np.float32)
        sq[40], sb[1], sb[2] = 0, np.nan, 0
        want = score(sq, sb)
        assert want.shape == (Qmax, Nmax) and np.isnan(want[:, 1]).all() and not want[:, 2].any() and not want[40, 2:].any()
        dq = [_cuda(a, a.dtype) for a in qside]
        db = [_embedded(r, a, 16) for a in bside]
        dsq, dsb = _cuda(sq), _cuda(sb)
        for N in (1, 33, 255, 257, 289):
            for Q in (1, 97, 193):
                out = torch.full((Q, N + 9), SENTINEL, dtype=torch.float32, device='cuda')
                got = similarity(*[t[:Q] for t in dq], dsq[:Q], *[t[:N] for t in db], dsb[:N], D, out=out)
                assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (Q, N)
                g = out.cpu().numpy()
                ok = _bits_equal(g[:, :N], want[:Q, :N])
                assert ok.all(), (fmt, D, Q, N, np.argwhere(~ok)[:5])
                assert (g[:, N:] == SENTINEL).all(), (fmt, D, Q, N, 'a store past column N')


def _quantizer(fmt):
    from dirtorch_amd import ops
    return {'i8': (ops.quantize_rows, index_ref.quantize), 'fp4': (ops.quantize_rows_fp4, fp4_ref.quantize),
            'bin': (ops.quantize_rows_bin, bin_ref.quantize)}[fmt]


@pytest.mark.parametrize('fmt', FORMATS)
def test_row_walk(fmt):
    """One wave per row, four rows per workgroup: N = 1, 5, 9 leave one live wave in the last workgroup.  D = 1; 2047, 2048
    and 2049 around the edge between the row that stays in registers and the one read twice; 4097: three chunks.  Rows at
    pitch D + 3 (the scalar loads) and D + 4 (the vector loads), values over many binades - of the row and of its blocks of
    32 - with an all-zero row, a NaN and an infinity among them; the outputs land where a block full of 0x55 was freed, so a
    padding byte the kernel does not write shows."""
    quantize, restatement = _quantizer(fmt)
    for D in (1, 2047, 2048, 2049, 4097):
        r = np.random.RandomState(800 + D)
        x = r.standard_normal((9, D)) * np.exp(r.uniform(-12, 12, (9, 1)))
        x = (x * np.exp(r.uniform(-3, 3, (9, (D + 31) // 32)).repeat(32, axis=1)[:, :D])).astype(np.float32)
        x[1] = 0
        x[2, D // 2] = np.nan
        x[3, D - 1] = -np.inf
        want = restatement(x)
        assert np.isnan(want[-1][2:4]).all() and want[-1][1] == 0 and not want[0][1:4].any()
        for N in (1, 5, 9):
            for pitch in (3, 4):
                wide = torch.full((N, D + pitch), float('nan'), dtype=torch.float32, device='cuda')
                wide[:, :D] = _cuda(x[:N])
                junk = [torch.full((N,) + w.shape[1:], 0x55, dtype=torch.uint8, device='cuda') for w in want[:-1]]
                del junk
                got = [t.cpu().numpy() for t in quantize(wide[:, :D])]
                assert len(got) == len(want)
                for g, w in zip(got[:-1], want[:-1]):
                    assert g.dtype == w.dtype and g.shape == w[:N].shape, (fmt, D, N, pitch)
                    assert (g == w[:N]).all(), (fmt, D, N, pitch, np.argwhere(g != w[:N])[:5])
                assert (bits(got[-1]) == bits(want[-1][:N])).all(), (fmt, D, N, pitch, got[-1], want[-1][:N])
