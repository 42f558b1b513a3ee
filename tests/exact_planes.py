"""Operands on which the descriptor tail's kernels compute ONE fp32 number per score, whatever the order, and the zero-tolerance
reference built on them (a helper module like exact_conv.py; tests/test_exact_planes_cpu.py checks the claims below on the CPU,
tests/test_exact_planes_gpu.py uses them on the device).

The kernels (csrc/sim_split.hip, csrc/gemm_f32.hip) split every fp32 operand into bf16 planes x = h + m + l (or fp16 planes
2^10 x = h + l), multiply plane by plane on the matrix cores and keep the six (three) products of weight >= 2^-16 (2^-11).  On
operands that are small integers times powers of two
  * the split is exact (h + m + l == x) and every plane is a multiple of the operand's resolution,
  * the products the kernels drop by design (m*l' + l*m' + l*l', resp. l*l') are identically zero,
  * every sum of every subset of the kept plane products is a multiple of (query resolution x database resolution) and small
    enough to fit SUM_BITS = 22 significant bits - two to spare in fp32 -
so the two accumulators, the rotated K walk, split-K slices, MFMA block order and sharding all form the same fp32 number, and
every comparison is torch.equal over every element.  A lost or doubled plane product moves a score by a whole number of
resolution units; the legs below are chosen so that each kept product carries information in most scores.

Operand classes (value = scale x (H + M 2^-mf + L 2^-lf), H != 0 so that every drawn entry is non-zero):
    A    +-1                                                    planes h
    B    H in +-{1,2,3}, M in {-2..2}, mf = 9                  planes h, m          B1: the same with H = +-1
    C    H = +-1, M, L in {-1,0,1}, mf = 9, lf = 18            planes h, m, l
    P2   2^-4 (H + L 2^-12), H in +-{1..hmax}, L in {-3..3}    fp16 planes h, l of 2^10 x     A4: +-2^-4
    G    H in +-{1,2,3}, M in {-2..2}, mf = 7                  the exact fp32 chain has no planes: coarser, room for alpha / bias
A SPARSE operand keeps nnz entries of each row, at k = (base(n) + i) mod K, i < nnz, base(n) = nnz r + step t + shift for row
n = 256 t + r (step = the first odd number above nnz): the rows of a 256-row tile cover every k, and over 32 tiles every pair
(row within the tile, k mod 32) occurs - no lane of no strip is spared any position of a slab (sparse_coverage asserts it).

Legs (queries x database; the products that carry information, query plane first):
    six-1  C dense x A sparse     hh mh lh        six-2  A sparse x C dense     hh hm hl
    six-3  B dense x A dense      hh mh           six-3t A dense x B dense      hh hm
    six-4  B1 dense x B1 sparse   hh hm mh mm     (H = +-1 on both sides: with H up to 3 the sums would need 23 bits)
    pair-1 P2 dense x A4 (dense at D <= 256, sparse nnz 64 above)   hh lh       pair-2 its transpose   hh hl
    gemm   B (or G, with alpha / bias) dense x A dense: no planes
"""
import math

import torch

SUM_BITS = 22                 # the project's convention (exact_conv.SUM_BITS): fp32 holds 24
TILE, STRIP, QBLOCK, ABLOCK = 256, 32, 96, 32
FP16_MAX = 65504.0
FP16_MIN_NORMAL = 2.0 ** -14
PAIR_SCALE = 1024.0
BIAS_MAX = 32.0
ROW_CHUNK = 32768             # rows drawn at a time: temporaries stay 4-byte and under 300 MB at K = 2048

#            H max, M max, mf, L max, lf, scale
CLASSES = {'A': (1, 0, 0, 0, 0, 1.0), 'B': (3, 2, 9, 0, 0, 1.0), 'B1': (1, 2, 9, 0, 0, 1.0), 'C': (1, 1, 9, 1, 18, 1.0),
           'P2': (3, 0, 0, 3, 12, 2.0 ** -4), 'A4': (1, 0, 0, 0, 0, 2.0 ** -4), 'G': (3, 2, 7, 0, 0, 1.0)}

#        kind, queries, database, sparse side, products that carry information
LEGS = {'six-1': ('bf16', 'C', 'A', 'd', ('hh', 'mh', 'lh')),
        'six-2': ('bf16', 'A', 'C', 'q', ('hh', 'hm', 'hl')),
        'six-3': ('bf16', 'B', 'A', None, ('hh', 'mh')),
        'six-3t': ('bf16', 'A', 'B', None, ('hh', 'hm')),
        'six-4': ('bf16', 'B1', 'B1', 'd', ('hh', 'hm', 'mh', 'mm')),
        'pair-1': ('fp16', 'P2', 'A4', 'd', ('hh', 'lh')),
        'pair-2': ('fp16', 'A4', 'P2', 'q', ('hh', 'hl')),
        'gemm': ('f32', 'B', 'A', None, ()),
        'gemm-epi': ('f32', 'G', 'A', None, ())}
KEPT = {'bf16': ('hh', 'hm', 'mh', 'hl', 'lh', 'mm'), 'fp16': ('hh', 'hl', 'lh'), 'f32': ()}
DROPPED = {'bf16': ('ml', 'lm', 'll'), 'fp16': ('ll',), 'f32': ()}
SIX_LEGS = ('six-1', 'six-2', 'six-3', 'six-3t', 'six-4')
PAIR_LEGS = ('pair-1', 'pair-2')
# what the planes of an operand can exceed the operand by, in sum of magnitudes (|x - h| <= 2^-8 |x| for bf16, 2^-11 for fp16)
SLACK = {'bf16': (1 + 2.0 ** -7) ** 2, 'fp16': (1 + 2.0 ** -10) ** 2, 'f32': 1.0}


def class_max(name, hmax=None):
    h, m, mf, l, lf, scale = CLASSES[name]
    return scale * ((hmax or h) + m * 2.0 ** -mf + l * 2.0 ** -lf)


def class_res(name):
    h, m, mf, l, lf, scale = CLASSES[name]
    return scale * 2.0 ** -(lf if l else mf if m else 0)


def leg_nnz(leg, K):
    """Non-zero entries per row of the leg's sparse side at width K; None where both sides are dense.  Six-product legs: 8 at
    K >= 1024, 15 where K is shorter (both within 22 bits: 15 x 1.002 x 2^18 < 2^22); pair legs: dense up to K = 256, 64 above."""
    kind, qc, dc, sparse, _ = LEGS[leg]
    if sparse is None:
        return None
    if kind == 'fp16':
        return None if K <= 256 else 64
    return 8 if K >= 1024 else min(15, K // 2)


def sparse_step(nnz):
    return nnz + 1 if nnz % 2 == 0 else nnz + 2


def _log2(v):
    return int(round(math.log2(v)))


def _odd_part(a):
    m, e = math.frexp(abs(a))
    while m != int(m):
        m *= 2
    return int(m)


def plane_budget(leg, K, nnz=None, alphas=(1.0,), bias_max=0.0, hmax=None, bits=SUM_BITS):
    """[(where, largest possible magnitude, resolution, significant bits)] of everything a kernel can form on the leg's operands at
    width K with `nnz` non-zero terms per score (None: dense, K terms): one plane product; any sum of any subset of the kept plane
    products (the two accumulators acc / lo, the rotated K walk, split-K slices and MFMA block order are all such sums); the sum
    times alpha (alpha = odd x 2^e costs the bits of its odd part); plus a bias that is a multiple of the resolution.  Asserts
    bits <= `bits` at each, and for the fp16 legs |2^10 x| < 65 504 with every plane value a normal fp16 number."""
    kind, qc, dc, sparse, _ = LEGS[leg]
    qmax, dmax = class_max(qc, hmax if qc == 'P2' else None), class_max(dc, hmax if dc == 'P2' else None)
    res = class_res(qc) * class_res(dc)
    n = K if nnz is None else min(nnz, K)
    one = qmax * dmax * SLACK[kind]
    points = [('one plane product', one, res), ('any subset sum of the kept plane products, %d terms' % n, n * one, res)]
    for a in alphas:
        p2 = abs(a) / _odd_part(a)                 # alpha = odd x p2
        points.append(('sum x alpha = %g' % a, n * one * abs(a), res * p2))
        if bias_max:
            points.append(('sum x alpha = %g + bias' % a, n * one * abs(a) + bias_max, res * min(p2, 1.0)))
    out = []
    for where, mag, r in points:
        b = int(mag / r).bit_length()
        assert b <= bits, ('%s K = %d: %s: multiples of 2^%d up to %g need %d significant bits (budget %d, fp32 holds 24)'
                           % (leg, K, where, _log2(r), mag, b, bits))
        out.append((where, mag, r, b))
    if kind == 'fp16':
        for c in (qc, dc):
            assert PAIR_SCALE * class_max(c, hmax if c == 'P2' else None) < FP16_MAX and class_max(c) < 64
            assert PAIR_SCALE * class_res(c) >= FP16_MIN_NORMAL, '%s: a plane value below the smallest normal fp16' % c
    return out


def leg_hmax(leg, K, alphas=(1.0,)):
    """The largest H digit of the P2 class (3, 2 or 1) that keeps a pair leg with these alphas inside plane_budget: 3 except for
    a dense product of more than 64 terms scaled by 3 x 2^e (K = 256: 22 bits before alpha)."""
    if LEGS[leg][0] != 'fp16':
        return None
    for h in (3, 2, 1):
        try:
            plane_budget(leg, K, leg_nnz(leg, K), alphas, hmax=h)
            return h
        except AssertionError:
            continue
    raise AssertionError('%s K = %d alphas %r: no P2 lattice fits %d bits' % (leg, K, alphas, SUM_BITS))


def leg_resolution(leg):
    return class_res(LEGS[leg][1]) * class_res(LEGS[leg][2])


# ---- plane splits: the restatement of split2 / split2h (csrc/sim_split.hip) with torch's round-to-nearest-even conversions --------
def split_bf16(x):
    """(h, m, l) as fp32: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)."""
    x = x.float()
    h = x.bfloat16().float()
    m = (x - h).bfloat16().float()
    l = (x - h - m).bfloat16().float()
    return h, m, l


def split_fp16(x):
    """(h, l) as fp32, planes of 2^10 x: h = fp16(2^10 x), l = fp16(2^10 x - h)."""
    s = x.float() * PAIR_SCALE
    h = s.half().float()
    l = (s - h).half().float()
    return h, l


def planes(x, kind):
    """{'h': ..., 'm': ..., 'l': ...} of the kernel's split, in units of x (the fp16 planes divided by 2^10)."""
    if kind == 'bf16':
        return dict(zip('hml', split_bf16(x)))
    h, l = split_fp16(x)
    return {'h': h / PAIR_SCALE, 'l': l / PAIR_SCALE}


def plane_products(q, d, kind, names=None):
    """{name: fp64 [Q, N] sum over k of (query plane name[0]) x (database plane name[1])} on the CPU."""
    pq, pd = planes(q.cpu(), kind), planes(d.cpu(), kind)
    return {n: pq[n[0]].double() @ pd[n[1]].double().t() for n in (names or KEPT[kind] + DROPPED[kind])}


# ---- drawing -------------------------------------------------------------------------------------------------------------------------
def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def _ints(shape, lo, hi, g, device):
    return torch.randint(lo, hi + 1, shape, generator=g, device=device, dtype=torch.int8)      # (no 8-byte temporaries)


def draw_class(name, shape, g, device, hmax=None):
    """fp32 tensor of the class' lattice, every entry non-zero (|H| >= 1)."""
    h, m, mf, l, lf, scale = CLASSES[name]
    h = hmax or h
    x = _ints(shape, 1, h, g, device).float() if h > 1 else torch.ones(shape, device=device)
    x *= _ints(shape, 0, 1, g, device).float().mul_(2).sub_(1)
    if m:
        x += _ints(shape, -m, m, g, device).float().mul_(2.0 ** -mf)
    if l:
        x += _ints(shape, -l, l, g, device).float().mul_(2.0 ** -lf)
    return x.mul_(scale)


def sparse_base(rows, K, nnz, shift=0):
    """int32 [n]: first kept position of each row index in `rows` (int32 tensor)."""
    r, t = rows % TILE, rows // TILE
    return (nnz * r + sparse_step(nnz) * t + shift) % K


def sparse_mask(n0, n, K, nnz, device, shift=0):
    rows = torch.arange(n0, n0 + n, device=device, dtype=torch.int32)
    k = torch.arange(K, device=device, dtype=torch.int32)
    return ((k[None, :] - sparse_base(rows, K, nnz, shift)[:, None]) % K) < nnz


def draw_rows(name, N, K, device, seed, nnz=None, shift=0, hmax=None):
    """fp32 [N, K] of class `name`, dense or sparse, drawn ROW_CHUNK rows at a time (chunk c from the generator seeded
    seed * 4099 + c, so a crop of the first rows of a large operand is the same data)."""
    out = torch.empty(N, K, device=device)
    for c, i in enumerate(range(0, N, ROW_CHUNK)):
        n = min(ROW_CHUNK, N - i)
        x = draw_class(name, (n, K), _gen(device, seed * 4099 + c), device, hmax)
        if nnz is not None:
            x *= sparse_mask(i, n, K, nnz, device, shift)
        out[i:i + n] = x
    return out


def queries(leg, Q, D, device='cpu', seed=0, shift=0, alphas=(1.0,)):
    """The leg's queries [Q, D] alone; `shift` moves the kept positions of sparse queries (query_shifts: the calls that between
    them meet every k) without changing the generator's seed."""
    kind, qc, dc, sparse, _ = LEGS[leg]
    nnz, hmax = leg_nnz(leg, D), leg_hmax(leg, D, alphas)
    plane_budget(leg, D, nnz, alphas, hmax=hmax)
    return draw_rows(qc, Q, D, device, seed * 2 + 1, nnz if sparse == 'q' else None, shift, hmax if qc == 'P2' else None)


def operands(leg, Q, N, D, device='cpu', seed=0, shift=0, alphas=(1.0,)):
    """(queries [Q, D], database [N, D]) of the leg, fp32 on `device`, from seeded generators; asserts the leg's plane_budget."""
    kind, qc, dc, sparse, _ = LEGS[leg]
    nnz, hmax = leg_nnz(leg, D), leg_hmax(leg, D, alphas)
    q = queries(leg, Q, D, device, seed, shift, alphas)
    d = draw_rows(dc, N, D, device, seed * 2 + 2, nnz if sparse == 'd' else None, 0, hmax if dc == 'P2' else None)
    return q, d


def query_shifts(leg, Q, D):
    """The shifts of the calls a sparse-queries leg needs so that the union of the kept positions covers every k (one call, shift
    0, for every other leg): Q rows of nnz consecutive positions each, back to back, cover Q nnz positions per call."""
    nnz = leg_nnz(leg, D)
    if LEGS[leg][3] != 'q' or nnz is None:
        return [0]
    per = min(Q, TILE) * nnz
    return [c * per for c in range(-(-D // per))]


def query_coverage(leg, Q, D):
    """Number of k positions that the sparse queries of all query_shifts calls meet (D when complete)."""
    nnz = leg_nnz(leg, D)
    if LEGS[leg][3] != 'q' or nnz is None:
        return D
    met = torch.zeros(D, dtype=torch.bool)
    for s in query_shifts(leg, Q, D):
        met |= sparse_mask(0, Q, D, nnz, 'cpu', s).any(dim=0)
    return int(met.sum())


def sparse_coverage(N, K, nnz):
    """Conditions (a) and (b) of a sparse DATABASE of N rows: (a) the rows of every complete 256-row tile together meet every k;
    (b) over all tiles every (row within the tile, k mod 32) occurs.  Returns (tiles failing (a), pairs missing from (b))."""
    tiles = N // TILE
    rows = torch.arange(tiles * TILE, dtype=torch.int32)
    pos = (sparse_base(rows, K, nnz)[:, None] + torch.arange(nnz, dtype=torch.int32)[None, :]) % K          # [rows, nnz]
    met = torch.zeros(tiles, K, dtype=torch.bool)
    met.scatter_(1, pos.reshape(tiles, TILE * nnz).long(), True)
    pairs = torch.zeros(TILE, min(32, K), dtype=torch.bool)
    r = (rows % TILE)[:, None].expand_as(pos)
    pairs[r.reshape(-1).long(), (pos % 32).reshape(-1).long()] = True
    return int((~met.all(dim=1)).sum()), int((~pairs).sum())


# ---- reference ---------------------------------------------------------------------------------------------------------------------
CPU_REFERENCE_MAX = 1e10       # multiply-adds above which the fp64 product runs on the device, in chunks


def reference(q, d, chunk=65536):
    """fp32 [Q, N] on d's device: the fp64 product q . d^T, after asserting that its conversion to fp32 is exact.  On the CPU, or
    - above CPU_REFERENCE_MAX multiply-adds, for device operands - torch's own fp64 matmul on the device in chunks of `chunk`
    database rows (no code shared with the library), the first 4096 x 4096 scores cross-checked against the CPU."""
    Q, N, D = q.shape[0], d.shape[0], d.shape[1]
    if not d.is_cuda or float(Q) * N * D <= CPU_REFERENCE_MAX:
        r = q.cpu().double() @ d.cpu().double().t()
        r32 = r.float()
        assert torch.equal(r32.double(), r), 'the fp64 product is not exact in fp32: badly chosen operands'
        return r32.to(d.device)
    out = torch.empty(Q, N, device=d.device)
    q64 = q.double()
    for i in range(0, N, chunk):
        r = q64 @ d[i:i + chunk].double().t()
        r32 = r.float()
        assert torch.equal(r32.double(), r), 'the fp64 product is not exact in fp32: badly chosen operands'
        if i == 0:
            n = min(N, 4096)
            cpu = q[:4096].cpu().double() @ d[:n].cpu().double().t()
            assert torch.equal(cpu, r[:4096, :n].cpu()), 'device fp64 matmul differs from the CPU on the first rows'
        out[:, i:i + chunk] = r32
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def mismatch_report(got, want, what, resolution):
    """None when got == want ([Q, N] fp32, any device; +0 == -0) in every element; otherwise the text of the finding: how many
    elements differ, the first (query row q, database row n) with its 256-row tile, 32-row strip, query block of 96 and accumulator
    block, got / want as values and bit patterns, and got - want in units of `resolution` (a whole number of 2^-18 units names a
    missing l product, of 2^-9 units a missing m product, and so on; a fraction a term that went through a rounding)."""
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return None
    bad = got != want                     # (a NaN - which the lattice cannot produce - differs from everything)
    n_bad = int(bad.sum())
    per_q = bad.sum(dim=1)
    q = int((per_q > 0).nonzero()[0])
    n = int(bad[q].nonzero()[0])
    gv, wv = float(got[q, n]), float(want[q, n])
    gb, wb = int(_bits(got[q, n].reshape(1))[0]) & 0xffffffff, int(_bits(want[q, n].reshape(1))[0]) & 0xffffffff
    cols = bad.any(dim=0).nonzero().reshape(-1)
    tiles = int(torch.unique(cols // TILE).numel())
    return ('%s: %d / %d elements differ (%.3f %%), in %d of %d query rows and %d of %d database tiles; first at query row %d '
            '(block of 96: %d, accumulator block %d), database row %d (tile %d, strip %d, lane row %d): got %r (0x%08x) want %r '
            '(0x%08x); got - want = %g units of 2^%d'
            % (what, n_bad, bad.numel(), 100.0 * n_bad / bad.numel(), int((per_q > 0).sum()), got.shape[0], tiles,
               -(-got.shape[1] // TILE), q, q // QBLOCK, (q % QBLOCK) // ABLOCK, n, n // TILE, (n % TILE) // STRIP, n % STRIP,
               gv, gb, wv, wb, (gv - wv) / resolution, _log2(resolution)))


def report_mismatch(got, want, what, resolution):
    """Fail (AssertionError carrying mismatch_report's text) unless got == want in every element."""
    msg = mismatch_report(got, want, what, resolution)
    assert msg is None, msg


# ---- the cases of tests/test_exact_planes_gpu.py (tests/test_exact_planes_cpu.py checks the conditions on each) ----------------------
SIM_SHAPES = [(70, 40000, 2048), (1, 33000, 64), (97, 32768 + 255, 512), (200, 50001, 128), (193, 32768, 32), (96, 65536 + 31, 96)]
BIG_SHAPE = (70, 1006322, 2048)
BIG_LEGS = ('six-1', 'pair-1')
SHARD_SHAPE = (24, 300007, 2048)
SHARD_LEGS = ('six-1', 'six-4', 'pair-1')
GEMM_SHAPES = [(2048, 1, 2048), (2048, 8, 2048), (96, 40, 96), (33, 7, 96), (130, 70, 64), (257, 131, 128), (5, 200, 36),
               (2048, 32, 2048), (2048, 64, 2048), (2048, 256, 2048), (515, 33, 2080), (300, 70, 1031), (2048, 5, 512)]
GEMM_SPLIT = {(2048, 32, 2048), (2048, 64, 2048), (2048, 256, 2048), (515, 33, 2080), (300, 70, 1031), (2048, 5, 512),
              (2048, 8, 2048)}                                  # the shapes test_gemm_nt_f32 asserts to run in K slices
GEMM_BIG_QSUB = [(300, 70, 1031), (257, 33, 37)]               # K % 4 != 0: the element-wise gather and its zero-filled tail
GEMM_ALPHAS = (0.5, 1.0, 2.0, 3.0)
# (N, D, v) of ops.pca_whiten
WHITEN_SHAPES = [(40013, 2048, 2048), (33000, 2048, 128), (32768 + 256 * 3, 256, 97), (33000, 64, 1), (32768 + 256 * 5 + 7, 512, 200)]
WHITEN_ALPHAS = (0.125, 1.0, 4.0, 0.75, 6.0)                   # powers of two and 3 x 2^e
WHITEN_LEGS = ('pair-2', 'pair-1')                              # components in the queries' place: sparse components / sparse X - mean


def gemm_operands(NP, NQ, K, device, seed, epilogue, big_qsub=False):
    """P [NP, K] (class A), the lattice part of Q [NQ, K] (class G with an epilogue, B without) and - with an epilogue - qsub [K],
    bias [NP], alpha [NP]: Q = lattice + qsub is exact in fp32 (qsub a multiple of 2^-7 of magnitude <= 4, or - big_qsub - an
    integer of magnitude 2048 ... 4095: 20 bits), alpha cycles through GEMM_ALPHAS, bias a multiple of 2^-7 within +-32."""
    leg = 'gemm-epi' if epilogue else 'gemm'
    plane_budget(leg, K, None, GEMM_ALPHAS if epilogue else (1.0,), BIAS_MAX if epilogue else 0.0)
    lat, P = operands(leg, NQ, NP, K, device, seed)
    if not epilogue:
        return P, lat, None, None, None
    g = _gen(device, seed + 77)
    if big_qsub:
        qsub = torch.randint(2048, 4096, (K,), generator=g, device=device, dtype=torch.int16).float()
        qsub *= _ints((K,), 0, 1, g, device).float().mul_(2).sub_(1)
    else:
        qsub = torch.randint(-512, 513, (K,), generator=g, device=device, dtype=torch.int16).float().mul_(2.0 ** -7)
    bias = torch.randint(-4096, 4097, (NP,), generator=g, device=device, dtype=torch.int16).float().mul_(2.0 ** -7)
    alpha = torch.tensor(GEMM_ALPHAS, device=device)[torch.arange(NP, device=device) % len(GEMM_ALPHAS)].contiguous()
    return P, lat, qsub, bias, alpha


def lattice_mean(D, device, seed):
    """A strong common mean: multiples of 2^-10 in [1/4, 1/2).  X = lattice + mean stays a multiple of 2^-16 below 1 (16 bits),
    2^10 mean is exact, and X - mean gives the lattice back exactly."""
    g = _gen(device, seed + 99)
    return torch.randint(256, 512, (D,), generator=g, device=device, dtype=torch.int16).float().mul_(2.0 ** -10)
