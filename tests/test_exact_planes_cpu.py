"""The conditions on the INPUTS of the bit-exact plane tests (tests/exact_planes.py), met by the CPU reference alone.

For every (leg, shape) tests/test_exact_planes_gpu.py uses - statistics on a crop of at most 1024 database rows, they are a
property of the leg, the width and nnz, not of the row count:
  * plane_budget holds (and refuses a leg that is not exact);
  * the plane split is exact for both operands, and every plane the leg is there for is non-zero in >= 30 % of the entries;
  * the plane products the kernels drop by design are identically zero at every k;
  * the kept plane products sum, in fp64, to the fp64 dot product, which is its own fp32 conversion;
  * leaving out any product the leg is there for changes at least half of the scores; over all legs every kept product of the
    six-product and of the three-product form is covered; at least 90 % of the scores are non-zero;
  * sparse layouts: the rows of a 256-row tile meet every k, over the tiles every (row, k mod 32) occurs; sparse queries meet
    every k over the repeated calls.
These are conditions, not measurements: inputs that miss one are badly chosen and are replaced.
"""
import functools

import pytest
import torch

import exact_planes as E

CROP = 1024


def _sim_cases():
    out = [(leg,) + s for s in E.SIM_SHAPES for leg in E.SIX_LEGS + E.PAIR_LEGS]
    out += [(leg,) + E.BIG_SHAPE for leg in E.BIG_LEGS] + [(leg,) + E.SHARD_SHAPE for leg in E.SHARD_LEGS]
    return [c + ((1.0,),) for c in out]


def _whiten_cases():
    return [(leg, v, N, D, E.WHITEN_ALPHAS) for N, D, v in E.WHITEN_SHAPES for leg in E.WHITEN_LEGS]


CASES = _sim_cases() + _whiten_cases()
IDS = ['%s-%dx%dx%d%s' % (c[:4] + ('-alpha' if len(c[4]) > 1 else '',)) for c in CASES]


@functools.lru_cache(maxsize=None)
def _crop(leg, Q, D, alphas, shift=0):
    """(q, d, fp64 plane products, reference) of the leg at width D on the CPU: Q query rows, CROP database rows."""
    q, d = E.operands(leg, Q, CROP, D, 'cpu', seed=Q * 7 + D, shift=shift, alphas=alphas)
    kind = E.LEGS[leg][0]
    return q, d, E.plane_products(q, d, kind), E.reference(q, d)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_budget_and_layout(case):
    leg, Q, N, D, alphas = case
    nnz, hmax = E.leg_nnz(leg, D), E.leg_hmax(leg, D, alphas)
    pts = E.plane_budget(leg, D, nnz, alphas, hmax=hmax)
    assert max(p[3] for p in pts) <= E.SUM_BITS
    sparse = E.LEGS[leg][3]
    if nnz is not None and sparse == 'd':
        assert E.TILE * nnz >= D
        assert E.sparse_coverage(N, D, nnz) == (0, 0), 'sparse database %r: (tiles that miss a k, (row, k mod 32) pairs never met)' % (case,)
    if nnz is not None and sparse == 'q':
        assert E.query_coverage(leg, Q, D) == D, 'sparse queries %r: the calls do not meet every k' % (case,)


def test_budget_refuses_what_is_not_exact():
    with pytest.raises(AssertionError):
        E.plane_budget('six-1', 2048, None)                   # dense C x dense A: 30 bits
    with pytest.raises(AssertionError):
        E.plane_budget('pair-1', 2048, None)                  # dense P2 x dense A4 at D = 2048: 25 bits
    with pytest.raises(AssertionError):
        E.plane_budget('pair-1', 256, None, (3.0,), hmax=3)   # 22 bits before alpha = 3
    assert E.leg_hmax('pair-1', 256, (3.0,)) == 1 and E.leg_hmax('pair-1', 256) == 3 and E.leg_hmax('pair-1', 2048, (6.0,)) == 3
    with pytest.raises(AssertionError):
        E.plane_budget('gemm', 4160, None)
    E.plane_budget('six-1', 2048, 8)
    E.plane_budget('six-1', 512, 15)
    with pytest.raises(AssertionError):
        E.plane_budget('six-1', 2048, 16)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_planes_and_products(case):
    leg, Q, N, D, alphas = case
    kind, qc, dc, sparse, carried = E.LEGS[leg]
    q, d, prod, ref = _crop(leg, min(Q, 200), D, alphas)
    for name, x, role in (('queries', q, 0), ('database', d, 1)):
        pl = E.planes(x, kind)
        assert torch.equal(sum(p.double() for p in pl.values()), x.double()), '%s %s: the planes do not add up to x' % (leg, name)
        nz = x != 0
        assert int(nz.sum()) > 0
        for p in sorted({c[role] for c in carried}):
            share = float((pl[p][nz] != 0).float().mean())
            assert share >= 0.30, '%s %s: plane %s is non-zero in only %.1f %% of the non-zero entries' % (leg, name, p, 100 * share)
    # what the kernels drop is zero at every k: the sum over k of |plane| x |plane'| is
    pq, pd = E.planes(q, kind), E.planes(d, kind)
    for n in E.DROPPED[kind]:
        assert float((pq[n[0]].abs().double() @ pd[n[1]].abs().double().t()).max()) == 0.0, '%s: dropped product %s is not zero' % (leg, n)
    kept = sum(prod[n] for n in E.KEPT[kind])
    assert torch.equal(kept, ref.double()), '%s: the kept plane products do not sum to the fp64 dot product' % leg
    assert float((ref != 0).float().mean()) >= 0.90, '%s: %.1f %% of the scores are non-zero' % (leg, 100 * float((ref != 0).float().mean()))
    for n in carried:
        share = float(((kept - prod[n]) != ref.double()).float().mean())
        assert share >= 0.50, '%s: leaving out %s changes only %.1f %% of the scores' % (leg, n, 100 * share)
    # resolution: every score is a whole number of the leg's units (what mismatch_report counts in)
    units = ref.double() / E.leg_resolution(leg)
    assert torch.equal(units, units.round())


def test_every_kept_product_is_some_legs_business():
    for kind, legs in (('bf16', E.SIX_LEGS), ('fp16', E.PAIR_LEGS)):
        covered = set()
        for leg in legs:
            covered |= set(E.LEGS[leg][4])
        assert covered == set(E.KEPT[kind]), (kind, covered)
    assert {n for leg in E.BIG_LEGS for n in E.LEGS[leg][4]} >= {'hh', 'mh', 'lh'}


def test_sparse_query_calls_change_the_positions():
    """six-2 at Q = 1, D = 64: several calls, disjoint positions, each call's operands pass the same conditions."""
    shifts = E.query_shifts('six-2', 1, 64)
    assert len(shifts) > 1
    seen = torch.zeros(64, dtype=torch.bool)
    for s in shifts:
        q, d, prod, ref = _crop('six-2', 1, 64, (1.0,), s)
        assert not bool((seen & (q[0] != 0)).any()) or s == shifts[-1]
        seen |= q[0] != 0
        assert torch.equal(sum(prod[n] for n in E.KEPT['bf16']), ref.double())
    assert bool(seen.all())
    assert E.query_shifts('six-2', 70, 2048) == [0, 560, 1120, 1680] and E.query_shifts('six-1', 70, 2048) == [0]


@pytest.mark.parametrize('shape', E.GEMM_SHAPES + E.GEMM_BIG_QSUB, ids=lambda s: '%dx%dx%d' % s)
def test_gemm_lattice(shape):
    NP, NQ, K = shape
    for epilogue, big in ((False, False), (True, False)) + (((True, True),) if shape in E.GEMM_BIG_QSUB else ()):
        P, lat, qsub, bias, alpha = E.gemm_operands(min(NP, 512), min(NQ, 64), K, 'cpu', NP + NQ + K, epilogue, big)
        ref = lat.double() @ P.double().t()
        assert torch.equal(ref.float().double(), ref) and float((ref != 0).float().mean()) >= 0.90
        if epilogue:
            Q = lat + qsub
            assert torch.equal(Q.double(), lat.double() + qsub.double()) and torch.equal(Q - qsub, lat)
            full = ref * alpha.double() + bias.double()
            assert torch.equal(full.float().double(), full)
            if big:
                assert float(qsub.abs().min()) >= 2048 and float(lat.abs().max()) < 4


def test_whiten_mean_keeps_x_exact():
    for N, D, v in E.WHITEN_SHAPES:
        mean = E.lattice_mean(D, 'cpu', D)
        for leg in E.WHITEN_LEGS:
            comps, lat = E.operands(leg, min(v, 64), 512, D, 'cpu', seed=v, alphas=E.WHITEN_ALPHAS)
            X = lat + mean
            assert torch.equal(X.double(), lat.double() + mean.double()) and torch.equal(X - mean, lat)
            # the kernel's one fma per value, fma(X, 2^10, -2^10 mean): its exact value is the scaled lattice, so it rounds nowhere
            assert torch.equal(X.double() * E.PAIR_SCALE - (mean * E.PAIR_SCALE).double(), (lat * E.PAIR_SCALE).double())
            assert float(X.min()) > 0 and float(X.abs().max()) < 1 and float(lat.abs().max()) < 64
            for a in E.WHITEN_ALPHAS:
                r = E.reference(lat, comps).double() * a
                assert torch.equal(r.float().double(), r)


def test_mismatch_report_names_the_place():
    want = torch.zeros(100, 600)
    assert E.mismatch_report(want.clone(), want, 'x', 2.0 ** -18) is None
    assert E.mismatch_report(-want, want, 'x', 2.0 ** -18) is None            # +0 == -0
    got = want.clone()
    got[97, 300] = 3 * 2.0 ** -18
    got[98, 599] = 1.0
    msg = E.mismatch_report(got, want, 'leg', 2.0 ** -18)
    assert '2 / 60000 elements differ' in msg and 'query row 97 (block of 96: 1, accumulator block 0)' in msg
    assert 'database row 300 (tile 1, strip 1, lane row 12)' in msg and '= 3 units of 2^-18' in msg
    with pytest.raises(AssertionError):
        E.report_mismatch(got, want, 'leg', 2.0 ** -18)
