"""-m gpu: the nine C exports of the Encoder in two parts (the stage-3 / stage-4 cache route of sv.Stage3Cache / sv.Stage4Cache), each called
directly and compared with the fp64 oracle at EVERY position and every one of the 128 channels - not after the 4 000x of MaxPools behind them,
where a wrong value survives only if it is a window's argmax - and the route's assembly (sv.s3_assemble / sv.s4_assemble) per position on a
small chromosome.  f16x2 arithmetic (the only one these entries accept).  Bounds are relative to the stage's max |ref| (`rel_err`)."""
import numpy as np
import pytest
import torch

from orca_amd import engine, sv
from orca_amd._lib import OrcaHipError
from tests.encoder_ref import P16_GUARD, WEIGHTS, WINDOWS, chromosome, encoder_sd, pack_p16, pool5, rel_err, stages, strand_codes, unpack_p16

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(1234.5)


def _net(cuda, seed, gain):
    from orca_amd import orca_modules as pm
    m = pm.Encoder()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in encoder_sd(seed, gain).items()}, strict=True)
    return m.eval().to(cuda)


@pytest.fixture(scope="module")
def nets(cuda):
    return {w: _net(cuda, *w) for w in (WEIGHTS[0], WEIGHTS[2])}


@pytest.fixture(scope="module")
def net(nets):
    return nets[WEIGHTS[0]]


def _codes(L, seed):
    rs = np.random.RandomState(seed)
    c = rs.randint(0, 4, L).astype(np.uint8)
    for s in rs.randint(0, max(1, L - 60), max(1, L // 3000)):
        c[s: s + 60] = 4                                                  # N runs
    if L > 200:
        c[:23] = 4                                                        # ... one at the start
    return c


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _untouched(planes, before, units_lo, units_hi):
    """Every unit of every plane outside [units_lo, units_hi) has the bits it had before."""
    a, b = planes.cpu().numpy().view(np.uint32), before.view(np.uint32)
    return np.array_equal(a[:, :units_lo], b[:, :units_lo]) and np.array_equal(a[:, units_hi:], b[:, units_hi:])


# ---- orca_encoder_stage3_planes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [WEIGHTS[0], WEIGHTS[2]])
def test_stage3_planes_every_position(nets, cuda, w):
    """Stage 3 (before MaxPool1d(5)) of L / 16 = 5, 255, 260, 510, 515 positions (around the conv tiles), both strands, N runs: every position
    including the first and last ~25 (where the composed 17/25-tap groups fix their edges) against the fp64 oracle on the same bases.
    Worst observed on the MI355X: 1.69e-6 (seed 0), 1.56e-6 (gain 1.6); bound 6e-6."""
    net = nets[w]
    sd = encoder_sd(*w)
    worst = 0.0
    for n in (5, 255, 260, 510, 515):
        codes = _codes(16 * n, 300 + n)
        for rev in (False, True):
            planes = net.stage3_planes(_dev(codes, cuda), reverse=rev)
            assert tuple(planes.shape) == (32, engine.p16_plane_units(n), 4)
            ref = stages(sd, strand_codes(codes, rev), 3)[3]
            got = unpack_p16(planes, n)
            err = rel_err(got, ref)
            worst = max(worst, err)
            assert err <= 6e-6, (n, rev, err)
    print(f"stage3_planes {w}: worst {worst:.3g}")


def test_stage3_planes_large_launch(net, cuda):
    """One launch of 65 600 positions (>= 65 536: the large-sequence kernels of conv_p16x.h), both strands: the first and last 40 positions
    and 40 around positions 32 768 and 65 536, against the oracle on slices of +-512 bases around them (exact: the reach is 336 bases,
    test_encoder_stages_cpu.py).  Worst observed on the MI355X: 1.71e-6; bound 6e-6."""
    n = 65_600
    codes = _codes(16 * n, 9)
    sd = encoder_sd(*WEIGHTS[0])
    worst = 0.0
    for rev in (False, True):
        got = unpack_p16(net.stage3_planes(_dev(codes, cuda), reverse=rev), n)
        sc = strand_codes(codes, rev)
        for a in (0, 32_748, 65_516, n - 40):
            b0, b1 = max(0, 16 * a - 512), min(16 * n, 16 * (a + 40) + 512)
            ref = stages(sd, sc[b0: b1], 3)[3][(16 * a - b0) // 16: (16 * a - b0) // 16 + 40]
            err = rel_err(got[a: a + 40], ref)
            worst = max(worst, err)
            assert err <= 6e-6, (rev, a, err)
    print(f"stage3_planes large: worst {worst:.3g}")


# ---- the pools ------------------------------------------------------------------------------------------------------------------------------
POOL_CASES = [(1, 3, 2), (255, 0, 7), (256, 11, 0), (257, 5, 300), (70_001, 9, 40)]     # (count, src_pos0, dst_pos0)


@pytest.mark.parametrize("count,src_pos0,dst_pos0", POOL_CASES + [(300, None, None)])
def test_p16_pool5_into(net, cuda, count, src_pos0, dst_pos0):
    """orca_p16_pool5_into on random values packed with `pack_p16`: positions [dst_pos0, dst_pos0 + count) = MaxPool1d(5) of the decoded source
    from src_pos0, exactly (the pool re-splits the max of hi + lo); every other unit of the destination keeps its sentinel.  (None, None): the
    source read to its last unit and the destination written to its last."""
    rs = np.random.RandomState(count)
    ctx = engine.get_context(cuda)
    n_src = 5 * count + (src_pos0 or 0) + 13
    src_units = engine.p16_plane_units(n_src)
    if src_pos0 is None:
        src_pos0 = src_units - P16_GUARD - 5 * count
        n_src = src_units - P16_GUARD
    vals = (rs.randn(n_src, 128) * 3).astype(np.float32)
    src = _dev(pack_p16(vals, src_units), cuda)
    dec = unpack_p16(src, n_src)
    dst_units = engine.p16_plane_units(count + (dst_pos0 or 0) + 4)
    if dst_pos0 is None:
        dst_pos0 = dst_units - P16_GUARD - count
    before = np.full((32, dst_units, 4), SENTINEL, np.float32)
    dst = _dev(before, cuda)
    engine.p16_pool5_into(ctx, src, src_pos0, dst, dst_pos0, count)
    torch.cuda.synchronize(cuda)
    got = unpack_p16(dst, dst_pos0 + count)[dst_pos0:]
    assert np.array_equal(got, pool5(dec[src_pos0: src_pos0 + 5 * count]))
    assert _untouched(dst, before, P16_GUARD + dst_pos0, P16_GUARD + dst_pos0 + count)


@pytest.mark.parametrize("count,src_pos0,dst_pos0", POOL_CASES + [(300, None, None)])
def test_rows_pool5_into(net, cuda, count, src_pos0, dst_pos0):
    """orca_rows_pool5_into on random fp32 rows: rows [dst_pos0, dst_pos0 + count) = MaxPool1d(5) of the source rows from src_pos0, exactly;
    every other row keeps its sentinel.  (None, None): the source read to its last row, the destination written to its last."""
    rs = np.random.RandomState(1000 + count)
    ctx = engine.get_context(cuda)
    n_src = 5 * count + (src_pos0 if src_pos0 is not None else 0) + (0 if src_pos0 is None else 7)
    if src_pos0 is None:
        src_pos0 = 0
    vals = (rs.randn(n_src, 128) * 3).astype(np.float32)
    n_dst = count + (dst_pos0 if dst_pos0 is not None else 0) + (0 if dst_pos0 is None else 6)
    dst_pos0 = n_dst - count if dst_pos0 is None else dst_pos0
    before = np.full((n_dst, 128), SENTINEL, np.float32)
    dst = _dev(before, cuda)
    engine.rows_pool5_into(ctx, _dev(vals, cuda), src_pos0, dst, dst_pos0, count)
    got = dst.cpu().numpy()
    assert np.array_equal(got[dst_pos0: dst_pos0 + count], pool5(vals[src_pos0: src_pos0 + 5 * count]))
    assert (got[:dst_pos0] == SENTINEL).all() and (got[dst_pos0 + count:] == SENTINEL).all()


# ---- the fronts ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rev", [False, True])
def test_front_snippet(net, cuda, rev):
    """orca_encoder_front_snippet: stages 1-3 + MaxPool1d(5) on strand bases [base0, base0 + nbases) alone (zero padded at the snippet's own
    ends; ``base0`` in strand coordinates), pooled positions [skip, skip + count) at dst_pos0; sentinels elsewhere.  Snippets at the window's
    start, inside it (base0 off the 80-base grid too) and at its end, N runs.  Worst observed on the MI355X: 2.18e-6; bound 8e-6."""
    L = 12_000
    codes = _codes(L, 21)
    sc = strand_codes(codes, rev)
    sd = encoder_sd(*WEIGHTS[0])
    dcodes = _dev(codes, cuda)
    n_dst = 90
    units = engine.p16_plane_units(n_dst)
    worst = 0.0
    for base0, nbases, skip, count, dst_pos0 in [(0, 4000, 0, 50, 0), (1600, 4000, 7, 30, 11), (2416, 3200, 3, 37, 53), (L - 4800, 4800, 20, 40, n_dst - 40)]:
        before = np.full((32, units, 4), SENTINEL, np.float32)
        dst = _dev(before, cuda)
        net.front_snippet(dcodes, rev, base0, nbases, skip, count, dst, dst_pos0)
        ref = pool5(stages(sd, sc[base0: base0 + nbases], 3)[3])[skip: skip + count]
        err = rel_err(unpack_p16(dst, dst_pos0 + count)[dst_pos0:], ref)
        worst = max(worst, err)
        assert err <= 8e-6, (base0, err)
        assert _untouched(dst, before, P16_GUARD + dst_pos0, P16_GUARD + dst_pos0 + count)
    print(f"front_snippet rev={rev}: worst {worst:.3g}")


@pytest.mark.parametrize("rev", [False, True])
def test_front4_snippet_and_ranges(net, cuda, rev):
    """orca_encoder_front4_snippet: stages 1-4 + MaxPool1d(5) on strand bases [base0, base0 + nbases) alone, pooled rows [skip, skip + count) at
    dst_pos0, sentinel rows elsewhere; orca_encoder_front4_ranges: several ranges of ONE run over all of its bases.  Worst observed on the
    MI355X: 1.85e-6; bound 7e-6."""
    L = 24_000
    codes = _codes(L, 22)
    sc = strand_codes(codes, rev)
    sd = encoder_sd(*WEIGHTS[0])
    dcodes = _dev(codes, cuda)
    n_dst = 60
    worst = 0.0
    for base0, nbases, skip, count, dst_pos0 in [(0, 8000, 0, 20, 0), (4000, 8000, 2, 15, 5), (L - 9200, 9200, 3, 20, n_dst - 20)]:
        dst = _dev(np.full((n_dst, 128), SENTINEL, np.float32), cuda)
        net.front4_snippet(dcodes, rev, base0, nbases, skip, count, dst, dst_pos0)
        ref = pool5(stages(sd, sc[base0: base0 + nbases], 4)[4])[skip: skip + count]
        got = dst.cpu().numpy()
        err = rel_err(got[dst_pos0: dst_pos0 + count], ref)
        worst = max(worst, err)
        assert err <= 7e-6, (base0, err)
        assert (got[:dst_pos0] == SENTINEL).all() and (got[dst_pos0 + count:] == SENTINEL).all()
    # ranges of one run over 16 000 bases (40 pooled rows) - the run's own ends are its sequence's, as in sv.s4_assemble
    run = _codes(16_000, 23)
    ranges = [(0, 6, 0), (17, 5, 20), (34, 6, n_dst - 6)]
    dst = _dev(np.full((n_dst, 128), SENTINEL, np.float32), cuda)
    net.front4_ranges(_dev(run, cuda), rev, ranges, dst)
    got, written = dst.cpu().numpy(), np.zeros(n_dst, bool)
    ref = pool5(stages(sd, strand_codes(run, rev), 4)[4])
    for skip, count, pos0 in ranges:
        err = rel_err(got[pos0: pos0 + count], ref[skip: skip + count])
        worst = max(worst, err)
        assert err <= 7e-6, (skip, err)
        written[pos0: pos0 + count] = True
    assert (got[~written] == SENTINEL).all()
    print(f"front4 rev={rev}: worst {worst:.3g}")


# ---- the backs, fed from the oracle ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def back_inputs():
    """The oracle's stage-4 input of 40 kb (500 positions, N runs), rounded to fp32 as the planes hold it, and its stages 4-7 in fp64."""
    sd = encoder_sd(*WEIGHTS[0])
    s4 = pool5(stages(sd, _codes(40_000, 31), 3)[3]).astype(np.float32)
    planes = pack_p16(s4, engine.p16_plane_units(500))
    ref = stages(sd, unpack_p16(planes, 500), 7, first=4)
    return planes, ref


def test_stage4_rows(net, cuda, back_inputs):
    """orca_encoder_stage4_rows from `pack_p16` planes of the oracle's pooled stage 3: every row against the oracle's stage 4 on the same
    (decoded) values.  Observed on the MI355X: 1.27e-6; bound 5e-6."""
    planes, ref = back_inputs
    rows = net.stage4_rows(_dev(planes, cuda), 500).cpu().numpy()
    err = rel_err(rows, ref[4])
    print(f"stage4_rows: {err:.3g}")
    assert err <= 5e-6


def test_back(net, cuda, back_inputs):
    """orca_encoder_back (stages 4-7) from `pack_p16` planes, n4 = 500: the 10 bins against the oracle's stage 7.  Observed on the MI355X: 1.96e-6;
    bound 7e-6."""
    planes, ref = back_inputs
    out = torch.full((128, 10), float("nan"), device=cuda)
    net.back(_dev(planes, cuda), 500, out)
    err = rel_err(out.cpu().numpy().T, ref[7])
    print(f"back: {err:.3g}")
    assert err <= 7e-6


def test_back5(net, cuda, back_inputs):
    """orca_encoder_back5 (stages 5-7) from fp32 rows of the oracle's stage-5 input (MaxPool1d(5) of its stage 4), n5 = 100: the 10 bins
    against the oracle's stages 5-7 on the same values.  Observed on the MI355X: 1.74e-6; bound 6e-6."""
    sd = encoder_sd(*WEIGHTS[0])
    _, ref = back_inputs
    s5 = pool5(ref[4]).astype(np.float32)
    ref5 = stages(sd, s5, 7, first=5)
    out = torch.full((128, 10), float("nan"), device=cuda)
    net.back5(_dev(s5, cuda), out)
    err = rel_err(out.cpu().numpy().T, ref5[7])
    print(f"back5: {err:.3g}")
    assert err <= 6e-6


# ---- the route, per position -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [3, 4])
def test_route_assembly_every_position(net, cuda, level):
    """sv.s3_assemble / sv.s4_assemble (what s3_encode / _s4_encode hand to `back` / `back5`) on a 64 kb chromosome with N runs, from a
    Stage3Cache / Stage4Cache of the whole chromosome and of a region: the windows of test_encoder_stages_cpu.py (a deletion, a duplication,
    an inversion, pieces at both chromosome ends, 4 - 48 kb, windows partly outside the region), both strands, assembled into a NaN-filled
    buffer - no NaN left in [0, n), and every position against the fp64 oracle's pooled stage 3 / 4 of the whole assembled window.  Worst
    observed on the MI355X: 2.06e-6 (level 3), 2.04e-6 (level 4); bound 8e-6."""
    codes = chromosome()
    C = len(codes)
    genome = _dev(codes, cuda)
    sd = encoder_sd(*WEIGHTS[0])
    Cache = sv.Stage3Cache if level == 3 else sv.Stage4Cache
    caches = {}
    worst, taken = 0.0, 0
    for pieces, region in WINDOWS:
        if region not in caches:
            caches[region] = Cache(net, genome, region=region)
        cache = caches[region]
        L = sum(p[1] for p in pieces)
        fw = sv.assemble_codes(codes, pieces)
        w = _dev(fw, cuda)
        for rev in (False, True):
            pcs = sv.revcomp_pieces(pieces) if rev else pieces
            takes, _ = sv.s3_plan(pcs, C, L, regions=cache.region, **({} if level == 3 else
                                  dict(margin=sv.S4_MARGIN_BP, grid=sv.S4_GRID, pad=sv.S4_PAD_BP, min_snippet=sv.S4_MIN_SNIPPET_BP)))
            taken += len(takes)
            ref = pool5(stages(sd, strand_codes(fw, rev), level)[level])
            n = len(ref)
            if level == 3:
                buf = torch.full((32, engine.p16_plane_units(n), 4), float("nan"), device=cuda)
                out, _ = sv.s3_assemble(net, {None: cache}, pcs, w, rev, s4=buf)
                got = unpack_p16(out, n)
            else:
                buf = torch.full((n, 128), float("nan"), device=cuda)
                out, _ = sv.s4_assemble(net, {None: cache}, pcs, w, rev, s5=buf)
                got = out.cpu().numpy().astype(np.float64)
            assert out is buf and not np.isnan(got).any(), (pieces, rev)
            err = rel_err(got, ref)
            worst = max(worst, err)
            assert err <= 8e-6, (pieces, region, rev, err)
    assert taken > 0
    print(f"route level {level}: worst {worst:.3g}")


# ---- argument checks (bounds the C side validates before it launches anything that reads them) ----------------------------------------------
def test_argument_checks(net, cuda):
    """Out-of-range positions, rows, bases and sizes are refused with ORCA_EINVAL before any kernel reads or writes them."""
    ctx = engine.get_context(cuda)
    units = engine.p16_plane_units(100)
    p = torch.zeros((32, units, 4), dtype=torch.float32, device=cuda)
    q = torch.zeros((32, units, 4), dtype=torch.float32, device=cuda)
    with pytest.raises(OrcaHipError, match="orca_p16_pool5_into"):
        engine.p16_pool5_into(ctx, p, units - P16_GUARD - 5 * 10 + 1, q, 0, 10)          # one position past the source
    with pytest.raises(OrcaHipError, match="orca_p16_pool5_into"):
        engine.p16_pool5_into(ctx, p, 0, q, units - P16_GUARD - 10 + 1, 10)              # ... past the destination
    r = torch.zeros((50, 128), dtype=torch.float32, device=cuda)
    with pytest.raises(OrcaHipError, match="orca_rows_pool5_into"):
        engine.rows_pool5_into(ctx, r, 1, r, 0, 10)                                       # rows [1, 51) of 50
    with pytest.raises(OrcaHipError, match="orca_rows_pool5_into"):
        engine.rows_pool5_into(ctx, r, 0, r, 41, 10)
    codes = _dev(_codes(8000, 41), cuda)
    with pytest.raises(OrcaHipError, match="orca_encoder_front_snippet"):
        net.front_snippet(codes, False, 800, 4000, 1, 50, p, 0)                           # skip + count = 51 > 50 pooled positions of the run
    with pytest.raises(OrcaHipError, match="encoder front"):
        net.front_snippet(codes, True, 4800, 4000, 0, 10, p, 0)                           # bases past the sequence
    with pytest.raises(OrcaHipError, match="orca_encoder_front4_snippet"):
        net.front4_snippet(codes, False, 80, 4000, 0, 2, r, 0)                           # base0 off the 400-base grid
    with pytest.raises(OrcaHipError, match="orca_encoder_front4_snippet"):
        net.front4_snippet(codes, False, 0, 4000, 8, 3, r, 0)                            # rows [8, 11) of 10
    with pytest.raises(OrcaHipError, match="orca_encoder_front4_ranges"):
        net.front4_ranges(codes, False, [(0, 5, 0), (15, 6, 10)], r)                      # rows [15, 21) of 20
    with pytest.raises(OrcaHipError, match="orca_encoder_back"):
        net.back(torch.zeros((32, engine.p16_plane_units(49), 4), dtype=torch.float32, device=cuda), 49, torch.zeros((128, 0), device=cuda))
    with pytest.raises(OrcaHipError, match="orca_encoder_back5"):
        net.back5(torch.zeros((15, 128), dtype=torch.float32, device=cuda), torch.zeros((128, 1), device=cuda))
