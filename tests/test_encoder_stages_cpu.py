"""The Encoder in two parts (sv.s3_plan, sv.Stage3Cache / sv.Stage4Cache) against the REAL network in fp64, on CPU: the oracle's stage
outputs, the dependency cone of a stage-3 / stage-4 position measured by single-base perturbations against the cone derived from the layer
list and against the constants S3_* / S4_*, translation covariance on the 16 / 80-base grids, and the plan's assembly (cache entries pooled,
snippets run on their own) against the pooled stage of the whole assembled window."""
import numpy as np
import pytest
import torch

from oracle import orca_oracle as O
from orca_amd import sv, synth
from tests.encoder_ref import C, WEIGHTS, WINDOWS, chromosome, encoder_sd, pool5, rel_err, stages, strand_codes
from tests.util import golden, maxabs, synth_sd


def test_oracle_stages_match_encoder_run_and_g1():
    """`encoder_stages` in float32 is `encoder_run` bit for bit at stage 7; in float64 it stays within G1's tolerance (2e-5) of the
    reference's own output (G1 y_single: one 148 kb block)."""
    sd = synth_sd("Encoder", 0)
    x = torch.from_numpy(synth.synth_sequence(4000 * 12, seed=5, n_frac=0.01)).transpose(1, 2)
    outs = O.encoder_stages(sd, x)
    assert len(outs) == 7 and torch.equal(outs[-1], O.encoder_run(sd, x))
    assert [o.shape[2] for o in outs] == [48000, 12000, 3000, 600, 120, 24, 12] and outs[0].dtype == torch.float32
    assert [o.shape[2] for o in O.encoder_stages(sd, x, upto=3)] == [48000, 12000, 3000]
    x2 = torch.from_numpy(synth.synth_sequence(4000 * 37, seed=12)).transpose(1, 2)
    y64 = O.encoder_stages(sd, x2, dtype=torch.float64)[-1]
    assert y64.dtype == torch.float64
    assert maxabs(y64[0].numpy(), golden("G1_encoder.npz")["y_single"]) < 2e-5


# ---- a. reach and covariance ---------------------------------------------------------------------------------------------------------------
def cone(level):
    """Bases [lo, hi] (relative to the first base of the cell) a stage-``level`` position depends on, from the layer list
    (orca_modules.py:811-927).  Every stage is 4 convs of kernel 9 (padding 4): +-16 positions of its own grid.  A stage-1 position is one
    base, a stage-2 position 4 (MaxPool1d(4)), stage 3 16, stage 4 80 (MaxPool1d(5)).  Backwards from a stage-3 position j (bases 16 j ..
    16 j + 15): stage-3 input positions j - 16 .. j + 16 -> stage-2 positions 4 (j - 16) .. 4 (j + 16) + 3 -> with stage 2's convs 4 j - 80 ..
    4 j + 83 -> stage-1 positions 16 j - 320 .. 16 j + 335 -> with stage 1's convs bases 16 j - 336 .. 16 j + 351: [-336, +351], i.e. 336
    bases either side of the cell.  A stage-4 position k (bases 80 k .. 80 k + 79): stage-4 input positions k - 16 .. k + 16 -> stage-3
    positions 5 (k - 16) .. 5 (k + 16) + 4 -> bases 80 k - 1 280 - 336 .. 80 k + 1 344 + 351: [-1 616, +1 695], 1 616 either side."""
    if level == 3:
        return -16 * 16 - 64 - 16, 16 * 16 + 64 + 15 + 16
    return -16 * 80 - 336, 16 * 80 + 4 * 16 + 351


@pytest.mark.parametrize("seed,gain", WEIGHTS)
@pytest.mark.parametrize("level", [3, 4])
def test_reach_of_a_position_is_the_analytic_cone(level, seed, gain):
    """Single-base perturbations (every other base and N) around both ends of the analytic cone of one stage-3 / stage-4 position of a
    random sequence: the bases that change it (any of its 128 channels) are exactly [lo, hi] of `cone` - and the constants the plan uses
    cover it: S3_MARGIN_BP / S4_MARGIN_BP >= the reach either side of the cell, the pads >= the margins."""
    sd = encoder_sd(seed, gain)
    grid = 16 if level == 3 else 80
    L, j = (1280, 40) if level == 3 else (4000, 25)
    lo, hi = cone(level)
    rs = np.random.RandomState(100 + seed)
    base = rs.randint(0, 4, L).astype(np.uint8)
    base[j * grid + 100: j * grid + 140] = 4                        # an N run inside the cone
    probe = [b for e in (lo, hi) for b in range(j * grid + e - 4, j * grid + e + 5)]
    seqs, where = [base], []
    for b in probe:
        for alt in range(5):
            if alt != base[b]:
                s = base.copy()
                s[b] = alt
                seqs.append(s)
                where.append(b)
    out = stages(sd, np.stack(seqs), level)[level][:, j, :]
    changed = sorted({b for b, o in zip(where, out[1:]) if np.abs(o - out[0]).max() > 0})
    inside = [b - j * grid for b in changed]
    assert inside[0] == lo and inside[-1] == hi, (inside[0], inside[-1])
    assert all(b in changed for b in probe if lo <= b - j * grid <= hi)
    reach = max(-lo, hi - (grid - 1))
    assert reach == (336 if level == 3 else 1616)
    margin, pad = (sv.S3_MARGIN_BP, sv.S3_PAD_BP) if level == 3 else (sv.S4_MARGIN_BP, sv.S4_PAD_BP)
    assert reach <= margin <= pad and margin % grid == 0 and pad % (5 * grid) == 0


@pytest.mark.parametrize("seed,gain", WEIGHTS)
@pytest.mark.parametrize("level", [3, 4])
def test_translation_covariance(level, seed, gain):
    """Shifting the bases by one cell (16 / 80) shifts stage 3 / 4 by one position wherever the cone lies inside both sequences: <= 1e-12."""
    sd = encoder_sd(seed, gain)
    grid = 16 if level == 3 else 80
    L = 2400 if level == 3 else 8000
    rs = np.random.RandomState(200 + seed)
    codes = rs.randint(0, 4, L).astype(np.uint8)
    codes[700: 760] = 4
    a = stages(sd, codes, level)[level]
    b = stages(sd, codes[grid:], level)[level]
    lo, hi = cone(level)
    j0, j1 = -(-(-lo) // grid), (L - grid - hi) // grid              # positions of b whose cone is inside b (and, one up, inside a)
    assert j1 - j0 > 20
    assert rel_err(b[j0: j1], a[j0 + 1: j1 + 1]) <= 1e-12
    assert np.abs(a).max() > 1.0


# ---- b. the plan on the real network -------------------------------------------------------------------------------------------------------
LEVELS = {3: dict(), 4: dict(margin=sv.S4_MARGIN_BP, grid=sv.S4_GRID, pad=sv.S4_PAD_BP, min_snippet=sv.S4_MIN_SNIPPET_BP)}


class _CacheEmulation:
    """What sv.Stage3Cache / Stage4Cache hold, from the fp64 oracle: entry (strand, phase) of a region = the stage on the strand's bases from
    e0 (the first strand coordinate >= the region's start with e0 % grid == phase, `Stage3Cache._origin`) to the region's end, zero padded
    at both (as the cache's own front run is)."""

    def __init__(self, sd, codes, level):
        self.sd, self.codes, self.level = sd, codes, level
        self.grid = 16 if level == 3 else 80
        self.entries = {}

    def origin(self, strand, phase, region):
        lo = region[0] if strand == "+" else C - region[1]
        return lo + (phase - lo) % self.grid

    def get(self, strand, phase, region):
        key = (strand, phase, region)
        if key not in self.entries:
            hi = region[1] if strand == "+" else C - region[0]
            e0 = self.origin(strand, phase, region)
            n = (hi - e0) // self.grid * self.grid
            self.entries[key] = stages(self.sd, strand_codes(self.codes, strand == "-")[e0: e0 + n], self.level)[self.level]
        return self.entries[key]


def assemble(sd, emu, codes_w, pcs, region):
    """The stage-4 (resp. stage-5) input of a window strand the way sv.s3_encode / sv._s4_encode assemble it, in fp64: [n, 128] and the
    coverage count of every pooled position."""
    level, grid = emu.level, emu.grid
    L = len(codes_w)
    takes, snippets = sv.s3_plan(pcs, C, L, regions=region, **LEVELS[level])
    n = L // (5 * grid)
    got, cov = np.full((n, 128), np.nan), np.zeros(n, int)
    for m_lo, m_hi, _, strand, phase, c in takes:
        e = emu.get(strand, phase, region or (0, C))
        j0 = (c - emu.origin(strand, phase, region or (0, C))) // grid
        assert phase == c % grid and j0 >= 0 and j0 + 5 * (m_hi - m_lo) <= len(e)
        got[m_lo: m_hi] = pool5(e[j0: j0 + 5 * (m_hi - m_lo)])
        cov[m_lo: m_hi] += 1
    for ga, gb, b0, nb, skip in snippets:
        got[ga: gb] = pool5(stages(sd, codes_w[b0: b0 + nb], level)[level])[skip: skip + gb - ga]
        cov[ga: gb] += 1
    if level == 4 and len(snippets) > 1 and snippets[0][0] == 0 and snippets[-1][1] == n:
        # sv._s4_encode's ONE front run over the strand's snippets concatenated (the window's ends first and last)
        cat = pool5(stages(sd, np.concatenate([codes_w[b0: b0 + nb] for _, _, b0, nb, _ in snippets]), level)[level])
        off = 0
        for ga, gb, b0, nb, skip in snippets:
            assert rel_err(cat[off // (5 * grid) + skip: off // (5 * grid) + skip + gb - ga], got[ga: gb]) <= 1e-10
            off += nb
    return got, cov, takes


@pytest.mark.parametrize("level", [3, 4])
def test_stage_plan_is_exact_on_the_real_network(level):
    """`sv.s3_plan` with the Stage3Cache (level 3) / Stage4Cache (level 4) parameters on a 64 kb synthetic chromosome with N runs, real
    synthetic Encoder weights in fp64: cache entries of the strand and phase the plan names (whole chromosome, and a region of it), pooled
    from the plan's offset, plus snippets run through the front on their own, against the pooled stage of the whole assembled window -
    every position of every window, both strands, <= 1e-10 relative.  The windows cover a deletion, a duplication, an inversion, pieces at
    both chromosome ends, 4 - 48 kb, and windows partly outside the cached region."""
    codes = chromosome()
    for wi, (pieces, region) in enumerate(WINDOWS):
        seed, gain = WEIGHTS[wi % len(WEIGHTS)]
        sd = encoder_sd(seed, gain)
        emu = _CacheEmulation(sd, codes, level)
        L = sum(p[1] for p in pieces)
        assert L % 400 == 0
        fw = sv.assemble_codes(codes, pieces)
        for rev in (False, True):
            pcs = sv.revcomp_pieces(pieces) if rev else pieces
            codes_w = strand_codes(fw, rev)
            assert np.array_equal(codes_w, sv.assemble_codes(codes, pcs))
            ref = pool5(stages(sd, codes_w, level)[level])
            got, cov, takes = assemble(sd, emu, codes_w, pcs, region)
            assert (cov == 1).all(), (pieces, rev)
            assert L < 12_000 or takes, (pieces, rev)                     # the cache serves the windows that are not all ends and junctions
            err = rel_err(got, ref)
            assert err <= 1e-10, (pieces, region, rev, err)
