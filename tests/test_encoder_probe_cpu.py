"""The preconditions of tests/test_gpu_encoder_probe.py, on CPU in fp64: the host pooling it applies to the oracle, the oracle's restart from a
stage's input (`first=k`), and the size of the faults that file exists for - a composed stage-1 group without its exact ends, an N base
expanded as 0, a reverse strand that is not complemented - against the bounds it holds the kernels to."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.encoder_probe_ref import BOUNDS, EDGE, FP32_CLASS, POOLS, PROBE_WEIGHTS, errs, oracle, pool, probe_codes, restart, stage1_faults
from tests.encoder_ref import encoder_sd, rel_err

L_RAGGED, SEED = 4000 * 3 + 777, 61            # no pool divides it: 12 777 -> 3 194 -> 798 -> 159 -> 31 -> 6 -> 3


@pytest.mark.parametrize("w", PROBE_WEIGHTS)
def test_host_pool_is_the_oracles_own_input_to_the_next_stage(w):
    """`pool` (tails dropped) is F.max_pool1d on every stage output of a ragged sequence, for the pool the next stage reads through; and the
    pooled tensor has as many positions as the oracle's next stage - it IS what `oracle.encoder_stages` feeds that stage."""
    ref = oracle(w, L_RAGGED, SEED, False, 7)
    assert [ref[k].shape[0] for k in range(1, 8)] == [12777, 3194, 798, 159, 31, 6, 3]
    sd = encoder_sd(*w)
    for k in range(2, 8):
        p = pool(ref[k - 1], POOLS[k - 1])
        t = F.max_pool1d(torch.from_numpy(np.array(ref[k - 1].T))[None], POOLS[k - 1], POOLS[k - 1])[0].numpy().T
        assert p.shape == t.shape and np.array_equal(p, t), k
        assert p.shape[0] == ref[k].shape[0]
    assert pool(ref[1], 1) is ref[1]


@pytest.mark.parametrize("w", PROBE_WEIGHTS)
@pytest.mark.parametrize("rev", [False, True])
def test_restart_from_a_stage_input(w, rev):
    """`restart`: fed the fp64 stage k - 1 - unpooled, or already pooled as the planar and channel-last pipelines leave it - it gives stage k
    to <= 1e-12; a pool other than the one stage k reads through is refused."""
    ref = oracle(w, L_RAGGED, SEED, rev, 7)
    sd = encoder_sd(*w)
    for k in range(2, 8):
        assert rel_err(restart(sd, ref[k - 1], 1, k), ref[k]) <= 1e-12, k
        assert rel_err(restart(sd, pool(ref[k - 1], POOLS[k - 1]), POOLS[k - 1], k), ref[k]) <= 1e-12, k
    with pytest.raises(ValueError):
        restart(sd, pool(ref[2], 4), 4, 4)


def test_errs_measure():
    """`errs` is `rel_err` over the whole tensor, and the same measure (the whole tensor's scale) over the first and last EDGE rows."""
    rs = np.random.RandomState(3)
    ref = rs.randn(300, 8) * 5
    got = ref.copy()
    got[150, 2] += 1e-3
    got[295, 1] -= 1e-4
    allp, edge = errs(got, ref)
    assert allp == rel_err(got, ref) and abs(edge - 1e-4 / np.abs(ref).max()) < 1e-12
    assert EDGE == 40


@pytest.mark.parametrize("w", PROBE_WEIGHTS)
def test_faults_exceed_the_bounds(w):
    """On the weights and a sequence of the GPU file (L = 16 x 260, N runs, one at position 0): stage 1 in fp64 with (i) the composed 17- and
    25-tap groups WITHOUT their exact ends, (ii) N expanded as 0, (iii) the reverse strand not complemented, against the true stage - unpooled
    (what the f32 pipeline leaves) and MaxPool1d(4)'d (the others) - in `errs`' measure.  (i) must show inside the edge zones, (ii) and (iii)
    anywhere, each by more than 10 x the largest stage-1 bound of the fp32-class modes.
    Measured, unpooled / pooled, the smaller of the two strands (seed 0 | gain 1.6): (i) 0.21 / 0.14 | 0.135 / 0.100, all of it inside the edge
    zones; (ii) 0.25 / 0.23 | 0.27 / 0.27; (iii) 1.47 / 0.99 | 1.19 / 0.92.  The largest fp32-class stage-1 bound is 4.1e-6 (f32)."""
    sd = encoder_sd(*w)
    codes = probe_codes(16 * 260, 260)
    bound = max(BOUNDS[p][1][0] for p in FP32_CLASS)
    assert np.isfinite(bound) and bound < 1e-3
    for rev in (False, True):
        f = stage1_faults(sd, codes, rev)
        assert rel_err(f["true"], oracle(w, 16 * 260, 260, rev, 1)[1]) <= 1e-12
        for k in (1, 4):
            true = pool(f["true"], k)
            allp, edge = errs(pool(f["no_edge_fix"], k), true)
            print(f"{w} rev={rev} pool {k}: no_edge_fix {allp:.3g} (edge {edge:.3g})", end="")
            assert edge > 10 * bound and allp == edge, (k, edge)          # and nowhere but at the ends
            for name in ("n_as_zero", "no_complement")[: 2 if rev else 1]:
                allp, _ = errs(pool(f[name], k), true)
                print(f"  {name} {allp:.3g}", end="")
                assert allp > 10 * bound, (name, k, allp)
            print()
