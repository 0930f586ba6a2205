"""Domain boundary calls per level of the SV screen on the MI355X (orca_screen_boundary_calls; sv.sv_screen(..., scores=True, insulation=,
boundaries=), sv.sv_scores): one model and the first three variants of tests/test_gpu_sv_incremental.py - a deletion, a duplication and an
inversion (synthetic H1esc(synthetic_seed=0)).  Every boundary field of an entry equals `sv.paired_boundary_scores_host` on the entry's own
``insulation``, ``ref_insulation``, ``insulation_delta`` and ``bin_map`` EXACTLY (comparisons and one fp32 subtraction: integers equal, floats bit
for bit, NaN in the same slots), with the maps kept or not, and through `sv_scores` on the kept output dicts; unset, an entry keeps its keys and
bits.  The kernel alone is held to its restatement in tests/test_gpu_screen_boundaries.py."""
import numpy as np
import pytest
import torch

from orca_amd import orca_models, sv
from orca_amd import screen as S
from tests.test_gpu_sv_incremental import CHR, VARIANTS
from tests.test_gpu_sv_scores import FIELDS as OLD_FIELDS
from tests.test_gpu_sv_scores import scores_same_bits

pytestmark = pytest.mark.gpu

THREE = VARIANTS[:3]                                                        # a deletion, a duplication, an inversion
WIDTHS = (5, 10)
Q = S.BoundaryParams(0.0, 24, 1)                                            # min_strength 0: every list as full as it gets
INS = ("insulation", "ref_insulation", "insulation_delta")
TOP_KEYS = ["bin_map", "boundary_params", "count", "insulation_widths", "junction_bins", "models"]


def same(x, y):
    """equal arrays: shape, dtype, and every value - floats bit for bit up to the NaN's payload"""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    if x.dtype.kind == "f":
        return bool(np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[~np.isnan(x)].view(np.uint32), y[~np.isnan(y)].view(np.uint32)))
    return bool(np.array_equal(x, y))


def boundaries_same(x, y):
    return (sorted(x) == sorted(y) and x["boundary_params"] == y["boundary_params"] and scores_same_bits(x, y)
            and all(sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in INS + sv.BOUNDARY_SCORE_FIELDS) for a, b in zip(x["models"], y["models"])))


@pytest.fixture(scope="module")
def case(cuda):
    g = torch.Generator(device=cuda).manual_seed(11)
    genome = torch.randint(0, 4, (CHR,), device=cuda, generator=g, dtype=torch.uint8)
    genome[7_000_000:7_003_000] = 4                                     # an N run inside the windows
    model = orca_models.H1esc(synthetic_seed=0)
    called = sv.sv_screen([model], genome, THREE, CHR, min_uses=1, scores=True, insulation=WIDTHS, boundaries=Q)
    return model, genome, called


def equals_host(scores, what):
    """an entry's boundary fields against the restatement on the entry's own tracks and bin maps"""
    assert sorted(scores) == TOP_KEYS and scores["boundary_params"] == Q
    bm = scores["bin_map"]
    K, W = Q.max_calls, len(WIDTHS)
    for m, got in enumerate(scores["models"]):
        assert sorted(got) == sorted(OLD_FIELDS + INS + sv.BOUNDARY_SCORE_FIELDS)
        C = got["insulation"].shape[1]
        flat = lambda a: a.reshape((6 * C,) + a.shape[2:])
        want = sv.paired_boundary_scores_host(flat(got["insulation"]), flat(got["ref_insulation"]), flat(got["insulation_delta"]), np.repeat(bm, C, axis=0), Q)
        for k in sv.BOUNDARY_SCORE_FIELDS:
            shape = (6, C, W) if k.endswith("_count") or k in ("boundaries_gained", "boundaries_lost") else (6, C, W, K)
            assert got[k].shape == shape, (what, m, k, got[k].shape)
            assert same(flat(got[k]), want[k]), (what, m, k)


def test_screen_boundary_fields_equal_the_host_restatement(case):
    """Printed, not asserted (the weights are synthetic): per level, how many reference boundaries (w = 5) each variant keeps, loses and leaves
    unmapped, and how many it gains."""
    model, genome, called = case
    for i, v in enumerate(THREE):
        e = called[i]
        assert sorted(e) == ["alt", "ref", "scores", "sv"] and e["sv"] == v
        equals_host(e["scores"], v)
        got = e["scores"]["models"][0]
        assert got["ref_boundaries"].dtype == np.int32 and got["boundary_strength"].dtype == np.float32 and got["ref_boundary_is_lost"].dtype == bool
        assert int(got["ref_boundary_count"].min()) >= 1
        kept = (got["boundary_followed_at"] >= 0).sum(axis=-1)
        print(v, "w = 5, per level: reference boundaries", got["ref_boundary_count"][:, 0, 0].tolist(), "kept", kept[:, 0, 0].tolist(), "lost",
              got["boundaries_lost"][:, 0, 0].tolist(), "unmapped", got["ref_boundary_is_unmapped"].sum(axis=-1)[:, 0, 0].tolist(), "gained",
              got["boundaries_gained"][:, 0, 0].tolist())
    # the deletion's finest level shares no locus with its reference window: every listed boundary there is unmapped, none lost or gained
    d = called[0]["scores"]
    assert (d["count"][5] == 0) and not d["models"][0]["ref_boundary_is_lost"][5].any() and not d["models"][0]["boundary_is_gained"][5].any()
    assert (d["models"][0]["ref_boundary_is_unmapped"][5] == (d["models"][0]["ref_boundaries"][5] >= 0)).all()
    # the inversion's maps do descend, and its boundaries are followed through them
    inv = called[2]["scores"]
    assert any((np.diff(inv["bin_map"][k][inv["bin_map"][k] >= 0]) < 0).any() for k in range(6))


def test_maps_can_stay_on_the_device_and_sv_scores_gives_the_same_dict(case, cuda):
    model, genome, called = case
    bare = sv.sv_screen([model], genome, THREE, CHR, min_uses=1, scores=True, keep_maps=False, insulation=WIDTHS, boundaries=Q)
    for i, v in enumerate(THREE):
        assert bare[i]["alt"]["predictions"] is None and bare[i]["ref"]["predictions"] is None
        assert boundaries_same(bare[i]["scores"], called[i]["scores"]), i
        again = sv.sv_scores(v, called[i]["ref"], called[i]["alt"], CHR, cuda, insulation=WIDTHS, boundaries=Q)
        assert boundaries_same(again, called[i]["scores"]), i


def test_boundaries_change_nothing_else(case, cuda):
    model, genome, called = case
    plain = sv.sv_screen([model], genome, THREE, CHR, min_uses=1, scores=True, insulation=WIDTHS)
    for i in range(3):
        s = plain[i]["scores"]
        assert sorted(s) == [k for k in TOP_KEYS if k != "boundary_params"] and sorted(s["models"][0]) == sorted(OLD_FIELDS + INS)
        assert scores_same_bits(s, called[i]["scores"]) and all(same(s["models"][0][k], called[i]["scores"]["models"][0][k]) for k in INS)
        for allele in ("ref", "alt"):
            for j in range(6):
                assert np.array_equal(plain[i][allele]["predictions"][0][j], called[i][allele]["predictions"][0][j]), (i, allele, j)
    off = sv.sv_scores(THREE[0], called[0]["ref"], called[0]["alt"], CHR, cuda, insulation=WIDTHS, boundaries=False)
    assert sorted(off) == sorted(plain[0]["scores"]) and sorted(off["models"][0]) == sorted(OLD_FIELDS + INS)
    defaults = sv.sv_scores(THREE[1], called[1]["ref"], called[1]["alt"], CHR, cuda, insulation=WIDTHS, boundaries=True)
    assert defaults["boundary_params"] == S.check_boundaries(True, 250) and defaults["models"][0]["boundaries"].shape[-1] == 32
    with pytest.raises(ValueError, match="insulation"):
        sv.sv_screen([model], genome, THREE[:1], CHR, scores=True, boundaries=True)
    with pytest.raises(ValueError, match="scores"):
        sv.sv_screen([model], genome, THREE[:1], CHR, insulation=WIDTHS, boundaries=True)
    with pytest.raises(ValueError, match="insulation"):
        sv.sv_scores(THREE[0], called[0]["ref"], called[0]["alt"], CHR, cuda, boundaries=True)
