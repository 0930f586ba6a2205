"""The readouts of the 1 Mb screen are independent: a screen with every readout set gives each of them the bits it gives alone.

The readouts are separate launches on the same final maps and no kernel of the screen uses atomics, so this holds by construction; the test pins
the decomposition into units (orca_amd/screen_readouts.py).  The window, the flank and the items are those of tests/test_gpu_screen_aligned.py
(200 000 bases, 50 bins, synthetic H1esc_1M(synthetic_seed=0)), ``aligned=True``, batches of 4 so that a batch boundary falls inside the item
list.  The loop threshold and the boundary strength are 0.0, so that the lists are not empty on synthetic weights.  Everything is compared bit
for bit; there is no tolerance."""
import dataclasses

import pytest
import torch

from orca_amd import orca_models as M
from orca_amd import screen as S
from tests.test_gpu_screen_aligned import F, REGIONS, _items
from tests.test_gpu_screen_boundaries import same_bits
from tests.test_gpu_screen_sets import _window
from tests.test_screen_indel_cpu import plan_flank

pytestmark = pytest.mark.gpu

READOUTS = {"regions": {"regions": REGIONS}, "insulation": {"insulation": (1, 3, 10)},
            "boundaries": {"insulation": (1, 3, 10), "boundaries": S.BoundaryParams(min_strength=0.0)}, "viewpoints": {"viewpoints": [0, 12, 20, 49]},
            "strata": {"strata": True}, "loops": {"loops": S.LoopParams(threshold=0.0)}}
ALWAYS = ("ref_map", "ref_1d", "delta_profile", "delta_abs_mean", "delta_abs_max", "delta_1d", "maps", "edits", "shift", "bin_map", "aligned_bins",
          "aligned_profile", "aligned_abs_mean", "aligned_abs_max", "strand_gap", "ref_strand_gap")
STATS = {"insulation": ("insulation_widths",), "boundaries": ("insulation_widths", "boundaries"), "viewpoints": ("viewpoints",), "strata": ("strata",),
         "loops": ("loops", "loop_truncated_items"), "regions": ()}


def owner(name):
    """the readout a `ScreenResult` field belongs to, None for the fields every screen has"""
    if name in ALWAYS:
        return None
    bare = name[len("aligned_"):] if name.startswith("aligned_") else name
    bare = bare[len("ref_"):] if bare.startswith("ref_") else bare
    for stem, who in (("region", "regions"), ("insulation", "insulation"), ("bound", "boundaries"), ("viewpoint", "viewpoints"), ("loop", "loops")):
        if stem in bare:
            return who
    if bare in S.STRATA_FIELDS or bare in ("strata_range", "dist_count"):
        return "strata"
    raise AssertionError(f"ScreenResult.{name}: which readout owns it?")


def same(a, b):
    return same_bits(a, b) if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) else type(a) is type(b) and a == b


def alone_equals_together(model, win, items, **kw):
    fields = [f.name for f in dataclasses.fields(S.ScreenResult)]
    st_all = {}
    together = S.screen_1m(model, win, items, stats=st_all, **kw, **{k: v for args in READOUTS.values() for k, v in args.items()})
    for name in fields:
        if name not in ("maps", "ref_1d", "delta_1d", "strand_gap", "ref_strand_gap"):
            assert getattr(together, name) is not None, name
    shared = [k for k in st_all if not any(k in v for v in STATS.values())]
    for who, args in READOUTS.items():
        st = {}
        alone = S.screen_1m(model, win, items, stats=st, **kw, **args)
        mine = (who, "insulation") if who == "boundaries" else (who,)
        for name in fields:
            if owner(name) is None or owner(name) in mine:
                assert same(getattr(alone, name), getattr(together, name)), (who, name)
            else:
                assert getattr(alone, name) is None, (who, name)
        assert set(st) == set(st_all), who
        for k in st:
            assert st[k] == (st_all[k] if k in shared or k in STATS[who] else 0), (who, k, st[k], st_all[k])
    return together, st_all


def test_all_readouts_together_equal_each_one_alone(cuda):
    c = _window()
    items = _items(c)
    model = M.H1esc_1M(synthetic_seed=0).to(cuda)
    win, flank = torch.from_numpy(c).to(cuda), torch.from_numpy(plan_flank(F)).to(cuda)
    res, st = alone_equals_together(model, win, list(items.values()), flank=flank, aligned=True, batch=4)
    assert st["route"] == "two_part" and st["two_part_batches"] == 2 and st["aligned_items"] == 5 and res.strand_gap is None
    assert res.ref_loop_count > 0 and int(res.loop_count.max()) > 0 and int(res.ref_boundary_count.max()) > 0 and int(res.boundary_count.max()) > 0    # the lists hold something
    both, st = alone_equals_together(model, win, [items[k] for k in ("snv", "del4000", "dup8000")], flank=flank, aligned=True, batch=2, strands="both")
    assert st["strands"] == "both" and st["two_part_batches"] == 2 and st["reverse_two_part_items"] == 3 and tuple(both.strand_gap.shape) == (3,)
