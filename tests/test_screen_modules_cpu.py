"""How the screens' modules build on each other: `map_readouts` is a leaf (numpy only), nothing under it reaches back up into `screen` from inside
a function, and every name that moved out of `screen` is still `screen.NAME`."""
import ast
import os
import subprocess
import sys

import pytest

from orca_amd import map_readouts, screen, screen_plan, screen_readouts, sv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MOVED = {
    map_readouts: ("BIN_BP", "STRATA_FIELDS", "LOOP_FIELDS", "BOUNDARY_MATCH_FIELDS", "LoopParams", "BoundaryParams", "check_regions", "check_insulation",
                   "check_viewpoints", "check_strata", "check_loops", "check_boundaries", "check_loops_arg", "check_boundaries_arg", "scores_host",
                   "region_scores_host", "aligned_scores_host", "aligned_region_scores_host", "insulation_host", "insulation_scores_host",
                   "viewpoint_scores_host", "strata_scores_host", "dot_enrichment_host", "dot_calls_host", "follow_loop", "match_loops_host",
                   "loop_scores_host", "boundary_strength_host", "boundary_calls_host", "match_boundaries_host", "boundary_scores_host",
                   "merge_strands_host", "epistasis_scores_host", "_widths", "_loop_params", "_bin_maps", "_follow_loops", "_match_loops",
                   "_match_boundaries", "_boundary_fields"),
    screen_plan: ("ROW_BP", "MARGIN_BP", "PAD_BP", "MIN_SNIPPET_BP", "RUN_MAX_BP", "N_CODE", "KINDS", "LEN_KINDS", "FLANK_BP", "Edit", "EditSet", "members_of",
                  "changes_length", "shift_of", "apply_edit", "saturation_edits", "tile_edits", "pair_edits", "snv_set", "indel", "deletion_scan",
                  "tandem_dup", "bin_map", "BatchPlan", "edit_rows", "edit_snippet", "set_clusters", "entry_rows", "item_pieces", "item_sources",
                  "needed_phases", "mirror_phases", "plan_batch", "mirror_plan", "whole_window_table", "whole_window_piece_tables",
                  "whole_window_set_tables", "epistasis_items", "_plan_indels", "_pieces_meeting"),
    screen_readouts: ("ScreenResult", "EpistasisResult"),
}


def test_map_readouts_is_a_leaf():
    code = "import sys; import orca_amd.map_readouts; bad = [m for m in ('torch', 'orca_amd.engine', 'orca_amd.sv', 'orca_amd.screen') if m in sys.modules]; sys.exit(repr(bad) if bad else 0)"
    got = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert got.returncode == 0, got.stderr


@pytest.mark.parametrize("name", ["sv_readouts", "sv", "scan", "map_readouts", "screen_plan", "screen_readouts"])
def test_no_function_level_import_of_screen(name):
    with open(os.path.join(ROOT, "orca_amd", name + ".py")) as f:
        tree = ast.parse(f.read())
    for fn in ast.walk(tree):
        if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
            for node in ast.walk(fn):
                if isinstance(node, ast.ImportFrom):
                    assert node.module != "screen" and "screen" not in [a.name for a in node.names], (name, fn.name, node.lineno)
                if isinstance(node, ast.Import):
                    assert not any(a.name.endswith(".screen") for a in node.names), (name, fn.name, node.lineno)


def test_screen_reexports_what_moved():
    for module, names in MOVED.items():
        for name in names:
            assert getattr(screen, name) is getattr(module, name), name
    for name in ("_Screen", "_net_of", "_run_screen", "screen_1m", "epistasis_1m"):              # the driver's own
        assert getattr(screen, name).__module__ == "orca_amd.screen", name
    assert sv.STRATA_FIELDS is map_readouts.STRATA_FIELDS


@pytest.mark.parametrize("n", [250, 200_000 // 4000, 1_000_000 // 4000])
def test_unset_arguments_are_none_in_both_spellings(n):
    """`check_loops_arg` / `check_boundaries_arg`: None or False is "unset"; anything else goes through the check.  ``sv``'s spelling is the same
    rule on the levels' 250 bins."""
    lp, bp = map_readouts.LoopParams(w=3, max_calls=7), map_readouts.BoundaryParams(min_strength=0.5, max_calls=5, tol=2)
    for unset in (None, False):
        assert map_readouts.check_loops_arg(unset, n) is None and map_readouts.check_boundaries_arg(unset, n, None) is None
        assert sv.check_loops_arg(unset) is None and sv.check_boundaries_arg(unset) is None
    for arg in (True, lp):
        assert map_readouts.check_loops_arg(arg, n) == map_readouts.check_loops(arg, n)
    for arg in (True, bp):
        assert map_readouts.check_boundaries_arg(arg, n, (5, 10)) == map_readouts.check_boundaries(arg, n)
        with pytest.raises(ValueError, match=r"boundaries: called on the insulation tracks \(insulation=widths\)"):
            map_readouts.check_boundaries_arg(arg, n, None)
    if n == sv.LEVEL_BINS:
        assert sv.check_loops_arg(lp) == map_readouts.check_loops(lp, n) and sv.check_boundaries_arg(bp, (5, 10)) == map_readouts.check_boundaries(bp, n)
        with pytest.raises(ValueError, match="called on the insulation tracks"):
            sv.check_boundaries_arg(True)
    with pytest.raises(ValueError, match="loops: True"):
        map_readouts.check_loops_arg("yes", n)
    with pytest.raises(ValueError, match="boundaries: True"):
        map_readouts.check_boundaries_arg(1, n, (5,))
