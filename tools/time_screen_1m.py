"""Edits per second of the 1 Mb mutagenesis screen (orca_amd/screen.py) against the naive route, in one process, alternated.

Workload: synthetic H1esc_1M on one 1 Mb window (random bases with N runs); the 3 000 saturation SNVs of 1 kb in its middle plus the 250 4 kb
mask tiles of the whole window (3 250 edits).
  screen  screen.screen_1m(model, window, edits, batch=B)
  naive   per batch of B edits: the edited windows (one orca_screen_edit_codes launch), Net's Encoder on them (forward_codes, whole 1 Mb each),
          Decoder_1m + the 1-D head on the batch, the same scores - what a user without the screen would run
Both routes' maps are compared on the first 64 edits (2e-5).  JSON on stdout and in profiles/screen_1m.json.

    python tools/time_screen_1m.py                          # B = 16 and 64, 2 alternated repetitions
    python tools/time_screen_1m.py --screen-only --batches 64 --reps 1 --out ''     # what a profiler run wraps
    python tools/time_screen_1m.py --pairs 50 --haplotype 400 --batches 64          # compound edits, into profiles/screen_1m_sets.json

Compound edits (screen.EditSet), items per second against the same edited windows through model.net:
  --pairs N      every pair of N 4 kb mask tiles of bases [100 000, ..) with N of bases [600 000, ..): N x N sets of two members
  --haplotype M  --haplotypes H sets (64 by default) of M SNVs each, drawn uniformly from --haplotype-span bases in the window's middle

Insertions and deletions, into profiles/screen_1m_indels.json:
  --indels N     N random indels of 1-50 bases (half deletions, half insertions, anywhere in the window, 8 000 bases of right flank) at B = 64,
                 against the same alt windows through model.net and against N SNVs at the same positions through the screen, in the same run

Aligned scores, into profiles/screen_1m_aligned.json:
  --aligned      the 3 250-edit workload above through screen_1m with aligned=True and with aligned=False, alternated in the same run (B from
                 --batches): what the bin maps and the aligned-score kernels add

Both strands, into profiles/screen_1m_strands.json:
  --strands both the 3 250-edit workload at B = 64 through screen_1m with strands="both", and alternated in the same run with strands="+" and the
                 naive both-strand route (the edited windows through Net on both strands, merged by orca_screen_merge_strands, the same scores)

Tracks, into profiles/screen_1m_tracks.json:
  --tracks       the 3 250-edit workload at B = 64 through screen_1m with insulation=(5, 10, 25), viewpoints=[125] and without, alternated in the same
                 run; with --aligned also aligned=True with and without the tracks: what the two track kernels add, set beside what aligned=True adds

Distance strata, into profiles/screen_1m_strata.json:
  --strata       the 3 250-edit workload at B = 64 through screen_1m with strata=True and without, and both again with aligned=True, alternated in
                 the same run, best of three: what orca_screen_strata_scores adds, set beside what aligned=True adds

Loops, into profiles/screen_1m_loops.json:
  --loops        the 3 250-edit workload at B = 64 through screen_1m with loops=True, with the lists filled (threshold 0.0) and without, and both again with aligned=True, alternated in
                 the same run, best of three: what the dot-call kernels and the host matching add, set beside what aligned=True adds

Boundaries, into profiles/screen_1m_boundaries.json:
  --boundaries   the 3 250-edit workload at B = 64 through screen_1m with insulation=(5, 10, 25), with the same plus boundaries=True and plus
                 boundaries=BoundaryParams(min_strength=0.0) (every list as full as it gets), alternated in the same run, best of three: what
                 orca_screen_boundary_calls and the host matching add to the insulation tracks, beside the spread of that baseline's repetitions

Non-additivity, into profiles/screen_1m_epistasis.json:
  --epistasis NA NB  the NA x NB pairs of 4 kb mask tiles (NA from base 100 000, NB from base 600 000) at B = 64 through screen.epistasis_1m, and
                 through today's route - screen_1m on the singles and on the pairs with keep_maps=True, then the residual in torch, in fp32 -
                 alternated in the same run, best of three; also the largest |fp32-route residual - fp64 residual| seen on the same maps
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from orca_amd import engine
from orca_amd import orca_models as M
from orca_amd import screen as S

L = 1_000_000


def window(seed=5):
    rs = np.random.RandomState(seed)
    c = rs.randint(0, 4, L).astype(np.uint8)
    for a in rs.randint(0, L - 2000, 12):
        c[a: a + rs.randint(50, 2000)] = 4
    return c


def naive(model, win, edits, batch, keep_maps=False, flank=None):
    net = model.net
    sc = S._Screen(net, win, {}, flank)
    ref_map, _ = sc.whole([])
    ref_map = ref_map[0].contiguous()
    out, maps_all = [], []
    with torch.no_grad():
        for i0 in range(0, len(edits), batch):
            maps, h = sc.whole(edits[i0: i0 + batch])
            out.append(engine.screen_scores(sc.ctx, maps, ref_map)[1])
            if keep_maps:
                maps_all.append(maps.clone())
    return torch.cat(out), (torch.cat(maps_all) if keep_maps else None)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def time_sets(a, model, win, c, dev):
    """The --pairs / --haplotype workloads: items/s of the screen and of the naive route, alternated, per batch size."""
    rep = {"device": torch.cuda.get_device_name(dev)}
    work = {}
    if a.pairs:
        ta = S.tile_edits("mask", 4000, 4000, 100_000, 100_000 + 4000 * a.pairs)
        tb = S.tile_edits("mask", 4000, 4000, 600_000, 600_000 + 4000 * a.pairs)
        work[f"pairs_{a.pairs}x{a.pairs}_mask_4kb"] = S.pair_edits(ta, tb)[0]
    if a.haplotype:
        rs = np.random.RandomState(17)
        lo = (L - a.haplotype_span) // 2
        sets = []
        for _ in range(a.haplotypes):
            pos = lo + np.sort(rs.choice(a.haplotype_span, a.haplotype, replace=False))
            sets.append(S.snv_set(c, [(int(p), int(c[p]), (int(c[p]) + 1 + int(p) % 3) % 4 if c[p] < 4 else int(p) % 4) for p in pos]))
        work[f"haplotype_{a.haplotype}_snvs_in_{a.haplotype_span}_bp"] = sets
    for name, items in work.items():
        st = {}
        rs_ = S.screen_1m(model, win, items[:64], batch=64, keep_maps=True, stats=st)            # warm-up and cross-check
        row = {"items": len(items), "route": st["route"], "segments_per_item": round(st["segments"] / max(1, len(items[:64])), 2),
               "front_bases_per_item": round(st["front_bases"] / max(1, len(items[:64])))}
        if not a.screen_only:
            _, mn = naive(model, win, items[:64], 64, keep_maps=True)
            row["maps_maxabs_screen_vs_naive"] = float((rs_.maps - mn).abs().max())
            assert row["maps_maxabs_screen_vs_naive"] < 2e-5, row
        del rs_
        for B in [int(b) for b in a.batches.split(",")]:
            ts, tn = [], []
            for _ in range(a.reps):
                ts.append(timed(lambda: S.screen_1m(model, win, items, batch=B))[0])
                if not a.screen_only:
                    tn.append(timed(lambda: naive(model, win, items, B))[0])
            r = {"screen_s": [round(t, 3) for t in ts], "screen_items_per_s": round(len(items) / min(ts), 1)}
            if tn:
                r.update({"naive_s": [round(t, 3) for t in tn], "naive_items_per_s": round(len(items) / min(tn), 1), "speedup": round(min(tn) / min(ts), 2)})
            row[f"B{B}"] = r
        rep[name] = row
        print(json.dumps({name: row}), flush=True)
    return rep


def time_indels(a, model, win, c, dev):
    """The --indels workload: items/s of the screen on N random indels, of the naive route on the same alt windows and of the screen on N SNVs
    at the same positions, alternated, at B = 64."""
    rs = np.random.RandomState(23)
    flank = torch.from_numpy(rs.randint(0, 4, S.FLANK_BP).astype(np.uint8)).to(dev)
    pos = rs.randint(1, L - 50, a.indels)
    size = rs.randint(1, 51, a.indels)
    items = [S.Edit("del", int(p), int(n)) if k % 2 == 0 else S.Edit("ins", int(p), rs.randint(0, 4, int(n))) for k, (p, n) in enumerate(zip(pos, size))]
    snvs = [S.Edit("sub", int(p), 1, [(int(c[p]) + 1) % 4]) for p in pos]
    B = 64
    st = {}
    rs_ = S.screen_1m(model, win, items[:B], batch=B, keep_maps=True, stats=st, flank=flank)               # warm-up and cross-check
    S.screen_1m(model, win, snvs[:B], batch=B)
    row = {"items": len(items), "batch": B, "flank": S.FLANK_BP, "route": st["route"], "segments_per_item": round(st["segments"] / B, 2),
           "front_bases_per_item": round(st["front_bases"] / B), "take_rows_per_item": round(st["take_rows"] / B), "cache_phases": st["cache_phases"]}
    _, mn = naive(model, win, items[:B], B, keep_maps=True, flank=flank)
    row["maps_maxabs_screen_vs_naive"] = float((rs_.maps - mn).abs().max())
    del rs_, mn
    ti, tn, tsub = [], [], []
    for _ in range(a.reps):
        st = {}
        ti.append(timed(lambda: S.screen_1m(model, win, items, batch=B, stats=st, flank=flank))[0])
        tn.append(timed(lambda: naive(model, win, items, B, flank=flank))[0])
        tsub.append(timed(lambda: S.screen_1m(model, win, snvs, batch=B))[0])
    row.update({"cache_phases_full_run": st["cache_phases"], "screen_s": [round(t, 3) for t in ti], "naive_s": [round(t, 3) for t in tn],
                "snv_screen_s": [round(t, 3) for t in tsub], "screen_items_per_s": round(len(items) / min(ti), 1),
                "naive_items_per_s": round(len(items) / min(tn), 1), "snv_screen_items_per_s": round(len(items) / min(tsub), 1),
                "speedup_over_naive": round(min(tn) / min(ti), 2), "cost_over_snv_screen": round(min(ti) / min(tsub), 2)})
    print(json.dumps({"indels": row}), flush=True)
    return {"device": torch.cuda.get_device_name(dev), f"indels_{a.indels}_of_1_to_50_bp": row}


def time_aligned(a, model, win, edits, dev):
    """The --aligned workload: screen_1m on the same edits with and without aligned=True, alternated, per batch size."""
    rep = {"device": torch.cuda.get_device_name(dev), "edits": len(edits)}
    st = {}
    S.screen_1m(model, win, edits[:64], batch=64, stats=st, aligned=True)                     # warm-up
    S.screen_1m(model, win, edits[:64], batch=64)
    rep["route"] = st["route"]
    for B in [int(b) for b in a.batches.split(",")]:
        ta, tp = [], []
        for _ in range(a.reps):
            tp.append(timed(lambda: S.screen_1m(model, win, edits, batch=B))[0])
            ta.append(timed(lambda: S.screen_1m(model, win, edits, batch=B, aligned=True))[0])
        rep[f"B{B}"] = {"plain_s": [round(t, 3) for t in tp], "aligned_s": [round(t, 3) for t in ta], "plain_edits_per_s": round(len(edits) / min(tp), 1),
                        "aligned_edits_per_s": round(len(edits) / min(ta), 1), "aligned_over_plain": round(min(ta) / min(tp), 4)}
        print(json.dumps({f"B{B}": rep[f"B{B}"]}), flush=True)
    return rep


TRACKS = {"insulation": (5, 10, 25), "viewpoints": [125]}


def time_tracks(a, model, win, edits, dev):
    """The --tracks workload: screen_1m on the same edits with and without the insulation tracks and the viewpoint profile, alternated, at B = 64;
    with --aligned also both with aligned=True.  The overheads are over the plain screen of the same run."""
    B = 64
    rep = {"device": torch.cuda.get_device_name(dev), "edits": len(edits), "batch": B, "insulation": list(TRACKS["insulation"]), "viewpoints": TRACKS["viewpoints"]}
    runs = {"plain": {}, "tracks": dict(TRACKS)}
    if a.aligned:
        runs.update({"aligned": {"aligned": True}, "aligned_tracks": dict(TRACKS, aligned=True)})
    st = {}
    for kw in runs.values():                                                                     # warm-up
        S.screen_1m(model, win, edits[:B], batch=B, stats=st, **kw)
    rep["route"] = st["route"]
    t = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, kw in runs.items():
            t[k].append(timed(lambda: S.screen_1m(model, win, edits, batch=B, **kw))[0])
    for k in runs:
        rep[f"{k}_s"] = [round(x, 3) for x in t[k]]
        rep[f"{k}_edits_per_s"] = round(len(edits) / min(t[k]), 1)
    plain = min(t["plain"])
    rep["tracks_over_plain"] = round(min(t["tracks"]) / plain, 4)
    if a.aligned:
        rep["aligned_over_plain"] = round(min(t["aligned"]) / plain, 4)
        rep["aligned_tracks_over_aligned"] = round(min(t["aligned_tracks"]) / min(t["aligned"]), 4)
        over = min(t["aligned"]) - plain
        rep["tracks_overhead_over_aligned_overhead"] = round((min(t["tracks"]) - plain) / over, 2) if over > 0 else None
    return rep


def time_strata(a, model, win, edits, dev):
    """The --strata workload: screen_1m on the same edits with and without strata=True, plain and with aligned=True, alternated, at B = 64, best of
    max(--reps, 3).  The overheads are over the plain screen of the same run."""
    B, reps = 64, max(a.reps, 3)
    rep = {"device": torch.cuda.get_device_name(dev), "edits": len(edits), "batch": B, "reps": reps}
    runs = {"plain": {}, "strata": {"strata": True}, "aligned": {"aligned": True}, "aligned_strata": {"aligned": True, "strata": True}}
    st = {}
    for kw in runs.values():                                                                     # warm-up
        S.screen_1m(model, win, edits[:B], batch=B, stats=st, **kw)
    rep["route"] = st["route"]
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, kw in runs.items():
            t[k].append(timed(lambda: S.screen_1m(model, win, edits, batch=B, **kw))[0])
    for k in runs:
        rep[f"{k}_s"] = [round(x, 3) for x in t[k]]
        rep[f"{k}_edits_per_s"] = round(len(edits) / min(t[k]), 1)
    plain = min(t["plain"])
    rep["strata_over_plain"] = round(min(t["strata"]) / plain, 4)
    rep["aligned_over_plain"] = round(min(t["aligned"]) / plain, 4)
    rep["aligned_strata_over_aligned"] = round(min(t["aligned_strata"]) / min(t["aligned"]), 4)
    rep["plain_spread"] = round(max(t["plain"]) / plain, 4)
    return rep


def time_loops(a, model, win, edits, dev):
    """The --loops workload: screen_1m on the same edits with and without loops=True, plain and with aligned=True, alternated, at B = 64, best of
    max(--reps, 3).  The overheads are over the plain screen of the same run.  The default threshold, 0.25, is not calibrated, and on these synthetic
    weights (enrichments near 0.03) it calls nothing: the kernels run in full but the lists stay empty and the host matching idles.  So the same is
    timed once more with the default parameters at threshold 0.0 (``*_full``), which fills every list; ``ref_loop_count_*`` and the largest
    ``loop_count`` of the first batch say how many dots there were."""
    B, reps = 64, max(a.reps, 3)
    rep = {"device": torch.cuda.get_device_name(dev), "edits": len(edits), "batch": B, "reps": reps, "full_threshold": 0.0}
    full = S.LoopParams(threshold=0.0)
    runs = {"plain": {}, "loops": {"loops": True}, "loops_full": {"loops": full}, "aligned": {"aligned": True},
            "aligned_loops": {"aligned": True, "loops": True}, "aligned_loops_full": {"aligned": True, "loops": full}}
    st = {}
    for k, kw in runs.items():                                                                   # warm-up
        res = S.screen_1m(model, win, edits[:B], batch=B, stats=st, **kw)
        if k in ("loops", "loops_full"):
            rep[f"ref_loop_count_{k}"], rep[f"max_loop_count_first_batch_{k}"] = res.ref_loop_count, int(res.loop_count.max())
    rep["route"] = st["route"]
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, kw in runs.items():
            t[k].append(timed(lambda: S.screen_1m(model, win, edits, batch=B, **kw))[0])
    for k in runs:
        rep[f"{k}_s"] = [round(x, 3) for x in t[k]]
        rep[f"{k}_edits_per_s"] = round(len(edits) / min(t[k]), 1)
    plain = min(t["plain"])
    rep["loops_over_plain"] = round(min(t["loops"]) / plain, 4)
    rep["loops_full_over_plain"] = round(min(t["loops_full"]) / plain, 4)
    rep["aligned_over_plain"] = round(min(t["aligned"]) / plain, 4)
    rep["aligned_loops_over_aligned"] = round(min(t["aligned_loops"]) / min(t["aligned"]), 4)
    rep["aligned_loops_full_over_aligned"] = round(min(t["aligned_loops_full"]) / min(t["aligned"]), 4)
    rep["plain_spread"] = round(max(t["plain"]) / plain, 4)
    return rep


def time_boundaries(a, model, win, edits, dev):
    """The --boundaries workload: screen_1m on the same edits with insulation=(5, 10, 25) alone, with boundaries=True on top and with
    boundaries=BoundaryParams(min_strength=0.0), which lists every minimum with a positive strength, alternated, at B = 64, best of max(--reps, 3).
    The added time is against the insulation-only repetition beside it and against the best of three, with the spread of the baseline's repetitions;
    ``ref_boundary_count_*`` and the largest ``boundary_count`` of the first batch say how many boundaries there were (the weights are synthetic and
    the default min_strength is not calibrated)."""
    B, reps = 64, max(a.reps, 3)
    ins = {"insulation": (5, 10, 25)}
    rep = {"device": torch.cuda.get_device_name(dev), "edits": len(edits), "batch": B, "reps": reps, "insulation": list(ins["insulation"]), "weights": "synthetic"}
    runs = {"insulation": ins, "boundaries": dict(ins, boundaries=True), "boundaries_filled": dict(ins, boundaries=S.BoundaryParams(min_strength=0.0))}
    st = {}
    for k, kw in runs.items():                                                                   # warm-up
        res = S.screen_1m(model, win, edits[:B], batch=B, stats=st, **kw)
        if k != "insulation":
            rep[f"ref_boundary_count_{k}"], rep[f"max_boundary_count_first_batch_{k}"] = res.ref_boundary_count.tolist(), int(res.boundary_count.max())
    rep["route"] = st["route"]
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, kw in runs.items():
            t[k].append(timed(lambda: S.screen_1m(model, win, edits, batch=B, **kw))[0])
    for k in runs:
        rep[f"{k}_s"] = [round(x, 3) for x in t[k]]
        rep[f"{k}_edits_per_s"] = round(len(edits) / min(t[k]), 1)
    base = min(t["insulation"])
    rep["insulation_spread_ms"] = round((max(t["insulation"]) - base) * 1e3, 1)
    for k in ("boundaries", "boundaries_filled"):
        rep[f"{k}_added_ms_per_repetition"] = [round((y - x) * 1e3, 1) for x, y in zip(t["insulation"], t[k])]
        rep[f"{k}_added_ms_best_of_three"] = round((min(t[k]) - base) * 1e3, 1)
        rep[f"{k}_over_insulation"] = round(min(t[k]) / base, 4)
        rep[f"{k}_within_insulation_spread"] = bool(min(t[k]) <= max(t["insulation"]))
    return rep


def naive_both(model, win, edits, batch, keep_maps=False):
    """`naive` on both strands: every batch's edited windows through Net's Encoder and Decoder_1m forwards and reverse-complemented, merged."""
    sc = S._Screen(model.net, win, {})
    ref_map, _ = engine.screen_merge_strands(sc.ctx, sc.whole([])[0], sc.whole([], reverse=True)[0])
    ref_map = ref_map[0].contiguous()
    out, maps_all = [], []
    with torch.no_grad():
        for i0 in range(0, len(edits), batch):
            maps, _ = engine.screen_merge_strands(sc.ctx, sc.whole(edits[i0: i0 + batch])[0], sc.whole(edits[i0: i0 + batch], reverse=True)[0])
            out.append(engine.screen_scores(sc.ctx, maps, ref_map)[1])
            if keep_maps:
                maps_all.append(maps.clone())
    return torch.cat(out), (torch.cat(maps_all) if keep_maps else None)


def time_strands(a, model, win, edits, dev):
    """The --strands both workload: screen_1m with strands="both", with strands="+" and the naive both-strand route, alternated, at B = 64."""
    B = 64
    rep = {"device": torch.cuda.get_device_name(dev), "edits": len(edits), "batch": B}
    st = {}
    rs_ = S.screen_1m(model, win, edits[:B], batch=B, keep_maps=True, stats=st, strands="both")          # warm-up and cross-check
    S.screen_1m(model, win, edits[:B], batch=B)
    _, mn = naive_both(model, win, edits[:B], B, keep_maps=True)
    rep.update({"route": st["route"], "reverse_two_part_items": st["reverse_two_part_items"], "reverse_whole_items": st["reverse_whole_items"],
                "front_bases_per_item": round(st["front_bases"] / B), "maps_maxabs_screen_vs_naive": float((rs_.maps - mn).abs().max()),
                "ref_strand_gap": float(rs_.ref_strand_gap), "strand_gap_over_delta_abs_mean_median": float((rs_.strand_gap / rs_.delta_abs_mean).median())})
    assert rep["maps_maxabs_screen_vs_naive"] < 2e-5, rep
    del rs_, mn
    tb, tp, tn = [], [], []
    for _ in range(a.reps):
        tb.append(timed(lambda: S.screen_1m(model, win, edits, batch=B, strands="both"))[0])
        tp.append(timed(lambda: S.screen_1m(model, win, edits, batch=B))[0])
        tn.append(timed(lambda: naive_both(model, win, edits, B))[0])
    rep.update({"both_s": [round(t, 3) for t in tb], "plus_s": [round(t, 3) for t in tp], "naive_both_s": [round(t, 3) for t in tn],
                "both_edits_per_s": round(len(edits) / min(tb), 1), "plus_edits_per_s": round(len(edits) / min(tp), 1),
                "naive_both_edits_per_s": round(len(edits) / min(tn), 1), "both_over_plus": round(min(tb) / min(tp), 3),
                "speedup_over_naive_both": round(min(tn) / min(tb), 2)})
    return rep


def fp32_residuals(model, win, ta, tb, pairs, index, batch):
    """Today's route to the non-additivity residual: the singles and the pairs through screen_1m with keep_maps=True, then
    r = (alt_AB - ref) - (alt_A - ref) - (alt_B - ref) in torch, in fp32.  (mean |r| per pair, the two results)."""
    one = S.screen_1m(model, win, ta + tb, batch=batch, keep_maps=True)
    two = S.screen_1m(model, win, pairs, batch=batch, keep_maps=True)
    ia = torch.tensor([i for i, _ in index], device=win.device)
    ib = torch.tensor([len(ta) + j for _, j in index], device=win.device)
    out = torch.empty(len(pairs), dtype=torch.float32, device=win.device)
    for k0 in range(0, len(pairs), 256):                                                  # chunks: the difference maps are temporaries
        k1 = min(k0 + 256, len(pairs))
        r = (two.maps[k0:k1] - two.ref_map) - (one.maps[ia[k0:k1]] - one.ref_map) - (one.maps[ib[k0:k1]] - one.ref_map)
        out[k0:k1] = r.abs().mean(dim=(1, 2))
    return out, one, two


def time_epistasis(a, model, win, dev):
    """The --epistasis NA NB workload: the NA x NB pairs of two lists of 4 kb mask tiles through epistasis_1m, and through two screen_1m calls with
    keep_maps=True plus the fp32 arithmetic in torch, alternated, best of three, at B = 64.  Outside the timing, the largest difference between the
    fp32 route's residual and the fp64 residual of the same maps, per pixel and in the per-pair mean."""
    na, nb = a.epistasis
    B = 64
    ta = S.tile_edits("mask", 4000, 4000, 100_000, 100_000 + 4000 * na)
    tb = S.tile_edits("mask", 4000, 4000, 600_000, 600_000 + 4000 * nb)
    pairs, index = S.pair_edits(ta, tb)
    rep = {"device": torch.cuda.get_device_name(dev), "pairs": len(pairs), "singles": na + nb, "batch": B}
    st = {}
    res = S.epistasis_1m(model, win, pairs, batch=B, stats=st)                              # warm-up and cross-check
    m32, one, two = fp32_residuals(model, win, ta, tb, pairs, index, B)
    rep.update({"route": st["route"], "bank_bytes": st["bank_bytes"], "kept_map_bytes_fp32_route": int(one.maps.numel() + two.maps.numel()) * 4})
    ref = two.ref_map.double()
    pix = torch.zeros((), dtype=torch.float64, device=dev)
    for k, (i, j) in enumerate(index):                                                    # the same maps, the kernel's arithmetic in torch fp64
        t = (one.maps[i].double() - ref) + (one.maps[na + j].double() - ref)
        r64 = (two.maps[k].double() - ref) - t
        r32 = (two.maps[k] - two.ref_map) - (one.maps[i] - one.ref_map) - (one.maps[na + j] - one.ref_map)
        pix = torch.maximum(pix, (r32.double() - r64).abs().max())
    rep.update({"max_abs_fp32_residual_minus_fp64_residual": float(pix), "max_abs_mean_fp32_route_minus_epistasis_1m": float((m32 - res.epi_abs_mean).abs().max()),
                "epi_abs_mean_median": float(res.epi_abs_mean.median()), "additive_abs_mean_median": float(res.additive_abs_mean.median()),
                "map_abs_max": float(two.ref_map.abs().max())})
    del one, two, m32, res
    te, tf = [], []
    for _ in range(3):
        te.append(timed(lambda: S.epistasis_1m(model, win, pairs, batch=B))[0])
        tf.append(timed(lambda: fp32_residuals(model, win, ta, tb, pairs, index, B)[0])[0])
    rep.update({"epistasis_1m_s": [round(t, 3) for t in te], "fp32_route_s": [round(t, 3) for t in tf], "epistasis_1m_pairs_per_s": round(len(pairs) / min(te), 1),
                "fp32_route_pairs_per_s": round(len(pairs) / min(tf), 1), "fp32_route_over_epistasis_1m": round(min(tf) / min(te), 3)})
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--screen-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "screen_1m.json"))
    ap.add_argument("--pairs", type=int, default=0, help="N: time the N x N pairs of two lists of N 4 kb mask tiles")
    ap.add_argument("--haplotype", type=int, default=0, help="M: time sets of M SNVs")
    ap.add_argument("--haplotypes", type=int, default=64)
    ap.add_argument("--haplotype-span", type=int, default=L)
    ap.add_argument("--indels", type=int, default=0, help="N: time N random 1-50-base indels at B = 64")
    ap.add_argument("--aligned", action="store_true", help="time the 3 250-edit workload with aligned=True against aligned=False")
    ap.add_argument("--tracks", action="store_true", help="time the 3 250-edit workload at B = 64 with insulation and viewpoint tracks against without")
    ap.add_argument("--strata", action="store_true", help="time the 3 250-edit workload at B = 64 with strata=True against without, plain and with aligned=True")
    ap.add_argument("--loops", action="store_true", help="time the 3 250-edit workload at B = 64 with loops=True against without, plain and with aligned=True")
    ap.add_argument("--boundaries", action="store_true", help="time the 3 250-edit workload at B = 64 with insulation=(5, 10, 25) and boundaries=True against "
                    "the insulation tracks alone")
    ap.add_argument("--strands", default="+", choices=("+", "both"), help="both: time the 3 250-edit workload on both strands at B = 64")
    ap.add_argument("--epistasis", type=int, nargs=2, metavar=("NA", "NB"), help="time the NA x NB mask-tile pairs through epistasis_1m against two screen_1m "
                    "calls with keep_maps=True plus fp32 arithmetic in torch")
    ap.add_argument("--commit", default="", help="recorded in the report")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = M.H1esc_1M(synthetic_seed=0).to(dev)
    c = window()
    win = torch.from_numpy(c).to(dev)
    if a.epistasis:
        rep = {"workload": f"H1esc_1M synthetic, 1 Mb window, the {a.epistasis[0]} x {a.epistasis[1]} pairs of 4 kb mask tiles; epistasis_1m against "
                           "screen_1m(singles, keep_maps=True) + screen_1m(pairs, keep_maps=True) + the residual in torch fp32, alternated, best of "
                           "three (every call includes its references)", "commit": a.commit}
        rep.update(time_epistasis(a, model, win, dev))
        print(json.dumps(rep))
        out = a.out if a.out != ap.get_default("out") else os.path.join(os.path.dirname(a.out), "screen_1m_epistasis.json")
        if out:
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:
                json.dump(rep, f, indent=1)
        return
    if a.indels:
        rep = {"workload": "H1esc_1M synthetic, 1 Mb window, random insertions and deletions; naive = the same alt windows through model.net; "
                           "snv_screen = SNVs at the same positions through the screen (every call includes its reference and, for indels, "
                           "building the stage-4 cache entries)", "commit": a.commit}
        rep.update(time_indels(a, model, win, c, dev))
        print(json.dumps(rep))
        out = a.out if a.out != ap.get_default("out") else os.path.join(os.path.dirname(a.out), "screen_1m_indels.json")
        if out:
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:
                json.dump(rep, f, indent=1)
        return
    if a.pairs or a.haplotype:
        rep = {"workload": "H1esc_1M synthetic, 1 Mb window, compound edits (screen.EditSet); naive = the same edited windows through model.net",
               "commit": a.commit}
        rep.update(time_sets(a, model, win, c, dev))
        print(json.dumps(rep))
        out = a.out if a.out != ap.get_default("out") else os.path.join(os.path.dirname(a.out), "screen_1m_sets.json")
        if out:
            os.makedirs(os.path.dirname(out), exist_ok=True)
            with open(out, "w") as f:
                json.dump(rep, f, indent=1)
        return
    edits = S.saturation_edits(c, 499_500, 500_500) + S.tile_edits("mask", 4000, 4000, 0, L)
    if a.strata:
        rep = {"workload": f"H1esc_1M synthetic, 1 Mb window, {len(edits)} edits (saturation SNVs of 1 kb + 250 4 kb mask tiles); screen_1m with "
                           "strata=True against without, each also with aligned=True, alternated (every call includes its reference)", "commit": a.commit}
        rep.update(time_strata(a, model, win, edits, dev))
        print(json.dumps(rep))
        out = a.out if a.out != ap.get_default("out") else os.path.join(os.path.dirname(a.out), "screen_1m_strata.json")
        if out:
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:
                json.dump(rep, f, indent=1)
        return
    if a.boundaries:
        rep = {"workload": f"H1esc_1M synthetic, 1 Mb window, {len(edits)} edits (saturation SNVs of 1 kb + 250 4 kb mask tiles); screen_1m with "
                           "insulation=(5, 10, 25) against the same plus boundaries=True and plus boundaries=BoundaryParams(min_strength=0.0) (full lists), "
                           "alternated (every call includes its reference)", "commit": a.commit}
        rep.update(time_boundaries(a, model, win, edits, dev))
        print(json.dumps(rep))
        out = a.out if a.out != ap.get_default("out") else os.path.join(os.path.dirname(a.out), "screen_1m_boundaries.json")
        if out:
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:
                json.dump(rep, f, indent=1)
        return
    if a.loops:
        rep = {"workload": f"H1esc_1M synthetic, 1 Mb window, {len(edits)} edits (saturation SNVs of 1 kb + 250 4 kb mask tiles); screen_1m with "
                           "loops=True and with loops=LoopParams(threshold=0.0) (full lists) against without, each also with aligned=True, alternated (every call includes its reference)", "commit": a.commit}
        rep.update(time_loops(a, model, win, edits, dev))
        print(json.dumps(rep))
        out = a.out if a.out != ap.get_default("out") else os.path.join(os.path.dirname(a.out), "screen_1m_loops.json")
        if out:
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:
                json.dump(rep, f, indent=1)
        return
    if a.tracks:
        rep = {"workload": f"H1esc_1M synthetic, 1 Mb window, {len(edits)} edits (saturation SNVs of 1 kb + 250 4 kb mask tiles); screen_1m with "
                           "insulation=(5, 10, 25), viewpoints=[125] against without, alternated (every call includes its reference)", "commit": a.commit}
        rep.update(time_tracks(a, model, win, edits, dev))
        print(json.dumps(rep))
        out = a.out if a.out != ap.get_default("out") else os.path.join(os.path.dirname(a.out), "screen_1m_tracks.json")
        if out:
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:
                json.dump(rep, f, indent=1)
        return
    if a.aligned:
        rep = {"workload": f"H1esc_1M synthetic, 1 Mb window, {len(edits)} edits (saturation SNVs of 1 kb + 250 4 kb mask tiles); screen_1m with "
                           "aligned=True against aligned=False, alternated (every call includes its reference)", "commit": a.commit}
        rep.update(time_aligned(a, model, win, edits, dev))
        print(json.dumps(rep))
        out = a.out if a.out != ap.get_default("out") else os.path.join(os.path.dirname(a.out), "screen_1m_aligned.json")
        if out:
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:
                json.dump(rep, f, indent=1)
        return
    if a.strands == "both":
        rep = {"workload": f"H1esc_1M synthetic, 1 Mb window, {len(edits)} edits (saturation SNVs of 1 kb + 250 4 kb mask tiles); screen_1m with "
                           "strands='both' against strands='+' and against the edited windows through Net on both strands, merged; alternated "
                           "(every call includes its reference)", "commit": a.commit}
        rep.update(time_strands(a, model, win, edits, dev))
        print(json.dumps(rep))
        out = a.out if a.out != ap.get_default("out") else os.path.join(os.path.dirname(a.out), "screen_1m_strands.json")
        if out:
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:
                json.dump(rep, f, indent=1)
        return
    rep = {"workload": f"H1esc_1M synthetic, 1 Mb window, {len(edits)} edits (saturation SNVs of 1 kb + 250 4 kb mask tiles)", "edits": len(edits)}
    # warm-up (library load, nets, workspaces) and the cross-check of both routes' maps
    st = {}
    rs = S.screen_1m(model, win, edits[:64], batch=64, keep_maps=True, stats=st)
    rep["route"] = st["route"]
    if not a.screen_only:
        _, mn = naive(model, win, edits[:64], 64, keep_maps=True)
        rep["maps_maxabs_screen_vs_naive"] = float((rs.maps - mn).abs().max())
        assert rep["maps_maxabs_screen_vs_naive"] < 2e-5, rep
    for B in [int(b) for b in a.batches.split(",")]:
        ts, tn = [], []
        for _ in range(a.reps):
            t, _ = timed(lambda: S.screen_1m(model, win, edits, batch=B))
            ts.append(t)
            if not a.screen_only:
                t, _ = timed(lambda: naive(model, win, edits, B))
                tn.append(t)
        row = {"screen_s": [round(t, 3) for t in ts], "screen_edits_per_s": round(len(edits) / min(ts), 1)}
        if tn:
            row.update({"naive_s": [round(t, 3) for t in tn], "naive_edits_per_s": round(len(edits) / min(tn), 1),
                        "speedup": round(min(tn) / min(ts), 2)})
        rep[f"B{B}"] = row
        print(json.dumps({f"B{B}": row}), flush=True)
    print(json.dumps(rep))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rep, f, indent=1)


if __name__ == "__main__":
    main()
