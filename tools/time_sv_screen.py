"""SV screen timing (BASELINE configs[4]) on one GPU: python tools/time_sv_screen.py [n_svs] [incremental 0|1] [streams: auxiliary contexts of the local encodes, 0 = none, -1 = default] [align: 1 = unaligned (default), 4000 = the 4 kb grid]
--scores: what the on-device impact scores cost - the same variants through (a) the plain screen, (b) scores=True, (c) scores=True, keep_maps=False,
alternated in one run, best of three each; writes profiles/sv_screen_scores.json
--tracks: what the readouts per level cost - the same variants with (a) scores=True, (b) scores=True, insulation=(5, 10, 25), viewpoints=[one position],
strata=True, alternated in one run, best of three each; the added ms per variant is reported against the scores=True repetition beside it, with the
spread of the baseline's three repetitions; writes profiles/sv_screen_tracks.json
--loops: what the loop calls per level cost - the same variants with (a) scores=True, (b) scores=True, loops=True (on the synthetic weights the default
threshold may call nothing) and (c) scores=True, loops=LoopParams(threshold=-1e30): every list full, alternated in one run, best of three each; the added
ms per variant against the scores=True repetition beside it, with the spread of the baseline's three repetitions; writes profiles/sv_screen_loops.json
--compartments: what the compartment eigenvectors per level cost - the same variants with (a) scores=True, (b) scores=True, compartments=True and (c)
scores=True, compartments=CompartmentParams(n_eigs=3), alternated in one run, best of three each; the added ms per variant against the scores=True
repetition beside it, with the spread of the baseline's three repetitions, and - the weights are synthetic - the share of (allele, level, channel, vector)
pairs that converged with the median and the largest number of iterations; writes profiles/sv_screen_compartments.json
--boundaries: what the boundary calls per level cost - the same variants with (a) scores=True, insulation=(5, 10, 25), (b) the same plus boundaries=True
and (c) the same plus boundaries=BoundaryParams(min_strength=0.0): every list as full as it gets, alternated in one run, best of three each; the added
ms per variant against the insulation-only repetition beside it, with the spread of that baseline's three repetitions, and the boundaries called per
run; writes profiles/sv_screen_boundaries.json"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SCORES = "--scores" in sys.argv
TRACKS = "--tracks" in sys.argv
LOOPS = "--loops" in sys.argv
COMPARTMENTS = "--compartments" in sys.argv
BOUNDARIES = "--boundaries" in sys.argv
sys.argv = [a for a in sys.argv if a not in ("--scores", "--tracks", "--loops", "--compartments", "--boundaries")]
import torch
from orca_amd import orca_models, sv
n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
inc = (sys.argv[2] != "0") if len(sys.argv) > 2 else True
streams = int(sys.argv[3]) if len(sys.argv) > 3 and int(sys.argv[3]) >= 0 else None
align = int(sys.argv[4]) if len(sys.argv) > 4 else 1
dev = torch.device("cuda:0")
h1 = orca_models.H1esc(synthetic_seed=0)
g = torch.Generator(device=dev).manual_seed(5)
genome = torch.randint(0, 4, (40_000_000,), device=dev, generator=g, dtype=torch.uint8)
svs = sv.synth_svs(n + 2, 40_000_000, align=align)
sv.sv_screen([h1], genome, svs[:2], 40_000_000, incremental=inc, min_uses=1, streams=streams)
torch.cuda.synchronize()


def timed_runs(modes, warm=None, on_result=None, note=None):
    """The loop of all four comparisons: {mode: [a record per repetition]} of three repetitions with the ``modes`` ({name: sv_screen keywords})
    alternated, a synchronise on both sides of the clock and the stage-cache build time subtracted.  ``warm``: the mode that is called once before
    the clock (a new kernel's first launch); ``on_result(name)``: called before every run, returns that run's on_result; ``note(name)``: more to print."""
    if warm is not None:
        sv.sv_screen([h1], genome, svs[:2], 40_000_000, incremental=inc, min_uses=1, streams=streams, **modes[warm])
        torch.cuda.synchronize()
    runs = {k: [] for k in modes}
    for rep in range(3):
        for k, kw in modes.items():
            st = {}
            cb = on_result(k) if on_result else (lambda i, e: None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sv.sv_screen([h1], genome, svs[2:], 40_000_000, incremental=inc, stats=st, streams=streams, on_result=cb, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            build = (st.get("stage3_cache") or {}).get("build_s", 0.0)      # the stage cache is rebuilt by every call: its time is not the screen's
            runs[k].append({"total_s": round(dt, 4), "stage_cache_build_s": build, "ms_per_sv": round((dt - build) / n * 1e3, 3)})
            print(k, runs[k][-1], *(note(k) if note else ()))
    return runs


def summary(flag, runs, base, **more):
    """The head of a mode's JSON: the run's settings, ``more``, the runs, the best of three per mode and the spread of the baseline ``base``'s three."""
    best = {k: min(r["ms_per_sv"] for r in v) for k, v in runs.items()}
    spread = max(r["ms_per_sv"] for r in runs[base]) - best[base]
    return {"tool": "tools/time_sv_screen.py " + flag, "n_svs": n, "incremental": inc, "streams": streams, "align": align, **more, "runs": runs,
            "best_ms_per_sv": best, base + "_spread_ms_per_sv": round(spread, 3)}, best, spread


def added(out, runs, best, spread, k, base="scores"):
    """What mode ``k`` adds to the baseline: per repetition against the baseline repetition beside it, and best of three against best of three."""
    out[k + "_added_ms_per_sv_per_repetition"] = [round(t["ms_per_sv"] - s["ms_per_sv"], 3) for s, t in zip(runs[base], runs[k])]
    out[k + "_added_ms_per_sv_best_of_three"] = round(best[k] - best[base], 3)
    out[k + "_within_" + base + "_spread"] = bool(best[k] <= best[base] + spread)


def finish(name, out):
    import json
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sv_screen_" + name + ".json")
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))
    sys.exit(0)


if SCORES:
    runs = timed_runs({"plain": {}, "scores": {"scores": True}, "scores_no_maps": {"scores": True, "keep_maps": False}})
    out, best, spread = summary("--scores", runs, "plain")
    out.update({"scores_cost_ms_per_sv": round(best["scores"] - best["plain"], 3), "scores_within_plain_spread": bool(best["scores"] <= best["plain"] + spread),
                "no_maps_saving_ms_per_sv": round(best["plain"] - best["scores_no_maps"], 3)})
    finish("scores", out)
if TRACKS:
    modes = {"scores": {"scores": True},
             "tracks": {"scores": True, "insulation": (5, 10, 25), "viewpoints": [20_000_000], "strata": True}}
    runs = timed_runs(modes, warm="tracks")
    out, best, spread = summary("--tracks", runs, "scores", modes={k: {a: list(b) if isinstance(b, tuple) else b for a, b in kw.items()} for k, kw in modes.items()})
    added(out, runs, best, spread, "tracks")
    finish("tracks", out)
if LOOPS:
    from orca_amd import screen
    modes = {"scores": {"scores": True}, "loops": {"scores": True, "loops": True},
             "loops_filled": {"scores": True, "loops": screen.LoopParams(threshold=-1e30)}}
    dots = {k: 0 for k in modes}

    def tally(k):
        dots[k] = 0

        def on_result(i, e):
            if "loop_params" in e["scores"]:
                dots[k] += int(sum(m["ref_loop_count"].sum() + m["loop_count"].sum() for m in e["scores"]["models"]))
        return on_result
    runs = timed_runs(modes, warm="loops_filled", on_result=tally, note=lambda k: ("dots", dots[k]))
    out, best, spread = summary("--loops", runs, "scores", dots_called_per_run=dots,
                                modes={"scores": "scores=True", "loops": "scores=True, loops=True", "loops_filled": "scores=True, loops=LoopParams(threshold=-1e30)"})
    for k in ("loops", "loops_filled"):
        added(out, runs, best, spread, k)
    finish("loops", out)
if COMPARTMENTS:
    import numpy as np
    modes = {"scores": {"scores": True}, "compartments": {"scores": True, "compartments": True},
             "compartments_3": {"scores": True, "compartments": sv.CompartmentParams(n_eigs=3)}}
    seen = {}

    def tally(k):
        seen[k] = {"converged": [], "iterations": []}

        def on_result(i, e):
            if "compartment_params" in e["scores"]:
                for m in e["scores"]["models"]:
                    for side in ("ref_", ""):
                        seen[k]["converged"].append(m[side + "compartment_converged"].reshape(-1))
                        seen[k]["iterations"].append(m[side + "compartment_iterations"].reshape(-1))
        return on_result
    runs = timed_runs(modes, warm="compartments_3", on_result=tally)
    out, best, spread = summary("--compartments", runs, "scores", weights="synthetic",
                                modes={"scores": "scores=True", "compartments": "scores=True, compartments=True", "compartments_3": "scores=True, compartments=CompartmentParams(n_eigs=3)"})
    for k in ("compartments", "compartments_3"):
        added(out, runs, best, spread, k)
        conv, its = np.concatenate(seen[k]["converged"]), np.concatenate(seen[k]["iterations"])
        out[k + "_convergence"] = {"pairs": int(conv.size), "converged_share": round(float(conv.mean()), 4), "iterations_median": float(np.median(its)),
                                   "iterations_max": int(its.max())}
    finish("compartments", out)
if BOUNDARIES:
    from orca_amd import screen
    ins = {"scores": True, "insulation": (5, 10, 25)}
    modes = {"insulation": ins, "boundaries": dict(ins, boundaries=True), "boundaries_filled": dict(ins, boundaries=screen.BoundaryParams(min_strength=0.0))}
    called = {k: 0 for k in modes}

    def tally(k):
        called[k] = 0

        def on_result(i, e):
            if "boundary_params" in e["scores"]:
                called[k] += int(sum(m["ref_boundary_count"].sum() + m["boundary_count"].sum() for m in e["scores"]["models"]))
        return on_result
    runs = timed_runs(modes, warm="boundaries_filled", on_result=tally, note=lambda k: ("boundaries", called[k]))
    out, best, spread = summary("--boundaries", runs, "insulation", weights="synthetic", boundaries_called_per_run=called,
                                modes={"insulation": "scores=True, insulation=(5, 10, 25)", "boundaries": "scores=True, insulation=(5, 10, 25), boundaries=True",
                                       "boundaries_filled": "scores=True, insulation=(5, 10, 25), boundaries=BoundaryParams(min_strength=0.0)"})
    for k in ("boundaries", "boundaries_filled"):
        added(out, runs, best, spread, k, base="insulation")
    finish("boundaries", out)
t0 = time.perf_counter()
st = {}
sv.sv_screen([h1], genome, svs[2:], 40_000_000, incremental=inc, stats=st, streams=streams)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(f"incremental={inc} streams={streams} {n} SVs: {dt / n * 1e3:.1f} ms per SV = {n / dt:.2f} SV/s  {st}")

if inc:   # where a variant's time goes (on the grid: bins from the chromosome encodings; off it: the stage-3 cache)
    import time as T
    cache = sv.ChromEncodings(h1.net0, genome)
    if align == 4000:
        for k in (("+", 0), ("-", 0), ("+", 2000), ("-", 2000)):
            cache.get(*k)
    else:
        cache.stage3 = sv.Stage4Cache(h1.net0, genome)
        torch.cuda.synchronize(); t = T.perf_counter()
        cache.stage3.build_all()
        torch.cuda.synchronize(); print(f"stage-4 cache: 160 entries in {T.perf_counter() - t:.2f} s")
    enc0 = torch.empty((4, 128, 8000), device=dev)
    from orca_amd import engine
    ns = 4 if streams is None else streams
    pool = engine.context_pool(dev, ns) if ns > 0 else None
    acc = {"assemble": 0.0, "encode_window": 0.0, "cascade": 0.0, "to_host": 0.0}
    for v in svs[2:18]:
        rp, rw, rm, ap, aw, am = sv.sv_windows(v, 40_000_000)
        torch.cuda.synchronize(); t = T.perf_counter()
        codes = torch.stack([sv.assemble_codes(genome, rp), sv.assemble_codes(genome, ap)])
        torch.cuda.synchronize(); acc["assemble"] += T.perf_counter() - t; t = T.perf_counter()
        with engine.defer_overflow_guard():      # as in sv_screen: no range check (= stream sync) per call
            sv.encode_windows(cache, [rp, ap], codes, enc0, build=False, pool=pool)
        torch.cuda.synchronize(); acc["encode_window"] += T.perf_counter() - t; t = T.perf_counter()
        with engine.defer_overflow_guard():
            merged, starts = sv._cascade_windows(h1, enc0, [(rm, rw), (am, aw)])
        torch.cuda.synchronize(); acc["cascade"] += T.perf_counter() - t; t = T.perf_counter()
        sv._window_outputs(h1, merged, starts, [(rm, rw), (am, aw)], "c")
        acc["to_host"] += T.perf_counter() - t
    print({k: round(v / 16 * 1e3, 2) for k, v in acc.items()}, "ms per SV")
