"""What the chromosome scan (orca_amd/scan.py: scan_1m) costs beside the model itself, in one process, alternated, best of three.

Workload: synthetic H1esc_1M on a synthetic chromosome (random bases with N runs; 40 Mb by default), 1 Mb windows every 400 kb, trim 10, 32 windows
per batch - `scan_1m`'s defaults.
  (a) decode_only   the same batches of code windows through Net's Encoder (forward_codes) and Decoder_1m, and nothing else: what a user could run
                    before `scan_1m` existed (the maps would still have to go to the host, 250 KB each, and be registered there) - the baseline
  (b) band          scan_1m(model, codes): (a) plus orca_scan_stitch_band per batch and orca_scan_band_finish
  (c) readouts      (b) with insulation=(5, 10, 25), boundaries=True, spread=True: plus orca_scan_band_insulation, orca_scan_boundary_strength and the lists
  (d) both_strands  (c) with strands="both": every window twice, merged by orca_screen_merge_strands
JSON on stdout and in profiles/scan_1m.json: the times, the ratios over (a) and the spread of (a)'s repetitions, which says how small a ratio the run
can resolve.

    python tools/time_scan_1m.py            # 40 Mb
    python tools/time_scan_1m.py 8          # 8 Mb

``--loops``: what the loop (dot) calls of ``scan_1m(..., loops=)`` add to (b), the same way - (b) alternated with
  (e) loops         (b) with loops=True: plus orca_scan_band_dot_enrichment, orca_scan_band_dot_offsets, orca_scan_band_dot_list and the lists' copy
  (f) loops_every   (b) with loops=LoopParams(threshold=-1e30): every local maximum of the enrichment is called, the longest list the band can give
into profiles/scan_1m_loops.json: the times, per repetition the difference to the band-only run beside it, and the spread of the band-only
repetitions, which says how small a difference the run can resolve.

    python tools/time_scan_1m.py --loops
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from orca_amd import orca_models as M
from orca_amd import scan as C
from orca_amd import screen as S

WINDOW_BP, STEP_BP, TRIM, BATCH = 1_000_000, 400_000, 10, 32
READOUTS = dict(insulation=(5, 10, 25), boundaries=True, spread=True)


def chromosome(length, seed=5):
    rs = np.random.RandomState(seed)
    c = rs.randint(0, 4, length).astype(np.uint8)
    for a in rs.randint(0, length - 2000, max(1, length // 80_000)):
        c[a: a + rs.randint(50, 2000)] = 4
    return c


def decode_only(model, codes):
    """(a): `scan_1m`'s batches of windows through the Encoder and Decoder_1m, the maps dropped"""
    net = S._net_of(model)
    off = C.plan_windows(codes.numel() // 4000, WINDOW_BP // 4000, STEP_BP // 4000, TRIM)
    with torch.no_grad():
        for k0 in range(0, off.size, BATCH):
            win = torch.stack([codes[int(a) * 4000: int(a) * 4000 + WINDOW_BP] for a in off[k0: k0 + BATCH]])
            maps = net._dec(net._enc.forward_codes(win))[:, 0]
    return maps


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def time_loops(a, model, codes):
    """--loops: (b) alternated with (e) and (f)"""
    every = S.LoopParams(threshold=-1e30)
    runs = {"band": lambda: C.scan_1m(model, codes), "loops": lambda: C.scan_1m(model, codes, loops=True),
            "loops_every": lambda: C.scan_1m(model, codes, loops=every)}
    for fn in runs.values():                                                                     # warm-up
        fn()
    st, st_every = {}, {}
    C.scan_1m(model, codes, loops=True, stats=st)
    C.scan_1m(model, codes, loops=every, stats=st_every)
    rep = {"workload": f"H1esc_1M synthetic, a synthetic chromosome of {a.mb:g} Mb, 1 Mb windows every 400 kb, trim 10, 32 windows per batch; scan_1m with "
                       "the band only against the same with loops=True (LoopParams(): p 1, w 4, r 2, threshold 0.25) and with "
                       "loops=LoopParams(threshold=-1e30), which calls every local maximum; alternated, best of three", "commit": a.commit,
           "device": torch.cuda.get_device_name(torch.device("cuda:0")), "weights": "synthetic", "windows": st["windows"], "batches": st["batches"], "bins": st["bins"],
           "depth": st["depth"], "reps": a.reps, "loops_listed": st["loops"], "loops_every_listed": st_every["loops"]}
    t = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, fn in runs.items():
            t[k].append(timed(fn)[0])
    for k in runs:
        rep[f"{k}_s"] = [round(x, 4) for x in t[k]]
    rep["band_spread_ms"] = round((max(t["band"]) - min(t["band"])) * 1e3, 3)
    for k in ("loops", "loops_every"):
        rep[f"{k}_minus_band_ms"] = [round((x - b) * 1e3, 3) for x, b in zip(t[k], t["band"])]       # per repetition, against the band-only run beside it
        rep[f"{k}_over_band"] = round(min(t[k]) / min(t["band"]), 4)
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", type=float, nargs="?", default=40.0, help="length of the synthetic chromosome in Mb")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loops", action="store_true", help="time the loop calls against the band-only scan (profiles/scan_1m_loops.json)")
    ap.add_argument("--out", default=None, help="the report; profiles/scan_1m.json, or profiles/scan_1m_loops.json with --loops")
    ap.add_argument("--commit", default="", help="recorded in the report")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scan_1m_loops.json" if a.loops else "scan_1m.json")
    dev = torch.device("cuda:0")
    model = M.H1esc_1M(synthetic_seed=0).to(dev)
    codes = torch.from_numpy(chromosome(int(a.mb * 1_000_000))).to(dev)
    if a.loops:
        return report(time_loops(a, model, codes), a.out)
    runs = {"decode_only": lambda: decode_only(model, codes), "band": lambda: C.scan_1m(model, codes),
            "readouts": lambda: C.scan_1m(model, codes, **READOUTS), "both_strands": lambda: C.scan_1m(model, codes, strands="both", **READOUTS)}
    st = {}
    for k, fn in runs.items():                                                                   # warm-up
        res = fn()
    C.scan_1m(model, codes, stats=st, **READOUTS)
    rep = {"workload": f"H1esc_1M synthetic, a synthetic chromosome of {a.mb:g} Mb, 1 Mb windows every 400 kb, trim 10, 32 windows per batch; the same "
                       "batches through Encoder + Decoder_1m alone (decode_only) against scan_1m with the band only, with insulation=(5, 10, 25), "
                       "boundaries=True, spread=True, and with the same on both strands; alternated, best of three", "commit": a.commit,
           "device": torch.cuda.get_device_name(dev), "weights": "synthetic", "windows": st["windows"], "batches": st["batches"], "bins": st["bins"], "depth": st["depth"],
           "reps": a.reps, "boundaries_listed": [int(len(b[0])) for b in res.boundaries], "band_mbytes": round(st["bins"] * st["depth"] * 4 / 1e6, 1)}
    t = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, fn in runs.items():
            t[k].append(timed(fn)[0])
    base = min(t["decode_only"])
    for k in runs:
        rep[f"{k}_s"] = [round(x, 4) for x in t[k]]
        rep[f"{k}_ms_per_window"] = round(min(t[k]) / st["windows"] * 1e3, 3)
    rep["decode_only_spread"] = round(max(t["decode_only"]) / base, 4)
    for k in ("band", "readouts", "both_strands"):
        rep[f"{k}_over_decode_only"] = round(min(t[k]) / base, 4)
    report(rep, a.out)


def report(rep, out):
    print(json.dumps(rep))
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            json.dump(rep, f, indent=1)


if __name__ == "__main__":
    main()
