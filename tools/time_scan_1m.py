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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", type=float, nargs="?", default=40.0, help="length of the synthetic chromosome in Mb")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scan_1m.json"))
    ap.add_argument("--commit", default="", help="recorded in the report")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = M.H1esc_1M(synthetic_seed=0).to(dev)
    codes = torch.from_numpy(chromosome(int(a.mb * 1_000_000))).to(dev)
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
    print(json.dumps(rep))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rep, f, indent=1)


if __name__ == "__main__":
    main()
