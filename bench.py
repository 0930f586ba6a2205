#!/usr/bin/env python
"""bench.py - headline benchmark of the Orca hot path on MI355X.

Timed region (the driver's contract; `value`): BASELINE.json configs[1] - H1-ESC-shaped 32 Mb model (Encoder + Encoder2 +
six Decoders + Decoder_1m), ONE random 32 Mb sequence, fp32-class arithmetic.  One "step" is what the reference's
`genomepredict` does on the device for one model: both strands through net0 -> net -> the 6-level decoder cascade
(+ denet_1_pt at 4 kb) and the strand merge.  The input is resident in HBM before the timed region: the sequence packed
to 1 byte per base (what `genomepredict` keeps after one pass over the reference's float32 [1,32e6,4] array; both strands
are encoded from that one buffer) - `--float-input` keeps the two float strands instead; weights are
deterministic synthetic tensors of the reference architecture (the real checkpoints are a 1.3 GB download, unavailable
offline).  N > 1: every rank runs this workload on its own sequence (independent 32 Mb windows, the reference's
structural-variant-screen pattern, BASELINE config 5): weak scaling, no data-path collective.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the line: `value`, `ms_per_step` and the fields derived from them.
`--dump-outputs DIR` writes what the last timed step returned on rank 0 - the six strand-merged maps, levels 32, 16, 8, 4, 2, 1 Mb
in that order, as DIR/pred_0.npy .. pred_5.npy (float32 [250,250], the fixture G8's `pred_<j>`); the inputs are seeded, so two
builds run with the same arguments can be compared map for map.

`--full` also times the conv kernels of the timed steps with HIP events (`roofline`, `roofline_hbm_bound_kernel`) and measures, in
the same run, OUTSIDE the timed region, and reports in the same JSON line:
  * `sharded_256mb` (every N, BASELINE config 4 / north star): H1esc_256M-shaped model on one random 256 Mb sequence,
    both strands - the Encoder's 64 000 bins sharded over the N ranks (each rank holds only its bins' bases +- the 112 kb halo),
    ONE RCCL all-gather per strand (through the C ABI's orca_allgather; torch.distributed if that cannot be set up), then
    Encoder2(64 000 bins) -> Encoder3 -> 4 Decoders, one strand each on ranks 0 / 1, one all-gather of the maps.  Strong scaling:
    per-rank encoder ms, all-gather ms, tail ms, Mb/s - and `parity` of the result against the reference's own
    genomepredict_256Mb on this sequence (tests/golden/G20_full256m.npz).
  * `sharded_32mb` (every even N and N = 1): the HEADLINE workload as one strong-scaling job - strand split x Encoder bin
    shards (orca_amd.dist.strand_bin_sharded_32m), with `parity` against G8.
  * `parity` (N = 1): the timed steps' own six maps against the shipped fixture tests/golden/G8_full32m.npz - the
    REFERENCE's genomepredict on CPU for exactly this sequence, weights and zoom position.
  * `exact_f32`, `bf16x3` (N = 1): short loops with every module on the exact fp32 MFMA kernels / in the range-safe fallback arithmetic, each with its parity vs G8.
  * `concurrent_strands` (N = 1): the opt-in mode ORCA_STRAND_STREAMS=1 (both strands' Encoders side by side on two streams), 5 steps.
  * `roofline_decoder` (N = 1): one Decoder forward (118 Conv2d) at B = 2 and at B = 4 under HIP events.
  * `config3` (N = 1): BASELINE configs[2] - HFF-shaped model, batch of 8, bf16 Encoder + fp16-plane Decoders, 2 timed batches,
    roofline of its dominant kernel, parity against the reference rows of G17.
  * `config5` (N = 1): BASELINE configs[4] - 256 of the 1024 synthetic SVs through orca_amd.sv.sv_screen (incremental encoding; 16 of them
    also as two whole genomepredict calls; the full screen: tools/run_configs.py config5_1024, profiles/r05_config5_1024.json).
  * `roofline.traffic` (N = 1): measured in the run by two rocprofv3 counter passes over the same Encoder launches in child processes.
  * `cpu_baseline` (N = 1): the oracle (= the torch CPU ops the reference dispatches) on ONE WHOLE 32 Mb strand (+ the 8 Mb sample of rounds 1-4).

Prints ONE JSON line (rank 0).  value = strand-Mb of sequence encoded AND decoded per second over the whole job
(2 strands x 32 Mb per step per rank).
"""
import argparse
import json
import os
import sys
import threading
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # multi-process GPU work on this driver needs dmabuf IPC (before the HIP runtime starts)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_16BIT_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: bf16/f16 MFMA dense peak (v_mfma_f32_32x32x16_{bf16,f16})
L_BP = 32_000_000
ENC_FLOP_PER_BP = 465555.5
DEC_TFLOP = {"first": 0.2812, "withy": 0.2905, "dec1m": 0.1774, "enc2": 0.0274}


def step_flops():
    per_strand = ENC_FLOP_PER_BP * L_BP / 1e12 + DEC_TFLOP["enc2"] + DEC_TFLOP["first"] + 5 * DEC_TFLOP["withy"] + DEC_TFLOP["dec1m"]
    return 2 * per_strand


def usable_cores():
    """Host cores this process may actually use: affinity mask capped by the cgroup CPU quota
    (the GPU box exposes 256 logical CPUs but grants a 16-core quota; oversubscribing torch's
    intra-op pool beyond the quota makes the CPU path several times SLOWER)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


def cpu_baseline(seed, sample_bp=8_000_000):
    """Reference-architecture PyTorch-CPU fp32 forward (oracle/orca_oracle.py = the torch ops the
    reference dispatches with use_cuda=False) on a bounded sample of the same workload: the Encoder on `sample_bp` bases, EXTRAPOLATED to the
    strand (its 800 kb blocks are independent and equal: orca_modules.py:955-977), everything after it in full.  `--cpu-full-strand` (or
    tools/run_configs.py cpu_full) times the whole 32 Mb strand once: profiles/r04_cpu_full_strand.json."""
    from oracle import orca_oracle as O
    from orca_amd import synth
    from tests.util import synth_sd
    ncores = usable_cores()
    torch.set_num_threads(ncores)
    # default: 10 reference blocks, ~13 s on the GPU box's 16 host cores, ~15 s with the rest
    x = torch.from_numpy(synth.synth_sequence(sample_bp, seed=1)).transpose(1, 2)
    sd0 = synth_sd("Encoder", seed)
    O.encoder_forward(sd0, x[:, :, :912000])  # warm-up
    t = time.perf_counter()
    enc = O.encoder_forward(sd0, x)
    t_enc = time.perf_counter() - t
    nm, _ = synth.synth_normmats_32m()
    sd2 = synth_sd("Encoder2", seed)
    encfull = torch.from_numpy((np.random.RandomState(3).rand(1, 128, 8000) * 0.5).astype(np.float32))
    t = time.perf_counter()
    encs = O.encoder2_forward(sd2, encfull)
    pred = None
    for j, lv in enumerate([32, 16, 8, 4, 2, 1]):
        de = torch.log(torch.from_numpy(nm[lv][None, None].astype(np.float32)))
        sdd = synth_sd("Decoder", seed + lv, upsample_mode="bilinear")
        pred = O.decoder_forward(sdd, encs[5 - j][:, :, :250], de, None if pred is None else pred[:, :, 60:185, 60:185], "bilinear")
    O.decoder_1m_forward(synth_sd("Decoder_1m", seed), encs[0][:, :, :250])
    t_rest = time.perf_counter() - t
    t_strand = t_enc * (L_BP / sample_bp) + t_rest
    return {"value": round(L_BP / 1e6 / t_strand, 4), "unit": "Mb/s", "cores": ncores, "kind": "port",
            "extrapolated": sample_bp < L_BP,
            "sample": (f"Encoder on {sample_bp // 1000000} Mb ({sample_bp // 800000} reference blocks, {t_enc:.1f}s" + (f", EXTRAPOLATED x{L_BP // sample_bp}" if sample_bp < L_BP else ", the whole strand") + ") + "
                       f"Encoder2(8000 bins) + 6 Decoder + Decoder_1m ({t_rest:.1f}s), torch CPU fp32, {ncores} threads"),
            "t_encoder_sample_s": round(t_enc, 2), "t_decoders_s": round(t_rest, 2)}


def measure_traffic_in_run(kernel_name, timeout_s=240):
    """HBM traffic of the dominant kernel measured IN THIS RUN: two separate `rocprofv3 --kernel-trace --pmc` passes
    (FETCH_SIZE, WRITE_SIZE: one counter per pass, MI355X_MICROARCH.md 'rocprofv3 PMC slots') over `tools/prof_encoder.py 32 f16x2 1 codes`
    (two forwards of a 32 Mb strand - the launches of the timed region, same kernels, same sizes) in child processes; bytes per launch =
    (2 x FETCH_SIZE + WRITE_SIZE) x 1024 / launches - FETCH_SIZE doubled per the guide's gfx950 correction, both counters in KiB.  Returns
    (bytes_per_launch, launches) or (None, reason): any failure (no rocprofv3, a timeout, an unknown kernel) leaves the committed number in place."""
    import csv, glob, re, shutil, subprocess, tempfile
    table = {"conv1d_k9_p16_kernel<cout=64,f16x2>": (re.compile(r"^void conv1d_k9_p16_kernel<64,"), 4000.0),
             "conv1d_k9_p16x_kernel<cout=96,f16x2>": (re.compile(r"^void conv1d_k9_p16x_kernel<\d, (true|false), 3, 96>"), 2500.0),
             "conv1d_first_mfma_p16_kernel<0,0,25>": (re.compile(r"^void conv1d_first_mfma_p16_kernel<0, 0, 25>"), 800.0)}
    if any(k.startswith(("ROCPROF", "ROCP_", "ROCPROFILER")) or (k == "LD_PRELOAD" and "rocprof" in v) for k, v in os.environ.items()):
        return None, "this run is itself under a profiler (its environment would be inherited by the counter passes)"
    if kernel_name not in table or shutil.which("rocprofv3") is None:
        return None, "no rocprofv3 on this box" if kernel_name in table else f"no counter recipe for {kernel_name}"
    rx, min_us = table[kernel_name]
    sums = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="orca_pmc_", dir="/tmp")
        try:
            subprocess.run(["rocprofv3", "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
                            os.path.join(ROOT, "tools", "prof_encoder.py"), "32", "f16x2", "1", "codes"], cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"),
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s, check=True)
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            tot, disp = 0.0, set()
            for r in csv.DictReader(open(files[0])):
                if r["Counter_Name"] == counter and rx.search(r["Kernel_Name"]) and (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 >= min_us:
                    tot += float(r["Counter_Value"])
                    disp.add(r["Dispatch_Id"])
            sums[counter] = (tot, len(disp))
        except Exception as e:
            return None, f"{counter} pass failed: {type(e).__name__}"
        finally:
            shutil.rmtree(d, ignore_errors=True)
    (fe, n1), (wr, n2) = sums["FETCH_SIZE"], sums["WRITE_SIZE"]
    if not n1 or n1 != n2:
        return None, f"launch counts of the two passes differ ({n1}, {n2})"
    return (2 * fe + wr) * 1024 / n1, n1


XGMI_LINK_GB_S, XGMI_LINKS = 153.0, 7     # MI355X: 7 point-to-point xGMI links per GPU


def make_comm(args, rank, world, dev, dist):
    """The RCCL communicator of the C ABI (orca_comm_init_rank / orca_allgather) for BOTH sharded sections, or - together, on every rank -
    the torch.distributed fall-back.  Returns (comm or None, description)."""
    from orca_amd import dist as odist
    if world == 1:
        return None, "none (single rank)"
    collective = f"torch.distributed all_gather_into_tensor ({'RCCL' if dist.get_backend() == 'nccl' else dist.get_backend()})"
    if args.torch_collective:
        return None, collective
    ok, comm = 1, None
    try:
        comm = odist.AbiComm(dev)
    except Exception as e:      # fall back together (see below)
        ok = 0
        if rank == 0:
            print(f"bench: C-ABI RCCL communicator unavailable ({e}); using torch.distributed", file=sys.stderr)
    t = torch.tensor([ok], dtype=torch.int32, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    if int(t.item()) == 1:
        return comm, "RCCL all-gather through the C ABI (orca_comm_init_rank / orca_allgather)"
    if comm is not None:
        comm.close()
    return None, collective


def section_roofline(enc_strand_mb_per_rank, enc_ms, gather_bytes_received, gather_ms):
    """Per-rank Encoder rate against the 16-bit MFMA peak and the all-gather's receive rate against xGMI, for a sharded section."""
    tflop = ENC_FLOP_PER_BP * enc_strand_mb_per_rank * 1e6 / 1e12
    out = {"encoder": {"bound": "mfma", "achieved": round(tflop / (enc_ms * 1e-3), 1), "peak": PEAK_16BIT_MFMA_TFLOPS, "unit": "TFLOP/s",
                       "frac": round(tflop / (enc_ms * 1e-3) / PEAK_16BIT_MFMA_TFLOPS, 4), "algorithmic_tflop_per_rank": round(tflop, 2)}}
    if gather_bytes_received > 0 and gather_ms > 0:
        gbs = gather_bytes_received / (gather_ms * 1e-3) / 1e9
        out["allgather"] = {"bound": "xgmi", "achieved": round(gbs, 1), "unit": "GB/s received per rank", "bytes_received_per_rank": int(gather_bytes_received),
                            "peak_one_link": XGMI_LINK_GB_S, "peak_all_links": XGMI_LINK_GB_S * XGMI_LINKS, "frac_of_all_links": round(gbs / (XGMI_LINK_GB_S * XGMI_LINKS), 4)}
    return out


def encoder_kernels_of(dev, net0, codes, reverse, lo, hi, L):
    """Which kernel families ONE rank-local Encoder call runs on (launch counters of the C ABI's context, orca_ctx_launch_counts): the short last
    stages of a small shard move to conv_small.h (rows of <= 2 048 positions) - another fp32 summation order than the whole window's kernels."""
    from orca_amd import engine
    ctx = engine.get_context(dev)
    c0 = ctx.launch_counts()
    net0.forward_codes(codes, reverse=reverse, bin_lo=lo, bin_hi=hi)
    torch.cuda.synchronize(dev)
    c1 = ctx.launch_counts()
    b0, b1 = max(0, lo * 4000 - 112000), min(L, hi * 4000 + 112000)
    return {"bins": [int(lo), int(hi)], "stage7_positions_with_halo": int((b1 - b0) // 4000),
            "launches": {k: c1[k] - c0[k] for k in ("planar", "conv_bf16s", "conv_small")},
            "stage7_kernel": "conv_small.h" if c1["conv_small"] > c0["conv_small"] else "conv_bf16s.h"}


def projection(n1_ms, enc_ms, tail_ms, n, units_tails=2, tail_b1_factor=0.6):
    """PROJECTED (not measured) time of an N-rank job from the N = 1 phases of this run: Encoder / N (the 224 kb halo per shard is < 3 % at
    8 ranks) + one unit's tail (a rank runs one strand's maps at B = 1: ~0.6 of the two-strand batch, tools/time_decoder.py) + ~0.3 ms of
    collectives.  The tail does not shard - it is the serial fraction."""
    ms = enc_ms / n + tail_ms * tail_b1_factor * (2.0 / units_tails) * max(1.0, units_tails / n) + 0.3      # a rank runs max(1, units / N) one-strand tails
    return {"n": n, "ms": round(ms, 2), "efficiency": round(n1_ms / (n * ms), 3), "projected": True}


def sharded_256mb(args, rank, world, dev, dist, comm=None, collective="none (single rank)"):
    """BASELINE config 4 / north star: the 256 Mb model with the Encoder's bins sharded over the ranks."""
    from orca_amd import dist as odist, engine, orca_models, orca_predict, synth
    L256 = 256_000_000
    model = orca_models.H1esc_256M(synthetic_seed=0)
    host_codes = synth.synth_base_codes(L256, seed=2)[None]                           # the SAME sequence on every rank ...
    total_bins = engine.encoder_num_bins(L256)
    lo, hi = odist.bin_range(total_bins, rank, world)
    if world > 1:      # ... of which a rank keeps only what its bins read: bin range +- 112 kb, once per strand (2 x 32 Mb at N = 8)
        wins = []
        for rev in (False, True):
            b0, b1 = engine.code_window_range(L256, lo, hi, reverse=rev)
            wins.append(engine.CodeWindow(torch.from_numpy(np.ascontiguousarray(host_codes[:, b0:b1])).to(dev), b0, L256))
    else:
        full = torch.from_numpy(host_codes).to(dev)
        wins = [full, full]
    del host_codes
    enc = odist.ShardedEncoder(model.net0, comm=comm)
    chrlen = 138_368_000
    # the 8000 x 8000 float64 background resident in HBM: per-level, per-strand block means + log + reverse-strand flip run on the
    # device inside the timed tail (orca_block_mean_f64), exactly what genomepredict_256Mb computes (orca_predict.py:703, :724-737)
    de = orca_predict.Background256.to_device(synth.synth_normmat_256m(chrlen, seed=0), dev)
    mpos, wpos = 70_000_000, 128_000_000
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    acc = np.zeros(3)

    last = {}

    def one(timed):
        ev[0].record()
        ef = enc._local(lambda: model.net0.forward_codes(wins[0], reverse=False, **rng))      # rank-local bins, both strands
        er = enc._local(lambda: model.net0.forward_codes(wins[1], reverse=True, **rng))
        ev[1].record()
        enc0 = torch.cat([gather(ef), gather(er)], dim=0)
        last["enc0"] = enc0
        ev[2].record()
        # N = 1: both strands batched; N > 1: one strand per rank parity + one all-gather of the maps (dist.strand_parallel_cascade_256m)
        outs_ = [m[0] for m in odist.strand_parallel_cascade_256m(model, enc0, mpos, wpos, chrlen, de, comm=comm)]
        ev[3].record()
        if timed:
            torch.cuda.synchronize(dev)
            acc[:] += [ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3])]
        return outs_

    rng = {"bin_lo": lo, "bin_hi": hi} if world > 1 else {}
    gather = (lambda part: odist.sharded_encode(lambda x, a, b: part, None, total_bins, None, comm)) if world > 1 else (lambda part: part)

    def sync():
        torch.cuda.synchronize(dev)
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize(dev)

    one(False)
    sync()
    t0 = time.perf_counter()
    for _ in range(args.sharded_steps):
        outs_ = one(True)
    sync()
    el = time.perf_counter() - t0
    parts = acc / args.sharded_steps
    if dist is not None:
        t = torch.tensor([el, parts[0], parts[1], parts[2]], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el, parts = float(t[0]), t[1:].cpu().numpy()
    chk = float(sum(float(o.double().sum()) for o in outs_))
    # parity of THIS run's result against the reference's own genomepredict_256Mb on this sequence / these weights / this position
    # with the REAL Encoder as net0 (tests/golden/G20_full256m.npz, tools/make_golden.py --full256m): the 4 maps and a column sample
    # of both strands' [128, 64000] encodings.  At N > 1 this checks the sharded path end to end (every rank holds the same result).
    parity = None
    g20 = os.path.join(ROOT, "tests", "golden", "G20_full256m.npz")
    if rank == 0 and os.path.exists(g20):
        g = np.load(g20)
        bins = torch.from_numpy(g["bins"]).to(dev)
        e_err = [float(np.abs(last["enc0"][k][:, bins].cpu().numpy().astype(np.float64) - g[f"enc_{k}_cols"]).max()) for k in range(2)]
        m_err, m_r = [], []
        for j, o in enumerate(outs_):
            a, b = o.cpu().numpy().astype(np.float64), g[f"pred_{j}"].astype(np.float64)
            m_err.append(float(np.abs(a - b).max()))
            m_r.append(float(np.corrcoef(a.ravel(), b.ravel())[0, 1]))
        parity = {"against": "tests/golden/G20_full256m.npz = the reference's genomepredict_256Mb (PyTorch CPU fp32, real Encoder as net0) on this sequence",
                  "encoder_max_abs_per_strand": [round(e, 8) for e in e_err], "encoder_columns_checked": int(bins.numel()),
                  "map_max_abs_per_level": [round(e, 8) for e in m_err], "map_pearson_min": round(min(m_r), 9), "tolerance": 1e-4,
                  "ok": bool(max(e_err + m_err) < 1e-4)}
    last.clear()
    ms = el / args.sharded_steps * 1e3
    # the N = 1 job inside this N-rank run (every rank runs it alone, no collective): what `efficiency_vs_n1` divides by
    n1_ms = ms
    if world > 1:
        full = torch.from_numpy(synth.synth_base_codes(L256, seed=2)[None]).to(dev)

        def one_local():
            e0 = torch.cat([enc._local(lambda: model.net0.forward_codes(full, reverse=False)), enc._local(lambda: model.net0.forward_codes(full, reverse=True))], dim=0)
            return odist.strand_parallel_cascade_256m(model, e0, mpos, wpos, chrlen, de, local_only=True)
        one_local()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        one_local()
        torch.cuda.synchronize(dev)
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        n1_ms = float(t[0]) * 1e3
        del full
    recv = 2 * (world - 1) * 128 * (-(-total_bins // world)) * 4 if world > 1 else 0
    return {"workload": "H1esc_256M-shaped model, one random 256 Mb sequence (replicated on every rank as 1 byte/base), both strands: Encoder bins "
                        f"sharded {total_bins}/{world} per rank (112 kb input halo, orca_modules.py:955-977), one all-gather of [1,128,{-(-total_bins // world)}] fp32 "
                        "per rank and strand, then Encoder2(64000 bins) -> Encoder3 -> 4 Decoders: both strands on the one rank at N = 1, one strand per rank parity at N > 1 "
                        "with one all-gather of the [4,1,250,250] maps, strand merge on every rank",
            "n_gpus": world, "steps": args.sharded_steps, "scaling": "strong", "collective": collective,
            "ms_per_step": round(ms, 2), "Mb_per_s": round(2 * 256 / (ms * 1e-3), 1),
            "encoder_ms_per_rank_max": round(float(parts[0]), 2), "allgather_ms_max": round(float(parts[1]), 3), "tail_ms_max": round(float(parts[2]), 2),
            "encoder_Mb_per_s": round(2 * 256 / (float(parts[0]) * 1e-3), 1), "n1_ms_same_run": round(n1_ms, 2), "efficiency_vs_n1": round(n1_ms / (world * ms), 4),
            "roofline": section_roofline(2 * 256 / world, float(parts[0]), recv, float(parts[1])), "maps_checksum": round(chk, 4), "parity": parity,
            "encoder_kernels_this_rank": encoder_kernels_of(dev, model.net0, wins[0], False, lo, hi, L256),
            "projection_n8": projection(n1_ms, float(parts[0]), float(parts[2]), 8) if world == 1 else None,
            "bins_this_rank": [int(lo), int(hi)], "sequence_bytes_on_this_rank": int(sum(w.codes.numel() if isinstance(w, engine.CodeWindow) else w.numel() for w in (wins if world > 1 else wins[:1])))}


def inst_rooflines(recs):
    """Per-kernel-instantiation HIP-event timings of the planar conv1d launches -> {name: {...}} (see main)."""
    groups = {}
    for cout, cin, tile, batch, n, ms, ksize in recs:
        g = groups.setdefault((cout, cin, tile, ksize), {"ms": 0.0, "launches": 0, "flop": 0.0, "bytes": 0.0})
        g["ms"] += ms
        g["launches"] += 1
        # a 17-tap launch is a composed linear pair Conv(cin->cout) - BN - Conv(cout->cout) - BN (orca_modules.py:811-816):
        # its ALGORITHMIC work is the pair's (SURVEY 8d counts the reference's convolutions)
        # (25 taps from the bases = conv1.a composed with lconv1: the launch carries conv1.a's 64 -> 64 work, lconv1's is on the 17-tap launch)
        g["flop"] += 2.0 * 9 * (cout * cout if ksize == 25 else cin * cout + (cout * cout if ksize == 17 else 0)) * n * batch
        # what the launch EXECUTES: a composed launch runs its 17 / 25 taps, not the pair's 2 x 9
        g["xflop"] = g.get("xflop", 0.0) + 2.0 * (25 * 4 * cout if ksize == 25 else (112 + 9 * 64 + 80) * 64 if tile == -15 else ksize * cin * cout) * n * batch
        # x elements in + out; bytes per element applied per arithmetic below.  (tile -15 = stage 1 in one kernel from the bases, conv_stage1.h:
        # 1 byte per base in, 64 channels x n / 4 pooled positions x 2 B out = 33 B per position, whatever `cin` says - it is recorded as 128 so
        # that the FLOP line above counts both of the stage's 64 -> 64 convs)
        g["bytes"] += (16.5 if tile == -15 else float(cin + cout)) * n * batch
    PREC = {0: ("f32", "conv1d_k9_kernel", PEAK_F32_MFMA_TFLOPS, 1, 4), 1: ("bf16", "conv1d_k9_bf16s_kernel", PEAK_16BIT_MFMA_TFLOPS, 1, 4),
            2: ("bf16x2", "conv1d_k9_bf16s_kernel", PEAK_16BIT_MFMA_TFLOPS, 3, 4), 3: ("bf16x3", "conv1d_k9_bf16s_kernel", PEAK_16BIT_MFMA_TFLOPS, 6, 4),
            4: ("f16x2", "conv1d_k9_bf16s_kernel", PEAK_16BIT_MFMA_TFLOPS, 3, 4),
            5: ("f16x2", "conv1d_k9_p16_kernel", PEAK_16BIT_MFMA_TFLOPS, 3, 4), 6: ("bf16", "conv1d_k9_p16_kernel", PEAK_16BIT_MFMA_TFLOPS, 1, 2),
            7: ("f16x2", "conv1d_k9_ws_kernel", PEAK_16BIT_MFMA_TFLOPS, 3, 4), 8: ("bf16", "conv1d_k9_ws_kernel", PEAK_16BIT_MFMA_TFLOPS, 1, 2),
            9: ("f16x2", "conv1d_k9_p16w1_kernel", PEAK_16BIT_MFMA_TFLOPS, 3, 4), 10: ("bf16", "conv1d_k9_p16w1_kernel", PEAK_16BIT_MFMA_TFLOPS, 1, 2),
            12: ("f16x2", "conv1d_k9_p16p5_kernel", PEAK_16BIT_MFMA_TFLOPS, 3, 4), 13: ("bf16", "conv1d_k9_p16p5_kernel", PEAK_16BIT_MFMA_TFLOPS, 1, 2), 14: ("f16x2", "conv1d_k9_p16x_kernel", PEAK_16BIT_MFMA_TFLOPS, 3, 4),
            15: ("bf16", "conv1d_stage1_b16_kernel[conv1.a o lconv1 produced in LDS + conv1.b + lout1]", PEAK_16BIT_MFMA_TFLOPS, 1, 2)}
    inst = {}
    for (cout, cin, tile, ksize), g in groups.items():
        prec = -tile if tile < 0 else 0
        pname, kname, peak, nprod, bpe = PREC[prec]
        if ksize == 17:
            kname = "conv1d_first_mfma_p16_kernel[17 taps: composed lconv1]" if cin == 4 else kname + "[17 taps: composed pair]"
        elif ksize == 25:
            kname = "conv1d_first_mfma_p16_kernel[25 taps: conv1.a o lconv1]"
        key = f"{kname}<cout={cout},{pname}>" if prec else f"{kname}<cout={cout},kc={4 if cin == 4 else 8},tile={tile}>"
        d = inst.setdefault(key, {"ms": 0.0, "launches": 0, "flop": 0.0, "xflop": 0.0, "bytes": 0.0, "peak": peak, "nprod": nprod, "arith": pname})
        for k in ("ms", "launches", "flop", "xflop"):
            d[k] += g[k]
        d["bytes"] += g["bytes"] * bpe
    return inst


def config3_section(dev):
    """BASELINE.json configs[2]: HFF-shaped 32 Mb model, batch of 8 random 32 Mb sequences, throughput mode - Encoder on single bf16
    planes (plain bf16 operands, one MFMA product), Decoders on single fp16 planes (2 B/element end to end; the residual stream keeps 11
    significant bits), module-level forward of the forward strand (`genomepredict` keeps only batch row 0, orca_predict.py:514-523)."""
    from orca_amd import engine, orca_models, orca_predict as P, synth
    seed, mpos, wpos = 7, 17_234_567, 16_000_000                      # = tools/make_golden.py CONFIG3 / tests/test_gpu_config3.py
    hff = orca_models.Hff(synthetic_seed=seed)
    codes = torch.from_numpy(np.stack([synth.synth_base_codes(L_BP, seed=10 + b) for b in range(8)])).to(dev)
    de = {lv: torch.log(torch.from_numpy(hff.normmats[lv][None, None].astype(np.float32))).to(dev) for lv in hff.levels}
    hff.net0.precision = "bf16"
    for lv in hff.levels:
        hff.denets[lv].precision = "f16"
    hff.denet_1_pt.precision = "f16"

    def fwd():
        enc0 = hff.net0.forward_codes(codes)
        encs = dict(zip([1, 2, 4, 8, 16, 32], hff.net(enc0)))
        return P.run_cascade(hff, encs, [32, 16, 8, 4, 2, 1], lambda lv: lv, 8, [False], lambda lv, k, st: de[lv],
                             lambda lv, st, rev: P.zoom_index_32m(lv, st, mpos, wpos, rev), add_1m_level=1)[0]

    ctx = engine.get_context(dev)
    fwd()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(2):
        preds = fwd()
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / 2
    # the per-kernel roofline from a pass on ONE context (ORCA_BATCH_STREAMS=0): in the timed passes above the bf16 Encoder runs the batch as two
    # halves on two HIP streams (engine.batch_streams) and a launch's duration is its share of the chip, not the kernel
    os.environ["ORCA_BATCH_STREAMS"] = "0"
    try:
        fwd()
        torch.cuda.synchronize(dev)
        ctx.set_timing(True)
        t1 = time.perf_counter()
        fwd()
        torch.cuda.synchronize(dev)
        dt1 = time.perf_counter() - t1
        ctx.set_timing(False)
    finally:
        del os.environ["ORCA_BATCH_STREAMS"]
    inst = inst_rooflines(ctx.get_timing())
    flop = 8 * step_flops() / 2          # one strand per row
    out = {"workload": "HFF-shaped 32 Mb model, batch of 8 random 32 Mb sequences (seeds 10-17), forward strand, module-level forward: Encoder "
                       "precision 'bf16' (B16 planes, one product), Decoders 'f16' (single fp16 planes), 2 bytes per activation end to end",
           "batches_timed": 2, "s_per_batch": round(dt, 4), "Mb_per_s": round(8 * 32 / dt, 1), "maps_per_s": round(48 / dt, 1),
           "whole_batch_tflops": round(flop / dt, 1), "frac_of_2500TF_16bit_peak": round(flop / dt / PEAK_16BIT_MFMA_TFLOPS, 4),
           "encoder_batch_streams": "the Encoder's batch as two halves on two contexts / HIP streams (engine.batch_streams; same bits); ORCA_BATCH_STREAMS=0 = one context: "
                                    "s_per_batch_one_context (that pass also times the kernels of `roofline`)",
           "s_per_batch_one_context": round(dt1, 4), "Mb_per_s_one_context": round(8 * 32 / dt1, 1)}
    if inst:
        name, d = max(inst.items(), key=lambda kv: kv[1]["ms"])
        ach = d["flop"] / (d["ms"] * 1e-3) / 1e12
        xach = d["xflop"] * d["nprod"] / (d["ms"] * 1e-3) / 1e12
        out["roofline"] = {"kernel": name, "bound": "hbm+mfma", "achieved": round(ach, 1), "peak": d["peak"], "unit": "TFLOP/s", "frac": round(ach / d["peak"], 4),
                           "frac_is": "ALGORITHMIC FLOP (the reference's convolutions of the stage, SURVEY 8d) / HIP-event time / peak - not pipe use",
                           "executed_mfma_tflops": round(xach, 1), "executed_frac": round(xach / d["peak"], 4),
                           "executed_is": "matrix-instruction FLOP the launch really issues (composed taps, products per MAC) / time / peak = matrix-pipe use",
                           "algorithmic_hbm_GBps": round(d["bytes"] / (d["ms"] * 1e-3) / 1e9, 1), "hbm_frac_of_8TBps": round(d["bytes"] / (d["ms"] * 1e-3) / 8e12, 4),
                           "avg_launch_ms": round(d["ms"] / d["launches"], 4), "launches": d["launches"]}
    g17 = os.path.join(ROOT, "tests", "golden", "G17_config3.npz")
    if os.path.exists(g17):
        g = np.load(g17)
        errs, rs = [], []
        for b in (0, 5):
            for j, p in enumerate(preds):
                a, r = p[b, 0].cpu().numpy().astype(np.float64), g[f"maps_row{b}"][j].astype(np.float64)
                errs.append(float(np.abs(a - r).max()))
                rs.append(float(np.corrcoef(a.ravel(), r.ravel())[0, 1]))
        out["parity"] = {"against": "tests/golden/G17_config3.npz = rows 0 and 5 through the reference's own modules (PyTorch CPU fp32)",
                         "max_abs": round(max(errs), 5), "pearson_min": round(min(rs), 7), "stated_tolerance": {"max_abs": 0.1, "pearson": 0.99999},
                         "ok": bool(max(errs) < 0.1 and min(rs) > 0.99999)}
    del codes, preds, hff
    ctx.release_workspace()
    engine.context_pool(dev, 1).release_workspaces()      # the second context the bf16 Encoder ran half of the batch on
    torch.cuda.empty_cache()
    return out


def config5_section(dev, n_svs=256, n_unaligned=256):
    """BASELINE.json configs[4] on this rank: synthetic structural variants (orca_amd.sv.synth_svs: del / dup / inv, 10 kb - 5 Mb) x reference +
    alternative allele, 6 maps each, from a packed 40 Mb chromosome in HBM, through the screen of orca_amd/sv.py.
    TWO sets: the workload as SURVEY 8(d) defines it - log-uniform sizes, NO alignment (`n_unaligned` of the 1024; the top-level
    figures) - and rounds 3-5's set with every coordinate on the 4 kb grid (`aligned_4kb`, `n_svs` of the 1024).  The incremental encoder reuses a
    chromosome encoding per 4 kb PHASE: on the grid every window shares one phase (the chromosome's strands are encoded once, a window
    re-encodes only its ends and junctions); off the grid every window has a phase of its own - there the screen takes stages 1-3 of the
    Encoder (99 % of its work, covariant on a 16-base grid) from the chromosome's stage-3 cache (sv.Stage3Cache, round 6: 16 phases x 2 strands
    = 41 GB of HBM, built inside the timed region) and runs only the window's ends, junctions and stages 4-7; `whole_window_route` times the
    same variants without it (round 5's route off the grid: every window through the whole Encoder).  Per set, 8 variants are also run as the
    reference does it - two whole `genomepredict` calls each - for the speed-up and the agreement of the maps.
    Variants are independent: N GPUs take every N-th (replicas, no collective)."""
    from orca_amd import engine, orca_models, sv
    h1 = orca_models.H1esc(synthetic_seed=0)
    g = torch.Generator(device=dev).manual_seed(5)
    genome = torch.randint(0, 4, (40_000_000,), device=dev, generator=g, dtype=torch.uint8)

    def run(svs, n_full=8):
        sv.sv_screen([h1], genome, svs[:2], 40_000_000, min_uses=1)      # warm-up: workspace growth, both window shapes
        torch.cuda.synchronize(dev)
        stats = {}
        t0 = time.perf_counter()
        res = sv.sv_screen([h1], genome, svs[2:], 40_000_000, stats=stats)     # includes the chromosome encodings (4 on the grid) / the stage-3 cache (off it)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        n = len(svs) - 2
        n_full = min(n_full, n)
        sv.sv_screen([h1], genome, svs[2:3], 40_000_000, incremental=False)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        full = sv.sv_screen([h1], genome, svs[2:2 + n_full], 40_000_000, incremental=False)
        torch.cuda.synchronize(dev)
        dt_full = time.perf_counter() - t0
        diff = max(float(np.abs(res[i][a]["predictions"][0][j] - full[i][a]["predictions"][0][j]).max()) for i in range(n_full) for a in ("ref", "alt") for j in range(6))
        chk = float(sum(float(np.sum(r[a]["predictions"][0][0], dtype=np.float64)) for r in res.values() for a in ("ref", "alt")))
        return {"svs": n, "s_per_sv": round(dt / n, 4), "svs_per_s": round(n / dt, 2), "window_Mb_per_s": round(n * 2 * 2 * 32 / dt, 1),
                "projected_1024_svs_s_one_gpu": round(1024 * dt / n, 1),
                "encoder_bins_encoded_frac": round(stats["bins_encoded"] / stats["bins_total"], 4), "chromosome_encodings": stats["chromosome_encodings"],
                "whole_window_runs": stats.get("whole_window_runs"), "stage3_cache": stats.get("stage3_cache"),
                "as_the_reference_does_it": {"svs": n_full, "s_per_sv": round(dt_full / n_full, 4), "svs_per_s": round(n_full / dt_full, 2),
                                             "what": "two whole genomepredict calls per variant (every window through the whole Encoder, decoders at B = 2)"},
                "speedup": round((dt_full / n_full) / (dt / n), 2), "max_abs_vs_whole_window_encoding": diff,
                "kinds": "".join(v.kind[0] for v in svs[2:]), "level32_maps_checksum": round(chk, 3)}

    una = sv.synth_svs(n_unaligned + 2, 40_000_000)
    out = run(una)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    sv.sv_screen([h1], genome, una[2:34], 40_000_000, stage3=False)      # round 5's route off the grid: every window through the whole Encoder
    torch.cuda.synchronize(dev)
    out["whole_window_route"] = {"svs": 32, "svs_per_s": round(32 / (time.perf_counter() - t0), 2),
                                 "what": "the same screen without the stage-3 cache (stage3=False): every window of an off-grid variant encoded whole, decoders batched"}
    out = {"workload": f"{n_unaligned} of the 1024 synthetic SVs AS SURVEY 8(d) DRAWS THEM (log-uniform size, arbitrary base positions: align = 1) x (reference + "
                       "alternative allele) x 6 maps of a 32 Mb window (both strands), from a packed 40 Mb chromosome in HBM, through orca_amd.sv.sv_screen: off the 4 kb "
                       "grid every window keeps its own phase (as the reference's windows do, orca_predict.py:1613): stages 1-3 of the Encoder come from the "
                       "chromosome's stage-3 cache (16 phases x 2 strands, built inside the timed region), a window runs its ends, junctions and stages 4-7; ref + alt "
                       "of TWO variants are decoded as one batch of 8 maps per level", "coordinates": "unaligned (align=1)", **out}
    out["aligned_4kb"] = {"workload": f"{n_svs} of the 1024 with every coordinate rounded down to the 4 kb grid (synth_svs(align=4000): rounds 3-5's set - the incremental "
                                      "screen's best case: chromosome encoded once per strand and phase, windows re-encode ends + junctions only)",
                          "coordinates": "4 kb-aligned (align=4000)", **run(sv.synth_svs(n_svs + 2, 40_000_000, align=4000))}
    out["note"] = ("samples of the 1024: the whole screen on one GPU is profiles/r06_config5_1024.json (tools/run_configs.py config5_1024, both sets); per-variant time "
                   "varies with the variant's size and kind, so 64-, 256- and 1024-variant figures differ by a few per cent - and by +-2 % from box to box")
    del genome, h1
    engine.get_context(dev).release_workspace()
    torch.cuda.empty_cache()
    return out


def sharded_32mb(args, rank, world, dev, dist, comm, collective, n_models=1):
    """Strong scaling of the HEADLINE workload (one 32 Mb window, both strands, H1-ESC-shaped model) as ONE job (dist.units_sharded_32m):
    units = (model, strand) - independent until the strand merge -, a unit's Encoder sharded further by bins, ONE all-gather of the
    encodings, the units' tails one per rank (from 2 x units ranks on their independent `+ denet_1_pt` term on the next ranks), ONE
    all-gather of the maps.  n_models = 2: the reference's default call (orca_predict.py:231, models=["h1esc","hff"]): four independent
    tails, half the serial fraction per model from 4 ranks on.  N = 1: everything here."""
    from orca_amd import dist as odist, engine, orca_models, synth
    U = 2 * n_models
    if world > 1 and (world % U if world >= U else U % world):
        return {"skipped": f"{U} (model, strand) units need a multiple or a divisor of {U} ranks, got {world}"}
    models = [orca_models.H1esc(synthetic_seed=0)] + ([orca_models.Hff(synthetic_seed=1)] if n_models == 2 else [])
    host_codes = synth.synth_base_codes(L_BP, seed=1)[None]                               # = the replica-mode sequence of rank 0 (G8's)
    total = engine.encoder_num_bins(L_BP)
    full = None
    if world > 1:
        plan = odist.unit_plan(U, total, rank, world)[0]
        if len(plan) == 1:          # a rank keeps only the bases its bins read (+- 112 kb)
            u, lo, hi = plan[0]
            b0, b1 = engine.code_window_range(L_BP, lo, hi, reverse=bool(u & 1))
            codes = engine.CodeWindow(torch.from_numpy(np.ascontiguousarray(host_codes[:, b0:b1])).to(dev), b0, L_BP)
        else:
            codes = torch.from_numpy(host_codes).to(dev)
        full = codes if not isinstance(codes, engine.CodeWindow) else torch.from_numpy(host_codes).to(dev)
    else:
        codes = torch.from_numpy(host_codes).to(dev)
    del host_codes
    distencs = [{lv: torch.log(torch.from_numpy(m.normmats[lv][None, None].astype(np.float32))).to(dev) for lv in m.levels} for m in models]
    mpos, wpos = L_BP // 2 + 1234567, L_BP // 2

    def sync():
        torch.cuda.synchronize(dev)
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize(dev)

    def timed(fn, steps):
        fn(None)
        fn(None)
        sync()
        phases = np.zeros(4)
        t0 = time.perf_counter()
        for _ in range(steps):
            marks = []
            outs = fn(marks)
            torch.cuda.synchronize(dev)
            ev = dict(marks)
            phases += [ev["start"].elapsed_time(ev["encode"]), ev["encode"].elapsed_time(ev["gather"]), ev["gather"].elapsed_time(ev["tails"]),
                       ev["tails"].elapsed_time(ev["maps"])]
        sync()
        el = (time.perf_counter() - t0) / steps
        t = torch.tensor([el] + list(phases / steps), dtype=torch.float64, device=dev)
        if dist is not None:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return outs, float(t[0]), t[1:].cpu().numpy()

    steps = args.sharded_steps * 2
    outs, el, ph = timed(lambda marks: odist.units_sharded_32m(models, codes, mpos, wpos, distencs, comm=comm, marks=marks), steps)
    n1 = el
    if world > 1:       # the N = 1 job inside this run (every rank alone, no collective)
        _, n1, _ = timed(lambda marks: odist.units_sharded_32m(models, full, mpos, wpos, distencs, local_only=True, marks=marks), 2)
    shards = max(1, world // U)
    width = -(-total // shards)
    units_here = max(1, U // world)
    recv = (world - 1) * units_here * 128 * width * 4 if world > 1 else 0
    out = {"workload": f"ONE job: {n_models} H1-ESC-shaped 32Mb model(s), one random 32 Mb sequence, both strands - {U} (model, strand) units x {shards} Encoder bin "
                       f"shard(s) per unit, one all-gather of the [1,128,{width}] encodings, the units' tails one per rank, one all-gather of the [6,1,250,250] maps, "
                       "strand merge on every rank", "n_gpus": world, "models": n_models, "scaling": "strong", "collective": collective, "steps": steps,
           "ms_per_step": round(el * 1e3, 3), "Mb_per_s": round(n_models * 2 * 32 / el, 1),
           "encoder_ms_per_rank_max": round(float(ph[0]), 3), "allgather_ms_max": round(float(ph[1]), 3), "tail_ms_max": round(float(ph[2]), 3),
           "map_gather_ms_max": round(float(ph[3]), 3), "n1_ms_same_run": round(n1 * 1e3, 3), "efficiency_vs_n1": round(n1 / (world * el), 4),
           "roofline": section_roofline(n_models * 2 * 32 / world, float(ph[0]), recv, float(ph[1])),
           "maps_checksum": round(float(sum(float(o.double().sum()) for mo in outs for o in mo)), 4)}
    u0, lo0, hi0 = (odist.unit_plan(U, total, rank, world)[0] if world > 1 else [(0, 0, total)])[0]
    out["encoder_kernels_this_rank"] = dict(encoder_kernels_of(dev, models[u0 // 2].net0, codes, bool(u0 & 1), lo0, hi0, L_BP), unit=int(u0))
    out["sequence_bytes_on_this_rank"] = int(codes.codes.numel() if isinstance(codes, engine.CodeWindow) else codes.numel())
    if world == 1:
        out["projection_n8"] = projection(el * 1e3, float(ph[0]), float(ph[2]), 8, units_tails=U)
    g8 = os.path.join(ROOT, "tests", "golden", "G8_full32m.npz")
    if rank == 0 and os.path.exists(g8):
        g = np.load(g8)
        errs = [float(np.abs(o[0].cpu().numpy().astype(np.float64) - g[f"pred_{j}"]).max()) for j, o in enumerate(outs[0])]
        out["parity"] = {"against": "tests/golden/G8_full32m.npz (the reference's genomepredict on this sequence; model 0)", "max_abs_per_level": [round(e, 8) for e in errs],
                         "tolerance": 1e-4, "ok": bool(max(errs) < 1e-4)}
    del models, outs
    engine.get_context(dev).release_workspace()
    torch.cuda.empty_cache()
    return out


def rccl_log_tail(nbytes=1500):
    """What RCCL printed at NCCL_DEBUG=WARN (N > 1 runs set NCCL_DEBUG_FILE): the tail of this process's log, for the error fields."""
    import glob
    txt = ""
    for f in sorted(glob.glob("/tmp/orca_bench_rccl_*.log")):
        try:
            txt += open(f).read()[-nbytes:]
        except OSError:
            pass
    return txt[-nbytes:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-traffic", action="store_true", help="do not measure the dominant kernel's HBM traffic with rocprofv3 counter passes in child processes (about a minute); the committed profiles/pmc_traffic.json is quoted instead")
    ap.add_argument("--cpu-sample-only", action="store_true", help="CPU baseline from the 8 Mb sample alone (extrapolated), as in rounds 1-4: saves a minute")
    ap.add_argument("--cpu-full-strand", action="store_true", help="only: time the CPU baseline on the WHOLE 32 Mb strand (about a minute of CPU), print it and exit")
    ap.add_argument("--seq-mb", type=int, default=32, help="debug only: shorter sequence (invalidates the metric)")
    ap.add_argument("--float-input", action="store_true", help="keep the strands as float32 [1,4,L] views (the reference's input form)")
    ap.add_argument("--no-sharded", action="store_true", help="skip the 256 Mb sharded-encoder section")
    ap.add_argument("--no-configs", action="store_true", help="skip the config 3 (B = 8 bf16) and config 5 (SV screen) sections")
    ap.add_argument("--sharded-timeout", type=float, default=420.0, help="N > 1: seconds the 256 Mb sharded section (and the final barrier) may take before the line is printed without it")
    ap.add_argument("--sharded-steps", type=int, default=3)
    ap.add_argument("--torch-collective", action="store_true", help="256 Mb section: torch.distributed all-gather instead of the C ABI's RCCL communicator")
    ap.add_argument("--full", action="store_true", help="also run every section beside the headline figure (module docstring); the --no-* and "
                                                        "--sharded-* options above select among them")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the six maps of the last timed step (rank 0) as DIR/pred_<j>.npy, float32")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.cpu_full_strand:
        print(json.dumps({"cpu_baseline_full_strand": cpu_baseline(0, L_BP)}))
        return
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs torch.distributed.run with {args.gpus} ranks (WORLD_SIZE={world})")
    if os.environ.get("ORCA_BENCH_ONE_DEVICE"):      # test hook: all ranks on cuda:0 (control-flow check of the N > 1 path on a 1-GPU box;
        local_rank = 0                               # needs ORCA_BENCH_BACKEND=gloo - RCCL refuses two ranks on one device)
        os.environ.setdefault("ORCA_RANKS_PER_DEVICE", str(world))    # the Encoder sizes its chunks (workspace) for `world` ranks on this GPU
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        os.environ.setdefault("NCCL_DEBUG", "WARN")       # RCCL's own diagnostics go to a per-process file; their tail is quoted in `error` fields
        os.environ.setdefault("NCCL_DEBUG_FILE", "/tmp/orca_bench_rccl_%h_%p.log")
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("ORCA_BENCH_BACKEND", "nccl")
        dist.init_process_group(backend, **({"device_id": dev} if backend == "nccl" else {}))

    from orca_amd import engine, orca_models, orca_predict, synth
    engine_pack = engine.pack_sequence

    Lbp = args.seq_mb * 1_000_000
    model = orca_models.H1esc(synthetic_seed=0)
    # device-resident inputs: forward strand and reverse complement as [1,4,L] views of [1,L,4] storage
    seq = synth.synth_sequence(Lbp, seed=1 + rank)
    x_fwd = torch.from_numpy(seq).to(dev).transpose(1, 2)
    if args.float_input:
        strands = [x_fwd, torch.from_numpy(np.ascontiguousarray(seq[:, ::-1, ::-1])).to(dev).transpose(1, 2)]
    else:
        codes, packable = engine_pack(x_fwd)
        assert packable
        strands = [codes, codes]          # the reverse strand is read from the same buffer (index flip + complement)
        del x_fwd
    del seq
    distencs = {lv: torch.log(torch.from_numpy(model.normmats[lv][None, None].astype(np.float32))).to(dev)
                for lv in model.levels}
    mpos, wpos = Lbp // 2 + 1234567 * Lbp // 32_000_000, Lbp // 2
    ctx = engine.get_context(dev)

    def step():
        return [m[0] for m in orca_predict.cascade_32m(model, strands, mpos, wpos, [False, True], distencs, merge=True)[2]]

    def sync():
        torch.cuda.synchronize(dev)
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize(dev)

    for _ in range(args.warmup):
        step()
    sync()
    ctx.set_timing(args.full)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        outs = step()
    sync()
    elapsed = time.perf_counter() - t0
    ctx.set_timing(False)
    recs = ctx.get_timing()
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        os.makedirs(args.dump_outputs, exist_ok=True)
        for j, o in enumerate(outs):
            np.save(os.path.join(args.dump_outputs, f"pred_{j}.npy"), o.float().cpu().numpy())

    # ---- dominant kernel: per-instantiation HIP-event timings collected in the timed region
    inst = inst_rooflines(recs)
    roofline = None
    if inst:
        name, d = max(inst.items(), key=lambda kv: kv[1]["ms"])
        achieved = d["flop"] / (d["ms"] * 1e-3) / 1e12
        traffic = traffic_src = None
        tp = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tp):
            try:
                tj = json.load(open(tp))
                traffic, traffic_src = tj.get(name), tj.get("_source")
            except Exception:
                traffic = None
        tot_ms = sum(v["ms"] for v in inst.values())
        roofline = {"bound": "mfma", "kernel": name, "achieved": round(achieved, 2), "peak": d["peak"],
                    "unit": "TFLOP/s", "frac": round(achieved / d["peak"], 4), "traffic": traffic, "traffic_source": traffic_src,
                    "traffic_measured_in_run": False,     # replayed from the committed rocprofv3 --pmc passes of the same kernel (tools/profile_run.sh)
                    "arithmetic": d["arith"], "mfma_products_per_algorithmic_mac": d["nprod"],
                    "mfma_pipe_frac": round(achieved * d["nprod"] / d["peak"], 4),
                    "achieved_is": "ALGORITHMIC FLOP (the reference's convolutions, SURVEY 8d) / HIP-event time",
                    "executed_mfma_tflops": round(d["xflop"] * d["nprod"] / (d["ms"] * 1e-3) / 1e12, 2),
                    "executed_frac": round(d["xflop"] * d["nprod"] / (d["ms"] * 1e-3) / 1e12 / d["peak"], 4),
                    "executed_is": "16-bit matrix-instruction FLOP issued (taps as launched x products per MAC) / HIP-event time; executed_frac = matrix-pipe use",
                    "frac_of_f32_mfma_peak": round(achieved / PEAK_F32_MFMA_TFLOPS, 4),
                    "avg_launch_ms": round(d["ms"] / d["launches"], 4), "launches": d["launches"],
                    "flop_per_launch": d["flop"] / d["launches"], "algorithmic_bytes_per_launch": d["bytes"] / d["launches"],
                    "conv1d_time_share_of_step": round(tot_ms / (elapsed * 1e3), 4),
                    "all_conv1d_tflops": round(sum(v["flop"] for v in inst.values()) / (tot_ms * 1e-3) / 1e12, 2)}

    # the one HBM-bound kernel of the step: the 25-tap first-layer GEMM (conv1.a o lconv1 from the bases) writes 4 B per element of a
    # 64-channel tensor and reads 1 byte per base - algorithmic bytes / HIP-event time against the 8 TB/s HBM3E peak
    roofline_hbm = None
    f25 = [(n, ms) for cout, cin, tile, batch, n, ms, ksize in recs if ksize == 25 and ms > 0]
    if f25:
        byts = sum(n * (64 * 4 + 1) for n, _ in f25)
        tms = sum(ms for _, ms in f25)
        roofline_hbm = {"bound": "hbm", "kernel": "conv1d_first_mfma_p16_kernel<0,0,25> (conv1.a o lconv1: 25 taps from the bases + ReLU, P16 out)",
                        "achieved": round(byts / (tms * 1e-3) / 1e9, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(byts / (tms * 1e-3) / 8e12, 4),
                        "bytes_per_launch_algorithmic": byts / len(f25), "avg_launch_ms": round(tms / len(f25), 4), "launches": len(f25),
                        "traffic": None, "traffic_measured_in_run": False}
        try:
            roofline_hbm["traffic"] = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json"))).get("conv1d_first_mfma_p16_kernel<0,0,25>")
        except Exception:
            pass
    ms_per_step = elapsed / args.steps * 1e3
    mb_per_s = world * 2 * (Lbp / 1e6) * args.steps / elapsed
    enc_prec, dec_prec = model.net0.precision, model.denets[32].precision
    ARITH = {"f32": "exact fp32 MFMA", "f16x2": "fp32 emulated as 2 x fp16 split operands, 3 MFMA products, fp32 accumulate (22 significant operand bits)",
             "bf16x3": "fp32 emulated as 3 x bf16 split operands, 6 MFMA products, fp32 accumulate", "bf16": "plain bf16 operands, fp32 accumulate"}
    res = {
        "metric": "Mb of sequence encoded+decoded per second (32Mb H1-ESC-shaped model, both strands, 6 levels)",
        "value": round(mb_per_s, 3), "unit": "Mb/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": f"{enc_prec} | Encoder Conv1d stages 1-7: {enc_prec} = {ARITH[enc_prec]}; Decoder / Decoder_1m Conv2d: {dec_prec} = {ARITH[dec_prec]}; "
                 f"Encoder2 Conv1d: {getattr(model.net, 'precision', 'f32')} = {ARITH[getattr(model.net, 'precision', 'f32')]}; "
                 "1x1 heads, pools, upsampling, merges: fp32",
        "data": "synthetic",
        "config": {"workload": f"H1-ESC 32Mb model forward, single random {args.seq_mb}Mb sequence, fp32-class ({enc_prec} split operands on the 16-bit matrix "
                               "cores, see dtype; parity vs the reference's fp32 in `parity` with --full), both strands (genomepredict-equivalent, 1 model): "
                               "Encoder+Encoder2+6 Decoder+Decoder_1m per strand",
                   "sequence_bp": Lbp, "strands": 2, "levels": 6, "weights": "synthetic seed 0",
                   "input": "float32 [1,4,L] strands in HBM" if args.float_input else "1 byte/base packed sequence in HBM, both strands read from it",
                   "parallelism": f"replicas x{world} (independent 32 Mb windows, no data-path collective)" if world > 1 else "single GPU"},
        "contact_map_pixels_per_s": round(world * 2 * 6 * 62500 * args.steps / elapsed, 1),
        "step_tflop_algorithmic": round(step_flops() * Lbp / L_BP, 3) if Lbp == L_BP else None,
        "whole_step_tflops": round(world * step_flops() * args.steps / elapsed, 2) if Lbp == L_BP else None,
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(res), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    res["roofline"], res["roofline_hbm_bound_kernel"] = roofline, roofline_hbm

    # ---- parity of THIS run's maps against the reference's own output for the same sequence / weights / position (G8)
    g8 = os.path.join(ROOT, "tests", "golden", "G8_full32m.npz")
    if rank == 0 and Lbp == L_BP and os.path.exists(g8):
        g = np.load(g8)
        errs, rs = [], []
        for j, o in enumerate(outs):
            a, b = o.cpu().numpy().astype(np.float64), g[f"pred_{j}"].astype(np.float64)
            errs.append(float(np.abs(a - b).max()))
            rs.append(float(np.corrcoef(a.ravel(), b.ravel())[0, 1]))
        res["parity"] = {"against": "tests/golden/G8_full32m.npz = the reference's genomepredict (PyTorch CPU fp32) on this sequence, these weights, this zoom position",
                         "max_abs_per_level": [round(e, 8) for e in errs], "pearson_min": round(min(rs), 9), "tolerance": 1e-4,
                         "ok": bool(max(errs) < 1e-4)}

    # ---- opt-in mode: the reverse strand's Encoder on an auxiliary context beside the forward strand's (engine.strand_streams()).  NOT the
    # timed configuration: with two persistent launches sharing the chip a kernel's duration no longer measures the kernel, and `roofline`
    # above is defined on launches that have the chip to themselves.  Same kernels, same data: the maps must equal the timed region's.
    if world == 1 and Lbp == L_BP and not args.float_input:
        os.environ["ORCA_STRAND_STREAMS"] = "1"
        try:
            for _ in range(2):
                step()
            sync()
            t0 = time.perf_counter()
            for _ in range(5):
                outs2 = step()
            sync()
            t2 = (time.perf_counter() - t0) / 5
            res["concurrent_strands"] = {"what": "ORCA_STRAND_STREAMS=1 (opt-in): the two strands' Encoders on two HIP streams / contexts; 5 steps after the timed region",
                                         "ms_per_step": round(t2 * 1e3, 3), "Mb_per_s": round(2 * Lbp / 1e6 / t2, 2),
                                         "maps_equal_timed_region": bool(all(torch.equal(a, b) for a, b in zip(outs, outs2)))}
        finally:
            os.environ.pop("ORCA_STRAND_STREAMS", None)
            engine.context_pool(dev, 1).release_workspaces()

    # ---- the reference's CALL FORM: `genomepredict(sequence)` with the host float32 [1, 32e6, 4] array the reference's
    #      callers hand over (orca_predict.py:231-233, :324-337) - upload over PCIe, on-device pack, both strands, six levels, maps back on the
    #      host - and the reference's DEFAULT of two models (:231).  `value` above starts from packed bases resident in HBM; this is the
    #      PCIe-inclusive figure, timed in the same run.
    if world == 1 and Lbp == L_BP and not args.float_input and rank == 0:
        try:
            seq_host = synth.synth_sequence(Lbp, seed=1 + rank)
            hff2 = orca_models.Hff(synthetic_seed=1)
            o1 = orca_predict.genomepredict(seq_host, "chrS", mpos, wpos, models=[model])
            t0 = time.perf_counter()
            for _ in range(3):
                o1 = orca_predict.genomepredict(seq_host, "chrS", mpos, wpos, models=[model])
            t_one = (time.perf_counter() - t0) / 3
            orca_predict.genomepredict(seq_host, "chrS", mpos, wpos, models=[model, hff2])
            t0 = time.perf_counter()
            for _ in range(2):
                orca_predict.genomepredict(seq_host, "chrS", mpos, wpos, models=[model, hff2])
            t_two = (time.perf_counter() - t0) / 2
            same = bool(all(np.array_equal(np.asarray(p), o.cpu().numpy().reshape(np.asarray(p).shape)) for p, o in zip(o1["predictions"][0], outs)))
            res["reference_call_form"] = {"what": "orca_predict.genomepredict(host float32 [1,32000000,4], mchr, mpos, wpos, models=[H1esc]) - the reference's own call: "
                                                  "512 MB over PCIe per call, packed on the device, both strands, 6 levels, maps returned as numpy (wall clock, 3 calls)",
                                          "ms_per_call": round(t_one * 1e3, 2), "Mb_per_s": round(2 * Lbp / 1e6 / t_one, 2),
                                          "over_value_ms": round(t_one * 1e3 - ms_per_step, 2),
                                          "two_models_ms": round(t_two * 1e3, 2), "two_models_what": "the reference's default models=['h1esc','hff'] (orca_predict.py:231): one upload, two models",
                                          "maps_equal_timed_region": same}
            del seq_host, hff2, o1
        except Exception as e:
            res["reference_call_form"] = {"error": f"{type(e).__name__}: {e}"}

    # ---- the strict-fp32 readings of the same step (N = 1), each with its OWN parity against the reference's G8 on the full cascade:
    #      exact fp32 MFMA everywhere, and the range-safe arithmetic the fp16 guard falls back to (bf16x3 Encoders, fp32 Decoders)
    if world == 1 and Lbp == L_BP:
        mods = [model.net0, model.net] + [model.denets[lv] for lv in model.levels] + [model.denet_1_pt]
        old = [m.precision for m in mods]
        g8p = os.path.join(ROOT, "tests", "golden", "G8_full32m.npz")

        def parity_of(maps):
            if not os.path.exists(g8p):
                return None
            g = np.load(g8p)
            errs, rs = [], []
            for j, o in enumerate(maps):
                a, b = o.cpu().numpy().astype(np.float64), g[f"pred_{j}"].astype(np.float64)
                errs.append(float(np.abs(a - b).max()))
                rs.append(float(np.corrcoef(a.ravel(), b.ravel())[0, 1]))
            return {"against": "tests/golden/G8_full32m.npz (the reference's genomepredict, PyTorch CPU fp32)", "max_abs_per_level": [round(e, 8) for e in errs],
                    "pearson_min": round(min(rs), 9), "tolerance": 1e-4, "ok": bool(max(errs) < 1e-4)}

        for key, precs, nsteps in (("exact_f32", ["f32"] * len(mods), 2), ("bf16x3", ["bf16x3", "bf16x3"] + ["f32"] * (len(mods) - 2), 2)):
            for m, p_ in zip(mods, precs):
                m.precision = p_
            step(); sync()
            t0 = time.perf_counter()
            for _ in range(nsteps):
                o32 = step()
            sync()
            t32 = (time.perf_counter() - t0) / nsteps
            res[key] = {"arithmetic": "every module on the exact fp32 MFMA kernels (v_mfma_f32_32x32x2_f32)" if key == "exact_f32" else
                        "Encoder + Encoder2 on 3-way split bf16 (6 MFMA products, exact for every finite fp32), Decoders on the exact fp32 kernels - what the fp16-range guard falls back to",
                        "ms_per_step": round(t32 * 1e3, 2), "Mb_per_s": round(2 * Lbp / 1e6 / t32, 2), "whole_step_tflops": round(step_flops() / t32, 2),
                        "frac_of_157TF_fp32_mfma_peak": round(step_flops() / t32 / PEAK_F32_MFMA_TFLOPS, 4), "parity": parity_of(o32)}
        for m, p_ in zip(mods, old):
            m.precision = p_
        del o32
    # ---- the Decoders' share: one Decoder forward (118 Conv2d, both strands batched as in the step) under HIP events
    if world == 1 and Lbp == L_BP:
        dec = model.denets[16]
        for Bd in (2, 4):
            xd = torch.from_numpy((np.random.RandomState(31).rand(Bd, 128, 250) * 0.5).astype(np.float32)).to(dev)
            yd = torch.from_numpy(np.random.RandomState(32).randn(Bd, 1, 125, 125).astype(np.float32)).to(dev)
            ded = distencs[16].expand(Bd, -1, -1, -1)
            dec(xd, ded, yd)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            for _ in range(10):
                dec(xd, ded, yd)
            e1.record()
            torch.cuda.synchronize(dev)
            dms = e0.elapsed_time(e1) / 10
            dtf = Bd * DEC_TFLOP["withy"] / (dms * 1e-3)
            if Bd == 2:
                res["roofline_decoder"] = {"kernel": "conv2d_3x3_m16q_kernel<32|64,2,1> (dilation 1-8, 72 launches: four-row tiles, both strands in one round) + conv2d_dblock_kernel<2,1> (dilation 16-64, 12 launches of 4 convs) "
                                                     "= one Decoder forward with y at B = 2 (the two strands)", "bound": "mfma", "ms_per_forward": round(dms, 3),
                                           "achieved": round(dtf, 1), "peak": PEAK_16BIT_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(dtf / PEAK_16BIT_MFMA_TFLOPS, 4),
                                           "mfma_products_per_algorithmic_mac": 3, "mfma_pipe_frac": round(3 * dtf / PEAK_16BIT_MFMA_TFLOPS, 4),
                                           "decoders_share_of_step": round(7 * dms / ms_per_step, 3),
                                           "mfma_busy_source": "profiles/r06_pmc_dec_sq.txt (SQ_VALU_MFMA_BUSY_CYCLES / SIMD cycles per kernel)"}
            else:      # the SV drivers' and the screen's batch: ref + alt x two strands (workgroups of one resident round walk the maps)
                res["roofline_decoder"]["batch_of_4"] = {"ms_per_forward": round(dms, 3), "achieved": round(dtf, 1), "frac": round(dtf / PEAK_16BIT_MFMA_TFLOPS, 4),
                                                         "ms_per_map": round(dms / 4, 3)}
        # config 3's Decoder mode: ONE fp16 plane per map (2 B/element, one MFMA product per MAC), batch of 8
        old_prec, dec.precision = dec.precision, "f16"
        try:
            xd = torch.from_numpy((np.random.RandomState(31).rand(8, 128, 250) * 0.5).astype(np.float32)).to(dev)
            yd = torch.from_numpy(np.random.RandomState(32).randn(8, 1, 125, 125).astype(np.float32)).to(dev)
            ded = distencs[16].expand(8, -1, -1, -1)
            dec(xd, ded, yd)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            for _ in range(10):
                dec(xd, ded, yd)
            e1.record()
            torch.cuda.synchronize(dev)
            dms = e0.elapsed_time(e1) / 10
            dtf = 8 * DEC_TFLOP["withy"] / (dms * 1e-3)
            res["roofline_decoder"]["single_plane_b8"] = {"precision": "f16 (one fp16 plane per map; config 3's Decoders)", "ms_per_forward": round(dms, 3), "ms_per_map": round(dms / 8, 3),
                                                          "achieved": round(dtf, 1), "frac": round(dtf / PEAK_16BIT_MFMA_TFLOPS, 4), "mfma_products_per_algorithmic_mac": 1}
        finally:
            dec.precision = old_prec
        del xd, yd, ded
    # ---- fp16-range evidence without the published checkpoints (tools/range_headroom.py): how far this model's activations are
    #      from the f16x2 arithmetic's range guard, and the synthetic-weight gain at which the guard fires per network
    if world == 1 and Lbp == L_BP and not args.no_configs and not args.float_input:
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import range_headroom
            hr = range_headroom.headroom(model, codes)
            sweep = range_headroom.trip_sweep(dev=dev)
            hr["trip_gain_synthetic_weights"] = {k: v["trip_gain"] for k, v in sweep.items() if isinstance(v, dict)}
            hr["worst_rel_err_vs_f32_up_to_the_trip"] = max(r["rel_err_vs_f32"] for v in sweep.values() if isinstance(v, dict) for r in v["rows"])
            hr["trip_sweep"] = {k: [[r["gain"], r["max_abs_activation"], r["guard_fired"]] for r in v["rows"]] for k, v in sweep.items() if isinstance(v, dict)}
            hr["cost_of_a_tripped_guard"] = ("the module redoes its forward in the range-safe arithmetic: a whole step in it is `bf16x3.ms_per_step` "
                                             "(2.4 x the f16x2 step), never a wrong result")
            res["fp16_headroom"] = hr
        except Exception as e:
            res["fp16_headroom"] = {"error": f"{type(e).__name__}: {e}"}
    strands = outs = codes = None
    engine.get_context(dev).release_workspace()
    torch.cuda.empty_cache()
    # ---- BASELINE configs 3 and 5 on this GPU (N = 1), outside the timed region
    if world == 1 and Lbp == L_BP and not args.no_configs:
        for name, fn in (("config3", config3_section), ("config5", config5_section)):
            try:
                res[name] = fn(dev)
            except Exception as e:
                res[name] = {"error": f"{type(e).__name__}: {e}"}

    # ---- north star / config 4: 256 Mb model, Encoder bins sharded over the ranks + one RCCL all-gather per strand
    #      (N > 1: under a watchdog - a collective that never completes must not take the replica-mode line above down with it)
    printed = threading.Event()

    def emit():
        if rank == 0 and not printed.is_set():
            printed.set()
            # the driver's record keeps `roofline`, `config`, `cpu_baseline` and the scalar fields: the other sections' headline numbers ride in those
            def pick(sec, *path):
                d = res.get(sec)
                for k in path:
                    d = d.get(k) if isinstance(d, dict) else None
                return d
            if isinstance(res.get("roofline"), dict):
                res["roofline"]["other_readings"] = {
                    "exact_f32_ms_per_step": pick("exact_f32", "ms_per_step"), "exact_f32_frac_of_157TF": pick("exact_f32", "frac_of_157TF_fp32_mfma_peak"),
                    "bf16x3_ms_per_step": pick("bf16x3", "ms_per_step"),
                    "decoder_ms_per_forward_b2": pick("roofline_decoder", "ms_per_forward"), "decoder_frac": pick("roofline_decoder", "frac"),
                    "decoder_mfma_pipe_frac": pick("roofline_decoder", "mfma_pipe_frac"),
                    "decoder_single_plane_b8_ms": pick("roofline_decoder", "single_plane_b8", "ms_per_forward"),
                    "hbm_bound_kernel_frac": pick("roofline_hbm_bound_kernel", "frac"),
                    "config3_executed_frac": pick("config3", "roofline", "executed_frac")}
            res["config"]["other_configs_in_this_line"] = {
                "reference_call_form_ms": pick("reference_call_form", "ms_per_call"), "two_models_ms": pick("reference_call_form", "two_models_ms"),
                "config3_strand_Mb_per_s": pick("config3", "Mb_per_s"), "config3_parity_ok": pick("config3", "parity", "ok"),
                "config5_unaligned_svs_per_s": pick("config5", "svs_per_s"), "config5_aligned_4kb_svs_per_s": pick("config5", "aligned_4kb", "svs_per_s"),
                "sharded_256mb_ms": pick("sharded_256mb", "ms_per_step"), "parity_ok": pick("parity", "ok"),
                "fp16_headroom": pick("fp16_headroom", "min_headroom"), "fp16_trip_gain": pick("fp16_headroom", "trip_gain_synthetic_weights")}
            print(json.dumps(res), flush=True)

    def bail():
        res.setdefault("sharded_256mb", {"error": f"no completion within {args.sharded_timeout} s (rank {rank}); the replica-mode figures of this line are unaffected",
                                         "rccl_log_tail": rccl_log_tail()})
        emit()
        os._exit(0)

    dog = None
    if world > 1:
        dog = threading.Timer(args.sharded_timeout, bail)
        dog.daemon = True
        dog.start()
    if not args.no_sharded and Lbp == L_BP:
        comm, collective = None, "none (single rank)"
        try:
            comm, collective = make_comm(args, rank, world, dev, dist)
        except Exception as e:
            res["sharded_comm_error"] = f"{type(e).__name__}: {e}"
        for name, fn in (("sharded_256mb", lambda: sharded_256mb(args, rank, world, dev, dist, comm, collective)),
                         ("sharded_32mb", lambda: sharded_32mb(args, rank, world, dev, dist, comm, collective, 1)),
                         ("sharded_32mb_two_models", lambda: sharded_32mb(args, rank, world, dev, dist, comm, collective, 2))):
            try:
                res[name] = fn()
            except Exception as e:      # reported, not fatal: the ranks may be out of step now, the watchdog covers the rest
                res[name] = {"error": f"{type(e).__name__}: {e}", "rccl_log_tail": rccl_log_tail() if world > 1 else ""}
        if comm is not None:
            comm.close()
        res["strong_scaling"] = {k: {f: res[k].get(f) for f in ("n_gpus", "ms_per_step", "Mb_per_s", "n1_ms_same_run", "efficiency_vs_n1")}
                                 for k in ("sharded_256mb", "sharded_32mb", "sharded_32mb_two_models") if isinstance(res.get(k), dict) and "ms_per_step" in res[k]}
        res["strong_scaling"]["note"] = ("`value` above is replica mode (independent 32 Mb windows per rank, weak scaling, no collective); these are the north star's "
                                         "one-job curves: efficiency_vs_n1 = the N = 1 time measured in THIS run / (N x this time).  Only the ENCODER shards: the tail "
                                         "(Encoder2 -> decoder levels, one dependent chain per strand) is the serial fraction.  256 Mb: the Encoder is 97 % of the job, "
                                         "so the curve is near-linear (projected 0.85-0.92 at N = 8: `projection_n8`); the 32 Mb window is TAIL-BOUND by design - 50 ms "
                                         "of Encoder against 15 ms of tails at N = 1 leaves ~6 + 9 ms at N = 8, efficiency ~0.5-0.6 (one model; two models have four "
                                         "tails: better from 4 ranks on).  Near-linear scaling is a property of the 256 Mb encoder only.")
        if world == 1:
            res["strong_scaling"]["projection_n8"] = {k: res[k].get("projection_n8") for k in ("sharded_256mb", "sharded_32mb", "sharded_32mb_two_models")
                                                      if isinstance(res.get(k), dict)}
    if rank == 0 and world == 1 and not args.no_traffic and Lbp == L_BP and isinstance(res.get("roofline"), dict):
        # (this process holds no workspace any more; the child processes run the Encoder on their own)
        engine.get_context(dev).release_workspace()
        torch.cuda.empty_cache()
        got, info = measure_traffic_in_run(res["roofline"]["kernel"])
        if got is not None:
            res["roofline"].update({"traffic": got, "traffic_measured_in_run": True, "traffic_launches": info,
                                    "traffic_source": "rocprofv3 --kernel-trace --pmc FETCH_SIZE | WRITE_SIZE (two passes) over tools/prof_encoder.py 32 f16x2 1 codes, child processes of this run",
                                    "traffic_committed": res["roofline"].get("traffic"),
                                    "traffic_over_algorithmic": round(got / res["roofline"]["algorithmic_bytes_per_launch"], 3)})
        else:
            res["roofline"]["traffic_not_measured_because"] = info
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        # the reference's CPU path on ONE WHOLE 32 Mb strand, timed on this box in this run (north star; about a minute on the 16-core quota),
        # and - first, while the cores are cool - the 8 Mb sample of rounds 1-4 scaled x4 (kept as a second field: the two differ by what the
        # host does under sustained load)
        sample = cpu_baseline(0)
        res["cpu_baseline"] = cpu_baseline(0, L_BP) if not args.cpu_sample_only else sample
        res["cpu_baseline"]["sample_8mb_scaled"] = {k: sample[k] for k in ("value", "unit", "extrapolated", "sample")}
        res["speedup_vs_cpu"] = round(res["value"] / world / res["cpu_baseline"]["value"], 1)
    emit()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if dog is not None:
        dog.cancel()


if __name__ == "__main__":
    main()
