"""-m gpu: the multi-GPU exchange.  On a 1-GPU box only the single-rank communicator runs (RCCL is
loaded, a communicator of one rank is created through the C ABI, the all-gather is a copy); with >= 2 GPUs a
torch.distributed.run world of 2 checks the sharded Encoder (bin ranges + ONE all-gather, orca_predict.py:675-683 /
orca_modules.py:955-977) against the unsharded one, through both the C ABI's RCCL communicator and torch.distributed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from tests import standins

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_communicator_single_rank(cuda):
    from orca_amd import dist as D
    comm = D.AbiComm(cuda, world=1, rank=0)
    x = torch.from_numpy(np.random.RandomState(0).randn(2, 128, 77).astype(np.float32)).to(cuda)
    y = comm.all_gather(x)
    torch.cuda.synchronize()
    assert y.shape == (1, 2, 128, 77) and torch.equal(y[0], x)
    comm.close()


def _tail_inputs(cuda):
    from orca_amd import orca_models, orca_predict, synth
    model = orca_models.H1esc_256M(synthetic_seed=0)
    enc0 = torch.from_numpy(np.random.RandomState(3).randn(2, 128, 64000).astype(np.float32)).to(cuda)
    chrlen = 138_368_000
    nm = orca_predict.Background256.to_device(synth.synth_normmat_256m(chrlen, seed=0), cuda)   # 8000 x 8000 float64 resident in HBM
    return model, enc0, chrlen, nm


def test_strand_parallel_tail_single_process(cuda):
    """The per-rank share of the 256 Mb tail (one strand, dist.strand_tail_256m) against the batched two-strand cascade:
    what ranks 0 and 1 of a world would all-gather, merged, must BE the single-rank result (same kernels per map)."""
    from orca_amd import dist as D
    from orca_amd import engine
    model, enc0, chrlen, de = _tail_inputs(cuda)
    mpos, wpos = 70_000_000, 128_000_000
    whole = D.strand_parallel_cascade_256m(model, enc0, mpos, wpos, chrlen, de)          # no process group: both strands here
    fwd = D.strand_tail_256m(model, enc0, 0, mpos, wpos, chrlen, de)
    rev = D.strand_tail_256m(model, enc0, 1, mpos, wpos, chrlen, de)
    assert fwd.shape == (4, 1, 250, 250) and len(whole) == 4
    assert float((fwd - rev).abs().max()) > 1e-3                                        # the strands do differ
    for j in range(4):
        assert torch.equal(engine.strand_merge(fwd[j, 0], rev[j, 0]), whole[j][0]), j


def test_strand_parallel_tail_equals_genomepredict_256mb_fixture(cuda):
    """`strand_parallel_cascade_256m` / `cascade_256m` = the part of genomepredict_256Mb after the Encoder, NUMERICALLY: per-strand
    backgrounds at each strand's own window start, flipped on the reverse strand (orca_predict.py:703, :724-737).  Against the maps
    the reference's own function produced (G9, all three zoom cases), with the background on the host and resident in HBM."""
    from orca_amd import dist as D
    from orca_amd import orca_models, orca_predict, synth
    from tests.util import golden, maxabs
    g = golden("G9_cascade256.npz")
    model = orca_models.H1esc_256M(synthetic_seed=0)
    net0 = standins.FakeNet0(nbins=64000, seed=0).to(cuda)
    seq = synth.synth_sequence(512000, seed=51)
    x = torch.from_numpy(seq).to(cuda).transpose(1, 2)
    xr = torch.from_numpy(np.ascontiguousarray(seq[:, ::-1, ::-1])).to(cuda).transpose(1, 2)
    enc0 = torch.cat([net0(x), net0(xr)], dim=0)
    for ci in range(3):
        mpos, wpos, chrlen = (int(v) for v in g[f"c{ci}_args"])
        nm = synth.synth_normmat_256m(chrlen, seed=0)
        dnm = orca_predict.Background256.to_device(nm, cuda)
        for bg in (nm, dnm):
            maps = D.strand_parallel_cascade_256m(model, enc0, mpos, wpos, chrlen, bg)
            for j, m in enumerate(maps):
                p = m[0].cpu().numpy()
                assert maxabs(p if ci == 0 else p[::5, ::5], g[f"c{ci}_sub_{j}"]) < 1e-4, (ci, j, type(bg))
        # one strand at a time (what a rank of an N > 1 world runs) merges to the same maps
        f = D.strand_tail_256m(model, enc0, 0, mpos, wpos, chrlen, dnm)
        r = D.strand_tail_256m(model, enc0, 1, mpos, wpos, chrlen, dnm)
        from orca_amd import engine
        for j in range(4):
            assert torch.equal(engine.strand_merge(f[j, 0], r[j, 0]), maps[j][0]), (ci, j)


def test_strand_bin_sharded_32m_single_process_equals_cascade(cuda):
    """dist.strand_bin_sharded_32m with one rank (both strands, all bins here) IS cascade_32m + merge; and the per-rank pieces of a
    4-rank world - strand x bin-shard encodings reassembled by hand, one strand's tail at a time - merge to the same maps."""
    from orca_amd import dist as D
    from orca_amd import engine, orca_models, orca_predict, synth
    model = orca_models.H1esc(synthetic_seed=0)
    L = 32_000_000      # the cascade needs the full 8000 bins
    codes = torch.from_numpy(synth.synth_base_codes(L, seed=33)[None]).to(cuda)
    mpos, wpos = L // 2 + 123456, L // 2
    ref = orca_predict.cascade_32m(model, [codes, codes], mpos, wpos, [False, True], merge=True)[2]
    one = D.strand_bin_sharded_32m(model, codes, mpos, wpos)
    assert all(torch.equal(a, b) for a, b in zip(one, ref))
    encs = []
    for st in range(2):
        parts = [model.net0.forward_codes(codes, reverse=bool(st), bin_lo=lo, bin_hi=hi) for (_, lo, hi) in (D.strand_bin_plan(8000, 2 * sh + st, 4)[0] for sh in range(2))]
        encs.append(torch.cat(parts, dim=2))
    tails = [torch.stack([p[0] for p in orca_predict.cascade_32m_from_enc(model, encs[st], mpos, wpos, [bool(st)])[0]]) for st in range(2)]
    for j in range(6):
        assert float((engine.strand_merge(tails[0][j, 0], tails[1][j, 0]) - ref[j][0]).abs().max()) < 2e-5, j
    # from 4 ranks on, ranks 2 / 3 supply the `+ denet_1_pt` term of the 4 kb level (it does not depend on the cascade): tails without it
    # plus `denet1m_32m_from_enc` must give the same maps, levels 32 .. 2 bit for bit
    for st in range(2):
        bare = torch.stack([p[0] for p in orca_predict.cascade_32m_from_enc(model, encs[st], mpos, wpos, [bool(st)], with_1m=False)[0]])
        one_m = orca_predict.denet1m_32m_from_enc(model, encs[st], mpos, wpos, [bool(st)])[0]
        assert torch.equal(bare[:5], tails[st][:5])
        assert float((bare[5] + one_m - tails[st][5]).abs().max()) < 1e-6
        assert float(one_m.abs().max()) > 1e-3


def test_encoder_from_a_code_window(cuda):
    """A rank's share of the packed sequence (engine.CodeWindow = its bins' bases +- the 112 kb halo, mirrored for the reverse complement)
    gives exactly the bins of the full-sequence call; a window that is too short is refused, not zero-filled."""
    from orca_amd import engine, synth
    from tests.util import product_module
    enc = product_module("Encoder", 0)
    L = 4000 * 900
    codes = torch.from_numpy(synth.synth_base_codes(L, seed=44)[None]).to(cuda)
    for rev in (False, True):
        full = enc.forward_codes(codes, reverse=rev)
        for lo, hi in ((0, 300), (300, 640), (640, 900)):
            b0, b1 = engine.code_window_range(L, lo, hi, reverse=rev)
            assert b1 - b0 <= (hi - lo) * 4000 + 224000
            win = engine.CodeWindow(codes[:, b0:b1].contiguous(), b0, L)
            part = enc.forward_codes(win, reverse=rev, bin_lo=lo, bin_hi=hi)
            assert torch.equal(part, full[:, :, lo:hi]), (rev, lo, hi)
    b0, b1 = engine.code_window_range(L, 300, 640)
    with pytest.raises(Exception, match="code window"):
        enc.forward_codes(engine.CodeWindow(codes[:, b0 + 4000:b1].contiguous(), b0 + 4000, L), bin_lo=300, bin_hi=640)


def test_block_mean_bit_identical_to_numpy(cuda):
    """engine.block_mean (orca_block_mean_f64) against numpy's nanmean-of-nanmean on the same float64 background: identical BITS for
    every level of the 256 Mb cascade, windows off the origin, NaN entries; the log-background and its reverse-strand flip."""
    from orca_amd import engine, orca_predict, synth
    nm = synth.synth_normmat_256m(138_368_000, seed=3)
    rs = np.random.RandomState(0)
    nm[rs.randint(0, 8000, 500), rs.randint(0, 8000, 500)] = np.nan
    nm[4000:4016, :] = np.nan                      # whole groups missing
    d = torch.from_numpy(nm).to(cuda)
    for level, start in ((256, 0), (128, 1000), (128, 4000), (64, 5999), (32, 7000), (32, 3993)):
        nb = level // 8
        w = 250 * nb
        with np.errstate(invalid="ignore", divide="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ref = np.nanmean(np.nanmean(np.reshape(nm[None, start:start + w, start:start + w], (1, 250, nb, 250, nb)), axis=4), axis=2)[0]
                lref = np.log(ref.astype(np.float32))
        mean, logt = engine.block_mean(d, start, nb)
        m = mean.cpu().numpy()
        assert np.array_equal(np.isnan(m), np.isnan(ref)) and np.array_equal(m[~np.isnan(m)].view(np.int64), ref[~np.isnan(ref)].view(np.int64)), (level, start)
        lg = logt[0, 0].cpu().numpy()
        ok = ~np.isnan(lref)
        assert np.abs(lg[ok] - lref[ok]).max() < 2e-6
        _, lflip = engine.block_mean(d, start, nb, flip=True, want_mean=False)
        assert torch.equal(lflip[0, 0].flip(0, 1).nan_to_num(7.0), logt[0, 0].nan_to_num(7.0))


def test_sharded_encoder_world2_rccl(cuda):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs (the driver's 8-GPU node); the partition / reassembly logic is covered on CPU by tests/test_dist_cpu.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(29600 + os.getpid() % 300), os.path.join(ROOT, "tests", "dist_gpu_worker.py")]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = [json.loads(l.split("DIST_RESULT ", 1)[1]) for l in p.stdout.splitlines() if "DIST_RESULT " in l]
    assert len(rows) == 2
    for r in rows:
        for k, v in r.items():
            if k not in ("rank", "world"):
                assert v == 0.0, (k, v, r)     # same kernels on the same bins: bit-identical to the unsharded encoding


def test_bench_two_ranks_on_one_gpu_over_gloo(cuda):
    """`bench.py --gpus 2` as the driver launches it (torch.distributed.run, one process per rank), with both ranks on cuda:0 and gloo as
    the process group (ORCA_BENCH_ONE_DEVICE / ORCA_BENCH_BACKEND test hooks): the whole N > 1 control flow - replica mode with the
    max-over-ranks clock, the 256 Mb section with bin-sharded Encoders, the all-gathers, one strand's tail per rank parity and the map
    gather - runs on a 1-GPU box.  The sharded maps must be the single-rank ones (checksum of the four merged maps)."""
    env = dict(os.environ, ORCA_BENCH_ONE_DEVICE="1", ORCA_BENCH_BACKEND="gloo")
    base = [os.path.join(ROOT, "bench.py"), "--full", "--steps", "1", "--warmup", "1", "--sharded-steps", "1", "--no-cpu-baseline"]
    p1 = subprocess.run([sys.executable] + base + ["--gpus", "1"], env=env, capture_output=True, text=True, timeout=900)
    assert p1.returncode == 0, p1.stderr[-2000:]
    one = json.loads([l for l in p1.stdout.splitlines() if l.startswith("{")][-1])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(29300 + os.getpid() % 300)] + base + ["--gpus", "2"]
    p2 = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert p2.returncode == 0, p2.stdout[-1500:] + p2.stderr[-1500:]
    lines = [l for l in p2.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                            # ONE JSON line, from rank 0
    two = json.loads(lines[0])
    assert two["n_gpus"] == 2 and two["scaling"] == "weak" and two["metric"] == one["metric"]
    s1, s2 = one["sharded_256mb"], two["sharded_256mb"]
    assert "error" not in s2, s2
    assert s2["n_gpus"] == 2 and s2["bins_this_rank"] == [0, 32000] and s1["bins_this_rank"] == [0, 64000]
    assert abs(s2["maps_checksum"] - s1["maps_checksum"]) <= 1e-6 * abs(s1["maps_checksum"]), (s1["maps_checksum"], s2["maps_checksum"])
    # both sharded sections check themselves against the reference's fixtures (G20 at 256 Mb, G8 at 32 Mb) - also at N = 2
    assert s2["parity"]["ok"] and s1["parity"]["ok"], (s1["parity"], s2["parity"])
    # a rank keeps its bins' bases +- halo, once per strand: at N = 2 that is two different halves (+ halos) - from N = 4 on it shrinks
    assert s2["sequence_bytes_on_this_rank"] == 2 * (128_000_000 + 112_000)
    t1, t2 = one["sharded_32mb"], two["sharded_32mb"]
    assert "error" not in t2, t2
    assert t2["n_gpus"] == 2 and t2["scaling"] == "strong" and t1["parity"]["ok"] and t2["parity"]["ok"], (t1, t2)
    # the one-job sections: same maps at every N (a map does not depend on the batch size it was decoded in), per-phase times, the N = 1 time
    # measured in the same run, rooflines, and the two-model job (four (model, strand) units: two per rank at N = 2)
    m1, m2 = one["sharded_32mb_two_models"], two["sharded_32mb_two_models"]
    assert "error" not in m2 and m2["models"] == 2 and m1["parity"]["ok"] and m2["parity"]["ok"], m2
    for a, b in ((t1, t2), (m1, m2)):
        assert abs(a["maps_checksum"] - b["maps_checksum"]) <= 1e-6 * abs(a["maps_checksum"]), (a["maps_checksum"], b["maps_checksum"])
        for k in ("encoder_ms_per_rank_max", "allgather_ms_max", "tail_ms_max", "n1_ms_same_run", "efficiency_vs_n1"):
            assert b[k] is not None and b[k] >= 0, (k, b)
        assert 0 < b["roofline"]["encoder"]["frac"] < 1 and a["efficiency_vs_n1"] == 1.0
    assert set(two["strong_scaling"]) >= {"sharded_256mb", "sharded_32mb", "sharded_32mb_two_models"} and s2["efficiency_vs_n1"] > 0
    # ---- the driver's N = 1 record is self-sufficient: strict-fp32 readings with their own parity on the full cascade,
    #      the Decoder roofline at B = 2 and B = 4, config 5 on 256 variants with the reference-style comparator on 16, projections + note
    for key in ("exact_f32", "bf16x3"):
        assert one[key]["parity"]["ok"] and max(one[key]["parity"]["max_abs_per_level"]) < 1e-4 and one[key]["ms_per_step"] > 0, one[key]
    rd = one["roofline_decoder"]
    assert rd["ms_per_forward"] > 0 and rd["batch_of_4"]["ms_per_forward"] > rd["ms_per_forward"] and 0 < rd["batch_of_4"]["frac"] < 1
    assert rd["single_plane_b8"]["ms_per_forward"] > 0 and rd["single_plane_b8"]["mfma_products_per_algorithmic_mac"] == 1
    # config 5 on the workload as SURVEY 8(d) draws it (unaligned) AND on rounds 3-5's 4 kb-aligned set, each with its comparator
    c5 = one["config5"]
    assert "error" not in c5 and c5["coordinates"].startswith("unaligned") and c5["svs"] == 256 and c5["max_abs_vs_whole_window_encoding"] < 1e-4, c5
    a5 = c5["aligned_4kb"]
    assert a5["svs"] == 256 and a5["as_the_reference_does_it"]["svs"] == 8 and a5["max_abs_vs_whole_window_encoding"] < 1e-4, a5
    # (round 6: off the grid the windows go through the stage-4 cache - a fraction of a per cent of the bins through the Encoder's front again)
    assert a5["encoder_bins_encoded_frac"] < 0.1 and c5["encoder_bins_encoded_frac"] < 0.01 and c5["stage3_cache"]["entries"] == 160 and a5["stage3_cache"] is None
    assert c5["svs_per_s"] > 2 * c5["whole_window_route"]["svs_per_s"] > 0 and a5["svs_per_s"] > 0.8 * c5["svs_per_s"]
    rc = one["reference_call_form"]                            # the reference's call: host float32 array in, numpy maps out (PCIe inclusive)
    assert "error" not in rc and rc["ms_per_call"] > one["ms_per_step"] and rc["two_models_ms"] > rc["ms_per_call"] and rc["maps_equal_timed_region"], rc
    assert one["dtype"].startswith("f16x2") and one["config"]["other_configs_in_this_line"]["config5_unaligned_svs_per_s"] == c5["svs_per_s"]
    assert one["roofline"]["other_readings"]["exact_f32_ms_per_step"] == one["exact_f32"]["ms_per_step"]
    assert one["roofline"]["executed_frac"] >= one["roofline"]["frac"] and one["config3"]["roofline"]["executed_frac"] > 0
    assert one["config3"]["parity"]["ok"], one["config3"]
    rf = one["roofline"]          # the dominant kernel's HBM traffic is measured by counter passes inside the run (child processes), not replayed
    assert rf["traffic_measured_in_run"] is True and 0.5 < rf["traffic_over_algorithmic"] < 1.3 and rf["traffic_launches"] >= 2, rf      # (conv1.b pools its output: its in + out count is an upper bound)
    note = one["strong_scaling"]["note"]
    assert "tail" in note.lower() and "256 Mb" in note
    pj = one["strong_scaling"]["projection_n8"]
    assert all(pj[k]["projected"] and 0 < pj[k]["efficiency"] <= 1 for k in ("sharded_256mb", "sharded_32mb", "sharded_32mb_two_models")), pj
    assert pj["sharded_256mb"]["efficiency"] > pj["sharded_32mb"]["efficiency"]            # the 32 Mb window is tail-bound
    k1 = t1["encoder_kernels_this_rank"]
    assert k1["stage7_kernel"] == "conv_bf16s.h" and k1["stage7_positions_with_halo"] == 8000 and k1["launches"]["planar"] > 0, k1


def test_bench_four_ranks_on_one_gpu_over_gloo(cuda):
    """The same with FOUR ranks (the first world size at which a strand's Encoder bins are split over several ranks, a rank holds less
    than half of the packed sequence, and ranks 2 / 3 only contribute placeholders to the map gathers): both sharded sections must
    reproduce the reference's fixtures (G20 at 256 Mb, G8 at 32 Mb) exactly as at N = 1."""
    env = dict(os.environ, ORCA_BENCH_ONE_DEVICE="1", ORCA_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=4", "--master-addr", "127.0.0.1",
           "--master-port", str(29700 + os.getpid() % 200), os.path.join(ROOT, "bench.py"), "--full", "--gpus", "4", "--steps", "1", "--warmup", "1",
           "--sharded-steps", "1", "--no-cpu-baseline"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    s, t = d["sharded_256mb"], d["sharded_32mb"]
    assert d["n_gpus"] == 4 and "error" not in s and "error" not in t, (s, t)
    assert s["bins_this_rank"] == [0, 16000] and s["sequence_bytes_on_this_rank"] == 2 * (64_000_000 + 112_000)
    assert s["parity"]["ok"] and t["parity"]["ok"], (s["parity"], t["parity"])
    m = d["sharded_32mb_two_models"]                                    # four units on four ranks: one tail each
    assert "error" not in m and m["parity"]["ok"] and m["models"] == 2, m
    for sec in (s, t, m):
        assert sec["efficiency_vs_n1"] > 0 and sec["n1_ms_same_run"] > 0 and 0 < sec["roofline"]["encoder"]["frac"] < 1, sec
    assert t["roofline"]["allgather"]["bytes_received_per_rank"] == 3 * 128 * 4000 * 4
    assert set(d["strong_scaling"]) >= {"sharded_256mb", "sharded_32mb", "sharded_32mb_two_models"}


def test_bench_eight_ranks_on_one_gpu_over_gloo(cuda):
    """De-risking N = 8 without the hardware: `bench.py --gpus 8` as the driver will launch it, all eight ranks on cuda:0
    over gloo.  256 Mb: 8 000-bin shards (each rank 32 Mb of bases + the 112 kb halo, the Encoder in 32 Mb chunks: eight workspaces on one
    GPU); 32 Mb, one model: 2 strands x 4 shards of 2 000 bins - the `conv_small.h` boundary: rank 0's shard starts at the window's end
    (2 028 positions at stage 7 with its one halo: the short-row kernel), interior shards have 2 056 (the chunk-after-chunk kernel); two
    models: 4 units x 2 shards, the `+ denet_1_pt` terms on ranks 4-7.  Every section must reproduce the reference's fixtures at 1e-4; the
    maps of the N = 8 job are NOT bit-equal to N = 1 where a shard's stage 7 changed kernels (another fp32 summation order, ~1e-6) - the
    checksum relation asserted here is the one that is true: relative 1e-6."""
    env = dict(os.environ, ORCA_BENCH_ONE_DEVICE="1", ORCA_BENCH_BACKEND="gloo")
    base = [os.path.join(ROOT, "bench.py"), "--full", "--steps", "1", "--warmup", "1", "--sharded-steps", "1", "--no-cpu-baseline", "--no-configs", "--sharded-timeout", "1500"]
    p1 = subprocess.run([sys.executable] + base + ["--gpus", "1"], env=env, capture_output=True, text=True, timeout=900)
    assert p1.returncode == 0, p1.stderr[-2000:]
    one = json.loads([l for l in p1.stdout.splitlines() if l.startswith("{")][-1])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8", "--master-addr", "127.0.0.1",
           "--master-port", str(29900 + os.getpid() % 90)] + base + ["--gpus", "8"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=2400)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    s, t, m = d["sharded_256mb"], d["sharded_32mb"], d["sharded_32mb_two_models"]
    assert d["n_gpus"] == 8 and all("error" not in x and "skipped" not in x for x in (s, t, m)), (s, t, m)
    assert s["bins_this_rank"] == [0, 8000] and s["sequence_bytes_on_this_rank"] == 2 * (32_000_000 + 112_000)
    assert s["parity"]["ok"] and t["parity"]["ok"] and m["parity"]["ok"], (s["parity"], t["parity"], m["parity"])
    ks, kt, km = s["encoder_kernels_this_rank"], t["encoder_kernels_this_rank"], m["encoder_kernels_this_rank"]
    assert ks["stage7_positions_with_halo"] == 8028 and ks["stage7_kernel"] == "conv_bf16s.h", ks
    assert kt["bins"] == [0, 2000] and kt["stage7_positions_with_halo"] == 2028 and kt["stage7_kernel"] == "conv_small.h" and kt["launches"]["conv_small"] == 4, kt
    assert km["bins"] == [0, 4000] and km["stage7_kernel"] == "conv_bf16s.h", km
    assert t["sequence_bytes_on_this_rank"] == 8_000_000 + 112_000 and m["sequence_bytes_on_this_rank"] == 16_000_000 + 112_000
    assert t["roofline"]["allgather"]["bytes_received_per_rank"] == 7 * 128 * 2000 * 4
    for a, b in ((one["sharded_256mb"], s), (one["sharded_32mb"], t), (one["sharded_32mb_two_models"], m)):
        assert abs(a["maps_checksum"] - b["maps_checksum"]) <= 1e-6 * abs(a["maps_checksum"]), (a["maps_checksum"], b["maps_checksum"])
        assert b["efficiency_vs_n1"] > 0 and b["n1_ms_same_run"] > 0
