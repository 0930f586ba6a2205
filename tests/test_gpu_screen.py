"""The 1 Mb mutagenesis screen (orca_amd/screen.py) on the MI355X: every alt map, 1-D head and score of the two-part route against the whole
window through Net (model.net on the edited windows), batch invariance (bit for bit), the CPU oracle on two edits, the whole-window route of
another precision, and the range-safe redo when the fp16-range check fires."""
import numpy as np
import pytest
import torch

from oracle import orca_oracle as O
from orca_amd import orca_models as M
from orca_amd import orca_modules as pm
from orca_amd import screen as S
from orca_amd import synth
from tests.util import maxabs

pytestmark = pytest.mark.gpu

L = 1_000_000
TOL = 2e-5


def _window():
    rs = np.random.RandomState(2024)
    c = rs.randint(0, 4, L).astype(np.uint8)
    for a, b in ((3_000, 3_400), (123_456, 124_000), (499_700, 500_300), (998_500, 998_900)):
        c[a:b] = 4
    return c


def _edits(c):
    def snv(p):
        return S.Edit("sub", p, 1, [(int(c[p]) + 1 + p % 3) % 4 if c[p] < 4 else p % 4])
    e = [snv(p) for p in (0, 1, L - 1, L - 2, 777, 1_999, L - 1_234, L - 2_000, 250_003, 400_000, 612_345, 777_777, 3_100, 998_600)]
    e += [S.Edit("mask", 3_900, 200), S.Edit("mask", 399_800, 400), S.Edit("mask", 123_000, 2_000), S.Edit("mask", L - 300, 300),
          S.Edit("inv", 7_990, 30), S.Edit("inv", 119_600, 800), S.Edit("inv", 499_500, 1_000), S.Edit("inv", 0, 2_500),
          S.Edit("inv", 300_000, 50_000), S.Edit("mask", 0, L), S.Edit("sub", 640_000, 5, "ACGTN"), S.Edit("sub", L - 4, 4, "GGGG"),
          S.Edit("inv", L - 5_000, 4_000), S.Edit("sub", 2, 3, "TTT")]
    e += [snv(p) for p in (11_111, 22_222, 333_333, 444_444, 555_555, 666_666, 888_888, 901_234, 950_001, 987_654)]
    return e


_LUT = None


def _x(codes_rows, dev):
    global _LUT
    if _LUT is None or _LUT.device != dev:
        _LUT = torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [.25, .25, .25, .25]], dtype=torch.float32, device=dev)
    return _LUT[codes_rows.long()].transpose(1, 2).contiguous()


def _net_on(net, wins, dev, chunk=8):
    """model.net (Net.forward, the whole-window route) on edited windows [E, L] numpy: maps [E, n, n], 1-D heads [E, num_1d, n]."""
    maps, heads = [], []
    with torch.no_grad():
        for i in range(0, len(wins), chunk):
            out = net(_x(torch.from_numpy(np.ascontiguousarray(wins[i: i + chunk])).to(dev), dev))
            mp, h = out if isinstance(out, tuple) else (out, None)
            maps.append(mp[:, 0].cpu().numpy())
            heads.append(None if h is None else h.cpu().numpy())
    return np.concatenate(maps), (None if heads[0] is None else np.concatenate(heads))


@pytest.fixture(scope="module")
def case(cuda):
    c = _window()
    edits = _edits(c)
    wins = np.stack([S.apply_edit(c, e) for e in edits])
    return c, edits, wins, torch.from_numpy(c).to(cuda)


def _check_against_net(res, net, c, wins, dev, tol=TOL):
    ref_map, ref_1d = _net_on(net, c[None], dev)
    maps, heads = _net_on(net, wins, dev)
    scale = max(1.0, float(np.abs(maps).max()))
    assert maxabs(res.ref_map.cpu().numpy(), ref_map[0]) / scale < tol
    assert maxabs(res.maps.cpu().numpy(), maps) / scale < tol
    if heads is not None:
        assert maxabs(res.ref_1d.cpu().numpy(), ref_1d[0]) < tol
        assert maxabs(res.delta_1d.cpu().numpy(), heads - res.ref_1d.cpu().numpy()[None]) < tol
    return maps


@pytest.mark.parametrize("cls,seed", [(M.H1esc_1M, 0), (M.Hff_1M, 1)])
def test_screen_matches_whole_window_net_and_is_batch_invariant(cuda, case, cls, seed):
    c, edits, wins, win = case
    model = cls(synthetic_seed=seed).to(cuda)
    st = {}
    res = S.screen_1m(model, win, edits, batch=64, keep_maps=True, stats=st)
    assert st["route"] == "two_part" and st["two_part_batches"] == 1 and st["range_fallback_batches"] == 0 and st["whole_window_batches"] == 0
    assert tuple(res.maps.shape) == (len(edits), 250, 250) and tuple(res.delta_1d.shape) == (len(edits), model.num_1d, 250)
    _check_against_net(res, model.net, c, wins, cuda)
    # scores = the host function on the returned maps
    prof, mean, amax = S.scores_host(res.maps.cpu().numpy(), res.ref_map.cpu().numpy())
    for got, want in ((res.delta_profile, prof), (res.delta_abs_mean, mean), (res.delta_abs_max, amax)):
        g = got.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(g - want) <= 1e-6 * np.maximum(np.abs(want), 1e-30)), float(np.abs(g - want).max())
    assert edits[23].length == L and float(res.delta_abs_max[23]) > 0           # the whole-window mask moves the map
    # batch invariance: bit for bit whatever the batch size and order
    for b in (1, 7):
        r2 = S.screen_1m(model, win, edits, batch=b, keep_maps=True)
        for name in ("maps", "delta_profile", "delta_abs_mean", "delta_abs_max", "delta_1d"):
            assert torch.equal(getattr(r2, name), getattr(res, name)), (b, name)
        assert torch.equal(r2.ref_map, res.ref_map)
    perm = np.random.RandomState(seed).permutation(len(edits))
    r3 = S.screen_1m(model, win, [edits[i] for i in perm], batch=64, keep_maps=True)
    assert torch.equal(r3.maps, res.maps[torch.from_numpy(perm).to(cuda)])
    assert torch.equal(r3.delta_abs_mean, res.delta_abs_mean[torch.from_numpy(perm).to(cuda)])
    # without keep_maps: the same scores, no maps
    r4 = S.screen_1m(model, win, edits[:5])
    assert r4.maps is None and torch.equal(r4.delta_profile, res.delta_profile[:5])


def test_screen_against_cpu_oracle(cuda, case):
    c, edits, wins, win = case
    model = M.H1esc_1M(synthetic_seed=0).to(cuda)
    pick = [4, 20]                                   # an SNV near the start, a 1 kb inversion across an N run
    res = S.screen_1m(model, win, [edits[i] for i in pick], keep_maps=True)
    sd = {k: v.cpu() for k, v in model.net.state_dict().items()}
    from tests.encoder_ref import onehot
    maps, heads = O.net_forward(sd, onehot(wins[pick], torch.float32), num_1d=32)
    assert maxabs(res.maps.cpu().numpy(), maps[:, 0].numpy()) < 1e-4
    assert maxabs(res.delta_1d.cpu().numpy() + res.ref_1d.cpu().numpy()[None], heads.numpy()) < 1e-4


def test_other_precision_takes_the_whole_window_route(cuda, case):
    c, edits, wins, win = case
    model = M.H1esc_1M(synthetic_seed=0).to(cuda)
    model.net.precision = "bf16x3"
    pick = [0, 4, 16, 23, 25]
    st = {}
    res = S.screen_1m(model, win, [edits[i] for i in pick], batch=3, keep_maps=True, stats=st)
    assert st["route"] == "whole_window" and st["whole_window_batches"] == 2 and st["two_part_batches"] == 0
    _check_against_net(res, model.net, c, wins[pick], cuda)


def test_range_fallback_when_the_fp16_check_fires(cuda, case):
    """Encoder weights x 2.0 (tools/range_headroom.py's sweep trips the Encoder there): the reference trips the deferred check, every batch is
    redone on the whole-window route in the range-safe arithmetic, and the results still equal model.net on the edited windows."""
    c, edits, wins, win = case
    net = pm.Net(num_1d=32)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    hot = synth.synth_state_dict(shapes, seed=0, relu_gain=2.0)
    cold = synth.synth_state_dict(shapes, seed=0)
    enc_keys = {k for k in shapes if k.startswith(("lconv", "conv"))}
    net.load_state_dict({k: torch.from_numpy(np.asarray(hot[k] if k in enc_keys else cold[k])) for k in shapes}, strict=True)
    net = net.eval().to(cuda)
    pick = [4, 17, 23]
    st = {}
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = S.screen_1m(net, win, [edits[i] for i in pick], keep_maps=True, stats=st)
        assert st["range_fallback_reference"] and st["range_fallback_batches"] == 1 and st["two_part_batches"] == 0
        _check_against_net(res, net, c, wins[pick], cuda)
