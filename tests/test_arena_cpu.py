"""What the fill bytes of tests/arena.py decode to in the three activation formats - the preconditions its docstring states - and its bit helper."""
import numpy as np
import torch

from tests import arena


def _decode(byte):
    raw = np.full(8, byte, dtype=np.uint8)
    f32 = raw.view(np.float32)
    f16 = raw.view(np.float16)                                               # both halves of a P16 unit word hold the same pattern
    bf16 = (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32)    # a bf16 is the upper half of an fp32
    return f32, f16, bf16


def test_the_fills_are_the_documented_bytes():
    assert arena.FILLS == (0x00, 0xFF, 0x3C, 0x7B)
    assert arena.EDGE_BYTES == 4 * 40 * 128 * 4


def test_0x00_is_zero_in_every_format():
    for a in _decode(0x00):
        assert (a == 0).all() and not np.signbit(a).any()


def test_0xff_is_nan_in_every_format_and_minus_one_as_an_integer():
    for a in _decode(0xFF):
        assert np.isnan(a).all()
    raw = np.full(8, 0xFF, dtype=np.uint8)
    assert (raw == 255).all() and (raw.view(np.int8) == -1).all() and (raw.view(np.int32) == -1).all() and (raw.view(np.int64) == -1).all()
    assert (raw > 4).all()                                                   # no base code (0..3, 4 = N)


def test_0x3c_is_a_small_finite_positive_value_in_every_format():
    f32, f16, bf16 = _decode(0x3C)
    assert float(f32[0]) == (1.0 + 0x3C3C3C / 2.0 ** 23) * 2.0 ** (0x78 - 127) and abs(float(f32[0]) - 0.011489) < 1e-6
    assert float(f16[0]) == 1.0 + 0x3C / 1024.0 == 1.05859375
    assert float(bf16[0]) == 0.011474609375
    for a in (f32, f16, bf16):
        assert np.isfinite(a).all() and (a > 0).all() and (a == a[0]).all()
    assert float(f16[0]) < 65504.0 / 1e4                                     # nowhere near the fp16 range: a flag under this fill is a finding
    # fmaxf drops a NaN but keeps this value: what a ReLU or a max-pool in front of the output does to each fill
    assert np.fmax(np.float32("nan"), np.float32(0)) == 0 and np.fmax(f16[0], np.float16(0)) == f16[0]


def test_0x7b_is_large_and_finite_in_every_format():
    f32, f16, bf16 = _decode(0x7B)
    assert float(f16[0]) == 61280.0 and 65504.0 / 2 < float(f16[0]) < 65504.0        # in range alone; the sum of two such lanes is not
    assert float(f32[0]) == (1.0 + 0x7B7B7B / 2.0 ** 23) * 2.0 ** (0xF6 - 127) and 1.30e36 < float(f32[0]) < 1.31e36
    assert float(bf16[0]) == (1.0 + 0x7B / 128.0) * 2.0 ** (0xF6 - 127)
    for a in (f32, f16, bf16):
        assert np.isfinite(a).all() and (a > 0).all()
    assert not np.isfinite(_decode(0x7C)[1]).any() and all(float(_decode(b)[1][0]) < 61280.0 for b in range(0x7B))   # no larger finite byte pattern
    assert np.fmax(np.float32("nan"), f32[0]) == f32[0]                      # what a guard's running maximum keeps of each fill


def test_as_bits_flattens_nested_outputs_of_any_dtype():
    a = torch.tensor([1.0, float("nan")], dtype=torch.float32)
    b = np.array([[7, -1]], dtype=np.int64)
    c = torch.tensor([True, False])
    bits = arena.as_bits([a, None, (b, c)])
    assert bits.dtype == np.int32 and bits.size == 2 + 4 + 2
    assert bits[0] == np.float32(1.0).view(np.int32) and bits[2:6].view(np.int64).tolist() == [7, -1] and bits[6:].tolist() == [1, 0]
    assert np.array_equal(bits, arena.as_bits([a, (b, c)]))                  # NaN compares equal as bits
