"""The guard-band arena (tests/arena.py) proved on CPU tensors with planted faults -- without this file the memory-contract
tests of tests/test_memory_contract_gpu.py could be vacuous."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from arena import ALIGN, MIN_BAND, SENTINEL, Arena, ArenaError, nbytes_of  # noqa: E402


def _case(shift=0, dtype=torch.float32, n=37):
    """x (input) -> out, with a scratch between them; returns (arena, x, ws, out)."""
    sizes = [nbytes_of(n, dtype)] * 3
    ar = Arena("cpu", sizes)
    x = ar.alloc(n, dtype, fill=torch.arange(n).to(dtype) + 1, name="x")
    ws = ar.alloc(n, dtype, kind="scratch", name="ws", shift=shift)
    out = ar.alloc(n, dtype, name="out", shift=shift)
    return ar, x, ws, out


def test_sentinel_is_nan_in_both_float_widths():
    ar = Arena("cpu", [64, 64])
    o32 = ar.alloc(4, torch.float32, name="o32")
    o64 = ar.alloc(4, torch.float64, name="o64")
    assert torch.isnan(o32).all() and torch.isnan(o64).all()
    assert int(o32.view(torch.int32)[0]) == SENTINEL
    assert ar.unwritten(o32) == 4 and ar.unwritten(o64) == 4


def test_layout_alignment_bands_and_margins():
    big = 3 << 20
    ar = Arena("cpu", [big, 100, 7])
    a = ar.alloc(big, torch.uint8, name="a")
    b = ar.alloc(25, torch.float32, name="b", shift=48)
    c = ar.alloc(7, torch.uint8, name="c")
    assert ar.band >= big and ar.band >= MIN_BAND
    base = ar.raw.data_ptr()
    assert (a.data_ptr() - base) % ALIGN == 0 and (c.data_ptr() - base) % ALIGN == 0
    assert (b.data_ptr() - base) % ALIGN == 48
    recs = sorted(ar.allocs, key=lambda r: r.start)
    assert recs[0].start >= ar.band                                         # head margin
    assert ar.capacity - recs[-1].end >= ar.band                            # tail margin
    for p, q in zip(recs, recs[1:]):
        assert q.start - p.end >= ar.band
    ar.check()


@pytest.mark.parametrize("shift", [0, 16, 256 + 48])
def test_clean_function_passes(shift):
    ar, x, ws, out = _case(shift)
    ws.copy_(x * 2)
    out.copy_(ws + 1)
    ar.check()
    assert ar.unwritten(out) == 0
    assert torch.equal(out, x * 2 + 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.uint8])
def test_one_element_past_the_end_is_reported(dtype):
    ar, x, ws, out = _case(dtype=dtype)
    out.copy_(x)
    rec = ar.find("out")
    size = out.element_size()
    ar.raw[rec.end:rec.end + size] = 0            # the planted fault, through the raw view
    with pytest.raises(ArenaError) as e:
        ar.check()
    assert (e.value.name, e.value.side, e.value.offset) == ("out", "after", 0)
    assert "'out'" in str(e.value) and "after" in str(e.value)


def test_one_element_before_the_start_is_reported():
    ar, x, ws, out = _case()
    out.copy_(x)
    rec = ar.find("out")
    ar.raw[rec.start - 4:rec.start] = 0
    with pytest.raises(ArenaError) as e:
        ar.check()
    assert (e.value.name, e.value.side, e.value.offset) == ("out", "before", 4)


def test_a_single_flipped_bit_far_inside_a_band_is_reported_with_its_offset():
    ar, x, ws, out = _case()
    out.copy_(x)
    rec = ar.find("ws")
    ar.raw[rec.end + 12345] ^= 1
    with pytest.raises(ArenaError) as e:
        ar.check()
    assert (e.value.name, e.value.side, e.value.offset) == ("ws", "after", 12345)


def test_overrun_at_the_arena_head_and_tail_is_reported():
    ar, x, ws, out = _case()
    ar.raw[0] = 0
    with pytest.raises(ArenaError) as e:
        ar.check()
    assert (e.value.name, e.value.side) == ("x", "before")
    ar, x, ws, out = _case()
    ar.raw[-1] = 0
    with pytest.raises(ArenaError) as e:
        ar.check()
    assert (e.value.name, e.value.side) == ("out", "after")


def test_modified_input_is_reported():
    ar, x, ws, out = _case()
    out.copy_(x)
    ar.bytes_of("x")[5 * 4] ^= 0x40
    with pytest.raises(ArenaError) as e:
        ar.check()
    assert (e.value.name, e.value.side, e.value.offset) == ("x", "input", 20)


def test_hole_left_unwritten_is_counted():
    ar, x, ws, out = _case()
    out[:20].copy_(x[:20])
    out[23:].copy_(x[23:])
    ar.check()
    assert ar.unwritten(out) == 3
    ar8 = Arena("cpu", [16])
    m = ar8.alloc(10, torch.uint8, name="m")
    m[:9] = 1
    assert ar8.unwritten(m) == 1


def _run(fn, fill):
    ar, x, ws, out = _case()
    rec = ar.find("out")
    if fill == "ff":
        ar.raw[rec.start:rec.end].fill_(0xFF)
    elif fill == "zero":
        ar.raw[rec.start:rec.end].zero_()
    fn(x, out)
    ar.check()
    return ar.bytes_of("out").clone()


def test_accumulating_instead_of_overwriting_is_reported():
    def good(x, out):
        out.copy_(x)

    def bad(x, out):
        out += x

    runs = [_run(good, f) for f in ("sentinel", "ff", "zero")]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    runs = [_run(bad, f) for f in ("sentinel", "ff", "zero")]
    assert not (torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]))
    # and the sentinel run alone already shows it: NaN + x stays NaN
    assert torch.isnan(runs[0].view(torch.float32)).all()


def test_out_of_space_and_duplicate_names_raise():
    ar = Arena("cpu", [64, 64])
    ar.alloc(16, torch.float32, name="a")
    with pytest.raises(ValueError):
        ar.alloc(1, torch.float32, name="a")
    with pytest.raises(RuntimeError):
        ar.alloc(1 << 22, torch.uint8, name="b")


def test_every_exported_function_has_a_memory_contract_case_or_a_reason():
    """the coverage ledger of tests/test_memory_contract_gpu.py needs no GPU: it parses the header against the case table"""
    import test_memory_contract_gpu as T
    T.ledger_check()
    assert len(T.CASES) > 100 and len(T.KNOB_CASES) >= 20
