"""tests/ws_contract.py can fail: the fills decode as claimed, the guarded view is what it says, and three faulty fake executors -- plain torch
functions over the byte view -- are each caught by the check that exists for them, while a clean one passes both.  No GPU."""
import math

import pytest
import torch

import ws_contract as W

CPU = torch.device("cpu")


# ---- the fills ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", W.ELEMENT_TYPES)
def test_fills_decode_as_claimed(kind):
    assert W.FILLS == {"zero": 0x00, "nan": 0xFF, "big": 0x47}
    nan, big, zero = (W.decode_fill(W.FILLS[k], kind) for k in ("nan", "big", "zero"))
    assert not math.isfinite(nan), f"0xFF must be non-finite as {kind}, decodes to {nan}"
    assert math.isfinite(big) and big > 0
    if kind in ("fp32", "bf16"):
        assert big > 1e4 and abs(big - 5.1e4) < 0.1e4, big          # 0x4747(4747): 1.555 * 2^15
        assert zero == 0.0
    if kind == "e4m3":
        assert big == 3.75 and zero == 0.0                             # 0 1000 111
    if kind == "e8m0":
        assert big == 2.0 ** (0x47 - 127) and zero == 2.0 ** -127


def test_fill_decoding_agrees_with_torch_dtypes():
    """the hand-written e4m3 / E8M0 decoders against torch's own dtypes, for every byte (where this torch has them)"""
    every = torch.arange(256, dtype=torch.int16).to(torch.uint8)
    if hasattr(torch, "float8_e4m3fn"):
        want = every.view(torch.float8_e4m3fn).float()
        for b in range(256):
            got = W.decode_fill(b, "e4m3")
            assert (math.isnan(got) and math.isnan(float(want[b]))) or got == float(want[b]), (b, got, float(want[b]))
    if hasattr(torch, "float8_e8m0fnu"):
        want = every.view(torch.float8_e8m0fnu).float()
        for b in range(256):
            got = W.decode_fill(b, "e8m0")
            assert (math.isnan(got) and math.isnan(float(want[b]))) or got == float(want[b]), (b, got, float(want[b]))


# ---- guarded -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("need", [1, 255, 256, 257, 4096 + 3, 1 << 20])
@pytest.mark.parametrize("fill", sorted(W.FILLS.values()))
def test_guarded_view(need, fill):
    ws, check = W.guarded(need, fill, CPU)
    assert ws.dtype == torch.uint8 and ws.numel() == need and ws.is_contiguous()
    assert ws.data_ptr() % 256 == 0
    assert W.holds_fill(ws, fill)
    base = ws._base
    assert base is not None and base.numel() >= need + 2 * W.GUARD
    front = ws.data_ptr() - base.data_ptr()
    assert front >= W.GUARD and base.numel() - front - need >= W.GUARD          # 64 KiB on both sides, in ONE allocation
    assert bool((base[:front] == W.BAND).all()) and bool((base[front + need:] == W.BAND).all())
    check("fresh")


def test_guarded_like_keeps_shape_and_dtype():
    for t in (torch.empty(2, 3, 16, 5, 7), torch.empty(5, 8, 8, 3, dtype=torch.uint8), torch.empty(3, 6, 4, dtype=torch.float64),
              torch.empty(7, 9, dtype=torch.bfloat16)):
        g, check = W.guarded_like(t, 0xFF)
        assert g.shape == t.shape and g.dtype == t.dtype and g.data_ptr() % 256 == 0 and g.is_contiguous()
        assert W.holds_fill(g, 0xFF)
        if t.dtype.is_floating_point:
            assert bool(torch.isnan(g).all())
        check()


# ---- four fake executors over the byte view: out = 2 * x, with x staged through the workspace -----------------------------------------------------
NEED, N = 1024, 64


def _clean(ws, x, out):
    stage = ws[:4 * N].view(torch.float32)
    stage.copy_(x)
    out.copy_(2 * stage)


def _writes_at_need(ws, x, out):
    _clean(ws, x, out)
    ws._base[ws.storage_offset() + NEED] = 0           # one byte past the end


def _writes_at_minus_one(ws, x, out):
    _clean(ws, x, out)
    ws._base[ws.storage_offset() - 1] = 0              # one byte in front of the start


def _reads_stale(ws, x, out):
    _clean(ws, x, out)
    out[-1] = ws[4 * N:8 * N].view(torch.float32)[0]   # an element nobody wrote


def _three_fills(executor):
    """the executor once per fill on the same input: ({fill name: output}, [guard check])"""
    x = torch.arange(N, dtype=torch.float32) - 7
    outs, checks = {}, []
    for name, fill in W.FILLS.items():
        ws, check = W.guarded(NEED, fill, CPU)
        out, out_check = W.guarded_like(torch.empty(N), 0xFF)
        snap = W.snapshot({"x": x})
        executor(ws, x, out)
        W.assert_unchanged(snap)
        outs[name] = out.clone()
        checks += [check, out_check]
    return outs, checks


def _bit_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _all_equal(outs):
    return all(_bit_equal(outs["zero"], o) for o in outs.values())


def test_clean_executor_passes_both_checks():
    outs, checks = _three_fills(_clean)
    for c in checks:
        c()
    assert _all_equal(outs) and all(bool(torch.isfinite(o).all()) for o in outs.values())
    assert torch.equal(outs["zero"], 2 * (torch.arange(N, dtype=torch.float32) - 7))


def test_write_one_byte_past_the_end_trips_the_guard():
    outs, checks = _three_fills(_writes_at_need)
    assert _all_equal(outs), "this executor's RESULT is right: only the guard can see it"
    with pytest.raises(AssertionError, match=r"write past the end: first damaged byte at end \+ 0 \(of 1024 bytes\)"):
        for c in checks:
            c()


def test_write_one_byte_in_front_trips_the_guard():
    outs, checks = _three_fills(_writes_at_minus_one)
    assert _all_equal(outs)
    with pytest.raises(AssertionError, match=r"write in front of the start: first damaged byte at start - 1, end - 1025"):
        for c in checks:
            c()


def test_stale_read_makes_the_three_fills_differ():
    outs, checks = _three_fills(_reads_stale)
    for c in checks:
        c()                                            # it stays inside the workspace: the guards cannot see it
    assert not _all_equal(outs)
    assert not _bit_equal(outs["zero"], outs["nan"]) and not _bit_equal(outs["zero"], outs["big"]) and not _bit_equal(outs["nan"], outs["big"])
    assert not bool(torch.isfinite(outs["nan"]).all()), "the NaN fill reaches the output"
    assert bool(torch.isfinite(outs["big"]).all()) and float(outs["big"][-1]) > 1e4, "the finite fill reaches it as a large finite number"


# ---- the reused workspace, the snapshot ----------------------------------------------------------------------------------------------------------
def test_reused_workspace_is_not_refilled_and_its_tail_is_watched():
    s = W.Session(0xFF, None, reuse=True)
    big = s.workspace(4096, CPU, "first")
    big[:100] = 7
    small = s.workspace(1000, CPU, "second")
    assert small.data_ptr() == big.data_ptr() and small.numel() == 1000
    assert bool((small[:100] == 7).all()) and bool((small[100:] == 0xFF).all())       # as the first call left it
    s.check()
    big[1000] = 1                                       # one byte behind the 1000 the second request was given
    with pytest.raises(AssertionError, match=r"second: write past the end of a reused workspace: first damaged byte at end \+ 0"):
        s.check()


def test_snapshot_sees_one_changed_bit_and_nan_payloads():
    lin = torch.nn.Linear(4, 4)
    objs = {"net": lin, "cond": {"k": torch.zeros(3, dtype=torch.bfloat16), "key": None}, "rope": (torch.ones(2), torch.full((2,), math.nan))}
    snap = W.snapshot(objs)
    assert len(snap) == 5
    W.assert_unchanged(snap)                             # NaN compares equal to itself: the comparison is of bytes
    objs["rope"][1].view(torch.int32)[0] ^= 1           # still NaN, another payload
    with pytest.raises(AssertionError, match=r"\['rope'\]\[1\] was changed"):
        W.assert_unchanged(snap)
    objs["rope"][1].view(torch.int32)[0] ^= 1
    with torch.no_grad():
        lin.bias[2] += 1
    with pytest.raises(AssertionError, match=r"\['net'\]\.bias was changed"):
        W.assert_unchanged(snap)
