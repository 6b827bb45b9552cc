"""Negative controls of tests/guarded.py, on the CPU: stand-in "kernels" of a few lines of Python
that overrun, underrun, skip an element or read past an input, and one that does none of these.
Each runs on torch CPU tensors and on numpy arrays, in fp64 and fp32.

The stand-in works on the whole allocation (handle.full viewed in the payload's type), the way a
kernel's plain global pointer can reach past the extent it was given.
"""
import numpy as np
import pytest

from guarded import (F32_PATTERN, F64_PATTERN, I32_PATTERN, GuardError, check, guard_bytes, guarded,
                     pattern_filled, problems)

BT, PER = 3, 64          # three "trajectories" of 64 elements: 8 × per-trajectory is 512 elements


def _arr(kind, dtype, n=BT * PER):
    a = (np.arange(n) % 7 + 1).astype(dtype)
    if kind == "torch":
        import torch

        return torch.from_numpy(a)
    return a


def _raw(h, dtype):
    """The whole allocation in the payload's type: index h.g is the payload's first element."""
    f = h.full
    if hasattr(f, "numpy"):
        import torch

        return f.view(torch.float64 if dtype == np.float64 else torch.float32)
    return f.view(dtype)


def _setup(kind, dtype):
    """x (in), y (out), info (out) guarded; the stand-in computes y = 2 x, info = 0."""
    x0 = _arr(kind, dtype)
    gb = guard_bytes(x0.nbytes if kind == "numpy" else x0.numel() * x0.element_size(), BT)
    x, hx = guarded(x0, "in", gb, "x")
    y, hy = guarded(x0, "out", gb, "y")
    i0 = np.zeros(BT, np.int32)
    if kind == "torch":
        import torch

        i0 = torch.from_numpy(i0)
    info, hi = guarded(i0, "out", guard_bytes(4 * BT, BT), "info")
    return x, y, info, [hx, hy, hi]


def _clean(x, y, info):
    y[...] = 2 * x
    info[...] = 0


KINDS = [(k, d) for k in ("numpy", "torch") for d in (np.float64, np.float32)]
IDS = [f"{k}-{np.dtype(d).name}" for k, d in KINDS]


def test_guard_bytes_rule():
    assert guard_bytes(3 * 8, 3) == 4096                      # the floor
    assert guard_bytes(BT * PER * 8, BT) == 4096              # 8 × 512 bytes
    assert guard_bytes(2 * 1000 * 8, 2) == 64000              # 8 × 8000 bytes, a multiple of 256 already
    assert guard_bytes(3 * 1001 * 8, 3) == 64256              # 64064 rounded up to 256
    assert guard_bytes(1, 1) % 256 == 0


@pytest.mark.parametrize("kind,dtype", KINDS, ids=IDS)
def test_fill_patterns_and_layout(kind, dtype):
    x, y, info, hs = _setup(kind, dtype)
    hx, hy, hi = hs
    pat = F64_PATTERN if dtype == np.float64 else F32_PATTERN
    bx, by, bi = hx.host_bits(), hy.host_bits(), hi.host_bits()
    item = np.dtype(dtype).itemsize
    assert hx.g * item == 4096 and bx.size == 2 * hx.g + BT * PER
    assert (bx[:hx.g] == pat).all() and (bx[hx.g + hx.size:] == pat).all()
    assert np.array_equal(np.asarray(x), np.asarray(_arr(kind, dtype)))      # input payload: the data
    assert (by == pat).all()                                                  # output: guards AND payload
    assert (bi == I32_PATTERN).all()
    assert np.isnan(np.asarray(y)).all()                                      # the pattern is a NaN
    assert tuple(y.shape) == (BT * PER,) and np.asarray(y).dtype == dtype
    p = pattern_filled(x)
    assert tuple(p.shape) == tuple(x.shape) and np.isnan(np.asarray(p)).all()
    view = np.asarray(p).view(np.int64 if dtype == np.float64 else np.int32)
    assert (view == pat).all()


@pytest.mark.parametrize("kind,dtype", KINDS, ids=IDS)
def test_clean_stand_in_passes(kind, dtype):
    x, y, info, hs = _setup(kind, dtype)
    _clean(x, y, info)
    assert problems(hs) == []
    check(hs)
    check({h.name: h for h in hs})


@pytest.mark.parametrize("kind,dtype", KINDS, ids=IDS)
def test_write_one_element_after_an_output(kind, dtype):
    x, y, info, hs = _setup(kind, dtype)
    _clean(x, y, info)
    raw = _raw(hs[1], dtype)
    raw[hs[1].g + hs[1].size] = 1.0
    with pytest.raises(GuardError, match=r"y \(out\): guard AFTER the payload overwritten, 1 element\(s\), offsets 0 \.\. 0 "):
        check(hs)
    assert len(problems(hs)) == 1


@pytest.mark.parametrize("kind,dtype", KINDS, ids=IDS)
def test_write_one_element_before_an_output(kind, dtype):
    x, y, info, hs = _setup(kind, dtype)
    _clean(x, y, info)
    raw = _raw(hs[1], dtype)
    raw[hs[1].g - 1] = 1.0
    with pytest.raises(GuardError, match=r"y \(out\): guard BEFORE the payload overwritten, 1 element\(s\), offsets -1 \.\. -1 "):
        check(hs)
    assert len(problems(hs)) == 1


def test_write_at_the_far_end_of_the_guard():
    """8 × per-trajectory − 1 elements after the output: the last element a guard of 8 trajectories
    covers (fp64, 64 elements per trajectory: the guard is exactly 512 elements)."""
    x, y, info, hs = _setup("torch", np.float64)
    _clean(x, y, info)
    h = hs[1]
    assert h.g == 8 * PER
    raw = _raw(h, np.float64)
    raw[h.g + h.size + 8 * PER - 1] = 0.0
    with pytest.raises(GuardError, match=rf"y \(out\): guard AFTER .* offsets {8 * PER - 1} \.\. {8 * PER - 1} "):
        check(hs)
    assert len(problems(hs)) == 1


@pytest.mark.parametrize("kind,dtype", KINDS, ids=IDS)
def test_one_payload_element_left_unwritten(kind, dtype):
    x, y, info, hs = _setup(kind, dtype)
    y[:100] = 2 * x[:100]
    y[101:] = 2 * x[101:]
    info[...] = 0
    with pytest.raises(GuardError, match=r"y \(out\): payload NOT WRITTEN .* 1 element\(s\), offsets 100 \.\. 100 "):
        check(hs)
    assert len(problems(hs)) == 1
    hs[1].unspecified = np.arange(BT * PER) == 100      # declared unspecified: exempt exactly that one
    check(hs)
    hs[1].unspecified = np.arange(BT * PER) == 99
    with pytest.raises(GuardError, match="NOT WRITTEN"):
        check(hs)


def test_unwritten_int32_output():
    x, y, info, hs = _setup("torch", np.float64)
    y[...] = 2 * x
    info[:2] = 0
    with pytest.raises(GuardError, match=r"info \(out\): payload NOT WRITTEN .* offsets 2 \.\. 2 "):
        check(hs)


@pytest.mark.parametrize("kind,dtype", KINDS, ids=IDS)
def test_write_into_an_inputs_guard(kind, dtype):
    x, y, info, hs = _setup(kind, dtype)
    _clean(x, y, info)
    raw = _raw(hs[0], dtype)
    raw[hs[0].g + hs[0].size + 2] = 0.0
    raw[hs[0].g + hs[0].size + 5] = 0.0
    with pytest.raises(GuardError, match=r"x \(in\): guard AFTER the payload overwritten, 2 element\(s\), offsets 2 \.\. 5 "):
        check(hs)
    assert len(problems(hs)) == 1


@pytest.mark.parametrize("kind,dtype", KINDS, ids=IDS)
def test_non_finite_output_is_reported(kind, dtype):
    x, y, info, hs = _setup(kind, dtype)
    _clean(x, y, info)
    y[7] = float("inf")
    with pytest.raises(GuardError, match=r"y \(out\): payload NOT FINITE, 1 element\(s\), offsets 7 \.\. 7 "):
        check(hs)


@pytest.mark.parametrize("kind,dtype", KINDS, ids=IDS)
def test_read_past_an_input_times_zero_reaches_the_result(kind, dtype):
    """The mechanism the GPU tests rely on: a padded operand loaded unmasked and multiplied by zero
    is 0 · NaN = NaN once the neighbour is a guard.  On a plain array whose neighbour is finite data
    the same stand-in is exact, which is why no test saw such a read before."""
    x, y, info, hs = _setup(kind, dtype)
    raw = _raw(hs[0], dtype)
    g, n = hs[0].g, hs[0].size

    def stand_in(src, first, out):
        # a dot product over a tile padded by one: the pad lane's weight is zero, its load unmasked
        w = np.ones(n + 1, dtype)
        w[n] = 0
        v = np.asarray(src[first:first + n + 1])
        o = np.asarray(out)             # shares the memory of a CPU tensor
        o[...] = 2 * v[:n]
        o[0] = (v * w).sum()

    stand_in(raw, g, y)
    info[...] = 0
    assert not np.isfinite(np.asarray(y)[0])
    # 0 · NaN keeps the NaN's payload bits, so the element may be the guard's pattern itself
    with pytest.raises(GuardError, match=r"y \(out\): payload NOT (FINITE|WRITTEN).* 1 element\(s\), offsets 0 \.\. 0 "):
        check(hs)
    # the same stand-in in the middle of finite data: finite, and equal to the masked result
    plain = np.concatenate([np.asarray(_arr(kind, dtype)), np.asarray(_arr(kind, dtype))])
    out = np.empty(n, dtype)
    stand_in(plain, 0, out)
    assert np.isfinite(out).all() and out[0] == plain[:n].sum()


def test_workspace_role_checks_guards_only():
    import torch

    ws, h = guarded(torch.empty(1000, dtype=torch.uint8), "ws", guard_bytes(1000, 2), "workspace")
    assert ws.numel() == 1000 and h.g == 4096
    check([h])                       # untouched workspace: fine, only the guards count
    ws[:10] = 1
    check([h])
    h.full[h.g + 1000] = 0
    with pytest.raises(GuardError, match=r"workspace \(ws\): guard AFTER .* offsets 0 \.\. 0 "):
        check([h])


def test_inout_role_keeps_payload_and_checks_guards():
    z0 = np.arange(12, dtype=np.float64)
    z, h = guarded(z0, "inout", 4096, "Z")
    assert np.array_equal(z, z0)
    check([h])                       # a payload nobody wrote is fine for an in/out array
    h.full[h.g - 1] = 0
    with pytest.raises(GuardError, match=r"Z \(inout\): guard BEFORE"):
        check([h])
