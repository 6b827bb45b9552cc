"""The Newton–Schulz acceptance test as integer compares on the wave-max key (lqrx_dp.hip NsKey)
against the floating-point decision it replaces, restated on the host and compared key by key.

The kernel reduces the residual to a wave-uniform integer key — the high word of the largest
|R| element in fp64, its bits in fp32 — and used to decide on ρ = 16·MT·key_bound(key):
    ρ ≤ v → accept;   !(ρ < 1) → reject (exact sweep);   after the update: ρ ≤ one_step → accept.
It now decides on the key:  key ≤ K_v;  key > K_1;  key ≤ K_one_step  (constants below, formed
exactly as NsKey forms them).  Both are restated here; for MT = 1, 2 and both precisions every
key within ±4096 of each of the three thresholds, plus 0, the +inf key and a NaN key, must get
the same three answers.
"""
import numpy as np
import pytest

TOL = {"f64": (1e-11, 1e-9), "f32": (np.float32(3e-4), np.float32(1e-5))}   # NsTol<T>::v, one_step


def key_bound(keys, prec):
    """key_bound(): fp64 — the largest double with high word `key`; fp32 — the float with those bits."""
    if prec == "f64":
        return ((keys.astype(np.uint64) << np.uint64(32)) | np.uint64(0xffffffff)).view(np.float64)
    return keys.astype(np.uint32).view(np.float32)


def old_decision(keys, mt, prec):
    T = np.float64 if prec == "f64" else np.float32
    v, one_step = TOL[prec]
    with np.errstate(over="ignore", invalid="ignore"):
        rho = T(16 * mt) * key_bound(keys, prec)
        assert rho.dtype == T
        return rho <= T(v), ~(rho < T(1)), rho <= T(one_step)


def thresholds(mt, prec):
    """NsKey<T, MT>: K_v, K_one_step (key ≤ K ⇔ ρ ≤ tol) and K_1 (key > K_1 ⇔ !(ρ < 1))."""
    v, one_step = TOL[prec]
    if prec == "f64":
        def le(t):
            b = int(np.float64(t).view(np.uint64))
            return (b >> 32) - (1 if (b & 0xffffffff) != 0xffffffff else 0)
        return (le(np.float64(v) / (16 * mt)), le(np.float64(one_step) / (16 * mt)),
                (int(np.float64(1.0 / (16 * mt)).view(np.uint64)) >> 32) - 1)
    bits = lambda t: int(np.float32(t).view(np.uint32))
    return (bits(np.float32(v) / np.float32(16 * mt)), bits(np.float32(one_step) / np.float32(16 * mt)),
            bits(np.float32(1.0) / np.float32(16 * mt)) - 1)


def new_decision(keys, mt, prec):
    kv, kone, k1 = thresholds(mt, prec)
    k = keys.astype(np.int64)
    return k <= kv, k > k1, k <= kone


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("mt", [1, 2])
def test_integer_key_decision_equals_float_decision(mt, prec):
    kv, kone, k1 = thresholds(mt, prec)
    inf_key = 0x7ff00000 if prec == "f64" else 0x7f800000
    nan_key = 0x7ff80000 if prec == "f64" else 0x7fc00000
    keys = np.concatenate([np.arange(t - 4096, t + 4097) for t in (kv, kone, k1)]
                          + [np.array([0, inf_key, nan_key, 0x7fffffff])]).astype(np.int64)
    assert keys.min() >= 0 and keys.max() <= 0x7fffffff
    old, new = old_decision(keys, mt, prec), new_decision(keys, mt, prec)
    for name, o, n in zip(("rho <= v", "!(rho < 1)", "rho <= one_step"), old, new):
        diff = keys[o != n]
        assert diff.size == 0, f"{prec} MT={mt} '{name}': decisions differ at keys {[hex(int(x)) for x in diff[:8]]}"
    # the thresholds sit where the float decision flips (the ±4096 window holds both answers)
    assert old[0][keys == kv].all() and not old[0][keys == kv + 1].any()
    assert old[2][keys == kone].all() and not old[2][keys == kone + 1].any()
    assert not old[1][keys == k1].any() and old[1][keys == k1 + 1].all()
    # +inf and NaN: never accepted, always "no contraction"
    for k in (inf_key, nan_key, 0x7fffffff):
        sel = keys == k
        assert not new[0][sel].any() and new[1][sel].all() and not new[2][sel].any()


def test_thresholds_are_the_kernel_constants():
    """The listing's immediates for the headline grid (fp64, MT = 1): s_cmp against K_v + 1,
    K_1 and K_one_step + 1 — 0x3d65fd7f, 0x3fafffff, 0x3dd12e0b."""
    kv, kone, k1 = thresholds(1, "f64")
    assert (kv + 1, k1, kone + 1) == (0x3d65fd7f, 0x3fafffff, 0x3dd12e0b)
