#!/usr/bin/env python3
"""Same-run timing of the DP solve kinds (plain ⊂ linear ⊂ affine ⊂ cross ⊂ value): bench.py has a
flag for the first two only.

  tools/dp_kinds_bench.py --kinds linear,affine,cross,value [--sets ti,tv] [--steps 5] [--warmup 1]

One process, one JSON line.  Per shape set: inputs seeded as bench.py seeds them (the library's
counter-based generator at seed 20260104; q, r, qf, then c ~ N(0, 1) from numpy default_rng(seed));
with the cross or value kind among `--kinds`, a cross term that keeps every problem strictly convex,
formed on the device: F ~ 0.3/√n · N(0, 1) per trajectory, M = R F and Q ← Q + FᵀRF (the joint cost
block is congruent to blkdiag(Q, R)) — the kinds below it then run on the same Q, so that cross and
affine differ by M alone.  Every variant is warmed up, then `--steps` rounds in which the solves
(lqrx_dp_solve[_linear|_affine|_cross|_value] through lqrx.dp_solve_device on a created stream) are
timed one after the other with device events — alternately, so that clock and thermal drift fall on
all alike.  They share one set of output buffers.  The value kind is timed twice: "value_noJ"
(val->J = NULL, no dp_value_cost_kernel behind the solve) and "value" (s_1, dV and J all asked for,
the J kernel inside the timed interval).

Keys per set: `<kind>_ms` {median, min, max} and, for kinds timed together, linear_minus_plain_ms,
affine_minus_linear_ms, cross_minus_affine_ms, value_minus_cross_ms, value_noJ_minus_cross_ms — the
keys of the records under profiles/r07/{affine,cross,value}.

Shape sets: "ti" = bench.py --linear (n=32 m=16 N=256 B=65536 fp64, time-invariant), "tv" =
bench.py --tv --linear (B=16384, per-knot A, B, Q, R, q, r, c, M).
A run without a gfx950 device fails.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lqr.jl_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

# the fields each kind adds to the one before it
LADDER = (("plain", ()), ("linear", ("q", "r", "qf")), ("affine", ("c",)), ("cross", ("M",)), ("value", ()))


def run_set(lqrx, torch, dev, stream, kinds, n, m, N, bt, tv, seed, steps, warmup):
    import numpy as np

    host = lqrx.random_batch(n, m, N, bt, seed=seed)
    rng = np.random.default_rng(seed)
    host.update(q=rng.standard_normal(bt * n), r=rng.standard_normal(bt * m), qf=rng.standard_normal(bt * n))
    host["c"] = rng.standard_normal(bt * n)
    t = {k: torch.from_numpy(host[k]).to(dev) for k in ("A", "B", "Q", "R", "Qf", "x0", "q", "r", "qf", "c")}
    t.update(n=n, m=m, batch=bt)
    del host
    if "cross" in kinds or "value" in kinds:
        # the flat column-major m×n block of M viewed (n, m) is Mᵀ = FᵀR (R symmetric)
        g = torch.Generator(device=dev).manual_seed(seed)
        Ft = torch.randn(bt, n, m, dtype=torch.float64, device=dev, generator=g) * (0.3 / n ** 0.5)
        Mt = Ft @ t["R"].view(bt, m, m)
        t["Q"] = (t["Q"].view(bt, n, n) + Mt @ Ft.transpose(1, 2)).reshape(-1)
        t["M"] = Mt.reshape(-1)
        del Ft, Mt
    if tv:   # every knot's block its own copy in HBM, as bench.py --tv
        for k in ("A", "B", "Q", "R", "q", "r", "c", "M"):
            if k in t:
                v = t[k].view(bt, 1, -1)
                t[k] = v.expand(bt, N - 1, v.shape[-1]).contiguous().view(-1)
        t.update(tv_AB=1, tv_QR=1)
    sh = stream.cuda_stream
    # one set of output buffers for all (K alone is 68 GB at the first shape set): those of the
    # highest kind timed
    value = "value" in kinds
    out = lqrx.dp_solve_device(t, N, p_mode=0, stream=sh, value=value)
    variants, has = {}, ()
    for kind, adds in LADDER:     # name → (inputs, value flag, outputs)
        has += adds
        inputs = {k: v for k, v in t.items() if k not in ("q", "r", "qf", "c", "M") or k in has}
        if kind == "value" and value:
            # "value_noJ": val->J = NULL, so no dp_value_cost_kernel behind the solve
            variants["value_noJ"] = (inputs, True, {k: v for k, v in out.items() if k != "J"})
            variants["value"] = (inputs, True, out)
        elif kind in kinds:
            variants[kind] = (inputs, False, out)
    for _ in range(warmup):
        for i, v, o in variants.values():
            lqrx.dp_solve_device(i, N, p_mode=0, stream=sh, out=o, value=v)
    torch.cuda.synchronize(dev)
    evs = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
           for k in variants}
    for s in range(steps):
        for k, (i, v, o) in variants.items():
            evs[k][s][0].record(stream)
            lqrx.dp_solve_device(i, N, p_mode=0, stream=sh, out=o, value=v)
            evs[k][s][1].record(stream)
    torch.cuda.synchronize(dev)
    res = dict(n=n, m=m, N=N, batch=bt, dtype="f64", time_varying=bool(tv))
    for k in variants:
        ms = sorted(a.elapsed_time(b) for a, b in evs[k])
        res[k + "_ms"] = dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1])
    res["bad_info"] = int((out["info"] != 0).sum().item())
    for hi, lo in (("linear", "plain"), ("affine", "linear"), ("cross", "affine"), ("value", "cross"),
                   ("value_noJ", "cross")):
        if hi in variants and lo in variants:
            res[f"{hi}_minus_{lo}_ms"] = res[hi + "_ms"]["median"] - res[lo + "_ms"]["median"]
    if value:
        res["J_mean"] = float(out["J"].mean().item())
        res["dV_min"] = float(out["dV"].min().item())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="linear,affine,cross,value",
                    help="comma-separated, of plain, linear, affine, cross, value")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20260104)
    ap.add_argument("--sets", default="ti,tv")
    ap.add_argument("--batch-ti", type=int, default=65536)
    ap.add_argument("--batch-tv", type=int, default=16384)
    args = ap.parse_args()
    kinds = args.kinds.split(",")
    if not kinds or any(k not in dict(LADDER) for k in kinds):
        ap.error("--kinds takes plain, linear, affine, cross, value")
    import torch
    import lqrx

    if not torch.cuda.is_available() or lqrx.load().lqrx_device_available() != 1:
        raise RuntimeError("dp_kinds_bench: no gfx950 device")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    out = dict(tool="dp_kinds_bench", kinds=kinds, steps=args.steps, warmup=args.warmup, seed=args.seed,
               device=torch.cuda.get_device_name(dev), library=lqrx._lib.build_info(), sets=[])
    for s in args.sets.split(","):
        tv = s == "tv"
        out["sets"].append(run_set(lqrx, torch, dev, stream, kinds, 32, 16, 256,
                                   args.batch_tv if tv else args.batch_ti, tv, args.seed, args.steps, args.warmup))
        torch.cuda.empty_cache()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
