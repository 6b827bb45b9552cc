#!/usr/bin/env python3
"""Same-run timing of factor + re-solve (lqrx_dp_factor, lqrx_dp_resolve) against what a caller had to
do without them: lqrx_dp_solve_cross on the problem replicated to batch·S trajectories.

  tools/dp_resolve_bench.py [--sets ti,tv] [--steps 5] [--warmup 1] [--S 64] [--shape 32,16,256]

One process, one JSON line.  Per shape set (n, m, N of --shape, fp64): the problem of
tools/dp_rollout_bench.py, solved once by lqrx_dp_solve_cross with p_mode 1 for K and every P_k; S
right-hand sides per problem with q, r, qf, x0 ~ N(0, 1) (q, r per knot in the time-varying set).
Variants, alternated in every round and timed with device events: "factor" (lqrx_dp_factor alone),
the re-solve with outputs "dp" (d + p_1), "dXU" (d + X + U) and "dpXU" (all four, p_1), and
"replicated", the cross solve of the batch·S replicated problems with the same right-hand sides —
the library's unchanged solve, timed in the same run.

Per variant: ms {median, min, max}, right-hand sides per second, the algorithmic HBM bytes (factor:
B, R, c, P in, E⁻¹, Pc out; re-solve: per problem A, B, c, Pc, E⁻¹ once and K once per pass, per
right-hand side q, r, qf, x0 in, the outputs out, and d read back when there is a forward pass), the
fraction of the 6.29 TB/s copy rate they imply, and replicated / (factor + variant).
Shape sets: "ti" = 1024 time-invariant problems × S, "tv" = 256 problems with per-knot A, B, c, Q, R, M, q, r.
A run without a gfx950 device fails.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lqr.jl_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dp_rollout_bench import COPY_RATE, PROBLEM, problem   # noqa: E402

VARIANTS = (("dp", ("d", "p")), ("dXU", ("d", "X", "U")), ("dpXU", ("d", "p", "X", "U")))


def factor_bytes(n, m, N, bt, tv):
    k = N - 1 if tv else 1
    return 8 * bt * (k * (n * m + m * m + n) + N * n * n + (N - 1) * (m * m + n))


def resolve_bytes(n, m, N, bt, S, tv, outputs):
    k = N - 1 if tv else 1
    fwd = "X" in outputs or "U" in outputs
    passes = 2 if fwd else 1
    per_problem = passes * ((N - 1) * m * n + k * (n * n + n * m)) + (N - 1) * (m * m + n) + (k * n if fwd else 0)
    per_rhs = k * (n + m) + n + (n if fwd else 0) + ((N - 1) * m if fwd else 0)
    per_rhs += sum(dict(d=(N - 1) * m, p=n, X=N * n, U=(N - 1) * m)[o] for o in outputs)
    return 8 * bt * (per_problem + S * per_rhs)


def run_set(lqrx, torch, dev, stream, n, m, N, bt, S, tv, seed, steps, warmup, replicated):
    sh = stream.cuda_stream
    t = problem(lqrx, torch, dev, n, m, N, bt, tv, seed)
    sol = lqrx.dp_solve_device(t, N, p_mode=1, stream=sh)
    fout = lqrx.dp_factor_device(t, N, sol["P"], stream=sh)
    fac = dict(K=sol["K"], Einv=fout["Einv"], Pc=fout["Pc"])
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, device=dev, generator=g)
    kq = N - 1 if tv else 1
    rhs = dict(S=S, q=rnd(bt * S * kq * n), r=rnd(bt * S * kq * m), qf=rnd(bt * S * n), x0=rnd(bt * S * n), tv_QR=int(tv))
    out = lqrx.dp_resolve_device(t, N, fac, rhs, stream=sh)
    rep = rout = None
    if replicated:   # the same right-hand sides as batch·S independent problems
        rep = {}
        for k in PROBLEM:
            per = t[k].numel() // bt
            rep[k] = rhs[k] if k in ("q", "r", "qf", "x0") else t[k].view(bt, 1, per).expand(bt, S, per).contiguous().view(-1)
        rep.update(n=n, m=m, batch=bt * S, tv_AB=int(tv), tv_QR=int(tv))
        rout = lqrx.dp_solve_device(rep, N, stream=sh)

    def launch(name):
        if name == "replicated":
            lqrx.dp_solve_device(rep, N, stream=sh, out=rout)
        elif name == "factor":
            lqrx.dp_factor_device(t, N, sol["P"], out=fout, stream=sh)
        else:
            lqrx.dp_resolve_device(t, N, fac, dict(rhs, outputs=dict(VARIANTS)[name]), stream=sh, out=out)

    names = ["factor"] + [v for v, _ in VARIANTS] + (["replicated"] if replicated else [])
    for _ in range(warmup):
        for k in names:
            launch(k)
    torch.cuda.synchronize(dev)
    evs = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
           for k in names}
    for s in range(steps):
        for k in names:
            evs[k][s][0].record(stream)
            launch(k)
            evs[k][s][1].record(stream)
    torch.cuda.synchronize(dev)
    res = dict(n=n, m=m, N=N, batch=bt, S=S, right_hand_sides=bt * S, dtype="f64", time_varying=bool(tv))
    ms = {k: sorted(a.elapsed_time(b) for a, b in evs[k]) for k in names}
    med = {k: ms[k][len(ms[k]) // 2] for k in names}
    for k in names:
        r = dict(ms=dict(median=med[k], min=ms[k][0], max=ms[k][-1]))
        if k == "factor":
            by = factor_bytes(n, m, N, bt, tv)
            r.update(problems_per_s=bt / (med[k] * 1e-3), hbm_bytes=by, copy_rate_fraction=by / (med[k] * 1e-3) / COPY_RATE)
        else:
            r["right_hand_sides_per_s"] = bt * S / (med[k] * 1e-3)
        if k in dict(VARIANTS):
            by = resolve_bytes(n, m, N, bt, S, tv, dict(VARIANTS)[k])
            r.update(hbm_bytes=by, copy_rate_fraction=by / (med[k] * 1e-3) / COPY_RATE)
            if replicated:
                r["replicated_over_factor_plus_this"] = med["replicated"] / (med["factor"] + med[k])
                r["replicated_over_this"] = med["replicated"] / med[k]
        res[k] = r
    res["factor_bad_info"] = int((fout["info"] != 0).sum().item())
    if replicated:   # the same right-hand sides: the replicated solve's outputs against the re-solve's
        res["bad_info"] = int((rout["info"] != 0).sum().item())
        full = lqrx.dp_resolve_device(t, N, fac, rhs, stream=sh)
        torch.cuda.synchronize(dev)
        for k in ("d", "p", "X", "U"):
            res[k + "_vs_replicated_maxabs"] = float((full[k] - rout[k]).abs().max().item())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20260104)
    ap.add_argument("--sets", default="ti,tv")
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--batch-ti", type=int, default=1024)
    ap.add_argument("--batch-tv", type=int, default=256)
    ap.add_argument("--shape", default="32,16,256", help="n,m,N of both shape sets")
    ap.add_argument("--no-replicated", action="store_true", help="time the factor and the re-solve variants alone")
    args = ap.parse_args()
    n, m, N = map(int, args.shape.split(","))
    import torch
    import lqrx

    if not torch.cuda.is_available() or lqrx.load().lqrx_device_available() != 1:
        raise RuntimeError("dp_resolve_bench: no gfx950 device")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    out = dict(tool="dp_resolve_bench", steps=args.steps, warmup=args.warmup, seed=args.seed,
               device=torch.cuda.get_device_name(dev), library=lqrx._lib.build_info(), sets=[])
    for s in args.sets.split(","):
        tv = s == "tv"
        out["sets"].append(run_set(lqrx, torch, dev, stream, n, m, N, args.batch_tv if tv else args.batch_ti,
                                   args.S, tv, args.seed, args.steps, args.warmup, not args.no_replicated))
        torch.cuda.empty_cache()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
