#!/usr/bin/env python3
"""Same-run timing of the scenario rollout (lqrx_dp_rollout) against what a caller had to do without
it: lqrx_dp_solve_cross on the problem replicated to batch·S trajectories.

  tools/dp_rollout_bench.py [--sets ti,tv] [--steps 5] [--warmup 1] [--S 64] [--shape 32,16,256]

One process, one JSON line.  Per shape set (n, m, N of --shape, fp64): the problem of
tools/dp_kinds_bench.py (library generator, q, r, qf, c ~ N(0, 1), a cross term that keeps every
problem strictly convex), solved once by lqrx_dp_solve_cross for the policy (K, d); S scenarios per
problem with x0 ~ N(0, 1), α ~ U[0, 1], w ~ 0.1·N(0, 1) and bounds at ±1.5 × the mean |u| per problem
and control row of the unclamped rollout.  Variants, alternated in every round and timed with device
events: "J" (J only), "XUJ" (X + U + J), each plain (no w, no bounds, α given) and "_bw" (with bounds
and w); and "replicated", the cross solve of the batch·S replicated trajectories from the scenarios' x0.

Per variant: ms {median, min, max}, trajectories per second, the algorithmic HBM bytes (K, A, B, c, d
and, with J, the cost matrices once per problem; x0, α, w, X, U, J per scenario), the fraction of the
6.29 TB/s copy rate they imply, and the ratio replicated / variant.
Shape sets: "ti" = 1024 time-invariant problems × S, "tv" = 256 problems with per-knot A, B, c, Q, R, M, q, r.
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

COPY_RATE = 6.29e12   # bytes / s
PROBLEM = ("A", "B", "Q", "R", "Qf", "x0", "q", "r", "qf", "c", "M")


def problem(lqrx, torch, dev, n, m, N, bt, tv, seed):
    import numpy as np

    host = lqrx.random_batch(n, m, N, bt, seed=seed)
    rng = np.random.default_rng(seed)
    host.update(q=rng.standard_normal(bt * n), r=rng.standard_normal(bt * m), qf=rng.standard_normal(bt * n))
    host["c"] = rng.standard_normal(bt * n)
    t = {k: torch.from_numpy(host[k]).to(dev) for k in PROBLEM if k != "M"}
    g = torch.Generator(device=dev).manual_seed(seed)
    Ft = torch.randn(bt, n, m, dtype=torch.float64, device=dev, generator=g) * (0.3 / n ** 0.5)
    Mt = Ft @ t["R"].view(bt, m, m)   # the flat column-major m×n block of M viewed (n, m) is Mᵀ = FᵀR
    t["Q"] = (t["Q"].view(bt, n, n) + Mt @ Ft.transpose(1, 2)).reshape(-1)
    t["M"] = Mt.reshape(-1)
    if tv:
        for k in ("A", "B", "Q", "R", "q", "r", "c", "M"):
            v = t[k].view(bt, 1, -1)
            t[k] = v.expand(bt, N - 1, v.shape[-1]).contiguous().view(-1)
    t.update(n=n, m=m, batch=bt, tv_AB=int(tv), tv_QR=int(tv))
    return t


def algorithmic_bytes(n, m, N, bt, S, tv, outputs, bw):
    k = N - 1 if tv else 1
    per_problem = (N - 1) * (m * n + m) + k * (n * n + n * m + n)
    if "J" in outputs:
        per_problem += k * (n * n + m * m + m * n + n + m) + n * n + n
    if bw:
        per_problem += 2 * m
    per_scen = n + 1 + ((N - 1) * n if bw else 0)
    per_scen += sum(dict(X=N * n, U=(N - 1) * m, J=1)[o] for o in outputs)
    return 8 * bt * (per_problem + S * per_scen)


def run_set(lqrx, torch, dev, stream, n, m, N, bt, S, tv, seed, steps, warmup, replicated):
    sh = stream.cuda_stream
    t = problem(lqrx, torch, dev, n, m, N, bt, tv, seed)
    sol = lqrx.dp_solve_device(t, N, stream=sh)
    K, d = sol["K"], sol["d"]
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, device=dev, generator=g)
    sc = dict(S=S, x0=rnd(bt * S * n), alpha=torch.rand(bt * S, dtype=torch.float64, device=dev, generator=g))
    w = 0.1 * rnd(bt * S * (N - 1) * n)
    out = lqrx.dp_rollout_device(t, N, K, d, sc, stream=sh)
    hi = 1.5 * out["U"].view(bt, S * (N - 1), m).abs().mean(dim=1).reshape(-1).contiguous()
    bw = dict(w=w, u_lo=-hi, u_hi=hi)
    variants = {}
    for name, outputs in (("J", ("J",)), ("XUJ", ("X", "U", "J"))):
        variants[name] = (dict(sc, outputs=outputs), outputs, False)
        variants[name + "_bw"] = (dict(sc, outputs=outputs, **bw), outputs, True)
    rep = rout = None
    if replicated:   # the same trajectories as batch·S independent problems
        rep = {}
        for k in PROBLEM:
            per = t[k].numel() // bt
            rep[k] = sc["x0"] if k == "x0" else t[k].view(bt, 1, per).expand(bt, S, per).contiguous().view(-1)
        rep.update(n=n, m=m, batch=bt * S, tv_AB=int(tv), tv_QR=int(tv))
        rout = lqrx.dp_solve_device(rep, N, stream=sh)

    def launch(name):
        if name == "replicated":
            lqrx.dp_solve_device(rep, N, stream=sh, out=rout)
        else:
            lqrx.dp_rollout_device(t, N, K, d, variants[name][0], stream=sh, out=out)

    names = list(variants) + (["replicated"] if replicated else [])
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
    res = dict(n=n, m=m, N=N, batch=bt, S=S, trajectories=bt * S, dtype="f64", time_varying=bool(tv))
    ms = {k: sorted(a.elapsed_time(b) for a, b in evs[k]) for k in names}
    for k in names:
        med = ms[k][len(ms[k]) // 2]
        r = dict(ms=dict(median=med, min=ms[k][0], max=ms[k][-1]), trajectories_per_s=bt * S / (med * 1e-3))
        if k != "replicated":
            by = algorithmic_bytes(n, m, N, bt, S, tv, variants[k][1], variants[k][2])
            r.update(hbm_bytes=by, copy_rate_fraction=by / (med * 1e-3) / COPY_RATE)
            if replicated:
                r["replicated_over_this"] = ms["replicated"][len(ms["replicated"]) // 2] / med
        res[k] = r
    if replicated:
        res["bad_info"] = int((rout["info"] != 0).sum().item())
        # the same trajectories: the replicated solve's J-free outputs against the α = 1 rollout
        one = lqrx.dp_rollout_device(t, N, K, d, dict(S=S, x0=sc["x0"], outputs=("X",)), stream=sh)
        torch.cuda.synchronize(dev)
        res["X_vs_replicated_maxabs"] = float((one["X"] - rout["X"]).abs().max().item())
    res["J_mean"] = float(out["J"].mean().item())
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
    ap.add_argument("--no-replicated", action="store_true", help="time the rollout variants alone")
    args = ap.parse_args()
    n, m, N = map(int, args.shape.split(","))
    import torch
    import lqrx

    if not torch.cuda.is_available() or lqrx.load().lqrx_device_available() != 1:
        raise RuntimeError("dp_rollout_bench: no gfx950 device")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    out = dict(tool="dp_rollout_bench", steps=args.steps, warmup=args.warmup, seed=args.seed,
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
