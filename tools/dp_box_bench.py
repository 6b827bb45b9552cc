#!/usr/bin/env python3
"""Same-run timing of the fused input-bounds kernel (lqrx_dp_resolve_box) against the loop a caller had to
compose without it, and of its early stopping.

  tools/dp_box_bench.py [--sets ti,tv] [--steps 5] [--warmup 1] [--S 64] [--shape 32,16,256] [--iters 50] [--max-iter 500] [--eps 1e-6]

One process, one JSON line.  Per shape set (n, m, N of --shape, fp64): the problem of
tools/dp_rollout_bench.py, solved once by lqrx_dp_solve_cross with R + ρI (ρ = 1) and p_mode 1 and factored by
lqrx_dp_factor; S instances per problem with q, r, qf, x0 ~ N(0, 1); bounds at ± half the peak of each problem's
unconstrained controls (from the factors of R itself), the lower side of input 0 left open.  Every run starts
cold (Z = W = 0, zeroed outside the timed interval).  Variants, alternated in every round and timed with device
events:

  (a) "fused"     lqrx_dp_resolve_box, eps = 0, max_iter = --iters, outputs d, X, U, iters, res
      "composed"  --iters × (r̂ = r − ρ(z − w), lqrx_dp_resolve for d, X, U, then û, z⁺ = clamp(û + w), w⁺ as
                  torch element-wise kernels), outputs preallocated, no host synchronise inside.  lqrx_dp_resolve takes a
                  knot axis on q and r together, so the composed loop carries q expanded over the knots.
  (b) "early"     the fused kernel with eps = --eps and max_iter = --max-iter; the distribution of `iters`
      "full"      the fused kernel with eps = 0 and max_iter = the largest `iters` "early" returned

Per variant: ms {median, min, max}.  For the fused kernel also the algorithmic HBM bytes per iteration (per
problem K, A, B once per pass, E⁻¹, Pc, c, the bounds; per instance q, r, qf, x0, z and w read in both passes and
written once, d written and read back, X and U written) and the fraction of the 6.29 TB/s copy rate they imply.
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

from dp_rollout_bench import COPY_RATE, problem   # noqa: E402

RHO, RELAX = 1.0, 1.6


def box_bytes_per_iteration(n, m, N, bt, S, tv):
    k = N - 1 if tv else 1
    per_problem = 2 * ((N - 1) * m * n + k * (n * n + n * m)) + (N - 1) * (m * m + n) + k * n + 2 * m
    per_instance = k * (n + m) + 2 * n + 8 * (N - 1) * m + N * n + (N - 1) * m
    return 8 * bt * (per_problem + S * per_instance)


def run_set(lqrx, torch, dev, stream, n, m, N, bt, S, tv, seed, steps, warmup, iters, max_iter, eps):
    sh = stream.cuda_stream
    f8 = torch.float64
    t = problem(lqrx, torch, dev, n, m, N, bt, tv, seed)
    tr = dict(t, R=(t["R"].view(-1, m, m) + RHO * torch.eye(m, dtype=f8, device=dev)).reshape(-1))

    def factors(tt):
        sol = lqrx.dp_solve_device(tt, N, p_mode=1, stream=sh)
        fo = lqrx.dp_factor_device(tt, N, sol["P"], stream=sh)
        bad = int((sol["info"] != 0).sum().item()) + int((fo["info"] != 0).sum().item())
        return dict(K=sol["K"], Einv=fo["Einv"], Pc=fo["Pc"]), bad

    fac, bad = factors(tr)
    fac0, bad0 = factors(t)
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    rnd = lambda *s: torch.randn(*s, dtype=f8, device=dev, generator=g)
    kq = N - 1 if tv else 1
    rhs = dict(S=S, q=rnd(bt * S * kq * n), r=rnd(bt * S * kq * m), qf=rnd(bt * S * n), x0=rnd(bt * S * n), tv_QR=int(tv))
    nu = bt * S * (N - 1) * m
    out = dict(d=torch.empty(nu, dtype=f8, device=dev), X=torch.empty(bt * S * N * n, dtype=f8, device=dev),
               U=torch.empty(nu, dtype=f8, device=dev), iters=torch.empty(bt * S, dtype=torch.int32, device=dev),
               res=torch.empty(2 * bt * S, dtype=f8, device=dev))
    lqrx.dp_resolve_device(t, N, fac0, dict(rhs, outputs=("d", "U")), stream=sh, out=out)
    peak = out["U"].view(bt, -1).abs().amax(dim=1)
    hi = (0.5 * peak)[:, None].expand(bt, m).contiguous()
    lo = -hi.clone()
    lo[:, 0] = float("-inf")
    del fac0
    Z, W = torch.zeros(nu, dtype=f8, device=dev), torch.zeros(nu, dtype=f8, device=dev)
    box = dict(rho=RHO, relax=RELAX, u_lo=lo.view(-1), u_hi=hi.view(-1), Z=Z, W=W)

    def fused(e, it):
        return lqrx.dp_box_device(t, N, fac, rhs, dict(box, eps_prim=e, eps_dual=e, max_iter=it), stream=sh, out=out)

    # the composed loop: q, r with a knot axis (r̂ has one), everything preallocated
    cq = rhs["q"] if tv else rhs["q"].view(bt * S, 1, n).expand(bt * S, N - 1, n).contiguous().view(-1)
    r4 = rhs["r"].view(bt, S, kq, m)
    rhat, tmp, uh = (torch.empty(nu, dtype=f8, device=dev) for _ in range(3))
    Zc, Wc = torch.zeros(nu, dtype=f8, device=dev), torch.zeros(nu, dtype=f8, device=dev)
    crhs = dict(S=S, q=cq, r=rhat, qf=rhs["qf"], x0=rhs["x0"], tv_QR=1, outputs=("d", "X", "U"))
    cout = dict(d=torch.empty(nu, dtype=f8, device=dev), X=torch.empty(bt * S * N * n, dtype=f8, device=dev),
                U=torch.empty(nu, dtype=f8, device=dev))
    v4 = lambda x: x.view(bt, S, N - 1, m)
    lo4, hi4 = lo.view(bt, 1, 1, m), hi.view(bt, 1, 1, m)

    def composed(it):
        for _ in range(it):
            torch.sub(Zc, Wc, out=tmp)
            torch.sub(r4, v4(tmp), alpha=RHO, out=v4(rhat))
            lqrx.dp_resolve_device(t, N, fac, crhs, stream=sh, out=cout)
            torch.mul(cout["U"], RELAX, out=uh)
            uh.add_(Zc, alpha=1.0 - RELAX)
            torch.add(uh, Wc, out=tmp)
            Wc.add_(uh)
            torch.clamp(v4(tmp), min=lo4, max=hi4, out=v4(Zc))
            Wc.sub_(Zc)

    res = dict(n=n, m=m, N=N, batch=bt, S=S, instances=bt * S, dtype="f64", time_varying=bool(tv), rho=RHO, relax=RELAX,
               bad_info=bad + bad0, iterations=iters)

    def cold():
        for x in (Z, W, Zc, Wc):
            x.zero_()

    # the distribution of iters under early stopping, and the two variants at equal iteration count, checked
    cold()
    fused(eps, max_iter)
    torch.cuda.synchronize(dev)
    it = out["iters"].to(torch.float64)
    longest = int(it.max().item())
    res["early_iters"] = dict(median=float(it.median().item()), max=longest, mean=float(it.mean().item()),
                              share_stopped_by_50=float((it <= 50).double().mean().item()),
                              share_at_max_iter=float((it >= max_iter).double().mean().item()), eps=eps, max_iter=max_iter)
    cold()
    fused(0.0, iters)
    composed(iters)
    torch.cuda.synchronize(dev)
    res["composed_vs_fused_Z_maxabs"] = float((Z - Zc).abs().max().item())
    res["composed_vs_fused_W_maxabs"] = float((W - Wc).abs().max().item())

    launch = dict(fused=lambda: fused(0.0, iters), composed=lambda: composed(iters), early=lambda: fused(eps, max_iter),
                  full=lambda: fused(0.0, longest))
    names = list(launch)
    for _ in range(warmup):
        for k in names:
            cold()
            launch[k]()
    torch.cuda.synchronize(dev)
    evs = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
           for k in names}
    for s in range(steps):
        for k in names:
            cold()
            evs[k][s][0].record(stream)
            launch[k]()
            evs[k][s][1].record(stream)
    torch.cuda.synchronize(dev)
    ms = {k: sorted(a.elapsed_time(b) for a, b in evs[k]) for k in names}
    med = {k: ms[k][len(ms[k]) // 2] for k in names}
    for k in names:
        res[k] = dict(ms=dict(median=med[k], min=ms[k][0], max=ms[k][-1]))
    by = box_bytes_per_iteration(n, m, N, bt, S, tv)
    res["fused"].update(ms_per_iteration=med["fused"] / iters, hbm_bytes_per_iteration=by,
                        copy_rate_fraction=by * iters / (med["fused"] * 1e-3) / COPY_RATE)
    res["composed"]["over_fused"] = med["composed"] / med["fused"]
    res["full"].update(max_iter=longest, over_early=med["full"] / med["early"])
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
    ap.add_argument("--N", type=int, help="overrides the N of --shape")
    ap.add_argument("--iters", type=int, default=50, help="iterations of the fused / composed comparison")
    ap.add_argument("--max-iter", type=int, default=500)
    ap.add_argument("--eps", type=float, default=1e-6)
    args = ap.parse_args()
    n, m, N = map(int, args.shape.split(","))
    N = args.N or N
    import torch
    import lqrx

    if not torch.cuda.is_available() or lqrx.load().lqrx_device_available() != 1:
        raise RuntimeError("dp_box_bench: no gfx950 device")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    out = dict(tool="dp_box_bench", steps=args.steps, warmup=args.warmup, seed=args.seed,
               device=torch.cuda.get_device_name(dev), library=lqrx._lib.build_info(), sets=[])
    for s in args.sets.split(","):
        tv = s == "tv"
        out["sets"].append(run_set(lqrx, torch, dev, stream, n, m, N, args.batch_tv if tv else args.batch_ti,
                                   args.S, tv, args.seed, args.steps, args.warmup, args.iters, args.max_iter, args.eps))
        torch.cuda.empty_cache()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
