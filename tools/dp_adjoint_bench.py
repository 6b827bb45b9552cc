#!/usr/bin/env python3
"""Same-run timing of the cross-term DP solve, the costate sweep and the adjoint pass (bench.py has
no flag for them).

One process, one JSON line.  Inputs as tools/dp_value_bench.py forms them (the library's
counter-based generator at seed 20260104; q, r, qf, c from numpy default_rng(seed); a cross term
M = R F with Q ← Q + FᵀRF, formed on the device), every per-knot field its own copy in HBM
(tv_AB = tv_QR = 1); gX, gU ~ N(0, 1) from the seed.  After a warm-up, `--steps` rounds in which

    cross         lqrx_dp_solve_cross                       (the yardstick)
    costates      lqrx_dp_costates on its K, X, U
    adjoint       lqrx_dp_solve_adjoint, all eleven outputs
    adjoint_gx0   lqrx_dp_solve_adjoint, only gx0

run one after the other on a created stream, timed with device events — alternately, so that clock
and thermal drift fall on all alike.  The JSON also carries the bytes the two new kernel groups must
move, computed from the shape (every matrix the sweep reads once: A, B, Q, R, M, K per knot; every
matrix the assembly writes once), and each time as a multiple of those bytes over `--copy-tbs`
(the measured device copy rate, 6.29 TB/s).  A run without a gfx950 device fails.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lqr.jl_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20260104)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--copy-tbs", type=float, default=6.29)
    args = ap.parse_args()
    import numpy as np
    import torch
    import lqrx

    if not torch.cuda.is_available() or lqrx.load().lqrx_device_available() != 1:
        raise RuntimeError("dp_adjoint_bench: no gfx950 device")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    n, m, N, bt, seed = args.n, args.m, args.N, args.batch, args.seed
    host = lqrx.random_batch(n, m, N, bt, seed=seed)
    rng = np.random.default_rng(seed)
    host.update(q=rng.standard_normal(bt * n), r=rng.standard_normal(bt * m), qf=rng.standard_normal(bt * n),
                c=rng.standard_normal(bt * n))
    t = {k: torch.from_numpy(host[k]).to(dev) for k in ("A", "B", "Q", "R", "Qf", "x0", "q", "r", "qf", "c")}
    t.update(n=n, m=m, batch=bt)
    del host
    g = torch.Generator(device=dev).manual_seed(seed)
    Ft = torch.randn(bt, n, m, dtype=torch.float64, device=dev, generator=g) * (0.3 / n ** 0.5)
    Mt = Ft @ t["R"].view(bt, m, m)
    t["Q"] = (t["Q"].view(bt, n, n) + Mt @ Ft.transpose(1, 2)).reshape(-1)
    t["M"] = Mt.reshape(-1)
    del Ft, Mt
    for k in ("A", "B", "Q", "R", "q", "r", "c", "M"):
        v = t[k].view(bt, 1, -1)
        t[k] = v.expand(bt, N - 1, v.shape[-1]).contiguous().view(-1)
    t.update(tv_AB=1, tv_QR=1)
    gX = torch.randn(bt * N * n, dtype=torch.float64, device=dev, generator=g)
    gU = torch.randn(bt * (N - 1) * m, dtype=torch.float64, device=dev, generator=g)
    sh = stream.cuda_stream
    sol = lqrx.dp_solve_device(t, N, stream=sh, costates=True)
    full = lqrx.dp_adjoint_device(t, sol, gX, gU, N=N, stream=sh)
    only = lqrx.dp_adjoint_device(t, sol, gX, gU, want=("x0",), N=N, stream=sh)
    torch.cuda.synchronize(dev)
    same_gx0 = bool(torch.equal(full["x0"], only["x0"]))
    del only

    import ctypes as C

    lib = lqrx.load()
    desc = lqrx._lib.DpDesc(n, m, N, 0, bt, 0, 0, 1, 1)
    ptr = lambda x: C.c_void_p(x.data_ptr())
    G = lqrx._lib.DpGrad(gX.data_ptr(), gU.data_ptr(), *[full[k].data_ptr() for k in lqrx.autograd.GRAD_FIELDS])
    G0 = lqrx._lib.DpGrad(gX.data_ptr(), gU.data_ptr(), *[full[k].data_ptr() if k == "x0" else None
                                                          for k in lqrx.autograd.GRAD_FIELDS])
    st = C.c_void_p(sh)

    def adjoint(gr):
        lqrx._lib.check(lib.lqrx_dp_solve_adjoint(C.byref(desc), ptr(t["A"]), ptr(t["B"]), ptr(t["Q"]), ptr(t["R"]),
                                                  ptr(t["M"]), ptr(t["Qf"]), ptr(sol["X"]), ptr(sol["U"]),
                                                  ptr(sol["lam"]), C.byref(gr), ptr(full["info"]), st))

    def costates():
        lqrx._lib.check(lib.lqrx_dp_costates(C.byref(desc), ptr(t["A"]), ptr(t["B"]), ptr(t["Q"]), ptr(t["R"]),
                                             ptr(t["M"]), ptr(t["Qf"]), ptr(t["q"]), ptr(t["r"]), ptr(t["qf"]),
                                             ptr(sol["K"]), ptr(sol["X"]), ptr(sol["U"]), ptr(sol["lam"]), st))

    variants = {"cross": lambda: lqrx.dp_solve_device(t, N, stream=sh, out=sol), "costates": costates,
                "adjoint": lambda: adjoint(G), "adjoint_gx0": lambda: adjoint(G0)}
    for _ in range(args.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize(dev)
    evs = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
           for k in variants}
    for s in range(args.steps):
        for k, f in variants.items():
            evs[k][s][0].record(stream)
            f()
            evs[k][s][1].record(stream)
    torch.cuda.synchronize(dev)
    res = dict(tool="dp_adjoint_bench", n=n, m=m, N=N, batch=bt, dtype="f64", time_varying=True, steps=args.steps,
               warmup=args.warmup, seed=seed, device=torch.cuda.get_device_name(dev),
               library=lqrx._lib.build_info(), gx0_same_bits=same_gx0,
               bad_info=int((full["info"] != 0).sum().item()),
               peak_allocated_gb=torch.cuda.max_memory_allocated(dev) / 1e9)
    for k in variants:
        ms = sorted(a.elapsed_time(b) for a, b in evs[k])
        res[k + "_ms"] = dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1])
    # bytes that must move (fp64): the sweep reads A, B, Q, R, M, K once per knot and X, U once, writes lam;
    # the assembly writes gA, gB, gQ, gR, gM per knot and reads the six trajectories
    k1 = N - 1
    sweep = 8 * bt * (k1 * (2 * n * n + m * m + 3 * n * m + 2 * n + 2 * m) + n * n + 3 * n * N)
    asm = 8 * bt * (k1 * (2 * n * n + 2 * n * m + m * m + 2 * n + m) + n * n + 3 * n + 2 * (2 * n * N + m * k1))
    floor = lambda b: b / (args.copy_tbs * 1e12) * 1e3
    res["costates_bytes_gb"], res["costates_floor_ms"] = sweep / 1e9, floor(sweep)
    res["assembly_bytes_gb"], res["assembly_floor_ms"] = asm / 1e9, floor(asm)
    res["costates_x_floor"] = res["costates_ms"]["median"] / floor(sweep)
    res["adjoint_minus_cross_ms"] = res["adjoint_ms"]["median"] - res["cross_ms"]["median"]
    res["adjoint_gx0_minus_cross_ms"] = res["adjoint_gx0_ms"]["median"] - res["cross_ms"]["median"]
    # adjoint = repack + cross solve + sweep + assembly: what is left of it beyond the cross solve and one sweep
    res["assembly_est_ms"] = res["adjoint_ms"]["median"] - res["adjoint_gx0_ms"]["median"]
    res["assembly_est_x_floor"] = res["assembly_est_ms"] / floor(asm)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
