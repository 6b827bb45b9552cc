// api_san_main.cpp — host-side sanitizer driver for the C ABI (SURVEY §5 "race detection /
// sanitizers").  Built by `make -C lqr.jl_amd/csrc asan`: lqrx_api.cpp compiled with
// AddressSanitizer + UBSan on the HOST side only (-Xarch_host; the kernels are the normal
// objects, GPU sanitizers are not available on this pool), linked into this program and run
// by tests/test_sanitizers.py on the CPU.  It drives everything the ABI does on the host
// without a GPU: argument validation of every entry point (LAPACK-style codes), the KKT
// block-structure layout / packing arithmetic (lqrx_kkt_sizes, workspace sizes), the
// counter-based problem generator (shard consistency), LS sizing, and the last-error
// buffer truncation.  With no device the device-touching paths must fail cleanly with
// LQRX_ERR_HIP / LQRX_ERR_NODEVICE rather than touch memory they do not own.
#include "../../include/lqrx.h"
#include "lqrx_internal.h"

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static int fails = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s (last error: %s)\n", __FILE__, __LINE__, \
                         #cond, lqrx_last_error());                                              \
            ++fails;                                                                             \
        }                                                                                        \
    } while (0)

static void dubins(int N, std::vector<int32_t> &n1, std::vector<int32_t> &p, std::vector<int32_t> &n2,
                   std::vector<int32_t> &w)
{
    n1.assign(N, 3); p.assign(N, 0); n2.assign(N, 3); w.assign(N, 5);
    n1[0] = 0; p[0] = 3; p[N - 1] = 3; n2[N - 1] = 0; w[N - 1] = 3;
}

// ---- NULL sweep of the DP solve entries (plain, linear, affine, cross, value; device and _host) ----
// One set of pointers by name; each entry's argument order behind desc as in include/lqrx.h.
struct DpSlots {
    const void *A, *B, *c, *Q, *R, *M, *Qf, *x0;
    lqrx_dp_linear lin;
    lqrx_dp_value val;
    void *K, *P, *X, *U;
    bool no_lin, no_val;
};
static const char *const dp_order[5] = {"A B Q R Qf x0 K P X U", "A B Q R Qf x0 lin K P X U", "A B c Q R Qf x0 lin K P X U",
                                        "A B c Q R M Qf x0 lin K P X U", "A B c Q R M Qf x0 lin val K P X U"};
static const struct { const char *name; size_t off; } dp_slot[] = {
    {"A", offsetof(DpSlots, A)}, {"B", offsetof(DpSlots, B)}, {"c", offsetof(DpSlots, c)}, {"Q", offsetof(DpSlots, Q)},
    {"R", offsetof(DpSlots, R)}, {"M", offsetof(DpSlots, M)}, {"Qf", offsetof(DpSlots, Qf)}, {"x0", offsetof(DpSlots, x0)},
    {"K", offsetof(DpSlots, K)}, {"P", offsetof(DpSlots, P)}, {"X", offsetof(DpSlots, X)}, {"U", offsetof(DpSlots, U)},
    {"lin->q", offsetof(DpSlots, lin.q)}, {"lin->r", offsetof(DpSlots, lin.r)}, {"lin->qf", offsetof(DpSlots, lin.qf)},
    {"lin->d", offsetof(DpSlots, lin.d)}, {"lin->p", offsetof(DpSlots, lin.p)}, {"val->s", offsetof(DpSlots, val.s)},
    {"val->dV", offsetof(DpSlots, val.dV)}, {"val->J", offsetof(DpSlots, val.J)}};

static DpSlots dp_without(DpSlots s, const std::string &name)
{
    if (name == "lin") s.no_lin = true;
    if (name == "val") s.no_val = true;
    for (const auto &e : dp_slot)
        if (name == e.name) std::memset(reinterpret_cast<char *>(&s) + e.off, 0, sizeof(void *));
    return s;
}

static int dp_call(int kind, bool host, const lqrx_dp_desc *d, const DpSlots &s, int32_t *info)
{
    const lqrx_dp_linear *lin = s.no_lin ? nullptr : &s.lin;
    const lqrx_dp_value *val = s.no_val ? nullptr : &s.val;
    switch (kind) {
    case 0: return host ? lqrx_dp_solve_host(d, s.A, s.B, s.Q, s.R, s.Qf, s.x0, s.K, s.P, s.X, s.U, info)
                        : lqrx_dp_solve(d, s.A, s.B, s.Q, s.R, s.Qf, s.x0, s.K, s.P, s.X, s.U, info, nullptr);
    case 1: return host ? lqrx_dp_solve_linear_host(d, s.A, s.B, s.Q, s.R, s.Qf, s.x0, lin, s.K, s.P, s.X, s.U, info)
                        : lqrx_dp_solve_linear(d, s.A, s.B, s.Q, s.R, s.Qf, s.x0, lin, s.K, s.P, s.X, s.U, info, nullptr);
    case 2: return host ? lqrx_dp_solve_affine_host(d, s.A, s.B, s.c, s.Q, s.R, s.Qf, s.x0, lin, s.K, s.P, s.X, s.U, info)
                        : lqrx_dp_solve_affine(d, s.A, s.B, s.c, s.Q, s.R, s.Qf, s.x0, lin, s.K, s.P, s.X, s.U, info, nullptr);
    case 3: return host ? lqrx_dp_solve_cross_host(d, s.A, s.B, s.c, s.Q, s.R, s.M, s.Qf, s.x0, lin, s.K, s.P, s.X, s.U, info)
                        : lqrx_dp_solve_cross(d, s.A, s.B, s.c, s.Q, s.R, s.M, s.Qf, s.x0, lin, s.K, s.P, s.X, s.U, info, nullptr);
    default: return host ? lqrx_dp_solve_value_host(d, s.A, s.B, s.c, s.Q, s.R, s.M, s.Qf, s.x0, lin, val, s.K, s.P, s.X, s.U, info)
                         : lqrx_dp_solve_value(d, s.A, s.B, s.c, s.Q, s.R, s.M, s.Qf, s.x0, lin, val, s.K, s.P, s.X, s.U, info, nullptr);
    }
}

// Every pointer NULL in turn, and each member of lin and val: minus the argument's position, with
// the argument's name in the text, decided before any device call (so also with no device — the
// plain and linear _host entries included).  val->dV and val->J may be NULL.
static void dp_null_sweep(double *buf, int32_t *info)
{
    lqrx_dp_desc d{};
    d.n = 8; d.m = 4; d.N = 10; d.dtype = LQRX_F64; d.batch = 4;
    const DpSlots full{buf, buf, buf, buf, buf, buf, buf, buf, {buf, buf, buf, buf, buf}, {buf, buf, buf},
                       buf, buf, buf, buf, false, false};
    for (int kind = 0; kind < 5; ++kind)
        for (int host = 0; host < 2; ++host) {
            std::vector<std::string> order;
            for (const char *p = dp_order[kind]; *p;) {
                const char *e = std::strchr(p, ' ');
                order.emplace_back(p, e ? e : p + std::strlen(p));
                p = e ? e + 1 : p + std::strlen(p);
            }
            int posU = 0;
            for (size_t i = 0; i < order.size(); ++i) {
                const int pos = (int)i + 2;              // desc is argument 1
                std::vector<std::string> names{order[i]};
                if (order[i] == "lin") names.insert(names.end(), {"lin->q", "lin->r", "lin->qf", "lin->d", "lin->p"});
                if (order[i] == "val") names.push_back("val->s");
                if (order[i] == "U") posU = pos;
                for (const std::string &nm : names) {
                    const int rc = dp_call(kind, host, &d, dp_without(full, nm), info);
                    if (rc != -pos || !std::strstr(lqrx_last_error(), nm.c_str())) {
                        std::fprintf(stderr, "NULL sweep: kind %d host %d %s NULL: got %d (%s), expected %d\n", kind, host,
                                     nm.c_str(), rc, lqrx_last_error(), -pos);
                        ++fails;
                    }
                }
            }
            if (kind == 4) CHECK(dp_call(kind, host, &d, dp_without(dp_without(dp_without(full, "val->dV"), "val->J"), "U"), info) == -posU);
            CHECK(dp_call(kind, host, nullptr, full, info) == -1);
            lqrx_dp_desc bad = d;
            bad.n = 0;                                   // the descriptor comes first, lin == NULL or not
            CHECK(dp_call(kind, host, &bad, dp_without(full, "lin"), info) == -1);
            bad = d;
            bad.batch = 0;                               // empty batch: a no-op whatever the pointers
            CHECK(dp_call(kind, host, &bad, DpSlots{}, info) == 0);
        }
}

// ---- lqrx_dp_rollout[_host]: every required pointer NULL in turn, bad S, no output, J without its
// cost — minus the argument's position (A 2, B 3, K 5, cost 7, sc 8), decided with no device ----
static int rollout_call(bool host, const lqrx_dp_desc *d, const void *A, const void *B, const void *c, const void *K,
                        const void *dd, const lqrx_dp_cost *cost, const lqrx_dp_scenarios *sc)
{
    return host ? lqrx_dp_rollout_host(d, A, B, c, K, dd, cost, sc) : lqrx_dp_rollout(d, A, B, c, K, dd, cost, sc, nullptr);
}

static void rollout_sweep(double *buf)
{
    lqrx_dp_desc d{};
    d.n = 8; d.m = 4; d.N = 10; d.dtype = LQRX_F64; d.batch = 4;
    const lqrx_dp_cost cost{buf, buf, buf, buf, buf, buf, buf};
    const lqrx_dp_scenarios sc{5, buf, buf, buf, buf, buf, buf, buf, buf};
    for (int host = 0; host < 2; ++host) {
        CHECK(rollout_call(host, nullptr, buf, buf, buf, buf, buf, &cost, &sc) == -1);
        CHECK(rollout_call(host, &d, nullptr, buf, buf, buf, buf, &cost, &sc) == -2 && std::strstr(lqrx_last_error(), "A"));
        CHECK(rollout_call(host, &d, buf, nullptr, buf, buf, buf, &cost, &sc) == -3 && std::strstr(lqrx_last_error(), "B"));
        CHECK(rollout_call(host, &d, buf, buf, buf, nullptr, buf, &cost, &sc) == -5 && std::strstr(lqrx_last_error(), "K"));
        CHECK(rollout_call(host, &d, buf, buf, buf, buf, buf, nullptr, &sc) == -7 && std::strstr(lqrx_last_error(), "cost"));
        CHECK(rollout_call(host, &d, buf, buf, buf, buf, buf, &cost, nullptr) == -8 && std::strstr(lqrx_last_error(), "sc"));
        lqrx_dp_cost cb = cost; cb.Q = nullptr;
        CHECK(rollout_call(host, &d, buf, buf, buf, buf, buf, &cb, &sc) == -7 && std::strstr(lqrx_last_error(), "cost->Q"));
        cb = cost; cb.R = nullptr;
        CHECK(rollout_call(host, &d, buf, buf, buf, buf, buf, &cb, &sc) == -7 && std::strstr(lqrx_last_error(), "cost->R"));
        cb = cost; cb.Qf = nullptr;
        CHECK(rollout_call(host, &d, buf, buf, buf, buf, buf, &cb, &sc) == -7 && std::strstr(lqrx_last_error(), "cost->Qf"));
        lqrx_dp_scenarios sb = sc; sb.S = 0;
        CHECK(rollout_call(host, &d, buf, buf, buf, buf, buf, &cost, &sb) == -8 && std::strstr(lqrx_last_error(), "sc->S"));
        sb = sc; sb.S = -3;
        CHECK(rollout_call(host, &d, buf, buf, buf, buf, buf, &cost, &sb) == -8 && std::strstr(lqrx_last_error(), "sc->S"));
        sb = sc; sb.x0 = nullptr;
        CHECK(rollout_call(host, &d, buf, buf, buf, buf, buf, &cost, &sb) == -8 && std::strstr(lqrx_last_error(), "sc->x0"));
        sb = sc; sb.X = sb.U = sb.J = nullptr;
        CHECK(rollout_call(host, &d, buf, buf, buf, buf, buf, nullptr, &sb) == -8 && std::strstr(lqrx_last_error(), "sc->X"));
        lqrx_dp_desc bad = d;
        bad.layout = 1;
        CHECK(rollout_call(host, &bad, buf, buf, buf, buf, buf, &cost, &sc) == LQRX_ERR_UNSUPPORTED);
        bad = d; bad.n = 0;
        CHECK(rollout_call(host, &bad, nullptr, buf, buf, buf, buf, &cost, &sc) == -1);
        bad = d; bad.p_mode = 7;                         // p_mode is ignored: the next check answers
        CHECK(rollout_call(host, &bad, nullptr, buf, buf, buf, buf, &cost, &sc) == -2);
        bad = d; bad.batch = 0;                          // empty batch: a no-op whatever the pointers
        CHECK(rollout_call(host, &bad, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    }
}

// ---- lqrx_dp_factor[_host], lqrx_dp_resolve[_host]: every required pointer NULL in turn, bad S, no output, X
// without d, the c / Pc mismatch, the unsupported shapes, p_mode and layout — minus the argument's position
// (factor: B 2, R 3, P 5, Einv 6, Pc 7; resolve: A 2, B 3, fac 5, rhs 6), decided with no device ----
static int factor_call(bool host, const lqrx_dp_desc *d, const void *B, const void *R, const void *c, const void *P,
                       void *Einv, void *Pc, int32_t *info)
{
    return host ? lqrx_dp_factor_host(d, B, R, c, P, Einv, Pc, info) : lqrx_dp_factor(d, B, R, c, P, Einv, Pc, info, nullptr);
}

static int resolve_call(bool host, const lqrx_dp_desc *d, const void *A, const void *B, const void *c,
                        const lqrx_dp_factors *fac, const lqrx_dp_rhs *rhs)
{
    return host ? lqrx_dp_resolve_host(d, A, B, c, fac, rhs) : lqrx_dp_resolve(d, A, B, c, fac, rhs, nullptr);
}

static void resolve_sweep(double *buf, int32_t *info)
{
    lqrx_dp_desc d{};
    d.n = 8; d.m = 4; d.N = 10; d.dtype = LQRX_F64; d.batch = 4; d.p_mode = 1;
    const lqrx_dp_factors fac{buf, buf, buf};
    const lqrx_dp_rhs rhs{5, buf, buf, buf, buf, buf, buf, buf, buf};
    for (int host = 0; host < 2; ++host) {
        // the factor
        CHECK(factor_call(host, nullptr, buf, buf, buf, buf, buf, buf, info) == -1);
        CHECK(factor_call(host, &d, nullptr, buf, buf, buf, buf, buf, info) == -2 && std::strstr(lqrx_last_error(), "B"));
        CHECK(factor_call(host, &d, buf, nullptr, buf, buf, buf, buf, info) == -3 && std::strstr(lqrx_last_error(), "R"));
        CHECK(factor_call(host, &d, buf, buf, buf, nullptr, buf, buf, info) == -5 && std::strstr(lqrx_last_error(), "P"));
        CHECK(factor_call(host, &d, buf, buf, buf, buf, nullptr, buf, info) == -6 && std::strstr(lqrx_last_error(), "Einv"));
        CHECK(factor_call(host, &d, buf, buf, buf, buf, buf, nullptr, info) == -7 && std::strstr(lqrx_last_error(), "Pc"));
        CHECK(factor_call(host, &d, buf, buf, nullptr, buf, buf, buf, info) == -7 && std::strstr(lqrx_last_error(), "Pc"));
        lqrx_dp_desc bad = d;
        bad.p_mode = 0;
        CHECK(factor_call(host, &bad, buf, buf, buf, buf, buf, buf, info) == LQRX_ERR_UNSUPPORTED);
        bad = d; bad.layout = 1;
        CHECK(factor_call(host, &bad, buf, buf, buf, buf, buf, buf, info) == LQRX_ERR_UNSUPPORTED);
        bad = d; bad.n = 65;
        CHECK(factor_call(host, &bad, buf, buf, buf, buf, buf, buf, info) == LQRX_ERR_UNSUPPORTED);
        bad = d; bad.m = 33;
        CHECK(factor_call(host, &bad, buf, buf, buf, buf, buf, buf, info) == LQRX_ERR_UNSUPPORTED);
        bad = d; bad.n = 0;
        CHECK(factor_call(host, &bad, nullptr, buf, buf, buf, buf, buf, info) == -1);
        bad = d; bad.batch = 0;                          // empty batch: a no-op whatever the pointers
        CHECK(factor_call(host, &bad, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
        // the re-solve
        CHECK(resolve_call(host, nullptr, buf, buf, buf, &fac, &rhs) == -1);
        CHECK(resolve_call(host, &d, nullptr, buf, buf, &fac, &rhs) == -2 && std::strstr(lqrx_last_error(), "A"));
        CHECK(resolve_call(host, &d, buf, nullptr, buf, &fac, &rhs) == -3 && std::strstr(lqrx_last_error(), "B"));
        CHECK(resolve_call(host, &d, buf, buf, buf, nullptr, &rhs) == -5 && std::strstr(lqrx_last_error(), "fac"));
        CHECK(resolve_call(host, &d, buf, buf, buf, &fac, nullptr) == -6 && std::strstr(lqrx_last_error(), "rhs"));
        lqrx_dp_factors fb = fac; fb.K = nullptr;
        CHECK(resolve_call(host, &d, buf, buf, buf, &fb, &rhs) == -5 && std::strstr(lqrx_last_error(), "fac->K"));
        fb = fac; fb.Einv = nullptr;
        CHECK(resolve_call(host, &d, buf, buf, buf, &fb, &rhs) == -5 && std::strstr(lqrx_last_error(), "fac->Einv"));
        fb = fac; fb.Pc = nullptr;                       // c without Pc, and Pc without c
        CHECK(resolve_call(host, &d, buf, buf, buf, &fb, &rhs) == -5 && std::strstr(lqrx_last_error(), "fac->Pc"));
        CHECK(resolve_call(host, &d, buf, buf, nullptr, &fac, &rhs) == -5 && std::strstr(lqrx_last_error(), "fac->Pc"));
        lqrx_dp_rhs rb = rhs; rb.S = 0;
        CHECK(resolve_call(host, &d, buf, buf, buf, &fac, &rb) == -6 && std::strstr(lqrx_last_error(), "rhs->S"));
        rb = rhs; rb.S = -3;
        CHECK(resolve_call(host, &d, buf, buf, buf, &fac, &rb) == -6 && std::strstr(lqrx_last_error(), "rhs->S"));
        rb = rhs; rb.d = rb.p = rb.X = rb.U = nullptr;
        CHECK(resolve_call(host, &d, buf, buf, buf, &fac, &rb) == -6 && std::strstr(lqrx_last_error(), "rhs->d"));
        rb = rhs; rb.d = nullptr;                        // X (and U) without d
        CHECK(resolve_call(host, &d, buf, buf, buf, &fac, &rb) == -6 && std::strstr(lqrx_last_error(), "rhs->X"));
        rb.X = nullptr;
        CHECK(resolve_call(host, &d, buf, buf, buf, &fac, &rb) == -6 && std::strstr(lqrx_last_error(), "rhs->U"));
        rb = rhs; rb.q = rb.r = rb.qf = rb.x0 = nullptr; // optional inputs: the next check answers
        CHECK(resolve_call(host, &d, nullptr, buf, buf, &fac, &rb) == -2);
        bad = d; bad.layout = 1;
        CHECK(resolve_call(host, &bad, buf, buf, buf, &fac, &rhs) == LQRX_ERR_UNSUPPORTED);
        bad = d; bad.n = 65;
        CHECK(resolve_call(host, &bad, buf, buf, buf, &fac, &rhs) == LQRX_ERR_UNSUPPORTED);
        bad = d; bad.m = 33;
        CHECK(resolve_call(host, &bad, buf, buf, buf, &fac, &rhs) == LQRX_ERR_UNSUPPORTED);
        bad = d; bad.p_mode = 0;                         // both p modes are served
        CHECK(resolve_call(host, &bad, nullptr, buf, buf, &fac, &rhs) == -2);
        bad = d; bad.batch = 0;
        CHECK(resolve_call(host, &bad, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    }
}

// ---- lqrx_dp_resolve_box[_host]: every required pointer NULL in turn, the members of rhs and box the entry
// refuses, the ends of the ranges, the unsupported shapes — minus the argument's position (A 2, B 3, fac 5,
// rhs 6, box 7), decided with no device ----
static int box_call(bool host, const lqrx_dp_desc *d, const void *A, const void *B, const void *c,
                    const lqrx_dp_factors *fac, const lqrx_dp_rhs *rhs, const lqrx_dp_box *box)
{
    return host ? lqrx_dp_resolve_box_host(d, A, B, c, fac, rhs, box) : lqrx_dp_resolve_box(d, A, B, c, fac, rhs, box, nullptr);
}

static void box_sweep(double *buf, int32_t *info)
{
    lqrx_dp_desc d{};
    d.n = 8; d.m = 4; d.N = 10; d.dtype = LQRX_F64; d.batch = 4;
    const lqrx_dp_factors fac{buf, buf, buf};
    const lqrx_dp_rhs rhs{5, buf, buf, buf, buf, buf, nullptr, buf, buf};
    const lqrx_dp_box box{1.0, 1.6, 1e-6, 1e-6, 100, buf, buf, buf, buf, info, buf};
    const double nan = std::nan(""), inf = HUGE_VAL;
    for (int host = 0; host < 2; ++host) {
        CHECK(box_call(host, nullptr, buf, buf, buf, &fac, &rhs, &box) == -1);
        CHECK(box_call(host, &d, nullptr, buf, buf, &fac, &rhs, &box) == -2 && std::strstr(lqrx_last_error(), "A"));
        CHECK(box_call(host, &d, buf, nullptr, buf, &fac, &rhs, &box) == -3 && std::strstr(lqrx_last_error(), "B"));
        CHECK(box_call(host, &d, buf, buf, buf, nullptr, &rhs, &box) == -5 && std::strstr(lqrx_last_error(), "fac"));
        CHECK(box_call(host, &d, buf, buf, buf, &fac, nullptr, &box) == -6 && std::strstr(lqrx_last_error(), "rhs"));
        CHECK(box_call(host, &d, buf, buf, buf, &fac, &rhs, nullptr) == -7 && std::strstr(lqrx_last_error(), "box"));
        lqrx_dp_factors fb = fac; fb.K = nullptr;
        CHECK(box_call(host, &d, buf, buf, buf, &fb, &rhs, &box) == -5 && std::strstr(lqrx_last_error(), "fac->K"));
        fb = fac; fb.Einv = nullptr;
        CHECK(box_call(host, &d, buf, buf, buf, &fb, &rhs, &box) == -5 && std::strstr(lqrx_last_error(), "fac->Einv"));
        fb = fac; fb.Pc = nullptr;                       // c without Pc, and Pc without c
        CHECK(box_call(host, &d, buf, buf, buf, &fb, &rhs, &box) == -5 && std::strstr(lqrx_last_error(), "fac->Pc"));
        CHECK(box_call(host, &d, buf, buf, nullptr, &fac, &rhs, &box) == -5 && std::strstr(lqrx_last_error(), "fac->Pc"));
        lqrx_dp_rhs rb = rhs; rb.S = 0;
        CHECK(box_call(host, &d, buf, buf, buf, &fac, &rb, &box) == -6 && std::strstr(lqrx_last_error(), "rhs->S"));
        rb = rhs; rb.d = nullptr;
        CHECK(box_call(host, &d, buf, buf, buf, &fac, &rb, &box) == -6 && std::strstr(lqrx_last_error(), "rhs->d"));
        rb = rhs; rb.p = buf;
        CHECK(box_call(host, &d, buf, buf, buf, &fac, &rb, &box) == -6 && std::strstr(lqrx_last_error(), "rhs->p"));
        const struct { double lqrx_dp_box::*field; double bad; const char *name; } reals[] = {
            {&lqrx_dp_box::rho, 0.0, "box->rho"}, {&lqrx_dp_box::rho, -1.0, "box->rho"}, {&lqrx_dp_box::rho, nan, "box->rho"},
            {&lqrx_dp_box::rho, inf, "box->rho"}, {&lqrx_dp_box::relax, 0.99, "box->relax"}, {&lqrx_dp_box::relax, 2.0, "box->relax"},
            {&lqrx_dp_box::relax, nan, "box->relax"}, {&lqrx_dp_box::eps_prim, -1e-9, "box->eps_prim"},
            {&lqrx_dp_box::eps_prim, nan, "box->eps_prim"}, {&lqrx_dp_box::eps_dual, -1.0, "box->eps_dual"},
            {&lqrx_dp_box::eps_dual, nan, "box->eps_dual"}};
        for (const auto &e : reals) {
            lqrx_dp_box bb = box;
            bb.*(e.field) = e.bad;
            CHECK(box_call(host, &d, buf, buf, buf, &fac, &rhs, &bb) == -7 && std::strstr(lqrx_last_error(), e.name));
        }
        lqrx_dp_box bb = box; bb.max_iter = 0;
        CHECK(box_call(host, &d, buf, buf, buf, &fac, &rhs, &bb) == -7 && std::strstr(lqrx_last_error(), "box->max_iter"));
        bb = box; bb.max_iter = 10001;
        CHECK(box_call(host, &d, buf, buf, buf, &fac, &rhs, &bb) == -7 && std::strstr(lqrx_last_error(), "box->max_iter"));
        bb = box; bb.Z = nullptr;
        CHECK(box_call(host, &d, buf, buf, buf, &fac, &rhs, &bb) == -7 && std::strstr(lqrx_last_error(), "box->Z"));
        bb = box; bb.W = nullptr;
        CHECK(box_call(host, &d, buf, buf, buf, &fac, &rhs, &bb) == -7 && std::strstr(lqrx_last_error(), "box->W"));
        // optional members and the ends of the ranges: the next check answers
        bb = box; bb.u_lo = bb.u_hi = nullptr; bb.iters = nullptr; bb.res = nullptr;
        bb.relax = 1.0; bb.eps_prim = bb.eps_dual = 0.0; bb.max_iter = 10000;
        rb = rhs; rb.q = rb.r = rb.qf = rb.x0 = nullptr; rb.X = rb.U = nullptr;
        CHECK(box_call(host, &d, nullptr, buf, buf, &fac, &rb, &bb) == -2);
        bb = box; bb.max_iter = 1; bb.eps_prim = inf;
        CHECK(box_call(host, &d, nullptr, buf, buf, &fac, &rhs, &bb) == -2);
        lqrx_dp_desc bad = d;
        bad.layout = 1;
        CHECK(box_call(host, &bad, buf, buf, buf, &fac, &rhs, &box) == LQRX_ERR_UNSUPPORTED);
        bad = d; bad.n = 65;
        CHECK(box_call(host, &bad, buf, buf, buf, &fac, &rhs, &box) == LQRX_ERR_UNSUPPORTED);
        bad = d; bad.m = 33;
        CHECK(box_call(host, &bad, buf, buf, buf, &fac, &rhs, &box) == LQRX_ERR_UNSUPPORTED);
        bad = d; bad.n = 0;
        CHECK(box_call(host, &bad, nullptr, buf, buf, &fac, &rhs, &box) == -1);
        bad = d; bad.p_mode = 1;                         // p_mode is not read: the next check answers
        CHECK(box_call(host, &bad, nullptr, buf, buf, &fac, &rhs, &box) == -2);
        bad = d; bad.batch = 0;
        CHECK(box_call(host, &bad, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    }
}

int main()
{
    CHECK(lqrx_abi_version() == LQRX_ABI_VERSION);
    const int have_gpu = lqrx_device_available();
    // dp_kind() on the 16 combinations of lin / aff / cross / value: the five nested ones (bits =
    // 2^k − 1) are the kinds 0 … 4, every other one is −1 (dp_launch then refuses it)
    for (int bits = 0; bits < 16; ++bits) {
        lqrx::DpArgs a{};
        a.lin = bits & 1; a.aff = bits >> 1 & 1; a.cross = bits >> 2 & 1; a.value = bits >> 3 & 1;
        CHECK(lqrx::dp_kind(a) == (bits == 0 ? 0 : bits == 1 ? 1 : bits == 3 ? 2 : bits == 7 ? 3 : bits == 15 ? 4 : -1));
    }

    // ---- DP validation ----
    double dummy[64] = {0};
    int32_t info[4] = {0};
    lqrx_dp_desc d{};
    d.n = 32; d.m = 16; d.N = 256; d.dtype = LQRX_F64; d.batch = 4;
    CHECK(lqrx_dp_solve(nullptr, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, info, nullptr) == -1);
    lqrx_dp_desc b = d; b.n = 0;
    CHECK(lqrx_dp_solve(&b, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, info, nullptr) == -1);
    b = d; b.N = 1;
    CHECK(lqrx_dp_solve_host(&b, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, info) == -1);
    b = d; b.dtype = 7;
    CHECK(lqrx_dp_solve(&b, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, info, nullptr) == -1);
    b = d; b.p_mode = 2;
    CHECK(lqrx_dp_solve(&b, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, info, nullptr) == -1);
    b = d; b.knot_stride_AB = 5;
    CHECK(lqrx_dp_solve(&b, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, info, nullptr) == -1);
    b = d; b.n = 513;                  // past the workgroup kernel's 512
    CHECK(lqrx_dp_solve(&b, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, info, nullptr) == LQRX_ERR_UNSUPPORTED);
    b = d; b.layout = 9;
    CHECK(lqrx_dp_solve(&b, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, info, nullptr) < 0);
    CHECK(lqrx_dp_solve(&d, dummy, nullptr, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, info, nullptr) == -3);
    CHECK(lqrx_dp_solve(&d, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, nullptr, dummy, info, nullptr) == -10);
    // linear cost terms: lin (argument 8) and its pointers validated before any device work
    CHECK(lqrx_dp_solve_linear(&d, dummy, dummy, dummy, dummy, dummy, dummy, nullptr, dummy, dummy, dummy, dummy, info, nullptr) == -8);
    {
        lqrx_dp_linear ln{dummy, dummy, nullptr, dummy, dummy};
        CHECK(lqrx_dp_solve_linear(&d, dummy, dummy, dummy, dummy, dummy, dummy, &ln, dummy, dummy, dummy, dummy, info, nullptr) == -8);
        CHECK(lqrx_dp_solve_linear_host(&d, dummy, dummy, dummy, dummy, dummy, dummy, nullptr, dummy, dummy, dummy, dummy, info) == -8);
        ln.qf = dummy;
        CHECK(lqrx_dp_solve_linear(&d, dummy, dummy, dummy, dummy, dummy, dummy, &ln, dummy, nullptr, dummy, dummy, info, nullptr) == -10);
    }
    dp_null_sweep(dummy, info);
    rollout_sweep(dummy);
    resolve_sweep(dummy, info);
    box_sweep(dummy, info);
    b = d; b.batch = 0;                                          // empty batch: nothing to do
    CHECK(lqrx_dp_solve(&b, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    if (!have_gpu) {                                             // valid call, no device: clean failure
        b = d; b.n = 4; b.m = 1; b.N = 5; b.batch = 1;
        CHECK(lqrx_dp_solve_host(&b, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, info) <= LQRX_ERR_HIP + 0);
    }

    // ---- last-error buffer ----
    b = d; b.m = -3;
    (void)lqrx_dp_solve(&b, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, info, nullptr);
    const int len = lqrx_get_last_error(nullptr, 0);
    CHECK(len > 10);
    char small[6];
    CHECK(lqrx_get_last_error(small, sizeof small) == len && std::strlen(small) == 5);
    char one[1] = {'x'};
    CHECK(lqrx_get_last_error(one, 1) == len && one[0] == '\0');
    std::vector<char> big(len + 1);
    CHECK(lqrx_get_last_error(big.data(), big.size()) == len && std::strcmp(big.data(), lqrx_last_error()) == 0);

    // ---- KKT structure layout ----
    std::vector<int32_t> n1, p, n2, w;
    dubins(101, n1, p, n2, w);
    lqrx_kkt_desc k{};
    k.N = 101; k.dtype = LQRX_F64; k.batch = 16384; k.n1 = n1.data(); k.p = p.data(); k.n2 = n2.data(); k.w = w.data();
    k.h_mode = 2; k.ginv = 1;
    int64_t nY = 0, ny = 0, nH = 0, ng = 0, nl = 0;
    CHECK(lqrx_kkt_sizes(&k, &nY, &ny, &nH, &ng, &nl) == 0);
    CHECK(nY == 6 * 5 + 99 * 30 + 6 * 3 && ny == 6 + 99 * 3 + 3 && nH == 100 * 5 + 3 && ng == nH && nl == ny);
    k.h_mode = 0;
    CHECK(lqrx_kkt_sizes(&k, nullptr, nullptr, &nH, nullptr, nullptr) == 0 && nH == 100 * 25 + 9);
    size_t ws = 0;
    CHECK(lqrx_kkt_workspace_size(&k, &ws) == 0 && ws > 0);
    CHECK(lqrx_kkt_workspace_size(&k, nullptr) == -2);
    lqrx_kkt_desc kb = k; kb.h_mode = 3;
    CHECK(lqrx_kkt_sizes(&kb, &nY, nullptr, nullptr, nullptr, nullptr) == -1);
    kb = k; kb.dtype = LQRX_F32;                               // fp32: the large-block kernels
    CHECK(lqrx_kkt_sizes(&kb, &nY, nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(lqrx_kkt_workspace_size(&kb, &ws) == 0 && ws > 0);
    kb = k; kb.dtype = 7;
    CHECK(lqrx_kkt_sizes(&kb, &nY, nullptr, nullptr, nullptr, nullptr) == -1);
    std::vector<int32_t> bad = n1;
    bad[7] = 2;                                                 // n1[k] != n2[k-1]
    kb = k; kb.n1 = bad.data();
    CHECK(lqrx_kkt_sizes(&kb, &nY, nullptr, nullptr, nullptr, nullptr) == -1);
    std::vector<int32_t> badn2 = n2;
    badn2[100] = 1;                                             // last knot must have n2 == 0
    kb = k; kb.n2 = badn2.data();
    CHECK(lqrx_kkt_sizes(&kb, &nY, nullptr, nullptr, nullptr, nullptr) == -1);
    std::vector<int32_t> bigp = p;
    bigp[50] = 600;                                             // block rows > 512
    kb = k; kb.p = bigp.data();
    CHECK(lqrx_kkt_sizes(&kb, &nY, nullptr, nullptr, nullptr, nullptr) == LQRX_ERR_UNSUPPORTED);
    kb = k; kb.w = nullptr;
    CHECK(lqrx_kkt_sizes(&kb, &nY, nullptr, nullptr, nullptr, nullptr) == -1);
    CHECK(lqrx_kkt_solve(&k, nullptr, dummy, dummy, dummy, dummy, dummy, info, nullptr) == -2);
    CHECK(lqrx_kkt_solve_ws(&k, dummy, dummy, dummy, dummy, dummy, dummy, info, nullptr, 0, nullptr) == -9);

    // ---- generator: a shard equals the matching slice of the whole batch ----
    for (int dt = 0; dt < 2; ++dt) {
        const int n = 5, m = 3, B = 6, s = dt ? 4 : 8;
        std::vector<unsigned char> A(B * n * n * s), Bm(B * n * m * s), Q(B * n * n * s), R(B * m * m * s),
            Qf(B * n * n * s), x0(B * n * s);
        CHECK(lqrx_make_random_dp(n, m, B, 0, 7, dt, A.data(), Bm.data(), Q.data(), R.data(), Qf.data(), x0.data()) == 0);
        std::vector<unsigned char> A2(2 * n * n * s), B2(2 * n * m * s), Q2(2 * n * n * s), R2(2 * m * m * s),
            Qf2(2 * n * n * s), x2(2 * n * s);
        CHECK(lqrx_make_random_dp(n, m, 2, 3, 7, dt, A2.data(), B2.data(), Q2.data(), R2.data(), Qf2.data(), x2.data()) == 0);
        CHECK(std::memcmp(A2.data(), A.data() + 3 * n * n * s, A2.size()) == 0);
        CHECK(std::memcmp(R2.data(), R.data() + 3 * m * m * s, R2.size()) == 0);
        CHECK(std::memcmp(x2.data(), x0.data() + 3 * n * s, x2.size()) == 0);
        if (!dt) {
            const double *q = (const double *)Q.data(), *f = (const double *)Qf.data();
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) CHECK(q[i + j * n] == q[j + i * n] && f[i + j * n] == 10.0 * q[i + j * n]);
        }
    }
    CHECK(lqrx_make_random_dp(0, 1, 1, 0, 1, 0, dummy, dummy, dummy, dummy, dummy, dummy) < 0);

    // ---- LS / SQP validation ----
    CHECK(lqrx_ls_lds_bytes(4, 1, 101) > 0 && lqrx_ls_lds_bytes(4, 1, 101) <= 163840);
    CHECK(lqrx_ls_lds_bytes(6, 3, 101) <= 163840);   // Nm = 300: the global-H path
    lqrx_ls_desc ls{4, 1, 101, 5, 8};
    CHECK(lqrx_ls_solve(&ls, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, info, nullptr, nullptr, nullptr) < 0);
    ls.hu_mode = 0; ls.N = 1026; ls.m = 1;                      // (N-1)m = 1025 > 1024
    CHECK(lqrx_ls_solve_host(&ls, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, info) == LQRX_ERR_UNSUPPORTED);
    lqrx_dubins_sqp_desc q{};
    q.N = 1; q.max_iters = 10; q.batch = 1; q.dt = 0.1;
    CHECK(lqrx_dubins_sqp_solve(&q, dummy, dummy, dummy, dummy, info, info, nullptr) < 0);
    lqrx_sqp_desc g{};
    g.model = LQRX_MODEL_CARTPOLE; g.N = 21; g.max_iters = 10; g.batch = 2; g.dt = 0.25; g.mu = 1.0;
    for (int i = 0; i < 4; ++i) g.Q[i] = 0.01, g.Qf[i] = 100.0;
    g.R[0] = 0.1;
    g.params[0] = 1.0; g.params[1] = 0.2; g.params[2] = 0.5; g.params[3] = 9.81;
    lqrx_sqp_desc gb = g; gb.model = 5;
    CHECK(lqrx_sqp_solve(&gb, dummy, dummy, dummy, dummy, info, info, nullptr) == -1);
    gb = g; gb.params[2] = 0.0;
    CHECK(lqrx_sqp_solve(&gb, dummy, dummy, dummy, dummy, info, info, nullptr) == -1);
    gb = g; gb.R[0] = 0.0;
    CHECK(lqrx_sqp_solve_host(&gb, dummy, dummy, dummy, dummy, info, info) == -1);
    CHECK(lqrx_sqp_solve(&g, nullptr, dummy, dummy, dummy, info, info, nullptr) == -2);
    int32_t nx = 0, nu = 0;
    CHECK(lqrx_sqp_model_dims(LQRX_MODEL_CARTPOLE, &nx, &nu) == 0 && nx == 4 && nu == 1);
    CHECK(lqrx_sqp_model_dims(-1, &nx, &nu) == -1 && lqrx_sqp_model_dims(5, &nx, &nu) == -1);
    CHECK(lqrx_sqp_model_dims(LQRX_MODEL_DOUBLE_INTEGRATOR3, &nx, &nu) == 0 && nx == 6 && nu == 3);
    gb = g; gb.stage_rows = 3;
    CHECK(lqrx_sqp_solve(&gb, dummy, dummy, dummy, dummy, info, info, nullptr) == -1);
    if (!have_gpu) {
        std::vector<double> Zh(2 * (21 * 4 + 20)), x0h(8), lamh(2 * 22 * 4);
        CHECK(lqrx_sqp_solve_host(&g, Zh.data(), x0h.data(), x0h.data(), lamh.data(), info, info) <= LQRX_ERR_HIP + 0);
    }

    std::printf("api sanitizer run: %s (%d failed checks, device %d)\n", fails ? "FAILED" : "ok", fails, have_gpu);
    return fails ? 1 : 0;
}
