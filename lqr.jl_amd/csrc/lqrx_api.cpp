// lqrx_api.cpp — the C ABI (include/lqrx.h): argument validation, stream-ordered scratch,
// host-pointer convenience wrappers, the synthetic-problem generator.
#include "../../include/lqrx.h"
#include "lqrx_internal.h"
#define LQRX_STR2(x) #x
#define LQRX_STR(x) LQRX_STR2(x)
// set by the Makefile: SHA-256 of the library sources (lqrx_build_info; results unaffected)
#ifndef LQRX_SRC_HASH
#define LQRX_SRC_HASH "unknown"
#endif

#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <map>
#include <mutex>
#include <vector>

namespace {

thread_local std::string g_err;

int set_err(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int set_err(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int hip_err(hipError_t e, const char *what)
{
    return set_err(LQRX_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

size_t dsize(int dtype) { return dtype == LQRX_F32 ? 4 : 8; }

// ---- stream-ordered device buffers (for the *_host wrappers) ----
struct DevBuf {
    void *p = nullptr;
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
};

int dev_alloc(DevBuf &b, size_t bytes, const char *name)
{
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) return hip_err(e, name);
    return 0;
}

int validate_dp(const lqrx_dp_desc *d)
{
    if (!d) return set_err(-1, "desc is NULL");
    if (d->n < 1) return set_err(-1, "desc.n must be >= 1 (got %d)", d->n);
    if (d->m < 1) return set_err(-1, "desc.m must be >= 1 (got %d)", d->m);
    if (d->N < 2) return set_err(-1, "desc.N must be >= 2 (got %d)", d->N);
    if (d->dtype != LQRX_F64 && d->dtype != LQRX_F32)
        return set_err(-1, "desc.dtype must be LQRX_F64 or LQRX_F32 (got %d)", d->dtype);
    if (d->batch < 0) return set_err(-1, "desc.batch must be >= 0");
    if (d->layout != 0 && d->layout != 1)
        return set_err(-1, "desc.layout must be 0 (batch slowest) or 1 (batch fastest, SoA) (got %d)", d->layout);
    if (d->p_mode != 0 && d->p_mode != 1) return set_err(-1, "desc.p_mode must be 0 or 1");
    if (d->knot_stride_AB != 0 && d->knot_stride_AB != 1)
        return set_err(-1, "desc.knot_stride_AB must be 0 (time-invariant) or 1 (per knot)");
    if (d->knot_stride_QR != 0 && d->knot_stride_QR != 1)
        return set_err(-1, "desc.knot_stride_QR must be 0 (time-invariant) or 1 (per knot)");
    const bool tv = d->knot_stride_AB != 0 || d->knot_stride_QR != 0;
    if (!lqrx::dp_supported(d->dtype, d->n, d->m, tv))
        return set_err(LQRX_ERR_UNSUPPORTED, "no kernel instantiated for n=%d m=%d%s", d->n, d->m,
                       tv ? " (time-varying)" : "");
    return 0;
}

} // namespace

namespace lqrx {
// The device a stream belongs to (the null stream: the calling thread's current device).
// Library state below is keyed on it, not on hipGetDevice(), so a call on a stream of
// device d works whatever device the calling thread has current.
hipError_t stream_device(hipStream_t s, int *dev)
{
    if (!s) return hipGetDevice(dev);
    hipDevice_t d = 0;
    hipError_t e = hipStreamGetDevice(s, &d);
    if (e == hipSuccess) *dev = (int)d;
    return e;
}

// Process-wide state (mutex-guarded, created on first use): one memory pool per device for
// stream-ordered scratch; freed blocks stay mapped (release threshold ∞), so steady-state
// calls allocate nothing from the driver.
static std::mutex pool_mu;
static std::map<int, hipMemPool_t> pools;
hipError_t scratch_alloc(void **p, size_t bytes, hipStream_t s)
{
    auto &mu = pool_mu;
    int dev = 0;
    hipError_t e = stream_device(s, &dev);
    if (e != hipSuccess) return e;
    hipMemPool_t pool = nullptr;
    {
        std::lock_guard<std::mutex> lock(mu);
        auto it = pools.find(dev);
        if (it == pools.end()) {
            hipMemPoolProps props{};
            props.allocType = hipMemAllocationTypePinned;
            props.location.type = hipMemLocationTypeDevice;
            props.location.id = dev;
            if ((e = hipMemPoolCreate(&pool, &props)) != hipSuccess) return e;
            uint64_t keep = UINT64_MAX;                     // never trim freed blocks
            if ((e = hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep)) != hipSuccess) return e;
            pools.emplace(dev, pool);
        } else {
            pool = it->second;
        }
    }
    return hipMallocFromPoolAsync(p, bytes, pool, s);
}
hipError_t scratch_free(void *p, hipStream_t s) { return hipFreeAsync(p, s); }
hipError_t scratch_trim(int device, size_t keep)
{
    std::lock_guard<std::mutex> lock(pool_mu);
    for (auto &kv : pools)
        if (device < 0 || kv.first == device) {
            hipError_t e = hipMemPoolTrimTo(kv.second, keep);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}
} // namespace lqrx

namespace {
// ---- the DP solve entries: one table of a call's buffers ----
// The entry kinds (enum DpKind, lqrx_internal.h) nest: each adds arguments to the one before it.
using lqrx::DpKind, lqrx::DP_PLAIN, lqrx::DP_LINEAR, lqrx::DP_AFFINE, lqrx::DP_CROSS, lqrx::DP_VALUE;

// the caller's pointers, whatever the entry's argument order
struct DpPtrs {
    const void *A, *B, *c, *Q, *R, *M, *Qf, *x0;
    const lqrx_dp_linear *lin;
    const lqrx_dp_value *val;
    void *K, *P, *X, *U;
    int32_t *info;
};

struct DpRow {
    const char *name;
    void *ptr;       // the caller's buffer, or its device / layout-0 twin in a staged copy of the table
    size_t field;    // offset of the DpArgs pointer it feeds (kNoField: val->J, or a NULL lin / val)
    int64_t elems;   // elements per trajectory
    int arg;         // argument number in the entry that was called (a member of lin, val: the struct's)
    bool out, optional;
};
constexpr size_t kNoField = ~(size_t)0;
#define DPF(f) offsetof(lqrx::DpArgs, f)

// The rows stand in the called entry's argument order, so a row's argument number is its position
// (desc is 1; lin and val take one number each, which their members share).  info, optional and
// int32, is not a row.
struct DpTable {
    enum { kIn = 0, kOut = 1, kOptional = 2, kMember = 4, kMaxRows = 20 };
    DpKind kind;
    DpRow row[kMaxRows];
    int nrows = 0, narg = 1, iJ = -1;

    void add(const char *name, const void *ptr, size_t field, int64_t elems, int flags = kIn)
    {
        if (!(flags & kMember)) ++narg;
        row[nrows++] = DpRow{name, const_cast<void *>(ptr), field, elems, narg, (flags & kOut) != 0,
                             (flags & kOptional) != 0};
    }
    // a struct argument: its members follow when it is there, else one NULL row reports it
    bool open(const char *name, const void *st)
    {
        ++narg;
        if (!st) add(name, nullptr, kNoField, 0, kMember);
        return st != nullptr;
    }

    DpTable(const lqrx_dp_desc *d, DpKind k, const DpPtrs &p) : kind(k)
    {
        const int64_t n = d->n, m = d->m, N = d->N;
        const int64_t kAB = d->knot_stride_AB ? N - 1 : 1, kQR = d->knot_stride_QR ? N - 1 : 1;
        const int64_t kP = d->p_mode ? N : 1;
        add("A", p.A, DPF(A), n * n * kAB);
        add("B", p.B, DPF(B), n * m * kAB);
        if (k >= DP_AFFINE) add("c", p.c, DPF(c), n * kAB);
        add("Q", p.Q, DPF(Q), n * n * kQR);
        add("R", p.R, DPF(R), m * m * kQR);
        if (k >= DP_CROSS) add("M", p.M, DPF(M), m * n * kQR);
        add("Qf", p.Qf, DPF(Qf), n * n);
        add("x0", p.x0, DPF(x0), n);
        if (k >= DP_LINEAR && open("lin", p.lin)) {
            add("lin->q", p.lin->q, DPF(q), n * kQR, kMember);
            add("lin->r", p.lin->r, DPF(r), m * kQR, kMember);
            add("lin->qf", p.lin->qf, DPF(qf), n, kMember);
            add("lin->d", p.lin->d, DPF(d), m * (N - 1), kMember | kOut);
            add("lin->p", p.lin->p, DPF(p), n * kP, kMember | kOut);
        }
        if (k >= DP_VALUE && open("val", p.val)) {
            add("val->s", p.val->s, DPF(vs), kP, kMember | kOut);
            add("val->dV", p.val->dV, DPF(vdV), 1, kMember | kOut | kOptional);
            iJ = nrows;
            add("val->J", p.val->J, kNoField, 1, kMember | kOut | kOptional);
        }
        add("K", p.K, DPF(K), m * n * (N - 1), kOut);
        add("P", p.P, DPF(P), n * n * kP, kOut);
        add("X", p.X, DPF(X), n * N, kOut);
        add("U", p.U, DPF(U), m * (N - 1), kOut);
    }

    // every required pointer, in argument order — before anything touches the device
    int check() const
    {
        for (int i = 0; i < nrows; ++i)
            if (!row[i].ptr && !row[i].optional)
                return set_err(-row[i].arg, "pointer %d (%s) is NULL", row[i].arg, row[i].name);
        return 0;
    }
    void *J() const { return iJ >= 0 ? row[iJ].ptr : nullptr; }
};
#undef DPF

// the kernels' arguments of a checked table; lin, aff, cross and value follow from the kind
lqrx::DpArgs dp_args(const lqrx_dp_desc *d, const DpTable &t, int32_t *info)
{
    lqrx::DpArgs a{};
    for (int i = 0; i < t.nrows; ++i)
        if (t.row[i].field != kNoField)
            *reinterpret_cast<void **>(reinterpret_cast<char *>(&a) + t.row[i].field) = t.row[i].ptr;
    a.lin = t.kind >= DP_LINEAR; a.aff = t.kind >= DP_AFFINE; a.cross = t.kind >= DP_CROSS;
    a.value = t.kind >= DP_VALUE;
    a.info = info;
    a.n = d->n; a.m = d->m; a.N = d->N; a.dtype = d->dtype; a.p_all = d->p_mode;
    a.batch = d->batch;
    a.tv_AB = (int)d->knot_stride_AB; a.tv_QR = (int)d->knot_stride_QR;
    a.layout = d->layout;
    return a;
}

// Layout 1 on the MFMA kernel (one trajectory per wave, contiguous blocks wanted): the SoA
// buffers are transposed to layout 0 in one stream-ordered scratch block, solved, and the
// outputs transposed back into the caller's SoA buffers.  Extra HBM traffic: one read + one
// write of every input and output (2× the algorithmic bytes); the n ≤ 4 kernels read SoA
// natively instead.
// A buffer of one element per trajectory (s_1, dV and J of a value solve) is the same in both
// layouts and is used in place; s is staged like p when it holds every s_k.  J is formed on the
// layout-0 scratch, before the transposition back.
hipError_t dp_launch_soa_staged(const lqrx_dp_desc *d, const DpTable &t, int32_t *info, hipStream_t s)
{
    const int64_t B = d->batch;
    const int es = (int)dsize(d->dtype);
    size_t off[DpTable::kMaxRows], total = 0;
    for (int i = 0; i < t.nrows; ++i) {
        off[i] = total;
        if (t.row[i].elems > 1) total += ((size_t)t.row[i].elems * B * es + 255) & ~(size_t)255;
    }
    void *blk = nullptr;
    hipError_t e = lqrx::scratch_alloc(&blk, total, s);
    if (e != hipSuccess) return e;
    DpTable t0 = t;
    for (int i = 0; i < t.nrows; ++i) {
        const DpRow &r = t.row[i];
        if (r.elems <= 1) continue;
        t0.row[i].ptr = (char *)blk + off[i];
        if (!r.out && e == hipSuccess)                            // [S][B] → [B][S]
            e = lqrx::batch_transpose(r.ptr, t0.row[i].ptr, r.elems, B, es, s);
    }
    lqrx_dp_desc d0 = *d;
    d0.layout = 0;
    const lqrx::DpArgs a0 = dp_args(&d0, t0, info);
    if (e == hipSuccess) e = lqrx::dp_launch(a0, s);
    if (e == hipSuccess && t.J()) e = lqrx::dp_value_cost_launch(a0, t.J(), s);
    for (int i = 0; i < t.nrows && e == hipSuccess; ++i)          // [B][S] → [S][B]
        if (t.row[i].out && t.row[i].elems > 1)
            e = lqrx::batch_transpose(t0.row[i].ptr, t.row[i].ptr, B, t.row[i].elems, es, s);
    hipError_t ef = lqrx::scratch_free(blk, s);
    return e != hipSuccess ? e : ef;
}

// ---- host staging: the device twins of a call's host buffers (the *_host entries) ----
// copied in; copied back; copied in and back; device only (an info nobody reads)
enum HostDir { H_IN, H_OUT, H_INOUT, H_SCRATCH };
struct HostBuf {
    void *host;      // NULL (an optional buffer the caller left out): no twin, unless H_SCRATCH
    size_t bytes;
    HostDir dir;
};
HostBuf host_in(const void *p, size_t bytes) { return HostBuf{const_cast<void *>(p), bytes, H_IN}; }
HostBuf host_info(int32_t *info, size_t batch) { return HostBuf{info, 4 * batch, info ? H_OUT : H_SCRATCH}; }

struct HostStage {
    DevBuf dev[DpTable::kMaxRows + 1];
    void *operator[](int i) const { return dev[i].p; }
    int upload(const HostBuf *l, int n)
    {
        for (int i = 0; i < n; ++i) {
            if (!l[i].host && l[i].dir != H_SCRATCH) continue;
            if (int st = dev_alloc(dev[i], l[i].bytes, "hipMalloc (host staging)")) return st;
            if (l[i].dir != H_IN && l[i].dir != H_INOUT) continue;
            const hipError_t e = hipMemcpy(dev[i].p, l[i].host, l[i].bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) return hip_err(e, "H2D");
        }
        return 0;
    }
    int download(const HostBuf *l, int n) const
    {
        for (int i = 0; i < n; ++i) {
            if ((l[i].dir != H_OUT && l[i].dir != H_INOUT) || !dev[i].p) continue;
            const hipError_t e = hipMemcpy(l[i].host, dev[i].p, l[i].bytes, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return hip_err(e, "D2H");
        }
        return 0;
    }
};
} // namespace

extern "C" {

int lqrx_abi_version(void) { return LQRX_ABI_VERSION; }
const char *lqrx_build_info(void)
{
    return "src_sha256=" LQRX_SRC_HASH " abi=" LQRX_STR(LQRX_ABI_VERSION) " arch=gfx950 built=" __DATE__ " " __TIME__;
}
int lqrx_scratch_trim(int32_t device, size_t keep_bytes)
{
    const hipError_t e = lqrx::scratch_trim(device, keep_bytes);
    return e == hipSuccess ? 0 : hip_err(e, "hipMemPoolTrimTo");
}

const char *lqrx_last_error(void) { return g_err.c_str(); }

int lqrx_get_last_error(char *buf, size_t len)
{
    if (buf && len > 0) {
        const size_t k = std::min(len - 1, g_err.size());
        std::memcpy(buf, g_err.data(), k);
        buf[k] = '\0';
    }
    return (int)g_err.size();
}

int lqrx_device_available(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return 0;
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    return std::strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

}   // extern "C"

namespace {
// launch of a checked table on device pointers; 1 where a trajectory's info is non-zero (null
// stream only: the call is then synchronous)
int dp_run(const lqrx_dp_desc *d, const DpTable &t, int32_t *info, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if (d->layout == 1 && !lqrx::dp_lane_supported(d->n, d->m)) {
        e = dp_launch_soa_staged(d, t, info, s);  // MFMA kernel: convert, solve, convert back
    } else {
        const lqrx::DpArgs a = dp_args(d, t, info);
        e = lqrx::dp_launch(a, s);
        if (e == hipSuccess && t.J()) e = lqrx::dp_value_cost_launch(a, t.J(), s);   // V_1(x0): one small kernel behind the solve
    }
    if (e == hipErrorNotSupported)
        return set_err(LQRX_ERR_UNSUPPORTED, "no kernel for n=%d m=%d", d->n, d->m);
    if (e != hipSuccess) return hip_err(e, "dp kernel launch");
    if (stream == nullptr) {
        e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) return hip_err(e, "dp kernel");
        if (info) {
            std::vector<int32_t> h((size_t)d->batch);
            e = hipMemcpy(h.data(), info, h.size() * 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return hip_err(e, "info D2H");
            for (int32_t v : h)
                if (v) return 1;
        }
    }
    return 0;
}

// Every DP solve entry on device pointers.  Order of the checks: descriptor, batch == 0 (a no-op),
// pointers in the argument order of the entry that was called.
int dp_solve_impl(const lqrx_dp_desc *d, DpKind kind, const DpPtrs &p, void *stream)
{
    int st = validate_dp(d);
    if (st) return st;
    if (d->batch == 0) return 0;
    const DpTable t(d, kind, p);
    if ((st = t.check())) return st;
    return dp_run(d, t, p.info, stream);
}

// Every DP solve entry on host pointers: the same checks, before any device call; then one device
// twin per buffer of the table, the solve on the null stream, and the outputs copied back.
int dp_solve_host_impl(const lqrx_dp_desc *d, DpKind kind, const DpPtrs &p)
{
    int st = validate_dp(d);
    if (st) return st;
    if (d->batch == 0) return 0;
    const DpTable t(d, kind, p);
    if ((st = t.check())) return st;
    const size_t bt = (size_t)d->batch, es = dsize(d->dtype);
    HostBuf hb[DpTable::kMaxRows + 1];
    for (int i = 0; i < t.nrows; ++i)
        hb[i] = HostBuf{t.row[i].ptr, (size_t)t.row[i].elems * es * bt, t.row[i].out ? H_OUT : H_IN};
    hb[t.nrows] = host_info(p.info, bt);
    HostStage dev;
    if ((st = dev.upload(hb, t.nrows + 1))) return st;
    DpTable td = t;
    for (int i = 0; i < t.nrows; ++i) td.row[i].ptr = dev[i];
    st = dp_run(d, td, (int32_t *)dev[t.nrows], nullptr);
    if (st < 0) return st;
    const int e = dev.download(hb, t.nrows + 1);
    return e ? e : st;
}
} // namespace

extern "C" {

int lqrx_dp_solve(const lqrx_dp_desc *d, const void *A, const void *B, const void *Q,
                  const void *R, const void *Qf, const void *x0, void *K, void *P, void *X,
                  void *U, int32_t *info, void *stream)
{
    return dp_solve_impl(d, DP_PLAIN, DpPtrs{A, B, nullptr, Q, R, nullptr, Qf, x0, nullptr, nullptr, K, P, X, U, info}, stream);
}

int lqrx_dp_solve_host(const lqrx_dp_desc *d, const void *A, const void *B, const void *Q,
                       const void *R, const void *Qf, const void *x0, void *K, void *P,
                       void *X, void *U, int32_t *info)
{
    return dp_solve_host_impl(d, DP_PLAIN, DpPtrs{A, B, nullptr, Q, R, nullptr, Qf, x0, nullptr, nullptr, K, P, X, U, info});
}

// compute_ctg!(K, solver, prob) / compute_gain!(K, solver, prob) for a batch
// (dynamic_programming.jl:34-52): one backward knot from P = solver.P.  It is exactly the
// first backward step of a 2-knot solve with Qf = P, so it runs the same kernel family on a
// 2-knot descriptor; the rollout's X, U and a zero x0 live in stream-ordered scratch.
int lqrx_dp_compute_ctg(const lqrx_dp_desc *d, const void *A, const void *B, const void *Q,
                        const void *R, const void *P, void *K, void *P_, int32_t *info, void *stream)
{
    if (!d) return set_err(-1, "desc is NULL");
    lqrx_dp_desc d2 = *d;
    d2.N = 2;
    d2.p_mode = 0;
    d2.knot_stride_AB = d2.knot_stride_QR = 0;
    int st = validate_dp(&d2);
    if (st) return st;
    if (d2.batch == 0) return 0;
    const void *in[5] = {A, B, Q, R, P};
    for (int i = 0; i < 5; ++i)
        if (!in[i]) return set_err(-(i + 2), "input pointer %d is NULL", i + 2);
    if (!K) return set_err(-7, "K is NULL");
    const size_t es = dsize(d2.dtype), bt = (size_t)d2.batch, n = d2.n, m = d2.m;
    // scratch: x0 (zeros) | X (2n) | U (m) | P_ when the caller passed none (compute_gain!)
    const size_t ox = 0, oX = ox + ((n * bt * es + 255) & ~(size_t)255);
    const size_t oU = oX + ((2 * n * bt * es + 255) & ~(size_t)255);
    const size_t oP = oU + ((m * bt * es + 255) & ~(size_t)255);
    const size_t tot = oP + (P_ ? 0 : n * n * bt * es);
    hipStream_t s = (hipStream_t)stream;
    void *blk = nullptr;
    hipError_t e = lqrx::scratch_alloc(&blk, tot, s);
    if (e != hipSuccess) return hip_err(e, "compute_ctg scratch");
    char *b = (char *)blk;
    e = hipMemsetAsync(b + ox, 0, n * bt * es, s);
    if (e != hipSuccess) {
        (void)lqrx::scratch_free(blk, s);
        return hip_err(e, "compute_ctg x0");
    }
    st = dp_solve_impl(&d2, DP_PLAIN, DpPtrs{A, B, nullptr, Q, R, nullptr, P, b + ox, nullptr, nullptr, K,
                                             P_ ? P_ : (void *)(b + oP), b + oX, b + oU, info}, stream);
    e = lqrx::scratch_free(blk, s);
    if (st) return st;
    return e == hipSuccess ? 0 : hip_err(e, "compute_ctg scratch free");
}

int lqrx_dp_compute_ctg_host(const lqrx_dp_desc *d, const void *A, const void *B, const void *Q,
                             const void *R, const void *P, void *K, void *P_, int32_t *info)
{
    if (!d) return set_err(-1, "desc is NULL");
    lqrx_dp_desc d2 = *d;
    d2.N = 2;
    d2.p_mode = 0;
    d2.knot_stride_AB = d2.knot_stride_QR = 0;
    int st = validate_dp(&d2);
    if (st) return st;
    if (d2.batch == 0) return 0;
    const void *hin[5] = {A, B, Q, R, P};
    for (int i = 0; i < 5; ++i)
        if (!hin[i]) return set_err(-(i + 2), "input pointer %d is NULL", i + 2);
    if (!K) return set_err(-7, "K is NULL");
    const size_t bt = (size_t)d2.batch, n = d2.n, m = d2.m, eb = dsize(d2.dtype) * bt;   // bytes per element row
    const size_t nn = n * n * eb, nm = n * m * eb, mm = m * m * eb;
    const HostBuf hb[8] = {host_in(A, nn), host_in(B, nm), host_in(Q, nn), host_in(R, mm), host_in(P, nn),
                           HostBuf{K, nm, H_OUT}, HostBuf{P_, nn, H_OUT}, host_info(info, bt)};
    HostStage dev;
    if ((st = dev.upload(hb, 8))) return st;
    st = lqrx_dp_compute_ctg(&d2, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], (int32_t *)dev[7], nullptr);
    if (st < 0) return st;
    const int e = dev.download(hb, 8);
    return e ? e : st;
}

int lqrx_dp_solve_linear(const lqrx_dp_desc *d, const void *A, const void *B, const void *Q,
                         const void *R, const void *Qf, const void *x0,
                         const lqrx_dp_linear *lin, void *K, void *P, void *X, void *U,
                         int32_t *info, void *stream)
{
    return dp_solve_impl(d, DP_LINEAR, DpPtrs{A, B, nullptr, Q, R, nullptr, Qf, x0, lin, nullptr, K, P, X, U, info}, stream);
}

int lqrx_dp_solve_linear_host(const lqrx_dp_desc *d, const void *A, const void *B,
                              const void *Q, const void *R, const void *Qf, const void *x0,
                              const lqrx_dp_linear *lin, void *K, void *P, void *X, void *U,
                              int32_t *info)
{
    return dp_solve_host_impl(d, DP_LINEAR, DpPtrs{A, B, nullptr, Q, R, nullptr, Qf, x0, lin, nullptr, K, P, X, U, info});
}

// affine dynamics x⁺ = A x + B u + c: the linear-terms solve with p̃ = p + P c_k (see lqrx.h)
int lqrx_dp_solve_affine(const lqrx_dp_desc *d, const void *A, const void *B, const void *c,
                         const void *Q, const void *R, const void *Qf, const void *x0,
                         const lqrx_dp_linear *lin, void *K, void *P, void *X, void *U,
                         int32_t *info, void *stream)
{
    return dp_solve_impl(d, DP_AFFINE, DpPtrs{A, B, c, Q, R, nullptr, Qf, x0, lin, nullptr, K, P, X, U, info}, stream);
}

int lqrx_dp_solve_affine_host(const lqrx_dp_desc *d, const void *A, const void *B, const void *c,
                              const void *Q, const void *R, const void *Qf, const void *x0,
                              const lqrx_dp_linear *lin, void *K, void *P, void *X, void *U,
                              int32_t *info)
{
    return dp_solve_host_impl(d, DP_AFFINE, DpPtrs{A, B, c, Q, R, nullptr, Qf, x0, lin, nullptr, K, P, X, U, info});
}

// cost cross term uᵀMx on top of the affine solve: G = BᵀPA + M_k (see lqrx.h)
int lqrx_dp_solve_cross(const lqrx_dp_desc *d, const void *A, const void *B, const void *c,
                        const void *Q, const void *R, const void *M, const void *Qf, const void *x0,
                        const lqrx_dp_linear *lin, void *K, void *P, void *X, void *U,
                        int32_t *info, void *stream)
{
    return dp_solve_impl(d, DP_CROSS, DpPtrs{A, B, c, Q, R, M, Qf, x0, lin, nullptr, K, P, X, U, info}, stream);
}

int lqrx_dp_solve_cross_host(const lqrx_dp_desc *d, const void *A, const void *B, const void *c,
                             const void *Q, const void *R, const void *M, const void *Qf,
                             const void *x0, const lqrx_dp_linear *lin, void *K, void *P, void *X,
                             void *U, int32_t *info)
{
    return dp_solve_host_impl(d, DP_CROSS, DpPtrs{A, B, c, Q, R, M, Qf, x0, lin, nullptr, K, P, X, U, info});
}

// the value function's constant on top of the cross solve: s, dV = Σ hᵀd, J = V_1(x0) (see lqrx.h)
int lqrx_dp_solve_value(const lqrx_dp_desc *d, const void *A, const void *B, const void *c,
                        const void *Q, const void *R, const void *M, const void *Qf, const void *x0,
                        const lqrx_dp_linear *lin, const lqrx_dp_value *val, void *K, void *P,
                        void *X, void *U, int32_t *info, void *stream)
{
    return dp_solve_impl(d, DP_VALUE, DpPtrs{A, B, c, Q, R, M, Qf, x0, lin, val, K, P, X, U, info}, stream);
}

int lqrx_dp_solve_value_host(const lqrx_dp_desc *d, const void *A, const void *B, const void *c,
                             const void *Q, const void *R, const void *M, const void *Qf,
                             const void *x0, const lqrx_dp_linear *lin, const lqrx_dp_value *val,
                             void *K, void *P, void *X, void *U, int32_t *info)
{
    return dp_solve_host_impl(d, DP_VALUE, DpPtrs{A, B, c, Q, R, M, Qf, x0, lin, val, K, P, X, U, info});
}

} // extern "C"

namespace {
// Descriptor checks shared by lqrx_dp_costates[_host] and lqrx_dp_solve_adjoint: p_mode is
// ignored, layout 1 is a stated follow-up
int validate_dp_adjoint(const lqrx_dp_desc *d, const char *entry)
{
    if (!d) return set_err(-1, "desc is NULL");
    lqrx_dp_desc d0 = *d;
    d0.p_mode = 0;
    int st = validate_dp(&d0);
    if (st) return st;
    if (d->layout != 0)
        return set_err(LQRX_ERR_UNSUPPORTED, "%s: desc.layout = 1 is not supported (layout 0 only)", entry);
    return 0;
}

// The arguments of lqrx_dp_costates[_host] behind desc, in order: A 2, B 3, Q 4, R 5, M 6, Qf 7,
// q 8, r 9, qf 10, K 11, X 12, U 13, lam 14; M, q, r, qf may be NULL (zero)
struct CostatePtrs {
    const void *A, *B, *Q, *R, *M, *Qf, *q, *r, *qf, *K, *X, *U;
    void *lam;
};

int check_costate_ptrs(const CostatePtrs &c)
{
    const void *p[13] = {c.A, c.B, c.Q, c.R, c.M, c.Qf, c.q, c.r, c.qf, c.K, c.X, c.U, c.lam};
    static const char *nm[13] = {"A", "B", "Q", "R", "M", "Qf", "q", "r", "qf", "K", "X", "U", "lam"};
    static const bool optional[13] = {false, false, false, false, true, false, true, true, true, false, false, false, false};
    for (int i = 0; i < 13; ++i)
        if (!p[i] && !optional[i]) return set_err(-(i + 2), "pointer %d (%s) is NULL", i + 2, nm[i]);
    return 0;
}

lqrx::DpCostateArgs costate_args(const lqrx_dp_desc *d, const CostatePtrs &c)
{
    lqrx::DpCostateArgs a{};
    a.A = c.A; a.B = c.B; a.Q = c.Q; a.R = c.R; a.M = c.M; a.Qf = c.Qf; a.q = c.q; a.r = c.r; a.qf = c.qf;
    a.K = c.K; a.X = c.X; a.U = c.U; a.lam = c.lam;
    a.n = d->n; a.m = d->m; a.N = d->N; a.dtype = d->dtype;
    a.tv_AB = (int)d->knot_stride_AB; a.tv_QR = (int)d->knot_stride_QR;
    a.batch = d->batch;
    return a;
}
} // namespace

extern "C" {

// costates λ_k = P_k x_k + p_k of a solve, by the closed-loop backward sweep on its K, X, U (see lqrx.h)
int lqrx_dp_costates(const lqrx_dp_desc *d, const void *A, const void *B, const void *Q, const void *R,
                     const void *M, const void *Qf, const void *q, const void *r, const void *qf, const void *K,
                     const void *X, const void *U, void *lam, void *stream)
{
    int st = validate_dp_adjoint(d, "lqrx_dp_costates");
    if (st) return st;
    if (d->batch == 0) return 0;
    const CostatePtrs c{A, B, Q, R, M, Qf, q, r, qf, K, X, U, lam};
    if ((st = check_costate_ptrs(c))) return st;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = lqrx::dp_costate_launch(costate_args(d, c), s);
    if (e == hipErrorNotSupported) return set_err(LQRX_ERR_UNSUPPORTED, "no costate kernel for n=%d m=%d", d->n, d->m);
    if (e != hipSuccess) return hip_err(e, "costate kernel launch");
    if (stream == nullptr && (e = hipStreamSynchronize(nullptr)) != hipSuccess) return hip_err(e, "costate kernel");
    return 0;
}

int lqrx_dp_costates_host(const lqrx_dp_desc *d, const void *A, const void *B, const void *Q, const void *R,
                          const void *M, const void *Qf, const void *q, const void *r, const void *qf,
                          const void *K, const void *X, const void *U, void *lam)
{
    int st = validate_dp_adjoint(d, "lqrx_dp_costates_host");
    if (st) return st;
    if (d->batch == 0) return 0;
    if ((st = check_costate_ptrs(CostatePtrs{A, B, Q, R, M, Qf, q, r, qf, K, X, U, lam}))) return st;
    const size_t es = dsize(d->dtype), bt = (size_t)d->batch, n = d->n, m = d->m, N = d->N;
    const size_t kAB = d->knot_stride_AB ? N - 1 : 1, kQR = d->knot_stride_QR ? N - 1 : 1;
    const void *hin[12] = {A, B, Q, R, M, Qf, q, r, qf, K, X, U};
    const size_t szin[12] = {n * n * kAB, n * m * kAB, n * n * kQR, m * m * kQR, m * n * kQR, n * n,
                             n * kQR, m * kQR, n, m * n * (N - 1), n * N, m * (N - 1)};
    HostBuf hb[13];
    for (int i = 0; i < 12; ++i) hb[i] = host_in(hin[i], szin[i] * es * bt);   // M, q, r, qf: NULL means zero
    hb[12] = HostBuf{lam, n * N * es * bt, H_OUT};
    HostStage dev;
    if ((st = dev.upload(hb, 13))) return st;
    st = lqrx_dp_costates(d, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], dev[7], dev[8], dev[9], dev[10],
                          dev[11], dev[12], nullptr);
    if (st < 0) return st;
    const int e = dev.download(hb, 13);
    return e ? e : st;
}

} // extern "C"

namespace {
// The checks of lqrx_dp_rollout[_host] behind desc, in argument order (A 2, B 3, K 5, cost 7, sc 8;
// c 4 and d 6 may be NULL).  sc comes before cost only as far as cost needs it: whether J is asked for.
int check_rollout_args(const void *A, const void *B, const void *K, const lqrx_dp_cost *cost,
                       const lqrx_dp_scenarios *sc)
{
    if (!A) return set_err(-2, "pointer 2 (A) is NULL");
    if (!B) return set_err(-3, "pointer 3 (B) is NULL");
    if (!K) return set_err(-5, "pointer 5 (K) is NULL");
    if (!sc) return set_err(-8, "pointer 8 (sc) is NULL");
    if (sc->J) {
        if (!cost) return set_err(-7, "pointer 7 (cost) is NULL and sc->J is asked for");
        if (!cost->Q) return set_err(-7, "cost->Q is NULL and sc->J is asked for");
        if (!cost->R) return set_err(-7, "cost->R is NULL and sc->J is asked for");
        if (!cost->Qf) return set_err(-7, "cost->Qf is NULL and sc->J is asked for");
    }
    if (sc->S < 1) return set_err(-8, "sc->S must be >= 1 (got %lld)", (long long)sc->S);
    if (!sc->x0) return set_err(-8, "sc->x0 is NULL");
    if (!sc->X && !sc->U && !sc->J) return set_err(-8, "sc->X, sc->U and sc->J are all NULL: nothing to compute");
    return 0;
}

lqrx::DpScenArgs scen_args(const lqrx_dp_desc *d, const void *A, const void *B, const void *c, const void *K,
                           const void *dd, const lqrx_dp_cost *cost, const lqrx_dp_scenarios *sc)
{
    lqrx::DpScenArgs a{};
    a.A = A; a.B = B; a.c = c; a.K = K; a.d = dd;
    if (sc->J) {   // the cost is read only for J
        a.Q = cost->Q; a.R = cost->R; a.Qf = cost->Qf; a.M = cost->M; a.q = cost->q; a.r = cost->r; a.qf = cost->qf;
    }
    a.x0 = sc->x0; a.alpha = sc->alpha; a.w = sc->w; a.u_lo = sc->u_lo; a.u_hi = sc->u_hi;
    a.X = sc->X; a.U = sc->U; a.J = sc->J;
    a.n = d->n; a.m = d->m; a.N = d->N; a.dtype = d->dtype;
    a.tv_AB = (int)d->knot_stride_AB; a.tv_QR = (int)d->knot_stride_QR;
    a.batch = d->batch; a.S = sc->S;
    return a;
}
} // namespace

extern "C" {

// closed-loop rollout of the policy (K, d) over sc->S scenarios per problem (see lqrx.h): one kernel, no scratch
int lqrx_dp_rollout(const lqrx_dp_desc *d, const void *A, const void *B, const void *c, const void *K,
                    const void *dd, const lqrx_dp_cost *cost, const lqrx_dp_scenarios *sc, void *stream)
{
    int st = validate_dp_adjoint(d, "lqrx_dp_rollout");
    if (st) return st;
    if (d->batch == 0) return 0;
    if ((st = check_rollout_args(A, B, K, cost, sc))) return st;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = lqrx::dp_scen_launch(scen_args(d, A, B, c, K, dd, cost, sc), s);
    if (e == hipErrorNotSupported) return set_err(LQRX_ERR_UNSUPPORTED, "no rollout kernel for n=%d m=%d", d->n, d->m);
    if (e != hipSuccess) return hip_err(e, "rollout kernel launch");
    if (stream == nullptr && (e = hipStreamSynchronize(nullptr)) != hipSuccess) return hip_err(e, "rollout kernel");
    return 0;
}

int lqrx_dp_rollout_host(const lqrx_dp_desc *d, const void *A, const void *B, const void *c, const void *K,
                         const void *dd, const lqrx_dp_cost *cost, const lqrx_dp_scenarios *sc)
{
    int st = validate_dp_adjoint(d, "lqrx_dp_rollout_host");
    if (st) return st;
    if (d->batch == 0) return 0;
    if ((st = check_rollout_args(A, B, K, cost, sc))) return st;
    const size_t es = dsize(d->dtype), bt = (size_t)d->batch, n = d->n, m = d->m, N = d->N, S = (size_t)sc->S;
    const size_t kAB = d->knot_stride_AB ? N - 1 : 1, kQR = d->knot_stride_QR ? N - 1 : 1;
    const lqrx_dp_cost none{};
    const lqrx_dp_cost &ct = sc->J ? *cost : none;   // without J the cost is not read: nothing to stage
    enum { iA, iB, ic, iK, id, iQ, iR, iQf, iM, iq, ir, iqf, ix0, ial, iw, ilo, ihi, iX, iU, iJ, kBufs };
    static_assert(kBufs <= DpTable::kMaxRows + 1, "HostStage holds kMaxRows + 1 twins");
    HostBuf hb[kBufs];
    hb[iA] = host_in(A, n * n * kAB * es * bt);
    hb[iB] = host_in(B, n * m * kAB * es * bt);
    hb[ic] = host_in(c, n * kAB * es * bt);
    hb[iK] = host_in(K, m * n * (N - 1) * es * bt);
    hb[id] = host_in(dd, m * (N - 1) * es * bt);
    hb[iQ] = host_in(ct.Q, n * n * kQR * es * bt);
    hb[iR] = host_in(ct.R, m * m * kQR * es * bt);
    hb[iQf] = host_in(ct.Qf, n * n * es * bt);
    hb[iM] = host_in(ct.M, m * n * kQR * es * bt);
    hb[iq] = host_in(ct.q, n * kQR * es * bt);
    hb[ir] = host_in(ct.r, m * kQR * es * bt);
    hb[iqf] = host_in(ct.qf, n * es * bt);
    hb[ix0] = host_in(sc->x0, n * S * es * bt);
    hb[ial] = host_in(sc->alpha, S * es * bt);
    hb[iw] = host_in(sc->w, n * (N - 1) * S * es * bt);
    hb[ilo] = host_in(sc->u_lo, m * es * bt);
    hb[ihi] = host_in(sc->u_hi, m * es * bt);
    hb[iX] = HostBuf{sc->X, n * N * S * es * bt, H_OUT};   // only the outputs asked for have a twin
    hb[iU] = HostBuf{sc->U, m * (N - 1) * S * es * bt, H_OUT};
    hb[iJ] = HostBuf{sc->J, S * es * bt, H_OUT};
    HostStage dev;
    if ((st = dev.upload(hb, kBufs))) return st;
    const lqrx_dp_cost dcost{dev[iQ], dev[iR], dev[iQf], dev[iM], dev[iq], dev[ir], dev[iqf]};
    const lqrx_dp_scenarios dsc{sc->S, dev[ix0], dev[ial], dev[iw], dev[ilo], dev[ihi], dev[iX], dev[iU], dev[iJ]};
    st = lqrx_dp_rollout(d, dev[iA], dev[iB], dev[ic], dev[iK], dev[id], sc->J ? &dcost : nullptr, &dsc, nullptr);
    if (st < 0) return st;
    const int e = dev.download(hb, kBufs);
    return e ? e : st;
}

} // extern "C"

namespace {
// Descriptor checks shared by lqrx_dp_factor[_host] and lqrx_dp_resolve[_host]: layout 0, the shapes of
// the register-tile kernels
int validate_dp_resolve(const lqrx_dp_desc *d, const char *entry)
{
    if (!d) return set_err(-1, "desc is NULL");
    if (int st = validate_dp(d)) return st;
    if (d->layout != 0)
        return set_err(LQRX_ERR_UNSUPPORTED, "%s: desc.layout = 1 is not supported (layout 0 only)", entry);
    if (!lqrx::dp_resolve_supported(d->n, d->m))
        return set_err(LQRX_ERR_UNSUPPORTED, "%s: n=%d m=%d is past the kernels' n <= 64, m <= 32", entry, d->n, d->m);
    return 0;
}

// The arguments of lqrx_dp_factor[_host] behind desc: B 2, R 3, c 4 (optional), P 5, Einv 6, Pc 7, info 8 (optional)
int check_factor_args(const void *B, const void *R, const void *c, const void *P, const void *Einv, const void *Pc)
{
    if (!B) return set_err(-2, "pointer 2 (B) is NULL");
    if (!R) return set_err(-3, "pointer 3 (R) is NULL");
    if (!P) return set_err(-5, "pointer 5 (P) is NULL");
    if (!Einv) return set_err(-6, "pointer 6 (Einv) is NULL");
    if (c && !Pc) return set_err(-7, "pointer 7 (Pc) is NULL and c is given");
    if (!c && Pc) return set_err(-7, "pointer 7 (Pc) is given and c is NULL: there is nothing to form");
    return 0;
}

// The dynamics and factors of lqrx_dp_resolve[_host] and lqrx_dp_resolve_box[_host] behind desc: A 2, B 3,
// c 4 (optional), fac 5
int check_resolve_factors(const void *A, const void *B, const void *c, const lqrx_dp_factors *fac)
{
    if (!A) return set_err(-2, "pointer 2 (A) is NULL");
    if (!B) return set_err(-3, "pointer 3 (B) is NULL");
    if (!fac) return set_err(-5, "pointer 5 (fac) is NULL");
    if (!fac->K) return set_err(-5, "fac->K is NULL");
    if (!fac->Einv) return set_err(-5, "fac->Einv is NULL");
    if (c && !fac->Pc) return set_err(-5, "fac->Pc is NULL and c is given");
    if (!c && fac->Pc) return set_err(-5, "fac->Pc is given and c is NULL");
    return 0;
}

// The arguments of lqrx_dp_resolve[_host] behind desc: A 2, B 3, c 4 (optional), fac 5, rhs 6
int check_resolve_args(const void *A, const void *B, const void *c, const lqrx_dp_factors *fac, const lqrx_dp_rhs *rhs)
{
    if (int st = check_resolve_factors(A, B, c, fac)) return st;
    if (!rhs) return set_err(-6, "pointer 6 (rhs) is NULL");
    if (rhs->S < 1) return set_err(-6, "rhs->S must be >= 1 (got %lld)", (long long)rhs->S);
    if (!rhs->d && !rhs->p && !rhs->X && !rhs->U)
        return set_err(-6, "rhs->d, rhs->p, rhs->X and rhs->U are all NULL: nothing to compute");
    if (!rhs->d && (rhs->X || rhs->U))
        return set_err(-6, "rhs->d is NULL and rhs->%s is asked for: d carries the backward pass to the forward one",
                       rhs->X ? "X" : "U");
    return 0;
}

// The arguments of lqrx_dp_resolve_box[_host] behind desc: A 2, B 3, c 4 (optional), fac 5, rhs 6, box 7
int check_box_args(const void *A, const void *B, const void *c, const lqrx_dp_factors *fac, const lqrx_dp_rhs *rhs,
                   const lqrx_dp_box *box)
{
    if (int st = check_resolve_factors(A, B, c, fac)) return st;
    if (!rhs) return set_err(-6, "pointer 6 (rhs) is NULL");
    if (rhs->S < 1) return set_err(-6, "rhs->S must be >= 1 (got %lld)", (long long)rhs->S);
    if (!rhs->d) return set_err(-6, "rhs->d is NULL: d carries the backward pass to the forward one");
    if (rhs->p) return set_err(-6, "rhs->p must be NULL: the box entry forms no p");
    if (!box) return set_err(-7, "pointer 7 (box) is NULL");
    if (!(box->rho > 0) || !std::isfinite(box->rho)) return set_err(-7, "box->rho must be positive and finite (got %g)", box->rho);
    if (!(box->relax >= 1 && box->relax < 2)) return set_err(-7, "box->relax must be in [1, 2) (got %g)", box->relax);
    if (!(box->eps_prim >= 0)) return set_err(-7, "box->eps_prim must be >= 0 (got %g)", box->eps_prim);
    if (!(box->eps_dual >= 0)) return set_err(-7, "box->eps_dual must be >= 0 (got %g)", box->eps_dual);
    if (box->max_iter < 1 || box->max_iter > 10000)
        return set_err(-7, "box->max_iter must be in 1 ... 10000 (got %d)", box->max_iter);
    if (!box->Z) return set_err(-7, "box->Z is NULL");
    if (!box->W) return set_err(-7, "box->W is NULL");
    return 0;
}
} // namespace

extern "C" {

// E_k⁻¹ and P_{k+1}c_k of a solve, from its p_mode = 1 P (see lqrx.h): one kernel, no scratch
int lqrx_dp_factor(const lqrx_dp_desc *d, const void *B, const void *R, const void *c, const void *P, void *Einv,
                   void *Pc, int32_t *info, void *stream)
{
    int st = validate_dp_resolve(d, "lqrx_dp_factor");
    if (st) return st;
    if (d->p_mode != 1)
        return set_err(LQRX_ERR_UNSUPPORTED, "lqrx_dp_factor: desc.p_mode must be 1 (P holds every P_k)");
    if (d->batch == 0) return 0;
    if ((st = check_factor_args(B, R, c, P, Einv, Pc))) return st;
    lqrx::DpFactorArgs a{};
    a.B = B; a.R = R; a.c = c; a.P = P; a.Einv = Einv; a.Pc = Pc; a.info = info;
    a.n = d->n; a.m = d->m; a.N = d->N; a.dtype = d->dtype;
    a.tv_AB = (int)d->knot_stride_AB; a.tv_QR = (int)d->knot_stride_QR;
    a.batch = d->batch;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = lqrx::dp_factor_launch(a, s);
    if (e != hipSuccess) return hip_err(e, "factor kernel launch");
    if (stream == nullptr && (e = hipStreamSynchronize(nullptr)) != hipSuccess) return hip_err(e, "factor kernel");
    return 0;
}

int lqrx_dp_factor_host(const lqrx_dp_desc *d, const void *B, const void *R, const void *c, const void *P, void *Einv,
                        void *Pc, int32_t *info)
{
    int st = validate_dp_resolve(d, "lqrx_dp_factor_host");
    if (st) return st;
    if (d->p_mode != 1)
        return set_err(LQRX_ERR_UNSUPPORTED, "lqrx_dp_factor_host: desc.p_mode must be 1 (P holds every P_k)");
    if (d->batch == 0) return 0;
    if ((st = check_factor_args(B, R, c, P, Einv, Pc))) return st;
    const size_t es = dsize(d->dtype), bt = (size_t)d->batch, n = d->n, m = d->m, N = d->N;
    const size_t kAB = d->knot_stride_AB ? N - 1 : 1, kQR = d->knot_stride_QR ? N - 1 : 1;
    enum { iB, iR, ic, iP, iE, iPc, iinfo, kBufs };
    HostBuf hb[kBufs];
    hb[iB] = host_in(B, n * m * kAB * es * bt);
    hb[iR] = host_in(R, m * m * kQR * es * bt);
    hb[ic] = host_in(c, n * kAB * es * bt);
    hb[iP] = host_in(P, n * n * N * es * bt);
    hb[iE] = HostBuf{Einv, m * m * (N - 1) * es * bt, H_OUT};
    hb[iPc] = HostBuf{Pc, n * (N - 1) * es * bt, H_OUT};
    hb[iinfo] = HostBuf{info, 4 * bt, H_OUT};   // optional: no twin, and NULL to the kernel, when the caller passes none
    HostStage dev;
    if ((st = dev.upload(hb, kBufs))) return st;
    st = lqrx_dp_factor(d, dev[iB], dev[iR], dev[ic], dev[iP], dev[iE], dev[iPc], (int32_t *)dev[iinfo], nullptr);
    if (st < 0) return st;
    const int e = dev.download(hb, kBufs);
    return e ? e : st;
}

// S right-hand sides per problem on the factors of one solve (see lqrx.h): one kernel, no scratch
int lqrx_dp_resolve(const lqrx_dp_desc *d, const void *A, const void *B, const void *c, const lqrx_dp_factors *fac,
                    const lqrx_dp_rhs *rhs, void *stream)
{
    int st = validate_dp_resolve(d, "lqrx_dp_resolve");
    if (st) return st;
    if (d->batch == 0) return 0;
    if ((st = check_resolve_args(A, B, c, fac, rhs))) return st;
    lqrx::DpResolveArgs a{};
    a.A = A; a.B = B; a.c = c; a.K = fac->K; a.Einv = fac->Einv; a.Pc = fac->Pc;
    a.q = rhs->q; a.r = rhs->r; a.qf = rhs->qf; a.x0 = rhs->x0;
    a.d = rhs->d; a.p = rhs->p; a.X = rhs->X; a.U = rhs->U;
    a.n = d->n; a.m = d->m; a.N = d->N; a.dtype = d->dtype;
    a.tv_AB = (int)d->knot_stride_AB; a.tv_QR = (int)d->knot_stride_QR; a.p_all = d->p_mode;
    a.batch = d->batch; a.S = rhs->S;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = lqrx::dp_resolve_launch(a, s);
    if (e != hipSuccess) return hip_err(e, "re-solve kernel launch");
    if (stream == nullptr && (e = hipStreamSynchronize(nullptr)) != hipSuccess) return hip_err(e, "re-solve kernel");
    return 0;
}

int lqrx_dp_resolve_host(const lqrx_dp_desc *d, const void *A, const void *B, const void *c, const lqrx_dp_factors *fac,
                         const lqrx_dp_rhs *rhs)
{
    int st = validate_dp_resolve(d, "lqrx_dp_resolve_host");
    if (st) return st;
    if (d->batch == 0) return 0;
    if ((st = check_resolve_args(A, B, c, fac, rhs))) return st;
    const size_t es = dsize(d->dtype), bt = (size_t)d->batch, n = d->n, m = d->m, N = d->N, S = (size_t)rhs->S;
    const size_t kAB = d->knot_stride_AB ? N - 1 : 1, kQR = d->knot_stride_QR ? N - 1 : 1, kP = d->p_mode ? N : 1;
    enum { iA, iB, ic, iK, iE, iPc, iq, ir, iqf, ix0, id, ip, iX, iU, kBufs };
    HostBuf hb[kBufs];
    hb[iA] = host_in(A, n * n * kAB * es * bt);
    hb[iB] = host_in(B, n * m * kAB * es * bt);
    hb[ic] = host_in(c, n * kAB * es * bt);
    hb[iK] = host_in(fac->K, m * n * (N - 1) * es * bt);
    hb[iE] = host_in(fac->Einv, m * m * (N - 1) * es * bt);
    hb[iPc] = host_in(fac->Pc, n * (N - 1) * es * bt);
    hb[iq] = host_in(rhs->q, n * kQR * S * es * bt);
    hb[ir] = host_in(rhs->r, m * kQR * S * es * bt);
    hb[iqf] = host_in(rhs->qf, n * S * es * bt);
    hb[ix0] = host_in(rhs->x0, n * S * es * bt);
    hb[id] = HostBuf{rhs->d, m * (N - 1) * S * es * bt, H_OUT};   // only the outputs asked for have a twin
    hb[ip] = HostBuf{rhs->p, n * kP * S * es * bt, H_OUT};
    hb[iX] = HostBuf{rhs->X, n * N * S * es * bt, H_OUT};
    hb[iU] = HostBuf{rhs->U, m * (N - 1) * S * es * bt, H_OUT};
    HostStage dev;
    if ((st = dev.upload(hb, kBufs))) return st;
    const lqrx_dp_factors dfac{dev[iK], dev[iE], dev[iPc]};
    const lqrx_dp_rhs drhs{rhs->S, dev[iq], dev[ir], dev[iqf], dev[ix0], dev[id], dev[ip], dev[iX], dev[iU]};
    st = lqrx_dp_resolve(d, dev[iA], dev[iB], dev[ic], &dfac, &drhs, nullptr);
    if (st < 0) return st;
    const int e = dev.download(hb, kBufs);
    return e ? e : st;
}

// Input bounds by ADMM on the factors of one solve made with R + ρI (see lqrx.h): one kernel, no scratch
int lqrx_dp_resolve_box(const lqrx_dp_desc *d, const void *A, const void *B, const void *c, const lqrx_dp_factors *fac,
                        const lqrx_dp_rhs *rhs, const lqrx_dp_box *box, void *stream)
{
    int st = validate_dp_resolve(d, "lqrx_dp_resolve_box");
    if (st) return st;
    if (d->batch == 0) return 0;
    if ((st = check_box_args(A, B, c, fac, rhs, box))) return st;
    lqrx::DpBoxArgs a{};
    a.A = A; a.B = B; a.c = c; a.K = fac->K; a.Einv = fac->Einv; a.Pc = fac->Pc;
    a.q = rhs->q; a.r = rhs->r; a.qf = rhs->qf; a.x0 = rhs->x0;
    a.u_lo = box->u_lo; a.u_hi = box->u_hi;
    a.d = rhs->d; a.X = rhs->X; a.U = rhs->U; a.Z = box->Z; a.W = box->W; a.res = box->res; a.iters = box->iters;
    a.rho = box->rho; a.relax = box->relax; a.eps_prim = box->eps_prim; a.eps_dual = box->eps_dual;
    a.max_iter = box->max_iter;
    a.n = d->n; a.m = d->m; a.N = d->N; a.dtype = d->dtype;
    a.tv_AB = (int)d->knot_stride_AB; a.tv_QR = (int)d->knot_stride_QR;
    a.batch = d->batch; a.S = rhs->S;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = lqrx::dp_box_launch(a, s);
    if (e != hipSuccess) return hip_err(e, "box kernel launch");
    if (stream == nullptr && (e = hipStreamSynchronize(nullptr)) != hipSuccess) return hip_err(e, "box kernel");
    return 0;
}

int lqrx_dp_resolve_box_host(const lqrx_dp_desc *d, const void *A, const void *B, const void *c,
                             const lqrx_dp_factors *fac, const lqrx_dp_rhs *rhs, const lqrx_dp_box *box)
{
    int st = validate_dp_resolve(d, "lqrx_dp_resolve_box_host");
    if (st) return st;
    if (d->batch == 0) return 0;
    if ((st = check_box_args(A, B, c, fac, rhs, box))) return st;
    const size_t es = dsize(d->dtype), bt = (size_t)d->batch, n = d->n, m = d->m, N = d->N, S = (size_t)rhs->S;
    const size_t kAB = d->knot_stride_AB ? N - 1 : 1, kQR = d->knot_stride_QR ? N - 1 : 1;
    enum { iA, iB, ic, iK, iE, iPc, iq, ir, iqf, ix0, ilo, ihi, iZ, iW, id, iX, iU, iit, ires, kBufs };
    static_assert(kBufs <= DpTable::kMaxRows + 1, "HostStage holds kMaxRows + 1 twins");
    HostBuf hb[kBufs];
    hb[iA] = host_in(A, n * n * kAB * es * bt);
    hb[iB] = host_in(B, n * m * kAB * es * bt);
    hb[ic] = host_in(c, n * kAB * es * bt);
    hb[iK] = host_in(fac->K, m * n * (N - 1) * es * bt);
    hb[iE] = host_in(fac->Einv, m * m * (N - 1) * es * bt);
    hb[iPc] = host_in(fac->Pc, n * (N - 1) * es * bt);
    hb[iq] = host_in(rhs->q, n * kQR * S * es * bt);
    hb[ir] = host_in(rhs->r, m * kQR * S * es * bt);
    hb[iqf] = host_in(rhs->qf, n * S * es * bt);
    hb[ix0] = host_in(rhs->x0, n * S * es * bt);
    hb[ilo] = host_in(box->u_lo, m * es * bt);
    hb[ihi] = host_in(box->u_hi, m * es * bt);
    hb[iZ] = HostBuf{box->Z, m * (N - 1) * S * es * bt, H_INOUT};
    hb[iW] = HostBuf{box->W, m * (N - 1) * S * es * bt, H_INOUT};
    hb[id] = HostBuf{rhs->d, m * (N - 1) * S * es * bt, H_OUT};   // only the outputs asked for have a twin
    hb[iX] = HostBuf{rhs->X, n * N * S * es * bt, H_OUT};
    hb[iU] = HostBuf{rhs->U, m * (N - 1) * S * es * bt, H_OUT};
    hb[iit] = HostBuf{box->iters, 4 * S * bt, H_OUT};
    hb[ires] = HostBuf{box->res, 2 * S * es * bt, H_OUT};
    HostStage dev;
    if ((st = dev.upload(hb, kBufs))) return st;
    const lqrx_dp_factors dfac{dev[iK], dev[iE], dev[iPc]};
    const lqrx_dp_rhs drhs{rhs->S, dev[iq], dev[ir], dev[iqf], dev[ix0], dev[id], nullptr, dev[iX], dev[iU]};
    lqrx_dp_box dbox = *box;
    dbox.u_lo = dev[ilo]; dbox.u_hi = dev[ihi]; dbox.Z = dev[iZ]; dbox.W = dev[iW];
    dbox.iters = (int32_t *)dev[iit]; dbox.res = dev[ires];
    st = lqrx_dp_resolve_box(d, dev[iA], dev[iB], dev[ic], &dfac, &drhs, &dbox, nullptr);
    if (st < 0) return st;
    const int e = dev.download(hb, kBufs);
    return e ? e : st;
}

// Gradients of a loss ℓ(X, U) through the solve: one more cross solve with ∂ℓ/∂X, ∂ℓ/∂U as the
// linear cost terms (x0' = 0, c' = 0), its costates, and the rank-2 assembly (see lqrx.h)
int lqrx_dp_solve_adjoint(const lqrx_dp_desc *d, const void *A, const void *B, const void *Q, const void *R,
                          const void *M, const void *Qf, const void *X, const void *U, const void *lam,
                          const lqrx_dp_grad *grad, int32_t *info, void *stream)
{
    int st = validate_dp_adjoint(d, "lqrx_dp_solve_adjoint");
    if (st) return st;
    if (d->knot_stride_QR != 1)
        return set_err(LQRX_ERR_UNSUPPORTED, "lqrx_dp_solve_adjoint: desc.knot_stride_QR must be 1 (dl/dX and dl/dU "
                                             "take the place of per-knot q, r): broadcast Q, R, M over the knots");
    if (d->batch == 0) return 0;
    const void *in[9] = {A, B, Q, R, M, Qf, X, U, lam};
    static const char *inm[9] = {"A", "B", "Q", "R", "M", "Qf", "X", "U", "lam"};
    for (int i = 0; i < 9; ++i)
        if (!in[i]) return set_err(-(i + 2), "input pointer %d (%s) is NULL", i + 2, inm[i]);
    if (!grad) return set_err(-11, "grad is NULL");
    if (!grad->gX || !grad->gU) return set_err(-11, "grad->%s is NULL", grad->gX ? "gU" : "gX");

    const size_t es = dsize(d->dtype), bt = (size_t)d->batch, n = d->n, m = d->m, N = d->N;
    const int tvAB = (int)d->knot_stride_AB;
    // scratch of the adjoint solve, elements per trajectory: q' n(N−1), qf' n, c' n(N−1 | 1), x0' n,
    // K' mn(N−1), P'_1 n², X' nN, U' m(N−1), d' m(N−1), p'_1 n, λ' nN — and info' when the caller passes none
    const size_t cnt[11] = {n * (N - 1), n, n * (tvAB ? N - 1 : 1), n, m * n * (N - 1), n * n,
                            n * N, m * (N - 1), m * (N - 1), n, n * N};
    size_t off[12], total = 0;
    for (int i = 0; i < 11; ++i) {
        off[i] = total;
        total += (cnt[i] * bt * es + 255) & ~(size_t)255;
    }
    off[11] = total;
    if (!info) total += (4 * bt + 255) & ~(size_t)255;
    hipStream_t s = (hipStream_t)stream;
    void *blk = nullptr;
    hipError_t e = lqrx::scratch_alloc(&blk, total, s);
    if (e != hipSuccess) return hip_err(e, "adjoint scratch");
    char *b = (char *)blk;
    void *qa = b + off[0], *qfa = b + off[1], *ca = b + off[2], *x0a = b + off[3], *Ka = b + off[4];
    void *Pa = b + off[5], *Xa = b + off[6], *Ua = b + off[7], *da = b + off[8], *pa = b + off[9], *lama = b + off[10];
    int32_t *infoa = info ? info : (int32_t *)(b + off[11]);
    const char *what = "adjoint pack";
    e = lqrx::dp_adjoint_pack_launch(grad->gX, qa, qfa, (int)n, (int)N, d->batch, d->dtype, s);
    if (e == hipSuccess) {
        what = "adjoint zero fill";   // c' and x0' are adjacent in the block
        e = hipMemsetAsync(ca, 0, off[4] - off[2], s);
    }
    if (e == hipSuccess) {
        what = "adjoint solve";
        lqrx_dp_desc d1 = *d;   // layout 0 and per-knot Q, R already; P_1 and p_1 only
        d1.p_mode = 0;
        const lqrx_dp_linear la{qa, grad->gU, qfa, da, pa};
        const DpTable t(&d1, DP_CROSS, DpPtrs{A, B, ca, Q, R, M, Qf, x0a, &la, nullptr, Ka, Pa, Xa, Ua, infoa});
        e = lqrx::dp_launch(dp_args(&d1, t, infoa), s);
    }
    if (e == hipSuccess) {
        what = "adjoint costates";
        e = lqrx::dp_costate_launch(costate_args(d, CostatePtrs{A, B, Q, R, M, Qf, qa, grad->gU, qfa, Ka, Xa, Ua, lama}), s);
    }
    if (e == hipSuccess) {
        what = "adjoint assembly";
        lqrx::DpGradArgs g{};
        g.X = X; g.U = U; g.lam = lam; g.Xa = Xa; g.Ua = Ua; g.lama = lama;
        g.gA = grad->gA; g.gB = grad->gB; g.gc = grad->gc; g.gQ = grad->gQ; g.gR = grad->gR; g.gM = grad->gM;
        g.gQf = grad->gQf; g.gx0 = grad->gx0; g.gq = grad->gq; g.gr = grad->gr; g.gqf = grad->gqf;
        g.n = d->n; g.m = d->m; g.N = d->N; g.dtype = d->dtype; g.tv_AB = tvAB; g.batch = d->batch;
        e = lqrx::dp_grad_launch(g, s);
    }
    int any = 0;
    if (e == hipSuccess && stream == nullptr) {
        what = "adjoint kernels";
        e = hipStreamSynchronize(nullptr);
        if (e == hipSuccess && info) {
            std::vector<int32_t> h(bt);
            e = hipMemcpy(h.data(), info, bt * 4, hipMemcpyDeviceToHost);
            for (int32_t v : h)
                if (v) any = 1;
        }
    }
    const hipError_t ef = lqrx::scratch_free(blk, s);
    if (e == hipErrorNotSupported) return set_err(LQRX_ERR_UNSUPPORTED, "no kernel for n=%d m=%d", d->n, d->m);
    if (e != hipSuccess) return hip_err(e, what);
    if (ef != hipSuccess) return hip_err(ef, "adjoint scratch free");
    return any;
}


// ------------------------------------------------------------------ KKT
namespace {
struct KktLayout {
    std::vector<int32_t> meta; // per knot: n1, p, n2, w, oY, oy, oH, og
    int64_t sY = 0, sy = 0, sH = 0, sg = 0;
    int maxw = 0, maxrows = 0, max_p1 = 0, max_ps = 0, max_p2 = 0;
};

int kkt_layout(const lqrx_kkt_desc *d, KktLayout &L)
{
    if (!d) return set_err(-1, "desc is NULL");
    if (d->N < 1) return set_err(-1, "desc.N must be >= 1");
    if (d->dtype != LQRX_F64 && d->dtype != LQRX_F32)
        return set_err(-1, "desc.dtype must be LQRX_F64 or LQRX_F32 (got %d)", d->dtype);
    if (d->batch < 0) return set_err(-1, "desc.batch must be >= 0");
    if (!d->n1 || !d->p || !d->n2 || !d->w) return set_err(-1, "block-size arrays are NULL");
    if (d->h_mode < 0 || d->h_mode > 2) return set_err(-1, "desc.h_mode must be 0, 1 or 2");
    if (d->ginv != 0 && d->ginv != 1) return set_err(-1, "desc.ginv must be 0 or 1");
    if (d->layout != 0 && d->layout != 1)
        return set_err(-1, "desc.layout must be 0 (per trajectory) or 1 (batch fastest) (got %d)", d->layout);
    L.meta.assign((size_t)d->N * 8, 0);
    for (int k = 0; k < d->N; ++k) {
        int n1 = d->n1[k], p = d->p[k], n2 = d->n2[k], w = d->w[k];
        if (n1 < 0 || p < 0 || n2 < 0 || w < 1)
            return set_err(-1, "knot %d: negative block size or w < 1", k);
        if (k == 0 && n1 != 0) return set_err(-1, "knot 0 must have n1 == 0");
        if (k > 0 && n1 != d->n2[k - 1])
            return set_err(-1, "knot %d: n1 (%d) != n2 of knot %d (%d)", k, n1, k - 1, d->n2[k - 1]);
        if (k == d->N - 1 && n2 != 0) return set_err(-1, "last knot must have n2 == 0");
        int rows = n1 + p + n2;
        if (n1 > lqrx::KW_MAX_BLOCK || p > lqrx::KW_MAX_BLOCK || n2 > lqrx::KW_MAX_BLOCK || w > lqrx::KW_MAX_W)
            return set_err(LQRX_ERR_UNSUPPORTED, "knot %d: block (n1 %d, p %d, n2 %d, w %d) past %d rows per "
                                                 "part / %d columns", k, n1, p, n2, w, lqrx::KW_MAX_BLOCK,
                           lqrx::KW_MAX_W);
        int32_t *m = &L.meta[(size_t)k * 8];
        m[0] = n1; m[1] = p; m[2] = n2; m[3] = w;
        m[4] = (int32_t)L.sY; m[5] = (int32_t)L.sy; m[6] = (int32_t)L.sH; m[7] = (int32_t)L.sg;
        L.sY += (int64_t)rows * w;
        L.sy += p + n2;
        L.sH += d->h_mode == 2 ? w : (int64_t)w * w;
        L.sg += w;
        L.maxw = std::max(L.maxw, w);
        L.maxrows = std::max(L.maxrows, rows);
        L.max_p1 = std::max(L.max_p1, n1);
        L.max_ps = std::max(L.max_ps, p);
        L.max_p2 = std::max(L.max_p2, n2);
    }
    if (L.sY > INT32_MAX) return set_err(LQRX_ERR_UNSUPPORTED, "trajectory too large");
    // layout 1: every array's element rows are addressed with 32-bit byte offsets
    if (d->layout == 1 && std::max(std::max(L.sY, L.sy), std::max(L.sH, L.sg)) * d->batch * 8 > INT32_MAX)
        return set_err(LQRX_ERR_UNSUPPORTED, "layout 1: arrays above 2 GiB (split the batch)");
    return 0;
}
// Per-device cache of uploaded structure tables (process-wide, mutex-guarded), keyed on the
// stream's device.  A structure's table is uploaded by a blocking copy on its first use;
// afterwards a solve issues no host→device traffic besides the launch.  (A per-call
// stream-ordered alloc + pageable async copy was observed to leave the device table stale on
// repeated calls with alternating structures.)  The cache holds at most meta_cache_cap() tables
// and never evicts (nothing is freed under work in flight on another stream); structures
// beyond that get a per-call table from the stream-ordered pool, copied and waited for on
// the CALL's stream only (*tmp set: the caller frees it, stream-ordered, after the launch).
size_t meta_cache_cap()   // LQRX_META_CACHE overrides 4096 (tests exercise the overflow path)
{
    static const size_t v = [] { const char *e = std::getenv("LQRX_META_CACHE"); return e ? (size_t)std::strtoull(e, nullptr, 10) : (size_t)4096; }();
    return v;
}
int device_meta(const std::vector<int32_t> &meta, hipStream_t s, const int32_t **out, void **tmp)
{
    static std::mutex mu;
    static std::map<std::pair<int, std::vector<int32_t>>, int32_t *> cache;
    *tmp = nullptr;
    int dev = 0;
    hipError_t e = lqrx::stream_device(s, &dev);
    if (e != hipSuccess) return hip_err(e, "stream device");
    const size_t bytes = meta.size() * sizeof(int32_t);
    std::lock_guard<std::mutex> lock(mu);
    auto key = std::make_pair(dev, meta);
    auto it = cache.find(key);
    if (it != cache.end()) {
        *out = it->second;
        return 0;
    }
    if (cache.size() >= meta_cache_cap()) {
        if ((e = lqrx::scratch_alloc(tmp, bytes, s)) != hipSuccess) return hip_err(e, "meta scratch");
        if ((e = hipMemcpyAsync(*tmp, meta.data(), bytes, hipMemcpyHostToDevice, s)) != hipSuccess ||
            (e = hipStreamSynchronize(s)) != hipSuccess) {
            (void)lqrx::scratch_free(*tmp, s);
            *tmp = nullptr;
            return hip_err(e, "meta H2D");
        }
        *out = (const int32_t *)*tmp;
        return 0;
    }
    int prev = -1;
    if ((e = hipGetDevice(&prev)) != hipSuccess) return hip_err(e, "hipGetDevice");
    if (prev != dev && (e = hipSetDevice(dev)) != hipSuccess) return hip_err(e, "hipSetDevice");
    int32_t *d = nullptr;
    e = hipMalloc((void **)&d, bytes);
    if (e == hipSuccess && (e = hipMemcpy(d, meta.data(), bytes, hipMemcpyHostToDevice)) != hipSuccess) {
        (void)hipFree(d);
        d = nullptr;
    }
    if (prev != dev) (void)hipSetDevice(prev);
    if (e != hipSuccess) return hip_err(e, "meta upload");
    cache.emplace(std::move(key), d);
    *out = d;
    return 0;
}
} // namespace

extern "C" int lqrx_kkt_sizes(const lqrx_kkt_desc *d, int64_t *nY, int64_t *ny, int64_t *nH,
                              int64_t *ng, int64_t *nlam)
{
    KktLayout L;
    int st = kkt_layout(d, L);
    if (st) return st;
    if (nY) *nY = L.sY;
    if (ny) *ny = L.sy;
    if (nH) *nH = L.sH;
    if (ng) *ng = L.sg;
    if (nlam) *nlam = L.sy;
    return 0;
}

namespace {
bool kkt_force_generic();
// kernel arguments of one KKT call (no device pointers yet)
lqrx::KktArgs kkt_args(const lqrx_kkt_desc *d, const KktLayout &L)
{
    lqrx::KktArgs a{};
    a.N = d->N; a.h_mode = d->h_mode; a.ginv = d->ginv; a.batch = d->batch;
    a.sY = L.sY; a.sy = L.sy; a.sH = L.sH; a.sg = L.sg; a.sl = L.sy;
    a.maxw = L.maxw; a.maxrows = L.maxrows;
    a.max_p1 = L.max_p1; a.max_ps = L.max_ps; a.max_p2 = L.max_p2;
    static const int force_lane = [] { const char *v = std::getenv("LQRX_KKT_FORCE_LANE"); return v && *v == '1'; }();
    a.force_lane = force_lane;
    a.layout = d->layout;
    a.dtype = d->dtype == LQRX_F32 ? 1 : 0;
    return a;
}
// Kernel family for a call.  fp32: the large-block MFMA kernels, past them the
// workgroup-per-trajectory kernel.  fp64: the compile-time shapes (FIL) first, then the
// LDS-staged / small lane generic kernels, then the large-block kernels (which also replace the
// scratch-spilling lane<8,8,8,12,16> kernel), then the workgroup-per-trajectory kernel (blocks
// past 64 rows / w past 128).  LQRX_KKT_BIG=1 forces the large-block kernels wherever they
// apply, =0 never uses them; LQRX_KKT_WG=1 forces the workgroup kernel (layout 0; A/B tests).
enum { KK_NONE = 0, KK_FIL, KK_GENERIC, KK_BIG, KK_WG };
int kkt_big_env()
{
    static const int v = [] { const char *e = std::getenv("LQRX_KKT_BIG"); return e && *e ? std::atoi(e) : -1; }();
    return v;
}
int kkt_wg_env()
{
    static const int v = [] { const char *e = std::getenv("LQRX_KKT_WG"); return e && *e == '1' ? 1 : 0; }();
    return v;
}
int kkt_route(const lqrx_kkt_desc *d, const lqrx::KktArgs &a)
{
    if (a.layout == 1) {   // SoA read natively by the compile-time shapes (fp64); else staged
        size_t b = 0;
        const bool fil = d->dtype == LQRX_F64 && !a.force_lane && !kkt_force_generic() &&
                         lqrx::kkt_fil_scratch_bytes(a, d->n1, d->p, d->n2, d->w, &b);
        return fil ? KK_FIL : KK_NONE;
    }
    const bool wgk = lqrx::kkt_wg_supported(a, d->n1, d->p, d->n2, d->w);
    if (kkt_wg_env() && wgk) return KK_WG;
    const bool big = kkt_big_env() != 0 && lqrx::kkt_big_supported(a, d->n1, d->p, d->n2, d->w);
    if (d->dtype == LQRX_F32) return big ? KK_BIG : wgk ? KK_WG : KK_NONE;
    if (kkt_big_env() == 1 && big) return KK_BIG;
    size_t b = 0;
    const bool fil = !a.force_lane && !kkt_force_generic() && lqrx::kkt_fil_scratch_bytes(a, d->n1, d->p, d->n2, d->w, &b);
    if (fil) return KK_FIL;
    const int gc = lqrx::kkt_generic_class(a);
    if (gc == 1 || gc == 2 || (gc == 3 && (!big || a.force_lane))) return KK_GENERIC;
    return big ? KK_BIG : wgk ? KK_WG : KK_NONE;
}
// LQRX_KKT_GENERIC=1 forces the generic (runtime-shaped) kernel, for A/B checks
bool kkt_force_generic()
{
    static const bool v = [] { const char *e = std::getenv("LQRX_KKT_GENERIC"); return e && *e == '1'; }();
    return v;
}
// workspace bytes of the kernel family `route` (kkt_route of the same call: sizing and launch
// use one routing decision)
size_t kkt_ws_bytes(const lqrx_kkt_desc *d, const lqrx::KktArgs &a, int route)
{
    size_t b = 0;
    switch (route) {
    case KK_FIL: (void)lqrx::kkt_fil_scratch_bytes(a, d->n1, d->p, d->n2, d->w, &b); return b;
    case KK_BIG: return lqrx::kkt_big_scratch_bytes(a, d->n1, d->p, d->n2, d->w);
    case KK_WG: return lqrx::kkt_wg_scratch_bytes(a, d->n1, d->p, d->n2, d->w);
    case KK_GENERIC: return lqrx::kkt_scratch_bytes(a);
    default: return 0;
    }
}
// a layout-1 call staged through layout 0: the six transposed arrays (Y y H g | dz λ), each
// 256-B aligned — part of the call's workspace (lqrx_kkt_workspace_size counts them)
size_t kkt_stage_bytes(const lqrx_kkt_desc *d, const KktLayout &L, size_t soff[6] = nullptr)
{
    const size_t es = d->dtype == LQRX_F32 ? 4 : 8, B = (size_t)d->batch;
    const int64_t S[6] = {L.sY, L.sy, L.sH, L.sg, L.sg, L.sy};
    size_t tot = 0;
    for (int i = 0; i < 6; ++i) {
        if (soff) soff[i] = tot;
        tot += ((size_t)S[i] * B * es + 255) & ~(size_t)255;
    }
    return tot;
}
int kkt_solve_impl(const lqrx_kkt_desc *d, const void *Y, const void *y, const void *H, const void *g,
                   void *dz, void *lam, int32_t *info, void *ws, size_t ws_bytes, void *stream,
                   bool null_sync = true, const int32_t *sel = nullptr, const int32_t *nsel = nullptr);
} // namespace

extern "C" int lqrx_kkt_workspace_size(const lqrx_kkt_desc *d, size_t *bytes)
{
    KktLayout L;
    int st = kkt_layout(d, L);
    if (st) return st;
    if (!bytes) return set_err(-2, "bytes is NULL");
    if (d->batch) {
        lqrx::KktArgs a = kkt_args(d, L);
        int route = kkt_route(d, a);
        size_t stage = 0;
        if (route == KK_NONE && a.layout == 1) {   // staged through layout 0 (kkt_solve_impl)
            a.layout = 0;
            route = kkt_route(d, a);
            if (route != KK_NONE) stage = kkt_stage_bytes(d, L);
        }
        *bytes = stage + kkt_ws_bytes(d, a, route);
    } else {
        *bytes = 0;
    }
    return 0;
}

extern "C" int lqrx_kkt_solve(const lqrx_kkt_desc *d, const void *Y, const void *y, const void *H,
                              const void *g, void *dz, void *lam, int32_t *info, void *stream)
{
    return kkt_solve_impl(d, Y, y, H, g, dz, lam, info, nullptr, 0, stream);
}

extern "C" int lqrx_kkt_solve_ws(const lqrx_kkt_desc *d, const void *Y, const void *y, const void *H,
                                 const void *g, void *dz, void *lam, int32_t *info, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    if (!workspace) return set_err(-9, "workspace is NULL");
    return kkt_solve_impl(d, Y, y, H, g, dz, lam, info, workspace, workspace_bytes, stream);
}

namespace {
int kkt_solve_impl(const lqrx_kkt_desc *d, const void *Y, const void *y, const void *H, const void *g,
                   void *dz, void *lam, int32_t *info, void *ws, size_t ws_bytes, void *stream, bool null_sync,
                   const int32_t *sel, const int32_t *nsel)
{
    KktLayout L;
    int st = kkt_layout(d, L);
    if (st) return st;
    if (d->batch == 0) return 0;
    const void *in[4] = {Y, y, H, g};
    for (int i = 0; i < 4; ++i)
        if (!in[i]) return set_err(-(i + 2), "input pointer %d is NULL", i + 2);
    if (!dz) return set_err(-6, "dz is NULL");
    if (!lam) return set_err(-7, "lam is NULL");
    hipStream_t s = (hipStream_t)stream;
    // device copy of the block-structure table, uploaded once per distinct structure
    const int32_t *dmeta = nullptr;
    void *meta_tmp = nullptr;
    if ((st = device_meta(L.meta, s, &dmeta, &meta_tmp))) return st;
    hipError_t e;
    lqrx::KktArgs a = kkt_args(d, L);
    a.Y = (const double *)Y; a.y = (const double *)y; a.H = (const double *)H; a.g = (const double *)g;
    a.dz = (double *)dz; a.lam = (double *)lam; a.info = info; a.meta = dmeta;
    // a trajectory subset (internal, SQP): per-lane offsets of the selected trajectories are
    // 32-bit in the layout-0 kernel
    if (sel && nsel && d->layout == 0 &&
        std::max(std::max(L.sY, L.sy), std::max(L.sH, L.sg)) * d->batch * 8 <= INT32_MAX) {
        a.sel = sel;
        a.nsel = nsel;
    }
    // one routing decision per call (the large-block plan is an O(N) pass over the structure)
    int route = kkt_route(d, a);
    // layout 1 without a compile-time shape: the SoA arrays are transposed to layout 0 in a
    // stream-ordered scratch block, solved by the layout-0 kernel family, and dz / λ transposed
    // back (one extra read + write of every array)
    bool staged = false;
    if (route == KK_NONE && a.layout == 1) {
        a.layout = 0;
        route = kkt_route(d, a);
        staged = route != KK_NONE;
        if (!staged) a.layout = 1;
    }
    // the staged arrays: at the front of the caller's workspace (counted by
    // lqrx_kkt_workspace_size: a _ws call draws nothing from the pool), else from the pool
    size_t soff[6];
    const size_t stot = staged ? kkt_stage_bytes(d, L, soff) : 0;
    if (ws) {
        const size_t need = stot + kkt_ws_bytes(d, a, route);
        if (ws_bytes < need) {
            if (meta_tmp) (void)lqrx::scratch_free(meta_tmp, s);
            return set_err(-10, "workspace of %zu bytes < %zu (lqrx_kkt_workspace_size)", ws_bytes, need);
        }
        a.ws = (char *)ws + stot;
        a.ws_bytes = ws_bytes - stot;
    }
    static const int debug_meta = [] { const char *v = std::getenv("LQRX_DEBUG_META"); return v && *v == '1'; }();
    if (route == KK_NONE) {
        if (meta_tmp) (void)lqrx::scratch_free(meta_tmp, s);
        return set_err(LQRX_ERR_UNSUPPORTED, "no KKT kernel for this structure / options (%s; layout 0 serves "
                                             "every structure with blocks <= %d rows and w <= %d, every h_mode "
                                             "and ginv)",
                       d->dtype == LQRX_F32 ? "fp32" : "fp64", lqrx::KW_MAX_BLOCK, lqrx::KW_MAX_W);
    }
    void *stage = nullptr, *pooled = nullptr;
    const int64_t es = d->dtype == LQRX_F32 ? 4 : 8, B = d->batch;
    const int64_t S[6] = {L.sY, L.sy, L.sH, L.sg, L.sg, L.sy};   // Y y H g | dz lam
    if (staged) {
        if (ws) {
            stage = ws;
            e = hipSuccess;
        } else {
            e = lqrx::scratch_alloc(&pooled, stot, s);
            stage = pooled;
        }
        const void *src[4] = {Y, y, H, g};
        const double **dst[4] = {&a.Y, &a.y, &a.H, &a.g};
        for (int i = 0; i < 4 && e == hipSuccess; ++i) {      // [S][B] → [B][S]
            *dst[i] = (const double *)((char *)stage + soff[i]);
            e = lqrx::batch_transpose(src[i], (char *)stage + soff[i], S[i], B, (int)es, s);
        }
        a.dz = (double *)((char *)stage + soff[4]);
        a.lam = (double *)((char *)stage + soff[5]);
        a.sel = nullptr;
        a.nsel = nullptr;
    } else {
        e = hipSuccess;
    }
    if (e != hipSuccess) {
    } else if (route == KK_BIG) e = lqrx::kkt_big_launch(a, d->n1, d->p, d->n2, d->w, s);
    else if (route == KK_WG) e = lqrx::kkt_wg_launch(a, d->n1, d->p, d->n2, d->w, s);
    else if (route == KK_GENERIC || !lqrx::kkt_fil_launch(a, d->n1, d->p, d->n2, d->w, s, &e))
        e = lqrx::kkt_launch(a, s);
    if (staged && e == hipSuccess) {                          // [B][S] → [S][B]
        e = lqrx::batch_transpose(a.dz, dz, B, S[4], (int)es, s);
        if (e == hipSuccess) e = lqrx::batch_transpose(a.lam, lam, B, S[5], (int)es, s);
    }
    if (pooled) {
        const hipError_t ef = lqrx::scratch_free(pooled, s);
        if (e == hipSuccess) e = ef;
    }
    if (debug_meta) {   // read the table back before a per-call table is released
        std::vector<int32_t> back(L.meta.size());
        (void)hipStreamSynchronize(s);
        (void)hipMemcpy(back.data(), dmeta, L.meta.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (back != L.meta) std::fprintf(stderr, "LQRX_DEBUG_META: device meta differs from host\n");
    }
    if (meta_tmp) (void)lqrx::scratch_free(meta_tmp, s);   // stream-ordered after the launch
    if (e == hipErrorNotSupported) return set_err(LQRX_ERR_UNSUPPORTED, "KKT kernel unavailable");
    if (e != hipSuccess) return hip_err(e, "kkt kernel launch");
    if (stream == nullptr && null_sync) {
        e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) return hip_err(e, "kkt kernel");
        if (info) {
            std::vector<int32_t> h((size_t)d->batch);
            e = hipMemcpy(h.data(), info, h.size() * 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return hip_err(e, "info D2H");
            for (int32_t v : h)
                if (v) return 1;
        }
    }
    return 0;
}
} // namespace

extern "C" int lqrx_kkt_solve_host(const lqrx_kkt_desc *d, const void *Y, const void *y,
                                   const void *H, const void *g, void *dz, void *lam,
                                   int32_t *info)
{
    KktLayout L;
    int st = kkt_layout(d, L);
    if (st) return st;
    if (d->batch == 0) return 0;
    const size_t bt = (size_t)d->batch, es = d->dtype == LQRX_F32 ? 4 : 8;
    const size_t szin[4] = {(size_t)L.sY, (size_t)L.sy, (size_t)L.sH, (size_t)L.sg};
    const void *hin[4] = {Y, y, H, g};
    DevBuf din[4], ddz, dlam, dinfo;
    for (int i = 0; i < 4; ++i) {
        if (!hin[i]) return set_err(-(i + 2), "input pointer %d is NULL", i + 2);
        if ((st = dev_alloc(din[i], szin[i] * es * bt, "hipMalloc input"))) return st;
        hipError_t e = hipMemcpy(din[i].p, hin[i], szin[i] * es * bt, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_err(e, "H2D");
    }
    if (!dz) return set_err(-6, "dz is NULL");
    if (!lam) return set_err(-7, "lam is NULL");
    if ((st = dev_alloc(ddz, (size_t)L.sg * es * bt, "hipMalloc dz"))) return st;
    if ((st = dev_alloc(dlam, (size_t)L.sy * es * bt, "hipMalloc lam"))) return st;
    if ((st = dev_alloc(dinfo, 4 * bt, "hipMalloc info"))) return st;
    st = lqrx_kkt_solve(d, din[0].p, din[1].p, din[2].p, din[3].p, ddz.p, dlam.p,
                        (int32_t *)dinfo.p, nullptr);
    if (st < 0) return st;
    hipError_t e = hipMemcpy(dz, ddz.p, (size_t)L.sg * es * bt, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(lam, dlam.p, (size_t)L.sy * es * bt, hipMemcpyDeviceToHost);
    if (e == hipSuccess && info) e = hipMemcpy(info, dinfo.p, 4 * bt, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_err(e, "D2H");
    return st;
}

// ------------------------------------------------------------------ generator
static inline uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static inline double gauss(uint64_t seed, uint64_t traj, uint64_t field, uint64_t elem)
{
    uint64_t h = splitmix64(seed ^ splitmix64(traj ^ splitmix64((field << 40) ^ elem)));
    uint64_t h2 = splitmix64(h);
    double u1 = ((h >> 11) + 1.0) * (1.0 / 9007199254740992.0); // (0, 1]
    double u2 = (h2 >> 11) * (1.0 / 9007199254740992.0);        // [0, 1)
    return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
}

static void gen_one(int n, int m, uint64_t seed, uint64_t t, double *A, double *B, double *Q,
                    double *R, double *Qf, double *x0, std::vector<double> &G)
{
    const double sn = std::sqrt((double)n);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i)
            A[i + j * n] = (i == j ? 1.0 : 0.0) + (0.1 / sn) * gauss(seed, t, 0, i + j * n);
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < n; ++i) B[i + j * n] = gauss(seed, t, 1, i + j * n) / sn;
    G.resize((size_t)n * n);
    for (int e = 0; e < n * n; ++e) G[e] = gauss(seed, t, 2, e);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            double s = 0.0;
            for (int p = 0; p < n; ++p) s += G[p + i * n] * G[p + j * n];
            Q[i + j * n] = (i == j ? 1.0 : 0.0) + s / n;
        }
    G.resize((size_t)m * m);
    for (int e = 0; e < m * m; ++e) G[e] = gauss(seed, t, 3, e);
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) {
            double s = 0.0;
            for (int p = 0; p < m; ++p) s += G[p + i * m] * G[p + j * m];
            R[i + j * m] = (i == j ? 1.0 : 0.0) + s / m;
        }
    for (int e = 0; e < n * n; ++e) Qf[e] = 10.0 * Q[e];
    for (int i = 0; i < n; ++i) x0[i] = gauss(seed, t, 4, i);
}

int lqrx_make_random_dp(int32_t n, int32_t m, int64_t batch, int64_t traj0, uint64_t seed,
                        int32_t dtype, void *A, void *B, void *Q, void *R, void *Qf, void *x0)
{
    if (n < 1) return set_err(-1, "n must be >= 1");
    if (m < 1) return set_err(-2, "m must be >= 1");
    if (batch < 0) return set_err(-3, "batch must be >= 0");
    if (dtype != LQRX_F64 && dtype != LQRX_F32) return set_err(-6, "bad dtype");
    void *outs[6] = {A, B, Q, R, Qf, x0};
    for (int i = 0; i < 6; ++i)
        if (!outs[i]) return set_err(-(7 + i), "output pointer is NULL");
    const size_t nn = (size_t)n * n, nm = (size_t)n * m, mm = (size_t)m * m;
    unsigned nth = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    if ((int64_t)nth > batch) nth = (unsigned)std::max<int64_t>(1, batch);
    auto work = [&](unsigned tid) {
        std::vector<double> a(nn), b(nm), q(nn), r(mm), qf(nn), x(n), G;
        for (int64_t t = tid; t < batch; t += nth) {
            gen_one(n, m, seed, (uint64_t)(traj0 + t), a.data(), b.data(), q.data(), r.data(),
                    qf.data(), x.data(), G);
            auto put = [&](void *dst, const std::vector<double> &src, size_t cnt) {
                if (dtype == LQRX_F64)
                    std::memcpy((double *)dst + t * cnt, src.data(), cnt * 8);
                else
                    for (size_t e = 0; e < cnt; ++e) ((float *)dst)[t * cnt + e] = (float)src[e];
            };
            put(A, a, nn); put(B, b, nm); put(Q, q, nn); put(R, r, mm); put(Qf, qf, nn);
            put(x0, x, n);
        }
    };
    std::vector<std::thread> th;
    for (unsigned i = 1; i < nth; ++i) th.emplace_back(work, i);
    work(0);
    for (auto &t : th) t.join();
    return 0;
}

} // extern "C"

// ------------------------------------------------------------------ multi-device host entries
// SURVEY §8(e) through the drop-in boundary: the batch split into contiguous shards, one per
// entry of devices[] (repeats allowed: two shards on one GPU), each shard on its own thread with
// its own non-blocking stream on its device — H2D of its slice, the single-device solve, D2H into
// the caller's arrays at the shard's offset.  Every trajectory is solved exactly as by the
// single-device call (one wave / lane / workgroup per trajectory, no cross-trajectory
// arithmetic), so the outputs are bit-identical whenever the shards select the same kernel as
// the whole batch (the n ≤ 4 quad/lane choice depends on the batch, see dp_lane.hip use_quad).
namespace {
struct Shard {
    int64_t b0 = 0, nb = 0;
    int dev = 0;
    int st = 0;
    std::string err;
};

// shard boundaries: contiguous, the first (B mod ndev) shards one trajectory longer
std::vector<Shard> make_shards(int64_t B, const int32_t *devices, int32_t ndev)
{
    std::vector<Shard> sh((size_t)ndev);
    const int64_t q = B / ndev, r = B % ndev;
    int64_t b0 = 0;
    for (int i = 0; i < ndev; ++i) {
        sh[i].b0 = b0;
        sh[i].nb = q + (i < r ? 1 : 0);
        sh[i].dev = devices[i];
        b0 += sh[i].nb;
    }
    return sh;
}

// devices / ndev of a _host_devices entry: the arguments themselves (no device call) …
int check_devices_args(const int32_t *devices, int32_t ndev, int ai_dev, int ai_ndev)
{
    if (ndev < 1) return set_err(-ai_ndev, "ndev must be >= 1 (got %d)", ndev);
    if (!devices) return set_err(-ai_dev, "devices is NULL");
    return 0;
}
// … and every ordinal against hipGetDeviceCount
int check_device_ordinals(const int32_t *devices, int32_t ndev, int ai_dev)
{
    int cnt = 0;
    const hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess) return set_err(LQRX_ERR_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    for (int i = 0; i < ndev; ++i)
        if (devices[i] < 0 || devices[i] >= cnt)
            return set_err(-ai_dev, "devices[%d] = %d is not a device (0..%d)", i, devices[i], cnt - 1);
    return 0;
}
int check_devices(const int32_t *devices, int32_t ndev, int ai_dev, int ai_ndev)
{
    const int st = check_devices_args(devices, ndev, ai_dev, ai_ndev);
    return st ? st : check_device_ordinals(devices, ndev, ai_dev);
}

// one host array of S elements per trajectory: the shard's slice ↔ a packed device buffer of
// nb trajectories in the same layout (layout 0: one contiguous run; layout 1: S rows of nb
// elements at pitch B)
hipError_t shard_h2d(void *dst, const void *src, size_t S, size_t es, const Shard &sh, int64_t B, int layout,
                     hipStream_t s)
{
    if (layout == 0)
        return hipMemcpyAsync(dst, (const char *)src + (size_t)sh.b0 * S * es, (size_t)sh.nb * S * es,
                              hipMemcpyHostToDevice, s);
    return hipMemcpy2DAsync(dst, (size_t)sh.nb * es, (const char *)src + (size_t)sh.b0 * es, (size_t)B * es,
                            (size_t)sh.nb * es, S, hipMemcpyHostToDevice, s);
}
hipError_t shard_d2h(void *dst, const void *src, size_t S, size_t es, const Shard &sh, int64_t B, int layout,
                     hipStream_t s)
{
    if (layout == 0)
        return hipMemcpyAsync((char *)dst + (size_t)sh.b0 * S * es, src, (size_t)sh.nb * S * es,
                              hipMemcpyDeviceToHost, s);
    return hipMemcpy2DAsync((char *)dst + (size_t)sh.b0 * es, (size_t)B * es, src, (size_t)sh.nb * es,
                            (size_t)sh.nb * es, S, hipMemcpyDeviceToHost, s);
}

// a shard's device buffers and stream, released on its own device
struct ShardCtx {
    hipStream_t s = nullptr;
    std::vector<void *> bufs;
    ~ShardCtx()
    {
        if (s) (void)hipStreamSynchronize(s);
        for (void *p : bufs) (void)hipFree(p);
        if (s) (void)hipStreamDestroy(s);
    }
    int alloc(void **p, size_t bytes)
    {
        hipError_t e = hipMalloc(p, bytes ? bytes : 16);
        if (e != hipSuccess) return hip_err(e, "hipMalloc shard");
        bufs.push_back(*p);
        return 0;
    }
};

// run fn(shard) for every non-empty shard concurrently, each on its device; the first failing
// shard's status and message become the call's; else 1 if any trajectory has info != 0
template <typename F> int run_shards(std::vector<Shard> &sh, const int32_t *info, int64_t B, F fn)
{
    std::vector<std::thread> th;
    for (auto &x : sh) {
        if (x.nb == 0) continue;
        th.emplace_back([&x, &fn] {
            hipError_t e = hipSetDevice(x.dev);
            x.st = e != hipSuccess ? hip_err(e, "hipSetDevice") : fn(x);
            if (x.st < 0) x.err = g_err;
        });
    }
    for (auto &t : th) t.join();
    for (auto &x : sh)
        if (x.st < 0) return set_err(x.st, "shard on device %d (trajectories %lld..%lld): %s", x.dev,
                                     (long long)x.b0, (long long)(x.b0 + x.nb - 1), x.err.c_str());
    if (info)
        for (int64_t b = 0; b < B; ++b)
            if (info[b]) return 1;
    return 0;
}

// The _host_devices entries (plain and linear): descriptor; devices and ndev, the two arguments
// behind info; pointers (a non-empty batch); the ordinals, the first device call; batch == 0 is a
// no-op.  Each shard stages its slice of every buffer of the table on its own device and stream.
int dp_solve_host_devices_impl(const lqrx_dp_desc *d, DpKind kind, const DpPtrs &p, const int32_t *devices,
                               int32_t ndev)
{
    int st = validate_dp(d);
    if (st) return st;
    const DpTable t(d, kind, p);
    if ((st = check_devices_args(devices, ndev, t.narg + 2, t.narg + 3))) return st;
    if (d->batch && (st = t.check())) return st;
    if ((st = check_device_ordinals(devices, ndev, t.narg + 2))) return st;
    if (d->batch == 0) return 0;
    const size_t es = dsize(d->dtype);
    std::vector<Shard> sh = make_shards(d->batch, devices, ndev);
    const int64_t Bt = d->batch;
    const int lay = d->layout;
    return run_shards(sh, p.info, Bt, [&](Shard &x) -> int {
        ShardCtx c;
        hipError_t e = hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking);
        if (e != hipSuccess) return hip_err(e, "hipStreamCreate");
        DpTable td = t;
        void *dinfo = nullptr;
        int r;
        for (int i = 0; i < t.nrows; ++i) {
            const DpRow &h = t.row[i];
            if ((r = c.alloc(&td.row[i].ptr, (size_t)h.elems * es * x.nb))) return r;
            if (!h.out && (e = shard_h2d(td.row[i].ptr, h.ptr, h.elems, es, x, Bt, lay, c.s)) != hipSuccess)
                return hip_err(e, "H2D");
        }
        if ((r = c.alloc(&dinfo, 4 * x.nb))) return r;
        lqrx_dp_desc ds = *d;
        ds.batch = x.nb;
        if ((r = dp_run(&ds, td, (int32_t *)dinfo, c.s)) < 0) return r;
        for (int i = 0; i < t.nrows; ++i)
            if (t.row[i].out && (e = shard_d2h(t.row[i].ptr, td.row[i].ptr, t.row[i].elems, es, x, Bt, lay, c.s)) != hipSuccess)
                return hip_err(e, "D2H");
        if (p.info && (e = hipMemcpyAsync(p.info + x.b0, dinfo, 4 * x.nb, hipMemcpyDeviceToHost, c.s)) != hipSuccess)
            return hip_err(e, "D2H info");
        if ((e = hipStreamSynchronize(c.s)) != hipSuccess) return hip_err(e, "dp shard");
        return 0;
    });
}
} // namespace

extern "C" int lqrx_dp_solve_host_devices(const lqrx_dp_desc *d, const void *A, const void *B, const void *Q,
                                          const void *R, const void *Qf, const void *x0, void *K, void *P, void *X,
                                          void *U, int32_t *info, const int32_t *devices, int32_t ndev)
{
    return dp_solve_host_devices_impl(d, DP_PLAIN, DpPtrs{A, B, nullptr, Q, R, nullptr, Qf, x0, nullptr, nullptr, K, P, X, U, info},
                                      devices, ndev);
}

extern "C" int lqrx_dp_solve_linear_host_devices(const lqrx_dp_desc *d, const void *A, const void *B,
                                                 const void *Q, const void *R, const void *Qf, const void *x0,
                                                 const lqrx_dp_linear *lin, void *K, void *P, void *X, void *U,
                                                 int32_t *info, const int32_t *devices, int32_t ndev)
{
    return dp_solve_host_devices_impl(d, DP_LINEAR, DpPtrs{A, B, nullptr, Q, R, nullptr, Qf, x0, lin, nullptr, K, P, X, U, info},
                                      devices, ndev);
}

extern "C" int lqrx_kkt_solve_host_devices(const lqrx_kkt_desc *d, const void *Y, const void *y, const void *H,
                                           const void *g, void *dz, void *lam, int32_t *info,
                                           const int32_t *devices, int32_t ndev)
{
    KktLayout L;
    int st = kkt_layout(d, L);
    if (st) return st;
    if ((st = check_devices(devices, ndev, 9, 10))) return st;
    if (d->batch == 0) return 0;
    const void *hin[4] = {Y, y, H, g};
    for (int i = 0; i < 4; ++i)
        if (!hin[i]) return set_err(-(i + 2), "input pointer %d is NULL", i + 2);
    if (!dz) return set_err(-6, "dz is NULL");
    if (!lam) return set_err(-7, "lam is NULL");
    const size_t es = d->dtype == LQRX_F32 ? 4 : 8;
    const size_t szin[4] = {(size_t)L.sY, (size_t)L.sy, (size_t)L.sH, (size_t)L.sg};
    std::vector<Shard> sh = make_shards(d->batch, devices, ndev);
    const int64_t Bt = d->batch;
    const int lay = d->layout;
    return run_shards(sh, info, Bt, [&](Shard &x) -> int {
        ShardCtx c;
        hipError_t e = hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking);
        if (e != hipSuccess) return hip_err(e, "hipStreamCreate");
        void *din[4] = {}, *ddz = nullptr, *dlam = nullptr, *dinfo = nullptr;
        int r;
        for (int i = 0; i < 4; ++i) {
            if ((r = c.alloc(&din[i], szin[i] * es * x.nb))) return r;
            if ((e = shard_h2d(din[i], hin[i], szin[i], es, x, Bt, lay, c.s)) != hipSuccess) return hip_err(e, "H2D");
        }
        if ((r = c.alloc(&ddz, (size_t)L.sg * es * x.nb)) || (r = c.alloc(&dlam, (size_t)L.sy * es * x.nb)) ||
            (r = c.alloc(&dinfo, 4 * x.nb)))
            return r;
        lqrx_kkt_desc ds = *d;
        ds.batch = x.nb;
        if ((r = kkt_solve_impl(&ds, din[0], din[1], din[2], din[3], ddz, dlam, (int32_t *)dinfo, nullptr, 0, c.s)) < 0)
            return r;
        if ((e = shard_d2h(dz, ddz, (size_t)L.sg, es, x, Bt, lay, c.s)) != hipSuccess ||
            (e = shard_d2h(lam, dlam, (size_t)L.sy, es, x, Bt, lay, c.s)) != hipSuccess)
            return hip_err(e, "D2H");
        if (info && (e = hipMemcpyAsync(info + x.b0, dinfo, 4 * x.nb, hipMemcpyDeviceToHost, c.s)) != hipSuccess)
            return hip_err(e, "D2H info");
        if ((e = hipStreamSynchronize(c.s)) != hipSuccess) return hip_err(e, "kkt shard");
        return 0;
    });
}

// ------------------------------------------------------------------ batched trajectory SQP
namespace {
int validate_sqp(const lqrx_sqp_desc *d, int *nx, int *nu)
{
    if (!d) return set_err(-1, "desc is NULL");
    if (!lqrx::sqp_model_dims(d->model, nx, nu)) return set_err(-1, "desc.model %d is not a known model", d->model);
    if (d->N < 2) return set_err(-1, "desc.N must be >= 2 (got %d)", d->N);
    if (d->batch < 0) return set_err(-1, "desc.batch must be >= 0");
    if (d->max_iters < 0) return set_err(-1, "desc.max_iters must be >= 0");
    if (d->stage_rows < 0 || d->stage_rows > 2 || d->stage_rows * *nx > 32)
        return set_err(-1, "desc.stage_rows must be 0..2 with stage_rows·nx <= 32 (got %d)", d->stage_rows);
    for (int i = 0; i < d->stage_rows * *nx; ++i)
        if (!std::isfinite(d->stage_A[i])) return set_err(-1, "desc.stage_A must be finite");
    for (int i = 0; i < d->stage_rows; ++i)
        if (!std::isfinite(d->stage_b[i])) return set_err(-1, "desc.stage_b must be finite");
    if (!(d->dt > 0)) return set_err(-1, "desc.dt must be > 0");
    for (int i = 0; i < *nx; ++i)
        if (!(d->Q[i] > 0) || !(d->Qf[i] > 0)) return set_err(-1, "desc.Q / desc.Qf must be positive");
    for (int i = 0; i < *nu; ++i)
        if (!(d->R[i] > 0)) return set_err(-1, "desc.R must be positive");
    if (d->model == LQRX_MODEL_CARTPOLE)
        for (int i = 0; i < 4; ++i)
            if (!(d->params[i] > 0) || !std::isfinite(d->params[i]))
                return set_err(-1, "desc.params (mc, mp, l, g) must be positive and finite");
    if (!(d->mu >= 0) || !(d->tol_p >= 0) || !(d->tol_d >= 0))
        return set_err(-1, "desc.mu / tol_p / tol_d must be >= 0");
    // more constraint rows than variables: the Newton KKT matrix is singular at every point
    const int64_t nvar = (int64_t)d->N * *nx + (int64_t)(d->N - 1) * *nu,
                  ncon = (int64_t)(d->N + 1) * *nx + (int64_t)(d->N - 2) * d->stage_rows;
    if (nvar < ncon)
        return set_err(-1, "over-constrained: %lld variables (N*nx + (N-1)*nu) < %lld constraint rows "
                           "(nx*(N+1) + stage_rows*(N-2))", (long long)nvar, (long long)ncon);
    return 0;
}

lqrx_sqp_desc from_dubins(const lqrx_dubins_sqp_desc *d)
{
    lqrx_sqp_desc q{};
    q.model = LQRX_MODEL_DUBINS;
    q.N = d->N; q.max_iters = d->max_iters; q.batch = d->batch; q.dt = d->dt;
    for (int i = 0; i < 3; ++i) q.Q[i] = d->Q[i], q.Qf[i] = d->Qf[i];
    for (int i = 0; i < 2; ++i) q.R[i] = d->R[i];
    q.mu = d->mu; q.tol_p = d->tol_p; q.tol_d = d->tol_d;
    return q;
}

struct SqpKkt {
    lqrx_kkt_desc kd;
    std::vector<int32_t> n1, p, n2, w;
    const double *Y, *y, *H, *g;
    double *lamn, *lams;
    int32_t *info;
    void *ws;
    size_t ws_bytes;
    hipStream_t s;
};

int sqp_kkt(void *ctx, int ginv, double *dz, const int32_t *sel, const int32_t *nsel)
{
    SqpKkt &c = *(SqpKkt *)ctx;
    c.kd.ginv = ginv;
    return kkt_solve_impl(&c.kd, c.Y, c.y, c.H, c.g, dz, ginv ? c.lamn : c.lams, c.info, c.ws, c.ws_bytes, c.s,
                          /*null_sync=*/false, sel, nsel);
}
} // namespace

extern "C" int lqrx_sqp_model_dims(int32_t model, int32_t *nx, int32_t *nu)
{
    int a = 0, b = 0;
    if (!lqrx::sqp_model_dims(model, &a, &b)) return set_err(-1, "model %d is not a known model", model);
    if (nx) *nx = a;
    if (nu) *nu = b;
    return 0;
}

extern "C" int lqrx_sqp_solve(const lqrx_sqp_desc *d, double *Z, const double *x0, const double *xf, double *lam,
                              int32_t *iters, int32_t *status, void *stream)
{
    int nx = 0, nu = 0;
    int st = validate_sqp(d, &nx, &nu);
    if (st) return st;
    if (d->batch == 0) return 0;
    if (!Z) return set_err(-2, "Z is NULL");
    if (!x0) return set_err(-3, "x0 is NULL");
    if (!xf) return set_err(-4, "xf is NULL");
    if (!lam) return set_err(-5, "lam is NULL");
    if (!iters) return set_err(-6, "iters is NULL");
    if (!status) return set_err(-7, "status is NULL");
    const int N = d->N;
    const int pk = d->stage_rows;
    const int64_t B = d->batch, NN = (int64_t)N * nx + (int64_t)(N - 1) * nu,
                  P = (int64_t)(N + 1) * nx + (int64_t)(N - 2) * pk;
    hipStream_t s = (hipStream_t)stream;
    SqpKkt c{};
    lqrx::sqp_structure(nx, nu, pk, N, c.n1, c.p, c.n2, c.w);
    c.kd.N = N; c.kd.dtype = LQRX_F64; c.kd.batch = B;
    c.kd.n1 = c.n1.data(); c.kd.p = c.p.data(); c.kd.n2 = c.n2.data(); c.kd.w = c.w.data();
    c.kd.h_mode = 2; c.kd.ginv = 1; c.kd.layout = 0;
    int64_t sY = 0, sy = 0, sH = 0, sg = 0;
    if ((st = lqrx_kkt_sizes(&c.kd, &sY, &sy, &sH, &sg, nullptr))) return st;
    size_t ws1 = 0, ws0 = 0;
    if ((st = lqrx_kkt_workspace_size(&c.kd, &ws1))) return st;
    c.kd.ginv = 0;
    if ((st = lqrx_kkt_workspace_size(&c.kd, &ws0))) return st;
    // one stream-ordered block, carved (256-B aligned pieces)
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t oY = take(B * sY * 8), oy = take(B * sy * 8), oH = take(B * sH * 8), og = take(B * sg * 8),
                 odz = take(B * NN * 8), olamn = take(B * P * 8), odzs = take(B * NN * 8), olams = take(B * P * 8),
                 ophi = take(B * 8), odphi = take(B * 8), osoc = take(B * 4),
                 oact = take(4), oinfo = take(B * 4), ows = take(std::max(ws0, ws1)),
                 osel = take(B * 4), onsel = take(4);
    void *blk = nullptr;
    hipError_t e = lqrx::scratch_alloc(&blk, off, s);
    if (e != hipSuccess) return hip_err(e, "sqp scratch");
    char *b = (char *)blk;
    lqrx::SqpArgs A{};
    A.model = d->model; A.N = N; A.B = B; A.dt = d->dt; A.mu = d->mu; A.tol_p = d->tol_p; A.tol_d = d->tol_d;
    for (int i = 0; i < 8; ++i) A.Q[i] = d->Q[i], A.Qf[i] = d->Qf[i], A.R[i] = d->R[i];
    for (int i = 0; i < 4; ++i) A.par[i] = d->params[i];
    A.stage_rows = pk;
    for (int i = 0; i < 32; ++i) A.SA[i] = d->stage_A[i];
    for (int i = 0; i < 4; ++i) A.Sb[i] = d->stage_b[i];
    A.x0 = x0; A.xf = xf; A.Z = Z; A.lam = lam; A.iters = iters; A.status = status;
    A.Y = (double *)(b + oY); A.y = (double *)(b + oy); A.H = (double *)(b + oH); A.g = (double *)(b + og);
    A.dz = (double *)(b + odz); A.lamn = (double *)(b + olamn); A.dzs = (double *)(b + odzs);
    A.phi0 = (double *)(b + ophi); A.dphi = (double *)(b + odphi);
    A.need_soc = (int32_t *)(b + osoc); A.n_active = (int32_t *)(b + oact);
    A.sel = (int32_t *)(b + osel); A.nsel = (int32_t *)(b + onsel);
    c.Y = A.Y; c.y = A.y; c.H = A.H; c.g = A.g; c.lamn = A.lamn; c.lams = (double *)(b + olams);
    c.info = (int32_t *)(b + oinfo); c.ws = b + ows; c.ws_bytes = std::max(ws0, ws1); c.s = s;
    int kkt_rc = 0;
    e = lqrx::sqp_run(A, d->max_iters, s, sqp_kkt, &c, &kkt_rc);
    hipError_t ef = lqrx::scratch_free(blk, s);
    if (kkt_rc < 0) return kkt_rc;
    if (e != hipSuccess) return hip_err(e, "sqp");
    if (ef != hipSuccess) return hip_err(ef, "sqp scratch free");
    if (stream == nullptr && (e = hipStreamSynchronize(nullptr)) != hipSuccess) return hip_err(e, "sqp");
    return 0;
}

extern "C" int lqrx_sqp_solve_host(const lqrx_sqp_desc *d, double *Z, const double *x0, const double *xf,
                                   double *lam, int32_t *iters, int32_t *status)
{
    int nx = 0, nu = 0;
    int st = validate_sqp(d, &nx, &nu);
    if (st) return st;
    if (d->batch == 0) return 0;
    if (!Z || !x0 || !xf || !lam || !iters || !status) return set_err(-2, "NULL host pointer");
    const int64_t B = d->batch, NN = (int64_t)d->N * nx + (int64_t)(d->N - 1) * nu,
                  P = (int64_t)(d->N + 1) * nx + (int64_t)(d->N - 2) * d->stage_rows;
    DevBuf dZ, dx0, dxf, dlam, dit, dst;
    if ((st = dev_alloc(dZ, B * NN * 8, "Z")) || (st = dev_alloc(dx0, B * nx * 8, "x0")) ||
        (st = dev_alloc(dxf, B * nx * 8, "xf")) || (st = dev_alloc(dlam, B * P * 8, "lam")) ||
        (st = dev_alloc(dit, B * 4, "iters")) || (st = dev_alloc(dst, B * 4, "status")))
        return st;
    hipError_t e;
    if ((e = hipMemcpy(dZ.p, Z, B * NN * 8, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(dx0.p, x0, B * nx * 8, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(dxf.p, xf, B * nx * 8, hipMemcpyHostToDevice)) != hipSuccess)
        return hip_err(e, "sqp H2D");
    if ((st = lqrx_sqp_solve(d, (double *)dZ.p, (const double *)dx0.p, (const double *)dxf.p, (double *)dlam.p,
                             (int32_t *)dit.p, (int32_t *)dst.p, nullptr)))
        return st;
    if ((e = hipMemcpy(Z, dZ.p, B * NN * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(lam, dlam.p, B * P * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(iters, dit.p, B * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(status, dst.p, B * 4, hipMemcpyDeviceToHost)) != hipSuccess)
        return hip_err(e, "sqp D2H");
    return 0;
}

extern "C" int lqrx_dubins_sqp_solve(const lqrx_dubins_sqp_desc *d, double *Z, const double *x0, const double *xf,
                                     double *lam, int32_t *iters, int32_t *status, void *stream)
{
    if (!d) return set_err(-1, "desc is NULL");
    const lqrx_sqp_desc q = from_dubins(d);
    return lqrx_sqp_solve(&q, Z, x0, xf, lam, iters, status, stream);
}

extern "C" int lqrx_dubins_sqp_solve_host(const lqrx_dubins_sqp_desc *d, double *Z, const double *x0,
                                          const double *xf, double *lam, int32_t *iters, int32_t *status)
{
    if (!d) return set_err(-1, "desc is NULL");
    const lqrx_sqp_desc q = from_dubins(d);
    return lqrx_sqp_solve_host(&q, Z, x0, xf, lam, iters, status);
}


// ------------------------------------------------------------------ condensed least squares
namespace {
constexpr size_t LS_LDS_MAX = 163840;

int validate_ls(const lqrx_ls_desc *d)
{
    if (!d) return set_err(-1, "desc is NULL");
    if (d->n < 1 || d->m < 1) return set_err(-1, "desc.n, desc.m must be >= 1 (got %d, %d)", d->n, d->m);
    if (d->N < 2) return set_err(-1, "desc.N must be >= 2 (got %d)", d->N);
    if (d->hu_mode < 0 || d->hu_mode > 2) return set_err(-1, "desc.hu_mode must be 0, 1 or 2");
    if (d->batch < 0 || d->batch > 0x7fffffff) return set_err(-1, "desc.batch must be in [0, 2^31)");
    if ((int64_t)(d->N - 1) * d->m > lqrx::ls_max_nm())
        return set_err(LQRX_ERR_UNSUPPORTED, "(N-1)*m = %lld > %d", (long long)(d->N - 1) * d->m, lqrx::ls_max_nm());
    const size_t lds = lqrx::ls_lds_bytes(d->n, d->m, d->N);
    if (lds > LS_LDS_MAX)
        return set_err(LQRX_ERR_UNSUPPORTED, "n=%d m=%d N=%d needs %zu B of LDS (> %zu)", d->n, d->m, d->N, lds,
                       LS_LDS_MAX);
    return 0;
}
} // namespace

extern "C" size_t lqrx_ls_lds_bytes(int32_t n, int32_t m, int32_t N)
{
    if (n < 1 || m < 1 || N < 2) return 0;
    return lqrx::ls_lds_bytes(n, m, N);
}

extern "C" int lqrx_ls_solve(const lqrx_ls_desc *d, const double *A, const double *B, const double *Q,
                             const double *R, const double *Qf, const double *x0, double *U, double *X,
                             int32_t *info, double *Abar, double *bbar, void *stream)
{
    int st = validate_ls(d);
    if (st) return st;
    if (d->batch == 0) return 0;
    const double *in[6] = {A, B, Q, R, Qf, x0};
    for (int i = 0; i < 6; ++i)
        if (!in[i]) return set_err(-(i + 2), "input pointer %d is NULL", i + 2);
    if (!U) return set_err(-8, "U is NULL");
    if (!X) return set_err(-9, "X is NULL");
    lqrx::LsArgs a{};
    a.A = A; a.B = B; a.Q = Q; a.R = R; a.Qf = Qf; a.x0 = x0;
    a.U = U; a.X = X; a.info = info; a.Ab = Abar; a.bb = bbar;
    a.n = d->n; a.m = d->m; a.N = d->N; a.hu_mode = d->hu_mode; a.batch = d->batch;
    hipError_t e = lqrx::ls_launch(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_err(e, "ls kernel launch");
    if (stream == nullptr) {
        if ((e = hipStreamSynchronize(nullptr)) != hipSuccess) return hip_err(e, "ls kernel");
        if (info) {
            std::vector<int32_t> h((size_t)d->batch);
            if ((e = hipMemcpy(h.data(), info, h.size() * 4, hipMemcpyDeviceToHost)) != hipSuccess)
                return hip_err(e, "info D2H");
            for (int32_t v : h)
                if (v) return 1;
        }
    }
    return 0;
}

extern "C" int lqrx_ls_solve_host(const lqrx_ls_desc *d, const double *A, const double *B, const double *Q,
                                  const double *R, const double *Qf, const double *x0, double *U, double *X,
                                  int32_t *info)
{
    int st = validate_ls(d);
    if (st) return st;
    if (d->batch == 0) return 0;
    const size_t bt = (size_t)d->batch, n = d->n, m = d->m, N = d->N;
    const size_t szin[6] = {n * n, n * m, n * n, m * m, n * n, n};
    const double *hin[6] = {A, B, Q, R, Qf, x0};
    DevBuf din[6], dU, dX, dinfo;
    for (int i = 0; i < 6; ++i) {
        if (!hin[i]) return set_err(-(i + 2), "input pointer %d is NULL", i + 2);
        if ((st = dev_alloc(din[i], szin[i] * 8 * bt, "hipMalloc input"))) return st;
        hipError_t e = hipMemcpy(din[i].p, hin[i], szin[i] * 8 * bt, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_err(e, "H2D");
    }
    if (!U) return set_err(-8, "U is NULL");
    if (!X) return set_err(-9, "X is NULL");
    if ((st = dev_alloc(dU, (N - 1) * m * 8 * bt, "hipMalloc U"))) return st;
    if ((st = dev_alloc(dX, N * n * 8 * bt, "hipMalloc X"))) return st;
    if ((st = dev_alloc(dinfo, 4 * bt, "hipMalloc info"))) return st;
    st = lqrx_ls_solve(d, (const double *)din[0].p, (const double *)din[1].p, (const double *)din[2].p,
                       (const double *)din[3].p, (const double *)din[4].p, (const double *)din[5].p,
                       (double *)dU.p, (double *)dX.p, (int32_t *)dinfo.p, nullptr, nullptr, nullptr);
    if (st < 0) return st;
    hipError_t e;
    if ((e = hipMemcpy(U, dU.p, (N - 1) * m * 8 * bt, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(X, dX.p, N * n * 8 * bt, hipMemcpyDeviceToHost)) != hipSuccess)
        return hip_err(e, "D2H");
    if (info && (e = hipMemcpy(info, dinfo.p, 4 * bt, hipMemcpyDeviceToHost)) != hipSuccess)
        return hip_err(e, "D2H info");
    return st;
}
