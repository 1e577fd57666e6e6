// wg_capi.hip -- C ABI (include/wg_mpc.h) over the HIP kernels: host code only (the kernels are in the headers).  gfx950 only.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/wg_mpc.h"
#include "wg_ql_device.hpp"
#include "wg_tick_device.hpp"
#include "wg_tick_kernels.hpp"
#include "wg_pldp_device.hpp"
#include "wg_dimitrov_device.hpp"
#include "wg_preview_device.hpp"
#include "wg_gramian_device.hpp"
#include "wg_zmpdisc_device.hpp"
#include "wg_footcons_device.hpp"
#include "wg_audit_device.hpp"
#include "wg_ql_kernels.hpp"
#include "wg_pldp_kernels.hpp"
#include "wg_dimitrov_kernels.hpp"
#include "wg_steps_kernels.hpp"
#include "wg_riccati_kernels.hpp"
#include "wg_morisawa_kernels.hpp"


namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                            \
  do {                                                                           \
    hipError_t e_ = (expr);                                                      \
    if (e_ != hipSuccess) return fail(WG_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// grow-only device buffer.  Growing never frees: a launch enqueued earlier may still be using the old allocation (and
// hipFree would make the host wait for the whole device), so the old one is retired and freed with the context.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  std::vector<void *> retired;
  int reserve(size_t bytes) {
    if (bytes <= cap) return WG_OK;
    if (p && bytes < cap + cap / 2) bytes = cap + cap / 2;   // grow geometrically: what is retired stays below twice what is live
    void *fresh = nullptr;
    hipError_t e = hipMalloc(&fresh, bytes);
    if (e != hipSuccess) return fail(WG_ERR_HIP, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    if (p) retired.push_back(p);
    p = fresh; cap = bytes;
    return WG_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    for (void *r : retired) (void)hipFree(r);
    retired.clear();
    p = nullptr; cap = 0;
  }
};


// environment knobs: read on EVERY call (tests flip them inside one process)
inline int env_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
inline bool env_flag(const char *name, bool dflt) { return env_int(name, dflt) != 0; }

// Residency.  LDS is handed out in granules of 1280 B, 128 to a CU: how many workgroups of `lds` bytes a CU keeps, at most the
// `wave_cap` waves the kernel's register budget admits, at least one (whatever passed the 160 KiB checks fits once)
inline size_t per_cu_granules(size_t lds, size_t wave_cap) {
  const size_t g = (lds + 1279) / 1280, k = g ? 128 / g : wave_cap;
  return k > wave_cap ? wave_cap : (k < 1 ? 1 : k);
}
// the same by whole bytes of the CU's 160 KiB (where an operand is placed: the dense boundary, PLDP)
inline size_t per_cu_160k(size_t lds, size_t cap) { const size_t k = (160 * 1024) / (lds ? lds : 1); return k > cap ? cap : k; }

// longest-solve-first start order of one kind of launch: [iterations of the last batch (B) | start order (B)], and the batch
// (array and size) those iterations belong to
struct Lpt {
  DevBuf buf;
  const void *key = nullptr;
  int B = 0;
  void release() { buf.release(); key = nullptr; B = 0; }
};

}  // namespace

// Everything the library keeps between calls: configured models (device copies of their tables), the workspaces its
// kernels need besides the caller's arrays, and the staging buffers of the host-pointer entry points.  The entry points
// without a context argument work on one process-wide default context.
struct wg_ctx {
  int device = 0;
  int num_cu = 256;
  std::mutex mu;
  // held from the ordering test of a launch that uses per-context device state (queue, solver slots, scratch states) through the
  // launch itself and the event record behind it: two host threads cannot both pass the test.  Lock order: mu -> launch_mu
  std::mutex launch_mu;
  // Herdt-2010 tick
  wg_model_t model;
  bool model_set = false;
  wg::TickTables *tables_dev = nullptr;
  wg_model_t *model_dev = nullptr;     // the model in device memory (the multi-tick kernels read it through a pointer)
  DevBuf tick_state, tick_out, tick_aux, run_buf, tick_z, asm_state;
  // one launch per tick: the gaits are started longest-solve-first, by the iteration counts of their previous tick
  // dense ql0001_ boundary: wa | b of every QP in a slot of global memory when that buys the eighth QP per CU; one launch at a
  // time uses the slots (a launch that arrives on another stream while one is pending keeps wa | b in LDS instead)
  DevBuf qp_slot;
  struct SlotOrder { hipEvent_t ev = nullptr; hipStream_t stream = nullptr; bool armed = false; };
  SlotOrder qp_order;
  // the tick, the dense QP boundary and the Dimitrov tick's QL back-ends: a batch that follows another one of the same size on
  // the same arrays (an MPC loop: problem k of consecutive calls is the same robot a tick later) starts longest-solve-first
  Lpt tick_lpt, qp_lpt, dim_lpt;
  // The tick / run kernels keep their queue and per-block solver slots in run_buf / tick_z: launches of one context must
  // not overlap ON THE DEVICE.  Every such launch leaves an event behind; a launch that arrives on ANOTHER stream while that
  // event is still pending is made to wait for it (hipStreamWaitEvent: ordered, not refused -- a double-buffered pipeline that
  // orders its streams with events of its own is enqueued ahead of time and must be accepted).  WG_OVERLAP_STRICT=1 refuses such a
  // launch instead (WG_ERR_BUSY, nothing launched): a way to find serialisation one did not intend.
  SlotOrder guard_order;
  // wg_mpc_assemble_batch_dev runs the tick on scratch copies of the states kept per context (asm_state): same ordering
  SlotOrder asm_order;
  // launches of the other back-ends (PLDP, Dimitrov tick, preview): they read constants a re-configuration overwrites, so they
  // leave an event for it to wait on (marked, never claimed: they keep nothing per launch in the context)
  SlotOrder aux_order;
  // The host-pointer entry points stage, launch and copy back on THIS stream (non-blocking: no implicit ordering against the
  // legacy stream or anybody else's) and wait for it alone -- never for the device: another context's launches, or a caller's
  // own streams, keep running while this context's host call waits for its own work.
  hipStream_t host_stream = nullptr;
  bool overlap_strict = false;           // WG_OVERLAP_STRICT at wg_ctx_create / wg_init, wg_set_overlap_strict afterwards
  long long serialised = 0;              // launches that were ordered behind one of another stream (wg_overlap_serialised)
  // one-robot path (wg_mpc_tick_pinned): its own stream, a completion counter in host-mapped memory
  hipStream_t pin_stream = nullptr;
  int *pin_flag = nullptr;               // host-mapped; the kernel adds 1 per gait when its outputs are visible
  int pin_seq = 0;
  // PLDP / Dimitrov
  wg::PldpModel *pldp_dev = nullptr;
  int pldp_N = 0;
  DevBuf pldp_buf;
  wg::DimitrovConst *dim_dev = nullptr;
  std::unique_ptr<wg::DimitrovConst> dim_host;
  bool dim_set = false;
  DevBuf dim_buf;
  // Dimitrov fleets on the device: the per-chunk counts of wg_foot_constraints_batch_dev / _append_dev (the latter keeps each
  // gait's done and count as they were on entry behind them), and the B x N polytopes
  // wg_dimitrov_walk_dev / _follow_dev select for the tick they launch next (follow: and the row each gait's tick writes, behind
  // them).  One launch at a time uses each: claimed and marked like the tick's buffers (fc_order, walk_order)
  DevBuf fc_buf, walk_polys;
  SlotOrder fc_order, walk_order;
  // the walk audit: one wg_zmp_audit_t per (chunk, gait) between the two kernels of wg_zmp_audit_dev / _append_dev; one launch at
  // a time uses it, claimed and marked (audit_order)
  DevBuf audit_buf;
  SlotOrder audit_order;
  // preview control
  wg::PreviewConst prev;
  double *prev_F = nullptr;            // device copy of the window gains
  bool prev_set = false;
  DevBuf prev_buf;
  // staging of the host-pointer entry points
  DevBuf in, out, gram_buf, zd_buf;
  // Morisawa walks: the sampler's clock of the launch (wg_morisawa_clock_kernel); one launch at a time uses it, claimed and marked
  DevBuf mo_clock;
  SlotOrder mo_order;
  void release_all() {
    if (tables_dev) (void)hipFree(tables_dev);
    if (model_dev) (void)hipFree(model_dev);
    if (pldp_dev) (void)hipFree(pldp_dev);
    if (dim_dev) (void)hipFree(dim_dev);
    if (prev_F) (void)hipFree(prev_F);
    tables_dev = nullptr; model_dev = nullptr; pldp_dev = nullptr; dim_dev = nullptr; prev_F = nullptr;
    model_set = false; pldp_N = 0; dim_set = false; prev_set = false;
    for (DevBuf *b : {&tick_state, &tick_out, &tick_aux, &run_buf, &tick_z, &asm_state, &qp_slot, &pldp_buf, &dim_buf, &fc_buf, &walk_polys, &prev_buf, &in, &out, &gram_buf, &zd_buf, &mo_clock, &audit_buf})
      b->release();
    for (Lpt *l : {&tick_lpt, &qp_lpt, &dim_lpt}) l->release();
    for (SlotOrder *o : {&guard_order, &qp_order, &asm_order, &aux_order, &fc_order, &walk_order, &mo_order, &audit_order}) {
      if (o->ev) (void)hipEventDestroy(o->ev);
      o->ev = nullptr; o->armed = false; o->stream = nullptr;
    }
    if (pin_stream) (void)hipStreamDestroy(pin_stream);
    if (host_stream) (void)hipStreamDestroy(host_stream);
    host_stream = nullptr;
    if (pin_flag) (void)hipHostFree(pin_flag);
    pin_stream = nullptr; pin_flag = nullptr; pin_seq = 0;
  }
};
namespace {

std::mutex g_default_mu;
wg_ctx *g_default = nullptr;          // created by wg_init() or by the first call that needs it

int make_ctx(int device_ordinal, wg_ctx **out) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(WG_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU path",
                e == hipSuccess ? "count = 0" : hipGetErrorString(e));
  if (device_ordinal < 0 || device_ordinal >= count)
    return fail(WG_ERR_BAD_ARG, "device ordinal %d out of range [0,%d)", device_ordinal, count);
  HIP_TRY(hipSetDevice(device_ordinal));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device_ordinal));
  wg_ctx *c = new wg_ctx();
  c->device = device_ordinal;
  c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (hipStreamCreateWithFlags(&c->host_stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return fail(WG_ERR_HIP, "hipStreamCreateWithFlags failed for the context's host stream");
  }
  c->overlap_strict = env_flag("WG_OVERLAP_STRICT", false);   // read once per context, not per launch
  *out = c;
  return WG_OK;
}

int default_ctx(wg_ctx **out) {
  std::lock_guard<std::mutex> lk(g_default_mu);
  if (!g_default)
    if (int rc = make_ctx(0, &g_default)) return rc;
  *out = g_default;
  return WG_OK;
}

// every entry point starts here: the context's device becomes the calling thread's current device
int use_ctx(wg_ctx *ctx) {
  if (!ctx) return fail(WG_ERR_BAD_ARG, "null context");
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != ctx->device) HIP_TRY(hipSetDevice(ctx->device));
  return WG_OK;
}

// Both with ctx->launch_mu held, around the launch.
// before a launch that uses device state of the context (`o`): behind the previous such launch, whatever stream that was on
inline bool slot_pending(const wg_ctx::SlotOrder &o) { return o.armed && hipEventQuery(o.ev) == hipErrorNotReady; }
inline bool slot_pending_elsewhere(const wg_ctx::SlotOrder &o, hipStream_t st) { return o.stream != st && slot_pending(o); }
int slot_claim(wg_ctx *ctx, wg_ctx::SlotOrder &o, hipStream_t st, const char *what) {
  if (!slot_pending(o)) return WG_OK;
  // the handle alone does not identify a stream (one destroyed and re-created at the same address counts as the same): the wait
  // is issued whenever the previous launch is pending -- behind a launch of the same stream it costs nothing
  if (o.stream != st) {
    if (ctx->overlap_strict)
      return fail(WG_ERR_BUSY, "a %s launch of this context is still in flight on another stream (WG_OVERLAP_STRICT: launches of one "
                               "context are refused instead of ordered; give each stream its own wg_ctx to overlap them)", what);
    if (ctx->serialised++ == 0 && getenv("WG_OVERLAP_NOTE"))
      fprintf(stderr, "wg_mpc: a %s launch was ordered behind one of another stream of the same context (first occurrence; "
                      "wg_overlap_serialised() counts them, one wg_ctx per stream overlaps them)\n", what);
  }
  HIP_TRY(hipStreamWaitEvent(st, o.ev, 0));
  return WG_OK;
}
// a re-configuration overwrites tables that launches of THIS context may still be reading: wait for those launches (their events,
// the context's own streams) -- not for the device
int ctx_wait_own(wg_ctx *ctx) {
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  for (wg_ctx::SlotOrder *o : {&ctx->guard_order, &ctx->qp_order, &ctx->asm_order, &ctx->aux_order, &ctx->fc_order, &ctx->walk_order, &ctx->mo_order, &ctx->audit_order})
    if (o->armed) HIP_TRY(hipEventSynchronize(o->ev));
  if (ctx->host_stream) HIP_TRY(hipStreamSynchronize(ctx->host_stream));
  if (ctx->pin_stream) HIP_TRY(hipStreamSynchronize(ctx->pin_stream));
  return WG_OK;
}
// Staging of the host-pointer entry points and the configure functions: copies, launches and copies back go on the context's
// stream, from and to the caller's pageable arrays (the runtime stages those), and the call waits for that stream before it
// returns -- on EVERY path: once anything was handed the stream, an error return first waits for what is queued on it.
// Constructed with ctx->mu held, behind every host buffer the copies name (so that it is destroyed, and waits, before they are).
struct HostScope {
  wg_ctx *ctx;
  bool used = false;
  explicit HostScope(wg_ctx *c) : ctx(c) {}
  HostScope(const HostScope &) = delete;
  ~HostScope() { if (used) (void)hipStreamSynchronize(ctx->host_stream); }
  hipStream_t stream() { used = true; return ctx->host_stream; }
  hipError_t wait() { used = false; return hipStreamSynchronize(ctx->host_stream); }
};
#define WG_H2D(dst, src, bytes) HIP_TRY(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyHostToDevice, hs.stream()))
#define WG_D2H(dst, src, bytes) HIP_TRY(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToHost, hs.stream()))
#define WG_ZERO(dst, bytes) HIP_TRY(hipMemsetAsync((dst), 0, (bytes), hs.stream()))
#define WG_HOST_WAIT() HIP_TRY(hs.wait())
// One device buffer carved into the arrays of a call: take<T>() every array first, reserve() once, then arena(seg) is the
// array (null for an array of no elements: an optional one the caller left out).  Every array starts on a 256-byte boundary.
template <class T> struct Seg {
  size_t off = 0, count = 0;
  size_t bytes() const { return count * sizeof(T); }
};
struct Arena {
  DevBuf &buf;
  size_t size = 0;
  explicit Arena(DevBuf &b) : buf(b) {}
  template <class T> Seg<T> take(size_t count) {
    Seg<T> s{size, count};
    size += (count * sizeof(T) + 255) & ~(size_t)255;
    return s;
  }
  int reserve() { return buf.reserve(size); }
  template <class T> T *operator()(const Seg<T> &s) const { return s.count ? reinterpret_cast<T *>(static_cast<char *>(buf.p) + s.off) : nullptr; }
};
// after it: the event later launches are ordered behind
int slot_mark(wg_ctx::SlotOrder &o, hipStream_t st) {
  if (!o.ev) HIP_TRY(hipEventCreateWithFlags(&o.ev, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(o.ev, st));
  o.stream = st; o.armed = true;
  return WG_OK;
}

// the order of one launch: (re)uses `s` for the batch (key, B) on stream st.  iters_out always; order only when the previous launch
// of this kind was the same batch (its iteration counts are the prediction)
int lpt_prepare(Lpt &s, const void *key, int B, hipStream_t st, int **order, int **iters_out) {
  const bool known = s.key == key && s.B == B && s.buf.p;
  if (int rc = s.buf.reserve((size_t)B * 2 * sizeof(int))) return rc;
  *iters_out = static_cast<int *>(s.buf.p);
  if (known) {
    *order = *iters_out + B;
    hipLaunchKernelGGL(wg_lpt_order_kernel, dim3(1), dim3(1024), 0, st, B, *iters_out, *order);
  }
  s.key = key; s.B = B;
  return WG_OK;
}

// one launch with `lds` bytes of dynamic LDS: above 64 KB the kernel is first given leave to use them
template <class Kernel, class... Args>
int launch_lds(Kernel kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  HIP_TRY(hipGetLastError());
  return WG_OK;
}

// the entry points without a context argument: the same call on the process-wide default context
template <class R, class... P, class... A>
R on_default(R (*fn)(wg_ctx *, P...), A... args) {
  wg_ctx *c = nullptr;
  if (int rc = default_ctx(&c)) return std::is_same<R, int>::value ? (R)rc : (R)-1;
  return fn(c, args...);
}

}  // namespace

extern "C" {

static_assert(sizeof(wg_tick_out_t) == 61 * 128, "wg_tick_out_t: whole 128-byte lines (include/wg_mpc.h)");
int wg_abi_version(void) { return 5; }

const char *wg_last_error(void) { return g_err.c_str(); }

int wg_ctx_create(int device_ordinal, wg_ctx_t **out) {
  if (!out) return fail(WG_ERR_BAD_ARG, "null out pointer");
  *out = nullptr;
  return make_ctx(device_ordinal, out);
}

void wg_ctx_destroy(wg_ctx_t *ctx) {
  if (!ctx) return;
  {
    std::lock_guard<std::mutex> lk(g_default_mu);
    if (ctx == g_default) g_default = nullptr;
  }
  int cur = -1;
  if (hipGetDevice(&cur) == hipSuccess && cur != ctx->device) (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  ctx->release_all();
  delete ctx;
}

int wg_ctx_device(const wg_ctx_t *ctx) { return ctx ? ctx->device : -1; }

int wg_set_overlap_strict_ctx(wg_ctx_t *ctx, int on) {
  if (!ctx) return fail(WG_ERR_BAD_ARG, "null context");
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  ctx->overlap_strict = on != 0;
  return WG_OK;
}

long long wg_overlap_serialised_ctx(wg_ctx_t *ctx) {
  if (!ctx) return -1;
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  return ctx->serialised;
}

int wg_shard_range(long long total, int rank, int world, long long *lo, long long *hi) {
  if (total < 0 || world < 1 || rank < 0 || rank >= world || !lo || !hi)
    return fail(WG_ERR_BAD_ARG, "wg_shard_range: need total >= 0, 0 <= rank < world");
  const long long base = total / world, rem = total % world;
  *lo = rank * base + (rank < rem ? rank : rem);
  *hi = *lo + base + (rank < rem ? 1 : 0);
  return WG_OK;
}

int wg_init(int device_ordinal) {
  std::lock_guard<std::mutex> lk(g_default_mu);
  if (g_default && g_default->device == device_ordinal) return use_ctx(g_default);
  wg_ctx *fresh = nullptr;
  if (int rc = make_ctx(device_ordinal, &fresh)) return rc;
  if (g_default) { g_default->release_all(); delete g_default; }
  g_default = fresh;
  return WG_OK;
}

void wg_shutdown(void) {
  wg_ctx *c = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_default_mu);
    c = g_default;
    g_default = nullptr;
  }
  if (c) { c->release_all(); delete c; }
}

#ifdef WG_PROFILE
// diagnostic build only: read-and-reset the in-kernel phase timers (shader cycles)
int wg_prof_read(unsigned long long *out48) {          // 48 counters (wg_ql_view.hpp, g_prof)
  if (hipMemcpyFromSymbol(out48, HIP_SYMBOL(wg::g_prof), 48 * sizeof(unsigned long long)) != hipSuccess) return -1;
  unsigned long long z[48] = {0};
  if (hipMemcpyToSymbol(HIP_SYMBOL(wg::g_prof), z, sizeof z) != hipSuccess) return -1;
  return 0;
}
#endif

size_t wg_qp_lds_bytes(int n, int m) { return wg::QlDims(n, m, m).bytes(); }

static int qp_check(wg_ctx *ctx, int B, int nmax, int mmax, const double *C, const double *d, const double *A, const double *b, const double *xl, const double *xu, const double *x, const int *ifail) {
  if (int rc = use_ctx(ctx)) return rc;
  if (B < 0 || nmax <= 0 || mmax <= 0) return fail(WG_ERR_BAD_ARG, "bad sizes B=%d nmax=%d mmax=%d", B, nmax, mmax);
  if (!C || !d || !A || !b || !xl || !xu || !x || !ifail) return fail(WG_ERR_BAD_ARG, "null required pointer");
  return WG_OK;
}

int wg_qp_solve_batch_dev_ctx(wg_ctx_t *ctx, int B, int nmax, int mmax, const int *n, const int *m, const int *me, const double *C, const double *d, const double *A, const double *b, const double *xl, const double *xu, double eps, double *x, double *u, int *ifail, int *n_iter, int *iact, int *nact, int *hist, int hist_cap, int *hist_len, void *hip_stream) {
  if (int rc = qp_check(ctx, B, nmax, mmax, C, d, A, b, xl, xu, x, ifail)) return rc;
  if (hist && (!hist_len || hist_cap <= 0)) return fail(WG_ERR_BAD_ARG, "hist needs hist_len and hist_cap > 0");
  if (B == 0) return WG_OK;
  const int m_cap = m ? mmax : mmax - 1;
  size_t lds = wg::QlDims(nmax, m_cap, m_cap).bytes();
  // A (m x n, the largest operand) is only ever read: staged in LDS it caps the residency (n = 36, m = 75: 54 KB, three QPs
  // per CU), read in place it comes from L2 and the CU holds five -- measured 274 k vs 223 k QPs/s on the probe's QPs.  It
  // goes to LDS only while that does not cost a resident QP (8 per CU = two waves per SIMD is the useful maximum).
  int a_in_lds = 1, g_in_lds = 1;
  auto lds_for = [&](bool a, bool g) { return wg::QlDims(nmax, m_cap, m_cap, true, a, 0, true, true, true, true, 0, g).bytes(); };
  const size_t lds_noa = lds_for(false, true), lds_noag = lds_for(false, false);
  // residency each placement reaches: LDS, and the registers -- the kernels with G in LDS take 259 registers (one wave per
  // SIMD, four QPs per CU), the one with G in place is compiled for two waves per SIMD
  if (per_cu_160k(lds_noa, 4) > per_cu_160k(lds, 4)) a_in_lds = 0;
  // G follows A out of the LDS when that buys at least two more resident QPs (G is cold after the factorisation; measured on the
  // Herdt workload's real QPs, n = 36, m = 75: 7 per CU against 4)
  if (!a_in_lds && per_cu_160k(lds_noag, 8) >= per_cu_160k(lds_noa, 4) + 2) g_in_lds = 0;
  a_in_lds = env_flag("WG_QL_A_IN_LDS", a_in_lds);                         // tests force either path
  g_in_lds = env_flag("WG_QL_G_IN_LDS", g_in_lds);
  if (lds > 160 * 1024) a_in_lds = 0;
  if (a_in_lds) g_in_lds = 1;                                              // G leaves only after A
  if (!a_in_lds && lds_noa > 160 * 1024) g_in_lds = 0;
  lds = lds_for(a_in_lds, g_in_lds);
  if (lds > 160 * 1024) return fail(WG_ERR_TOO_LARGE, "QP (n=%d, m=%d) needs %zu B of LDS > 160 KiB", nmax, m_cap, lds);
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  // wa | b follow A and G out of the LDS when that buys one more resident QP (n = 36, m = 75: 21.7 -> 20.2 KB, the eighth QP
  // of the CU -- a batch of 4096 is then exactly two rounds of the 2048 resident waves).  WG_QL_W_IN_LDS=0/1 forces either.
  // The slots are used by one launch at a time: the test "are they free", the launch and the event behind it happen under one
  // lock (two host threads on two streams cannot both find them free); a launch that finds them in use by another stream keeps
  // wa | b in LDS instead of waiting for them.
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  double *wab = nullptr;
  if (!a_in_lds && !g_in_lds) {
    const size_t lds_now = wg::QlDims(nmax, m_cap, m_cap, true, false, 0, true, true, false, true, 0, false).bytes();
    const bool w_out = !env_flag("WG_QL_W_IN_LDS", per_cu_granules(lds_now, 8) <= per_cu_granules(lds, 8));
    if (w_out && !slot_pending_elsewhere(ctx->qp_order, st)) {
      if (int rc = ctx->qp_slot.reserve((size_t)B * (2 * (size_t)mmax + nmax) * 8)) return rc;
      wab = static_cast<double *>(ctx->qp_slot.p);
      lds = lds_now;
    }
  }
  // more QPs than resident waves: start them longest-solve-first by the iteration counts of the previous batch on the same
  // arrays (scheduling only; a caller that interleaves unrelated batches merely loses the benefit).  WG_QL_LPT=0: index order
  int *order = nullptr, *iters_out = nullptr;
  // the order lives in a buffer of the context: only a launch that also owns the context's wa | b slots uses it (those are
  // handed to one launch at a time: see above), so no other launch rewrites the order under this one's blocks
  if (wab != nullptr && (size_t)B > (size_t)ctx->num_cu * per_cu_granules(lds, 8) && env_flag("WG_QL_LPT", true))
    if (int rc = lpt_prepare(ctx->qp_lpt, C, B, st, &order, &iters_out)) return rc;
  // where A / G / wa | b live is a template argument; the Herdt-sized boundary (what QPProblem::solve hands over at N = 16:
  // nmax = 36, mmax = 76) has its own instantiation
  const bool fixed36 = wab && nmax == 36 && mmax == 76 && env_flag("WG_QL_FIXED", true);
  if (fixed36) lds = wg::QlView::fixed_dense_bytes<36>();
  void (*kern)(int, int, int, const int *, const int *, const int *, const double *, const double *, const double *, const double *,
               const double *, const double *, double, double *, double *, int *, int *, int *, int *, int *, int, int *, double *,
               const int *, int *);
  if (fixed36) kern = wg_ql_dense_kernel<false, false, false, 36, 76>;
  else if (a_in_lds) kern = wg_ql_dense_kernel<true, true>;
  else if (g_in_lds) kern = wg_ql_dense_kernel<false, true>;
  else if (wab) kern = wg_ql_dense_kernel<false, false, false>;
  else kern = wg_ql_dense_kernel<false, false>;
  if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3(B), dim3(64), lds, st, B, nmax, mmax, n, m, me, C, d, A, b, xl, xu, eps, x, u, ifail, n_iter, iact, nact,
                     hist, hist_cap, hist_len, wab, order, iters_out);
  if (wab)
    if (int rc = slot_mark(ctx->qp_order, st)) return rc;
  HIP_TRY(hipGetLastError());
  return WG_OK;
}

int wg_qp_solve_batch_ctx(wg_ctx_t *ctx, int B, int nmax, int mmax, const int *n, const int *m, const int *me, const double *C, const double *d, const double *A, const double *b, const double *xl, const double *xu, double eps, double *x, double *u, int *ifail, int *n_iter, int *iact, int *nact, int *hist, int hist_cap, int *hist_len) {
  if (int rc = qp_check(ctx, B, nmax, mmax, C, d, A, b, xl, xu, x, ifail)) return rc;
  if (B == 0) return WG_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HostScope hs(ctx);
  const size_t sB = (size_t)B, sn = (size_t)nmax, sm = (size_t)mmax;
  Arena in(ctx->in), out(ctx->out);
  const auto iC = in.take<double>(sB * sn * sn), id = in.take<double>(sB * sn), iA = in.take<double>(sB * sm * sn), ib = in.take<double>(sB * sm),
             ixl = in.take<double>(sB * sn), ixu = in.take<double>(sB * sn);
  const auto in_ = in.take<int>(n ? sB : 0), im = in.take<int>(m ? sB : 0), ime = in.take<int>(me ? sB : 0);
  const auto ox = out.take<double>(sB * sn), ou = out.take<double>(u ? sB * (sm + 2 * sn) : 0);
  const auto oifail = out.take<int>(sB), oiter = out.take<int>(n_iter ? sB : 0), oiact = out.take<int>(iact ? sB * sn : 0),
             onact = out.take<int>(nact ? sB : 0), ohist = out.take<int>(hist ? sB * hist_cap : 0), ohlen = out.take<int>(hist_len ? sB : 0);
  if (int rc = in.reserve()) return rc;
  if (int rc = out.reserve()) return rc;
  WG_H2D(in(iC), C, iC.bytes());
  WG_H2D(in(id), d, id.bytes());
  WG_H2D(in(iA), A, iA.bytes());
  WG_H2D(in(ib), b, ib.bytes());
  WG_H2D(in(ixl), xl, ixl.bytes());
  WG_H2D(in(ixu), xu, ixu.bytes());
  if (n) WG_H2D(in(in_), n, in_.bytes());
  if (m) WG_H2D(in(im), m, im.bytes());
  if (me) WG_H2D(in(ime), me, ime.bytes());
  WG_ZERO(ctx->out.p, out.size);
  if (int rc = wg_qp_solve_batch_dev_ctx(ctx, B, nmax, mmax, in(in_), in(im), in(ime), in(iC), in(id), in(iA), in(ib), in(ixl), in(ixu), eps, out(ox),
                                         out(ou), out(oifail), out(oiter), out(oiact), out(onact), out(ohist), hist_cap, out(ohlen), hs.stream()))
    return rc;
  WG_D2H(x, out(ox), ox.bytes());
  if (u) WG_D2H(u, out(ou), ou.bytes());
  WG_D2H(ifail, out(oifail), oifail.bytes());
  if (n_iter) WG_D2H(n_iter, out(oiter), oiter.bytes());
  if (iact) WG_D2H(iact, out(oiact), oiact.bytes());
  if (nact) WG_D2H(nact, out(onact), onact.bytes());
  if (hist) WG_D2H(hist, out(ohist), ohist.bytes());
  if (hist_len) WG_D2H(hist_len, out(ohlen), ohlen.bytes());
  WG_HOST_WAIT();
  return WG_OK;
}

}  // extern "C"

// ===========================================================================
// Herdt-2010 MPC tick, batched (include/wg_mpc.h, second half)
// ===========================================================================

namespace {
inline bool tick_compact(const wg_model_t &m);
// at most two step changes fit in the preview window when N*T <= 2*step_period (each change is one step period
// after the previous one and the first previewed change is at pi >= 1): the compact kernel is sized for that
inline int tick_smax(const wg_model_t &m) { return tick_compact(m) ? 2 : wg::kSMax; }
inline int tick_max_n(const wg_model_t &m) { return 2 * m.N + 2 * tick_smax(m); }
inline int tick_max_m(const wg_model_t &m) { return 1 + 4 * m.N + 5 * tick_smax(m); }
// Problem views of the tick kernel (template argument of wg_mpc_tick_kernel):
//   16  compact  rows in registers, no G / A anywhere: N == 16 with at most two previewed steps (the benchmark model)
//   -1  element  G / A regenerated per element from the compact tables, Z in a global slot: every other model
//    0  dense    G and A as LDS matrices: on request (WG_TICK_DENSE=1, while they fit the CU's 160 KiB) and for
//                wg_mpc_assemble_batch, which writes the QP out
// WG_TICK_VIEW=element sends N == 16 through the element view as well (tests).
// the most steps a horizon can preview (wg_tick_tables_math.hpp): the kernels hold wg::kSMax, wg_mpc_configure refuses models beyond
inline int tick_max_prw_steps(const wg_model_t &m) { return wg::tt_max_prw_steps(m); }
inline bool tick_compact(const wg_model_t &m) {
  const char *v = getenv("WG_TICK_VIEW");
  return m.N == 16 && m.N * m.T <= 2.0 * m.step_period + 1e-12 && !env_flag("WG_TICK_DENSE", false) && !(v && *v);
}
// element view (-1: any horizon; 32: BASELINE config 5's horizon as a compile-time constant -- same LDS bytes, same slot, a fixed
// layout): Z in a per-block slot of global memory instead of LDS (decided at compile time: mpc_tick<-1>, mpc_tick<32>)
inline bool tick_elem(int view) { return view == -1 || view == 32; }
inline int tick_waves_per_simd(int view) { return tick_elem(view) ? WG_TICK32_WPE : WG_TICK_WPE_MAX; }
inline bool tick_z_global(int view) { return tick_elem(view); }
// compact view (N = 16): wa, b and the border block Gv in a per-block slot of global memory (decided at compile time: mpc_tick<16>)
inline bool tick16_ext(int view) { return view == 16; }
// the solver area of a wave's LDS (the tick's own arrays follow it)
inline size_t tick_ql_bytes_for(const wg_model_t &m, int view, int r_cols) {
  const bool ext = tick16_ext(view) || tick_z_global(view);
  return (wg::QlDims(tick_max_n(m), tick_max_m(m), tick_max_m(m), view == 0, true, 0, view == 0, !tick_z_global(view),
                           !ext, !tick_elem(view), r_cols).bytes() + 15) & ~(size_t)15;
}
inline size_t tick_lds_with_cap(const wg_model_t &m, int view, int r_cols) {
  const bool ext = tick16_ext(view) || tick_z_global(view);        // wa, b, Gv (element view: the rows too) in the global slot
  const size_t ql = tick_ql_bytes_for(m, view, r_cols);
  const int gvld = view == 16 ? wg::kGvLd : (tick_elem(view) ? wg::kGvLdElem : 0);
  size_t tick = wg::TickLds::bytes(m.N, tick_smax(m), gvld, view == 16, !ext, !tick_elem(view), tick_elem(view));
  tick = (tick + 15) & ~(size_t)15;                        // the fixed element view puts the solver area behind it
  // element view, short horizons: the pre-solve overlay does not fit over R; it gets its own bytes behind the tick's arrays
  if (view == -1 && wg::TickLds::elem_overlay_apart(m.N, sizeof(wg_gait_state_t)))
    tick = ((tick + 15) & ~(size_t)15) + wg::TickLds::elem_overlay_need(m.N, sizeof(wg_gait_state_t));
  return ql + tick;
}
// Element view: how many columns of R the LDS holds (0: all of them).  R is the operand that decides the residency at N = 32
// (21.6 KB of the 26.8): the LDS keeps the first c columns and one working column, and a solve whose active set outgrows them
// moves its R to the per-block global slot and GOES ON there (mpc_tick<-1>, QlResume: no repeat; measured: even a cap most solves
// outgrow costs a few per cent).  So the cap is simply the largest one that reaches the best residency the kernel's register
// budget admits: 41 columns at N = 32 = 12 640 B of LDS = twelve gaits per CU, three on every SIMD.  WG_ELEM_NACT_CAP forces a
// value (tests run with tiny caps so that every solve takes the second route).
inline int tick_elem_cap(const wg_model_t &m, int view) {
  if (!tick_elem(view)) return 0;
  const int n = tick_max_n(m);
  const size_t overlay = wg::TickLds::pre_bytes(m.N, tick_smax(m)) + sizeof(wg_gait_state_t) + 32;
  // the pre-solve overlay -- the parked state copy at its end is fetched back right after the solve, while x still holds the
  // solution -- must lie within R and the four scratch vectors behind it (QlView::carve, lean layout); sized for the smallest
  // problem of the model (no previewed step: n = 2N: working column and scratch vectors of 2N entries each)
  auto fits = [&](int c) { return (size_t)8 * ((size_t)c * (c + 1) / 2 + (size_t)(2 * m.N) + (size_t)(4 * 2 * m.N)) >= overlay; };
  if (wg::TickLds::elem_overlay_apart(m.N, sizeof(wg_gait_state_t))) return 0;     // short horizons: R whole, the overlay apart
  if (const char *e = getenv("WG_ELEM_NACT_CAP")) {
    int c = atoi(e);
    if (c <= 0 || c >= n) return 0;
    while (c < n - 1 && !fits(c)) ++c;
    return (c < n && fits(c)) ? c : 0;
  }
  // waves a CU holds by the registers the element view's kernels are compiled for (WG_TICK32_WPE per SIMD, four SIMDs)
  auto per_cu = [&](int c) { return per_cu_granules(tick_lds_with_cap(m, view, c), 4 * (size_t)tick_waves_per_simd(view)); };
  const size_t full = per_cu(0);
  int best = 0;
  size_t best_k = full;
  for (int c = n - 1; c >= n / 4; --c)                   // descending: the first cap that reaches a residency is the largest
    if (fits(c) && per_cu(c) > best_k) { best = c; best_k = per_cu(c); }
  return best;
}
// what the kernels receive: the column cap in the low 16 bits; tests may ask the solver to give up EARLIER than the layout
// requires (WG_ELEM_ABORT_AT: active-set size at which the first attempt stops), so that the second route is taken often
inline int tick_elem_cap_arg(int c) {
  if (!c) return 0;
  const int v = env_int("WG_ELEM_ABORT_AT", 0);
  return c | ((v >= 1 && v < c ? v : c) << 16);
}
inline size_t tick_z_slot_doubles(const wg_model_t &m, int view) {
  const size_t n = (size_t)tick_max_n(m), mm = (size_t)tick_max_m(m);
  if (view == 16) return (n + 2 * mm) + n * wg::kGvLd;       // wa | b | Gv
  // element view: Z | wa | b | Gv | rowA | rowB | rowK | gd | d | wd | wx | R in full (mpc_tick<-1>)
  // (the fixed N = 32 view keeps Z with leading dimension n: whole cache lines per column; slots are multiples of 64 bytes)
  const size_t zd = view == 32 ? n * n : n * (n | 1);
  return (zd + (n + 2 * mm) + n * wg::kGvLdElem + 2 * mm + (mm + 1) / 2 + 2 + 4 * n + (n * (n + 1) / 2 + n) + 7) & ~(size_t)7;
}
inline size_t tick_lds_for(const wg_model_t &m, int view) { return tick_lds_with_cap(m, view, tick_elem_cap(m, view)); }
inline int tick_view(const wg_model_t &m) {
  if (tick_compact(m)) return 16;
  const bool dense_fits = tick_lds_for(m, 0) <= 160 * 1024;
  if (env_flag("WG_TICK_DENSE", false) && dense_fits) return 0;          // tests: the dense view where the element view would be taken
  // Everywhere else the element view: 5 - 12.6 KB of LDS per gait (twelve per CU, three on every SIMD) against the dense view's
  // G and A as LDS matrices (N = 20: 100 KB, ONE gait per CU -- measured 1.65 M against 0.39 M ticks/s; N = 24: 1.15 M against
  // 0.27 M; same bits).  Its pre-solve group lies over R (short horizons: in bytes of its own, TickLds::elem_overlay_apart)
  // N = 32 (BASELINE config 5) has an instantiation with the horizon as a compile-time constant (mpc_tick<32>: every slot and
  // LDS offset a constant, only the two-rows-per-lane forms of the solver); WG_TICK_ELEM_GENERIC=1 keeps the any-horizon
  // kernel there too (tests run both: same bytes)
  if (m.N == 32) {
    if (env_flag("WG_TICK_ELEM_GENERIC", false)) return -1;
    return 32;
  }
  return -1;
}

// Everything a launch of the tick / run kernels derives from the model and the environment, in one place.
struct TickPlan {
  int view;            // problem view = template argument of the kernels
  size_t lds;          // dynamic LDS per block (what wg_mpc_tick_lds_bytes* report)
  size_t launch_lds;   // the same plus WG_TICK_LDS_PAD (experiments: lower the residency)
  size_t qlb;          // the solver area's share of it
  size_t zslot;        // doubles per block in tick_z (views that keep operands in a global slot; see `slots`)
  int ecap;            // element view: the column cap of R as the kernels receive it
  size_t wave_cap;     // waves per CU the kernel's register budget admits
  bool slots;
  explicit TickPlan(const wg_model_t &m) : view(tick_view(m)) {
    const int cap = tick_elem_cap(m, view);
    lds = tick_lds_with_cap(m, view, cap);
    launch_lds = lds + (size_t)env_int("WG_TICK_LDS_PAD", 0);
    qlb = tick_ql_bytes_for(m, view, cap);
    zslot = tick_z_slot_doubles(m, view);
    ecap = tick_elem_cap_arg(cap);
    wave_cap = 4 * (size_t)tick_waves_per_simd(view);
    slots = tick_z_global(view) || tick16_ext(view);
  }
  int per_cu() const { return (int)per_cu_granules(launch_lds, wave_cap); }   // blocks a CU keeps resident
  // the per-block solver slots for a grid of `blocks`: sized for the grid a launch has (a one-robot facade pays for one slot, a
  // fleet for its resident waves); growing never frees what a launch in flight may be using (DevBuf)
  int reserve_slots(wg_ctx *ctx, int blocks, double **zs) const {
    *zs = nullptr;
    if (!slots) return WG_OK;
    if (int rc = ctx->tick_z.reserve((size_t)blocks * zslot * 8)) return rc;
    *zs = static_cast<double *>(ctx->tick_z.p);
    return WG_OK;
  }
  int raise_lds(const void *kernel) const {
    if (launch_lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)launch_lds));
    return WG_OK;
  }
};
// multi-tick launches, hand-over inside one XCD: ring slots per XCD (a gait is in at most one ring, at most once) and the bytes
// of run_buf [control | rings | done flags]
inline int run_ring_cap(int B) { int cap = 1; while (cap < 2 * B) cap <<= 1; return cap; }
inline size_t run_buf_bytes(int B) { return sizeof(wg_xrun_ctl) + (size_t)kXcds * run_ring_cap(B) * 8 + (size_t)B * 4; }
// hand-over inside one XCD (default) or through one device-wide queue (WG_RUN_QUEUE=global: A/B tests)
inline bool run_queue_xcd() { const char *e = getenv("WG_RUN_QUEUE"); return !e || e[0] != 'g'; }

// TickTables::ql_sums from the environment, read at the call (wg_mpc_configure, wg_mpc_block*): tests and A/B.
int tick_ql_knobs(int *out) {
  int k = 0;
  // the compact view's decision-only sums: unset = guarded by certificates, "ordered" = the reference's order throughout,
  // "doubt" = every dependence test falls back and every solve is run twice
  if (const char *e = getenv("WG_QL_SUMS")) {
    const std::string v(e);
    if (v == "ordered") k = wg::kSumsOrdered;
    else if (v == "doubt") k = wg::kSumsDoubt;
    else if (!v.empty() && v != "guarded") return fail(WG_ERR_BAD_ARG, "WG_QL_SUMS=%s: ordered, doubt or unset", e);
  }
  // the compact view's norm chain of a sweep (in bits 8 - 9 of the same word): unset or "seeded" = from seeds, checked once;
  // "exact" = the exact chain throughout; "doubt" = the check reports a mismatch in every sweep
  if (const char *e = getenv("WG_QL_NORMS")) {
    const std::string v(e);
    if (v == "exact") k |= wg::kNormsExact;
    else if (v == "doubt") k |= wg::kNormsDoubt;
    else if (!v.empty() && v != "seeded") return fail(WG_ERR_BAD_ARG, "WG_QL_NORMS=%s: seeded, exact, doubt or unset", e);
  }
  *out = k;
  return WG_OK;
}

int tick_check(wg_ctx *ctx, int B, const wg_gait_state_t *states) {
  if (int rc = use_ctx(ctx)) return rc;
  if (!ctx->model_set) return fail(WG_ERR_BAD_ARG, "wg_mpc_configure() has not been called on this context");
  if (B < 0 || !states) return fail(WG_ERR_BAD_ARG, "bad arguments");
  return WG_OK;
}
}  // namespace

extern "C" {

void wg_model_defaults(wg_model_t *m) {
  memset(m, 0, sizeof *m);
  m->N = 16; m->flags = 0; m->T = 0.1; m->Tctrl = 0.005; m->com_height_qp = 0.814;
  m->alpha = 1.0; m->beta = 0.00001; m->gamma = 0.000001;
  m->sole_w = 0.25; m->sole_h = 0.14;
  m->margin_x = 0.04; m->margin_y = 0.04; m->ds_feet_distance = 0.2;
  m->hip_l_lo = -30.0 / 180.0 * wg::kPi; m->hip_l_hi = 45.0 / 180.0 * wg::kPi;
  m->hip_r_lo = -30.0 / 180.0 * wg::kPi; m->hip_r_hi = 45.0 / 180.0 * wg::kPi;
  m->hip_vmax = 0.0; m->hip_amax = 0.1; m->feet_cross_max = 5.0 / 180.0 * wg::kPi;
  m->step_period = 0.8; m->ds_period = 1e9; m->dsss_period = 0.8;
  m->t_single = 0.7; m->t_double = 0.1; m->step_height = 0.05; m->feet_distance = 0.2;
}

void wg_gait_init(const wg_model_t *, wg_gait_state_t *s, const double com0[3], const double left_xyt[3],
                  const double right_xyt[3]) {
  memset(s, 0, sizeof *s);
  s->online = 1; s->time_to_stop = -1.0;
  for (int k = 0; k < 3; k++) {
    s->lf[k].x = left_xyt[0]; s->lf[k].y = left_xyt[1]; s->lf[k].theta = left_xyt[2];
    s->rf[k].x = right_xyt[0]; s->rf[k].y = right_xyt[1]; s->rf[k].theta = right_xyt[2];
  }
  s->phase = WG_DS; s->foot = WG_LEFT; s->time_limit = 1000000000; s->nb_steps_left = 1;
  s->sup_x = left_xyt[0]; s->sup_y = left_xyt[1]; s->sup_yaw = left_xyt[2] * wg::kPi / 180;
  s->com_x[0] = com0[0]; s->com_y[0] = com0[1]; s->com_z = com0[2];
  s->front_com_x[0] = com0[0]; s->front_com_y[0] = com0[1];
  s->nb_steps_ssds = 2; s->rot_support_foot = WG_LEFT;
}

int wg_mpc_configure_ctx(wg_ctx_t *ctx, const wg_model_t *model) {
  if (int rc = use_ctx(ctx)) return rc;
  if (!model) return fail(WG_ERR_BAD_ARG, "null model");
  if (model->N < 2 || model->N > wg::kNMaxH) return fail(WG_ERR_BAD_ARG, "N=%d outside [2,%d]", model->N, wg::kNMaxH);
  if ((int)(model->T / model->Tctrl) != WG_SAMPLES_PER_TICK)
    return fail(WG_ERR_BAD_ARG, "T/Tctrl must be %d", WG_SAMPLES_PER_TICK);
  if (tick_max_prw_steps(*model) > wg::kSMax)
    return fail(WG_ERR_BAD_ARG, "step_period=%g: a horizon of N=%d instants of T=%g previews up to %d steps, the tick holds %d",
                model->step_period, model->N, model->T, tick_max_prw_steps(*model), wg::kSMax);
  const size_t lds = TickPlan(*model).lds;
  if (lds > 160 * 1024) return fail(WG_ERR_TOO_LARGE, "tick needs %zu B of LDS > 160 KiB", lds);
  std::vector<double> qb;                              // Q_b from the matrix cores, when the model asks for it
  if (model->flags & (WG_FLAG_GRAMIAN_MFMA_F64 | WG_FLAG_GRAMIAN_MFMA_F32)) {
    qb.resize((size_t)model->N * model->N);
    const int prec = (model->flags & WG_FLAG_GRAMIAN_MFMA_F32) ? WG_GRAMIAN_F32 : WG_GRAMIAN_F64;
    if (int rc = wg_gramian_batch_ctx(ctx, 1, model->N, &model->T, &model->com_height_qp, model->alpha, model->beta, model->gamma,
                                  prec, qb.data()))
      return rc;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  std::unique_ptr<wg::TickTables> host_tables_p(new wg::TickTables);
  wg::TickTables &host_tables = *host_tables_p;
  wg::build_tables(*model, host_tables, qb.empty() ? nullptr : qb.data());
  if (!host_tables.blocks_ok && !qb.empty())
    return fail(WG_ERR_BAD_ARG, "the matrix-core Gramian is not positive definite enough for ql0002's factorisation");
  if (int rc = tick_ql_knobs(&host_tables.ql_sums)) return rc;
  if (!ctx->tables_dev) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->tables_dev), sizeof(wg::TickTables)));
  if (!ctx->model_dev) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->model_dev), sizeof(wg_model_t)));
  // a launch of an earlier configuration may still be reading the tables: this context's own launches, on whatever stream they
  // went (every tick / run / assemble launch leaves an event) -- other contexts and other work on the device are not waited for
  if (int rc = ctx_wait_own(ctx)) return rc;
  HostScope hs(ctx);
  WG_H2D(ctx->tables_dev, &host_tables, sizeof host_tables);
  WG_H2D(ctx->model_dev, model, sizeof(wg_model_t));
  WG_HOST_WAIT();
  ctx->model = *model;
  ctx->model_set = true;
  // The queue and the per-block solver slots of the tick / run kernels are sized by the launches themselves, for the grid they have
  // (a one-robot facade object -- B = 1 through wg_mpc_tick_pinned -- pays for ONE slot, 74 KB at N = 32, not for a fleet's
  // 230 MB); wg_mpc_reserve sizes them ahead of time for a fleet that wants no allocation on its first launch.
  return WG_OK;
}

size_t wg_mpc_tick_lds_bytes_for(const wg_model_t *model) {   // host arithmetic only: no device needed
  if (!model || model->N < 2 || model->N > wg::kNMaxH || tick_max_prw_steps(*model) > wg::kSMax) return 0;
  return TickPlan(*model).lds;
}

size_t wg_mpc_tick_lds_bytes_ctx(wg_ctx_t *ctx) {
  if (!ctx || !ctx->model_set) return 0;
  return TickPlan(ctx->model).lds;
}

/* The tick / run kernels' per-block solver slots and queue for fleets of up to max_gaits, allocated now instead of by the first
 * launch that needs them (the launches size them for their own grid otherwise). */
int wg_mpc_reserve_ctx(wg_ctx_t *ctx, int max_gaits) {
  if (int rc = use_ctx(ctx)) return rc;
  if (!ctx->model_set) return fail(WG_ERR_BAD_ARG, "wg_mpc_configure() has not been called on this context");
  if (max_gaits < 1) return fail(WG_ERR_BAD_ARG, "max_gaits = %d", max_gaits);
  const TickPlan plan(ctx->model);
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  double *zs = nullptr;
  if (int rc = plan.reserve_slots(ctx, max_gaits, &zs)) return rc;
  return ctx->run_buf.reserve(run_buf_bytes(max_gaits));
}

/* ---- a model per gait: blocks (the model and its tick tables as opaque bytes, wg_tick_tables_math.hpp) ---------------------- */
size_t wg_mpc_block_bytes(void) { return wg::kMpcBlockBytes; }

// host arithmetic (tt_build through build_tables, as wg_mpc_configure runs it); no device call
int wg_mpc_block(const wg_model_t *model, void *block) {
  if (!block) return fail(WG_ERR_BAD_ARG, "null block");
  memset(block, 0, wg::kMpcBlockBytes);
  if (!model) return fail(WG_ERR_BAD_ARG, "null model");
  if (!wg::tt_model_ok(*model))
    return fail(WG_ERR_BAD_ARG, "not a model a block can be made of: N outside [2,%d], T/Tctrl != %d, more than %d previewed steps, a "
                                "matrix-core Gramian flag, or a T, Tctrl, com_height_qp, alpha, beta, gamma or step_period that is not finite",
                wg::kNMaxH, WG_SAMPLES_PER_TICK, wg::kSMax);
  int knobs = 0;
  if (int rc = tick_ql_knobs(&knobs)) return rc;
  std::unique_ptr<wg::TickTables> t(new wg::TickTables);
  wg::build_tables(*model, *t);
  t->ql_sums = knobs;
  memcpy(block, model, sizeof *model);
  memcpy(static_cast<char *>(block) + wg::kMpcBlockTables, t.get(), sizeof *t);
  return WG_OK;
}

int wg_mpc_block_unpack(const void *block, wg_model_t *model, double *Sv, double *Sz, double *Uv, double *Uz, double *Qb, double *R2, double *Z2, double *diag_b, int *blocks_ok) {
  if (!block) return fail(WG_ERR_BAD_ARG, "null block");
  const wg_model_t &m = *static_cast<const wg_model_t *>(block);
  if (m.N < 2 || m.N > wg::kNMaxH) return fail(WG_ERR_BAD_ARG, "not a block of a model that exists (N = %d)", m.N);
  const wg::TickTables &t = *reinterpret_cast<const wg::TickTables *>(static_cast<const char *>(block) + wg::kMpcBlockTables);
  const size_t N = (size_t)m.N, M2 = 2 * N;
  if (model) *model = m;
  if (Sv) memcpy(Sv, t.Sv, 8 * N * 3);
  if (Sz) memcpy(Sz, t.Sz, 8 * N * 3);
  for (size_t i = 0; i < N; i++) {                       // the tables are laid out for kNMaxH: row by row
    if (Uv) memcpy(Uv + i * N, t.Uv[i], 8 * N);
    if (Uz) memcpy(Uz + i * N, t.Uz[i], 8 * N);
    if (Qb) memcpy(Qb + i * N, t.Qb[i], 8 * N);
  }
  if (R2) memcpy(R2, t.R2, 8 * (M2 * (M2 + 1) / 2));
  if (Z2) memcpy(Z2, t.Z2, 8 * M2 * M2);
  if (diag_b) *diag_b = t.diag_b;
  if (blocks_ok) *blocks_ok = t.blocks_ok;
  return WG_OK;
}

}  // extern "C"
namespace {
// what the fleet launches refuse on the host, before any device call
int mpc_fleet_check(wg_ctx *ctx, int B, const wg_mpc_fleet_t *fl, const wg_gait_state_t *states) {
  if (!fl || !fl->blocks || !fl->model_of) return fail(WG_ERR_BAD_ARG, "null fleet, blocks or model_of");
  if (fl->M < 1 || B < 0) return fail(WG_ERR_BAD_ARG, "M = %d, B = %d", fl->M, B);
  if (!wg::tt_model_ok(fl->base)) return fail(WG_ERR_BAD_ARG, "the fleet's base is not a model a block can be made of (wg_mpc_block refuses it)");
  if (!states) return fail(WG_ERR_BAD_ARG, "bad arguments");
  return use_ctx(ctx);
}
// fl == nullptr: the context's configured model; otherwise a model per gait (blocks[model_of[g]]) in the launch shape of fl->base
int tick_launch(wg_ctx_t *ctx, int B, wg_gait_state_t *states, wg_tick_out_t *outs, int *diag, int advance_calls, int *hist, int hist_cap, int *hist_len, void *hip_stream, wg_gait_state_t *host_states, int *host_done, const wg_mpc_fleet_t *fl = nullptr) {
  if (int rc = fl ? mpc_fleet_check(ctx, B, fl, states) : tick_check(ctx, B, states)) return rc;
  if (hist && (!hist_len || hist_cap <= 0)) return fail(WG_ERR_BAD_ARG, "hist needs hist_len and hist_cap > 0");
  if (B == 0) return WG_OK;
  const TickPlan plan(fl ? fl->base : ctx->model);
  if (int rc = plan.raise_lds(fl ? WG_KERNEL_BY_VIEW(wg_mpc_tick_fleet_kernel, plan.view) : WG_KERNEL_BY_VIEW(wg_mpc_tick_kernel, plan.view))) return rc;
  const int grid = B;                             // one gait per block; the dispatcher balances uneven iteration counts
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);   // ordering test, launch and event record are one critical section
  if (int rc = slot_claim(ctx, ctx->guard_order, st, "tick / run")) return rc;
  double *zs = nullptr;
  if (int rc = plan.reserve_slots(ctx, grid, &zs)) return rc;    // wg_mpc_reserve sizes them ahead of time
  // more gaits than resident waves: start them longest-solve-first (see wg_lpt_order_kernel); the iteration counts are those of
  // the previous call on the same state array -- a prediction, so a caller that interleaves batches merely loses the benefit
  int *order = nullptr, *iters_out = nullptr;
  if (B > ctx->num_cu * plan.per_cu() && !host_states && env_flag("WG_TICK_LPT", true))
    if (int rc = lpt_prepare(ctx->tick_lpt, states, B, st, &order, &iters_out)) return rc;
  if (fl)
    WG_LAUNCH_BY_VIEW(wg_mpc_tick_fleet_kernel, plan.view, grid, plan.launch_lds, st, B, fl->base.N, fl->base.T, fl->base.Tctrl, fl->M,
                      static_cast<const unsigned char *>(fl->blocks), fl->model_of, states, outs, diag, advance_calls, hist, hist_cap, hist_len,
                      (unsigned)plan.qlb, zs, (unsigned)plan.zslot, plan.ecap, order, iters_out);
  else
    WG_LAUNCH_BY_VIEW(wg_mpc_tick_kernel, plan.view, grid, plan.launch_lds, st, B, ctx->model, ctx->tables_dev, states, outs, diag, advance_calls, hist,
                      hist_cap, hist_len, (unsigned)plan.qlb, zs, (unsigned)plan.zslot, plan.ecap, host_states, host_done, order, iters_out);
  HIP_TRY(hipGetLastError());
  return slot_mark(ctx->guard_order, st);
}
}  // namespace
extern "C" {

int wg_mpc_tick_batch_dev_ctx(wg_ctx_t *ctx, int B, wg_gait_state_t *states, wg_tick_out_t *outs, int *diag, int advance_calls, int *hist, int hist_cap, int *hist_len, void *hip_stream) {
  return tick_launch(ctx, B, states, outs, diag, advance_calls, hist, hist_cap, hist_len, hip_stream, nullptr, nullptr);
}

/* ---- one robot (BASELINE configs[1]): state and outputs in host-mapped memory, no copies, no device synchronisation ---- */
int wg_host_alloc(void **out, size_t bytes) {
  if (!out || !bytes) return fail(WG_ERR_BAD_ARG, "wg_host_alloc: null pointer or zero size");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(WG_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU path", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
  HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocMapped | hipHostMallocPortable));   // visible to every device's contexts
  memset(*out, 0, bytes);
  return WG_OK;
}

void wg_host_free(void *p) { if (p) (void)hipHostFree(p); }

int wg_mpc_tick_pinned_ctx(wg_ctx_t *ctx, wg_gait_state_t *state, wg_tick_out_t *out, int *diag, int advance_calls) {
  if (int rc = use_ctx(ctx)) return rc;
  if (!ctx->model_set) return fail(WG_ERR_BAD_ARG, "wg_mpc_configure() has not been called on this context");
  if (!state) return fail(WG_ERR_BAD_ARG, "null state");
  void *d_state = nullptr, *d_out = nullptr, *d_diag = nullptr;
  if (hipHostGetDevicePointer(&d_state, state, 0) != hipSuccess || (out && hipHostGetDevicePointer(&d_out, out, 0) != hipSuccess) ||
      (diag && hipHostGetDevicePointer(&d_diag, diag, 0) != hipSuccess)) {
    (void)hipGetLastError();
    return fail(WG_ERR_BAD_ARG, "wg_mpc_tick_pinned: state / out / diag must come from wg_host_alloc (host-mapped memory)");
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->pin_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx->pin_stream, hipStreamNonBlocking));
  if (!ctx->pin_flag) {
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ctx->pin_flag), 64, hipHostMallocMapped));
    *ctx->pin_flag = 0; ctx->pin_seq = 0;
  }
  if (int rc = ctx->tick_state.reserve(sizeof(wg_gait_state_t))) return rc;
  void *d_flag = nullptr;
  HIP_TRY(hipHostGetDevicePointer(&d_flag, ctx->pin_flag, 0));
  const int want = ++ctx->pin_seq;
  int rc = tick_launch(ctx, 1, static_cast<wg_gait_state_t *>(ctx->tick_state.p), static_cast<wg_tick_out_t *>(d_out),
                       static_cast<int *>(d_diag), advance_calls, nullptr, 0, nullptr, ctx->pin_stream,
                       static_cast<wg_gait_state_t *>(d_state), static_cast<int *>(d_flag));
  if (rc) { --ctx->pin_seq; return rc; }
  // the kernel's last act is a system-scope release on the counter: spin on it (a stream synchronise costs more than the
  // copies this path avoids); fall back to the runtime if it does not move for a long time (a fault, a hung device)
  volatile int *flag = ctx->pin_flag;
  for (long spins = 0; __atomic_load_n(flag, __ATOMIC_ACQUIRE) != want; ++spins) {
    if (spins > 200000000L) { HIP_TRY(hipStreamSynchronize(ctx->pin_stream)); break; }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != want) return fail(WG_ERR_HIP, "wg_mpc_tick_pinned: the kernel ended without signalling");
  return WG_OK;
}

/* ---- the QP of every gait's next tick at the ql0001_ boundary (QPProblem::dump_problem) -------------------------------- */
int wg_mpc_assemble_batch_dev_ctx(wg_ctx_t *ctx, int B, const wg_gait_state_t *states, int advance_calls, int nmax, int mmax, double *C, double *d, double *A, double *b, double *xl, double *xu, int *n, int *m, void *hip_stream) {
  if (int rc = use_ctx(ctx)) return rc;
  if (!ctx->model_set) return fail(WG_ERR_BAD_ARG, "wg_mpc_configure() has not been called on this context");
  if (B < 0 || !states || !C || !d || !A || !b || !xl || !xu || !n || !m) return fail(WG_ERR_BAD_ARG, "bad arguments");
  const wg_model_t &M = ctx->model;
  const int need_n = 2 * M.N + 2 * wg::kSMax, need_m = 1 + 4 * M.N + 5 * wg::kSMax;
  const int need_n2 = tick_compact(M) ? 2 * M.N + 4 : need_n, need_m2 = tick_compact(M) ? 1 + 4 * M.N + 10 : need_m;
  if (nmax < need_n2 || mmax < need_m2 + 1)
    return fail(WG_ERR_BAD_ARG, "nmax >= %d and mmax >= %d needed for this model (mmax = m + 1, qp-problem.cpp:250)", need_n2, need_m2 + 1);
  if (B == 0) return WG_OK;
  // the dense view, laid out for the largest problem any model of this horizon can pose
  const size_t qlb = (wg::QlDims(need_n, need_m, need_m).bytes() + 15) & ~(size_t)15;
  const size_t lds = qlb + wg::TickLds::bytes(M.N, wg::kSMax, 0, false, true, true, false);
  if (lds > 160 * 1024) return fail(WG_ERR_TOO_LARGE, "the dense view of this model needs %zu B of LDS > 160 KiB", lds);
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(wg_mpc_assemble_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // the scratch copies of the states are the context's: assemble launches of one context are ordered like its tick / run launches
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  if (int rc = slot_claim(ctx, ctx->asm_order, st, "assemble")) return rc;
  if (int rc = ctx->asm_state.reserve((size_t)B * sizeof(wg_gait_state_t))) return rc;
  hipLaunchKernelGGL(wg_mpc_assemble_kernel, dim3(B), dim3(64), lds, st, B, ctx->model,
                     ctx->tables_dev, states, static_cast<wg_gait_state_t *>(ctx->asm_state.p), advance_calls, (unsigned)qlb, nmax, mmax,
                     C, d, A, b, xl, xu, n, m);
  HIP_TRY(hipGetLastError());
  return slot_mark(ctx->asm_order, st);
}

int wg_mpc_assemble_batch_ctx(wg_ctx_t *ctx, int B, const wg_gait_state_t *states, int advance_calls, int nmax, int mmax, double *C, double *d, double *A, double *b, double *xl, double *xu, int *n, int *m) {
  if (int rc = use_ctx(ctx)) return rc;
  if (B < 0 || !states || !C || !d || !A || !b || !xl || !xu || !n || !m || nmax <= 0 || mmax <= 0) return fail(WG_ERR_BAD_ARG, "bad arguments");
  if (B == 0) return WG_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HostScope hs(ctx);
  const size_t sB = (size_t)B, sn = (size_t)nmax, sm = (size_t)mmax;
  Arena a(ctx->in);
  const auto s_st = a.take<wg_gait_state_t>(sB);
  const auto sC = a.take<double>(sB * sn * sn), sd = a.take<double>(sB * sn), sA = a.take<double>(sB * sm * sn), sb = a.take<double>(sB * sm),
             sxl = a.take<double>(sB * sn), sxu = a.take<double>(sB * sn);
  const auto s_n = a.take<int>(sB), s_m = a.take<int>(sB);
  if (int rc = a.reserve()) return rc;
  WG_H2D(a(s_st), states, s_st.bytes());
  if (int rc = wg_mpc_assemble_batch_dev_ctx(ctx, B, a(s_st), advance_calls, nmax, mmax, a(sC), a(sd), a(sA), a(sb), a(sxl), a(sxu), a(s_n), a(s_m),
                                             hs.stream()))
    return rc;
  WG_D2H(C, a(sC), sC.bytes());
  WG_D2H(d, a(sd), sd.bytes());
  WG_D2H(A, a(sA), sA.bytes());
  WG_D2H(b, a(sb), sb.bytes());
  WG_D2H(xl, a(sxl), sxl.bytes());
  WG_D2H(xu, a(sxu), sxu.bytes());
  WG_D2H(n, a(s_n), s_n.bytes());
  WG_D2H(m, a(s_m), s_m.bytes());
  WG_HOST_WAIT();
  return WG_OK;
}

}  // extern "C"
namespace {
int run_launch(wg_ctx_t *ctx, const wg_mpc_fleet_t *fl, int B, wg_gait_state_t *states, int n_ticks, int advance_calls, const double *vref_sched, int period, wg_tick_out_t *outs, int *diag, void *hip_stream);
}
extern "C" {
int wg_mpc_run_batch_dev_ctx(wg_ctx_t *ctx, int B, wg_gait_state_t *states, int n_ticks, int advance_calls, wg_tick_out_t *outs, int *diag, void *hip_stream) {
  return wg_mpc_run_sched_dev_ctx(ctx, B, states, n_ticks, advance_calls, nullptr, 1, outs, diag, hip_stream);
}

int wg_mpc_run_sched_dev_ctx(wg_ctx_t *ctx, int B, wg_gait_state_t *states, int n_ticks, int advance_calls, const double *vref_sched, int period, wg_tick_out_t *outs, int *diag, void *hip_stream) {
  return run_launch(ctx, nullptr, B, states, n_ticks, advance_calls, vref_sched, period, outs, diag, hip_stream);
}

}  // extern "C"
namespace {
// fl == nullptr: the context's configured model; otherwise a model per gait, always with the hand-over inside an XCD
int run_launch(wg_ctx_t *ctx, const wg_mpc_fleet_t *fl, int B, wg_gait_state_t *states, int n_ticks, int advance_calls, const double *vref_sched, int period, wg_tick_out_t *outs, int *diag, void *hip_stream) {
  if (fl) { if (int rc = mpc_fleet_check(ctx, B, fl, states)) return rc; }
  else {
    if (int rc = use_ctx(ctx)) return rc;
    if (!ctx->model_set) return fail(WG_ERR_BAD_ARG, "wg_mpc_configure() has not been called on this context");
  }
  if (B < 0 || n_ticks < 0 || !states || period < 1) return fail(WG_ERR_BAD_ARG, "bad arguments");
  if (B == 0 || n_ticks == 0) return WG_OK;
  if (vref_sched && !fl && !run_queue_xcd()) {              // the device-wide queue of round 1 has no staged form: one launch per stretch
    for (int t = 0; t < n_ticks; t += period) {
      const int n = n_ticks - t < period ? n_ticks - t : period;
      if (int rc = wg_mpc_set_velref_dev_ctx(ctx, B, states, vref_sched + (size_t)(t / period) * B * 3, hip_stream)) return rc;
      if (int rc = wg_mpc_run_sched_dev_ctx(ctx, B, states, n, advance_calls, nullptr, 1, outs ? outs + (size_t)t * B : nullptr,
                                            diag ? diag + (size_t)t * B * 6 : nullptr, hip_stream))
        return rc;
    }
    return WG_OK;
  }
  if ((long long)B * n_ticks > 0x3fffffffLL) return fail(WG_ERR_TOO_LARGE, "B * n_ticks = %lld work items", (long long)B * n_ticks);
  const int total = B * n_ticks;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);   // ordering test, launch and event record are one critical section
  if (int rc = slot_claim(ctx, ctx->guard_order, st, "tick / run")) return rc;
  const bool xcd_mode = fl || run_queue_xcd();
  const int cap = run_ring_cap(B);
  if (int rc = ctx->run_buf.reserve(xcd_mode ? run_buf_bytes(B) : sizeof(wg_run_queue) + (size_t)(total + B) * 4)) return rc;
  wg_run_queue *q = static_cast<wg_run_queue *>(ctx->run_buf.p);
  int *ring = reinterpret_cast<int *>(q + 1), *done = ring + total;
  wg_xrun_ctl *xctl = static_cast<wg_xrun_ctl *>(ctx->run_buf.p);
  unsigned long long *xrings = reinterpret_cast<unsigned long long *>(xctl + 1);
  int *xdone = reinterpret_cast<int *>(xrings + (size_t)kXcds * cap);
  if (xcd_mode) {
    const int items = kXcds * cap > B ? kXcds * cap : B;
    hipLaunchKernelGGL(wg_xrun_init_kernel, dim3((items + 255) / 256), dim3(256), 0, st, B, xctl, xrings, cap, xdone);
  } else
    hipLaunchKernelGGL(wg_run_queue_init_kernel, dim3((total + 255) / 256), dim3(256), 0, st, B, total, q, ring, done);
  const TickPlan plan(fl ? fl->base : ctx->model);
  if (fl) { if (int rc = plan.raise_lds(WG_KERNEL_BY_VIEW(wg_mpc_run_xcd_fleet_kernel, plan.view))) return rc; }
  else {
    if (int rc = plan.raise_lds(WG_KERNEL_BY_VIEW(wg_mpc_run_kernel, plan.view))) return rc;
    if (int rc = plan.raise_lds(WG_KERNEL_BY_VIEW(wg_mpc_run_xcd_kernel, plan.view))) return rc;
  }
  // as many blocks as the device keeps resident: LDS granules, and the waves the kernel's register budget admits per CU
  int grid = ctx->num_cu * plan.per_cu();
  if (grid > B) grid = B;
  double *zs = nullptr;
  if (int rc = plan.reserve_slots(ctx, grid, &zs)) return rc;
  int keep_k = 0;                                    // a wave keeps a gait that is behind its XCD's mean progress (see the kernel)
  if (const char *e = getenv("WG_RUN_KEEP")) keep_k = (e[0] == 'o' || e[0] == '-') ? -1 : atoi(e);
  else if (B <= grid) keep_k = -1;                   // a wave per gait: nothing waits, the launch takes what its slowest gait takes
  if (fl)
    WG_LAUNCH_BY_VIEW(wg_mpc_run_xcd_fleet_kernel, plan.view, grid, plan.launch_lds, st, B, n_ticks, fl->base.N, fl->base.T, fl->base.Tctrl, fl->M,
                      static_cast<const unsigned char *>(fl->blocks), fl->model_of, states, outs, diag, advance_calls, xctl, xrings, cap, xdone,
                      (unsigned)plan.qlb, zs, (unsigned)plan.zslot, vref_sched, period, plan.ecap, keep_k);
  else if (xcd_mode)
    WG_LAUNCH_BY_VIEW(wg_mpc_run_xcd_kernel, plan.view, grid, plan.launch_lds, st, B, n_ticks, ctx->model_dev, ctx->tables_dev, states, outs, diag,
                      advance_calls, xctl, xrings, cap, xdone, (unsigned)plan.qlb, zs, (unsigned)plan.zslot, vref_sched, period, plan.ecap, keep_k);
  else
    WG_LAUNCH_BY_VIEW(wg_mpc_run_kernel, plan.view, grid, plan.launch_lds, st, B, n_ticks, ctx->model_dev, ctx->tables_dev, states, outs, diag,
                      advance_calls, q, ring, done, (unsigned)plan.qlb, zs, (unsigned)plan.zslot, plan.ecap);
  HIP_TRY(hipGetLastError());
  return slot_mark(ctx->guard_order, st);
}
}  // namespace
extern "C" {

// the launches of wg_mpc_tick_batch_dev and wg_mpc_run_sched_dev with blocks[model_of[g]] as gait g's model: the same launcher
// code, the context's slots, run buffer, launch ordering and start order; nothing of the context's configured model is read
int wg_mpc_tick_fleet_dev_ctx(wg_ctx_t *ctx, int B, const wg_mpc_fleet_t *fleet, wg_gait_state_t *states, wg_tick_out_t *outs, int *diag, int advance_calls, int *hist, int hist_cap, int *hist_len, void *hip_stream) {
  if (!fleet) return fail(WG_ERR_BAD_ARG, "null fleet");
  return tick_launch(ctx, B, states, outs, diag, advance_calls, hist, hist_cap, hist_len, hip_stream, nullptr, nullptr, fleet);
}
int wg_mpc_run_fleet_dev_ctx(wg_ctx_t *ctx, int B, const wg_mpc_fleet_t *fleet, wg_gait_state_t *states, int n_ticks, int advance_calls, const double *vref_sched, int period, wg_tick_out_t *outs, int *diag, void *hip_stream) {
  if (!fleet) return fail(WG_ERR_BAD_ARG, "null fleet");
  return run_launch(ctx, fleet, B, states, n_ticks, advance_calls, vref_sched, period, outs, diag, hip_stream);
}

// one wave per model (wg_tick_kernels.hpp); the host twin is wg_mpc_block, the arithmetic wg_tick_tables_math.hpp
int wg_mpc_blocks_batch_dev_ctx(wg_ctx_t *ctx, int M, const wg_model_t *models, void *blocks, int *status, void *hip_stream) {
  if (M < 0 || (M > 0 && (!models || !blocks || !status))) return fail(WG_ERR_BAD_ARG, "M = %d, or a NULL models, blocks or status", M);
  int knobs = 0;
  if (int rc = tick_ql_knobs(&knobs)) return rc;
  if (int rc = use_ctx(ctx)) return rc;
  if (M == 0) return WG_OK;
  hipLaunchKernelGGL(wg_mpc_blocks_kernel, dim3(M), dim3(64), 0, reinterpret_cast<hipStream_t>(hip_stream), M, models,
                     static_cast<unsigned char *>(blocks), status, knobs);
  HIP_TRY(hipGetLastError());
  return WG_OK;
}

// host pointers
int wg_mpc_blocks_batch_ctx(wg_ctx_t *ctx, int M, const wg_model_t *models, void *blocks, int *status) {
  if (M < 0 || (M > 0 && (!models || !blocks || !status))) return fail(WG_ERR_BAD_ARG, "M = %d, or a NULL models, blocks or status", M);
  if (int rc = use_ctx(ctx)) return rc;
  if (M == 0) return WG_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HostScope hs(ctx);
  Arena a(ctx->tick_aux);
  const auto sm = a.take<wg_model_t>((size_t)M);
  const auto sk = a.take<unsigned char>((size_t)M * wg::kMpcBlockBytes);
  const auto ss = a.take<int>((size_t)M);
  if (int rc = a.reserve()) return rc;
  WG_H2D(a(sm), models, sm.bytes());
  if (int rc = wg_mpc_blocks_batch_dev_ctx(ctx, M, a(sm), a(sk), a(ss), hs.stream())) return rc;
  WG_D2H(blocks, a(sk), sk.bytes());
  WG_D2H(status, a(ss), ss.bytes());
  WG_HOST_WAIT();
  return WG_OK;
}

int wg_mpc_tick_batch_ctx(wg_ctx_t *ctx, int B, wg_gait_state_t *states, wg_tick_out_t *outs, int *diag, int advance_calls, int *hist, int hist_cap, int *hist_len) {
  if (int rc = tick_check(ctx, B, states)) return rc;
  if (B == 0) return WG_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HostScope hs(ctx);
  const size_t sB = (size_t)B;
  if (int rc = ctx->tick_state.reserve(sB * sizeof(wg_gait_state_t))) return rc;
  if (outs) if (int rc = ctx->tick_out.reserve(sB * sizeof(wg_tick_out_t))) return rc;
  Arena aux(ctx->tick_aux);
  const auto s_diag = aux.take<int>(sB * 6), s_hist = aux.take<int>(hist ? sB * hist_cap : 0), s_hlen = aux.take<int>(hist ? sB : 0);
  if (int rc = aux.reserve()) return rc;
  wg_gait_state_t *d_states = static_cast<wg_gait_state_t *>(ctx->tick_state.p);
  wg_tick_out_t *d_outs = outs ? static_cast<wg_tick_out_t *>(ctx->tick_out.p) : nullptr;
  WG_H2D(d_states, states, sB * sizeof(wg_gait_state_t));
  WG_ZERO(ctx->tick_aux.p, aux.size);
  if (int rc = wg_mpc_tick_batch_dev_ctx(ctx, B, d_states, d_outs, aux(s_diag), advance_calls, aux(s_hist), hist_cap, aux(s_hlen), hs.stream()))
    return rc;
  WG_D2H(states, d_states, sB * sizeof(wg_gait_state_t));
  if (outs) WG_D2H(outs, d_outs, sB * sizeof(wg_tick_out_t));
  if (diag) WG_D2H(diag, aux(s_diag), s_diag.bytes());
  if (hist) {
    WG_D2H(hist, aux(s_hist), s_hist.bytes());
    WG_D2H(hist_len, aux(s_hlen), s_hlen.bytes());
  }
  WG_HOST_WAIT();
  return WG_OK;
}

int wg_mpc_set_velref_dev_ctx(wg_ctx_t *ctx, int B, wg_gait_state_t *states, const double *vref, void *hip_stream) {
  if (int rc = use_ctx(ctx)) return rc;
  if (B < 0 || !states || !vref) return fail(WG_ERR_BAD_ARG, "bad arguments");
  if (B == 0) return WG_OK;
  hipLaunchKernelGGL(wg_set_velref_kernel, dim3((B + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream),
                     B, states, vref);
  HIP_TRY(hipGetLastError());
  return WG_OK;
}

}  // extern "C"

// ---- PLDP / OptCholesky back-end -----------------------------------------------------------------------------------

namespace {
int pldp_check(wg_ctx *ctx, int B, int mcap, const int *m, const double *D, const double *A, const double *b, const double *zmpref, const double *xkyk, const int *similar, const int *n_removed, const int *starting, const wg_pldp_state_t *states, const double *X, const int *ret) {
  if (int rc = use_ctx(ctx)) return rc;
  if (!ctx->pldp_N) return fail(WG_ERR_BAD_ARG, "wg_pldp_configure() has not been called on this context");
  if (B < 0 || mcap < 1 || mcap > WG_PLDP_MMAX) return fail(WG_ERR_BAD_ARG, "need 1 <= mcap <= %d", WG_PLDP_MMAX);
  if (!m || !D || !A || !b || !zmpref || !xkyk || !similar || !n_removed || !starting || !states || !X || !ret)
    return fail(WG_ERR_BAD_ARG, "null argument");
  return WG_OK;
}
}  // namespace

extern "C" {

size_t wg_pldp_lds_bytes(void) { return wg::PldpLds::bytes(WG_PLDP_MMAX); }

int wg_pldp_configure_ctx(wg_ctx_t *ctx, int N, const double *iPu, const double *Px, const double *Pu) {
  if (int rc = use_ctx(ctx)) return rc;
  if (N < 1 || N > WG_PLDP_N || !iPu || !Px || !Pu) return fail(WG_ERR_BAD_ARG, "wg_pldp_configure: 1 <= N <= %d", WG_PLDP_N);
  std::unique_ptr<wg::PldpModel> host_p(new wg::PldpModel);
  wg::PldpModel &host = *host_p;
  std::lock_guard<std::mutex> lk(ctx->mu);
  memset(&host, 0, sizeof host);
  host.N = N;
  memcpy(host.iPu, iPu, sizeof(double) * N * N);
  memcpy(host.Pu, Pu, sizeof(double) * N * N);
  memcpy(host.Px, Px, sizeof(double) * N * 3);
  // PLDPSolver::PrecomputeiPuPx, PLDPSolver.cpp:263-283 (block diagonal, k ascending)
  for (int i = 0; i < N; i++)
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
      for (int k = 0; k < N; k++) s += iPu[k * N + i] * Px[k * 3 + j];
      host.iPuPx[i * 6 + j] = s;
      host.iPuPx[(i + N) * 6 + j + 3] = s;
    }
  if (!ctx->pldp_dev) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->pldp_dev), sizeof(wg::PldpModel)));
  if (int rc = ctx_wait_own(ctx)) return rc;             // a solve of the previous model may still be reading it
  HostScope hs(ctx);
  WG_H2D(ctx->pldp_dev, &host, sizeof host);
  WG_HOST_WAIT();
  ctx->pldp_N = N;
  return WG_OK;
}

int wg_pldp_solve_batch_dev_ctx(wg_ctx_t *ctx, int B, int mcap, const int *m, const double *D, const double *A, const double *b, const double *zmpref, const double *xkyk, const int *similar, const int *n_removed, const int *starting, int max_iter, wg_pldp_state_t *states, double *X, int *ret, int *n_iter, int *active, int *n_active, void *hip_stream) {
  if (int rc = pldp_check(ctx, B, mcap, m, D, A, b, zmpref, xkyk, similar, n_removed, starting, states, X, ret)) return rc;
  if (B == 0) return WG_OK;
  // like the dense QP kernel: A in LDS only while that does not cost a resident problem (8 per CU is the useful maximum)
  size_t lds = wg::PldpLds::bytes(mcap);
  const size_t lds_noa = wg::PldpLds::bytes(mcap, WG_PLDP_ACTIVE_CAP, false, false);
  const bool a_in_lds = env_flag("WG_PLDP_A_IN_LDS", per_cu_160k(lds_noa, 8) <= per_cu_160k(lds, 8));   // tests force either path
  if (!a_in_lds) lds = lds_noa;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const auto kern = a_in_lds ? wg_pldp_kernel<true> : wg_pldp_kernel<false>;     // A's place is a template argument
  if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3(B), dim3(64), lds, st, B, mcap, ctx->pldp_dev, m, D, A, b, zmpref, xkyk, similar, n_removed, starting, max_iter,
                     states, X, ret, n_iter, active, n_active);
  HIP_TRY(hipGetLastError());
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  return slot_mark(ctx->aux_order, st);
}

int wg_pldp_solve_batch_ctx(wg_ctx_t *ctx, int B, int mcap, const int *m, const double *D, const double *A, const double *b, const double *zmpref, const double *xkyk, const int *similar, const int *n_removed, const int *starting, int max_iter, wg_pldp_state_t *states, double *X, int *ret, int *n_iter, int *active, int *n_active) {
  if (int rc = pldp_check(ctx, B, mcap, m, D, A, b, zmpref, xkyk, similar, n_removed, starting, states, X, ret)) return rc;
  if (B == 0) return WG_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HostScope hs(ctx);
  const size_t sB = (size_t)B, n = 2 * (size_t)ctx->pldp_N;
  Arena a(ctx->pldp_buf);
  const auto sD = a.take<double>(sB * n), sA = a.take<double>(sB * (mcap + 1) * n), sb = a.take<double>(sB * mcap), sz = a.take<double>(sB * n),
             sx = a.take<double>(sB * 6), sX = a.take<double>(sB * n);
  const auto sst = a.take<wg_pldp_state_t>(sB);
  const auto sm = a.take<int>(sB), ssim = a.take<int>(sB * mcap), snr = a.take<int>(sB), sstart = a.take<int>(sB);
  const auto sret = a.take<int>(sB), sit = a.take<int>(sB), sact = a.take<int>(sB * mcap), snact = a.take<int>(sB);   // the outputs: last, zeroed
  if (int rc = a.reserve()) return rc;
  WG_H2D(a(sD), D, sD.bytes());
  WG_H2D(a(sA), A, sA.bytes());
  WG_H2D(a(sb), b, sb.bytes());
  WG_H2D(a(sz), zmpref, sz.bytes());
  WG_H2D(a(sx), xkyk, sx.bytes());
  WG_H2D(a(sst), states, sst.bytes());
  WG_H2D(a(sm), m, sm.bytes());
  WG_H2D(a(ssim), similar, ssim.bytes());
  WG_H2D(a(snr), n_removed, snr.bytes());
  WG_H2D(a(sstart), starting, sstart.bytes());
  WG_ZERO(a(sret), a.size - sret.off);
  if (int rc = wg_pldp_solve_batch_dev_ctx(ctx, B, mcap, a(sm), a(sD), a(sA), a(sb), a(sz), a(sx), a(ssim), a(snr), a(sstart), max_iter, a(sst), a(sX),
                                           a(sret), a(sit), a(sact), a(snact), hs.stream()))
    return rc;
  WG_D2H(states, a(sst), sst.bytes());
  WG_D2H(X, a(sX), sX.bytes());
  WG_D2H(ret, a(sret), sret.bytes());
  if (n_iter) WG_D2H(n_iter, a(sit), sit.bytes());
  if (active) WG_D2H(active, a(sact), sact.bytes());
  if (n_active) WG_D2H(n_active, a(snact), snact.bytes());
  WG_HOST_WAIT();
  return WG_OK;
}

}  // extern "C"

// ---- Dimitrov-2008 tick around PLDP ------------------------------------------------------------------------------------

namespace {
inline size_t dimitrov_lds_bytes() {
  return wg::PldpLds::bytes(WG_PLDP_MMAX, wg::kDimitrovActiveCap, true) + (4 * 2 * WG_PLDP_N + 8) * 8 +
         ((WG_PLDP_N + 1) * 4 + 15) / 16 * 16;
}
int dimitrov_check(wg_ctx *ctx, int B, const wg_zmp_polytope_t *polys, const wg_dimitrov_state_t *states) {
  if (int rc = use_ctx(ctx)) return rc;
  if (!ctx->dim_set) return fail(WG_ERR_BAD_ARG, "wg_dimitrov_configure() has not been called on this context");
  if (B < 0 || !polys || !states) return fail(WG_ERR_BAD_ARG, "bad arguments");
  return WG_OK;
}

// one tick launch of the form the two bindings name (wg_dimitrov_kernels.hpp); with ctx->launch_mu held.  The plain form goes by the
// name and the arguments it is timed by, every other form is an instantiation of the form kernels.
template <class Model, class Row>
int dimitrov_launch_form(wg_ctx *ctx, int solver, int B, Model Mo, Row Ro, const wg_zmp_polytope_t *polys, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int max_iter, hipStream_t stq) {
  constexpr bool plain = std::is_same<Model, DimOneModel>::value && std::is_same<Row, DimOwnRow>::value;
  constexpr bool follows = std::is_same<Row, DimFollowRow>::value;
  if (solver != WG_DIMITROV_PLDP) {                      // modes QLD / QLDANDLQ: the in-wave ql0002 as the back-end
    const size_t ldsq = wg::dimitrov_qld_lds_bytes();
    const bool lq = solver == WG_DIMITROV_QLDANDLQ;
    // more gaits than resident waves (eight per CU: 256 registers, two waves per SIMD): longest-solve-first by the previous tick
    // on the same state array (scheduling only).  The order lives in a buffer of the context: not while another stream's launch
    // of this context may still be reading it
    int *order = nullptr, *iters_out = nullptr;
    if ((size_t)B > (size_t)ctx->num_cu * per_cu_granules(ldsq, 8) && !slot_pending_elsewhere(ctx->aux_order, stq) && env_flag("WG_QL_LPT", true)) {
      // a follow launch writes the counts of the gaits that go only: the others keep their last one, which a fresh buffer has not
      const bool fresh = follows && !(ctx->dim_lpt.key == states && ctx->dim_lpt.B == B && ctx->dim_lpt.buf.p);
      if (int rc = lpt_prepare(ctx->dim_lpt, states, B, stq, &order, &iters_out)) return rc;
      if (fresh) HIP_TRY(hipMemsetAsync(iters_out, 0, (size_t)B * sizeof(int), stq));
    }
    if constexpr (plain) {
      if (int rc = launch_lds(lq ? wg_dimitrov_qld_tick_kernel<true> : wg_dimitrov_qld_tick_kernel<false>, dim3(B), dim3(64), ldsq, stq, B, Mo.K, polys, states, outs, order, iters_out)) return rc;
    } else {
      if (int rc = launch_lds(lq ? wg_dimitrov_qld_tick_form_kernel<true, Model, Row> : wg_dimitrov_qld_tick_form_kernel<false, Model, Row>, dim3(B), dim3(64), ldsq, stq, B, Mo, polys, states, outs, Ro, order, iters_out)) return rc;
    }
  } else if constexpr (plain) {
    if (int rc = launch_lds(wg_dimitrov_tick_kernel, dim3(B), dim3(64), dimitrov_lds_bytes(), stq, B, Mo.K, polys, states, outs, max_iter)) return rc;
  } else {
    if (int rc = launch_lds(wg_dimitrov_tick_form_kernel<Model, Row>, dim3(B), dim3(64), dimitrov_lds_bytes(), stq, B, Mo, polys, states, outs, Ro, max_iter)) return rc;
  }
  return slot_mark(ctx->aux_order, stq);
}

// the tick launch of wg_dimitrov_tick_batch_dev and of every tick of wg_dimitrov_walk_dev.  With `row` (wg_dimitrov_follow_dev): gait g
// writes row row[g] of outs, or sits the launch out.  With `fl` (the wg_dimitrov_*_fleet_dev calls): gait g binds
// blocks[model_of[g]] where the others bind the context's one model, of which nothing is read.
int dimitrov_tick_launch(wg_ctx *ctx, int B, const wg_zmp_polytope_t *polys, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int max_iter, hipStream_t stq, const int *row = nullptr, const wg_dimitrov_fleet_t *fl = nullptr) {
  auto go = [&](int solver, auto Mo) {
    return row ? dimitrov_launch_form(ctx, solver, B, Mo, DimFollowRow{row}, polys, states, outs, max_iter, stq)
               : dimitrov_launch_form(ctx, solver, B, Mo, DimOwnRow{}, polys, states, outs, max_iter, stq);
  };
  if (fl) return go(fl->solver, DimFleetModels{fl->N, fl->M, static_cast<const unsigned char *>(fl->blocks), fl->model_of});
  return go(ctx->dim_host->solver, DimOneModel{ctx->dim_dev});
}
}  // namespace

extern "C" {

void wg_dimitrov_defaults(wg_dimitrov_model_t *m) {      // ZMPConstrainedQPFastFormulation.cpp:81-97
  if (!m) return;
  memset(m, 0, sizeof *m);
  m->N = 16; m->T = 0.1; m->Tctrl = 0.005; m->com_height = 0.80; m->alpha = 200.0; m->beta = 1000.0;
}

int wg_dimitrov_configure_ctx(wg_ctx_t *ctx, const wg_dimitrov_model_t *model) {
  if (int rc = use_ctx(ctx)) return rc;
  if (!model) return fail(WG_ERR_BAD_ARG, "null model");
  if (model->N < 1 || model->N > WG_PLDP_N) return fail(WG_ERR_BAD_ARG, "N=%d outside [1,%d]", model->N, WG_PLDP_N);
  if (!(model->T > 0.0) || !(model->Tctrl > 0.0) || (int)(model->T / model->Tctrl) != WG_SAMPLES_PER_TICK)
    return fail(WG_ERR_BAD_ARG, "T/Tctrl must be %d", WG_SAMPLES_PER_TICK);
  if (model->solver != WG_DIMITROV_PLDP && model->solver != WG_DIMITROV_QLD && model->solver != WG_DIMITROV_QLDANDLQ)
    return fail(WG_ERR_BAD_ARG, "solver = %d: WG_DIMITROV_PLDP (0), WG_DIMITROV_QLD (1) or WG_DIMITROV_QLDANDLQ (2)", model->solver);
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->dim_host) ctx->dim_host.reset(new wg::DimitrovConst);
    ctx->dim_set = false;
    if (!wg::DimitrovHost::build(*model, (*ctx->dim_host)))
      return fail(WG_ERR_BAD_ARG, "the LQ factor or the inverse of Pu does not exist for this model");
    if (!ctx->dim_dev) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->dim_dev), sizeof(wg::DimitrovConst)));
    if (int rc = ctx_wait_own(ctx)) return rc;           // a tick of the previous model may still be reading the constants
    HostScope hs(ctx);
    WG_H2D(ctx->dim_dev, &(*ctx->dim_host), sizeof (*ctx->dim_host));
    WG_HOST_WAIT();
    ctx->dim_set = true;
  }
  // the PLDPSolver constructor of the reference (:104-109): same iPu, Px, Pu
  return wg_pldp_configure_ctx(ctx, model->N, (*ctx->dim_host).pldp.iPu, (*ctx->dim_host).pldp.Px, (*ctx->dim_host).pldp.Pu);
}

int wg_dimitrov_get_constants_ctx(wg_ctx_t *ctx, double *iLQ, double *OptB, double *OptC, double *Pu, double *iPu, double *Px) {
  if (!ctx) return fail(WG_ERR_BAD_ARG, "null context");
  if (!ctx->dim_set) return fail(WG_ERR_BAD_ARG, "wg_dimitrov_configure() has not been called on this context");
  const size_t N = (size_t)(*ctx->dim_host).N, n = 2 * N;
  if (iLQ) memcpy(iLQ, (*ctx->dim_host).iLQ, 8 * n * n);
  if (OptB) memcpy(OptB, (*ctx->dim_host).OptB, 8 * n * 6);
  if (OptC) memcpy(OptC, (*ctx->dim_host).OptC, 8 * n * n);
  if (Pu) memcpy(Pu, (*ctx->dim_host).pldp.Pu, 8 * N * N);
  if (iPu) memcpy(iPu, (*ctx->dim_host).pldp.iPu, 8 * N * N);
  if (Px) memcpy(Px, (*ctx->dim_host).pldp.Px, 8 * N * 3);
  return WG_OK;
}

int wg_dimitrov_get_qld_constants_ctx(wg_ctx_t *ctx, double *Q, double *OptB, double *OptC, double *PuT) {
  if (!ctx) return fail(WG_ERR_BAD_ARG, "null context");
  if (!ctx->dim_set) return fail(WG_ERR_BAD_ARG, "wg_dimitrov_configure() has not been called on this context");
  const size_t N = (size_t)(*ctx->dim_host).N, n = 2 * N;
  if (Q) memcpy(Q, (*ctx->dim_host).Qq, 8 * n * n);
  if (OptB) memcpy(OptB, (*ctx->dim_host).OptBq, 8 * n * 6);
  if (OptC) memcpy(OptC, (*ctx->dim_host).OptCq, 8 * n * n);
  if (PuT) memcpy(PuT, (*ctx->dim_host).PuTq, 8 * N * N);
  return WG_OK;
}

int wg_dimitrov_tick_batch_dev_ctx(wg_ctx_t *ctx, int B, const wg_zmp_polytope_t *polys, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int max_iter, void *hip_stream) {
  if (int rc = dimitrov_check(ctx, B, polys, states)) return rc;
  if (B == 0) return WG_OK;
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  return dimitrov_tick_launch(ctx, B, polys, states, outs, max_iter, reinterpret_cast<hipStream_t>(hip_stream));
}

int wg_dimitrov_tick_batch_ctx(wg_ctx_t *ctx, int B, const wg_zmp_polytope_t *polys, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int max_iter) {
  if (int rc = dimitrov_check(ctx, B, polys, states)) return rc;
  if (B == 0) return WG_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HostScope hs(ctx);
  const size_t sB = (size_t)B;
  Arena a(ctx->dim_buf);
  const auto sp = a.take<wg_zmp_polytope_t>(sB * (size_t)ctx->dim_host->N);
  const auto ss = a.take<wg_dimitrov_state_t>(sB);
  const auto so = a.take<wg_dimitrov_out_t>(outs ? sB : 0);
  if (int rc = a.reserve()) return rc;
  WG_H2D(a(sp), polys, sp.bytes());
  WG_H2D(a(ss), states, ss.bytes());
  if (outs) WG_ZERO(a(so), so.bytes());
  if (int rc = wg_dimitrov_tick_batch_dev_ctx(ctx, B, a(sp), a(ss), a(so), max_iter, hs.stream())) return rc;
  WG_D2H(states, a(ss), ss.bytes());
  if (outs) WG_D2H(outs, a(so), so.bytes());
  WG_HOST_WAIT();
  return WG_OK;
}

}  // extern "C"

// ---- Dimitrov fleets on the device: polytope queues, the queue walk of a tick, n ticks on a stream --------------------------

namespace {
int queue_check(int B, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count) {
  if (B < 0 || qcap < 1 || !queues || !t_start || !t_end || !count) return fail(WG_ERR_BAD_ARG, "need B >= 0, qcap >= 1, non-null queues, intervals and counts");
  return WG_OK;
}
int select_check(wg_ctx *ctx, int B, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count) {
  if (int rc = use_ctx(ctx)) return rc;
  if (!ctx->dim_set) return fail(WG_ERR_BAD_ARG, "wg_dimitrov_configure() has not been called on this context");
  return queue_check(B, qcap, queues, t_start, t_end, count);
}
void select_launch(int N, double T, int B, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, double t0, wg_zmp_polytope_t *polys, int *ran_out, int sticky, hipStream_t st) {
  hipLaunchKernelGGL(wg::wg_dimitrov_select_kernel, dim3((B + 3) / 4), dim3(256), 0, st, B, qcap, queues, t_start, t_end, count, t0,
                     N, T, polys, ran_out, sticky);
}

// the launches of wg_dimitrov_walk_dev (fl == nullptr: N, T and the ticks' model are the context's) and of
// wg_dimitrov_walk_fleet_dev (the fleet's); the arguments are checked
int dimitrov_walk_launch(wg_ctx *ctx, const wg_dimitrov_fleet_t *fl, int B, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, double t0, int n_ticks, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int *ran_out, int max_iter, void *hip_stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int Ni = fl ? fl->N : ctx->dim_host->N;
  const size_t N = (size_t)Ni;
  const double T = fl ? fl->T : ctx->dim_host->T;
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  // the selected polytopes live in a buffer of the context, rewritten tick by tick: behind the previous walk, whatever stream
  // that was on; growing retires the old allocation, which a launch in flight may still be reading (DevBuf)
  if (int rc = slot_claim(ctx, ctx->walk_order, st, "Dimitrov walk")) return rc;
  if (int rc = ctx->walk_polys.reserve((size_t)B * N * sizeof(wg_zmp_polytope_t))) return rc;
  wg_zmp_polytope_t *polys = static_cast<wg_zmp_polytope_t *>(ctx->walk_polys.p);
  if (ran_out) HIP_TRY(hipMemsetAsync(ran_out, 0, (size_t)B * sizeof(int), st));
  double t = t0;
  for (int k = 0; k < n_ticks; k++) {
    select_launch(Ni, T, B, qcap, queues, t_start, t_end, count, t, polys, ran_out, 1, st);
    HIP_TRY(hipGetLastError());
    if (int rc = dimitrov_tick_launch(ctx, B, polys, states, outs ? outs + (size_t)k * (size_t)B : nullptr, max_iter, st, nullptr, fl)) return rc;
    t += T;                                               // BuildZMPTrajectoryFromFootTrajectory's own accumulation (:1189-1192)
  }
  return slot_mark(ctx->walk_order, st);
}

// likewise wg_dimitrov_follow_dev and wg_dimitrov_follow_fleet_dev
int dimitrov_follow_launch(wg_ctx *ctx, const wg_dimitrov_fleet_t *fl, int B, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, int lcap, const double *time, const int *have, const wg_zmpdisc_state_t *walk, int flags, double *clock, int *ticks, int tick_cap, int max_ticks, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int *ran_out, int max_iter, void *hip_stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int N = fl ? fl->N : ctx->dim_host->N;
  const double T = fl ? fl->T : ctx->dim_host->T;
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  if (int rc = slot_claim(ctx, ctx->walk_order, st, "Dimitrov walk")) return rc;
  Arena a(ctx->walk_polys);
  const auto sp = a.take<wg_zmp_polytope_t>((size_t)B * (size_t)N);
  const auto sr = a.take<int>((size_t)B);
  if (int rc = a.reserve()) return rc;
  for (int k = 0; k < max_ticks; k++) {
    hipLaunchKernelGGL(wg::wg_dimitrov_follow_select_kernel, dim3((B + 3) / 4), dim3(256), 0, st, B, qcap, queues, t_start, t_end, count,
                       lcap, time, have, walk, flags & WG_DIMITROV_FOLLOW_ALL_FINAL, clock, ticks, tick_cap, N, T, a(sp), ran_out, a(sr));
    HIP_TRY(hipGetLastError());
    if (int rc = dimitrov_tick_launch(ctx, B, a(sp), states, outs, max_iter, st, a(sr), fl)) return rc;
  }
  return slot_mark(ctx->walk_order, st);
}
int follow_args_check(int lcap, const double *time, const int *have, int flags, const double *clock, const int *ticks, int tick_cap, int max_ticks, const wg_dimitrov_state_t *states) {
  if (lcap < 1 || tick_cap < 0 || max_ticks < 0 || !time || !have || !clock || !ticks || !states)
    return fail(WG_ERR_BAD_ARG, "need lcap >= 1, tick_cap >= 0, max_ticks >= 0, non-null time, have, clock, ticks and states");
  if (flags & ~WG_DIMITROV_FOLLOW_ALL_FINAL) return fail(WG_ERR_BAD_ARG, "flags = %#x: WG_DIMITROV_FOLLOW_ALL_FINAL (1) is the only flag", flags);
  return WG_OK;
}

// What wg_foot_constraints_batch_dev (res = false: first_sample 0, no done) and _append_dev (res = true) share: the checks, the
// half sole, the kernels' arguments, the chunks from first_sample's on, the claim of the context's buffer -- the per-chunk counts
// live there between the two passes (and two ints per gait behind them for a resumed call): one launch at a time uses it --
// and the mark behind the launches, which `passes` issues.
template <class Passes>
int footcons_launch(wg_ctx *ctx, bool res, int B, int lcap, int first_sample, const int *done, const int *length, const double *time, const double *left_tm, const int *left_type_tm, const double *right_tm, double sole_w, double sole_h, double constraint_x, double constraint_y, int qcap, wg_zmp_polytope_t *queues, double *t_start, double *t_end, int *count, void *hip_stream, Passes passes) {
  if (int rc = use_ctx(ctx)) return rc;
  if (B < 0 || qcap < 0 || first_sample < 0) return fail(WG_ERR_BAD_ARG, res ? "need B >= 0, qcap >= 0, first_sample >= 0" : "need B >= 0, qcap >= 0");
  if (B == 0) return WG_OK;
  if (qcap > 0 && (!queues || !t_start || !t_end)) return fail(WG_ERR_BAD_ARG, "need non-null queues and intervals for qcap > 0");
  if (lcap < 1 || (res && !done) || !length || !time || !left_tm || !left_type_tm || !right_tm || !count)
    return fail(WG_ERR_BAD_ARG, "need lcap >= 1, non-null %slengths, times, feet arrays and counts", res ? "done, " : "");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  double hw = sole_w * 0.5, hh = sole_h * 0.5;
  hh -= constraint_y;
  hw -= constraint_x;
  const wg::FcIn I{B, lcap, length, time, left_tm, right_tm, left_type_tm, hw, hh};
  const wg::FcOut Q{qcap, queues, t_start, t_end, count};
  const int chunk0 = first_sample / wg::kFcChunk, chunks = (lcap + wg::kFcChunk - 1) / wg::kFcChunk - chunk0;
  if (chunks > 65535) {
    if (res) return fail(WG_ERR_TOO_LARGE, "lcap = %d, first_sample = %d: more than 65535 chunks of %d samples", lcap, first_sample, wg::kFcChunk);
    return fail(WG_ERR_TOO_LARGE, "lcap = %d: more than 65535 chunks of %d samples", lcap, wg::kFcChunk);
  }
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  if (int rc = slot_claim(ctx, ctx->fc_order, st, "foot-constraints")) return rc;
  const size_t sB = (size_t)B, n_cnt = (size_t)(chunks > 0 ? chunks : 0) * sB;
  if (int rc = ctx->fc_buf.reserve((n_cnt + (res ? 2 * sB : 0)) * sizeof(int))) return rc;
  if (int rc = passes(I, Q, static_cast<int *>(ctx->fc_buf.p), n_cnt, chunk0, chunks, st)) return rc;
  HIP_TRY(hipGetLastError());
  return slot_mark(ctx->fc_order, st);
}

// The two calls, each in its two forms: kFleet = false with the launch's sole (S is empty), kFleet = true with a sole per gait in
// S.soles (`sole` is then unused: the kernels make hw, hh in the gait's lane).
template <bool kFleet>
int footcons_batch(wg_ctx *ctx, int B, int lcap, const int *length, const double *time, const double *left_tm, const int *left_type_tm, const double *right_tm, const wg_sole_t &sole, wg::FcSoles<kFleet> S, int qcap, wg_zmp_polytope_t *queues, double *t_start, double *t_end, int *count, void *hip_stream) {
  return footcons_launch(ctx, false, B, lcap, 0, nullptr, length, time, left_tm, left_type_tm, right_tm, sole.sole_w, sole.sole_h, sole.constraint_x, sole.constraint_y, qcap, queues, t_start, t_end, count, hip_stream,
                         [&](const wg::FcIn &I, const wg::FcOut &Q, int *cnt, size_t, int, int chunks, hipStream_t st) -> int {
    const dim3 grid((B + 63) / 64, chunks);
    HIP_TRY(hipMemsetAsync(count, 0, (size_t)B * sizeof(int), st));
    hipLaunchKernelGGL((wg::wg_footcons_kernel<false, false, kFleet>), grid, dim3(64), 0, st, I, Q, cnt, wg::FcRes{}, S);
    hipLaunchKernelGGL((wg::wg_footcons_kernel<true, false, kFleet>), grid, dim3(64), 0, st, I, Q, cnt, wg::FcRes{}, S);
    return WG_OK;
  });
}

template <bool kFleet>
int footcons_append(wg_ctx *ctx, int B, int lcap, int first_sample, int *done, const int *length, const double *time, const double *left_tm, const int *left_type_tm, const double *right_tm, const wg_sole_t &sole, wg::FcSoles<kFleet> S, int qcap, wg_zmp_polytope_t *queues, double *t_start, double *t_end, int *count, void *hip_stream) {
  // chunks that lie wholly below first_sample hold no new sample of any gait: not launched (a gait whose done[b] is below it
  // is refused on the device).  first_sample >= lcap: every gait sits out or is refused, the first kernel alone says so.
  // done[b] / count[b] as they were on entry live behind the per-chunk counts
  return footcons_launch(ctx, true, B, lcap, first_sample, done, length, time, left_tm, left_type_tm, right_tm, sole.sole_w, sole.sole_h, sole.constraint_x, sole.constraint_y, qcap, queues, t_start, t_end, count, hip_stream,
                         [&](const wg::FcIn &I, const wg::FcOut &Q, int *cnt, size_t n_cnt, int chunk0, int chunks, hipStream_t st) -> int {
    int *from = cnt + n_cnt, *base = from + (size_t)B;
    hipLaunchKernelGGL(wg::wg_footcons_resume_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, lcap, first_sample, length, done, count, from, base);
    if (chunks > 0) {
      const wg::FcRes Z{from, base, done, chunk0};
      const dim3 grid((B + 63) / 64, chunks);
      hipLaunchKernelGGL((wg::wg_footcons_kernel<false, true, kFleet>), grid, dim3(64), 0, st, I, Q, cnt, Z, S);
      hipLaunchKernelGGL((wg::wg_footcons_kernel<true, true, kFleet>), grid, dim3(64), 0, st, I, Q, cnt, Z, S);
    }
    return WG_OK;
  });
}
// What wg_zmp_audit_dev (res = false: first_sample 0, no done) and _append_dev (res = true) share: the checks, the kernels'
// arguments, the chunks from first_sample's on, the claim of the context's buffer -- the per-chunk partial results live there
// between the two kernels: one launch at a time uses it -- and the mark behind the launches.
template <bool kRes>
int audit_launch(wg_ctx *ctx, int B, int lcap, int first_sample, int *done, const int *length, const double *time, const double *px_tm, const double *py_tm, long long pitch, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, wg_zmp_audit_t *audit, double *margin_tm, void *hip_stream) {
  if (int rc = use_ctx(ctx)) return rc;
  if (B < 0 || lcap < 1 || qcap < 1 || first_sample < 0) return fail(WG_ERR_BAD_ARG, kRes ? "need B >= 0, lcap >= 1, qcap >= 1, first_sample >= 0" : "need B >= 0, lcap >= 1, qcap >= 1");
  if (B == 0) return WG_OK;
  if ((kRes && !done) || !length || !time || !px_tm || !py_tm || !queues || !t_start || !t_end || !count || !audit)
    return fail(WG_ERR_BAD_ARG, "need non-null %slengths, times, tracks, queues, intervals, counts and audits", kRes ? "done, " : "");
  if (pitch < (long long)B) return fail(WG_ERR_BAD_ARG, "pitch = %lld: the samples of B = %d gaits lie at least B apart", pitch, B);
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int chunk0 = first_sample / wg::kFcChunk, chunks = (lcap + wg::kFcChunk - 1) / wg::kFcChunk - chunk0;
  if (chunks > 65535) return fail(WG_ERR_TOO_LARGE, "lcap = %d, first_sample = %d: more than 65535 chunks of %d samples", lcap, first_sample, wg::kFcChunk);
  const wg::AuIn I{B, lcap, length, time, px_tm, py_tm, pitch, qcap, queues, t_start, t_end, count};
  const wg::AuRes Z{done, first_sample, chunk0};
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  if (int rc = slot_claim(ctx, ctx->audit_order, st, "walk-audit")) return rc;
  const size_t n_part = (size_t)(chunks > 0 ? chunks : 0) * (size_t)B;
  if (int rc = ctx->audit_buf.reserve((n_part ? n_part : 1) * sizeof(wg_zmp_audit_t))) return rc;
  wg_zmp_audit_t *part = static_cast<wg_zmp_audit_t *>(ctx->audit_buf.p);
  // chunks that lie wholly below first_sample hold no new sample of any gait: not launched (a gait whose done[b] is below it
  // is refused on the device).  first_sample >= lcap: every gait sits out or is refused, the combine kernel alone says so.
  if (chunks > 0)
    hipLaunchKernelGGL((wg::wg_zmp_audit_kernel<kRes>), dim3((B + 63) / 64, chunks), dim3(64), 0, st, I, Z, audit, part, margin_tm);
  hipLaunchKernelGGL((wg::wg_zmp_audit_combine_kernel<kRes>), dim3((B + 255) / 256), dim3(256), 0, st, I, Z, part, audit);
  HIP_TRY(hipGetLastError());
  return slot_mark(ctx->audit_order, st);
}
}  // namespace

extern "C" {

int wg_foot_constraints_chunk(void) { return wg::kFcChunk; }

int wg_foot_constraints_batch_dev_ctx(wg_ctx_t *ctx, int B, int lcap, const int *length, const double *time, const double *left_tm, const int *left_type_tm, const double *right_tm, double sole_w, double sole_h, double constraint_x, double constraint_y, int qcap, wg_zmp_polytope_t *queues, double *t_start, double *t_end, int *count, void *hip_stream) {
  return footcons_batch(ctx, B, lcap, length, time, left_tm, left_type_tm, right_tm, wg_sole_t{sole_w, sole_h, constraint_x, constraint_y}, wg::FcSoles<false>{}, qcap, queues, t_start, t_end, count, hip_stream);
}

int wg_foot_constraints_append_dev_ctx(wg_ctx_t *ctx, int B, int lcap, int first_sample, int *done, const int *length, const double *time, const double *left_tm, const int *left_type_tm, const double *right_tm, double sole_w, double sole_h, double constraint_x, double constraint_y, int qcap, wg_zmp_polytope_t *queues, double *t_start, double *t_end, int *count, void *hip_stream) {
  return footcons_append(ctx, B, lcap, first_sample, done, length, time, left_tm, left_type_tm, right_tm, wg_sole_t{sole_w, sole_h, constraint_x, constraint_y}, wg::FcSoles<false>{}, qcap, queues, t_start, t_end, count, hip_stream);
}

int wg_foot_constraints_fleet_dev_ctx(wg_ctx_t *ctx, int B, int lcap, const int *length, const double *time, const double *left_tm, const int *left_type_tm, const double *right_tm, const wg_sole_t *soles, int qcap, wg_zmp_polytope_t *queues, double *t_start, double *t_end, int *count, void *hip_stream) {
  if (!soles) return fail(WG_ERR_BAD_ARG, "null soles");
  return footcons_batch(ctx, B, lcap, length, time, left_tm, left_type_tm, right_tm, wg_sole_t{}, wg::FcSoles<true>{soles}, qcap, queues, t_start, t_end, count, hip_stream);
}

int wg_foot_constraints_append_fleet_dev_ctx(wg_ctx_t *ctx, int B, int lcap, int first_sample, int *done, const int *length, const double *time, const double *left_tm, const int *left_type_tm, const double *right_tm, const wg_sole_t *soles, int qcap, wg_zmp_polytope_t *queues, double *t_start, double *t_end, int *count, void *hip_stream) {
  if (!soles) return fail(WG_ERR_BAD_ARG, "null soles");
  return footcons_append(ctx, B, lcap, first_sample, done, length, time, left_tm, left_type_tm, right_tm, wg_sole_t{}, wg::FcSoles<true>{soles}, qcap, queues, t_start, t_end, count, hip_stream);
}

int wg_zmp_audit_dev_ctx(wg_ctx_t *ctx, int B, int lcap, const int *length, const double *time, const double *px_tm, const double *py_tm, long long pitch, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, wg_zmp_audit_t *audit, double *margin_tm, void *hip_stream) {
  return audit_launch<false>(ctx, B, lcap, 0, nullptr, length, time, px_tm, py_tm, pitch, qcap, queues, t_start, t_end, count, audit, margin_tm, hip_stream);
}

int wg_zmp_audit_append_dev_ctx(wg_ctx_t *ctx, int B, int lcap, int first_sample, int *done, const int *length, const double *time, const double *px_tm, const double *py_tm, long long pitch, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, wg_zmp_audit_t *audit, double *margin_tm, void *hip_stream) {
  return audit_launch<true>(ctx, B, lcap, first_sample, done, length, time, px_tm, py_tm, pitch, qcap, queues, t_start, t_end, count, audit, margin_tm, hip_stream);
}

int wg_dimitrov_select_polys_dev_ctx(wg_ctx_t *ctx, int B, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, double t0, wg_zmp_polytope_t *polys, int *ran_out, void *hip_stream) {
  if (int rc = select_check(ctx, B, qcap, queues, t_start, t_end, count)) return rc;
  if (!polys) return fail(WG_ERR_BAD_ARG, "null polys");
  if (B == 0) return WG_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  select_launch(ctx->dim_host->N, ctx->dim_host->T, B, qcap, queues, t_start, t_end, count, t0, polys, ran_out, 0, st);
  HIP_TRY(hipGetLastError());
  return slot_mark(ctx->aux_order, st);                   // N and T are the configured model's: a re-configuration waits for it
}

int wg_dimitrov_walk_dev_ctx(wg_ctx_t *ctx, int B, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, double t0, int n_ticks, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int *ran_out, int max_iter, void *hip_stream) {
  if (int rc = select_check(ctx, B, qcap, queues, t_start, t_end, count)) return rc;
  if (n_ticks < 0 || !states) return fail(WG_ERR_BAD_ARG, "need n_ticks >= 0 and non-null states");
  if (B == 0 || n_ticks == 0) return WG_OK;
  return dimitrov_walk_launch(ctx, nullptr, B, qcap, queues, t_start, t_end, count, t0, n_ticks, states, outs, ran_out, max_iter, hip_stream);
}

// The walk with a clock and a tick count per gait: max_ticks rounds of { follow select, follow tick }.  The select launch decides,
// per gait, whether the gait's own queue covers the tick at the gait's own clock, and leaves the row its tick writes (or -1) in an
// int per gait behind the selected polytopes -- the context's walk buffer, claimed and marked like a walk's.
int wg_dimitrov_follow_dev_ctx(wg_ctx_t *ctx, int B, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, int lcap, const double *time, const int *have, const wg_zmpdisc_state_t *walk, int flags, double *clock, int *ticks, int tick_cap, int max_ticks, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int *ran_out, int max_iter, void *hip_stream) {
  if (int rc = select_check(ctx, B, qcap, queues, t_start, t_end, count)) return rc;
  if (int rc = follow_args_check(lcap, time, have, flags, clock, ticks, tick_cap, max_ticks, states)) return rc;
  if (B == 0 || max_ticks == 0) return WG_OK;
  return dimitrov_follow_launch(ctx, nullptr, B, qcap, queues, t_start, t_end, count, lcap, time, have, walk, flags, clock, ticks, tick_cap, max_ticks, states, outs, ran_out, max_iter, hip_stream);
}

// the clock of wg_dimitrov_walk_dev_ctx above, on the host: the same repeated addition of the configured T
double wg_dimitrov_walk_time_ctx(wg_ctx_t *ctx, double t0, int n_ticks) {
  if (!ctx || !ctx->dim_set) {
    (void)fail(WG_ERR_BAD_ARG, "wg_dimitrov_configure() has not been called on this context");
    return std::numeric_limits<double>::quiet_NaN();
  }
  const double T = ctx->dim_host->T;
  double t = t0;
  for (int k = 0; k < n_ticks; k++) t += T;
  return t;
}

int wg_dimitrov_walk_safe_ticks_ctx(wg_ctx_t *ctx, double t0, double t_have) {
  if (!ctx || !ctx->dim_set) return fail(WG_ERR_BAD_ARG, "wg_dimitrov_configure() has not been called on this context");
  if (!std::isfinite(t0) || !std::isfinite(t_have)) return fail(WG_ERR_BAD_ARG, "need finite t0 and t_have");
  const int i = ctx->dim_host->N - 1;
  const double T = ctx->dim_host->T;
  int n = 0;
  for (double t = t0; n < INT_MAX && t + i * T <= t_have; t += T) n++;       // the select kernel's t0 + i * T at its last instant
  return n;
}

}  // extern "C"

// ---- Dimitrov fleets with a model per gait: the constants as blocks, made on the host or on the device; the fleet launches ----

namespace {
int dimitrov_base_check(int N, int solver, double T) {
  if (N < 1 || N > WG_PLDP_N) return fail(WG_ERR_BAD_ARG, "N=%d outside [1,%d]", N, WG_PLDP_N);
  if (solver != WG_DIMITROV_PLDP && solver != WG_DIMITROV_QLD && solver != WG_DIMITROV_QLDANDLQ)
    return fail(WG_ERR_BAD_ARG, "solver = %d: WG_DIMITROV_PLDP (0), WG_DIMITROV_QLD (1) or WG_DIMITROV_QLDANDLQ (2)", solver);
  if (!(T > 0.0) || !std::isfinite(T)) return fail(WG_ERR_BAD_ARG, "need a finite T > 0");
  return WG_OK;
}
int dimitrov_constants_batch_check(int M, const wg_dimitrov_model_t *base, const void *blocks, const int *status) {
  if (M < 1 || !base || !blocks || !status) return fail(WG_ERR_BAD_ARG, "need M >= 1, non-null base, blocks and status");
  return dimitrov_base_check(base->N, base->solver, base->T);
}
int dimitrov_fleet_check(int B, const wg_dimitrov_fleet_t *fl) {
  if (!fl) return fail(WG_ERR_BAD_ARG, "null fleet");
  if (B < 0 || fl->M < 1 || !fl->blocks || !fl->model_of) return fail(WG_ERR_BAD_ARG, "need B >= 0, fleet M >= 1, non-null fleet blocks and model_of");
  return dimitrov_base_check(fl->N, fl->solver, fl->T);
}
// the fleet calls refuse their arguments before a context (and with it the device) is looked for
int dimitrov_tick_fleet_check(int B, const wg_dimitrov_fleet_t *fl, const wg_zmp_polytope_t *polys, const wg_dimitrov_state_t *states) {
  if (int rc = dimitrov_fleet_check(B, fl)) return rc;
  if (!polys || !states) return fail(WG_ERR_BAD_ARG, "need non-null polys and states");
  return WG_OK;
}
int dimitrov_walk_fleet_check(int B, const wg_dimitrov_fleet_t *fl, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, int n_ticks, const wg_dimitrov_state_t *states) {
  if (int rc = dimitrov_fleet_check(B, fl)) return rc;
  if (int rc = queue_check(B, qcap, queues, t_start, t_end, count)) return rc;
  if (n_ticks < 0 || !states) return fail(WG_ERR_BAD_ARG, "need n_ticks >= 0 and non-null states");
  return WG_OK;
}
int dimitrov_follow_fleet_check(int B, const wg_dimitrov_fleet_t *fl, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, int lcap, const double *time, const int *have, int flags, const double *clock, const int *ticks, int tick_cap, int max_ticks, const wg_dimitrov_state_t *states) {
  if (int rc = dimitrov_fleet_check(B, fl)) return rc;
  if (int rc = queue_check(B, qcap, queues, t_start, t_end, count)) return rc;
  return follow_args_check(lcap, time, have, flags, clock, ticks, tick_cap, max_ticks, states);
}
}  // namespace

extern "C" {

size_t wg_dimitrov_constants_bytes(void) { return wg::kDimitrovBlockBytes; }

// host arithmetic (wg_dimitrov_math.hpp through DimitrovHost::build, as wg_dimitrov_configure runs it); no device call
int wg_dimitrov_constants(const wg_dimitrov_model_t *model, void *block) {
  if (!block) return fail(WG_ERR_BAD_ARG, "null block");
  memset(block, 0, wg::kDimitrovBlockBytes);
  if (!model) return fail(WG_ERR_BAD_ARG, "null model");
  if (int rc = dimitrov_base_check(model->N, model->solver, model->T)) return rc;
  std::unique_ptr<wg::DimitrovConst> K(new wg::DimitrovConst);
  if (!wg::DimitrovHost::build(*model, *K))
    return fail(WG_ERR_BAD_ARG, "a height or weight is not finite, or the LQ factor or the inverse of Pu does not exist for this model");
  memcpy(block, K.get(), sizeof *K);
  return WG_OK;
}

int wg_dimitrov_constants_unpack(const void *block, wg_dimitrov_model_t *model, double *iLQ, double *OptB, double *OptC, double *Pu, double *iPu, double *Px, double *Q, double *OptBq, double *OptCq, double *PuT, double *iPuPx) {
  if (!block) return fail(WG_ERR_BAD_ARG, "null block");
  const wg::DimitrovConst &K = *static_cast<const wg::DimitrovConst *>(block);
  if (K.N < 1 || K.N > WG_PLDP_N) return fail(WG_ERR_BAD_ARG, "not a block of a model that exists (N = %d)", K.N);
  const size_t N = (size_t)K.N, n = 2 * N;
  if (model) {                                           // the weights are not kept in a block: reported as zeros
    memset(model, 0, sizeof *model);
    model->N = K.N; model->solver = K.solver; model->T = K.T; model->Tctrl = K.Tctrl; model->com_height = K.h;
  }
  if (iLQ) memcpy(iLQ, K.iLQ, 8 * n * n);
  if (OptB) memcpy(OptB, K.OptB, 8 * n * 6);
  if (OptC) memcpy(OptC, K.OptC, 8 * n * n);
  if (Pu) memcpy(Pu, K.pldp.Pu, 8 * N * N);
  if (iPu) memcpy(iPu, K.pldp.iPu, 8 * N * N);
  if (Px) memcpy(Px, K.pldp.Px, 8 * N * 3);
  if (Q) memcpy(Q, K.Qq, 8 * n * n);
  if (OptBq) memcpy(OptBq, K.OptBq, 8 * n * 6);
  if (OptCq) memcpy(OptCq, K.OptCq, 8 * n * n);
  if (PuT) memcpy(PuT, K.PuTq, 8 * N * N);
  if (iPuPx) memcpy(iPuPx, K.pldp.iPuPx, 8 * n * 6);
  return WG_OK;
}

// one wave per model (wg_dimitrov_kernels.hpp); the host twin is wg_dimitrov_constants, the arithmetic wg_dimitrov_math.hpp
int wg_dimitrov_constants_batch_dev_ctx(wg_ctx_t *ctx, int M, const wg_dimitrov_model_t *base, const double *com_height, const double *alpha, const double *beta, void *blocks, int *status, void *hip_stream) {
  if (int rc = dimitrov_constants_batch_check(M, base, blocks, status)) return rc;
  if (int rc = use_ctx(ctx)) return rc;
  hipLaunchKernelGGL(wg_dimitrov_constants_kernel, dim3((M + kDimConstWaves - 1) / kDimConstWaves), dim3(64 * kDimConstWaves), 0,
                     reinterpret_cast<hipStream_t>(hip_stream), M, *base, com_height, alpha, beta, static_cast<unsigned char *>(blocks), status);
  HIP_TRY(hipGetLastError());
  return WG_OK;
}

// host pointers
int wg_dimitrov_constants_batch_ctx(wg_ctx_t *ctx, int M, const wg_dimitrov_model_t *base, const double *com_height, const double *alpha, const double *beta, void *blocks, int *status) {
  if (int rc = dimitrov_constants_batch_check(M, base, blocks, status)) return rc;
  if (int rc = use_ctx(ctx)) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HostScope hs(ctx);
  const size_t sM = (size_t)M;
  Arena a(ctx->dim_buf);
  const auto sh = a.take<double>(com_height ? sM : 0), sa = a.take<double>(alpha ? sM : 0), sb = a.take<double>(beta ? sM : 0);
  const auto sk = a.take<unsigned char>(sM * wg::kDimitrovBlockBytes);
  const auto ss = a.take<int>(sM);
  if (int rc = a.reserve()) return rc;
  if (com_height) WG_H2D(a(sh), com_height, sh.bytes());
  if (alpha) WG_H2D(a(sa), alpha, sa.bytes());
  if (beta) WG_H2D(a(sb), beta, sb.bytes());
  if (int rc = wg_dimitrov_constants_batch_dev_ctx(ctx, M, base, com_height ? a(sh) : nullptr, alpha ? a(sa) : nullptr, beta ? a(sb) : nullptr, a(sk), a(ss), hs.stream())) return rc;
  WG_D2H(blocks, a(sk), sk.bytes());
  WG_D2H(status, a(ss), ss.bytes());
  WG_HOST_WAIT();
  return WG_OK;
}

// the launches of wg_dimitrov_tick_batch_dev, wg_dimitrov_walk_dev and wg_dimitrov_follow_dev with blocks[model_of[g]] as gait g's
// model: the same launcher code, the context's buffers and orders; nothing of the context's configured model is read
int wg_dimitrov_tick_fleet_dev_ctx(wg_ctx_t *ctx, int B, const wg_dimitrov_fleet_t *fleet, const wg_zmp_polytope_t *polys, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int max_iter, void *hip_stream) {
  if (int rc = dimitrov_tick_fleet_check(B, fleet, polys, states)) return rc;
  if (int rc = use_ctx(ctx)) return rc;
  if (B == 0) return WG_OK;
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  return dimitrov_tick_launch(ctx, B, polys, states, outs, max_iter, reinterpret_cast<hipStream_t>(hip_stream), nullptr, fleet);
}

int wg_dimitrov_walk_fleet_dev_ctx(wg_ctx_t *ctx, int B, const wg_dimitrov_fleet_t *fleet, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, double t0, int n_ticks, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int *ran_out, int max_iter, void *hip_stream) {
  if (int rc = dimitrov_walk_fleet_check(B, fleet, qcap, queues, t_start, t_end, count, n_ticks, states)) return rc;
  if (int rc = use_ctx(ctx)) return rc;
  if (B == 0 || n_ticks == 0) return WG_OK;
  return dimitrov_walk_launch(ctx, fleet, B, qcap, queues, t_start, t_end, count, t0, n_ticks, states, outs, ran_out, max_iter, hip_stream);
}

int wg_dimitrov_follow_fleet_dev_ctx(wg_ctx_t *ctx, int B, const wg_dimitrov_fleet_t *fleet, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, int lcap, const double *time, const int *have, const wg_zmpdisc_state_t *walk, int flags, double *clock, int *ticks, int tick_cap, int max_ticks, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int *ran_out, int max_iter, void *hip_stream) {
  if (int rc = dimitrov_follow_fleet_check(B, fleet, qcap, queues, t_start, t_end, count, lcap, time, have, flags, clock, ticks, tick_cap, max_ticks, states)) return rc;
  if (int rc = use_ctx(ctx)) return rc;
  if (B == 0 || max_ticks == 0) return WG_OK;
  return dimitrov_follow_launch(ctx, fleet, B, qcap, queues, t_start, t_end, count, lcap, time, have, walk, flags, clock, ticks, tick_cap, max_ticks, states, outs, ran_out, max_iter, hip_stream);
}

}  // extern "C"

// ---- Kajita stage-1 preview control -------------------------------------------------------------------------------------

namespace {
int preview_check(wg_ctx *ctx, int B, int L, const double *zmp_x, const double *zmp_y, const double *state) {
  if (int rc = use_ctx(ctx)) return rc;
  if (!ctx->prev_set) return fail(WG_ERR_BAD_ARG, "wg_preview_configure() has not been called on this context");
  if (B < 0 || L < 0 || !zmp_x || !zmp_y || !state) return fail(WG_ERR_BAD_ARG, "bad arguments");
  return WG_OK;
}
// the split-chain kernel's instantiations, a table per form: T steps of the window per lane, eight lanes per gait-axis; full: the
// window is a whole number of T (no tail test).  The batch form of one model goes by the name and the arguments it is timed by.
constexpr int kSplitK = 8;
template <int T, bool FULL, bool RAGGED, bool FLEET>
constexpr auto split_kernel() {
  if constexpr (!RAGGED && !FLEET) return &wg::wg_preview_split_kernel<T, kSplitK, FULL>;
  else return &wg::wg_preview_split_form_kernel<T, kSplitK, FULL, RAGGED, FLEET>;
}
template <bool RAGGED, bool FLEET>
constexpr auto l2_kernel() {
  if constexpr (!RAGGED && !FLEET) return &wg::wg_preview_kernel;
  else return &wg::wg_preview_form_kernel<RAGGED, FLEET>;
}
template <bool RAGGED, bool FLEET>
struct SplitRow {
  int T;
  decltype(split_kernel<16, true, RAGGED, FLEET>()) full, part;
};
#define WG_SPLIT(T) {T, split_kernel<T, true, RAGGED, FLEET>(), split_kernel<T, false, RAGGED, FLEET>()}
template <bool RAGGED, bool FLEET>
constexpr SplitRow<RAGGED, FLEET> kSplitKernels[] = {WG_SPLIT(16), WG_SPLIT(24), WG_SPLIT(32), WG_SPLIT(40), WG_SPLIT(48)};
#undef WG_SPLIT

// The launch of the four preview entry points, behind their checks.  `may_split`: the split-chain kernel (eight lanes per
// gait-axis, nothing re-read) where it covers the window, 64 .. 384 samples; else the ring kernel where the caller asks for it
// (`ring`: the batch form of one model has one), else the L2 kernel.  The follow forms (RAGGED) put both axes of a gait in one wave,
// the batch forms use blockIdx.y.
template <bool RAGGED, bool FLEET>
int preview_launch(int B, int L, const wg::PreviewRows<RAGGED> &R, const wg::PreviewConst &K, const wg::PreviewFleet<FLEET> &fl, const double *F, const double *zx, const double *zy, double *state, double *com, double *zmp2, int simulation, bool may_split, bool ring, hipStream_t st) {
  constexpr int axes = RAGGED ? 1 : 2;                         // as grid rows; RAGGED: as halves of a wave
  auto launch = [&](auto kern, int blocks, int threads, size_t lds) {
    if constexpr (!RAGGED && !FLEET) hipLaunchKernelGGL(kern, dim3(blocks, axes), dim3(threads), lds, st, B, L, K, F, zx, zy, state, com, zmp2, simulation);
    else hipLaunchKernelGGL(kern, dim3(blocks, axes), dim3(threads), lds, st, B, L, R, K, fl, F, zx, zy, state, com, zmp2, simulation);
  };
  const SplitRow<RAGGED, FLEET> *split = nullptr;              // smallest instantiated T with K T >= nl
  for (const auto &s : kSplitKernels<RAGGED, FLEET>)
    if (!split && kSplitK * s.T >= K.nl) split = &s;
  if (may_split && split && K.nl >= 64) {
    const int per_wave = 64 / kSplitK * axes / 2;
    launch(K.nl % split->T == 0 ? split->full : split->part, (B + per_wave - 1) / per_wave, 64, (size_t)split->T * 64 * 8);
  } else if (ring) {
    int Rn = K.nl < 288 ? K.nl : 288;                          // 288 x 512 B = 144 KB of the CU's 160 KB
    if (Rn < 1) Rn = 1;
    return launch_lds(wg::wg_preview_ring_kernel, dim3((B + 63) / 64, 2), dim3(64), (size_t)Rn * 64 * 8, st, B, L, K, Rn, F, zx, zy, state, com, zmp2, simulation);
  } else {
    const int threads = !RAGGED && B >= 4096 ? 256 : 64;       // small batches: more blocks, one wave each
    const int per_block = threads * axes / 2;
    launch(l2_kernel<RAGGED, FLEET>(), (B + per_block - 1) / per_block, threads, 0);
  }
  HIP_TRY(hipGetLastError());
  return WG_OK;
}
}  // namespace

extern "C" {

int wg_preview_configure_ctx(wg_ctx_t *ctx, const wg_preview_gains_t *gains, const double *F) {
  if (int rc = use_ctx(ctx)) return rc;
  if (!gains || !F) return fail(WG_ERR_BAD_ARG, "null argument");
  if (gains->nl < 1 || gains->nl > WG_PREVIEW_NL_MAX) return fail(WG_ERR_BAD_ARG, "need 1 <= nl <= %d", WG_PREVIEW_NL_MAX);
  if (!(gains->T > 0.0)) return fail(WG_ERR_BAD_ARG, "sampling period must be positive");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->prev_F) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->prev_F), sizeof(double) * WG_PREVIEW_NL_MAX));
  if (int rc = ctx_wait_own(ctx)) return rc;             // a run with the previous window may still be reading the gains
  HostScope hs(ctx);
  WG_H2D(ctx->prev_F, F, sizeof(double) * gains->nl);
  WG_HOST_WAIT();
  const double T = gains->T;                                   // PreviewControl.cpp:203-214
  ctx->prev.A01 = T; ctx->prev.A02 = T * T / 2.0; ctx->prev.A12 = T;
  ctx->prev.B0 = T * T * T / 6.0; ctx->prev.B1 = T * T / 2.0; ctx->prev.B2 = T;
  ctx->prev.C2 = -gains->zc / 9.81;
  ctx->prev.Kx0 = gains->Kx[0]; ctx->prev.Kx1 = gains->Kx[1]; ctx->prev.Kx2 = gains->Kx[2]; ctx->prev.Ks = gains->Ks;
  ctx->prev.nl = gains->nl;
  ctx->prev_set = true;
  return WG_OK;
}

int wg_preview_window_ctx(wg_ctx_t *ctx) { return (ctx && ctx->prev_set) ? ctx->prev.nl : 0; }

int wg_preview_run_batch_dev_ctx(wg_ctx_t *ctx, int B, int L, const double *zmp_x_tm, const double *zmp_y_tm, double *state, double *com_tm, double *zmp2_tm, int simulation, void *hip_stream) {
  if (int rc = preview_check(ctx, B, L, zmp_x_tm, zmp_y_tm, state)) return rc;
  if (B == 0 || L == 0) return WG_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const char *force = getenv("WG_PREVIEW_KERNEL");            // "l2" / "ring" / "split": tests hold each to the oracle
  // The ring kernel keeps one wave per CU (its window fills the LDS): it wins while the batch is too small to give every
  // SIMD several waves of the L2 kernel (measured: B = 4096: 0.62 vs 0.43 G gait-steps/s; B = 32768: 1.18 vs 1.50), and
  // a few steps do not repay filling the ring.
  const bool ring = force ? force[0] == 'r' : (L >= 8 && (long long)B * 2 <= (long long)ctx->num_cu * 64 * 2);
  // The split-chain kernel covers the standard window sizes and wins at every batch size measured; other windows, and runs too
  // short to repay filling its rings, use the other two.
  const bool may_split = force ? force[0] == 's' : L >= 4;
  if (int rc = preview_launch<false, false>(B, L, {}, ctx->prev, {}, ctx->prev_F, zmp_x_tm, zmp_y_tm, state, com_tm, zmp2_tm, simulation, may_split, ring, st)) return rc;
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  return slot_mark(ctx->aux_order, st);
}

int wg_preview_follow_dev_ctx(wg_ctx_t *ctx, int B, int lcap, const int *length, int *done, const double *zmp_x_tm, const double *zmp_y_tm, double *state, double *com_tm, double *zmp2_tm, int simulation, void *hip_stream) {
  if (int rc = preview_check(ctx, B, lcap, zmp_x_tm, zmp_y_tm, state)) return rc;
  if (!length || !done) return fail(WG_ERR_BAD_ARG, "null length or done");
  if (lcap < ctx->prev.nl) return fail(WG_ERR_BAD_ARG, "lcap=%d holds no window of nl=%d samples", lcap, ctx->prev.nl);
  if (B == 0) return WG_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const char *force = getenv("WG_PREVIEW_KERNEL");            // "l2" / "split" as in the batch call; "ring" has no follow form: l2
  if (int rc = preview_launch<true, false>(B, 0, {lcap, length, done}, ctx->prev, {}, ctx->prev_F, zmp_x_tm, zmp_y_tm, state, com_tm, zmp2_tm, simulation, force ? force[0] == 's' : true, false, st)) return rc;
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  return slot_mark(ctx->aux_order, st);
}

int wg_preview_run_batch_ctx(wg_ctx_t *ctx, int B, int L, const double *zmp_x, const double *zmp_y, double *state, double *com, double *zmp2, int simulation) {
  if (int rc = preview_check(ctx, B, L, zmp_x, zmp_y, state)) return rc;
  if (B == 0 || L == 0) return WG_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HostScope hs(ctx);
  const size_t sB = (size_t)B, sL = (size_t)L, Lz = sL + ctx->prev.nl - 1;
  // arena: gait-major staging (largest user: com, B x L x 6), time-major zx, zy, com, zmp2, state
  Arena a(ctx->prev_buf);
  const auto s_stage = a.take<double>(sB * (sL * 6 > Lz ? sL * 6 : Lz)), s_zx = a.take<double>(sB * Lz), s_zy = a.take<double>(sB * Lz),
             s_com = a.take<double>(sB * sL * 6), s_z2 = a.take<double>(sB * sL * 2), s_st = a.take<double>(sB * 8);
  if (int rc = a.reserve()) return rc;
  double *d_stage = a(s_stage);
  auto transpose = [&](int rows, int cols, const double *in, double *out) {
    hipLaunchKernelGGL(wg::wg_transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(32, 8), 0, hs.stream(), rows, cols, in, out);
  };
  // everything below is in order on the context's stream: the staging buffer is reused only behind the transpose that read it
  WG_H2D(d_stage, zmp_x, s_zx.bytes());
  transpose(B, (int)Lz, d_stage, a(s_zx));
  WG_H2D(d_stage, zmp_y, s_zy.bytes());
  transpose(B, (int)Lz, d_stage, a(s_zy));
  WG_H2D(a(s_st), state, s_st.bytes());
  if (int rc = wg_preview_run_batch_dev_ctx(ctx, B, L, a(s_zx), a(s_zy), a(s_st), com ? a(s_com) : nullptr, zmp2 ? a(s_z2) : nullptr, simulation,
                                            hs.stream()))
    return rc;
  WG_D2H(state, a(s_st), s_st.bytes());
  if (com) {                                                   // [L*6][B] -> [B][L*6]
    transpose(L * 6, B, a(s_com), d_stage);
    WG_D2H(com, d_stage, s_com.bytes());
  }
  if (zmp2) {
    transpose(L * 2, B, a(s_z2), d_stage);
    WG_D2H(zmp2, d_stage, s_z2.bytes());
  }
  HIP_TRY(hipGetLastError());
  WG_HOST_WAIT();
  return WG_OK;
}

}  // extern "C"

// ---- Kajita fleets with a CoM height per gait: gains made on the device, preview with gains per gait --------------------------

namespace {
// everything the fleet calls refuse is refused here, before a context or the device is touched
int riccati_batch_check(int B, double T, const double *zc, double R, int Nl, int mode, const double *K, const double *F, const int *status) {
  if (B < 0 || !(T > 0.0) || !(R > 0.0) || Nl < 0 || Nl > WG_PREVIEW_NL_MAX || (mode != WG_RICCATI_WITH_INITIALPOS && mode != WG_RICCATI_WITHOUT_INITIALPOS))
    return fail(WG_ERR_BAD_ARG, "need B >= 0, T > 0, R > 0, 0 <= Nl <= %d and a known mode", WG_PREVIEW_NL_MAX);
  if (!zc || !K || !status || (Nl > 0 && !F)) return fail(WG_ERR_BAD_ARG, "null argument");
  return WG_OK;
}
int preview_fleet_check(int B, int L, const wg_preview_fleet_t *fleet, const double *zmp_x, const double *zmp_y, const double *state) {
  if (!fleet || !fleet->zc || !fleet->K_tm || !fleet->F_tm) return fail(WG_ERR_BAD_ARG, "null fleet, or a null array in it");
  if (fleet->nl < 1 || fleet->nl > WG_PREVIEW_NL_MAX) return fail(WG_ERR_BAD_ARG, "need 1 <= nl <= %d", WG_PREVIEW_NL_MAX);
  if (!(fleet->T > 0.0)) return fail(WG_ERR_BAD_ARG, "sampling period must be positive");
  if (B < 0 || L < 0 || !zmp_x || !zmp_y || !state) return fail(WG_ERR_BAD_ARG, "bad arguments");
  return WG_OK;
}
int preview_follow_fleet_check(int B, int lcap, const int *length, const int *done, const wg_preview_fleet_t *fleet, const double *zmp_x, const double *zmp_y, const double *state) {
  if (int rc = preview_fleet_check(B, lcap, fleet, zmp_x, zmp_y, state)) return rc;
  if (!length || !done) return fail(WG_ERR_BAD_ARG, "null length or done");
  if (lcap < fleet->nl) return fail(WG_ERR_BAD_ARG, "lcap=%d holds no window of nl=%d samples", lcap, fleet->nl);
  return WG_OK;
}
// A and B of the fleet-wide T, as wg_preview_configure fills them (PreviewControl.cpp:203-214); what depends on the height is
// read per gait in the kernel
wg::PreviewConst preview_fleet_const(const wg_preview_fleet_t *fleet) {
  wg::PreviewConst k;
  memset(&k, 0, sizeof k);
  const double T = fleet->T;
  k.A01 = T; k.A02 = T * T / 2.0; k.A12 = T;
  k.B0 = T * T * T / 6.0; k.B1 = T * T / 2.0; k.B2 = T;
  k.nl = fleet->nl;
  return k;
}
}  // namespace

extern "C" {

// one lane per model (wg_riccati_kernels.hpp); the host twin is wg_riccati_gains (wg_riccati.cpp), the arithmetic wg_riccati_math.hpp
int wg_riccati_gains_batch_dev_ctx(wg_ctx_t *ctx, int B, double T, const double *zc, double Q, double R, int Nl, int mode, double *K_tm, double *F_tm, int *status, void *hip_stream) {
  if (int rc = riccati_batch_check(B, T, zc, R, Nl, mode, K_tm, F_tm, status)) return rc;
  if (int rc = use_ctx(ctx)) return rc;
  if (B == 0) return WG_OK;
  hipLaunchKernelGGL(wg::wg_riccati_gains_kernel, dim3((B + 63) / 64), dim3(64), 0, reinterpret_cast<hipStream_t>(hip_stream), B, T, zc, Q, R, Nl,
                     mode, K_tm, F_tm, status);
  HIP_TRY(hipGetLastError());
  return WG_OK;
}

// host pointers, gait-major: K [B][4], F [B][Nl]
int wg_riccati_gains_batch_ctx(wg_ctx_t *ctx, int B, double T, const double *zc, double Q, double R, int Nl, int mode, double *K, double *F, int *status) {
  if (int rc = riccati_batch_check(B, T, zc, R, Nl, mode, K, F, status)) return rc;
  if (int rc = use_ctx(ctx)) return rc;
  if (B == 0) return WG_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HostScope hs(ctx);
  const size_t sB = (size_t)B, sN = (size_t)Nl;
  Arena a(ctx->prev_buf);
  const auto s_zc = a.take<double>(sB), s_K = a.take<double>(4 * sB), s_F = a.take<double>(sN * sB), s_stage = a.take<double>(sB * (sN > 4 ? sN : 4));
  const auto s_st = a.take<int>(sB);
  if (int rc = a.reserve()) return rc;
  auto transpose = [&](int rows, int cols, const double *in, double *out) {
    hipLaunchKernelGGL(wg::wg_transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(32, 8), 0, hs.stream(), rows, cols, in, out);
  };
  WG_H2D(a(s_zc), zc, s_zc.bytes());
  if (int rc = wg_riccati_gains_batch_dev_ctx(ctx, B, T, a(s_zc), Q, R, Nl, mode, a(s_K), a(s_F), a(s_st), hs.stream())) return rc;
  transpose(4, B, a(s_K), a(s_stage));                         // [4][B] -> [B][4]; the staging buffer is reused behind the copy that reads it
  WG_D2H(K, a(s_stage), s_K.bytes());
  if (Nl > 0) {
    transpose(Nl, B, a(s_F), a(s_stage));
    WG_D2H(F, a(s_stage), s_F.bytes());
  }
  WG_D2H(status, a(s_st), s_st.bytes());
  HIP_TRY(hipGetLastError());
  WG_HOST_WAIT();
  return WG_OK;
}

// wg_preview_run_batch_dev with the gains of `fleet` per gait: reads nothing of the context's configured gains; the split-chain
// kernel for windows of 64 .. 384 samples, whatever L
int wg_preview_run_fleet_dev_ctx(wg_ctx_t *ctx, int B, int L, const wg_preview_fleet_t *fleet, const double *zmp_x_tm, const double *zmp_y_tm, double *state, double *com_tm, double *zmp2_tm, int simulation, void *hip_stream) {
  if (int rc = preview_fleet_check(B, L, fleet, zmp_x_tm, zmp_y_tm, state)) return rc;
  if (int rc = use_ctx(ctx)) return rc;
  if (B == 0 || L == 0) return WG_OK;
  return preview_launch<false, true>(B, L, {}, preview_fleet_const(fleet), {fleet->zc, fleet->K_tm}, fleet->F_tm, zmp_x_tm, zmp_y_tm, state, com_tm, zmp2_tm, simulation, true, false, reinterpret_cast<hipStream_t>(hip_stream));
}

int wg_preview_follow_fleet_dev_ctx(wg_ctx_t *ctx, int B, int lcap, const int *length, int *done, const wg_preview_fleet_t *fleet, const double *zmp_x_tm, const double *zmp_y_tm, double *state, double *com_tm, double *zmp2_tm, int simulation, void *hip_stream) {
  if (int rc = preview_follow_fleet_check(B, lcap, length, done, fleet, zmp_x_tm, zmp_y_tm, state)) return rc;
  if (int rc = use_ctx(ctx)) return rc;
  if (B == 0) return WG_OK;
  return preview_launch<true, true>(B, 0, {lcap, length, done}, preview_fleet_const(fleet), {fleet->zc, fleet->K_tm}, fleet->F_tm, zmp_x_tm, zmp_y_tm, state, com_tm, zmp2_tm, simulation, true, false, reinterpret_cast<hipStream_t>(hip_stream));
}


}  // extern "C"

// ---- invariant Hessian block on the matrix cores (fleets with per-gait models) -----------------------------------------

namespace {
int gramian_check(wg_ctx *ctx, int B, int N, const double *T, const double *h, const double *Qb) {
  if (int rc = use_ctx(ctx)) return rc;
  if (B < 0 || N < 1 || N > 32 || !T || !h || !Qb) return fail(WG_ERR_BAD_ARG, "need B >= 0, 1 <= N <= 32, non-null arrays");
  return WG_OK;
}
}  // namespace

extern "C" {

int wg_gramian_batch_dev_ctx(wg_ctx_t *ctx, int B, int N, const double *T, const double *h, double alpha, double beta, double gamma, int precision, double *Qb, void *hip_stream) {
  if (int rc = gramian_check(ctx, B, N, T, h, Qb)) return rc;
  if (precision != WG_GRAMIAN_F64 && precision != WG_GRAMIAN_F32) return fail(WG_ERR_BAD_ARG, "unknown precision %d", precision);
  if (B == 0) return WG_OK;
  const auto kern = precision == WG_GRAMIAN_F32 ? wg::wg_gramian_kernel<true> : wg::wg_gramian_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(hip_stream), B, N, T, h, alpha, beta, gamma, Qb);
  HIP_TRY(hipGetLastError());
  return WG_OK;
}

int wg_gramian_batch_ctx(wg_ctx_t *ctx, int B, int N, const double *T, const double *h, double alpha, double beta, double gamma, int precision, double *Qb) {
  if (int rc = gramian_check(ctx, B, N, T, h, Qb)) return rc;
  if (B == 0) return WG_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HostScope hs(ctx);
  const size_t sB = (size_t)B;
  Arena a(ctx->gram_buf);
  const auto sT = a.take<double>(sB), sh = a.take<double>(sB), sQ = a.take<double>(sB * N * N);
  if (int rc = a.reserve()) return rc;
  WG_H2D(a(sT), T, sT.bytes());
  WG_H2D(a(sh), h, sh.bytes());
  if (int rc = wg_gramian_batch_dev_ctx(ctx, B, N, a(sT), a(sh), alpha, beta, gamma, precision, a(sQ), hs.stream())) return rc;
  WG_D2H(Qb, a(sQ), sQ.bytes());
  WG_HOST_WAIT();
  return WG_OK;
}

}  // extern "C"

// ---- Kajita stage-1 inputs: ZMPDiscretization, batched (one lane per gait) ----------------------------------------------

namespace {
// InitializeFilter, ZMPDiscretization.cpp:240-262 (sin from include/wg_trig.h: same bits on host and device)
int zd_make_const(const wg_zmpdisc_model_t *model, wg::ZdConst *K) {
  if (!model) return fail(WG_ERR_BAD_ARG, "null model");
  if (!(model->T > 0.0)) return fail(WG_ERR_BAD_ARG, "sampling period must be positive");
  const int n = (int)floor(0.05 / model->T);
  if (n < 1 || n + 1 > WG_ZD_WIN_MAX)
    return fail(WG_ERR_BAD_ARG, "filter window of %d taps unsupported (1 < taps <= %d)", n + 1, WG_ZD_WIN_MAX);
  K->M = *model;
  K->nwin = n + 1;
  K->pad_ = 0;
  double sum = 0;
  for (int i = 0; i < n + 1; i++) {
    const double tmp = wg_sin((WG_ZD_PI * i) / n);
    K->win[i] = tmp * tmp;
  }
  for (int i = 0; i < n + 1; i++) sum += K->win[i];
  for (int i = 0; i < n + 1; i++) K->win[i] /= sum;
  for (int i = n + 1; i < WG_ZD_WIN_MAX; i++) K->win[i] = 0.0;
  return WG_OK;
}

// what the three entry points check alike: the context, the model (-> K), the sizes; `ptrs_ok`: the arrays each of them requires
int zd_check(wg_ctx *ctx, const wg_zmpdisc_model_t *model, wg::ZdConst *K, int B, int smax, int lcap, bool ptrs_ok, const char *what) {
  if (int rc = use_ctx(ctx)) return rc;
  if (int rc = zd_make_const(model, K)) return rc;
  if (B < 0 || smax < 2 || smax > WG_ZMPDISC_MAX_STEPS || lcap < 1 || !ptrs_ok)
    return fail(WG_ERR_BAD_ARG, "need B >= 0, 2 <= smax <= %d, lcap >= 1, non-null %s", WG_ZMPDISC_MAX_STEPS, what);
  return WG_OK;
}

// the one launch of the walk's kernels: a lane per gait, the rings (`fleet`: and the models of the wave) in LDS; K is their first argument
template <class Kernel, class... Args>
int zd_launch_kernel(Kernel kernel, const wg::ZdConst &K, int B, bool fleet, hipStream_t st, Args... args) {
  return launch_lds(kernel, dim3((B + 63) / 64), dim3(64), wg::zd_lds_bytes(K.nwin, fleet), st, K, args...);
}
int zd_launch(const wg::ZdConst &K, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
              const double *init_feet, int lcap, const wg::ZdOut &O, int *length, hipStream_t st) {
  return zd_launch_kernel(wg::wg_zmpdisc_kernel, K, B, false, st, B, smax, steps, n_steps, init_feet, lcap, O, length);
}

// what begin / append / end check of their arguments, the model aside
int zd_online_check(int op, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, int lcap,
                    const wg::ZdOut &O, const wg_zmpdisc_state_t *state) {
  const int smin = op == wg::ZD_OP_BEGIN ? 2 : 1;
  const bool steps_ok = op == wg::ZD_OP_END || (steps && n_steps && smax >= smin && smax <= WG_ZMPDISC_MAX_STEPS);
  if (B < 0 || lcap < 1 || !state || !steps_ok || (op == wg::ZD_OP_BEGIN && !init_feet))
    return fail(WG_ERR_BAD_ARG, "need B >= 0, %d <= smax <= %d, lcap >= 1, non-null inputs and state", smin, WG_ZMPDISC_MAX_STEPS);
  if ((O.zx == nullptr) != (O.zy == nullptr)) return fail(WG_ERR_BAD_ARG, "zmp_x_tm and zmp_y_tm go together");
  return WG_OK;
}

// A model per gait: what the four fleet entry points check alike before the checks of their one-model twins -- the fleet itself,
// its base model (-> K: the window and the taps; the gaits' own models are read on the device) and the room for the wave's models
// in LDS beside the rings -- and the kernel's view of the fleet.
int zd_fleet_check(wg_ctx *ctx, const wg_zmpdisc_fleet_t *fleet, int B, wg::ZdConst *K, wg::ZdFleet *FL) {
  if (int rc = use_ctx(ctx)) return rc;
  if (!fleet || !fleet->models) return fail(WG_ERR_BAD_ARG, "null fleet or models");
  if (fleet->M < 1 || (!fleet->model_of && fleet->M != B))
    return fail(WG_ERR_BAD_ARG, "M = %d: need M >= 1, and M == B = %d without model_of", fleet->M, B);
  if (int rc = zd_make_const(&fleet->base, K)) return rc;
  if (wg::zd_lds_bytes(K->nwin, true) > 160 * 1024)
    return fail(WG_ERR_BAD_ARG, "filter window of %d taps leaves no room for the models of a wave in LDS", K->nwin);
  *FL = wg::ZdFleet{fleet->models, fleet->model_of, fleet->M, 0};
  return WG_OK;
}

// begin / append / end of an on-line walk, with one model or a model per gait (`mf`): the model checks of either, the checks
// they share, then one launch of the resumable kernel
template <class ModelOrFleet>
int zd_online(wg_ctx *ctx, int op, const ModelOrFleet *mf, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
              const double *init_feet, const int *select, int lcap, const wg::ZdOut &O, wg_zmpdisc_state_t *state, int *length,
              void *hip_stream) {
  constexpr bool fleet = std::is_same<ModelOrFleet, wg_zmpdisc_fleet_t>::value;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  wg::ZdConst K;
  [[maybe_unused]] wg::ZdFleet FL;
  if constexpr (fleet) {
    if (int rc = zd_fleet_check(ctx, mf, B, &K, &FL)) return rc;
  } else {
    if (int rc = use_ctx(ctx)) return rc;
    if (int rc = zd_make_const(mf, &K)) return rc;
  }
  if (int rc = zd_online_check(op, B, smax, steps, n_steps, init_feet, lcap, O, state)) return rc;
  if (B == 0) return WG_OK;
  if constexpr (fleet) return zd_launch_kernel(wg::wg_zmpdisc_form_kernel<true, true>, K, B, true, st, FL, op, B, smax, steps, n_steps, init_feet, select, lcap, O, state, length);
  else return zd_launch_kernel(wg::wg_zmpdisc_online_kernel, K, B, false, st, op, B, smax, steps, n_steps, init_feet, select, lcap, O, state, length);
}
}  // namespace

extern "C" {

void wg_zmpdisc_defaults(wg_zmpdisc_model_t *m) {
  if (!m) return;
  memset(m, 0, sizeof *m);
  m->T = 0.005;                    // ZMPRefTrajectoryGeneration's members as PatternGeneratorInterfacePrivate.cpp sets them
  m->preview_time = 1.6;
  m->t_single = 0.78;
  m->t_double = 0.02;
  m->step_height = 0.07;
  m->omega = 0.0;
  m->modulation = 0.9;             // ZMPDiscretization.cpp:99
}

int wg_zmpdisc_length(const wg_zmpdisc_model_t *model, const wg_rel_step_t *steps, int n_steps) {
  if (!model || !steps) return WG_ZMPDISC_BAD_INPUT;
  return wg::zd_length(*model, steps, n_steps);
}

int wg_zmpdisc_batch_dev_ctx(wg_ctx_t *ctx, const wg_zmpdisc_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, int lcap, double *zmp_x_tm, double *zmp_y_tm, int *length, void *hip_stream) {
  wg::ZdConst K;
  if (int rc = zd_check(ctx, model, &K, B, smax, lcap, steps && n_steps && init_feet && zmp_x_tm && zmp_y_tm, "arrays")) return rc;
  if (B == 0) return WG_OK;
  wg::ZdOut O;
  memset(&O, 0, sizeof O);
  O.zx = zmp_x_tm;
  O.zy = zmp_y_tm;
  return zd_launch(K, B, smax, steps, n_steps, init_feet, lcap, O, length, reinterpret_cast<hipStream_t>(hip_stream));
}

int wg_zmpdisc_full_batch_dev_ctx(wg_ctx_t *ctx, const wg_zmpdisc_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, int *length, void *hip_stream) {
  wg::ZdConst K;
  if (int rc = zd_check(ctx, model, &K, B, smax, lcap, steps && n_steps && init_feet, "inputs")) return rc;
  if ((zmp_x_tm == nullptr) != (zmp_y_tm == nullptr)) return fail(WG_ERR_BAD_ARG, "zmp_x_tm and zmp_y_tm go together");
  if (B == 0) return WG_OK;
  wg::ZdOut O;
  O.zx = zmp_x_tm; O.zy = zmp_y_tm; O.ztheta = zmp_theta_tm; O.ztype = zmp_type_tm;
  O.left = left_tm; O.ltype = left_type_tm; O.right = right_tm; O.rtype = right_type_tm;
  return zd_launch(K, B, smax, steps, n_steps, init_feet, lcap, O, length, reinterpret_cast<hipStream_t>(hip_stream));
}

int wg_zmpdisc_length_after(const wg_zmpdisc_model_t *model, const wg_rel_step_t *steps, int n_steps, int ended) {
  if (!model || !steps) return WG_ZMPDISC_BAD_INPUT;
  return wg::zd_length_after(*model, steps, n_steps, ended);
}

int wg_zmpdisc_begin_dev_ctx(wg_ctx_t *ctx, const wg_zmpdisc_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, wg_zmpdisc_state_t *state, int *length, void *hip_stream) {
  const wg::ZdOut O{zmp_x_tm, zmp_y_tm, zmp_theta_tm, zmp_type_tm, left_tm, right_tm, left_type_tm, right_type_tm};
  return zd_online(ctx, wg::ZD_OP_BEGIN, model, B, smax, steps, n_steps, init_feet, nullptr, lcap, O, state, length, hip_stream);
}

int wg_zmpdisc_append_dev_ctx(wg_ctx_t *ctx, const wg_zmpdisc_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, wg_zmpdisc_state_t *state, int *length, void *hip_stream) {
  const wg::ZdOut O{zmp_x_tm, zmp_y_tm, zmp_theta_tm, zmp_type_tm, left_tm, right_tm, left_type_tm, right_type_tm};
  return zd_online(ctx, wg::ZD_OP_APPEND, model, B, smax, steps, n_steps, nullptr, nullptr, lcap, O, state, length, hip_stream);
}

int wg_zmpdisc_end_dev_ctx(wg_ctx_t *ctx, const wg_zmpdisc_model_t *model, int B, const int *select, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, wg_zmpdisc_state_t *state, int *length, void *hip_stream) {
  const wg::ZdOut O{zmp_x_tm, zmp_y_tm, zmp_theta_tm, zmp_type_tm, left_tm, right_tm, left_type_tm, right_type_tm};
  return zd_online(ctx, wg::ZD_OP_END, model, B, 0, nullptr, nullptr, nullptr, select, lcap, O, state, length, hip_stream);
}

// the four with a model per gait
int wg_zmpdisc_full_fleet_dev_ctx(wg_ctx_t *ctx, const wg_zmpdisc_fleet_t *fleet, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, int *length, void *hip_stream) {
  wg::ZdConst K;
  wg::ZdFleet FL;
  if (int rc = zd_fleet_check(ctx, fleet, B, &K, &FL)) return rc;
  if (int rc = zd_check(ctx, &fleet->base, &K, B, smax, lcap, steps && n_steps && init_feet, "inputs")) return rc;
  if ((zmp_x_tm == nullptr) != (zmp_y_tm == nullptr)) return fail(WG_ERR_BAD_ARG, "zmp_x_tm and zmp_y_tm go together");
  if (B == 0) return WG_OK;
  const wg::ZdOut O{zmp_x_tm, zmp_y_tm, zmp_theta_tm, zmp_type_tm, left_tm, right_tm, left_type_tm, right_type_tm};
  return zd_launch_kernel(wg::wg_zmpdisc_form_kernel<false, true>, K, B, true, reinterpret_cast<hipStream_t>(hip_stream), FL, 0, B, smax, steps,
                          n_steps, init_feet, nullptr, lcap, O, nullptr, length);
}

int wg_zmpdisc_begin_fleet_dev_ctx(wg_ctx_t *ctx, const wg_zmpdisc_fleet_t *fleet, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, wg_zmpdisc_state_t *state, int *length, void *hip_stream) {
  const wg::ZdOut O{zmp_x_tm, zmp_y_tm, zmp_theta_tm, zmp_type_tm, left_tm, right_tm, left_type_tm, right_type_tm};
  return zd_online(ctx, wg::ZD_OP_BEGIN, fleet, B, smax, steps, n_steps, init_feet, nullptr, lcap, O, state, length, hip_stream);
}

int wg_zmpdisc_append_fleet_dev_ctx(wg_ctx_t *ctx, const wg_zmpdisc_fleet_t *fleet, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, wg_zmpdisc_state_t *state, int *length, void *hip_stream) {
  const wg::ZdOut O{zmp_x_tm, zmp_y_tm, zmp_theta_tm, zmp_type_tm, left_tm, right_tm, left_type_tm, right_type_tm};
  return zd_online(ctx, wg::ZD_OP_APPEND, fleet, B, smax, steps, n_steps, nullptr, nullptr, lcap, O, state, length, hip_stream);
}

int wg_zmpdisc_end_fleet_dev_ctx(wg_ctx_t *ctx, const wg_zmpdisc_fleet_t *fleet, int B, const int *select, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *zmp_theta_tm, int *zmp_type_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, wg_zmpdisc_state_t *state, int *length, void *hip_stream) {
  const wg::ZdOut O{zmp_x_tm, zmp_y_tm, zmp_theta_tm, zmp_type_tm, left_tm, right_tm, left_type_tm, right_type_tm};
  return zd_online(ctx, wg::ZD_OP_END, fleet, B, 0, nullptr, nullptr, nullptr, select, lcap, O, state, length, hip_stream);
}

}  // extern "C"

namespace {
// the step stack on the device, one wave per gait (wg_steps_kernels.hpp): what the two entry points below check and launch alike.
// `times_ok` and `refusal` (a format that takes WG_ZMPDISC_MAX_STEPS) are each one's own.
template <class Kernel, class... Times>
int steps_plan_launch(Kernel kernel, wg_ctx *ctx, int B, int ccap, const wg_step_cmd_t *cmds, const int *n_cmds, bool times_ok, const char *refusal, wg_step_stack_t *stack, int smax, wg_rel_step_t *steps, int *n_steps, void *hip_stream, Times... times) {
  if (int rc = use_ctx(ctx)) return rc;
  if (B < 0 || ccap < 1 || smax < 1 || smax > WG_ZMPDISC_MAX_STEPS || !cmds || !n_cmds || !stack || !steps || !n_steps || !times_ok)
    return fail(WG_ERR_BAD_ARG, refusal, WG_ZMPDISC_MAX_STEPS);
  if (B == 0) return WG_OK;
  hipLaunchKernelGGL(kernel, dim3((B + wg::kSpWaves - 1) / wg::kSpWaves), dim3(64 * wg::kSpWaves), 0, reinterpret_cast<hipStream_t>(hip_stream), B, ccap, cmds,
                     n_cmds, times..., stack, smax, steps, n_steps);
  HIP_TRY(hipGetLastError());
  return WG_OK;
}
}  // namespace

extern "C" {

// with the support times of each gait (a non-finite time is the gait's own refusal, on the device)
int wg_steps_plan_fleet_dev_ctx(wg_ctx_t *ctx, int B, int ccap, const wg_step_cmd_t *cmds, const int *n_cmds, const double *ss, const double *ds, wg_step_stack_t *stack, int smax, wg_rel_step_t *steps, int *n_steps, void *hip_stream) {
  return steps_plan_launch(wg::wg_steps_plan_form_kernel<true>, ctx, B, ccap, cmds, n_cmds, ss && ds, "need B >= 0, ccap >= 1, 1 <= smax <= %d, non-null arrays",
                           stack, smax, steps, n_steps, hip_stream, wg::SpTimes<true>{ss, ds});
}

// with the call's times; the host twins are wg_steps.cpp
int wg_steps_plan_dev_ctx(wg_ctx_t *ctx, int B, int ccap, const wg_step_cmd_t *cmds, const int *n_cmds, double ss, double ds, wg_step_stack_t *stack, int smax, wg_rel_step_t *steps, int *n_steps, void *hip_stream) {
  return steps_plan_launch(wg::wg_steps_plan_kernel, ctx, B, ccap, cmds, n_cmds, wg::sp_finite(ss) && wg::sp_finite(ds),
                           "need B >= 0, ccap >= 1, 1 <= smax <= %d, finite times, non-null arrays", stack, smax, steps, n_steps, hip_stream, ss, ds);
}


int wg_zmpdisc_batch_ctx(wg_ctx_t *ctx, const wg_zmpdisc_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, int lcap, double *zmp, double *zmp_theta, int *zmp_type, double *left, int *left_type, double *right, int *right_type, int *length) {
  wg::ZdConst K;
  if (int rc = zd_check(ctx, model, &K, B, smax, lcap, steps && n_steps && init_feet && length, "arrays")) return rc;
  if (B == 0) return WG_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  std::vector<double> hd;                                      // host staging of the time-major arrays (outlive the copies into them)
  std::vector<int> hi;
  HostScope hs(ctx);
  const size_t sB = (size_t)B, sL = (size_t)lcap, row = sB * sL;
  Arena a(ctx->zd_buf);
  const auto s_steps = a.take<wg_rel_step_t>(sB * smax);
  const auto s_feet = a.take<double>(sB * 6), s_zx = a.take<double>(row), s_zy = a.take<double>(row), s_zt = a.take<double>(row),
             s_l = a.take<double>(6 * row), s_r = a.take<double>(6 * row);
  const auto s_ns = a.take<int>(sB), s_len = a.take<int>(sB), s_zty = a.take<int>(row), s_lty = a.take<int>(row), s_rty = a.take<int>(row);
  if (int rc = a.reserve()) return rc;
  WG_H2D(a(s_steps), steps, s_steps.bytes());
  WG_H2D(a(s_feet), init_feet, s_feet.bytes());
  WG_H2D(a(s_ns), n_steps, s_ns.bytes());
  wg::ZdOut O;
  memset(&O, 0, sizeof O);
  if (zmp) { O.zx = a(s_zx); O.zy = a(s_zy); }
  if (zmp_theta) O.ztheta = a(s_zt);
  if (zmp_type) O.ztype = a(s_zty);
  if (left) O.left = a(s_l);
  if (left_type) O.ltype = a(s_lty);
  if (right) O.right = a(s_r);
  if (right_type) O.rtype = a(s_rty);
  if (int rc = zd_launch(K, B, smax, a(s_steps), a(s_ns), a(s_feet), lcap, O, a(s_len), hs.stream())) return rc;
  WG_D2H(length, a(s_len), s_len.bytes());
  WG_HOST_WAIT();
  // time-major device arrays -> the caller's gait-major arrays, samples below each gait's length only
  auto fetch_d = [&](const double *dev, int comps, double *dst, int dst_stride, int dst_off) -> int {
    hd.resize(row * comps);
    WG_D2H(hd.data(), dev, row * comps * 8);
    WG_HOST_WAIT();
    for (size_t b = 0; b < sB; b++)
      for (int l = 0; l < length[b]; l++)
        for (int c = 0; c < comps; c++)
          dst[(b * sL + l) * dst_stride + dst_off + c] = hd[((size_t)l * comps + c) * sB + b];
    return WG_OK;
  };
  auto fetch_i = [&](const int *dev, int *dst) -> int {
    hi.resize(row);
    WG_D2H(hi.data(), dev, row * 4);
    WG_HOST_WAIT();
    for (size_t b = 0; b < sB; b++)
      for (int l = 0; l < length[b]; l++) dst[b * sL + l] = hi[(size_t)l * sB + b];
    return WG_OK;
  };
  if (zmp) {
    if (int rc = fetch_d(a(s_zx), 1, zmp, 2, 0)) return rc;
    if (int rc = fetch_d(a(s_zy), 1, zmp, 2, 1)) return rc;
  }
  if (zmp_theta) if (int rc = fetch_d(a(s_zt), 1, zmp_theta, 1, 0)) return rc;
  if (left) if (int rc = fetch_d(a(s_l), 6, left, 6, 0)) return rc;
  if (right) if (int rc = fetch_d(a(s_r), 6, right, 6, 0)) return rc;
  if (zmp_type) if (int rc = fetch_i(a(s_zty), zmp_type)) return rc;
  if (left_type) if (int rc = fetch_i(a(s_lty), left_type)) return rc;
  if (right_type) if (int rc = fetch_i(a(s_rty), right_type)) return rc;
  return WG_OK;
}

}  // extern "C"

// ---- the same entry points on the process-wide default context -----------------------------------------------------
extern "C" {

// the plain ones, one per entry of the header's list
#define WG_CTX_FORWARD_(ret, name, params, args) ret name params { return on_default(&name##_ctx, WG_CTX_UNPAREN_ args); }
WG_CTX_FORWARDED(WG_CTX_FORWARD_)
#undef WG_CTX_FORWARD_

long long wg_overlap_serialised(void) { return on_default(&wg_overlap_serialised_ctx); }
size_t wg_mpc_tick_lds_bytes(void) {                 // a query: does not create the default context
  std::lock_guard<std::mutex> lk(g_default_mu);
  return wg_mpc_tick_lds_bytes_ctx(g_default);
}
int wg_preview_window(void) {                        // a query: does not create the default context
  std::lock_guard<std::mutex> lk(g_default_mu);
  return wg_preview_window_ctx(g_default);
}
// the fleet calls refuse their arguments before the default context (and with it the device) is looked for
int wg_riccati_gains_batch_dev(int B, double T, const double *zc, double Q, double R, int Nl, int mode, double *K_tm, double *F_tm, int *status, void *hip_stream) {
  if (int rc = riccati_batch_check(B, T, zc, R, Nl, mode, K_tm, F_tm, status)) return rc;
  return on_default(&wg_riccati_gains_batch_dev_ctx, B, T, zc, Q, R, Nl, mode, K_tm, F_tm, status, hip_stream);
}
int wg_riccati_gains_batch(int B, double T, const double *zc, double Q, double R, int Nl, int mode, double *K, double *F, int *status) {
  if (int rc = riccati_batch_check(B, T, zc, R, Nl, mode, K, F, status)) return rc;
  return on_default(&wg_riccati_gains_batch_ctx, B, T, zc, Q, R, Nl, mode, K, F, status);
}
int wg_preview_run_fleet_dev(int B, int L, const wg_preview_fleet_t *fleet, const double *zmp_x_tm, const double *zmp_y_tm, double *state, double *com_tm, double *zmp2_tm, int simulation, void *hip_stream) {
  if (int rc = preview_fleet_check(B, L, fleet, zmp_x_tm, zmp_y_tm, state)) return rc;
  return on_default(&wg_preview_run_fleet_dev_ctx, B, L, fleet, zmp_x_tm, zmp_y_tm, state, com_tm, zmp2_tm, simulation, hip_stream);
}
int wg_preview_follow_fleet_dev(int B, int lcap, const int *length, int *done, const wg_preview_fleet_t *fleet, const double *zmp_x_tm, const double *zmp_y_tm, double *state, double *com_tm, double *zmp2_tm, int simulation, void *hip_stream) {
  if (int rc = preview_follow_fleet_check(B, lcap, length, done, fleet, zmp_x_tm, zmp_y_tm, state)) return rc;
  return on_default(&wg_preview_follow_fleet_dev_ctx, B, lcap, length, done, fleet, zmp_x_tm, zmp_y_tm, state, com_tm, zmp2_tm, simulation, hip_stream);
}
int wg_dimitrov_constants_batch_dev(int M, const wg_dimitrov_model_t *base, const double *com_height, const double *alpha, const double *beta, void *blocks, int *status, void *hip_stream) {
  if (int rc = dimitrov_constants_batch_check(M, base, blocks, status)) return rc;
  return on_default(&wg_dimitrov_constants_batch_dev_ctx, M, base, com_height, alpha, beta, blocks, status, hip_stream);
}
int wg_dimitrov_constants_batch(int M, const wg_dimitrov_model_t *base, const double *com_height, const double *alpha, const double *beta, void *blocks, int *status) {
  if (int rc = dimitrov_constants_batch_check(M, base, blocks, status)) return rc;
  return on_default(&wg_dimitrov_constants_batch_ctx, M, base, com_height, alpha, beta, blocks, status);
}
int wg_dimitrov_tick_fleet_dev(int B, const wg_dimitrov_fleet_t *fleet, const wg_zmp_polytope_t *polys, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int max_iter, void *hip_stream) {
  if (int rc = dimitrov_tick_fleet_check(B, fleet, polys, states)) return rc;
  return on_default(&wg_dimitrov_tick_fleet_dev_ctx, B, fleet, polys, states, outs, max_iter, hip_stream);
}
int wg_dimitrov_walk_fleet_dev(int B, const wg_dimitrov_fleet_t *fleet, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, double t0, int n_ticks, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int *ran_out, int max_iter, void *hip_stream) {
  if (int rc = dimitrov_walk_fleet_check(B, fleet, qcap, queues, t_start, t_end, count, n_ticks, states)) return rc;
  return on_default(&wg_dimitrov_walk_fleet_dev_ctx, B, fleet, qcap, queues, t_start, t_end, count, t0, n_ticks, states, outs, ran_out, max_iter, hip_stream);
}
int wg_dimitrov_follow_fleet_dev(int B, const wg_dimitrov_fleet_t *fleet, int qcap, const wg_zmp_polytope_t *queues, const double *t_start, const double *t_end, const int *count, int lcap, const double *time, const int *have, const wg_zmpdisc_state_t *walk, int flags, double *clock, int *ticks, int tick_cap, int max_ticks, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int *ran_out, int max_iter, void *hip_stream) {
  if (int rc = dimitrov_follow_fleet_check(B, fleet, qcap, queues, t_start, t_end, count, lcap, time, have, flags, clock, ticks, tick_cap, max_ticks, states)) return rc;
  return on_default(&wg_dimitrov_follow_fleet_dev_ctx, B, fleet, qcap, queues, t_start, t_end, count, lcap, time, have, walk, flags, clock, ticks, tick_cap, max_ticks, states, outs, ran_out, max_iter, hip_stream);
}

}  // extern "C"

// ---- Morisawa-2007 analytic walks (wg_morisawa_kernels.hpp; the host twins are wg_morisawa.cpp) ---------------------------------
// LONG: the wg_morisawa_long_* family -- its cap on smax, its layout and kernels; checks, lock and clock slot are the one text
namespace {

template <bool LONG>
constexpr int mo_cap() { return LONG ? WG_MORISAWA_LONG_MAX_STEPS : WG_MORISAWA_MAX_STEPS; }
template <bool LONG>
int mo_solve_check(const void *models, int B, int smax, const void *steps, const void *n_steps, const void *init_feet, const void *com0, const void *blocks, const void *status) {
  if (!models || B < 0 || smax < 2 || smax > mo_cap<LONG>() || !steps || !n_steps || !init_feet || !com0 || !blocks || !status)
    return fail(WG_ERR_BAD_ARG, "need a model, B >= 0, 2 <= smax <= %d, non-null steps, n_steps, init_feet, com0, blocks, status", mo_cap<LONG>());
  return WG_OK;
}
template <bool LONG>
int mo_sample_check(int B, int smax, const void *blocks, double t_start, double T, int lcap) {
  if (!blocks || B < 0 || smax < 2 || smax > mo_cap<LONG>() || lcap < 1 || lcap > (1 << 19) || !wg::mo_finite(T) || !(T > 0.0) || !wg::mo_finite(t_start) || t_start < 0.0)
    return fail(WG_ERR_BAD_ARG, "need blocks, B >= 0, 2 <= smax <= %d, 1 <= lcap <= %d, finite T > 0 and t_start >= 0", mo_cap<LONG>(), 1 << 19);
  return WG_OK;
}
// one wave per gait, the gait's work area in LDS; under the context's launch lock like every launch of a context
template <bool FLEET, bool LONG>
int mo_solve_launch(wg_ctx *ctx, const wg_morisawa_model_t *mf, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, const double *com0, void *blocks, int *status, hipStream_t st) {
  if (int rc = use_ctx(ctx)) return rc;
  if (int rc = mo_solve_check<LONG>(mf, B, smax, steps, n_steps, init_feet, com0, blocks, status)) return rc;
  if (B == 0) return WG_OK;
  wg_morisawa_model_t m;
  memset(&m, 0, sizeof m);
  if (!FLEET) m = *mf;
  const size_t lds = (size_t)(LONG ? wg::mo_layout_long(smax) : wg::mo_layout(smax)).work_words * sizeof(double);
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  if (LONG)
    return launch_lds(wg::wg_morisawa_solve_long_kernel<FLEET>, dim3(B), dim3(64), lds, st, m, FLEET ? mf : nullptr, B, smax, steps, n_steps, init_feet, com0, static_cast<double *>(blocks), status);
  return launch_lds(wg::wg_morisawa_solve_kernel<FLEET>, dim3(B), dim3(64), lds, st, m, FLEET ? mf : nullptr, B, smax, steps, n_steps, init_feet, com0, static_cast<double *>(blocks), status);
}
// the re-plan from kept factors: the solve's launch shape and work area; a gait's step count is its factor block's
template <bool FLEET, bool LONG>
int mo_resolve_launch(wg_ctx *ctx, const wg_morisawa_model_t *mf, int B, int smax, const void *factors, int n_factors, const int *factor_of, const wg_rel_step_t *steps, const double *init_feet, const double *com0, void *blocks, int *status, hipStream_t st) {
  if (int rc = use_ctx(ctx)) return rc;
  if (!mf || B < 0 || smax < 2 || smax > mo_cap<LONG>() || !factors || n_factors < 1 || !steps || !init_feet || !com0 || !blocks || !status)
    return fail(WG_ERR_BAD_ARG, "need a model, B >= 0, 2 <= smax <= %d, factors, n_factors >= 1, non-null steps, init_feet, com0, blocks, status", mo_cap<LONG>());
  if (B == 0) return WG_OK;
  wg_morisawa_model_t m;
  memset(&m, 0, sizeof m);
  if (!FLEET) m = *mf;
  const size_t lds = (size_t)(LONG ? wg::mo_layout_long(smax) : wg::mo_layout(smax)).work_words * sizeof(double);
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  if (LONG)
    return launch_lds(wg::wg_morisawa_resolve_long_kernel<FLEET>, dim3(B), dim3(64), lds, st, m, FLEET ? mf : nullptr, B, smax, static_cast<const double *>(factors), n_factors, factor_of, steps, init_feet, com0, static_cast<double *>(blocks), status);
  return launch_lds(wg::wg_morisawa_resolve_kernel<FLEET>, dim3(B), dim3(64), lds, st, m, FLEET ? mf : nullptr, B, smax, static_cast<const double *>(factors), n_factors, factor_of, steps, init_feet, com0, static_cast<double *>(blocks), status);
}
// the clock of the launch into the context's buffer, then a lane per gait and kMoSampleChunk samples
template <bool LONG>
int mo_sample_launch(wg_ctx *ctx, int B, int smax, const void *blocks, const int *status, double t_start, double T, int lcap, const wg::MoOut &O, int *length, hipStream_t st) {
  if (int rc = use_ctx(ctx)) return rc;
  if (int rc = mo_sample_check<LONG>(B, smax, blocks, t_start, T, lcap)) return rc;
  if (B == 0) return WG_OK;
  std::lock_guard<std::mutex> launch_lk(ctx->launch_mu);
  if (int rc = slot_claim(ctx, ctx->mo_order, st, "Morisawa sample")) return rc;
  if (int rc = ctx->mo_clock.reserve((size_t)(lcap + 1) * sizeof(double))) return rc;
  double *clock = static_cast<double *>(ctx->mo_clock.p);
  hipLaunchKernelGGL(wg::wg_morisawa_clock_kernel, dim3(1), dim3(1), 0, st, t_start, T, lcap + 1, clock);
  HIP_TRY(hipGetLastError());
  const int chunks = (lcap + wg::kMoSampleChunk - 1) / wg::kMoSampleChunk;
  hipLaunchKernelGGL(wg::wg_morisawa_sample_kernel<LONG>, dim3((B + 63) / 64, chunks), dim3(64), 0, st, B, smax, static_cast<const double *>(blocks), status, clock, lcap, O, length);
  HIP_TRY(hipGetLastError());
  return slot_mark(ctx->mo_order, st);
}
// solve, then sample, on the caller's stream: the stream orders them, the host does not wait
template <bool FLEET, bool LONG>
int mo_walk_launch(wg_ctx *ctx, const wg_morisawa_model_t *mf, double T, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, const double *com0, void *blocks, int *status, double t_start, int lcap, const wg::MoOut &O, int *length, hipStream_t st) {
  if (int rc = mo_solve_check<LONG>(mf, B, smax, steps, n_steps, init_feet, com0, blocks, status)) return rc;
  if (!FLEET) T = mf->T;
  if (int rc = mo_sample_check<LONG>(B, smax, blocks, t_start, T, lcap)) return rc;
  if (int rc = mo_solve_launch<FLEET, LONG>(ctx, mf, B, smax, steps, n_steps, init_feet, com0, blocks, status, st)) return rc;
  return mo_sample_launch<LONG>(ctx, B, smax, blocks, status, t_start, T, lcap, O, length, st);
}

}  // namespace

extern "C" {

#define WG_MO_ENTRIES_(stem, LONG)                                                                                                              \
  int stem##solve_dev_ctx(wg_ctx_t *ctx, const wg_morisawa_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, const double *com0, void *blocks, int *status, void *hip_stream) { \
    return mo_solve_launch<false, LONG>(ctx, model, B, smax, steps, n_steps, init_feet, com0, blocks, status, reinterpret_cast<hipStream_t>(hip_stream)); \
  }                                                                                                                                             \
  int stem##solve_fleet_dev_ctx(wg_ctx_t *ctx, const wg_morisawa_model_t *models, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, const double *com0, void *blocks, int *status, void *hip_stream) { \
    return mo_solve_launch<true, LONG>(ctx, models, B, smax, steps, n_steps, init_feet, com0, blocks, status, reinterpret_cast<hipStream_t>(hip_stream)); \
  }                                                                                                                                             \
  int stem##resolve_dev_ctx(wg_ctx_t *ctx, const wg_morisawa_model_t *model, int B, int smax, const void *factors, int n_factors, const int *factor_of, const wg_rel_step_t *steps, const double *init_feet, const double *com0, void *blocks, int *status, void *hip_stream) { \
    return mo_resolve_launch<false, LONG>(ctx, model, B, smax, factors, n_factors, factor_of, steps, init_feet, com0, blocks, status, reinterpret_cast<hipStream_t>(hip_stream)); \
  }                                                                                                                                             \
  int stem##resolve_fleet_dev_ctx(wg_ctx_t *ctx, const wg_morisawa_model_t *models, int B, int smax, const void *factors, int n_factors, const int *factor_of, const wg_rel_step_t *steps, const double *init_feet, const double *com0, void *blocks, int *status, void *hip_stream) { \
    return mo_resolve_launch<true, LONG>(ctx, models, B, smax, factors, n_factors, factor_of, steps, init_feet, com0, blocks, status, reinterpret_cast<hipStream_t>(hip_stream)); \
  }                                                                                                                                             \
  int stem##sample_dev_ctx(wg_ctx_t *ctx, int B, int smax, const void *blocks, const int *status, double t_start, double T, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *com_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, int *length, void *hip_stream) { \
    const wg::MoOut O{zmp_x_tm, zmp_y_tm, com_tm, left_tm, right_tm, left_type_tm, right_type_tm};                                               \
    return mo_sample_launch<LONG>(ctx, B, smax, blocks, status, t_start, T, lcap, O, length, reinterpret_cast<hipStream_t>(hip_stream));         \
  }                                                                                                                                             \
  int stem##walk_dev_ctx(wg_ctx_t *ctx, const wg_morisawa_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, const double *com0, void *blocks, int *status, double t_start, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *com_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, int *length, void *hip_stream) { \
    const wg::MoOut O{zmp_x_tm, zmp_y_tm, com_tm, left_tm, right_tm, left_type_tm, right_type_tm};                                               \
    return mo_walk_launch<false, LONG>(ctx, model, 0.0, B, smax, steps, n_steps, init_feet, com0, blocks, status, t_start, lcap, O, length, reinterpret_cast<hipStream_t>(hip_stream)); \
  }                                                                                                                                             \
  int stem##walk_fleet_dev_ctx(wg_ctx_t *ctx, const wg_morisawa_model_t *models, double T, int B, int smax, const wg_rel_step_t *steps, const int *n_steps, const double *init_feet, const double *com0, void *blocks, int *status, double t_start, int lcap, double *zmp_x_tm, double *zmp_y_tm, double *com_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, int *length, void *hip_stream) { \
    const wg::MoOut O{zmp_x_tm, zmp_y_tm, com_tm, left_tm, right_tm, left_type_tm, right_type_tm};                                               \
    return mo_walk_launch<true, LONG>(ctx, models, T, B, smax, steps, n_steps, init_feet, com0, blocks, status, t_start, lcap, O, length, reinterpret_cast<hipStream_t>(hip_stream)); \
  }
WG_MO_ENTRIES_(wg_morisawa_, false)
WG_MO_ENTRIES_(wg_morisawa_long_, true)
#undef WG_MO_ENTRIES_

}  // extern "C"
