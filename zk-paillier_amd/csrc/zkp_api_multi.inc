// zkp_api_multi.inc — one caller, several GPUs (included by zkp_api.hip).
//
// Proofs are independent units (the reference spreads them, and the rows inside them, over a rayon pool:
// range_proof.rs:161-187,270-348): a batch is cut into contiguous blocks of proof indices, one block per
// device context, one host thread per context.  Two ways to reassemble the outputs (zkp_multi_set_gather):
//   ZKP_GATHER_HOST (default): every block writes its slab of the caller's HOST output arrays directly, the reassembly step is the
//     D2H copy of each slab (SURVEY §8(e): "if only the host needs the result, per-GPU D2H replaces the collective");
//   ZKP_GATHER_RCCL: north_star's "RCCL all-gather over xGMI to reassemble proof batches" inside this library — every context
//     computes on device-resident copies of its block and writes its output slab into ITS segment of a buffer that holds the whole
//     batch; ONE grouped ncclAllGather per output (verdict / status bytes; the c1 and c2 slabs of a prove call) over the contexts'
//     own streams then leaves the whole gathered output in the memory of EVERY GPU (zkp_multi_gathered), for a follow-on stage on
//     any of them (verify-after-prove), and the caller's host arrays are filled from ONE device's copy.  Blocks of unequal size are
//     padded to the largest (as zk-paillier_amd/shard.py does for the one-process-per-GPU layout).
#include <chrono>
#include <thread>
#include <rccl/rccl.h>      // types and prototypes only: the library itself is loaded on demand (below)

// RCCL is loaded when a caller first asks for ZKP_GATHER_RCCL, not when libzkp_hip.so is: a single-GPU user needs no RCCL installed
// (the same pattern as the latency engine, lat_engine()).  $ZKP_RCCL_LIB names the file; default librccl.so.1 by the loader's search
// path, then /opt/rocm/lib.
#define ZKP_RCCL_FUNCS(X) X(ncclCommInitAll) X(ncclCommDestroy) X(ncclGetErrorString) X(ncclGroupStart) X(ncclGroupEnd) X(ncclAllGather)
struct RcclLib {
  void* handle = nullptr;
  std::string why;          // why it could not be loaded
#define X(f) decltype(&f) p_##f = nullptr;
  ZKP_RCCL_FUNCS(X)
#undef X
};
static const RcclLib& rccl_lib() {
  static RcclLib lib;
  static std::once_flag once;
  std::call_once(once, [] {
    std::vector<std::string> names;
    if (const char* e = std::getenv("ZKP_RCCL_LIB")) names.push_back(e);
    else names = {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"};
    void* h = nullptr;
    for (const std::string& nm : names) {
      h = dlopen(nm.c_str(), RTLD_NOW | RTLD_LOCAL);
      if (h) break;
      const char* e = dlerror();
      lib.why += (lib.why.empty() ? "" : "; ") + nm + ": " + (e ? e : "dlopen failed");
    }
    if (!h) return;
    bool all = true;
#define X(f) lib.p_##f = (decltype(&f))dlsym(h, #f); all = all && lib.p_##f;
    ZKP_RCCL_FUNCS(X)
#undef X
    if (!all) { lib.why = "the RCCL library lacks an entry point this library calls"; dlclose(h); return; }
    lib.handle = h;
  });
  return lib;
}

// buffers of one device context in ZKP_GATHER_RCCL mode (grow-only, freed by zkp_multi_destroy)
struct MultiDev {
  DevBuf in[16];          // the staged inputs of this context's block
  DevBuf gathered[3];     // 0: verdict / status bytes, 1: c1, 2: c2 — the WHOLE batch, block i at i * stride
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};      // on the context's stream: its block starts | its block is computed | the gathers are done
};

struct zkp_multi {
  std::vector<zkp_ctx*> ctx;
  std::string err;
  uint32_t gather = ZKP_GATHER_HOST;
  std::vector<ncclComm_t> comm;        // one communicator per context (ncclCommInitAll), created by the first zkp_multi_set_gather(RCCL)
  std::vector<MultiDev> dev;
  uint64_t gathered_stride[3] = {0, 0, 0}, gathered_bytes[3] = {0, 0, 0};   // of the most recent call
  // the most recent batch call, per device context: the block it was given and the wall time of its call (H2D staging,
  // launches, D2H of its output slab) — what a driver on a multi-GPU node prints to see the shards side by side
  std::vector<double> last_ms;
  std::vector<uint64_t> last_lo, last_hi;
  // ... and, in the gathering modes, the two phases of that call on each device's own stream (events): its block's compute (staging
  // included) and the all-gather behind it — which ends when the SLOWEST peer has delivered, so it holds the wait for stragglers too
  std::vector<double> last_compute_ms, last_gather_ms;
};

// contiguous, balanced block of [0, total) owned by part i of parts (the first total % parts blocks get one more)
static void multi_block(uint64_t total, uint64_t parts, uint64_t i, uint64_t* lo, uint64_t* hi) {
  const uint64_t base = total / parts, extra = total % parts;
  *lo = i * base + std::min<uint64_t>(i, extra);
  *hi = *lo + base + (i < extra ? 1 : 0);
}

extern "C" int32_t zkp_multi_create(const int32_t* device_ids, uint32_t n_devices, zkp_multi** out) try {
  if (!out) return ZKP_EINVAL;
  *out = nullptr;
  if (!device_ids || n_devices == 0 || n_devices > 64) return ZKP_EINVAL;
  zkp_multi* m = new zkp_multi();
  for (uint32_t i = 0; i < n_devices; i++) {
    zkp_ctx* c = nullptr;
    const int32_t st = zkp_ctx_create(device_ids[i], &c);
    if (st) {
      for (zkp_ctx* d : m->ctx) (void)zkp_ctx_destroy(d);
      delete m;
      return st;
    }
    m->ctx.push_back(c);
  }
  *out = m;
  return ZKP_OK;
} ZKP_CATCH(nullptr)

extern "C" int32_t zkp_multi_destroy(zkp_multi* m) try {
  if (!m) return ZKP_EINVAL;
  for (size_t i = 0; i < m->dev.size(); i++) {
    (void)hipSetDevice(m->ctx[i]->device);
    (void)hipStreamSynchronize(m->ctx[i]->stream);
    for (DevBuf& b : m->dev[i].in) if (b.p) (void)hipFree(b.p);
    for (DevBuf& b : m->dev[i].gathered) if (b.p) (void)hipFree(b.p);
    for (hipEvent_t& e : m->dev[i].ev) if (e) (void)hipEventDestroy(e);
  }
  for (ncclComm_t cm : m->comm) (void)rccl_lib().p_ncclCommDestroy(cm);
  for (zkp_ctx* c : m->ctx) (void)zkp_ctx_destroy(c);
  delete m;
  return ZKP_OK;
} ZKP_CATCH(nullptr)

#define NCCLCHK(m, call)                                                                          \
  do {                                                                                            \
    ncclResult_t r_ = rccl_lib().p_##call;                                                        \
    if (r_ != ncclSuccess) {                                                                      \
      (m)->err = std::string(#call) + ": " + rccl_lib().p_ncclGetErrorString(r_);                              \
      return ZKP_EDEVICE;                                                                         \
    }                                                                                             \
  } while (0)

extern "C" int32_t zkp_multi_set_gather(zkp_multi* m, uint32_t mode) try {
  if (!m || (mode != ZKP_GATHER_HOST && mode != ZKP_GATHER_RCCL && mode != ZKP_GATHER_COPY)) return ZKP_EINVAL;
  if (mode == ZKP_GATHER_COPY && m->dev.empty()) m->dev.resize(m->ctx.size());
  if (mode == ZKP_GATHER_RCCL && m->comm.empty()) {
    if (!rccl_lib().handle) { m->err = "zkp_multi_set_gather: RCCL could not be loaded (" + rccl_lib().why + ")"; return ZKP_EDEVICE; }
    // one process, one communicator per device: ncclCommInitAll (a device listed twice has no communicator: RCCL's error text)
    std::vector<int> devs;
    for (zkp_ctx* c : m->ctx) devs.push_back(c->device);
    for (size_t i = 0; i < devs.size(); i++)
      for (size_t k = 0; k < i; k++)
        if (devs[i] == devs[k]) { m->err = "zkp_multi_set_gather: device " + std::to_string(devs[i]) + " is listed twice: an RCCL communicator needs distinct GPUs"; return ZKP_EDEVICE; }
    std::vector<ncclComm_t> comm(devs.size());
    NCCLCHK(m, ncclCommInitAll(comm.data(), (int)devs.size(), devs.data()));
    m->comm = comm;
    m->dev.resize(devs.size());
  }
  m->gather = mode;
  return ZKP_OK;
} ZKP_CATCH(nullptr)

extern "C" int32_t zkp_multi_gathered(zkp_multi* m, uint32_t device_index, uint32_t which, void** out_device_ptr, uint64_t* out_block_stride_bytes,
                                      uint64_t* out_bytes) {
  if (!m || device_index >= m->dev.size() || which > 2 || !m->gathered_bytes[which]) return ZKP_EINVAL;
  if (out_device_ptr) *out_device_ptr = m->dev[device_index].gathered[which].p;
  if (out_block_stride_bytes) *out_block_stride_bytes = m->gathered_stride[which];
  if (out_bytes) *out_bytes = m->gathered_bytes[which];
  return ZKP_OK;
}

extern "C" uint32_t zkp_multi_size(zkp_multi* m) { return m ? (uint32_t)m->ctx.size() : 0; }
extern "C" zkp_ctx* zkp_multi_ctx(zkp_multi* m, uint32_t i) { return (m && i < m->ctx.size()) ? m->ctx[i] : nullptr; }
extern "C" const char* zkp_multi_last_error_string(zkp_multi* m) { return m ? m->err.c_str() : "null handle"; }
extern "C" int32_t zkp_multi_last_timing(zkp_multi* m, uint32_t i, double* out_ms, uint64_t* out_lo, uint64_t* out_hi) {
  if (!m || i >= m->last_ms.size()) return ZKP_EINVAL;
  if (out_ms) *out_ms = m->last_ms[i];
  if (out_lo) *out_lo = m->last_lo[i];
  if (out_hi) *out_hi = m->last_hi[i];
  return ZKP_OK;
}

extern "C" int32_t zkp_multi_last_phases(zkp_multi* m, uint32_t i, double* out_compute_ms, double* out_gather_ms) {
  if (!m || i >= m->last_compute_ms.size()) return ZKP_EINVAL;
  if (out_compute_ms) *out_compute_ms = m->last_compute_ms[i];
  if (out_gather_ms) *out_gather_ms = m->last_gather_ms[i];
  return ZKP_OK;
}
// phase events of context i (gathering modes only: m->dev is sized there); a failure to create one just leaves the phases unreported
static hipEvent_t multi_phase_event(zkp_multi* m, size_t i, int k) {
  if (i >= m->dev.size()) return nullptr;
  hipEvent_t& e = m->dev[i].ev[k];
  if (!e && hipEventCreate(&e) != hipSuccess) e = nullptr;
  return e;
}
static void multi_phase_mark(zkp_multi* m, size_t i, int k) {
  if (hipEvent_t e = multi_phase_event(m, i, k)) (void)hipEventRecord(e, m->ctx[i]->stream);
}
// after the streams are drained: event times -> last_compute_ms / last_gather_ms
static void multi_phase_collect(zkp_multi* m) {
  for (size_t i = 0; i < m->dev.size() && i < m->last_compute_ms.size(); i++) {
    if (m->last_lo[i] == m->last_hi[i]) continue;
    float a = 0, b = 0;
    hipEvent_t* e = m->dev[i].ev;
    if (e[0] && e[1] && hipEventElapsedTime(&a, e[0], e[1]) == hipSuccess) m->last_compute_ms[i] = a;
    if (e[1] && e[2] && hipEventElapsedTime(&b, e[1], e[2]) == hipSuccess) m->last_gather_ms[i] = b;
  }
}

// run fn(part, ctx, lo, hi) on one thread per context; first non-zero status wins
template <class F> static int32_t multi_run(zkp_multi* m, uint64_t total, F fn) {
  const uint64_t parts = m->ctx.size();
  std::vector<int32_t> st(parts, ZKP_OK);
  std::vector<std::thread> th;
  m->last_ms.assign(parts, 0.0); m->last_lo.assign(parts, 0); m->last_hi.assign(parts, 0);
  m->last_compute_ms.assign(parts, 0.0); m->last_gather_ms.assign(parts, 0.0);
  auto timed = [&](uint64_t i, uint64_t lo, uint64_t hi) {
    const auto t0 = std::chrono::steady_clock::now();
    if (m->gather != ZKP_GATHER_HOST && hipSetDevice(m->ctx[i]->device) == hipSuccess) multi_phase_mark(m, i, 0);
    st[i] = fn(m->ctx[i], lo, hi);
    if (m->gather != ZKP_GATHER_HOST) multi_phase_mark(m, i, 1);
    m->last_ms[i] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (m->gather == ZKP_GATHER_HOST) m->last_compute_ms[i] = m->last_ms[i];      // (a blocking call per device: its wall time is its compute)
  };
  for (uint64_t i = 0; i < parts; i++) {
    uint64_t lo, hi;
    multi_block(total, parts, i, &lo, &hi);
    m->last_lo[i] = lo; m->last_hi[i] = hi;
    if (lo == hi) continue;
    try {
      th.emplace_back([&, i, lo, hi] { timed(i, lo, hi); });
    } catch (...) {                     // no thread for this block: run it here, after the others were started
      timed(i, lo, hi);
    }
  }
  for (auto& t : th) t.join();
  for (uint64_t i = 0; i < parts; i++)
    if (st[i]) {
      m->err = "device context " + std::to_string(i) + ": " + m->ctx[i]->err;
      return st[i];
    }
  return ZKP_OK;
}

// ---- ZKP_GATHER_RCCL ------------------------------------------------------------------------------------------------------------
// stage `bytes` of host memory into input buffer `slot` of context i (its stream, its device) -> device pointer
static int32_t multi_stage_in(zkp_multi* m, size_t i, int slot, const void* host, size_t bytes, const void** out) {
  zkp_ctx* c = m->ctx[i];
  *out = nullptr;
  if (!host || !bytes) return ZKP_OK;
  int32_t st = ensure(c, m->dev[i].in[slot], bytes);
  if (st) return st;
  HIPCHK(c, hipMemcpyAsync(m->dev[i].in[slot].p, host, bytes, hipMemcpyHostToDevice, c->stream));
  *out = m->dev[i].in[slot].p;
  return ZKP_OK;
}

// One grouped all-gather of output `which` (block stride `stride` bytes, in place: context i's slab already sits at i * stride of
// its own buffer) over the contexts' streams, issued from this one thread between ncclGroupStart / ncclGroupEnd.
static int32_t multi_sync_all(zkp_multi* m, bool after_gather);
static int32_t multi_all_gather(zkp_multi* m, int which, uint64_t stride) {
  const size_t parts = m->ctx.size();
  if (m->gather == ZKP_GATHER_COPY) {
    // the same exchange by device-to-device copies: every context fetches every other context's segment (for device lists RCCL
    // has no communicator for — one GPU listed several times — and as a check of the padded layout on a 1-GPU box)
    int32_t st = multi_sync_all(m, false);
    if (st) return st;
    for (size_t i = 0; i < parts; i++) {
      zkp_ctx* c = m->ctx[i];
      HIPCHK(c, hipSetDevice(c->device));
      for (size_t j = 0; j < parts; j++)
        if (j != i) HIPCHK(c, hipMemcpyAsync((char*)m->dev[i].gathered[which].p + j * stride, (const char*)m->dev[j].gathered[which].p + j * stride, stride, hipMemcpyDeviceToDevice, c->stream));
    }
    m->gathered_stride[which] = stride; m->gathered_bytes[which] = stride * parts;
    return ZKP_OK;
  }
  NCCLCHK(m, ncclGroupStart());
  for (size_t i = 0; i < parts; i++) {
    if (hipSetDevice(m->ctx[i]->device) != hipSuccess) { (void)rccl_lib().p_ncclGroupEnd(); m->err = "hipSetDevice"; return ZKP_EDEVICE; }
    char* buf = (char*)m->dev[i].gathered[which].p;
    const ncclResult_t r = rccl_lib().p_ncclAllGather(buf + i * stride, buf, stride, ncclUint8, m->comm[i], m->ctx[i]->stream);
    if (r != ncclSuccess) { (void)rccl_lib().p_ncclGroupEnd(); m->err = std::string("ncclAllGather: ") + rccl_lib().p_ncclGetErrorString(r); return ZKP_EDEVICE; }
  }
  NCCLCHK(m, ncclGroupEnd());
  m->gathered_stride[which] = stride; m->gathered_bytes[which] = stride * parts;
  return ZKP_OK;
}

// the gathered (padded) output `which` of device 0 -> the caller's host array, block by block
static int32_t multi_gathered_to_host(zkp_multi* m, int which, uint64_t total, uint64_t unit_bytes, void* host) {
  if (!host) return ZKP_OK;
  const size_t parts = m->ctx.size();
  zkp_ctx* c = m->ctx[0];
  HIPCHK(c, hipSetDevice(c->device));
  for (size_t i = 0; i < parts; i++) {
    uint64_t lo, hi;
    multi_block(total, parts, i, &lo, &hi);
    if (hi > lo) HIPCHK(c, hipMemcpyAsync((char*)host + lo * unit_bytes, (char*)m->dev[0].gathered[which].p + i * m->gathered_stride[which], (hi - lo) * unit_bytes, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ZKP_OK;
}

// drain every context's stream.  `after_gather`: the gathers of this call are enqueued — close the phase clock behind them
static int32_t multi_sync_all(zkp_multi* m, bool after_gather) {
  for (size_t i = 0; i < m->ctx.size(); i++) {
    zkp_ctx* c = m->ctx[i];
    if (hipSetDevice(c->device) != hipSuccess) { m->err = "hipSetDevice"; return ZKP_EDEVICE; }
    if (after_gather && i < m->last_lo.size() && m->last_lo[i] != m->last_hi[i]) multi_phase_mark(m, i, 2);
  }
  for (zkp_ctx* c : m->ctx) {
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { m->err = "stream synchronize after the gather"; return ZKP_EDEVICE; }
  }
  if (after_gather) multi_phase_collect(m);
  return ZKP_OK;
}

// largest block of `total` over `parts`
static uint64_t multi_max_block(uint64_t total, uint64_t parts) { return (total + parts - 1) / parts; }

// the [lo, hi) block of a proof batch (host pointers)
static zkp_range_ni_proofs range_slice(const zkp_range_ni_proofs& p, uint64_t lo, uint64_t hi) {
  const uint64_t kw = p.n_bits / 32, EF = p.error_factor;
  zkp_range_ni_proofs s = p;
  s.batch = hi - lo;
  auto adv32 = [&](auto* q, uint64_t words_per_proof) { return q ? q + lo * words_per_proof : q; };
  s.n = p.n_stride ? adv32(p.n, p.n_stride) : p.n;
  s.range = adv32(p.range, kw);
  s.ciphertext = adv32(p.ciphertext, 2 * kw);
  s.c1 = adv32(p.c1, EF * 2 * kw); s.c2 = adv32(p.c2, EF * 2 * kw);
  s.resp_kind = adv32(p.resp_kind, EF); s.resp_j = adv32(p.resp_j, EF);
  s.resp_w1 = adv32(p.resp_w1, EF * kw); s.resp_r1 = adv32(p.resp_r1, EF * kw);
  s.resp_w2 = adv32(p.resp_w2, EF * kw); s.resp_r2 = adv32(p.resp_r2, EF * kw);
  return s;
}

// the block [lo, hi) of a host proof batch staged into context i's input buffers -> the same struct with device pointers
static int32_t multi_stage_range(zkp_multi* m, size_t i, const zkp_range_ni_proofs& host_slice, bool with_pairs_and_responses, zkp_range_ni_proofs* d) {
  const uint64_t kw = host_slice.n_bits / 32, EF = host_slice.error_factor, B = host_slice.batch;
  *d = host_slice;
  const void* q;
  int32_t st = multi_stage_in(m, i, 0, host_slice.n, (host_slice.n_stride ? B : 1) * kw * 4, &q); d->n = (const uint32_t*)q;
  if (!st) { st = multi_stage_in(m, i, 1, host_slice.range, B * kw * 4, &q); d->range = (const uint32_t*)q; }
  if (!st) { st = multi_stage_in(m, i, 2, host_slice.ciphertext, B * 2 * kw * 4, &q); d->ciphertext = (const uint32_t*)q; }
  if (with_pairs_and_responses) {
    if (!st) { st = multi_stage_in(m, i, 3, host_slice.c1, B * EF * 2 * kw * 4, &q); d->c1 = (uint32_t*)q; }
    if (!st) { st = multi_stage_in(m, i, 4, host_slice.c2, B * EF * 2 * kw * 4, &q); d->c2 = (uint32_t*)q; }
    if (!st) { st = multi_stage_in(m, i, 5, host_slice.resp_kind, B * EF, &q); d->resp_kind = (uint8_t*)q; }
    if (!st) { st = multi_stage_in(m, i, 6, host_slice.resp_j, B * EF, &q); d->resp_j = (uint8_t*)q; }
    if (!st) { st = multi_stage_in(m, i, 7, host_slice.resp_w1, B * EF * kw * 4, &q); d->resp_w1 = (uint32_t*)q; }
    if (!st) { st = multi_stage_in(m, i, 8, host_slice.resp_r1, B * EF * kw * 4, &q); d->resp_r1 = (uint32_t*)q; }
    if (!st) { st = multi_stage_in(m, i, 9, host_slice.resp_w2, B * EF * kw * 4, &q); d->resp_w2 = (uint32_t*)q; }
    if (!st) { st = multi_stage_in(m, i, 10, host_slice.resp_r2, B * EF * kw * 4, &q); d->resp_r2 = (uint32_t*)q; }
  }
  return st;
}

// ZKP_GATHER_RCCL flavour of a verdict-producing call: fn(ctx, i, lo, hi, device verdict slab) enqueues context i's work
template <class F> static int32_t multi_run_gather_bytes(zkp_multi* m, uint64_t total, uint8_t* out_host, F fn) {
  const uint64_t parts = m->ctx.size(), stride = multi_max_block(total, parts);
  for (uint64_t i = 0; i < parts; i++) {
    zkp_ctx* c = m->ctx[i];
    HIPCHK(c, hipSetDevice(c->device));
    const int32_t st = ensure(c, m->dev[i].gathered[0], stride * parts);
    if (st) { m->err = "device context " + std::to_string(i) + ": " + c->err; return st; }
    HIPCHK(c, hipMemsetAsync(m->dev[i].gathered[0].p, 0, stride * parts, c->stream));
  }
  int32_t st = multi_run(m, total, [&](zkp_ctx* c, uint64_t lo, uint64_t hi) {
    size_t i = 0;
    while (m->ctx[i] != c) i++;
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice"; return (int32_t)ZKP_EDEVICE; }
    return fn(c, i, lo, hi, (uint8_t*)m->dev[i].gathered[0].p + i * stride);
  });
  if (!st) st = multi_all_gather(m, 0, stride);
  if (!st) st = multi_sync_all(m, true);
  if (!st) st = multi_gathered_to_host(m, 0, total, 1, out_host);
  if (st && m->err.empty()) m->err = m->ctx[0]->err;
  return st;
}

extern "C" int32_t zkp_multi_range_ni_verify_batch(zkp_multi* m, const zkp_range_ni_proofs* p, uint8_t* out_verdict) try {
  if (!m || !p) return ZKP_EINVAL;
  if (p->batch == 0) return ZKP_OK;
  if (m->gather != ZKP_GATHER_HOST)
    return multi_run_gather_bytes(m, p->batch, out_verdict, [&](zkp_ctx* c, size_t i, uint64_t lo, uint64_t hi, uint8_t* d_verdict) {
      const zkp_range_ni_proofs s = range_slice(*p, lo, hi);
      zkp_range_ni_proofs d;
      const int32_t st = multi_stage_range(m, i, s, true, &d);
      return st ? st : zkp_range_ni_verify_batch(c, &d, d_verdict, ZKP_F_DEVICE_PTRS);
    });
  return multi_run(m, p->batch, [&](zkp_ctx* c, uint64_t lo, uint64_t hi) {
    const zkp_range_ni_proofs s = range_slice(*p, lo, hi);
    return zkp_range_ni_verify_batch(c, &s, out_verdict ? out_verdict + lo : nullptr, 0);
  });
} ZKP_CATCH(nullptr)

extern "C" int32_t zkp_multi_range_ni_prove_batch(zkp_multi* m, const zkp_range_ni_proofs* p, const zkp_range_ni_witness* w, uint8_t* out_e,
                                                  uint8_t* out_e_len, uint8_t* out_status) try {
  if (!m || !p || !w) return ZKP_EINVAL;
  if (p->batch == 0) return ZKP_OK;
  const uint64_t kw = p->n_bits / 32, EF = ZKP_SECURITY_PARAMETER;
  if (m->gather != ZKP_GATHER_HOST) {
    // c1 / c2 (the 128 KiB per proof that a verifier, or a verify-after-prove stage, consumes) and the status bytes are gathered on
    // every GPU; the responses and challenge bytes of a block go to the caller's host arrays from the GPU that made them
    const uint64_t parts = m->ctx.size(), B = p->batch, blk = multi_max_block(B, parts), pair_stride = blk * EF * 2 * kw * 4;
    if (!p->c1 || !p->c2) { m->err = "zkp_multi_range_ni_prove_batch: c1 / c2 are required"; return ZKP_EINVAL; }
    for (uint64_t i = 0; i < parts; i++) {
      zkp_ctx* c = m->ctx[i];
      HIPCHK(c, hipSetDevice(c->device));
      int32_t st = ensure(c, m->dev[i].gathered[0], blk * parts);
      if (!st) st = ensure(c, m->dev[i].gathered[1], pair_stride * parts);
      if (!st) st = ensure(c, m->dev[i].gathered[2], pair_stride * parts);
      if (st) { m->err = "device context " + std::to_string(i) + ": " + c->err; return st; }
      HIPCHK(c, hipMemsetAsync(m->dev[i].gathered[0].p, 0, blk * parts, c->stream));
    }
    int32_t st = multi_run(m, B, [&](zkp_ctx* c, uint64_t lo, uint64_t hi) {
      size_t i = 0;
      while (m->ctx[i] != c) i++;
      if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice"; return (int32_t)ZKP_EDEVICE; }
      const uint64_t nb = hi - lo, rows = nb * EF;
      zkp_range_ni_proofs s = *p;
      s.error_factor = (uint32_t)EF;
      s = range_slice(s, lo, hi);
      zkp_range_ni_proofs d;
      int32_t st2 = multi_stage_range(m, i, s, false, &d);
      d.error_factor = p->error_factor;
      // outputs: c1 / c2 straight into this context's segment of the gathered buffers, responses into staging blocks of the ctx
      d.c1 = (uint32_t*)((char*)m->dev[i].gathered[1].p + i * pair_stride);
      d.c2 = (uint32_t*)((char*)m->dev[i].gathered[2].p + i * pair_stride);
      DevBuf* rb = &m->dev[i].in[3];                // slots 3..8: kind, j, w1, r1, w2, r2 of this block (outputs here)
      const size_t rbytes[6] = {rows, rows, rows * kw * 4, rows * kw * 4, rows * kw * 4, rows * kw * 4};
      for (int q = 0; q < 6 && !st2; q++) st2 = ensure(c, rb[q], rbytes[q]);
      if (st2) return st2;
      d.resp_kind = (uint8_t*)rb[0].p; d.resp_j = (uint8_t*)rb[1].p;
      d.resp_w1 = (uint32_t*)rb[2].p; d.resp_r1 = (uint32_t*)rb[3].p; d.resp_w2 = (uint32_t*)rb[4].p; d.resp_r2 = (uint32_t*)rb[5].p;
      zkp_range_ni_witness wd = *w;
      const void* q;
      const struct { const uint32_t* h; size_t words; const uint32_t** dst; } wi[6] = {
          {w->x ? w->x + lo * kw : nullptr, nb * kw, &wd.x}, {w->r ? w->r + lo * kw : nullptr, nb * kw, &wd.r},
          {w->w1 ? w->w1 + lo * EF * kw : nullptr, rows * kw, &wd.w1}, {w->w2 ? w->w2 + lo * EF * kw : nullptr, rows * kw, &wd.w2},
          {w->r1 ? w->r1 + lo * EF * kw : nullptr, rows * kw, &wd.r1}, {w->r2 ? w->r2 + lo * EF * kw : nullptr, rows * kw, &wd.r2}};
      for (int k = 0; k < 6 && !st2; k++) { st2 = multi_stage_in(m, i, 9 + k, wi[k].h, wi[k].words * 4, &q); *wi[k].dst = (const uint32_t*)q; }
      DevBuf& eb = m->dev[i].in[15];                // challenge bytes + lengths of this block
      if (!st2) st2 = ensure(c, eb, nb * 33);
      if (st2) return st2;
      uint8_t* d_e = (uint8_t*)eb.p; uint8_t* d_elen = d_e + nb * 32;
      st2 = zkp_range_ni_prove_batch(c, &d, &wd, d_e, d_elen, (uint8_t*)m->dev[i].gathered[0].p + i * blk, ZKP_F_DEVICE_PTRS);
      if (st2) return st2;
      // this block's responses and challenge bytes -> the caller's host arrays (ordered on the ctx stream behind the kernels)
      const struct { void* h; void* dv; size_t n; } outs[8] = {
          {s.resp_kind, rb[0].p, rbytes[0]}, {s.resp_j, rb[1].p, rbytes[1]}, {s.resp_w1, rb[2].p, rbytes[2]}, {s.resp_r1, rb[3].p, rbytes[3]},
          {s.resp_w2, rb[4].p, rbytes[4]}, {s.resp_r2, rb[5].p, rbytes[5]}, {out_e ? out_e + lo * 32 : nullptr, d_e, nb * 32}, {out_e_len ? out_e_len + lo : nullptr, d_elen, nb}};
      for (auto& o : outs)
        if (o.h && hipMemcpyAsync(o.h, o.dv, o.n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) { c->err = "D2H copy of a response slab"; return (int32_t)ZKP_EDEVICE; }
      return (int32_t)ZKP_OK;
    });
    if (!st) st = multi_all_gather(m, 0, blk);
    if (!st) st = multi_all_gather(m, 1, pair_stride);
    if (!st) st = multi_all_gather(m, 2, pair_stride);
    if (!st) st = multi_sync_all(m, true);
    if (!st) st = multi_gathered_to_host(m, 0, B, 1, out_status);
    if (!st) st = multi_gathered_to_host(m, 1, B, EF * 2 * kw * 4, p->c1);
    if (!st) st = multi_gathered_to_host(m, 2, B, EF * 2 * kw * 4, p->c2);
    if (st && m->err.empty()) m->err = m->ctx[0]->err;
    return st;
  }
  return multi_run(m, p->batch, [&](zkp_ctx* c, uint64_t lo, uint64_t hi) {
    zkp_range_ni_proofs s = *p;
    s.error_factor = (uint32_t)EF;            // prove always writes ZKP_SECURITY_PARAMETER rows: slice with that row count
    s = range_slice(s, lo, hi);
    s.error_factor = p->error_factor;
    zkp_range_ni_witness ws = *w;
    if (w->x) ws.x = w->x + lo * kw;
    if (w->r) ws.r = w->r + lo * kw;
    if (w->w1) ws.w1 = w->w1 + lo * EF * kw;
    if (w->w2) ws.w2 = w->w2 + lo * EF * kw;
    if (w->r1) ws.r1 = w->r1 + lo * EF * kw;
    if (w->r2) ws.r2 = w->r2 + lo * EF * kw;
    return zkp_range_ni_prove_batch(c, &s, &ws, out_e ? out_e + lo * 32 : nullptr, out_e_len ? out_e_len + lo : nullptr,
                                    out_status ? out_status + lo : nullptr, 0);
  });
} ZKP_CATCH(nullptr)

// zkp_range_ni_prove_seeded_batch over the contexts: block i expands the witness of ITS proof indices (first_index + lo), so the bytes are
// those of one single-context call.  The per-GPU D2H reassembly only (ZKP_GATHER_HOST).
extern "C" int32_t zkp_multi_range_ni_prove_seeded_batch(zkp_multi* m, const zkp_range_ni_proofs* p, const uint32_t* x, const uint32_t* r,
                                                         const uint8_t* seed, uint64_t first_index, uint8_t* out_e, uint8_t* out_e_len,
                                                         uint8_t* out_status) try {
  if (!m) return ZKP_EINVAL;
  if (!p || !seed) { m->err = "zkp_multi_range_ni_prove_seeded_batch: invalid argument"; return ZKP_EINVAL; }
  if (m->gather != ZKP_GATHER_HOST) { m->err = "zkp_multi_range_ni_prove_seeded_batch: ZKP_GATHER_HOST only"; return ZKP_EINVAL; }
  if (p->batch == 0) return ZKP_OK;
  const uint64_t kw = p->n_bits / 32, EF = ZKP_SECURITY_PARAMETER;
  return multi_run(m, p->batch, [&](zkp_ctx* c, uint64_t lo, uint64_t hi) {
    zkp_range_ni_proofs s = *p;
    s.error_factor = (uint32_t)EF;            // prove always writes ZKP_SECURITY_PARAMETER rows: slice with that row count
    s = range_slice(s, lo, hi);
    s.error_factor = p->error_factor;
    return zkp_range_ni_prove_seeded_batch(c, &s, x ? x + lo * kw : nullptr, r ? r + lo * kw : nullptr, seed, first_index + lo,
                                           out_e ? out_e + lo * 32 : nullptr, out_e_len ? out_e_len + lo : nullptr, out_status ? out_status + lo : nullptr, 0);
  });
} ZKP_CATCH(nullptr)

extern "C" int32_t zkp_multi_correct_key_ni_verify_batch(zkp_multi* m, uint32_t n_bits, uint64_t batch, const uint32_t* n, const uint32_t* sigma,
                                                         const uint8_t* salt, uint32_t salt_len, uint8_t* out_verdict) try {
  if (!m) return ZKP_EINVAL;
  if (batch == 0) return ZKP_OK;
  if (!n || !sigma || !out_verdict) return ZKP_EINVAL;
  const uint64_t kw = n_bits / 32;
  if (m->gather != ZKP_GATHER_HOST)
    return multi_run_gather_bytes(m, batch, out_verdict, [&](zkp_ctx* c, size_t i, uint64_t lo, uint64_t hi, uint8_t* d_verdict) {
      const void *dn, *ds;
      int32_t st = multi_stage_in(m, i, 0, n + lo * kw, (hi - lo) * kw * 4, &dn);
      if (!st) st = multi_stage_in(m, i, 1, sigma + lo * ZKP_CORRECT_KEY_M2 * kw, (hi - lo) * ZKP_CORRECT_KEY_M2 * kw * 4, &ds);
      // (the salt is a host byte string in both memory modes)
      return st ? st : zkp_correct_key_ni_verify_batch(c, n_bits, hi - lo, (const uint32_t*)dn, (const uint32_t*)ds, salt, salt_len, d_verdict, ZKP_F_DEVICE_PTRS);
    });
  return multi_run(m, batch, [&](zkp_ctx* c, uint64_t lo, uint64_t hi) {
    return zkp_correct_key_ni_verify_batch(c, n_bits, hi - lo, n + lo * kw, sigma + lo * ZKP_CORRECT_KEY_M2 * kw, salt, salt_len, out_verdict + lo, 0);
  });
} ZKP_CATCH(nullptr)
