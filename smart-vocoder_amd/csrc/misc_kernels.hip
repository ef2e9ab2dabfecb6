// Small memory-bound kernels of the inference path (everything that is not a convolution GEMM).
#include "svoc_internal.h"

#include <cstdlib>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <mutex>
#include <map>
#include <set>
#include <tuple>
#include <vector>

namespace svoc {

// diagnostics: kernels that support phase stamps write them here when set (svoc_debug_set_stamp_buffer)
int xcd_mapping_enabled() { return 1; }                     // XCD-aware tile order (xcd_linear); the natural order was an A/B switch until round 5

static std::atomic<int> g_variant_batch{getenv("SVOC_VARIANT_BATCH") ? atoi(getenv("SVOC_VARIANT_BATCH")) : 0};
int variant_batch(int B) { const int v = g_variant_batch.load(std::memory_order_relaxed); return v > 0 ? v : B; }
int set_variant_batch(int n) { return g_variant_batch.exchange(n > 0 ? n : 0); }

static std::mutex g_dev_mu;
// Fewest workgroup tiles for which the MRF's grouped / paired / accumulate Winograd launches are taken instead of the K-split and direct kernels on
// three streams: half a tile per CU.  (Two per CU until round 5 - round 3's break-even for the F(2,3) kernels; with the F(4,4) kernels, ms per
// call at 2 / 1 / 0.5 / 0.25 / 0 tiles per CU: 1 x 200 2.56 / 2.55 / 2.44 / 2.52 / 2.52, 1 x 512 4.33 / 3.86 / 3.71 / 3.70 / 3.72, 4 x 512 unchanged:
// profiles/r05_small_shape_tile_gates.txt.)
long long mrf_min_tiles() {
  static const long long cfg = getenv("SVOC_MRF_MIN_TILES") ? atoll(getenv("SVOC_MRF_MIN_TILES")) : -1;      // tunable, as SVOC_CT_MIN_TILES
  return cfg >= 0 ? cfg : device_cu_count() / 2;
}
int device_cu_count() {
  static int cus[64] = {};
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return 256;
  std::lock_guard<std::mutex> lk(g_dev_mu);
  if (cus[d] == 0) {
    int n = 0;
    cus[d] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess && n > 0) ? n : 256;
  }
  return cus[d];
}
int ensure_max_dyn_lds(const void* kernel) {
  static std::set<std::pair<const void*, int>> done;
  int d = 0;
  SVOC_HIP(hipGetDevice(&d));
  std::lock_guard<std::mutex> lk(g_dev_mu);
  if (done.count({kernel, d})) return SVOC_OK;
  SVOC_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  done.insert({kernel, d});
  return SVOC_OK;
}

// Asynchronous failures of the persistent launches (wn_stack.hip, wn_mesh.hip): their workgroups wait for each other, the waits are bounded by wall
// time (SVOC_PERSIST_TIMEOUT_MS, default 2000), and a workgroup that gives up (a) turns its part of the SAME call's result into NaN - its mask
// factor becomes NaN, so its x tile, the edges its neighbours fetch and its rows of the stack's output are NaN and the waveform of the call is not
// finite - and (b) raises this word - pinned host memory the device writes through, so the host can read it without a synchronisation.  The word is
// looked at when the next call comes in (WNStack::forward, Synth::infer) and through svoc_check_async_error(); the first time it is found raised the
// process stops taking the persistent launches (the per-layer kernels compute the same function): persist_disabled().
static int* g_async_err = nullptr;
int* async_error_word() {
  std::lock_guard<std::mutex> lk(g_dev_mu);
  if (!g_async_err) {
    void* q = nullptr;
    if (hipHostMalloc(&q, 64, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    memset(q, 0, 64);
    g_async_err = static_cast<int*>(q);
  }
  return g_async_err;
}
static std::atomic<int> g_persist_off{0}, g_persist_fault{-1}, g_persist_timeout_ms{-1};
static std::atomic<unsigned> g_persist_epoch{0};
bool persist_disabled() { return g_persist_off.load(std::memory_order_relaxed) != 0; }
int persist_fault_tile() { return g_persist_fault.load(std::memory_order_relaxed); }
unsigned persist_epoch() { return g_persist_epoch.load(std::memory_order_relaxed); }
int persist_timeout_ms() {
  static const int env = [] {
    const char* e = getenv("SVOC_PERSIST_TIMEOUT_MS");
    const long v = e ? atol(e) : 2000;
    return (int)std::min<long>(std::max<long>(v, 1), 600000);
  }();
  const int o = g_persist_timeout_ms.load(std::memory_order_relaxed);
  return o > 0 ? o : env;
}
unsigned long long persist_timeout_ticks() { return (unsigned long long)persist_timeout_ms() * 100000ull; }      // s_memrealtime: 100 MHz
int persist_control(int fault_tile, int timeout_ms, int reenable) {
  g_persist_fault.store(fault_tile, std::memory_order_relaxed);
  g_persist_timeout_ms.store(timeout_ms, std::memory_order_relaxed);
  if (reenable) g_persist_off.store(0, std::memory_order_relaxed);
  g_persist_epoch.fetch_add(1, std::memory_order_relaxed);      // captured plans hold the old launch arguments: they are captured again
  return SVOC_OK;
}
int async_error_check() {
  int* w = g_async_err;
  if (!w) return SVOC_OK;
  if (__atomic_load_n(w, __ATOMIC_RELAXED) == 0) return SVOC_OK;
  if (__atomic_exchange_n(w, 0, __ATOMIC_ACQ_REL) == 0) return SVOC_OK;      // (another thread reported it)
  g_persist_off.store(1, std::memory_order_relaxed);
  g_persist_epoch.fetch_add(1, std::memory_order_relaxed);
  SVOC_FAIL(SVOC_ERR_HIP, "a persistent WN launch of an EARLIER call gave up waiting for its other workgroups after %d ms (SVOC_PERSIST_TIMEOUT_MS): the GPU "
                          "is shared by more work than the launch can be resident beside.  The outputs of that call are NaN where the launch gave up; this "
                          "process runs one launch per WN layer from now on (SVOC_WN_STACK=0 SVOC_WN_MESH=0 select that from the start)", persist_timeout_ms());
}
// Workgroups of `kernel` (block threads, dynamic LDS bytes) that the CURRENT device can hold at one time, as the runtime's occupancy calculator sees
// it - the residency the persistent launches need is asked for, not assumed (0: the query failed, the caller does not take the launch)
int persist_capacity(const void* kernel, int threads, size_t lds_bytes) {
  static std::map<std::tuple<const void*, int, int, size_t>, int> cache;
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) return 0;
  const auto key = std::make_tuple(kernel, d, threads, lds_bytes);
  {
    std::lock_guard<std::mutex> lk(g_dev_mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
  }
  if (ensure_max_dyn_lds(kernel) != SVOC_OK) return 0;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds_bytes) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }
  const int cap = per_cu > 0 ? per_cu * device_cu_count() : 0;
  std::lock_guard<std::mutex> lk(g_dev_mu);
  cache[key] = cap;
  return cap;
}

static long long* g_stamp_buffer = nullptr;
long long* debug_stamp_buffer() { return g_stamp_buffer; }
void set_debug_stamp_buffer(long long* p) { g_stamp_buffer = p; }


// ------------------------------------------------------------------ errors / stats
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* last_error() { return g_err; }

static std::atomic<long long> g_conv_launches{0}, g_other_launches{0}, g_convs{0};
static std::atomic<double> g_conv_flops{0.0}, g_exec_flops{0.0};
static inline void atomic_add(std::atomic<double>& a, double v) {
  double cur = a.load(std::memory_order_relaxed);
  while (!a.compare_exchange_weak(cur, cur + v, std::memory_order_relaxed)) {}
}
long long stats_convs() { return g_convs.load(); }
double stats_exec_flops() { return g_exec_flops.load(); }
void stats_add_conv(double flops, int nconv, double exec_flops) {
  g_conv_launches.fetch_add(1, std::memory_order_relaxed);
  g_convs.fetch_add(nconv, std::memory_order_relaxed);
  atomic_add(g_conv_flops, flops);
  atomic_add(g_exec_flops, exec_flops < 0 ? flops : exec_flops);
}
void stats_add_other() { g_other_launches.fetch_add(1, std::memory_order_relaxed); }
void stats_add_bulk(long long cl, double cf, long long ol, long long nc, double ef) {
  g_conv_launches.fetch_add(cl, std::memory_order_relaxed);
  g_convs.fetch_add(nc, std::memory_order_relaxed);
  g_other_launches.fetch_add(ol, std::memory_order_relaxed);
  atomic_add(g_conv_flops, cf);
  atomic_add(g_exec_flops, ef);
}
void stats_reset() { g_conv_launches = 0; g_other_launches = 0; g_conv_flops = 0.0; g_exec_flops = 0.0; g_convs = 0; }
void stats_get(long long* cl, double* cf, long long* ol) {
  if (cl) *cl = g_conv_launches.load();
  if (cf) *cf = g_conv_flops.load();
  if (ol) *ol = g_other_launches.load();
}

// ------------------------------------------------------------------ per-launch profiler (diagnostics only)
// When enabled, every convolution launch is bracketed with HIP events on its stream; the report aggregates
// by layer shape.  Off by default (events serialise nothing but cost a few microseconds per launch).
struct ProfRec { std::string desc; hipEvent_t e0, e1; double flops; };
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;
bool prof_enabled() { return g_prof_on; }
void prof_enable(bool on) {
  for (auto& r : g_prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  g_prof.clear();
  g_prof_on = on;
}
int prof_begin(hipStream_t st, const std::string& desc, double flops) {
  ProfRec r; r.desc = desc; r.flops = flops;
  if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return -1;
  (void)hipEventRecord(r.e0, st);
  g_prof.push_back(r);
  return (int)g_prof.size() - 1;
}
void prof_end(hipStream_t st, int idx) { if (idx >= 0) (void)hipEventRecord(g_prof[idx].e1, st); }
std::string prof_report() {
  std::map<std::string, std::pair<int, std::pair<double, double>>> agg;   // desc -> (n, (ms, flops))
  std::vector<std::string> order;
  for (auto& r : g_prof) {
    (void)hipEventSynchronize(r.e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.e0, r.e1);
    auto it = agg.find(r.desc);
    if (it == agg.end()) { order.push_back(r.desc); agg[r.desc] = {1, {ms, r.flops}}; }
    else { it->second.first++; it->second.second.first += ms; it->second.second.second += r.flops; }
  }
  std::string out = "layer-shape                                                      n   total_ms    mean_us   TFLOP/s\n";
  char line[256];
  double tms = 0, tfl = 0;
  for (auto& d : order) {
    auto& a = agg[d];
    snprintf(line, sizeof(line), "%-62s %5d %10.3f %10.1f %9.1f\n", d.c_str(), a.first, a.second.first,
             a.second.first * 1e3 / a.first, a.second.second / (a.second.first * 1e-3) / 1e12);
    out += line;
    tms += a.second.first; tfl += a.second.second;
  }
  snprintf(line, sizeof(line), "%-62s %5zu %10.3f %10s %9.1f\n", "TOTAL", g_prof.size(), tms, "", tms > 0 ? tfl / (tms * 1e-3) / 1e12 : 0.0);
  out += line;
  return out;
}

// ------------------------------------------------------------------ sequence mask (commons.py:121-125, models.py:40)
__global__ void sequence_mask_kernel(const int64_t* __restrict__ lengths, float* __restrict__ mask, int B, int T) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (t < T) mask[(long long)b * T + t] = ((int64_t)t < lengths[b]) ? 1.0f : 0.0f;
}
// ------------------------------------------------------------------ weight prefetch into the Infinity Cache
// The decoder moves ~5 MB per frame through the memory system, so by the time the next call's WN stacks run their weight images (99 MB for the five stacks
// of iitp_base) are neither in the L2s nor in the 256 MB memory-side cache, and a WN layer's weight stream - 2 MB that every XCD fetches for itself,
// requested three loads ahead - then waits on HBM latency: 44.0 -> 49.6 us per layer (tools/wn_in_step_probe.py, profiles/r06_wn_in_step_probe.txt; the
// in-step figure VERDICT r5 quotes is 49.9).  One streaming pass over the images at the head of the call puts them back into the memory-side cache.
// A block reads one segment of at most 64 KB, sixteen independent 16-byte loads per thread; the sum is only there so that the loads cannot be dropped.
__global__ void __launch_bounds__(256) prefetch_kernel(const PrefetchSeg* __restrict__ segs, float* __restrict__ sink) {
  const PrefetchSeg sg = segs[blockIdx.x];
  const float4* q = static_cast<const float4*>(sg.p);
  float4 v[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const unsigned i = threadIdx.x + 256u * u;
    v[u] = i < sg.n16 ? q[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float acc = 0.f;
#pragma unroll
  for (int u = 0; u < 16; ++u) acc += (v[u].x + v[u].y) + (v[u].z + v[u].w);
  if (acc == 1.2345678e38f) sink[0] = acc;
}
bool weight_prefetch_enabled() {
  static const bool on = !(getenv("SVOC_WN_PREFETCH") && atoi(getenv("SVOC_WN_PREFETCH")) == 0);      // SVOC_WN_PREFETCH=0: no prefetch pass (A/B)
  return on;
}
int WeightPrefetch::build(const std::vector<std::pair<const void*, size_t>>& bufs, hipStream_t st) {
  std::vector<PrefetchSeg> h;
  bytes = 0;
  for (const auto& b : bufs) {
    if (!b.first) continue;
    const char* q = static_cast<const char*>(b.first);
    for (size_t o = 0; o + 16 <= b.second; o += 65536) {
      PrefetchSeg sg{q + o, (unsigned)(std::min<size_t>(65536, b.second - o) / 16), 0u};
      h.push_back(sg);
    }
    bytes += b.second;
  }
  n = (int)h.size();
  if (n == 0) return SVOC_OK;
  SVOC_TRY(tab.ensure(h.size() * sizeof(PrefetchSeg) + 64));
  SVOC_HIP(hipMemcpyAsync(tab.p, h.data(), h.size() * sizeof(PrefetchSeg), hipMemcpyHostToDevice, st));
  SVOC_HIP(hipStreamSynchronize(st));                      // `h` lives on this stack frame
  return SVOC_OK;
}
int WeightPrefetch::run(hipStream_t st) const {
  if (n == 0 || !weight_prefetch_enabled()) return SVOC_OK;
  const PrefetchSeg* segs = static_cast<const PrefetchSeg*>(tab.p);
  hipLaunchKernelGGL(prefetch_kernel, dim3((unsigned)n), dim3(256), 0, st, segs, reinterpret_cast<float*>(static_cast<char*>(tab.p) + (size_t)n * sizeof(PrefetchSeg)));
  SVOC_HIP(hipGetLastError());
  stats_add_other();
  return SVOC_OK;
}

int k_sequence_mask(hipStream_t st, const int64_t* lengths, float* mask, int B, int T) {
  if (B <= 0 || T <= 0) return SVOC_OK;
  hipLaunchKernelGGL(sequence_mask_kernel, dim3((T + 255) / 256, B), dim3(256), 0, st, lengths, mask, B, T);
  SVOC_HIP(hipGetLastError());
  stats_add_other();
  return SVOC_OK;
}

// ------------------------------------------------------------------ gate (commons.py:100-107), standalone form
__global__ void gate_kernel(const float* __restrict__ a, const float* __restrict__ g, float* __restrict__ y, int H,
                            long long T, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long t = i % T;
  const long long c = (i / T) % H;
  const long long b = i / (T * H);
  const long long ia = (b * 2 * H + c) * T + t, ib = (b * 2 * H + H + c) * T + t;
  const float u = a[ia] + g[ia], v = a[ib] + g[ib];
  y[i] = gate_tanh_sigmoid(u, v);
}
int k_gate(hipStream_t st, const float* a, const float* b, float* y, int B, int H, int T) {
  const long long total = (long long)B * H * T;
  if (total <= 0) return SVOC_OK;
  hipLaunchKernelGGL(gate_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, b, y, H, (long long)T, total);
  SVOC_HIP(hipGetLastError());
  stats_add_other();
  return SVOC_OK;
}

// ------------------------------------------------------------------ lrelu -> conv_post (C->1, k taps, no bias) -> tanh
// (models.py:156-158).  One output row per utterance; every thread produces 4 consecutive samples.  Only the samples [c0, c0 + n) of
// the L computed are stored, at y[b * y_bs + t - c0] (the stateful stream keeps the interior of a window; infer: c0 = 0, n = L).
template <int K>
__global__ void conv_post_tanh_kernel(const float* __restrict__ x, long long x_bs, int x_ld, const float* __restrict__ w,
                                      int C, float slope, float* __restrict__ y, long long y_bs, int L, int c0, int n, int vec) {
  extern __shared__ float ws[];   // [C][K]
  for (int i = threadIdx.x; i < C * K; i += blockDim.x) ws[i] = w[i];
  __syncthreads();
  constexpr int P = (K - 1) / 2;
  constexpr int LEAD = (P + 3) / 4 * 4;           // staging starts at t0 - LEAD
  constexpr int NV = (LEAD + 3 + P) / 4 + 1;      // float4 groups covering [t0-LEAD, t0+3+P]
  const int b = blockIdx.y;
  const int t0 = (c0 & ~3) + (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (t0 >= c0 + n) return;
  const float* xb = x + (long long)b * x_bs;
  float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
  for (int c = 0; c < C; ++c) {
    const float* row = xb + (long long)c * x_ld;
    float v[NV * 4];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const int t = t0 - LEAD + 4 * q;
      if (vec && t >= 0 && t + 3 < L) {
        const float4 f = *reinterpret_cast<const float4*>(row + t);
        v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = (t + e >= 0 && t + e < L) ? row[t + e] : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < NV * 4; ++i) v[i] = v[i] > 0.f ? v[i] : v[i] * slope;
    const float* wc = ws + c * K;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const float wj = wc[j];
      acc0 = fmaf(wj, v[LEAD - P + j + 0], acc0);
      acc1 = fmaf(wj, v[LEAD - P + j + 1], acc1);
      acc2 = fmaf(wj, v[LEAD - P + j + 2], acc2);
      acc3 = fmaf(wj, v[LEAD - P + j + 3], acc3);
    }
  }
  float* yb = y + (long long)b * y_bs - c0;
  const int e = c0 + n;
  if (t0 >= c0 && t0 < e) yb[t0] = tanhf(acc0);
  if (t0 + 1 >= c0 && t0 + 1 < e) yb[t0 + 1] = tanhf(acc1);
  if (t0 + 2 >= c0 && t0 + 2 < e) yb[t0 + 2] = tanhf(acc2);
  if (t0 + 3 >= c0 && t0 + 3 < e) yb[t0 + 3] = tanhf(acc3);
}

__global__ void conv_post_tanh_generic_kernel(const float* __restrict__ x, long long x_bs, int x_ld,
                                              const float* __restrict__ w, int C, int K, float slope,
                                              float* __restrict__ y, long long y_bs, int L, int c0, int n) {
  const int t = c0 + blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (t >= c0 + n) return;
  const int P = (K - 1) / 2;
  const float* xb = x + (long long)b * x_bs;
  float acc = 0.f;
  for (int c = 0; c < C; ++c)
    for (int j = 0; j < K; ++j) {
      const int tt = t + j - P;
      if (tt >= 0 && tt < L) {
        float v = xb[(long long)c * x_ld + tt];
        v = v > 0.f ? v : v * slope;
        acc = fmaf(w[c * K + j], v, acc);
      }
    }
  y[(long long)b * y_bs + t - c0] = tanhf(acc);
}

int k_conv_post_tanh(hipStream_t st, const float* x, long long x_bs, int x_ld, const float* w, int C, int K, float slope,
                     float* y, int B, int L) {
  return k_conv_post_tanh_range(st, x, x_bs, x_ld, w, C, K, slope, y, L, B, L, 0, L);
}
int k_conv_post_tanh_range(hipStream_t st, const float* x, long long x_bs, int x_ld, const float* w, int C, int K, float slope,
                           float* y, long long y_bs, int B, int L, int c0, int n) {
  if (B <= 0 || L <= 0 || n <= 0) return SVOC_OK;
  if (c0 < 0 || c0 + n > L) SVOC_FAIL(SVOC_ERR_INVALID_ARG, "conv_post: samples [%d, %d) outside the window of %d", c0, c0 + n, L);
  if (K == 7 && C * K * 4 <= 48 * 1024) {
    const int vec = ((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (x_ld & 3) == 0 && (x_bs & 3) == 0) ? 1 : 0;
    const int nthr = (c0 + n - (c0 & ~3) + 3) / 4;
    hipLaunchKernelGGL(conv_post_tanh_kernel<7>, dim3((nthr + 255) / 256, B), dim3(256), (size_t)C * K * sizeof(float), st,
                       x, x_bs, x_ld, w, C, slope, y, y_bs, L, c0, n, vec);
  } else {
    hipLaunchKernelGGL(conv_post_tanh_generic_kernel, dim3((n + 255) / 256, B), dim3(256), 0, st, x, x_bs, x_ld, w, C, K,
                       slope, y, y_bs, L, c0, n);
  }
  SVOC_HIP(hipGetLastError());
  stats_add_other();
  return SVOC_OK;
}

// ------------------------------------------------------------------ strided 2-D copy (optionally * mask[col])
__global__ void copy2d_kernel(const float* __restrict__ src, long long s_bs, int s_ld, float* __restrict__ dst,
                              long long d_bs, int d_ld, int rows, int cols, const float* __restrict__ mask,
                              long long mask_bs) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  const int b = blockIdx.z;
  if (c >= cols) return;
  float v = src[(long long)b * s_bs + (long long)r * s_ld + c];
  if (mask) v *= mask[(long long)b * mask_bs + c];
  dst[(long long)b * d_bs + (long long)r * d_ld + c] = v;
}
int k_copy2d(hipStream_t st, const float* src, long long s_bs, int s_ld, float* dst, long long d_bs, int d_ld, int B,
             int rows, int cols, const float* mask, long long mask_bs) {
  if (B <= 0 || rows <= 0 || cols <= 0) return SVOC_OK;
  hipLaunchKernelGGL(copy2d_kernel, dim3((cols + 255) / 256, rows, B), dim3(256), 0, st, src, s_bs, s_ld, dst, d_bs, d_ld,
                     rows, cols, mask, mask_bs);
  SVOC_HIP(hipGetLastError());
  stats_add_other();
  return SVOC_OK;
}

// up to five strided 2-D copies in ONE launch (round 6: the user-visible outputs of infer - m_p, logs_p, z_p, z, x_mask - were five launches behind every call;
// at 1 x 200 four launches are 0.5 % of the call); blockIdx.z = (copy, batch element)
__global__ void copy2d_many_kernel(const CopyMany m) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  const int k = blockIdx.z / m.B, b = blockIdx.z - k * m.B;
  if (c >= m.cols || r >= m.rows[k]) return;
  m.dst[k][(long long)b * m.d_bs[k] + (long long)r * m.d_ld[k] + c] = m.src[k][(long long)b * m.s_bs[k] + (long long)r * m.s_ld[k] + c];
}
int k_copy2d_many(hipStream_t st, const CopyMany& m) {
  if (m.n <= 0 || m.B <= 0 || m.cols <= 0) return SVOC_OK;
  int rows = 0;
  for (int k = 0; k < m.n; ++k) rows = std::max(rows, m.rows[k]);
  if (rows <= 0 || (long long)m.n * m.B > 65535) return SVOC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(copy2d_many_kernel, dim3((m.cols + 255) / 256, rows, m.n * m.B), dim3(256), 0, st, m);
  SVOC_HIP(hipGetLastError());
  stats_add_other();
  return SVOC_OK;
}

// channel flip (modules.Flip, modules.py:272) as a strided copy: dst[b][c] = src[b][C-1-c]
__global__ void flip_copy_kernel(const float* __restrict__ src, long long s_bs, int s_ld, float* __restrict__ dst,
                                 long long d_bs, int d_ld, int C, int T) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int c = blockIdx.y;
  const int b = blockIdx.z;
  if (t >= T) return;
  dst[(long long)b * d_bs + (long long)c * d_ld + t] = src[(long long)b * s_bs + (long long)(C - 1 - c) * s_ld + t];
}
int k_flip_copy(hipStream_t st, const float* src, long long s_bs, int s_ld, float* dst, long long d_bs, int d_ld, int B,
                int C, int T) {
  if (B <= 0 || C <= 0 || T <= 0) return SVOC_OK;
  hipLaunchKernelGGL(flip_copy_kernel, dim3((T + 255) / 256, C, B), dim3(256), 0, st, src, s_bs, s_ld, dst, d_bs, d_ld, C, T);
  SVOC_HIP(hipGetLastError());
  stats_add_other();
  return SVOC_OK;
}

// Reflect-pad the waveform by `pad` on both sides (mel_processing.py:63) and lay it out as xt[b][c][t] =
// padded[t*hop + c]: frames of n_fft = q*hop samples become a q-tap convolution over t with hop input channels.
// pad2 > 0: torch.stft's own center=True padding (n_fft / 2, reflect) around the once-padded signal (mel_processing.py:66-67).
__global__ void frame_blocks_kernel(const float* __restrict__ y, int Lw, int pad, int pad2, int hop, float* __restrict__ xt,
                                    long long xt_bs, int xt_ld, int nblocks) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int c = blockIdx.y, b = blockIdx.z;
  if (t >= nblocks) return;
  const long long L1 = (long long)Lw + 2 * pad, Lp = L1 + 2 * pad2;
  const long long i = (long long)t * hop + c;
  float v = 0.f;
  if (i < Lp) {
    long long j = i - pad2;                  // index into the once-padded signal
    if (j < 0) j = -j;
    if (j >= L1) j = 2 * (L1 - 1) - j;
    long long s = j - pad;
    if (s < 0) s = -s;                       // reflect (no edge repeat)
    if (s >= Lw) s = 2LL * (Lw - 1) - s;
    s = s < 0 ? 0 : (s >= Lw ? Lw - 1 : s);
    v = y[(long long)b * Lw + s];
  }
  xt[(long long)b * xt_bs + (long long)c * xt_ld + t] = v;
}
int k_frame_blocks(hipStream_t st, const float* y, int B, int Lw, int pad, int pad2, int hop, float* xt, long long xt_bs, int xt_ld, int nblocks) {
  if (B <= 0 || nblocks <= 0) return SVOC_OK;
  hipLaunchKernelGGL(frame_blocks_kernel, dim3((nblocks + 255) / 256, hop, B), dim3(256), 0, st, y, Lw, pad, pad2, hop, xt, xt_bs, xt_ld, nblocks);
  SVOC_HIP(hipGetLastError());
  stats_add_other();
  return SVOC_OK;
}

__global__ void fill_kernel(float* p, size_t n, float v) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
int k_fill(hipStream_t st, float* p, size_t n, float v) {
  if (n == 0) return SVOC_OK;
  hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, n, v);
  SVOC_HIP(hipGetLastError());
  stats_add_other();
  return SVOC_OK;
}

}  // namespace svoc

extern "C" {
const char* svoc_last_error(void) { return svoc::last_error(); }
int svoc_abi_version(void) { return 7; }
const char* svoc_build_arch(void) { return "gfx950"; }
int svoc_stats_reset(void) { svoc::stats_reset(); return SVOC_OK; }
int svoc_stats_get(int64_t* conv_launches, double* conv_flops, int64_t* other_launches) {
  long long cl, ol; double cf;
  svoc::stats_get(&cl, &cf, &ol);
  if (conv_launches) *conv_launches = cl;
  if (conv_flops) *conv_flops = cf;
  if (other_launches) *other_launches = ol;
  return SVOC_OK;
}
int64_t svoc_stats_convolutions(void) { return svoc::stats_convs(); }
double svoc_stats_executed_flops(void) { return svoc::stats_exec_flops(); }
int svoc_set_variant_batch(int n) { return svoc::set_variant_batch(n); }
int svoc_check_async_error(void) { return svoc::async_error_check(); }
int svoc_debug_raise_async_error(void) {
  int* w = svoc::async_error_word();
  if (!w) SVOC_FAIL(SVOC_ERR_NOMEM, "svoc_debug_raise_async_error: no pinned host memory");
  __atomic_store_n(w, 1, __ATOMIC_RELAXED);
  return SVOC_OK;
}
int svoc_debug_persist_control(int fault_tile, int timeout_ms, int reenable) { return svoc::persist_control(fault_tile, timeout_ms, reenable); }
int svoc_persist_state(int* disabled, int* timeout_ms) {
  if (disabled) *disabled = svoc::persist_disabled() ? 1 : 0;
  if (timeout_ms) *timeout_ms = svoc::persist_timeout_ms();
  return SVOC_OK;
}
int svoc_profile_enable(int on) { svoc::prof_enable(on != 0); return SVOC_OK; }
int svoc_profile_report(char* buf, int buflen) {
  if (!buf || buflen <= 0) SVOC_FAIL(SVOC_ERR_INVALID_ARG, "svoc_profile_report: bad buffer");
  const std::string r = svoc::prof_report();
  const int n = (int)std::min<size_t>(r.size(), (size_t)buflen - 1);
  memcpy(buf, r.data(), n);
  buf[n] = 0;
  return SVOC_OK;
}
int svoc_sequence_mask(void* stream, const int64_t* lengths, float* mask, int B, int T) {
  if (!lengths || !mask || B < 0 || T < 0) SVOC_FAIL(SVOC_ERR_INVALID_ARG, "svoc_sequence_mask: bad arguments");
  return svoc::k_sequence_mask(svoc::as_stream(stream), lengths, mask, B, T);
}
int svoc_fused_add_tanh_sigmoid_multiply(void* stream, const float* a, const float* b, float* acts, int B, int H, int T) {
  if (!a || !b || !acts || B < 0 || H < 0 || T < 0) SVOC_FAIL(SVOC_ERR_INVALID_ARG, "svoc_fused_add_tanh_sigmoid_multiply: bad arguments");
  return svoc::k_gate(svoc::as_stream(stream), a, b, acts, B, H, T);
}
}
