// Stateful streaming inference (svoc_stream_*): SynthesizerTrn.infer cut into its stages, each run over a window of its own input that
// reaches back only by that stage's halo.  Every stage boundary keeps, in stream-owned buffers, the columns the next stage still needs;
// a push runs each stage over [consumed - h_left, available), keeps the columns whose whole receptive field lay inside the window (or
// beyond a true utterance edge) and appends them to the next boundary.  The launches of a stage are infer's own (engine.hip stage_ops);
// this file owns the geometry, the windows and the carry kernel that moves columns between the buffers.
#include "svoc_internal.h"

#include <algorithm>
#include <cstring>

namespace svoc {

// ------------------------------------------------------------------ geometry (host only)
// Stage s maps input columns m to output columns n at u_s outputs per input; output n depends on exactly the inputs m with
// n - h_left <= m * u <= n + h_right.  Stages: mel encoder (-> z_p), the reverse couplings in run order, conv_pre, each upsampler + MRF,
// conv_post + tanh (-> waveform).
struct StageGeom { int u, rate, hl, hr; };     // rate: output columns per mel frame

static int wn_reach(int k, int dr, int nl) {  // WN (modules.py:148-176): layer i pads (k * d - d) / 2 with d = dr^i
  long long r = 0, d = 1;
  for (int i = 0; i < nl; ++i) { r += (long long)(k - 1) * d / 2; d *= dr; }
  return (int)r;
}

static int stream_geometry(const svoc_synth_config& c, std::vector<StageGeom>& g, int& lookahead, int& hop) {
  const svoc_generator_config& d = c.dec;
  if (c.enc_kernel_size <= 0 || c.flow_kernel_size <= 0 || c.enc_n_layers <= 0 || c.flow_n_layers <= 0 || c.flow_n_flows <= 0 ||
      c.enc_dilation_rate <= 0 || c.flow_dilation_rate <= 0 || (c.enc_kernel_size % 2) == 0 || (c.flow_kernel_size % 2) == 0)
    SVOC_FAIL(SVOC_ERR_INVALID_ARG, "stream geometry: bad encoder / flow configuration");
  if (d.n_upsamples <= 0 || d.n_upsamples > 8 || d.n_kernels <= 0 || d.n_kernels > 8 || (d.resblock_kind != 1 && d.resblock_kind != 2))
    SVOC_FAIL(SVOC_ERR_INVALID_ARG, "stream geometry: bad decoder configuration");
  g.clear();
  g.push_back({1, 1, wn_reach(c.enc_kernel_size, c.enc_dilation_rate, c.enc_n_layers), 0});
  g.back().hr = g.back().hl;
  const int cr = wn_reach(c.flow_kernel_size, c.flow_dilation_rate, c.flow_n_layers);
  for (int j = 0; j < c.flow_n_flows; ++j) g.push_back({1, 1, cr, cr});
  g.push_back({1, 1, 3, 3});                                              // conv_pre: k 7, padding 3 (models.py:121)
  int rate = 1;
  // the widest ResBlock chain of the configured kind (modules.py:187-256): ResBlock1 = dilated k conv + undilated k conv per dilation,
  // ResBlock2 = dilated k conv per dilation
  int reach = 0;
  for (int j = 0; j < d.n_kernels; ++j) {
    const int k = d.resblock_kernel_sizes[j];
    if (k <= 0 || (k % 2) == 0 || d.n_dilations[j] <= 0 || d.n_dilations[j] > 8) SVOC_FAIL(SVOC_ERR_INVALID_ARG, "stream geometry: bad ResBlock %d", j);
    int w = 0;
    for (int q = 0; q < d.n_dilations[j]; ++q) w += (k - 1) * d.resblock_dilation_sizes[j][q] / 2 + (d.resblock_kind == 1 ? (k - 1) / 2 : 0);
    reach = std::max(reach, w);
  }
  for (int i = 0; i < d.n_upsamples; ++i) {
    const int u = d.upsample_rates[i], k = d.upsample_kernel_sizes[i];
    if (u <= 0 || k < u || ((k - u) % 2) != 0) SVOC_FAIL(SVOC_ERR_UNSUPPORTED, "stream geometry: upsample kernel %d / rate %d", k, u);
    // ConvTranspose1d(k, u, padding tpad): y[p] += w[j] x[m] for p = m * u + j - tpad, 0 <= j < k  ->  p - (k - 1 - tpad) <= m * u <= p + tpad
    const int tpad = (k - u) / 2;
    rate *= u;
    g.push_back({u, rate, reach + k - 1 - tpad, reach + tpad});
  }
  g.push_back({1, rate, 3, 3});                                           // conv_post: k 7, padding 3 (models.py:157)
  hop = rate;
  // look-ahead: a sample at frame f needs frames up to f + sum_s h_right_s / rate_s
  long long la = 0;
  for (const auto& s : g) la += (long long)s.hr * (hop / s.rate);
  lookahead = (int)((la + hop - 1) / hop);
  return SVOC_OK;
}

// ------------------------------------------------------------------ carry kernel
// Up to 8 strided copies, each with its own rows and columns, in one launch: blockIdx.z = (entry, batch element).  Sources and
// destinations never overlap (the boundary buffers are ping-ponged).
constexpr int CARRY_MAX = 8;
struct CarryEntry { const float* src; float* dst; long long s_bs, d_bs; int s_ld, d_ld, rows, cols; };
struct CarryBatch { CarryEntry e[CARRY_MAX]; int n, B; };

__global__ void carry_kernel(const CarryBatch cb) {
  const int k = blockIdx.z / cb.B, b = blockIdx.z - k * cb.B;
  const CarryEntry& e = cb.e[k];
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= e.cols) return;
  const float* s = e.src + (long long)b * e.s_bs + c;
  float* d = e.dst + (long long)b * e.d_bs + c;
  for (int r = blockIdx.y; r < e.rows; r += gridDim.y) d[(long long)r * e.d_ld] = s[(long long)r * e.s_ld];
}

static int k_carry(hipStream_t st, CarryBatch& cb) {
  int cols = 0, rows = 0, m = 0;
  for (int i = 0; i < cb.n; ++i) {
    if (cb.e[i].rows <= 0 || cb.e[i].cols <= 0) continue;              // drop empty entries
    cb.e[m++] = cb.e[i];
    cols = std::max(cols, cb.e[m - 1].cols);
    rows = std::max(rows, cb.e[m - 1].rows);
  }
  cb.n = m;
  if (m == 0) return SVOC_OK;
  if ((long long)m * cb.B > 65535) SVOC_FAIL(SVOC_ERR_UNSUPPORTED, "stream: batch %d too large for the carry launch", cb.B);
  hipLaunchKernelGGL(carry_kernel, dim3((cols + 255) / 256, std::min(rows, 64), m * cb.B), dim3(256), 0, st, cb);
  SVOC_HIP(hipGetLastError());
  stats_add_other();
  return SVOC_OK;
}

// ------------------------------------------------------------------ the stream
struct Stream {
  svoc_synth* syn = nullptr;
  svoc_synth_config cfg{};
  std::vector<StageGeom> geo;
  int S = 0, NF = 0, NU = 0, B = 0, M = 0, Tres = 0, lookahead = 0, hop = 1;

  // Boundary s is the input of stage s (0: the mel, with the eps draw as its twin at index S).  Columns [base, avail) of the utterance
  // are held in buf[cur] as [B][C][ld]; base is a multiple of 4, so a window that starts at a multiple of 4 has 16-byte aligned rows.
  struct Bnd { int C = 0; long long cap = 0; int ld = 0; DevBuf buf[2]; int cur = 0; };
  std::vector<Bnd> bnd;
  struct Cursor { std::vector<long long> base, avail, done; };   // per boundary / per stage (done: output columns produced)
  Cursor cur;
  std::vector<long long> cols;                                   // input columns each stage has processed (stats)
  DevBuf ones, xe, eo, mp, lp, fs;                               // all-ones mask, encoder scratch, frame-rate stage output
  size_t state_bytes = 0;

  int create(svoc_synth* h, int B_, int max_chunk) {
    syn = h; B = B_; M = max_chunk;
    SVOC_TRY(stage_ops::config(h, &cfg));
    SVOC_TRY(stream_geometry(cfg, geo, lookahead, hop));
    S = (int)geo.size(); NF = cfg.flow_n_flows; NU = cfg.dec.n_upsamples;
    if (NF % 2) SVOC_FAIL(SVOC_ERR_UNSUPPORTED, "stream: odd n_flows is not supported");
    // every window, and every boundary's held columns, stay below Tres frames' worth: a push adds at most M frames, the columns held
    // back for the right halos are the look-ahead, and a window reaches back by its left halo (also below the look-ahead) + 3 of alignment
    Tres = round_up(M + 2 * lookahead + 16, 4);
    bnd = std::vector<Bnd>(S + 1);
    for (int s = 0; s <= S; ++s) {
      Bnd& b = bnd[s];
      const int rate = s == 0 || s == S ? 1 : geo[s - 1].rate;
      if (s == 0) b.C = cfg.n_mel;
      else if (s == S) b.C = cfg.inter_channels;                               // eps, next to the mel
      else if (s <= NF + 1) b.C = cfg.inter_channels;                          // z_p, after each coupling
      else b.C = cfg.dec.upsample_initial_channel >> (s - NF - 2);              // after conv_pre, after each upsampler + MRF
      b.cap = (long long)Tres * rate;
      b.ld = (int)b.cap + 32;                                                   // (rows padded like the decoder's stage_ld: 16-byte loads past a window's end stay in the row)
      for (int q = 0; q < 2; ++q) SVOC_TRY(b.buf[q].ensure(((size_t)B * b.C * b.ld + 64) * sizeof(float)));
      state_bytes += b.buf[0].bytes + b.buf[1].bytes;
    }
    const int H = cfg.hidden_channels, IC = cfg.inter_channels;
    const size_t fr = (size_t)B * Tres;
    SVOC_TRY(ones.ensure(fr * sizeof(float)));
    SVOC_TRY(xe.ensure(fr * H * sizeof(float)));
    SVOC_TRY(eo.ensure(fr * H * sizeof(float)));
    SVOC_TRY(mp.ensure(fr * IC * sizeof(float)));
    SVOC_TRY(lp.ensure(fr * IC * sizeof(float)));
    SVOC_TRY(fs.ensure((size_t)B * (Tres + 20) * std::max(IC, cfg.dec.upsample_initial_channel) * sizeof(float)));
    state_bytes += ones.bytes + xe.bytes + eo.bytes + mp.bytes + lp.bytes + fs.bytes;
    SVOC_TRY(k_fill(nullptr, ones.f(), fr, 1.0f));
    SVOC_TRY(stage_ops::reserve(h, B, Tres));
    SVOC_HIP(hipStreamSynchronize(nullptr));
    reset();
    cols.assign(S, 0);
    return SVOC_OK;
  }

  void reset() { cur.base.assign(S + 1, 0); cur.avail.assign(S + 1, 0); cur.done.assign(S, 0); }

  // first input column stage s needs for output column `done` onwards, aligned down to 4
  long long window_start(int s, long long done) const {
    const StageGeom& g = geo[s];
    const long long v = done - g.hl;
    if (v <= 0) return 0;
    return (v + g.u - 1) / g.u / 4 * 4;
  }

  float* at(int s, long long col, int row = 0) {                // column `col` of boundary s's current buffer
    Bnd& b = bnd[s];
    return b.buf[b.cur].f() + (long long)row * b.ld + (col - cur.base[s]);
  }

  // Boundary n takes columns [nb, avail) of its current buffer plus `add` (rows of `src` x cols) into the other buffer: nb is where the
  // next window of stage n starts.  Appends the entries to `cb`; flips the buffer.
  int carry_into(CarryBatch& cb, Cursor& c, int n, long long nb, const float* src, long long s_bs, int s_ld, int rows, int row0, long long add) {
    Bnd& b = bnd[n];
    if (nb < c.base[n] || nb > c.avail[n]) SVOC_FAIL(SVOC_ERR_INVALID_ARG, "stream: boundary %d retains [%lld, %lld) of [%lld, %lld)", n, nb, c.avail[n], c.base[n], c.avail[n]);
    if (c.avail[n] + add - nb > b.cap) SVOC_FAIL(SVOC_ERR_SHAPE, "stream: boundary %d would hold %lld columns, capacity %lld", n, c.avail[n] + add - nb, b.cap);
    float* dst = b.buf[b.cur ^ 1].f();
    const long long bs = (long long)b.C * b.ld;
    const int keep = (int)(c.avail[n] - nb);
    if (keep > 0) cb.e[cb.n++] = CarryEntry{b.buf[b.cur].f() + (nb - c.base[n]), dst, bs, bs, b.ld, b.ld, b.C, keep};
    if (add > 0 && src) cb.e[cb.n++] = CarryEntry{src, dst + (long long)row0 * b.ld + keep, s_bs, bs, s_ld, b.ld, rows, (int)add};
    return SVOC_OK;
  }

  // One sub-push of T <= M frames (T = 0 and final: the flush).  exec = false only advances the cursor (the sample count of a push).
  int advance(Cursor& c, bool exec, hipStream_t st, const float* mel, const float* eps, long long in_ld, float noise, int T, bool final,
              float* out, long long out_ld, long long& out_pos) {
    if (T > 0) {   // the mel and eps columns: the left halo of the encoder's next window + what the caller hands over
      const long long nb = window_start(0, c.done[0]);
      if (exec) {
        CarryBatch cb{}; cb.B = B;
        SVOC_TRY(carry_into(cb, c, 0, nb, mel, (long long)cfg.n_mel * in_ld, (int)in_ld, cfg.n_mel, 0, T));
        SVOC_TRY(carry_into(cb, c, S, nb, eps, (long long)cfg.inter_channels * in_ld, (int)in_ld, cfg.inter_channels, 0, T));
        SVOC_TRY(k_carry(st, cb));
        bnd[0].cur ^= 1; bnd[S].cur ^= 1;
      }
      c.base[0] = c.base[S] = nb;
      c.avail[0] += T; c.avail[S] = c.avail[0];
    }
    for (int s = 0; s < S; ++s) {
      const StageGeom& g = geo[s];
      const long long in_av = c.avail[s];
      long long hi = final ? in_av * g.u : in_av * g.u - g.hr;
      if (s == S - 1 && !final) hi = hi / hop * hop;                   // whole frames of waveform
      if (hi <= c.done[s]) continue;
      const long long ws = window_start(s, c.done[s]);
      const long long L = in_av - ws;
      const long long lo = c.done[s] - ws * g.u;                      // first kept column of the window's output
      const long long add = hi - c.done[s];
      if (exec) {
        if (ws < c.base[s] || L > bnd[s].cap) SVOC_FAIL(SVOC_ERR_INVALID_ARG, "stream: stage %d window [%lld, %lld) outside its buffer", s, ws, in_av);
        cols[s] += L;
        const float* x = at(s, ws);
        const int xld = bnd[s].ld;
        CarryBatch cb{}; cb.B = B;
        if (s == S - 1) {
          SVOC_TRY(stage_ops::post(syn, st, x, xld, B, (int)L, (int)lo, (int)add, out + out_pos, out_ld));
        } else if (s == 0) {
          const int Tp = round_up((int)L, 4);
          SVOC_TRY(stage_ops::encoder(syn, st, x, xld, at(S, ws), bnd[S].ld, noise, ones.f(), Tres, xe.f(), eo.f(), mp.f(), lp.f(), fs.f(), B, (int)L));
          SVOC_TRY(carry_into(cb, c, 1, window_start(1, c.done[1]), fs.f() + lo, (long long)cfg.inter_channels * Tp, Tp, cfg.inter_channels, 0, add));
        } else if (s <= NF) {
          const int Tp = round_up((int)L, 4);
          const int x1 = stage_ops::coupling(syn, st, s - 1, x, xld, fs.f(), Tp, ones.f(), Tres, B, (int)L);
          if (x1 < 0) return x1;
          const int half = cfg.inter_channels / 2, x0 = x1 == 0 ? half : 0;
          const long long nb = window_start(s + 1, c.done[s + 1]);
          SVOC_TRY(carry_into(cb, c, s + 1, nb, fs.f() + (long long)x1 * Tp + lo, (long long)cfg.inter_channels * Tp, Tp, half, x1, add));
          // the x0 block passes through: from the input window, behind the entries above
          const int keep = (int)(c.avail[s + 1] - nb);
          Bnd& nbd = bnd[s + 1];
          cb.e[cb.n++] = CarryEntry{x + (long long)x0 * xld + lo, nbd.buf[nbd.cur ^ 1].f() + (long long)x0 * nbd.ld + keep, (long long)bnd[s].C * xld,
                                    (long long)nbd.C * nbd.ld, xld, nbd.ld, half, (int)add};
        } else if (s == NF + 1) {
          const int Tp = round_up((int)L, 4) + 20;                      // conv_pre's output rows as forward() lays them out (stage_ld)
          SVOC_TRY(stage_ops::conv_pre(syn, st, x, xld, fs.f(), Tp, B, (int)L));
          SVOC_TRY(carry_into(cb, c, s + 1, window_start(s + 1, c.done[s + 1]), fs.f() + lo, (long long)cfg.dec.upsample_initial_channel * Tp, Tp,
                              cfg.dec.upsample_initial_channel, 0, add));
        } else {
          const float* y = nullptr; int yld = 0;
          SVOC_TRY(stage_ops::dec_stage(syn, st, s - NF - 2, x, xld, B, (int)L, Tres, &y, &yld));
          const int C = bnd[s + 1].C;
          SVOC_TRY(carry_into(cb, c, s + 1, window_start(s + 1, c.done[s + 1]), y + lo, (long long)C * yld, yld, C, 0, add));
        }
        if (s < S - 1) { SVOC_TRY(k_carry(st, cb)); bnd[s + 1].cur ^= 1; }
      }
      if (s < S - 1) { c.base[s + 1] = window_start(s + 1, c.done[s + 1]); c.avail[s + 1] = hi; }
      else out_pos += add;
      c.done[s] = hi;
    }
    return SVOC_OK;
  }

  // samples a push of T frames (flush: T = 0, final) returns; changes nothing
  int samples(int T, bool final, long long& n) {
    Cursor c = cur;
    long long pos = 0;
    for (int t0 = 0; t0 < T; t0 += M) SVOC_TRY(advance(c, false, nullptr, nullptr, nullptr, 0, 0.f, std::min(M, T - t0), false, nullptr, 0, pos));
    if (final && c.avail[0] > 0) SVOC_TRY(advance(c, false, nullptr, nullptr, nullptr, 0, 0.f, 0, true, nullptr, 0, pos));
    n = pos;
    return SVOC_OK;
  }

  int push(hipStream_t st, const float* mel, const float* eps, int T, float noise, float* out, long long out_ld, long long& n) {
    long long want = 0;
    SVOC_TRY(samples(T, false, want));
    if (want > out_ld) SVOC_FAIL(SVOC_ERR_SHAPE, "svoc_stream_push: %lld samples do not fit a row of %lld", want, out_ld);
    long long pos = 0;
    for (int t0 = 0; t0 < T; t0 += M) {                               // a push larger than max_chunk_frames: sub-pushes
      const int t = std::min(M, T - t0);
      SVOC_TRY(advance(cur, true, st, mel + t0, eps + t0, T, noise, t, false, out, out_ld, pos));
    }
    n = pos;
    return SVOC_OK;
  }

  int flush(hipStream_t st, float noise, float* out, long long out_ld, long long& n) {
    long long want = 0;
    SVOC_TRY(samples(0, true, want));
    if (want > out_ld) SVOC_FAIL(SVOC_ERR_SHAPE, "svoc_stream_flush: %lld samples do not fit a row of %lld", want, out_ld);
    long long pos = 0;
    if (cur.avail[0] > 0) SVOC_TRY(advance(cur, true, st, nullptr, nullptr, 0, noise, 0, true, out, out_ld, pos));
    reset();                                                           // the next push starts a new utterance
    n = pos;
    return SVOC_OK;
  }
};

}  // namespace svoc

// ======================================================================= C ABI
using namespace svoc;

struct svoc_stream : svoc::HandleDevice { Stream m; };

extern "C" {

int svoc_stream_geometry(const svoc_synth_config* cfg, int* out, int n) {
  if (!cfg || (n > 0 && !out) || n < 0) SVOC_FAIL(SVOC_ERR_INVALID_ARG, "svoc_stream_geometry: bad arguments");
  try {
    std::vector<StageGeom> g;
    int la = 0, hop = 1;
    SVOC_TRY(stream_geometry(*cfg, g, la, hop));
    std::vector<int> v = {(int)g.size(), la, hop};
    for (const auto& s : g) { v.push_back(s.u); v.push_back(s.rate); v.push_back(s.hl); v.push_back(s.hr); }
    for (int i = 0; i < n && i < (int)v.size(); ++i) out[i] = v[i];
    return (int)v.size();
  } catch (const std::exception& e) { set_error("exception: %s", e.what()); return SVOC_ERR_NOMEM; }
}

int svoc_stream_create(svoc_stream** out, svoc_synth* synth, int B, int max_chunk_frames) {
  if (!out || !synth || B <= 0 || max_chunk_frames <= 0 || max_chunk_frames > (1 << 20)) SVOC_FAIL(SVOC_ERR_INVALID_ARG, "svoc_stream_create: bad arguments");
  *out = nullptr;
  try {
    std::unique_ptr<svoc_stream> h(new svoc_stream());
    SVOC_TRY(h->m.create(synth, B, max_chunk_frames));
    *out = h.release();
    return SVOC_OK;
  } catch (const std::exception& e) { set_error("exception: %s", e.what()); return SVOC_ERR_NOMEM; }
}

int svoc_stream_samples(svoc_stream* s, int T, int flush, int64_t* n_samples) {
  if (!s || !n_samples || T < 0 || (flush && T != 0) || (!flush && T == 0)) SVOC_FAIL(SVOC_ERR_INVALID_ARG, "svoc_stream_samples: bad arguments");
  try {
    long long n = 0;
    SVOC_TRY(s->m.samples(T, flush != 0, n));
    *n_samples = n;
    return SVOC_OK;
  } catch (const std::exception& e) { set_error("exception: %s", e.what()); return SVOC_ERR_NOMEM; }
}

int svoc_stream_push(svoc_stream* s, void* stream, const float* mel, const float* eps, int T, float noise_scale, float* out, int64_t out_ld,
                     int64_t* n_samples) {
  if (!s || !mel || !eps || !n_samples || T <= 0 || out_ld < 0 || (out_ld > 0 && !out)) SVOC_FAIL(SVOC_ERR_INVALID_ARG, "svoc_stream_push: bad arguments");
  *n_samples = 0;
  try {
    long long n = 0;
    SVOC_TRY(s->m.push(as_stream(stream), mel, eps, T, noise_scale, out, out_ld, n));
    *n_samples = n;
    return SVOC_OK;
  } catch (const std::exception& e) { set_error("exception: %s", e.what()); return SVOC_ERR_NOMEM; }
}

int svoc_stream_flush(svoc_stream* s, void* stream, float noise_scale, float* out, int64_t out_ld, int64_t* n_samples) {
  if (!s || !n_samples || out_ld < 0 || (out_ld > 0 && !out)) SVOC_FAIL(SVOC_ERR_INVALID_ARG, "svoc_stream_flush: bad arguments");
  *n_samples = 0;
  try {
    long long n = 0;
    SVOC_TRY(s->m.flush(as_stream(stream), noise_scale, out, out_ld, n));
    *n_samples = n;
    return SVOC_OK;
  } catch (const std::exception& e) { set_error("exception: %s", e.what()); return SVOC_ERR_NOMEM; }
}

int svoc_stream_stats(svoc_stream* s, int64_t* columns, int n, int64_t* state_bytes) {
  if (!s || n < 0 || (n > 0 && !columns)) SVOC_FAIL(SVOC_ERR_INVALID_ARG, "svoc_stream_stats: bad arguments");
  for (int i = 0; i < n && i < s->m.S; ++i) columns[i] = s->m.cols[i];
  if (state_bytes) *state_bytes = (int64_t)s->m.state_bytes;
  return s->m.S;
}

void svoc_stream_destroy(svoc_stream* s) { svoc::destroy_handle(s); }

}  // extern "C"
