// Opt-in fp16 form of the decoder's ResBlock convolutions (svoc_synth_set_decoder_precision / svoc_generator_set_decoder_precision,
// SVOC_PREC_F16): lrelu(slope) -> Conv1d(Cin -> Cout, k, d, "same" zero padding) + bias [+ residual] [-> accumulate, / div], direct form on
// v_mfma_f32_32x32x16_f16.
//
// Numerics (include/svoc.h): the activated input and the weight-norm-folded weight are rounded to fp16 with round-to-nearest-even
// (a plain cast: v_cvt_pk_f16_f32, never the round-toward-zero form); products are summed in fp32 accumulators; bias, residual, accumulate and
// division are fp32; what is read and written in HBM is fp32.  No clamping: |x| beyond 65504 becomes +-inf as a cast would make it.
//
// Anatomy: implicit GEMM, M = Cout rows, N = time, K = Cin per tap.  A workgroup (4 waves) owns TM rows x TN columns of one utterance and walks
// the input channels in chunks of 32: the chunk's window [t0 - pad, t0 + TN + pad) is staged activated and converted into LDS time-major,
// [t][ci] fp16, so that one ds_read_b128 gives a lane the 8 channels of its B fragment (lane l: B[k = 8(l>>5) + e][col l&31]) and tap j reads
// the same image j*d rows further down: no im2col copy.  A row is 64 B of data in an 80-B pitch (an odd number of 16-B slots: every 16-lane group
// of a ds_read_b128 hits 16 distinct slots).  The weights are packed once into A-fragment order [co-block][tap][ci-step of 16][lane][8] (16 B per
// lane and MFMA).  The tile is chosen from Cout alone, never from B or L, so batch composition cannot change a result bit.
#include "svoc_internal.h"

#include <cstdio>

namespace svoc {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

namespace {
constexpr int KCH = 32;        // input channels per staged chunk
constexpr int PITCH = 40;      // halves per LDS row (32 data + 8 pad)

struct ConvF16Args {
  const float* x; long long x_bs; int x_ld;
  const half8* wp; const float* bias;
  int Cin, Cout, L, K, dil, pad;
  float slope;
  float* y; long long y_bs; int y_ld;
  const float* res; long long res_bs; int res_ld;
  unsigned flags; float div;
  int ntn;                     // time tiles per utterance
};

template <int WM, int WN, int MR, int NR>
__global__ __launch_bounds__(256) void conv_f16_kernel(ConvF16Args p) {
  constexpr int TM = WM * MR * 32, TN = WN * NR * 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  _Float16* lds = reinterpret_cast<_Float16*>(smem_raw);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave % WM, wn = wave / WM;
  const int b = blockIdx.x / p.ntn;
  const int t0 = (blockIdx.x - b * p.ntn) * TN;
  const int row0 = blockIdx.y * TM + wm * MR * 32;         // first output row of this wave
  const int R = TN + (p.K - 1) * p.dil;                    // staged window rows
  const int S = (p.Cin + 31) / 32 * 2;                     // ci-steps over the input channels padded to a multiple of 32
  const float* xb = p.x + (long long)b * p.x_bs;

  floatx16 acc[MR][NR];
#pragma unroll
  for (int mr = 0; mr < MR; ++mr)
#pragma unroll
    for (int nr = 0; nr < NR; ++nr)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mr][nr][r] = 0.0f;

  const int l31 = lane & 31, hi = lane >> 5;
  // B fragment base of this lane: row (wn*NR*32 + nr*32 + l31 + j*d), halves 16*s + 8*hi
  const int brow0 = wn * NR * 32 + l31;

  for (int c0 = 0; c0 < S * 16; c0 += KCH) {
    __syncthreads();                                       // previous chunk's reads are done
    // stage: item i -> window row r = i % R (consecutive lanes: consecutive t, coalesced loads), channel group g = i / R
    for (int i = tid; i < R * (KCH / 8); i += 256) {
      const int g = i / R, r = i - g * R;
      const int t = t0 - p.pad + r;
      half8 h;
      const int c = c0 + 8 * g;
      if (t >= 0 && t < p.L) {
        const float* src = xb + (long long)c * p.x_ld + t;
        if (c + 8 <= p.Cin) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float v = src[(long long)e * p.x_ld];
            v = v < 0.0f ? v * p.slope : v;
            h[e] = (_Float16)v;
          }
        } else {                                           // channel padding (Cin not a multiple of 32): zeros
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float v = c + e < p.Cin ? src[(long long)e * p.x_ld] : 0.0f;
            v = v < 0.0f ? v * p.slope : v;
            h[e] = (_Float16)v;
          }
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = (_Float16)0.0f;
      }
      *reinterpret_cast<half8*>(lds + r * PITCH + 8 * g) = h;
    }
    __syncthreads();
    const int sc0 = c0 / 16;
    for (int j = 0; j < p.K; ++j) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        half8 a[MR], bf[NR];
#pragma unroll
        for (int mr = 0; mr < MR; ++mr)
          a[mr] = p.wp[((long long)((row0 / 32 + mr) * p.K + j) * S + sc0 + s) * 64 + lane];
#pragma unroll
        for (int nr = 0; nr < NR; ++nr)
          bf[nr] = *reinterpret_cast<const half8*>(lds + (brow0 + nr * 32 + j * p.dil) * PITCH + 16 * s + 8 * hi);
#pragma unroll
        for (int mr = 0; mr < MR; ++mr)
#pragma unroll
          for (int nr = 0; nr < NR; ++nr)
            acc[mr][nr] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mr], bf[nr], acc[mr][nr], 0, 0, 0);
      }
    }
  }

  // epilogue (EpiOut semantics of the fp32 kernels): v = acc + bias [+ res] ; [y_old + v] ; [/ div]
  const unsigned fl = p.flags;
#pragma unroll
  for (int mr = 0; mr < MR; ++mr) {
    const int rb = row0 + mr * 32 + 4 * hi;
    const bool full = row0 + mr * 32 + 32 <= p.Cout;      // else rows >= Cout are the block's padding (Cout not a multiple of 32)
    if (row0 + mr * 32 >= p.Cout) continue;
#pragma unroll
    for (int nr = 0; nr < NR; ++nr) {
      const int col = t0 + wn * NR * 32 + nr * 32 + l31;
      if (col >= p.L) continue;
      float* yb = p.y + (long long)b * p.y_bs + (long long)rb * p.y_ld + col;
      float rv[16], yo[16];
      if (fl & F_RES) {
        const float* rp = p.res + (long long)b * p.res_bs + (long long)rb * p.res_ld + col;
#pragma unroll
        for (int r = 0; r < 16; ++r) rv[r] = (full || rb + (r & 3) + 8 * (r >> 2) < p.Cout) ? rp[(long long)((r & 3) + 8 * (r >> 2)) * p.res_ld] : 0.0f;
      }
      if (fl & F_ACC) {
#pragma unroll
        for (int r = 0; r < 16; ++r) yo[r] = (full || rb + (r & 3) + 8 * (r >> 2) < p.Cout) ? yb[(long long)((r & 3) + 8 * (r >> 2)) * p.y_ld] : 0.0f;
      }
      float vo[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = acc[mr][nr][r] + p.bias[rb + (r & 3) + 8 * (r >> 2)];   // (the packed bias covers the padded rows)
        if (fl & F_RES) v = v + rv[r];
        if (fl & F_ACC) v = yo[r] + v;
        vo[r] = v;
      }
      if (fl & F_DIV) {
        asm volatile("" ::: "memory");
#pragma unroll
        for (int r = 0; r < 16; ++r) vo[r] = vo[r] / p.div;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (full || rb + (r & 3) + 8 * (r >> 2) < p.Cout) yb[(long long)((r & 3) + 8 * (r >> 2)) * p.y_ld] = vo[r];
    }
  }
}

// fp16 A-fragment image from the fp32 image of pack_conv (weight norm already folded there; its layout is documented at the top of
// pack.hip and decoded here - the two change together): element e of lane l at
// [co-block cb][tap j][ci-step s] is W[32 cb + (l & 31)][16 s + 8 (l >> 5) + e][j]
__global__ void pack_f16_kernel(const float* __restrict__ wp32, int ksg_total, int K, int S, half8* __restrict__ out, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;    // one lane fragment
  if (i >= total) return;
  const int lane = (int)(i & 63);
  long long q = i >> 6;
  const int s = (int)(q % S); q /= S;
  const int j = (int)(q % K);
  const int cb = (int)(q / K);
  half8 h;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int chan = 16 * s + 8 * (lane >> 5) + e;
    // pack_conv: lane' = row & 31 | (chan & 1) << 5, ks = (chunk * K + j) * 16 + (chan % 32) / 2, element (ks / 4, lane', ks % 4)
    const int ln = (lane & 31) | ((chan & 1) << 5);
    const int ks = ((chan / KC) * K + j) * (KC / 2) + (chan % KC) / 2;
    const float w = wp32[(((long long)cb * ksg_total + ks / 4) * 64 + ln) * 4 + (ks & 3)];
    h[e] = (_Float16)w;
  }
  out[i] = h;
}

struct TileF16 { int WM, WN, MR, NR; };
TileF16 tile_f16(int Cout) {                     // Cout alone decides (never B or L)
  if (Cout % 128 == 0) return {2, 2, 2, 2};      // 128 x 128
  if (Cout % 64 == 0) return {2, 2, 1, 2};       // 64 x 128
  return {1, 4, 1, 2};                           // 32 x 256 (Cout = 32, 96, ..., and Cout not a multiple of 32: padded rows)
}

template <int WM, int WN, int MR, int NR>
int launch_f16_cfg(const ConvF16Args& a0, int B, hipStream_t st) {
  constexpr int TM = WM * MR * 32, TN = WN * NR * 32;
  ConvF16Args a = a0;
  a.ntn = (a.L + TN - 1) / TN;
  const size_t lds = (size_t)(TN + (a.K - 1) * a.dil) * PITCH * sizeof(_Float16);
  if (lds > 64 * 1024) SVOC_FAIL(SVOC_ERR_UNSUPPORTED, "conv_f16: window of %d rows does not fit the LDS", TN + (a.K - 1) * a.dil);
  if ((long long)a.ntn * B > 0x7fffffffLL) SVOC_FAIL(SVOC_ERR_UNSUPPORTED, "conv_f16: grid too large");
  dim3 grid((unsigned)(a.ntn * B), (unsigned)((a.Cout + TM - 1) / TM));
  hipLaunchKernelGGL((conv_f16_kernel<WM, WN, MR, NR>), grid, dim3(256), lds, st, a);
  SVOC_HIP(hipGetLastError());
  return SVOC_OK;
}
}  // namespace

bool conv_f16_supported(int Cin, int Cout, int K, int dil) {
  return Cin > 0 && Cout > 0 && K > 0 && (K % 2) == 1 && dil > 0 &&
         (size_t)(256 + (K - 1) * dil) * PITCH * sizeof(_Float16) <= 64 * 1024;
}

int pack_conv_f16(PackedConvF16& pf, const PackedConv& pc, hipStream_t st) {
  if (pc.transposed || pc.paired || pc.split_row != (1 << 30) || !conv_f16_supported(pc.Cin, pc.Cout, pc.ktaps, pc.dil) ||
      pc.pad != (pc.ktaps * pc.dil - pc.dil) / 2)
    SVOC_FAIL(SVOC_ERR_UNSUPPORTED, "conv_f16: Cin %d Cout %d k %d d %d is not a plain same-padded convolution with odd k", pc.Cin, pc.Cout,
              pc.ktaps, pc.dil);
  pf.Cin = pc.Cin; pf.Cout = pc.Cout; pf.K = pc.ktaps; pf.dil = pc.dil; pf.pad = pc.pad;
  pf.bias = pc.bias.f();
  pf.flops_per_col = pc.flops_per_col;
  const int S = pc.CinP / 16;                    // pack_conv pads channels to a multiple of 32 and rows to mtiles * 32, with zeros
  const long long total = (long long)pc.mtiles * pc.ktaps * S * 64;
  SVOC_TRY(pf.wp.ensure((size_t)total * 16));
  hipLaunchKernelGGL(pack_f16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, pc.wp.f(), pc.ksg_total, pc.ktaps, S,
                     (half8*)pf.wp.p, total);
  SVOC_HIP(hipGetLastError());
  SVOC_HIP(hipStreamSynchronize(st));
  return SVOC_OK;
}

int launch_conv_f16(const PackedConvF16& pf, const float* x, long long x_bs, int x_ld, float slope, const EpiOut& out, int B, int L,
                    hipStream_t st) {
  if (B <= 0 || L <= 0) return SVOC_OK;
  if (!pf.wp.p) SVOC_FAIL(SVOC_ERR_INVALID_ARG, "conv_f16: no fp16 weight image");
  if (out.flags & ~(unsigned)(F_RES | F_ACC | F_DIV)) SVOC_FAIL(SVOC_ERR_UNSUPPORTED, "conv_f16: epilogue flags 0x%x", out.flags);
  ConvF16Args a{};
  a.x = x; a.x_bs = x_bs; a.x_ld = x_ld;
  a.wp = (const half8*)pf.wp.p; a.bias = pf.bias;
  a.Cin = pf.Cin; a.Cout = pf.Cout; a.L = L; a.K = pf.K; a.dil = pf.dil; a.pad = pf.pad;
  a.slope = slope;
  a.y = out.y; a.y_bs = out.y_bs; a.y_ld = out.y_ld;
  a.res = out.res; a.res_bs = out.res_bs; a.res_ld = out.res_ld;
  a.flags = out.flags; a.div = out.div;
  const TileF16 c = tile_f16(pf.Cout);
  const double flops = pf.flops_per_col * (double)B * (double)L;
  stats_add_conv(flops);                                   // direct form: executed == algorithmic
  int prof_idx = -1;
  if (prof_enabled()) {
    char d[160];
    snprintf(d, sizeof(d), "convh Ci%-4d Co%-4d k%-2d d%-2d N%-7d B%-3d %dx%d f16", pf.Cin, pf.Cout, pf.K, pf.dil, L, B, c.WM * c.MR * 32,
             c.WN * c.NR * 32);
    prof_idx = prof_begin(st, d, flops);
  }
  int r;
  if (c.MR == 2) r = launch_f16_cfg<2, 2, 2, 2>(a, B, st);
  else if (c.WM == 2) r = launch_f16_cfg<2, 2, 1, 2>(a, B, st);
  else r = launch_f16_cfg<1, 4, 1, 2>(a, B, st);
  prof_end(st, prof_idx);
  return r;
}

}  // namespace svoc
