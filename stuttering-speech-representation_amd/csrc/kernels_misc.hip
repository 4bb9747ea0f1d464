// Non-GEMM kernels of the hot path (gfx950):
//   wave_stats        Wav2Vec2FeatureExtractor zero-mean/unit-var stats      (a2)
//   conv0_stats/apply WavLM conv0 (1->C, k=10, s=5) + GroupNorm(C, C) + GELU  (K1, a3)
//   layernorm         LN over rows (feature projection, post/pre-LN encoders) (K3, K7)
//   pool_mean         time-mean of one hidden state into the embedding slot  (K8, K12)
//   attention         flash-style MFMA attention; WavLM gated rel-pos bias    (K5, K6, K11)
#include "common.h"
#include "kernels.h"

// ---------------------------------------------------------------------------------------
// a2: per-clip mean / rstd for do_normalize (HF feature_extraction_wav2vec2.py:94).
__global__ __launch_bounds__(256) void wave_stats_kernel(const float* __restrict__ x, int LS,
                                                         float* __restrict__ out, const int* __restrict__ lens) {
  const float* xb = x + (long long)blockIdx.x * LS;
  // ragged batches: the clip's own samples, clamped to the row (a length past the row never reads
  // the next clip; an empty clip gives mean 0, rstd of eps alone)
  const int L = lens ? min(max(lens[blockIdx.x], 0), LS) : LS;
  double s = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < L; i += 256) {
    const double v = xb[i];
    s += v;
    q += v * v;
  }
  s = wave_sum_d(s);
  q = wave_sum_d(q);
  __shared__ double sh[2][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[0][w] = s; sh[1][w] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double S = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
    const double Q = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
    const double mean = L > 0 ? S / L : 0.0, var = L > 0 ? Q / L - mean * mean : 0.0;
    out[2 * blockIdx.x] = (float)mean;
    out[2 * blockIdx.x + 1] = (float)(1.0 / sqrt((var > 0 ? var : 0.0) + 1e-7));
  }
}

int launch_wave_stats(const float* x, int B, int L, float* out, hipStream_t s, const int* lens) {
  hipLaunchKernelGGL(wave_stats_kernel, dim3(B), dim3(256), 0, s, x, L, out, lens);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---------------------------------------------------------------------------------------
// K1: conv0 (1 -> C, k0 = 10, s0 = 5) + GroupNorm(C, C) + GELU  (HF modeling_wavlm.py:723-744).
//
// GroupNorm statistics without recomputing the conv: y_t[c] = w_c . x_t (+ b_c) over the
// 10-sample windows x_t = x[s0 t : s0 t + k0], so per clip and channel
//   sum_t y_t = w_c . S + T0 b_c,   sum_t (y_t - b_c)^2 = w_c^T G w_c,
// with the clip's window moments S_j = sum_t x_t[j] and Gram matrix G_jk = sum_t x_t[j] x_t[k]
// (k0 + k0(k0+1)/2 = 65 numbers per clip, fp64).  conv0_moments computes S, G in one pass
// over the waveform; gn_finalize turns them into a per-(clip, channel) affine; conv0_apply
// then evaluates conv + affine + GELU once and writes the channels-last bf16/fp32 tensor.
constexpr int C0_T = 64;                 // frames per apply block
constexpr int K0 = 10;                   // conv0 kernel (WavLM)
constexpr int NG = K0 * (K0 + 1) / 2;    // unique Gram entries
constexpr int NMOM = K0 + NG;            // 65 moments per clip

// One block per (clip, frame chunk): a clip's frames in MOM_NCH chunks, each block's partial moments
// written to mom[b][chunk]; gn_finalize sums the chunks in chunk order (deterministic, and every clip's
// result independent of the batch).  One block per clip walked ~38 dependent load rounds per thread
// (latency-bound, 72 us at B = 128 while the GPU was otherwise idle at the step's start); 8 chunks spent
// most of their time in the 65 fp64 wave reductions per block (~5 frames per thread): 2 chunks (~19 frames per
// thread) took the conv0 + GroupNorm role 0.633 -> 0.576 ms/step at B = 256 (round 6, profiles/r6_ab_conv0_moments.txt).
constexpr int MOM_NCH = 2;

__global__ __launch_bounds__(256) void conv0_moments_kernel(const float* __restrict__ x, int L,
                                                            const float* __restrict__ norm, int s0, int T0S,
                                                            double* __restrict__ mom, const int* __restrict__ t0len) {
  const int ch = blockIdx.x, b = blockIdx.y;
  const int T0 = t0len ? t0len[b] : T0S;
  const int per = (T0 + MOM_NCH - 1) / MOM_NCH;   // the clip's own chunks: batch-independent grouping
  const int te = min(ch * per + per, T0);
  const float* xb = x + (long long)b * L;
  float mu = 0.f, rs = 1.f;
  if (norm) { mu = norm[2 * b]; rs = norm[2 * b + 1]; }
  double S[K0], G[NG];
  #pragma unroll
  for (int j = 0; j < K0; ++j) S[j] = 0.0;
  #pragma unroll
  for (int j = 0; j < NG; ++j) G[j] = 0.0;
  #pragma unroll 2
  for (int t = ch * per + threadIdx.x; t < te; t += 256) {
    double w[K0];
    #pragma unroll
    for (int j = 0; j < K0; ++j) {
      const float v = xb[(long long)t * s0 + j];
      w[j] = norm ? (double)((v - mu) * rs) : (double)v;
      S[j] += w[j];
    }
    int k = 0;
    #pragma unroll
    for (int i = 0; i < K0; ++i)
      #pragma unroll
      for (int j = i; j < K0; ++j) G[k++] += w[i] * w[j];
  }
  __shared__ double red[4][NMOM];
  const int wv = threadIdx.x >> 6;
  #pragma unroll
  for (int j = 0; j < NMOM; ++j) {
    double v = wave_sum_d(j < K0 ? S[j] : G[j - K0]);
    if ((threadIdx.x & 63) == 0) red[wv][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < NMOM)
    mom[((long long)b * MOM_NCH + ch) * NMOM + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

SSE_DEV void c0m_split(float v, bf16& h, bf16& l) {
  h = (bf16)v;
  l = (bf16)(v - (float)h);
}

// wf[cb][lane]: A fragment of channel block cb (16 channels) for lane (q, r16) of the matrix-core
// conv0 (conv0_mfma_kernel): split-bf16 weights, the lane-group order of its B fragments
SSE_DEV void conv0_wfrag(const float* __restrict__ w0, int i, bf16x8* __restrict__ wf) {
  const int cb = i >> 6, lane = i & 63, q = lane >> 4, c = cb * 16 + (lane & 15);
  bf16 h[K0], l[K0];
  #pragma unroll
  for (int j = 0; j < K0; ++j) c0m_split(w0[c * K0 + j], h[j], l[j]);
  const bf16 z = (bf16)0.f;
  bf16x8 f;
  if (q == 0) f = bf16x8{h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]};
  else if (q == 1) f = bf16x8{h[8], h[9], h[0], h[1], h[2], h[3], h[4], h[5]};
  else if (q == 2) f = bf16x8{h[6], h[7], h[8], h[9], l[0], l[1], l[2], l[3]};
  else f = bf16x8{l[4], l[5], l[6], l[7], l[8], l[9], z, z};
  wf[i] = f;
}

// grid (ceil(C / 256), B): the block's clip moments summed over the chunks (fixed order) into LDS, then
// one (clip, channel) affine per thread; the blocks also write the matrix-core conv0's weight
// fragments when wf is given (C / 16 x 64 lanes, one launch fewer)
__global__ __launch_bounds__(256) void gn_finalize_kernel(const double* __restrict__ mom, int B, int C, int T0S,
                                                          const float* __restrict__ w0, const float* __restrict__ b0,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps,
                                                          float2* __restrict__ ss, const int* __restrict__ t0len,
                                                          bf16x8* __restrict__ wf) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (wf) {
    const int nb = gridDim.x * gridDim.y;
    for (int i = (blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; i < C / 16 * 64; i += nb * 256)
      conv0_wfrag(w0, i, wf);
  }
  __shared__ double M[NMOM];
  if (threadIdx.x < NMOM) {
    const double* p = mom + (long long)b * MOM_NCH * NMOM + threadIdx.x;
    double v = p[0];
    #pragma unroll
    for (int k = 1; k < MOM_NCH; ++k) v += p[k * NMOM];
    M[threadIdx.x] = v;
  }
  __syncthreads();
  if (c >= C) return;
  const int T0 = t0len ? t0len[b] : T0S;
  const double* S = M;
  const double* G = M + K0;
  double w[K0];
  #pragma unroll
  for (int j = 0; j < K0; ++j) w[j] = w0[c * K0 + j];
  double sw = 0.0, q = 0.0;
  int k = 0;
  #pragma unroll
  for (int a = 0; a < K0; ++a) {
    sw += w[a] * S[a];
    #pragma unroll
    for (int j = a; j < K0; ++j) q += (a == j ? 1.0 : 2.0) * w[a] * w[j] * G[k++];
  }
  const double inv = T0 > 0 ? 1.0 / T0 : 0.0;         // a frameless clip (ragged) stays finite
  const double m0 = sw * inv;                          // mean of w.x_t
  double var = q * inv - m0 * m0;
  var = var > 0 ? var : 0;
  const double mean = m0 + (b0 ? (double)b0[c] : 0.0);
  const float rstd = (float)(1.0 / sqrt(var + (double)eps));
  const float sc = gamma[c] * rstd;
  ss[(long long)b * C + c] = make_float2(sc, beta[c] - (float)mean * sc);
}

// LNG (WavLM-large "layer" frontend, C == 512): the frame's 512 channels are exactly the wave's 64
// lanes x 8, so LayerNorm over channels (layernorm_kernel's expression, statistics from the fp32
// conv values) and GELU are applied before the single store -- no second pass over the
// [B][T0][512] activation.
// OUT3 (split-fp16 path, TO = float): the fp32 result written as tripled f16 rows [hi | lo' | hi] of 3C
// (x3_split4) -- the conv1 GEMM's operand, no fp32 [B][T0][C] round trip through split3.
template <typename TO, bool RAW, bool FAST, bool LNG = false, bool OUT3 = false>
__global__ __launch_bounds__(256) void conv0_apply_kernel(const float* __restrict__ x, int L,
                                                          const float* __restrict__ norm,
                                                          const float* __restrict__ w0, const float* __restrict__ b0,
                                                          int C, int T0, const float2* __restrict__ ss,
                                                          TO* __restrict__ out, const float* __restrict__ lnw = nullptr,
                                                          const float* __restrict__ lnb = nullptr, float eps = 0.f) {
  constexpr int S0 = 5;
  __shared__ float xs[(C0_T - 1) * S0 + K0 + 2];
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int t0 = chunk * C0_T;
  const int nt = min(C0_T, T0 - t0);
  const int nx = (nt - 1) * S0 + K0;
  const float* xb = x + (long long)b * L + (long long)t0 * S0;
  float mu = 0.f, rs = 1.f;
  if (norm) { mu = norm[2 * b]; rs = norm[2 * b + 1]; }
  for (int i = threadIdx.x; i < nx; i += blockDim.x) xs[i] = norm ? (xb[i] - mu) * rs : xb[i];
  __syncthreads();
  // each lane owns 8 adjacent channels (4 packed-fp32 pairs: 4 independent FMA / GELU chains,
  // one 16-B store per frame); the block's 4 waves split the chunk's frames.  C % 8 == 0.
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int c = lane * 8; c < C; c += 512) {
    f32x2 w[4][K0], bias[4], sc[4], sh[4], gw[4], gb[4];
    #pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int c0 = c + 2 * p;
      #pragma unroll
      for (int j = 0; j < K0; ++j) w[p][j] = f32x2{w0[c0 * K0 + j], w0[(c0 + 1) * K0 + j]};
      bias[p] = b0 ? f32x2{b0[c0], b0[c0 + 1]} : f32x2{0.f, 0.f};
      sc[p] = f32x2{1.f, 1.f};
      sh[p] = f32x2{0.f, 0.f};
      if (!RAW) {
        const float2 s0v = ss[(long long)b * C + c0], s1v = ss[(long long)b * C + c0 + 1];
        sc[p] = f32x2{s0v.x, s1v.x};
        sh[p] = f32x2{s0v.y, s1v.y};
      }
      if (LNG) {
        gw[p] = f32x2{lnw[c0], lnw[c0 + 1]};
        gb[p] = f32x2{lnb[c0], lnb[c0 + 1]};
      }
    }
    TO* ob = out + ((long long)b * T0 + t0) * C + c;   // (OUT3 stores address the tripled rows below)
    if constexpr (LNG) {
      // two frames (t, t + 4) per trip: their reduction chains (DPP / permlane, each step dependent
      // on the previous) interleave instead of stalling one after the other
      for (int t = wv; t < nt; t += 8) {
        const bool two = t + 4 < nt;
        f32x2 y[2][4];
        #pragma unroll
        for (int f = 0; f < 2; ++f) {
          const int tf = two ? t + 4 * f : t;
          #pragma unroll
          for (int p = 0; p < 4; ++p) y[f][p] = bias[p];
          #pragma unroll
          for (int j = 0; j < K0; ++j) {
            const float xv = xs[tf * S0 + j];
            #pragma unroll
            for (int p = 0; p < 4; ++p) y[f][p] = __builtin_elementwise_fma(w[p][j], f32x2{xv, xv}, y[f][p]);
          }
        }
        float sm[2], qs[2], mean[2], rstd[2];
        #pragma unroll
        for (int f = 0; f < 2; ++f) {
          sm[f] = 0.f;
          #pragma unroll
          for (int p = 0; p < 4; ++p) sm[f] += y[f][p].x + y[f][p].y;
        }
        #pragma unroll
        for (int f = 0; f < 2; ++f) mean[f] = wave_sum_fast(sm[f]) / C;
        #pragma unroll
        for (int f = 0; f < 2; ++f) {
          qs[f] = 0.f;
          #pragma unroll
          for (int p = 0; p < 4; ++p) {
            const float d0 = y[f][p].x - mean[f], d1 = y[f][p].y - mean[f];
            qs[f] = fmaf(d0, d0, qs[f]);
            qs[f] = fmaf(d1, d1, qs[f]);
          }
        }
        #pragma unroll
        for (int f = 0; f < 2; ++f) rstd[f] = 1.0f / sqrtf(wave_sum_fast(qs[f]) / C + eps);
        #pragma unroll
        for (int f = 0; f < 2; ++f) {
          if (f == 1 && !two) break;
          f32x2 o[4];
          #pragma unroll
          for (int p = 0; p < 4; ++p) {
            const f32x2 z = {fmaf((y[f][p].x - mean[f]) * rstd[f], gw[p].x, gb[p].x),
                             fmaf((y[f][p].y - mean[f]) * rstd[f], gw[p].y, gb[p].y)};
            o[p] = FAST ? gelu_out2<!__is_same(TO, bf16)>(z) : gelu_erf2(z);
          }
          const long long row = (long long)(t + 4 * f) * C;
          if constexpr (OUT3) {   // split-fp16 path: tripled f16 rows of 3C
            f16x4 h0, l0, h1, l1;
            x3_split4(f32x4{o[0].x, o[0].y, o[1].x, o[1].y}, h0, l0);
            x3_split4(f32x4{o[2].x, o[2].y, o[3].x, o[3].y}, h1, l1);
            f16* o3 = (f16*)(void*)out + ((long long)b * T0 + t0 + t + 4 * f) * 3 * C + c;
            const f16x8 h = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
            *(f16x8*)o3 = h;
            *(f16x8*)(o3 + C) = f16x8{l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
            *(f16x8*)(o3 + 2 * C) = h;
          } else if constexpr (sizeof(TO) == 2) {
            *(uint4*)(ob + row) = pack_h8<is_f16_v<TO>>(f32x4{o[0].x, o[0].y, o[1].x, o[1].y},
                                                         f32x4{o[2].x, o[2].y, o[3].x, o[3].y});
          } else {
            *(f32x4*)((float*)ob + row) = f32x4{o[0].x, o[0].y, o[1].x, o[1].y};
            *(f32x4*)((float*)ob + row + 4) = f32x4{o[2].x, o[2].y, o[3].x, o[3].y};
          }
        }
      }
      continue;
    }
    for (int t = wv; t < nt; t += 4) {
      f32x2 y[4] = {bias[0], bias[1], bias[2], bias[3]};
      #pragma unroll
      for (int j = 0; j < K0; ++j) {
        const float xv = xs[t * S0 + j];
        #pragma unroll
        for (int p = 0; p < 4; ++p) y[p] = __builtin_elementwise_fma(w[p][j], f32x2{xv, xv}, y[p]);
      }
      if (!RAW) {
        #pragma unroll
        for (int p = 0; p < 4; ++p) {
          const f32x2 z = __builtin_elementwise_fma(y[p], sc[p], sh[p]);
          y[p] = FAST ? gelu_out2<!__is_same(TO, bf16)>(z) : gelu_erf2(z);
        }
      }
      if constexpr (OUT3) {
        f16x4 h0, l0, h1, l1;
        x3_split4(f32x4{y[0].x, y[0].y, y[1].x, y[1].y}, h0, l0);
        x3_split4(f32x4{y[2].x, y[2].y, y[3].x, y[3].y}, h1, l1);
        f16* o3 = (f16*)(void*)out + ((long long)b * T0 + t0 + t) * 3 * C + c;
        const f16x8 h = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
        *(f16x8*)o3 = h;
        *(f16x8*)(o3 + C) = f16x8{l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
        *(f16x8*)(o3 + 2 * C) = h;
      } else if constexpr (sizeof(TO) == 2) {
        *(uint4*)(ob + (long long)t * C) = pack_h8<is_f16_v<TO>>(f32x4{y[0].x, y[0].y, y[1].x, y[1].y},
                                                                   f32x4{y[2].x, y[2].y, y[3].x, y[3].y});
      } else {
        *(f32x4*)((float*)ob + (long long)t * C) = f32x4{y[0].x, y[0].y, y[1].x, y[1].y};
        *(f32x4*)((float*)ob + (long long)t * C + 4) = f32x4{y[2].x, y[2].y, y[3].x, y[3].y};
      }
    }
  }
}

// ---- bf16 GroupNorm path on the matrix cores ----
// conv0 as MFMAs: out[t][c] = w_c . x_t with K = 10 taps.  v_mfma_f32_16x16x32_bf16 has K = 32, which
// holds the three terms of a split-bf16 product, x = xh + xl, w = wh + wl (hi = RNE bf16, lo = bf16
// of the exact remainder): sum_j xh wh + xl wh + xh wl (the dropped xl wl is ~2^-16 relative), so
// one MFMA evaluates a 16-channel x 16-frame block of the fp32 convolution to ~1e-5 -- far below
// the bf16 output rounding -- and the VALU is left with the GroupNorm affine, GELU and the packing.
// K slots per lane group q (A = weights of channel r16, B = taps of frame r16):
//   q0: xh0-7 | wh0-7   q1: xh8,9 xl0-5 | wh8,9 wh0-5   q2: xl6-9 xh0-3 | wh6-9 wl0-3   q3: xh4-9 0 0 | wl4-9 0 0
// MFMAs compute C^T (channels x frames), so a lane holds 4 consecutive channels of one frame; two
// channel blocks per step and a v_permlane16_swap give every lane 8 consecutive bf16 = one 16-B store.
constexpr int C0M_T = 32;
constexpr int C0M_C = 512;               // channels of the matrix-core conv0 (conv0_wfrag fragments)

// A block owns one clip and walks its 32-frame chunks (blockIdx.x, + gridDim.x, ...): the clip's
// weights and GroupNorm affine stay in registers, the next chunk's waveform is fetched while this
// chunk computes, and the LDS tile turns the MFMA layout (4 channels x 16 frames per lane group)
// into whole 1 KiB row stores that drain while the next chunk computes (one short-lived block per
// chunk, or lane-scattered 64-B row pieces, both left the kernel at half the fill bandwidth).
// Wave w computes channel blocks cb = w, w+4, ..., both 16-frame blocks of the chunk.
typedef unsigned int u32x4nt __attribute__((ext_vector_type(4)));
constexpr int C0M_PAD = 16;              // bf16 per tile row of padding: row stride = 8 banks mod 64

template <typename TO>   // bf16 or fp16 output (the products are split-bf16 either way)
__global__ __launch_bounds__(256) void conv0_mfma_kernel(const float* __restrict__ x, int L,
                                                         const float* __restrict__ norm,
                                                         const bf16x8* __restrict__ wf, const float* __restrict__ b0,
                                                         int T0, const float2* __restrict__ ss,
                                                         TO* __restrict__ out) {
  constexpr int S0 = 5, C = 512, NCB = C / 16 / 4;
  __shared__ float xs[(C0M_T - 1) * S0 + K0 + 2];
  __shared__ __attribute__((aligned(16))) bf16 tile[C0M_T][C + C0M_PAD];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int nchunk = (T0 + C0M_T - 1) / C0M_T;
  const float* xb = x + (long long)b * L;
  float mu = 0.f, rs = 1.f;
  if (norm) { mu = norm[2 * b]; rs = norm[2 * b + 1]; }
  const int lane = tid & 63, wv = tid >> 6, q = lane >> 4, r16 = lane & 15;
  bf16x8 wfr[NCB];
  f32x2 sc0[NCB], sh0[NCB], sc1[NCB], sh1[NCB];
  {
    const float2* ssb = ss + (long long)b * C;
    #pragma unroll
    for (int i = 0; i < NCB; ++i) {
      const int cb = wv + 4 * i, c = cb * 16 + 4 * q;
      wfr[i] = wf[cb * 64 + lane];
      const f32x4 s01 = *(const f32x4*)(ssb + c), s23 = *(const f32x4*)(ssb + c + 2);
      sc0[i] = f32x2{s01[0], s01[2]}; sh0[i] = f32x2{s01[1], s01[3]};
      sc1[i] = f32x2{s23[0], s23[2]}; sh1[i] = f32x2{s23[1], s23[3]};
      if (b0) {
        const f32x4 bb = *(const f32x4*)(b0 + c);
        sh0[i] = __builtin_elementwise_fma(f32x2{bb[0], bb[1]}, sc0[i], sh0[i]);
        sh1[i] = __builtin_elementwise_fma(f32x2{bb[2], bb[3]}, sc1[i], sh1[i]);
      }
    }
  }
  auto fetch = [&](int ch) {
    const int t0 = ch * C0M_T, nt = min(C0M_T, T0 - t0), nx = (nt - 1) * S0 + K0;
    return tid < nx ? xb[(long long)t0 * S0 + tid] : 0.f;
  };
  float xv = blockIdx.x < nchunk ? fetch(blockIdx.x) : 0.f;
  for (int ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    const int t0 = ch * C0M_T, nt = min(C0M_T, T0 - t0);
    __syncthreads();                                // previous chunk: xs read, tile rows stored
    if (tid < (C0M_T - 1) * S0 + K0) xs[tid] = norm ? (xv - mu) * rs : xv;
    __syncthreads();
    bf16x8 xf[C0M_T / 16];
    #pragma unroll
    for (int fb = 0; fb < C0M_T / 16; ++fb) {
      const int tl = fb * 16 + r16;
      bf16 h[K0], l[K0];
      #pragma unroll
      for (int j = 0; j < K0; ++j) c0m_split(tl < nt ? xs[tl * S0 + j] : 0.f, h[j], l[j]);
      const bf16 z = (bf16)0.f;
      if (q == 0) xf[fb] = bf16x8{h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]};
      else if (q == 1) xf[fb] = bf16x8{h[8], h[9], l[0], l[1], l[2], l[3], l[4], l[5]};
      else if (q == 2) xf[fb] = bf16x8{l[6], l[7], l[8], l[9], h[0], h[1], h[2], h[3]};
      else xf[fb] = bf16x8{h[4], h[5], h[6], h[7], h[8], h[9], z, z};
    }
    if (ch + (int)gridDim.x < nchunk) xv = fetch(ch + gridDim.x);
    #pragma unroll
    for (int i = 0; i < NCB; ++i) {
      const int c = (wv + 4 * i) * 16 + 4 * q;
      #pragma unroll
      for (int fb = 0; fb < C0M_T / 16; ++fb) {
        const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[i], xf[fb], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        const f32x2 o0 = gelu_out2<!__is_same(TO, bf16)>(__builtin_elementwise_fma(f32x2{acc[0], acc[1]}, sc0[i], sh0[i]));
        const f32x2 o1 = gelu_out2<!__is_same(TO, bf16)>(__builtin_elementwise_fma(f32x2{acc[2], acc[3]}, sc1[i], sh1[i]));
        *(uint2*)&tile[fb * 16 + r16][c] = pack_h4<is_f16_v<TO>>(f32x4{o0.x, o0.y, o1.x, o1.y});
      }
    }
    __syncthreads();
    TO* ob = out + ((long long)b * T0 + t0) * C;
    // non-temporal: the 2.5 GB (B = 256) output streams past L2 (conv1 reads it back from HBM either way)
    for (int r = wv; r < nt; r += 4)
      __builtin_nontemporal_store(*(const u32x4nt*)&tile[r][lane * 8], (u32x4nt*)(ob + (long long)r * C + lane * 8));
  }
}

// moments [B][MOM_NCH][NMOM] fp64 | the matrix-core conv0's weight fragments (C0M_C / 16 x 64 lanes x 16 B)
size_t conv0_moments_bytes(int B) {
  return ((size_t)B * MOM_NCH * NMOM * sizeof(double) + 255) / 256 * 256 + C0M_C / 16 * 64 * 16;
}


template <typename TO>
int launch_conv0_gn(const float* x, int B, int L, const float* norm, const float* w0, const float* b0,
                    int C, int k0, int s0, int T0, const float* gamma, const float* beta, float eps,
                    double* mom, float2* ss, TO* out, hipStream_t s, const int* t0len) {
  if (k0 != K0 || s0 != 5) return -3;
  if (C % 8) return -3;
  dim3 grid((T0 + C0_T - 1) / C0_T, B), block(256);
  const bool valu = sse_opt(OPT_CONV0_VALU) != 0;   // A/B and tests: the VALU kernel below
  // matrix-core conv0: C == C0M_C channels, whose weight fragments conv0_moments_bytes reserves
  const bool mfma = sizeof(TO) == 2 && !gelu_exact_env() && C == C0M_C && !valu;
  bf16x8* wf = mfma ? (bf16x8*)((char*)mom + ((size_t)B * MOM_NCH * NMOM * sizeof(double) + 255) / 256 * 256)
                    : nullptr;
  hipLaunchKernelGGL(conv0_moments_kernel, dim3(MOM_NCH, B), dim3(256), 0, s, x, L, norm, s0, T0, mom, t0len);
  hipLaunchKernelGGL(gn_finalize_kernel, dim3((C + 255) / 256, B), dim3(256), 0, s, mom, B, C, T0, w0, b0, gamma,
                     beta, eps, ss, t0len, wf);
  if (mfma) {
    // 3 resident blocks per CU (168 VGPRs): spread each clip's chunks over G blocks, G * B ~ 3 * CUs
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -2;
    if (!cus[dev] && hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      return -2;
    const int nchunk = (T0 + C0M_T - 1) / C0M_T;
    int G = (3 * sse_stream_cus(s, cus[dev]) + B - 1) / B;
    G = G < 1 ? 1 : (G > nchunk ? nchunk : G);
    hipLaunchKernelGGL(conv0_mfma_kernel<TO>, dim3(G, B), dim3(256), 0, s, x, L, norm, (const bf16x8*)wf, b0, T0,
                       (const float2*)ss, out);
  } else if (sizeof(TO) == 2 && !gelu_exact_env())   // bf16 output: gelu_fast2 (common.h)
    hipLaunchKernelGGL((conv0_apply_kernel<TO, false, true>), grid, block, 0, s, x, L, norm, w0, b0, C, T0, ss, out);
  else
    hipLaunchKernelGGL((conv0_apply_kernel<TO, false, false>), grid, block, 0, s, x, L, norm, w0, b0, C, T0, ss, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// split-fp16 path: conv0 + GroupNorm + erf-GELU in fp32, written as tripled f16 rows (OUT3)
int launch_conv0_gn_x3(const float* x, int B, int L, const float* norm, const float* w0, const float* b0, int C,
                       int k0, int s0, int T0, const float* gamma, const float* beta, float eps, double* mom,
                       float2* ss, f16* out3, hipStream_t s, const int* t0len) {
  if (k0 != K0 || s0 != 5 || C % 8) return -3;
  hipLaunchKernelGGL(conv0_moments_kernel, dim3(MOM_NCH, B), dim3(256), 0, s, x, L, norm, s0, T0, mom, t0len);
  hipLaunchKernelGGL(gn_finalize_kernel, dim3((C + 255) / 256, B), dim3(256), 0, s, mom, B, C, T0, w0, b0, gamma,
                     beta, eps, ss, t0len, (bf16x8*)nullptr);
  hipLaunchKernelGGL((conv0_apply_kernel<float, false, false, false, true>), dim3((T0 + C0_T - 1) / C0_T, B),
                     dim3(256), 0, s, x, L, norm, w0, b0, C, T0, ss, (float*)out3);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// split-fp16 path, "layer" frontend (WavLM-large): conv0 + LayerNorm(512) + erf-GELU in fp32, written as
// tripled f16 rows (OUT3); -3: not covered
int launch_conv0_ln_x3(const float* x, int B, int L, const float* norm, const float* w0, const float* b0, int C,
                       int k0, int s0, int T0, const float* lnw, const float* lnb, float eps, f16* out3, hipStream_t s) {
  if (k0 != K0 || s0 != 5 || C != 512) return -3;
  hipLaunchKernelGGL((conv0_apply_kernel<float, true, false, true, true>), dim3((T0 + C0_T - 1) / C0_T, B), dim3(256),
                     0, s, x, L, norm, w0, b0, C, T0, (const float2*)nullptr, (float*)out3, lnw, lnb, eps);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// conv0 without GroupNorm/GELU (WavLM-large "layer" frontend: LN + GELU follow per frame)
template <typename TO>
int launch_conv0_raw(const float* x, int B, int L, const float* norm, const float* w0, const float* b0, int C,
                     int k0, int s0, int T0, TO* out, hipStream_t s) {
  if (k0 != K0 || s0 != 5) return -3;
  if (C % 8) return -3;
  dim3 grid((T0 + C0_T - 1) / C0_T, B), block(256);
  hipLaunchKernelGGL((conv0_apply_kernel<TO, true, false>), grid, block, 0, s, x, L, norm, w0, b0, C, T0,
                     (const float2*)nullptr, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
// conv0 + LayerNorm(C) + GELU in one pass ("layer" frontend, C == 512); -3: not covered (the caller
// runs launch_conv0_raw + launch_layernorm)
template <typename TO>
int launch_conv0_ln(const float* x, int B, int L, const float* norm, const float* w0, const float* b0, int C, int k0,
                    int s0, int T0, const float* lnw, const float* lnb, float eps, TO* out, hipStream_t s) {
  if (k0 != K0 || s0 != 5 || C != 512) return -3;
  dim3 grid((T0 + C0_T - 1) / C0_T, B), block(256);
  if (sizeof(TO) == 2 && !gelu_exact_env())   // bf16 output: gelu_fast2 (common.h)
    hipLaunchKernelGGL((conv0_apply_kernel<TO, true, true, true>), grid, block, 0, s, x, L, norm, w0, b0, C, T0,
                       (const float2*)nullptr, out, lnw, lnb, eps);
  else
    hipLaunchKernelGGL((conv0_apply_kernel<TO, true, false, true>), grid, block, 0, s, x, L, norm, w0, b0, C, T0,
                       (const float2*)nullptr, out, lnw, lnb, eps);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template int launch_conv0_ln<float>(const float*, int, int, const float*, const float*, const float*, int, int, int,
                                    int, const float*, const float*, float, float*, hipStream_t);
template int launch_conv0_ln<bf16>(const float*, int, int, const float*, const float*, const float*, int, int, int,
                                   int, const float*, const float*, float, bf16*, hipStream_t);
template int launch_conv0_raw<float>(const float*, int, int, const float*, const float*, const float*, int, int, int,
                                     int, float*, hipStream_t);
template int launch_conv0_raw<bf16>(const float*, int, int, const float*, const float*, const float*, int, int, int,
                                    int, bf16*, hipStream_t);
template int launch_conv0_gn<float>(const float*, int, int, const float*, const float*, const float*, int, int,
                                    int, int, const float*, const float*, float, double*, float2*, float*,
                                    hipStream_t, const int*);
template int launch_conv0_gn<bf16>(const float*, int, int, const float*, const float*, const float*, int, int,
                                   int, int, const float*, const float*, float, double*, float2*, bf16*,
                                   hipStream_t, const int*);
template int launch_conv0_gn<f16>(const float*, int, int, const float*, const float*, const float*, int, int,
                                  int, int, const float*, const float*, float, double*, float2*, f16*,
                                  hipStream_t, const int*);
template int launch_conv0_ln<f16>(const float*, int, int, const float*, const float*, const float*, int, int, int,
                                  int, const float*, const float*, float, f16*, hipStream_t);
template int launch_conv0_raw<f16>(const float*, int, int, const float*, const float*, const float*, int, int, int,
                                   int, f16*, hipStream_t);

// ---------------------------------------------------------------------------------------
// LayerNorm over rows of H (H % 4 == 0, H <= 2048).  One wave per row, 4 rows per block;
// lane l handles 4-element groups l, l+64, ... (16-B fp32 / 8-B bf16 accesses).
template <typename TI> SSE_DEV f32x4 load4(const TI* p);
template <> SSE_DEV f32x4 load4<float>(const float* p) { return *(const f32x4*)p; }
template <> SSE_DEV f32x4 load4<bf16>(const bf16* p) {
  const bf16x4 v = *(const bf16x4*)p;
  return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
template <> SSE_DEV f32x4 load4<f16>(const f16* p) {
  const f16x4 v = *(const f16x4*)p;
  return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
// a split-fp16 value from its hi plane (p) and lo' plane (p + H): hi + lo' * 2^-11
SSE_DEV f32x4 load4_x3(const f16* p, int H) {
  const f16x4 h = *(const f16x4*)p, l = *(const f16x4*)(p + H);
  f32x4 o;
  #pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = fmaf((float)l[e], 1.f / X3_LO_SCALE, (float)h[e]);
  return o;
}

// MX-fp8 quantisation of 4 consecutive values (columns c..c+3 of row `row`, K = H) held by a lane
// whose 7 neighbours (lane ^ 1, 2, 4) hold the rest of the 32-column block: amax, E8M0 exponent
// (mx_scale_exp), e4m3 = RNE(x * 2^-E), one dword store; lane % 8 == 0 stores the scale byte.
SSE_DEV void mx_quant4(f32x4 o, unsigned char* dst, unsigned char* scale, long long row, int c, int K, int lane) {
  const float a = max8_dpp(__builtin_elementwise_maximum(__builtin_elementwise_maximum(fabsf(o[0]), fabsf(o[1])),
                                                               __builtin_elementwise_maximum(fabsf(o[2]), fabsf(o[3]))));
  const int e = mx_scale_exp(a);
  const float inv = mx_inv_scale(e);
  int x = __builtin_amdgcn_cvt_pk_fp8_f32(o[0] * inv, o[1] * inv, 0, false);
  x = __builtin_amdgcn_cvt_pk_fp8_f32(o[2] * inv, o[3] * inv, x, true);
  *(int*)dst = x;
  if ((lane & 7) == 0) scale[mx_a_scale_off(row, c >> 5, K >> 7)] = (unsigned char)e;
}

// IN3 / OUT3 (split-fp16 path, TI / TO = f16): rows are tripled [hi | lo' | hi] of 3H (x3_split4);
// the input value is hi + lo' 2^-11.
template <typename TI, typename TO, bool IN3 = false, bool OUT3 = false>
__global__ __launch_bounds__(256) void layernorm_kernel(const TI* __restrict__ in, const float* __restrict__ w,
                                                        const float* __restrict__ bta, int rows, int H,
                                                        float eps, int act, float* __restrict__ out_f,
                                                        TO* __restrict__ out_t, float2* __restrict__ stats) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int n4 = H >> 2;
  const TI* x = in + (long long)row * H * (IN3 ? 3 : 1);
  f32x4 v[8];
  float s = 0.f;
  #pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int g = lane + 64 * i;
    if (g < n4) {
      if constexpr (IN3) v[i] = load4_x3(x + 4 * g, H);
      else v[i] = load4<TI>(x + 4 * g);
      s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
    }
  }
  const float mean = wave_sum(s) / H;
  float q = 0.f;
  #pragma unroll
  for (int i = 0; i < 8; ++i)
    if (lane + 64 * i < n4)
      #pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = v[i][e] - mean;
        q = fmaf(d, d, q);
      }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / H + eps);
  if constexpr (sizeof(TO) != 1)
    if (stats && lane == 0) stats[row] = make_float2(mean, rstd);
  #pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int g = lane + 64 * i;
    if (g < n4) {
      const int c = 4 * g;
      const f32x4 wv = *(const f32x4*)(w + c), bv = *(const f32x4*)(bta + c);
      f32x4 o;
      #pragma unroll
      for (int e = 0; e < 4; ++e) {
        float y = fmaf((v[i][e] - mean) * rstd, wv[e], bv[e]);   // = ln_apply4 (common.h)
        o[e] = act == ACT_GELU ? gelu_erf(y) : y;
      }
      const long long off = (long long)row * H + c;
      if (out_f) *(f32x4*)(out_f + off) = o;
      if constexpr (OUT3) {
        const long long o3 = (long long)row * 3 * H + c;
        f16x4 hi, lo;
        x3_split4(o, hi, lo);
        *(f16x4*)((f16*)out_t + o3) = hi;
        *(f16x4*)((f16*)out_t + o3 + H) = lo;
        *(f16x4*)((f16*)out_t + o3 + 2 * H) = hi;
      } else if constexpr (sizeof(TO) == 1) {
        // MX-fp8 GEMM operand (A layout): 8 lanes = one 32-column block (H % 32 == 0, so a block's
        // lanes are active together); out_t is e4m3 bytes, stats carries the scale tensor
        mx_quant4(o, (unsigned char*)out_t + off, (unsigned char*)stats, row, c, H, lane);
      } else if (out_t) {
        if constexpr (sizeof(TO) == 2) {
          *(uint2*)(out_t + off) = pack_h4<is_f16_v<TO>>(o);
        } else {
          *(f32x4*)(out_t + off) = o;
        }
      }
    }
  }
}

// bf16 -> bf16 LayerNorm of narrow rows (H <= 512: the WavLM conv frontend's per-layer LN + GELU
// and the feature projection's LN): one 16-B load per lane per row, R rows per wave with every load
// issued first (the one-row-per-wave kernel keeps only 1 KiB in flight per wave: ~2.4 TB/s on these
// rows), DPP/permlane reductions for the R rows interleaved.  GELU: the bf16 path's gelu_fast2.
// NC > 1 (round 3): rows of up to 512 NC columns (WavLM-large 1024, Whisper 1280 / 768) with R = 2 rows per
// wave, the weight / bias of the lane's columns loaded once per wave (the one-row-per-wave
// layernorm_kernel re-read them per row: 4x the row's own bytes through L1).
template <int R, bool H16 = false, int NC = 1>   // H16: fp16 rows (SSE_DTYPE_FP16) in bf16x8 containers
__global__ __launch_bounds__(256) void layernorm_bf16_rows_kernel(const bf16* __restrict__ in, const float* __restrict__ w,
                                                                  const float* __restrict__ bta, int rows, int H,
                                                                  float eps, int act, bf16* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r0 = ((long long)blockIdx.x * 4 + wave) * R;
  bool on[NC];
  #pragma unroll
  for (int k = 0; k < NC; ++k) on[k] = 512 * k + 8 * lane < H;
  bf16x8 v[R][NC];
  #pragma unroll
  for (int i = 0; i < R; ++i) {
    const long long row = r0 + i;
    #pragma unroll
    for (int k = 0; k < NC; ++k)
      v[i][k] = (on[k] && row < rows) ? *(const bf16x8*)(in + row * H + 512 * k + lane * 8) : bf16x8{};
  }
  f32x4 w0[NC], w1[NC], b0[NC], b1[NC];
  #pragma unroll
  for (int k = 0; k < NC; ++k) {
    w0[k] = f32x4{1.f, 1.f, 1.f, 1.f}; w1[k] = w0[k]; b0[k] = f32x4{0.f, 0.f, 0.f, 0.f}; b1[k] = b0[k];
    if (on[k]) {
      const int c = 512 * k + lane * 8;
      w0[k] = *(const f32x4*)(w + c);
      w1[k] = *(const f32x4*)(w + c + 4);
      b0[k] = *(const f32x4*)(bta + c);
      b1[k] = *(const f32x4*)(bta + c + 4);
    }
  }
  float x[R][NC][8], mean[R], rstd[R];
  #pragma unroll
  for (int i = 0; i < R; ++i) {
    float sm = 0.f;
    #pragma unroll
    for (int k = 0; k < NC; ++k)
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        x[i][k][e] = hval<H16>(v[i][k][e]);
        sm += x[i][k][e];
      }
    mean[i] = sm;
  }
  #pragma unroll
  for (int i = 0; i < R; ++i) mean[i] = wave_sum_fast(mean[i]) / H;
  #pragma unroll
  for (int i = 0; i < R; ++i) {
    float q = 0.f;
    #pragma unroll
    for (int k = 0; k < NC; ++k)
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = on[k] ? x[i][k][e] - mean[i] : 0.f;
        q = fmaf(d, d, q);
      }
    rstd[i] = q;
  }
  #pragma unroll
  for (int i = 0; i < R; ++i) rstd[i] = 1.0f / sqrtf(wave_sum_fast(rstd[i]) / H + eps);
  #pragma unroll
  for (int i = 0; i < R; ++i) {
    const long long row = r0 + i;
    #pragma unroll
    for (int k = 0; k < NC; ++k) {
      float y[8];
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float wv = e < 4 ? w0[k][e] : w1[k][e - 4], bv = e < 4 ? b0[k][e] : b1[k][e - 4];
        y[e] = fmaf((x[i][k][e] - mean[i]) * rstd[i], wv, bv);   // = ln_apply4
      }
      if (act != ACT_NONE) {
        #pragma unroll
        for (int e = 0; e < 8; e += 2) {
          const f32x2 g2 = act == ACT_GELU ? gelu_erf2(f32x2{y[e], y[e + 1]}) : gelu_out2<H16>(f32x2{y[e], y[e + 1]});
          y[e] = g2.x;
          y[e + 1] = g2.y;
        }
      }
      if (on[k] && row < rows) {
        *(uint4*)(out + row * H + 512 * k + lane * 8) =
            pack_h8<H16>(f32x4{y[0], y[1], y[2], y[3]}, f32x4{y[4], y[5], y[6], y[7]});
      }
    }
  }
}

template <typename TI, typename TO>
int launch_layernorm(const TI* in, const float* w, const float* b, int rows, int H, float eps, int act,
                     float* out_f, TO* out_t, hipStream_t s, float2* stats) {
  if (H % 4 || H > 2048) return -3;
  if constexpr (sizeof(TI) == 2 && sizeof(TO) == 2) {
    static_assert(is_f16_v<TI> == is_f16_v<TO>, "16-bit LayerNorm: one format in and out");
    if (H % 8 == 0 && H <= 512 && !out_f && !stats && out_t) {
      constexpr int R = 4;
      const int a2 = act == ACT_GELU && !gelu_exact_env() ? (int)ACT_GELU_FAST : act;   // 16-bit output
      hipLaunchKernelGGL((layernorm_bf16_rows_kernel<R, is_f16_v<TO>>), dim3((rows + 4 * R - 1) / (4 * R)), dim3(256), 0,
                         s, (const bf16*)in, w, b, rows, H, eps, a2, (bf16*)out_t);
      return hipGetLastError() == hipSuccess ? 0 : -2;
    }
    if (H % 8 == 0 && H > 512 && H <= 2048 && act == ACT_NONE && !out_f && !stats && out_t && !sse_opt(OPT_LN_ROWS_V1)) {
      constexpr int R = 2;
      const dim3 g((rows + 4 * R - 1) / (4 * R));
      switch ((H + 511) / 512) {
        case 2: hipLaunchKernelGGL((layernorm_bf16_rows_kernel<R, is_f16_v<TO>, 2>), g, dim3(256), 0, s, (const bf16*)in, w,
                                   b, rows, H, eps, act, (bf16*)out_t); break;
        case 3: hipLaunchKernelGGL((layernorm_bf16_rows_kernel<R, is_f16_v<TO>, 3>), g, dim3(256), 0, s, (const bf16*)in, w,
                                   b, rows, H, eps, act, (bf16*)out_t); break;
        default: hipLaunchKernelGGL((layernorm_bf16_rows_kernel<R, is_f16_v<TO>, 4>), g, dim3(256), 0, s, (const bf16*)in, w,
                                    b, rows, H, eps, act, (bf16*)out_t); break;
      }
      return hipGetLastError() == hipSuccess ? 0 : -2;
    }
  }
  hipLaunchKernelGGL((layernorm_kernel<TI, TO>), dim3((rows + 3) / 4), dim3(256), 0, s, in, w, b, rows, H, eps,
                     act, out_f, out_t, stats);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template int launch_layernorm<float, float>(const float*, const float*, const float*, int, int, float, int,
                                            float*, float*, hipStream_t, float2*);

// split-fp16 LayerNorm of fp32 rows, H = 256 NI: R rows per wave with every load issued first (the
// one-row-per-wave layernorm_kernel keeps 3 KiB in flight per wave and ran at ~1.3 TB/s on the
// fp16x3 path's 50 launches per step); the same per-lane sums, wave_sum and expressions as
// layernorm_kernel<float, f16, false, true>, so the outputs are bit-identical to it.
template <int R, int NI>
__global__ __launch_bounds__(256) void layernorm_x3_rows_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                                const float* __restrict__ bta, int rows, float eps,
                                                                float* __restrict__ out_f, f16* __restrict__ out3) {
  constexpr int H = NI * 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r0 = ((long long)blockIdx.x * 4 + wave) * R;
  f32x4 v[R][NI];
  #pragma unroll
  for (int i = 0; i < R; ++i)
    #pragma unroll
    for (int k = 0; k < NI; ++k)
      v[i][k] = r0 + i < rows ? *(const f32x4*)(in + (r0 + i) * H + 4 * (lane + 64 * k)) : f32x4{0.f, 0.f, 0.f, 0.f};
  float mean[R], rstd[R];
  #pragma unroll
  for (int i = 0; i < R; ++i) {
    float sm = 0.f;
    #pragma unroll
    for (int k = 0; k < NI; ++k) sm += v[i][k][0] + v[i][k][1] + v[i][k][2] + v[i][k][3];
    mean[i] = sm;
  }
  #pragma unroll
  for (int i = 0; i < R; ++i) mean[i] = wave_sum(mean[i]) / H;
  #pragma unroll
  for (int i = 0; i < R; ++i) {
    float q = 0.f;
    #pragma unroll
    for (int k = 0; k < NI; ++k)
      #pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = v[i][k][e] - mean[i];
        q = fmaf(d, d, q);
      }
    rstd[i] = q;
  }
  #pragma unroll
  for (int i = 0; i < R; ++i) rstd[i] = 1.0f / sqrtf(wave_sum(rstd[i]) / H + eps);
  #pragma unroll
  for (int k = 0; k < NI; ++k) {
    const int c = 4 * (lane + 64 * k);
    const f32x4 wv = *(const f32x4*)(w + c), bv = *(const f32x4*)(bta + c);
    #pragma unroll
    for (int i = 0; i < R; ++i) {
      const long long row = r0 + i;
      if (row >= rows) break;
      f32x4 o;
      #pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = fmaf((v[i][k][e] - mean[i]) * rstd[i], wv[e], bv[e]);   // = ln_apply4
      if (out_f) *(f32x4*)(out_f + row * H + c) = o;
      f16x4 hi, lo;
      x3_split4(o, hi, lo);
      f16* o3 = out3 + row * 3 * H + c;
      *(f16x4*)o3 = hi;
      *(f16x4*)(o3 + H) = lo;
      *(f16x4*)(o3 + 2 * H) = hi;
    }
  }
}

// split-fp16 LayerNorm: input fp32 [rows][H] or tripled f16 [rows][3H] (in3), output fp32 (optional)
// and tripled f16 [rows][3H]
int launch_layernorm_x3(const void* in, bool in3, const float* w, const float* b, int rows, int H, float eps,
                        float* out_f, f16* out3, hipStream_t s, int act) {
  if (H % 4 || H > 2048 || !out3) return -3;
  constexpr int R = 4;
  if (act != ACT_NONE) {   // LayerNorm + erf-GELU (the "layer" conv frontend)
    if (in3 || act != ACT_GELU) return -3;
    hipLaunchKernelGGL((layernorm_kernel<float, f16, false, true>), dim3((rows + 3) / 4), dim3(256), 0, s,
                       (const float*)in, w, b, rows, H, eps, act, out_f, out3, (float2*)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : -2;
  }
  if (!in3 && H == 768 && !sse_opt(OPT_LN_X3_V1))
    hipLaunchKernelGGL((layernorm_x3_rows_kernel<R, 3>), dim3((rows + 4 * R - 1) / (4 * R)), dim3(256), 0, s,
                       (const float*)in, w, b, rows, eps, out_f, out3);
  else if (in3)
    hipLaunchKernelGGL((layernorm_kernel<f16, f16, true, true>), dim3((rows + 3) / 4), dim3(256), 0, s,
                       (const f16*)in, w, b, rows, H, eps, (int)ACT_NONE, out_f, out3, (float2*)nullptr);
  else
    hipLaunchKernelGGL((layernorm_kernel<float, f16, false, true>), dim3((rows + 3) / 4), dim3(256), 0, s,
                       (const float*)in, w, b, rows, H, eps, (int)ACT_NONE, out_f, out3, (float2*)nullptr);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// fp32 [rows][C] -> tripled f16 [rows][3C] ([hi | lo' | hi], x3_split4), 4 values per thread
__global__ __launch_bounds__(256) void split3_kernel(const float* __restrict__ x, long long n4, int C,
                                                     f16* __restrict__ y) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const long long e = i * 4, r = e / C, c = e - r * C;
  f16x4 hi, lo;
  x3_split4(*(const f32x4*)(x + e), hi, lo);
  f16* o = y + r * 3 * C + c;
  *(f16x4*)o = hi;
  *(f16x4*)(o + C) = lo;
  *(f16x4*)(o + 2 * C) = hi;
}

int launch_split3(const float* x, long long rows, int C, f16* y, hipStream_t s) {
  if (C % 4) return -3;
  const long long n4 = rows * C / 4;
  hipLaunchKernelGGL(split3_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, x, n4, C, y);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template int launch_layernorm<float, bf16>(const float*, const float*, const float*, int, int, float, int,
                                           float*, bf16*, hipStream_t, float2*);
template int launch_layernorm<bf16, bf16>(const bf16*, const float*, const float*, int, int, float, int, float*,
                                          bf16*, hipStream_t, float2*);
template int launch_layernorm<bf16, float>(const bf16*, const float*, const float*, int, int, float, int, float*,
                                           float*, hipStream_t, float2*);
template int launch_layernorm<float, f16>(const float*, const float*, const float*, int, int, float, int,
                                          float*, f16*, hipStream_t, float2*);
template int launch_layernorm<f16, f16>(const f16*, const float*, const float*, int, int, float, int, float*,
                                        f16*, hipStream_t, float2*);
template int launch_layernorm<f16, float>(const f16*, const float*, const float*, int, int, float, int, float*,
                                          float*, hipStream_t, float2*);

// LayerNorm -> MX-fp8 GEMM operand (pre-LN Whisper, SSE_DTYPE_FP8).  Block = 64 consecutive rows
// (4 waves x 16 rows, one row per wave at a time, the layernorm_kernel arithmetic), so the block
// owns whole A-layout scale dwords (rows r16 + 16i, i = 0..3, of its 64-row group): the E8M0 bytes
// go to LDS and leave as one dword store per (r16, block) instead of one byte store per
// (row, block).  Data: e4m3 dwords (4 columns per lane).
constexpr int LNMX_MAXB = 2048 / 32;
// One wave per row, 16 rows per wave walked with the NEXT row's loads issued before this row's
// math (two rows in flight per wave), lane-sliced 16-B loads, DPP / permlane reductions (no LDS
// round trips): the kernel streams the fp32 residual at HBM rate instead of paying one exposed
// round trip per row.
template <typename TI, int NI>
__global__ __launch_bounds__(256) void layernorm_mx_kernel(const TI* __restrict__ in, const float* __restrict__ w,
                                                           const float* __restrict__ bta, int rows, int H, float eps,
                                                           unsigned char* __restrict__ q, unsigned char* __restrict__ scale) {
  __shared__ unsigned char sc[64 * LNMX_MAXB];
  const int r0 = blockIdx.x * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n4 = H >> 2, nb = H >> 5;
  const float inv_h = 1.0f / (float)H;
  f32x4 cur[NI], nxt[NI];
  auto load = [&](f32x4 (&v)[NI], int row) {
    const TI* x = in + (long long)(row < rows ? row : rows - 1) * H;
    #pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int g = lane + 64 * i;
      v[i] = g < n4 ? load4<TI>(x + 4 * g) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  load(cur, r0 + wave);
  for (int rr = wave; rr < 64; rr += 4) {
    const int row = r0 + rr;
    if (row >= rows) break;
    if (rr + 4 < 64) load(nxt, row + 4);
    float s = 0.f;
    #pragma unroll
    for (int i = 0; i < NI; ++i) s += (cur[i][0] + cur[i][1]) + (cur[i][2] + cur[i][3]);
    const float mean = wave_sum_fast(s) * inv_h;
    float qs = 0.f;
    #pragma unroll
    for (int i = 0; i < NI; ++i)
      if (lane + 64 * i < n4)
        #pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = cur[i][e] - mean;
          qs = fmaf(d, d, qs);
        }
    const float rstd = 1.0f / sqrtf(wave_sum_fast(qs) * inv_h + eps);
    #pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int g = lane + 64 * i;
      if (g < n4) {
        const int c = 4 * g;
        const f32x4 wv = *(const f32x4*)(w + c), bv = *(const f32x4*)(bta + c);
        f32x4 o;
        #pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaf((cur[i][e] - mean) * rstd, wv[e], bv[e]);   // = ln_apply4
        const float a = max8_dpp(__builtin_elementwise_maximum(__builtin_elementwise_maximum(fabsf(o[0]), fabsf(o[1])),
                                                               __builtin_elementwise_maximum(fabsf(o[2]), fabsf(o[3]))));
        const int e8 = mx_scale_exp(a);
        const float inv = mx_inv_scale(e8);
        int xq = __builtin_amdgcn_cvt_pk_fp8_f32(o[0] * inv, o[1] * inv, 0, false);
        xq = __builtin_amdgcn_cvt_pk_fp8_f32(o[2] * inv, o[3] * inv, xq, true);
        *(int*)(q + (long long)row * H + c) = xq;
        if ((lane & 7) == 0) sc[rr * LNMX_MAXB + (c >> 5)] = (unsigned char)e8;
      }
    }
    #pragma unroll
    for (int i = 0; i < NI; ++i) cur[i] = nxt[i];
  }
  __syncthreads();
  // scale dwords of this 64-row group: (r16, block) -> bytes i = 0..3 of rows r16 + 16i
  for (int u = threadIdx.x; u < 16 * nb; u += 256) {
    const int r16 = u & 15, blk = u >> 4;
    if (r0 + r16 >= rows) continue;
    const unsigned v = (unsigned)sc[r16 * LNMX_MAXB + blk] | ((unsigned)sc[(r16 + 16) * LNMX_MAXB + blk] << 8) |
                       ((unsigned)sc[(r16 + 32) * LNMX_MAXB + blk] << 16) |
                       ((unsigned)sc[(r16 + 48) * LNMX_MAXB + blk] << 24);
    *(unsigned*)(scale + mx_a_scale_off(r0 + r16, blk, H >> 7)) = v;
  }
}

// bf16 input: 8 elements (one 16-B load) per lane per 512-element chunk, so a row of 1280 is 3 load
// instructions per lane instead of 5; an MX block of 32 is 4 lanes (DPP quad max); 16-byte fp8 stores (chunk pairs).
SSE_DEV float max4_dpp(float v) {
  v = __builtin_elementwise_maximum(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true)));
  v = __builtin_elementwise_maximum(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true)));
  return v;
}
template <int NC>
__global__ __launch_bounds__(256) void layernorm_mx8_kernel(const bf16* __restrict__ in, const float* __restrict__ w,
                                                            const float* __restrict__ bta, int rows, int H, float eps,
                                                            unsigned char* __restrict__ q,
                                                            unsigned char* __restrict__ scale) {
  __shared__ unsigned char sc[64 * LNMX_MAXB];
  const int r0 = blockIdx.x * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nb = H >> 5;
  const float inv_h = 1.0f / (float)H;
  bf16x8 cur[NC], nxt[NC];
  auto load = [&](bf16x8 (&v)[NC], int row) {
    const bf16* x = in + (long long)(row < rows ? row : rows - 1) * H;
    #pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = 512 * i + 8 * lane;
      v[i] = c < H ? *(const bf16x8*)(x + c) : bf16x8{};
    }
  };
  load(cur, r0 + wave);
  // the LayerNorm weight / bias of the lane's columns, loaded once (per row they were 4x the row's
  // own bytes through L1)
  f32x4 wr[NC][2], br[NC][2];
  #pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = 512 * i + 8 * lane, cc = c < H ? c : 0;
    wr[i][0] = *(const f32x4*)(w + cc);
    wr[i][1] = *(const f32x4*)(w + cc + 4);
    br[i][0] = *(const f32x4*)(bta + cc);
    br[i][1] = *(const f32x4*)(bta + cc + 4);
  }
  for (int rr = wave; rr < 64; rr += 4) {
    const int row = r0 + rr;
    if (row >= rows) break;
    if (rr + 4 < 64) load(nxt, row + 4);
    float s = 0.f;
    #pragma unroll
    for (int i = 0; i < NC; ++i)
      #pragma unroll
      for (int e = 0; e < 8; ++e) s += (float)cur[i][e];
    const float mean = wave_sum_fast(s) * inv_h;
    float qs = 0.f;
    #pragma unroll
    for (int i = 0; i < NC; ++i)
      if (512 * i + 8 * lane < H)
        #pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = (float)cur[i][e] - mean;
          qs = fmaf(d, d, qs);
        }
    const float rstd = 1.0f / sqrtf(wave_sum_fast(qs) * inv_h + eps);
    int xq[NC][2];   // this lane's 8 fp8 bytes of each chunk (stored below, chunk pairs as 16-B stores)
    #pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = 512 * i + 8 * lane;
      const bool ok = c < H;   // wave-uniform per 4-lane block (H % 128 == 0)
      const f32x4 w0 = wr[i][0], w1 = wr[i][1], b0 = br[i][0], b1 = br[i][1];
      float o[8];
      #pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = fmaf(((float)cur[i][e] - mean) * rstd, w0[e], b0[e]);   // = ln_apply4
        o[4 + e] = fmaf(((float)cur[i][4 + e] - mean) * rstd, w1[e], b1[e]);
      }
      float m = 0.f;
      #pragma unroll
      for (int e = 0; e < 8; ++e) m = __builtin_elementwise_maximum(m, fabsf(o[e]));
      const float a = max4_dpp(m);
      const int e8 = mx_scale_exp(a);
      const float inv = mx_inv_scale(e8);
      int x0 = __builtin_amdgcn_cvt_pk_fp8_f32(o[0] * inv, o[1] * inv, 0, false);
      x0 = __builtin_amdgcn_cvt_pk_fp8_f32(o[2] * inv, o[3] * inv, x0, true);
      int x1 = __builtin_amdgcn_cvt_pk_fp8_f32(o[4] * inv, o[5] * inv, 0, false);
      x1 = __builtin_amdgcn_cvt_pk_fp8_f32(o[6] * inv, o[7] * inv, x1, true);
      xq[i][0] = x0;
      xq[i][1] = x1;
      if (ok && (lane & 3) == 0) sc[rr * LNMX_MAXB + (c >> 5)] = (unsigned char)e8;
    }
    // round 6: chunks 2p and 2p + 1 go out as 16-B stores (the per-CU store path costs per instruction): lane pairs
    // (l, l ^ 1) swap pieces by DPP, the even lane stores columns 8l .. 8l + 15 of chunk 2p, the odd one columns
    // 8(l - 1) .. of chunk 2p + 1; an unpaired last chunk keeps its 8-B stores
    const bool odd = lane & 1;
    unsigned char* qrow = q + (long long)row * H;
    #pragma unroll
    for (int i = 0; i + 1 < NC; i += 2) {
      const int s0 = odd ? xq[i][0] : xq[i + 1][0], s1 = odd ? xq[i][1] : xq[i + 1][1];
      const int r0v = __builtin_amdgcn_mov_dpp(s0, 0xB1, 0xF, 0xF, false);   // quad_perm [1, 0, 3, 2]
      const int r1v = __builtin_amdgcn_mov_dpp(s1, 0xB1, 0xF, 0xF, false);
      const int c = odd ? 512 * (i + 1) + 8 * (lane - 1) : 512 * i + 8 * lane;
      const int4 v = odd ? make_int4(r0v, r1v, xq[i + 1][0], xq[i + 1][1]) : make_int4(xq[i][0], xq[i][1], r0v, r1v);
      if (c < H) *(int4*)(qrow + c) = v;
    }
    if constexpr ((NC & 1) != 0) {
      const int c = 512 * (NC - 1) + 8 * lane;
      if (c < H) *(int2*)(qrow + c) = make_int2(xq[NC - 1][0], xq[NC - 1][1]);
    }
    #pragma unroll
    for (int i = 0; i < NC; ++i) cur[i] = nxt[i];
  }
  __syncthreads();
  for (int u = threadIdx.x; u < 16 * nb; u += 256) {
    const int r16 = u & 15, blk = u >> 4;
    if (r0 + r16 >= rows) continue;
    const unsigned v = (unsigned)sc[r16 * LNMX_MAXB + blk] | ((unsigned)sc[(r16 + 16) * LNMX_MAXB + blk] << 8) |
                       ((unsigned)sc[(r16 + 32) * LNMX_MAXB + blk] << 16) |
                       ((unsigned)sc[(r16 + 48) * LNMX_MAXB + blk] << 24);
    *(unsigned*)(scale + mx_a_scale_off(r0 + r16, blk, H >> 7)) = v;
  }
}

template <typename TI>
int launch_layernorm_mx(const TI* in, const float* w, const float* b, int rows, int H, float eps, unsigned char* q,
                        unsigned char* scale, hipStream_t s) {
  if (H % 128 || H > 2048) return -3;
  const dim3 grid((rows + 63) / 64);
  if constexpr (sizeof(TI) == 2) {
    auto go8 = [&](auto ncc) {
      constexpr int NC = decltype(ncc)::value;
      hipLaunchKernelGGL((layernorm_mx8_kernel<NC>), grid, dim3(256), 0, s, in, w, b, rows, H, eps, q, scale);
    };
    switch ((H + 511) / 512) {
      case 1: go8(std::integral_constant<int, 1>{}); break;
      case 2: go8(std::integral_constant<int, 2>{}); break;
      case 3: go8(std::integral_constant<int, 3>{}); break;
      default: go8(std::integral_constant<int, 4>{}); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
  }
  auto go = [&](auto nic) {
    constexpr int NI = decltype(nic)::value;
    hipLaunchKernelGGL((layernorm_mx_kernel<TI, NI>), grid, dim3(256), 0, s, in, w, b, rows, H, eps, q, scale);
  };
  switch ((H + 255) / 256) {   // 16-B pieces per lane
    case 1: go(std::integral_constant<int, 1>{}); break;
    case 2: go(std::integral_constant<int, 2>{}); break;
    case 3: go(std::integral_constant<int, 3>{}); break;
    case 4: go(std::integral_constant<int, 4>{}); break;
    case 5: go(std::integral_constant<int, 5>{}); break;
    case 6: go(std::integral_constant<int, 6>{}); break;
    case 7: go(std::integral_constant<int, 7>{}); break;
    default: go(std::integral_constant<int, 8>{}); break;
  }
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template int launch_layernorm_mx<float>(const float*, const float*, const float*, int, int, float, unsigned char*,
                                        unsigned char*, hipStream_t);
template int launch_layernorm_mx<bf16>(const bf16*, const float*, const float*, int, int, float, unsigned char*,
                                       unsigned char*, hipStream_t);

// ---------------------------------------------------------------------------------------
// MX-fp8 quantisation of a row-major fp32 [R][K] tensor (K % 128 == 0) into e4m3 bytes [R][K]
// and E8M0 scales in the GEMM's A layout (role 0) or B layout (role 1).  One wave per (row,
// 256-column segment), 4 values per lane.
__global__ __launch_bounds__(256) void mx_quantize_kernel(const float* __restrict__ x, int R, int K, int role,
                                                          unsigned char* __restrict__ q,
                                                          unsigned char* __restrict__ scale) {
  const int segs = (K + 255) / 256;
  const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= (long long)R * segs) return;
  const int lane = threadIdx.x & 63;
  const long long row = wid / segs;
  const int c = (int)(wid % segs) * 256 + lane * 4;
  if (c >= K) return;   // whole 8-lane blocks leave together (K % 32 == 0)
  const f32x4 o = *(const f32x4*)(x + row * K + c);
  if (role == 0) {
    mx_quant4(o, q + row * K + c, scale, row, c, K, lane);
  } else {
    const float a = max8_dpp(__builtin_elementwise_maximum(__builtin_elementwise_maximum(fabsf(o[0]), fabsf(o[1])),
                                                               __builtin_elementwise_maximum(fabsf(o[2]), fabsf(o[3]))));
    const int e = mx_scale_exp(a);
    const float inv = mx_inv_scale(e);
    int v = __builtin_amdgcn_cvt_pk_fp8_f32(o[0] * inv, o[1] * inv, 0, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(o[2] * inv, o[3] * inv, v, true);
    *(int*)(q + row * K + c) = v;
    if ((lane & 7) == 0) scale[mx_b_scale_off(row, c >> 5, K >> 7)] = (unsigned char)e;
  }
}

int launch_mx_quantize(const float* x, int R, int K, int role, unsigned char* q, unsigned char* scale, hipStream_t s) {
  if (R <= 0 || K <= 0 || K % 128) return -3;
  const long long waves = (long long)R * ((K + 255) / 256);
  hipLaunchKernelGGL(mx_quantize_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, x, R, K, role, q, scale);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---------------------------------------------------------------------------------------
// K8/K12: out[b*out_stride + n] = mean_t x[b][t][n]  (torch.mean(hs, dim=1), fp64 accumulation).
// Block = (256 columns, clip), POOL_W = 16 waves; lane owns 4 consecutive columns (16-B loads, one
// 1 KiB row piece per wave-instruction), wave w sums frames t = w, w+16, ... with 4 frames' loads in
// flight, then an LDS combine in wave order (4 waves walked ~9 dependent load rounds per 149-frame
// clip: 27 us per launch at B = 128, 7x the HBM time of its bytes).  With per-row LayerNorm statistics (st: (mean, rstd); or lpart: per-256-column
// partials, ln_part_stats), each element is first normalised exactly as layernorm_kernel would have
// written it; the clip's per-frame statistics are formed once into LDS.
constexpr int POOL_TMAX = 1024;   // frames whose statistics fit the LDS table (longer clips: per-frame loads)
constexpr int POOL_W = 16;
template <typename TI>
__global__ __launch_bounds__(64 * POOL_W) void pool_mean_kernel(const TI* __restrict__ x, int T, int H,
                                                        float* __restrict__ out, long long out_stride,
                                                        const float2* __restrict__ st, const float* __restrict__ w,
                                                        const float* __restrict__ bb, const float2* __restrict__ lpart,
                                                        int nt, float eps, const int* __restrict__ tlen) {
  __shared__ double part[POOL_W][256];
  __shared__ float2 fst[POOL_TMAX];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = blockIdx.x * 256 + lane * 4, b = blockIdx.y;
  const int TS = T;   // row stride per clip; T: this clip's frames (ragged batches)
  T = tlen ? tlen[b] : T;
  const bool ln = st || lpart;
  const bool tab = ln && T <= POOL_TMAX;
  if (tab) {
    for (int t = threadIdx.x; t < T; t += 64 * POOL_W)
      fst[t] = st ? st[(long long)b * TS + t] : ln_part_stats(lpart, nt, (long long)b * TS + t, eps);
    __syncthreads();
  }
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (n < H) {
    const TI* xb = x + (long long)b * TS * H + n;
    const f32x4 wn = ln ? *(const f32x4*)(w + n) : f32x4{1.f, 1.f, 1.f, 1.f};
    const f32x4 bn = ln ? *(const f32x4*)(bb + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    auto add = [&](f32x4 v, int t) {
      if (ln) {
        const float2 q = tab ? fst[t] : (st ? st[(long long)b * TS + t] : ln_part_stats(lpart, nt, (long long)b * TS + t, eps));
        #pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf((v[e] - q.x) * q.y, wn[e], bn[e]);
      }
      s0 += v[0];
      s1 += v[1];
      s2 += v[2];
      s3 += v[3];
    };
    int t = wv;
    constexpr int W = POOL_W;
    for (; t + 3 * W < T; t += 4 * W) {   // 4 frames of this wave in flight
      const f32x4 v0 = load4<TI>(xb + (long long)t * H), v1 = load4<TI>(xb + (long long)(t + W) * H);
      const f32x4 v2 = load4<TI>(xb + (long long)(t + 2 * W) * H), v3 = load4<TI>(xb + (long long)(t + 3 * W) * H);
      add(v0, t);
      add(v1, t + W);
      add(v2, t + 2 * W);
      add(v3, t + 3 * W);
    }
    for (; t < T; t += W) add(load4<TI>(xb + (long long)t * H), t);
  }
  part[wv][lane * 4 + 0] = s0;
  part[wv][lane * 4 + 1] = s1;
  part[wv][lane * 4 + 2] = s2;
  part[wv][lane * 4 + 3] = s3;
  __syncthreads();
  const int c = threadIdx.x, nc = blockIdx.x * 256 + c;
  // a clip with no frames (ragged batch, shorter than the receptive field) pools to zeros, never
  // 0/0; the host wrapper rejects such clips before the call (SSEModel.embed)
  if (c < 256 && nc < H) {
    double v = part[0][c];
    #pragma unroll
    for (int k = 1; k < POOL_W; ++k) v += part[k][c];
    out[b * out_stride + nc] = T > 0 ? (float)(v / T) : 0.f;
  }
}

template <typename TI>
int launch_pool_mean(const TI* x, int B, int T, int H, float* out, long long out_stride, hipStream_t s,
                     const float2* st, const float* w, const float* b, const float2* part, int nt, float eps,
                     const int* tlen) {
  if (H % 4) return -3;
  hipLaunchKernelGGL(pool_mean_kernel<TI>, dim3((H + 255) / 256, B), dim3(64 * POOL_W), 0, s, x, T, H, out, out_stride, st, w,
                     b, part, nt, eps, tlen);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template int launch_pool_mean<float>(const float*, int, int, int, float*, long long, hipStream_t, const float2*,
                                     const float*, const float*, const float2*, int, float, const int*);
template int launch_pool_mean<bf16>(const bf16*, int, int, int, float*, long long, hipStream_t, const float2*,
                                    const float*, const float*, const float2*, int, float, const int*);
template int launch_pool_mean<f16>(const f16*, int, int, int, float*, long long, hipStream_t, const float2*,
                                   const float*, const float*, const float2*, int, float, const int*);

// ---------------------------------------------------------------------------------------
// Statistics / windowed pooling: mean, std (torch.std(hs, dim=1), correction ddof) and max of one hidden
// state, over the whole clip or over windows of win frames every hop frames (win % hop == 0).  A kernel of
// its own: pool_mean_kernel and the default embedding path stay as they are.
// Block = (256 columns, clip), POOL_SW = 8 waves, lane = 4 consecutive columns (16-B loads, 4 frames of a wave
// in flight) and the same element normalisation as pool_mean_kernel.  Every frame's (sum, sum of squares) go to
// fp64 accumulators, the maximum to fp32.  The unit of work of a wave is a task; its partial (sum, sumsq, max per
// column, 5 KiB for 256 columns) goes to one of POOL_SW LDS slots (40 KiB for the three tables + 8 KiB of
// LayerNorm statistics: three blocks fit a CU's 160 KiB, and a block still fits beside the GEMM workgroups of
// the other half-batch's stream.  16 waves / 88 KiB measured 17.0 us against 14.1 us per launch at B = 256):
//   one segment (win = 0, or the clip no longer than win): task w = frames w, w + POOL_SW, ... (the mean
//     kernel's interleave); the segment combines the POOL_SW slots in wave order.
//   R = win / hop <= POOL_SW: task k = hop-chunk k, frames [k hop, (k+1) hop); the slots are a ring of chunk
//     partials, segment s combines chunks s .. s + R - 1 in order once the last of them is in.  The first
//     round fills the ring, each later one replaces the POOL_SW - (R - 1) chunks no open segment needs, so
//     each element is read once whatever the overlap, and the LDS does not grow with T / hop (T = 1500 at
//     hop = 1 is 1500 chunks walked through 8 slots).
//   R > POOL_SW (a window of more than 8 hops): R chunk partials of 256 columns do not fit the slots, so
//     task k is segment k itself, frames [k hop, k hop + win): rows are then loaded by up to R tasks of the
//     same block, back to back (cache hits after the first), not once.
// The order of every sum depends only on the clip's own frame count and (win, hop): a clip pools to the same
// bits alone and inside a ragged batch.  tlen is clamped to [0, TS]; no frame at or past it is read.
constexpr int POOL_SW = 8;   // waves (and LDS slots) of pool_stats_kernel
template <typename TI>
__global__ __launch_bounds__(64 * POOL_SW) void pool_stats_kernel(const TI* __restrict__ x, int TS, int H,
                                                         float* __restrict__ out, long long stride_b,
                                                         long long stride_s, int nseg, PoolDesc d,
                                                         const float2* __restrict__ st, const float* __restrict__ w,
                                                         const float* __restrict__ bb, const float2* __restrict__ lpart,
                                                         int nt, float eps, const int* __restrict__ tlen) {
  __shared__ double psum[POOL_SW][256];
  __shared__ double psq[POOL_SW][256];
  __shared__ float pmax[POOL_SW][256];
  __shared__ float2 fst[POOL_TMAX];
  constexpr int W = POOL_SW, NQ = W / 4;   // NQ segments emitted side by side
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = blockIdx.x * 256 + lane * 4, b = blockIdx.y;
  const int T = tlen ? min(max(tlen[b], 0), TS) : TS;   // this clip's frames; TS: row stride per clip
  const bool ln = st || lpart;
  const bool tab = ln && T <= POOL_TMAX;
  if (tab) {
    for (int t = threadIdx.x; t < T; t += 64 * W)
      fst[t] = st ? st[(long long)b * TS + t] : ln_part_stats(lpart, nt, (long long)b * TS + t, eps);
    __syncthreads();
  }
  const TI* xb = x + (long long)b * TS * H + n;
  const f32x4 wn = ln && n < H ? *(const f32x4*)(w + n) : f32x4{1.f, 1.f, 1.f, 1.f};
  const f32x4 bn = ln && n < H ? *(const f32x4*)(bb + n) : f32x4{0.f, 0.f, 0.f, 0.f};
  // frames t, t + step, ... < end of this wave's task -> slot
  auto run_task = [&](int t, int step, int end, int slot) {
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q2[4] = {0.0, 0.0, 0.0, 0.0};
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    auto add = [&](f32x4 v, int tt) {
      if (ln) {
        const float2 q = tab ? fst[tt] : (st ? st[(long long)b * TS + tt] : ln_part_stats(lpart, nt, (long long)b * TS + tt, eps));
        #pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf((v[e] - q.x) * q.y, wn[e], bn[e]);
      }
      #pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double dv = (double)v[e];
        s[e] += dv;
        q2[e] = fma(dv, dv, q2[e]);
        mx[e] = fmaxf(mx[e], v[e]);
      }
    };
    if (n < H) {
      for (; t + 3 * step < end; t += 4 * step) {   // 4 frames of this wave in flight
        const f32x4 v0 = load4<TI>(xb + (long long)t * H), v1 = load4<TI>(xb + (long long)(t + step) * H);
        const f32x4 v2 = load4<TI>(xb + (long long)(t + 2 * step) * H), v3 = load4<TI>(xb + (long long)(t + 3 * step) * H);
        add(v0, t);
        add(v1, t + step);
        add(v2, t + 2 * step);
        add(v3, t + 3 * step);
      }
      for (; t < end; t += step) add(load4<TI>(xb + (long long)t * H), t);
    }
    #pragma unroll
    for (int e = 0; e < 4; ++e) {
      psum[slot][lane * 4 + e] = s[e];
      psq[slot][lane * 4 + e] = q2[e];
      pmax[slot][lane * 4 + e] = mx[e];
    }
  };
  // thread (c, q): column c of segments q, q + NQ, ...
  const int c = threadIdx.x & 255, q = threadIdx.x >> 8, nc = blockIdx.x * 256 + c;
  const int nst = ((d.stats & POOL_MEAN) ? 1 : 0) + ((d.stats & POOL_STD) ? 1 : 0) + ((d.stats & POOL_MAX) ? 1 : 0);
  float* ob = out + (long long)b * stride_b + nc;
  // segment sg of cnt frames = slots slot0, slot0 + 1, ... (ns of them, ring order)
  auto emit = [&](int sg, int slot0, int ns, int cnt) {
    double s = 0.0, q2 = 0.0;
    float mx = -INFINITY;
    for (int j = 0; j < ns; ++j) {
      const int sl = (slot0 + j) & (W - 1);
      s += psum[sl][c];
      q2 += psq[sl][c];
      mx = fmaxf(mx, pmax[sl][c]);
    }
    float* o = ob + (long long)sg * stride_s;
    if (d.stats & POOL_MEAN) { *o = (float)(s / cnt); o += H; }
    if (d.stats & POOL_STD) {
      const int dof = cnt - d.ddof;
      const double var = dof > 0 ? (q2 - s * s / cnt) / dof : 0.0;
      *o = var > 0.0 ? (float)sqrt(var) : 0.f;
      o += H;
    }
    if (d.stats & POOL_MAX) *o = mx;
  };
  static_assert((W & (W - 1)) == 0, "ring index");
  int S = 0;   // segments of this clip
  if (T > 0) S = (d.win == 0 || T <= d.win) ? 1 : 1 + (T - d.win + d.hop - 1) / d.hop;
  if (S == 1) {
    run_task(wv, W, T, wv);
    __syncthreads();
    if (q == 0 && nc < H) emit(0, 0, W, T);
  } else if (S > 1) {
    const int R = d.win / d.hop;
    const bool direct = R > W;            // a task is a whole segment
    const int Rr = direct ? 1 : R;        // slots per segment
    const int len = direct ? d.win : d.hop;
    const int ntask = S + Rr - 1;         // = ceil(T / hop) chunks, or S segments
    int done = 0;                          // tasks in the ring so far
    int emitted = 0;
    for (int cnt = W; done < ntask; cnt = W - (Rr - 1)) {
      const int k = done + wv;
      if (wv < cnt && k < ntask) {
        const long long t0 = (long long)k * d.hop;
        run_task((int)t0, 1, (int)(t0 + len < T ? t0 + len : T), k & (W - 1));
      }
      done = done + cnt < ntask ? done + cnt : ntask;
      __syncthreads();
      const int upto = done - Rr + 1;     // segments whose last chunk is in
      if (nc < H)
        for (int sg = emitted + q; sg < upto; sg += NQ) {
          const long long t0 = (long long)sg * d.hop;
          emit(sg, sg & (W - 1), Rr, (int)((t0 + d.win < T ? t0 + d.win : T) - t0));
        }
      emitted = upto > emitted ? upto : emitted;
      __syncthreads();
    }
  }
  // slots past this clip's segments (ragged batch; every slot of a clip with no frames): zeros
  if (nc < H)
    for (int sg = S + q; sg < nseg; sg += NQ) {
      float* o = ob + (long long)sg * stride_s;
      for (int k = 0; k < nst; ++k) o[(long long)k * H] = 0.f;
    }
}

int pool_segments(int T, int win, int hop) {
  if (T < 0 || win < 0 || (win > 0 && (hop <= 0 || win % hop))) return -1;
  if (win == 0 || T <= win) return 1;
  return 1 + (T - win + hop - 1) / hop;
}

template <typename TI>
int launch_pool_stats(const TI* x, int B, int T, int H, float* out, long long stride_b, long long stride_s, int nseg,
                      PoolDesc d, hipStream_t s, const float2* st, const float* w, const float* b, const float2* part,
                      int nt, float eps, const int* tlen) {
  if (H % 4 || B <= 0 || T <= 0) return -3;
  if (!(d.stats & 7) || (d.stats & ~7) || d.ddof < 0 || d.ddof > 1 || nseg != pool_segments(T, d.win, d.hop)) return -3;
  hipLaunchKernelGGL(pool_stats_kernel<TI>, dim3((H + 255) / 256, B), dim3(64 * POOL_SW), 0, s, x, T, H, out, stride_b,
                     stride_s, nseg, d, st, w, b, part, nt, eps, tlen);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template int launch_pool_stats<float>(const float*, int, int, int, float*, long long, long long, int, PoolDesc,
                                      hipStream_t, const float2*, const float*, const float*, const float2*, int,
                                      float, const int*);
template int launch_pool_stats<bf16>(const bf16*, int, int, int, float*, long long, long long, int, PoolDesc,
                                     hipStream_t, const float2*, const float*, const float*, const float2*, int, float,
                                     const int*);
template int launch_pool_stats<f16>(const f16*, int, int, int, float*, long long, long long, int, PoolDesc,
                                    hipStream_t, const float2*, const float*, const float*, const float2*, int, float,
                                    const int*);

// Whisper valid-frame pooling (the twin of clip_frames_kernel): encoder frames that cover real audio, one per
// two 160-sample mel hops; the sample count is clamped to [0, L] as there, the result to the encoder's Tq.
__global__ void whisper_frames_kernel(const int* __restrict__ lens, int B, int L, int Tq, int* __restrict__ tq) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int len = lens ? min(max(lens[b], 0), L) : L;
  tq[b] = min(Tq, (len + 319) / 320);
}

int launch_whisper_frames(const int* lens, int B, int L, int Tq, int* tq, hipStream_t s) {
  hipLaunchKernelGGL(whisper_frames_kernel, dim3((B + 255) / 256), dim3(256), 0, s, lens, B, L, Tq, tq);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---------------------------------------------------------------------------------------
// Ragged batches: per-clip frame counts after conv0 and after the last conv layer (the same
// integer recurrence as wavlm_frames on the host); 0 for a clip shorter than the receptive field.
// The sample count is clamped to [0, L] (L = the batch's row length) on the device, so no length
// the caller passes makes a later kernel read past its clip's rows: the recurrence is monotone, so
// t0 <= T0 and tf <= Tf of the padded batch.
__global__ void clip_frames_kernel(const int* __restrict__ lens, int B, int L, ClipFrames cf, int* __restrict__ t0,
                                   int* __restrict__ tf) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int t = min(max(lens[b], 0), L), f0 = 0;
  for (int i = 0; i < cf.n_conv; ++i) {
    t = t < cf.kernel[i] ? 0 : (t - cf.kernel[i]) / cf.stride[i] + 1;
    if (i == 0) f0 = t;
  }
  t0[b] = f0;
  tf[b] = t;
}

int launch_clip_frames(const int* lens, int B, int L, ClipFrames cf, int* t0, int* tf, hipStream_t s) {
  hipLaunchKernelGGL(clip_frames_kernel, dim3((B + 255) / 256), dim3(256), 0, s, lens, B, L, cf, t0, tf);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// Range flag of the fp16-range dtypes (sse_check_range): *flag = 1 if any of x[0, n) is non-finite.
// Grid-stride over 16-B groups; every thread that sees a non-finite value stores 1 (a plain vector
// store: all writers write the same value).
__global__ __launch_bounds__(256) void finite_flag_kernel(const float* __restrict__ x, long long n, int* flag) {
  const long long n4 = n >> 2;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const f32x4 v = *(const f32x4*)(x + 4 * i);
    bad |= !(__builtin_isfinite(v[0]) && __builtin_isfinite(v[1]) && __builtin_isfinite(v[2]) &&
             __builtin_isfinite(v[3]));
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) bad |= !__builtin_isfinite(x[4 * n4 + threadIdx.x]);
  if (bad) *flag = 1;
}

int launch_finite_flag(const float* x, long long n, int* flag, hipStream_t s) {
  if (n <= 0) return 0;
  long long nb = ((n >> 2) + 255) / 256;
  nb = nb < 1 ? 1 : (nb > 2048 ? 2048 : nb);
  hipLaunchKernelGGL(finite_flag_kernel, dim3((unsigned)nb), dim3(256), 0, s, x, n, flag);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <typename TE>
__global__ __launch_bounds__(256) void mask_rows_kernel(TE* __restrict__ x, int T, int H, const int* __restrict__ tlen) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T || t < tlen[b]) return;
  TE* row = x + ((long long)b * T + t) * H;
  for (int c = (threadIdx.x & 63); c < H; c += 64) row[c] = (TE)0.f;
}

template <typename TE>
int launch_mask_rows(TE* x, int B, int T, int H, const int* tlen, hipStream_t s) {
  hipLaunchKernelGGL(mask_rows_kernel<TE>, dim3((T + 3) / 4, B), dim3(256), 0, s, x, T, H, tlen);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template int launch_mask_rows<float>(float*, int, int, int, const int*, hipStream_t);
template int launch_mask_rows<bf16>(bf16*, int, int, int, const int*, hipStream_t);
template int launch_mask_rows<f16>(f16*, int, int, int, const int*, hipStream_t);

// ---------------------------------------------------------------------------------------
// K5/K6/K11: attention, flash style.  Block = (64 queries, head, clip), 4 waves x 16 queries.
// Keys stream through LDS in tiles of 64.  Per tile and wave:
//   S^T = K_tile . Q^T      (key on the MFMA row, query on the lane: lane holds one query)
//   s   = S^T*scale (+ gate[q] * relbias[key - q])   -- WavLM gated relative-position bias
//   online softmax over keys (max/sum in-lane + 2 cross-lane-group shuffles)
//   O^T += V^T_tile . P^T   (the S^T accumulators ARE the B operand, no lane movement)
// bf16 path: v_mfma_f32_16x16x32_bf16 on K [key][d] (128-B rows, XOR swizzle) and V^T
// [d][key]; f32 path: v_mfma_f32_16x16x4_f32 on K [key][d] (256-B rows, XOR swizzle) and
// V [key][d] (68-float rows).  HF: modeling_wavlm.py:141-241, modeling_whisper.py:215-238.
constexpr int AT_Q = 64, AT_K = 64, AT_HD = 64;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
constexpr int VT_STRIDE = 72;     // bf16 V^T row stride (36 dwords = 16k+4: conflict-free b64 reads)
constexpr int VF_STRIDE = 68;     // f32 V row stride (4 mod 8: conflict-free b32 reads)



// XCD-aware block order for the (query block, head, clip) grids: workgroup i runs on XCD i % 8
// (each XCD has its own L2), so the linear id is remapped bijectively to make consecutive ids share
// an XCD; the query blocks of one (clip, head) are then consecutive and read their K/V tiles from one
// L2 instead of up to 8 (PMC: 8.9 GB of HBM traffic per Whisper launch at B = 128 without it, for
// ~2 GB of unique bytes).
SSE_DEV void attn_block_xcd(int& qc, int& h, int& b) {
  const int nwg = gridDim.x * gridDim.y * gridDim.z;
  const int id = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const int q8 = nwg / 8, r8 = nwg % 8, x = id % 8;
  const int lid = (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + id / 8;
  qc = lid % gridDim.x;
  h = (lid / gridDim.x) % gridDim.y;
  b = lid / (gridDim.x * gridDim.y);
}

template <typename TE>
SSE_DEV float wavlm_gate(const TE* rp, float c) {
  float v[8];
  if constexpr (sizeof(TE) == 2) {
    const bf16x8 r = *(const bf16x8*)rp;
    #pragma unroll
    for (int o = 0; o < 8; ++o) v[o] = (float)r[o];
  } else {
    const f32x4 r0 = *(const f32x4*)rp, r1 = *(const f32x4*)(rp + 4);
    #pragma unroll
    for (int o = 0; o < 4; ++o) { v[o] = r0[o]; v[4 + o] = r1[o]; }
  }
  const float ra = v[0] + v[1] + v[2] + v[3], rb = v[4] + v[5] + v[6] + v[7];
  const float ga = 1.f / (1.f + expf(-ra)), gb = 1.f / (1.f + expf(-rb));
  return ga * (gb * c - 1.0f) + 2.0f;
}

template <bool H16 = false>   // H16: the 8 projections are fp16 (SSE_DTYPE_FP16) in a bf16x8 container
SSE_DEV float wavlm_gate_v(const bf16x8& r, float c) {
  const float ra = hval<H16>(r[0]) + hval<H16>(r[1]) + hval<H16>(r[2]) + hval<H16>(r[3]);
  const float rb = hval<H16>(r[4]) + hval<H16>(r[5]) + hval<H16>(r[6]) + hval<H16>(r[7]);
  const float ga = 1.f / (1.f + expf(-ra)), gb = 1.f / (1.f + expf(-rb));
  return ga * (gb * c - 1.0f) + 2.0f;
}
// wavlm_gate_v for the 16 rows of a wave whose 4 lane groups hold the same row (attn_head_body): each lane
// pair of groups (0, 1) / (2, 3) evaluates one of the two sigmoids and swaps it with its partner
// (v_permlane16_swap: result 0 = the even group's value, 1 = the odd group's), one exp + one divide per
// lane instead of two; bit-identical to wavlm_gate_v
template <bool H16 = false>
SSE_DEV float wavlm_gate_pair(const bf16x8& r, float c, int g) {
  const float ra = hval<H16>(r[0]) + hval<H16>(r[1]) + hval<H16>(r[2]) + hval<H16>(r[3]);
  const float rb = hval<H16>(r[4]) + hval<H16>(r[5]) + hval<H16>(r[6]) + hval<H16>(r[7]);
  const float x = (g & 1) ? rb : ra;
  const float sg = 1.f / (1.f + expf(-x));
  const auto t = __builtin_amdgcn_permlane16_swap(__float_as_uint(sg), __float_as_uint(sg), false, false);
  const float ga = __uint_as_float(t[0]), gb = __uint_as_float(t[1]);
  return ga * (gb * c - 1.0f) + 2.0f;
}

// X3 (split-fp16 path, TE = float, a.out3): fp32 q/k/v from the QKV GEMM, split while loaded / staged
// (x3_split4) into hi and lo' 2^-11 planes, and both products on the f16 matrix cores with the bf16
// form's fragment layout: S = qh.kh + 2^-11 (qh.kl' + ql'.kh), O = ph.vh + 2^-11 (ph.vl' + pl'.vh), the
// 2^-11 terms in their own accumulators (the dropped lo.lo' is ~2^-22 relative); the softmax in fp32.
// The exact-f32 form (16x16x4 f32 MFMAs, scalar V reads) ran at ~30 TF/s.
template <typename TE, bool BIAS, bool X3 = false>
__global__ __launch_bounds__(256) void attention_kernel(AttnArgs a) {
  constexpr bool BF = sizeof(TE) == 2;
  static_assert(!(BF && X3), "X3: fp32 q/k/v");
  constexpr int KS_BYTES = X3 ? 2 * AT_K * 128 : BF ? AT_K * 128 : AT_K * 256;
  constexpr int VS_BYTES = X3 ? 2 * AT_K * 128 : BF ? AT_HD * VT_STRIDE * 2 : AT_K * VF_STRIDE * 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + KS_BYTES;
  float* gate = (float*)(Vs + VS_BYTES);           // [AT_Q]
  float* rb = gate + AT_Q;                         // [2*Tk]  (BIAS)

  int qc, h, b;
  attn_block_xcd(qc, h, b);
  // T: this clip's frames (ragged batches: a.tlen), TS: the batch's row stride per clip
  const int TS = a.T, T = a.tlen ? a.tlen[b] : a.T, H = a.H, H3 = a.ldq;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r16 = lane & 15;
  const int q0 = qc * AT_Q;
  const int nkt = (T + AT_K - 1) / AT_K;
  const int Tk = nkt * AT_K;
  const TE* qkv = (const TE*)a.qkv + (long long)b * TS * H3;

  if (BIAS) {
    // gate[q] = sigmoid(a) * (sigmoid(b) * const_h - 1) + 2 with a, b the pairwise sums of the
    // 8 gru_rel_pos_linear outputs the QKV GEMM produced (HF modeling_wavlm.py:158-170)
    if (tid < AT_Q) {
      float gv = 0.f;
      if (q0 + tid < T) gv = wavlm_gate(qkv + (long long)(q0 + tid) * a.ldq + 3 * H + 8 * h, a.gconst[h]);
      gate[tid] = gv;
    }
    // relative bias slice: rb[u] = relb[h][u - (Tk-1)], u in [0, 2*Tk-1)
    const float* rh = a.relb + (long long)h * (2 * a.maxd + 1) + a.maxd;
    for (int u = tid; u < 2 * Tk - 1; u += 256) {
      int d = u - (Tk - 1);
      d = d < -a.maxd ? -a.maxd : (d > a.maxd ? a.maxd : d);
      rb[u] = rh[d];
    }
  }

  // Q fragments (B operand of S^T = K.Q^T), straight from global.
  const int qi = q0 + wave * 16 + r16;
  const bool qv = qi < T;
  const TE* qrow = qkv + (long long)(qv ? qi : 0) * H3 + h * AT_HD;
  bf16x8 qb[2];
  f32x4 qf[4];
  f16x8 qh[2], ql[2];
  if constexpr (X3) {
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      f32x4 v0 = *(const f32x4*)((const float*)qrow + ks * 32 + g * 8), v1 = *(const f32x4*)((const float*)qrow + ks * 32 + g * 8 + 4);
      if (!qv) v0 = v1 = f32x4{0.f, 0.f, 0.f, 0.f};
      f16x4 h0, l0, h1, l1;
      x3_split4(v0, h0, l0);
      x3_split4(v1, h1, l1);
      qh[ks] = f16x8{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
      ql[ks] = f16x8{l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
    }
  } else if constexpr (BF) {
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qb[ks] = *(const bf16x8*)(qrow + ks * 32 + g * 8);
      if (!qv) qb[ks] = bf16x8{};
    }
  } else {
    #pragma unroll
    for (int c = 0; c < 4; ++c) {
      qf[c] = *(const f32x4*)((const float*)qrow + (g + 4 * c) * 4);
      if (!qv) qf[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }

  f32x4 o[4], o2[4];   // o2: the 2^-11 terms (X3)
  #pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = o2[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const float LOG2E = 1.4426950408889634f;

  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();   // previous tile fully consumed
    // ---- stage K (swizzled rows) and V (transposed for bf16) ----
    const int kbase = kt * AT_K;
    if constexpr (X3) {
      for (int i = tid; i < AT_K * 8; i += 256) {
        const int kr = i >> 3, ch = i & 7;
        const int key = kbase + kr;
        f32x4 k0 = f32x4{0.f, 0.f, 0.f, 0.f}, k1 = k0, v0 = k0, v1 = k0;
        if (key < T) {
          const float* kp = (const float*)(qkv + (long long)key * H3 + H + h * AT_HD) + ch * 8;
          const float* vp = (const float*)(qkv + (long long)key * H3 + 2 * H + h * AT_HD) + ch * 8;
          k0 = *(const f32x4*)kp; k1 = *(const f32x4*)(kp + 4);
          v0 = *(const f32x4*)vp; v1 = *(const f32x4*)(vp + 4);
        }
        f16x4 h0, l0, h1, l1;
        x3_split4(k0, h0, l0);
        x3_split4(k1, h1, l1);
        char* kd = Ks + kr * 128 + ((ch ^ ((kr >> 1) & 7)) * 16);
        *(f16x8*)kd = f16x8{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
        *(f16x8*)(kd + AT_K * 128) = f16x8{l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
        x3_split4(v0, h0, l0);
        x3_split4(v1, h1, l1);
        // V row-major (128-B rows, 16-B chunks XOR 2 ((row >> 1) & 3)), read transposed by
        // ds_read_b64_tr_b16 (attention_full_kernel's layout)
        char* vd = Vs + kr * 128 + ((ch ^ (((kr >> 1) & 3) << 1)) << 4);
        *(f16x8*)vd = f16x8{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
        *(f16x8*)(vd + AT_K * 128) = f16x8{l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
      }
    } else if constexpr (BF) {
      for (int i = tid; i < AT_K * 8; i += 256) {
        const int kr = i >> 3, ch = i & 7;
        const int key = kbase + kr;
        bf16x8 kv = bf16x8{}, vv = bf16x8{};
        if (key < T) {
          kv = *(const bf16x8*)(qkv + (long long)key * H3 + H + h * AT_HD + ch * 8);
          vv = *(const bf16x8*)(qkv + (long long)key * H3 + 2 * H + h * AT_HD + ch * 8);
        }
        *(bf16x8*)(Ks + kr * 128 + ((ch ^ ((kr >> 1) & 7)) * 16)) = kv;
        bf16* vt = (bf16*)Vs;
        #pragma unroll
        for (int e = 0; e < 8; ++e) vt[(ch * 8 + e) * VT_STRIDE + kr] = vv[e];
      }
    } else {
      for (int i = tid; i < AT_K * 16; i += 256) {
        const int kr = i >> 4, ch = i & 15;
        const int key = kbase + kr;
        f32x4 kv = f32x4{0.f, 0.f, 0.f, 0.f}, vv = kv;
        if (key < T) {
          kv = *(const f32x4*)((const float*)(qkv + (long long)key * H3 + H + h * AT_HD) + ch * 4);
          vv = *(const f32x4*)((const float*)(qkv + (long long)key * H3 + 2 * H + h * AT_HD) + ch * 4);
        }
        *(f32x4*)(Ks + kr * 256 + ((ch ^ (kr & 15)) * 16)) = kv;
        *(f32x4*)((float*)Vs + kr * VF_STRIDE + ch * 4) = vv;
      }
    }
    __syncthreads();

    // ---- S^T tiles: s[kb][r] = score(key = kbase + kb*16 + 4g + r, query = qi) ----
    f32x4 s[4];
    #pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
      const int kr = kb * 16 + r16;
      if constexpr (X3) {
        f32x4 acc2 = f32x4{0.f, 0.f, 0.f, 0.f};
        #pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const char* kp = Ks + kr * 128 + (((g + 4 * ks) ^ ((kr >> 1) & 7)) * 16);
          const f16x8 kh = *(const f16x8*)kp, kl = *(const f16x8*)(kp + AT_K * 128);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, qh[ks], acc, 0, 0, 0);
          acc2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl, qh[ks], acc2, 0, 0, 0);
          acc2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, ql[ks], acc2, 0, 0, 0);
        }
        #pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(acc2[e], 1.f / X3_LO_SCALE, acc[e]);
      } else if constexpr (BF) {
        #pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bf16x8 kf = *(const bf16x8*)(Ks + kr * 128 + (((g + 4 * ks) ^ ((kr >> 1) & 7)) * 16));
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qb[ks], acc, 0, 0, 0);
        }
      } else {
        #pragma unroll
        for (int c = 0; c < 4; ++c) {
          const f32x4 kf = *(const f32x4*)(Ks + kr * 256 + (((g + 4 * c) ^ (kr & 15)) * 16));
          #pragma unroll
          for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[e], qf[c][e], acc, 0, 0, 0);
        }
      }
      s[kb] = acc;
    }
    // ---- scale, bias, mask; online softmax ----
    float tmax = -INFINITY;
    #pragma unroll
    for (int kb = 0; kb < 4; ++kb)
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kbase + kb * 16 + 4 * g + r;
        float v = s[kb][r] * a.scale;
        if (BIAS) v = fmaf(gate[wave * 16 + r16], rb[key - qi + (Tk - 1)], v);
        v = key < T ? v : -INFINITY;
        s[kb][r] = v;
        tmax = __builtin_elementwise_maximum(tmax, v);
      }
    tmax = __builtin_elementwise_maximum(tmax, __shfl_xor(tmax, 16, 64));
    tmax = __builtin_elementwise_maximum(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = __builtin_elementwise_maximum(m_run, tmax);
    const float alpha = exp2f((m_run - m_new) * LOG2E);
    m_run = m_new;
    l_run *= alpha;
    #pragma unroll
    for (int i = 0; i < 4; ++i) o[i] *= alpha;
    if constexpr (X3) {
      #pragma unroll
      for (int i = 0; i < 4; ++i) o2[i] *= alpha;
    }
    const float mb = m_new * LOG2E;
    #pragma unroll
    for (int kb = 0; kb < 4; ++kb)
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = exp2f(fmaf(s[kb][r], LOG2E, -mb));
        s[kb][r] = p;
        l_run += p;
      }
    // ---- O^T += V^T . P^T ----
    if constexpr (X3) {
      const int rowv = 4 * g + (r16 >> 2), swv = ((rowv >> 1) & 3) << 1;
      #pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        f16x4 h0, l0, h1, l1;
        x3_split4(s[2 * ks], h0, l0);
        x3_split4(s[2 * ks + 1], h1, l1);
        const f16x8 ph = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
        const f16x8 pl = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
        #pragma unroll
        for (int db = 0; db < 4; ++db) {
          const char* va = Vs + ks * 4096 + rowv * 128 + (((2 * db + ((r16 & 3) >> 1)) ^ swv) << 4) + 8 * (r16 & 1);
          const bf16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)va);
          const bf16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(va + 2048));
          const bf16x4 c0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(va + AT_K * 128));
          const bf16x4 c1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(va + AT_K * 128 + 2048));
          const f16x8 vh = __builtin_bit_cast(f16x8, bf16x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]});
          const f16x8 vl = __builtin_bit_cast(f16x8, bf16x8{c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]});
          o[db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph, o[db], 0, 0, 0);
          o2[db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph, o2[db], 0, 0, 0);
          o2[db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl, o2[db], 0, 0, 0);
        }
      }
    } else if constexpr (BF) {
      const bf16* vt = (const bf16*)Vs;
      #pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 pf;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          pf[r] = (bf16)s[2 * ks][r];
          pf[4 + r] = (bf16)s[2 * ks + 1][r];
        }
        #pragma unroll
        for (int db = 0; db < 4; ++db) {
          const bf16* vrow = vt + (db * 16 + r16) * VT_STRIDE + ks * 32 + 4 * g;
          const bf16x4 v0 = *(const bf16x4*)(vrow);
          const bf16x4 v1 = *(const bf16x4*)(vrow + 16);
          const bf16x8 vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
          o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[db], 0, 0, 0);
        }
      }
    } else {
      const float* vs = (const float*)Vs;
      #pragma unroll
      for (int kb = 0; kb < 4; ++kb)
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float* vrow = vs + (kb * 16 + 4 * g + r) * VF_STRIDE + r16;
          #pragma unroll
          for (int db = 0; db < 4; ++db)
            o[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(vrow[db * 16], s[kb][r], o[db], 0, 0, 0);
        }
    }
  }
  // ---- normalise and store: lane holds O[query qi][dims db*16 + 4g .. +3] ----
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  if (!qv) return;
  const float inv = 1.0f / l_run;
  if constexpr (X3) {
    #pragma unroll
    for (int db = 0; db < 4; ++db)
      #pragma unroll
      for (int e = 0; e < 4; ++e) o[db][e] = fmaf(o2[db][e], 1.f / X3_LO_SCALE, o[db][e]);
  }
  TE* orow = (TE*)a.out + ((long long)b * TS + qi) * H + h * AT_HD;
  #pragma unroll
  for (int db = 0; db < 4; ++db) {
    if constexpr (BF) {
      bf16x4 ov = {(bf16)(o[db][0] * inv), (bf16)(o[db][1] * inv), (bf16)(o[db][2] * inv), (bf16)(o[db][3] * inv)};
      *(bf16x4*)(orow + db * 16 + 4 * g) = ov;
    } else if (a.out3) {   // the out-projection's split-fp16 operand row [hi | lo' | hi] directly
      f16x4 hi, lo;
      x3_split4(o[db] * inv, hi, lo);
      f16* o3 = (f16*)a.out + ((long long)b * TS + qi) * 3 * H + h * AT_HD + db * 16 + 4 * g;
      *(f16x4*)o3 = hi;
      *(f16x4*)(o3 + H) = lo;
      *(f16x4*)(o3 + 2 * H) = hi;
    } else {
      *(f32x4*)((float*)orow + db * 16 + 4 * g) = o[db] * inv;
    }
  }
}

// Short-sequence variant (T <= 256, WavLM clips up to ~5 s): one block per (head, clip),
// K and V staged into LDS ONCE and shared by all query blocks; each wave owns query blocks of
// 16 and keeps the whole score row (NKB 16-key blocks) in registers: exact softmax, no
// online rescaling.  Keys are padded to a multiple of 32 (not 64): at T = 149, 160 keys.
// Long-sequence bf16 variant (Whisper T = 1500, WavLM clips > 160 frames): block = 128 queries
// of one (head, clip) = 4 waves x 32 queries (two 16-query MFMA blocks per wave, so every K and
// V fragment read from LDS feeds two MFMAs).  K/V tiles of 64 keys are double-buffered: the
// next tile's global loads are issued into registers before the current tile's MFMAs and
// written to the other LDS buffer after them — one barrier per tile.
constexpr int F2_QPW = 32, F2_Q = 128, F2_K = 64;
constexpr float F2_TH = 8.0f;   // no-bias flash kernel: running-max slack (log2 units) before an O / l rescale
// V is staged row-major ([key][64 dims], 160-B rows) and read transposed by ds_read_b64_tr_b16:
// the 8 key rows x 32 B one half-wave touches land on 8 disjoint 8-bank ranges at a 40-dword stride
constexpr int VR_STRIDE = 160;
constexpr int F2_KS = F2_K * 128, F2_VS = F2_K * VR_STRIDE, F2_BUF = F2_KS + F2_VS;

// A operand of O^T += V^T . P^T for 32 keys from row-major V in LDS: lane (g, r16) gets dim
// d0 + r16 of keys k0 + 4g + 0..3 (elements 0-3) and k0 + 16 + 4g + 0..3 (elements 4-7) -- the
// key order of the P^T fragment built from the S^T accumulators.  Per 16-lane group, lane 4q+p
// addresses row q, columns 4p..4p+3 of a 4 x 16 block (ds_read_b64_tr_b16); EXEC must be full.
SSE_DEV bf16x8 v_frag_tr(const char* Vs, int k0, int d0, int g, int r16) {
  const char* p = Vs + (k0 + 4 * g + (r16 >> 2)) * VR_STRIDE + (d0 + 4 * (r16 & 3)) * 2;
  const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p));
  const bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p + 16 * VR_STRIDE));
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

template <bool BIAS, bool H16 = false>   // H16: fp16 q/k/v/gate and output (SSE_DTYPE_FP16)
__global__ __launch_bounds__(256, 3) void attention_flash2_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* gate = (float*)(smem + 2 * F2_BUF);       // [F2_Q]
  float* rb = gate + F2_Q;                         // [2*Tk]
  int qc, h, b;
  attn_block_xcd(qc, h, b);
  const int TS = a.T, T = a.tlen ? a.tlen[b] : a.T, H = a.H, LQ = a.ldq;   // frames of this clip / row stride
  if (T <= a.min_t) return;   // a short clip of a mixed ragged batch: the short-T kernel's
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r16 = lane & 15;
  const int q0 = qc * F2_Q;
  const int nkt = (T + F2_K - 1) / F2_K, Tk = nkt * F2_K;
  const bf16* qkv = (const bf16*)a.qkv + (long long)b * TS * LQ;

  if (BIAS) {
    if (tid < F2_Q)
      gate[tid] = q0 + tid < T ? wavlm_gate_v<H16>(*(const bf16x8*)(qkv + (long long)(q0 + tid) * LQ + 3 * H + 8 * h),
                                                   a.gconst[h])
                               : 0.f;
    const float* rh = a.relb + (long long)h * (2 * a.maxd + 1) + a.maxd;
    for (int u = tid; u < 2 * Tk - 1; u += 256) {
      int d = u - (Tk - 1);
      d = d < -a.maxd ? -a.maxd : (d > a.maxd ? a.maxd : d);
      rb[u] = rh[d];
    }
  }
  // staging roles: K and V rows, 2 chunks of 16 B per thread each (chunk tid and tid + 256)
  const int kr0 = tid >> 3, kch = tid & 7;
  bf16x8 kreg[2], vreg[2];
  auto load_tile = [&](int kt) {
    const int kb0 = kt * F2_K;
    #pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int key = kb0 + kr0 + 32 * u;
      const bf16* row = qkv + (long long)key * LQ + h * AT_HD + kch * 8;
      kreg[u] = key < T ? *(const bf16x8*)(row + H) : bf16x8{};
      vreg[u] = key < T ? *(const bf16x8*)(row + 2 * H) : bf16x8{};
    }
  };
  auto store_tile = [&](int buf) {
    char* Ks = smem + buf * F2_BUF;
    char* Vs = Ks + F2_KS;
    #pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int kr = kr0 + 32 * u;
      *(bf16x8*)(Ks + kr * 128 + ((kch ^ ((kr >> 1) & 7)) * 16)) = kreg[u];
      *(bf16x8*)(Vs + kr * VR_STRIDE + kch * 16) = vreg[u];
    }
  };

  // Q fragments of the wave's two 16-query blocks
  bf16x8 qf[2][2];
  int qi[2];
  #pragma unroll
  for (int qq = 0; qq < 2; ++qq) {
    qi[qq] = q0 + wave * F2_QPW + qq * 16 + r16;
    const bool v = qi[qq] < T;
    const bf16* qrow = qkv + (long long)(v ? qi[qq] : 0) * LQ + h * AT_HD;
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[qq][ks] = v ? *(const bf16x8*)(qrow + ks * 32 + g * 8) : bf16x8{};
  }
  f32x4 o[2][4];
  float m_run[2];
  f32x2 l_run[2];
  #pragma unroll
  for (int qq = 0; qq < 2; ++qq) {
    m_run[qq] = -INFINITY;
    l_run[qq] = f32x2{0.f, 0.f};
    #pragma unroll
    for (int i = 0; i < 4; ++i) o[qq][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float LOG2E = 1.4426950408889634f;
  const float sl2 = a.scale * LOG2E;

  load_tile(0);
  store_tile(0);
  __syncthreads();
  // one K/V tile; LAST: the ragged final tile (keys >= T masked), a separate instantiation so the
  // steady tiles carry no mask selects
  auto tile_step = [&](int kt, auto last_c) {
    constexpr bool last = decltype(last_c)::value;
    const int cur = kt & 1;
    if (kt + 1 < nkt) load_tile(kt + 1);           // in flight during this tile's MFMAs
    const char* Ks = smem + cur * F2_BUF;
    const char* Vs = Ks + F2_KS;
    const int kbase = kt * F2_K;
    f32x4 sc[2][4];
    #pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const int kr = kb * 16 + r16;
      const bf16x8 k0 = *(const bf16x8*)(Ks + kr * 128 + (((g) ^ ((kr >> 1) & 7)) * 16));
      const bf16x8 k1 = *(const bf16x8*)(Ks + kr * 128 + (((g + 4) ^ ((kr >> 1) & 7)) * 16));
      #pragma unroll
      for (int qq = 0; qq < 2; ++qq) {
        f32x4 acc = mfma_h<H16>(k0, qf[qq][0], f32x4{0.f, 0.f, 0.f, 0.f});
        sc[qq][kb] = mfma_h<H16>(k1, qf[qq][1], acc);
      }
    }
    // online softmax in the log2 domain: v = s * scale * log2(e) (+ gate * log2(e) * bias), p = 2^(v - m)
    // with the raw v_exp_f32; pairs of scores in packed fp32 (v_pk_mul / v_pk_add); the cross-lane
    // max over the 4 key groups by v_permlane16/32_swap; key masking only in the ragged last tile
    bf16x8 pf[2][2];
    if constexpr (!BIAS) {
      // Whisper (no bias): the row max over the RAW scores (scale > 0 commutes with max), the running max
      // in the scaled log2 domain moved only when a row's max grows past it by more than F2_TH (p then
      // stays <= 2^F2_TH, exact in the bf16 P and the fp32 sums), and p = 2^fma(s, scale log2 e, -m):
      // one packed fma per score pair where the scaled form took a multiply and a subtract, and the O / l
      // rescale only on a real jump
      #pragma unroll
      for (int qq = 0; qq < 2; ++qq) {
        f32x2 s2[8];
        #pragma unroll
        for (int kb = 0; kb < 4; ++kb)
          #pragma unroll
          for (int hh = 0; hh < 2; ++hh) {
            f32x2 v = f32x2{sc[qq][kb][2 * hh], sc[qq][kb][2 * hh + 1]};
            if (last) {
              const int key = kbase + kb * 16 + 4 * g + 2 * hh;
              v = f32x2{key < T ? v.x : -INFINITY, key + 1 < T ? v.y : -INFINITY};
            }
            s2[kb * 2 + hh] = v;
          }
        float tmax;
        {
          tmax = __builtin_elementwise_maximum(__builtin_elementwise_maximum(s2[0].x, s2[0].y), s2[1].x);
          tmax = __builtin_elementwise_maximum(__builtin_elementwise_maximum(tmax, s2[1].y), s2[2].x);
          #pragma unroll
          for (int e = 2; e < 8; ++e) tmax = e == 2 ? __builtin_elementwise_maximum(tmax, s2[2].y) : __builtin_elementwise_maximum(__builtin_elementwise_maximum(tmax, s2[e].x), s2[e].y);
          const auto t16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(tmax), __float_as_uint(tmax), false, false);
          tmax = __builtin_elementwise_maximum(__uint_as_float(t16[0]), __uint_as_float(t16[1]));
          const auto t32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(tmax), __float_as_uint(tmax), false, false);
          tmax = __builtin_elementwise_maximum(__uint_as_float(t32[0]), __uint_as_float(t32[1]));
        }
        const float tm = tmax * sl2;
        // finite floor: a row with every key so far masked keeps fma(-inf, ., -m) = -inf, never NaN
        const float m_use = fmaxf(tm > m_run[qq] + F2_TH ? tm : m_run[qq], -1e30f);
        if (__any(m_use > m_run[qq])) {
          const float alpha = __builtin_amdgcn_exp2f(m_run[qq] - m_use);
          l_run[qq] *= f32x2{alpha, alpha};
          #pragma unroll
          for (int i = 0; i < 4; ++i) {
            const f32x2 lo = f32x2{o[qq][i][0], o[qq][i][1]} * alpha, hi = f32x2{o[qq][i][2], o[qq][i][3]} * alpha;
            o[qq][i] = f32x4{lo.x, lo.y, hi.x, hi.y};
          }
        }
        m_run[qq] = m_use;
        const f32x2 sl = {sl2, sl2}, nm = {-m_use, -m_use};
        #pragma unroll
        for (int e = 0; e < 8; ++e) {
          const f32x2 d = __builtin_elementwise_fma(s2[e], sl, nm);
          const f32x2 pv = {__builtin_amdgcn_exp2f(d.x), __builtin_amdgcn_exp2f(d.y)};
          l_run[qq] += pv;
          pf[qq][e >> 2][(e & 3) * 2] = hbits<H16>(pv.x);
          pf[qq][e >> 2][(e & 3) * 2 + 1] = hbits<H16>(pv.y);
        }
      }
    }
    #pragma unroll
    for (int qq = 0; qq < (BIAS ? 2 : 0); ++qq) {
      const float gq2 = BIAS ? gate[wave * F2_QPW + qq * 16 + r16] * LOG2E : 0.f;
      f32x2 v2[8];
      #pragma unroll
      for (int kb = 0; kb < 4; ++kb)
        #pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          f32x2 v = f32x2{sc[qq][kb][2 * hh], sc[qq][kb][2 * hh + 1]} * sl2;
          if (BIAS) {
            const int key = kbase + kb * 16 + 4 * g + 2 * hh - qi[qq] + (Tk - 1);
            v = __builtin_elementwise_fma(f32x2{gq2, gq2}, f32x2{rb[key], rb[key + 1]}, v);
          }
          if (last) {
            const int key = kbase + kb * 16 + 4 * g + 2 * hh;
            v = f32x2{key < T ? v.x : -INFINITY, key + 1 < T ? v.y : -INFINITY};
          }
          v2[kb * 2 + hh] = v;
        }
      float tmax = __builtin_elementwise_maximum(__builtin_elementwise_maximum(v2[0].x, v2[0].y), v2[1].x);
      tmax = __builtin_elementwise_maximum(__builtin_elementwise_maximum(tmax, v2[1].y), v2[2].x);
      #pragma unroll
      for (int e = 2; e < 8; ++e) tmax = e == 2 ? __builtin_elementwise_maximum(tmax, v2[2].y) : __builtin_elementwise_maximum(__builtin_elementwise_maximum(tmax, v2[e].x), v2[e].y);
      {
        const auto t16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(tmax), __float_as_uint(tmax), false, false);
        tmax = __builtin_elementwise_maximum(__uint_as_float(t16[0]), __uint_as_float(t16[1]));
        const auto t32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(tmax), __float_as_uint(tmax), false, false);
        tmax = __builtin_elementwise_maximum(__uint_as_float(t32[0]), __uint_as_float(t32[1]));
      }
      const float m_new = __builtin_elementwise_maximum(m_run[qq], tmax);
      // rescale only when some row's max grew (alpha == 1 exactly otherwise: skipping is exact)
      if (__any(m_new > m_run[qq])) {
        const float alpha = __builtin_amdgcn_exp2f(m_run[qq] - m_new);
        l_run[qq] *= f32x2{alpha, alpha};
        #pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x2 lo = f32x2{o[qq][i][0], o[qq][i][1]} * alpha, hi = f32x2{o[qq][i][2], o[qq][i][3]} * alpha;
          o[qq][i] = f32x4{lo.x, lo.y, hi.x, hi.y};
        }
      }
      m_run[qq] = m_new;
      const f32x2 mm = {-m_new, -m_new};
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        const f32x2 d = v2[e] + mm;
        const f32x2 pv = {__builtin_amdgcn_exp2f(d.x), __builtin_amdgcn_exp2f(d.y)};
        l_run[qq] += pv;
        pf[qq][e >> 2][(e & 3) * 2] = hbits<H16>(pv.x);
        pf[qq][e >> 2][(e & 3) * 2 + 1] = hbits<H16>(pv.y);
      }
    }
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      #pragma unroll
      for (int db = 0; db < 4; ++db) {
        const bf16x8 vf = v_frag_tr(Vs, ks * 32, db * 16, g, r16);
        #pragma unroll
        for (int qq = 0; qq < 2; ++qq) o[qq][db] = mfma_h<H16>(vf, pf[qq][ks], o[qq][db]);
      }
    if (kt + 1 < nkt) store_tile(cur ^ 1);         // buffer cur^1 was last read before the previous barrier
    __syncthreads();
  };
  const bool ragged = (T % F2_K) != 0;
  for (int kt = 0; kt < nkt - (ragged ? 1 : 0); ++kt) tile_step(kt, std::integral_constant<bool, false>{});
  if (ragged) tile_step(nkt - 1, std::integral_constant<bool, true>{});
  #pragma unroll
  for (int qq = 0; qq < 2; ++qq) {
    float l = l_run[qq].x + l_run[qq].y;
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (qi[qq] < T) {
      const float inv = 1.0f / l;
      bf16* orow = (bf16*)a.out + ((long long)b * TS + qi[qq]) * H + h * AT_HD;
      #pragma unroll
      for (int db = 0; db < 4; ++db) {
        *(uint2*)(orow + db * 16 + 4 * g) = pack_h4<H16>(o[qq][db] * inv);
      }
    }
  }
}

// Whisper flash attention (no bias), round 4: the 32x32x16 MFMA on the swapped product S^T = K Q^T, so a
// lane holds 16 scores of ONE query (its column) for each 32-key block and the row max / sum need a single
// v_permlane32_swap (the two half-waves hold the other 16 keys of the same queries), and half as many
// MFMA instructions as the 16x16x32 form (each holds the SIMD's vector issue for 8 cycles).  The K rows of a
// 32-key block enter the MFMA permuted (MFMA row r <- key pi(r)) so that the C layout leaves each lane's 16
// probabilities as exactly the two 8-key B operands of the P.V MFMAs (O^T = V^T P^T): no lane shuffles.
// Block = 4 waves x 32 queries, 64-key tiles double-buffered in LDS (register staging, flash2's layout and
// swizzles); the running max moves only past an 8 (log2) slack (flash2's no-bias path), and the row max
// itself is taken only on tiles whose row sums show a probability past that slack; the subtraction of
// the running max is a fifth k-step of the S^T MFMA (scores arrive in log2 units: q_log2).  Per tile the
// vector issue, not the MFMA pipe, is the bound, so the loop is written for VALU count:
// K / V / Q arrive by buffer loads from a resource covering the clip's T rows (keys past T read as
// zeros: no predication, no 64-bit address math), the max (when taken) is v_maximum3 on the raw MFMA
// outputs, and the softmax arithmetic is scalar f32.
// QB query blocks of 32 per wave (QB = 2: 64 queries, 256 per block, 2 waves / SIMD): every K fragment and
// V^T fragment read from LDS feeds QB MFMAs, halving the LDS instructions per query.
template <bool H16 = false, int QB = 1>
__global__ __launch_bounds__(256, QB == 1 ? 3 : 2) void attention_flash3_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int qc, h, b;
  attn_block_xcd(qc, h, b);
  const int TS = a.T, T = a.tlen ? a.tlen[b] : a.T, H = a.H, LQ = a.ldq;
  if (T <= a.min_t) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, hw = lane >> 5, g16 = lane >> 4, r16 = lane & 15;
  const int nkt = (T + F2_K - 1) / F2_K;
  // the clip's T valid rows (the host bounds T * ldq * 2 bytes below 2^31)
  const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)((const bf16*)a.qkv + (long long)b * TS * LQ), (short)0,
                                                    T * LQ * 2, 0x00020000);
  const int q0 = qc * (F2_Q * QB) + wave * (32 * QB) + j;   // this lane's query in block qb: q0 + 32 qb
  bf16x8 qf[QB][4];
  #pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const int qo = ((q0 + 32 * qb) * LQ + h * AT_HD + 8 * hw) * 2;
    #pragma unroll
    for (int ds = 0; ds < 4; ++ds)
      qf[qb][ds] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, qo + 32 * ds, 0, 0));
  }
  // staging roles (flash2): K and V rows, 2 chunks of 16 B per thread each
  const int kr0 = tid >> 3, kch = tid & 7;
  const int kvo = (kr0 * LQ + h * AT_HD + kch * 8 + H) * 2;
  bf16x8 kreg[2], vreg[2];
  auto load_tile = [&](int kt) {
    #pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int o = kvo + (kt * F2_K + 32 * u) * LQ * 2;
      kreg[u] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0));
      vreg[u] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, o + 2 * H, 0, 0));
    }
  };
  auto store_tile = [&](int buf) {
    char* Ks = smem + buf * F2_BUF;
    char* Vs = Ks + F2_KS;
    #pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int kr = kr0 + 32 * u;
      *(bf16x8*)(Ks + kr * 128 + ((kch ^ ((kr >> 1) & 7)) * 16)) = kreg[u];
      *(bf16x8*)(Vs + kr * VR_STRIDE + kch * 16) = vreg[u];
    }
  };
  // K row read by this lane for the S^T MFMA of key block kb: key 32 kb + pi(j), pi = the C-layout
  // permutation (chunk c = j / 4: 16 (c / 4) + 8 (c % 2) + 4 ((c / 2) % 2) + j % 4); 16 B at d = 16 ds + 8 hw
  const int cq = j >> 2;
  const int pik = 16 * (cq >> 2) + 8 * (cq & 1) + 4 * ((cq >> 1) & 1) + (j & 3);
  int koff[2][4];
  #pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    const int kr = 32 * kb + pik;
    #pragma unroll
    for (int ds = 0; ds < 4; ++ds) koff[kb][ds] = kr * 128 + (((2 * ds + hw) ^ ((kr >> 1) & 7)) * 16);
  }
  // V^T operand of the P.V MFMA (dims 32 db + j, keys 32 kb + 16 hh + 8 hw + 0..7): two transpose reads,
  // this 16-lane group's 4 x 16 block at keys +0..3 / +4..7, lane 4q + p -> row q, dims 4p .. 4p + 3
  const int voff0 = (8 * hw + (r16 >> 2)) * VR_STRIDE + (16 * (g16 & 1) + 4 * (r16 & 3)) * 2;
  f32x16 o[QB][2];
  #pragma unroll
  for (int qb = 0; qb < QB; ++qb)
    #pragma unroll
    for (int e = 0; e < 16; ++e) o[qb][0][e] = o[qb][1][e] = 0.f;
  // Scores arrive in log2 units (the host folded scale * log2 e into Q: AttnArgs::q_log2), and from the
  // second tile on the running max is subtracted by the matrix core: a fifth k-step of the S^T MFMA with
  // A (key side) = 1 at k = 0 and B (query side) = -m at k = 0 adds -m to every score of the query's
  // column, so p = 2^(MFMA output) with no VALU op between.  -m enters as three 16-bit terms (k = 0, 1,
  // 2: hi + mid + lo carry all 24 bits of the fp32 value), so m is the exact row max: the dominant key's p
  // is exactly 1, the same in the bf16 P of O and in the fp32 l (a 16-bit m would put up to 2^-9 between
  // the numerator's and the denominator's weight of that key).
  const bf16 h_one = hbits<H16>(1.0f), h_zero = hbits<H16>(0.0f);
  bf16x8 aext, bext[QB];
  #pragma unroll
  for (int e = 0; e < 8; ++e) aext[e] = h_zero;
  #pragma unroll
  for (int qb = 0; qb < QB; ++qb)
    #pragma unroll
    for (int e = 0; e < 8; ++e) bext[qb][e] = h_zero;
  if (hw == 0) aext[0] = aext[1] = aext[2] = h_one;
  auto set_bext = [&](int qb, float m) {
    const float nm = -m;
    const bf16 t0 = hbits<H16>(nm);
    const float r1 = nm - hval<H16>(t0);
    const bf16 t1 = hbits<H16>(r1);
    const bf16 t2 = hbits<H16>(r1 - hval<H16>(t1));
    bext[qb][0] = hw == 0 ? t0 : h_zero;
    bext[qb][1] = hw == 0 ? t1 : h_zero;
    bext[qb][2] = hw == 0 ? t2 : h_zero;
  };
  float m_run[QB], l_run[QB];
  #pragma unroll
  for (int qb = 0; qb < QB; ++qb) l_run[qb] = 0.f;
  const float lmax = 32.f * (1 << (int)F2_TH);
  load_tile(0);
  store_tile(0);
  __syncthreads();
  // kt == 0 (FIRST): plain S^T, the exact row max sets m; later tiles: see exp_tile below
  auto tile_step = [&](int kt, auto cur_c, auto first_c, auto last_c) {
    constexpr bool first = decltype(first_c)::value, last = decltype(last_c)::value;
    const int cur = cur_c;
    if (kt + 1 < nkt) load_tile(kt + 1);
    const char* Ks = smem + cur * F2_BUF;
    const char* Vs = Ks + F2_KS;
    const int kbase = kt * F2_K;
    f32x16 st[QB][2];
    #pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      bf16x8 kf[4];
      #pragma unroll
      for (int ds = 0; ds < 4; ++ds) kf[ds] = *(const bf16x8*)(Ks + koff[kb][ds]);
      #pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        #pragma unroll
        for (int e = 0; e < 16; ++e) st[qb][kb][e] = 0.f;
        if (!first) st[qb][kb] = mfma32_h<H16>(aext, bext[qb], st[qb][kb]);
        #pragma unroll
        for (int ds = 0; ds < 4; ++ds) st[qb][kb] = mfma32_h<H16>(kf[ds], qf[qb][ds], st[qb][kb]);
      }
    }
    // element e of key block kb is key 32 kb + 16 (e / 8) + 8 hw + e % 8, masked past T on the ragged tile
    if (last) {
      #pragma unroll
      for (int qb = 0; qb < QB; ++qb)
        #pragma unroll
        for (int kb = 0; kb < 2; ++kb)
          #pragma unroll
          for (int e = 0; e < 16; ++e)
            if (kbase + 32 * kb + 16 * (e >> 3) + 8 * hw + (e & 7) >= T) st[qb][kb][e] = -INFINITY;
    }
    bf16x8 pf[QB][2][2];
    #pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      // the row max over both half-waves (IEEE-754 2019 maximum: v_maximum3_f32 takes MFMA outputs as
      // they are, where fmaxf's maxnum first canonicalises each operand)
      auto row_max = [&]() {
        float ta = __builtin_elementwise_maximum(st[qb][0][0], st[qb][0][1]);
        float tb = __builtin_elementwise_maximum(st[qb][1][0], st[qb][1][1]);
        #pragma unroll
        for (int e = 2; e < 16; e += 2) {
          ta = __builtin_elementwise_maximum(__builtin_elementwise_maximum(ta, st[qb][0][e]), st[qb][0][e + 1]);
          tb = __builtin_elementwise_maximum(__builtin_elementwise_maximum(tb, st[qb][1][e]), st[qb][1][e + 1]);
        }
        const float t = __builtin_elementwise_maximum(ta, tb);
        const auto t32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(t), __float_as_uint(t), false, false);
        return __builtin_elementwise_maximum(__uint_as_float(t32[0]), __uint_as_float(t32[1]));
      };
      float lt;   // one chain: two would be paired into v_pk_add_f32, slower beside MFMAs than two v_add
      auto exp_tile = [&](float sub) {
        lt = 0.f;
        #pragma unroll
        for (int kb = 0; kb < 2; ++kb)
          #pragma unroll
          for (int e = 0; e < 16; ++e) {
            const float p = __builtin_amdgcn_exp2f(st[qb][kb][e] - sub);   // sub = 0 folds away
            lt += p;
            pf[qb][kb][e >> 3][e & 7] = hbits<H16>(p);
          }
      };
      if (first) {
        // key 0 is valid (T >= 1), so the max is finite
        m_run[qb] = row_max();
        set_bext(qb, m_run[qb]);
        exp_tile(m_run[qb]);
      } else {
        // p = 2^(s - m) against the running max as it stands, with no max taken over this tile: the
        // lane's row sum shows whether any p passed the slack (sum > 32 * 2^F2_TH).  Only then (any lane
        // of the wave) the tile's exact row max moves m by flash2's rule, O and l are rescaled and the
        // tile is exponentiated again.  p <= 2^13 where flash2 bounds it by 2^8: the same fp32 O / l
        // headroom and bf16 relative precision.
        exp_tile(0.f);
        if (__any(!(lt <= lmax))) {
          const float tmax = row_max();   // relative to m_run
          const float m_new = tmax > F2_TH ? m_run[qb] + tmax : m_run[qb];
          const float delta = m_new - m_run[qb];
          const float alpha = __builtin_amdgcn_exp2f(-delta);
          l_run[qb] *= alpha;
          #pragma unroll
          for (int db = 0; db < 2; ++db)
            #pragma unroll
            for (int e = 0; e < 16; ++e) o[qb][db][e] *= alpha;
          m_run[qb] = m_new;
          set_bext(qb, m_new);
          exp_tile(delta);
        }
      }
      l_run[qb] += lt;
    }
    #pragma unroll
    for (int kb = 0; kb < 2; ++kb)
      #pragma unroll
      for (int hh = 0; hh < 2; ++hh)
        #pragma unroll
        for (int db = 0; db < 2; ++db) {
          const char* va = Vs + (32 * kb + 16 * hh) * VR_STRIDE + 32 * db * 2 + voff0;
          const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)va);
          const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(va + 4 * VR_STRIDE));
          const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          #pragma unroll
          for (int qb = 0; qb < QB; ++qb) o[qb][db] = mfma32_h<H16>(vf, pf[qb][kb][hh], o[qb][db]);
        }
    if (kt + 1 < nkt) store_tile(cur ^ 1);
    __syncthreads();
  };
  using F = std::integral_constant<bool, false>;
  using L = std::integral_constant<bool, true>;
  const int nsteady = nkt - ((T % F2_K) != 0 ? 1 : 0);
  if (nsteady == 0) {
    tile_step(0, 0, L{}, L{});
  } else {
    tile_step(0, 0, L{}, F{});
    for (int kt = 1; kt < nsteady; ++kt) tile_step(kt, kt & 1, F{}, F{});
    if (nsteady < nkt) tile_step(nsteady, nsteady & 1, F{}, L{});
  }
  #pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    // row sum: this lane's keys + the partner half-wave's
    float l = l_run[qb];
    const auto t32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(l), __float_as_uint(l), false, false);
    l = __uint_as_float(t32[0]) + __uint_as_float(t32[1]);
    const int qi = q0 + 32 * qb;
    if (qi < T) {
      const float inv = 1.0f / l;
      bf16* orow = (bf16*)a.out + ((long long)b * TS + qi) * H + h * AT_HD;
      // o[db] element e: dim 32 db + 8 (e / 4) + 4 hw + e % 4 -> 4 consecutive dims per (db, e / 4)
      #pragma unroll
      for (int db = 0; db < 2; ++db)
        #pragma unroll
        for (int c = 0; c < 4; ++c) {
          const f32x4 x = {o[qb][db][4 * c] * inv, o[qb][db][4 * c + 1] * inv, o[qb][db][4 * c + 2] * inv,
                           o[qb][db][4 * c + 3] * inv};
          *(uint2*)(orow + 32 * db + 8 * c + 4 * hw) = pack_h4<H16>(x);
        }
    }
  }
}

// fp8 Whisper attention (round 5, SSE_DTYPE_FP8): flash3's structure -- S^T = K Q^T so that a lane holds the
// scores of ONE query, the running max subtracted by a bf16 "ext" MFMA k-step, the max taken only when a lane's
// row sum shows it moved -- with both products on the block-scaled fp8 MFMA v_mfma_scale_f32_32x32x64_f8f6f4
// (twice the bf16 rate; tools/probe_f8attn.hip fixed its layouts on gfx950):
//   operands: lane l is row (A) / column (B) l % 32; byte t of its 32 holds K index 32 (t / 16) + 16 (l / 32) +
//   t % 16, and the E8M0 scale of K block t / 16 of row r comes from lane r + 32 (t / 16); C as the bf16
//   32x32x16 (element e of lane l: row 8 (e / 4) + 4 (l / 32) + e % 4, column l % 32).
//   S^T: one MFMA per 32-key block covers d = 64.  A = K rows (e4m3 from the Q|K GEMM), B = Q, the scales
//        the GEMM's row-major MX scales (blocks of 32 dims).
//   P.V: O^T = V^T P^T.  B = P^T is the lane's own 32 probabilities in e4m3 in the order they come out of
//        S^T (byte 16 kb + e), so key(hw, 16 kb + e) = 32 kb + 8 (e / 4) + 4 hw + e % 4; A = V^T in that key
//        order, gathered by ds_read_b64_tr_b8 (a 16-lane group's 16 addresses as 8 rows x 2 halves: lane i
//        gets byte i % 8 of the rows of lanes 2k + i / 8, k = 0..7) from row-major e4m3 V in LDS.
//   V is quantised while it is staged (bf16 loads -> e4m3 with one power-of-two scale per (clip, head),
//   mx_scale_exp of the max of the V GEMM's column amax), that scale being the A scale of every key block.
// e4m3 P needs p <= 448: the row-sum trigger is 448 (every p of a lane below it), and a triggered tile moves
// the max past a 3 (log2) slack, so p <= 8 afterwards.  The row sum l adds the fp32 p before rounding
// (oracle/emulate_whisper.py: the format costs the large-v2 fixture 0.0665 -> 0.0667 rel-L2).
// Block = 4 waves x 2 query blocks of 32 (256 queries), 64-key tiles of K | V (4 KiB each, e4m3) double-
// buffered in LDS.
constexpr float F8_TH = 3.0f;
constexpr int F8_KV = 64 * 64;      // one 64-key tile of K or V, e4m3
constexpr int F8_BUF = 2 * F8_KV;   // K | V
typedef int i32x8f8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4f8 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) i32x2 lds_i32x2;
typedef short v2i16f8 __attribute__((ext_vector_type(2)));
typedef __bf16 v2bf16f8 __attribute__((ext_vector_type(2)));

template <int QB>   // query blocks of 32 per wave (2: 256 queries per block)
__global__ __launch_bounds__(256, QB == 1 ? 3 : 2) void attention_f8_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[2 * F8_BUF];
  int qc, h, b;
  attn_block_xcd(qc, h, b);
  const int T = a.T, H = a.H, L8 = 2 * H, LS = (2 * H) >> 5;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, hw = lane >> 5, g16 = (lane >> 4) & 1, i16 = lane & 15;
  const int nkt = (T + 63) / 64;
  const long long row0 = (long long)b * T;
  // the clip's T rows of Q|K, their scales and V (rows past T read as zeros)
  const auto rq = __builtin_amdgcn_make_buffer_rsrc((void*)(a.qk8 + row0 * L8), (short)0, T * L8, 0x00020000);
  const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.qks + row0 * LS), (short)0, T * LS, 0x00020000);
  const auto rv = __builtin_amdgcn_make_buffer_rsrc((void*)((const bf16*)a.v16 + row0 * H), (short)0, T * H * 2,
                                                    0x00020000);
  const int q0 = qc * (128 * QB) + wave * (32 * QB) + j;   // this lane's query in block qb: q0 + 32 qb
  i32x8f8 qf[QB];
  int qsc[QB];
  #pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const int qo = (q0 + 32 * qb) * L8 + 64 * h + 16 * hw;
    const u32x4f8 lo = __builtin_bit_cast(u32x4f8, __builtin_amdgcn_raw_buffer_load_b128(rq, qo, 0, 0));
    const u32x4f8 hi = __builtin_bit_cast(u32x4f8, __builtin_amdgcn_raw_buffer_load_b128(rq, qo + 32, 0, 0));
    qf[qb] = i32x8f8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    qsc[qb] = __builtin_amdgcn_raw_buffer_load_b8(rs, (q0 + 32 * qb) * LS + 2 * h + hw, 0, 0);
  }
  // V scale: one power of two per (clip, head), from the max of the head's 64 column amax (the e4m3 normal range
  // spans 14 binades below it, so a per-column scale buys nothing measurable: oracle/emulate_whisper.py
  // qk8pv8x 0.06673 vs qk8pv8h 0.06683) -- the A scale of every V^T block and its inverse for the staging
  const int kch = tid & 7;
  int vsc;
  {
    const unsigned* vam = a.vamax + (long long)b * H + 64 * h;
    unsigned vm = max(vam[j], vam[32 + j]);   // non-negative float bits order as unsigned
    #pragma unroll
    for (int o = 1; o < 32; o <<= 1) vm = max(vm, (unsigned)__shfl_xor((int)vm, o, 64));
    vsc = mx_scale_exp(__uint_as_float(vm));
  }
  // staging: K row tid >> 2, 16-B chunk tid & 3 (swizzled by (row >> 2) & 3: the S^T reads of 16 rows at one
  // chunk hit 16 distinct bank groups); V rows tid >> 3 (+32), dims 8 kch (16-B chunks swizzled by
  // (row >> 3) & 3: a transpose read's rows r and r + 8 apart)
  const int kr = tid >> 2, kc = tid & 3, vr = tid >> 3;
  const int ko = kr * L8 + H + 64 * h + 16 * kc;
  const int kw = kr * 64 + 16 * (kc ^ ((kr >> 2) & 3));
  const int vo = (vr * H + 64 * h + 8 * kch) * 2;
  u32x4f8 kreg;
  bf16x8 vreg[2];
  int ksn[2];   // K scales of the tile in flight: lane (hw, r) = key 32 kb + r, dim block hw
  auto load_tile = [&](int kt) {
    kreg = __builtin_bit_cast(u32x4f8, __builtin_amdgcn_raw_buffer_load_b128(rq, ko + kt * 64 * L8, 0, 0));
    #pragma unroll
    for (int u = 0; u < 2; ++u)
      vreg[u] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rv, vo + (kt * 64 + 32 * u) * H * 2, 0, 0));
    #pragma unroll
    for (int kb = 0; kb < 2; ++kb)
      ksn[kb] = __builtin_amdgcn_raw_buffer_load_b8(rs, (kt * 64 + 32 * kb + j) * LS + (LS >> 1) + 2 * h + hw, 0, 0);
  };
  // bf16 pairs -> e4m3 / 2^E in one v_cvt_scalef32_pk_fp8_bf16 each (tools/probe_cvt.hip: x / 2^exponent(scale),
  // RNE, the same bytes as cvt_pk_fp8_f32(x * 2^-E))
  const float vdiv = __builtin_bit_cast(float, (unsigned)(vsc > 0 ? vsc : 1) << 23);
  auto store_tile = [&](int buf) {
    char* Ks = smem + buf * F8_BUF;
    char* Vs = Ks + F8_KV;
    *(u32x4f8*)(Ks + kw) = kreg;
    #pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int row = vr + 32 * u;
      const bf16x8 x = vreg[u];
      v2i16f8 w0 = {0, 0}, w1 = {0, 0};
      w0 = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(w0, v2bf16f8{x[0], x[1]}, vdiv, false);
      w0 = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(w0, v2bf16f8{x[2], x[3]}, vdiv, true);
      w1 = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(w1, v2bf16f8{x[4], x[5]}, vdiv, false);
      w1 = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(w1, v2bf16f8{x[6], x[7]}, vdiv, true);
      *(i32x2*)(Vs + row * 64 + 16 * ((kch >> 1) ^ ((row >> 3) & 3)) + 8 * (kch & 1)) =
          i32x2{__builtin_bit_cast(int, w0), __builtin_bit_cast(int, w1)};
    }
  };
  // S^T A-operand reads: key row 32 kb + j, dim chunks hw and 2 + hw (kb = 1: + 2048, the same swizzle)
  const int koff0 = j * 64 + 16 * (hw ^ ((j >> 2) & 3)), koff1 = j * 64 + 16 * ((2 + hw) ^ ((j >> 2) & 3));
  // V^T transpose-read addresses (this lane as a source of its 16-lane group: k = i16 >> 1, half i16 & 1):
  // read rho (bytes 8 rho .. +7 of the operand) -> key row 32 (rho >> 1) + 16 (rho & 1) + 8 (k >> 2) + 4 hw + k % 4
  // (rho >> 1 adds 2048 with the same swizzle)
  int voff[2][2];
  {
    const int k = i16 >> 1, hh = i16 & 1;
    #pragma unroll
    for (int db = 0; db < 2; ++db)
      #pragma unroll
      for (int r1 = 0; r1 < 2; ++r1) {
        const int row = 16 * r1 + 8 * (k >> 2) + 4 * hw + (k & 3);
        voff[db][r1] = row * 64 + 16 * ((2 * db + g16) ^ ((row >> 3) & 3)) + 8 * hh;
      }
  }
  f32x16 o[QB][2];
  #pragma unroll
  for (int qb = 0; qb < QB; ++qb)
    #pragma unroll
    for (int e = 0; e < 16; ++e) o[qb][0][e] = o[qb][1][e] = 0.f;
  // the running max enters S^T as a bf16 k-step (flash3): A (key side) = 1 at k = 0..2, B = -m in 3 terms
  bf16x8 aext, bext[QB];
  #pragma unroll
  for (int e = 0; e < 8; ++e) aext[e] = (bf16)0.0f;
  #pragma unroll
  for (int qb = 0; qb < QB; ++qb)
    #pragma unroll
    for (int e = 0; e < 8; ++e) bext[qb][e] = (bf16)0.0f;
  if (hw == 0) aext[0] = aext[1] = aext[2] = (bf16)1.0f;
  auto set_bext = [&](int qb, float m) {
    const float nm = -m;
    const bf16 t0 = (bf16)nm;
    const float r1 = nm - (float)t0;
    const bf16 t1 = (bf16)r1;
    const bf16 t2 = (bf16)(r1 - (float)t1);
    bext[qb][0] = hw == 0 ? t0 : (bf16)0.0f;
    bext[qb][1] = hw == 0 ? t1 : (bf16)0.0f;
    bext[qb][2] = hw == 0 ? t2 : (bf16)0.0f;
  };
  float m_run[QB], l_run[QB];
  #pragma unroll
  for (int qb = 0; qb < QB; ++qb) l_run[qb] = 0.f;
  constexpr float lmax = 448.f;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  auto tile_step = [&](int kt, int cur, auto first_c, auto last_c) {
    constexpr bool first = decltype(first_c)::value, last = decltype(last_c)::value;
    const int ksc0 = ksn[0], ksc1 = ksn[1];
    if (kt + 1 < nkt) load_tile(kt + 1);
    const char* Ks = smem + cur * F8_BUF;
    const char* Vs = Ks + F8_KV;
    const int kbase = kt * 64;
    f32x16 st[QB][2];
    #pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const u32x4f8 lo = *(const u32x4f8*)(Ks + 2048 * kb + koff0);
      const u32x4f8 hi = *(const u32x4f8*)(Ks + 2048 * kb + koff1);
      const i32x8f8 kf = {(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
      #pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        #pragma unroll
        for (int e = 0; e < 16; ++e) st[qb][kb][e] = 0.f;
        if (!first) st[qb][kb] = mfma32_h<false>(aext, bext[qb], st[qb][kb]);
        st[qb][kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf, qf[qb], st[qb][kb], 0, 0, 0, kb ? ksc1 : ksc0,
                                                                     0, qsc[qb]);
      }
    }
    if (last) {   // element e of key block kb is key 32 kb + 8 (e / 4) + 4 hw + e % 4
      #pragma unroll
      for (int qb = 0; qb < QB; ++qb)
        #pragma unroll
        for (int kb = 0; kb < 2; ++kb)
          #pragma unroll
          for (int e = 0; e < 16; ++e)
            if (kbase + 32 * kb + 8 * (e >> 2) + 4 * hw + (e & 3) >= T) st[qb][kb][e] = -INFINITY;
    }
    i32x8f8 pf[QB];
    #pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      auto row_max = [&]() {
        float ta = __builtin_elementwise_maximum(st[qb][0][0], st[qb][0][1]);
        float tb = __builtin_elementwise_maximum(st[qb][1][0], st[qb][1][1]);
        #pragma unroll
        for (int e = 2; e < 16; e += 2) {
          ta = __builtin_elementwise_maximum(__builtin_elementwise_maximum(ta, st[qb][0][e]), st[qb][0][e + 1]);
          tb = __builtin_elementwise_maximum(__builtin_elementwise_maximum(tb, st[qb][1][e]), st[qb][1][e + 1]);
        }
        const float t = __builtin_elementwise_maximum(ta, tb);
        const auto t32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(t), __float_as_uint(t), false, false);
        return __builtin_elementwise_maximum(__uint_as_float(t32[0]), __uint_as_float(t32[1]));
      };
      float lt;
      auto exp_tile = [&](float sub) {
        lt = 0.f;
        #pragma unroll
        for (int w = 0; w < 8; ++w) {   // dword w: bytes 4 w .. 4 w + 3 = (kb, e) = (w / 4, 4 (w % 4) ..)
          const int kb = w >> 2, e0 = 4 * (w & 3);
          const float p0 = __builtin_amdgcn_exp2f(st[qb][kb][e0] - sub);
          const float p1 = __builtin_amdgcn_exp2f(st[qb][kb][e0 + 1] - sub);
          const float p2 = __builtin_amdgcn_exp2f(st[qb][kb][e0 + 2] - sub);
          const float p3 = __builtin_amdgcn_exp2f(st[qb][kb][e0 + 3] - sub);
          lt += p0;
          lt += p1;
          lt += p2;
          lt += p3;
          int x = __builtin_amdgcn_cvt_pk_fp8_f32(p0, p1, 0, false);
          pf[qb][w] = __builtin_amdgcn_cvt_pk_fp8_f32(p2, p3, x, true);
        }
      };
      if (first) {
        m_run[qb] = row_max();
        set_bext(qb, m_run[qb]);
        exp_tile(m_run[qb]);
      } else {
        exp_tile(0.f);
        if (__any(!(lt <= lmax))) {
          const float tmax = row_max();   // relative to m_run
          const float m_new = tmax > F8_TH ? m_run[qb] + tmax : m_run[qb];
          const float delta = m_new - m_run[qb];
          const float alpha = __builtin_amdgcn_exp2f(-delta);
          l_run[qb] *= alpha;
          #pragma unroll
          for (int db = 0; db < 2; ++db)
            #pragma unroll
            for (int e = 0; e < 16; ++e) o[qb][db][e] *= alpha;
          m_run[qb] = m_new;
          set_bext(qb, m_new);
          exp_tile(delta);
        }
      }
      l_run[qb] += lt;
    }
    #pragma unroll
    for (int db = 0; db < 2; ++db) {
      i32x8f8 vf;
      #pragma unroll
      for (int rho = 0; rho < 4; ++rho) {
        const i32x2 r = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(Vs + 2048 * (rho >> 1) + voff[db][rho & 1]));
        vf[2 * rho] = r[0];
        vf[2 * rho + 1] = r[1];
      }
      #pragma unroll
      for (int qb = 0; qb < QB; ++qb)
        o[qb][db] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf, pf[qb], o[qb][db], 0, 0, 0, vsc, 0, 0x7F);
    }
    if (kt + 1 < nkt) store_tile(cur ^ 1);
    __syncthreads();
  };
  using F = std::integral_constant<bool, false>;
  using L = std::integral_constant<bool, true>;
  const int nsteady = nkt - ((T % 64) != 0 ? 1 : 0);
  if (nsteady == 0) {
    tile_step(0, 0, L{}, L{});
  } else {
    tile_step(0, 0, L{}, F{});
    for (int kt = 1; kt < nsteady; ++kt) tile_step(kt, kt & 1, F{}, F{});
    if (nsteady < nkt) tile_step(nsteady, nsteady & 1, F{}, L{});
  }
  #pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    float l = l_run[qb];
    const auto t32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(l), __float_as_uint(l), false, false);
    l = __uint_as_float(t32[0]) + __uint_as_float(t32[1]);
    const int qi = q0 + 32 * qb;
    if (qi < T) {
      const float inv = 1.0f / l;
      if (a.out_q) {
        // MX-fp8 output (the out-projection's A operand): block 2 h + db of the row = dims 32 db .. 32 db + 31 of
        // this head, 16 in this lane (8 c + 4 hw + e, c = 0..3) and 16 in its partner (lane ^ 32).  amax over both
        // halves, E8M0 exponent, e4m3 = RNE(x 2^-E) four values per dword; the partners trade dwords so that lane
        // hw stores dims 16 hw .. 16 hw + 15 as one 16-B store (hw = 0: its dwords 0, 1 with the partner's after
        // each; hw = 1: the partner's dwords 2, 3 before its own); lane hw = 0 writes the scale byte
        unsigned char* orow = a.out_q + (row0 + qi) * H + h * AT_HD;
        #pragma unroll
        for (int db = 0; db < 2; ++db) {
          float am = 0.f;
          #pragma unroll
          for (int e = 0; e < 16; ++e) am = __builtin_elementwise_maximum(am, fabsf(o[qb][db][e] * inv));
          const auto t32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(am), __float_as_uint(am), false, false);
          am = __builtin_elementwise_maximum(__uint_as_float(t32[0]), __uint_as_float(t32[1]));
          const int e8 = mx_scale_exp(am);
          const float qs = inv * mx_inv_scale(e8);
          int w[4];
          #pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int x = __builtin_amdgcn_cvt_pk_fp8_f32(o[qb][db][4 * c] * qs, o[qb][db][4 * c + 1] * qs, 0, false);
            w[c] = __builtin_amdgcn_cvt_pk_fp8_f32(o[qb][db][4 * c + 2] * qs, o[qb][db][4 * c + 3] * qs, x, true);
          }
          const auto r0 = __builtin_amdgcn_permlane32_swap((unsigned)w[0], (unsigned)w[2], false, false);
          const auto r1 = __builtin_amdgcn_permlane32_swap((unsigned)w[1], (unsigned)w[3], false, false);
          const uint4 v = hw == 0 ? make_uint4((unsigned)w[0], r0[1], (unsigned)w[1], r1[1])
                                  : make_uint4(r0[0], (unsigned)w[2], r1[0], (unsigned)w[3]);
          *(uint4*)(orow + 32 * db + 16 * hw) = v;
          if (hw == 0) a.out_s[mx_a_scale_off(row0 + qi, (h * AT_HD + 32 * db) >> 5, H >> 7)] = (unsigned char)e8;
        }
        continue;
      }
      bf16* orow = (bf16*)a.out + (row0 + qi) * H + h * AT_HD;
      #pragma unroll
      for (int db = 0; db < 2; ++db)
        #pragma unroll
        for (int c = 0; c < 4; ++c) {
          const f32x4 x = {o[qb][db][4 * c] * inv, o[qb][db][4 * c + 1] * inv, o[qb][db][4 * c + 2] * inv,
                           o[qb][db][4 * c + 3] * inv};
          *(uint2*)(orow + 32 * db + 8 * c + 4 * hw) = pack_h4<false>(x);
        }
    }
  }
}

int launch_attention_f8(const AttnArgs& a, int B, hipStream_t s) {
  if (a.H != a.nh * AT_HD || !a.q_log2 || a.tlen || !a.qk8 || !a.qks || !a.v16 || !a.vamax || a.T <= 0) return -3;
  if (a.out_q ? (!a.out_s || a.H % 128) : !a.out) return -3;   // MX output: K-tiles of 128 columns
  if ((long long)a.T * 2 * a.H >= (1LL << 31)) return -3;   // 32-bit buffer offsets
  // (one query block per wave, 168 VGPRs at three blocks per CU, measured 1.4 % slower per step: not kept)
  hipLaunchKernelGGL(attention_f8_kernel<2>, dim3((a.T + 255) / 256, a.nh, B), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// Short-sequence bf16 attention (T <= 160, WavLM 3 s clips: T = 149): block = (clip, hpb heads),
// one wave per 16-query block, the whole padded key row (NKB x 16 keys) of one head in LDS.
// K and V go HBM -> LDS by LDS-DMA (buffer_load ... lds, 16 B per lane, XOR-swizzled 16-B chunks
// like the GEMM's operand tiles), from a buffer resource that covers only the clip's T valid rows,
// so padded keys read as zeros (a padded V row must be finite: its probability is exactly 0).
// No register staging and a lean register budget (<= 96 VGPRs): two or three blocks share a CU,
// so one block's loads overlap another's MFMA / softmax work.
// V^T fragments come from swizzled row-major V (row = key, 128 B) by ds_read_b64_tr_b16: a lane reads
// 8 B of row k, columns d0 + 4 (r16 & 3) .. +3, and the transpose read gathers the 16-bit elements
// across lanes.  V's 16-B chunks are XOR-swizzled by 2 ((row >> 1) & 3): the 32 lanes of one LDS pass
// read 8 rows x 32 B and every row pair lands on its own 8 banks of each half (the K swizzle,
// (row >> 1) & 7, maps chunk pairs {c, c+1} onto each other and conflicts here).
template <bool BIAS, int NKB, bool RAG, bool H16 = false>   // H16: fp16 operands / output (SSE_DTYPE_FP16)
__global__ __launch_bounds__(32 * NKB, 3) void attention_full_kernel(AttnArgs a, int hpb) {
  constexpr int TP = NKB * 16;                                   // padded keys
  constexpr int QPW = 2;                                         // query blocks per wave (NKB is even)
  constexpr int NW = NKB / QPW;                                  // waves per block
  constexpr int KS_BYTES = TP * 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + KS_BYTES;
  float* gate = (float*)(Vs + KS_BYTES);                          // [TP]
  float* rb = gate + TP;                                          // [2*TP]

  const int h0 = blockIdx.x * hpb, b = blockIdx.y;
  const int TS = a.T, T = a.tlen ? a.tlen[b] : a.T, H = a.H, H3 = a.ldq;   // frames of this clip / row stride
  if (T > TP) return;   // a long clip of a mixed ragged batch: the flash kernel's
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r16 = lane & 15;
  const bf16* qkv = (const bf16*)a.qkv + (long long)b * TS * H3;
  const float LOG2E = 1.4426950408889634f;
  // rows >= T of this clip are out of range: the DMA writes zeros
  const __amdgpu_buffer_rsrc_t clip =
      __builtin_amdgcn_make_buffer_rsrc((void*)qkv, (short)0, T * H3 * 2, 0x00020000);
  // wave-instruction u (u = wave + NW * i) stages rows [8u, 8u + 8): lane -> row 8u + lane/8, LDS
  // chunk lane%8 holding source chunk (lane%8) ^ swizzle(row) (K: (row >> 1) & 7, V: 2 ((row >> 1) & 3))
  constexpr int NU = 2 * NKB / NW;   // wave-instructions per wave for each of K and V
  // fragment read offsets are lane constants + compile-time immediates: the K swizzle of row
  // kb*16 + r16 is (r16 >> 1) & 7 and the V swizzle of row 32 ks + 4 g + (r16 >> 2) (+16) is
  // 2 (((4 g + (r16 >> 2)) >> 1) & 3), whatever kb / ks
  const int swk = (r16 >> 1) & 7;
  const int koff0 = r16 * 128 + ((g ^ swk) << 4), koff1 = r16 * 128 + (((g + 4) ^ swk) << 4);
  const int rowv = 4 * g + (r16 >> 2), swv = ((rowv >> 1) & 3) << 1;
  int voffs[4];
  #pragma unroll
  for (int db = 0; db < 4; ++db) voffs[db] = rowv * 128 + (((2 * db + ((r16 & 3) >> 1)) ^ swv) << 4) + 8 * (r16 & 1);

  for (int hh = 0; hh < hpb; ++hh) {
    const int h = h0 + hh;
    if (hh) __syncthreads();   // every wave is done reading the previous head's LDS image
    #pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int row = 8 * (wave + NW * u) + (lane >> 3);
      const unsigned rbase = (unsigned)(row * H3 * 2);
      const unsigned kch = (unsigned)(((lane & 7) ^ ((row >> 1) & 7)) << 4);
      const unsigned vch = (unsigned)(((lane & 7) ^ (((row >> 1) & 3) << 1)) << 4);
      char* kdst = Ks + (wave + NW * u) * 1024;
      char* vdst = Vs + (wave + NW * u) * 1024;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(clip, LPTR(kdst), 16, rbase + kch + (unsigned)((H + h * AT_HD) * 2), 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(clip, LPTR(vdst), 16, rbase + vch + (unsigned)((2 * H + h * AT_HD) * 2), 0,
                                               0, 0);
    }
    bf16x8 qf[QPW][2];
    #pragma unroll
    for (int qq = 0; qq < QPW; ++qq) {
      const int qi = (wave + NW * qq) * 16 + r16;
      const bf16* qrow = qkv + (long long)(qi < T ? qi : 0) * H3 + h * AT_HD;
      #pragma unroll
      for (int ks = 0; ks < 2; ++ks) qf[qq][ks] = qi < T ? *(const bf16x8*)(qrow + ks * 32 + g * 8) : bf16x8{};
    }
    if (BIAS) {   // 64 * NW = 2 * TP threads: one gate entry and one bias entry per thread
      bf16x8 greg = bf16x8{};
      float rbv = 0.f;
      if (tid < T) greg = *(const bf16x8*)(qkv + (long long)tid * H3 + 3 * H + 8 * h);
      if (tid < 2 * TP - 1) {
        int d = tid - (TP - 1);
        d = d < -a.maxd ? -a.maxd : (d > a.maxd ? a.maxd : d);
        rbv = a.relb[(long long)h * (2 * a.maxd + 1) + a.maxd + d];
      }
      const float gc = a.gconst[h];
      if (tid < TP) gate[tid] = tid < T ? wavlm_gate_v<H16>(greg, gc) : 0.f;
      if (tid < 2 * TP - 1) rb[tid] = rbv;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    #pragma unroll
    for (int qq = 0; qq < QPW; ++qq) {
    const int qb = wave + NW * qq;
    const int qi = qb * 16 + r16;
    const bool qv = qi < T;
    if (qb * 16 >= T) continue;
    f32x4 s[NKB];
    #pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 kf = *(const bf16x8*)(Ks + kb * 2048 + (ks ? koff1 : koff0));
        acc = mfma_h<H16>(kf, qf[qq][ks], acc);
      }
      s[kb] = acc;
    }
    // exact softmax over the whole (padded) row (lane holds keys kb*16 + 4g + r), log2 domain:
    // v = s * scale * log2(e) (+ gate * log2(e) * bias) in packed fp32, p = 2^(v - max) with the raw
    // v_exp_f32, cross-lane max / sum over the 4 key groups by v_permlane16/32_swap.  Keys >= T can
    // only fall in the last two key blocks (dispatch: T > (NKB - 2) * 16) unless the batch is ragged.
    const float gq2 = BIAS ? gate[qb * 16 + r16] * LOG2E : 0.f;
    const float sl2 = a.scale * LOG2E;
    // scores are rewritten in place (one live copy of the row: the kernel stays at <= 96 VGPRs, two
    // 640-thread blocks per CU)
    #pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
      #pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int key = kb * 16 + 4 * g + 2 * hf;
        f32x2 v = f32x2{s[kb][2 * hf], s[kb][2 * hf + 1]} * sl2;
        if (BIAS) {
          const int d = key - qi + (TP - 1);
          v = __builtin_elementwise_fma(f32x2{gq2, gq2}, f32x2{rb[d], rb[d + 1]}, v);
        }
        if (RAG || kb >= NKB - 2) v = f32x2{key < T ? v.x : -INFINITY, key + 1 < T ? v.y : -INFINITY};
        s[kb][2 * hf] = v.x;
        s[kb][2 * hf + 1] = v.y;
      }
    float mx = __builtin_elementwise_maximum(s[0][0], s[0][1]);
    #pragma unroll
    for (int kb = 0; kb < NKB; ++kb) mx = __builtin_elementwise_maximum(__builtin_elementwise_maximum(mx, __builtin_elementwise_maximum(s[kb][0], s[kb][1])), __builtin_elementwise_maximum(s[kb][2], s[kb][3]));
    {
      const auto t16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
      mx = __builtin_elementwise_maximum(__uint_as_float(t16[0]), __uint_as_float(t16[1]));
      const auto t32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
      mx = __builtin_elementwise_maximum(__uint_as_float(t32[0]), __uint_as_float(t32[1]));
    }
    f32x2 l2 = {0.f, 0.f};
    const f32x2 mm = {-mx, -mx};
    #pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
      #pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const f32x2 d = f32x2{s[kb][2 * hf], s[kb][2 * hf + 1]} + mm;
        const f32x2 p = {__builtin_amdgcn_exp2f(d.x), __builtin_amdgcn_exp2f(d.y)};
        l2 += p;
        s[kb][2 * hf] = p.x;
        s[kb][2 * hf + 1] = p.y;
      }
    float l = l2.x + l2.y;
    {
      const auto t16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(l), __float_as_uint(l), false, false);
      l = __uint_as_float(t16[0]) + __uint_as_float(t16[1]);
      const auto t32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(l), __float_as_uint(l), false, false);
      l = __uint_as_float(t32[0]) + __uint_as_float(t32[1]);
    }
    // O^T = V^T . P^T
    f32x4 o[4];
    #pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    #pragma unroll
    for (int ks = 0; ks < NKB / 2; ++ks) {
      bf16x8 pf;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        pf[r] = hbits<H16>(s[2 * ks][r]);
        pf[4 + r] = hbits<H16>(s[2 * ks + 1][r]);
      }
      #pragma unroll
      for (int db = 0; db < 4; ++db)
      {
        const char* va = Vs + ks * 4096 + voffs[db];
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)va);
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(va + 2048));
        const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[db] = mfma_h<H16>(vf, pf, o[db]);
      }
    }
    if (qv) {
      const float inv = 1.0f / l;
      bf16* orow = (bf16*)a.out + ((long long)b * TS + qi) * H + h * AT_HD;
      #pragma unroll
      for (int db = 0; db < 4; ++db) *(uint2*)(orow + db * 16 + 4 * g) = pack_h4<H16>(o[db] * inv);
    }
    }
  }
}

template <bool BIAS, int NKB, bool RAG, bool H16>
int launch_attention_full(const AttnArgs& a, int B, hipStream_t s) {
  constexpr int TP = NKB * 16;
  const size_t lds = (size_t)2 * TP * 128 + (size_t)TP * 4 + (size_t)2 * TP * 4;
  constexpr int NT = 32 * NKB;   // NKB / 2 waves, two query blocks each
  // heads per block: resident blocks per device x rounds should cover nh / hpb * B evenly
  static int per_cu[64] = {0}, cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -2;
  if (!cus[dev]) {
    if (hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu[dev], attention_full_kernel<BIAS, NKB, RAG, H16>, NT, lds) !=
            hipSuccess)
      return -2;
    if (per_cu[dev] < 1) per_cu[dev] = 1;
  }
  const long long slots = (long long)sse_stream_cus(s, cus[dev]) * per_cu[dev];
  int hpb = 1;
  double best = 1e30;
  for (int c = 1; c <= a.nh; ++c) {   // fewest block rounds, then fewest blocks
    if (a.nh % c) continue;
    const long long nb = (long long)(a.nh / c) * B;
    const long long rounds = (nb + slots - 1) / slots;
    const double cost = (double)rounds * c + 1e-3 * c;
    if (cost < best) best = cost, hpb = c;
  }
  hipLaunchKernelGGL((attention_full_kernel<BIAS, NKB, RAG, H16>), dim3(a.nh / hpb, B), dim3(NT), lds, s, a, hpb);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// Pipelined form of attention_full_kernel: block = (clip, hpb heads) with one wave per 16-query block
// (NKB waves), looping over its heads with the NEXT head's K, V, Q and gate rows in flight (LDS-DMA into
// the other half of a double-buffered LDS image) while the current head computes.  The short-T kernel
// loads a head, waits for it and computes it: its blocks spend most of their residency waiting on loads
// (r2 PMC: VALU ~32 %, MFMA ~10 % busy, the CU reading ~10 GB/s).  Per wave the arithmetic is the
// short-T kernel's, instruction for instruction (same fragments, same softmax order), so the two are
// bit-identical; the output goes out through a buffer resource covering the clip's T rows (padded
// query rows are dropped by the range check: every wave issues exactly 4 stores per head, which the
// counted vmcnt at the top of the next head relies on).
// LDS: 2 x (K | V | Q images of TP x 128 B, gate rows TP x 16 B) + the relative-position bias rows of
// the block's heads (pairs, 2.5 KB per head); NKB = 10: 2 x 63 KB + 15 KB (hpb 6), one block per CU.
SSE_DEV void attn_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
typedef unsigned int u32x2a __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const f32x2 lds_f32x2;
typedef unsigned int u32x4a __attribute__((ext_vector_type(4)));

// One head of one 16-query block (one wave): S = K Q^T from the LDS images (K fragments first, then the
// 2 x NKB MFMAs as NKB independent chains), the gated-bias softmax over the whole padded row, O^T = V^T P^T,
// and the 4 output stores (exactly 4 buffer stores: the pipelined kernels' counted vmcnt relies on it).
// Used by attention_pipe_kernel, instruction for instruction the per-query-
// block body of attention_full_kernel (bit-identical results).
// Hooks (attention_pipe2_kernel): mid() runs once the head's K / Q / gate-row reads are consumed (after the S
// MFMAs and the gate read), end() once its V^T reads are (after the P.V MFMAs, before the stores); the other
// kernels pass no-ops, so their code is unchanged.
struct AttnNoHook {
  SSE_DEV void operator()() const {}
};
template <bool BIAS, int NKB, bool RAG, bool H16, typename Mid = AttnNoHook, typename End = AttnNoHook>
SSE_DEV void attn_head_body(const char* Ks, const char* Vs, const char* grow, const bf16x8 (&qf)[2], const float2* rbp,
                            float gcon, int T, int qi, int g, int koff0, int koff1, const int (&voffs)[4], float sl2,
                            __amdgpu_buffer_rsrc_t orsrc, unsigned obase, Mid&& mid = Mid{}, End&& end = End{}) {
  constexpr int TP = NKB * 16;
  const float LOG2E = 1.4426950408889634f;
  // all K fragments first, then the 2 x NKB MFMAs as NKB independent chains (the per-kb read ->
  // wait -> dependent MFMA pair the compiler schedules otherwise is latency-bound at 2-3 waves/SIMD)
  bf16x8 kf[NKB][2];
  #pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    kf[kb][0] = *(const bf16x8*)(Ks + kb * 2048 + koff0);
    kf[kb][1] = *(const bf16x8*)(Ks + kb * 2048 + koff1);
  }
  f32x4 s[NKB];
  #pragma unroll
  for (int kb = 0; kb < NKB; ++kb) s[kb] = mfma_h<H16>(kf[kb][0], qf[0], f32x4{0.f, 0.f, 0.f, 0.f});
  #pragma unroll
  for (int kb = 0; kb < NKB; ++kb) s[kb] = mfma_h<H16>(kf[kb][1], qf[1], s[kb]);
  float gq2 = 0.f;
  if (BIAS) gq2 = wavlm_gate_pair<H16>(*(const bf16x8*)grow, gcon, g) * LOG2E;
  mid();
  // this lane's bias pairs start at d0 = 4 g - qi + TP - 1 (d = d0 + 16 kb + 2 hf): its LDS address in a
  // register the compiler cannot fold (the table sits past 64 KB, beyond a ds_read's 16-bit offset, and a
  // folded constant base costs a v_add per read), the key-block offsets as immediates
  unsigned rl = (unsigned)(size_t)LPTR(rbp + (4 * g - qi + (TP - 1)));
  asm volatile("" : "+v"(rl));
  #pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
    #pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      // scalar f32 (packed f32 VALU issues slower than two scalar ops beside MFMAs; same values)
      const int key = kb * 16 + 4 * g + 2 * hf;
      float vx = s[kb][2 * hf] * sl2, vy = s[kb][2 * hf + 1] * sl2;
      if (BIAS) {
        const f32x2 rr = *(const lds_f32x2*)(size_t)(rl + (unsigned)((kb * 16 + 2 * hf) * 8));   // (bias[d], bias[d + 1])
        vx = __builtin_fmaf(gq2, rr.x, vx);
        vy = __builtin_fmaf(gq2, rr.y, vy);
      }
      if (RAG || kb >= NKB - 2) {
        vx = key < T ? vx : -INFINITY;
        vy = key + 1 < T ? vy : -INFINITY;
      }
      s[kb][2 * hf] = vx;
      s[kb][2 * hf + 1] = vy;
    }
  // row max: IEEE-754 2019 maximum (v_maximum3_f32) -- the same value as fmaxf on these finite / -inf
  // scores, without maxnum's canonicalising v_max in front of every operand
  float mx = __builtin_elementwise_maximum(s[0][0], s[0][1]);
  #pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    mx = __builtin_elementwise_maximum(__builtin_elementwise_maximum(mx, s[kb][0]), s[kb][1]);
    mx = __builtin_elementwise_maximum(__builtin_elementwise_maximum(mx, s[kb][2]), s[kb][3]);
  }
  {
    const auto t16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
    mx = __builtin_elementwise_maximum(__uint_as_float(t16[0]), __uint_as_float(t16[1]));
    const auto t32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
    mx = __builtin_elementwise_maximum(__uint_as_float(t32[0]), __uint_as_float(t32[1]));
  }
  float lx = 0.f, ly = 0.f;   // the even / odd keys' sums (the order of the packed form this replaced)
  #pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
    #pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const float px = __builtin_amdgcn_exp2f(s[kb][2 * hf] - mx), py = __builtin_amdgcn_exp2f(s[kb][2 * hf + 1] - mx);
      lx += px;
      ly += py;
      s[kb][2 * hf] = px;
      s[kb][2 * hf + 1] = py;
    }
  float l = lx + ly;
  {
    const auto t16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(l), __float_as_uint(l), false, false);
    l = __uint_as_float(t16[0]) + __uint_as_float(t16[1]);
    const auto t32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(l), __float_as_uint(l), false, false);
    l = __uint_as_float(t32[0]) + __uint_as_float(t32[1]);
  }
  f32x4 o[4];
  #pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  #pragma unroll
  for (int ks = 0; ks < NKB / 2; ++ks) {
    bf16x8 pf;
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      pf[r] = hbits<H16>(s[2 * ks][r]);
      pf[4 + r] = hbits<H16>(s[2 * ks + 1][r]);
    }
    #pragma unroll
    for (int db = 0; db < 4; ++db) {
      const char* va = Vs + ks * 4096 + voffs[db];
      const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)va);
      const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(va + 2048));
      const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      o[db] = mfma_h<H16>(vf, pf, o[db]);
    }
  }
  end();
  const float inv = 1.0f / l;
  #pragma unroll
  for (int db = 0; db < 4; ++db) {
    const uint2 p = pack_h4<H16>(o[db] * inv);
    __builtin_amdgcn_raw_buffer_store_b64(u32x2a{p.x, p.y}, orsrc, obase + (unsigned)((db * 16 + 4 * g) * 2), 0, 0);
  }
}

// DBG (tools/attn_probe.hip timing only): 1 = loads and waits, no compute / stores; 2 = compute on the
// first head's image, no further loads
template <bool BIAS, int NKB, bool RAG, bool H16 = false, int DBG = 0>
__global__ __launch_bounds__(64 * NKB, 1) void attention_pipe_kernel(AttnArgs a, int hpb) {
  constexpr int TP = NKB * 16;
  constexpr int NW = NKB;                      // waves: one 16-query block each
  constexpr int KS = TP * 128;                 // one head's K (V, Q) image
  constexpr int NGP = (TP + 63) / 64;          // gate-row pieces (64 rows x 16 B)
  constexpr int BUF = 3 * KS + NGP * 1024;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2* rb2 = (float2*)(smem + 2 * BUF);     // [hpb][2 * TP] bias pairs, then [hpb] gate constants
  float* gcs = (float*)(rb2 + hpb * 2 * TP);

  const int h0 = blockIdx.x * hpb, b = blockIdx.y;
  const int TS = a.T, T = a.tlen ? a.tlen[b] : a.T, H = a.H, H3 = a.ldq;
  if (T > TP) return;   // a long clip of a mixed ragged batch: the flash kernel's
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r16 = lane & 15;
  const bf16* qkv = (const bf16*)a.qkv + (long long)b * TS * H3;
  const float LOG2E = 1.4426950408889634f;
  const __amdgpu_buffer_rsrc_t orsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)((bf16*)a.out + (long long)b * TS * H), (short)0, T * H * 2, 0x00020000);
  const int swk = (r16 >> 1) & 7;
  const int koff0 = r16 * 128 + ((g ^ swk) << 4), koff1 = r16 * 128 + (((g + 4) ^ swk) << 4);
  const int rowv = 4 * g + (r16 >> 2), swv = ((rowv >> 1) & 3) << 1;
  int voffs[4];
  #pragma unroll
  for (int db = 0; db < 4; ++db) voffs[db] = rowv * 128 + (((2 * db + ((r16 & 3) >> 1)) ^ swv) << 4) + 8 * (r16 & 1);

  // head hh's K / V / Q (8-row pieces, wave w: pieces w and w + NW) and gate rows into image `buf`.
  // The DMA is inline asm: issued through the builtin, the compiler puts a vmcnt(0) in front of every
  // ds_read_b64_tr_b16 while it is in flight (it cannot tell the V^T reads from the DMA's target image),
  // which would drain the next head's loads.  Invisible to the compiler, the DMA only ever makes its own
  // vmcnt waits stronger (the asm is volatile with a memory clobber: no LDS access crosses it).  The
  // s_nop is the M0-write -> LDS-DMA wait state the hazard recognizer would otherwise have inserted.
  const u32x4a crs = {(unsigned)(size_t)qkv, (unsigned)((size_t)qkv >> 32) & 0xffffu, (unsigned)(T * H3 * 2), 0x00020000u};
  const unsigned sbase = (unsigned)(size_t)LPTR(smem);
  auto dma = [&](unsigned lds, unsigned voff) {
    asm volatile("s_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voff), "s"(crs), "{m0}"(lds) : "memory");
  };
  auto issue = [&](int hh, int buf) {
    const int h = h0 + hh;
    const unsigned base = sbase + buf * BUF;
    #pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int p = wave + NW * u;
      const int row = 8 * p + (lane >> 3);
      const unsigned rbase = (unsigned)(row * H3 * 2);
      const unsigned kch = (unsigned)(((lane & 7) ^ ((row >> 1) & 7)) << 4);
      const unsigned vch = (unsigned)(((lane & 7) ^ (((row >> 1) & 3) << 1)) << 4);
      dma(base + p * 1024, rbase + kch + (unsigned)((H + h * AT_HD) * 2));
      dma(base + KS + p * 1024, rbase + vch + (unsigned)((2 * H + h * AT_HD) * 2));
      dma(base + 2 * KS + p * 1024, rbase + kch + (unsigned)(h * AT_HD * 2));
    }
    if (BIAS && wave < NGP) dma(base + 3 * KS + wave * 1024, (unsigned)((64 * wave + lane) * H3 * 2 + (3 * H + 8 * h) * 2));
  };
  issue(0, 0);
  if (BIAS) {
    // pairs (bias[j], bias[j + 1]) per head, j < 2 TP (bias[j] = 0 for j >= 2 TP - 1)
    for (int i = tid; i < hpb * 2 * TP; i += 64 * NW) {
      const int hh = i / (2 * TP), j = i - hh * 2 * TP;
      const float* rh = a.relb + (long long)(h0 + hh) * (2 * a.maxd + 1) + a.maxd;
      float v[2];
      #pragma unroll
      for (int e = 0; e < 2; ++e) {
        v[e] = 0.f;
        if (j + e < 2 * TP - 1) {
          int d = j + e - (TP - 1);
          d = d < -a.maxd ? -a.maxd : (d > a.maxd ? a.maxd : d);
          v[e] = rh[d];
        }
      }
      rb2[i] = make_float2(v[0], v[1]);
    }
    // the gate constants too (a per-head load in the loop would be a vector load, and its wait a
    // vmcnt(0) that drains the next head's DMA)
    if (tid < hpb) gcs[tid] = a.gconst[h0 + tid];
  }
  const int qb = wave, qi = qb * 16 + r16;
  const float sl2 = a.scale * LOG2E;
  for (int hh = 0; hh < hpb; ++hh) {
    const int h = h0 + hh;
    // this wave's pieces of head hh have landed (only the 4 stores of head hh - 1 may be younger)
    if (hh == 0 || DBG == 2) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    attn_barrier();   // ...every wave's have, and every wave is done with image (hh + 1) & 1
    if (DBG != 2 && hh + 1 < hpb) issue(hh + 1, (hh + 1) & 1);
    if constexpr (DBG == 1) {
      for (int db = 0; db < 4; ++db) __builtin_amdgcn_raw_buffer_store_b64(u32x2a{0u, 0u}, orsrc, 0x7FFFFFF0u, 0, 0);
      continue;
    }
    const char* base = smem + (DBG == 2 ? 0 : (hh & 1)) * BUF;
    const char* Ks = base;
    const char* Vs = base + KS;
    const char* Qs = base + 2 * KS + qb * 2048;
    bf16x8 qf[2];
    qf[0] = *(const bf16x8*)(Qs + koff0);
    qf[1] = *(const bf16x8*)(Qs + koff1);
    // the clip's length re-read per head (opaque): hoisted out of the head loop, the ragged build's 40 key
    // masks occupied 80 SGPRs across the loop (spills into VGPR lanes, and a miscompare vs the one-head
    // kernel on ragged batches)
    int Th = T;
    if constexpr (RAG) asm volatile("" : "+s"(Th));
    attn_head_body<BIAS, NKB, RAG, H16>(Ks, Vs, base + 3 * KS + qi * 16, qf, rb2 + hh * 2 * TP, BIAS ? gcs[hh] : 0.f, Th,
                                        qi, g, koff0, koff1, voffs, sl2, orsrc, (unsigned)((qi * H + h * AT_HD) * 2));
  }
}

// Two blocks per CU (round 6; option attn_short = 2 -- measured slower, not the default).  attention_pipe_kernel's double-buffered images (2 x 63 KB)
// allow one block of 10 waves per CU: 2.5 waves per SIMD, and its SQ counters (profiles/r6_pmc_sq_attention_pipe
// .json) show a latency-bound kernel -- 45 % of wave cycles waiting, VALU 14 % and MFMA 10 % busy, no LDS bank
// conflicts.  Here a block keeps ONE image (K | V | Q | gate rows, 63 KB) and refills it in two parts while it
// computes, so two blocks fit on a CU (<= 80 KB each with the bias pairs of up to 6 heads: 5 waves per SIMD at
// the kernel's 96 VGPRs):
//   head h:  wait K|Q|gate(h), barrier 1 -> K / Q / gate reads, S MFMAs (attn_head_body part 1) -> wait V(h),
//            barrier 2 (every wave is done with K|Q|gate(h)) -> issue K|Q|gate(h + 1) -> softmax, V^T reads,
//            P.V -> barrier 3 (every wave is done with V(h)) -> issue V(h + 1) -> the 4 output stores.
// Vector-memory ops of a wave in issue order: K|Q|gate(h+1) [4 or 5], V(h+1) [2], stores(h) [4]; so the wait at
// the top of head h+1 is vmcnt(2 + 4) and the V wait at barrier 2 vmcnt(4) (head 0: vmcnt(2) / vmcnt(0)).
// Per wave the arithmetic is attn_head_body's, so the outputs are bit-identical to the other short-T kernels.
template <bool BIAS, int NKB, bool RAG, bool H16 = false>
__global__ __launch_bounds__(64 * NKB, 5) void attention_pipe2_kernel(AttnArgs a, int hpb) {
  constexpr int TP = NKB * 16;
  constexpr int NW = NKB;
  constexpr int KS = TP * 128;
  constexpr int NGP = (TP + 63) / 64;
  constexpr int BUF = 3 * KS + NGP * 1024;     // K | V | Q | gate rows
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2* rb2 = (float2*)(smem + BUF);
  float* gcs = (float*)(rb2 + hpb * 2 * TP);

  const int h0 = blockIdx.x * hpb, b = blockIdx.y;
  const int TS = a.T, T = a.tlen ? a.tlen[b] : a.T, H = a.H, H3 = a.ldq;
  if (T > TP) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r16 = lane & 15;
  const bf16* qkv = (const bf16*)a.qkv + (long long)b * TS * H3;
  const float LOG2E = 1.4426950408889634f;
  const __amdgpu_buffer_rsrc_t orsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)((bf16*)a.out + (long long)b * TS * H), (short)0, T * H * 2, 0x00020000);
  const int swk = (r16 >> 1) & 7;
  const int koff0 = r16 * 128 + ((g ^ swk) << 4), koff1 = r16 * 128 + (((g + 4) ^ swk) << 4);
  const int rowv = 4 * g + (r16 >> 2), swv = ((rowv >> 1) & 3) << 1;
  int voffs[4];
  #pragma unroll
  for (int db = 0; db < 4; ++db) voffs[db] = rowv * 128 + (((2 * db + ((r16 & 3) >> 1)) ^ swv) << 4) + 8 * (r16 & 1);
  // (inline-asm LDS-DMA as in attention_pipe_kernel: the builtin would put a vmcnt(0) before every transpose read)
  const u32x4a crs = {(unsigned)(size_t)qkv, (unsigned)((size_t)qkv >> 32) & 0xffffu, (unsigned)(T * H3 * 2), 0x00020000u};
  const unsigned sbase = (unsigned)(size_t)LPTR(smem);
  auto dma = [&](unsigned lds, unsigned voff) {
    asm volatile("s_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voff), "s"(crs), "{m0}"(lds) : "memory");
  };
  // the DMA lane offsets are recomputed from an opaque lane id at every issue: these issues sit inside the head
  // body (S scores / O accumulators live), where 7 loop-invariant offsets held across the loop spilled
  auto issue_kqg = [&](int hh) {   // K and Q (2 pieces each per wave), the gate rows (waves < NGP: one more)
    const int h = h0 + hh;
    int ln = lane;
    asm volatile("" : "+v"(ln));
    #pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int p = wave + NW * u;
      const int row = 8 * p + (ln >> 3);
      const unsigned rbase = (unsigned)(row * H3 * 2);
      const unsigned kch = (unsigned)(((ln & 7) ^ ((row >> 1) & 7)) << 4);
      dma(sbase + p * 1024, rbase + kch + (unsigned)((H + h * AT_HD) * 2));
      dma(sbase + 2 * KS + p * 1024, rbase + kch + (unsigned)(h * AT_HD * 2));
    }
    if (BIAS && wave < NGP) dma(sbase + 3 * KS + wave * 1024, (unsigned)((64 * wave + ln) * H3 * 2 + (3 * H + 8 * h) * 2));
  };
  auto issue_v = [&](int hh) {     // V (2 pieces per wave)
    const int h = h0 + hh;
    int ln = lane;
    asm volatile("" : "+v"(ln));
    #pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int p = wave + NW * u;
      const int row = 8 * p + (ln >> 3);
      const unsigned rbase = (unsigned)(row * H3 * 2);
      const unsigned vch = (unsigned)(((ln & 7) ^ (((row >> 1) & 3) << 1)) << 4);
      dma(sbase + KS + p * 1024, rbase + vch + (unsigned)((2 * H + h * AT_HD) * 2));
    }
  };
  issue_kqg(0);
  issue_v(0);
  if (BIAS) {
    for (int i = tid; i < hpb * 2 * TP; i += 64 * NW) {
      const int hh = i / (2 * TP), j = i - hh * 2 * TP;
      const float* rh = a.relb + (long long)(h0 + hh) * (2 * a.maxd + 1) + a.maxd;
      float v[2];
      #pragma unroll
      for (int e = 0; e < 2; ++e) {
        v[e] = 0.f;
        if (j + e < 2 * TP - 1) {
          int d = j + e - (TP - 1);
          d = d < -a.maxd ? -a.maxd : (d > a.maxd ? a.maxd : d);
          v[e] = rh[d];
        }
      }
      rb2[i] = make_float2(v[0], v[1]);
    }
    if (tid < hpb) gcs[tid] = a.gconst[h0 + tid];
  }
  const int qb = wave, qi = qb * 16 + r16;
  const float sl2 = a.scale * LOG2E;
  const char* Ks = smem;
  const char* Vs = smem + KS;
  const char* Qs = smem + 2 * KS + qb * 2048;
  for (int hh = 0; hh < hpb; ++hh) {
    const int h = h0 + hh;
    const bool more = hh + 1 < hpb;
    // K|Q|gate(hh) landed for this wave (younger: V(hh) and head hh - 1's 4 stores)
    if (hh == 0) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    attn_barrier();
    bf16x8 qf[2];
    qf[0] = *(const bf16x8*)(Qs + koff0);
    qf[1] = *(const bf16x8*)(Qs + koff1);
    int Th = T;
    if constexpr (RAG) asm volatile("" : "+s"(Th));
    auto mid = [&]() {
      // every K / Q / gate read of this wave retired; V(hh) landed (younger: head hh - 1's stores)
      if (hh == 0) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
      attn_barrier();
      if (more) issue_kqg(hh + 1);
    };
    auto end = [&]() {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      attn_barrier();
      if (more) issue_v(hh + 1);
    };
    attn_head_body<BIAS, NKB, RAG, H16>(Ks, Vs, smem + 3 * KS + qi * 16, qf, rb2 + hh * 2 * TP, BIAS ? gcs[hh] : 0.f, Th,
                                        qi, g, koff0, koff1, voffs, sl2, orsrc, (unsigned)((qi * H + h * AT_HD) * 2), mid,
                                        end);
  }
}

template <bool BIAS, int NKB, bool RAG, bool H16>
int launch_attention_pipe2(const AttnArgs& a, int B, hipStream_t s) {
  constexpr int TP = NKB * 16;
  constexpr int IMG = 3 * TP * 128 + ((TP + 63) / 64) * 1024;
  const auto kern = attention_pipe2_kernel<BIAS, NKB, RAG, H16>;
  constexpr int NT = 64 * NKB;
  static int per_cu[64][13] = {{0}}, cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64 || a.nh > 12 * 64) return -2;
  if (!cus[dev] && hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -2;
  // heads per block: blocks of one round, fewest heads per block (each block's first head load is exposed)
  int hpb = 1;
  double best = 1e30;
  for (int c = 1; c <= a.nh && c <= 12; ++c) {
    if (a.nh % c) continue;
    const size_t lds = (size_t)IMG + (BIAS ? (size_t)c * (2 * TP * 8 + 4) : 0);
    if (lds > 160 * 1024) continue;
    int& pc = per_cu[dev][c];
    if (!pc) {
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, kern, NT, lds) != hipSuccess) return -2;
      if (pc < 1) pc = -1;
    }
    if (pc < 1) continue;
    const long long slots = (long long)sse_stream_cus(s, cus[dev]) * pc;
    const long long nb = (long long)(a.nh / c) * B;
    const long long rounds = (nb + slots - 1) / slots;
    const double cost = (double)rounds * (c + 1);
    if (cost < best) best = cost, hpb = c;
  }
  if (best >= 1e30) return -3;
  const size_t lds = (size_t)IMG + (BIAS ? (size_t)hpb * (2 * TP * 8 + 4) : 0);
  hipLaunchKernelGGL(kern, dim3(a.nh / hpb, B), dim3(NT), lds, s, a, hpb);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <bool BIAS, int NKB, bool RAG, bool H16, int DBG = 0>
int launch_attention_pipe(const AttnArgs& a, int B, hipStream_t s) {
  constexpr int TP = NKB * 16;
  // 2 x (K | V | Q | gate rows)
  constexpr int IMG = 2 * (3 * TP * 128 + ((TP + 63) / 64) * 1024);
  const auto kern = attention_pipe_kernel<BIAS, NKB, RAG, H16, DBG>;
  constexpr int NT = 64 * NKB;
  static int per_cu[64][13] = {{0}}, cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64 || a.nh > 12 * 64) return -2;
  if (!cus[dev] && hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -2;
  // heads per block: each block pays one exposed head load (its prologue), so the cost of a choice is
  // block rounds x (heads per block + 1)
  int hpb = 1;
  double best = 1e30;
  for (int c = 1; c <= a.nh && c <= 12; ++c) {
    if (a.nh % c) continue;
    const size_t lds = (size_t)IMG + (BIAS ? (size_t)c * (2 * TP * 8 + 4) : 0);
    if (lds > 160 * 1024) continue;
    int& pc = per_cu[dev][c];
    if (!pc) {
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, kern, NT, lds) != hipSuccess)
        return -2;
      if (pc < 1) pc = -1;
    }
    if (pc < 1) continue;
    const long long slots = (long long)sse_stream_cus(s, cus[dev]) * pc;
    const long long nb = (long long)(a.nh / c) * B;
    const long long rounds = (nb + slots - 1) / slots;
    const double cost = (double)rounds * (c + 1);
    if (cost < best) best = cost, hpb = c;
  }
  if (best >= 1e30) return -3;
  const size_t lds = (size_t)IMG + (BIAS ? (size_t)hpb * (2 * TP * 8 + 4) : 0);
  hipLaunchKernelGGL(kern, dim3(a.nh / hpb, B), dim3(NT), lds, s, a, hpb);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <bool BIAS, int NKB, bool RAG, bool H16>
int launch_attention_short(const AttnArgs& a, int B, hipStream_t s) {
  // 0 (default): the double-buffered head pipeline, one block per CU (attention_pipe_kernel); 1: one head at a time
  // (the bit-identity reference); 2: two blocks per CU with single-buffered refills (attention_pipe2_kernel, round 6:
  // bit-identical and slower -- B = 128 39.3 vs 32.0 us, profiles/r6_attn_probe.txt)
  const int o = sse_opt(OPT_ATTN_SHORT);
  if (o == 1) return launch_attention_full<BIAS, NKB, RAG, H16>(a, B, s);
  if (o == 2) return launch_attention_pipe2<BIAS, NKB, RAG, H16>(a, B, s);
  return launch_attention_pipe<BIAS, NKB, RAG, H16>(a, B, s);
}

template <bool BIAS, bool RAG, bool H16>
int dispatch_full(const AttnArgs& a, int B, hipStream_t s) {
  const int nkb = ((a.T + 31) / 32) * 2;
  switch (nkb) {
    case 2: return launch_attention_short<BIAS, 2, RAG, H16>(a, B, s);
    case 4: return launch_attention_short<BIAS, 4, RAG, H16>(a, B, s);
    case 6: return launch_attention_short<BIAS, 6, RAG, H16>(a, B, s);
    case 8: return launch_attention_short<BIAS, 8, RAG, H16>(a, B, s);
    case 10: return launch_attention_short<BIAS, 10, RAG, H16>(a, B, s);
    default: return -3;
  }
}

template <typename T>
int launch_attention(const AttnArgs& a, int B, hipStream_t s) {
  if (a.H != a.nh * AT_HD) return -3;
  constexpr bool BF = sizeof(T) == 2;
  constexpr int KS_BYTES = BF ? AT_K * 128 : AT_K * 256;
  constexpr int VS_BYTES = BF ? AT_HD * VT_STRIDE * 2 : AT_K * VF_STRIDE * 4;
  const int nkt = (a.T + AT_K - 1) / AT_K;
  size_t lds = KS_BYTES + VS_BYTES + AT_Q * 4;
  if (a.relb) lds += (size_t)(2 * nkt * AT_K) * 4;
  if (lds > 160 * 1024) return -3;
  if constexpr (BF) {   // fp32 (parity) path keeps the flash kernel: its full-row form spills
    constexpr bool H = is_f16_v<T>;   // fp16 (SSE_DTYPE_FP16) or bf16 operands
    if (a.T <= 160) {   // <= 10 key blocks: the whole row in registers
      if (a.relb) return a.tlen ? dispatch_full<true, true, H>(a, B, s) : dispatch_full<true, false, H>(a, B, s);
      return a.tlen ? dispatch_full<false, true, H>(a, B, s) : dispatch_full<false, false, H>(a, B, s);
    }
    AttnArgs af = a;
    if (a.tlen) {
      // ragged batch with clips on both sides of 160 frames: each clip runs the kernel it would run
      // alone (the short-T kernel at 10 key blocks skips the long clips, the flash kernel the short
      // ones), so every clip's result is bit-identical to its solo call
      const int rc = a.relb ? launch_attention_short<true, 10, true, H>(a, B, s)
                            : launch_attention_short<false, 10, true, H>(a, B, s);
      if (rc) return rc;
      af.min_t = 160;
    }
    const int Tk = ((a.T + F2_K - 1) / F2_K) * F2_K;
    const size_t lds2 = 2 * F2_BUF + F2_Q * 4 + (a.relb ? (size_t)2 * Tk * 4 : 0);
    if (lds2 > 160 * 1024) return -3;
    dim3 g2((a.T + F2_Q - 1) / F2_Q, a.nh, B);
    if (a.relb)
      hipLaunchKernelGGL((attention_flash2_kernel<true, H>), g2, dim3(256), lds2, s, af);
    else if (!a.q_log2 || sse_opt(OPT_ATTN_LONG) == 1 || (long long)a.T * a.ldq * 2 >= (1LL << 31))   // flash3: 32-bit offsets
      hipLaunchKernelGGL((attention_flash2_kernel<false, H>), g2, dim3(256), lds2, s, af);
    else
      if (sse_opt(OPT_ATTN_LONG) == 2)
        hipLaunchKernelGGL((attention_flash3_kernel<H, 1>), g2, dim3(256), lds2, s, af);
      else
        hipLaunchKernelGGL((attention_flash3_kernel<H, 2>), dim3((a.T + 2 * F2_Q - 1) / (2 * F2_Q), a.nh, B), dim3(256),
                           lds2, s, af);
    return hipGetLastError() == hipSuccess ? 0 : -2;
  }
  if constexpr (!is_f16_v<T>) {   // fp32 (and the bf16 grid's unused tail)
    dim3 grid((a.T + AT_Q - 1) / AT_Q, a.nh, B);
    if constexpr (!BF) {
      if (a.out3 && !sse_opt(OPT_ATTN_X3_F32)) {   // split-fp16 path: the f16 matrix cores
        const size_t lx = 4 * AT_K * 128 + AT_Q * 4 + (a.relb ? (size_t)(2 * nkt * AT_K) * 4 : 0);
        if (lx > 160 * 1024) return -3;
        if (a.relb)
          hipLaunchKernelGGL((attention_kernel<T, true, true>), grid, dim3(256), lx, s, a);
        else
          hipLaunchKernelGGL((attention_kernel<T, false, true>), grid, dim3(256), lx, s, a);
        return hipGetLastError() == hipSuccess ? 0 : -2;
      }
    }
    if (a.relb)
      hipLaunchKernelGGL((attention_kernel<T, true>), grid, dim3(256), lds, s, a);
    else
      hipLaunchKernelGGL((attention_kernel<T, false>), grid, dim3(256), lds, s, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template int launch_attention<float>(const AttnArgs&, int, hipStream_t);
template int launch_attention<bf16>(const AttnArgs&, int, hipStream_t);
template int launch_attention<f16>(const AttnArgs&, int, hipStream_t);

// ---------------------------------------------------------------------------------------
// Whisper decoder cross-attention for ONE query token per clip (REF/whisper_embeddings_large.py
// :257-262 -> HF modeling_whisper.py:284-356 with key_value_states): block = (head, clip),
// 256 threads.  Scores over the T encoder frames in fp32, block softmax, then
// out[d] = sum_j p_j V[j][d] with 4 key groups x 64 dims and an LDS reduction.  Memory-bound
// (reads each K/V row once); q is pre-scaled by head_dim^-1/2 at load time.
template <typename TE>
__global__ __launch_bounds__(256) void xattn1_kernel(const TE* __restrict__ q, const TE* __restrict__ kv, int T,
                                                     int D, TE* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float sh[];
  float* qs = sh;                 // [64]
  float* sc = sh + 64;            // [T]
  float* red = sc + T;            // [4][64] + reductions
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const TE* kvb = kv + (long long)b * T * 2 * D;
  if (tid < 64) qs[tid] = to_f32(q[(long long)b * D + h * 64 + tid]);
  __syncthreads();
  float mx = -INFINITY;
  for (int j = tid; j < T; j += 256) {
    const TE* kr = kvb + (long long)j * 2 * D + h * 64;
    float s = 0.f;
    #pragma unroll 8
    for (int d = 0; d < 64; ++d) s = fmaf(qs[d], to_f32(kr[d]), s);
    sc[j] = s;
    mx = fmaxf(mx, s);
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int j = tid; j < T; j += 256) {
    const float p = expf(sc[j] - mx);
    sc[j] = p;
    sum += p;
  }
  sum = wave_sum(sum);
  if ((tid & 63) == 0) red[4 + (tid >> 6)] = sum;
  __syncthreads();
  sum = red[4] + red[5] + red[6] + red[7];
  const int kg = tid >> 6, d = tid & 63;
  float acc = 0.f;
  for (int j = kg; j < T; j += 4) acc = fmaf(sc[j], to_f32(kvb[(long long)j * 2 * D + D + h * 64 + d]), acc);
  red[8 + kg * 64 + d] = acc;
  __syncthreads();
  if (tid < 64) {
    const float o = (red[8 + d] + red[8 + 64 + d] + red[8 + 128 + d] + red[8 + 192 + d]) / sum;
    out[(long long)b * D + h * 64 + d] = from_f32<TE>(o);
  }
}

template <typename TE>
int launch_xattn1(const TE* q, const TE* kv, int B, int T, int D, int nh, TE* out, hipStream_t s) {
  const size_t lds = (64 + (size_t)T + 8 + 256) * 4;
  if (lds > 160 * 1024 || D != nh * 64) return -3;
  hipLaunchKernelGGL((xattn1_kernel<TE>), dim3(nh, B), dim3(256), lds, s, q, kv, T, D, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template int launch_xattn1<float>(const float*, const float*, int, int, int, int, float*, hipStream_t);
template int launch_xattn1<bf16>(const bf16*, const bf16*, int, int, int, int, bf16*, hipStream_t);

__global__ void bcast_rows_kernel(const float* __restrict__ v, int D, int B, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < (long long)B * D) out[i] = v[i % D];
}
int launch_bcast_rows(const float* v, int D, int B, float* out, hipStream_t s) {
  hipLaunchKernelGGL(bcast_rows_kernel, dim3((unsigned)(((long long)B * D + 255) / 256)), dim3(256), 0, s, v, D, B, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <typename TI, typename TO>
__global__ void cast_kernel(const TI* __restrict__ x, long long n, TO* __restrict__ y) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = from_f32<TO>(to_f32(x[i]));
}
template <typename TO, typename TI>
int launch_cast(const TI* x, long long n, TO* y, hipStream_t s) {
  hipLaunchKernelGGL((cast_kernel<TI, TO>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, y);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template int launch_cast<float, float>(const float*, long long, float*, hipStream_t);
template int launch_cast<bf16, float>(const float*, long long, bf16*, hipStream_t);
template int launch_cast<float, bf16>(const bf16*, long long, float*, hipStream_t);
template int launch_cast<f16, float>(const float*, long long, f16*, hipStream_t);
template int launch_cast<float, f16>(const f16*, long long, float*, hipStream_t);
