// Training-mode ConvE query trunk for gfx950, forward and backward: bn0 -> valid ks x ks convolution -> bn1 -> relu ->
// feature_drop -> fc, with batch statistics, from the rows s, r [B, O] to z [B, O]. include/mgcn_hip.h (9) has the formulas.
//
// Forward, eight launches:
//   tt_bn0_stat<false>, tt_bn0_stat<true>   sum and centred squares of the image, one partial per block of TT_RC0 rows
//   tt_conv<KS>                             one row per workgroup: x0 in LDS, c[b, f, p] as an fma chain in tap order
//   tt_bn1_stat<false>, tt_bn1_stat<true>   per filter, one partial per block of TT_RC1 rows
//   tt_bn1_finish                           mean1, rstd1, the running statistics, the (mean, rstd, gamma, beta) table
//   tt_fc_fwd                               split-K h W^T on v_mfma_f32_16x16x4_f32; h is formed from c in the A register
//   tt_fc_fold                              split partials in ascending order, then the bias
// Backward, up to ten: tt_prep (the tables from the saved statistics), tt_colsum (d fc.bias partials), tt_dw (gz^T h),
// tt_gh (gz W with the dropout / relu mask as epilogue -> ga), tt_bn1_bwd_sums, tt_bn1_bwd_apply (ga -> gc in place),
// tt_tap (tap and conv-bias partials), tt_corr (gx0 and its bn0 sums, one row per workgroup), tt_bn0_bwd_apply (ds, dr),
// tt_fold (d fc.bias, taps, conv bias).
//
// Every reduction over the batch: one partial per block of rows (a strided per-thread chain, then a halving tree in LDS: a
// function of the block's size alone), and the partials added in ascending block order from 0 by every consumer that needs
// the total (more than TT_FOLD_F32 of them in a double accumulator, rounded once). No atomics, no waiting between workgroups: same inputs, same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mgcn_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TT_MAX_O = 512;      // image of 2 O <= 1024 floats, as the eval trunk
constexpr int TT_MAX_B = 4096;     // rows: at most 256 blocks of TT_RC1 per-row partials in tt_bn0_bwd_apply's LDS
constexpr int TT_TPB = 256;
constexpr int TT_RC0 = 8;          // rows per bn0 partial
constexpr int TT_RC1 = 16;         // rows per bn1 / tap partial
constexpr int TT_RCB = 32;         // rows per fc-bias partial
constexpr int TT_NTW = 13;         // column tiles of 16 per wave in the products over O
constexpr int TT_MAX_SPLIT = 128;  // split-K of h W^T
constexpr int TT_SPLIT_BLOCKS = 512;
constexpr int TT_STAGE = 4096;     // floats of gc / taps staged in LDS by tt_corr
constexpr int TT_SLOTS_T = 5;      // ceil((1024 + 1) / 256): taps + bias per thread in tt_tap
constexpr int TT_SLOTS_I = 4;      // 1024 / 256: image elements per thread in tt_corr
constexpr int TT_FOLD_F32 = 128;   // partials added as an f32 chain; more of them in a double accumulator

struct TGeo {
  int kw, kh, ks, F, O, H, W, P, T, I, NT, NCG;
  int64_t K;
};

inline int64_t up4(int64_t v) { return (v + 3) & ~int64_t(3); }

// MGCN_OK, MGCN_EINVAL (not a ConvE geometry) or MGCN_EUNSUPPORTED
int tgeo_make(int32_t kw, int32_t kh, int32_t ks, int32_t F, int32_t O, TGeo &g) {
  if (kw < 1 || kh < 1 || ks < 1 || F < 1 || O < 1) return MGCN_EINVAL;
  if (int64_t(kw) * kh != O) return MGCN_EINVAL;
  if (ks > 2 * kw || ks > kh) return MGCN_EINVAL;
  if (O > TT_MAX_O) return MGCN_EUNSUPPORTED;
  g.kw = kw; g.kh = kh; g.ks = ks; g.F = F; g.O = O;
  g.H = 2 * kw - ks + 1; g.W = kh - ks + 1; g.P = g.H * g.W; g.T = ks * ks; g.I = 2 * O;
  g.NT = (O + 15) / 16; g.NCG = (g.NT + TT_NTW - 1) / TT_NTW;
  g.K = int64_t(F) * g.P;
  if (F > (1 << 20) || g.K >= (int64_t(1) << 28)) return MGCN_EUNSUPPORTED;
  return MGCN_OK;
}

struct TPlan {
  int MT, S, upS, KU, NB0, NB1, NBR;
  // sections of the workspace, in floats from its start (each a multiple of 4)
  int64_t o_c, o_g, o_gx0, o_zp, o_tab1, o_st0, o_p0a, o_p0b, o_p1a, o_p1b, o_q1, o_q0, o_pw, o_pfb, floats;
};

// A function of (batch, geometry) alone. MGCN_EUNSUPPORTED: a batch this file does not take
int tplan_make(int32_t B, const TGeo &g, TPlan &p) {
  if (B < 1 || B > TT_MAX_B || int64_t(B) * g.K >= (int64_t(1) << 31) || int64_t(B) * g.P < 2) return MGCN_EUNSUPPORTED;
  p.MT = (B + 15) / 16;
  p.KU = int((g.K + 15) / 16);
  const int gx = (p.MT + 3) / 4;
  int want = (TT_SPLIT_BLOCKS + gx * g.NCG - 1) / (gx * g.NCG);
  want = want > TT_MAX_SPLIT ? TT_MAX_SPLIT : want;
  want = want > p.KU ? p.KU : want;
  want = want < 1 ? 1 : want;
  p.upS = (p.KU + want - 1) / want;
  p.S = (p.KU + p.upS - 1) / p.upS;
  p.NB0 = (B + TT_RC0 - 1) / TT_RC0;
  p.NB1 = (B + TT_RC1 - 1) / TT_RC1;
  p.NBR = (B + TT_RCB - 1) / TT_RCB;
  int64_t o = 0;
  auto take = [&](int64_t n) { const int64_t at = o; o += up4(n); return at; };
  p.o_c = take(int64_t(B) * g.K);
  p.o_g = take(int64_t(B) * g.K);
  p.o_gx0 = take(int64_t(B) * g.I);
  p.o_zp = take(int64_t(p.S) * B * g.O);
  p.o_tab1 = take(int64_t(4) * g.F);
  p.o_st0 = take(4);
  p.o_p0a = take(p.NB0);
  p.o_p0b = take(p.NB0);
  p.o_p1a = take(int64_t(p.NB1) * g.F);
  p.o_p1b = take(int64_t(p.NB1) * g.F);
  p.o_q1 = take(int64_t(2) * p.NB1 * g.F);
  p.o_q0 = take(int64_t(2) * B);
  p.o_pw = take(int64_t(p.NB1) * g.F * (g.T + 1));
  p.o_pfb = take(int64_t(p.NBR) * g.O);
  p.floats = o;
  return MGCN_OK;
}

// ---------------------------------------------------------------------------------------------- shared device code
// sum over the workgroup (blockDim.x a power of two <= TT_TPB): a halving tree, the same order for the same block size
__device__ __forceinline__ float block_sum(float v, float *red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = int(blockDim.x) >> 1; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// partials in ascending order from 0: up to TT_FOLD_F32 of them an f32 chain. A longer chain (bn0 past 1024 rows, the 16-row
// blocks past 2048) runs in a double accumulator and is rounded once: 512 f32 adds are ~sqrt(512) u / 4 off, which at
// B = 4095 put rstd0 5.7 u and, through x0, rstd1 9.7 u from float64, past the 8 u such a statistic is held to
__device__ __forceinline__ float fold(const float *__restrict__ part, int n, int64_t stride) {
  if (n > TT_FOLD_F32) {
    double d = 0.0;
    for (int i = 0; i < n; ++i) d += double(part[int64_t(i) * stride]);
    return float(d);
  }
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += part[int64_t(i) * stride];
  return s;
}

// bn affine step on a centred value: the one expression both passes use, so that [a > 0] is the forward's
__device__ __forceinline__ float bn_apply(float v, float mean, float rstd, float gamma, float beta) {
  return fmaf((v - mean) * rstd, gamma, beta);
}
__device__ __forceinline__ float act_of(float c, const float4 tb) { return bn_apply(c, tb.x, tb.y, tb.z, tb.w); }
__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }
__device__ __forceinline__ float drop_of(float a, bool kept, float inv_keep) { return kept ? relu_keep_nan(a) * inv_keep : 0.f; }

struct Rows {
  const float *s, *r;
  int64_t lds, ldr;
};
// image element i of row b: 2 j = s[j], 2 j + 1 = r[j]
__device__ __forceinline__ float image_at(const Rows &q, int b, int i) {
  return (i & 1) ? q.r[int64_t(b) * q.ldr + (i >> 1)] : q.s[int64_t(b) * q.lds + (i >> 1)];
}

// ---------------------------------------------------------------------------------------------- forward: bn0
template <bool CENTER>
__global__ __launch_bounds__(TT_TPB) void tt_bn0_stat_kernel(Rows q, int batch, int O, const float *__restrict__ sums, int nb0,
                                                             float *__restrict__ out) {
  __shared__ float red[TT_TPB];
  float mean = 0.f;
  if (CENTER) mean = fold(sums, nb0, 1) / float(int64_t(2) * O * batch);
  const int b0 = int(blockIdx.x) * TT_RC0, b1 = b0 + TT_RC0 < batch ? b0 + TT_RC0 : batch;
  const int n = (b1 - b0) * O;
  float acc = 0.f;
  for (int idx = threadIdx.x; idx < n; idx += TT_TPB) {
    const int row = b0 + idx / O, j = idx % O;
    float u = q.s[int64_t(row) * q.lds + j], v = q.r[int64_t(row) * q.ldr + j];
    if (CENTER) {
      u -= mean; v -= mean;
      acc += u * u;
      acc += v * v;
    } else {
      acc += u;
      acc += v;
    }
  }
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// ---------------------------------------------------------------------------------------------- forward: convolution
struct ConvArgs {
  Rows q;
  const float *cw, *cb, *g0, *b0;
  float *rm0, *rv0;
  float mom0, eps0;
  const float *p0a, *p0b;
  int nb0, batch;
  float *saved, *st0, *c;
  TGeo g;
};

template <int KS>
__global__ __launch_bounds__(TT_TPB) void tt_conv_kernel(ConvArgs a) {
  __shared__ float img[2 * TT_MAX_O];
  const TGeo &g = a.g;
  const float n0 = float(int64_t(g.I) * a.batch);
  const float mean = fold(a.p0a, a.nb0, 1) / n0;
  const float sq = fold(a.p0b, a.nb0, 1);
  const float var = sq / n0;
  const float rstd = 1.0f / sqrtf(var + a.eps0);
  const float gam = a.g0[0], bet = a.b0[0];
  const int b = blockIdx.x;
  if (b == 0 && threadIdx.x == 0) {
    a.saved[0] = mean; a.saved[1] = rstd;
    a.st0[0] = mean; a.st0[1] = rstd; a.st0[2] = gam; a.st0[3] = bet;
    const float unbiased = sq / float(int64_t(g.I) * a.batch - 1);
    a.rm0[0] = (1.0f - a.mom0) * a.rm0[0] + a.mom0 * mean;
    a.rv0[0] = (1.0f - a.mom0) * a.rv0[0] + a.mom0 * unbiased;
  }
  for (int i = threadIdx.x; i < g.I; i += TT_TPB) img[i] = bn_apply(image_at(a.q, b, i), mean, rstd, gam, bet);
  __syncthreads();
  float *crow = a.c + int64_t(b) * g.K;
  constexpr int NP = KS ? KS * KS : 1;
  for (int p = threadIdx.x; p < g.P; p += TT_TPB) {
    const int y = p / g.W, x = p - y * g.W;
    const int base = y * g.kh + x;
    float patch[NP];
    if (KS) {
#pragma unroll
      for (int t = 0; t < NP; ++t) patch[t] = img[base + (t / (KS ? KS : 1)) * g.kh + t % (KS ? KS : 1)];
    }
    for (int f = 0; f < g.F; ++f) {
      float h = a.cb ? a.cb[f] : 0.f;
      if (KS) {
        const float *tp = a.cw + f * NP;
#pragma unroll
        for (int t = 0; t < NP; ++t) h = fmaf(tp[t], patch[t], h);
      } else {
        const float *tp = a.cw + int64_t(f) * g.T;
        for (int dy = 0; dy < g.ks; ++dy)
          for (int dx = 0; dx < g.ks; ++dx) h = fmaf(tp[dy * g.ks + dx], img[base + dy * g.kh + dx], h);
      }
      crow[int64_t(f) * g.P + p] = h;
    }
  }
}

// ---------------------------------------------------------------------------------------------- forward: bn1
// grid (F, NB1): filter f over the rows of one block
template <bool CENTER>
__global__ __launch_bounds__(TT_TPB) void tt_bn1_stat_kernel(const float *__restrict__ c, int batch, int F, int P, int64_t K,
                                                             const float *__restrict__ sums, int nb1, float *__restrict__ out) {
  __shared__ float red[TT_TPB];
  const int f = blockIdx.x;
  float mean = 0.f;
  if (CENTER) mean = fold(sums + f, nb1, F) / float(int64_t(batch) * P);
  const int b0 = int(blockIdx.y) * TT_RC1, b1 = b0 + TT_RC1 < batch ? b0 + TT_RC1 : batch;
  const int n = (b1 - b0) * P;
  float acc = 0.f;
  for (int idx = threadIdx.x; idx < n; idx += TT_TPB) {
    const int row = b0 + idx / P, p = idx % P;
    float v = c[int64_t(row) * K + int64_t(f) * P + p];
    if (CENTER) {
      v -= mean;
      acc += v * v;
    } else {
      acc += v;
    }
  }
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) out[int64_t(blockIdx.y) * F + f] = tot;
}

__global__ __launch_bounds__(TT_TPB) void tt_bn1_finish_kernel(const float *__restrict__ p1a, const float *__restrict__ p1b, int nb1,
                                                               int F, int64_t n1, const float *__restrict__ g1,
                                                               const float *__restrict__ b1, float eps, float mom,
                                                               float *__restrict__ rm, float *__restrict__ rv,
                                                               float *__restrict__ saved, float *__restrict__ tab1) {
  const int f = int(blockIdx.x) * TT_TPB + threadIdx.x;
  if (f >= F) return;
  const float mean = fold(p1a + f, nb1, F) / float(n1);
  const float sq = fold(p1b + f, nb1, F);
  const float var = sq / float(n1);
  const float rstd = 1.0f / sqrtf(var + eps);
  saved[2 + f] = mean;
  saved[2 + F + f] = rstd;
  tab1[4 * f + 0] = mean; tab1[4 * f + 1] = rstd; tab1[4 * f + 2] = g1[f]; tab1[4 * f + 3] = b1[f];
  rm[f] = (1.0f - mom) * rm[f] + mom * mean;
  rv[f] = (1.0f - mom) * rv[f] + mom * (sq / float(n1 - 1));
}

// ---------------------------------------------------------------------------------------------- forward: fc
struct FcArgs {
  const float *c, *tab1, *fw;
  const uint8_t *keep;
  float inv_keep;
  int64_t ldw;
  float *zp;
  int batch, upS, KU, vec;
  TGeo g;
};

// grid (ceil(MT / 4), S, NCG): wave = one tile of 16 rows, up to TT_NTW column tiles, the K units [u0, u1) of its split. A
// unit is 16 k: lane (fr, fq) holds k = 16 u + 4 fq + j, j = 0..3, of its row (one 16-byte load of c, four mask bytes) and of
// its weight rows; MFMA j multiplies the lanes' j-th elements. Order of one output: units ascending, j ascending inside.
__global__ __launch_bounds__(TT_TPB) void tt_fc_fwd_kernel(FcArgs a) {
  const TGeo &g = a.g;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = (int(blockIdx.x) * 4 + wave) * 16;
  if (r0 >= a.batch) return;
  const int fr = lane & 15, fq = lane >> 4;
  const int ct0 = int(blockIdx.z) * TT_NTW;
  const int row = r0 + fr < a.batch ? r0 + fr : a.batch - 1;
  const float *crow = a.c + int64_t(row) * g.K;
  const uint8_t *krow = a.keep ? a.keep + int64_t(row) * g.K : nullptr;
  const float4 *tab = reinterpret_cast<const float4 *>(a.tab1);
  const float *wrow[TT_NTW];
#pragma unroll
  for (int t = 0; t < TT_NTW; ++t) {
    const int o = (ct0 + t) * 16 + fr;
    wrow[t] = a.fw + int64_t(o < g.O ? o : g.O - 1) * a.ldw;
  }
  f32x4 acc[TT_NTW];
#pragma unroll
  for (int t = 0; t < TT_NTW; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int u0 = int(blockIdx.y) * a.upS, u1 = u0 + a.upS < a.KU ? u0 + a.upS : a.KU;
  for (int u = u0; u < u1; ++u) {
    const int64_t k = int64_t(16) * u + 4 * fq;
    const bool whole = a.vec && k + 3 < g.K;
    float cv[4];
    uint32_t kp = 0x01010101u;
    if (whole) {
      const float4 v = *reinterpret_cast<const float4 *>(crow + k);
      cv[0] = v.x; cv[1] = v.y; cv[2] = v.z; cv[3] = v.w;
      if (krow) kp = *reinterpret_cast<const uint32_t *>(krow + k);
    } else {
      kp = krow ? 0u : kp;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        cv[j] = k + j < g.K ? crow[k + j] : 0.f;
        if (krow && k + j < g.K) kp |= uint32_t(krow[k + j]) << (8 * j);
      }
    }
    float h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      h[j] = 0.f;
      if (k + j < g.K) h[j] = drop_of(act_of(cv[j], tab[int((k + j) / g.P)]), ((kp >> (8 * j)) & 0xffu) != 0, a.inv_keep);
    }
#pragma unroll
    for (int t = 0; t < TT_NTW; ++t) {
      float w[4];
      if (whole) {
        const float4 v = *reinterpret_cast<const float4 *>(wrow[t] + k);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = k + j < g.K ? wrow[t][k + j] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(h[j], w[j], acc[t], 0, 0, 0);
    }
  }
  // lane holds rows r0 + 4 fq + i of column (ct0 + t) 16 + fr
#pragma unroll
  for (int t = 0; t < TT_NTW; ++t) {
    const int col = (ct0 + t) * 16 + fr;
    if (col >= g.O) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rw = r0 + 4 * fq + i;
      if (rw < a.batch) a.zp[(int64_t(blockIdx.y) * a.batch + rw) * g.O + col] = acc[t][i];
    }
  }
}

__global__ __launch_bounds__(TT_TPB) void tt_fc_fold_kernel(const float *__restrict__ zp, int S, int batch, int O,
                                                            const float *__restrict__ fb, float *__restrict__ z, int64_t ldz) {
  const int64_t idx = int64_t(blockIdx.x) * TT_TPB + threadIdx.x;
  if (idx >= int64_t(batch) * O) return;
  const int row = int(idx / O), col = int(idx - int64_t(row) * O);
  float total = fold(zp + idx, S, int64_t(batch) * O);
  if (fb) total += fb[col];
  z[int64_t(row) * ldz + col] = total;
}

// ---------------------------------------------------------------------------------------------- backward
__global__ __launch_bounds__(TT_TPB) void tt_prep_kernel(const float *__restrict__ saved, int F, const float *__restrict__ g0,
                                                         const float *__restrict__ b0, const float *__restrict__ g1,
                                                         const float *__restrict__ b1, float *__restrict__ st0,
                                                         float *__restrict__ tab1) {
  const int f = int(blockIdx.x) * TT_TPB + threadIdx.x;
  if (f < F) {
    tab1[4 * f + 0] = saved[2 + f]; tab1[4 * f + 1] = saved[2 + F + f]; tab1[4 * f + 2] = g1[f]; tab1[4 * f + 3] = b1[f];
  }
  if (f == 0) {
    st0[0] = saved[0]; st0[1] = saved[1]; st0[2] = g0[0]; st0[3] = b0[0];
  }
}

// grid (ceil(O / 256), NBR): column sums of gz over one block of rows
__global__ __launch_bounds__(TT_TPB) void tt_colsum_kernel(const float *__restrict__ gz, int64_t ldg, int batch, int O,
                                                           float *__restrict__ out) {
  const int o = int(blockIdx.x) * TT_TPB + threadIdx.x;
  if (o >= O) return;
  const int b0 = int(blockIdx.y) * TT_RCB, b1 = b0 + TT_RCB < batch ? b0 + TT_RCB : batch;
  float s = 0.f;
  for (int b = b0; b < b1; ++b) s += gz[int64_t(b) * ldg + o];
  out[int64_t(blockIdx.y) * O + o] = s;
}

struct BwdArgs {
  const float *gz, *c, *tab1, *fw;
  const uint8_t *keep;
  float inv_keep;
  int64_t ldg, ldw, lddw;
  float *dw, *ga;
  int batch;
  TGeo g;
};

// d fc.weight [O, K] = gz^T h. grid (ceil(K / 64), NCG): wave = 16 columns k, up to TT_NTW tiles of 16 outputs o; one chain
// over the batch in steps of four rows (ascending), h formed from c in the B register.
__global__ __launch_bounds__(TT_TPB) void tt_dw_kernel(BwdArgs a) {
  const TGeo &g = a.g;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t k0 = (int64_t(blockIdx.x) * 4 + wave) * 16;
  if (k0 >= g.K) return;
  const int fr = lane & 15, fq = lane >> 4;
  const int64_t k = k0 + fr;
  const bool kv = k < g.K;
  const int64_t kc = kv ? k : g.K - 1;
  const float4 tb = reinterpret_cast<const float4 *>(a.tab1)[int(kc / g.P)];
  const int ct0 = int(blockIdx.y) * TT_NTW;
  int ocol[TT_NTW];
#pragma unroll
  for (int t = 0; t < TT_NTW; ++t) {
    const int o = (ct0 + t) * 16 + fr;
    ocol[t] = o < g.O ? o : g.O - 1;
  }
  f32x4 acc[TT_NTW];
#pragma unroll
  for (int t = 0; t < TT_NTW; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int b0 = 0; b0 < a.batch; b0 += 4) {
    const int b = b0 + fq;
    const bool bv = b < a.batch;
    const int bc = bv ? b : a.batch - 1;
    const int64_t at = int64_t(bc) * g.K + kc;
    const bool kept = a.keep ? a.keep[at] != 0 : true;
    const float h = (bv && kv) ? drop_of(act_of(a.c[at], tb), kept, a.inv_keep) : 0.f;
    const float *grow = a.gz + int64_t(bc) * a.ldg;
#pragma unroll
    for (int t = 0; t < TT_NTW; ++t) {
      const float gv = bv ? grow[ocol[t]] : 0.f;
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv, h, acc[t], 0, 0, 0);
    }
  }
  if (!kv) return;
#pragma unroll
  for (int t = 0; t < TT_NTW; ++t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = (ct0 + t) * 16 + 4 * fq + i;
      if (o < g.O) a.dw[int64_t(o) * a.lddw + k] = acc[t][i];
    }
  }
}

// ga [B, K] = (gz W) keep inv_keep [a > 0]. grid (ceil(K / 256), ceil(MT / 4)): wave = 4 row tiles x 4 column tiles of 16;
// one chain over the outputs o in steps of four (ascending).
__global__ __launch_bounds__(TT_TPB) void tt_gh_kernel(BwdArgs a) {
  const TGeo &g = a.g;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t k0 = (int64_t(blockIdx.x) * 4 + wave) * 64;
  if (k0 >= g.K) return;
  const int fr = lane & 15, fq = lane >> 4;
  const int r0 = int(blockIdx.y) * 64;
  int64_t kc[4];
  const float *grow[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int64_t k = k0 + 16 * n + fr;
    kc[n] = k < g.K ? k : g.K - 1;
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int b = r0 + 16 * m + fr;
    grow[m] = a.gz + int64_t(b < a.batch ? b : a.batch - 1) * a.ldg;
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int o0 = 0; o0 < g.O; o0 += 4) {
    const int o = o0 + fq;
    const bool ov = o < g.O;
    const int oc = ov ? o : g.O - 1;
    float av[4], bv[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) av[m] = ov ? grow[m][oc] : 0.f;
    const float *wr = a.fw + int64_t(oc) * a.ldw;
#pragma unroll
    for (int n = 0; n < 4; ++n) bv[n] = ov ? wr[kc[n]] : 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv[n], acc[m][n], 0, 0, 0);
  }
  const float4 *tab = reinterpret_cast<const float4 *>(a.tab1);
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int64_t k = k0 + 16 * n + fr;
    if (k >= g.K) continue;
    const float4 tb = tab[int(k / g.P)];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int b = r0 + 16 * m + 4 * fq + i;
        if (b >= a.batch) continue;
        const int64_t at = int64_t(b) * g.K + k;
        const bool kept = a.keep ? a.keep[at] != 0 : true;
        const float act = act_of(a.c[at], tb);
        a.ga[at] = (act > 0.f && kept) ? acc[m][n][i] * a.inv_keep : 0.f;
      }
    }
  }
}

// grid (F, NB1): sum ga and sum ga ch of filter f over one block of rows -> q1[(blk F + f) 2 + {0, 1}]
__global__ __launch_bounds__(TT_TPB) void tt_bn1_bwd_sums_kernel(const float *__restrict__ c, const float *__restrict__ ga,
                                                                 const float *__restrict__ tab1, int batch, int F, int P, int64_t K,
                                                                 float *__restrict__ q1) {
  __shared__ float red[TT_TPB];
  const int f = blockIdx.x;
  const float mean = tab1[4 * f], rstd = tab1[4 * f + 1];
  const int b0 = int(blockIdx.y) * TT_RC1, b1 = b0 + TT_RC1 < batch ? b0 + TT_RC1 : batch;
  const int n = (b1 - b0) * P;
  float s1 = 0.f, s2 = 0.f;
  for (int idx = threadIdx.x; idx < n; idx += TT_TPB) {
    const int64_t at = int64_t(b0 + idx / P) * K + int64_t(f) * P + idx % P;
    const float gv = ga[at], ch = (c[at] - mean) * rstd;
    s1 += gv;
    s2 += gv * ch;
  }
  const float t1 = block_sum(s1, red), t2 = block_sum(s2, red);
  if (threadIdx.x == 0) {
    q1[(int64_t(blockIdx.y) * F + f) * 2] = t1;
    q1[(int64_t(blockIdx.y) * F + f) * 2 + 1] = t2;
  }
}

// grid (F, NB1): gc = g1 rstd1 (ga - d b1 / n1 - ch d g1 / n1), in place over ga; the first block of rows writes d b1, d g1
__global__ __launch_bounds__(TT_TPB) void tt_bn1_bwd_apply_kernel(const float *__restrict__ c, float *__restrict__ ga,
                                                                  const float *__restrict__ tab1, const float *__restrict__ q1,
                                                                  int nb1, int batch, int F, int P, int64_t K,
                                                                  float *__restrict__ dg1, float *__restrict__ db1) {
  const int f = blockIdx.x;
  const float mean = tab1[4 * f], rstd = tab1[4 * f + 1], gam = tab1[4 * f + 2];
  const float sb = fold(q1 + 2 * f, nb1, int64_t(2) * F), sg = fold(q1 + 2 * f + 1, nb1, int64_t(2) * F);
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    if (db1) db1[f] = sb;
    if (dg1) dg1[f] = sg;
  }
  const float n1 = float(int64_t(batch) * P);
  const float mb = sb / n1, mg = sg / n1, scale = gam * rstd;
  const int b0 = int(blockIdx.y) * TT_RC1, b1 = b0 + TT_RC1 < batch ? b0 + TT_RC1 : batch;
  const int n = (b1 - b0) * P;
  for (int idx = threadIdx.x; idx < n; idx += TT_TPB) {
    const int64_t at = int64_t(b0 + idx / P) * K + int64_t(f) * P + idx % P;
    const float ch = (c[at] - mean) * rstd;
    ga[at] = scale * ((ga[at] - mb) - ch * mg);
  }
}

// grid (F, NB1), T + 1 <= 64 ? 64 : 256 threads: thread t < T holds tap t = (dy, dx) of filter f, thread T the conv bias; one
// chain per thread over the rows of the block (ascending), inside a row over the positions in y, x order
__global__ __launch_bounds__(TT_TPB) void tt_tap_kernel(Rows q, const float *__restrict__ st0, const float *__restrict__ gc,
                                                        int batch, TGeo g, float *__restrict__ pw) {
  __shared__ float gs[2 * TT_MAX_O], img[2 * TT_MAX_O];
  const int f = blockIdx.x, nth = blockDim.x;
  const float mean = st0[0], rstd = st0[1], gam = st0[2], bet = st0[3];
  const int b0 = int(blockIdx.y) * TT_RC1, b1 = b0 + TT_RC1 < batch ? b0 + TT_RC1 : batch;
  float acc[TT_SLOTS_T];
#pragma unroll
  for (int s = 0; s < TT_SLOTS_T; ++s) acc[s] = 0.f;
  for (int b = b0; b < b1; ++b) {
    __syncthreads();
    for (int p = threadIdx.x; p < g.P; p += nth) gs[p] = gc[int64_t(b) * g.K + int64_t(f) * g.P + p];
    for (int i = threadIdx.x; i < g.I; i += nth) img[i] = bn_apply(image_at(q, b, i), mean, rstd, gam, bet);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < TT_SLOTS_T; ++s) {
      const int t = int(threadIdx.x) + s * nth;
      float v = acc[s];
      if (t < g.T) {
        const int dy = t / g.ks, dx = t - dy * g.ks;
        for (int y = 0; y < g.H; ++y) {
          const float *gr = gs + y * g.W, *ir = img + (y + dy) * g.kh + dx;
          for (int x = 0; x < g.W; ++x) v = fmaf(gr[x], ir[x], v);
        }
      } else if (t == g.T) {
        for (int p = 0; p < g.P; ++p) v += gs[p];
      }
      acc[s] = v;
    }
  }
#pragma unroll
  for (int s = 0; s < TT_SLOTS_T; ++s) {
    const int t = int(threadIdx.x) + s * nth;
    if (t <= g.T) pw[(int64_t(blockIdx.y) * g.F + f) * (g.T + 1) + t] = acc[s];
  }
}

// grid (B): gx0 [B, 2 O] of one row, thread = image element(s); chain over f, dy, dx ascending (only the taps whose window
// holds the element). gc and the taps are staged in LDS fc filters at a time. Then the row's bn0 sums -> q0[2 b + {0, 1}].
__global__ __launch_bounds__(TT_TPB) void tt_corr_kernel(Rows q, const float *__restrict__ st0, const float *__restrict__ gc,
                                                         const float *__restrict__ cw, TGeo g, int fc, float *__restrict__ gx0,
                                                         float *__restrict__ q0) {
  __shared__ float gs[TT_STAGE], wl[TT_STAGE], red[TT_TPB];
  const int b = blockIdx.x;
  float acc[TT_SLOTS_I];
#pragma unroll
  for (int s = 0; s < TT_SLOTS_I; ++s) acc[s] = 0.f;
  for (int f0 = 0; f0 < g.F; f0 += fc) {
    const int nf = f0 + fc < g.F ? fc : g.F - f0;
    __syncthreads();
    for (int i = threadIdx.x; i < nf * g.P; i += TT_TPB) gs[i] = gc[int64_t(b) * g.K + int64_t(f0) * g.P + i];
    for (int i = threadIdx.x; i < nf * g.T; i += TT_TPB) wl[i] = cw[int64_t(f0) * g.T + i];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < TT_SLOTS_I; ++s) {
      const int i = int(threadIdx.x) + s * TT_TPB;
      if (i >= g.I) continue;
      const int iy = i / g.kh, ix = i - iy * g.kh;
      const int dy0 = iy - g.H + 1 > 0 ? iy - g.H + 1 : 0, dy1 = iy < g.ks - 1 ? iy : g.ks - 1;
      const int dx0 = ix - g.W + 1 > 0 ? ix - g.W + 1 : 0, dx1 = ix < g.ks - 1 ? ix : g.ks - 1;
      float v = acc[s];
      for (int ff = 0; ff < nf; ++ff) {
        const float *gf = gs + ff * g.P, *wf = wl + ff * g.T;
        for (int dy = dy0; dy <= dy1; ++dy)
          for (int dx = dx0; dx <= dx1; ++dx) v = fmaf(gf[(iy - dy) * g.W + ix - dx], wf[dy * g.ks + dx], v);
      }
      acc[s] = v;
    }
  }
  const float mean = st0[0], rstd = st0[1];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int s = 0; s < TT_SLOTS_I; ++s) {
    const int i = int(threadIdx.x) + s * TT_TPB;
    if (i >= g.I) continue;
    gx0[int64_t(b) * g.I + i] = acc[s];
    s1 += acc[s];
    s2 += acc[s] * ((image_at(q, b, i) - mean) * rstd);
  }
  const float t1 = block_sum(s1, red), t2 = block_sum(s2, red);
  if (threadIdx.x == 0) {
    q0[2 * b] = t1;
    q0[2 * b + 1] = t2;
  }
}

// grid (B): gx = g0 rstd0 (gx0 - d b0 / n0 - xh d g0 / n0) -> ds, dr; row 0 writes d b0, d g0
__global__ __launch_bounds__(TT_TPB) void tt_bn0_bwd_apply_kernel(Rows q, const float *__restrict__ st0, const float *__restrict__ gx0,
                                                                  const float *__restrict__ q0, int batch, int I, float *__restrict__ ds,
                                                                  int64_t ldds, float *__restrict__ dr, int64_t lddr,
                                                                  float *__restrict__ dg0, float *__restrict__ db0) {
  __shared__ float gb[TT_MAX_B / TT_RC1], gg[TT_MAX_B / TT_RC1];
  const int b = blockIdx.x;
  const float mean = st0[0], rstd = st0[1], gam = st0[2];
  // the per-row partials in blocks of TT_RC1 rows (rows ascending), then the block sums ascending: at most 16 + 256 adds
  const int ng = (batch + TT_RC1 - 1) / TT_RC1;
  for (int gi = threadIdx.x; gi < ng; gi += TT_TPB) {
    const int r0 = gi * TT_RC1, nr = r0 + TT_RC1 < batch ? TT_RC1 : batch - r0;
    gb[gi] = fold(q0 + 2 * r0, nr, 2);
    gg[gi] = fold(q0 + 2 * r0 + 1, nr, 2);
  }
  __syncthreads();
  const float sb = fold(gb, ng, 1), sg = fold(gg, ng, 1);
  if (b == 0 && threadIdx.x == 0) {
    if (db0) db0[0] = sb;
    if (dg0) dg0[0] = sg;
  }
  const float n0 = float(int64_t(I) * batch);
  const float mb = sb / n0, mg = sg / n0, scale = gam * rstd;
  for (int i = threadIdx.x; i < I; i += TT_TPB) {
    const float xh = (image_at(q, b, i) - mean) * rstd;
    const float v = scale * ((gx0[int64_t(b) * I + i] - mb) - xh * mg);
    if (i & 1) {
      if (dr) dr[int64_t(b) * lddr + (i >> 1)] = v;
    } else {
      if (ds) ds[int64_t(b) * ldds + (i >> 1)] = v;
    }
  }
}

// d fc.bias [O] from its NBR partials, taps [F, T] and conv bias [F] from their NB1 partials, ascending
__global__ __launch_bounds__(TT_TPB) void tt_fold_kernel(const float *__restrict__ pfb, int nbr, int O, const float *__restrict__ pw,
                                                         int nb1, int F, int T, float *__restrict__ dfb, float *__restrict__ dcw,
                                                         float *__restrict__ dcb) {
  const int64_t idx = int64_t(blockIdx.x) * TT_TPB + threadIdx.x;
  if (idx < O) {
    if (dfb) dfb[idx] = fold(pfb + idx, nbr, O);
    return;
  }
  const int64_t e = idx - O;
  if (e >= int64_t(F) * (T + 1) || !(dcw || dcb)) return;
  const int f = int(e / (T + 1)), t = int(e - int64_t(f) * (T + 1));
  if (t < T ? dcw == nullptr : dcb == nullptr) return;
  const float v = fold(pw + e, nb1, int64_t(F) * (T + 1));
  if (t < T) dcw[int64_t(f) * T + t] = v;
  else dcb[f] = v;
}

template <int KS>
void launch_conv(const ConvArgs &a, hipStream_t s) {
  hipLaunchKernelGGL((tt_conv_kernel<KS>), dim3(unsigned(a.batch)), dim3(TT_TPB), 0, s, a);
}

// shared argument checks of both entries; MGCN_OK with g, p filled
int tt_check(const char *what, int32_t batch, int32_t kw, int32_t kh, int32_t ks, int32_t F, int32_t O, TGeo &g, TPlan &p) {
  const int rc = tgeo_make(kw, kh, ks, F, O, g);
  MGCN_REQUIRE(rc != MGCN_EINVAL, "%s: not a ConvE geometry (k_w %d, k_h %d, kernel %d, filters %d, O %d)", what, kw, kh, ks, F, O);
  if (rc) return mgcn::fail(rc, "%s: O = %d > %d or too many filters", what, O, TT_MAX_O);
  MGCN_REQUIRE(batch >= 0, "%s: negative batch", what);
  if (tplan_make(batch, g, p))
    return mgcn::fail(MGCN_EUNSUPPORTED, "%s: batch %d outside [1, %d], one value per channel, or 2^31 activations", what, batch,
                      TT_MAX_B);
  return MGCN_OK;
}

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" size_t mgcn_conve_train_workspace(int32_t batch, int32_t k_w, int32_t k_h, int32_t kernel_size, int32_t num_filter,
                                             int32_t dim_out) {
  TGeo g;
  TPlan p;
  if (tgeo_make(k_w, k_h, kernel_size, num_filter, dim_out, g) != MGCN_OK || tplan_make(batch, g, p) != MGCN_OK) return 0;
  return size_t(p.floats) * sizeof(float);
}

extern "C" int mgcn_conve_train_fwd(int32_t batch, int32_t k_w, int32_t k_h, int32_t kernel_size, int32_t num_filter,
                                    int32_t dim_out, const float *s_dev, int64_t lds, const float *r_dev, int64_t ldr,
                                    const float *conv_w_dev, const float *conv_b_dev, const float *fc_w_dev, int64_t ldw,
                                    const float *fc_b_dev, const float *bn0_gamma_dev, const float *bn0_beta_dev,
                                    float *bn0_running_mean_dev, float *bn0_running_var_dev, float bn0_momentum, float bn0_eps,
                                    const float *bn1_gamma_dev, const float *bn1_beta_dev, float *bn1_running_mean_dev,
                                    float *bn1_running_var_dev, float bn1_momentum, float bn1_eps, const uint8_t *keep_dev,
                                    float inv_keep, float *z_dev, int64_t ldz, float *saved_dev, void *workspace_dev,
                                    size_t workspace_bytes, void *stream) {
  TGeo g;
  TPlan p;
  const int rc = tt_check("conve_train_fwd", batch, k_w, k_h, kernel_size, num_filter, dim_out, g, p);
  if (rc) return rc;
  MGCN_REQUIRE(s_dev && r_dev && conv_w_dev && fc_w_dev && z_dev && saved_dev, "conve_train_fwd: null pointer");
  MGCN_REQUIRE(bn0_gamma_dev && bn0_beta_dev && bn1_gamma_dev && bn1_beta_dev, "conve_train_fwd: null BN weight or bias");
  MGCN_REQUIRE(bn0_running_mean_dev && bn0_running_var_dev && bn1_running_mean_dev && bn1_running_var_dev,
               "conve_train_fwd: null running statistics");
  MGCN_REQUIRE(lds >= g.O && ldr >= g.O && ldz >= g.O, "conve_train_fwd: leading dimension below O = %d", g.O);
  MGCN_REQUIRE(ldw >= g.K, "conve_train_fwd: ldw %lld < F H W = %lld", (long long)ldw, (long long)g.K);
  MGCN_REQUIRE(workspace_dev && mgcn::aligned16(workspace_dev), "conve_train_fwd: workspace null or not 16-byte aligned");
  MGCN_REQUIRE(workspace_bytes >= size_t(p.floats) * sizeof(float), "conve_train_fwd: workspace of %zu bytes, needs %zu",
               workspace_bytes, size_t(p.floats) * sizeof(float));

  hipStream_t st = static_cast<hipStream_t>(stream);
  float *ws = static_cast<float *>(workspace_dev);
  const Rows q = {s_dev, r_dev, lds, ldr};
  hipLaunchKernelGGL((tt_bn0_stat_kernel<false>), dim3(unsigned(p.NB0)), dim3(TT_TPB), 0, st, q, batch, g.O, nullptr, 0, ws + p.o_p0a);
  MGCN_CHECK_LAUNCH("tt_bn0_stat_kernel");
  hipLaunchKernelGGL((tt_bn0_stat_kernel<true>), dim3(unsigned(p.NB0)), dim3(TT_TPB), 0, st, q, batch, g.O, ws + p.o_p0a, p.NB0,
                     ws + p.o_p0b);
  MGCN_CHECK_LAUNCH("tt_bn0_stat_kernel");
  ConvArgs ca = {};
  ca.q = q; ca.cw = conv_w_dev; ca.cb = conv_b_dev; ca.g0 = bn0_gamma_dev; ca.b0 = bn0_beta_dev;
  ca.rm0 = bn0_running_mean_dev; ca.rv0 = bn0_running_var_dev; ca.mom0 = bn0_momentum; ca.eps0 = bn0_eps;
  ca.p0a = ws + p.o_p0a; ca.p0b = ws + p.o_p0b; ca.nb0 = p.NB0; ca.batch = batch;
  ca.saved = saved_dev; ca.st0 = ws + p.o_st0; ca.c = ws + p.o_c; ca.g = g;
  switch (g.ks) {
    case 3: launch_conv<3>(ca, st); break;
    case 5: launch_conv<5>(ca, st); break;
    case 7: launch_conv<7>(ca, st); break;
    default: launch_conv<0>(ca, st); break;
  }
  MGCN_CHECK_LAUNCH("tt_conv_kernel");
  const dim3 g1(unsigned(g.F), unsigned(p.NB1));
  hipLaunchKernelGGL((tt_bn1_stat_kernel<false>), g1, dim3(TT_TPB), 0, st, ws + p.o_c, batch, g.F, g.P, g.K, nullptr, 0, ws + p.o_p1a);
  MGCN_CHECK_LAUNCH("tt_bn1_stat_kernel");
  hipLaunchKernelGGL((tt_bn1_stat_kernel<true>), g1, dim3(TT_TPB), 0, st, ws + p.o_c, batch, g.F, g.P, g.K, ws + p.o_p1a, p.NB1,
                     ws + p.o_p1b);
  MGCN_CHECK_LAUNCH("tt_bn1_stat_kernel");
  hipLaunchKernelGGL(tt_bn1_finish_kernel, dim3(unsigned((g.F + TT_TPB - 1) / TT_TPB)), dim3(TT_TPB), 0, st, ws + p.o_p1a,
                     ws + p.o_p1b, p.NB1, g.F, int64_t(batch) * g.P, bn1_gamma_dev, bn1_beta_dev, bn1_eps, bn1_momentum,
                     bn1_running_mean_dev, bn1_running_var_dev, saved_dev, ws + p.o_tab1);
  MGCN_CHECK_LAUNCH("tt_bn1_finish_kernel");
  FcArgs fa = {};
  fa.c = ws + p.o_c; fa.tab1 = ws + p.o_tab1; fa.fw = fc_w_dev; fa.keep = keep_dev; fa.inv_keep = keep_dev ? inv_keep : 1.0f;
  fa.ldw = ldw; fa.zp = ws + p.o_zp; fa.batch = batch; fa.upS = p.upS; fa.KU = p.KU;
  fa.vec = g.K % 4 == 0 && ldw % 4 == 0 && mgcn::aligned16(fc_w_dev) && (!keep_dev || aligned4(keep_dev));
  fa.g = g;
  hipLaunchKernelGGL(tt_fc_fwd_kernel, dim3(unsigned((p.MT + 3) / 4), unsigned(p.S), unsigned(g.NCG)), dim3(TT_TPB), 0, st, fa);
  MGCN_CHECK_LAUNCH("tt_fc_fwd_kernel");
  const int64_t n = int64_t(batch) * g.O;
  hipLaunchKernelGGL(tt_fc_fold_kernel, dim3(unsigned((n + TT_TPB - 1) / TT_TPB)), dim3(TT_TPB), 0, st, ws + p.o_zp, p.S, batch, g.O,
                     fc_b_dev, z_dev, ldz);
  MGCN_CHECK_LAUNCH("tt_fc_fold_kernel");
  return MGCN_OK;
}

extern "C" int mgcn_conve_train_bwd(int32_t batch, int32_t k_w, int32_t k_h, int32_t kernel_size, int32_t num_filter,
                                    int32_t dim_out, const float *s_dev, int64_t lds, const float *r_dev, int64_t ldr,
                                    const float *conv_w_dev, const float *fc_w_dev, int64_t ldw, const float *bn0_gamma_dev,
                                    const float *bn0_beta_dev, const float *bn1_gamma_dev, const float *bn1_beta_dev,
                                    const uint8_t *keep_dev, float inv_keep, const float *saved_dev, const float *gz_dev,
                                    int64_t ldg, float *ds_dev, int64_t ldds, float *dr_dev, int64_t lddr, float *d_conv_w_dev,
                                    float *d_conv_b_dev, float *d_bn0_gamma_dev, float *d_bn0_beta_dev, float *d_bn1_gamma_dev,
                                    float *d_bn1_beta_dev, float *d_fc_w_dev, int64_t lddw, float *d_fc_b_dev,
                                    void *workspace_dev, size_t workspace_bytes, void *stream) {
  TGeo g;
  TPlan p;
  const int rc = tt_check("conve_train_bwd", batch, k_w, k_h, kernel_size, num_filter, dim_out, g, p);
  if (rc) return rc;
  MGCN_REQUIRE(s_dev && r_dev && conv_w_dev && fc_w_dev && saved_dev && gz_dev, "conve_train_bwd: null pointer");
  MGCN_REQUIRE(bn0_gamma_dev && bn0_beta_dev && bn1_gamma_dev && bn1_beta_dev, "conve_train_bwd: null BN weight or bias");
  MGCN_REQUIRE(lds >= g.O && ldr >= g.O && ldg >= g.O, "conve_train_bwd: leading dimension below O = %d", g.O);
  MGCN_REQUIRE((!ds_dev || ldds >= g.O) && (!dr_dev || lddr >= g.O), "conve_train_bwd: gradient leading dimension below O = %d", g.O);
  MGCN_REQUIRE(ldw >= g.K && (!d_fc_w_dev || lddw >= g.K), "conve_train_bwd: fc leading dimension below F H W = %lld", (long long)g.K);
  MGCN_REQUIRE(workspace_dev && mgcn::aligned16(workspace_dev), "conve_train_bwd: workspace null or not 16-byte aligned");
  MGCN_REQUIRE(workspace_bytes >= size_t(p.floats) * sizeof(float), "conve_train_bwd: workspace of %zu bytes, needs %zu",
               workspace_bytes, size_t(p.floats) * sizeof(float));

  hipStream_t st = static_cast<hipStream_t>(stream);
  float *ws = static_cast<float *>(workspace_dev);
  const Rows q = {s_dev, r_dev, lds, ldr};
  const bool need_tap = d_conv_w_dev || d_conv_b_dev;
  const bool need_corr = ds_dev || dr_dev || d_bn0_gamma_dev || d_bn0_beta_dev;
  const bool need_gh = need_tap || need_corr || d_bn1_gamma_dev || d_bn1_beta_dev;

  hipLaunchKernelGGL(tt_prep_kernel, dim3(unsigned((g.F + TT_TPB - 1) / TT_TPB)), dim3(TT_TPB), 0, st, saved_dev, g.F, bn0_gamma_dev,
                     bn0_beta_dev, bn1_gamma_dev, bn1_beta_dev, ws + p.o_st0, ws + p.o_tab1);
  MGCN_CHECK_LAUNCH("tt_prep_kernel");
  if (d_fc_b_dev) {
    hipLaunchKernelGGL(tt_colsum_kernel, dim3(unsigned((g.O + TT_TPB - 1) / TT_TPB), unsigned(p.NBR)), dim3(TT_TPB), 0, st, gz_dev, ldg,
                       batch, g.O, ws + p.o_pfb);
    MGCN_CHECK_LAUNCH("tt_colsum_kernel");
  }
  BwdArgs ba = {};
  ba.gz = gz_dev; ba.c = ws + p.o_c; ba.tab1 = ws + p.o_tab1; ba.fw = fc_w_dev; ba.keep = keep_dev;
  ba.inv_keep = keep_dev ? inv_keep : 1.0f;
  ba.ldg = ldg; ba.ldw = ldw; ba.lddw = lddw; ba.dw = d_fc_w_dev; ba.ga = ws + p.o_g; ba.batch = batch; ba.g = g;
  if (d_fc_w_dev) {
    hipLaunchKernelGGL(tt_dw_kernel, dim3(unsigned((g.K + 63) / 64), unsigned(g.NCG)), dim3(TT_TPB), 0, st, ba);
    MGCN_CHECK_LAUNCH("tt_dw_kernel");
  }
  if (need_gh) {
    const dim3 g1(unsigned(g.F), unsigned(p.NB1));
    hipLaunchKernelGGL(tt_gh_kernel, dim3(unsigned((g.K + 255) / 256), unsigned((p.MT + 3) / 4)), dim3(TT_TPB), 0, st, ba);
    MGCN_CHECK_LAUNCH("tt_gh_kernel");
    hipLaunchKernelGGL(tt_bn1_bwd_sums_kernel, g1, dim3(TT_TPB), 0, st, ws + p.o_c, ws + p.o_g, ws + p.o_tab1, batch, g.F, g.P, g.K,
                       ws + p.o_q1);
    MGCN_CHECK_LAUNCH("tt_bn1_bwd_sums_kernel");
    hipLaunchKernelGGL(tt_bn1_bwd_apply_kernel, g1, dim3(TT_TPB), 0, st, ws + p.o_c, ws + p.o_g, ws + p.o_tab1, ws + p.o_q1, p.NB1, batch,
                       g.F, g.P, g.K, d_bn1_gamma_dev, d_bn1_beta_dev);
    MGCN_CHECK_LAUNCH("tt_bn1_bwd_apply_kernel");
    if (need_tap) {
      hipLaunchKernelGGL(tt_tap_kernel, g1, dim3(g.T + 1 <= 64 ? 64 : TT_TPB), 0, st, q, ws + p.o_st0, ws + p.o_g, batch, g, ws + p.o_pw);
      MGCN_CHECK_LAUNCH("tt_tap_kernel");
    }
    if (need_corr) {
      int fc = TT_STAGE / (g.P > g.T ? g.P : g.T);
      fc = fc < 1 ? 1 : fc > g.F ? g.F : fc;
      hipLaunchKernelGGL(tt_corr_kernel, dim3(unsigned(batch)), dim3(TT_TPB), 0, st, q, ws + p.o_st0, ws + p.o_g, conv_w_dev, g, fc,
                         ws + p.o_gx0, ws + p.o_q0);
      MGCN_CHECK_LAUNCH("tt_corr_kernel");
      hipLaunchKernelGGL(tt_bn0_bwd_apply_kernel, dim3(unsigned(batch)), dim3(TT_TPB), 0, st, q, ws + p.o_st0, ws + p.o_gx0, ws + p.o_q0,
                         batch, g.I, ds_dev, ldds, dr_dev, lddr, d_bn0_gamma_dev, d_bn0_beta_dev);
      MGCN_CHECK_LAUNCH("tt_bn0_bwd_apply_kernel");
    }
  }
  if (d_fc_b_dev || need_tap) {
    const int64_t n = int64_t(g.O) + (need_tap ? int64_t(g.F) * (g.T + 1) : 0);
    hipLaunchKernelGGL(tt_fold_kernel, dim3(unsigned((n + TT_TPB - 1) / TT_TPB)), dim3(TT_TPB), 0, st, ws + p.o_pfb, p.NBR, g.O,
                       ws + p.o_pw, p.NB1, g.F, g.T, d_fc_b_dev, d_conv_w_dev, d_conv_b_dev);
    MGCN_CHECK_LAUNCH("tt_fold_kernel");
  }
  return MGCN_OK;
}
