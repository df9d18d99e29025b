// Eval-mode ConvE query trunk (reference model.py:161-175) for gfx950: bn0 -> valid ks x ks convolution -> bn1 -> relu -> flatten ->
// fc -> bn2 -> relu, from the two embedding tables (rows picked by index inside the kernel) to x [B, O]. include/mgcn_hip.h (8).
//
// One wave owns a tile of 16 queries and up to 13 column tiles of 16 outputs. The [B, F H W] activation exists only as MFMA A
// operands: lane (q = lane & 15, j = lane >> 4) keeps the ks x ks image patch of position 4 pq + j of query q in registers, and
// for every filter f forms ONE activation h = relu(const[f] + sum_t tap[f][t] patch[t]) (an fma chain in tap order; bn0, the conv
// bias and bn1 are folded into taps and const by the pack kernel, in double, rounded once) which is at once the A fragment of
// v_mfma_f32_16x16x4_f32 (exact f32) against the FC weights of (pq, f), stored in fragment order by the pack kernel. The taps are
// wave-uniform (scalar loads), the patch is loaded once per position quad and reused by all F filters.
//
// Summation order of output (query, o), a function of the geometry only:
//   segment pq = 0 .. ceil(H W / 4) - 1: one accumulator chain from 0 over f = 0 .. F-1, each step the MFMA's four terms
//   (positions 4 pq .. 4 pq + 3 of filter f; positions past H W carry zero weights);
//   total = 0; total += segment[pq] in ascending pq; y = relu(fma(total, scale[o], shift[o])).
// The launch walks all segments inside one wave (large batches: totals in registers) or spreads them over workgroups (small
// batches: every segment's partial goes to the workspace, a second launch adds them in the same order and applies the same
// epilogue). Both give the same bits, and a row's bits do not depend on the batch or on its position in it: MFMA rows are
// independent, and nothing else is shared between queries. A non-finite input makes its own row non-finite only (the relus keep
// NaN: v < 0 ? 0 : v).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mgcn_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CT_MAX_O = 512;         // image of 2 O floats per query; wider shapes are refused
constexpr int CT_NTW = 13;            // column tiles of 16 per wave (208 outputs): wider outputs take several column groups
constexpr int CT_ROWS = 16;           // queries per wave
constexpr int CT_WAVES = 4;           // independent waves per workgroup (they share the weight stream in L1)
constexpr int CT_SPLIT_TILES = 512;   // at most this many query tiles: segments go across workgroups
constexpr int CT_SPLIT_WAVES = 4096;  // ... over about this many waves

struct Geo {
  int kw, kh, ks, F, O;
  int H, W, P, PQ, NT, OP, NCG, NTP;   // NT column tiles of 16 in NCG groups of CT_NTW: NTP = NCG CT_NTW tiles in the pack
  int64_t off_cst, off_scale, off_shift, off_w, floats;   // sections of the pack, in floats (each a multiple of 16)
};

inline int64_t up16(int64_t v) { return (v + 15) & ~int64_t(15); }

// MGCN_OK, MGCN_EINVAL (not a ConvE geometry) or MGCN_EUNSUPPORTED (one this kernel does not take)
int geo_make(int32_t kw, int32_t kh, int32_t ks, int32_t F, int32_t O, Geo &g) {
  if (kw < 1 || kh < 1 || ks < 1 || F < 1 || O < 1) return MGCN_EINVAL;
  if (int64_t(kw) * kh != O) return MGCN_EINVAL;
  if (ks > 2 * kw || ks > kh) return MGCN_EINVAL;
  if (O > CT_MAX_O) return MGCN_EUNSUPPORTED;
  g.kw = kw; g.kh = kh; g.ks = ks; g.F = F; g.O = O;
  g.H = 2 * kw - ks + 1; g.W = kh - ks + 1; g.P = g.H * g.W; g.PQ = (g.P + 3) / 4;
  g.NT = (O + 15) / 16; g.OP = g.NT * 16; g.NCG = (g.NT + CT_NTW - 1) / CT_NTW; g.NTP = g.NCG * CT_NTW;
  g.off_cst = up16(int64_t(F) * ks * ks);
  g.off_scale = g.off_cst + up16(F);
  g.off_shift = g.off_scale + g.OP;
  g.off_w = g.off_shift + g.OP;
  g.floats = g.off_w + int64_t(g.PQ) * F * g.NTP * 64;
  if (g.floats >= (int64_t(1) << 31)) return MGCN_EUNSUPPORTED;
  return MGCN_OK;
}

struct Plan {
  int tiles, nsplit, seg_per;   // nsplit == 0: every wave walks all segments, no workspace
  size_t ws_bytes;
};

// A function of (batch, geometry) alone: mgcn_conve_trunk_workspace and the launch must agree, and the header keeps no device state
Plan plan_make(int32_t batch, const Geo &g) {
  Plan p = {};
  p.tiles = (batch + CT_ROWS - 1) / CT_ROWS;
  if (batch > 0 && p.tiles <= CT_SPLIT_TILES && g.PQ > 1) {
    int want = CT_SPLIT_WAVES / (p.tiles * g.NCG);
    want = want < 1 ? 1 : want > g.PQ ? g.PQ : want;
    p.seg_per = (g.PQ + want - 1) / want;
    p.nsplit = (g.PQ + p.seg_per - 1) / p.seg_per;
    p.ws_bytes = size_t(g.PQ) * size_t(batch) * size_t(g.OP) * sizeof(float);
  }
  return p;
}

// ---------------------------------------------------------------------------------------------- pack
struct BnPtrs { const float *mean, *var, *gamma, *beta; float eps; };
struct PackArgs {
  const float *cw, *cb, *fw, *fb;
  int64_t ldw;
  BnPtrs bn0, bn1, bn2;
  float *out;
  Geo g;
};

__device__ __forceinline__ double bn_scale(const BnPtrs &b, int i) {
  return (b.gamma ? double(b.gamma[i]) : 1.0) / sqrt(double(b.var[i]) + double(b.eps));
}
__device__ __forceinline__ double bn_beta(const BnPtrs &b, int i) { return b.beta ? double(b.beta[i]) : 0.0; }

// out[idx], one float per thread:
//   [0, F ks^2)            tap'[f][t] = w[f][t] s0 s1[f]
//   [off_cst, + F)         const[f] = s1[f] (t0 sum_t w[f][t] + conv bias[f] - mean1[f]) + beta1[f],  t0 = beta0 - mean0 s0
//   [off_scale, + OP)      s2[o];   [off_shift, + OP)  (fc bias[o] - mean2[o]) s2[o] + beta2[o]      (0 past O)
//   [off_w, ...)           ((pq F + f) NTP + ct) 64 + lane: fc.weight[16 ct + (lane & 15)][f P + 4 pq + (lane >> 4)], 0 outside
//                          (every column group is padded to CT_NTW tiles, so the trunk's inner loop has no tile guards)
__global__ __launch_bounds__(256) void conve_pack_kernel(PackArgs a) {
  const Geo &g = a.g;
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= g.floats) return;
  const int ks2 = g.ks * g.ks;
  float v = 0.f;
  if (idx < g.off_cst) {
    if (idx < int64_t(g.F) * ks2) {
      const int f = int(idx / ks2);
      v = float(double(a.cw[idx]) * bn_scale(a.bn0, 0) * bn_scale(a.bn1, f));
    }
  } else if (idx < g.off_scale) {
    const int f = int(idx - g.off_cst);
    if (f < g.F) {
      const double s0 = bn_scale(a.bn0, 0), t0 = bn_beta(a.bn0, 0) - double(a.bn0.mean[0]) * s0;
      double sum = 0.0;
      for (int t = 0; t < ks2; ++t) sum += double(a.cw[int64_t(f) * ks2 + t]);
      v = float(bn_scale(a.bn1, f) * (t0 * sum + (a.cb ? double(a.cb[f]) : 0.0) - double(a.bn1.mean[f])) + bn_beta(a.bn1, f));
    }
  } else if (idx < g.off_shift) {
    const int o = int(idx - g.off_scale);
    if (o < g.O) v = float(bn_scale(a.bn2, o));
  } else if (idx < g.off_w) {
    const int o = int(idx - g.off_shift);
    if (o < g.O) v = float(((a.fb ? double(a.fb[o]) : 0.0) - double(a.bn2.mean[o])) * bn_scale(a.bn2, o) + bn_beta(a.bn2, o));
  } else {
    int64_t r = idx - g.off_w;
    const int lane = int(r & 63);
    r >>= 6;
    const int ct = int(r % g.NTP);
    r /= g.NTP;
    const int f = int(r % g.F), pq = int(r / g.F);
    const int o = ct * 16 + (lane & 15), p = 4 * pq + (lane >> 4);
    if (o < g.O && p < g.P) v = a.fw[int64_t(o) * a.ldw + int64_t(f) * g.P + p];
  }
  a.out[idx] = v;
}

// ---------------------------------------------------------------------------------------------- trunk
struct TrunkArgs {
  const float *ent, *rel;
  const int64_t *si, *ri;      // null: row b
  int64_t lde, ldr, n_ent, n_rel, ldo;
  int32_t batch, seg_per;
  Geo g;
};

__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }
__device__ __forceinline__ float trunk_epilogue(float total, float scale, float shift) {
  return relu_keep_nan(fmaf(total, scale, shift));
}

// KS: the kernel size as a constant (patch in registers, taps unrolled), 0 = any (image values re-read per tap)
template <int KS, bool SPLIT>
__global__ __launch_bounds__(CT_WAVES * 64, 2) void conve_trunk_kernel(TrunkArgs a, const float *__restrict__ pk,
                                                                       float *__restrict__ out, float *__restrict__ ws) {
  const Geo &g = a.g;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q0 = (int(blockIdx.x) * CT_WAVES + wave) * CT_ROWS;
  if (q0 >= a.batch) return;
  const int fr = lane & 15, fq = lane >> 4;
  const int ct0 = int(blockIdx.z) * CT_NTW;

  // this lane's query (rows past the batch repeat the last one: their outputs are not stored)
  const int q = q0 + fr < a.batch ? q0 + fr : a.batch - 1;
  int64_t srow = a.si ? a.si[q] : q, rrow = a.ri ? a.ri[q] : q;
  srow = srow < 0 ? 0 : srow >= a.n_ent ? a.n_ent - 1 : srow;
  rrow = rrow < 0 ? 0 : rrow >= a.n_rel ? a.n_rel - 1 : rrow;
  const float *sp = a.ent + srow * a.lde, *rp = a.rel + rrow * a.ldr;
  // image [2 k_w, k_h], flat element 2 j = s[j], 2 j + 1 = r[j] (the reference interleaves)
  auto image = [&](int i) { return ((i & 1) ? rp : sp)[i >> 1]; };

  const float *taps = pk, *cst = pk + g.off_cst;
  constexpr int NP = KS ? KS * KS : 1;
  const int ks2 = g.ks * g.ks;
  const int seg0 = SPLIT ? int(blockIdx.y) * a.seg_per : 0;
  const int seg1 = SPLIT ? (seg0 + a.seg_per < g.PQ ? seg0 + a.seg_per : g.PQ) : g.PQ;
  const int64_t wstep = int64_t(g.NTP) * 64;

  f32x4 tot[CT_NTW];
#pragma unroll
  for (int t = 0; t < CT_NTW; ++t) tot[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int seg = seg0; seg < seg1; ++seg) {
    const int p = 4 * seg + fq < g.P ? 4 * seg + fq : g.P - 1;   // (a position past H W: any finite value, its weights are 0)
    const int y = p / g.W, x = p - y * g.W;
    const int base = y * g.kh + x;
    float patch[NP];
    if (KS) {
#pragma unroll
      for (int t = 0; t < NP; ++t) patch[t] = image(base + (t / (KS ? KS : 1)) * g.kh + t % (KS ? KS : 1));
    }
    f32x4 acc[CT_NTW];
#pragma unroll
    for (int t = 0; t < CT_NTW; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *wp = pk + g.off_w + int64_t(seg) * g.F * wstep + ct0 * 64 + lane;
    // filter f: its B fragments are in `bc`; those of filter f + 1 are loaded into `bn` first, so that they are in flight under
    // this filter's taps and MFMAs (the last filter re-reads its own: a load without a branch)
    auto step = [&](int f, float (&bc)[CT_NTW], float (&bn)[CT_NTW]) {
      if (f + 1 < g.F) wp += wstep;
#pragma unroll
      for (int t = 0; t < CT_NTW; ++t) bn[t] = wp[t * 64];
      float h = cst[f];
      if (KS) {
        const float *tp = taps + f * NP;
#pragma unroll
        for (int t = 0; t < NP; ++t) h = fmaf(tp[t], patch[t], h);
      } else {
        const float *tp = taps + int64_t(f) * ks2;
        for (int dy = 0; dy < g.ks; ++dy)
          for (int dx = 0; dx < g.ks; ++dx) h = fmaf(tp[dy * g.ks + dx], image(base + dy * g.kh + dx), h);
      }
      h = relu_keep_nan(h);
#pragma unroll
      for (int t = 0; t < CT_NTW; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(h, bc[t], acc[t], 0, 0, 0);
    };
    float b0[CT_NTW], b1[CT_NTW];
#pragma unroll
    for (int t = 0; t < CT_NTW; ++t) b0[t] = wp[t * 64];
    int f = 0;
    for (; f + 1 < g.F; f += 2) {
      step(f, b0, b1);
      step(f + 1, b1, b0);
    }
    if (f < g.F) step(f, b0, b1);
    // lane holds rows q0 + 4 fq + i (i = 0..3) of column (ct0 + t) 16 + fr
    if (SPLIT) {
#pragma unroll
      for (int t = 0; t < CT_NTW; ++t) {
        const int col = (ct0 + t) * 16 + fr;
        if (col >= g.O) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = q0 + 4 * fq + i;
          if (row < a.batch) ws[(int64_t(seg) * a.batch + row) * g.OP + col] = acc[t][i];
        }
      }
    } else {
#pragma unroll
      for (int t = 0; t < CT_NTW; ++t) tot[t] += acc[t];
    }
  }
  if (!SPLIT) {
#pragma unroll
    for (int t = 0; t < CT_NTW; ++t) {
      const int col = (ct0 + t) * 16 + fr;
      if (col >= g.O) continue;
      const float sc = pk[g.off_scale + col], sh = pk[g.off_shift + col];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = q0 + 4 * fq + i;
        if (row < a.batch) out[int64_t(row) * a.ldo + col] = trunk_epilogue(tot[t][i], sc, sh);
      }
    }
  }
}

// The split form's second launch: segment partials in ascending order, then the epilogue of the one-launch form
__global__ __launch_bounds__(256) void conve_fold_kernel(const float *__restrict__ ws, const float *__restrict__ pk,
                                                         float *__restrict__ out, int64_t ldo, int32_t batch, Geo g) {
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= int64_t(batch) * g.O) return;
  const int row = int(idx / g.O), col = int(idx - int64_t(row) * g.O);
  float total = 0.f;
  for (int seg = 0; seg < g.PQ; ++seg) total += ws[(int64_t(seg) * batch + row) * g.OP + col];
  out[int64_t(row) * ldo + col] = trunk_epilogue(total, pk[g.off_scale + col], pk[g.off_shift + col]);
}

template <int KS>
void launch_trunk(const TrunkArgs &a, const Plan &p, const float *pk, float *out, float *ws, hipStream_t s) {
  const dim3 block(CT_WAVES * 64);
  const unsigned gx = unsigned((p.tiles + CT_WAVES - 1) / CT_WAVES);
  if (p.nsplit)
    hipLaunchKernelGGL((conve_trunk_kernel<KS, true>), dim3(gx, unsigned(p.nsplit), unsigned(a.g.NCG)), block, 0, s, a, pk, out, ws);
  else
    hipLaunchKernelGGL((conve_trunk_kernel<KS, false>), dim3(gx, 1, unsigned(a.g.NCG)), block, 0, s, a, pk, out, ws);
}

}  // namespace

extern "C" size_t mgcn_conve_packed_bytes(int32_t k_w, int32_t k_h, int32_t kernel_size, int32_t num_filter, int32_t dim_out) {
  Geo g;
  return geo_make(k_w, k_h, kernel_size, num_filter, dim_out, g) == MGCN_OK ? size_t(g.floats) * sizeof(float) : 0;
}

extern "C" int mgcn_conve_pack(int32_t k_w, int32_t k_h, int32_t kernel_size, int32_t num_filter, int32_t dim_out,
                               const float *conv_w_dev, const float *conv_b_dev, const float *fc_w_dev, int64_t ldw,
                               const float *fc_b_dev, const float *bn0_mean_dev, const float *bn0_var_dev,
                               const float *bn0_gamma_dev, const float *bn0_beta_dev, float bn0_eps, const float *bn1_mean_dev,
                               const float *bn1_var_dev, const float *bn1_gamma_dev, const float *bn1_beta_dev, float bn1_eps,
                               const float *bn2_mean_dev, const float *bn2_var_dev, const float *bn2_gamma_dev,
                               const float *bn2_beta_dev, float bn2_eps, void *packed_dev, size_t packed_bytes, void *stream) {
  Geo g;
  const int rc = geo_make(k_w, k_h, kernel_size, num_filter, dim_out, g);
  MGCN_REQUIRE(rc != MGCN_EINVAL, "conve_pack: not a ConvE geometry (k_w %d, k_h %d, kernel %d, filters %d, O %d)", k_w, k_h,
               kernel_size, num_filter, dim_out);
  if (rc) return mgcn::fail(rc, "conve_pack: O = %d > %d or a pack past 2^31 floats", dim_out, CT_MAX_O);
  MGCN_REQUIRE(conv_w_dev && fc_w_dev && packed_dev, "conve_pack: null pointer");
  MGCN_REQUIRE(bn0_mean_dev && bn0_var_dev && bn1_mean_dev && bn1_var_dev && bn2_mean_dev && bn2_var_dev,
               "conve_pack: null running statistics");
  MGCN_REQUIRE(ldw >= int64_t(g.F) * g.P, "conve_pack: ldw %lld < F H W = %lld", (long long)ldw, (long long)(int64_t(g.F) * g.P));
  MGCN_REQUIRE(packed_bytes >= size_t(g.floats) * sizeof(float), "conve_pack: pack of %zu bytes, needs %zu", packed_bytes,
               size_t(g.floats) * sizeof(float));
  MGCN_REQUIRE(mgcn::aligned16(packed_dev), "conve_pack: the pack must be 16-byte aligned");
  PackArgs a = {};
  a.cw = conv_w_dev; a.cb = conv_b_dev; a.fw = fc_w_dev; a.fb = fc_b_dev; a.ldw = ldw;
  a.bn0 = BnPtrs{bn0_mean_dev, bn0_var_dev, bn0_gamma_dev, bn0_beta_dev, bn0_eps};
  a.bn1 = BnPtrs{bn1_mean_dev, bn1_var_dev, bn1_gamma_dev, bn1_beta_dev, bn1_eps};
  a.bn2 = BnPtrs{bn2_mean_dev, bn2_var_dev, bn2_gamma_dev, bn2_beta_dev, bn2_eps};
  a.out = static_cast<float *>(packed_dev);
  a.g = g;
  hipLaunchKernelGGL(conve_pack_kernel, dim3(unsigned((g.floats + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  MGCN_CHECK_LAUNCH("conve_pack_kernel");
  return MGCN_OK;
}

extern "C" size_t mgcn_conve_trunk_workspace(int32_t batch, int32_t k_w, int32_t k_h, int32_t kernel_size, int32_t num_filter,
                                             int32_t dim_out) {
  Geo g;
  if (batch < 0 || geo_make(k_w, k_h, kernel_size, num_filter, dim_out, g) != MGCN_OK) return 0;
  return plan_make(batch, g).ws_bytes;
}

extern "C" int mgcn_conve_trunk_fwd(int32_t batch, int32_t k_w, int32_t k_h, int32_t kernel_size, int32_t num_filter,
                                    int32_t dim_out, const float *ent_dev, int64_t lde, int64_t ent_rows,
                                    const int64_t *src_index_dev, const float *rel_dev, int64_t ldr, int64_t rel_rows,
                                    const int64_t *rel_index_dev, const void *packed_dev, float *out_dev, int64_t ldo,
                                    void *workspace_dev, size_t workspace_bytes, void *stream) {
  Geo g;
  const int rc = geo_make(k_w, k_h, kernel_size, num_filter, dim_out, g);
  MGCN_REQUIRE(rc != MGCN_EINVAL, "conve_trunk_fwd: not a ConvE geometry (k_w %d, k_h %d, kernel %d, filters %d, O %d)", k_w, k_h,
               kernel_size, num_filter, dim_out);
  if (rc) return mgcn::fail(rc, "conve_trunk_fwd: O = %d > %d or a pack past 2^31 floats", dim_out, CT_MAX_O);
  MGCN_REQUIRE(batch >= 0 && ent_rows >= 0 && rel_rows >= 0, "conve_trunk_fwd: negative size");
  MGCN_REQUIRE(ent_dev && rel_dev && packed_dev && out_dev, "conve_trunk_fwd: null pointer");
  MGCN_REQUIRE(lde >= g.O && ldr >= g.O && ldo >= g.O, "conve_trunk_fwd: leading dimension too small");
  MGCN_REQUIRE(mgcn::aligned16(packed_dev), "conve_trunk_fwd: the pack must be 16-byte aligned");
  const Plan p = plan_make(batch, g);
  MGCN_REQUIRE(workspace_bytes >= p.ws_bytes, "conve_trunk_fwd: workspace of %zu bytes, needs %zu", workspace_bytes, p.ws_bytes);
  MGCN_REQUIRE(p.ws_bytes == 0 || (workspace_dev && mgcn::aligned16(workspace_dev)),
               "conve_trunk_fwd: workspace null or not 16-byte aligned");
  if (batch == 0) return MGCN_OK;
  MGCN_REQUIRE(ent_rows >= 1 && rel_rows >= 1, "conve_trunk_fwd: empty table");
  MGCN_REQUIRE(src_index_dev || ent_rows >= batch, "conve_trunk_fwd: no src index and fewer than batch entity rows");
  MGCN_REQUIRE(rel_index_dev || rel_rows >= batch, "conve_trunk_fwd: no rel index and fewer than batch relation rows");

  TrunkArgs a = {};
  a.ent = ent_dev; a.rel = rel_dev; a.si = src_index_dev; a.ri = rel_index_dev;
  a.lde = lde; a.ldr = ldr; a.n_ent = ent_rows; a.n_rel = rel_rows; a.ldo = ldo;
  a.batch = batch; a.seg_per = p.seg_per;
  a.g = g;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float *pk = static_cast<const float *>(packed_dev);
  float *ws = static_cast<float *>(workspace_dev);
  switch (g.ks) {
    case 3: launch_trunk<3>(a, p, pk, out_dev, ws, s); break;
    case 5: launch_trunk<5>(a, p, pk, out_dev, ws, s); break;
    case 7: launch_trunk<7>(a, p, pk, out_dev, ws, s); break;
    default: launch_trunk<0>(a, p, pk, out_dev, ws, s); break;
  }
  MGCN_CHECK_LAUNCH("conve_trunk_kernel");
  if (p.nsplit) {
    const int64_t n = int64_t(batch) * g.O;
    hipLaunchKernelGGL(conve_fold_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, ws, pk, out_dev, ldo, batch, g);
    MGCN_CHECK_LAUNCH("conve_fold_kernel");
  }
  return MGCN_OK;
}
